"""What the GPU tests of encrypted inference (tests/test_gpu_secure*.py) share: share comparison, seeded contexts, the oracle's
worker pool, guard words, runs of inference.py, and the launch of the three-role cases (tests/three_role_cases.py) with
their in-process reference.  A module of helpers, not of tests."""
import argparse
import contextlib
import ctypes
import json
import multiprocessing as mp
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import secure_oracle as S
from primia_amd.secure import (Dealer, SecureContext, SecureResNet18, architecture_of, fold_batch_norm, image_requests,
                               model_requests)
from tests.three_role_cases import CASES

I64 = torch.int64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A5A5A5A
# max |secure - float64 plaintext| of pf = 3 logits: the bound tests/test_gpu_secure_fullsize.py established for the 224 network
# (a maximum of 0.047 over 300 dealer draws, 99th percentile 0.030)
PLAIN_TOL = 0.05


def host(t):
    return t.cpu().numpy()


def shares_equal(gpu, ora):
    return all(np.array_equal(host(gpu[j]), ora[j]) for j in range(2))


def context(cuda, seed, pf, fused=True):
    """(dealer, context) under a debug seed, the dealer logging for an oracle replay; fused=False: the step-by-step chain."""
    dealer = Dealer(cuda, seed=seed)
    dealer.log = []
    ctx = SecureContext(dealer, 10, pf)
    ctx.local_fused = fused
    ctx.fuse_newton = fused
    return dealer, ctx


@contextlib.contextmanager
def time_limit(seconds):
    """A test's own time limit: SIGALRM raises in the main thread (a pool.map of the oracle's fan-out wakes up for it)."""
    def expired(signum, frame):
        raise TimeoutError(f"test exceeded its own limit of {seconds} s")

    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def oracle_pool():
    """Worker processes for the oracle's FSS fan-out, the way the reference fans out above MULTI_LIMIT (mpc/fss.py:43-44,
    214-266): the CPUs this process may run on (not the host's count), capped by OMP_NUM_THREADS when it is set, with the
    reference's floor of 4.  Spawned (fresh interpreters, numpy only), never forked: this process holds a HIP context.  Each
    worker evaluates whole elements of a slice, so the size changes no bit of a result.  (A test module imports the
    fixture by name.)"""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 8
    omp = os.environ.get("OMP_NUM_THREADS", "").strip()
    if omp.isdigit() and int(omp) > 0:
        n = min(n, int(omp))
    n = max(4, min(64, n))
    with mp.get_context("spawn").Pool(n) as pool:
        S.use_pool(pool, n_slices=2 * n)
        yield pool
        S.use_pool(None)


def wrapping_shares(rng, shape):
    """Uniform int64 with every fifth value within 16 of +-2^63 (the two extremes among them): window sums wrap, and
    truncation meets the most negative value."""
    x = rng.integers(-2 ** 63, 2 ** 63 - 1, size=shape, dtype=np.int64, endpoint=True)
    flat = x.reshape(-1)
    near = rng.integers(0, 16, size=flat[::5].size, dtype=np.int64)
    flat[::5] = np.where(rng.integers(0, 2, size=near.size) == 1, np.int64(2 ** 63 - 1) - near, np.int64(-2 ** 63) + near)
    flat[0], flat[-1] = np.int64(-2 ** 63), np.int64(2 ** 63 - 1)
    return x


def guarded(n, cuda):
    buf = torch.full((n + 128,), GUARD, dtype=I64, device=cuda)
    return buf, buf[64:64 + n]


def guards_intact(buf, n):
    return bool((buf[:64] == GUARD).all()) and bool((buf[64 + n:] == GUARD).all())


def six(t):
    """The six tensors of a Beaver triple's two halves, party 0's first."""
    return (t[0][0], t[0][1], t[0][2], t[1][0], t[1][1], t[1][2])


def host_ptrs(t):
    return (ctypes.c_void_p * 6)(*[q.data_ptr() for q in six(t)])


def padded(chunk, batch):
    """A ragged last pass filled up with all-zero images."""
    pad = batch - len(chunk)
    return torch.cat([chunk, torch.zeros_like(chunk[:1]).expand(pad, -1, -1, -1)]) if pad else chunk


def chunks(images, labels, batch):
    return [(images[i:i + batch], labels[i:i + batch]) for i in range(0, len(images), batch)]


# ---- inference.py on a 32 x 32 checkpoint -----------------------------------------------------------------------------------
def write_checkpoint(path, sd, pooling="max", encrypted_inference=False):
    """`sd` as train.py saves it, with the pickled arguments inference.py reads; returns the path as a string."""
    args = argparse.Namespace(train_resolution=32, inference_resolution=32, clahe=False, pooling_type=pooling,
                              encrypted_inference=encrypted_inference)
    torch.save({"model_state_dict": sd, "args": args}, str(path))
    return str(path)


def run_inference(ckpt, num_images, pf, extra=(), batch_size=None, dump=None):
    """inference.py on `synthetic` under debug dealer seed 7, its own time limit 600 s; PRIMIA_DUMP_LOGITS is `dump` or unset.
    Returns the CompletedProcess: the caller checks the exit status."""
    cmd = [sys.executable, "inference.py", "--model_weights", ckpt, "--data_dir", "synthetic", "--num_images", str(num_images),
           "--cuda", "--debug_dealer_seed", "7", "--precision_fractional", str(pf)]
    if batch_size is not None:
        cmd += ["--batch_size", str(batch_size)]
    env = {k: v for k, v in os.environ.items() if k != "PRIMIA_DUMP_LOGITS"}
    if dump is not None:
        env["PRIMIA_DUMP_LOGITS"] = dump
    return subprocess.run(cmd + list(extra), cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def json_line(r):
    """The JSON object on the last line a successful inference.py run printed."""
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


# ---- three roles ----------------------------------------------------------------------------------------------------------
def in_process_logits(cuda, case, pf, seed):
    """A logits-form three-role case in ONE process under the same debug seed: the logits both parties must end up with.  What
    its dealer was asked for is held to the host-side schedule the dealer rank will follow -- model_requests once,
    image_requests per pass -- so a schedule mismatch fails here, as an assertion, and not as a stall between three processes."""
    c = CASES[case]
    assert c.reveal == "logits"
    sd, images = c.tensors()
    if c.fold:
        sd = fold_batch_norm(sd)
    dealer = Dealer(cuda, seed=seed, fss_bits=c.fss_bits)
    dealer.requests = []
    model = SecureResNet18(SecureContext(dealer, 10, pf), sd, input_size=c.size, blocks=c.blocks, pooling=c.pooling)
    dv, rows = images.to(cuda), []
    for i in range(0, len(dv), c.batch):
        chunk = dv[i:i + c.batch]
        rows.append(model(padded(chunk, c.batch))[:len(chunk)])
    assert [tuple(r.shape) for r in rows] == c.shapes
    arch = architecture_of(sd)
    assert dealer.requests == model_requests(arch) + len(rows) * image_requests(arch, c.size, c.batch, c.blocks, pooling=c.pooling)
    return torch.cat(rows).cpu()


ROLE_LIMIT = 240      # seconds, each role's own
_role_failures = []      # what failed first in this pytest session: after it no three-role test starts a process


def run_roles(commands, out, limit=ROLE_LIMIT, failures=_role_failures, what="three roles"):
    """One process per command -- rank r runs commands[r] with RANK, LOCAL_RANK, WORLD_SIZE, MASTER_ADDR and MASTER_PORT set,
    under `timeout -k 10 <limit>` of its own, writing to `out`.log<r>.  The processes are polled; when one exits with a
    non-zero status its peers, which would wait for it, are terminated.  Returns [(rank, exit status, log)] when every
    status is zero; otherwise the assertion names the first role that failed and carries rank, status and log tail of every
    role that did not exit with 0, and `failures` keeps it: while `failures` holds anything, nothing is started."""
    from tests.conftest import free_port

    assert not failures, f"an earlier three-role run failed ({failures[0]}): no further processes are started"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE=str(len(commands)))
    logs = [open(f"{out}.log{r}", "w+") for r in range(len(commands))]
    procs = [subprocess.Popen(["timeout", "-k", "10", str(limit)] + list(cmd), cwd=ROOT,
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=logs[r], stderr=subprocess.STDOUT)
             for r, cmd in enumerate(commands)]
    first = []
    while any(p.poll() is None for p in procs):
        for p in procs:
            try:
                p.wait(timeout=0.25)
            except subprocess.TimeoutExpired:
                pass
        first = first or [(r, p.poll()) for r, p in enumerate(procs) if p.poll() not in (None, 0)]
        if first:      # its peers wait for a role that is gone: end them
            for q in procs:
                if q.poll() is None:
                    q.terminate()      # (`timeout` hands the signal on to the role's process, and kills it 10 s later)
                    q.wait()
    results = []
    for r, (p, log) in enumerate(zip(procs, logs)):
        log.seek(0)
        results.append((r, p.returncode, log.read()))
        log.close()
    bad = [(r, rc, text[-3000:]) for r, rc, text in results if rc != 0]
    if bad:
        r, rc = first[0] if first else bad[0][:2]
        failures.append(f"{what}: rank {r} exited with {rc}")
    assert not bad, (failures[-1], bad)
    return results


def three_roles(case, pf, seed, out):
    """model_owner / data_owner / crypto_provider as three processes on one GPU over gloo (tests/party_worker.py, run_roles):
    each role that holds a result leaves it in `out`.<role>."""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "party_worker.py"), out, case, str(pf), str(seed)]
    run_roles([cmd] * 3, out, what=case)


def three_role_logits(case, pf, seed, tmp_path):
    """The decoded logits of party 0 and party 1 of a logits-form case."""
    out = str(tmp_path / "logits")
    three_roles(case, pf, seed, out)
    return [torch.load(f"{out}.{j}") for j in range(2)]
