"""What the GPU tests of encrypted inference (tests/test_gpu_secure*.py) and their three-role worker (tests/party_worker.py)
share: share comparison, seeded contexts, the oracle's worker pool, guard words, and the three-role cases with their launch.
A module of helpers, not of tests."""
import contextlib
import multiprocessing as mp
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import secure_oracle as S
from primia_amd.secure import (Dealer, SecureContext, SecureResNet18, architecture_of, image_requests,
                               model_requests)
from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet
from tests.secure_groupnorm_nets import group_mini

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


# ---- three roles ----------------------------------------------------------------------------------------------------------
# name -> (network, seed of the generator that draws it and then the images, images, input size, images per protocol pass,
#          stem pool, shapes of the logits each party holds per pass): three images at two per pass pad the second pass
THREE_ROLE_CASES = {
    "mini": (mini_resnet, 21, 2, 16, 1, "max", [(1, 3), (1, 3)]),
    "batch": (mini_resnet, 61, 3, 32, 2, "max", [(2, 3), (1, 3)]),
    "avg": (mini_resnet, 61, 3, 32, 2, "avg", [(2, 3), (1, 3)]),
    "group": (group_mini, 71, 3, 32, 2, "max", [(2, 3), (1, 3)]),
}


def three_role_case(case):
    """(state dict, images, blocks, input size, batch, pooling) of a three-role test, identical in every process."""
    net, seed, n, size, batch, pooling, _ = THREE_ROLE_CASES[case]
    gen = torch.Generator().manual_seed(seed)
    sd = net(gen)
    return sd, torch.randn(n, 3, size, size, generator=gen), MINI_BLOCKS, size, batch, pooling


def in_process_logits(cuda, case, pf, seed):
    """The three-role case in ONE process under the same debug seed: the logits both parties must end up with.  What its
    dealer was asked for is held to the host-side schedule the dealer rank will follow -- model_requests once, image_requests
    per pass -- so a schedule mismatch fails here, as an assertion, and not as a stall between three processes."""
    sd, images, blocks, size, batch, pooling = three_role_case(case)
    dealer = Dealer(cuda, seed=seed)
    dealer.requests = []
    model = SecureResNet18(SecureContext(dealer, 10, pf), sd, input_size=size, blocks=blocks, pooling=pooling)
    dv, rows = images.to(cuda), []
    for i in range(0, len(dv), batch):
        chunk = dv[i:i + batch]
        pad = batch - len(chunk)
        rows.append(model(torch.cat([chunk, torch.zeros_like(dv[:pad])]) if pad else chunk)[:len(chunk)])
    arch = architecture_of(sd)
    assert dealer.requests == model_requests(arch) + len(rows) * image_requests(arch, size, batch, blocks, pooling)
    return torch.cat(rows).cpu()


def three_role_logits(case, pf, seed, tmp_path):
    """model_owner / data_owner / crypto_provider as three processes on one GPU over gloo (tests/party_worker.py under
    torch.distributed.run): the decoded logits of party 0 and party 1."""
    from tests.conftest import free_port

    out = str(tmp_path / "logits")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "tests", "party_worker.py"),
           out, case, str(pf), str(seed)]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, MASTER_ADDR="127.0.0.1"), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return [torch.load(f"{out}.{j}") for j in range(2)]
