"""GPU: the batched augmentation chain (csrc/augment_batch.hip, TrainTransform.batch) — bit-identical to the per-image
chain `tf(img, rng)` with the same consumption of both random streams, every batched stage against
oracle/augment_oracle.py (the warps against their per-image entry points) with inactive slices and guard bytes
untouched, one C-ABI call per stage per batch whatever the batch size, and the loaders that go through it."""
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import augment_oracle as A  # noqa: E402
from primia_amd._lib import call, query  # noqa: E402

GUARD = 64
SIZES = [(120, 100), (90, 140), (50, 60), (200, 160), (77, 131), (64, 64), (300, 210), (61, 240)]    # (50, 60) < R

STANDARD = dict(rotation=30, translate=0.0, scale=0.15, shear=10, clahe=True, albu_prob=0.75, individual_albu_probs=0.2,
                noise_std=0.05, noise_prob=0.5, randomgamma=True, randombrightness=True, blur=True, elastic=True,
                optical_distortion=True, grid_distortion=True, fog=True)      # configs/torch/pneumonia-resnet-pretrained.ini
FAST = dict(STANDARD, grid_shuffle=True, hsv=True, invert=True, cutout=True, shadow=True, sun_flare=True, solarize=True,
            equalize=True, grid_dropout=True)                                 # ...-fast.ini: every member on
GREY = dict(clahe=True)


def img_of(rng, H, W, C):
    base = rng.integers(0, 256, size=(H, W, C), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = (127 + 100 * np.sin(xx / 17.0) * np.cos(yy / 11.0)).astype(np.int64)[..., None]
    base = np.clip(ramp + (base.astype(np.int64) - 128) // 6, 0, 255).astype(np.uint8)
    base[: H // 5, : W // 4] = 250
    base[-H // 6:, -W // 3:] = 3
    return base


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def images(cuda, B, C, seed=0, sizes=SIZES):
    rng = np.random.default_rng(seed)
    return [dev(img_of(rng, *sizes[i % len(sizes)], C), cuda) for i in range(B)]


def transform(cuda, switches, S, R, C, seed=3):
    from primia_amd.augment import TrainTransform

    mean, std = torch.linspace(0.4, 0.5, C), torch.linspace(0.2, 0.3, C)
    return TrainTransform(SimpleNamespace(train_resolution=S, inference_resolution=R, **switches), mean, std, cuda, C, seed=seed)


def check_batch_equals_per_image(cuda, switches, S, R, C, B, augment, seed, sizes=SIZES):
    imgs = images(cuda, B, C, seed=B, sizes=sizes)
    tf_a, tf_b = transform(cuda, switches, S, R, C), transform(cuda, switches, S, R, C)
    rng_a, rng_b = random.Random(seed), random.Random(seed)
    got = tf_a.batch(imgs, rng_a, augment)
    want = torch.stack([tf_b(im, rng_b, augment) for im in imgs])
    assert got.shape == (B, C, S, S) and got.dtype == torch.float32
    assert torch.equal(got, want), (B, (got != want).float().mean().item())
    assert rng_a.getstate() == rng_b.getstate()
    assert torch.equal(tf_a.gen.get_state(), tf_b.gen.get_state())
    # a second batch through the same transform reuses its working memory
    got2 = tf_a.batch(imgs[::-1], rng_a, augment)
    want2 = torch.stack([tf_b(im, rng_b, augment) for im in imgs[::-1]])
    assert torch.equal(got2, want2) and torch.equal(tf_a.gen.get_state(), tf_b.gen.get_state())
    return tf_a


SEED64 = {"standard": 11, "fast": 11}


@pytest.mark.parametrize("name,switches,C,augment", [("standard", STANDARD, 3, True), ("fast", FAST, 3, True),
                                                     ("grey", GREY, 1, False)])
@pytest.mark.parametrize("B", [1, 7, 64])
def test_batch_is_bit_identical_to_the_per_image_chain(cuda, name, switches, C, augment, B):
    """The acceptance test: no tolerance (uint8 stages are exact, the final fp32 normalise is the same expression)."""
    seed = SEED64.get(name, 5)
    tf = check_batch_equals_per_image(cuda, switches, 64, 72, C, B, augment, seed)
    if B == 64 and augment:
        # every member of the configuration fired on some image and was skipped on another: asserted from the plans
        rng = random.Random(seed)
        plans = [tf.plan(*SIZES[i % len(SIZES)], rng) for i in range(B)]
        for key in tf.members() + ["affine"]:
            n = sum(bool(key in p) for p in plans)
            assert (0 < n < B) if key != "affine" else n == B, (key, n)


def test_batch_of_200_at_224_on_the_standard_preset(cuda):
    big = [(900, 700), (512, 640), (230, 1000), (150, 180), (1024, 1024)]        # (150, 180) < R = 224
    check_batch_equals_per_image(cuda, STANDARD, 224, 224, 3, 200, True, 7, sizes=big)


# ---- the stages through the C ABI ------------------------------------------------------------------------------------
class Slices:
    """n slices of `nbytes` in one device buffer with GUARD bytes either side, filled with a pattern."""

    def __init__(self, cuda, n, nbytes, fill):
        self.n, self.nbytes = n, nbytes
        self.buf = torch.full((2 * GUARD + n * nbytes,), fill, dtype=torch.uint8, device=cuda)
        self.before = None

    def ptr(self, i):
        return self.buf.data_ptr() + GUARD + i * self.nbytes

    def put(self, i, arr):
        self.buf[GUARD + i * self.nbytes:GUARD + (i + 1) * self.nbytes] = torch.from_numpy(
            np.ascontiguousarray(arr).reshape(-1).view(np.uint8)).to(self.buf.device)

    def get(self, i, dtype=np.uint8, shape=None):
        a = self.buf[GUARD + i * self.nbytes:GUARD + (i + 1) * self.nbytes].cpu().numpy().view(dtype)
        return a.reshape(shape) if shape else a

    def snapshot(self):
        self.before = self.buf.clone()

    def untouched_except(self, active):
        now, was = self.buf.cpu().numpy(), self.before.cpu().numpy()
        assert np.array_equal(now[:GUARD], was[:GUARD]) and np.array_equal(now[-GUARD:], was[-GUARD:]), "guard bytes"
        for i in range(self.n):
            if i not in active:
                lo = GUARD + i * self.nbytes
                assert np.array_equal(now[lo:lo + self.nbytes], was[lo:lo + self.nbytes]), ("inactive slice", i)


def table(cuda, rows, dtype):
    return dev(np.ascontiguousarray(np.array(rows, dtype=dtype)), cuda)


@pytest.mark.parametrize("C", [1, 3])
def test_fused_affine_resize_crop_matches_the_oracle(cuda, C):
    rng = np.random.default_rng(C)
    R, S = 80, 64
    sizes = [(90, 70), (57, 121), (60, 50), (200, 160), (128, 96)]
    draws = [None, (30, (0, 0), 1.15, 10), (45, (0, 0), 0.85, 0), (-17.5, (3, -2), 0.9, -7), (80, (0, 0), 0.7, 5)]
    offs = [(0, 0), (5, 9), (16, 16), (3, 0), (16, 2)]
    imgs = [img_of(rng, H, W, C) for H, W in sizes]
    imgs[2][:] = np.maximum(imgs[2], 40)                 # no zero of its own: zero fill in the crop is the rotation's
    d_imgs = [dev(im, cuda) for im in imgs]
    n_slices = 7
    out = Slices(cuda, n_slices, S * S * C, 0xAB)
    active = [5, 0, 3, 1, 6]                             # slices 2 and 4 take no image
    mats = [np.zeros(6) if d is None else A.inverse_affine_matrix((W * 0.5 + 0.5, H * 0.5 + 0.5), *d)
            for d, (H, W) in zip(draws, sizes)]
    ptrs = table(cuda, [(d_imgs[j].data_ptr(), out.ptr(s)) for j, s in enumerate(active)], np.int64)
    ip = table(cuda, [(H, W, int(draws[j] is not None), *offs[j]) for j, (H, W) in enumerate(sizes)], np.int32)
    fp = table(cuda, mats, np.float32)
    out.snapshot()
    call("primia_image_affine_resize_crop_batch_u8", ptrs, ip, fp, len(active), C, R, S)
    for j, s in enumerate(active):
        warped = imgs[j] if draws[j] is None else A.affine_nearest(imgs[j], mats[j])
        want = A.resize_crop(warped, R, offs[j][0], offs[j][1], S, False)
        assert np.array_equal(out.get(s, shape=(S, S, C)), want), j
    assert (out.get(active[2], shape=(S, S, C)) == 0).any()     # the 45 degree rotation brought zero fill into the crop
    out.untouched_except(active)


@pytest.mark.parametrize("S,C", [(64, 1), (96, 3)])
def test_batched_stages_match_the_oracle_on_the_active_subset(cuda, S, C):
    """Every batched stage on a batch of 6 slices of which a subset is active: the active images equal the oracle bit for
    bit (the warps: the per-image entry point on the same parameters), the other slices and the guard bytes are untouched."""
    from primia_amd.augment import TrainTransform, fog_params, grid_axis

    rng = np.random.default_rng(S + C)
    n, px = 6, S * S * C
    imgs = [img_of(rng, S, S, C) for _ in range(n)]
    per_image = TrainTransform(SimpleNamespace(train_resolution=S, inference_resolution=S), None, None, cuda, C)

    def fresh(active, in_place=False):
        src, dst = Slices(cuda, n, px, 0x11), Slices(cuda, n, px, 0xCD)
        for i in range(n):
            src.put(i, imgs[i])
        src.snapshot(), dst.snapshot()
        pairs = [(src.ptr(i), src.ptr(i) if in_place else dst.ptr(i)) for i in active]
        return src, dst, table(cuda, pairs, np.int64)

    def done(src, dst, active, in_place=False):
        src.untouched_except(active if in_place else [])
        dst.untouched_except([] if in_place else active)

    # CLAHE (grey: the oracle; colour: the per-image entry point, as tests/test_gpu_augment.py holds it), out of place and in place
    wsb = query("primia_clahe_workspace_bytes", S, S, C)
    for in_place in (False, True):
        active = [4, 1, 2]
        src, dst, ptrs = fresh(active, in_place)
        ws = Slices(cuda, 1, len(active) * wsb, 0)
        ws.snapshot()
        call("primia_clahe_batch_u8", ptrs, len(active), S, S, C, 1.0, ws.ptr(0), len(active) * wsb)
        for i in active:
            got = (src if in_place else dst).get(i, shape=(S, S, C))
            one = torch.empty(S, S, C, dtype=torch.uint8, device=cuda)
            call("primia_clahe_u8", dev(imgs[i], cuda), S, S, C, 1.0, per_image.ws, per_image.ws_bytes, one)
            assert np.array_equal(got, one.cpu().numpy())
            if C == 1:
                assert np.array_equal(got, A.clahe_plane(imgs[i][:, :, 0], 1.0)[:, :, None])
        done(src, dst, active, in_place)
        ws.untouched_except([0])
    # flip + table
    active = [0, 5, 3, 2]
    src, dst, ptrs = fresh(active)
    tables = np.stack([A.brightness_table(1.0, 0.2)[A.gamma_table(0.8)], A.gamma_table(1.2), A.invert_table()])
    ip = [(1, 0), (0, 1), (1, -1), (0, 2)]
    call("primia_image_flip_lut_batch_u8", ptrs, table(cuda, ip, np.int32), dev(tables, cuda), len(active), S, C)
    for (flip, ti), i in zip(ip, active):
        want = imgs[i][::-1] if flip else imgs[i]
        want = tables[ti][want] if ti >= 0 else want
        assert np.array_equal(dst.get(i, shape=(S, S, C)), want)
    assert np.array_equal(tables[0][imgs[0]], A.brightness_table(1.0, 0.2)[A.gamma_table(0.8)[imgs[0]]])     # composition
    done(src, dst, active)
    # box blur with a k per image (a.Blur's odd kernels, RandomFog's any)
    active, ks = [1, 3, 4, 5], [3, 7, 2, 6]
    src, dst, ptrs = fresh(active)
    call("primia_image_box_blur_batch_u8", ptrs, table(cuda, ks, np.int32), len(active), S, C)
    for k, i in zip(ks, active):
        assert np.array_equal(dst.get(i, shape=(S, S, C)), A.box_blur_anchor(imgs[i], k)), k
    done(src, dst, active)
    # fog: haze lists by offset + count into one list (one image without haze points)
    active = [2, 0, 5]
    src, dst, ptrs = fresh(active)
    params = [fog_params(S, S, random.Random(s_)) for s_ in (1, 2, 3)]
    hazes = [params[0][1] + [(5, 7), (30, 12), (-3, 40)], [], params[2][1] + [(S // 2, S // 3)]]
    hws = [max(int(S // 3 * fc), 10) for fc, _ in params]
    first = np.cumsum([0] + [len(h) for h in hazes[:-1]])
    ip = [(hws[j], first[j], len(hazes[j])) for j in range(3)]
    alphas = [np.float32(0.08 * fc) for fc, _ in params]
    call("primia_image_fog_batch_u8", ptrs, table(cuda, ip, np.int32), table(cuda, alphas, np.float32),
         table(cuda, [q for h in hazes for q in h], np.int32), 3, S, C)
    for j, i in enumerate(active):
        one = torch.empty(S, S, C, dtype=torch.uint8, device=cuda)
        hz = table(cuda, hazes[j], np.int32) if hazes[j] else None
        call("primia_image_fog_u8", dev(imgs[i], cuda), S, S, C, hz, len(hazes[j]), hws[j], float(alphas[j]), one)
        assert np.array_equal(dst.get(i, shape=(S, S, C)), one.cpu().numpy())
        if hws[j] // 10 <= 1:            # (A.add_fog = discs + blur: comparable directly where no blur follows)
            assert np.array_equal(dst.get(i, shape=(S, S, C)), A.add_fog(imgs[i], params[j][0], hazes[j]))
    done(src, dst, active)
    # fill rectangles in place (Cutout, GridDropout)
    active = [3, 4]
    src, dst, ptrs = fresh(active, in_place=True)
    holes = [A.cutout_holes(S, S, random.Random(4)), A.grid_dropout_holes(S, S)]
    ip = [(0, len(holes[0])), (len(holes[0]), len(holes[1]))]
    call("primia_image_fill_rects_batch_u8", table(cuda, [src.ptr(i) for i in active], np.int64), table(cuda, ip, np.int32),
         table(cuda, holes[0] + holes[1], np.int32), 2, S, C, 0)
    for h, i in zip(holes, active):
        assert np.array_equal(src.get(i, shape=(S, S, C)), A.fill_rects(imgs[i], h))
    done(src, dst, active, in_place=True)
    # noise in place: normal values scaled by the image's sigma
    active, sds = [5, 1, 0], [np.float32(0.03 * 255), np.float32(0.0), np.float32(7.5)]
    src, dst, ptrs = fresh(active, in_place=True)
    normal = rng.standard_normal((3, px)).astype(np.float32)
    call("primia_image_add_noise_batch_u8", table(cuda, [src.ptr(i) for i in active], np.int64), dev(normal, cuda),
         table(cuda, sds, np.float32), 3, px)
    for j, i in enumerate(active):
        want = A.add_noise(imgs[i], (normal[j] * sds[j]).astype(np.float32).reshape(imgs[i].shape))
        assert np.array_equal(src.get(i, shape=(S, S, C)), want)
    done(src, dst, active, in_place=True)
    # finish: uint8 HWC -> fp32 CHW slices of a [n, C, S, S] output
    active = [2, 5, 0]
    src, _, _ = fresh(active)
    out = Slices(cuda, n, px * 4, 0x7F)
    out.snapshot()
    mean, std = np.linspace(0.4, 0.5, C).astype(np.float32), np.linspace(0.2, 0.3, C).astype(np.float32)
    call("primia_image_finish_batch", table(cuda, [(src.ptr(i), out.ptr(i)) for i in active], np.int64), 3, S, C,
         dev(mean, cuda), dev(std, cuda))
    for i in active:
        assert np.array_equal(out.get(i, np.float32, (C, S, S)), A.finish(imgs[i], mean, std))
    out.untouched_except(active), src.untouched_except([])
    # the warps: affine, optical, grid axes, displacement planes — against primia_warp_map_* + primia_image_remap_u8
    active, kinds = [1, 4, 0, 3], [0, 1, 2, 3]
    src, dst, _ = fresh(active)
    inv = np.array([0.97, 0.05, 1.5, -0.04, 1.02, -2.25])
    opt = [float(np.float32(0.043)), float(S), float(S), S * 0.5 + 1, S * 0.5 + 0, (S - 1) * 0.5, (S - 1) * 0.5]
    r = random.Random(S)
    axes = np.stack([grid_axis(S, 5, [1 + r.uniform(-0.3, 0.3) for _ in range(6)]) for _ in range(2)]).astype(np.float32)
    dxy = rng.uniform(-3, 3, (2, S, S)).astype(np.float32)
    d_axes, d_dxy = dev(axes, cuda), dev(dxy, cuda)
    aux = [(0, 0), (0, 0), (d_axes[0].data_ptr(), d_axes[1].data_ptr()), (d_dxy[0].data_ptr(), d_dxy[1].data_ptr())]
    ptrs = table(cuda, [(src.ptr(i), dst.ptr(i), *aux[j]) for j, i in enumerate(active)], np.int64)
    dp = table(cuda, [list(inv) + [0.0], opt, [0.0] * 7, [0.0] * 7], np.float64)
    call("primia_image_warp_batch_u8", ptrs, table(cuda, kinds, np.int32), dp, 4, S, C)
    mx, my = per_image.map_x, per_image.map_y
    for j, i in enumerate(active):
        if j == 0:
            call("primia_warp_map_affine", S, S, *[float(v) for v in inv], mx, my)
        elif j == 1:
            call("primia_warp_map_optical", S, S, *opt, mx, my)
        elif j == 2:
            call("primia_warp_map_grid", S, S, d_axes[0], d_axes[1], mx, my)
        else:
            mx.copy_(d_dxy[0] + torch.arange(S, device=cuda, dtype=torch.float32)[None, :])
            my.copy_(d_dxy[1] + torch.arange(S, device=cuda, dtype=torch.float32)[:, None])
        one = torch.empty(S, S, C, dtype=torch.uint8, device=cuda)
        call("primia_image_remap_u8", dev(imgs[i], cuda), S, S, C, mx, my, one)
        assert np.array_equal(dst.get(i, shape=(S, S, C)), one.cpu().numpy()), j
        assert not np.array_equal(one.cpu().numpy(), imgs[i])
    done(src, dst, active)


@pytest.mark.parametrize("S", [64, 224])
def test_elastic_displacements_equal_the_per_image_maps(cuda, S):
    seeds = (1234, 9999)
    fields = np.stack([np.stack([rs.rand(S, S), rs.rand(S, S)]) for rs in (np.random.RandomState(s_) for s_ in seeds)])
    d_fields = dev(fields, cuda)
    n = len(seeds)
    wsb = query("primia_warp_elastic_disp_workspace_bytes", n, S, S, 50.0)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    disp = Slices(cuda, 1, n * 2 * S * S * 4, 0x55)
    disp.snapshot()
    call("primia_warp_elastic_disp_batch", d_fields, n, S, S, 50.0, 1.0, ws, wsb, disp.ptr(0))
    got = torch.from_numpy(disp.get(0, np.float32, (n, 2, S, S)).copy()).to(cuda)
    disp.untouched_except([0])
    ws1 = torch.empty(S * S * 16, dtype=torch.uint8, device=cuda)
    mx, my = torch.empty(S, S, device=cuda), torch.empty(S, S, device=cuda)
    col = torch.arange(S, device=cuda, dtype=torch.float32)
    for j in range(n):
        call("primia_warp_map_elastic", S, S, d_fields[j, 0], d_fields[j, 1], 50.0, 1.0, ws1, ws1.numel(), mx, my)
        assert torch.equal(col[None, :] + got[j, 0], mx) and torch.equal(col[:, None] + got[j, 1], my)
        assert got[j].abs().max() > 0


# ---- launch economy ----------------------------------------------------------------------------------------------------
def test_calls_and_uploads_per_batch_do_not_grow_with_the_batch(cuda, monkeypatch):
    import primia_amd.augment as P

    calls, uploads = [], []
    real_call, real_upload = P.call, P.TrainTransform._upload
    monkeypatch.setattr(P, "call", lambda name, *a, **k: (calls.append(name), real_call(name, *a, **k))[1])
    monkeypatch.setattr(P.TrainTransform, "_upload", lambda self, d, s: (uploads.append(d.numel()), real_upload(self, d, s))[1])
    tf = transform(cuda, STANDARD, 64, 72, 3)
    for B in (64, 8, 200):
        imgs = images(cuda, B, 3, seed=B)
        rng_plan = random.Random(B)
        plans = [tf.plan(im.shape[0], im.shape[1], rng_plan) for im in imgs]
        elastic = any("elastic" in p for p in plans)
        del calls[:], uploads[:]
        tf.batch(imgs, random.Random(B))
        # the count depends on which stages fired, never on B
        assert len(calls) <= len(P.TrainTransform.STAGES), (B, calls)
        assert all(name.endswith("_batch_u8") or name.endswith("_batch") for name in calls), calls
        assert len(uploads) <= 2 + (1 if elastic else 0), (B, uploads)
    imgs = images(cuda, 64, 3, seed=64)
    del calls[:]
    rng = random.Random(64)
    for im in imgs:
        tf(im, rng)
    assert len(calls) >= 3 * 64


# ---- the loaders ---------------------------------------------------------------------------------------------------------
def test_augmenting_loader_epoch_equals_the_per_image_epoch(cuda):
    from primia_amd.imagefolder import AugmentingLoader

    imgs = images(cuda, 23, 3, seed=23)
    targets = torch.arange(23, device=cuda) % 3
    tf_a, tf_b = transform(cuda, STANDARD, 64, 72, 3), transform(cuda, STANDARD, 64, 72, 3)
    loader = AugmentingLoader(imgs, targets, tf_a, random.Random(9), batch_size=5, seed=4)
    rng_b, gen = random.Random(9), torch.Generator().manual_seed(4)
    for _ in range(2):
        order = torch.randperm(23, generator=gen).tolist()
        batches = list(loader)
        assert len(batches) == 5 and batches[-1][0].shape[0] == 3           # the ragged last batch
        for b, (x, y) in enumerate(batches):
            idx = order[b * 5:(b + 1) * 5]
            assert torch.equal(x, torch.stack([tf_b(imgs[i], rng_b) for i in idx]))
            assert torch.equal(y, targets[torch.tensor(idx, device=cuda)])


def test_federated_registration_equals_the_per_image_construction(cuda, tmp_path, monkeypatch):
    from PIL import Image

    import primia_amd.imagefolder as F
    from primia_amd.augment import TrainTransform
    from primia_amd.datapipe import calc_mean_std

    rng = np.random.default_rng(2)
    for c in ("bacterial", "normal", "viral"):
        os.makedirs(tmp_path / c)
        for k in range(4):
            H, W = SIZES[(k + len(c)) % len(SIZES)]
            Image.fromarray(img_of(rng, H, W, 3)).save(tmp_path / c / "{:d}.png".format(k))
    args = SimpleNamespace(train_resolution=64, inference_resolution=72, batch_size=4, train_federated=True,
                           repetitions_dataset=2, mixup=False, weight_classes=False, **STANDARD)
    monkeypatch.setattr(F, "REGISTRATION_CHUNK", 5)              # 12 images: chunks of 5, 5, 2
    loader, (mean, std) = F.client_loader(str(tmp_path), args, cuda, 3, seed=6)
    # the per-image construction client_loader replaced
    _, samples = F.scan(str(tmp_path))
    r = random.Random(6)
    mean2, std2 = calc_mean_std(F.prepare(samples, args, cuda, 3, r))
    tf = TrainTransform(args, mean2, std2, cuda, 3, 6)
    imgs = [torch.from_numpy(np.ascontiguousarray(F.decode(fn, 3))).to(cuda) for fn, _ in samples]
    walks = [torch.stack([tf(im, r) for im in imgs]) for _ in range(2)]
    assert torch.equal(mean, mean2) and torch.equal(std, std2)
    assert loader.data.shape == (24, 3, 64, 64) and torch.equal(loader.data, torch.cat(walks))
