"""The training-time transform chain of the reference, create_albu_transform (torchlib/dataloader.py:138-217), with the
image arithmetic on the GPU (csrc/augment.hip) and the random PARAMETERS drawn on the host:

    transforms.RandomAffine(rotation, (translate, translate), (1 - scale, 1 + scale), shear)      [PIL image]
    a.Resize(R, R) -> a.RandomCrop(S, S) [-> a.FromFloat -> a.CLAHE(always_apply, clip_limit (1, 1))]
    a.Compose([a.VerticalFlip, a.RandomGamma, a.RandomBrightness, a.Blur, ..., a.GaussNoise], p = albu_prob)
    a.ToFloat(255) -> a.Normalize(mean, std, 1.0)

Built: every member of create_albu_transform — RandomAffine, Resize, RandomCrop, CLAHE, VerticalFlip, RandomGamma,
RandomBrightness, Blur, ElasticTransform, OpticalDistortion, GridDistortion, RandomGridShuffle, HueSaturationValue,
InvertImg, Cutout, RandomShadow, RandomFog, RandomSunFlare, Solarize, Equalize, GridDropout, GaussNoise, ToFloat,
Normalize — so both shipped presets (configs/torch/pneumonia-resnet-pretrained.ini and ...-fast.ini, which switches every
one of them on) run as written.  `UNBUILT` is empty; `check(args)` stays as the place a future gap would be refused.

The three warping transforms are `cv2.remap` with a generated coordinate field (albumentations 0.4.6, the release the
reference pins: functional.py elastic_transform / optical_distortion / grid_distortion): the host draws their few
parameters (ElasticTransform: a seed for numpy's RandomState; the per-image path draws its two uniform fields on the host
and copies them, the batch path generates the same stream on the device, primia_mt19937_fields_batch), the maps are formed
and sampled on the GPU (primia_warp_map_*, primia_image_remap_u8).

Draw order (Python's `random`, as torchvision's RandomAffine.get_params and albumentations' BasicTransform.__call__ use
it): affine angle, [translate x, y], scale, shear; crop h, w; Compose coin; then per enabled transform its own coin and,
if it fires, its parameters.  GaussNoise's per-pixel normal values come from torch's generator on the device
(albumentations uses NumPy's RandomState, whose stream cannot be reproduced here).  cv2 / albumentations / Pillow are
not in this image: the chain follows their published behaviour and is unpinned against their binaries.

Draw and apply are separate.  `draw_plan` (TrainTransform.plan) makes all draws of one image in the order above — none
depends on pixel values — and returns them as a plan.  `TrainTransform.__call__` applies a plan to ONE image with the
per-image entry points (4 to 15 calls and as many small uploads).  `TrainTransform.batch` plans image 0, image 1, ... (the
`random` stream is consumed exactly as that many `__call__`s consume it), packs every parameter of the batch into one
table (`pack_plans`; the batch's one host-to-device copy) and applies the
chain stage by stage: one C-ABI call per stage (TrainTransform.STAGES) covers every image on which the stage fired
(csrc/augment_batch.hip, the same per-pixel functions as the per-image kernels: csrc/augment_px.h).  GaussNoise's values
are requested from torch's generator with the same calls in the same image order.  The tensors equal the per-image chain's
bit for bit; the loaders of primia_amd.imagefolder go through `batch`.
"""
import math
import os
from warnings import warn

import numpy as np
import torch

from ._lib import call, query

UNBUILT = ()


def unsupported(args):
    return [k for k in UNBUILT if getattr(args, k, False)]


def check(args):
    """Refuse a configuration whose augmentations cannot be honoured (or, on request, say what is dropped)."""
    bad = unsupported(args)
    if not bad or not getattr(args, "albu_prob", 0) or not getattr(args, "individual_albu_probs", 0):
        return
    msg = ("the albumentations transforms {:s} are not part of the accelerated data path".format(", ".join(bad)))
    if os.environ.get("PRIMIA_SKIP_UNSUPPORTED_AUG") == "1":
        warn(msg + ": training WITHOUT them (PRIMIA_SKIP_UNSUPPORTED_AUG=1)")
    else:
        raise SystemExit(msg + "; switch them off in the [albumentations] section, or set PRIMIA_SKIP_UNSUPPORTED_AUG=1 "
                               "to train without them")


def inverse_affine_matrix(center, angle, translate, scale, shear):
    """torchvision 0.5 `_get_inverse_affine_matrix` (one shear angle, degrees): output pixel -> source pixel."""
    angle, shear = math.radians(angle), math.radians(shear)
    scale = 1.0 / scale
    d = math.cos(angle + shear) * math.cos(angle) + math.sin(angle + shear) * math.sin(angle)
    m = [math.cos(angle + shear), math.sin(angle + shear), 0, -math.sin(angle), math.cos(angle), 0]
    m = [scale / d * v for v in m]
    m[2] += m[0] * (-center[0] - translate[0]) + m[1] * (-center[1] - translate[1])
    m[5] += m[3] * (-center[0] - translate[0]) + m[4] * (-center[1] - translate[1])
    m[2] += center[0]
    m[5] += center[1]
    return m


def gamma_table(gamma):
    return (np.power(np.arange(0, 256.0 / 255, 1.0 / 255)[:256], gamma) * 255).astype(np.uint8)


def brightness_table(alpha, beta):
    lut = np.arange(0, 256, dtype=np.float32)
    if alpha != 1:
        lut *= np.float32(alpha)
    if beta != 0:
        lut += np.float32(beta * 255.0)
    return np.clip(lut, 0, 255).astype(np.uint8)


def affine_from_points(pts1, pts2):
    """cv2.getAffineTransform: the 2 x 3 float64 matrix mapping the three points pts1 onto pts2."""
    a = np.zeros((6, 6), np.float64)
    b = np.zeros(6, np.float64)
    for i in range(3):
        x, y = float(pts1[i][0]), float(pts1[i][1])
        a[2 * i] = [x, y, 1, 0, 0, 0]
        a[2 * i + 1] = [0, 0, 0, x, y, 1]
        b[2 * i], b[2 * i + 1] = float(pts2[i][0]), float(pts2[i][1])
    return np.linalg.solve(a, b).reshape(2, 3)


def invert_affine(m):
    """cv2.invertAffineTransform (warpAffine samples the source through the inverse)."""
    d = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22, a12, a21 = m[1, 1] * d, m[0, 0] * d, -m[0, 1] * d, -m[1, 0] * d
    return np.array([[a11, a12, -a11 * m[0, 2] - a12 * m[1, 2]], [a21, a22, -a21 * m[0, 2] - a22 * m[1, 2]]], np.float64)


def grid_axis(n, num_steps, steps):
    """One axis of albumentations' F.grid_distortion: float32 source positions of n pixels."""
    step = n // num_steps
    xx = np.zeros(n, np.float32)
    prev = 0
    for idx, x in enumerate(range(0, n, step)):
        start, end = x, x + step
        if end > n:
            end, cur = n, n
        else:
            cur = prev + step * steps[idx]
        xx[start:end] = np.linspace(prev, cur, end - start)
        prev = cur
    return xx


def fog_params(H, W, rng, fog_coef_lower=0.3, fog_coef_upper=1.0):
    """RandomFog.get_params_dependent_on_targets: fog_coef and the haze points, from Python's `random` stream."""
    fog_coef = rng.uniform(fog_coef_lower, fog_coef_upper)
    hw = max(1, int(W // 3 * fog_coef))
    haze = []
    midx, midy = W // 2 - 2 * hw, H // 2 - hw
    index = 1
    while midx > -hw or midy > -hw:
        for _ in range(hw // 10 * index):
            haze.append((rng.randint(midx, W - midx - hw), rng.randint(midy, H - midy - hw)))
        midx -= 3 * hw * W // (H + W)
        midy -= 3 * hw * H // (H + W)
        index += 1
    return fog_coef, haze


def cutout_holes(H, W, rng, num_holes=5, max_h_size=80, max_w_size=80):
    """a.Cutout.get_params_dependent_on_targets (dataloader.py:178-182: 5 holes of at most 80 x 80)."""
    holes = []
    for _ in range(num_holes):
        y, x = rng.randint(0, H), rng.randint(0, W)
        y1 = min(max(y - max_h_size // 2, 0), H)
        y2 = min(max(y1 + max_h_size, 0), H)
        x1 = min(max(x - max_w_size // 2, 0), W)
        x2 = min(max(x1 + max_w_size, 0), W)
        holes.append((x1, y1, x2, y2))
    return holes


def grid_dropout_holes(H, W, ratio=0.5):
    """a.GridDropout with its defaults: unit = max(2, W // 10), holes of ratio x unit at the unit grid's corners."""
    unit_w = max(2, W // 10)
    unit_h = max(min(unit_w, H), 2)
    hole_w = min(max(int(unit_w * ratio), 1), unit_w - 1)
    hole_h = min(max(int(unit_h * ratio), 1), unit_h - 1)
    holes = []
    for i in range(W // unit_w + 1):
        for j in range(H // unit_h + 1):
            x1, y1 = min(unit_w * i, W), min(unit_h * j, H)
            holes.append((x1, y1, min(x1 + hole_w, W), min(y1 + hole_h, H)))
    return holes


def grid_shuffle_tiles(H, W, seed, grid=(3, 3)):
    """a.RandomGridShuffle.get_params_dependent_on_targets: tiles of equal shape are permuted among themselves by
    np.random.RandomState(seed); rows (y, x, old_y, old_x, height, width)."""
    n, m = grid
    rs = np.random.RandomState(seed)
    hs = np.linspace(0, H, n + 1, dtype=np.int64)
    ws = np.linspace(0, W, m + 1, dtype=np.int64)
    hm, wm = np.meshgrid(hs, ws, indexing="ij")
    ih, iw = hm[:-1, :-1], wm[:-1, :-1]
    sizes = np.stack((hm[1:, 1:] - ih, wm[1:, 1:] - iw), axis=2)
    new_index = np.stack(np.indices((n, m)), axis=2)
    for size in np.unique(sizes.reshape(-1, 2), axis=0):
        eq = np.all(sizes == size, axis=2)
        new_index[eq] = rs.permutation(new_index[eq])
    a, b = new_index[..., 0], new_index[..., 1]
    return np.stack([ih.reshape(-1), iw.reshape(-1), ih[a, b].reshape(-1), iw[a, b].reshape(-1),
                     sizes[..., 0].reshape(-1), sizes[..., 1].reshape(-1)], axis=1).astype(np.int32)


def hsv_tables(hue_shift, sat_shift, val_shift):
    """F._shift_hsv_uint8's three cv2.LUT tables (hue mod 180; saturation and value clipped)."""
    i = np.arange(256, dtype=np.int16)
    return np.stack([np.mod(i + hue_shift, 180).astype(np.uint8), np.clip(i + sat_shift, 0, 255).astype(np.uint8),
                     np.clip(i + val_shift, 0, 255).astype(np.uint8)])


def solarize_table(threshold):
    i = np.arange(256)
    return np.where(i < threshold, i, 255 - i).astype(np.uint8)


def shadow_vertices(H, W, rng, shadow_roi=(0, 0.5, 1, 1), lower=1, upper=2, dimension=5):
    """a.RandomShadow.get_params_dependent_on_targets: [num_shadows][5][(x, y)] in the lower half of the image."""
    n = rng.randint(lower, upper)
    x_min, y_min, x_max, y_max = shadow_roi
    x_min, x_max, y_min, y_max = int(x_min * W), int(x_max * W), int(y_min * H), int(y_max * H)
    return np.array([[(rng.randint(x_min, x_max), rng.randint(y_min, y_max)) for _ in range(dimension)] for _ in range(n)],
                    np.int32)


def sun_flare_steps(H, W, rng, flare_roi=(0, 0, 1, 0.5), angle_lower=0.0, angle_upper=1.0, circles_lower=6,
                    circles_upper=10, src_radius=400, src_color=(255, 255, 255)):
    """a.RandomSunFlare.get_params_dependent_on_targets + the drawing schedule of F.add_sun_flare: rows
    (x, y, radius, r, g, b), their blend weights, and the step at which the overlay restarts from the output."""
    angle = 2 * math.pi * rng.uniform(angle_lower, angle_upper)
    lx, ly, ux, uy = flare_roi
    cx, cy = rng.uniform(lx, ux), rng.uniform(ly, uy)
    cx, cy = int(W * cx), int(H * cy)
    num = rng.randint(circles_lower, circles_upper)
    xs, ys = [], []
    for rx in range(0, W, 10):
        xs.append(rx)
        ys.append(2 * cy - (math.tan(angle) * (rx - cx) + cy))
    geo, alpha = [], []
    for _ in range(num):
        a = rng.uniform(0.05, 0.2)
        r = rng.randint(0, len(xs) - 1)
        rad = rng.randint(1, max(H // 100 - 2, 2))
        col = tuple(rng.randint(max(c - 50, 0), c) for c in src_color)
        geo.append((int(xs[r]), int(ys[r]), rad ** 3, *col))
        alpha.append(a)
    n_first = len(geo)
    num_times = src_radius // 10
    al = np.linspace(0.0, 1, num=num_times)
    rad = np.linspace(1, src_radius, num=num_times)
    for i in range(num_times):
        geo.append((cx, cy, int(rad[i]), *src_color))
        alpha.append(al[num_times - i - 1] ** 3)
    geo = np.clip(np.array(geo, np.int64), -2 ** 30, 2 ** 30).astype(np.int32).reshape(-1, 6)
    return geo, np.array(alpha, np.float64), n_first


def transform_config(args):
    """The keys of `args` the chain reads (keys a hand-built `args` may lack count as switched off, like an INI with every
    probability at zero)."""
    from types import SimpleNamespace

    keys = dict(rotation=0.0, translate=0.0, scale=0.0, shear=0.0, albu_prob=0.0, individual_albu_probs=0.0,
                noise_std=0.0, noise_prob=0.0, clahe=False, randomgamma=False, randombrightness=False, blur=False,
                elastic=False, optical_distortion=False, grid_distortion=False, fog=False, grid_shuffle=False, hsv=False,
                invert=False, cutout=False, shadow=False, sun_flare=False, solarize=False, equalize=False,
                grid_dropout=False)
    return SimpleNamespace(inference_resolution=args.inference_resolution, train_resolution=args.train_resolution,
                           **{k: getattr(args, k, v) for k, v in keys.items()})


def draw_plan(cfg, H, W, rng, augment=True):
    """Everything the chain draws for one decoded image of H x W pixels, in the draw order of the module docstring (no draw
    depends on pixel values, so all of them can be made before any pixel is touched): {stage: parameters} for the stages
    that fired, plus H, W and the crop offsets.  THE one source of the draw order: `TrainTransform.__call__` applies a
    plan image by image, `TrainTransform.batch` applies many stage by stage.  `cfg`: transform_config(args)."""
    a = cfg
    R, S = a.inference_resolution, a.train_resolution
    p = {"H": int(H), "W": int(W)}
    if augment and (a.rotation or a.translate or a.scale or a.shear):
        # RandomAffine.get_params (torchvision 0.5): angle, translations (rounded pixels), scale, shear
        angle = rng.uniform(-a.rotation, a.rotation)
        max_dx, max_dy = a.translate * W, a.translate * H
        tr = (np.round(rng.uniform(-max_dx, max_dx)), np.round(rng.uniform(-max_dy, max_dy)))
        sc = rng.uniform(1.0 - a.scale, 1.0 + a.scale)
        sh = rng.uniform(-a.shear, a.shear)
        # (float32: what the kernels take the inverse matrix as)
        p["affine"] = np.array(inverse_affine_matrix((W * 0.5 + 0.5, H * 0.5 + 0.5), angle, tr, sc, sh), np.float32)
    p["oy"], p["ox"] = int((R - S) * rng.random()), int((R - S) * rng.random())     # a.RandomCrop
    if augment and rng.random() < a.albu_prob:                                     # a.Compose(train_tf_albu, p)
        q = a.individual_albu_probs
        if rng.random() < q:                                                       # a.VerticalFlip
            p["flip"] = True
        table = None
        if a.randomgamma and rng.random() < q:                  # gamma_limit (80, 120)
            table = gamma_table(rng.randint(80, 120) / 100.0)
        if a.randombrightness and rng.random() < q:             # limit 0.2, contrast fixed at 1
            alpha = 1.0 + rng.uniform(0.0, 0.0)
            beta = 0.0 + rng.uniform(-0.2, 0.2)
            t2 = brightness_table(alpha, beta)
            table = t2 if table is None else t2[table]          # two consecutive cv2.LUTs compose exactly on uint8
        if table is not None:
            p["lut"] = np.ascontiguousarray(table, dtype=np.uint8)
        if a.blur and rng.random() < q:                         # blur_limit 7
            p["blur"] = rng.choice(list(range(3, 8, 2)))
        if a.elastic and rng.random() < q:                      # get_params: random.randint(0, 10000)
            p["elastic"] = rng.randint(0, 10000)
        if a.optical_distortion and rng.random() < q:           # distort_limit 0.05, shift_limit 0.05
            k = rng.uniform(-0.05, 0.05)
            dx, dy = round(rng.uniform(-0.05, 0.05)), round(rng.uniform(-0.05, 0.05))
            p["optical"] = (float(np.float32(k)), int(dx), int(dy))         # (k as the map kernel takes it)
        if a.grid_distortion and rng.random() < q:              # num_steps 5, distort_limit 0.3
            xsteps = [1 + rng.uniform(-0.3, 0.3) for _ in range(6)]
            ysteps = [1 + rng.uniform(-0.3, 0.3) for _ in range(6)]
            p["grid"] = (xsteps, ysteps)
        if a.grid_shuffle and rng.random() < q:                 # grid (3, 3); get_params: random.randint(0, 10000)
            p["grid_shuffle"] = rng.randint(0, 10000)
        if a.hsv and rng.random() < q:                          # hue 20, saturation 30, value 20
            p["hsv"] = (rng.uniform(-20, 20), rng.uniform(-30, 30), rng.uniform(-20, 20))
        if a.invert and rng.random() < q:
            p["invert"] = True
        if a.cutout and rng.random() < q:                       # num_holes 5, 80 x 80 (dataloader.py:178-182)
            p["cutout"] = cutout_holes(S, S, rng)
        if a.shadow and rng.random() < q:
            p["shadow"] = shadow_vertices(S, S, rng)
        if a.fog and rng.random() < q:                          # fog_coef (0.3, 1), alpha_coef 0.08
            p["fog"] = fog_params(S, S, rng)
        if a.sun_flare and rng.random() < q:
            p["sun_flare"] = sun_flare_steps(S, S, rng)
        if a.solarize and rng.random() < q:                     # threshold (128, 128): the draw is still made
            p["solarize"] = solarize_table(rng.uniform(128, 128))
        if a.equalize and rng.random() < q:
            p["equalize"] = True
        if a.grid_dropout and rng.random() < q:
            p["grid_dropout"] = True
        if rng.random() < a.noise_prob:                                            # a.GaussNoise(var_limit = noise_std^2)
            p["noise"] = rng.uniform(0.0, a.noise_std ** 2)
    return p


INVERT_TABLE = (255 - np.arange(256)).astype(np.uint8)


def elastic_affine(S, seed, alpha_affine=50.0):
    """F.elastic_transform's first draws from np.random.RandomState(seed): the INVERSE 2 x 3 matrix of its random affine,
    and the RandomState positioned where the two uniform displacement fields come next."""
    rs = np.random.RandomState(seed)
    center_square = np.float32((S, S)) // 2
    square_size = min((S, S)) // 3
    pts1 = np.float32([center_square + square_size, [center_square[0] + square_size, center_square[1] - square_size],
                       center_square - square_size])
    pts2 = pts1 + rs.uniform(-alpha_affine, alpha_affine, size=pts1.shape).astype(np.float32)
    return invert_affine(affine_from_points(pts1, pts2)), rs


class PackedTable:
    """The parameters of one batch as ONE byte string: named arrays at 16-byte aligned offsets (`layout[name]` = (offset,
    dtype, shape)).  What crosses to the device in `TrainTransform.batch`'s single parameter copy; pointer columns that
    refer to the table itself are stored relative and rebased by `write`."""

    def __init__(self):
        self.layout, self.arrays, self.relative, self.size = {}, {}, [], 0

    def add(self, name, array, dtype, shape=None):
        arr = np.ascontiguousarray(array, dtype=dtype)
        if shape is not None:
            arr = arr.reshape(shape)
        self.layout[name] = (self.size, np.dtype(dtype).str, arr.shape)
        self.arrays[name] = arr
        self.size += (arr.nbytes + 15) // 16 * 16
        return arr

    def view(self, name):
        return self.arrays[name]

    def offset(self, name, row=0):
        off, dtype, shape = self.layout[name]
        return off + row * np.dtype(dtype).itemsize * int(np.prod(shape[1:], dtype=np.int64))

    def write(self, buf, table_address=0):
        """Lay the arrays out in `buf` (uint8, >= size bytes) for a table that will live at `table_address`."""
        for name, cols in self.relative:
            self.arrays[name][:, cols] += table_address
        self.relative = []
        for name, (off, _, _) in self.layout.items():
            arr = self.arrays[name]
            buf[off:off + arr.nbytes] = arr.reshape(-1).view(np.uint8)
        return buf


def pack_plans(plans, S, C, clahe=False, addr=None):
    """The plans of a batch (TrainTransform.plan) -> PackedTable: per stage the indices of the images on which it fired
    (`<stage>.idx`), its parameters as the kernels of csrc/augment_batch.hip read them, and its pointer records.  An image
    moves between slice i of two ping-pong buffers; which one holds it after each stage is decided here.  `addr`: device
    addresses (src: one per image; buf: the two buffers; out, disp, noise); omitted, the pointers are offsets from zero."""
    B, px = len(plans), S * S * C
    addr = addr or dict(src=[0] * B, buf=(0, 0), out=0, disp=0, noise=0)
    t = PackedTable()
    side = [0] * B                                   # which buffer holds image i

    def here(i):
        return addr["buf"][side[i]] + i * px

    def move(i):                                     # (src, dst) of an out-of-place stage
        s = here(i)
        side[i] ^= 1
        return s, here(i)

    def fired(key):
        return [i for i, p in enumerate(plans) if p.get(key) is not None and p.get(key) is not False]

    t.add("arc.ptrs", [(addr["src"][i], here(i)) for i in range(B)], np.int64, (B, 2))
    t.add("arc.ip", [(p["H"], p["W"], int("affine" in p), p["oy"], p["ox"]) for p in plans], np.int32, (B, 5))
    t.add("arc.fp", [p["affine"] if "affine" in p else np.zeros(6, np.float32) for p in plans], np.float32, (B, 6))
    if clahe:
        t.add("clahe.ptrs", [(here(i), here(i)) for i in range(B)], np.int64, (B, 2))
    idx = [i for i, p in enumerate(plans) if p.get("flip") or "lut" in p]
    if idx:
        with_lut = [i for i in idx if "lut" in plans[i]]
        t.add("fl.idx", idx, np.int32)
        t.add("fl.ptrs", [move(i) for i in idx], np.int64, (len(idx), 2))
        t.add("fl.ip", [(int(bool(plans[i].get("flip"))), with_lut.index(i) if i in with_lut else -1) for i in idx], np.int32,
              (len(idx), 2))
        t.add("fl.luts", [plans[i]["lut"] for i in with_lut] or np.zeros((1, 256)), np.uint8, (max(len(with_lut), 1), 256))
    idx = fired("blur")
    if idx:
        t.add("blur.idx", idx, np.int32)
        t.add("blur.ptrs", [move(i) for i in idx], np.int64, (len(idx), 2))
        t.add("blur.k", [plans[i]["blur"] for i in idx], np.int32)
    idx = fired("elastic")
    if idx:
        n = len(idx)
        t.add("el.idx", idx, np.int32)
        t.add("el.seed", [plans[i]["elastic"] for i in idx], np.int32)
        t.add("ela.ptrs", [move(i) + (0, 0) for i in idx], np.int64, (n, 4))
        t.add("ela.kind", np.zeros(n), np.int32)
        t.add("ela.dp", [list(elastic_affine(S, plans[i]["elastic"])[0].reshape(-1)) + [0.0] for i in idx], np.float64, (n, 7))
        plane = S * S * 4
        t.add("elw.ptrs", [move(i) + (addr["disp"] + 2 * j * plane, addr["disp"] + (2 * j + 1) * plane)
                           for j, i in enumerate(idx)], np.int64, (n, 4))
        t.add("elw.kind", np.full(n, 3), np.int32)
    idx = fired("optical")
    if idx:
        n = len(idx)
        t.add("opt.idx", idx, np.int32)
        t.add("opt.ptrs", [move(i) + (0, 0) for i in idx], np.int64, (n, 4))
        t.add("opt.kind", np.ones(n), np.int32)
        t.add("opt.dp", [(k, float(S), float(S), S * 0.5 + dx, S * 0.5 + dy, (S - 1) * 0.5, (S - 1) * 0.5)
                         for k, dx, dy in (plans[i]["optical"] for i in idx)], np.float64, (n, 7))
    idx = fired("grid")
    if idx:
        n = len(idx)
        t.add("grid.idx", idx, np.int32)
        t.add("grid.steps", [list(plans[i]["grid"][0]) + list(plans[i]["grid"][1]) for i in idx], np.float64, (n, 12))
        t.add("grid.axes", [(grid_axis(S, 5, plans[i]["grid"][0]), grid_axis(S, 5, plans[i]["grid"][1])) for i in idx],
              np.float32, (n, 2, S))
        axes = t.offset("grid.axes")
        t.add("grid.ptrs", [move(i) + (axes + 2 * j * S * 4, axes + (2 * j + 1) * S * 4) for j, i in enumerate(idx)], np.int64,
              (n, 4))
        t.relative.append(("grid.ptrs", [2, 3]))
        t.add("grid.kind", np.full(n, 2), np.int32)
    idx = fired("grid_shuffle")
    if idx:
        t.add("gs.idx", idx, np.int32)
        t.add("gs.seed", [plans[i]["grid_shuffle"] for i in idx], np.int32)
        t.add("gs.tiles", [grid_shuffle_tiles(S, S, plans[i]["grid_shuffle"]) for i in idx], np.int32, (len(idx), 9, 6))
        t.add("gs.ptrs", [move(i) for i in idx], np.int64, (len(idx), 2))
    idx = fired("hsv")
    if idx:
        t.add("hsv.idx", idx, np.int32)
        t.add("hsv.raw", [plans[i]["hsv"] for i in idx], np.float64, (len(idx), 3))
        t.add("hsv.luts", [hsv_tables(*plans[i]["hsv"]) for i in idx], np.uint8, (len(idx), 3, 256))
        t.add("hsv.ptrs", [move(i) for i in idx], np.int64, (len(idx), 2))
    idx = fired("invert")
    if idx:
        t.add("inv.idx", idx, np.int32)
        t.add("inv.ptrs", [move(i) for i in idx], np.int64, (len(idx), 2))
        t.add("inv.ip", [(0, 0)] * len(idx), np.int32, (len(idx), 2))
        t.add("inv.luts", INVERT_TABLE, np.uint8, (1, 256))
    for key, tag in (("cutout", "cut"),):
        idx = fired(key)
        if idx:
            t.add(tag + ".idx", idx, np.int32)
            t.add(tag + ".ptrs", [here(i) for i in idx], np.int64)
            t.add(tag + ".ip", [(5 * j, 5) for j in range(len(idx))], np.int32, (len(idx), 2))
            t.add(tag + ".rects", [plans[i]["cutout"] for i in idx], np.int32, (5 * len(idx), 4))
    idx = fired("shadow")
    if idx:
        counts = [len(plans[i]["shadow"]) for i in idx]
        first = np.cumsum([0] + counts[:-1])
        t.add("sh.idx", idx, np.int32)
        t.add("sh.cnt", list(zip(first, counts)), np.int32, (len(idx), 2))
        t.add("sh.verts", np.concatenate([plans[i]["shadow"] for i in idx]), np.int32, (sum(counts), 5, 2))
        t.add("sh.ptrs", [move(i) for i in idx], np.int64, (len(idx), 2))
    idx = fired("fog")
    if idx:
        n = len(idx)
        coef = [plans[i]["fog"][0] for i in idx]
        haze = [plans[i]["fog"][1] for i in idx]
        hw = [max(int(S // 3 * c), 10) for c in coef]
        first = np.cumsum([0] + [len(h) for h in haze[:-1]])
        t.add("fog.idx", idx, np.int32)
        t.add("fog.coef", coef, np.float64)
        t.add("fog.ptrs", [move(i) for i in idx], np.int64, (n, 2))
        t.add("fog.ip", [(hw[j], first[j], len(haze[j])) for j in range(n)], np.int32, (n, 3))
        t.add("fog.alpha", [np.float32(0.08 * c) for c in coef], np.float32)
        pts = [q for h in haze for q in h]
        t.add("fog.haze", pts or [(0, 0)], np.int32, (max(len(pts), 1), 2))
        blur = [j for j in range(n) if hw[j] // 10 > 1]              # cv2.blur(hw // 10) follows where it is more than 1 x 1
        if blur:
            t.add("fogb.ptrs", [move(idx[j]) for j in blur], np.int64, (len(blur), 2))
            t.add("fogb.k", [hw[j] // 10 for j in blur], np.int32)
    idx = fired("sun_flare")
    if idx:
        geo = [plans[i]["sun_flare"][0] for i in idx]
        alpha = [plans[i]["sun_flare"][1] for i in idx]
        first = np.cumsum([0] + [len(g) for g in geo[:-1]])
        t.add("sf.idx", idx, np.int32)
        t.add("sf.cnt", [(first[j], len(geo[j]), plans[i]["sun_flare"][2]) for j, i in enumerate(idx)], np.int32, (len(idx), 3))
        t.add("sf.geo", np.concatenate(geo), np.int32, (-1, 6))
        t.add("sf.alpha", np.concatenate(alpha), np.float64)
        t.add("sf.a32", np.concatenate([al.astype(np.float32) for al in alpha]), np.float32)
        t.add("sf.b32", np.concatenate([(1.0 - al).astype(np.float32) for al in alpha]), np.float32)
        t.add("sf.ptrs", [move(i) for i in idx], np.int64, (len(idx), 2))
    idx = fired("solarize")
    if idx:
        t.add("sol.idx", idx, np.int32)
        t.add("sol.ptrs", [move(i) for i in idx], np.int64, (len(idx), 2))
        t.add("sol.ip", [(0, j) for j in range(len(idx))], np.int32, (len(idx), 2))
        t.add("sol.luts", [plans[i]["solarize"] for i in idx], np.uint8, (len(idx), 256))
    idx = fired("equalize")
    if idx:
        t.add("eq.idx", idx, np.int32)
        t.add("eq.ptrs", [move(i) for i in idx], np.int64, (len(idx), 2))
    idx = fired("grid_dropout")
    if idx:
        holes = grid_dropout_holes(S, S)
        t.add("gd.idx", idx, np.int32)
        t.add("gd.ptrs", [here(i) for i in idx], np.int64)
        t.add("gd.ip", [(0, len(holes))] * len(idx), np.int32, (len(idx), 2))
        t.add("gd.rects", holes, np.int32, (len(holes), 4))
    idx = fired("noise")
    if idx:
        t.add("noise.idx", idx, np.int32)
        t.add("noise.var", [plans[i]["noise"] for i in idx], np.float64)
        t.add("noise.ptrs", [here(i) for i in idx], np.int64)
        t.add("noise.sd", [np.float32(plans[i]["noise"] ** 0.5) for i in idx], np.float32)
    t.add("fin.ptrs", [(here(i), addr["out"] + i * px * 4) for i in range(B)], np.int64, (B, 2))
    return t


def unpack_plans(buf, layout):
    """The inverse of pack_plans on the table's bytes: the list of plans it was packed from."""
    def get(name):
        off, dtype, shape = layout[name]
        n = int(np.prod(shape, dtype=np.int64))
        return np.frombuffer(bytes(buf[off:off + n * np.dtype(dtype).itemsize]), dtype=dtype).reshape(shape)

    def rows(tag):
        return enumerate(get(tag + ".idx").tolist()) if tag + ".idx" in layout else ()

    ip, fp = get("arc.ip"), get("arc.fp")
    plans = []
    for i in range(ip.shape[0]):
        p = {"H": int(ip[i, 0]), "W": int(ip[i, 1]), "oy": int(ip[i, 3]), "ox": int(ip[i, 4])}
        if ip[i, 2]:
            p["affine"] = fp[i].copy()
        plans.append(p)
    for j, i in rows("fl"):
        flip, ti = get("fl.ip")[j]
        if flip:
            plans[i]["flip"] = True
        if ti >= 0:
            plans[i]["lut"] = get("fl.luts")[ti].copy()
    for j, i in rows("blur"):
        plans[i]["blur"] = int(get("blur.k")[j])
    for j, i in rows("el"):
        plans[i]["elastic"] = int(get("el.seed")[j])
    for j, i in rows("opt"):
        d = get("opt.dp")[j]
        S = d[1]
        plans[i]["optical"] = (float(d[0]), int(d[3] - S * 0.5), int(d[4] - S * 0.5))
    for j, i in rows("grid"):
        s = get("grid.steps")[j].tolist()
        plans[i]["grid"] = (s[:6], s[6:])
    for j, i in rows("gs"):
        plans[i]["grid_shuffle"] = int(get("gs.seed")[j])
    for j, i in rows("hsv"):
        plans[i]["hsv"] = tuple(get("hsv.raw")[j].tolist())
    for j, i in rows("inv"):
        plans[i]["invert"] = True
    for j, i in rows("cut"):
        first, count = get("cut.ip")[j]
        plans[i]["cutout"] = [tuple(r) for r in get("cut.rects")[first:first + count].tolist()]
    for j, i in rows("sh"):
        first, count = get("sh.cnt")[j]
        plans[i]["shadow"] = get("sh.verts")[first:first + count].copy()
    for j, i in rows("fog"):
        _, first, count = get("fog.ip")[j]
        plans[i]["fog"] = (float(get("fog.coef")[j]), [tuple(q) for q in get("fog.haze")[first:first + count].tolist()])
    for j, i in rows("sf"):
        first, count, n_first = get("sf.cnt")[j]
        plans[i]["sun_flare"] = (get("sf.geo")[first:first + count].copy(), get("sf.alpha")[first:first + count].copy(),
                                 int(n_first))
    for j, i in rows("sol"):
        plans[i]["solarize"] = get("sol.luts")[j].copy()
    for j, i in rows("eq"):
        plans[i]["equalize"] = True
    for j, i in rows("gd"):
        plans[i]["grid_dropout"] = True
    for j, i in rows("noise"):
        plans[i]["noise"] = float(get("noise.var")[j])
    return plans


def plans_equal(a, b):
    """Two plans hold the same stages with the same parameters (arrays by value and dtype)."""
    def same(x, y):
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            return isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and x.dtype == y.dtype and np.array_equal(x, y)
        if isinstance(x, (tuple, list)):
            return type(x) is type(y) and len(x) == len(y) and all(same(u, v) for u, v in zip(x, y))
        return type(x) is type(y) and x == y
    return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)


class TrainTransform:
    """create_albu_transform(args, mean, std) for device-resident uint8 HWC images: `tf(img, rng) -> fp32 [C, S, S]` for one
    image, `tf.batch(images, rng) -> fp32 [B, C, S, S]` for a list of them (the same tensors, one launch per stage)."""

    # the stage kinds of `batch`, in chain order: each is at most ONE C-ABI call per batch (the five members that only the
    # -fast preset switches on — grid_shuffle, hsv, shadow, sun_flare, equalize — go image by image instead)
    STAGES = ("affine_resize_crop", "clahe", "flip_lut", "blur", "elastic_fields", "elastic_affine", "elastic_displacements",
              "elastic_warp", "optical", "grid", "grid_shuffle", "hsv", "invert", "cutout", "shadow", "fog", "fog_blur",
              "sun_flare", "solarize", "equalize", "grid_dropout", "noise", "finish")
    # plan key of every member that fires on its own coin -> the configuration switches that enable it
    MEMBERS = {"flip": (), "lut": ("randomgamma", "randombrightness"), "blur": ("blur",), "elastic": ("elastic",),
               "optical": ("optical_distortion",), "grid": ("grid_distortion",), "grid_shuffle": ("grid_shuffle",),
               "hsv": ("hsv",), "invert": ("invert",), "cutout": ("cutout",), "shadow": ("shadow",), "fog": ("fog",),
               "sun_flare": ("sun_flare",), "solarize": ("solarize",), "equalize": ("equalize",),
               "grid_dropout": ("grid_dropout",), "noise": ()}

    def members(self):
        """The plan keys this configuration can fire."""
        return [k for k, sw in self.MEMBERS.items() if not sw or any(getattr(self.cfg, s) for s in sw)]

    def __init__(self, args, mean, std, device, channels, seed=0):
        check(args)
        self.cfg = transform_config(args)
        self.device, self.C = torch.device(device), channels
        self.mean = None if mean is None else mean.to(device).float().reshape(-1).contiguous()
        self.std = None if std is None else std.to(device).float().reshape(-1).contiguous()
        self.gen = torch.Generator(device=self.device).manual_seed(seed)          # GaussNoise values
        S = args.train_resolution
        self.ws_bytes = query("primia_clahe_workspace_bytes", S, S, channels)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)
        # coordinate maps and the elastic workspace (float64 plane + two float32 planes), built once
        self.map_x = torch.empty(S, S, dtype=torch.float32, device=self.device)
        self.map_y = torch.empty(S, S, dtype=torch.float32, device=self.device)
        self.warp_ws = torch.empty(S * S * 16, dtype=torch.uint8, device=self.device)
        for key, name in (("shadow", "RandomShadows"), ("fog", "RandomFog"), ("sun_flare", "RandomSunFlare")):
            if getattr(self.cfg, key) and channels != 3:
                raise AssertionError(name + " needs 3 channels")          # torchlib/dataloader.py:184-191
        if self.cfg.hsv and channels != 3:
            raise AssertionError("HueSaturationValue needs 3 channels")   # (albumentations raises for grayscale input)
        self.eq_ws = torch.empty(3 * 256 * 5, dtype=torch.uint8, device=self.device)
        self._bufs, self._uploaded = {}, None            # `batch`'s working memory and the event behind its last upload

    def _remap(self, cur):
        out = torch.empty_like(cur)
        S = cur.shape[0]
        call("primia_image_remap_u8", cur, S, S, self.C, self.map_x, self.map_y, out)
        return out

    def elastic(self, cur, seed, alpha=1.0, sigma=50.0, alpha_affine=50.0):
        """a.ElasticTransform().apply(img, random_state=seed) (F.elastic_transform, approximate=False)."""
        S, dev = cur.shape[0], self.device
        inv, rs = elastic_affine(S, seed, alpha_affine)
        call("primia_warp_map_affine", S, S, *[float(v) for v in inv.reshape(-1)], self.map_x, self.map_y)
        cur = self._remap(cur)
        fx = torch.from_numpy(rs.rand(S, S)).to(dev)
        fy = torch.from_numpy(rs.rand(S, S)).to(dev)
        call("primia_warp_map_elastic", S, S, fx, fy, float(sigma), float(alpha), self.warp_ws, self.warp_ws.numel(),
             self.map_x, self.map_y)
        return self._remap(cur)

    def optical(self, cur, k, dx, dy):
        """F.optical_distortion (albumentations 0.4.6: fx = fy = width)."""
        S = cur.shape[0]
        call("primia_warp_map_optical", S, S, float(np.float32(k)), float(S), float(S), S * 0.5 + dx, S * 0.5 + dy,
             (S - 1) * 0.5, (S - 1) * 0.5, self.map_x, self.map_y)
        return self._remap(cur)

    def grid(self, cur, xsteps, ysteps, num_steps=5):
        """F.grid_distortion: piecewise-linear axes (host, a few hundred values), meshgrid + remap on the device."""
        S, dev = cur.shape[0], self.device
        xx = torch.from_numpy(grid_axis(S, num_steps, xsteps)).to(dev)
        yy = torch.from_numpy(grid_axis(S, num_steps, ysteps)).to(dev)
        call("primia_warp_map_grid", S, S, xx, yy, self.map_x, self.map_y)
        return self._remap(cur)

    def fog(self, cur, fog_coef, haze_list, alpha_coef=0.08):
        """F.add_fog: haze discs blended in list order, then cv2.blur(hw // 10)."""
        S, dev = cur.shape[0], self.device
        hw = max(int(S // 3 * fog_coef), 10)
        hz = torch.tensor(haze_list, dtype=torch.int32).reshape(-1, 2).contiguous().to(dev)
        out = torch.empty_like(cur)
        call("primia_image_fog_u8", cur, S, S, self.C, hz if len(haze_list) else None, len(haze_list), hw,
             float(np.float32(alpha_coef * fog_coef)), out)
        k = hw // 10
        if k <= 1:
            return out
        blurred = torch.empty_like(out)
        call("primia_image_box_blur_u8", out, S, S, self.C, k, blurred)
        return blurred

    def _i32(self, rows):
        return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(self.device)

    def grid_shuffle(self, cur, seed):
        S = cur.shape[0]
        tiles = grid_shuffle_tiles(S, S, seed)
        out = torch.empty_like(cur)
        call("primia_image_swap_tiles_u8", cur, S, S, self.C, self._i32(tiles), len(tiles), out)
        return out

    def hsv_shift(self, cur, hue_shift, sat_shift, val_shift):
        S = cur.shape[0]
        luts = torch.from_numpy(hsv_tables(hue_shift, sat_shift, val_shift)).to(self.device)
        out = torch.empty_like(cur)
        call("primia_image_hsv_shift_u8", cur, S, S, luts, out)
        return out

    def lut(self, cur, table):
        call("primia_image_lut_u8", cur, cur.numel(), torch.from_numpy(table).to(self.device), cur)
        return cur

    def fill_rects(self, cur, holes, fill=0):
        S = cur.shape[0]
        call("primia_image_fill_rects_u8", cur, S, S, self.C, self._i32(holes), len(holes), int(fill))
        return cur

    def shadow(self, cur, vertices):
        S = cur.shape[0]
        out = torch.empty_like(cur)
        call("primia_image_shadow_u8", cur, S, S, self._i32(vertices), vertices.shape[0], vertices.shape[1], out)
        return out

    def sun_flare(self, cur, geo, alpha, n_first):
        S = cur.shape[0]
        a32 = torch.from_numpy(alpha.astype(np.float32)).to(self.device)
        b32 = torch.from_numpy((1.0 - alpha).astype(np.float32)).to(self.device)
        out = torch.empty_like(cur)
        call("primia_image_sun_flare_u8", cur, S, S, self._i32(geo), a32, b32, len(geo), n_first, out)
        return out

    def equalize(self, cur):
        S = cur.shape[0]
        out = torch.empty_like(cur)
        call("primia_image_equalize_u8", cur, S, S, self.C, self.eq_ws, self.eq_ws.numel(), out)
        return out

    # ---- the draws ---------------------------------------------------------------------------------------------------
    def plan(self, H, W, rng, augment=True):
        """draw_plan for this transform's configuration: what `__call__` draws for one image of H x W pixels."""
        return draw_plan(self.cfg, H, W, rng, augment)

    # ---- one image: a launch per stage -----------------------------------------------------------------------------
    def apply(self, img, p):
        """The chain on ONE device uint8 HWC image with the draws of plan `p`: per-image entry points, 4 to 15 calls."""
        dev, C = self.device, self.C
        a = self.cfg
        R, S = a.inference_resolution, a.train_resolution
        H, W = img.shape[0], img.shape[1]
        if "affine" in p:
            warped = torch.empty_like(img)
            call("primia_image_affine_u8", img, H, W, C, *[float(v) for v in p["affine"]], warped)
            img = warped
        cur = torch.empty(S, S, C, dtype=torch.uint8, device=dev)
        call("primia_image_resize_crop_u8", img, H, W, C, R, p["oy"], p["ox"], S, 0, cur)
        if a.clahe:
            call("primia_clahe_u8", cur, S, S, C, 1.0, self.ws, self.ws_bytes, cur)        # clip_limit = (1, 1)
        if p.get("flip"):
            cur = torch.flip(cur, dims=[0]).contiguous()
        if "lut" in p:                                              # RandomGamma and / or RandomBrightness
            call("primia_image_lut_u8", cur, cur.numel(), torch.from_numpy(p["lut"]).to(dev), cur)
        if "blur" in p:
            out = torch.empty_like(cur)
            call("primia_image_box_blur_u8", cur, S, S, C, p["blur"], out)
            cur = out
        if "elastic" in p:
            cur = self.elastic(cur, p["elastic"])
        if "optical" in p:
            cur = self.optical(cur, *p["optical"])
        if "grid" in p:
            cur = self.grid(cur, *p["grid"])
        if "grid_shuffle" in p:
            cur = self.grid_shuffle(cur, p["grid_shuffle"])
        if "hsv" in p:
            cur = self.hsv_shift(cur, *p["hsv"])
        if p.get("invert"):
            cur = self.lut(cur, INVERT_TABLE)
        if "cutout" in p:
            cur = self.fill_rects(cur, p["cutout"])
        if "shadow" in p:
            cur = self.shadow(cur, p["shadow"])
        if "fog" in p:
            cur = self.fog(cur, *p["fog"])
        if "sun_flare" in p:
            cur = self.sun_flare(cur, *p["sun_flare"])
        if "solarize" in p:
            cur = self.lut(cur, p["solarize"])
        if p.get("equalize"):
            cur = self.equalize(cur)
        if p.get("grid_dropout"):
            cur = self.fill_rects(cur, grid_dropout_holes(S, S))
        if "noise" in p:
            noise = torch.randn(cur.numel(), generator=self.gen, device=dev) * (p["noise"] ** 0.5)
            call("primia_image_add_noise_u8", cur, noise, cur.numel(), cur)
        out = torch.empty(C, S, S, dtype=torch.float32, device=dev)
        call("primia_image_finish", cur, S, C, self.mean, self.std, out)
        return out

    def __call__(self, img, rng, augment=True):
        return self.apply(img, self.plan(img.shape[0], img.shape[1], rng, augment))

    # ---- a batch: a launch per stage ---------------------------------------------------------------------------------
    def _upload(self, dst, src):
        """THE host-to-device copy of `batch`: the parameter table."""
        dst.copy_(src, non_blocking=True)

    def _grow(self, name, nbytes, pinned=False):
        """The named reusable buffer (uint8), at least nbytes long: allocated once, regrown only for a larger batch."""
        buf = self._bufs.get(name)
        if buf is None or buf.numel() < nbytes:
            nbytes = max(int(nbytes), 256)
            if pinned:
                if self._uploaded is not None:          # the previous batch's copies read the old host buffer
                    self._uploaded.synchronize()
                buf = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            else:
                buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._bufs[name] = buf
        return buf

    def batch(self, images, rng, augment=True):
        """`torch.stack([self(img, rng, augment) for img in images])`, bit for bit and with the same consumption of `rng`
        and of the device generator, for a list of device uint8 HWC images of any sizes: all draws first (image 0, image 1,
        ...), one packed parameter table to the device, then the chain stage by stage — ONE C-ABI call per stage covers
        every image on which the stage fired (csrc/augment_batch.hip).  -> fp32 [B, C, S, S]."""
        plans = [self.plan(im.shape[0], im.shape[1], rng, augment) for im in images]
        return self.apply_batch(images, plans)

    def apply_batch(self, images, plans):
        dev, C = self.device, self.C
        a = self.cfg
        R, S = a.inference_resolution, a.train_resolution
        B, px = len(images), S * S * C
        out = torch.empty(B, C, S, S, dtype=torch.float32, device=dev)
        if B == 0:
            return out
        for im in images:
            assert im.dtype == torch.uint8 and im.is_contiguous() and im.dim() == 3 and im.shape[2] == C
        n_el = sum("elastic" in p for p in plans)
        n_noise = sum("noise" in p for p in plans)
        # working memory, once per TrainTransform: two [B, S, S, C] buffers to ping-pong between, the CLAHE workspace per
        # image, elastic's fields / displacements / Gaussian workspace and the noise planes per firing image
        pong = self._grow("pong", 2 * B * px)
        half = pong.numel() // 2
        disp = self._grow("disp", n_el * 2 * S * S * 4)
        noise = self._grow("noise", n_noise * px * 4)
        addr = dict(src=[im.data_ptr() for im in images], buf=(pong.data_ptr(), pong.data_ptr() + half), out=out.data_ptr(),
                    disp=disp.data_ptr(), noise=noise.data_ptr())
        if self._uploaded is not None:
            self._uploaded.synchronize()                # the previous batch's table has left the host buffer
        tab = pack_plans(plans, S, C, bool(a.clahe), addr)
        host = self._grow("table_host", tab.size, pinned=True)        # one reusable host buffer, one copy
        table = self._grow("table", tab.size)
        tab.write(host.numpy(), table.data_ptr())
        self._upload(table[:tab.size], host[:tab.size])
        at = lambda name, row=0: table.data_ptr() + tab.offset(name, row)
        n_of = lambda name: tab.layout[name][2][0] if name in tab.layout else 0

        call("primia_image_affine_resize_crop_batch_u8", at("arc.ptrs"), at("arc.ip"), at("arc.fp"), B, C, R, S)
        if a.clahe:
            ws = self._grow("clahe", B * self.ws_bytes)
            call("primia_clahe_batch_u8", at("clahe.ptrs"), B, S, S, C, 1.0, ws, ws.numel())
        if n_of("fl.idx"):
            call("primia_image_flip_lut_batch_u8", at("fl.ptrs"), at("fl.ip"), at("fl.luts"), n_of("fl.idx"), S, C)
        if n_of("blur.idx"):
            call("primia_image_box_blur_batch_u8", at("blur.ptrs"), at("blur.k"), n_of("blur.idx"), S, C)
        if n_el:
            # the uniform fields of numpy's RandomState(seed), after elastic_affine's six draws, made on the device
            fields = self._grow("fields", n_el * 2 * S * S * 8)
            call("primia_mt19937_fields_batch", at("el.seed"), n_el, 6, 2 * S * S, fields)
            wsb = query("primia_warp_elastic_disp_workspace_bytes", n_el, S, S, 50.0)
            gws = self._grow("gauss", wsb)
            call("primia_image_warp_batch_u8", at("ela.ptrs"), at("ela.kind"), at("ela.dp"), n_el, S, C)
            call("primia_warp_elastic_disp_batch", fields, n_el, S, S, 50.0, 1.0, gws, gws.numel(), disp)
            call("primia_image_warp_batch_u8", at("elw.ptrs"), at("elw.kind"), at("ela.dp"), n_el, S, C)
        if n_of("opt.idx"):
            call("primia_image_warp_batch_u8", at("opt.ptrs"), at("opt.kind"), at("opt.dp"), n_of("opt.idx"), S, C)
        if n_of("grid.idx"):
            call("primia_image_warp_batch_u8", at("grid.ptrs"), at("grid.kind"), at("grid.steps"), n_of("grid.idx"), S, C)
        # (members of the -fast preset only: their per-image entry points on the image's slice, parameters in the table)
        for j in range(n_of("gs.idx")):
            s, d = tab.view("gs.ptrs")[j]
            call("primia_image_swap_tiles_u8", int(s), S, S, C, at("gs.tiles", j), 9, int(d))
        for j in range(n_of("hsv.idx")):
            s, d = tab.view("hsv.ptrs")[j]
            call("primia_image_hsv_shift_u8", int(s), S, S, at("hsv.luts", j), int(d))
        if n_of("inv.idx"):
            call("primia_image_flip_lut_batch_u8", at("inv.ptrs"), at("inv.ip"), at("inv.luts"), n_of("inv.idx"), S, C)
        if n_of("cut.idx"):
            call("primia_image_fill_rects_batch_u8", at("cut.ptrs"), at("cut.ip"), at("cut.rects"), n_of("cut.idx"), S, C, 0)
        for j in range(n_of("sh.idx")):
            s, d = tab.view("sh.ptrs")[j]
            first, count = tab.view("sh.cnt")[j]
            call("primia_image_shadow_u8", int(s), S, S, at("sh.verts", int(first)), int(count), 5, int(d))
        if n_of("fog.idx"):
            call("primia_image_fog_batch_u8", at("fog.ptrs"), at("fog.ip"), at("fog.alpha"), at("fog.haze"), n_of("fog.idx"), S, C)
        if n_of("fogb.k"):
            call("primia_image_box_blur_batch_u8", at("fogb.ptrs"), at("fogb.k"), n_of("fogb.k"), S, C)
        for j in range(n_of("sf.idx")):
            s, d = tab.view("sf.ptrs")[j]
            first, count, n_first = tab.view("sf.cnt")[j]
            f = int(first)
            call("primia_image_sun_flare_u8", int(s), S, S, at("sf.geo", f), at("sf.a32", f), at("sf.b32", f), int(count),
                 int(n_first), int(d))
        if n_of("sol.idx"):
            call("primia_image_flip_lut_batch_u8", at("sol.ptrs"), at("sol.ip"), at("sol.luts"), n_of("sol.idx"), S, C)
        for j in range(n_of("eq.idx")):
            s, d = tab.view("eq.ptrs")[j]
            call("primia_image_equalize_u8", int(s), S, S, C, self.eq_ws, self.eq_ws.numel(), int(d))
        if n_of("gd.idx"):
            call("primia_image_fill_rects_batch_u8", at("gd.ptrs"), at("gd.ip"), at("gd.rects"), n_of("gd.idx"), S, C, 0)
        if n_noise:
            # the values stay torch's: the same calls, of the same size, in image order, so the device generator ends where
            # the per-image path leaves it; scaling by sigma and the add are one batched launch
            planes = noise[:n_noise * px * 4].view(torch.float32).view(n_noise, px)
            for j in range(n_noise):
                torch.randn(px, generator=self.gen, out=planes[j])
            call("primia_image_add_noise_batch_u8", at("noise.ptrs"), planes, at("noise.sd"), n_noise, px)
        call("primia_image_finish_batch", at("fin.ptrs"), B, S, C, self.mean, self.std)
        if self._uploaded is None:
            self._uploaded = torch.cuda.Event()
        self._uploaded.record()
        return out


def create_albu_transform(args, mean, std, device="cuda:0", channels=None, seed=0):
    """torchlib/dataloader.py:138-217 by its own name: the training transform chain for `args`, as a TrainTransform
    (`tf(uint8 HWC device image, random.Random) -> fp32 [C, S, S]`).  `channels` defaults to 3 for `pretrained` presets and
    1 otherwise, as the reference's end_transformations do."""
    if channels is None:
        channels = 3 if getattr(args, "pretrained", True) else 1
    return TrainTransform(args, mean, std, device, channels, seed)

