"""Host only: the draws of the augmentation chain (primia_amd.augment.draw_plan) follow the draw order written in the
module's docstring, and the packed parameter table of a batch (pack_plans / unpack_plans) loses nothing."""
import random
from types import SimpleNamespace

import numpy as np

import primia_amd.augment as P

EVERY = dict(train_resolution=64, inference_resolution=72, rotation=30, translate=0.1, scale=0.15, shear=10, clahe=True,
             albu_prob=0.9, individual_albu_probs=0.6, noise_std=0.05, noise_prob=0.5, randomgamma=True,
             randombrightness=True, blur=True, elastic=True, optical_distortion=True, grid_distortion=True, grid_shuffle=True,
             hsv=True, invert=True, cutout=True, shadow=True, fog=True, sun_flare=True, solarize=True, equalize=True,
             grid_dropout=True)


class LoggingRandom(random.Random):
    def __init__(self, seed):
        super().__init__(seed)
        self.log = []

    def random(self):
        self.log.append(("random",))
        return super().random()

    def uniform(self, a, b):
        self.log.append(("uniform", a, b))
        return super().uniform(a, b)

    def randint(self, a, b):
        self.log.append(("randint", a, b))
        return super().randint(a, b)

    def choice(self, seq):
        self.log.append(("choice", tuple(seq)))
        return super().choice(seq)


def expected_log(H, W, rng, cfg):
    """The docstring's draw order, restated: affine angle, translate x, y, scale, shear; crop h, w; Compose coin; then per
    enabled transform its own coin and, if it fires, its parameters.  `rng` (a LoggingRandom on the same seed) decides the
    coins; the helpers that draw lists (holes, vertices, haze, flare) are the product's own, logged through `rng`."""
    S = cfg.train_resolution
    rng.uniform(-cfg.rotation, cfg.rotation)
    rng.uniform(-cfg.translate * W, cfg.translate * W), rng.uniform(-cfg.translate * H, cfg.translate * H)
    rng.uniform(1.0 - cfg.scale, 1.0 + cfg.scale)
    rng.uniform(-cfg.shear, cfg.shear)
    rng.random(), rng.random()
    if not rng.random() < cfg.albu_prob:
        return
    q = cfg.individual_albu_probs
    coin = lambda: rng.random() < q
    coin()                                                  # VerticalFlip
    if coin():
        rng.randint(80, 120)                                # RandomGamma
    if coin():
        rng.uniform(0.0, 0.0), rng.uniform(-0.2, 0.2)       # RandomBrightness
    if coin():
        rng.choice([3, 5, 7])                               # Blur
    if coin():
        rng.randint(0, 10000)                               # ElasticTransform
    if coin():
        rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)        # OpticalDistortion
    if coin():
        for _ in range(12):
            rng.uniform(-0.3, 0.3)                          # GridDistortion
    if coin():
        rng.randint(0, 10000)                               # RandomGridShuffle
    if coin():
        rng.uniform(-20, 20), rng.uniform(-30, 30), rng.uniform(-20, 20)                    # HueSaturationValue
    coin()                                                  # InvertImg
    if coin():
        P.cutout_holes(S, S, rng)
    if coin():
        P.shadow_vertices(S, S, rng)
    if coin():
        P.fog_params(S, S, rng)
    if coin():
        P.sun_flare_steps(S, S, rng)
    if coin():
        rng.uniform(128, 128)                               # Solarize
    coin()                                                  # Equalize
    coin()                                                  # GridDropout
    if rng.random() < cfg.noise_prob:
        rng.uniform(0.0, cfg.noise_std ** 2)                # GaussNoise


def test_plan_draws_in_the_documented_order():
    cfg = P.transform_config(SimpleNamespace(**EVERY))
    a, b = LoggingRandom(5), LoggingRandom(5)
    fired = set()
    for i in range(60):
        H, W = 100 + 3 * i, 80 + i
        p = P.draw_plan(cfg, H, W, a)
        expected_log(H, W, b, cfg)
        assert a.log == b.log, i
        fired |= set(p)
        assert p["H"] == H and p["W"] == W and p["affine"].dtype == np.float32 and 0 <= p["oy"] <= 8 and 0 <= p["ox"] <= 8
    assert a.getstate() == b.getstate() and len(a.log) > 1000
    assert fired >= set(P.TrainTransform.MEMBERS), set(P.TrainTransform.MEMBERS) - fired
    # augment=False draws the crop only
    c = LoggingRandom(1)
    assert set(P.draw_plan(cfg, 50, 60, c, augment=False)) == {"H", "W", "oy", "ox"} and c.log == [("random",), ("random",)]


def test_packing_plans_and_unpacking_them_is_the_identity():
    cfg = P.transform_config(SimpleNamespace(**EVERY))
    rng = random.Random(3)
    plans = [P.draw_plan(cfg, 100 + i, 90 + 2 * i, rng, augment=i % 7 != 0) for i in range(40)]
    assert set().union(*plans) >= set(P.TrainTransform.MEMBERS)
    S, C, px = 64, 3, 64 * 64 * 3
    addr = dict(src=[1000 * i for i in range(40)], buf=(1 << 20, 1 << 24), out=1 << 28, disp=1 << 29, noise=1 << 30)
    tab = P.pack_plans(plans, S, C, True, addr)
    buf = tab.write(np.full(tab.size + 32, 0xEE, np.uint8), table_address=1 << 32)
    assert (buf[tab.size:] == 0xEE).all() and all(off % 16 == 0 for off, _, _ in tab.layout.values())
    back = P.unpack_plans(buf, tab.layout)
    assert len(back) == len(plans) and all(P.plans_equal(x, y) for x, y in zip(plans, back))
    assert not P.plans_equal(plans[1], plans[2])
    # the pointer records: every image starts in buffer 0, each out-of-place stage moves it to the other buffer's slice i,
    # and the last stage reads it where the chain left it
    get = lambda name: np.frombuffer(bytes(buf[tab.layout[name][0]:]), tab.layout[name][1],
                                     int(np.prod(tab.layout[name][2]))).reshape(tab.layout[name][2])
    arc, fin = get("arc.ptrs"), get("fin.ptrs")
    for i in range(40):
        assert arc[i, 0] == 1000 * i and arc[i, 1] == (1 << 20) + i * px and fin[i, 1] == (1 << 28) + i * px * 4
        assert fin[i, 0] in ((1 << 20) + i * px, (1 << 24) + i * px)
    blur = get("blur.ptrs")
    assert all(abs(int(s) - int(d)) == (1 << 24) - (1 << 20) for s, d in blur)
    grid = get("grid.ptrs")                                   # the axes live in the table itself: rebased to its address
    lo = (1 << 32) + tab.layout["grid.axes"][0]
    assert all(lo <= int(p) < lo + tab.arrays["grid.axes"].nbytes for p in grid[:, 2:].reshape(-1))
