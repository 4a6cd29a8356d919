"""The float64 form of DP-SGD's class-weighted pieces (csrc/dp_weighted.hip, primia_amd/dp_weights.py) in numpy.

`xent_weighted` walks the classes in the kernel's order (the sum of exponentials is sequential, the target element is
softmax - 1 as written), so that the only difference left between the two is the device's `exp` against numpy's in the last
float64 place and the kernel's one rounding to float32."""
import numpy as np


def xent_weighted(logits, target, weight, scale):
    """(dlogits float64 [N, C], loss float64) of primia_xent_dp_weighted: rows with target < 0 are zero and not counted,
    rows with target >= C are NaN and make the loss NaN, every other row is w[t] * scale * (softmax - onehot); the loss is
    the mean of w[t] * CE over the counted rows, 0 when there is none."""
    o = np.asarray(logits, dtype=np.float32).astype(np.float64)
    t = np.asarray(target, dtype=np.int64)
    w = np.asarray(weight, dtype=np.float32).astype(np.float64)
    s = np.float64(np.float32(scale))
    N, C = o.shape
    d = np.zeros((N, C))
    num, valid = 0.0, 0
    for n in range(N):
        if t[n] < 0:
            continue
        valid += 1
        if t[n] >= C:
            d[n] = np.nan
            num = np.nan
            continue
        mx = o[n].max()
        se = 0.0
        for c in range(C):
            se = se + np.exp(o[n, c] - mx)
        num = num + w[t[n]] * (mx + np.log(se) - o[n, t[n]])
        ws = w[t[n]] * s
        for c in range(C):
            d[n, c] = ws * (np.exp(o[n, c] - mx) / se - (1.0 if c == t[n] else 0.0))
    return d, (num / valid if valid else 0.0)


def histogram(targets, num_classes):
    t = np.asarray(targets, dtype=np.int64)
    t = t[(t >= 0) & (t < num_classes)]
    return np.bincount(t, minlength=num_classes)[:num_classes].astype(np.int64)


def noised_counts(targets, num_classes, z, sigma):
    """int64 [C]: max(0, rint(count + sigma * z)), sigma and z taken at their float32 values, as the kernel does."""
    z = np.zeros(num_classes, dtype=np.float32) if z is None else np.asarray(z, dtype=np.float32)
    v = np.rint(histogram(targets, num_classes).astype(np.float64) + np.float64(np.float32(sigma)) * z.astype(np.float64))
    return np.maximum(v, 0.0).astype(np.int64)


def balanced_weights(counts):
    """float64 [C]: sum / (C * count) over counts clamped at 1."""
    c = np.maximum(np.asarray(counts, dtype=np.float64), 1.0)
    return c.sum() / (c.size * c)
