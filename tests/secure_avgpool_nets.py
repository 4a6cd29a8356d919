"""The oracle's average pool and the plaintext reference of tests/test_gpu_secure_avgpool.py for a network trained with
pooling_type = avg: a module of helpers, not of tests."""
import numpy as np
import torch

from oracle import secure_oracle as S
from oracle import train_oracle as O

I64, U64 = np.int64, np.uint64


def oracle_avg_pool(x, k, stride, pad):
    """_pool2d(mode="avg") of both shares on the host: per share `pre_pool` (zero padding of the SHARES), the wrapping sum of
    each window and AST.mean's truncating division by k*k -- for every window, border windows included."""
    out = []
    for j in range(2):
        im, (B, C, Ho, Wo) = S.pre_pool(x[j], k, stride, pad)
        s = np.ascontiguousarray(im).view(U64).sum(axis=-1, dtype=U64).view(I64)
        out.append(S.trunc_div(s, k * k).reshape(B, C, Ho, Wo))
    return out


def plaintext_logits(sd, images, pf, size, pooling):
    """oracle.train_oracle.forward in float64 on the fixed-point-rounded parameters and images (the recipe of
    tests/test_gpu_secure_batch.py's plaintext_logits); the secure BatchNorm has no eps: the reference's 1e-5 is taken back
    out of running_var."""
    def q(v):
        return torch.from_numpy(S.fix_encode(v.numpy(), 10, pf).astype(np.float64) / 10 ** pf)

    sd64 = {k: (q(v) if v.is_floating_point() else v) for k, v in sd.items()}
    for k in sd64:
        if k.endswith(".running_var"):
            sd64[k] = sd64[k] - 1e-5
    with torch.no_grad():
        return O.forward(sd64, q(images), training=False, pooling=pooling, input_size=size).numpy()
