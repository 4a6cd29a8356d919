"""The composed oracle forward and the plaintext reference of tests/test_gpu_secure_avgpool.py and its three-role worker
(tests/party_worker_avgpool.py) for a network trained with pooling_type = avg: a module of helpers, not of tests."""
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


def oracle_avg_forward(ctx, state_dict, images, blocks=None):
    """The secure forward of images [B, C, S, S] composed from OracleContext's own methods, as
    tests/secure_batch_nets.py's oracle_batch_forward, with the stem of a pooling_type = avg network in the order it was
    trained with: conv1 -> bn1 -> ReLU -> AvgPool2d(3, 2, 1).  state_dict values / images are float32 numpy arrays."""
    p = {}
    for k in S.share_order(list(state_dict.keys())):
        p[k] = ctx.share(S.fix_encode(state_dict[k], ctx.base, ctx.pf))
    if blocks is None:
        blocks = [(f"layer{li}.{bi}", (2 if (li > 1 and bi == 0) else 1)) for li in range(1, 5) for bi in range(2)]
    x = ctx.share(S.fix_encode(images, ctx.base, ctx.pf))
    names = ["bn1"]
    for prefix, _ in blocks:
        names += [prefix + ".bn1", prefix + ".bn2"]
        if (prefix + ".downsample.0.weight") in p:
            names.append(prefix + ".downsample.1")
    inv_all = ctx.reciprocal_newton([np.concatenate([p[n + ".running_var"][j] for n in names]) for j in range(2)])
    inv, off = {}, 0
    for n in names:
        k = p[n + ".running_var"][0].size
        inv[n] = [inv_all[j][off:off + k] for j in range(2)]
        off += k

    def bn(t, prefix):
        return ctx.batch_norm_eval(t, p[prefix + ".running_mean"], p[prefix + ".running_var"], p[prefix + ".weight"],
                                   p[prefix + ".bias"], inv=inv[prefix])

    x = ctx.conv2d(x, p["conv1.weight"], 2, 3)
    x = ctx.relu(bn(x, "bn1"))
    x = oracle_avg_pool(x, 3, 2, 1)
    for prefix, stride in blocks:
        identity = x
        out = ctx.conv2d(x, p[prefix + ".conv1.weight"], stride, 1)
        out = ctx.relu(bn(out, prefix + ".bn1"))
        out = ctx.conv2d(out, p[prefix + ".conv2.weight"], 1, 1)
        out = bn(out, prefix + ".bn2")
        if (prefix + ".downsample.0.weight") in p:
            identity = ctx.conv2d(x, p[prefix + ".downsample.0.weight"], stride, 0)
            identity = bn(identity, prefix + ".downsample.1")
        x = ctx.relu(ctx.add(out, identity))
    x = ctx.avg_pool2d(x, x[0].shape[-1])
    B = x[0].shape[0]
    x = [t.reshape(B, -1) for t in x]
    return ctx.linear(x, p["fc.weight"], p["fc.bias"])


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
