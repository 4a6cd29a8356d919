"""Networks and the composed oracle forward (every stem pool, every norm) shared by the tests of encrypted inference: a module
of helpers, not of tests."""
import numpy as np
import torch

from oracle import secure_oracle as S
from primia_amd import resnet_spec
from tests.secure_avgpool_nets import oracle_avg_pool
from tests.secure_groupnorm_nets import oracle_group_norm


def draw_bn(sd, name, c, gen):
    """A BatchNorm that is not the identity: weight U[0.5, 1.5), bias and mean N(0, 0.1), var U[0.5, 1.5)."""
    sd[name + ".weight"] = torch.rand(c, generator=gen) + 0.5
    sd[name + ".bias"] = torch.randn(c, generator=gen) * 0.1
    sd[name + ".running_mean"] = torch.randn(c, generator=gen) * 0.1
    sd[name + ".running_var"] = torch.rand(c, generator=gen) + 0.5


def resnet18(size, seed):
    """The 8-block ResNet-18 for `size` x `size` RGB images and 3 classes from the reference's initialisation under a
    fixed seed, every BatchNorm redrawn (init's (1, 0, 0, 1) makes each one the identity)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        sd = resnet_spec.init_state_dict(resnet_spec.resnet18_spec(3, 3, size, "max"))
    gen = torch.Generator().manual_seed(seed + 1)
    for k in [k for k in sd if k.endswith(".running_var")]:
        draw_bn(sd, k[:-len(".running_var")], sd[k].numel(), gen)
    return sd


MINI_BLOCKS = [("layer1.0", 1), ("layer2.0", 2)]


def mini_resnet(gen):
    """Stem, one identity block and one projection block: the full op mix on a network a three-process run finishes soon."""
    sd = {}

    def conv(name, o, i, k):
        sd[name + ".weight"] = torch.randn(o, i, k, k, generator=gen) * (1.0 / (i * k * k) ** 0.5)

    def bn(name, c):
        draw_bn(sd, name, c, gen)
        sd[name + ".num_batches_tracked"] = torch.tensor(1)

    conv("conv1", 64, 3, 7)
    bn("bn1", 64)
    for p, cin, cout in (("layer1.0", 64, 64), ("layer2.0", 64, 128)):
        conv(p + ".conv1", cout, cin, 3)
        bn(p + ".bn1", cout)
        conv(p + ".conv2", cout, cout, 3)
        bn(p + ".bn2", cout)
    conv("layer2.0.downsample.0", 128, 64, 1)
    bn("layer2.0.downsample.1", 128)
    sd["fc.weight"] = torch.randn(3, 128, generator=gen) * 0.1
    sd["fc.bias"] = torch.randn(3, generator=gen) * 0.1
    return sd


def numpy_sd(sd):
    return {k: v.numpy() for k, v in sd.items()}


def oracle_forward(ctx, state_dict, images, blocks=None, pooling="max", norm="batch"):
    """The secure forward of images [B, C, S, S], composed from OracleContext's own methods (which are batch-general),
    oracle_avg_pool and oracle_group_norm -- nothing of primia_amd.secure, so that it stays an independent reference.
    oracle.secure_oracle.secure_resnet_forward flattens the pooled features with reshape(1, -1), this one with reshape(B, -1).
    pooling="avg": the stem in the order a pooling_type = avg network was trained with, conv1 -> norm -> ReLU ->
    AvgPool2d(3, 2, 1); "max": the swapped stem, max pool before ReLU.  norm="batch": the Newton reciprocal of every layer's
    running_var hoisted into one call; "group": oracle_group_norm at every norm site, nothing hoisted.
    state_dict values / images are float32 numpy arrays."""
    p = {}
    for k in S.share_order(list(state_dict.keys())):
        p[k] = ctx.share(S.fix_encode(state_dict[k], ctx.base, ctx.pf))
    if blocks is None:
        blocks = [(f"layer{li}.{bi}", (2 if (li > 1 and bi == 0) else 1)) for li in range(1, 5) for bi in range(2)]
    x = ctx.share(S.fix_encode(images, ctx.base, ctx.pf))
    if norm == "batch":
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
        if norm == "group":
            return oracle_group_norm(ctx, t, p[prefix + ".weight"], p[prefix + ".bias"])
        return ctx.batch_norm_eval(t, p[prefix + ".running_mean"], p[prefix + ".running_var"], p[prefix + ".weight"],
                                   p[prefix + ".bias"], inv=inv[prefix])

    x = bn(ctx.conv2d(x, p["conv1.weight"], 2, 3), "bn1")
    if pooling == "max":
        x = ctx.relu(ctx.max_pool2d_3x3s2(x))
    else:
        x = oracle_avg_pool(ctx.relu(x), 3, 2, 1)
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


def plain_forward(sd, images, blocks, pf):
    """float64 plaintext forward of a network given as (state dict, blocks) on the fixed-point-rounded parameters and images:
    what the secure forward computes up to its truncations and its Newton reciprocal square root (BatchNorm without eps, as
    the secure one; max pool before ReLU, as the swapped stem -- the two commute)."""
    F = torch.nn.functional

    def q(v):
        return torch.from_numpy(S.fix_encode(v.numpy(), 10, pf).astype(np.float64) / 10 ** pf)

    p = {k: q(v) for k, v in sd.items() if v.is_floating_point()}

    def bn(t, n):
        sh = (1, -1, 1, 1)
        return (t - p[n + ".running_mean"].view(sh)) / p[n + ".running_var"].view(sh).sqrt() * p[n + ".weight"].view(sh) \
            + p[n + ".bias"].view(sh)

    x = bn(F.conv2d(q(images), p["conv1.weight"], stride=2, padding=3), "bn1")
    x = F.relu(F.max_pool2d(x, 3, 2, 1))
    for prefix, stride in blocks:
        out = F.relu(bn(F.conv2d(x, p[prefix + ".conv1.weight"], stride=stride, padding=1), prefix + ".bn1"))
        out = bn(F.conv2d(out, p[prefix + ".conv2.weight"], stride=1, padding=1), prefix + ".bn2")
        if (prefix + ".downsample.0.weight") in p:
            x = bn(F.conv2d(x, p[prefix + ".downsample.0.weight"], stride=stride), prefix + ".downsample.1")
        x = F.relu(out + x)
    x = x.mean(dim=(2, 3))
    return (x @ p["fc.weight"].t() + p["fc.bias"]).numpy()
