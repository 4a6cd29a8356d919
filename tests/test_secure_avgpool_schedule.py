"""CPU: the host-side primitive schedule of the encrypted forward for a checkpoint trained with pooling_type = avg.

The avg stem is conv1 -> bn1 -> ReLU -> AvgPool2d(3, 2, 1): one comparison batch and one element-wise triple at conv1's
output resolution, and a party-local pool that asks the dealer for nothing.  At 224 x 224 that is 64 * 112 * 112 = 802,816
comparisons in place of the max stem's 64 * 56 * 56 * (4 + 2 + 1 + 1 + 1) = 1,806,336: 2,308,096 per image against 3,311,616,
and 294 element-wise triples against 298 (one ReLU in place of four tree levels and one ReLU).  The default and
pooling="max" stay what they were."""
import pytest

from primia_amd import resnet_spec
from primia_amd.secure import (DIF_KEY_BYTES, architecture_of, image_requests, largest_batch_that_fits, primitive_bytes,
                               serving_bytes)

MAX_COMPARISONS, AVG_COMPARISONS = 3_311_616, 2_308_096


@pytest.fixture(scope="module")
def arch():
    return architecture_of(resnet_spec.init_state_dict(resnet_spec.resnet18_spec(3, 3, 224, "avg")))


def comparisons(req):
    return sum(args[0] for kind, args, _ in req if kind == "dif_keys")


def triples(req, op):
    return sum(1 for kind, args, _ in req if kind == "triple" and args[0] == op)


def test_avg_schedule_of_one_224_image(arch):
    req = image_requests(arch, 224, 1, pooling="avg")
    assert comparisons(req) == AVG_COMPARISONS
    assert triples(req, "mul") == 294 and triples(req, "matmul") == 21
    # the stem: conv1's product, bn1's two products, then ONE comparison batch and ONE product on the 112 x 112 map, and the
    # first block's conv follows at once (the pool requests nothing)
    i = req.index(("triple", ("matmul", (1, 112 * 112, 147), (147, 64)), {}))
    assert req[i + 3:i + 6] == [("dif_keys", (64 * 112 * 112,), {}),
                                ("triple", ("mul", (1, 64, 112, 112), (1, 64, 112, 112)), {}),
                                ("triple", ("matmul", (1, 56 * 56, 576), (576, 64)), {})]


def test_max_schedule_is_unchanged(arch):
    default = image_requests(arch, 224, 1)
    assert image_requests(arch, 224, 1, pooling="max") == default
    assert comparisons(default) == MAX_COMPARISONS
    assert triples(default, "mul") == 298 and triples(default, "matmul") == 21
    # the two schedules differ in the stem only: max's tree (4 comparison batches + 4 products) and its ReLU on the 56 x 56
    # map against avg's ReLU on the 112 x 112 map
    avg = image_requests(arch, 224, 1, pooling="avg")
    i = default.index(("triple", ("matmul", (1, 112 * 112, 147), (147, 64)), {})) + 3
    assert default[:i] == avg[:i] and default[i + 10:] == avg[i + 2:]
    rows = 64 * 56 * 56
    assert [a[0] for k, a, _ in default[i:i + 10] if k == "dif_keys"] == [4 * rows, 2 * rows, rows, rows, rows]


@pytest.mark.parametrize("batch", [2, 5])
def test_avg_comparisons_scale_with_the_batch(arch, batch):
    req = image_requests(arch, 224, batch, pooling="avg")
    assert comparisons(req) == batch * AVG_COMPARISONS
    assert triples(req, "mul") == 294 and triples(req, "matmul") == 21          # per batch, not per image


def test_avg_needs_less_memory_and_admits_no_smaller_batch(arch):
    for batch in (1, 4):
        avg, mx = serving_bytes(arch, 224, batch, pooling="avg"), serving_bytes(arch, 224, batch, pooling="max")
        assert mx == serving_bytes(arch, 224, batch)
        assert avg < mx
        # at least the keys of the comparisons the avg stem does not make
        assert mx - avg >= batch * (MAX_COMPARISONS - AVG_COMPARISONS) * DIF_KEY_BYTES
    b = primitive_bytes(image_requests(arch, 224, 1, pooling="avg"))
    assert serving_bytes(arch, 224, 1, pooling="avg") == b + b // 8
    for images in (3, 7):
        budget = serving_bytes(arch, 224, images) + 1000
        assert largest_batch_that_fits(arch, 224, budget) == images
        assert largest_batch_that_fits(arch, 224, budget, pooling="max") == images
        fits = largest_batch_that_fits(arch, 224, budget, pooling="avg")
        assert fits >= images
        assert serving_bytes(arch, 224, fits, pooling="avg") <= budget < serving_bytes(arch, 224, fits + 1, pooling="avg")


def test_unknown_pooling_is_refused(arch):
    for fn in (lambda: image_requests(arch, 224, 1, pooling="median"),
               lambda: serving_bytes(arch, 224, 1, pooling="median"),
               lambda: largest_batch_that_fits(arch, 224, 10 ** 10, pooling=None)):
        with pytest.raises(ValueError, match="pooling"):
            fn()
