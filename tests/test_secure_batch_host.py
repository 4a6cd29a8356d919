"""CPU: the host-side schedule and memory arithmetic of batched encrypted inference (no device is touched)."""
import pytest
import torch

from primia_amd import _lib, resnet_spec
from primia_amd.secure import (DIF_KEY_BYTES, GraphedSecureInference, architecture_of, image_requests, largest_batch_that_fits,
                               primitive_bytes, serving_bytes)


@pytest.fixture(scope="module")
def arch224():
    return architecture_of(resnet_spec.init_state_dict(resnet_spec.resnet18_spec(3, 3, 224, "max")))


@pytest.mark.parametrize("B", [1, 2, 8])
def test_schedule_of_a_batch_at_224(arch224, B):
    """What a batch shares and what it does not: the comparisons are B times one image's 3,311,616; the 21 matrix products
    and the 298 element-wise Beaver products (237 of them Newton's, on all 4,800 BatchNorm channels at once) are per batch,
    with B times the rows on the image side and the weight side unchanged."""
    req = image_requests(arch224, 224, B)
    assert sum(a[0] for k, a, _ in req if k == "dif_keys") == B * 3_311_616
    mm = [a for k, a, _ in req if k == "triple" and a[0] == "matmul"]
    assert len(mm) == 21 and mm[0] == ("matmul", (B, 12544, 147), (147, 64)) and mm[-1] == ("matmul", (B, 512), (512, 3))
    mul = [a for k, a, _ in req if k == "triple" and a[0] == "mul"]
    assert len(mul) == 298 and mul[:237] == [("mul", (4800,), (4800,))] * 237
    assert mul[237] == ("mul", (64,), (B * 12544, 64))
    assert req[0] == ("const_mask", (B, 3, 224, 224), {"owner": 1})


def test_static_bytes_are_affine_in_the_batch_and_dominated_by_the_keys(arch224):
    assert DIF_KEY_BYTES == 1244
    b = [primitive_bytes(image_requests(arch224, 224, k)) for k in (1, 2, 3, 8)]
    per_image = b[1] - b[0]
    assert b[2] - b[1] == per_image and b[3] - b[0] == 7 * per_image
    keys = 3_311_616 * DIF_KEY_BYTES
    assert keys < per_image < 1.25 * keys
    # per batch: Newton's 237 triples on 4,800 channels (55 MB) and the weight sides of the 21 products (11.2 M weights, four
    # shares each: 179 MB), about 5 % of one image's primitives
    fixed = b[0] - per_image
    assert 230e6 < fixed < 240e6
    for budget_images in (1, 5, 40):
        budget = serving_bytes(arch224, 224, budget_images)
        assert largest_batch_that_fits(arch224, 224, budget) == budget_images
        assert largest_batch_that_fits(arch224, 224, budget - 1) == budget_images - 1


def test_a_batch_beyond_the_budget_is_refused_before_anything_is_allocated():
    sd = resnet_spec.init_state_dict(resnet_spec.resnet18_spec(3, 3, 224, "max"))
    budget = 16 << 30
    fits = largest_batch_that_fits(architecture_of(sd), 224, budget)
    assert fits == 3
    with pytest.raises(ValueError, match=f"largest batch that fits is {fits}"):
        GraphedSecureInference(sd, "cuda:0", input_size=224, batch=8, memory_budget=budget)
    with pytest.raises(ValueError):
        GraphedSecureInference(sd, "cuda:0", input_size=224, batch=0, memory_budget=budget)


def test_header_declares_the_batch_entry_points():
    protos = _lib.parse_header()
    for name in ("primia_bn_eval_local_batch", "primia_nchw_to_rows", "primia_rows_to_nchw"):
        assert name in protos
    assert len(protos["primia_bn_eval_local_batch"][1]) == len(protos["primia_bn_eval_local"][1]) + 1
