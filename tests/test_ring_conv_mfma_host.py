"""Host: which kernel a ring convolution runs on (primia_ring_conv2d_route) with the option ring_mfma off and on."""
from primia_amd import _lib

# B, C, H, W, O, R, S, stride, pad, jobs
GEOMETRIES = {(3, 1): (1, 64, 56, 56, 64, 3, 3, 1, 1, 2), (3, 2): (1, 64, 56, 56, 128, 3, 3, 2, 1, 2),
              (1, 2): (1, 64, 56, 56, 128, 1, 1, 2, 0, 1), (7, 2): (1, 3, 224, 224, 64, 7, 7, 2, 3, 2)}


def test_route_follows_the_option():
    route = _lib.lib().primia_ring_conv2d_route
    try:
        for on in (0, 1):
            _lib.set_option("ring_mfma", on)
            assert {k: route(*g) for k, g in GEOMETRIES.items()} == {k: int(on and k != (7, 2)) for k in GEOMETRIES}
            assert route(1, 64, 56, 56, 64, 5, 5, 1, 2, 1) == -3 and route(1, 64, 56, 56, 64, 3, 3, 3, 1, 1) == -3
            assert route(1, 0, 56, 56, 64, 3, 3, 1, 1, 1) == -1 and route(1, 64, 56, 56, 64, 3, 3, 1, 1, 3) == -1
    finally:
        _lib.set_option("ring_mfma", 0)
