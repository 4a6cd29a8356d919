"""primia_mt19937_fields_batch's argument checks, on a machine without a GPU: a refusal (and n = 0) returns before any HIP call,
so the entry point can be driven with made-up addresses that nothing dereferences."""
import pytest

from primia_amd import _lib

OK, ERR_ARG = 0, -1
PTR = 0x1000                       # non-null, aligned, never read: every case below returns before a launch


@pytest.mark.parametrize("seeds,n,skip,count,out,want", [
    (PTR, 0, 6, 4, PTR, OK),                       # nothing to do
    (None, 1, 6, 4, PTR, ERR_ARG), (PTR, 1, 6, 4, None, ERR_ARG),
    (PTR, -1, 6, 4, PTR, ERR_ARG), (PTR, 1, -1, 4, PTR, ERR_ARG),
    (PTR, 1, 6, 0, PTR, ERR_ARG), (PTR, 1, 6, -3, PTR, ERR_ARG),
    (PTR, 32768, 0, 1, PTR, ERR_ARG),              # 2 * n > PRIMIA_BATCH_MAX
    (PTR, 2 ** 30 + 1, 0, 1, PTR, ERR_ARG),        # 2 * n does not wrap into range
    (PTR, 1, 2 ** 63 - 1, 2, PTR, ERR_ARG),        # skip + count overflows
    (PTR, 1, 6, 4, PTR + 4, ERR_ARG),              # out not aligned for a double
])
def test_refused_before_any_launch(seeds, n, skip, count, out, want):
    assert _lib.lib().primia_mt19937_fields_batch(seeds, n, skip, count, out, None) == want
