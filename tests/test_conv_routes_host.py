"""CPU: every host-side convolution query of the library against tests/golden/conv_routes.npz, the table minted from the
build BEFORE the dispatch moved onto one route decision per pass (tests/golden/make_conv_routes_golden.py).  The engine
sizes device buffers from these queries and launches through the dispatch, and the GPU tests prove a case's kernel by the id
queries: one route function now feeds both, and this table pins what it must answer — shape by shape, dtype by dtype, under
every option setting a test or a tool uses.  No compute calls: there is no GPU here."""
import importlib.util
import os

import numpy as np
import pytest

from primia_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def mint():
    spec = importlib.util.spec_from_file_location("make_conv_routes_golden", os.path.join(GOLDEN, "make_conv_routes_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "conv_routes.npz"))


def test_table_describes_the_cases_of_the_minting_script(mint, gold):
    assert np.array_equal(gold["shapes"], np.array(mint.shapes(), np.int64))
    assert np.array_equal(gold["dtypes"], np.array(mint.DTYPES, np.int64))
    assert np.array_equal(gold["settings"], mint.settings_array())
    assert gold["values"].shape == (len(mint.SETTINGS), len(mint.shapes()), len(mint.DTYPES), len(mint.QUERIES))
    assert gold["values"].dtype == np.int64


def test_table_reaches_every_kernel_id(mint, gold):
    """A condition on the cases, not a measurement: each id of the two dispatch tables is somebody's answer."""
    v, col = gold["values"], mint.QUERIES.index
    assert {1, 2, 4, 5, 6} <= set(v[..., [col("kernel_id fwd"), col("kernel_id dgrad")]].flatten().tolist())
    assert {13, 14, 15, 17, 18} <= set(v[..., col("wgrad_kernel_id")].flatten().tolist())
    assert {21, 24, 25, 26} <= set(v[..., col("wgrad_persample_kernel_id")].flatten().tolist())


def test_every_query_answers_as_before_the_route(mint, gold):
    got = mint.table(_lib)
    want = gold["values"]
    bad = np.argwhere(got != want)
    shp = mint.shapes()
    lines = [f"{mint.SETTINGS[s] or 'defaults'} {shp[h]} {'bf16' if mint.DTYPES[d] else 'fp32'} {mint.QUERIES[q]}: "
             f"{got[s, h, d, q]} != {want[s, h, d, q]}" for s, h, d, q in bad[:12].tolist()]
    assert not len(bad), f"{len(bad)} of {want.size} answers changed:\n" + "\n".join(lines)


@pytest.mark.parametrize("dt", [_lib.PRIMIA_F32, _lib.PRIMIA_BF16])
def test_the_stem_always_asks_for_a_weight_gradient_workspace(dt):
    """conv1 takes the route's stem branch, whose workspace is a product of positive counts: the engine's shared
    weight-gradient workspace therefore exists at every shape, and the engine has no accumulate-form alternative."""
    for size in (32, 64, 96, 224):
        for batch in (1, 4, 256):
            d = _lib.ConvDesc.make(batch, size, size, 4, 64, 7, 7, 2, 3)
            assert _lib.query("primia_conv_wgrad_ws_bytes", d, dt) > 0, (batch, size)
