"""Host: what train.py decides about --dp_augmult (augmentation multiplicity) before anything touches a GPU, the sizes the
loaders and the micro-batch passes count in records and in slots, the walks a record's views read, and the new entry points'
declarations and refusals (no GPU needed)."""
import ctypes
import warnings
from types import SimpleNamespace

import pytest
import torch

import train
from primia_amd import _lib, dp_micro, graphed_train
from primia_amd.dp_sampling import PoissonAugmentingLoader, PoissonLoader, _PoissonBase

ON = SimpleNamespace(differentially_private=True, pretrained=False, batch_size=8)
OFF = SimpleNamespace(differentially_private=False, pretrained=False, batch_size=8)


def test_parser_and_options():
    p = train.build_parser()
    assert p.parse_args(["--config", "x.ini"]).dp_augmult == 1
    assert p.parse_args(["--config", "x.ini", "--dp_augmult", "4"]).dp_augmult == 4
    with pytest.raises(SystemExit):
        p.parse_args(["--config", "x.ini", "--dp_augmult", "two"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        dp = train.DPOptions.from_args(ON, SimpleNamespace(dp_augmult=4, dp_sampling="poisson"))
        assert dp.augmult == 4 and dp.poisson and dp.micro == 1
        assert train.DPOptions.from_args(ON, SimpleNamespace(dp_sampling="poisson")).augmult == 1
        assert train.DPOptions.from_args(ON, None).augmult == 1
        assert train.DPOptions.from_args(ON, SimpleNamespace(dp_augmult=1)).augmult == 1     # one view: shuffle mode is fine
        assert train.DPOptions().augmult == 1
    for bad in (0, -3):
        with pytest.raises(SystemExit, match="at least 1"):
            train.DPOptions.from_args(ON, SimpleNamespace(dp_augmult=bad, dp_sampling="poisson"))


def test_shuffle_mode_is_refused_by_name():
    for cmd in (SimpleNamespace(dp_augmult=2), SimpleNamespace(dp_augmult=2, dp_sampling="shuffle")):
        with pytest.raises(SystemExit, match=r"--dp_augmult 2 needs --dp_sampling poisson"):
            train.DPOptions.from_args(ON, cmd)


def test_without_dp_the_flag_warns_and_does_nothing():
    with pytest.warns(UserWarning, match="--dp_augmult 3 has no effect"):
        assert train.DPOptions.from_args(OFF, SimpleNamespace(dp_augmult=3)).augmult == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert train.DPOptions.from_args(OFF, SimpleNamespace(dp_augmult=1)).augmult == 1


class _Sampler:
    device = torch.device("cpu")


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_sizes_in_records_and_slots(m, K):
    """capacity, micro_size and slots count records; the batch and an engine of one pass hold m rows per record."""
    cap = 7
    base = _PoissonBase(20, 4, cap, _Sampler(), micro_batches=K, views=m)
    assert base.views == m and base.capacity == cap
    assert base.micro_size == train.micro_batch_size(cap, K, True) == -(-cap // K)
    assert base.slots == K * base.micro_size >= cap
    plain = _PoissonBase(20, 4, cap, _Sampler(), micro_batches=K)
    assert (base.q, base.threshold, base.expected_batch, len(base)) == (plain.q, plain.threshold, plain.expected_batch,
                                                                        len(plain))
    data = torch.zeros(2 * 20, 4)
    loader = PoissonLoader(data, torch.zeros(40, dtype=torch.int64), 4, cap, _Sampler(), repetitions=2, micro_batches=K,
                           views=m)
    assert loader.x.shape[0] == loader.y.shape[0] == loader.slots * m and loader.n == 20
    assert (loader.x.shape[0] // K) % m == 0 and loader.x.shape[0] // K == loader.micro_size * m    # an engine of one pass
    assert (loader.y == -1).all()
    aug = PoissonAugmentingLoader([None] * 20, torch.zeros(20, dtype=torch.int64), None, None, 4, cap, _Sampler(), (1, 2, 2),
                                  micro_batches=K, views=m)
    assert aug.x.shape == (aug.slots * m, 1, 2, 2) and aug.n == 20
    with pytest.raises(ValueError, match="views"):
        _PoissonBase(20, 4, cap, _Sampler(), views=0)


def test_walks_of_an_epoch():
    """Epoch e reads walks (e * m + v) % repetitions; with m > repetitions the views repeat stored copies."""
    data, targets = torch.zeros(5 * 6, 4), torch.zeros(30, dtype=torch.int64)
    loader = PoissonLoader(data, targets, 2, 4, _Sampler(), repetitions=5, views=2)
    assert [loader.walks(e) for e in range(4)] == [[0, 1], [2, 3], [4, 0], [1, 2]]
    one = PoissonLoader(data, targets, 2, 4, _Sampler(), repetitions=5)
    assert [one.walks(e) for e in range(6)] == [[0], [1], [2], [3], [4], [0]]      # as before: epoch % repetitions
    few = PoissonLoader(data[:12], targets[:12], 2, 4, _Sampler(), repetitions=2, views=3)
    assert few.walks(0) == [0, 1, 0] and few.walks(1) == [1, 0, 1]


def test_logical_batch_of_a_split_step_counts_records(monkeypatch):
    """dp_micro.step on 12 rows of 3-view records, an engine of 6 slots: two passes, logical_batch = 4 records."""
    seen = []
    root = SimpleNamespace(N=6, dp_params={"views": 3})
    root._root = root

    def one_pass(engine, optimizer, x, y, soft=False, phase=None, logical_batch=None):
        seen.append((x.shape[0], phase, logical_batch))
        return torch.ones(())

    import primia_amd.step as step_module

    monkeypatch.setattr(step_module, "eager_step", one_pass)
    dp_micro.step(root, None, torch.zeros(12, 1), torch.zeros(12, dtype=torch.int64))
    assert seen == [(6, "first", 4), (6, "last", 4)]
    del seen[:]
    root.dp_params = {}
    dp_micro.step(root, None, torch.zeros(12, 1), torch.zeros(12, dtype=torch.int64))
    assert seen == [(6, "first", 12), (6, "last", 12)]


def test_graph_key_and_divisor_count_records():
    eng = SimpleNamespace(N=8)
    assert graphed_train._divisor(eng, {"views": 2}) == 4 and graphed_train._divisor(eng, {}) == 8
    assert graphed_train._divisor(eng, {"views": 2, "expected_batch": 3.5}) == 3.5
    assert graphed_train._divisor(eng, {"views": 2}, "last", 6) == 6


def test_entry_points_are_declared_and_refuse_bad_records():
    protos = _lib.protos()
    names = ("primia_conv2d_wgrad_record_sqnorm", "primia_stem_conv_wgrad_record_sqnorm", "primia_conv_wgrad_record_kernel_id",
             "primia_record_sqnorm", "primia_record_sqnorm_many", "primia_dp_expand_clip", "primia_gather_records")
    lib = _lib.lib()
    for n in names:
        assert n in protos and hasattr(lib, n), n
    assert [a for _, a in protos["primia_conv2d_wgrad_record_sqnorm"][1]] == ["d", "x", "dy", "sqnorm", "views", "dtype",
                                                                              "stream"]
    assert [a for _, a in protos["primia_stem_conv_wgrad_record_sqnorm"][1]] == ["x_padded", "dy", "sqnorm", "N", "H", "W",
                                                                                 "views", "dtype", "stream"]
    assert [a for _, a in protos["primia_conv_wgrad_record_kernel_id"][1]] == ["d", "dtype", "views"]
    # the route (host only): one view answers as the per-sample query; several views never name a Gram-matrix kernel
    ghost = _lib.ConvDesc.make(12, 7, 7, 512, 512, 3, 3, 1, 1)
    assert _lib.query("primia_conv_wgrad_persample_kernel_id", ghost, 1) == 21
    assert _lib.query("primia_conv_wgrad_record_kernel_id", ghost, 1, 1) == 21
    assert _lib.query("primia_conv_wgrad_record_kernel_id", ghost, 1, 4) == 25
    assert _lib.query("primia_conv_wgrad_record_kernel_id", ghost, 0, 4) == 14
    for views in (0, -1, 5):
        assert _lib.query("primia_conv_wgrad_record_kernel_id", ghost, 1, views) == -1
    # refused before any launch (non-null pointers that are never dereferenced)
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for views in (0, 5):
        assert lib.primia_conv2d_wgrad_record_sqnorm(ctypes.cast(ctypes.pointer(ghost), ctypes.c_void_p), ptr, ptr, ptr, views,
                                                     1, None) == -1
        assert lib.primia_stem_conv_wgrad_record_sqnorm(ptr, ptr, ptr, 12, 64, 64, views, 1, None) == -1
        assert lib.primia_record_sqnorm(ptr, 12, 4, views, ptr, None) == -1
        assert lib.primia_record_sqnorm_many(ptr, ptr, 1, 12, views, ptr, None) == -1
        assert lib.primia_dp_expand_clip(ptr, ptr, 12, views, None) == -1
    assert lib.primia_gather_records(ptr, 4, 3, ptr, ptr, 0, 1, 0, ptr, ptr, 2, 0, None) == -1
    assert lib.primia_gather_records(ptr, 4, 3, ptr, ptr, 0, 0, 2, ptr, ptr, 2, 0, None) == -1
    assert lib.primia_gather_records(ptr, 4, 3, ptr, ptr, -1, 1, 2, ptr, ptr, 2, 0, None) == -1
