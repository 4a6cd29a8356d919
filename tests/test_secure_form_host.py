"""CPU: primia_amd.secure.ProtocolForm, the one place for the options the three roles of an encrypted inference agree on.
a. Nothing moved: request lists, static bytes, largest batches and refusals over the whole option grid equal what the commit
   before the form computed (tests/golden/secure_form_schedules.json, tests/golden/make_secure_form_golden.py).
b. The form itself: frozen, validated with the messages of old, `of`, `check`.
c. Every entry point takes `form=` or the five names by keyword, no option by position (but the stem pool, as fifth
   argument of the three schedule functions), and means the same by either."""
import dataclasses
import importlib.util
import inspect
import json
import os

import pytest
import torch

from primia_amd import secure
from primia_amd.secure import (EVALUATION_REVEALS, POOLINGS, GraphedSecureInference, PipelinedSecureInference, ProtocolForm,
                               SecureResNet18, image_requests, largest_batch_that_fits, party_context, run_three_role,
                               serving_bytes)
from tests.secure_batch_nets import MINI_BLOCKS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_secure_form_golden", os.path.join(GOLDEN, "make_secure_form_golden.py"))
G = importlib.util.module_from_spec(_spec)      # the grid and its walk: the generator's own
_spec.loader.exec_module(G)

OPTIONS = ("pooling", "reveal", "fss_bits", "wide_norm", "faithful_trunc")
SCHEDULE_FUNCTIONS = (image_requests, serving_bytes, largest_batch_that_fits)
ENTRY_POINTS = (image_requests, serving_bytes, largest_batch_that_fits, SecureResNet18, GraphedSecureInference,
                PipelinedSecureInference, party_context, run_three_role)


# ---- a. nothing moved -------------------------------------------------------------------------------------------------------
def test_schedules_and_refusals_equal_the_commit_before_the_form():
    """All 384 combinations of the grid, entry by entry: the SHA-256 of the request list, serving_bytes, largest_batch_that_fits
    at the two budgets, or the type and text of the refusal.  160 are accepted: a form that refused everything would not pass."""
    with open(os.path.join(GOLDEN, "secure_form_schedules.json")) as f:
        want = json.load(f)
    got = G.table()
    assert len(want) == 384 and sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    assert sum("error" not in v for v in got.values()) == 160


# ---- b. the form itself -----------------------------------------------------------------------------------------------------
def test_form_is_frozen_and_normalised():
    f = ProtocolForm()
    assert dataclasses.astuple(f) == ("max", "logits", secure.FSS_BITS, False, False)
    assert tuple(x.name for x in dataclasses.fields(f)) == OPTIONS
    with pytest.raises(dataclasses.FrozenInstanceError):
        f.pooling = "avg"
    g = ProtocolForm(fss_bits="48", wide_norm=1, faithful_trunc=0)
    assert (g.fss_bits, g.wide_norm, g.faithful_trunc) == (48, True, False) and type(g.wide_norm) is bool is type(g.faithful_trunc)
    assert g == ProtocolForm(fss_bits=48, wide_norm=True) and hash(g) == hash(ProtocolForm(fss_bits=48, wide_norm=True))


def test_of():
    f = ProtocolForm(reveal="class")
    assert ProtocolForm.of(f) is f
    assert ProtocolForm.of() == ProtocolForm() and ProtocolForm.of(None, reveal="class") == f
    with pytest.raises(TypeError):
        ProtocolForm.of(f, reveal="class")
    with pytest.raises(TypeError):
        ProtocolForm.of(poolin="avg")
    with pytest.raises(TypeError):
        ProtocolForm(blocks=None)


@pytest.mark.parametrize("option,value,message", [
    ("pooling", "mean", f"pooling must be one of {POOLINGS}, got 'mean'"),
    ("reveal", "scores", f"reveal must be one of {EVALUATION_REVEALS}, got 'scores'"),
    ("fss_bits", 31, "fss_bits must be in [32, 64], got 31"),
    ("fss_bits", 65, "fss_bits must be in [32, 64], got 65"),
])
def test_bad_values_raise_the_messages_of_old(option, value, message):
    for build in (ProtocolForm, ProtocolForm.of):
        with pytest.raises(ValueError) as e:
            build(**{option: value})
        assert str(e.value) == message


def test_check_makes_the_refusals_that_depend_on_the_network():
    def refusal(fn, *args):
        with pytest.raises(ValueError) as e:
            fn(*args)
        return str(e.value)

    ProtocolForm().check("batch")
    wide, faithful = ProtocolForm(wide_norm=True), ProtocolForm(faithful_trunc=True)
    wide.check("group")
    for norm in ("batch", "folded"):      # the very text of check_wide_norm, with and without a precision
        assert refusal(wide.check, norm) == refusal(wide.check, norm, 10, 3) == refusal(secure.check_wide_norm, 10, 3, norm)
        assert refusal(wide.check, norm).startswith("wide_norm is a form of the secret-shared GroupNorm")
    faithful.check("folded")
    for norm in ("batch", "group"):
        assert refusal(faithful.check, norm, 10, 3) == refusal(faithful.check, norm) == refusal(secure.check_faithful_trunc, norm)
        assert refusal(faithful.check, norm).startswith("faithful_trunc covers the products of a folded network")
    for pf in (2, 7):      # the precision is refused only where one is given
        wide.check("group")
        assert refusal(wide.check, "group", 10, pf) == refusal(secure.check_wide_norm, 10, pf)
        assert refusal(wide.check, "group", 10, pf).startswith("wide_norm is defined for base 10 and 3 <= precision_fractional <= 6")
    for pf in (3, 6):
        wide.check("group", 10, pf)
    assert refusal(wide.check, "group", 2, 4).startswith("wide_norm is defined for base 10")
    with pytest.raises(ValueError, match="wide_norm is a form"):      # both flags: the wide form's refusal comes first, as before
        ProtocolForm(wide_norm=True, faithful_trunc=True).check("folded")


# ---- c. every entry point ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRY_POINTS, ids=lambda e: e.__name__)
def test_entry_point_takes_the_form_or_its_fields_by_keyword_only(entry):
    """No option name is a parameter -- but `pooling`, which the three schedule functions still take as their fifth positional
    argument, the way existing callers pass it; `form` is keyword-only and the rest of the keywords are collected for
    ProtocolForm.of; one positional argument more (for every schedule function: a sixth) does not bind."""
    sig = inspect.signature(entry)
    params = sig.parameters
    assert set(OPTIONS) & set(params) == ({"pooling"} if entry in SCHEDULE_FUNCTIONS else set())
    assert params["form"].kind is inspect.Parameter.KEYWORD_ONLY and params["form"].default is None
    assert [p.kind for p in params.values()][-1] is inspect.Parameter.VAR_KEYWORD
    positional = [p for p in params.values() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert not any(p.kind is inspect.Parameter.VAR_POSITIONAL for p in params.values())
    fill = [None] * len(positional)
    sig.bind(*fill, form=None)
    if entry in SCHEDULE_FUNCTIONS:
        assert len(fill) == 5 and positional[-1].name == "pooling" and positional[-1].default is ...
        fill = fill[:-1]
    for name in OPTIONS:
        bound = sig.bind(*fill, **{name: "x"}).arguments
        assert bound.get(name) == "x" or bound[list(params)[-1]] == {name: "x"}
    sig.bind(*fill, **dict.fromkeys(OPTIONS))
    fill = [None] * len(positional)
    with pytest.raises(TypeError):
        sig.bind(*fill, None)
    with pytest.raises(TypeError):      # (a sixth positional argument, where fewer than six parameters are no options)
        sig.bind(*[None] * max(6, len(fill) + 1))


def test_positional_parameters_keep_their_names_and_order():
    names = lambda fn: [p.name for p in inspect.signature(fn).parameters.values()
                        if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert names(image_requests) == ["arch", "input_size", "batch", "blocks", "pooling"] == names(serving_bytes)
    assert names(largest_batch_that_fits) == ["arch", "input_size", "budget", "blocks", "pooling"]
    assert names(SecureResNet18) == ["ctx", "state_dict", "input_size", "blocks", "batched_newton"]
    assert names(GraphedSecureInference) == ["state_dict", "device", "input_size", "precision_fractional", "base", "seed", "blocks",
                                             "batch", "memory_budget"]
    assert names(PipelinedSecureInference) == ["state_dict", "device", "input_size", "precision_fractional", "base", "seed",
                                               "blocks", "slots", "batch"]
    assert names(party_context) == ["link", "precision_fractional", "base"]
    assert names(run_three_role) == ["link", "arch", "input_size", "n_images", "state_dict", "images", "seed", "blocks",
                                     "precision_fractional", "base", "batch"]
    # what followed an option stays reachable by its name
    assert "norm" in inspect.signature(SecureResNet18).parameters and "labels" in inspect.signature(run_three_role).parameters


SPELLINGS = [("group", dict(wide_norm=True)), ("folded", dict(faithful_trunc=True)), ("batch", dict(pooling="avg", reveal="class")),
             ("batch", dict(reveal="metrics", fss_bits=64)), ("group", dict())]


@pytest.mark.parametrize("norm,options", SPELLINGS, ids=lambda v: v if isinstance(v, str) else ",".join(v) or "default")
def test_schedule_functions_mean_the_same_by_form_and_by_keyword(norm, options):
    arch, form = G.architectures()[norm], ProtocolForm(**options)
    listed = {k: v for k, v in options.items() if k != "fss_bits"}
    assert image_requests(arch, 32, 3, MINI_BLOCKS, form=form) == image_requests(arch, 32, 3, MINI_BLOCKS, **listed)
    assert image_requests(arch, 32, 3, MINI_BLOCKS, form=form) == image_requests(arch, 32, 3, MINI_BLOCKS, **options)      # the width is ignored
    assert serving_bytes(arch, 32, 3, MINI_BLOCKS, form=form) == serving_bytes(arch, 32, 3, MINI_BLOCKS, **options)
    budget = serving_bytes(arch, 32, 2, MINI_BLOCKS, form=form)
    for b in (budget, budget - 1):
        assert largest_batch_that_fits(arch, 32, b, MINI_BLOCKS, form=form) == largest_batch_that_fits(arch, 32, b, MINI_BLOCKS, **options)
    for fn, third in ((image_requests, 3), (serving_bytes, 3), (largest_batch_that_fits, budget)):
        with pytest.raises(TypeError):
            fn(arch, 32, third, MINI_BLOCKS, form=form, reveal="logits")
        want = fn(arch, 32, third, MINI_BLOCKS, form=dataclasses.replace(form, pooling="avg"))
        rest = {k: v for k, v in options.items() if k != "pooling"}
        assert fn(arch, 32, third, MINI_BLOCKS, "avg", **rest) == want == fn(arch, 32, third, MINI_BLOCKS, pooling="avg", **rest)
        with pytest.raises(TypeError):      # the fifth positional argument is the stem pool, and the last
            fn(arch, 32, third, MINI_BLOCKS, "max", "logits")
        with pytest.raises(TypeError):
            fn(arch, 32, third, MINI_BLOCKS, "max", form=form)


class _NoDevice:
    """What SecureResNet18 reads of a context before it shares anything."""
    base, pf, faithful_trunc = 10, 3, False


def test_model_refuses_through_the_form_before_it_touches_the_device():
    """SecureResNet18 resolves and checks its form first: the refusals of old, with the context's precision, on a context
    that has no dealer at all."""
    gn = {k: torch.empty(s) for k, s in G.architectures()["group"].items()}
    with pytest.raises(TypeError):
        SecureResNet18(_NoDevice(), gn, 32, MINI_BLOCKS, form=ProtocolForm(), wide_norm=True)
    with pytest.raises(ValueError, match="faithful_trunc covers the products of a folded network"):
        SecureResNet18(_NoDevice(), gn, 32, MINI_BLOCKS, form=ProtocolForm(faithful_trunc=True))
    ctx = _NoDevice()
    ctx.pf = 7
    with pytest.raises(ValueError, match="wide_norm is defined for base 10"):
        SecureResNet18(ctx, gn, 32, MINI_BLOCKS, wide_norm=True)
    ctx = _NoDevice()
    ctx.faithful_trunc = True      # a faithful context makes the model's form faithful: refused on a GroupNorm network
    with pytest.raises(ValueError, match="faithful_trunc covers"):
        SecureResNet18(ctx, gn, 32, MINI_BLOCKS)
