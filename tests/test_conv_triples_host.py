"""Host: convolution-shaped Beaver triples before anything touches a GPU -- the option on the ProtocolForm, the
request schedule and its bytes, and the refusals of the new entry points."""
import ctypes
import dataclasses

import pytest

from primia_amd import _lib, resnet_spec
from primia_amd.secure import ProtocolForm, architecture_of, image_requests, primitive_bytes


def test_the_option_is_a_field_of_the_form():
    on = ProtocolForm(conv_triples=True)
    assert on.conv_triples and not ProtocolForm().conv_triples and ProtocolForm(conv_triples=1) == on
    assert on != ProtocolForm() and hash(on) != hash(ProtocolForm()) and len({on, ProtocolForm(), ProtocolForm(conv_triples=True)}) == 2
    assert dataclasses.replace(on, pooling="avg").conv_triples and not dataclasses.replace(on, conv_triples=False).conv_triples
    assert "conv_triples=True" in repr(on) and "conv_triples" not in repr(ProtocolForm())
    assert [f.name for f in dataclasses.fields(on)] == ["pooling", "reveal", "fss_bits", "wide_norm", "faithful_trunc"]
    with pytest.raises(ValueError):
        ProtocolForm(conv_triples=True, pooling="sum")
    with pytest.raises(TypeError):
        ProtocolForm(conv_triple=True)


def test_schedule_and_bytes_at_224():
    """c and b keep their element counts, a goes from 14,689,024 to 2,182,656 words per image: 16 B x 12,506,368 less."""
    arch = architecture_of(resnet_spec.init_state_dict(resnet_spec.resnet18_spec(3, 3, 224, "max")))
    old, new = image_requests(arch, 224, 1), image_requests(arch, 224, 1, conv_triples=True)
    assert primitive_bytes(old) == 4_946_995_888 and primitive_bytes(new) == 4_746_894_000
    assert primitive_bytes(image_requests(arch, 224, 4)) == 19_087_620_928
    assert primitive_bytes(image_requests(arch, 224, 4, conv_triples=True)) == 18_287_213_376
    assert old == image_requests(arch, 224, 1, form=ProtocolForm()) and len(old) == len(new)
    changed = [(a, b) for a, b in zip(old, new) if a != b]
    assert len(changed) == 20 and all(a[1][0] == "matmul" and b[1][0] == "conv" for a, b in changed)
    assert changed[0][1] == ("triple", ("conv", (1, 3, 224, 224), (64, 3, 7, 7)), {"stride": 2, "padding": 3})
    assert changed[-1][1] == ("triple", ("conv", (1, 512, 7, 7), (512, 512, 3, 3)), {"stride": 1, "padding": 1})
    assert sum(x[0] * x[1] * x[2] * x[3] for x in (b[1][1] for _, b in changed)) == 2_182_656
    assert sum(a[1][1][1] * a[1][1][2] for a, _ in changed) == 14_689_024
    with pytest.raises(ValueError, match="no kernel for a 5 x 5 / stride 1"):      # refused on the host, before any launch
        image_requests({**arch, "layer1.0.conv1.weight": (64, 64, 5, 5)}, 224, 1, conv_triples=True)


GEOMETRY = {"B": 1, "C": 3, "H": 9, "W": 9, "O": 4, "R": 3, "S": 3, "stride": 1, "pad": 1}


@pytest.mark.parametrize("name", ["primia_ring_conv2d", "primia_beaver_combine_conv", "primia_beaver_conv_local",
                                  "primia_triple_conv_c1"])
def test_entry_point_is_declared_and_refuses_bad_arguments(name):
    protos, fn = _lib.protos(), getattr(_lib.lib(), name)
    buf = ctypes.create_string_buffer(256)
    ptr = lambda k: ctypes.c_void_p(ctypes.addressof(buf) + 8 * k)      # distinct, never dereferenced
    params = protos[name][1][:-1]
    names = [a for _, a in params]
    assert protos[name][0] is ctypes.c_int and protos[name][1][-1][1] == "stream"
    valid = [ptr(k) if t is ctypes.c_void_p else {**GEOMETRY, "div": 1000, "j": 0, "accumulate": 0}[a]
             for k, (t, a) in enumerate(params)]
    refused = lambda **change: fn(*[change.get(a, v) for a, v in zip(names, valid)], None)
    assert all(refused(**{a: None}) == -1 for t, a in params if t is ctypes.c_void_p)
    assert all(refused(**{a: 0}) == -1 for a in ("B", "C", "H", "W", "O", "R", "S", "stride"))
    assert refused(pad=-1) == -1 and refused(pad=3) == -1 and refused(H=1, W=1, pad=0) == -1
    assert refused(R=5, S=5) == -3 and refused(S=1) == -3 and refused(stride=3) == -3      # PRIMIA_ERR_UNSUPPORTED
    if name == "primia_beaver_combine_conv":
        assert refused(j=2) == -1
    if name == "primia_beaver_conv_local":
        assert refused(div=-1) == -1 and refused(div=2 ** 62) == -1
    split = _lib.lib().primia_ring_conv2d_split
    assert split(1, 160, 7, 7, 64, 3, 3, 1, 1, 1) > 1 and split(8, 64, 56, 56, 64, 3, 3, 1, 1, 2) == 1
    assert split(1, 0, 7, 7, 64, 3, 3, 1, 1, 1) == -1
