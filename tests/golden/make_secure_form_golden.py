"""Mint tests/golden/secure_form_schedules.json: what the host-side schedule functions of encrypted inference answer for every
combination of the options the three roles agree on.

    python tests/golden/make_secure_form_golden.py

No GPU is needed.  The grid is norm {batch, group, folded} (the mini network at 32 x 32) x pooling x reveal x batch {1, 3} x
wide_norm x faithful_trunc x fss_bits {32, 64}: 384 combinations.  An accepted one records the SHA-256 of
repr(image_requests(...)), serving_bytes(...) and largest_batch_that_fits(...) at the budgets serving_bytes(batch=2) and one
byte less; a refused one the exception's type and message.  Every option is named by keyword.  The file was minted ONCE, on
the commit BEFORE the options moved into primia_amd.secure.ProtocolForm; tests/test_secure_form_host.py imports `table()` from
here and holds the code to it.  Mint it again only when a schedule or a refusal changes on purpose, and say so in that commit.
"""
import hashlib
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
OUT = os.path.join(HERE, "secure_form_schedules.json")

SIZE = 32
BATCHES = (1, 3)
FSS_WIDTHS = (32, 64)


def architectures():
    """norm -> (name -> shape) of the mini network in its three forms."""
    import torch

    from primia_amd.secure import architecture_of, folded_architecture
    from tests.secure_batch_nets import mini_resnet
    from tests.secure_groupnorm_nets import group_mini

    batch = architecture_of(mini_resnet(torch.Generator().manual_seed(21)))
    return {"batch": batch, "group": architecture_of(group_mini(torch.Generator().manual_seed(71))),
            "folded": folded_architecture(batch)}


def entry(arch, blocks, batch, **options):
    """What the three schedule functions answer for one combination, or the refusal."""
    from primia_amd.secure import image_requests, largest_batch_that_fits, serving_bytes

    try:
        requests = image_requests(arch, SIZE, batch, blocks, **{k: v for k, v in options.items() if k != "fss_bits"})
        budget = serving_bytes(arch, SIZE, 2, blocks, **options)
        return {"requests": hashlib.sha256(repr(requests).encode()).hexdigest(),
                "bytes": serving_bytes(arch, SIZE, batch, blocks, **options),
                "fits": [largest_batch_that_fits(arch, SIZE, budget, blocks, **options),
                         largest_batch_that_fits(arch, SIZE, budget - 1, blocks, **options)]}
    except Exception as e:      # a refusal: its type and text are part of the contract
        return {"error": [type(e).__name__, str(e)]}


def table():
    """"norm|pooling|reveal|batch|wide_norm|faithful_trunc|fss_bits" -> entry, over the whole grid."""
    from primia_amd.secure import EVALUATION_REVEALS, POOLINGS
    from tests.secure_batch_nets import MINI_BLOCKS

    archs, out = architectures(), {}
    for norm, pooling, reveal, batch, wide, faithful, bits in itertools.product(
            archs, POOLINGS, EVALUATION_REVEALS, BATCHES, (False, True), (False, True), FSS_WIDTHS):
        key = f"{norm}|{pooling}|{reveal}|{batch}|{int(wide)}|{int(faithful)}|{bits}"
        out[key] = entry(archs[norm], MINI_BLOCKS, batch, pooling=pooling, reveal=reveal, wide_norm=wide,
                         faithful_trunc=faithful, fss_bits=bits)
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    values = table()
    with open(OUT, "w") as f:
        json.dump(values, f, indent=0, sort_keys=True)
        f.write("\n")
    accepted = sum("error" not in v for v in values.values())
    print(f"{OUT}: {len(values)} combinations, {accepted} accepted, {os.path.getsize(OUT)} bytes")
