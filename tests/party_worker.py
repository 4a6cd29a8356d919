"""One role of a three-role encrypted-inference test (started by tests/secure_common.py's run_three_roles, one process per role,
all on GPU 0 over gloo; RANK, WORLD_SIZE, MASTER_ADDR and MASTER_PORT come from the parent): `out case pf seed`, the case one
of tests/three_role_cases.py's CASES.  The model owner alone holds (and folds) the weights, the data owner alone the images and
the labels.  A role that holds a result checks its shapes and dtypes and writes it to `out.<role>`; every other role must
hold nothing, and writes nothing."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from primia_amd.secure import (PartyLink, architecture_of, fold_batch_norm, folded_architecture,  # noqa: E402
                               run_three_role)
from tests.three_role_cases import CASES  # noqa: E402

if __name__ == "__main__":
    out_path, case, pf, seed = sys.argv[1], CASES[sys.argv[2]], int(sys.argv[3]), int(sys.argv[4])
    device = torch.device("cuda:0")
    dist.init_process_group("gloo")
    sd, images = case.tensors()
    link = PartyLink(device)
    arch = architecture_of(sd)
    if case.fold:      # the data owner and the crypto provider fold the architecture alone: they never see a weight
        arch = folded_architecture(arch)
        if link.role == 0:
            sd = fold_batch_norm(sd)
    labels = None
    if case.labels and link.role == 1:      # the data owner alone knows the labels
        labels = case.labels(sd, images, pf)
    res = run_three_role(link, arch, case.size, len(images), state_dict=sd if link.role == 0 else None,
                         images=images.to(device) if link.role == 1 else None, seed=seed, blocks=case.blocks,
                         precision_fractional=pf, batch=case.batch, labels=labels, form=case.form())
    if link.role in ((1,) if case.reveal == "class" else (0, 1)):
        held = [res] if case.reveal == "confusion" else list(res)
        assert [tuple(t.shape) for t in held] == case.shapes
        assert case.reveal == "logits" or all(t.dtype == torch.int64 for t in held)
        if case.reveal in ("logits", "class"):      # one tensor per pass
            saved = torch.cat(held).cpu()
        else:      # the matrix; the matrix and the rank counts
            saved = res.cpu() if case.reveal == "confusion" else tuple(t.cpu() for t in res)
        torch.save(saved, f"{out_path}.{link.role}")
    else:
        assert res is None
    dist.barrier()
    dist.destroy_process_group()
