"""One role of the three-role test of the faithful truncation (tests/test_gpu_secure_faithful.py, started through
tests/secure_common.py's run_roles, one process per role, all on GPU 0 over gloo): `out pf seed batch`.  The network and the
images are tests/three_role_cases.py's folded case; the model owner alone holds the weights and folds them, the data owner
alone holds the images, the other two know the folded architecture.  Each party writes its decoded logits to `out.<role>`;
the crypto provider holds nothing."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from primia_amd.secure import PartyLink, architecture_of, fold_batch_norm, folded_architecture, run_three_role  # noqa: E402
from tests.three_role_cases import CASES  # noqa: E402

if __name__ == "__main__":
    out_path, pf, seed, batch = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    device = torch.device("cuda:0")
    dist.init_process_group("gloo")
    case = CASES["folded"]
    sd, images = case.tensors()
    link = PartyLink(device)
    res = run_three_role(link, folded_architecture(architecture_of(sd)), case.size, len(images),
                         state_dict=fold_batch_norm(sd) if link.role == 0 else None,
                         images=images.to(device) if link.role == 1 else None, seed=seed, blocks=case.blocks,
                         precision_fractional=pf, batch=batch, faithful_trunc=True)
    if link.role in (0, 1):
        assert [tuple(t.shape) for t in res] == [(2, 3), (1, 3)]
        torch.save(torch.cat(res).cpu(), f"{out_path}.{link.role}")
    else:
        assert res is None
    dist.barrier()
    dist.destroy_process_group()
