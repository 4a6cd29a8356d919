"""One rank of the three-role test of a folded BatchNorm network (launched by tests/test_gpu_secure_folded.py through
torch.distributed.run, 3 ranks sharing GPU 0 over gloo): `out pf seed`.  Rank 0, the model owner, folds the weights
(fold_batch_norm); the data owner and the crypto provider fold the architecture alone (folded_architecture) -- they never see
a weight.  Writes each party's decoded logits."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from primia_amd.secure import PartyLink, architecture_of, fold_batch_norm, folded_architecture, run_three_role  # noqa: E402
from tests.secure_folded_nets import three_role_case  # noqa: E402

if __name__ == "__main__":
    out_path, pf, seed = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    device = torch.device("cuda:0")
    dist.init_process_group("gloo")
    sd, images, blocks, size, batch = three_role_case()
    link = PartyLink(device)
    arch = folded_architecture(architecture_of(sd))
    res = run_three_role(link, arch, size, len(images), state_dict=fold_batch_norm(sd) if link.role == 0 else None,
                         images=images.to(device) if link.role == 1 else None, seed=seed, blocks=blocks,
                         precision_fractional=pf, batch=batch)
    if link.role in (0, 1):
        assert [tuple(r.shape) for r in res] == [(2, 3), (1, 3)]
        torch.save(torch.cat(res).cpu(), f"{out_path}.{link.role}")
    dist.barrier()
    dist.destroy_process_group()
