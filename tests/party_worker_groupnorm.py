"""One rank of the three-role encrypted-inference test of a GroupNorm network (launched by test_gpu_secure_groupnorm.py
through torch.distributed.run, 3 ranks sharing GPU 0 over gloo): three images, two per protocol pass, so the second pass is
padded.  Writes each party's decoded logits."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from primia_amd.secure import PartyLink, architecture_of, run_three_role  # noqa: E402
from tests.secure_groupnorm_nets import three_role_group_case  # noqa: E402

if __name__ == "__main__":
    out_path, pf, seed = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    device = torch.device("cuda:0")
    dist.init_process_group("gloo")
    sd, images, blocks = three_role_group_case()
    link = PartyLink(device)
    res = run_three_role(link, architecture_of(sd), 32, 3, state_dict=sd if link.role == 0 else None,
                         images=images.to(device) if link.role == 1 else None, seed=seed, blocks=blocks,
                         precision_fractional=pf, batch=2)
    if link.role in (0, 1):
        assert [tuple(r.shape) for r in res] == [(2, 3), (1, 3)]
        torch.save(torch.cat(res).cpu(), f"{out_path}.{link.role}")
    dist.barrier()
    dist.destroy_process_group()
