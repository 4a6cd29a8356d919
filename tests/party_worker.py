"""One rank of a three-role encrypted-inference test (launched by tests/secure_common.py's three_role_logits through
torch.distributed.run, 3 ranks sharing GPU 0 over gloo): `out case pf seed`, the case one of secure_common.THREE_ROLE_CASES.
Writes each party's decoded logits."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from primia_amd.secure import PartyLink, architecture_of, run_three_role  # noqa: E402
from tests.secure_common import THREE_ROLE_CASES, three_role_case  # noqa: E402

if __name__ == "__main__":
    out_path, case, pf, seed = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    device = torch.device("cuda:0")
    dist.init_process_group("gloo")
    sd, images, blocks, size, batch, pooling = three_role_case(case)
    link = PartyLink(device)
    res = run_three_role(link, architecture_of(sd), size, len(images), state_dict=sd if link.role == 0 else None,
                         images=images.to(device) if link.role == 1 else None, seed=seed, blocks=blocks,
                         precision_fractional=pf, batch=batch, pooling=pooling)
    if link.role in (0, 1):
        assert [tuple(r.shape) for r in res] == THREE_ROLE_CASES[case][-1]
        torch.save(torch.cat(res).cpu(), f"{out_path}.{link.role}")
    dist.barrier()
    dist.destroy_process_group()
