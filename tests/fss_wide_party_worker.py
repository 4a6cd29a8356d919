"""One rank of the three-role test of wide comparisons (launched by tests/test_gpu_secure_wide.py through
torch.distributed.run, 3 ranks sharing GPU 0 over gloo): `out pf seed fss_bits`, on that module's network and images.  Writes
each party's decoded logits."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from primia_amd.secure import PartyLink, architecture_of, run_three_role  # noqa: E402
from tests.test_gpu_secure_wide import net  # noqa: E402

if __name__ == "__main__":
    out_path, pf, seed, bits = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    device = torch.device("cuda:0")
    dist.init_process_group("gloo")
    sd, images = net()
    link = PartyLink(device)
    res = run_three_role(link, architecture_of(sd), 32, len(images), state_dict=sd if link.role == 0 else None,
                         images=images.to(device) if link.role == 1 else None, seed=seed, precision_fractional=pf,
                         batch=len(images), fss_bits=bits)
    if link.role in (0, 1):
        assert [tuple(r.shape) for r in res] == [(len(images), 3)]
        torch.save(torch.cat(res).cpu(), f"{out_path}.{link.role}")
    dist.barrier()
    dist.destroy_process_group()
