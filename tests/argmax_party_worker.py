"""One rank of the three-rank test of encrypted inference that reveals the class only (launched by
tests/test_gpu_secure_argmax.py through torch.distributed.run, 3 ranks sharing GPU 0 over gloo): `out norm pf seed`, the case
tests/secure_argmax_nets.py's network_case(norm).  Party 1 writes the classes it learnt; party 0 must have learnt nothing."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from primia_amd.secure import PartyLink, architecture_of, run_three_role  # noqa: E402
from tests.secure_argmax_nets import THREE_RANK_BATCH, network_case  # noqa: E402

if __name__ == "__main__":
    out_path, norm, pf, seed = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    device = torch.device("cuda:0")
    dist.init_process_group("gloo")
    sd, images = network_case(norm)
    link = PartyLink(device)
    res = run_three_role(link, architecture_of(sd), 32, len(images), state_dict=sd if link.role == 0 else None,
                         images=images.to(device) if link.role == 1 else None, seed=seed, precision_fractional=pf,
                         batch=THREE_RANK_BATCH, reveal="class")
    if link.role == 1:
        assert [tuple(r.shape) for r in res] == [(3,), (1,)] and all(r.dtype == torch.int64 for r in res)
        torch.save(torch.cat(res).cpu(), f"{out_path}.1")
    else:
        assert res is None
    dist.barrier()
    dist.destroy_process_group()
