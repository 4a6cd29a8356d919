"""One role of the three-role test of an encrypted evaluation that opens the confusion matrix and the rank counts of the ROC
AUC (started by tests/test_gpu_secure_auc.py, one process per role, all on GPU 0 over gloo; RANK, WORLD_SIZE, MASTER_ADDR and
MASTER_PORT come from the parent): `out norm pf seed l0,l1,...`, the case tests/secure_argmax_nets.py's network_case(norm) with
the labels the parent names.  Both parties write the (M, U) they hold; the dealer must hold nothing."""
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
    labels = None
    if link.role == 1:      # the data owner alone knows the labels
        labels = torch.tensor([int(v) for v in sys.argv[5].split(",")], dtype=torch.int64)
    res = run_three_role(link, architecture_of(sd), 32, len(images), state_dict=sd if link.role == 0 else None,
                         images=images.to(device) if link.role == 1 else None, seed=seed, precision_fractional=pf,
                         batch=THREE_RANK_BATCH, reveal="metrics", labels=labels)
    if link.role == "dealer":
        assert res is None
    else:
        M, U = res
        assert M.dtype == U.dtype == torch.int64 and tuple(M.shape) == (3, 3) and tuple(U.shape) == (3, 3, 3)
        torch.save((M.cpu(), U.cpu()), f"{out_path}.{link.role}")
    dist.barrier()
    dist.destroy_process_group()
