"""The cases of the three-role tests of encrypted inference, by name: everything the model owner, the data owner, the crypto
provider -- three processes, tests/party_worker.py -- and the test that starts them must agree on.  Every process builds the
same tensors from the same seeds.  A module of helpers, not of tests."""
from collections import namedtuple

import torch

from tests.secure_batch_nets import MINI_BLOCKS, mini_resnet, resnet18
from tests.secure_folded_nets import wide_mini
from tests.secure_groupnorm_nets import group_mini, group_resnet18

THREE_RANK_BATCH = 3      # four images at three per pass: the second pass is padded with two all-zero images
AUC_LABELS = [0, 1, 2, 1]      # of the four images of network_case: every class is labelled, so the score is defined


# norm -> the 8-block network at 32 x 32 and four images whose float64 plaintext classes differ, each with a margin between
# its two largest logits of more than twice the project's bound on pf = 3 logits (batch: classes 0, 2, 2, 0 with margins 0.19,
# 0.69, 0.14, 1.44 against 2 x 0.05; group: 0, 2, 0, 0 with 0.15, 0.22, 0.14, 0.11 against 2 x 0.0124), so that the secure
# passes see two classes as well.  (The BatchNorm networks of this initialisation barely look at a unit-variance image: two
# of the four are scaled by 3.)
def network_case(norm):
    if norm == "batch":
        images = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(522))
        return resnet18(32, 333), images * torch.tensor([1.0, 3.0, 1.0, 3.0]).view(4, 1, 1, 1)
    return group_resnet18(32, 520), torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(521))


def wide_net():
    """The 8-block network at 32 x 32 and two images, one scaled by 3, of the tests of comparisons wider than 32 bits."""
    sd = resnet18(32, 320)
    images = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(321)) * torch.tensor([1.0, 3.0]).view(2, 1, 1, 1)
    return sd, images


def drawn(net, seed, n, size):
    """A network and then n images of size x size, drawn from ONE generator seeded with `seed`."""
    def tensors():
        gen = torch.Generator().manual_seed(seed)
        sd = net(gen)
        return sd, torch.randn(n, 3, size, size, generator=gen)

    return tensors


def confusion_labels(norm):
    """The labels tests/secure_confusion_nets.py chooses from the float64 plaintext classes of network_case(norm)."""
    def labels(sd, images, pf):
        from tests.secure_confusion_nets import chosen_labels, plaintext_classes

        return torch.from_numpy(chosen_labels(plaintext_classes(norm, sd, images, pf)))

    return labels


def auc_labels(sd, images, pf):
    return torch.tensor(AUC_LABELS, dtype=torch.int64)


# tensors: () -> (checkpoint, images); blocks None: the eight of a ResNet-18; fold: the model owner folds the BatchNorm sites
# before sharing; labels: (checkpoint, images, pf) -> the data owner's int64 labels, or None; shapes: of what a party that
# holds a result holds -- logits and classes per pass, the opened matrix, the matrix and the rank counts; pooling, reveal,
# fss_bits, wide_norm, faithful_trunc: the fields of the ProtocolForm the three roles run under (Case.form)
class Case(namedtuple("Case", "tensors size blocks batch pooling reveal fss_bits fold labels shapes wide_norm faithful_trunc")):
    def form(self):
        from primia_amd.secure import ProtocolForm

        return ProtocolForm(pooling=self.pooling, reveal=self.reveal, fss_bits=self.fss_bits, wide_norm=self.wide_norm,
                            faithful_trunc=self.faithful_trunc)


def logits_case(tensors, size, blocks, batch, shapes, pooling="max", fss_bits=32, fold=False, wide_norm=False,
                faithful_trunc=False):
    return Case(tensors, size, blocks, batch, pooling, "logits", fss_bits, fold, None, shapes, wide_norm, faithful_trunc)


def reveal_case(norm, reveal, labels, shapes):
    return Case(lambda: network_case(norm), 32, None, THREE_RANK_BATCH, "max", reveal, 32, False, labels, shapes, False, False)


def gn_wide_net():
    """The mini GroupNorm network whose group variances spread over four decades, and its three images (the wide-range
    GroupNorm's whole-network case)."""
    from tests import secure_gn_wide_nets as W

    return W.wide_networks()["mini"][0], W.spread_images()


# three images at two per pass pad the second pass
CASES = {
    "mini": logits_case(drawn(mini_resnet, 21, 2, 16), 16, MINI_BLOCKS, 1, [(1, 3), (1, 3)]),
    "batch": logits_case(drawn(mini_resnet, 61, 3, 32), 32, MINI_BLOCKS, 2, [(2, 3), (1, 3)]),
    "avg": logits_case(drawn(mini_resnet, 61, 3, 32), 32, MINI_BLOCKS, 2, [(2, 3), (1, 3)], pooling="avg"),
    "group": logits_case(drawn(group_mini, 71, 3, 32), 32, MINI_BLOCKS, 2, [(2, 3), (1, 3)]),
    "folded": logits_case(drawn(wide_mini, 81, 3, 32), 32, MINI_BLOCKS, 2, [(2, 3), (1, 3)], fold=True),
    "wide": logits_case(wide_net, 32, None, 2, [(2, 3)], fss_bits=64),
    "gn-wide": logits_case(gn_wide_net, 32, MINI_BLOCKS, 2, [(2, 3), (1, 3)], wide_norm=True),
}
CASES["faithful"] = CASES["folded"]._replace(faithful_trunc=True)      # the folded case's tensors, truncated faithfully
for _norm in ("batch", "group"):
    CASES[f"class-{_norm}"] = reveal_case(_norm, "class", None, [(3,), (1,)])
    CASES[f"confusion-{_norm}"] = reveal_case(_norm, "confusion", confusion_labels(_norm), [(3, 3)])
    CASES[f"metrics-{_norm}"] = reveal_case(_norm, "metrics", auc_labels, [(3, 3), (3, 3, 3)])
