"""CPU: what `inference.py --evaluate` prints is derived from the confusion matrix alone -- the report and the MCC against
scikit-learn's, the ROC AUC of the logits form against the plaintext test()'s recipe, the class-folder listing -- and the
serving form that cannot hold one accumulator refuses reveal="confusion" (no device is touched)."""
import numpy as np
import pytest
import torch
from sklearn import metrics as mt

import inference
from primia_amd.secure import PipelinedSecureInference
from primia_amd.torchlib_compat import confusion_mcc, confusion_report, matthews_corrcoef, stats_table

# labels / predictions over 4 classes: class 3 never occurs as a label (an empty row), class 1 is never predicted (an empty
# column), class 2 is always right
Y_TRUE = [0, 0, 0, 1, 1, 2, 2, 2, 0, 1]
Y_PRED = [0, 2, 3, 0, 3, 2, 2, 2, 0, 2]


def test_confusion_report_is_sklearns_classification_report():
    labels = list(range(4))
    cm = mt.confusion_matrix(Y_TRUE, Y_PRED, labels=labels)
    assert cm[3].sum() == 0 and cm[:, 1].sum() == 0
    want = mt.classification_report(Y_TRUE, Y_PRED, labels=labels, output_dict=True, zero_division=0)
    got = confusion_report(cm)
    for key in ["0", "1", "2", "3", "macro avg", "weighted avg"]:
        assert set(got[key]) == {"precision", "recall", "f1-score", "support"}
        for field in got[key]:
            assert got[key][field] == pytest.approx(want[key][field], abs=1e-12), (key, field)
    assert got["accuracy"] == pytest.approx(mt.accuracy_score(Y_TRUE, Y_PRED), abs=1e-12)
    assert all(isinstance(got[str(i)]["support"], int) for i in labels)
    # an all-zero matrix (nothing evaluated) divides by nothing
    empty = confusion_report(np.zeros((3, 3), np.int64))
    assert empty["accuracy"] == 0.0 and empty["macro avg"]["f1-score"] == 0.0 and empty["weighted avg"]["support"] == 0
    table = stats_table(cm, got, roc_auc=None, matthews_coeff=confusion_mcc(cm))
    assert "n/a" in table and "matthews coeff" in table
    assert "0.500" in stats_table(cm, got, roc_auc=0.5, matthews_coeff=confusion_mcc(cm))


def test_confusion_mcc_is_sklearns_mcc():
    cm = mt.confusion_matrix(Y_TRUE, Y_PRED, labels=list(range(4)))
    want = mt.matthews_corrcoef(Y_TRUE, Y_PRED)
    assert confusion_mcc(cm) == pytest.approx(want, abs=1e-12)
    assert confusion_mcc(cm) == matthews_corrcoef(Y_TRUE, Y_PRED, 4)      # (the existing function, now through the matrix)
    assert confusion_mcc(np.diag([3, 2, 4])) == pytest.approx(1.0)
    assert confusion_mcc(np.array([[5, 0], [3, 0]])) == 0.0               # one predicted class: the denominator vanishes
    assert confusion_mcc(np.zeros((3, 3), np.int64)) == 0.0


def test_confusion_of_counts_pairs():
    m = inference.confusion_of(torch.tensor(Y_TRUE), Y_PRED, 4)
    assert m.dtype == torch.int64 and np.array_equal(m.numpy(), mt.confusion_matrix(Y_TRUE, Y_PRED, labels=list(range(4))))


def test_roc_auc_of_follows_the_plaintext_recipe():
    """One-vs-one ROC AUC on the min-shifted, row-normalised logits, as torchlib_compat.test computes it; two classes take the
    score of class 1; a label set with one class only gives 0 and a warning on stderr."""
    gen = torch.Generator().manual_seed(4)
    labels = torch.tensor([0, 1, 2, 0, 1, 2, 1, 0])
    logits = torch.randn(8, 3, generator=gen) + 2 * torch.nn.functional.one_hot(labels, 3)
    s = logits.double().numpy().copy()
    s -= s.min(axis=1)[:, None]
    s /= s.sum(axis=1)[:, None]
    assert inference.roc_auc_of(labels, logits) == pytest.approx(mt.roc_auc_score(labels.numpy(), s, multi_class="ovo"), abs=1e-12)
    two = torch.tensor([[2.0, 0.0], [0.0, 1.0], [0.5, 0.4], [0.0, 3.0]])
    assert inference.roc_auc_of(torch.tensor([0, 1, 0, 1]), two) == 1.0
    assert inference.roc_auc_of(torch.tensor([1, 1, 1, 1]), two) == 0.0


def test_labelled_files_lists_a_class_folder_tree(tmp_path):
    """<dir>/<class>/<image>, listed like the validation folder: classes are the sorted folder names, files sorted per class;
    n picks evenly over the listing; more class folders than the checkpoint has classes, an empty tree and a missing folder
    are refused."""
    for name, count in (("b_bacterial", 3), ("a_normal", 2), ("c_viral", 1)):
        (tmp_path / name).mkdir()
        for i in range(count):
            (tmp_path / name / f"img{i}.png").write_bytes(b"")
    (tmp_path / "a_normal" / "notes.txt").write_text("not an image")
    files, labels, names = inference.labelled_files(str(tmp_path), None, 3)
    assert names == ["a_normal", "b_bacterial", "c_viral"]
    assert labels.dtype == torch.int64 and labels.tolist() == [0, 0, 1, 1, 1, 2]
    assert [f[len(str(tmp_path)) + 1:] for f in files] == ["a_normal/img0.png", "a_normal/img1.png", "b_bacterial/img0.png",
                                                           "b_bacterial/img1.png", "b_bacterial/img2.png", "c_viral/img0.png"]
    files3, labels3, _ = inference.labelled_files(str(tmp_path), 3, 3)
    assert labels3.tolist() == [0, 1, 1] and files3 == [files[0], files[2], files[4]]
    assert inference.labelled_files(str(tmp_path), 100, 4)[1].tolist() == labels.tolist()
    with pytest.raises(SystemExit, match="class folders"):
        inference.labelled_files(str(tmp_path), None, 2)
    (tmp_path / "empty" / "x").mkdir(parents=True)
    with pytest.raises(SystemExit, match="no images"):
        inference.labelled_files(str(tmp_path / "empty"), None, 3)
    with pytest.raises(SystemExit, match="does not exist"):
        inference.labelled_files(str(tmp_path / "missing"), None, 3)


def test_synthetic_labels_are_seeded():
    a, b = inference.synthetic_labels(16, 3), inference.synthetic_labels(16, 3)
    assert a.dtype == torch.int64 and torch.equal(a, b) and set(a.tolist()) == {0, 1, 2}


def test_pipelined_form_refuses_confusion():
    """Two slots would hold two accumulators: the pipelined form says so before it touches a device."""
    with pytest.raises(ValueError, match="confusion"):
        PipelinedSecureInference({}, "cpu", reveal="confusion")
