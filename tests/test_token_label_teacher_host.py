"""Host logic of the teacher's token labels without a GPU: the tie rule of the tests' reference (tests/_topk_ref.py) against a brute-force
sort, and what TeacherLabeler, AutoProgDriver(teacher=...) and SparseTokenLabelTarget.from_logits refuse before anything is launched."""
import pytest
import torch

from tests._topk_ref import topk_ref


def _teacher(**kw):
    from autoprog_amd.models import create_model
    return create_model("model_variant", variant="volo_h2_l3", num_classes=24, img_size=64, stem_hidden_dim=64, **kw)


def _driver(**kw):
    from autoprog_amd.prog.driver import AutoProgDriver
    return AutoProgDriver(model=kw.pop("model", None), loss_fn=None, optimizer=None, reducer=None, get_batch=lambda r: None, r_list=[64, 96], l_list=[3, 6],
                          dp_list=[0.0, 0.0], grow_epochs=[0, 2], steps_per_epoch=1, **kw)


def test_reference_tie_rule_is_the_brute_force_order():
    """3 x 7 with planted ties (bf16): equal logits rank by ascending class index, -0 equals +0, -inf sorts last; the scores are the fp64
    softmax of inv_temp * x at those classes"""
    x = torch.tensor([[1.0, 3.0, 3.0, -2.0, 3.0, 1.0, 0.5],
                      [0.0, -0.0, 0.0, -1.0, 0.0, -0.0, -1.0],
                      [2.0, float("-inf"), 2.0, float("-inf"), 5.0, 2.0, 5.0]]).to(torch.bfloat16)
    idx, val = topk_ref(x, 7, inv_temp=0.5)
    for r in range(3):
        row = x[r].float().tolist()
        brute = sorted(range(7), key=lambda c: (-row[c], c))
        assert idx[r].tolist() == brute, (r, idx[r].tolist(), brute)
    assert idx[0].tolist() == [1, 2, 4, 0, 5, 6, 3] and idx[1].tolist() == [0, 1, 2, 4, 5, 3, 6] and idx[2].tolist() == [4, 6, 0, 2, 5, 1, 3]
    p = torch.softmax(0.5 * x.double(), dim=1)
    assert torch.equal(val, p.gather(1, idx)) and bool((val[:, 1:] <= val[:, :-1]).all()) and float(val[2, -1]) == 0.0


def test_labeler_refuses_a_teacher_without_an_aux_head():
    from autoprog_amd.prog.teacher import TeacherLabeler
    with pytest.raises(ValueError):
        TeacherLabeler(_teacher(return_dense=False, mix_token=False))
    with pytest.raises(ValueError):
        TeacherLabeler(torch.nn.Linear(4, 4))


def test_labeler_and_driver_refuse_a_class_count_mismatch():
    from autoprog_amd.prog.teacher import TeacherLabeler
    teacher = _teacher()
    with pytest.raises(ValueError):
        TeacherLabeler(teacher, num_classes=25)
    labeler = TeacherLabeler(teacher, num_classes=24)
    assert labeler.num_classes == 24 and not teacher.training
    student = torch.nn.Linear(4, 4)
    student.num_classes = 25
    with pytest.raises(ValueError):
        _driver(model=student, teacher=labeler)
    student.num_classes = 24
    assert _driver(model=student, teacher=labeler).teacher is labeler


def test_driver_refuses_a_teacher_beside_mixup_or_cutmix():
    from autoprog_amd.data import DeviceBatchPrep
    from autoprog_amd.prog.teacher import TeacherLabeler
    labeler = TeacherLabeler(_teacher())
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for kw in (dict(mixup_alpha=0.8), dict(cutmix_alpha=1.0)):
        with pytest.raises(ValueError):
            _driver(teacher=labeler, batch_prep=DeviceBatchPrep(mean, std, device="cpu", **kw))
    drv = _driver(teacher=labeler, batch_prep=DeviceBatchPrep(mean, std, device="cpu", re_prob=0.25))
    assert drv.teacher is labeler
    assert _driver().teacher is None                                 # the default: nothing changes


def test_k_beyond_eight_is_refused():
    from autoprog_amd.loss import SparseTokenLabelTarget
    from autoprog_amd.prog.teacher import TeacherLabeler
    with pytest.raises(ValueError):
        TeacherLabeler(_teacher(), k=9)
    labels, cls, aux = torch.zeros(2, dtype=torch.int64), torch.zeros(2, 16, dtype=torch.bfloat16), torch.zeros(2, 4, 16, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        SparseTokenLabelTarget.from_logits(labels, cls, aux, k=9)
    with pytest.raises(ValueError):
        SparseTokenLabelTarget.from_logits(labels, cls, aux, k=0)
