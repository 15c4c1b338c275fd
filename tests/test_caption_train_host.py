"""CPU: the host side of caption fine-tuning (lavender_amd/captioning.py: Agent_Captioning.masking, get_predict_file, the kept-row count of
CaptioningLoss) and the float64 loss reference of the GPU tests (tests/caption_loss_ref.py) against the fixtures recorded from the reference
(tests/golden/cap_train_micro.npz, written by tests/golden/make_goldens_caption_train.py).  No kernel is launched."""
import os

import numpy as np
import pytest
import torch

from tests import caption_loss_ref as CR


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cap_train_micro.npz"))


def test_masking_is_bit_identical_to_the_reference(golden):
    """one torch.rand(X) per row in row order; [PAD] and [MASK] are the only special tokens ([CLS] / [SEP] may be masked)"""
    from lavender_amd.captioning import masking
    n_cls_masked = 0
    for i, (B, X, seed, p) in enumerate(golden["mask_cases"]):
        txt = torch.from_numpy(golden[f"mask{i}_in"].copy())
        assert txt.shape == (int(B), int(X))
        torch.manual_seed(int(seed))
        r = masking(txt, float(p), pad_id=0, mask_id=103)
        assert set(r) == {"txt", "ans_mtm"}
        assert r["txt"] is txt                                             # masked in place, as the reference does
        assert np.array_equal(r["txt"].numpy(), golden[f"mask{i}_txt"])
        assert np.array_equal(r["ans_mtm"].numpy(), golden[f"mask{i}_ans"])
        assert r["ans_mtm"].dtype == torch.int64
        src = golden[f"mask{i}_in"]
        lab = r["ans_mtm"].numpy()
        assert not (lab[(src == 0) | (src == 103)] != -1).any()             # [PAD] / [MASK] never carry a label
        n_cls_masked += int(((src == 101) | (src == 102))[lab != -1].sum())
        if p == 0:
            assert (lab == -1).all() and np.array_equal(r["txt"].numpy(), src)
    assert n_cls_masked > 0, "the fixture should contain a masked [CLS] / [SEP] (the difference to the pre-training masking)"


def test_agent_masking_uses_the_agents_token_ids(golden):
    from lavender_amd.captioning import Agent_Captioning
    me = Agent_Captioning.__new__(Agent_Captioning)
    me.pad_token_id, me.mask_token_id = 0, 103
    txt = torch.from_numpy(golden["mask1_in"].copy())
    torch.manual_seed(int(golden["mask_cases"][1][2]))
    r = me.masking(txt, p_mask=float(golden["mask_cases"][1][3]))
    assert np.array_equal(r["ans_mtm"].numpy(), golden["mask1_ans"])


def test_float64_loss_reference_matches_the_reference_module(golden):
    """tests/caption_loss_ref.captioning_loss (closed form, selection by counting order) against model_for_captioning.CaptioningLoss
    (KLDivLoss + topk) on float64 logits, three calls per configuration so that drop_worst_after switches the selection on mid-way"""
    V, n = int(golden["meta"][0]), int(golden["meta"][1])
    for i, (eps, ratio, after) in enumerate(golden["loss_configs"]):
        for call, seed in enumerate(golden[f"loss{i}_seed"]):
            x, lab = CR.make_case(n, V, n, int(seed))
            drop = ratio > 0 and call + 1 > after
            r = CR.captioning_loss(x, lab, float(eps), float(ratio), drop=drop)
            assert r["n"] == n and r["k"] == (int(n * (1 - ratio)) if drop else n)
            g64, g32 = float(golden[f"loss{i}_f64"][call]), float(golden[f"loss{i}_f32"][call])
            print(f"eps {eps} ratio {ratio} after {after} call {call}: ref {r['loss']:.12f} golden f64 {g64:.12f} f32 {g32:.8f}")
            assert abs(r["loss"] - g64) < 1e-10 * max(1.0, abs(g64))
            assert abs(r["loss"] - g32) < 2e-5                             # the reference's own fp32 arithmetic over 30522 classes


def test_float64_gradient_is_the_derivative_of_the_loss():
    x, lab = CR.make_case(6, 97, 4, 3, sigma=0.5)
    for eps, ratio in ((0.0, 0.0), (0.1, 0.0), (0.1, 0.25)):
        r = CR.captioning_loss(x, lab, eps, ratio)
        xt = torch.from_numpy(x).double().requires_grad_(True)
        rl = CR.row_losses(xt, lab, eps)
        (rl[r["kept"]].sum() / r["k"]).backward()
        assert (xt.grad - r["grad"]).abs().max() < 1e-14
        assert r["kept"].sum() == r["k"] and not r["kept"][lab < 0].any()


def test_kept_rows_order_and_ties():
    loss = np.array([0.5, 0.0, 0.25, 0.25, 0.0, 0.75])
    lab = np.array([3, -1, 5, 2, -1, 1])
    assert CR.kept_rows(loss, lab, 2).tolist() == [False, False, True, True, False, False]
    assert CR.kept_rows(loss, lab, 1).tolist() == [False, False, True, False, False, False]      # tie: the lower row
    assert CR.kept_rows(loss, lab, 4).tolist() == [True, False, True, True, False, True]


def test_kept_count_edge_cases():
    from lavender_amd.captioning import kept_count
    assert kept_count(4, 0.25) == 3 and kept_count(150, 0.0) == 150 and kept_count(180, 0.25) == 135 and kept_count(22, 0.25) == 16
    assert kept_count(3, 0.5) == 1 and kept_count(2, 0.25) == 1
    assert kept_count(10, 0.3) == int(10 * (1 - 0.3)) == 7                 # the reference's own float expression
    assert kept_count(0, 0.25) == 0                                        # a batch without labels is not an error of the ratio
    for n, ratio in ((1, 0.25), (1, 0.5), (3, 0.75), (5, 1.0)):
        with pytest.raises(ValueError, match="mean of no rows"):
            kept_count(n, ratio)


def test_loss_object_keeps_the_reference_surface():
    from lavender_amd.captioning import CaptioningLoss
    ls = CaptioningLoss({"label_smoothing": 0.1, "drop_worst_ratio": 0.25, "drop_worst_after": 2})
    assert (ls.label_smoothing, ls.drop_worst_ratio, ls.drop_worst_after, ls.iter) == (0.1, 0.25, 2, 0)
    from lavender_amd.args import EasyDict
    ls = CaptioningLoss(EasyDict(label_smoothing=0.2))
    assert (ls.label_smoothing, ls.drop_worst_ratio, ls.drop_worst_after) == (0.2, 0, 0)
    assert ls.cuda() is ls


def test_predict_file_names():
    from lavender_amd.args import EasyDict
    from lavender_amd.captioning import get_predict_file, Agent_Captioning
    f = get_predict_file(EasyDict(max_gen_length=20), 3, "out/caption_predictions", "_datasets/msrvtt/val.yaml")
    assert f == "out/caption_predictions/ep3_pred.msrvtt.val.max20.tsv"
    f = get_predict_file(EasyDict(max_gen_length=20), 0, "o", "_datasets/coco_caption/test.yaml")
    assert f == "o/ep0_pred.test.max20.tsv"
    a = EasyDict(max_gen_length=30, num_beams=4, use_asr=True, num_keep_best=2)
    assert get_predict_file(a, 12, "o", "d/msvd/test.caption.yaml") == "o/ep12_pred.msvd.test.caption.beam4.max30.w_asr.best2.tsv"
    a = EasyDict(max_gen_length=20, num_beams=1, use_asr=False, num_keep_best=1)
    assert get_predict_file(a, 1, "o", "d/msvd/val.yaml") == "o/ep1_pred.msvd.val.beam1.max20.tsv"
    me = Agent_Captioning.__new__(Agent_Captioning)
    me.args = a
    assert me.get_predict_file(1, "o", "d/msvd/val.yaml") == "o/ep1_pred.msvd.val.beam1.max20.tsv"
    assert me.get_evaluate_file("o/x.tsv") == "o/x.eval.json"


def test_prediction_tsv_rows_follow_the_dataset_key_order(tmp_path):
    from lavender_amd.captioning import write_prediction_tsv
    p = str(tmp_path / "pred.tsv")
    write_prediction_tsv([["b", "[1]"], ["c", "[2]"], ["a", "[3]"]], p, key_order=["a", "b", "c"])
    assert open(p).read() == "a\t[3]\nb\t[1]\nc\t[2]\n"


def test_error_bounds_shrink_and_grow_as_derived():
    """the bound module on a small case: positive on labelled / kept entries, zero elsewhere, and larger for a longer row"""
    x, lab = CR.make_case(7, 1003, 2, 5, sigma=0.25)
    r = CR.captioning_loss(x, lab, 0.1, 0.25)
    b = CR.bounds(x, lab, 0.1, 1008, r)
    assert (b["row_loss"][lab >= 0] > 0).all() and (b["row_loss"][lab < 0] == 0).all()
    assert (b["grad"][r["kept"]] > 0).all() and (b["grad"][~r["kept"]] == 0).all()
    assert b["row_loss"].max() < 1e-4 and b["loss"] < 1e-4
    b2 = CR.bounds(x, lab, 0.1, 8 * 1008, r)
    assert (b2["row_loss"][lab >= 0] > b["row_loss"][lab >= 0]).all()


def test_args_carry_the_captioning_defaults():
    from lavender_amd.args import parse_with_config
    a = parse_with_config([])
    assert (a.label_smoothing, a.drop_worst_ratio, a.drop_worst_after, a.max_gen_length) == (0.0, 0.0, 0, 20)
    a = parse_with_config(["--label_smoothing", "0.1", "--drop_worst_ratio", "0.2", "--drop_worst_after", "100", "--max_gen_length", "12"])
    assert (a.label_smoothing, a.drop_worst_ratio, a.drop_worst_after, a.max_gen_length) == (0.1, 0.2, 100, 12)
