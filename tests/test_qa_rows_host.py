"""Host side of the video-QA rows path: the numpy restatement of lav_answer_readout's rules (tests/qa_answer_ref.py) against torch.topk /
torch.argmax and the reference's quotient formula, the planted rows, label_rows, the synthetic QA dataset's text layout and the entry points'
argument defaults.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import qa_answer_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_agrees_with_topk_and_the_quotient_formula_on_untied_rows():
    rng = np.random.default_rng(3)
    n, V = 16, 997
    x = rng.permutation(n * V).reshape(n, V).astype(np.float32) / 50.0 - 5000.0 / 50.0      # all values distinct
    labels = rng.integers(0, V, size=n).astype(np.int32)
    labels[3] = -1
    cand = [11, 500, 3, 996, 42]
    pred, rank, choice = QR.answer_ref(x, labels, cand)
    xt = torch.from_numpy(x)
    assert (torch.argmax(xt, -1).numpy() == pred).all()
    for k in (1, 5):
        top = torch.topk(xt, k=k, dim=-1).indices
        hit = (top == torch.from_numpy(labels.astype(np.int64)).view(-1, 1)).any(-1).float().numpy()
        assert (hit == QR.top_k_hit(rank, k)).all()
    assert rank[3] == -1 and QR.top_k_hit(rank, 5)[3] == 0
    p = xt[:, cand]                                            # main_qamc_mlm.py:161-166
    q = p / p.sum(dim=-1).view(n, 1)
    assert (torch.argmax(q, -1).numpy() == choice).all()
    assert (QR.answer_ref(x, labels, ())[2] == -1).all()


@pytest.mark.parametrize("V", [8, 257, 30522])
@pytest.mark.parametrize("bf16", [False, True])
def test_planted_rows(V, bf16):
    x, labels, what = QR.planted_rows(V, np.random.default_rng(5), bf16)
    pred, rank, _ = QR.answer_ref(x, labels)
    want = {"ties": 2, "rank exactly 0 (k = 1)": 0, "rank exactly 1 (k = 1)": 1, "rank exactly 4 (k = 5)": 4, "rank exactly 5 (k = 5)": 5,
            "NaN row, the label is a number": 2, "second NaN": 1, "first NaN": 0, "-0 and +0": 1, "+inf first": V - 1}
    seen = set()
    for r, name in enumerate(what):
        for key, val in want.items():
            if key in name:
                assert rank[r] == val, (name, rank[r])
                seen.add(key)
    assert seen == set(want)
    by = {name: r for r, name in enumerate(what)}
    assert pred[by["ties: the label's value at two lower and one higher index -> rank 2"]] == 0         # lowest index of the tied maximum
    assert pred[by["NaN row, the label is a number: both NaNs sort before it"]] == 3                      # the first NaN
    # top-k flags at the boundary
    for k in (1, 5):
        assert QR.top_k_hit(rank[[by[f"rank exactly {k - 1} (k = {k})"]]], k)[0] == 1
        assert QR.top_k_hit(rank[[by[f"rank exactly {k} (k = {k})"]]], k)[0] == 0


def test_choice_with_candidate_sums_of_either_sign():
    V = 64
    x = np.zeros((4, V), dtype=np.float32)
    cand = [5, 9, 20]
    x[0, cand] = [1.0, 3.0, 2.0]          # sum  6: the largest logit wins
    x[1, cand] = [-1.0, -3.0, -2.5]       # sum -6.5: the order reverses, the most negative logit wins
    x[2, cand] = [2.0, -4.0, 0.5]         # sum -1.5: q = [-1.33, 2.67, -0.33]
    x[3, cand] = [2.0, 2.0, -3.0]         # sum  1: tie between the first two, the first wins
    for r in range(4):
        assert abs(float(x[r, cand].sum())) >= 1.0
    _, _, choice = QR.answer_ref(x, np.full(4, -1), cand)
    assert choice.tolist() == [1, 1, 1, 0]
    xt = torch.from_numpy(x)[:, cand]
    assert torch.argmax(xt / xt.sum(-1, keepdim=True), -1).tolist()[:3] == [1, 1, 1]
    # a NaN candidate makes every quotient NaN: the first index
    x[0, 9] = np.nan
    assert QR.answer_ref(x[:1], [-1], cand)[2][0] == 0


def test_bf16_round_matches_torch():
    a = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 7
    assert (QR.bf16_round(a) == torch.from_numpy(a).bfloat16().float().numpy()).all()


@pytest.mark.parametrize("Lp", [0, 1, 9])
def test_label_rows(Lp):
    from lavender_amd.qa_mlm import label_rows
    X = 7
    ans = torch.full((4, X), -1, dtype=torch.long)
    ans[0, 6] = 11                       # one
    ans[2, 1] = 21; ans[2, 5] = 22       # two; samples 1 and 3 carry none
    lr = label_rows(ans, Lp)
    assert lr.sample.tolist() == [0, 2, 2] and lr.pos.tolist() == [6, 1, 5] and lr.label.tolist() == [11, 21, 22]
    assert lr.width == Lp + X and lr.row.tolist() == [Lp + 6, 2 * (Lp + X) + Lp + 1, 2 * (Lp + X) + Lp + 5]
    # the same rows and order as boolean indexing of the label block with its -1 pre-text in front
    full = torch.cat([torch.full((4, Lp), -1, dtype=torch.long), ans], 1)
    assert torch.nonzero(full.flatten() != -1).flatten().tolist() == lr.row.tolist()
    assert full[full != -1].tolist() == lr.label.tolist()
    assert lr.label.dtype == np.int32
    empty = label_rows(torch.full((3, X), -1, dtype=torch.long), Lp)
    assert len(empty.row) == 0 and len(empty.label) == 0


def test_synthetic_qa_text_layout():
    from lavender_amd.args import EasyDict
    from lavender_amd.data import QA_TOK, StubTokenizer, SyntheticQA
    tok = StubTokenizer()
    a = EasyDict(size_txt=21, size_frame=2, size_img=32, size_option=5)
    ds = SyntheticQA(a, 6, "val", tok, "oe", vocab=8192)
    for i in range(6):
        txt, mask, ans, idx = ds.text(i)
        assert txt.shape == (26,) and idx is None                           # X = size_txt + 5
        k = int((txt != 0).sum())
        assert txt[0] == 101 and txt[k - 1] == 102 and (txt[k:] == 0).all() and (mask == (txt != 0).long()).all()
        assert txt[k - 4:k - 1].tolist() == [QA_TOK["answer"], QA_TOK[":"], 103]      # "... answer: [MASK]" [SEP]
        assert int((ans != -1).sum()) == 1 and ans[k - 2] >= 1000 and (txt[ans != -1] == 103).all()
    b = ds.collate_batch([ds[0], ds[1]])
    assert set(b) == {"img", "txt", "mask", "mask_ans"} and b["img"].shape == (2, 2, 3, 32, 32) and b["txt"].shape == (2, 26)
    a.size_txt = 98
    ds = SyntheticQA(a, 6, "test", tok, "mc", vocab=8192)
    assert ds.ans_tok_ids == [1014, 1015, 1016, 1017, 1018]
    for i in range(6):
        txt, mask, ans, idx = ds.text(i)
        assert txt.shape == (101,) and 0 <= idx < 5                         # X = size_txt + 3
        k = int((txt != 0).sum())
        assert txt[0] == 101 and txt[k - 2] == 103 and txt[k - 1] == 102 and int((txt == 103).sum()) == 1
        assert ans[k - 2] == 1014 + idx and int((ans != -1).sum()) == 1
        body = txt[1:k - 2].tolist()
        for o in range(5):                                                  # "option o :" for every option, in order
            assert any(body[j:j + 3] == [QA_TOK["option"], 1014 + o, QA_TOK[":"]] for j in range(len(body) - 2))
    b = ds.collate_batch([ds[0], ds[1], ds[2]])
    assert b["ans_idx"].dtype == torch.long and b["ans_idx"].shape == (3,) and b["txt"].shape == (3, 101)
    ids, m = ds.get_prompt()
    assert ids[0] == 101 and ids[-1] == 102 and (m == 1).all()


def test_entry_point_argument_defaults():
    sys.path.insert(0, ROOT)
    import main_qamc_mlm
    import main_qaoe_mlm
    from lavender_amd.args import parse_with_config
    assert parse_with_config([]).qa_rows is False                           # the library default stays off
    for mod, task in ((main_qaoe_mlm, "qaoe"), (main_qamc_mlm, "qamc")):
        a = mod.cli_args([], distributed=False)
        assert a.qa_rows is True and a.size_vocab == -1 and a.task == task and a.enable_task_token is False and a.enable_prompt is False
        a = mod.cli_args(["--qa_rows", "false", "--enable_task_token", "--size_vocab", "500"], distributed=False)
        assert a.qa_rows is False and a.enable_task_token is True and a.size_vocab == -1
        assert mod.cli_args(["--enable_prompt"], distributed=False).enable_prompt is True
    assert main_qamc_mlm.cli_args([], distributed=False).task_token == "mc"
