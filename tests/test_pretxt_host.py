"""CPU: the pre-text callers (task token / prompt, model.py:194-307) restated from the unmodified oracle pieces (tests/pretxt_ref.py)
against the vectors captured from the reference (tests/golden/make_goldens_pretxt.py), and the host-side shapes of the model's pre-text
surface (labels, masks, pair map).  Tolerances as test_oracle_golden.py."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import lavender_ref as R
from tests import pretxt_ref as PR
from tests.helpers import BERT_CFGS, make_batch, sub


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)


def _params(bert, swin):
    bc = BERT_CFGS[bert]
    P = R.filled_params(swin, hidden=bc["hidden"], layers=bc["layers"], ffn=bc["ffn"], vocab=bc["vocab"])
    for v in P.values():
        v.requires_grad_(True)
    return P, bc


def _spec(kind, task, g):
    if kind == "task":
        return ("task", PR.TASK_TOK2ID[task])
    ids = torch.from_numpy(g["prompt"]).long()
    return ("prompt", (ids, torch.ones_like(ids)))


def _check(P, g, out, ans, ls):
    np.testing.assert_allclose(out[..., torch.from_numpy(g["cols"])].detach().numpy(), g["out_cols"], atol=1e-5)
    np.testing.assert_allclose(torch.logsumexp(out, -1).detach().numpy(), g["out_lse"], atol=1e-5)
    assert (ans.numpy() == g["ans"]).all()
    assert abs(ls.item() - g["loss"][0]) < 1e-5
    ls.backward()
    for k, v in zip(g["grad_norm_keys"].tolist(), g["grad_norm_vals"].tolist()):
        gr = P[k].grad
        if v < 0:
            assert gr is None, k
        else:
            assert abs(gr.double().norm().item() - v) <= 1e-4 * v + 2e-6, k
    ge = P["emb_task"].grad
    ge = torch.zeros_like(P["emb_task"]) if ge is None else ge
    np.testing.assert_allclose(ge.detach().numpy(), g["grad_emb_task"], atol=2e-6, rtol=1e-4)
    for k in g.files:
        if k.startswith("grad_sub::"):
            np.testing.assert_allclose(sub(P[k[10:]].grad, 2048), g[k], atol=2e-6, rtol=1e-3)


@pytest.mark.parametrize("kind", ["task", "prompt"])
def test_qaoe_pretxt_matches_reference(golden_dir, kind):
    g = _load(golden_dir, f"pretxt_qaoe_{kind}")
    swin, bert, B, _, X = g["meta"].tolist()
    P, bc = _params(bert, swin)
    batch = make_batch(int(B), X=int(X), vocab=bc["vocab"], seed=6)
    txt = torch.from_numpy(g["txt"])
    batch.update(txt=txt, mask=(txt != 0).long(), mask_ans=torch.from_numpy(g["mask_ans"]))
    out, ans = PR.qa_forward(P, batch, swin, bc["heads"], _spec(kind, "oe", g))
    Lp = 1 if kind == "task" else len(g["prompt"])
    assert out.shape[:2] == (int(B), Lp + int(X)) and (ans[:, :Lp] == -1).all()
    _check(P, g, out, ans, torch.nn.functional.cross_entropy(out.flatten(0, 1), ans.flatten(), ignore_index=-1))


def test_retmc_task_token_matches_reference(golden_dir):
    g = _load(golden_dir, "pretxt_retmc_task")
    swin, bert, B, _, X, O = g["meta"].tolist()
    B, O = int(B), int(O)
    P, bc = _params(bert, swin)
    txt = torch.from_numpy(g["txt"])
    batch = {"img": make_batch(B, vocab=bc["vocab"], seed=13)["img"], "txt": txt, "mask": (txt != 0).long(),
             "mask_ans": torch.from_numpy(g["mask_ans"])}
    out, ans = PR.retmc_forward(P, batch, swin, bc["heads"], _spec("task", "vtm", g))
    assert ans.shape == (B, O, 1 + int(X))
    _check(P, g, out, ans, torch.nn.functional.cross_entropy(out.flatten(0, 1), ans.flatten(), ignore_index=-1))
    assert np.abs(g["grad_emb_task"][1:]).max() == 0 and np.abs(g["grad_emb_task"][0]).max() > 0     # only the "vtm" row


@pytest.mark.parametrize("kind", ["task", "prompt"])
def test_captioning_pretxt_matches_reference(golden_dir, kind):
    g = _load(golden_dir, f"pretxt_cap_{kind}")
    swin, bert, B, _, X = g["meta"].tolist()
    P, bc = _params(bert, swin)
    batch = make_batch(int(B), vocab=bc["vocab"], seed=6)
    batch.update(txt=torch.from_numpy(g["txt"]), ans_mtm=torch.from_numpy(g["ans_mtm"]))
    out = PR.captioning_forward(P, batch, swin, bc["heads"], _spec(kind, "cap", g))
    Lp = 1 if kind == "task" else len(g["prompt"])
    assert int(g["cap_prompt_txt_L"][0]) == Lp
    ls = torch.nn.functional.cross_entropy(out["out"].flatten(0, 1), out["ans"].flatten(), ignore_index=-1)
    _check(P, g, out["out"], out["ans"], ls)


def test_seq2seq_mask_with_pretxt_matches_the_model_surface():
    """LAVENDER_Base.get_attn_mask(mask_pretxt=) (host tensors, no device) against the restatement; "full" is the concatenation"""
    from lavender_amd.model import LAVENDER_Base
    B, Lv, Lp, X = 2, 5, 3, 4
    m_img = torch.ones(B, Lv, dtype=torch.long)
    m_img[1, -2:] = 0
    m_pre = torch.ones(B, Lp, dtype=torch.long)
    m_txt = torch.ones(B, X, dtype=torch.long)
    m = LAVENDER_Base.get_attn_mask(None, m_img, m_txt, "seq2seq", mask_pretxt=m_pre)
    assert torch.equal(m, PR.seq2seq_mask(torch.cat([m_img, m_pre], 1), X))
    assert m.shape == (B, Lv + Lp + X, Lv + Lp + X)
    assert (m[:, :Lv + Lp, Lv + Lp:] == 0).all()                  # prefix queries see no text key
    assert (m[:, Lv + Lp:, Lv:Lv + Lp] == 1).all()                 # text queries see the whole pre-text
    full = LAVENDER_Base.get_attn_mask(None, m_img, m_txt, "full", mask_pretxt=m_pre)
    assert torch.equal(full, torch.cat([m_img, m_pre, m_txt], 1))


def _surface(enable_task_token=False, enable_prompt=False, qa=False):
    """the model's pre-text methods on a stand-in object (no parameters, no device)"""
    from lavender_amd.model import LAVENDER_Base
    from lavender_amd.qa_mlm import LAVENDER_QAOE_MLM
    cls = LAVENDER_QAOE_MLM if qa else LAVENDER_Base
    o = SimpleNamespace(args=SimpleNamespace(enable_task_token=enable_task_token, enable_prompt=enable_prompt), task_tok2id=PR.TASK_TOK2ID)
    for name in ("_pretxt_spec", "_pretxt_ids", "prepro_pretxt"):
        setattr(o, name, getattr(cls, name).__get__(o))
    return o


def test_pretxt_ids_and_masks():
    B, X = 3, 7
    mask = torch.ones(B, X, dtype=torch.long)
    o = _surface(enable_task_token=True, enable_prompt=True)
    prompt = (torch.tensor([101, 5, 6, 102]), torch.ones(4, dtype=torch.long))
    spec = o._pretxt_spec("cap", prompt)
    assert spec == ("task", 3)                                         # the task token wins over a prompt
    ids, m = o._pretxt_ids(spec, mask)
    assert ids.shape == (B, 1) and (ids == 0).all() and (m == 1).all()
    o = _surface(enable_prompt=True)
    assert o._pretxt_spec("cap", None) is None
    ids, m = o._pretxt_ids(o._pretxt_spec(None, prompt), mask)
    assert ids.shape == (B, 4) and (ids == prompt[0]).all() and m.shape == (B, 4)
    ids, m = o._pretxt_ids(o._pretxt_spec(None, prompt), mask[0])      # 1-D text (one caption)
    assert ids.shape == (4,)
    per_text = (torch.arange(B * 4).view(B, 4), torch.ones(B, 4, dtype=torch.long))
    ids, _ = o._pretxt_ids(o._pretxt_spec(None, per_text), mask)
    assert torch.equal(ids, per_text[0])
    ids, _ = _surface(enable_task_token=True, qa=True)._pretxt_ids(("task", 2), mask)
    assert (ids == -1).all()                                            # QA callers: no label at the pre-text
    with pytest.raises(AssertionError):
        _surface(enable_task_token=True)._pretxt_spec("nope", None)
    assert _surface()._pretxt_spec("oe", prompt) is None                # both switches off: no pre-text


def test_pair_map_with_pretxt():
    """downstream of the embedding the text length is X' = Lp + X: the pair map of the fused first layer addresses the pre-text rows as text
    rows of the one (B * Lv + n * (Lp + X), H) source"""
    from lavender_amd import engine as E
    B, Lv, Lp, X = 2, 4, 3, 5
    idx = E.pair_index(B, Lv, B, Lp + X, np.arange(B), np.arange(B))
    assert idx.shape == (B, Lv + Lp + X)
    assert idx[1, Lv] == B * Lv + (Lp + X) and idx[1, -1] == B * Lv + 2 * (Lp + X) - 1


def test_emb_task_trains_only_with_the_switch():
    from lavender_amd.arena import NO_GRAD_PARAMS, no_grad_params
    off = SimpleNamespace(args=SimpleNamespace(enable_task_token=False))
    on = SimpleNamespace(args=SimpleNamespace(enable_task_token=True))
    assert no_grad_params(off) == NO_GRAD_PARAMS and "emb_task" in NO_GRAD_PARAMS
    assert "emb_task" not in no_grad_params(on) and "enc_img.emb_odr" in no_grad_params(on)


def test_retrieval_prompt_matches_reference(golden_dir):
    """LAVENDER_Retrieval_MLM with a prompt: the reference prepends it per pair (main_retrieval_mlm.py:62-80), the restatement once per text"""
    g = _load(golden_dir, "pretxt_retrieval_prompt")
    swin, bert, B, _, X = g["meta"].tolist()
    P, bc = _params(bert, swin)
    batch = make_batch(int(B), vocab=bc["vocab"], seed=4)
    batch.update(txt=torch.from_numpy(g["txt"]), vid=g["vid"].tolist())
    out, ans = PR.retrieval_forward(P, batch, swin, bc["heads"], _spec("prompt", None, g))
    assert out.shape[:2] == (int(B) ** 2, len(g["prompt"]) + int(X))
    _check(P, g, out, ans, torch.nn.functional.cross_entropy(out.flatten(0, 1), ans.flatten(), ignore_index=-1))


@pytest.mark.parametrize("kind", ["task", "prompt"])
def test_pretrain_vtm_pretxt_matches_reference(golden_dir, kind):
    g = _load(golden_dir, f"pretxt_pretrain_{kind}")
    swin, bert, B, _, X = g["meta"].tolist()
    P, bc = _params(bert, swin)
    batch = make_batch(int(B), vocab=bc["vocab"], seed=1)
    batch.update(txt=torch.from_numpy(g["txt"]), ans_mtm=torch.from_numpy(g["ans_mtm"]))
    np.random.seed(88)
    out = PR.pretrain_forward(P, batch, swin, bc["heads"], _spec(kind, "vtm", g))
    np.testing.assert_allclose(torch.logsumexp(out["out_mtm"], -1).detach().numpy(), g["mtm_lse"], atol=1e-5)
    l_mtm = torch.nn.functional.cross_entropy(out["out_mtm"].flatten(0, 1), out["ans_mtm"].flatten(), ignore_index=-1)
    l_vtm = torch.nn.functional.cross_entropy(out["out_vtm"].flatten(0, 1), out["ans_vtm"].flatten(), ignore_index=-1)
    np.testing.assert_allclose([l_mtm.item(), l_vtm.item()], g["losses"], atol=1e-5)
    _check(P, g, out["out_vtm"], out["ans_vtm"], l_mtm + l_vtm)


class _WordTok:
    """a tokenizer stand-in with tokenize / convert_tokens_to_ids over a fixed word list (bert-base-uncased ids of these words)"""
    cls_token, sep_token, pad_token, mask_token, unk_token = "[CLS]", "[SEP]", "[PAD]", "[MASK]", "[UNK]"
    ids = {"[PAD]": 0, "[UNK]": 100, "[CLS]": 101, "[SEP]": 102, "[MASK]": 103, "true": 2995, "false": 6270, "is": 2003, "the": 1996,
           "video": 2678, "-": 1011, "text": 3793, "paired": 12739, ",": 1010, "or": 2030, "?": 1029}

    def tokenize(self, s):
        return s.replace("-", " - ").replace(",", " , ").replace("?", " ?").split()

    def convert_tokens_to_ids(self, toks):
        return [self.ids.get(t, 100) for t in toks]


def test_get_prompt_tokenises_prompt_texts():
    """Dataset_Base.get_prompt (dataset.py:72-81): [CLS] + tokens + [SEP], mask of ones; Dataset_Pretrain_MLM's vtm / cap prompts"""
    from lavender_amd import data as D
    ds = D.Dataset_Base.__new__(D.Dataset_Base)
    D.Dataset_Base.__init__(ds, SimpleNamespace(), tokzr=_WordTok())
    txt, mask = ds.get_prompt(D.PROMPT_TEXTS["pretrain_vtm"])
    assert txt.tolist() == [101, 2003, 1996, 2678, 1011, 3793, 12739, 1010, 2995, 2030, 6270, 1029, 102]
    assert mask.tolist() == [1] * 13 and txt.dtype == torch.long
    with pytest.raises(NotImplementedError):
        ds.get_prompt()                                        # the caller's dataset defines prompt_text
    assert D.Dataset_Pretrain_MLM.vtm_prompt_text.fget(ds) == D.PROMPT_TEXTS["pretrain_vtm"]
    assert D.PROMPT_TEXTS["qamc"](5) == "which answer is correct, from [0, 1, 2, 3, 4]?"


def test_set_pretxt_follows_the_switches():
    from lavender_amd.agent import set_pretxt
    dl = SimpleNamespace(dataset=SimpleNamespace(get_prompt=lambda: ("ids", "mask")))
    assert set_pretxt(SimpleNamespace(enable_prompt=True, enable_task_token=True), {}, dl, "oe") == {"prompt": ("ids", "mask")}
    assert set_pretxt(SimpleNamespace(enable_prompt=False, enable_task_token=True), {}, dl, "oe") == {"task_name": "oe"}
    assert set_pretxt(SimpleNamespace(enable_prompt=False, enable_task_token=False), {}, dl, "oe") == {}
