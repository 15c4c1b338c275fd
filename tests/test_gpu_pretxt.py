"""Task tokens and prompts in the fusion encoder (enable_task_token / enable_prompt, model.py:194-307) on the HIP engine:
  * kernels: lav_text_embed_pre_fwd / _bwd against lav_text_embed_fwd / _bwd (Lp = 0 and the text rows bit for bit) and the pre-text
    gradient against a float64 sum (fixed order: two runs give the same bits), per-text pre-text blocks;
  * callers (QAOE, RetMC, captioning encode_forward) against the reference fixtures (tests/golden/pretxt_*.npz) and, tensor by tensor, the
    CPU restatement tests/pretxt_ref.py;
  * the optimizer: emb_task becomes an ordinary AdamW parameter with the switch on and stays untouched with it off."""
import os

import numpy as np
import pytest
import torch

from tests import pretxt_ref as PR
from tests.helpers import BERT_CFGS, make_batch
from tests.test_gpu_variants import _grad_check

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16


def _emb_tables(V=512, P=64, Hd=768, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = [torch.randn(V, Hd, generator=g) * 0.05, torch.randn(P, Hd, generator=g) * 0.05, torch.randn(2, Hd, generator=g) * 0.05,
         1 + 0.1 * torch.randn(Hd, generator=g), 0.1 * torch.randn(Hd, generator=g)]
    return [x.cuda() for x in t]


def _zeros_like_grads(word, pos, type_, gamma, beta):
    return [torch.zeros_like(x) for x in (word, pos, type_[0], gamma, beta)]


@pytest.mark.parametrize("n,Lp,X,p", [(5, 0, 33, 0.1), (5, 1, 33, 0.1), (32, 9, 26, 0.1), (160, 1, 26, 0.0)])
def test_pre_fwd_text_rows_bit_identical(n, Lp, X, p):
    from lavender_amd import hip as K
    Hd = 768
    word, pos, type_, gamma, beta = _emb_tables(Hd=Hd)
    ids = torch.randint(0, 512, (n, X), generator=torch.Generator().manual_seed(n)).cuda()
    pre = (torch.randn(max(Lp, 1), Hd) * 0.3).to(bf16).cuda()
    ref, m0, r0 = K.text_embed_fwd(ids, n, X, Hd, word, pos, type_, gamma, beta, 1e-12, p, 1234)
    out, m1, r1 = K.text_embed_pre_fwd(ids, n, Lp, X, Hd, word, pos, type_, gamma, beta, 1e-12, p, 1234, pre, 0)
    torch.cuda.synchronize()
    o = out.view(n, Lp + X, Hd)
    assert torch.equal(o[:, Lp:].view(torch.int16), ref.view(n, X, Hd).view(torch.int16))
    assert torch.equal(m0, m1) and torch.equal(r0, r1)
    if Lp:
        assert torch.equal(o[:, :Lp].view(torch.int16), pre[:Lp].unsqueeze(0).expand(n, -1, -1).view(torch.int16))


def test_pre_fwd_per_text_block():
    from lavender_amd import hip as K
    n, Lp, X, Hd = 6, 4, 20, 768
    word, pos, type_, gamma, beta = _emb_tables(Hd=Hd)
    ids = torch.randint(0, 512, (n, X)).cuda()
    pre = (torch.randn(n, Lp, Hd) * 0.3).to(bf16).cuda()
    out, _, _ = K.text_embed_pre_fwd(ids, n, Lp, X, Hd, word, pos, type_, gamma, beta, 1e-12, 0.0, 7, pre, Lp * Hd)
    torch.cuda.synchronize()
    assert torch.equal(out.view(n, Lp + X, Hd)[:, :Lp].view(torch.int16), pre.view(torch.int16))


@pytest.mark.parametrize("n,Lp,X,p", [(5, 0, 33, 0.1), (5, 1, 33, 0.1), (40, 9, 26, 0.1)])
def test_pre_bwd_text_gradients_match_text_embed_bwd(n, Lp, X, p):
    """the parameter gradients of the text rows: the same kernel arithmetic as lav_text_embed_bwd.  Its column sums (d_pos, d_type0, dgamma,
    dbeta) and the word rows are fp32 atomics across blocks whose order is not fixed, so two runs of EITHER entry may differ in the last bits
    of a sum (one ulp of the column total per reordered add: ~1e-6 at these magnitudes) -- compared at 1e-4 relative / 1e-5 absolute."""
    from lavender_amd import hip as K
    Hd = 768
    word, pos, type_, gamma, beta = _emb_tables(Hd=Hd)
    ids = torch.randint(0, 512, (n, X), generator=torch.Generator().manual_seed(3)).cuda()
    _, mean, rstd = K.text_embed_fwd(ids, n, X, Hd, word, pos, type_, gamma, beta, 1e-12, p, 99)
    dout = (torch.randn(n, Lp + X, Hd) * 0.1).to(bf16).cuda()
    ga = _zeros_like_grads(word, pos, type_, gamma, beta)
    gb = _zeros_like_grads(word, pos, type_, gamma, beta)
    K.text_embed_bwd(ids, dout[:, Lp:].contiguous(), n, X, Hd, word, pos, type_[0], gamma, mean, rstd, p, 99, *ga)
    d_pre = torch.zeros(max(Lp, 1), Hd, device="cuda")
    K.text_embed_pre_bwd(ids, dout, n, Lp, X, Hd, word, pos, type_[0], gamma, mean, rstd, p, 99, *gb, 0, d_pre, 0)
    torch.cuda.synchronize()
    for a, b in zip(ga, gb):
        torch.testing.assert_close(b, a, rtol=1e-4, atol=1e-5)
    if Lp:
        exact = dout[:, :Lp].double().sum(0)
        tol = n * 2.0 ** -24 * dout[:, :Lp].double().abs().sum(0) + 1e-12
        assert ((d_pre[:Lp].double() - exact).abs() <= tol).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_pre_grad_fixed_order_at_n160(mode):
    """pre_stride 0 at n = 160 texts (B * O of RetMC / pretrain VTM): fp32 sum within the summation bound of a float64 sum, and the same bits in
    two runs; mode 0 accumulates into the fp32 row, mode 1 writes bf16 rows"""
    from lavender_amd import hip as K
    n, Lp, X, Hd = 160, 3, 8, 768
    word, pos, type_, gamma, beta = _emb_tables(Hd=Hd)
    ids = torch.randint(0, 512, (n, X)).cuda()
    _, mean, rstd = K.text_embed_fwd(ids, n, X, Hd, word, pos, type_, gamma, beta, 1e-12, 0.0, 5)
    dout = (torch.randn(n, Lp + X, Hd) * 0.1).to(bf16).cuda()
    runs = []
    for _ in range(2):
        gr = _zeros_like_grads(word, pos, type_, gamma, beta)
        if mode == 0:
            d_pre = torch.full((Lp, Hd), 0.25, device="cuda")
        else:
            d_pre = torch.empty(Lp, Hd, dtype=bf16, device="cuda")
        K.text_embed_pre_bwd(ids, dout, n, Lp, X, Hd, word, pos, type_[0], gamma, mean, rstd, 0.0, 5, *gr, 0, d_pre, mode)
        torch.cuda.synchronize()
        runs.append(d_pre.clone())
    assert torch.equal(runs[0].view(torch.int32 if mode == 0 else torch.int16), runs[1].view(torch.int32 if mode == 0 else torch.int16))
    exact = dout[:, :Lp].double().sum(0)
    bound = n * 2.0 ** -24 * dout[:, :Lp].double().abs().sum(0) + 1e-12
    got = runs[0].double() - (0.25 if mode == 0 else 0.0)
    if mode == 1:
        bound = bound + exact.abs() * 2.0 ** -8                # bf16 rounding of the result
    else:
        bound = bound + 2.0 ** -24 * (exact.abs() + 0.25)        # the accumulate into 0.25
    assert ((got - exact).abs() <= bound).all()


def test_pre_bwd_per_text_rows():
    from lavender_amd import hip as K
    n, Lp, X, Hd = 12, 4, 10, 768
    word, pos, type_, gamma, beta = _emb_tables(Hd=Hd)
    ids = torch.randint(0, 512, (n, X)).cuda()
    _, mean, rstd = K.text_embed_fwd(ids, n, X, Hd, word, pos, type_, gamma, beta, 1e-12, 0.0, 5)
    dout = (torch.randn(n, Lp + X, Hd) * 0.1).to(bf16).cuda()
    gr = _zeros_like_grads(word, pos, type_, gamma, beta)
    d_pre = torch.empty(n, Lp, Hd, dtype=bf16, device="cuda")
    K.text_embed_pre_bwd(ids, dout, n, Lp, X, Hd, word, pos, type_[0], gamma, mean, rstd, 0.0, 5, *gr, Lp * Hd, d_pre, 1)
    torch.cuda.synchronize()
    assert torch.equal(d_pre.view(torch.int16), dout[:, :Lp].contiguous().view(torch.int16))


# ---- callers against the reference fixtures ------------------------------------------------------------------------------------------
def _oracle_params(bert, swin):
    from oracle import lavender_ref as R
    bc = BERT_CFGS[bert]
    P = R.filled_params(swin, hidden=bc["hidden"], layers=bc["layers"], ffn=bc["ffn"], vocab=bc["vocab"])
    for v in P.values():
        v.requires_grad_(True)
    return P, bc


def _model(cls, swin, bert, B, kind):
    from tests.helpers import build_filled_model
    m = build_filled_model(swin, bert, B, cls=cls)
    m.args.enable_task_token, m.args.enable_prompt = kind == "task", kind == "prompt"
    return m.eval()


def _prompt(g):
    ids = torch.from_numpy(g["prompt"]).long()
    return ids, torch.ones_like(ids)


def _check_logits(out, g, tag):
    a = out.detach().float().cpu()
    lse = torch.logsumexp(a, -1).numpy()
    d = np.abs(a[..., torch.from_numpy(g["cols"])].numpy() - g["out_cols"])
    print(tag, "logits max", d.max(), "mean", d.mean(), "lse max", np.abs(lse - g["out_lse"]).max())
    assert d.max() < 3e-2 and d.mean() < 5e-3
    assert np.abs(lse - g["out_lse"]).max() < 2e-2


def _check_emb_task(m, P, row):
    ge = m.emb_task.grad.float().cpu()
    others = [r for r in range(ge.shape[0]) if r != row]
    assert float(ge[others].abs().max()) == 0.0                   # rows of other tasks: exactly zero
    if row is not None:
        ref = P["emb_task"].grad[row]
        rel = ((ge[row] - ref).norm() / ref.norm()).item()
        print("emb_task row", row, "rel", rel)
        assert rel < 0.05


@pytest.mark.parametrize("kind", ["task", "prompt"])
def test_qaoe_pretxt_against_reference(golden_dir, kind):
    import lavender_amd as LA
    from lavender_amd.agent import CrossEntropyIgnore
    g = np.load(os.path.join(golden_dir, f"pretxt_qaoe_{kind}.npz"))
    swin, bert, B, _, X = g["meta"].tolist()
    B, X = int(B), int(X)
    P, bc = _oracle_params(bert, swin)
    batch = make_batch(B, X=X, vocab=bc["vocab"], seed=6)
    txt = torch.from_numpy(g["txt"])
    batch.update(txt=txt, mask=(txt != 0).long(), mask_ans=torch.from_numpy(g["mask_ans"]))
    spec = ("task", 2) if kind == "task" else ("prompt", _prompt(g))
    ref, ans_ref = PR.qa_forward(P, batch, swin, bc["heads"], spec)
    torch.nn.functional.cross_entropy(ref.flatten(0, 1), ans_ref.flatten(), ignore_index=-1).backward()
    if kind == "prompt":
        P["emb_task"].grad = None

    m = _model(LA.LAVENDER_QAOE_MLM, swin, bert, B, kind)
    m.arena().zero_grad()
    b = {k: v.cuda() for k, v in batch.items()}
    b["task_name"], b["prompt"] = ("oe", None) if kind == "task" else (None, _prompt(g))
    out, ans = m(b)
    Lp = 1 if kind == "task" else len(g["prompt"])
    assert out.shape == (B, Lp + X, bc["vocab"]) and (ans.cpu().numpy() == g["ans"]).all()
    _check_logits(out, g, f"qaoe/{kind}")
    ls = CrossEntropyIgnore()(out.flatten(0, 1), ans.flatten(), count=int((ans != -1).sum()))
    ls.backward()
    torch.cuda.synchronize()
    assert abs(ls.item() - g["loss"][0]) < 1e-2
    _grad_check(m, P)
    _check_emb_task(m, P, 2 if kind == "task" else None)


def test_retmc_task_token_against_reference(golden_dir):
    import lavender_amd as LA
    from lavender_amd.agent import CrossEntropyIgnore
    g = np.load(os.path.join(golden_dir, "pretxt_retmc_task.npz"))
    swin, bert, B, _, X, O = g["meta"].tolist()
    B, X, O = int(B), int(X), int(O)
    P, bc = _oracle_params(bert, swin)
    txt = torch.from_numpy(g["txt"])
    batch = {"img": make_batch(B, vocab=bc["vocab"], seed=13)["img"], "txt": txt, "mask": (txt != 0).long(),
             "mask_ans": torch.from_numpy(g["mask_ans"])}
    ref, ans_ref = PR.retmc_forward(P, batch, swin, bc["heads"], ("task", 0))
    torch.nn.functional.cross_entropy(ref.flatten(0, 1), ans_ref.flatten(), ignore_index=-1).backward()
    m = _model(LA.LAVENDER_RetMC_MLM, swin, bert, B, "task")
    m.arena().zero_grad()
    b = {k: v.cuda() for k, v in batch.items()}
    b["task_name"] = "vtm"
    out, ans = m(b)
    assert out.shape == (B * O, 1 + X, bc["vocab"]) and (ans.cpu().numpy() == g["ans"]).all()
    _check_logits(out, g, "retmc/task")
    ls = CrossEntropyIgnore()(out.flatten(0, 1), ans.flatten(), count=int((ans != -1).sum()))
    ls.backward()
    torch.cuda.synchronize()
    assert abs(ls.item() - g["loss"][0]) < 1e-2
    _grad_check(m, P)
    _check_emb_task(m, P, 0)


@pytest.mark.parametrize("kind", ["task", "prompt"])
def test_captioning_pretxt_against_reference(golden_dir, kind):
    import lavender_amd as LA
    from lavender_amd.agent import CrossEntropyIgnore
    g = np.load(os.path.join(golden_dir, f"pretxt_cap_{kind}.npz"))
    swin, bert, B, _, X = g["meta"].tolist()
    B, X = int(B), int(X)
    P, bc = _oracle_params(bert, swin)
    batch = make_batch(B, vocab=bc["vocab"], seed=6)
    batch.update(txt=torch.from_numpy(g["txt"]), ans_mtm=torch.from_numpy(g["ans_mtm"]))
    spec = ("task", 3) if kind == "task" else ("prompt", _prompt(g))
    ref = PR.captioning_forward(P, batch, swin, bc["heads"], spec)
    torch.nn.functional.cross_entropy(ref["out"].flatten(0, 1), ref["ans"].flatten(), ignore_index=-1).backward()
    if kind == "prompt":
        P["emb_task"].grad = None
    m = _model(LA.LAVENDER_Captioning, swin, bert, B, kind)
    m.arena().zero_grad()
    b = {k: v.cuda() for k, v in batch.items()}
    b["attn_mask_type"] = "seq2seq"
    b["prompt"] = _prompt(g) if kind == "prompt" else None
    out = m(b)
    assert m.cap_prompt_txt_L == int(g["cap_prompt_txt_L"][0])
    assert (out["ans"].cpu().numpy() == g["ans"]).all()
    _check_logits(out["out"], g, f"cap/{kind}")
    ls = CrossEntropyIgnore()(out["out"].flatten(0, 1), out["ans"].flatten(), count=int((out["ans"] != -1).sum()))
    ls.backward()
    torch.cuda.synchronize()
    assert abs(ls.item() - g["loss"][0]) < 1e-2
    _grad_check(m, P)
    _check_emb_task(m, P, 3 if kind == "task" else None)


def test_one_buffer_no_copy_of_the_text_rows():
    """go_feat with a task token: video, pre-text and text rows are views of ONE buffer (the fused first layer reads it in place)"""
    import lavender_amd as LA
    from lavender_amd import engine as E
    m = _model(LA.LAVENDER_QAOE_MLM, "micro", "micro", 2, "task")
    b = make_batch(2, X=12, vocab=BERT_CFGS["micro"]["vocab"])
    with torch.no_grad():
        f_img, _, f_txt, mask = m.go_feat(b["img"].cuda(), b["txt"].cuda(), b["mask"].cuda(), task_name="mc")
    assert f_txt.shape == (2, 13, f_img.shape[-1]) and mask.shape == (2, 12)
    assert E.rows_adjacent(f_img, f_txt)
    torch.cuda.synchronize()
    row = m.emb_task.detach()[1].to(bf16)
    assert torch.equal(f_txt[:, 0].cpu().view(torch.int16), row.cpu().view(torch.int16).expand(2, -1))


@pytest.mark.parametrize("on", [True, False])
def test_agent_step_moves_emb_task_as_adamw(on):
    """Agent_QAOE_MLM.step: with enable_task_token emb_task is updated like every "other/decay" parameter (oracle adamw_step on the gradient
    the step produced; the rows of other tasks only decay); with the switch off it does not move"""
    import lavender_amd as LA
    from oracle import lavender_ref as R
    from tests.helpers import Tok, make_args
    from lavender_amd.dist import set_seed
    set_seed(88)
    B, X = 2, 16
    args = make_args("micro", "micro", B, lr=1e-3, decay=0.5, max_iter=1, max_grad_norm=-1.0, size_vocab=-1, enable_task_token=on)
    m = LA.LAVENDER_QAOE_MLM(args, Tok()).cuda()
    m.arena()
    ag = LA.Agent_QAOE_MLM(args, m)
    b = make_batch(B, X=X, vocab=BERT_CFGS["micro"]["vocab"], seed=6)
    ans = torch.full(b["txt"].shape, -1, dtype=torch.long)
    ans[:, -1] = torch.tensor([1016, 1014])
    b["mask_ans"] = ans
    if on:
        b["task_name"] = "oe"
    p0 = m.emb_task.detach().clone()
    seen = {}
    orig = ag.optzr.step

    def step(**kw):
        seen["g"] = m.emb_task.grad.detach().clone()
        seen["lr"], seen["wd"] = ag.optzr.param_groups[1]["lr"], ag.optzr.param_groups[1]["weight_decay"]
        return orig(**kw)
    ag.optzr.step = step
    ag.step(ag.prepare_batch(dict(b)), True)
    torch.cuda.synchronize()
    p1 = m.emb_task.detach()
    if not on:
        assert torch.equal(p0, p1) and float(seen["g"].abs().max()) == 0.0
        return
    g = seen["g"].cpu()
    assert float(g[[0, 1, 3]].abs().max()) == 0.0 and float(g[2].abs().max()) > 0
    exp, _, _ = R.adamw_step(p0.cpu().double(), g.double(), 0.0, 0.0, 1, seen["lr"], seen["wd"])
    d = (p1.cpu().double() - exp).abs().max().item()
    print("emb_task vs oracle adamw_step: max |d|", d, "moved", (p1 - p0).abs().max().item())
    assert d < 1e-6 and not torch.equal(p0[0], p1[0]) and not torch.equal(p0[2], p1[2])     # row 0 decays, row 2 ("oe") takes its step


# ---- caption generation with a pre-text ---------------------------------------------------------------------------------------------
def _gen_model(golden_dir, kind, **kw):
    import lavender_amd as LA
    g = np.load(os.path.join(golden_dir, "pretxt_cap_gen_prompt.npz"))
    m = _model(LA.LAVENDER_Captioning, "micro", "micro", 2, kind)
    with torch.no_grad():
        m.fc_mtm.predictions.decoder.weight.mul_(float(str(g["meta"][4]).split("x")[-1]))
    m.sync_weights()
    m.args.update(max_gen_length=int(g["meta"][3]), **kw)
    return g, m


def test_greedy_generation_with_prompt_matches_reference(golden_dir):
    """LAVENDER_Captioning.generate with a prompt (model_for_captioning.py:160-176, 258-290): the cached decoder's prefix is [video rows ;
    prompt rows] -- the reference's greedy ids, log-probabilities and cap_prompt_txt_L"""
    g, m = _gen_model(golden_dir, "prompt")
    batch = make_batch(2, vocab=BERT_CFGS["micro"]["vocab"], seed=6)
    b = {k: v.cuda() for k, v in batch.items()}
    b.update(attn_mask_type="seq2seq", prompt=_prompt(g))
    ids, lp = m(b, is_decode=True)
    assert (ids.cpu().numpy() == g["ids"]).all(), (ids.cpu().tolist(), g["ids"].tolist())
    np.testing.assert_allclose(lp.cpu().numpy(), g["logprob"], atol=2e-2)
    assert m.cap_prompt_txt_L == int(g["cap_prompt_txt_L"][0])


@pytest.mark.parametrize("kind", ["task", "prompt"])
@pytest.mark.parametrize("beams", [1, 3])
def test_cached_generation_with_pretxt_matches_full_recompute(golden_dir, kind, beams):
    """the key / value cached decoder (prefix Lv' = Lv + Lp) and the literal loop (LAV_CAP_KV=0: the pre-text concatenated, causal_from =
    Lv + Lp) choose the same tokens, greedy and beam search"""
    from lavender_amd import caption_decode as CD
    g, m = _gen_model(golden_dir, kind, **({} if beams == 1 else dict(num_beams=beams, num_keep_best=2)))
    img = make_batch(2, vocab=BERT_CFGS["micro"]["vocab"], seed=6)["img"].cuda()
    pretxt = m._pretxt_spec("cap", _prompt(g))
    cfg = CD.make_config(m.args, 32)
    with torch.no_grad():
        run = CD.generate if beams == 1 else CD.generate_beam
        ids_k, lp_k = run(m.eval(), img, 32, cfg, kv=True, pretxt=pretxt)
        ids_f, lp_f = run(m, img, 32, cfg, kv=False, pretxt=pretxt)
        _, lp_0 = run(m, img, 32, cfg, kv=True)
    print(kind, beams, "cached", ids_k[:, 0].tolist(), "literal", ids_f[:, 0].tolist())
    assert torch.equal(ids_k, ids_f)
    np.testing.assert_allclose(lp_k.cpu().numpy(), lp_f.cpu().numpy(), atol=2e-2)
    assert not torch.equal(lp_k, lp_0)                            # the pre-text does reach the decoder (the key-filled micro model picks the same words)


# ---- retrieval MLM and pre-training with a pre-text ----------------------------------------------------------------------------------
def test_retrieval_prompt_against_reference(golden_dir):
    """LAVENDER_Retrieval_MLM with a prompt (eval: the reference's per-pair prompt dropout is off): logits, labels, loss normalised by the
    B^2 labelled rows (Agent_Retrieval_MLM.step's count), every gradient"""
    import lavender_amd as LA
    from lavender_amd.agent import CrossEntropyIgnore
    g = np.load(os.path.join(golden_dir, "pretxt_retrieval_prompt.npz"))
    swin, bert, B, _, X = g["meta"].tolist()
    B, X = int(B), int(X)
    P, bc = _oracle_params(bert, swin)
    batch = make_batch(B, vocab=bc["vocab"], seed=4)
    batch.update(txt=torch.from_numpy(g["txt"]), vid=g["vid"].tolist())
    ref, ans_ref = PR.retrieval_forward(P, batch, swin, bc["heads"], ("prompt", _prompt(g)))
    torch.nn.functional.cross_entropy(ref.flatten(0, 1), ans_ref.flatten(), ignore_index=-1).backward()
    P["emb_task"].grad = None
    m = _model(LA.LAVENDER_Retrieval_MLM, swin, bert, B, "prompt")
    m.arena().zero_grad()
    b = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    b["prompt"] = _prompt(g)
    out, ans = m(b)
    Lp = len(g["prompt"])
    assert out.shape == (B * B, Lp + X, bc["vocab"]) and (ans.cpu().numpy() == g["ans"]).all()
    _check_logits(out, g, "retrieval/prompt")
    ls = CrossEntropyIgnore()(out.flatten(0, 1), ans.flatten(), out.shape[0])          # the count Agent_Retrieval_MLM.step passes
    ls.backward()
    torch.cuda.synchronize()
    assert abs(ls.item() - g["loss"][0]) < 1e-2
    _grad_check(m, P)
    _check_emb_task(m, P, None)


def test_retrieval_eval_feat_cross_with_per_text_prompt(golden_dir):
    """LAVENDER_RetrievalMlmEval 'feat' with 2-D prompt_txt / prompt_mask (eval_retrieval_mlm.py:24,154-162: a prompt block per text, the
    pre_stride = Lp * H mode) and 'cross' on the cached features, against the restatement"""
    import lavender_amd as LA
    from oracle import lavender_ref as R
    g = np.load(os.path.join(golden_dir, "pretxt_retrieval_prompt.npz"))
    B, X = 3, 32
    P, bc = _oracle_params("micro", "micro")
    b = make_batch(B, vocab=bc["vocab"], seed=4)
    ids = torch.from_numpy(g["prompt"]).long()
    p_txt = ids.unsqueeze(0).repeat(B, 1)
    p_txt[1, 2] = 2003                                           # texts get different prompts: the per-text blocks are really read per text
    p_mask = torch.ones_like(p_txt)
    m = _model(LA.LAVENDER_RetrievalMlmEval, "micro", "micro", B, "prompt")
    with torch.no_grad():
        f_img, m_img, f_txt, m_txt, txt = m("feat", {"img": b["img"].unsqueeze(1).cuda(), "txt": b["txt"].cuda(), "mask": b["mask"].cuda(),
                                                   "prompt_txt": p_txt.cuda(), "prompt_mask": p_mask.cuda()})
        Lp = p_txt.shape[1]
        assert f_txt.shape == (B, Lp + X, f_img.shape[-1]) and torch.equal(txt.cpu(), torch.cat([p_txt, b["txt"]], 1))
        assert torch.equal(m_txt.cpu(), torch.cat([p_mask, b["mask"]], 1))
        ref_txt = torch.cat([R.enc_txt(P, p_txt), R.enc_txt(P, b["txt"])], 1)
        d = (f_txt.float().cpu() - ref_txt).abs().max().item()
        print("feat: text rows max |d|", d)
        assert d < 3e-2
        vi, ti = np.repeat(np.arange(B), B), np.tile(np.arange(B), B)
        out, _ = m("cross", {"feat_img": f_img[vi], "mask_img": m_img[vi], "feat_txt": f_txt[ti], "mask_txt": m_txt[ti]})
    f_ref, mi_ref = R.enc_video(P, b["img"], "micro")
    x = PR.encoder(P, torch.cat([f_ref[vi], ref_txt[ti]], 1), torch.cat([mi_ref[vi], m_txt.cpu()[ti]], 1), bc["heads"])
    ref = R.mlm_head(P, x[:, f_ref.shape[1]:])
    d = (out.float().cpu() - ref).abs()
    print("cross: logits max", d.max().item(), "mean", d.mean().item())
    assert d.max() < 3e-2 and d.mean() < 5e-3


@pytest.mark.parametrize("kind", ["task", "prompt"])
def test_pretrain_vtm_pretxt_against_reference(golden_dir, kind):
    """LAVENDER_Pretrain_MLM with the "vtm" task token / vtm_prompt (main_pretrain_mlm.py:55-119): MTM on the plain text, VTM on
    [pre-text ; text], same negatives (numpy draws), logits / labels / losses / gradients"""
    import lavender_amd as LA
    from lavender_amd.agent import CrossEntropyIgnore
    g = np.load(os.path.join(golden_dir, f"pretxt_pretrain_{kind}.npz"))
    swin, bert, B, _, X = g["meta"].tolist()
    B, X = int(B), int(X)
    P, bc = _oracle_params(bert, swin)
    batch = make_batch(B, vocab=bc["vocab"], seed=1)
    batch.update(txt=torch.from_numpy(g["txt"]), ans_mtm=torch.from_numpy(g["ans_mtm"]))
    spec = ("task", 0) if kind == "task" else ("prompt", _prompt(g))
    np.random.seed(88)
    ref = PR.pretrain_forward(P, batch, swin, bc["heads"], spec)
    lf = lambda o, a: torch.nn.functional.cross_entropy(o.flatten(0, 1), a.flatten(), ignore_index=-1)
    (lf(ref["out_mtm"], ref["ans_mtm"]) + lf(ref["out_vtm"], ref["ans_vtm"])).backward()
    if kind == "prompt":
        P["emb_task"].grad = None
    m = _model(LA.LAVENDER_Pretrain_MLM, swin, bert, B, kind)
    m.arena().zero_grad()
    b = {k: v.cuda() for k, v in batch.items()}
    if kind == "prompt":
        b["vtm_prompt"] = _prompt(g)
    np.random.seed(88)
    out = m(b)
    Lp = 1 if kind == "task" else len(g["prompt"])
    assert out["out_vtm"].shape[1] == Lp + X and out["out_mtm"].shape[1] == X
    assert (out["ans_vtm"].cpu().numpy() == g["ans"]).all()
    _check_logits(out["out_vtm"], g, f"pretrain/{kind} vtm")
    lse = torch.logsumexp(out["out_mtm"].detach().float().cpu(), -1).numpy()
    assert np.abs(lse - g["mtm_lse"]).max() < 2e-2
    ce = CrossEntropyIgnore()
    ls_m = ce(out["out_mtm"].flatten(0, 1), out["ans_mtm"].flatten(), count=int((batch["ans_mtm"] != -1).sum()))
    ls_v = ce(out["out_vtm"].flatten(0, 1), out["ans_vtm"].flatten(), count=out["out_vtm"].shape[0])
    (ls_m + ls_v).backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose([ls_m.item(), ls_v.item()], g["losses"], atol=1e-2)
    _grad_check(m, P)
    _check_emb_task(m, P, 0 if kind == "task" else None)


# ---- two data-parallel ranks with different task tokens --------------------------------------------------------------------------------
def _dp_task_worker(rank, port, q):
    import sys
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    import lavender_amd as LA
    from tests.helpers import Tok, make_args
    args = make_args("micro", "micro", 2, lr=1e-3, size_vocab=-1, enable_task_token=True)
    m = LA.LAVENDER_QAOE_MLM(args, Tok()).cuda()
    m.arena()
    agent = LA.Agent_QAOE_MLM(args, m)
    agent.prepare_dist_model()
    tasks = ("oe", "mc")

    def grads(r):
        b = make_batch(2, X=16, vocab=BERT_CFGS["micro"]["vocab"], seed=20 + r)
        ans = torch.full(b["txt"].shape, -1, dtype=torch.long)
        ans[:, -1] = torch.tensor([1016, 1014])
        b.update(mask_ans=ans, task_name=tasks[r])
        m.eval()
        m.arena().zero_grad()
        out, a = m({k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in b.items()})
        agent.loss_func(out.flatten(0, 1), a.flatten()).backward()
        return m.emb_task.grad.detach().clone()

    listeners, m.arena().listeners = m.arena().listeners, []
    g_local = [grads(0), grads(1)]
    m.arena().listeners = listeners
    agent.dp.begin_step()
    grads(rank)
    agent.dp.finish()
    torch.cuda.synchronize()
    g = m.emb_task.grad.detach()
    want = g_local[0] + g_local[1]
    q.put((rank, float((g - want).abs().max()), float(want.abs().max()), float(g[[0, 3]].abs().max()),
           float(g_local[0][1].abs().max()), float(g_local[1][2].abs().max())))
    dist.destroy_process_group()


def test_two_ranks_different_task_tokens_sum_emb_task_gradients():
    """rank 0 trains "oe", rank 1 "mc" (two processes on the one visible device, process group over gloo -- tests/test_gpu_dp.py's set-up):
    after the exchange both ranks hold emb_task gradients equal to the sum of the two local ones; rows of unused tasks stay zero"""
    import queue as _queue
    import time as _time
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29900 + (os.getpid() % 500)
    ps = [ctx.Process(target=_dp_task_worker, args=(r, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res, t0 = [], _time.time()
    while len(res) < 2:
        try:
            res.append(q.get(timeout=2))
        except _queue.Empty:
            if any(p.exitcode not in (None, 0) for p in ps) or _time.time() - t0 > 300:
                for p in ps:
                    if p.is_alive():
                        p.terminate()
                pytest.fail(f"worker failed (exit codes {[p.exitcode for p in ps]})")
    for p in ps:
        p.join(timeout=60)
    for rank, d, scale, unused, own0, own1 in sorted(res):
        print("rank", rank, "max |sum - exchanged|", d, "scale", scale)
        assert d <= 1e-6 * scale + 1e-9 and unused == 0.0
        assert own0 == 0.0 and own1 == 0.0                       # rank 0's local gradient has no "mc" row, rank 1's no "oe" row
