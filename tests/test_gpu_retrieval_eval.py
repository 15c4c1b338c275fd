"""GPU: the text-to-video retrieval evaluation (eval_retrieval_mlm.py:138-247) -- the [MASK]-row kernels against float64, the rows-only last
fusion layer against the full layer, the pair scorer against 'cross' + fc_mtm and the float64 oracle, the evaluator's invariances, and the root
script on synthetic clips.

Bounds: every GPU result is held to |got - ref64| <= 2 * |full GPU path - ref64| + floor, where the full path is the existing kernel sequence
(lav_bert_layer_fwd / 'cross' + BertOnlyMLMHead) on the same inputs: the rows-only path does the same arithmetic on fewer rows and keeps the
residual stream of the last layer in fp32, so it may not be worse than the path it replaces.  The kernels themselves get first-principles bounds
(bf16 output rounding 2^-8 relative + fp32 accumulation over the contraction)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import BERT_CFGS, make_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
F64 = torch.float64
U32 = 2.0 ** -24


def _bf(t):
    return t.to(torch.bfloat16)


# ---- lav_attention_rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L, heads, n", [(17, 2, 5), (276, 12, 3), (1024, 2, 7)])
def test_attention_rows_against_float64(L, heads, n):
    from lavender_amd import hip as K
    g = torch.Generator().manual_seed(L)
    H = heads * 64
    qkv = _bf(torch.randn(n * L, 3 * H, generator=g) * 0.8)
    mask = torch.ones(n, L, dtype=torch.int32)
    for s in range(n):                                       # padded text tails / masked video rows, different per sequence
        mask[s, L - 1 - s % 3:] = 0 if s % 2 else 1
        mask[s, :s] = 0
    Lv = L // 2
    q_row = torch.tensor([[Lv, (Lv + L) // 2, L - 1][s % 3] for s in range(n)], dtype=torch.int32)
    for s in range(n):
        mask[s, q_row[s]] = 1
    out = K.attention_rows(qkv.cuda(), n, L, heads, mask.cuda(), q_row.cuda())
    out2 = K.attention_rows(qkv.cuda(), n, L, heads, mask.cuda(), q_row.cuda())
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))         # no atomics: identical bits
    x = qkv.to(F64).view(n, L, 3, heads, 64)
    ref = torch.empty(n, H, dtype=F64)
    for s in range(n):
        q = x[s, q_row[s], 0]                                                 # (heads, 64)
        k, v = x[s, :, 1], x[s, :, 2]                                         # (L, heads, 64)
        sc = torch.einsum("hd,lhd->hl", q, k) * 0.125
        sc = sc.masked_fill(mask[s][None, :] == 0, float("-inf"))
        p = sc.softmax(-1)
        ref[s] = torch.einsum("hl,lhd->hd", p, v).reshape(H)
    got = out.cpu().to(F64)
    vmax = x[:, :, 2].abs().amax()
    bound = 2.0 ** -8 * ref.abs() + 64 * L * U32 * vmax
    err = (got - ref).abs()
    print(f"attention_rows L={L}: max err {err.max():.3e}, max bound ratio {(err / bound).max():.3f}")
    assert (err <= bound).all()


# ---- lav_mlm_pair_readout ----------------------------------------------------------------------------------------------------------------------
def test_mlm_pair_readout_against_float64():
    from lavender_amd import _lib as L, hip as K
    g = torch.Generator().manual_seed(3)
    n, H, V, tid, fid = 13, 256, 1000, 7, 991
    x = _bf(torch.randn(n, H, generator=g))
    wd, bd = _bf(torch.randn(H, H, generator=g) / 16), torch.randn(H, generator=g) * 0.1
    gam, bet = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    wdec, bdec = _bf(torch.randn(V, H, generator=g) / 16), torch.randn(V, generator=g)
    d = {k: v.cuda() for k, v in dict(x=x, wd=wd, bd=bd, gam=gam, bet=bet, wdec=wdec, bdec=bdec).items()}
    S = torch.full((4, 5), -7.0, device="cuda")
    rows = torch.tensor([k % 4 for k in range(n)], dtype=torch.int32, device="cuda")
    cols = torch.tensor([(k // 4) if k < 12 else 9 for k in range(n)], dtype=torch.int32, device="cuda")   # pair 12 lands outside: skipped
    t = torch.empty(n, H, device="cuda")
    lg = torch.empty(n, 2, device="cuda")
    desc = L.MlmPairReadoutDesc(n, H, V, tid, fid, 1e-12, d["x"].data_ptr(), H, d["wd"].data_ptr(), d["bd"].data_ptr(), d["gam"].data_ptr(),
                                d["bet"].data_ptr(), d["wdec"].data_ptr(), H, d["bdec"].data_ptr(), t.data_ptr(), rows.data_ptr(), cols.data_ptr(),
                                S.data_ptr(), 5, 4, 5, lg.data_ptr())
    K.mlm_pair_readout(desc)
    torch.cuda.synchronize()
    th = torch.nn.functional.gelu(x.to(F64) @ wd.to(F64).T + bd.to(F64))
    mu, var = th.mean(-1, keepdim=True), th.var(-1, unbiased=False, keepdim=True)
    tn = (th - mu) / torch.sqrt(var + 1e-12) * gam.to(F64) + bet.to(F64)
    w2 = wdec.to(F64)[[tid, fid]]
    ref = tn @ w2.T + bdec.to(F64)[[tid, fid]]
    # fp32 GEMM (K = H) into the LayerNorm, fp32 dot products over H: relative fp32 accumulation errors, scaled by the absolute sums
    scale = (tn.abs() @ w2.abs().T) + bdec.to(F64)[[tid, fid]].abs()
    err = (lg.cpu().to(F64) - ref).abs()
    bound = 4 * H * U32 * scale * 8
    print(f"readout: max err {err.max():.3e}, max bound ratio {(err / bound).max():.3f}")
    assert (err <= bound).all()
    Sh, lh = S.cpu(), lg.cpu()
    for k in range(12):                                      # s = pt / (pt + pf) of the kernel's own fp32 logits, at (out_row, out_col)
        assert Sh[k % 4, k // 4].item() == (lh[k, 0] / (lh[k, 0] + lh[k, 1])).item()
    assert (Sh[:, 3:] == -7.0).all()                         # nothing else written; the pair whose column is outside was skipped


# ---- lav_retrieval_rank ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt, nv", [(9, 1), (33, 70), (5, 700)])
def test_rank_kernel_bit_exact_against_host_rule(nt, nv):
    from lavender_amd import hip as K
    from lavender_amd.retrieval_eval import ranks_host
    rng = np.random.default_rng(nt * nv)
    S = (np.round(rng.random((nt, nv)) * 16) / 16).astype(np.float32)
    S[rng.random((nt, nv)) < 0.05] = np.nan
    S[rng.random((nt, nv)) < 0.03] = np.inf
    S[rng.random((nt, nv)) < 0.03] = -np.inf
    S[rng.random((nt, nv)) < 0.03] = -0.0
    gt = rng.integers(0, nv, nt).astype(np.int32)
    S[0, gt[0]] = np.nan
    r = K.retrieval_rank(torch.from_numpy(S).cuda(), torch.from_numpy(gt).cuda()).cpu().numpy()
    assert r.tolist() == ranks_host(S, gt).tolist()


# ---- the model: micro fixture -------------------------------------------------------------------------------------------------------------------
def _micro(B=4, Cl=2, T=2, seed=9):
    """4 videos x 2 clips and 6 captions (videos 0 and 1 have two captions each), every caption ending in [MASK]"""
    from tests.helpers import build_filled_model
    from lavender_amd import LAVENDER_RetrievalMlmEval
    bc = BERT_CFGS["micro"]
    b = make_batch(B * Cl, T=T, vocab=bc["vocab"], seed=seed)
    img = b["img"].view(B, Cl, T, 3, 224, 224)
    tb = make_batch(6, T=1, vocab=bc["vocab"], seed=seed + 1)
    txt, mask = tb["txt"].clone(), tb["mask"].clone()
    txt[:, -1], mask[:, -1] = 103, 1
    body = txt[:, :-1]
    body[body == 103] = 104
    m = build_filled_model("micro", "micro", B, cls=LAVENDER_RetrievalMlmEval).eval()
    vid_of_text = [0, 0, 1, 1, 2, 3]
    return m, img, txt, mask, vid_of_text


def _feat(m, img, txt, mask):
    with torch.no_grad():
        f_img, m_img, _, _, _ = m('feat', {"img": img.cuda(), "txt": txt[:img.shape[0]].cuda(), "mask": mask[:img.shape[0]].cuda()})
        _, _, f_txt, m_txt, t = m('feat', {"img": img[:1].expand(txt.shape[0], -1, -1, -1, -1, -1).contiguous().cuda(), "txt": txt.cuda(),
                                           "mask": mask.cuda()})
    return f_img, m_img, f_txt, m_txt, t


def _ref64_layer(layer, x, res, key_mask, n, L, q, rb=lambda t: t):
    """float64 BertLayer on the bf16 working weights: all rows give K / V, the selected rows the rest.  rb: the rounding model of
    lav_bert_layer_fwd_rows (tests/rounding_model.py's convention) -- the tensors it stores as bf16 (qkv, the attention context, the LN1 output
    as the FFN1 operand, the GELU output) are rounded there; the residual stream (pre1, LN1 output, pre2) stays fp32 / exact."""
    from lavender_amd import engine as E
    Hd = x.shape[1]
    arena = layer._arena()
    att, ao, inter, outp = layer.attention.self, layer.attention.output, layer.intermediate, layer.output
    wqkv, _, _ = arena.fused_view(att.query.weight, 3 * Hd)
    _, _, bqkv = arena.fused_view(att.query.bias, 3 * Hd)
    d = lambda t: t.detach().cpu().to(F64)
    qkv = rb(d(x) @ d(wqkv).T + d(bqkv)).view(n, L, 3, layer.num_heads, 64)
    sel = torch.arange(n)
    qs = qkv[sel, q, 0]
    sc = torch.einsum("nhd,nlhd->nhl", qs, qkv[:, :, 1]) * 0.125
    sc = sc.masked_fill(d(key_mask)[:, None, :] == 0, float("-inf"))
    cx = rb(torch.einsum("nhl,nlhd->nhd", sc.softmax(-1), qkv[:, :, 2]).reshape(n, Hd))
    ln = lambda v, m: torch.nn.functional.layer_norm(v, (Hd,), d(m.weight), d(m.bias), m.eps)
    pre1 = res + cx @ d(E.W16(ao.dense.weight)).T + d(ao.dense.bias)
    x1 = ln(pre1, ao.LayerNorm)
    h = rb(torch.nn.functional.gelu(rb(x1) @ d(E.W16(inter.dense.weight)).T + d(inter.dense.bias)))
    return ln(x1 + h @ d(E.W16(outp.dense.weight)).T + d(outp.dense.bias), outp.LayerNorm)


_RB = lambda t: t.to(torch.bfloat16).to(F64)


def test_bert_layer_rows_against_the_full_layer_for_each_residual_form():
    """the last layer of the pair scorer against lav_bert_layer_fwd at the [MASK] rows, for the residual forms _encode hands the last layer:
    RESLN pre-LayerNorm rows as fp16 (default) and as fp32 (LAV_STREAM_DTYPE=fp32), plain fp32 rows, and the bf16 input itself"""
    from lavender_amd import engine as E, hip as K
    m, img, txt, mask, _ = _micro()
    f_img, m_img, f_txt, m_txt, t = _feat(m, img, txt, mask)
    with torch.no_grad():
        src = m.pair_source(f_img, m_img, f_txt, m_txt, t)
        vi, ti = np.array([0, 1, 2, 3, 0, 3, 1]), np.array([0, 1, 2, 3, 5, 4, 2])
        n, Lv, X = len(vi), src.Lv, src.X
        L = Lv + X
        km = K.pair_key_mask(src.mask_img, src.mask_txt, vi, ti)
        flat = torch.from_numpy(E.pair_index(src.n_video, Lv, src.n_text, X, vi, ti).reshape(-1)).cuda()
        x = K.gather_rows(src.src, flat, n * L, src.src.shape[1])
        arena = m.arena()
        lyr0, lyr = m.trsfr.layer[0], m.trsfr.layer[1]
        o = E.BertLayerFn.apply(arena.anchor, x, None, lyr0, km, n, L, 0.0, 0.0, True, 0, None)
        assert len(o) == 4, "default configuration: RESLN carriers"
        ln0 = lyr0.output.LayerNorm
        x1, pre, mean, rstd = o
        q = Lv + src.q_row[ti]
        sel = torch.from_numpy(np.arange(n) * L + q).cuda()
        q_d = torch.from_numpy(q.astype(np.int32)).cuda()
        sel32 = sel.to(torch.int32)
        full = E.BertLayerFn.apply(arena.anchor, x1, (pre, mean, rstd, ln0.weight.data, ln0.bias.data), lyr, km, n, L, 0.0, 0.0, False, 0, None)[0]
        pre32 = pre.float()
        ln_rows = torch.nn.functional.layer_norm(pre32.double(), (pre.shape[1],), ln0.weight.data.double(), ln0.bias.data.double(), ln0.eps)
        forms = {"resln_fp16": (pre, mean, rstd, ln0.weight.data, ln0.bias.data), "resln_fp32": (pre32, mean, rstd, ln0.weight.data, ln0.bias.data),
                 "fp32_rows": ln_rows.float().contiguous(), "bf16_input": None}
        full_rows = full.view(n * L, -1)[sel].cpu().to(F64)
        res64 = ln_rows.cpu()[sel.cpu()]
        ref_full = _ref64_layer(lyr, x1, res64, km, n, L, torch.from_numpy(q))
        err_full = (full_rows - ref_full).abs().max().item()
        qt = torch.from_numpy(q)
        for name, x32 in forms.items():
            y, y32 = E.bert_layer_rows_eval(x1, x32, lyr, km, n, L, q_d, sel32)
            res_in = res64 if x32 is not None else x1.view(n * L, -1)[sel].cpu().to(F64)
            r64 = _ref64_layer(lyr, x1, res_in, km, n, L, qt)
            # the bound: what the path's own bf16 stores cost in float64 (rounding model), x3, plus an fp32 accumulation floor
            dev = (_ref64_layer(lyr, x1, res_in, km, n, L, qt, rb=_RB) - r64).abs().max().item()
            err = (y32.cpu().to(F64) - r64).abs().max().item()
            vs_full = (y32.cpu().to(F64) - full_rows).abs().max().item()
            print(f"{name}: rows vs float64 {err:.3e} (rounding model {dev:.3e}), full layer vs float64 {err_full:.3e}, rows vs full {vs_full:.3e}")
            assert err <= 3 * dev + 2.0 ** -14, name
            if x32 is not None:
                assert vs_full <= 3 * err_full + 2.0 ** -10, name
            yb = (y.cpu().float() - y32.cpu()).abs()
            assert (yb <= 2.0 ** -8 * y32.cpu().abs() + 1e-30).all()


# ---- score_pairs ---------------------------------------------------------------------------------------------------------------------------------
def test_score_pairs_against_cross_and_the_float64_oracle():
    from oracle import lavender_ref as R
    m, img, txt, mask, vot = _micro()
    bc = BERT_CFGS["micro"]
    P = R.filled_params("micro", hidden=bc["hidden"], layers=bc["layers"], ffn=bc["ffn"], vocab=bc["vocab"])
    f_img, m_img, f_txt, m_txt, t = _feat(m, img, txt, mask)
    Nt, Mv = txt.shape[0], img.shape[0]
    ti, vi = np.repeat(np.arange(Nt), Mv), np.tile(np.arange(Mv), Nt)        # Dataset_Product order: text outer, video inner
    with torch.no_grad():
        src = m.pair_source(f_img, m_img, f_txt, m_txt, t)
        lg = torch.empty(len(vi), 2, device="cuda")
        s = m.score_pairs(src, vi, ti, logits=lg)
        out, _ = m('cross', {"feat_img": f_img[torch.from_numpy(vi).cuda()], "mask_img": m_img[torch.from_numpy(vi).cuda()],
                             "feat_txt": f_txt[torch.from_numpy(ti).cuda()], "mask_txt": m_txt[torch.from_numpy(ti).cuda()]})
        rf_img, rm_img, rf_txt = R.retrieval_eval_feat(P, img, txt, "micro")
        ref = R.retrieval_eval_cross(P, rf_img[vi], rm_img[vi], rf_txt[ti], mask[ti], bc["heads"])
    torch.cuda.synchronize()
    q = torch.from_numpy(src.q_row[ti])
    k = torch.arange(len(vi))
    pair64 = torch.stack([ref[k, q, 2995], ref[k, q, 6270]], 1).to(F64)
    cross = torch.stack([out[k.cuda(), q.cuda(), 2995], out[k.cuda(), q.cuda(), 6270]], 1).float().cpu().to(F64)
    ours = lg.cpu().to(F64)
    e_cross = (cross - pair64).abs().max().item()
    e_ours = (ours - pair64).abs().max().item()
    print(f"score_pairs (pt, pf) vs float64 oracle {e_ours:.3e}; 'cross' + fc_mtm vs oracle {e_cross:.3e}; ours vs cross {(ours - cross).abs().max():.3e}")
    assert e_ours <= 2 * e_cross + 2.0 ** -10
    assert (ours - cross).abs().max().item() <= 3 * e_cross + 2.0 ** -10
    s_ref = pair64[:, 0] / pair64.sum(1)
    s_got = s.cpu().to(F64)
    assert torch.equal(s_got, (ours[:, 0].float() / (ours[:, 0].float() + ours[:, 1].float())).to(F64))
    # the reference itself (tests/golden/make_goldens_retrieval_eval.py: its LAVENDER_RetrievalMlmEval + Dataset_Product on the same inputs)
    g = np.load(os.path.join(ROOT, "tests", "golden", "retr_rank_micro.npz"))
    assert g["pair_tid"].tolist() == ti.tolist() and g["pair_vid"].tolist() == vi.tolist()      # product order: text outer, video inner
    assert g["txt"].tolist() == txt.tolist() and g["video_of_text"].tolist() == list(vot)
    gold = torch.from_numpy(np.stack([g["p_true"], g["p_false"]], 1)).to(F64)
    e_gold = (ours - gold).abs().max().item()
    print(f"score_pairs (pt, pf) vs the reference's golden {e_gold:.3e}")
    assert e_gold <= 2 * e_cross + 2.0 ** -10
    # ranks: every text's rank lies in the interval the golden scores allow once scores closer than twice the measured score error are treated
    # as ties -- a single value (hence equality) wherever the golden margins are wider than that
    from lavender_amd.retrieval_eval import ranks_host
    S, S_g = s_got.view(Nt, Mv).numpy(), g["S"].astype(np.float64)
    tol = float(np.abs(S - S_g).max())
    gt = g["gt"]
    assert gt.tolist() == list(vot)
    r = ranks_host(S.astype(np.float32), gt)
    exact = 0
    for tt in range(Nt):
        d = S_g[tt] - S_g[tt, gt[tt]]
        others = np.arange(Mv) != gt[tt]
        lo = 1 + int(((d > 2 * tol) & others).sum())
        hi = 1 + int(((d >= -2 * tol) & others).sum())
        assert lo <= r[tt] <= hi, (tt, lo, int(r[tt]), hi)
        exact += lo == hi
        if lo == hi:
            assert r[tt] == g["ranks"][tt]
    print(f"ranks within the golden's interval for all {Nt} texts, pinned exactly for {exact} (score error {tol:.2e})")


# ---- evaluate_t2v --------------------------------------------------------------------------------------------------------------------------------
def _batches(img, txt, mask, vot, bs=4):
    out = []
    for i in range(0, txt.shape[0], bs):
        j = list(range(i, min(txt.shape[0], i + bs)))
        out.append({"img": img[[vot[k] for k in j]], "txt": txt[j], "mask": mask[j], "tid": j, "vid": [f"v{vot[k]}" for k in j]})
    return out


def test_evaluate_t2v_chunk_invariance_repeatability_and_separate_features():
    from lavender_amd.retrieval_eval import evaluate_t2v, ranks_host, score_matrix
    m, img, txt, mask, vot = _micro()
    gt = {k: f"v{v}" for k, v in enumerate(vot)}
    batches = _batches(img, txt, mask, vot)
    Mv = 4
    results = {}
    with torch.no_grad():
        for chunk in (1, 7, Mv, 6 * Mv, None):
            r = evaluate_t2v(m, batches, gt, pair_chunk=chunk, return_scores=True)
            results[chunk] = r
        again = evaluate_t2v(m, batches, gt, pair_chunk=7, return_scores=True)
    base = results[None]
    assert base["vids"] == ["v0", "v1", "v2", "v3"] and base["tids"] == list(range(6))
    for chunk, r in results.items():
        assert r["ranks"].tolist() == base["ranks"].tolist(), chunk
        assert {k: r[k] for k in ("r@1", "r@5", "r@10", "median")} == {k: base[k] for k in ("r@1", "r@5", "r@10", "median")}
    S7 = results[7]["scores"].cpu()
    assert torch.equal(S7.view(torch.int32), again["scores"].cpu().view(torch.int32))
    assert ranks_host(S7.numpy(), np.array(vot)).tolist() == base["ranks"].tolist()
    # the same features held in separate tensors (not one buffer): pair_source joins them once, S is unchanged
    from lavender_amd import engine as E
    from lavender_amd.retrieval_eval import collect_features
    _, _, src0 = collect_features(m, batches)
    Lv = src0.Lv
    f_img = src0.src[:Mv * Lv].view(Mv, Lv, -1).clone()
    f_txt = src0.src[Mv * Lv:].view(6, src0.X, -1).clone()
    assert not E.rows_adjacent(f_img, f_txt)
    with torch.no_grad():
        src = m.pair_source(f_img, src0.mask_img.clone(), f_txt, src0.mask_txt.clone(), txt.cuda())
        S_sep = score_matrix(m, src, 0, 6, pair_chunk=7).cpu()
    assert torch.equal(S_sep.view(torch.int32), S7.view(torch.int32))
    # evaluation only
    with pytest.raises(RuntimeError):
        evaluate_t2v(m, batches, gt)                                           # gradients enabled
    m.train()
    with torch.no_grad(), pytest.raises(RuntimeError):
        evaluate_t2v(m, batches, gt)
    with torch.no_grad(), pytest.raises(RuntimeError):
        m.score_pairs(src, [0], [0])
    m.eval()


def test_ret_rows_off_gives_the_reference_formulation():
    """LAV_RET_ROWS=0: full last layer + full-vocabulary head, two columns sliced -- same ranks on the micro fixture, scores within the bound"""
    import lavender_amd.retrieval_mlm as RM
    m, img, txt, mask, vot = _micro()
    f_img, m_img, f_txt, m_txt, t = _feat(m, img, txt, mask)
    Nt, Mv = 6, 4
    ti, vi = np.repeat(np.arange(Nt), Mv), np.tile(np.arange(Mv), Nt)
    with torch.no_grad():
        src = m.pair_source(f_img, m_img, f_txt, m_txt, t)
        lg_rows, lg_full = torch.empty(Nt * Mv, 2, device="cuda"), torch.empty(Nt * Mv, 2, device="cuda")
        m.score_pairs(src, vi, ti, logits=lg_rows)
        RM.RET_ROWS = False
        try:
            m.score_pairs(src, vi, ti, logits=lg_full)
        finally:
            RM.RET_ROWS = True
    d = (lg_rows - lg_full).abs().max().item()
    print(f"rows vs full-vocabulary logits: {d:.3e}")
    assert d < 3e-2


# ---- the root script -----------------------------------------------------------------------------------------------------------------------------
def test_eval_script_on_synthetic_clips_writes_the_reference_results_json(tmp_path):
    from tests.helpers import hf_cfg
    cfg = hf_cfg("micro")
    c = dict(type="retrieval", task="msrvtt-retrieval", dataset="msrvtt", vis_backbone_size="micro", vis_backbone_init="random", kinetics=400,
             txt_backbone=cfg, fusion_encoder=cfg, tokenizer=cfg, txt_backbone_embed_only=True, fusion_encoder_rand_init=True,
             size_img=224, size_frame=2, size_txt=15, n_workers=0, seed=88)
    p = tmp_path / "args_msrvtt-retrieval.json"
    p.write_text(json.dumps(c))
    out = tmp_path / "out"
    env = dict(os.environ, LAV_SYNTH_VIDEOS="5", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_retrieval_mlm.py"), "--config", str(p), "--path_output", str(out),
                        "--multi_clip_testing", "true"], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "initial weights" in r.stdout and "synthetic" in r.stdout
    log = json.load(open(out / "retrieval_mlm_results.json"))
    assert set(log) == {"test", "multi_clip_testing"} and log["multi_clip_testing"] is True
    assert set(log["test"]) == {"r@1", "r@5", "r@10", "median"}
    assert all(isinstance(v, str) for v in log["test"].values()) and log["test"]["median"].isdigit()
    assert 1 <= int(log["test"]["median"]) <= 5
