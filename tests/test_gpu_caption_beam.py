"""Beam-search caption generation on the MI355X (lavender_amd/caption_decode.py, csrc/decode.hip): the beam kernels against fp32 torch and
the host bookkeeping, the cached beam search of the micro model against the reference golden (tests/golden/make_goldens_caption_beam.py),
the cached path against the full-recompute loop (LAV_CAP_KV=0) at the Base size, chunking, side effects and determinism."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import BERT_CFGS, make_batch
from tests.test_gpu_caption_generate import LOGIT_MAX, LOGIT_MEAN, _attn_ref, _bf

pytestmark = pytest.mark.gpu
CLS, SEP, PAD, MASK = 101, 102, 0, 103


def _cfg(nb, K, L, **kw):
    from lavender_amd import caption_decode as CD
    from lavender_amd.args import EasyDict
    return CD.BeamConfig(EasyDict(num_beams=nb, num_keep_best=K, max_gen_length=L, **kw), 64)


# ---- kernels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [30522, 1000, 257])
@pytest.mark.parametrize("nb", [2, 5, 8])
def test_beam_step(V, nb):
    from lavender_amd import hip as K
    from lavender_amd import caption_decode as CD
    R, cur, L = 3 * nb, 6, 12
    g = torch.Generator().manual_seed(V + nb)
    logits = torch.randn(R, V, generator=g) * 3
    logits[0, 5] = logits[0, V - 1] = logits[0, V // 2] = 40.0          # planted ties: the lower index first
    logits[1] = torch.round(logits[1])                                   # ties everywhere
    ids = torch.randint(0, min(V, 200), (R, L), generator=g)
    ids[:, 0] = 1
    ids[0, 1:cur] = torch.tensor([10, 11, 12, 13, 14])
    ids[2, 1:cur] = torch.tensor([7, 7, 8, 9, 9])
    logits[2, 7], logits[2, 8], logits[2, 9] = 30.0, -4.0, 29.5           # penalised ids of both signs, repeated once
    bs = torch.randn(R, generator=g) * 5
    bs[nb:2 * nb] = -1e9
    for pen in (1.0, 1.3):
        ref_s, ref_w = CD.host_beam_candidates(logits, ids, cur, pen, bs, nb)
        d_log = logits.cuda()
        cs = torch.empty(R, 2 * nb, device="cuda")
        cw = torch.empty(R, 2 * nb, dtype=torch.int32, device="cuda")
        K.beam_step(d_log, V, ids.cuda(), cur, pen, bs.cuda(), nb, cs, cw)
        torch.cuda.synchronize()
        # rows at -1e9 (the unused beams of step 1) have every score tied in fp32: their order is the clip merge's business (they never win
        # there), so only their scores are compared
        live = bs > -1e8
        assert torch.equal(cw.cpu()[live], ref_w[live]), (cw[:3].tolist(), ref_w[:3].tolist())
        torch.testing.assert_close(cs.cpu(), ref_s, atol=2e-5, rtol=1e-6)
        assert cw[0, :3].tolist() == [5, V // 2, V - 1]
        pl = CD.apply_repetition_penalty(logits.clone(), ids[:, :cur], pen)     # the penalty is applied in place
        assert torch.equal(d_log.cpu(), pl)


def _random_cands(R, nb, V, g, eos_rate):
    s = -torch.rand(R, 2 * nb, generator=g) * 6
    s = torch.round(s * 8) / 8                                           # exact ties within and across beams
    s, _ = torch.sort(s, dim=1, descending=True)
    w = torch.stack([torch.randperm(V, generator=g)[:2 * nb] for _ in range(R)]).to(torch.int32)
    w[torch.rand(R, 2 * nb, generator=g) < eos_rate] = SEP
    for r in range(R):                                                   # one row never repeats a word
        seen = set()
        for j in range(2 * nb):
            while int(w[r, j]) in seen:
                w[r, j] = (int(w[r, j]) + 1) % V
            seen.add(int(w[r, j]))
    return s, w


@pytest.mark.parametrize("nb,K,alpha,early", [(3, 2, 1.0, False), (5, 5, 0.6, False), (2, 1, 2.0, True), (8, 3, 0.0, False), (4, 2, 1.0, True)])
def test_beam_select_matches_host(nb, K, alpha, early):
    """the device select and the host bookkeeping on identical fp32 candidates over a whole generation: every state tensor bit for bit"""
    from lavender_amd import hip as K_
    from lavender_amd import caption_decode as CD
    clips, L, V = 5, 10, 300
    cfg = _cfg(nb, K, L, length_penalty=alpha, early_stopping=early)
    R = clips * nb
    host = CD.BeamState(clips, cfg, CLS, PAD, "cpu")
    dev = CD.BeamState(clips, cfg, CLS, PAD, "cuda")
    cs, cw = torch.empty(R, 2 * nb, device="cuda"), torch.empty(R, 2 * nb, dtype=torch.int32, device="cuda")
    nxt = torch.full((R, 2), -1, dtype=torch.long, device="cuda")
    desc = K_.beam_select_desc(clips, nb, K, V, L, early, SEP, PAD, cs, cw, *dev.tensors()[:3], *dev.tensors()[3:], next_ids=nxt, ld_next=2)
    g = torch.Generator().manual_seed(nb * 10 + K)
    for cur in range(1, L):
        s, w = _random_cands(R, nb, V, g, 0.25 if cur > 1 else 0.5)
        s = s + host.beam_scores[:, None]
        cs.copy_(s)
        cw.copy_(w)
        words = CD.host_beam_select(s, w, host, cur, cfg, V, SEP, PAD)
        K_.beam_select(desc, cur, cfg.norm(cur), cfg.norm(L))
        torch.cuda.synchronize()
        for name, a, b in zip(("beam_scores", "ids", "parent", "hyp_ids", "hyp_score", "hyp_seq", "state", "worst"), host.tensors(), dev.tensors()):
            assert torch.equal(a, b.cpu()), (cur, name, a.tolist(), b.cpu().tolist())
        assert torch.equal(nxt[:, 0].cpu(), words) and (nxt[:, 1] == -1).all()
    assert int(host.state[:, 0].min()) == K                               # every slot filled
    ids, lp = CD.finish_beams(dev.hyp_ids, dev.hyp_score, dev.hyp_seq)
    hi, hl = CD.finish_beams(host.hyp_ids, host.hyp_score, host.hyp_seq)
    assert torch.equal(ids.cpu(), hi) and torch.equal(lp.cpu(), hl)


def test_beam_reparent_is_a_copy():
    from lavender_amd import hip as K
    layers, R, heads, L = 12, 30, 12, 20
    g = torch.Generator(device="cuda").manual_seed(1)
    src = [(_bf(torch.randn(R, heads, L, 64, device="cuda", generator=g)), _bf(torch.randn(R, heads, L, 64, device="cuda", generator=g)))
           for _ in range(layers)]
    dst = [(torch.zeros_like(k), torch.zeros_like(v)) for k, v in src]
    parent = torch.randint(0, R, (R,), device="cuda", generator=g).to(torch.int32)
    parent[3] = -1                                                       # out of range: the row itself
    d = K.beam_reparent_desc(src, dst, parent, L)
    K.beam_reparent(d, 13)
    torch.cuda.synchronize()
    p = parent.long().clone()
    p[3] = 3
    for (sk, sv), (dk, dv) in zip(src, dst):
        assert torch.equal(dk[:, :, :13], sk[p, :, :13]) and torch.equal(dv[:, :, :13], sv[p, :, :13])
        assert (dk[:, :, 13:] == 0).all() and (dv[:, :, 13:] == 0).all()


@pytest.mark.parametrize("clips,nb", [(1, 5), (6, 5), (4, 8), (16, 2)])
@pytest.mark.parametrize("t", [1, 19])
def test_attention_decode_beam(clips, nb, t):
    """the beams of a clip read its prefix in place: against the existing entry on the prefix expanded nb times and against fp32 torch"""
    from lavender_amd import hip as K
    heads, Lv, max_len, q_len = 12, 250, 50, 2
    H, B = heads * 64, clips * nb
    g = torch.Generator().manual_seed(clips * 7 + nb + t)
    qkv_pre = _bf(torch.randn(clips, Lv, 3 * H, generator=g))
    mask = torch.ones(clips, Lv, dtype=torch.int32)
    for c in range(clips):
        mask[c, (11 * c) % 60: (11 * c) % 60 + 9] = 0
    ck, cv = _bf(torch.randn(B, heads, max_len, 64, generator=g)), _bf(torch.randn(B, heads, max_len, 64, generator=g))
    qkv_new = _bf(torch.randn(B, q_len, 3 * H, generator=g))
    outs, caches = [], []
    for beams in (nb, 1):
        pre, km = (qkv_pre, mask) if beams > 1 else (qkv_pre.repeat_interleave(nb, 0), mask.repeat_interleave(nb, 0))
        d_ck, d_cv = ck.cuda(), cv.cuda()
        out = torch.empty(B * q_len, H, dtype=torch.bfloat16, device="cuda")
        d_pre, d_km, d_new = pre.cuda(), km.cuda(), qkv_new.cuda()          # the descriptor holds raw pointers: keep the tensors alive
        desc = K.attn_decode_desc(B, heads, q_len, Lv, t - 1, 1, max_len, d_pre, d_km, d_new, d_ck, d_cv, out)
        part = torch.empty(B * heads * K.attention_decode_splits(desc) * q_len * 66, device="cuda")
        desc.partials, desc.partials_capacity = part.data_ptr(), part.numel()
        (K.attention_decode_beam(desc, beams) if beams > 1 else K.attention_decode(desc))
        torch.cuda.synchronize()
        outs.append(out.float().cpu())
        caches.append((d_ck.cpu(), d_cv.cpu()))
    d = (outs[0] - outs[1]).abs()
    assert d.max() < 2e-2 and d.mean() < 2e-3, (d.max().item(), d.mean().item())
    assert torch.equal(caches[0][0], caches[1][0]) and torch.equal(caches[0][1], caches[1][1])
    ref = _attn_ref(qkv_pre.repeat_interleave(nb, 0), mask.repeat_interleave(nb, 0), ck, cv, qkv_new, B, heads, Lv, t - 1, q_len)
    d = (outs[0].view(B, q_len, H) - ref).abs()
    assert d.max() < 2e-2 and d.mean() < 2e-3, (d.max().item(), d.mean().item())


# ---- the micro model against the reference golden ---------------------------------------------------------------------------------------
def _micro_beam(golden_dir, case, clips=2):
    from tests.helpers import build_filled_model
    from lavender_amd import LAVENDER_Captioning
    g = np.load(os.path.join(golden_dir, "cap_beam_micro_b2.npz"))
    nb, K, L, scale = int(g["meta"][0]), int(g["meta"][1]), int(g["meta"][2]), float(g["meta"][3])
    m = build_filled_model("micro", "micro", clips, cls=LAVENDER_Captioning)
    with torch.no_grad():
        m.fc_mtm.predictions.decoder.weight.mul_(scale)
    m.sync_weights()
    kw = {"plain": {}, "pen": dict(repetition_penalty=1.3), "alpha": dict(length_penalty=0.6)}[case]
    m.args.update(max_gen_length=L, num_beams=nb, num_keep_best=K, **kw)
    batch = make_batch(clips, vocab=BERT_CFGS["micro"]["vocab"], seed=6)
    return g, m, {k: v.cuda() for k, v in batch.items()}, batch


@pytest.mark.parametrize("case", ["plain", "pen", "alpha"])
def test_micro_beam_search_matches_golden(golden_dir, case):
    from tests.test_caption_beam_host import oracle_beam_step_fn
    from tests.test_caption_generate_host import _oracle_params
    from lavender_amd import caption_decode as CD
    g, m, batch, cpu_batch = _micro_beam(golden_dir, case)
    cfg = CD.make_config(m.args, 32)
    nb, L, sc = cfg.num_beams, cfg.max_len, float(g["meta"][3])
    forced = (torch.from_numpy(g["parents_" + case]), torch.from_numpy(g["words_" + case]))
    n = forced[0].shape[1]
    # teacher-forced: the golden's beams fed back; each beam's [MASK] logits (after the penalty) against the golden's
    steps, hist = [], []
    with torch.no_grad():
        CD.generate_beam(m.eval(), batch["img"], 32, cfg, kv=True, forced=forced, step_logits=steps)
        ora = []
        CD.host_beam_search(oracle_beam_step_fn(_oracle_params(sc), cpu_batch["img"]), 2, cfg, CLS, PAD, SEP, forced=forced, step_logits=ora,
                            trace=hist)
    # the penalty of each step on the ids the forced beams hold then (the oracle run's histories are those)
    pen = []
    ids = torch.full((2 * nb, L), PAD, dtype=torch.long)
    ids[:, 0] = CLS
    for i in range(n):
        pen.append(CD.apply_repetition_penalty(steps[i].float().cpu().clone(), ids[:, :i + 1], cfg.penalty))
        ora[i] = CD.apply_repetition_penalty(ora[i].float().clone(), ids[:, :i + 1], cfg.penalty)
        par = (torch.arange(2)[:, None] * nb + forced[0][:, i]).flatten()
        ids[:, :i + 1] = ids[par, :i + 1].clone()
        ids[:, i + 1] = forced[1][:, i].flatten()
    lg = torch.stack(pen, 1).view(2, nb, n, -1).transpose(1, 2)           # (B, steps, nb, V)
    cols = torch.from_numpy(g["cols"])
    d = (lg[..., cols] - torch.from_numpy(g["cols_" + case])).abs()
    dl = (torch.logsumexp(lg, -1) - torch.from_numpy(g["lse_" + case])).abs()
    print(case, "teacher-forced beam logits vs golden: max", d.max().item(), "mean", d.mean().item(), "lse max", dl.max().item())
    assert d.max() < sc * LOGIT_MAX and d.mean() < sc * LOGIT_MEAN and dl.max() < sc * LOGIT_MAX
    # free running through the public entry; the margin rule on the measured error (whole vocabulary, against the fp32 oracle that reproduces
    # the golden): a candidate score sums log-softmax values, each off by at most twice its row's logit error
    ids_out, lp = m({"img": batch["img"], "txt": batch["txt"], "mask": batch["mask"]}, is_decode=True)
    assert ids_out.shape == (2, cfg.keep, L) and lp.shape == (2, cfg.keep) and ids_out.dtype == torch.long
    err = (lg - torch.stack(ora, 1).view(2, nb, n, -1).transpose(1, 2)).abs().amax((-1, -2)).numpy()   # (B, steps)
    bound = np.cumsum(2 * err, 1)
    gap = g["gap_" + case][:, :n]
    trace = []
    with torch.no_grad():
        CD.generate_beam(m.eval(), batch["img"], 32, cfg, kv=True, trace=trace)
    cov = [int(np.argmin(np.append(gap[c] >= 2 * bound[c], False))) for c in range(2)]
    print("steps covered", cov, "bound at the last step", bound[:, -1].tolist(), "smallest gap", gap.min())
    assert max(cov) >= 1
    for c in range(2):
        for i in range(min(cov[c], n - 1)):
            assert trace[i][0][c].tolist() == g["parents_" + case][c, i].tolist() and trace[i][1][c].tolist() == g["words_" + case][c, i].tolist(), \
                (c, i)
        if cov[c] >= n and g["final_gap_" + case][c] >= 2 * bound[c, -1]:
            assert torch.equal(ids_out[c].cpu(), torch.from_numpy(g["ids_" + case][c]))
            np.testing.assert_allclose(lp[c].cpu().numpy(), g["logprob_" + case][c], atol=2 * bound[c, -1])


def test_beam_chunks_and_clip_independence(golden_dir):
    """nb 5: at most 6 clips per cached chunk; 7 clips decode as 6 + 1, and the lone clip gives the same bits as in its own call"""
    g, m, batch, _ = _micro_beam(golden_dir, "plain", clips=7)
    m.args.update(num_beams=5, num_keep_best=3, max_gen_length=8)
    b = {k: batch[k] for k in ("img", "txt", "mask")}
    ids, lp = m(b, is_decode=True)
    assert ids.shape == (7, 3, 8) and lp.shape == (7, 3)
    i0, l0 = m({k: v[:6] for k, v in b.items()}, is_decode=True)
    i1, l1 = m({k: v[6:] for k, v in b.items()}, is_decode=True)
    assert torch.equal(ids, torch.cat([i0, i1])) and torch.equal(lp, torch.cat([l0, l1]))
    assert (lp[:, :-1] >= lp[:, 1:]).all() and (ids[:, :, 0] == CLS).all()


def test_beam_generation_leaves_model_untouched_and_is_deterministic(golden_dir):
    g, m, batch, _ = _micro_beam(golden_dir, "pen")
    m.train()
    ar = m.arena()
    ar.zero_grad()
    ar.grad.fill_(0.25)
    w0 = [p.detach().clone() for p in m.parameters()]
    g0 = ar.grad.clone()
    b = {"img": batch["img"], "txt": batch["txt"], "mask": batch["mask"]}
    i1, l1 = m(b, is_decode=True)
    i2, l2 = m(b, is_decode=True)
    torch.cuda.synchronize()
    assert m.training and all(mm.training for mm in m.modules())
    assert all(torch.equal(a, p.detach()) for a, p in zip(w0, m.parameters()))
    assert torch.equal(ar.grad, g0)
    assert torch.equal(i1, i2) and torch.equal(l1, l2)


# ---- Base size: the cached beams against the full-recompute loop -----------------------------------------------------------------------
def test_base_beam_kv_matches_full_recompute():
    from tests.helpers import build_filled_model
    from lavender_amd import LAVENDER_Captioning
    from lavender_amd import caption_decode as CD
    B, nb, L = 4, 3, 12
    m = build_filled_model("base", "b12l", B, cls=LAVENDER_Captioning).eval()
    m.args.update(max_gen_length=L, num_beams=nb, num_keep_best=2)
    img = make_batch(B, seed=11)["img"].cuda()
    cfg = CD.make_config(m.args, 32)
    with torch.no_grad():
        tr_f, steps_f, steps_k, tr_k = [], [], [], []
        ids_f, lp_f = CD.generate_beam(m, img, 32, cfg, kv=False, trace=tr_f, step_logits=steps_f)
        n = len(tr_f)
        forced = (torch.stack([t[0] for t in tr_f[:n]], 1), torch.stack([t[1] for t in tr_f[:n]], 1))
        if n < L - 1:
            pad = (L - 1 - n, nb)
            forced = tuple(torch.cat([f, f[:, -1:].expand(B, *pad)], 1) for f in forced)
        CD.generate_beam(m, img, 32, cfg, kv=True, forced=forced, step_logits=steps_k)
        ids_k, lp_k = CD.generate_beam(m, img, 32, cfg, kv=True, trace=tr_k)
    k = min(n, L - 2)
    a, b = torch.stack(steps_k[:k], 1), torch.stack(steps_f[:k], 1)
    d = (a - b).abs()
    print("Base, teacher-forced beam logits, cached vs full recompute: max", d.max().item(), "mean", d.mean().item(), "steps", k)
    assert d.max() < 2 * LOGIT_MAX and d.mean() < 2 * LOGIT_MEAN
    # the margin rule: the full-recompute run's merged candidate scores, an error of 2 x 2 LOGIT_MAX per step on a cumulative score
    cand = torch.stack([t[2] for t in tr_f[:k]], 1).numpy()                # (B, steps, 2 nb), descending
    gaps = np.diff(-cand, axis=-1).min(-1)
    bound = 2 * 2 * 2 * LOGIT_MAX * np.arange(1, k + 1)
    cov = [int(np.argmin(np.append(gaps[c] >= 2 * bound, False))) for c in range(B)]
    print("steps covered by the margin rule", cov)
    for c in range(B):
        for i in range(cov[c]):
            assert torch.equal(tr_k[i][0][c].cpu(), tr_f[i][0][c]) and torch.equal(tr_k[i][1][c].cpu(), tr_f[i][1][c]), (c, i)
    assert ids_k.shape == ids_f.shape == (B, 2, L)
