"""Beam search for caption generation, host side: the package's host bookkeeping (lavender_amd.caption_decode.host_beam_search, the
LAV_CAP_KV=0 path) against this file's own plain-Python restatement of Oscar / SwinBERT's _generate_beam_search + BeamHypotheses on
synthetic logits; the oracle-built micro model against the beam golden of the real reference (tests/golden/make_goldens_caption_beam.py);
the argument checks."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import BERT_CFGS, make_batch

CLS, SEP, PAD, MASK = 101, 102, 0, 103
V = 160


def _penalise(row, prev, penalty):
    row = row.clone()
    for tok in set(prev):
        row[tok] = row[tok] * penalty if row[tok] < 0 else row[tok] / penalty
    return row


def reference_beam_search(step_fn, clips, nb, K, L, alpha=1.0, early=False, penalty=1.0):
    """HF-2.x beam search as Oscar / SwinBERT ran it, in plain Python (scores as Python floats; the logits and the log-softmax in fp32 torch)"""
    beams = [[([CLS], 0.0 if b == 0 else -1e9) for b in range(nb)] for _ in range(clips)]
    hyps = [[] for _ in range(clips)]
    worst = [1e9] * clips
    done = [False] * clips
    for cur in range(1, L):
        rows = [ids for c in range(clips) for ids, _ in beams[c]]
        hist = torch.full((clips * nb, L), PAD, dtype=torch.long)
        for r, ids in enumerate(rows):
            hist[r, :len(ids)] = torch.tensor(ids)
        logits = step_fn(hist, cur)
        for c in range(clips):
            if done[c]:
                continue
            flat = []
            for b, (ids, sc) in enumerate(beams[c]):
                lp = torch.log_softmax(_penalise(logits[c * nb + b].float(), ids, penalty), -1) + torch.tensor(sc, dtype=torch.float32)
                flat += [(float(v), b * V + w) for w, v in enumerate(lp.tolist())]
            flat.sort(key=lambda t: (-t[0], t[1]))
            cands = flat[:2 * nb]
            if len(hyps[c]) == K and (early or worst[c] >= cands[0][0] / L ** alpha):
                done[c] = True
                continue
            nxt = []
            for sc, f in cands:
                b, w = f // V, f % V
                if w == SEP or cur + 1 == L:
                    s = sc / cur ** alpha
                    if len(hyps[c]) < K or s > worst[c]:
                        hyps[c].append((s, list(beams[c][b][0])))
                        if len(hyps[c]) > K:
                            srt = sorted([(h[0], i) for i, h in enumerate(hyps[c])])
                            del hyps[c][srt[0][1]]
                            worst[c] = srt[1][0]
                        else:
                            worst[c] = min(s, worst[c])
                else:
                    nxt.append((beams[c][b][0] + [w], sc))
                if len(nxt) == nb:
                    break
            if cur + 1 < L:
                beams[c] = nxt
        if all(done):
            break
    ids = torch.full((clips, K, L), PAD, dtype=torch.long)
    lps = torch.zeros(clips, K)
    for c in range(clips):
        for k, (s, h) in enumerate(sorted(hyps[c], key=lambda t: t[0], reverse=True)[:K]):
            ids[c, k, :len(h)] = torch.tensor(h)
            ids[c, k, len(h)] = SEP
            lps[c, k] = s
    return ids, lps


def _synthetic(case):
    """per-row logits as a function of that row's own history only (both loops see the same numbers for the same beam)"""
    def fn(hist, cur):
        out = torch.empty(hist.shape[0], V)
        for r in range(hist.shape[0]):
            key = sum((i + 1) * 1009 * int(t) for i, t in enumerate(hist[r, :cur].tolist())) % (2 ** 31)
            x = torch.randn(V, generator=torch.Generator().manual_seed(key)) * 2.0
            if case == "ties":
                x = torch.round(x * 2) / 2                         # many exact ties, across words and across beams
            if case == "eos_step1" and cur == 1:
                x[SEP] = 12.0                                      # beam 0 ends at step 1
            if case == "all_end" and cur >= 3:
                x[SEP] = 15.0                                      # every beam's best word is [SEP]
            out[r] = x
        return out
    return fn


class _Cfg:
    def __init__(self, nb, K, L, alpha, early, penalty):
        from lavender_amd.args import EasyDict
        from lavender_amd import caption_decode as CD
        self.c = CD.BeamConfig(EasyDict(num_beams=nb, num_keep_best=K, max_gen_length=L, length_penalty=alpha, early_stopping=early,
                                        repetition_penalty=penalty), 32)


CASES = [(case, nb, K, alpha, early) for case in ("random", "eos_step1", "all_end", "ties") for nb, K in ((3, 2), (4, 4), (2, 1))
         for alpha, early in ((1.0, False), (0.6, True))] + \
        [("random", 3, K, alpha, early) for K in (1, 2, 3) for alpha in (0.0, 0.6, 1.0, 2.0) for early in (False, True)]


@pytest.mark.parametrize("case,nb,K,alpha,early", CASES)
def test_host_bookkeeping_matches_restatement(case, nb, K, alpha, early):
    from lavender_amd import caption_decode as CD
    L, clips = 9, 3
    penalty = 1.3 if case == "random" and nb == 3 else 1.0
    cfg = _Cfg(nb, K, L, alpha, early, penalty).c
    fn = _synthetic(case)
    ref_ids, ref_lp = reference_beam_search(fn, clips, nb, K, L, alpha, early, penalty)
    ids, lp = CD.host_beam_search(fn, clips, cfg, CLS, PAD, SEP)
    assert ids.shape == (clips, K, L) and lp.shape == (clips, K) and ids.dtype == torch.long and lp.dtype == torch.float32
    assert torch.equal(ids, ref_ids), (ids.tolist(), ref_ids.tolist())
    torch.testing.assert_close(lp, ref_lp, atol=1e-6, rtol=0)
    assert (ids[:, :, 0] == CLS).all() and (ids == SEP).sum(-1).ge(1).all()
    if case == "eos_step1":                                        # beam 0's [CLS] alone is a hypothesis of every clip
        assert any((ids[c, k, 1] == SEP).item() for c in range(clips) for k in range(K))


def test_finish_orders_ties_by_insertion():
    from lavender_amd import caption_decode as CD
    hyp_ids = torch.arange(12).view(1, 4, 3)
    score = torch.tensor([[-1.0, -0.5, -1.0, -0.5]])
    seq = torch.tensor([[5, 3, 1, 4]], dtype=torch.int32)
    ids, lp = CD.finish_beams(hyp_ids, score, seq)
    assert lp.tolist() == [[-0.5, -0.5, -1.0, -1.0]]
    assert ids[0, :, 0].tolist() == [3, 9, 6, 0]                  # equal scores: the earlier insertion (seq 3 < 4, 1 < 5) first


# ---- the micro model against the golden of the real reference -------------------------------------------------------------------------
def _beam_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cap_beam_micro_b2.npz"))


def oracle_beam_step_fn(P, img):
    """the full-recompute [MASK] logits of the oracle for a history (rows, L) at step cur, the video features expanded to the rows"""
    from oracle import lavender_ref as R
    f_img, m_img = R.enc_video(P, img, "micro")
    Lv = f_img.shape[1]
    heads = BERT_CFGS["micro"]["heads"]

    def fn(hist, cur):
        nb = hist.shape[0] // f_img.shape[0]
        fi, mi = f_img.repeat_interleave(nb, 0), m_img.repeat_interleave(nb, 0)
        inp = torch.cat([hist[:, :cur], torch.full((hist.shape[0], 1), MASK, dtype=torch.long)], 1)
        hid = R.go_cross(P, fi, mi, R.enc_txt(P, inp), torch.ones_like(inp), heads, attn_mask_type="seq2seq")
        return R.mlm_head(P, hid[:, Lv + cur])
    return fn


@pytest.mark.parametrize("case", ["plain", "pen", "alpha"])
def test_oracle_beam_search_matches_reference_golden(golden_dir, case):
    from tests.test_caption_generate_host import _oracle_params
    from lavender_amd import caption_decode as CD
    from lavender_amd.args import EasyDict
    g = _beam_golden(golden_dir)
    nb, K, L, scale = int(g["meta"][0]), int(g["meta"][1]), int(g["meta"][2]), float(g["meta"][3])
    kw = {"plain": {}, "pen": dict(repetition_penalty=1.3), "alpha": dict(length_penalty=0.6)}[case]
    cfg = CD.BeamConfig(EasyDict(num_beams=nb, num_keep_best=K, max_gen_length=L, **kw), 32)
    P = _oracle_params(scale)
    batch = make_batch(2, vocab=BERT_CFGS["micro"]["vocab"], seed=6)
    with torch.no_grad():
        ids, lp = CD.host_beam_search(oracle_beam_step_fn(P, batch["img"]), 2, cfg, CLS, PAD, SEP)
    assert torch.equal(ids, torch.from_numpy(g["ids_" + case])), (ids.tolist(), g["ids_" + case].tolist())
    np.testing.assert_allclose(lp.numpy(), g["logprob_" + case], atol=1e-5)


# ---- argument checks --------------------------------------------------------------------------------------------------------------------
def test_beam_arguments_are_checked():
    from lavender_amd import caption_decode as CD
    from lavender_amd.args import EasyDict
    c = CD.make_config(EasyDict(num_beams=5, num_keep_best=3, length_penalty=0.6, early_stopping=True, repetition_penalty=1.2, top_k=7,
                                max_gen_length=20), 32)
    assert isinstance(c, CD.BeamConfig)
    assert (c.num_beams, c.keep, c.length_penalty, c.early_stopping, c.penalty, c.max_len) == (5, 3, 0.6, True, 1.2, 20)
    assert isinstance(CD.make_config(EasyDict(max_gen_length=20), 32), CD.GenConfig)
    with pytest.raises(NotImplementedError):
        CD.make_config(EasyDict(num_beams=3, do_sample=True), 32)
    for k in ("num_return_sequences", "num_fsm_states"):
        with pytest.raises(NotImplementedError):
            CD.make_config(EasyDict(num_beams=3, **{k: 2}), 32)
    for bad in (dict(num_beams=9), dict(num_beams=0), dict(num_beams=3, num_keep_best=4), dict(num_beams=3, num_keep_best=0),
                dict(num_beams=3, max_gen_length=33)):
        with pytest.raises(ValueError):
            CD.make_config(EasyDict(**bad), 32)
    with pytest.raises(NotImplementedError):                       # the non-beam path still refuses num_keep_best != 1
        CD.GenConfig(EasyDict(num_beams=2), 32)
