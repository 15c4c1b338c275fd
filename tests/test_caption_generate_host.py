"""Caption generation, host side: the reference's greedy loop restated on the oracle primitives against the golden of the real
reference (tests/golden/make_goldens_caption_gen.py), the end-of-generation bookkeeping of lavender_amd.caption_decode on scripted
cases, and the argument checks of generate()."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import BERT_CFGS, make_batch

CLS, SEP, PAD, MASK = 101, 102, 0, 103


def _oracle_params(scale):
    from oracle import lavender_ref as R
    bc = BERT_CFGS["micro"]
    P = R.filled_params("micro", hidden=bc["hidden"], layers=bc["layers"], ffn=bc["ffn"], vocab=bc["vocab"])
    P["fc_mtm.predictions.decoder.weight"] = P["fc_mtm.predictions.decoder.weight"] * scale
    return P


def oracle_generate(P, img, max_len, penalty=1.0):
    """full-recompute greedy generation composed from the oracle: per step, text [ids ; MASK] at positions 0..cur_len through the whole
    fusion encoder under the seq2seq mask, MLM head at the [MASK] row.  Returns (ids, logprob, per-step logits after the penalty)."""
    from oracle import lavender_ref as R
    from lavender_amd import caption_decode as CD
    heads = BERT_CFGS["micro"]["heads"]
    f_img, m_img = R.enc_video(P, img, "micro")
    B, Lv = m_img.shape
    ids = torch.full((B, max_len), PAD, dtype=torch.long)
    ids[:, 0] = CLS
    state = (torch.ones(B, dtype=torch.int32), torch.zeros(B), torch.zeros(B))
    steps = []
    cur = 1
    while cur < max_len:
        inp = torch.cat([ids[:, :cur], torch.full((B, 1), MASK, dtype=torch.long)], 1)
        hid = R.go_cross(P, f_img, m_img, R.enc_txt(P, inp), torch.ones_like(inp), heads, attn_mask_type="seq2seq")
        logits = R.mlm_head(P, hid[:, Lv + cur])
        CD.apply_repetition_penalty(logits, ids[:, :cur], penalty)
        steps.append(logits.clone())
        tok = logits.argmax(-1)
        score = torch.log_softmax(logits, -1).gather(1, tok[:, None]).squeeze(1)
        CD.record_step(ids, cur, tok, score, state, PAD, SEP)
        cur += 1
        if int(state[0].max()) == 0:
            break
    out, lp = CD.finish_generation(ids, cur, max_len, *state, PAD, SEP)
    return out, lp, torch.stack(steps, 1)


@pytest.mark.parametrize("pen", [False, True])
def test_oracle_greedy_generation_matches_reference_golden(golden_dir, pen):
    g = np.load(os.path.join(golden_dir, "cap_gen_micro_b2.npz"))
    scale = float(str(g["meta"][6]).split("x")[-1])
    max_len, penalty = int(g["meta"][4]), (float(g["meta"][5]) if pen else 1.0)
    P = _oracle_params(scale)
    batch = make_batch(2, vocab=BERT_CFGS["micro"]["vocab"], seed=6)
    assert (batch["txt"].numpy() == g["txt"]).all()
    with torch.no_grad():
        ids, lp, steps = oracle_generate(P, batch["img"], max_len, penalty)
    sfx = "_pen" if pen else ""
    assert (ids.numpy() == g["ids" + sfx]).all(), (ids[:, 0].tolist(), g["ids" + sfx][:, 0].tolist())
    np.testing.assert_allclose(lp.numpy(), g["logprob" + sfx], atol=1e-5)
    cols = torch.from_numpy(g["cols"])
    np.testing.assert_allclose(steps[..., cols].numpy(), g["step_cols" + sfx], atol=1e-4)
    np.testing.assert_allclose(torch.logsumexp(steps, -1).numpy(), g["step_lse" + sfx], atol=1e-4)


def _reference_bookkeeping(tokens, scores, max_len):
    """the reference's loop body on scripted per-step tokens / scores (B, steps): finished rows emit PAD, a row finishes on SEP, early stop,
    SEP fill of the last column, masked mean, PAD padding"""
    B = tokens.shape[0]
    ids = [[CLS] for _ in range(B)]
    unf = [1] * B
    lps, masks = [], []
    cur = 1
    for s in range(tokens.shape[1]):
        if cur >= max_len:
            break
        add = [int(tokens[b, s]) if unf[b] else PAD for b in range(B)]
        lps.append([float(scores[b, s]) for b in range(B)])
        masks.append(list(unf))
        for b in range(B):
            ids[b].append(add[b])
            unf[b] = unf[b] * int(add[b] != SEP)
        cur += 1
        if max(unf) == 0:
            break
    if cur == max_len:
        for b in range(B):
            if unf[b]:
                ids[b][-1] = SEP
    lp = [sum(lps[i][b] * masks[i][b] for i in range(len(lps))) / sum(masks[i][b] for i in range(len(lps))) for b in range(B)]
    ids = [r + [PAD] * (max_len - len(r)) for r in ids]
    return torch.tensor(ids), torch.tensor(lp)


@pytest.mark.parametrize("case", ["early_finish", "no_finish", "all_finish_step1"])
def test_finish_generation_bookkeeping(case):
    from lavender_amd import caption_decode as CD
    max_len = 6
    tokens = {"early_finish": [[5, SEP, 7, 8, 9], [5, 6, 7, SEP, 9]],
              "no_finish": [[5, 6, 7, 8, 9], [5, SEP, 7, 8, 9]],
              "all_finish_step1": [[SEP, 6, 7, 8, 9], [SEP, 6, 7, 8, 9]]}[case]
    tokens = torch.tensor(tokens)
    scores = -torch.arange(1, 11, dtype=torch.float32).view(2, 5) / 7.0
    ref_ids, ref_lp = _reference_bookkeeping(tokens, scores, max_len)
    # the cached path: every step runs to max_len, no early stop
    ids = torch.full((2, max_len), PAD, dtype=torch.long)
    ids[:, 0] = CLS
    state = (torch.ones(2, dtype=torch.int32), torch.zeros(2), torch.zeros(2))
    for s in range(max_len - 1):
        CD.record_step(ids, s + 1, tokens[:, s], scores[:, s], state, PAD, SEP)
    out, lp = CD.finish_generation(ids, max_len, max_len, *state, PAD, SEP)
    assert out.shape == (2, 1, max_len) and lp.shape == (2, 1) and out.dtype == torch.long
    assert (out[:, 0] == ref_ids).all(), (out[:, 0].tolist(), ref_ids.tolist())
    torch.testing.assert_close(lp[:, 0], ref_lp, atol=1e-6, rtol=0)


def test_generation_arguments_are_checked():
    from lavender_amd import caption_decode as CD
    from lavender_amd.args import EasyDict
    with pytest.raises(NotImplementedError):
        CD.GenConfig(EasyDict(num_beams=2), 32)
    with pytest.raises(NotImplementedError):
        CD.GenConfig(EasyDict(num_return_sequences=2), 32)
    with pytest.raises(ValueError):
        CD.GenConfig(EasyDict(max_gen_length=33), 32)
    c = CD.GenConfig(EasyDict(max_gen_length=20, do_sample=True, top_k=5, repetition_penalty=1.3), 32)
    assert (c.max_len, c.do_sample, c.top_k, c.penalty, c.top_p) == (20, True, 5, 1.3, 1.0)
