"""Golden vectors of beam-search caption generation (CONTAINER ONLY -- needs the reference checkout).  The reference reads num_beams and
expands its video features and attention mask num_beams times (model_for_captioning.py:148-215) but has no beam loop: this script replaces
its _generate_no_beam_search with the HF-2.x beam search that Oscar / SwinBERT ran (_generate_beam_search + BeamHypotheses, written here
from that contract), driven by the reference's own full-recompute step (prepare_inputs_for_generation + forward, is_decoder False).  Same
micro recipe and decoder scale as make_goldens_caption_gen.py; B = 2, num_beams 3, num_keep_best 2, max_gen_length 12, three cases:
plain, repetition_penalty 1.3, length_penalty 0.6.  Writes cap_beam_micro_b2.npz next to this file; per case:
  * ids (B, K, L) / logprob (B, K);
  * per step: parents / words of the next beams (B, steps, nb), the clip's 2 nb candidate scores, the smallest gap between any two
    quantities a decision of that step compared (the last candidate walked against the first one left out, a hypothesis against
    the worst kept, the done test), and each beam's [MASK] logits (after the penalty) at a fixed 256-column subset with their
    logsumexp.

    python tests/golden/make_goldens_caption_beam.py
"""
import sys
sys.dont_write_bytecode = True
import importlib
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG  # noqa: E402
from make_goldens import make_batch, BERT_CFGS  # noqa: E402
from make_goldens_variants import build  # noqa: E402
from make_goldens_caption_gen import DECODER_SCALE  # noqa: E402

NB, KEEP, MAX_LEN = 3, 2, 12
CASES = {"plain": dict(), "pen": dict(repetition_penalty=1.3), "alpha": dict(length_penalty=0.6)}


def beam_loop(m, B, nb, K, L, penalty, alpha, early, pad, eos, cls, cols):
    V = m.fc_mtm.predictions.decoder.weight.shape[0]
    beams = [[([cls], 0.0 if b == 0 else -1e9) for b in range(nb)] for _ in range(B)]
    hyps = [[] for _ in range(B)]
    worst, done = [1e9] * B, [False] * B
    rec = {k: [] for k in ("parents", "words", "cand", "gap", "cols", "lse")}
    for cur in range(1, L):
        rows = [ids for c in range(B) for ids, _ in beams[c]]
        curr = torch.tensor(rows, dtype=torch.long)
        logits = m(m.prepare_inputs_for_generation(curr))["logits"][:, -1].float()
        par, wd, cs, gap = np.zeros((B, nb), np.int64), np.full((B, nb), pad, np.int64), np.zeros((B, 2 * nb), np.float32), np.full(B, np.inf)
        lgs = []
        for c in range(B):
            flat = []
            for b, (ids, sc) in enumerate(beams[c]):
                lg = logits[c * nb + b].clone()
                for tok in set(ids):
                    lg[tok] = lg[tok] * penalty if lg[tok] < 0 else lg[tok] / penalty
                lgs.append(lg)
                lp = torch.log_softmax(lg, -1) + torch.tensor(sc, dtype=torch.float32)
                top = torch.topk(lp, 2 * nb + 1)
                flat += [(float(v), b * V + int(w)) for v, w in zip(top.values, top.indices)]
            flat.sort(key=lambda t: (-t[0], t[1]))
            cands = flat[:2 * nb]
            cs[c] = [v for v, _ in cands]
            if done[c]:
                par[c] = np.arange(nb)
                continue
            gaps = []
            if len(hyps[c]) == K and not early:
                gaps.append(abs(worst[c] - cands[0][0] / L ** alpha))
            if len(hyps[c]) == K and (early or worst[c] >= cands[0][0] / L ** alpha):
                done[c] = True
                par[c] = np.arange(nb)
                gap[c] = min(gaps)
                continue
            nxt, used = [], 0
            for sc, f in cands:
                used += 1
                b, w = f // V, f % V
                if w == eos or cur + 1 == L:
                    s = sc / cur ** alpha
                    if len(hyps[c]) == K:
                        gaps.append(abs(s - worst[c]))
                    if len(hyps[c]) < K or s > worst[c]:
                        hyps[c].append((s, list(beams[c][b][0])))
                        if len(hyps[c]) > K:
                            srt = sorted([(h[0], i) for i, h in enumerate(hyps[c])])
                            del hyps[c][srt[0][1]]
                            worst[c] = srt[1][0]
                        else:
                            worst[c] = min(s, worst[c])
                else:
                    nxt.append((beams[c][b][0] + [w], sc, b))
                if len(nxt) == nb:
                    break
            gaps.append(flat[used - 1][0] - flat[used][0])      # the last candidate walked against the first one left out
            gap[c] = min(gaps)
            if cur + 1 < L:
                par[c] = [p for _, _, p in nxt]
                wd[c] = [ids[-1] for ids, _, _ in nxt]
                beams[c] = [(ids, sc) for ids, sc, _ in nxt]
        lg = torch.stack(lgs).view(B, nb, V)
        for k, v in (("parents", par), ("words", wd), ("cand", cs), ("gap", gap), ("cols", lg[..., cols].numpy()),
                     ("lse", torch.logsumexp(lg, -1).numpy())):
            rec[k].append(v)
        if all(done):
            break
    ids = np.full((B, K, L), pad, np.int64)
    lps = np.zeros((B, K), np.float32)
    final_gap = np.full(B, np.inf)
    for c in range(B):
        srt = sorted(hyps[c], key=lambda t: t[0], reverse=True)
        for k, (s, h) in enumerate(srt[:K]):
            ids[c, k, :len(h)] = h
            ids[c, k, len(h)] = eos
            lps[c, k] = s
        if len(srt) > 1:
            final_gap[c] = min(srt[i][0] - srt[i + 1][0] for i in range(len(srt) - 1))
    out = {k: np.stack(v, 1) for k, v in rec.items()}
    out.update(ids=ids, logprob=lps, final_gap=final_gap)
    return out


def run(ref, case, cols):
    CAP = importlib.import_module("model_for_captioning")
    B, swin, bert = 2, "micro", "micro"
    kw = dict(repetition_penalty=1.0, length_penalty=1.0)
    kw.update(CASES[case])
    m, _ = build(ref, CAP.LAVENDER_Captioning, swin, bert, B, max_gen_length=MAX_LEN, num_beams=NB, num_keep_best=KEEP, is_decoder=False, **kw)
    m.config.is_decoder = False
    with torch.no_grad():
        m.fc_mtm.predictions.decoder.weight.mul_(DECODER_SCALE)

    class _Enc(torch.nn.Module):                         # the HF encoder call of the generation branch (use_cache / output_attentions)
        def __init__(s, enc):
            super().__init__()
            s.enc = enc

        def forward(s, feat, mask, output_attentions=False, use_cache=False, past_key_values=None):
            return {"last_hidden_state": s.enc(feat, mask).last_hidden_state, "attentions": None, "past_key_values": None}
    m.trsfr = _Enc(m.trsfr.enc)
    res = {}

    def _beam(self, input_ids, cur_len, max_length, do_sample, temperature, top_k, top_p, repetition_penalty, pad_token_id, eos_token_ids,
              batch_size):
        # the reference has expanded img_feats / full_attention_mask num_beams times before this call
        assert self.img_feats.shape[0] == batch_size * NB and cur_len == 1
        res.update(beam_loop(self, batch_size, NB, KEEP, max_length, repetition_penalty, kw["length_penalty"], False, pad_token_id,
                             eos_token_ids[0], int(input_ids[0, 0]), cols))
        return None
    m._generate_no_beam_search = _beam.__get__(m)
    vocab = BERT_CFGS[bert]["vocab_size"]
    batch = make_batch(B, vocab=vocab, seed=6)
    m.eval()
    with torch.no_grad():
        m({"img": batch["img"], "txt": batch["txt"], "mask": batch["mask"], "attn_mask_type": "seq2seq", "prompt": None}, is_decode=True)
    return res, batch


if __name__ == "__main__":
    torch.set_num_threads(8)
    ref = MG.import_reference()
    V = BERT_CFGS["micro"]["vocab_size"]
    cols = torch.randperm(V, generator=torch.Generator().manual_seed(5))[:256]
    arrays = {"cols": cols.numpy(), "meta": np.array([str(NB), str(KEEP), str(MAX_LEN), str(DECODER_SCALE), "micro", "micro", "2", "224"])}
    for case in CASES:
        res, batch = run(ref, case, cols)
        arrays["txt"] = batch["txt"].numpy()
        for k, v in res.items():
            arrays[f"{k}_{case}"] = v
        print(case, "ids", res["ids"].tolist(), "logprob", res["logprob"].tolist())
        print("  smallest selection gap per clip", res["gap"].min(1).tolist(), "final gap", res["final_gap"].tolist(),
              "steps", res["gap"].shape[1])
    np.savez_compressed(f"{HERE}/cap_beam_micro_b2.npz", **arrays)
    print("caption beam-search golden written to", HERE)
