"""Golden vectors of caption generation (CONTAINER ONLY -- needs the reference checkout): LAVENDER_Captioning.generate
(model_for_captioning.py:139-500) as main_caption.py:98-125 drives it (is_decoder False: every step re-runs the fusion encoder over
the video rows and the text so far + [MASK]).  Same recipe as make_goldens_variants.py (micro Swin + micro BERT, B = 2, parameters
filled from their state_dict keys); writes cap_gen_micro_b2.npz next to this file:
  * greedy ids / logprob at max_gen_length 12, and the same with repetition_penalty 1.3;
  * per step, the [MASK]-row logits (after the penalty, as the token is chosen from them) at a fixed 256-column subset, their
    logsumexp and the top-1 / top-2 margin.

    python tests/golden/make_goldens_caption_gen.py
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
from make_goldens import R, make_batch, BERT_CFGS  # noqa: E402
from make_goldens_variants import build  # noqa: E402

MAX_LEN = 12
# with the key-filled weights attention is nearly uniform and the [MASK]-row logits of consecutive steps are close: the decoder weight
# is scaled by this factor so that the greedy choices have top-1 margins well above the bf16 tolerance of the device path
DECODER_SCALE = 8.0


def run(ref, penalty):
    CAP = importlib.import_module("model_for_captioning")
    B, swin, bert = 2, "micro", "micro"
    m, _ = build(ref, CAP.LAVENDER_Captioning, swin, bert, B, max_gen_length=MAX_LEN, repetition_penalty=penalty, is_decoder=False)
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
    vocab = BERT_CFGS[bert]["vocab_size"]
    batch = make_batch(B, vocab=vocab, seed=6)
    rows = []
    m.fc_mtm.register_forward_hook(lambda mod, inp, out: rows.append(out[:, -1].detach().clone()))
    m.eval()
    with torch.no_grad():
        ids, lp = m({"img": batch["img"], "txt": batch["txt"], "mask": batch["mask"], "attn_mask_type": "seq2seq", "prompt": None}, is_decode=True)
    steps = []
    for i, lg in enumerate(rows):                       # the penalty as the reference applies it, on the ids known at that step
        lg = lg.clone()
        if penalty != 1.0:
            for b in range(B):
                for tok in set(ids[b, 0, :i + 1].tolist()):
                    lg[b, tok] = lg[b, tok] * penalty if lg[b, tok] < 0 else lg[b, tok] / penalty
        steps.append(lg)
    lg = torch.stack(steps, 1)                          # (B, steps, V)
    top2 = lg.topk(2, -1).values
    P = {k.replace("trsfr.enc.", "trsfr."): v.detach() for k, v in m.state_dict().items()}
    return ids, lp, lg, (top2[..., 0] - top2[..., 1]), P, batch


if __name__ == "__main__":
    torch.set_num_threads(8)
    ref = MG.import_reference()
    ids, lp, lg, margin, P, batch = run(ref, 1.0)
    ids_p, lp_p, lg_p, margin_p, _, _ = run(ref, 1.3)
    V = lg.shape[-1]
    cols = torch.randperm(V, generator=torch.Generator().manual_seed(5))[:256]
    np.savez_compressed(
        f"{HERE}/cap_gen_micro_b2.npz", txt=batch["txt"].numpy(), ids=ids.numpy(), logprob=lp.numpy(), step_cols=lg[..., cols].numpy().astype(np.float32),
        step_lse=torch.logsumexp(lg, -1).numpy(), step_margin=margin.numpy(), ids_pen=ids_p.numpy(), logprob_pen=lp_p.numpy(),
        step_cols_pen=lg_p[..., cols].numpy().astype(np.float32), step_lse_pen=torch.logsumexp(lg_p, -1).numpy(), step_margin_pen=margin_p.numpy(),
        cols=cols.numpy(), meta=np.array(["micro", "micro", "2", "224", str(MAX_LEN), "1.3", f"decoder.weight x {DECODER_SCALE}"]))
    print("ids", ids[:, 0].tolist(), "logprob", lp.flatten().tolist())
    print("ids (penalty 1.3)", ids_p[:, 0].tolist(), "logprob", lp_p.flatten().tolist())
    print("smallest top-1 margin per row", margin.min(1).values.tolist(), "(penalty)", margin_p.min(1).values.tolist())
    print("caption-generation golden written to", HERE)
