#!/usr/bin/env python
"""Caption generation timings (LAVENDER_Captioning.generate, lavender_amd/caption_decode.py): Swin-B + 12 fusion layers, 5 x 224^2
frames, max_gen_length 20, greedy.  One JSON line per (batch, path): video encoder ms, prefix ms (the video rows through the fusion
layers, cached path only), ms per generated token (the whole generation minus the video encoder and the prefix, divided by the
max_gen_length - 1 steps, for both paths; the cached path also reports its layers + head alone), captions/s; for the cached path
also the skinny GEMM's achieved HBM bandwidth on the decoder projection (N = 30522, K = 768).  Every step of the full-recompute loop (LAV_CAP_KV=0) is timed the same way.
--beams: num_beams values (1 = the greedy records above); for nb > 1 the record is beam search with num_keep_best 1 over min(B, 32 // nb)
clips (one cached chunk, B * nb rows): ms per token as above (the prefix included on both paths) and, for the cached path, the beam-specific
kernels of one step (lav_beam_step + lav_beam_select + lav_beam_reparent at the last step's cache length, event-timed in isolation) in us
and as a share of the step.

    python tools/caption_decode_bench.py [--batches 1 8 32] [--reps 3] [--paths kv full] [--beams 1 3 5]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--paths", nargs="+", default=["kv", "full"])
    ap.add_argument("--max-len", type=int, default=20)
    ap.add_argument("--beams", type=int, nargs="+", default=[1])
    a = ap.parse_args()
    from tests.helpers import build_filled_model, make_batch
    from lavender_amd import LAVENDER_Captioning
    from lavender_amd import caption_decode as CD
    from lavender_amd import engine as E
    from lavender_amd import hip as K
    torch.manual_seed(0)
    m = build_filled_model("base", "b12l", max(a.batches), cls=LAVENDER_Captioning).eval()
    m.args.update(max_gen_length=a.max_len)
    cfg = CD.GenConfig(m.args, 32)
    T = a.max_len - 1
    with torch.no_grad():
        for nb in a.beams:
            if nb > 1:
                for B in a.batches:
                    beam_records(m, a, nb, min(B, CD.KV_MAX_CLIPS // nb))
        for B in (a.batches if 1 in a.beams else []):
            img = make_batch(B, seed=11)["img"].cuda()
            CD.generate(m, img, 32, cfg)                                     # warm-up (first-use allocations, code objects)
            enc_ms, (feat, mask) = timed(lambda: m.enc_img(img), a.reps)
            for path in a.paths:
                kv = path == "kv"
                tot_ms, _ = timed(lambda: CD.generate(m, img, 32, cfg, kv=kv), a.reps)
                rec = dict(metric="caption_decode", path=path, B=B, max_gen_length=a.max_len, video_encoder_ms=round(enc_ms, 3),
                           total_ms=round(tot_ms, 3), captions_per_s=round(B / tot_ms * 1e3, 1))
                if kv:
                    # per token: everything after the video encoder and the prefix pass (layers, head, lav_greedy_step, host work), the
                    # same span as the full-recompute figure below minus the prefix that path does not have
                    pre_ms, dec = timed(lambda: CD.KVDecoder(m, feat, mask, a.max_len), a.reps)
                    step_ms, _ = timed(lambda: [dec.step(t) for t in range(1, a.max_len)], a.reps)
                    rec.update(prefix_ms=round(pre_ms, 3), ms_per_token=round((tot_ms - enc_ms - pre_ms) / T, 4),
                               ms_per_token_layers_and_head=round(step_ms / T, 4))
                    dw = E.W16(m.fc_mtm.predictions.decoder.weight)
                    V, H = dw.shape
                    x = torch.randn(B, H, device="cuda").to(torch.bfloat16)
                    out = torch.empty(B, V, device="cuda")
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    K.gemm_skinny(x, dw, B, V, H, out, K.SKINNY_F32)
                    ev[0].record()
                    for _ in range(50):
                        K.gemm_skinny(x, dw, B, V, H, out, K.SKINNY_F32)
                    ev[1].record()
                    torch.cuda.synchronize()
                    us = ev[0].elapsed_time(ev[1]) / 50 * 1e3
                    rec.update(decoder_gemm_us=round(us, 2), decoder_gemm_tb_s=round(V * H * 2 / (us * 1e-6) / 1e12, 2))
                else:
                    rec.update(ms_per_token=round((tot_ms - enc_ms) / T, 4))
                print(json.dumps(rec), flush=True)


def beam_records(m, a, nb, clips):
    from tests.helpers import make_batch
    from lavender_amd import caption_decode as CD
    from lavender_amd import hip as K
    from lavender_amd.args import EasyDict
    cfg = CD.BeamConfig(EasyDict(num_beams=nb, num_keep_best=1, max_gen_length=a.max_len), 32)
    T, L = a.max_len - 1, a.max_len
    img = make_batch(clips, seed=11)["img"].cuda()
    CD.generate_beam(m, img, 32, cfg)                                        # warm-up
    enc_ms, (feat, mask) = timed(lambda: m.enc_img(img), a.reps)
    for path in a.paths:
        kv = path == "kv"
        tot_ms, _ = timed(lambda: CD.generate_beam(m, img, 32, cfg, kv=kv), a.reps)
        rec = dict(metric="caption_decode_beam", path=path, B=clips, num_beams=nb, rows=clips * nb, max_gen_length=L,
                   video_encoder_ms=round(enc_ms, 3), total_ms=round(tot_ms, 3), captions_per_s=round(clips / tot_ms * 1e3, 1),
                   ms_per_token=round((tot_ms - enc_ms) / T, 4))
        if kv:
            R = clips * nb
            dec = CD.KVDecoder(m, feat, mask, L, beams=nb)
            step_ms, _ = timed(lambda: [dec.step(t) for t in range(1, L)], a.reps)
            st = CD.BeamState(clips, cfg, m.cls_token_id, m.pad_token_id, "cuda")
            cs = torch.empty((R, 2 * nb), device="cuda")
            cw = torch.empty((R, 2 * nb), dtype=torch.int32, device="cuda")
            logits = torch.randn(R, dec.V, device="cuda")
            sel = K.beam_select_desc(clips, nb, 1, dec.V, L, False, m.sep_token_id, m.pad_token_id, cs, cw, *st.tensors())
            rp = K.beam_reparent_desc(dec.cache, dec.cache_alt, st.parent, L)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            n = 50
            ev[0].record()
            for _ in range(n):
                K.beam_step(logits, dec.V, st.ids, L - 1, 1.0, st.beam_scores, nb, cs, cw)
            ev[1].record()
            for _ in range(n):
                K.beam_select(sel, L - 2, cfg.norm(L - 2), cfg.norm(L))
            ev[2].record()
            for _ in range(n):
                K.beam_reparent(rp, L - 2)
            ev[3].record()
            torch.cuda.synchronize()
            us = [ev[i].elapsed_time(ev[i + 1]) / n * 1e3 for i in range(3)]
            rec.update(ms_per_token_layers_and_head=round(step_ms / T, 4), beam_step_us=round(us[0], 2), beam_select_us=round(us[1], 2),
                       beam_reparent_us=round(us[2], 2), beam_kernels_share=round(sum(us) / 1e3 / rec["ms_per_token"], 4))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
