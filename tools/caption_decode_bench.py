#!/usr/bin/env python
"""Caption generation timings (LAVENDER_Captioning.generate, lavender_amd/caption_decode.py): Swin-B + 12 fusion layers, 5 x 224^2
frames, max_gen_length 20, greedy.  One JSON line per (batch, path): video encoder ms, prefix ms (the video rows through the fusion
layers, cached path only), ms per generated token (the whole generation minus the video encoder and the prefix, divided by the
max_gen_length - 1 steps, for both paths; the cached path also reports its layers + head alone), captions/s; for the cached path
also the skinny GEMM's achieved HBM bandwidth on the decoder projection (N = 30522, K = 768).  Every step of the full-recompute loop (LAV_CAP_KV=0) is timed the same way.

    python tools/caption_decode_bench.py [--batches 1 8 32] [--reps 3] [--paths kv full]
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
        for B in a.batches:
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


if __name__ == "__main__":
    main()
