"""Caption fine-tuning cost on the MI355X.

  * training step time (Agent_Captioning.train_step: forward + fused CaptioningLoss + backward + AdamW) at Swin-B + 12-layer fusion encoder,
    B = 24 clips of 4 x 224^2 frames, X = 50 text tokens, p_mask 0.15, dropout on: the labelled-rows head against the full (B, X, V) head
    (LAV_CAP_ROWS=0), in alternating rounds on one model in one process;
  * lav_caption_loss_fwd_bwd alone at the two heads' logit shapes ((1200, 30528) with 15 % labelled rows; (176, 30528) all labelled), with and
    without the drop-the-worst selection, next to lav_cross_entropy_fwd_bwd on the same buffer: microseconds and GB/s.  Bytes moved: a kept row is
    read twice and written once, a dropped row read once and zeroed, an unlabelled row zeroed.  (The caption entry also allocates its five small
    result tensors per call and launches the one-block total kernel; the times include that.)

    python tools/caption_train_bench.py [--steps 8] [--warmup 3] [--rounds 3] [--out results.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def step_times(B, T, X, steps, warmup, rounds):
    import lavender_amd as LA
    from lavender_amd.dist import set_seed
    from tests.helpers import Tok, make_args, make_batch
    set_seed(88)
    args = make_args("base", "b12l", B, lr=1e-5, max_iter=100000, size_vocab=-1, label_smoothing=0.1, p_mask=0.15, task="caption")
    m = LA.LAVENDER_Captioning(args, Tok()).cuda()
    m.arena()
    ag = LA.Agent_Captioning(args, m)
    b = make_batch(B, T=T, X=X, seed=6)
    torch.manual_seed(88)
    b.update(ag.masking(b["txt"], p_mask=0.15))
    n_lab = int((b["ans_mtm"] != -1).sum())
    times = {True: [], False: []}
    for rnd in range(rounds + 1):                       # round 0 warms both paths up
        for rows_head in (True, False):
            ag.rows_head = rows_head
            batch = ag.prepare_batch(dict(b))
            batch["attn_mask_type"] = "seq2seq"
            n = warmup if rnd == 0 else steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                ag.train_step(dict(batch), sync=False)
            torch.cuda.synchronize()
            if rnd > 0:
                times[rows_head].append((time.perf_counter() - t0) / n * 1e3)
    return {"B": B, "T": T, "X": X, "head_rows_full": B * X, "head_rows_labelled": n_lab,
            "rows_head_ms": [round(t, 2) for t in times[True]], "full_head_ms": [round(t, 2) for t in times[False]],
            "rows_head_ms_median": round(statistics.median(times[True]), 2), "full_head_ms_median": round(statistics.median(times[False]), 2)}


def loss_kernel(rows, n_lab, V=30522, ld=30528):
    from lavender_amd import hip as K
    from _bench import bench
    rng = np.random.default_rng(0)
    labels = np.full(rows, -1, dtype=np.int64)
    labels[rng.permutation(rows)[:n_lab]] = rng.integers(0, V, size=n_lab)
    lab = torch.from_numpy(labels).cuda()
    buf = torch.randn((rows, ld), device="cuda").bfloat16()   # repeated calls read the previous call's gradient as logits: same traffic
    view = buf[:, :V]
    acc = torch.zeros(2, dtype=torch.float32, device="cuda")
    k_drop = int(n_lab * 0.75)
    row = ld * 2
    moved = row * (3 * n_lab + (rows - n_lab))
    moved_drop = row * (3 * k_drop + 2 * (n_lab - k_drop) + (rows - n_lab))      # a dropped row is read once and zeroed
    res = {"rows": rows, "labelled": n_lab}
    for name, nbytes, f in (("caption_loss", moved, lambda: K.caption_loss(view, V, lab, 0.1, n_lab, False, True)),
                            ("caption_loss_drop", moved_drop, lambda: K.caption_loss(view, V, lab, 0.1, k_drop, True, True)),
                            ("cross_entropy", moved, lambda: K.cross_entropy(view, V, lab, acc, 1.0 / n_lab, True))):
        us = bench(f, n=50, warm=5)
        res[name] = {"us": round(us, 2), "bytes_moved": nbytes, "GBps": round(nbytes / us / 1e3, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--B", type=int, default=24)
    ap.add_argument("--out", default=None, help="also write the results as JSON to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "caption_train_bench measures on the GPU"
    res = {"loss_kernel": [loss_kernel(1200, 180), loss_kernel(176, 176)]}
    print(json.dumps(res), flush=True)
    res["train_step"] = step_times(a.B, 4, 50, a.steps, a.warmup, a.rounds)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
