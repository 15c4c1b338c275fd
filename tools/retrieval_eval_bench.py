"""Text-to-video retrieval evaluation (lavender_amd/retrieval_eval.py) at the shipped retrieval shape: Swin-B + 12-layer fusion encoder, 5 x 224^2
frames (Lv = 250), size_txt 25 + the appended [MASK] (X = 26, L = 276), random weights.

  * pairs/s of the pair scorer (score_pairs: last layer and MLM head on the [MASK] row) against LAV_RET_ROWS=0 (full last layer + full-vocabulary
    head, two columns sliced), both at the default chunk, measured alternately; the scores of the two paths are compared;
  * the time of each phase of evaluate_t2v ('feat', scoring, ranking);
  * peak device memory of the scoring phase at the default chunk, for both paths;
  * the projected scoring time of 10^6 pairs (MSR-VTT 1k-A);
  * the multiply-accumulates per pair of both paths, counted from the shapes.

    python tools/retrieval_eval_bench.py [--videos 64] [--texts 256] [--reps 2] [--out results.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def macs_per_pair(Lv, X, H=768, F=3072, layers=12, V=30522):
    """(full path, rows path) multiply-accumulates of the fusion encoder + MLM head for one pair"""
    L = Lv + X
    layer = L * (4 * H * H + 2 * H * F) + 2 * L * L * H
    rows_last = L * 3 * H * H + 2 * L * H + (H * H + 2 * H * F)
    full = layers * layer + X * (H * H + H * V)
    rows = (layers - 1) * layer + rows_last + H * H + 2 * H
    return full, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--texts", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lavender_amd as LA
    import lavender_amd.retrieval_mlm as RM
    from lavender_amd import hip as K
    from lavender_amd.dist import set_seed
    from lavender_amd.retrieval_eval import collect_features, metrics_from_ranks, pair_chunk_for, score_matrix
    from tests.helpers import Tok, make_args
    set_seed(88)
    T, S, X = 5, 224, 26
    args = make_args("base", "b12l", a.batch, size_vocab=-1)
    m = LA.LAVENDER_RetrievalMlmEval(args, Tok()).cuda().eval()
    m.arena()
    g = torch.Generator().manual_seed(3)
    vid_of = [t % a.videos for t in range(a.texts)]
    clips = torch.randn(a.videos, 1, T, 3, S, S, generator=g)
    batches = []
    for i in range(0, a.texts, a.batch):
        j = list(range(i, min(a.texts, i + a.batch)))
        txt = torch.zeros(len(j), X, dtype=torch.long)
        for r, t in enumerate(j):
            k = 6 + t % 15
            txt[r, 0] = 101
            txt[r, 1:1 + k] = torch.randint(1000, 30000, (k,), generator=g)
            txt[r, 1 + k] = 102
            txt[r, -1] = 103
        batches.append({"img": clips[[vid_of[t] for t in j]], "txt": txt, "mask": (txt != 0).long(), "tid": j, "vid": [vid_of[t] for t in j]})
    gt = {t: vid_of[t] for t in range(a.texts)}
    out = {"shape": dict(swin="base", layers=12, hidden=768, frames=T, size_img=S, X=X, videos=a.videos, texts=a.texts, pairs=a.videos * a.texts)}
    sync = torch.cuda.synchronize
    with torch.no_grad():
        # warm-up of every shape the timed phases use (feature pass, both scorer paths, the rank kernel)
        _, _, src = collect_features(m, batches[:1])
        for rows in (True, False):
            RM.RET_ROWS = rows
            score_matrix(m, src, 0, 1)
        sync()
        t0 = time.perf_counter()
        vids, tids, src = collect_features(m, batches)
        sync()
        t_feat = time.perf_counter() - t0
        L = src.Lv + src.X
        chunk = pair_chunk_for(L)
        out["default_chunk_pairs"] = chunk
        for rows in (True, False):                          # warm the full chunk shape of both paths
            RM.RET_ROWS = rows
            score_matrix(m, src, 0, max(1, chunk // a.videos + 1))
        sync()
        times = {True: [], False: []}
        peak = {}
        S_of = {}
        base = torch.cuda.memory_allocated()
        for _ in range(a.reps):
            for rows in (True, False):
                RM.RET_ROWS = rows
                torch.cuda.reset_peak_memory_stats()
                sync()
                t0 = time.perf_counter()
                Sm = score_matrix(m, src, 0, len(tids))
                sync()
                times[rows].append(time.perf_counter() - t0)
                peak[rows] = max(peak.get(rows, 0), torch.cuda.max_memory_allocated() - base)
                S_of[rows] = Sm
        RM.RET_ROWS = True
        gt_col = torch.tensor([vids.index(gt[t]) for t in tids], dtype=torch.int32, device="cuda")
        sync()
        t0 = time.perf_counter()
        r = K.retrieval_rank(S_of[True], gt_col).cpu().numpy()
        res = metrics_from_ranks(r)
        t_rank = time.perf_counter() - t0
        r_full = K.retrieval_rank(S_of[False], gt_col).cpu().numpy()
    n_pairs = len(vids) * len(tids)
    t_rows, t_full = float(np.median(times[True])), float(np.median(times[False]))
    full_mac, rows_mac = macs_per_pair(src.Lv, src.X)
    d = (S_of[True] - S_of[False]).abs()
    out.update({
        "pairs_per_s_rows": n_pairs / t_rows, "pairs_per_s_full": n_pairs / t_full, "speedup": t_full / t_rows,
        "score_s_rows": times[True], "score_s_full": times[False],
        "phase_s": {"feat": t_feat, "score": t_rows, "rank": t_rank},
        "peak_mem_score_MiB": {"rows": peak[True] / 2 ** 20, "full": peak[False] / 2 ** 20},
        "projected_1e6_pairs_s": {"rows": 1e6 / (n_pairs / t_rows), "full": 1e6 / (n_pairs / t_full)},
        "gmac_per_pair": {"full": full_mac / 1e9, "rows": rows_mac / 1e9, "saving": 1 - rows_mac / full_mac},
        "achieved_tflops_rows": 2 * rows_mac * n_pairs / t_rows / 1e12,
        "score_diff_max": d.max().item(), "ranks_equal_frac": float((r == r_full).mean()), "metrics_synthetic": res,
    })
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
