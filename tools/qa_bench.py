"""Video QA on the MI355X: the rows path (args.qa_rows: MLM head, in evaluation also the last fusion layer and the read-out, on the labelled
[MASK] rows only) against the full path (the reference's formulation over all B * X text rows).

  * training ms/step (Agent.step: forward + loss + backward + AdamW, dropout on) and evaluation samples/s (Agent.go_dl over a list of batches)
    for QAOE (X = 26) and QAMC (X = 101) at Swin-B + 12-layer fusion encoder, B = 32 clips of 5 x 224^2 frames, one [MASK] per sample: rows
    against full in alternating rounds on ONE model in ONE process (round 0 warms both paths up), medians over the rounds;
  * peak device memory of a training step and of an evaluation batch on both paths;
  * lav_answer_readout alone on (32, 30522) logits (row stride 30528), fp32 and bf16, 5 candidates, for each grid choice (column ranges per
    row; > 1 adds the merge launch): microseconds per call from device events over back-to-back calls, and the GB/s of the logit read.

    python tools/qa_bench.py [--steps 6] [--warmup 2] [--rounds 3] [--kernel-only] [--out results.json]
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

OPT_IDS = [1014, 1015, 1016, 1017, 1018]


def readout_kernel(n=32, V=30522, ld=30528, splits=(1, 2, 4, 8, 16)):
    """the C entry called directly with prebuilt arguments (the Python wrapper's argument handling would otherwise set the pace of back-to-back
    calls); "wrapper_us" is hip.answer_readout at the default grid, as the model path calls it"""
    import ctypes as C
    from lavender_amd import _lib as L
    from lavender_amd import hip as K
    from _bench import bench
    rng = np.random.default_rng(0)
    labels = torch.from_numpy(rng.integers(0, V, size=n).astype(np.int32)).cuda()
    cand = np.asarray(OPT_IDS, dtype=np.int32)
    res = []
    for dt in (torch.float32, torch.bfloat16):
        view = torch.randn((n, ld), device="cuda").to(dt)[:, :V]
        out = torch.empty((3, n), dtype=torch.int32, device="cuda")
        nbytes = n * V * view.element_size()
        row = {"n": n, "V": V, "ld": ld, "dtype": str(dt).split(".")[-1], "logit_bytes": nbytes, "us": {}, "GBps": {}}
        ref = None
        for s in splits:
            need = int(L.lib.lav_answer_readout_workspace_bytes(n, s))
            ws = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")
            argv = (K._s(), n, V, K._p(view), ld, int(dt == torch.float32), K._p(labels), None, cand.ctypes.data_as(C.c_void_p), len(cand), s,
                    K._p(ws), need, K._p(out[0]), K._p(out[1]), K._p(out[2]))
            assert L.lib.lav_answer_readout(*argv) == 0
            us = bench(lambda: L.lib.lav_answer_readout(*argv), n=2000, warm=100)
            row["us"][str(s)] = round(us, 2)
            row["GBps"][str(s)] = round(nbytes / us / 1e3, 1)
            got = out.cpu()
            ref = got if ref is None else ref
            assert torch.equal(got, ref), "the split count changed the outputs"
        row["wrapper_us"] = round(bench(lambda: K.answer_readout(view, V, labels, OPT_IDS, out=out), n=500, warm=50), 2)
        res.append(row)
    return res


def _batch(kind, B, X, T=5):
    from tests.helpers import make_batch
    b = make_batch(B, T=T, X=X, seed=6)
    ans = torch.full(b["txt"].shape, -1, dtype=torch.long)
    g = torch.Generator().manual_seed(11)
    if kind == "oe":
        ans[:, -1] = torch.randint(1000, 30000, (B,), generator=g)          # make_batch ends every row with [MASK]
    else:
        idx = torch.randint(0, 5, (B,), generator=g)
        ans[:, -1] = torch.tensor(OPT_IDS)[idx]
        b["ans_idx"] = idx
    b["mask_ans"] = ans
    return b


class _DL(list):
    dataset = None


def model_paths(kind, B, X, steps, warmup, rounds, eval_batches=4):
    import lavender_amd as LA
    from lavender_amd.dist import set_seed
    from tests.helpers import Tok, make_args
    set_seed(88)
    args = make_args("base", "b12l", B, lr=1e-5, max_iter=100000, size_vocab=-1, size_option=5, task=f"qa{kind}")
    m = (LA.LAVENDER_QAOE_MLM if kind == "oe" else LA.LAVENDER_QAMC_MLM)(args, Tok()).cuda()
    m.arena()
    ag = LA.Agent_QAOE_MLM(args, m) if kind == "oe" else LA.Agent_QAMC_MLM(args, m, OPT_IDS)
    b = _batch(kind, B, X)
    dl = _DL([b] * eval_batches)
    tr, ev, mem = {True: [], False: []}, {True: [], False: []}, {}
    for rnd in range(rounds + 1):                          # round 0 warms both paths up
        for rows in (True, False):
            args.qa_rows = rows
            n = warmup if rnd == 0 else steps
            batch = ag.prepare_batch(dict(b))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            for _ in range(n):
                ag.step(dict(batch), True)                 # both paths read the loss back every step, as the reference does
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n * 1e3
            mem[f"train_peak_GiB_{'rows' if rows else 'full'}"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            ag.go_dl(1, dl, False)
            torch.cuda.synchronize()
            de = time.perf_counter() - t0
            mem[f"eval_peak_GiB_{'rows' if rows else 'full'}"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
            if rnd > 0:
                tr[rows].append(dt)
                ev[rows].append(eval_batches * B / de)
    med = statistics.median
    out = {"kind": kind, "B": B, "X": X, "head_rows_full": B * X, "head_rows_labelled": B,
           "train_ms_rows": [round(t, 2) for t in tr[True]], "train_ms_full": [round(t, 2) for t in tr[False]],
           "train_ms_rows_median": round(med(tr[True]), 2), "train_ms_full_median": round(med(tr[False]), 2),
           "eval_samples_per_s_rows": [round(t, 1) for t in ev[True]], "eval_samples_per_s_full": [round(t, 1) for t in ev[False]],
           "eval_samples_per_s_rows_median": round(med(ev[True]), 1), "eval_samples_per_s_full_median": round(med(ev[False]), 1)}
    out.update(mem)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the results as JSON to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "qa_bench measures on the GPU"
    res = {"device": torch.cuda.get_device_name(0), "invocation": {"steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "B": a.B, "eval_batches": 4,
                                                                   "kernel_only": a.kernel_only, "readout_calls": 2000, "readout_warm": 100},
           "answer_readout": readout_kernel()}
    print(json.dumps(res), flush=True)
    if not a.kernel_only:
        res["model"] = []
        for kind, X in (("oe", 26), ("mc", 101)):
            res["model"].append(model_paths(kind, a.B, X, a.steps, a.warmup, a.rounds))
            print(json.dumps(res["model"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
