"""Multi-task MLM fine-tuning on the MI355X (lavender_amd/multi_task.py), Swin-B + 12-layer fusion encoder, ONE process:

  1. training ms/step of each task type inside the multi-task loop (Agent_Multi_Task.train_step, one model, the five tasks interleaved so that
     the geometry changes every step) against the same batch through that task's existing single-task agent (its own model of the same size),
     in alternating rounds; round 0 warms every path up.  Measured with the full (rows, X, vocab) head on both sides (mt_rows / qa_rows off,
     Agent_Captioning.rows_head off): the kernels are then the same, so the expectation is "equal within the spread of the rounds";
  2. evaluation samples/s of retrieval (B = 8: 64 pairs) and lsmdc-mc (B = 8, O = 5) with args.mt_rows on against off
     (Agent_Multi_Task.non_cap_evaluate over a list of batches);
  3. lav_match_readout against the torch formulation it replaces (column reads of the (pairs, X, 30522) logits, boolean indexing, argmax,
     nonzero, tolist): device time per call from events over back-to-back calls, and host wall time per batch including the read-back.

    python tools/multi_task_bench.py [--steps 4] [--warmup 2] [--rounds 3] [--B 8] [--out results.json]
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
TRUE, FALSE = 2995, 6270
TASKS = ["captioning_x", "retrieval_x", "qamc_x", "qamc_lsmdc-mc", "qaoe_x"]
SINGLE = {"captioning_x": ("LAVENDER_Captioning", "Agent_Captioning"), "retrieval_x": ("LAVENDER_Retrieval_MLM", "Agent_Retrieval_MLM"),
          "qamc_x": ("LAVENDER_QAMC_MLM", "Agent_QAMC_MLM"), "qamc_lsmdc-mc": ("LAVENDER_RetMC_MLM", "Agent_RetMC_MLM"),
          "qaoe_x": ("LAVENDER_QAOE_MLM", "Agent_QAOE_MLM")}


def make_task_batch(task, B, T=4, O=5):
    """host batches with the datasets' layouts; every text of the non-captioning tasks ends in its one [MASK] (tests.helpers.make_batch)"""
    from tests.helpers import make_batch
    from lavender_amd.captioning import masking
    g = torch.Generator().manual_seed(11)
    if task == "captioning_x":
        b = make_batch(B, T=T, X=51, seed=3)
        b["txt"][:, -1] = 0
        b["mask"] = (b["txt"] != 0).long()
        torch.manual_seed(3)
        r = masking(b["txt"], 0.15, 0, 103)
        b["txt"], b["ans_mtm"] = r["txt"], r["ans_mtm"]
    elif task == "retrieval_x":
        b = make_batch(B, T=T, X=26, seed=4)
        b["vid"] = list(range(B))
    elif task == "qamc_lsmdc-mc":
        txt = make_batch(B * O, T=1, S=32, X=26, seed=5)["txt"].view(B, O, 26)
        ans = torch.full(txt.shape, -1, dtype=torch.long)
        right = torch.randint(0, O, (B,), generator=g)
        ans[:, :, -1] = FALSE
        ans[torch.arange(B), right, -1] = TRUE
        b = {"img": make_batch(B, T=T, seed=6)["img"], "txt": txt, "mask": (txt != 0).long(), "mask_ans": ans}
    else:
        b = make_batch(B, T=T, X=101 if task == "qamc_x" else 26, seed=7)
        ans = torch.full(b["txt"].shape, -1, dtype=torch.long)
        if task == "qamc_x":
            idx = torch.randint(0, 5, (B,), generator=g)
            ans[:, -1] = torch.tensor(OPT_IDS)[idx]
            b["ans_idx"] = idx
        else:
            ans[:, -1] = torch.randint(1000, 30000, (B,), generator=g)
        b["mask_ans"] = ans
    return b


def _clone(b):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def _single_step(ag, task, b):
    pb = ag.prepare_batch(_clone(b))
    if task == "captioning_x":
        pb["attn_mask_type"] = "seq2seq"
        return ag.train_step(pb)
    return ag.step(pb, True)


def train_paths(B, steps, warmup, rounds, mt_rows):
    import lavender_amd as LA
    from lavender_amd.dist import set_seed
    from tests.helpers import Tok, make_args
    set_seed(88)
    mk = lambda: make_args("base", "b12l", B, lr=1e-5, max_iter=100000, size_vocab=-1, size_option=5, task="mt", mt_rows=mt_rows, qa_rows=mt_rows)
    batches = {t: make_task_batch(t, B) for t in TASKS}
    args = mk()
    mm = LA.LAVENDER_Multi_Task(args, Tok()).cuda()
    mm.arena()
    multi = LA.Agent_Multi_Task(args, mm, OPT_IDS)
    singles = {}
    for t in TASKS:
        a = mk()
        m = getattr(LA, SINGLE[t][0])(a, Tok()).cuda()
        m.arena()
        singles[t] = getattr(LA, SINGLE[t][1])(a, m, OPT_IDS) if t == "qamc_x" else getattr(LA, SINGLE[t][1])(a, m)
    singles["captioning_x"].rows_head = mt_rows            # Agent_Captioning's labelled-rows head follows the setting under test
    ms = {(t, who): [] for t in TASKS for who in ("multi", "single")}
    for rnd in range(rounds + 1):
        n = warmup if rnd == 0 else steps
        # the multi-task loop: the five tasks interleaved, each step timed on its own (a read-back per step, as the reference's .item())
        per = {t: 0.0 for t in TASKS}
        for _ in range(n):
            for t in TASKS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                b = _clone(batches[t])                     # the host copy and the upload are inside the timed step on both sides
                b["task"] = t
                multi.train_step(multi.prepare_batch(b))
                torch.cuda.synchronize()
                per[t] += time.perf_counter() - t0
        for t in TASKS:
            s0 = 0.0
            for _ in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _single_step(singles[t], t, batches[t])
                torch.cuda.synchronize()
                s0 += time.perf_counter() - t0
            if rnd > 0:
                ms[(t, "multi")].append(per[t] / n * 1e3)
                ms[(t, "single")].append(s0 / n * 1e3)
    out = []
    for t in TASKS:
        a, b = ms[(t, "multi")], ms[(t, "single")]
        out.append({"task": t, "B": B, "mt_rows": mt_rows, "multi_ms": [round(x, 2) for x in a], "single_ms": [round(x, 2) for x in b],
                    "multi_ms_median": round(statistics.median(a), 2), "single_ms_median": round(statistics.median(b), 2)})
    return out, multi, batches


def eval_paths(multi, batches, B, rounds, eval_batches=4):
    out = []
    for t in ("retrieval_x", "qamc_lsmdc-mc"):
        dl = [batches[t]] * eval_batches
        sps = {True: [], False: []}
        for rnd in range(rounds + 1):
            for rows in (True, False):
                multi.args.mt_rows = rows
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = multi.non_cap_evaluate(t, dl)
                torch.cuda.synchronize()
                if rnd > 0:
                    sps[rows].append(eval_batches * B / (time.perf_counter() - t0))
        out.append({"task": t, "B": B, "pairs": B * B if t == "retrieval_x" else B * 5, "ac": res,
                    "samples_per_s_rows": [round(x, 1) for x in sps[True]], "samples_per_s_full": [round(x, 1) for x in sps[False]],
                    "samples_per_s_rows_median": round(statistics.median(sps[True]), 1),
                    "samples_per_s_full_median": round(statistics.median(sps[False]), 1)})
    return out


def readout_kernel(G=8, O=8, X=26, V=30522, ld=30528):
    """lav_match_readout on the (pairs, 2) fp32 block and through a row map on the bf16 (pairs * X, ld) logits, against the torch formulation
    of Agent_Retrieval_MLM.step on the same logits"""
    from lavender_amd import hip as K
    from _bench import bench
    n = G * O
    out = torch.randn((n, X, ld), device="cuda").to(torch.bfloat16)[:, :, :V]
    ans = torch.full((n, X), -1, dtype=torch.long)
    gt = np.arange(G) % O
    ans[:, -1] = FALSE
    ans[torch.arange(G) * O + torch.from_numpy(gt), -1] = TRUE
    ans_d = ans.cuda()
    rows2d = out.as_strided((n * X, V), (ld, 1))
    row = torch.from_numpy((np.arange(n) * X + X - 1).astype(np.int32)).cuda()
    gt_d = torch.from_numpy(gt.astype(np.int32)).cuda()
    pair = torch.stack([out[:, -1, TRUE], out[:, -1, FALSE]], 1).float().contiguous()
    buf = torch.empty((2, G), dtype=torch.int32, device="cuda")

    def torch_form():
        p_true, p_false = out[:, :, TRUE].float(), out[:, :, FALSE].float()
        s = p_true / (p_true + p_false)
        s = s[ans_d != -1].view(G, O)
        a = ans_d[ans_d != -1].view(G, O)
        return (torch.argmax(s, dim=-1) == (a == TRUE).nonzero()[:, 1]).float().tolist()

    def host_us(f, n_calls=200):
        f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_calls):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n_calls * 1e6
    kern_flags = K.match_readout(rows2d, G, O, TRUE, FALSE, row=row, gt=gt_d, out=buf)[1].float().tolist()
    assert kern_flags == torch_form() == K.match_readout(pair, G, O, 0, 1, gt=gt_d)[1].float().tolist()
    return {"G": G, "O": O, "X": X, "V": V,
            "device_us_pair_block": round(bench(lambda: K.match_readout(pair, G, O, 0, 1, gt=gt_d, out=buf), n=2000, warm=100), 2),
            "device_us_row_map_bf16": round(bench(lambda: K.match_readout(rows2d, G, O, TRUE, FALSE, row=row, gt=gt_d, out=buf), n=2000, warm=100), 2),
            "host_us_per_batch_kernel_no_readback": round(host_us(lambda: K.match_readout(rows2d, G, O, TRUE, FALSE, row=row, gt=gt_d, out=buf)), 2),
            "host_us_per_batch_kernel_with_tolist": round(host_us(lambda: K.match_readout(rows2d, G, O, TRUE, FALSE, row=row, gt=gt_d, out=buf)[1].tolist()), 2),
            "host_us_per_batch_torch_formulation": round(host_us(torch_form), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the results as JSON to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "multi_task_bench measures on the GPU"
    res = {"device": torch.cuda.get_device_name(0), "invocation": {"steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "B": a.B, "eval_batches": 4},
           "match_readout": readout_kernel()}
    print(json.dumps(res), flush=True)
    if not a.kernel_only:
        res["train"], multi, batches = train_paths(a.B, a.steps, a.warmup, a.rounds, mt_rows=False)
        print(json.dumps(res["train"]), flush=True)
        res["eval"] = eval_paths(multi, batches, a.B, a.rounds)
        print(json.dumps(res["eval"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
