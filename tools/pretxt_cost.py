"""Cost of the pre-text (task token / prompt) in front of the fusion encoder.

  * training step time (forward + backward + AdamW, Agent.step) at the QAOE and retrieval-MLM shapes -- Swin-B + 12-layer fusion encoder,
    B = 32 clips of 5 x 224^2 frames, X = 26 (QAOE) / 33 (retrieval, B^2 pairs) text tokens -- with both switches off, with a task token and
    with a prompt (the 9-token prompt of the tests);
  * lav_text_embed_pre_bwd at n = 160 texts (B * O of RetMC / pretrain VTM) against lav_text_embed_bwd on the same rows.

    python tools/pretxt_cost.py [--steps 5] [--warmup 2] [--out results.json]
"""
import argparse
import gc
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PROMPT = [101, 2003, 1996, 2678, 1011, 3793, 103, 1029, 102]


def step_time(kind, mode, B, steps, warmup):
    import lavender_amd as LA
    from lavender_amd.dist import set_seed
    from tests.helpers import Tok, make_args, make_batch
    set_seed(88)
    X = 26 if kind == "qaoe" else 33
    args = make_args("base", "b12l", B, lr=1e-5, max_iter=1000, size_vocab=-1, enable_task_token=(mode == "task"), enable_prompt=(mode == "prompt"))
    if kind == "qaoe":
        m = LA.LAVENDER_QAOE_MLM(args, Tok()).cuda()
        m.arena()
        ag = LA.Agent_QAOE_MLM(args, m)
        b = make_batch(B, X=X, seed=6)
        ans = torch.full(b["txt"].shape, -1, dtype=torch.long)
        ans[:, -1] = 2023
        b["mask_ans"] = ans
        task = "oe"
    else:
        m = LA.LAVENDER_Retrieval_MLM(args, Tok()).cuda()
        m.arena()
        ag = LA.Agent_Retrieval_MLM(args, m)
        b = make_batch(B, X=X, seed=6)
        b["vid"] = list(range(B))
        task = "vtm"
    if mode == "task":
        b["task_name"] = task
    elif mode == "prompt":
        ids = torch.tensor(PROMPT)
        b["prompt"] = (ids, torch.ones_like(ids))
    batch = ag.prepare_batch(dict(b))
    for _ in range(warmup):
        ag.step(dict(batch), True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ag.step(dict(batch), True)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    del ag, m, batch
    gc.collect()
    torch.cuda.empty_cache()
    return ms


def embed_bwd_us(n=160, X=26, Hd=768):
    from lavender_amd import hip as K
    from _bench import bench
    g = torch.Generator().manual_seed(0)
    word, pos, type_ = [torch.randn(s, Hd, generator=g).cuda() * 0.05 for s in (30522, 512, 2)]
    gamma, beta = torch.ones(Hd).cuda(), torch.zeros(Hd).cuda()
    ids = torch.randint(0, 30522, (n, X), generator=g).cuda()
    _, mean, rstd = K.text_embed_fwd(ids, n, X, Hd, word, pos, type_, gamma, beta, 1e-12, 0.1, 3)
    grads = [torch.zeros_like(t) for t in (word, pos, type_[0], gamma, beta)]
    res = {}
    dout = (torch.randn(n, X, Hd, generator=g) * 0.1).to(torch.bfloat16).cuda()
    res["text_embed_bwd"] = bench(lambda: K.text_embed_bwd(ids, dout, n, X, Hd, word, pos, type_[0], gamma, mean, rstd, 0.1, 3, *grads), n=50, warm=5)
    for Lp, mode in ((1, 0), (9, 1)):
        doutp = (torch.randn(n, Lp + X, Hd, generator=g) * 0.1).to(torch.bfloat16).cuda()
        d_pre = torch.zeros(Lp, Hd, device="cuda") if mode == 0 else torch.empty(Lp, Hd, dtype=torch.bfloat16, device="cuda")
        res[f"text_embed_pre_bwd_Lp{Lp}_mode{mode}"] = bench(
            lambda: K.text_embed_pre_bwd(ids, doutp, n, Lp, X, Hd, word, pos, type_[0], gamma, mean, rstd, 0.1, 3, *grads, 0, d_pre, mode), n=50, warm=5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the results as JSON to this file")
    a = ap.parse_args()
    res = {"embed_bwd_us_n160": embed_bwd_us()}
    print(json.dumps(res), flush=True)
    for kind in ("qaoe", "retrieval"):
        for mode in ("off", "task", "prompt"):
            res[f"{kind}_{mode}_ms"] = round(step_time(kind, mode, a.B, a.steps, a.warmup), 2)
            print(kind, mode, res[f"{kind}_{mode}_ms"], "ms / step", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
