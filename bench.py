#!/usr/bin/env python
"""Headline benchmark: LAVENDER pretrain step (Video-Swin-B 5x224^2 + 32-token text + 12-layer fusion encoder +
MLM head; forward + backward + clip + AdamW) on N MI355X GPUs of one node, data parallel.

    python bench.py --gpus 1 --steps 5 --warmup 2
    python bench.py --gpus 1 --steps 5 --warmup 2 --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A "step" = one pass of the hot path over one synthetic batch of 32 clips per GPU (inputs resident in HBM, labels
already built).  Rank 0 prints ONE JSON line: `value` = whole-job samples/s over the --steps timed steps, `ms_per_step`
= wall-clock milliseconds per timed step.

A plain run does only that: set up, warm up, time the steps, write --dump-outputs, print the line.  --full adds the
measurements beyond the headline, each after the timed steps and outside their window:
`ms_per_step_reference_loop` (the reference's own loop semantics), `roofline` (the dominant kernel, the bf16 MFMA GEMM,
measured per launch with HIP events on its stream over two more steps), `cpu_baseline` (the CPU oracle, a restated
reference path, timed on the host cores at N=1), `side_workloads` (cfg4, cfg5) and `ab_baseline` / `dp1_*` (child runs
of this script).  In a plain line `ms_per_step_reference_loop` and `roofline` are null.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0        # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
TRAFFIC_FILE = next((f for f in ("r06_pmc_hbm_traffic", "r05_pmc_hbm_traffic", "r04b_pmc_hbm_traffic", "r04_pmc_hbm_traffic", "r03_pmc_hbm_traffic") if os.path.exists(os.path.join(ROOT, "profiles", f + ".json"))), "r03_pmc_hbm_traffic")   # newest committed PMC traffic table


def flops_per_sample(E=128, depths=(2, 2, 18, 2), T=5, S=224, X=32, layers=12, hid=768, vocab=30522, n_seq=5, win=(8, 7, 7)):
    """Algorithmic forward FLOPs per sample (SURVEY.md section 8d closed form: GEMM + attention MACs x2)."""
    f = 0.0
    n0 = T * (S // 4) ** 2
    f += n0 * 2 * 96 * E
    for s, d in enumerate(depths):
        C = E * 2 ** s
        side = S // 4 // 2 ** s
        n = T * side * side
        N = min(T, win[0]) * min(side, win[1]) * min(side, win[2])
        f += d * n * (24 * C * C + 4 * N * C)
        if s < 3:
            f += (n // 4) * 2 * (4 * C) * (2 * C)
    hw = (S // 32) ** 2
    if 8 * E != hid:
        f += T * hw * 2 * 8 * E * hid
    L = T * (1 + hw) + X
    f_seq = layers * L * (24 * hid * hid + 4 * L * hid)
    f_head = X * (2 * hid * hid + 2 * hid * vocab)
    return f + n_seq * (f_seq + f_head)


def synth_batch(B, T, S, X, rank, device):
    g = torch.Generator().manual_seed(1234 + rank)
    img = torch.randn(B, T, 3, S, S, generator=g)
    txt = torch.zeros(B, X, dtype=torch.long)
    for b in range(B):
        k = int(torch.randint(6, min(28, X - 3), (1,), generator=g))
        txt[b, 0] = 101
        txt[b, 1:1 + k] = torch.randint(1000, 30000, (k,), generator=g)
        txt[b, 1 + k] = 102
        txt[b, -1] = 103
    return dict(img=img, txt=txt, mask=(txt != 0).long())


def tsv_feed(args, B, T, rank, world):
    """Endless batches from the input pipeline over the committed fixture rows (two rows of the reference's sample TSV, T JPEG
    frames each) replicated to 8 B rows in a scratch TSV -- the on-disk format of _tools/extract_tsv.py, captions from the ids."""
    import tempfile
    from lavender_amd import data as D
    here = os.path.dirname(os.path.abspath(__file__))
    src = os.path.join(here, "tests", "golden", "msrvtt_2rows.tsv")
    rows = [ln.rstrip("\n").split("\t") for ln in open(src)]
    assert all(len(r) - 1 >= T for r in rows), "fixture rows hold 5 frames"
    d = tempfile.mkdtemp(prefix="lav_bench_tsv_")
    txt = {}
    with open(f"{d}/data.tsv", "w") as f, open(f"{d}/data.lineidx", "w") as fi:
        for i in range(8 * B):
            r = rows[i % len(rows)]
            fi.write("%d\n" % f.tell())
            f.write("\t".join([f"clip{i}"] + r[1:1 + T]) + "\n")
            txt[f"clip{i}"] = [f"a person is doing something in clip number {i} of the set"]

    class WordTok:
        cls_token = "[CLS]"; sep_token = "[SEP]"; pad_token = "[PAD]"; mask_token = "[MASK]"; unk_token = "[UNK]"
        ids = {"[PAD]": 0, "[UNK]": 100, "[CLS]": 101, "[SEP]": 102, "[MASK]": 103, "true": 2995, "false": 6270}

        def convert_tokens_to_ids(self, toks):
            return [self.ids[t] for t in toks]

        def encode(self, s, padding=None, max_length=None, truncation=None):
            ids = [101] + [1000 + (hash(w) % 20000) for w in s.split()][:max_length - 2] + [102]
            return ids + [0] * (max_length - len(ids))
    args.size_frame, args.img_transform, args.n_workers, args.distributed = T, ["img_rand_crop"], 8, world > 1
    ds = D.Dataset_Pretrain(args, {"train": txt}, f"{d}/data.tsv", f"{d}/data.lineidx", split="train", dataset="fixture", tokzr=WordTok())
    dl = D.PretrainLoader(ds, args, rank=rank, world=world)
    ep = 0
    while True:
        dl.sampler.set_epoch(ep)
        for b in dl:
            if b["img"].shape[0] == B:
                yield b
        ep += 1


def cpu_baseline_child():
    """Reference CPU path (restated: oracle/lavender_ref.py, parity-pinned to the real reference), Swin-B + 12L,
    B=2, fp32, forward + loss + backward, on this box's host cores.  Bounded: 1 warm-up + 2 timed iterations.
    16 intra-op threads: measured fastest on the 256-core GPU host (8: 1.3 s, 16: 1.0 s, 32: 1.1 s per forward; the
    default of one thread per core oversubscribes the container and is >100x slower)."""
    from oracle import lavender_ref as R
    threads = min(16, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    P = R.filled_params("base")
    for v in P.values():
        v.requires_grad_(True)
    B = 2
    batch = synth_batch(B, 5, 224, 32, 0, "cpu")
    torch.manual_seed(88)
    batch["txt"], batch["ans_mtm"] = R.masking(batch["txt"])
    times = []
    for it in range(3):
        t0 = time.time()
        np.random.seed(88)
        out = R.pretrain_forward(P, batch, "base", 12)
        l1, l2 = R.pretrain_loss(out)
        (l1 + l2).backward()
        for v in P.values():
            v.grad = None
        times.append(time.time() - t0)
    t = float(np.median(times[1:]))
    print("CPU_BASELINE " + json.dumps({"value": round(B / t, 4), "unit": "samples/s", "cores": threads, "threads": threads, "host_cpus": os.cpu_count(), "kind": "port",
          "cores_note": "`cores` = intra-op threads the port was given (measured fastest on this host: 8 / 16 / 32 threads = 1.3 / 1.0 / 1.1 s per forward); `host_cpus` = os.cpu_count() of the box",
          "sample": f"Swin-B + 12L fusion + MLM head, B={B}, 5x224^2 + 32 tok, fp32, fwd+loss+bwd, median of 2 (after 1 warm-up), {t:.2f} s/iter"}))


def cpu_baseline(timeout_s=240):
    """Runs the CPU leg in a child process with a hard timeout so it can never stall the benchmark."""
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-only"], capture_output=True, text=True,
                           timeout=timeout_s, env={**os.environ, "HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""})
        for line in r.stdout.splitlines():
            if line.startswith("CPU_BASELINE "):
                return json.loads(line[len("CPU_BASELINE "):])
        return {"value": None, "unit": "samples/s", "cores": 0, "kind": "port", "sample": "cpu leg failed: " + r.stderr[-200:]}
    except subprocess.TimeoutExpired:
        return {"value": None, "unit": "samples/s", "cores": 0, "kind": "port", "sample": f"cpu leg exceeded {timeout_s}s"}


# The switches that turn THIS ROUND's new paths off (read once at import by the library / engine, hence child processes).  The driver's boxes differ
# by +-2.5 %, more than a round usually gains: `ab_baseline` times the same build with these set, back to back with an unmodified child on the same box.
AB_ENV = {"LAV_FIRST_TOUCH": "0", "LAV_FUSION_SRC": "0", "LAV_GEMM_PS": "0"}      # round 6: first-touch weight gradients (no 886 MB fill, no read-modify-write read), one fusion source buffer (no T.cat), phase-shifted two-group GEMM tiles (off = gemm_huge / gemm_h192l)


def child_ms(extra_args=(), env=None, steps=10, warmup=3, timeout_s=150):
    """ms per cfg2 step of a plain child run of this script (no --full: no CPU leg, no side workloads, no reference loop, no roofline)."""
    import subprocess
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(steps), "--warmup", str(warmup), *extra_args],
                       capture_output=True, text=True, timeout=timeout_s, env={**os.environ, **(env or {})})
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if not lines:
        raise RuntimeError(f"child {list(extra_args)} {env or {}} printed no line (rc {p.returncode}): {p.stderr.strip()[-300:]}")
    return json.loads(lines[-1])["ms_per_step"]


def ab_and_dp_legs():
    """After the contract line's measurement, outside its timed region: (1) `ab_baseline` -- this round's new paths switched off vs on, alternating
    child processes on this box (off, on, off, on; 10 steps each); (2) `dp1_overhead_ms` -- a 1-rank RCCL process group with the gradient reducer
    attached (--force-dp) minus the plain child: what the range events, the comm stream and RCCL's kernels cost when there is nobody to talk to --
    the only multi-GPU-relevant number a 1-GPU box can produce."""
    res = {}
    try:
        on, off = [], []
        for _ in range(2):
            if AB_ENV:
                off.append(child_ms(env=AB_ENV))
            on.append(child_ms())
        res["ab_baseline"] = {"env": AB_ENV, "ms_per_step": (round(min(off), 2) if off else None), "ms_per_step_all": [round(x, 2) for x in off],
                              "default_ms_per_step": round(min(on), 2), "default_ms_per_step_all": [round(x, 2) for x in on], "steps": 10,
                              "note": "same build, same box, alternating child processes; `env` switches this round's new paths off"}
        dp = child_ms(extra_args=("--force-dp",))
        res["dp1_overhead_ms"] = round(dp - min(on), 2)
        res["dp1_ms_per_step"] = round(dp, 2)
    except Exception as e:  # a side measurement must never take the contract line down
        res["ab_error"] = f"{type(e).__name__}: {e}"[:600]
    return res


def side_workloads():
    """cfg4 (Swin-L 384^2, B = 8) and cfg5 (retrieval, 8 x 8 pairs) for 5 timed steps each, in plain child runs AFTER the contract line's
    measurement (outside its timed region; the parent is idle meanwhile): the --full record then carries them too.  Not the headline metric."""
    import subprocess
    res = {}
    for wl in ("cfg4", "cfg5"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", wl, "--steps", "5", "--warmup", "2"],
                               capture_output=True, text=True, timeout=180)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
            d = json.loads(line)
            res[wl] = {"ms_per_step": d["ms_per_step"], "samples_per_s": d["value"], "step_mfma_frac": d["config"]["step_mfma_frac"], "steps": d["steps"],
                       "per_gpu_batch": d["config"]["per_gpu_batch"], "workload": d["config"]["workload"].split(",")[0]}
        except Exception as e:  # a side measurement must never take the contract line down
            res[wl] = {"error": f"{type(e).__name__}: {e}"[:200]}
    return res


def full_legs(a, world):
    """The measurements a run makes beyond its headline (set-up, warm-up, timed steps, --dump-outputs, the result line), in the
    order they run after the timed steps.  None of them without --full; the --no-* switches drop single legs of a --full run."""
    if not a.full:
        return []
    legs = []
    if a.workload != "cfg5" and a.input == "resident" and not a.no_ref_loop:
        legs.append("ref_loop")
    legs.append("roofline")
    if world == 1 and a.workload == "cfg2" and not a.no_cpu_baseline:
        legs.append("cpu_baseline")
        if not a.no_side_workloads and a.input == "resident":
            legs.append("children")      # side workloads, A/B and 1-rank RCCL child runs
    return legs


DUMP_PARAM_SAMPLE = 1 << 22       # 16 MB of fp32: the full parameter set of cfg2 is 0.9 GB


def dump_outputs(d, model, agent, last, rank):
    """--dump-outputs: the losses of the last timed step (loss_<name>.npy) and the fp32 parameters it left behind (param_sample.npy: the
    sorted, de-duplicated positions a generator seeded with 0 draws over model.named_parameters() laid end to end, so the same model
    samples the same positions whatever the arena layout).  Called on every rank: under ZeRO-1 gathering the masters is a collective."""
    if agent.dp is not None:
        agent.dp.gather_master()
    if rank != 0:
        return
    os.makedirs(d, exist_ok=True)
    for k, v in last.items():
        np.save(os.path.join(d, f"loss_{k}.npy"), np.asarray(float(v), dtype=np.float32))
    flat = torch.cat([p.detach().reshape(-1) for _, p in model.named_parameters()])
    idx = np.unique(np.random.default_rng(0).integers(0, flat.numel(), DUMP_PARAM_SAMPLE))
    np.save(os.path.join(d, "param_sample.npy"), flat[torch.from_numpy(idx).to(flat.device)].float().cpu().numpy())
    del flat


def arg_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--selftest-launch", action="store_true",
                    help="launch check only (no model, works without a GPU over gloo): every rank joins the process group, "
                         "all-reduces a one and rank 0 prints the observed world size")
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (weak scaling); default 32 (cfg2), 8 (cfg4, cfg5)")
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "cfg4", "cfg5"],
                    help="BASELINE.json configs: cfg2 = headline (Swin-B 224, pretrain MLM); cfg4 = Swin-L 384^2 pretrain; "
                         "cfg5 = retrieval B x B pairing, 26 text tokens.  The driver's contract line is cfg2 (default).")
    ap.add_argument("--size", default=None)
    ap.add_argument("--loss-aware-head", action="store_true",
                    help="opt-in side measurement (NOT the contract line): MLM head + loss on the supervised positions only")
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure what the headline does not need: the reference-loop timing, the GEMM roofline "
                         "(two more steps), the CPU baseline, the cfg4 / cfg5 side workloads and the A/B and 1-rank RCCL child runs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline (and with it the side workloads and child runs)")
    ap.add_argument("--no-side-workloads", action="store_true", help="with --full: skip the cfg4 / cfg5 side measurements and the A/B and 1-rank RCCL child runs")
    ap.add_argument("--no-ref-loop", action="store_true", help="with --full: skip the ms_per_step_reference_loop leg (profile collection: keeps the step count of the run fixed)")
    ap.add_argument("--force-dp", action="store_true",
                    help="side measurement at --gpus 1: join a 1-rank RCCL process group and attach the gradient reducer (what the "
                         "overlap bookkeeping and the comm-stream events cost when there is nobody to talk to)")
    ap.add_argument("--zero1", action="store_true", help="side measurement: args.deepspeed = True (ZeRO-1 reducer)")
    ap.add_argument("--input", default="resident", choices=["resident", "tsv"],
                    help="side measurement 'tsv': every step pulls its batch through the input pipeline (TSV rows of base64 JPEG frames "
                         "-> host Huffman decode -> GPU IDCT / resize / crop / normalise, prefetched) and masks it on the host, inside "
                         "the timed region; the contract value keeps inputs resident in HBM")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned to its caller as DIR/<name>.npy (float32): the losses "
                         "and a fixed, seeded sample of the updated fp32 parameters -- for comparing two builds on the same inputs")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    return ap


def main():
    ap = arg_parser()
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.cpu_baseline_only:
        cpu_baseline_child()
        return

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started as a plain `python bench.py --gpus N`: spawn the N ranks ourselves (same launcher the driver uses) instead
        # of silently running one rank and labelling it N GPUs
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world != a.gpus:
        raise SystemExit(f"bench.py: launched with WORLD_SIZE={world} but --gpus {a.gpus}: refusing to report a {world}-rank run as {a.gpus} GPUs")
    legs = full_legs(a, world)
    import torch.distributed as dist
    use_cuda = torch.cuda.is_available()
    if use_cuda:
        torch.cuda.set_device(local_rank)
        if os.environ.get("LAV_MAIN_HIPRI", "0") != "0":      # probe hook: the dy -> dx chain on a high-priority stream (the weight-gradient stream stays normal)
            torch.cuda.set_stream(torch.cuda.Stream(priority=-1))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl" if use_cuda else "gloo", init_method="env://")
        if dist.get_world_size() != a.gpus:
            raise SystemExit(f"bench.py: process group has {dist.get_world_size()} ranks, --gpus says {a.gpus}")
    elif a.force_dp and not a.selftest_launch:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group(backend="nccl", init_method="env://", rank=0, world_size=1)
    if a.selftest_launch:
        seen = 1
        if world > 1:
            t = torch.ones(1, device="cuda" if use_cuda else "cpu")
            dist.all_reduce(t)
            seen = int(t.item())
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"selftest_launch": True, "n_gpus": a.gpus, "world_observed": seen,
                              "backend": ("nccl" if use_cuda else "gloo") if world > 1 else None}))
        return

    import lavender_amd as LA
    from lavender_amd import hip as K
    from lavender_amd.args import EasyDict
    from lavender_amd.dist import set_seed

    wl = {"cfg2": dict(size="base", S=224, X=32, B=32), "cfg4": dict(size="large", S=384, X=32, B=8),
          "cfg5": dict(size="base", S=224, X=26, B=8)}[a.workload]
    a.size = a.size or wl["size"]
    B, T, S, X = a.batch or wl["B"], 5, wl["S"], wl["X"]
    retrieval = a.workload == "cfg5"
    cfg = dict(num_hidden_layers=a.layers)
    args = EasyDict(vis_backbone_size=a.size, size_img=S, vis_backbone_init="random", kinetics=600, txt_backbone=cfg,
                    txt_backbone_embed_only=True, fusion_encoder=cfg, fusion_encoder_rand_init=True, use_checkpoint=False,
                    size_patch=32, size_batch=B, tokenizer=cfg, enable_task_token=False, enable_prompt=False, temp=0.05,
                    lr=2e-5, decay=1e-3, max_iter=10000, max_grad_norm=1.0, deepspeed=bool(a.zero1), vis_backbone_lr_mul=1.0,
                    dataset=["synthetic"], logging_steps=20, path_output="/tmp/lav_bench", task="pretrain", seed=88,
                    loss_aware_head=bool(a.loss_aware_head))

    class Tok:
        cls_token = "[CLS]"; sep_token = "[SEP]"; pad_token = "[PAD]"; mask_token = "[MASK]"; unk_token = "[UNK]"
        ids = {"[PAD]": 0, "[UNK]": 100, "[CLS]": 101, "[SEP]": 102, "[MASK]": 103, "true": 2995, "false": 6270}

        def convert_tokens_to_ids(self, toks):
            return [self.ids[t] for t in toks]

    set_seed(88)
    model = (LA.LAVENDER_Retrieval_MLM if retrieval else LA.LAVENDER_Pretrain_MLM)(args, Tok()).cuda()
    model.arena()
    agent = (LA.Agent_Retrieval_MLM if retrieval else LA.Agent_Pretrain_MLM)(args, model)
    agent.prepare_dist_model()
    if a.force_dp and world == 1:
        from lavender_amd.dp import ArenaReducer, ZeroOneReducer
        agent.dp = (ZeroOneReducer if a.zero1 else ArenaReducer)(model)
    nparam = sum(p.numel() for p in model.parameters())

    # synthetic batches resident in HBM, labels built like the reference does (host masking, then H2D)
    nb = 2
    batches = []
    torch.manual_seed(88)
    for i in range(nb):
        b = synth_batch(B, T, S, X, rank * 7 + i, "cuda")
        if retrieval:
            b["vid"] = list(range(B))
        else:
            b.update(agent.masking(b["txt"], b["mask"]))
        batches.append(agent.prepare_batch(b))
    np.random.seed(88)
    feed = None
    if a.input == "tsv":
        assert not retrieval, "--input tsv is wired for the pretrain workloads"
        args.size_txt = X
        feed = tsv_feed(args, B, T, rank, world)

    def run_step(i):
        if retrieval:
            return {"mtm": agent.step(batches[i % nb], True, sync=False)}
        if feed is not None:
            b = next(feed)
            b.update(agent.masking(b["txt"], b["mask"]))
            return agent.step(agent.prepare_batch(b), True, sync=False)
        return agent.step(batches[i % nb], True, sync=False)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(a.warmup):
        run_step(i)
    barrier()
    if os.environ.get("LAV_BENCH_HOST_PROFILE"):          # tools: cProfile of the launch thread over a few steps (host-paced side workloads), to stderr
        import cProfile, pstats
        pr = cProfile.Profile(); pr.enable()
        for i in range(10):
            run_step(i)
        pr.disable(); barrier()
        pstats.Stats(pr, stream=sys.stderr).sort_stats("tottime").print_stats(45)
    try:                                                  # RCCL's init banner (NCCL_DEBUG=VERSION in this image) sits in C stdio buffers of EVERY
        import ctypes                                     # rank until exit when stdout is a pipe: flush it now, long before rank 0's JSON line
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(a.steps):
        last = run_step(i)
        evs[i + 1].record()                              # per-step marks on the main stream (median below); the contract value uses the wall clock
    host_ms = (time.perf_counter() - t0) * 1e3 / a.steps  # how long the launch thread needed to ENQUEUE a step (it runs ahead of the GPU when this is below ms_per_step)
    barrier()
    dt = time.perf_counter() - t0
    step_ms = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(a.steps))
    ms_median = step_ms[len(step_ms) // 2]
    ms_p99 = step_ms[min(len(step_ms) - 1, int(0.99 * len(step_ms)))]
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    loss_vals = {k: float(v) for k, v in last.items()}
    if a.dump_outputs:                                    # before the reference loop and the roofline sampling steps move the parameters on
        dump_outputs(a.dump_outputs, model, agent, last, rank)

    # ---- the reference's own loop semantics (go_dl, main_pretrain_mlm.py:202-232 + step :145-176), timed beside the contract value: per
    # step a HOST batch (pinned, as a DataLoader with pin_memory hands it over), masking() on the host, prepare_batch (H2D of frames,
    # ids, labels) and .item() on both losses -- i.e. one device round trip per step and no enqueue run-ahead
    ref_loop_ms = None
    if "ref_loop" in legs and use_cuda:
        host_batches = []
        for i in range(nb):
            hb = synth_batch(B, T, S, X, rank * 7 + i, "cpu")
            host_batches.append({k: v.pin_memory() for k, v in hb.items()})
        n_ref = max(5, min(20, a.steps))

        def ref_step(i):
            hb = host_batches[i % nb]
            b = dict(img=hb["img"], txt=hb["txt"].clone(), mask=hb["mask"])
            b.update(agent.masking(b["txt"], b["mask"]))
            return agent.step(agent.prepare_batch(b), True)         # sync=True: ls_mtm.item(), ls_vtm.item()
        for i in range(2):
            ref_step(i)
        barrier()
        t1 = time.perf_counter()
        for i in range(n_ref):
            ref_step(i)
        barrier()
        ref_loop_ms = (time.perf_counter() - t1) * 1e3 / n_ref
        if world > 1:
            t = torch.tensor([ref_loop_ms], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            ref_loop_ms = float(t.item())

    # ---- dominant-kernel roofline: every K-contiguous (layout 0) GEMM launch of one more step, HIP events on its stream ----
    # every rank runs the sampling step (it contains the gradient all-reduce); only rank 0 instruments and reports
    roof = None
    if "roofline" in legs:
        rec = []
        orig = K.gemm

        def timed(layout, A, Bm, M, N, Kd, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = orig(layout, A, Bm, M, N, Kd, **kw)
            e1.record()
            # algorithmic HBM bytes of the launch: operands once, output once, plus the epilogue tensors it reads / writes
            by = 2.0 * (M * Kd + N * Kd + M * N)
            for k in ("preact", "gelu_in", "residual"):
                if kw.get(k) is not None:
                    by += 2.0 * M * N
            rec.append((layout, 2.0 * M * N * Kd, e0, e1, by))
            return r
        # the stage-level C entries (engine.STAGE_C) enqueue their GEMMs from C, where this Python hook does not see them: the two sampling
        # steps run the per-kernel host path instead -- the same kernels with the same arguments (bit-identical, tests/test_gpu_variants.py),
        # each launch bracketed by its own pair of HIP events on the launch stream
        import lavender_amd.engine as _E
        _stage_c = _E.STAGE_C
        _E.STAGE_C = False
        if rank == 0:
            K.gemm = timed
        run_step(0)
        torch.cuda.synchronize()
        rec_shared = rec
        # the same sampling once more with the weight-gradient side stream off: the timed steps overlap dW kernels with the
        # chain, so the per-launch durations above include sharing the CUs; this pass times each GEMM launch on its own
        rec = []
        _side = _E._DW_SIDE
        _E._DW_SIDE = False
        run_step(0)
        torch.cuda.synchronize()
        _E._DW_SIDE = _side
        _E.STAGE_C = _stage_c
        rec_iso, rec = rec, rec_shared
        K.gemm = orig
        if rank == 0:
            by = {}
            for layout, fl, e0, e1, nbytes in rec:
                d = by.setdefault(layout, [0, 0.0, 0.0, 0.0])
                d[0] += 1; d[1] += fl; d[2] += e0.elapsed_time(e1) * 1e-3; d[3] += nbytes
            n, fl, tm, nb = by[0]
            # HBM bytes per launch from the committed rocprofv3 PMC passes of this same command (profiles/)
            traffic = None
            try:
                with open(os.path.join(ROOT, "profiles", TRAFFIC_FILE + ".json")) as fh:
                    pm = json.load(fh)
                if a.workload == "cfg2" and B == 32 and a.layers == 12 and a.size == "base":
                    traffic = pm["hbm_bytes_per_launch"]
            except Exception:
                traffic = None
            tot_fl = sum(v[1] for v in by.values()); tot_t = sum(v[2] for v in by.values())
            iso = [0, 0.0, 0.0]
            for lay_i, fl_i, e0_i, e1_i, _nb_i in rec_iso:
                if lay_i == 0:
                    iso[0] += 1; iso[1] += fl_i; iso[2] += e0_i.elapsed_time(e1_i) * 1e-3
            roof = {"bound": "mfma", "kernel": "lav_gemm_bf16 layout 0 (forward x.W^T and input-gradient dy.(W^T)^T GEMMs: gemm_ps<256 | 192 rows> / gemm_huge / gemm_big / gemm_kernel<NT>)",
                    "achieved": round(fl / tm / 1e12, 2),
                    "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(fl / tm / 1e12 / PEAK_BF16_TFLOPS, 4), "traffic": traffic,
                    "traffic_unit": f"HBM bytes per launch, STATIC: read from the committed rocprofv3 PMC passes of this same command (FETCH_SIZE x2 + WRITE_SIZE, profiles/{TRAFFIC_FILE}.md), not collected in this run",
                    "algorithmic_bytes_per_launch": round(nb / n),
                    "launches_per_step": n, "avg_launch_us": round(tm / n * 1e6, 2), "avg_launch_gflop": round(fl / n / 1e9, 3),
                    "note": "achieved / avg_launch_us are measured in the shipped configuration, where weight-gradient GEMMs of a second "
                            "stream share the CUs with these launches; `isolated` = same launches with that stream off; the sampling steps issue "
                            "every launch through the per-kernel host path (the stage-level C entries enqueue the identical launches from C)",
                    "isolated": {"achieved": round(iso[1] / iso[2] / 1e12, 2), "frac": round(iso[1] / iso[2] / 1e12 / PEAK_BF16_TFLOPS, 4),
                                 "avg_launch_us": round(iso[2] / max(iso[0], 1) * 1e6, 2)},
                    "all_gemm_layouts": {"launches": sum(v[0] for v in by.values()), "tflops": round(tot_fl / tot_t / 1e12, 2),
                                         "gemm_time_ms_per_step": round(tot_t * 1e3, 2)}}
    if world > 1:
        dist.barrier()

    if rank == 0:
        ms = dt / a.steps * 1e3
        value = world * B * a.steps / dt
        fstep = 3.0 * flops_per_sample(**{"base": {}, "tiny": dict(E=96, depths=(2, 2, 6, 2)),
                                          "large": dict(E=192, win=(8, 12, 12))}.get(a.size, {}), layers=a.layers, S=S, X=X,
                                       n_seq=B if retrieval else 1 + min(B, 4))
        if a.force_dp:
            what_dp = "SIDE CASE 1-rank RCCL reducer attached -- "
        else:
            what_dp = ""
        what = {"cfg2": "cfg2: ", "cfg4": "cfg4 (parity/bench side case): ", "cfg5": "cfg5 retrieval B x B pairing (side case): "}[a.workload]
        if a.loss_aware_head:
            what = "SIDE CASE loss-aware head (labelled positions only, not the reference's full-logit outputs) -- " + what
        out = {"metric": "video-text samples/sec (node) pretrain step, Swin-B 5x224^2 + 32-tok", "value": round(value, 2),
               "unit": "samples/s", "n_gpus": world, "world_size_observed": (dist.get_world_size() if world > 1 else 1),
               "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 2),
               "ms_per_step_reference_loop": (round(ref_loop_ms, 2) if ref_loop_ms is not None else None),
               "ms_per_step_median_hip_events": round(ms_median, 2), "ms_per_step_p99_hip_events": round(ms_p99, 2), "host_enqueue_ms_per_step": round(host_ms, 2),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
               "data": "synthetic" if a.input == "resident" else "SIDE CASE input pipeline in the timed region: fixture JPEG frames (320x240, "
                       "replicated rows) read from a TSV, decoded / resized / cropped on the GPU, host masking, per step",
               "config": {"workload": f"{what_dp}{what}Swin-{a.size}-K600-22k + {a.layers}-layer fusion + MLM head, "
                                      f"{'main_retrieval_mlm' if retrieval else 'main_pretrain_mlm'} path, "
                                      f"fwd+bwd+clip+AdamW, dropout 0.1 / drop-path 0.2 on; "
                                      + ("inputs resident in HBM, labels prebuilt: host masking() + H2D copy are outside the timed region"
                                         if a.input == "resident" else "input pipeline + host masking() inside the timed region"),
                          "loop": "value / ms_per_step: device-scalar losses (agent.step(sync=False): no .item() per step), pre-masked batches resident in HBM; "
                                  "ms_per_step_reference_loop: the reference's go_dl semantics (main_pretrain_mlm.py:202-232, :167-169) -- pinned host batch, "
                                  "host masking(), prepare_batch H2D of frames + ids + labels, .item() on both losses every step",
                          "per_gpu_batch": B, "global_batch": B * world, "frames": T, "size_img": S, "size_txt": X,
                          "parallelism": f"dp{world}", "params_M": round(nparam / 1e6, 2),
                          "algorithmic_tflop_per_step_per_gpu": round(fstep * B / 1e12, 2),
                          "step_mfma_frac": round(value / world * fstep / 1e12 / PEAK_BF16_TFLOPS, 4),
                          "loss": loss_vals},
               "roofline": roof}
        if "cpu_baseline" in legs:
            out["cpu_baseline"] = cpu_baseline()
        if "children" in legs:
            # the children need the HBM this process's caching allocator still holds (a child that finds the device full dies in the HSA runtime)
            import gc
            gc.collect(); torch.cuda.synchronize(); torch.cuda.empty_cache()
            out["hbm_free_gb_before_children"] = round(torch.cuda.mem_get_info()[0] / 2**30, 1)
            out["side_workloads"] = side_workloads()
            out.update(ab_and_dp_legs())
        # RCCL prints its version banner through C stdio, which is flushed at exit when stdout is a pipe: push it out first so that
        # the JSON line is the LAST line of stdout
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
