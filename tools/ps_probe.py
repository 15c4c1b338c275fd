"""GPU probe (round 6): the phase-shifted 256 x 256 x 64 GEMM (gemm_ps_kernel: the two waves of a SIMD one barrier apart -- one issues MFMAs while the
other reads fragments and issues the operand DMA) against the shipped kernels, ISOLATED, COLD operands (six rotating buffer sets), with the epilogues
the step uses.  Checks bit identity first, then times interleaved rounds.  python tools/ps_probe.py [n_shapes]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lavender_amd import hip as K, _lib as L
bf, f32, f16 = torch.bfloat16, torch.float32, torch.float16
dev = "cuda"
OPTS = [1, 3]       # lav_gemm_select(11, v): bit 0 = 256-row phase-shifted kernel, bit 1 = 192-row one where the 192-row tiles are chosen
OPT = 3
NSET = 6


def sel(v):
    K.gemm_select(11, v)


def make(M, N, Kd, epi):
    sets = []
    for s in range(NSET):
        torch.manual_seed(100 + s)
        d = dict(A=torch.randn(M, Kd, device=dev).to(bf), W=(0.05 * torch.randn(N, Kd, device=dev)).to(bf), bias=torch.randn(N, device=dev))
        if epi == "b":
            d["out"] = torch.empty(M, N, device=dev, dtype=bf)
        elif epi == "bGp":
            d["out"] = torch.empty(M, N, device=dev, dtype=bf); d["pre"] = torch.empty(M, N, device=dev, dtype=bf)
        elif epi == "bdrO":
            d["out"] = torch.empty(M, N, device=dev, dtype=f16); d["res"] = torch.randn(M, N, device=dev).to(f16)
            d["mean"] = 0.1 * torch.randn(M, device=dev); d["rstd"] = 1.0 + 0.1 * torch.rand(M, device=dev)
            d["g"] = 1.0 + 0.1 * torch.randn(N, device=dev); d["b"] = 0.1 * torch.randn(N, device=dev)
        elif epi == "bsr":
            d["out"] = torch.empty(M, N, device=dev, dtype=bf); d["res"] = torch.randn(M, N, device=dev).to(bf)
            d["rs"] = (torch.rand(M // 245 + 1, device=dev) > 0.1).float() / 0.9
        elif epi == "gc":
            d["out"] = torch.empty(M, N, device=dev, dtype=bf); d["gin"] = torch.rand(M, N, device=dev).to(bf)
            d["rs"] = (torch.rand(M // 245 + 1, device=dev) > 0.1).float() / 0.9; d["cs"] = torch.zeros(N, device=dev)
        sets.append(d)
    return sets


def call(M, N, Kd, epi, d):
    if epi == "b":
        K.gemm(0, d["A"], d["W"], M, N, Kd, out=d["out"], bias=d["bias"])
    elif epi == "bGp":
        K.gemm(0, d["A"], d["W"], M, N, Kd, out=d["out"], bias=d["bias"], act=1, preact=d["pre"], preact_is_grad=True)
    elif epi == "bdrO":
        K.gemm(0, d["A"], d["W"], M, N, Kd, out=d["out"], bias=d["bias"], dropout_p=0.1, seed=3, residual=d["res"], res_ln=(d["mean"], d["rstd"], d["g"], d["b"]))
    elif epi == "bsr":
        K.gemm(0, d["A"], d["W"], M, N, Kd, out=d["out"], bias=d["bias"], row_scale=d["rs"], rows_per_group=245, residual=d["res"])
    elif epi == "gc":
        K.gemm(0, d["A"], d["W"], M, N, Kd, out=d["out"], gelu_in=d["gin"], gelu_in_is_grad=True, row_scale=d["rs"], rows_per_group=245, colsum=d["cs"])


def timed(M, N, Kd, epi, sets, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(reps):
        call(M, N, Kd, epi, sets[r % NSET])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


SHAPES = [(45120, 3072, 768, "bGp"), (45120, 768, 3072, "bdrO"), (31360, 2048, 512, "bGp"),
          (45120, 3072, 768, "b"), (45120, 2304, 768, "b"), (45120, 768, 768, "bdrO"), (45120, 3072, 768, "gc"),
          (45120, 768, 2304, "b"), (31360, 1536, 512, "b"), (31360, 512, 2048, "bsr"), (31360, 512, 512, "bsr"), (31360, 2048, 512, "gc"),
          (125440, 1024, 256, "bGp"), (125440, 256, 1024, "bsr"), (125440, 768, 256, "b"),
          (501760, 512, 128, "bGp"), (501760, 128, 512, "bsr"), (7840, 4096, 1024, "bGp"), (45121, 768, 192, "bdrO")]
if len(sys.argv) > 1:
    SHAPES = SHAPES[:int(sys.argv[1])]
for (M, N, Kd, epi) in SHAPES:
    sets = make(M, N, Kd, epi)
    # bit identity on set 0
    d = sets[0]
    sel(0)
    if "cs" in d: d["cs"].zero_()
    call(M, N, Kd, epi, d); torch.cuda.synchronize()
    ref = {k: d[k].clone() for k in ("out", "pre", "cs") if k in d}
    for k in ("out", "pre"):
        if k in d: d[k].zero_()
    if "cs" in d: d["cs"].zero_()
    sel(3)
    bad = []
    for trial in range(3):
        if "cs" in d: d["cs"].zero_()
        call(M, N, Kd, epi, d); torch.cuda.synchronize()
        for k in ref:
            if k == "cs":
                if not torch.allclose(d[k], ref[k], rtol=1e-4, atol=1e-2): bad.append((trial, k, float((d[k] - ref[k]).abs().max())))
            elif not torch.equal(d[k].view(torch.int16), ref[k].view(torch.int16)):
                bad.append((trial, k, int((d[k].view(torch.int16) != ref[k].view(torch.int16)).sum())))
    ta, tb = [], {o: [] for o in OPTS}
    for rnd in range(5):
        sel(0); timed(M, N, Kd, epi, sets, 6); ta.append(timed(M, N, Kd, epi, sets, 12))
        for o in OPTS:
            sel(o); timed(M, N, Kd, epi, sets, 6); tb[o].append(timed(M, N, Kd, epi, sets, 12))
    ta.sort()
    a = ta[2]
    txt = "  ".join(f"ps[{o}] {sorted(tb[o])[2]:7.1f} us x{a / sorted(tb[o])[2]:5.3f}" for o in OPTS)
    print(f"{M:7d} x {N:5d} x {Kd:5d} {epi:5s} shipped {a:7.1f} us  {txt}  {'BIT-IDENTICAL' if not bad else 'MISMATCH ' + str(bad[:3])}", flush=True)
    del sets
    torch.cuda.empty_cache()
sel(0)
