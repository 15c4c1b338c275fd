"""GPU probe (round 6): fixed per-tile cost vs k-loop cost of the phase-shifted GEMM -- the same M x N output at growing K (cold operands, rotating sets).
The slope is the time of one 64-wide k-step per round of tiles, the intercept what a tile pays outside its k-loop (first operand round trip + epilogue)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lavender_amd import hip as K, _lib as L
bf = torch.bfloat16
dev = "cuda"
NSET = 6
for sel, dbg in ((3, 0), (3, 1), (3, 2), (0, 0), (0, 1), (0, 2)):
    K.gemm_select(11, sel)
    K.gemm_select(5, dbg)
    for (M, N) in ((45120, 3072), (45120, 768)):
        for epi in ("b", "none"):
            rows = []
            for Kd in (64, 256, 768, 3072):
                sets = []
                for s in range(NSET):
                    torch.manual_seed(s)
                    sets.append(dict(A=torch.randn(M, Kd, device=dev).to(bf), W=(0.05 * torch.randn(N, Kd, device=dev)).to(bf), bias=torch.randn(N, device=dev),
                                     out=torch.empty(M, N, device=dev, dtype=bf)))
                def run(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for r in range(reps):
                        d = sets[r % NSET]
                        K.gemm(0, d["A"], d["W"], M, N, Kd, out=d["out"], bias=d["bias"])

                    e1.record(); torch.cuda.synchronize()
                    return e0.elapsed_time(e1) / reps * 1e3
                run(6)
                t = sorted(run(12) for _ in range(5))[2]
                rows.append((Kd, t))
                del sets
            (k0, t0), (k1, t1) = rows[0], rows[-1]
            slope = (t1 - t0) / ((k1 - k0) / 64)
            print(f"ps={sel} dbg={dbg} {M}x{N} " + "  ".join(f"K={k}: {t:6.1f}" for k, t in rows) + f"   us per k-step {slope:5.2f}, intercept {t0 - slope:6.1f} us", flush=True)
            break
K.gemm_select(5, 0)
