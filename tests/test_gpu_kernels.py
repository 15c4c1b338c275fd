"""GPU: every HIP kernel family, called through the C ABI, against a plain fp32 reference of the same op
(torch on CPU/GPU for generic math, oracle/lavender_ref.py for the LAVENDER-specific ops).

bf16 tolerances: GEMM-like outputs are compared with |d| <= atol + rtol*|ref| at bf16 resolution (2^-8);
index / mask / counting paths are exact."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16


def K():
    from lavender_amd import hip
    return hip


def rb(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(bf16).cuda()


def close(a, b, atol=2e-2, rtol=2e-2, what=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    lim = atol + rtol * b.abs()
    assert (err <= lim).all(), f"{what}: max err {err.max().item():.4g}, worst excess {(err - lim).max().item():.4g}"


# ---------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("shape", [(128, 128, 64), (200, 136, 96), (77, 40, 160), (384, 250, 768), (1000, 384, 128)])
def test_gemm_layouts(layout, shape):
    M, N, Kd = shape
    pad8 = lambda n: (n + 7) // 8 * 8                      # the ABI wants 16-byte rows: ragged extents live in padded buffers
    A = rb(Kd, pad8(M))[:, :M] if layout == 2 else rb(M, Kd)
    B = rb(N, Kd, seed=1) if layout == 0 else rb(Kd, pad8(N), seed=1)[:, :N]
    out = K().gemm(layout, A, B, M, N, Kd, out_dtype=torch.float32)
    a = A.float().t() if layout == 2 else A.float()
    b = B.float().t() if layout == 0 else B.float()
    close(out, a @ b, atol=1e-3 * math.sqrt(Kd), rtol=1e-3, what=f"gemm layout {layout} {shape}")


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("shape", [(2304, 256, 128), (4100, 512, 192), (2500, 384, 64), (3000, 1000, 256)])
def test_gemm_large_m_kernels(layout, shape):
    """M >= 2048 routes to the 256x128 (three-stage) or, when N % 256 == 0, the 256x256 direct-to-LDS kernels;
    the fused epilogue must behave identically there (bias + GELU + residual + column sums)."""
    M, N, Kd = shape
    A = rb(M, Kd)
    B = rb(N, Kd, seed=1, scale=0.2) if layout == 0 else rb(Kd, N, seed=1, scale=0.2)
    bias, res = torch.randn(N).cuda(), rb(M, N, seed=2)
    cs = torch.zeros(N, device="cuda")
    out = K().gemm(layout, A, B, M, N, Kd, bias=bias, act=1, residual=res, colsum=cs)
    b = B.float().t() if layout == 0 else B.float()
    ref = F.gelu(A.float() @ b + bias) + res.float()
    close(out, ref, atol=3e-2, what=f"large-M gemm layout {layout} {shape}")
    close(cs, ref.sum(0), atol=2.0, rtol=2e-2, what="colsum")


@pytest.mark.parametrize("shape,flags", [((8448, 2048, 128), "bGp"), ((8448, 2048, 192), "bdrO"), ((45120, 768, 128), "bdr"),
                                         ((45120, 768, 64), "gsc"), ((70000, 256, 64), "b")])
def test_gemm_many_tiles_per_cu(shape, flags):
    """Outputs with more 256 (192) x 256 tiles than CUs (several rounds of workgroups; the B = 32 shapes of the benchmark step: 45120-row
    fusion GEMMs on the 192-row loader-wave tiles, column sums accumulated over a tile's row chunks before the flush) with every
    specialised epilogue, against the fp32 reference."""
    M, N, Kd = shape
    A, W = rb(M, Kd), rb(N, Kd, seed=1, scale=0.2)
    o32 = "O" in flags
    kw = {}
    if "b" in flags: kw["bias"] = torch.randn(N).cuda()
    if "G" in flags: kw["act"] = 1
    if "g" in flags: kw["gelu_in"] = rb(M, N, seed=5).abs(); kw["gelu_in_is_grad"] = 1
    if "d" in flags: kw["dropout_p"] = 0.1; kw["seed"] = 4321
    if "s" in flags: kw["row_scale"] = (torch.tensor([1.25, 0.0, 1.25, 1.25] * 8)).cuda(); kw["rows_per_group"] = (M + 31) // 32
    if "r" in flags: kw["residual"] = rb(M, N, seed=2).float() if o32 else rb(M, N, seed=2)
    if "p" in flags: kw["preact"] = torch.zeros(M, N, dtype=bf16, device="cuda"); kw["preact_is_grad"] = 1
    if "c" in flags: kw["colsum"] = torch.zeros(N, device="cuda")
    out = K().gemm(0, A, W, M, N, Kd, out_dtype=torch.float32 if o32 else bf16, **kw)
    torch.cuda.synchronize()
    z = A.float() @ W.float().t()
    if "b" in flags: z = z + kw["bias"]
    if flags == "bGp":
        hh = z.detach().clone().requires_grad_(True)
        y = F.gelu(hh); y.sum().backward()
        close(out, y.detach(), atol=3e-2, what="gelu")
        close(kw["preact"], hh.grad, atol=3e-2, what="stored gelu'")
    elif flags == "b":
        close(out, z, atol=3e-2, what="bias")
    elif flags == "gsc":
        ref = z * kw["gelu_in"].float() * kw["row_scale"].repeat_interleave(kw["rows_per_group"])[:M, None]
        close(out, ref, atol=3e-2, what="gelu' x row scale")
        close(kw["colsum"], ref.sum(0), atol=2.0, rtol=2e-2, what="colsum")
    else:                                                  # dropout: the kept elements are (z / 0.9 + residual), the dropped ones the residual
        o, r = out.float(), kw["residual"].float()
        kept = (o - r).abs() > 0
        assert 0.88 < kept.float().mean().item() < 0.92
        close(torch.where(kept, o, r + z / 0.9), r + z / 0.9, atol=3e-2, what="dropout + residual")


@pytest.mark.parametrize("shape,flags", [((8448, 2048, 64), "b"), ((8448, 2048, 128), "bGp"), ((8449, 2048, 192), "bGp"), ((45121, 768, 192), "bdrO"),
                                         ((45120, 768, 64), "gsc"), ((45120, 768, 320), "bsr"), ((70001, 256, 448), "b")])
def test_gemm_phase_shifted_tiles_are_bit_identical_to_the_two_phase_kernels(shape, flags):
    """gemm_ps_kernel (round 6: the two waves of a SIMD one barrier apart; 256- and 192-row tiles) against the kernels it replaces
    (lav_gemm_select(11, 0): gemm_huge / gemm_h192l) -- same accumulation order, so every output is equal bit for bit; k-loops of 1, 2, 3, 5 and 7
    steps (prologue / tail counts of the operand DMA), ragged last row tile."""
    from lavender_amd import _lib
    M, N, Kd = shape
    A, W = rb(M, Kd), rb(N, Kd, seed=1, scale=0.2)
    o32 = "O" in flags

    def run():
        kw = {}
        if "b" in flags: kw["bias"] = torch.randn(N, generator=torch.Generator().manual_seed(3)).cuda()
        if "G" in flags: kw["act"] = 1
        if "g" in flags: kw["gelu_in"] = rb(M, N, seed=5).abs(); kw["gelu_in_is_grad"] = 1
        if "d" in flags: kw["dropout_p"] = 0.1; kw["seed"] = 4321
        if "s" in flags: kw["row_scale"] = (torch.tensor([1.25, 0.0, 1.25, 1.25] * 8)).cuda(); kw["rows_per_group"] = (M + 31) // 32
        if "r" in flags: kw["residual"] = rb(M, N, seed=2).float() if o32 else rb(M, N, seed=2)
        if "p" in flags: kw["preact"] = torch.zeros(M, N, dtype=bf16, device="cuda"); kw["preact_is_grad"] = 1
        if "c" in flags: kw["colsum"] = torch.zeros(N, device="cuda")
        out = K().gemm(0, A, W, M, N, Kd, out_dtype=torch.float32 if o32 else bf16, **kw)
        torch.cuda.synchronize()
        return out, kw.get("preact"), kw.get("colsum")

    old = K().gemm_select(11, 0)
    try:
        ref = run()
        K().gemm_select(11, 3)
        got = run()
    finally:
        K().gemm_select(11, old)
    assert torch.equal(got[0], ref[0])
    if ref[1] is not None: assert torch.equal(got[1], ref[1])
    if ref[2] is not None: close(got[2], ref[2], atol=1e-2, rtol=1e-4, what="column sums (atomics: order differs)")
    z = A.float() @ W.float().t()
    if flags == "b": close(got[0], z + torch.randn(N, generator=torch.Generator().manual_seed(3)).cuda(), atol=3e-2, what="bias")


@pytest.mark.parametrize("splits", [1, 3])
def test_gemm_tn_contraction_multiple_of_32(splits):
    """Swin stage 3 has 7840 token rows (= 245 x 32, not a multiple of 64): the weight-gradient GEMM takes the ping-pong 256 x 256
    kernel (k-tiles of 32) instead of the 128 x 128 one; drop-path groups of 245 rows straddle k-tiles."""
    M, N, Kd = 1024, 512, 7840
    dY, X = rb(Kd, M), rb(Kd, N, seed=1)
    keep = torch.tensor([1.25, 0.0, 1.25, 0.0] * 8, device="cuda")
    dW = torch.zeros(M, N, device="cuda")
    db = torch.zeros(M, device="cuda")
    K().gemm(2, dY, X, M, N, Kd, out=dW, accumulate=True, splits=splits, k_keep=keep, k_rows_per_group=245, alpha=1.25, rowsum_a=db)
    m = (keep != 0).float().repeat_interleave(245)[:Kd, None].cpu()
    ref = 1.25 * (dY.float().cpu() * m).t() @ X.float().cpu()
    close(dW, ref, atol=0.5, rtol=1e-2, what="dW, K = 245 x 32")
    close(db, 1.25 * (dY.float().cpu() * m).sum(0), atol=0.5, rtol=1e-2, what="fused bias gradient")


def test_gemm_tn_ragged_long_contraction_is_split():
    """A weight gradient whose contraction is long and NOT a multiple of 32 (the fusion encoder's n * L token rows: 40 x 757 = 30280 at cfg4,
    120 x 282 = 33840 at the reference's shipped batch of 24): lav_gemm_bf16 runs the first K - K % 64 rows on the large-tile kernels and
    the tail on the 128 x 128 one; both accumulate, the fused bias gradient included."""
    for (M, N, Kd) in ((768, 768, 30280), (2304, 768, 33840), (768, 384, 4100), (192, 768, 36864), (192, 192, 36872)):      # the last two: Swin-L stage 0 (C = 192 < 256 output rows)
        dY, X = rb(Kd, M, scale=0.5), rb(Kd, N, seed=1, scale=0.5)
        dW = torch.full((M, N), 0.25, device="cuda")
        db = torch.zeros(M, device="cuda")
        sp = K().splits_for(M, N, Kd)
        assert sp > 1
        K().gemm(2, dY, X, M, N, Kd, out=dW, accumulate=True, splits=sp, rowsum_a=db)
        ref = dY.double().cpu().t() @ X.double().cpu() + 0.25
        err = (dW.double().cpu() - ref).abs().max().item()
        assert err < 2e-3 * math.sqrt(Kd), (M, N, Kd, err)
        close(db, dY.float().cpu().sum(0), atol=0.5, rtol=1e-2, what="fused bias gradient, ragged K")


def test_gemm_epilogue_bias_gelu_preact_residual_rowscale():
    M, N, Kd = 300, 264, 128
    A, W, res = rb(M, Kd), rb(N, Kd, seed=1, scale=0.1), rb(M, N, seed=2)
    bias = torch.randn(N).cuda()
    scale = torch.tensor([0.0, 1.25, 1.25], device="cuda")            # 3 samples of 100 rows, first one dropped
    pre = torch.empty(M, N, dtype=bf16, device="cuda")
    out = K().gemm(0, A, W, M, N, Kd, bias=bias, act=1, preact=pre, row_scale=scale, rows_per_group=100, residual=res)
    z = A.float() @ W.float().t() + bias
    close(pre, z, what="preact")
    ref = F.gelu(z) * scale.repeat_interleave(100)[:, None] + res.float()
    close(out, ref, what="gelu+rowscale+residual")
    assert torch.equal(out[:100], res[:100])                           # dropped sample: identity branch, exactly


def test_gemm_gelu_grad_and_colsum():
    M, N, Kd = 260, 136, 96
    dY, W, h = rb(M, Kd), rb(Kd, N, seed=1, scale=0.2), rb(M, N, seed=3)
    cs = torch.zeros(N, device="cuda")
    out = K().gemm(1, dY, W, M, N, Kd, gelu_in=h, colsum=cs)
    hh = h.float().requires_grad_(True)
    F.gelu(hh).sum().backward()
    ref = (dY.float() @ W.float()) * hh.grad
    close(out, ref, what="gelu' epilogue")
    close(cs, ref.sum(0), atol=0.3, rtol=2e-2, what="colsum")


def test_gemm_tn_splitk_rowsum_keep():
    M, N, Kd = 200, 136, 3000                       # dW[M,N] = dY[K,M]^T X[K,N], K = token rows, 3 samples of 1000 rows
    dY, X = rb(Kd, M), rb(Kd, N, seed=1)
    keep = torch.tensor([1.25, 0.0, 1.25], device="cuda")
    dW = torch.zeros(M, N, device="cuda")
    db = torch.zeros(M, device="cuda")
    K().gemm(2, dY, X, M, N, Kd, out=dW, accumulate=True, splits=5, k_keep=keep, k_rows_per_group=1000, alpha=1.25, rowsum_a=db)
    m = (keep != 0).float().repeat_interleave(1000)[:, None].cpu()
    ref = 1.25 * (dY.float().cpu() * m).t() @ X.float().cpu()
    close(dW, ref, atol=0.3, rtol=1e-2, what="dW split-K + keep")
    close(db, 1.25 * (dY.float().cpu() * m).sum(0), atol=0.3, rtol=1e-2, what="fused bias gradient")
    K().gemm(2, dY, X, M, N, Kd, out=dW, accumulate=True, splits=2, k_keep=keep, k_rows_per_group=1000, alpha=1.25)
    close(dW, 2 * ref, atol=0.6, rtol=1e-2, what="accumulation across calls")


@pytest.mark.parametrize("shape", [(512, 512, 3008), (304, 384, 3008), (768, 256, 6016)])
@pytest.mark.parametrize("splits", [1, 3, 11])
def test_gemm_tn_large_tiles_keep_rowsum(shape, splits):
    """Weight-gradient GEMM on the 256x256 / 256x128 tile kernels (M >= 256, K % 64 == 0): split-K through the
    workspace + reduction pass, drop-path row skipping with k-tiles that straddle kept / dropped samples (rows per
    sample = 1000, not a multiple of the 64-row k-tile), fused bias gradient, accumulation across calls."""
    M, N, Kd = shape
    dY, X = rb(Kd, M), rb(Kd, N, seed=1)
    ng = (Kd + 999) // 1000
    keep = torch.tensor([1.25, 0.0, 1.25, 0.0, 0.0, 1.25, 1.25][:ng], device="cuda")
    dW = torch.zeros(M, N, device="cuda")
    db = torch.zeros(M, device="cuda")
    K().gemm(2, dY, X, M, N, Kd, out=dW, accumulate=True, splits=splits, k_keep=keep, k_rows_per_group=1000, alpha=1.25, rowsum_a=db)
    m = (keep != 0).float().repeat_interleave(1000)[:Kd, None].cpu()
    ref = 1.25 * (dY.float().cpu() * m).t() @ X.float().cpu()
    close(dW, ref, atol=0.3, rtol=1e-2, what="dW large tile + keep")
    close(db, 1.25 * (dY.float().cpu() * m).sum(0), atol=0.3, rtol=1e-2, what="fused bias gradient")
    K().gemm(2, dY, X, M, N, Kd, out=dW, accumulate=True, splits=splits)
    close(dW, ref + dY.float().cpu().t() @ X.float().cpu(), atol=0.6, rtol=1e-2, what="accumulation, no keep")


@pytest.mark.parametrize("layout", [0, 1])
def test_gemm_splitk_bf16_output(layout):
    """Workspace split-K of a forward / input-gradient GEMM with a long ragged contraction (K = 30522-like vocabulary)."""
    M, N, Kd = 200, 136, 5002
    ldk = (Kd + 7) // 8 * 8
    A = torch.zeros(M, ldk, device="cuda", dtype=torch.bfloat16)
    A[:, :Kd] = rb(M, Kd, scale=0.1)
    Bm = rb(N, ldk, seed=1, scale=0.1) if layout == 0 else rb(Kd, N, seed=1, scale=0.1)
    if layout == 0:
        Bm[:, Kd:] = 0
    out = K().gemm(layout, A[:, :Kd], Bm[:, :Kd] if layout == 0 else Bm, M, N, Kd, splits=4)
    ref = A[:, :Kd].float() @ (Bm[:, :Kd].float().t() if layout == 0 else Bm.float())
    close(out, ref, atol=2e-2, rtol=1e-2, what="split-K bf16 output")
    assert K().splits_nn(1024, 768, 30522) > 1 and K().splits_nn(36096, 768, 3072) == 1


def test_gemm_splitk_large_tile_and_vocab_rounding():
    """d_hidden = dlogits . W_dec with the contraction rounded up to the row stride of the logits buffer (30522 -> 30528):
    zero padding columns x finite rows past V.  Runs the 256x256 split-K path (workspace + bf16 reduction)."""
    M, N, V = 512, 768, 30522
    ld = (V + 7) // 8 * 8
    assert ld % 64 == 0
    dl = torch.zeros(M, ld, device="cuda", dtype=torch.bfloat16)
    dl[:, :V] = rb(M, V, scale=0.05)
    W = torch.zeros(ld, N, device="cuda", dtype=torch.bfloat16)
    W[:V] = rb(V, N, seed=1, scale=0.05)
    W[V:] = 3.0                                           # "next parameter" rows: must not contribute
    s = K().splits_nn(M, N, ld)
    assert s > 1
    out = K().gemm(1, dl, W, M, N, ld, splits=s)
    ref = dl[:, :V].float() @ W[:V].float()
    close(out, ref, atol=3e-2, rtol=1e-2, what="vocab contraction, rounded K, large-tile split-K")
    out1 = K().gemm(1, dl[:, :V], W[:V], M, N, V)
    close(out1, ref, atol=3e-2, rtol=1e-2, what="vocab contraction, exact K")


def test_batched_weight_transpose_and_arena_copy():
    """lav_transpose_bf16_batched: ragged row counts (30522-like), narrow matrices, several matrices in one launch; and the
    ParamArena keeps W^T (q/k/v fused into one (3H, H) matrix) in step with the bf16 working copy."""
    import numpy as np
    from lavender_amd._lib import MatDesc
    shapes = [(1018, 64), (128, 96), (72, 200), (64, 64)]
    src = torch.zeros(sum(r * c for r, c in shapes) + 64, device="cuda", dtype=torch.bfloat16)
    descs, so, do, t0, mats = [], 0, 0, 0, []
    for r, c in shapes:
        m = rb(r, c, seed=r)
        src[so:so + r * c] = m.reshape(-1)
        ld = (r + 63) // 64 * 64
        descs.append(MatDesc(so, do, r, c, ld, t0))
        mats.append((m, do, ld))
        so += (r * c + 7) // 8 * 8; do += c * ld; t0 += ((r + 63) // 64) * ((c + 63) // 64)
    # offsets must be 8-aligned for the 16-byte loads: rebuild src with aligned offsets
    src.zero_(); so = 0
    for i, (r, c) in enumerate(shapes):
        src[so:so + r * c] = mats[i][0].reshape(-1)
        descs[i].src_off = so
        so += (r * c + 7) // 8 * 8
    dst = torch.zeros(do, device="cuda", dtype=torch.bfloat16)
    arr = (MatDesc * len(descs))(*descs)
    dev = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).cuda()
    K().transpose_batched(len(descs), dev, t0, src, dst)
    for (m, off, ld), (r, c) in zip(mats, shapes):
        got = dst[off:off + c * ld].view(c, ld)
        assert torch.equal(got[:, :r], m.t()), (r, c)
        assert float(got[:, r:].abs().max()) == 0.0 if ld > r else True

    import torch.nn as nn
    from lavender_amd.arena import ParamArena

    class Att(nn.Module):
        def __init__(s):
            super().__init__()
            s.query, s.key, s.value = nn.Linear(64, 64), nn.Linear(64, 64), nn.Linear(64, 64)

    class M(nn.Module):
        def __init__(s):
            super().__init__()
            s.attention = nn.Module(); s.attention.self = Att()
            s.fc = nn.Linear(64, 136)
            s.word_embeddings = nn.Embedding(50, 64)
    mod = M().cuda()
    ar = ParamArena(mod, "cuda")
    q = mod.attention.self.query.weight
    fused = torch.cat([mod.attention.self.query.weight, mod.attention.self.key.weight, mod.attention.self.value.weight]).bfloat16()
    assert q._lav16t.shape == (64, 192) and torch.equal(q._lav16t, fused.t())
    assert torch.equal(mod.fc.weight._lav16t, mod.fc.weight.bfloat16().t()) and not hasattr(mod.word_embeddings.weight, "_lav16t")
    with torch.no_grad():
        mod.fc.weight.mul_(2.0)
    ar.sync_half()
    assert torch.equal(mod.fc.weight._lav16t, mod.fc.weight.bfloat16().t())


def test_gemm_gelu_grad_one_byte_code():
    """preact_is_grad = 2 / gelu_in_is_grad = 2: GELU'(z) stored as one byte per element (q = round((g + 0.25) * 256 / 1.5))."""
    M, N, Kd = 512, 256, 128
    X, W = rb(M, Kd), rb(N, Kd, seed=1, scale=0.2)
    bias = torch.randn(N).cuda()
    code = torch.empty(M, N, device="cuda", dtype=torch.uint8)
    y = K().gemm(0, X, W, M, N, Kd, bias=bias, act=1, preact=code, preact_is_grad=2)
    z = (X.float() @ W.float().t() + bias).detach().requires_grad_(True)
    yr = F.gelu(z)
    yr.sum().backward()
    close(y, yr, what="gelu output")
    dec = code.float() * (1.5 / 256) - 0.25
    assert (dec - z.grad).abs().max().item() < 0.004, (dec - z.grad).abs().max().item()
    dY, W2 = rb(M, 64, seed=2), rb(64, N, seed=3, scale=0.2)           # dh = (dY W2^T^T) * gelu'
    out = K().gemm(0, dY, W2.t().contiguous(), M, N, 64, gelu_in=code, gelu_in_is_grad=2)
    close(out, (dY.float() @ W2.float()) * dec, what="multiply by the decoded GELU'")


def test_gemm_ragged_vocab_tail():
    M, V, Kd = 64, 1018, 128                         # V % 8 == 2 like 30522
    ld = (V + 7) // 8 * 8
    X, W = rb(M, Kd), rb(V, Kd, seed=1, scale=0.1)
    bias = torch.randn(V).cuda()
    buf = torch.full((M, ld), 7.0, dtype=bf16, device="cuda")
    K().gemm(0, X, W, M, V, Kd, out=buf, bias=bias)
    close(buf[:, :V], X.float() @ W.float().t() + bias, what="ragged N")
    assert (buf[:, V:] == 7.0).all()                                     # padding columns untouched
    buf[:, V:] = 0
    dX = K().gemm(1, buf[:, :V], W, M, Kd, V)                             # K-contiguous operand with padded tail
    close(dX, buf[:, :V].float() @ W.float(), atol=5e-2, what="ragged K")


def test_gemm_ragged_vocab_with_writable_padding():
    """lav_gemm_epilogue.c_pad_writable: the vocabulary projection (N % 8 == 2, like 30522) into its row-padded logits buffer on the
    large-tile kernel with full 16-byte chunks.  The N real columns are exact; W and bias are read for N entries only (the buffers end
    right after them: a guard region behind W stays NaN-free in the result); padding columns may hold anything finite."""
    M, V, Kd = 2304, 1018, 128
    ld = (V + 7) // 8 * 8
    X = rb(M, Kd)
    wfull = torch.full(((V + 8) * Kd,), float("nan"), dtype=bf16, device="cuda")      # rows past V are poison
    W = wfull[:V * Kd].view(V, Kd)
    W.copy_(rb(V, Kd, seed=1, scale=0.1))
    bfull = torch.full((V + 8,), float("nan"), device="cuda")
    bias = bfull[:V]
    bias.copy_(torch.randn(V))
    buf = torch.full((M, ld), 7.0, dtype=bf16, device="cuda")
    K().gemm(0, X, W, M, V, Kd, out=buf, bias=bias, c_pad_writable=True)
    close(buf[:, :V], X.float() @ W.float().t() + bias, what="ragged N, writable padding")
    assert torch.isfinite(buf.float()).all()
    ref = torch.full((M, ld), 7.0, dtype=bf16, device="cuda")
    K().gemm(0, X, W, M, V, Kd, out=ref, bias=bias)                      # the generic ragged-N path: same values in the real columns
    assert torch.equal(ref[:, :V], buf[:, :V]) and (ref[:, V:] == 7.0).all()


@pytest.mark.parametrize("shapes,Kd,splits,rpg", [
    ([(512, 2048), (2048, 512), (1536, 512), (512, 512)], 31360 // 4, 3, 980),       # a Swin-B stage-2 block (a quarter of the batch), drop-path masks
    ([(768, 3072), (3072, 768), (2304, 768), (768, 768)], 2 * 282 * 8, 1, 0),         # a fusion layer, no split at all
    ([(1024, 4096), (4096, 1024)], 7840, 2, 245),                                     # stage 3: contraction a multiple of 32, not of 64
    ([(512, 512), (96, 512)], 4096, 2, 0),                                            # a job the large kernel cannot take: everything falls back
])
def test_grouped_weight_gradient_gemm_matches_the_separate_launches(shapes, Kd, splits, rpg):
    """lav_gemm_tn_grouped: up to four C_j += alpha_j A_j^T B_j in one launch of the weight-gradient kernel (bias row sums and stochastic-depth
    row skipping included) against the same products launched one by one: equal up to fp32 summation order (different split factors), and
    ACCUMULATED onto what C held."""
    g = torch.Generator().manual_seed(17)
    jobs, refs = [], []
    for i, (M, N) in enumerate(shapes):
        A, B = rb(Kd, M, scale=0.5, seed=i), rb(Kd, N, scale=0.5, seed=50 + i)
        base = torch.randn(M, N, generator=g).cuda()
        keep = None
        if rpg and i % 2 == 0:
            ns = -(-Kd // rpg)
            keep = (torch.rand(ns, generator=g) > 0.3).float().cuda()
        want_rs = i % 2 == 1
        alpha = 1.25 if keep is not None else 1.0
        o_ref, o_grp = base.clone(), base.clone()
        rs_ref = torch.zeros(M, device="cuda") if want_rs else None
        rs_grp = torch.zeros(M, device="cuda") if want_rs else None
        K().gemm(2, A, B, M, N, Kd, out=o_ref, accumulate=True, splits=K().splits_for(M, N, Kd, keep is not None), rowsum_a=rs_ref, k_keep=keep,
                 k_rows_per_group=rpg or 1, alpha=alpha)
        jobs.append(dict(A=A, B=B, out=o_grp, rowsum_a=rs_grp, k_keep=keep, k_rows_per_group=rpg or 1, alpha=alpha,
                         fallback_splits=K().splits_for(M, N, Kd, keep is not None)))
        refs.append((o_ref, rs_ref, base))
    K().gemm_tn_grouped(jobs, splits)
    torch.cuda.synchronize()
    for j, (o_ref, rs_ref, base) in zip(jobs, refs):
        scale = (o_ref - base).abs().max().item()
        assert scale > 0
        close(j["out"], o_ref, atol=2e-5 * scale + 1e-5, rtol=1e-5, what="grouped weight gradient")
        if rs_ref is not None:
            close(j["rowsum_a"], rs_ref, atol=1e-3 * rs_ref.abs().max().item() + 1e-4, rtol=1e-4, what="grouped bias row sums")


def test_fp16_rows_of_the_residual_stream_gemm_and_layernorm():
    """The fusion encoder's wide residual stream as fp16 rows (lav_gemm_epilogue.out_mode 3 / residual_f32 2, lav_ln_f32.x_f32 2,
    lav_ln_bwd_extra.x_f32 2).  With values that are exactly representable as halves, every kernel must give the SAME bits as with the fp32
    rows: the GEMM epilogue that adds LayerNorm(residual) recomputed from saved pre-LN rows, its fp16 store against the rounded fp32 store,
    LayerNorm forward (statistics included) and backward (dx, dx2, dgamma, dbeta, colsum).  Plus: the store saturates instead of overflowing."""
    M, N, Kd = 4512, 768, 768
    A, Wt = rb(M, Kd, scale=0.5), rb(N, Kd, scale=0.05, seed=1)
    bias = (0.1 * torch.randn(N, generator=torch.Generator().manual_seed(3))).cuda()
    pre32 = (2.0 * torch.randn(M, N, generator=torch.Generator().manual_seed(4))).half().float().cuda()      # halves, held as fp32
    pre16 = pre32.half()
    g = (1.0 + 0.1 * torch.randn(N, generator=torch.Generator().manual_seed(5))).cuda()
    b = (0.1 * torch.randn(N, generator=torch.Generator().manual_seed(6))).cuda()
    # LayerNorm forward on the two row types
    y32, m32, r32 = K().layernorm_fwd(pre32, M, N, g, b, 1e-12)
    y16, m16, r16 = K().layernorm_fwd(pre16, M, N, g, b, 1e-12)
    assert torch.equal(y32, y16) and torch.equal(m32, m16) and torch.equal(r32, r16)
    # GEMM: bias + dropout + residual = LayerNorm(pre) recomputed in the epilogue, fp32 rows in / fp32 out  vs  fp16 rows in / fp16 out
    o32 = K().gemm(0, A, Wt, M, N, Kd, bias=bias, dropout_p=0.1, seed=9, residual=pre32, res_ln=(m32, r32, g, b), out_dtype=torch.float32)
    o16 = K().gemm(0, A, Wt, M, N, Kd, bias=bias, dropout_p=0.1, seed=9, residual=pre16, res_ln=(m16, r16, g, b), out_dtype=torch.float16)
    assert o16.dtype == torch.float16 and torch.equal(o32.half(), o16)
    # plain residual add (no LayerNorm recompute) and the 128 x 128 kernel (small M)
    o32 = K().gemm(0, A[:300], Wt, 300, N, Kd, bias=bias, residual=pre32[:300], out_dtype=torch.float32)
    o16 = K().gemm(0, A[:300], Wt, 300, N, Kd, bias=bias, residual=pre16[:300], out_dtype=torch.float16)
    assert torch.equal(o32.half(), o16)
    # saturation instead of infinity
    big = K().gemm(0, (A * 0 + 200).to(bf16), (Wt * 0 + 1).to(bf16), M, N, Kd, out_dtype=torch.float16)      # 200 * 768 = 153600 > 65504
    assert torch.isfinite(big.float()).all() and (big.float() == 65504.0).all()
    # LayerNorm backward
    dy = rb(M, N, seed=11)
    outs = []
    for x in (pre32, pre16):
        dg, db, cs = (torch.zeros(N, device="cuda") for _ in range(3))
        dx2 = torch.empty(M, N, dtype=bf16, device="cuda")
        dx = K().layernorm_bwd(dy, x, M, N, g, m32, r32, dg, db, dx2=dx2, dropout_p=0.1, seed=13, colsum=cs)
        torch.cuda.synchronize()
        outs.append((dx, dx2, dg, db, cs))
    for u, v, what in zip(outs[0], outs[1], ("dx", "dx2", "dgamma", "dbeta", "colsum")):
        assert torch.equal(u, v), f"LayerNorm backward on fp16 rows: {what} differs from the fp32-row result"


def test_layernorm_bwd_deferred_column_reductions_match_immediate_ones():
    """lav_layernorm_set_defer / lav_layernorm_flush: the row pass queues the reduction of its per-block column partials and ONE launch per
    flush completes all of them.  60 backward calls on three shapes (more than the 48-entry job table: the 49th call flushes by itself),
    two of them accumulating into the SAME vectors, against the same calls completed one by one: dgamma / dbeta / colsum bit-identical
    (the same partials are summed in the same order), dx identical."""
    from lavender_amd import hip as KK
    if not KK.LN_DEFER:
        pytest.skip("LAV_LN_DEFER=0")
    shapes = [(31360, 512), (4512, 768), (7840, 1024)]
    def run(flush_each):
        outs = []
        shared = [torch.zeros(C, device="cuda") for C in (512, 512, 512)]
        for i in range(60):
            rows, C = shapes[i % 3]
            x, dy = rb(rows, C, seed=i), rb(rows, C, seed=100 + i)
            g = (1.0 + 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(7 + i))).cuda()
            _, mean, rstd = KK.layernorm_fwd(x, rows, C, g, torch.zeros(C, device="cuda"), 1e-5)
            if i % 3 == 0 and i < 6:
                dg, db, cs = shared                                               # two calls add into the same three vectors
            else:
                dg, db, cs = (torch.zeros(C, device="cuda") for _ in range(3))
            dx2 = torch.empty(rows, C, dtype=bf16, device="cuda")
            dx = KK.layernorm_bwd(dy, x, rows, C, g, mean, rstd, dg, db, dx2=dx2, dropout_p=0.1, seed=i, colsum=cs, flush=flush_each)
            outs.append((dx, dx2, dg, db, cs))
        KK.layernorm_flush()
        torch.cuda.synchronize()
        return outs
    a, b = run(True), run(False)
    for i, (ta, tb) in enumerate(zip(a, b)):
        for u, v, what in zip(ta, tb, ("dx", "dx2", "dgamma", "dbeta", "colsum")):
            assert torch.equal(u, v), f"call {i}: {what} differs between immediate and deferred reduction"
    assert a[0][2].abs().max() > 0


def test_gemm_dropout_mask_consistent_with_layernorm_bwd():
    """The GEMM epilogue and the LN backward regenerate the SAME counter-based dropout mask."""
    M, N, Kd, p, seed = 256, 128, 64, 0.3, 1234
    ones = torch.ones(M, Kd, dtype=bf16, device="cuda")
    W = (torch.ones(N, Kd) / Kd).to(bf16).cuda()
    y = K().gemm(0, ones, W, M, N, Kd, dropout_p=p, seed=seed).float()        # = mask / (1-p)
    mask = (y > 0).float()
    assert abs(mask.mean().item() - (1 - p)) < 0.02
    close(y, mask / (1 - p), atol=1e-2)
    # LN backward "extra" output = dropout(dx): use gamma=1 and a dy that makes dx easy to compare
    x = rb(M, N, seed=5)
    dy = rb(M, N, seed=6)
    g1 = torch.ones(N, device="cuda")
    _, mean, rstd = K().layernorm_fwd(x, M, N, g1, torch.zeros(N, device="cuda"), 1e-5)
    dg, db = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    dx2 = torch.empty(M, N, dtype=bf16, device="cuda")
    cs = torch.zeros(N, device="cuda")
    dx = K().layernorm_bwd(dy, x, M, N, g1, mean, rstd, dg, db, dx2=dx2, dropout_p=p, seed=seed, colsum=cs)
    close(dx2, dx.float() * mask / (1 - p), atol=1e-2, what="masked LN-bwd output")
    close(cs, (dx.float() * mask / (1 - p)).sum(0), atol=0.2, what="its column sums")


# ---------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("C", [96, 128, 256, 512, 768, 1024, 2048, 3072])
def test_layernorm_fwd_bwd(C):
    rows = 333
    x, dy, add = rb(rows, C), rb(rows, C, seed=1), rb(rows, C, seed=2)
    gamma, beta = (1 + 0.1 * torch.randn(C)).cuda(), (0.1 * torch.randn(C)).cuda()
    y, mean, rstd = K().layernorm_fwd(x, rows, C, gamma, beta, 1e-5)
    xr = x.float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yr = F.layer_norm(xr, (C,), gr, br, 1e-5)
    close(y, yr, what="LN fwd")
    yr.backward(dy.float())
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dx = K().layernorm_bwd(dy, x, rows, C, gamma, mean, rstd, dg, db, add_in=add)
    close(dx, xr.grad + add.float(), atol=3e-2, what="LN dx (+add)")
    close(dg, gr.grad, atol=0.15, rtol=2e-2, what="dgamma")
    close(db, br.grad, atol=0.15, rtol=2e-2, what="dbeta")


def test_layernorm_patch_merge_gather():
    BT, H, W, C0 = 3, 8, 6, 64
    x = rb(BT * H * W, C0)
    gamma, beta = (1 + 0.1 * torch.randn(4 * C0)).cuda(), (0.1 * torch.randn(4 * C0)).cuda()
    rows = BT * H * W // 4
    y, mean, rstd = K().layernorm_fwd(x, rows, 4 * C0, gamma, beta, 1e-5, gather=(H, W, C0))
    xr = x.float().view(BT, H, W, C0).requires_grad_(True)
    cat = torch.cat([xr[:, 0::2, 0::2], xr[:, 1::2, 0::2], xr[:, 0::2, 1::2], xr[:, 1::2, 1::2]], -1)   # video_swin.py:278-282
    yr = F.layer_norm(cat, (4 * C0,), gamma, beta, 1e-5).reshape(rows, 4 * C0)
    close(y, yr, what="gather LN fwd")
    dy = rb(rows, 4 * C0, seed=3)
    yr.backward(dy.float())
    dg, db = torch.zeros(4 * C0, device="cuda"), torch.zeros(4 * C0, device="cuda")
    dx = K().layernorm_bwd(dy, x, rows, 4 * C0, gamma, mean, rstd, dg, db, gather=(H, W, C0))
    close(dx.view(BT, H, W, C0), xr.grad, atol=3e-2, what="gather LN scatter-back")


def test_gemm_reads_a_and_residual_through_a_row_map():
    """lav_gemm_epilogue.a_rowmap / res_rowmap (the fused B x B pair expansion): same bits as the GEMM on the gathered operand."""
    U, M, N, Kd = 700, 2 * 276 + 5, 768, 768
    src = rb(U, Kd, seed=1)
    W = rb(N, Kd, seed=2) * 0.05
    bias = torch.randn(N, device="cuda")
    g = torch.Generator().manual_seed(3)
    rowmap = torch.randint(0, U, (M,), generator=g, dtype=torch.int32).cuda()
    gathered = src[rowmap.long()].contiguous()
    y0 = K().gemm(0, gathered, W, M, N, Kd, bias=bias)
    y1 = K().gemm(0, src, W, M, N, Kd, bias=bias, a_rowmap=rowmap)
    torch.cuda.synchronize()
    ref = gathered.float() @ W.float().t() + bias
    close(y1, ref, atol=3e-2, rtol=2e-2, what="row-mapped GEMM vs fp32 reference")
    # fp32-out + dropout + residual form of the first fusion layer's output projection, residual rows through the map
    y2 = K().gemm(0, gathered, W, M, N, Kd, bias=bias, dropout_p=0.1, seed=11, residual=gathered, out_dtype=torch.float32)
    y3 = K().gemm(0, src, W, M, N, Kd, bias=bias, dropout_p=0.1, seed=11, residual=src, res_rowmap=rowmap, a_rowmap=rowmap, out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(y2, y3)
    close(y0, ref, atol=3e-2, rtol=2e-2, what="gathered GEMM vs fp32 reference")


def test_layernorm_deferred_reductions_of_another_stream_are_completed_by_flush_all():
    """The backward runs on stream A (deferred column reductions queued THERE), the reader calls layernorm_flush() on stream B: every queue is
    completed on its own stream and B waits for it (lav_layernorm_flush_all) -- the gradients are whole, bit-identical to the immediate mode."""
    from lavender_amd import hip as KK
    if not KK.LN_DEFER:
        pytest.skip("LAV_LN_DEFER=0")
    rows, Cn = 45120 // 4, 768
    x, dy = rb(rows, Cn, seed=1), rb(rows, Cn, seed=2)
    gamma = torch.randn(Cn, device="cuda")
    _, mean, rstd = KK.layernorm_fwd(x, rows, Cn, gamma, torch.zeros(Cn, device="cuda"), 1e-5)
    outs = []
    for deferred_on_side in (False, True):
        dg, db, cs = (torch.zeros(Cn, device="cuda") for _ in range(3))
        dx2 = torch.empty_like(x)
        torch.cuda.synchronize()
        if deferred_on_side:
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                dx = KK.layernorm_bwd(dy, x, rows, Cn, gamma, mean, rstd, dg, db, dx2=dx2, dropout_p=0.1, seed=5, colsum=cs, flush=False)
            KK.layernorm_flush()                                   # on the default stream: must also complete what `side` queued
            snap = (dg.clone(), db.clone(), cs.clone())            # enqueued on the default stream, behind the flush's event wait
            torch.cuda.synchronize()
            outs.append((dx,) + snap)
        else:
            dx = KK.layernorm_bwd(dy, x, rows, Cn, gamma, mean, rstd, dg, db, dx2=dx2, dropout_p=0.1, seed=5, colsum=cs)
            torch.cuda.synchronize()
            outs.append((dx, dg, db, cs))
    assert float(outs[0][1].abs().sum()) > 0 and float(outs[0][3].abs().sum()) > 0
    for u, v, what in zip(outs[0], outs[1], ("dx", "dgamma", "dbeta", "colsum")):
        assert torch.equal(u, v), f"{what}: the queue of the other stream was not completed"


def test_two_host_threads_on_two_streams_split_k_gemm_and_deferred_layernorm():
    """The library's mutable state is per stream and mutex-guarded (include/lavender_hip.h conventions): two host threads, each on its own
    stream with its own registered workspaces, run split-K weight-gradient GEMMs and deferred LayerNorm backwards concurrently; every result
    is bit-equal to the same calls made serially on one stream."""
    import threading
    from lavender_amd import hip as KK
    M, N, Kd, rows, Cn = 768, 768, 8192, 6144, 768
    A, Bm = rb(Kd, M, seed=3), rb(Kd, N, seed=4)
    x, dy = rb(rows, Cn, seed=5), rb(rows, Cn, seed=6)
    gamma = torch.randn(Cn, device="cuda")
    _, mean, rstd = KK.layernorm_fwd(x, rows, Cn, gamma, torch.zeros(Cn, device="cuda"), 1e-5)
    torch.cuda.synchronize()

    def work(reps):
        res = []
        for _ in range(reps):
            dW = torch.zeros(M, N, device="cuda")
            KK.gemm(2, A, Bm, M, N, Kd, out=dW, accumulate=True, splits=8)
            dg, db, cs = (torch.zeros(Cn, device="cuda") for _ in range(3))
            dx = KK.layernorm_bwd(dy, x, rows, Cn, gamma, mean, rstd, dg, db, colsum=cs, dx2=torch.empty_like(x), flush=False)
            res.append((dW, dg, db, cs, dx))
        KK.layernorm_flush()
        torch.cuda.current_stream().synchronize()
        return res

    serial = work(6)
    out, err = {}, []

    def runner(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                out[i] = work(6)
        except Exception as e:  # pragma: no cover
            err.append(e)

    ts = [threading.Thread(target=runner, args=(i,)) for i in range(2)]
    for t in ts: t.start()
    for t in ts: t.join()
    assert not err, err
    torch.cuda.synchronize()
    for i in range(2):
        for r, (got, want) in enumerate(zip(out[i], serial)):
            for u, v, what in zip(got, want, ("dW", "dgamma", "dbeta", "colsum", "dx")):
                assert torch.equal(u, v), f"thread {i}, repetition {r}: {what} differs from the serial run"


def test_a_registered_workspace_is_never_outgrown_behind_the_caller():
    """lav_set_workspace: a call that needs more than the registered size fails with LAV_E_WORKSPACE and names the size; nothing is allocated,
    synchronised or freed behind the caller.  Registering a larger buffer makes the same call succeed."""
    import ctypes as C
    from lavender_amd import hip as KK, _lib as L
    M, N, Kd = 768, 768, 4096
    A, Bm = rb(Kd, M, seed=3), rb(Kd, N, seed=4)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        sp = st.cuda_stream
        small = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        L.check(L.lib.lav_set_workspace(C.c_void_p(sp), KK.WS_SPLITK, C.c_void_p(small.data_ptr()), small.numel()))
        KK._workspaces[(sp, KK.WS_SPLITK)] = torch.empty(1 << 30, dtype=torch.uint8, device="meta")     # keep ensure_workspace out of the way
        dW = torch.zeros(M, N, device="cuda")
        with pytest.raises(L.LavenderHipError, match="LAV_WS_SPLITK.*register a larger buffer"):
            KK.gemm(2, A, Bm, M, N, Kd, out=dW, accumulate=True, splits=8)
        del KK._workspaces[(sp, KK.WS_SPLITK)]
        KK.gemm(2, A, Bm, M, N, Kd, out=dW, accumulate=True, splits=8)     # ensure_workspace registers lav_workspace_bytes(kind)
        st.synchronize()
    ref = A.float().t() @ Bm.float()
    close(dW, ref, atol=0.5, rtol=2e-2, what="split-K weight gradient through a caller-owned workspace")
    assert int(L.lib.lav_workspace_bytes(KK.WS_SPLITK)) == 256 << 20


def test_replacing_the_deferred_layernorm_arena_flushes_and_is_picked_up():
    """lav_set_workspace(stream, LAV_WS_LN_DEFER, ...) completes the stream's queued reductions first and the queue re-reads the
    workspace table when empty -- after a replacement nothing is written to the old buffer (it is poisoned here and released), an un-registration
    falls back to the internal allocation, and every result equals the undeferred one bit for bit."""
    import ctypes as C
    from lavender_amd import hip as KK, _lib as L
    rows, Cn = 6144, 768
    x, dy = rb(rows, Cn, seed=5), rb(rows, Cn, seed=6)
    gamma = torch.randn(Cn, device="cuda")
    _, mean, rstd = KK.layernorm_fwd(x, rows, Cn, gamma, torch.zeros(Cn, device="cuda"), 1e-5)

    def bwd(flush):
        dg, db, cs = (torch.zeros(Cn, device="cuda") for _ in range(3))
        KK.layernorm_bwd(dy, x, rows, Cn, gamma, mean, rstd, dg, db, colsum=cs, dx2=torch.empty_like(x), flush=flush)
        return dg, db, cs

    want = bwd(True)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        sp = st.cuda_stream
        KK.ensure_workspace(KK.WS_LN_PARTIALS)
        first = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
        L.check(L.lib.lav_set_workspace(C.c_void_p(sp), KK.WS_LN_DEFER, C.c_void_p(first.data_ptr()), first.numel()))
        KK._workspaces[(sp, KK.WS_LN_DEFER)] = first
        assert L.lib.lav_layernorm_set_defer(C.c_void_p(sp), 1) >= 0
        a = bwd(False)                                                  # queued: partials in `first`
        second = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
        L.check(L.lib.lav_set_workspace(C.c_void_p(sp), KK.WS_LN_DEFER, C.c_void_p(second.data_ptr()), second.numel()))   # flushes the queue
        KK._workspaces[(sp, KK.WS_LN_DEFER)] = second
        st.synchronize()
        for u, v, what in zip(a, want, ("dgamma", "dbeta", "colsum")):
            assert torch.equal(u, v), f"{what}: the reduction queued before the replacement was not completed by it"
        first.fill_(0x7f)                                               # a stale pointer would now read / write garbage
        b = bwd(False)
        L.check(L.lib.lav_layernorm_flush(C.c_void_p(sp)))
        st.synchronize()
        assert bool((first == 0x7f).all()), "the replaced arena was written after lav_set_workspace"
        for u, v, what in zip(b, want, ("dgamma", "dbeta", "colsum")):
            assert torch.equal(u, v), f"{what} differs after the arena was replaced"
        L.check(L.lib.lav_set_workspace(C.c_void_p(sp), KK.WS_LN_DEFER, None, 0))        # un-register: the library's own allocation takes over
        KK._workspaces[(sp, KK.WS_LN_DEFER)] = torch.empty(1, dtype=torch.uint8, device="meta")        # keep ensure_workspace out of the way
        second.fill_(0x7f)
        c = bwd(False)
        L.check(L.lib.lav_layernorm_flush(C.c_void_p(sp)))
        st.synchronize()
        assert bool((second == 0x7f).all()), "the un-registered arena was written"
        for u, v, what in zip(c, want, ("dgamma", "dbeta", "colsum")):
            assert torch.equal(u, v), f"{what} differs after the arena was un-registered"
        assert L.lib.lav_layernorm_set_defer(C.c_void_p(sp), 0) == 1
        del KK._workspaces[(sp, KK.WS_LN_DEFER)]


# ---------------------------------------------------------------------------------------------- attention
def _win_ref(qkv, table, B, D, H, W, C, heads, win, shift, cfg):
    """window attention of video_swin.py:145-170,218-239 on a (tokens, 3C) qkv tensor via the oracle helpers."""
    from oracle import lavender_ref as R
    N = win[0] * win[1] * win[2]
    hd = C // heads
    x = qkv.float().cpu().view(B, D, H, W, 3 * C)
    if any(shift):
        x = torch.roll(x, (-shift[0], -shift[1], -shift[2]), (1, 2, 3))
    xw = R.partition(x, win)                                        # (Bw, N, 3C)
    q, k, v = [t.reshape(-1, N, heads, hd).transpose(1, 2) for t in xw.split(C, -1)]
    att = (q * hd ** -0.5) @ k.transpose(-1, -2)
    idx = R.rel_pos_index(cfg)[:N, :N].reshape(-1)
    att = att + table.float().cpu()[idx].reshape(N, N, heads).permute(2, 0, 1)[None]
    if any(shift):
        m = R.shift_mask(D, H, W, win, shift)
        att = (att.view(B, -1, heads, N, N) + m[None, :, None]).view(-1, heads, N, N)
    o = (att.softmax(-1) @ v).transpose(1, 2).reshape(-1, N, C)
    o = R.unpartition(o, win, B, D, H, W)
    if any(shift):
        o = torch.roll(o, shift, (1, 2, 3))
    return o.reshape(-1, C)


@pytest.mark.parametrize("case", [
    (2, 5, 14, 14, 64, 2, (5, 7, 7), (0, 3, 3)),        # N=245 shifted (persistent path)
    (3, 5, 14, 14, 64, 2, (5, 7, 7), (0, 0, 0)),        # unshifted
    (2, 4, 14, 7, 32, 1, (4, 7, 7), (0, 3, 0)),         # N=196, one axis clamped
    (2, 1, 14, 14, 32, 1, (1, 7, 7), (0, 3, 3)),        # N=49 (image-text data, T=1)
    (1, 16, 14, 14, 32, 1, (8, 7, 7), (4, 3, 3)),       # N=392 > 256: large-window kernels, temporal shift
    (1, 5, 24, 24, 64, 2, (5, 12, 12), (0, 6, 6), (8, 12, 12)),   # N=720 (Swin-L 384^2), shifted: windows with 1, 2 and 4 regions; 3 query parts
    (2, 5, 12, 24, 32, 1, (5, 12, 12), (0, 0, 0), (8, 12, 12)),   # N=720 unshifted
    (90, 5, 12, 12, 32, 1, (5, 12, 12), (0, 0, 0), (8, 12, 12)),  # N=720, 270 items on 256 workgroups (persistent walk)
    (2, 5, 24, 24, 64, 2, (5, 12, 12), (0, 6, 6), (8, 12, 12), 1),  # N=720 shifted, whole problems per workgroup (the many-problem form)
    (1, 16, 14, 14, 32, 1, (8, 7, 7), (4, 3, 3), None, -1),       # N=392 on the GENERIC kernels (what windows of more than 768 tokens use)
])
def test_window_attention_fwd_bwd(case):
    B, D, H, W, C, heads, win, shift = case[:8]
    cfg = case[8] if len(case) > 8 and case[8] else (8, 7, 7)
    M = B * D * H * W
    qkv = rb(M, 3 * C)
    table = (0.5 * torch.randn((2 * cfg[0] - 1) * (2 * cfg[1] - 1) * (2 * cfg[2] - 1), heads)).cuda()
    att = K().Attn(0, heads, 32, B=B, D=D, H=H, W=W, wd=win[0], wh=win[1], ww=win[2], sd=shift[0], sh=shift[1], sw=shift[2],
                   cfg_wd=cfg[0], cfg_wh=cfg[1], cfg_ww=cfg[2], bias_table=table)
    assert (win[0] * win[1] * win[2] <= 256) == hasattr(att, "comb")
    assert (att.plan(0)[0].route == b"window persistent") == hasattr(att, "comb")      # the tables are what selects the persistent kernels
    if len(case) > 9:
        from lavender_amd import _lib
        old_parts = _lib.lib.lav_winl_select(case[9])
        try:
            _window_attention_check(att, case, qkv, table, cfg)
        finally:
            _lib.lib.lav_winl_select(old_parts)
    else:
        _window_attention_check(att, case, qkv, table, cfg)


@pytest.mark.parametrize("case", [
    (2, 5, 14, 14, 2, (5, 7, 7), (0, 3, 3), (8, 7, 7)),       # N=245 shifted: four mask types
    (1, 5, 28, 28, 4, (5, 7, 7), (0, 0, 0), (8, 7, 7)),       # unshifted, 16 windows
    (2, 1, 14, 14, 1, (1, 7, 7), (0, 3, 3), (8, 7, 7)),       # N=49
    (2, 4, 14, 7, 3, (4, 7, 7), (0, 3, 0), (8, 7, 7)),        # N=196, one shifted axis
    (1, 16, 7, 7, 2, (8, 7, 7), (4, 0, 0), (8, 7, 7)),        # N=392 does not take this path; (8,7,7) clamps nothing here: skipped below
    (1, 5, 12, 12, 2, (5, 6, 6), (0, 3, 3), (8, 12, 12)),     # spatial window clamped below the configured one: N=180
])
def test_window_bias_tables_through_the_geometry_map_are_bit_identical(case):
    """lav_attn_desc.bias_map: the (bias + shift mask + key padding) fragment tables built by a gather through the per-geometry index map
    equal the tables built with the index arithmetic in the kernel, bit for bit, and follow the CURRENT bias table (second build after the
    table changed)."""
    from lavender_amd import hip as KK
    B, D, H, W, heads, win, shift, cfg = case
    if win[0] * win[1] * win[2] > 256:
        pytest.skip("large windows do not use the precomputed tables")
    table = (0.5 * torch.randn((2 * cfg[0] - 1) * (2 * cfg[1] - 1) * (2 * cfg[2] - 1), heads)).cuda()
    def build(use_map):
        old = KK.BIAS_MAP
        KK.BIAS_MAP = use_map
        try:
            att = KK.Attn(0, heads, 32, B=B, D=D, H=H, W=W, wd=win[0], wh=win[1], ww=win[2], sd=shift[0], sh=shift[1], sw=shift[2],
                          cfg_wd=cfg[0], cfg_wh=cfg[1], cfg_ww=cfg[2], bias_table=table)
        finally:
            KK.BIAS_MAP = old
        torch.cuda.synchronize()
        return att
    a0, a1 = build(False), build(True)
    assert hasattr(a1, "_bias_map") and not hasattr(a0, "_bias_map")
    assert torch.equal(a0.comb.view(torch.int16), a1.comb.view(torch.int16)) and torch.equal(a0.combT.view(torch.int16), a1.combT.view(torch.int16))
    table.mul_(-1.5)                                                          # the optimizer moved the table: the cached map still applies
    b0, b1 = build(False), build(True)
    assert torch.equal(b0.comb.view(torch.int16), b1.comb.view(torch.int16)) and torch.equal(b0.combT.view(torch.int16), b1.combT.view(torch.int16))
    assert not torch.equal(a1.comb.view(torch.int16), b1.comb.view(torch.int16))


@pytest.mark.parametrize("case", [
    (2, 5, 14, 14, 64, 2, (5, 7, 7), (0, 3, 3)),        # N=245 shifted
    (3, 5, 14, 14, 128, 4, (5, 7, 7), (0, 0, 0)),       # four heads, unshifted
    (2, 1, 14, 14, 32, 1, (1, 7, 7), (0, 3, 3)),        # N=49
    (2, 4, 14, 7, 96, 3, (4, 7, 7), (0, 3, 0)),         # N=196, three heads
])
def test_window_attention_head_major_qkv(case):
    """Round 4: the persistent window kernels fetch q / k / v from a HEAD-MAJOR operand [q | k | v][head][token][32]
    (lav_attn_desc.qkv_headmajor; the QKV GEMM epilogue writes it, lav_gemm_epilogue.hm_*): forward, dQ / dK / dV and the split
    bias-table gradient are bit-identical to the row-major layout on the same values."""
    B, D, H, W, C, heads, win, shift = case
    cfg = (8, 7, 7)
    M = B * D * H * W
    qkv = rb(M, 3 * C)
    qkv_hm = qkv.view(M, 3, heads, 32).permute(1, 2, 0, 3).contiguous().view(M, 3 * C)     # same bytes count, head-major order
    table = (0.5 * torch.randn((2 * cfg[0] - 1) * (2 * cfg[1] - 1) * (2 * cfg[2] - 1), heads)).cuda()
    dout = rb(M, C, seed=9)
    res = []
    for hm, x in ((0, qkv), (1, qkv_hm)):
        att = K().Attn(0, heads, 32, B=B, D=D, H=H, W=W, wd=win[0], wh=win[1], ww=win[2], sd=shift[0], sh=shift[1], sw=shift[2],
                       cfg_wd=cfg[0], cfg_wh=cfg[1], cfg_ww=cfg[2], bias_table=table, qkv_headmajor=hm)
        lse = torch.empty(att.lse_elems(), device="cuda")
        out = torch.empty(M, C, dtype=bf16, device="cuda")
        att.fwd(x, out, lse)
        dqkv, dtab = torch.empty(M, 3 * C, dtype=bf16, device="cuda"), torch.zeros_like(table)
        att.bwd(x, out, dout, lse, dqkv, None)
        att.bwd_bias(x, dout, lse, dtab)
        torch.cuda.synchronize()
        res.append((out, dqkv, dtab))
    assert torch.equal(res[0][0], res[1][0]), "forward differs between the layouts"
    assert torch.equal(res[0][1], res[1][1]), "dqkv (row-major in both cases) differs"
    assert torch.allclose(res[0][2], res[1][2], rtol=1e-4, atol=1e-4), "bias-table gradient differs"      # fp32 atomics across workgroups
    # and the reference, once
    qr = qkv.float().cpu().requires_grad_(True)
    tr = table.float().cpu().requires_grad_(True)
    ref = _win_ref(qr, tr, B, D, H, W, C, heads, win, shift, cfg)
    close(res[1][0], ref, atol=2e-2, what=f"head-major window fwd {case}")
    ref.backward(dout.float().cpu())
    close(res[1][1], qr.grad, atol=4e-2, rtol=4e-2, what=f"head-major window dqkv {case}")


def test_gemm_head_major_store():
    """lav_gemm_epilogue.hm_*: the fused q | k | v projection stored as [q | k | v][head][row][32] -- through the 256-wide tile kernel
    (M >= 2048, N % 256 == 0), the 256 x 128 one and the generic 128 x 128 one (ragged M)."""
    for M, heads, Kd in ((2304, 8, 128), (2500, 4, 64), (300, 2, 96), (77, 1, 64)):
        C = heads * 32
        X, W = rb(M, Kd), rb(3 * C, Kd, seed=1, scale=0.2)
        bias = torch.randn(3 * C).cuda()
        ref = K().gemm(0, X, W, M, 3 * C, Kd, bias=bias)
        hm = K().gemm(0, X, W, M, 3 * C, Kd, bias=bias, headmajor=(heads, 32))
        assert torch.equal(hm.reshape(3, heads, M, 32).permute(2, 0, 1, 3).reshape(M, 3 * C), ref), (M, heads, Kd)
        close(ref, X.float() @ W.float().t() + bias, what="qkv projection")


def _window_attention_check(att, case, qkv, table, cfg):
    B, D, H, W, C, heads, win, shift = case[:8]
    M = B * D * H * W
    lse = torch.empty(att.lse_elems(), device="cuda")
    out = torch.empty(M, C, dtype=bf16, device="cuda")
    att.fwd(qkv, out, lse)
    qr = qkv.float().cpu().requires_grad_(True)
    tr = table.float().cpu().requires_grad_(True)
    ref = _win_ref(qr, tr, B, D, H, W, C, heads, win, shift, cfg)
    close(out, ref, atol=2e-2, what=f"window fwd {case}")
    dout = rb(M, C, seed=9)
    ref.backward(dout.float().cpu())
    dqkv = torch.empty_like(qkv)
    dtab = torch.zeros_like(table)
    att.bwd(qkv, out, dout, lse, dqkv, dtab)
    close(dqkv, qr.grad, atol=4e-2, rtol=4e-2, what=f"window dqkv {case}")
    rel = (dtab.cpu() - tr.grad).norm() / tr.grad.norm()
    assert rel < 2e-2, f"bias-table gradient rel err {rel.item():.3g}"
    if att.split_bias_grad:
        # the engine's form: dQ / dK / dV on the main stream, the table gradient as its own launch (lav_attention_bwd_bias)
        dqkv2, dtab2 = torch.empty_like(qkv), torch.zeros_like(table)
        att.bwd(qkv, out, dout, lse, dqkv2, None)
        att.bwd_bias(qkv, dout, lse, dtab2)
        assert torch.equal(dqkv2, dqkv)
        rel2 = (dtab2.cpu() - tr.grad).norm() / tr.grad.norm()
        assert rel2 < 2e-2, f"bias-table gradient (split launch) rel err {rel2.item():.3g}"
        # split launch vs the launch that produces it inside lav_attention_bwd: the same kernel arithmetic, only the order of the fp32
        # atomics across workgroups differs
        rel3 = ((dtab2 - dtab).norm() / dtab.norm()).item()
        assert rel3 < 1e-5, f"split vs fused bias-table gradient differ by {rel3:.3g}"


def _seq_ref(qkv, mask, n, L, heads):
    Hd = heads * 64
    q, k, v = [t.reshape(n, L, heads, 64).transpose(1, 2) for t in qkv.split(Hd, -1)]
    s = q @ k.transpose(-1, -2) / 8.0 + (1.0 - mask[:, None, None, :].float()) * torch.finfo(torch.float32).min
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(n * L, Hd)


@pytest.mark.parametrize("n,L,heads", [(3, 282, 2), (2, 276, 1), (1, 757, 2), (5, 50, 1),
                                       (3, 300, 1), (2, 768, 1), (44, 757, 2),      # chunked long-sequence kernels: 2 chunks / full 3 chunks / 264 items on 256 workgroups
                                       (1, 800, 1)])                               # beyond 768 tokens: the generic kernels
def test_sequence_attention_fwd_bwd(n, L, heads):
    Hd = heads * 64
    qkv = rb(n * L, 3 * Hd)
    mask = torch.ones(n, L, dtype=torch.int32)
    mask[0, L - 7:L - 1] = 0                                          # padded caption tokens
    att = K().Attn(1, heads, 64, n_seq=n, L=L, key_mask=mask.cuda(), dropout_p=0.0, seed=0)
    lse = torch.empty(att.lse_elems(), device="cuda")
    out = torch.empty(n * L, Hd, dtype=bf16, device="cuda")
    att.fwd(qkv, out, lse)
    qr = qkv.float().cpu().requires_grad_(True)
    ref = _seq_ref(qr, mask, n, L, heads)
    close(out, ref, atol=2e-2, what="seq fwd")
    dout = rb(n * L, Hd, seed=4)
    ref.backward(dout.float().cpu())
    dqkv = torch.empty_like(qkv)
    att.bwd(qkv, out, dout, lse, dqkv, None)
    close(dqkv, qr.grad, atol=4e-2, rtol=4e-2, what="seq dqkv")


@pytest.mark.parametrize("n,L,Lv,heads", [(3, 282, 250, 2), (2, 757, 725, 1), (2, 70, 50, 1)])
def test_sequence_attention_seq2seq_mask_fwd_bwd(n, L, Lv, heads):
    """Causal-block mode (lav_attn_desc.causal_from = number of prefix keys; LAVENDER_Base.get_attn_mask "seq2seq",
    model.py:208-218) against fp32 torch on the explicit (n, L, L) mask -- on random rows, where the mask moves the outputs by
    O(1): forward, dQ pass and dK/dV pass."""
    Hd = heads * 64
    qkv = rb(n * L, 3 * Hd)
    km = torch.ones(n, L, dtype=torch.int32)
    km[0, Lv - 9:Lv - 2] = 0                                           # masked video keys (vt_mask), for every query
    att = K().Attn(1, heads, 64, n_seq=n, L=L, key_mask=km.cuda(), dropout_p=0.0, seed=0, causal_from=Lv)
    lse = torch.empty(att.lse_elems(), device="cuda")
    out = torch.empty(n * L, Hd, dtype=bf16, device="cuda")
    att.fwd(qkv, out, lse)
    m3 = torch.zeros(n, L, L)
    m3[:, :, :Lv] = km[:, None, :Lv].float()
    m3[:, Lv:, Lv:] = torch.tril(torch.ones(L - Lv, L - Lv))
    qr = qkv.float().cpu().requires_grad_(True)
    q, k, v = [t.reshape(n, L, heads, 64).transpose(1, 2) for t in qr.split(Hd, -1)]
    sc = q @ k.transpose(-1, -2) / 8.0 + (1.0 - m3[:, None]) * torch.finfo(torch.float32).min
    ref = (sc.softmax(-1) @ v).transpose(1, 2).reshape(n * L, Hd)
    close(out, ref, atol=2e-2, what="seq2seq fwd")
    full = _seq_ref(qkv.float().cpu(), torch.ones(n, L, dtype=torch.int32), n, L, heads)
    assert (full - ref).abs().max() > 0.08                             # the mask is not a no-op on this input (4x the tolerance)
    dout = rb(n * L, Hd, seed=4)
    ref.backward(dout.float().cpu())
    dqkv = torch.empty_like(qkv)
    att.bwd(qkv, out, dout, lse, dqkv, None)
    close(dqkv, qr.grad, atol=4e-2, rtol=4e-2, what="seq2seq dqkv")


def test_sequence_attention_dropout_statistics():
    n, L, heads, p = 4, 282, 2, 0.1
    Hd = heads * 64
    qkv = rb(n * L, 3 * Hd)
    qkv[:, 2 * Hd:] = 1.0                                              # V = 1  ->  out = sum_k dropout(P)_k, mean 1
    outs = []
    for seed in (11, 11, 12):
        att = K().Attn(1, heads, 64, n_seq=n, L=L, key_mask=None, dropout_p=p, seed=seed)
        out = torch.empty(n * L, Hd, dtype=bf16, device="cuda")
        att.fwd(qkv, out, torch.empty(att.lse_elems(), device="cuda"))
        outs.append(out.float())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])     # pure function of the seed
    assert abs(outs[0].mean().item() - 1.0) < 0.01 and outs[0].std().item() > 0.01


@pytest.mark.parametrize("n,L,heads", [(2, 757, 2), (3, 282, 2), (2, 300, 1)])
def test_sequence_attention_dropout_same_mask_fwd_bwd(n, L, heads):
    """Train-mode attention (p = 0.1) of the one-image kernels (L <= 288) AND the chunked long-sequence kernels (288 < L <= 768: cfg4's
    757 tokens) against torch with the SAME dropout mask, rebuilt on the host from the seed (tests/helpers.attn_keep_multiplier):
    a forward / backward mismatch of the regenerated mask (drow / dcol index arithmetic of seql_fwd / seql_dq / seql_dkv) shows here."""
    from tests.helpers import attn_keep_multiplier
    Hd, p, seed = heads * 64, 0.1, 4242
    qkv = rb(n * L, 3 * Hd)
    mask = torch.ones(n, L, dtype=torch.int32)
    mask[0, L - 5:L - 1] = 0
    att = K().Attn(1, heads, 64, n_seq=n, L=L, key_mask=mask.cuda(), dropout_p=p, seed=seed)
    lse = torch.empty(att.lse_elems(), device="cuda")
    out = torch.empty(n * L, Hd, dtype=bf16, device="cuda")
    att.fwd(qkv, out, lse)
    keep = attn_keep_multiplier(seed, n, heads, L, p)                     # (n, heads, L, L): 0 or 1 / (1 - p)
    qr = qkv.float().cpu().requires_grad_(True)
    q, k, v = [t.reshape(n, L, heads, 64).transpose(1, 2) for t in qr.split(Hd, -1)]
    sc = q @ k.transpose(-1, -2) / 8.0 + (1.0 - mask[:, None, None, :].float()) * torch.finfo(torch.float32).min
    ref = ((sc.softmax(-1) * keep) @ v).transpose(1, 2).reshape(n * L, Hd)
    close(out, ref, atol=2.5e-2, what=f"seq fwd with dropout L={L}")
    dout = rb(n * L, Hd, seed=4)
    ref.backward(dout.float().cpu())
    dqkv = torch.empty_like(qkv)
    att.bwd(qkv, out, dout, lse, dqkv, None)
    close(dqkv, qr.grad, atol=5e-2, rtol=5e-2, what=f"seq dqkv with dropout L={L}")


def test_attention_at_the_benchmark_batch_matches_small_batch_slices():
    """Size-independent property at the cfg2 bench shapes (B = 32: 2048-window persistent walks per Swin stage-2 launch, 160-sequence
    fusion batch): a sample's attention output does not depend on the batch it sits in, so the rows of the first two samples / first
    three sequences must be BIT-identical to a small-batch launch on those rows (eval mode: dropout seeds index by global position)."""
    # Swin stage 2: 14 x 14 x 5 tokens, C = 512, 16 heads, shifted; row-major and head-major operands
    D, H, W, C, heads = 5, 14, 14, 512, 16
    table = (0.5 * torch.randn(2535, heads)).cuda()
    tps = D * H * W
    for hm in (0, 1):
        outs = {}
        qkv_full = rb(32 * tps, 3 * C)
        for B in (32, 2):
            x = qkv_full[:B * tps]
            if hm:
                x = x.reshape(B * tps, 3, heads, 32).permute(1, 2, 0, 3).contiguous().view(B * tps, 3 * C)
            att = K().Attn(0, heads, 32, B=B, D=D, H=H, W=W, wd=5, wh=7, ww=7, sd=0, sh=3, sw=3, cfg_wd=8, cfg_wh=7, cfg_ww=7,
                           bias_table=table, qkv_headmajor=hm)
            lse = torch.empty(att.lse_elems(), device="cuda")
            out = torch.empty(B * tps, C, dtype=bf16, device="cuda")
            att.fwd(x, out, lse)
            dout = rb(32 * tps, C, seed=3)[:B * tps]
            dqkv = torch.empty(B * tps, 3 * C, dtype=bf16, device="cuda")
            att.bwd(x, out, dout, lse, dqkv, None)
            torch.cuda.synchronize()
            outs[B] = (out, dqkv)
        assert torch.equal(outs[32][0][:2 * tps], outs[2][0]) and torch.equal(outs[32][1][:2 * tps], outs[2][1]), f"window attention, head-major={hm}"
    # fusion encoder: 160 sequences of 282 tokens, 12 heads
    L, heads = 282, 12
    Hd = heads * 64
    qkv_full = rb(160 * L, 3 * Hd)
    km = torch.ones(160, L, dtype=torch.int32)
    km[1, L - 9:L - 1] = 0
    outs = {}
    for n in (160, 3):
        att = K().Attn(1, heads, 64, n_seq=n, L=L, key_mask=km[:n].contiguous().cuda(), dropout_p=0.0, seed=0)
        lse = torch.empty(att.lse_elems(), device="cuda")
        out = torch.empty(n * L, Hd, dtype=bf16, device="cuda")
        x = qkv_full[:n * L]
        att.fwd(x, out, lse)
        dqkv = torch.empty_like(x)
        att.bwd(x, out, rb(160 * L, Hd, seed=5)[:n * L], lse, dqkv, None)
        torch.cuda.synchronize()
        outs[n] = (out, dqkv)
    assert torch.equal(outs[160][0][:3 * L], outs[3][0]) and torch.equal(outs[160][1][:3 * L], outs[3][1]), "fusion attention"


# ---------------------------------------------------------------------------------------------- embeddings / gathers
def test_patch_im2col_matches_conv3d():
    from oracle import lavender_ref as R
    B, T, H, W, E = 2, 3, 16, 24, 32
    img = torch.randn(B, T, 3, H, W)
    w, b = torch.randn(E, 3, 2, 4, 4) * 0.1, torch.randn(E) * 0.1
    cols = K().patch_im2col(img.cuda(), B, T, H, W, True)
    y = K().gemm(0, cols, w.view(E, 96).to(bf16).cuda(), cols.shape[0], E, 96, bias=b.cuda(), out_dtype=torch.float32)
    x = F.pad(img.transpose(1, 2), (0, 0, 0, 0, 0, 1))
    ref = F.conv3d(x, w, b, stride=(1, 4, 4)).permute(0, 2, 3, 4, 1).reshape(-1, E)
    close(y, ref, atol=3e-2, what="patch embed")


def test_text_embed_fwd_bwd():
    n, X, Hd, V = 3, 32, 128, 500
    ids = torch.randint(0, V, (n, X))
    word, pos, typ = torch.randn(V, Hd) * 0.5, torch.randn(64, Hd) * 0.5, torch.randn(2, Hd) * 0.5
    gamma, beta = 1 + 0.1 * torch.randn(Hd), 0.1 * torch.randn(Hd)
    c = lambda t: t.cuda().contiguous()
    out, mean, rstd = K().text_embed_fwd(c(ids), n, X, Hd, c(word), c(pos), c(typ), c(gamma), c(beta), 1e-12, 0.0, 0)
    ps = [t.clone().requires_grad_(True) for t in (word, pos, typ, gamma, beta)]
    ref = F.layer_norm(ps[0][ids] + ps[1][:X] + ps[2][0], (Hd,), ps[3], ps[4], 1e-12)
    close(out.view(n, X, Hd), ref, what="text embed fwd")
    dout = rb(n * X, Hd, seed=2)
    ref.backward(dout.float().cpu().view(n, X, Hd))
    g = [torch.zeros_like(t).cuda() for t in (word, pos, typ, gamma, beta)]
    K().text_embed_bwd(c(ids), dout, n, X, Hd, c(word), c(pos), c(typ), c(gamma), mean, rstd, 0.0, 0, g[0], g[1], g[2], g[3], g[4])
    for got, p_, name in zip(g, ps, ("word", "pos", "type", "gamma", "beta")):
        ref_g = p_.grad if name != "type" else torch.cat([p_.grad[:1], torch.zeros(1, Hd)])
        close(got, ref_g, atol=0.05, rtol=2e-2, what=f"text embed d{name}")


def test_video_embed_fwd_bwd():
    B, T, hw, Hd = 2, 3, 4, 128
    feat = rb(B * T * hw, Hd)
    cls, pos, ln = torch.randn(1, 1, 1, Hd) * 0.5, torch.randn(1, 1, 1 + 9, Hd) * 0.5, torch.randn(1, 6, 1, Hd) * 0.5
    gamma, beta = 1 + 0.1 * torch.randn(Hd), 0.1 * torch.randn(Hd)
    c = lambda t: t.cuda().contiguous()
    Lv = T * (1 + hw)
    out = torch.empty(B, Lv, Hd, dtype=bf16, device="cuda")
    mean, rstd = K().video_embed_fwd(feat, B, T, hw, Hd, c(cls), c(pos), c(ln), c(gamma), c(beta), 1e-5, out, Lv)
    ps = [t.clone().requires_grad_(True) for t in (cls, pos, ln, gamma, beta)]
    fr = feat.float().cpu().view(B, T, hw, Hd).requires_grad_(True)
    f = torch.cat([ps[0].expand(B, T, 1, Hd), fr], 2) + ps[1][:, :, :1 + hw] + ps[2][:, :T]     # model.py:69-83
    ref = F.layer_norm(f, (Hd,), ps[3], ps[4], 1e-5).view(B, Lv, Hd)
    close(out, ref, what="video embed fwd")
    dout = rb(B, Lv, Hd, seed=3)
    ref.backward(dout.float().cpu())
    g = [torch.zeros_like(t).cuda() for t in (cls, pos, ln, gamma, beta)]
    dfeat = torch.empty_like(feat)
    K().video_embed_bwd(dout, Lv, feat, B, T, hw, Hd, c(cls), c(pos), c(ln), c(gamma), mean, rstd, dfeat, g[0], g[1], g[2], g[3], g[4])
    close(dfeat.view(B, T, hw, Hd), fr.grad, atol=3e-2, what="video embed dfeat")
    for got, p_, name in zip(g, ps, ("cls", "pos", "len", "gamma", "beta")):
        close(got, p_.grad, atol=0.08, rtol=2e-2, what=f"video embed d{name}")


def test_gather_rows_and_gather_sum():
    src = rb(40, 64)
    idx = torch.tensor([3, 3, 39, -1, 0, 7], dtype=torch.int32).cuda()
    out = K().gather_rows(src, idx, 6, 64)
    ref = src[[3, 3, 39, 0, 0, 7]].clone(); ref[3] = 0
    assert torch.equal(out, ref)                                         # pure copy: bit-exact
    start = torch.tensor([0, 2, 2, 5], dtype=torch.int32).cuda()
    lst = torch.tensor([1, 4, 0, 2, 9], dtype=torch.int32).cuda()
    s = K().gather_sum_rows(src, start, lst, 3, 64)
    close(s[0], src[1].float() + src[4].float()); assert (s[1] == 0).all(); close(s[2], src[0].float() + src[2].float() + src[9].float())


# ---------------------------------------------------------------------------------------------- loss / optimizer
def test_cross_entropy_ignore_index():
    rows, V = 37, 1018
    ld = (V + 7) // 8 * 8
    buf = torch.zeros(rows, ld, dtype=bf16, device="cuda")
    buf[:, :V] = rb(rows, V, scale=2.0)
    buf[:, V:] = 99.0                                                   # garbage in the padding must be ignored
    labels = torch.randint(0, V, (rows,))
    labels[::3] = -1
    logits = buf[:, :V].float().cpu().requires_grad_(True)
    ref = F.cross_entropy(logits, labels, ignore_index=-1)
    ref.backward()
    acc = torch.zeros(2, device="cuda")
    K().cross_entropy(buf[:, :V], V, labels.cuda(), acc, 1.0 / int((labels >= 0).sum()), True)
    assert acc[1].item() == int((labels >= 0).sum())
    assert abs((acc[0] / acc[1]).item() - ref.item()) < 2e-3
    close(buf[:, :V], logits.grad, atol=2e-4, rtol=2e-2, what="dlogits")
    assert (buf[:, V:] == 0).all() and (buf[labels < 0] == 0).all()


def test_fused_adamw_matches_torch():
    n = 64 * 50
    p0, g = torch.randn(n), torch.randn(n) * 3
    grp = torch.randint(0, 4, (n // 64,), dtype=torch.uint8)
    lr4, wd4 = [1e-3, 2e-3, 1e-3, 2e-3], [1e-2, 1e-2, 0.0, 0.0]
    ps = [p0[(grp.repeat_interleave(64) == k)].clone().requires_grad_(True) for k in range(4)]
    opt = torch.optim.AdamW([dict(params=[ps[k]], lr=lr4[k], weight_decay=wd4[k]) for k in range(4)], betas=(0.9, 0.98))
    p, m, v = p0.clone().cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
    p16 = torch.empty(n, dtype=bf16, device="cuda")
    for step in (1, 2, 3):
        gs = g * step
        for k in range(4):
            ps[k].grad = gs[(grp.repeat_interleave(64) == k)].clone()
        torch.nn.utils.clip_grad_norm_(ps, 1.0)                         # agent.py:246
        opt.step()
        sq = torch.zeros(1, device="cuda")
        K().sumsq(gs.cuda(), n, sq)
        K().adamw(n, p, gs.cuda(), m, v, p16, grp.cuda(), lr4, wd4, 0.9, 0.98, 1e-8, step, sq, 1.0, 1.0)
    got = p.cpu()
    for k in range(4):
        np.testing.assert_allclose(got[(grp.repeat_interleave(64) == k)].numpy(), ps[k].detach().numpy(), rtol=2e-5, atol=2e-6)
    close(p16, got, atol=1e-2, rtol=1e-2)
