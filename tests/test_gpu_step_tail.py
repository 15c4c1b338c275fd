"""GPU: the kernels between a loss and the next step's weights -- cross-entropy (bf16 and fp32 logits), the clip norm, the fused AdamW, the
gradient-exchange casts, the block zeroing and scaling kernels, the matching-score head and the pair key mask -- each against a float64
restatement on the same bf16- or fp32-rounded inputs, at the shapes and edges where such kernels go wrong.

Tolerances are derived from the kernel's arithmetic and written next to each assertion.  u = 2^-24 is the unit roundoff of fp32; a sum of
terms of one sign evaluated through a chain of at most d additions is within d * u * sum|terms| of the exact sum; one bf16 rounding
(round-to-nearest-even, 8 significant bits) is within 2^-8 of the value it rounds.  Where the kernel rounds exactly as an fp32 restatement
does, the comparison is bit for bit."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
U = 2.0 ** -24                  # fp32 unit roundoff
BF_HALF_ULP = 2.0 ** -8         # one bf16 rounding, relative (8 significant bits)
TINY = 2.0 ** -126              # smallest normal fp32: results below it may be flushed by the hardware exp / log


def K():
    from lavender_amd import hip
    return hip


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    """raw bit patterns as int32 (fp32) / int16 (bf16) tensors on the CPU"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _within(got, ref, tol, what):
    got, ref, tol = got.double(), ref.double(), torch.as_tensor(tol, dtype=torch.float64, device=ref.device)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    ratio = float((err / tol.clamp_min(1e-300)).max())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the bound, worst err/bound {ratio:.3g}"
    return ratio


# ------------------------------------------------------------------------------------------------------------ cross-entropy, bf16 logits
def _ce_logits(rows, V, ld, seed):
    """bf16 logits with per-row (spread, offset) cycling over (1, 0), (30, 0), (3, 75), (3, -75), clamped to +-80: the rows near +80 overflow
    fp32 if summed without subtracting the row maximum (30522 * e^78 > 3.4e38).  The padding [V, ld) holds 1e30 garbage."""
    g = _gen(seed)
    spread = torch.tensor([1.0, 30.0, 3.0, 3.0]).repeat((rows + 3) // 4)[:rows, None]
    offset = torch.tensor([0.0, 0.0, 75.0, -75.0]).repeat((rows + 3) // 4)[:rows, None]
    x = (torch.randn(rows, V, generator=g) * spread + offset).clamp(-80, 80).to(bf16)
    buf = torch.full((rows, ld), 1e30, dtype=bf16)
    buf[:, :V] = x
    return buf


def _ce_labels(rows, V, seed, all_ignored=False):
    lab = torch.randint(0, V, (rows,), generator=_gen(seed + 1))
    lab[0] = 0
    if rows > 1:
        lab[1] = V - 1
        lab[2::5] = -1
    else:
        lab[0] = V - 1
    if all_ignored:
        lab[:] = -1
    return lab


@pytest.mark.parametrize("V,ld", [(30522, 30528), (8192, 8192), (2049, 2056), (7, 8)])
@pytest.mark.parametrize("rows", [1, 37, 4097])
def test_cross_entropy_bf16_against_fp64(V, ld, rows):
    """Breaks caught: no max subtraction (the +75 rows overflow to inf), the padding columns entering the max or the sum (1e30 garbage), the label
    logit read after the gradient overwrote it, an off-by-one at label 0 / V - 1, ignored rows counted or given a gradient, the padding left
    unzeroed, grad_scale applied twice or not at all."""
    buf = _ce_logits(rows, V, ld, seed=V + rows)
    lab = _ce_labels(rows, V, seed=V + rows)
    x64 = buf[:, :V].cuda().double()
    lse = torch.logsumexp(x64, 1)
    keep = (lab >= 0).cuda()
    labc = lab.cuda().clamp_min(0)
    xl = x64.gather(1, labc[:, None])[:, 0]
    loss_r = torch.where(keep, lse - xl, torch.zeros_like(lse))
    n = int(keep.sum())
    scale = 1.0 / max(n, 1)
    d = buf.cuda()
    acc = torch.zeros(2, device="cuda")
    K().cross_entropy(d[:, :V], V, lab.cuda(), acc, scale, True)
    torch.cuda.synchronize()
    # the count is a sum of ones in fp32: exact below 2^24
    assert acc[1].item() == n
    # loss: per row, lse = M + log(S) where S sums at most 8 * ceil(ld / 2048) terms per thread and 8 tree levels (relative error
    # (8 * ceil(ld / 2048) + 8) u), each term through __expf (relative error ~2^-21 plus |v - M| u ln 2 <= 2^-21 for the terms that matter),
    # log(S) through __logf (absolute ~2^-21), then two roundings at the scale of |lse| and |x_label|; the rows then meet in fp32 atomics:
    # (rows - 1) u sum|loss_r|
    chain = 8 * math.ceil(ld / 2048) + 8
    e_row = (chain * U + 2 * 2.0 ** -21) + 2.0 ** -21 + 2 * U * (lse.abs() + xl.abs())
    tol = float((e_row * keep).sum() + (rows - 1) * U * loss_r.abs().sum()) + 1e-30
    got, ref = acc[0].item(), float(loss_r.sum())
    print(f"CE bf16 V={V} rows={rows}: loss sum {got:.9g} vs fp64 {ref:.9g}, |d| {abs(got - ref):.3g} (bound {tol:.3g})")
    assert abs(got - ref) <= tol
    # gradient: (softmax - onehot) * grad_scale in fp32, then ONE bf16 rounding.  Before the rounding the fp32 value is off by p * (the lse
    # error above + 2^-21 of __expf + the roundings of the exponent x - lse and of its scaling by log2(e), 2 u |x - lse|) + 2 roundings;
    # below the smallest normal fp32 the hardware may flush to zero.
    p = torch.softmax(x64, 1)
    g64 = (p - torch.nn.functional.one_hot(labc, V).double()) * scale
    g64[~keep] = 0
    pre = (p * (e_row[:, None] + 2.0 ** -21 + 2 * U * (x64 - lse[:, None]).abs()) + 2 * U) * scale + TINY
    tol_g = BF_HALF_ULP * (g64.abs() + pre) + pre
    ratio = _within(d[:, :V], g64, tol_g, "dlogits")
    print(f"   dlogits within {ratio:.3f} of the one-bf16-rounding bound")
    assert bool((d[:, V:] == 0).all()), "padding columns must be zeroed"
    assert bool((d[~keep] == 0).all()), "ignored rows must have a zero gradient"
    # write_grad = 0: same loss, logits untouched bit for bit
    d2 = buf.cuda()
    acc2 = torch.zeros(2, device="cuda")
    K().cross_entropy(d2[:, :V], V, lab.cuda(), acc2, scale, False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(d2), _bits(buf))
    assert acc2[1].item() == n and abs(acc2[0].item() - ref) <= tol


@pytest.mark.parametrize("rows", [1, 37])
def test_cross_entropy_bf16_every_row_ignored(rows):
    """Break caught: an ignored row counted, or its logits left in place (the next GEMM would read them as a gradient)."""
    V, ld = 2049, 2056
    buf = _ce_logits(rows, V, ld, seed=3)
    d = buf.cuda()
    acc = torch.full((2,), 0.25, device="cuda")                  # the kernel ADDS into (loss, count)
    K().cross_entropy(d[:, :V], V, torch.full((rows,), -1, dtype=torch.long, device="cuda"), acc, 1.0, True)
    torch.cuda.synchronize()
    assert acc.tolist() == [0.25, 0.25]
    assert bool((d == 0).all())


# ------------------------------------------------------------------------------------------------------------ cross-entropy, fp32 logits
@pytest.mark.parametrize("O", [1, 2, 4])
@pytest.mark.parametrize("rows", [6, 33])
def test_cross_entropy_f32_against_fp64(O, rows):
    """(B, O) matching scores, one wave per row, four rows per block.  Rows not a multiple of 4 (a block with idle waves), strided rows
    (ld = O + 5, the columns [O, ld) must stay untouched).  Breaks caught: the row index taken from the block only (rows 4k+1.. reading row 4k),
    ld ignored, the label column's -1 missing, an ignored row given a loss."""
    ld = O + 5
    g = _gen(100 * O + rows)
    x = torch.randn(rows, ld, generator=g) * 20
    lab = torch.randint(0, O, (rows,), generator=g)
    lab[3::4] = -1
    keep = lab >= 0
    x64 = x[:, :O].double()
    lse = torch.logsumexp(x64, 1)
    xl = x64.gather(1, lab.clamp_min(0)[:, None])[:, 0]
    loss_r = torch.where(keep, lse - xl, torch.zeros_like(lse))
    scale = 1.0 / int(keep.sum())
    d = x.cuda()
    acc = torch.zeros(2, device="cuda")
    K().cross_entropy(d[:, :O], O, lab.cuda(), acc, scale, True)
    torch.cuda.synchronize()
    assert acc[1].item() == int(keep.sum())
    # per row: O <= 4 terms (64-lane tree, 6 levels), __expf / __logf ~2^-21 each, two roundings at |lse| and |x_label|; rows meet in atomics
    e_row = 6 * U + 2 * 2.0 ** -21 + 2 * U * (lse.abs() + xl.abs())
    tol = float((e_row * keep).sum() + (rows - 1) * U * loss_r.abs().sum())
    assert abs(acc[0].item() - float(loss_r.sum())) <= tol
    # the gradient stays fp32: p * (lse error + 2^-21 + 2 u |x - lse| for the exponent) + two roundings, times grad_scale
    p = torch.softmax(x64, 1)
    g64 = (p - torch.nn.functional.one_hot(lab.clamp_min(0), O).double()) * scale
    g64[~keep] = 0
    pre = p * (e_row[:, None] + 2.0 ** -21 + 2 * U * (x64 - lse[:, None]).abs()) + 3 * U * (g64.abs() / scale + 1)
    _within(d[:, :O].cpu(), g64, pre * scale + TINY, "dlogits f32")
    assert torch.equal(_bits(d[:, O:]), _bits(x[:, O:])), "columns past V must not be written"


# ------------------------------------------------------------------------------------------------------------ sum of squares (clip norm)
@pytest.fixture(scope="module")
def base_arena_total():
    """The Base model's gradient arena size (Video-Swin base + 12-layer fusion encoder), read from a built model."""
    import lavender_amd as LA
    from tests.helpers import Tok, make_args
    m = LA.LAVENDER_Pretrain_MLM(make_args("base", "b12l", 1), Tok()).cuda()
    total = int(m.arena().total)
    del m
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return total


def test_sumsq_against_fp64_up_to_the_base_arena(base_arena_total):
    """Breaks caught: the scalar tail (n mod 4 elements) skipped or counted twice (the last three elements are 1000), `out` overwritten instead
    of added to, a grid that does not cover the whole arena, a reduction whose order depends on timing (two calls must agree bit for bit:
    the clip coefficient of every data-parallel replica comes from this number)."""
    total = base_arena_total
    assert total > 100_000_000
    sizes = [64, 67, 4099, (1 << 20) + 3, total, total + 3]
    buf = torch.empty(total + 64, device="cuda")
    torch.randn(total + 64, out=buf, generator=torch.Generator(device="cuda").manual_seed(5))
    for n in sizes:
        g = buf[:n]
        g[-3:] = 1000.0
        ref = float(g.double().square().sum())
        out = torch.full((1,), 7.0, device="cuda")
        K().sumsq(g, n, out)
        out2 = torch.zeros(1, device="cuda")
        K().sumsq(g, n, out2)
        out3 = torch.zeros(1, device="cuda")
        K().sumsq(g, n, out3)
        torch.cuda.synchronize()
        # all terms are positive, so the fp32 error is at most (longest addition chain) u * sum: per thread 4 adds per float4 of a
        # 1024 x 256-thread grid stride, 3 for the tail thread, 6 + 2 tree levels, 4 partials per thread and 6 + 2 levels in the final
        # pass, one rounding of each square, one for `+=`
        depth = 4 * math.ceil((n // 4) / (1024 * 256)) + 3 + 8 + 4 + 8 + 2
        tol = depth * U * ref
        rel = abs(out2.item() - ref) / ref
        print(f"sumsq n={n}: relative error {rel:.3e} (bound {depth * U:.3e})")
        assert abs(out2.item() - ref) <= tol
        assert abs(out.item() - (7.0 + ref)) <= tol + U * (7.0 + ref)
        assert torch.equal(_bits(out2), _bits(out3)), "sumsq must be deterministic"
        g[-3:] = buf[n + 1]                                       # (restore something random for the next size)


# ------------------------------------------------------------------------------------------------------------ fused clip + AdamW
B1, B2, EPS = 0.9, 0.98, 1e-8
LR4 = [1e-3, 2e-3, 3e-4, 2.5e-3]
WD4 = [1e-2, 5e-2, 0.0, 0.0]


def _f32(x):
    return float(np.float32(x))


def _adamw_case(n, steps, step0, max_norm, grad_div, gscale, seed, skip_blocks=0):
    """Runs lav_adamw_step for `steps` steps (step counter from step0) next to torch.optim.AdamW in float64 with the four parameter groups of
    block_group (hyper-parameters rounded to fp32 as the kernel receives them).  grad_div > 1: the kernel gets the SUM of grad_div rank
    gradients, torch their mean.  Blocks with bit 2 set get no torch update and must stay bit-unchanged.  Returns the worst err/bound ratios."""
    g = _gen(seed)
    nb = n // 64
    grp = torch.randint(0, 4, (nb,), generator=g, dtype=torch.uint8)
    frozen = torch.zeros(nb, dtype=torch.bool)
    if skip_blocks:
        frozen[torch.randperm(nb, generator=g)[:skip_blocks]] = True
        frozen[-1] = True
        grp[frozen] |= 4
    ge = (grp & 3).long().repeat_interleave(64)
    fe = frozen.repeat_interleave(64)
    p0 = torch.randn(n, generator=g)
    m0 = torch.randn(n, generator=g) * 0.01 if step0 > 1 else torch.zeros(n)
    v0 = torch.rand(n, generator=g) * 1e-4 if step0 > 1 else torch.zeros(n)
    lr = [_f32(x) for x in LR4]
    wd = [_f32(x) for x in WD4]
    b1, b2, eps = _f32(B1), _f32(B2), _f32(EPS)
    sel = [(ge == k) & ~fe for k in range(4)]
    ps = [p0[s].double().clone().requires_grad_(True) for s in sel]
    opt = torch.optim.AdamW([dict(params=[ps[k]], lr=lr[k], weight_decay=wd[k]) for k in range(4)], betas=(b1, b2), eps=eps, foreach=False)
    if step0 > 1:
        for k in range(4):
            opt.state[ps[k]] = dict(step=torch.tensor(float(step0 - 1)), exp_avg=m0[sel[k]].double().clone(),
                                    exp_avg_sq=v0[sel[k]].double().clone())
    p, m, v = p0.cuda(), m0.cuda(), v0.cuda()
    p16_0 = torch.full((n,), -7.0, dtype=bf16)                    # frozen blocks keep this sentinel (never p.bf16())
    p16 = p16_0.cuda()
    grp_d = grp.cuda()
    # running error bounds (per element, fp64), see the assertion below
    bp, bm, bv = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(steps):
        step = step0 + t
        ranks = [torch.randn(n, generator=g) * gscale for _ in range(grad_div)]
        gsum = ranks[0].clone()
        for r in ranks[1:]:
            gsum += r                                              # what the exchange leaves in the fp32 arena
        gsum[fe] = 0.0                                             # bit 2: no gradient reaches these parameters, their arena range stays zero
        gmean = gsum.double() / grad_div
        for k in range(4):
            ps[k].grad = gmean[sel[k]].clone()
        coef = 1.0
        if max_norm > 0:
            tn = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))      # agent.py:246, float64, on the mean gradient
            coef = min(1.0, max_norm / (tn + 1e-6))
        opt.step()
        sq = torch.zeros(1, device="cuda")
        gd = gsum.cuda()
        if max_norm > 0:
            K().sumsq(gd, n, sq)
        K().adamw(n, p, gd, m, v, p16, grp_d, lr, wd, b1, b2, eps, step, sq if max_norm > 0 else None, max_norm, float(grad_div))
        # Error bounds, element by element.  The kernel's gradient g / grad_div * c carries the clip coefficient's relative error dc (the sumsq
        # chain halved by the square root, + a few roundings) and one rounding.  m = b1 m + (1 - b1) g: 3 roundings (1 - b1 is exact);
        # v = b2 v + (1 - b2) g^2: 4 roundings; the errors of earlier steps decay with b1 / b2.  The update lr / bc1 * m / (sqrt(v) / sqrt(bc2)
        # + eps): the errors of m and of sqrt(v) (<= min(dv / 2 sqrt(v), sqrt(dv))) plus ~6 roundings and powf's 2 u on beta^step.  p: the
        # decay factor (2 roundings) and the product / subtraction (2 more).
        dc = ((4 * math.ceil(n / 2 ** 20) + 30) / 2 + 6) * U if max_norm > 0 else 0.0
        gk = (gmean * coef).abs() * (1 + dc + U)
        mm, vv, pp = (torch.zeros(n, dtype=torch.float64) for _ in range(3))
        order = torch.cat([torch.nonzero(s)[:, 0] for s in sel])
        mm[order] = torch.cat([opt.state[ps[k]]["exp_avg"] for k in range(4)])
        vv[order] = torch.cat([opt.state[ps[k]]["exp_avg_sq"] for k in range(4)])
        pp[order] = torch.cat([x.detach() for x in ps])
        bm = b1 * bm + 3 * U * (mm.abs() + 2 * (1 - b1) * gk) + (1 - b1) * gk * (dc + U)
        bv = b2 * bv + 4 * U * (vv + 2 * (1 - b2) * gk * gk) + (1 - b2) * gk * gk * 2 * (dc + U)
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        den = vv.sqrt() / math.sqrt(bc2) + eps
        dsq = torch.minimum(bv / (2 * vv.sqrt()).clamp_min(1e-300), bv.sqrt()) / math.sqrt(bc2) + 4 * U * den
        lrv = torch.tensor(lr, dtype=torch.float64)[ge]
        upd = lrv / bc1 * mm.abs() / den
        rel = 6 * U + 2 * U * b1 ** step / bc1 + U * b2 ** step / bc2
        bp = bp + 4 * U * pp.abs() + lrv / bc1 * (bm / den + mm.abs() * dsq / (den * den)) + upd * rel
    torch.cuda.synchronize()
    live = ~fe
    r_p = _within(p.cpu()[live], pp[live], bp[live] + TINY, "p")
    r_m = _within(m.cpu()[live], mm[live], bm[live] + TINY, "m")
    r_v = _within(v.cpu()[live], vv[live], bv[live] + TINY, "v")
    # the bf16 working copy: p rounded once, round-to-nearest-even
    assert torch.equal(_bits(p16)[live.numpy()], _bits(p.cpu().to(bf16))[live.numpy()])
    if skip_blocks:
        fz = fe.numpy()
        assert torch.equal(_bits(p.cpu())[fz], _bits(p0)[fz]) and torch.equal(_bits(m.cpu())[fz], _bits(m0)[fz])
        assert torch.equal(_bits(v.cpu())[fz], _bits(v0)[fz]) and torch.equal(_bits(p16)[fz], _bits(p16_0)[fz])
    return r_p, r_m, r_v


@pytest.mark.parametrize("case", ["clip_active", "clip_inactive", "no_clip", "grad_div_2", "grad_div_8"])
def test_adamw_ten_steps_against_torch_fp64(case):
    """Breaks caught: clip_active -- the clip coefficient not applied or applied to the summed gradient's norm; clip_inactive -- the clip applied
    when the norm is under max_norm (the gradients are ~1e-8 so m and v would scale by ~1e4); no_clip -- max_norm = 0 with gradsq = None still
    reading gradsq or clipping; grad_div -- the rank sum not divided (m 2x / 8x) or the norm not divided before the clip comparison."""
    n = 64 * 997
    kw = dict(clip_active=dict(max_norm=1.0, grad_div=1, gscale=3.0), clip_inactive=dict(max_norm=1.0, grad_div=1, gscale=1e-8),
              no_clip=dict(max_norm=0.0, grad_div=1, gscale=3.0), grad_div_2=dict(max_norm=1.0, grad_div=2, gscale=3.0),
              grad_div_8=dict(max_norm=1.0, grad_div=8, gscale=3.0))[case]
    r = _adamw_case(n, 10, 1, seed=11, skip_blocks=23, **kw)
    print(f"AdamW {case}: worst err/bound p {r[0]:.3f}, m {r[1]:.3f}, v {r[2]:.3f}")


@pytest.mark.parametrize("step0", [1, 2, 1000, 100000])
def test_adamw_bias_correction_at_large_step_counts(step0):
    """fp32 powf bias corrections at steps 1, 2, 1000, 100000 (beta2^1000 ~ 1.7e-9, beta2^100000 underflows).  Break caught: the bias
    correction computed with step - 1 (at step 1 that divides by zero; at step 2 it is off by 2x)."""
    _adamw_case(64 * 311, 3, step0, max_norm=1.0, grad_div=1, gscale=3.0, seed=17 + step0, skip_blocks=5)


def test_adamw_grid_stride_beyond_4096_blocks():
    """n > 4 M elements: 4096 blocks x 256 threads x 4 elements do not cover the arena, the kernel's grid-stride loop must.  Break caught: a loop
    without the stride (the tail past 4 M elements never updated) or a block_group index from the thread instead of the element."""
    _adamw_case((1 << 22) + 64 * 37, 2, 1, max_norm=1.0, grad_div=2, gscale=3.0, seed=23, skip_blocks=40)


# ------------------------------------------------------------------------------------------------------------ casts
def _special_f32():
    """bit patterns: +-0, +-inf, quiet / signalling / negative NaN, around the bf16 overflow threshold (0x7F7F7FFF stays finite, the tie
    0x7F7F8000 and above round to inf), FLT_MAX, subnormals (ties included), the largest subnormal, the smallest normal, RNE ties of normals"""
    pats = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FBFFFFF,
            0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF, 0xFF7F7FFF, 0xFF7F8000, 0xFF7FFFFF,
            0x00000001, 0x80000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x0000FFFF, 0x007FFFFF, 0x807FFFFF, 0x007F8000,
            0x00800000, 0x80800000, 0x3F808000, 0x3F818000, 0x3F80FFFF, 0x3F7FFFFF, 0xBF808000, 0x0001ABCD]
    return torch.tensor(np.array(pats, dtype=np.uint32).view(np.int32)).view(torch.float32)


def _check_bf16_cast(src, got, what):
    ref = src.to(bf16)                                                   # torch: round-to-nearest-even, NaN stays NaN
    nan = torch.isnan(src)
    assert bool(torch.isnan(got.float())[nan].all()), f"{what}: NaN must stay NaN"
    gb, rb = _bits(got)[~nan], _bits(ref)[~nan]
    bad = torch.nonzero(gb != rb)[:, 0]
    assert bad.numel() == 0, (f"{what}: {bad.numel()} values differ from round-to-nearest-even, e.g. input 0x"
                              f"{int(_bits(src[~nan][bad[0]]).item()) & 0xffffffff:08x} -> 0x{int(gb[bad[0]]) & 0xffff:04x}, "
                              f"expected 0x{int(rb[bad[0]]) & 0xffff:04x}")


def test_cast_f32_to_bf16_special_values_in_body_and_tail():
    """lav_cast_f32_to_bf16 converts float4s with v_cvt_pk_bf16_f32 and the n mod 4 tail element by element.  Every special value goes through
    both paths: once in the vector body, once in the scalar tail (n = 4k + 3, three specials at a time).  Break caught: a tail conversion that
    differs from the body (truncation instead of rounding, a NaN turned into inf, subnormals flushed on one path only)."""
    sp = _special_f32()
    rnd = torch.randn(4096, generator=_gen(3)) * torch.logspace(-30, 30, 4096)
    body = torch.cat([sp, rnd, sp])
    body = body[: body.numel() // 4 * 4]
    src = body.cuda()
    out = torch.full((src.numel() + 8,), 3.0, dtype=bf16, device="cuda")
    K().cast_bf16(src, out, src.numel())
    torch.cuda.synchronize()
    _check_bf16_cast(body, out[: body.numel()].cpu(), "vector body")
    assert bool((out[body.numel():] == 3.0).all())
    # the tail: 4k + 3 elements whose last three are specials
    k = 64
    tails = []
    for j in range(0, sp.numel(), 3):
        tri = sp[j:j + 3]
        if tri.numel() < 3:
            tri = torch.cat([tri, sp[: 3 - tri.numel()]])
        s = torch.cat([rnd[: 4 * k], tri])
        d = s.cuda()
        o = torch.full((s.numel() + 5,), 3.0, dtype=bf16, device="cuda")
        K().cast_bf16(d, o, s.numel())
        tails.append((s, o))
    torch.cuda.synchronize()
    for s, o in tails:
        _check_bf16_cast(s, o[: s.numel()].cpu(), "scalar tail")
        assert bool((o[s.numel():] == 3.0).all())


@pytest.mark.parametrize("n", [1, 7, 8, 9, 8 * 4099 + 5])
def test_cast_bf16_to_f32_bit_exact(n):
    """lav_cast_bf16_to_f32 widens 8 at a time with a scalar tail: bit-exact (a widening is a shift, NaN payloads included), nothing written past
    n.  Break caught: the tail loop starting at the wrong element or the last partial group of 8 skipped."""
    g = _gen(n)
    x = (torch.randn(n, generator=g) * 100).to(bf16)
    sp = _special_f32().to(bf16)
    x[: min(n, sp.numel())] = sp[: min(n, sp.numel())]
    x[-min(n, 3):] = sp[-min(n, 3):]
    d = x.cuda()
    out = torch.full((n + 8,), -2.0, device="cuda")
    K().widen_bf16(d, out, n)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:n]), _bits(x.float()))
    assert bool((out[n:] == -2.0).all())


# ------------------------------------------------------------------------------------------------------------ zero_blocks / scale kernels
@pytest.mark.parametrize("blocks", [[5], [0], [9, 2, 31, 0, 17], [31], list(range(31, -1, -3)), []])
@pytest.mark.parametrize("block_elems", [64, 16])
def test_zero_blocks(blocks, block_elems):
    """The listed blocks become zero, every other element keeps its bits (unsorted lists, a single block, the last block, an empty list).
    Break caught: a block index used as an element offset, or a thread of a block writing into its neighbour."""
    nb = 32
    x = torch.randn(nb * block_elems + 64, generator=_gen(block_elems + len(blocks)))
    d = x.cuda()
    K().zero_blocks(d, torch.tensor(blocks, dtype=torch.int32, device="cuda"), block_elems)
    torch.cuda.synchronize()
    ref = x.clone()
    for b in blocks:
        ref[b * block_elems:(b + 1) * block_elems] = 0
    assert torch.equal(_bits(d), _bits(ref))


@pytest.mark.parametrize("count", [None, 0.0, 1.0, 37.0, 4097.0])
def test_scale_by_count_bit_exact(count):
    """x *= gscale / max(count, 1) with the count read on the device (count 0 divides by 1): the kernel's two roundings -- an fp32 product and one
    bf16 rounding -- restated in fp32 on the host give the same bits.  Break caught: a division by the raw count (inf at 0), the loss sum taken
    as the count, truncation instead of rounding."""
    n = 8 * 5003
    x = (torch.randn(n, generator=_gen(4)) * 10).to(bf16)
    gscale = 0.7
    d = x.cuda()
    ls = None if count is None else torch.tensor([123.0, count], device="cuda")
    K().scale_by_count(d, n, ls, gscale)
    torch.cuda.synchronize()
    s32 = torch.tensor(gscale, dtype=torch.float32) / max(count if count is not None else 1.0, 1.0)
    ref = (x.float() * s32).to(bf16)
    assert torch.equal(_bits(d), _bits(ref))
    s64 = gscale / max(count or 1.0, 1.0)
    _within(d.cpu(), x.double() * s64, BF_HALF_ULP * (x.double().abs() * s64) * (1 + 2 ** -7) + 2 * U * x.double().abs() * s64, "scale_by_count vs fp64")


@pytest.mark.parametrize("dtype", [torch.float32, bf16])
@pytest.mark.parametrize("s", [1.0, 0.5, -3.25, 1.0 + 2 ** -20])
def test_scale_by_scalar(dtype, s):
    """x *= scalar on the device, fp32 and bf16.  A scalar of exactly 1 leaves the data bit-identical (NaN payloads included: the kernel returns
    early); otherwise one fp32 product (and one bf16 rounding) restated on the host.  Break caught: 1 + 2^-20 taken for 1, the bf16 path truncating."""
    n = 8 * 3001
    x = (torch.randn(n, generator=_gen(5)) * 10).to(dtype)
    if s == 1.0:
        x[7] = float("nan")
        if dtype == torch.float32:
            x.view(torch.int32)[9] = 0x7FC0_1234
    d = x.cuda()
    K().scale_by_scalar(d, n, torch.tensor([s], device="cuda"))
    torch.cuda.synchronize()
    ref = x.clone() if s == 1.0 else (x.float() * torch.tensor(s, dtype=torch.float32)).to(dtype)
    assert torch.equal(_bits(d), _bits(ref))


# ------------------------------------------------------------------------------------------------------------ matching-score head
@pytest.mark.parametrize("F", [256, 1536, 4096])
@pytest.mark.parametrize("n", [4, 24, 132])
@pytest.mark.parametrize("O", [1, 2, 4])
def test_pair_score_fwd_bwd_against_fp64(F, n, O):
    """Linear(F, 1) over n pair rows, laid out as (n / O, O) logits / temp, and its backward.  F = 4096 takes the backward's second column pass
    (512 chunks of 8 over 256 threads), n = 132 ends in a partial 32-row block, the hidden rows and the logit gradient are strided, dw / db are
    pre-filled.  Breaks caught: dw / db overwritten instead of accumulated, the second column pass skipped, the 32-row block tail dropped or
    overrun, dlogits read with stride O instead of its leading dimension, act_grad ignored."""
    g = _gen(F + n + O)
    inv_temp = 1.0 / 0.05
    hf = (torch.randn(n, F + 24, generator=g)).to(bf16)
    h = hf[:, :F]
    w = (torch.randn(F, generator=g) * 0.05).to(bf16)
    b = torch.randn(1, generator=g)
    # forward: products of two bf16 values are exact in fp32; per lane ceil(F / 512) * 8 sequential adds, 6 tree levels, + b, * inv_temp
    hd, wd, bd = hf.cuda()[:, :F], w.cuda(), b.cuda()
    lg = K().pair_score_fwd(hd, n, F, wd, bd, inv_temp, O)
    torch.cuda.synchronize()
    prod = h.double() * w.double()
    ref = ((prod.sum(1) + float(b)) * inv_temp).view(n // O, O)
    depth = 8 * math.ceil(F / 512) + 6
    tol = (depth * U * prod.abs().sum(1) + 2 * U * (prod.sum(1).abs() + abs(float(b)))) * inv_temp
    _within(lg.cpu(), ref, tol.view(n // O, O) + 1e-30, "pair_score_fwd")
    for with_act in (False, True):
        dlf = torch.randn(n // O, O + 3, generator=g) * 0.1
        dl = dlf[:, :O]
        act = (torch.rand(n, F + 8, generator=g) * 1.2 - 0.1).to(bf16) if with_act else None
        dw0 = torch.randn(F, generator=g)
        db0 = torch.randn(1, generator=g)
        dw_d, db_d = dw0.cuda(), db0.cuda()
        dh = K().pair_score_bwd(dlf.cuda()[:, :O], n, F, O, inv_temp, hd, None if act is None else act.cuda()[:, :F], wd, dw_d, db_d)
        torch.cuda.synchronize()
        dz32 = (dl.reshape(-1) * torch.tensor(inv_temp, dtype=torch.float32)).double()           # dz: one fp32 rounding in the kernel
        gg = act[:, :F].double() if with_act else torch.ones(n, F, dtype=torch.float64)
        dh_ref = dz32[:, None] * w.double()[None, :] * gg
        # dh = dz * w * act': two fp32 roundings, then one bf16 rounding
        _within(dh.cpu(), dh_ref, BF_HALF_ULP * dh_ref.abs() * (1 + 2 ** -7) + 3 * U * dh_ref.abs() + 1e-38, f"dh (act_grad {with_act})")
        # dw += sum_r dz_r h_r: <= 32 rows per block in sequence, then one atomic per block onto the pre-filled value
        terms = dz32[:, None] * h.double()
        dw_ref = dw0.double() + terms.sum(0)
        chain = 32 + math.ceil(n / 32) + 1
        _within(dw_d.cpu(), dw_ref, chain * U * (terms.abs().sum(0) + dw0.double().abs()) + U * terms.abs().sum(0), f"dw (act_grad {with_act})")
        db_ref = float(db0) + float(dz32.sum())
        assert abs(db_d.item() - db_ref) <= chain * U * (float(dz32.abs().sum()) + abs(float(db0))) + U * float(dz32.abs().sum())


# ------------------------------------------------------------------------------------------------------------ pair key mask
def _mask_ref(mask_img, mask_txt, vi, ti):
    """get_attn_mask("full") over the pair list: the video mask of vi[k] followed by the text mask of ti[k]"""
    return torch.cat([mask_img[torch.as_tensor(vi).long()], mask_txt[torch.as_tensor(ti).long()]], 1).int()


@pytest.mark.parametrize("B,nt,Lv,X", [(3, 4, 250, 32), (2, 5, 0, 40), (4, 3, 100, 0), (1, 1, 7, 9)])
def test_pair_key_mask(B, nt, Lv, X):
    """Exact against the restatement, with duplicate pairs, Lv = 0 and X = 0, from host arrays and from device tensors.  Break caught: the
    video / text boundary off by one, a row stride of Lv + X used for the source masks."""
    g = _gen(B * 100 + nt)
    mi = torch.randint(0, 2, (B, Lv), generator=g)
    mt = torch.randint(0, 2, (nt, X), generator=g)
    vi = np.array([0, B - 1, 0, B - 1] + list(torch.randint(0, B, (9,), generator=g).numpy()), dtype=np.int64)
    ti = np.array([nt - 1, 0, nt - 1, 0] + list(torch.randint(0, nt, (9,), generator=g).numpy()), dtype=np.int64)
    ref = _mask_ref(mi, mt, vi, ti)
    got = K().pair_key_mask(mi.cuda(), mt.cuda(), vi, ti)
    got_d = K().pair_key_mask(mi.cuda(), mt.cuda(), torch.tensor(vi, dtype=torch.int32, device="cuda"),
                              torch.tensor(ti, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), ref) and torch.equal(got_d.cpu(), ref)


@pytest.mark.parametrize("bad", ["vi_high", "vi_negative", "ti_high", "ti_negative", "length"])
def test_pair_key_mask_rejects_out_of_range_indices_before_launch(bad, monkeypatch):
    """The kernel reads mask_img[vi[k]] and mask_txt[ti[k]] unchecked: an index outside [0, B) / [0, nt) must raise on the host, and the entry
    point must never be called."""
    from lavender_amd import _lib as L
    B, nt = 3, 5
    mi, mt = torch.ones(B, 10, dtype=torch.long, device="cuda"), torch.ones(nt, 6, dtype=torch.long, device="cuda")
    vi, ti = np.array([0, 1, 2, 1]), np.array([4, 0, 3, 2])
    if bad == "vi_high":
        vi[2] = B
    elif bad == "vi_negative":
        vi[0] = -1
    elif bad == "ti_high":
        ti[1] = nt
    elif bad == "ti_negative":
        ti[3] = -2
    else:
        ti = ti[:3]
    calls = []
    monkeypatch.setattr(L.lib, "lav_pair_key_mask", lambda *a: calls.append(a) or 0)
    with pytest.raises(ValueError, match="pair_key_mask"):
        K().pair_key_mask(mi, mt, vi, ti)
    with pytest.raises(ValueError, match="pair_key_mask"):
        K().pair_key_mask(mi, mt, torch.as_tensor(vi, dtype=torch.int32, device="cuda"), torch.as_tensor(ti, dtype=torch.int32, device="cuda"))
    assert calls == []


# ------------------------------------------------------------------------------------------------------------ row scale / dropout / GELU' / column sums
def _gelu_grad64(h):
    return 0.5 * (1 + torch.erf(h / math.sqrt(2))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2 * math.pi)


ROWS, RPG = 1100, 3                               # rows > 512: the grid's y dimension (512) wraps


@pytest.mark.parametrize("C", [776, 2056])
@pytest.mark.parametrize("mode", ["row_scale", "gelu", "colsum", "all"])
def test_scale_mask_rows_modes_against_fp64(C, mode):
    """out = row_scale[row / rpg] * GELU'(gelu_in) * x (, dropout), column sums added into `colsum`.  C = 2056 needs two column blocks.
    Breaks caught: row_scale indexed by row instead of row / rows_per_group, rows past 512 skipped (the y-grid wrap), GELU'(x) taken of the
    data instead of gelu_in, colsum overwritten instead of accumulated, the last column chunk of a partial column block dropped."""
    g = _gen(C)
    x = (torch.randn(ROWS, C + 8, generator=g)).to(bf16)            # strided input rows
    rs = torch.rand((ROWS + RPG - 1) // RPG, generator=g) + 0.5 if mode in ("row_scale", "all") else None
    hin = (torch.randn(ROWS, C, generator=g) * 2).to(bf16) if mode in ("gelu", "all") else None
    cs0 = torch.randn(C, generator=g) if mode in ("colsum", "all") else None
    p = 0.1 if mode == "all" else 0.0
    seed = 777
    xd = x.cuda()[:, :C]
    out = torch.empty(ROWS, C, dtype=bf16, device="cuda")
    cs = None if cs0 is None else cs0.cuda()
    K().scale_mask_rows(xd, ROWS, C, out=out, row_scale=None if rs is None else rs.cuda(), rows_per_group=RPG, dropout_p=p, seed=seed,
                        colsum=cs, gelu_in=None if hin is None else hin.cuda())
    torch.cuda.synchronize()
    x64 = x[:, :C].double()
    rsr = rs.double().repeat_interleave(RPG)[:ROWS, None] if rs is not None else torch.ones(ROWS, 1, dtype=torch.float64)
    gg = _gelu_grad64(hin.double()) if hin is not None else torch.ones(ROWS, C, dtype=torch.float64)
    keep = torch.ones(ROWS, C, dtype=torch.float64)
    if p > 0:
        from tests.helpers import hidden_keep_multiplier
        keep = hidden_keep_multiplier(seed, ROWS, C, p).double()
    t64 = x64 * rsr * gg * keep
    if mode == "row_scale":
        # x * rs * 1: one fp32 product, one bf16 rounding -- restated in fp32 they agree bit for bit
        ref = ((x[:, :C].float() * rs.repeat_interleave(RPG)[:ROWS, None]) * 1.0).to(bf16)
        assert torch.equal(_bits(out), _bits(ref))
    # GELU' through the fast erf (A&S 7.1.26, |error| <= 1.5e-7 on erf, so <= 7.5e-8 on the cdf) and exp2: <= ~2e-7 absolute on GELU';
    # then up to three fp32 roundings and one bf16 rounding
    pre = 4 * U * t64.abs() + (x64 * rsr * keep).abs() * (2e-7 if hin is not None else 0.0)
    ratio = _within(out.cpu(), t64, BF_HALF_ULP * (t64.abs() + pre) + pre + 1e-38, f"out ({mode})")
    print(f"scale_mask_rows {mode} C={C}: out within {ratio:.3f} of its bound")
    if cs0 is not None:
        # fp32 sums of the un-rounded t: each thread adds ceil(rows / 512) rows, then 512 atomics onto the pre-filled value
        chain = math.ceil(ROWS / 512) + 512 + 1
        ref_cs = cs0.double() + t64.sum(0)
        _within(cs.cpu(), ref_cs, chain * U * (t64.abs().sum(0) + cs0.double().abs()) + pre.sum(0), f"colsum ({mode})")


def test_scale_mask_rows_dropout():
    """Kept elements equal x * scale / (1 - p) (fp32, one bf16 rounding: bit for bit), the others are exactly 0, the kept fraction is within
    5 binomial standard deviations of 1 - p, the same seed gives the same mask and another seed a different one.  Break caught: the keep test
    inverted (kept fraction p), the 1 / (1 - p) missing, a mask that ignores the row (rows past 512 repeating rows below)."""
    C, p = 776, 0.3
    g = _gen(9)
    x = (torch.randn(ROWS, C, generator=g).sign() * (torch.rand(ROWS, C, generator=g) + 0.01)).to(bf16)      # no zeros
    rs = torch.rand((ROWS + RPG - 1) // RPG, generator=g) + 0.5
    outs = []
    for seed in (41, 41, 42):
        out = torch.empty(ROWS, C, dtype=bf16, device="cuda")
        K().scale_mask_rows(x.cuda(), ROWS, C, out=out, row_scale=rs.cuda(), rows_per_group=RPG, dropout_p=p, seed=seed)
        outs.append(out.cpu())
    torch.cuda.synchronize()
    o = outs[0]
    kept = o != 0
    inv = torch.tensor(1.0, dtype=torch.float32) / (1.0 - torch.tensor(p, dtype=torch.float32))
    ref = (((x.float() * rs.repeat_interleave(RPG)[:ROWS, None]) * 1.0) * inv).to(bf16)
    assert torch.equal(_bits(o)[kept], _bits(ref)[kept])
    N = ROWS * C
    frac = float(kept.sum()) / N
    sd = math.sqrt(p * (1 - p) / N)
    assert abs(frac - (1 - p)) <= 5 * sd, (frac, 1 - p, sd)
    assert torch.equal(_bits(outs[1]), _bits(o))
    assert not torch.equal(outs[2] != 0, kept)
    # rows 512 apart must not share a mask
    assert not torch.equal(kept[:512], kept[512:1024])
    from tests.helpers import hidden_keep_multiplier
    assert torch.equal(kept, hidden_keep_multiplier(41, ROWS, C, p) != 0)
