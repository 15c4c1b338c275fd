"""Float64 reference of lav_layernorm_fwd / lav_layernorm_bwd, per-element first-order error bounds derived from the kernels' arithmetic, and the
rounding model the per-row-block check compares against (test infrastructure; used by tests/test_gemm_layernorm_bounds_host.py on the CPU and by
tests/test_gpu_layernorm_bounds.py on the MI355X).

Rows x (R, C) are the values the kernel reads (bf16, fp16 or fp32 rows, after the patch-merge gather), as float64.

    mean = sum x / C ; var = sum (x - mean)^2 / C ; rstd = 1 / sqrt(var + eps) ; y = (x - mean) rstd gamma + beta
    xh = (x - mean) rstd ; gy = gamma dy ; m1 = mean(gy) ; m2 = mean(gy xh) ; dx = rstd (gy - m1 - xh m2) + add_in
    dgamma = sum_rows dy xh ; dbeta = sum_rows dy ; dx2 = keep (row_scale dx) ; colsum = sum_rows dx2

Error bound (first order; u = 2^-24, g(n) = n u / (1 - n u)):

  mean      B_m = g(C) mean|x| + u |mean|                 fp32 lane sums, the group butterfly, the division (layernorm.hip:54-66)
  var       two passes around the COMPUTED mean (layernorm.hip:67-74): sum (x - m^)^2 = C var + C (m - m^)^2, so
            B_var = B_m^2 + (g(C) + 3u) var + u var       (subtraction, square, fp32 sum of C terms; the division)
  rstd      rho = (B_var / (var + eps) + u) / 2 + RSQ_REL, relative     (eps added in fp32; rsqrtf = v_rsq_f32, within 2^-22 relative)
  y         |gamma| (B_m rstd + |x - m| rstd rho) + 3u |xh gamma| + u |y|, then the store: bf16 2^-8 (|y| + B), fp32 copy exact (:75-90)
  backward  the stored mean and rstd are inputs with the forward's B_m and rho (layernorm.hip:130-135):
            e_xh = B_m rstd + |xh| rho + 2u |xh| ; e_gy = u |gy|
            e_m1 = mean(e_gy) + g(C) mean|gy| ; e_m2 = mean(|gy| e_xh + |xh| e_gy) + (g(C) + u) mean|gy xh|
            e_dx = rstd (e_gy + e_m1 + |m2| e_xh + |xh| e_m2) + rho |dx - add_in| + 4u rstd (|gy| + |m1| + |xh m2|) + u |dx|   (:160-184)
            dx store bf16 2^-8 (|dx| + e_dx) ; dx2 = keep (row_scale dx) on the fp32 dx: keep |s| e_dx + 2u |dx2|, bf16 store (:186-197)
  columns   dgamma: sum_rows (|dy| e_xh + u |dy xh|) + g(R) sum_rows |dy xh| ; dbeta: g(R) sum_rows |dy| ;
            colsum: sum_rows e_dx2 + g(R) sum_rows |dx2|   (per-lane row sums, the LDS sum of a block, then atomics or the partial-tile
            reduction ln_bwd_finish_kernel / ln_bwd_finish_many_kernel: every column is one R-term fp32 sum, :201-263)
  dropout   the exact mask (tests.helpers.hidden_keep_multiplier with cols = C, as lav_keep indexes row * C + col, :191)

Per-row-block check: in every block of the kernel's rows-per-block (256 / G rows) the relative Frobenius error must stay within TILE_FACTOR of the
rounding model's (the reference with the kernel's bf16 stores injected) plus the block's bound norm over sqrt(C) plus the norm of the bound's
per-row part (the mean and rstd terms, which do not average over a row); column vectors are checked in blocks of 32 columns (one finish-kernel
block) with the floor over sqrt(R).  For mean, rstd and the fp32 copy y32 the per-row part is the whole bound and the model is the exact
value, so there the block check is no stricter than the per-element one: it guards y, dx, dx2 and the column sums only."""
import math

import torch

from tests.gemm_bounds import TILE_FACTOR, U32, U_BF, bfr, gam, tile_norms

RSQ_REL = 2.0 ** -22


def geometry(C, fwd=True):
    """pick_geom (layernorm.hip:321-330) at the default LAV_LN_G32 = 1: (G, iters, rows per block)"""
    G = 16 if C <= 128 else (32 if C <= 256 else 64)
    it = (C + G * 8 - 1) // (G * 8)
    if fwd and C == 768:
        G, it = 32, 3
    if fwd and C == 384:
        G, it = 16, 3
    inst = it if G != 64 or it <= 4 else 6
    return G, inst, 256 // G


def fwd(x, gamma, beta, eps, y32=False, one_pass=False, no_eps=False, drop_chunk=None):
    """reference, bounds and rounding model of lav_layernorm_fwd.  x (R, C) float64 of the rows read.  one_pass / no_eps / drop_chunk: kernel bugs
    the host test injects into the model (E[x^2] - mean^2 variance, eps left out, the last 8-column chunk of every row left unwritten)."""
    R, C = x.shape
    m = x.mean(1)
    d = x - m[:, None]
    var = d.pow(2).mean(1)
    rstd = (var + eps).rsqrt()
    xh = d * rstd[:, None]
    y = xh * gamma[None, :] + beta[None, :]
    b_m = gam(C) * x.abs().mean(1) + U32 * m.abs()
    b_var = b_m.pow(2) + (gam(C) + 4 * U32) * var
    rho = 0.5 * (b_var / (var + eps) + U32) + RSQ_REL
    b_y = gamma.abs()[None, :] * (b_m[:, None] * rstd[:, None] + d.abs() * rstd[:, None] * rho[:, None]) + 3 * U32 * (xh * gamma[None, :]).abs() + U32 * y.abs()
    s_y = gamma.abs()[None, :] * (b_m[:, None] * rstd[:, None] + d.abs() * rstd[:, None] * rho[:, None])
    r = dict(mean=m, rstd=rstd, y=y, b_mean=b_m, b_rstd=rho * rstd, rho=rho, b_y=b_y + U_BF * (y.abs() + b_y), s_y=s_y, xh=xh, var=var, C=C,
             s_mean=b_m, s_rstd=rho * rstd)
    if y32:
        r["y32"], r["b_y32"], r["s_y32"] = y, b_y, s_y
    # rounding model
    mm = m
    vv = var
    if one_pass:
        xf = x.float()
        vv = ((xf * xf).sum(1) / C - (xf.sum(1) / C) ** 2).double()
    ee = 0.0 if no_eps else eps
    rs = (vv + ee).clamp_min(1e-30).rsqrt()
    ym = (x - mm[:, None]) * rs[:, None] * gamma[None, :] + beta[None, :]
    if drop_chunk is not None:
        ym = ym.clone()
        ym[:, C - 8:] = drop_chunk
    r["m_y"], r["m_mean"], r["m_rstd"] = bfr(ym), mm, rs
    r["m_y32"] = ym
    return r


def bwd(f, x, dy, gamma, add_in=None, row_scale=None, keep=None, want_dx2=False, skip_rows=None):
    """reference, bounds and rounding model of lav_layernorm_bwd on the forward dict f (fwd()).  dy, add_in (R, C) as read; row_scale (R,) per row;
    keep (R, C) dropout multiplier.  skip_rows (host test only): rows whose contribution the model leaves out of dgamma (a lost block partial)."""
    R, C = x.shape
    rstd, xh = f["rstd"], f["xh"]
    b_m, rho = f["b_mean"], f["rho"]
    gy = gamma[None, :] * dy
    m1 = gy.mean(1)
    m2 = (gy * xh).mean(1)
    core = gy - m1[:, None] - xh * m2[:, None]
    dx = rstd[:, None] * core
    e_xh = b_m[:, None] * rstd[:, None] + xh.abs() * (rho[:, None] + 2 * U32)
    e_gy = U32 * gy.abs()
    e_m1 = e_gy.mean(1) + gam(C) * gy.abs().mean(1)
    e_m2 = (gy.abs() * e_xh + xh.abs() * e_gy).mean(1) + (gam(C) + U32) * (gy * xh).abs().mean(1)
    e_dx = (rstd[:, None] * (e_gy + e_m1[:, None] + m2.abs()[:, None] * e_xh + xh.abs() * e_m2[:, None]) + rho[:, None] * dx.abs()
            + 4 * U32 * rstd[:, None] * (gy.abs() + m1.abs()[:, None] + (xh * m2[:, None]).abs()))
    if add_in is not None:
        dx = dx + add_in
    e_dx = e_dx + U32 * dx.abs()
    s_dx = rstd[:, None] * (e_m1[:, None] + m2.abs()[:, None] * e_xh + xh.abs() * e_m2[:, None]) + rho[:, None] * (dx - (add_in if add_in is not None else 0)).abs()
    r = dict(dx=dx, e_dx=e_dx, b_dx=e_dx + U_BF * (dx.abs() + e_dx), m_dx=bfr(dx), s_dx=s_dx, R=R)          # e_dx: before the store (tests/embed_bounds.py)
    r["dgamma"] = (dy * xh).sum(0)
    r["b_dgamma"] = (dy.abs() * e_xh + U32 * (dy * xh).abs()).sum(0) + gam(R) * (dy * xh).abs().sum(0)
    r["dbeta"] = dy.sum(0)
    r["b_dbeta"] = gam(R) * dy.abs().sum(0)
    dgm = dy * xh
    if skip_rows is not None:
        dgm = dgm.clone()
        dgm[skip_rows] = 0
    r["m_dgamma"], r["m_dbeta"] = dgm.sum(0), r["dbeta"]
    if want_dx2 or keep is not None or row_scale is not None:
        s = row_scale[:, None] if row_scale is not None else torch.ones_like(dx[:, :1])
        kp = keep if keep is not None else torch.ones_like(dx)
        t = kp * s * dx
        e_t = kp * s.abs() * e_dx + 2 * U32 * t.abs()
        r.update(dx2=t, b_dx2=e_t + U_BF * (t.abs() + e_t), m_dx2=bfr(t), s_dx2=kp * s.abs() * s_dx, colsum=t.sum(0), b_colsum=e_t.sum(0) + gam(R) * t.abs().sum(0),
                 m_colsum=t.sum(0))
    return r


def check(name, got, ref, bound, model, block, floor_n, sys=None):
    """per-element |got - ref| <= bound; per block (rows of a (R, C) tensor, 32-column slices of a vector) ||got - ref|| <= TILE_FACTOR
    ||model - ref|| + ||bound|| / sqrt(floor_n) + ||sys||: sys is the part of the bound that is one value per row (the error of the mean and
    of rstd moves a whole row the same way, it does not average out over the row).  Returns (failures, max err/bound, max block ratio)."""
    got = got.double()
    err = (got - ref).abs()
    ok = (err <= bound) | ((got == ref) & torch.isfinite(ref))
    ratio = float((err / bound.clamp_min(1e-300)).masked_fill(got == ref, 0).max())
    fails = []
    if not bool(ok.all()):
        idx = torch.nonzero(~ok)[0].tolist()
        fails.append(f"{name}: {int((~ok).sum())} of {ok.numel()} elements outside the bound, worst err/bound {ratio:.3g}, first at {idx}")
    if got.dim() == 1:
        tl = (32, 1)
    else:
        tl = (block, got.shape[1])
    ek = tile_norms(got - ref, *tl)
    em = tile_norms(model - ref, *tl)
    fl = tile_norms(bound, *tl) / math.sqrt(max(floor_n, 1))
    if sys is not None:
        fl = fl + tile_norms(sys, *tl)
    lim = TILE_FACTOR * em + fl
    tr = float((ek / lim.clamp_min(1e-300)).max())
    if not bool((ek <= lim).all()):
        i = int((ek / lim.clamp_min(1e-300)).argmax())
        fails.append(f"{name}: block {i} error norm {float(ek.flatten()[i]):.3g} > {TILE_FACTOR} x model {float(em.flatten()[i]):.3g} + floor {float(fl.flatten()[i]):.3g}")
    return fails, ratio, tr


ROW_T = ("y", "y32", "mean", "rstd", "dx", "dx2")
COL_T = ("dgamma", "dbeta", "colsum")


def check_all(got, ref, block):
    fails, stats = [], {}
    C = ref.get("C", None)
    for t in ROW_T + COL_T:
        if t not in got or t not in ref:
            continue
        b = ref["b_" + t]
        m = ref.get("m_" + t, ref[t])
        sy = ref.get("s_" + t)
        if t in ("mean", "rstd"):
            g, rr, bb, mm, sy = got[t][:, None], ref[t][:, None], b[:, None], m[:, None], sy[:, None]
        else:
            g, rr, bb, mm = got[t], ref[t], b, m
        fn = ref.get("R", 1) if t in COL_T else (C or g.shape[-1])
        f, er, tr = check(t, g, rr, bb, mm, block, fn, sy)
        fails += f
        stats[t] = (er, tr)
    return fails, stats
