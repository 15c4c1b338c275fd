"""Float64 reference of lav_gemm_bf16 / lav_gemm_tn_grouped, a per-element first-order error bound derived from the kernels' arithmetic, the
rounding model the per-tile check compares against, and a host copy of the kernel selector (test infrastructure; used by
tests/test_gemm_layernorm_bounds_host.py on the CPU and by tests/test_gpu_gemm_bounds.py on the MI355X).

Every layout is reduced to one problem: a (M, K) and b (K, N), the bf16 operand values the kernel reads (layout 0: b = B^T, layout 2: a = A^T),
as float64; k_mask (K,) zeroes the contraction rows of dropped samples (TN drop-path, lav_gemm_epilogue.k_keep: a 0 / non-zero mask, the value
is not a multiplier -- tn_keep_mode, gemm.hip:663-670).  The epilogue runs in the kernel's order (gemm_epilogue, gemm.hip:159-395):

    z = a b ; v = alpha z + bias ; [preact] ; GELU | ReLU ; [* gelu_in] ; dropout ; row scale ; + residual ; [column sums] ; store

Error bound (first order; u = 2^-24 fp32 unit roundoff, g(n) = n u / (1 - n u) for an n-term fp32 sum, |a||b| the product of elementwise
absolute values).  Each term and where it comes from:

  accumulation     g(K + splits) (|a||b|)        fp32 MFMA accumulation over K (v_mfma_f32_16x16x32_bf16 / 32x32x16, gemm.hip:1-11), and the fp32
                                                   sum of the split partials: splitk_reduce_bf16_kernel (gemm.hip:1634-1649), tn_reduce_body
                                                   (gemm.hip:1595-1613) or the fp32 atomics of the ragged-N flush (gemm.hip:199)
  alpha, bias      u |alpha z| + u |v|           v = acc * alpha + bias, two fp32 roundings (gemm.hip:295)
  preact value     2^-8 |v|                       bf16 store of v (gemm.hip:296-300)
  GELU (erf)       1.13 E + |v| (ERF_ABS / 2 + 2u) + 3u |y|       gelu_f / fast_erf (common.h:83-93, 110): A&S 7.1.26, |erf error| <= 1.5e-7;
                                                   GELU's slope is at most 1.13; 1 + erf cancels for negative v (an absolute u on it)
  GELU + GELU'     1.13 E + |v| ERF3 / 2 + 3u |y|                 gelu_and_grad (common.h:96-109): the three-term A&S 7.1.25, |erf error| <= 2.5e-5
                   GELU' = Phi + v phi: 0.8 E + ERF3 / 2 + 4u     (|GELU''| <= 2 phi(0) < 0.8)
  GELU' store      bf16: 2^-8 |g'| ; one byte: half a step, 1 / (2 x 170.67) (gq_pack8, common.h:119-127)
  gelu_in          grad (bf16 or byte, read exactly): |h| E + u |v h| ; value: |g'(h)| E + |v| GG_ABS + u |v g'(h)|  (gelu_grad_f, common.h:111-114)
  ReLU             E (slope 1); the stored ReLU' is exact except where |v| <= E (either sign possible): bound 1 there
  dropout          keep E + 2u |v|                exact mask (lav_keep, common.h:141-147); 1 / (1 - p) and the product rounded (gemm.hip:336-340)
  row scale        |s| E + u |v|                  (gemm.hip:342-346)
  residual         E + E_res + u |v + r|          bf16 / fp16 / fp32 rows read exactly; res_ln: (r - mean) rstd gamma + beta in fp32 from the stored
                                                   statistics, E_res = 4u (|r - mean| rstd |gamma| + |beta|) (gemm.hip:366-371)
  column sums      sum_rows E + g(M) sum_rows |v|  over the fp32 v before the store (gemm.hip:377-380), thread, LDS and atomic sums (:391-410)
  store            bf16 E + 2^-8 (|v| + E) ; fp16 E + 2^-11 (|v| + E) + 2^-25 (subnormals), saturated at +-65504 (pack8_h, common.h:69-75) ;
                   fp32 E ; accumulate into C: E + u |C + v|, or E with assign (gemm.hip:186-199, 395-403)
  rowsum_a         g(K + splits) sum_k |a_km| + u |alpha s|     the row sums on the matrix cores against a ones fragment, alpha, atomics
                                                   across splits (gemm.hip:489, 578)

bf16 has 8 significant bits: one round-to-nearest store is within 2^-8 of the value, relative (2^-9 would be half of that).

Per-tile check: in every output tile of the route's own tile size (128 x 128, 256 x 128, 192 x 256 or 256 x 256) the relative Frobenius error of the
kernel must stay within TILE_FACTOR of the rounding model's (the reference with the kernel's store roundings injected), plus a floor of the
tile's bound norm divided by sqrt(K): the K accumulation roundings have random signs and add in quadrature, which the per-element bound adds in
magnitude.  A wrong or missing tile, a dropped k-tile or a shifted bias hides under a loose per-element bound but not under this check."""
import math

import torch

U32 = 2.0 ** -24
U_BF = 2.0 ** -8
U_H = 2.0 ** -11
H_SUB = 2.0 ** -25                 # half of the fp16 subnormal spacing 2^-24
H_MAX = 65504.0
ERF_ABS = 1.5e-7                   # fast_erf, A&S 7.1.26
ERF3_ABS = 2.5e-5                  # gelu_and_grad, A&S 7.1.25 (three terms)
GG_ABS = 0.5 * ERF_ABS + 8 * U32   # gelu_grad_f: erf term, plus exp2 / product roundings on x phi(x) <= 0.25
GELU_SLOPE = 1.13
GELU2_MAX = 0.8
GQ_SCALE = 170.66666666666666
GQ_OFF = 0.25
GQ_HALF = 0.5 / GQ_SCALE
TILE_FACTOR = 3.0


def gam(n):
    return n * U32 / (1.0 - n * U32)


def bfr(t):
    return t.float().bfloat16().double()


def h16r(t):
    return t.clamp(-H_MAX, H_MAX).float().half().double()


def gq_code(g):
    """the one-byte GELU' code and its decoded value (gq_pack8 / gq_unpack8): q = rne(g * 170.67 + 0.25 * 170.67), saturated to 0..255"""
    q = torch.round(g.float() * float(GQ_SCALE) + float(GQ_OFF * GQ_SCALE)).clamp(0, 255)
    return q.double() / GQ_SCALE - GQ_OFF


def erf_gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def gelu_grad(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def tanh_gelu(v):
    return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


# ------------------------------------------------------------------------------------------------------------------------------ reference
def case(a, b, *, alpha=1.0, bias=None, act=0, preact=None, gelu_in=None, gelu_in_mode="grad", keep=None, row_scale=None, residual=None,
         res_ln=None, colsum=False, out="bf16", c0=None, assign=False, splits=1, k_mask=None, rowsum=False, fns=None):
    """reference, bound and rounding model of one lav_gemm_bf16 call.  a (M, K), b (K, N) float64 of the bf16 operands; bias (N,), gelu_in (M, N)
    (the values the kernel reads: bf16, or the decoded byte code), keep (M, N) dropout multiplier (0 or 1 / (1 - p)), row_scale (M,) per output
    row, residual (M, N) as read, res_ln = (mean, rstd, gamma, beta) of the residual rows, c0 (M, N) the accumulate target before the call.
    preact: None | 'value' | 'grad' | 'byte'; out: 'bf16' | 'fp32' | 'fp16' | 'acc'.
    fns (host test only): replaces pieces of the arithmetic to express kernel bugs -- 'gelu' (the activation), 'z' (applied to the accumulated
    product), 'z32' (accumulate in fp32, as a kernel does), 'gq' (the GELU' byte code).
    Returns a dict: y / b_y / m_y, and when present pre, cs, rs with their b_ / m_ entries."""
    fns = fns or {}
    M, K = a.shape
    N = b.shape[1]
    am = a * k_mask[None, :] if k_mask is not None else a
    z = (am.float() @ b.float()).double() if fns.get("z32") else am @ b          # z32: the product accumulated in fp32 (host emulation)
    if "z" in fns:
        z = fns["z"](z)
    E = gam(K + (splits if splits > 1 else 0)) * (am.abs() @ b.abs())
    v = alpha * z
    E = abs(alpha) * E + U32 * v.abs()
    if bias is not None:
        v = v + bias[None, :]
        E = E + U32 * v.abs()
    r = {}
    if preact == "value":
        r["pre"], r["b_pre"], r["m_pre"] = v, E + U_BF * (v.abs() + E), bfr(v)
    if act == 1:
        gfn = fns.get("gelu", erf_gelu)
        y = gfn(v)
        if preact in ("grad", "byte"):
            gp = gelu_grad(v)
            eg = GELU2_MAX * E + 0.5 * ERF3_ABS + 4 * U32
            if preact == "grad":
                r["pre"], r["b_pre"], r["m_pre"] = gp, eg + U_BF * (gp.abs() + eg), bfr(gp)
            else:
                r["pre"], r["b_pre"], r["m_pre"] = gp, eg + GQ_HALF + U32 * 4, fns.get("gq", gq_code)(gp)
            E = GELU_SLOPE * E + 0.5 * ERF3_ABS * v.abs() + 3 * U32 * y.abs()
        else:
            E = GELU_SLOPE * E + v.abs() * (0.5 * ERF_ABS + 2 * U32) + 3 * U32 * y.abs()
        v = y
    elif act == 2:
        if preact in ("grad",):
            gp = (v > 0).double()                            # ReLU' is exact, except where |v| <= E: there the fp32 v may have either sign
            r["pre"], r["b_pre"], r["m_pre"] = gp, (v.abs() <= E).double(), gp
        v = v.clamp_min(0.0)
    if gelu_in is not None:
        if gelu_in_mode == "value":
            gg = gelu_grad(gelu_in)
            E = gg.abs() * E + v.abs() * GG_ABS
            v = v * gg
        else:
            E = gelu_in.abs() * E
            v = v * gelu_in
        E = E + (3 if gelu_in_mode == "byte" else 1) * U32 * v.abs()          # byte: the fp32 decode q / 170.67 - 0.25 (gq_unpack8)
    if keep is not None:
        v = v * keep
        E = keep * E + 2 * U32 * v.abs()
    if row_scale is not None:
        v = v * row_scale[:, None]
        E = row_scale.abs()[:, None] * E + U32 * v.abs()
    if residual is not None:
        h = residual
        if res_ln is not None:
            mu, rs, gma, bta = res_ln
            d = residual - mu[:, None]
            h = d * rs[:, None] * gma[None, :] + bta[None, :]
            E = E + 4 * U32 * (d.abs() * rs[:, None] * gma.abs()[None, :] + bta.abs()[None, :])
        v = v + h
        E = E + U32 * v.abs()
    if colsum:
        r["cs"] = v.sum(0)
        r["b_cs"] = E.sum(0) + gam(M) * v.abs().sum(0)
        r["m_cs"] = r["cs"]
    if out == "bf16":
        r["y"], r["b_y"], r["m_y"] = v, E + U_BF * (v.abs() + E), bfr(v)
    elif out == "fp16":
        y = v.clamp(-H_MAX, H_MAX)
        r["y"], r["b_y"], r["m_y"] = y, E + U_H * (y.abs() + E) + H_SUB, h16r(v)
    elif out == "fp32":
        r["y"], r["b_y"], r["m_y"] = v, E, v
    else:
        y = v if (assign or c0 is None) else c0 + v
        r["y"], r["b_y"], r["m_y"] = y, E + (0.0 if assign else U32 * y.abs()), y
    if rowsum:
        s = alpha * am.sum(1)
        r["rs"], r["b_rs"], r["m_rs"] = s, abs(alpha) * gam(K + splits) * am.abs().sum(1) + U32 * s.abs(), s
    r["K"] = K
    return r


# ------------------------------------------------------------------------------------------------------------------------------ checks
def tile_norms(x, tm, tn):
    """per-tile Frobenius norms of a (M, N) (or (M,)) tensor over tm x tn tiles (ragged last tiles included)"""
    if x.dim() == 1:
        x = x[:, None]
        tn = 1
    M, N = x.shape
    pm, pn = (-M) % tm, (-N) % tn
    x = torch.nn.functional.pad(x.pow(2), (0, pn, 0, pm))
    return x.reshape((M + pm) // tm, tm, (N + pn) // tn, tn).sum((1, 3)).sqrt()


def check(name, got, ref, bound, model, tile, K, rows=None):
    """per-element |got - ref| <= bound, and per tile ||got - ref|| <= TILE_FACTOR ||model - ref|| + ||bound|| / sqrt(K).
    rows (optional): the sampled rows got / ref / bound / model hold (then the tile check runs over row blocks of the sample).
    Returns (failure messages, max err/bound, max tile ratio)."""
    got = got.double()
    err = (got - ref).abs()
    ok = (err <= bound) | ((got == ref) & torch.isfinite(ref))
    ratio = float((err / bound.clamp_min(1e-300)).masked_fill(got == ref, 0).max())
    fails = []
    if not bool(ok.all()):
        idx = torch.nonzero(~ok)[0].tolist()
        fails.append(f"{name}: {int((~ok).sum())} of {ok.numel()} elements outside the bound, worst err/bound {ratio:.3g}, first at {idx}")
    tm, tn = tile
    if rows is not None:
        tm = max(1, min(tm, got.shape[0]))
    ek = tile_norms(got - ref, tm, tn)
    em = tile_norms(model - ref, tm, tn)
    fl = tile_norms(bound, tm, tn) / math.sqrt(max(K, 1))
    lim = TILE_FACTOR * em + fl
    tr = float((ek / lim.clamp_min(1e-300)).max())
    if not bool((ek <= lim).all()):
        i = int((ek / lim.clamp_min(1e-300)).argmax())
        fails.append(f"{name}: tile {divmod(i, ek.shape[1])} error norm {float(ek.flatten()[i]):.3g} > {TILE_FACTOR} x model "
                     f"{float(em.flatten()[i]):.3g} + floor {float(fl.flatten()[i]):.3g}")
    return fails, ratio, tr


def check_all(got, r, tile, rows=None):
    """got: dict with 'y' and any of 'pre', 'cs', 'rs'.  Returns (failures, {name: (max err/bound, max tile ratio)})"""
    fails, stats = [], {}
    for t in ("y", "pre", "cs", "rs"):
        if t not in got:
            continue
        tl = tile if t in ("y", "pre") else ((tile[1], 1) if t == "cs" else (tile[0], 1))
        kk = r["K"] if t != "cs" else got["y"].shape[0] * r["K"]
        f, er, tr = check(t, got[t], r[t], r["b_" + t], r["m_" + t], tl, kk, rows if t in ("y", "pre", "rs") else None)
        fails += f
        stats[t] = (er, tr)
    return fails, stats


# ------------------------------------------------------------------------------------------------------------------------------ selector
EF_BIAS, EF_ACT, EF_GIN, EF_DROP, EF_RSCALE, EF_RES, EF_COLSUM, EF_O32, EF_GENERIC, EF_ALL = 1, 2, 4, 8, 16, 32, 64, 128, 0x8000, 0xFFFF
S_B, S_BG, S_GC = EF_BIAS, EF_BIAS | EF_ACT, EF_GIN | EF_RSCALE | EF_COLSUM
S_BDR = EF_BIAS | EF_DROP | EF_RSCALE | EF_RES
S_BDRO = S_BDR | EF_O32
FSEL_NAME = {S_B: "S_B", S_BG: "S_BG", S_GC: "S_GC", S_BDR: "S_BDR", S_BDRO: "S_BDRO", EF_ALL: "EF_ALL"}


def feature_select(N, epi):
    """gemm.hip gemm_feature_index: the epilogue feature mask of a call and the instantiated superset it runs"""
    fm = 0
    if epi.get("bias"): fm |= EF_BIAS
    act, pre = epi.get("act", 0), epi.get("preact")
    if act == 1 and pre in (None, "grad", "byte"): fm |= EF_ACT
    elif act != 0 or pre is not None: fm |= EF_GENERIC
    if epi.get("gelu_in"): fm |= EF_GIN if epi.get("gelu_in") in ("grad", "byte") else EF_GENERIC
    if epi.get("drop"): fm |= EF_DROP
    if epi.get("rscale"): fm |= EF_RSCALE
    if epi.get("res"): fm |= EF_RES
    if epi.get("colsum"): fm |= EF_COLSUM
    out = epi.get("out", "bf16")
    if out in ("fp32", "fp16"): fm |= EF_O32
    if out == "acc" or N % 8: fm |= EF_GENERIC
    if not fm & ~S_B: return S_B
    if not fm & ~S_BG: return S_BG
    if not fm & ~S_GC: return S_GC
    if not fm & ~S_BDR: return S_BDR
    if (fm & EF_O32) and not fm & ~S_BDRO: return S_BDRO
    return EF_ALL


def _fill(tiles, slots, w):
    return w * tiles / (((tiles + slots - 1) // slots) * slots)


def route(layout, M, N, K, lda, ldb, epi=None, splits=1, ps=3, h192=1, h192l=1, pp_tn=True, tn_min_m=160):
    """host copy of lav_gemm_bf16's kernel choice (gemm.hip gemm_plan / gemm_plan_part) at the default switches (lav_gemm_select overrides:
    ps = 11, h192 = 7, h192l = 9, pp_tn = 2, tn_min_m = 12).  Returns a list of launches [(kernel name, (tile rows, tile cols))] in order.
    tests/test_gemm_layernorm_bounds_host.py holds it to the library's own plan (lav_gemm_plan) over a sweep of calls."""
    epi = epi or {}
    out = epi.get("out", "bf16")
    kps = ((K + splits - 1) // splits + 63) // 64 * 64
    splits = (K + kps - 1) // kps
    nb_rows = 0
    if (epi.get("c_pad") and N % 8 and layout == 0 and splits == 1 and K % 64 == 0 and M >= 2048 and out == "bf16"
            and not epi.get("colsum") and not epi.get("preact") and not epi.get("gelu_in") and not epi.get("res") and not epi.get("a_rowmap")):
        nb_rows, N = N, (N + 7) // 8 * 8
    big = layout != 2 and splits == 1 and K % 64 == 0 and M >= 2048
    fsel = feature_select(N, epi)
    t_small = -(-M // 128) * -(-N // 128)
    t_big = -(-M // 256) * -(-N // 128)
    t_huge = -(-M // 256) * (N // 256)
    f_small, f_big = _fill(t_small, 512, 0.80), _fill(t_big, 256, 0.80)
    f_huge = _fill(t_huge, 256, 1.0) if N % 256 == 0 and not nb_rows and t_huge else 0.0
    t_h192 = -(-M // 192) * (N // 256)
    f_h192 = _fill(t_h192, 256, 0.97) if N % 256 == 0 and fsel != EF_ALL and h192 and not nb_rows and t_h192 else 0.0
    small32 = M * lda * 2 < 2 ** 31 and N * ldb * 2 < 2 ** 31
    if epi.get("a_rowmap"):
        if (ps & 1) and fsel != EF_ALL and small32:
            return [("gemm_ps_kernel", (256, 256))]
        return [("gemm_huge_kernel", (256, 256))]
    if big and f_h192 > f_huge + 0.02 and f_h192 >= f_big and f_h192 >= f_small:
        if (ps & 2) and layout == 0 and small32:
            return [("gemm_ps_kernel", (192, 256))]
        if layout == 0 and h192l:
            return [("gemm_h192l_kernel", (192, 256))]
        return [("gemm_h192_kernel", (192, 256))]
    if big and f_huge >= f_big and f_huge >= f_small:
        if (ps & 1) and layout == 0 and fsel != EF_ALL and small32:
            return [("gemm_ps_kernel", (256, 256))]
        return [("gemm_huge_kernel", (256, 256))]
    if big and (f_big >= f_small or nb_rows):
        return [("gemm_big_kernel", (256, 128))]
    if layout != 2:
        sk = splits > 1 and out == "bf16"
        sk_huge = sk and K % 64 == 0 and kps % 64 == 0 and M >= 256 and N % 256 == 0
        r = [("gemm_huge_kernel", (256, 256))] if sk_huge else [("gemm_kernel", (128, 128))]
        if sk:
            r.append(("splitk_reduce_bf16_kernel", (256, 256) if sk_huge else (128, 128)))
        return r
    plain = out == "acc" and not any(epi.get(f) for f in ("bias", "act", "preact", "gelu_in", "drop", "rscale", "res", "colsum"))
    keep_rpg = epi.get("k_keep_rpg")
    mm = tn_min_m if N >= 512 else max(tn_min_m, 256)
    if plain and not keep_rpg and M >= mm and K >= 2048 and K % 32 and K % 64:
        K0 = K // 64 * 64
        return (route(2, M, N, K0, lda, ldb, epi, splits, ps, h192, h192l, pp_tn, tn_min_m)
                + route(2, M, N, K - K0, lda, ldb, dict(epi, assign=False), 1, ps, h192, h192l, pp_tn, tn_min_m))
    kind = 0
    large_ok = plain and K % 64 == 0 and kps % 64 == 0 and M >= mm and (not keep_rpg or keep_rpg >= 64)
    if large_ok:
        kind = 2 if N % 256 == 0 else 1
    pp_only = (not large_ok and plain and K % 32 == 0 and K % 64 and M >= mm and N % 256 == 0 and pp_tn
               and (not keep_rpg or (keep_rpg >= 64 and -(-K // keep_rpg) <= 128)))
    if pp_only:
        kind = 2
    rpt = 256 if kind else 128
    reduce = out == "acc" and splits > 1 and N % 4 == 0
    if kind == 2 and pp_tn and K % 32 == 0 and kps % 32 == 0 and (not keep_rpg or (keep_rpg >= 32 and -(-K // keep_rpg) <= 128)):
        r = [("gemm_pp_kernel", (256, 256))]
    elif kind == 2:
        r = [("gemm_huge_kernel", (256, 256))]
    elif kind == 1:
        r = [("gemm_big_kernel", (256, 128))]
    else:
        r = [("gemm_kernel", (128, 128))]
    if reduce:
        r.append(("tn_reduce_kernel", (rpt, 128)))
    return r


def grouped_route(jobs, splits, tn_min_m=160, pp_tn=True):
    """lav_gemm_tn_grouped (gemm.hip tn_group_fits / tn_group_plan): one ping-pong launch when every job fits it, else the jobs one by one"""
    ok = bool(pp_tn)
    for q in jobs:
        mm = tn_min_m if q["N"] >= 512 else max(tn_min_m, 256)
        ok = ok and q["M"] >= mm and q["N"] % 256 == 0 and q["K"] >= 32 and q["K"] % 32 == 0 and (
            not q.get("k_keep_rpg") or (q["k_keep_rpg"] >= 64 and -(-q["K"] // q["k_keep_rpg"]) <= 128))
    if not ok:
        r = []
        for q in jobs:
            r += route(2, q["M"], q["N"], q["K"], q["M"], q["N"], dict(out="acc", k_keep_rpg=q.get("k_keep_rpg")), q.get("fallback_splits", 1),
                       pp_tn=pp_tn, tn_min_m=tn_min_m)
        return r
    r = [("gemm_pp_group_kernel", (256, 256))]
    sp = []
    for q in jobs:
        s = min(splits, q["K"] // 256) if q["K"] // 256 > 0 else 1
        s = max(s, 1)
        kps = ((q["K"] + s - 1) // s + 63) // 64 * 64
        sp.append((q["K"] + kps - 1) // kps)
    if any(s > 1 for s in sp):
        r.append(("tn_reduce_group_kernel", (256, 128)))
    return r


# ---- the split-K policy as lavender_amd/hip.py held it before it moved into the library (gemm.hip: tn_splits, nn_splits, tn_group_splits): the
# bodies verbatim, the module constants they read as parameters.  tests/test_gemm_layernorm_bounds_host.py holds the library's answers to these.
def splits_for(M, N, K, keep=False, tn_min_m=160, tn_blocks=128):
    _TN_MINM, _TN_BLOCKS = tn_min_m, tn_blocks
    if M >= (_TN_MINM if N >= 512 else max(_TN_MINM, 256)) and (K % 64 == 0 or (K % 32 == 0 and N % 256 == 0) or (K >= 2048 and not keep)):   # ragged long K: lav_gemm_bf16 splits off the < 64-row tail
        tiles = ((M + 255) // 256) * (N // 256 if N % 256 == 0 else (N + 127) // 128)
        return int(max(1, min(_TN_BLOCKS // tiles if tiles <= _TN_BLOCKS else 1, K // 256)))
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles >= 200:
        return 1
    s = 5 if tiles > 128 else max(1, 256 // tiles)
    return int(max(1, min(s, 256, (K + 255) // 256)))


def group_splits_for(shapes, K, tn_min_m=160, tn_group=True, tn_group_blocks=192, tn_group_blocks_wide=192):
    _TN_MINM, _TN_GROUP, _TN_GROUP_BLOCKS, _TN_GROUP_BLOCKS_WIDE = tn_min_m, tn_group, tn_group_blocks, tn_group_blocks_wide
    if not _TN_GROUP or K % 32:
        return 0
    tiles = 0
    for M, N in shapes:
        if N % 256 or M < (_TN_MINM if N >= 512 else max(_TN_MINM, 256)):
            return 0
        tiles += ((M + 255) // 256) * (N // 256)
    return int(max(1, min(round((_TN_GROUP_BLOCKS_WIDE if tiles >= 96 else _TN_GROUP_BLOCKS) / tiles), K // 256)))


def splits_nn(M, N, K):
    if K < 4096 or N % 8:
        return 1
    if M >= 256 and N % 256 == 0 and K % 64 == 0:
        tiles = ((M + 255) // 256) * (N // 256)
        return int(max(1, min(256 // tiles, K // 1024))) if tiles < 128 else 1
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles >= 256:
        return 1
    return int(max(1, min(512 // tiles, K // 1024)))


def tn_need(M, N, splits):
    """upper bound of the split-K workspace bytes of one weight-gradient / split-K GEMM (256 x 256 fp32 partial tiles per split)"""
    return 0 if splits <= 1 else int(splits) * ((M + 255) // 256) * ((N + 255) // 256) * 262144
