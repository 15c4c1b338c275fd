"""Float64 references of the embedding and gather kernels (lavender_amd/csrc/embed.hip, embed_rows_kernel of lavender_amd/csrc/decode.hip), per-element
first-order error bounds derived from the kernels' arithmetic, and the rounding models the per-block check compares against (test infrastructure;
used by tests/test_embed_bounds_host.py on the CPU and by tests/test_gpu_embed_bounds.py on the MI355X).

Both embeddings are a LayerNorm with C = Hd over rows the kernel builds itself in fp32, so the bound is the LayerNorm bound of
tests/layernorm_bounds.py (LB.fwd / LB.bwd are called, not copied) on the exact rows x, plus the terms below (u = 2^-24, g(n) = n u / (1 - n u)).

  text rows    x = (word[id] + pos[x]) + type0, two fp32 additions (embed.hip:240, :379; decode.hip:319): e_x = u (|word + pos| + |x|)
  video rows   forward x = ((cls | feat) + pos[p]) + len[t] (embed.hip:59-62), feat bf16 read exactly: e_x = u (|x0 + pos| + |x|);
               backward x = feat + ((pos[p] + cls) + len[t]) (embed.hip:110, :132), another association:
               e_xb = u (|pos + cls| [p = 0] + |pos + cls + len| + |x| [p > 0])
  input error  the rows read are x + dx, |dx| <= e_x.  First order, with d = x - mean:
               mean      + mean(e_x)                                              =: e_m
               var       + 2 mean(|d| (e_x + e_m)) + mean((e_x + e_m)^2)          -> rho_x = that / (2 (var + eps)), relative on rstd
               y         + |gamma| rstd (e_x + e_m + |d| rho_x)                   before the store
               xh (bwd)  the backward recomputes x (e_xb) and reads the forward's mean and rstd: LB.bwd runs with
                         b_mean + e_m + max_row(e_xb) as the row's mean error (the largest e_xb of a row stands for each of its elements) and rho + rho_x
  row sums     lane sums (8 or 16 values), the wave butterfly (common.h wave_sum) and, in embed_rows_kernel, the four wave partials through LDS
               (decode.hip:322-335): one Hd-term fp32 sum, g(Hd) as in LB.fwd
  dropout      exact mask lav_keep(seed, row * Hd + col) (embed.hip:263, :378) = tests.helpers.hidden_keep_multiplier(seed, n X, Hd, p) > 0;
               inv = 1 / (1 - p) is two fp32 roundings (1 - p, the division; :254, :358) and the product a third: 3u |keep v|, against a reference
               multiplier 1 / (1 - fp32(p)) in float64 (two roundings more than the single product rounding one would count with inv taken as exact).  Forward: after
               the affine, E -> keep E + 3u |y|; backward: on dout before anything else, e_dy = 3u |dy|, which enters
               e_dx + rstd (|gamma| e_dy + mean(|gamma| e_dy) + |xh| mean(|xh gamma| e_dy)), dgamma + sum |xh| e_dy, dbeta + sum e_dy
  stores       y, dfeat, gather_sum: bf16, E + 2^-8 (|v| + E); mean, rstd, every gradient table: fp32
  fp32 sums    d_word[v] (atomics per row, embed.hip:397), d_pos, d_type0 / d_len / d_cls, dgamma, dbeta (register sums per wave, four waves through LDS,
               one atomic per block, embed.hip:402-423, :151-179), all onto the buffer's initial value.  Atomics make the order free:
               sum_rows e + g(rows) (|initial| + sum_rows |v|), rows = the rows summed into the element: count_v for d_word[v], n for the text d_pos[x],
               n X for d_type0, B T for the video d_pos[p] and d_cls, B (1 + hw) for d_len[t], all rows for dgamma and dbeta.  Wave partials and block
               atomics are inner nodes of one summation tree whose leaves are the rows and the initial value (rows + 1 leaves, rows inexact
               additions); an addition onto a zero register or of an idle wave's zero partial is exact.
               A table row no input row maps to has bound 0: it must come back bit-identical (d_type0 row 1, unused vocabulary and position rows).
  text groups  lav_text_embed_bwd launches X x groups blocks, groups = 8 at n >= 32, 2 at n >= 8, else 1 (embed.hip:459); the grouping changes the
               order of the sums only, not their bound (text_groups() serves the host emulation)
  gather_sum   acc += v over the k rows of a segment in list order in fp32, then a bf16 store (embed.hip:514-522):
               E = g(k) sum |v| ; bound E + 2^-8 (|s| + E); an empty segment is exact zeros
  im2col, gather_rows   data movement with one round-to-nearest-even conversion (pack8) or none: the reference is the rearranged input's .bfloat16()
               (im2col) or the copied bits (gather_rows), compared with torch.equal; no bound.

Per-block check (LB.check): the relative Frobenius error of a block must stay within TILE_FACTOR of the rounding model's plus the block's bound norm
over sqrt(floor) plus the norm of the bound's per-row part.  y, mean, rstd, dfeat: blocks of the 4 rows of one thread block (1 row for
embed_rows_kernel), floor Hd; dgamma, dbeta, d_cls: blocks of 32 columns, floor = rows summed; the tables d_word / d_pos / d_len / d_type0: one table
row per block, floor 1 for d_word (a row may hold a single term), the rows summed for the others; gather_sum: one row, floor C."""
import torch

from tests import layernorm_bounds as LB
from tests.gemm_bounds import U32 as u, U_BF, bfr, gam as g          # TILE_FACTOR and tile_norms act through LB.check, RSQ_REL through LB.fwd


def text_groups(n):
    """lav_text_embed_bwd (embed.hip:459)"""
    return 8 if n >= 32 else (2 if n >= 8 else 1)


def keep_multiplier(seed, rows, cols, p):
    """the exact dropout multiplier: 0 or 1 / (1 - p) at the fp32 value of p, on the mask of tests.helpers.hidden_keep_multiplier"""
    import numpy as np
    from tests.helpers import hidden_keep_multiplier
    return (hidden_keep_multiplier(seed, rows, cols, p) > 0).double() / (1.0 - float(np.float32(p)))


def _ln_rows(x, e_x, e_xb, gamma, beta, eps, keep):
    """LayerNorm forward of built rows: LB.fwd on the exact rows plus the input-error terms"""
    f = LB.fwd(x, gamma, beta, eps, y32=True)
    C = x.shape[1]
    rstd, var = f["rstd"], f["var"]
    d = x - f["mean"][:, None]
    e_m = e_x.mean(1)
    e_d = e_x + e_m[:, None]
    rho_x = 0.5 * (2 * (d.abs() * e_d).mean(1) + e_d.pow(2).mean(1)) / (var + eps)
    ex_y = gamma.abs()[None, :] * rstd[:, None] * (e_d + d.abs() * rho_x[:, None])
    y, E, s = f["y"], f["b_y32"] + ex_y, f["s_y32"] + ex_y
    ym = f["m_y32"]
    if keep is not None:
        y, ym = keep * y, keep * ym
        E, s = keep * E + 3 * u * y.abs(), keep * s
    r = dict(y=y, b_y=E + U_BF * (y.abs() + E), s_y=s, m_y=bfr(ym), mean=f["mean"], b_mean=f["b_mean"] + e_m, s_mean=f["b_mean"] + e_m,
             m_mean=f["m_mean"], rstd=rstd, b_rstd=(f["rho"] + rho_x) * rstd, s_rstd=(f["rho"] + rho_x) * rstd, m_rstd=f["m_rstd"], C=C, x=x)
    # what LB.bwd reads: the stored statistics' errors and the recomputed rows' error
    r["f_bwd"] = dict(f, b_mean=f["b_mean"] + e_m + e_xb.max(1).values, rho=f["rho"] + rho_x)
    return r


def _ln_rows_bwd(fr, dy, gamma, e_dy):
    """LB.bwd on the forward dict.  Returns dx, e_dx (before any store), s_dx and, for dgamma and dbeta, (sum over the rows, summed error of the
    terms, summed magnitude): LB.bwd's own column bounds less its g(R) term, which the caller replaces by g(terms)"""
    f, x = fr["f_bwd"], fr["x"]
    b = LB.bwd(f, x, dy, gamma)
    dx, R = b["dx"], x.shape[0]
    e_dx = b["e_dx"]                                             # before the bf16 store that b_dx includes
    rstd, xh = f["rstd"], f["xh"]
    mag_g, mag_b = (dy * xh).abs().sum(0), dy.abs().sum(0)
    e_g, e_b = b["b_dgamma"] - g(R) * mag_g, b["b_dbeta"] - g(R) * mag_b
    if e_dy is not None:
        e_gy = gamma.abs()[None, :] * e_dy
        e_dx = e_dx + rstd[:, None] * (e_gy + e_gy.mean(1)[:, None] + xh.abs() * (xh.abs() * e_gy).mean(1)[:, None])
        e_g = e_g + (xh.abs() * e_dy).sum(0)
        e_b = e_b + e_dy.sum(0)
    return dx, e_dx, b["s_dx"], (b["dgamma"], e_g, mag_g), (b["dbeta"], e_b.clamp_min(0), mag_b)


def _col(c, init, terms):
    val, err, mag = c
    return init + val, err + g(terms) * (init.abs() + mag)


def _table(rows, e_rows, index, n_table, init):
    """fp32 sums of rows into a table: table[index[r]] += rows[r] onto init, g(rows summed into the table row).  Returns (values, bound)"""
    val = torch.zeros(n_table, rows.shape[1], dtype=torch.float64).index_add_(0, index, rows)
    mag = torch.zeros_like(val).index_add_(0, index, rows.abs())
    err = torch.zeros_like(val).index_add_(0, index, e_rows)
    cnt = torch.zeros(n_table, dtype=torch.float64).index_add_(0, index, torch.ones(len(index), dtype=torch.float64))
    return init + val, err + g(cnt)[:, None] * (init.abs() + mag)


def _vec(rows, e_rows, init, sel=None):
    if sel is not None:
        rows, e_rows = rows[sel], e_rows[sel]
    return init + rows.sum(0), e_rows.sum(0) + g(rows.shape[0]) * (init.abs() + rows.abs().sum(0))


# ------------------------------------------------------------------------------------------------------------------------------ text embedding
def text_fwd(ids, word, pos, type0, gamma, beta, eps, keep=None, pos_ids=None):
    """lav_text_embed_fwd (pos_ids None: row (j, x) reads pos[x]) / lav_text_embed_rows_fwd (ids (n,), explicit pos_ids).  Tables float64;
    keep (rows, Hd): keep_multiplier().  Returns y / mean / rstd with b_, s_ (per-row part) and m_ (rounding model) entries."""
    if pos_ids is None:
        n, X = ids.shape
        pos_ids = torch.arange(X).repeat(n)
    idf = ids.reshape(-1)
    wp = word[idf] + pos[pos_ids]
    x = wp + type0[None, :]
    e_x = u * (wp.abs() + x.abs())
    r = _ln_rows(x, e_x, e_x, gamma, beta, eps, keep)
    r["spec"] = dict(y=(4, r["C"]), mean=(4, r["C"]), rstd=(4, r["C"])) if ids.dim() == 2 else dict(y=(1, r["C"]))
    return r


def rows_fwd(ids, pos_ids, word, pos, type0, gamma, beta, eps):
    return text_fwd(ids, word, pos, type0, gamma, beta, eps, pos_ids=pos_ids)


def text_bwd(fr, ids, dout, gamma, init, keep=None):
    """lav_text_embed_bwd on text_fwd's dict.  dout (n X, Hd) as read; init: dict of the buffers before the call (d_word (V, Hd), d_pos (Pt, Hd),
    d_type0 (2, Hd), dgamma, dbeta), float64.  Every output is initial + gradient."""
    n, X = ids.shape
    R, C = n * X, dout.shape[1]
    dy, e_dy = dout, None
    if keep is not None:
        dy = keep * dout
        e_dy = 3 * u * dy.abs()
    dx, e_dx, _, cg, cb = _ln_rows_bwd(fr, dy, gamma, e_dy)
    idf = ids.reshape(-1)
    r = {}
    r["d_word"], r["b_d_word"] = _table(dx, e_dx, idf, init["d_word"].shape[0], init["d_word"])
    r["d_pos"], r["b_d_pos"] = _table(dx, e_dx, torch.arange(X).repeat(n), init["d_pos"].shape[0], init["d_pos"])
    t0, b0 = _vec(dx, e_dx, init["d_type0"][0])
    r["d_type0"] = torch.stack([t0, init["d_type0"][1]])
    r["b_d_type0"] = torch.stack([b0, torch.zeros_like(b0)])
    r["dgamma"], r["b_dgamma"] = _col(cg, init["dgamma"], R)
    r["dbeta"], r["b_dbeta"] = _col(cb, init["dbeta"], R)
    r["spec"] = dict(d_word=(1, 1), d_pos=(1, n), d_type0=(1, R), dgamma=(4, R), dbeta=(4, R))
    return r


# ------------------------------------------------------------------------------------------------------------------------------ video token assembly
def video_rows(B, T, hw):
    """(b, t, p) of every row r = (b T + t) (1 + hw) + p, the order of mean / rstd and of the kernel's row index"""
    P = 1 + hw
    r = torch.arange(B * T * P)
    return r // P // T, r // P % T, r % P


def video_fwd(feat, B, T, hw, cls, pos, len_, gamma, beta, eps):
    """lav_video_embed_fwd.  feat (B T hw, Hd) bf16 values, cls (Hd,), pos (>= 1 + hw, Hd), len_ (>= T, Hd), float64.  Rows in video_rows order."""
    b, t, p = video_rows(B, T, hw)
    is_cls = (p == 0)[:, None]
    fidx = ((b * T + t) * hw + (p - 1).clamp_min(0))
    x0 = torch.where(is_cls, cls[None, :], feat[fidx])
    xp = x0 + pos[p]
    x = xp + len_[t]
    e_x = u * (xp.abs() + x.abs())
    pc = pos[p] + torch.where(is_cls, cls[None, :], torch.zeros_like(x))
    e_xb = u * (torch.where(is_cls, pc.abs(), torch.zeros_like(x)) + (pc + len_[t]).abs() + torch.where(is_cls, torch.zeros_like(x), x.abs()))
    r = _ln_rows(x, e_x, e_xb, gamma, beta, eps, None)
    r["spec"] = dict(y=(4, r["C"]), mean=(4, r["C"]), rstd=(4, r["C"]))
    r["geom"] = (B, T, hw)
    return r


def video_bwd(fr, dout, gamma, init):
    """lav_video_embed_bwd on video_fwd's dict.  dout (rows, Hd) in video_rows order; init: d_cls (Hd,), d_pos (Pt, Hd), d_len (Tt, Hd), dgamma, dbeta.
    dfeat (B T hw, Hd): the bf16 store of dx of the rows p > 0."""
    B, T, hw = fr["geom"]
    P = 1 + hw
    b, t, p = video_rows(B, T, hw)
    R = len(p)
    dx, e_dx, s_dx, cg, cb = _ln_rows_bwd(fr, dout, gamma, None)
    tok = p > 0
    r = dict(dfeat=dx[tok], b_dfeat=e_dx[tok] + U_BF * (dx[tok].abs() + e_dx[tok]), s_dfeat=s_dx[tok], m_dfeat=bfr(dx[tok]))
    r["d_pos"], r["b_d_pos"] = _table(dx, e_dx, p, init["d_pos"].shape[0], init["d_pos"])
    r["d_len"], r["b_d_len"] = _table(dx, e_dx, t, init["d_len"].shape[0], init["d_len"])
    r["d_cls"], r["b_d_cls"] = _vec(dx, e_dx, init["d_cls"], sel=~tok)
    r["dgamma"], r["b_dgamma"] = _col(cg, init["dgamma"], R)
    r["dbeta"], r["b_dbeta"] = _col(cb, init["dbeta"], R)
    r["spec"] = dict(dfeat=(4, fr["C"]), d_pos=(1, B * T), d_len=(1, B * P), d_cls=(4, B * T), dgamma=(4, R), dbeta=(4, R))
    return r


# ------------------------------------------------------------------------------------------------------------------------------ gathers
def gather_sum(src, start, lst):
    """lav_gather_sum_rows: out[r] = sum of src[lst[k]] for k in [start[r], start[r + 1]).  src (rows, C) float64 of the bf16 values"""
    n_out, C = len(start) - 1, src.shape[1]
    seg = torch.repeat_interleave(torch.arange(n_out), torch.as_tensor(start[1:]) - torch.as_tensor(start[:-1]))
    rows = src[torch.as_tensor(lst, dtype=torch.long)]
    k = (torch.as_tensor(start[1:]) - torch.as_tensor(start[:-1])).double()
    s = torch.zeros(n_out, C, dtype=torch.float64).index_add_(0, seg, rows)
    mag = torch.zeros(n_out, C, dtype=torch.float64).index_add_(0, seg, rows.abs())
    E = g(k)[:, None] * mag
    return dict(out=s, b_out=E + U_BF * (s.abs() + E), m_out=bfr(s), spec=dict(out=(1, C)))


def gather_rows_ref(src, idx):
    """lav_gather_rows: the copied bits; a negative index gives a row of zeros.  src (rows, C) bf16, any device"""
    out = src[idx.long().clamp_min(0)].clone()
    out[idx < 0] = 0
    return out


def im2col_ref(img, B, T, H, W, frame_major):
    """lav_patch_im2col: PatchEmbed3D's (2, 4, 4) patches of clips padded with one zero frame at the end, row (b, t, ph, pw), column
    c 32 + kt 16 + kh 4 + kw (the Conv3d weight's (c, kt, kh, kw) order), rounded to bf16.  img: fp32 (B, T, 3, H, W) when frame_major,
    else (B, 3, T, H, W); any device."""
    x = img.bfloat16().view(B, T, 3, H, W).transpose(1, 2) if frame_major else img.bfloat16().view(B, 3, T, H, W)
    nxt = torch.cat([x[:, :, 1:], torch.zeros_like(x[:, :, :1])], 2)
    x = torch.stack([x, nxt], 3)                                  # (B, 3, T, kt, H, W)
    x = x.view(B, 3, T, 2, H // 4, 4, W // 4, 4).permute(0, 2, 4, 6, 1, 3, 5, 7)
    return x.reshape(B * T * (H // 4) * (W // 4), 96)


# ------------------------------------------------------------------------------------------------------------------------------ checks
def check_all(got, ref, block=None):
    """every output ref["spec"] names: the per-element bound and LB.check's per-block check (block rows, floor) against the rounding model.
    An output the spec names and got lacks is a failure.  Returns (failures, {name: (max err/bound, max block ratio)})"""
    fails, stats = [], {}
    for t, (blk, fn) in ref["spec"].items():
        if t not in got:
            fails.append(f"{t}: not among the outputs checked")
            continue
        gt, rr, bb, mm, sy = got[t], ref[t], ref["b_" + t], ref.get("m_" + t, ref[t]), ref.get("s_" + t)
        if tuple(gt.shape) != tuple(rr.shape):
            fails.append(f"{t}: shape {tuple(gt.shape)}, reference {tuple(rr.shape)}")
            continue
        if t in ("mean", "rstd"):
            gt, rr, bb, mm, sy = gt[:, None], rr[:, None], bb[:, None], mm[:, None], sy[:, None]
        f, er, tr = LB.check(t, gt, rr, bb, mm, block or blk, fn, sy)
        fails += f
        stats[t] = (er, tr)
    return fails, stats


# ------------------------------------------------------------------------------------------------------------------------------ case inputs
def _rn(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def text_inputs(n, X, Hd, V=40, seed=0, offset=0.0):
    """host tensors of one text-embedding case: every text starts with id 1, text j ends in j % X zeros (padding), the rest is drawn from
    2 .. V - 9, so ids collide heavily and the last 8 vocabulary rows are never hit; the position table has X + 3 rows, the type table 2; the
    gradient buffers start non-zero.  offset: a common offset on the word table (rows with mean >> spread)."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * n + X + Hd)
    ids = torch.randint(2, V - 8, (n, X), generator=gen)
    ids[:, 0] = 1
    for j in range(n):
        k = j % X
        if k:
            ids[j, X - k:] = 0
    d = dict(ids=ids, word=_rn(gen, V, Hd, scale=0.5) + offset, pos=_rn(gen, X + 3, Hd, scale=0.5), type=_rn(gen, 2, Hd, scale=0.5),
             gamma=1 + 0.1 * _rn(gen, Hd), beta=0.1 * _rn(gen, Hd), dout=_rn(gen, n * X, Hd).bfloat16())
    d["init"] = dict(d_word=_rn(gen, V, Hd, scale=0.1), d_pos=_rn(gen, X + 3, Hd, scale=0.1), d_type0=_rn(gen, 2, Hd, scale=0.1),
                     dgamma=_rn(gen, Hd, scale=0.1), dbeta=_rn(gen, Hd, scale=0.1))
    return d


def video_inputs(B, T, hw, Hd, seed=0, len_rows=None):
    """host tensors of one video-assembly case: the pos table has 3 + hw rows, the len table T + 2 (or len_rows); non-zero gradient buffers"""
    gen = torch.Generator().manual_seed(1000 * seed + 31 * B + 7 * T + hw + Hd)
    R = B * T * (1 + hw)
    d = dict(feat=_rn(gen, B * T * hw, Hd).bfloat16(), cls=_rn(gen, Hd, scale=0.5), pos=_rn(gen, 3 + hw, Hd, scale=0.5),
             len=_rn(gen, len_rows or T + 2, Hd, scale=0.5), gamma=1 + 0.1 * _rn(gen, Hd), beta=0.1 * _rn(gen, Hd), dout=_rn(gen, R, Hd).bfloat16())
    d["init"] = dict(d_cls=_rn(gen, Hd, scale=0.1), d_pos=_rn(gen, 3 + hw, Hd, scale=0.1), d_len=_rn(gen, d["len"].shape[0], Hd, scale=0.1),
                     dgamma=_rn(gen, Hd, scale=0.1), dbeta=_rn(gen, Hd, scale=0.1))
    return d


def text_reference(d, eps, p, seed):
    """text_fwd + text_bwd of a text_inputs() dict in one dict"""
    n, X = d["ids"].shape
    Hd = d["word"].shape[1]
    keep = keep_multiplier(seed, n * X, Hd, p) if p > 0 else None
    dd = lambda t: t.double()
    ref = text_fwd(d["ids"], dd(d["word"]), dd(d["pos"]), dd(d["type"][0]), dd(d["gamma"]), dd(d["beta"]), eps, keep)
    b = text_bwd(ref, d["ids"], dd(d["dout"]), dd(d["gamma"]), {k: dd(v) for k, v in d["init"].items()}, keep)
    spec = dict(ref["spec"], **b["spec"])
    ref.update(b)
    ref["spec"] = spec
    return ref


def video_reference(d, B, T, hw, eps):
    dd = lambda t: t.double()
    ref = video_fwd(dd(d["feat"]), B, T, hw, dd(d["cls"]), dd(d["pos"]), dd(d["len"]), dd(d["gamma"]), dd(d["beta"]), eps)
    b = video_bwd(ref, dd(d["dout"]), dd(d["gamma"]), {k: dd(v) for k, v in d["init"].items()})
    spec = dict(ref["spec"], **b["spec"])
    ref.update(b)
    ref["spec"] = spec
    return ref


def im2col_input(B, T, H, W, frame_major, seed=0, device="cpu"):
    """fp32 frames whose bf16 conversion has work to do: bf16 rounding ties (both directions of round-to-even), both signs of zero, magnitudes
    just under the bf16 overflow threshold, and ordinary values"""
    gen = torch.Generator(device=device).manual_seed(seed)
    shape = (B, T, 3, H, W) if frame_major else (B, 3, T, H, W)
    x = torch.randn(shape, generator=gen, device=device)
    flat = x.view(-1)
    # bit patterns: ties 1 + 2^-8 (to even: down), 1 + 3 2^-8 (up), their negatives, 257 and 259, +0, -0, the largest bf16, the last fp32 that still
    # rounds to it (0x7f7f7fff), the tie above it (0x7f7f8000: to even = infinity), their negatives
    special = torch.tensor([0x3f808000, 0x3f818000, 0x3f808000 - 2 ** 31, 0x3f818000 - 2 ** 31, 0x43808000, 0x43818000, 0, -2 ** 31, 0x7f7f0000,
                            0x7f7f7fff, 0x7f7f8000, 0x7f7f7fff - 2 ** 31, 0x7f7f8000 - 2 ** 31], dtype=torch.int32).view(torch.float32).to(device)
    k = min(len(special), flat.numel())
    flat[torch.arange(k, device=device) * (flat.numel() // k)] = special[:k]
    return x
