"""Float64 references of the attention kernels, per-element first-order error bounds derived from the kernels' arithmetic, and the
rounding model the per-slice check compares against (test infrastructure; used by tests/test_attention_bounds_host.py on the CPU and by
tests/test_gpu_attention_bounds.py on the MI355X).

Every mode is reduced to one batched problem: G = (problem, head) slices, each with queries q (G, Nq, hd), keys k and values v (G, Nk, hd),
an additive score term `add` (G or broadcast, Nq, Nk: relative-position bias, shift mask -100, key mask / causal block -inf) and an optional
dropout keep multiplier (0 or 1 / (1 - p)).  The reference works on the same bf16 values the kernel reads, in float64:

    s = scale q k^T + add ;  p = softmax(s) ;  o = (p o keep) v ;  lse2 = logsumexp(s) / ln 2            (log2 domain, as the kernels store it)
    delta = sum_d dO o ;  dV = (p o keep)^T dO ;  dS = p o (keep o dO v^T - delta) ;  dQ = scale dS k ;  dK = scale dS^T q

Error bound (first order; u = 2^-24 fp32 unit roundoff, b = 2^-8 one bf16 rounding, g(n) = n u / (1 - n u) for an n-term fp32 sum).
Every term below is read off the kernel code; "|x|" is elementwise, products of absolute values bound the worst case of each sum.

  scores   E_ik = scale g(hd) sum_d |q_id k_kd|           fp32 MFMA accumulation of the bf16 products over hd (attention_seq.hip:99-160,
                                                           attention_win.hip:155, attention_winl.hip:179, decode.hip:176-181)
                + 4 u (|s_ik| + max_k s_ik)              s * (scale * LOG2E) and the subtraction of the running maximum in fp32
                + EXP_REL                                 fast_exp2 / v_exp_f32 (and __expf in decode.hip:196,243): relative error of 2^-21
                + add_err_ik                              persistent window path only: (bias + mask) / scale stored as a bf16 MFMA fragment
                                                           (attention_win.hip:1169-1255): b |bias + mask|
  forward  |dO|  <= b |o|                                 final bf16 store of O (half an ulp)
                  + b sum_k p_k (keep_k |v_k| + |o|)     P packed to bf16 as the PV MFMA operand (pack_frag, attn_common.h:122); whether the
                                                           row sum l adds the rounded P (seq / window kernels: one more MFMA against a ones
                                                           fragment) or the fp32 P (attention.hip), this covers both normalisation orders
                  + sum_k p_k E_k (keep_k |v_k| + |o|)   the score errors, through d o / d s_k = p_k (keep_k v_k - o)
                  + 2 g(Nk) sum_k p_k keep_k |v_k| + 2 g(Nk) |o|   fp32 accumulation of PV and of l over the keys; the split-K rescale
                                                           of decode.hip:240-245 (one more __expf per split) is inside EXP_REL + g(Nk)
           |dlse2| <= (b + g(Nk) + sum_k p_k E_k) / ln 2 + 4 u |lse2|       l from the bf16 P, the score errors, log2f
           |ddelta| <= sum_d |dO_d| B_o,d + g(hd) sum_d |dO_d o_d|           delta from the STORED bf16 O, fp32 sum over hd
  backward P is recomputed as exp2(v - lse2): relative error ep_ik = E_ik + ln 2 B_lse,i
           E_dS,ik = p_ik (ep_ik |keep dP - delta| + keep g(hd) sum_d |dO_id v_kd| + B_delta,i) + b |dS_ik|      (dS packed to bf16)
           B_dQ = b |dQ| + scale (E_dS |k| + g(Nk) |dS| |k|)      B_dK = b |dK| + scale (E_dS^T |q| + g(Nq) |dS|^T |q|)
           B_dV = b |dV| + ((b + ep) p keep)^T |dO| + g(Nq) (p keep)^T |dO|     (P packed to bf16 for the dV MFMA, bf16 store)
           bias table: sum of E_dS over the (window, i, j) that share a table row, + g(count) sum |dS| (fp32 LDS / atomic sums); the
                       persistent and large-window kernels (win_dbias3, winl_dbias) pack dS to bf16 for their one-hot MFMA sums
                       (attention_winl.hip:642-646), which the b |dS| term of E_dS covers and the rounding model injects (dtab_bf16)
  underflow: P below 2^-126 may flush to zero: + 2^-126 sum_k keep_k |v_k| on O and 2^-126 |keep dP - delta| on dS

Per-slice check: in every (problem, head) slice -- and every head column of the bias-table gradient -- the relative-norm error of the kernel
must stay within SLICE_FACTOR of the rounding model's (the reference with the kernels' bf16 roundings injected, as tests/rounding_model
._AttnCore does).  Rounding errors of random sign add in quadrature and the per-element bound adds them in magnitude, so a systematic error
(a wrong scale, a missing key, a stale delta) that hides under the per-element bound stands out against the model by a large factor."""
import math

import torch

U32 = 2.0 ** -24                # fp32 unit roundoff
U_BF = 2.0 ** -8                # one bf16 rounding, relative (8 significant bits)
EXP_REL = 2.0 ** -21            # v_exp_f32 (fast_exp2, __expf): within 1 ulp of 2^x, plus the product x * log2(e) rounded to fp32
LN2 = math.log(2.0)
TINY = 2.0 ** -126              # smallest normal fp32: an exp2 result below it may be flushed to zero (P of pairs behind the -100 shift mask)
SLICE_FACTOR = 3.0              # the kernel's per-slice relative-norm error may exceed the rounding model's by at most this factor
SLICE_FLOOR = 1e-6              # ... plus this relative floor (slices whose rounding-model error is near fp32 resolution)
NEG = float("-inf")


def gam(n):
    return n * U32 / (1.0 - n * U32)


def bfr(t):
    """one bf16 rounding of a float64 tensor, as the kernels round fp32 (round to nearest even)"""
    return t.float().bfloat16().double()


# ------------------------------------------------------------------------------------------------------------------------------ core
def core(q, k, v, add, scale, keep=None, do=None, add_err=None, p_bf16=True):
    """float64 reference and per-element bounds of one batched attention.  q (G, Nq, hd), k / v (G, Nk, hd), add broadcastable to
    (G, Nq, Nk) with -inf for masked pairs, keep (G, Nq, Nk) or None, do (G, Nq, hd) or None.  Returns a dict of reference tensors and their
    bounds (b_*).  p_bf16 = False: the kernel keeps P in fp32 (decode.hip)."""
    G, Nq, hd = q.shape
    Nk = k.shape[1]
    s = scale * (q @ k.transpose(-1, -2)) + add
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    pk = p * keep if keep is not None else p
    kp = keep if keep is not None else torch.ones_like(p)
    o = pk @ v
    lse2 = ((m + torch.log(l)) / LN2).squeeze(-1)
    fin = torch.isfinite(s)
    E = scale * gam(hd) * (q.abs() @ k.abs().transpose(-1, -2)) + 4 * U32 * (s.abs() + m.abs()) + EXP_REL
    if add_err is not None:
        E = E + add_err
    E = torch.where(fin, E, torch.zeros((), dtype=E.dtype, device=E.device))
    ao, av = o.abs(), v.abs()
    pv_abs = pk @ av
    ub = U_BF if p_bf16 else 0.0
    pE = p * E
    b_o = (U_BF * ao + ub * (pv_abs + ao) + (pE * kp) @ av + pE.sum(-1, keepdim=True) * ao + 2 * gam(Nk) * (pv_abs + ao)
           + TINY * ((kp * fin) @ av))
    b_lse = (ub + gam(Nk) + pE.sum(-1)) / LN2 + 4 * U32 * lse2.abs()
    r = dict(s=s, p=p, o=o, lse2=lse2, b_o=b_o, b_lse=b_lse)
    if do is None:
        return r
    delta = (do * o).sum(-1)
    b_delta = (do.abs() * b_o).sum(-1) + gam(hd) * (do * o).abs().sum(-1)
    dp = do @ v.transpose(-1, -2)
    dpk = dp * kp
    ds = p * (dpk - delta[..., None])
    ep = E + LN2 * b_lse[..., None]
    e_ds = (p * (ep * (dpk - delta[..., None]).abs() + kp * gam(hd) * (do.abs() @ av.transpose(-1, -2)) + b_delta[..., None]) + U_BF * ds.abs()
            + TINY * (dpk - delta[..., None]).abs() * fin)
    dq = scale * (ds @ k)
    dk = scale * (ds.transpose(-1, -2) @ q)
    dv = pk.transpose(-1, -2) @ do
    ads = ds.abs()
    b_dq = U_BF * dq.abs() + scale * (e_ds @ k.abs() + gam(Nk) * (ads @ k.abs()))
    b_dk = U_BF * dk.abs() + scale * (e_ds.transpose(-1, -2) @ q.abs() + gam(Nq) * (ads.transpose(-1, -2) @ q.abs()))
    b_dv = U_BF * dv.abs() + (((U_BF + ep) * pk).transpose(-1, -2) @ do.abs()) + gam(Nq) * (pk.transpose(-1, -2) @ do.abs())
    r.update(delta=delta, b_delta=b_delta, ds=ds, e_ds=e_ds, dq=dq, dk=dk, dv=dv, b_dq=b_dq, b_dk=b_dk, b_dv=b_dv)
    return r


def model(q, k, v, add, scale, keep=None, do=None, keep_bwd=None, delta_fn=None, dv_rows=None, p_bf16=True):
    """the kernels' arithmetic in float64 with their bf16 roundings injected (tests/rounding_model._AttnCore): P a bf16 MFMA operand, O stored
    as bf16, delta from the stored O, dS packed to bf16 for dQ / dK, dQ / dK / dV stored as bf16.  `add` is what the kernel adds (on the
    persistent window path: the bf16 fragment value).  keep_bwd / delta_fn / dv_rows exist so that the host test can express kernel bugs
    that live in the backward only (a mask regenerated with another seed, a wrong delta, a dV sum that misses queries)."""
    s = scale * (q @ k.transpose(-1, -2)) + add
    p = torch.softmax(s, -1)
    pk = p * keep if keep is not None else p
    rp = bfr if p_bf16 else (lambda t: t)
    o = bfr(rp(pk) @ v)
    lse2 = torch.logsumexp(s, -1) / LN2
    r = dict(o=o, lse2=lse2)
    if do is None:
        return r
    kb = keep_bwd if keep_bwd is not None else keep
    pkb = p * kb if kb is not None else p
    delta = (do * o).sum(-1)
    if delta_fn is not None:
        delta = delta_fn(delta)
    dp = do @ v.transpose(-1, -2)
    ds32 = p * ((dp * kb if kb is not None else dp) - delta[..., None])
    ds = bfr(ds32)
    pv = bfr(pkb)
    if dv_rows is not None:
        pv = pv * dv_rows[..., :, None]
    r.update(delta=delta, ds=ds32, dq=bfr(scale * (ds @ k)), dk=bfr(scale * (ds.transpose(-1, -2) @ q)), dv=bfr(pv.transpose(-1, -2) @ do))
    return r


# ------------------------------------------------------------------------------------------------------------------------------ checks
def slice_rel(x, ref, dims):
    d = (x.double() - ref).pow(2).sum(dims).sqrt()
    n = ref.pow(2).sum(dims).sqrt()
    return d / n.clamp_min(1e-300)


def check(name, got, ref, bound, pred=None, slice_dims=None):
    """per-element |got - ref| <= bound, and (pred given) per-slice rel-norm error <= SLICE_FACTOR * pred's + SLICE_FLOOR.
    Returns (failure messages, max err/bound, max slice ratio)."""
    got = got.double()
    err = (got - ref).abs()
    ok = err <= bound
    ok = ok | ((got == ref) & torch.isfinite(ref))
    fails = []
    ratio = float((err / bound.clamp_min(1e-300)).masked_fill(got == ref, 0).max())
    if not bool(ok.all()):
        fails.append(f"{name}: {int((~ok).sum())} of {ok.numel()} elements outside the bound, worst err/bound {ratio:.3g}")
    sr = 0.0
    if pred is not None:
        rk = slice_rel(got, ref, slice_dims)
        rm = slice_rel(pred, ref, slice_dims)
        lim = SLICE_FACTOR * rm + SLICE_FLOOR
        sr = float((rk / lim).max())
        if not bool((rk <= lim).all()):
            i = int((rk / lim).argmax())
            fails.append(f"{name}: slice {i} rel-norm error {float(rk.flatten()[i]):.3g} > {SLICE_FACTOR} x model {float(rm.flatten()[i]):.3g}")
    return fails, ratio, sr


TENSORS = ("o", "lse2", "delta", "dq", "dk", "dv")


def check_all(got, ref, pred, extra=()):
    """got / pred: dicts with any of TENSORS (shape (G, N, ...)) and 'dtab' (rows, heads); ref: the dict of core() (+ 'dtab', 'b_dtab').
    Returns (failures, {tensor: (max err/bound, max slice ratio)})."""
    fails, stats = [], {}
    for t in TENSORS + ("dtab",) + tuple(extra):
        if t not in got:
            continue
        g, r, b = got[t], ref[t], ref["b_" + {"lse2": "lse", "delta": "delta"}.get(t, t)]
        sd = (0,) if t == "dtab" else tuple(range(1, r.dim()))
        f, er, sr = check(t, g, r, b, pred.get(t) if t != "lse2" else None, sd)
        fails += f
        stats[t] = (er, sr)
    return fails, stats


# ------------------------------------------------------------------------------------------------------------------------------ modes
def seq_problem(qkv, n, L, heads, mask=None, causal_from=0, keep=None, dout=None, key_of=None):
    """sequence mode (lav_attn_desc.mode 1, head_dim 64): qkv (n L, 3 heads 64) float64 of the bf16 operand, mask (n, L) (1 attend), causal_from
    (> 0: key k >= causal_from is visible to query i only when i >= causal_from and k <= i; the key mask applies to every key, as
    attention_seq.hip:116,152 do), keep (n, heads, L, L).  Returns (q, k, v, add, keep, do) in the (n heads, L, 64) slice layout; key_of
    (optional) maps (query index, key index) -> the key index the causal test compares with (mutations)."""
    Hd = heads * 64
    dev = qkv.device
    split = lambda t: t.reshape(n, L, heads, 64).transpose(1, 2).reshape(n * heads, L, 64)
    q, k, v = [split(t) for t in qkv.split(Hd, -1)]
    vis = torch.ones(n, L, L, dtype=torch.bool, device=dev)
    if mask is not None:
        vis &= (mask != 0).to(dev)[:, None, :]
    if causal_from:
        i = torch.arange(L, device=dev)[:, None]
        j = torch.arange(L, device=dev)[None, :] if key_of is None else key_of(torch.arange(L, device=dev))[None, :]
        hidden = (torch.arange(L, device=dev)[None, :] >= causal_from) & ((i < causal_from) | (j > i))
        vis &= ~hidden[None]
    add = torch.zeros(n, L, L, dtype=torch.float64, device=dev).masked_fill(~vis, NEG)
    add = add[:, None].expand(n, heads, L, L).reshape(n * heads, L, L)
    kp = keep.to(dev).double().reshape(n * heads, L, L) if keep is not None else None
    do = split(dout) if dout is not None else None
    return q, k, v, add, kp, do


def seq_rows(x, n, L, heads):
    """(n L, heads 64) kernel tensor -> (n heads, L, 64)"""
    return x.reshape(n, L, heads, 64).transpose(1, 2).reshape(n * heads, L, 64)


class Window:
    """window mode geometry (lav_attn_desc.mode 0, head_dim 32) from the oracle helpers, as tests/test_gpu_kernels._win_ref uses them:
    rows (Bw, N) = token row of in-window slot i of window w (shifted coordinates, video_swin.py:218-239), idx (N, N) = bias-table row
    (relative_position_index[:N, :N] of the CONFIGURED window), smask (nW, N, N) = shift mask {-100, 0} or None."""

    def __init__(self, B, D, H, W, heads, win, shift, cfg, device="cpu"):
        from oracle import lavender_ref as R
        self.B, self.D, self.H, self.W, self.heads, self.win, self.shift, self.cfg = B, D, H, W, heads, win, shift, cfg
        self.N = win[0] * win[1] * win[2]
        self.C = heads * 32
        self.M = B * D * H * W
        r = torch.arange(self.M).view(B, D, H, W, 1)
        if any(shift):
            r = torch.roll(r, (-shift[0], -shift[1], -shift[2]), (1, 2, 3))
        self.rows = R.partition(r, win)[..., 0].to(device)                       # (Bw, N)
        self.Bw = self.rows.shape[0]
        self.nW = self.Bw // B
        self.idx = R.rel_pos_index(cfg)[:self.N, :self.N].to(device)
        self.smask = R.shift_mask(D, H, W, win, shift).double().to(device) if any(shift) else None
        self.tbl_rows = (2 * cfg[0] - 1) * (2 * cfg[1] - 1) * (2 * cfg[2] - 1)
        self.device = device

    def gather(self, x, part=None):
        """(M, C) or (M, 3C) kernel tensor -> (Bw heads, N, 32) slices (part 0 / 1 / 2 of a 3C tensor)"""
        if part is not None:
            x = x[:, part * self.C:(part + 1) * self.C]
        return x[self.rows].reshape(self.Bw, self.N, self.heads, 32).transpose(1, 2).reshape(self.Bw * self.heads, self.N, 32)

    def add(self, table, idx=None, smask=None, stored_bf16=False, scale=32 ** -0.5):
        """(Bw heads, N, N) bias + shift mask; stored_bf16: the persistent path's bf16 fragment value scale * bf16((bias + mask) / scale)
        (attention_win.hip:1197-1202), with its rounding bound"""
        idx = self.idx if idx is None else idx
        smask = self.smask if smask is None else smask
        bias = table.double().to(self.device)[idx].permute(2, 0, 1)               # (heads, N, N)
        a = bias[None].expand(self.B * self.nW, -1, -1, -1)
        if smask is not None:
            a = (a.reshape(self.B, self.nW, self.heads, self.N, self.N) + smask[None, :, None]).reshape(self.Bw, self.heads, self.N, self.N)
        a = a.reshape(self.Bw * self.heads, self.N, self.N)
        if not stored_bf16:
            return a, None
        inv = float(torch.tensor(1.0 / scale, dtype=torch.float32))
        stored = (a.float() * inv).bfloat16().double() * scale
        return stored, U_BF * a.abs()

    def dtab(self, ds, idx=None, skip_window=None):
        """bias-table gradient (tbl_rows, heads) from the dS slices (Bw heads, N, N): sum over windows, then over the pairs of a table row"""
        idx = self.idx if idx is None else idx
        d = ds.reshape(self.Bw, self.heads, self.N, self.N)
        if skip_window is not None:
            d = torch.cat([d[:skip_window], d[skip_window + 1:]])
        d = d.sum(0)
        out = torch.zeros(self.tbl_rows, self.heads, dtype=torch.float64, device=ds.device)
        out.index_add_(0, idx.reshape(-1), d.reshape(self.heads, -1).t())
        return out

    def dtab_bound(self, ds, e_ds):
        """E_dS summed like dS, + g(terms) sum |dS| for the fp32 sums (LDS, then atomics across workgroups) of Bw * (pairs per row) terms"""
        cnt = torch.bincount(self.idx.reshape(-1), minlength=self.tbl_rows).max().item()
        return self.dtab(e_ds) + gam(self.Bw * cnt) * self.dtab(ds.abs())


# ------------------------------------------------------------------------------------------------------------------------------ whole cases
def seq_case(qkv, n, L, heads, mask=None, causal_from=0, keep=None, dout=None):
    """reference (+ bounds) and rounding-model prediction of a sequence-mode launch; qkv / dout: float64 (on the device the reference runs on)"""
    q, k, v, add, kp, do = seq_problem(qkv, n, L, heads, mask, causal_from, keep, dout)
    ref = core(q, k, v, add, 0.125, kp, do)
    pred = model(q, k, v, add, 0.125, kp, do)
    return ref, pred


def win_case(geo, qkv, table, dout=None, persistent=False):
    """reference (+ bounds, + bias-table gradient) and rounding-model prediction of a window-mode launch on geometry geo (Window)"""
    q, k, v = (geo.gather(qkv, i) for i in range(3))
    add, _ = geo.add(table)
    add_k, add_err = geo.add(table, stored_bf16=True) if persistent else (add, None)
    do = geo.gather(dout) if dout is not None else None
    ref = core(q, k, v, add, 32 ** -0.5, None, do, add_err=add_err)
    pred = model(q, k, v, add_k, 32 ** -0.5, None, do)
    if do is not None:
        ref["dtab"] = geo.dtab(ref["ds"])
        ref["b_dtab"] = geo.dtab_bound(ref["ds"], ref["e_ds"])
        pred["dtab"] = geo.dtab(pred["ds"])
        pred["dtab_bf16"] = geo.dtab(bfr(pred["ds"]))
    return ref, pred


def decode_problem(qkv_pre, mask, ck, cv, qkv_new, B, heads, Lv, nc, q_len, beams=1):
    """the decode attention (decode.hip:139-229, lav_attn_decode_desc) as (B heads) slices: queries = the q_len new rows; keys = the Lv
    prefix rows of clip b // beams (key mask applies), the nc cached text rows, then the new rows causally.  All float64 on one device."""
    H = heads * 64
    dev = qkv_new.device
    pre = qkv_pre.repeat_interleave(beams, 0) if beams > 1 else qkv_pre
    km = mask.repeat_interleave(beams, 0) if beams > 1 else mask
    hs = lambda t: t.reshape(t.shape[0], t.shape[1], heads, 64).transpose(1, 2)          # (B, heads, rows, 64)
    q = hs(qkv_new[:, :, :H])
    k = torch.cat([hs(pre[:, :, H:2 * H]), ck[:, :, :nc], hs(qkv_new[:, :, H:2 * H])], 2)
    v = torch.cat([hs(pre[:, :, 2 * H:]), cv[:, :, :nc], hs(qkv_new[:, :, 2 * H:])], 2)
    Lk = Lv + nc + q_len
    vis = torch.ones(B, q_len, Lk, dtype=torch.bool, device=dev)
    vis[:, :, :Lv] = (km != 0).to(dev)[:, None, :]
    vis[:, :, Lv + nc:] = torch.tril(torch.ones(q_len, q_len, dtype=torch.bool, device=dev))[None]
    add = torch.zeros(B, q_len, Lk, dtype=torch.float64, device=dev).masked_fill(~vis, NEG)
    add = add[:, None].expand(B, heads, q_len, Lk).reshape(B * heads, q_len, Lk)
    f = lambda t: t.reshape(B * heads, t.shape[2], 64)
    return f(q), f(k), f(v), add


def decode_case(*args, **kw):
    q, k, v, add = decode_problem(*args, **kw)
    return core(q, k, v, add, 0.125, p_bf16=False), model(q, k, v, add, 0.125, p_bf16=False)
