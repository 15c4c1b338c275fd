"""Forward/backward orchestration of the hot path on top of the HIP kernels (lavender_amd.hip).

Each torch.autograd.Function below is one *stage* of the reference model (a Swin block, a patch merge, a BERT
layer, ...): its forward enqueues the stage's kernels and keeps the activations the backward needs; its backward
enqueues the hand-written backward kernels, ACCUMULATES parameter gradients straight into the flat gradient
arena (fp32 atomics) and returns only the activation gradient.  torch.autograd is used for the stage-level graph
bookkeeping only -- no arithmetic runs in ATen.

`anchor` is a 1-element requires-grad tensor (arena.anchor) threaded through every stage so that autograd runs
the stage's backward even though its parameters are not autograd inputs.
"""
import ctypes
import os

import numpy as np
import torch

from . import hip as K

bf16 = torch.bfloat16

# ---- the LAV_* switches of this file ------------------------------------------------------------------------------------
# Module attributes: tests, bench.py and the tools set them at run time, so every reader takes them at call time.
# dW = dy^T x is never needed before the optimizer, so it does not have to sit in the dy -> dx dependency chain: issued on
# a second stream it fills the CUs the main stream leaves idle (partial last rounds of 1-block-per-CU GEMMs, kernel
# ramps and tails between ~1500 dependent launches per step).  All dW kernels share that ONE stream, so their
# accumulations into the gradient arena (and the split-K workspace of that stream) stay ordered among themselves.
_DW_SIDE = os.environ.get("LAV_DW_STREAM", "1") != "0"
_GQ = 2 if os.environ.get("LAV_GELU_GRAD_U8", "0") != "0" else 1          # GELU' storage: 1 = bf16 (default), 2 = one byte per element (measured 0.8 ms/step SLOWER: the pack / unpack VALU work outweighs the bytes)
_GQ_DT = torch.uint8 if _GQ == 2 else torch.bfloat16
_DW_PRIORITY = int(os.environ.get("LAV_DW_PRIORITY", "0"))      # probe hook: HIP priority of the weight-gradient stream (positive = lower than the main stream)
# fp32 residual stream of the post-LN fusion encoder: the pre-LN sums x + dropout(dense(.)) and the LayerNorm outputs that
# feed the next residual add stay fp32 (the GEMM operands are the bf16 copies).  Measured on the oracle with bf16 rounding
# injected (tests/bf16_error_budget.py): this halves the logit error of the full-width model (mean 5.5e-3 -> 2.5e-3, max
# 3.6e-2 -> 1.6e-2); the same change on the pre-LN Swin stream changes nothing, so the video side stays bf16.
STREAM32 = os.environ.get("LAV_STREAM32", "1") != "0"
# Late round 4: that wide stream is stored as fp16 rows, not fp32 -- 11 mantissa bits against bf16's 8 keep the logit error where the fp32
# stream had it (oracle with the rounding injected, Swin-B + 12 layers: mean |d| 2.65e-3 / max 1.72e-2 with an fp16 stream, 2.56e-3 / 1.64e-2
# with fp32, 5.49e-3 / 3.55e-2 with bf16) at half the bytes: 69 instead of 138 MB per pre-LayerNorm tensor at the cfg2 shape, read three
# times and written once per LayerNorm.  Stores saturate at +-65504.  LAV_STREAM_DTYPE=fp32 restores fp32 rows (the reference itself ran
# fp16 autocast, utils/deepspeed.py:20-51).
STREAM_DT = torch.float32 if os.environ.get("LAV_STREAM_DTYPE", "fp16") == "fp32" else torch.float16
# The fp32 copy of a LayerNorm output only ever feeds the NEXT residual add, so it is not written: that GEMM epilogue takes the
# saved pre-LayerNorm rows + (mean, rstd, gamma, beta) and adds LayerNorm(rows) itself (lav_gemm_epilogue.res_ln_*; same
# arithmetic, same bits).  138 MB less written per LayerNorm at the cfg2 shape.  LAV_RESLN=0 restores the fp32 LayerNorm output.
RESLN = STREAM32 and os.environ.get("LAV_RESLN", "1") != "0"
# Swin blocks whose windows run the persistent kernels (<= 256 tokens, head_dim 32: every Swin-T / Swin-B stage) keep their fused
# q | k | v projection HEAD-MAJOR -- [q | k | v][head][token][32], written that way by the QKV GEMM epilogue (lav_gemm_epilogue.hm_*) --
# so that a window's operand pieces are whole 128-byte lines instead of 64-byte halves of the (rows, 3C) rows.  Only the attention
# kernels read qkv (its gradient dqkv stays row-major: it is a GEMM operand).  LAV_QKV_HEADMAJOR=0 restores the row-major layout.
QKV_HEADMAJOR = os.environ.get("LAV_QKV_HEADMAJOR", "1") != "0"
# Fusion-encoder layers through the stage-level C entries (lav_bert_layer_fwd / _bwd, csrc/stages.cpp): one host -> C transition per
# layer pass instead of 7 (forward) / 15 (backward); the same kernels with the same arguments, bit-identical results.  Applies to the
# default configuration (fp32 residual stream with the recomputed-LayerNorm residual, bf16 GELU') of every layer that does not read its
# input through the pair map.  LAV_STAGE_C=0 restores the per-kernel path.
STAGE_C = os.environ.get("LAV_STAGE_C", "1") != "0"
_FUSION_SRC = os.environ.get("LAV_FUSION_SRC", "1") != "0"       # 0: separate feat_img / feat_txt buffers + T.cat in front of the fusion encoder (A/B baseline)
# the first fusion layer reads its input THROUGH the pair map (lav_gemm_epilogue.a_rowmap / res_rowmap) instead of a gathered
# (pairs, L, H) copy; needs the 256-column GEMM tiles.  LAV_PAIR_FUSED=0 restores the materialised gather (PairSeqFn).
PAIR_FUSED = os.environ.get("LAV_PAIR_FUSED", "1") != "0"


def W16(p):
    try:
        return p._lav16
    except AttributeError:
        raise RuntimeError("parameter is not in a ParamArena: call model.cuda() / model.build_arena() first") from None


def W16T(p):
    """transposed bf16 working copy (in_features, out_features): the K-contiguous operand of dx = dy W"""
    try:
        return p._lav16t
    except AttributeError:
        raise RuntimeError("parameter has no transposed working copy in the ParamArena") from None


def G(p):
    """gradient view of p for a writer that ACCUMULATES (atomics, read-modify-write): a first-touch unit (arena.FtUnit) is made valid first"""
    u = p.__dict__.get("_lav_ft")
    if u is not None and u.state != 2:
        u.before_accumulate()
    return p._lavg


def GR(p):
    """the raw gradient view (address only: descriptor caches; no first-touch bookkeeping)"""
    return p._lavg


def GW(p):
    """(gradient view, assign) for the layout-2 GEMM that writes p's weight gradient: assign = this call is the first writer since zero_grad and
    stores its result (lav_gemm_epilogue.assign) instead of adding to the memory -- which then need not have been zeroed"""
    u = p.__dict__.get("_lav_ft")
    return p._lavg, (u.take() if u is not None else False)


def _assign_mask(params):
    """lav_*_bwd_desc.assign_mask of a stage-level backward entry: bit j = the j-th weight gradient is assigned (first writer of the step)"""
    m = 0
    for j, p in enumerate(params):
        if GW(p)[1]:
            m |= 1 << j
    return m


def _gw(p, shape=None):
    """keyword arguments of the weight-gradient GEMM into p: out / accumulate / assign (first writer since zero_grad assigns)"""
    g, a = GW(p)
    return dict(out=g if shape is None else g.view(shape), accumulate=True, assign=a)


_arenas = []


def register_arena(a):
    import weakref
    _arenas.append(weakref.ref(a))


_dw_streams = {}


def dw_stream(device):
    st = _dw_streams.get(device)
    if st is None:
        st = _dw_streams[device] = torch.cuda.Stream(device=device, priority=_DW_PRIORITY)
    return st


def on_dw_stream(device, fn, tensors):
    """fn() on the weight-gradient stream of `device`, behind everything the current stream holds; the join at the end of the backward is armed
    and `tensors` (what fn's kernels touch; None entries are skipped) are recorded on that stream, so the caller may free them right after this
    returns.  With LAV_DW_STREAM=0 (read here, at call time) or off the GPU fn() runs in place."""
    if not _DW_SIDE or device.type != "cuda":
        return fn()
    side = dw_stream(device)
    _arm_join()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    for t in tensors:
        if t is not None:
            t.record_stream(side)


def dw_gemm(A, Bm, M, N, Kd, **kw):
    """layout-2 GEMM accumulating into the gradient arena; A / Bm may be freed by the caller right after this returns."""
    on_dw_stream(A.device, lambda: K.gemm(2, A, Bm, M, N, Kd, **kw), (A, Bm, kw.get("k_keep")))


class DwGroup:
    """The weight-gradient GEMMs of one stage collected and issued as ONE grouped launch on the weight-gradient stream (lav_gemm_tn_grouped;
    the stage-level C entries do the same from C).  add() has dw_gemm's meaning; launch() after the last operand was produced.  Without the
    side stream or with grouping switched off every add() launches at once, as dw_gemm does."""

    def __init__(self, shapes, Kd):
        self.gs = K.group_splits_for(shapes, Kd) if _DW_SIDE else 0
        self.jobs = []

    def add(self, A, Bm, M, N, Kd, gw, splits, rowsum_a=None):
        out, assign = gw                                       # GW(parameter): (gradient view, first writer of the step)
        if not self.gs:
            return dw_gemm(A, Bm, M, N, Kd, out=out, accumulate=True, splits=splits, rowsum_a=rowsum_a, assign=assign)
        self.jobs.append(dict(A=A, B=Bm, M=M, N=N, out=out, rowsum_a=rowsum_a, fallback_splits=splits, assign=assign))

    def launch(self, device):
        if self.jobs:
            on_dw_stream(device, lambda: K.gemm_tn_grouped(self.jobs, self.gs), [j[k] for j in self.jobs for k in "AB"])
            self.jobs = []


def _stage_bwd(entry, fields, shapes, Kd, rpg, device, operands):
    """a stage-level backward entry (K.swin_block_bwd / K.bert_layer_bwd): it issues the stage's weight-gradient GEMMs (outputs `shapes` over Kd
    token rows, rpg: K.ensure_stage_workspaces) on the weight-gradient stream itself (None: in line), so their `operands` are recorded there --
    not to be recycled before that stream ran"""
    side = dw_stream(device) if _DW_SIDE else None
    raw = side.cuda_stream if side is not None else None
    _arm_join()
    K.ensure_stage_workspaces(shapes, Kd, rpg, raw)
    entry(fields, raw)
    for t in operands if side is not None else ():
        t.record_stream(side)


def ln_bwd(dy, *args, **kw):
    """K.layernorm_bwd with the column reductions (dgamma / dbeta / bias column sums: parameter gradients) DEFERRED: completed by dw_join /
    the arena's range events / the end-of-backward callback (K.layernorm_flush), one launch for all of them."""
    _arm_join()
    return K.layernorm_bwd(dy, *args, flush=False, **kw)


_join_armed = [-1]                      # id of the autograd graph task whose end-of-backward callback is queued (-1: none)


def _end_of_backward():
    _join_armed[0] = -1
    dw_join()


def _arm_join():
    """Called by everything that leaves gradient work pending (weight-gradient kernels on the side stream, deferred LayerNorm reductions): the
    join + flush run once as a final callback of the CURRENT autograd backward pass, so `.grad` is whole when backward() returns -- also for a
    caller that never heard of dw_join.  The armed state is keyed to the graph task: a backward that raised (OOM, a user hook) never runs its
    callback, and the next backward -- a new graph task -- arms its own instead of trusting the stale flag.  Outside a backward pass
    (kernel-level tests drive these helpers directly) nothing is armed."""
    task = torch._C._current_graph_task_id()
    if task >= 0 and _join_armed[0] != task:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_end_of_backward)
            _join_armed[0] = task
        except RuntimeError:
            pass


def dw_join(device=None):
    """main stream waits for every weight-gradient kernel issued so far (before the gradients are read); the LayerNorm column
    reductions queued on the main stream (lav_layernorm_set_defer) are completed first."""
    # (idempotent and cheap: an explicit call and the end-of-backward callback may both run; _join_armed is left to the callback, so a dw_join
    # made from INSIDE a backward -- the data-parallel range events -- does not queue a second callback for the same graph task)
    if torch.cuda.is_available():
        K.layernorm_flush()
    for dev, st in _dw_streams.items():
        if device is None or dev == device:
            torch.cuda.current_stream(dev).wait_stream(st)
    dead = False
    for r in _arenas:                                         # weight gradients nobody wrote in this step: zero instead of last step's values
        a = r()
        if a is None:
            dead = True
        elif a._ft_armed:
            a.finish_first_touch()
    if dead:
        _arenas[:] = [r for r in _arenas if r() is not None]


def _keep(ctx):
    """True when this stage will be differentiated (autograd Function.forward itself runs in no-grad mode, so
    the decision comes from the inputs' needs_input_grad -- the arena anchor requires grad iff grad mode was on)."""
    return any(ctx.needs_input_grad)


_PAD_MAPS = {}


def pad_maps(device, B, grid, window):
    """Row maps between a (B, D, H, W) token grid and the same grid zero-padded at the far edges up to multiples of `window`
    (F.pad of video_swin.py:211-215 / :273-276 as two row gathers).  None when nothing is padded; else
    ((Dp, Hp, Wp), padded row count, to_pad[int32: padded row -> real row or -1], to_real[int32: real row -> padded row])."""
    D, H, W = grid
    Dp, Hp, Wp = (-(-g // w) * w for g, w in zip(grid, window))
    if (Dp, Hp, Wp) == (D, H, W):
        return None
    key = (str(device), B, D, H, W, Dp, Hp, Wp)
    if key not in _PAD_MAPS:
        real = np.arange(B * D * H * W, dtype=np.int32).reshape(B, D, H, W)
        to_pad = np.full((B, Dp, Hp, Wp), -1, dtype=np.int32)
        to_pad[:, :D, :H, :W] = real
        to_real = np.arange(B * Dp * Hp * Wp, dtype=np.int32).reshape(B, Dp, Hp, Wp)[:, :D, :H, :W]
        _PAD_MAPS[key] = ((Dp, Hp, Wp), B * Dp * Hp * Wp, torch.from_numpy(to_pad.reshape(-1)).to(device),
                          torch.from_numpy(np.ascontiguousarray(to_real).reshape(-1)).to(device))
    return _PAD_MAPS[key]


# ---------------------------------------------------------------------------------------------------
# Swin stages
# ---------------------------------------------------------------------------------------------------
class PatchEmbedFn(torch.autograd.Function):
    """PatchEmbed3D.forward (video_swin.py:388-405): im2col + GEMM + LayerNorm -> channels-last tokens."""

    @staticmethod
    def forward(ctx, anchor, img, mod, frame_major):
        B, T = (img.shape[0], img.shape[1]) if frame_major else (img.shape[0], img.shape[2])
        H, W = img.shape[-2], img.shape[-1]
        E = mod.embed_dim
        img = img.contiguous().float()
        cols = K.patch_im2col(img, B, T, H, W, frame_major)
        M = cols.shape[0]
        w16 = W16(mod.proj.weight).view(E, 96)
        y = K.gemm(0, cols, w16, M, E, 96, bias=mod.proj.bias.data)
        x, mean, rstd = K.layernorm_fwd(y, M, E, mod.norm.weight.data, mod.norm.bias.data, 1e-5, want_stats=_keep(ctx))
        ctx.mod = mod
        ctx.save_for_backward(cols, y, mean, rstd)
        return x

    @staticmethod
    def backward(ctx, dx):
        mod = ctx.mod
        cols, y, mean, rstd = ctx.saved_tensors
        M, E = y.shape
        dx = dx.contiguous()
        dy = ln_bwd(dx, y, M, E, mod.norm.weight.data, mean, rstd, G(mod.norm.weight), G(mod.norm.bias),
                             colsum=G(mod.proj.bias))
        dw_gemm(dy, cols, E, 96, M, **_gw(mod.proj.weight, (E, 96)), splits=K.splits_for(E, 96, M))
        dw_join(dy.device)                                # last stage of the backward: every gradient is final on the main stream
        return None, None, None, None


# ---- lav_swin_block_desc / lav_swin_block_bwd_desc: values labelled by field name, placed by K.SB_FWD / K.SB_BWD -------------------------
_SB_PARAMS = ("ln1_gamma", "ln1_beta", "w_qkv", "b_qkv", "w_proj", "b_proj", "ln2_gamma", "ln2_beta", "w_fc1", "b_fc1", "w_fc2", "b_fc2")
_SB_FWD_NAMES = ("rows", "C", "heads", "rows_per_group", "qkv_headmajor", "ln_eps", "attn") + _SB_PARAMS + (
    "dp_attn", "dp_mlp", "x", "y1", "mean1", "rstd1", "mean2", "rstd2", "qkv", "ao", "lse", "x_mid", "y2", "h_pre", "h", "out")
_SB_BWD_CONSTS = ("wt_qkv", "wt_proj", "wt_fc1", "wt_fc2", "ldt_qkv", "ldt_proj", "ldt_fc1", "ldt_fc2", "g_ln1_gamma", "g_ln1_beta", "g_w_qkv",
                  "g_b_qkv", "g_bias_table", "g_w_proj", "g_b_proj", "g_ln2_gamma", "g_ln2_beta", "g_w_fc1", "g_b_fc1", "g_w_fc2", "g_b_fc2")
_SB_BWD_NAMES = _SB_FWD_NAMES + ("dy", "alpha_attn", "alpha_mlp") + _SB_BWD_CONSTS + ("splits_qkv", "splits_proj", "splits_fc1", "splits_fc2") + (
    "dh", "d_y2", "d_mid", "d_ao", "dqkv", "d_y1", "dx", "group_splits", "assign_mask")
_SB_FWD_PLACE, _SB_BWD_PLACE = K.SB_FWD.placer(_SB_FWD_NAMES), K.SB_BWD.placer(_SB_BWD_NAMES)


def _stage_consts(owner, arena, params, wt, grads, **more):
    """The cached constants of a stage on `owner` (a Swin block, a fusion layer): `params` = the device addresses of its parameter tensors,
    `bwd` = those of the transposed weight copies `wt`, their row strides, and the gradient accumulators `grads`.  All are arena views, fixed
    for the arena's life: the cache is keyed on the arena."""
    dp = lambda ts: tuple(t.data_ptr() for t in ts)
    consts = dict(params=dp(params), bwd=dp(wt) + tuple(K._ld(t) for t in wt) + dp(grads), **more)
    owner.__dict__["_lav_stage_consts"] = (arena, consts)
    return consts


def _block_consts(blk, arena):
    """a Swin block's `params` (labelled _SB_PARAMS) and `bwd` (labelled _SB_BWD_CONSTS) addresses"""
    c = blk.__dict__.get("_lav_stage_consts")
    if c is not None and c[0] is arena:
        return c[1]
    a, mlp, n1, n2 = blk.attn, blk.mlp, blk.norm1, blk.norm2
    mats = (a.qkv.weight, a.proj.weight, mlp.fc1.weight, mlp.fc2.weight)
    params = (n1.weight.data, n1.bias.data, W16(a.qkv.weight), a.qkv.bias.data, W16(a.proj.weight), a.proj.bias.data, n2.weight.data, n2.bias.data,
              W16(mlp.fc1.weight), mlp.fc1.bias.data, W16(mlp.fc2.weight), mlp.fc2.bias.data)
    grads = (n1.weight, n1.bias, a.qkv.weight, a.qkv.bias, a.relative_position_bias_table, a.proj.weight, a.proj.bias, n2.weight, n2.bias,
             mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias)
    assert len(params) == len(_SB_PARAMS) and 2 * len(mats) + len(grads) == len(_SB_BWD_CONSTS)
    return _stage_consts(blk, arena, params, [W16T(p) for p in mats], [GR(p) for p in grads])


def _window_attn(blk, geo, C, grid):
    """(the window K.Attn of a Swin block on the (D, H, W) `grid`, head-major qkv or not)"""
    heads = blk.num_heads
    win, sh, cfg = geo["window"], geo["shift"], geo["cfg_window"]
    hm = QKV_HEADMAJOR and C // heads == 32 and win[0] * win[1] * win[2] <= 256
    att = K.Attn(0, heads, C // heads, B=geo["B"], D=grid[0], H=grid[1], W=grid[2], wd=win[0], wh=win[1], ww=win[2], sd=sh[0], sh=sh[1],
                 sw=sh[2], cfg_wd=cfg[0], cfg_wh=cfg[1], cfg_ww=cfg[2], bias_table=blk.attn.relative_position_bias_table.data,
                 qkv_headmajor=int(hm))
    return att, hm


def _keep_swin_ctx(ctx, blk, att, rpg, geo, dp_attn, pad):
    ctx.blk, ctx.att, ctx.rpg, ctx.pad = blk, att, rpg, pad
    ctx.notify, ctx.arena = geo.get("notify"), geo.get("arena")     # notify: first block of a stage, its backward completes the stage's gradients
    ctx.has_dp, ctx.keep_attn = dp_attn is not None, float(blk.keep_prob) if dp_attn is not None else 1.0


def _stat_rows(st, n):
    """addresses of the n rows (mean, rstd, ...) of a statistics tensor; NULLs when nothing was kept"""
    return tuple(r.data_ptr() for r in st.unbind(0)) if st is not None else (0,) * n


def _swin_fwd_values(head, dp_attn, dp_mlp, x, y1, st, qkv, ao, lse, x_mid, y2, h_pre, h, out_ptr):
    """lav_swin_block_desc, labelled _SB_FWD_NAMES.  head: the scalars, the window descriptor's address and the parameter addresses;
    st: the (4, rows) statistics mean1, rstd1, mean2, rstd2.  Called on the fresh tensors (forward) and on the unpacked saved ones (backward)."""
    dp = K._dp
    return head + (dp(dp_attn), dp(dp_mlp), x.data_ptr(), y1.data_ptr()) + _stat_rows(st, 4) + (
        qkv.data_ptr(), ao.data_ptr(), dp(lse), x_mid.data_ptr(), y2.data_ptr(), dp(h_pre), h.data_ptr(), out_ptr)


class SwinBlockFn(torch.autograd.Function):
    """SwinTransformerBlock3D.forward (video_swin.py:204-261) on (M, C) channels-last tokens."""

    @staticmethod
    def forward(ctx, anchor, x, blk, geo, dp_attn, dp_mlp):
        M, C = x.shape
        heads = blk.num_heads
        B, D, H, Wd = geo["B"], geo["D"], geo["H"], geo["W"]
        rpg = M // B
        a, mlp = blk.attn, blk.mlp
        keep = _keep(ctx)
        pad = pad_maps(x.device, B, (D, H, Wd), geo["window"])
        if STAGE_C and pad is None and _GQ == 1 and x.is_contiguous():
            return SwinBlockFn._forward_c(ctx, x, blk, geo, dp_attn, dp_mlp, keep)
        y1, mean1, rstd1 = K.layernorm_fwd(x, M, C, blk.norm1.weight.data, blk.norm1.bias.data, 1e-5, want_stats=keep)
        if pad is not None:
            # zero rows AFTER norm1 up to window multiples (video_swin.py:211-215): the qkv GEMM then gives the padded tokens
            # q = k = v = bias, exactly what Linear(0) is in the reference; they attend and are attended to (no mask)
            (D, H, Wd), Ma, to_pad, to_real = pad
            y1 = K.gather_rows(y1, to_pad, Ma, C)
        else:
            Ma = M
        att, hm = _window_attn(blk, geo, C, (D, H, Wd))
        qkv = K.gemm(0, y1, W16(a.qkv.weight), Ma, 3 * C, C, bias=a.qkv.bias.data, headmajor=(heads, 32) if hm else None)
        lse = torch.empty(att.lse_elems(), dtype=torch.float32, device=x.device) if keep else None
        ao = torch.empty((Ma, C), dtype=bf16, device=x.device)
        att.fwd(qkv, ao, lse)
        ao_p = ao
        if pad is not None:
            ao = K.gather_rows(ao_p, to_real, M, C)       # crop (video_swin.py:241-242), before proj: proj is row-wise
        x_mid = K.gemm(0, ao, W16(a.proj.weight), M, C, C, bias=a.proj.bias.data, row_scale=dp_attn, rows_per_group=rpg,
                       residual=x)
        y2, mean2, rstd2 = K.layernorm_fwd(x_mid, M, C, blk.norm2.weight.data, blk.norm2.bias.data, 1e-5, want_stats=keep)
        h_pre = torch.empty((M, 4 * C), dtype=_GQ_DT, device=x.device) if keep else None      # GELU' (bf16, or the one-byte code with LAV_GELU_GRAD_U8=1)
        h = K.gemm(0, y2, W16(mlp.fc1.weight), M, 4 * C, C, bias=mlp.fc1.bias.data, act=1, preact=h_pre, preact_is_grad=_GQ)
        out = K.gemm(0, h, W16(mlp.fc2.weight), M, C, 4 * C, bias=mlp.fc2.bias.data, row_scale=dp_mlp, rows_per_group=rpg,
                     residual=x_mid)
        if keep:
            _keep_swin_ctx(ctx, blk, att, rpg, geo, dp_attn, pad)
            ctx.save_for_backward(x, y1, mean1, rstd1, qkv, ao, lse, x_mid, y2, mean2, rstd2, h_pre, h,
                                  dp_attn if dp_attn is not None else x.new_empty(0),
                                  dp_mlp if dp_mlp is not None else x.new_empty(0),
                                  ao_p if pad is not None else x.new_empty(0))
        return out

    @staticmethod
    def _forward_c(ctx, x, blk, geo, dp_attn, dp_mlp, keep):
        """the seven launches of the block (grid a multiple of the window) through ONE call of lav_swin_block_fwd"""
        M, Cn = x.shape
        rpg = M // geo["B"]
        c = _block_consts(blk, geo.get("arena"))
        att, hm = _window_attn(blk, geo, Cn, (geo["D"], geo["H"], geo["W"]))
        dev, e = x.device, torch.empty
        y1, ao, x_mid, y2, out = (e((M, Cn), dtype=bf16, device=dev) for _ in range(5))
        qkv, h = e((M, 3 * Cn), dtype=bf16, device=dev), e((M, 4 * Cn), dtype=bf16, device=dev)
        st = lse = h_pre = None
        if keep:
            st = e((4, M), dtype=torch.float32, device=dev)           # mean1, rstd1, mean2, rstd2
            lse = e(att.lse_elems(), dtype=torch.float32, device=dev)
            h_pre = e((M, 4 * Cn), dtype=bf16, device=dev)
        head = (M, Cn, blk.num_heads, rpg, int(hm), 1e-5, ctypes.addressof(att.d)) + c["params"]
        K.swin_block_fwd(_SB_FWD_PLACE(_swin_fwd_values(head, dp_attn, dp_mlp, x, y1, st, qkv, ao, lse, x_mid, y2, h_pre, h, out.data_ptr())))
        if keep:
            # ctx.att: the window K.Attn must outlive the backward -- its address is inside the descriptor head
            _keep_swin_ctx(ctx, blk, att, rpg, geo, dp_attn, None)
            # the backward rebuilds the activation addresses from the UNPACKED saved tensors (saved-tensor hooks may move them); kept from
            # here: the scalar / parameter head of the descriptor, the address of the block output (never read by the backward) and
            # c_consts, the FORWARD's constants (not re-queried in the backward: the cache may have been rebuilt since)
            ctx.c_stage, ctx.c_head, ctx.c_out, ctx.c_consts = True, head, out.data_ptr(), c
            ctx.save_for_backward(x, y1, st, qkv, ao, lse, x_mid, y2, h_pre, h,
                                  dp_attn if dp_attn is not None else x.new_empty(0), dp_mlp if dp_mlp is not None else x.new_empty(0))
        return out

    @staticmethod
    def _backward_c(ctx, dy):
        blk = ctx.blk
        x, y1, st, qkv, ao, lse, x_mid, y2, h_pre, h, dp_attn, dp_mlp = ctx.saved_tensors
        has_dp = ctx.has_dp
        if not has_dp:
            dp_attn = dp_mlp = None
        (M, Cn), dev, e = x.shape, x.device, torch.empty
        d_y2, d_mid, d_ao, d_y1, dx = (e((M, Cn), dtype=bf16, device=dev) for _ in range(5))
        dh, dqkv = e((M, 4 * Cn), dtype=bf16, device=dev), e((M, 3 * Cn), dtype=bf16, device=dev)
        alpha = 1.0 / ctx.keep_attn
        am = (blk.mlp.fc2.weight, blk.mlp.fc1.weight, blk.attn.proj.weight, blk.attn.qkv.weight)      # order of lav_swin_block_bwd_desc.assign_mask
        splits = (K.splits_for(3 * Cn, Cn, M), K.splits_for(Cn, Cn, M, has_dp), K.splits_for(4 * Cn, Cn, M), K.splits_for(Cn, 4 * Cn, M, has_dp))
        gs = K.group_splits_for(((Cn, 4 * Cn), (4 * Cn, Cn), (Cn, Cn), (3 * Cn, Cn)), M)
        fwd = _swin_fwd_values(ctx.c_head, dp_attn, dp_mlp, x, y1, st, qkv, ao, lse, x_mid, y2, h_pre, h, ctx.c_out)
        fields = _SB_BWD_PLACE(fwd + (dy.data_ptr(), alpha, alpha) + ctx.c_consts["bwd"] + splits + tuple(
            t.data_ptr() for t in (dh, d_y2, d_mid, d_ao, dqkv, d_y1, dx)) + (gs, _assign_mask(am)))       # labelled _SB_BWD_NAMES
        _stage_bwd(K.swin_block_bwd, fields, ((3 * Cn, Cn), (Cn, Cn), (4 * Cn, Cn), (Cn, 4 * Cn)), M, (0, ctx.rpg, 0, ctx.rpg) if has_dp else None, dev,
                   (dy, h, dh, y2, d_mid, ao, dqkv, y1, qkv, d_ao, lse) + ((dp_attn, dp_mlp) if has_dp else ()))
        if ctx.notify and ctx.arena is not None:
            ctx.arena.notify(ctx.notify)
        return None, dx, None, None, None, None

    @staticmethod
    def backward(ctx, dy):
        if getattr(ctx, "c_stage", False):
            return SwinBlockFn._backward_c(ctx, dy.contiguous())
        blk, att, rpg = ctx.blk, ctx.att, ctx.rpg
        a, mlp = blk.attn, blk.mlp
        x, y1, mean1, rstd1, qkv, ao, lse, x_mid, y2, mean2, rstd2, h_pre, h, dp_attn, dp_mlp, ao_p = ctx.saved_tensors
        if not ctx.has_dp:
            dp_attn = dp_mlp = None
        alpha = 1.0 / ctx.keep_attn
        M, C = x.shape
        pad = ctx.pad
        Ma = M if pad is None else pad[1]
        dy = dy.contiguous()
        # --- MLP branch: out = x_mid + s * fc2(gelu(fc1(LN2(x_mid)))) -----------------------------------
        dw_gemm(dy, h, C, 4 * C, M, **_gw(mlp.fc2.weight), k_keep=dp_mlp, k_rows_per_group=rpg,
               alpha=alpha if dp_mlp is not None else 1.0, splits=K.splits_for(C, 4 * C, M, dp_mlp is not None), rowsum_a=G(mlp.fc2.bias))
        dh = K.gemm(0, dy, W16T(mlp.fc2.weight), M, 4 * C, C, gelu_in=h_pre, gelu_in_is_grad=_GQ, row_scale=dp_mlp,
                    rows_per_group=rpg, colsum=G(mlp.fc1.bias))
        dw_gemm(dh, y2, 4 * C, C, M, **_gw(mlp.fc1.weight), splits=K.splits_for(4 * C, C, M))
        d_y2 = K.gemm(0, dh, W16T(mlp.fc1.weight), M, C, 4 * C)
        del dh
        d_mid = ln_bwd(d_y2, x_mid, M, C, blk.norm2.weight.data, mean2, rstd2, G(blk.norm2.weight), G(blk.norm2.bias),
                                add_in=dy)
        # --- attention branch: x_mid = x + s * proj(attn(qkv(LN1(x)))) ---------------------------------
        dw_gemm(d_mid, ao, C, C, M, **_gw(a.proj.weight), k_keep=dp_attn, k_rows_per_group=rpg,
               alpha=alpha if dp_attn is not None else 1.0, splits=K.splits_for(C, C, M, dp_attn is not None), rowsum_a=G(a.proj.bias))
        d_ao = K.gemm(0, d_mid, W16T(a.proj.weight), M, C, C, row_scale=dp_attn, rows_per_group=rpg)
        dqkv = torch.empty_like(qkv)
        if pad is not None:
            # padded geometry: zero output-gradient rows for the padded tokens; their dK / dV (they ARE attended to) reach the
            # qkv bias through the row sum over all Ma rows, the weight sees nothing from them (their y1 rows are zero)
            d_ao, ao = K.gather_rows(d_ao, pad[2], Ma, C), ao_p
        if att.split_bias_grad and _DW_SIDE:
            # the relative-position-bias gradient is a parameter gradient: its kernel (it re-derives dS from qkv, dO, lse and
            # the -delta the dQ pass leaves behind the lse) runs on the weight-gradient stream, off the dy -> dx chain
            att.bwd(qkv, ao, d_ao, lse, dqkv, None)
            on_dw_stream(qkv.device, lambda: att.bwd_bias(qkv, d_ao, lse, G(a.relative_position_bias_table)), (qkv, d_ao, lse))
        else:
            att.bwd(qkv, ao, d_ao, lse, dqkv, G(a.relative_position_bias_table))
        dw_gemm(dqkv, y1, 3 * C, C, Ma, **_gw(a.qkv.weight), splits=K.splits_for(3 * C, C, Ma),
               rowsum_a=G(a.qkv.bias))
        d_y1 = K.gemm(0, dqkv, W16T(a.qkv.weight), Ma, C, 3 * C)
        if pad is not None:
            d_y1 = K.gather_rows(d_y1, pad[3], M, C)
        dx = ln_bwd(d_y1, x, M, C, blk.norm1.weight.data, mean1, rstd1, G(blk.norm1.weight), G(blk.norm1.bias),
                             add_in=d_mid)
        if ctx.notify and ctx.arena is not None:
            ctx.arena.notify(ctx.notify)                 # data-parallel reducer: this stage's gradient range is final
        return None, dx, None, None, None, None


class PatchMergeFn(torch.autograd.Function):
    """PatchMerging.forward (video_swin.py:271-287): 2x2 gather + LN(4C) + Linear(4C -> 2C, no bias)."""

    @staticmethod
    def forward(ctx, anchor, x, mod, BT, H, W):
        M, C = x.shape
        pad = None
        if H % 2 or W % 2:
            # odd H / W: one zero row / column at the far edge before the 2x2 gather (video_swin.py:273-276)
            pad = pad_maps(x.device, BT, (1, H, W), (1, 2, 2))
            (_, H, W), M, to_pad, _ = pad
            x = K.gather_rows(x, to_pad, M, C)
        rows = M // 4
        y, mean, rstd = K.layernorm_fwd(x, rows, 4 * C, mod.norm.weight.data, mod.norm.bias.data, 1e-5, gather=(H, W, C),
                                        want_stats=_keep(ctx))
        out = K.gemm(0, y, W16(mod.reduction.weight), rows, 2 * C, 4 * C)
        ctx.mod, ctx.geo, ctx.pad = mod, (H, W, C), pad
        ctx.save_for_backward(x, y, mean, rstd)
        return out

    @staticmethod
    def backward(ctx, dout):
        mod = ctx.mod
        H, W, C = ctx.geo
        x, y, mean, rstd = ctx.saved_tensors
        rows = y.shape[0]
        dout = dout.contiguous()
        dw_gemm(dout, y, 2 * C, 4 * C, rows, **_gw(mod.reduction.weight), splits=K.splits_for(2 * C, 4 * C, rows))
        d_y = K.gemm(0, dout, W16T(mod.reduction.weight), rows, 4 * C, 2 * C)
        dx = ln_bwd(d_y, x, rows, 4 * C, mod.norm.weight.data, mean, rstd, G(mod.norm.weight), G(mod.norm.bias),
                             gather=(H, W, C))
        if ctx.pad is not None:
            dx = K.gather_rows(dx, ctx.pad[3], len(ctx.pad[3]), C)
        return None, dx, None, None, None, None


class LayerNormFn(torch.autograd.Function):
    """Plain LayerNorm stage (SwinTransformer3D.norm, video_swin.py:476-478)."""

    @staticmethod
    def forward(ctx, anchor, x, mod, eps):
        M, C = x.shape
        y, mean, rstd = K.layernorm_fwd(x, M, C, mod.weight.data, mod.bias.data, eps, want_stats=_keep(ctx))
        ctx.mod = mod
        ctx.save_for_backward(x, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        mod = ctx.mod
        x, mean, rstd = ctx.saved_tensors
        M, C = x.shape
        dx = ln_bwd(dy.contiguous(), x, M, C, mod.weight.data, mean, rstd, G(mod.weight), G(mod.bias))
        return None, dx, None, None


# ---------------------------------------------------------------------------------------------------
# EncVideo tail / EncTxt
# ---------------------------------------------------------------------------------------------------
# ---- ONE source buffer for the fusion encoder: [video rows of every clip ; text rows of every text] -----------------------
# go_feat announces how many text rows follow (fusion_tail_hint); VideoEmbedFn then allocates B * Lv + tail rows, writes its rows at the top and
# leaves the buffer as "pending"; TextEmbedFn, when its n * X rows are exactly that tail, writes them behind.  feat_img / feat_txt are views of the
# one buffer, and JoinRowsFn hands the whole of it to the first fusion layer without the T.cat of model.py:235 (no copy forward, no split backward).
_fusion_tail = {"hint": 0, "pending": None}


def fusion_tail_hint(rows):
    _fusion_tail["hint"] = int(rows) if _FUSION_SRC else 0
    _fusion_tail["pending"] = None


def _claim_fusion_tail(rows, Hd, device):
    """the tail of the video rows' buffer when exactly `rows` rows of width Hd are pending on `device`, else None; nothing stays pending"""
    pend, _fusion_tail["pending"] = _fusion_tail["pending"], None
    if pend is not None and pend[2] == rows and pend[0].shape[1] == Hd and pend[0].device == device:
        return pend[0][pend[1]:]
    return None


class JoinRowsFn(torch.autograd.Function):
    """(a, b): adjacent row blocks of one buffer -> the (rows_a + rows_b, H) tensor over both, no copy; backward: the two slices of the gradient."""

    @staticmethod
    def forward(ctx, a, b):
        Hd = a.shape[-1]
        ra, rb = a.numel() // Hd, b.numel() // Hd
        ctx.sa, ctx.sb, ctx.ra = a.shape, b.shape, ra
        return a.new_empty(0).set_(a.untyped_storage(), a.storage_offset(), (ra + rb, Hd), (Hd, 1))

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        return g[:ctx.ra].view(ctx.sa), g[ctx.ra:].view(ctx.sb)


def rows_adjacent(a, b):
    """b's rows start where a's end, in the same storage (the layout VideoEmbedFn / TextEmbedFn produce under a fusion_tail_hint)"""
    return (a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype and a.shape[-1] == b.shape[-1] and
            a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and b.storage_offset() == a.storage_offset() + a.numel())


class VideoEmbedFn(torch.autograd.Function):
    """EncVideo.forward after the backbone (model.py:48-91): fc, cls/pos/len, LayerNorm."""

    @staticmethod
    def forward(ctx, anchor, tok, enc, B, T, hw):
        M, Cl = tok.shape
        Hd = enc.img_feature_dim
        if enc.fc is not None:
            feat = K.gemm(0, tok, W16(enc.fc.weight), M, Hd, Cl, bias=enc.fc.bias.data)
        else:
            feat = tok
        Lv = T * (1 + hw)
        tail = _fusion_tail["hint"]
        _fusion_tail["hint"] = 0
        buf = torch.empty((B * Lv + tail, Hd), dtype=bf16, device=tok.device)
        out = buf[:B * Lv].view(B, Lv, Hd)
        _fusion_tail["pending"] = (buf, B * Lv, tail) if tail else None
        mean, rstd = K.video_embed_fwd(feat, B, T, hw, Hd, enc.emb_cls.data, enc.emb_pos.data, enc.emb_len.data,
                                       enc.norm.weight.data, enc.norm.bias.data, 1e-5, out, Lv)
        ctx.enc, ctx.dims = enc, (B, T, hw)
        ctx.save_for_backward(tok, feat, mean, rstd)
        return out

    @staticmethod
    def backward(ctx, dout):
        enc = ctx.enc
        B, T, hw = ctx.dims
        tok, feat, mean, rstd = ctx.saved_tensors
        M, Cl = tok.shape
        Hd = enc.img_feature_dim
        # every fusion-layer / MLM-head gradient (MTM and VTM pass) is final here: let the data-parallel reducer start
        # their all-reduce under the video-encoder backward
        arena = enc._arena_of() if enc._arena_of is not None else None
        if arena is not None:
            arena.notify("fusion_grads_final")
        dout = dout.contiguous()
        dfeat = torch.empty((M, Hd), dtype=bf16, device=tok.device)
        K.video_embed_bwd(dout, T * (1 + hw), feat, B, T, hw, Hd, enc.emb_cls.data, enc.emb_pos.data, enc.emb_len.data,
                          enc.norm.weight.data, mean, rstd, dfeat, G(enc.emb_cls), G(enc.emb_pos), G(enc.emb_len),
                          G(enc.norm.weight), G(enc.norm.bias))
        if enc.fc is None:
            return None, dfeat, None, None, None, None
        dw_gemm(dfeat, tok, Hd, Cl, M, **_gw(enc.fc.weight), splits=K.splits_for(Hd, Cl, M),
               rowsum_a=G(enc.fc.bias))
        dtok = K.gemm(0, dfeat, W16T(enc.fc.weight), M, Cl, Hd)
        return None, dtok, None, None, None, None


class TextEmbedFn(torch.autograd.Function):
    """BertEmbeddings as used by EncTxt.forward (model.py:125-129)."""

    @staticmethod
    def forward(ctx, anchor, ids, emb, dropout_p):
        n, X = ids.shape
        Hd = emb.word_embeddings.weight.shape[1]
        ids = ids.contiguous()
        seed = K.next_seed()
        out = _claim_fusion_tail(n * X, Hd, ids.device)
        out, mean, rstd = K.text_embed_fwd(ids, n, X, Hd, emb.word_embeddings.weight.data, emb.position_embeddings.weight.data,
                                           emb.token_type_embeddings.weight.data, emb.LayerNorm.weight.data,
                                           emb.LayerNorm.bias.data, emb.LayerNorm.eps, dropout_p, seed, out=out)
        ctx.emb, ctx.p, ctx.seed = emb, dropout_p, seed
        ctx.save_for_backward(ids, mean, rstd)
        return out.view(n, X, Hd)

    @staticmethod
    def backward(ctx, dout):
        emb = ctx.emb
        ids, mean, rstd = ctx.saved_tensors
        n, X = ids.shape
        Hd = emb.word_embeddings.weight.shape[1]
        dout = dout.contiguous()
        args = (ids, dout, n, X, Hd, emb.word_embeddings.weight.data, emb.position_embeddings.weight.data,
                emb.token_type_embeddings.weight.data, emb.LayerNorm.weight.data, mean, rstd, ctx.p, ctx.seed,
                G(emb.word_embeddings.weight), G(emb.position_embeddings.weight), G(emb.token_type_embeddings.weight),
                G(emb.LayerNorm.weight), G(emb.LayerNorm.bias))
        # Only parameter gradients come out of this kernel, so it runs on the WEIGHT-GRADIENT stream: the word-embedding gradient is also
        # written by the tied decoder's weight-gradient GEMM there (an assign when it is the step's first writer, a read-modify-write otherwise)
        # and the stream's FIFO order puts these atomics behind it.  (Autograd runs this node right after the fusion backward, before the
        # Swin backward: making the MAIN stream wait for the weight-gradient stream here stalled it for 0.6 ms per step.)
        on_dw_stream(dout.device, lambda: K.text_embed_bwd(*args), (ids, dout, mean, rstd))
        return None, None, None, None


class PreTextEmbedFn(torch.autograd.Function):
    """TextEmbedFn behind a pre-text segment (get_pretxt / prepro_txt_inputs, model.py:250-307): (n, Lp + X, H) rows [pre-text ; text] from
    ONE kernel (lav_text_embed_pre_fwd) -- under a fusion_tail_hint of n * (Lp + X) rows they land behind the video rows, so video, pre-text
    and text stay one buffer.  The pre-text is either
      task = (emb_task, row): the task token, read in place from the arena's bf16 copy of that row; its gradient (the sum over the n texts,
             fixed-order fp32) is accumulated straight into G(emb_task)[row];
      pre: the bf16 (1, Lp, H) (broadcast) or (n, Lp, H) (a block per text) prompt features, an autograd input: its gradient is returned as
             bf16 rows to the prompt's own TextEmbedFn.
    The text rows are bit-identical to TextEmbedFn's for the same ids and seed."""

    @staticmethod
    def forward(ctx, anchor, ids, emb, dropout_p, pre, task):
        n, X = ids.shape
        Hd = emb.word_embeddings.weight.shape[1]
        ids = ids.contiguous()
        if task is not None:
            param, row = task
            Lp, stride, src = 1, 0, W16(param)[row]
        else:
            Lp = pre.shape[-2]
            src = pre.contiguous()
            stride = 0 if src.shape[0] == 1 else Lp * Hd
            assert src.dtype == bf16 and src.shape[-1] == Hd and src.shape[0] in (1, n), (tuple(src.shape), n)
        seed = K.next_seed()
        out = _claim_fusion_tail(n * (Lp + X), Hd, ids.device)
        out, mean, rstd = K.text_embed_pre_fwd(ids, n, Lp, X, Hd, emb.word_embeddings.weight.data, emb.position_embeddings.weight.data,
                                               emb.token_type_embeddings.weight.data, emb.LayerNorm.weight.data, emb.LayerNorm.bias.data,
                                               emb.LayerNorm.eps, dropout_p, seed, src, stride, out=out)
        ctx.emb, ctx.p, ctx.seed, ctx.task, ctx.pre_meta = emb, dropout_p, seed, task, (Lp, stride, None if pre is None else tuple(src.shape))
        ctx.save_for_backward(ids, mean, rstd)
        return out.view(n, Lp + X, Hd)

    @staticmethod
    def backward(ctx, dout):
        emb = ctx.emb
        ids, mean, rstd = ctx.saved_tensors
        n, X = ids.shape
        Lp, stride, pre_shape = ctx.pre_meta
        Hd = emb.word_embeddings.weight.shape[1]
        dout = dout.contiguous()
        if ctx.task is not None:
            param, row = ctx.task
            d_pre, mode = G(param)[row], 0                     # G: a first-touch unit is made valid zero before this accumulate
        else:
            d_pre, mode = torch.empty(pre_shape, dtype=bf16, device=dout.device), 1
        args = (ids, dout, n, Lp, X, Hd, emb.word_embeddings.weight.data, emb.position_embeddings.weight.data,
                emb.token_type_embeddings.weight.data, emb.LayerNorm.weight.data, mean, rstd, ctx.p, ctx.seed,
                G(emb.word_embeddings.weight), G(emb.position_embeddings.weight), G(emb.token_type_embeddings.weight),
                G(emb.LayerNorm.weight), G(emb.LayerNorm.bias), stride, d_pre, mode)
        # the stream placement of TextEmbedFn.backward (see there).  A prompt's d_pre is written on the weight-gradient stream too; its one
        # reader is the prompt's own TextEmbedFn.backward, which runs on that stream after this kernel (FIFO order).
        on_dw_stream(dout.device, lambda: K.text_embed_pre_bwd(*args), (ids, dout, mean, rstd, d_pre))
        return None, None, None, None, (d_pre if ctx.task is None else None), None


class TaskRowFn(torch.autograd.Function):
    """The task-token row emb_task[row] as bf16 (1, H) features for a caller that concatenates it itself (features that did not come from
    go_feat); the backward sums the incoming rows into G(emb_task)[row] (lav_colsum_bf16)."""

    @staticmethod
    def forward(ctx, anchor, param, row):
        ctx.param, ctx.row = param, row
        return W16(param)[row:row + 1].clone()

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        Hd = dy.shape[-1]
        K.colsum(dy.view(-1, Hd), dy.numel() // Hd, Hd, G(ctx.param)[ctx.row])
        return None, None, None


def pair_index(B, Lv, nt, X, vi, ti):
    """(n, L) int32 map: row r of pair k's sequence [video rows of clip vi[k] | text rows of text ti[k]] -> row of the un-expanded
    source [B * Lv video rows ; nt * X text rows] (T.cat at model.py:235 over the pair list of main_pretrain_mlm.py:74-111 /
    main_retrieval_mlm.py:62-87)."""
    vi = np.asarray(vi, dtype=np.int64)
    ti = np.asarray(ti, dtype=np.int64)
    idx = np.empty((len(vi), Lv + X), dtype=np.int32)
    idx[:, :Lv] = vi[:, None] * Lv + np.arange(Lv)[None, :]
    idx[:, Lv:] = B * Lv + ti[:, None] * X + np.arange(X)[None, :]
    return idx


def pair_csr(flat, n_src):
    """inverse of a pair map as (start, order): source row u is read by the pair rows order[start[u]:start[u + 1]]"""
    order = np.argsort(flat, kind="stable").astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_src))]).astype(np.int32)
    return start, order


def pair_fused_ok(Hd):
    return PAIR_FUSED and Hd % 64 == 0 and (3 * Hd) % 256 == 0


class PairSeqFn(torch.autograd.Function):
    """Builds the fusion input [video rows of sample vi | text rows of sample ti] for every pair
    (T.cat at model.py:235 + the pair list of main_pretrain_mlm.py:74-111) with one row-gather kernel;
    the backward is one gather-sum kernel over the inverse (CSR) map."""

    @staticmethod
    def forward(ctx, f_img, f_txt, vi, ti):
        B, Lv, Hd = f_img.shape
        nt, X = f_txt.shape[0], f_txt.shape[1]             # nt == B on the pre-training path, B * O texts for retrieval multiple choice
        n = len(vi)
        L = Lv + X
        dev = f_img.device
        src = torch.cat([f_img.reshape(B * Lv, Hd), f_txt.reshape(nt * X, Hd)], 0)
        flat = pair_index(B, Lv, nt, X, vi, ti).reshape(-1)
        out = K.gather_rows(src, torch.from_numpy(flat).to(dev, non_blocking=True), n * L, Hd)
        if _keep(ctx):
            start, order = pair_csr(flat, B * Lv + nt * X)
            ctx.csr = (torch.from_numpy(start).to(dev, non_blocking=True), torch.from_numpy(order).to(dev, non_blocking=True))
            ctx.meta = (B, Lv, X, Hd, n, nt)
        return out.view(n, L, Hd)

    @staticmethod
    def backward(ctx, dout):
        B, Lv, X, Hd, n, nt = ctx.meta
        start, order = ctx.csr
        d = K.gather_sum_rows(dout.contiguous().view(n * (Lv + X), Hd), start, order, B * Lv + nt * X, Hd)
        return d[:B * Lv].view(B, Lv, Hd), d[B * Lv:].view(nt, X, Hd), None, None


class RowGatherFn(torch.autograd.Function):
    """rows[idx] of a (R, C) tensor with distinct indices (the supervised positions of the loss-aware MLM head); the
    backward is the same gather kernel over the inverse map (unselected rows read as zero)."""

    @staticmethod
    def forward(ctx, src, idx):
        R, C = src.shape
        idx = np.asarray(idx, dtype=np.int32)
        out = K.gather_rows(src, torch.from_numpy(idx).to(src.device, non_blocking=True), len(idx), C)
        if ctx.needs_input_grad[0]:
            inv = np.full(R, -1, dtype=np.int32)
            inv[idx] = np.arange(len(idx), dtype=np.int32)
            ctx.inv = torch.from_numpy(inv).to(src.device, non_blocking=True)
            ctx.shape = (R, C)
        return out

    @staticmethod
    def backward(ctx, dy):
        R, C = ctx.shape
        return K.gather_rows(dy.contiguous(), ctx.inv, R, C), None


# ---------------------------------------------------------------------------------------------------
# fusion encoder layer / MLM head / loss
# ---------------------------------------------------------------------------------------------------
# ---- lav_bert_layer_desc / lav_bert_layer_bwd_desc: values labelled by field name, placed by K.BL_FWD / K.BL_BWD -----------------------
_BL_PARAMS = ("w_qkv", "b_qkv", "w_ao", "b_ao", "ln1_gamma", "ln1_beta", "w_ff1", "b_ff1", "w_ff2", "b_ff2", "ln2_gamma", "ln2_beta")
_BL_FWD_NAMES = ("n_seq", "L", "hidden", "heads", "ffn", "p_hidden", "p_attn", "ln_eps", "seed_attn", "seed1", "seed2", "causal_from", "stream_f16",
                 "ln2_eps") + _BL_PARAMS + ("key_mask", "x", "res_pre", "res_mean", "res_rstd", "res_gamma", "res_beta", "qkv", "cx", "lse", "pre1",
                                            "mean1", "rstd1", "x1", "h_pre", "h", "pre2", "mean2", "rstd2", "y")
_BL_BWD_CONSTS = ("wt_qkv", "wt_ao", "wt_ff1", "wt_ff2", "ldt_qkv", "ldt_ao", "ldt_ff1", "ldt_ff2", "g_w_qkv", "g_b_qkv", "g_w_ao", "g_b_ao",
                  "g_ln1_gamma", "g_ln1_beta", "g_w_ff1", "g_b_ff1", "g_w_ff2", "g_b_ff2", "g_ln2_gamma", "g_ln2_beta")
_BL_BWD_NAMES = _BL_FWD_NAMES + ("dy",) + _BL_BWD_CONSTS + ("splits_qkv", "splits_ao", "splits_ff1", "splits_ff2") + (
    "d_pre2", "d_dense2", "dh", "d_x1", "d_pre1", "d_dense1", "d_cx", "dqkv", "dx", "group_splits", "assign_mask")
_BL_FWD_PLACE, _BL_BWD_PLACE = K.BL_FWD.placer(_BL_FWD_NAMES), K.BL_BWD.placer(_BL_BWD_NAMES)


def _layer_consts(layer):
    """What both paths of a fusion layer need of its parameters, cached on the layer per arena (arena views: fixed for the arena's life):
    `params` (labelled _BL_PARAMS; also the parameter run of lav_bert_layer_rows_desc) and `bwd` (labelled _BL_BWD_CONSTS), the device addresses
    of the parameters / the transposed copies and gradient accumulators, and the fused q | k | v views wqkv16, bqkv, gwqkv, gbqkv as tensors."""
    arena = layer._arena()
    c = layer.__dict__.get("_lav_stage_consts")
    if c is not None and c[0] is arena:
        return c[1]
    att_m, ao, inter, outp = layer.attention.self, layer.attention.output, layer.intermediate, layer.output
    Hd = att_m.query.weight.shape[1]
    wqkv16, gwqkv, _ = arena.fused_view(att_m.query.weight, 3 * Hd)
    _, gbqkv, bqkv = arena.fused_view(att_m.query.bias, 3 * Hd)
    mats = (att_m.query.weight, ao.dense.weight, inter.dense.weight, outp.dense.weight)
    params = (wqkv16, bqkv, W16(ao.dense.weight), ao.dense.bias.data, ao.LayerNorm.weight.data, ao.LayerNorm.bias.data, W16(inter.dense.weight),
              inter.dense.bias.data, W16(outp.dense.weight), outp.dense.bias.data, outp.LayerNorm.weight.data, outp.LayerNorm.bias.data)
    grads = [gwqkv, gbqkv] + [GR(p) for p in (ao.dense.weight, ao.dense.bias, ao.LayerNorm.weight, ao.LayerNorm.bias, inter.dense.weight,
                                              inter.dense.bias, outp.dense.weight, outp.dense.bias, outp.LayerNorm.weight, outp.LayerNorm.bias)]
    assert len(params) == len(_BL_PARAMS) and 2 * len(mats) + len(grads) == len(_BL_BWD_CONSTS)
    return _stage_consts(layer, arena, params, [W16T(p) for p in mats], grads, eps=float(ao.LayerNorm.eps), eps2=float(outp.LayerNorm.eps),
                         ffn=inter.dense.weight.shape[0], heads=layer.num_heads, wqkv16=wqkv16, bqkv=bqkv, gwqkv=gwqkv, gbqkv=gbqkv)


def _bert_fwd_values(head, key_mask, resln_t, x, qkv, cx, lse, pre1, st1, x1, h_pre, h, pre2, st2, y_ptr):
    """lav_bert_layer_desc, labelled _BL_FWD_NAMES.  head: the scalars, seeds and parameter addresses; resln_t: (pre, mean, rstd, gamma, beta) of
    the LayerNorm that produced x, or None; st1 / st2: the (2, R) statistics (mean, rstd) of the layer's two LayerNorms.  Called on the fresh
    tensors (forward, eval) and on the unpacked saved ones (backward)."""
    dp = K._dp
    (mean1, rstd1), (mean2, rstd2) = _stat_rows(st1, 2), _stat_rows(st2, 2)
    return head + (dp(key_mask), x.data_ptr()) + (tuple(t.data_ptr() for t in resln_t) if resln_t is not None else (0, 0, 0, 0, 0)) + (
        qkv.data_ptr(), cx.data_ptr(), dp(lse), pre1.data_ptr(), mean1, rstd1, x1.data_ptr(), dp(h_pre), h.data_ptr(), pre2.data_ptr(), mean2, rstd2,
        y_ptr)


class BertLayerFn(torch.autograd.Function):
    """One post-LN BertLayer of the fusion encoder (HF BertLayer as called from model.py:242)."""

    @staticmethod
    def forward(ctx, anchor, x, x32, layer, key_mask, n, L, p_hidden, p_attn, want32, causal_from=0, pair=None):
        """x: (R, H) bf16 layer input (GEMM operand); x32: its fp32 copy for the residual add, or None (first layer:
        the embeddings are bf16); returns (y bf16, y32 fp32 or None when want32 is false).
        pair = (rowmap, start, order) (first layer only): x holds the UN-EXPANDED rows [video rows of every clip ; text rows of
        every text] and row r of the n * L pair rows is x[rowmap[r]] -- the QKV GEMM and the residual add read x through the map,
        the (n, L, H) expansion of main_retrieval_mlm.py:62-87 / main_pretrain_mlm.py:74-111 never exists; (start, order) is the
        map's inverse for the backward.
        With RESLN, x32 is not an fp32 tensor but the tuple (pre, mean, rstd, gamma, beta) of the LayerNorm that produced x, and
        the second return value is that tuple for this layer's output LayerNorm (pre2, mean2, rstd2 as extra non-differentiable
        outputs -- see model._encode)."""
        Hd = x.shape[1]
        R = n * L
        # the extra outputs (pre2 / mean2 / rstd2 or y32) are non-differentiable carriers: without this autograd hands the backward a
        # zero-filled tensor for each of them -- 36 fills per step, twelve of them 138 MB (0.5 ms per step in the r03 kernel trace)
        ctx.set_materialize_grads(False)
        rowmap = pair[0] if pair is not None else None
        assert pair is not None or x.shape[0] == R
        sdt = STREAM_DT if STREAM32 else bf16
        heads = layer.num_heads
        c = _layer_consts(layer)
        keep = _keep(ctx)
        resln_t = x32 if isinstance(x32, tuple) else None          # (pre, mean, rstd, gamma, beta) of the producing LayerNorm
        if STAGE_C and RESLN and _GQ == 1 and pair is None and (x32 is None or resln_t is not None):
            return BertLayerFn._forward_c(ctx, x, resln_t, layer, c, key_mask, n, L, p_hidden, p_attn, want32, causal_from, keep)
        qkv = K.gemm(0, x, c["wqkv16"], R, 3 * Hd, Hd, bias=c["bqkv"], a_rowmap=rowmap)
        s_att, s1, s2 = K.next_seed(), K.next_seed(), K.next_seed()
        att = K.Attn(1, heads, Hd // heads, n_seq=n, L=L, key_mask=key_mask, dropout_p=p_attn, seed=s_att, causal_from=int(causal_from))
        lse = torch.empty(att.lse_elems(), dtype=torch.float32, device=x.device) if keep else None
        cx = torch.empty((R, Hd), dtype=bf16, device=x.device)
        att.fwd(qkv, cx, lse)
        ao = layer.attention.output
        pre1 = K.gemm(0, cx, W16(ao.dense.weight), R, Hd, Hd, bias=ao.dense.bias.data, dropout_p=p_hidden, seed=s1,
                      residual=(resln_t[0] if resln_t is not None else (x32 if x32 is not None else x)), res_rowmap=rowmap,
                      res_ln=(resln_t[1:] if resln_t is not None else None), out_dtype=sdt)
        x1_32 = torch.empty((R, Hd), dtype=torch.float32, device=x.device) if (STREAM32 and not RESLN) else None
        x1, mean1, rstd1 = K.layernorm_fwd(pre1, R, Hd, ao.LayerNorm.weight.data, ao.LayerNorm.bias.data, ao.LayerNorm.eps,
                                           want_stats=keep or RESLN, out32=x1_32)
        inter, outp = layer.intermediate, layer.output
        F = inter.dense.weight.shape[0]
        h_pre = torch.empty((R, F), dtype=_GQ_DT, device=x.device) if keep else None
        h = K.gemm(0, x1, W16(inter.dense.weight), R, F, Hd, bias=inter.dense.bias.data, act=1, preact=h_pre, preact_is_grad=_GQ)
        pre2 = K.gemm(0, h, W16(outp.dense.weight), R, Hd, F, bias=outp.dense.bias.data, dropout_p=p_hidden, seed=s2,
                      residual=(pre1 if RESLN else (x1_32 if STREAM32 else x1)),
                      res_ln=((mean1, rstd1, ao.LayerNorm.weight.data, ao.LayerNorm.bias.data) if RESLN else None), out_dtype=sdt)
        y32 = torch.empty((R, Hd), dtype=torch.float32, device=x.device) if (STREAM32 and want32 and not RESLN) else None
        y, mean2, rstd2 = K.layernorm_fwd(pre2, R, Hd, outp.LayerNorm.weight.data, outp.LayerNorm.bias.data, outp.LayerNorm.eps,
                                          want_stats=keep or (RESLN and want32), out32=y32)
        if keep:
            ctx.layer, ctx.att, ctx.seeds, ctx.p = layer, att, (s1, s2), p_hidden
            ctx.pair, ctx.c_consts = pair, c                  # c_consts: the FORWARD's constants (the cache may be rebuilt before the backward)
            ctx.save_for_backward(x, qkv, cx, lse, pre1, mean1, rstd1, x1, h_pre, h, pre2, mean2, rstd2)
        if RESLN and want32:
            ctx.mark_non_differentiable(pre2, mean2, rstd2)
            return y, pre2, mean2, rstd2
        ctx.mark_non_differentiable(*([y32] if y32 is not None else []))
        return y, y32

    @staticmethod
    def _launch_c(x, resln_t, c, key_mask, n, L, p_hidden, p_attn, seeds, causal_from, keep):
        """allocate one layer's activations and enqueue lav_bert_layer_fwd on them: (descriptor head, (qkv, cx, lse, pre1, st1, x1, h_pre, h,
        pre2, st2, y)).  st1 / st2 = (mean, rstd) of the two LayerNorms; lse and h_pre exist only when `keep`."""
        Hd, R, F = x.shape[1], n * L, c["ffn"]
        dev, f32, e = x.device, torch.float32, torch.empty
        qkv, cx, x1, h, y = e((R, 3 * Hd), dtype=bf16, device=dev), e((R, Hd), dtype=bf16, device=dev), e((R, Hd), dtype=bf16, device=dev), \
            e((R, F), dtype=bf16, device=dev), e((R, Hd), dtype=bf16, device=dev)
        pre1, pre2 = e((R, Hd), dtype=STREAM_DT, device=dev), e((R, Hd), dtype=STREAM_DT, device=dev)
        st1, st2 = e((2, R), dtype=f32, device=dev), e((2, R), dtype=f32, device=dev)          # (mean, rstd) of the two LayerNorms
        lse = h_pre = None
        if keep:
            att = K.Attn(1, c["heads"], Hd // c["heads"], n_seq=n, L=L, key_mask=key_mask, dropout_p=p_attn, seed=seeds[0], causal_from=int(causal_from))
            lse = e(att.lse_elems(), dtype=f32, device=dev)
            h_pre = e((R, F), dtype=bf16, device=dev)
        head = (n, L, Hd, c["heads"], F, float(p_hidden), float(p_attn), c["eps"]) + tuple(seeds) + (
            int(causal_from), int(STREAM_DT == torch.float16), c["eps2"]) + c["params"]
        K.bert_layer_fwd(_BL_FWD_PLACE(_bert_fwd_values(head, key_mask, resln_t, x, qkv, cx, lse, pre1, st1, x1, h_pre, h, pre2, st2, y.data_ptr())))
        return head, (qkv, cx, lse, pre1, st1, x1, h_pre, h, pre2, st2, y)

    @staticmethod
    def _forward_c(ctx, x, resln_t, layer, c, key_mask, n, L, p_hidden, p_attn, want32, causal_from, keep):
        """the same seven launches as the per-kernel path below, enqueued by ONE call of lav_bert_layer_fwd"""
        assert x.shape[0] == n * L and x.is_contiguous()
        s_att, s1, s2 = K.next_seed(), K.next_seed(), K.next_seed()
        head, (qkv, cx, lse, pre1, st1, x1, h_pre, h, pre2, st2, y) = BertLayerFn._launch_c(
            x, resln_t, c, key_mask, n, L, p_hidden, p_attn, (s_att, s1, s2), causal_from, keep)
        if keep:
            ctx.layer, ctx.seeds, ctx.p, ctx.pair = layer, (s1, s2), p_hidden, None
            # the backward rebuilds the activation addresses from the UNPACKED saved tensors (saved-tensor hooks may move them); kept from
            # here: the descriptor head, gamma / beta of the residual carrier (parameters), the address of y (never read by the backward) and
            # c_consts, the FORWARD's constants (not re-queried in the backward: the cache may have been rebuilt since)
            ctx.c_stage, ctx.c_head, ctx.c_res_gb, ctx.c_y, ctx.c_consts = True, head, (resln_t[3:] if resln_t is not None else None), y.data_ptr(), c
            ctx.save_for_backward(x, qkv, cx, lse, pre1, st1, x1, h_pre, h, pre2, st2, key_mask if key_mask is not None else x.new_empty(0),
                                  *(resln_t[:3] if resln_t is not None else ()))
        if want32:
            mean2, rstd2 = st2[0], st2[1]
            ctx.mark_non_differentiable(pre2, mean2, rstd2)
            return y, pre2, mean2, rstd2
        return y, None

    @staticmethod
    def _backward_c(ctx, dy):
        layer = ctx.layer
        x, qkv, cx, lse, pre1, st1, x1, h_pre, h, pre2, st2, key_mask, *res = ctx.saved_tensors
        key_mask = key_mask if key_mask.numel() else None
        resln_t = tuple(res) + tuple(ctx.c_res_gb) if res else None
        c, dev, e = ctx.c_consts, x.device, torch.empty
        (R, Hd), F = cx.shape, c["ffn"]
        d_pre2, d_dense2, d_x1, d_pre1, d_dense1, d_cx, dx = (e((R, Hd), dtype=bf16, device=dev) for _ in range(7))
        dh, dqkv = e((R, F), dtype=bf16, device=dev), e((R, 3 * Hd), dtype=bf16, device=dev)
        splits = (K.splits_for(3 * Hd, Hd, R), K.splits_for(Hd, Hd, R), K.splits_for(F, Hd, R), K.splits_for(Hd, F, R))
        gs = K.group_splits_for(((Hd, F), (F, Hd), (Hd, Hd), (3 * Hd, Hd)), R)
        am = (layer.output.dense.weight, layer.intermediate.dense.weight, layer.attention.output.dense.weight, layer.attention.self.query.weight)
        fwd = _bert_fwd_values(ctx.c_head, key_mask, resln_t, x, qkv, cx, lse, pre1, st1, x1, h_pre, h, pre2, st2, ctx.c_y)
        fields = _BL_BWD_PLACE(fwd + (dy.data_ptr(),) + c["bwd"] + splits + tuple(
            t.data_ptr() for t in (d_pre2, d_dense2, dh, d_x1, d_pre1, d_dense1, d_cx, dqkv, dx)) + (gs, _assign_mask(am)))     # labelled _BL_BWD_NAMES
        _stage_bwd(K.bert_layer_bwd, fields, ((3 * Hd, Hd), (Hd, Hd), (F, Hd), (Hd, F)), R, None, dev, (d_dense2, h, dh, x1, d_dense1, cx, dqkv, x))
        return None, dx, None, None, None, None, None, None, None, None, None, None

    @staticmethod
    def backward(ctx, dy, *_unused):
        if dy is None:                                     # nothing downstream used the layer output (grads are not materialised, see forward)
            return (None,) * 12
        if getattr(ctx, "c_stage", False):
            return BertLayerFn._backward_c(ctx, dy.contiguous())
        layer, att, (s1, s2), p = ctx.layer, ctx.att, ctx.seeds, ctx.p
        x, qkv, cx, lse, pre1, mean1, rstd1, x1, h_pre, h, pre2, mean2, rstd2 = ctx.saved_tensors
        R, Hd = cx.shape
        att_m, ao, inter, outp = layer.attention.self, layer.attention.output, layer.intermediate, layer.output
        F = inter.dense.weight.shape[0]
        dy = dy.contiguous()
        # out = LN(pre2), pre2 = x1 + dropout(dense(h))
        d_dense2 = torch.empty((R, Hd), dtype=bf16, device=x.device)
        d_pre2 = ln_bwd(dy, pre2, R, Hd, outp.LayerNorm.weight.data, mean2, rstd2, G(outp.LayerNorm.weight),
                                 G(outp.LayerNorm.bias), dx2=d_dense2, dropout_p=p, seed=s2, colsum=G(outp.dense.bias))
        grp = DwGroup(((Hd, F), (F, Hd), (Hd, Hd), (3 * Hd, Hd)), R)      # the layer's four weight gradients: one grouped launch at the end
        grp.add(d_dense2, h, Hd, F, R, GW(outp.dense.weight), K.splits_for(Hd, F, R))
        dh = K.gemm(0, d_dense2, W16T(outp.dense.weight), R, F, Hd, gelu_in=h_pre, gelu_in_is_grad=_GQ, colsum=G(inter.dense.bias))
        grp.add(dh, x1, F, Hd, R, GW(inter.dense.weight), K.splits_for(F, Hd, R))
        d_x1 = K.gemm(0, dh, W16T(inter.dense.weight), R, Hd, F, residual=d_pre2)
        del dh
        # x1 = LN(pre1), pre1 = x + dropout(dense(ctx))
        d_dense1 = torch.empty_like(d_dense2) if _DW_SIDE else d_dense2     # the side stream may still read d_dense2
        d_pre1 = ln_bwd(d_x1, pre1, R, Hd, ao.LayerNorm.weight.data, mean1, rstd1, G(ao.LayerNorm.weight),
                                 G(ao.LayerNorm.bias), dx2=d_dense1, dropout_p=p, seed=s1, colsum=G(ao.dense.bias))
        grp.add(d_dense1, cx, Hd, Hd, R, GW(ao.dense.weight), K.splits_for(Hd, Hd, R))
        d_cx = K.gemm(0, d_dense1, W16T(ao.dense.weight), R, Hd, Hd)
        dqkv = torch.empty_like(qkv)
        att.bwd(qkv, cx, d_cx, lse, dqkv, None)
        rows = x.shape[0]                                  # R, or with a pair map the U un-expanded source rows
        if ctx.pair is not None:
            # every pair row that read source row u sends its gradient back to u: sum the pair rows first (one gather-sum each
            # for dqkv and the residual branch), then the weight gradient and the input gradient run on the U source rows
            _, start, order = ctx.pair
            dqkv = K.gather_sum_rows(dqkv, start, order, rows, 3 * Hd)
            d_pre1 = K.gather_sum_rows(d_pre1, start, order, rows, Hd)
        c = ctx.c_consts
        grp.add(dqkv, x, 3 * Hd, Hd, rows, (c["gwqkv"], GW(att_m.query.weight)[1]), K.splits_for(3 * Hd, Hd, rows), rowsum_a=c["gbqkv"])
        grp.launch(x.device)
        dx = K.gemm(0, dqkv, W16T(att_m.query.weight), rows, Hd, 3 * Hd, residual=d_pre1)
        return None, dx, None, None, None, None, None, None, None, None, None, None


def bert_layer_eval_c(x, resln_t, layer, key_mask, n, L):
    """BertLayerFn._forward_c at eval (no dropout, nothing kept, causal_from 0, no seeds drawn), returning the layer's qkv too:
    (y, (pre2, mean2, rstd2, gamma2, beta2) for the next layer's residual, qkv).  The prefix pass of caption decoding (caption_decode.py)."""
    assert x.shape[0] == n * L and x.is_contiguous()
    _, (qkv, _, _, _, _, _, _, _, pre2, st2, y) = BertLayerFn._launch_c(x, resln_t, _layer_consts(layer), key_mask, n, L, 0.0, 0.0, (0, 0, 0), 0, False)
    out = layer.output.LayerNorm
    return y, (pre2, st2[0], st2[1], out.weight.data, out.bias.data), qkv


def bert_layer_rows_eval(x, x32, layer, key_mask, n, L, q_row, res_rowmap, x_rowmap=None):
    """The last fusion layer of the retrieval pair scorer (lav_bert_layer_fwd_rows): BertLayerFn's eval arithmetic with everything after the QKV
    GEMM on row q_row[s] of every sequence s.  x / x32 are what model._encode hands the layer: x the bf16 input (n * L rows, or the un-expanded
    pair source read through x_rowmap), x32 None (residual = x), an fp32 tensor, or RESLN's (pre, mean, rstd, gamma, beta).  res_rowmap (n,)
    int32: the residual row of each selected row.  Returns (y bf16, y32 fp32), both (n, H)."""
    Hd, dev, f32, e, dp = x.shape[1], x.device, torch.float32, torch.empty, K._dp
    c = _layer_consts(layer)
    F = c["ffn"]
    if isinstance(x32, tuple):
        res, (rm, rr, rg, rb) = x32[0], x32[1:]
    else:
        res, rm, rr, rg, rb = (x32 if x32 is not None else x), None, None, None, None
    res_dtype = {bf16: 0, f32: 1, torch.float16: 2}[res.dtype]
    qkv = e((n * L, 3 * Hd), dtype=bf16, device=dev)
    cx, x1, y = (e((n, Hd), dtype=bf16, device=dev) for _ in range(3))
    pre1, pre2, y32 = (e((n, Hd), dtype=f32, device=dev) for _ in range(3))
    st = e((4, n), dtype=f32, device=dev)
    h = e((n, F), dtype=bf16, device=dev)
    # lav_bert_layer_rows_desc declares the twelve parameter addresses in the order of _BL_PARAMS
    d = K.L.BertLayerRowsDesc(n, L, Hd, c["heads"], F, c["eps"], c["eps2"], dp(key_mask), dp(q_row), *c["params"], dp(x), dp(x_rowmap), dp(res),
                              K._ld(res), res_dtype, dp(res_rowmap), dp(rm), dp(rr), dp(rg), dp(rb), dp(qkv), dp(cx), dp(pre1), dp(st[0]), dp(st[1]),
                              dp(x1), dp(h), dp(pre2), dp(st[2]), dp(st[3]), dp(y), dp(y32))
    K.bert_layer_fwd_rows(d)
    return y, y32


class MLMHeadFn(torch.autograd.Function):
    """BertOnlyMLMHead (main_pretrain_mlm.py:46-48,69,115): dense+GELU, LayerNorm, vocab projection."""

    @staticmethod
    def forward(ctx, anchor, x, head, split=None):
        """split = n0: x is (n, X, H) holding two groups of sequences (the MTM and the VTM pairs run through the encoder as one
        batch); returns the logits of x[:n0] and x[n0:] as two views of ONE buffer, so that each loss can overwrite its part
        with its gradient in place and the backward below still sees a single (rows, vocab) operand."""
        shp = x.shape
        Hd = shp[-1]
        x2 = x.reshape(-1, Hd).contiguous()
        R = x2.shape[0]
        tr, dec = head.predictions.transform, head.predictions.decoder
        V = dec.weight.shape[0]
        keep = _keep(ctx)
        t_pre = torch.empty((R, Hd), dtype=bf16, device=x.device) if keep else None
        t = K.gemm(0, x2, W16(tr.dense.weight), R, Hd, Hd, bias=tr.dense.bias.data, act=1, preact=t_pre)
        tn, mean, rstd = K.layernorm_fwd(t, R, Hd, tr.LayerNorm.weight.data, tr.LayerNorm.bias.data, tr.LayerNorm.eps,
                                         want_stats=keep)
        ld = (V + 7) // 8 * 8
        buf = torch.empty((R, ld), dtype=bf16, device=x.device)
        K.gemm(0, tn, W16(dec.weight), R, V, Hd, out=buf, bias=dec.bias.data, c_pad_writable=True)   # the 6 padding columns of buf are never read as logits
        ctx.head, ctx.shp, ctx.split = head, shp, split
        ctx.save_for_backward(x2, t_pre, t, mean, rstd, tn)
        if split is None:
            return buf[:, :V].view(*shp[:-1], V)
        assert x.dim() == 3 and 0 < split < shp[0]
        r0 = split * shp[1]
        ctx.buf = buf if keep else None
        return buf[:r0, :V].view(split, shp[1], V), buf[r0:, :V].view(shp[0] - split, shp[1], V)

    @staticmethod
    def backward(ctx, dlogits, dlogits_b=None):
        head = ctx.head
        x2, t_pre, t, mean, rstd, tn = ctx.saved_tensors
        R, Hd = x2.shape
        tr, dec = head.predictions.transform, head.predictions.decoder
        V = dec.weight.shape[0]
        ld = (V + 7) // 8 * 8
        if ctx.split is not None:
            buf, r0 = ctx.buf, ctx.split * ctx.shp[1]
            same = (dlogits is not None and dlogits_b is not None and dlogits.data_ptr() == buf.data_ptr() and
                    dlogits_b.data_ptr() == buf[r0:].data_ptr() and dlogits.stride(-2) == ld and dlogits_b.stride(-2) == ld)
            if same:
                dlogits = buf[:, :V]                       # both losses wrote their gradient into their part of the logits buffer
            else:
                parts = [torch.zeros((n, V), dtype=bf16, device=x2.device) if g is None else g.reshape(n, V)
                         for g, n in ((dlogits, r0), (dlogits_b, R - r0))]
                dlogits = torch.cat(parts, 0)
        d2 = dlogits.reshape(R, V) if dlogits.is_contiguous() else dlogits
        if d2.dim() != 2:
            d2 = d2.reshape(R, V)
        if d2.stride(-1) != 1 or d2.stride(0) % 8 != 0:
            pad = torch.zeros((R, ld), dtype=bf16, device=d2.device)
            pad[:, :V].copy_(d2)
            d2 = pad[:, :V]
        dw_gemm(d2, tn, V, Hd, R, **_gw(dec.weight), splits=K.splits_for(V, Hd, R), rowsum_a=G(dec.bias))
        # contraction over the vocabulary, rounded up to the row stride of the gradient buffer (30528 = 477 k-tiles): its
        # padding columns are zeros (written by the loss kernel) and so are those of the transposed weight copy, so the
        # product is unchanged and the GEMM can take the large-tile path
        Kv = d2.stride(0) if (d2.stride(0) % 64 == 0 and d2.stride(0) - V < 64) else V
        d_tn = K.gemm(0, d2, W16T(dec.weight), R, Hd, Kv, splits=K.splits_nn(R, Hd, Kv))   # W^T rows are padded to 64 with zeros
        d_t = ln_bwd(d_tn, t, R, Hd, tr.LayerNorm.weight.data, mean, rstd, G(tr.LayerNorm.weight), G(tr.LayerNorm.bias))
        d_tpre = torch.empty((R, Hd), dtype=bf16, device=d_t.device)
        K.scale_mask_rows(d_t, R, Hd, out=d_tpre, colsum=G(tr.dense.bias), gelu_in=t_pre)
        dw_gemm(d_tpre, x2, Hd, Hd, R, **_gw(tr.dense.weight), splits=K.splits_for(Hd, Hd, R))
        dx = K.gemm(0, d_tpre, W16T(tr.dense.weight), R, Hd, Hd)
        return None, dx.view(ctx.shp), None, None


class ScoreHeadFn(torch.autograd.Function):
    """self.fc of the task-specific pre-training model (main_pretrain_task_specific.py:128-133) applied to the
    first text position, reshaped to (B, O) and divided by the temperature (:168-170)."""

    @staticmethod
    def forward(ctx, anchor, x, fc, O, inv_temp, dropout_p):
        n, Hd = x.shape
        lin1, lin2 = fc[1], fc[3]
        F = lin1.weight.shape[0]
        keep = _keep(ctx)
        x = x.contiguous()
        seed = K.next_seed()
        xd = x
        if dropout_p > 0:
            xd = torch.empty_like(x)
            K.scale_mask_rows(x, n, Hd, out=xd, dropout_p=dropout_p, seed=seed)
        act_grad = torch.empty((n, F), dtype=bf16, device=x.device) if keep else None
        h = K.gemm(0, xd, W16(lin1.weight), n, F, Hd, bias=lin1.bias.data, act=2, preact=act_grad, preact_is_grad=True)
        logits = K.pair_score_fwd(h, n, F, W16(lin2.weight).view(F), lin2.bias.data, inv_temp, O)
        if keep:
            ctx.fc, ctx.cfg = fc, (O, inv_temp, dropout_p, seed)
            ctx.save_for_backward(xd, h, act_grad)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        fc, (O, inv_temp, dropout_p, seed) = ctx.fc, ctx.cfg
        xd, h, act_grad = ctx.saved_tensors
        lin1, lin2 = fc[1], fc[3]
        n, Hd = xd.shape
        F = lin1.weight.shape[0]
        assert dlogits.stride(-1) == 1
        dz1 = K.pair_score_bwd(dlogits, n, F, O, inv_temp, h, act_grad, W16(lin2.weight).view(F), G(lin2.weight).view(F),
                               G(lin2.bias))
        K.colsum(dz1, n, F, G(lin1.bias))
        dw_gemm(dz1, xd, F, Hd, n, **_gw(lin1.weight), splits=1)
        dx = K.gemm(0, dz1, W16T(lin1.weight), n, Hd, F)
        if dropout_p > 0:
            K.scale_mask_rows(dx, n, Hd, out=dx, dropout_p=dropout_p, seed=seed)
        return None, dx, None, None, None, None


class CrossEntropyFn(torch.autograd.Function):
    """CrossEntropyLoss(ignore_index=-1) (agent.py:72).  Training: the logits buffer is consumed -- it is
    overwritten in place with d(loss)/d(logits) -- unless `keep_logits`, which spends one copy of the logits (312 MB at the
    benchmark batch) so that the caller's tensor stays readable after the loss (accuracy read-outs, a second loss on the same logits)."""

    @staticmethod
    def forward(ctx, logits, labels, count, keep_logits=False):
        if keep_logits and ctx.needs_input_grad[0]:
            src = logits
            if src.dim() == 2 and src.stride(-1) == 1:
                # a FULL (rows, row stride) buffer with a [:, :V] view: the scale kernels below run over rows * stride elements,
                # so the storage must not end at the last row's V-th column (empty_strided's does)
                logits = torch.empty((src.shape[0], src.stride(0)), dtype=src.dtype, device=src.device)[:, :src.shape[1]]
            else:
                logits = src.clone()
            logits.copy_(src)
        V = logits.shape[-1]
        f32 = logits.dtype == torch.float32
        assert logits.dim() == 2 and logits.stride(-1) == 1 and (f32 or logits.stride(0) % 8 == 0), \
            "logits must be a (rows, V) view of a row-padded bf16 buffer (as produced by the MLM head) or fp32 scores"
        labels = labels.contiguous()
        acc = torch.zeros(2, dtype=torch.float32, device=logits.device)
        train = ctx.needs_input_grad[0]
        scale = (1.0 / max(count, 1)) if count is not None else 1.0
        K.cross_entropy(logits, V, labels, acc, scale, train)
        if train and count is None:
            assert not f32, "fp32 score logits: pass the labelled-row count"
            n = logits.shape[0] * logits.stride(0)
            K.scale_by_count(logits, n, acc, 1.0)
        ctx.grad_buf = logits if train else None
        return acc[0] / acc[1]

    @staticmethod
    def backward(ctx, g):
        buf = ctx.grad_buf
        if buf is None:
            return None, None, None, None
        # d(loss)/d(logits) sits in `buf` for an upstream gradient of 1 (loss = ls_mtm + ls_vtm, main_pretrain_mlm.py:163).
        # Any other upstream scale (gradient accumulation loss / k, loss weights, a GradScaler) is applied by a kernel that
        # reads the scalar on the device -- no host sync; an upstream gradient of exactly 1 costs one load per thread.
        if not CrossEntropyFn.assume_unit_grad:
            n = buf.shape[0] * buf.stride(0)
            if n % 8 == 0:
                K.scale_by_scalar(buf, n, g.reshape(1).float())
            else:                                          # tiny fp32 score matrices whose size is not a multiple of 8
                buf.mul_(g)
        return buf, None, None, None


# Set to True only by a caller that guarantees an upstream gradient of exactly 1 (skips the scale launch above).
CrossEntropyFn.assume_unit_grad = False


class CaptionLossFn(torch.autograd.Function):
    """CaptioningLoss (model_for_captioning.py:10-37) on the labelled rows of a (rows, V) logits view: (loss, stats) with stats (4,) fp32 =
    [sum of the kept row losses, k, number of rows whose arg-max is the label, number of labelled rows] (lav_caption_loss_fwd_bwd).  `k` rows
    are averaged (the caller derives it from the labelled-row count it knows), `select` turns the drop-the-worst selection on.  As with
    CrossEntropyFn, training consumes the logits buffer: it is overwritten in place with d(loss)/d(logits), unless `keep_logits`."""

    @staticmethod
    def forward(ctx, logits, labels, label_smoothing, k, select, keep_logits=False):
        assert logits.dim() == 2 and logits.dtype == torch.bfloat16 and logits.stride(-1) == 1 and logits.stride(0) % 8 == 0, \
            "logits must be a (rows, V) view of a row-padded bf16 buffer (as produced by the MLM head)"
        train = ctx.needs_input_grad[0]
        if keep_logits and train:
            src = logits
            logits = torch.empty((src.shape[0], src.stride(0)), dtype=src.dtype, device=src.device)[:, :src.shape[1]]
            logits.copy_(src)
        stats, row_loss, correct, kept = K.caption_loss(logits, logits.shape[-1], labels.contiguous(), label_smoothing, k, select, train)
        ctx.grad_buf = logits if train else None
        ctx.mark_non_differentiable(stats)
        ctx.rows = (row_loss, correct, kept)               # per-row results, for tests and diagnostics
        return stats[0] / stats[1], stats

    @staticmethod
    def backward(ctx, g, _):
        buf = ctx.grad_buf
        if buf is None:
            return None, None, None, None, None, None
        # the upstream gradient is applied on the device, as in CrossEntropyFn.backward
        K.scale_by_scalar(buf, buf.shape[0] * buf.stride(0), g.reshape(1).float())
        return buf, None, None, None, None, None
