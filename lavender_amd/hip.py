"""Tensor-level wrappers over the C ABI: each function enqueues ONE hand-written HIP kernel on the current
torch stream.  torch is used only for device memory and the stream handle."""
import ctypes as C

import torch

from . import _lib as L

bf16 = torch.bfloat16
_seed_counter = [0x1234567]


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _s():
    # the current torch stream's hipStream_t; the raw getter costs ~0.3 us against 2.7 us for torch.cuda.current_stream().cuda_stream
    # (~1500 calls per training step)
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- caller-owned scratch (lav_set_workspace): torch allocations registered per (stream, kind) on first need, held for the life of the process.
WS_SPLITK, WS_LN_PARTIALS, WS_LN_DEFER = 0, 1, 2
_workspaces = {}
_retired = []          # replaced workspace buffers, kept alive (see ensure_workspace); release_retired_workspaces() after a device synchronisation


def _stream_ptr(stream_ptr=None):
    if stream_ptr is not None:
        return int(stream_ptr)
    if _raw_stream is not None:
        return int(_raw_stream(torch.cuda.current_device()))
    return int(torch.cuda.current_stream().cuda_stream)


def ensure_workspace(kind, need=0, stream_ptr=None):
    """The (stream, kind) workspace exists and holds >= need bytes: lav_workspace_bytes(kind) by default, re-registered larger when a call needs
    more (the library itself never allocates behind a registered buffer: it fails with LAV_E_WORKSPACE)."""
    sp = _stream_ptr(stream_ptr)
    t = _workspaces.get((sp, kind))
    if t is not None and t.numel() >= need:
        return
    size = max(int(L.lib.lav_workspace_bytes(kind)), int(need) + (int(need) // 2 if t is not None else 0))
    old = t
    t = torch.empty(size, dtype=torch.uint8, device="cuda")
    L.check(L.lib.lav_set_workspace(C.c_void_p(sp), kind, C.c_void_p(t.data_ptr()), size), "lav_set_workspace")
    _workspaces[(sp, kind)] = t
    if old is not None:
        # the buffer was allocated on torch's CURRENT stream but may serve another one (the weight-gradient stream): the caching allocator would hand
        # it out again as soon as the current stream is past this point, while kernels of `sp` may still use it -- keep it until the next device-wide
        # quiet point instead (replacement only happens when a call outgrows 256 MiB; no shipped configuration does)
        _retired.append(old)
    if kind == WS_LN_DEFER and LN_DEFER:
        rc = L.lib.lav_layernorm_set_defer(C.c_void_p(sp), 1)      # returns the previous mode (0 / 1); more than 16 streams: stays off (reductions finish at once)
        if rc < 0:
            L.check(rc, "lav_layernorm_set_defer")


def zero_blocks(base, blocks, block_elems):
    """base[blocks[i] * block_elems : + block_elems] = 0 (fp32 base, int32 device list): lav_zero_blocks"""
    L.check(L.lib.lav_zero_blocks(_s(), _p(base), _p(blocks), blocks.numel(), int(block_elems)), "lav_zero_blocks")


def release_retired_workspaces():
    """call after torch.cuda.synchronize(): no kernel can still use a replaced workspace buffer"""
    _retired.clear()


def _split_query(entry, *call):
    """lav_gemm_splits / lav_gemm_tn_splits: (the split factor the entry answers with, the split-K workspace bytes the call will request)"""
    need = C.c_size_t()
    rc = entry(*call, need)
    if rc < 0:
        L.check(rc, entry.__name__)
    return rc, need.value


def ensure_stage_workspaces(shapes, Kd, rpg, side_stream_ptr):
    """before a stage-level backward entry: LayerNorm scratch on the current stream, split-K partial tiles on the stream that runs the weight
    gradients `shapes` (M, N) over Kd token rows (rpg[j] > 0: output j skips drop-path rows in groups of that many)"""
    ensure_workspace(WS_LN_PARTIALS)
    ensure_workspace(WS_LN_DEFER)
    ensure_workspace(WS_SPLITK, _tn_splits(shapes, Kd, rpg)[2], side_stream_ptr)


def next_seed():
    """Fresh 32-bit dropout seed (host-side counter hashed; deterministic under torch.manual_seed order)."""
    _seed_counter[0] = (_seed_counter[0] * 1664525 + 1013904223) & 0xFFFFFFFF
    return _seed_counter[0]


def reseed(seed):
    _seed_counter[0] = (int(seed) * 2654435761 + 12345) & 0xFFFFFFFF


def _ld(t):
    assert t.stride(-1) == 1, "innermost dimension must be contiguous"
    return t.stride(-2) if t.dim() >= 2 else t.shape[-1]


import struct as _struct
from operator import itemgetter as _itemgetter
import threading as _threading
import os as _os_mod
_os_env = _os_mod.environ.get

# lav_gemm_epilogue, packed in ONE struct.pack_into instead of ~30 ctypes field stores (13 -> ~6 us per call on ~450 calls per step:
# the launch thread's Python time is what the step falls back on when the GPU gets faster).  Native alignment ("@") reproduces the C
# layout; tests/test_host_logic.py holds the format to ctypes' own view of the struct, field by field.
_EPI_FIELDS = ("bias", "act", "preact", "ldp", "gelu_in", "ldg", "dropout_p", "seed", "row_scale", "rows_per_group", "residual", "ldr",
               "colsum", "alpha", "out_mode", "k_keep", "k_rows_per_group", "rowsum_a", "preact_is_grad", "gelu_in_is_grad", "residual_f32",
               "a_rowmap", "res_rowmap", "res_ln_mean", "res_ln_rstd", "res_ln_gamma", "res_ln_beta", "hm_heads", "hm_head_dim", "hm_rows",
               "c_pad_writable", "assign")
_EPI_PACK = _struct.Struct("@PiPqPqfIPiPqPfiPiPiiiPPPPPPiiqii")
assert tuple(f[0] for f in L.GemmEpilogue._fields_) == _EPI_FIELDS and _EPI_PACK.size <= C.sizeof(L.GemmEpilogue)
_tls = _threading.local()


def _epi_buffer():
    b = getattr(_tls, "epi", None)
    if b is None:
        raw = C.create_string_buffer(C.sizeof(L.GemmEpilogue))
        b = _tls.epi = (raw, C.cast(raw, C.POINTER(L.GemmEpilogue)))
    return b


def _dp(t):
    return 0 if t is None else t.data_ptr()


def gemm(layout, A, B, M, N, K, out=None, out_dtype=bf16, bias=None, act=0, preact=None, gelu_in=None, dropout_p=0.0,
         seed=0, row_scale=None, rows_per_group=1, residual=None, colsum=None, alpha=1.0, accumulate=False,
         k_keep=None, k_rows_per_group=1, splits=1, ldc=None, rowsum_a=None, preact_is_grad=False, gelu_in_is_grad=False,
         a_rowmap=None, res_rowmap=None, res_ln=None, c_pad_writable=False, headmajor=None, assign=False):
    """layout 0: A[M,K] B[N,K]; 1: A[M,K] B[K,N]; 2: A[K,M] B[K,N].  Returns the (M, N) output view.
    a_rowmap / res_rowmap (int32 [M]): logical row m of A / of the residual is physical row map[m] (pair expansion, layout 0).
    res_ln = (mean, rstd, gamma, beta): `residual` (fp32) is a PRE-LayerNorm tensor, the epilogue adds LayerNorm(residual).
    headmajor = (heads, head_dim): bf16 output stored [plane][head][row][head_dim] (lav_gemm_epilogue.hm_*); `out` is then just M * N elements.
    c_pad_writable: N % 8 != 0 and the padding columns [N, round_up(N, 8)) of `out` may be overwritten (lav_gemm_epilogue.c_pad_writable).
    assign (layout 2 with accumulate=True only): out = result instead of out += result (lav_gemm_epilogue.assign: first writer of a weight gradient)."""
    if out is None:
        ldc = ldc or ((N + 7) // 8 * 8)
        out = torch.empty((M, ldc), dtype=out_dtype, device=A.device)
    else:
        ldc = _ld(out)
    res32 = 0 if residual is None else (1 if residual.dtype == torch.float32 else (2 if residual.dtype == torch.float16 else 0))   # lav_gemm_epilogue.residual_f32
    if res_ln is not None:
        assert res32 and out.dtype in (torch.float32, torch.float16)
        ln_m, ln_r, ln_g, ln_b = (t.data_ptr() for t in res_ln)
    else:
        ln_m = ln_r = ln_g = ln_b = 0
    hm_h, hm_d, hm_rows = (int(headmajor[0]), int(headmajor[1]), int(M)) if headmajor is not None else (0, 0, 0)
    raw, ref = _epi_buffer()
    _EPI_PACK.pack_into(raw, 0,
                        _dp(bias), act, _dp(preact), _ld(preact) if preact is not None else 0,
                        _dp(gelu_in), _ld(gelu_in) if gelu_in is not None else 0,
                        float(dropout_p), int(seed) & 0xFFFFFFFF, _dp(row_scale), int(rows_per_group),
                        _dp(residual), _ld(residual) if residual is not None else 0, _dp(colsum), float(alpha),
                        2 if accumulate else (1 if out.dtype == torch.float32 else (3 if out.dtype == torch.float16 else 0)),
                        _dp(k_keep), int(k_rows_per_group), _dp(rowsum_a), int(preact_is_grad), int(gelu_in_is_grad), int(res32),
                        _dp(a_rowmap), _dp(res_rowmap), ln_m, ln_r, ln_g, ln_b, hm_h, hm_d, hm_rows, int(bool(c_pad_writable)), int(bool(assign)))
    if splits > 1:
        ensure_workspace(WS_SPLITK, _split_query(L.lib.lav_gemm_splits, layout, M, N, K, _ld(A), _ld(B), ldc, ref, splits)[1])
    rc = L.lib.lav_gemm_bf16(_s(), layout, M, N, K, A.data_ptr(), _ld(A), B.data_ptr(), _ld(B), out.data_ptr(), ldc, ref, splits)
    if rc != 0:
        L.check(rc, "lav_gemm_bf16")
    return out[:, :N] if out.shape[-1] != N else out


def gemm_tn_grouped(jobs, splits):
    """Grouped weight gradients (lav_gemm_tn_grouped): jobs = up to four dicts with A [K, M], B [K, N] (bf16), out [M, N] (fp32, accumulated)
    and optionally rowsum_a, k_keep, k_rows_per_group, alpha, fallback_splits; one launch when every job fits the 256 x 256 weight-gradient kernel."""
    arr = (L.GemmTnJob * len(jobs))()
    for q, j in zip(arr, jobs):
        A, B, out = j["A"], j["B"], j["out"]
        q.K, q.M, q.N = A.shape[0], j.get("M", A.shape[1]), j.get("N", B.shape[1])
        q.A, q.lda, q.B, q.ldb, q.C, q.ldc = A.data_ptr(), _ld(A), B.data_ptr(), _ld(B), out.data_ptr(), _ld(out)
        q.rowsum_a, q.k_keep = _dp(j.get("rowsum_a")), _dp(j.get("k_keep"))
        q.k_rows_per_group, q.alpha, q.fallback_splits = int(j.get("k_rows_per_group", 1)), float(j.get("alpha", 1.0)), int(j.get("fallback_splits", 1))
        q.assign = int(bool(j.get("assign", False)))
    ensure_workspace(WS_SPLITK, _split_query(L.lib.lav_gemm_tn_splits, len(jobs), arr, max(int(splits), 1))[1])
    rc = L.lib.lav_gemm_tn_grouped(_s(), len(jobs), arr, int(splits))
    if rc != 0:
        L.check(rc, "lav_gemm_tn_grouped")


# ---- stage-level entries (lavender_amd/csrc/stages.cpp): one C call per Swin block / fusion-encoder layer pass ----------------------------
_PACK_CODE = {L.i32: "i", L.f32: "f", L.u32: "I", L.i64: "q", L.vp: "P"}


class DescLayout:
    """Flat view of a ctypes descriptor declaration (nested structs flattened): .names in declaration order, .pos name -> position and .pack,
    the struct.Struct that fills the descriptor with ONE pack_into (native alignment "@" reproduces the C layout)."""

    def __init__(self, st):
        self.struct = st
        fields, fmt = self._flatten(st)
        self.names = tuple(n for n, _ in fields)
        self.pos = {n: i for i, n in enumerate(self.names)}
        assert len(self.pos) == len(self.names), "field names of a descriptor and its nested parts must be distinct"
        self.pack = _struct.Struct("@" + fmt)
        self._tls = _threading.local()
        assert self.pack.size <= C.sizeof(st) < self.pack.size + 8, st          # only tail padding may differ

    @staticmethod
    def _flatten(st):
        fields, fmt = [], ""
        for name, ct in st._fields_:
            if issubclass(ct, C.Structure):
                sub, f = DescLayout._flatten(ct)
                fields += sub
                fmt += f + {4: "0i", 8: "0q"}[C.alignment(ct)]                    # the nested struct's own tail padding
            else:
                fields.append((name, ct))
                fmt += _PACK_CODE[ct]
        return fields, fmt

    def fill(self, fields):
        """this thread's descriptor filled with one pack_into: the pointer to hand the C entry"""
        b = getattr(self._tls, "b", None)
        if b is None:
            raw = C.create_string_buffer(C.sizeof(self.struct))
            b = self._tls.b = (raw, C.cast(raw, C.POINTER(self.struct)))
        self.pack.pack_into(b[0], 0, *fields)
        return b[1]

    def placer(self, names, partial=False):
        """f(values given in the order of `names`) -> the values in declaration order.  The permutation is worked out here, once; a call
        is one itemgetter.  partial: fields that `names` lacks are filled with 0 (otherwise they are an error)."""
        src = {n: i for i, n in enumerate(names)}
        assert len(src) == len(names) and not set(names) - set(self.names), (set(names) - set(self.names), len(src), len(names))
        assert partial or len(names) == len(self.names), set(self.names) - set(names)
        pick = _itemgetter(*(src.get(n, len(names)) for n in self.names))
        return (lambda vals: pick(vals + (0,))) if len(names) != len(self.names) else pick


BL_FWD, BL_BWD, SB_FWD, SB_BWD = (DescLayout(st) for st in (L.BertLayerDesc, L.BertLayerBwdDesc, L.SwinBlockDesc, L.SwinBlockBwdDesc))
_BL_FWD_PACK, _BL_BWD_PACK, _SB_FWD_PACK, _SB_BWD_PACK = BL_FWD.pack, BL_BWD.pack, SB_FWD.pack, SB_BWD.pack


def _stage_call(name, layout, fields, *streams):
    rc = getattr(L.lib, name)(_s(), *streams, layout.fill(fields))
    if rc != 0:
        L.check(rc, name)


def swin_block_fwd(fields):
    """fields: lav_swin_block_desc in declaration order (SB_FWD.names: ints / floats / device addresses, 0 = NULL)"""
    _stage_call("lav_swin_block_fwd", SB_FWD, fields)


def swin_block_bwd(fields, side_stream):
    _stage_call("lav_swin_block_bwd", SB_BWD, fields, side_stream)


def bert_layer_fwd(fields):
    _stage_call("lav_bert_layer_fwd", BL_FWD, fields)


def bert_layer_bwd(fields, side_stream):
    """fields: lav_bert_layer_bwd_desc in declaration order (BL_BWD.names: the forward's values first); side_stream: raw hipStream_t or None"""
    _stage_call("lav_bert_layer_bwd", BL_BWD, fields, side_stream)


# ---- split-K policy: the library's (gemm.hip, beside the route plan); these ask for it ---------------------------------------------------------
_tn_cache = {}       # per shape: a ctypes job array per stage call would cost more than the arithmetic did when it lived here


def gemm_select(which, value):
    """lav_gemm_select.  The switches move the split factors, so everything cached from the policy is dropped: call this, never the library's
    entry directly."""
    _tn_cache.clear()
    return L.lib.lav_gemm_select(which, value)


def _tn_splits(shapes, K, rpg=None):
    """lav_gemm_tn_splits for the weight gradients `shapes` (M, N) with contraction K (rpg[j] > 0: drop-path keep rows in groups of that many):
    (split factor of each output alone, group factor or 0, split-K workspace bytes that cover either way of launching them)"""
    key = (shapes, K, rpg)
    r = _tn_cache.get(key)
    if r is None:
        arr = (L.GemmTnJob * len(shapes))()
        for q, (M, N), g in zip(arr, shapes, rpg or (0,) * len(shapes)):
            q.M, q.N, q.K, q.lda, q.ldb, q.ldc = M, N, K, (M + 7) // 8 * 8, (N + 7) // 8 * 8, (N + 3) // 4 * 4
            q.k_keep, q.k_rows_per_group = (8 if g else None), g          # (only tested for presence)
        gs, need = _split_query(L.lib.lav_gemm_tn_splits, len(arr), arr, 0)
        r = _tn_cache[key] = (tuple(q.fallback_splits for q in arr), gs, need)
    return r


def splits_for(M, N, K, keep=False):
    """split-K factor for a weight-gradient GEMM, matched to the tile lav_gemm_bf16 runs the shape on (gemm.hip: tn_splits)"""
    return _tn_splits(((M, N),), K, (K,) if keep else None)[0][0]          # (the factor depends on keep rows being there, not on their grouping)


def group_splits_for(shapes, K):
    """split factor of a GROUPED weight-gradient launch over the (M, N) outputs `shapes` with contraction K (lav_gemm_tn_grouped), 0 when the
    group does not apply (an output the 256 x 256 kernel cannot take: the stage entries then launch one by one with splits_for)."""
    return _tn_splits(tuple(shapes), K)[1]


def splits_nn(M, N, K):
    """split-K factor for a forward / input-gradient GEMM whose output is too small to fill the chip while K is long
    (d_hidden = dlogits . W_dec: K = vocabulary): gemm.hip nn_splits"""
    return L.lib.lav_gemm_splits(1, M, N, K, 0, 0, 0, None, 0, None)


def _gather(g):
    if g is None:
        return None
    s = L.LnGather()
    s.mode, s.H, s.W, s.C0 = 1, g[0], g[1], g[2]
    return C.byref(s)


def layernorm_fwd(x, rows, Cn, gamma, beta, eps, gather=None, out=None, want_stats=True, out32=None, want16=True):
    """x bf16, fp32 or fp16 (the wide residual stream of the fusion encoder); out32: optional fp32 copy of the output (then returned 4th)."""
    dev = x.device
    y = out if out is not None else (torch.empty((rows, Cn), dtype=bf16, device=dev) if want16 else None)
    mean = torch.empty(rows, dtype=torch.float32, device=dev) if want_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=dev) if want_stats else None
    ldx = gather[2] if gather is not None else _ld(x)
    f = None
    if x.dtype in (torch.float32, torch.float16) or out32 is not None:
        st = L.LnF32()
        st.x_f32 = 1 if x.dtype == torch.float32 else (2 if x.dtype == torch.float16 else 0)
        st.y32 = _p(out32)
        st.ldy32 = _ld(out32) if out32 is not None else 0
        f = C.byref(st)
    L.check(L.lib.lav_layernorm_fwd(_s(), rows, Cn, _p(x), ldx, _gather(gather), _p(gamma), _p(beta), float(eps), _p(y),
                                    _ld(y) if y is not None else 0, _p(mean), _p(rstd), f), "lav_layernorm_fwd")
    return y, mean, rstd


LN_DEFER = _os_env("LAV_LN_DEFER", "1") != "0"      # deferred column reductions of the LayerNorm backward (lav_layernorm_set_defer): one finish launch per flush


def layernorm_flush():
    """complete the queued column reductions (dgamma / dbeta / colsum) of EVERY stream (each on its own stream) and make the current stream
    wait for them: lav_layernorm_flush_all.  Whatever stream ran the backward, work enqueued on the current stream afterwards sees them."""
    if LN_DEFER:
        rc = L.lib.lav_layernorm_flush_all(_s())
        if rc != 0:
            L.check(rc, "lav_layernorm_flush_all")


def layernorm_bwd(dy, x, rows, Cn, gamma, mean, rstd, dgamma, dbeta, gather=None, add_in=None, dx=None, dx2=None,
                  row_scale=None, rows_per_group=1, dropout_p=0.0, seed=0, colsum=None, flush=True):
    """flush=False (the engine): in the deferred mode dgamma / dbeta / colsum are only complete after layernorm_flush(); the default
    completes them before returning, as without the mode."""
    dev = dy.device
    ensure_workspace(WS_LN_PARTIALS)
    ensure_workspace(WS_LN_DEFER)
    if dx is None:
        dx = torch.empty((rows * 4, Cn // 4) if gather is not None else (rows, Cn), dtype=bf16, device=dev)
    ldx = gather[2] if gather is not None else _ld(x)
    lddx = gather[2] if gather is not None else _ld(dx)
    ex = None
    x32 = 1 if x.dtype == torch.float32 else (2 if x.dtype == torch.float16 else 0)      # lav_ln_bwd_extra.x_f32
    if dx2 is not None or colsum is not None or x32:
        s = L.LnBwdExtra()
        s.x_f32 = int(x32)
        s.dx2 = _p(dx2)
        s.lddx2 = _ld(dx2) if dx2 is not None else 0
        s.row_scale = _p(row_scale)
        s.rows_per_group = int(rows_per_group)
        s.dropout_p = float(dropout_p)
        s.seed = int(seed) & 0xFFFFFFFF
        s.colsum = _p(colsum)
        ex = C.byref(s)
    L.check(L.lib.lav_layernorm_bwd(_s(), rows, Cn, _p(dy), _ld(dy), _p(x), ldx, _gather(gather), _p(gamma), _p(mean),
                                    _p(rstd), _p(add_in), (_ld(add_in) if add_in is not None else 0), _p(dx), lddx,
                                    _p(dgamma), _p(dbeta), ex), "lav_layernorm_bwd")
    if flush:
        layernorm_flush()
    return dx


def scale_mask_rows(x, rows, Cn, out=None, row_scale=None, rows_per_group=1, dropout_p=0.0, seed=0, colsum=None,
                    gelu_in=None):
    L.check(L.lib.lav_scale_mask_rows(_s(), rows, Cn, _p(x), _ld(x), _p(out), (_ld(out) if out is not None else 0),
                                      _p(row_scale), int(rows_per_group), float(dropout_p), int(seed) & 0xFFFFFFFF,
                                      _p(colsum), _p(gelu_in), (_ld(gelu_in) if gelu_in is not None else 0)),
            "lav_scale_mask_rows")
    return out


def colsum(x, rows, Cn, out):
    L.check(L.lib.lav_colsum_bf16(_s(), rows, Cn, _p(x), _ld(x), _p(out)), "lav_colsum_bf16")


_WIN_TABLES = {}


def window_tables(device, D, H, W, window, shift):
    """Host-side geometry tables of the fast window-attention path (cached per geometry):
    token row of (window, in-window index) in the un-rolled tensor (roll + window_partition of
    video_swin.py:82-86,218-227 as a lookup), the mask type of every window and the shift-region id of every
    in-window token per type (compute_mask, video_swin.py:290-305, in closed form)."""
    key = (str(device), D, H, W, tuple(window), tuple(shift))
    if key in _WIN_TABLES:
        return _WIN_TABLES[key]
    import numpy as np
    wd, wh, ww = window
    sd, sh, sw = shift
    N = wd * wh * ww
    assert N <= 256
    nd, nh, nw = D // wd, H // wh, W // ww
    bd, bh, bw = np.meshgrid(np.arange(nd), np.arange(nh), np.arange(nw), indexing="ij")
    bd, bh, bw = bd.reshape(-1, 1), bh.reshape(-1, 1), bw.reshape(-1, 1)
    i_d, i_h, i_w = np.meshgrid(np.arange(wd), np.arange(wh), np.arange(ww), indexing="ij")
    i_d, i_h, i_w = i_d.reshape(1, -1), i_h.reshape(1, -1), i_w.reshape(1, -1)
    src_d, src_h, src_w = (bd * wd + i_d + sd) % D, (bh * wh + i_h + sh) % H, (bw * ww + i_w + sw) % W
    tok = np.full((nd * nh * nw, 256), -1, dtype=np.int32)
    tok[:, :N] = (src_d * H + src_h) * W + src_w
    flags = ((bd[:, 0] == nd - 1) & (sd > 0)) * 4 + ((bh[:, 0] == nh - 1) & (sh > 0)) * 2 + ((bw[:, 0] == nw - 1) & (sw > 0)) * 1
    uniq = sorted(set(flags.tolist()))
    wtype = np.array([uniq.index(f) for f in flags.tolist()], dtype=np.uint8)
    region = np.zeros((len(uniq), 256), dtype=np.uint8)
    for t, f in enumerate(uniq):
        rd = (1 + (i_d[0] >= wd - sd)) if (f & 4) else 0 * i_d[0]
        rh = (1 + (i_h[0] >= wh - sh)) if (f & 2) else 0 * i_h[0]
        rw = (1 + (i_w[0] >= ww - sw)) if (f & 1) else 0 * i_w[0]
        region[t, :N] = rd * 9 + rh * 3 + rw
    out = dict(tok=torch.from_numpy(tok).to(device), wtype=torch.from_numpy(wtype).to(device),
               region=torch.from_numpy(region).to(device), ntypes=len(uniq))
    _WIN_TABLES[key] = out
    return out


BIAS_MAP = _os_env("LAV_BIAS_MAP", "1") != "0"     # window bias fragments gathered through a per-geometry index map (lav_attn_desc.bias_map); 0 = index arithmetic in every build


class Attn:
    """Descriptor + scratch for one attention call (window or sequence mode)."""

    def __init__(self, mode, heads, head_dim, fast=True, **kw):
        d = L.AttnDesc()
        d.mode, d.heads, d.head_dim = mode, heads, head_dim
        d.scale = float(head_dim) ** -0.5
        for k, v in kw.items():
            if k in ("bias_table", "key_mask"):
                setattr(d, k, _p(v))
            else:
                setattr(d, k, v)
        self.d = d
        self._keep = kw
        if mode == 0 and fast and kw["wd"] * kw["wh"] * kw["ww"] <= 256:
            # fast path: precomputed token rows + fragment-ordered (bias + mask) tables, rebuilt from the
            # current bias table (one small kernel per call site per step)
            dev = kw["bias_table"].device
            t = window_tables(dev, kw["D"], kw["H"], kw["W"], (kw["wd"], kw["wh"], kw["ww"]), (kw["sd"], kw["sh"], kw["sw"]))
            n = t["ntypes"] * heads * 64 * 64 * 16
            self.comb = torch.empty(n, dtype=bf16, device=dev)
            self.combT = torch.empty(n, dtype=bf16, device=dev)
            d.tok_table, d.win_type, d.type_region, d.n_types = _p(t["tok"]), _p(t["wtype"]), _p(t["region"]), t["ntypes"]
            d.comb, d.combT = _p(self.comb), _p(self.combT)
            self._tables = t
            if BIAS_MAP:
                # the index half of the table build (relative_position_index + shift mask + padding classes): once per geometry
                mkey = ("bias_map", kw["cfg_wd"], kw["cfg_wh"], kw["cfg_ww"])
                bm = t.get(mkey)
                if bm is None:
                    bm = torch.empty(2 * t["ntypes"] * 65536, dtype=torch.int32, device=dev)
                    d.bias_map = _p(bm)
                    L.check(L.lib.lav_attention_build_bias_map(_s(), C.byref(d)), "lav_attention_build_bias_map")
                    bm.record_stream(torch.cuda.current_stream(dev))
                    t[mkey] = bm
                d.bias_map = _p(bm)
                self._bias_map = bm
            L.check(L.lib.lav_attention_build_bias(_s(), C.byref(d)), "lav_attention_build_bias")

    def lse_elems(self):
        n = L.lib.lav_attention_lse_elems(C.byref(self.d))
        if n == 0:
            L.check(-1, "lav_attention_lse_elems")
        return n

    def fwd(self, qkv, out, lse):
        L.check(L.lib.lav_attention_fwd(_s(), C.byref(self.d), _p(qkv), _p(out), _p(lse)), "lav_attention_fwd")

    def bwd(self, qkv, out, dout, lse, dqkv, dbias):
        L.check(L.lib.lav_attention_bwd(_s(), C.byref(self.d), _p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), _p(dbias)),
                "lav_attention_bwd")

    @property
    def split_bias_grad(self):
        """True when the bias-table gradient can run as its own launch (bwd(..., dbias=None) then bwd_bias on any stream)."""
        return bool(L.lib.lav_attention_bias_split(C.byref(self.d)))

    def bwd_bias(self, qkv, dout, lse, dbias):
        L.check(L.lib.lav_attention_bwd_bias(_s(), C.byref(self.d), _p(qkv), _p(dout), _p(lse), _p(dbias)), "lav_attention_bwd_bias")

    def plan(self, which=0):
        """the launches pass `which` would make (0 forward, 1 backward, 2 backward with the bias-table gradient, 3 that gradient alone) as
        lav_attn_launch_info entries (kernel, route, grid, block, LDS bytes, split, delta_negated), without making them: lav_attention_plan"""
        out = (L.AttnLaunchInfo * 4)()
        n = L.lib.lav_attention_plan(C.byref(self.d), which, out, 4)
        if n < 0:
            L.check(n, "lav_attention_plan")
        return list(out[:n])


def patch_im2col(img, B, T, H, W, frame_major):
    out = torch.empty((B * T * (H // 4) * (W // 4), 96), dtype=bf16, device=img.device)
    L.check(L.lib.lav_patch_im2col(_s(), _p(img), B, T, H, W, int(frame_major), _p(out)), "lav_patch_im2col")
    return out


def video_embed_fwd(feat, B, T, hw, Hd, cls, pos, len_, gamma, beta, eps, out, seq_rows):
    rows = B * T * (1 + hw)
    mean = torch.empty(rows, dtype=torch.float32, device=feat.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=feat.device)
    L.check(L.lib.lav_video_embed_fwd(_s(), B, T, hw, Hd, _p(feat), _p(cls), _p(pos), _p(len_), _p(gamma), _p(beta),
                                      float(eps), _p(out), int(seq_rows), _p(mean), _p(rstd)), "lav_video_embed_fwd")
    return mean, rstd


def video_embed_bwd(dout, seq_rows, feat, B, T, hw, Hd, cls, pos, len_, gamma, mean, rstd, dfeat, d_cls, d_pos, d_len,
                    dgamma, dbeta):
    L.check(L.lib.lav_video_embed_bwd(_s(), B, T, hw, Hd, _p(dout), int(seq_rows), _p(feat), _p(cls), _p(pos), _p(len_),
                                      _p(gamma), _p(mean), _p(rstd), _p(dfeat), _p(d_cls), _p(d_pos), _p(d_len),
                                      _p(dgamma), _p(dbeta)), "lav_video_embed_bwd")


def text_embed_fwd(ids, n, X, Hd, word, pos, type0, gamma, beta, eps, dropout_p, seed, out=None):
    dev = ids.device
    if out is None:
        out = torch.empty((n * X, Hd), dtype=bf16, device=dev)
    mean = torch.empty(n * X, dtype=torch.float32, device=dev)
    rstd = torch.empty(n * X, dtype=torch.float32, device=dev)
    L.check(L.lib.lav_text_embed_fwd(_s(), n, X, Hd, _p(ids), _p(word), _p(pos), _p(type0), _p(gamma), _p(beta), float(eps),
                                     float(dropout_p), int(seed) & 0xFFFFFFFF, _p(out), _p(mean), _p(rstd)),
            "lav_text_embed_fwd")
    return out, mean, rstd


def text_embed_bwd(ids, dout, n, X, Hd, word, pos, type0, gamma, mean, rstd, dropout_p, seed, d_word, d_pos, d_type0,
                   dgamma, dbeta):
    L.check(L.lib.lav_text_embed_bwd(_s(), n, X, Hd, _p(ids), _p(dout), _p(word), _p(pos), _p(type0), _p(gamma), _p(mean),
                                     _p(rstd), float(dropout_p), int(seed) & 0xFFFFFFFF, _p(d_word), _p(d_pos),
                                     _p(d_type0), _p(dgamma), _p(dbeta)), "lav_text_embed_bwd")


def text_embed_pre_fwd(ids, n, Lp, X, Hd, word, pos, type0, gamma, beta, eps, dropout_p, seed, pre, pre_stride, out=None):
    """lav_text_embed_pre_fwd: (n * (Lp + X), Hd) bf16 rows [pre-text ; text] per text; pre: bf16 rows read from pre + j * pre_stride"""
    dev = ids.device
    if out is None:
        out = torch.empty((n * (Lp + X), Hd), dtype=bf16, device=dev)
    assert out.numel() >= n * (Lp + X) * Hd and out.is_contiguous()
    mean = torch.empty(n * X, dtype=torch.float32, device=dev)
    rstd = torch.empty(n * X, dtype=torch.float32, device=dev)
    L.check(L.lib.lav_text_embed_pre_fwd(_s(), n, Lp, X, Hd, _p(ids), _p(word), _p(pos), _p(type0), _p(gamma), _p(beta), float(eps),
                                         float(dropout_p), int(seed) & 0xFFFFFFFF, _p(pre) if Lp else None, int(pre_stride), _p(out),
                                         _p(mean), _p(rstd)), "lav_text_embed_pre_fwd")
    return out, mean, rstd


def text_embed_pre_bwd(ids, dout, n, Lp, X, Hd, word, pos, type0, gamma, mean, rstd, dropout_p, seed, d_word, d_pos, d_type0,
                       dgamma, dbeta, pre_stride, d_pre, d_pre_mode):
    """lav_text_embed_pre_bwd: d_pre_mode 0 accumulates the summed pre-text gradient into the fp32 rows d_pre, 1 writes bf16 rows"""
    if Lp and pre_stride == 0 and n >= 8:
        ensure_workspace(WS_LN_PARTIALS, 8 * Lp * Hd * 4)          # the texts' fp32 partials of the broadcast pre-text gradient
    L.check(L.lib.lav_text_embed_pre_bwd(_s(), n, Lp, X, Hd, _p(ids), _p(dout), _p(word), _p(pos), _p(type0), _p(gamma), _p(mean),
                                         _p(rstd), float(dropout_p), int(seed) & 0xFFFFFFFF, _p(d_word), _p(d_pos), _p(d_type0),
                                         _p(dgamma), _p(dbeta), int(pre_stride), _p(d_pre) if Lp else None, int(d_pre_mode)),
            "lav_text_embed_pre_bwd")


def _pair_index(idx, bound, what, device):
    """int32 device copy of a pair-list index, every entry checked against [0, bound) on the host first: the kernel reads the mask rows it names
    without a bounds check.  Host arrays (what the model passes) cost no device read; a device tensor is read back once."""
    if isinstance(idx, torch.Tensor):
        host = idx.detach().to("cpu", torch.int64)
    else:
        import numpy as np
        host = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64))
    host = host.reshape(-1)
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= bound):
        raise ValueError(f"pair_key_mask: {what} holds {int(host.min())}..{int(host.max())}, outside [0, {bound})")
    if isinstance(idx, torch.Tensor) and idx.device == device and idx.dtype == torch.int32 and idx.is_contiguous():
        return idx
    # non-blocking upload: a synchronous copy would wait for everything queued so far
    return host.to(torch.int32).to(device, non_blocking=True)


def pair_key_mask(mask_img, mask_txt, vi, ti):
    """(n, Lv + X) int32 key mask of the pair list (vi[k], ti[k]) from the int64 (B, Lv) / (nt, X) masks: lav_pair_key_mask.
    vi / ti: host arrays or device tensors; an index outside [0, B) / [0, nt) raises ValueError before anything is launched."""
    n, Lv, X = len(vi), mask_img.shape[1], mask_txt.shape[1]
    if len(ti) != n:
        raise ValueError(f"pair_key_mask: {n} video indices but {len(ti)} text indices")
    vi32 = _pair_index(vi, mask_img.shape[0], "vi", mask_img.device)
    ti32 = _pair_index(ti, mask_txt.shape[0], "ti", mask_img.device)
    if mask_img.dtype != torch.int64 or not mask_img.is_contiguous():
        mask_img = mask_img.long().contiguous()
    if mask_txt.dtype != torch.int64 or not mask_txt.is_contiguous():
        mask_txt = mask_txt.long().contiguous()
    out = torch.empty((n, Lv + X), dtype=torch.int32, device=mask_img.device)
    L.check(L.lib.lav_pair_key_mask(_s(), n, Lv, X, _p(mask_img), _p(mask_txt), _p(vi32), _p(ti32), _p(out)), "lav_pair_key_mask")
    return out


def gather_rows(src, src_row, n_rows, Cn, out=None):
    if out is None:
        out = torch.empty((n_rows, Cn), dtype=bf16, device=src.device)
    L.check(L.lib.lav_gather_rows(_s(), n_rows, Cn, _p(src), _ld(src), _p(src_row), _p(out), _ld(out)), "lav_gather_rows")
    return out


def gather_sum_rows(src, start, lst, n_out, Cn):
    out = torch.empty((n_out, Cn), dtype=bf16, device=src.device)
    L.check(L.lib.lav_gather_sum_rows(_s(), n_out, Cn, _p(src), _ld(src), _p(start), _p(lst), _p(out), _ld(out)),
            "lav_gather_sum_rows")
    return out


def cross_entropy(logits2d, V, labels, loss_sum, grad_scale, write_grad):
    rows = logits2d.shape[0]
    if logits2d.dtype == torch.float32:
        L.check(L.lib.lav_cross_entropy_f32_fwd_bwd(_s(), rows, V, _p(logits2d), _ld(logits2d), _p(labels), _p(loss_sum),
                                                    float(grad_scale), int(write_grad)), "lav_cross_entropy_f32_fwd_bwd")
        return
    L.check(L.lib.lav_cross_entropy_fwd_bwd(_s(), rows, V, _p(logits2d), _ld(logits2d), _p(labels), _p(loss_sum),
                                            float(grad_scale), int(write_grad)), "lav_cross_entropy_fwd_bwd")


def caption_loss(logits2d, V, labels, label_smoothing, k, select, write_grad):
    """lav_caption_loss_fwd_bwd on a (rows, V) view of a row-padded bf16 logits buffer: (out (4,) fp32 = [sum of kept losses, k, sum of correct,
    number of labelled rows], row_loss (rows,) fp32, correct (rows,) int32, kept (rows,) int32); write_grad overwrites the logits with (p - q) / k"""
    rows, dev = logits2d.shape[0], logits2d.device
    f = torch.empty((2, rows), dtype=torch.float32, device=dev)          # row losses, row log-sum-exps
    i = torch.empty((2, rows), dtype=torch.int32, device=dev)            # correct, kept
    out = torch.empty(4, dtype=torch.float32, device=dev)
    L.check(L.lib.lav_caption_loss_fwd_bwd(_s(), rows, V, _p(logits2d), _ld(logits2d), _p(labels), float(label_smoothing), int(k), int(select),
                                           _p(f[0]), _p(f[1]), _p(i[0]), _p(i[1]), _p(out), int(write_grad)), "lav_caption_loss_fwd_bwd")
    return out, f[0], i[0], i[1]


def scale_by_count(x, n_elems, loss_sum, gscale):
    L.check(L.lib.lav_scale_by_count(_s(), int(n_elems), _p(x), _p(loss_sum), float(gscale)), "lav_scale_by_count")


def scale_by_scalar(x, n_elems, scalar_dev):
    """x *= scalar_dev[0] (device scalar, no host sync; exactly 1 is a no-op)."""
    L.check(L.lib.lav_scale_by_scalar(_s(), int(n_elems), _p(x), int(x.dtype == torch.float32), _p(scalar_dev)), "lav_scale_by_scalar")


def pair_score_fwd(h, n, F, w16, bias, inv_temp, O):
    """(n, F) hidden rows -> (n // O, O) fp32 logits."""
    buf = torch.empty((n // O, O), dtype=torch.float32, device=h.device)
    L.check(L.lib.lav_pair_score_fwd(_s(), n, F, _p(h), _ld(h), _p(w16), _p(bias), float(inv_temp), O, _p(buf), O),
            "lav_pair_score_fwd")
    return buf


def pair_score_bwd(dlogits, n, F, O, inv_temp, h, act_grad, w16, dw, db):
    dh = torch.empty((n, F), dtype=bf16, device=h.device)
    L.check(L.lib.lav_pair_score_bwd(_s(), n, F, _p(dlogits), dlogits.stride(0), O, float(inv_temp), _p(h), _ld(h),
                                     _p(act_grad), _ld(act_grad) if act_grad is not None else 0, _p(w16), _p(dh), F,
                                     _p(dw), _p(db)), "lav_pair_score_bwd")
    return dh


def sumsq(g, n, out):
    L.check(L.lib.lav_sumsq_f32(_s(), int(n), _p(g), _p(out)), "lav_sumsq_f32")


def adamw(n, p, g, m, v, p16, block_group, lr4, wd4, b1, b2, eps, step, gradsq, max_norm, grad_div):
    lr_a = (C.c_float * 4)(*[float(x) for x in lr4])
    wd_a = (C.c_float * 4)(*[float(x) for x in wd4])
    L.check(L.lib.lav_adamw_step(_s(), int(n), _p(p), _p(g), _p(m), _p(v), _p(p16), _p(block_group), lr_a, wd_a, float(b1),
                                 float(b2), float(eps), int(step), _p(gradsq), float(max_norm), float(grad_div)),
            "lav_adamw_step")


def transpose_batched(n_mats, descs_dev, total_tiles, src, dst):
    L.check(L.lib.lav_transpose_bf16_batched(_s(), int(n_mats), _p(descs_dev), int(total_tiles), _p(src), _p(dst)),
            "lav_transpose_bf16_batched")


def cast_bf16(src, dst, n):
    L.check(L.lib.lav_cast_f32_to_bf16(_s(), int(n), _p(src), _p(dst)), "lav_cast_f32_to_bf16")


def widen_bf16(src, dst, n):
    L.check(L.lib.lav_cast_bf16_to_f32(_s(), int(n), _p(src), _p(dst)), "lav_cast_bf16_to_f32")


def fill_droppath(n_blocks, B, keep_prob, seed, out):
    L.check(L.lib.lav_fill_droppath(_s(), n_blocks, B, _p(keep_prob), int(seed) & 0xFFFFFFFF, _p(out)), "lav_fill_droppath")


# ---- fp32-I/O validation mode (csrc/validate.hip; see lavender_amd/validate.py) ---------------------------------------
def v_gemm(A, B, out, M, N, K, bias=None, act=0, residual=None):
    """out[M,N] = act(A[M,K] . B[N,K]^T + bias) + residual, everything fp32."""
    for t in (A, B, out, bias, residual):
        assert t is None or t.dtype == torch.float32
    L.check(L.lib.lav_v_gemm_f32(_s(), M, N, K, _p(A), _ld(A), _p(B), _ld(B), _p(out), _ld(out), _p(bias), int(act), _p(residual),
                                 _ld(residual) if residual is not None else 0), "lav_v_gemm_f32")
    return out


def v_attention(att, qkv, out, pad_qkv=None):
    L.check(L.lib.lav_v_attention_f32(_s(), C.byref(att.d), _p(qkv), _p(out), _p(pad_qkv)), "lav_v_attention_f32")


def v_im2col(img, B, T, H, W, frame_major, out):
    L.check(L.lib.lav_v_im2col_f32(_s(), _p(img), B, T, H, W, int(frame_major), _p(out)), "lav_v_im2col_f32")


def v_video_embed(feat, B, T, hw, Hd, cls, pos, len_, gamma, beta, eps, out, seq_rows):
    L.check(L.lib.lav_v_video_embed_f32(_s(), B, T, hw, Hd, _p(feat), _p(cls), _p(pos), _p(len_), _p(gamma), _p(beta), float(eps),
                                        _p(out), int(seq_rows)), "lav_v_video_embed_f32")


def v_text_embed(ids, n, X, Hd, word, pos, type0, gamma, beta, eps, out):
    L.check(L.lib.lav_v_text_embed_f32(_s(), n, X, Hd, _p(ids), _p(word), _p(pos), _p(type0), _p(gamma), _p(beta), float(eps),
                                       _p(out)), "lav_v_text_embed_f32")


def v_gather_rows(src, src_row, n_rows, Cn, out):
    L.check(L.lib.lav_v_gather_rows_f32(_s(), n_rows, Cn, _p(src), _ld(src), _p(src_row), _p(out), _ld(out)), "lav_v_gather_rows_f32")


# ---- caption decoding (csrc/decode.hip) ----------------------------------------------------------------------------------------
SKINNY_BF16, SKINNY_GELU, SKINNY_RES_F32, SKINNY_F32 = 0, 1, 2, 3


def gemm_skinny(x, w, M, N, K, out, epi=SKINNY_BF16, bias=None, residual=None, ldx=None, ldo=None):
    """out[M, N] = x[M, K] . w[N, K]^T (+ bias, epilogue epi) for M <= 64: lav_gemm_skinny_bf16"""
    res_bf16 = int(residual is not None and residual.dtype == bf16)
    L.check(L.lib.lav_gemm_skinny_bf16(_s(), M, N, K, _p(x), ldx or _ld(x), _p(w), _ld(w), _p(bias), epi, _p(residual),
                                        _ld(residual) if residual is not None else 0, res_bf16, _p(out), ldo or _ld(out)), "lav_gemm_skinny_bf16")
    return out


def attn_decode_desc(B, heads, q_len, Lv, n_cached, n_append, max_len, prefix_qkv, key_mask, qkv_new, cache_k, cache_v, out, partials=None):
    H = heads * 64
    return L.AttnDecodeDesc(B, heads, 64, q_len, Lv, n_cached, n_append, max_len, 0.125, _dp(prefix_qkv), 3 * H, _dp(key_mask), _dp(qkv_new),
                            3 * H, _dp(cache_k), _dp(cache_v), _dp(out), H, _dp(partials), partials.numel() if partials is not None else 0)


def attention_decode_splits(desc):
    return int(L.lib.lav_attention_decode_splits(C.byref(desc)))


def attention_decode(desc):
    L.check(L.lib.lav_attention_decode(_s(), C.byref(desc)), "lav_attention_decode")


def text_embed_rows(ids, pos_ids, Hd, word, pos, type0, gamma, beta, eps, out):
    n = ids.numel()
    L.check(L.lib.lav_text_embed_rows_fwd(_s(), n, Hd, _p(ids), _p(pos_ids), _p(word), _p(pos), _p(type0), _p(gamma), _p(beta), eps, _p(out)),
            "lav_text_embed_rows_fwd")
    return out


def greedy_step(logits, V, ids, cur, penalty, unfinished, score_sum, count, pad_id, eos_id, next_ids=None, ld_next=0):
    B = logits.shape[0]
    L.check(L.lib.lav_greedy_step(_s(), B, V, _p(logits), logits.stride(0), _p(ids), ids.stride(0), cur, float(penalty), _p(unfinished),
                                  _p(score_sum), _p(count), int(pad_id), int(eos_id), _p(next_ids), ld_next), "lav_greedy_step")


def bert_layer_decode(desc):
    L.check(L.lib.lav_bert_layer_decode(_s(), C.byref(desc)), "lav_bert_layer_decode")


# ---- beam search (csrc/decode.hip) ----------------------------------------------------------------------------------------------
BEAM_MAX = 8                                 # LAV_BEAM_MAX


def attention_decode_beam(desc, beams):
    L.check(L.lib.lav_attention_decode_beam(_s(), C.byref(desc), int(beams)), "lav_attention_decode_beam")


def bert_layer_decode_beam(desc, beams):
    L.check(L.lib.lav_bert_layer_decode_beam(_s(), C.byref(desc), int(beams)), "lav_bert_layer_decode_beam")


def beam_step(logits, V, ids, cur, penalty, beam_scores, beams, cand_score, cand_word):
    """per row: penalty in place, top 2 * beams of log_softmax + beam score -> cand_score / cand_word (rows, 2 * beams): lav_beam_step"""
    rows = logits.shape[0]
    L.check(L.lib.lav_beam_step(_s(), rows, int(beams), V, _p(logits), logits.stride(0), _p(ids), ids.stride(0), cur, float(penalty), _p(beam_scores),
                                _p(cand_score), _p(cand_word)), "lav_beam_step")


def beam_select_desc(clips, beams, keep, V, max_len, early_stopping, eos_id, pad_id, cand_score, cand_word, beam_scores, ids, parent, hyp_ids,
                     hyp_score, hyp_seq, state, worst, next_ids=None, ld_next=0):
    """the descriptor of lav_beam_select; cur, cur_norm and max_norm are set per step (beam_select)"""
    return L.BeamSelectDesc(clips, beams, keep, V, 0, max_len, int(bool(early_stopping)), 1.0, 1.0, int(eos_id), int(pad_id), _dp(cand_score),
                            _dp(cand_word), _dp(beam_scores), _dp(ids), ids.stride(0), _dp(next_ids), ld_next, _dp(parent), _dp(hyp_ids),
                            _dp(hyp_score), _dp(hyp_seq), _dp(state), _dp(worst))


def beam_select(desc, cur, cur_norm, max_norm):
    desc.cur, desc.cur_norm, desc.max_norm = cur, cur_norm, max_norm
    L.check(L.lib.lav_beam_select(_s(), C.byref(desc)), "lav_beam_select")


def beam_reparent_desc(src, dst, parent, max_len):
    """src / dst: lists of per-layer (k, v) caches (rows, heads, max_len, 64) bf16"""
    n = len(src)
    if n > L.REPARENT_MAX_LAYERS:
        raise ValueError(f"lav_beam_reparent: {n} layers, at most {L.REPARENT_MAX_LAYERS}")
    rows, heads = src[0][0].shape[:2]
    d = L.BeamReparentDesc(n, rows, heads, 0, max_len, _dp(parent))
    for i in range(n):
        d.src_k[i], d.src_v[i] = src[i][0].data_ptr(), src[i][1].data_ptr()
        d.dst_k[i], d.dst_v[i] = dst[i][0].data_ptr(), dst[i][1].data_ptr()
    return d


def beam_reparent(desc, n_pos):
    desc.n_pos = n_pos
    L.check(L.lib.lav_beam_reparent(_s(), C.byref(desc)), "lav_beam_reparent")


# ---- retrieval evaluation (csrc/retrieval.hip, csrc/stages.cpp) ----------------------------------------------------------------------
def attention_rows(qkv, n, seq_len, heads, key_mask, q_row, out=None, scale=0.125):
    """(n, heads * 64) bf16: attention of row q_row[s] of every sequence s over its L keys (qkv (n * L, 3 hidden) bf16, key_mask (n, L) int32,
    q_row (n,) int32, both on the device): lav_attention_rows"""
    H = heads * 64
    if out is None:
        out = torch.empty((n, H), dtype=bf16, device=qkv.device)
    L.check(L.lib.lav_attention_rows(_s(), n, seq_len, heads, 64, _p(qkv), _ld(qkv), _p(key_mask), _p(q_row), float(scale), _p(out), _ld(out)),
            "lav_attention_rows")
    return out


def bert_layer_fwd_rows(desc):
    L.check(L.lib.lav_bert_layer_fwd_rows(_s(), C.byref(desc)), "lav_bert_layer_fwd_rows")


def mlm_pair_readout(desc):
    L.check(L.lib.lav_mlm_pair_readout(_s(), C.byref(desc)), "lav_mlm_pair_readout")


def retrieval_rank(S, gt, out=None):
    """(n_text,) int32 1-based rank of column gt[t] in row t of the fp32 score matrix S (stable, NaN last): lav_retrieval_rank"""
    nt, nv = S.shape
    if out is None:
        out = torch.empty(nt, dtype=torch.int32, device=S.device)
    L.check(L.lib.lav_retrieval_rank(_s(), nt, nv, _p(S), _ld(S), _p(gt), _p(out)), "lav_retrieval_rank")
    return out


# ---- video-QA read-out (csrc/qa.hip) ------------------------------------------------------------------------------------------------------
ANSWER_MAX_CAND, ANSWER_MAX_SPLITS = 32, 16          # LAV_ANSWER_MAX_CAND, LAV_ANSWER_MAX_SPLITS
# column ranges per row of lav_answer_readout (probe hook; every value gives identical outputs).  1: one workgroup per row, one launch.
# Measured at (32 x 30522) back to back (profiles/r13_qa_bench.json): bf16 8.83 us at 1, 8.11 us at 8; fp32 10.41 / 8.25 us.  The
# 0.7 us do not pay for the workspace allocation a split adds to a call whose host side costs 14-16 us: the default stays 1.
ANSWER_SPLITS = int(_os_env("LAV_QA_SPLITS", "1"))


def answer_readout(logits, V, labels, cand=(), splits=None, out=None):
    """(pred, rank, choice), each (n,) int32 on the device, of the n rows of a (n, V) bf16 / fp32 logits view (lav_answer_readout: arg-max column,
    number of columns sorting before the label, arg-max of the candidates' share of their sum).  labels: (n,) label columns, -1 = none -- a host
    array (numpy / CPU tensor: checked against [0, V) by the entry, then uploaded -- a copy from pageable host memory, which the runtime stages
    and which may wait for that staging, not for the kernels queued before it) or an int32 device tensor (the caller vouches
    for its values).  cand: up to 32 token ids on the host.  out: a (3, n) int32 device tensor to write into."""
    import numpy as np
    assert logits.dim() == 2 and logits.stride(-1) == 1 and logits.dtype in (bf16, torch.float32), "logits: a (n, V) bf16 / fp32 view with unit column stride"
    n, dev = logits.shape[0], logits.device
    if isinstance(labels, torch.Tensor) and labels.is_cuda:
        assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == n
        lab_dev, lab_host = labels, None
    else:
        lab_np = np.ascontiguousarray(labels.numpy() if isinstance(labels, torch.Tensor) else labels, dtype=np.int32).reshape(-1)
        assert lab_np.size == n, (lab_np.size, n)
        lab_dev, lab_host = torch.from_numpy(lab_np).to(dev, non_blocking=True), lab_np.ctypes.data_as(C.c_void_p)
    cand_np = np.ascontiguousarray(list(cand), dtype=np.int32)
    splits = ANSWER_SPLITS if splits is None else int(splits)
    if out is None:
        out = torch.empty((3, n), dtype=torch.int32, device=dev)
    assert out.dtype == torch.int32 and out.shape == (3, n) and out.is_contiguous()
    need = int(L.lib.lav_answer_readout_workspace_bytes(n, splits))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    L.check(L.lib.lav_answer_readout(_s(), n, int(V), _p(logits), _ld(logits), int(logits.dtype == torch.float32), _p(lab_dev), lab_host,
                                     cand_np.ctypes.data_as(C.c_void_p) if cand_np.size else None, int(cand_np.size), splits, _p(ws), need,
                                     _p(out[0]), _p(out[1]), _p(out[2])), "lav_answer_readout")
    return out[0], out[1], out[2]


def match_readout(logits, G, O, true_col, false_col, row=None, gt=None, want_score=False, out=None):
    """(choice (G,) int32, hit (G,) int32 or None, score (G * O,) fp32 or None) on the device: lav_match_readout over G groups of O candidates of
    a (n_rows, width) bf16 / fp32 logits view -- s = t / (t + f) of columns true_col / false_col of row[k] (row None: row k), choice = arg-max of
    s over a group (NaN above every number, lowest o on a tie), hit = choice == gt.  row / gt: host arrays (checked here: a row outside
    [0, n_rows) raises ValueError; then uploaded) or int32 device tensors (the caller vouches; the kernel reads nothing for a row outside the
    block).  out: a (2, G) int32 device tensor for (choice, hit)."""
    import numpy as np
    if not (logits.dim() == 2 and logits.stride(-1) == 1 and logits.dtype in (bf16, torch.float32)):
        raise ValueError("match_readout: logits must be a (rows, width) bf16 / fp32 view with unit column stride")
    G, O = int(G), int(O)
    n_rows, width = logits.shape
    dev = logits.device
    if not (0 <= int(true_col) < width and 0 <= int(false_col) < width):
        raise ValueError(f"match_readout: columns {true_col} / {false_col} outside the {width} columns of the logits")

    def dev_i32(a, n, what):
        if a is None:
            return None
        if isinstance(a, torch.Tensor) and a.is_cuda:
            if not (a.dtype == torch.int32 and a.is_contiguous() and a.numel() == n):
                raise ValueError(f"match_readout: a device {what} must be a contiguous int32 tensor of {n} entries")
            return a
        a = np.ascontiguousarray(a.numpy() if isinstance(a, torch.Tensor) else a).reshape(-1)
        if a.size != n:
            raise ValueError(f"match_readout: {what} has {a.size} entries, expected {n}")
        if what == "row" and a.size and (a.min() < 0 or a.max() >= n_rows):
            raise ValueError(f"match_readout: row entry outside the {n_rows} rows of the logits")
        return torch.from_numpy(a.astype(np.int32)).to(dev, non_blocking=True)

    row_d, gt_d = dev_i32(row, max(G, 0) * max(O, 0), "row"), dev_i32(gt, max(G, 0), "gt")
    if out is None:
        out = torch.empty((2, max(G, 1)), dtype=torch.int32, device=dev)       # a G < 1 is the entry's to reject
    elif not (out.dtype == torch.int32 and out.shape == (2, G) and out.is_contiguous()):
        raise ValueError(f"match_readout: out must be a contiguous (2, {G}) int32 tensor")
    score = torch.empty(max(G, 0) * max(O, 0), dtype=torch.float32, device=dev) if want_score else None
    L.check(L.lib.lav_match_readout(_s(), G, O, _p(logits), _ld(logits), int(logits.dtype == torch.float32), _p(row_d), n_rows, int(true_col),
                                    int(false_col), _p(gt_d), _p(score), _p(out[0]), _p(out[1]) if gt_d is not None else None), "lav_match_readout")
    return out[0], (out[1] if gt_d is not None else None), score
