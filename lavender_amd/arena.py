"""Flat parameter / gradient arena.

MI355X-first replacement for per-tensor parameter storage: every parameter of the model lives in ONE fp32
master buffer (in execution order, 64-element aligned), mirrored by ONE bf16 working copy (what the MFMA GEMMs
read) and ONE fp32 gradient buffer (what the backward kernels atomically accumulate into).  Consequences:
  * the optimizer (agent.py:241-250) is two kernel launches over the whole arena (sum of squares + fused
    clip/AdamW/bf16 refresh) instead of ~220 per-tensor updates;
  * data-parallel gradient exchange (agent.py:261-265) is RCCL all-reduce on contiguous slices -- buckets are
    plain views, no flatten/unflatten copies;
  * query/key/value weights of a BERT layer are adjacent, so the fused (2304, 768) QKV GEMM needs no concat.
nn.Parameter objects stay the public surface (same names/shapes as the reference state_dict): their .data are
views of the master buffer and their .grad are views of the gradient buffer.
"""
import os
import re

import torch

from . import hip as K

# First-touch weight gradients (round 6): the weight MATRICES are not zeroed per step -- their first writer of a step (a layout-2 GEMM) ASSIGNS
# (lav_gemm_epilogue.assign) instead of reading, adding and writing back; only the atomically accumulated rest of the arena (vectors, tables:
# ~1 % of it) is zeroed, by one launch over a block list.  Saves the 886 MB fill and the 870 MB read of the read-modify-write per step.
# LAV_FIRST_TOUCH=0 restores the whole-arena fill + accumulate.
FIRST_TOUCH = os.environ.get("LAV_FIRST_TOUCH", "1") != "0"


class FtUnit:
    """One first-touch range of the gradient arena (a weight matrix; the fused q | k | v block of a BERT attention is one unit).
    state 0 CLEAN: memory is zero (never written, or zeroed by finish) -- the next writer may assign or accumulate;
          1 ARMED: memory holds the LAST step's gradient -- the first writer must assign (take() says so), anything else zeroes first;
          2 WRITTEN: this step's gradient so far -- further writers accumulate."""
    __slots__ = ("arena", "lo", "hi", "state")

    def __init__(self, arena, lo, hi):
        self.arena, self.lo, self.hi, self.state = arena, lo, hi, 0

    def take(self):
        """called by the writer that can assign: True = assign (first writer since zero_grad), False = accumulate"""
        if self.state == 2:
            return False
        if self.state == 1:
            self.arena._ft_armed -= 1
        self.state = 2
        return True

    def before_accumulate(self):
        """called on behalf of a writer that can only accumulate (atomics, an un-converted call site): the memory must be valid"""
        if self.state == 1:
            self.arena.grad[self.lo:self.hi].zero_()
            self.arena._ft_armed -= 1
        self.state = 2

ALIGN = 64
SLACK = 64 * 1024
# parameters that never receive a gradient on the paths built here (after one pretrain step exactly these
# have grad None in the reference, so torch.optim.AdamW never touches them -- no weight decay either); bit 2 of block_group
NO_GRAD_PARAMS = ("emb_task", "enc_img.emb_odr")


def no_grad_params(module):
    """NO_GRAD_PARAMS of this model: with args.enable_task_token the task-token table is read by every task-token pass and is an ordinary
    parameter (AdamW updates and decays all its rows, group "other/decay", as torch.optim.AdamW does in the reference)"""
    args = getattr(module, "args", None)
    if getattr(args, "enable_task_token", False):
        return tuple(n for n in NO_GRAD_PARAMS if n != "emb_task")
    return NO_GRAD_PARAMS
_QKV = re.compile(r"(.*attention\.self)\.(query|key|value)\.(weight|bias)$")


def param_group_of(name):
    """Agent_Base.build_optimizer grouping (agent.py:96-120), by substring on the unwrapped name:
    0 swin/decay, 1 other/decay, 2 swin/no-decay, 3 other/no-decay."""
    nd = any(s in name for s in ("bias", "LayerNorm.bias", "LayerNorm.weight"))
    return (2 if nd else 0) + (0 if "swin." in name else 1)


def _order(named):
    """execution order = registration order, except q/k/v of one attention are regrouped [wq wk wv bq bk bv]."""
    out, i = [], 0
    named = list(named)
    while i < len(named):
        m = _QKV.match(named[i][0])
        if m:
            pre = m.group(1)
            blk = [x for x in named[i:i + 6] if x[0].startswith(pre + ".")]
            assert len(blk) == 6, f"unexpected attention parameter layout near {named[i][0]}"
            d = dict(blk)
            for kind in ("weight", "bias"):
                for n in ("query", "key", "value"):
                    out.append((f"{pre}.{n}.{kind}", d[f"{pre}.{n}.{kind}"]))
            i += 6
        else:
            out.append(named[i])
            i += 1
    return out


class ParamArena:
    def __init__(self, module, device):
        named = _order(module.named_parameters())
        self.device = torch.device(device)
        self.names, self.offsets, self.numels = [], {}, {}
        off = 0
        for n, p in named:
            self.names.append(n)
            self.offsets[n] = off
            self.numels[n] = p.numel()
            off += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
        self.total = off
        # SLACK zero elements past the last parameter: a GEMM may read a weight matrix with its row count rounded up to the
        # k-tile (the vocabulary projection as a (30528, H) operand) without leaving the buffer; never written, never stepped
        self.master = torch.zeros(off + SLACK, dtype=torch.float32, device=self.device)[:off]
        self.half_full = torch.zeros(off + SLACK, dtype=torch.bfloat16, device=self.device)
        self.half = self.half_full[:off]
        # same slack behind the gradients: the ZeRO-1 reduce-scatter works on world x shard elements (shard = the arena
        # split into 64-aligned equal parts), which may reach a few blocks past the last parameter
        self.grad_full = torch.zeros(off + SLACK, dtype=torch.float32, device=self.device)
        self.grad = self.grad_full[:off]
        grp = torch.zeros(off // ALIGN, dtype=torch.uint8)
        no_grad = no_grad_params(module)
        self.params = {}
        for n, p in named:
            o, k = self.offsets[n], p.numel()
            self.master[o:o + k].copy_(p.data.reshape(-1).to(self.device, torch.float32))
            p.data = self.master[o:o + k].view(p.shape)
            p.grad = self.grad[o:o + k].view(p.shape)
            p._lav16 = self.half[o:o + k].view(p.shape)
            p._lavg = p.grad
            p._lav_name = n
            grp[o // ALIGN:(o + k + ALIGN - 1) // ALIGN] = param_group_of(n) | (4 if n in no_grad else 0)
            self.params[n] = p
        self.block_group = grp.to(self.device)
        self._build_transposed(named)
        self._build_first_touch(named)
        self.m = None
        self.v = None
        self.gradsq = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.anchor = torch.zeros(1, dtype=torch.float32, device=self.device, requires_grad=True)
        self.listeners = []          # callables(event_name): e.g. the data-parallel reducer
        self.stale = True
        self.sync_half()

    # -- transposed bf16 copy of the weight matrices ---------------------------------------------------
    def _build_transposed(self, named):
        """W^T next to W for every nn.Linear-style weight (2-D, not an embedding / bias table): the input-gradient GEMMs
        dx = dy W then read a K-contiguous operand like the forward ones.  q/k/v of one attention form ONE (3H, H)
        matrix (they are adjacent in the arena), so its transpose is the (H, 3H) operand of the fused backward GEMM."""
        import ctypes as C
        import numpy as np
        from ._lib import MatDesc
        mats, off_t, tile0 = [], 0, 0
        skip = ("embeddings", "relative_position_bias_table", "emb_", ".key.weight", ".value.weight")
        for n, p in named:
            if p.dim() != 2 or not n.endswith("weight") or any(k in n for k in skip) or p.shape[0] < 8 or p.shape[1] % 8:
                continue
            rows, cols = p.shape
            if _QKV.match(n):
                rows *= 3                                       # query.weight heads the fused (3H, H) block
            ld = (rows + 63) // 64 * 64
            mats.append((n, self.offsets[n], off_t, rows, cols, ld, tile0))
            tile0 += ((rows + 63) // 64) * ((cols + 63) // 64)
            off_t += (cols * ld + ALIGN - 1) // ALIGN * ALIGN
        self.half_t = torch.zeros(max(off_t, ALIGN), dtype=torch.bfloat16, device=self.device)
        self._t_tiles = tile0
        self._t_views = {}
        arr = (MatDesc * max(len(mats), 1))()
        for i, (n, so, do, rows, cols, ld, t0) in enumerate(mats):
            arr[i] = MatDesc(so, do, rows, cols, ld, t0)
            self._t_views[n] = self.half_t[do:do + cols * ld].view(cols, ld)
        self._t_n = len(mats)
        raw = np.frombuffer(bytes(arr), dtype=np.uint8).copy()
        self._t_desc = torch.from_numpy(raw).to(self.device)
        for n, p in named:
            if n in self._t_views:
                rows = p.shape[0] * (3 if _QKV.match(n) else 1)
                p._lav16t = self._t_views[n][:, :rows]

    # -- first-touch units ----------------------------------------------------------------------------
    def _build_first_touch(self, named):
        """Units = the matrices whose gradient a layout-2 GEMM writes first: every nn.Linear-style weight (the ones with a transposed copy; q | k | v of
        a BERT attention as ONE unit: the fused GEMM writes all three), the tied word-embedding / decoder matrix and the patch-embedding kernel."""
        import numpy as np
        self.ft_units, self._ft_armed = [], 0
        covered = np.zeros(self.total // ALIGN, dtype=bool)
        if FIRST_TOUCH and self.device.type == "cuda":
            d = dict(named)
            for n, p in named:
                if not (n in self._t_views or n.endswith("word_embeddings.weight") or n.endswith("patch_embed.proj.weight")):
                    continue
                members = [n]
                if _QKV.match(n):
                    members = [n, n.replace(".query.", ".key."), n.replace(".query.", ".value.")]
                lo = self.offsets[members[0]]
                hi = self.offsets[members[-1]] + (self.numels[members[-1]] + ALIGN - 1) // ALIGN * ALIGN
                if hi - lo < 16384 or any(m not in d for m in members):
                    continue
                u = FtUnit(self, lo, hi)
                self.ft_units.append(u)
                covered[lo // ALIGN:hi // ALIGN] = True
                for m in members:
                    d[m]._lav_ft = u
        self._zero_blocks = torch.from_numpy(np.nonzero(~covered)[0].astype(np.int32)).to(self.device)
        from .engine import register_arena
        register_arena(self)

    def finish_first_touch(self, lo=0, hi=None):
        """Gradients in [lo, hi) are about to be read (gradient exchange, norm, optimizer, the user after backward()): a unit that is still ARMED
        was not written in this step -- its memory is last step's gradient -- and becomes zero.  O(1) when every unit was written."""
        if not self._ft_armed:
            return
        hi = self.total if hi is None else hi
        for u in self.ft_units:
            if u.state == 1 and u.lo < hi and u.hi > lo:
                self.grad[u.lo:u.hi].zero_()
                u.state = 0
                self._ft_armed -= 1

    def sync_transposed(self):
        if self._t_n:
            K.transpose_batched(self._t_n, self._t_desc, self._t_tiles, self.half_full, self.half_t)

    # -- bf16 working copy -------------------------------------------------------------------------
    # ZeRO-1 (dp.ZeroOneReducer): after a sharded optimizer step only this rank's slice of the fp32 master is current until
    # dp.gather_master() -- a collective, so it cannot be triggered from a single rank's read.  Readers of the master check this.
    masters_sharded = False

    def require_full_master(self, what):
        if self.masters_sharded:
            raise RuntimeError(f"{what}: the fp32 masters are sharded across ranks (ZeRO-1 step taken); call "
                               "agent.dp.gather_master() on EVERY rank first (Agent_Base.save_model does)")

    def sync_half(self):
        """Refresh the bf16 working copies from the fp32 master (after load_state_dict / a foreign optimizer)."""
        self.require_full_master("ParamArena.sync_half")
        K.cast_bf16(self.master, self.half, self.total)
        self.sync_transposed()
        self.stale = False

    def sync_half_if_stale(self):
        if self.stale:
            self.sync_half()

    def owns(self, p):
        n = getattr(p, "_lav_name", None)
        return n is not None and p.data_ptr() == self.master.data_ptr() + 4 * self.offsets[n]

    def fused_view(self, first, rows_total):
        """(rows_total, cols) bf16 / grad views starting at parameter `first` (adjacent q,k,v weights)."""
        o = self.offsets[first._lav_name]
        cols = first.shape[1] if first.dim() == 2 else 1
        n = rows_total * cols
        shape = (rows_total, cols) if first.dim() == 2 else (rows_total,)
        return self.half[o:o + n].view(shape), self.grad[o:o + n].view(shape), self.master[o:o + n].view(shape)

    def span(self, names):
        """[start, end) arena range covering the given parameter names (for gradient buckets)."""
        lo = min(self.offsets[n] for n in names)
        hi = max(self.offsets[n] + (self.numels[n] + ALIGN - 1) // ALIGN * ALIGN for n in names)
        return lo, hi

    def notify(self, event):
        if self.listeners and self.grad.is_cuda:
            from . import hip as K
            K.layernorm_flush()                               # a range of gradients is final: complete its queued LayerNorm column reductions first
        for f in self.listeners:
            f(event)

    # -- optimizer ---------------------------------------------------------------------------------
    def zero_grad(self):
        from .engine import dw_join
        dw_join()
        if self.ft_units:
            K.zero_blocks(self.grad_full, self._zero_blocks, ALIGN)      # vectors and tables (atomic accumulation); the matrices are assigned by their first writer
            # a listener (the data-parallel reducer) may have written into a CLEAN unit after finish_first_touch zeroed it -- an all-reduce
            # lands the other ranks' gradient there -- so with listeners attached every unit is re-armed, whoever wrote its memory
            rearm_all = bool(self.listeners)
            n = 0
            for u in self.ft_units:
                if u.state or rearm_all:                      # WRITTEN (or still ARMED, or possibly written by a listener): stale from here on
                    u.state = 1
                    n += 1
            self._ft_armed = n
        else:
            self.grad_full.zero_()
        for p in self.params.values():
            if p.grad is None or p.grad.data_ptr() != p._lavg.data_ptr():
                p.grad = p._lavg

    def adamw_step(self, lr4, wd4, step, max_norm, grad_div=1.0, betas=(0.9, 0.98), eps=1e-8, shard=None, sum_gradsq=None):
        """One fused clip + AdamW + bf16-refresh launch.  shard = (lo, hi): ZeRO-1 -- this rank owns (and keeps the
        optimizer state of) arena elements [lo, hi) only; `sum_gradsq(t)` then sums the 1-element squared-norm tensor over
        the ranks (each contributes its own shard of the already reduced gradient)."""
        from .engine import dw_join
        dw_join()                                             # weight-gradient kernels run on a side stream
        lo, hi = (0, self.total) if shard is None else shard
        n = hi - lo
        if self.m is None or self.m.numel() != n:
            self.m = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.v = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.gradsq.zero_()
        if n <= 0:
            if max_norm > 0 and sum_gradsq is not None:
                sum_gradsq(self.gradsq)
            return
        if max_norm > 0:
            K.sumsq(self.grad[lo:hi], n, self.gradsq)
            if sum_gradsq is not None:
                sum_gradsq(self.gradsq)
        K.adamw(n, self.master[lo:hi], self.grad[lo:hi], self.m, self.v, self.half[lo:hi], self.block_group[lo // ALIGN:hi // ALIGN],
                lr4, wd4, betas[0], betas[1], eps, step, self.gradsq if max_norm > 0 else None, max_norm, grad_div)
        if shard is None:
            self.sync_transposed()
