"""GPU: lav_gemm_bf16 / lav_gemm_tn_grouped on every route of the kernel selector against the float64 reference of tests/gemm_bounds.py (per-element
bound, per-tile check against the rounding model).  Each case names the kernels it must reach; the launch is captured with torch.profiler (kernel
names only) and the names must match both the case and the host copy of the selector (gemm_bounds.route).  Variants are forced in-process with
lav_gemm_select (2 = ping-pong TN, 7 = h192, 9 = h192l, 11 = phase-shifted), restored afterwards."""
import re

import pytest
import torch

from tests import gemm_bounds as GB
from tests.helpers import hidden_keep_multiplier

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
SEL = {"ps": 11, "h192": 7, "h192l": 9, "pp_tn": 2}

# id: (layout, M, N, K, epilogue, splits, selector overrides, expected kernels)
CASES = {
    "small_l0_tail1": (0, 2049, 256, 96, dict(bias=True), 1, {}, ["gemm_kernel"]),
    "small_l1_generic_relu_ragged": (1, 193, 130, 192, dict(act=2, preact="grad", gelu_in="value", colsum=True, out="fp32", ldc_pad=8), 1, {}, ["gemm_kernel"]),
    "splitk_small": (0, 255, 512, 3008, dict(), 4, {}, ["gemm_kernel", "splitk_reduce_bf16_kernel"]),
    "splitk_huge_cancel": (1, 513, 512, 6016, dict(cancel=True), 4, {}, ["gemm_huge_kernel", "splitk_reduce_bf16_kernel"]),
    "splitk_collapsed_to_big": (0, 2049, 256, 64, dict(), 4, {}, ["gemm_big_kernel"]),
    "big_vocab_tail": (0, 2049, 1002, 128, dict(bias=True, c_pad=True), 1, {}, ["gemm_big_kernel"]),
    "big_l1_S_BG": (1, 2049, 256, 64, dict(bias=True, act=1), 1, {}, ["gemm_big_kernel"]),
    "big_l0_S_GC_byte": (0, 2049, 256, 64, dict(gelu_in="byte", rscale=True, colsum=True), 1, {}, ["gemm_big_kernel"]),
    "huge_l1_EF_ALL": (1, 4289, 2048, 64, dict(bias=True, act=1, preact="value", drop=True, res=True), 1, {}, ["gemm_huge_kernel"]),
    "ps256_S_B": (0, 20481, 768, 64, dict(bias=True), 1, {}, ["gemm_ps_kernel"]),
    "huge_l0_S_B_ps_off": (0, 20481, 768, 64, dict(bias=True), 1, {"ps": 0}, ["gemm_huge_kernel"]),
    "huge_l1_S_GC": (1, 20481, 768, 64, dict(gelu_in="grad", rscale=True, colsum=True), 1, {}, ["gemm_huge_kernel"]),
    "ps256_S_BDRO_resln": (0, 20481, 768, 64, dict(bias=True, drop=True, rscale=True, res="ln", out="fp32"), 1, {}, ["gemm_ps_kernel"]),
    "ps256_fp16_saturating": (0, 20481, 768, 64, dict(bias=True, res="fp16", out="fp16", big=True), 1, {}, ["gemm_ps_kernel"]),
    "ps192_S_BG_preact": (0, 4289, 2048, 64, dict(bias=True, act=1, preact="grad"), 1, {}, ["gemm_ps_kernel"]),
    "ps192_S_BDR": (0, 4289, 2048, 64, dict(bias=True, drop=True, rscale=True, res=True), 1, {}, ["gemm_ps_kernel"]),
    "h192l_S_BG_byte": (0, 4289, 2048, 64, dict(bias=True, act=1, preact="byte"), 1, {"ps": 0}, ["gemm_h192l_kernel"]),
    "h192_l0_S_GC": (0, 4289, 2048, 64, dict(gelu_in="grad", rscale=True, colsum=True), 1, {"ps": 0, "h192l": 0}, ["gemm_h192_kernel"]),
    "h192_l1_S_BDRO": (1, 4289, 2048, 64, dict(bias=True, drop=True, rscale=True, res="fp32", out="fp32"), 1, {}, ["gemm_h192_kernel"]),
    "headmajor_big": (0, 2049, 768, 64, dict(bias=True, headmajor=(12, 64)), 1, {}, None),
    "rowmap_ps": (0, 4096, 512, 128, dict(bias=True, res=True, a_rowmap=True), 1, {}, ["gemm_ps_kernel"]),
    "rowmap_huge": (0, 4096, 512, 128, dict(bias=True, res=True, a_rowmap=True), 1, {"ps": 0}, ["gemm_huge_kernel"]),
    "over_2gib_operand": (0, 1400000, 768, 768, dict(bias=True), 1, {}, ["gemm_huge_kernel"]),
    # weight gradients (layout 2, fp32 C accumulated)
    "tn_ragged_k_split": (2, 768, 768, 4100, dict(out="acc", rowsum=True), 3, {}, ["gemm_pp_kernel", "tn_reduce_kernel", "gemm_kernel"]),
    "tn_pp_owner_assign": (2, 512, 512, 2048, dict(out="acc", assign=True), 1, {}, ["gemm_pp_kernel"]),
    "tn_pp_only_k32_keep": (2, 1024, 512, 7840, dict(out="acc", k_keep_rpg=245, alpha=1.25, rowsum=True), 3, {}, ["gemm_pp_kernel", "tn_reduce_kernel"]),
    "tn_huge_pp_off_cancel": (2, 512, 512, 1024, dict(out="acc", assign=True, cancel=True), 3, {"pp_tn": 0}, ["gemm_huge_kernel", "tn_reduce_kernel"]),
    "tn_big_n384": (2, 512, 384, 1024, dict(out="acc", k_keep_rpg=256), 11, {}, ["gemm_big_kernel", "tn_reduce_kernel"]),
    "tn_small_m130": (2, 130, 256, 1024, dict(out="acc", rowsum=True), 11, {}, ["gemm_kernel", "tn_reduce_kernel"]),
    "tn_small_m192_assign": (2, 192, 256, 2048, dict(out="acc", assign=True), 1, {}, ["gemm_kernel"]),
    "tn_atomics_ragged_n": (2, 264, 130, 512, dict(out="acc", ldc_pad=4), 3, {}, ["gemm_big_kernel"]),
    "tn_generic_epilogue": (2, 200, 256, 512, dict(out="fp32"), 1, {}, ["gemm_kernel"]),
}

# every large-tile kernel of layouts 0 / 1 with every epilogue feature set it is instantiated for (the gemm_kernels table
# in gemm.hip).  Dropout cases store through a padded ldc (the mask index is row * N + col, not row * ldc + col); M tails of 191 and 255
# rows past a 256-row multiple; A read through a strided view on the 256 x 128 and 192-row kernels.
FSETS = {
    "S_B": dict(bias=True),
    "S_BG": dict(bias=True, act=1, preact="grad"),
    "S_GC": dict(gelu_in="byte", rscale=True, colsum=True),
    "S_BDR": dict(bias=True, drop=True, rscale=True, res=True, ldc_pad=8),
    "S_BDRO": dict(bias=True, drop=True, rscale=True, res="ln", out="fp32", ldc_pad=8),
    "S_BDRO16": dict(bias=True, drop=True, rscale=True, res="fp16", out="fp16", ldc_pad=8),
    "EF_ALL": dict(act=2, preact="grad", gelu_in="value", drop=True, colsum=True, ldc_pad=8),
}
LARGE = {   # kernel, tile rows: (layout, M, N, K, selector overrides, extra epilogue, feature sets)
    ("gemm_big_kernel", 256): (0, 8 * 256 + 191, 264, 64, {}, dict(lda_pad=64), ("S_B", "S_BG", "S_GC", "S_BDR", "S_BDRO16", "EF_ALL")),
    ("gemm_huge_kernel", 256): (0, 80 * 256 + 255, 768, 64, {"ps": 0}, {}, ("S_B", "S_BG", "S_GC", "S_BDR", "S_BDRO", "EF_ALL")),
    ("gemm_ps_kernel", 256): (0, 80 * 256 + 191, 768, 64, {}, {}, ("S_B", "S_BG", "S_GC", "S_BDR", "S_BDRO")),
    ("gemm_ps_kernel", 192): (0, 4289, 2048, 64, {}, dict(lda_pad=32), ("S_B", "S_BG", "S_GC", "S_BDR", "S_BDRO16")),
    ("gemm_h192l_kernel", 192): (0, 4289, 2048, 64, {"ps": 0}, {}, ("S_B", "S_BG", "S_GC", "S_BDR", "S_BDRO")),
    ("gemm_h192_kernel", 192): (1, 4289, 2048, 64, {}, dict(lda_pad=64), ("S_B", "S_BG", "S_GC", "S_BDR", "S_BDRO16")),
}
for (_k, _rows), (_lay, _M, _N, _K, _over, _extra, _fs) in LARGE.items():
    for _f in _fs:
        _e = dict(FSETS[_f], **_extra)
        _n = _N
        if _f == "EF_ALL" and _k == "gemm_big_kernel":
            _n = 1001                                        # ragged 8-column chunks (N % 8 != 0) on a large-tile kernel
        CASES[f"matrix_{_k[5:-7]}{_rows}_{_f}"] = (_lay, _M, _n, _K, _e, 1, _over, [_k])
# weight gradients: every layout-2 route with splits 1 (owner), 3 (workspace reduce) and 11 (collapsed by the kps rounding), assign onto a C of
# NaN at splits 1 and 11, the drop-path k_keep and the fused rowsum_a
TN = {   # route: (M, N, K, k_keep rows per group, selector overrides, kernel)
    "pp": (768, 512, 2048, 256, {}, "gemm_pp_kernel"),
    "pp_only_k32": (1024, 512, 7840, 245, {}, "gemm_pp_kernel"),
    "huge_pp_off": (512, 512, 1024, 256, {"pp_tn": 0}, "gemm_huge_kernel"),
    "big_n384": (512, 384, 1024, 256, {}, "gemm_big_kernel"),
    "small_m130": (130, 256, 1024, 256, {}, "gemm_kernel"),
    "small_m192_n256": (192, 256, 2048, 256, {}, "gemm_kernel"),
    "ragged_k": (768, 768, 4100, 0, {}, "gemm_pp_kernel"),
    "atomics_ragged_n": (264, 130, 512, 256, {}, "gemm_big_kernel"),
}
for _r, (_M, _N, _K, _rpg, _over, _k) in TN.items():
    for _sp in (1, 3, 11):
        _assign = _sp != 3 and not (_N % 4 and _sp > 1)     # assign with split-K needs the workspace reduction (N % 4 == 0)
        _e = dict(out="acc", assign=_assign, rowsum=True, alpha=1.25 if _sp == 3 else 1.0, ldc_pad=4 if _N % 4 else 0)
        if _rpg:
            _e["k_keep_rpg"] = _rpg
        CASES[f"tn_{_r}_splits{_sp}"] = (2, _M, _N, _K, _e, _sp, _over, [_k])
GEMM_KERNELS = ("gemm_kernel", "gemm_big_kernel", "gemm_huge_kernel", "gemm_h192_kernel", "gemm_h192l_kernel", "gemm_ps_kernel", "gemm_pp_kernel",
                "gemm_pp_group_kernel", "splitk_reduce_bf16_kernel", "tn_reduce_kernel", "tn_reduce_group_kernel")


def _rb(shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(bf16)


def _names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def _has(names, k):
    pat = re.compile(r"(?<![A-Za-z0-9_])" + re.escape(k) + r"(?![A-Za-z0-9_])")
    return any(pat.search(n) for n in names)


def _mn(M, N, dtype, fill=0.0):
    """an (M, N) view of a buffer whose rows are padded to 16 elements (the epilogues read and write 8-element chunks)"""
    return torch.full((M, (N + 15) // 16 * 16), fill, dtype=dtype, device="cuda")[:, :N]


def _launched(names):
    """the GEMM-family kernels among the launches"""
    return {k for k in GEMM_KERNELS if _has(names, k)}


def _ps_rows(names):
    """row tiles of the phase-shifted launches, from the template argument RF (gemm_ps_kernel<F, RF>: 8 -> 256 rows, 6 -> 192 rows)"""
    out = set()
    for n in names:
        m = re.search(r"gemm_ps_kernel<[^<>]*?(\d+)>", n)
        if m:
            out.add({8: 256, 6: 192}.get(int(m.group(1)), -1))
    return out


def _select(over):
    from lavender_amd import hip
    return {k: hip.gemm_select(SEL[k], int(v)) for k, v in over.items()}


def _restore(old):
    from lavender_amd import hip
    for k, v in old.items():
        hip.gemm_select(SEL[k], v)


def _operands(layout, M, N, K, epi, seed):
    """kernel operands + the float64 a (M, K), b (K, N) they hold.  cancel: the second half of the contraction repeats the first with the sign
    of b flipped plus a small perturbation, so |a||b| is much larger than |ab|"""
    if epi.get("cancel"):
        h = K // 2
        a0, b0 = _rb((M, h), seed, 0.5), _rb((h, N), seed + 1, 0.5)
        a_ = torch.cat([a0, a0], 1)
        b_ = torch.cat([b0, (-b0.float() + 0.01 * torch.randn(h, N, device="cuda")).to(bf16)], 0)
    else:
        a_, b_ = _rb((M, K), seed, 0.5), _rb((K, N), seed + 1, 0.5)
    pad = lambda n: (n + 7) // 8 * 8
    if layout != 2 and epi.get("lda_pad"):                   # A as a strided view: lda > K
        A = torch.zeros(M, K + epi["lda_pad"], dtype=bf16, device="cuda")
        A[:, :K] = a_
        a_ = A[:, :K]
    if layout == 0:
        A, B = a_, b_.t().contiguous()
    elif layout == 1:
        A = a_
        B = torch.zeros(K, pad(N), dtype=bf16, device="cuda")
        B[:, :N] = b_
        B = B[:, :N]
    else:
        A = torch.zeros(K, pad(M), dtype=bf16, device="cuda")
        A[:, :M] = a_.t()
        A = A[:, :M]
        B = torch.zeros(K, pad(N), dtype=bf16, device="cuda")
        B[:, :N] = b_
        B = B[:, :N]
    return A, B, a_.double(), b_.double()


def _run_case(cid):
    from lavender_amd import hip
    layout, M, N, K, epi, splits, over, want = CASES[cid]
    seed = sum(map(ord, cid))
    A, B, a, b = _operands(layout, M, N, K, epi, seed)
    out = epi.get("out", "bf16")
    kw, ref_kw = {}, dict(alpha=epi.get("alpha", 1.0), act=epi.get("act", 0), preact=epi.get("preact"), colsum=bool(epi.get("colsum")),
                          out=out, splits=splits, assign=bool(epi.get("assign")), rowsum=bool(epi.get("rowsum")))
    kw["alpha"] = ref_kw["alpha"]
    if epi.get("big"):
        A = (A.float() * 40000).to(bf16)
        a = A.double() if layout != 2 else a
    if epi.get("a_rowmap"):
        perm = torch.randperm(M, generator=torch.Generator().manual_seed(seed)).to(torch.int32).cuda()
        kw["a_rowmap"] = perm
        a = a[perm.long()]
    if epi.get("bias"):
        kw["bias"] = torch.randn(N, generator=torch.Generator().manual_seed(seed + 2)).cuda()
        ref_kw["bias"] = kw["bias"].double()
    if epi.get("act"):
        kw["act"] = epi["act"]
    if epi.get("preact"):
        kw["preact"] = _mn(M, N, torch.uint8 if epi["preact"] == "byte" else bf16)
        kw["preact_is_grad"] = {"value": 0, "grad": 1, "byte": 2}[epi["preact"]]
    gin = epi.get("gelu_in")
    if gin:
        if gin == "byte":
            q = _mn(M, N, torch.uint8)
            q.copy_(torch.randint(0, 256, (M, N), generator=torch.Generator(device="cuda").manual_seed(seed + 3), device="cuda", dtype=torch.uint8))
            kw["gelu_in"] = q
            ref_kw["gelu_in"] = (q.float() * torch.tensor(1.0 / GB.GQ_SCALE, dtype=torch.float32) - GB.GQ_OFF).double()
        else:
            kw["gelu_in"] = _mn(M, N, bf16)
            kw["gelu_in"].copy_(_rb((M, N), seed + 3))
            ref_kw["gelu_in"] = kw["gelu_in"].double()
        kw["gelu_in_is_grad"] = {"grad": 1, "byte": 2, "value": 0}[gin]
        ref_kw["gelu_in_mode"] = gin
    if epi.get("drop"):
        kw["dropout_p"], kw["seed"] = 0.1, seed + 4
        ref_kw["keep"] = hidden_keep_multiplier(seed + 4, M, N, 0.1).double().cuda()
    if epi.get("rscale"):
        rpg = (M + 31) // 32
        rs = torch.tensor([1.25, 0.0, 0.75, 1.25] * 8, device="cuda")
        kw["row_scale"], kw["rows_per_group"] = rs, rpg
        ref_kw["row_scale"] = rs.double().repeat_interleave(rpg)[:M]
    res = epi.get("res")
    if res:
        r = _mn(M, N, bf16 if res is True else (torch.float16 if res == "fp16" else torch.float32))
        r.copy_(_rb((M, N), seed + 5) if res is True else torch.randn(M, N, device="cuda") * 3 + (0 if res == "fp16" else 2))
        kw["residual"] = r
        rr = r.double()
        if epi.get("a_rowmap"):
            kw["res_rowmap"] = kw["a_rowmap"]
            rr = rr[kw["a_rowmap"].long()]
        ref_kw["residual"] = rr
        if res == "ln":
            mu, rstd = r.mean(1).contiguous(), (r.var(1, unbiased=False) + 1e-12).rsqrt().contiguous()
            gm, bt = torch.randn(N, device="cuda"), torch.randn(N, device="cuda")
            kw["res_ln"] = (mu, rstd, gm, bt)
            ref_kw["res_ln"] = (mu.double(), rstd.double(), gm.double(), bt.double())
    if epi.get("colsum"):
        kw["colsum"] = torch.zeros(N, device="cuda")
    if epi.get("rowsum"):
        kw["rowsum_a"] = torch.zeros(M, device="cuda")
    if epi.get("k_keep_rpg"):
        rpg = epi["k_keep_rpg"]
        ng = -(-K // rpg)
        keep = torch.tensor([1.25 if i % 3 != 1 else 0.0 for i in range(ng)], device="cuda")
        kw["k_keep"], kw["k_rows_per_group"] = keep, rpg
        ref_kw["k_mask"] = (keep != 0).double().repeat_interleave(rpg)[:K]
    ldc = (N + 7) // 8 * 8 + epi.get("ldc_pad", 0)
    if out == "acc":
        C = torch.randn(M, ldc, device="cuda") if not epi.get("assign") else torch.full((M, ldc), float("nan"), device="cuda")
        if not epi.get("assign"):
            ref_kw["c0"] = C[:, :N].double()
        kw.update(out=C[:, :N], accumulate=True, assign=bool(epi.get("assign")))
    elif epi.get("headmajor"):
        kw["out"] = torch.zeros(M * N, dtype=bf16, device="cuda").view(M, N)
        kw["headmajor"] = epi["headmajor"]
    else:
        dt = {"bf16": bf16, "fp32": torch.float32, "fp16": torch.float16}[out]
        kw["out"] = torch.zeros(M, ldc, dtype=dt, device="cuda")[:, :N] if not epi.get("c_pad") else torch.zeros(M, ldc, dtype=dt, device="cuda")
        if epi.get("c_pad"):
            kw["c_pad_writable"] = True
    res_out = {}

    def call():
        res_out["y"] = hip.gemm(layout, A, B, M, N, K, splits=splits, **kw)

    old = _select(over)
    try:
        names = _names(call)
    finally:
        _restore(old)
    torch.cuda.synchronize()
    y = res_out["y"]
    if epi.get("headmajor"):
        h, d = epi["headmajor"]
        y = kw["out"].reshape(-1).view(N // (h * d), h, M, d).permute(2, 0, 1, 3).reshape(M, N)
    y = y[:, :N]
    lda = A.stride(0)
    ldb = B.stride(0)
    host = GB.route(layout, M, N, K, lda, ldb, dict(epi, out=out), splits, **{k: v for k, v in over.items()})
    tile = host[0][1]
    got = {"y": y}
    if epi.get("preact"):
        p = kw["preact"]
        got["pre"] = (p.double() / GB.GQ_SCALE - GB.GQ_OFF) if epi["preact"] == "byte" else p
    if epi.get("colsum"):
        got["cs"] = kw["colsum"]
    if epi.get("rowsum"):
        got["rs"] = kw["rowsum_a"]
    return names, host, want, a, b, ref_kw, got, tile


@pytest.mark.parametrize("cid", list(CASES))
def test_gemm_route_against_float64(cid):
    names, host, want, a, b, ref_kw, got, tile = _run_case(cid)
    kern = [k for k, _ in host]
    if want is not None:
        # generated cases name the GEMM kernel only (the reduction pass follows from splits); the hand-written ones name every launch
        n = 1 if cid.startswith("matrix_") or "_splits" in cid else len(kern)
        assert kern[:n] == want, f"{cid}: the host selector picks {kern}, the case was written for {want}"
    seen = _launched(names)
    assert seen == set(kern), f"{cid}: GEMM kernels launched {sorted(seen)}, expected {sorted(set(kern))}; device kernels: {sorted(set(names))}"
    if "gemm_ps_kernel" in kern:
        assert _ps_rows(names) == {tile[0]}, f"{cid}: phase-shifted tile rows {_ps_rows(names)}, expected {tile[0]}; {sorted(set(names))}"
    M = a.shape[0]
    if M > 200000:                                            # the operand above 2 GiB: sampled rows (the last tile, the rows around byte 2^31)
        lda = a.shape[1]
        r31 = (1 << 31) // (lda * 2)
        rows = torch.cat([torch.arange(0, 64), torch.arange(r31 - 96, r31 + 96), torch.arange(M - 256, M)]).cuda()
        kw = dict(ref_kw)
        kw["bias"] = kw.get("bias")
        r = GB.case(a[rows], b, **kw)
        g = {t: v[rows] if t != "cs" else v for t, v in got.items()}
        fails, stats = GB.check_all(g, r, tile, rows=rows)
    else:
        r = GB.case(a, b, **ref_kw)
        fails, stats = GB.check_all(got, r, tile)
    print(f"\n{cid}: {kern} tile {tile}: " + ", ".join(f"{t} err/bound {e:.3g} tile ratio {tr:.3g}" for t, (e, tr) in stats.items()))
    assert not fails, fails


GROUPS = {   # jobs (M, N, K, k_keep rows per group or 0, assign), splits, expected kernels
    "grouped_3_jobs": ([(768, 768, 2048, 0, False), (512, 1024, 2048, 0, True), (1024, 256, 2048, 256, False)], 3,
                       ["gemm_pp_group_kernel", "tn_reduce_group_kernel"]),
    "grouped_4_jobs_owner": ([(256, 256, 512, 0, True), (384, 512, 512, 0, False), (768, 256, 512, 0, False), (160, 512, 512, 0, True)], 1,
                             ["gemm_pp_group_kernel"]),
    "grouped_fallback": ([(768, 768, 1024, 0, False), (130, 256, 1024, 0, True)], 3, ["gemm_pp_kernel", "gemm_kernel"]),
}


@pytest.mark.parametrize("gid", list(GROUPS))
def test_gemm_tn_grouped_against_float64(gid):
    from lavender_amd import hip
    spec, splits, want = GROUPS[gid]
    jobs, refs = [], []
    for i, (M, N, K, rpg, assign) in enumerate(spec):
        A, B, a, b = _operands(2, M, N, K, {}, 100 * i + len(gid))
        C = torch.full((M, N), float("nan"), device="cuda") if assign else torch.randn(M, N, device="cuda")
        j = dict(A=A, B=B, out=C, M=M, N=N, alpha=0.75, rowsum_a=torch.zeros(M, device="cuda"), assign=assign, fallback_splits=2)
        rk = dict(alpha=0.75, out="acc", assign=assign, rowsum=True, splits=max(splits, 2))
        if not assign:
            rk["c0"] = C.double()
        if rpg:
            keep = torch.tensor([1.0 if g % 2 == 0 else 0.0 for g in range(-(-K // rpg))], device="cuda")
            j["k_keep"], j["k_rows_per_group"] = keep, rpg
            rk["k_mask"] = (keep != 0).double().repeat_interleave(rpg)[:K]
        jobs.append(j)
        refs.append((a, b, rk))
    host = GB.grouped_route([dict(M=M, N=N, K=K, k_keep_rpg=rpg, fallback_splits=2) for (M, N, K, rpg, _) in spec], splits)
    names = _names(lambda: hip.gemm_tn_grouped(jobs, splits))
    kern = [k for k, _ in host]
    for k in want:
        assert k in kern, f"{gid}: the host selector picks {kern}, the case was written for {want}"
    seen = _launched(names)
    assert seen == set(kern), f"{gid}: GEMM kernels launched {sorted(seen)}, expected {sorted(set(kern))}; device kernels: {sorted(set(names))}"
    for j, (a, b, rk) in zip(jobs, refs):
        r = GB.case(a, b, **rk)
        fails, stats = GB.check_all({"y": j["out"], "rs": j["rowsum_a"]}, r, (256, 256))
        print(f"\n{gid} job {tuple(a.shape)}x{b.shape[1]}: " + ", ".join(f"{t} err/bound {e:.3g} tile ratio {tr:.3g}" for t, (e, tr) in stats.items()))
        assert not fails, fails
