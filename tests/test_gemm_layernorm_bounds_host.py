"""CPU: the GEMM and LayerNorm bounds of tests/gemm_bounds.py and tests/layernorm_bounds.py can fail.  "Kernel outputs" are built on the host from
the rounding model of each route family (the product accumulated in fp32, the epilogue in float64, the kernel's stores injected): the assertion
must accept them, and with each injected kernel bug it must reject them.  Every case prints its largest err/bound and tile ratio."""
import pytest
import torch

from tests import gemm_bounds as GB
from tests import layernorm_bounds as LB
from tests.helpers import hidden_keep_multiplier

torch.set_num_threads(min(16, torch.get_num_threads()))


def _bf(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).bfloat16().double()


def _f(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float().double()


# ---- GEMM families: (M, N, K, tile, epilogue) -- shapes small enough for the CPU, with the tails the kernels' tiles leave -------------------
FAM = {
    "small_128": (193, 136, 192, (128, 128), dict(bias=True)),
    "big_256x128": (300, 264, 128, (256, 128), dict(bias=True, act=1, preact="grad")),
    "huge_256": (300, 256, 128, (256, 256), dict(bias=True, keep=True, rscale=True, res=True, colsum=True)),
    "h192": (200, 256, 64, (192, 256), dict(bias=True, act=1, preact="byte")),
    "o32_resln": (200, 256, 96, (256, 256), dict(bias=True, keep=True, rscale=True, res="ln", out="fp32")),
    "fp16_out": (136, 136, 64, (128, 128), dict(bias=True, res="fp16", out="fp16", big=True)),
    "gc": (257, 256, 64, (256, 256), dict(gelu_in="grad", rscale=True, colsum=True)),
    "gelu_in_value": (130, 128, 96, (128, 128), dict(gelu_in="value", act=2, preact="grad", colsum=True)),
    "tn_split": (260, 256, 1024, (256, 256), dict(out="acc", splits=3, alpha=1.25, rowsum=True, k_keep=True)),
    "tn_assign": (160, 512, 384, (256, 256), dict(out="acc", splits=11, assign=True)),
    "tn_owner": (130, 130, 192, (128, 128), dict(out="acc", splits=1)),
}


def _inputs(fam):
    M, N, K, tile, epi = FAM[fam]
    a, b = _bf((M, K), M + K, 0.25), _bf((K, N), N + K, 0.25)
    kw = dict(alpha=epi.get("alpha", 1.0), act=epi.get("act", 0), preact=epi.get("preact"), colsum=bool(epi.get("colsum")),
              out=epi.get("out", "bf16"), splits=epi.get("splits", 1), rowsum=bool(epi.get("rowsum")), assign=bool(epi.get("assign")))
    if epi.get("big"):
        a = a * 1e5                                          # outputs past the fp16 range: the store must saturate
    if epi.get("bias"):
        kw["bias"] = _f((N,), 5)
    if epi.get("gelu_in"):
        kw["gelu_in"] = _bf((M, N), 6)
        kw["gelu_in_mode"] = epi["gelu_in"]
    if epi.get("keep"):
        kw["keep"] = hidden_keep_multiplier(77, M, N, 0.1).double()
    if epi.get("rscale"):
        kw["row_scale"] = torch.tensor([0.0, 1.25, 1.25]).double().repeat_interleave((M + 2) // 3)[:M]
    if epi.get("res"):
        kw["residual"] = _bf((M, N), 8) if epi["res"] is True else _f((M, N), 8).half().double() if epi["res"] == "fp16" else _f((M, N), 8, 3.0) + 2.0
        if epi["res"] == "ln":
            r = kw["residual"]
            kw["res_ln"] = (r.mean(1), (r.var(1, unbiased=False) + 1e-12).rsqrt(), _f((N,), 9), _f((N,), 10))
    if epi.get("out") == "acc" and not epi.get("assign"):
        kw["c0"] = _f((M, N), 11)
    if epi.get("assign"):
        kw["c0"] = torch.full((M, N), 1e3, dtype=torch.float64)          # garbage in C: assign must not read it
    if epi.get("k_keep"):
        kw["k_mask"] = (torch.arange(K) // 128 % 3 != 0).double()          # the last k-tile belongs to a kept sample
    return M, N, K, tile, epi, a, b, kw


GEMM_MUT = {   # bug -> the family it is injected into
    "last_ktile_dropped": "tn_split",
    "mtail_last_row_unwritten": "small_128",
    "bias_shift_last_block": "big_256x128",
    "alpha_twice_splitk": "tn_split",
    "colsum_tile_missing": "huge_256",
    "dropout_index_ldc": "huge_256",
    "tanh_gelu_fp32": "gelu_fp32",
    "residual_rowmap_off_by_one": "huge_256",
    "fp16_no_saturation": "fp16_out",
    "assign_ignored": "tn_assign",
    "gelu_byte_truncated": "h192",
    "rowsum_without_alpha": "tn_split",
    "res_ln_stale_rstd": "o32_resln",
}
FAM["gelu_fp32"] = (200, 264, 64, (256, 128), dict(bias=True, act=1, out="fp32"))


def _gemm_emulate(fam, mut=None):
    M, N, K, tile, epi, a, b, kw = _inputs(fam)
    ref = GB.case(a, b, **kw)
    k2 = dict(kw)
    fns = {"z32": True}
    if mut == "last_ktile_dropped":                           # the final split's last k-tile never read
        m = (k2.get("k_mask") if k2.get("k_mask") is not None else torch.ones(K, dtype=torch.float64)).clone()
        m[K - 64:] = 0
        k2["k_mask"] = m
    elif mut == "bias_shift_last_block":
        bb = k2["bias"].clone()
        n0 = (N - 16) // tile[1] * tile[1]                   # the last column block with more than one 8-column chunk
        n1 = min(n0 + tile[1], N)
        bb[n0:n1 - 8] = kw["bias"][n0 + 8:n1]
        k2["bias"] = bb
    elif mut == "alpha_twice_splitk":
        k2["alpha"] = kw["alpha"] ** 2
    elif mut == "dropout_index_ldc":
        ldc = (N + 7) // 8 * 8 + 8
        k2["keep"] = hidden_keep_multiplier(77, M, ldc, 0.1).double()[:, :N]
    elif mut == "tanh_gelu_fp32":
        fns["gelu"] = GB.tanh_gelu
    elif mut == "residual_rowmap_off_by_one":
        k2["residual"] = torch.cat([kw["residual"][1:], kw["residual"][:1]])
    elif mut == "gelu_byte_truncated":
        fns["gq"] = lambda g: torch.floor(g.float() * float(GB.GQ_SCALE) + float(GB.GQ_OFF * GB.GQ_SCALE)).clamp(0, 255).double() / GB.GQ_SCALE - GB.GQ_OFF
    elif mut == "assign_ignored":
        k2["assign"] = False
    elif mut == "res_ln_stale_rstd":
        mu, rs, g_, b_ = kw["res_ln"]
        k2["res_ln"] = (mu, rs * (1 + 2 ** -10), g_, b_)
    r = GB.case(a, b, fns=fns, **k2)
    got = {t: r["m_" + t].clone() for t in ("y", "pre", "cs", "rs") if "m_" + t in r}
    if mut == "mtail_last_row_unwritten":
        got["y"][M - 1] = 0.0
    elif mut == "colsum_tile_missing":
        v = GB.case(a, b, fns=fns, **dict(k2, colsum=False, out="fp32"))["y"]
        got["cs"] = got["cs"] - v[:tile[0]].sum(0) * (torch.arange(N) < tile[1]).double()
    elif mut == "fp16_no_saturation":
        v = GB.case(a, b, fns=fns, **dict(k2, out="fp32"))["y"]
        got["y"] = v.float().half().double()
    elif mut == "rowsum_without_alpha":
        got["rs"] = got["rs"] / kw["alpha"]
    return GB.check_all(got, ref, tile)


@pytest.mark.parametrize("fam", list(FAM))
def test_gemm_rounding_model_is_accepted(fam):
    fails, stats = _gemm_emulate(fam)
    print(fam, {k: (f"{e:.3g}", f"{t:.3g}") for k, (e, t) in stats.items()})
    assert not fails, fails
    assert all(e <= 1.0 and t <= 1.0 for e, t in stats.values()), stats


@pytest.mark.parametrize("mut", list(GEMM_MUT))
def test_gemm_mutation_is_rejected(mut):
    fails, stats = _gemm_emulate(GEMM_MUT[mut], mut)
    print(mut, {k: (f"{e:.3g}", f"{t:.3g}") for k, (e, t) in stats.items()})
    assert fails, f"{GEMM_MUT[mut]}: the bound accepts the mutation {mut}"


def test_route_table_host_selector():
    """the host copy of the selector on shapes whose choice is worked out by hand from gemm_plan_part (gemm.hip)"""
    assert GB.route(0, 193, 136, 192, 192, 192) == [("gemm_kernel", (128, 128))]
    assert GB.route(0, 8448, 2048, 128, 128, 128, dict(bias=True, act=1, preact="grad")) == [("gemm_ps_kernel", (192, 256))]
    assert GB.route(0, 8448, 2048, 128, 128, 128, dict(bias=True, act=1, preact="grad"), ps=0) == [("gemm_h192l_kernel", (192, 256))]
    assert GB.route(0, 45120, 768, 128, 128, 128, dict(bias=True)) == [("gemm_ps_kernel", (192, 256))]
    assert GB.route(0, 45120, 768, 128, 128, 128, dict(bias=True), ps=0) == [("gemm_h192l_kernel", (192, 256))]
    assert GB.route(1, 45120, 768, 128, 128, 768, dict(bias=True)) == [("gemm_h192_kernel", (192, 256))]
    assert GB.route(2, 1024, 512, 7840, 1024, 512, dict(out="acc", k_keep_rpg=245), 3) == [("gemm_pp_kernel", (256, 256)), ("tn_reduce_kernel", (256, 128))]
    r = GB.route(2, 768, 768, 30280, 768, 768, dict(out="acc"), 4)
    assert [k for k, _ in r] == ["gemm_pp_kernel", "tn_reduce_kernel", "gemm_kernel"]



# ---- the library's own route plan (lav_gemm_plan, no device) against the host copy ------------------------------------------------------------
SEL = {"ps": 11, "h192": 7, "h192l": 9, "pp_tn": 2, "tn_min_m": 12, "group_n": 6, "dbg": 5, "tn_group": 13}
_PTR = 4096          # a non-null, 16-byte aligned stand-in: the plan only tests the epilogue's pointers for presence


def _c_epilogue(epi):
    """the lav_gemm_epilogue of a gemm_bounds epilogue dict (as tests/test_gpu_gemm_bounds.py and hip.gemm fill it)"""
    from lavender_amd import _lib
    e = _lib.GemmEpilogue()
    e.alpha, e.rows_per_group, e.k_rows_per_group = epi.get("alpha", 1.0), 1, 1
    e.bias = _PTR if epi.get("bias") else None
    e.act = epi.get("act", 0)
    if epi.get("preact"):
        e.preact, e.preact_is_grad = _PTR, {"value": 0, "grad": 1, "byte": 2}[epi["preact"]]
    if epi.get("gelu_in"):
        e.gelu_in, e.gelu_in_is_grad = _PTR, {"value": 0, "grad": 1, "byte": 2}[epi["gelu_in"]]
    e.dropout_p = 0.1 if epi.get("drop") else 0.0
    e.row_scale = _PTR if epi.get("rscale") else None
    e.residual = _PTR if epi.get("res") else None
    e.colsum = _PTR if epi.get("colsum") else None
    e.out_mode = {"bf16": 0, "fp32": 1, "acc": 2, "fp16": 3}[epi.get("out", "bf16")]
    if epi.get("k_keep_rpg"):
        e.k_keep, e.k_rows_per_group = _PTR, epi["k_keep_rpg"]
    e.rowsum_a = _PTR if epi.get("rowsum") else None
    e.a_rowmap = _PTR if epi.get("a_rowmap") else None
    e.c_pad_writable, e.assign = int(bool(epi.get("c_pad"))), int(bool(epi.get("assign")))
    return e


def _launches(n, out, what):
    from lavender_amd import _lib
    assert n > 0, f"{what}: the library refuses the call (rc={n}): {_lib.lib.lav_last_error()}"
    return [(out[i].kernel.decode(), (out[i].tile_rows, out[i].tile_cols)) for i in range(n)]


def _plan(layout, M, N, K, lda, ldb, ldc, epi, splits):
    import ctypes as C
    from lavender_amd import _lib
    out = (_lib.GemmLaunchInfo * 4)()
    n = _lib.lib.lav_gemm_plan(layout, M, N, K, lda, ldb, ldc, C.byref(_c_epilogue(epi)), splits, out, 4)
    return _launches(n, out, (layout, M, N, K, lda, ldb, ldc, epi, splits))


def _job_array(jobs):
    from lavender_amd import _lib
    arr = (_lib.GemmTnJob * len(jobs))()
    for q, j in zip(arr, jobs):
        q.M, q.N, q.K, q.lda, q.ldb, q.ldc = j["M"], j["N"], j["K"], (j["M"] + 7) // 8 * 8, (j["N"] + 7) // 8 * 8, (j["N"] + 3) // 4 * 4
        if j.get("k_keep_rpg"):
            q.k_keep, q.k_rows_per_group = _PTR, j["k_keep_rpg"]
        q.alpha, q.fallback_splits = 1.0, j.get("fallback_splits", 1)
    return arr


def _grouped_plan(jobs, splits):
    from lavender_amd import _lib
    arr = _job_array(jobs)
    out = (_lib.GemmLaunchInfo * 16)()
    return _launches(_lib.lib.lav_gemm_tn_grouped_plan(len(jobs), arr, splits, out, 16), out, (jobs, splits))


class _switches:
    """lav_gemm_select overrides for a block (through hip.gemm_select: the split factors hip.py caches follow the switches), restored afterwards"""

    def __init__(self, **over):
        self.over = over

    def __enter__(self):
        from lavender_amd import hip
        self.old = {k: hip.gemm_select(SEL[k], int(v)) for k, v in self.over.items()}

    def __exit__(self, *exc):
        from lavender_amd import hip
        for k, v in self.old.items():
            hip.gemm_select(SEL[k], v)


def _route_kw(over):
    return {k: v for k, v in over.items() if k not in ("group_n", "dbg")}          # the tile walk and the probe bits change no kernel choice


def _ld(layout, M, N, K):
    """contiguous leading dimensions (rows padded to 8 elements), as test_gpu_gemm_bounds._operands builds them"""
    pad = lambda n: (n + 7) // 8 * 8
    return (pad(K), pad(K)) if layout == 0 else (pad(K), pad(N)) if layout == 1 else (pad(M), pad(N))


def test_plan_matches_route_on_the_gpu_cases():
    """every case of tests/test_gpu_gemm_bounds.py at the lav_gemm_select settings it runs it with: the library's plan and gemm_bounds.route name
    the same kernels with the same tiles in the same order"""
    from tests.test_gpu_gemm_bounds import CASES, GROUPS
    for cid, (layout, M, N, K, epi, splits, over, want) in CASES.items():
        out = epi.get("out", "bf16")
        lda, ldb = _ld(layout, M, N, K)
        lda += epi.get("lda_pad", 0) if layout != 2 else 0
        ldc = (N + 7) // 8 * 8 + epi.get("ldc_pad", 0)
        with _switches(**over):
            got = _plan(layout, M, N, K, lda, ldb, ldc, dict(epi, out=out), splits)
        host = GB.route(layout, M, N, K, lda, ldb, dict(epi, out=out), splits, **over)
        assert got == host, f"{cid}: lav_gemm_plan {got}, gemm_bounds.route {host}"
        if want is not None:
            assert [k for k, _ in got][:len(want)] == want or cid.startswith("matrix_") or "_splits" in cid, (cid, got, want)
    for gid, (spec, splits, want) in GROUPS.items():
        jobs = [dict(M=M, N=N, K=K, k_keep_rpg=rpg, fallback_splits=2) for (M, N, K, rpg, _) in spec]
        got, host = _grouped_plan(jobs, splits), GB.grouped_route(jobs, splits)
        assert got == host, f"{gid}: lav_gemm_tn_grouped_plan {got}, gemm_bounds.grouped_route {host}"


# GEMM calls of the bench models (bench.py: cfg2 = Swin-B 224^2, 32 text tokens, batch 32; cfg4 = Swin-L 384^2, batch 8; cfg5 = retrieval, Swin-B,
# 26 text tokens, 8 x 8 pairs; 5 frames each), from the model dimensions: every nn.Linear (rows, out, in) of the Swin stages (video_swin.SWIN_SIZES:
# each frame is a clip of its own, rows = B * 5 * (S / 4)^2 / 4^stage, C = E * 2^stage), the patch merging, the 12 + 12 BERT layers (hidden 768,
# FFN 3072, rows = sequences * (5 * ((S / 32)^2 + 1) + X)) and the MLM head (30522-wide vocabulary), as forward (layout 0), input-gradient
# (layout 1) and weight-gradient (layout 2) calls with the epilogues and split factors the step uses.
def _model_linears(size, S, X, B, pairs=None):
    from lavender_amd.video_swin import SWIN_SIZES as SIZES
    E, n = SIZES[size]["embed_dim"], B * 5
    lin, groups = [], []
    rows = n * (S // 4) ** 2
    lin.append((rows, E, 96, 0))
    for st in range(4):
        C, R = E << st, rows >> (2 * st)
        blk = [(R, 3 * C, C), (R, C, C), (R, 4 * C, C), (R, C, 4 * C)]
        lin += [(r, o, i, R // n) for r, o, i in blk]
        groups.append(([(o, i) for _, o, i in blk], R, R // n))
        if st < 3:
            lin.append((R // 4, 2 * C, 4 * C, 0))
    tok = (S // 32) ** 2
    lin.append((n * tok, 768, 8 * E, 0))
    seqs = pairs or n
    R = seqs * (5 * (tok + 1) + X)
    blk = [(R, 2304, 768), (R, 768, 768), (R, 3072, 768), (R, 768, 3072)]
    lin += [(r, o, i, 0) for r, o, i in blk] + [(R, 768, 768, 0), (n * X, 768, 768, 0), (seqs * X, 768, 768, 0), (seqs * X, 30522, 768, 0)]
    groups.append(([(o, i) for _, o, i in blk], R, 0))
    return lin, groups


FWD_EPI = [dict(), dict(bias=True), dict(bias=True, act=1, preact="grad"), dict(bias=True, act=1, preact="byte"), dict(bias=True, drop=True, rscale=True, res=True),
           dict(bias=True, drop=True, res="fp16", out="fp16"), dict(bias=True, drop=True, res="ln", out="fp32"), dict(bias=True, c_pad=True),
           dict(bias=True, res=True, a_rowmap=True)]
BWD_EPI = [dict(), dict(gelu_in="grad", colsum=True), dict(gelu_in="byte", rscale=True, colsum=True), dict(colsum=True), dict(rscale=True, colsum=True)]


def test_plan_matches_route_on_the_bench_models():
    from lavender_amd import hip
    n = 0
    for size, S, X, B, pairs in (("base", 224, 32, 32, None), ("large", 384, 32, 8, None), ("base", 224, 26, 8, 64)):
        lin, groups = _model_linears(size, S, X, B, pairs)
        for R, o, i, rpg in lin:
            calls = [(0, R, o, i, e, 1) for e in FWD_EPI if not e.get("a_rowmap") or (o % 256 == 0 and i % 64 == 0)]
            calls += [(1, R, i, o, e, 1) for e in BWD_EPI] + [(1, R, i, o, {}, hip.splits_nn(R, i, o) if i % 8 == 0 else 1)]
            for keep in ((0, rpg) if rpg else (0,)):
                e = dict(out="acc", rowsum=True, **({"k_keep_rpg": keep} if keep else {}))
                sp = hip.splits_for(o, i, R, bool(keep))
                calls += [(2, o, i, R, e, sp), (2, o, i, R, dict(e, assign=o % 4 == 0 and i % 4 == 0), sp), (2, o, i, R, e, 1)]
            for layout, M, N, K, e, sp in calls:
                lda, ldb = _ld(layout, M, N, K)
                ldc = (N + 7) // 8 * 8
                got, host = _plan(layout, M, N, K, lda, ldb, ldc, e, sp), GB.route(layout, M, N, K, lda, ldb, e, sp)
                assert got == host, f"{size} {S}: {(layout, M, N, K, e, sp)}: lav_gemm_plan {got}, gemm_bounds.route {host}"
                n += 1
        for shapes, K, rpg in groups:
            for keep in ((0, rpg) if rpg else (0,)):
                jobs = [dict(M=M, N=N, K=K, k_keep_rpg=keep, fallback_splits=hip.splits_for(M, N, K, bool(keep))) for M, N in shapes]
                sp = hip.group_splits_for(shapes, K)
                got, host = _grouped_plan(jobs, max(sp, 1)), GB.grouped_route(jobs, max(sp, 1))
                assert got == host, f"{size} {S}: grouped {jobs}: lav_gemm_tn_grouped_plan {got}, gemm_bounds.grouped_route {host}"
                if not keep:
                    assert (sp > 0) == (got[0][0] == "gemm_pp_group_kernel"), (shapes, K, sp, got)
                n += 1
    print(f"{n} model calls")
    assert n > 1000


# ---- seeded random sweep of valid calls ---------------------------------------------------------------------------------------------------------
SWEEP_EPI = FWD_EPI + BWD_EPI + [
    dict(bias=True, drop=True, rscale=True, res="ln", out="fp32"), dict(bias=True, drop=True, rscale=True, res="fp16", out="fp16"),
    dict(act=2, preact="grad", gelu_in="value", drop=True, colsum=True), dict(bias=True, act=1, preact="value"), dict(act=2), dict(out="fp32"),
    dict(bias=True, out="fp16"), dict(out="acc"), dict(out="acc", bias=True), dict(gelu_in="value"), dict(bias=True, act=1, gelu_in="grad")]
SWEEP_SWITCHES = [dict(ps=ps, h192=h, h192l=hl, pp_tn=pp, tn_min_m=mm, group_n=gn, dbg=dbg)
                  for ps, h, hl, pp, mm, gn, dbg in [(3, 1, 1, 1, 160, -1, 0), (0, 1, 1, 1, 160, 0, 0), (1, 1, 0, 1, 256, 4, 1), (2, 1, 1, 0, 160, -1, 2),
                                                     (0, 1, 0, 0, 300, 2, 4), (3, 0, 1, 1, 128, -1, 0), (0, 0, 0, 1, 160, -1, 0), (1, 1, 1, 0, 256, 0, 0)]]


def _pick(rng, xs):
    return xs[int(rng.integers(len(xs)))]


def _random_call(rng):
    """one valid lav_gemm_bf16 call around the thresholds of the route: (layout, M, N, K, lda, ldb, ldc, epilogue dict, splits)"""
    layout = int(rng.integers(3))
    M = max(1, _pick(rng, [160, 256, 2048, 192, 128, 512, 4096, 4289, 8448, 20481, 45120, int(rng.integers(1, 60000))]) + _pick(rng, [-1, 0, 0, 1, 31, -97]))
    N = max(1, _pick(rng, [256, 512, 768, 1024, 2048, 3072, 256 * int(rng.integers(1, 40)), 128 * int(rng.integers(1, 40))])
            + _pick(rng, [0, 0, 0, 0, 4, 8, 12, 128, 132, 136, -8, -4, 1, 2, 3, 5, 6, 7, -128, -250]))
    if rng.random() < 0.15:                                  # outputs that under-fill the last round of 256-row tiles: the 192-row tiles
        M, N = _pick(rng, [(4289, 2048), (8448, 2048), (45120, 768), (45120, 2304), (20481, 768)])
    K = max(1, _pick(rng, [64, 128, 768, 1024, 2048, 1984, 2112, 3072, 7840, 30280, 64 * int(rng.integers(1, 600))]) + _pick(rng, [0, 0, 0, 32, -32, 4, 36, -20, 1, 63]))
    if layout == 2:
        epi = dict(_pick(rng, [dict(out="acc")] * 8 + [dict(out="fp32"), dict(out="acc", bias=True), dict(), dict(out="acc", colsum=True)]))
        if rng.random() < 0.5:
            epi["rowsum"] = True
        if rng.random() < 0.4:
            g128 = -(-K // 128)                              # rows per group that give exactly 128 groups: the cap of the ping-pong kernel
            epi["k_keep_rpg"] = max(1, _pick(rng, [16, 31, 32, 33, 63, 64, 65, 245, 256, g128, g128 - 1, g128 + 1, -(-K // 129), K]))
    else:
        epi = dict(_pick(rng, SWEEP_EPI))
        if epi.get("a_rowmap") and not (layout == 0 and N % 256 == 0 and K % 64 == 0):
            del epi["a_rowmap"]
        if rng.random() < 0.15:
            epi["c_pad"] = True
    out = epi.get("out", "bf16")
    splits = int(rng.integers(1, 17)) if rng.random() < 0.6 else 1
    if not (out == "acc" or (out == "bf16" and layout != 2 and not (set(epi) - {"c_pad"}) and N % 8 == 0)):
        splits = 1                                           # split-K: fp32 accumulate, or a bf16 output without epilogue and N % 8 == 0
    if epi.get("a_rowmap"):
        splits = 1
    if layout == 2 and out == "acc" and rng.random() < 0.4 and (N % 4 == 0 or splits == 1):
        epi["assign"] = True                                 # with split-K the reduction pass assigns: N % 4 == 0
    lda, ldb = _ld(layout, M, N, K)
    if rng.random() < 0.3:                                   # operands on both sides of 2 GiB (the phase-shifted kernels address 32 bits)
        rows_a, rows_b = (M, N) if layout == 0 else (M, K) if layout == 1 else (K, K)
        lda = max(lda, ((1 << 30) // rows_a + _pick(rng, [-16, 8, 64])) // 8 * 8)
        if rng.random() < 0.5:
            ldb = max(ldb, ((1 << 30) // rows_b + _pick(rng, [-16, 8, 64])) // 8 * 8)
    ldc = (N + 7) // 8 * 8 + _pick(rng, [0, 0, 8, 16]) if out in ("bf16", "fp16") else (N + 3) // 4 * 4 + _pick(rng, [0, 0, 4, 8])
    return layout, M, N, K, lda, ldb, ldc, epi, splits


def test_plan_matches_route_on_a_random_sweep():
    """24 000 valid calls (seeded) over the three layouts, every feature set, output mode, split factor, drop-path grouping, the M / N / K
    thresholds and residues of the route and each lav_gemm_select setting: kernel names, tiles and launch order agree on every one, and the
    sweep reaches every kernel and every multi-launch form"""
    import numpy as np
    rng = np.random.default_rng(20260)
    seen, fsets, n = set(), set(), 0
    for over in SWEEP_SWITCHES:
        calls = [_random_call(rng) for _ in range(3000)]
        with _switches(**over):
            got = [_plan(*c) for c in calls]
        for c, g in zip(calls, got):
            layout, M, N, K, lda, ldb, ldc, epi, splits = c
            host = GB.route(layout, M, N, K, lda, ldb, epi, splits, **_route_kw(over))
            assert g == host, f"{c} at {over}: lav_gemm_plan {g}, gemm_bounds.route {host}"
            seen.add(tuple(k for k, _ in g))
            seen.update(g)
            fsets.add((g[0][0], GB.FSEL_NAME[GB.feature_select(N, epi)]) if layout != 2 else None)
            n += 1
    assert n >= 20000
    for k in (("gemm_kernel", (128, 128)), ("gemm_big_kernel", (256, 128)), ("gemm_huge_kernel", (256, 256)), ("gemm_h192_kernel", (192, 256)),
              ("gemm_h192l_kernel", (192, 256)), ("gemm_ps_kernel", (256, 256)), ("gemm_ps_kernel", (192, 256)), ("gemm_pp_kernel", (256, 256)),
              ("tn_reduce_kernel", (256, 128)), ("tn_reduce_kernel", (128, 128)), ("splitk_reduce_bf16_kernel", (256, 256)),
              ("splitk_reduce_bf16_kernel", (128, 128)), ("gemm_pp_kernel", "tn_reduce_kernel", "gemm_kernel"), ("gemm_huge_kernel", "tn_reduce_kernel", "gemm_kernel"),
              ("gemm_big_kernel", "gemm_kernel")):
        assert k in seen, f"the sweep never reaches {k}"
    for kern, sets in (("gemm_big_kernel", 6), ("gemm_huge_kernel", 6), ("gemm_ps_kernel", 5), ("gemm_h192_kernel", 5), ("gemm_h192l_kernel", 5)):
        assert len({f for f in fsets if f and f[0] == kern}) == sets, (kern, sorted(f for f in fsets if f and f[0] == kern))


def test_grouped_plan_matches_route_and_hip_split_heuristic():
    """random groups of 1 ... 4 weight-gradient jobs with a common contraction: lav_gemm_tn_grouped_plan against gemm_bounds.grouped_route at each
    pp_tn / tn_min_m setting, and hip.group_splits_for(shapes, K) > 0 exactly when the library takes the grouped launch (jobs without k_keep,
    which group_splits_for is not told of)"""
    import numpy as np
    from lavender_amd import hip
    rng = np.random.default_rng(7)
    grouped = 0
    for over in (dict(), dict(pp_tn=0), dict(tn_min_m=256), dict(tn_min_m=300, pp_tn=1)):
        for _ in range(1000):
            K = max(32, _pick(rng, [512, 2048, 7840, 30280, 45120, 32 * int(rng.integers(1, 300))]) + _pick(rng, [0, 0, 0, 0, 32, 16, -1]))
            rpg = _pick(rng, [0, 0, 0, 245, 256, 64, 63, 32, -(-K // 128), -(-K // 129)])
            jobs = [dict(M=max(1, _pick(rng, [160, 256, 192, 384, 768, 1024, 3072]) + _pick(rng, [0, 0, 0, -1, 1])),
                         N=_pick(rng, [256, 512, 768, 1024, 3072, 384, 260]), K=K, k_keep_rpg=rpg, fallback_splits=int(rng.integers(1, 12)))
                    for _ in range(int(rng.integers(1, 5)))]
            splits = int(rng.integers(1, 9))
            with _switches(**over):
                got = _grouped_plan(jobs, splits)
            host = GB.grouped_route(jobs, splits, **over)
            assert got == host, f"{jobs} splits {splits} at {over}: lav_gemm_tn_grouped_plan {got}, gemm_bounds.grouped_route {host}"
            is_group = got[0][0] == "gemm_pp_group_kernel"
            assert not is_group or len(got) <= 2
            grouped += is_group
            if not over and not rpg:
                assert (hip.group_splits_for([(j["M"], j["N"]) for j in jobs], K) > 0) == is_group, (jobs, got)
    assert grouped > 200


# ---- the split-K policy (lav_gemm_splits / lav_gemm_tn_splits, no device) against the copy of what hip.py computed before (gemm_bounds) ---------
def _plan_ws(layout, M, N, K, lda, ldb, ldc, epi, splits):
    """split-K workspace bytes of a call, read off the launches of the library's route plan: a reduction pass sums one fp32 partial tile per
    workgroup of the GEMM launch in front of it"""
    import ctypes as C
    from lavender_amd import _lib
    out = (_lib.GemmLaunchInfo * 4)()
    n = _lib.lib.lav_gemm_plan(layout, M, N, K, lda, ldb, ldc, C.byref(_c_epilogue(epi)), splits, out, 4)
    assert n > 0, (layout, M, N, K, epi, splits, _lib.lib.lav_last_error())
    return max([out[i - 1].grid * out[i - 1].tile_rows * out[i - 1].tile_cols * 4 for i in range(1, n) if b"reduce" in out[i].kernel], default=0)


def _group_ws(jobs, gs):
    """the same of a grouped launch (gemm.hip tn_group_plan): 256-row partial tiles of every job that is split"""
    ws = 0
    for q in jobs:
        s = max(1, min(gs, q["K"] // 256))
        kps = ((q["K"] + s - 1) // s + 63) // 64 * 64
        sp = -(-q["K"] // kps)
        ws += sp * -(-q["M"] // 256) * (q["N"] // 128) * 256 * 128 * 4 if sp > 1 else 0
    return ws


def _check_split_policy(shapes, K, rpg, **par):
    """one group of weight gradients `shapes` over K rows (rpg: drop-path rows per group, 0 = none) and each of them alone: factors against the
    copy evaluated at `par`, workspace bytes against the plan and the old bound.  Returns (group factor, tiles of the group)."""
    import ctypes as C
    from lavender_amd import _lib, hip
    mm = {k: par[k] for k in ("tn_min_m",) if k in par}
    want = [GB.splits_for(M, N, K, bool(rpg), **mm) for M, N in shapes]
    epi = dict(out="acc", rowsum=True, **({"k_keep_rpg": rpg} if rpg else {}))
    for (M, N), w in zip(shapes, want):
        assert hip.splits_for(M, N, K, bool(rpg)) == w, (M, N, K, rpg, par, hip.splits_for(M, N, K, bool(rpg)), w)
        (lda, ldb), ldc, ws = _ld(2, M, N, K), (N + 3) // 4 * 4, C.c_size_t(1 << 60)
        got = _lib.lib.lav_gemm_splits(2, M, N, K, lda, ldb, ldc, C.byref(_c_epilogue(epi)), 0, C.byref(ws))
        assert got == w, (M, N, K, rpg, par, got, w, _lib.lib.lav_last_error())
        assert ws.value == _plan_ws(2, M, N, K, lda, ldb, ldc, epi, w) <= GB.tn_need(M, N, w), (M, N, K, rpg, par, ws.value, GB.tn_need(M, N, w))
        assert hip.splits_nn(K, N, M) == GB.splits_nn(K, N, M), (K, N, M)           # the same numbers as a long-K forward call, contraction M
    want_gs = GB.group_splits_for(shapes, K, **par)
    assert hip.group_splits_for(shapes, K) == want_gs, (shapes, K, par, hip.group_splits_for(shapes, K), want_gs)
    jobs = [dict(M=M, N=N, K=K, k_keep_rpg=rpg, fallback_splits=0) for M, N in shapes]
    arr, ws = _job_array(jobs), C.c_size_t(1 << 60)
    gs = _lib.lib.lav_gemm_tn_splits(len(jobs), arr, 0, C.byref(ws))
    assert gs >= 0 and [q.fallback_splits for q in arr] == want, (jobs, par, gs, [q.fallback_splits for q in arr], want)
    for j, w in zip(jobs, want):
        j["fallback_splits"] = w
    is_group = _grouped_plan(jobs, max(gs, 1))[0][0] == "gemm_pp_group_kernel"
    assert (gs > 0) == is_group and (gs == want_gs or (rpg and gs == 0)), (jobs, par, gs, want_gs)      # keep rows the kernel cannot take: one by one
    ws_plan = max([_group_ws(jobs, gs) if gs else 0] + [_plan_ws(2, M, N, K, *_ld(2, M, N, K), (N + 3) // 4 * 4, epi, w) for (M, N), w in zip(shapes, want)])
    assert ws.value == ws_plan <= sum(GB.tn_need(M, N, max(w, gs)) for (M, N), w in zip(shapes, want)), (jobs, par, gs, ws.value, ws_plan)
    return gs, sum(-(-M // 256) * (N // 256) for M, N in shapes)


def test_split_policy_matches_the_copy_on_the_bench_models():
    """every nn.Linear and every stage group of cfg2 / cfg4 / cfg5, with and without drop-path rows, at the default switches"""
    n = grouped = 0
    for size, S, X, B, pairs in (("base", 224, 32, 32, None), ("large", 384, 32, 8, None), ("base", 224, 26, 8, 64)):
        lin, groups = _model_linears(size, S, X, B, pairs)
        for R, o, i, rpg in lin:
            for keep in ((0, rpg) if rpg else (0,)):
                _check_split_policy([(o, i)], R, keep)
                n += 1
        for shapes, K, rpg in groups:
            for keep in ((0, rpg) if rpg else (0,)):
                grouped += _check_split_policy(shapes, K, keep)[0] > 0
                n += 1
    print(f"{n} linears and groups, {grouped} grouped")
    assert n > 150 and grouped > 0                           # (the cfg2 fusion layers, 45120 token rows, are grouped launches)


def _random_group(rng):
    """1 ... 4 weight-gradient outputs with a common contraction around every threshold of the policy: (shapes, K, rows per drop-path group)"""
    if rng.random() < 0.45:                                  # a group the 256 x 256 kernel takes, on both sides of 96 tiles
        K = 32 * int(rng.integers(1, 1500)) if rng.random() < 0.7 else _pick(rng, [7840, 30280 - 8, 45120, 224, 256, 288, 2048, 2080])
        shapes = [(_pick(rng, [160, 161, 192, 256, 257, 384, 768, 1024, 1536, 3072, 4096]), 256 * int(rng.integers(2, 17))) for _ in range(int(rng.integers(1, 5)))]
    else:
        K = max(1, _pick(rng, [32 * int(rng.integers(1, 1500)), 64 * int(rng.integers(1, 750)), 2048 + int(rng.integers(-70, 71)), int(rng.integers(1, 256)),
                               30280, 33840, 7840, int(rng.integers(1, 50000))]))
        shapes = [(_pick(rng, [127, 128, 129, 159, 160, 161, 255, 256, 257, 300, 301, 512, 1000, 3072, 30522, int(rng.integers(1, 9000))]),
                   max(4, _pick(rng, [128, 256]) * int(rng.integers(1, 25)) + _pick(rng, [0, 0, 0, 4, -4, 8, -8])))
                  for _ in range(int(rng.integers(1, 5)))]
    rpg = _pick(rng, [0, 0, 64, 245, 256, 32, 63, -(-K // 128), -(-K // 129), K])
    return shapes, K, rpg


@pytest.mark.parametrize("par", [dict(), dict(tn_min_m=256), dict(tn_min_m=300), dict(tn_group=0)], ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()) or "default")
def test_split_policy_matches_the_copy_on_a_random_sweep(par):
    """seeded groups of 1 ... 4 outputs (20 000 shapes and more at the default switches): M 127 ... 129, 159 ... 161, 255 ... 257 and larger, N multiples
    of 128 and 256 +- 4 and 8, K multiples of 32 and 64, ragged on both sides of 2048 and below 256, drop-path rows on and off, groups on both sides of
    96 tiles.  The library's factors equal the copy evaluated at the selected tn_min_m / tn_group; its workspace bytes are the plan's and within the
    old bound."""
    import numpy as np
    rng = np.random.default_rng(1606 + len(par) + par.get("tn_min_m", 0))
    shapes_n = groups = 0
    side = [0, 0]
    with _switches(**par):
        while shapes_n < (20000 if not par else 4000):
            shapes, K, rpg = _random_group(rng)
            gs, tiles = _check_split_policy(shapes, K, rpg, **par)
            shapes_n += len(shapes)
            groups += gs > 0
            side[tiles >= 96] += gs > 0
    print(f"{shapes_n} shapes, {groups} grouped launches ({side[0]} below 96 tiles, {side[1]} from 96 up)")
    assert par.get("tn_group", 1) == 0 or min(side) > (100 if not par else 20)
    assert par.get("tn_group", 1) != 0 or groups == 0


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------------
LN_FAM = {   # rows, C, input kind, eps
    "c128_bf16": (80, 128, "bf16", 1e-5),
    "c384_g16x3": (64, 384, "bf16", 1e-12),
    "c520_ragged": (40, 520, "fp32", 1e-5),
    "c768_offset_fp32": (48, 768, "fp32_offset", 1e-12),
    "c264_small_var": (48, 264, "small", 1e-5),
}
LN_MUT = {"one_pass_variance": "c768_offset_fp32", "missing_eps": "c264_small_var", "ragged_chunk_dropped": "c520_ragged",
          "dgamma_last_block_missing": "c128_bf16", "dx2_dropout_seed": "c384_g16x3"}


def _ln_inputs(fam):
    R, C, kind, eps = LN_FAM[fam]
    if kind == "bf16":
        x = _bf((R, C), C)
    elif kind == "small":
        x = _f((R, C), C, 0.01) + 0.5
    elif kind == "fp32_offset":
        x = _f((R, C), C) + 1e3
    else:
        x = _f((R, C), C)
    g, b = _f((C,), 1) * 0.5 + 1.0, _f((C,), 2) * 0.1
    dy, add = _bf((R, C), 3), _bf((R, C), 4)
    rs = torch.tensor([1.25, 0.0]).double().repeat_interleave((R + 1) // 2)[:R]
    keep = hidden_keep_multiplier(99, R, C, 0.1).double()
    return R, C, eps, x, g, b, dy, add, rs, keep


def _ln_emulate(fam, mut=None):
    R, C, eps, x, g, b, dy, add, rs, keep = _ln_inputs(fam)
    G, _, rpb = LB.geometry(C)
    f = LB.fwd(x, g, b, eps, y32=True)
    ref = dict(f)
    ref.update(LB.bwd(f, x, dy, g, add_in=add, row_scale=rs, keep=keep))
    fm = LB.fwd(x, g, b, eps, y32=True, one_pass=mut == "one_pass_variance", no_eps=mut == "missing_eps",
                drop_chunk=0.0 if mut == "ragged_chunk_dropped" else None)
    km = hidden_keep_multiplier(100, R, C, 0.1).double() if mut == "dx2_dropout_seed" else keep
    # the backward runs on the kernel's own (fp32) statistics, as in training
    fk = dict(f, rstd=fm["m_rstd"].float().double(), xh=(x - fm["m_mean"][:, None]) * fm["m_rstd"].float().double()[:, None])
    bm = LB.bwd(fk, x, dy, g, add_in=add, row_scale=rs, keep=km, skip_rows=slice(R - rpb, R) if mut == "dgamma_last_block_missing" else None)
    got = dict(y=fm["m_y"], y32=fm["m_y32"].float().double(), mean=fm["m_mean"].float().double(), rstd=fm["m_rstd"].float().double(),
               dx=bm["m_dx"], dx2=bm["m_dx2"], dgamma=bm["m_dgamma"].float().double(), dbeta=bm["m_dbeta"].float().double(),
               colsum=bm["m_colsum"].float().double())
    return LB.check_all(got, ref, rpb)


@pytest.mark.parametrize("fam", list(LN_FAM))
def test_layernorm_rounding_model_is_accepted(fam):
    fails, stats = _ln_emulate(fam)
    print(fam, {k: (f"{e:.3g}", f"{t:.3g}") for k, (e, t) in stats.items()})
    assert not fails, fails
    assert all(e <= 1.0 and t <= 1.0 for e, t in stats.values()), stats


@pytest.mark.parametrize("mut", list(LN_MUT))
def test_layernorm_mutation_is_rejected(mut):
    fails, stats = _ln_emulate(LN_MUT[mut], mut)
    print(mut, {k: (f"{e:.3g}", f"{t:.3g}") for k, (e, t) in stats.items()})
    assert fails, f"{LN_MUT[mut]}: the bound accepts the mutation {mut}"


def test_layernorm_geometry_reaches_every_instantiation():
    """pick_geom over the C of tests/test_gpu_layernorm_bounds.py reaches every LN_DISPATCH_T branch (layernorm.hip:332-342)"""
    from tests.test_gpu_layernorm_bounds import CS
    seen = {LB.geometry(C, fwd)[:2] for C in CS for fwd in (True, False)}
    assert seen >= {(16, 3), (16, 1), (32, 3), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4), (64, 6)}, seen
