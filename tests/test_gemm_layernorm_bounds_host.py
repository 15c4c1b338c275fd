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
    """the host copy of the selector on shapes whose choice is worked out by hand from gemm.hip:1765-1931"""
    assert GB.route(0, 193, 136, 192, 192, 192) == [("gemm_kernel", (128, 128))]
    assert GB.route(0, 8448, 2048, 128, 128, 128, dict(bias=True, act=1, preact="grad")) == [("gemm_ps_kernel", (192, 256))]
    assert GB.route(0, 8448, 2048, 128, 128, 128, dict(bias=True, act=1, preact="grad"), ps=0) == [("gemm_h192l_kernel", (192, 256))]
    assert GB.route(0, 45120, 768, 128, 128, 128, dict(bias=True)) == [("gemm_ps_kernel", (192, 256))]
    assert GB.route(0, 45120, 768, 128, 128, 128, dict(bias=True), ps=0) == [("gemm_h192l_kernel", (192, 256))]
    assert GB.route(1, 45120, 768, 128, 128, 768, dict(bias=True)) == [("gemm_h192_kernel", (192, 256))]
    assert GB.route(2, 1024, 512, 7840, 1024, 512, dict(out="acc", k_keep_rpg=245), 3) == [("gemm_pp_kernel", (256, 256)), ("tn_reduce_kernel", (256, 128))]
    r = GB.route(2, 768, 768, 30280, 768, 768, dict(out="acc"), 4)
    assert [k for k, _ in r] == ["gemm_pp_kernel", "tn_reduce_kernel", "gemm_kernel"]


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
