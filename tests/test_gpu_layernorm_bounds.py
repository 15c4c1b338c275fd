"""GPU: lav_layernorm_fwd / lav_layernorm_bwd against the float64 reference of tests/layernorm_bounds.py (per-element bound, per-row-block check
against the rounding model) on every LN_DISPATCH_T instantiation, every input type, the fp32 output copy, the patch-merge gather, add_in, dx2 with
dropout and row scale, column sums, and the four ways the backward finishes its column reductions (in-kernel atomics, immediate partials,
deferred partials, the grid capped at 768 blocks); each case states its path and the test recomputes it from the host copy of the geometry."""
import pytest
import torch

from tests import layernorm_bounds as LB
from tests.helpers import hidden_keep_multiplier

pytestmark = pytest.mark.gpu
CS = (96, 128, 136, 256, 264, 384, 512, 520, 768, 1024, 1032, 2048, 2056, 3072)


def _x(R, C, kind, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(R, C, generator=g, device="cuda")
    if kind == "offset":
        x = x + 1e3
    if kind == "offset_bf16":                                # bf16 rows around 1e3 (spacing 4 there: a spread of a few steps)
        return (x * 8 + 1e3).bfloat16()
    if kind == "const":
        x = torch.full((R, C), 0.37, device="cuda")
    if kind in ("bf16", "const"):
        return x.bfloat16()
    if kind == "fp16":
        return x.half()
    return x


def _run(R, C, kind="bf16", eps=1e-12, y32=False, gather=None, add_in=False, dx2=False, defer=True, seed=0):
    from lavender_amd import _lib, hip
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    x = _x(R, C, kind, seed)
    gamma = torch.randn(C, generator=g, device="cuda") * 0.5 + 1.0
    beta = torch.randn(C, generator=g, device="cuda") * 0.1
    dy = torch.randn(R, C, generator=g, device="cuda").bfloat16()
    xr = x
    if gather is not None:                                   # patch merge: x is (B T, H, W, C0), row r gathers the 2 x 2 patch (video_swin.py:271-284)
        H, W, C0 = gather
        xr = x.reshape(-1, H // 2, 2, W // 2, 2, C0).permute(0, 1, 3, 4, 2, 5).reshape(R, C)
    o32 = torch.empty(R, C, device="cuda") if y32 else None
    res = hip.layernorm_fwd(x, R, C, gamma, beta, eps, gather=gather, out32=o32)
    y, mean, rstd = res[0], res[1], res[2]
    ad = torch.randn(R, C, generator=g, device="cuda").bfloat16() if add_in else None
    ad_k = ad
    if add_in and gather is not None:                        # add_in is read in the gathered layout
        H, W, C0 = gather
        ad_k = ad.reshape(-1, H // 2, W // 2, 2, 2, C0).permute(0, 1, 4, 2, 3, 5).reshape(-1, C0)
    dgamma = torch.zeros(C, device="cuda")
    dbeta = torch.zeros(C, device="cuda")
    kw = {}
    rs = keep = None
    if dx2:
        kw = dict(dx2=torch.empty(R, C, dtype=torch.bfloat16, device="cuda"), row_scale=torch.tensor([1.25, 0.0, 0.75], device="cuda"),
                  rows_per_group=(R + 2) // 3, dropout_p=0.1, seed=seed + 7, colsum=torch.zeros(C, device="cuda"))
        rs = kw["row_scale"].double().repeat_interleave(kw["rows_per_group"])[:R]
        keep = hidden_keep_multiplier(seed + 7, R, C, 0.1).double().cuda()
    sp = torch.cuda.current_stream().cuda_stream
    hip.ensure_workspace(hip.WS_LN_DEFER)
    old = _lib.lib.lav_layernorm_set_defer(torch.cuda.current_stream().cuda_stream, 1 if defer else 0)
    try:
        dx = hip.layernorm_bwd(dy, x, R, C, gamma, mean, rstd, dgamma, dbeta, gather=gather, add_in=ad_k, **kw)
        torch.cuda.synchronize()
    finally:
        _lib.lib.lav_layernorm_set_defer(sp, old)
    if gather is not None:
        H, W, C0 = gather
        dx = dx.reshape(-1, H // 2, 2, W // 2, 2, C0).permute(0, 1, 3, 4, 2, 5).reshape(R, C)
    xd = xr.double()
    f = LB.fwd(xd, gamma.double(), beta.double(), eps, y32=y32)
    ref = dict(f)
    ref.update(LB.bwd(f, xd, dy.double(), gamma.double(), add_in=ad.double() if add_in else None, row_scale=rs, keep=keep, want_dx2=dx2))
    got = dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta)
    if y32:
        got["y32"] = o32
    if dx2:
        got["dx2"], got["colsum"] = kw["dx2"], kw["colsum"]
    G, inst, rpb = LB.geometry(C)
    fails, stats = LB.check_all(got, ref, rpb)
    return fails, stats, (G, inst, LB.geometry(C, False)[:2])


@pytest.mark.parametrize("C", CS)
def test_layernorm_every_width(C):
    """every forward / backward geometry, bf16 rows, immediate + deferred column sums (grid >= 64), fp32 output copy"""
    R = 64 * 256 // LB.geometry(C, False)[0] + 37
    fails, stats, geo = _run(R, C, y32=True, add_in=True, dx2=True, seed=C)
    print(f"\nC={C} rows={R} fwd G{geo[0]}x{geo[1]} bwd G{geo[2][0]}x{geo[2][1]}: " + ", ".join(f"{t} {e:.3g}/{r:.3g}" for t, (e, r) in stats.items()))
    assert not fails, fails


CASES = {   # rows, C, input, eps, deferred mode on, how the backward finishes its column sums, extras
    "atomics_grid_lt_64": (251, 512, "bf16", 1e-12, True, "atomics", dict(dx2=True, add_in=True)),
    "atomics_grid_lt_64_c128": (63 * 16 - 5, 128, "bf16", 1e-12, True, "atomics", dict(dx2=True)),
    "immediate_partials": (2051, 384, "bf16", 1e-12, False, "immediate", dict(dx2=True)),
    "deferred_partials": (2051, 384, "bf16", 1e-12, True, "deferred", dict(dx2=True)),
    "grid_cap_768_c512": (3 * 3072 + 517, 512, "bf16", 1e-12, True, "deferred+cap", dict(dx2=True)),
    "grid_cap_768_c128": (2 * 12288 + 4100, 128, "bf16", 1e-12, False, "immediate+cap", dict(dx2=True)),
    "grid_cap_768_c1032": (3 * 3072 + 5, 1032, "bf16", 1e-12, True, "deferred+cap", dict(dx2=True)),
    "fp32_rows_y32": (2000, 768, "fp32", 1e-12, True, "deferred", dict(y32=True)),
    "fp16_rows": (2000, 768, "fp16", 1e-12, True, "deferred", dict(add_in=True)),
    "offset_rows_fp32": (1000, 768, "offset", 1e-12, True, "deferred", dict(y32=True)),
    "offset_rows_bf16": (1000, 1024, "offset_bf16", 1e-12, True, "deferred", {}),
    "constant_rows": (500, 256, "const", 1e-5, True, "atomics", {}),
    "patch_merge_gather": (2 * 4 * 7 * 7, 512, "bf16", 1e-5, True, "deferred", dict(gather=(14, 14, 128), add_in=True)),
    "patch_merge_c384": (2 * 8 * 7 * 7, 384, "bf16", 1e-5, True, "deferred", dict(gather=(14, 14, 96))),
}


def reduction_path(R, C, defer):
    """lav_layernorm_bwd (layernorm.hip:451-470): grid = ceil(rows / rows per block), capped at 768; below 64 blocks the kernel adds its column sums
    with atomics, otherwise it writes per-block partials that a finish pass sums, queued (deferred mode) or launched at once"""
    G = LB.geometry(C, False)[0]
    grid = -(-R // (256 // G))
    if grid < 64:
        return "atomics"
    return ("deferred" if defer else "immediate") + ("+cap" if grid > 768 else "")


@pytest.mark.parametrize("cid", list(CASES))
def test_layernorm_paths(cid):
    R, C, kind, eps, defer, path, ex = CASES[cid]
    assert reduction_path(R, C, defer) == path, f"{cid}: rows {R} at C {C} reduce by {reduction_path(R, C, defer)}, the case was written for {path}"
    if path.endswith("+cap"):
        rstride = 768 * (256 // LB.geometry(C, False)[0])
        assert R % rstride and R % (2 * rstride), f"{cid}: rows must not be a multiple of the grid stride"
    fails, stats, geo = _run(R, C, kind=kind, eps=eps, defer=defer, seed=R, **ex)
    print(f"\n{cid} ({path}): fwd G{geo[0]}x{geo[1]} bwd G{geo[2][0]}x{geo[2][1]}: " + ", ".join(f"{t} {e:.3g}/{r:.3g}" for t, (e, r) in stats.items()))
    assert not fails, fails
