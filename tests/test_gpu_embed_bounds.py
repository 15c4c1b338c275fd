"""GPU: the embedding and gather kernels (lav_text_embed_fwd / bwd, lav_video_embed_fwd / bwd, lav_text_embed_rows_fwd, lav_gather_sum_rows)
against the float64 references and derived bounds of tests/embed_bounds.py -- per-element bound and per-block check against the rounding model --
and lav_patch_im2col / lav_gather_rows bit for bit against the rearranged input.  The shapes are the smallest at which each path of the kernels
runs (tests/test_embed_bounds_host.py holds the same bounds to an emulation of every kernel and to injected bugs); the two grid-cap cases are the
only large ones."""
import pytest
import torch

from tests import embed_bounds as EB
from tests.test_embed_bounds_host import (GSUM_C, IM2COL_SHAPES, ROWS_SHAPES, TEXT_SHAPES, VIDEO_SHAPES, gsum_inputs, rows_inputs,
                                          rows_reference, same_bits)

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
SENTINEL = -77.0


def _report(tag, fails, stats):
    print(f"\n{tag}: " + ", ".join(f"{t} {e:.3g}/{r:.3g}" for t, (e, r) in stats.items()))
    for f in fails:
        print("  " + f)


def _cpu(got):
    return {k: v.detach().cpu() for k, v in got.items()}


# ---- text embedding ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", (0.0, 0.1))
@pytest.mark.parametrize("shape", TEXT_SHAPES, ids=lambda s: "n%d_X%d_Hd%d" % s)
def test_text_embed(shape, p):
    from lavender_amd import hip
    n, X, Hd = shape
    eps, seed = 1e-12, 4242 + Hd
    d = EB.text_inputs(n, X, Hd, seed=11)
    c = {k: v.cuda() for k, v in d.items() if k != "init"}
    out = torch.full((n * X, Hd), SENTINEL, dtype=bf16, device="cuda")
    _, mean, rstd = hip.text_embed_fwd(c["ids"], n, X, Hd, c["word"], c["pos"], c["type"], c["gamma"], c["beta"], eps, p, seed, out=out)
    g = {k: v.clone().cuda() for k, v in d["init"].items()}
    hip.text_embed_bwd(c["ids"], c["dout"], n, X, Hd, c["word"], c["pos"], c["type"], c["gamma"], mean, rstd, p, seed, g["d_word"], g["d_pos"],
                       g["d_type0"], g["dgamma"], g["dbeta"])
    torch.cuda.synchronize()
    got = _cpu(dict(y=out, mean=mean, rstd=rstd, **g))
    ref = EB.text_reference(d, eps, p, seed)
    fails, stats = EB.check_all(got, ref)
    _report(f"text n={n} X={X} Hd={Hd} p={p}", fails, stats)
    assert fails == []
    assert len(stats) == 8
    # what no row maps to stays bit-identical: the type table's second row, the unused vocabulary rows, the position rows past X
    hit = torch.zeros(d["word"].shape[0], dtype=torch.bool)
    hit[d["ids"].reshape(-1)] = True
    assert int((~hit).sum()) >= 8
    assert torch.equal(got["d_type0"][1], d["init"]["d_type0"][1])
    assert torch.equal(got["d_word"][~hit], d["init"]["d_word"][~hit])
    assert torch.equal(got["d_pos"][X:], d["init"]["d_pos"][X:])


# ---- video token assembly -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", (0, 7))
@pytest.mark.parametrize("shape", VIDEO_SHAPES, ids=lambda s: "B%d_T%d_hw%d_Hd%d" % s)
def test_video_embed(shape, pad):
    from lavender_amd import hip
    B, T, hw, Hd = shape
    eps = 1e-5
    Lv = T * (1 + hw)
    seq_rows = Lv + pad
    d = EB.video_inputs(B, T, hw, Hd, seed=12)
    c = {k: v.cuda() for k, v in d.items() if k != "init"}
    out = torch.full((B, seq_rows, Hd), SENTINEL, dtype=bf16, device="cuda")
    dout = torch.full((B, seq_rows, Hd), SENTINEL, dtype=bf16, device="cuda")
    dout[:, :Lv] = c["dout"].view(B, Lv, Hd)
    mean, rstd = hip.video_embed_fwd(c["feat"], B, T, hw, Hd, c["cls"], c["pos"], c["len"], c["gamma"], c["beta"], eps, out, seq_rows)
    g = {k: v.clone().cuda() for k, v in d["init"].items()}
    dfeat = torch.full_like(c["feat"], float("nan"))
    hip.video_embed_bwd(dout, seq_rows, c["feat"], B, T, hw, Hd, c["cls"], c["pos"], c["len"], c["gamma"], mean, rstd, dfeat, g["d_cls"],
                        g["d_pos"], g["d_len"], g["dgamma"], g["dbeta"])
    torch.cuda.synchronize()
    got = _cpu(dict(y=out[:, :Lv].reshape(B * Lv, Hd), mean=mean, rstd=rstd, dfeat=dfeat, **g))
    ref = EB.video_reference(d, B, T, hw, eps)
    fails, stats = EB.check_all(got, ref)
    _report(f"video B={B} T={T} hw={hw} Hd={Hd} seq_rows={seq_rows}", fails, stats)
    assert fails == []
    assert len(stats) == 9
    assert not bool(torch.isnan(got["dfeat"].float()).any())
    tail = torch.full((B, pad, Hd), SENTINEL, dtype=bf16)
    assert same_bits(out[:, Lv:].cpu(), tail) and same_bits(dout[:, Lv:].cpu(), tail)
    assert torch.equal(got["d_pos"][1 + hw:], d["init"]["d_pos"][1 + hw:]) and torch.equal(got["d_len"][T:], d["init"]["d_len"][T:])


# ---- single rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ROWS_SHAPES, ids=lambda s: "n%d_Hd%d" % s)
def test_text_embed_rows(shape):
    from lavender_amd import hip
    n, Hd = shape
    d = rows_inputs(n, Hd)
    c = {k: v.cuda() for k, v in d.items() if k not in ("init", "dout")}
    out = torch.full((n + 1, Hd), SENTINEL, dtype=bf16, device="cuda")
    hip.text_embed_rows(c["ids"], c["pos_ids"], Hd, c["word"], c["pos"], c["type"], c["gamma"], c["beta"], 1e-12, out)
    torch.cuda.synchronize()
    fails, stats = EB.check_all(dict(y=out[:n].cpu()), rows_reference(d, 1e-12))
    _report(f"rows n={n} Hd={Hd}", fails, stats)
    assert fails == []
    assert bool((out[n] == SENTINEL).all())


# ---- gather_sum ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", GSUM_C)
def test_gather_sum_rows(C):
    from lavender_amd import hip
    wide, src, start, lst = gsum_inputs(C)
    wd = wide.cuda()
    out = hip.gather_sum_rows(wd[:, 8:8 + C], start.cuda(), lst.cuda(), len(start) - 1, C)
    torch.cuda.synchronize()
    ref = EB.gather_sum(src.double(), start.long(), lst)
    fails, stats = EB.check_all(dict(out=out.cpu()), ref)
    _report(f"gather_sum C={C}", fails, stats)
    assert fails == []
    assert bool((out[0].view(torch.int16) == 0).all()) and bool((out[4].view(torch.int16) == 0).all())


# ---- im2col, gather_rows: bit-exact ---------------------------------------------------------------------------------------------------------
IM2COL_CASES = [(s, fm) for s in IM2COL_SHAPES for fm in (True, False)] + [((2, 3, 1936, 1936), True)]


@pytest.mark.parametrize("shape,frame_major", IM2COL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("frame_major" if v else "channel_major"))
def test_patch_im2col_bits(shape, frame_major):
    """the last shape has 16.87 M chunks, above the 65535 x 256 threads of the capped grid: the grid-stride loop takes a second trip"""
    from lavender_amd import hip
    B, T, H, W = shape
    if H > 100:
        assert B * T * (H // 4) * 12 * (W // 4) > 65535 * 256
    img = EB.im2col_input(B, T, H, W, frame_major, seed=3, device="cuda")
    out = hip.patch_im2col(img, B, T, H, W, frame_major)
    ref = EB.im2col_ref(img, B, T, H, W, frame_major)
    torch.cuda.synchronize()
    assert same_bits(out, ref), f"{int((out.view(torch.int16) != ref.view(torch.int16)).sum())} of {ref.numel()} values differ"
    assert bool((ref.view(torch.int16) == 0x7F80).any()) and bool((ref.view(torch.int16) == -32768).any())          # the overflow tie, -0


def _gather_rows_case(n_rows, C, src_rows, seed):
    from lavender_amd import hip
    gen = torch.Generator(device="cuda").manual_seed(seed)
    wide = torch.randn(src_rows, C + 16, generator=gen, device="cuda").bfloat16()
    src = wide[:, 8:8 + C]                                    # a column slice: lds = C + 16
    idx = torch.randint(0, src_rows, (n_rows,), generator=gen, device="cuda", dtype=torch.int32)
    idx[1] = idx[0]
    idx[n_rows // 2] = -1
    idx[n_rows - 1] = -1
    dst = torch.full((n_rows, C + 24), SENTINEL, dtype=bf16, device="cuda")
    hip.gather_rows(src, idx, n_rows, C, out=dst[:, 16:16 + C])
    torch.cuda.synchronize()
    ref = EB.gather_rows_ref(src, idx)
    assert same_bits(dst[:, 16:16 + C], ref)
    assert bool((dst[n_rows - 1, 16:16 + C].view(torch.int16) == 0).all())
    assert bool((dst[:, :16] == SENTINEL).all()) and bool((dst[:, 16 + C:] == SENTINEL).all())


@pytest.mark.parametrize("C", (8, 200, 768))
def test_gather_rows_bits(C):
    _gather_rows_case(37, C, 40, C)


def test_gather_rows_grid_cap():
    """140000 x 128 chunks, above the 65535 x 256 threads of the capped grid"""
    assert 140000 * (1024 // 8) > 65535 * 256
    _gather_rows_case(140000, 1024, 1000, 9)
