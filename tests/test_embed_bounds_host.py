"""CPU: the embedding and gather bounds of tests/embed_bounds.py can fail.  Each kernel of lavender_amd/csrc/embed.hip (and embed_rows_kernel of
decode.hip) is emulated in fp32 torch -- the kernel's association, its bf16 stores, a shuffled order for the sums its atomics form -- at every shape
of tests/test_gpu_embed_bounds.py: check_all must accept the emulation, and with each injected kernel bug it must reject it, at the smallest
shape of the table that can show the bug.  Every case prints its largest err/bound and block ratio."""
import numpy as np
import pytest
import torch

from tests import embed_bounds as EB
from tests.helpers import hidden_keep_multiplier

torch.set_num_threads(min(16, torch.get_num_threads()))

TEXT_SHAPES = [(3, 5, Hd) for Hd in (8, 128, 520, 768, 1024)] + [(9, 3, 768), (33, 2, 768), (40, 1, 768)]
VIDEO_SHAPES = [(B, T, hw, 768) for B in (1, 2, 5, 9) for T, hw in ((1, 1), (3, 4))] + [(5, 3, 4, Hd) for Hd in (8, 520, 1024)]
ROWS_SHAPES = [(n, Hd) for Hd in (7, 250, 768, 1024) for n in (1, 5)]
GSUM_C = (8, 64, 2304)
GSUM_SEG = (0, 1, 2, 300, 0)
IM2COL_SHAPES = [(1, 1, 4, 4), (2, 3, 8, 12)]
SEED = 4242


def _seq_sum(init, rows, index, order):
    """table[index[r]] += rows[r] in fp32, one row after the other in the given order (what atomics do, in some order)"""
    out = init.clone()
    for r in order:
        out[index[r]] += rows[r]
    return out


def _ln_fwd32(x, Hd, gamma, beta, eps, lim=None, one_pass=False):
    xs = x if lim is None else x[:, :lim]
    mean = xs.sum(1) / Hd
    d = x - mean[:, None]
    if one_pass:
        var = (xs * xs).sum(1) / Hd - mean * mean
    else:
        ds = d if lim is None else d[:, :lim]
        var = (ds * ds).sum(1) / Hd
    rstd = torch.rsqrt((var + np.float32(eps)).clamp_min(1e-30))
    return mean, rstd, d * rstd[:, None] * gamma + beta


def _ln_bwd32(x, mean, rstd, dd, gamma, Hd):
    xh = (x - mean[:, None]) * rstd[:, None]
    gy = gamma * dd
    m1, m2 = gy.sum(1) / Hd, (gy * xh).sum(1) / Hd
    return xh, rstd[:, None] * (gy - m1[:, None] - xh * m2[:, None])


# ---- text embedding ---------------------------------------------------------------------------------------------------------------------
def emulate_text(d, eps, p, seed, mut=None):
    ids = d["ids"]
    n, X = ids.shape
    R, Hd = n * X, d["word"].shape[1]
    idf, xp = ids.reshape(-1), torch.arange(X).repeat(n)
    sq = torch.arange(R) // X
    gamma, beta = d["gamma"], d["beta"]
    x = (d["word"][idf] + d["pos"][xp]) + d["type"][0]
    mean, rstd, y = _ln_fwd32(x, Hd, gamma, beta, eps, lim=512 if mut == "sums_skip_512" else None, one_pass=mut == "one_pass")
    inv = np.float32(1) / (np.float32(1) - np.float32(p))
    km = None
    if p > 0:
        km = hidden_keep_multiplier(seed, R, Hd + 8, p)[:, :Hd] > 0 if mut == "mask_stride" else hidden_keep_multiplier(seed, R, Hd, p) > 0
        y = torch.where(km, y * inv, torch.zeros_like(y))
    out = y.bfloat16()
    if mut == "unwritten_512":
        out[:, 512:] = 0
    dd = d["dout"].float()
    if p > 0 and mut != "no_bwd_dropout":
        dd = torch.where(km, dd * inv, torch.zeros_like(dd))
    xh, dx = _ln_bwd32(x, mean, rstd, dd, gamma, Hd)
    groups = EB.text_groups(n)
    per = -(-n // groups)
    rows = torch.ones(R, dtype=torch.bool)                   # rows that reach any sum
    cols = torch.ones(R, dtype=torch.bool)                   # rows that reach the per-block column sums
    if mut == "last_group":                                  # the last group that holds a text never runs
        rows &= sq < (n - 1) // per * per
    if mut == "second_row":                                  # a wave's second trip (sq = s0 + 4 ...) misses the register sums
        cols &= sq % per < 4
    order = torch.randperm(R, generator=torch.Generator().manual_seed(R)).tolist()
    use = [r for r in order if rows[r]]
    usec = [r for r in use if cols[r]]
    i0 = d["init"]
    g = dict(y=out, mean=mean, rstd=rstd)
    if mut == "last_writer":
        g["d_word"] = i0["d_word"].clone()
        for r in use:
            g["d_word"][idf[r]] = i0["d_word"][idf[r]] + dx[r]
    else:
        g["d_word"] = _seq_sum(i0["d_word"], dx, idf, use)
    g["d_pos"] = _seq_sum(i0["d_pos"], dx, xp, usec)
    zero = torch.zeros(R, dtype=torch.long)
    g["d_type0"] = _seq_sum(i0["d_type0"], dx, zero, usec)
    g["dgamma"] = _seq_sum(i0["dgamma"][None], dd * xh, zero, usec)[0]
    g["dbeta"] = _seq_sum(i0["dbeta"][None], dd, zero, usec)[0]
    return g


def _text_case(n, X, Hd, p, mut=None, offset=0.0):
    d = EB.text_inputs(n, X, Hd, seed=1, offset=offset)
    ref = EB.text_reference(d, 1e-12, p, SEED)
    return EB.check_all(emulate_text(d, 1e-12, p, SEED, mut), ref)


def _report(tag, fails, stats):
    print(tag, {k: (f"{e:.3g}", f"{t:.3g}") for k, (e, t) in stats.items()})


@pytest.mark.parametrize("p", (0.0, 0.1))
@pytest.mark.parametrize("shape", TEXT_SHAPES, ids=lambda s: "n%d_X%d_Hd%d" % s)
def test_text_emulation_is_accepted(shape, p):
    fails, stats = _text_case(*shape, p)
    _report((shape, p), fails, stats)
    assert not fails, fails
    assert len(stats) == 8 and all(e <= 1.0 and t <= 1.0 for e, t in stats.values()), stats


def test_text_emulation_is_accepted_on_offset_rows():
    fails, stats = _text_case(3, 5, 768, 0.0, offset=1e3)
    _report("offset", fails, stats)
    assert not fails, fails


TEXT_MUT = {   # bug -> (n, X, Hd, p, word offset)
    "unwritten_512@520": ("unwritten_512", 3, 5, 520, 0.0, 0.0),
    "unwritten_512@768": ("unwritten_512", 3, 5, 768, 0.0, 0.0),
    "sums_skip_512@520": ("sums_skip_512", 3, 5, 520, 0.0, 0.0),
    "sums_skip_512@768": ("sums_skip_512", 3, 5, 768, 0.0, 0.0),
    "second_row@n9": ("second_row", 9, 3, 768, 0.0, 0.0),
    "last_group@n9": ("last_group", 9, 3, 768, 0.0, 0.0),
    "last_group@n33": ("last_group", 33, 2, 768, 0.0, 0.0),
    "last_writer": ("last_writer", 3, 5, 8, 0.0, 0.0),
    "no_bwd_dropout": ("no_bwd_dropout", 3, 5, 8, 0.1, 0.0),
    "mask_stride": ("mask_stride", 3, 5, 8, 0.1, 0.0),
    "one_pass": ("one_pass", 3, 5, 768, 0.0, 1e3),
}


@pytest.mark.parametrize("mid", list(TEXT_MUT))
def test_text_mutation_is_rejected(mid):
    mut, n, X, Hd, p, off = TEXT_MUT[mid]
    fails, stats = _text_case(n, X, Hd, p, mut, off)
    _report(mid, fails, stats)
    assert fails, f"{mid}: the bound accepts the mutation"


# ---- video token assembly -----------------------------------------------------------------------------------------------------------------
def emulate_video(d, B, T, hw, eps, mut=None):
    P, Hd = 1 + hw, d["feat"].shape[1]
    b, t, p = EB.video_rows(B, T, hw)
    R = len(p)
    bt = b * T + t
    gamma, beta = d["gamma"], d["beta"]
    is_cls = (p == 0)[:, None]
    feat = d["feat"].float()[bt * hw + (p - 1).clamp_min(0)]
    li = bt % d["len"].shape[0] if mut == "len_by_bt" else t
    pi = torch.arange(R) % d["pos"].shape[0] if mut == "pos_flat" else p
    x0 = torch.where(is_cls, d["cls"][None, :].expand(R, Hd), feat + d["cls"] if mut == "cls_everywhere" else feat)
    x = (x0 + d["pos"][pi]) + d["len"][li]
    mean, rstd, y = _ln_fwd32(x, Hd, gamma, beta, eps)
    # backward: the kernel's own association of the row
    cls0 = d["cls"][None, :].expand(R, Hd) if mut == "cls_everywhere" else torch.where(is_cls, d["cls"][None, :].expand(R, Hd), torch.zeros(R, Hd))
    xe = (d["pos"][pi] + cls0) + d["len"][li]
    xb = torch.where(is_cls, xe, feat + xe)
    dd = d["dout"].float()
    xh, dx = _ln_bwd32(xb, mean, rstd, dd, gamma, Hd)
    order = torch.randperm(R, generator=torch.Generator().manual_seed(R)).tolist()
    if mut == "second_row":
        order = [r for r in order if b[r] < 4]
    i0 = d["init"]
    zero = torch.zeros(R, dtype=torch.long)
    return dict(y=y.bfloat16(), mean=mean, rstd=rstd, dfeat=dx[p > 0].bfloat16(), d_pos=_seq_sum(i0["d_pos"], dx, pi, order),
                d_len=_seq_sum(i0["d_len"], dx, li, order),
                d_cls=_seq_sum(i0["d_cls"][None], dx, zero, [r for r in order if p[r] == 0 or mut == "d_cls_all"])[0],
                dgamma=_seq_sum(i0["dgamma"][None], dd * xh, zero, order)[0], dbeta=_seq_sum(i0["dbeta"][None], dd, zero, order)[0])


def _video_case(B, T, hw, Hd, mut=None):
    d = EB.video_inputs(B, T, hw, Hd, seed=2, len_rows=B * T + 1 if mut == "len_by_bt" else None)
    ref = EB.video_reference(d, B, T, hw, 1e-5)
    return EB.check_all(emulate_video(d, B, T, hw, 1e-5, mut), ref)


@pytest.mark.parametrize("shape", VIDEO_SHAPES, ids=lambda s: "B%d_T%d_hw%d_Hd%d" % s)
def test_video_emulation_is_accepted(shape):
    fails, stats = _video_case(*shape)
    _report(shape, fails, stats)
    assert not fails, fails
    assert len(stats) == 9 and all(e <= 1.0 and t <= 1.0 for e, t in stats.values()), stats


VIDEO_MUT = {"second_row": (5, 3, 4, 8), "cls_everywhere": (1, 1, 1, 768), "d_cls_all": (1, 1, 1, 768), "len_by_bt": (2, 3, 4, 768),
             "pos_flat": (1, 3, 4, 768)}


@pytest.mark.parametrize("mut", list(VIDEO_MUT))
def test_video_mutation_is_rejected(mut):
    fails, stats = _video_case(*VIDEO_MUT[mut], mut)
    _report(mut, fails, stats)
    assert fails, f"{mut}: the bound accepts the mutation"


# ---- single rows --------------------------------------------------------------------------------------------------------------------------
def rows_inputs(n, Hd):
    d = EB.text_inputs(5, 6, 8 * ((Hd + 7) // 8), seed=3)
    for k in ("word", "pos", "type", "gamma", "beta"):
        d[k] = d[k][..., :Hd].contiguous()
    d["ids"] = torch.tensor([1, 7, 7, 1, 30])[:n]                 # repeats
    d["pos_ids"] = torch.tensor([4, 0, 8, 4, 2], dtype=torch.int32)[:n]          # not monotone, repeated, up to the table's last row
    return d


def rows_reference(d, eps):
    dd = lambda t: t.double()
    return EB.rows_fwd(d["ids"], d["pos_ids"].long(), dd(d["word"]), dd(d["pos"]), dd(d["type"][0]), dd(d["gamma"]), dd(d["beta"]), eps)


@pytest.mark.parametrize("shape", ROWS_SHAPES, ids=lambda s: "n%d_Hd%d" % s)
def test_rows_emulation_is_accepted(shape):
    n, Hd = shape
    d = rows_inputs(n, Hd)
    x = (d["word"][d["ids"]] + d["pos"][d["pos_ids"].long()]) + d["type"][0]
    y = _ln_fwd32(x, Hd, d["gamma"], d["beta"], 1e-12)[2]
    fails, stats = EB.check_all(dict(y=y.bfloat16()), rows_reference(d, 1e-12))
    _report(shape, fails, stats)
    assert not fails, fails
    if Hd > 512:                                             # and the same bounds reject a block that leaves the columns past 512 alone
        y[:, 512:] = 0
        assert EB.check_all(dict(y=y.bfloat16()), rows_reference(d, 1e-12))[0]


# ---- gather_sum ---------------------------------------------------------------------------------------------------------------------------
def gsum_inputs(C, seed=5):
    """segments of GSUM_SEG rows out of a 64-row source that is a column slice of a wider buffer; rows recur within and across segments"""
    gen = torch.Generator().manual_seed(seed + C)
    wide = torch.randn(64, C + 16, generator=gen).bfloat16()
    lst = torch.randint(0, 64, (sum(GSUM_SEG),), generator=gen, dtype=torch.int32)
    lst[1] = lst[0]                                          # the row of segment 1 again in segment 2
    start = torch.tensor([0] + list(np.cumsum(GSUM_SEG)), dtype=torch.int32)
    return wide, wide[:, 8:8 + C], start, lst


def emulate_gsum(src, start, lst, bf16_acc=False):
    out = torch.zeros(len(start) - 1, src.shape[1])
    for r in range(len(start) - 1):
        for k in range(int(start[r]), int(start[r + 1])):
            out[r] += src[int(lst[k])].float()
            if bf16_acc:
                out[r] = out[r].bfloat16().float()
    return out.bfloat16()


@pytest.mark.parametrize("C", GSUM_C)
def test_gather_sum_emulation_is_accepted_and_bf16_accumulation_rejected(C):
    _, src, start, lst = gsum_inputs(C)
    ref = EB.gather_sum(src.double(), start.long(), lst)
    fails, stats = EB.check_all(dict(out=emulate_gsum(src, start, lst)), ref)
    _report(C, fails, stats)
    assert not fails, fails
    assert bool((ref["b_out"][0] == 0).all()) and bool((ref["b_out"][4] == 0).all())          # empty segments: exact zeros
    fails, stats = EB.check_all(dict(out=emulate_gsum(src, start, lst, bf16_acc=True)), ref)
    _report((C, "bf16 accumulation"), fails, stats)
    assert fails, "the bound accepts a bf16 accumulator at k = 300"


# ---- im2col, gather_rows --------------------------------------------------------------------------------------------------------------------
def emulate_im2col(img, B, T, H, W, frame_major, mut=None):
    """the kernel's index arithmetic (embed.hip:10-27), one chunk of 8 values per index"""
    Hp, Wp = H // 4, W // 4
    idx = np.arange(B * T * Hp * 12 * Wp)
    pw, t1 = idx % Wp, idx // Wp
    chunk, t1 = t1 % 12, t1 // 12
    ph, t1 = t1 % Hp, t1 // Hp
    t, b = t1 % T, t1 // T
    c, kt, khp = chunk >> 2, (chunk >> 1) & 1, chunk & 1
    ts = t + kt - (1 if mut == "zero_frame_first" else 0)
    ok = (ts < T) & (ts >= 0)
    tsc = np.clip(ts, 0, T - 1)
    plane = (b * T + tsc) * 3 + c if frame_major else (b * 3 + c) * T + tsc
    base = plane * H * W + (4 * ph + 2 * khp) * W + 4 * pw
    flat = img.reshape(-1)
    off = np.concatenate([np.arange(4), W + np.arange(4)])
    v = flat[torch.from_numpy(base[:, None] + off[None, :])]
    v = torch.where(torch.from_numpy(ok)[:, None], v, torch.zeros_like(v))
    row = ((b * T + t) * Hp + ph) * Wp + pw
    slot = c * 32 + (khp * 16 + kt * 8 if mut == "kt_khp_swapped" else kt * 16 + khp * 8)
    out = torch.zeros(B * T * Hp * Wp, 96, dtype=torch.bfloat16)
    out.view(-1)[torch.from_numpy(row[:, None] * 96 + slot[:, None] + np.arange(8)[None, :])] = v.bfloat16()
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("frame_major", (True, False))
@pytest.mark.parametrize("shape", IM2COL_SHAPES)
def test_im2col_reference_is_the_kernels_index_arithmetic(shape, frame_major):
    B, T, H, W = shape
    img = EB.im2col_input(B, T, H, W, frame_major)
    ref = EB.im2col_ref(img, B, T, H, W, frame_major)
    assert same_bits(emulate_im2col(img, B, T, H, W, frame_major), ref)
    assert bool(torch.isinf(ref.float()).any()) and bool((ref.view(torch.int16) == -32768).any())          # the overflow tie and -0 are in the frames
    if T == 1:
        assert bool((ref.view(-1, 3, 2, 16)[:, :, 1] == 0).all())                                        # every kt = 1 slot is the zero frame
    for mut in ("kt_khp_swapped", "zero_frame_first"):
        assert not same_bits(emulate_im2col(img, B, T, H, W, frame_major, mut), ref), mut


def test_im2col_reference_matches_conv3d():
    """the reference rearrangement against PatchEmbed3D's own Conv3d on bf16-exact frames"""
    import torch.nn.functional as F
    B, T, H, W, E = 2, 3, 8, 12, 5
    img = torch.randn(B, T, 3, H, W, generator=torch.Generator().manual_seed(0)).bfloat16().float()
    w = torch.randn(E, 3, 2, 4, 4, generator=torch.Generator().manual_seed(1)).double()
    cols = EB.im2col_ref(img, B, T, H, W, True).double()
    x = F.pad(img.transpose(1, 2), (0, 0, 0, 0, 0, 1)).double()
    ref = F.conv3d(x, w, None, stride=(1, 4, 4)).permute(0, 2, 3, 4, 1).reshape(-1, E)
    assert torch.allclose(cols @ w.view(E, 96).t(), ref, rtol=1e-12, atol=1e-12)


def test_gather_rows_reference():
    src = torch.randn(10, 24).bfloat16()[:, 8:16]
    idx = torch.tensor([3, 3, -1, 9, 0], dtype=torch.int32)
    ref = EB.gather_rows_ref(src, idx)
    assert same_bits(ref[0], src[3]) and same_bits(ref[1], src[3]) and same_bits(ref[3], src[9]) and bool((ref[2].view(torch.int16) == 0).all())
