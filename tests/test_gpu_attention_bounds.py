"""GPU: every attention path held to the float64 reference and the derived per-element bounds of tests/attention_bounds.py -- forward O, the
log2-domain lse, the delta scratch behind it, dQ / dK / dV and the bias-table gradient -- plus the per-slice relative-norm check against the
rounding model, and exact (bit-for-bit) invariants: masked keys, the seq2seq block structure, window independence and repeatability.

Paths are chosen by shape (the env probes LAV_SEQL / LAV_WINL stay at their defaults) and every case asserts the route it expects against the
library's own plan (lav_attention_plan) before it launches: window persistent (N <= 256 with the fragment tables), window large (N <= 768
without them, winl_*, 1 or 3 query parts), window generic (N > 768, or lav_winl_select(-1)), sequence one-image (L <= 288), chunked
(289 <= L <= 768), generic (L > 768), and the decode attention with its split-K combine.

The delta scratch: lav_attention_bwd stores delta = sum_d dO O behind the lse; the persistent window route stores it NEGATED (win_bwd1 writes
-delta, the C operand of its dP MFMAs, and win_dbias3 reads it), every other route stores +delta.  The sign is taken from the plan."""
import pytest
import torch

from tests import attention_bounds as AB

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
DEV = "cuda"


def K():
    from lavender_amd import hip
    return hip


def _rb(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(bf16).to(DEV)


def _assert(fails, what, stats):
    print(f"\nBOUNDS {what}: " + " ".join(f"{t}={er:.3f}/{sr:.3f}" for t, (er, sr) in stats.items()))
    assert not fails, f"{what}: " + "; ".join(fails)


def _scratch(buf, G, N):
    Npad = buf.numel() // (2 * G)
    assert Npad % 32 == 0 and Npad >= N
    lse = buf[:G * Npad].view(G, Npad)[:, :N]
    delta = buf[G * Npad:].view(G, Npad)[:, :N]
    return lse, delta


# ---------------------------------------------------------------------------------------------------------------------------- window
WIN_CASES = {   # B, D, H, W, heads, window, shift, configured window, qkv_headmajor, lav_winl_select parts (None = not set)
    "p49": (2, 1, 14, 14, 1, (1, 7, 7), (0, 3, 3), (8, 7, 7), 0, None),
    "p180_clamped": (1, 5, 12, 12, 2, (5, 6, 6), (0, 3, 3), (8, 12, 12), 0, None),
    "p245_shift": (2, 5, 14, 14, 2, (5, 7, 7), (0, 3, 3), (8, 7, 7), 0, None),
    "p245_shift_hm": (2, 5, 14, 14, 2, (5, 7, 7), (0, 3, 3), (8, 7, 7), 1, None),
    "p256": (1, 8, 16, 16, 2, (4, 8, 8), (2, 4, 4), (4, 8, 8), 0, None),
    "l288": (1, 4, 24, 24, 1, (2, 12, 12), (1, 6, 6), (2, 12, 12), 0, None),
    "l288_parts1": (1, 4, 24, 24, 1, (2, 12, 12), (1, 6, 6), (2, 12, 12), 0, 1),
    "l392": (1, 16, 14, 14, 1, (8, 7, 7), (4, 3, 3), (8, 7, 7), 0, None),
    "l720_shift": (1, 5, 24, 24, 2, (5, 12, 12), (0, 6, 6), (8, 12, 12), 0, None),
    "l720_shift_parts1": (1, 5, 24, 24, 2, (5, 12, 12), (0, 6, 6), (8, 12, 12), 0, 1),
    "g392": (1, 16, 14, 14, 1, (8, 7, 7), (4, 3, 3), (8, 7, 7), 0, -1),
    "g800": (1, 8, 10, 20, 1, (8, 10, 10), (0, 5, 5), (8, 10, 10), 0, None),
}
PERSISTENT = ("window persistent", ["win_fwd3"], ["win_bwd1", "win_dbias3"])        # route, forward kernels, kernels of the backward with the bias-table gradient
LARGE = ("window large", ["winl_fwd"], ["winl_dq", "winl_dkv", "winl_dbias"])
GENERIC = ("generic window", ["attn_fwd_kernel"], ["attn_bwd_dq_kernel", "attn_bwd_dkv_kernel"])
WIN_ROUTES = {   # expected route and, on the large-window route, query parts per problem (few problems: 3 unless lav_winl_select forces 1)
    "p49": (PERSISTENT, None), "p180_clamped": (PERSISTENT, None), "p245_shift": (PERSISTENT, None), "p245_shift_hm": (PERSISTENT, None),
    "p256": (PERSISTENT, None), "l288": (LARGE, 3), "l288_parts1": (LARGE, 1), "l392": (LARGE, 3), "l720_shift": (LARGE, 3),
    "l720_shift_parts1": (LARGE, 1), "g392": (GENERIC, None), "g800": (GENERIC, None),
}
assert set(WIN_ROUTES) == set(WIN_CASES)


def _assert_route(att, route, parts=None):
    """the library's plan for this descriptor names the expected route and kernels; returns whether the route keeps -delta"""
    name, fwd_kernels, bwd_kernels = route
    fwd, bwd = att.plan(0), att.plan(2)
    assert {l.route.decode() for l in fwd + bwd} == {name}, [l.route for l in fwd + bwd]
    assert [l.kernel.decode() for l in fwd] == fwd_kernels and [l.kernel.decode() for l in bwd] == bwd_kernels
    if parts is not None:
        assert [l.split for l in fwd + bwd[:2]] == [parts] * 3
    return bool(fwd[0].delta_negated)


class _WinSelect:
    def __init__(self, parts):
        self.parts = parts

    def __enter__(self):
        if self.parts is not None:
            from lavender_amd import _lib
            self.old = _lib.lib.lav_winl_select(self.parts)

    def __exit__(self, *exc):
        if self.parts is not None:
            from lavender_amd import _lib
            _lib.lib.lav_winl_select(self.old)


def _win_run(name, qkv, table, dout, split=False):
    """forward + backward of one window launch on the route WIN_ROUTES expects; returns (att, out, lse buffer, dqkv, dtab)"""
    B, D, H, W, heads, win, shift, cfg, hm, parts = WIN_CASES[name]
    M, C = B * D * H * W, heads * 32
    x = qkv.view(M, 3, heads, 32).permute(1, 2, 0, 3).contiguous().view(M, 3 * C) if hm else qkv
    att = K().Attn(0, heads, 32, B=B, D=D, H=H, W=W, wd=win[0], wh=win[1], ww=win[2], sd=shift[0], sh=shift[1], sw=shift[2],
                   cfg_wd=cfg[0], cfg_wh=cfg[1], cfg_ww=cfg[2], bias_table=table, qkv_headmajor=hm)
    N = win[0] * win[1] * win[2]
    assert (N <= 256) == hasattr(att, "comb")
    with _WinSelect(parts):
        att.negated = _assert_route(att, *WIN_ROUTES[name])
        buf = torch.full((att.lse_elems(),), float("nan"), device=DEV)
        out = torch.empty(M, C, dtype=bf16, device=DEV)
        att.fwd(x, out, buf)
        dqkv, dtab = torch.empty(M, 3 * C, dtype=bf16, device=DEV), torch.zeros_like(table)
        att.split_ok = att.split_bias_grad             # persistent and large-window paths: win_dbias3 / winl_dbias (bf16 dS)
        if split:
            assert att.split_bias_grad
            att.bwd(x, out, dout, buf, dqkv, None)
            att.bwd_bias(x, dout, buf, dtab)
        else:
            att.bwd(x, out, dout, buf, dqkv, dtab)
    torch.cuda.synchronize()
    return att, out, buf, dqkv, dtab


def _win_inputs(case, seed=0):
    B, D, H, W, heads, win, shift, cfg = case[:8]
    M, C = B * D * H * W, heads * 32
    geo = AB.Window(B, D, H, W, heads, win, shift, cfg, device=DEV)
    qkv, dout = _rb((M, 3 * C), seed + M), _rb((M, C), seed + M + 1)
    table = (0.5 * torch.randn(geo.tbl_rows, heads, generator=torch.Generator().manual_seed(seed + 7))).to(DEV)
    return geo, qkv, dout, table


@pytest.mark.parametrize("name", list(WIN_CASES))
def test_window_attention_within_bounds(name):
    case = WIN_CASES[name]
    geo, qkv, dout, table = _win_inputs(case)
    att, *_ = _win_run(name, qkv, table, dout)
    persistent = att.negated                          # the plan's flag: the route keeps -delta (win_bwd1 writes it, win_dbias3 reads it)
    assert persistent == (WIN_ROUTES[name][0] is PERSISTENT)
    ref, pred = AB.win_case(geo, qkv.double(), table, dout.double(), persistent)
    launches = [False]
    if att.split_ok:
        launches.append(True)                         # the engine's form: dQ / dK / dV, then the bias-table gradient as its own launch
    for split in launches:
        att, out, buf, dqkv, dtab = _win_run(name, qkv, table, dout, split)
        lse, delta = _scratch(buf, geo.Bw * geo.heads, geo.N)
        sign = -1.0 if att.negated else 1.0
        got = dict(o=geo.gather(out), lse2=lse, delta=sign * delta, dq=geo.gather(dqkv, 0), dk=geo.gather(dqkv, 1), dv=geo.gather(dqkv, 2),
                   dtab=dtab)
        fails, stats = AB.check_all(got, ref, dict(pred, dtab=pred["dtab_bf16" if att.split_ok else "dtab"]))
        _assert(fails, f"window {name} N={geo.N} {'split' if split else 'fused'} bias gradient", stats)


@pytest.mark.parametrize("name", ["p245_shift", "p256", "l392", "l720_shift", "g392", "g800"])
def test_window_attention_windows_are_independent_and_runs_repeat(name):
    """perturbing q / k / v of every token of one window (shifted coordinates) leaves every other window's O and dQ / dK / dV rows bit for bit;
    two runs on the same inputs give the same O and dqkv"""
    case = WIN_CASES[name]
    geo, qkv, dout, table = _win_inputs(case, seed=3)
    _, out0, _, dq0, _ = _win_run(name, qkv, table, dout)
    _, out1, _, dq1, _ = _win_run(name, qkv, table, dout)
    assert torch.equal(out0, out1) and torch.equal(dq0, dq1), "two runs differ"
    w = min(geo.Bw - 1, geo.Bw // 2 + 1)
    rows = geo.rows[w]
    qkv2 = qkv.clone()
    qkv2[rows] = _rb((rows.numel(), qkv.shape[1]), 99)
    _, out2, _, dq2, _ = _win_run(name, qkv2, table, dout)
    other = torch.ones(geo.M, dtype=torch.bool, device=DEV)
    other[rows] = False
    assert geo.Bw > 1 and bool(other.any())
    assert torch.equal(out2[other], out0[other]), "another window's output changed"
    assert torch.equal(dq2[other], dq0[other]), "another window's dQ / dK / dV changed"
    assert not torch.equal(out2[rows], out0[rows])


# ---------------------------------------------------------------------------------------------------------------------------- sequence
SEQ_L = [50, 282, 288, 289, 300, 757, 768, 769, 800]
SEQ_ONE = ("sequence one-image", ["seq_fwd3"], ["seq_dq3", "seq_dkv3"])
SEQ_CHUNKED = ("sequence chunked", ["seql_fwd"], ["seql_dq", "seql_dkv"])
SEQ_GENERIC = ("generic sequence", ["attn_fwd_kernel"], ["attn_bwd_dq_kernel", "attn_bwd_dkv_kernel"])
SEQ_ROUTES = {50: SEQ_ONE, 282: SEQ_ONE, 288: SEQ_ONE, 289: SEQ_CHUNKED, 300: SEQ_CHUNKED, 757: SEQ_CHUNKED, 768: SEQ_CHUNKED, 769: SEQ_GENERIC,
              800: SEQ_GENERIC}


def _seq_inputs(n, L, heads, seed=0):
    Hd = heads * 64
    qkv, dout = _rb((n * L, 3 * Hd), seed + L), _rb((n * L, Hd), seed + L + 1)
    cf = L - 32                                        # 32 text rows after the prefix
    mask = torch.ones(n, L, dtype=torch.int32)
    mask[0, cf - 9:cf - 2] = 0                         # masked video keys
    mask[-1, 3:5] = 0
    return qkv, dout, mask, cf


def _seq_run(n, L, heads, qkv, dout, mask, cf=0, p=0.0, seed=0):
    Hd = heads * 64
    att = K().Attn(1, heads, 64, n_seq=n, L=L, key_mask=mask.to(DEV), dropout_p=p, seed=seed, causal_from=cf)
    assert not _assert_route(att, SEQ_ROUTES[L])       # every sequence route keeps +delta
    buf = torch.full((att.lse_elems(),), float("nan"), device=DEV)
    out = torch.empty(n * L, Hd, dtype=bf16, device=DEV)
    att.fwd(qkv, out, buf)
    dqkv = torch.empty_like(qkv)
    att.bwd(qkv, out, dout, buf, dqkv, None)
    torch.cuda.synchronize()
    return out, buf, dqkv


def _seq_check(n, L, heads, variant, seed=4242):
    from tests.helpers import attn_keep_multiplier
    qkv, dout, mask, cf = _seq_inputs(n, L, heads)
    causal = cf if "causal" in variant else 0
    p = 0.1 if "dropout" in variant else 0.0
    keep = attn_keep_multiplier(seed, n, heads, L, p) if p else None
    out, buf, dqkv = _seq_run(n, L, heads, qkv, dout, mask, causal, p, seed)
    ref, pred = AB.seq_case(qkv.double(), n, L, heads, mask, causal, keep, dout.double())
    Hd = heads * 64
    lse, delta = _scratch(buf, n * heads, L)
    got = dict(o=AB.seq_rows(out, n, L, heads), lse2=lse, delta=delta,
               dq=AB.seq_rows(dqkv[:, :Hd], n, L, heads), dk=AB.seq_rows(dqkv[:, Hd:2 * Hd], n, L, heads), dv=AB.seq_rows(dqkv[:, 2 * Hd:], n, L, heads))
    fails, stats = AB.check_all(got, ref, pred)
    _assert(fails, f"sequence n={n} L={L} heads={heads} {variant}", stats)


@pytest.mark.parametrize("L", SEQ_L)
@pytest.mark.parametrize("variant", ["mask", "causal", "dropout", "causal_dropout"])
def test_sequence_attention_within_bounds(L, variant):
    _seq_check(2, L, 1, variant)


def test_sequence_attention_many_problems_within_bounds():
    _seq_check(44, 757, 2, "mask")                   # 264 items on 256 workgroups of the chunked kernels


@pytest.mark.parametrize("L", [282, 300, 800])
def test_sequence_masked_keys_are_inert(L):
    """K and V at masked keys replaced by +-1e4: O, lse and dQ bit for bit; dK and dV rows of masked keys exactly 0"""
    n, heads = 2, 1
    Hd = heads * 64
    qkv, dout, mask, cf = _seq_inputs(n, L, heads)
    out0, buf0, dq0 = _seq_run(n, L, heads, qkv, dout, mask)
    rows = torch.nonzero(mask.reshape(-1) == 0).reshape(-1).to(DEV)
    x = qkv.clone()
    sgn = torch.where(torch.arange(Hd, device=DEV) % 2 == 0, 1e4, -1e4).to(bf16)
    x[rows, Hd:2 * Hd] = sgn
    x[rows, 2 * Hd:] = -sgn
    out1, buf1, dq1 = _seq_run(n, L, heads, x, dout, mask)
    G = n * heads
    assert torch.equal(out1, out0), "output moved with masked keys"
    assert torch.equal(_scratch(buf1, G, L)[0], _scratch(buf0, G, L)[0]), "lse moved with masked keys"
    assert torch.equal(dq1[:, :Hd], dq0[:, :Hd]), "dQ moved with masked keys"
    assert (dq1[rows, Hd:] == 0).all() and (dq0[rows, Hd:] == 0).all(), "dK / dV of masked keys are not 0"


@pytest.mark.parametrize("L", [282, 300, 800])
def test_sequence_seq2seq_block_structure(L):
    """causal_from: perturbing the text rows leaves O and dQ of the prefix rows unchanged; perturbing text key j leaves text queries < j
    unchanged (bit for bit)"""
    n, heads = 2, 1
    Hd = heads * 64
    qkv, dout, mask, cf = _seq_inputs(n, L, heads)
    out0, _, dq0 = _seq_run(n, L, heads, qkv, dout, mask, cf)
    row = lambda r: torch.cat([b * L + r for b in range(n)])
    text = row(torch.arange(cf, L, device=DEV))
    pre = row(torch.arange(0, cf, device=DEV))
    x = qkv.clone()
    x[text] = _rb((text.numel(), 3 * Hd), 5)
    out1, _, dq1 = _seq_run(n, L, heads, x, dout, mask, cf)
    assert torch.equal(out1[pre], out0[pre]) and torch.equal(dq1[pre, :Hd], dq0[pre, :Hd]), "prefix rows see the text"
    assert not torch.equal(out1[text], out0[text])
    j = cf + 17
    x = qkv.clone()
    x[row(torch.tensor([j], device=DEV)), Hd:] = _rb((n, 2 * Hd), 6)
    out2, _, dq2 = _seq_run(n, L, heads, x, dout, mask, cf)
    before = row(torch.arange(0, j, device=DEV))
    after = row(torch.arange(j, L, device=DEV))
    assert torch.equal(out2[before], out0[before]) and torch.equal(dq2[before, :Hd], dq0[before, :Hd]), "a query sees a later text key"
    assert not torch.equal(out2[after], out0[after])


# ---------------------------------------------------------------------------------------------------------------------------- decode
def _dec_run(qkv_pre, mask, ck, cv, qkv_new, B, heads, Lv, nc, q_len, max_len, beams=1):
    H = heads * 64
    d_ck, d_cv = ck.clone(), cv.clone()
    out = torch.empty(B * q_len, H, dtype=bf16, device=DEV)
    d_mask = mask.to(DEV)
    desc = K().attn_decode_desc(B, heads, q_len, Lv, nc, 1, max_len, qkv_pre, d_mask, qkv_new, d_ck, d_cv, out)
    sp = K().attention_decode_splits(desc)
    part = torch.empty(B * heads * sp * q_len * 66, device=DEV)
    desc.partials, desc.partials_capacity = part.data_ptr(), part.numel()
    (K().attention_decode_beam(desc, beams) if beams > 1 else K().attention_decode(desc))
    torch.cuda.synchronize()
    return out, sp


def _dec_check(B, t, q_len, beams=1, masked=None, heads=12, Lv=250, max_len=50):
    H = heads * 64
    clips = B // beams
    seed = B * 100 + t * 3 + q_len + beams
    qkv_pre, qkv_new = _rb((clips, Lv, 3 * H), seed), _rb((B, q_len, 3 * H), seed + 1)
    ck, cv = _rb((B, heads, max_len, 64), seed + 2), _rb((B, heads, max_len, 64), seed + 3)
    mask = torch.ones(clips, Lv, dtype=torch.int32)
    if masked is None:
        for b in range(clips):
            mask[b, (7 * b) % 40:(7 * b) % 40 + 10] = 0
    else:
        mask[:, masked] = 0
    nc = t - 1
    out, sp = _dec_run(qkv_pre, mask, ck, cv, qkv_new, B, heads, Lv, nc, q_len, max_len, beams)
    ref, pred = AB.decode_case(qkv_pre.double(), mask, ck.double(), cv.double(), qkv_new.double(), B, heads, Lv, nc, q_len, beams=beams)
    got = dict(o=out.view(B, q_len, heads, 64).transpose(1, 2).reshape(B * heads, q_len, 64))
    fails, stats = AB.check_all(got, ref, pred)
    _assert(fails, f"decode B={B} t={t} q_len={q_len} beams={beams} splits={sp}", stats)
    return qkv_pre, mask, ck, cv, qkv_new, out, sp


@pytest.mark.parametrize("B", [1, 3, 32])
@pytest.mark.parametrize("t", [1, 2, 19, 49])
@pytest.mark.parametrize("q_len", [1, 2])
def test_attention_decode_within_bounds(B, t, q_len):
    _dec_check(B, t, q_len)


@pytest.mark.parametrize("clips,nb", [(1, 5), (6, 5), (4, 8), (16, 2)])
@pytest.mark.parametrize("t", [1, 19])
def test_attention_decode_beam_within_bounds(clips, nb, t):
    _dec_check(clips * nb, t, 2, beams=nb)


def test_attention_decode_fully_masked_split_chunk():
    """B = 1: 16 splits of 16 keys; the first three chunks are all masked video keys, so their partials carry max = -inf and the combine
    skips them (decode.hip:240-245).  Replacing those keys' K / V with +-1e4 changes nothing, bit for bit."""
    B, t, q_len, heads, Lv, max_len = 1, 1, 2, 12, 250, 50
    H = heads * 64
    qkv_pre, mask, ck, cv, qkv_new, out0, sp = _dec_check(B, t, q_len, masked=slice(0, 48))
    chunk = -(-(Lv + t - 1 + q_len) // sp)
    assert sp > 1 and chunk <= 24, (sp, chunk)        # at least two whole chunks are masked
    x = qkv_pre.clone()
    x[:, :48, H:2 * H] = 1e4
    x[:, :48, 2 * H:] = -1e4
    out1, _ = _dec_run(x, mask, ck, cv, qkv_new, B, heads, Lv, t - 1, q_len, max_len)
    assert torch.equal(out1, out0)
