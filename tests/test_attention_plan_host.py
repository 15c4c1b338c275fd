"""CPU: the attention route plan (attn_plan in attention.hip) read through lav_attention_plan, no device: one descriptor on each side of every
route threshold, the attention shapes of the bench models (cfg2 / cfg4 / cfg5), the bias-split flag against lav_attention_bias_split with the
launch limits of every planned launch, and the error codes of invalid descriptors against the entries themselves (they return before any launch).

Pointers of a descriptor are only tested for presence, so the tables are a dummy address."""
import ctypes as C
import random

import pytest

FWD, BWD, BWD_BIAS, BIAS = 0, 1, 2, 3
_PTR = 0x1000
LDS_CU = 160 * 1024


def _lib():
    from lavender_amd import _lib
    return _lib


def win_desc(B, D, H, W, heads, win, shift=(0, 0, 0), cfg=None, tables=False, hm=0, head_dim=32):
    cfg = cfg or win
    d = _lib().AttnDesc()
    d.mode, d.heads, d.head_dim, d.scale = 0, heads, head_dim, head_dim ** -0.5
    d.B, d.D, d.H, d.W = B, D, H, W
    (d.wd, d.wh, d.ww), (d.sd, d.sh, d.sw), (d.cfg_wd, d.cfg_wh, d.cfg_ww) = win, shift, cfg
    d.bias_table = _PTR
    if tables:
        d.tok_table = d.win_type = d.type_region = d.comb = d.combT = _PTR
        d.n_types = 1
    d.qkv_headmajor = hm
    return d


def seq_desc(n, L, heads, causal_from=0, p=0.0, head_dim=64):
    d = _lib().AttnDesc()
    d.mode, d.heads, d.head_dim, d.scale = 1, heads, head_dim, head_dim ** -0.5
    d.n_seq, d.L, d.causal_from, d.dropout_p, d.seed = n, L, causal_from, p, 1
    return d


def plan(d, which):
    """the launches of one pass as dicts, or the (negative) error code"""
    out = (_lib().AttnLaunchInfo * 4)()
    n = _lib().lib.lav_attention_plan(C.byref(d), which, out, 4)
    if n < 0:
        return n
    assert 1 <= n <= 3
    return [dict(kernel=o.kernel.decode(), route=o.route.decode(), grid=(o.grid_x, o.grid_y), block=o.block, lds=o.lds_bytes, split=o.split,
                 neg=o.delta_negated) for o in out[:n]]


def kernels(d, which):
    p = plan(d, which)
    return p if isinstance(p, int) else [l["kernel"] for l in p]


def routes(d):
    got = set()
    for which in (FWD, BWD, BWD_BIAS):
        got |= {l["route"] for l in plan(d, which)}
    assert len(got) == 1, got
    return got.pop()


class winl_select:
    def __init__(self, parts):
        self.parts = parts

    def __enter__(self):
        self.old = _lib().lib.lav_winl_select(self.parts)

    def __exit__(self, *exc):
        _lib().lib.lav_winl_select(self.old)


PERSISTENT = dict(fwd=["win_fwd3"], bwd=["win_bwd1"], bwd_bias=["win_bwd1", "win_dbias3"], bias=["win_dbias3"])
LARGE = dict(fwd=["winl_fwd"], bwd=["winl_dq", "winl_dkv"], bwd_bias=["winl_dq", "winl_dkv", "winl_dbias"], bias=["winl_dbias"])
GENERIC = dict(fwd=["attn_fwd_kernel"], bwd=["attn_bwd_dq_kernel", "attn_bwd_dkv_kernel"], bwd_bias=["attn_bwd_dq_kernel", "attn_bwd_dkv_kernel"], bias=-1)
SEQ_ONE = dict(fwd=["seq_fwd3"], bwd=["seq_dq3", "seq_dkv3"], bwd_bias=["seq_dq3", "seq_dkv3"], bias=-1)
SEQ_CHUNKED = dict(fwd=["seql_fwd"], bwd=["seql_dq", "seql_dkv"], bwd_bias=["seql_dq", "seql_dkv"], bias=-1)


def _expect(d, route, family, what):
    assert routes(d) == route, what
    got = dict(fwd=kernels(d, FWD), bwd=kernels(d, BWD), bwd_bias=kernels(d, BWD_BIAS), bias=kernels(d, BIAS))
    assert got == family, f"{what}: {got}"
    neg = {l["neg"] for which in (FWD, BWD, BWD_BIAS) for l in plan(d, which)}
    assert neg == {1 if route == "window persistent" else 0}, what        # -delta: win_bwd1 writes it, win_dbias3 reads it; every other route +delta


# ---- thresholds ----------------------------------------------------------------------------------------------------------------------------
def test_window_token_thresholds():
    _expect(win_desc(2, 4, 8, 8, 2, (4, 8, 8), tables=True), "window persistent", PERSISTENT, "256 tokens with the tables")
    _expect(win_desc(2, 4, 8, 8, 2, (4, 8, 8)), "window large", LARGE, "256 tokens without the tables")
    _expect(win_desc(2, 1, 7, 7, 2, (1, 7, 7), cfg=(8, 7, 7)), "window large", LARGE, "49 tokens without the tables")
    _expect(win_desc(2, 1, 1, 257, 1, (1, 1, 257)), "window large", LARGE, "257 tokens")
    assert plan(win_desc(2, 1, 1, 257, 1, (1, 1, 257), tables=True), FWD) == -1          # the tables hold 256 slots
    _expect(win_desc(1, 3, 16, 16, 1, (3, 16, 16)), "window large", LARGE, "768 tokens")
    _expect(win_desc(1, 1, 1, 769, 1, (1, 1, 769)), "generic window", GENERIC, "769 tokens")
    nt = {N: plan(win_desc(1, 1, 1, N, 1, (1, 1, N), tables=True), FWD)[0]["grid"] for N in (32, 33, 256)}
    assert nt[32] == nt[33] == nt[256], "the NT template fan-out must not change the grid"


def test_reachable_table_rows_never_leave_the_table():
    """attn_plan keeps the parent's guard on the reachable bias-table rows [t.lo, t.lo + t.n) of a large window.  For a descriptor that attn_setup
    accepts it cannot fire: window <= configured window per axis, so the last slot's code mc (decoded with the configured extents, monotone in
    the slot index) is at most tbl_const, the code of the configured window's last slot; hence t.lo = tbl_const - mc >= 0 and
    t.lo + t.n = tbl_const + mc + 1 <= 2 tbl_const + 1 = tbl_rows.  So no descriptor exists on the far side of it: what can be held is that every
    window of at most 768 tokens without the tables plans to the large-window kernels, whatever its clamping."""
    rng = random.Random(5)
    seen = 0
    while seen < 300:
        cfg = (rng.randint(1, 8), rng.randint(1, 16), rng.randint(1, 16))
        win = tuple(rng.randint(1, c) for c in cfg)
        if win[0] * win[1] * win[2] > 768:
            continue
        seen += 1
        d = win_desc(1, win[0], 2 * win[1], win[2], 2, win, cfg=cfg)
        lds = max(l["lds"] for which in (FWD, BWD_BIAS) for l in plan(d, which))
        assert routes(d) == "window large" and lds <= LDS_CU, (win, cfg)


def test_four_gigabyte_guards():
    # window, row-major operand: B * tokens * 3 C * 2 bytes against 4e9 (32-bit DMA offsets); 288-token windows, C = 128
    below, above = win_desc(18084, 2, 12, 12, 4, (2, 12, 12)), win_desc(18085, 2, 12, 12, 4, (2, 12, 12))
    assert 18084 * 288 * 768 < 4e9 <= 18085 * 288 * 768
    _expect(below, "window large", LARGE, "qkv below 4e9 bytes")
    _expect(above, "generic window", GENERIC, "qkv of 4e9 bytes and more")
    # window, head-major operand with the tables: 6 heads head_dim rows bytes against 2^32 -- an error, not another route
    assert 456522 * 49 * 192 < 2 ** 32 <= 456523 * 49 * 192
    _expect(win_desc(456522, 1, 7, 7, 1, (1, 7, 7), tables=True, hm=1), "window persistent", PERSISTENT, "head-major qkv below 4 GiB")
    assert [plan(win_desc(456523, 1, 7, 7, 1, (1, 7, 7), tables=True, hm=1), which) for which in range(4)] == [-1] * 4
    # sequence, 288 < L <= 768: n L 3 C 2 bytes against 4e9; no guard at L <= 288 (offsets are per problem)
    assert 1146 * 757 * 4608 < 4e9 <= 1147 * 757 * 4608
    _expect(seq_desc(1146, 757, 12), "sequence chunked", SEQ_CHUNKED, "qkv below 4e9 bytes")
    _expect(seq_desc(1147, 757, 12), "generic sequence", GENERIC, "qkv of 4e9 bytes and more")
    assert 4000 * 282 * 4608 > 4e9
    _expect(seq_desc(4000, 282, 12), "sequence one-image", SEQ_ONE, "one-image sequences have no size guard")


def test_large_window_query_parts():
    few, many = win_desc(1023, 2, 12, 12, 1, (2, 12, 12)), win_desc(256, 2, 12, 12, 4, (2, 12, 12))      # problems x heads = 1023 / 1024
    for d, parts in ((few, 3), (many, 1)):
        for which in (FWD, BWD):
            assert [l["split"] for l in plan(d, which)] == [parts] * (1 + which), (parts, which)
            assert all(l["grid"] == (256, 1) for l in plan(d, which))
    small = win_desc(1, 4, 24, 24, 1, (2, 12, 12))            # 8 problems: 24 items at 3 parts, 8 at 1
    assert plan(small, FWD)[0]["grid"] == (24, 1)
    for parts, want in ((1, 1), (3, 3), (0, 3)):
        with winl_select(parts):
            assert [(l["kernel"], l["split"], l["grid"]) for l in plan(small, BWD)] == [(k, want, (8 * want, 1)) for k in ("winl_dq", "winl_dkv")]
            assert plan(few, FWD)[0]["split"] == (parts or 3) and plan(many, FWD)[0]["split"] == (parts or 1)
    with winl_select(-1):
        _expect(small, "generic window", GENERIC, "lav_winl_select(-1)")
        assert _lib().lib.lav_attention_bias_split(C.byref(small)) == 0
        _expect(win_desc(2, 4, 8, 8, 2, (4, 8, 8), tables=True), "window persistent", PERSISTENT, "lav_winl_select(-1) leaves the persistent route")
    _expect(small, "window large", LARGE, "lav_winl_select restored")


@pytest.mark.parametrize("L,route,family", [(288, "sequence one-image", SEQ_ONE), (289, "sequence chunked", SEQ_CHUNKED),
                                            (768, "sequence chunked", SEQ_CHUNKED), (769, "generic sequence", GENERIC)])
def test_sequence_row_thresholds(L, route, family):
    base = None
    for cf in (0, L - 32):
        for p in (0.0, 0.1):
            d = seq_desc(3, L, 2, cf, p)
            _expect(d, route, family, f"L={L} causal_from={cf} p={p}")
            got = [plan(d, which) for which in (FWD, BWD)]
            base = base or got
            assert got == base, "the CAUSAL x DROP template fan-out must not change route, grid, block or LDS"
    blocks = {l["block"] for l in plan(seq_desc(3, L, 2), BWD)}
    assert blocks == {256 if route != "sequence chunked" else 512}
    if route == "sequence chunked":
        assert plan(seq_desc(3, L, 2), FWD)[0]["split"] == (-(-L // 32) + 7) // 8       # 8-tile parts


# ---- the bench models ----------------------------------------------------------------------------------------------------------------------
def _swin_stages(B, S, heads, cfg):
    """(descriptor, tables) of both blocks of every stage: 5 frames, S / 4 tokens per side halving per stage, window clamped to the grid
    (video_swin.get_window_size), tables built by hip.Attn for windows of at most 256 tokens"""
    from lavender_amd.video_swin import get_window_size
    for s, h in enumerate(heads):
        grid = (5, S // 4 >> s, S // 4 >> s)
        win, shift = get_window_size(grid, cfg, tuple(c // 2 for c in cfg))
        for sh in ((0, 0, 0), shift):
            yield win_desc(B, *grid, h, win, sh, cfg, tables=win[0] * win[1] * win[2] <= 256), win


def test_bench_models_plan_to_the_kernels_of_the_design():
    from lavender_amd.video_swin import SWIN_SIZES
    base, large = SWIN_SIZES["base"], SWIN_SIZES["large"]
    for name, B, n_seq, L in (("cfg2", 32, 32, 282), ("cfg5", 8, 64, 276)):       # Swin-B 224^2: 245-token windows; fusion L = 250 + 32 / 26
        for d, win in _swin_stages(B, 224, base["num_heads"], base["window_size"]):
            assert win == (5, 7, 7)
            _expect(d, "window persistent", PERSISTENT, f"{name} window {win}")
            d.qkv_headmajor = 1                               # the engine's operand layout for these windows
            _expect(d, "window persistent", PERSISTENT, f"{name} window {win} head-major")
        _expect(seq_desc(n_seq, L, 12, 0, 0.1), "sequence one-image", SEQ_ONE, f"{name} fusion L={L}")
    for d, win in _swin_stages(8, 384, large["num_heads"], large["window_size"]):  # cfg4, Swin-L 384^2: 720-token windows, L = 725 + 32
        assert win == (5, 12, 12)
        _expect(d, "window large", LARGE, f"cfg4 window {win}")
    _expect(seq_desc(8, 757, 12, 0, 0.1), "sequence chunked", SEQ_CHUNKED, "cfg4 fusion L=757")


# ---- bias split and launch limits ----------------------------------------------------------------------------------------------------------
def _random_desc(rng):
    if rng.random() < 0.35:
        L = rng.choice([1, 31, 32, 50, 282, 288, 289, 300, 757, 768, 769, 800, 1500])
        return seq_desc(rng.randint(1, 70), L, rng.choice([1, 2, 12]), rng.choice([0, min(5, L)]), rng.choice([0.0, 0.1]))
    # configured windows up to (8, 12, 12): the bias tables of every Swin size (7935 rows at most)
    cfg = (rng.randint(1, 8), rng.randint(1, 12), rng.randint(1, 12))
    win = tuple(rng.randint(1, c) for c in cfg)
    if rng.random() < 0.15:
        cfg = win = (rng.randint(6, 8), 12, 12)              # more than 768 tokens: the generic kernels
    mult = (rng.randint(1, 2), rng.randint(1, 3), rng.randint(1, 3))
    shift = tuple(rng.randint(0, w - 1) for w in win)
    N = win[0] * win[1] * win[2]
    return win_desc(rng.choice([1, 2, 8, 300]), *(w * m for w, m in zip(win, mult)), rng.choice([1, 3, 4]), win, shift, cfg,
                    tables=N <= 256 and rng.random() < 0.6)


def test_bias_split_is_the_plans_flag_and_launches_fit_the_machine():
    rng = random.Random(11)
    split_seen = set()
    for _ in range(600):
        d = _random_desc(rng)
        bias = plan(d, BIAS)
        flag = _lib().lib.lav_attention_bias_split(C.byref(d))
        assert flag == (0 if bias == -1 else 1)
        split_seen.add((flag, routes(d)))
        n_bwd, n_bwd_bias = len(plan(d, BWD)), len(plan(d, BWD_BIAS))
        assert n_bwd_bias == n_bwd + flag                    # the split routes append their bias launch; the others fold it into the dQ kernel
        for which in (FWD, BWD, BWD_BIAS) + ((BIAS,) if flag else ()):
            for l in plan(d, which):
                assert l["block"] in (256, 512) and l["block"] <= 1024 and l["grid"][0] >= 1 and l["grid"][1] >= 1 and l["lds"] <= LDS_CU, (which, l)
    assert split_seen == {(1, "window persistent"), (1, "window large"), (0, "generic window"), (0, "sequence one-image"),
                          (0, "sequence chunked"), (0, "generic sequence")}


# ---- error codes ---------------------------------------------------------------------------------------------------------------------------
def _entries(d):
    """the entries' own return codes for a descriptor they refuse (they return before any launch; operands are a dummy address)"""
    lib, p = _lib().lib, C.c_void_p(_PTR)
    return [lib.lav_attention_fwd(None, C.byref(d), p, p, p), lib.lav_attention_bwd(None, C.byref(d), p, p, p, p, p, None),
            lib.lav_attention_bwd(None, C.byref(d), p, p, p, p, p, p), lib.lav_attention_bwd_bias(None, C.byref(d), p, p, p, p)]


@pytest.mark.parametrize("what,d", [
    ("window head_dim", lambda: win_desc(2, 4, 8, 8, 2, (4, 8, 8), head_dim=64)),
    ("sequence head_dim", lambda: seq_desc(2, 282, 2, head_dim=32)),
    ("bad shift", lambda: win_desc(2, 4, 8, 8, 2, (4, 8, 8), shift=(0, 8, 0))),
    ("negative shift", lambda: win_desc(2, 4, 8, 8, 2, (4, 8, 8), shift=(0, -1, 0))),
    ("qkv_headmajor without the tables", lambda: win_desc(2, 4, 8, 8, 2, (4, 8, 8), hm=1)),
    ("qkv_headmajor in sequence mode", lambda: (lambda s: (setattr(s, "qkv_headmajor", 1), s)[1])(seq_desc(2, 282, 2))),
    ("tables for more than 256 tokens", lambda: win_desc(1, 3, 16, 16, 1, (3, 16, 16), tables=True)),
])
def test_invalid_descriptors_return_the_entries_error_code(what, d):
    d = d()
    got = [plan(d, which) for which in range(4)]
    assert got == _entries(d) == [-1] * 4, what


def test_bias_alone_is_refused_where_the_entry_refuses_it():
    for d in (win_desc(1, 1, 1, 769, 1, (1, 1, 769)), seq_desc(2, 282, 2)):
        p = C.c_void_p(_PTR)
        assert plan(d, BIAS) == _lib().lib.lav_attention_bwd_bias(None, C.byref(d), p, p, p, p) == -1
    assert plan(seq_desc(2, 282, 2), 4) == -1 and plan(seq_desc(2, 282, 2), -1) == -1
