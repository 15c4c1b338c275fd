"""CPU: the attention bounds of tests/attention_bounds.py can fail.  "Kernel outputs" are built on the host from the float64 reference of each
path family (shapes inside the persistent window, large window, generic window, one-image sequence, chunked sequence, generic sequence and
decode ranges): with the kernels' roundings injected (the rounding model) the assertion must accept them, and with each of eleven kernel
bugs injected it must reject them."""
import pytest
import torch

from tests import attention_bounds as AB
from tests.helpers import attn_keep_multiplier

torch.set_num_threads(min(16, torch.get_num_threads()))


def _bf(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).bfloat16().double()


# ---- sequence families ------------------------------------------------------------------------------------------------------------------
SEQ = {"seq3": (2, 282, 1, 250), "seql": (1, 300, 1, 268), "seq_generic": (1, 800, 1, 768)}      # n, L, heads, causal_from (prefix keys)
SEQ_MUT = ["scale", "drop_last_key", "key_mask_shift", "delta_scale", "delta_last_tile", "dv_last_query", "causal_off_by_one", "dropout_seed"]


def _seq_inputs(fam):
    n, L, heads, cf = SEQ[fam]
    Hd = heads * 64
    qkv, dout = _bf((n * L, 3 * Hd), L), _bf((n * L, Hd), L + 1)
    mask = torch.ones(n, L, dtype=torch.int32)
    mask[0, cf - 9:cf - 2] = 0                              # masked video keys
    return n, L, heads, cf, qkv, dout, mask


def _seq_emulate(fam, variant, mut=None):
    """(failures, stats) of the assertion on the rounding model of one sequence launch, with kernel bug `mut` injected"""
    n, L, heads, cf, qkv, dout, mask = _seq_inputs(fam)
    causal = cf if "causal" in variant else 0
    seed, p = 4242, 0.1
    keep = attn_keep_multiplier(seed, n, heads, L, p) if "dropout" in variant else None
    ref, _ = AB.seq_case(qkv, n, L, heads, mask, causal, keep, dout)
    q, k, v, add, kp, do = AB.seq_problem(qkv, n, L, heads, mask, causal, keep, dout)
    scale, kw = 0.125, {}
    if mut == "scale":
        scale *= 1.01
    elif mut == "drop_last_key":
        add = add.clone()
        add[:, :, L - 1] = AB.NEG
    elif mut == "key_mask_shift":
        add = AB.seq_problem(qkv, n, L, heads, torch.roll(mask, 1, -1), causal, keep, dout)[3]
    elif mut == "causal_off_by_one":
        add = AB.seq_problem(qkv, n, L, heads, mask, causal, keep, dout, key_of=lambda j: j - 1)[3]     # query i sees key i + 1
    elif mut == "delta_scale":
        kw["delta_fn"] = lambda d: d * 0.99
    elif mut == "delta_last_tile":
        last = 32 * ((L - 1) // 32)
        kw["delta_fn"] = lambda d: torch.cat([d[:, :last], torch.zeros_like(d[:, last:])], 1)
    elif mut == "dv_last_query":
        rows = torch.ones(n * heads, L, dtype=torch.float64)
        rows[:, L - 1] = 0
        kw["dv_rows"] = rows
    elif mut == "dropout_seed":
        kw["keep_bwd"] = attn_keep_multiplier(seed + 1, n, heads, L, p).double().reshape(n * heads, L, L)
    got = AB.model(q, k, v, add, scale, kp, do, **kw)
    return AB.check_all(got, ref, AB.model(*AB.seq_problem(qkv, n, L, heads, mask, causal, keep, dout)[:4], 0.125, kp, do))


@pytest.mark.parametrize("fam", list(SEQ))
@pytest.mark.parametrize("variant", ["mask", "causal", "dropout", "causal_dropout"])
def test_sequence_rounding_model_is_accepted(fam, variant):
    fails, stats = _seq_emulate(fam, variant)
    assert not fails, fails
    assert all(er <= 1.0 for er, _ in stats.values()), stats


@pytest.mark.parametrize("fam", list(SEQ))
@pytest.mark.parametrize("mut", SEQ_MUT)
def test_sequence_mutation_is_rejected(fam, mut):
    variant = {"causal_off_by_one": "causal", "dropout_seed": "causal_dropout"}.get(mut, "mask")
    fails, _ = _seq_emulate(fam, variant, mut)
    assert fails, f"{fam}: the bound accepts the mutation {mut}"


# ---- window families --------------------------------------------------------------------------------------------------------------------
WIN = {   # B, D, H, W, heads, window, shift, configured window, persistent (bf16 bias fragments)
    "win_persistent": (2, 5, 14, 14, 2, (5, 7, 7), (0, 3, 3), (8, 7, 7), True),
    "win_large": (1, 16, 14, 14, 1, (8, 7, 7), (4, 3, 3), (8, 7, 7), False),
    "win_generic": (1, 8, 10, 20, 1, (8, 10, 10), (0, 5, 5), (8, 10, 10), False),
}
WIN_MUT = ["scale", "drop_last_key", "relpos_off_by_one", "shift_region_inverted", "delta_scale", "delta_last_tile", "dv_last_query",
           "dtab_missing_window"]


def _win_emulate(fam, mut=None):
    B, D, H, W, heads, win, shift, cfg, persistent = WIN[fam]
    geo = AB.Window(B, D, H, W, heads, win, shift, cfg)
    N, C = geo.N, geo.C
    qkv, dout = _bf((geo.M, 3 * C), N), _bf((geo.M, C), N + 1)
    table = 0.5 * torch.randn(geo.tbl_rows, heads, generator=torch.Generator().manual_seed(N + 2))
    ref, pred = AB.win_case(geo, qkv, table, dout, persistent)
    q, k, v = (geo.gather(qkv, i) for i in range(3))
    do = geo.gather(dout)
    idx, smask, scale, kw = None, None, 32 ** -0.5, {}
    if mut == "scale":
        scale *= 1.01
    elif mut == "relpos_off_by_one":
        idx = (geo.idx + 1).clamp_max(geo.tbl_rows - 1)                       # one step along the w axis of the code
    elif mut == "shift_region_inverted":
        smask = geo.smask.clone()
        w = geo.nW - 1                                                       # the last window holds every region of the shift
        a = smask[w, 0] == 0                                                 # region of slot 0
        b = smask[w, N - 1] == 0                                             # region of the last slot
        assert not bool(a[N - 1]), "the last window should hold two regions"
        smask[w][a[:, None] & b[None, :]] = 0.0                              # queries of region a see region b
    elif mut == "delta_scale":
        kw["delta_fn"] = lambda d: d * 0.99
    elif mut == "delta_last_tile":
        last = 32 * ((N - 1) // 32)
        kw["delta_fn"] = lambda d: torch.cat([d[:, :last], torch.zeros_like(d[:, last:])], 1)
    elif mut == "dv_last_query":
        rows = torch.ones(geo.Bw * heads, N, dtype=torch.float64)
        rows[:, N - 1] = 0
        kw["dv_rows"] = rows
    add, _ = geo.add(table, idx=idx, smask=smask, stored_bf16=persistent)
    if mut == "drop_last_key":
        add = add.clone()
        add[:, :, N - 1] = AB.NEG
    got = AB.model(q, k, v, add, scale, None, do, **kw)
    got["dtab"] = geo.dtab(got["ds"], idx=idx, skip_window=0 if mut == "dtab_missing_window" else None)
    return AB.check_all(got, ref, pred)


@pytest.mark.parametrize("fam", list(WIN))
def test_window_rounding_model_is_accepted(fam):
    fails, stats = _win_emulate(fam)
    assert not fails, fails
    assert all(er <= 1.0 for er, _ in stats.values()), stats


@pytest.mark.parametrize("fam", list(WIN))
@pytest.mark.parametrize("mut", WIN_MUT)
def test_window_mutation_is_rejected(fam, mut):
    fails, _ = _win_emulate(fam, mut)
    assert fails, f"{fam}: the bound accepts the mutation {mut}"


# ---- decode -----------------------------------------------------------------------------------------------------------------------------
def _dec_emulate(mut=None, beams=1):
    B, heads, Lv, nc, q_len, max_len = 3 * beams, 2, 250, 18, 2, 50
    clips = B // beams
    H = heads * 64
    qkv_pre, qkv_new = _bf((clips, Lv, 3 * H), 1), _bf((B, q_len, 3 * H), 2)
    ck, cv = _bf((B, heads, max_len, 64), 3), _bf((B, heads, max_len, 64), 4)
    mask = torch.ones(clips, Lv, dtype=torch.int32)
    mask[:, 0:48] = 0                                                        # whole split chunks of masked video keys
    args = (qkv_pre, mask, ck, cv, qkv_new, B, heads, Lv, nc, q_len)
    ref, pred = AB.decode_case(*args, beams=beams)
    q, k, v, add = AB.decode_problem(*args, beams=beams)
    scale = 0.125
    if mut == "scale":
        scale *= 1.01
    elif mut == "drop_last_key":
        add = add.clone()
        add[:, :, -1] = AB.NEG
    elif mut == "key_mask_shift":
        add = AB.decode_problem(qkv_pre, torch.roll(mask, 1, -1), *args[2:], beams=beams)[3]
    got = AB.model(q, k, v, add, scale, p_bf16=False)
    return AB.check_all(got, ref, pred)


@pytest.mark.parametrize("beams", [1, 4])
def test_decode_rounding_model_is_accepted(beams):
    fails, stats = _dec_emulate(beams=beams)
    assert not fails, fails


@pytest.mark.parametrize("mut", ["scale", "drop_last_key", "key_mask_shift"])
def test_decode_mutation_is_rejected(mut):
    fails, _ = _dec_emulate(mut)
    assert fails, f"decode: the bound accepts the mutation {mut}"
