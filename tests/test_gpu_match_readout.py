"""lav_match_readout (lavender_amd/csrc/qa.hip) against the numpy restatement of its rule (tests/match_readout_ref.py): exact integer equality of
choice / hit and bit equality of score, over group sizes on both sides of the 64-lane wave, group counts up to more than a grid dimension holds,
both dtypes, the (n, 2) block without a row map and a padded vocabulary-wide block read through a scrambled row map, planted ties / NaN / +-0 /
zero-denominator groups, gt = -1, an out-of-range row entry, and every rejected argument.  The padding columns hold NaN: a kernel that read one
would answer with it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import match_readout_ref as MR
from tests.qa_answer_ref import bf16_round

pytestmark = pytest.mark.gpu

OS = (1, 2, 63, 64, 65, 130)
GS = (1, 3, 70000)
DTYPES = [torch.float32, torch.bfloat16]


def _values(rng, shape, dtype):
    x = (rng.standard_normal(shape) * 4).astype(np.float32)
    return bf16_round(x) if dtype == torch.bfloat16 else x


def _run(x, G, O, tc, fc, dtype, row=None, gt=None, width=None):
    """x (n_rows, width) float32 of values exact in dtype -> the kernel's (score, choice, hit) as numpy, from a NaN-padded device buffer"""
    from lavender_amd import hip as K
    n_rows, w = x.shape
    ld = w if width is None else width
    buf = torch.full((n_rows, ld), float("nan"), dtype=torch.float32)
    buf[:, :w] = torch.from_numpy(x)
    view = buf.to(dtype).cuda()[:, :w]
    out = torch.full((2, G), -7, dtype=torch.int32, device="cuda")
    choice, hit, score = K.match_readout(view, G, O, tc, fc, row=row, gt=gt, want_score=True, out=out)
    return score.cpu().numpy(), choice.cpu().numpy(), None if hit is None else hit.cpu().numpy()


def _same(got, want, what):
    s, c, h = got
    rs, rc, rh = want
    assert (c == rc).all(), (what, "choice", np.nonzero(c != rc)[0][:5], c[c != rc][:5], rc[c != rc][:5])
    assert (s.view(np.uint32) == rs.view(np.uint32)).all(), (what, "score", np.nonzero(s.view(np.uint32) != rs.view(np.uint32))[0][:5])
    if rh is not None:
        assert (h == rh).all(), (what, "hit")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("G", GS)
def test_pair_block_without_a_row_map(G, dtype):
    """the (n, 2) block of lav_mlm_pair_readout: ld = 2, columns 0 / 1, row = NULL"""
    for O in OS:
        rng = np.random.default_rng(100 * O + G % 97)
        x = _values(rng, (G * O, 2), dtype)
        gt = rng.integers(-1, O + 1, size=G)                   # -1 and O: outside [0, O), never a hit
        _same(_run(x, G, O, 0, 1, dtype, gt=gt), MR.match_ref(x, G, O, 0, 1, gt=gt), (G, O))
        few = rng.choice(np.array([-1.0, 0.0, -0.0, 0.5, 2.0], dtype=np.float32), size=(G * O, 2))   # ties, zero denominators, NaN quotients
        _same(_run(few, G, O, 1, 0, dtype, gt=gt), MR.match_ref(few, G, O, 1, 0, gt=gt), (G, O, "few"))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("G", GS)
def test_wide_block_through_a_scrambled_row_map(G, dtype):
    """the reference's formulation: (pairs * X, ld) logits with padding columns, row[k] = the [MASK] row of pair k, in scrambled order"""
    V, ld, tc, fc = 33, 40, 29, 6
    for O in ((2, 65) if G > 1000 else OS):
        rng = np.random.default_rng(7 * O + G % 89)
        n_rows = min(G * O, 4096) + 5
        x = _values(rng, (n_rows, V), dtype)
        row = rng.integers(0, n_rows, size=G * O)
        row[:min(n_rows, G * O)] = rng.permutation(n_rows)[:min(n_rows, G * O)]
        gt = rng.integers(0, O, size=G)
        _same(_run(x, G, O, tc, fc, dtype, row=row, gt=gt, width=ld), MR.match_ref(x, G, O, tc, fc, row=row, gt=gt), (G, O))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_vocabulary_wide_rows(dtype):
    V, ld, X, G, O = 30522, 30528, 3, 3, 5
    rng = np.random.default_rng(3)
    x = _values(rng, (G * O * X, V), dtype)
    row = np.arange(G * O) * X + rng.integers(0, X, size=G * O)
    gt = rng.integers(0, O, size=G)
    _same(_run(x, G, O, 2995, 6270, dtype, row=row, gt=gt, width=ld), MR.match_ref(x, G, O, 2995, 6270, row=row, gt=gt), "vocab")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_planted_groups(dtype):
    O = 130
    base = np.tile(np.array([[1.0, 3.0]], dtype=np.float32), (O, 1))          # s = 0.25 everywhere

    def grp(edit):
        g = base.copy()
        edit(g)
        return g

    def tie(g): g[[63, 64, 129]] = [3.0, 1.0]                                  # s = 0.75 at 63, 64 (across the lane boundary) and 129 -> 63
    def tie_hi(g): g[[64, 128]] = [3.0, 1.0]                                   # the same lane (0) meets both -> 64
    def nans(g): g[70] = [np.nan, 1.0]; g[5] = [1.0, -1.0]; g[6] = [0.0, 0.0]  # 1/0 = +inf at 5 is a number; NaN quotients at 6 (0/0) and 70 -> 6
    def zeros(g): g[:] = [-1.0, -3.0]; g[100] = [-0.0, 1.0]; g[3] = [0.0, 1.0]; g[90] = [0.0, 2.0]   # s = 0.25 everywhere but -0, +0, +0: the 0.25 at 0 wins
    def zeros2(g): g[:] = [1.0, -3.0]; g[100] = [-0.0, 1.0]; g[3] = [0.0, 1.0]  # s = -0.5 but -0 at 100 and +0 at 3: one value -> 3
    def zeros3(g): g[:] = [1.0, -3.0]; g[3] = [-0.0, 1.0]; g[100] = [0.0, 1.0]  # the other way round -> 3 again
    def zden(g): g[:] = [1.0, -3.0]; g[77] = [2.0, -2.0]; g[78] = [-2.0, 2.0]   # +inf at 77, -inf at 78 -> 77
    def infs(g): g[:] = [-2.0, 2.0]                                             # every quotient -inf -> 0

    groups = [grp(e) for e in (tie, tie_hi, nans, zeros, zeros2, zeros3, zden, infs)]
    want = [63, 64, 6, 0, 3, 3, 77, 0]
    x = np.concatenate(groups)
    G = len(groups)
    gt = np.array(want)
    gt[1] = -1                                                                  # no ground truth: no hit
    got = _run(x, G, O, 0, 1, dtype, gt=gt)
    _same(got, MR.match_ref(x, G, O, 0, 1, gt=gt), "planted")
    assert got[1].tolist() == want and got[2].tolist() == [1, 0, 1, 1, 1, 1, 1, 1]


def test_out_of_range_row_entry_is_not_read_and_never_wins():
    from lavender_amd import hip as K
    O, G = 66, 3
    rng = np.random.default_rng(11)
    x = _values(rng, (G * O, 2), torch.float32)
    x[O + 2] = [0.0, 0.0]                                       # group 1: a NaN quotient at o = 2
    x[2 * O:3 * O] = [-2.0, 2.0]                                # group 2: every read candidate scores -inf
    row = np.arange(G * O)
    row[[1, 65, O + 0, 2 * O + 0]] = [-1, G * O, G * O + 1000, -5]
    want = MR.match_ref(x, G, O, 0, 1, row=row)
    assert want[1][1] == 2 and want[1][2] == 1                  # the NaN quotient beats the unread candidate 0; so does -inf
    view = torch.from_numpy(x).cuda()
    with pytest.raises(ValueError):                             # a host array is checked by the wrapper
        K.match_readout(view, G, O, 0, 1, row=row)
    choice, _, score = K.match_readout(view, G, O, 0, 1, row=torch.from_numpy(row.astype(np.int32)).cuda(), want_score=True)
    _same((score.cpu().numpy(), choice.cpu().numpy(), None), want, "row outside")
    allout = torch.full((O,), -1, dtype=torch.int32, device="cuda")           # nothing read at all: the lowest o
    assert K.match_readout(view, 1, O, 0, 1, row=allout)[0].item() == 0


def test_rejected_arguments_launch_nothing():
    from lavender_amd import _lib as L
    from lavender_amd import hip as K
    G, O, ld = 3, 4, 8
    x = torch.randn(G * O, ld, device="cuda")
    row = torch.arange(G * O, dtype=torch.int32, device="cuda")
    gt = torch.zeros(G, dtype=torch.int32, device="cuda")
    out = torch.full((2, G), -7, dtype=torch.int32, device="cuda")
    score = torch.full((G * O,), -7.0, device="cuda")

    def call(G=G, O=O, ld=ld, dtype=1, row=row, n_rows=G * O, tc=0, fc=1, gt=gt):
        return L.lib.lav_match_readout(K._s(), G, O, K._p(x), ld, dtype, K._p(row), n_rows, tc, fc, K._p(gt), K._p(score), K._p(out[0]), K._p(out[1]))
    assert call(G=0) == -1 and call(O=0) == -1 and call(G=-1) == -1
    assert call(tc=ld) == -1 and call(fc=-1) == -1 and call(tc=-1) == -1 and call(fc=ld) == -1
    assert call(dtype=2) == -1 and call(dtype=-1) == -1
    assert call(row=None, n_rows=G * O - 1) == -1
    assert b"lav_match_readout" in L.lib.lav_last_error()
    assert call(gt=None) == -1                                 # hit without gt
    torch.cuda.synchronize()
    assert (out.cpu() == -7).all() and (score.cpu() == -7).all()
    assert call(row=None) == 0                                 # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert (out.cpu() != -7).all() and (score.cpu() != -7).all()
    with pytest.raises(ValueError):
        K.match_readout(x, G, O, 0, ld)
