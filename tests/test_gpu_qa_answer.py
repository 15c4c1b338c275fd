"""lav_answer_readout (lavender_amd/csrc/qa.hip) against the numpy restatement of its rules (tests/qa_answer_ref.py): exact integer equality of
pred / rank / choice over row counts, widths (the real vocabulary with its padded row stride included), both dtypes, every label kind and
candidate count, the planted tie / boundary / NaN rows, rows drawn from few distinct values, views that start off a 16-byte boundary, and every
case at split counts 1 and the largest (the outputs must not depend on the split).  The padding columns of every buffer hold NaN: a kernel that
read one would answer with it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import qa_answer_ref as QR

pytestmark = pytest.mark.gpu

SHAPES = [(30522, 30528), (257, 264), (8, 8)]
SPLITS = (1, 16)                                   # 16 = LAV_ANSWER_MAX_SPLITS


def _device_rows(x, ld, dtype, col0=0):
    """x (n, V) float32 of values exactly representable in dtype -> a (n, V) device view of a NaN-filled (n, ld) buffer starting at column col0"""
    n, V = x.shape
    buf = torch.full((n, ld), float("nan"), dtype=torch.float32)
    buf[:, col0:col0 + V] = torch.from_numpy(x)
    return buf.to(dtype).cuda()[:, col0:col0 + V]


def _check(x, ld, dtype, labels, cand, col0=0):
    from lavender_amd import hip as K
    view = _device_rows(x, ld, dtype, col0)
    ref = QR.answer_ref(x, labels, cand)
    outs = []
    for s in SPLITS:
        out = torch.full((3, x.shape[0]), -7, dtype=torch.int32, device="cuda")
        K.answer_readout(view, x.shape[1], np.asarray(labels, dtype=np.int32), cand, splits=s, out=out)
        outs.append(out.cpu().numpy())
        for name, got, want in zip(("pred", "rank", "choice"), outs[-1], ref):
            assert (got == want).all(), (name, s, np.nonzero(got != want)[0][:5], got[got != want][:5], want[got != want][:5])
    assert (outs[0] == outs[1]).all()


def _values(rng, n, V, dtype, few=False):
    if few:
        x = rng.choice(np.array([-1.0, 0.0, 0.5, 2.0], dtype=np.float32), size=(n, V))
    else:
        x = (rng.standard_normal((n, V)) * 4).astype(np.float32)
    return QR.bf16_round(x) if dtype == torch.bfloat16 else x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,ld", SHAPES)
@pytest.mark.parametrize("n", [1, 5, 33])
def test_answer_readout_matches_the_reference(n, V, ld, dtype):
    rng = np.random.default_rng(1000 * n + V)
    x = _values(rng, n, V, dtype)
    few = _values(rng, n, V, torch.bfloat16, few=True)       # ties everywhere (exact in both dtypes)
    for n_cand in (0, 1, 5, 32):
        cand = rng.integers(0, V, size=n_cand).tolist()
        for lab in (0, V - 1, -1):
            _check(x, ld, dtype, np.full(n, lab), cand)
        mixed = rng.integers(-1, V, size=n)
        _check(x, ld, dtype, mixed, cand)
        _check(few, ld, dtype, mixed, cand)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_answer_readout_planted_rows(V, ld, dtype):
    x, labels, _ = QR.planted_rows(V, np.random.default_rng(5), bf16=dtype == torch.bfloat16)
    cand = [0, V - 1, V // 2, 3, 1]
    _check(x, ld, dtype, labels, cand)
    # candidate sums of either sign, at least 1.0 from zero
    y = np.zeros((4, V), dtype=np.float32)
    cc = [5, 1, 6]
    y[0, cc] = [1.0, 3.0, 2.0]; y[1, cc] = [-1.0, -3.0, -2.5]; y[2, cc] = [2.0, -4.0, 0.5]; y[3, cc] = [2.0, 2.0, -3.0]
    _check(y, ld, dtype, np.full(4, -1), cc)
    from lavender_amd import hip as K
    got = K.answer_readout(_device_rows(y, ld, dtype), V, np.full(4, -1, dtype=np.int32), cc)[2].cpu().tolist()
    assert got == [1, 1, 1, 0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("col0", [1, 3])
def test_answer_readout_rows_off_the_16_byte_boundary(dtype, col0):
    """a view that starts col0 columns into its buffer with an odd row stride: every row has another scalar head and tail"""
    rng = np.random.default_rng(col0)
    V, ld, n = 1031, 1031 + 7, 5
    x = _values(rng, n, V, dtype)
    _check(x, ld, dtype, rng.integers(-1, V, size=n), rng.integers(0, V, size=5).tolist(), col0=col0)


def test_answer_readout_rejects_bad_arguments_without_a_launch():
    from lavender_amd import _lib as L
    from lavender_amd import hip as K
    n, V, ld = 3, 40, 48
    x = torch.randn(n, ld, device="cuda")
    lab = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.full((3, n), -7, dtype=torch.int32, device="cuda")
    i32s = lambda v: np.asarray(v, dtype=np.int32)

    def call(V=V, ld=ld, dtype=1, lab_host=None, cand=(), n_cand=None, splits=1, ws=None, ws_bytes=0):
        c = i32s(list(cand))
        return L.lib.lav_answer_readout(K._s(), n, V, K._p(x), ld, dtype, K._p(lab), None if lab_host is None else i32s(lab_host).ctypes.data_as(C.c_void_p),
                                        c.ctypes.data_as(C.c_void_p) if c.size else None, len(c) if n_cand is None else n_cand, splits,
                                        ws, ws_bytes, K._p(out[0]), K._p(out[1]), K._p(out[2]))
    assert call(ld=V - 1) == -1                                # ld < V
    assert call(cand=list(range(33))) == -1                    # more than 32 candidates
    assert call(cand=[0, V]) == -1 and call(cand=[-1]) == -1   # candidate outside [0, V)
    assert call(lab_host=[0, V, 1]) == -1 and call(lab_host=[0, -2, 1]) == -1     # label outside [0, V) other than -1
    assert call(dtype=2) == -1 and call(splits=0) == -1 and call(splits=17) == -1
    assert call(n_cand=2) == -1                                # candidates announced, no array
    assert call(splits=4) == -4                                # a split needs the caller's workspace
    assert b"workspace" in L.lib.lav_last_error()
    torch.cuda.synchronize()
    assert (out.cpu() == -7).all()                             # nothing ran
    assert L.lib.lav_answer_readout_workspace_bytes(n, 4) == n * 4 * 12 and L.lib.lav_answer_readout_workspace_bytes(n, 1) == 0
    assert call(lab_host=[0, -1, V - 1], cand=[1, 2]) == 0     # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert (out.cpu() != -7).all()
    with pytest.raises(L.LavenderHipError):
        K.answer_readout(x[:, :V], V, np.array([0, V, 0], dtype=np.int32))
