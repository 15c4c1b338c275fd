"""The three output rules of lav_answer_readout (include/lavender_hip.h) restated with numpy, and the planted rows both the host and the GPU test
use.  The inputs are the STORED values (fp32, or bf16 widened exactly), compared in float64, so the integer outputs are exact.

Order of the columns of a row: value descending, a NaN above every number (torch.topk / torch.argmax), the lower index first among equal values
and among NaNs.
  pred    the first column in that order
  rank    #{c : x_c sorts before x_t} for the label t, -1 where t == -1; a top-k hit is 0 <= rank < k
  choice  arg-max over the candidates of x_cand[c] / sum_c x_cand[c] (main_qamc_mlm.py:159-166); the rule fixes fp32 for the sum (in candidate
          order) and for the quotients, so those two steps are float32 here as well; first index wins, NaN above every number; -1 without
          candidates"""
import numpy as np


def bf16_round(a):
    """float32 array -> the nearest bf16 values (round to nearest even), as float32"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = np.isnan(a)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = (u & 0xFFFFFFFF).astype(np.uint32).view(np.float32).copy()
    out[nan] = np.nan
    return out


def _first_in_order(v):
    """index of the first element of v in the order above"""
    nan = np.isnan(v)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(v))                                # numpy returns the first occurrence of the maximum


def before(row, t):
    """boolean mask of the columns that sort before column t"""
    x = np.asarray(row, dtype=np.float64)
    cols = np.arange(x.size)
    nan = np.isnan(x)
    if nan[t]:
        return nan & (cols < t)
    with np.errstate(invalid="ignore"):
        return nan | (x > x[t]) | ((x == x[t]) & (cols < t))


def answer_ref(x, labels, cand=()):
    """x (n, V) float array of stored values, labels (n,) with -1 = none, cand: token ids -> (pred, rank, choice) int32 arrays"""
    x = np.asarray(x)
    n = x.shape[0]
    pred, rank, choice = (np.full(n, -1, dtype=np.int32) for _ in range(3))
    cand = [int(c) for c in cand]
    for r in range(n):
        row = x[r].astype(np.float64)
        pred[r] = _first_in_order(row)
        t = int(labels[r])
        if t >= 0:
            rank[r] = int(before(row, t).sum())
        if cand:
            v = x[r, cand].astype(np.float32)
            s = np.float32(0.0)
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                for c in range(len(cand)):
                    s = np.float32(s + v[c])
                q = (v / s).astype(np.float32)
            choice[r] = _first_in_order(q.astype(np.float64))
    return pred, rank, choice


def top_k_hit(rank, k):
    rank = np.asarray(rank)
    return ((rank >= 0) & (rank < k)).astype(np.float32)


def planted_rows(V, rng, bf16=False):
    """(rows (m, V) float32, labels (m,), description list): the hand-made rows of the issue, built for any V >= 8
       * the label's value repeated at lower and at higher indices (ties on both sides)
       * ranks exactly k - 1 and k for k = 1 and k = 5
       * a row with NaNs (label a number / label a NaN)
       * -0 against +0, +inf / -inf"""
    assert V >= 8
    rows, labels, what = [], [], []
    base = rng.standard_normal(V).astype(np.float32)
    base = np.clip(base, -3, 3)

    def add(row, t, name):
        rows.append(row.astype(np.float32)); labels.append(t); what.append(name)

    t = V // 2
    r = base.copy(); r[:] = np.minimum(r, 2.0); r[t] = 2.5; r[1] = 2.5; r[V - 1] = 2.5; r[0] = 2.5
    add(r, t, "ties: the label's value at two lower and one higher index -> rank 2")
    for k in (1, 5):
        for want in (k - 1, k):
            r = np.minimum(base.copy(), 1.0); r[t] = 2.0
            others = [c for c in range(V) if c != t][:want]
            for j, c in enumerate(others):
                r[c] = 3.0 + j
            add(r, t, f"rank exactly {want} (k = {k})")
    r = base.copy(); r[3] = np.nan; r[V - 2] = np.nan; r[t] = 5.0            # the label holds the largest number
    add(r, t, "NaN row, the label is a number: both NaNs sort before it")
    add(r.copy(), V - 2, "NaN row, the label is the second NaN: rank 1")
    add(r.copy(), 3, "NaN row, the label is the first NaN: rank 0")
    r = np.full(V, -1.0, dtype=np.float32); r[2] = -0.0; r[5] = 0.0; r[6] = 0.0
    add(r, 5, "-0 and +0 are one value: rank 1")
    r = base.copy(); r[4] = np.inf; r[1] = -np.inf
    add(r, 1, "+inf first, the label -inf last: rank V - 1")
    x = np.stack(rows)
    if bf16:
        x = bf16_round(x)
    return x, np.asarray(labels, dtype=np.int32), what
