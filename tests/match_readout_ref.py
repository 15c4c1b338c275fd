"""The rule of lav_match_readout (include/lavender_hip.h) restated with numpy.  The inputs are the STORED values (fp32, or bf16 widened exactly);
the rule fixes fp32 for the sum and the quotient, so those two steps are float32 here as well.

  s[k]       t / (t + f) of the two columns of row[k]; every NaN as the one pattern 0x7fc00000
  choice[g]  first candidate o of the group in the order: NaN quotients (lowest o first), then numbers descending (-0 = +0, lowest o first among
             equals), then the candidates whose row lies outside the block ("NaN-last": not read, never ahead of one that was; lowest o first)
  hit[g]     choice[g] == gt[g]; a gt outside [0, O) never hits"""
import numpy as np

NAN_BITS = np.uint32(0x7FC00000)


def match_ref(x, G, O, true_col, false_col, row=None, gt=None):
    """x (n_rows, width) float array of stored values -> (score (G * O,) float32, choice (G,) int32, hit (G,) int32 or None)"""
    x = np.asarray(x)
    n_rows = x.shape[0]
    row = np.arange(G * O, dtype=np.int64) if row is None else np.asarray(row, dtype=np.int64).reshape(-1)
    assert row.size == G * O
    read = (row >= 0) & (row < n_rows)
    r = np.where(read, row, 0)
    t, f = x[r, true_col].astype(np.float32), x[r, false_col].astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = (t / (t + f).astype(np.float32)).astype(np.float32)
    s[~read] = np.nan
    bits = s.view(np.uint32).copy()
    bits[np.isnan(s)] = NAN_BITS
    s = bits.view(np.float32)
    v, rd = s.astype(np.float64).reshape(G, O), read.reshape(G, O)
    nan = np.isnan(v) & rd
    num = rd & ~nan
    with np.errstate(invalid="ignore"):
        top = np.where(num, v, -np.inf).max(1, keepdims=True)
        first_num = np.argmax(num & (v == top), axis=1)         # == holds between -0 and +0, and finds a -inf maximum among the READ candidates
    choice = np.where(nan.any(1), np.argmax(nan, axis=1), np.where(num.any(1), first_num, 0)).astype(np.int32)
    hit = None if gt is None else (choice == np.asarray(gt, dtype=np.int64).reshape(-1)).astype(np.int32)
    return s, choice, hit


def torch_formulation(out, ans, true_id, false_id, G, O):
    """the agents' read-out (main_retrieval_mlm.py:107-118 / main_retmc_mlm.py:129-140) on (pairs, X, V) logits and (pairs, X) labels: the flags as a list"""
    import torch
    p_true, p_false = out[:, :, true_id].float(), out[:, :, false_id].float()
    s = p_true / (p_true + p_false)
    s = s[ans != -1].view(G, O)
    a = ans[ans != -1].view(G, O)
    return (torch.argmax(s, dim=-1) == (a == true_id).nonzero()[:, 1]).float().tolist(), s
