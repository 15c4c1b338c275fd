"""Float64 reference of the captioning loss (lav_caption_loss_fwd_bwd, lavender_amd.captioning.CaptioningLoss), the seeded inputs of its tests and
first-order error bounds derived from the kernel's arithmetic (test infrastructure; used by tests/test_caption_train_host.py on the CPU and by
tests/test_gpu_caption_loss.py / tests/test_gpu_caption_train.py on the MI355X).

Reference (model_for_captioning.py:10-37 on the labelled rows; V classes, target t, eps = label_smoothing, q_t = 1 - eps, q_c = eps / (V - 1)):

    loss_row = sum_c q_c (log q_c - log p_c) = C - (1 - eps) log p_t - eps / (V - 1) sum_{c != t} log p_c
    C        = (1 - eps) log(1 - eps) + eps log(eps / (V - 1))          (terms with q_c = 0 are 0: eps = 0 is -log p_t)
    d loss_row / d logit_c = p_c - q_c
    k = int(n (1 - ratio)) rows with the smallest losses are averaged when the drop is on (ties: the lower row first), else all n

Error bound of the kernel (lavender_amd/csrc/loss_optim.hip, cap_row_kernel / cap_select_kernel / cap_total_kernel; u = 2^-24, g(n) = n u / (1 - n u)).
A thread reads T = ceil(ld / 8 / 256) chunks of 8 columns; a term passes through at most D = T + 7 rescale stages (one per chunk whose maximum
rises, six wave-butterfly levels, the four-wave sum).

  exp       e(a) = __expf(a), a = x - m:  the fp32 subtraction (u |a|), the product a log2(e) (u |a|) and v_exp_f32 (one ulp = 2u), doubled for the
            rounded constant:  rho_e(a) = (2 |a| + 4) u, relative
  S         sum of V exponentials: a chain of 8 T additions per thread, 6 + 2 additions of the block tree, every rescale one exponential and one
            product:  rho_S = g(8 T + 16) + (D + 1) (rho_e(A) + 2u), A = max - min of the row;  S >= 1 (the maximum contributes exp(0))
  lse       M + __logf(S): v_log_f32 and the product with ln 2 (4u |log S| + 2u), the addition:  b_lse = rho_S + 4u log S + 2u + u |lse|
  loss      eps = 0:  lse - x_t:  b_lse + u |loss|
            eps > 0:  (C + lse) - (1 - eps) x_t - q (SX - x_t), SX the fp32 sum of the V logits (chain 8 T + 10):
                      b_lse + 2u |C| + u |C + lse| + 3u |(1 - eps) x_t| + q g(8 T + 10) sum|x| + 4u |q (SX - x_t)| + u (|C + lse - (1 - eps) x_t| + |loss|)
  total     fp32 sum of the kept losses, ceil(rows / 256) + 8 additions:  sum b_loss + g(ceil(rows / 256) + 8) sum|loss|;  loss = total / k: + u
  gradient  (e(x - lse) - q) (1 / k) stored as bf16:  b = [p (rho_e(|x - lse|) + b_lse) + u |p - q| + u q] / k + 3u |g|, then the store:
            2^-8 (|g| + b)   (tests.gemm_bounds.U_BF)
"""
import math

import numpy as np
import torch

from tests.gemm_bounds import U32, U_BF, gam


def bf16_round(a):
    """float array -> the nearest bf16 values (ties to even), as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def make_logits(rows, V, seed, sigma=1.0):
    """the (rows, V) bf16-valued logits of a seed (numpy default_rng), float32"""
    return bf16_round(sigma * np.random.default_rng(seed).standard_normal((rows, V), dtype=np.float32))


def make_case(rows, V, n_lab, seed, sigma=1.0):
    """(x (rows, V) float32 bf16-valued, labels (rows,) int64): n_lab labelled rows at seeded positions with seeded target columns.  The target
    logit of the j-th labelled row is -4 + j / 16 in a seeded order (exact in bf16 up to 16): the row losses form a ladder whose steps are far
    above the kernel's error bound, so the kept set of the drop-the-worst selection is unambiguous (the GPU test asserts that on the float64 losses)."""
    assert n_lab <= min(rows, 180)
    rng = np.random.default_rng(seed + 7919)
    x = make_logits(rows, V, seed, sigma)
    labels = np.full(rows, -1, dtype=np.int64)
    pos = np.sort(rng.permutation(rows)[:n_lab])
    cols = rng.integers(0, V, size=n_lab)
    ladder = (-4.0 + rng.permutation(n_lab) / 16.0).astype(np.float32)
    labels[pos] = cols
    x[pos, cols] = ladder
    return x, labels


def _t(a, dtype):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(dtype)


def const_term(eps, V):
    return (1.0 - eps) * math.log(1.0 - eps) + (eps * math.log(eps / (V - 1)) if eps > 0 else 0.0)


def row_losses(x, labels, eps):
    """float64 row losses of the closed form; 0 on unlabelled rows.  x (rows, V) array or tensor, labels (rows,) int64"""
    x = _t(x, torch.float64)
    labels = _t(labels, torch.int64)
    V = x.shape[1]
    lab = labels >= 0
    t = labels.clamp_min(0)
    lse = torch.logsumexp(x, 1)
    xt = x.gather(1, t[:, None])[:, 0]
    logp_t = xt - lse
    loss = -logp_t if eps == 0 else const_term(eps, V) - (1.0 - eps) * logp_t - eps / (V - 1) * ((x.sum(1) - V * lse) - logp_t)
    return torch.where(lab, loss, torch.zeros_like(loss))


def kept_rows(loss, labels, k):
    """bool (rows,): the k labelled rows that come first by (loss ascending, row ascending)"""
    loss, labels = np.asarray(loss, dtype=np.float64), np.asarray(labels)
    idx = np.nonzero(labels >= 0)[0]
    order = idx[np.lexsort((idx, loss[idx]))]
    kept = np.zeros(len(labels), dtype=bool)
    kept[order[:k]] = True
    return kept


def captioning_loss(x, labels, eps, ratio=0.0, drop=True):
    """CaptioningLoss.forward in float64 on rows that may carry -1 labels: dict(loss, row_loss, kept, k, n, correct, grad).  grad = d loss / d x."""
    x = _t(x, torch.float64)
    lab_t = _t(labels, torch.int64)
    V = x.shape[1]
    rl = row_losses(x, lab_t, eps)
    n = int((lab_t >= 0).sum())
    k = int(n * (1 - ratio)) if (drop and ratio > 0) else n
    kept = torch.from_numpy(kept_rows(rl.numpy(), lab_t.numpy(), k))
    total = rl[kept].sum()
    pred = x.argmax(1)                                       # lowest index on a tie
    correct = (pred == lab_t) & (lab_t >= 0)
    p = torch.softmax(x, 1)
    q = torch.full_like(p, eps / (V - 1))
    q.scatter_(1, lab_t.clamp_min(0)[:, None], 1.0 - eps)
    grad = torch.where(kept[:, None], (p - q) / max(k, 1), torch.zeros_like(p))
    return dict(loss=(total / k).item() if k > 0 else float("nan"), total=total.item(), row_loss=rl, kept=kept, k=k, n=n, correct=correct, grad=grad, p=p, q=q)


def bounds(x, labels, eps, ld, ref):
    """first-order error bounds of the kernel's results on the case `ref` = captioning_loss(...) describes (see the module docstring):
    dict(row_loss (rows,), total, loss, grad (rows, V))"""
    x = _t(x, torch.float64)
    lab_t = _t(labels, torch.int64)
    rows, V = x.shape
    u = U32
    T = -(-(ld // 8) // 256)
    D = T + 7
    rho_e = lambda a: (2.0 * a + 4.0) * u
    A = x.max(1).values - x.min(1).values
    lse = torch.logsumexp(x, 1)
    logS = lse - x.max(1).values
    rho_S = gam(8 * T + 16) + (D + 1) * (rho_e(A) + 2 * u)
    b_lse = rho_S + 4 * u * logS + 2 * u + u * lse.abs()
    xt = x.gather(1, lab_t.clamp_min(0)[:, None])[:, 0]
    loss = ref["row_loss"]
    if eps == 0:
        b_loss = b_lse + u * loss.abs()
    else:
        C, q = const_term(eps, V), eps / (V - 1)
        sx = x.sum(1)
        b_loss = (b_lse + 2 * u * abs(C) + u * (C + lse).abs() + 3 * u * ((1 - eps) * xt).abs() + q * gam(8 * T + 10) * x.abs().sum(1) +
                  4 * u * (q * (sx - xt)).abs() + u * ((C + lse - (1 - eps) * xt).abs() + loss.abs()))
    b_loss = torch.where(lab_t >= 0, b_loss, torch.zeros_like(b_loss))
    kept = ref["kept"]
    b_total = b_loss[kept].sum().item() + gam(-(-rows // 256) + 8) * loss[kept].abs().sum().item()
    k = max(ref["k"], 1)
    b_mean = b_total / k + u * abs(ref["total"]) / k
    g = ref["grad"]
    b_g = (ref["p"] * (rho_e((x - lse[:, None]).abs()) + b_lse[:, None]) + u * (ref["p"] - ref["q"]).abs() + u * ref["q"]) / k + 3 * u * g.abs()
    b_g = U_BF * (g.abs() + b_g) + b_g
    b_g = torch.where(kept[:, None], b_g, torch.zeros_like(b_g))
    return dict(row_loss=b_loss, total=b_total, loss=b_mean, grad=b_g)
