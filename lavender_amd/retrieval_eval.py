"""Text-to-video retrieval evaluation of LAVENDER_RetrievalMlmEval -- the loop of the reference's eval_retrieval_mlm.py:138-247.

Three phases, all on the device until the ranks come back:
  'feat'     every batch through model('feat'); video features deduplicated by video id (first occurrence wins, :176-183), text features
             per text id (the last occurrence wins, in first-seen order, as the featt dict does); both land in ONE (U, H) buffer.
  scoring    every (text, video) pair, text outer / video inner (Dataset_Product), through model.score_pairs in chunks into a device score
             matrix S (N_t, M_v); no host synchronisation per chunk.
  ranking    lav_retrieval_rank on S, one device -> host copy of the int32 ranks, then R@1 / R@5 / R@10 / median restated from :220-240.

Rank rule (the stable sort of :223-227 over the columns in first-seen video order): rank = 1 + #{v : S[t,v] > S[t,gt]}
+ #{v before gt : S[t,v] == S[t,gt]}.  A score of NaN (p_true + p_false == 0) sorts after every number and NaNs keep their column order; the
reference's sort has no defined order there.

With torch.distributed initialised at world > 1 every rank runs 'feat' over all batches, scores a contiguous shard of the texts, and the
int32 ranks are all-gathered (text_shards / merge_ranks)."""
import os

import numpy as np
import torch

# rows (pairs x sequence length) per scoring chunk when the caller gives no chunk size: bounds the fusion-layer activations of a chunk
# (about 18 KB per row at hidden 768) while keeping the tile GEMMs full
CHUNK_ROWS = int(os.environ.get("LAV_RET_CHUNK_ROWS", "131072"))


# ---- host restatements (the reference's arithmetic, in our own code) ---------------------------------------------------------------------
def metrics_from_ranks(ranks):
    """eval_retrieval_mlm.py:220-240: R@K adds 1.0 / N per hit in query order (Python floats), median = int(np.median), strings as the
    reference formats them"""
    ranks = [int(p) for p in ranks]
    n = len(ranks)
    res = {'r@1': 0, 'r@5': 0, 'r@10': 0, 'median': []}
    for p in ranks:
        if p <= 1:
            res['r@1'] += 1.0 / n
        if p <= 5:
            res['r@5'] += 1.0 / n
        if p <= 10:
            res['r@10'] += 1.0 / n
        res['median'].append(p)
    res['median'] = int(np.median(res['median']))
    return {k: (f"{v * 100:.2f}" if k != 'median' else f"{v}") for k, v in res.items()}


def ranks_host(S, gt):
    """the rank rule of lav_retrieval_rank on the host: S (N_t, M_v) float32, gt (N_t,) column of each text's ground-truth video"""
    S = np.asarray(S, dtype=np.float32)
    out = np.empty(S.shape[0], dtype=np.int64)
    cols = np.arange(S.shape[1])
    for t in range(S.shape[0]):
        row, g = S[t], int(gt[t])
        sg = row[g]
        nan = np.isnan(row)
        if np.isnan(sg):
            before = ~nan | (cols < g)
        else:
            with np.errstate(invalid="ignore"):
                before = ~nan & ((row > sg) | ((row == sg) & (cols < g)))
        out[t] = 1 + int(before.sum())
    return out


def first_seen_order(vids, tids):
    """column order and row order of the evaluation: videos by first appearance (featv, first occurrence kept), texts by first appearance of
    their id with the LAST occurrence's position (featt[tid] is overwritten).  vids / tids: the per-sample ids in loader order.  Returns
    (video ids, sample index of each video, text ids, sample index of each text)."""
    vcol, vsrc = {}, []
    for i, v in enumerate(vids):
        if v not in vcol:
            vcol[v] = len(vsrc)
            vsrc.append(i)
    trow = {}
    for i, t in enumerate(tids):
        trow[t] = i                                         # dict keeps the first insertion's place, the value is the last
    return list(vcol), vsrc, list(trow), list(trow.values())


def text_shards(n_text, world):
    """contiguous text ranges [t0, t1) of each of `world` ranks (sizes differ by at most one)"""
    base, extra = divmod(n_text, world)
    out, t0 = [], 0
    for r in range(world):
        t1 = t0 + base + (1 if r < extra else 0)
        out.append((t0, t1))
        t0 = t1
    return out


def merge_ranks(parts, shards):
    """the full rank vector from every rank's shard result (in rank order)"""
    assert len(parts) == len(shards)
    for p, (t0, t1) in zip(parts, shards):
        assert len(p) == t1 - t0, (len(p), t0, t1)
    return np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1) for p in parts]) if parts else np.zeros(0, np.int64)


def distributed_ranks(n_text, local_ranks):
    """local_ranks(t0, t1) -> ranks of texts [t0, t1) (host array); with torch.distributed at world > 1 each rank computes its shard and the
    shards are all-gathered, else one call covers every text"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return np.asarray(local_ranks(0, n_text), dtype=np.int64)
    world, rank = dist.get_world_size(), dist.get_rank()
    shards = text_shards(n_text, world)
    t0, t1 = shards[rank]
    mine = np.asarray(local_ranks(t0, t1) if t1 > t0 else np.zeros(0, np.int64), dtype=np.int32)
    parts = [None] * world
    dist.all_gather_object(parts, mine)
    return merge_ranks(parts, shards)


def pair_chunk_for(L, rows=None):
    """default pairs per scoring chunk: the row budget over the sequence length"""
    return max(1, (rows or CHUNK_ROWS) // max(1, L))


# ---- the evaluator ---------------------------------------------------------------------------------------------------------------------------
def _to(dev, v):
    return v.to(dev, non_blocking=True) if isinstance(v, torch.Tensor) else v


def collect_features(model, batches):
    """phase 'feat': model('feat') over the batches.  Returns (video ids, text ids, PairSource) with every kept feature row in one buffer.
    Each batch keeps only what survives deduplication -- the rows of the videos it shows first and its text rows -- so the device holds the
    deduplicated features plus one batch, not one video block per caption."""
    dev = next(model.parameters()).device
    vcol, v_parts = {}, []                                   # video id -> column; per batch: (features, masks) of its new videos
    t_parts, t_where = [], {}                                # per batch: (features, masks, ids) of its texts; text id -> (part, row)
    with torch.no_grad():
        for b in batches:
            bd = {k: _to(dev, v) for k, v in b.items()}
            f_img, m_img, f_txt, m_txt, t = model('feat', bd)
            bv = [v.item() if isinstance(v, torch.Tensor) else v for v in b["vid"]]
            bt = [x.item() if isinstance(x, torch.Tensor) else x for x in b["tid"]]
            new = []
            for r, v in enumerate(bv):                       # first occurrence of a video wins (featv, eval_retrieval_mlm.py:176-183)
                if v not in vcol:
                    vcol[v] = len(vcol)
                    new.append(r)
            if new:
                idx = torch.tensor(new, device=dev)
                v_parts.append((f_img.index_select(0, idx), m_img.index_select(0, idx)))
            t_parts.append((f_txt.clone(), m_txt.clone(), t.clone()))   # own storage: go_feat's buffer (video rows included) is released
            for r, x in enumerate(bt):
                t_where[x] = (len(t_parts) - 1, r)           # the last occurrence's features, the first occurrence's place (featt)
            del f_img, m_img, f_txt, m_txt, t
    if not t_parts:
        raise ValueError("evaluate_t2v: no batches")
    Lv, Hd = v_parts[0][0].shape[1], v_parts[0][0].shape[2]
    X = t_parts[0][0].shape[1]
    Mv, Nt = len(vcol), len(t_where)
    buf = torch.empty((Mv * Lv + Nt * X, Hd), dtype=v_parts[0][0].dtype, device=dev)
    f_img, f_txt = buf[:Mv * Lv].view(Mv, Lv, Hd), buf[Mv * Lv:].view(Nt, X, Hd)
    m_img = torch.empty((Mv, Lv), dtype=torch.int64, device=dev)
    m_txt = torch.empty((Nt, X), dtype=torch.int64, device=dev)
    txt = torch.empty((Nt, X), dtype=torch.int64, device=dev)
    with torch.no_grad():
        c = 0
        for fi, mi in v_parts:
            f_img[c:c + fi.shape[0]].copy_(fi)
            m_img[c:c + fi.shape[0]].copy_(mi)
            c += fi.shape[0]
        del v_parts
        by_part = {}
        for j, (pi, r) in enumerate(t_where.values()):
            by_part.setdefault(pi, ([], []))
            by_part[pi][0].append(j)
            by_part[pi][1].append(r)
        for pi, (js, rs) in by_part.items():
            jd, rd = torch.tensor(js, device=dev), torch.tensor(rs, device=dev)
            for target, part in zip((f_txt, m_txt, txt), t_parts[pi]):
                target.index_copy_(0, jd, part.index_select(0, rd).to(target.dtype))
    del t_parts
    return list(vcol), list(t_where), model.pair_source(f_img, m_img, f_txt, m_txt, txt)


def score_matrix(model, src, t0, t1, pair_chunk=None):
    """phase 2 for texts [t0, t1): S (t1 - t0, M_v) fp32 on the device, pairs text-major in chunks of pair_chunk pairs"""
    Mv = src.n_video
    n_pairs = (t1 - t0) * Mv
    chunk = int(pair_chunk) if pair_chunk else pair_chunk_for(src.Lv + src.X)
    S = torch.empty((t1 - t0, Mv), dtype=torch.float32, device=src.src.device)
    with torch.no_grad():
        for p0 in range(0, n_pairs, chunk):
            p = np.arange(p0, min(n_pairs, p0 + chunk), dtype=np.int64)
            t, v = p // Mv, p % Mv
            model.score_pairs(src, v, t0 + t, out=S, out_rows=t)
    return S


def evaluate_t2v(model, batches, gt_txt2vid, pair_chunk=None, return_scores=False):
    """eval_retrieval_mlm.py:138-247 on LAVENDER_RetrievalMlmEval.  batches: dicts as Dataset_RetrievalMlmEval.collate_batch builds them
    ("img" (B, Clips, T, C, H, W), "txt", "mask", "vid", "tid", optionally "task_name" / "prompt_txt" / "prompt_mask"); gt_txt2vid: text
    id -> video id.  pair_chunk: pairs per scoring call (default: a row budget, CHUNK_ROWS).  Returns {'r@1', 'r@5', 'r@10', 'median'} as the
    reference formats them, plus 'ranks' (int64, per text in first-seen order), 'tids', 'vids' and, with return_scores, 'scores' (this rank's
    rows of S, on the device)."""
    if model.training or torch.is_grad_enabled():
        raise RuntimeError("evaluate_t2v: evaluation only -- call model.eval() and run it under torch.no_grad()")
    vids, tids, src = collect_features(model, batches)
    col = {v: i for i, v in enumerate(vids)}
    missing = [t for t in tids if gt_txt2vid.get(t) not in col]
    if missing:
        raise KeyError(f"evaluate_t2v: no ground-truth video among the evaluated ones for text ids {missing[:5]}")
    gt = np.array([col[gt_txt2vid[t]] for t in tids], dtype=np.int32)
    kept = {}

    def local(t0, t1):
        from . import hip as K
        S = score_matrix(model, src, t0, t1, pair_chunk)
        g = torch.from_numpy(gt[t0:t1]).to(S.device, non_blocking=True)
        r = K.retrieval_rank(S, g)
        kept["S"] = S
        return r.cpu().numpy()                              # the one device -> host copy of the evaluation

    ranks = distributed_ranks(len(tids), local)
    res = metrics_from_ranks(ranks)
    res.update(ranks=ranks, tids=tids, vids=vids)
    if return_scores:
        res["scores"] = kept.get("S")
    return res
