"""Golden vectors of the text-to-video retrieval evaluation (CONTAINER ONLY -- needs /root/reference), written to retr_rank_micro.npz:
  * the reference's LAVENDER_RetrievalMlmEval ('feat' then 'cross', eval_retrieval_mlm.py:10-47) and Dataset_Product (:77-115) on the micro
    model: 4 videos x 2 clips, 6 captions ending in [MASK] (videos 0 and 1 have two captions each); features kept as the script keeps them
    (featv: first occurrence of a video, featt: per text id, :176-192); (p_true, p_false) at the [MASK] of every pair in the product's order;
  * S (text x video, first-seen video order) and the ranks / metrics of :213-240, restated below in this file's own code;
  * the clip frame indices of Dataset_RetrievalTsEval.get_clips_with_temporal_sampling (eval_retrieval_task_specific.py:24-58), called on a
    stub `self` whose get_img_or_video returns the indices it is given.  (A row with fewer frames than size_frame is not a case: the
    reference's error print there names a variable that is assigned only later and raises.)
Same recipe as make_goldens_variants.py (stubbed third-party imports, parameters filled from their state_dict keys, seeded inputs).

    python tests/golden/make_goldens_retrieval_eval.py
"""
import sys
sys.dont_write_bytecode = True
import importlib
import os
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG  # noqa: E402
from make_goldens import make_batch, BERT_CFGS  # noqa: E402
from make_goldens_variants import build  # noqa: E402

VIDEO_OF_TEXT = [0, 0, 1, 1, 2, 3]
CLIP_CASES = [(5, 5, 0), (1, 5, 1), (12, 5, 0), (12, 5, 1), (10, 4, 1), (17, 5, 1), (30, 6, 0), (30, 6, 1)]


def micro_inputs(vocab):
    """the inputs of tests/test_gpu_retrieval_eval.py::_micro: clips (4, 2, 2, 3, 224, 224), captions (6, 32) ending in [MASK]"""
    b = make_batch(4 * 2, T=2, vocab=vocab, seed=9)
    img = b["img"].view(4, 2, 2, 3, 224, 224)
    tb = make_batch(6, T=1, vocab=vocab, seed=10)
    txt, mask = tb["txt"].clone(), tb["mask"].clone()
    txt[:, -1], mask[:, -1] = 103, 1
    body = txt[:, :-1]
    body[body == 103] = 104
    return img, txt, mask


def rank_and_metrics(S, gt):
    """eval_retrieval_mlm.py:213-240 in this file's words: per text, columns in order, stable sort by descending score, 1-based place of the
    ground truth; R@K sums 1 / N per hit in text order; median truncated to int; the script's string formats"""
    ranks = []
    for t in range(S.shape[0]):
        order = sorted(range(S.shape[1]), key=lambda v: -float(S[t, v]))
        ranks.append(order.index(int(gt[t])) + 1)
    n = len(ranks)
    acc = {"r@1": 0, "r@5": 0, "r@10": 0}
    for p in ranks:
        for k, lim in (("r@1", 1), ("r@5", 5), ("r@10", 10)):
            if p <= lim:
                acc[k] += 1.0 / n
    out = {k: f"{v * 100:.2f}" for k, v in acc.items()}
    out["median"] = f"{int(np.median(ranks))}"
    return np.array(ranks), out


def run_pairs(ref):
    EV = importlib.import_module("eval_retrieval_mlm")
    m, _ = build(ref, EV.LAVENDER_RetrievalMlmEval, "micro", "micro", 4)
    vocab = BERT_CFGS["micro"]["vocab_size"]
    img, txt, mask = micro_inputs(vocab)
    m.eval()
    vids = [f"v{v}" for v in VIDEO_OF_TEXT]
    featv, featt = {}, {}
    with torch.no_grad():
        f_img, m_img, f_txt, m_txt, t_out = m('feat', {"img": img[VIDEO_OF_TEXT], "txt": txt, "mask": mask})
        for i, v in enumerate(vids):                       # eval_retrieval_mlm.py:176-192
            if v not in featv:
                featv[v] = {'video': v, 'feat_img': f_img[i], 'mask_img': m_img[i]}
            featt[i] = {'tid': i, 'feat_txt': f_txt[i], 'mask_txt': m_txt[i], 'txt': t_out[i]}
        ds = EV.Dataset_Product(featv, featt)
        dl = torch.utils.data.DataLoader(ds, batch_size=7, shuffle=False, num_workers=0, collate_fn=ds.collate_batch)
        pt, pf, tids, vids_p = [], [], [], []
        for batch in dl:                                    # :195-212, with the two logits kept apart
            out_ret, t = m(typ='cross', batch=batch)
            sel = t == 103
            pt.append(out_ret[:, :, 2995][sel])
            pf.append(out_ret[:, :, 6270][sel])
            tids += list(batch["tid"])
            vids_p += list(batch["vid"])
    pt, pf = torch.cat(pt).numpy(), torch.cat(pf).numpy()
    assert len(pt) == len(ds) == 24
    col = {v: i for i, v in enumerate(featv)}              # first-seen video order (the order rank[tid_] is filled in)
    S = np.zeros((len(featt), len(featv)), dtype=np.float32)
    for k, (ti, vi) in enumerate(zip(tids, vids_p)):
        S[ti, col[vi]] = pt[k] / (pt[k] + pf[k])
    gt = np.array([col[v] for v in vids])
    ranks, res = rank_and_metrics(S, gt)
    print(f"   retrieval eval: {len(pt)} pairs, ranks {ranks.tolist()}, {res}")
    return dict(txt=txt.numpy(), pair_tid=np.array(tids), pair_vid=np.array([col[v] for v in vids_p]), p_true=pt.astype(np.float32),
                p_false=pf.astype(np.float32), S=S, gt=gt, ranks=ranks, metrics_keys=np.array(list(res)), metrics_vals=np.array(list(res.values())),
                video_of_text=np.array(VIDEO_OF_TEXT))


def run_clips(ref):
    EVT = importlib.import_module("eval_retrieval_task_specific")
    DS = importlib.import_module("dataset")
    out = {}
    for n, sf, multi in CLIP_CASES:
        stub = types.SimpleNamespace(size_frame=sf, args=types.SimpleNamespace(multi_clip_testing=bool(multi)))
        stub.sampling = lambda s, e, k, _st=stub: DS.Dataset_Base.sampling(_st, s, e, k)
        stub.get_img_or_video = lambda bufs: torch.tensor(bufs, dtype=torch.long)
        clips = EVT.Dataset_RetrievalTsEval.get_clips_with_temporal_sampling(stub, list(range(n)))
        out[f"clips_{n}_{sf}_{multi}"] = clips.numpy()
    return out


if __name__ == "__main__":
    torch.set_num_threads(8)
    ref = MG.import_reference()
    res = run_pairs(ref)
    res.update(run_clips(ref))
    res["clip_cases"] = np.array(CLIP_CASES)
    np.savez_compressed(f"{HERE}/retr_rank_micro.npz", **res)
    print("written", f"{HERE}/retr_rank_micro.npz")
