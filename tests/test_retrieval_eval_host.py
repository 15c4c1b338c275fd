"""CPU: the host side of the text-to-video retrieval evaluation (lavender_amd/retrieval_eval.py) -- rank rule and metric strings against a
restatement of the reference's loop (eval_retrieval_mlm.py:213-240), first-seen video / text order, the clip frame rule of the eval dataset,
the data-parallel text shards at gloo world 2, and the [MASK] check of pair_source."""
import os
import socket

import numpy as np
import pytest
import torch


def _reference_loop(S, gt):
    """eval_retrieval_mlm.py:213-240 restated: per text a list of (column, score) in column order, sorted by -score (stable), 1-based position
    of the ground truth; R@K by 1.0 / N per hit; median truncated; the reference's string formats"""
    ranks = []
    for t in range(S.shape[0]):
        items = [(v, float(S[t, v])) for v in range(S.shape[1])]
        tmp = sorted(items, key=lambda d: -d[1])
        ranks.append([d[0] for d in tmp].index(int(gt[t])) + 1)
    n = len(ranks)
    res = {'r@1': 0, 'r@5': 0, 'r@10': 0, 'median': []}
    for p in ranks:
        res['r@1'] += 1.0 / n if p <= 1 else 0
        res['r@5'] += 1.0 / n if p <= 5 else 0
        res['r@10'] += 1.0 / n if p <= 10 else 0
        res['median'].append(p)
    res['median'] = int(np.median(res['median']))
    return ranks, {k: (f"{v * 100:.2f}" if k != 'median' else f"{v}") for k, v in res.items()}


@pytest.mark.parametrize("seed, nt, nv", [(0, 7, 12), (1, 10, 3), (2, 64, 40), (3, 2, 2)])
def test_ranks_and_metric_strings_match_the_reference_loop(seed, nt, nv):
    from lavender_amd.retrieval_eval import metrics_from_ranks, ranks_host
    rng = np.random.default_rng(seed)
    S = np.round(rng.random((nt, nv)) * 8).astype(np.float32) / 8          # many ties
    S[rng.random((nt, nv)) < 0.05] = np.inf
    S[rng.random((nt, nv)) < 0.05] = -np.inf
    gt = rng.integers(0, nv, nt)
    ref_ranks, ref_res = _reference_loop(S, gt)
    ours = ranks_host(S, gt)
    assert ours.tolist() == ref_ranks
    assert metrics_from_ranks(ours) == ref_res


def test_even_count_median_truncates_and_duplicate_captions():
    from lavender_amd.retrieval_eval import metrics_from_ranks
    assert metrics_from_ranks([1, 2])["median"] == "1"                     # np.median 1.5 -> int 1
    assert metrics_from_ranks([2, 5, 6, 9])["median"] == "5"               # 5.5 -> 5
    # two captions of the same video are two queries: each adds 1.0 / N in query order
    r = metrics_from_ranks([1, 1, 3])
    assert r == {'r@1': f"{(1.0 / 3 + 1.0 / 3) * 100:.2f}", 'r@5': f"{(1.0 / 3 * 3) * 100:.2f}", 'r@10': f"{(1.0 / 3 * 3) * 100:.2f}", 'median': "1"}


def test_nan_sorts_last_in_column_order():
    from lavender_amd.retrieval_eval import ranks_host
    nan, inf = np.nan, np.inf
    S = np.array([[0.5, nan, 0.7, nan, -inf],
                  [0.5, nan, 0.7, nan, -inf],
                  [0.5, nan, 0.7, nan, -inf],
                  [nan, nan, nan, nan, nan],
                  [inf, 0.2, inf, 0.2, nan]], dtype=np.float32)
    gt = np.array([0, 1, 3, 2, 2])
    # row 0: 0.7 before 0.5 -> 2; row 1: all 3 numbers, then the NaN of column 1 -> 4; row 2: 3 numbers, NaN col 1, then col 3 -> 5
    # row 3: all NaN, column order -> 3; row 4: tie of +inf, column 0 first -> 2
    assert ranks_host(S, gt).tolist() == [2, 4, 5, 3, 2]


def test_video_dedupe_and_column_order():
    from lavender_amd.retrieval_eval import first_seen_order
    vids = ["b", "a", "b", "c", "a", "d"]
    tids = [10, 11, 12, 13, 11, 14]
    v, vsrc, t, tsrc = first_seen_order(vids, tids)
    assert v == ["b", "a", "c", "d"] and vsrc == [0, 1, 3, 5]               # first occurrence of each video wins
    assert t == [10, 11, 12, 13, 14] and tsrc == [0, 4, 2, 3, 5]            # text 11: first place, last occurrence


class _Stub:
    size_frame = 5

    @staticmethod
    def sampling(start, end, n):
        from lavender_amd.data import Dataset_Base
        return Dataset_Base.sampling(None, start, end, n)


@pytest.mark.parametrize("frames, size_frame, multi, want", [
    (5, 5, False, [[0, 1, 2, 3, 4]]),
    (1, 5, True, [[0]]),
    (12, 5, False, [[0, 3, 6, 8, 11]]),                                    # round(2.75) = 3, round(5.5) = 6, round(8.25) = 8
    (12, 5, True, [[0, 3, 6, 8, 11], [1, 4, 6, 8, 11], [2, 4, 6, 9, 11]]),     # round(8.5) = 8 (half to even)
    (3, 5, True, [[0, 1, 2]]),
    (10, 4, True, [[0, 3, 6, 9], [1, 4, 6, 9], [2, 4, 7, 9]]),
])
def test_clip_frame_indices(frames, size_frame, multi, want):
    """Dataset_RetrievalTsEval.get_clips_with_temporal_sampling (eval_retrieval_task_specific.py:24-58) restated: clip k of the multi-clip test
    samples size_frame positions from frame k to min(k + (size_frame - 1) * n_clips, frames - 1)"""
    from lavender_amd.data import clip_frame_indices
    assert clip_frame_indices(frames, size_frame, multi, _Stub.sampling) == want


def test_text_shards_cover_every_text_once():
    from lavender_amd.retrieval_eval import merge_ranks, text_shards
    for n in (1, 2, 7, 100):
        for w in (1, 2, 3, 8):
            sh = text_shards(n, w)
            assert sh[0][0] == 0 and sh[-1][1] == n and all(a[1] == b[0] for a, b in zip(sh, sh[1:]))
            assert max(t1 - t0 for t0, t1 in sh) - min(t1 - t0 for t0, t1 in sh) <= 1
            full = np.arange(n) + 1
            assert merge_ranks([full[t0:t1] for t0, t1 in sh], sh).tolist() == full.tolist()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, S, gt, q):
    import torch.distributed as dist
    from lavender_amd.retrieval_eval import distributed_ranks, ranks_host
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    seen = []

    def stub(t0, t1):                                       # the scorer of this rank's texts only
        seen.append((t0, t1))
        return ranks_host(S[t0:t1], gt[t0:t1])
    r = distributed_ranks(S.shape[0], stub)
    q.put((rank, r.tolist(), seen))
    dist.destroy_process_group()


def test_distributed_ranks_gloo_world2():
    import torch.multiprocessing as mp
    from lavender_amd.retrieval_eval import ranks_host
    rng = np.random.default_rng(5)
    S = rng.random((9, 6)).astype(np.float32)
    gt = rng.integers(0, 6, 9)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_gloo_worker, args=(r, 2, port, S, gt, q)) for r in range(2)]
    for p in ps:
        p.start()
    out = [q.get(timeout=120) for _ in ps]
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    want = ranks_host(S, gt).tolist()
    out.sort()
    assert out[0][1] == want and out[1][1] == want
    assert out[0][2] == [(0, 5)] and out[1][2] == [(5, 9)]


@pytest.mark.parametrize("n_mask", [0, 2])
def test_pair_source_needs_exactly_one_mask_token(n_mask):
    from tests.helpers import Tok, make_args
    from lavender_amd import LAVENDER_RetrievalMlmEval
    m = LAVENDER_RetrievalMlmEval(make_args("micro", "micro", 2), Tok())
    Nt, X, Mv, Lv, H = 3, 8, 2, 4, 128
    txt = torch.full((Nt, X), 2000, dtype=torch.long)
    txt[:, -1] = 103
    txt[1, -1] = 2000
    if n_mask == 2:
        txt[1, 2] = 103
        txt[1, 5] = 103
    with pytest.raises(ValueError, match="text 1 holds %d \\[MASK\\]" % n_mask):
        m.pair_source(torch.zeros(Mv, Lv, H), torch.ones(Mv, Lv, dtype=torch.long), torch.zeros(Nt, X, H), torch.ones(Nt, X, dtype=torch.long), txt)


def test_clip_frame_indices_match_the_reference_golden(golden_dir):
    """clip_frame_indices against Dataset_RetrievalTsEval.get_clips_with_temporal_sampling of the reference itself
    (tests/golden/make_goldens_retrieval_eval.py: the method called on a stub whose get_img_or_video returns the indices)"""
    from lavender_amd.data import Dataset_Base, clip_frame_indices
    g = np.load(os.path.join(golden_dir, "retr_rank_micro.npz"))
    for n, sf, multi in g["clip_cases"].tolist():
        want = g[f"clips_{n}_{sf}_{multi}"].tolist()
        assert clip_frame_indices(n, sf, bool(multi), lambda s, e, k: Dataset_Base.sampling(None, s, e, k)) == want, (n, sf, multi)


class _WordTok:
    """tokenizer stub for str2txt: [CLS] one id per word [SEP], padded to max_length"""
    cls_token = "[CLS]"; sep_token = "[SEP]"; pad_token = "[PAD]"; mask_token = "[MASK]"; unk_token = "[UNK]"
    ids = {"[PAD]": 0, "[UNK]": 100, "[CLS]": 101, "[SEP]": 102, "[MASK]": 103, "true": 2995, "false": 6270}

    def convert_tokens_to_ids(self, toks):
        return [self.ids[t] for t in toks]

    def encode(self, s, padding=None, max_length=None, truncation=None):
        body = [2000 + len(w) for w in s.split()][:max_length - 2]
        ids = [101] + body + [102]
        return ids + [0] * (max_length - len(ids))


@pytest.mark.parametrize("multi, transform", [(False, ["img_center_crop"]), (True, ["vid_rand_crop"]), (False, ["pad_resize"])])
def test_eval_dataset_takes_frames_from_field_2_of_the_video_row(tmp_path, golden_dir, multi, transform):
    """Dataset_RetrievalMlmEval on a TSV fixture laid out as the reference's img_{dataset}.tsv: id2lineidx gives the byte offset of a video's
    line, the frames are the fields from 2 on (eval_retrieval_task_specific.py:86), clips follow clip_frame_indices, captions get [MASK]"""
    import json
    import pickle
    import shutil
    from lavender_amd import data as D
    from lavender_amd.args import EasyDict
    shutil.copy(os.path.join(golden_dir, "msrvtt_2rows.tsv"), tmp_path / "img_msrvtt.tsv")
    offs = [int(x) for x in open(os.path.join(golden_dir, "msrvtt_2rows.lineidx"))]
    pickle.dump({"vidA": offs[0], "vidB": offs[1]}, open(tmp_path / "img_msrvtt.id2lineidx.pkl", "wb"))
    json.dump({"test": [{"video": "vidB", "caption": ["a man", "is cooking"]}, {"video": "vidA", "caption": "a dog runs"}]},
              open(tmp_path / "txt_msrvtt-retrieval.json", "w"))
    args = EasyDict(dataset="msrvtt", task="msrvtt-retrieval", data_dir=str(tmp_path), size_frame=2, size_img=224, size_txt=8,
                    img_transform=transform, multi_clip_testing=multi)
    ds = D.Dataset_RetrievalMlmEval(args, "test", tokzr=_WordTok())
    assert len(ds) == 2 and ds.gt_txt2vid == {0: "vidB", 1: "vidA"}
    clips, txt, mask, tid, vid = ds[0]
    assert tid == 0 and vid == "vidB"
    assert txt.tolist() == [101, 2001, 2003, 2002, 2007, 102, 0, 0, 103] and mask.tolist() == [1] * 6 + [0, 0, 1]   # joined captions + [MASK]
    fields = ds.tsv.fields(offs[1])                                          # the line of vidB in the same mapping
    frames = fields[2:]
    want = D.clip_frame_indices(len(frames), 2, multi, ds.sampling)
    assert len(clips) == len(want) and (len(want) > 1) == multi
    for clip, idx in zip(clips, want):
        assert [p.buf for p in clip] == [frames[i] for i in idx]              # the same (address, length) field references
    p0 = clips[0][0]
    if transform == ["pad_resize"]:
        assert (p0.resize_w, p0.resize_h) == (224, 224)
    else:
        assert (p0.resize_w, p0.resize_h, p0.crop_x, p0.crop_y) == (298, 224, 37, 0)     # 320 x 240 -> 298 x 224, centre window


def test_rank_and_metrics_of_the_reference_golden(golden_dir):
    """ranks_host / metrics_from_ranks on the golden's S (the reference's LAVENDER_RetrievalMlmEval + Dataset_Product scores) give the golden's
    ranks and strings, digit for digit"""
    from lavender_amd.retrieval_eval import metrics_from_ranks, ranks_host
    g = np.load(os.path.join(golden_dir, "retr_rank_micro.npz"))
    S = g["S"]
    assert np.array_equal(S, (g["p_true"] / (g["p_true"] + g["p_false"])).reshape(S.shape))
    ranks = ranks_host(S, g["gt"])
    assert ranks.tolist() == g["ranks"].tolist()
    assert metrics_from_ranks(ranks) == dict(zip(g["metrics_keys"].tolist(), g["metrics_vals"].tolist()))


def test_eval_script_with_a_checkpoint_refuses_synthetic_clips(tmp_path):
    """--path_ckpt without the test split (or the tokenizer) is an error: no results file is written next to the checkpoint"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ckpt = tmp_path / "ckpt_violet_retrieval_0.pt"
    ckpt.write_bytes(b"")
    cfg = tmp_path / "args.json"
    cfg.write_text(json.dumps(dict(type="retrieval", task="msrvtt-retrieval", dataset="msrvtt", data_dir=str(tmp_path / "none"), size_txt=15)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(root, "eval_retrieval_mlm.py"), "--config", str(cfg), "--path_ckpt", str(ckpt)],
                       capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert p.returncode != 0 and "nothing was evaluated" in p.stderr, p.stdout[-1000:] + p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == ["args.json", "ckpt_violet_retrieval_0.pt"]
