"""Host side of multi-task MLM fine-tuning (lavender_amd/multi_task.py, main_multi_task_mlm.py): MetaLoader against the reference's recorded
draws (tests/golden/multitask_micro.npz), its restart / accum_steps / broadcast behaviour, the task dispatch, token and log-key rules, the
per-dataset args overlay, and the numpy restatement of lav_match_readout (tests/match_readout_ref.py) against the agents' torch formulation
and its own stated rule."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import match_readout_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pools():
    return {"a": ([("a", i) for i in range(3)], 1), "b": ([("b", i) for i in range(2)], 2), "c": ([("c", i) for i in range(4)], 1)}


def _draw(ml, n):
    out = []
    for i, (task, batch) in enumerate(ml):
        out.append((task, batch))
        if i == n - 1:
            break
    return out


def test_metaloader_reproduces_the_references_draws(golden_dir):
    from lavender_amd.multi_task import MetaLoader
    g = np.load(os.path.join(golden_dir, "multitask_micro.npz"))
    random.seed(88)
    ml = MetaLoader(_pools())
    assert ml.sampling_pools == ["a", "b", "b", "c"]
    got = [f"{t}:{b[1]}" for t, b in _draw(ml, 50)]
    assert got == g["meta_draws"].tolist()
    assert all(t == b[0] for t, b in _draw(MetaLoader(_pools()), 20))           # every batch comes from the loader of the task drawn


def test_metaloader_restarts_an_exhausted_loader_and_honours_accum_steps():
    from lavender_amd.multi_task import MetaLoader
    ml = MetaLoader({"only": [10, 11, 12]})
    assert [b for _, b in _draw(ml, 8)] == [10, 11, 12, 10, 11, 12, 10, 11]
    random.seed(3)
    tasks = [t for t, _ in _draw(MetaLoader(_pools(), accum_steps=4), 24)]
    assert all(len(set(tasks[i:i + 4])) == 1 for i in range(0, 24, 4))           # the task is redrawn every fourth step only
    assert len(set(tasks)) > 1
    with pytest.raises(ValueError):
        MetaLoader({"x": 5})


def _gloo_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lavender_amd.multi_task import MetaLoader
    random.seed(100 + rank)                                                      # different seeds: only the broadcast can align the ranks
    ml = MetaLoader(_pools(), distributed=True)
    seq = [t for t, _ in _draw(ml, 30)]
    random.seed(100)
    own = [random.choice(ml.sampling_pools) for _ in range(30)]
    q.put((rank, seq, own))
    dist.barrier()
    dist.destroy_process_group()


def test_metaloader_broadcasts_rank_zeros_choice():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29300 + (os.getpid() % 500)
    ps = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = dict()
    for _ in range(2):
        rank, seq, own = q.get(timeout=120)
        res[rank] = (seq, own)
    for p in ps:
        p.join(timeout=60)
    assert res[0][0] == res[1][0] == res[0][1]                                   # both ranks ran rank 0's sequence


def test_dispatch_order_and_task_tokens():
    from lavender_amd.multi_task import best_metric_of, task_kind, task_token_of
    kinds = {"captioning_x": "captioning", "retrieval_msrvtt": "retrieval", "qamc_tgif-action": "qamc", "qamc_lsmdc-mc": "qamc_ret",
             "qaoe_msvd": "qaoe", "qaoe_lsmdc-fib": "qaoe", "captioning_retrieval": "captioning", "retrieval_qamc": "retrieval",
             "qamc_qaoe": "qamc"}
    for task, kind in kinds.items():
        assert task_kind(task) == kind, task
    with pytest.raises(NotImplementedError, match="forward\\(\\) for vqa_x"):
        task_kind("vqa_x")
    tokens = {"retrieval_x": "vtm", "qamc_x": "mc", "qamc_lsmdc-mc": "vtm", "qaoe_x": "oe", "qaoe_lsmdc-fib": "oe", "captioning_x": "cap"}
    for task, tok in tokens.items():
        assert task_token_of(task) == tok, task
    with pytest.raises(NotImplementedError):
        task_token_of("vqa_x")
    assert [best_metric_of(t) for t in ("captioning_x", "qaoe_x", "qamc_x", "retrieval_x")] == ["CIDEr", "ac_1", "ac", "ac"]


class _Agent:
    """Agent_Multi_Task's host-side methods on a bare object (no model, no device)"""

    def __init__(self, **args):
        from collections import defaultdict
        from lavender_amd.args import EasyDict
        from lavender_amd.multi_task import Agent_Multi_Task
        self.args = EasyDict(dict(enable_prompt=False, enable_task_token=False, iter_per_ep=2, max_iter=2, logging_steps=100, p_mask=0.0), **args)
        self.log = defaultdict(list)
        for name in ("add_prompt_or_task_token", "best_epoch", "run", "_eval_all", "meter_loss", "meter_acc"):
            setattr(self, name, getattr(Agent_Multi_Task, name).__get__(self))
        self.task2loss, self.task2acc, self.saved = {}, {}, []

    def log_train(self, ep, step):
        return "log"

    def prepare_batch(self, batch):
        return batch

    def train_step(self, batch):
        return {"ls": 1.0, "ac": 0.5}

    def save_model(self, ep):
        self.saved.append(ep)

    def evaluate(self, ep, task, dl, tag=None):
        if "captioning" in task:
            return {}
        return {"ac_1": 0.25, "ac_5": 0.5} if "qaoe" in task else {"ac": 0.75}


class _DS:
    def __init__(self, name):
        self.name = name

    def get_prompt(self):
        return self.name


class _DL(list):
    def __init__(self, name, items):
        super().__init__(items)
        self.dataset = _DS(name)


def test_task_token_prompt_log_keys_and_best_epoch(capsys):
    from lavender_amd.multi_task import MetaLoader
    ag = _Agent(enable_task_token=True)
    assert ag.add_prompt_or_task_token({"task": "qamc_lsmdc-mc"}, None)["task_name"] == "vtm"
    assert ag.add_prompt_or_task_token({"task": "qamc_tgif"}, None)["task_name"] == "mc"
    ag = _Agent(enable_prompt=True)
    tr = {"qaoe_a": _DL("prompt of qaoe_a", [{}]), "captioning_b": _DL("prompt of captioning_b", [{"txt": torch.zeros(1, 4, dtype=torch.long)}])}
    ml = MetaLoader(tr)
    assert ag.add_prompt_or_task_token({"task": "captioning_b"}, ml)["prompt"] == "prompt of captioning_b"      # the task's OWN dataset
    assert ag.add_prompt_or_task_token({"task": "qaoe_a"}, tr["qaoe_a"])["prompt"] == "prompt of qaoe_a"
    # run: evaluation and save_model when step % iter_per_ep == 0 and step, the step >= max_iter break, no tail when the last step closed an epoch
    ag = _Agent()
    ag.masking = lambda txt, p_mask: {}
    vl = {"qaoe_a": [], "captioning_b": [], "retrieval_c": []}
    ag.run(MetaLoader(tr), vl, {"qaoe_a": []})
    assert ag.saved == [2]
    assert set(ag.log) == {"qaoe_a_vl_ac_1", "qaoe_a_vl_ac_5", "retrieval_c_vl_ac", "qaoe_a_ts_ac_1", "qaoe_a_ts_ac_5"}
    assert ag.best_epoch("qaoe_a", "vl", "ac_1") == (0, 0.25) and ag.best_epoch("captioning_b", "vl", "CIDEr") is None
    assert "captioning_b_vl_CIDEr" not in ag.log                                     # asking did not create the key
    so = capsys.readouterr().out
    assert "Best ac_1 on qaoe_a val @ ep 0, 25.00" in so and "Best ac on retrieval_c val @ ep 0, 75.00" in so and "Best ac_1 on qaoe_a test @ ep 0" in so
    assert "captioning_b val" not in so and "Ep 2 captioning_b vl: {}" in so
    # tail evaluation: max_iter not a multiple of iter_per_ep -> "Last step", checkpoint numbered by the step
    ag = _Agent()
    ag.args.max_iter, ag.args.iter_per_ep = 3, 2
    ag.masking = lambda txt, p_mask: {}
    ag.run(MetaLoader(tr), vl, {})
    assert ag.saved == [2, 3] and "Last step 3 qaoe_a vl: " in capsys.readouterr().out


def test_per_dataset_args_overlay(tmp_path):
    import importlib
    sys.path.insert(0, ROOT)
    M = importlib.import_module("main_multi_task_mlm")
    from lavender_amd.args import EasyDict
    shared = EasyDict(size_batch=8, size_txt=25, size_frame=4, size_option=5, nested=EasyDict(a=1, b=[1, 2]), datasets=[])
    d = {"type": "qamc", "task": "lsmdc-mc", "size_batch": 2, "size_txt": 40, "nested": {"a": 7, "deep": {"x": 1}}}
    full = M.dataset_args(shared, d)
    assert (full.size_batch, full.size_txt, full.size_frame, full.size_option, full.type, full.task) == (2, 40, 4, 5, "qamc", "lsmdc-mc")
    assert isinstance(full.nested, EasyDict) and full.nested.a == 7 and full.nested.deep.x == 1     # update(): the nested dict is replaced, as an EasyDict
    assert shared.size_batch == 8 and shared.nested.a == 1 and "type" not in shared
    full.nested.deep.x = 2
    assert d["nested"]["deep"]["x"] == 1                                          # a deep copy either way
    assert "mt_rows" in __import__("lavender_amd.args", fromlist=["_DEFAULTS"])._DEFAULTS
    assert __import__("lavender_amd.args", fromlist=["_DEFAULTS"])._DEFAULTS["mt_rows"] is False and M.CLI_DEFAULTS["mt_rows"] is True


# ---- the numpy restatement of lav_match_readout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,O", [(3, 3), (4, 5), (1, 7), (6, 2)])
def test_match_ref_equals_the_agents_torch_formulation(G, O):
    rng = np.random.default_rng(10 * G + O)
    X, V, T, F = 6, 50, 29, 6
    out = torch.from_numpy((rng.standard_normal((G * O, X, V)) * 3).astype(np.float32))
    ans = torch.full((G * O, X), -1, dtype=torch.long)
    pos = rng.integers(0, X, size=G * O)
    gt = rng.integers(0, O, size=G)
    for k in range(G * O):
        ans[k, pos[k]] = T if (k % O) == gt[k // O] else F
    flags, s = MR.torch_formulation(out, ans, T, F, G, O)
    score, choice, hit = MR.match_ref(out.reshape(G * O * X, V).numpy(), G, O, T, F, row=np.arange(G * O) * X + pos, gt=gt)
    assert hit.astype(np.float32).tolist() == flags
    assert (score.view(np.uint32) == s.numpy().reshape(-1).view(np.uint32)).all()
    pair = torch.stack([out[torch.arange(G * O), torch.from_numpy(pos), T], out[torch.arange(G * O), torch.from_numpy(pos), F]], 1).numpy()
    assert (MR.match_ref(pair, G, O, 0, 1, gt=gt)[1] == choice).all()            # the (n, 2) block without a row map: the same answer


def test_match_ref_obeys_the_stated_rule_on_planted_groups():
    nan, inf = np.nan, np.inf
    cases = [  # (t, f) per candidate, expected choice
        ([(3, 1), (3, 1), (1, 3)], 0),                       # a tie: the lowest o
        ([(1, 3), (3, 1), (3, 1)], 1),
        ([(3, 1), (nan, 1), (0, 0)], 1),                     # NaN above every number; the first NaN (0 / 0 at o = 2 is a NaN too)
        ([(0, 0), (inf, 1), (3, 1)], 0),
        ([(1, -3), (-0.0, 1), (0.0, 1)], 1),                 # -0 equals +0: the lowest o of the two; both above -0.5
        ([(1, -3), (0.0, 1), (-0.0, 1)], 1),
        ([(1, -3), (2, -2), (-2, 2)], 1),                    # t + f = 0: +inf at o = 1, -inf at o = 2
        ([(-2, 2), (-2, 2)], 0),                             # all -inf
        ([(1, 3)], 0)]
    for pairs, want in cases:
        x = np.array(pairs, dtype=np.float32)
        s, c, h = MR.match_ref(x, 1, len(pairs), 0, 1, gt=[want])
        assert c.tolist() == [want] and h.tolist() == [1], (pairs, c)
        assert MR.match_ref(x, 1, len(pairs), 0, 1, gt=[-1])[2].tolist() == [0] and MR.match_ref(x, 1, len(pairs), 0, 1, gt=[len(pairs)])[2].tolist() == [0]
        assert (s.view(np.uint32)[np.isnan(s)] == 0x7FC00000).all()
    # a row outside the block is not read: NaN in `score`, but below every number, -inf and a NaN quotient included
    x = np.array([[9, 1], [-2, 2], [0, 0]], dtype=np.float32)
    assert MR.match_ref(x, 1, 3, 0, 1, row=[7, 1, -1])[1].tolist() == [1]
    assert MR.match_ref(x, 1, 3, 0, 1, row=[7, 2, 1])[1].tolist() == [1]
    assert MR.match_ref(x, 1, 3, 0, 1, row=[7, 3, -1])[1].tolist() == [0]
    assert np.isnan(MR.match_ref(x, 1, 3, 0, 1, row=[7, 1, 0])[0][0])


def test_match_readout_is_declared_bound_and_wrapped():
    from lavender_amd import _lib, hip
    header = open(os.path.join(ROOT, "include", "lavender_hip.h")).read()
    assert "int lav_match_readout(" in header and "lav_match_readout" in _lib.EXPORTS and hasattr(_lib.lib, "lav_match_readout")
    assert callable(hip.match_readout) and _lib.ABI_VERSION == 7


# ---- the synthetic datasets of the entry point ------------------------------------------------------------------------------------------------
def _ds_args(**kw):
    from lavender_amd.args import EasyDict
    return EasyDict(dict(size_txt=12, size_frame=2, size_img=32, size_option=4, size_batch=2, n_workers=0, distributed=False), **kw)


def test_synthetic_retrieval_and_retmc_datasets():
    from lavender_amd.data import StubTokenizer, SyntheticRetMC, SyntheticRetrieval
    tok, a = StubTokenizer(), _ds_args()
    ds = SyntheticRetrieval(a, 5, "val", tok, vocab=8192)
    b = ds.collate_batch([ds[i] for i in range(3)])
    assert b["img"].shape == (3, 2, 3, 32, 32) and b["txt"].shape == b["mask"].shape == (3, 13) and len(set(b["vid"])) == 3
    assert ((b["txt"] == 103).sum(1) == 1).all() and (b["txt"][:, -1] == 103).all() and (b["txt"][:, 0] == 101).all()     # the appended [MASK]
    assert ((b["txt"] == 102).sum(1) == 1).all() and (b["mask"] == (b["txt"] != 0).long()).all() and int(b["txt"].max()) < 8192
    assert torch.equal(ds[1][1], ds[1][1]) and not torch.equal(ds[1][1], SyntheticRetrieval(a, 5, "test", tok, vocab=8192)[1][1])
    ids, m = ds.get_prompt()
    assert ids.dim() == 1 and ids[0] == 101 and ids[-1] == 102 and m.shape == ids.shape and bool(m.all()) and "true or false" in ds.prompt_text
    mc = SyntheticRetMC(a, 5, "train", tok, vocab=8192)
    b = mc.collate_batch([mc[i] for i in range(3)])
    assert b["txt"].shape == b["mask"].shape == b["mask_ans"].shape == (3, 4, 13) and b["img"].shape == (3, 2, 3, 32, 32)
    assert ((b["txt"] == 103).sum(-1) == 1).all() and ((b["mask_ans"] != -1) == (b["txt"] == 103)).all()       # one labelled [MASK] per candidate
    assert ((b["mask_ans"] == 2995).sum((1, 2)) == 1).all() and ((b["mask_ans"] == 6270).sum((1, 2)) == 3).all()   # one "true" per clip
    ids, m = mc.get_prompt()
    assert ids[0] == 101 and ids[-1] == 102 and bool(m.all())
    from lavender_amd.data import SyntheticCaption
    import main_caption
    assert main_caption.SyntheticCaption is SyntheticCaption


def test_entry_point_builds_a_loader_per_task_type(tmp_path):
    import importlib
    sys.path.insert(0, ROOT)
    M = importlib.import_module("main_multi_task_mlm")
    from lavender_amd.data import StubTokenizer, SyntheticQA, SyntheticRetMC, SyntheticRetrieval, SyntheticCaption
    a = _ds_args(datasets=M.easy([{"type": "retrieval", "task": "a", "size_batch": 3}, {"type": "qaoe", "task": "lsmdc-fib"},
                                  {"type": "qamc", "task": "lsmdc-mc", "size_option": 3, "size_txt": 9}, {"type": "qamc", "task": "tgif"},
                                  {"type": "captioning", "task": "c", "size_frame": 3}]))
    tr, vl, ts, n, ans = M.get_meta_dataloaders(a, StubTokenizer(), 2, 0, 8192)
    assert list(tr) == list(vl) == list(ts) == ["retrieval_a", "qaoe_lsmdc-fib", "qamc_lsmdc-mc", "qamc_tgif", "captioning_c"]
    kinds = [type(tr[t].dataset) for t in tr]
    assert kinds == [SyntheticRetrieval, SyntheticQA, SyntheticRetMC, SyntheticQA, SyntheticCaption]
    assert n == 10 and all(len(tr[t]) == 2 for t in tr) and ans == [1014, 1015, 1016, 1017]        # the QAMC dataset's option tokens, not lsmdc-mc's
    b = next(iter(tr["qamc_lsmdc-mc"]))
    assert b["txt"].shape == (2, 3, 10) and b["mask_ans"].shape == (2, 3, 10) and b["img"].shape[1] == 2
    assert next(iter(tr["retrieval_a"]))["txt"].shape == (3, 13) and next(iter(tr["captioning_c"]))["img"].shape[1] == 3
    assert tr["qaoe_lsmdc-fib"].dataset.kind == "oe" and len(vl["retrieval_a"].dataset) == 3        # one batch of the task's own size
    with pytest.raises(NotImplementedError):
        M.get_meta_dataloaders(_ds_args(datasets=M.easy([{"type": "vqa", "task": "x"}])), StubTokenizer(), 1, 0, 8192)
