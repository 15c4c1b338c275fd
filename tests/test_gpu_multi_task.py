"""LAVENDER_Multi_Task / Agent_Multi_Task (lavender_amd/multi_task.py) against the reference's own multi-task code (tests/golden/
multitask_micro.npz, written by tests/golden/make_goldens_multitask.py from main_multi_task_mlm.py), against the single-task callers on the same
weights, and against itself across geometry changes.  Micro configuration, dropout and drop-path 0 wherever weights or gradients are compared.

Evaluation flags of retrieval / lsmdc-mc are arg-maxima of t / (t + f) on RAW logits that lie within 0.2 of zero on this configuration, with the
candidates of a group about 1e-3 apart: an error far below the logit tolerance overturns them, so the fixture records none (see its script).
These two tasks' flags are checked against the numpy restatement of lav_match_readout (tests/match_readout_ref.py) on the very logits the
model handed to the kernel, on both mt_rows settings, and their logits against the oracle under DESIGN 6d's criterion."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.helpers import BERT_CFGS, Tok, hf_cfg, make_args, make_batch, sub
from tests.test_gpu_qa_rows import _grad_check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = ["captioning_x", "retrieval_x", "qamc_x", "qamc_lsmdc-mc", "qaoe_x"]
SINGLE = {"captioning_x": "LAVENDER_Captioning", "retrieval_x": "LAVENDER_Retrieval_MLM", "qamc_x": "LAVENDER_QAMC_MLM",
          "qamc_lsmdc-mc": "LAVENDER_RetMC_MLM", "qaoe_x": "LAVENDER_QAOE_MLM"}
TRUE, FALSE = 2995, 6270


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "multitask_micro.npz"))


def task_batch(g, task):
    """the host batch of a task as the fixture script built it: clips from its seeds, text and labels from the fixture"""
    V = BERT_CFGS["micro"]["vocab"]
    t = lambda k: torch.from_numpy(g[f"{task}::{k}"])
    if task == "captioning_x":
        b = {"img": make_batch(2, T=4, X=20, vocab=V, seed=21)["img"], "txt": t("txt"), "ans_mtm": t("ans_mtm")}
    elif task == "retrieval_x":
        b = {"img": make_batch(3, T=2, X=26, vocab=V, seed=int(g[f"{task}::seed"]))["img"], "txt": t("txt"), "vid": g[f"{task}::vid"].tolist()}
    elif task == "qamc_x":
        b = {"img": make_batch(3, T=4, vocab=V, seed=23)["img"], "txt": t("txt"), "mask_ans": t("mask_ans"), "ans_idx": t("ans_idx")}
    elif task == "qamc_lsmdc-mc":
        b = {"img": make_batch(2, T=2, vocab=V, seed=int(g[f"{task}::seed"]) + 100)["img"], "txt": t("txt"), "mask_ans": t("mask_ans")}
    else:
        b = {"img": make_batch(3, T=6, vocab=V, seed=25)["img"], "txt": t("txt"), "mask_ans": t("mask_ans")}
    b["mask"] = (b["txt"] != 0).long()
    b["task"] = task
    return b


def clone(b):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def dev(b):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def filled(cls_name, **kw):
    """a model of lavender_amd class `cls_name` with the oracle's key-seeded weights, dropout and drop-path 0"""
    import lavender_amd as LA
    from oracle import lavender_ref as R
    cfg = dict(hf_cfg("micro"), hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    args = make_args("micro", "micro", 3, txt_backbone=cfg, fusion_encoder=cfg, tokenizer=cfg, lr=2e-5, decay=1e-3, max_iter=20, max_grad_norm=1.0,
                     vis_backbone_lr_mul=1, size_vocab=-1, size_option=5, label_smoothing=0.0, drop_worst_ratio=0.0, task="multi_task", **kw)     # 0: what the reference's loss runs with (see the fixture script)
    m = getattr(LA, cls_name)(args, Tok())
    sd = m.state_dict()
    new = {k: R.fill_tensor(k, v.shape) for k, v in sd.items() if v.is_floating_point()}
    new["fc_mtm.predictions.decoder.bias"] = new["fc_mtm.predictions.bias"]
    m.load_state_dict(new, strict=False)
    m.cuda()
    for layer in m.enc_img.swin.layers:
        for blk in layer.blocks:
            blk.drop_prob, blk.keep_prob = 0.0, 1.0
    m.arena()
    return m, args


def single_forward(m, task, b):
    b = {k: v for k, v in dev(b).items() if k != "task"}
    out = m(b)
    return (out["out"], out["ans"]) if isinstance(out, dict) else out


def loss_of(task, logits, ans, args):
    from lavender_amd.agent import CrossEntropyIgnore
    from lavender_amd.captioning import CaptioningLoss
    flat, lab = logits.flatten(0, logits.dim() - 2), ans.flatten()
    n = int((ans != -1).sum())
    if "captioning" in task:
        return CaptioningLoss({"label_smoothing": args.label_smoothing}, keep_logits=True)(flat, lab, n)
    return CrossEntropyIgnore(keep_logits=True)(flat, lab, n)


# ---- 1. the same bits as the single-task callers; the reference's numbers ---------------------------------------------------------------------
@pytest.mark.parametrize("task", TASKS)
def test_forward_is_bit_identical_to_the_single_task_caller_and_matches_the_reference(task):
    g = _golden()
    b = task_batch(g, task)
    ms, _ = filled(SINGLE[task])
    mm, args = filled("LAVENDER_Multi_Task")
    ms.eval(), mm.eval()
    with torch.no_grad():
        o1, a1 = single_forward(ms, task, clone(b))
        o1, a1 = o1.clone(), a1.clone()
        o2, a2 = single_forward(ms, task, clone(b))
        assert torch.equal(o1, o2) and torch.equal(a1, a2), "the single-task caller is not bit-identical to itself on a second run"
        r = mm(dev(clone(b)))
        assert set(r) == {"out", "ans"}
        assert r["out"].shape == o1.shape and torch.equal(r["out"], o1), (task, (r["out"].float() - o1.float()).abs().max().item())
        assert r["ans"].shape == a1.shape and torch.equal(r["ans"], a1)
        a = r["out"].float().cpu()
        assert (r["ans"].cpu().numpy() == g[f"{task}::ans"]).all()
        d_cols = np.abs(a[..., torch.from_numpy(g["cols"])].numpy() - g[f"{task}::out_cols"]).max()
        d_lse = np.abs(torch.logsumexp(a, -1).numpy() - g[f"{task}::out_lse"]).max()
        ls = loss_of(task, r["out"], r["ans"], args).item()
    print(f"{task}: logits vs the reference max {d_cols:.3e}, lse {d_lse:.3e}, loss {ls:.5f} (reference {g[f'{task}::loss'][0]:.5f})")
    assert d_cols < 3e-2 and d_lse < 2e-2 and abs(ls - g[f"{task}::loss"][0]) < 1e-2


# ---- 2. forward_rows: the same loss, gradients under the QA rows criterion ---------------------------------------------------------------------
class _G:
    def __init__(self, grad):
        self.grad = grad


class _Named:
    """gradients by parameter name, shaped like a module for tests.test_gpu_variants._grad_check"""

    def __init__(self, grads):
        self.grads = grads

    def named_parameters(self):
        return [(k, _G(v)) for k, v in self.grads.items()]


def _prepared(ag, b, dl=None):
    b = clone(b)
    if dl is not None or getattr(ag.args, "enable_task_token", False):
        b = ag.add_prompt_or_task_token(b, dl)
    return ag.prepare_batch(b)


@pytest.mark.parametrize("task,pretxt", [(t, None) for t in TASKS] + [("qaoe_x", "task"), ("qamc_lsmdc-mc", "prompt")])
def test_forward_rows_has_the_loss_and_the_gradients_of_forward(task, pretxt):
    import lavender_amd as LA
    g = _golden()
    b = task_batch(g, task)
    m, args = filled("LAVENDER_Multi_Task", mt_rows=True)
    args.enable_task_token, args.enable_prompt = pretxt == "task", pretxt == "prompt"
    ag = LA.Agent_Multi_Task(args, m, list(g["ans_tok_ids"]))
    if pretxt == "prompt":
        ids = torch.tensor([101, 2003, 1996, 2678, 102])
        b["prompt"] = (ids, torch.ones_like(ids))
    m.eval()                                                     # no dropout either way; the graph is the training graph
    res = {}
    for rows in (False, True):
        pb = _prepared(ag, b)
        pb["_mt_rows"] = rows
        m.arena().zero_grad()
        out = m(pb)
        n_lab = pb["_n_lab"]
        if rows:
            assert out["out"].dim() == 2 and out["out"].shape[0] == n_lab and out["ans"].shape == (n_lab,) and bool((out["ans"] != -1).all())
            assert out["ans"].cpu().tolist() == res[False][2]
        else:
            a = out["ans"].flatten()
            res_labels = a[a != -1].cpu().tolist()
        ls = loss_of(task, out["out"], out["ans"], args)
        ls.backward()
        from lavender_amd.engine import dw_join
        dw_join()
        torch.cuda.synchronize()
        res[rows] = (ls.item(), {k: p.grad.float().cpu().clone() for k, p in m.named_parameters()}, res_labels if not rows else None)
    print(f"{task} pretxt={pretxt}: loss full {res[False][0]:.6f} rows {res[True][0]:.6f}")
    assert abs(res[False][0] - res[True][0]) < 1e-4
    _grad_check(_Named(res[True][1]), {k: _G(v) for k, v in res[False][1].items()})


# ---- 3. ten steps of the reference's Agent_Multi_Task ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt_rows", [False, True], ids=["full", "rows"])
def test_ten_steps_match_the_reference(mt_rows):
    """tests/test_gpu_agent_steps.py's criteria over the ten recorded steps: loss within 1e-2 per step, learning rates rtol 1e-6, every update norm
    within 5 %, update cosine above 0.99, ac equal to the fixture's (the fixture keeps rows whose top-1 margin is inside the logit tolerance
    out).  For each picked parameter the number of sampled elements that carry a sizeable update, and the cosine over those, is printed:
    only the vocabulary rows the batches use move in the word embeddings, so few sampled elements decide that cosine."""
    import lavender_amd as LA
    g = _golden()
    m, args = filled("LAVENDER_Multi_Task", mt_rows=mt_rows)
    ag = LA.Agent_Multi_Task(args, m, list(g["ans_tok_ids"]))
    before = {k: p.detach().float().cpu().clone() for k, p in m.named_parameters()}
    for step, task in enumerate(g["order"].tolist() * 2):
        r = ag.train_step(_prepared(ag, task_batch(g, task)))
        lrs = [grp["lr"] for grp in ag.optzr.param_groups]
        print(f"step {step} {task}: ls {r['ls']:.5f} (reference {g['train_ls'][step]:.5f}) ac {r['ac']:.4f} (reference {g['train_ac'][step]:.4f})")
        assert set(r) == {"ls", "ac"} and abs(r["ls"] - g["train_ls"][step]) < 1e-2
        assert r["ac"] == pytest.approx(float(g["train_ac"][step]), abs=1e-6)
        assert np.allclose(sorted(set(lrs)), sorted(set(g["train_lrs"][step].tolist())), rtol=1e-6), (lrs, g["train_lrs"][step])
    torch.cuda.synchronize()
    after = {k: p.detach().float().cpu() for k, p in m.named_parameters()}
    bad = []
    for k, n in zip(g["delta_keys"].tolist(), g["delta_norms"]):
        if k not in after or k.endswith("attention.self.key.bias"):      # see tests/test_gpu_agent_steps.py: the true gradient is 0
            continue
        d = (after[k] - before[k]).double().norm().item()
        if n < 1e-12:
            assert d < 1e-9, (k, d)
        elif abs(d - n) > 0.05 * n:
            bad.append((k, d, n))
    assert not bad, bad[:10]
    worst = []
    for key in g.files:
        if key.startswith("delta_sub::"):
            k = key.split("::")[1]
            a, b = sub(after[k] - before[k], 2048).astype(np.float64), g[key].astype(np.float64)
            cos = float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))
            big = np.abs(b) > 0.1 * np.abs(b).max()
            cos_big = float((a[big] * b[big]).sum() / (np.linalg.norm(a[big]) * np.linalg.norm(b[big]) + 1e-30))
            print(f"{k}: cosine of the update vs the reference {cos:.4f}; {int(big.sum())} of {b.size} sampled elements carry an update above a "
                  f"tenth of the largest, cosine over those {cos_big:.4f}")
            worst.append((k, cos))
    assert all(c > 0.99 for _, c in worst), [w for w in worst if w[1] <= 0.99]


# ---- 4. no state leaks across geometries ----------------------------------------------------------------------------------------------------------
def _freeze(ag):
    ag.lr_scheduler.min_lr = 0.0
    ag.lr_scheduler.base_lrs = [0.0 for _ in ag.lr_scheduler.base_lrs]
    for grp in ag.optzr.param_groups:
        grp["lr"] = 0.0


def _grab_grads(ag, m):
    """every parameter's gradient as the optimizer meets it (backward_step zeroes the arena afterwards): a list of {name: tensor}, one per step"""
    seen = []
    step = ag.optzr.step

    def spy(*a, **kw):
        torch.cuda.synchronize()
        seen.append({k: p.grad.detach().double().cpu() for k, p in m.named_parameters()})
        return step(*a, **kw)
    ag.optzr.step = spy
    return seen


def _single_step_grads(task, b):
    """one training step of the task's existing single-task agent on a fresh model: its gradients by parameter name"""
    import lavender_amd as LA
    m, args = filled(SINGLE[task])
    b = {k: v for k, v in clone(b).items() if k != "task"}
    if task == "captioning_x":
        ag = LA.Agent_Captioning(args, m)
    elif task == "retrieval_x":
        ag = LA.Agent_Retrieval_MLM(args, m)
    elif task == "qamc_x":
        ag = LA.Agent_QAMC_MLM(args, m, [1014, 1015, 1016, 1017, 1018])
    elif task == "qamc_lsmdc-mc":
        ag = LA.Agent_RetMC_MLM(args, m)
    else:
        ag = LA.Agent_QAOE_MLM(args, m)
    _freeze(ag)
    seen = _grab_grads(ag, m)
    pb = ag.prepare_batch(b)
    if task == "captioning_x":
        pb["attn_mask_type"] = "seq2seq"
        ag.train_step(pb)
    else:
        ag.step(pb, True)
    return seen[0]


@pytest.mark.parametrize("task", TASKS)
def test_no_state_leaks_from_the_other_tasks_geometries(task):
    """Two checks on the gradients of a step on `task` by a fresh multi-task agent (a) and by one that first ran the four other tasks (b).
    1. The arena: |a - b|_2 / |a|_2 over all gradients must not exceed twice the same distance between two fresh runs of the task's single-task
       agent, and a and b must be equal where that spread is exactly 0.
    2. Per named parameter, so that a stale unit as small as one LayerNorm reduction or one bias cannot hide among millions of other
       gradients: |a_k - b_k|_2 <= 2 spread_k + 2^-20 |a_k|_2 + 2^-23 sqrt(n_k) rms(arena).  One pair of runs does not measure a parameter's
       spread: the runs differ by the order of fp32 atomic sums, single ulps of a few elements, and most small tensors show a spread of
       exactly 0 in one pair and a flipped ulp in the next.  The two further terms are that noise in the number format: 8 ulps of the tensor's own
       norm (a reordered fp32 sum), and one ulp of a typical gradient per element (tensors whose gradient is pure cancellation, like the key
       bias).  A stale workspace, another tensor's reduction or a wrong descriptor is wrong by a fraction of the gradient itself."""
    import lavender_amd as LA
    g = _golden()
    batches = {t: task_batch(g, t) for t in TASKS}
    s1, s2 = _single_step_grads(task, batches[task]), _single_step_grads(task, batches[task])
    grads = []
    for others in ([], [t for t in TASKS if t != task]):
        m, args = filled("LAVENDER_Multi_Task")
        ag = LA.Agent_Multi_Task(args, m, list(g["ans_tok_ids"]))
        _freeze(ag)
        seen = _grab_grads(ag, m)
        for t in others + [task]:
            ag.train_step(_prepared(ag, batches[t]))
        grads.append(seen[-1])
    assert set(grads[0]) == set(s1)
    tot = lambda a, b: (sum((a[k] - b[k]).norm().item() ** 2 for k in a) ** 0.5) / (sum(b[k].norm().item() ** 2 for k in b) ** 0.5)
    spread, d = tot(s1, s2), tot(grads[1], grads[0])
    n_all = sum(v.numel() for v in grads[0].values())
    rms = (sum(v.norm().item() ** 2 for v in grads[0].values()) / n_all) ** 0.5
    bad, n_exact = [], 0
    for k, a in grads[0].items():
        spread_k, d_k = (s1[k] - s2[k]).norm().item(), (a - grads[1][k]).norm().item()
        n_exact += spread_k == 0.0
        if d_k > 2 * spread_k + 2.0 ** -20 * a.norm().item() + 2.0 ** -23 * a.numel() ** 0.5 * rms:
            bad.append((k, d_k, spread_k, a.norm().item()))
    print(f"{task}: arena |d| / |g| {d:.3e}, bound 2 x single-task spread = {2 * spread:.3e}; multi-task vs single-task agent {tot(grads[0], s1):.3e}; "
          f"{len(grads[0])} parameters, {n_exact} with a spread of exactly 0 in this pair of runs, over the per-parameter bound: {bad[:6]}")
    if spread == 0.0:
        assert all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])
    else:
        assert d <= 2 * spread
    assert not bad, bad[:10]


# ---- 5. evaluation ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt_rows", [False, True], ids=["full", "rows"])
def test_eval_flags(mt_rows):
    """qamc / qaoe: eval_step's flags equal the reference's (the fixture holds only flags that no logit error within the tolerance overturns).
    retrieval / lsmdc-mc: eval_step's flags equal the numpy restatement of the read-out rule applied to the logits, row map, columns and ground
    truth that the agent handed to lav_match_readout -- which are checked in turn: the ground truth against the batch, the row map against the
    labelled positions, and (next test) the logits against the oracle."""
    import lavender_amd as LA
    from lavender_amd import hip as K
    from tests import match_readout_ref as MR
    g = _golden()
    m, args = filled("LAVENDER_Multi_Task", mt_rows=mt_rows)
    ag = LA.Agent_Multi_Task(args, m, list(g["ans_tok_ids"]))
    for task in ("qamc_x", "qaoe_x"):
        flags = ag.eval_step(_prepared(ag, task_batch(g, task)))
        want = {k.split("::flag_")[1]: g[k].tolist() for k in g.files if k.startswith(f"{task}::flag_")}
        print(task, "flags", flags, "reference", want)
        assert want and flags == want
    real = K.match_readout
    for task, G, O, gt_want in (("retrieval_x", 3, 3, [0, 1, 2]), ("qamc_lsmdc-mc", 2, 3, None)):
        b = task_batch(g, task)
        if gt_want is None:
            gt_want = (b["mask_ans"] == TRUE).any(-1).int().argmax(1).tolist()
        calls = []

        def spy(logits, G_, O_, tc, fc, row=None, gt=None, **kw):
            calls.append((logits.detach().float().cpu().numpy(), G_, O_, tc, fc, None if row is None else np.asarray(row), np.asarray(gt)))
            return real(logits, G_, O_, tc, fc, row=row, gt=gt, **kw)
        K.match_readout = spy
        try:
            flags = ag.eval_step(_prepared(ag, b))
        finally:
            K.match_readout = real
        assert len(calls) == 1 and set(flags) == {"ac"}
        x, G_, O_, tc, fc, row, gt = calls[0]
        assert (G_, O_) == (G, O) and gt.tolist() == gt_want
        if mt_rows:
            assert x.shape == (G * O, 2) and (tc, fc) == (0, 1) and row is None
        else:
            X = b["txt"].shape[-1]
            assert x.shape == (G * O * X, BERT_CFGS["micro"]["vocab"]) and (tc, fc) == (TRUE, FALSE)
            assert row.tolist() == (np.arange(G * O) * X + X - 1).tolist()          # the [MASK] closes every text of these batches
        _, _, hit = MR.match_ref(x, G, O, tc, fc, row=row, gt=gt)
        print(task, "mt_rows", mt_rows, "flags", flags)
        assert flags["ac"] == hit.astype(np.float32).tolist()


@pytest.mark.parametrize("task", ["retrieval_x", "qamc_lsmdc-mc"])
def test_match_rows_logits_within_twice_the_full_paths_error(task):
    """DESIGN 6d's criterion (tests/test_gpu_retrieval_eval.py: e_ours <= 2 e_cross + 2^-10) on the batch's own pairs: the rows path's
    (p_true, p_false) against the float64-evaluated oracle, e = the full path's error against the same oracle"""
    import lavender_amd as LA
    from lavender_amd import hip as K
    from oracle import lavender_ref as R
    g = _golden()
    b = task_batch(g, task)
    bc = BERT_CFGS["micro"]
    P = R.filled_params("micro", hidden=bc["hidden"], layers=bc["layers"], ffn=bc["ffn"], vocab=bc["vocab"])
    with torch.no_grad():
        ref, _ = (R.retrieval_forward if task == "retrieval_x" else R.retmc_mlm_forward)(P, clone(b), "micro", bc["heads"])
    pair64 = torch.stack([ref[:, -1, TRUE], ref[:, -1, FALSE]], 1).double()
    m, args = filled("LAVENDER_Multi_Task", mt_rows=True)
    ag = LA.Agent_Multi_Task(args, m, list(g["ans_tok_ids"]))
    m.eval()
    seen = []
    real = K.match_readout

    def spy(logits, *a, **kw):
        seen.append(logits.detach().float().cpu().double().clone())
        return real(logits, *a, **kw)
    K.match_readout = spy
    try:
        with torch.no_grad():
            pb = _prepared(ag, b)
            res = m.match_rows(pb)
    finally:
        K.match_readout = real
    assert res is not None and len(seen) == 1, "the [MASK]-row path must apply to the micro configuration"
    with torch.no_grad():
        out = m({k: v for k, v in pb.items() if k != "_mt_rows"})["out"]
        full_choice, full_hit = m.match_full(pb, out)
    rows = seen[0]
    full = torch.stack([out[:, -1, TRUE], out[:, -1, FALSE]], 1).float().cpu().double()
    assert rows.shape == full.shape == pair64.shape
    e_full, e_rows = (full - pair64).abs().max().item(), (rows - pair64).abs().max().item()
    print(f"{task}: (p_true, p_false) rows path vs float64 oracle {e_rows:.3e}; full path vs oracle {e_full:.3e}; rows vs full {(rows - full).abs().max():.3e}")
    assert e_rows <= 2 * e_full + 2.0 ** -10
    assert (rows - full).abs().max().item() <= 2 * e_full + 2.0 ** -10


def test_one_device_to_host_copy_per_evaluated_loader(monkeypatch):
    import lavender_amd as LA
    g = _golden()
    counts = {"n": 0}

    def counting(name):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **kw):
            if self.is_cuda:
                counts["n"] += 1
            return real(self, *a, **kw)
        return f
    for mt_rows in (True, False):
        m, args = filled("LAVENDER_Multi_Task", mt_rows=mt_rows)
        ag = LA.Agent_Multi_Task(args, m, list(g["ans_tok_ids"]))
        for task in TASKS[1:]:
            dl = [{k: v for k, v in task_batch(g, task).items() if k != "task"} for _ in range(3)]
            with monkeypatch.context() as mp_:
                for name in ("tolist", "cpu", "item", "numpy", "__bool__", "__int__", "__float__"):
                    mp_.setattr(torch.Tensor, name, counting(name))
                counts["n"] = 0
                res = ag.non_cap_evaluate(task, dl)
                n = counts["n"]
            print(task, "mt_rows", mt_rows, res, "device -> host reads", n)
            assert n == 1, (task, mt_rows, n)
            assert set(res) == ({"ac_1", "ac_5"} if "qaoe" in task else {"ac"})


# ---- 6. one rank over RCCL with the arena reducer attached ------------------------------------------------------------------------------------------
def _rccl_worker(port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    import lavender_amd as LA
    from lavender_amd.dp import ArenaReducer
    g = _golden()
    plan = ["retrieval_x", "captioning_x", "qaoe_x"]
    runs = []
    for attach in (False, True):
        m, args = filled("LAVENDER_Multi_Task", mt_rows=True)
        ag = LA.Agent_Multi_Task(args, m, list(g["ans_tok_ids"]))
        _freeze(ag)
        if attach:
            ag.dp = ArenaReducer(m)                          # prepare_dist_model() only attaches it for world > 1
        seen = _grab_grads(ag, m)
        for t in plan:
            ag.train_step(_prepared(ag, task_batch(g, t)))
        torch.cuda.synchronize()
        runs.append(seen)
    flat = lambda d: torch.cat([d[k].flatten() for k in sorted(d)])
    ok = all(((flat(a) - flat(b)).norm() / flat(b).norm()).item() < 1e-4 for a, b in zip(runs[1], runs[0])) and len(runs[1]) == len(plan)
    q.put(bool(ok))
    dist.destroy_process_group()


def test_three_alternating_steps_over_rccl_single_rank():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(29700 + (os.getpid() % 1000), q))
    p.start()
    import queue as _queue
    import time as _time
    t0, res = _time.time(), None
    while res is None:
        try:
            res = q.get(timeout=2)
        except _queue.Empty:
            if p.exitcode not in (None, 0) or _time.time() - t0 > 240:
                if p.is_alive():
                    p.terminate()
                pytest.fail(f"RCCL worker failed (exit code {p.exitcode})")
    p.join(timeout=60)
    assert res is True
