"""The rows path of the MLM-head QA callers (lavender_amd/qa_mlm.py: forward_rows, answer_rows, the agents under args.qa_rows) against the
reference fixtures, the CPU oracle and the full path of the same model.

Interval rule of the evaluation checks (DESIGN 6d's criterion): let e be the FULL path's measured max logit error against the float32 oracle on
the same weights; both paths then sit within e of the oracle, so a rows-path logit differs from the full-path logit by at most bound = 2 e.
From the full-path fp32 logits x of a labelled row with label t: rank_lo = #{x_c > x_t + bound}, rank_hi = #{x_c >= x_t - bound}; the rows
path's rank must lie in [rank_lo, rank_hi], a top-k flag must be 1 when rank_hi < k and 0 when rank_lo >= k, and is undetermined between.  The
predicted column's full-path value must be within bound of the row maximum.

Option choice: q_c = x_c / s, s = the sum of the n_c candidate logits.  With every candidate logit of the rows path within bound of the full
path's, |s' - s| <= ds = n_c bound, and where |s| > ds
    q'_c - q_c = ((x'_c - x_c) s - x_c (s' - s)) / (s s'),   so   |q'_c - q_c| <= qb_c = (bound + |q_c| ds) / (|s| - ds)
exactly (no linearisation).  The rows path picks c* with q'_c* >= q'_best, hence the full path's q_c* + qb_c* >= q_best - qb_best: that is
asserted.  A row is DETERMINED when q_best - qb_best > q_c + qb_c for every other candidate (no admissible perturbation changes the arg-max;
then the rows path must give the full path's choice); a row with |s| <= ds is undetermined and nothing is asserted of it.  At most a quarter
of the top-k / hit flags may be undetermined (a condition on the fixture, not a tolerance)."""
import os

import numpy as np
import pytest
import torch

from tests import pretxt_ref as PR
from tests.helpers import BERT_CFGS, make_batch
from tests.test_gpu_variants import _grad_check

pytestmark = pytest.mark.gpu

OPT_IDS = [1014, 1015, 1016, 1017, 1018]


def _oracle_params(bert, swin):
    from oracle import lavender_ref as R
    bc = BERT_CFGS[bert]
    P = R.filled_params(swin, hidden=bc["hidden"], layers=bc["layers"], ffn=bc["ffn"], vocab=bc["vocab"])
    for v in P.values():
        v.requires_grad_(True)
    return P, bc


def _dev(batch, host_labels=True):
    b = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    if host_labels:
        b["_lab_host"] = batch["mask_ans"]
    return b


def _check_rows_training(m, batch, g, P, Lp, tag):
    """forward_rows + loss + backward of model m (eval mode: no dropout) against the fixture g and the oracle gradients in P"""
    from lavender_amd.agent import CrossEntropyIgnore
    from lavender_amd.qa_mlm import label_rows
    lr = label_rows(batch["mask_ans"], Lp)
    m.arena().zero_grad()
    out, lab = m.forward_rows(_dev(batch))
    V = out.shape[-1]
    assert out.shape == (len(lr.row), V) and lab.cpu().tolist() == lr.label.tolist()
    a = out.detach().float().cpu()
    want_cols = g["out_cols"].reshape(-1, g["out_cols"].shape[-1])[lr.row]
    d = np.abs(a[:, torch.from_numpy(g["cols"])].numpy() - want_cols)
    lse = np.abs(torch.logsumexp(a, -1).numpy() - g["out_lse"].reshape(-1)[lr.row])
    print(tag, "labelled rows", len(lr.row), "logits max", d.max(), "lse max", lse.max())
    assert d.max() < 3e-2 and lse.max() < 2e-2
    ls = CrossEntropyIgnore()(out, lab, count=len(lr.row))
    ls.backward()
    torch.cuda.synchronize()
    print(tag, "loss", ls.item(), "fixture", g["loss"][0])
    assert abs(ls.item() - g["loss"][0]) < 1e-2
    _grad_check(m, P)


@pytest.mark.parametrize("name,cls", [("qaoe_micro_b3", "LAVENDER_QAOE_MLM"), ("qamc_micro_b3", "LAVENDER_QAMC_MLM")])
def test_forward_rows_against_fixtures(golden_dir, name, cls):
    import lavender_amd as LA
    from oracle import lavender_ref as R
    from tests.helpers import build_filled_model
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    swin, bert, B, S, heads, X = g["meta"].tolist()
    B, heads, X = int(B), int(heads), int(X)
    P, bc = _oracle_params(bert, swin)
    batch = make_batch(B, X=X, vocab=bc["vocab"], seed=6)
    batch["txt"] = torch.from_numpy(g["txt"]); batch["mask"] = (batch["txt"] != 0).long(); batch["mask_ans"] = torch.from_numpy(g["mask_ans"])
    ref, ans_ref = R.qa_mlm_forward(P, batch, swin, heads)
    torch.nn.functional.cross_entropy(ref.flatten(0, 1), ans_ref.flatten(), ignore_index=-1).backward()
    P["emb_task"].grad = None
    m = build_filled_model(swin, bert, B, cls=getattr(LA, cls)).eval()
    _check_rows_training(m, batch, g, P, 0, name)


@pytest.mark.parametrize("kind", ["task", "prompt"])
def test_forward_rows_with_pretext_against_fixtures(golden_dir, kind):
    import lavender_amd as LA
    from tests.helpers import build_filled_model
    g = np.load(os.path.join(golden_dir, f"pretxt_qaoe_{kind}.npz"))
    swin, bert, B, _, X = g["meta"].tolist()
    B, X = int(B), int(X)
    P, bc = _oracle_params(bert, swin)
    batch = make_batch(B, X=X, vocab=bc["vocab"], seed=6)
    txt = torch.from_numpy(g["txt"])
    batch.update(txt=txt, mask=(txt != 0).long(), mask_ans=torch.from_numpy(g["mask_ans"]))
    ids = torch.from_numpy(g["prompt"]).long() if kind == "prompt" else None
    prompt = (ids, torch.ones_like(ids)) if kind == "prompt" else None
    spec = ("task", 2) if kind == "task" else ("prompt", prompt)
    ref, ans_ref = PR.qa_forward(P, batch, swin, bc["heads"], spec)
    torch.nn.functional.cross_entropy(ref.flatten(0, 1), ans_ref.flatten(), ignore_index=-1).backward()
    if kind == "prompt":
        P["emb_task"].grad = None
    m = build_filled_model(swin, bert, B, cls=LA.LAVENDER_QAOE_MLM)
    m.args.enable_task_token, m.args.enable_prompt = kind == "task", kind == "prompt"
    m.eval()
    batch["task_name"], batch["prompt"] = ("oe", None) if kind == "task" else (None, prompt)
    Lp = 1 if kind == "task" else len(g["prompt"])
    _check_rows_training(m, batch, g, P, Lp, f"pretxt/{kind}")
    if kind == "task":
        ge = m.emb_task.grad.float().cpu()
        assert float(ge[[r for r in range(ge.shape[0]) if r != 2]].abs().max()) == 0.0
        assert ((ge[2] - P["emb_task"].grad[2]).norm() / P["emb_task"].grad[2].norm()).item() < 0.05


# ---- evaluation: the interval rule -------------------------------------------------------------------------------------------------------------
def _intervals(rows, labels, bound):
    """rows (n, V) float64 full-path logits of the labelled rows -> (rank_lo, rank_hi)"""
    xt = rows[np.arange(len(labels)), labels][:, None]
    return (rows > xt + bound).sum(1), (rows >= xt - bound).sum(1)


def _check_flags(flags, lo, hi, k):
    """flags of the rows path for top-k; returns the number of undetermined ones"""
    und = 0
    for f, l, h in zip(flags, lo, hi):
        if h < k:
            assert f == 1.0, (f, l, h, k)
        elif l >= k:
            assert f == 0.0, (f, l, h, k)
        else:
            und += 1
    return und


def _check_choice(choice, rows, cand, bound, tag=""):
    """the band of the module docstring; returns the per-row 'determined' mask and prints every margin"""
    p = rows[:, cand]
    s = p.sum(1)
    ds = len(cand) * bound
    det = np.zeros(len(choice), dtype=bool)
    for r in range(len(choice)):
        if abs(s[r]) <= ds:
            print(tag, "row", r, "sum", s[r], "within", ds, "of zero: undetermined")
            continue
        q = p[r] / s[r]
        qb = (bound + np.abs(q) * ds) / (abs(s[r]) - ds)
        best, got = int(q.argmax()), int(choice[r])
        others = [c for c in range(len(cand)) if c != best]
        margin = min((q[best] - qb[best]) - (q[c] + qb[c]) for c in others)
        det[r] = margin > 0
        print(tag, "row", r, "sum", round(float(s[r]), 4), "q", np.round(q, 4).tolist(), "qb", np.round(qb, 4).tolist(), "best", best, "got", got,
              "margin", round(float(margin), 4))
        assert q[got] + qb[got] >= q[best] - qb[best], (r, got, best, q.tolist(), qb.tolist())
        if det[r]:
            assert got == best, (r, got, best)
    return det


def _full_path(m, batch):
    with torch.no_grad():
        out, ans = m(_dev(batch, host_labels=False))
    return out.float().cpu(), ans.cpu()


@pytest.mark.parametrize("labels", ["one_each", "mixed"])
def test_answer_rows_against_the_full_path(golden_dir, labels):
    """one_each: the fixture's one [MASK] per sample (the last layer runs on those rows only); mixed: two labels in sample 0 and none in
    sample 1 (the full last layer, rows gathered)"""
    import lavender_amd as LA
    from lavender_amd.qa_mlm import label_rows
    from oracle import lavender_ref as R
    from tests.helpers import build_filled_model
    g = np.load(os.path.join(golden_dir, "qamc_micro_b3.npz"))
    swin, bert, B, S, heads, X = g["meta"].tolist()
    B, heads, X = int(B), int(heads), int(X)
    P, bc = _oracle_params(bert, swin)
    batch = make_batch(B, X=X, vocab=bc["vocab"], seed=6)
    batch["txt"] = torch.from_numpy(g["txt"]); batch["mask"] = (batch["txt"] != 0).long()
    ans = torch.from_numpy(g["mask_ans"]).clone()
    if labels == "mixed":
        p0 = int(torch.nonzero(ans[0] != -1)[0])
        ans[0, 2 if p0 != 2 else 3] = 1500
        ans[1] = -1
    batch["mask_ans"] = ans
    with torch.no_grad():
        ref, _ = R.qa_mlm_forward(P, batch, swin, heads)
    m = build_filled_model(swin, bert, B, cls=LA.LAVENDER_QAMC_MLM).eval()
    full, _ = _full_path(m, batch)
    e = (full - ref).abs().max().item()
    bound = 2 * e
    lr = label_rows(ans, 0)
    rows = full.flatten(0, 1)[lr.row].double().numpy()
    with torch.no_grad():
        pred, rank, choice = (t.cpu().numpy() for t in m.answer_rows(_dev(batch), cand=OPT_IDS))
    assert pred.shape == rank.shape == choice.shape == (len(lr.row),) and pred.dtype == np.int32
    lo, hi = _intervals(rows, lr.label, bound)
    print(labels, "e", e, "bound", bound, "rank", rank.tolist(), "lo", lo.tolist(), "hi", hi.tolist())
    assert ((lo <= rank) & (rank <= hi)).all()
    und = 0
    for k in (1, 5):
        und += _check_flags(((rank >= 0) & (rank < k)).astype(np.float32), lo, hi, k)
    assert (rows[np.arange(len(pred)), pred] >= rows.max(1) - bound).all()
    det = _check_choice(choice, rows, OPT_IDS, bound, labels)
    und += int((~det).sum())
    n_flags = 3 * len(lr.row)
    print(labels, "undetermined flags", und, "of", n_flags, "rank band sizes", (hi - lo).tolist())
    assert und * 4 <= n_flags


def _agent_batch(B=4, X=26, answers=(1016, 1014, 1018, 1015)):
    b = make_batch(B, X=X, vocab=BERT_CFGS["micro"]["vocab"], seed=6)
    ans = torch.full(b["txt"].shape, -1, dtype=torch.long)
    ans[:, -1] = torch.tensor(answers)                                  # make_batch ends every row with [MASK]
    b["mask_ans"] = ans
    b["ans_idx"] = torch.tensor([2, 0, 4, 1])
    return b


def _trained_oracle_error(m, b, full):
    """e of the interval rule on TRAINED weights: the oracle run on the model's own state dict"""
    from oracle import lavender_ref as R
    P = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    P["fc_mtm.predictions.decoder.bias"] = P["fc_mtm.predictions.bias"]
    with torch.no_grad():
        ref, _ = R.qa_mlm_forward(P, b, "micro", BERT_CFGS["micro"]["heads"])
    return (full - ref).abs().max().item()


class _DL(list):
    dataset = None


@pytest.mark.parametrize("kind", ["oe", "mc"])
def test_agents_with_qa_rows_train_and_evaluate(kind):
    """12 steps on a repeated batch whose four samples share ONE answer (token 1016 = option 2), so that after training the answer stands clear
    of every other token and the evaluation flags are determined; the evaluation batch then asks each sample for a different answer
    (1016, 1014, 1018, 1015 / options 2, 0, 4, 1), so the expected flags are not all alike.  Seeds: set_seed for the weights and hip.reseed
    for the dropout counter, which set_seed does not touch -- the trained weights do not depend on what ran earlier in the process."""
    import lavender_amd as LA
    from lavender_amd import hip as K
    from lavender_amd.dist import set_seed
    from lavender_amd.qa_mlm import label_rows
    from oracle import lavender_ref as R
    from tests.helpers import Tok, make_args
    set_seed(88)
    K.reseed(88)
    B, X = 4, 26
    bt = _agent_batch(B, X, answers=(1016, 1016, 1016, 1016))
    b = _agent_batch(B, X)
    # multiple choice with TWO options (tokens 1014, 1016): with five, the four untrained option logits tie within the band and -- the sum of
    # the raw logits being negative after training (measured -2.96) -- decide the reversed order among themselves: 4 of 4 rows undetermined.
    # Two options leave one trained and one untrained logit, a quotient margin far outside the band.
    opts = [1014, 1016]
    if kind == "mc":
        b = _agent_batch(B, X, answers=(1016, 1014, 1016, 1014))
        b["ans_idx"] = torch.tensor([1, 0, 1, 0])
    args = make_args("micro", "micro", B, lr=2e-3, max_iter=40, size_vocab=-1, size_option=5 if kind == "oe" else 2, qa_rows=True)
    m = (LA.LAVENDER_QAOE_MLM if kind == "oe" else LA.LAVENDER_QAMC_MLM)(args, Tok()).cuda()
    m.arena()
    ag = LA.Agent_QAOE_MLM(args, m) if kind == "oe" else LA.Agent_QAMC_MLM(args, m, opts)
    losses = []
    for _ in range(12):
        prepared = ag.prepare_batch(dict(bt))
        assert prepared["_lab_host"] is bt["mask_ans"]
        r = ag.step(prepared, True)
        losses.append(r["ls"] if kind == "oe" else r)
    print(kind, "rows losses", [round(x, 3) for x in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] - 1.0
    ev = ag.step(ag.prepare_batch(dict(b)), False)
    m.eval()
    full, a = _full_path(m, b)
    e = _trained_oracle_error(m, b, full)
    bound = 2 * e
    lr = label_rows(b["mask_ans"], 0)
    rows = full.flatten(0, 1)[lr.row].double().numpy()
    lo, hi = _intervals(rows, lr.label, bound)
    print(kind, "e", e, "bound", bound, "rank lo", lo.tolist(), "hi", hi.tolist(), "ev", ev)
    if kind == "oe":
        assert set(ev) == {"ac_1", "ac_5"} and all(isinstance(v, list) and len(v) == B for v in ev.values())
        und = 0
        for k in (1, 5):
            want = R.qa_top_k_acc(full, b["mask_ans"], k)
            und_k = _check_flags(ev[f"ac_{k}"], lo, hi, k)
            und += und_k
            if und_k == 0:
                assert ev[f"ac_{k}"] == want
        print("oe undetermined", und, "of", 2 * B)
        assert und * 4 <= 2 * B
        assert all(t5 >= t1 for t1, t5 in zip(ev["ac_1"], ev["ac_5"]))
        # one unlabelled sample: its hits come last as zero (get_top_k_acc's padding)
        b2 = dict(b)
        b2["mask_ans"] = b["mask_ans"].clone()
        b2["mask_ans"][1] = -1
        ev2 = ag.step(ag.prepare_batch(dict(b2)), False)
        assert len(ev2["ac_1"]) == B and len(ev2["ac_5"]) == B and ev2["ac_1"][-1] == 0.0 and ev2["ac_5"][-1] == 0.0
        keep = [0, 2, 3]
        for k in (1, 5):
            _check_flags(ev2[f"ac_{k}"][:3], lo[keep], hi[keep], k)
        # more labelled rows than samples (two labels in sample 2): one flag per labelled row, as get_top_k_acc returns them
        b4 = dict(b)
        b4["mask_ans"] = b["mask_ans"].clone()
        b4["mask_ans"][2, 3] = 1500
        ev4 = ag.step(ag.prepare_batch(dict(b4)), False)
        assert len(ev4["ac_1"]) == B + 1 and len(ev4["ac_5"]) == B + 1
        lr4 = label_rows(b4["mask_ans"], 0)
        lo4, hi4 = _intervals(_full_path(m, b4)[0].flatten(0, 1)[lr4.row].double().numpy(), lr4.label, bound)
        for k in (1, 5):
            _check_flags(ev4[f"ac_{k}"], lo4, hi4, k)
        # go_dl in evaluation: the averages of the same rows-path flags (ev, ev2 come from step on the same weights), copied once after the loader
        res = ag.go_dl(1, _DL([dict(b), dict(b2)]), False)
        assert abs(res["ac_1"] - np.average(ev["ac_1"] + ev2["ac_1"])) < 1e-6 and abs(res["ac_5"] - np.average(ev["ac_5"] + ev2["ac_5"])) < 1e-6
        assert ag.go_dl(1, _DL([]), False) == {}
    else:
        assert isinstance(ev, list) and len(ev) == B and set(ev) <= {0.0, 1.0}
        want = R.qamc_choice_acc(full, b["mask_ans"], opts, b["ans_idx"])
        with torch.no_grad():
            choice = m.answer_rows(_dev(b), cand=opts)[2].cpu().numpy()
        det = _check_choice(choice, rows, opts, bound, "mc")
        print("mc undetermined", int((~det).sum()), "of", B, "ev", ev, "full path", want)
        assert int((~det).sum()) * 4 <= B
        assert all(ev[i] == want[i] for i in range(B) if det[i])
        assert ev == (choice == b["ans_idx"].numpy()).astype(np.float32).tolist()
        # go_dl: the average of the same rows-path flags, copied once after the loader; an empty loader gives the existing path's NaN
        assert abs(ag.go_dl(1, _DL([dict(b), dict(b)]), False) - np.average(ev)) < 1e-6
        with pytest.warns(RuntimeWarning):
            assert np.isnan(ag.go_dl(1, _DL([]), False))
        b3 = dict(b)
        b3["mask_ans"] = b["mask_ans"].clone()
        b3["mask_ans"][2, 3] = 1015                                    # two labels in one sample
        for is_train in (False, True):
            with pytest.raises(ValueError, match="exactly one"):
                ag.step(ag.prepare_batch(dict(b3)), is_train)


class _Recorder:
    """pass-through around an agent's loss_func that keeps a copy of what it was given (the loss kernel overwrites the logits in training)"""

    def __init__(self, inner):
        self.inner, self.seen = inner, []

    def __call__(self, logits, labels, count=None):
        self.seen.append((logits.detach().clone(), labels.detach().clone(), count))
        return self.inner(logits, labels, count)


@pytest.mark.parametrize("kind", ["oe", "mc"])
def test_default_step_is_bit_identical_to_the_existing_path(kind):
    """qa_rows unset: step() runs the code it ran before.  Two identically seeded models; one goes through step(), the other through a direct
    call of that code (forward_step on the whole batch, loss_func over all B * X rows with the host's label count, the reference's read-out).
    Bit for bit equal: the evaluation results, and the (B * X, V) training logits (dropout on), labels and count that reach the loss.
    The loss VALUE is compared to (n_lab - 1) ulp instead: lav_cross_entropy_fwd_bwd adds the row losses with atomics, so the fp32 order of that
    sum of n_lab terms is not fixed from run to run even on unchanged code (on an MI355X two identically seeded runs of this very comparison,
    both through the unchanged full path, once returned 9.0667725 and 9.0667734, 1 ulp apart, and were equal on other runs); each reordering of a sum of n positive terms moves it by at most n - 1 roundings."""
    import lavender_amd as LA
    from lavender_amd.dist import set_seed
    from lavender_amd import hip as K
    from oracle import lavender_ref as R
    from tests.helpers import Tok, make_args
    B, X = 4, 26
    b = _agent_batch(B, X)
    res = []
    for direct in (False, True):
        set_seed(88)
        K.reseed(88)
        args = make_args("micro", "micro", B, lr=2e-3, max_iter=40, size_vocab=-1, size_option=5)
        assert "qa_rows" not in args
        m = (LA.LAVENDER_QAOE_MLM if kind == "oe" else LA.LAVENDER_QAMC_MLM)(args, Tok()).cuda()
        m.arena()
        ag = LA.Agent_QAOE_MLM(args, m) if kind == "oe" else LA.Agent_QAMC_MLM(args, m, OPT_IDS)
        ag.loss_func = _Recorder(ag.loss_func)
        batch = ag.prepare_batch(dict(b))
        assert "_lab_host" not in batch
        if not direct:
            ev = ag.step(batch, False)
        else:
            ag._set_mode(False)
            batch.pop("_n_lab")
            with torch.no_grad():
                out, ans = ag.forward_step(batch)
            out, ans = out.float().cpu(), ans.cpu()
            ev = ({"ac_1": R.qa_top_k_acc(out, ans, 1), "ac_5": R.qa_top_k_acc(out, ans, 5)} if kind == "oe"
                  else R.qamc_choice_acc(out, ans, OPT_IDS, b["ans_idx"]))
        batch = ag.prepare_batch(dict(b))
        if not direct:
            r = ag.step(batch, True)
            loss = r["ls"] if kind == "oe" else r
        else:
            ag._set_mode(True)
            n_lab = batch.pop("_n_lab")
            out, ans = ag.forward_step(batch)
            ls = ag.loss_func(out.flatten(0, 1), ans.flatten(), n_lab)
            ag.backward_step(ls)
            loss = ls.item()
        assert len(ag.loss_func.seen) == 1
        res.append((ev, ag.loss_func.seen[0], loss))
    (ev0, (lg0, lb0, c0), l0), (ev1, (lg1, lb1, c1), l1) = res
    print(kind, "default eval", ev0, "losses", l0, l1)
    assert ev0 == ev1
    assert lg0.shape == (B * X, BERT_CFGS["micro"]["vocab"]) and c0 == c1 == B
    assert torch.equal(lg0, lg1) and torch.equal(lb0, lb1)
    assert abs(l0 - l1) <= (B - 1) * float(np.spacing(np.float32(max(l0, l1))))
