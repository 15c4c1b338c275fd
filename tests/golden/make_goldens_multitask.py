"""Golden vectors of multi-task MLM fine-tuning (CONTAINER ONLY -- needs the reference checkout): LAVENDER_Multi_Task, Agent_Multi_Task
(main_multi_task_mlm.py:78-486) and MetaLoader (dataset.py:702-748), run from the reference's own code on the CPU.  Same recipe and third-party
stubs as make_goldens_qa.py / make_goldens_caption_train.py; one more name is supplied in memory: main_multi_task_mlm.py imports
Dataset_QAOE_LSMDC_TSV from main_qaoe_mlm_lsmdc_fib.py, which defines that dataset as Dataset_QAOE_MLM_LSMDC (no dataset is used here).
Writes multitask_micro.npz next to this file -- ONE weight set (the key-seeded fill of the oracle), five tasks of different geometry:

    captioning_x    B 2, T 4, X 20        retrieval_x   B 3 (9 pairs), T 2, X 26        qamc_x   B 3, T 4, X 41
    qamc_lsmdc-mc   B 2, O 3, T 2, X 26   qaoe_x        B 3, T 6, X 26

  * per task: the inputs that are not regenerated from a seed (txt, labels), forward()'s logits at a column subset (the "true" / "false" and
    option-index columns first), their logsumexp, the labels it returns and the training loss of Agent_Multi_Task's loss functions on them;
  * eval_step's flags of qamc_x and qaoe_x.  The script asserts that each of them, and every training row's arg-max hit, is decided by a margin
    larger than what an error of ATOL (the tolerance of the full-path GPU tests on this configuration) on every logit could overturn; a draw
    that does not satisfy this is replaced by changing its seed below;
  * NO flags of retrieval_x and qamc_lsmdc-mc.  Their flags are arg-maxima of t / (t + f) on RAW logits.  With this weight set both logits lie
    within 0.2 of zero and the candidates of a group differ by about 1e-3, thirty times less than ATOL, so no draw of inputs has a flag that
    such an error could not overturn: the script prints the error the flags of this draw do survive (below 1e-3) and records none of them.  The
    GPU tests check these two tasks' flags against the numpy restatement of lav_match_readout applied to the logits the model itself produced;
  * ten Agent_Multi_Task.train_step calls, the five tasks twice in the order above (stochastic modules set to p = 0 on the MODULES): ls and ac
    per step, the learning rates, every parameter's total update norm and sub-samples of a few updates;
  * 50 draws of MetaLoader after random.seed(88) over three pools with ratios 1 / 2 / 1.

    python tests/golden/make_goldens_multitask.py
"""
import sys
sys.dont_write_bytecode = True
import importlib
import os
import random

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG  # noqa: E402
from make_goldens import R, make_batch, sub, BERT_CFGS  # noqa: E402
from make_goldens_variants import build  # noqa: E402
from make_goldens_caption_train import import_caption_modules  # noqa: E402
from make_goldens_qa import ANS_TOK_IDS, qa_batch  # noqa: E402
from make_goldens_agent import PICK  # noqa: E402

ATOL = 3e-2                                        # tests/test_gpu_qa.py: logits of the full path on the micro configuration
TRUE, FALSE = 2995, 6270
ORDER = ["captioning_x", "retrieval_x", "qamc_x", "qamc_lsmdc-mc", "qaoe_x"]
SEEDS = {"captioning_x": 21, "retrieval_x": 64, "qamc_x": 23, "qamc_lsmdc-mc": 108, "qaoe_x": 25}
N_COLS = 128


def make_task_batch(task, vocab, MAIN):
    """the batch of a task as its dataset's collate function would deliver it (host tensors), seeded by SEEDS[task]"""
    s = SEEDS[task]
    if task == "captioning_x":
        b = make_batch(2, T=4, X=20, vocab=vocab, seed=s)
        b["txt"][:, -1] = 0                                    # a caption ends in [SEP] [PAD]..., not in make_batch's trailing [MASK]
        b["mask"] = (b["txt"] != 0).long()
        torch.manual_seed(s)
        me = type("A", (), {"pad_token_id": 0, "mask_token_id": 103})()
        b.update(MAIN.Agent_Captioning.masking(me, b["txt"], p_mask=0.3))
        return b
    if task == "retrieval_x":
        b = make_batch(3, T=2, X=26, vocab=vocab, seed=s)     # every text ends with the appended [MASK]
        b["vid"] = [7, 3, 5]
        return b
    if task == "qamc_x":
        b = qa_batch(3, 41, vocab, s, [1016, 1014, 1018])
        b["img"] = make_batch(3, T=4, vocab=vocab, seed=s)["img"]
        b["ans_idx"] = torch.tensor([2, 0, 4])
        return b
    if task == "qamc_lsmdc-mc":
        B, O, X = 2, 3, 26
        txt = make_batch(B * O, T=1, S=32, X=X, vocab=vocab, seed=s)["txt"].view(B, O, X)
        ans = torch.full(txt.shape, -1, dtype=torch.long)
        ans[:, :, -1] = torch.tensor([[FALSE, TRUE, FALSE], [FALSE, FALSE, TRUE]])
        return {"img": make_batch(B, T=2, vocab=vocab, seed=s + 100)["img"], "txt": txt, "mask": (txt != 0).long(), "mask_ans": ans}
    b = qa_batch(3, 26, vocab, s, [2023, 3899, 2158])
    b["img"] = make_batch(3, T=6, vocab=vocab, seed=s)["img"]
    return b


def clone(b):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def top1_margin_ok(logits, labels):
    """every labelled row's arg-max hit survives a +-ATOL error on every logit: the label is ahead of, or behind, the best other column by > 2 ATOL"""
    x, a = logits.detach().flatten(0, logits.dim() - 2).double(), labels.flatten()
    keep = a != -1
    x, a = x[keep], a[keep]
    own = x.gather(1, a.view(-1, 1)).squeeze(1)
    other = x.scatter(1, a.view(-1, 1), -float("inf")).max(1).values
    return bool(((own - other).abs() > 2 * ATOL).all()), float((own - other).abs().min()) if len(a) else float("inf")


def rank_margin_ok(logits, labels, k):
    """the top-k flag of every labelled row survives: the label's logit is > 2 ATOL away from the k-th best other column"""
    x, a = logits.detach().flatten(0, 1).double(), labels.flatten()
    keep = a != -1
    x, a = x[keep], a[keep]
    own = x.gather(1, a.view(-1, 1)).squeeze(1)
    kth = x.scatter(1, a.view(-1, 1), -float("inf")).topk(k, dim=1).values[:, -1]
    return bool(((own - kth).abs() > 2 * ATOL).all())


def ratio_margin_ok(t, f, G, O, ATOL=ATOL):
    """arg-max of t / (t + f) over each group survives: with every logit anywhere within +-ATOL the denominators keep their sign and the
    winner's lowest quotient stays above every other candidate's highest"""
    t, f = t.detach().double().view(G, O), f.detach().double().view(G, O)
    lo, hi = None, None
    for dt in (-ATOL, ATOL):
        for df in (-ATOL, ATOL):
            q = (t + dt) / (t + dt + f + df)
            lo, hi = (q, q) if lo is None else (torch.minimum(lo, q), torch.maximum(hi, q))
    if not bool(((t + f).abs() > 2 * ATOL).all()):
        return False
    win = (t / (t + f)).argmax(1)
    ok = True
    for g in range(G):
        others = [o for o in range(O) if o != int(win[g])]
        ok = ok and all(lo[g, win[g]] > hi[g, o] for o in others)
    return ok


def ratio_tolerated(t, f, G, O):
    """the largest logit error (up to ATOL, by bisection) under which ratio_margin_ok still holds"""
    if ratio_margin_ok(t, f, G, O):
        return ATOL
    lo, hi = 0.0, ATOL
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if ratio_margin_ok(t, f, G, O, mid) else (lo, mid)
    return lo


def share_margin_ok(x, G):
    """arg-max of x_c / sum_c x_c (qamc): the sum keeps its sign (|sum| > n ATOL) and the winning candidate is > 2 ATOL from the runner-up"""
    x = x.detach().double().view(G, -1)
    s = x.sum(1)
    if not bool((s.abs() > x.shape[1] * ATOL).all()):
        return False
    y = torch.where(s.view(-1, 1) > 0, x, -x).sort(1, descending=True).values
    return bool(((y[:, 0] - y[:, 1]) > 2 * ATOL).all())


def main():
    MAIN, _ = import_caption_modules()
    fib = importlib.import_module("main_qaoe_mlm_lsmdc_fib")
    if not hasattr(fib, "Dataset_QAOE_LSMDC_TSV"):
        fib.Dataset_QAOE_LSMDC_TSV = fib.Dataset_QAOE_MLM_LSMDC
    MT = importlib.import_module("main_multi_task_mlm")
    ref = MG.import_reference()
    swin, bert = "micro", "micro"
    vocab, heads = BERT_CFGS[bert]["vocab_size"], BERT_CFGS[bert]["num_attention_heads"]
    m, keys = build(ref, MT.LAVENDER_Multi_Task, swin, bert, 3, size_vocab=-1, size_option=5)
    m.args.update(lr=2e-5, decay=1e-3, max_iter=20, max_grad_norm=1.0, deepspeed=False, vis_backbone_lr_mul=1, dataset=["x"], logging_steps=10,
                  path_output="/tmp/lav_golden/out", task="multi_task", label_smoothing=0.0, drop_worst_ratio=0.0, distributed=False)
    # label_smoothing 0: the reference reads its loss config with getattr from a plain dict (main_multi_task_mlm.py:231-236,
    # model_for_captioning.py:13-15), so it always trains with 0 whatever args say; lavender_amd honours the keys, and 0 is where both agree
    n_drop = 0
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
            n_drop += 1
        if type(mod).__name__ == "DropPath":
            mod.drop_prob = 0.0
            n_drop += 1
    wrapped = m.trsfr
    m.trsfr = wrapped.enc                                  # the Agent's group rules match unwrapped names
    ag = MT.Agent_Multi_Task(m.args, m, mc_ans_tok_ids=ANS_TOK_IDS)
    m.trsfr = wrapped
    res = {"order": np.array(ORDER), "n_neutralised": np.array(n_drop), "ans_tok_ids": np.array(ANS_TOK_IDS),
           "meta": np.array([swin, bert, str(heads), str(ATOL)])}
    cols = torch.cat([torch.tensor([TRUE, FALSE] + ANS_TOK_IDS), torch.randperm(vocab, generator=torch.Generator().manual_seed(5))[:N_COLS - 7]])
    res["cols"] = cols.numpy()
    for t in ("retrieval_x", "qamc_lsmdc-mc"):
        res[f"{t}::seed"] = np.array(SEEDS[t])
    batches = {t: make_task_batch(t, vocab, MAIN) for t in ORDER}

    # ---- forward and evaluation flags at the filled weights ------------------------------------------------------------------------------
    m.eval()
    for t in ORDER:
        b = clone(batches[t])
        b["task"] = t
        for k in ("txt", "ans_mtm", "mask_ans", "ans_idx"):
            if k in b:
                res[f"{t}::{k}"] = b[k].numpy().copy()
        if "vid" in b:
            res[f"{t}::vid"] = np.array(b["vid"])
        with torch.no_grad():
            o = m(clone(b))
        out, ans = o["out"], o["ans"]
        flat, lab = out.flatten(0, out.dim() - 2), ans.flatten()
        if "captioning" in t:
            ls = ag.cap_loss_func(flat[lab != -1].float(), lab[lab != -1])
            ag.cap_loss_func.iter = 0
        else:
            ls = ag.loss_func(flat, lab)
        res[f"{t}::ans"] = ans.numpy().copy()
        res[f"{t}::out_cols"] = out[..., cols].numpy().astype(np.float32)
        res[f"{t}::out_lse"] = torch.logsumexp(out, -1).numpy()
        res[f"{t}::loss"] = np.array([ls.item()])
        line = f"   {t}: logits {tuple(out.shape)} labels {int((lab != -1).sum())} loss {ls.item():.4f}"
        if "retrieval" in t or "lsmdc-mc" in t:
            with torch.no_grad():
                flags = ag.eval_step(clone(b))
            keep = lab != -1
            tol = ratio_tolerated(flat[keep][:, TRUE], flat[keep][:, FALSE], len(flags["ac"]), int(keep.sum()) // len(flags["ac"]))
            line += f" flags {flags} survive a logit error of {tol:.2e} (tolerance {ATOL}): not recorded"
            assert tol < ATOL, f"{t}: this draw's flags ARE decided outside the tolerance: record them"
        elif "captioning" not in t:
            with torch.no_grad():
                flags = ag.eval_step(clone(b))
            for k, v in flags.items():
                res[f"{t}::flag_{k}"] = np.array(v, dtype=np.float32)
            if "qamc" in t:
                ok = share_margin_ok(flat[lab != -1][:, ANS_TOK_IDS], out.shape[0])
            else:
                ok = rank_margin_ok(out, ans, 1) and rank_margin_ok(out, ans, 5)
            assert ok, f"{t}: an evaluation flag is decided inside the logit tolerance {ATOL}: change SEEDS[{t!r}]"
            line += f" flags {flags}"
        print(line)

    # ---- ten training steps ------------------------------------------------------------------------------------------------------------------
    unwrap = lambda k: k.replace("trsfr.enc.", "trsfr.")
    before = {unwrap(k): p.detach().clone() for k, p in m.named_parameters()}
    seen = {}
    fwd = ag.forward_step
    ag.forward_step = lambda batch: seen.__setitem__("out", fwd(batch)) or seen["out"]
    ls_all, ac_all, lrs = [], [], []
    for step, t in enumerate(ORDER + ORDER):
        b = clone(batches[t])
        b["task"] = t
        r = ag.train_step(b)
        ok, margin = top1_margin_ok(seen["out"]["out"], seen["out"]["ans"])
        assert ok, f"step {step} ({t}): a labelled row's top-1 margin {margin:.3e} is inside the logit tolerance: change SEEDS[{t!r}]"
        ls_all.append(r["ls"]); ac_all.append(r["ac"]); lrs.append([g["lr"] for g in ag.optzr.param_groups])
        print(f"   step {step} {t}: ls {r['ls']:.5f} ac {r['ac']:.4f} lr {lrs[-1][1]:.3e} smallest top-1 margin {margin:.3f}")
    after = {unwrap(k): p.detach().clone() for k, p in m.named_parameters()}
    res["train_ls"], res["train_ac"], res["train_lrs"] = np.array(ls_all), np.array(ac_all, dtype=np.float64), np.array(lrs)
    res["delta_keys"] = np.array(list(after.keys()))
    res["delta_norms"] = np.array([(after[k] - before[k]).double().norm().item() for k in after])
    for k in PICK:
        res[f"delta_sub::{k}"] = sub(after[k] - before[k], 2048)

    # ---- MetaLoader ------------------------------------------------------------------------------------------------------------------------------
    loaders = {"a": ([("a", i) for i in range(3)], 1), "b": ([("b", i) for i in range(2)], 2), "c": ([("c", i) for i in range(4)], 1)}
    random.seed(88)
    ml = MT.MetaLoader(loaders)
    draws = []
    for i, (task, batch) in enumerate(ml):
        draws.append(f"{task}:{batch[1]}")
        if i == 49:
            break
    res["meta_draws"] = np.array(draws)
    path = f"{HERE}/multitask_micro.npz"
    np.savez_compressed(path, **res)
    print("written", path, os.path.getsize(path), "bytes;", n_drop, "stochastic modules neutralised; draws", draws[:12])


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
