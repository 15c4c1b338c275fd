"""LAVENDER_Multi_Task / Agent_Multi_Task / MetaLoader -- mirror of the reference's main_multi_task_mlm.py:78-486 and dataset.py:702-748.

One model answers every downstream task through the one MLM head, so one optimizer loop can fine-tune on all of them: each step the MetaLoader
draws a task, and the batch of that task runs through the forward of its single-task caller -- the same methods, shared as mixins
(captioning.LAVENDER_Captioning, qa_mlm.QAForwardMixin, retrieval_mlm.RetrievalPairsMixin), so the logits are the bits those callers produce.
Geometry (B, T, X, pair count, mask type) changes from one step to the next on one arena and one optimizer.

Rows paths (args.mt_rows): training runs the MLM head on the labelled rows only (forward_rows, engine.RowGatherFn) for all five task
types; evaluation of qaoe / qamc is answer_rows (qa_mlm), evaluation of retrieval / lsmdc-mc runs the last fusion layer and the head on the one
[MASK] row per pair (pair_source / score_pairs) and reads choice and hit out on the device (lav_match_readout).  With mt_rows off the agent
evaluates the reference's formulation -- the full (pairs, X, vocab) logits -- and reads the same kernels' outputs from it through a row map."""
import json
import random
from collections import defaultdict

import numpy as np
import torch

from . import hip as K
from .agent import Agent_Base
from .captioning import Agent_Captioning, CaptioningLoss, LAVENDER_Captioning, RunningMeter, _all_gather_objects
from .dist import is_main_process
from .qa_mlm import QAForwardMixin, _pad_hits, label_rows
from .retrieval_mlm import RetrievalPairsMixin, all_pairs

TASK_KINDS = ("captioning", "retrieval", "qamc_ret", "qamc", "qaoe")


def task_kind(task):
    """the forward a task name selects, by substring in the reference's order (main_multi_task_mlm.py:86-99): captioning, retrieval, qamc (with
    lsmdc-mc inside it: the RetMC forward), qaoe; anything else raises as the reference's forward does"""
    if "captioning" in task:
        return "captioning"
    if "retrieval" in task:
        return "retrieval"
    if "qamc" in task:
        return "qamc_ret" if "lsmdc-mc" in task else "qamc"
    if "qaoe" in task:
        return "qaoe"
    raise NotImplementedError(f"forward() for {task}")


def task_token_of(task):
    """main_multi_task_mlm.py:262-274"""
    if 'retrieval' in task:
        return "vtm"
    if 'qamc' in task:
        return "vtm" if 'lsmdc-mc' in task else "mc"
    if 'qaoe' in task:
        return "oe"
    if 'captioning' in task:
        return "cap"
    raise NotImplementedError(f"no task name for {task}")


def best_metric_of(task):
    """the metric of the closing "Best ..." lines (main_multi_task_mlm.py:456-462)"""
    return 'CIDEr' if 'captioning' in task else ('ac_1' if 'qaoe' in task else 'ac')


def _rows_2d(out):
    """the (pairs * X, vocab) view of (pairs, X, vocab) logits, row stride kept (the head's buffer is row-padded)"""
    n, X, V = out.shape
    if out.stride(2) != 1 or out.stride(0) != X * out.stride(1):
        out = out.contiguous()
    return out.as_strided((n * X, V), (out.stride(1), 1))


class LAVENDER_Multi_Task(QAForwardMixin, RetrievalPairsMixin, LAVENDER_Captioning):
    """main_multi_task_mlm.py:78-225.  The pre-text positions of every task are labelled -1 (QAForwardMixin.prepro_pretxt; the reference's
    `ans[:, :_L] = -1`, which the captioning forward applies itself)."""

    def __init__(self, args, tokzr, is_decoder=True):
        super().__init__(args, tokzr, is_decoder)

    def forward(self, batch, is_decode=False):
        batch = defaultdict(lambda: None, batch)
        task = batch["task"]
        kind = task_kind(task)
        batch["attn_mask_type"] = "seq2seq" if kind == "captioning" else "full"
        if kind == "captioning":
            if batch["_mt_rows"] and not is_decode:
                return self.forward_rows(batch)
            return self.forward_captioning(batch, is_decode=is_decode)
        if batch["_mt_rows"]:
            return self.forward_rows(batch)
        out = getattr(self, "forward_" + kind)(batch)
        return {"out": out[0], "ans": out[1]}

    def forward_captioning(self, batch, is_decode=False):
        return LAVENDER_Captioning.forward(self, batch, is_decode=is_decode)

    def forward_retrieval(self, batch):
        return self.retrieval_forward(batch)

    def forward_qamc_ret(self, batch):
        return self.retmc_forward(batch)

    def forward_qamc(self, batch):
        return self.qa_forward(batch)

    def forward_qaoe(self, batch):
        return self.qa_forward(batch)

    # ---- rows paths (args.mt_rows) ----------------------------------------------------------------------------------------------------------
    def forward_rows(self, batch):
        """forward with the MLM head on the labelled rows only: {"out": (n_lab, V) logits, "ans": (n_lab,) labels}, rows in the order of
        `ans[ans != -1]`, for every task type.  Which rows carry a label comes from the host copy of the labels the agent keeps (captioning:
        batch["_ans_mtm_cpu"]; qaoe / qamc / lsmdc-mc: batch["_lab_host"]; retrieval: the last text position of every pair, labelled from
        batch["vid"]); a batch without that copy takes forward() and is flattened.  The whole last fusion layer runs: its backward needs every row."""
        batch = defaultdict(lambda: None, batch)
        kind = task_kind(batch["task"])
        batch["attn_mask_type"] = "seq2seq" if kind == "captioning" else "full"
        if kind == "captioning":
            if batch["_ans_mtm_cpu"] is not None:
                return self.encode_forward_rows(batch)
        elif kind == "retrieval":
            out = self.retrieval_forward(batch, rows=True)
            return {"out": out[0], "ans": out[1]}
        elif batch["_lab_host"] is not None and bool((batch["_lab_host"] != -1).any()):
            out = self.retmc_forward(batch, rows=True) if kind == "qamc_ret" else self.qa_forward_rows(batch)
            return {"out": out[0], "ans": out[1]}
        full = self.forward({k: v for k, v in batch.items() if k != "_mt_rows"})
        return {"out": full["out"].flatten(0, full["out"].dim() - 2), "ans": full["ans"].flatten()}

    def match_groups(self, batch):
        """(G, O, vi, ti, gt) of an in-batch matching evaluation: retrieval scores all B x B (video i, text j) pairs and video i's group holds
        the B texts, gt = the text of the same `vid` (main_retrieval_mlm.py:107-118); lsmdc-mc scores (video i, text i * O + o) and gt is the
        candidate labelled "true" (main_retmc_mlm.py:129-140; the host labels batch["_lab_host"] (B, O, X)).  Exactly one candidate of every
        group must be the true one, as the reference's nonzero()[:, 1] needs: ValueError otherwise."""
        if task_kind(batch["task"]) == "retrieval":
            vid = batch["vid"]
            vid = list(vid.tolist()) if isinstance(vid, torch.Tensor) else list(vid)
            B = len(vid)
            same = np.array([[vid[i] == vid[j] for j in range(B)] for i in range(B)])
            vi, ti = all_pairs(B)
            G, O = B, B
        else:
            lab = batch["_lab_host"]
            if lab is None:
                raise ValueError("match_groups: the batch has no host copy of its labels (Agent_Multi_Task.prepare_batch)")
            G, O, _ = lab.shape
            same = (lab.numpy() == int(self.true_token_id)).any(-1)
            vi, ti = np.repeat(np.arange(G), O), np.arange(G * O)
        if not bool((same.sum(1) == 1).all()):
            raise ValueError(f"{batch['task']}: every group needs exactly one true candidate, got {same.sum(1).tolist()}")
        return G, O, vi, ti, same.argmax(1).astype(np.int32)

    def match_rows(self, batch):
        """In-batch matching evaluation of retrieval / lsmdc-mc on the [MASK] rows (eval mode, under no_grad): device int32 (choice (G,), hit (G,)).
        Layers 0 .. n-2 run through the pair map, the last layer and the two-column head on the one [MASK] row per pair (pair_source /
        score_pairs on the batch's own features), lav_match_readout on the (pairs, 2) block.  Needs the host copy of the text
        (batch["_txt_host"]).  Returns None where that path does not apply -- a one-layer encoder, head_dim != 64, a text whose labelled position
        is not its one [MASK] -- and the caller evaluates the full logits (match_full)."""
        if torch.is_grad_enabled() or self.training:
            raise RuntimeError("match_rows is evaluation only: call model.eval() and run it under torch.no_grad()")
        batch = defaultdict(lambda: None, batch)
        layers = self.trsfr.layer
        host_txt = batch["_txt_host"]
        if host_txt is None or len(layers) < 2 or self.hidden_size != 64 * layers[-1].num_heads:
            return None
        G, O, vi, ti, gt = self.match_groups(batch)
        X = host_txt.shape[-1]
        host_txt = host_txt.reshape(-1, X)
        if task_kind(batch["task"]) == "retrieval":
            pos = np.full(host_txt.shape[0], X - 1)                # the reference labels the last text position of every pair
        else:
            lr = label_rows(batch["_lab_host"].reshape(-1, X))
            if len(lr.sample) != host_txt.shape[0] or not bool((lr.sample == np.arange(host_txt.shape[0])).all()):
                return None
            pos = lr.pos
        is_mask = host_txt.numpy() == int(self.mask_token_id)
        if not bool((is_mask.sum(1) == 1).all()) or not bool(is_mask[np.arange(len(pos)), pos].all()):
            return None
        img, txt, mask = batch["img"], batch["txt"], batch["mask"]
        task_name, prompt = batch["task_name"], batch["prompt"]
        txt, mask = txt.reshape(-1, X), mask.reshape(-1, X)
        feat_img, mask_img, feat_txt, mask_txt = self.go_feat(img, txt, mask, task_name=task_name, prompt=prompt)
        _, mask_txt, feat_txt = self.prepro_txt_inputs(txt, mask_txt, feat_txt, task_name=task_name, prompt=prompt)
        Lp = feat_txt.shape[1] - X
        host_full = torch.cat([torch.full((host_txt.shape[0], Lp), -1, dtype=host_txt.dtype), host_txt], 1)
        src = self.pair_source(feat_img, mask_img, feat_txt, mask_txt, host_full)
        logits = torch.empty((len(vi), 2), dtype=torch.float32, device=feat_img.device)
        self.score_pairs(src, vi, ti, logits=logits)
        choice, hit, _ = K.match_readout(logits, G, O, 0, 1, gt=gt)
        return choice, hit

    def match_full(self, batch, out):
        """the same read-out from the reference's formulation: `out` the (pairs, Lp + X, vocab) logits of forward(), read at the labelled row of
        every pair and the "true" / "false" columns through lav_match_readout's row map"""
        G, O, _, _, gt = self.match_groups(batch)
        n, Xf, _ = out.shape
        if task_kind(batch["task"]) == "retrieval":
            pos = np.full(n, Xf - 1)
        else:
            lab = batch["_lab_host"]
            lr = label_rows(lab.reshape(-1, lab.shape[-1]), Xf - lab.shape[-1])
            if len(lr.sample) != n or not bool((lr.sample == np.arange(n)).all()):
                raise ValueError(f"{batch['task']}: every candidate text needs exactly one labelled position")
            pos = lr.row - lr.sample * lr.width
        choice, hit, _ = K.match_readout(_rows_2d(out), G, O, int(self.true_token_id), int(self.false_token_id), row=np.arange(n) * Xf + pos, gt=gt)
        return choice, hit


class MetaLoader:
    """dataset.py:702-748: wraps several data loaders and yields (task, batch) for ever.  loaders: {name: loader or (loader, ratio)}; every name
    enters the sampling pool `ratio` times; whenever step % accum_steps == 0 the task is drawn with random.choice (Python's `random`: seed it
    for a reproducible order); an exhausted loader is restarted.

    EVERY RANK MUST RUN THE SAME TASK IN A STEP: the gradient exchange reduces the same arena slices on all ranks and the first-touch units
    are filled by what a step runs, so a rank on another task would exchange gradients of parameters it did not touch (and the sequence
    shapes of the ranks would differ).  With distributed=True rank 0's draw is broadcast (broadcast_object_list) before every use."""

    def __init__(self, loaders, accum_steps=1, distributed=False):
        assert isinstance(loaders, dict)
        self.name2loader, self.name2iter, self.sampling_pools = {}, {}, []
        for n, l in loaders.items():
            if isinstance(l, tuple):
                l, r = l
            elif hasattr(l, "__iter__"):
                r = 1
            else:
                raise ValueError(f"MetaLoader: {n!r} is neither a loader nor a (loader, ratio) pair")
            assert isinstance(r, int)
            self.name2loader[n] = l
            self.name2iter[n] = iter(l)
            self.sampling_pools.extend([n] * r)
        self.accum_steps = accum_steps
        self.distributed = distributed
        self.step = 0

    def __iter__(self):
        """this iterator runs indefinitely"""
        task = self.sampling_pools[0]
        while True:
            if self.step % self.accum_steps == 0:
                task = random.choice(self.sampling_pools)
                if self.distributed:
                    import torch.distributed as DIST
                    objects = [task]
                    DIST.broadcast_object_list(objects, src=0)
                    task = objects[0]
            self.step += 1
            iter_ = self.name2iter[task]
            try:
                batch = next(iter_)
            except StopIteration:
                iter_ = iter(self.name2loader[task])
                batch = next(iter_)
                self.name2iter[task] = iter_
            yield task, batch


def info(msg):
    if is_main_process():
        print(msg, flush=True)


class Agent_Multi_Task(Agent_Captioning):
    """main_multi_task_mlm.py:228-486.  caption_metric: as Agent_Captioning's (none is built in; without one the captioning task logs nothing)."""

    def __init__(self, args, model, mc_ans_tok_ids, caption_metric=None):
        Agent_Base.__init__(self, args, model)
        keep = getattr(args, "keep_logits", False)
        # the three flags as Agent_Captioning takes them.  (The reference's CaptioningLoss reads its config dict with getattr, so there every one
        # of them stays at its default 0; here, as in Agent_Captioning, the keys count.)
        cap_loss_config = {'label_smoothing': getattr(args, 'label_smoothing', 0), 'drop_worst_ratio': getattr(args, 'drop_worst_ratio', 0),
                           'drop_worst_after': getattr(args, 'drop_worst_after', 0)}
        self.cap_loss_func = CaptioningLoss(cap_loss_config, keep_logits=keep).cuda()
        # T.nn.CrossEntropyLoss(ignore_index=-1): the caption-loss kernel at label_smoothing 0 is bit-equal to the cross-entropy kernel and
        # counts the correct arg-max rows in the same pass
        self.non_cap_loss_func = CaptioningLoss({}, keep_logits=keep).cuda()
        self.log = defaultdict(list)
        self.task2loss, self.task2acc = {}, {}
        self.mc_ans_tok_ids = None if mc_ans_tok_ids is None else list(mc_ans_tok_ids)
        self.caption_metric = caption_metric
        self.rows_head = bool(getattr(args, "mt_rows", False))

    def meter_loss(self, task, ls):
        key = f'ls_{task}'
        if key not in self.task2loss:
            self.task2loss[key] = RunningMeter(key)
        self.task2loss[key](ls)

    def meter_acc(self, task, acc):
        key = f'ac_{task}'
        if key not in self.task2acc:
            self.task2acc[key] = RunningMeter(key)
        self.task2acc[key](acc)

    def add_prompt_or_task_token(self, batch, dl):
        """main_multi_task_mlm.py:254-275: under enable_prompt the prompt of the task's OWN dataset, else under enable_task_token the task's token"""
        task = batch["task"]
        if getattr(self.args, "enable_prompt", False):
            ds = dl.name2loader[task].dataset if isinstance(dl, MetaLoader) else dl.dataset
            batch["prompt"] = ds.get_prompt()
        elif getattr(self.args, "enable_task_token", False):
            batch["task_name"] = task_token_of(task)
        return batch

    def prepare_batch(self, batch):
        """move_to_cuda, plus what the rows paths and the loss take from the host: the labels (captioning: "_ans_mtm_cpu"; others: "_lab_host"),
        their count "_n_lab", the text "_txt_host", and the switch "_mt_rows".  `vid` stays on the host (the labels are built there)."""
        out = Agent_Base.prepare_batch(self, batch)
        kind = task_kind(batch["task"])
        rows = bool(getattr(self.args, "mt_rows", False))
        if kind == "captioning":
            lab = batch.get("ans_mtm")
            if isinstance(lab, torch.Tensor) and not lab.is_cuda:
                out["_ans_mtm_cpu"], out["_n_lab"] = lab, int((lab != -1).sum())
            out["_mt_rows"] = rows and "_ans_mtm_cpu" in out
            return out
        if kind == "retrieval":
            out["vid"] = batch["vid"]
            out["_n_lab"] = len(batch["vid"]) ** 2
        else:
            lab = batch.get("mask_ans")
            if isinstance(lab, torch.Tensor) and not lab.is_cuda:
                out["_lab_host"], out["_n_lab"] = lab, int((lab != -1).sum())
        txt = batch.get("txt")
        if isinstance(txt, torch.Tensor) and not txt.is_cuda:
            out["_txt_host"] = txt
        out["_mt_rows"] = rows
        return out

    def train_step(self, batch, sync=True):
        """main_multi_task_mlm.py:369-390 -> {'ls', 'ac'}: CaptioningLoss for a captioning task, cross entropy over the labelled rows otherwise;
        ac = correct arg-max rows / labelled rows, 0 without labels -- counted by the loss kernel while it reads the logits.  sync=False
        returns the two as device scalars."""
        self._set_mode(True)
        out = self.forward_step(batch)
        logits, ans = out["out"], out["ans"]
        loss_func = self.cap_loss_func if "captioning" in batch["task"] else self.non_cap_loss_func
        ls = loss_func(logits.flatten(0, len(logits.shape) - 2), ans.flatten(), batch.get("_n_lab"))
        stats = loss_func.stats
        self.backward_step(ls)
        acc = stats[2] / torch.clamp(stats[3], min=1.0)
        if not sync:
            return {'ls': ls.detach(), 'ac': acc}
        return {'ls': ls.item(), 'ac': float(acc)}

    def _labelled_logit_rows(self, batch, out):
        """the labelled rows of forward()'s (B, Lp + X, V) logits, gathered by the host labels, and those labels"""
        lab = batch["_lab_host"]
        lr = label_rows(lab, out.shape[1] - lab.shape[1])
        rows = _rows_2d(out)
        idx = torch.from_numpy(lr.row).to(rows.device, non_blocking=True)
        return rows.index_select(0, idx), lr

    def eval_step(self, batch, sync=True):
        """main_multi_task_mlm.py:316-361: the per-sample flags of one batch -- {'ac'} for retrieval / qamc, {'ac_1', 'ac_5'} for qaoe -- as
        lists, or with sync=False as device tensors (non_cap_evaluate copies once per loader).  args.mt_rows: the [MASK]-row paths
        (answer_rows / match_rows); otherwise forward()'s full logits.  Both read out with lav_answer_readout / lav_match_readout."""
        self._set_mode(False)
        kind = task_kind(batch["task"])
        model = self._unwrapped()
        rows = bool(batch.get("_mt_rows"))
        with torch.no_grad():
            if kind in ("retrieval", "qamc_ret"):
                res = model.match_rows(batch) if rows else None
                if res is None:
                    out = self.forward_step({k: v for k, v in batch.items() if k != "_mt_rows"})["out"]
                    res = model.match_full(batch, out)
                ac = {'ac': res[1].float()}
            else:
                cand = self.mc_ans_tok_ids if kind == "qamc" else None
                lab = batch.get("_lab_host")
                if lab is None:
                    raise ValueError(f"{batch['task']}: the batch has no host copy of its labels (Agent_Multi_Task.prepare_batch)")
                _B = lab.shape[0]
                if rows:
                    _, rank, choice = model.answer_rows(batch, cand=cand)
                else:
                    out = self.forward_step({k: v for k, v in batch.items() if k != "_mt_rows"})["out"]
                    got, lr = self._labelled_logit_rows(batch, out)
                    _, rank, choice = K.answer_readout(got, got.shape[-1], lr.label, cand or ())
                if kind == "qaoe":
                    ac = {f'ac_{k}': _pad_hits(((rank >= 0) & (rank < k)).float(), _B) for k in (1, 5)}
                else:
                    if choice.numel() != _B:
                        raise ValueError(f"{batch['task']}: {choice.numel()} labelled positions for {_B} samples; the multiple-choice read-out needs one each")
                    ac = {'ac': (choice == batch["ans_idx"].to(choice.device, non_blocking=True).to(torch.int32)).float()}
        return {k: v.tolist() for k, v in ac.items()} if sync else ac

    def non_cap_evaluate(self, task, dl):
        """main_multi_task_mlm.py:283-302.  The flags of every batch stay on the device: ONE device -> host copy per loader."""
        self._set_mode(False)
        ret = defaultdict(list)
        for batch in dl:
            batch = dict(batch)
            batch["task"] = task
            batch = self.prepare_batch(self.add_prompt_or_task_token(batch, dl))
            for k, v in self.eval_step(batch, sync=False).items():
                ret[k].append(v)
        keys = sorted(ret)
        flags = {}
        if keys:
            flat = torch.stack([torch.cat(ret[k]) for k in keys]).tolist()
            flags = dict(zip(keys, flat))
        gathered = defaultdict(list)
        for per_rank in _all_gather_objects(flags):
            for k in per_rank:
                gathered[k].extend(per_rank[k])
        self._set_mode(True)
        return {k: float(np.average(gathered[k])) for k in flags}

    def cap_evaluate(self, ep, val_dataloader, task="captioning", tag=None):
        """Agent_Captioning.evaluate with the prediction files under caption_predictions/<task>[/<tag>]: the file name holds only the number
        and the dataset's yaml name, so two captioning tasks, or the tail evaluation's step number and an earlier epoch number, would
        otherwise meet in one file and the later one would reuse the earlier one's predictions"""
        self._set_mode(False)
        result = Agent_Captioning.evaluate(self, ep, val_dataloader, subdir=task if tag is None else f"{task}/{tag}")
        self._set_mode(True)
        return result or {}                                   # no caption_metric: nothing to log

    def evaluate(self, ep, task, dl, tag=None):
        if "captioning" in task:
            return self.cap_evaluate(ep, dl, task, tag)
        return self.non_cap_evaluate(task, dl)

    def log_train(self, ep, step):
        log_info = self.log_memory(ep, step)
        log_info += "\n\t"
        for task, rm in self.task2loss.items():
            log_info += f" {task}: {rm.val:.2e}"
        log_info += "\n\t"
        for task, rm in self.task2acc.items():
            log_info += f" {task}: {rm.val * 100:.2f}"
        return log_info

    def _eval_all(self, tag, ep_vl, ep_ts, meta_dl_vl, meta_dl_ts, sub=None):
        for task, dl_vl in meta_dl_vl.items():
            res_vl = self.evaluate(ep_vl, task, dl_vl, sub)
            for k in res_vl:
                self.log[f'{task}_vl_{k}'].append(res_vl[k])
            info(f'{tag} {task} vl: {json.dumps(res_vl)}')
        for task, dl_ts in meta_dl_ts.items():
            res_ts = self.evaluate(ep_ts, task, dl_ts, sub)
            for k in res_ts:
                self.log[f'{task}_ts_{k}'].append(res_ts[k])
            info(f'{tag} {task} ts: {json.dumps(res_ts)}')

    def run(self, meta_dl_tr, meta_dl_vl, meta_dl_ts):
        """main_multi_task_mlm.py:404-478"""
        info("Start training....")
        step, ep = 0, 1
        for step, (task, batch) in enumerate(meta_dl_tr):
            ep = (step // self.args.iter_per_ep + 1)
            if step % self.args.logging_steps == 0:
                info(self.log_train(ep, step))
            batch = dict(batch)
            batch["task"] = task
            if "captioning" in task:
                batch.update(self.masking(batch['txt'], p_mask=self.args.p_mask))
            batch = self.add_prompt_or_task_token(batch, meta_dl_tr)
            batch = self.prepare_batch(batch)
            out = self.train_step(batch)
            self.meter_loss(task, out['ls'])
            self.meter_acc(task, out['ac'])
            if step % self.args.iter_per_ep == 0 and step:
                self._eval_all(f'Ep {ep}', ep, ep, meta_dl_vl, meta_dl_ts)
                self.save_model(ep)
            if step >= self.args.max_iter:
                break
        if step % self.args.logging_steps != 0:
            info(self.log_train(ep, step))
        if step % self.args.iter_per_ep != 0:
            # as the reference has it (:441-454): the tail evaluation passes `step` for validation and `ep` for test (the number only names
            # the captioning prediction file), and the checkpoint is numbered by step
            self._eval_all(f'Last step {step}', step, ep, meta_dl_vl, meta_dl_ts, sub="last_step")
            self.save_model(step)
        for split, dls in (('vl', meta_dl_vl), ('ts', meta_dl_ts)):
            for task in dls.keys():
                metric = best_metric_of(task)
                best = self.best_epoch(task, split, metric)
                if best is None:                               # e.g. captioning without a caption_metric: nothing was logged
                    continue
                info(f'Best {metric} on {task} {"val" if split == "vl" else "test"} @ ep {best[0]}, {best[1] * 100:.2f}')

    def best_epoch(self, task, split, metric):
        """(index, value) of the best logged `{task}_{split}_{metric}`, None when nothing was logged under that key"""
        vals = self.log.get(f"{task}_{split}_{metric}") if self.log is not None else None
        if not vals:
            return None
        i = int(np.argmax(vals))
        return (i, vals[i])
