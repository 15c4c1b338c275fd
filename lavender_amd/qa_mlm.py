"""Video question answering posed as masked-LM -- mirrors of the reference's MLM-head QA callers:

    LAVENDER_QAOE_MLM / Agent_QAOE_MLM   main_qaoe_mlm_lsmdc_fib.py:64-125, main_qaoe_mlm.py:92-125   open-ended: the answer token is
                                         predicted at the "[MASK]" of "... answer: [MASK]" (X = 26 in the shipped configs)
    LAVENDER_QAMC_MLM / Agent_QAMC_MLM   main_qamc_mlm.py:109-209                                     multiple choice: question and all
                                         options as ONE text (X = 101), the [MASK] is trained to the option index token

    LAVENDER_RetMC_MLM / Agent_RetMC_MLM main_retmc_mlm.py:70-140                                      retrieval multiple choice: O candidate texts per
                                         video, each scored true / false at its [MASK]; the video prefix is shared by the O sequences
                                         through the pair-index gather (the reference expand()s and flattens feat_img)

The first two run one (video, text) sequence per sample through go_feat -> go_cross -> fc_mtm over the text positions -- the same HIP
kernels as the pre-training path ("they inherit the speed-up because they sit on the same modules").
With args.enable_task_token (batch["task_name"]) or args.enable_prompt (batch["prompt"] = (ids, mask)) the pre-text sits between the video
and the text rows (LAVENDER_Base.go_feat / prepro_txt_inputs); as in the reference these callers label it -1 (prepro_pretxt).

Rows path (args.qa_rows): exactly the labelled [MASK] rows reach the loss and the accuracy, so with the labels still on the host
(Agent.prepare_batch) forward_rows runs the MLM head on those rows only, and answer_rows additionally runs the last fusion layer on them only
and reads prediction, label rank and option choice out on the device (lav_answer_readout) -- no (B, X, vocab) logit block, no boolean indexing,
no per-batch host round trip.  The default (qa_rows off) is the reference's formulation, unchanged."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from . import engine as E
from . import hip as K
from .agent import Agent_Base, set_pretxt
from .bert import BertConfigLite, BertOnlyMLMHead, load_hf_into, load_hf_state
from .model import LAVENDER_Base


LabelRows = namedtuple("LabelRows", "sample pos row label width")


def label_rows(mask_ans, Lp=0):
    """The labelled positions of a host (B, X) label block (-1 = no label), in row-major order as `ans[ans != -1]` lists them: sample (n,) and
    pos (n,) int64 = sample and text position of each, row (n,) int64 = its row in the flattened (B * (Lp + X)) text block that carries Lp
    pre-text positions (labelled -1, LAVENDER_QAOE_MLM.prepro_pretxt) in front of every text, label (n,) int32, width = Lp + X."""
    a = mask_ans.numpy() if isinstance(mask_ans, torch.Tensor) else np.asarray(mask_ans)
    if a.ndim != 2:
        raise ValueError(f"label_rows: mask_ans must be (B, X), got {a.shape}")
    sample, pos = np.nonzero(a != -1)
    width = int(Lp) + a.shape[1]
    return LabelRows(sample.astype(np.int64), pos.astype(np.int64), sample.astype(np.int64) * width + int(Lp) + pos.astype(np.int64),
                     a[sample, pos].astype(np.int32), width)


def host_labels_of(args, batch, out):
    """prepare_batch with args.qa_rows: the prepared batch `out` also carries the host labels of `batch`"""
    if getattr(args, "qa_rows", False):
        lab = batch.get("mask_ans")
        if isinstance(lab, torch.Tensor) and not lab.is_cuda and lab.dim() == 2:
            out["_lab_host"] = lab
    return out


class QAForwardMixin:
    """What the MLM-head QA callers share (a LAVENDER_Base with the MLM head `fc_mtm`): the forwards of LAVENDER_QAOE_MLM / LAVENDER_QAMC_MLM
    (qa_forward) and LAVENDER_RetMC_MLM (retmc_forward), the -1 labels of the pre-text and the rows path (qa_forward_rows, answer_rows).
    multi_task.LAVENDER_Multi_Task inherits the same methods."""

    def qa_forward(self, batch):
        """main_qaoe_mlm_lsmdc_fib.py:79-93 / main_qamc_mlm.py:124-140: (B, X, vocab) logits over the text positions and the
        (B, X) labels (-1 everywhere but the [MASK])."""
        feat_img, mask_img, feat_txt, mask_txt, ans, Lv, _ = self._front(batch)
        out, _ = self.go_cross(feat_img, mask_img, feat_txt, mask_txt)
        out = self.fc_mtm(out[:, Lv:])
        return out, ans

    def prepro_pretxt(self, task_or_prompt_txt):
        """main_qaoe_mlm_lsmdc_fib.py:76-77 (main_qamc_mlm.py:121-122, main_retmc_mlm.py:87-88): the pre-text positions carry no label"""
        return torch.ones_like(task_or_prompt_txt) * -1

    def _front(self, batch):
        """forward up to the fusion encoder's input: (feat_img, mask_img, feat_txt, mask_txt, labels with the pre-text's -1 in front, Lv, Lp)"""
        img, txt, mask, ans = [batch.get(key) for key in ["img", "txt", "mask", "mask_ans"]]
        (_B, _T, _, _H, _W) = img.shape
        _h, _w = _H // 32, _W // 32
        task_name, prompt = batch.get("task_name"), batch.get("prompt")
        feat_img, mask_img, feat_txt, mask_txt = self.go_feat(img, txt, mask, task_name=task_name, prompt=prompt)
        ans, mask_txt, feat_txt = self.prepro_txt_inputs(ans, mask_txt, feat_txt, task_name=task_name, prompt=prompt)
        return feat_img, mask_img, feat_txt, mask_txt, ans, (1 + _h * _w) * _T, feat_txt.shape[1] - txt.shape[1]

    # ---- rows path: only the labelled rows ------------------------------------------------------------------------------------
    def qa_forward_rows(self, batch, full=None):
        """qa_forward (or the caller's own `full` forward) restricted to the labelled positions: ((n_lab, vocab) logits, (n_lab,) labels) in the order of `ans[ans != -1]`.  The batch
        carries the host copy of its labels as batch["_lab_host"] (qa_mlm.host_labels_of); the encoder runs as in forward, engine.RowGatherFn takes
        the labelled rows of the last hidden state and fc_mtm runs on those.  Any number of labelled rows per sample; a batch without a host
        copy or without any label takes forward() (flattened), so the loss behaves as on the full path."""
        host = batch.get("_lab_host")
        if host is None or not bool((host != -1).any()):
            out, ans = (full or self.qa_forward)({k: v for k, v in batch.items() if k != "_lab_host"})
            return out.flatten(0, 1), ans.flatten()
        feat_img, mask_img, feat_txt, mask_txt, _, Lv, Lp = self._front(batch)
        lr = label_rows(host, Lp)
        out, _ = self.go_cross(feat_img, mask_img, feat_txt, mask_txt)
        n, L, Hd = out.shape
        rows = E.RowGatherFn.apply(out.view(n * L, Hd), lr.sample * L + Lv + (lr.row - lr.sample * lr.width))
        labels = torch.from_numpy(lr.label.astype(np.int64)).to(rows.device, non_blocking=True)
        return self.fc_mtm(rows), labels

    def answer_rows(self, batch, cand=None):
        """Evaluation read-out of the labelled positions (eval mode, under no_grad): device int32 (pred, rank, choice), each (n_lab,) in the
        order of `ans[ans != -1]` -- arg-max token, number of tokens sorting before the label (top-k hit: 0 <= rank < k), arg-max over `cand`
        of x_cand / sum x_cand (-1 without candidates); rules of lav_answer_readout.  Layers 0 .. n-2 run as _encode runs them; with exactly one
        labelled row per sample (and head_dim 64, more than one layer) the last layer runs on those rows only (engine.bert_layer_rows_eval),
        otherwise it runs in full and the rows are gathered.  The head runs on n_lab rows.  No result is read back: the only host <-> device traffic is the upload of the small index arrays (from
        pageable memory, so staged by the runtime rather than fully asynchronous)."""
        if torch.is_grad_enabled() or self.training:
            raise RuntimeError("answer_rows is evaluation only: call model.eval() and run it under torch.no_grad()")
        host = batch.get("_lab_host")
        if host is None:
            raise ValueError("answer_rows: the batch has no host copy of its labels (Agent.prepare_batch with args.qa_rows)")
        feat_img, mask_img, feat_txt, mask_txt, _, Lv, Lp = self._front(batch)
        lr = label_rows(host, Lp)
        n_lab = len(lr.row)
        dev, Hd = feat_img.device, feat_img.shape[-1]
        if n_lab == 0:
            e = torch.empty(0, dtype=torch.int32, device=dev)
            return e, e.clone(), e.clone()
        n = feat_img.shape[0]
        ident = np.arange(n)
        x, pair = self._pair_source(feat_img, feat_txt, ident, ident)
        mask = self.get_attn_mask(mask_img, mask_txt)
        L = mask.shape[1]
        assert Lv + feat_txt.shape[1] == L, f"mask and feat must have the same length, got {Lv + feat_txt.shape[1]} vs. {L}"
        self.arena().sync_half_if_stale()
        km = mask.to(torch.int32).contiguous()
        x = x.reshape(-1, Hd)
        if not x.is_contiguous():
            x = x.contiguous()
        layers = self.trsfr.layer
        last = len(layers) - 1
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev, non_blocking=True)
        q = Lv + (lr.row - lr.sample * lr.width)              # row of each labelled position within its sequence
        sel = lr.sample * L + q
        one_each = n_lab == n and bool((lr.sample == ident).all())
        if one_each and last > 0 and Hd == 64 * layers[last].num_heads:
            x, x32 = self._layers(x, km, n, L, pair=pair, stop=last)
            y, _ = E.bert_layer_rows_eval(x, x32, layers[last], km, n, L, up(q), up(sel))
        else:
            x, _ = self._layers(x, km, n, L, pair=pair)
            y = K.gather_rows(x, up(sel), n_lab, Hd)
        logits = self.fc_mtm(y)
        return K.answer_readout(logits, logits.shape[-1], lr.label, cand if cand is not None else ())

    def retmc_forward(self, batch, rows=False):
        """main_retmc_mlm.py:89-113: txt / mask / mask_ans are (B, O, X); logits (B * O, X, vocab), labels back as (B, O, X).  rows: the MLM head on the
        labelled positions only, by the host copy batch["_lab_host"] (B, O, X) of the labels -- ((n_lab, vocab) logits, (n_lab,) labels)."""
        img, txt, mask, ans = [batch.get(key) for key in ["img", "txt", "mask", "mask_ans"]]
        (_B, _T, _, _H, _W), (_, _O, _X) = img.shape, txt.shape
        _h, _w = _H // 32, _W // 32
        task_name, prompt = batch.get("task_name"), batch.get("prompt")
        feat_img, mask_img, feat_txt, mask_txt = self.go_feat(img, txt.flatten(0, 1), mask.flatten(0, 1), task_name=task_name, prompt=prompt)
        ans = ans.flatten(0, 1)
        ans, mask_txt, feat_txt = self.prepro_txt_inputs(ans, mask_txt, feat_txt, task_name=task_name, prompt=prompt)
        vi, ti = np.repeat(np.arange(_B), _O), np.arange(_B * _O)       # video i with each of its O texts (expand + flatten, :100-103)
        out, _ = self.go_cross_pairs(feat_img, mask_img, feat_txt, mask_txt, vi, ti)
        if rows:
            Lv, Lp = (1 + _h * _w) * _T, feat_txt.shape[1] - _X
            lr = label_rows(batch["_lab_host"].flatten(0, 1), Lp)
            n, L, Hd = out.shape
            got = E.RowGatherFn.apply(out.reshape(n * L, Hd), lr.sample * L + Lv + Lp + lr.pos)
            return self.fc_mtm(got), torch.from_numpy(lr.label.astype(np.int64)).to(got.device, non_blocking=True)
        out = self.fc_mtm(out[:, (1 + _h * _w) * _T:])
        return out, ans.view(_B, _O, -1)


class LAVENDER_QAOE_MLM(QAForwardMixin, LAVENDER_Base):
    def __init__(self, args, tokzr=None):
        super().__init__(args, tokzr)
        assert getattr(args, "size_vocab", -1) == -1, "the MLM-head QA model answers with the tokenizer's vocabulary (size_vocab = -1)"
        cfg = BertConfigLite.from_pretrained(args.tokenizer)
        self.fc_mtm = BertOnlyMLMHead(cfg)
        sd = load_hf_state(args.tokenizer, [("cls.", "")])
        if sd:
            load_hf_into(self.fc_mtm, sd, "MLM head (HF checkpoint)")
        self.task_tok2id = {"vtm": 0, "mc": 1, "oe": 2, "cap": 3}
        self.emb_task = nn.Parameter(0.02 * torch.randn(10, self.hidden_size))

    def forward(self, batch):
        return self.qa_forward(batch)

    def forward_rows(self, batch):
        return self.qa_forward_rows(batch, self.forward)


class LAVENDER_QAMC_MLM(LAVENDER_QAOE_MLM):
    """main_qamc_mlm.py:109-140: the multiple-choice model is the same graph (its task-specific `fc` is deleted in favour of the
    MLM head); only the text it is fed and the agent's evaluation differ."""


class LAVENDER_RetMC_MLM(LAVENDER_QAOE_MLM):
    def forward(self, batch):
        return self.retmc_forward(batch)


class Agent_RetMC_MLM(Agent_Base):
    def __init__(self, args, model):
        super().__init__(args, model)
        self.log = {'ls_tr': [], 'ac_vl': [], 'ac_ts': []}

    def prepare_batch(self, batch):
        lab = batch.get("mask_ans")
        if isinstance(lab, torch.Tensor) and not lab.is_cuda:
            batch["_n_lab"] = int((lab != -1).sum())
        return super().prepare_batch(batch)

    def step(self, batch, is_train):
        """main_retmc_mlm.py:120-140."""
        self._set_mode(is_train)
        n_lab = batch.pop("_n_lab", None) if isinstance(batch, dict) else None
        with torch.set_grad_enabled(is_train):
            out, ans = self.forward_step(batch)
            if is_train:
                ls = self.loss_func(out.flatten(0, len(out.shape) - 2), ans.flatten(0, 1).flatten(0, 1), n_lab)
                self.backward_step(ls)
                return ls.item()
        _B, _O, _L = ans.shape
        p_true = out[:, :, self.true_token_id].float()
        p_false = out[:, :, self.false_token_id].float()
        out_mtm = p_true / (p_true + p_false)
        ans_mtm = ans.view(_B * _O, _L)
        assert ans_mtm.shape == out_mtm.shape
        out_mtm = torch.argmax(out_mtm[ans_mtm != -1].view(_B, _O), dim=-1)
        ans_idx = (ans_mtm[ans_mtm != -1].view(_B, _O) == self.true_token_id).nonzero()[:, 1]
        return (out_mtm == ans_idx).float().tolist()

    def go_dl(self, ep, dl, is_train):
        """main_retmc_mlm.py:145-170."""
        self._set_mode(is_train)
        ret = []
        for batch in dl:
            batch = set_pretxt(self.args, dict(batch), dl, "vtm" if ep == 0 else getattr(self.args, "task_token", "vtm"))
            r = self.step(self.prepare_batch(batch), is_train)
            ret.extend(r) if isinstance(r, list) else ret.append(r)
        return self.reduce_mean(float(np.average(ret)))


def _rows_on(agent, batch):
    return bool(getattr(agent.args, "qa_rows", False)) and isinstance(batch, dict) and batch.get("_lab_host") is not None


def _rows_train(agent, batch):
    """one training step on the labelled rows: the loss as a device scalar"""
    n_lab = batch.pop("_n_lab", None)
    with torch.enable_grad():
        out, lab = agent._unwrapped().forward_rows(batch)
        ls = agent.loss_func(out, lab, n_lab)
        agent.backward_step(ls)
    return ls.detach()


def _pad_hits(hits, B):
    """flags as get_top_k_acc returns them: the labelled rows' hits in order, then zeros up to B entries (more labels than samples: all of them)"""
    out = torch.zeros(max(B, hits.numel()), dtype=torch.float32, device=hits.device)
    out[:hits.numel()] = hits
    return out


class Agent_QAOE_MLM(Agent_Base):
    def __init__(self, args, model):
        super().__init__(args, model)
        self.log = {}

    def step_rows(self, batch, is_train, sync=True):
        """step on the rows path (args.qa_rows): same results as step; sync=False leaves them on the device ({'ls': scalar} /
        {'ac_1', 'ac_5'}: (B,) float tensors) so that a loop can copy once at its end."""
        self._set_mode(is_train)
        if is_train:
            ls = _rows_train(self, batch)
            return {'ls': ls.item() if sync else ls}
        _B = batch["_lab_host"].shape[0]
        with torch.no_grad():
            _, rank, _ = self._unwrapped().answer_rows(batch)
        ac = {f'ac_{k}': _pad_hits(((rank >= 0) & (rank < k)).float(), _B) for k in (1, 5)}
        return {k: v.tolist() for k, v in ac.items()} if sync else ac

    def step(self, batch, is_train):
        """main_qaoe_mlm_lsmdc_fib.py:100-113."""
        if _rows_on(self, batch):
            return self.step_rows(batch, is_train)
        self._set_mode(is_train)
        n_lab = batch.pop("_n_lab", None) if isinstance(batch, dict) else None
        with torch.set_grad_enabled(is_train):
            out, ans = self.forward_step(batch)
            if is_train:
                ls = self.loss_func(out.flatten(0, len(out.shape) - 2), ans.flatten(0, len(ans.shape) - 1), n_lab)
                self.backward_step(ls)
                return {'ls': ls.item()}
        return {'ac_1': self.get_top_k_acc(out, ans, k=1), 'ac_5': self.get_top_k_acc(out, ans, k=5)}

    def best_epoch(self):
        """main_qaoe_mlm_lsmdc_fib.py:128-137: ((epoch index, value) of the best ac_1 on val, the same on test)"""
        if "ac_1_vl" not in self.log or "ac_1_ts" not in self.log:
            raise ValueError("calling best_epoch in pretraining, maybe?")
        vi, ti = int(np.argmax(self.log["ac_1_vl"])), int(np.argmax(self.log["ac_1_ts"]))
        return (vi, self.log["ac_1_vl"][vi]), (ti, self.log["ac_1_ts"][ti])

    def get_top_k_acc(self, out, ans, k=5):
        """main_qaoe_mlm_lsmdc_fib.py:115-126."""
        _B = out.shape[0]
        ans_mtm = ans[ans != -1].view(-1, 1)
        out_mtm = out[ans != -1].view(ans_mtm.shape[0], -1).float()
        _, out_mtm_i = torch.topk(out_mtm, k=k, dim=-1)
        ac = (out_mtm_i == ans_mtm).any(dim=-1).float().tolist()
        if len(ac) < _B:
            ac += [0.] * (_B - len(ac))
        return ac

    def prepare_batch(self, batch):
        lab = batch.get("mask_ans")
        if isinstance(lab, torch.Tensor) and not lab.is_cuda:
            batch["_n_lab"] = int((lab != -1).sum())       # counted on the host: the loss kernel needs no device round trip
        out = super().prepare_batch(batch)
        return host_labels_of(self.args, batch, out)

    def go_dl(self, ep, dl, is_train):
        """main_qaoe_mlm.py:96-125.  Rows path in evaluation: the per-batch flags stay on the device, one copy after the loader."""
        self._set_mode(is_train)
        ret = {}
        if getattr(self.args, "qa_rows", False) and not is_train:
            for batch in dl:
                b = self.prepare_batch(set_pretxt(self.args, dict(batch), dl, "oe"))
                r = self.step_rows(b, False, sync=False) if _rows_on(self, b) else {k: torch.tensor(v) for k, v in self.step(b, False).items()}
                for k, v in r.items():
                    ret.setdefault(k, []).append(v)
            keys = sorted(ret)
            if keys:                                           # ONE device -> host copy of the evaluation: every metric's flags in one tensor
                dev = ret[keys[0]][0].device
                flat = torch.stack([torch.cat([t.to(dev) for t in ret[k]]) for k in keys]).tolist()
                ret = dict(zip(keys, flat))
            return {k: self.reduce_mean(float(np.average(v))) for k, v in ret.items()}
        for batch in dl:
            r = self.step(self.prepare_batch(set_pretxt(self.args, dict(batch), dl, "oe")), is_train)
            for k, l in r.items():
                ret.setdefault(k, []).extend(l if isinstance(l, list) else [l])
        return {k: self.reduce_mean(float(np.average(v))) for k, v in ret.items()}


class Agent_QAMC_MLM(Agent_Base):
    def __init__(self, args, model, ans_tok_ids):
        super().__init__(args, model)
        self.ans_tok_ids = list(ans_tok_ids)
        self.log = {'ls_tr': [], 'ac_vl': [], 'ac_ts': []}

    def prepare_batch(self, batch):
        lab = batch.get("mask_ans")
        if isinstance(lab, torch.Tensor) and not lab.is_cuda:
            batch["_n_lab"] = int((lab != -1).sum())
        out = super().prepare_batch(batch)
        return host_labels_of(self.args, batch, out)

    def step_rows(self, batch, is_train, sync=True):
        """step on the rows path (args.qa_rows): the float loss / B hit flags of step; sync=False leaves them on the device.  Every sample
        must carry exactly one labelled position (the reference's view(_B, 1) of the option scores): ValueError otherwise."""
        self._set_mode(is_train)
        cnt = (batch["_lab_host"] != -1).sum(1)
        if not bool((cnt == 1).all()):
            b = int(torch.nonzero(cnt != 1)[0])
            raise ValueError(f"Agent_QAMC_MLM: sample {b} has {int(cnt[b])} labelled positions; the multiple-choice read-out needs exactly one")
        if is_train:
            ls = _rows_train(self, batch)
            return ls.item() if sync else ls
        with torch.no_grad():
            _, _, choice = self._unwrapped().answer_rows(batch, cand=self.ans_tok_ids)
        hits = (choice == batch["ans_idx"].to(choice.device, non_blocking=True).to(torch.int32)).float()
        return hits.tolist() if sync else hits

    def step(self, batch, is_train):
        """main_qamc_mlm.py:148-170."""
        if _rows_on(self, batch):
            return self.step_rows(batch, is_train)
        self._set_mode(is_train)
        n_lab = batch.pop("_n_lab", None) if isinstance(batch, dict) else None
        with torch.set_grad_enabled(is_train):
            out, ans = self.forward_step(batch)
            if is_train:
                ls = self.loss_func(out.flatten(0, len(out.shape) - 2), ans.flatten(0, len(ans.shape) - 1), n_lab)
                self.backward_step(ls)
                return ls.item()
        _B = ans.shape[0]
        p_all = out[:, :, self.ans_tok_ids].float()
        out_mtm = p_all[ans != -1]
        out_mtm = (out_mtm / out_mtm.sum(dim=-1).view(_B, 1)).view(_B, -1)
        return (torch.argmax(out_mtm, dim=-1) == batch["ans_idx"].to(out_mtm.device)).float().tolist()

    def best_epoch(self):
        """agent.py:267-276: ((epoch index, value) of the best validation accuracy, the same on test)"""
        if "ac_vl" not in self.log or "ac_ts" not in self.log:
            raise ValueError("calling best_epoch in pretraining, maybe?")
        vi, ti = int(np.argmax(self.log["ac_vl"])), int(np.argmax(self.log["ac_ts"]))
        return (vi, self.log["ac_vl"][vi]), (ti, self.log["ac_ts"][ti])

    def go_dl(self, ep, dl, is_train):
        """main_qamc_mlm.py:172-207.  Rows path in evaluation: the per-batch flags stay on the device, one copy after the loader."""
        self._set_mode(is_train)
        ret = []
        rows_eval = getattr(self.args, "qa_rows", False) and not is_train
        for batch in dl:
            batch = set_pretxt(self.args, dict(batch), dl, "vtm" if ep == 0 else getattr(self.args, "task_token", "vtm"))
            b = self.prepare_batch(batch)
            if rows_eval:
                ret.append(self.step_rows(b, False, sync=False) if _rows_on(self, b) else torch.tensor(self.step(b, False)))
                continue
            r = self.step(b, is_train)
            ret.extend(r) if isinstance(r, list) else ret.append(r)
        if rows_eval and ret:
            ret = torch.cat([t.to(ret[0].device) for t in ret]).tolist()       # the one device -> host copy of the evaluation
        return self.reduce_mean(float(np.average(ret)))
