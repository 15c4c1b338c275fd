"""LAVENDER_Captioning -- the training forward of the reference's model_for_captioning.py:40-95 on the HIP engine.

Captioning is MLM under a sequence-to-sequence attention mask (model.py:208-218): every position sees the video tokens,
a text position additionally sees the text up to itself, video positions see no text.  The mask is not materialised as a
(B, L, L) tensor on the device path: the fusion attention kernels take (key mask, number of prefix keys)
(lav_attn_desc.causal_from).  Generation (greedy, sampled and beam-search decoding, model_for_captioning.py:139-500) runs on a key / value
cache of the fusion encoder: lavender_amd/caption_decode.py.

Fine-tuning (main_caption.py:49-270): CaptioningLoss (label smoothing as a KL divergence, "drop the worst" rows, one fused kernel that also
counts the correct arg-max rows and leaves d(loss)/d(logits) in the logits buffer) and Agent_Captioning (masking, train_step, train, test,
evaluate).  By default the agent runs the MLM head on the labelled text rows only (encode_forward_rows; LAV_CAP_ROWS=0 restores the full
(B, X, V) head): loss, accuracy and gradients are the same quantities, because pred == ans can only hold where ans != -1."""
import json
import os
import os.path as op
import time
from collections import defaultdict

import numpy as np
import torch
import torch.nn as nn

from . import engine as E
from .agent import Agent_Base
from .bert import BertConfigLite, BertOnlyMLMHead, load_hf_into, load_hf_state
from .dist import get_rank, get_world_size, is_main_process, synchronize
from .model import LAVENDER_Base


def rows_head_default():
    """LAV_CAP_ROWS=0: Agent_Captioning trains through the full (B, X, V) head of encode_forward"""
    return os.environ.get("LAV_CAP_ROWS", "1") != "0"


def kept_count(n, drop_worst_ratio):
    """k of CaptioningLoss.forward (model_for_captioning.py:29-33): int(n * (1 - ratio)) of n labelled rows are averaged.  k = 0 with n > 0
    (e.g. one labelled row at ratio 0.25) is the mean of nothing -- NaN in the reference -- and raises here."""
    n = int(n)
    k = int(n * (1 - drop_worst_ratio))
    if n > 0 and k <= 0:
        raise ValueError(f"CaptioningLoss: drop_worst_ratio {drop_worst_ratio} keeps int({n} * (1 - {drop_worst_ratio})) = {k} of {n} labelled rows; "
                         "the loss would be the mean of no rows (NaN).  Lower drop_worst_ratio, raise drop_worst_after or mask more tokens")
    return k


def masking(txt, p_mask, pad_id, mask_id):
    """Agent_Captioning.masking (main_caption.py:62-79): [PAD] and [MASK] are the only special tokens ([CLS] / [SEP] can be masked, unlike
    pre-training); one torch.rand(X) per row in row order, so the CPU RNG is consumed as by the reference's loop and the outputs are bit-identical."""
    _B, _X = txt.shape
    spc = torch.logical_or(txt == pad_id, txt == mask_id)
    ans_mtm = torch.ones(txt.shape).long() * -1
    if p_mask <= 0:
        return {"txt": txt, "ans_mtm": ans_mtm}
    for i in range(_B):
        hit = torch.logical_and(torch.logical_not(spc[i]), torch.rand(_X) < p_mask)
        ans_mtm[i][hit] = txt[i][hit]
        txt[i][hit] = mask_id
    return {"txt": txt, "ans_mtm": ans_mtm}


def get_predict_file(args, ep, output_dir, data_yaml_file):
    """main_caption.py:161-176: ep{ep}_pred[.{data}].{split}[.beam{n}].max{L}[.w_asr][.best{n}].tsv"""
    cc = [f'ep{ep}_pred']
    data = data_yaml_file.split('/')[-2]                    # example data_yaml_file: _datasets/coco_caption/test.yaml
    if data != 'coco_caption':
        cc.append(data)
    cc.append(op.splitext(op.basename(data_yaml_file))[0])
    if hasattr(args, 'num_beams'):
        cc.append('beam{}'.format(args.num_beams))
    cc.append('max{}'.format(args.max_gen_length))
    if hasattr(args, 'use_asr') and args.use_asr:
        cc.append('w_asr')
    if hasattr(args, 'num_keep_best') and args.num_keep_best != 1:
        cc.append('best{}'.format(args.num_keep_best))
    return op.join(output_dir, '{}.tsv'.format('.'.join(cc)))


class CaptioningLoss:
    """CaptioningLoss of model_for_captioning.py:10-37 on the HIP engine (lav_caption_loss_fwd_bwd): the constructor keys label_smoothing,
    drop_worst_ratio, drop_worst_after, the call counter `iter`, forward(logits, target) -> loss.

    config: a mapping or an object with these keys.  (The reference reads them with getattr from the plain dict main_caption.py:52-55 builds,
    which always yields the defaults 0; here a mapping's keys count, which is what its flags mean.)
    logits: a (rows, V) view of the MLM head's row-padded bf16 buffer; in training it is consumed (overwritten with the gradient) unless
    keep_logits.  target: int64, -1 = ignore -- the rows need not be filtered first, logits[ans != -1] and ans[ans != -1] work as well.
    count: the number of labelled rows when the host knows it (the labels are built on the host); without it one device read-back.
    After a call, `stats` holds the device tensor [sum of kept losses, k, number of correct rows, number of labelled rows]: the accuracy
    needs no second pass over the logits."""

    def __init__(self, config, keep_logits=False):
        get = config.get if hasattr(config, "get") else (lambda k, d: getattr(config, k, d))
        self.label_smoothing = get('label_smoothing', 0)
        self.drop_worst_ratio = get('drop_worst_ratio', 0)
        self.drop_worst_after = get('drop_worst_after', 0)
        self.keep_logits = bool(keep_logits)
        self.iter = 0
        self.stats = None

    def forward(self, logits, target, count=None):
        self.iter += 1
        n = int((target != -1).sum()) if count is None else int(count)
        select = self.drop_worst_ratio > 0 and self.iter > self.drop_worst_after
        k = kept_count(n, self.drop_worst_ratio) if select else n
        loss, self.stats = E.CaptionLossFn.apply(logits, target, float(self.label_smoothing), k, bool(select and k < n), self.keep_logits)
        return loss

    __call__ = forward

    def cuda(self):
        return self


class LAVENDER_Captioning(LAVENDER_Base):
    def __init__(self, args, tokzr=None, is_decoder=True):
        super().__init__(args, tokzr)
        self.config.is_decoder = is_decoder
        cfg = BertConfigLite.from_pretrained(args.tokenizer)
        self.fc_mtm = BertOnlyMLMHead(cfg)
        sd = load_hf_state(args.tokenizer, [("cls.", "")])
        if sd:
            load_hf_into(self.fc_mtm, sd, "MLM head (HF checkpoint)")
        self.task_tok2id = {"vtm": 0, "mc": 1, "oe": 2, "cap": 3}
        self.emb_task = nn.Parameter(0.02 * torch.randn(10, self.hidden_size))
        self.cap_prompt_txt_L = 0

    def forward(self, batch, is_decode=False):
        batch = defaultdict(lambda: None, batch)
        if is_decode:
            return self.generate(batch)
        if batch["_cap_rows"]:
            return self.encode_forward_rows(batch)
        return self.encode_forward(batch)

    def generate(self, batch, generator=None):
        """model_for_captioning.py:139-240 + _generate_no_beam_search (num_beams 1): (ids (B, 1, max_gen_length) int64 starting with [CLS],
        logprob (B, 1)); num_beams > 1: beam search (caption_decode.generate_beam), (ids (B, num_keep_best, max_gen_length), logprob (B,
        num_keep_best)), the hypotheses best first.  The input text matters only through its length; it is not embedded.  Runs without autograd and in eval mode
        (model.training is restored afterwards); parameters and gradients are not touched.  `generator`: optional torch.Generator of the
        sampling draws."""
        from . import caption_decode as CD
        batch = defaultdict(lambda: None, batch)
        pretxt = self._pretxt_spec("cap", batch["prompt"])       # task token / prompt between the video rows and the caption
        if pretxt is not None:
            self.cap_prompt_txt_L = 1 if pretxt[0] == "task" else int(pretxt[1][0].shape[-1])
        cfg = CD.make_config(self.args, batch["txt"].shape[1])
        was_training = self.training
        try:
            self.eval()
            with torch.no_grad():
                self.arena().sync_half_if_stale()
                if isinstance(cfg, CD.BeamConfig):
                    return CD.generate_beam(self, batch["img"], batch["txt"].shape[1], cfg, pretxt=pretxt)
                return CD.generate(self, batch["img"], batch["txt"].shape[1], cfg, generator=generator, pretxt=pretxt)
        finally:
            self.train(was_training)

    def encode_forward(self, batch):
        """model_for_captioning.py:54-95, branch input_ids is None.  With a task token / prompt the pre-text joins the fully visible prefix of
        the seq2seq mask (causal_from = Lv + Lp), its labels are -1 and its length is recorded in cap_prompt_txt_L."""
        out, ans_mtm, Lv, _ = self._fused_hidden(batch)
        out = self.fc_mtm(out[:, Lv:])
        return {"out": out, "ans": ans_mtm}

    def encode_forward_rows(self, batch):
        """encode_forward with the MLM head on the labelled text rows only (engine.RowGatherFn, as the loss-aware head of pretrain_mlm.py):
        {"out": (n_labelled, V) logits, "ans": (n_labelled,) labels}, rows in (clip, position) order.  Needs the host copy of the labels the
        agent keeps (batch["_ans_mtm_cpu"], (B, X) before the pre-text is prepended); a batch without any label takes the full head."""
        batch = defaultdict(lambda: None, batch)
        lab_cpu = batch["_ans_mtm_cpu"]
        assert lab_cpu is not None, "encode_forward_rows: batch['_ans_mtm_cpu'] (host labels, Agent_Captioning.prepare_batch) is missing"
        rows_b, rows_x = np.nonzero(lab_cpu.numpy() != -1)
        out, ans_mtm, Lv, _L = self._fused_hidden(batch)
        if len(rows_b) == 0:
            return {"out": self.fc_mtm(out[:, Lv:]), "ans": ans_mtm}
        n, Ltot, Hd = out.shape
        logits = self.fc_mtm(E.RowGatherFn.apply(out.reshape(n * Ltot, Hd), rows_b * Ltot + Lv + _L + rows_x))
        return {"out": logits, "ans": lab_cpu[rows_b, rows_x].to(out.device, non_blocking=True)}

    def _fused_hidden(self, batch):
        """the fusion encoder's output of encode_forward: (hidden (B, Lv + _L + X, H), labels with the pre-text's -1 in front, Lv, _L)"""
        if batch["input_ids"] is not None:
            raise NotImplementedError("the incremental-decoding branch (model_for_captioning.py:96-130) belongs to generation")
        img, txt, mask, ans_mtm = batch["img"], batch["txt"], batch["mask"], batch["ans_mtm"]
        prompt = batch["prompt"]
        (_B, _T, _, _H, _W) = img.shape
        _h, _w = _H // 32, _W // 32
        feat_img, mask_img, feat_txt, mask_txt = self.go_feat(img, txt, mask, task_name="cap", prompt=prompt)
        ans_mtm, _, feat_txt = self.prepro_txt_inputs(ans_mtm, mask_txt, feat_txt, task_name="cap", prompt=prompt)
        if prompt is not None and getattr(self.args, "enable_prompt", False):
            _L = len(prompt[0])
            self.cap_prompt_txt_L = _L
        elif getattr(self.args, "enable_task_token", False):
            _L = 1
            self.cap_prompt_txt_L = _L
        else:
            _L = 0
            assert self.cap_prompt_txt_L == _L
        ans_mtm[:, :_L] = -1
        mask_pretxt = torch.ones_like(mask_txt)[:, :_L] if _L > 0 else None
        out, _ = self.go_cross(feat_img, mask_img, feat_txt, mask_txt, attn_mask_type=batch["attn_mask_type"] or "seq2seq",
                               mask_pretxt=mask_pretxt)
        return out, ans_mtm, (1 + _h * _w) * _T, _L


class RunningMeter:
    """utils/logger.py RunningMeter: exponential running mean (smooth 0.99), val is None before the first value"""

    def __init__(self, name, val=None, smooth=0.99):
        self.name, self.val, self.smooth = name, val, smooth

    def __call__(self, value):
        self.val = value if self.val is None else value * (1 - self.smooth) + self.val * self.smooth


def _decode_caption(tokzr, ids):
    """tokenizer.decode(ids, skip_special_tokens=True); a tokenizer stub without decode (synthetic runs) gives the ids as words"""
    if hasattr(tokzr, "decode"):
        return tokzr.decode(ids, skip_special_tokens=True)
    special = set(getattr(tokzr, "ids", {}).get(t) for t in ("[PAD]", "[CLS]", "[SEP]", "[MASK]"))
    return " ".join(str(i) for i in ids if i not in special)


def _all_gather_objects(obj):
    """utils/dist.py all_gather: the list of every rank's object"""
    world = get_world_size()
    if world == 1:
        return [obj]
    import torch.distributed as DIST
    out = [None] * world
    DIST.all_gather_object(out, obj)
    return out


def write_prediction_tsv(rows, path, key_order=None):
    """tsv_writer + reorder_tsv_keys (utils/tsv_file_ops.py): one `key <tab> json` line per clip, in the dataset's key order when given"""
    if key_order is not None:
        pos = {str(k): i for i, k in enumerate(key_order)}
        rows = sorted(rows, key=lambda r: pos.get(str(r[0]), len(pos)))
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        for key, val in rows:
            f.write(f"{key}\t{val}\n")
    os.replace(tmp, path)


class Agent_Captioning(Agent_Base):
    """Agent_Captioning of main_caption.py:49-270.  caption_metric: optional callable (predict_file, caption_file) -> dict of scores for
    evaluate(); the reference's COCO metrics live in a package (evalcap) that is not part of its tree, so none is built in."""

    def __init__(self, args, model, caption_metric=None):
        super().__init__(args, model)
        loss_config = {'label_smoothing': getattr(args, 'label_smoothing', 0), 'drop_worst_ratio': getattr(args, 'drop_worst_ratio', 0),
                       'drop_worst_after': getattr(args, 'drop_worst_after', 0)}
        self.loss_func = CaptioningLoss(loss_config, keep_logits=getattr(args, "keep_logits", False)).cuda()
        self.log = defaultdict(list)
        self.running_meter = {'ls_tr': RunningMeter('ls_tr'), 'ac_tr': RunningMeter('ac_tr')}
        self.caption_metric = caption_metric
        self.rows_head = rows_head_default()

    def masking(self, txt, p_mask=0.15):
        return masking(txt, p_mask, self.pad_token_id, self.mask_token_id)

    def prepare_batch(self, batch):
        """move_to_cuda, plus the host copy of the labels: the labelled-rows head indexes with it and the loss takes its count (no device sync)"""
        lab = batch.get("ans_mtm")
        out = super().prepare_batch(batch)
        if isinstance(lab, torch.Tensor) and not lab.is_cuda:
            out["_ans_mtm_cpu"] = lab
            out["_n_lab"] = int((lab != -1).sum())
            out["_cap_rows"] = self.rows_head
        return out

    def train_step(self, batch, sync=True):
        """main_caption.py:219-231 -> (loss, accuracy); accuracy = correct arg-max rows / labelled rows, 0 without labels.  The loss kernel counts
        the correct rows while it reads the logits (pred == ans can only hold where ans != -1, so the labelled rows are all that matter).
        sync=False returns the two as device scalars."""
        self._set_mode(True)
        out = self.forward_step(batch)
        logits, ans = out["out"], out["ans"]
        n_lab = batch.get("_n_lab") if isinstance(batch, dict) else None
        ls = self.loss_func(logits.flatten(0, len(logits.shape) - 2), ans.flatten(), n_lab)
        stats = self.loss_func.stats
        self.backward_step(ls)
        acc = stats[2] / torch.clamp(stats[3], min=1.0)
        if not sync:
            return ls.detach(), acc
        return ls.item(), float(acc)

    def log_train(self):
        ls_tr, ac_tr = self.running_meter['ls_tr'].val, self.running_meter['ac_tr'].val
        log_info = self.log_memory()
        if ls_tr is not None and ac_tr is not None:
            log_info += f" ls_tr: {ls_tr:.2e} ac_tr: {ac_tr * 100:.2f}"
        return log_info

    def train(self, ep, dl):
        """main_caption.py:241-270"""
        self._set_mode(True)
        ret_ls, ret_ac = [], []
        idx = 0
        for idx, batch in enumerate(dl):
            batch = dict(batch)
            if idx % self.args.logging_steps == 0 and is_main_process():
                print(self.log_train())
            batch.update(self.masking(batch['txt'], p_mask=self.args.p_mask))
            if getattr(self.args, "enable_prompt", False):
                batch["prompt"] = dl.dataset.get_prompt()
            batch = self.prepare_batch(batch)
            batch["attn_mask_type"] = "seq2seq"
            ls, ac = self.train_step(batch)
            self.running_meter['ls_tr'](ls)
            self.running_meter['ac_tr'](ac)
            ret_ls.append(ls)
            ret_ac.append(ac)
        if idx % self.args.logging_steps != 0 and is_main_process():
            print(self.log_train())
        ret_ls, ret_ac = float(np.average(ret_ls)), float(np.average(ret_ac))
        if getattr(self.args, "distributed", False):
            ret_ls, ret_ac = self.reduce_mean(ret_ls), self.reduce_mean(ret_ac)
        return {'loss': ret_ls, 'acc': ret_ac}

    def test(self, test_dataloader, predict_file):
        """main_caption.py:81-159: generate, one [key, json([{caption, conf}, ...])] row per clip, gathered over the ranks, written by rank 0"""
        tokenizer = getattr(test_dataloader.dataset, "tokzr", None) or self.tokzr
        self._set_mode(False)
        time_meter, step, all_preds = 0.0, 0, []
        with torch.no_grad():
            for step, batch in enumerate(test_dataloader):
                batch = dict(batch)
                batch['task'] = 'captioning_generation'
                batch["attn_mask_type"] = "seq2seq"
                if getattr(self.args, "enable_prompt", False):
                    batch["prompt"] = test_dataloader.dataset.get_prompt()
                batch = self.prepare_batch(batch)
                tic = time.time()
                outputs = self.model(batch, is_decode=True)
                all_caps, all_confs = outputs[0].cpu(), torch.exp(outputs[1]).cpu()      # (B, num_keep_best, max_len), (B, num_keep_best)
                time_meter += time.time() - tic
                for img_key, caps, confs in zip(batch["img_keys"], all_caps, all_confs):
                    res = [{'caption': _decode_caption(tokenizer, cap.tolist()), 'conf': conf.item()} for cap, conf in zip(caps, confs)]
                    if isinstance(img_key, torch.Tensor):
                        img_key = img_key.item()
                    all_preds.append([img_key, json.dumps(res)])
        if is_main_process():
            print(f"Inference model computing time: {time_meter / (step + 1)} seconds per batch")
        gathered = [p for preds in _all_gather_objects(all_preds) for p in preds]
        if is_main_process():
            write_prediction_tsv(gathered, predict_file, getattr(test_dataloader.dataset, "image_keys", None))
        synchronize()

    def get_predict_file(self, ep, output_dir, data_yaml_file):
        return get_predict_file(self.args, ep, output_dir, data_yaml_file)

    def get_evaluate_file(self, predict_file):
        assert predict_file.endswith('.tsv')
        return op.splitext(predict_file)[0] + '.eval.json'

    def evaluate(self, ep, val_dataloader, subdir=None):
        """main_caption.py:182-217: the prediction file under <path_output>/caption_predictions[/<subdir>] (skipped when it exists), then
        caption_metric(predict_file, caption_file) on rank 0, its result on every rank; None without a metric."""
        self._set_mode(False)
        output_dir = op.join(self.args.path_output, "caption_predictions", *([subdir] if subdir else []))
        if is_main_process():
            os.makedirs(output_dir, exist_ok=True)
        synchronize()
        predict_file = self.get_predict_file(ep, output_dir, val_dataloader.dataset.yaml_file)
        if op.isfile(predict_file):
            if is_main_process():
                print(f'Skip predict. {predict_file} already exists')
        else:
            self.test(val_dataloader, predict_file)
        synchronize()
        objects = [None]
        if is_main_process() and self.caption_metric is not None:
            evaluate_file = self.get_evaluate_file(predict_file)
            if op.isfile(evaluate_file):
                objects = [json.load(open(evaluate_file))]
            else:
                caption_file = val_dataloader.dataset.get_caption_file_in_coco_format()
                objects = [self.caption_metric(predict_file, caption_file)]
                json.dump(objects[0], open(evaluate_file, 'w'))
        if get_world_size() > 1:
            import torch.distributed as DIST
            DIST.broadcast_object_list(objects, src=0)
        return objects[0]

    def best_epoch(self, metric, split):
        val_index = int(np.argmax(self.log[f"{split}_{metric}"]))
        return (val_index, self.log[f"{split}_{metric}"][val_index])
