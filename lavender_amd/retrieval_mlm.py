"""LAVENDER_Retrieval_MLM / Agent_Retrieval_MLM -- mirror of the reference's main_retrieval_mlm.py:30-118.

Text-to-video retrieval posed as masked-LM: every one of the B x B (video i, text j) pairs is run through the
fusion encoder and the MLM head; the appended [MASK] position is trained to say "true" when vid[i] == vid[j]."""
import os
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn

from .agent import Agent_Base, set_pretxt
from .bert import BertConfigLite, BertOnlyMLMHead, load_hf_into, load_hf_state
from .model import LAVENDER_Base


def all_pairs(B):
    """Pair order of the double loop main_retrieval_mlm.py:63-64: i (video) outer, j (text) inner."""
    vi = np.repeat(np.arange(B), B)
    ti = np.tile(np.arange(B), B)
    return vi, ti


# Pair scorer of the retrieval evaluation: the last fusion layer and the MLM head run on the [MASK] row of each pair only (lav_bert_layer_fwd_rows,
# lav_mlm_pair_readout).  LAV_RET_ROWS=0 runs the full last layer and the full-vocabulary head and slices the two columns instead: the
# reference's formulation on this engine, for A/B.
RET_ROWS = os.environ.get("LAV_RET_ROWS", "1") != "0"


@dataclass
class PairSource:
    """What LAVENDER_RetrievalMlmEval.pair_source builds once for a whole evaluation: the un-expanded (U, H) rows [every video's Lv rows ;
    every text's X rows] that the first fusion layer reads through the pair map, the int64 key masks, and each text's [MASK] row."""
    src: torch.Tensor
    mask_img: torch.Tensor
    mask_txt: torch.Tensor
    n_video: int
    Lv: int
    n_text: int
    X: int
    q_row: np.ndarray                                  # (n_text,) int64: position of the [MASK] token within the text rows


class RetrievalPairsMixin:
    """What the MLM retrieval callers share (a LAVENDER_Base with the MLM head `fc_mtm` and a tokenizer): the all-pairs training forward of
    LAVENDER_Retrieval_MLM and the [MASK]-row pair scorer of LAVENDER_RetrievalMlmEval (pair_source / score_pairs), which
    multi_task.LAVENDER_Multi_Task applies to a batch's own features."""

    def retrieval_forward(self, batch, rows=False):
        """main_retrieval_mlm.py:50-91: same (B*B, X, vocab) logits and (B*B, X) labels; the B^2 python list of
        slices + T.cat is one gather kernel over the pair index list.  rows: the MLM head on the one labelled row of each pair (the last text
        position) only -- (B*B, vocab) logits and (B*B,) labels (engine.RowGatherFn; the labels are built on the host either way)."""
        img, txt, mask, vid = [batch.get(key) for key in ["img", "txt", "mask", "vid"]]
        task_name, prompt = batch.get("task_name"), batch.get("prompt")
        (_B, _T, _, _H, _W) = img.shape
        _h, _w = _H // 32, _W // 32
        Lv = (1 + _h * _w) * _T
        feat_img, mask_img, feat_txt, mask_txt = self.go_feat(img, txt, mask, task_name=task_name, prompt=prompt)
        # the pre-text (if any) is the same for every pair of text j: prepended once per text, not per pair as in the loop of :62-80
        txt, mask_txt, feat_txt = self.prepro_txt_inputs(txt, mask_txt, feat_txt, task_name=task_name, prompt=prompt)
        _X = txt.shape[1]
        vi, ti = all_pairs(_B)
        out, _ = self.go_cross_pairs(feat_img, mask_img, feat_txt, mask_txt, vi, ti)
        vid = list(vid.tolist()) if isinstance(vid, torch.Tensor) else list(vid)
        same = torch.tensor([vid[i] == vid[j] for i, j in zip(vi, ti)])
        if rows:
            from . import engine as E
            n, L, Hd = out.shape
            last = E.RowGatherFn.apply(out.reshape(n * L, Hd), np.arange(n, dtype=np.int64) * L + (L - 1))
            lab = torch.where(same, self.true_token_id, self.false_token_id).to(torch.int64)
            return self.fc_mtm(last), lab.to(txt.device, non_blocking=True)
        out = self.fc_mtm(out[:, Lv:])
        mtm_ans = torch.full((_B * _B, _X), -1, dtype=torch.long)
        mtm_ans[:, -1] = torch.where(same, self.true_token_id, self.false_token_id)
        return out, mtm_ans.to(txt.device, non_blocking=True)

    # ---- pair scorer (eval_retrieval_mlm.py:185-206 without the (pairs, X, vocab) logits) ---------------------------------------------------
    def pair_source(self, feat_img, mask_img, feat_txt, mask_txt, txt):
        """PairSource of 'feat' outputs: feat_img (M_v, Lv, H), mask_img (M_v, Lv), feat_txt (N_t, X, H), mask_txt / txt (N_t, X).  Each text
        must hold exactly one [MASK] token (the reference asserts one score per pair, eval_retrieval_mlm.py:207-208): ValueError otherwise.
        Features in go_feat's single buffer are used in place; separate tensors are joined by ONE copy here, never per chunk."""
        from . import engine as E
        Mv, Lv, Hd = feat_img.shape
        Nt, X = txt.shape
        if feat_txt.shape[:2] != (Nt, X) or mask_txt.shape != (Nt, X) or mask_img.shape != (Mv, Lv):
            raise ValueError(f"pair_source: feat_img {tuple(feat_img.shape)} / mask_img {tuple(mask_img.shape)} / feat_txt {tuple(feat_txt.shape)} / "
                             f"mask_txt {tuple(mask_txt.shape)} / txt {tuple(txt.shape)} do not agree")
        mask_id = getattr(self, "mask_token_id", None)
        if mask_id is None:
            raise ValueError("pair_source: the model has no [MASK] id (build it with a tokenizer)")
        hit = (txt.detach().to("cpu") == int(mask_id))
        cnt = hit.sum(1)
        bad = torch.nonzero(cnt != 1).flatten()
        if bad.numel():
            t = int(bad[0])
            raise ValueError(f"pair_source: text {t} holds {int(cnt[t])} [MASK] tokens; every text needs exactly one (Dataset_RetrievalMlmEval "
                             f"appends it)")
        q_row = hit.to(torch.int64).argmax(1).numpy()
        if E.rows_adjacent(feat_img, feat_txt):
            src = E.JoinRowsFn.apply(feat_img, feat_txt)
        else:
            src = torch.cat([feat_img.reshape(Mv * Lv, Hd), feat_txt.reshape(Nt * X, Hd).to(feat_img.dtype)], 0)
        return PairSource(src, mask_img.to(torch.int64).contiguous(), mask_txt.to(torch.int64).contiguous(), Mv, Lv, Nt, X, q_row)

    def score_pairs(self, src, vi, ti, out=None, logits=None, out_rows=None):
        """Scores p_true / (p_true + p_false) of the pairs (video vi[k], text ti[k]) of a PairSource (eval_retrieval_mlm.py:185-206), fp32 on
        the device.  out=None: returns the (n,) scores; else they are written to out[out_rows[k], vi[k]] (out_rows defaults to ti) and out is
        returned.  logits: an (n, 2) fp32 buffer for (p_true, p_false).  Nothing here waits for the device."""
        from . import engine as E
        from . import hip as K
        if torch.is_grad_enabled() or self.training:
            raise RuntimeError("score_pairs is evaluation only: call model.eval() and run it under torch.no_grad()")
        vi = np.ascontiguousarray(vi, dtype=np.int64).reshape(-1)
        ti = np.ascontiguousarray(ti, dtype=np.int64).reshape(-1)
        n = len(vi)
        if n == 0 or len(ti) != n:
            raise ValueError(f"score_pairs: {n} video and {len(ti)} text indices")
        if vi.min() < 0 or vi.max() >= src.n_video or ti.min() < 0 or ti.max() >= src.n_text:
            raise ValueError(f"score_pairs: index outside the {src.n_video} videos / {src.n_text} texts of the pair source")
        dev, Hd = src.src.device, src.src.shape[1]
        Lv, X = src.Lv, src.X
        L = Lv + X
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev, non_blocking=True)
        if out is None:
            S = torch.empty((1, n), dtype=torch.float32, device=dev)
            rows, cols = np.zeros(n, dtype=np.int64), np.arange(n)
        else:
            S = out
            assert S.dtype == torch.float32 and S.dim() == 2 and S.stride(1) == 1
            rows, cols = (ti if out_rows is None else np.asarray(out_rows, dtype=np.int64).reshape(-1)), vi
            if rows.min() < 0 or rows.max() >= S.shape[0] or cols.max() >= S.shape[1]:
                raise ValueError(f"score_pairs: output index outside the {tuple(S.shape)} score matrix")
        if logits is not None:
            assert logits.dtype == torch.float32 and logits.shape == (n, 2) and logits.is_contiguous()
        arena = self.arena()
        arena.sync_half_if_stale()
        flat = E.pair_index(src.n_video, Lv, src.n_text, X, vi, ti).reshape(-1)
        km = K.pair_key_mask(src.mask_img, src.mask_txt, vi, ti)
        if E.pair_fused_ok(Hd):
            x, pair = src.src, (up(flat), None, None)
        else:                                               # the map-reading GEMM tiles do not apply: this chunk's pairs gathered once
            x, pair = K.gather_rows(src.src, up(flat), n * L, Hd), None
        layers = self.trsfr.layer
        last = len(layers) - 1
        x, x32 = self._layers(x, km, n, L, pair=pair, stop=last)   # model._encode's layer loop (eval: no dropout), all but the last layer
        first = pair if last == 0 else None
        q = Lv + src.q_row[ti]                              # the [MASK] row of every pair within its sequence
        tid_true, tid_false = int(self.true_token_id), int(self.false_token_id)
        if not RET_ROWS:
            o = E.BertLayerFn.apply(arena.anchor, x, x32, layers[last], km, n, L, 0.0, 0.0, False, 0, first)
            out_l = self.fc_mtm(o[0].view(n, L, Hd)[:, Lv:])       # (n, X, vocab): the reference's logit block
            kk = torch.arange(n, device=dev)
            qq = torch.from_numpy(q - Lv).to(dev)
            pt = out_l[kk, qq, tid_true].float()
            pf = out_l[kk, qq, tid_false].float()
            S[torch.from_numpy(rows).to(dev), torch.from_numpy(cols).to(dev)] = pt / (pt + pf)
            if logits is not None:
                logits[:, 0] = pt
                logits[:, 1] = pf
            return S[0] if out is None else S
        sel = np.arange(n, dtype=np.int64) * L + q
        res_map = flat[sel] if first is not None else sel
        y, _ = E.bert_layer_rows_eval(x, x32, layers[last], km, n, L, up(q), up(res_map), x_rowmap=first[0] if first is not None else None)
        pred = self.fc_mtm.predictions
        tr, dec = pred.transform, pred.decoder
        t = torch.empty((n, Hd), dtype=torch.float32, device=dev)
        w_dec = E.W16(dec.weight)
        rows_d, cols_d = up(rows), up(cols)
        d = K.L.MlmPairReadoutDesc(n, Hd, dec.weight.shape[0], tid_true, tid_false, float(tr.LayerNorm.eps), y.data_ptr(), K._ld(y),
                                   E.W16(tr.dense.weight).data_ptr(), tr.dense.bias.data.data_ptr(), tr.LayerNorm.weight.data.data_ptr(),
                                   tr.LayerNorm.bias.data.data_ptr(), w_dec.data_ptr(), K._ld(w_dec), dec.bias.data.data_ptr(), t.data_ptr(),
                                   rows_d.data_ptr(), cols_d.data_ptr(), S.data_ptr(), K._ld(S), S.shape[0], S.shape[1],
                                   K._dp(logits))
        K.mlm_pair_readout(d)
        return S[0] if out is None else S


class LAVENDER_Retrieval_MLM(RetrievalPairsMixin, LAVENDER_Base):
    def __init__(self, args, tokzr=None):
        super().__init__(args, tokzr)
        cfg = BertConfigLite.from_pretrained(args.tokenizer)
        self.fc_mtm = BertOnlyMLMHead(cfg)
        sd = load_hf_state(args.tokenizer, [("cls.", "")])
        if sd:
            load_hf_into(self.fc_mtm, sd, "MLM head (HF checkpoint)")
        self.task_tok2id = {"vtm": 0, "mc": 1, "oe": 2, "cap": 3}
        self.emb_task = nn.Parameter(0.02 * torch.randn(10, self.hidden_size))

    def forward(self, batch):
        return self.retrieval_forward(batch)


class Agent_Retrieval_MLM(Agent_Base):
    def __init__(self, args, model):
        super().__init__(args, model)
        self.log = {'ls_tr': [], 'ac_vl': [], 'ac_ts': []}

    def step(self, batch, is_train, sync=True):
        """main_retrieval_mlm.py:99-118.  sync=False returns the training loss as a device scalar (no host round trip per step)."""
        self._set_mode(is_train)
        with torch.set_grad_enabled(is_train):
            out, ans = self.forward_step(batch)
            if is_train:
                n_pairs = out.shape[0]                         # one labelled position per pair
                out = out.flatten(0, len(out.shape) - 2)
                ans = ans.flatten(0, len(ans.shape) - 1)
                ls = self.loss_func(out, ans, n_pairs)
                self.backward_step(ls)
                return ls.item() if sync else ls.detach()
        _B = len(batch["vid"])
        p_true = out[:, :, self.true_token_id].float()
        p_false = out[:, :, self.false_token_id].float()
        out_mtm = p_true / (p_true + p_false)
        out_mtm = out_mtm[ans != -1].view(_B, _B)
        ans_mtm = ans[ans != -1].view(_B, _B)
        out_mtm = torch.argmax(out_mtm, dim=-1)
        ans_idx = (ans_mtm == self.true_token_id).nonzero()[:, 1]
        return (out_mtm == ans_idx).float().tolist()

    def go_dl(self, ep, dl, is_train):
        """main_retrieval_mlm.py:120-150."""
        self._set_mode(is_train)
        ret = []
        for batch in dl:
            batch = self.prepare_batch(set_pretxt(self.args, dict(batch), dl, "vtm"))
            r = self.step(batch, is_train)
            ret.extend(r) if isinstance(r, list) else ret.append(r)
        return self.reduce_mean(float(np.average(ret)))


class LAVENDER_RetrievalMlmEval(LAVENDER_Retrieval_MLM):
    """Two-phase retrieval inference of the reference (eval_retrieval_mlm.py:10-47): 'feat' encodes every video once
    (mean over its clips) and every caption once; 'cross' runs the fusion encoder + MLM head on (video, text) pairs
    of cached features.  Forward only."""

    def forward(self, typ, batch):
        from . import hip as K
        if typ == 'feat':
            img, txt, mask = [batch.get(key) for key in ["img", "txt", "mask"]]
            task_name = batch.get("task_name")
            # eval_retrieval_mlm.py:24,154-164: the prompt comes as (n, Lp) rows prompt_txt / prompt_mask (a block per text)
            prompt = (batch["prompt_txt"], batch["prompt_mask"]) if batch.get("prompt_txt") is not None else None
            _B, _Clips, _T, _C, _H, _W = img.shape
            feat_img, mask_img, feat_txt, mask_txt = self.go_feat(img.view(-1, _T, _C, _H, _W), txt, mask, task_name=task_name, prompt=prompt)
            Lv, Hd = feat_img.shape[1], feat_img.shape[2]
            if _Clips > 1:                                # mean over the clips of a video: gather-sum kernel + 1/Clips scale kernel
                rows = feat_img.reshape(_B * _Clips * Lv, Hd)
                idx = (torch.arange(_B * Lv).view(_B, 1, Lv) // Lv * (_Clips * Lv) + torch.arange(Lv).view(1, 1, Lv)
                       + torch.arange(_Clips).view(1, _Clips, 1) * Lv)                      # (B, Clips, Lv) source rows
                lst = idx.permute(0, 2, 1).reshape(-1).to(torch.int32).to(rows.device)      # per output row: its Clips sources
                start = (torch.arange(_B * Lv + 1, dtype=torch.int32) * _Clips).to(rows.device)
                summed = K.gather_sum_rows(rows, start, lst, _B * Lv, Hd)
                scale = torch.full((1,), 1.0 / _Clips, dtype=torch.float32, device=rows.device)
                mean = torch.empty_like(summed)
                K.scale_mask_rows(summed, _B * Lv, Hd, out=mean, row_scale=scale, rows_per_group=_B * Lv)
                feat_img = mean.view(_B, Lv, Hd)
            else:
                feat_img = feat_img.view(_B, Lv, Hd)
            mask_img = mask_img.view(_B, _Clips, -1)[:, 0, :]
            txt, mask_txt, feat_txt = self.prepro_txt_inputs(txt, mask_txt, feat_txt, task_name=task_name, prompt=prompt)
            return feat_img, mask_img, feat_txt, mask_txt, txt
        elif typ == 'cross':
            feat_img, mask_img, feat_txt, mask_txt = [batch.get(key) for key in ["feat_img", "mask_img", "feat_txt", "mask_txt"]]
            out, _ = self.go_cross(feat_img, mask_img, feat_txt, mask_txt)
            return self.fc_mtm(out[:, feat_img.shape[1]:]), batch.get("txt")
        raise ValueError(f"typ must be 'feat' or 'cross', got {typ!r}")
