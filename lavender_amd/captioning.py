"""LAVENDER_Captioning -- the training forward of the reference's model_for_captioning.py:40-95 on the HIP engine.

Captioning is MLM under a sequence-to-sequence attention mask (model.py:208-218): every position sees the video tokens,
a text position additionally sees the text up to itself, video positions see no text.  The mask is not materialised as a
(B, L, L) tensor on the device path: the fusion attention kernels take (key mask, number of prefix keys)
(lav_attn_desc.causal_from).  Generation (greedy, sampled and beam-search decoding, model_for_captioning.py:139-500) runs on a key / value
cache of the fusion encoder: lavender_amd/caption_decode.py."""
from collections import defaultdict

import torch
import torch.nn as nn

from .bert import BertConfigLite, BertOnlyMLMHead, load_hf_into, load_hf_state
from .model import LAVENDER_Base


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
        out = self.fc_mtm(out[:, (1 + _h * _w) * _T:])
        return {"out": out, "ans": ans_mtm}
