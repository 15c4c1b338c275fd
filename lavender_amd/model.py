"""EncVideo / EncTxt / LAVENDER_Base -- MI355X-native mirror of the reference's model.py.

Same class, attribute, method and state_dict key names; the arithmetic runs on the HIP
engine.  Activations are bf16 (the reference trains under fp16 autocast / DeepSpeed fp16, agent.py:199-233);
parameters are fp32 masters in a flat arena with a bf16 working copy (lavender_amd.arena).
"""
import os
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import engine as E
from . import hip as K
from .arena import ParamArena
from .bert import BertConfigLite, BertEmbeddings, BertEncoder, load_hf_into, load_hf_state
from .video_swin import LayerNorm, Linear, get_vidswin_model


class EncVideo(nn.Module):
    """model.py:5-93."""

    def __init__(self, args, hidden_size):
        super().__init__()
        self.swin = get_vidswin_model(args)
        self.latent_feat_size = self.swin.norm.normalized_shape[0]
        self.img_feature_dim = hidden_size
        self.swinbert = getattr(args, 'swinbert', False)
        if self.swinbert:
            raise NotImplementedError("the SwinBERT-initialised variant (model.py:33-35,52-66) is outside the pretrain hot path")
        self.max_size_frame = getattr(args, 'max_size_frame', 6)
        self.max_size_patch = getattr(args, 'max_size_patch', 14)
        self.fc = Linear(self.latent_feat_size, self.img_feature_dim) if self.latent_feat_size != self.img_feature_dim else None
        self.emb_cls = nn.Parameter(0.02 * torch.randn(1, 1, 1, hidden_size))
        self.emb_pos = nn.Parameter(0.02 * torch.randn(1, 1, 1 + self.max_size_patch ** 2, hidden_size))
        self.emb_len = nn.Parameter(0.02 * torch.randn(1, self.max_size_frame, 1, hidden_size))
        self.emb_odr = nn.Parameter(0.02 * torch.randn(1, 1, 1, hidden_size))
        self.norm = LayerNorm(hidden_size)
        self.transform_normalize = None
        self._arena_of = None

    def forward(self, img, odr=None, vt_mask=None, taps=None):
        if odr is not None:
            raise NotImplementedError("frame-order embeddings (model.py:72-81) are not used by the pretrain path")
        _B, _T, _C, _H, _W = img.shape
        _h, _w = _H // 32, _W // 32
        assert _T <= self.max_size_frame and _h * _w <= self.max_size_patch ** 2
        if self.transform_normalize is not None:
            img = self.transform_normalize(img)
        arena = self._arena_of() if self._arena_of is not None else self.swin._arena()
        tok, _ = self.swin.forward_tokens(img, frame_major=True, taps=taps)
        f_img = E.VideoEmbedFn.apply(arena.anchor, tok, self, _B, _T, _h * _w)
        m_img = torch.ones((_B, _T, 1 + _h * _w), dtype=torch.long, device=img.device)
        if vt_mask is not None:
            m_img = m_img * vt_mask
        return f_img, m_img.view(_B, _T * (1 + _h * _w))


class EncTxt(nn.Module):
    """model.py:96-142 (txt_backbone_embed_only branch: BERT embeddings only)."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        cfg = BertConfigLite.from_pretrained(args.txt_backbone)
        if not getattr(args, "txt_backbone_embed_only", True):
            raise NotImplementedError("a full text transformer in EncTxt (model.py:106-108) is not on the pretrain hot path")
        self.emb_txt = BertEmbeddings(cfg)
        self.txt_trsfr = None
        self.mask_ext = None
        self.size_vocab = cfg.vocab_size
        sd = load_hf_state(args.txt_backbone, [("bert.embeddings.", "emb_txt."), ("embeddings.", "emb_txt.")])
        if sd:
            load_hf_into(self, sd, "text embeddings (HF checkpoint)")
        self._arena_of = None

    def forward(self, txt, mask_txt=None, token_type_ids=None, position_ids=None, attn_mask_type="full"):
        assert token_type_ids is None and position_ids is None, "custom token_type/position ids are not supported"
        arena = self._arena_of()
        p = self.emb_txt.dropout_p if self.training else 0.0
        return E.TextEmbedFn.apply(arena.anchor, txt, self.emb_txt, p)

    def embed_with_pretxt(self, txt, pre=None, task=None):
        """(n, Lp + X, H) [pre-text ; embedded text]: pre = prompt features (1 or n, Lp, H), or task = (emb_task, row) (engine.PreTextEmbedFn)"""
        arena = self._arena_of()
        p = self.emb_txt.dropout_p if self.training else 0.0
        return E.PreTextEmbedFn.apply(arena.anchor, txt, self.emb_txt, p, pre, task)


class _AttentionsNotMaterialised:
    """Second return value of go_cross / go_cross_pairs.  The reference asks the HF encoder for output_attentions=True
    (model.py:242-243) and every pre-training / retrieval / QA caller drops them; the fused attention kernels never write the
    (n, heads, L, L) probabilities (19 MB per layer at the benchmark batch, 12 layers).  A caller that does USE them gets a clear
    error instead of a silent None."""

    def _fail(self, *a, **k):
        raise NotImplementedError("go_cross: attention probabilities are not materialised by the fused MI355X attention kernels "
                                  "(model.py:242-243 returns them; no caller on the pre-training path reads them)")
    __getitem__ = __iter__ = __len__ = __bool__ = _fail

    def __repr__(self):
        return "<attentions: not materialised>"


_NO_ATTN = _AttentionsNotMaterialised()


class LAVENDER_Base(nn.Module):
    """model.py:145-473 (hot-path methods + checkpoint contract)."""

    def __init__(self, args, tokzr=None):
        super().__init__()
        self.args = args
        self.enc_txt = EncTxt(args)
        cfg = BertConfigLite.from_pretrained(args.fusion_encoder)
        self.hidden_size = cfg.hidden_size
        self.config = cfg
        self.trsfr = BertEncoder(cfg)
        if not getattr(args, "fusion_encoder_rand_init", False):
            sd = load_hf_state(args.fusion_encoder, [("bert.encoder.", "")])
            if sd:
                load_hf_into(self.trsfr, sd, "fusion encoder (HF checkpoint)")
        self.mask_ext = self._extended_mask
        self.enc_img = EncVideo(args, self.hidden_size)
        self.use_checkpoint = bool(getattr(args, "use_checkpoint", False))   # 288 GB HBM: activations are kept, no CPU offload
        self.tokzr = tokzr
        if tokzr is not None:
            (self.cls_token_id, self.sep_token_id, self.pad_token_id, self.mask_token_id,
             self.unk_token_id) = self.tokzr.convert_tokens_to_ids(
                [self.tokzr.cls_token, self.tokzr.sep_token, self.tokzr.pad_token, self.tokzr.mask_token, self.tokzr.unk_token])
            self.true_token_id = self.tokzr.convert_tokens_to_ids(["true"])[0]
            self.false_token_id = self.tokzr.convert_tokens_to_ids(["false"])[0]
        self._lav_arena = None
        self.register_load_state_dict_post_hook(lambda m, k: m._mark_stale(k))

    # ---- arena ---------------------------------------------------------------------------------
    def _mark_stale(self, keys=None):
        a = self._lav_arena
        if a is not None:
            a.stale = True
            # a FULL load (no arena parameter missing from the state dict) rewrote every fp32 master on this rank: the masters
            # are whole again even if a ZeRO-1 step had sharded them (dp.ZeroOneReducer.gather_master then has nothing to do)
            if keys is not None and not any(k in a.offsets for k in getattr(keys, "missing_keys", ())):
                a.masters_sharded = False

    def arena(self):
        a = self._lav_arena
        probe = self.enc_img.norm.weight
        if a is None or not a.owns(probe):
            if probe.device.type != "cuda":
                raise RuntimeError("lavender_amd runs on the MI355X only: call model.cuda() first (there is no CPU path)")
            a = ParamArena(self, probe.device)
            self._lav_arena = a
            ref = weakref.ref(a)
            self.enc_img.swin._arena_ref = ref
            self.enc_img._arena_of = ref
            self.enc_txt._arena_of = ref
            for lyr in self.trsfr.layer:
                lyr._arena_of = ref
            for m in self.children():
                if hasattr(m, "predictions"):
                    m._arena_of = ref
        return a

    build_arena = arena

    def state_dict(self, *a, **kw):
        """nn.Module.state_dict over the fp32 masters; refuses to hand out a half-updated copy after a ZeRO-1 step (the masters
        are then sharded: gather them on every rank first, as Agent_Base.save_model does)."""
        if self._lav_arena is not None:
            self._lav_arena.require_full_master("state_dict")
        return super().state_dict(*a, **kw)

    def sync_weights(self):
        """Call after modifying parameters in place outside the built-in optimizer."""
        self.arena().sync_half()

    # ---- reference surface -----------------------------------------------------------------------
    @staticmethod
    def _extended_mask(mask, shape=None, device=None, dtype=torch.float32):
        """get_extended_attention_mask as used at model.py:136,239: (B,L) 0/1 -> additive (B,1,1,L)."""
        return (1.0 - mask[:, None, None, :].to(dtype)) * torch.finfo(dtype).min

    def go_feat(self, img, txt, mask, odr=None, vt_mask=None, attn_mask_type="full", task_name=None, prompt=None):
        """model.py:186-192.  task_name / prompt (this engine's addition): when get_pretxt would add a pre-text for them, feat_txt comes back
        as (n, Lp + X, H) [pre-text ; text] rows written by one kernel behind the video rows -- prepro_txt_inputs with the same task_name /
        prompt then prepends the ids and masks only.  mask is returned as given, as in the reference."""
        self.arena().sync_half_if_stale()
        spec = self._pretxt_spec(task_name, prompt) if (task_name is not None or prompt is not None) else None
        pre, task, Lp = None, None, 0
        if spec is not None and spec[0] == "task":
            task, Lp = (self.emb_task, spec[1]), 1
        elif spec is not None:
            pre = self._embed_prompt(spec[1][0], txt.device)   # before the tail hint: this small embedding is not part of the one buffer
            Lp = pre.shape[1]
        E.fusion_tail_hint(txt.shape[0] * (Lp + txt.shape[1]))   # feat_img and feat_txt land in ONE buffer: no T.cat in front of the fusion encoder
        feat_img, mask_img = self.enc_img(img, odr, vt_mask)
        if spec is None:
            feat_txt = self.enc_txt(txt, mask_txt=mask, attn_mask_type=attn_mask_type)
        else:
            feat_txt = self.enc_txt.embed_with_pretxt(txt, pre, task)
            feat_txt._lav_pretxt = spec
        E.fusion_tail_hint(0)
        return feat_img, mask_img, feat_txt, mask

    def get_attn_mask(self, mask_img, mask_txt, attn_mask_type="full", mask_pretxt=None):
        """model.py:194-221.  "full": (B, L) concatenation of the 0/1 masks.  "seq2seq" (captioning): the (B, L, L) mask of
        model.py:208-218 -- every query sees the video keys (by mask_img), text queries additionally see the text keys up to
        themselves, video queries see no text key.  The attention kernels take it as (key mask, number of prefix keys)."""
        full_mask = mask_img if mask_pretxt is None else torch.cat([mask_img, mask_pretxt.to(mask_img.device, mask_img.dtype)], dim=1)
        if attn_mask_type == "seq2seq":
            _B, _Lfull = full_mask.shape                       # the pre-text belongs to the fully visible prefix
            _Lt = mask_txt.shape[1]
            _L = _Lfull + _Lt
            mask = torch.zeros((_B, _L, _L), dtype=torch.long, device=mask_img.device)
            mask[:, :, :_Lfull] = full_mask[:, None, :]
            mask[:, _Lfull:, _Lfull:] = torch.tril(torch.ones((_Lt, _Lt), dtype=torch.long, device=mask_img.device))
            return mask
        return torch.cat([full_mask, mask_txt], dim=1)

    def _layers(self, x, km, n, L, causal_from=0, pair=None, stop=None):
        """The fusion encoder's layers [0, stop) (all of them by default) on x ((n * L, H) bf16 rows, or the un-expanded pair source with pair),
        km the (n, L) int32 key mask: (x, x32) as the next layer takes them -- x32 is None, the fp32 copy, or with engine.RESLN the tuple
        (pre, mean, rstd, gamma, beta) of the LayerNorm that produced x.  Dropout follows self.training.  The one layer loop of _encode,
        LAVENDER_RetrievalMlmEval.score_pairs and LAVENDER_QAOE_MLM.answer_rows."""
        arena = self.arena()
        ph = self.config.hidden_dropout_prob if self.training else 0.0
        pa = self.config.attention_probs_dropout_prob if self.training else 0.0
        layers = self.trsfr.layer
        x32, last = None, len(layers) - 1
        for i, lyr in enumerate(layers[:stop]):
            out = E.BertLayerFn.apply(arena.anchor, x, x32, lyr, km, n, L, ph, pa, i < last, int(causal_from), pair if i == 0 else None)
            if len(out) == 4:                                 # engine.RESLN: the next residual add normalises this layer's pre-LN rows itself
                ln = lyr.output.LayerNorm
                x, x32 = out[0], (out[1], out[2], out[3], ln.weight.data, ln.bias.data)
            else:
                x, x32 = out
        return x, x32

    def _encode(self, feat, mask, causal_from=0, pair=None):
        """feat (n, L, H) bf16, mask (n, L) 0/1 key mask -> last_hidden_state (n, L, H).  causal_from > 0: seq2seq mask with that
        many prefix (video) keys (lav_attn_desc.causal_from).  pair = (rowmap, start, order): feat is the UN-EXPANDED (U, H) source
        and the first layer reads it through the pair map (engine.BertLayerFn)."""
        self.arena().sync_half_if_stale()                     # e.g. load_ckpt followed directly by a 'cross' call on cached features
        n, L = mask.shape
        Hd = feat.shape[-1]
        km = mask.to(torch.int32).contiguous()
        x = feat.reshape(-1, Hd)
        if not x.is_contiguous():
            x = x.contiguous()
        x, _ = self._layers(x, km, n, L, causal_from, pair)
        return x.view(n, L, Hd)

    def _pair_source(self, feat_img, feat_txt, vi, ti):
        """([video rows of every clip ; text rows of every text] (U, H), (rowmap, start, order)) for the fused pair expansion, or
        (the gathered (n, L, H) input, None) where the map-reading GEMM tiles do not apply."""
        B, Lv, Hd = feat_img.shape
        nt, X = feat_txt.shape[0], feat_txt.shape[1]
        if not E.pair_fused_ok(Hd):
            return E.PairSeqFn.apply(feat_img, feat_txt, vi, ti), None
        dev = feat_img.device
        flat = E.pair_index(B, Lv, nt, X, vi, ti).reshape(-1)
        if E.rows_adjacent(feat_img, feat_txt):               # go_feat's layout: already one (U, H) buffer
            src = E.JoinRowsFn.apply(feat_img, feat_txt)
        else:                                                  # features from elsewhere (cached eval features, a caller's own tensors)
            src = torch.cat([feat_img.reshape(B * Lv, Hd), feat_txt.reshape(nt * X, Hd)], 0)   # U rows: one copy of each clip / text
        pair = [torch.from_numpy(flat).to(dev, non_blocking=True), None, None]
        if torch.is_grad_enabled():
            start, order = E.pair_csr(flat, B * Lv + nt * X)
            pair[1] = torch.from_numpy(start).to(dev, non_blocking=True)
            pair[2] = torch.from_numpy(order).to(dev, non_blocking=True)
        return src, tuple(pair)

    def go_cross(self, feat_img, mask_img, feat_txt, mask_txt, attn_mask_type="full", feat_pretxt=None, mask_pretxt=None):
        """model.py:223-245.  feat_pretxt (n, Lp, H): placed between the video and the text rows (one copy of the text rows; go_feat's
        pre-text path writes them in place instead).  mask_pretxt (n, Lp): the key mask of pre-text rows that feat_txt already carries in
        front of its text rows (captioning, model_for_captioning.py:83-92)."""
        if feat_pretxt is not None:
            feat_txt = torch.cat([feat_pretxt.to(feat_txt.dtype).expand(feat_txt.shape[0], -1, -1), feat_txt], dim=1)
        n = feat_img.shape[0]
        ident = np.arange(n)
        feat, pair = self._pair_source(feat_img, feat_txt, ident, ident)
        if attn_mask_type == "seq2seq":
            # (B, L, L) mask of get_attn_mask in kernel form: video (and pre-text) keys by their masks, text keys all valid but causal
            prefix = mask_img if mask_pretxt is None else torch.cat([mask_img, mask_pretxt.to(mask_img.device, mask_img.dtype)], dim=1)
            key_mask = torch.cat([prefix, torch.ones_like(mask_txt)], dim=1)
            assert key_mask.shape[1] == feat_img.shape[1] + feat_txt.shape[1], "mask and feat must have the same length"
            return self._encode(feat, key_mask, causal_from=prefix.shape[1], pair=pair), _NO_ATTN
        mask = self.get_attn_mask(mask_img, mask_txt, attn_mask_type=attn_mask_type, mask_pretxt=mask_pretxt)
        assert feat_img.shape[1] + feat_txt.shape[1] == mask.shape[1], f"mask and feat must have the same length, got {feat_img.shape[1] + feat_txt.shape[1]} vs. {mask.shape[1]}"
        return self._encode(feat, mask, pair=pair), _NO_ATTN

    def go_cross_pairs(self, feat_img, mask_img, feat_txt, mask_txt, vi, ti):
        """go_cross on the pair list (video vi[k], text ti[k]) without materialising per-pair copies in Python
        (replaces the list building + T.cat of main_pretrain_mlm.py:74-111)."""
        feat, pair = self._pair_source(feat_img, feat_txt, vi, ti)
        # host index arrays: checked against B / nt on the host and uploaded without blocking (torch.as_tensor(..., device=) is a synchronous
        # copy that waits for everything queued so far: it cost two device drains per step, 2 x 18 ms of host stall at the cfg2 shape)
        mask = K.pair_key_mask(mask_img, mask_txt, vi, ti)         # (n, L) int32: get_attn_mask("full") over the pair list, one launch
        return self._encode(feat, mask, pair=pair), _NO_ATTN

    # ---- pre-text: task token / prompt (model.py:247-307) ---------------------------------------------------------
    def _pretxt_spec(self, task_name=None, prompt=None):
        """what get_pretxt adds, with its precedence: ("task", row of emb_task) when args.enable_task_token, else ("prompt", (ids, mask))
        when a prompt is given and args.enable_prompt, else None"""
        if getattr(self.args, "enable_task_token", False):
            assert task_name is not None, "enable_task_token: the batch must name its task (batch['task_name'])"
            assert task_name in self.task_tok2id, f"unknown task {task_name!r} (task_tok2id: {sorted(self.task_tok2id)})"
            return ("task", self.task_tok2id[task_name])
        if prompt is not None and getattr(self.args, "enable_prompt", False):
            return ("prompt", prompt)
        return None

    def _embed_prompt(self, prompt_txt, device):
        """a prompt's features, embedded ONCE per call (dropout included) with the text embedding: (1, Lp, H) for a 1-D prompt (broadcast to
        every text), (n, Lp, H) for a 2-D one.  The reference's batched callers do the same (enc_txt(prompt), then expand); its per-pair loops
        (pretrain VTM, retrieval) embed the prompt once per pair and so draw a fresh dropout mask per pair -- the difference vanishes in eval."""
        ids = prompt_txt.to(device, non_blocking=True)
        return self.enc_txt(ids.unsqueeze(0) if ids.dim() == 1 else ids)

    def prepro_pretxt(self, task_or_prompt_txt):
        """model.py:247-248: the pre-text ids as they enter the returned txt (the QA callers override this with -1 labels)"""
        return task_or_prompt_txt

    def _pretxt_ids(self, spec, mask_txt):
        """(ids, mask) of the pre-text, shaped like mask_txt's leading dimensions (model.py:253-290 without the features)"""
        txt_dim, dev = mask_txt.dim(), mask_txt.device
        if spec[0] == "task":
            ids = torch.zeros(1, device=dev, dtype=mask_txt.dtype)
            m = torch.ones(1, device=dev, dtype=mask_txt.dtype)
            if txt_dim > 1:
                ids, m = ids.unsqueeze(0).expand(mask_txt.shape[0], -1), m.unsqueeze(0).expand(mask_txt.shape[0], -1)
            return self.prepro_pretxt(ids), m
        ids, m = spec[1]
        ids, m = ids.to(dev, non_blocking=True), m.to(dev, non_blocking=True)
        if txt_dim > 1 and ids.dim() == 1:
            ids, m = ids.unsqueeze(0).expand(mask_txt.shape[0], -1), m.unsqueeze(0).expand(mask_txt.shape[0], -1)
        elif txt_dim > 1 and ids.dim() > 1:
            assert mask_txt.shape[0] == ids.shape[0]
        elif not (txt_dim == 1 and ids.dim() == 1):
            raise ValueError(f"txt dim: {txt_dim}, prompt_txt dim {ids.dim()}")
        return self.prepro_pretxt(ids), m

    def get_pretxt(self, mask_txt, task_name=None, prompt=None):
        """model.py:250-290: (ids, mask, features) of the pre-text, or (None, None, None).  The features here are a separate tensor for a caller
        that concatenates them itself; go_feat(..., task_name=, prompt=) writes them in place instead."""
        spec = self._pretxt_spec(task_name, prompt)
        if spec is None:
            return None, None, None
        ids, m = self._pretxt_ids(spec, mask_txt)
        if spec[0] == "task":
            feat = E.TaskRowFn.apply(self.arena().anchor, self.emb_task, spec[1])          # (1, H)
            if mask_txt.dim() > 1:
                feat = feat.unsqueeze(0).expand(mask_txt.shape[0], -1, -1)
        else:
            feat = self._embed_prompt(spec[1][0], mask_txt.device)                         # (1 or n, Lp, H)
            if mask_txt.dim() > 1 and feat.shape[0] == 1:
                feat = feat.expand(mask_txt.shape[0], -1, -1)
            elif mask_txt.dim() == 1:
                feat = feat[0]
        return ids, m, feat

    def prepro_txt_inputs(self, txt, mask_txt, feat_txt, task_name=None, prompt=None):
        """model.py:292-307: the pre-text prepended to txt, mask_txt and feat_txt (identity with both switches off).  When feat_txt came from
        go_feat with the same task_name / prompt it already holds the pre-text rows (one buffer, no copy); other features take one copy."""
        spec = self._pretxt_spec(task_name, prompt)
        if spec is None:
            return txt, mask_txt, feat_txt
        ids, m = self._pretxt_ids(spec, mask_txt)
        done = getattr(feat_txt, "_lav_pretxt", None)
        if done is not None and done[0] == spec[0] and (done[1] == spec[1] if spec[0] == "task" else done[1] is spec[1]):
            out_feat = feat_txt
        else:
            _, _, pf = self.get_pretxt(mask_txt, task_name, prompt)
            out_feat = torch.cat([pf.to(feat_txt.dtype), feat_txt], dim=-2)
        return torch.cat([ids.to(txt.dtype), txt], dim=-1), torch.cat([m, mask_txt], dim=-1), out_feat

    # ---- checkpoint contract (model.py:352-429) ----------------------------------------------------
    def load_ckpt(self, ckpt):
        if ckpt == '':
            print('===== Finished Init LAVENDER  =====')
            return
        elif not os.path.exists(ckpt):
            print(f'Try to load pre-trained weights from {ckpt}, but file does not exists...')
            return
        print(f'Loading pre-trained weights from {ckpt}')
        loaded = torch.load(ckpt, map_location='cpu')
        self.__load_ckpt__(loaded)

    def __load_ckpt__(self, loaded_state_dict):
        own = self.state_dict()
        model_keys, load_keys = set(own.keys()), set(loaded_state_dict.keys())
        toload, mismatched = {}, []
        for k in model_keys:
            if k in load_keys:
                if own[k].shape != loaded_state_dict[k].shape:
                    mismatched.append((k, tuple(loaded_state_dict[k].shape), tuple(own[k].shape)))
                else:
                    toload[k] = loaded_state_dict[k]
        print("You can ignore the keys with `position_ids` or from task heads")
        strict = True
        unexpected = load_keys - model_keys
        if unexpected:
            strict = False
            print("=========================Unexpected==================================")
            print(f"\tIn total {len(unexpected)}, {sorted(unexpected)}")
        missing = model_keys - load_keys
        if missing:
            strict = False
            print("===========================Missing===================================")
            print(f"\tIn total {len(missing)}, {sorted(missing)}")
        if mismatched:
            strict = False
            print("======================Shape Mismatched===============================")
            print(f"\tIn total {len(mismatched)}, {sorted(mismatched)}")
        self.load_state_dict(toload, strict=strict)
        # emb_len / emb_pos resizing exactly as model.py:404-429 (getattr on a dict: always the defaults 6 / 14)
        lf, lp = 6, 14
        with torch.no_grad():
            if lf < self.enc_img.max_size_frame:
                self.enc_img.emb_len.data[:, :lf].copy_(loaded_state_dict["enc_img.emb_len"])
            elif lf > self.enc_img.max_size_frame:
                self.enc_img.emb_len.data.copy_(loaded_state_dict["enc_img.emb_len"][:, :self.enc_img.max_size_frame])
            else:
                print("enc_img.enc_len shape matched")
            if lp < self.enc_img.max_size_patch:
                self.enc_img.emb_pos.data[:, :, :lp].copy_(loaded_state_dict["enc_img.emb_pos"])
            elif lp > self.enc_img.max_size_patch:
                self.enc_img.emb_pos.data.copy_(loaded_state_dict["enc_img.emb_pos"][:, :, :self.enc_img.max_size_patch])
            else:
                print("enc_img.emb_pos shape matched")
        self._mark_stale()
