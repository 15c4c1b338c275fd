"""Caption generation for LAVENDER_Captioning (model_for_captioning.py:139-500, driven by main_caption.py:98-125): greedy, sampled
and beam-search decoding.

Under the seq2seq mask video rows never see text and text row i never sees rows after i, so the fusion encoder's keys and
values can be cached exactly:
  * prefix, once per batch: the video rows alone through every layer (lav_bert_layer_fwd, eval); each layer's qkv buffer is kept,
    its k | v columns are the video part of that layer's cache (read in place by the decode attention);
  * step t: two rows per clip -- the token chosen at step t - 1 (position t - 1; its k / v were those of [MASK] the step before and are
    recomputed) and a fresh [MASK] at position t -- through every layer (lav_bert_layer_decode); the real token's k / v go to the
    per-layer text cache (B, heads, max_len, 64); the MLM head runs on the B [MASK] rows only, with fp32 logits.
Greedy steps choose the token on the device (lav_greedy_step): a whole greedy generation makes no host synchronisation until
the final copy.  Sampling (do_sample) draws with torch ops on the fp32 [MASK] logits, as the reference does.
LAV_CAP_KV=0 runs the reference's literal loop instead: the whole fusion encoder over Lv + cur_len + 1 rows for every token.
Beam search (num_beams > 1, the HF-2.x _generate_beam_search + BeamHypotheses that Oscar / SwinBERT used): each clip keeps num_beams rows
that share the clip's prefix in place; per step lav_beam_step (penalty, top 2 * beams of the log-softmax), lav_beam_select (the clip's
candidates, hypotheses, next beams) and lav_beam_reparent (the text caches follow the parents) keep the whole generation on the device.
LAV_CAP_KV=0 runs the reference-shaped loop with the video features expanded num_beams times and the bookkeeping on the host."""
import os

import numpy as np
import torch

from . import engine as E
from . import hip as K

KV = os.environ.get("LAV_CAP_KV", "1") != "0"


class GenConfig:
    """The generation arguments generate() reads from args (model_for_captioning.py:150-162), checked."""

    def __init__(self, args, X):
        get = args.get if hasattr(args, "get") else (lambda k, d: getattr(args, k, d))
        self.max_len = int(get("max_gen_length", 20))
        self.do_sample = bool(get("do_sample", False))
        self.temperature = float(get("gen_temperature", 1.0))
        self.top_k = int(get("top_k", 0))
        self.top_p = float(get("top_p", 1.0))
        self.penalty = float(get("repetition_penalty", 1.0))
        for k in ("num_beams", "num_keep_best", "num_return_sequences", "num_fsm_states"):
            if int(get(k, 1)) != 1:
                raise NotImplementedError(f"caption generation: {k} = {get(k, 1)}; only 1 is supported (the reference has no beam search: "
                                          "with num_beams > 1 it expands the video features but not the ids and fails)")
        if self.max_len > X:
            raise ValueError(f"caption generation: max_gen_length {self.max_len} exceeds the text length {X} of the batch (the reference slices "
                             "its (Lv + X)-wide seq2seq mask to Lv + max_gen_length rows)")
        if self.max_len < 2:
            raise ValueError(f"caption generation: max_gen_length {self.max_len} < 2 generates nothing")


class BeamConfig:
    """The beam-search arguments of generate() (num_beams > 1), checked: num_beams 2..8, num_keep_best 1..num_beams, length_penalty,
    early_stopping, repetition_penalty, max_gen_length.  top_k / top_p / gen_temperature are ignored (the reference's non-sampling path)."""

    def __init__(self, args, X):
        get = args.get if hasattr(args, "get") else (lambda k, d: getattr(args, k, d))
        self.num_beams = int(get("num_beams", 1))
        self.keep = int(get("num_keep_best", 1))
        self.max_len = int(get("max_gen_length", 20))
        self.penalty = float(get("repetition_penalty", 1.0))
        self.length_penalty = float(get("length_penalty", 1.0))
        self.early_stopping = bool(get("early_stopping", False))
        if bool(get("do_sample", False)):
            raise NotImplementedError("caption generation: do_sample with num_beams > 1 (beam sampling) is not built")
        for k in ("num_return_sequences", "num_fsm_states"):
            if int(get(k, 1)) != 1:
                raise NotImplementedError(f"caption generation: {k} = {get(k, 1)}; only 1 is supported")
        if not 2 <= self.num_beams <= K_BEAM_MAX:
            raise ValueError(f"caption generation: num_beams {self.num_beams}; beam search takes 2..{K_BEAM_MAX}")
        if not 1 <= self.keep <= self.num_beams:
            raise ValueError(f"caption generation: num_keep_best {self.keep}; it takes 1..num_beams ({self.num_beams})")
        if self.max_len > X:
            raise ValueError(f"caption generation: max_gen_length {self.max_len} exceeds the text length {X} of the batch")
        if self.max_len < 2:
            raise ValueError(f"caption generation: max_gen_length {self.max_len} < 2 generates nothing")

    def norm(self, n):
        """n ** length_penalty rounded to fp32: the length normaliser of both bookkeeping paths"""
        return float(np.float32(float(n) ** self.length_penalty))


K_BEAM_MAX = 8                             # LAV_BEAM_MAX


def make_config(args, X):
    """GenConfig for num_beams 1 (greedy / sampling), BeamConfig above"""
    get = args.get if hasattr(args, "get") else (lambda k, d: getattr(args, k, d))
    return BeamConfig(args, X) if int(get("num_beams", 1)) != 1 else GenConfig(args, X)


# ---- host pieces shared by every path (pure torch) ---------------------------------------------------------------------------
def apply_repetition_penalty(logits, prev_ids, penalty):
    """in place: every distinct id of prev_ids[b] scales logits[b, id] once -- multiplied when negative, divided otherwise"""
    if penalty == 1.0:
        return logits
    v = logits.gather(1, prev_ids)
    logits.scatter_(1, prev_ids, torch.where(v < 0, v * penalty, v / penalty))      # duplicates write the same value
    return logits


def top_k_top_p_filtering(logits, top_k=0, top_p=1.0, filter_value=-float("inf")):
    """the reference's filter (model_for_captioning.py:502-534, min_tokens_to_keep 1), in place"""
    if top_k > 0:
        top_k = min(top_k, logits.size(-1))
        logits[logits < torch.topk(logits, top_k)[0][..., -1, None]] = filter_value
    if top_p < 1.0:
        srt, idx = torch.sort(logits, descending=True)
        drop = torch.cumsum(torch.softmax(srt, dim=-1), dim=-1) > top_p
        drop[..., 1:] = drop[..., :-1].clone()
        drop[..., 0] = False
        logits[drop.scatter(1, idx, drop)] = filter_value
    return logits


def choose_tokens(logits, prev_ids, cfg, generator=None):
    """one step of _generate_no_beam_search on fp32 logits (B, V): penalty, then temperature + filtering + multinomial or argmax;
    returns (token, log_softmax score of the token under the logits it was drawn from)"""
    logits = apply_repetition_penalty(logits, prev_ids, cfg.penalty)
    if cfg.do_sample:
        if cfg.temperature != 1.0:
            logits = logits / cfg.temperature
        logits = top_k_top_p_filtering(logits, cfg.top_k, cfg.top_p)
        tok = torch.multinomial(torch.softmax(logits, dim=-1), num_samples=1, generator=generator).squeeze(1)
    else:
        tok = torch.argmax(logits, dim=-1)
    score = torch.log_softmax(logits, dim=-1).gather(1, tok[:, None]).squeeze(1)
    return tok, score


def record_step(ids, cur, tok, score, state, pad_id, eos_id):
    """the bookkeeping of one step: finished rows emit [PAD] and do not count; a row finishes on [SEP].  state = (unfinished int32,
    score_sum fp32, count fp32), updated in place (what lav_greedy_step does on the device)."""
    unf, ssum, cnt = state
    u = unf.bool()
    t = torch.where(u, tok, torch.full_like(tok, pad_id))
    ids[:, cur] = t
    ssum += torch.where(u, score.float(), torch.zeros_like(ssum))
    cnt += u.float()
    unf.copy_((u & (t != eos_id)).to(unf.dtype))
    return t


def finish_generation(ids, cur_len, max_len, unfinished, score_sum, count, pad_id, eos_id):
    """end of _generate_no_beam_search: ids (B, >= cur_len) holds [CLS] + the generated tokens in columns < cur_len.  When the loop ran
    to max_len, still-unfinished rows get [SEP] in the last column; the score is the mean over the counted steps; ids are padded with
    [PAD] to max_len.  Returns (ids (B, 1, max_len) int64, logprob (B, 1))."""
    B = ids.shape[0]
    out = torch.full((B, max_len), pad_id, dtype=torch.long, device=ids.device)
    out[:, :cur_len] = ids[:, :cur_len]
    if cur_len == max_len:
        out[:, -1] = torch.where(unfinished.bool(), torch.full_like(out[:, -1], eos_id), out[:, -1])
    logprob = score_sum.float() / count.float()
    return out.unsqueeze(1), logprob.unsqueeze(1)


# ---- the key / value cached decoder --------------------------------------------------------------------------------------------
class KVDecoder:
    """Buffers and launches of the cached path for one batch of at most KV_MAX_CLIPS row groups: the prefix pass in the constructor, then
    step(t) for t = 1 .. max_len - 1.  beams > 1: each clip decodes `beams` row groups (row group clip * beams + beam) that read the clip's
    prefix in place; the text caches come in two sets, and swap_caches() makes the other set current (lav_beam_reparent fills it)."""

    def __init__(self, model, feat_img, mask_img, max_len, beams=1):
        self.m = model
        model.arena()                                          # the layers' constants below are arena addresses
        dev = feat_img.device
        clips, Lv, H = feat_img.shape
        B = clips * beams
        assert B <= KV_MAX_CLIPS, f"KVDecoder: {clips} clips x {beams} beams, at most {KV_MAX_CLIPS} rows at once (caption_decode.generate splits larger batches)"
        self.clips, self.beams = clips, beams
        layers = model.trsfr.layer
        heads = layers[0].num_heads
        F = layers[0].intermediate.dense.weight.shape[0]
        self.B, self.Lv, self.H, self.heads, self.F, self.max_len = B, Lv, H, heads, F, max_len
        self.km = mask_img.to(torch.int32).contiguous()
        e, bf16, f32 = torch.empty, torch.bfloat16, torch.float32
        R = 2 * B
        # prefix: the video rows through every layer, each layer's qkv kept
        x = feat_img.reshape(clips * Lv, H).contiguous()
        resln = None
        self.prefix_qkv, consts = [], []
        for lyr in layers:
            x, resln, qkv = E.bert_layer_eval_c(x, resln, lyr, self.km, clips, Lv)
            self.prefix_qkv.append(qkv)
            consts.append(E._layer_consts(lyr))
        # per-layer text caches and the step's workspaces
        self.cache = [(torch.zeros((B, heads, max_len, 64), dtype=bf16, device=dev), torch.zeros((B, heads, max_len, 64), dtype=bf16, device=dev))
                      for _ in layers]
        self.cache_alt = ([(torch.zeros_like(k), torch.zeros_like(v)) for k, v in self.cache] if beams > 1 else None)
        self.emb = e((R, H), dtype=bf16, device=dev)
        self.qkv, self.cx, self.x1, self.h = e((R, 3 * H), dtype=bf16, device=dev), e((R, H), dtype=bf16, device=dev), e((R, H), dtype=bf16, device=dev), \
            e((R, F), dtype=bf16, device=dev)
        self.pre1, self.pre2, self.x1_32 = e((R, H), dtype=f32, device=dev), e((R, H), dtype=f32, device=dev), e((R, H), dtype=f32, device=dev)
        self.stats = e((2 * R,), dtype=f32, device=dev)
        self.y = [e((R, H), dtype=bf16, device=dev) for _ in range(2)]
        self.y32 = [e((R, H), dtype=f32, device=dev) for _ in range(2)]
        # the key-split partials of the decode attention: sized for the step that needs the most splits (lav_attention_decode also checks the
        # capacity it is given and refuses a smaller workspace)
        splits = max(K.attention_decode_splits(K.attn_decode_desc(B, heads, 2, Lv, t - 1, 1, max_len, None, None, None, None, None, None))
                     for t in range(1, max_len))
        self.partials = e((B * heads * splits * 2 * 66,), dtype=f32, device=dev)
        self.descs = []
        for i, c in enumerate(consts):
            p = c["params"]
            d = K.L.BertLayerDecodeDesc(B, 2, H, heads, F, Lv, 0, 1, max_len, c["eps"], c["eps2"], self.km.data_ptr(), *p,
                                        self.prefix_qkv[i].data_ptr(), self.cache[i][0].data_ptr(), self.cache[i][1].data_ptr(),
                                        0, 0, 0, self.qkv.data_ptr(), self.cx.data_ptr(), self.pre1.data_ptr(), self.x1.data_ptr(),
                                        self.x1_32.data_ptr(), self.h.data_ptr(), self.pre2.data_ptr(), self.stats.data_ptr(),
                                        self.y[i % 2].data_ptr(), self.y32[i % 2].data_ptr(), self.partials.data_ptr(), self.partials.numel())
            d.x = self.emb.data_ptr() if i == 0 else self.y[(i - 1) % 2].data_ptr()
            d.x_res = self.emb.data_ptr() if i == 0 else self.y32[(i - 1) % 2].data_ptr()
            d.x_res_bf16 = 1 if i == 0 else 0
            self.descs.append(d)
        self.last_y = self.y[(len(layers) - 1) % 2]
        # head
        head = model.fc_mtm.predictions
        self.V = head.decoder.weight.shape[0]
        self.t1, self.tn = e((B, H), dtype=bf16, device=dev), e((B, H), dtype=bf16, device=dev)
        self.logits = e((B, self.V), dtype=f32, device=dev)
        # step inputs: the known token (written by the greedy step) and [MASK], positions t - 1 and t
        self.step_ids = torch.full((B, 2), model.mask_token_id, dtype=torch.long, device=dev)
        self.step_ids[:, 0] = model.cls_token_id
        tt = torch.arange(max_len, dtype=torch.int32, device=dev)
        self.pos = torch.stack([tt - 1, tt], 1)[:, None, :].expand(max_len, B, 2).contiguous()

    def step(self, t):
        """the [MASK]-row logits (B, V) fp32 of step t (cur_len = t): the known token at position t - 1 is step_ids[:, 0]"""
        m = self.m
        emb = m.enc_txt.emb_txt
        K.text_embed_rows(self.step_ids, self.pos[t], self.H, emb.word_embeddings.weight.data, emb.position_embeddings.weight.data,
                          emb.token_type_embeddings.weight.data, emb.LayerNorm.weight.data, emb.LayerNorm.bias.data, emb.LayerNorm.eps, self.emb)
        for d in self.descs:
            d.n_cached = t - 1
            if self.beams == 1:
                K.bert_layer_decode(d)
            else:
                K.bert_layer_decode_beam(d, self.beams)
        tr, dec = m.fc_mtm.predictions.transform, m.fc_mtm.predictions.decoder
        ymask = self.last_y.view(self.B, 2, self.H)[:, 1]
        K.gemm_skinny(ymask, E.W16(tr.dense.weight), self.B, self.H, self.H, self.t1, K.SKINNY_GELU, bias=tr.dense.bias.data)
        K.layernorm_fwd(self.t1, self.B, self.H, tr.LayerNorm.weight.data, tr.LayerNorm.bias.data, tr.LayerNorm.eps, out=self.tn, want_stats=False)
        K.gemm_skinny(self.tn, E.W16(dec.weight), self.B, self.V, self.H, self.logits, K.SKINNY_F32, bias=dec.bias.data)
        return self.logits

    def swap_caches(self):
        """beams > 1: the other cache set becomes the one the layers read and append to"""
        self.cache, self.cache_alt = self.cache_alt, self.cache
        for d, (k, v) in zip(self.descs, self.cache):
            d.cache_k, d.cache_v = k.data_ptr(), v.data_ptr()


def encode_prefix(model, img, pretxt=None):
    """the fully visible prefix of every clip: its video rows, then the pre-text (model_for_captioning.py:160-176, 258-290: the task token or the
    embedded prompt sits between the video and the caption, whose positions still count from 0) -- (feat (B, Lv + Lp, H), key mask (B, Lv + Lp)).
    The prefix's rows see only prefix keys, so the cached path runs it once per clip like the video rows alone (Lv' = Lv + Lp) and the literal
    path masks with causal_from = Lv + Lp.  pretxt: LAVENDER_Base._pretxt_spec("cap", prompt), or None."""
    feat_img, mask_img = model.enc_img(img)
    if pretxt is None:
        return feat_img, mask_img
    B, H = feat_img.shape[0], feat_img.shape[2]
    if pretxt[0] == "task":
        pf = E.W16(model.emb_task)[pretxt[1]].view(1, 1, H)
    else:
        pf = model._embed_prompt(pretxt[1][0], feat_img.device)
    pf = pf.expand(B, -1, -1) if pf.shape[0] == 1 else pf
    assert pf.shape[0] == B, f"a per-clip prompt needs one row block per clip ({pf.shape[0]} for {B} clips)"
    feat = torch.cat([feat_img, pf.to(feat_img.dtype)], 1)
    mask = torch.cat([mask_img, torch.ones((B, pf.shape[1]), dtype=mask_img.dtype, device=mask_img.device)], 1)
    return feat, mask


def recompute_logits(model, feat_img, mask_img, ids, cur_len):
    """the reference's step (model_for_captioning.py:96-130, past is None): text [ids[:, :cur_len] ; MASK] at positions 0..cur_len, the whole
    fusion encoder over Lv + cur_len + 1 rows under the seq2seq mask, the MLM head at the [MASK] row; fp32 (B, V)"""
    B, Lv, _ = feat_img.shape
    inp = torch.cat([ids[:, :cur_len], torch.full((B, 1), model.mask_token_id, dtype=torch.long, device=ids.device)], 1)
    f_txt = model.enc_txt(inp)
    key_mask = torch.cat([mask_img, torch.ones((B, cur_len + 1), dtype=mask_img.dtype, device=mask_img.device)], 1)
    hid = model._encode(torch.cat([feat_img, f_txt], 1), key_mask, causal_from=Lv)
    return model.fc_mtm(hid[:, Lv + cur_len].contiguous()).float()


KV_MAX_CLIPS = 32          # the cached path decodes at most this many clips at once: 2 rows per clip through the skinny GEMMs (M <= 64)


def generate(model, img, X, cfg, kv=None, generator=None, forced_ids=None, step_logits=None, pretxt=None):
    """(ids (B, 1, max_len), logprob (B, 1)).  forced_ids (B, max_len): teacher forcing (tests; the chosen tokens are replaced by these
    before the next step); step_logits: a list that receives each step's fp32 [MASK] logits (B, V) before the penalty.  The cached path
    decodes larger batches in chunks of KV_MAX_CLIPS clips (every clip's caption is independent of the others)."""
    kv = KV if kv is None else kv
    B = img.shape[0]
    if not kv or B <= KV_MAX_CLIPS:
        return _generate(model, img, X, cfg, kv, generator, forced_ids, step_logits, pretxt)
    ids, lps, chunk_steps = [], [], []
    for s in range(0, B, KV_MAX_CLIPS):
        st = [] if step_logits is not None else None
        i, lp = _generate(model, img[s:s + KV_MAX_CLIPS], X, cfg, kv, generator,
                          None if forced_ids is None else forced_ids[s:s + KV_MAX_CLIPS], st, pretxt)
        ids.append(i)
        lps.append(lp)
        chunk_steps.append(st)
    if step_logits is not None:
        step_logits.extend(torch.cat(parts, 0) for parts in zip(*chunk_steps))
    return torch.cat(ids, 0), torch.cat(lps, 0)


def _generate(model, img, X, cfg, kv, generator, forced_ids, step_logits, pretxt=None):
    pad_id, eos_id, cls_id = model.pad_token_id, model.sep_token_id, model.cls_token_id
    feat_img, mask_img = encode_prefix(model, img, pretxt)
    B, dev, L = feat_img.shape[0], feat_img.device, cfg.max_len
    ids = torch.full((B, L), pad_id, dtype=torch.long, device=dev)
    ids[:, 0] = cls_id
    state = (torch.ones(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.float32, device=dev),
             torch.zeros(B, dtype=torch.float32, device=dev))
    dec = KVDecoder(model, feat_img, mask_img, L) if kv else None
    cur = 1
    while cur < L:
        logits = dec.step(cur) if kv else recompute_logits(model, feat_img, mask_img, ids, cur)
        if step_logits is not None:
            step_logits.append(logits.clone())
        if kv and not cfg.do_sample:
            K.greedy_step(logits, dec.V, ids, cur, cfg.penalty, *state, pad_id, eos_id, next_ids=dec.step_ids, ld_next=2)
        else:
            tok, score = choose_tokens(logits.clone() if kv else logits, ids[:, :cur], cfg, generator)
            t = record_step(ids, cur, tok, score, state, pad_id, eos_id)
            if kv:
                dec.step_ids[:, 0] = t
        if forced_ids is not None:
            ids[:, cur] = forced_ids[:, cur]
            if kv:
                dec.step_ids[:, 0] = forced_ids[:, cur]
        cur += 1
        if not kv and int(state[0].max()) == 0:           # the reference's early stop (the cached path runs on: identical outputs)
            break
    return finish_generation(ids, cur, L, *state, pad_id, eos_id)


# ---- beam search --------------------------------------------------------------------------------------------------------------------
class BeamState:
    """The state of a beam search over `clips` clips x nb beams (row r = clip * nb + beam), as lav_beam_select reads and writes it:
    beam_scores (R,) fp32, ids (R, L) history, parent (R,) int32 (global row), the hypothesis store hyp_ids (clips, K, L) / hyp_score (clips, K) /
    hyp_seq (clips, K) insertion numbers, state (clips, 3) int32 = (held, done, insertions so far), worst (clips,) fp32."""

    def __init__(self, clips, cfg, cls_id, pad_id, device):
        nb, K, L = cfg.num_beams, cfg.keep, cfg.max_len
        R = clips * nb
        self.beam_scores = torch.zeros(R, dtype=torch.float32, device=device)
        self.beam_scores.view(clips, nb)[:, 1:] = -1e9
        self.ids = torch.full((R, L), pad_id, dtype=torch.long, device=device)
        self.ids[:, 0] = cls_id
        self.parent = torch.arange(R, dtype=torch.int32, device=device)
        self.hyp_ids = torch.full((clips, K, L), pad_id, dtype=torch.long, device=device)
        self.hyp_score = torch.zeros((clips, K), dtype=torch.float32, device=device)
        self.hyp_seq = torch.zeros((clips, K), dtype=torch.int32, device=device)
        self.state = torch.zeros((clips, 3), dtype=torch.int32, device=device)
        self.worst = torch.full((clips,), 1e9, dtype=torch.float32, device=device)

    def tensors(self):
        return (self.beam_scores, self.ids, self.parent, self.hyp_ids, self.hyp_score, self.hyp_seq, self.state, self.worst)


def row_candidates(logprobs, k):
    """per row of fp32 scores (R, V): the k best (value descending, lower index on a tie -- torch.topk's tie order is not relied on);
    returns (values (R, k) fp32, indices (R, k) int32) on the CPU"""
    x = logprobs.float().cpu()
    thr = torch.topk(x, k, dim=1).values[:, -1:]
    vals, idx = torch.empty(x.shape[0], k), torch.empty(x.shape[0], k, dtype=torch.int32)
    for r in range(x.shape[0]):
        cand = torch.nonzero(x[r] >= thr[r]).flatten().numpy()
        v = x[r, cand].numpy()
        order = np.lexsort((cand, -v))[:k]
        vals[r], idx[r] = torch.from_numpy(v[order].copy()), torch.from_numpy(cand[order].astype(np.int32))
    return vals, idx


def host_beam_candidates(logits, ids, cur, penalty, beam_scores, nb):
    """the host restatement of lav_beam_step: penalty (on a copy), log_softmax + beam score, each row's top 2 * nb"""
    lg = apply_repetition_penalty(logits.float().clone(), ids[:, :cur].to(logits.device), penalty)
    return row_candidates(torch.log_softmax(lg, dim=-1) + beam_scores.to(lg.device)[:, None], 2 * nb)


def host_beam_select(cand_score, cand_word, st, cur, cfg, V, eos_id, pad_id):
    """lav_beam_select restated in plain Python over fp32 values, on a BeamState of CPU tensors (updated in place); returns the next words (R,)"""
    nb, K, L = cfg.num_beams, cfg.keep, cfg.max_len
    k2 = 2 * nb
    f32 = np.float32
    cur_norm, max_norm = f32(cfg.norm(cur)), f32(cfg.norm(L))
    cs, cw = cand_score.cpu().numpy().astype(np.float32), cand_word.cpu().numpy().astype(np.int64)
    clips = st.state.shape[0]
    old_ids = st.ids.clone()
    words = torch.full((clips * nb,), pad_id, dtype=torch.long)
    for c in range(clips):
        r0 = c * nb
        cands = [(cs[r0 + b, j], b * V + cw[r0 + b, j]) for b in range(nb) for j in range(k2)]
        cands.sort(key=lambda t: (-t[0], t[1]))
        cands = cands[:k2]
        held, done, seq = (int(v) for v in st.state[c])
        worst = f32(st.worst[c].item())
        hs, hq = st.hyp_score[c].numpy(), st.hyp_seq[c].numpy()
        nxt = [(b, pad_id, f32(st.beam_scores[r0 + b].item())) for b in range(nb)]
        if not done and held == K and (cfg.early_stopping or worst >= f32(cands[0][0] / max_norm)):
            done = 1
        if not done:
            last, nn = cur + 1 == L, 0
            for sc, flat in cands:
                if nn >= nb:
                    break
                b, w = int(flat // V), int(flat % V)
                if w == eos_id or last:
                    s = f32(sc / cur_norm)
                    if held < K:                          # a plain add
                        slot, held = held, held + 1
                        hs[slot], hq[slot] = s, seq
                        worst = min(worst, s)
                    elif s > worst:                       # overflow: the lowest score goes, the earliest insertion among equals
                        slot = min(range(K), key=lambda q: (hs[q], hq[q]))
                        hs[slot], hq[slot] = s, seq
                        worst = f32(hs.min())
                    else:
                        continue
                    seq += 1
                    st.hyp_ids[c, slot] = pad_id
                    st.hyp_ids[c, slot, :cur] = old_ids[r0 + b, :cur]
                    st.hyp_ids[c, slot, cur] = eos_id
                else:
                    nxt[nn] = (b, w, sc)
                    nn += 1
        st.state[c] = torch.tensor([held, done, seq], dtype=torch.int32)
        st.worst[c] = float(worst)
        for b, (pb, w, sc) in enumerate(nxt):
            r = r0 + b
            st.ids[r, :cur] = old_ids[r0 + pb, :cur]
            st.ids[r, cur] = w
            st.parent[r] = r0 + pb
            st.beam_scores[r] = float(sc)
            words[r] = w
    return words


def finish_beams(hyp_ids, hyp_score, hyp_seq):
    """hypotheses -> (ids (clips, K, L), logprob (clips, K)): score descending, the earlier insertion first among equals (torch ops, no sync)"""
    o1 = torch.argsort(hyp_seq, dim=1)
    o2 = torch.sort(hyp_score.gather(1, o1), dim=1, descending=True, stable=True).indices
    o = o1.gather(1, o2)
    return hyp_ids.gather(1, o[..., None].expand(-1, -1, hyp_ids.shape[2])), hyp_score.gather(1, o)


def generate_beam(model, img, X, cfg, kv=None, forced=None, step_logits=None, trace=None, pretxt=None):
    """beam search: (ids (B, K, max_len) int64, logprob (B, K) fp32).  Test hooks: forced = (parents (B, max_len - 2, nb) in-clip beam indices,
    words (B, max_len - 2, nb)) replaces the selection of steps 1 .. max_len - 2 (teacher forcing of the beams); step_logits receives each
    step's fp32 [MASK] logits (B * nb, V) before the penalty; trace receives per step (parents (B, nb) in-clip, words (B, nb), the clip's
    2 * nb candidate scores (B, 2 nb) in order) -- the cached path fills only the first two.  The cached path decodes at most
    KV_MAX_CLIPS // num_beams clips at once (2 rows per beam through the skinny GEMMs, M <= 64)."""
    kv = KV if kv is None else kv
    B, per = img.shape[0], KV_MAX_CLIPS // cfg.num_beams
    if not kv or B <= per:
        return _generate_beam(model, img, cfg, kv, forced, step_logits, trace, pretxt)
    ids, lps, steps, traces = [], [], [], []
    for s in range(0, B, per):
        sl, tr = ([] if step_logits is not None else None), ([] if trace is not None else None)
        f = None if forced is None else (forced[0][s:s + per], forced[1][s:s + per])
        i, lp = _generate_beam(model, img[s:s + per], cfg, kv, f, sl, tr, pretxt)
        ids.append(i)
        lps.append(lp)
        steps.append(sl)
        traces.append(tr)
    if step_logits is not None:
        step_logits.extend(torch.cat(parts, 0) for parts in zip(*steps))
    if trace is not None:
        trace.extend(tuple(torch.cat(x, 0) if x[0] is not None else None for x in zip(*parts)) for parts in zip(*traces))
    return torch.cat(ids, 0), torch.cat(lps, 0)


def _apply_forced(forced, cur, st, clips, nb, dec):
    """teacher forcing of step cur (tests): the selection is replaced by the forced parents / words (the hypothesis store is left as it is)"""
    dev = st.ids.device
    fp, fw = forced[0][:, cur - 1].to(dev), forced[1][:, cur - 1].to(dev)
    par = (torch.arange(clips, device=dev)[:, None] * nb + fp).flatten()
    st.ids[:, :cur] = st.ids_before[par, :cur]
    st.ids[:, cur] = fw.flatten()
    st.parent.copy_(par.to(torch.int32))
    if dec is not None:
        dec.step_ids[:, 0] = fw.flatten()


def _generate_beam(model, img, cfg, kv, forced, step_logits, trace, pretxt=None):
    pad_id, eos_id, cls_id = model.pad_token_id, model.sep_token_id, model.cls_token_id
    feat_img, mask_img = encode_prefix(model, img, pretxt)
    clips, dev, L, nb = feat_img.shape[0], feat_img.device, cfg.max_len, cfg.num_beams
    R = clips * nb
    if kv:
        st = BeamState(clips, cfg, cls_id, pad_id, dev)
        dec = KVDecoder(model, feat_img, mask_img, L, beams=nb)
        V = dec.V
        cand_s = torch.empty((R, 2 * nb), dtype=torch.float32, device=dev)
        cand_w = torch.empty((R, 2 * nb), dtype=torch.int32, device=dev)
        sel = K.beam_select_desc(clips, nb, cfg.keep, V, L, cfg.early_stopping, eos_id, pad_id, cand_s, cand_w, st.beam_scores, st.ids, st.parent,
                                 st.hyp_ids, st.hyp_score, st.hyp_seq, st.state, st.worst, next_ids=dec.step_ids, ld_next=2)
        rep = [K.beam_reparent_desc(dec.cache, dec.cache_alt, st.parent, L), K.beam_reparent_desc(dec.cache_alt, dec.cache, st.parent, L)]
        for cur in range(1, L):
            logits = dec.step(cur)
            if step_logits is not None:
                step_logits.append(logits.clone())
            K.beam_step(logits, V, st.ids, cur, cfg.penalty, st.beam_scores, nb, cand_s, cand_w)
            if forced is not None:
                st.ids_before = st.ids.clone()
            K.beam_select(sel, cur, cfg.norm(cur), cfg.norm(L))
            if forced is not None and cur + 1 < L:
                _apply_forced(forced, cur, st, clips, nb, dec)
            if trace is not None:
                trace.append(((st.parent.view(clips, nb) % nb).long(), st.ids[:, cur].view(clips, nb).clone(), None))
            if cur + 1 < L:
                K.beam_reparent(rep[(cur - 1) % 2], cur)
                dec.swap_caches()
        return finish_beams(st.hyp_ids, st.hyp_score, st.hyp_seq)
    # full recompute: the reference-shaped loop over the video features expanded nb times, the bookkeeping on the host
    feat_x, mask_x = feat_img.repeat_interleave(nb, 0), mask_img.repeat_interleave(nb, 0)
    ids, lp = host_beam_search(lambda ids, cur: recompute_logits(model, feat_x, mask_x, ids.to(dev), cur), clips, cfg, cls_id, pad_id, eos_id,
                               forced, step_logits, trace)
    return ids.to(dev), lp.to(dev)


def host_beam_search(step_fn, clips, cfg, cls_id, pad_id, eos_id, forced=None, step_logits=None, trace=None):
    """the beam search with the bookkeeping on the host: step_fn(ids (clips * nb, L) history, cur) gives the fp32 [MASK] logits (clips * nb, V)
    of step cur; hooks as generate_beam.  Stops when every clip is done (the reference's early stop)."""
    nb = cfg.num_beams
    st = BeamState(clips, cfg, cls_id, pad_id, "cpu")
    for cur in range(1, cfg.max_len):
        logits = step_fn(st.ids, cur)
        if step_logits is not None:
            step_logits.append(logits.clone())
        cs, cw = host_beam_candidates(logits, st.ids, cur, cfg.penalty, st.beam_scores, nb)
        if forced is not None:
            st.ids_before = st.ids.clone()
        host_beam_select(cs, cw, st, cur, cfg, logits.shape[1], eos_id, pad_id)
        if forced is not None and cur + 1 < cfg.max_len:
            _apply_forced(forced, cur, st, clips, nb, None)
        if trace is not None:
            merged = torch.sort(cs.view(clips, -1), dim=1, descending=True).values[:, :2 * nb]
            trace.append(((st.parent.view(clips, nb) % nb).long(), st.ids[:, cur].view(clips, nb).clone(), merged))
        if int(st.state[:, 1].min()) == 1:
            break
    return finish_beams(st.hyp_ids, st.hyp_score, st.hyp_seq)
