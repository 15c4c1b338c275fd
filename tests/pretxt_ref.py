"""CPU restatement of the pre-text (task token / prompt) callers, composed from the unmodified oracle pieces (oracle/lavender_ref.py):
LAVENDER_Base.get_pretxt / prepro_txt_inputs / get_attn_mask(mask_pretxt=) (model.py:194-307) in front of the QA and captioning forwards.

A pre-text is ("task", row of emb_task) or ("prompt", (ids, mask)) with 1-D prompt ids (broadcast to every text)."""
import numpy as np
import torch

from oracle import lavender_ref as R

TASK_TOK2ID = {"vtm": 0, "mc": 1, "oe": 2, "cap": 3}


def pretxt_feat(P, spec, n):
    """(n, Lp, H) pre-text features: the emb_task row, or the embedded prompt (enc_txt of the (1, Lp) ids, expanded)"""
    if spec[0] == "task":
        return P["emb_task"][spec[1]].view(1, 1, -1).expand(n, -1, -1)
    ids = spec[1][0]
    return R.enc_txt(P, ids.view(1, -1)).expand(n, -1, -1)


def pretxt_ids(spec, n, label_pretxt):
    """(ids, mask) prepended to txt / mask_txt; label_pretxt=False: the QA callers' prepro_pretxt (-1 at every pre-text position)"""
    if spec[0] == "task":
        ids, m = torch.zeros(n, 1, dtype=torch.long), torch.ones(n, 1, dtype=torch.long)
    else:
        ids, m = spec[1][0].view(1, -1).expand(n, -1), spec[1][1].view(1, -1).expand(n, -1)
    return (ids if label_pretxt else torch.full_like(ids, -1)), m


def seq2seq_mask(m_prefix, Lt):
    """get_attn_mask "seq2seq" with the pre-text in the fully visible prefix: (B, Lfull + Lt, Lfull + Lt), causal from Lfull = Lv + Lp"""
    B, Lf = m_prefix.shape
    L = Lf + Lt
    mask = torch.zeros((B, L, L), dtype=torch.long)
    mask[:, :, :Lf] = m_prefix[:, None, :]
    mask[:, Lf:, Lf:] = torch.tril(torch.ones((B, Lt, Lt), dtype=torch.long))
    return mask


def encoder(P, x, mask, heads):
    add = R.extended_mask(mask)
    for i in range(R.n_fusion_layers(P)):
        x = R.bert_layer(P, f"trsfr.layer.{i}", x, add, heads)
    return x


def qa_forward(P, batch, size, heads, spec):
    """LAVENDER_QAOE_MLM / QAMC forward with a pre-text: logits (B, Lp + X, V), labels -1 at the pre-text"""
    f_img, m_img = R.enc_video(P, batch["img"], size)
    txt, mask, ans = batch["txt"], batch["mask"], batch["mask_ans"]
    n = txt.shape[0]
    f_txt = torch.cat([pretxt_feat(P, spec, n), R.enc_txt(P, txt)], 1)
    ids, m = pretxt_ids(spec, n, False)
    x = encoder(P, torch.cat([f_img, f_txt], 1), torch.cat([m_img, m, mask], 1), heads)
    return R.mlm_head(P, x[:, f_img.shape[1]:]), torch.cat([ids, ans], 1)


def retmc_forward(P, batch, size, heads, spec):
    """LAVENDER_RetMC_MLM forward with a pre-text: logits (B * O, Lp + X, V), labels (B, O, Lp + X)"""
    txt, mask, ans = batch["txt"], batch["mask"], batch["mask_ans"]
    B, O, X = txt.shape
    f_img, m_img = R.enc_video(P, batch["img"], size)
    n = B * O
    f_txt = torch.cat([pretxt_feat(P, spec, n), R.enc_txt(P, txt.flatten(0, 1))], 1)
    ids, m = pretxt_ids(spec, n, False)
    vi = np.repeat(np.arange(B), O)
    x = encoder(P, torch.cat([f_img[vi], f_txt], 1), torch.cat([m_img[vi], m, mask.flatten(0, 1)], 1), heads)
    return R.mlm_head(P, x[:, f_img.shape[1]:]), torch.cat([ids, ans.flatten(0, 1)], 1).view(B, O, -1)


def captioning_forward(P, batch, size, heads, spec):
    """LAVENDER_Captioning.encode_forward with a pre-text (model_for_captioning.py:61-95): seq2seq mask causal from Lv + Lp, labels -1 at
    the pre-text"""
    img, txt, mask, ans = batch["img"], batch["txt"], batch["mask"], batch["ans_mtm"]
    f_img, m_img = R.enc_video(P, img, size)
    n, X = txt.shape
    pf = pretxt_feat(P, spec, n)
    Lp = pf.shape[1]
    ids, _ = pretxt_ids(spec, n, True)
    ans = torch.cat([ids, ans], 1).clone()
    ans[:, :Lp] = -1
    full = torch.cat([m_img, torch.ones(n, Lp, dtype=torch.long)], 1)
    x = encoder(P, torch.cat([f_img, pf, R.enc_txt(P, txt)], 1), seq2seq_mask(full, X), heads)
    return dict(out=R.mlm_head(P, x[:, f_img.shape[1]:]), ans=ans)


def retrieval_forward(P, batch, size, heads, spec, ids=R.SPECIAL):
    """LAVENDER_Retrieval_MLM.forward with a pre-text (main_retrieval_mlm.py:50-91, the pre-text prepended to every pair's text): logits
    (B * B, Lp + X, V), labels -1 but the last position (true / false)"""
    img, txt, mask, vid = batch["img"], batch["txt"], batch["mask"], list(batch["vid"])
    B, X = txt.shape
    f_img, m_img = R.enc_video(P, img, size)
    f_txt = torch.cat([pretxt_feat(P, spec, B), R.enc_txt(P, txt)], 1)
    _, m = pretxt_ids(spec, B, True)
    m_txt = torch.cat([m, mask], 1)
    vi, ti = np.repeat(np.arange(B), B), np.tile(np.arange(B), B)
    x = encoder(P, torch.cat([f_img[vi], f_txt[ti]], 1), torch.cat([m_img[vi], m_txt[ti]], 1), heads)
    ans = torch.full((B * B, f_txt.shape[1]), -1, dtype=torch.long)
    ans[:, -1] = torch.tensor([ids["true"] if vid[i] == vid[j] else ids["false"] for i, j in zip(vi, ti)])
    return R.mlm_head(P, x[:, f_img.shape[1]:]), ans


def pretrain_forward(P, batch, size, heads, spec, vtm_batch=4, ids=R.SPECIAL):
    """LAVENDER_Pretrain_MLM.forward with the "vtm" pre-text (main_pretrain_mlm.py:55-119): the MTM pass on the plain text, the VTM pass on
    [pre-text ; text] over R.vtm_pairs (same numpy draws)"""
    img, txt, mask = batch["img"], batch["txt"], batch["mask"]
    B, X = txt.shape
    O = min(B, vtm_batch)
    f_img, m_img = R.enc_video(P, img, size)
    f_txt = R.enc_txt(P, txt)
    Lv = f_img.shape[1]
    out_mtm = R.mlm_head(P, encoder(P, torch.cat([f_img, f_txt], 1), torch.cat([m_img, mask], 1), heads)[:, Lv:])
    f_p = torch.cat([pretxt_feat(P, spec, B), f_txt], 1)
    _, m = pretxt_ids(spec, B, True)
    m_p = torch.cat([m, mask], 1)
    vi, ti, tr = R.vtm_pairs(B, O)
    out_vtm = R.mlm_head(P, encoder(P, torch.cat([f_img[vi], f_p[ti]], 1), torch.cat([m_img[vi], m_p[ti]], 1), heads)[:, Lv:])
    ans_vtm = torch.full((B * O, f_p.shape[1]), -1, dtype=torch.long)
    ans_vtm[:, -1] = torch.where(torch.from_numpy(tr), ids["true"], ids["false"])
    return dict(out_mtm=out_mtm, out_vtm=out_vtm, ans_vtm=ans_vtm, ans_mtm=batch.get("ans_mtm"))
