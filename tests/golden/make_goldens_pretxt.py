"""Golden vectors for the pre-text callers -- task token (enable_task_token) and prompt (enable_prompt), LAVENDER_Base.get_pretxt /
prepro_txt_inputs / get_attn_mask(mask_pretxt=) (model.py:194-307) -- (CONTAINER ONLY -- needs the reference checkout):
  * LAVENDER_QAOE_MLM (main_qaoe_mlm_lsmdc_fib.py:64-93) with the "oe" task token and with a prompt -> pretxt_qaoe_task.npz, pretxt_qaoe_prompt.npz
  * LAVENDER_RetMC_MLM (main_retmc_mlm.py:70-113) with the "vtm" task token                           -> pretxt_retmc_task.npz
  * LAVENDER_Captioning.encode_forward (model_for_captioning.py:54-95, seq2seq) with the "cap" task token and with a prompt
                                                                                                      -> pretxt_cap_task.npz, pretxt_cap_prompt.npz
  * LAVENDER_Retrieval_MLM (main_retrieval_mlm.py:50-91, the per-pair loop) with a prompt             -> pretxt_retrieval_prompt.npz
  * LAVENDER_Pretrain_MLM (main_pretrain_mlm.py:55-119) with the "vtm" task token and with vtm_prompt -> pretxt_pretrain_task.npz,
                                                                                                         pretxt_pretrain_prompt.npz
  * LAVENDER_Captioning.generate (model_for_captioning.py:139-290), greedy, with a prompt, as make_goldens_caption_gen.py drives it
                                                                                                      -> pretxt_cap_gen_prompt.npz
Same recipe as make_goldens_qa.py (micro configs, eval mode, filled parameters): sub-sampled logits, labels, the loss, every parameter's
gradient norm, emb_task's whole gradient and sub-samples of the word / position embedding gradients.

    python tests/golden/make_goldens_pretxt.py
"""
import sys
sys.dont_write_bytecode = True
import importlib
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG  # noqa: E402
from make_goldens import make_batch, sub, BERT_CFGS  # noqa: E402
from make_goldens_variants import build, grads_of  # noqa: E402
from make_goldens_qa import qa_batch  # noqa: E402

PROMPT = [101, 2003, 1996, 2678, 1011, 3793, 103, 1029, 102]      # "[CLS] is the video - text [MASK] ? [SEP]" (ids of the shipped vocabulary)
SUB_KEYS = ("enc_txt.emb_txt.word_embeddings.weight", "enc_txt.emb_txt.position_embeddings.weight", "trsfr.layer.0.attention.self.query.weight",
            "fc_mtm.predictions.transform.dense.weight", "enc_img.emb_pos")


def prompt_pair():
    ids = torch.tensor(PROMPT, dtype=torch.long)
    return ids, torch.ones_like(ids)


def save(name, m, out, ans, ls, extra, meta):
    gk, gv = grads_of(m)
    named = {k.replace("trsfr.enc.", "trsfr."): p for k, p in m.named_parameters()}
    V = out.shape[-1]
    cols = torch.cat([torch.tensor([2995, 6270, 2023]), torch.randperm(V, generator=torch.Generator().manual_seed(5))[:253]])
    np.savez_compressed(
        f"{HERE}/{name}.npz", ans=ans.numpy(), out_cols=out[..., cols].detach().numpy().astype(np.float32), cols=cols.numpy(),
        out_lse=torch.logsumexp(out, -1).detach().numpy(), loss=np.array([ls.item()]), grad_norm_keys=gk, grad_norm_vals=gv,
        grad_emb_task=(named["emb_task"].grad if named["emb_task"].grad is not None else torch.zeros_like(named["emb_task"])).numpy(), **{"grad_sub::" + k: sub(named[k].grad, 2048) for k in SUB_KEYS},
        meta=np.array(meta), **extra)
    g = named["emb_task"].grad
    print(f"   {name}: loss {ls.item():.5f}, emb_task grad rows with mass {[] if g is None else np.nonzero(np.abs(g.numpy()).sum(1))[0].tolist()}")


def run_qaoe(ref, kind):
    M = importlib.import_module("main_qaoe_mlm_lsmdc_fib")
    B, X, swin, bert = 3, 26, "micro", "micro"
    m, _ = build(ref, M.LAVENDER_QAOE_MLM, swin, bert, B, size_vocab=-1, size_option=5,
                 enable_task_token=(kind == "task"), enable_prompt=(kind == "prompt"))
    vocab = BERT_CFGS[bert]["vocab_size"]
    batch = qa_batch(B, X, vocab, 6, [2023, 3899, 2158])
    batch["task_name"], batch["prompt"] = ("oe", None) if kind == "task" else (None, prompt_pair())
    m.eval()
    out, ans = m(batch)
    ls = torch.nn.CrossEntropyLoss(ignore_index=-1)(out.flatten(0, 1), ans.flatten())
    m.zero_grad()
    ls.backward()
    save(f"pretxt_qaoe_{kind}", m, out, ans, ls, dict(txt=batch["txt"].numpy(), mask_ans=batch["mask_ans"].numpy(), prompt=np.array(PROMPT)),
         [swin, bert, str(B), kind, str(X)])


def run_retmc(ref):
    M = importlib.import_module("main_retmc_mlm")
    B, O, X, swin, bert = 2, 3, 26, "micro", "micro"
    m, _ = build(ref, M.LAVENDER_RetMC_MLM, swin, bert, B, size_vocab=-1, size_option=O, enable_task_token=True)
    vocab = BERT_CFGS[bert]["vocab_size"]
    b = make_batch(B * O, X=X, vocab=vocab, seed=12)
    txt = b["txt"].view(B, O, X)
    ans = torch.full(txt.shape, -1, dtype=torch.long)
    ans[:, :, -1] = torch.tensor([[2995, 6270, 6270], [6270, 6270, 2995]])
    batch = {"img": make_batch(B, vocab=vocab, seed=13)["img"], "txt": txt, "mask": (txt != 0).long(), "mask_ans": ans,
             "task_name": "vtm", "prompt": None}
    m.eval()
    out, a = m(batch)
    ls = torch.nn.CrossEntropyLoss(ignore_index=-1)(out.flatten(0, 1), a.flatten())
    m.zero_grad()
    ls.backward()
    save("pretxt_retmc_task", m, out, a, ls, dict(txt=txt.numpy(), mask_ans=ans.numpy()), [swin, bert, str(B), "task", str(X), str(O)])


def run_captioning(ref, kind):
    CAP = importlib.import_module("model_for_captioning")
    B, swin, bert = 2, "micro", "micro"
    m, _ = build(ref, CAP.LAVENDER_Captioning, swin, bert, B, enable_task_token=(kind == "task"), enable_prompt=(kind == "prompt"))
    vocab = BERT_CFGS[bert]["vocab_size"]
    batch = make_batch(B, vocab=vocab, seed=6)
    torch.manual_seed(88)
    batch["txt"], ans = MG.R.masking(batch["txt"])
    m.eval()
    out = m({"img": batch["img"], "txt": batch["txt"].clone(), "mask": batch["mask"], "ans_mtm": ans.clone(), "attn_mask_type": "seq2seq",
             "prompt": prompt_pair() if kind == "prompt" else None})
    ls = torch.nn.CrossEntropyLoss(ignore_index=-1)(out["out"].flatten(0, 1), out["ans"].flatten())
    m.zero_grad()
    ls.backward()
    save(f"pretxt_cap_{kind}", m, out["out"], out["ans"], ls,
         dict(txt=batch["txt"].numpy(), ans_mtm=ans.numpy(), prompt=np.array(PROMPT), cap_prompt_txt_L=np.array([m.cap_prompt_txt_L])),
         [swin, bert, str(B), kind, str(batch["txt"].shape[1])])


def run_retrieval_prompt(ref):
    RM = importlib.import_module("main_retrieval_mlm")
    B, swin, bert = 3, "micro", "micro"
    m, _ = build(ref, RM.LAVENDER_Retrieval_MLM, swin, bert, B, enable_prompt=True)
    batch = make_batch(B, vocab=BERT_CFGS[bert]["vocab_size"], seed=4)
    batch["vid"] = [7, 9, 7]
    batch["prompt"], batch["task_name"] = prompt_pair(), None
    m.eval()
    out, ans = m(batch)
    ls = torch.nn.CrossEntropyLoss(ignore_index=-1)(out.flatten(0, 1), ans.flatten())
    m.zero_grad()
    ls.backward()
    save("pretxt_retrieval_prompt", m, out, ans, ls, dict(txt=batch["txt"].numpy(), vid=np.array(batch["vid"]), prompt=np.array(PROMPT)),
         [swin, bert, str(B), "prompt", str(batch["txt"].shape[1])])


def run_pretrain(ref, kind):
    PM = importlib.import_module("main_pretrain_mlm")
    B, swin, bert = 3, "micro", "micro"
    m, _ = build(ref, PM.LAVENDER_Pretrain_MLM, swin, bert, B, enable_task_token=(kind == "task"), enable_prompt=(kind == "prompt"))
    batch = make_batch(B, vocab=BERT_CFGS[bert]["vocab_size"], seed=1)
    torch.manual_seed(88)
    batch["txt"], batch["ans_mtm"] = MG.R.masking(batch["txt"])
    if kind == "prompt":
        batch["vtm_prompt"] = prompt_pair()
    m.eval()
    np.random.seed(88)
    out = m({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()})
    lf = torch.nn.CrossEntropyLoss(ignore_index=-1)
    l_mtm = lf(out["out_mtm"].flatten(0, 1), out["ans_mtm"].flatten())
    l_vtm = lf(out["out_vtm"].flatten(0, 1), out["ans_vtm"].flatten())
    m.zero_grad()
    (l_mtm + l_vtm).backward()
    V = out["out_vtm"].shape[-1]
    cols = torch.cat([torch.tensor([2995, 6270]), torch.randperm(V, generator=torch.Generator().manual_seed(5))[:254]])
    save(f"pretxt_pretrain_{kind}", m, out["out_vtm"], out["ans_vtm"], l_mtm + l_vtm, dict(
        txt=batch["txt"].numpy(), ans_mtm=batch["ans_mtm"].numpy(), prompt=np.array(PROMPT), losses=np.array([l_mtm.item(), l_vtm.item()]),
        mtm_cols=out["out_mtm"][..., cols].detach().numpy().astype(np.float32), mtm_lse=torch.logsumexp(out["out_mtm"], -1).detach().numpy()),
        [swin, bert, str(B), kind, str(batch["txt"].shape[1])])


def run_generate_prompt(ref):
    """greedy ids / logprob and the per-step [MASK]-row top-1 / top-2 margins (eval, dropout 0, max_gen_length 12, decoder weight x 8 as in
    make_goldens_caption_gen.py)"""
    import make_goldens_caption_gen as CG
    CAP = importlib.import_module("model_for_captioning")
    B, swin, bert = 2, "micro", "micro"
    m, _ = build(ref, CAP.LAVENDER_Captioning, swin, bert, B, max_gen_length=CG.MAX_LEN, repetition_penalty=1.0, is_decoder=False,
                 enable_prompt=True)
    m.config.is_decoder = False
    with torch.no_grad():
        m.fc_mtm.predictions.decoder.weight.mul_(CG.DECODER_SCALE)

    class _Enc(torch.nn.Module):
        def __init__(s, enc):
            super().__init__()
            s.enc = enc

        def forward(s, feat, mask, output_attentions=False, use_cache=False, past_key_values=None):
            return {"last_hidden_state": s.enc(feat, mask).last_hidden_state, "attentions": None, "past_key_values": None}
    m.trsfr = _Enc(m.trsfr.enc)
    batch = make_batch(B, vocab=BERT_CFGS[bert]["vocab_size"], seed=6)
    rows = []
    m.fc_mtm.register_forward_hook(lambda mod, inp, out: rows.append(out[:, -1].detach().clone()))
    m.eval()
    with torch.no_grad():
        ids, lp = m({"img": batch["img"], "txt": batch["txt"], "mask": batch["mask"], "attn_mask_type": "seq2seq", "prompt": prompt_pair()},
                    is_decode=True)
    top2 = torch.stack(rows, 1).topk(2, -1).values
    np.savez_compressed(f"{HERE}/pretxt_cap_gen_prompt.npz", ids=ids.numpy(), logprob=lp.numpy(), step_margin=(top2[..., 0] - top2[..., 1]).numpy(),
                        prompt=np.array(PROMPT), cap_prompt_txt_L=np.array([m.cap_prompt_txt_L]),
                        meta=np.array([swin, bert, str(B), str(CG.MAX_LEN), f"decoder.weight x {CG.DECODER_SCALE}"]))
    print("   pretxt_cap_gen_prompt: ids", ids[:, 0].tolist(), "logprob", lp.flatten().tolist())


if __name__ == "__main__":
    torch.set_num_threads(8)
    ref = MG.import_reference()
    run_qaoe(ref, "task")
    run_qaoe(ref, "prompt")
    run_retmc(ref)
    run_captioning(ref, "task")
    run_captioning(ref, "prompt")
    run_generate_prompt(ref)
    run_retrieval_prompt(ref)
    run_pretrain(ref, "task")
    run_pretrain(ref, "prompt")
    print("pre-text goldens written to", HERE)
