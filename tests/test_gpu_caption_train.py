"""MI355X: caption fine-tuning on the micro model (Agent_Captioning.train_step / train / test, the labelled-rows head against the full head) against
oracle.lavender_ref.captioning_encode_forward + the float64 loss of tests/caption_loss_ref.py.  Bounds: the ones
test_gpu_variants.py::test_captioning_seq2seq_matches_oracle_and_golden uses for this model and config (logits 1.5e-2, loss 1e-2, gradients 5 %)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import caption_loss_ref as CR
from tests import pretxt_ref as PR
from tests.helpers import BERT_CFGS, Tok, hf_cfg, make_args, make_batch
from tests.test_gpu_variants import _grad_check

pytestmark = pytest.mark.gpu

SWIN, BERT, B = "micro", "micro", 2
EPS = 0.1


def _oracle_params():
    from oracle import lavender_ref as R
    bc = BERT_CFGS[BERT]
    P = R.filled_params(SWIN, hidden=bc["hidden"], layers=bc["layers"], ffn=bc["ffn"], vocab=bc["vocab"])
    for v in P.values():
        v.requires_grad_(True)
    return P, bc


def _agent(rows_head, caption_metric=None, **kw):
    """filled micro LAVENDER_Captioning in an Agent_Captioning; dropout and stochastic depth off, so a train-mode step has the oracle's arithmetic"""
    import lavender_amd as LA
    from oracle import lavender_ref as R
    cfg = dict(hf_cfg(BERT), hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    args = make_args(SWIN, BERT, B, **dict(dict(txt_backbone=cfg, fusion_encoder=cfg, tokenizer=cfg, label_smoothing=EPS, p_mask=0.15, task="caption",
                                                max_gen_length=8), **kw))
    m = LA.LAVENDER_Captioning(args, Tok())
    new = {k: R.fill_tensor(k, v.shape) for k, v in m.state_dict().items() if v.is_floating_point()}
    new["fc_mtm.predictions.decoder.bias"] = new["fc_mtm.predictions.bias"]
    m.load_state_dict(new, strict=False)
    m.cuda()
    m.arena()
    for layer in m.enc_img.swin.layers:
        for blk in layer.blocks:
            blk.drop_prob, blk.keep_prob = 0.0, 1.0
    ag = LA.Agent_Captioning(args, m, caption_metric=caption_metric)
    ag.rows_head = rows_head
    return ag, m


def _masked_batch(ag, seed=6):
    batch = make_batch(B, vocab=BERT_CFGS[BERT]["vocab"], seed=seed)
    torch.manual_seed(88)
    batch.update(ag.masking(batch["txt"], p_mask=0.15))
    assert int((batch["ans_mtm"] != -1).sum()) >= 2
    return batch


def _oracle(batch, spec=None):
    """(P with gradients of the float64 label-smoothed loss, logits (B, Lp + X, V), labels, loss, number of correct rows)"""
    from oracle import lavender_ref as R
    P, bc = _oracle_params()
    b = dict(batch, attn_mask_type="seq2seq")
    ref = PR.captioning_forward(P, b, SWIN, bc["heads"], spec) if spec is not None else R.captioning_encode_forward(P, b, SWIN, bc["heads"])
    ans = ref["ans"] if spec is not None else batch["ans_mtm"]
    x, lab = ref["out"].flatten(0, 1), ans.flatten()
    rl = CR.row_losses(x, lab, EPS)
    loss = rl.sum() / int((lab != -1).sum())
    loss.backward()
    correct = int(((x.argmax(1) == lab) & (lab != -1)).sum())
    return P, ref["out"].detach(), ans, loss.item(), correct


def _forward_loss_backward(ag, m, batch, prompt=None):
    """the front half of train_step (forward, loss, backward) without the optimizer, so that the gradients can be read"""
    from lavender_amd.engine import dw_join
    m.train()
    m.arena().zero_grad()
    b = ag.prepare_batch(dict(batch))
    b["attn_mask_type"] = "seq2seq"
    if prompt is not None:
        b["prompt"] = prompt
    out = ag.forward_step(b)
    logits = out["out"].detach().float().cpu()
    ls = ag.loss_func(out["out"].flatten(0, len(out["out"].shape) - 2), out["ans"].flatten(), b["_n_lab"])
    stats = ag.loss_func.stats
    ls.backward()
    dw_join()
    torch.cuda.synchronize()
    return logits, out["ans"].cpu(), ls.item(), stats.cpu().tolist()


def test_train_step_matches_the_oracle_on_both_heads():
    ag_full, m_full = _agent(rows_head=False)
    batch = _masked_batch(ag_full)
    lab = batch["ans_mtm"]
    n_lab = int((lab != -1).sum())
    P, ref_logits, _, ref_loss, ref_correct = _oracle(batch)
    # full head: (B, X, V) logits
    logits, ans, loss_full, stats = _forward_loss_backward(ag_full, m_full, batch)
    assert logits.shape == ref_logits.shape and torch.equal(ans, lab)
    d = (logits - ref_logits).abs()
    e_full = abs(loss_full - ref_loss)
    print(f"full head: logits max {d.max().item():.3e} mean {d.mean().item():.3e}, loss {loss_full:.5f} oracle {ref_loss:.5f} (|d| {e_full:.3e}), "
          f"correct {stats[2]} oracle {ref_correct}, labelled {stats[3]}")
    assert d.max() < 1.5e-2 and d.mean() < 2.5e-3
    assert e_full < 1e-2
    assert stats[1:] == [n_lab, ref_correct, n_lab]
    _grad_check(m_full, P, rel_tol=0.05)
    # labelled-rows head: (n_labelled, V) logits of the same rows
    ag_rows, m_rows = _agent(rows_head=True)
    logits_r, ans_r, loss_rows, stats_r = _forward_loss_backward(ag_rows, m_rows, batch)
    assert logits_r.shape == (n_lab, ref_logits.shape[-1]) and torch.equal(ans_r, lab[lab != -1])
    d_r = (logits_r - ref_logits[lab != -1]).abs()
    e_rows = abs(loss_rows - ref_loss)
    print(f"rows head: logits max {d_r.max().item():.3e}, loss {loss_rows:.5f} (|d| vs oracle {e_rows:.3e}, vs full head {abs(loss_rows - loss_full):.3e})")
    assert d_r.max() < 1.5e-2
    assert e_rows < 1e-2
    assert e_rows <= 2 * e_full + 2.0 ** -10                              # the rule of tests/test_gpu_retrieval_eval.py for a second path
    assert stats_r[1:] == stats[1:]                                       # same accuracy count
    _grad_check(m_rows, P, rel_tol=0.05)
    # the whole train_step (optimizer included) reports the same loss and accuracy, on both heads
    for ag, m, want in ((ag_full, m_full, loss_full), (ag_rows, m_rows, loss_rows)):
        b = ag.prepare_batch(dict(batch))
        b["attn_mask_type"] = "seq2seq"
        ls, acc = ag.train_step(b)
        print(f"train_step: loss {ls:.5f} acc {acc:.4f}")
        assert abs(ls - want) < 1e-5 and abs(acc - ref_correct / n_lab) < 1e-6
        assert ag.loss_func.iter == 2 and ag.global_step == 1             # the optimizer stepped once


def test_train_step_without_labels_reports_zero_accuracy():
    ag, m = _agent(rows_head=True)
    batch = make_batch(B, vocab=BERT_CFGS[BERT]["vocab"], seed=6)
    batch.update(ag.masking(batch["txt"], p_mask=0.0))
    b = ag.prepare_batch(batch)
    b["attn_mask_type"] = "seq2seq"
    ls, acc = ag.train_step(b)
    assert acc == 0 and np.isnan(ls)                                      # the reference's mean over no rows
    assert torch.isfinite(m.arena().grad).all()


@pytest.mark.parametrize("kind", ["task", "prompt"])
def test_pretext_rows_carry_no_label(golden_dir, kind):
    """task token / prompt: the labels the rows head gathers are the caption's, shifted behind the pre-text; both heads against the oracle with
    the pre-text (tests/pretxt_ref.py), the rows head within twice the full head's loss error"""
    g = np.load(os.path.join(golden_dir, f"pretxt_cap_{kind}.npz"))
    ids = torch.from_numpy(g["prompt"]).long() if kind == "prompt" else None
    prompt = (ids, torch.ones_like(ids)) if kind == "prompt" else None
    spec = ("task", 3) if kind == "task" else ("prompt", prompt)
    Lp = 1 if kind == "task" else len(ids)
    res = {}
    for rows_head in (False, True):
        ag, m = _agent(rows_head, enable_task_token=kind == "task", enable_prompt=kind == "prompt")
        batch = _masked_batch(ag)
        lab = batch["ans_mtm"]
        if not rows_head:
            P, ref_logits, ref_ans, ref_loss, ref_correct = _oracle(batch, spec)
            if kind == "prompt":
                P["emb_task"].grad = None
            assert (ref_ans[:, :Lp] == -1).all() and torch.equal(ref_ans[:, Lp:], lab)
        logits, ans, loss, stats = _forward_loss_backward(ag, m, batch, prompt)
        assert m.cap_prompt_txt_L == Lp
        if rows_head:
            assert torch.equal(ans, lab[lab != -1])
            d = (logits - ref_logits[:, Lp:][lab != -1]).abs().max().item()
        else:
            assert torch.equal(ans, ref_ans)
            d = (logits - ref_logits).abs().max().item()
        print(f"{kind}, rows head {rows_head}: logits max {d:.3e}, loss {loss:.5f} oracle {ref_loss:.5f}, correct {stats[2]} oracle {ref_correct}")
        assert d < 3e-2                                                   # the logit bound tests/test_gpu_pretxt.py uses with a pre-text
        assert abs(loss - ref_loss) < 1e-2
        assert stats[1:] == [int((lab != -1).sum()), ref_correct, int((lab != -1).sum())]
        _grad_check(m, P, rel_tol=0.08)                                   # tests/test_gpu_pretxt.py's gradient bound with a pre-text
        res[rows_head] = loss
    assert abs(res[True] - ref_loss) <= 2 * abs(res[False] - ref_loss) + 2.0 ** -10


class _Clips(torch.utils.data.Dataset):
    """one fixed synthetic batch, served `steps` times, with the keys of Dataset_Caption.collate_batch"""
    yaml_file = "_datasets/synthetic/val.yaml"

    def __init__(self, steps):
        self.b = make_batch(B, vocab=BERT_CFGS[BERT]["vocab"], seed=6)
        self.steps = steps
        self.image_keys = [f"clip{i}" for i in range(B)]
        self.tokzr = Tok()

    def __len__(self):
        return self.steps

    def __getitem__(self, i):
        return {"img": self.b["img"].clone(), "txt": self.b["txt"].clone(), "mask": self.b["mask"].clone(), "img_keys": list(self.image_keys)}

    def get_caption_file_in_coco_format(self):
        return "captions.json"


def test_short_run_learns_and_writes_predictions(tmp_path):
    seen = []
    ag, m = _agent(rows_head=True, caption_metric=lambda pred, cap: seen.append((pred, cap)) or {"CIDEr": 0.0},
                   path_output=str(tmp_path), lr=3e-4, max_iter=40, logging_steps=10, p_mask=0.3)
    ag.lr_scheduler = type(ag.lr_scheduler)(ag.optzr, 40, warmup_ratio=0.0)
    dl = torch.utils.data.DataLoader(_Clips(1), batch_size=None)
    torch.manual_seed(3)
    losses = []
    for step in range(30):
        torch.manual_seed(3)                                              # the same masked positions every step: one fixed batch
        r = ag.train(1, dl)
        losses.append(r["loss"])
        assert 0.0 <= r["acc"] <= 1.0
    first, last = float(np.mean(losses[:5])), float(np.mean(losses[-5:]))
    print(f"mean loss of the first five steps {first:.4f}, of the last five {last:.4f}")
    assert np.isfinite(losses).all() and last < first
    res = ag.evaluate(1, dl)
    pred = os.path.join(str(tmp_path), "caption_predictions", "ep1_pred.synthetic.val.max8.tsv")
    assert res == {"CIDEr": 0.0} and seen == [(pred, "captions.json")]
    rows = [l.rstrip("\n").split("\t") for l in open(pred)]
    assert [r[0] for r in rows] == ["clip0", "clip1"]                     # one row per clip, in the dataset's key order
    for _, val in rows:
        caps = json.loads(val)
        assert len(caps) == 1 and set(caps[0]) == {"caption", "conf"} and 0.0 < caps[0]["conf"] <= 1.0
    import lavender_amd as LA
    ag2 = LA.Agent_Captioning(ag.args, m)                                 # without a metric: the file is reused, the result is None
    assert ag2.evaluate(1, dl) is None
