"""Golden vectors of caption fine-tuning (CONTAINER ONLY -- needs the reference checkout): Agent_Captioning.masking (main_caption.py:62-79) and
CaptioningLoss (model_for_captioning.py:10-37), both run from the reference's own code.  Writes cap_train_micro.npz next to this file:
  * masking: for a few (B, X, seed, p_mask), p_mask 0 included, the input ids and the (txt, ans_mtm) the reference returns after torch.manual_seed(seed);
  * loss: for (label_smoothing, drop_worst_ratio, drop_worst_after) in LOSS_CONFIGS, three calls each of one CaptioningLoss object on seeded
    (N_ROWS, 30522) logits -- its fp32 result as main_caption.py:225 computes it, and the same module on float64 logits.  The logits are not stored:
    tests.caption_loss_ref.make_case(N_ROWS, V, N_ROWS, seed) regenerates them (numpy default_rng, rounded to bf16).

    python tests/golden/make_goldens_caption_train.py
"""
import sys
sys.dont_write_bytecode = True
import importlib
import os
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_goldens as MG  # noqa: E402
from tests.caption_loss_ref import make_case  # noqa: E402

V, N_ROWS = 30522, 24
LOSS_CONFIGS = [(0.0, 0.0, 0), (0.1, 0.0, 0), (0.1, 0.25, 0), (0.0, 0.25, 2)]
MASK_CASES = [(2, 32, 1, 0.15), (4, 51, 2, 0.15), (3, 20, 3, 0.5), (2, 32, 4, 0.0)]
PAD, CLS, SEP, MASK = 0, 101, 102, 103


def caption_ids(B, X, seed):
    """[CLS] words [SEP] [PAD]..., one row with a [MASK] already in it"""
    rng = np.random.default_rng(seed)
    txt = np.zeros((B, X), dtype=np.int64)
    for b in range(B):
        k = int(rng.integers(4, X - 3))
        txt[b, 0] = CLS
        txt[b, 1:1 + k] = rng.integers(1000, 30000, size=k)
        txt[b, 1 + k] = SEP
    txt[0, 2] = MASK
    return txt


def import_caption_modules():
    MG.import_reference()
    stubs = ["evalcap", "evalcap.utils_caption_evaluate", "easydict", "toolz", "toolz.sandbox", "cv2", "av", "deepspeed", "apex", "progressbar"]
    for m in stubs:
        try:
            importlib.import_module(m)
        except Exception:
            sys.modules[m] = MagicMock(name=m)
    return importlib.import_module("main_caption"), importlib.import_module("model_for_captioning")


if __name__ == "__main__":
    torch.set_num_threads(8)
    MAIN, CAP = import_caption_modules()
    out = {"loss_configs": np.array(LOSS_CONFIGS, dtype=np.float64), "mask_cases": np.array(MASK_CASES, dtype=np.float64),
           "meta": np.array([str(V), str(N_ROWS)])}
    me = SimpleNamespace(pad_token_id=PAD, mask_token_id=MASK)
    for i, (B, X, seed, p) in enumerate(MASK_CASES):
        txt = torch.from_numpy(caption_ids(B, X, seed))
        out[f"mask{i}_in"] = txt.numpy().copy()
        torch.manual_seed(seed)
        r = MAIN.Agent_Captioning.masking(me, txt, p_mask=p)
        out[f"mask{i}_txt"], out[f"mask{i}_ans"] = r["txt"].numpy().copy(), r["ans_mtm"].numpy().copy()
        print("masking", (B, X, seed, p), "labelled", int((r["ans_mtm"] != -1).sum()))
    for i, (eps, ratio, after) in enumerate(LOSS_CONFIGS):
        cfg = SimpleNamespace(label_smoothing=eps, drop_worst_ratio=ratio, drop_worst_after=after)
        f32, f64 = CAP.CaptioningLoss(cfg), CAP.CaptioningLoss(cfg)
        l32, l64, seeds = [], [], []
        for call in range(3):
            seed = 100 * i + call
            x, lab = make_case(N_ROWS, V, N_ROWS, seed)
            x, lab = torch.from_numpy(x), torch.from_numpy(lab)
            l32.append(f32(x.float(), lab).item())
            l64.append(f64(x.double(), lab).item())
            seeds.append(seed)
        out[f"loss{i}_f32"], out[f"loss{i}_f64"], out[f"loss{i}_seed"] = np.array(l32, np.float32), np.array(l64, np.float64), np.array(seeds)
        print("loss", (eps, ratio, after), l64, "fp32 - fp64", [a - b for a, b in zip(l32, l64)])
    np.savez_compressed(f"{HERE}/cap_train_micro.npz", **out)
    print("caption-training golden written to", HERE)
