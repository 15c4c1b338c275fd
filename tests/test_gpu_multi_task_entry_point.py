"""main_multi_task_mlm.py run as the reference's is -- `python main_multi_task_mlm.py --config <json> --path_output <dir>` -- in a fresh child
process under a time limit, on the micro configuration: four datasets, one per type, with differing size_frame / size_txt, one synthetic step
each (LAV_SYNTH_STEPS=1), one epoch.  Checked: the run directory `<path_output>/_multi_task_<timestamp>`, args.json (iter_per_ep = 4),
ckpt_violet_multi_task_0.pt and the final checkpoint with the model's key set, the log.json keys `{task}_{vl|ts}_{metric}` and the reference's
log lines; once on the rows paths with task tokens, once with --mt_rows false (the reference's formulation)."""
import glob
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

DATASETS = [{"type": "retrieval", "task": "synth", "size_frame": 2, "size_txt": 12, "size_batch": 3},
            {"type": "qaoe", "task": "synth-lsmdc-fib", "size_frame": 3, "size_txt": 16},
            {"type": "qamc", "task": "synth", "size_frame": 2, "size_txt": 40, "size_option": 5},
            {"type": "captioning", "task": "synth", "size_frame": 4, "size_txt": 14}]
TASKS = ["retrieval_synth", "qaoe_synth-lsmdc-fib", "qamc_synth", "captioning_synth"]


def _config(tmp_path):
    from tests.helpers import hf_cfg
    cfg = hf_cfg("micro")
    c = dict(vis_backbone_size="micro", kinetics=400, txt_backbone=cfg, fusion_encoder=cfg, tokenizer=cfg, txt_backbone_embed_only=True,
             fusion_encoder_rand_init=True, size_img=224, size_frame=2, size_txt=10, size_batch=2, size_epoch=1, n_workers=0, lr=2e-5,
             decay=1e-3, max_grad_norm=1.0, logging_steps=1, seed=88, size_option=5, max_gen_length=6, p_mask=0.3, datasets=DATASETS)
    p = tmp_path / "args_multi_task_synthetic.json"
    p.write_text(json.dumps(c))
    return str(p)


@pytest.mark.parametrize("extra", [["--enable_task_token"], ["--mt_rows", "false"]], ids=["rows_task_token", "full_path"])
def test_multi_task_entry_point_runs_one_synthetic_epoch(tmp_path, extra):
    out = tmp_path / "snapshot"
    env = dict(os.environ, LAV_SYNTH_STEPS="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("LAV_SYNTH_VAL", None)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "main_multi_task_mlm.py"), "--config", _config(tmp_path), "--path_output", str(out),
           "--vis_backbone_init", "random"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    runs = glob.glob(str(out / "_multi_task_*"))
    assert len(runs) == 1, (runs, os.listdir(out) if out.exists() else None)
    run = runs[0]
    stamp = os.path.basename(run).rsplit("_", 1)[1]
    assert len(stamp) == 14 and stamp.isdigit()                                     # %Y%m%d%H%M%S
    args = json.load(open(os.path.join(run, "args.json")))
    assert args["task"] == "multi_task" and args["path_output"] == run and args["iter_per_ep"] == 4 and args["max_iter"] == 4
    assert args["mt_rows"] is ("--mt_rows" not in extra) and args["enable_task_token"] is ("--enable_task_token" in extra)
    assert [d["type"] for d in args["datasets"]] == [d["type"] for d in DATASETS]
    ckpts = sorted(os.path.basename(f) for f in glob.glob(os.path.join(run, "ckpt_violet_multi_task_*.pt")))
    # step 4 = iter_per_ep closes epoch 4 // 4 + 1 = 2 (the reference's numbering) and reaches max_iter: evaluation, save_model(2), break
    assert ckpts == ["ckpt_violet_multi_task_0.pt", "ckpt_violet_multi_task_2.pt"], ckpts
    assert os.path.exists(os.path.join(run, "log.json"))
    log = json.load(open(os.path.join(run, "log.json")))
    want = set()
    for t in TASKS[:3]:
        for split in ("vl", "ts"):
            want |= {f"{t}_{split}_ac_1", f"{t}_{split}_ac_5"} if t.startswith("qaoe") else {f"{t}_{split}_ac"}
    assert set(log) == want, sorted(log)                                            # captioning: no caption_metric, nothing logged
    assert all(len(v) == 2 and all(0.0 <= x <= 1.0 for x in v) for v in log.values()), log   # zero-shot + the epoch's evaluation
    so = p.stdout
    assert "Zero shot evaluation ..." in so and "Start training...." in so
    for t in TASKS[:3]:
        assert f"Ep 0 {t} vl: " in so and f"Ep 0 {t} ts: " in so and f"Ep 2 {t} vl: " in so and f"Ep 2 {t} ts: " in so
        metric = "ac_1" if t.startswith("qaoe") else "ac"
        assert f"Best {metric} on {t} val @ ep " in so and f"Best {metric} on {t} test @ ep " in so
    assert "Ep 0 captioning_synth vl: {}" in so and "on captioning_synth" not in so
    sd0 = torch.load(os.path.join(run, "ckpt_violet_multi_task_0.pt"), map_location="cpu")
    sd1 = torch.load(os.path.join(run, "ckpt_violet_multi_task_2.pt"), map_location="cpu")
    assert set(sd0) == set(sd1) and "fc_mtm.predictions.decoder.weight" in sd0 and "emb_task" in sd0
    import lavender_amd as LA
    from tests.helpers import Tok, make_args
    assert set(sd0) == set(LA.LAVENDER_Multi_Task(make_args("micro", "micro", 2), Tok()).state_dict())
    moved = [k for k in sd0 if sd0[k].is_floating_point() and not torch.equal(sd0[k], sd1[k])]
    assert len(moved) > 50, len(moved)
    assert all(torch.isfinite(v).all() for v in sd1.values() if v.is_floating_point())
