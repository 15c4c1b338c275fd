"""main_qaoe_mlm.py / main_qamc_mlm.py run as the reference's are -- `python main_qa*_mlm.py --config <json> --path_output <dir>` -- in a child
process on the micro configuration for two synthetic steps of one epoch: the run directory `<path_output>/_<task>_<timestamp>`, args.json, the
checkpoints ckpt_violet_<task>_{0,1}.pt, log.json and the reference's log lines; once on the rows path with a task token, once with
--qa_rows false (the reference's formulation)."""
import glob
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _config(tmp_path, size_txt):
    from tests.helpers import hf_cfg
    cfg = hf_cfg("micro")
    c = dict(vis_backbone_size="micro", kinetics=400, txt_backbone=cfg, fusion_encoder=cfg, tokenizer=cfg, txt_backbone_embed_only=True,
             fusion_encoder_rand_init=True, size_img=224, size_frame=2, size_txt=size_txt, size_batch=2, size_epoch=1, n_workers=0, lr=2e-5,
             decay=1e-3, max_grad_norm=1.0, logging_steps=1, seed=88, size_option=5)
    p = tmp_path / "args_qa_synthetic.json"
    p.write_text(json.dumps(c))
    return str(p)


@pytest.mark.parametrize("extra", [["--enable_task_token"], ["--qa_rows", "false"]], ids=["rows_task_token", "full_path"])
@pytest.mark.parametrize("script,task,size_txt,X", [("main_qaoe_mlm.py", "qaoe", 21, 26), ("main_qamc_mlm.py", "qamc", 46, 49)])
def test_qa_entry_point_runs_two_synthetic_steps(tmp_path, script, task, size_txt, X, extra):
    out = tmp_path / "snapshot"
    env = dict(os.environ, LAV_SYNTH_STEPS="2", LAV_SYNTH_VAL="4", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, script), "--config", _config(tmp_path, size_txt), "--path_output", str(out),
           "--vis_backbone_init", "random"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    runs = glob.glob(str(out / f"_{task}_*"))
    assert len(runs) == 1, (runs, os.listdir(out) if out.exists() else None)
    run = runs[0]
    stamp = os.path.basename(run).rsplit("_", 1)[1]
    assert len(stamp) == 14 and stamp.isdigit()                                     # %Y%m%d%H%M%S
    args = json.load(open(os.path.join(run, "args.json")))
    assert args["task"] == task and args["path_output"] == run and args["max_iter"] == 2 and args["size_vocab"] == -1
    assert args["qa_rows"] is ("--qa_rows" not in extra) and args["enable_task_token"] is ("--enable_task_token" in extra)
    files = sorted(os.listdir(run))
    assert f"ckpt_violet_{task}_0.pt" in files and f"ckpt_violet_{task}_1.pt" in files and "log.json" in files, files
    log = json.load(open(os.path.join(run, "log.json")))
    so = p.stdout
    assert "No pre-trained weight, skip zero-shot Evaluation" in so and "Start training...." in so and "Best val @ ep 1" in so and "Best test @ ep 1" in so
    if task == "qaoe":
        assert "Ep 0, Loss (train):" in so and "Ep 0, Acc (val):" in so and "Ep 0, Acc (test):" in so
        assert all(len(log[k]) == 1 and 0.0 <= log[k][0] <= 1.0 for k in ("ac_1_vl", "ac_5_vl", "ac_1_ts", "ac_5_ts"))
    else:
        assert "Ep 1: " in so
        assert len(log["ls_tr"]) == 1 and np_finite(log["ls_tr"][0]) and all(0.0 <= log[k][0] <= 1.0 for k in ("ac_vl", "ac_ts"))
    sd0 = torch.load(os.path.join(run, f"ckpt_violet_{task}_0.pt"), map_location="cpu")
    sd1 = torch.load(os.path.join(run, f"ckpt_violet_{task}_1.pt"), map_location="cpu")
    assert set(sd0) == set(sd1) and "fc_mtm.predictions.decoder.weight" in sd0 and "emb_task" in sd0
    moved = [k for k in sd0 if sd0[k].is_floating_point() and not torch.equal(sd0[k], sd1[k])]
    assert len(moved) > 50, len(moved)                                              # two optimizer steps happened between the two files
    assert all(torch.isfinite(v).all() for v in sd1.values() if v.is_floating_point())
    if "--enable_task_token" in extra:
        assert not torch.equal(sd0["emb_task"], sd1["emb_task"])                    # the task row was trained


def np_finite(x):
    import math
    return isinstance(x, float) and math.isfinite(x)
