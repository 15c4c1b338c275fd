"""Multi-task MLM fine-tuning entry point with the reference's command line (main_multi_task_mlm.py:489-537):

    python -m torch.distributed.run --nproc_per_node=N main_multi_task_mlm.py --config _args/args_multi_task.json --path_output D [--path_ckpt P]
    python main_multi_task_mlm.py --config my_tasks.json --vis_backbone_init random --size_epoch 1         # synthetic loaders, one GPU

--config is JSON whose "datasets" is a list of {"type": ..., "task": ..., ...} overrides; each is laid over a deep copy of the shared args (the
reference's d_full_args.update(d_args)), so size_batch, size_txt, size_frame, size_option ... may differ per task.  Types: retrieval, qaoe
("lsmdc-fib" in the task name: the same text layout), qamc ("lsmdc-mc" in the task name: the RetMC layout, txt / mask / mask_ans (B, O, X)),
captioning; a task is called "<type>_<task>".  One LAVENDER_Multi_Task model and one Agent_Multi_Task train on all of them: every step the
MetaLoader draws a task.  --mt_rows (default true here; false = the reference's formulation over all text rows) runs the MLM head on the labelled
rows only, and in evaluation the last fusion layer and the read-outs on the [MASK] rows.  --enable_task_token / --enable_prompt as in the
reference.  The reference reads its clips through TSV / yaml datasets, which are not part of this package: the script runs on synthetic clips
with those datasets' text layouts and batch keys (lavender_amd.data.SyntheticQA / SyntheticCaption / SyntheticRetrieval / SyntheticRetMC).
Flow: zero-shot evaluation of every task on val and test, then agent.run.  LAV_SYNTH_STEPS sets each task's training steps per epoch (default 20),
LAV_SYNTH_VAL the validation / test samples (default one batch)."""
import copy
import json
import os
from datetime import datetime

import lavender_amd as LA
from lavender_amd.args import EasyDict, get_args
from lavender_amd.bert import BertConfigLite
from lavender_amd.data import StubTokenizer, SyntheticCaption, SyntheticQA, SyntheticRetMC, SyntheticRetrieval, synthetic_loader
from lavender_amd.dist import get_rank, get_world_size, is_main_process
from lavender_amd.multi_task import info

CLI_DEFAULTS = dict(mt_rows=True, size_vocab=-1)


def easy(v):
    """nested dicts of a JSON config as attribute dicts"""
    if isinstance(v, dict):
        return EasyDict({k: easy(x) for k, x in v.items()})
    if isinstance(v, list):
        return [easy(x) for x in v]
    return v


def dataset_args(args, d_args):
    """main_multi_task_mlm.py:27-28: the shared args, deep-copied, with the dataset's own keys laid over them"""
    full = copy.deepcopy(args)
    full.update(easy(dict(d_args)))
    return full


def get_meta_dataloaders(args, tokzr, n_steps, n_val, vocab):
    """main_multi_task_mlm.py:18-75 on synthetic datasets: ({task: train loader}, {task: val loader}, {task: test loader}, the sum of the train
    loaders' lengths, the option tokens of the (last) multiple-choice dataset)"""
    meta_dl_tr, meta_dl_vl, meta_dl_ts, len_dl_tr, mc_ans_tok_ids = {}, {}, {}, 0, None
    rank, world = get_rank(), get_world_size()
    info(f"In total {len(args.datasets)} datasets: {args.datasets}")
    for d_args in args.datasets:
        d_type = d_args["type"]
        task = f'{d_type}_{d_args["task"]}'
        full = dataset_args(args, d_args)
        if d_type == "retrieval":
            make = lambda n, split: SyntheticRetrieval(full, n, split, tokzr, vocab)
        elif d_type == "qaoe":
            full.size_vocab = -1                           # use shared answer vocab
            make = lambda n, split: SyntheticQA(full, n, split, tokzr, "oe", vocab)
        elif d_type == "qamc":
            if 'lsmdc-mc' in task:
                make = lambda n, split: SyntheticRetMC(full, n, split, tokzr, vocab)
            else:
                make = lambda n, split: SyntheticQA(full, n, split, tokzr, "mc", vocab)
        elif d_type == "captioning":
            make = lambda n, split: SyntheticCaption(full, n, split, tokzr)
        else:
            raise NotImplementedError(f"failed to load data for {task}")
        dl_tr, _ = synthetic_loader(make(n_steps * full.size_batch * world, "train"), full, True, rank, world)
        dl_vl, _ = synthetic_loader(make(n_val or full.size_batch, "val"), full, False, rank, world)
        dl_ts, _ = synthetic_loader(make(n_val or full.size_batch, "test"), full, False, rank, world)
        if d_type == "qamc" and 'lsmdc-mc' not in task:
            mc_ans_tok_ids = dl_ts.dataset.ans_tok_ids
        meta_dl_tr[task], meta_dl_vl[task], meta_dl_ts[task] = dl_tr, dl_vl, dl_ts
        len_dl_tr += len(dl_tr)
    return meta_dl_tr, meta_dl_vl, meta_dl_ts, len_dl_tr, mc_ans_tok_ids


def cli_args(argv=None, distributed=True):
    args = get_args(argv, distributed, defaults=CLI_DEFAULTS)
    args.size_vocab = -1                                   # the MLM head answers with the tokenizer's vocabulary
    if args.task == "pretrain":
        args.type, args.task = "multi_task", "multi_task"
    if not args.get("datasets"):
        raise SystemExit("main_multi_task_mlm.py: --config must list the tasks under \"datasets\": [{\"type\": ..., \"task\": ...}, ...]")
    args.datasets = easy(args.datasets)
    return args


if __name__ == '__main__':
    args = cli_args()
    tokzr = StubTokenizer()
    vocab = BertConfigLite.from_pretrained(args.tokenizer).vocab_size
    meta_dl_tr, meta_dl_vl, meta_dl_ts, len_dl_tr, mc_ans_tok_ids = get_meta_dataloaders(
        args, tokzr, int(os.environ.get("LAV_SYNTH_STEPS", 20)), int(os.environ.get("LAV_SYNTH_VAL", 0)), vocab)
    meta_dl_tr = LA.MetaLoader(meta_dl_tr, distributed=args.distributed)
    args.max_iter = 1 if args.size_epoch == 0 else len_dl_tr * args.size_epoch      # estimated
    args.iter_per_ep = len_dl_tr

    model = LA.LAVENDER_Multi_Task(args, tokzr, is_decoder=getattr(args, 'is_decoder', False))
    model.load_ckpt(args.path_ckpt)
    model.cuda()
    if args.distributed:
        info(f"n_gpu: {args.num_gpus}, rank: {get_rank()}, world_size: {get_world_size()}")
    args.path_output = '%s/_%s_%s' % (args.path_output, args.task, datetime.now().strftime('%Y%m%d%H%M%S'))
    agent = LA.Agent_Multi_Task(args, model, mc_ans_tok_ids=mc_ans_tok_ids)
    if args.distributed:
        agent.prepare_dist_model()
    agent.save_training_meta()

    info("Zero shot evaluation ...")
    for task, dl_vl in meta_dl_vl.items():
        res_vl = agent.evaluate(0, task, dl_vl)
        for k in res_vl:
            agent.log[f'{task}_vl_{k}'].append(res_vl[k])
        info(f'Ep 0 {task} vl: {json.dumps(res_vl)}')
    for task, dl_ts in meta_dl_ts.items():
        res_ts = agent.evaluate(0, task, dl_ts)
        for k in res_ts:
            agent.log[f'{task}_ts_{k}'].append(res_ts[k])
        info(f'Ep 0 {task} ts: {json.dumps(res_ts)}')

    if args.size_epoch:
        agent.run(meta_dl_tr, meta_dl_vl, meta_dl_ts)
