"""Open-ended video QA fine-tuning entry point with the reference's command line (main_qaoe_mlm.py:130-230):

    python -m torch.distributed.run --nproc_per_node=N main_qaoe_mlm.py --config _args/args_msrvtt_qa.json --path_output D [--path_ckpt P]
    python main_qaoe_mlm.py --vis_backbone_init random --size_batch 8 --size_epoch 1          # one synthetic epoch on one GPU

LAVENDER_QAOE_MLM / Agent_QAOE_MLM of lavender_amd: the answer token is predicted at the [MASK] of "... answer: [MASK]".  --qa_rows (default
true here; false = the reference's formulation over all text rows) runs the MLM head, in evaluation also the last fusion layer and the top-k
read-out, on the labelled rows only.  --enable_task_token / --enable_prompt as in the reference.  The reference reads its clips through
Dataset_QAOE_MLM's TSV files, which are not part of this package: the script runs on synthetic clips and questions with that dataset's text
layout and batch keys (lavender_amd.data.SyntheticQA).  Zero-shot evaluation when --path_ckpt exists; each epoch: train, val, test, save_model
(log.json holds ac_1 / ac_5 per epoch); the best epochs at the end.  LAV_SYNTH_STEPS sets the steps per epoch (default 20), LAV_SYNTH_VAL the
validation / test samples (default one batch)."""
import os
from datetime import datetime

import lavender_amd as LA
from lavender_amd.args import get_args
from lavender_amd.bert import BertConfigLite
from lavender_amd.data import StubTokenizer, synthetic_qa_loaders
from lavender_amd.dist import get_rank, get_world_size, is_main_process

CLI_DEFAULTS = dict(qa_rows=True, size_vocab=-1)


def cli_args(argv=None, distributed=True):
    args = get_args(argv, distributed, defaults=CLI_DEFAULTS)
    args.size_vocab = -1           # the pre-trained tokenizer's vocabulary answers (main_qaoe_mlm.py:132-133)
    if args.task == "pretrain":
        args.type, args.task = "qaoe_mlm", "qaoe"
    return args


def info(msg):
    if is_main_process():
        print(msg, flush=True)


if __name__ == '__main__':
    args = cli_args()
    tokzr = StubTokenizer()
    vocab = BertConfigLite.from_pretrained(args.tokenizer).vocab_size
    dl_tr, dl_vl, dl_ts, sampler = synthetic_qa_loaders(args, tokzr, "oe", int(os.environ.get("LAV_SYNTH_STEPS", 20)),
                                                        int(os.environ.get("LAV_SYNTH_VAL", args.size_batch)), vocab, get_rank(), get_world_size())
    args.max_iter = 1 if args.size_epoch == 0 else len(dl_tr) * args.size_epoch
    args.actual_size_test = len(dl_ts.dataset)
    model = LA.LAVENDER_QAOE_MLM(args, tokzr=tokzr)
    model.load_ckpt(args.path_ckpt)
    model.cuda()
    if args.distributed:
        info(f"n_gpu: {args.num_gpus}, rank: {get_rank()}, world_size: {get_world_size()}")
    args.path_output = '%s/_%s_%s' % (args.path_output, args.task, datetime.now().strftime('%Y%m%d%H%M%S'))
    agent = LA.Agent_QAOE_MLM(args, model)
    if args.distributed:
        agent.prepare_dist_model()
    agent.save_training_meta()
    info("Saved training meta infomation...")

    if os.path.exists(args.path_ckpt):
        info("Zero-shot Evaluation")
        if len(dl_vl):
            ac_vl = agent.go_dl(0, dl_vl, False)
            info(f'ZS (val): {ac_vl["ac_1"] * 100:.2f}, {ac_vl["ac_5"] * 100:.2f}')
        if len(dl_ts):
            ac_ts = agent.go_dl(0, dl_ts, False)
            info(f'ZS (test): {ac_ts["ac_1"] * 100:.2f}, {ac_ts["ac_5"] * 100:.2f}')
    else:
        info("No pre-trained weight, skip zero-shot Evaluation")

    if args.size_epoch:
        info("Start training....")
        for e in range(args.size_epoch):
            if sampler is not None:
                sampler.set_epoch(e)
            ls_tr = agent.go_dl(e + 1, dl_tr, True)
            info(f'Ep {e}, Loss (train): {ls_tr["ls"] * 100:.4e}')
            if len(dl_vl):
                ac_vl = agent.go_dl(e + 1, dl_vl, False)
                for k in ac_vl:
                    agent.log.setdefault(f'{k}_vl', []).append(ac_vl[k])
                info(f'Ep {e}, Acc (val): {ac_vl["ac_1"] * 100:.2f}, {ac_vl["ac_5"] * 100:.2f}')
            if len(dl_ts):
                ac_ts = agent.go_dl(e + 1, dl_ts, False)
                for k in ac_ts:
                    agent.log.setdefault(f'{k}_ts', []).append(ac_ts[k])
                info(f'Ep {e}, Acc (test): {ac_ts["ac_1"] * 100:.2f}, {ac_ts["ac_5"] * 100:.2f}')
            agent.save_model(e + 1)
        best_vl, best_ts = agent.best_epoch()
        info(f'Best val @ ep {best_vl[0] + 1}, {best_vl[1] * 100:.2f}')
        info(f'Best test @ ep {best_ts[0] + 1}, {best_ts[1] * 100:.2f}')
