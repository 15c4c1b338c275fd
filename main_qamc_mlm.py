"""Multiple-choice video QA fine-tuning entry point with the reference's command line (main_qamc_mlm.py:211-275):

    python -m torch.distributed.run --nproc_per_node=N main_qamc_mlm.py --config _args/args_tgif_action.json --path_output D [--path_ckpt P]
    python main_qamc_mlm.py --vis_backbone_init random --size_batch 8 --size_txt 98 --size_epoch 1     # one synthetic epoch, X = 101

LAVENDER_QAMC_MLM / Agent_QAMC_MLM of lavender_amd: the question and its --size_option options form one text, the [MASK] is trained to the
option-index token and evaluation takes the option with the largest share of the option tokens' logits.  --qa_rows (default true here; false =
the reference's formulation over all text rows) runs the MLM head, in evaluation also the last fusion layer and the option read-out, on the
[MASK] rows only.  --enable_task_token (with --task_token) / --enable_prompt as in the reference.  The reference reads its clips through
Dataset_QAMC_MLM's TSV files, which are not part of this package: the script runs on synthetic clips and questions with that dataset's text
layout and batch keys (lavender_amd.data.SyntheticQA).  Zero-shot evaluation when --path_ckpt exists; each epoch: train, val, test, the log
line "Ep e: loss val test", save_model; the best epochs at the end.  LAV_SYNTH_STEPS sets the steps per epoch (default 20), LAV_SYNTH_VAL the
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
    args.size_vocab = -1           # the MLM head answers with the tokenizer's vocabulary
    if args.task == "pretrain":
        args.type, args.task = "qamc_mlm", "qamc"
    if args.get("task_token") is None:
        args.task_token = "mc"
    return args


def info(msg):
    if is_main_process():
        print(msg, flush=True)


if __name__ == '__main__':
    args = cli_args()
    tokzr = StubTokenizer()
    vocab = BertConfigLite.from_pretrained(args.tokenizer).vocab_size
    dl_tr, dl_vl, dl_ts, sampler = synthetic_qa_loaders(args, tokzr, "mc", int(os.environ.get("LAV_SYNTH_STEPS", 20)),
                                                        int(os.environ.get("LAV_SYNTH_VAL", args.size_batch)), vocab, get_rank(), get_world_size())
    args.max_iter = 1 if (args.size_epoch == 0 or len(dl_tr) == 0) else len(dl_tr) * args.size_epoch
    model = LA.LAVENDER_QAMC_MLM(args, tokzr=tokzr)
    model.load_ckpt(args.path_ckpt)
    model.cuda()
    if args.distributed:
        info(f"n_gpu: {args.num_gpus}, rank: {get_rank()}, world_size: {get_world_size()}")
    args.path_output = '%s/_%s_%s' % (args.path_output, args.task, datetime.now().strftime('%Y%m%d%H%M%S'))
    agent = LA.Agent_QAMC_MLM(args, model, dl_ts.dataset.ans_tok_ids)
    if args.distributed:
        agent.prepare_dist_model()
    agent.save_training_meta()
    info("Saved training meta infomation, start training ...")

    if os.path.exists(args.path_ckpt):
        info("Zero-shot Evaluation")
        ac_vl = agent.go_dl(0, dl_vl, False) if len(dl_vl) else float("nan")
        ac_ts = agent.go_dl(0, dl_ts, False) if len(dl_ts) else float("nan")
        info('ZS: %.2f %.2f' % (ac_vl * 100, ac_ts * 100))
    else:
        info("No pre-trained weight, skip zero-shot Evaluation")

    if args.size_epoch:
        info("Start training....")
        for e in range(args.size_epoch):
            if sampler is not None:
                sampler.set_epoch(e)
            ls_tr = agent.go_dl(e + 1, dl_tr, True)
            ac_vl = agent.go_dl(e + 1, dl_vl, False) if len(dl_vl) else float("nan")      # an empty split: the reference's average of nothing
            ac_ts = agent.go_dl(e + 1, dl_ts, False) if len(dl_ts) else float("nan")
            agent.log['ls_tr'].append(ls_tr)
            agent.log['ac_vl'].append(ac_vl)
            agent.log['ac_ts'].append(ac_ts)
            info('Ep %d: %.6f %.2f %.2f' % (e + 1, ls_tr, ac_vl * 100, ac_ts * 100))
            agent.save_model(e + 1)
        best_vl, best_ts = agent.best_epoch()
        info(f'Best val @ ep {best_vl[0] + 1}, {best_vl[1] * 100:.2f}')
        info(f'Best test @ ep {best_ts[0] + 1}, {best_ts[1] * 100:.2f}')
