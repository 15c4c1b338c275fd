"""Caption fine-tuning entry point with the reference's command line (main_caption.py:281-364):

    python -m torch.distributed.run --nproc_per_node=N main_caption.py --config _args/args_msrvtt_cap.json --path_output D [--path_ckpt P]
    python main_caption.py --vis_backbone_init random --size_batch 8 --size_epoch 1          # one synthetic epoch on one GPU

Model, agent, loss, optimizer and data-parallel path are the MI355X-native ones of lavender_amd (LAVENDER_Captioning, Agent_Captioning with the
fused CaptioningLoss kernel; --label_smoothing, --drop_worst_ratio, --drop_worst_after, --max_gen_length, --num_beams ... as in the reference).
The reference reads its clips through a yaml TsvCompositeDataset, which is not part of this package: the script trains on synthetic clips and
captions with the batch keys of Dataset_Caption.collate_batch (img, txt, mask, img_keys).  Each epoch: train, evaluate (the prediction TSV under
<path_output>/caption_predictions; COCO metrics need a caption_metric callable, see Agent_Captioning), save_model.
LAV_SYNTH_STEPS sets the steps per epoch (default 20), LAV_SYNTH_VAL the validation clips (default one batch)."""
import json
import os
from datetime import datetime

import torch

import lavender_amd as LA
from lavender_amd.args import get_args
from lavender_amd.data import SyntheticCaption  # noqa: F401  (lived here before the multi-task entry point shared it)
from lavender_amd.dist import get_rank, get_world_size, is_main_process


class _Tok:
    cls_token = "[CLS]"; sep_token = "[SEP]"; pad_token = "[PAD]"; mask_token = "[MASK]"; unk_token = "[UNK]"
    ids = {"[PAD]": 0, "[UNK]": 100, "[CLS]": 101, "[SEP]": 102, "[MASK]": 103, "true": 2995, "false": 6270}

    def convert_tokens_to_ids(self, toks):
        return [self.ids[t] for t in toks]


def loader(ds, args, train):
    sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=get_world_size(), rank=get_rank(), shuffle=train) \
        if args.distributed else None
    return torch.utils.data.DataLoader(ds, batch_size=args.size_batch, sampler=sampler, num_workers=args.n_workers, pin_memory=True,
                                       drop_last=train, collate_fn=ds.collate_batch), sampler


if __name__ == '__main__':
    args = get_args()
    if args.task == "pretrain":
        args.type, args.task = "caption", "caption"
    tokzr = _Tok()
    n_steps = int(os.environ.get("LAV_SYNTH_STEPS", 20))
    ds_tr = SyntheticCaption(args, n_steps * args.size_batch * get_world_size(), "train", tokzr)
    ds_vl = SyntheticCaption(args, int(os.environ.get("LAV_SYNTH_VAL", args.size_batch)), "val", tokzr)
    dl_tr, sampler = loader(ds_tr, args, True)
    dl_vl, _ = loader(ds_vl, args, False)
    args.max_iter = 1 if args.size_epoch == 0 else len(dl_tr) * args.size_epoch
    model = LA.LAVENDER_Captioning(args, tokzr, is_decoder=getattr(args, 'is_decoder', False))
    model.load_ckpt(args.path_ckpt)
    model.cuda()
    args.path_output = '%s/_%s_%s' % (args.path_output, args.task, datetime.now().strftime('%Y%m%d%H%M%S'))
    agent = LA.Agent_Captioning(args, model)
    if args.distributed:
        agent.prepare_dist_model()
    agent.save_training_meta()
    for e in range(args.size_epoch):
        if sampler is not None:
            sampler.set_epoch(e)
        res_tr = agent.train(e + 1, dl_tr)
        res_vl = agent.evaluate(e + 1, dl_vl)
        for k in res_tr:
            agent.log[f'tr_{k}'].append(res_tr[k])
        for k in (res_vl or {}):
            agent.log[f'vl_{k}'].append(res_vl[k])
        if is_main_process():
            print(f'Ep {e + 1}: train: {json.dumps(res_tr)}, val: {json.dumps(res_vl)}')
        agent.save_model(e + 1)
