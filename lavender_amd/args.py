"""Config / flags -- thin restatement of the reference's utils/args.py for the pretrain entry point: an argparse
front end with a JSON overlay (CLI flag > JSON > default, utils/args.py:16-34) returning an attribute dict."""
import argparse
import json
import sys


class EasyDict(dict):
    """dict with attribute access; missing keys raise AttributeError (the code relies on getattr(args, k, default))."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None

    __setattr__ = dict.__setitem__
    __delattr__ = dict.__delitem__


def str_to_bool(v):
    return v if isinstance(v, bool) else str(v).lower() in ("yes", "true", "t", "1")


_DEFAULTS = dict(
    data_dir='./_datasets', txt_dir='', img_tsv_dir='', dataset='', data_ratio=1.0, path_output='./_snapshot/',
    reinit_head=False, vis_backbone='vidswin', vis_backbone_size='base', kinetics=-1, vis_backbone_init='2d',
    txt_backbone='bert-base-uncased', txt_backbone_embed_only=True, fusion_encoder='bert-base-uncased',
    fusion_encoder_rand_init=False, n_workers=4, size_batch=8, size_img=224, size_frame=4, max_size_frame=6,
    max_size_patch=14, size_patch=32, size_vocab=-1, size_txt_pre=25, img_transform=["img_rand_crop"], size_txt=25,
    lr=1.2e-5, decay=1e-3, size_epoch=20, seed=88, logging_steps=20, vis_backbone_lr_mul=1.0, max_grad_norm=-1.0,
    deepspeed=False, use_checkpoint=False, temp=1.0, local_rank=0, size_part=8, pretrain_tasks=["mtm", "vtm"],
    p_mask=0.15, enable_task_token=False, task_token=None, enable_prompt=False, mask_pos='append', path_ckpt='',
    multi_clip_testing=False, tokenizer='bert-base-uncased',
    # captioning (main_caption.py, model_for_captioning.py:10-37)
    label_smoothing=0.0, drop_worst_ratio=0.0, drop_worst_after=0, max_gen_length=20,
    # video QA (main_qaoe_mlm.py, main_qamc_mlm.py): head, last layer and read-out on the labelled [MASK] rows only (qa_mlm.py)
    qa_rows=False, size_option=5,
    # multi-task MLM fine-tuning (main_multi_task_mlm.py): the rows paths of multi_task.py
    mt_rows=False)


def parse_with_config(argv=None, defaults=None):
    """utils/args.py:16-34: every default is overridable by --flag; --config JSON fills what the CLI left unset
    and may add undeclared keys (type, task, ...).  defaults: an entry point's own defaults over _DEFAULTS."""
    p = argparse.ArgumentParser(description="lavender_amd pretrain")
    for k, v in {**_DEFAULTS, **(defaults or {})}.items():
        if isinstance(v, bool):
            p.add_argument(f"--{k}", type=str_to_bool, nargs='?', const=True, default=v)
        elif isinstance(v, list):
            p.add_argument(f"--{k}", type=type(v[0]), nargs="+", default=v)
        elif v is None:
            p.add_argument(f"--{k}", type=str, default=None)
        else:
            p.add_argument(f"--{k}", type=type(v), default=v)
    p.add_argument("--config", help="JSON config files")
    argv = sys.argv[1:] if argv is None else argv
    ns = p.parse_args(argv)
    args = EasyDict(vars(ns))
    if ns.config is not None:
        cfg = json.load(open(ns.config))
        given = {a[2:].split('=')[0] for a in argv if a.startswith('--')}
        for k, v in cfg.items():
            if k not in given:
                args[k] = v
    args.pop("config", None)
    return args


def get_args(argv=None, distributed=True, defaults=None):
    """utils/args.py:245-258: parse, init the process group from the launcher env, derive effective batch."""
    from .dist import dist_init
    args = parse_with_config(argv, defaults)
    args.setdefault("type", "pretrain")
    args.setdefault("task", "pretrain")
    dist_init(args, distributed)
    if not args.distributed:
        args.deepspeed = False
    args.effective_batch_size = args.size_batch * args.num_gpus
    return args
