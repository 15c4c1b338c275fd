"""Text-to-video retrieval evaluation with the reference's command line (eval_retrieval_mlm.py:138-247):

    python eval_retrieval_mlm.py --config <args json> --path_ckpt P [--multi_clip_testing true] [--enable_prompt true | --enable_task_token true]

Every caption of the test split is scored against every test video through the fusion encoder and the MLM head (p_true / (p_true + p_false) at
the appended [MASK]), the videos are ranked per caption and R@1 / R@5 / R@10 / the median rank are written to {ckpt dir}/{ckpt name}_results.json
as {"test": {...}, "multi_clip_testing": ...}.  The evaluation runs in lavender_amd.retrieval_eval (feature pass, pair scorer on the [MASK] row,
ranks on the device).  When `--data_dir` holds img_<dataset>.tsv / img_<dataset>.id2lineidx.pkl / txt_<task>.json and `--tokenizer` is a local
tokenizer directory, the test split is read from there; otherwise the script evaluates synthetic clips (no data, tokenizer or network needed)
and, without --path_ckpt, the model's initial weights -- it says so -- writing the JSON to --path_output.
"""
import json
import os

import torch

import lavender_amd as LA
from lavender_amd.args import get_args
from lavender_amd.dist import is_main_process
from lavender_amd.retrieval_eval import evaluate_t2v


class _Tok:
    cls_token = "[CLS]"; sep_token = "[SEP]"; pad_token = "[PAD]"; mask_token = "[MASK]"; unk_token = "[UNK]"
    ids = {"[PAD]": 0, "[UNK]": 100, "[CLS]": 101, "[SEP]": 102, "[MASK]": 103, "true": 2995, "false": 6270}

    def convert_tokens_to_ids(self, toks):
        return [self.ids[t] for t in toks]


def synthetic_batches(args, n_video, captions_per_video, clips, batch_size):
    """test-split-shaped batches of random clips: video v has captions_per_video[v] captions (text ids in order), each caption ends in [MASK]"""
    X = int(args.size_txt) + 1
    items = []
    for v, k in enumerate(captions_per_video[:n_video]):
        g = torch.Generator().manual_seed(1000 + v)
        img = torch.randn(clips, int(args.size_frame), 3, int(args.size_img), int(args.size_img), generator=g)
        for _ in range(k):
            tid = len(items)
            gt = torch.Generator().manual_seed(5000 + tid)
            n = int(torch.randint(4, X - 4, (1,), generator=gt))
            txt = torch.zeros(X, dtype=torch.long)
            txt[0] = 101; txt[1:1 + n] = torch.randint(1000, 8000, (n,), generator=gt); txt[1 + n] = 102; txt[-1] = 103
            items.append((img, txt, (txt != 0).long(), tid, f"video{v}"))
    gt_txt2vid = {tid: vid for _, _, _, tid, vid in items}
    batches = []
    for i in range(0, len(items), batch_size):
        part = items[i:i + batch_size]
        batches.append({"img": torch.stack([p[0] for p in part]), "txt": torch.stack([p[1] for p in part]),
                        "mask": torch.stack([p[2] for p in part]), "tid": [p[3] for p in part], "vid": [p[4] for p in part]})
    return batches, gt_txt2vid


def real_split(args, split):
    """(dataset, tokenizer) when the reference's data layout and a local tokenizer are present, else None"""
    d = getattr(args, "data_dir", None)
    if not (d and os.path.exists(f"{d}/txt_{args.task}.json") and os.path.exists(f"{d}/img_{args.dataset}.tsv")
            and os.path.isdir(str(args.tokenizer))):
        return None
    import transformers
    from lavender_amd.data import Dataset_RetrievalMlmEval
    tokzr = transformers.AutoTokenizer.from_pretrained(args.tokenizer)
    return Dataset_RetrievalMlmEval(args, split, tokzr=tokzr), tokzr


def with_pretext(args, ds, batch):
    """eval_retrieval_mlm.py:151-164: the VTM prompt (one block per text) or the task token"""
    if args.enable_prompt:
        p_txt, p_mask = ds.get_prompt()
        B = batch["txt"].shape[0]
        batch["prompt_txt"], batch["prompt_mask"] = p_txt.unsqueeze(0).expand(B, -1), p_mask.unsqueeze(0).expand(B, -1)
    elif args.enable_task_token:
        batch["task_name"] = "vtm"
    return batch


if __name__ == '__main__':
    args = get_args()
    args.use_checkpoint = False
    # eval_retrieval_mlm.py:127-134: batch size by the reference's rule
    if args.multi_clip_testing:
        args.size_batch = 10 * args.num_gpus
    else:
        args.size_batch = (100 if args.size_txt <= 32 else 80) * args.num_gpus
    split = "test"
    real = real_split(args, split)
    if real is not None:
        ds, tokzr = real
        batches = (with_pretext(args, ds, ds.collate_batch([ds[j] for j in range(i, min(len(ds), i + args.size_batch))]))
                   for i in range(0, len(ds), args.size_batch))
        gt_txt2vid = ds.gt_txt2vid
    elif args.path_ckpt:
        # a checkpoint's results file holds numbers of its test split, never of synthetic clips
        raise SystemExit(f"--path_ckpt {args.path_ckpt}: the test split (data_dir {getattr(args, 'data_dir', None)!r}: txt_{args.task}.json, "
                         f"img_{args.dataset}.tsv) or the local tokenizer directory ({args.tokenizer!r}) is missing; nothing was evaluated")
    else:
        print("no test split / tokenizer found and no --path_ckpt: evaluating synthetic clips")
        tokzr = _Tok()
        n_video = int(os.environ.get("LAV_SYNTH_VIDEOS", "6"))
        caps = [2 if v % 3 == 0 else 1 for v in range(n_video)]
        batches, gt_txt2vid = synthetic_batches(args, n_video, caps, 2 if args.multi_clip_testing else 1, args.size_batch)
        if args.enable_prompt or args.enable_task_token:
            raise SystemExit("synthetic clips carry no prompt tokenizer: run without enable_prompt / enable_task_token")
    model = LA.LAVENDER_RetrievalMlmEval(args, tokzr)
    if args.path_ckpt:
        assert os.path.exists(args.path_ckpt), args.path_ckpt
        model.load_ckpt(args.path_ckpt)
    else:
        print("no --path_ckpt: evaluating the model's initial weights")
    model.cuda()
    model.eval()
    log = {}
    with torch.no_grad():
        res = evaluate_t2v(model, batches, gt_txt2vid)
    print(f"number of videos: {len(res['vids'])}")
    print(f"number of queries (by text): {len(res['tids'])}")
    log[split] = {k: res[k] for k in ('r@1', 'r@5', 'r@10', 'median')}
    print(split, log[split])
    log["multi_clip_testing"] = args.multi_clip_testing
    if args.path_ckpt:
        path_ckpt_dir = os.path.dirname(args.path_ckpt)
        filename, _ = os.path.splitext(args.path_ckpt.split("/")[-1])
        log_path = f"{path_ckpt_dir}/{filename}_results.json"
    else:
        os.makedirs(args.path_output, exist_ok=True)
        log_path = os.path.join(args.path_output, "retrieval_mlm_results.json")
    if is_main_process():
        json.dump(log, open(log_path, "w"))
        print(f"wrote {log_path}")
