#!/usr/bin/env python3
"""LoRA fine-tune loop for MI355X — the train_ds.py contract of the reference (2Haff/train_ds.py:125-622).

Same flags (the ones that drive the loop), same trainable set, same optimiser schedule (AdamW lr/betas, WarmupDecayLR
100 warm-up steps then linear decay, gradient clipping 1.0, gradient accumulation), same meter names / log format
(`Epoch: [e][ i/500] Time ... Loss ...`, train_ds.py:500-523, temp_log.txt:16445), best-IoU-only checkpoint with
auto-resume (train_ds.py:395-412,470-486), validation IoU / IoCM (train_ds.py:625-796).

MI355X-first differences: DeepSpeed ZeRO-2 is replaced by plain data parallelism — one process per GPU, gradients of
the trainable set (294 M params for 7B) accumulate locally over the micro-steps and are averaged ONCE per optimizer
step with bucketed RCCL all-reduces over xGMI; optimizer state is replicated (3.5 GB fp32 for 7B in 288 GB).
The 2HANDS loaders (h5 / HF datasets, cv2 contour masks) are replaced by a seeded synthetic sample generator that
emits the same 12-tuple per sample and the same collate_fn batch dict (utils/dataset.py:47-60,152-169).

--device_ingest (off by default; real datasets only): the batch is made on the device from uint8 frames, contour lists and token
ids that one prefetch thread prepares (train_ingest.py) instead of on the main thread inside the step loop.

--aug_flip P / --aug_jitter P (both 0 by default; real datasets only, training set only): 2HANDS' offline augmentations
(horizontal_flip.py, apply_jitter.py) drawn per sample from (--seed, sample index): Pillow on the host loader, HIP kernels with
--device_ingest (csrc/frame_augment.hip), the same augmented samples either way.

--aug_crop P (0 by default; same conditions): the third one, process_cropped_sequences.py's object-centred view, applied between
the flip and the jitter (csrc/frame_crop.hip with --device_ingest). --aug_flip 0.5 --aug_crop 0.6667 --aug_jitter 0.25 is the
reference's distribution from un-augmented records.

  python -m torch.distributed.run --nproc-per-node 8 2handedafforder_amd/train_ds.py --synthetic 7b --epochs 1 ...
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import haff  # noqa: F401
    from haff import checkpoint, config as hcfg, dist as hdist, ops, prompt as hprompt, scoring, train_ops as T
    from haff.aff_dataset import AffRecordsDataset
    from haff.train_ingest import DeviceIngest, Prefetcher
    from haff.train_model import LisaTrainable
else:
    from . import checkpoint, config as hcfg, dist as hdist, ops, prompt as hprompt, scoring, train_ops as T
    from .aff_dataset import AffRecordsDataset
    from .train_ingest import DeviceIngest, Prefetcher
    from .train_model import LisaTrainable


def parse_args(args):
    p = argparse.ArgumentParser(description="LISA Model Training")
    p.add_argument("--local_rank", default=0, type=int, help="node rank")
    p.add_argument("--version", default="liuhaotian/llava-v1.5-13b")
    p.add_argument("--vis_save_path", default="./vis_output", type=str)
    p.add_argument("--precision", default="bf16", type=str, choices=["fp32", "bf16", "fp16"])
    p.add_argument("--load_in_8bit", action="store_true", default=False)
    p.add_argument("--load_in_4bit", action="store_true", default=False,
                   help="QLoRA: train on the frozen NF4 base (the seven Llama projections and mm_projector; needs --precision fp16)")
    p.add_argument("--image_size", default=1024, type=int)
    p.add_argument("--model_max_length", default=575, type=int)
    p.add_argument("--lora_r", default=8, type=int)
    p.add_argument("--vision-tower", default="openai/clip-vit-large-patch14", type=str)
    p.add_argument("--dataset_dir", default="./dataset", type=str)
    p.add_argument("--log_base_dir", default="./runs", type=str)
    p.add_argument("--exp_name", default="lisa", type=str)
    p.add_argument("--epochs", default=10, type=int)
    p.add_argument("--steps_per_epoch", default=500, type=int)
    p.add_argument("--batch_size", default=2, type=int, help="batch size per device per step")
    p.add_argument("--grad_accumulation_steps", default=10, type=int)
    p.add_argument("--val_batch_size", default=1, type=int)
    p.add_argument("--workers", default=4, type=int)
    p.add_argument("--lr", default=0.001, type=float)
    p.add_argument("--ce_loss_weight", default=1.0, type=float)
    p.add_argument("--dice_loss_weight", default=0.5, type=float)
    p.add_argument("--bce_loss_weight", default=2.0, type=float)
    p.add_argument("--lora_alpha", default=16, type=int)
    p.add_argument("--lora_dropout", default=0.05, type=float)
    p.add_argument("--lora_target_modules", default="q_proj,v_proj", type=str)
    p.add_argument("--beta1", default=0.9, type=float)
    p.add_argument("--beta2", default=0.95, type=float)
    p.add_argument("--no_eval", action="store_true", default=False)
    p.add_argument("--benchmark_dir", default="", type=str,
                   help="validation folders <root>/<video>/<frame>/{inpainting.png, aff_left.png, aff_right.png, annotation.json} "
                        "(AffDatasetVal, train_ds.py:121,330-336 of the reference); empty: validate on held-out training records")
    p.add_argument("--eval_only", action="store_true", default=False)
    p.add_argument("--vision_pretrained", default="PATH_TO_SAM_ViT-H", type=str)
    p.add_argument("--out_dim", default=256, type=int)
    p.add_argument("--resume", default="", type=str)
    p.add_argument("--print_freq", default=1, type=int)
    p.add_argument("--start_epoch", default=0, type=int)
    p.add_argument("--train_mask_decoder", action="store_true", default=True)
    p.add_argument("--use_mm_start_end", action="store_true", default=True)
    p.add_argument("--auto_resume", action="store_true", default=True)
    p.add_argument("--conv_type", default="llava_v1", type=str, choices=["llava_v1", "llava_llama_2"])
    # MI355X / offline extras
    p.add_argument("--synthetic", default=None, choices=["tiny", "mid", "7b", "13b"],
                   help="random-init model of this geometry + byte tokenizer + synthetic samples (no checkpoints needed); "
                        "without it --version / --vision-tower / --vision_pretrained / --dataset_dir are REAL local paths")
    p.add_argument("--sam_records", default=None, type=str,
                   help="a torch-saved list of 2HANDS records (narration, inpainted/image, taxonomy, masks) when the HF "
                        "`datasets` hub / the h5 layout under --dataset_dir is not available")
    p.add_argument("--val_samples", default=4, type=int)
    p.add_argument("--mask_hw", default=None, type=int, nargs=2, help="ground-truth mask size (default: image size)")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--device_ingest", action="store_true", default=False,
                   help="make the batch on the device (train_ingest.py): the loader hands over uint8 frames, contour lists and token "
                        "ids from one prefetch thread; resizes, normalisation and the contour fill are HIP kernels. Same samples and "
                        "prompts as the host loader for one --seed. Not with --synthetic, whose dataset yields tensors")
    p.add_argument("--aug_flip", default=0.0, type=float,
                   help="probability of mirroring a training sample left-right, hands and taxonomy exchanged (2HANDS' "
                        "horizontal_flip.py; its data corresponds to 0.5). Training set only; not with --synthetic")
    p.add_argument("--aug_jitter", default=0.0, type=float,
                   help="probability of Pillow's Brightness -> Contrast -> Color jitter with factors from U(0.4, 1.6) on a training "
                        "frame (2HANDS' apply_jitter.py; its data corresponds to 0.25). With --device_ingest both run in HIP, "
                        "byte for byte what the host loader's Pillow gives for one --seed. Training set only; not with --synthetic")
    p.add_argument("--aug_crop", default=0.0, type=float,
                   help="probability of replacing a training sample by its object-centred view: the box of the object masks grown by "
                        "50 px, pasted centred on a black square and stretched back to the original size (2HANDS' "
                        "process_cropped_sequences.py; its data corresponds to 0.6667). A narration that says 'something' or 'things' "
                        "is always cropped. Applied after the flip and before the jitter; the records need obj_left / obj_right "
                        "contours. Training set only; not with --synthetic")
    return p.parse_args(args)


# ---------------------------------------------------------------------------------------------------------------------
# meters (utils/utils.py:52-150) — same names/format, all-reduced in ONE 2*len(meters)-float collective
# ---------------------------------------------------------------------------------------------------------------------
class AverageMeter:
    def __init__(self, name, fmt=":f"):
        self.name, self.fmt = name, fmt
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count

    def __str__(self):
        return ("{name} {val" + self.fmt + "} ({avg" + self.fmt + "})").format(**self.__dict__)


def all_reduce_meters(meters, device):
    import torch.distributed as dist
    if not dist.is_initialized():
        return
    t = torch.tensor([v for m in meters for v in (m.sum, m.count)], dtype=torch.float32, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    vals = t.tolist()
    for i, m in enumerate(meters):
        m.sum, m.count = vals[2 * i], vals[2 * i + 1]
        m.avg = m.sum / (m.count + 1e-5)


def progress_line(epoch, step, total, meters):
    nd = len(str(total))
    head = "Epoch: [{}][{:>{w}d}/{}]".format(epoch, step, total, w=nd)
    return "\t".join([head] + [str(m) for m in meters])


# ---------------------------------------------------------------------------------------------------------------------
# synthetic 2HANDS-shaped samples + collate (utils/aff_dataset.py:267-280, utils/dataset.py:30-169)
# ---------------------------------------------------------------------------------------------------------------------
QUESTION = "Where would you interact with the object to perform action {}? Please output segmentation mask."
ANSWER = "It is [SEG]."


class SyntheticAffDataset:
    """Seeded stand-in for AffDataset: (image_path, image, image_clip, conversations, masks_left, masks_right,
    taxonomy, label, resize, questions, sampled_classes, inference)."""

    def __init__(self, cfg, n, seed, mask_hw=None, inference=False):
        self.cfg, self.n, self.seed, self.inference = cfg, n, seed, inference
        self.hw = tuple(mask_hw) if mask_hw else (cfg.sam.img_size, cfg.sam.img_size)

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        cfg = self.cfg
        g = torch.Generator().manual_seed(self.seed * 100003 + idx)
        S = cfg.sam.img_size
        image = torch.randn((3, S, S), generator=g)
        image_clip = torch.randn((3, cfg.clip.image, cfg.clip.image), generator=g)
        h, w = self.hw
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")

        def blob():
            cy, cx = torch.rand(2, generator=g).tolist()
            r = 0.1 + 0.2 * torch.rand(1, generator=g).item()
            return (((yy / h - cy) ** 2 + (xx / w - cx) ** 2) < r * r).float()[None]
        tax_idx = int(torch.randint(0, 4, (1,), generator=g))
        taxonomy = [0.0] * 4
        taxonomy[tax_idx] = 1.0
        action = "action%d" % int(torch.randint(0, 50, (1,), generator=g))
        conv = hprompt.default_conversation()
        conv.append_message(conv.roles[0], hprompt.DEFAULT_IMAGE_TOKEN + "\n" + QUESTION.format(action))
        conv.append_message(conv.roles[1], ANSWER)
        label = {"left": torch.zeros(h, w), "right": torch.zeros(h, w)}
        return ("synthetic/%06d.png" % idx, image, image_clip, [conv.get_prompt()], blob(), blob(), taxonomy, label,
                (S, S), [QUESTION.format(action)], [action], self.inference)


def collate_text(conversations, tokenizer, model_max_length=575, use_mm_start_end=True, conv_type="llava_v1", inference=False,
                 offsets=None):
    """The text half of collate_fn (utils/dataset.py:62-150), shared with train_ingest.DeviceIngest: image placeholder, token ids
    padded with pad_token, the instruction spans masked with -100, truncation for training batches. `conversations` is the flat
    list of prompts, `offsets` the per-sample prefix counts (one conversation per sample when left out)."""
    convs = list(conversations)
    offs = list(offsets) if offsets is not None else list(range(len(convs) + 1))
    if use_mm_start_end:
        convs = [c.replace(hprompt.DEFAULT_IMAGE_TOKEN, hprompt.image_placeholder(True)) for c in convs]
    ids = [hprompt.tokenizer_image_token(c, tokenizer, return_tensors="pt") for c in convs]
    input_ids = torch.nn.utils.rnn.pad_sequence(ids, batch_first=True, padding_value=tokenizer.pad_token_id)
    attention_masks = input_ids.ne(tokenizer.pad_token_id)
    targets = input_ids.clone()
    conv = hprompt.get_conv(conv_type)
    sep = hprompt.label_separator(conv_type, conv)
    for conversation, target in zip(convs, targets):
        cur = 1
        target[:cur] = -100
        for rou in conversation.split(conv.sep2):
            if rou == "":
                break
            parts = rou.split(sep)
            assert len(parts) == 2, (len(parts), rou)
            parts[0] += sep
            round_len = len(hprompt.tokenizer_image_token(rou, tokenizer))
            instruction_len = len(hprompt.tokenizer_image_token(parts[0], tokenizer)) - 2
            target[cur:cur + instruction_len] = -100
            cur += round_len
        target[cur:] = -100
    if not inference:
        trunc = model_max_length - 255
        input_ids, targets, attention_masks = input_ids[:, :trunc], targets[:, :trunc], attention_masks[:, :trunc]
    return {"input_ids": input_ids, "labels": targets, "attention_masks": attention_masks, "offset": torch.LongTensor(offs),
            "conversation_list": convs}


def collate_fn(batch, tokenizer, model_max_length=575, use_mm_start_end=True, conv_type="llava_v1"):
    """utils/dataset.py:30-169: pad with pad_token, mask the instruction spans with -100; conv_type picks the template whose sep2
    splits the rounds and the separator that ends a round's instruction (:97-101: " ASSISTANT: " or "[/INST] ")."""
    images, clips, convs, ml, mr, labels_l, resizes, tax, offs = [], [], [], [], [], [], [], [], [0]
    paths, questions, classes = [], [], []
    for (path, image, image_clip, conversations, m_left, m_right, taxonomy, label, resize, _q, _c, inference) in batch:
        paths.append(path)
        questions.append(_q)
        classes.append(_c)
        images.append(image)
        clips.append(image_clip)
        convs.extend(conversations)
        ml.append(m_left.float())
        mr.append(m_right.float())
        labels_l.append(label)
        resizes.append(resize)
        tax.append(torch.tensor(taxonomy))
        offs.append(offs[-1] + len(conversations))
    text = collate_text(convs, tokenizer, model_max_length, use_mm_start_end, conv_type, inference=batch[0][-1], offsets=offs)
    return {"images": torch.stack(images, 0), "images_clip": torch.stack(clips, 0), "input_ids": text["input_ids"],
            "labels": text["labels"], "attention_masks": text["attention_masks"], "masks_list_left": ml, "masks_list_right": mr,
            "label_list": labels_l, "resize_list": resizes, "offset": text["offset"],
            "inference": batch[0][-1], "conversation_list": text["conversation_list"], "taxonomies_list": torch.stack(tax, 0),
            "image_paths": paths, "questions_list": questions, "sampled_classes_list": classes}


# ---------------------------------------------------------------------------------------------------------------------
# validation metrics (train_ds.py:761-796)
# ---------------------------------------------------------------------------------------------------------------------
def calculate_iou(a, b):
    inter = np.logical_and(a, b).sum()
    union = np.logical_or(a, b).sum()
    return inter / union if union != 0 else 0.0


def calculate_iocm(benchmark_mask, comparison_mask):
    inter = np.logical_and(benchmark_mask, comparison_mask).sum()
    area = comparison_mask.sum()
    return inter / area if area != 0 else 0.0


def _label_hw(sample, raw):
    """The ground-truth mask size of one validation sample: what decides which samples can share a forward."""
    return tuple(sample["mask_hw"]) if raw else tuple(sample[4].shape[-2:])


def validation_groups(fetch, lo, hi, batch_size, raw):
    """Consecutive samples lo..hi-1 in runs of at most batch_size whose label sizes are equal (forward(inference=True) stacks the
    predictions of a batch, so one batch has one label size). Yields lists of samples, in order."""
    group, hw = [], None
    for idx in range(lo, hi):
        sample = fetch(idx)
        shw = _label_hw(sample, raw)
        if group and (shw != hw or len(group) >= max(int(batch_size), 1)):
            yield group
            group = []
        group.append(sample)
        hw = shw
    if group:
        yield group


def validation_frames(out):
    """The scoring descriptors (scoring.pack_frames) of one forward(inference=True): per sample the first prompt's two logit planes
    at the label size, its four taxonomy probabilities as the gate, and the two ground-truth planes as uint8."""
    gt_l, gt_r = (out["gt_masks_left"] > 0).to(torch.uint8), (out["gt_masks_right"] > 0).to(torch.uint8)
    tax = out["pred_taxonomies"].float().contiguous()
    left, right = out["pred_masks_left"].float().contiguous(), out["pred_masks_right"].float().contiguous()
    return [{"left": left[b][0], "right": right[b][0], "taxonomy": tax[b][0], "gt_left": gt_l[b][0], "gt_right": gt_r[b][0],
             "target_hw": tuple(left.shape[-2:])} for b in range(left.shape[0])]


@torch.no_grad()
def validate(model, dataset, tokenizer, args, rank, world, device, ingest=None):
    """train_ds.py:625-758: teacher-forced forward(inference=True), masks > 0, taxonomy-gated union of L/R vs GT union.
    ingest (--device_ingest): the DeviceIngest that makes each batch on the device from dataset.raw_item.
    --val_batch_size consecutive samples of one label size share a forward. The three integers of each sample (intersection, union,
    predicted area) are counted on the device (ops.score_masks: threshold 0.0 on the raw logits, equal sizes, the gate from
    pred_taxonomies) and read back once per validation; the meters then see the same numbers in the same order as before."""
    model.eval()
    iou_m, iocm_m = AverageMeter("IoU"), AverageMeter("IoCM")
    lo, hi = hdist.shard_bounds(len(dataset), rank, world)
    fetch = dataset.raw_item if ingest is not None else dataset.__getitem__
    counts = []
    for group in validation_groups(fetch, lo, hi, args.val_batch_size, ingest is not None):
        if ingest is not None:
            batch = ingest.batch(group, tokenizer, args.model_max_length, args.conv_type)
        else:
            batch = collate_fn(group, tokenizer, args.model_max_length, conv_type=args.conv_type)
            batch = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}
        frames = validation_frames(model(**batch))
        counts.append(ops.score_masks(scoring.pack_frames(frames), [0.0], device).reshape(-1, 4))
    if counts:
        for inter, union, area, _ in torch.cat(counts).cpu().tolist():   # the one read-back
            iou_m.update(inter / union if union != 0 else 0.0)
            iocm_m.update(inter / area if area != 0 else 0.0)
    all_reduce_meters([iou_m, iocm_m], device)
    model.train()
    return iou_m.avg, iocm_m.avg


# ---------------------------------------------------------------------------------------------------------------------
PRECISIONS = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def precision_dtype(precision):
    """--precision -> the trainer's dtype (train_ds.py:365-370 of the reference: bf16, fp16 with dynamic loss scaling, or fp32)."""
    return PRECISIONS[precision]


def main(argv):
    closers = []   # what must end with the run however it ends (the --device_ingest prefetch thread)
    try:
        _main(argv, closers)
    finally:
        for close in closers:
            close()


def _main(argv, closers):
    args = parse_args(argv)
    if args.device_ingest and args.synthetic:
        raise SystemExit("--device_ingest cannot be combined with --synthetic: the synthetic dataset yields tensors, not uint8 frames "
                         "and contours (use --sam_records or --dataset_dir)")
    for flag in ("aug_flip", "aug_jitter", "aug_crop"):
        value = getattr(args, flag)
        if not 0.0 <= value <= 1.0:
            raise SystemExit(f"--{flag} is a probability in [0, 1], not {value}")
        if value > 0.0 and args.synthetic:
            raise SystemExit(f"--{flag} cannot be combined with --synthetic: the synthetic dataset yields tensors, not uint8 frames "
                             "and contours (use --sam_records or --dataset_dir)")
    if args.load_in_8bit:
        raise SystemExit("--load_in_8bit: LLM.int8 is not built for training (inference only; --load_in_4bit trains on the NF4 base)")
    if args.load_in_4bit and args.precision != "fp16":
        raise SystemExit(f"--load_in_4bit requires --precision fp16 (NF4 fine-tuning computes in float16), not --precision {args.precision}")
    hprompt.set_default_conversation(args.conv_type)      # train_ds.py:188-190
    rank, world, local_rank = hdist.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("train_ds.py needs MI355X devices: the fine-tune path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dtype = precision_dtype(args.precision)
    if args.synthetic:
        cfg = {"tiny": hcfg.tiny, "mid": hcfg.mid, "7b": hcfg.haff_7b, "13b": hcfg.haff_13b}[args.synthetic]()
        tokenizer = checkpoint.ByteTokenizer(cfg)
        tokenizer.model_max_length = args.model_max_length
        sd = checkpoint.synthetic_state_dict(cfg, 1234, device, dtype)   # identical on every rank (same seed)
    else:
        # the reference's model construction (train_ds.py:135-181): tokenizer + added tokens from --version, the base
        # checkpoint, the CLIP tower from --vision-tower, SAM from --vision_pretrained, text_hidden_fcs / taxonomy head /
        # the three new vocabulary rows freshly initialised (checkpoint.complete_for_training, same seed on every rank)
        for flag, path in (("--version", args.version), ("--vision-tower", args.vision_tower),
                           ("--vision_pretrained", args.vision_pretrained)):
            if not os.path.exists(path):
                raise SystemExit(f"{flag} {path!r} is not a local path (no hub access here); pass a directory/file, "
                                 f"or --synthetic <geometry> for a random-init plumbing run")
        cfg = checkpoint.config_from_dir(args.version)
        cfg.out_dim = args.out_dim
        tokenizer = checkpoint.SentencePieceTokenizer(os.path.join(args.version, "tokenizer.model"))
        tokenizer.model_max_length = args.model_max_length
        cfg.seg_token_idx = tokenizer("[SEG]", add_special_tokens=False).input_ids[0]
        cfg.im_start_idx = tokenizer("<im_start>", add_special_tokens=False).input_ids[0]
        cfg.im_end_idx = tokenizer("<im_end>", add_special_tokens=False).input_ids[0]
        cfg.bos_token_id, cfg.eos_token_id, cfg.pad_token_id = tokenizer.bos_token_id, tokenizer.eos_token_id, tokenizer.pad_token_id
        # the vocabulary of the model being built is the tokenizer's (train_ds.py:231-233: resize_token_embeddings(len(tokenizer))),
        # whatever config.json's vocab_size says about added tokens (a base that already carries 32003 rows stays 32003)
        cfg.llm.vocab = len(tokenizer)
        sd = checkpoint.load_state_dict(args.version, args.vision_tower, args.vision_pretrained, for_training=True,
                                        seed=args.seed, cfg=cfg)
    model = LisaTrainable(cfg, sd, dtype=dtype, device=device, lora_r=args.lora_r, lora_alpha=args.lora_alpha,
                          lora_dropout=args.lora_dropout, ce_loss_weight=args.ce_loss_weight,
                          dice_loss_weight=args.dice_loss_weight, bce_loss_weight=args.bce_loss_weight, seed=args.seed,
                          lora_target_modules=args.lora_target_modules, load_in_4bit=args.load_in_4bit)
    del sd
    n_lora = sum(p.numel() for k, p in model.named_parameters() if "lora_" in k)
    n_train = sum(p.numel() for p in model.parameters())
    if rank == 0:
        print(f"trainable params: {n_train:,d} (LoRA {n_lora:,d} in {len(model.lora_modules)} adapters) | world_size {world} | micro-batch {args.batch_size} "
              f"x accum {args.grad_accumulation_steps}")
    reducer = T.GradBucketReducer(model.named_parameters())   # p.grad become views into flat per-dtype buckets
    opt = T.BucketAdamW(reducer, model.named_parameters())    # fp32 master / moments per bucket, one fused launch each
    states = opt.states
    # fp16: dynamic loss scaling with DeepSpeed's defaults (the reference's config enables fp16 and states nothing else)
    scaler = T.DynamicLossScaler() if dtype == torch.float16 else None
    ckpt_dir = os.path.join(args.log_base_dir, args.exp_name, "ckpt_model")
    global_step, best_score, start_epoch = 0, 0.0, args.start_epoch
    resume = args.resume or (ckpt_dir if args.auto_resume and os.path.exists(os.path.join(ckpt_dir, "latest.pt")) else "")
    if resume:
        blob = torch.load(os.path.join(resume, "latest.pt"), map_location=device, weights_only=False)
        # adapters fitted against one base do not continue on the other (a checkpoint from before the field existed: 16-bit base)
        saved_fmt = blob.get("base_format")
        if saved_fmt != model.base_format:
            name = {"nf4": "NF4 (--load_in_4bit)", None: "16-bit"}
            raise ValueError(f"checkpoint {resume} was trained on the {name.get(saved_fmt, saved_fmt)} base, this run uses the "
                             f"{name[model.base_format]} base: {'pass' if saved_fmt == 'nf4' else 'drop'} --load_in_4bit to resume it")
        model.load_state_dict(blob["params"])
        for k, st in blob["optim"].items():
            states[k].master.copy_(st["master"]); states[k].m.copy_(st["m"]); states[k].v.copy_(st["v"]); states[k].step = st["step"]
        opt.refresh_lp()
        if scaler is not None and "loss_scaler" in blob:
            scaler.load_state_dict(blob["loss_scaler"])
        global_step, best_score = blob["global_step"], blob["best_score"]
        start_epoch = global_step // args.steps_per_epoch
        if rank == 0:
            print(f"resume training from {resume}, start from epoch {start_epoch}")
    if args.synthetic:
        train_ds = SyntheticAffDataset(cfg, 10 ** 9, args.seed + 1000 * rank, args.mask_hw)
        val_ds = SyntheticAffDataset(cfg, args.val_samples, 777, args.mask_hw, inference=True)
    else:
        # AffRecordsDataset = utils/aff_dataset.py:48-346 on the records' HF layout
        aug = {"aug_flip": args.aug_flip, "aug_jitter": args.aug_jitter}   # the training set only: validation is never augmented
        if args.aug_crop > 0.0:
            aug["aug_crop"] = args.aug_crop
        if args.sam_records:
            records = torch.load(args.sam_records, weights_only=False)
            train_ds = AffRecordsDataset(records, cfg, seed=args.seed + 1000 * rank, **aug)
            val_ds = AffRecordsDataset(records[:max(args.val_samples, 1)], cfg, samples_per_epoch=args.val_samples, inference=True, seed=777)
        elif os.path.isdir(args.dataset_dir):
            train_ds = AffRecordsDataset.from_local(args.dataset_dir, cfg, seed=args.seed + 1000 * rank, **aug)
            val_ds = AffRecordsDataset.from_local(args.dataset_dir, cfg, samples_per_epoch=args.val_samples, inference=True, seed=777)
        else:
            train_ds = AffRecordsDataset.from_hf(args.dataset_dir, cfg, seed=args.seed + 1000 * rank, **aug)
            val_ds = AffRecordsDataset.from_hf(args.dataset_dir, cfg, samples_per_epoch=args.val_samples, inference=True, seed=777)
    if not args.synthetic and args.benchmark_dir and os.path.isdir(args.benchmark_dir) and not args.no_eval:
        AffValDataset = sys.modules[AffRecordsDataset.__module__].AffValDataset   # the reference's validation set (train_ds.py:330-336)
        val_ds = AffValDataset(args.benchmark_dir, cfg, seed=777)
        if rank == 0:
            print(f"Training with {len(train_ds)} examples and validating with {len(val_ds)} examples.")
    if rank == 0 and (args.aug_flip > 0.0 or args.aug_jitter > 0.0 or args.aug_crop > 0.0):
        crop = f", object crop p={args.aug_crop:g}" if args.aug_crop > 0.0 else ""
        print(f"training augmentation: flip p={args.aug_flip:g}{crop}, colour jitter p={args.aug_jitter:g} "
              f"({'HIP kernels on the device' if args.device_ingest else 'Pillow on the host'})")
    total_steps = args.epochs * args.steps_per_epoch
    ingest = DeviceIngest(cfg, device, dtype) if args.device_ingest else None
    if args.eval_only:
        iou, iocm = validate(model, val_ds, tokenizer, args, rank, world, device, ingest)
        if rank == 0:
            print(f"IoU: {iou:.4f}, IoCM: {iocm:.4f}")
        return
    sample_idx = global_step * args.grad_accumulation_steps * args.batch_size
    prefetch = None
    if ingest is not None:   # one thread, two batches ahead: raw_item (decode, prompt) and the tokeniser, in sample order
        prefetch = Prefetcher(train_ds.raw_item, sample_idx, args.batch_size,
                              prepare=lambda raws: ingest.text(raws, tokenizer, args.model_max_length, args.conv_type))
        closers.append(prefetch.close)
    for epoch in range(start_epoch, args.epochs):
        meters = [AverageMeter("Time", ":6.3f"), AverageMeter("Loss", ":.4f"), AverageMeter("CeLoss", ":.4f"),
                  AverageMeter("MaskLoss", ":.4f"), AverageMeter("MaskBCELoss", ":.4f"), AverageMeter("MaskDICELoss", ":.4f"),
                  AverageMeter("TaxonomyCELoss", ":.4f")]
        keys = [None, "loss", "ce_loss", "mask_loss", "mask_bce_loss", "mask_dice_loss", "taxonomy_ce_loss"]
        model.train()
        end = time.time()
        loss_acc = torch.zeros((len(keys) - 1,), dtype=torch.float32, device=device)   # meters stay on the device
        n_acc = 0
        for step in range(args.steps_per_epoch):
            reducer.zero()
            for micro in range(args.grad_accumulation_steps):
                if prefetch is not None:
                    raws, text = prefetch.get()
                    batch = ingest.batch(raws, tokenizer, args.model_max_length, args.conv_type, text=text)
                else:
                    batch = collate_fn([train_ds[sample_idx + j] for j in range(args.batch_size)], tokenizer, args.model_max_length,
                                       conv_type=args.conv_type)
                    batch = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}
                sample_idx += args.batch_size
                out = model(**batch)
                # gradients accumulate into the bucket views across the micro-steps; on the last one each bucket's
                # all-reduce (RCCL) is issued as soon as its last gradient lands, under the rest of backward
                reducer.begin(sync=micro == args.grad_accumulation_steps - 1)
                if scaler is not None:   # fp16: the f32 loss times the current scale, so small f16 gradients stay representable
                    (out["loss"] * scaler.loss_scale).backward()
                else:
                    out["loss"].backward()
                loss_acc += torch.stack([out[k].detach().float().reshape(()) for k in keys[1:]])   # no host sync
                n_acc += 1
            reducer.finish()
            grads = reducer.grads()
            gscale = 1.0 / args.grad_accumulation_steps
            if scaler is not None:
                gscale /= scaler.loss_scale
            # gradient_clipping: 1.0 — the coefficient min(1, 1 / (norm + 1e-6)) of the UNSCALED norm is computed and consumed on
            # the device (the optimizer launches queue up behind backward; no host read of the norm)
            norm = T.grad_norm(grads)
            clip = T.clip_coef_device(norm * gscale, 1.0)
            # the schedule counts the steps that were taken (DeepSpeed does not step its lr_scheduler on a skipped step); global_step
            # counts every optimizer step, skipped ones included (the engine's global_steps: data position, epochs, print cadence)
            lr = T.warmup_decay_lr(global_step - (scaler.skipped_steps if scaler is not None else 0), total_steps, args.lr)
            # fp16: the kernels skip the update when the norm is not finite (an inf / NaN gradient: the scale overflowed f16). The
            # buckets were all-reduced before the norm, so every rank sees the same norm and skips the same step: no extra collective
            opt.step(lr=lr, betas=(args.beta1, args.beta2), eps=1e-8, wd=0.0, gscale=gscale, gscale_dev=clip,
                     skip_norm=norm if scaler is not None else None)
            skipped = False
            if scaler is not None:
                # the one host read of the step (DeepSpeed reads its overflow flag once per step too): decides the step count, the
                # schedule and the scale. A skipped step is not counted: neither Adam's step nor the LR schedule advance
                scale_used = scaler.loss_scale
                skipped = scaler.update_scale(not bool(torch.isfinite(norm).item()))
                if skipped:
                    opt.unstep()
                    if rank == 0:
                        print(f"[fp16] gradient overflow: step skipped, loss scale {scale_used:g} -> {scaler.loss_scale:g}", flush=True)
            global_step += 1
            meters[0].update(time.time() - end)
            end = time.time()
            if global_step % args.print_freq == 0:
                for m, v in zip(meters[1:], (loss_acc / max(n_acc, 1)).tolist()):   # ONE device->host read per log line
                    m.update(v, n_acc * args.batch_size)
                loss_acc.zero_()
                n_acc = 0
                all_reduce_meters(meters, device)
                if rank == 0:
                    line = progress_line(epoch, step + 1, args.steps_per_epoch, meters[:6])
                    if scaler is not None:
                        line += f"\tLossScale {scaler.loss_scale:g}" + ("\tskipped" if skipped else "")
                    print(line, flush=True)
                for m in meters:
                    m.reset()
        if not args.no_eval:
            iou, iocm = validate(model, val_ds, tokenizer, args, rank, world, device, ingest)
            if rank == 0:
                print(f"IoU: {iou:.4f}, IoCM: {iocm:.4f}")
            is_best = iou > best_score
            best_score = max(iou, best_score)
        else:
            is_best = True
        if is_best:
            if world > 1:
                torch.distributed.barrier()
            if rank == 0:  # parameters and optimizer state are replicated: rank 0 writes the only copy
                os.makedirs(ckpt_dir, exist_ok=True)
                blob = {"params": model.state_dict(), "global_step": global_step, "best_score": best_score, "epoch": epoch,
                        "base_format": model.base_format,   # "nf4" (--load_in_4bit) or None: the frozen base the adapters were fitted on
                        "optim": {k: {"master": s.master, "m": s.m, "v": s.v, "step": s.step} for k, s in states.items()}}
                if scaler is not None:
                    blob["loss_scaler"] = scaler.state_dict()
                torch.save(blob, os.path.join(ckpt_dir, "latest.pt"))
                print(f"saved checkpoint to {ckpt_dir} (global_step{global_step})")
    if ingest is not None and ingest.host_augments:
        print(f"[rank {rank}] {ingest.host_augments} frames beyond {ops.AUG_MAX_PIXELS} pixels were augmented on the host (Pillow)")
    if args.aug_crop > 0.0:
        host_crops = ingest.host_crops if ingest is not None else 0
        skipped = ingest.crop_skipped if ingest is not None else getattr(train_ds, "crop_skipped", 0)
        if host_crops or skipped:
            print(f"[rank {rank}] object crop: {host_crops} samples cropped on the host (Pillow) under --device_ingest, "
                  f"{skipped} drew the crop and had no object contour")
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
