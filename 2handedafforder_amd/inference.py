#!/usr/bin/env python3
"""Batch inference CLI — same flags, directory walk, prompt and output files as the reference's 2Haff/inference.py
(:20-49 flags, :199-334 loop), running the model on MI355X through LisaMI355.evaluate().

  python -m 2handedafforder_amd.inference ...   (or: python 2handedafforder_amd/inference.py ...)

Offline extras: --synthetic (seeded random weights + byte tokenizer, for plumbing runs without checkpoints).
Images are read/written with PIL (cv2 is not a dependency here); thresholds and file names follow :197,299,331.

--score scores the run against the aff_*.png under --benchmark-dir on the device, as `evaluation.py --map` would score the written
tree (scoring.BenchmarkScorer, one kernel launch per batch, one host read at the end); --score_only writes no PNGs at all.

--write_records PATH also writes the run as 2HANDS contour records (contours.py: one ops.contour_extract call per chunk over the
planes of --records_threshold, every external contour of each hand), a torch-saved list `train_ds.py --sam_records PATH` loads.

--smooth_masks applies ActAffordance's scripts/utils/gaussian.py (7x7 Gaussian blur of each written plane, then `> --smooth_threshold`)
to the fp32 masks on the device, once for all thresholds (postprocess.smooth_mask_lists, csrc/mask_smooth.hip): the PNGs, --score /
--score_only and --write_records then equal what that script would leave behind on the unsmoothed run's tree.

--device_png makes the mask files on the device (png.py, csrc/png_encode.hip): the planes of a chunk stay in HBM, one measure and one
emit call turn them into PNG streams of run tokens, and the host reads those few KB back instead of ten planes per frame and runs no
encoder. Same names, order and pixels as the default route; the files are a few times the size of Pillow's. Not with --score_only, which
writes no files.

--visualize DIR (with --score / --score_only) writes the panels of `calculate_iou.py --visualize`: ground truth and prediction over the
frame, side by side, captioned with the IoU of the scored counts. The scoring call draws them (haff_score_vis, csrc/mask_score.hip)
from the per-pixel decisions it counts, so smoothing, --score_cropped and --score_intersection show as they are scored.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import haff  # noqa: F401
    from haff import checkpoint, config as hcfg, contours, png, postprocess, preprocess, prompt as hprompt, scoring
    from haff.lisa import LisaMI355
else:
    from . import checkpoint, config as hcfg, contours, png, postprocess, preprocess, prompt as hprompt, scoring
    from .lisa import LisaMI355


def parse_args(args):
    parser = argparse.ArgumentParser(description="LISA chat")
    parser.add_argument("--version", default="sjauhri/2HAff")
    parser.add_argument("--vis_save_path", default="./vis_output", type=str)
    parser.add_argument("--precision", default="bf16", type=str, choices=["fp32", "bf16", "fp16"], help="precision for inference")
    parser.add_argument("--image_size", default=1024, type=int, help="image size")
    parser.add_argument("--model_max_length", default=512, type=int)
    parser.add_argument("--lora_r", default=8, type=int)
    parser.add_argument("--vision-tower", default="openai/clip-vit-large-patch14", type=str)
    parser.add_argument("--local-rank", default=0, type=int, help="node rank")
    parser.add_argument("--load_in_8bit", action="store_true", default=False)
    parser.add_argument("--load_in_4bit", action="store_true", default=False)
    parser.add_argument("--use_mm_start_end", action="store_true", default=True)
    parser.add_argument("--conv_type", default="llava_v1", type=str, choices=["llava_v1", "llava_llama_2"])
    parser.add_argument("--benchmark-dir", default=None, type=str, help="directory containing subfolders of benchmark examples")
    # MI355X / offline extras
    parser.add_argument("--synthetic", default=None, choices=["tiny", "mid", "7b", "13b"], help="random-init model of this geometry")
    parser.add_argument("--sam-checkpoint", default=None, type=str)
    parser.add_argument("--max-new-tokens", default=512, type=int)
    parser.add_argument("--batch-size", default=1, type=int,
                        help="frames per evaluate() call (the reference runs 1; prompts of different lengths are right-padded)")
    # scoring on the device (scoring.py): off by default, the written files are the same either way
    parser.add_argument("--score", action="store_true", default=False,
                        help="also score the masks against <benchmark-dir>/<video>/<frame>/aff_{left,right}.png on the device and "
                             "print what `evaluation.py --map` prints for the written tree")
    parser.add_argument("--score_only", action="store_true", default=False,
                        help="--score without writing any PNG: nothing is read back per frame")
    parser.add_argument("--score_cropped", action="store_true", default=False, help="evaluation.py --cropped: score at the frame's size")
    parser.add_argument("--score_intersection", action="store_true", default=False,
                        help="evaluation.py --intersection: a hand counts only inside its obj_<side>.png")
    parser.add_argument("--score_hausdorff", action="store_true", default=False,
                        help="also the two Hausdorff distances (the union planes are read back; the contour walk runs in a host thread)")
    parser.add_argument("--score_hausdorff_device", action="store_true", default=False,
                        help="the two Hausdorff distances from the device: contour walk and point-set distance in HIP, nothing read "
                             "back per batch and no host thread")
    # calculate_iou.py --visualize on the device (scoring.BenchmarkScorer(visualize=)): off by default
    parser.add_argument("--visualize", default=None, type=str, metavar="DIR",
                        help="with --score / --score_only: also write the benchmark's overlay panels (ground truth | prediction over the "
                             "frame, captioned with the frame's IoU) into DIR, drawn on the device from the pixels that are scored")
    parser.add_argument("--visualize_threshold", default=None, type=float,
                        help=f"the threshold whose prediction is drawn: one of {postprocess.THRESHOLDS} (default 0.5)")
    parser.add_argument("--visualize_caption", default=None, type=str,
                        help='the caption on the prediction half (default Aff-Ex); "." writes the prediction overlay alone, for frames '
                             "above IoU 0.2")
    parser.add_argument("--visualize_examples", default=None, type=int, help="panels to write (default 20; 0 = every scored frame)")
    # predictions as 2HANDS contour records (contours.py): off by default
    parser.add_argument("--write_records", default=None, type=str, metavar="PATH",
                        help="also torch.save the run as a list of 2HANDS records (narration, image, taxonomy, masks = the contours "
                             "of both hands at --records_threshold, extracted on the device): what train_ds.py --sam_records loads")
    parser.add_argument("--records_threshold", default=None, type=float,
                        help=f"the threshold whose masks --write_records writes: one of {postprocess.THRESHOLDS} (default 0.5)")
    # gaussian.py, step 2 of the benchmark workflow, on the logits (postprocess.smooth_mask_lists): off by default
    parser.add_argument("--smooth_masks", action="store_true", default=False,
                        help="smooth every mask as ActAffordance's scripts/utils/gaussian.py smooths the written PNGs (7x7 Gaussian blur, "
                             "then --smooth_threshold), once on the device before anything is written, scored or traced")
    parser.add_argument("--smooth_threshold", default=None, type=float, help="gaussian.py --threshold, in [0, 1) (default 0.5)")
    # the mask files as PNG streams made on the device (png.py): off by default
    parser.add_argument("--device_png", action="store_true", default=False,
                        help="encode the mask PNGs on the device, one call pair per chunk: the host reads back the compressed streams, "
                             "not the planes (same pixels, files a few times the size of Pillow's)")
    args = parser.parse_args(args)
    check_score_args(args)
    check_png_args(args)
    check_visualize_args(args)
    check_records_args(args)
    check_smooth_args(args)
    return args


def check_score_args(args):
    """--score_only implies --score; the modifiers mean nothing without it, and scoring needs the benchmark's masks."""
    args.score = bool(args.score or args.score_only)
    for flag in ("score_cropped", "score_intersection", "score_hausdorff", "score_hausdorff_device"):
        if getattr(args, flag, False) and not args.score:
            raise SystemExit(f"--{flag} modifies --score / --score_only: pass one of them")
    if args.score_hausdorff and getattr(args, "score_hausdorff_device", False):
        raise SystemExit("--score_hausdorff_device and --score_hausdorff are two routes to the same numbers: pass one of them")
    if args.score and not args.benchmark_dir:
        raise SystemExit("--score needs --benchmark-dir: the ground truth is its aff_{left,right}.png")


def check_png_args(args):
    """--device_png is a route to the mask files; --score_only writes none."""
    if getattr(args, "device_png", False) and args.score_only:
        raise SystemExit("--device_png makes the mask files and --score_only writes none: pass one of them")


def check_visualize_args(args):
    """--visualize modifies --score / --score_only, and its own modifiers mean nothing without it."""
    if args.visualize and not args.score:
        raise SystemExit("--visualize modifies --score / --score_only: pass one of them")
    for flag in ("visualize_threshold", "visualize_caption", "visualize_examples"):
        if getattr(args, flag) is not None and not args.visualize:
            raise SystemExit(f"--{flag} modifies --visualize: pass a directory to write to")
    if args.visualize_threshold is None:
        args.visualize_threshold = 0.5
    if args.visualize_threshold not in postprocess.THRESHOLDS:
        raise SystemExit(f"--visualize_threshold {args.visualize_threshold}: one of {postprocess.THRESHOLDS}")
    if args.visualize_caption is None:
        args.visualize_caption = "Aff-Ex"
    if args.visualize_examples is None:
        args.visualize_examples = 20
    if args.visualize_examples < 0:
        raise SystemExit("--visualize_examples: 0 (every scored frame) or a count")


def check_records_args(args):
    """--records_threshold modifies --write_records and names one of the thresholds the run computes anyway."""
    if args.records_threshold is not None and not args.write_records:
        raise SystemExit("--records_threshold modifies --write_records: pass a path to write to")
    if args.records_threshold is None:
        args.records_threshold = 0.5
    if args.records_threshold not in postprocess.THRESHOLDS:
        raise SystemExit(f"--records_threshold {args.records_threshold}: one of {postprocess.THRESHOLDS}")
    if args.write_records and not args.benchmark_dir:
        raise SystemExit("--write_records needs --benchmark-dir: the frames and narrations come from it")


def check_smooth_args(args):
    """--smooth_threshold modifies --smooth_masks and is a gaussian.py threshold."""
    if args.smooth_threshold is not None and not args.smooth_masks:
        raise SystemExit("--smooth_threshold modifies --smooth_masks: pass it too")
    if args.smooth_threshold is None:
        args.smooth_threshold = 0.5
    try:
        postprocess.smooth_need(args.smooth_threshold)
    except ValueError as e:
        raise SystemExit(f"--smooth_threshold: {e}")


PRECISIONS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def precision_dtype(precision):
    """--precision -> the model dtype (inference.py:170-186 of the reference: fp32 | bf16 | fp16). fp16 is the inference mode on the
    f16 MFMA kernels (the ViT-H neck and the decoder tail in f32, README "Precision modes")."""
    if precision not in PRECISIONS:
        raise SystemExit(f"--precision {precision}: one of {', '.join(PRECISIONS)}")
    return PRECISIONS[precision]


def build_model_and_tokenizer(args):
    if args.load_in_8bit or args.load_in_4bit:
        raise SystemExit("bitsandbytes 4/8-bit quantisation is outside this build's scope (SURVEY §2.2); "
                         "use --precision bf16, fp16 or fp32")
    dtype = precision_dtype(args.precision)
    device = f"cuda:{args.local_rank}"
    if args.synthetic:
        cfg = {"tiny": hcfg.tiny, "mid": hcfg.mid, "7b": hcfg.haff_7b, "13b": hcfg.haff_13b}[args.synthetic]()
        # fp16: the bf16 values of the same seed, so that --precision bf16 and fp16 run one model
        sd = checkpoint.synthetic_state_dict(cfg, 1234, device, torch.bfloat16 if dtype == torch.float16 else dtype)
        tokenizer = checkpoint.ByteTokenizer(cfg)
    else:
        # inference.py:115-127,158-168: slow (sentencepiece) Llama tokenizer of the checkpoint + [SEG]; the model from
        # LISAForCausalLM.from_pretrained(version, vision_tower=, seg_token_idx=) — local directories (no hub here)
        sp_file = os.path.join(args.version, "tokenizer.model")
        if not os.path.isfile(sp_file):
            raise SystemExit(f"{sp_file} not found: --version must be a local merged-checkpoint directory")
        tokenizer = checkpoint.SentencePieceTokenizer(sp_file)
        seg = tokenizer("[SEG]", add_special_tokens=False).input_ids[0]
        clip_dir = args.vision_tower if os.path.isdir(args.vision_tower) else None
        model = LisaMI355.from_pretrained(args.version, vision_tower=clip_dir, seg_token_idx=seg, torch_dtype=dtype,
                                          sam_checkpoint=args.sam_checkpoint, device=device).eval()
        cfg = model.cfg
        cfg.bos_token_id, cfg.eos_token_id, cfg.pad_token_id = tokenizer.bos_token_id, tokenizer.eos_token_id, tokenizer.pad_token_id
        return model, tokenizer, cfg, dtype
    model = LisaMI355(cfg, sd, dtype=dtype, device=device).eval()
    return model, tokenizer, cfg, dtype


def load_rgb(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def prepare_frame(image_np, cfg, dtype, device):
    """inference.py:229-256 with the host work moved to the device: the uint8 RGB frame is uploaded once; evaluate()
    derives the CLIP tensor (CLIPImageProcessor.preprocess) and the resized SAM frame (ResizeLongestSide.apply_image,
    then normalise + pad fused into the patch-embedding ingest) from it with the Pillow-exact HIP kernels.
    Returns (frames_u8 [1,H0,W0,3] on the device, resize_list, original_size_list)."""
    original_size = tuple(image_np.shape[:2])
    frames = torch.from_numpy(np.array(image_np, copy=True)).unsqueeze(0).to(device)
    resize = preprocess.get_preprocess_shape(original_size[0], original_size[1], cfg.sam.img_size)
    return frames, [resize], [original_size]


def save_mask(path, plane_u8):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(plane_u8).save(path)
    print(f"{path} has been saved.")


def save_png_bytes(path, data):
    """save_mask for a file that is already encoded (--device_png)."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(data)
    print(f"{path} has been saved.")


def output_planes(masks_left, masks_right, taxonomies, thresholds=postprocess.THRESHOLDS, on_device=False):
    """inference.py:276-334 on the device: {(side, th): uint8 [H0,W0] 0/255} — gating from taxonomies[0] (one host read of
    its argmax decides which files exist), all five thresholds of a hand from ONE pass over its fp32 mask. on_device: the planes
    stay CUDA tensors (--device_png encodes them there)."""
    out = {}
    taxonomy = taxonomies[0]
    if taxonomy.numel() == 0:
        return out
    tax = taxonomy.reshape(-1).float().contiguous()
    t = int(torch.argmax(tax))
    for side, masks, blank in (("left", masks_left, 1), ("right", masks_right, 0)):
        if t == blank:
            continue
        for pred_mask in masks:
            if pred_mask.shape[0] == 0:
                continue
            planes = postprocess.inference_planes(pred_mask[0], None, side, thresholds)
            if not on_device:
                planes = planes.cpu().numpy()
            for k, th in enumerate(thresholds):
                out[(side, th)] = planes[k]
    return out


def record_planes(masks_left, masks_right, taxonomies, threshold):
    """The planes output_planes writes for one frame at `threshold`, left on the device: (predicted class index or None without a
    [SEG], {side: uint8 [H0, W0] of 0 / 255}) under output_planes' own gate; a gated hand has no entry."""
    out = {}
    taxonomy = taxonomies[0]
    if taxonomy.numel() == 0:
        return None, out
    t = int(torch.argmax(taxonomy.reshape(-1).float().contiguous()))
    for side, masks, blank in (("left", masks_left, 1), ("right", masks_right, 0)):
        if t == blank:
            continue
        for pred_mask in masks:
            if pred_mask.shape[0] == 0:
                continue
            out[side] = postprocess.inference_planes(pred_mask[0], None, side, (threshold,))[0]
    return t, out


def chunk_records(reader, narrations, images, masks_left, masks_right, taxonomies, original_size_list, threshold):
    """One record per frame of a chunk, from ONE ContourReader.read over every open hand's plane. A frame without a [SEG] has no
    prediction: both hands empty and the records' default class 2."""
    per_frame = [record_planes(masks_left[b:b + 1], masks_right[b:b + 1], taxonomies[b:b + 1], threshold) for b in range(len(images))]
    keys = [(b, side) for b, (_, planes) in enumerate(per_frame) for side in planes]
    found = dict(zip(keys, reader.read([per_frame[b][1][side] for b, side in keys])))
    return [contours.prediction_record(narrations[b], images[b], 2 if t is None or t > 3 else t, found.get((b, "left"), []),
                                       found.get((b, "right"), []), original_size_list[b])
            for b, (t, _) in enumerate(per_frame)]


def pad_prompts(id_rows, pad_token_id):
    """collate_fn's rule (utils/dataset.py:90-93,144-150): right-pad with pad_token_id, mask = real positions."""
    L = max(r.numel() for r in id_rows)
    ids = torch.full((len(id_rows), L), pad_token_id, dtype=torch.long)
    mask = torch.zeros((len(id_rows), L), dtype=torch.bool)
    for b, r in enumerate(id_rows):
        ids[b, :r.numel()] = r
        mask[b, :r.numel()] = True
    return ids, mask


def iter_examples(benchmark_dir):
    """The directory walk of inference.py:199-219: <dir>/<folder>/{inpainting.png, annotation.json}, sorted."""
    for dir_name in sorted(os.listdir(benchmark_dir)):
        dir_path = os.path.join(benchmark_dir, dir_name)
        if not os.path.isdir(dir_path):
            continue
        for folder_name in sorted(os.listdir(dir_path)):
            folder_path = os.path.join(dir_path, folder_name)
            if not os.path.isdir(folder_path):
                continue
            image_path = os.path.join(folder_path, "inpainting.png")
            annotation_path = os.path.join(folder_path, "annotation.json")
            if not os.path.exists(image_path) or not os.path.exists(annotation_path):
                print(f"Required files not found in {folder_path}, skipping...")
                continue
            with open(annotation_path) as f:
                narration = json.load(f).get("narration", "")
            yield dir_name, folder_name, image_path, narration


def main(argv):
    """Returns the score report (evaluation.evaluate_folders' dict) with --score, else None."""
    args = parse_args(argv)
    closers = []   # what must end with the run however it ends (the --score_hausdorff worker thread)
    try:
        return _main(args, closers)
    finally:
        for close in closers:
            close()


def _main(args, closers):
    model, tokenizer, cfg, dtype = build_model_and_tokenizer(args)
    device = model.device
    scorer = None
    if args.score:
        stem = os.path.basename(os.path.normpath(args.vis_save_path))
        scorer = scoring.BenchmarkScorer(args.benchmark_dir, device, postprocess.THRESHOLDS,
                                         names=[stem + str(th) for th in postprocess.THRESHOLDS], cropped=args.score_cropped,
                                         intersection=args.score_intersection,
                                         hausdorff="device" if args.score_hausdorff_device else args.score_hausdorff,
                                         visualize=None if not args.visualize else {
                                             "dir": args.visualize, "threshold": args.visualize_threshold,
                                             "caption": args.visualize_caption, "examples": args.visualize_examples})
        closers.append(scorer.close)
    reader, records = (contours.ContourReader(), []) if args.write_records else (None, None)
    encoder = png.PngEncoder() if args.device_png else None
    examples = list(iter_examples(args.benchmark_dir))
    for i in range(0, len(examples), max(args.batch_size, 1)):
        chunk = examples[i:i + max(args.batch_size, 1)]
        frames, resize_list, original_size_list, id_rows, images = [], [], [], [], []
        for _, _, image_path, narration in chunk:
            images.append(load_rgb(image_path))
            fr, rs, osz = prepare_frame(images[-1], cfg, dtype, device)
            frames.append(fr[0])
            resize_list += rs
            original_size_list += osz
            prompt = hprompt.build_inference_prompt(narration, args.use_mm_start_end)
            id_rows.append(hprompt.tokenizer_image_token(prompt, tokenizer, return_tensors="pt"))
        input_ids, mask = pad_prompts(id_rows, cfg.pad_token_id)
        output_ids, masks_left, masks_right, taxonomies = model.evaluate(
            None, None, input_ids.to(device), resize_list, original_size_list, max_new_tokens=args.max_new_tokens,
            tokenizer=tokenizer, frames_u8=frames, attention_mask=mask)
        if args.smooth_masks:    # once, for all five thresholds and every consumer below
            masks_left, masks_right = postprocess.smooth_mask_lists(masks_left, masks_right, args.smooth_threshold)
        if scorer is not None:   # one launch for the chunk; the counts stay on the device until the report
            scorer.add_batch([(d, f) for d, f, _, _ in chunk], masks_left, masks_right, taxonomies, original_size_list,
                             frames_u8=frames if args.visualize else None)
        if reader is not None:   # one extraction for the chunk, on the very planes the PNGs below are read back from
            records += chunk_records(reader, [n for _, _, _, n in chunk], images, masks_left, masks_right, taxonomies,
                                     original_size_list, args.records_threshold)
        if args.score_only:
            continue
        if encoder is not None:  # the chunk's planes stay on the device: one encode makes all its files, written in the usual order
            named = [(os.path.join(args.vis_save_path + str(th), dir_name, folder_name, f"aff_{side}.png"), plane)
                     for b, (dir_name, folder_name, _, _) in enumerate(chunk)
                     for (side, th), plane in output_planes(masks_left[b:b + 1], masks_right[b:b + 1], taxonomies[b:b + 1],
                                                            on_device=True).items()]
            for (path, _), data in zip(named, encoder.encode([plane for _, plane in named])):
                save_png_bytes(path, data)
            continue
        for b, (dir_name, folder_name, _, _) in enumerate(chunk):   # per frame, exactly the reference's B = 1 rule
            for (side, th), plane in output_planes(masks_left[b:b + 1], masks_right[b:b + 1], taxonomies[b:b + 1]).items():
                save_mask(os.path.join(args.vis_save_path + str(th), dir_name, folder_name, f"aff_{side}.png"), plane)
    if reader is not None:
        contours.save_records(args.write_records, records)
        print(f"{args.write_records}: {len(records)} records at threshold {args.records_threshold}, {reader.host_walks} planes walked "
              "on the host")
    png.report_host_encodes(encoder)
    if scorer is not None:
        return scorer.report(verbose=True)
    return None


if __name__ == "__main__":
    main(sys.argv[1:])
