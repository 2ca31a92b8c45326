#!/usr/bin/env python3
"""Robot loop CLI — same flags, file protocol and output files as the reference's 2Haff/robot_demo.py (:22-55 flags, :168-336
loop), running the model on the MI355X through LisaMI355.evaluate().

  python -m 2handedafforder_amd.robot_demo --force_both ...   (or: python 2handedafforder_amd/robot_demo.py ...)

A robot-side process drops img.png, prompt.txt (first line: the action) and margins.txt (`left,top,right,bottom`) into
--zed2_img_path, plus mask_left.png / mask_right.png (8-bit grayscale, the padded size). Each request writes, into
--vis_save_path, aff_<hand>_heat.png and aff_<hand>.png for the hands the --force_* flags select and cropped_img.png, then deletes
img.png, prompt.txt and margins.txt (never the masks). The heat map and the padded, ANDed mask are computed on the device
(postprocess.robot_planes: haff_robot_heatmap, haff_robot_mask); only the finished uint8 planes leave it.

--multi_prompt (off by default: the first line of prompt.txt, as above): every non-empty line of prompt.txt is an action on the one
frame. They go through one evaluate(offset=[0, n]) call; line 0 writes the file names above, line i >= 1 the same set with _<i> in front
of the extension (aff_left_1.png, aff_left_heat_1.png, cropped_img_1.png, ...).

--contours (off by default): beside each aff_<hand><suffix>.png, aff_<hand><suffix>.json = {"original_size": [H, W], "contours":
[[[x, y], ...], ...]}: every external contour of that very plane (padded and ANDed), extracted on the device (contours.py) before the
plane is read back, for a planner that wants polygons instead of a raster.

--device_png (off by default): the aff_<hand><suffix>.png masks are encoded on the device (png.py, csrc/png_encode.hip) from the padded
and ANDed planes, and the host reads back the PNG streams instead of the planes: same pixels, no encoder in the request's latency. The
heat maps and cropped_img.png are RGB and stay on Pillow.

Offline extras as in inference.py: --synthetic, --sam-checkpoint, --max-new-tokens. Stated deviation: the two waits sleep
--poll-interval seconds between polls instead of busy-looping. Images are read and written with PIL (cv2 is not a dependency).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import haff  # noqa: F401
    from haff import contours as hcontours, png as hpng, postprocess, prompt as hprompt
    from haff.inference import build_model_and_tokenizer, load_rgb, prepare_frame
else:
    from . import contours as hcontours, png as hpng, postprocess, prompt as hprompt
    from .inference import build_model_and_tokenizer, load_rgb, prepare_frame


# Every non-empty line of prompt.txt is an action on the one frame: ONE evaluate(offset=[0, n]) call, so the frame is encoded and the
# prompt's common head prefilled once. Line 0 writes today's file names, line i >= 1 the same set with _<i> in front of the extension.
MULTI_PROMPT_FLAG = "--multi_prompt"
# Also an option of the loop: aff_<hand><suffix>.json with the contours of aff_<hand><suffix>.png beside every such file.
CONTOURS_FLAG = "--contours"
# Also an option of the loop: the aff_<hand><suffix>.png masks leave the device as PNG streams (png.PngEncoder).
DEVICE_PNG_FLAG = "--device_png"


def parse_args(args):
    parser = argparse.ArgumentParser(description="LISA chat")
    parser.add_argument("--version", default="aff_weights")
    parser.add_argument("--vis_save_path", default="./robot_demo/out", type=str)
    parser.add_argument("--force_left", action="store_true", default=False)
    parser.add_argument("--force_right", action="store_true", default=False)
    parser.add_argument("--force_both", action="store_true", default=False)
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
    parser.add_argument("--zed2_img_path", default="robot_demo/in", type=str,
                        help="directory containing subfolders of benchmark examples")
    parser.add_argument("--th", default=-5, type=int)
    # MI355X / offline extras
    parser.add_argument("--synthetic", default=None, choices=["tiny", "mid", "7b", "13b"], help="random-init model of this geometry")
    parser.add_argument("--sam-checkpoint", default=None, type=str)
    parser.add_argument("--max-new-tokens", default=512, type=int)
    parser.add_argument("--poll-interval", default=0.05, type=float, help="seconds between polls of --zed2_img_path")
    return parser.parse_args(args)


def load_gray(path):
    """cv2.imread(path, IMREAD_GRAYSCALE): exact for the 8-bit grayscale PNGs the protocol uses; other modes through PIL's
    convert("L") (restated: cv2 weighs the colour channels in its own fixed point)."""
    from PIL import Image
    im = Image.open(path)
    return np.array(im if im.mode == "L" else im.convert("L"))


def and_mask(side, mask_left, mask_right):
    """robot_demo.py:289-292,321-324: a hand is ANDed with its own mask, with the other hand's when its own is missing"""
    own, other = (mask_left, mask_right) if side == "left" else (mask_right, mask_left)
    return own if own is not None else other


def read_margins(path):
    with open(path, "r") as f:
        m = f.readline().split(",")
    return int(m[0]), int(m[1]), int(m[2]), int(m[3])


def write_hands(args, masks_left, masks_right, mask_left, mask_right, margins, device, suffix="", contours=False, encoder=None):
    """robot_demo.py:266-327 for a request whose taxonomy is not empty: the hands the --force_* flags select, every non-empty
    entry of pred_masks_<hand> in order (a later one overwrites the files of an earlier one, as there). suffix ("_<i>", --multi_prompt:
    prompt line i >= 1) goes in front of the file names' extension. contours: also aff_<hand><suffix>.json, from the planes while
    they are still on the device. encoder: a png.PngEncoder that makes the aff_<hand><suffix>.png files there too."""
    from PIL import Image
    hands = []
    for side, masks, forced in (("left", masks_left, args.force_left), ("right", masks_right, args.force_right)):
        if forced or args.force_both:
            hands += [(side, m[0]) for m in masks if m.shape[0] != 0]
    if not hands:
        return
    uploaded = {}
    and_masks = []
    for side, _ in hands:
        m = and_mask(side, mask_left, mask_right)
        if id(m) not in uploaded:
            uploaded[id(m)] = torch.from_numpy(m).to(device)
        and_masks.append(uploaded[id(m)])
    heat, planes = postprocess.robot_planes(torch.stack([x for _, x in hands]), args.th, margins, and_masks)
    found = hcontours.ContourReader().read(list(planes)) if contours else None
    files = encoder.encode(list(planes)) if encoder is not None else None
    heat, planes = heat.cpu().numpy(), planes.cpu().numpy() if files is None else planes
    for k, (side, _) in enumerate(hands):
        Image.fromarray(heat[k]).save(os.path.join(args.vis_save_path, f"aff_{side}_heat{suffix}.png"))
        mask_save_path = os.path.join(args.vis_save_path, f"aff_{side}{suffix}.png")
        os.makedirs(os.path.dirname(mask_save_path), exist_ok=True)
        if files is None:
            Image.fromarray(planes[k]).save(mask_save_path)
        else:
            with open(mask_save_path, "wb") as f:
                f.write(files[k])
        print(f"{mask_save_path} has been saved.")
        if found is not None:
            with open(os.path.join(args.vis_save_path, f"aff_{side}{suffix}.json"), "w") as f:
                json.dump({"original_size": list(planes[k].shape), "contours": hcontours.contour_lists(found[k])}, f)


def main(argv, max_requests=None):
    """max_requests: return after that many passes that found img.png, prompt.txt and margins.txt (a test hook, like
    chat.main(max_turns=)); None polls forever, as the reference does.
    --multi_prompt is an option of this loop, not one of parse_args' flags (those stay the reference's plus the four offline extras):
    it is taken out of argv here, and so are --contours and --device_png."""
    from PIL import Image
    multi_prompt = MULTI_PROMPT_FLAG in argv
    contours = CONTOURS_FLAG in argv
    encoder = hpng.PngEncoder() if DEVICE_PNG_FLAG in argv else None
    args = parse_args([a for a in argv if a not in (MULTI_PROMPT_FLAG, CONTOURS_FLAG, DEVICE_PNG_FLAG)])
    os.makedirs(args.vis_save_path, exist_ok=True)
    model, tokenizer, cfg, dtype = build_model_and_tokenizer(args)
    device = model.device
    if multi_prompt:
        # an action's files must not depend on which other actions share its call: one mask-decoder pass per action (lisa.py)
        model.tail_per_row = True
    print("Ready")
    requests = 0
    while max_requests is None or requests < max_requests:
        image_path = os.path.join(args.zed2_img_path, "img.png")
        prompt_path = os.path.join(args.zed2_img_path, "prompt.txt")
        margins_path = os.path.join(args.zed2_img_path, "margins.txt")
        mask_right_path = os.path.join(args.zed2_img_path, "mask_right.png")
        mask_left_path = os.path.join(args.zed2_img_path, "mask_left.png")
        if not os.path.exists(image_path) or not os.path.exists(prompt_path) or not os.path.exists(margins_path):
            print("Files not found, continuing")
            time.sleep(args.poll_interval)
            continue
        requests += 1
        mask_left = load_gray(mask_left_path) if os.path.exists(mask_left_path) else None
        mask_right = load_gray(mask_right_path) if os.path.exists(mask_right_path) else None
        if mask_left is None and mask_right is None:
            print("Masks not found")
            time.sleep(args.poll_interval)
            continue
        with open(prompt_path, "r") as f:
            narrations = [line for line in f.readlines() if line.strip()] if multi_prompt else [f.readline()]
        margins = read_margins(margins_path)
        image_np = load_rgb(image_path)
        frames, resize_list, original_size_list = prepare_frame(image_np, cfg, dtype, device)
        rows = [hprompt.tokenizer_image_token(hprompt.build_inference_prompt(n, args.use_mm_start_end), tokenizer, return_tensors="pt")
                for n in narrations]
        if len(rows) <= 1:
            input_ids = rows[0].unsqueeze(0).to(device) if rows else None
            grouped = {}
        else:
            # several actions on the one frame: right-padded rows, one call; the frame is encoded once (evaluate(offset=))
            input_ids = torch.full((len(rows), max(r.numel() for r in rows)), cfg.pad_token_id, dtype=torch.long)
            attention_mask = torch.zeros(input_ids.shape, dtype=torch.bool)
            for i, r in enumerate(rows):
                input_ids[i, :r.numel()] = r
                attention_mask[i, :r.numel()] = True
            input_ids = input_ids.to(device)
            grouped = {"attention_mask": attention_mask.to(device), "offset": torch.tensor([0, len(rows)], dtype=torch.int64)}
        if input_ids is None:
            print("No action found in prompt.txt")
            masks_left, masks_right, taxonomies = [], [], []
        else:
            output_ids, masks_left, masks_right, taxonomies = model.evaluate(
                None, None, input_ids, resize_list, original_size_list, max_new_tokens=args.max_new_tokens,
                tokenizer=tokenizer, frames_u8=frames, **grouped)
        for i, taxonomy in enumerate(taxonomies):
            suffix = f"_{i}" if i else ""
            if taxonomy.numel() != 0:   # the taxonomy does not gate here (robot_demo.py:268,298 are commented out)
                write_hands(args, masks_left[i:i + 1], masks_right[i:i + 1], mask_left, mask_right, margins, device, suffix,
                            contours=contours, encoder=encoder)
            else:
                print("No taxonomy found!!")
            Image.fromarray(image_np).save(os.path.join(args.vis_save_path, f"cropped_img{suffix}.png"))
        os.remove(image_path)
        os.remove(prompt_path)
        os.remove(margins_path)
    hpng.report_host_encodes(encoder)


if __name__ == "__main__":
    main(sys.argv[1:])
