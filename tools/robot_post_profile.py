"""The device post-processing of robot_demo.py requests at 1024^2, for a kernel trace: per request, both hands' heat maps (one
haff_robot_heatmap call: min/max partials + the heat-map tiles) and their padded, ANDed masks (two haff_robot_mask calls), then the
copy of the finished uint8 planes to the host — what write_hands runs after evaluate().

  rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- python tools/robot_post_profile.py --requests 20

Prints one JSON line: the host-timed request (launches, kernels and the device-to-host copy, synchronised) and its spread."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    import torch
    import haff  # noqa: F401
    from haff import postprocess
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    S = args.size
    margins = (40, 30, 20, 10)
    logits = torch.from_numpy((rng.standard_normal((2, S, S)) * 8).astype(np.float32)).to(dev)
    masks = [torch.from_numpy(rng.integers(0, 256, (S + 40, S + 60), dtype=np.uint8)).to(dev) for _ in range(2)]
    times = []
    for i in range(args.warmup + args.requests):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        heat, planes = postprocess.robot_planes(logits, -5, margins, masks)
        heat, planes = heat.cpu().numpy(), planes.cpu().numpy()
        t1 = time.perf_counter()
        if i >= args.warmup:
            times.append((t1 - t0) * 1e6)
    print(json.dumps({"requests": args.requests, "size": S, "hands": 2, "host_us_median": round(float(np.median(times)), 1),
                      "host_us_min": round(min(times), 1), "host_us_max": round(max(times), 1),
                      "heat_bytes": int(heat.nbytes), "mask_bytes": int(planes.nbytes)}))


if __name__ == "__main__":
    main()
