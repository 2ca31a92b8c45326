#!/usr/bin/env python3
"""What serving a QLoRA adapter through merge + load_in_4bit costs, on the CPU (tests/nf4_ref.py; no GPU, no product code).

  python tools/requant_error.py [--N 1024] [--K 4096] [--M 64]

W ~ N(0, 0.02) [N, K], rank 8, s = alpha / r = 2, A ~ U(+-1/sqrt(K)), B ~ U(+-b) with b chosen per row of the table, x ~ N(0, 1) in
f16. The reference is the function the trainer optimised, y = x (deq(Q(W)) + s B A)^T. Per adapter size (rms of s B A over rms of W):
  requantised  |x deq(Q(f16(W + s B A)))^T - y| / |x (s B A)^T|   (merge_lora.py, then load_in_4bit: the second quantisation)
  unmerged     |x f16(deq(Q(W)) + s B A)^T - y| / |x (s B A)^T|   (one f16 rounding of the effective weight: what
               haff_nf4_dequant_lora_f16 hands the prefill products)
both in L2 norm over the outputs: the error as a multiple of the adapter's whole effect. Above 1, serving no adapter at all is
closer to the trained model. Prints one JSON line."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import nf4_ref as R   # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--K", type=int, default=4096)
    ap.add_argument("--M", type=int, default=64)
    args = ap.parse_args(argv)
    N, K, M, s = args.N, args.K, args.M, 2.0
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(N, K, generator=g) * 0.02).half()
    x = torch.randn(M, K, generator=g).half().double()
    a = ((torch.rand(8, K, generator=g) * 2 - 1) / math.sqrt(K)).half().double()
    b0 = (torch.rand(N, 8, generator=g) * 2 - 1)
    deq = R.dequant(*R.quantize(w)[:2]).double()
    rows = []
    for bmax in (0.002, 0.005, 0.016, 0.05, 0.16):
        delta = s * ((b0 * bmax).half().double() @ a)
        eff = deq + delta
        y = x @ eff.T
        effect = (x @ delta.T).norm()
        merged = (w.double() + delta).half()
        requant = R.dequant(*R.quantize(merged)[:2]).double()
        rows.append({"B_max": bmax, "delta_rms_over_W_rms": round((delta.pow(2).mean().sqrt() / w.double().pow(2).mean().sqrt()).item(), 4),
                     "requantised_err_over_effect": round(((x @ requant.T - y).norm() / effect).item(), 4),
                     "unmerged_f16_err_over_effect": float(f"{((x @ eff.half().double().T - y).norm() / effect).item():.3g}")})
    print(json.dumps({"N": N, "K": K, "M": M, "scale": s, "rows": rows}))


if __name__ == "__main__":
    main()
