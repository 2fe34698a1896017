#!/usr/bin/env python3
"""Time the random-walk encodings of connectome_gnn_amd.ingest (csrc/rw.hip) beside a plain copy of the
cohort and the torch formulation of the same values on the same GPU.

    python tools/rw_time.py [--points 4096x360:0.10,4096x360:0.30,32768x84:0.10,32768x84:0.30] [--rounds 5]

A point is S x n : keep.  Per point, on one resident cohort of seeded symmetric matrices (tools/ingest_time.py's) and
the thresholds of ``keep`` selected beforehand (their selection is not timed on either side):

  steps8                ingest.random_walk_encodings(m, min_weight=thr, steps=8): M2, M3 and M4
  steps4                the same for steps=4: M2 alone
  steps2                the same for steps=2: no product, the row sums and one walk
  torch_<the same>      mask, row-normalise in fp32, the fp32 torch.bmm products the steps need, and the diagonals as
                        (M_a * M_b^T).sum(-1) -- with its peak memory above the inputs
  copy                  work.copy_(m): the streaming floor is HALF of it for steps2; the products are n^3 work on the
                        fp32 matrix pipe and have no streaming floor

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, the ratio of every median to the copy's, of every torch median to the kernel's,
the share of the fp32 matrix peak (157.3 TFLOP/s) on the flops the definition needs (2 n^3 per product and subject), the
workspace the call asks for, and the largest difference between the kernel and the torch formulation on the first 64
subjects.  One JSON line.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import _lib, ingest  # noqa: E402
from tools.ingest_time import cohort, spread, timed  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12
PRODUCTS = {8: 3, 4: 1, 2: 0}


def torch_rw(m, thr, steps):
    """[S, n, steps] the way one writes it in torch."""
    S, n, _ = m.shape
    eye = torch.eye(n, dtype=torch.bool, device=m.device)
    mask = (m > thr.view(S, 1, 1)) & (m > 0) & ~eye
    a = torch.where(mask, m, 0.0)
    del mask
    s = a.sum(2, keepdim=True)
    M = {1: torch.where(s > 0, a / s, 0.0)}
    del a
    if steps >= 3:
        M[2] = torch.bmm(M[1], M[1])
    if steps >= 5:
        M[3] = torch.bmm(M[1], M[2])
    if steps >= 7:
        M[4] = torch.bmm(M[2], M[2])
    cols = [torch.zeros(S, n, device=m.device)]
    for k in range(2, steps + 1):
        cols.append((M[k // 2] * M[k - k // 2].transpose(1, 2)).sum(2))
    return torch.stack(cols, 2)


def workspace_bytes(S, n, steps):
    ids = (ctypes.c_int32 * steps)(*range(steps))
    return int(_lib.load().cgnn_ingest_rw_workspace_bytes(S, n, ids, steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x360:0.10,4096x360:0.30,32768x84:0.10,32768x84:0.30")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rw_time.py measures on a ROCm GPU; none is visible")
    out = {"rounds": args.rounds, "points": []}
    for spec in args.points.split(","):
        shape, keep = spec.split(":")
        S, n = (int(v) for v in shape.split("x"))
        keep = float(keep)
        torch.cuda.empty_cache()
        m = cohort(S, n)
        work = torch.empty_like(m)
        thr = ingest.select_thresholds(m, keep=keep)
        variants = {"copy": lambda: work.copy_(m)}
        for steps in PRODUCTS:
            variants[f"steps{steps}"] = lambda steps=steps: ingest.random_walk_encodings(m, min_weight=thr, steps=steps)
            variants[f"torch_steps{steps}"] = lambda steps=steps: torch_rw(m, thr, steps)
        for fn in variants.values():                                       # warm-up of all
            fn()
        head, head_thr = m[:64].contiguous(), thr[:64].contiguous()
        diff = (ingest.random_walk_encodings(head, min_weight=head_thr)
                - torch_rw(head, head_thr, 8)).abs().amax((0, 1)).tolist()
        ms = {name: [] for name in variants}
        peak = {name: 0 for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                t, p, res = timed(fn)
                del res
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        med = {name: spread(v)["median"] for name, v in ms.items()}
        cohort_bytes = 4 * S * n * n
        point = {"S": S, "n": n, "keep": keep, "cohort_bytes": cohort_bytes,
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_over_copy": med[name] / med["copy"] for name in ms if name != "copy"},
                 **{f"torch_over_kernel_steps{k}": med[f"torch_steps{k}"] / med[f"steps{k}"] for k in PRODUCTS},
                 **{name + "_peak_bytes_above_inputs": p for name, p in peak.items() if name != "copy"},
                 **{f"steps{k}_workspace_bytes": workspace_bytes(S, n, k) for k in PRODUCTS},
                 **{f"steps{k}_share_of_fp32_matrix_peak":
                    c * 2.0 * n ** 3 * S / (med[f"steps{k}"] * 1e-3) / FP32_MATRIX_PEAK
                    for k, c in PRODUCTS.items() if c},
                 "copy_bytes_per_s_at_median": 2 * cohort_bytes / (med["copy"] * 1e-3),
                 "max_abs_difference_to_torch_first_64_subjects": diff}
        del work
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del m
    print(json.dumps(out))


if __name__ == "__main__":
    main()
