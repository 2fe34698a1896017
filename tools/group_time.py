#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest.group_matrix and group_sparsify (csrc/group.hip) beside a plain copy of
the cohort and the torch formulations of the same results on the same GPU.

    python tools/group_time.py [--points 4096x360,32768x84] [--rounds 5]

A point is S x n.  Per point, on one resident cohort of seeded symmetric matrices in (0, 1) (tools/ingest_time.py's):

  mean / fisher_mean         ingest.group_matrix(m, statistic)
  mean_among_half            ingest.group_matrix(m, among=every other unit)
  consistency                ingest.group_matrix(m, "consistency", keep=0.1): the select of the units' thresholds, then the reduce
  consistency_thresholds     ingest.group_matrix(m, "consistency", min_weight=thr [S]): the reduce alone
  mask / mask_in_place       ingest.group_sparsify(m | work, G, keep=0.1, out=work), G the mean: the select of the group
                             matrix's threshold (one workgroup), then the mask; in place on a fresh copy (the copy is not
                             timed)
  mask_threshold             ingest.group_sparsify(m, G, min_weight=t [1], out=work): the mask's launch alone
  sparsify_mean              ingest.group_sparsify(m, "mean", keep=0.1, out=work): the statistic, the choice, the mask
  torch_mean                 m.mean(0, dtype=torch.float64).float()
  torch_fisher_mean          tanh(atanh(m.double()).mean(0)).float()
  torch_consistency          the boolean edge mask at thr [S] and its mean
  torch_mask                 torch.where(E & (m > 0), m, 0.0)
  copy                       work.copy_(m): reads and writes the cohort once -- the reduce reads what it reads and writes
                             almost nothing, the mask moves the same bytes plus the group matrix

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, the ratio of every median to the copy's, the peak memory of the torch
formulations above the inputs, and whether the kernels agree with torch (the mean to 1e-6, the consistency and the mask
exactly).  One JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import ingest  # noqa: E402
from tools.ingest_time import cohort, spread, timed  # noqa: E402


def torch_consistency(m, thr):
    S, n, _ = m.shape
    eye = torch.eye(n, dtype=torch.bool, device=m.device)
    mask = (m > thr.view(S, 1, 1)) & (m > 0) & ~eye
    return (mask.sum(0, dtype=torch.float64) / S).float()


def torch_mask(m, G, t):
    n = m.shape[1]
    E = (G > t) & (G > 0) & ~torch.eye(n, dtype=torch.bool, device=m.device)
    return torch.where(E & (m > 0), m, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x360,32768x84")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_time.py measures on a ROCm GPU; none is visible")
    if args.rounds < 5:
        raise SystemExit("medians of at least 5 rounds")
    out = {"rounds": args.rounds, "points": []}
    for spec in args.points.split(","):
        S, n = (int(v) for v in spec.split("x"))
        torch.cuda.empty_cache()
        m = cohort(S, n)
        work = torch.empty_like(m)
        half = (torch.arange(S, device=m.device) % 2 == 0)
        thr = ingest.select_thresholds(m, keep=0.1)
        G = ingest.group_matrix(m)
        t = ingest.select_thresholds(G[None], keep=0.1)
        variants = {
            "copy": lambda: work.copy_(m),
            "mean": lambda: ingest.group_matrix(m),
            "fisher_mean": lambda: ingest.group_matrix(m, "fisher_mean"),
            "mean_among_half": lambda: ingest.group_matrix(m, among=half),
            "consistency": lambda: ingest.group_matrix(m, "consistency", keep=0.1),
            "consistency_thresholds": lambda: ingest.group_matrix(m, "consistency", min_weight=thr),
            "mask": lambda: ingest.group_sparsify(m, G, keep=0.1, out=work),
            "mask_in_place": lambda: ingest.group_sparsify(work, G, keep=0.1, out=work),
            "mask_threshold": lambda: ingest.group_sparsify(m, G, min_weight=t, out=work),
            "sparsify_mean": lambda: ingest.group_sparsify(m, "mean", keep=0.1, out=work),
            "torch_mean": lambda: m.mean(0, dtype=torch.float64).float(),
            "torch_fisher_mean": lambda: torch.tanh(torch.atanh(m.double()).mean(0)).float(),
            "torch_consistency": lambda: torch_consistency(m, thr),
            "torch_mask": lambda: torch_mask(m, G, t),
        }
        fresh = {"mask_in_place"}
        for name, fn in variants.items():                                  # warm-up of all
            if name in fresh:
                work.copy_(m)
            fn()
        agree = {"mean": bool(torch.allclose(G, variants["torch_mean"](), rtol=1e-6, atol=0.0)),
                 "consistency": bool(torch.equal(variants["consistency_thresholds"](), variants["torch_consistency"]())),
                 "mask": bool(torch.equal(variants["mask"]().view(torch.int32), variants["torch_mask"]().view(torch.int32)))}
        ms = {name: [] for name in variants}
        peak = {name: 0 for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                if name in fresh:
                    work.copy_(m)
                ti, p, res = timed(fn)
                del res
                ms[name].append(ti)
                peak[name] = max(peak[name], p)
        copy_ms = spread(ms["copy"])["median"]
        cohort_bytes = 4 * S * n * n
        point = {"S": S, "n": n, "cohort_bytes": cohort_bytes,
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_over_copy": spread(v)["median"] / copy_ms for name, v in ms.items() if name != "copy"},
                 **{name + "_peak_bytes_above_inputs": p for name, p in peak.items() if name.startswith("torch")},
                 "copy_bytes_per_s_at_median": 2 * cohort_bytes / (copy_ms * 1e-3),
                 "mean_bytes_per_s_at_median": cohort_bytes / (spread(ms["mean"])["median"] * 1e-3),
                 "mask_bytes_per_s_at_median": 2 * cohort_bytes / (spread(ms["mask"])["median"] * 1e-3),
                 "agrees_with_torch": agree}
        del work
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del m
    print(json.dumps(out))


if __name__ == "__main__":
    main()
