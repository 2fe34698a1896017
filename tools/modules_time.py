#!/usr/bin/env python3
"""Time the module measures of connectome_gnn_amd.ingest (csrc/modules.hip) beside a plain copy of the
cohort and the torch formulation of the same values on the same GPU.

    python tools/modules_time.py [--points 4096x360:7,4096x360:17,32768x84:7] [--keep 0.10] [--rounds 5]

A point is S x n : M.  Per point, on one resident cohort of seeded symmetric matrices (tools/ingest_time.py's), a seeded
partition of the n ROIs into M modules, and the thresholds of ``keep`` selected beforehand (their selection is not timed
on either side):

  all_five              ingest.node_measures(m, min_weight=thr, measures=MODULE_MEASURES, modules=c)
  participation_pair    the same for ("participation", "weighted_participation"): no z-score phase
  profile               ingest.module_profile(m, c, min_weight=thr)
  torch_<the same>      mask, where, bmm with the one-hot [n, M], reductions (fp32) -- with its peak memory above the inputs
  copy                  work.copy_(m): the streaming floor is HALF of it, the kernel reads the cohort once and writes [S, n, F]

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, the ratio of every median to the copy's, of every torch median to the kernel's,
and the largest difference between the kernel and the torch formulation on the first 64 subjects (the torch side sums in
fp32).  One JSON line.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import ingest  # noqa: E402
from tools.ingest_time import cohort, spread, timed  # noqa: E402

PAIR = ("participation", "weighted_participation")


def partition(n, M, seed=0):
    """int64 [n] on the host: seeded labels, every one of 0 .. M - 1 used."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, M, (n,), generator=g)
    c[torch.randperm(n, generator=g)[:M]] = torch.arange(M)
    return c


def torch_sums(m, thr, onehot):
    """(k_i(m), s_i(m)) [S, n, M] the way one writes them in torch: the mask, the kept weights, two products."""
    S, n, _ = m.shape
    eye = torch.eye(n, dtype=torch.bool, device=m.device)
    mask = (m > thr.view(S, 1, 1)) & (m > 0) & ~eye
    a = torch.where(mask, m, 0.0)
    hot = onehot.unsqueeze(0).expand(S, n, -1)
    return torch.bmm(mask.to(m.dtype), hot), torch.bmm(a, hot)


def _participation(v):
    total = v.sum(2, keepdim=True)
    return torch.where(total.squeeze(2) > 0, 1 - ((v / total) ** 2).sum(2), 0.0)


def _zscore(v, onehot, c):
    count = onehot.sum(0)
    mean = (v @ onehot) / count
    dev = v - mean[:, c]
    std = torch.sqrt(((dev * dev) @ onehot) / count)
    return torch.where(std[:, c] > 0, dev / std[:, c], 0.0)


def torch_measures(m, thr, onehot, c, names):
    km, sm = torch_sums(m, thr, onehot)
    M = onehot.shape[1]
    cols = []
    for name in names:
        if name == "participation":
            cols.append(_participation(km))
        elif name == "weighted_participation":
            cols.append(_participation(sm))
        elif name == "module_zscore":
            cols.append(_zscore(km.gather(2, c.view(1, -1, 1).expand(km.shape[0], -1, 1)).squeeze(2), onehot, c))
        elif name == "weighted_module_zscore":
            cols.append(_zscore(sm.gather(2, c.view(1, -1, 1).expand(sm.shape[0], -1, 1)).squeeze(2), onehot, c))
        else:
            s = sm.sum(2, keepdim=True)
            p = sm / s
            h = torch.where(p > 0, p * torch.log(p), 0.0).sum(2)
            cols.append(torch.where(s.squeeze(2) > 0, -h / math.log(M), 0.0) if M > 1 else torch.zeros_like(h))
    return torch.stack(cols, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x360:7,4096x360:17,32768x84:7")
    ap.add_argument("--keep", type=float, default=0.10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("modules_time.py measures on a ROCm GPU; none is visible")
    out = {"rounds": args.rounds, "keep": args.keep, "points": []}
    names = ingest.MODULE_MEASURES
    for spec in args.points.split(","):
        shape, M = spec.split(":")
        S, n = (int(v) for v in shape.split("x"))
        M = int(M)
        torch.cuda.empty_cache()
        m = cohort(S, n)
        work = torch.empty_like(m)
        c = partition(n, M)
        c_dev = c.cuda()
        onehot = torch.nn.functional.one_hot(c_dev, M).to(m.dtype)
        thr = ingest.select_thresholds(m, keep=args.keep)
        variants = {
            "copy": lambda: work.copy_(m),
            "all_five": lambda: ingest.node_measures(m, min_weight=thr, measures=names, modules=c),
            "participation_pair": lambda: ingest.node_measures(m, min_weight=thr, measures=PAIR, modules=c),
            "profile": lambda: ingest.module_profile(m, c, min_weight=thr),
            "torch_all_five": lambda: torch_measures(m, thr, onehot, c_dev, names),
            "torch_participation_pair": lambda: torch_measures(m, thr, onehot, c_dev, PAIR),
            "torch_profile": lambda: torch_sums(m, thr, onehot)[1],
        }
        for fn in variants.values():                                       # warm-up of all
            fn()
        head, head_thr = m[:64].contiguous(), thr[:64].contiguous()
        diff = (ingest.node_measures(head, min_weight=head_thr, measures=names, modules=c)
                - torch_measures(head, head_thr, onehot, c_dev, names)).abs().amax((0, 1)).tolist()
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
        point = {"S": S, "n": n, "M": M, "cohort_bytes": cohort_bytes,
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_over_copy": med[name] / med["copy"] for name in ms if name != "copy"},
                 **{f"torch_over_kernel_{name}": med["torch_" + name] / med[name]
                    for name in ("all_five", "participation_pair", "profile")},
                 **{name + "_peak_bytes_above_inputs": p for name, p in peak.items() if name != "copy"},
                 "copy_bytes_per_s_at_median": 2 * cohort_bytes / (med["copy"] * 1e-3),
                 "all_five_read_bytes_per_s_at_median": cohort_bytes / (med["all_five"] * 1e-3),
                 "max_abs_difference_to_torch_first_64_subjects": dict(zip(names, diff))}
        del work
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del m
    print(json.dumps(out))


if __name__ == "__main__":
    main()
