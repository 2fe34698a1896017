#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest.knn_sparsify (csrc/knn.hip) beside a plain copy of the cohort and the
torch formulation of the same graph on the same GPU.

    python tools/knn_time.py [--points 4096x360,32768x84] [--ks 8,36] [--rounds 5]

A point is S x n.  Per point, on one resident cohort of seeded symmetric matrices (tools/ingest_time.py's), and per k:

  knn_<mode>            ingest.knn_sparsify(m, k, mode=mode, out=work), for the three modes
  knn_<mode>_in_place   ingest.knn_sparsify(work, k, mode=mode, out=work) on a fresh copy (the copy is not timed)
  torch_union           topk, scatter_ into a mask, mask | mask.mT, where -- with its peak memory above the inputs
  copy                  work.copy_(m): the streaming floor, the call must read and write the cohort once

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, the ratio of every knn median to the copy's, and whether the kernel's "union"
equals the torch formulation on the first 64 subjects (the cohort is continuous: no ties).  One JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import ingest  # noqa: E402
from tools.ingest_time import cohort, spread, timed  # noqa: E402


def torch_union(m, k):
    """The "union" k-NN graph of ``m`` ``[S, n, n]`` in torch (ties in topk's order, not by column)."""
    S, n, _ = m.shape
    eye = torch.eye(n, dtype=torch.bool, device=m.device)
    cand = (m > 0) & ~eye
    keyed = torch.where(cand, m, float("-inf"))
    idx = keyed.topk(min(k, n), dim=2).indices
    del keyed
    mask = torch.zeros(S, n, n, dtype=torch.bool, device=m.device)
    mask.scatter_(2, idx, True)
    mask &= cand                                       # a row with fewer than k candidates
    mask = mask | (mask.mT & (m > 0))
    return torch.where(mask, m, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x360,32768x84")
    ap.add_argument("--ks", default="8,36")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_time.py measures on a ROCm GPU; none is visible")
    ks = [int(v) for v in args.ks.split(",")]
    out = {"rounds": args.rounds, "ks": ks, "points": []}
    for spec in args.points.split(","):
        S, n = (int(v) for v in spec.split("x"))
        torch.cuda.empty_cache()
        m = cohort(S, n)
        work = torch.empty_like(m)
        variants, fresh = {"copy": lambda: work.copy_(m)}, set()
        for k in ks:
            for mode in ingest.KNN_MODES:
                variants[f"knn_{mode}_k{k}"] = lambda k=k, mode=mode: ingest.knn_sparsify(m, k, mode=mode, out=work)
                variants[f"knn_{mode}_in_place_k{k}"] = lambda k=k, mode=mode: ingest.knn_sparsify(work, k, mode=mode,
                                                                                                   out=work)
                fresh.add(f"knn_{mode}_in_place_k{k}")
            variants[f"torch_union_k{k}"] = lambda k=k: torch_union(m, k)
        equal = {}
        for name, fn in variants.items():                                  # warm-up of all
            if name in fresh:
                work.copy_(m)
            fn()
        for k in ks:
            head = m[:64].contiguous()
            equal[f"k{k}"] = bool(torch.equal(ingest.knn_sparsify(head, k), torch_union(head, k)))
        ms = {name: [] for name in variants}
        peak = {name: 0 for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                if name in fresh:
                    work.copy_(m)
                t, p, res = timed(fn)
                del res
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        copy_ms = spread(ms["copy"])["median"]
        cohort_bytes = 4 * S * n * n
        point = {"S": S, "n": n, "cohort_bytes": cohort_bytes,
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_over_copy": spread(v)["median"] / copy_ms for name, v in ms.items() if name != "copy"},
                 **{name + "_peak_bytes_above_inputs": p for name, p in peak.items() if name.startswith("torch")},
                 "copy_bytes_per_s_at_median": 2 * cohort_bytes / (copy_ms * 1e-3),
                 "union_equals_torch_first_64_subjects": equal}
        del work
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del m
    print(json.dumps(out))


if __name__ == "__main__":
    main()
