#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest.mst_backbone (csrc/mst.hip) beside a plain copy of the cohort,
knn_sparsify and scipy's spanning tree per subject on the host.

    python tools/mst_time.py [--points 4096x360,32768x84] [--keep 0.10] [--knn 8] [--rounds 5] [--host-subjects 32]

A point is S x n.  Per point, on one resident cohort of seeded symmetric matrices (tools/ingest_time.py's):

  mst_tree               ingest.mst_backbone(m, out=work): the tree alone
  mst_tree_in_place      ingest.mst_backbone(work, out=work) on a fresh copy (the copy is not timed)
  mst_keep               ingest.mst_backbone(m, keep=keep, out=work): the selection of the thresholds and the kernel
  mst_keep_in_place      the same in place, on a fresh copy
  mst_thresholds_given   ingest.mst_backbone(m, min_weight=t, out=work) with the selected thresholds t: the kernel alone
  select                 ingest.select_thresholds(m, keep=keep): the other launch of mst_keep
  knn_union              ingest.knn_sparsify(m, knn, out=work)
  copy                   work.copy_(m): the streaming floor, the call must read and write the cohort once

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported and the ratio of every median to the copy's.  scipy's minimum_spanning_tree of
``max + 1 - W`` runs on --host-subjects subjects on the host (the matrices already there) and is scaled to the cohort:
the only route a user has without the kernel, the copy of the cohort off the device not counted.  The cohort is
continuous (no ties), so the kernel's tree must be scipy's: that is checked on those subjects.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import ingest  # noqa: E402
from tools.ingest_time import cohort, spread, timed  # noqa: E402


def scipy_trees(sub):
    """(seconds, [n, n] bool masks) of scipy's spanning trees of the host matrices ``sub`` ``[s, n, n]``."""
    from scipy.sparse.csgraph import minimum_spanning_tree
    masks = []
    t0 = time.perf_counter()
    for A in sub.numpy():
        W = np.maximum(np.where(A > 0, A, 0), np.where(A.T > 0, A.T, 0)).astype(np.float64)
        np.fill_diagonal(W, 0)
        cost = np.where(W > 0, W.max() + 1 - W, 0)      # (a dense zero is no edge to csgraph)
        masks.append(minimum_spanning_tree(cost).toarray() > 0)
    seconds = time.perf_counter() - t0
    return seconds, [torch.from_numpy(t | t.T) for t in masks]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x360,32768x84")
    ap.add_argument("--keep", type=float, default=0.10)
    ap.add_argument("--knn", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-subjects", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mst_time.py measures on a ROCm GPU; none is visible")
    out = {"rounds": args.rounds, "keep": args.keep, "knn": args.knn, "points": []}
    for spec in args.points.split(","):
        S, n = (int(v) for v in spec.split("x"))
        torch.cuda.empty_cache()
        m = cohort(S, n)
        work = torch.empty_like(m)
        thr = ingest.select_thresholds(m, keep=args.keep)
        variants = {
            "copy": lambda: work.copy_(m),
            "mst_tree": lambda: ingest.mst_backbone(m, out=work),
            "mst_tree_in_place": lambda: ingest.mst_backbone(work, out=work),
            "mst_keep": lambda: ingest.mst_backbone(m, keep=args.keep, out=work),
            "mst_keep_in_place": lambda: ingest.mst_backbone(work, keep=args.keep, out=work),
            "mst_thresholds_given": lambda: ingest.mst_backbone(m, min_weight=thr, out=work),
            "select": lambda: ingest.select_thresholds(m, keep=args.keep),
            "knn_union": lambda: ingest.knn_sparsify(m, args.knn, out=work),
        }
        fresh = {"mst_tree_in_place", "mst_keep_in_place"}
        for name, fn in variants.items():                                  # warm-up of all
            if name in fresh:
                work.copy_(m)
            fn()
        ms = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                if name in fresh:
                    work.copy_(m)
                t, _, res = timed(fn)
                del res
                ms[name].append(t)
        copy_ms = spread(ms["copy"])["median"]
        cohort_bytes = 4 * S * n * n
        point = {"S": S, "n": n, "cohort_bytes": cohort_bytes,
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_over_copy": spread(v)["median"] / copy_ms for name, v in ms.items() if name != "copy"},
                 "copy_bytes_per_s_at_median": 2 * cohort_bytes / (copy_ms * 1e-3)}
        subjects = min(args.host_subjects, S)
        if subjects > 0:
            head = m[:subjects].contiguous()
            seconds, trees = scipy_trees(head.cpu())
            kept = (ingest.mst_backbone(head) > 0).cpu()
            point["scipy_host_ms_scaled_to_cohort"] = seconds / subjects * S * 1e3
            point["scipy_host_subjects"] = subjects
            point["tree_equals_scipy_on_those_subjects"] = all(bool(torch.equal(k, t)) for k, t in zip(kept, trees))
        del work
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del m
    print(json.dumps(out))


if __name__ == "__main__":
    main()
