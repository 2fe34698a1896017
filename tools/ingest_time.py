#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest.from_matrices (csrc/ingest.hip) against what it replaces.

    python tools/ingest_time.py [--shapes 4096x360,32768x84] [--keeps 0.1,0.02] [--rounds 3] [--host-subjects 16]

Per shape S x n and density `keep`, on one resident cohort of seeded symmetric matrices (values in (0, 1)):

  new    ingest.from_matrices(matrices, labels, keep=keep)  -- select + count, running sums, fill, default feature
  torch  the plain-torch device formulation: diagonal and NaN to -inf, `sort` over [S, n^2], the value of rank k,
         mask, `nonzero`, the per-subject cut (counts + cumsum).  It runs without csrc/ingest.hip and gives the same
         edge arrays (checked here on every shape before anything is timed).
  host   the recipe of tests/ingest_data.py per subject on the CPU (sort, mask, nonzero), timed on the first
         --host-subjects subjects and scaled to S: what users of the package do today.

Every shape is warmed up by both device variants first; the two then alternate for --rounds rounds in this one
process, each call between two HIP events; min / median / max are reported, with torch.cuda.max_memory_allocated
above the resident cohort for each variant, and the bytes of the traffic model of DESIGN.md 4.3b.  One JSON line.
Under `rocprofv3 --kernel-trace --stats -- python tools/ingest_time.py --rounds 1 --host-subjects 0` the kernel
statistics hold k_ingest / k_ingest_fill next to the torch kernels of the sort formulation.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import ingest  # noqa: E402
from tests import ingest_data as D  # noqa: E402


def cohort(S, n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(S, n, n, device="cuda")
    step = max(1, (1 << 26) // (n * n))
    for lo in range(0, S, step):                       # in slices: no second cohort-sized temporary
        r = torch.rand(min(step, S - lo), n, n, device="cuda", generator=g)
        out[lo:lo + step] = (r + r.transpose(1, 2)) / 2
    return out


def torch_device(mats, k):
    """(edge_local [2, E], edge_weight [E], edge_ptr [S + 1] on the device) by sort + mask + nonzero."""
    S, n, _ = mats.shape
    eye = torch.eye(n, dtype=torch.bool, device=mats.device)
    if k < n * (n - 1):
        cand = torch.where(torch.isnan(mats) | eye, float("-inf"), mats)
        thr = torch.sort(cand.view(S, n * n), dim=1, descending=True).values[:, k]
        del cand
    else:
        thr = torch.full((S,), float("-inf"), device=mats.device)
    mask = (mats > thr.view(S, 1, 1)) & (mats > 0) & ~eye
    idx = mask.nonzero()                               # global (s, i, j) order
    edge_ptr = torch.zeros(S + 1, dtype=torch.long, device=mats.device)
    edge_ptr[1:] = torch.cumsum(mask.view(S, -1).sum(1), 0)
    return idx[:, 1:].t().contiguous(), mats[mask], edge_ptr


def timed(fn):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e), torch.cuda.max_memory_allocated() - base, out


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def host_seconds(mats, k, subjects):
    if subjects <= 0:
        return None
    sub = mats[:subjects].cpu()
    t0 = time.perf_counter()
    for A in sub:
        D.host_edges(A, D.host_threshold(A, k))
    return (time.perf_counter() - t0) / subjects * mats.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x360,32768x84")
    ap.add_argument("--keeps", default="0.1,0.02")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-subjects", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_time.py measures on a ROCm GPU; none is visible")
    out = {"rounds": args.rounds, "points": []}
    for shape in args.shapes.split(","):
        S, n = (int(v) for v in shape.split("x"))
        mats = cohort(S, n)
        labels = torch.zeros(S, dtype=torch.long, device="cuda")
        for keep in (float(v) for v in args.keeps.split(",")):
            k = D.rank_of(n, keep=keep)
            new = lambda: ingest.from_matrices(mats, labels, keep=keep)      # noqa: E731
            old = lambda: torch_device(mats, k)                             # noqa: E731
            ds, ref = new(), old()                                           # warm-up of both, and the same arrays
            same = torch.equal(ds.edge_local, ref[0]) and torch.equal(ds.edge_weight, ref[1]) \
                and torch.equal(ds.edge_ptr_dev, ref[2])
            E = int(ds.edge_ptr[-1])
            del ds, ref
            ms = {"new": [], "torch": [], "select_only": []}
            peak = {"new": 0, "torch": 0}
            for _ in range(args.rounds):
                for name, fn in (("new", new), ("torch", old)):
                    t, p, _ = timed(fn)
                    ms[name].append(t)
                    peak[name] = max(peak[name], p)
                ms["select_only"].append(timed(lambda: ingest.select_thresholds(mats, keep=keep))[0])
            # traffic model: select + count read the cohort once from HBM (their repeat passes are
            # meant to hit cache), fill reads it again; outputs 20 B per edge, 12 + 8 B per row of bookkeeping
            model = 2 * 4 * S * n * n + 20 * E + 20 * S * n + 4 * S * n
            point = {"S": S, "n": n, "keep": keep, "k": k, "edges": E, "same_arrays": same,
                     "new_ms": spread(ms["new"]), "torch_ms": spread(ms["torch"]),
                     "select_only_ms": spread(ms["select_only"]),
                     "new_peak_bytes_above_cohort": peak["new"], "torch_peak_bytes_above_cohort": peak["torch"],
                     "cohort_bytes": 4 * S * n * n, "model_bytes": model,
                     "model_gb_per_s": model / statistics.median(ms["new"]) / 1e6,
                     "host_s_scaled": host_seconds(mats, k, min(args.host_subjects, S))}
            out["points"].append(point)
            print(json.dumps(point), file=sys.stderr, flush=True)
        del mats
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
