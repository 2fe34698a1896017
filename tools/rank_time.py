#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest.rank_timeseries (csrc/rank.hip) beside a plain copy of the same
cohort, the Spearman connectivity it feeds beside the Pearson one, and a torch formulation of the mid-ranks on the same
GPU.

    python tools/rank_time.py [--points 4096x1200x360,8192x1200x84] [--window 300] [--stride 100] [--censored 0.2]
                              [--rounds 5] [--only a,b] [--skip-torch]

A point is S x T x n.  Per point, on one resident cohort of seeded time series (tools/timeseries_time.py's) and a seeded
mask that censors the same share of every subject's frames at random (tools/censor_time.py's):

  rank            ingest.rank_timeseries(ts, out=work)
  rank_in_place   ingest.rank_timeseries(work, out=work)
  rank_masked     ingest.rank_timeseries(ts, sample_mask=keep, out=work)
  rank_windows    ingest.rank_timeseries(ts, window=, stride=, out=units): [U, L, n], W L / T times the cohort
  copy            work.copy_(ts): the streaming floor
  corr            ingest.correlation_matrices(ts)
  corr_rank       ingest.correlation_matrices(ts, rank=True)
  torch           torch.sort along the frames, torch.searchsorted left and right on the sorted columns:
                  rank = (left + right + 1) / 2, the same mid-ranks (checked against rank_timeseries, bit for bit)

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, with torch.cuda.max_memory_allocated above the resident inputs for each, and
the rates the copy and the ranking make of the bytes they must move (one read and one write of the cohort).  One JSON
line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import _lib, ingest  # noqa: E402
from tools.censor_time import random_mask  # noqa: E402
from tools.timeseries_time import cohort, spread, timed  # noqa: E402


def torch_ranks(ts):
    """[S, T, n] fp32: the mid-ranks by one sort and two binary searches per value."""
    x = ts.transpose(1, 2).contiguous()                                   # frames last: sort and search run along them
    v = torch.sort(x, dim=2).values
    lo = torch.searchsorted(v, x, right=False)                            # values below
    hi = torch.searchsorted(v, x, right=True)                             # values below or equal
    del v, x
    r = lo.add_(hi).add_(1).to(torch.float32).mul_(0.5)
    del lo, hi
    return r.transpose(1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x1200x360,8192x1200x84")
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--stride", type=int, default=100)
    ap.add_argument("--censored", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated variants to time (default: all)")
    ap.add_argument("--skip-torch", action="store_true", help="leave the torch formulation out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_time.py measures on a ROCm GPU; none is visible")
    out = {"rounds": args.rounds, "window": args.window, "stride": args.stride, "censored": args.censored,
           "library": _lib.LIB_PATH, "points": []}
    for spec in args.points.split(","):
        S, T, n = (int(v) for v in spec.split("x"))
        torch.cuda.empty_cache()
        ts = cohort(S, T, n)
        keep = random_mask(S, T, args.censored)
        work = ts.clone()
        W = (T - args.window) // args.stride + 1
        units = torch.empty(S * W, args.window, n, device="cuda")
        variants = {
            "rank": lambda: ingest.rank_timeseries(ts, out=work),
            "rank_in_place": lambda: ingest.rank_timeseries(work, out=work),
            "rank_masked": lambda: ingest.rank_timeseries(ts, sample_mask=keep, out=work),
            "rank_windows": lambda: ingest.rank_timeseries(ts, window=args.window, stride=args.stride, out=units),
            "copy": lambda: work.copy_(ts),
            "corr": lambda: ingest.correlation_matrices(ts),
            "corr_rank": lambda: ingest.correlation_matrices(ts, rank=True),
            "torch": lambda: torch_ranks(ts),
        }
        if args.skip_torch:
            del variants["torch"]
        if args.only:
            variants = {name: variants[name] for name in args.only.split(",")}
        same = None
        for name, fn in variants.items():                                 # warm-up of all
            got = fn()
            if name == "torch":
                same = bool(torch.equal(got.view(torch.int32), ingest.rank_timeseries(ts).view(torch.int32)))
            del got
        ms = {name: [] for name in variants}
        peak = {name: 0 for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                if name == "rank_in_place":
                    work.copy_(ts)
                t, p, _ = timed(fn)
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        cohort_bytes = 4 * S * T * n
        moved = {name: 2 * cohort_bytes for name in ("rank", "rank_in_place", "copy") if name in variants}
        point = {"S": S, "T": T, "n": n, "units_of_the_windows": S * W, "kept_frames": int(keep[0].sum()),
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_peak_bytes_above_inputs": p for name, p in peak.items()},
                 **{name + "_bytes_per_s_at_median": b / (spread(ms[name])["median"] * 1e-3) for name, b in moved.items()},
                 "cohort_bytes": cohort_bytes, "windows_bytes": 4 * S * W * args.window * n,
                 "torch_gives_the_same_bits": same}
        for a, b in (("rank", "copy"), ("torch", "rank"), ("corr_rank", "corr")):
            if a in ms and b in ms:
                point[f"{a}_over_{b}_at_median"] = spread(ms[a])["median"] / spread(ms[b])["median"]
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del work, units, keep, ts, variants
    print(json.dumps(out))


if __name__ == "__main__":
    main()
