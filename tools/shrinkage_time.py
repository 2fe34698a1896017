#!/usr/bin/env python3
"""Time the Ledoit-Wolf shrinkage estimate (csrc/shrinkage.hip, k_lw) against its yardsticks.

    python tools/shrinkage_time.py [--points 4096x1200x360,32768x1200x84,4096x1200x360:300:100] [--rounds 5]
    python tools/shrinkage_time.py --kernel-trace DIR        # summarise a rocprofv3 kernel trace of the line above

A point is S x T x n, optionally :window:stride.  Per point, on one resident cohort of seeded time series whose
statistics and signed correlations cgnn_ingest_corr has left on the device:

  lw       cgnn_ingest_shrinkage alone: the one launch of k_lw
  corr     cgnn_ingest_corr alone: k_corr_stats + k_corr, the two launches in front of it
  partial  ingest.partial_correlation(R, shrinkage=0.1): the scalar path, which this estimate must not slow down
  each     ingest.partial_correlation(R, shrinkage=alpha): the same kernel reading a value per unit
  torch    the plain-torch device formulation of the estimate in fp32: (unfold the windows,) standardise,
           (z * z).sum(-1), R.square().sum(); the largest difference between the two results is reported.

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, with the bytes k_lw must move (the frames of every unit once, the upper
triangles once) and its rate on them, torch.cuda.max_memory_allocated above the resident data for lw and torch, and the
largest error of lw against the fp64 host statement (tests/shrinkage_data.py) on the first two units with its ratio to
2^-24 cond.  --end-to-end adds ingest.from_timeseries(kind="partial") with shrinkage="ledoit_wolf" against
shrinkage=0.1.  One JSON line.

k_corr_stats, the yardstick that streams the same frames, has no call of its own: run the tool under
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/shrinkage_time.py --points P --skip-torch` and
give DIR to --kernel-trace, which prints the median duration of every k_lw / k_corr_stats / k_corr / k_partial
dispatch and the ratio k_lw / k_corr_stats.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import _lib, ingest  # noqa: E402
from tests import shrinkage_data as D  # noqa: E402
from tests import timeseries_data as TS  # noqa: E402
from tools.timeseries_time import cohort, spread, timed  # noqa: E402

KERNELS = ("k_lw", "k_corr_stats", "k_corr<", "k_partial<")


def summarise_trace(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    ms = {k: [] for k in KERNELS}
    for row in csv.DictReader(open(files[0])):
        for k in KERNELS:
            if "::" + k in row["Kernel_Name"]:
                ms[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    out = {k.rstrip("<"): {"calls": len(v), **spread(v)} for k, v in ms.items() if v}
    if ms["k_lw"] and ms["k_corr_stats"]:
        out["k_lw_over_k_corr_stats"] = statistics.median(ms["k_lw"]) / statistics.median(ms["k_corr_stats"])
    print(json.dumps(out))


def torch_device(ts, R, window, stride):
    """[U] by standardise + two reductions, all fp32."""
    x = ts
    if window is not None:
        x = ts.unfold(1, window, stride).permute(0, 1, 3, 2).reshape(-1, window, ts.shape[2])  # the unfolded copy
    L = x.shape[1]
    d = x - x.mean(1, keepdim=True)
    q = (d * d).sum(1, keepdim=True)
    rs = torch.where(q > 0, torch.rsqrt(q), torch.zeros_like(q))
    z = d * rs
    del d
    s = (z * z).sum(-1)
    B = L * (s * s).sum(1)
    F = R.square().sum((1, 2))
    O = F - (q.squeeze(1) > 0).sum(1)
    return torch.where(O > 0, ((B - F) / (L * O)).clamp(0.0, 1.0), torch.zeros_like(O))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x1200x360,32768x1200x84,4096x1200x360:300:100")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="leave the torch formulation out (for a kernel trace)")
    ap.add_argument("--end-to-end", action="store_true", help="also from_timeseries(ledoit_wolf | 0.1)")
    ap.add_argument("--kernel-trace", metavar="DIR", help="summarise a rocprofv3 kernel trace and exit")
    args = ap.parse_args()
    if args.kernel_trace:
        return summarise_trace(args.kernel_trace)
    if not torch.cuda.is_available():
        raise SystemExit("shrinkage_time.py measures on a ROCm GPU; none is visible")
    lib = _lib.load()
    sp = _lib.stream_ptr()
    out = {"rounds": args.rounds, "points": []}
    held = (None, None)
    for spec in args.points.split(","):
        shape, *win = spec.split(":")
        S, T, n = (int(v) for v in shape.split("x"))
        window = int(win[0]) if win else None
        stride = int(win[1]) if len(win) > 1 else window
        if held[0] != (S, T, n):
            held = (None, None)
            torch.cuda.empty_cache()
            held = ((S, T, n), cohort(S, T, n))
        ts = held[1]
        W = TS.num_windows(T, window, stride)
        U, L = S * W, window or T
        stats = torch.empty(U, n, 2, device="cuda")
        R = torch.empty(U, n, n, device="cuda")
        alpha = torch.empty(U, dtype=torch.float64, device="cuda")
        wargs = (window or 0, stride or 0)

        def corr():
            _lib.check(lib.cgnn_ingest_corr(_lib.ptr(ts), S, T, n, *wargs, 0, _lib.ptr(stats), _lib.nbytes(stats),
                                            _lib.ptr(R), _lib.nbytes(R), sp), "cgnn_ingest_corr")

        def lw():
            _lib.check(lib.cgnn_ingest_shrinkage(_lib.ptr(ts), S, T, n, *wargs, _lib.ptr(stats), _lib.ptr(R),
                                                 _lib.ptr(alpha), _lib.nbytes(alpha), sp), "cgnn_ingest_shrinkage")

        variants = {"lw": lw, "corr": corr, "partial": lambda: ingest.partial_correlation(R, shrinkage=0.1),
                    "each": lambda: ingest.partial_correlation(R, shrinkage=alpha)}
        if not args.skip_torch:
            variants["torch"] = lambda: torch_device(ts, R, window, stride)
        corr()
        lw()
        head = ts[:2].cpu()
        want = D.host_cohort(head, window, stride)
        got = alpha[:2 * W].cpu()
        conds = [D.cond(head[s, w * (stride or 0):w * (stride or 0) + L]) for s in range(2) for w in range(W)]
        err = (got - want).abs()
        diff = None
        for name, fn in variants.items():                             # warm-up of all
            res = fn()
            if name == "torch":
                diff = float((res.double() - alpha).abs().max())
            del res
        ms = {name: [] for name in variants}
        peak = {name: 0 for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                t, p, _ = timed(fn)
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        frames_bytes, tri_bytes = 4 * U * L * n, 4 * U * (n * (n - 1) // 2)
        med = statistics.median(ms["lw"])
        point = {"S": S, "T": T, "n": n, "window": window, "stride": stride, "units": U,
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 "lw_frames_bytes": frames_bytes, "lw_triangle_bytes": tri_bytes,
                 "lw_gb_per_s": (frames_bytes + tri_bytes) / med / 1e6,
                 "lw_peak_bytes_above_input": peak["lw"], "torch_peak_bytes_above_input": peak.get("torch"),
                 "alpha_min_median_max": [float(alpha.min()), float(alpha.median()), float(alpha.max())],
                 "max_abs_diff_lw_vs_torch": diff, "max_abs_err_vs_fp64_first_2_subjects": float(err.max()),
                 "err_over_eps_cond": max(float(e) / (D.EPS * k) for e, k in zip(err, conds) if k > 0)}
        if args.end_to_end:
            y = torch.arange(S, dtype=torch.long) % 2
            e2e = {}
            for name, a in (("0.1", 0.1), ("ledoit_wolf", "ledoit_wolf")):
                fn = lambda: ingest.from_timeseries(ts, y, keep=0.1, window=window, stride=stride,   # noqa: E731
                                                    kind="partial", shrinkage=a)
                fn()
                e2e[name] = spread([timed(fn)[0] for _ in range(args.rounds)])
            point["from_timeseries_ms"] = e2e
        del stats, R, alpha
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
