#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest.partial_correlation (csrc/partial.hip) against what it replaces.

    python tools/partial_time.py [--points 4096x1200x360,32768x400x84] [--shrinkage 0.1] [--rounds 3] [--end-to-end]

A point is U x T x n: the correlation matrices of U units of T frames and n ROIs, built on the device by
ingest.correlation_matrices in slices of units (the time series of a slice are dropped again).  Per point:

  new    ingest.partial_correlation(R, shrinkage=)  -- one launch, a slab per workgroup
  torch  the solver-library formulation on the same GPU: (1 - a) R + a I, torch.linalg.cholesky,
         torch.cholesky_inverse, the normalisation, the clamp and the diagonal.  It runs without csrc/partial.hip; the
         largest difference between the two results is reported.

Both variants are warmed up first; the two then alternate for --rounds rounds in this one process, each call between
two HIP events; min / median / max are reported, with torch.cuda.max_memory_allocated above the resident matrices for
each variant, the workspace of the new call, its rate on the ~ n^3 multiply-adds of a unit as a fraction of the fp32
matrix pipe (157.3 TFLOP/s), and the largest error of `new` against the fp64 host statement (tests/partial_data.py)
on the first two units with its ratio to kappa 2^-24.  --end-to-end adds ingest.from_timeseries(kind="partial")
against kind="correlation" on the time series of the point (then held whole: U x T x n floats).  One JSON line.
Under `rocprofv3 --kernel-trace --stats -- python tools/partial_time.py --rounds 1 --skip-torch` the kernel
statistics hold k_partial.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import _lib, ingest  # noqa: E402
from tests import partial_data as D  # noqa: E402
from tools.timeseries_time import cohort, spread, timed  # noqa: E402

PIPE_TFLOPS = 157.3                               # fp32 matrix pipe of the MI355X


def matrices(U, T, n, keep_series):
    """([U, n, n] correlations on the device, the time series if asked for)"""
    if keep_series:
        ts = cohort(U, T, n)
        return ingest.correlation_matrices(ts), ts
    out = torch.empty(U, n, n, device="cuda")
    step = max(1, (1 << 27) // (T * n))
    for lo in range(0, U, step):
        k = min(step, U - lo)
        out[lo:lo + k] = ingest.correlation_matrices(cohort(k, T, n, seed=lo))
    return out, None


def torch_device(R, a):
    """[U, n, n] through the solver library, all fp32."""
    n = R.shape[1]
    C = (1.0 - a) * R
    C.diagonal(dim1=1, dim2=2).add_(a)
    L = torch.linalg.cholesky(C)
    del C
    P = torch.cholesky_inverse(L)
    del L
    d = torch.rsqrt(P.diagonal(dim1=1, dim2=2))
    out = (-P * d[:, :, None] * d[:, None, :]).clamp_(-1.0, 1.0)
    out.diagonal(dim1=1, dim2=2).fill_(1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x1200x360,32768x400x84")
    ap.add_argument("--shrinkage", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true", help="time the new call alone (for a kernel trace)")
    ap.add_argument("--end-to-end", action="store_true", help="also from_timeseries(kind=partial | correlation)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("partial_time.py measures on a ROCm GPU; none is visible")
    a = args.shrinkage
    out = {"rounds": args.rounds, "shrinkage": a, "points": []}
    for spec in args.points.split(","):
        U, T, n = (int(v) for v in spec.split("x"))
        torch.cuda.empty_cache()
        R, ts = matrices(U, T, n, args.end_to_end)
        new = lambda: ingest.partial_correlation(R, shrinkage=a)                          # noqa: E731
        old = lambda: torch_device(R, a)                                                  # noqa: E731
        got = new()                                                                       # warm-up of both
        head = R[:2].cpu()
        kappa = D.kappa_of(head, a)
        err64 = float((got[:2].cpu().double() - D.host_partial(head, a)).abs().max())
        nan_units = int(torch.isnan(got.view(U, -1)[:, 0]).sum())
        diff = None
        if not args.skip_torch:
            ref = old()
            diff = float((got - ref).abs().max())
            del ref
        del got
        ms = {"new": [], "torch": []}
        peak = {"new": 0, "torch": 0}
        for _ in range(args.rounds):
            for name, fn in (("new", new), ("torch", old)):
                if name == "torch" and args.skip_torch:
                    continue
                t, p, _ = timed(fn)
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        med = statistics.median(ms["new"])
        macs = U * n ** 3                         # factorisation n^3 / 3, the inverse n^3 / 3, W^T W n^3 / 3
        tflops = 2 * macs / med / 1e9
        point = {"U": U, "T": T, "n": n, "new_ms": spread(ms["new"]),
                 "torch_ms": spread(ms["torch"]) if ms["torch"] else None,
                 "new_peak_bytes_above_input": peak["new"], "torch_peak_bytes_above_input": peak["torch"],
                 "output_bytes": 4 * U * n * n,
                 "workspace_bytes": int(_lib.load().cgnn_ingest_partial_workspace_bytes(U, n)),
                 "macs_n3_per_unit": macs, "tflops_on_n3": tflops, "fraction_of_fp32_matrix_pipe": tflops / PIPE_TFLOPS,
                 "max_abs_diff_new_vs_torch": diff, "all_nan_units": nan_units, "kappa_first_2_units": kappa,
                 "max_abs_err_vs_fp64_first_2_units": err64, "err_over_kappa_eps": err64 / (kappa * D.EPS)}
        if args.end_to_end:
            y = torch.arange(U, dtype=torch.long) % 2
            e2e = {}
            for kind, kw in (("correlation", {}), ("partial", {"kind": "partial", "shrinkage": a})):
                fn = lambda: ingest.from_timeseries(ts, y, keep=0.1, **kw)                # noqa: E731
                fn()
                e2e[kind] = spread([timed(fn)[0] for _ in range(args.rounds)])
            point["from_timeseries_ms"] = e2e
        del R, ts
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
