#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest.filter_timeseries (csrc/filter.hip) against the torch formulation it replaces.

    python tools/filter_time.py [--points 4096x1200x360,8192x1200x84] [--t-r 0.72] [--bands 0.01:0.1,0.01:] [--rounds 5]

A point is S x T x n; a band is high_pass:low_pass in Hz, either side empty for none.  Per point and band, on one
resident cohort of seeded time series (tools/timeseries_time.py's, plus an offset of 100):

  new      ingest.filter_timeseries(ts, t_r=, high_pass=, low_pass=): the basis table, the means, k_filter
  inplace  the same with out=ts on a copy (what a pipeline that no longer needs the raw series calls)
  torch    the plain-torch device formulation in fp32: centre, then B @ (B.T @ xc) by torch.matmul against a resident
           [T, K] basis (built once, outside the timed call), subtracted from xc in the complement form; the same
           choice of form as the call.  The largest difference between the two results is reported in units of
           2^-24 max |xc|.

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, with torch.cuda.max_memory_allocated above the resident cohort for each (the
output included: 4 S T n bytes of it are the result), the bytes the call must move (the means' read, the coefficients'
read, the complement form's second read, one write), the multiply-adds k_filter issues (components padded to 32, frames
to 32, columns to 64) with the rates on both, and the largest error ratio of `new` against the fp64 host statement
(tests/filter_data.py) on the first two subjects.  One JSON line.
Under `rocprofv3 --kernel-trace --stats -- python tools/filter_time.py --rounds 1 --skip-torch` the kernel statistics
hold k_filter_basis / k_filter_mean / k_filter.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import ingest  # noqa: E402
from tests import filter_data as D  # noqa: E402
from tools.timeseries_time import cohort, spread, timed  # noqa: E402


def torch_device(ts, B, complement):
    """[S, T, n] by centre + two matmuls, all fp32."""
    xc = ts - ts.mean(1, keepdim=True)
    if B is None:
        return xc
    p = torch.matmul(B, torch.matmul(B.t(), xc))
    return xc.sub_(p) if complement else p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x1200x360,8192x1200x84")
    ap.add_argument("--t-r", type=float, default=0.72)
    ap.add_argument("--bands", default="0.01:0.1,0.01:")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="time the new call alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filter_time.py measures on a ROCm GPU; none is visible")
    out = {"rounds": args.rounds, "t_r": args.t_r, "points": []}
    for spec in args.points.split(","):
        S, T, n = (int(v) for v in spec.split("x"))
        torch.cuda.empty_cache()
        ts = cohort(S, T, n).add_(100.0)
        head = ts[:2].cpu()
        scale = float(D.centred(head[0]).abs().max())
        for band in args.bands.split(","):
            hp, lp = (float(v) if v else None for v in band.split(":"))
            kw = dict(t_r=args.t_r, high_pass=hp, low_pass=lp)
            k_lo, k_hi = ingest.filter_components(T, args.t_r, hp, lp)
            complement, comps = D.form(T, k_lo, k_hi)
            K = len(comps)
            B = D.basis(T, comps).float().cuda() if K else None
            work = ts.clone()
            variants = {"new": lambda: ingest.filter_timeseries(ts, **kw),
                        "inplace": lambda: ingest.filter_timeseries(work, out=work, **kw)}
            if not args.skip_torch:
                variants["torch"] = lambda: torch_device(ts, B, complement)
            got = variants["new"]()                                       # warm-up of all
            ratio = max(float(D.column_ratios(got[s].cpu(), head[s], args.t_r, hp, lp).max()) for s in range(2))
            variants["inplace"]()
            diff = None
            if not args.skip_torch:
                ref = variants["torch"]()
                diff = float((got - ref).abs().max()) / (D.EPS * scale)
                del ref
            del got
            ms = {name: [] for name in variants}
            peak = {name: 0 for name in variants}
            for _ in range(args.rounds):
                for name, fn in variants.items():
                    t, p, _ = timed(fn)
                    ms[name].append(t)
                    peak[name] = max(peak[name], p)
            cohort_bytes = 4 * S * T * n
            reads = 1 + (1 if K else 0) + (1 if complement else 0)        # means | coefficients | y = xc - ...
            model = (reads + 1) * cohort_bytes
            kpad = -(-K // 32) * 32
            macs = 2 * S * (-(-n // 64) * 64) * (-(-T // 32) * 32) * kpad
            med = statistics.median(ms["new"])
            point = {"S": S, "T": T, "n": n, "high_pass": hp, "low_pass": lp, "k_lo": k_lo, "k_hi": k_hi,
                     "form": "complement" if complement else "keep", "components": K, "kpad": kpad,
                     **{name + "_ms": spread(v) for name, v in ms.items()},
                     **{name + "_peak_bytes_above_input": p for name, p in peak.items()},
                     "cohort_bytes": cohort_bytes, "model_bytes": model, "model_gb_per_s": model / med / 1e6,
                     "useful_macs": 2 * S * n * T * K, "issued_macs": macs, "issued_tflops": 2 * macs / med / 1e9,
                     "max_diff_new_vs_torch_over_eps_scale": diff, "err_over_eps_scale_first_2_subjects": ratio,
                     "tolerance_of_the_tests": 4 * 15.95}
            del work, B
            out["points"].append(point)
            print(json.dumps(point), file=sys.stderr, flush=True)
        del ts
    print(json.dumps(out))


if __name__ == "__main__":
    main()
