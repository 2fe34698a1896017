#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest.interpolate_censored (csrc/interpolate.hip) and the band-pass under a
frame mask that it makes possible, beside the unmasked band-pass and a plain copy of the same run.

    python tools/interp_time.py [--points 4096x1200x360x24,8192x1200x84x24] [--t-r 0.72] [--high-pass 0.01]
                                [--low-pass 0.1] [--censored 0.2] [--rounds 5]

A point is S x T x n x q.  Per point, on one resident cohort of seeded time series (tools/timeseries_time.py's, plus an
offset of 100), seeded motion-like confounds (tools/confound_time.py's) and a seeded mask that censors the same share of
every subject's frames at random (tools/censor_time.py's):

  interp_in_place   ingest.interpolate_censored(work, mask, out=work)
  interp            ingest.interpolate_censored(ts, mask, out=work): the kept frames are copied as well
  band_masked       ingest.filter_timeseries(ts, band, sample_mask=, interpolate=True, out=work): interpolate, the
                    orthogonal DCT projection, masked centring
  band_masked_conf  the same with confounds=: the confounds interpolated and filtered too, their masked basis, the
                    regression on the kept frames
  band              the unmasked ingest.filter_timeseries(ts, band, out=work) of the same band
  copy              work.copy_(ts): the streaming floor

There is no torch formulation of a not-a-knot spline to stand beside these (torch has no banded or tridiagonal solve,
and a dense ``torch.linalg.solve`` of a 960 x 960 system per subject is another algorithm on another scale), so none is
invented: the yardsticks are the copy and the unmasked band-pass.

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, with torch.cuda.max_memory_allocated above the resident inputs for each, the
bytes the interpolation must move (the kept frames twice, the censored frames once, out of place the kept frames once
more; the workspace's own traffic is left out) and the rate that makes at the median, and the largest ratio of
``interpolate_censored`` against the fp64 host statement (tests/interp_data.py) on the first two subjects.  One JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import _lib, ingest  # noqa: E402
from tests import interp_data as I  # noqa: E402
from tools.censor_time import random_mask  # noqa: E402
from tools.confound_time import motion  # noqa: E402
from tools.timeseries_time import cohort, spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x1200x360x24,8192x1200x84x24")
    ap.add_argument("--t-r", type=float, default=0.72)
    ap.add_argument("--high-pass", type=float, default=0.01)
    ap.add_argument("--low-pass", type=float, default=0.1)
    ap.add_argument("--censored", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interp_time.py measures on a ROCm GPU; none is visible")
    band = dict(t_r=args.t_r, high_pass=args.high_pass, low_pass=args.low_pass)
    out = {"rounds": args.rounds, **band, "censored": args.censored, "points": []}
    for spec in args.points.split(","):
        S, T, n, q = (int(v) for v in spec.split("x"))
        torch.cuda.empty_cache()
        ts = cohort(S, T, n).add_(100.0)
        conf = motion(S, T, q)
        keep = random_mask(S, T, args.censored)
        head, khead = ts[:2].cpu(), keep[:2].cpu()
        work = ts.clone()
        variants = {
            "interp_in_place": lambda: ingest.interpolate_censored(work, keep, out=work),
            "interp": lambda: ingest.interpolate_censored(ts, keep, out=work),
            "band_masked": lambda: ingest.filter_timeseries(ts, sample_mask=keep, interpolate=True, out=work, **band),
            "band_masked_conf": lambda: ingest.filter_timeseries(ts, sample_mask=keep, interpolate=True, confounds=conf,
                                                                 out=work, **band),
            "band": lambda: ingest.filter_timeseries(ts, out=work, **band),
            "copy": lambda: work.copy_(ts),
        }
        for fn in variants.values():                                      # warm-up of all
            fn()
        got = ingest.interpolate_censored(ts[:2].contiguous(), keep[:2].contiguous()).cpu()
        ratio = max(float(I.column_ratios(got[s], I.host_interpolate(head[s], khead[s]), head[s], khead[s]).max())
                    for s in range(2))
        del got
        work.copy_(ts)
        ms = {name: [] for name in variants}
        peak = {name: 0 for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                t, p, _ = timed(fn)
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        cohort_bytes = 4 * S * T * n
        kept = int(keep[0].sum()) / T
        moved = {"interp_in_place": cohort_bytes * (2 * kept + (1 - kept)), "interp": cohort_bytes * (3 * kept + (1 - kept)),
                 "copy": 2 * cohort_bytes}
        point = {"S": S, "T": T, "n": n, "q": q, "kept_frames": int(keep[0].sum()),
                 "components_kept": ingest.filter_components(T, **band)[1] - ingest.filter_components(T, **band)[0] + 1,
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_peak_bytes_above_inputs": p for name, p in peak.items()},
                 **{name + "_bytes_moved": int(b) for name, b in moved.items()},
                 **{name + "_bytes_per_s_at_median": b / (spread(ms[name])["median"] * 1e-3) for name, b in moved.items()},
                 "cohort_bytes": cohort_bytes, "mask_bytes": S * T,
                 "workspace_bytes": _lib.load().cgnn_ingest_interpolate_workspace_bytes(S, T, n),
                 "interp_err_over_bound_first_2_subjects": ratio}
        del work, conf, keep
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del ts
    print(json.dumps(out))


if __name__ == "__main__":
    main()
