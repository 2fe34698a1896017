#!/usr/bin/env python3
"""Time the Butterworth band-pass of connectome_gnn_amd.ingest.filter_timeseries (filter="butterworth",
csrc/butterworth.hip) beside the cosine band-pass of the same band and a plain copy of the same run.

    python tools/butter_time.py [--points 4096x1200x360x24,8192x1200x84x24] [--t-r 0.72] [--high-pass 0.01]
                                [--low-pass 0.1] [--order 5] [--censored 0.2] [--rounds 5]

A point is S x T x n x q.  Per point, on one resident cohort of seeded time series (tools/timeseries_time.py's, plus an
offset of 100), seeded motion-like confounds (tools/confound_time.py's) and a seeded mask that censors the same share of
every subject's frames at random (tools/censor_time.py's):

  butter_in_place    ingest.filter_timeseries(work, band, filter="butterworth", out=work)
  butter             ingest.filter_timeseries(ts, band, filter="butterworth", out=work)
  butter_conf        the same with confounds=: the confounds filtered alike, their basis, the regression
  butter_masked      the same with sample_mask=, interpolate=True: interpolate, the Butterworth pass, masked centring
  butter_masked_conf ... and confounds=: the confounds interpolated and filtered too, the regression on the kept frames
  cosine             ingest.filter_timeseries(ts, band, out=work): the DCT projection of the same band
  cosine_conf        the same with confounds=
  cosine_masked      the same with sample_mask=, interpolate=True
  copy               work.copy_(ts): the streaming floor

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, with torch.cuda.max_memory_allocated above the resident inputs for each, the
bytes the Butterworth pass must move (two reads of the series and one write; the boundary states, 2 L fp64 per column
out and in again every 48 frames, are counted apart) and the rate that makes at the median, its fp64 multiply-adds (15 per
section and frame of the padded run: forward, forward again, backward), and the largest ratio of the Butterworth call
against the fp64 host statement (tests/butter_data.py: scipy's sosfiltfilt) on the first two subjects.  One JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import _lib, ingest  # noqa: E402
from tests import butter_data as B  # noqa: E402
from tools.censor_time import random_mask  # noqa: E402
from tools.confound_time import motion  # noqa: E402
from tools.timeseries_time import cohort, spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x1200x360x24,8192x1200x84x24")
    ap.add_argument("--t-r", type=float, default=0.72)
    ap.add_argument("--high-pass", type=float, default=0.01)
    ap.add_argument("--low-pass", type=float, default=0.1)
    ap.add_argument("--order", type=int, default=5)
    ap.add_argument("--censored", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated variants to time (default: all)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("butter_time.py measures on a ROCm GPU; none is visible")
    band = dict(t_r=args.t_r, high_pass=args.high_pass, low_pass=args.low_pass)
    butter = dict(filter="butterworth", order=args.order, **band)
    sos = ingest.butterworth_sos(args.t_r, args.high_pass, args.low_pass, args.order)
    L, edge = len(sos), B.edge_of(sos)
    out = {"rounds": args.rounds, **band, "order": args.order, "sections": L, "edge": edge, "censored": args.censored,
           "library": _lib.LIB_PATH, "points": []}
    for spec in args.points.split(","):
        S, T, n, q = (int(v) for v in spec.split("x"))
        torch.cuda.empty_cache()
        ts = cohort(S, T, n).add_(100.0)
        conf = motion(S, T, q)
        keep = random_mask(S, T, args.censored)
        head = ts[:2].cpu()
        work = ts.clone()
        variants = {
            "butter_in_place": lambda: ingest.filter_timeseries(work, out=work, **butter),
            "butter": lambda: ingest.filter_timeseries(ts, out=work, **butter),
            "butter_conf": lambda: ingest.filter_timeseries(ts, confounds=conf, out=work, **butter),
            "butter_masked": lambda: ingest.filter_timeseries(ts, sample_mask=keep, interpolate=True, out=work, **butter),
            "butter_masked_conf": lambda: ingest.filter_timeseries(ts, sample_mask=keep, interpolate=True, confounds=conf,
                                                                   out=work, **butter),
            "cosine": lambda: ingest.filter_timeseries(ts, out=work, **band),
            "cosine_conf": lambda: ingest.filter_timeseries(ts, confounds=conf, out=work, **band),
            "cosine_masked": lambda: ingest.filter_timeseries(ts, sample_mask=keep, interpolate=True, out=work, **band),
            "copy": lambda: work.copy_(ts),
        }
        if args.only:
            variants = {name: variants[name] for name in args.only.split(",")}
        for fn in variants.values():                                      # warm-up of all
            fn()
        got = ingest.filter_timeseries(ts[:2].contiguous(), **butter).cpu()
        want = B.host(head, args.t_r, args.high_pass, args.low_pass, args.order)
        ratio = max(float(B.column_ratios(got[s], want[s], head[s]).max()) for s in range(2))
        del got, want
        work.copy_(ts)
        ms = {name: [] for name in variants}
        peak = {name: 0 for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                if name == "butter_in_place":
                    work.copy_(ts)                                        # (filtering a filtered run decays to zeros)
                t, p, _ = timed(fn)
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        cohort_bytes = 4 * S * T * n
        panels = (n + 63) // 64
        state_bytes = 2 * S * panels * 64 * len(B.segments(T, edge)) * 2 * L * 8
        moved = {"butter_in_place": 3 * cohort_bytes, "butter": 3 * cohort_bytes, "copy": 2 * cohort_bytes}
        moved = {name: b for name, b in moved.items() if name in variants}
        fma = 15 * L * S * panels * 64 * (T + 2 * edge)
        point = {"S": S, "T": T, "n": n, "q": q, "kept_frames": int(keep[0].sum()),
                 "cosine_components_kept": ingest.filter_components(T, **band)[1] - ingest.filter_components(T, **band)[0] + 1,
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_peak_bytes_above_inputs": p for name, p in peak.items()},
                 **{name + "_bytes_moved": int(b) for name, b in moved.items()},
                 **{name + "_bytes_per_s_at_median": b / (spread(ms[name])["median"] * 1e-3) for name, b in moved.items()},
                 "cohort_bytes": cohort_bytes, "butter_state_bytes": state_bytes, "butter_fp64_fma": fma,
                 "workspace_bytes": _lib.load().cgnn_ingest_butterworth_workspace_bytes(S, T, n, L),
                 "butter_err_over_bound_first_2_subjects": ratio}
        if "butter" in ms:
            point["butter_fp64_fma_per_s_at_median"] = fma / (spread(ms["butter"])["median"] * 1e-3)
        del work, conf, keep
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del ts
    print(json.dumps(out))


if __name__ == "__main__":
    main()
