#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest.series_features (csrc/activity.hip) beside a plain copy of the same
cohort and the torch formulation of the same features on the same GPU.

    python tools/activity_time.py [--points 4096x1200x360,8192x1200x84] [--t-r 0.72] [--lo 0.01] [--hi 0.08] [--rounds 5]

A point is S x T x n.  Per point, on one resident cohort of seeded time series (tools/timeseries_time.py's, plus an offset
of 100), for each of three requests -- ("std", "autocorr1"), all but "falff", all six:

  call     ingest.series_features(ts, t_r=, band=, features=request)
  torch    centre, torch.fft.rfft over the frames, abs, the sums and ratios, all fp32 / complex64
  copy     work.copy_(ts): one read and one write of the cohort, the streaming floor (once per point)

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, with torch.cuda.max_memory_allocated above the resident input for each, the
bytes the call reads (the moments pass reads the cohort twice, every chunk of 128 bins of a spectrum launch once more),
the fp32 multiply-adds of its products as flops with the rate at the median against the 155 TFLOP/s of the fp32 matrix
pipe -- counted twice: what the kernel issues (2 T x the table columns of every chunk, per column of a 64-column item,
padding included) and what the statement needs (2 T x 2 bins per real column: the band's bins, and K more with falff) --
and the largest error of the call against the fp64 host statement (tests/activity_data.py) on the first two subjects in
units of the GPU tests' bound.  One JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import _lib, ingest  # noqa: E402
from tests import activity_data as A  # noqa: E402
from tests.test_activity_math import HOST32_RATIO  # noqa: E402
from tools.timeseries_time import cohort, spread, timed  # noqa: E402

REQUESTS = {"moments": ("std", "autocorr1"),
            "band": ("std", "autocorr1", "alff", "band_std", "band_fraction"),
            "all": ingest.SERIES_FEATURES}
PEAK_FP32_MATRIX = 155e12


def torch_features(ts, names, k_lo, k_hi):
    """[S, n, F] fp32 by the FFT route; the temporaries are cohort-sized."""
    S, T, n = ts.shape
    xc = ts - ts.mean(1, keepdim=True)
    q = (xc * xc).sum(1)
    cols = {}
    if "std" in names or "band_fraction" in names:
        cols["std"] = (q / (T - 1)).sqrt()
    if "autocorr1" in names:
        cols["autocorr1"] = (xc[:, :-1] * xc[:, 1:]).sum(1) / q
    if set(names) & set(A.SPECTRAL):
        amp = torch.fft.rfft(xc, dim=1)[:, 1:T // 2 + 1].abs()            # [S, K, n]
        del xc
        band = amp[:, k_lo - 1:k_hi]
        if "alff" in names:
            cols["alff"] = 2.0 * band.sum(1) / T / (k_hi - k_lo + 1)
        if "falff" in names:
            cols["falff"] = band.sum(1) / amp.sum(1)
        if "band_std" in names or "band_fraction" in names:
            w = torch.full((k_hi - k_lo + 1, 1), 2.0, device=ts.device)
            if T % 2 == 0 and k_hi == T // 2:
                w[-1] = 1.0
            cols["band_std"] = ((w * band * band).sum(1) / T / (T - 1)).sqrt()
        if "band_fraction" in names:
            cols["band_fraction"] = cols["band_std"] / cols["std"]
    return torch.stack([cols[name] for name in names], dim=2)


def products(T, n, S, k_lo, k_hi, names):
    """(chunk passes over the frames, flops the products issue, flops the statement needs) of a request, as the entry
    point lays its launches out."""
    if not set(names) & set(A.SPECTRAL):
        return 0, 0, 0

    def launch(bins):
        cols = 2 * bins
        pad = -(-cols // 64) * 64 if cols <= 256 else 256
        return -(-cols // pad), pad

    k_first = (k_lo - 1) | 1
    chunks, pad = launch(k_hi - k_first + 1)
    passes, columns = chunks, chunks * pad
    if "falff" in names:
        chunks, pad = launch(T // 2)
        passes, columns = passes + chunks, columns + chunks * pad
    bins = k_hi - k_lo + 1 + (T // 2 if "falff" in names else 0)
    return passes, 2 * T * columns * 64 * S * (-(-n // 64)), 2 * T * 2 * bins * S * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x1200x360,8192x1200x84")
    ap.add_argument("--t-r", type=float, default=0.72)
    ap.add_argument("--lo", type=float, default=0.01)
    ap.add_argument("--hi", type=float, default=0.08)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="time the call and the copy alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("activity_time.py measures on a ROCm GPU; none is visible")
    band = (args.lo, args.hi)
    out = {"rounds": args.rounds, "t_r": args.t_r, "band": band, "library": _lib.LIB_PATH, "points": []}
    for spec in args.points.split(","):
        S, T, n = (int(v) for v in spec.split("x"))
        torch.cuda.empty_cache()
        ts = cohort(S, T, n).add_(100.0)
        k_lo, k_hi = ingest.series_band(T, args.t_r, band)
        head = ts[:2].cpu()
        work = torch.empty_like(ts)
        variants = {"copy": lambda: work.copy_(ts)}
        for key, names in REQUESTS.items():
            variants[key] = lambda names=names: ingest.series_features(ts, t_r=args.t_r, band=band, features=names)
            if not args.skip_torch:
                variants[key + "_torch"] = lambda names=names: torch_features(ts, names, k_lo, k_hi)
        for fn in variants.values():                                      # warm-up of all
            fn()
        got = ingest.series_features(ts[:2].contiguous(), t_r=args.t_r, band=band).cpu()
        want = A.host_features(head, args.t_r, band)
        ratio = {}
        for j, name in enumerate(A.NAMES):
            if name in A.SPECTRAL:
                bound = 4 * HOST32_RATIO[name] * A.scale_of(name, head)
            else:
                bound = 2.0 ** -24 * want[:, :, j].abs() + 2.0 ** -40 * (A.amplitude(head) if name == "std" else 1.0)
            ratio[name] = float(A.ratios(got[:, :, j], want[:, :, j], bound).max())
        if not args.skip_torch:
            fft = torch_features(ts[:2].contiguous(), A.NAMES, k_lo, k_hi).cpu()
            ratio["torch_over_the_same_bounds"] = {
                name: float(A.ratios(fft[:, :, j], want[:, :, j],
                                     4 * HOST32_RATIO[name] * A.scale_of(name, head)).max())
                for j, name in enumerate(A.NAMES) if name in A.SPECTRAL}
            del fft
        del got, want
        ms = {name: [] for name in variants}
        peak = {name: 0 for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                t, p, res = timed(fn)
                del res
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        cohort_bytes = 4 * S * T * n
        point = {"S": S, "T": T, "n": n, "k_lo": k_lo, "k_hi": k_hi, "cohort_bytes": cohort_bytes,
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_peak_bytes_above_input": p for name, p in peak.items()},
                 "err_over_bound_first_2_subjects": ratio}
        for key, names in REQUESTS.items():
            passes, flops, useful = products(T, n, S, k_lo, k_hi, names)
            median = spread(ms[key])["median"] * 1e-3
            bins = 0 if not passes else T // 2 if "falff" in names else k_hi - ((k_lo - 1) | 1) + 1
            point[key + "_passes_over_the_cohort"] = 2 + passes
            point[key + "_bytes_read"] = (2 + passes) * cohort_bytes
            point[key + "_bytes_read_per_s_at_median"] = (2 + passes) * cohort_bytes / median
            point[key + "_over_copy"] = spread(ms[key])["median"] / spread(ms["copy"])["median"]
            point[key + "_workspace_bytes"] = _lib.load().cgnn_ingest_activity_workspace_bytes(S, T, n, bins)
            if flops:
                point[key + "_product_flops"] = flops
                point[key + "_flops_per_s_at_median"] = flops / median
                point[key + "_fraction_of_fp32_matrix_peak"] = flops / median / PEAK_FP32_MATRIX
                point[key + "_useful_flops"] = useful
                point[key + "_useful_fraction_of_fp32_matrix_peak"] = useful / median / PEAK_FP32_MATRIX
        del work
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del ts
    print(json.dumps(out))


if __name__ == "__main__":
    main()
