#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest.correlation_matrices (csrc/timeseries.hip) against what it replaces.

    python tools/timeseries_time.py [--points 4096x1200x360,8192x1200x84,4096x1200x360:300:100] [--rounds 3]

A point is S x T x n, optionally :window:stride.  Per point, on one resident cohort of seeded time series (four
shared latent signals plus noise, per-ROI scales and offsets):

  new    ingest.correlation_matrices(ts, window=, stride=)  -- statistics pass + product kernel
  torch  the plain-torch device formulation without fp64: (unfold the windows,) centre, scale by 1/sqrt of the
         centred sum of squares, torch.bmm in fp32, clamp, set the diagonal.  It runs without csrc/timeseries.hip;
         the largest difference between the two results is reported.

Both variants are warmed up first; the two then alternate for --rounds rounds in this one process, each call
between two HIP events; min / median / max are reported, with torch.cuda.max_memory_allocated above the resident
cohort for each variant, the traffic model of DESIGN.md 4.3c, and the largest error of `new` against the fp64 host
statement (tests/timeseries_data.py) on the first three subjects.  One JSON line.
Under `rocprofv3 --kernel-trace --stats -- python tools/timeseries_time.py --rounds 1` the kernel statistics hold
k_corr_stats / k_corr next to the torch kernels of the bmm formulation.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import ingest  # noqa: E402
from tests import timeseries_data as D  # noqa: E402


def cohort(S, T, n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(S, T, n, device="cuda")
    mix = 0.6 * torch.randn(4, n, device="cuda", generator=g)
    scale = 0.5 + 3.0 * torch.rand(n, device="cuda", generator=g)
    shift = torch.randn(n, device="cuda", generator=g)
    step = max(1, (1 << 26) // (T * n))
    for lo in range(0, S, step):                       # in slices: no second cohort-sized temporary
        k = min(step, S - lo)
        lat = torch.randn(k, T, 4, device="cuda", generator=g)
        out[lo:lo + k] = (lat @ mix + torch.randn(k, T, n, device="cuda", generator=g) + shift) * scale
    return out


def torch_device(ts, window, stride):
    """[U, n, n] by standardise + bmm, all fp32."""
    S, T, n = ts.shape
    x = ts
    if window is not None:
        x = ts.unfold(1, window, stride).permute(0, 1, 3, 2).reshape(-1, window, n)     # the unfolded copy
    d = x - x.mean(1, keepdim=True)
    q = (d * d).sum(1, keepdim=True)
    rs = torch.where(q > 0, torch.rsqrt(q), torch.zeros_like(q))
    z = d * rs
    del d
    r = torch.bmm(z.transpose(1, 2), z).clamp_(-1.0, 1.0)
    r.diagonal(dim1=1, dim2=2).copy_((q.squeeze(1) > 0).float())
    return r


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x1200x360,8192x1200x84,4096x1200x360:300:100")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true", help="time the new call alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("timeseries_time.py measures on a ROCm GPU; none is visible")
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
        W = D.num_windows(T, window, stride)
        U, L = S * W, window or T
        new = lambda: ingest.correlation_matrices(ts, window=window, stride=stride)      # noqa: E731
        old = lambda: torch_device(ts, window, stride)                                   # noqa: E731
        got = new()                                                                       # warm-up of both
        head = ts[:3].cpu()
        err64 = float((got[:3 * W].cpu().double() - D.host_corr(head, window, stride)).abs().max())
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
        # traffic model: the statistics pass reads every unit's frames once (its second sweep is
        # meant to hit cache), the product reads them once more, the output is written once
        nt = -(-n // 96)
        model = 2 * 4 * U * L * n + 4 * U * n * n + 2 * 8 * U * n
        # multiply-adds issued: 36 blocks of 16 x 16 per off-diagonal tile pair, 21 per diagonal tile, frames
        # padded to a multiple of 32
        macs = U * (36 * (nt * (nt - 1) // 2) + 21 * nt) * 256 * (-(-L // 32) * 32)
        med = statistics.median(ms["new"])
        point = {"S": S, "T": T, "n": n, "window": window, "stride": stride, "units": U,
                 "new_ms": spread(ms["new"]), "torch_ms": spread(ms["torch"]) if ms["torch"] else None,
                 "new_peak_bytes_above_input": peak["new"], "torch_peak_bytes_above_input": peak["torch"],
                 "input_bytes": 4 * S * T * n, "output_bytes": 4 * U * n * n, "model_bytes": model,
                 "model_gb_per_s": model / med / 1e6, "useful_macs": U * n * n * L // 2, "issued_macs": macs,
                 "issued_tflops": 2 * macs / med / 1e9, "max_abs_diff_new_vs_torch": diff,
                 "max_abs_err_vs_fp64_first_3_subjects": err64,
                 "atol_of_the_tests": D.atol(L, D.kappa(head, window, stride))}
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
