#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest under a frame mask (``sample_mask=``): every masked launch beside the
unmasked call of the same run, and the torch formulation of the censored cleaning.

    python tools/censor_time.py [--points 4096x1200x360x24,8192x1200x84x24] [--t-r 0.72] [--high-pass 0.01]
                                [--censored 0.2] [--rounds 5]

A point is S x T x n x q.  Per point, on one resident cohort of seeded time series (tools/timeseries_time.py's, plus an
offset of 100), seeded motion-like confounds (tools/confound_time.py's) and a seeded mask that censors the same share of
every subject's frames at random (so that the torch formulation can batch its subjects):

  basis     ingest.confound_basis(confounds)                      | the same with sample_mask=
  regress   the means and k_filter<qpad> against a basis built beforehand (cgnn_ingest_regress | _masked)
  whole     ingest.regress_confounds(ts, confounds, out=work)     | the same with sample_mask=
  centre    ingest.filter_timeseries(ts, t_r=, out=work)          | the same with sample_mask=: masked centring
  corr      ingest.correlation_matrices(ts)                       | the same with sample_mask=
  lw        ingest.ledoit_wolf_shrinkage(ts)                      | the same with sample_mask=
  cleaned   ingest.filter_timeseries(ts, t_r=, high_pass=, confounds=, out=work): band, basis, regress
            | with sample_mask=: design, masked basis, masked regress -- another algorithm, both are reported
  torch     the yardstick for `cleaned` under the mask, plain torch in fp32: index-select the kept rows of the series and
            of [cosines | confounds], centre, torch.linalg.qr, xc - Q @ (Q.mT @ xc), scattered back into zeros

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, with torch.cuda.max_memory_allocated above the resident inputs for each, and the
largest error ratio of the masked `cleaned` against the fp64 host statement (tests/censor_data.py) on the first two
subjects.  One JSON line.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import ingest  # noqa: E402
from tests import censor_data as C  # noqa: E402
from tools.confound_time import motion  # noqa: E402
from tools.timeseries_time import cohort, spread, timed  # noqa: E402


def random_mask(S, T, share, seed=2):
    """bool [S, T] on the device: round(share T) frames of every subject censored, at random."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    order = torch.rand(S, T, device="cuda", generator=g).argsort(1)
    keep = torch.ones(S, T, dtype=torch.bool, device="cuda")
    keep.scatter_(1, order[:, :round(share * T)], False)
    return keep.contiguous()


def torch_device(ts, conf, keep, comps):
    """[S, T, n]: the censored cleaning by index-select + centre + batched QR + two batched matmuls, all fp32."""
    S, T, n = ts.shape
    idx = keep.nonzero()[:, 1].view(S, -1)                                # the same count for every subject
    t = torch.arange(T, device=ts.device, dtype=torch.float32)
    k = torch.tensor(comps, device=ts.device, dtype=torch.float32)
    cos = math.sqrt(2.0 / T) * torch.cos(math.pi * (2 * t[:, None] + 1) * k[None, :] / (2 * T))
    design = torch.cat([cos.expand(S, T, len(comps)), conf], 2)
    dk = design.gather(1, idx[:, :, None].expand(-1, -1, design.shape[2]))
    xk = ts.gather(1, idx[:, :, None].expand(-1, -1, n))
    Q = torch.linalg.qr(dk - dk.mean(1, keepdim=True)).Q
    xc = xk - xk.mean(1, keepdim=True)
    xc.sub_(torch.matmul(Q, torch.matmul(Q.mT, xc)))
    return torch.zeros_like(ts).scatter_(1, idx[:, :, None].expand(-1, -1, n), xc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x1200x360x24,8192x1200x84x24")
    ap.add_argument("--t-r", type=float, default=0.72)
    ap.add_argument("--high-pass", type=float, default=0.01)
    ap.add_argument("--censored", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="time the project's calls alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("censor_time.py measures on a ROCm GPU; none is visible")
    out = {"rounds": args.rounds, "t_r": args.t_r, "high_pass": args.high_pass, "censored": args.censored, "points": []}
    for spec in args.points.split(","):
        S, T, n, q = (int(v) for v in spec.split("x"))
        torch.cuda.empty_cache()
        ts = cohort(S, T, n).add_(100.0)
        conf = motion(S, T, q)
        keep = random_mask(S, T, args.censored)
        comps = list(range(1, ingest.filter_components(T, args.t_r, args.high_pass)[0]))
        head, chead, khead = ts[:2].cpu(), conf[:2].cpu(), keep[:2].cpu()
        band = dict(t_r=args.t_r, high_pass=args.high_pass)
        work = ts.clone()
        basis, _ = ingest.confound_basis(conf)
        mbasis, _ = ingest.confound_basis(conf, sample_mask=keep)
        pairs = {"basis": lambda m: ingest.confound_basis(conf, sample_mask=m),
                 "regress": lambda m: ingest._regress(ts, basis if m is None else mbasis, work, m),
                 "whole": lambda m: ingest.regress_confounds(ts, conf, sample_mask=m, out=work),
                 "centre": lambda m: ingest.filter_timeseries(ts, t_r=args.t_r, sample_mask=m, out=work),
                 "corr": lambda m: ingest.correlation_matrices(ts, sample_mask=m),
                 "lw": lambda m: ingest.ledoit_wolf_shrinkage(ts, sample_mask=m),
                 "cleaned": lambda m: ingest.filter_timeseries(ts, confounds=conf, sample_mask=m, out=work, **band)}
        variants = {}
        for name, fn in pairs.items():
            variants[name] = lambda fn=fn: fn(None)
            variants[name + "_masked"] = lambda fn=fn: fn(keep)
        if not args.skip_torch:
            variants["torch"] = lambda: torch_device(ts, conf, keep, comps)
        for fn in variants.values():                                      # warm-up of all
            fn()
        got = ingest.filter_timeseries(ts, confounds=conf, sample_mask=keep, **band)
        ratio = max(float(C.column_ratios(got[s].cpu(), head[s], C.host_design(chead[s], T, args.t_r, args.high_pass),
                                          khead[s]).max()) for s in range(2))
        diff = None
        if not args.skip_torch:
            ref = torch_device(ts, conf, keep, comps)
            scale = float(C.host_centred(head[0], khead[0]).abs().max())
            diff = float((got - ref).abs().max()) / (C.EPS * scale)
            del ref
        del got
        ms = {name: [] for name in variants}
        peak = {name: 0 for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                t, p, _ = timed(fn)
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        point = {"S": S, "T": T, "n": n, "q": q, "dropped_cosines": len(comps), "kept_frames": int(keep[0].sum()),
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_peak_bytes_above_inputs": p for name, p in peak.items()},
                 "cohort_bytes": 4 * S * T * n, "mask_bytes": S * T,
                 "design_bytes": 4 * S * T * (len(comps) + q),
                 "max_diff_cleaned_masked_vs_torch_over_eps_scale": diff,
                 "err_over_eps_scale_first_2_subjects": ratio, "tolerance_of_the_tests": 4 * 23.42}
        del work, basis, mbasis, conf, keep
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del ts
    print(json.dumps(out))


if __name__ == "__main__":
    main()
