#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest's confound regression (csrc/confounds.hip, csrc/filter.hip) against the torch
formulation it replaces and against the band-pass launch whose kernel it shares.

    python tools/confound_time.py [--points 4096x1200x360x24,8192x1200x84x24] [--t-r 0.72] [--high-pass 0.01] [--rounds 5]

A point is S x T x n x q.  Per point, on one resident cohort of seeded time series (tools/timeseries_time.py's, plus an
offset of 100) and seeded motion-like confounds (q / 4 random walks with offsets, their differences, the squares of
both):

  basis     ingest.confound_basis(confounds): the one launch of k_confound_basis
  regress   the means and k_filter<qpad> in complement form against a basis built beforehand (cgnn_ingest_regress)
  whole     ingest.regress_confounds(ts, confounds, out=work): basis + regress, in place on a copy
  filter    the yardstick: ingest.filter_timeseries(ts, t_r=, high_pass=) alone, in place on a copy -- the same kernel in
            complement form against the one table of the cohort
  cleaned   ingest.filter_timeseries(ts, t_r=, high_pass=, confounds=, out=work): the band on both, basis, regress
  torch     the plain-torch device formulation in fp32: Q = torch.linalg.qr of the centred confounds, xc - Q @ (Q.mT @ xc)

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, with torch.cuda.max_memory_allocated above the resident inputs for each, the
bytes the regress launch must move (the means' read, the coefficients' read, the second read, one write, and the
per-subject tables twice) against the filter's, and the largest error ratio of `whole` against the fp64 host statement
(tests/confound_data.py) on the first two subjects.  One JSON line.
Under `rocprofv3 --kernel-trace --stats -- python tools/confound_time.py --rounds 1 --skip-torch` the kernel statistics
hold k_confound_basis / k_filter_mean / k_filter.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import ingest  # noqa: E402
from tests import confound_data as D  # noqa: E402
from tools.timeseries_time import cohort, spread, timed  # noqa: E402


def motion(S, T, q, seed=1):
    """[S, T, q] fp32 on the device: q / 4 random walks with offsets, their differences, the squares of both (and
    white noise in what is left of q)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    m = max(q // 4, 1)
    walk = (0.05 * torch.randn(S, T, m, device="cuda", generator=g)).cumsum(1)
    walk += torch.rand(S, 1, m, device="cuda", generator=g) - 0.5
    diff = torch.zeros_like(walk)
    diff[:, 1:] = walk[:, 1:] - walk[:, :-1]
    rest = torch.randn(S, T, max(q - 4 * m, 0), device="cuda", generator=g)
    return torch.cat([walk, diff, walk ** 2, diff ** 2, rest], 2)[:, :, :q].contiguous()


def torch_device(ts, conf):
    """[S, T, n] by centre + batched QR + two batched matmuls, all fp32."""
    cc = conf - conf.mean(1, keepdim=True)
    Q = torch.linalg.qr(cc).Q
    xc = ts - ts.mean(1, keepdim=True)
    return xc.sub_(torch.matmul(Q, torch.matmul(Q.mT, xc)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x1200x360x24,8192x1200x84x24")
    ap.add_argument("--t-r", type=float, default=0.72)
    ap.add_argument("--high-pass", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="time the new calls alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("confound_time.py measures on a ROCm GPU; none is visible")
    out = {"rounds": args.rounds, "t_r": args.t_r, "high_pass": args.high_pass, "points": []}
    for spec in args.points.split(","):
        S, T, n, q = (int(v) for v in spec.split("x"))
        torch.cuda.empty_cache()
        ts = cohort(S, T, n).add_(100.0)
        conf = motion(S, T, q)
        head, chead = ts[:2].cpu(), conf[:2].cpu()
        kw = dict(t_r=args.t_r, high_pass=args.high_pass)
        work = ts.clone()
        basis, rank = ingest.confound_basis(conf)
        qpad = int(basis.shape[2])
        variants = {"basis": lambda: ingest.confound_basis(conf),
                    "regress": lambda: ingest._regress(ts, basis, work),
                    "whole": lambda: ingest.regress_confounds(ts, conf, out=work),
                    "filter": lambda: ingest.filter_timeseries(ts, out=work, **kw),
                    "cleaned": lambda: ingest.filter_timeseries(ts, confounds=conf, out=work, **kw)}
        if not args.skip_torch:
            variants["torch"] = lambda: torch_device(ts, conf)
        for fn in variants.values():                                      # warm-up of all
            fn()
        got = ingest.regress_confounds(ts, conf)
        ratio = max(float(D.column_ratios(got[s].cpu(), head[s], chead[s]).max()) for s in range(2))
        diff = None
        if not args.skip_torch:
            ref = torch_device(ts, conf)
            scale = float((head[0].double() - head[0].double().mean(0)).abs().max())
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
        cohort_bytes, table_bytes = 4 * S * T * n, 4 * S * T * qpad
        chunks = -(-n // 64)
        point = {"S": S, "T": T, "n": n, "q": q, "qpad": qpad, "rank_min": int(rank.min()), "rank_max": int(rank.max()),
                 "filter_components": ingest.filter_components(T, args.t_r, args.high_pass)[0] - 1,
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_peak_bytes_above_inputs": p for name, p in peak.items()},
                 "cohort_bytes": cohort_bytes, "confound_bytes": 4 * S * T * q, "basis_bytes": table_bytes,
                 "filter_model_bytes": 4 * cohort_bytes,
                 "regress_model_bytes": 4 * cohort_bytes + 2 * table_bytes,
                 "regress_table_bytes_read_by_every_item": 2 * table_bytes * chunks,
                 "regress_model_gb_per_s": (4 * cohort_bytes + 2 * table_bytes) / statistics.median(ms["regress"]) / 1e6,
                 "filter_model_gb_per_s": 4 * cohort_bytes / statistics.median(ms["filter"]) / 1e6,
                 "basis_fp64_fmas": 4 * S * T * q * q,
                 "max_diff_whole_vs_torch_over_eps_scale": diff, "err_over_eps_scale_first_2_subjects": ratio,
                 "tolerance_of_the_tests": 4 * 11.09}
        del work, basis, conf
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del ts
    print(json.dumps(out))


if __name__ == "__main__":
    main()
