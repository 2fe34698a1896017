#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest.kendall_matrices (csrc/kendall.hip) beside a plain copy of the same
cohort, the Spearman connectivity of the same run, the ranking that both start with, and a torch formulation of the
same counts on the same GPU.

    python tools/kendall_time.py [--points 4096x1200x360,8192x1200x84,4096x1200x360:300:100] [--rounds 5]
                                 [--torch-units 4] [--only a,b] [--skip-torch]

A point is S x T x n, or S x T x n : window : stride.  Per point, on one resident cohort of seeded time series
(tools/timeseries_time.py's):

  kendall         ingest.kendall_matrices(ts, window=, stride=): the ranking, the counts, the normalisation
  counts          ingest.kendall_counts(ts, window=, stride=)
  rank            ingest.rank_timeseries(ts, window=, stride=): the share of the call that is the ranking
  corr_rank       ingest.correlation_matrices(ts, rank=True, window=, stride=)
  copy            work.copy_(ts): the streaming floor
  torch           per unit: A = torch.sign(x[i0] - x[i1]) over triu_indices(L, 1) in bf16, A.mT @ A accumulated and
                  returned in fp32 (exact below 2^24), the same fp64 normalisation; timed on the first --torch-units
                  units, its counts checked equal to kendall_counts' there, and scaled to the cohort

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported.  The multiply-adds the definition needs are pairs x n (n + 1) / 2 per unit; the
int8 matrix peak they are set against is 2 x the 2.5e15 bf16 FLOP/s of the data sheet, 2.5e15 multiply-adds a second.
One JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import _lib, ingest  # noqa: E402
from tools.timeseries_time import cohort, spread, timed  # noqa: E402

INT8_PEAK_MACS = 2.5e15


def torch_counts(x, how):
    """fp32 [n, n]: G = A^T A of one unit x [L, n] on the device; ``how`` is "mm" (bf16 operands, fp32 result) or
    "bmm" (for a torch whose mm has no out_dtype on this backend: chunks of 256 pairs, whose sums a bf16 result holds
    exactly, added up in fp32)."""
    L, n = x.shape
    i = torch.triu_indices(L, L, 1, device=x.device)
    a = torch.sign(x[i[0]] - x[i[1]]).to(torch.bfloat16)
    if how == "mm":
        return torch.mm(a.mT, a, out_dtype=torch.float32)
    pad = -a.shape[0] % 256
    if pad:
        a = torch.cat([a, a.new_zeros(pad, n)])
    a = a.view(-1, 256, n)
    return torch.bmm(a.mT, a).sum(0, dtype=torch.float32)


def torch_tau(units, how):
    """fp32 [u, n, n]: tau-b of the units [u, L, n], one at a time; also the counts as int32."""
    taus, gs = [], []
    for x in units:
        g = torch_counts(x, how)
        d = torch.diagonal(g).double()
        t = g.double() / torch.sqrt(d[:, None] * d[None, :])
        t = torch.where((d[:, None] == 0) | (d[None, :] == 0), torch.zeros_like(t), t)
        taus.append(t.float())
        gs.append(g.to(torch.int32))
    return torch.stack(taus), torch.stack(gs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x1200x360,8192x1200x84,4096x1200x360:300:100")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-units", type=int, default=4, help="units the torch formulation is timed on")
    ap.add_argument("--only", default="", help="comma-separated variants to time (default: all)")
    ap.add_argument("--skip-torch", action="store_true", help="leave the torch formulation out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kendall_time.py measures on a ROCm GPU; none is visible")
    out = {"rounds": args.rounds, "torch_units": args.torch_units, "library": _lib.LIB_PATH,
           "int8_peak_multiply_adds_per_s": INT8_PEAK_MACS, "points": []}
    for spec in args.points.split(","):
        shape, _, win = spec.partition(":")
        S, T, n = (int(v) for v in shape.split("x"))
        window, stride = (int(v) for v in win.split(":")) if win else (None, None)
        kw = dict(window=window, stride=stride) if win else {}
        L = window or T
        W = (T - L) // (stride or T) + 1
        U = S * W
        torch.cuda.empty_cache()
        ts = cohort(S, T, n)
        work = torch.empty_like(ts)
        tu = min(args.torch_units, U)
        s_need = -(-tu // W)                                              # subjects that hold the first tu units
        head = ts[:s_need]
        units = (head.unfold(1, L, stride).permute(0, 1, 3, 2).reshape(-1, L, n) if win else head)[:tu].contiguous()
        how = "mm"
        if not args.skip_torch:
            try:
                torch_counts(units[0], "mm")
            except (NotImplementedError, RuntimeError, TypeError):
                how = "bmm"
        variants = {
            "kendall": lambda: ingest.kendall_matrices(ts, **kw),
            "counts": lambda: ingest.kendall_counts(ts, **kw),
            "rank": lambda: ingest.rank_timeseries(ts, **kw),
            "corr_rank": lambda: ingest.correlation_matrices(ts, rank=True, **kw),
            "copy": lambda: work.copy_(ts),
            "torch": lambda: torch_tau(units, how),
        }
        if args.skip_torch:
            del variants["torch"]
        if args.only:
            variants = {name: variants[name] for name in args.only.split(",")}
        same = close = None
        for name, fn in variants.items():                                 # warm-up of all
            got = fn()
            if name == "torch":
                same = bool(torch.equal(got[1], ingest.kendall_counts(head, **kw)[:tu]))
                close = float((got[0] - ingest.kendall_matrices(head, **kw)[:tu]).abs().max())
            del got
        ms = {name: [] for name in variants}
        peak = {name: 0 for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                t, p, _ = timed(fn)
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        med = {name: spread(v)["median"] for name, v in ms.items()}
        macs = U * (L * (L - 1) // 2) * (n * (n + 1) // 2)
        point = {"S": S, "T": T, "n": n, "window": window, "stride": stride, "units": U, "frames_per_unit": L,
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_peak_bytes_above_inputs": p for name, p in peak.items()},
                 "cohort_bytes": 4 * S * T * n, "multiply_adds_of_the_definition": macs,
                 "torch_formulation": how if "torch" in variants else None,
                 "torch_counts_equal_on_its_units": same, "torch_tau_max_abs_difference_on_its_units": close}
        if "torch" in med:
            point["torch_ms_scaled_to_the_cohort_at_median"] = med["torch"] * U / tu
        if "kendall" in med:
            point["kendall_share_of_int8_peak_at_median"] = macs / INT8_PEAK_MACS / (med["kendall"] * 1e-3)
            if "rank" in med:
                point["rank_share_of_kendall_at_median"] = med["rank"] / med["kendall"]
            if "torch" in med:
                point["torch_scaled_over_kendall_at_median"] = med["torch"] * U / tu / med["kendall"]
            for other in ("copy", "corr_rank"):
                if other in med:
                    point[f"kendall_over_{other}_at_median"] = med["kendall"] / med[other]
        if "counts" in med and "rank" in med:                             # the counts kernel alone, by difference
            point["counts_less_rank_share_of_int8_peak_at_median"] = \
                macs / INT8_PEAK_MACS / ((med["counts"] - med["rank"]) * 1e-3)
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del work, units, head, ts, variants
    print(json.dumps(out))


if __name__ == "__main__":
    main()
