#!/usr/bin/env python3
"""Time the weighted shortest-path node measures of connectome_gnn_amd.ingest (csrc/wpaths.hip) against a torch
formulation.

    python tools/wpaths_time.py [--points 4096x360:0.1,4096x360:0.3,32768x84:0.1] [--rounds 3]

A point is S x n : keep.  Per point, on one resident cohort of seeded symmetric matrices and the thresholds
``select_thresholds`` gives for ``keep`` (selected once, outside the timed calls):

  new    ingest.node_measures(mats, min_weight=thr, measures=WEIGHTED_PATH_MEASURES): one launch of k_wpaths
  torch  the obvious torch formulation on the same GPU from the same thresholds: the lengths ``wmax / A`` where kept,
         ``+inf`` elsewhere, a zero diagonal, then ``n`` steps of
         ``D = torch.minimum(D, D[:, :, k:k+1] + D[:, k:k+1, :])``, and the three row reductions in fp64 -- in chunks
         of --chunk subjects, so that its temporaries fit memory.  The largest relative difference between the two is
         reported.

Both variants are warmed up first; the two then alternate for --rounds rounds in this one process, each call between
two HIP events; min / median / max are reported, with torch.cuda.max_memory_allocated above the resident cohort for
each variant.  The new call's peak is ASSERTED to be its output plus cgnn_ingest_wpaths_workspace_bytes (512-byte
allocator rounding aside).  The first three subjects are also compared with the fp64 host statement
(tests/wpaths_data.py).  ``fraction_of_floor`` is the derived VALU floor -- ``S npad^3`` relaxations at 1.5 vector
instructions each (two adds and one min3 per two relaxations) against CUs x 4 SIMDs x 16 lanes x clock lane
instructions a second -- over the measured median.  One JSON line.
Under `rocprofv3 --kernel-trace --stats -- python tools/wpaths_time.py --rounds 1 --skip-torch` the kernel statistics
hold k_wpaths (one launch per point and round, and one for the warm-up).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import _lib, ingest  # noqa: E402
from tests import wpaths_data as W  # noqa: E402
from tools.measures_time import cohort, spread, timed  # noqa: E402

NAMES = ingest.WEIGHTED_PATH_MEASURES


def torch_device(mats, thr, chunk):
    """[S, n, 3] by n Floyd-Warshall steps on whole chunks of subjects."""
    S, n, _ = mats.shape
    eye = torch.eye(n, dtype=torch.bool, device=mats.device)
    inf = torch.tensor(float("inf"), device=mats.device)
    out = torch.empty(S, n, 3, device=mats.device)
    nm1 = max(n - 1, 1)
    for lo in range(0, S, chunk):
        A = mats[lo:lo + chunk]
        mask = (A > thr[lo:lo + chunk, None, None]) & (A > 0) & ~eye
        wmax = torch.where(mask, A, torch.zeros_like(A)).amax((1, 2), keepdim=True)
        D = torch.where(mask, wmax / A, inf)
        D.diagonal(dim1=1, dim2=2).zero_()
        for k in range(n):
            D = torch.minimum(D, D[:, :, k:k + 1] + D[:, k:k + 1, :])
        reached = torch.isfinite(D) & ~eye
        Dd = D.double()
        r = reached.sum(2).double()
        inv = torch.where(reached, 1.0 / Dd, torch.zeros_like(Dd)).sum(2)
        total = torch.where(reached, Dd, torch.zeros_like(Dd)).sum(2)
        far = torch.where(reached, Dd, torch.zeros_like(Dd)).amax(2)
        close = torch.where(r > 0, (r / nm1) * (r / total.clamp_min(1e-300)), torch.zeros_like(r))
        out[lo:lo + chunk] = torch.stack([inv / nm1, close, far / nm1], 2).float()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x360:0.1,4096x360:0.3,32768x84:0.1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=0, help="subjects per torch chunk (0: ~1 GB of distances)")
    ap.add_argument("--skip-torch", action="store_true", help="time the new call alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wpaths_time.py measures on a ROCm GPU; none is visible")
    lib = _lib.load()
    props = torch.cuda.get_device_properties(0)
    lane_rate = props.multi_processor_count * 4 * 16 * getattr(props, "clock_rate", 2400000) * 1e3   # lane instructions/s
    out = {"rounds": args.rounds, "points": []}
    held = (None, None)
    for spec in args.points.split(","):
        shape, keep = spec.split(":")
        S, n = (int(v) for v in shape.split("x"))
        keep = float(keep)
        if held[0] != (S, n):
            held = (None, None)
            torch.cuda.empty_cache()
            held = ((S, n), cohort(S, n))
        mats = held[1]
        chunk = args.chunk or max(1, (1 << 28) // (n * n))
        thr = ingest.select_thresholds(mats, keep=keep)
        new = lambda: ingest.node_measures(mats, min_weight=thr, measures=NAMES)          # noqa: E731
        old = lambda: torch_device(mats, thr, chunk)                                      # noqa: E731
        got = new()                                                                       # warm-up of both
        head, head_thr = mats[:3].cpu(), thr[:3].cpu().tolist()
        want = torch.stack([W.host_statement(A, t)[1] for A, t in zip(head, head_thr)])
        rel64 = ((got[:3].cpu().double() - want).abs() / want.abs().clamp_min(1e-30)).amax((0, 1)).tolist()
        diff = None
        if not args.skip_torch:
            ref = old()
            diff = float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max())
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
        ids = (ctypes.c_int32 * 3)(0, 1, 2)
        out_bytes = 4 * S * n * 3
        ws_bytes = int(lib.cgnn_ingest_wpaths_workspace_bytes(S, n, ids, 3))
        assert out_bytes + ws_bytes <= peak["new"] <= out_bytes + ws_bytes + 4096, (peak["new"], out_bytes, ws_bytes)
        block = 32 if -(-n // 32) * 32 <= 512 else 16
        npad = -(-n // block) * block
        floor_ms = S * npad ** 3 * 1.5 / lane_rate * 1e3
        med = statistics.median(ms["new"])
        point = {"S": S, "n": n, "keep": keep, "new_ms": spread(ms["new"]),
                 "torch_ms": spread(ms["torch"]) if ms["torch"] else None,
                 "new_below_torch_min": med < min(ms["torch"]) if ms["torch"] else None,
                 "new_peak_bytes_above_input": peak["new"], "output_bytes": out_bytes, "workspace_bytes": ws_bytes,
                 "torch_peak_bytes_above_input": peak["torch"], "torch_chunk": chunk, "input_bytes": 4 * S * n * n,
                 "npad": npad, "relaxations": S * npad ** 3, "valu_floor_ms": floor_ms, "fraction_of_floor": floor_ms / med,
                 "max_rel_diff_new_vs_torch": diff, "max_rel_err_vs_fp64_first_3_subjects_per_measure": rel64}
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
