#!/usr/bin/env python3
"""Time connectome_gnn_amd.ingest.node_measures (csrc/measures.hip) against the torch formulation it replaces.

    python tools/measures_time.py [--points 4096x360:0.1,4096x360:0.3,32768x84:0.1] [--rounds 3]

A point is S x n : keep.  Per point, on one resident cohort of seeded symmetric matrices and the thresholds
``select_thresholds`` gives for ``keep`` (selected once, outside the timed calls):

  new    ingest.node_measures(mats, min_weight=thr)  -- row pass, one product kernel per value map, finish
  torch  the plain-torch device formulation from the same thresholds: the mask, ``where``, the cube roots of the
         scaled weights, two ``torch.bmm(v.transpose(1, 2), v)``, a multiply and a row sum per value map, the
         quotients.  It runs without csrc/measures.hip; the largest difference between the two is reported.

Both variants are warmed up first; the two then alternate for --rounds rounds in this one process, each call between
two HIP events; min / median / max are reported, with torch.cuda.max_memory_allocated above the resident cohort for
each variant.  The new call's peak is ASSERTED to be its output plus cgnn_ingest_measures_workspace_bytes (512-byte
allocator rounding aside).  The first three subjects are also compared with the fp64 host statement
(tests/measures_data.py).  One JSON line.
Under `rocprofv3 --kernel-trace --stats -- python tools/measures_time.py --rounds 1 --skip-torch` the kernel
statistics hold k_measure_rows / k_measure_tri / k_measure_finish.
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
from tests import measures_data as M  # noqa: E402


def cohort(S, n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(S, n, n, device="cuda")
    step = max(1, (1 << 26) // (n * n))
    for lo in range(0, S, step):                       # in slices: no second cohort-sized temporary
        k = min(step, S - lo)
        r = torch.rand(k, n, n, device="cuda", generator=g)
        out[lo:lo + k] = torch.maximum(r, r.transpose(1, 2))
    return out


def torch_device(mats, thr):
    """[S, n, 5] by masks and bmm, all fp32."""
    S, n, _ = mats.shape
    off = ~torch.eye(n, dtype=torch.bool, device=mats.device)
    mask = (mats > thr[:, None, None]) & (mats > 0) & off
    a = torch.where(mask, mats, torch.zeros_like(mats))
    k = mask.sum(2).float()
    s = a.sum(2)
    wmax = a.amax((1, 2), keepdim=True)
    pairs = k * (k - 1)
    cols = [s / (s.amax(1, keepdim=True) + 1e-8), k / max(n - 1, 1), s / (k + 1e-8)]
    for v in (mask.float(), torch.where(mask, (a / wmax).pow(1.0 / 3.0), torch.zeros_like(a))):
        g = torch.bmm(v.transpose(1, 2), v)
        t = (g * v).sum(2)
        cols.append(torch.where(k >= 2, t / pairs.clamp_min(1.0), torch.zeros_like(t)))
    return torch.stack(cols, 2)


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
    ap.add_argument("--points", default="4096x360:0.1,4096x360:0.3,32768x84:0.1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true", help="time the new call alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measures_time.py measures on a ROCm GPU; none is visible")
    lib = _lib.load()
    ids = (ctypes.c_int32 * 5)(0, 1, 2, 3, 4)
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
        thr = ingest.select_thresholds(mats, keep=keep)
        new = lambda: ingest.node_measures(mats, min_weight=thr)                          # noqa: E731
        old = lambda: torch_device(mats, thr)                                             # noqa: E731
        got = new()                                                                       # warm-up of both
        head, head_thr = mats[:3].cpu(), thr[:3].cpu().tolist()
        want = M.cohort_measures(head, head_thr)
        rel64 = ((got[:3].cpu().double() - want).abs() / want.abs().clamp_min(1e-30)).amax((0, 1)).tolist()
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
        out_bytes = 4 * S * n * 5
        ws_bytes = int(lib.cgnn_ingest_measures_workspace_bytes(S, n, ids, 5))
        assert out_bytes + ws_bytes <= peak["new"] <= out_bytes + ws_bytes + 4096, (peak["new"], out_bytes, ws_bytes)
        # multiply-adds issued per value map: 36 blocks of 16 x 16 per off-diagonal tile pair, 21 per diagonal tile,
        # matrix rows padded to a multiple of 32
        nt = -(-n // 96)
        macs = 2 * S * (36 * (nt * (nt - 1) // 2) + 21 * nt) * 256 * (-(-n // 32) * 32)
        med = statistics.median(ms["new"])
        point = {"S": S, "n": n, "keep": keep, "new_ms": spread(ms["new"]),
                 "torch_ms": spread(ms["torch"]) if ms["torch"] else None,
                 "new_below_torch_min": med < min(ms["torch"]) if ms["torch"] else None,
                 "new_peak_bytes_above_input": peak["new"], "output_bytes": out_bytes, "workspace_bytes": ws_bytes,
                 "torch_peak_bytes_above_input": peak["torch"], "input_bytes": 4 * S * n * n,
                 "issued_macs_both_maps": macs, "issued_tflops": 2 * macs / med / 1e9,
                 "max_abs_diff_new_vs_torch": diff, "max_rel_err_vs_fp64_first_3_subjects_per_measure": rel64}
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
