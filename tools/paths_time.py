#!/usr/bin/env python3
"""Time the shortest-path node measures of connectome_gnn_amd.ingest (csrc/paths.hip) against a torch formulation.

    python tools/paths_time.py [--points 4096x360:0.1,4096x360:0.3,32768x84:0.1] [--rounds 3]

A point is S x n : keep.  Per point, on one resident cohort of seeded symmetric matrices and the thresholds
``select_thresholds`` gives for ``keep`` (selected once, outside the timed calls):

  global  ingest.node_measures(mats, min_weight=thr, measures=(nodal_efficiency, closeness, eccentricity))
  all     the same call with local_efficiency as the fourth column (the BFS per neighbour pair on top)
  torch   the plain-torch device formulation of the three global measures from the same thresholds: the mask as a
          half matrix, then per BFS level one ``torch.bmm(frontier, adjacency)`` for all sources of all subjects at
          once, ``> 0``, ``& ~visited``, a row sum for the level's counts, and one host read of "any node reached" to
          stop.  (Local efficiency has no such form: one such BFS per node, n times the work and a cohort-sized mask
          per node; it is timed for the new call only.)  The largest difference between the two is reported.

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two
HIP events; min / median / max are reported, with torch.cuda.max_memory_allocated above the resident cohort for each
variant.  The new call's peak is ASSERTED to be its output plus cgnn_ingest_paths_workspace_bytes (512-byte allocator
rounding aside).  The first three subjects are also compared with the fp64 host statement (tests/paths_data.py).
One JSON line.
Under `rocprofv3 --kernel-trace --stats -- python tools/paths_time.py --rounds 1 --skip-torch` the kernel statistics
hold k_paths (two launches per point and round: global, all).
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
from tests import paths_data as P  # noqa: E402
from tools.measures_time import cohort, spread, timed  # noqa: E402

GLOBAL = ingest.PATH_MEASURES[:3]


def torch_device(mats, thr):
    """[S, n, 3] (nodal_efficiency, closeness, eccentricity) by boolean frontier matrices and bmm."""
    S, n, _ = mats.shape
    eye = torch.eye(n, dtype=torch.bool, device=mats.device)
    adj = ((mats > thr[:, None, None]) & (mats > 0) & ~eye).half()
    visited = eye.expand(S, n, n).clone()
    frontier = visited.half()
    r = torch.zeros(S, n, device=mats.device)
    sum_d, ecc = torch.zeros_like(r), torch.zeros_like(r)
    eff = torch.zeros(S, n, dtype=torch.float64, device=mats.device)
    level = 0
    while True:
        level += 1
        nxt = (torch.bmm(frontier, adj) > 0) & ~visited       # row i: the nodes first reached from i at this level
        cnt = nxt.sum(2)
        if not bool(cnt.any()):
            break
        visited |= nxt
        frontier = nxt.half()
        r += cnt
        sum_d += level * cnt
        ecc = torch.where(cnt > 0, torch.full_like(ecc, level), ecc)
        eff += cnt.double() / level
    nm1 = max(n - 1, 1)
    close = torch.where(r > 0, (r.double() / nm1) * (r.double() / sum_d.double().clamp_min(1.0)),
                        torch.zeros_like(eff))
    return torch.stack([(eff / nm1).float(), close.float(), ecc / nm1], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x360:0.1,4096x360:0.3,32768x84:0.1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true", help="time the new calls alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("paths_time.py measures on a ROCm GPU; none is visible")
    lib = _lib.load()
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
        variants = {"global": lambda: ingest.node_measures(mats, min_weight=thr, measures=GLOBAL),
                    "all": lambda: ingest.node_measures(mats, min_weight=thr, measures=ingest.PATH_MEASURES),
                    "torch": lambda: torch_device(mats, thr)}
        if args.skip_torch:
            del variants["torch"]
        got = variants["all"]()                                                           # warm-up of all
        want = P.cohort_measures(mats[:3].cpu(), thr[:3].cpu().tolist())
        rel64 = ((got[:3].cpu().double() - want).abs() / want.abs().clamp_min(1e-30)).amax((0, 1)).tolist()
        three = variants["global"]()
        assert torch.equal(three, got[:, :, :3]), "the columns do not depend on the request"
        diff = None
        if not args.skip_torch:
            ref = variants["torch"]()
            diff = float((three - ref).abs().max())
            del ref
        del got, three
        ms = {name: [] for name in variants}
        peak = {name: 0 for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                t, p, _ = timed(fn)
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        ids = (ctypes.c_int32 * 4)(0, 1, 2, 3)
        ws_bytes = int(lib.cgnn_ingest_paths_workspace_bytes(S, n, ids, 4))
        for name, F in (("global", 3), ("all", 4)):
            assert 4 * S * n * F + ws_bytes <= peak[name] <= 4 * S * n * F + ws_bytes + 4096, (name, peak[name])
        med = statistics.median(ms["global"])
        point = {"S": S, "n": n, "keep": keep, "global_ms": spread(ms["global"]), "all_ms": spread(ms["all"]),
                 "torch_ms": spread(ms["torch"]) if "torch" in ms else None,
                 "global_below_torch_min": med < min(ms["torch"]) if "torch" in ms else None,
                 "peak_bytes_above_input": peak, "workspace_bytes": ws_bytes, "input_bytes": 4 * S * n * n,
                 # 64-bit LDS word reads of the global pass: every node expanded once per source
                 "global_word_reads": S * n * n * -(-n // 64),
                 "max_abs_diff_global_vs_torch": diff, "max_rel_err_vs_fp64_first_3_subjects_per_measure": rel64}
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
