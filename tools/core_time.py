#!/usr/bin/env python3
"""Time the core decomposition of connectome_gnn_amd.ingest (csrc/core.hip) beside a plain copy of the
cohort and the torch formulation of the same values on the same GPU.

    python tools/core_time.py [--points 4096x360:0.10,4096x360:0.30,32768x84:0.10] [--rounds 5]

A point is S x n : keep.  Per point, on one resident cohort of seeded symmetric matrices (tools/ingest_time.py's) and
the thresholds of ``keep`` selected beforehand (their selection is not timed on either side):

  coreness              ingest.core_measures(m, min_weight=thr, measures=("coreness",))
  onion_layer           the same for ("onion_layer",): the same binary pass
  s_coreness            the same for ("s_coreness",): the weighted pass
  all                   the three names, one launch off one bitset
  torch_<the same>      mask, then per round (mask & alive[:, None, :]).sum(-1) -- the weighted pass a torch.bmm of the
                        fp64 weights with the alive vector --, a min, a where; as many rounds as the kernel's levels
                        report for the slowest subject (without a read-back a torch loop cannot know when to stop) --
                        with its peak memory above the inputs
  copy                  work.copy_(m): the streaming floor is HALF of it, the kernel reads the cohort once (the weighted
                        pass its kept entries once more, from L2) and writes [S, n, F]

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, the ratio of every median to the copy's, of every torch median to the kernel's,
the rounds the kernel took (median and maximum over the subjects, binary and weighted), and the largest difference
between the kernel and the torch formulation on the first 64 subjects.  One JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import ingest  # noqa: E402
from tools.ingest_time import cohort, spread, timed  # noqa: E402

NAMES = ingest.CORE_MEASURES


def torch_peel(p_of, S, n, rounds, device, dtype):
    """(value, layer) [S, n] after ``rounds`` rounds; ``p_of(alive)`` is p_u(alive) [S, n]."""
    alive = torch.ones(S, n, dtype=torch.bool, device=device)
    value = torch.zeros(S, n, dtype=dtype, device=device)
    layer = torch.zeros(S, n, dtype=torch.int32, device=device)
    level = torch.zeros(S, 1, dtype=dtype, device=device)
    none = float("inf") if dtype.is_floating_point else n
    for r in range(1, rounds + 1):
        p = p_of(alive).to(dtype)
        lowest = torch.where(alive, p, none).amin(1, keepdim=True)
        level = torch.where(lowest == none, level, torch.maximum(level, lowest))     # a subject that is done stays
        gone = alive & (p <= level)
        value = torch.where(gone, level, value)
        layer = torch.where(gone, r, layer)
        alive = alive & ~gone
    return value, layer


def torch_cores(m, thr, rounds, names):
    """[S, n, len(names)] the way one writes it in torch; ``rounds`` = (binary, weighted)."""
    S, n, _ = m.shape
    eye = torch.eye(n, dtype=torch.bool, device=m.device)
    mask = (m > thr.view(S, 1, 1)) & (m > 0) & ~eye
    cols = {}
    if "coreness" in names or "onion_layer" in names:
        k, r = torch_peel(lambda alive: (mask & alive[:, None, :]).sum(-1), S, n, rounds[0], m.device, torch.int32)
        cols["coreness"] = k.float() / max(n - 1, 1)
        cols["onion_layer"] = r.float() / n
    if "s_coreness" in names:
        w = torch.where(mask, m, 0.0).double()
        top = w.sum(2).amax(1, keepdim=True)
        sigma, _ = torch_peel(lambda alive: torch.bmm(w, alive.double().unsqueeze(2)).squeeze(2), S, n, rounds[1],
                              m.device, torch.float64)
        cols["s_coreness"] = (sigma / (top + 1e-8)).float()
        del w
    return torch.stack([cols[name] for name in names], 2)


def rounds_taken(m, thr):
    """The rounds per subject, binary and weighted: the largest layer of ``core_levels``."""
    lv = ingest.core_levels(m, min_weight=thr).amax(1).cpu()
    return {kind: {"median": int(lv[:, c].median()), "max": int(lv[:, c].max())}
            for kind, c in (("binary", 1), ("weighted", 2))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x360:0.10,4096x360:0.30,32768x84:0.10")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("core_time.py measures on a ROCm GPU; none is visible")
    out = {"rounds": args.rounds, "points": []}
    requests = {"coreness": NAMES[:1], "onion_layer": NAMES[1:2], "s_coreness": NAMES[2:], "all": NAMES}
    for spec in args.points.split(","):
        shape, keep = spec.split(":")
        S, n = (int(v) for v in shape.split("x"))
        keep = float(keep)
        torch.cuda.empty_cache()
        m = cohort(S, n)
        work = torch.empty_like(m)
        thr = ingest.select_thresholds(m, keep=keep)
        took = rounds_taken(m, thr)
        caps = (took["binary"]["max"], took["weighted"]["max"])
        variants = {"copy": lambda: work.copy_(m)}
        for key, names in requests.items():
            variants[key] = lambda names=names: ingest.core_measures(m, min_weight=thr, measures=names)
            variants["torch_" + key] = lambda names=names: torch_cores(m, thr, caps, names)
        for fn in variants.values():                                       # warm-up of all
            fn()
        head, head_thr = m[:64].contiguous(), thr[:64].contiguous()
        diff = (ingest.core_measures(head, min_weight=head_thr)
                - torch_cores(head, head_thr, caps, NAMES)).abs().amax((0, 1)).tolist()
        ms = {name: [] for name in variants}
        peak = {name: 0 for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                t, p, res = timed(fn)
                del res
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        med = {name: spread(v)["median"] for name, v in ms.items()}
        cohort_bytes = 4 * S * n * n
        point = {"S": S, "n": n, "keep": keep, "cohort_bytes": cohort_bytes,
                 **{name + "_ms": spread(v) for name, v in ms.items()},
                 **{name + "_over_copy": med[name] / med["copy"] for name in ms if name != "copy"},
                 **{f"torch_over_kernel_{name}": med["torch_" + name] / med[name] for name in requests},
                 **{name + "_peak_bytes_above_inputs": p for name, p in peak.items() if name != "copy"},
                 "copy_bytes_per_s_at_median": 2 * cohort_bytes / (med["copy"] * 1e-3),
                 "kernel_rounds": took,
                 "max_abs_difference_to_torch_first_64_subjects": dict(zip(NAMES, diff))}
        del work
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del m
    print(json.dumps(out))


if __name__ == "__main__":
    main()
