#!/usr/bin/env python3
"""Time PageRank centrality of connectome_gnn_amd.ingest (csrc/pagerank.hip) beside a plain copy of the
cohort and the torch formulation of the same values on the same GPU.

    python tools/pagerank_time.py [--points 4096x360:0.10,4096x360:0.30,32768x84:0.10] [--damping 0.85] [--rounds 5]

A point is S x n : keep.  Per point, on one resident cohort of seeded symmetric matrices (tools/ingest_time.py's) and
the thresholds of ``keep`` selected beforehand (their selection is not timed on either side):

  pagerank              ingest.centrality_measures(m, min_weight=thr, measures=("pagerank",))
  weighted_pagerank     the same for ("weighted_pagerank",)
  both                  both names, one launch off one staging pass
  torch_<the same>      mask, where, column-normalise in fp64, K_max(d) steps of torch.bmm in fp64 (without a read-back
                        a torch loop cannot know when to stop) -- with its peak memory above the inputs
  copy                  work.copy_(m): the streaming floor is HALF of it, the kernel reads the cohort at least three times
                        (twice from L2) and writes [S, n, F]

All variants are warmed up first; they then alternate for --rounds rounds in this one process, each call between two HIP
events; min / median / max are reported, the ratio of every median to the copy's, of every torch median to the kernel's,
the steps the kernel took (median and maximum over the subjects, per name), and the largest difference between the
kernel and the torch formulation on the first 64 subjects.  One JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import _lib, ingest  # noqa: E402
from tools.ingest_time import cohort, spread, timed  # noqa: E402

NAMES = ingest.CENTRALITY_MEASURES


def torch_pagerank(m, thr, d, steps, names):
    """[S, n, len(names)] the way one writes it in torch: the Google matrix in fp64, ``steps`` products."""
    S, n, _ = m.shape
    eye = torch.eye(n, dtype=torch.bool, device=m.device)
    mask = (m > thr.view(S, 1, 1)) & (m > 0) & ~eye
    cols = []
    for name in names:
        w = torch.where(mask, m, 0.0).double() if name == "weighted_pagerank" else mask.double()
        c = w.sum(1, keepdim=True)
        dangling = (c == 0).double().transpose(1, 2)                       # [S, n, 1]
        w /= torch.where(c == 0, 1.0, c)
        x = torch.full((S, n, 1), 1.0 / n, dtype=torch.float64, device=m.device)
        for _ in range(steps):
            x = d * (torch.bmm(w, x) + (x * dangling).sum(1, keepdim=True) / n) + (1.0 - d) / n
        cols.append(x.squeeze(2).float())
        del w
    return torch.stack(cols, 2)


def steps_taken(m, thr, d, ident):
    S, n, _ = m.shape
    it = torch.empty(S, dtype=torch.int32, device=m.device)
    x = torch.empty(S, n, 1, device=m.device)
    ingest._run_family(ingest._CENTRALITY, m, thr, [ident], [0], x, mid=(d,), tail=_lib.buf(it))
    it = it.cpu()
    return {"median": int(it.median()), "max": int(it.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="4096x360:0.10,4096x360:0.30,32768x84:0.10")
    ap.add_argument("--damping", type=float, default=0.85)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pagerank_time.py measures on a ROCm GPU; none is visible")
    d = args.damping
    cap = ingest.pagerank_max_steps(d)
    out = {"rounds": args.rounds, "damping": d, "max_steps": cap, "points": []}
    requests = {"pagerank": NAMES[:1], "weighted_pagerank": NAMES[1:], "both": NAMES}
    for spec in args.points.split(","):
        shape, keep = spec.split(":")
        S, n = (int(v) for v in shape.split("x"))
        keep = float(keep)
        torch.cuda.empty_cache()
        m = cohort(S, n)
        work = torch.empty_like(m)
        thr = ingest.select_thresholds(m, keep=keep)
        variants = {"copy": lambda: work.copy_(m)}
        for key, names in requests.items():
            variants[key] = lambda names=names: ingest.centrality_measures(m, min_weight=thr, measures=names, damping=d)
            variants["torch_" + key] = lambda names=names: torch_pagerank(m, thr, d, cap, names)
        for fn in variants.values():                                       # warm-up of all
            fn()
        head, head_thr = m[:64].contiguous(), thr[:64].contiguous()
        diff = (ingest.centrality_measures(head, min_weight=head_thr, damping=d)
                - torch_pagerank(head, head_thr, d, cap, NAMES)).abs().amax((0, 1)).tolist()
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
                 "steps": {name: steps_taken(m, thr, d, i) for i, name in enumerate(NAMES)},
                 "max_abs_difference_to_torch_first_64_subjects": dict(zip(NAMES, diff))}
        del work
        out["points"].append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
        del m
    print(json.dumps(out))


if __name__ == "__main__":
    main()
