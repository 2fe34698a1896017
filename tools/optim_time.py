#!/usr/bin/env python3
"""Time the optimizer launch of connectome_gnn_amd.optim (csrc/adam.hip): the entry that takes the
hyper-parameters by value (cgnn_adam_step) beside the one that reads them from the device table (cgnn_adam_step_dev),
the headline step of two source trees, and what one recapture costs a Trainer whose optimizer freezes its values.

    python tools/optim_time.py [--models gcn:64,sage:128] [--chain 200] [--rounds 9] [--parent-lib PATH]
                               [--parent-tree DIR] [--bench-steps 20] [--bench-warmup 5] [--bench-rounds 3]
                               [--recapture 512x84] [--recapture-rounds 5] [--only launch,headline,recapture]

  launch     per model (kind:hidden, 3 layers, 5 input features): the update of all its parameters, seeded gradients,
             lr 1e-3, weight_decay 1e-4.  Per variant a HIP graph of --chain consecutive optimizer steps is captured
             once and replayed between two HIP events (back-to-back launches on one stream: the figure is the launch's
             time on the device, not the host's time to issue it); after a warm-up replay of all, the variants
             alternate for --rounds rounds; min / median / max of microseconds per step.  Variants: by_value and
             device (AdamW: device_decoupled) of this build's library and, with --parent-lib, by_value of that library
             (the parent commit's build): the spread of its repeats is the margin the comparison has.
  headline   with --parent-tree: `bench.py --gpus 1 --steps K --warmup W` as a child process in that tree and in this
             one, alternately, --bench-rounds times each; ms_per_step of each run.
  recapture  S x n: the unchanged reference script (a list-backed ConnectomeDataLoader of 2 S subjects of n ROIs,
             batch S, Trainer defaults, torch.optim.Adam): after the epoch that captures, epochs alternate between one
             before which lr was changed (its first batch releases the stale step, runs eagerly and captures again;
             the second replays) and one before which nothing changed (two replays), each between two
             synchronisations on the host clock.  The difference of the medians is the host time from the release of
             the stale step to the first replay, less one replayed step.  The same with optim.Adam: no recapture.
One JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import connectome_gnn_amd as C  # noqa: E402
from connectome_gnn_amd import _lib  # noqa: E402

LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 1e-4


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def jobs_of(ps, gs, ms, vs):
    out = []
    for lo in range(0, len(ps), _lib.ADAM_MAX_JOBS):
        jb = _lib.CgnnAdamJobs()
        jb.n = len(ps[lo:lo + _lib.ADAM_MAX_JOBS])
        for i in range(jb.n):
            jb.numel[i] = ps[lo + i].numel()
            jb.param[i], jb.grad[i] = ps[lo + i].data_ptr(), gs[lo + i].data_ptr()
            jb.exp_avg[i], jb.exp_avg_sq[i] = ms[lo + i].data_ptr(), vs[lo + i].data_ptr()
        out.append(jb)
    return out


def launch_point(kind, hidden, chain, rounds, parent):
    torch.manual_seed(0)
    cls = C.GCNConnectome if kind == "gcn" else C.GraphSAGEConnectome
    ps = [p.detach().clone() for p in cls(5, hidden, 2, 3, 0.3).to("cuda").parameters()]
    gs = [torch.randn_like(p) * 1e-2 for p in ps]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    jobs = jobs_of(ps, gs, ms, vs)
    step = torch.zeros((), device="cuda")
    arrivals = torch.zeros(1, dtype=torch.int32, device="cuda")
    hyper = torch.zeros(_lib.ADAM_HYPER_STRIDE, dtype=torch.float64)
    hyper[:5] = torch.tensor([LR, B1, B2, EPS, WD], dtype=torch.float64)
    hyper = hyper.to("cuda")
    last = len(jobs) - 1

    def by_value(fn):
        def one():
            sp = _lib.stream_ptr()
            for i, jb in enumerate(jobs):
                rc = fn(jb, step, arrivals, int(i == last), LR, B1, B2, EPS, WD, sp)
                assert rc == 0, rc
        return one

    def device(decoupled):
        def one():
            for i, jb in enumerate(jobs):
                _lib.call("cgnn_adam_step_dev", jb, step, arrivals, int(i == last), hyper, decoupled)
        return one

    variants = {"by_value": by_value(_lib.load().cgnn_adam_step), "device": device(0), "device_decoupled": device(1)}
    if parent is not None:
        variants["parent_by_value"] = by_value(parent.cgnn_adam_step)
    graphs = {}
    side = torch.cuda.Stream()
    for name, one in variants.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            one()                                                 # (loads the code object outside the capture)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(chain):
                one()
        g.replay()                                                # warm-up of all
        graphs[name] = g
    torch.cuda.synchronize()
    us = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            e.record()
            torch.cuda.synchronize()
            us[name].append(a.elapsed_time(e) * 1e3 / chain)
    return {"model": f"{kind}:{hidden}", "tensors": len(ps), "parameters": sum(p.numel() for p in ps),
            "launches_per_step": len(jobs), "chain": chain, **{name + "_us": spread(v) for name, v in us.items()},
            "steps_taken": float(step)}


def bench_once(tree, steps, warmup):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                         cwd=tree, check=True, capture_output=True, text=True, timeout=900).stdout
    rec = json.loads([line for line in out.splitlines() if line.startswith("{")][-1])
    return rec["ms_per_step"]


def recapture_point(S, n, rounds, ours):
    graphs = C.generate_dataset(2 * S, n, 8, seed=5)
    torch.manual_seed(3)
    m = C.GCNConnectome(5, 64, dropout=0.0)
    if ours:
        from connectome_gnn_amd.optim import Adam
        opt = Adam(m.parameters(), lr=1e-3)
    else:
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    tr = C.Trainer(m, opt, device="cuda")
    ld = C.ConnectomeDataLoader(graphs, batch_size=S, shuffle=True)

    def epoch():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.train_epoch(ld)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    first = epoch()                                              # packs the dataset and captures
    epoch()                                                      # (a replayed epoch as warm-up)
    changed, unchanged = [], []
    for _ in range(rounds):
        opt.param_groups[0]["lr"] *= 0.9
        changed.append(epoch())
        unchanged.append(epoch())
    return {"optimizer": "optim.Adam" if ours else "torch.optim.Adam", "S": S, "n": n, "graph": bool(tr.graph),
            "first_epoch_ms": first, "epoch_after_lr_change_ms": spread(changed), "epoch_unchanged_ms": spread(unchanged),
            "difference_of_medians_ms": statistics.median(changed) - statistics.median(unchanged),
            "hyper_recaptures": tr.hyper_recaptures}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="gcn:64,sage:128")
    ap.add_argument("--chain", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent-lib", default="", help="libcgnn_hip.so of the parent commit: its cgnn_adam_step is timed too")
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: its bench.py is run too")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--recapture", default="512x84")
    ap.add_argument("--recapture-rounds", type=int, default=5)
    ap.add_argument("--only", default="launch,headline,recapture")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_time.py measures on a ROCm GPU; none is visible")
    only = set(args.only.split(","))
    out = {"library": _lib.LIB_PATH, "device": torch.cuda.get_device_name(0)}
    if "headline" in only and args.parent_tree:
        # child processes first, before this process holds the device's memory
        runs = {"parent": [], "this": []}
        for _ in range(args.bench_rounds):
            runs["parent"].append(bench_once(args.parent_tree, args.bench_steps, args.bench_warmup))
            runs["this"].append(bench_once(ROOT, args.bench_steps, args.bench_warmup))
        out["headline_ms_per_step"] = {"steps": args.bench_steps, "warmup": args.bench_warmup, "runs": runs,
                                       **{k: spread(v) for k, v in runs.items()}}
        print(json.dumps(out["headline_ms_per_step"]), file=sys.stderr, flush=True)
    if "launch" in only:
        parent = None
        if args.parent_lib:
            parent = ctypes.CDLL(args.parent_lib)
            parent.cgnn_adam_step.restype, parent.cgnn_adam_step.argtypes = _lib.PROTOTYPES["cgnn_adam_step"]
        out["launch"] = []
        for spec in args.models.split(","):
            kind, hidden = spec.split(":")
            out["launch"].append(launch_point(kind, int(hidden), args.chain, args.rounds, parent))
            print(json.dumps(out["launch"][-1]), file=sys.stderr, flush=True)
    if "recapture" in only:
        S, n = (int(v) for v in args.recapture.split("x"))
        out["recapture"] = [recapture_point(S, n, args.recapture_rounds, ours) for ours in (False, True)]
        print(json.dumps(out["recapture"]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
