#!/usr/bin/env python3
"""Time the ROI-saliency pass -- forward + backward with requires_grad node features, eval mode -- on the fused
per-tile GCN path (k_l0_bwd<WANT_G> + k_l0_dx, csrc/fused_gcn_l0.hip) and on the layered path, same commit.

    python tools/saliency_time.py [--graphs 4096] [--nodes 360] [--k 20] [--iters 20] [--warmup 5] [--reference-pass]

Structure (CSR, blocked-ELL) is prepared outside the timed region; times are HIP events around `iters` passes
after `warmup`.  Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats -- python tools/saliency_time.py`
the per-launch times of the two kernels are in the kernel statistics; with --reference-pass the fused model also
runs `iters` passes with respect to its parameters only (no requires_grad features), so that the same trace
holds the plain k_l0_bwd next to its WANT_G variant.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import connectome_gnn_amd as C  # noqa: E402


def time_impl(impl, batch, iters, warmup, frozen):
    torch.manual_seed(0)
    m = C.GCNConnectome(batch.node_features.shape[1], 64, num_layers=3, dropout=0.3, impl=impl).to("cuda").eval()
    if frozen:
        for p in m.parameters():
            p.requires_grad_(False)
    x = batch.node_features.detach().clone().requires_grad_(True)
    batch.node_features = x
    m.prepare_batch(batch)

    def step():
        x.grad = None
        m(batch)[:, 1].sum().backward()

    for _ in range(warmup):
        step()
    assert m.impl_used == impl, (m.impl_used, impl)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters, x.grad.detach().clone()


def time_params_only(batch, iters, warmup):
    torch.manual_seed(0)
    m = C.GCNConnectome(batch.node_features.shape[1], 64, num_layers=3, dropout=0.3, impl="fused").to("cuda").eval()
    batch.node_features = batch.node_features.detach()

    def step():
        m.zero_grad(set_to_none=True)
        m(batch)[:, 1].sum().backward()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=360)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--train-params", action="store_true", help="leave the parameters requiring grad")
    ap.add_argument("--reference-pass", action="store_true",
                    help="also time forward + backward w.r.t. the parameters only, fused path (plain k_l0_bwd)")
    args = ap.parse_args()
    # a few distinct subjects repeated: the timing depends on the sizes, not on the subjects
    base = C.generate_dataset(min(args.graphs, 32), args.nodes, args.k, seed=5)
    batch = C.collate_graphs([base[i % len(base)] for i in range(args.graphs)]).to("cuda")
    out = {"graphs": args.graphs, "nodes": args.nodes, "in_channels": int(batch.node_features.shape[1]),
           "frozen_parameters": not args.train_params}
    grads = {}
    for impl in ("fused", "layered"):
        out[f"{impl}_ms"], grads[impl] = time_impl(impl, batch, args.iters, args.warmup, not args.train_params)
    if args.reference_pass:
        out["fused_parameters_only_ms"] = time_params_only(batch, args.iters, args.warmup)
    scale = float(grads["layered"].abs().max())
    diff = (grads["fused"] - grads["layered"]).abs()
    out["max_abs_diff_over_scale"] = float(diff.max()) / scale
    # the two paths decide ReLU pre-activations within rounding of zero independently: a few rows differ by
    # more than rounding, the rest agree to fp32 accuracy
    out["rows_differing_by_1e-5_of_scale"] = int((diff.max(1).values > 1e-5 * scale).sum())
    out["median_abs_diff_over_scale"] = float(diff.median()) / scale
    out["speedup"] = out["layered_ms"] / out["fused_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
