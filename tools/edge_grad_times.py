#!/usr/bin/env python3
"""What differentiable edge weights cost: HIP-event time of one layered training step (forward, loss,
backward) with and without ``batch.edge_weight.requires_grad``, at 512 x 84-ROI GCN h64, 4096 x 360-ROI
GCN h64 and 512 x 360-ROI GraphSAGE h128.  Per-kernel times (cgnn_sddmm_f32 against the transposed aggregate
of the same layer) come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
usage: python tools/edge_grad_times.py [--steps N] [--warmup W] [--only TAG]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import connectome_gnn_amd as C  # noqa: E402

CASES = [("gcn_512x84_h64", "gcn", 512, 84, 64), ("gcn_4096x360_h64", "gcn", 4096, 360, 64),
         ("sage_512x360_h128", "sage", 512, 360, 128)]


def step_time(model, batch, edge_grad: bool, steps: int, warmup: int) -> float:
    base = batch.edge_weight.detach()
    ew = base.clone().requires_grad_(True) if edge_grad else base
    batch.edge_weight = ew
    batch.structure()                                 # built once, outside the timed region

    def one():
        model.zero_grad(set_to_none=True)
        if ew.grad is not None:
            ew.grad = None
        loss = torch.nn.functional.cross_entropy(model(batch), batch.labels)
        loss.backward()
    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        one()
    b.record()
    torch.cuda.synchronize()
    assert model.impl_used == "layered" and (ew.grad is not None) == edge_grad
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    for tag, kind, nb, n, hid in CASES:
        if args.only and args.only != tag:
            continue
        b = C.collate_graphs(C.generate_dataset(nb, n, 10, seed=1)).to("cuda")
        torch.manual_seed(0)
        cls = C.GCNConnectome if kind == "gcn" else C.GraphSAGEConnectome
        m = cls(5, hid, dropout=0.3, impl="layered").to("cuda").train()
        t0 = step_time(m, b, False, args.steps, args.warmup)
        t1 = step_time(m, b, True, args.steps, args.warmup)
        print(f"{tag:20s} E={b.edge_index.shape[1]:9d}  step {t0:8.3f} ms  with edge grads {t1:8.3f} ms  "
              f"overhead {t1 - t0:7.3f} ms ({100 * (t1 / t0 - 1):5.1f} %)", flush=True)


if __name__ == "__main__":
    main()
