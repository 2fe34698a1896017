"""SHA-256 of the losses and of every parameter after three training steps from a fixed seed, once per way a
batch can reach an encoder, as one JSON object: two commits choose and run the same encoders iff their objects
are equal.  Written against the public surface only (the models, Trainer, prepare_batch, the loaders), so the
same file runs on both.

  python tools/encoder_bits.py [--out FILE]      (the object goes to FILE, or to stdout; a summary line to stderr)
"""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import connectome_gnn_amd as C  # noqa: E402
from connectome_gnn_amd.optim import Adam  # noqa: E402

DEV = "cuda"
STEPS = 3


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def graphs(n: int, nodes: int, k: int, seed: int):
    return C.generate_dataset(n, nodes, k, seed=seed)


# name: (model class, hidden, model kwargs, graphs, prepare_batch(reuse=True) first)
EAGER = {
    "tile":             (C.GCNConnectome, 64, {}, lambda: graphs(4, 84, 8, 1), False),
    "tile kept twin":   (C.GCNConnectome, 64, {}, lambda: graphs(4, 84, 8, 1), True),
    "wide h128":        (C.GCNConnectome, 128, {}, lambda: graphs(4, 84, 8, 2), False),
    "wide h128 twin":   (C.GCNConnectome, 128, {}, lambda: graphs(4, 84, 8, 2), True),
    "wide 400 band":    (C.GCNConnectome, 64, {}, lambda: graphs(2, 400, 6, 3) + graphs(1, 30, 4, 4), False),
    "wide 500 band":    (C.GCNConnectome, 64, {}, lambda: graphs(2, 500, 100, 5), True),
    # (more than 1024 nodes: no band operators)
    "wide 1100":        (C.GCNConnectome, 64, {}, lambda: graphs(1, 1100, 6, 9) + graphs(1, 30, 4, 4), False),
    "sage 1100":        (C.GraphSAGEConnectome, 64, {}, lambda: graphs(1, 1100, 6, 9) + graphs(1, 30, 4, 4), True),
    "layered gcn band": (C.GCNConnectome, 32, {}, lambda: graphs(2, 500, 100, 5), True),
    "layered sage band": (C.GraphSAGEConnectome, 32, {}, lambda: graphs(2, 500, 100, 5), False),
    "half":             (C.GCNConnectome, 64, {"storage": "fp16"}, lambda: graphs(2, 500, 100, 5), False),
    "sage tiled":       (C.GraphSAGEConnectome, 64, {}, lambda: graphs(4, 84, 8, 6), False),
    "sage tiled twin":  (C.GraphSAGEConnectome, 128, {}, lambda: graphs(4, 84, 8, 6), True),
    "sage 500 band":    (C.GraphSAGEConnectome, 64, {}, lambda: graphs(2, 500, 100, 5), True),
    "layered gcn h32":  (C.GCNConnectome, 32, {}, lambda: graphs(4, 84, 8, 7), False),
    "layered gcn impl": (C.GCNConnectome, 64, {"impl": "layered"}, lambda: graphs(4, 84, 8, 7), True),
    "layered sage h32": (C.GraphSAGEConnectome, 32, {}, lambda: graphs(4, 84, 8, 7), False),
}


def state(model, losses) -> dict:
    out = {"losses": digest(torch.tensor(losses, dtype=torch.float64))}
    for name, p in model.named_parameters():
        out[name] = digest(p)
    for name, b in model.named_buffers():
        out[name] = digest(b)
    return out


def eager(cls, hidden, kw, make, reuse) -> dict:
    torch.manual_seed(11)
    m = cls(5, hidden, dropout=0.3, **kw).to(DEV).train()
    b = C.collate_graphs(make()).to(DEV)
    if reuse:
        m.prepare_batch(b, reuse=True)
    opt = Adam(m.parameters(), lr=1e-2)
    losses = []
    for _ in range(STEPS):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(m(b), b.labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    out = state(m, losses)
    out["ran"] = f"{m.impl_used}/{getattr(m, '_fused_kind', None)}"       # (compared like a digest)
    out["band"] = str(sorted((k, v is not None) for k, v in b.structure().__dict__.get("_band_ops", {}).items()))
    return out


def through_trainer(cls) -> dict:
    """Twelve same-atlas graphs, batches of four: Trainer packs them into HBM and serves the batches from the
    per-subject structure cache, one captured step per batch size."""
    torch.manual_seed(13)
    m = cls(5, 64, dropout=0.3)
    tr = C.Trainer(m, torch.optim.Adam(m.parameters(), lr=1e-2), device=DEV)
    torch.manual_seed(14)
    ld = C.ConnectomeDataLoader(graphs(12, 84, 8, 8), batch_size=4, shuffle=True)
    losses = [tr.train_epoch(ld) for _ in range(2)]
    out = state(m, losses)
    out["ran"] = f"{m.impl_used}/{getattr(m, '_fused_kind', None)}"
    out["cache"] = str([v[2] is not None and v[2].structure_cache is not None for v in tr._resident.values()])
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", help="also write the JSON object to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "encoder_bits.py needs a ROCm GPU"
    out = {}
    for name, cfg in EAGER.items():
        for key, val in eager(*cfg).items():
            out[f"{name}: {key}"] = val
    for name, cls in (("trainer gcn", C.GCNConnectome), ("trainer sage", C.GraphSAGEConnectome)):
        for key, val in through_trainer(cls).items():
            out[f"{name}: {key}"] = val
    text = json.dumps(out, indent=0, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    print(json.dumps({"package": os.path.dirname(C.__file__), "entries": len(out),
                      "sha256_of_all": hashlib.sha256(text.encode()).hexdigest()}), file=sys.stderr)


if __name__ == "__main__":
    main()
