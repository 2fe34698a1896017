"""SHA-256 of every output of the matrix entry points on seeded cohorts, and the C entry points each public call
launched, as one JSON object: two builds (CGNN_LIB selects the library, the package next to this file is the host side,
a fresh process each) compute the same bits with the same launches iff the two objects are equal.  The matrix-side
counterpart of ingest_bits.py.

  python tools/matrix_bits.py [--out FILE]      (the object goes to FILE, or to stdout; a summary line to stderr)

S = 3; n in {5, 68, 70, 260} (below one 64-column chunk; two chunks with n % 4 == 0 and not; two 256-column chunks of
k_knn, R = 6 of k_modules and a PageRank subject whose entries do not all fit LDS); bit-symmetric and asymmetric
cohorts, each with one NaN and one subject without a positive entry; ten edge choices; every public call that takes one.
"""
import argparse
import hashlib
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import _lib, ingest  # noqa: E402

DEV = "cuda"
S, T, M = 3, 45, 3
SIZES = (5, 68, 70, 260)
ALL = ingest.MEASURES + ingest.PATH_MEASURES + ingest.WEIGHTED_PATH_MEASURES + ingest.MODULE_MEASURES
CLASSIC = ("weighted_clustering", "degree", "strength")
PAGERANK = ingest.CENTRALITY_MEASURES


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def cohort(n: int, symmetric: bool) -> torch.Tensor:
    gen = torch.Generator().manual_seed(10 * n + int(symmetric))
    m = torch.rand(S, n, n, generator=gen) - 0.25
    if symmetric:
        m = torch.maximum(m, m.transpose(1, 2))
    m[0, 1, 3] = float("nan")
    m[2] = -m[2].abs()                                # a subject without a positive entry
    return m.contiguous()


def choices() -> dict:
    thr = torch.tensor([0.05, 0.3, -1.0])
    out = {"keep": dict(keep=0.2), "num_edges": dict(num_edges=7), "min_weight": dict(min_weight=0.1),
           "min_weight tensor": dict(min_weight=thr)}
    for mode in ingest.KNN_MODES:
        out[f"knn {mode}"] = dict(knn=3, knn_mode=mode)
    out["mst"] = dict(backbone="mst")
    out["mst keep"] = dict(backbone="mst", keep=0.2)
    out["mst knn"] = dict(backbone="mst", knn=3)
    return out


class Recorder:
    """Every ``_lib.call`` by name, in order; ``take()`` returns and forgets them."""

    def __init__(self):
        self.names, self.call = [], _lib.call
        _lib.call = self

    def __call__(self, name, *args, **kw):
        self.names.append(name)
        return self.call(name, *args, **kw)

    def take(self) -> list:
        names, self.names = self.names, []
        return names


def run(out: dict) -> None:
    rec = Recorder()

    def put(key, call):
        rec.take()
        res = call()
        res = res if isinstance(res, dict) else {"": res}
        for name, t in res.items():
            out[f"{key}{name}"] = digest(t)
        out[f"{key}: launches"] = " ".join(rec.take())

    def dataset(ds) -> dict:
        return {f".{f}": getattr(ds, f) for f in ("x", "edge_local", "edge_weight", "edge_ptr", "edge_ptr_dev")}

    for n in SIZES:
        modules = [i % M for i in range(n)]
        shuffled = list(ALL)
        random.Random(n).shuffle(shuffled)
        y = torch.arange(S) % 2
        ts = torch.randn(S, T, n, generator=torch.Generator().manual_seed(n)).to(DEV)
        for ch, kw in (("knn", dict(knn=3)), ("mst", dict(backbone="mst", keep=0.2)),
                       ("measures", dict(keep=0.2, measures=tuple(shuffled), modules=modules))):
            put(f"n{n} T{T}: from_timeseries {ch}", lambda: dataset(ingest.from_timeseries(ts, y, **kw)))
        for symmetric in (True, False):
            m = cohort(n, symmetric).to(DEV)
            tag = f"n{n} {'sym' if symmetric else 'asym'}"
            for mode in ingest.KNN_MODES:
                put(f"{tag}: knn_sparsify {mode}", lambda: ingest.knn_sparsify(m, 3, mode=mode))
                same = m.clone()
                put(f"{tag}: knn_sparsify {mode} out=matrices", lambda: ingest.knn_sparsify(same, 3, mode=mode, out=same))
            for ch, kw in choices().items():
                key = f"{tag} {ch}: "
                kw = {k: v.to(DEV) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
                if set(kw) <= {"keep", "num_edges"}:
                    put(key + "select_thresholds", lambda: ingest.select_thresholds(m, **kw))
                if "knn" not in kw:
                    tree = {k: v for k, v in kw.items() if k != "backbone"}
                    put(key + "mst_backbone", lambda: ingest.mst_backbone(m, **tree))
                    same = m.clone()
                    put(key + "mst_backbone out=matrices", lambda: ingest.mst_backbone(same, out=same, **tree))
                put(key + "from_matrices", lambda: dataset(ingest.from_matrices(m, y, **kw)))
                for name, req in (("all", tuple(shuffled)), ("classic", CLASSIC)):
                    mod = dict(modules=modules) if name == "all" else {}
                    put(key + f"from_matrices {name}", lambda: dataset(ingest.from_matrices(m, y, measures=req, **mod, **kw)))
                    put(key + f"node_measures {name}", lambda: ingest.node_measures(m, measures=req, **mod, **kw))
                for binary in (False, True):
                    for normalize in (False, True):
                        put(key + f"module_profile binary={binary} normalize={normalize}",
                            lambda: ingest.module_profile(m, modules, binary=binary, normalize=normalize, **kw))
                for req in (PAGERANK, PAGERANK[::-1]):
                    put(key + f"centrality_measures {' '.join(req)}", lambda: ingest.centrality_measures(m, measures=req, **kw))
                put(key + "path_lengths", lambda: ingest.path_lengths(m, **kw))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", help="also write the JSON object to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "matrix_bits.py needs a ROCm GPU"
    out = {}
    run(out)
    text = json.dumps(out, indent=0, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    print(json.dumps({"library": _lib.LIB_PATH, "entries": len(out),
                      "sha256_of_all": hashlib.sha256(text.encode()).hexdigest()}), file=sys.stderr)


if __name__ == "__main__":
    main()
