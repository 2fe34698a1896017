"""SHA-256 of every output of the time-series entry points on seeded inputs, as one JSON object: two builds of the
library (CGNN_LIB selects one, a fresh process each) compute the same bits iff the two objects are equal.

  python tools/ingest_bits.py [--out FILE]      (the object goes to FILE, or to stdout; a summary line to stderr)

S = 3; n in {5, 68, 70} (below one column item, two items vectorised, two items scalar); T in {45, 75} (no multiple of
32; the last block of 8 frames partly filled, for some waves empty); whole runs and window=20, stride=7; q in {5, 40}
(qpad 32 and 64); six masks; every public call that takes a mask, and filter_timeseries in each of its forms.  The
unmasked k_filter at Kpad = 32, 64, 192 and 256 runs through cgnn_ingest_filter itself at T = 400: the smaller set of
a band of a 400-frame run holds at most 199 components, so filter_timeseries never asks for Kpad = 256 there.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connectome_gnn_amd import _lib, ingest  # noqa: E402

DEV = "cuda"
S = 3
MASKS = ("none", "all", "random", "empty", "one", "poison")
BAND = dict(t_r=2.0, high_pass=0.01, low_pass=0.1)
HIGH = dict(t_r=2.0, high_pass=0.01)


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def inputs(T: int, n: int, kind: str):
    """(time series [S, T, n], {q: confounds [S, T, q]}, mask [S, T] or None), seeded by the shape and the kind."""
    gen = torch.Generator().manual_seed(1000 * T + 10 * n + MASKS.index(kind))
    t = torch.arange(T, dtype=torch.float32)[None, :, None]
    ts = torch.randn(S, T, n, generator=gen) + 0.01 * t + 3.0         # a drift and an offset for the filter to remove
    conf = {q: torch.randn(S, T, q, generator=gen) + 0.02 * t for q in (5, 40)}
    if kind == "none":
        return ts, conf, None
    mask = torch.ones(S, T, dtype=torch.bool) if kind == "all" else torch.rand(S, T, generator=gen) > 0.3
    if kind == "empty":
        mask[1] = False                               # a subject with no kept frame
    if kind == "one":
        mask[1] = False
        mask[1, 7] = True                             # a subject with exactly one
    if kind == "poison":                              # what a censored frame holds is never looked at
        for x in (ts, *conf.values()):
            x[~mask] = torch.where(torch.arange(x.shape[2]) % 2 == 0, float("nan"), 1e30).expand_as(x)[~mask]
    return ts, conf, mask


def public_calls(out: dict) -> None:
    for n in (5, 68, 70):
        for T in (45, 75):
            for kind in MASKS:
                ts, conf, mask = inputs(T, n, kind)
                ts, mask = ts.to(DEV), None if mask is None else mask.to(DEV)
                conf = {q: c.to(DEV) for q, c in conf.items()}
                m = dict(sample_mask=mask)

                def put(name, t):
                    out[f"n{n} T{T} {kind}: {name}"] = digest(t)

                for q, c in conf.items():
                    basis, rank = ingest.confound_basis(c, **m)
                    put(f"basis q{q}", basis)
                    put(f"rank q{q}", rank)
                    put(f"regress q{q}", ingest.regress_confounds(ts, c, **m))
                    same = ts.clone()
                    put(f"regress q{q} in place", ingest.regress_confounds(same, c, out=same, **m))
                for name, w in (("run", {}), ("windows", dict(window=20, stride=7))):
                    put(f"corr {name}", ingest.correlation_matrices(ts, **w, **m))
                    put(f"partial {name}", ingest.correlation_matrices(ts, kind="partial", shrinkage="ledoit_wolf", **w, **m))
                    put(f"ledoit_wolf {name}", ingest.ledoit_wolf_shrinkage(ts, **w, **m))
                if mask is None:
                    put("filter centre", ingest.filter_timeseries(ts, t_r=2.0))
                    put("filter high-pass", ingest.filter_timeseries(ts, **HIGH))
                    put("filter band-pass", ingest.filter_timeseries(ts, **BAND))
                    put("filter band-pass confounds", ingest.filter_timeseries(ts, confounds=conf[5], **BAND))
                    continue
                put("interpolate", ingest.interpolate_censored(ts, mask))
                put("filter masked centre", ingest.filter_timeseries(ts, t_r=2.0, **m))
                put("filter masked high-pass", ingest.filter_timeseries(ts, **HIGH, **m))
                put("filter masked band-pass confounds", ingest.filter_timeseries(ts, confounds=conf[5], **BAND, **m))
                put("filter interpolated", ingest.filter_timeseries(ts, interpolate=True, **BAND, **m))
                put("filter interpolated confounds",
                    ingest.filter_timeseries(ts, confounds=conf[40], interpolate=True, **BAND, **m))


def wide_tables(out: dict) -> None:
    """The unmasked k_filter at every LDS layout it has: the keep form on components 1 .. K through the C call."""
    T, n = 400, 68
    ts = (torch.randn(S, T, n, generator=torch.Generator().manual_seed(400)) + 3.0).to(DEV)
    for K in (20, 50, 180, 250):
        kpad = (K + 31) // 32 * 32
        print(f"cgnn_ingest_filter T = {T}, K = {K}: Kpad = {kpad}", file=sys.stderr)
        res = torch.empty_like(ts)
        ingest._call(ts.device, "cgnn_ingest_filter", ts, S, T, n, (ctypes.c_int32 * K)(*range(1, K + 1)), K, 0,
                     ingest._WORK, *_lib.buf(res), workspace=("cgnn_ingest_filter", S, T, n, K))
        out[f"n{n} T{T}: filter Kpad {kpad}"] = digest(res)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", help="also write the JSON object to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ingest_bits.py needs a ROCm GPU"
    out = {}
    public_calls(out)
    wide_tables(out)
    text = json.dumps(out, indent=0, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    print(json.dumps({"library": _lib.LIB_PATH, "outputs": len(out),
                      "sha256_of_all": hashlib.sha256(text.encode()).hexdigest()}), file=sys.stderr)


if __name__ == "__main__":
    main()
