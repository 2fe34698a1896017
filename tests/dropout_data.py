"""Host statement of the dropout stream (csrc/drop_ew.h, csrc/head.hip, _lib.next_seed, graphed.py), in
plain numpy / Python integers, written from the contract and importing nothing of the package:

  keys        key0 = lo32(seed) * 0x9E3779B9 + salt0,  key1 = hi32(seed) ^ salt1 ^ (device word)
  threshold   thr16 = min(floor(p * 65536 + 0.5), 65535);  an element is KEPT iff its 16-bit draw >= thr16
  layers      chunk index = row * (width / 4) + chunk;  h0 = mix32((index ^ key0) + key1),
              h1 = mix32(h0 + 0x9E3779B9);  draws (h0 lo16, h0 hi16, h1 lo16, h1 hi16) <-> columns 4*chunk + 0..3
  head        element e = r * H2 + j, salts of its own, draw = lo16(mix32(mix32(e ^ key0) + key1))
  replay      device word i of a captured step becomes mix32(word + 0x9E3779B9 * (i + 1)) every step
  seeds       outside capture: mix64(mix64(initial_seed) + offset) >> 2, the generator's offset advancing by 4

tests/test_dropout_math.py establishes the statistical quality of this model on the CPU;
tests/test_gpu_dropout.py shows that every kernel draws exactly these bits.
"""
from __future__ import annotations

import numpy as np

GOLDEN = 0x9E3779B9
LAYER_SALTS = (0x85EBCA6B, 0xC2B2AE35)
HEAD_SALTS = (0x7F4A7C15, 0x94D049BB)
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


def mix32(x):
    """The mixer of drop_ew.h on a Python int or a uint32 array (arithmetic mod 2^32)."""
    if isinstance(x, np.ndarray):
        x = x.astype(np.uint64) & np.uint64(M32)
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
        x ^= x >> np.uint64(15)
        x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
        x ^= x >> np.uint64(16)
        return x
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def keys(seed: int, salt0: int = LAYER_SALTS[0], salt1: int = LAYER_SALTS[1]):
    """(key0, key1) of make_drop for a 64-bit seed."""
    seed &= M64
    return ((seed & M32) * GOLDEN + salt0) & M32, ((seed >> 32) ^ salt1) & M32


def thr16(p: float) -> int:
    """make_drop's threshold: p enters as the fp32 the C ABI carries."""
    return int(min(np.floor(float(np.float32(p)) * 65536.0 + 0.5), 65535.0))


def keep_probability(p: float) -> float:
    """q: the exact probability that a uniform 16-bit draw is >= thr16(p)."""
    return 1.0 - thr16(p) / 65536.0


def layer_keep(seed: int, p: float, rows: int, width: int, word: int = 0) -> np.ndarray:
    """bool [rows, width]: the keep decisions of a layer's dropout (every kernel that calls drop_bits)."""
    assert width % 4 == 0
    k0, k1 = keys(seed)
    k1 ^= word & M32
    idx = np.arange(rows * (width // 4), dtype=np.uint64) & np.uint64(M32)      # (the kernels index in uint32)
    h0 = mix32(((idx ^ np.uint64(k0)) + np.uint64(k1)) & np.uint64(M32))
    h1 = mix32((h0 + np.uint64(GOLDEN)) & np.uint64(M32))
    draws = np.stack([h0 & np.uint64(0xFFFF), h0 >> np.uint64(16), h1 & np.uint64(0xFFFF), h1 >> np.uint64(16)], axis=1)
    return (draws >= np.uint64(thr16(p))).reshape(rows, width)


def head_keep(seed: int, p: float, B: int, H2: int, word: int = 0) -> np.ndarray:
    """bool [B, H2]: the keep decisions of the classifier's dropout (head.hip)."""
    k0, k1 = keys(seed, *HEAD_SALTS)
    k1 ^= word & M32
    e = np.arange(B * H2, dtype=np.uint64) & np.uint64(M32)
    h = mix32((mix32(e ^ np.uint64(k0)) + np.uint64(k1)) & np.uint64(M32))
    return ((h & np.uint64(0xFFFF)) >= np.uint64(thr16(p))).reshape(B, H2)


def refresh(word: int, i: int) -> int:
    """Device word i after one more captured step (rng_refresh)."""
    return mix32((word + GOLDEN * (i + 1)) & M32)


def refresh_state(state, n: int) -> np.ndarray:
    """A whole uint32 state after one step that advances its first n words; the rest stay put."""
    out = np.array(state, dtype=np.uint32).copy()
    for i in range(n):
        out[i] = refresh(int(out[i]), i)
    return out


def _mix64(x: int) -> int:
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def next_seeds(initial_seed: int, offset: int, n: int) -> list:
    """The next n seeds outside capture from a generator at (initial_seed, offset)."""
    base = _mix64(initial_seed)
    return [_mix64(base + offset + 4 * i) >> 2 for i in range(n)]


# Which replay word each draw site reads in an L-layer model, as the code has it.  "stage": the op-by-op
# path and every BnStage encoder (GraphSAGE, wide GCN, fp16 storage) -- the dropout after layer li reads
# word li.  "tile": the per-tile GCN (fused.py) -- the dropout after layer li is drawn by layer li+1's launch
# from word li+1, the readout's from word L; word 0 is advanced but never read.  The classifier reads word L
# on every path (on the per-tile path it shares that WORD with the readout: the two streams differ in seed
# and salts).  Seeds are drawn in the order layers 0..L-1, head on every path.
def site_words(path: str, num_layers: int) -> dict:
    if path not in ("stage", "tile"):
        raise ValueError(path)
    first = 1 if path == "tile" else 0
    return {"layers": [first + li for li in range(num_layers)], "head": num_layers, "advanced": num_layers + 1}


def unpack(mask_bytes, rows: int, width: int) -> np.ndarray:
    """Keep bytes as the kernels record them (byte row * width/4 + chunk, bit i <-> column 4*chunk + i)
    -> bool [rows, width]."""
    m = np.asarray(mask_bytes, dtype=np.uint8).reshape(rows, width // 4, 1)
    return ((m >> np.arange(4, dtype=np.uint8).reshape(1, 1, 4)) & 1).astype(bool).reshape(rows, width)


def first_mismatch(got, want):
    """The comparator of the GPU tests: None when the two bool arrays are equal, else the first differing
    (row, column) in row-major order (a shape mismatch reports (-1, -1))."""
    got, want = np.asarray(got, dtype=bool), np.asarray(want, dtype=bool)
    if got.shape != want.shape:
        return (-1, -1)
    diff = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    if diff.size == 0:
        return None
    cols = want.shape[1] if want.ndim == 2 else 1
    return (int(diff[0]) // cols, int(diff[0]) % cols)


# ----------------------------------------------------------------- statistics of test_dropout_math.py
def z_rate(mask: np.ndarray, q: float, axis=None):
    """(keep rate - q) in units of sqrt(q (1 - q) / n): a scalar, or one value per column (axis=0) / row."""
    n = mask.size if axis is None else mask.shape[axis]
    return (mask.mean(axis=axis) - q) / np.sqrt(q * (1.0 - q) / n)


def z_corr(a: np.ndarray, b: np.ndarray, q: float) -> float:
    """Correlation of two masks about the KNOWN mean q, in units of its standard deviation under
    independence: sum((a - q)(b - q)) / (q (1 - q) sqrt(n))."""
    n = a.size
    return float(((a.astype(np.float64) - q) * (b.astype(np.float64) - q)).sum() / (q * (1.0 - q) * np.sqrt(n)))
