"""The dropout stream's host model (tests/dropout_data.py) on the CPU: its statistical quality, the exact
statements about the 16-bit threshold, the refusals of the C ABI, and a self-test of the comparator that
tests/test_gpu_dropout.py uses.  The statistics are statements about the model; once the GPU tests show that
the kernels draw the model's bits, they hold for the kernels.

Masks of 2048 x 64, p in {0.1, 0.3, 0.5}, four consecutive seeds from next_seeds(s, 0, 4) for s in
{0, 1, 5, 42, 1234567}; q = 1 - thr16 / 65536.  Bounds: |z| <= 5 for a single statistic, |z| <= 6 for a
maximum over the rows or columns of one mask.  Every test prints the worst |z| it saw (pytest -s)."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

from tests import dropout_data as D

ROWS, WIDTH = 2048, 64
PS = (0.1, 0.3, 0.5)
INITIAL = (0, 1, 5, 42, 1234567)
SHIFTS = (84, 360, 384)             # the graph sizes and the tile height
WORD = 0x12345678                   # a device word as graphed.py draws one (31 bits)
Z_ONE, Z_MAX = 5.0, 6.0


@functools.lru_cache(maxsize=None)
def _seeds(s):
    return tuple(D.next_seeds(s, 0, 4))


@functools.lru_cache(maxsize=None)
def _layer(seed, p, word=0):
    m = D.layer_keep(seed, p, ROWS, WIDTH, word)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _head(seed, p, word=0):
    m = D.head_keep(seed, p, ROWS, WIDTH, word)
    m.setflags(write=False)
    return m


def _cases():
    for s, p in itertools.product(INITIAL, PS):
        yield s, p, _seeds(s)


def _worst(name, found, bound):
    """found: [(|z|, where)] -> print the worst and assert the bound on all of them."""
    found.sort(key=lambda t: -t[0])
    print(f"\n[dropout-math] {name}: worst |z| = {found[0][0]:.2f} at {found[0][1]} (bound {bound})")
    bad = [f for f in found if not f[0] <= bound]
    assert not bad, (name, bad[:5])


@pytest.mark.parametrize("stream", ["layer", "head"])
def test_keep_rate_of_every_mask(stream):
    make = _layer if stream == "layer" else _head
    found = []
    for s, p, seeds in _cases():
        q = D.keep_probability(p)
        for seed in seeds:
            found.append((abs(float(D.z_rate(make(seed, p), q))), (s, p, seed)))
    _worst(f"{stream} keep rate", found, Z_ONE)


@pytest.mark.parametrize("stream", ["layer", "head"])
@pytest.mark.parametrize("axis,what", [(0, "columns"), (1, "rows")])
def test_keep_rate_of_every_column_and_row(stream, axis, what):
    make = _layer if stream == "layer" else _head
    found = []
    for s, p, seeds in _cases():
        q = D.keep_probability(p)
        for seed in seeds:
            z = np.abs(D.z_rate(make(seed, p), q, axis=axis))
            found.append((float(z.max()), (s, p, seed, int(z.argmax()))))
    _worst(f"{stream} {what}", found, Z_MAX)


@pytest.mark.parametrize("stream", ["layer", "head"])
def test_masks_of_two_seeds_are_uncorrelated(stream):
    make = _layer if stream == "layer" else _head
    found = []
    for s, p, seeds in _cases():
        q = D.keep_probability(p)
        for a, b in itertools.combinations(seeds, 2):
            found.append((abs(D.z_corr(make(a, p), make(b, p), q)), (s, p, a, b)))
    _worst(f"{stream} against {stream}, two seeds", found, Z_ONE)


@pytest.mark.parametrize("stream", ["layer", "head"])
def test_masks_of_successive_replay_words_are_uncorrelated(stream):
    """One seed under the words (w, refresh(w, i)) of two successive replays, for the word index i of each of
    the first four sites, and under (no word, w)."""
    make = _layer if stream == "layer" else _head
    found = []
    for s, p, seeds in _cases():
        q = D.keep_probability(p)
        for i, seed in enumerate(seeds):
            nxt = D.refresh(WORD, i)
            found.append((abs(D.z_corr(make(seed, p, WORD), make(seed, p, nxt), q)), (s, p, seed, i)))
            found.append((abs(D.z_corr(make(seed, p), make(seed, p, WORD), q)), (s, p, seed, "0->w")))
    _worst(f"{stream} successive words", found, Z_ONE)


@pytest.mark.parametrize("stream", ["layer", "head"])
def test_neighbouring_rows_and_columns_are_uncorrelated(stream):
    make = _layer if stream == "layer" else _head
    found = []
    for s, p, seeds in _cases():
        q = D.keep_probability(p)
        for seed in seeds:
            m = make(seed, p)
            found.append((abs(D.z_corr(m[:-1], m[1:], q)), (s, p, seed, "rows")))
            found.append((abs(D.z_corr(m[:, :-1], m[:, 1:], q)), (s, p, seed, "columns")))
    _worst(f"{stream} neighbouring rows / columns", found, Z_ONE)


@pytest.mark.parametrize("stream", ["layer", "head"])
def test_rows_a_graph_or_a_tile_apart_are_uncorrelated(stream):
    """Row r against row r + d for d = 84, 360 (graph sizes) and 384 (tile height): a stream indexed by the
    row inside the tile or the graph repeats at these distances."""
    make = _layer if stream == "layer" else _head
    found = []
    for s, p, seeds in _cases():
        q = D.keep_probability(p)
        for seed in seeds:
            m = make(seed, p)
            for d in SHIFTS:
                found.append((abs(D.z_corr(m[:-d], m[d:], q)), (s, p, seed, d)))
    _worst(f"{stream} row shifts {SHIFTS}", found, Z_ONE)


def test_head_stream_is_uncorrelated_with_the_layer_stream_of_its_seed():
    found = []
    for s, p, seeds in _cases():
        q = D.keep_probability(p)
        for seed in seeds:
            found.append((abs(D.z_corr(_head(seed, p), _layer(seed, p), q)), (s, p, seed, "no word")))
            found.append((abs(D.z_corr(_head(seed, p, WORD), _layer(seed, p, WORD), q)), (s, p, seed, "one word")))
    _worst("head against layer, one seed", found, Z_ONE)


# ------------------------------------------------------------------------------------- exact statements
BELOW = float(np.nextafter(np.float32(2.0 ** -17), np.float32(0)))


def test_threshold_values():
    assert D.thr16(0.3) == 19661 and D.thr16(0.5) == 32768
    assert D.thr16(2.0 ** -17) == 1
    assert D.thr16(BELOW) == 0                                   # ... which never drops:
    assert D.layer_keep(7, BELOW, 64, 64).all() and D.head_keep(7, BELOW, 64, 64).all()
    assert D.thr16(0.99999) == 65535                             # the clamp: one draw in 65536 is still kept
    assert D.thr16(0.1) == 6554


def test_realised_keep_probability_is_exactly_q():
    """Over all 65536 values of a 16-bit draw the kept fraction is q = 1 - thr16 / 65536 (mix32 is a bijection
    of the 32-bit words, so over a whole period each 16-bit half takes every value equally often)."""
    draws = np.arange(65536, dtype=np.uint64)
    for p in PS + (2.0 ** -17, BELOW, 0.99999):
        assert (draws >= np.uint64(D.thr16(p))).mean() == D.keep_probability(p)
    x = np.arange(1 << 16, dtype=np.uint64) * np.uint64(65537)
    assert np.unique(D.mix32(x)).size == x.size                  # (no collisions on a sample of the bijection)


def test_expectation_bias_of_the_sixteen_bit_threshold():
    """The kernels scale the kept elements by 1 / (1 - p), not by 1 / q: E[dropout(x)] = x q / (1 - p).
    Away from the clamp thr16 / 65536 is p rounded to 2^-16, so |q / (1 - p) - 1| <= 2^-17 / (1 - p).
    At the clamp (p > 1 - 1.5 * 2^-16) q stays 2^-16 whatever p is: q / (1 - p) = 2^-16 / (1 - p), which is
    1.52 at p = 0.99999 (fp32) and grows without bound as p -> 1."""
    for p in list(PS) + [2.0 ** -17, 0.25, 0.7, 0.9, 0.999, 1.0 - 2.0 ** -15] + list(np.linspace(0.001, 0.9999, 97)):
        p32 = float(np.float32(p))
        assert D.thr16(p) < 65535
        assert abs(D.keep_probability(p) / (1.0 - p32) - 1.0) <= 2.0 ** -17 / (1.0 - p32) * (1 + 1e-12), p
    p32 = float(np.float32(0.99999))
    assert D.keep_probability(0.99999) == 2.0 ** -16
    assert abs(D.keep_probability(0.99999) / (1.0 - p32) - 2.0 ** -16 / (1.0 - p32)) < 1e-12
    assert 1.5 < D.keep_probability(0.99999) / (1.0 - p32) < 1.6             # (1 - fp32(0.99999) = 1.0014e-5)


def test_seed_formula_and_keys():
    s = D.next_seeds(42, 0, 4)
    assert len(set(s)) == 4 and all(0 <= v < 2 ** 62 for v in s)
    assert D.next_seeds(42, 8, 2) == s[2:]                       # the offset advances by 4 per seed
    assert D.next_seeds(43, 0, 1) != s[:1]
    lo, hi = D.keys(0x00000001_00000000), D.keys(0x00000000_00000001)
    assert lo[0] == D.keys(0)[0] and lo[1] != D.keys(0)[1]       # the high half moves key1 only,
    assert hi[1] == D.keys(0)[1] and hi[0] != D.keys(0)[0]       # the low half key0 only
    assert D.keys(5) != D.keys(5, *D.HEAD_SALTS)
    assert D.refresh(0, 0) == D.mix32(D.GOLDEN) and D.refresh(7, 2) == D.mix32(7 + 3 * D.GOLDEN)
    assert int(D.mix32(np.array([123456789], dtype=np.uint64))[0]) == D.mix32(123456789)
    t = D.site_words("tile", 3), D.site_words("stage", 3)
    assert t[0] == {"layers": [1, 2, 3], "head": 3, "advanced": 4}
    assert t[1] == {"layers": [0, 1, 2], "head": 3, "advanced": 4}


# ---------------------------------------------------------------------- refusals of the C ABI (no device)
_A = 0x1000


def _refusal_calls():
    """name -> (a call with p_drop = p that does nothing when p is valid: zero rows / graphs / tiles)."""
    from connectome_gnn_amd import _lib
    lib = _lib.load()
    t = _lib.CgnnTiles()
    t.num_nodes, t.num_tiles, t.max_tile_rows = 10, 0, 16
    for f in ("tile_ptr", "tile_blk", "blk_off_dst", "ent_dst", "blk_off_src", "ent_src", "dis"):
        setattr(t, f, _A)
    tp = ctypes.byref(t)
    calls = {}
    for sfx in ("", "_f16"):
        calls["cgnn_bn_act_fwd_apply" + sfx] = lambda p, f=getattr(lib, "cgnn_bn_act_fwd_apply" + sfx): f(
            _A, _A, 1, p, 5, None, None, _A, 0, 64, None)
        calls["cgnn_bn_act_pool_fwd" + sfx] = lambda p, f=getattr(lib, "cgnn_bn_act_pool_fwd" + sfx): f(
            _A, _A, 1, p, 5, None, None, _A, 0, _A, 64, None, None)
        calls["cgnn_bn_act_bwd_stats" + sfx] = lambda p, f=getattr(lib, "cgnn_bn_act_bwd_stats" + sfx): f(
            _A, _A, _A, _A, 1, p, 0, 64, _A, 1 << 20, None, None, None, None)
        calls["cgnn_bn_act_bwd_apply" + sfx] = lambda p, f=getattr(lib, "cgnn_bn_act_bwd_apply" + sfx): f(
            _A, _A, _A, _A, _A, 1, p, 0, None, 0, _A, 0, 64, None, None, None, None)
    calls["cgnn_head_fwd_f32"] = lambda p: lib.cgnn_head_fwd_f32(_A, 0, 64, 32, 2, _A, _A, _A, _A, p, 5, None, _A, _A, _A, None)
    calls["cgnn_gcn_fused_pool_fwd"] = lambda p: lib.cgnn_gcn_fused_pool_fwd(_A, _A, p, 5, None, None, _A, 0, _A, None, None, None)
    calls["cgnn_aggregate_tiled_bn_f32"] = lambda p: lib.cgnn_aggregate_tiled_bn_f32(
        tp, 0, _A, 64, 64, None, None, None, _A, 64, _A, 1, p, 5, None, None, _A, 64, None)
    return lib, _lib, calls, t


# entry points whose call with zero rows is CGNN_OK for a valid p: the refusal below is then p's doing
_NOOP_OK = ("cgnn_bn_act_fwd_apply", "cgnn_bn_act_fwd_apply_f16", "cgnn_bn_act_pool_fwd", "cgnn_bn_act_pool_fwd_f16",
            "cgnn_bn_act_bwd_stats", "cgnn_bn_act_bwd_stats_f16", "cgnn_bn_act_bwd_apply", "cgnn_bn_act_bwd_apply_f16",
            "cgnn_head_fwd_f32", "cgnn_gcn_fused_pool_fwd", "cgnn_aggregate_tiled_bn_f32")


def test_entry_points_refuse_a_probability_outside_zero_one():
    """p_drop < 0 and p_drop >= 1 are CGNN_EINVAL at every entry point that takes p_drop and checks it before it
    launches (the tile kernels' are pinned in test_host_logic.py).  Calls with zero rows / graphs / tiles: with a
    valid p they return CGNN_OK without touching a pointer, so nothing here needs a device."""
    lib, _lib, calls, _keep = _refusal_calls()
    for name in _NOOP_OK:
        for p in (0.0, 0.3, 0.99999):
            assert calls[name](p) == _lib.CGNN_OK, (name, p)
        for p in (-0.5, -1e-6, 1.0, 1.5):
            assert calls[name](p) == _lib.CGNN_EINVAL, (name, p)
    # the one-launch classifier + loss has no empty form (B <= 0 is itself refused): a full argument list
    for p in (-0.5, 1.0):
        assert lib.cgnn_head_loss_f32(_A, 8, 64, 32, 2, _A, _A, _A, _A, _A, p, 5, None, _A, _A, _A, _A, _A, 1 << 24,
                                      None) == _lib.CGNN_EINVAL
    # the words: none, and more than the 64 a state may hold (checked before the launch)
    assert lib.cgnn_rng_advance(_A, 0, None) == _lib.CGNN_EINVAL
    assert lib.cgnn_rng_advance(_A, 65, None) == _lib.CGNN_EINVAL
    assert lib.cgnn_rng_advance(None, 4, None) == _lib.CGNN_EINVAL
    assert lib.cgnn_bn_stats_finalize_rng(_A, 4, 10.0, _A, _A, _A, _A, 0.1, 1e-5, _A, _A, _A, 65, None, None) == _lib.CGNN_EINVAL
    assert lib.cgnn_bn_stats_finalize_rng(_A, 4, 10.0, _A, _A, _A, _A, 0.1, 1e-5, _A, _A, None, 4, None, None) == _lib.CGNN_EINVAL


# ------------------------------------------------------------------------ the comparator's self-test
def test_comparator_reports_each_wrong_mask_with_its_first_difference():
    """first_mismatch (what the GPU tests assert with) on a model mask against itself and against the masks the
    wrong kernels of the issue would record: shifted by a row, the first 384 rows repeated (a tile-local row
    index), the bits of a chunk in another order, the neighbouring replay word, the other stream's keys, a seed
    that lost either half."""
    seed, p, rows, width = D.next_seeds(42, 0, 1)[0], 0.3, 1000, 64
    want = D.layer_keep(seed, p, rows, width, 3)
    assert D.first_mismatch(want.copy(), want) is None
    packed = np.zeros((rows, width // 4), dtype=np.uint8)
    for i in range(4):
        packed |= want[:, i::4].astype(np.uint8) << i
    assert D.first_mismatch(D.unpack(packed.reshape(-1), rows, width), want) is None     # (the recorded layout)

    def first(got):
        hit = D.first_mismatch(got, want)
        assert hit is not None
        r, c = hit
        assert got[r, c] != want[r, c] and np.array_equal(got.reshape(-1)[:r * width + c], want.reshape(-1)[:r * width + c])
        return hit

    assert first(np.roll(want, 1, axis=0))[0] == 0
    tiled = np.concatenate([want[:384]] * 3)[:rows]
    assert first(tiled)[0] == 384                                 # right up to the second tile
    swapped = want.reshape(rows, width // 4, 4)[:, :, [1, 0, 2, 3]].reshape(rows, width)
    assert first(swapped)[0] == 0
    reversed_ = want.reshape(rows, width // 4, 4)[:, :, ::-1].reshape(rows, width)
    assert first(reversed_)[0] == 0
    for word in (2, 4):
        assert first(D.layer_keep(seed, p, rows, width, word))[0] == 0
    assert first(D.layer_keep(seed & 0xFFFFFFFF, p, rows, width, 3))[0] == 0
    assert first(D.layer_keep(seed >> 32 << 32, p, rows, width, 3))[0] == 0
    assert first(D.head_keep(seed, p, rows, width, 3))[0] == 0
    one = want.copy()
    one[999, 63] ^= True
    assert first(one) == (999, 63)
    assert D.first_mismatch(want[:999], want) == (-1, -1)


# ------------------------------------------------- the captured step's dropout words are sized from the model
def test_captured_step_sizes_its_dropout_words_from_the_model_and_refuses_what_it_cannot_hold():
    """GraphedTrainStep: word i < num_layers belongs to an encoder site, word num_layers to the classifier, and a
    step advances num_layers + 1 of them (at most 64).  The state is at least 16 words and at least num_layers + 1;
    more than 64, or a preset state that is too short, is a ValueError before anything is captured."""
    import types

    import torch
    from connectome_gnn_amd.graphed import GraphedTrainStep
    cpu = torch.device("cpu")

    def model(layers, state=None):
        return types.SimpleNamespace(convs=[None] * layers, rng_device_state=state)

    for layers, words in ((1, 16), (3, 16), (15, 16), (16, 17), (40, 41), (63, 64)):
        m = model(layers)
        GraphedTrainStep._own_rng_words(m, cpu)
        assert m.rng_device_state.shape == (words,) and m.rng_device_state.dtype == torch.int32
    with pytest.raises(ValueError, match="at most 64"):
        GraphedTrainStep._own_rng_words(model(64), cpu)
    keep = torch.arange(17, dtype=torch.int32)
    m = model(16, keep)
    GraphedTrainStep._own_rng_words(m, cpu)
    assert m.rng_device_state is keep                             # a preset state that is long enough stays
    for bad in (torch.zeros(16, dtype=torch.int32), torch.zeros(17, dtype=torch.int64),
                torch.zeros(17, 1, dtype=torch.int32), torch.zeros(34, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="at least 17 words"):
            GraphedTrainStep._own_rng_words(model(16, bad), cpu)
