"""The random-walk encodings of connectome_gnn_amd.ingest on the device (csrc/rw.hip) against the fp64 host statement of
tests/rw_data.py (explicit powers of ``P`` in numpy).

What is asserted, derived and not taken from what the kernel gives:

* every column of a step ``k >= 2`` lies within ``1.01 ((k - 2) n + 2 k + 1) 2^-24 |r_k| + 2^-40`` of the statement
  (``rw_data``'s module docstring derives it from the arithmetic that include/cgnn_rw.h fixes), unclamped;
* step 1, an isolated node's row, a subject without edges, ``n == 1`` and every odd step on a bipartite kept set are
  ``+0.0`` bit for bit;
* a NaN is never an edge; a kept ``+inf`` makes its subject's columns for ``k >= 2`` NaN and changes no bit elsewhere;
* every subset and order of the steps, a second run and a grid of 3 give the bits of the full call on the default grid.

The measured maxima are printed, in units of the bound.
"""
import ctypes

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import cohort_kit as K
from tests import ingest_data as I
from tests import rw_data as RD
from tests.cohort_kit import DEV, NAN_BITS, bits as _bits

pytestmark = pytest.mark.gpu
ALL = list(range(8))


def _raw(dev, thr, ids=ALL, cols=ALL, ldx=8, flags=0, short_by=0, expect=_lib.CGNN_OK):
    """One cgnn_ingest_rw call into a NaN-filled x ``[S, n, ldx]`` with the workspace its query asks for, less
    ``short_by`` bytes."""
    S, n, num = int(dev.shape[0]), int(dev.shape[1]), len(ids)
    need = _lib.load().cgnn_ingest_rw_workspace_bytes(S, n, (ctypes.c_int32 * num)(*ids), num)
    assert need >= 0
    work = torch.empty(max(need - short_by, 0), dtype=torch.uint8, device=DEV) if need else None
    x, rc = K.raw("cgnn_ingest_rw", dev, thr, ids, cols, ldx, mid=(flags,), work=work, accept=(expect,))
    assert rc == expect
    torch.cuda.synchronize()
    return x, need


def _thresholds(dev, mats, keep):
    return K.thresholds(dev, mats, {"keep": keep})


def _assert_within_bound(got, want, n, what, steps=RD.STEPS):
    """``got`` fp32 ``[.., n, len(steps)]`` against the fp64 statement ``want``; returns the share of the bound."""
    got = got.cpu()
    assert bool(torch.isfinite(got).all()), what
    assert bool((got >= 0).all()), (what, "a probability")
    for c, k in enumerate(steps):
        if k == 1:
            assert not _bits(got[..., c]).any(), (what, "step 1 is +0.0")
    share = RD.share_of_bound(got.numpy(), want, n, steps)
    assert share <= 1.0, (what, share)
    return share


# ---- 1: parity at every size, both densities, weighted and binary ----
@pytest.mark.parametrize("n", RD.GPU_SIZES)
def test_parity_with_the_fp64_statement(n):
    mats = RD.cohort(n)
    dev = mats.to(DEV)
    worst = 0.0
    for keep in RD.KEEPS:
        thr, _ = _thresholds(dev, mats, keep)
        for binary in (False, True):
            what = f"n={n} keep={keep} binary={binary}"
            want = RD.cohort_statement(n, keep, binary)
            got = ingest.random_walk_encodings(dev, keep=keep, binary=binary)
            assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (len(mats), n, 8)
            worst = max(worst, _assert_within_bound(got, want, n, what))
            assert not _bits(got[RD.ALL_ZERO]).any(), (what, "a subject without edges")
            isolated = torch.from_numpy(want.sum(2) == 0)
            assert not _bits(got.cpu()[isolated]).any(), (what, "an isolated node's row")
            x, _ = _raw(dev, thr, flags=int(binary))
            assert torch.equal(_bits(x), _bits(got)), (what, "the raw call")
    if n == 1:
        assert not _bits(got).any(), "one node: all zeros"
    print(f"n={n}: largest error {worst:.3f} of the bound")


@pytest.mark.parametrize("n,keep,binary", [(600, 0.30, False), (1024, 0.10, False), (1024, 0.10, True)])
def test_the_largest_sizes(n, keep, binary):
    mats = RD.large(n)
    dev = mats.to(DEV)
    _thresholds(dev, mats, keep)
    t = RD.host_thresholds(mats, {"keep": keep})[0]
    want = RD.statement(mats[0], t, RD.STEPS, binary)[None]
    got = ingest.random_walk_encodings(dev, keep=keep, binary=binary)
    share = _assert_within_bound(got, want, n, f"n={n}")
    print(f"n={n} keep={keep} binary={binary}: largest error {share:.3f} of the bound")


def test_more_than_1024_nodes_are_refused():
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.random_walk_encodings(torch.zeros(1, 1025, 1025, device=DEV), keep=0.1)


# ---- 2: the exact zeros ----
def test_the_exact_zeros():
    n = 97
    complete = RD.complete(n)
    complete[40, :] = 0.0
    complete[:, 40] = 0.0                                        # node 40 is isolated
    mats = torch.stack([RD.bipartite(n), RD.star(n), torch.zeros(n, n), complete, RD.bipartite(n, 1).t()]).contiguous()
    dev = mats.to(DEV)
    for binary in (False, True):
        got = ingest.random_walk_encodings(dev, min_weight=0.0, binary=binary)
        assert torch.equal(got[:, :, 0], torch.zeros(5, n, device=DEV)), "step 1"
        for s in (0, 1, 4):
            assert not _bits(got[s, :, 0::2]).any(), (s, "bipartite: every odd step is +0.0, not a small number")
            assert bool((got[s, :, 1::2] > 0).all())
        assert torch.equal(got[2], torch.zeros(n, 8, device=DEV)) and not _bits(got[2]).any(), "no edges"
        assert not _bits(got[3, 40]).any() and bool((got[3, :40, 1:] > 0).all()), "the isolated node"
        want = np.stack([RD.statement(A, 0.0, RD.STEPS, binary) for A in mats])
        _assert_within_bound(got, want, n, f"binary={binary}")
    for n in (2, 16):                                            # an even cycle (an edge at n = 2), and one node
        ring = ingest.random_walk_encodings(RD.cycle(n)[None].to(DEV), min_weight=0.0)
        assert not _bits(ring[0, :, 0::2]).any() and bool((ring[0, :, 1::2] > 0).all())
    one = ingest.random_walk_encodings(torch.full((3, 1, 1), 0.5, device=DEV), min_weight=0.0)
    assert tuple(one.shape) == (3, 1, 8) and not _bits(one).any(), "n == 1"


# ---- 3: NaN and +inf ----
def test_a_nan_is_no_edge_and_a_kept_infinity_stays_in_its_subject():
    n, s = 84, 5
    raw = I.recipe(n)                                            # unclamped: subject 5 has +inf at (0, 3) and (3, 0)
    assert float(raw[s, 0, 3]) == float("inf") and float(raw[4, n // 2, n // 2]) == float("inf")
    assert bool(torch.isnan(raw[4]).any())
    dev = raw.to(DEV)
    got = ingest.random_walk_encodings(dev, min_weight=0.0).cpu()
    assert bool(torch.isnan(got[s, :, 1:]).all()) and not _bits(got[s, :, 0]).any(), "k >= 2 of the subject, and no r_1"
    assert int(torch.isnan(got).sum()) == 7 * n, "and nothing else: NaN entries and a +inf diagonal are never kept"
    others = ingest.random_walk_encodings(dev[:s].contiguous(), min_weight=0.0).cpu()
    assert torch.equal(_bits(got[:s]), _bits(others)), "no bit of another subject changes"
    worst = 0.0
    for u in range(s):
        want = RD.statement(raw[u], 0.0)
        worst = max(worst, _assert_within_bound(got[u], want, n, f"unclamped subject {u}"))
    without = raw[4].clone()
    without[torch.isnan(without)] = 0.0
    assert torch.equal(_bits(got[4]), _bits(ingest.random_walk_encodings(without[None].to(DEV), min_weight=0.0).cpu()[0]))
    # with equal weights the +inf is an edge like any other: no weight is read as a number
    binary = ingest.random_walk_encodings(dev, min_weight=0.0, binary=True).cpu()
    want = np.stack([RD.statement(A, 0.0, RD.STEPS, True) for A in raw])
    worst = max(worst, _assert_within_bound(binary, want, n, "binary"))
    # kept by a selected threshold too
    top = ingest.random_walk_encodings(dev, keep=0.1).cpu()
    assert bool(torch.isnan(top[s, :, 1:]).all()) and int(torch.isnan(top).sum()) == 7 * n
    print(f"unclamped n={n}: largest error {worst:.3f} of the bound")


# ---- 4: every request gives the bits of the full call ----
def test_every_subset_and_order_of_the_steps_gives_the_bits_of_the_full_call():
    n = 97
    mats = RD.cohort(n)
    dev = mats.to(DEV)
    thr, _ = _thresholds(dev, mats, 0.10)
    for binary in (False, True):
        full = ingest.random_walk_encodings(dev, keep=0.10, steps=8, binary=binary)
        requests = [(k,) for k in RD.STEPS] + [(8, 3), (2, 1), (5,), [4, 7, 1], 4, 2, 1, 6]
        for steps in requests:
            cols = [k - 1 for k in (steps if isinstance(steps, (tuple, list)) else range(1, steps + 1))]
            part = ingest.random_walk_encodings(dev, keep=0.10, steps=steps, binary=binary)
            assert tuple(part.shape) == (len(mats), n, len(cols))
            assert torch.equal(_bits(part), _bits(full[:, :, cols])), (steps, binary)
        # inside a wider x: the other columns keep their bits
        ids, cols = [7, 2, 0], [4, 0, 9]
        x, _ = _raw(dev, thr, ids, cols, 11, int(binary))
        assert torch.equal(_bits(x[:, :, cols]), _bits(full[:, :, ids]))
        rest = [c for c in range(11) if c not in cols]
        assert bool((_bits(x[:, :, rest]) == NAN_BITS).all()), "the columns that were not asked for"


def test_a_grid_of_three_gives_the_bits_of_the_default_grid_and_of_a_second_run():
    """12 subjects at n = 84: a grid of 3 is at most 6 workgroups, hence at least 2 subjects each, and their slabs are
    used again."""
    n = 84
    mats = torch.cat([RD.cohort(n, seed) for seed in range(2)]).contiguous()
    assert mats.shape[0] == 12
    dev = mats.to(DEV)

    def run():
        return (ingest.random_walk_encodings(dev, keep=0.1), ingest.random_walk_encodings(dev, keep=0.3, steps=(6, 2)),
                ingest.random_walk_encodings(dev, keep=0.1, binary=True))
    with K.grid_of_three():
        assert _lib.load().cgnn_ingest_rw_workspace_bytes(12, n, (ctypes.c_int32 * 1)(7), 1) == 6 * 3 * 96 * 96 * 4
    few, full = K.check_grid_of_three(run)
    alone = ingest.random_walk_encodings(RD.cohort(n).to(DEV), keep=0.1)
    assert torch.equal(_bits(full[0][:6]), _bits(alone)), "a subject's result does not depend on its cohort"
    tail = mats[6:]
    want = np.stack([RD.statement(A, t) for A, t in zip(tail, RD.host_thresholds(tail, {"keep": 0.1}))])
    _assert_within_bound(few[0][6:], want, n, "the second half at a grid of 3")


# ---- 5: composition ----
def test_knn_the_backbone_and_the_group_are_the_call_on_the_sparsified_matrices():
    n = 84
    dev = RD.cohort(n).to(DEV)
    call = ingest.random_walk_encodings
    K.check_knn(call, dev)
    K.check_backbone(call, dev)
    K.check_group(call, dev, steps=4)
    tree = call(dev, backbone="mst")
    assert not _bits(tree[:, :, 0::2]).any(), "a tree is bipartite: every odd step is +0.0"


# ---- 6: the workspace ----
def test_a_short_workspace_is_refused():
    n = 20
    mats = RD.cohort(n)
    dev = mats.to(DEV)
    thr = torch.zeros(len(mats), device=DEV)
    for ids in ([7], [4, 0], [2]):
        x, need = _raw(dev, thr, ids, list(range(len(ids))), 8, short_by=1, expect=_lib.CGNN_EINVAL)
        assert need == 6 * {7: 3, 4: 2, 2: 1}[max(ids)] * 96 * 96 * 4, "a slab set per workgroup"
        assert bool((_bits(x) == NAN_BITS).all()), "nothing was launched"
    x, need = _raw(dev, thr, [1, 0], [0, 1], 2)
    assert need == 0 and bool(torch.isfinite(x).all()), "steps up to 2 need no workspace"


# ---- 7: training ----
def test_the_eight_columns_train_on_the_fused_path():
    _, feats = K.check_trains_on_the_fused_path(lambda m: ingest.random_walk_encodings(m, keep=0.1), 8)
    assert bool((feats >= 0).all()) and bool((feats <= 1).all())


# ---- 8: an empty cohort ----
def test_no_subjects_give_an_empty_tensor_without_a_launch():
    n = 20
    K.check_no_subjects(lambda m: ingest.random_walk_encodings(m, keep=0.1, steps=(3, 1)), RD.cohort(n).to(DEV)[:0], 2)
    lib = _lib.load()
    assert lib.cgnn_ingest_rw(None, 0, n, None, (ctypes.c_int32 * 1)(7), 1, (ctypes.c_int32 * 1)(0), 1, 0, None, 0,
                              None, 0, _lib.stream_ptr()) == _lib.CGNN_OK
