"""The one family runner against the headers: ``ingest._run_family`` builds the argument list of
every measure-shaped C call from the family and three extra argument tuples.  Each public call that uses an extra
slot is compared, bit for bit, with one direct ``_lib.call`` whose arguments are written out in the order of its
header, into NaN-filled outputs: a slot in the wrong place gives other bits or a refused call."""
import ctypes

import pytest
import torch

from connectome_gnn_amd import _lib, ingest

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, N, KEEP = 3, 68, 0.2


@pytest.fixture(scope="module")
def cohort():
    """A seeded symmetric cohort with one NaN, one subject without a positive entry, and its thresholds."""
    g = torch.Generator().manual_seed(68)
    m = torch.rand(S, N, N, generator=g) - 0.3
    m = ((m + m.transpose(1, 2)) / 2).contiguous()
    m[0, 3, 7] = float("nan")
    m[1] = -m[1].abs()
    m = m.to(DEV)
    return m, ingest.select_thresholds(m, keep=KEEP)


def _nans(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _ids(*ids):
    return (ctypes.c_int32 * len(ids))(*ids), len(ids)


def _same_bits(got, want):
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_centrality_measures_is_the_direct_pagerank_call(cohort):
    m, thr = cohort
    x = _nans(S, N, 2)
    cols, ldx = _ids(0, 1)
    _lib.call("cgnn_ingest_pagerank", m, S, N, thr, *_ids(1, 0), cols, ldx, 0.5, None, 0, *_lib.buf(x), None, 0)
    got = ingest.centrality_measures(m, keep=KEEP, measures=("weighted_pagerank", "pagerank"), damping=0.5)
    _same_bits(got, x)
    assert not bool(torch.isnan(x).any())
    default = ingest.centrality_measures(m, keep=KEEP, measures=("weighted_pagerank", "pagerank"))
    assert not torch.equal(default, got), "the damping reaches the kernel"


def test_module_profile_is_the_direct_modules_call(cohort):
    m, thr = cohort
    M = 3
    labels = torch.arange(N, dtype=torch.int32) % M
    profile = _nans(S, N, M)
    flags = _lib.MODULE_PROFILE_BINARY | _lib.MODULE_PROFILE_NORMALIZE
    _lib.call("cgnn_ingest_modules", m, S, N, thr, labels.to(DEV), M, None, 0, None, 1, None, 0, None, 0,
              *_lib.buf(profile), flags)
    _same_bits(ingest.module_profile(m, labels, keep=KEEP, binary=True, normalize=True), profile)
    assert not bool(torch.isnan(profile).any())


def test_path_lengths_is_the_direct_wpaths_call(cohort):
    m, thr = cohort
    need = _lib.load().cgnn_ingest_wpaths_workspace_bytes(S, N, None, 0)
    assert need > 0
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    dist = _nans(S, N, N)
    _lib.call("cgnn_ingest_wpaths", m, S, N, thr, None, 0, None, 1, *_lib.buf(work), None, 0, *_lib.buf(dist))
    _same_bits(ingest.path_lengths(m, keep=KEEP), dist)
    assert not bool(torch.isnan(dist).any())
