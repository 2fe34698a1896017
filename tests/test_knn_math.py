"""The host statement of the k-NN sparsification (tests/knn_data.py) against a brute-force count, a hand-written
example and the consequences the module docstring lists; the public argument checks of ``ingest.knn_sparsify`` and of
``knn=`` on CPU tensors; the header and the binding of cgnn_ingest_knn.  No device is touched."""
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import ingest_data as D
from tests import knn_data as K
from tests.abi_header import check_header

NAN, INF = float("nan"), float("inf")
SIZES = (1, 2, 3, 5, 20)


@pytest.mark.parametrize("n", SIZES)
def test_the_sort_agrees_with_the_brute_force_count(n):
    for A in K.cohort(n):
        for k in range(n + 1):
            d = K.host_picks(A, k)
            assert torch.equal(d, K.brute_picks(A, k)), k
            for mode in K.MODES:
                kept = K.kept_of(A, d, mode)
                B = K.host_knn(A, k, mode)
                assert torch.equal(K.bits(B), K.bits(torch.where(kept, A, torch.zeros_like(A)))), (k, mode)
                assert not torch.isnan(B).any() and bool((B.diagonal() == 0).all())
                assert bool((K.bits(B)[~kept] == 0).all()), "a dropped entry is +0.0, never -0.0"


def test_a_hand_written_example():
    A = torch.tensor([[9.0, 0.5, 0.5, -1.0],
                      [0.5, 0.0, NAN, 0.25],
                      [0.5, 0.75, 0.0, 0.75],
                      [0.25, 0.5, 0.75, 7.0]])
    want = {
        (1, "directed"): [[0, .5, 0, 0], [.5, 0, 0, 0], [0, .75, 0, 0], [0, 0, .75, 0]],
        (1, "union"): [[0, .5, 0, 0], [.5, 0, 0, 0], [0, .75, 0, .75], [0, 0, .75, 0]],
        (1, "mutual"): [[0, .5, 0, 0], [.5, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]],
        (2, "directed"): [[0, .5, .5, 0], [.5, 0, 0, .25], [0, .75, 0, .75], [0, .5, .75, 0]],
        (2, "union"): [[0, .5, .5, 0], [.5, 0, 0, .25], [.5, .75, 0, .75], [0, .5, .75, 0]],
        (2, "mutual"): [[0, .5, 0, 0], [.5, 0, 0, .25], [0, 0, 0, .75], [0, .5, .75, 0]],
    }
    for (k, mode), rows in want.items():
        assert torch.equal(K.bits(K.host_knn(A, k, mode)), K.bits(torch.tensor(rows, dtype=torch.float32))), (k, mode)
    every = [[0, .5, .5, 0], [.5, 0, 0, .25], [.5, .75, 0, .75], [.25, .5, .75, 0]]
    both = [[0, .5, .5, 0], [.5, 0, 0, .25], [.5, 0, 0, .75], [0, .5, .75, 0]]
    for mode in K.MODES:                               # k >= n - 1: every positive off-diagonal entry, NaN and -1 gone
        # ("mutual": those whose mirror entry is positive too -- (2, 1) faces the NaN and (3, 0) the -1)
        assert torch.equal(K.host_knn(A, 3, mode), torch.tensor(both if mode == "mutual" else every)), mode
        assert torch.equal(K.bits(K.host_knn(A, 0, mode)), torch.zeros(4, 4, dtype=torch.int32)), mode


@pytest.mark.parametrize("n", SIZES)
def test_the_consequences_of_the_statement(n):
    off = ~torch.eye(n, dtype=torch.bool)
    for s, A in enumerate(K.cohort(n)):
        cand = K.candidates(A)
        p = cand.sum(1)
        for k in range(n + 2):
            d = K.host_picks(A, k)
            kept = {mode: K.kept_of(A, d, mode) for mode in K.MODES}
            want = torch.clamp(p, max=k)
            assert torch.equal(kept["directed"].sum(1), want)
            assert bool((kept["union"].sum(1) >= want).all())
            for mode in K.MODES:
                assert bool((kept[mode].sum(1) <= p).all()) and not (kept[mode] & ~cand).any()
                B = K.host_knn(A, k, mode)
                # from_matrices(B, min_weight=0.0) has exactly the edges `kept`
                ei, w = D.host_edges(B, 0.0)
                assert torch.equal(ei, torch.nonzero(kept[mode]).t()) and torch.equal(K.bits(w), K.bits(A[kept[mode]]))
                if k >= n - 1:                         # ("mutual": the mirror entry must be positive too)
                    assert torch.equal(kept[mode], cand & cand.t() if mode == "mutual" else cand)
                if k == 0:
                    assert not kept[mode].any()
                for scale in (2.0 ** -3, 2.0 ** 5):
                    if torch.isfinite(A * scale).all() and bool(((A * scale)[cand] >= 2.0 ** -126).all()):
                        assert torch.equal(K.bits(K.host_knn(A * scale, k, mode)), K.bits(B * scale)), (k, mode)
            assert not (kept["mutual"] & ~kept["directed"]).any() and not (kept["directed"] & ~kept["union"]).any()
            if torch.equal(K.bits(A), K.bits(A.t().contiguous())):
                for mode in ("union", "mutual"):
                    B = K.host_knn(A, k, mode)
                    assert torch.equal(K.bits(B), K.bits(B.t().contiguous())), (s, k, mode)
            v, c = K.last_picks(A, k)
            assert torch.equal(K.picks_from_last(A, v, c), d), (s, k)
        assert bool((off | ~K.host_picks(A, n)).all())               # the diagonal is never picked


def test_a_constant_matrix_picks_the_first_columns_past_the_diagonal():
    n, k = 20, 3
    A = D.worst_cases(n)[0]
    d = K.host_picks(A, k)
    for i in range(n):
        assert torch.nonzero(d[i]).flatten().tolist() == [j for j in range(n) if j != i][:k]
    assert not K.host_picks(D.worst_cases(n)[2], k).any()             # all negative: no picks


def _mats(n=5, S=3):
    return D.recipe(n)[:S].contiguous()


def test_knn_sparsify_checks_its_arguments_before_the_device():
    m = _mats()
    assert ingest.KNN_MODES == ("union", "mutual", "directed") and ingest.KNN_MAX_NODES == 1024
    for bad in (True, 2.0, "3", None):
        with pytest.raises(TypeError, match="k must be an int"):
            ingest.knn_sparsify(m, bad)
    with pytest.raises(ValueError, match="k must be >= 0"):
        ingest.knn_sparsify(m, -1)
    for bad in ("both", "UNION", None, 1):
        with pytest.raises(ValueError, match="unknown mode"):
            ingest.knn_sparsify(m, 2, mode=bad)
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.knn_sparsify(torch.zeros(1, 1025, 1025), 2)
    with pytest.raises(TypeError, match="float32"):
        ingest.knn_sparsify(m.double(), 2)
    with pytest.raises(ValueError, match=r"\[S, n, n\]"):
        ingest.knn_sparsify(m[:, :, :4], 2)
    with pytest.raises(ValueError, match="out must be"):
        ingest.knn_sparsify(m, 2, out=torch.empty(3, 5, 4))
    with pytest.raises(TypeError, match="out must be float32"):
        ingest.knn_sparsify(m, 2, out=torch.empty(3, 5, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be contiguous"):
        ingest.knn_sparsify(m, 2, out=torch.empty(3, 5, 5).transpose(1, 2))
    with pytest.raises(TypeError, match="out must be a torch.Tensor"):
        ingest.knn_sparsify(m, 2, out=[0.0])
    # valid arguments on CPU tensors get as far as the residency check, and no further
    for kw in (dict(), dict(mode="mutual"), dict(mode="directed", out=torch.empty_like(m)), dict(out=m.clone())):
        for k in (0, 2, 2 ** 40):
            with pytest.raises(RuntimeError, match="ROCm"):
                ingest.knn_sparsify(m, k, **kw)


def _entry_points():
    m, y = _mats(), D.labels(3)
    ts = torch.randn(6, 40, 20, generator=torch.Generator().manual_seed(4))
    return {"from_matrices": lambda **kw: ingest.from_matrices(m, y, **kw),
            "node_measures": lambda **kw: ingest.node_measures(m, **kw),
            "path_lengths": lambda **kw: ingest.path_lengths(m, **kw),
            "from_timeseries": lambda **kw: ingest.from_timeseries(ts, D.labels(6), **kw)}


@pytest.mark.parametrize("name", ["from_matrices", "node_measures", "path_lengths", "from_timeseries"])
def test_knn_is_a_fourth_choice_of_every_entry_point(name):
    call = _entry_points()[name]
    for other in (dict(keep=0.1), dict(num_edges=4), dict(min_weight=0.0)):
        with pytest.raises(ValueError, match="knn= is a fourth way"):
            call(knn=2, **other)
    with pytest.raises(ValueError, match="give exactly one of keep=, num_edges= and min_weight="):
        call()                                         # the text of the existing error stays
    with pytest.raises(ValueError, match="give knn= with it"):
        call(keep=0.1, knn_mode="mutual")
    for bad in (True, 1.5):
        with pytest.raises(TypeError, match="k must be an int"):
            call(knn=bad)
    with pytest.raises(ValueError, match="k must be >= 0"):
        call(knn=-2)
    with pytest.raises(ValueError, match="unknown mode"):
        call(knn=2, knn_mode="either")
    for kw in (dict(knn=2), dict(knn=0, knn_mode="mutual"), dict(knn=2 ** 40, knn_mode="directed"), dict(keep=0.1)):
        with pytest.raises(RuntimeError, match="ROCm"):
            call(**kw)


def test_knn_refuses_more_than_1024_nodes_in_every_matrix_entry_point():
    big = torch.zeros(1, 1025, 1025)
    for call in (lambda: ingest.from_matrices(big, D.labels(1), knn=3), lambda: ingest.node_measures(big, knn=3),
                 lambda: ingest.path_lengths(big, knn=3)):
        with pytest.raises(ValueError, match="n <= 1024"):
            call()


def test_the_prototype_matches_its_header_type_by_type():
    """cgnn_ingest_knn is declared in include/cgnn_knn.h, which cgnn.h includes, and bound by ``_lib.KNN_PROTOTYPES``:
    the return type and every argument type, the library's export, the constants, and the comparison itself against a
    doctored header."""
    hdr = check_header("cgnn_knn.h", _lib.KNN_PROTOTYPES, ["cgnn_ingest_knn"],
                       [("int64_t k, int32_t mode", "int32_t k, int32_t mode")])
    for name, value in (("CGNN_KNN_DIRECTED", 0), ("CGNN_KNN_UNION", 1), ("CGNN_KNN_MUTUAL", 2),
                        ("CGNN_KNN_MAX_NODES", 1024)):
        assert f"#define {name} {value}\n" in hdr
    assert (_lib.KNN_DIRECTED, _lib.KNN_UNION, _lib.KNN_MUTUAL) == (0, 1, 2)
    assert _lib.ABI_VERSION == 2, "the change is additive"


def test_the_entry_point_refuses_before_any_launch():
    """No device is present here: a call that went as far as a launch could not return these codes."""
    fn = _lib.load().cgnn_ingest_knn
    S, n = 3, 20
    a, b = 1 << 20, 1 << 24                            # addresses that nothing dereferences
    nbytes = 4 * S * n * n
    good = [a, S, n, 4, _lib.KNN_UNION, b, nbytes, None]

    def rc(at, v):
        return fn(*(good[:at] + [v] + good[at + 1:]))

    for at, v in ((0, None), (5, None), (0, a + 2), (5, b + 1), (1, -1), (2, 0), (2, -5), (3, -1), (4, 3), (4, -1),
                  (6, nbytes - 1), (1, 2 ** 31 // n + 1), (5, a + 4 * n * n), (5, a - 4), (5, a + nbytes - 4)):
        assert rc(at, v) == _lib.CGNN_EINVAL, (at, v)
    assert rc(2, 1025) == _lib.CGNN_EUNSUPPORTED
    assert fn(a, S, 1025, 4, 7, b, 0, None) == _lib.CGNN_EINVAL       # a bad value comes before an unsupported shape
    assert rc(1, 0) == _lib.CGNN_OK and fn(None, 0, n, 4, _lib.KNN_MUTUAL, None, 0, None) == _lib.CGNN_OK
