"""The edge choice of the matrix entry points, without a device: ``from_matrices``, ``node_measures``,
``module_profile``, ``centrality_measures``, ``path_lengths`` and ``from_timeseries`` validate ``keep=`` / ``num_edges=``
/ ``min_weight=`` / ``knn=`` / ``knn_mode=`` / ``backbone=`` with one function, so each bad choice
is refused by all six with the same exception, and before any later argument is looked at.  The expected texts are
literals recorded from the commit before the entry points shared that function: they are the yardstick, not the code
under test.  Every case raises before the residency check, so no library is needed."""
import pytest
import torch

from connectome_gnn_amd import ingest

NAN = float("nan")
ONE_OF = "give exactly one of keep=, num_edges= and min_weight="
KNN_SIZE = "k-NN sparsification takes n <= 1024 nodes (a row lives in 16 registers per lane), got n = 1025"
MST_SIZE = "the spanning-tree backbone takes n <= 1024 nodes (a lane owns 4 nodes of the tree phase), got n = 1025"

# (the choice, the exception, its whole text; {unit} is the letter that names the unit: S, or U for time series)
BAD_CHOICES = {
    "none of the four": (dict(), ValueError, ONE_OF),
    "keep with num_edges": (dict(keep=0.1, num_edges=3), ValueError, ONE_OF),
    "keep above 1": (dict(keep=1.5), ValueError, "keep must lie in [0, 1], got 1.5"),
    "keep nan": (dict(keep=NAN), ValueError, "keep must lie in [0, 1], got nan"),
    "num_edges negative": (dict(num_edges=-1), ValueError, "num_edges must be >= 0, got -1"),
    "num_edges a bool": (dict(num_edges=True), TypeError, "num_edges must be an int, got bool"),
    "min_weight tensor of the wrong length": (
        dict(min_weight=torch.zeros(3)), ValueError,
        "a min_weight tensor must be floating point [{unit}] = [2], got torch.float32 (3,)"),
    "min_weight tensor of integers": (
        dict(min_weight=torch.zeros(2, dtype=torch.int64)), ValueError,
        "a min_weight tensor must be floating point [{unit}] = [2], got torch.int64 (2,)"),
    "knn with keep": (dict(knn=3, keep=0.1), ValueError,
                      "knn= is a fourth way to choose the edges: give none of keep=, num_edges= and min_weight= with it"),
    "knn_mode without knn": (dict(knn_mode="mutual"), ValueError,
                             "knn_mode='mutual' says how the picks of knn= are symmetrised: give knn= with it"),
    "knn negative": (dict(knn=-1), ValueError, "k must be >= 0, got -1"),
    "knn a string": (dict(knn="3"), TypeError, "k must be an int, got str"),
    "knn_mode unknown": (dict(knn=3, knn_mode="both"), ValueError,
                         "unknown mode 'both': the modes are KNN_MODES = ('union', 'mutual', 'directed')"),
    "backbone unknown": (dict(backbone="tree", keep=0.1), ValueError,
                         "unknown backbone 'tree': the backbones are BACKBONES = ('mst',)"),
    "backbone with two thresholds": (dict(backbone="mst", keep=0.1, num_edges=3), ValueError,
                                     "the backbone is united with at most one of keep=, num_edges= and min_weight="),
    "knn beyond its size": (dict(knn=3), ValueError, KNN_SIZE),
    "backbone beyond its size": (dict(backbone="mst"), ValueError, MST_SIZE),
}
LARGE = ("knn beyond its size", "backbone beyond its size")

SMALL_DATA = dict(matrices=torch.zeros(2, 6, 6), timeseries=torch.zeros(2, 12, 6), labels=torch.zeros(2, dtype=torch.long))
LARGE_DATA = dict(matrices=torch.zeros(1, 1025, 1025), timeseries=torch.zeros(1, 1025, 1025),
                  labels=torch.zeros(1, dtype=torch.long))

# name -> (the call on the data above, the unit's letter)
ENTRY_POINTS = {
    "from_matrices": (lambda d, **kw: ingest.from_matrices(d["matrices"], d["labels"], **kw), "S"),
    "node_measures": (lambda d, **kw: ingest.node_measures(d["matrices"], **kw), "S"),
    "module_profile": (lambda d, **kw: ingest.module_profile(
        d["matrices"], kw.pop("modules", [0] * d["matrices"].shape[1]), **kw), "S"),
    "centrality_measures": (lambda d, **kw: ingest.centrality_measures(d["matrices"], **kw), "S"),
    "path_lengths": (lambda d, **kw: ingest.path_lengths(d["matrices"], **kw), "S"),
    "from_timeseries": (lambda d, **kw: ingest.from_timeseries(d["timeseries"], d["labels"], **kw), "U"),
}


def _raised(call, data, **kw):
    with pytest.raises(Exception) as info:
        call(data, **kw)
    return type(info.value), str(info.value)


@pytest.mark.parametrize("case", list(BAD_CHOICES))
def test_a_bad_edge_choice_is_refused_alike(case):
    choice, kind, text = BAD_CHOICES[case]
    data = LARGE_DATA if case in LARGE else SMALL_DATA
    for name, (call, unit) in ENTRY_POINTS.items():
        assert _raised(call, data, **choice) == (kind, text.format(unit=unit)), name


# a later argument that is bad too, per entry point, and what it raises on its own with a good choice (from the same
# commit: the check below would pass vacuously if these were not refused at all)
LATER = {
    "from_matrices": [
        (dict(measures=("degree", "modularity")), ValueError, "unknown measure 'modularity': the measures are "),
        (dict(modules=[0, 0, 0, 1, 1, 1]), ValueError, "modules= was given but no measure of MODULE_MEASURES = "),
        (dict(labels=torch.zeros(3, dtype=torch.long)), ValueError, "labels must be an int64 tensor [S] = [2]"),
    ],
    "node_measures": [
        (dict(measures=("degree", "modularity")), ValueError, "unknown measure 'modularity': the measures are "),
        (dict(modules=[0, 0, 0, 1, 1, 1]), ValueError, "modules= was given but no measure of MODULE_MEASURES = "),
    ],
    "module_profile": [
        (dict(modules=[0, 0, 1]), ValueError, "modules must be [n] = [6] labels, one per ROI, got (3,)"),
    ],
    "centrality_measures": [
        (dict(measures=("eigenvector",)), ValueError, "unknown measure 'eigenvector': the centrality measures are "
                                                      "('pagerank', 'weighted_pagerank')"),
        (dict(damping=2), ValueError, "damping must lie in [0, 0.99], got 2"),
    ],
    "from_timeseries": [
        (dict(labels=torch.zeros(3, dtype=torch.long)), ValueError, "labels must be an int64 tensor [S] = [2]"),
    ],
}
# from_timeseries looks at its measures before its edges (and always did): there the later argument wins
EARLIER = {
    "from_timeseries": [
        (dict(measures=("degree", "modularity")), ValueError, "unknown measure 'modularity': the measures are "),
        (dict(modules=[0, 0, 0, 1, 1, 1]), ValueError, "modules= was given but no measure of MODULE_MEASURES = "),
    ],
}
PRECEDENCE_CHOICES = ("none of the four", "keep above 1", "knn with keep", "knn_mode unknown", "backbone unknown",
                      "backbone with two thresholds")


def _call_with(name, later, **choice):
    data = dict(SMALL_DATA)
    later = dict(later)
    if "labels" in later:
        data["labels"] = later.pop("labels")
    return _raised(ENTRY_POINTS[name][0], data, **later, **choice)


@pytest.mark.parametrize("name", list(LATER))
def test_the_edge_choice_is_refused_before_a_later_argument(name):
    for later, kind, text in LATER[name]:
        got = _call_with(name, later, keep=0.2)
        assert got[0] is kind and got[1].startswith(text), (name, later, got)
        for case in PRECEDENCE_CHOICES:
            choice, want_kind, want_text = BAD_CHOICES[case]
            assert _call_with(name, later, **choice) == (want_kind, want_text), (name, later, case)


def test_from_timeseries_keeps_its_own_order():
    for later, kind, text in EARLIER["from_timeseries"]:
        for case in PRECEDENCE_CHOICES:
            got = _call_with("from_timeseries", later, **BAD_CHOICES[case][0])
            assert got[0] is kind and got[1].startswith(text), (later, case, got)
