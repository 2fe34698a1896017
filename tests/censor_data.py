"""The host statement of frame censoring (``sample_mask=`` of ``connectome_gnn_amd.ingest``) by
compaction, and the seeded masks its tests share.

Statement: take a subject's kept rows, apply the existing host statements to them -- ``confound_data.host_basis`` /
``host_regress`` on ``[fl32 cosines | confounds][K]``, ``timeseries_data.host_unit`` on a unit's kept rows,
``shrinkage_data.host_lw`` on them -- and scatter the result back with zeros at the censored frames.  Nothing here
knows how the device does it.

Masks: one kind per subject, cycling through ``KINDS``; where a kind is random its seed is ``9000 + s``.
"""
import functools

import torch

from tests import confound_data as D
from tests import filter_data as F
from tests import shrinkage_data as W
from tests import timeseries_data as TS

EPS = F.EPS
KINDS = ("all", "ends", "random", "phase", "head32", "block8", "few", "two", "one", "none")
S = len(KINDS)                                    # every kind occurs once
# (T, n, q, t_r, high_pass) on confound_data.frames / confounds
REGRESSION_CASES = [
    (9, 5, 5, 1.0, 0.1),
    (33, 65, 24, 2.0, 0.01),
    (67, 97, 33, 0.72, 0.05),                     # 4 cosines, 37 columns, qpad 64
    (130, 84, 32, 0.72, 0.01),
    (300, 360, 24, 2.0, 0.008),                   # 9 cosines
    (300, 72, 64, None, None),
]
# (T, n, window, stride) on timeseries_data.planted
CONNECTIVITY_CASES = [
    (9, 5, None, None),
    (33, 65, 8, 4),                               # head32 empties whole windows
    (67, 97, None, None),
    (130, 84, 50, 25),
    (300, 360, None, None),
]


def mask_of(kind, T, s):
    """bool [T], True = kept: the mask of ``kind`` for subject ``s`` of a ``T``-frame run."""
    g = torch.Generator().manual_seed(9000 + s)
    t = torch.arange(T)
    keep = torch.ones(T, dtype=torch.bool)
    if kind == "ends":
        keep[0] = keep[T - 1] = False
    elif kind == "random":
        keep = torch.rand(T, generator=g) < 0.7
        keep[T - 1] = False
    elif kind == "phase":                         # a whole wave's share of the frames
        keep = t % 4 != 1
    elif kind == "head32":                        # a whole step
        keep = t >= min(32, T - 1)
    elif kind == "block8":                        # one thread's whole block of 8: t = 2, 6, .., 30
        keep = ~((t % 4 == 2) & (t <= 30))
    elif kind == "few":
        keep = torch.zeros(T, dtype=torch.bool)
        keep[torch.randperm(T, generator=g)[:20]] = True
    elif kind == "two":
        keep = torch.zeros(T, dtype=torch.bool)
        keep[T // 3] = keep[(2 * T) // 3] = True
    elif kind == "one":
        keep = torch.zeros(T, dtype=torch.bool)
        keep[T // 2] = True
    elif kind == "none":
        keep = torch.zeros(T, dtype=torch.bool)
    else:
        assert kind == "all", kind
    return keep


@functools.lru_cache(maxsize=None)
def masks(num, T):
    """bool [num, T] (host, shared between tests: do not modify): subject s has kind ``KINDS[s % 10]``."""
    return torch.stack([mask_of(KINDS[s % len(KINDS)], T, s) for s in range(num)]).contiguous()


def dropped_components(T, t_r, high_pass):
    """The components a high-pass drops, ascending (none without one)."""
    if high_pass is None:
        return []
    return list(range(1, F.components(T, t_r, high_pass, None)[0]))


def host_design(c, T, t_r, high_pass):
    """float32 [T, K + q]: [fl32(b_k[t]) for the dropped components | the confounds c [T, q] (None: none)]."""
    cols = []
    comps = dropped_components(T, t_r, high_pass)
    if comps:
        cols.append(F.basis(T, comps).float())
    if c is not None:
        cols.append(c)
    return torch.cat(cols, 1).contiguous() if cols else None


def host_basis(d, keep):
    """The masked basis of one subject's design d [T, q]: (Q float64 [T, q] with zero rows at censored frames, kept, piv)
    of ``confound_data.host_basis`` on the kept rows; no kept row keeps no column."""
    T, q = d.shape
    Q = torch.zeros(T, q, dtype=torch.float64)
    if not bool(keep.any()):
        return Q, [False] * q, [float("nan")] * q
    Qk, kept, piv = D.host_basis(d[keep])
    Q[keep] = Qk
    return Q, kept, piv


def host_centred(x, keep):
    """float64 [T, n]: x minus its column means over the kept frames there, zeros elsewhere."""
    out = torch.zeros(x.shape, dtype=torch.float64)
    if bool(keep.any()):
        out[keep] = F.centred(x[keep])
    return out


def host_regress(x, d, keep):
    """The statement for one subject: float64 [T, n]; d None is masked centring."""
    if d is None:
        return host_centred(x, keep)
    out = torch.zeros(x.shape, dtype=torch.float64)
    if bool(keep.any()):
        out[keep] = D.host_regress(x[keep], d[keep])
    return out


def host_regress32(x, d, keep):
    """The statement on the operands the device holds (``confound_data.host_regress32`` on the kept rows): float32."""
    out = torch.zeros(x.shape, dtype=torch.float32)
    if bool(keep.any()):
        out[keep] = D.host_regress32(x[keep], d[keep])
    return out


def column_ratios(got, x, d, keep):
    """Per column of one subject: max_t |got - host_regress| / (2^-24 max_K |xc|), float64 [n]; a column whose xc is all
    zero (constant on the kept frames, or fewer than two of them) must be matched exactly: 0 if it is, inf if not."""
    scale = host_centred(x, keep).abs().max(0).values
    err = (got.double() - host_regress(x, d, keep)).abs().max(0).values
    flat = scale == 0
    r = err / (EPS * torch.where(flat, torch.ones_like(scale), scale))
    return torch.where(flat & (err > 0), torch.full_like(r, float("inf")), r)


def regression_subjects(case):
    """(x [T, n], design [T, K + q], keep [T], kind) of every subject of a regression case"""
    T, n, q, t_r, hp = case
    x, c, m = D.frames(S, T, n, q), D.confounds(S, T, q), masks(S, T)
    return [(x[s], host_design(c[s], T, t_r, hp), m[s], KINDS[s]) for s in range(S)]


def worst_host32_ratio():
    """(the largest ratio of ``host_regress32`` over the regression cases, subjects and columns, where it is met)"""
    worst, at = 0.0, None
    for case in REGRESSION_CASES:
        for x, d, keep, kind in regression_subjects(case):
            r = float(column_ratios(host_regress32(x, d, keep), x, d, keep).max())
            if r > worst:
                worst, at = r, (case, kind)
    return worst, at


# ---- connectivity ------------------------------------------------------------------------------------------------------
def units(ts, keep, window=None, stride=None):
    """The kept rows [L_u, n] of every unit of ts [S, T, n] under keep [S, T], units as in ``timeseries_data``."""
    num, T, _ = ts.shape
    L = T if window is None else window
    st = L if stride is None else stride
    return [ts[s, w * st:w * st + L][keep[s, w * st:w * st + L]]
            for s in range(num) for w in range(TS.num_windows(T, window, stride))]


def host_unit(x, absolute=False):
    """``timeseries_data.host_unit`` of the kept rows x [L_u, n]; fewer than two rows give the all-zero matrix."""
    n = x.shape[1]
    return torch.zeros(n, n, dtype=torch.float64) if x.shape[0] < 2 else TS.host_unit(x, absolute)


def unit_kappa(x):
    """max |m_i| / std_i over the columns of the kept rows that are not constant (0 if there is none)"""
    return TS.kappa(x[None]) if x.shape[0] >= 2 else 0.0


def host_lw(x):
    """``shrinkage_data.host_lw`` of the kept rows; L_u <= 2 gives exactly 0 (a NaN stays a NaN at L_u == 2)."""
    return 0.0 if x.shape[0] < 2 else W.host_lw(x)


def host_lw32(x):
    return 0.0 if x.shape[0] < 2 else W.host_lw32(x)


def cond(x):
    return 0.0 if x.shape[0] < 2 else W.cond(x)


def connectivity_units(case):
    T, n, window, stride = case
    return units(TS.planted(S, T, n), masks(S, T), window, stride)


def worst_lw32_ratio():
    """The largest |host_lw32 - host_lw| / (2^-24 cond) over the units of the connectivity cases (n <= 1024)."""
    worst = 0.0
    for case in CONNECTIVITY_CASES:
        for x in connectivity_units(case):
            k = cond(x)
            if k > 0.0:
                worst = max(worst, abs(host_lw32(x) - host_lw(x)) / (EPS * k))
    return worst
