"""CPU tests of what lets hyper-parameters change under captured steps: the packing of the device table
(optim.hyper_rows), the validation that runs before every upload (optim.check_hyper, refresh_hyper), the snapshot a
captured step keeps of a foreign optimizer's param groups (graphed.hyper_snapshot / hyper_changed), and the C ABI of
the entry that reads the table (include/cgnn_optim.h, _lib.OPTIM_PROTOTYPES).  No device is touched."""
import ctypes
import math

import pytest
import torch

from connectome_gnn_amd import _lib, graphed, optim
from tests.abi_header import check_header


def _params(n=2):
    return [torch.zeros(3, requires_grad=True) for _ in range(n)]


# ---- the table as a pure function of param_groups ---------------------------------------------------------------------
def test_hyper_rows_are_the_groups_in_order_as_doubles():
    a, b = _params()
    opt = optim.Adam([{"params": [a], "lr": 1e-2, "betas": (0.8, 0.99), "weight_decay": 1e-4},
                      {"params": [b], "lr": 3e-4, "betas": (0.5, 0.9), "eps": 1e-6, "weight_decay": 0.25}])
    rows = optim.hyper_rows(opt.param_groups)
    assert rows == [(1e-2, 0.8, 0.99, 1e-8, 1e-4), (3e-4, 0.5, 0.9, 1e-6, 0.25)]
    assert all(type(v) is float for row in rows for v in row)
    # doubles, not floats: 1e-2 survives exactly (float32(1e-2) != 1e-2)
    assert rows[0][0] == 1e-2 != float(torch.tensor(1e-2, dtype=torch.float32))
    # a tensor-valued lr is read with float(); plain dicts will do (pure function of the groups)
    assert optim.hyper_rows([{"lr": torch.tensor(0.5), "betas": (0, 0.5), "eps": 0, "weight_decay": 0}]) \
        == [(0.5, 0.0, 0.5, 0.0, 0.0)]
    opt.param_groups[1]["lr"] = 7.0
    assert optim.hyper_rows(opt.param_groups)[1][0] == 7.0 and optim.hyper_rows(opt.param_groups)[0] == rows[0]
    assert optim.AdamW(_params()).param_groups[0]["weight_decay"] == 1e-2          # torch's default
    assert _lib.ADAM_HYPER_STRIDE == 8


BAD = [("lr", -1e-3), ("lr", math.nan), ("lr", math.inf), ("betas", (1.0, 0.999)), ("betas", (0.9, 1.0)),
       ("betas", (-0.1, 0.999)), ("betas", (math.nan, 0.5)), ("eps", -1e-8), ("eps", math.nan),
       ("weight_decay", -1e-2), ("weight_decay", math.nan), ("weight_decay", math.inf)]


@pytest.mark.parametrize("key,value", BAD)
def test_refused_values_raise_before_anything_is_uploaded(key, value):
    """check_hyper refuses what cgnn_adam_step answers with CGNN_EINVAL, plus a negative or non-finite lr or
    weight_decay; refresh_hyper runs it before it looks for a device (these parameters live on the CPU: an upload
    would be a TypeError, a launch impossible), and step() goes through refresh_hyper."""
    good = {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0}
    optim.check_hyper(optim.hyper_rows([good]))
    with pytest.raises(ValueError, match="param group 0"):
        optim.check_hyper(optim.hyper_rows([{**good, key: value}]))
    for cls in (optim.Adam, optim.AdamW):
        opt = cls(_params())
        opt.param_groups[0][key] = value
        with pytest.raises(ValueError):
            opt.refresh_hyper()
        assert opt._hyper is None and opt._hyper_host is None
    # the second group is checked too, and named
    with pytest.raises(ValueError, match="param group 1"):
        optim.check_hyper(optim.hyper_rows([good, {**good, key: value}]))


def test_the_by_value_entry_refuses_the_same_values():
    """cgnn_adam_step's own refusals (CGNN_EINVAL before any launch: no device here) are a subset of check_hyper's."""
    lib = _lib.load()
    jb = _lib.CgnnAdamJobs()
    jb.n = 1
    jb.numel[0], jb.param[0], jb.grad[0], jb.exp_avg[0], jb.exp_avg_sq[0] = 0, 4096, 4096, 4096, 4096
    for lr, b1, b2, eps in ((-1.0, 0.9, 0.999, 1e-8), (math.nan, 0.9, 0.999, 1e-8), (1e-3, 1.0, 0.999, 1e-8),
                            (1e-3, 0.9, 1.0, 1e-8), (1e-3, 0.9, 0.999, -1.0)):
        assert lib.cgnn_adam_step(jb, 4096, 4096, 1, lr, b1, b2, eps, 0.0, None) == _lib.CGNN_EINVAL
        with pytest.raises(ValueError):
            optim.check_hyper([(lr, b1, b2, eps, 0.0)])


# ---- the snapshot of a foreign optimizer's param groups ------------------------------------------------------------------
def _groups():
    a, b = _params()
    return torch.optim.Adam([{"params": [a], "lr": 1e-2}, {"params": [b], "lr": torch.tensor(1e-3), "foreach": False}],
                            betas=(0.9, 0.999), weight_decay=0.0).param_groups


def test_snapshot_compare():
    groups = _groups()
    snap = graphed.hyper_snapshot(groups)
    assert all("params" not in g for g in snap) and set(snap[0]) == set(groups[0]) - {"params"}
    assert graphed.hyper_changed(snap, groups) is None                            # equal groups are current
    assert graphed.hyper_changed(snap, [dict(g) for g in groups]) is None         # (by value, not by identity)
    groups[0]["lr"] = 5e-3                                                        # a changed float
    assert graphed.hyper_changed(snap, groups) == "param_groups[0]['lr']"
    groups[0]["lr"] = 1e-2
    assert graphed.hyper_changed(snap, groups) is None
    groups[1]["betas"] = (0.9, 0.99)                                              # a changed entry of the betas tuple
    assert graphed.hyper_changed(snap, groups) == "param_groups[1]['betas']"
    groups[1]["betas"] = (0.9, 0.999)
    assert graphed.hyper_changed(snap, groups) is None
    kept = groups[1]["lr"]
    groups[1]["lr"] = kept.clone()                                                # a replaced tensor (equal value)
    assert graphed.hyper_changed(snap, groups) == "param_groups[1]['lr']"
    groups[1]["lr"] = kept
    assert graphed.hyper_changed(snap, groups) is None
    kept.mul_(0.5)                                                                # a tensor edited in place
    assert graphed.hyper_changed(snap, groups) == "param_groups[1]['lr']"
    snap = graphed.hyper_snapshot(groups)
    assert graphed.hyper_changed(snap, groups) is None
    groups[0]["lr"] = torch.tensor(1e-2)                                          # a float that became a tensor
    assert graphed.hyper_changed(snap, groups) == "param_groups[0]['lr']"
    groups[0]["lr"] = 1e-2
    groups[0]["params"] = groups[0]["params"] + _params(1)                        # "params" is ignored
    assert graphed.hyper_changed(snap, groups) is None
    groups[0]["weight_decay"] = None                                              # None, bools: by equality
    assert graphed.hyper_changed(snap, groups) == "param_groups[0]['weight_decay']"
    groups[0]["weight_decay"] = 0.0
    groups[1]["amsgrad"] = True
    assert graphed.hyper_changed(snap, groups) == "param_groups[1]['amsgrad']"
    groups[1]["amsgrad"] = False
    groups[1]["new_key"] = 1                                                      # a key that appeared / went away
    assert graphed.hyper_changed(snap, groups) == "param_groups[1]['new_key']"
    del groups[1]["new_key"], groups[1]["eps"]
    assert graphed.hyper_changed(snap, groups) == "param_groups[1]['eps']"
    assert graphed.hyper_changed(snap, groups[:1]) == "len(param_groups)"


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_the_prototype_matches_its_header_type_by_type():
    """cgnn_adam_step_dev is declared in include/cgnn_optim.h, which cgnn.h includes (the butterworth entries' layout:
    tests/test_host_logic.py pins the row count of _lib.PROTOTYPES), bound by _lib.OPTIM_PROTOTYPES and exported; the
    by-value entry keeps its row; the ABI version is unchanged."""
    hdr = check_header("cgnn_optim.h", _lib.OPTIM_PROTOTYPES, ["cgnn_adam_step_dev"],
                       [("int32_t decoupled", "int64_t decoupled")])
    assert "#define CGNN_ADAM_HYPER_STRIDE 8" in hdr
    lib = _lib.load()
    assert _lib.PROTOTYPES["cgnn_adam_step"] == (ctypes.c_int, [ctypes.POINTER(_lib.CgnnAdamJobs), _lib.P, _lib.P, _lib.I32]
                                                 + [_lib.F64] * 5 + [_lib.P])
    assert _lib.ABI_VERSION == 2 and lib.cgnn_abi_version() == 2, "the change is additive"


def test_the_entry_refuses_pointers_and_jobs_before_any_launch():
    """No device is present here: a call that went as far as a launch could not return CGNN_EINVAL for these."""
    lib = _lib.load()

    def jobs(n=1, numel=0, param=4096):
        jb = _lib.CgnnAdamJobs()
        jb.n = n
        for i in range(max(0, min(n, _lib.ADAM_MAX_JOBS))):
            jb.numel[i], jb.param[i], jb.grad[i], jb.exp_avg[i], jb.exp_avg_sq[i] = numel, param, 4096, 4096, 4096
        return jb

    good = [jobs(), 4096, 4096, 1, 8192, 0, None]
    for at, bad in ((0, jobs(0)), (0, jobs(_lib.ADAM_MAX_JOBS + 1)), (0, jobs(numel=-1)), (0, jobs(param=None)),
                    (1, None), (2, None), (4, None), (4, 8196), (5, 2), (5, -1)):
        args = good[:at] + [bad] + good[at + 1:]
        assert lib.cgnn_adam_step_dev(*args) == _lib.CGNN_EINVAL, (at, bad)
