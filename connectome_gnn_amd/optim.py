"""torch.optim.Adam / AdamW whose update is ONE HIP launch (csrc/adam.hip: ``cgnn_adam_step_dev``, ``cgnn_adam_step``).

Same algorithm, hyper-parameters, ``param_groups`` and ``state_dict`` layout (``step``, ``exp_avg``,
``exp_avg_sq`` per parameter) as ``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` -- what the
reference's demo trains with (demo.py:105-134) -- so it drops into ``Trainer(model, optimizer)``
and checkpoints interchange.  torch's fused multi-tensor Adam is two launches per step and takes
7-43 us for these models' 15 k - 400 k parameters; this is one launch of 5-8 us, and it is
graph-capturable (the step counter lives on the device and is advanced by the same launch).

The hyper-parameters live on the device too: one ``[G, 8]`` float64 table, a row
``{lr, beta1, beta2, eps, weight_decay, 0, 0, 0}`` per param group, which the launch reads when it RUNS.  A captured
step therefore follows a learning-rate schedule (``torch.optim.lr_scheduler.*``, a manual ``param_groups[i]["lr"] =``,
a weight-decay change): ``refresh_hyper()`` -- called by ``step()`` and by the captured steps of graphed.py before they
replay -- compares the groups' Python values with what the table holds and, only when they differ, validates them and
rewrites the table with one stream-ordered copy.  It cannot do that while a stream is capturing (the copy would be
recorded into the step graph with that moment's values): a stale table then raises.  An eager ``Adam.step()`` hands
the same values to ``cgnn_adam_step`` by value instead (equal bits, a slightly shorter launch); every recorded launch,
and every AdamW launch, is ``cgnn_adam_step_dev``.

Restrictions (checked): fp32 CUDA parameters with dense contiguous gradients, no amsgrad /
maximize / differentiable.  All parameters of the optimizer step together and share one step
counter (``state[p]['step']`` is the same 0-dim fp32 device tensor for every parameter).
"""
from __future__ import annotations

import math

import torch

from . import _lib


def hyper_rows(param_groups) -> list:
    """The table as the host states it: per param group, in order, ``(lr, beta1, beta2, eps, weight_decay)`` as Python
    floats (doubles).  Pure: no device, no validation.  (A tensor-valued ``lr`` is read with ``float()``.)"""
    return [(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
            for g in param_groups]


def check_hyper(rows) -> None:
    """ValueError for a row that ``cgnn_adam_step`` answers with CGNN_EINVAL (lr < 0, a beta outside [0, 1), eps < 0;
    NaN fails each) and for an ``lr`` or ``weight_decay`` that is negative or not finite.  The launch that reads the
    table cannot check: this runs before every upload."""
    for gi, (lr, b1, b2, eps, wd) in enumerate(rows):
        if not (lr >= 0.0 and math.isfinite(lr)):
            raise ValueError(f"param group {gi}: invalid learning rate {lr}")
        if not 0.0 <= b1 < 1.0:
            raise ValueError(f"param group {gi}: invalid beta parameter at index 0: {b1}")
        if not 0.0 <= b2 < 1.0:
            raise ValueError(f"param group {gi}: invalid beta parameter at index 1: {b2}")
        if not eps >= 0.0:
            raise ValueError(f"param group {gi}: invalid epsilon value {eps}")
        if not (wd >= 0.0 and math.isfinite(wd)):
            raise ValueError(f"param group {gi}: invalid weight_decay value {wd}")


class _OneLaunch:
    """What Adam and AdamW below share; in front of the torch class in their bases."""

    def _init_one_launch(self):
        self._shared_step = None
        self._arrivals = None
        self._plan = None                 # (key, [(jobs struct, group index), ...], keepalive)
        self._hyper = None                # [G, 8] float64 on the parameters' device
        self._hyper_host = None           # hyper_rows() of what the table holds (or will, in stream order)
        self._hyper_src = None            # the host tensor of the last upload, kept until the next one

    # ---- hyper-parameters
    def _device(self):
        for grp in self.param_groups:
            for p in grp["params"]:
                return p.device
        return None

    def refresh_hyper(self) -> bool:
        """Bring the device table up to the param groups' current values: nothing is issued when they are what the
        table holds; else they are validated (ValueError) and uploaded by ONE copy on the current stream, which
        orders it before every launch issued -- and every graph replayed -- on that stream afterwards.  RuntimeError
        while the current stream is capturing.  True if a copy was issued."""
        rows = hyper_rows(self.param_groups)
        if rows == self._hyper_host:
            return False
        check_hyper(rows)
        dev = self._device()
        if dev is None or dev.type != "cuda":
            raise TypeError(f"connectome_gnn_amd.{type(self).__name__} needs contiguous float32 CUDA parameters")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(
                f"connectome_gnn_amd.{type(self).__name__}: hyper-parameters changed and the device table is stale "
                "while a stream is capturing; a copy from host memory must not be recorded into a step graph.  Call "
                "refresh_hyper() before the capture begins.")
        # a fresh pageable tensor per upload (changes are rare): a reused pinned buffer could be overwritten
        # before an earlier copy has run
        src = torch.zeros(len(rows), _lib.ADAM_HYPER_STRIDE, dtype=torch.float64)
        src[:, :5] = torch.tensor(rows, dtype=torch.float64)
        if self._hyper is None or self._hyper.shape[0] != len(rows) or self._hyper.device != dev:
            self._hyper = torch.empty(len(rows), _lib.ADAM_HYPER_STRIDE, dtype=torch.float64, device=dev)
        self._hyper.copy_(src, non_blocking=True)
        self._hyper_src, self._hyper_host = src, rows
        return True

    # ---- state
    def _ensure_state(self):
        dev = None
        name = type(self).__name__
        for grp in self.param_groups:
            if grp.get("amsgrad") or grp.get("maximize") or grp.get("differentiable"):
                raise ValueError(f"connectome_gnn_amd.{name}: amsgrad / maximize / differentiable are not supported")
            for p in grp["params"]:
                if p.grad is None:
                    continue
                if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                    raise TypeError(f"connectome_gnn_amd.{name} needs contiguous float32 CUDA parameters")
                dev = p.device
        if dev is None:
            return None
        if self._shared_step is None:
            # adopt a loaded state_dict's counter if there is one (all parameters step together)
            init = 0.0
            for st in self.state.values():
                if "step" in st:
                    init = float(st["step"])
                    break
            self._shared_step = torch.full((), init, dtype=torch.float32, device=dev)
            self._arrivals = torch.zeros(1, dtype=torch.int32, device=dev)
        for grp in self.param_groups:
            for p in grp["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] = self._shared_step
        return dev

    def state_dict(self):
        """torch's layout with a PRIVATE 0-dim ``step`` per parameter: the shared device counter is
        an internal of this class, and exporting it aliased would make a torch.optim.Adam that
        loads the checkpoint bump one counter once per parameter each step."""
        sd = super().state_dict()
        sd["state"] = {k: {n: (v.clone() if n == "step" and torch.is_tensor(v) else v) for n, v in st.items()}
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._shared_step = None          # re-adopt the loaded counter at the next step
        self._plan = None                 # (the loaded groups' hyper-parameters reach the table at the next refresh)

    def _build_plan(self):
        key, launches, keep = [], [], []
        name = type(self).__name__
        for gi, grp in enumerate(self.param_groups):
            ps = [p for p in grp["params"] if p.grad is not None]
            for lo in range(0, len(ps), _lib.ADAM_MAX_JOBS):
                chunk = ps[lo:lo + _lib.ADAM_MAX_JOBS]
                jb = _lib.CgnnAdamJobs()
                jb.n = len(chunk)
                for i, p in enumerate(chunk):
                    g = p.grad
                    if g.dtype != torch.float32 or not g.is_contiguous() or g.is_sparse:
                        raise TypeError(f"connectome_gnn_amd.{name} needs dense contiguous float32 gradients")
                    st = self.state[p]
                    jb.numel[i] = p.numel()
                    jb.param[i], jb.grad[i] = p.data_ptr(), g.data_ptr()
                    jb.exp_avg[i], jb.exp_avg_sq[i] = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                    key.append((p.data_ptr(), g.data_ptr()))
                launches.append((jb, gi))
        return tuple(key), launches

    def _current_key(self):
        return tuple((p.data_ptr(), p.grad.data_ptr()) for grp in self.param_groups for p in grp["params"]
                     if p.grad is not None)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dev = self._ensure_state()
        if dev is None:
            return loss
        if self._plan is None or self._plan[0] != self._current_key():
            self._plan = self._build_plan()
        launches = self._plan[1]
        with _lib.device_guard(dev):
            self.refresh_hyper()
            sp = _lib.stream_ptr(dev)
            table, row_bytes = self._hyper.data_ptr(), 8 * _lib.ADAM_HYPER_STRIDE
            # A launch that is being RECORDED reads the table when it is replayed.  One that runs now may as well
            # carry the (validated, identical) values by value -- same bits, and cgnn_adam_step measures 0.1 us
            # under cgnn_adam_step_dev -- where that entry has the update: L2 weight decay.
            recorded = torch.cuda.is_current_stream_capturing()
            for i, (jb, gi) in enumerate(launches):
                advance = int(i == len(launches) - 1)
                decoupled = bool(self.param_groups[gi].get("decoupled_weight_decay", self._decoupled))
                if recorded or decoupled:
                    _lib.call("cgnn_adam_step_dev", jb, self._shared_step, self._arrivals, advance,
                              table + gi * row_bytes, int(decoupled), stream=sp)
                else:
                    _lib.call("cgnn_adam_step", jb, self._shared_step, self._arrivals, advance,
                              *self._hyper_host[gi], stream=sp)
        return loss


class Adam(_OneLaunch, torch.optim.Adam):
    """torch.optim.Adam (L2 weight decay) in one launch."""
    _decoupled = False

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=True)
        self._init_one_launch()


class AdamW(_OneLaunch, torch.optim.AdamW):
    """torch.optim.AdamW (decoupled weight decay: ``p *= 1 - lr * weight_decay`` before the Adam update, the gradient
    untouched) in one launch; restrictions, shared step counter and ``state_dict`` behaviour as Adam above, and its
    checkpoints interchange with ``torch.optim.AdamW``."""
    _decoupled = True

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=True)
        self._init_one_launch()
