"""Which encoder a (model, batch) call runs on: one pure function, and the ranks' agreement on its answer
(the table: DESIGN.md section 4.2b2)."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch.distributed as dist
import torch.nn as nn

from . import fused, gcn_half_path, gcn_wide_path, sage_path

ENCODERS = {"tile": fused, "wide": gcn_wide_path, "half": gcn_half_path, "sage": sage_path}
_WIRE = {None: 0, "wide": 1, "half": 1, "tile": 2, "sage": 2}      # the codes of the all-reduce(MIN)


class Choice(NamedTuple):
    kind: Optional[str]       # key of ENCODERS, or None = the layered path
    reason: Optional[str]     # why no encoder covers the call
    record: Optional[str]     # what encode() leaves in model._fused_kind; None = not written


def choose(model, batch, structure) -> Choice:
    """Reads the model's configuration, the batch's requires_grad flags and the structure's declared facts;
    writes nothing.  Raises where the caller insists (impl="fused", storage="fp16") and nothing covers the call."""
    if model.storage == "fp16":
        why = gcn_half_path.eligible(model, batch, structure)
        if why is not None:
            raise RuntimeError(f"storage='fp16' requested but not applicable: {why}")
        return Choice("half", None, "half")
    if model.impl == "layered" or model._family is None:
        return Choice(None, None, None)
    if model._family == "gcn":
        why = fused.eligible(model, batch, structure)
        kind = "tile" if why is None else "wide" if gcn_wide_path.eligible(model, batch, structure) is None else None
        # a GCN that falls to the layered path is still recorded as "tile": bench.py picks its dominant
        # kernel from _fused_kind without looking at impl_used, and has always seen that value
        record = kind or "tile"
    else:
        why = sage_path.eligible(model, batch, structure)
        kind, record = ("sage" if why is None else None), None
    if kind is None and model.impl == "fused":
        raise RuntimeError(f"impl='fused' requested but not applicable: {why}")
    return Choice(kind, None if kind else why, record)


def agreed(model, batch, structure, choice: Choice) -> Choice:
    """`choice` -- or, while training with SyncBatchNorm across ranks, the ranks' common answer: the choice
    depends on the local shard, and the one-node encoders exchange their BatchNorm sums with another collective
    than torch's SyncBatchNorm, so mixed paths would hang.  One all-reduce(MIN) per (model, structure)."""
    if not (model.training and dist.is_initialized() and dist.get_world_size() > 1
            and any(isinstance(bn, nn.SyncBatchNorm) for bn in model.batch_norms)):
        return choice
    key = (type(model).__name__, model.impl, id(model))
    cache = structure._path_agreement
    if key not in cache:
        from . import dist as cdist
        cache[key] = cdist.agree_min(_WIRE[choice.kind], batch.node_features.device)
    if choice.kind is not None and cache[key] == 0:
        return Choice(None, "another rank's shard is not covered", choice.record)
    if choice.kind == "tile" and cache[key] == 1:
        return Choice("wide", None, "wide")
    return choice
