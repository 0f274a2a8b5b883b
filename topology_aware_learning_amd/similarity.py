"""Model-to-model cosine similarity (K2), for the `*_sim` aggregation strategies: the GPU kernels,
or - in a process that sees no GPU - the library's host form of the same arithmetic
(tal_host_cosine).

Reference: cosine_similarity, src/decentralized_client.py:661-681 — over `named_parameters`
(buffers excluded), nn.CosineSimilarity(dim=1, eps=1e-6) per tensor (1-D tensors get a
trailing unit dim), mean per tensor, average over tensors.  K2 performs the reference's fp32
operations in the order of the torch CPU kernels it runs on (include/tal_agg.h), so the
values are the reference's bit for bit and sim_centrality_module_avg's arg-min (:511) —
near-ties and exact fp32 ties included — picks the reference's neighbor
(tests/golden/near_ties.*).  A tensor mean over >= 32768 outputs (ViT-B/16's patch embedding,
196,608) is a two-pass parallel sum in torch whose order depends on the intra-op thread count;
K2 follows torch.get_num_threads() of the calling process (tests/golden/cosine_threads.json).

bf16 models (every parameter bfloat16, as after `model.to(torch.bfloat16)`): the reference has no
such path; here their cosine similarity is K2's fp32 result for the models widened exactly to
fp32, bit for bit the reference's cosine_similarity(m1.float(), m2.float()) (include/tal_agg.h
"K2 on bf16 models").  The kernels read the bf16 segment of the rows in place of the fp32 one.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops
from .aggregate import _device_for, _stage, layout_of_module
from .arena import bound_row

_plans: Dict[Tuple, ops.CosinePlan] = {}


def _param_names(model: nn.Module) -> List[str]:
    return [n for n, _ in model.named_parameters()]


def _row(pool, r: int, kind: str) -> torch.Tensor:
    return pool.row_f32(r) if kind == "f32" else pool.row_b16(r)


def _flat(models: Sequence[nn.Module], layout, device, kind: str) -> List[torch.Tensor]:
    """Each model's parameter segment (kind: "f32" or "b16") on `device`."""
    out: List = [None] * len(models)
    rest = []
    for j, m in enumerate(models):
        b = bound_row(m)
        if b is not None and b[0].device == device and b[0].layout == layout:
            out[j] = _row(b[0], b[1], kind)
        else:
            rest.append(j)
    if rest:
        staged = _stage([models[j] for j in rest], layout, device)
        for k, j in enumerate(rest):
            out[j] = staged[k][kind]
    return out


def _plan_for(layout, names: Sequence[str]) -> Tuple[ops.CosinePlan, str]:
    """The layout's cosine plan over `names` and the segment its offsets index ("f32" or "b16")."""
    # a tensor mean over >= 32768 outputs follows torch's parallel order for this process's
    # intra-op thread count, as the reference's own call would (tal_agg.h K2).  The plan holds
    # at most 1024 (tal_cosine_plan_set_threads); a process with more intra-op threads gets
    # 1024's order, which differs from torch's only for a tensor mean over > 1024 x 32768
    # outputs (none in the reference's models: ViT-B/16's largest is 196,608)
    threads = max(1, min(torch.get_num_threads(), 1024))
    kind = layout.param_segment_kind(names)
    key = (layout.key, tuple(names), threads, kind)
    plan = _plans.get(key)
    if plan is None:
        plan = ops.build_cosine_plan(layout.param_segments(names), threads=threads)
        _plans[key] = plan
    return plan, kind


def cosine_round(pool, pairs: Sequence[Tuple[int, int]], model: nn.Module) -> List[float]:
    """[cosine_similarity(row a, row b) for (a, b) in pairs] over the rows of one ModelPool, a
    whole round's pairs in one launch sequence and one copy to the host (K2r, tal_agg.h): every
    model's norms once, every unordered pair once, the values bit for bit cosine_pairs'.
    model: any model of the pool's layout (its named_parameters say which entries count).  With
    no GPU visible the pool is a host pool and the library's host form runs."""
    if not len(pairs):
        return []
    layout = pool.layout
    if layout_of_module(model) != layout:
        raise ValueError("cosine_round: the model does not have the pool's layout")
    plan, kind = _plan_for(layout, _param_names(model))
    seg = pool.f32 if kind == "f32" else pool.b16
    if not torch.cuda.is_available():
        return [float(x) for x in ops.host_cosine_round(seg, pairs, plan).tolist()]
    with torch.cuda.device(pool.device):
        return [float(x) for x in ops.cosine_round(seg, pairs, plan).cpu().tolist()]


def cosine_pairs(model: nn.Module, others: Sequence[nn.Module]) -> List[float]:
    """[cosine_similarity(model, o) for o in others] in one kernel launch."""
    if not others:
        return []
    layout = layout_of_module(model)
    plan, kind = _plan_for(layout, _param_names(model))
    if not torch.cuda.is_available():  # no GPU (config 1's setting): the library's host K2
        flats = _host_flat([model, *others], layout, kind)
        return [float(x) for x in ops.host_cosine([flats[0]] * len(others), flats[1:], plan).tolist()]
    device = _device_for([model, *others])
    b0 = bound_row(model)
    mp = getattr(b0[0], "multi", None) if b0 is not None else None
    bounds = [bound_row(m) for m in others]
    if mp is not None and all(b is not None and mp[0].member(b[0]) is not None for b in bounds):
        # clients over several GPUs (multipool.MultiPool): the neighbors other GPUs own are read
        # from this GPU's ghost rows, refreshed first
        pool = b0[0]
        with torch.cuda.device(pool.device):
            rows = mp[0].rows_for(mp[1], bounds)
            res = ops.cosine([_row(pool, b0[1], kind)] * len(others), [_row(pool, r, kind) for r in rows], plan)
            return [float(x) for x in res.cpu().tolist()]
    flats = _flat([model, *others], layout, device, kind)
    res = ops.cosine([flats[0]] * len(others), flats[1:], plan)
    return [float(x) for x in res.cpu().tolist()]


def _host_flat(models: Sequence[nn.Module], layout, kind: str) -> List[torch.Tensor]:
    """Each model's parameter segment (kind: "f32" or "b16") as a contiguous CPU tensor: a
    pinned-row view when the model is bound to a host row, else the segment's entries
    concatenated in state_dict order."""
    out = []
    for j, m in enumerate(models):
        b = bound_row(m)
        if b is not None and b[0].device.type == "cpu" and b[0].layout == layout:
            out.append(_row(b[0], b[1], kind))
            continue
        sd = m.state_dict()
        layout.check_compatible(sd, f"model {j}")
        if any(t.device.type != "cpu" for t in sd.values()):
            raise RuntimeError("no GPU is visible, but a model has tensors off the CPU")
        out.append(torch.cat([t.detach().reshape(-1) for t in layout.flatten_cat(sd, kind)]))
    return out
