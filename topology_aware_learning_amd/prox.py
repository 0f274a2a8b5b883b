"""Fused FedProx proximal term over device-pool models.

Reference (tasks.py:277-286), once per training batch:

    proximal_term = 0.0
    for neighbor in neighbors:
        for w, w_t in zip(client.model.parameters(), neighbor.model.parameters()):
            proximal_term += (w - w_t).norm(2)
    loss += (prox_coeff / 2) * proximal_term

With the client and its neighbors bound to rows of one ModelPool, `prox_term` computes every
norm in one pass over the rows (tal_prox_norms: the client row read once per 8 neighbors from
cache, each neighbor row once) and its gradient in one more (tal_prox_grad), instead of
2·K·P small torch ops per batch.  Gradients flow to the client's parameters and, as in the
reference (whose neighbor parameters are leaves with requires_grad), to neighbor parameters
that require grad.  Numerics: fp32 squares summed per chunk, chunks combined in double
(deterministic); the reference's torch norm uses its own fp32 reduction order, so parity is a
tolerance (tests/test_gpu_interface.py).

bf16 models (every parameter bfloat16: the layout of `model.to(torch.bfloat16)`) run the same two
passes on the rows' b16 segment (tal_prox_norms_bf16 / tal_prox_grad_bf16): the arithmetic is the
fp32 passes' on the parameters widened exactly to fp32, the value stays fp32 and the gradients
are rounded to bf16 once, at the store (include/tal_agg.h "K4 on bf16 models";
tests/test_gpu_prox_bf16.py).  A model with parameters of both dtypes raises NotImplementedError.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check
from .arena import StateLayout, bound_row

_MAX_NB = 64  # neighbors per launch (kProxMaxNb): past it tal_prox_grad_bf16 needs its fp32 scratch


class ProxPlan:
    """Chunk plan of the parameter segments of one layout on one device.  `kind` is the segment
    the parameters lie in, "f32" or "b16" (StateLayout.param_segment_kind); the plan keeps its
    layout alive, so the plan cache can tell it from any other layout object."""

    def __init__(self, layout: StateLayout, param_names: Sequence[str], device):
        self.kind = layout.param_segment_kind(param_names)
        self.layout = layout
        entries = [layout.by_name[n] for n in param_names]
        self.names = list(param_names)
        self.offsets = [int(e.offset) for e in entries]
        self.shapes = [tuple(e.shape) for e in entries]
        self.numels = [int(e.numel) for e in entries]
        seg = np.array([x for o, m in zip(self.offsets, self.numels) for x in (o, m)], dtype=np.int64)
        L = _lib.load()
        P64 = ctypes.POINTER(ctypes.c_int64)
        words = L.tal_prox_plan_words(seg.ctypes.data_as(P64), len(entries))
        if words < 0:
            raise ValueError("empty or invalid parameter segments")
        blob = np.zeros(words, dtype=np.int64)
        nc = ctypes.c_int32()
        check(L.tal_prox_plan_build(seg.ctypes.data_as(P64), len(entries), blob.ctypes.data_as(P64), words,
                                    ctypes.byref(nc)))
        self.n_seg = len(entries)
        self.n_chunks = int(nc.value)
        self.device = torch.device(device)
        self.plan = torch.from_numpy(blob).to(self.device)


_plans: Dict[tuple, ProxPlan] = {}


def _plan_for(layout: StateLayout, names: Sequence[str], device) -> ProxPlan:
    """The cached plan of this layout object.  An entry holds its layout (ProxPlan.layout), so the
    id in the key cannot pass to another layout while the entry lives, and a hit is a hit only
    for that very object."""
    key = (id(layout), tuple(names), str(device), layout.param_segment_kind(names))
    p = _plans.get(key)
    if p is None or p.layout is not layout:
        p = _plans[key] = ProxPlan(layout, names, device)
    return p


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _rows(pool, kind: str):
    """(row accessor, row pitch in elements, torch dtype) of the segment the plan's kind names."""
    if kind == "b16":
        return pool.row_b16, pool.layout.ld_b16, torch.bfloat16
    return pool.row_f32, pool.layout.ld_f32, torch.float32


def prox_norms(pool, row: int, neighbor_rows: Sequence[int], plan: ProxPlan) -> torch.Tensor:
    """norms[t, p] = ||w_p - wt_p||_2 for the pool rows (float32 [K, P], for bf16 rows too)."""
    L = _lib.load()
    k = len(neighbor_rows)
    row_of = _rows(pool, plan.kind)[0]
    fn = L.tal_prox_norms_bf16 if plan.kind == "b16" else L.tal_prox_norms
    scratch = torch.empty(int(L.tal_prox_scratch_bytes(plan.n_chunks, k)), dtype=torch.uint8, device=pool.device)
    norms = torch.empty((k, plan.n_seg), dtype=torch.float32, device=pool.device)
    wt = _lib.ptr_array([row_of(r).data_ptr() for r in neighbor_rows])
    check(fn(ctypes.c_void_p(row_of(row).data_ptr()), wt, k,
             ctypes.c_void_p(plan.plan.data_ptr()), plan.n_chunks, plan.n_seg,
             ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(norms.data_ptr()),
             _stream(pool.device)))
    return norms


class _ProxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, pool, row, neighbor_rows, n_client, *params):
        norms = prox_norms(pool, row, neighbor_rows, plan)
        ctx.plan, ctx.pool, ctx.row, ctx.neighbor_rows, ctx.n_client = plan, pool, row, list(neighbor_rows), n_client
        ctx.needs = [p.requires_grad for p in params]
        ctx.save_for_backward(norms)
        return norms.double().sum().float()

    @staticmethod
    def backward(ctx, g):
        (norms,) = ctx.saved_tensors
        plan, pool, k, P = ctx.plan, ctx.pool, len(ctx.neighbor_rows), ctx.n_client
        L = _lib.load()
        scale = g.detach().to(torch.float32).reshape(1).contiguous()
        row_of, n, dtype = _rows(pool, plan.kind)
        gw = torch.zeros(n, dtype=dtype, device=pool.device)
        want_t = [any(ctx.needs[P + t * P: P + (t + 1) * P]) for t in range(k)]
        gwt = [torch.zeros(n, dtype=dtype, device=pool.device) if wnt else None for wnt in want_t]
        wt = _lib.ptr_array([row_of(r).data_ptr() for r in ctx.neighbor_rows])
        gwt_p = _lib.ptr_array([x.data_ptr() if x is not None else 0 for x in gwt])
        args = [ctypes.c_void_p(row_of(ctx.row).data_ptr()), wt, k,
                ctypes.c_void_p(plan.plan.data_ptr()), plan.n_chunks, plan.n_seg,
                ctypes.c_void_p(norms.data_ptr()), ctypes.c_void_p(scale.data_ptr()),
                ctypes.c_void_p(gw.data_ptr()), gwt_p]
        if plan.kind == "b16":
            # the running sum of more than one launch stays fp32 (never a bf16 gw in between)
            acc = torch.empty(n, dtype=torch.float32, device=pool.device) if k > _MAX_NB else None
            check(L.tal_prox_grad_bf16(*args, ctypes.c_void_p(acc.data_ptr() if acc is not None else 0),
                                       n if acc is not None else 0, _stream(pool.device)))
        else:
            check(L.tal_prox_grad(*args, _stream(pool.device)))

        def views(buf, need):
            return [buf[o: o + m].view(s) if nd else None
                    for o, m, s, nd in zip(plan.offsets, plan.numels, plan.shapes, need)]

        grads = views(gw, ctx.needs[:P])
        for t in range(k):
            need = ctx.needs[P + t * P: P + (t + 1) * P]
            grads += views(gwt[t], need) if gwt[t] is not None else [None] * P
        return (None, None, None, None, None, *grads)


def prox_term(model: torch.nn.Module, neighbor_models: Sequence[torch.nn.Module]) -> Optional[torch.Tensor]:
    """sum_t sum_p ||w_p - wt_p||_2 with autograd, when the model and every neighbor are rows of
    one device ModelPool; None otherwise (the caller keeps the reference's torch loop)."""
    if not neighbor_models:
        return None
    b = bound_row(model)
    if b is None or b[0].device.type != "cuda":
        return None
    pool, row = b
    rows: List[int] = []
    for m in neighbor_models:
        nb = bound_row(m)
        if nb is None or nb[0] is not pool:
            return None
        rows.append(nb[1])
    names = [n for n, _ in model.named_parameters()]
    plan = _plan_for(pool.layout, names, pool.device)
    params = [p for _, p in model.named_parameters()]
    for m in neighbor_models:
        params += [p for _, p in m.named_parameters()]
    return _ProxFn.apply(plan, pool, row, rows, len(names), *params)
