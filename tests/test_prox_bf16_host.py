"""The FedProx term of bf16 models, host side (no GPU): the chunk plan of a bf16 layout and its
kind, the refusal of a model with parameters of both dtypes, the plan cache (an entry holds its
layout, so a layout's id can never come back on another layout while its plan is cached) and
the argument errors of tal_prox_norms / tal_prox_grad and their _bf16 twins (include/tal_agg.h
"K4 on bf16 models").  The kernels are tested in tests/test_gpu_prox_bf16.py."""
import ctypes
import gc
import weakref

import numpy as np
import pytest
import torch

from _models import TinyNet
from topology_aware_learning_amd import _lib
from topology_aware_learning_amd.aggregate import layout_of_module
from topology_aware_learning_amd.arena import StateLayout
from topology_aware_learning_amd.prox import ProxPlan, _plan_for


def _check_table(pl, lay, names):
    """test_prox_plan_covers_parameter_segments' checks (tests/test_host_logic.py)."""
    h = pl.plan.numpy()
    ptr = h[: pl.n_seg + 1]
    ch = h[pl.n_seg + 1:].reshape(-1, 3)
    assert len(ch) == pl.n_chunks == ptr[-1]
    for s, name in enumerate(names):
        e = lay.by_name[name]
        rows = ch[ptr[s]: ptr[s + 1]]
        assert np.all(rows[:, 0] == s)
        assert rows[0, 1] == e.offset and rows[:, 2].sum() == e.numel
        assert np.all(rows[1:, 1] == rows[:-1, 1] + rows[:-1, 2])  # contiguous chunks


def test_plan_of_a_bf16_layout():
    m = TinyNet().to(torch.bfloat16)
    lay = layout_of_module(m)
    names = [n for n, _ in m.named_parameters()]
    pl = ProxPlan(lay, names, "cpu")
    assert pl.kind == "b16"
    assert all(lay.by_name[n].seg == "b16" for n in names)
    _check_table(pl, lay, names)
    f32 = TinyNet()
    assert ProxPlan(layout_of_module(f32), names, "cpu").kind == "f32"


def test_mixed_model_is_refused():
    m = TinyNet()
    m.fc.weight.data = m.fc.weight.data.to(torch.bfloat16)
    lay = layout_of_module(m)
    names = [n for n, _ in m.named_parameters()]
    with pytest.raises(NotImplementedError):
        _plan_for(lay, names, "cpu")
    with pytest.raises(NotImplementedError):
        ProxPlan(lay, names, "cpu")


def test_cache_holds_the_layout():
    names = ["a", "b"]
    lay = StateLayout.from_layout([("a", (5, 3), "bfloat16"), ("b", (7,), "bfloat16")])
    p = _plan_for(lay, names, "cpu")
    assert _plan_for(lay, names, "cpu") is p  # the same layout object: the same plan object
    r = weakref.ref(lay)
    del lay
    gc.collect()
    assert r() is not None  # the cache holds it: its id cannot be recycled
    assert p.layout is r()
    # another layout object, the same names, other shapes: its own plan, its own offsets
    lay2 = StateLayout.from_layout([("a", (2, 3), "bfloat16"), ("b", (9000,), "bfloat16")])
    p2 = _plan_for(lay2, names, "cpu")
    assert p2 is not p and p2.layout is lay2
    _check_table(p2, lay2, names)
    assert p2.offsets == [0, 6] and p2.n_chunks == 3
    _check_table(p, r(), names)
    # an equal layout that is another object is another entry too
    lay3 = StateLayout.from_layout([("a", (2, 3), "bfloat16"), ("b", (9000,), "bfloat16")])
    assert lay3 == lay2 and _plan_for(lay3, names, "cpu") is not p2
    assert _plan_for(lay2, names, "cpu") is p2


def test_cache_never_serves_another_layout_object(monkeypatch):
    """An entry whose layout is not the asking object is a miss, whatever its key says."""
    from topology_aware_learning_amd import prox

    names = ["a"]
    old = StateLayout.from_layout([("a", (4,), "float32")])
    new = StateLayout.from_layout([("pad", (3,), "float32"), ("a", (4,), "float32")])
    stale = ProxPlan(old, names, "cpu")
    monkeypatch.setitem(prox._plans, (id(new), ("a",), "cpu", "f32"), stale)
    got = _plan_for(new, names, "cpu")
    assert got is not stale and got.layout is new and got.offsets == [3]


def test_argument_errors():
    L = _lib.load()
    ok = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused before a launch
    one = (ctypes.c_void_p * 1)(0x2000)
    null1 = (ctypes.c_void_p * 1)(None)
    E = _lib.TAL_ERR_INVALID

    def norms(w=ok, wt=one, k=1):
        return L.tal_prox_norms_bf16(w, wt, k, ok, 1, 1, ok, ok, None)

    def grad(w=ok, wt=one, k=1, acc=None, acc_elems=0):
        return L.tal_prox_grad_bf16(w, wt, k, ok, 1, 1, ok, ok, ok, None, acc, acc_elems, None)

    def norms_f32(w=ok, wt=one, k=1):
        return L.tal_prox_norms(w, wt, k, ok, 1, 1, ok, ok, None)

    def grad_f32(w=ok, wt=one, k=1):
        return L.tal_prox_grad(w, wt, k, ok, 1, 1, ok, ok, ok, None, None)

    # a null neighbor in the second launch's batch: refused with the rest, before the first launch
    late = (ctypes.c_void_p * 65)(*([0x2000] * 64 + [None]))
    for call, name in ((norms, b"tal_prox_norms_bf16"), (grad, b"tal_prox_grad_bf16"),
                       (norms_f32, b"tal_prox_norms"), (grad_f32, b"tal_prox_grad")):
        assert call(w=None) == E and name in L.tal_last_error()
        assert call(k=0) == E and name in L.tal_last_error()
        assert call(wt=null1) == E and name in L.tal_last_error() and b"null neighbor" in L.tal_last_error()
        more = dict(acc=ok, acc_elems=1) if call is grad else {}  # the scratch is fine: the pointer is refused
        assert call(wt=late, k=65, **more) == E and name in L.tal_last_error() and b"null neighbor" in L.tal_last_error()
    many = (ctypes.c_void_p * 65)(*([0x2000] * 65))
    assert grad(wt=many, k=65, acc=None) == E and b"tal_prox_grad_bf16" in L.tal_last_error()
    assert grad(wt=many, k=65, acc=ok, acc_elems=0) == E  # too small for the plan's one chunk
