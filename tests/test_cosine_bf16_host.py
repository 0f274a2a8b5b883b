"""Cosine similarity of bf16 models without a GPU: the library's host forms
(tal_host_cosine_bf16, tal_host_cosine_round_bf16) through ops and similarity.

The cosine similarity of two bf16 models is K2's fp32 result for the two models with every
parameter widened exactly to fp32 (include/tal_agg.h "K2 on bf16 models"), so the expected value
of every case is the existing fp32 oracle (oracle.cosine_model, torch's CPU order) on the widened
rows, compared bit for bit.  The reference (cosine_similarity, src/decentralized_client.py:661-681
of the reference) has no bf16 path of its own.
"""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

from _cosine_bf16 import HOST_SHAPES, as_torch, bf16_rows, bits, module_row, ref, refs, small_bf16
from topology_aware_learning_amd import _lib, ops, similarity
from topology_aware_learning_amd.aggregate import layout_of_module
from topology_aware_learning_amd.arena import StateLayout


def _check(rows, segs, a_idx, b_idx, threads=1):
    t = [as_torch(r) for r in rows]
    plan = ops.build_cosine_plan(segs, threads=threads)
    got = ops.host_cosine([t[j] for j in a_idx], [t[j] for j in b_idx], plan)
    assert got.dtype == torch.float32
    want = refs(rows, segs, list(zip(a_idx, b_idx)), threads)
    assert bits(got.numpy()) == bits(want), (segs[:3], got, want)


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mis", [0, 1, 3])
def test_host_shapes_vs_oracle(shape, mis):
    """One tensor per plan, its segment `mis` elements into the row."""
    a, i, b = shape
    segs = [(mis, a, i, b)]
    rows = bf16_rows(np.random.default_rng(a * 1000 + i * 10 + b + mis), segs, 3)
    _check(rows, segs, [0, 0, 2], [1, 2, 1])


def test_host_all_shapes_one_plan():
    segs, off = [], 5
    for a, i, b in HOST_SHAPES:
        segs.append((off, a, i, b))
        off += a * i * b + 3
    rows = bf16_rows(np.random.default_rng(11), segs, 4)
    _check(rows, segs, [0, 0, 0, 2], [1, 2, 3, 3])


@pytest.mark.parametrize("threads", [1, 8])
def test_host_thread_word(threads):
    """A tensor mean over 49,152 outputs (>= 32768) follows torch's two-pass order for the plan's
    thread word."""
    segs = [(1, 768, 3, 64), (1 + 768 * 3 * 64 + 2, 40, 7, 1)]
    rows = bf16_rows(np.random.default_rng(8), segs, 2)
    _check(rows, segs, [0], [1], threads=threads)


def test_host_cosine_round_vs_oracle_and_per_pair():
    """A 7-row bf16 pool view with an odd row pitch: a star plus a ring, both orders of some
    edges; bitwise the oracle and bitwise ops.host_cosine pair by pair."""
    segs, off = [], 5
    for a, i, b in [(8, 64, 9), (16, 72, 1), (30, 1, 1), (3, 50, 32), (4, 2, 7)]:
        segs.append((off, a, i, b))
        off += a * i * b + 3
    n = off
    rows = bf16_rows(np.random.default_rng(17), [(0, 1, n, 1)], 7)
    pool = torch.zeros(7, (n + 37) | 1, dtype=torch.bfloat16)
    assert pool.stride(0) % 2 == 1
    view = pool[:, :n]
    view.copy_(as_torch(np.stack(rows)))
    pairs = [(0, r) for r in range(1, 7)] + [(r, r % 6 + 1) for r in range(1, 7)] + [(3, 0), (2, 1), (6, 5)]
    plan = ops.build_cosine_plan(segs)
    got = ops.host_cosine_round(view, pairs, plan)
    assert got.dtype == torch.float32
    want = refs(rows, segs, pairs)
    assert bits(got.numpy()) == bits(want)
    per_pair = ops.host_cosine([view[a].contiguous() for a, _ in pairs], [view[b].contiguous() for _, b in pairs], plan)
    assert bits(got.numpy()) == bits(per_pair.numpy())


def test_mixed_dtype_operands_are_refused():
    segs = [(0, 4, 6, 1)]
    plan = ops.build_cosine_plan(segs)
    b = as_torch(bf16_rows(np.random.default_rng(1), segs, 1)[0])
    f = b.float()
    with pytest.raises(ValueError, match="dtype"):
        ops.host_cosine([b], [f], plan)
    with pytest.raises(ValueError, match="dtype"):
        ops.host_cosine([f, f], [f, b], plan)
    with pytest.raises(ValueError):
        ops.host_cosine([b.to(torch.float16)], [b.to(torch.float16)], plan)
    # one dtype: both forms answer, and the bf16 one is the fp32 one on the widened rows
    assert bits(ops.host_cosine([b], [b], plan).numpy()) == bits(ops.host_cosine([f], [f], plan).numpy())


def test_param_segment_kind_and_mixed_models():
    lay32 = StateLayout.from_layout([("w", (4, 3, 3, 3), "float32"), ("b", (4,), "float32"), ("n", (), "int64")])
    lay16 = StateLayout.from_layout([("w", (4, 3, 3, 3), "bfloat16"), ("b", (4,), "bfloat16"), ("n", (), "int64")])
    mixed = StateLayout.from_layout([("w", (4, 3, 3, 3), "bfloat16"), ("b", (4,), "float32")])
    assert lay32.param_segment_kind(["w", "b"]) == "f32"
    assert lay16.param_segment_kind(["w", "b"]) == "b16"
    assert lay16.param_segments(["w", "b"]) == lay32.param_segments(["w", "b"]) == [(0, 4, 3, 9), (108, 4, 1, 1)]
    assert mixed.param_segment_kind(["w"]) == "b16" and mixed.param_segment_kind(["b"]) == "f32"
    for call in (mixed.param_segment_kind, mixed.param_segments):
        with pytest.raises(NotImplementedError) as exc:
            call(["w", "b"])
        assert "w" in str(exc.value) and "b is fp32" in str(exc.value) and "w is bf16" in str(exc.value)
    with pytest.raises(NotImplementedError):
        lay32.param_segment_kind(["n"])


def test_similarity_on_bf16_modules(monkeypatch):
    """similarity.cosine_pairs and the reference interface's cosine_similarity on modules after
    .to(torch.bfloat16), in a process that sees no GPU (the host form)."""
    import src.decentralized_client as dc

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    models = [small_bf16(s) for s in (3, 4, 5)]
    layout = layout_of_module(models[0])
    names = [n for n, _ in models[0].named_parameters()]
    assert layout.param_segment_kind(names) == "b16" and layout.n_f32 == 0
    segs = layout.param_segments(names)
    rows = [module_row(m, layout) for m in models]
    threads = max(1, min(torch.get_num_threads(), 1024))
    want = [ref(rows[0], rows[j], segs, threads) for j in (1, 2)]
    got = similarity.cosine_pairs(models[0], models[1:])
    assert bits(got) == bits(want)
    one = dc.cosine_similarity(models[2], models[1])
    assert one.dtype == torch.float32 and one.dim() == 0
    assert bits([one.item()]) == bits([ref(rows[2], rows[1], segs, threads)])
    # the fp32 copies of the same models give the same values: the definition
    wide = [copy.deepcopy(m).float() for m in models]
    again = similarity.cosine_pairs(wide[0], wide[1:])
    assert bits(again) == bits(want)


def test_abi_and_symbols():
    L = _lib.load()
    assert L.tal_abi_version() == _lib.ABI_VERSION >= 27
    for name in ("tal_cosine_params_bf16", "tal_cosine_round_bf16", "tal_host_cosine_bf16",
                 "tal_host_cosine_round_bf16"):
        assert name in _lib.EXPORTED and name in _lib._SIGS
        assert getattr(L, name) is not None
