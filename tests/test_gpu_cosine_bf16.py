"""K2 and K2r on bf16 models (tal_cosine_params_bf16, tal_cosine_round_bf16) on the GPU.

The cosine similarity of two bf16 models is K2's fp32 result for the two models with every
parameter widened exactly to fp32 (include/tal_agg.h "K2 on bf16 models"): the kernels are the
fp32 kernels with the loads widening a bf16 bit pattern u to the fp32 bits u << 16.  So every
expected value is the existing fp32 oracle (oracle.cosine_model, torch's CPU order) on the
widened rows, compared bit for bit: the shape families of test_gpu_cosine_staged.py at element
offsets 0, 1 and 3 (rows 2-byte aligned only), streamed and direct chunks in one call, more pairs
than one launch, special values, the round form on a pool with an odd pitch, similarity on bf16
modules, a sim_centrality_module_avg call and the batched `*_sim` round on bf16 pool-bound models.
Reference: cosine_similarity / sim_centrality_module_avg, src/decentralized_client.py:452-550,
661-681 of the reference (which has no bf16 path of its own).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
from torch.utils.data import Subset, TensorDataset

from _cosine_bf16 import (HOST_SHAPES, as_torch, bf16_rows, bits, extent, module_row, ref, refs, same, small_bf16,
                          torch_bits)
from _models import TinyNet
from topology_aware_learning_amd import ops, similarity
from topology_aware_learning_amd import weights as W
from topology_aware_learning_amd.aggregate import aggregate_models, layout_of_module
from topology_aware_learning_amd.arena import ModelPool, bound_row

pytestmark = pytest.mark.gpu

_SHAPES = HOST_SHAPES + [(4, 100, 2), (4, 2, 7), (2, 1024, 9)]


def _check(cuda, rows, segs, a_idx, b_idx):
    dev = [as_torch(r, cuda) for r in rows]
    plan = ops.build_cosine_plan(segs)
    got = ops.cosine([dev[j] for j in a_idx], [dev[j] for j in b_idx], plan)
    assert got.dtype == torch.float32
    got = got.cpu().numpy()
    want = refs(rows, segs, list(zip(a_idx, b_idx)))
    assert same(got, want), (segs[:3], [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if not same(g, w)][:4])


@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mis", [0, 1, 3])
def test_shapes_vs_oracle(cuda, shape, mis):
    """One tensor per plan, its segment `mis` elements (2 `mis` bytes) into the row; pairs that
    share one `a`, then pairs that each have their own."""
    a, i, b = shape
    segs = [(mis, a, i, b)]
    rows = bf16_rows(np.random.default_rng(a * 1000 + i * 10 + b + mis), segs, 4)
    _check(cuda, rows, segs, [0, 0, 0], [1, 2, 3])
    _check(cuda, rows, segs, [1, 2, 3], [0, 0, 0])


def test_all_shapes_one_plan(cuda):
    """Every shape in one model at odd gaps: streamed and direct chunks in one call (the direct
    chunks fork onto the side stream)."""
    segs, off = [], 5
    for a, i, b in _SHAPES:
        segs.append((off, a, i, b))
        off += a * i * b + 3
    plan = ops.build_cosine_plan(segs)
    assert 0 < int(plan.host[3]) < plan.n_chunks  # both kinds of chunk
    rows = bf16_rows(np.random.default_rng(11), segs, 5)
    _check(cuda, rows, segs, [0, 0, 0, 0], [1, 2, 3, 4])


def test_more_pairs_than_one_launch(cuda):
    segs = [(0, 8, 64, 9), (4608, 16, 72, 1), (4608 + 1152, 30, 1, 1)]
    rows = bf16_rows(np.random.default_rng(3), segs, 36)
    _check(cuda, rows, segs, [0] * 35, list(range(1, 36)))


# bf16 patterns: +0, -0, the smallest denormal, 2^-60, 2^70, +inf, a NaN (cos_rdiv's range checks
# and the IEEE-division fallback)
_SPECIAL = [0x0000, 0x8000, 0x0001, (127 - 60) << 7, (127 + 70) << 7, 0x7F80, 0x7FC1]
_KINDS = {"streamed_col": (3, 37, 9), "direct_col": (2, 20, 32), "row": (5, 40, 1), "elem": (30, 1, 1)}


@pytest.mark.parametrize("kind", list(_KINDS))
def test_special_values(cuda, kind):
    """One small tensor of each kind: model 1 + k carries special value k at the tensor's first,
    a middle and its last element, and in one whole reduced run; model 8 every special value;
    model 9 only zeros of both signs (the norm's 1e-6 clamp).  Against a plain model, against
    each other and against themselves."""
    a, i, b = _KINDS[kind]
    segs = [(1, a, i, b)]
    n = a * i * b
    rng = np.random.default_rng(a + i + b)
    rows = bf16_rows(rng, segs, 10)
    for k, v in enumerate(_SPECIAL):
        r = rows[1 + k]
        r[[1, 1 + n // 2, n]] = v
        r[1 + (a - 1) * i * b: 1 + n: b] = v  # output (a - 1, column 0): its whole reduced run
        rows[8][1 + (3 + 4 * k) % n] = v
    rows[9][:] = np.where(rng.random(len(rows[9])) < 0.5, 0x0000, 0x8000).astype(np.uint16)
    others = list(range(1, 10))
    _check(cuda, rows, segs, [0] * 9, others)
    _check(cuda, rows, segs, others, others[1:] + others[:1])
    _check(cuda, rows, segs, others, others)
    nan_free = refs(rows, segs, [(0, j) for j in (1, 2, 3, 4, 9)])
    assert not np.isnan(nan_free).any()  # zeros, denormals and 2^-60 leave finite values to compare


def _round_segments():
    segs, off = [], 5
    for a, i, b in [(8, 64, 9), (16, 72, 1), (30, 1, 1), (3, 50, 32), (4, 2, 7), (3, 37, 31)]:
        segs.append((off, a, i, b))
        off += a * i * b + 3
    return segs


def test_round_form(cuda):
    """ops.cosine_round on a 13-row bf16 pool view with an odd pitch: a 12-neighbour star (one row
    gets two groups), reversed duplicates and a self pair; bitwise the oracle, bitwise ops.cosine
    on the same pairs, and again under a budget that takes more than one batch."""
    segs = _round_segments()
    n = extent(segs)
    rows = bf16_rows(np.random.default_rng(23), segs, 13)
    row_of = list(np.random.default_rng(6).permutation(13))
    pool = torch.zeros(13, (n + 29) | 1, dtype=torch.bfloat16, device=cuda)
    assert pool.stride(0) % 2 == 1
    view = pool[:, :n]
    for m, r in enumerate(row_of):
        view[r].copy_(as_torch(rows[m], cuda))
    pairs = [(0, m) for m in range(1, 13)] + [(3, 0), (7, 0), (12, 0), (0, 3), (4, 4)]
    on_pool = [(int(row_of[a]), int(row_of[b])) for a, b in pairs]
    plan = ops.build_cosine_plan(segs)
    table = ops.build_cosine_round(on_pool, 13)
    assert table.info.n_unique == 13 and table.info.n_groups >= 2
    want = refs(rows, segs, pairs)
    got = ops.cosine_round(view, table, plan)
    assert got.dtype == torch.float32 and table.info.n_batches == 1
    assert bits(got.cpu().numpy()) == bits(want)
    per_call = ops.cosine([view[a] for a, _ in on_pool], [view[b] for _, b in on_pool], plan)
    assert bits(per_call.cpu().numpy()) == bits(want)
    n_out, n_seg = int(plan.host[1]), plan.n_seg
    budget = 4 * (table.info.n_models * n_out + table.info.n_unique) + 4 * (n_out + n_seg) * 8
    got = ops.cosine_round(view, table, plan, budget_bytes=budget)
    assert table.info.n_batches >= 2 and table.info.batch_pairs <= 8
    assert bits(got.cpu().numpy()) == bits(want)
    with pytest.raises(ValueError):
        ops.cosine([view[0]], [view[1].float()], plan)  # one dtype per call


def _threads():
    return max(1, min(torch.get_num_threads(), 1024))


def test_similarity_on_bf16_modules(cuda):
    """similarity.cosine_pairs on bf16 modules bound to a ModelPool (the rows' b16 segment in
    place), on unbound GPU modules and on unbound CPU modules (staged)."""
    models = [small_bf16(s) for s in (3, 4, 5, 6)]
    layout = layout_of_module(models[0])
    names = [n for n, _ in models[0].named_parameters()]
    assert layout.param_segment_kind(names) == "b16"
    segs = layout.param_segments(names)
    rows = [module_row(m, layout) for m in models]
    want = [ref(rows[0], rows[j], segs, _threads()) for j in (1, 2, 3)]
    assert bits(similarity.cosine_pairs(models[0], models[1:])) == bits(want)  # CPU modules
    on_gpu = [m.to(cuda) for m in models]
    assert bits(similarity.cosine_pairs(on_gpu[0], on_gpu[1:])) == bits(want)
    pool = ModelPool(layout, 6, cuda)
    for m, r in zip(on_gpu, (4, 0, 5, 2)):
        pool.bind(m, r)
    assert all(bound_row(m) is not None for m in on_gpu)
    assert bits(similarity.cosine_pairs(on_gpu[0], on_gpu[1:])) == bits(want)
    # the round form over the same pool
    pairs = [(4, 0), (0, 4), (4, 5), (4, 2)]
    got = similarity.cosine_round(pool, pairs, on_gpu[0])
    assert bits(got) == bits([want[0], want[0], want[1], want[2]])


DUMMY = TensorDataset(torch.zeros(4, 1), torch.zeros(4, dtype=torch.long))


def _client(idx, model):
    from src.decentralized_client import DecentralClient

    return DecentralClient(idx=idx, prox_coeff=0.0, model=model, train_data=Subset(DUMMY, [0, 1, 2, 3]), test_data=None,
                           valid_data=None, global_test_data=DUMMY, global_backdoor_test_data=None, neighbors=[],
                           neighbor_probs=[])


def _ring(cuda, n=5, seed=40):
    """n bf16 TinyNets (conv, batch norm with an int64 counter, 1 x 1 conv, linear) bound to rows of
    a device pool; their b16 rows as bit patterns, the parameters' segments, the clients."""
    models = []
    for k in range(n):
        torch.manual_seed(seed + k)
        models.append(TinyNet().to(torch.bfloat16).to(cuda))
    layout = layout_of_module(models[0])
    pool = ModelPool(layout, n, cuda)
    for k, m in enumerate(models):
        pool.bind(m, k)
    names = [nm for nm, _ in models[0].named_parameters()]
    assert layout.param_segment_kind(names) == "b16" and layout.n_i64 > 0
    segs = layout.param_segments(names)
    return pool, layout, segs, [_client(k, m) for k, m in enumerate(models)]


def _pool_rows(pool):
    return torch_bits(pool.b16[:, : pool.layout.n_b16])


_CENT = {"degree": {0: 0.3, 1: 0.5, 2: 0.2, 3: 0.7, 4: 0.4}}


@pytest.mark.parametrize("softmax", [True, False])
def test_sim_centrality_app_call(cuda, monkeypatch, softmax):
    """sim_centrality_module_avg on bf16 pool-bound models of a 5-client ring: the weights it gives
    to aggregate_models are weights.sim_centrality on the oracle's similarities, and the client's
    state after the call is aggregate_models' with those weights."""
    import src.decentralized_client as dc

    pool, layout, segs, clients = _ring(cuda)
    before = _pool_rows(pool)
    me, nbrs = 0, [1, 4]
    order = nbrs + [me]
    # unbound copies of the operands, for the expected state
    copies = {}
    for k in order:
        torch.manual_seed(0)
        c = TinyNet().to(torch.bfloat16).to(cuda)
        c.load_state_dict({n: t.clone() for n, t in clients[k].model.state_dict().items()})
        copies[k] = c
    seen = []
    real = dc.aggregate_models

    def spy(operands, w, target, *a, **kw):
        seen.append((list(operands), [float(x) for x in w], target))
        return real(operands, w, target, *a, **kw)

    monkeypatch.setattr(dc, "aggregate_models", spy)
    futures = [(["r"], clients[k]) for k in order]
    res = dc.sim_centrality_module_avg(futures[-1], 0, *futures, centrality_metric="degree", centrality_dict=_CENT,
                                       softmax=softmax, softmax_coeff=10.0).result()
    assert res[1] is clients[me] and len(seen) == 1
    operands, w, target = seen[0]
    assert [id(m) for m in operands] == [id(clients[k].model) for k in order] and target is clients[me].model
    sims = {k: float(ref(before[me], before[k], segs, _threads())) for k in nbrs}
    want, _ = W.sim_centrality(order, me, _CENT["degree"], sims, softmax, 10.0)
    assert w == [float(x) for x in want]
    aggregate_models([copies[k] for k in order], w, copies[me])
    got_sd, want_sd = clients[me].model.state_dict(), copies[me].state_dict()
    for name in want_sd:
        a, b = got_sd[name].detach().cpu(), want_sd[name].detach().cpu()
        assert a.dtype == b.dtype
        if a.dtype == torch.bfloat16:
            assert np.array_equal(torch_bits(a), torch_bits(b)), name
        else:
            assert torch.equal(a, b), name
    after = _pool_rows(pool)
    assert np.array_equal(after[1:], before[1:]) and not np.array_equal(after[0], before[0])


def test_batched_sim_round(cuda, monkeypatch):
    """The batched `*_sim` round (TAL_BATCHED_ROUND=1: DecentrallearnApp._batched_aggregation) on
    bf16 pool-bound models: one similarity.cosine_round call for the round and no cosine_pairs
    call; its values are the per-client cosine_pairs values (and the oracle's); the weights the
    round launches with are sim_centrality's on them."""
    import src.decentralized_app as da
    import src.decentralized_client as dc
    from topology_aware_learning_amd.round import RoundExecutor

    pool, layout, segs, clients = _ring(cuda)
    before = _pool_rows(pool)
    nbrs = {k: sorted([(k - 1) % 5, (k + 1) % 5]) for k in range(5)}
    per_client = {k: similarity.cosine_pairs(clients[k].model, [clients[j].model for j in nbrs[k]]) for k in range(5)}
    for k in range(5):
        assert bits(per_client[k]) == bits([ref(before[k], before[j], segs, _threads()) for j in nbrs[k]])
    seen = {"round": [], "pairs": 0, "runs": []}
    real_round, real_pairs = similarity.cosine_round, dc.cosine_pairs

    def spy_round(p, pairs, model):
        vals = real_round(p, pairs, model)
        seen["round"].append((list(pairs), list(vals)))
        return vals

    def spy_pairs(model, others):
        seen["pairs"] += 1
        return real_pairs(model, others)

    real_run = RoundExecutor.run

    def spy_run(self, orders, weights, out_rows=None, sequential=False, plan=None):
        seen["runs"].append(([list(o) for o in orders], [list(w) for w in weights], list(out_rows)))
        return real_run(self, orders, weights, out_rows, sequential, plan)

    monkeypatch.setattr(similarity, "cosine_round", spy_round)
    monkeypatch.setattr(dc, "cosine_pairs", spy_pairs)
    monkeypatch.setattr(RoundExecutor, "run", spy_run)
    app = object.__new__(da.DecentrallearnApp)
    app.pool, app.clients, app.seed = pool, clients, 0
    app.aggregation_function, app.centrality_metric = da.STRATEGIES["degCent_sim"]
    app._executor, app._round_cache, app.round_cache_hits = None, {}, 0
    nxt = {k: {"train": (["r"], clients[k])} for k in range(5)}
    kw = dict(centrality_metric="degree", centrality_dict=_CENT, softmax=True, softmax_coeff=10.0)
    batch = [(k, k, nxt[k]["train"], tuple(nbrs[k] + [k]), kw) for k in range(5)]
    done = app._batched_aggregation(batch, nxt)
    assert len(done) == 5 and all(d[1] is c for d, c in zip(done, clients))
    assert len(seen["round"]) == 1 and seen["pairs"] == 0 and len(seen["runs"]) == 1
    pairs, vals = seen["round"][0]
    assert pairs == [(k, j) for k in range(5) for j in nbrs[k]]
    assert bits(vals) == bits([v for k in range(5) for v in per_client[k]])
    orders, weights, out_rows = seen["runs"][0]
    assert out_rows == list(range(5))
    for k in range(5):
        order = nbrs[k] + [k]
        assert orders[k] == order
        want, _ = W.sim_centrality(order, k, _CENT["degree"], dict(zip(nbrs[k], per_client[k])), True, 10.0)
        assert weights[k] == [float(x) for x in want]
    assert not np.array_equal(_pool_rows(pool), before)  # the round ran on the bf16 rows
