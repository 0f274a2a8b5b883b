"""K2r on the GPU (tal_cosine_round): the cosine similarities of a whole round's ordered pairs
over the rows of one pool - every norm once per model, every unordered pair once - bitwise the
oracle (torch's CPU order, oracle/cosine_oracle.c) for every ordered pair: the shape families of
test_gpu_cosine_staged.py at every 4-byte offset, pair groups and scratch batches, the plan's
thread word, a whole ResNet-50, a non-default stream, and the batched `*_sim` round of the driver
(one similarity.cosine_round per round, no per-client cosine_pairs).
Reference: cosine_similarity / sim_centrality_module_avg, src/decentralized_client.py:452-550,
661-681 of the reference.
"""
from __future__ import annotations

import networkx as nx
import numpy as np
import pytest
import torch

import oracle
from oracle import reference_alg as ra
from topology_aware_learning_amd import ops, synth
from topology_aware_learning_amd import weights as W
from topology_aware_learning_amd.arena import StateLayout, bound_row
from topology_aware_learning_amd.round import RoundExecutor

pytestmark = pytest.mark.gpu

# (A, I, B) as in test_gpu_cosine_staged.py: column kind B > 1, row kind B == 1
_SHAPES = [
    (64, 3, 9), (61, 3, 9),            # conv1: 28 slabs per chunk, the last chunk partial
    (8, 512, 9), (3, 511, 9),          # one slab per chunk (4,608 floats: the capacity); 511: a partial run
    (6, 256, 9), (5, 128, 9), (9, 64, 9),
    (4, 100, 2), (3, 37, 31), (2, 148, 31),  # B 2 / 31; 148 x 31 = 4,588
    (3, 4609, 1), (2, 513, 9),         # one element past the capacity: the direct form
    (5, 4608, 1), (7, 2048, 1), (33, 512, 1),
    (40, 7, 1), (9, 8, 1), (11, 13, 1), (6, 100, 1), (3, 1030, 1),
    (2, 1024, 9), (1, 16400, 3), (3, 1001, 5), (2, 70, 28), (5, 33, 14), (4, 2, 7), (3, 50, 32),
]


def _models(rng, segs, n):
    total = max(o + a * i * b for o, a, i, b in segs)
    return [rng.standard_normal(total).astype(np.float32) for _ in range(n)]


def _pool(cuda, rows, row_of, pad=29):
    """The models as rows row_of[m] of a device pool whose pitch exceeds the row."""
    n = len(rows[0])
    pool = torch.zeros(max(row_of) + 1, n + pad, device=cuda)
    for m, r in enumerate(row_of):
        pool[r, :n] = torch.from_numpy(rows[m]).to(cuda)
    return pool[:, :n]


def _refs(rows, segs, pairs, threads=1):
    """The oracle's value of every ordered pair, each unordered pair evaluated once (the oracle is
    symmetric bit for bit: tests/test_cosine_round.py)."""
    memo = {}
    for a, b in pairs:
        k = (min(a, b), max(a, b))
        if k not in memo:
            memo[k] = np.float32(oracle.cosine_model(rows[k[0]], rows[k[1]], segs, threads=threads))
    return [memo[(min(a, b), max(a, b))] for a, b in pairs]


def _bits(v):
    return [int(np.float32(x).view(np.uint32)) for x in v]


def _check(cuda, rows, segs, pairs, row_of, threads=1, **kw):
    pool = _pool(cuda, rows, row_of)
    plan = ops.build_cosine_plan(segs, threads=threads)
    got = ops.cosine_round(pool, [(row_of[a], row_of[b]) for a, b in pairs], plan, **kw).cpu().numpy()
    ref = _refs(rows, segs, pairs, threads)
    assert _bits(got) == _bits(ref), (segs[:3], [(p, g, r) for p, g, r in zip(pairs, got, ref) if g != r][:4])
    return pool, plan, got


_PAIRS = [(0, 1), (1, 0), (0, 2), (0, 3), (0, 4), (2, 3), (3, 2), (4, 1), (1, 1), (0, 1)]


@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mis", [0, 1, 3])
def test_round_shapes_vs_oracle(cuda, shape, mis):
    """One tensor per plan, its segment `mis` floats past a 16-byte boundary; 5 models as rows
    out of order; both directions, a repeated pair and a self pair."""
    a, i, b = shape
    segs = [(mis, a, i, b)]
    rows = _models(np.random.default_rng(a * 1000 + i * 10 + b + mis), segs, 5)
    _check(cuda, rows, segs, _PAIRS, row_of=[3, 0, 5, 1, 4])


def test_round_all_shapes_one_plan(cuda):
    """Every shape in one model at odd offsets, all 30 ordered pairs of 6 models: the oracle's
    bits, and ops.cosine's on the same pairs."""
    segs, off = [], 5
    for a, i, b in _SHAPES:
        segs.append((off, a, i, b))
        off += a * i * b + 3
    rows = _models(np.random.default_rng(11), segs, 6)
    pairs = [(a, b) for a in range(6) for b in range(6) if a != b]
    row_of = [4, 2, 6, 0, 1, 5]
    pool, plan, got = _check(cuda, rows, segs, pairs, row_of)
    per_call = ops.cosine([pool[row_of[a]] for a, _ in pairs], [pool[row_of[b]] for _, b in pairs], plan).cpu().numpy()
    assert _bits(got) == _bits(per_call)


def test_round_groups_and_batches(cuda):
    """A star of one row against 12 others (two groups) and a 3-regular graph on 40 rows in both
    directions; once in one batch, once under a budget that forces at least 3."""
    segs = [(0, 8, 64, 9), (4608, 16, 72, 1), (4608 + 1152, 30, 1, 1)]
    rows = _models(np.random.default_rng(5), segs, 41)
    g = nx.random_regular_graph(3, 40, seed=4)
    pairs = [(0, r) for r in range(1, 13)]
    for u, v in g.edges():
        pairs += [(u + 1, v + 1), (v + 1, u + 1)]
    assert len(pairs) == 12 + 120
    row_of = list(np.random.default_rng(6).permutation(41))
    table = ops.build_cosine_round([(row_of[a], row_of[b]) for a, b in pairs], 41)
    ref = _refs(rows, segs, pairs)
    pool = _pool(cuda, rows, row_of)
    plan = ops.build_cosine_plan(segs)
    got = ops.cosine_round(pool, table, plan).cpu().numpy()
    assert table.info.n_batches == 1 and table.info.batch_pairs == table.info.n_unique
    assert _bits(got) == _bits(ref)
    n_out, n_seg = int(plan.host[1]), plan.n_seg
    fixed = 4 * (table.info.n_models * n_out + table.info.n_unique)
    budget = fixed + 4 * (n_out + n_seg) * (table.info.n_unique // 3)
    got = ops.cosine_round(pool, table, plan, budget_bytes=budget).cpu().numpy()
    assert table.info.n_batches >= 3 and table.info.batch_pairs <= table.info.n_unique // 3
    assert _bits(got) == _bits(ref)
    with pytest.raises(ValueError, match="budget"):
        ops.cosine_round(pool, table, plan, budget_bytes=fixed)


# the direct kinds: row (B == 1), element (I == 1) and columns with B >= 32; the last shape's one
# chunk is a streamed one
_DIRECT_SHAPES = [(33, 7, 1), (5, 13, 1), (3, 100, 1), (2, 1030, 1), (300, 1, 1), (3, 50, 32), (2, 37, 40), (2, 513, 9)]


@pytest.fixture(scope="module")
def star_rows():
    """One plan of the direct shapes at odd offsets; 9 models as float32 rows, and 9 as bf16 bit
    patterns with their exact float32 values (what the oracle runs on)."""
    segs, off = [], 3
    for a, i, b in _DIRECT_SHAPES:
        segs.append((off, a, i, b))
        off += a * i * b + 5
    f32 = _models(np.random.default_rng(31), segs, 9)
    b16 = [oracle.f32_to_bf16(r) for r in _models(np.random.default_rng(32), segs, 9)]
    return segs, {"float32": (f32, f32), "bfloat16": (b16, [oracle.bf16_to_f32(r).astype(np.float32) for r in b16])}


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("k", range(1, 9))
def test_round_star_group_sizes(cuda, star_rows, k, dtype):
    """One row against k others, one pair group of k pairs: the row kind takes a group's pairs
    four, two and one at a time, so k = 5, 6, 7 are its 4 + 1, 4 + 2 and 4 + 2 + 1 paths, and
    ops.cosine takes every pair through the one-pair form of the same function.  Both are the
    oracle's bits for every pair."""
    segs, by_dtype = star_rows
    rows, wide = by_dtype[dtype]
    n, row_of = len(rows[0]), [4, 0, 7, 2, 8, 1, 6, 3, 5]
    pool = torch.zeros(9, (n + 29) | 1, dtype=getattr(torch, dtype), device=cuda)[:, :n]
    for m, r in enumerate(row_of):
        t = torch.from_numpy(rows[m].view(np.int16)).view(torch.bfloat16) if dtype == "bfloat16" else torch.from_numpy(rows[m])
        pool[r].copy_(t.to(cuda))
    pairs = [(0, m) for m in range(1, k + 1)]
    on_pool = [(row_of[a], row_of[b]) for a, b in pairs]
    plan = ops.build_cosine_plan(segs)
    table = ops.build_cosine_round(on_pool, 9)
    assert table.info.n_groups == 1 and table.info.max_group == k
    want = _bits(_refs(wide, segs, pairs))
    assert _bits(ops.cosine_round(pool, table, plan).cpu().numpy()) == want
    per_call = ops.cosine([pool[a] for a, _ in on_pool], [pool[b] for _, b in on_pool], plan)
    assert _bits(per_call.cpu().numpy()) == want


@pytest.mark.parametrize("threads", [1, 3, 8])
def test_round_thread_word(cuda, threads):
    """A tensor mean over 196,608 outputs follows torch's two-pass order for the plan's thread
    count, as tal_cosine_params does."""
    segs = [(0, 768, 3, 256), (768 * 3 * 256 + 1, 40, 7, 1)]
    rows = _models(np.random.default_rng(8), segs, 3)
    _check(cuda, rows, segs, [(0, 1), (1, 0), (1, 2)], row_of=[2, 0, 1], threads=threads)


def test_round_resnet50_model(cuda):
    """A whole ResNet-50 parameter set, 4 models on a 4-ring in both directions."""
    lay = synth.get_layout("resnet50")
    layout = StateLayout.from_layout(lay)
    segs = layout.param_segments(synth.param_names(lay))
    flat = []
    for s in (9300, 9301, 9302, 9303):
        sd = synth.synth_state_dict(lay, s)
        flat.append(torch.cat([v.reshape(-1) for (n, _, d), v in zip(lay, sd.values()) if d == "float32"]).numpy())
    pairs = []
    for a in range(4):
        pairs += [(a, (a + 1) % 4), ((a + 1) % 4, a)]
    _check(cuda, flat, segs, pairs, row_of=[2, 0, 3, 1])


def test_round_on_a_side_stream(cuda):
    """Every launch runs on the caller's stream: the pool is filled and the round computed on a
    non-default stream, and the result read after synchronising that stream only."""
    segs, off = [], 1
    for a, i, b in [(8, 512, 9), (33, 512, 1), (61, 3, 9), (40, 7, 1), (30, 1, 1)]:
        segs.append((off, a, i, b))
        off += a * i * b + 5
    rows = _models(np.random.default_rng(21), segs, 4)
    pairs = [(0, 1), (1, 0), (2, 3), (3, 1), (0, 3)]
    ref = _refs(rows, segs, pairs)
    plan = ops.build_cosine_plan(segs)
    host = torch.from_numpy(np.stack(rows)).pin_memory()
    pool = torch.zeros(4, host.shape[1] + 12, device=cuda)
    torch.cuda.synchronize(cuda)
    s = torch.cuda.Stream(cuda)
    with torch.cuda.stream(s):
        pool[:, : host.shape[1]].copy_(host, non_blocking=True)
        out = ops.cosine_round(pool[:, : host.shape[1]], pairs, plan)
        back = torch.empty(len(pairs), dtype=torch.float32).pin_memory()
        back.copy_(out, non_blocking=True)
    s.synchronize()
    assert _bits(back.numpy()) == _bits(ref)
    out2 = ops.cosine_round(pool[:, : host.shape[1]], pairs, plan, stream=s)
    s.synchronize()
    assert _bits(out2.cpu().numpy()) == _bits(ref)


@pytest.mark.parametrize("strategy", ["degCent_sim", "betCent_sim"])
def test_driver_batched_round_sim(cuda, tmp_path, monkeypatch, strategy):
    """TAL_BATCHED_ROUND=1 with a `*_sim` strategy: one similarity.cosine_round per round and no
    cosine_pairs; every row's weights are sim_centrality's for the oracle's similarities of the
    pool as it was after training (so the softmax coefficient's sign follows the least similar
    neighbor); the pool after the launch is the oracle's snapshot round."""
    monkeypatch.setenv("TAL_SYNTHETIC_DATA", "1")
    monkeypatch.setenv("TAL_SYNTHETIC_SAMPLES", "64")
    monkeypatch.setenv("TAL_BATCHED_ROUND", "1")
    import src.decentralized_app as da
    import src.decentralized_client as dc
    from topology_aware_learning_amd import similarity

    seen = {"round_calls": 0, "pair_calls": 0, "batches": [], "runs": 0, "signs": {}}
    real_round, real_pairs = similarity.cosine_round, dc.cosine_pairs

    def spy_round(pool, pairs, model):
        seen["round_calls"] += 1
        return real_round(pool, pairs, model)

    def spy_pairs(model, others):
        seen["pair_calls"] += 1
        return real_pairs(model, others)

    monkeypatch.setattr(similarity, "cosine_round", spy_round)
    monkeypatch.setattr(dc, "cosine_pairs", spy_pairs)
    real_batched = da.DecentrallearnApp._batched_aggregation

    def spy_batched(self, batch, nxt):
        seen["batches"].append((self, list(batch)))
        return real_batched(self, batch, nxt)

    monkeypatch.setattr(da.DecentrallearnApp, "_batched_aggregation", spy_batched)
    real_run = RoundExecutor.run

    def checked_run(self, orders, weights, out_rows=None, sequential=False, plan=None):
        app, batch = seen["batches"][-1]
        lay = self.pool.layout
        f_in = self.pool.f32[:, : lay.n_f32].cpu().numpy().copy()
        i_in = self.pool.i64[:, : lay.n_i64].cpu().numpy().copy()
        real_run(self, orders, weights, out_rows, sequential, plan)
        rp, col, w = ra.round_csr(orders, weights)
        ref = oracle.round_f32(f_in, rp, col, w, np.asarray(out_rows))
        iref = oracle.round_i64(i_in, rp, col, w, np.asarray(out_rows))
        assert np.array_equal(self.pool.f32[:, : lay.n_f32].cpu().numpy().view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(self.pool.i64[:, : lay.n_i64].cpu().numpy(), iref)
        # the weights: sim_centrality over the oracle's similarities of the rows before the run
        row = {c.idx: bound_row(c.model)[1] for c in app.clients}
        names = [n for n, _ in app.clients[0].model.named_parameters()]
        segs = lay.param_segments(names)
        threads = max(1, min(torch.get_num_threads(), 1024))
        assert len(batch) == len(orders) == 10
        for (_, idx, _, idxs, kw), order, wts, out_row in zip(batch, orders, weights, out_rows):
            assert list(order) == [row[i] for i in idxs] and out_row == row[idx] and idxs[-1] == idx
            sims = {i: float(oracle.cosine_model(f_in[row[idx]], f_in[row[i]], segs, threads=threads))
                    for i in idxs if i != idx}
            cent = kw["centrality_dict"][kw["centrality_metric"]]
            want, coeff = W.sim_centrality(list(idxs), idx, cent, sims, True, kw["softmax_coeff"])
            assert [float(x) for x in wts] == [float(x) for x in want], (idx, wts, want)
            seen["signs"].setdefault(idx, []).append(coeff)
        seen["runs"] += 1

    monkeypatch.setattr(RoundExecutor, "run", checked_run)
    topo = tmp_path / "barbell.txt"
    np.savetxt(topo, nx.to_numpy_array(nx.barbell_graph(4, 2)), fmt="%d")
    from src.experiments import decentralized_main

    rc = decentralized_main.main(["--dataset", "cifar10", "--aggregation_strategy", strategy, "--softmax", "--rounds",
                                  "2", "--epochs", "1", "--topology_file", str(topo), "--out_dir",
                                  str(tmp_path / "logs"), "--batch_size", "32"])
    assert rc == 0 and seen["runs"] == 2
    assert seen["round_calls"] == 2 and seen["pair_calls"] == 0
    assert seen["batches"][-1][0].round_cache_hits == 0  # _round_key stays None for these strategies
    if strategy == "degCent_sim":
        # client 3 (degree 4) has only lower-degree neighbors, client 4 (degree 2) none: the
        # graph fixes these two signs whatever the similarities are
        assert all(c < 0 for c in seen["signs"][3]) and all(c > 0 for c in seen["signs"][4])
