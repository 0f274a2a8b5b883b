"""K3q on the GPU (tal_agg_round_seq_f32 / _bf16 / _i64): the sequential round in one launch, in
place, bit for bit the row-by-row oracle (tests/_seq.py) - every graph, row order, participation,
width, layout and input kind of the list below - and bit for bit RoundExecutor's K1 loop, with the
dispatch counted."""
import json

import networkx as nx
import numpy as np
import pytest
import torch

import oracle
from oracle import reference_alg as ra
from topology_aware_learning_amd import _lib, ops
from topology_aware_learning_amd.arena import ModelPool, StateLayout
from topology_aware_learning_amd.round import RoundExecutor, csr_from_lists

from _clique import MODES, bits, count, inputs, np_dtype, round_of, same, tdtype, to_dev
from _seq import csr, graph, sequential_oracle
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

WIDTHS = (1, 63, 64, 65, 130, 1003)  # one lane, a tile less one, a tile, a tile and one, three tiles, 16 tiles
ORDERS = ("ascending", "reversed", "permuted")
LAYOUTS = ("contiguous", "padded", "offset")
SENTINEL = {False: 0x7FC0BEEF, True: 0x7FCE}
# (graph, the rows' order hook): star 17 runs with the hub first and with the hub last
GRAPHS = ("ring4", "ring8", "star17 hub first", "star17 hub last", "ba33", "rr64", "barbell12_4", "complete9")
K1_ENTRIES = ("tal_agg_f32", "tal_agg_bf16", "tal_agg_i64", "tal_agg_model_f32")
SEQ_ENTRIES = ("tal_agg_round_seq_f32", "tal_agg_round_seq_bf16", "tal_agg_round_seq_i64")


def _who(name, g, order, thirds):
    """The rows that aggregate, in sweep order."""
    nodes = sorted(g.nodes)
    if thirds:
        nodes = [i for i in nodes if i % 3 != 2]  # every third row is a source only
    if order == "reversed":
        nodes = nodes[::-1]
    elif order == "permuted":
        nodes = np.random.default_rng(len(nodes)).permutation(nodes).tolist()
    if name.startswith("star17"):  # the hub (node 0, read by every row) first or last, whatever the order
        nodes = [i for i in nodes if i != 0]
        nodes = [0] + nodes if name.endswith("first") else nodes + [0]
    return nodes


def _device_pool(pool, layout, bf16, dev):
    """(device view [rows + 1, n or ld], ld): the pool's rows plus one row no plan names, padding
    and extra row filled with the sentinel."""
    rows, n = pool.shape
    ld = n if layout == "contiguous" else n + 3 - n % 2  # odd
    host = np.full((rows + 1, ld), SENTINEL[bf16], np_dtype(bf16))
    host[:rows, :n] = pool
    if layout != "offset":
        return to_dev(host, bf16, dev), host
    flat = torch.empty((rows + 1) * ld + 1, dtype=tdtype(bf16), device=dev)
    view = flat[1:].view(rows + 1, ld)  # one element past the allocation's alignment
    view.copy_(to_dev(host, bf16, dev))
    assert view.data_ptr() % (4 if bf16 else 8) != 0
    return view, host


def _run(pool_dev, plan, n, bf16, mode):
    (ops.round_seq_bf16 if bf16 else ops.round_seq_f32)(pool_dev, plan, n=n, mode=mode)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", MODES, ids=["exact", "fma"])
@pytest.mark.parametrize("name", GRAPHS)
def test_kernel_vs_oracle(cuda, name, mode, bf16):
    """Every width; orders, participation, layouts and weight kinds rotate over the widths so that
    each graph meets each of them, and over the graphs so that the pairings differ."""
    g = graph(name.split()[0])
    gi = GRAPHS.index(name)
    exact = mode == ops.MODE_EXACT
    seen = set()
    for k, n in enumerate(WIDTHS):
        order, layout = ORDERS[(k + gi) % 3], LAYOUTS[(k // 2 + gi) % 3]
        thirds, kind = bool((k + gi) % 2), ("signed", "uniform")[(k // 3 + gi) % 2]
        seen.add((order, layout, thirds, kind))
        who = _who(name, g, order, thirds)
        orders, ws = round_of(g, kind, who=who, n=n)
        pool, _ = inputs(len(g), n, seed=100 * gi + k, bf16=bf16)
        ref = sequential_oracle(pool, orders, ws, who, "bf16" if bf16 else "f32", exact=exact)
        plan = ops.build_seq_plan(*csr(orders, ws), np.asarray(who, np.int32))
        dev, host = _device_pool(pool, layout, bf16, cuda)
        _run(dev, plan, n, bf16, mode)
        got = bits(dev)
        assert same(got[: len(g), :n], ref, nan_payloads_free=not bf16), (name, n, order, layout, thirds, kind)
        # rows the round does not write, the row no plan names and the padding keep their bits
        idle = sorted(set(range(len(g) + 1)) - set(who))
        assert np.array_equal(got[idle], host[idle]) and np.array_equal(got[:, n:], host[:, n:]), (name, n, layout)
    assert len({s[0] for s in seen}) == 3 and len({s[1] for s in seen}) == 3
    assert len({s[2] for s in seen}) == 2 and len({s[3] for s in seen}) == 2


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", MODES, ids=["exact", "fma"])
def test_duplicate_operands_long_rows_and_rows_read_by_nobody(cuda, mode, bf16):
    """What the graphs above do not have: a source twice in a row, rows of 1, 9, 10, 17 and 18
    operands (the batch of eight's edges), an output row no row reads (out_slot -1), self first."""
    rng = np.random.default_rng(7)
    n, rows = 131, 24
    orders = [[3], [0, 1, 0, 2], [2] + list(range(8)), list(range(10)), [4] + list(range(16)),
              list(range(17, -1, -1)), [5, 6]]
    who = [0, 1, 2, 20, 3, 21, 4]  # rows 20 and 21 are read by nobody
    ws = [(rng.standard_normal(len(o)) * 0.4).tolist() for o in orders]
    pool, _ = inputs(rows, n, seed=5, bf16=bf16)
    plan = ops.build_seq_plan(*csr(orders, ws), np.asarray(who, np.int32))
    assert plan.host[plan.info.off_out_slot: plan.info.off_out_slot + len(who)].tolist() == [0, 1, 2, -1, 3, -1, 4]
    ref = sequential_oracle(pool, orders, ws, who, "bf16" if bf16 else "f32", exact=mode == ops.MODE_EXACT)
    dev = to_dev(pool, bf16, cuda)
    _run(dev, plan, n, bf16, mode)
    assert same(bits(dev), ref, nan_payloads_free=not bf16)


def test_sequential_differs_from_snapshot_where_it_must(cuda):
    """Ring 8 in index order: row 0 reads only pre-round models, so it equals the snapshot round;
    every later row has a neighbor written before it (row i - 1; row 7 also row 0), so it differs."""
    g = nx.cycle_graph(8)
    orders, ws = round_of(g, "uniform")
    pool = (np.random.default_rng(3).standard_normal((8, 257)) * 3).astype(np.float32)
    rp, col, w = csr(orders, ws)
    snap = oracle.round_f32(pool, rp, col, w, np.arange(8, dtype=np.int32)).view(np.uint32)
    dev = torch.from_numpy(pool).to(cuda)
    ops.round_seq_f32(dev, ops.build_seq_plan(rp, col, w, np.arange(8, dtype=np.int32)))
    got = bits(dev)
    assert np.array_equal(got, sequential_oracle(pool.view(np.uint32), orders, ws, range(8), "f32"))
    assert np.array_equal(got[0], snap[0])
    for r in range(1, 8):
        assert not np.array_equal(got[r], snap[r]), r


def test_int64_counters(cuda):
    """64 rows x 53 columns under 1/9 weights: column 0 holds 1000 everywhere, so row 0's chain is
    nine times fl(1/9) * 1000 = 999.99994 -> 999, and the rows after it read that 999."""
    g = graph("rr64")
    orders = [sorted(g.neighbors(i)) + [i] for i in range(64)]
    ws = [[1.0 / 9] * 9] * 64
    pool = np.random.default_rng(0).integers(-(2 ** 40), 2 ** 40, size=(64, 53)).astype(np.int64)
    pool[:, 0] = 1000
    pool[:, 1] = np.arange(64) * 1000003
    ref = sequential_oracle(pool, orders, ws, range(64), "i64")
    plan = ops.build_seq_plan(*csr(orders, ws), np.arange(64, dtype=np.int32))
    dev = torch.zeros(64, 56, dtype=torch.int64, device=cuda)
    dev[:, 53:] = -7
    dev[:, :53] = torch.from_numpy(pool).to(cuda)
    ops.round_seq_i64(dev, plan, n=53)
    got = dev.cpu().numpy()
    assert np.array_equal(got[:, :53], ref) and np.all(got[:, 53:] == -7)
    assert got[0, 0] == 999 and np.all(got[:, 0] < 1000)  # no later row saw nine 1000s


@pytest.mark.parametrize("mode", MODES, ids=["exact", "fma"])
def test_reference_fixture(cuda, mode):
    """tests/golden/round_4ring.*, written by driving the reference in client order: every entry of
    every client after ops.round_seq_* on a ModelPool (EXACT: bitwise the reference's)."""
    meta = json.loads((GOLDEN / "round_4ring.json").read_text())
    z = np.load(GOLDEN / "round_4ring.npz")
    lay = [(n, tuple(s), d) for n, s, d in meta["layout"]]
    layout = StateLayout.from_layout(lay)
    pool = ModelPool(layout, 4, cuda)
    for i in range(4):
        pool.load_row(i, {n: torch.from_numpy(z[f"in{i}_{n}"]) for n, _, _ in lay})
    orders = meta["orders"]
    ws = [ra.unweighted_weights(len(o)) for o in orders]
    plan = ops.build_seq_plan(*csr(orders, ws), np.arange(4, dtype=np.int32))
    f_in = bits(pool.f32[:, : layout.n_f32])
    ops.round_seq_f32(pool.f32, plan, n=layout.n_f32, mode=mode)
    if layout.n_i64:
        ops.round_seq_i64(pool.i64, plan, n=layout.n_i64)
    if mode == ops.MODE_FMA:  # the fixture pins the reference's arithmetic; FMA mode has the oracle's
        ref = sequential_oracle(f_in, orders, ws, range(4), "f32", exact=False)
        assert same(bits(pool.f32[:, : layout.n_f32]), ref, nan_payloads_free=True)
        return
    for i in range(4):
        sd = pool.state_dict(i)
        for n, _, _ in lay:
            a, b = sd[n].cpu().numpy(), z[f"seq{i}_{n}"]
            if a.dtype == np.float32:
                assert same(a.view(np.uint32).reshape(-1), b.view(np.uint32).reshape(-1), nan_payloads_free=True), (i, n)
            else:
                assert np.array_equal(a, b), (i, n)


# ---- RoundExecutor.run(sequential=True) -----------------------------------------------------------
def _tiny_layout(bf16):
    f = "bfloat16" if bf16 else "float32"
    return StateLayout.from_layout([("conv.weight", (5, 3, 3), f), ("bn.weight", (5,), f), ("bn.running_var", (5,), f),
                                    ("bn.num_batches_tracked", (), "int64"), ("fc.weight", (7, 5), f),
                                    ("bn2.num_batches_tracked", (), "int64")])


def _filled_pool(layout, rows, bf16, dev, seed):
    pool = ModelPool(layout, rows, dev)
    n = layout.n_b16 if bf16 else layout.n_f32
    x, _ = inputs(rows, n, seed=seed, bf16=bf16)
    (pool.b16 if bf16 else pool.f32)[:, :n] = to_dev(x, bf16, dev)
    cnt = np.random.default_rng(seed).integers(0, 5000, size=(rows, layout.n_i64)).astype(np.int64)
    cnt[:, 0] = 1000
    pool.i64[:, : layout.n_i64] = torch.from_numpy(cnt).to(dev)
    return pool, x, cnt


def _segments(pool, bf16):
    lay = pool.layout
    n = lay.n_b16 if bf16 else lay.n_f32
    return bits((pool.b16 if bf16 else pool.f32)[:, :n]), pool.i64[:, : lay.n_i64].cpu().numpy()


def _all_on(monkeypatch, on=True):
    for key in list(ops.SEQ_DEFAULT):
        monkeypatch.setitem(ops.SEQ_DEFAULT, key, on)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", MODES, ids=["exact", "fma"])
@pytest.mark.parametrize("name", ["barbell12_4", "ba33"])
def test_executor_kernel_equals_the_k1_loop(cuda, monkeypatch, name, mode, bf16):
    """sequential=True with the kernel on against sequential="calls" on a tiny model with BN
    counters: every segment bit for bit, and the dispatch counted - one tal_agg_round_seq_* per
    segment and no K1 call with the kernel on; no seq entry with SEQ_DEFAULT off."""
    g = graph(name)
    orders, ws = round_of(g, "degcent")
    layout = _tiny_layout(bf16)
    want_seq = {"tal_agg_round_seq_f32": int(not bf16), "tal_agg_round_seq_bf16": int(bf16), "tal_agg_round_seq_i64": 1}
    results = []
    for form in ("kernel", "calls", "gated off"):
        with monkeypatch.context() as mp:
            _all_on(mp, on=form != "gated off")
            pool, x, cnt = _filled_pool(layout, len(g), bf16, cuda, seed=11)
            ex = RoundExecutor(pool, mode=mode)
            counters = {e: count(mp, e) for e in K1_ENTRIES + SEQ_ENTRIES}
            ex.run(orders, ws, sequential="calls" if form == "calls" else True)
            calls = {e: c.calls for e, c in counters.items()}
        if form == "kernel":
            assert {e: calls[e] for e in SEQ_ENTRIES} == want_seq and not any(calls[e] for e in K1_ENTRIES), calls
        else:
            assert not any(calls[e] for e in SEQ_ENTRIES) and sum(calls[e] for e in K1_ENTRIES) >= len(g), (form, calls)
        assert not ex.swaps and ex.spare is None  # in place on the one pool
        results.append(_segments(pool, bf16))
    for got in results[1:]:
        assert np.array_equal(results[0][0], got[0]) and np.array_equal(results[0][1], got[1])
    exact = mode == ops.MODE_EXACT
    ref = sequential_oracle(x, orders, ws, range(len(g)), "bf16" if bf16 else "f32", exact=exact)
    assert same(results[0][0], ref, nan_payloads_free=not bf16)
    assert np.array_equal(results[0][1], sequential_oracle(cnt, orders, ws, range(len(g)), "i64"))


def test_capacity_fallback(cuda, monkeypatch):
    """Complete 257 at n = 70: more distinct sources than the kernel's tile holds, so the plan does
    not build (TAL_ERR_CAPACITY) and the executor runs the K1 loop; the result is the oracle's."""
    _all_on(monkeypatch)
    m, n = 257, 70
    orders = [[j for j in range(m) if j != i] + [i] for i in range(m)]
    ws = [[1.0 / m] * m] * m
    with pytest.raises(_lib.TalError) as e:
        ops.build_seq_plan(*csr_from_lists(orders, ws), np.arange(m, dtype=np.int32))
    assert e.value.code == _lib.TAL_ERR_CAPACITY
    layout = StateLayout.from_layout([("w", (n,), "float32")])
    pool = ModelPool(layout, m, cuda)
    x = (np.random.default_rng(2).standard_normal((m, n)) * 3).astype(np.float32)
    pool.f32[:, :n] = torch.from_numpy(x).to(cuda)
    seq, k1 = count(monkeypatch, "tal_agg_round_seq_f32"), count(monkeypatch, "tal_agg_f32")
    ex = RoundExecutor(pool)
    ex.run(orders, ws, sequential=True)
    assert seq.calls == 0 and k1.calls == m
    ref = sequential_oracle(x.view(np.uint32), orders, ws, range(m), "f32")
    assert np.array_equal(bits(pool.f32[:, :n]), ref)


def test_repeat_reuses_the_plan(cuda, monkeypatch):
    """A second run with the same lists builds no second plan and continues from the first
    round's result: two oracle sweeps."""
    _all_on(monkeypatch)
    g = graph("ba33")
    orders, ws = round_of(g, "datasize")
    layout = _tiny_layout(False)
    pool, x, cnt = _filled_pool(layout, len(g), False, cuda, seed=4)
    built = count(monkeypatch, "tal_seq_plan_build")
    ex = RoundExecutor(pool)
    ex.run(orders, ws, sequential=True)
    ex.run([list(o) for o in orders], [list(w) for w in ws], list(range(len(g))), sequential=True)
    assert built.calls == 1
    ref, iref = x, cnt
    for _ in range(2):
        ref = sequential_oracle(ref, orders, ws, range(len(g)), "f32")
        iref = sequential_oracle(iref, orders, ws, range(len(g)), "i64")
    got = _segments(pool, False)
    assert same(got[0], ref, nan_payloads_free=True) and np.array_equal(got[1], iref)


def test_argument_checks(cuda):
    g = nx.cycle_graph(4)
    orders, ws = round_of(g, "uniform")
    plan = ops.build_seq_plan(*csr(orders, ws), np.arange(4, dtype=np.int32))
    pool = torch.zeros(4, 8, device=cuda)
    with pytest.raises(ValueError):
        ops.round_seq_f32(pool.cpu(), plan)
    with pytest.raises(ValueError):
        ops.round_seq_bf16(pool, plan)
    with pytest.raises(ValueError):
        ops.round_seq_f32(pool[0], plan)
    with pytest.raises(ValueError):
        ops.round_seq_f32(pool[:, ::2], plan)
    with pytest.raises(ValueError):
        ops.round_seq_f32(pool[:3], plan)
    with pytest.raises(ValueError):
        ops.round_seq_f32(pool, plan, n=9)
    with pytest.raises(TypeError):
        ops.round_seq_f32(pool, ops.build_plan(*csr(orders, ws), np.arange(4, dtype=np.int32)))
    assert ops.round_seq_f32(pool, plan, n=0) is pool
