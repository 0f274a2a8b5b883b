"""K3c1 with per-source weights on the GPU (tal_agg_round_clique_col_w_f32 / _bf16): clique blocks
of 65..128 members whose source j carries the same fp32 weight w_j in every row (the weighted and
centrality apps), one column per lane, bit for bit against
  fp32 EXACT   oracle.round_f32
  fp32 FMA     oracle.round_f32(exact=False), and K1-FMA on three rows
  bf16         oracle.round_bf16 of the mode (NaN stored as 0xFFFF)
plus the Python dispatch of a per-source CliquePlan with a col_wtable: which entries run, that odd
strides and element-offset pools stay on the clique path, the cross-checks against the K3c-w and
the uniform column entries, and a round through RoundExecutor."""
import ctypes

import networkx as nx
import numpy as np
import pytest
import torch

import oracle
from oracle import reference_alg as ra
from topology_aware_learning_amd import _lib, ops
from topology_aware_learning_amd.arena import ModelPool, StateLayout
from topology_aware_learning_amd.round import RoundExecutor

from _clique import (MODES, bits, count, inputs, is_nan, k1_fma, np_dtype, oracle_round, padded, round_of, run, same,
                     sentinel_pool, to_dev)

pytestmark = pytest.mark.gpu

SENTINEL = {False: 0x40E01234, True: 0x1234}  # fp32 / bf16 bits of an untouched output element
WIDE = dict(per_source=True, max_members=128, wide_per_source=True)

_GRAPHS = {
    "complete65": lambda: nx.complete_graph(65),    # MMAX 68; the first member past 64: the second weight batch
    "complete100": lambda: nx.complete_graph(100),  # exact MMAX
    "complete128": lambda: nx.complete_graph(128),  # no padding slot
    "two_blocks": lambda: nx.disjoint_union(nx.complete_graph(70), nx.complete_graph(100)),  # two paddings, two weight records
    "mixed": lambda: nx.disjoint_union(nx.disjoint_union(nx.complete_graph(20), nx.complete_graph(100)),
                                       nx.random_regular_graph(4, 30, seed=1)),  # K3c-w, the new kernel and a rest plan
    "barbell66": lambda: nx.barbell_graph(66, 3),   # bridges through the rest plan
}
# degree-centrality weights are uniform on a lone complete graph: barbell and the mixed graph only
_KINDS = {g: ["datasize", "signed"] + (["degcent"] if g in ("mixed", "barbell66") else []) for g in _GRAPHS}
_CASES = ([(g, k, n) for g in _GRAPHS for k in _KINDS[g] for n in (1, 7, 259)]
          + [(g, k, 4099) for g in ("complete100", "complete128") for k in ("datasize", "signed")])


def _round_of(graph, kind, who=None):
    """Per-source weights of one kind (_clique.round_of)."""
    return round_of(_GRAPHS[graph]() if isinstance(graph, str) else graph, kind, who=who)


def _sentinel_pool(rows, ld, bf16, dev):
    return sentinel_pool(rows, ld, bf16, dev, SENTINEL[bf16])


def _padded(pool, bf16, dev, odd=True):
    return padded(pool, bf16, dev, odd=odd)


def _same(got, ref, bf16):
    """Bit for bit; on fp32 a NaN matches a NaN (payloads are not the oracle's to pin)."""
    return same(got, ref, nan_payloads_free=not bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("graph,kind,n", _CASES)
def test_round_clique_col_weighted_vs_oracle(cuda, graph, kind, n, bf16):
    """Both modes bitwise the oracle's round of the mode, fp32 FMA also K1-FMA on three rows.
    Per-source weights of three kinds, specials, a payload NaN in member 1 (every row reading it is
    NaN there; bf16: 0xFFFF), -0.0 and +-inf columns, output rows permuted and shifted by 2, a
    padded odd stride (even where the plan also holds K3c blocks), and nothing else written."""
    orders, ws = _round_of(graph, kind)
    rows = len(orders)
    csr = ra.round_csr(orders, ws)
    out_rows = (np.random.default_rng(rows).permutation(rows) + 2).astype(np.int32)
    plan = ops.build_clique_plan(*csr, out_rows, bf16=bf16, **WIDE)
    assert plan is not None and plan.n_col >= 1 and plan.col_wtable is not None
    assert (plan.n_cliques > 0) == (graph == "mixed") and (plan.rest is not None) == (graph in ("mixed", "barbell66"))
    pool, nan_col = inputs(rows, n, rows + n, bf16)
    pin = _padded(pool, bf16, cuda, odd=plan.n_cliques == 0)
    for mode in MODES:
        pout = _sentinel_pool(rows + 2, pin.shape[1], bf16, cuda)
        run(pin, pout, plan, n, mode)
        got = bits(pout)
        ref = oracle_round(pool, csr, out_rows - 2, bf16, exact=(mode == ops.MODE_EXACT))
        assert _same(got[2:, :n], ref, bf16), (graph, kind, n, mode)
        if mode == ops.MODE_FMA and not bf16:
            for r in (0, rows // 2, rows - 1):
                assert _same(got[out_rows[r], :n], k1_fma(pin, orders, ws, r, n), bf16), (graph, kind, n, r)
        for r in range(rows):
            if 1 in orders[r]:
                assert is_nan(got[out_rows[r], nan_col], bf16), (r, mode)
        assert np.all(got[:2] == SENTINEL[bf16]) and np.all(got[:, n:] == SENTINEL[bf16])  # nothing else written


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_partial_participation(cuda, bf16):
    """complete(100) under data-size weights with output rows for 37 members: those rows are the
    oracle's, the other 63 rows of the output pool keep their sentinel."""
    n = 259
    who = sorted(np.random.default_rng(5).choice(100, 37, replace=False).tolist())
    orders, ws = _round_of(nx.complete_graph(100), "datasize", who=who)
    csr = ra.round_csr(orders, ws)
    out_rows = np.array(who, dtype=np.int32)
    plan = ops.build_clique_plan(*csr, out_rows, bf16=bf16, **WIDE)
    assert (plan.n_cliques, plan.n_col, plan.col_mmax) == (0, 1, 100) and plan.rest is None
    pool, _ = inputs(100, n, 11, bf16)
    pin = _padded(pool, bf16, cuda)
    for mode in MODES:
        pout = _sentinel_pool(100, pin.shape[1], bf16, cuda)
        run(pin, pout, plan, n, mode)
        got = bits(pout)
        ref = oracle_round(pool, csr, out_rows, bf16, exact=(mode == ops.MODE_EXACT),
                      pool_out=np.full((100, n), SENTINEL[bf16], np_dtype(bf16)))
        assert _same(got[:, :n], ref, bf16), mode
        idle = np.setdiff1d(np.arange(100), who)
        assert len(idle) == 63 and np.all(got[idle] == SENTINEL[bf16]) and np.all(got[:, n:] == SENTINEL[bf16])


def _entry(bf16):
    return getattr(_lib.load(), "tal_agg_round_clique_col_w_bf16" if bf16 else "tal_agg_round_clique_col_w_f32")


def _call_entry(bf16, pin, pout, n, table, n_blocks, mmax, mode, wtab, dev):
    ops.check(_entry(bf16)(ctypes.c_void_p(pin.data_ptr()), pin.stride(0), ctypes.c_void_p(pout.data_ptr()),
                           pout.stride(0), n, ctypes.c_void_p(table.data_ptr()), n_blocks, mmax, int(mode),
                           ops._stream(dev, None), ctypes.c_void_p(wtab.data_ptr())))
    torch.cuda.synchronize()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [7, 259])
def test_small_block_equals_k3c_weighted(cuda, bf16, n):
    """Blocks of <= 64 members are legal input: complete(40) under signed per-source weights, given
    to the new entry as a column record, gives tal_agg_round_clique_w_*'s bits in both modes."""
    orders, ws = _round_of(nx.complete_graph(40), "signed")
    csr = ra.round_csr(orders, ws)
    out_rows = np.arange(40, dtype=np.int32)
    plan = ops.build_clique_plan(*csr, out_rows, bf16=bf16, per_source=True)
    assert plan.n_cliques == 1 and plan.mmax == 40 and plan.rest is None and plan.wtable is not None
    t = plan.table.reshape(1, ops.CLIQUE_WORDS)
    assert t[0, 2] == 0
    c = np.zeros((1, ops.CLIQUE_COL_WORDS), np.int32)
    c[0, 0] = 40
    c[0, 4: 4 + ops.CLIQUE_MAX] = t[0, 4: 4 + ops.CLIQUE_MAX]
    c[0, 4 + ops.CLIQUE_COL_MAX:] = -1
    c[0, 4 + ops.CLIQUE_COL_MAX: 4 + ops.CLIQUE_COL_MAX + ops.CLIQUE_MAX] = t[0, 4 + ops.CLIQUE_MAX: 4 + 2 * ops.CLIQUE_MAX]
    cw = np.ones((1, ops.CLIQUE_COL_WWORDS), np.float32)
    cw[0, :ops.CLIQUE_MAX] = plan.wtable.reshape(1, ops.CLIQUE_WWORDS)[0, :ops.CLIQUE_MAX]
    pool, _ = inputs(40, n, 40 + n, bf16)
    pin = _padded(pool, bf16, cuda, odd=False)
    table = torch.from_numpy(c.reshape(-1)).to(cuda)
    wtab = torch.from_numpy(cw.reshape(-1)).to(cuda)
    for mode in MODES:
        want = _sentinel_pool(40, pin.shape[1], bf16, cuda)
        run(pin, want, plan, n, mode)
        pout = _sentinel_pool(40, pin.shape[1], bf16, cuda)
        _call_entry(bf16, pin, pout, n, table, 1, 40, mode, wtab, cuda)
        assert np.array_equal(bits(pout), bits(want)), mode
        assert _same(bits(want)[:, :n], oracle_round(pool, csr, out_rows, bf16, exact=(mode == ops.MODE_EXACT)), bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [7, 259])
def test_equal_weights_equal_uniform_entry(cuda, bf16, n):
    """A uniform complete(100) round given to the new entry with all 100 weights equal gives
    tal_agg_round_clique_col_*'s bits (negative weights on odd n: FMA's padding differs between
    the two forms, -0.0 under weight 1.0 here, and must not show)."""
    g = nx.complete_graph(100)
    orders = [sorted(g.neighbors(i)) + [i] for i in sorted(g.nodes)]
    ws = [[-1.0 / 100] * 100 for _ in orders]
    csr = ra.round_csr(orders, ws)
    out_rows = np.arange(100, dtype=np.int32)
    uni = ops.build_clique_plan(*csr, out_rows, bf16=bf16, max_members=128)
    assert (uni.n_cliques, uni.n_col) == (0, 1) and uni.col_wtable is None
    per = ops.build_clique_plan(*csr, out_rows, bf16=bf16, **WIDE)
    assert (per.n_cliques, per.n_col) == (0, 1)
    cw = per.col_wtable.reshape(1, ops.CLIQUE_COL_WWORDS)
    assert np.all(cw[0, :100] == np.float32(-0.01)) and np.all(cw[0, 100:] == 1.0)
    pool, _ = inputs(100, n, 17 + n, bf16)
    pin = _padded(pool, bf16, cuda)
    table = torch.from_numpy(uni.col_table).to(cuda)  # the uniform record: its weight word is ignored
    wtab = torch.from_numpy(per.col_wtable).to(cuda)
    for mode in MODES:
        want = _sentinel_pool(100, pin.shape[1], bf16, cuda)
        run(pin, want, uni, n, mode)
        pout = _sentinel_pool(100, pin.shape[1], bf16, cuda)
        _call_entry(bf16, pin, pout, n, table, 1, 100, mode, wtab, cuda)
        assert np.array_equal(bits(pout), bits(want)), mode
        via_plan = _sentinel_pool(100, pin.shape[1], bf16, cuda)
        run(pin, via_plan, per, n, mode)
        assert np.array_equal(bits(via_plan), bits(want)), mode


def _entries(monkeypatch, bf16):
    """Counters: the new entry, K3c-w, the regular round, the uniform column entry, uniform K3c."""
    t = "bf16" if bf16 else "f32"
    return [count(monkeypatch, f"tal_agg_round_{k}{t}") for k in ("clique_col_w_", "clique_w_", "", "clique_col_", "clique_")]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
def test_dispatch_counts(cuda, monkeypatch, bf16, mode):
    """complete(100) under data-size weights: the new entry once, the column, K3c and regular
    entries never; the mixed round: the new entry, K3c-w and the regular entry once each.  In place
    is a ValueError with no launch."""
    n = 259
    cs = _entries(monkeypatch, bf16)
    for graph, want in (("complete100", (1, 0, 0, 0, 0)), ("mixed", (1, 1, 1, 0, 0))):
        orders, ws = _round_of(graph, "datasize")
        rows = len(orders)
        csr = ra.round_csr(orders, ws)
        out_rows = np.arange(rows, dtype=np.int32)
        plan = ops.plan_from_spec(*csr, out_rows, {"wclique": 1, "members": 128, "rest": None})
        assert plan.col_wtable is not None and ops.round_kernel_name(plan) == (
            "k_round_clique" if graph == "mixed" else "k_round_clique_col")
        pool, _ = inputs(rows, n, 3, bf16)
        pin = _padded(pool, bf16, cuda, odd=False)
        pout = torch.zeros_like(pin)
        before = [c.calls for c in cs]
        run(pin, pout, plan, n, mode)
        assert tuple(c.calls - b for c, b in zip(cs, before)) == want, graph
        assert _same(bits(pout)[:, :n], oracle_round(pool, csr, out_rows, bf16, exact=(mode == ops.MODE_EXACT)), bf16)
        with pytest.raises(ValueError):
            run(pin, pin, plan, n, mode)
        assert tuple(c.calls - b for c, b in zip(cs, before)) == want


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
def test_unaligned_pools_stay_on_the_clique_path(cuda, monkeypatch, bf16, mode):
    """An odd row stride and pools that start one element (4 B / 2 B) into an aligned buffer: the
    new entry runs (no fallback to plan.full, whose entry is never called) and gives the aligned
    run's bits."""
    n = 259
    orders, ws = _round_of("complete100", "datasize")
    csr = ra.round_csr(orders, ws)
    out_rows = np.arange(100, dtype=np.int32)
    plan = ops.build_clique_plan(*csr, out_rows, bf16=bf16, **WIDE)
    pool, _ = inputs(100, n, 9, bf16)
    aligned = _padded(pool, bf16, cuda, odd=False)
    want = torch.zeros_like(aligned)
    run(aligned, want, plan, n, mode)
    want = bits(want)[:, :n]
    assert _same(want, oracle_round(pool, csr, out_rows, bf16, exact=(mode == ops.MODE_EXACT)), bf16)
    cs = _entries(monkeypatch, bf16)
    ld = aligned.shape[1] + 1  # odd
    assert ld % 2 == 1
    esize = aligned.element_size()
    src = torch.zeros(100 * ld + 1, dtype=aligned.dtype, device=cuda)[1:].view(100, ld)
    dst = torch.zeros(100 * ld + 1, dtype=aligned.dtype, device=cuda)[1:].view(100, ld)
    assert src.data_ptr() % (2 * esize) == esize and dst.data_ptr() % (2 * esize) == esize
    src[:, : aligned.shape[1]] = aligned
    run(src, dst, plan, n, mode)
    assert np.array_equal(bits(dst)[:, :n], want)
    assert tuple(c.calls for c in cs) == (1, 0, 0, 0, 0)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_round_executor_complete66(cuda, monkeypatch, bf16):
    """RoundExecutor on a small ModelPool, complete(66) under data-size weights, with the plan of
    spec {"wclique": 1, "members": 128}: every row equals the oracle round on the pre-round
    snapshot, and exactly one call of the new entry ran."""
    n = 1001
    layout = StateLayout.from_layout([("w", (n,), "bfloat16" if bf16 else "float32")])
    orders, ws = _round_of(nx.complete_graph(66), "datasize")
    csr = ra.round_csr(orders, ws)
    out_rows = np.arange(66, dtype=np.int32)
    plan = ops.plan_from_spec(*csr, out_rows, {"wclique": 1, "members": 128}).to(cuda)
    assert (plan.n_cliques, plan.n_col, plan.col_mmax) == (0, 1, 66) and plan.rest is None
    plan.rest_rows = None  # every row aggregates: nothing to carry into the spare (RoundExecutor.plan's form)
    pool = ModelPool(layout, 66, cuda)
    seg = pool.b16 if bf16 else pool.f32
    before, _ = inputs(66, n, 4, bf16)
    seg[:, :n].copy_(to_dev(before, bf16, cuda))
    new = count(monkeypatch, "tal_agg_round_clique_col_w_" + ("bf16" if bf16 else "f32"))
    ex = RoundExecutor(pool, mode=ops.MODE_EXACT, placement_trials=1)  # no placement runs: the round alone
    ex.run(orders, ws, plan=plan)
    seg = pool.b16 if bf16 else pool.f32
    assert _same(bits(seg[:, :n]), oracle_round(before, csr, out_rows, bf16), bf16)
    assert new.calls == 1
