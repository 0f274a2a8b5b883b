"""K3c1 on the GPU (tal_agg_round_clique_col_f32 / _bf16): clique blocks of 65..128 members,
one column per lane, bit for bit against the C oracle's rounds (EXACT on fp32 and bf16, FMA on
bf16) and against K1 in FMA mode, plus the Python dispatch of a CliquePlan with a col_table:
which entries run, that odd strides and element-offset pools stay on the clique path, and that
blocks of <= 64 members give K3c's bits."""
import ctypes

import networkx as nx
import numpy as np
import pytest
import torch

import oracle
from oracle import reference_alg as ra
from topology_aware_learning_amd import _lib, ops

from _clique import (MODES, bits, count, inputs, is_nan, k1_fma, np_dtype, oracle_round, padded, round_of, run, same,
                     sentinel_pool, tdtype)

pytestmark = pytest.mark.gpu

SENTINEL = {False: 0x40E01234, True: 0x1234}  # fp32 / bf16 bits of an untouched output element

_GRAPHS = {
    "complete65": lambda: nx.complete_graph(65),    # the smallest block past 64: MMAX 68, a row group of one
    "complete100": lambda: nx.complete_graph(100),  # exact MMAX
    "complete128": lambda: nx.complete_graph(128),  # the largest block
    "two_blocks": lambda: nx.disjoint_union(nx.complete_graph(70), nx.complete_graph(100)),  # two paddings, one MMAX
    "mixed": lambda: nx.disjoint_union(nx.disjoint_union(nx.complete_graph(20), nx.complete_graph(100)),
                                       nx.random_regular_graph(4, 30, seed=1)),  # K3c, K3c1 and a rest plan
    "barbell66": lambda: nx.barbell_graph(66, 3),   # bridges through the rest plan, reading clique members
}
_CASES = [(g, n) for g in _GRAPHS for n in (1, 7, 259)] + [("complete100", 4099), ("complete128", 4099)]


def _round_of(graph, n, who=None):
    """Uniform weights, negative for odd n."""
    return round_of(_GRAPHS[graph]() if isinstance(graph, str) else graph, "uniform", who=who, n=n)


def _sentinel_pool(rows, ld, bf16, dev):
    return sentinel_pool(rows, ld, bf16, dev, SENTINEL[bf16])


def _padded(pool, bf16, dev, odd=True):
    return padded(pool, bf16, dev, odd=odd)


def _same(got, ref, bf16):
    """Bit for bit; on fp32 a NaN matches a NaN (payloads are not the oracle's to pin)."""
    return same(got, ref, nan_payloads_free=not bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("graph,n", _CASES)
def test_round_clique_col_vs_oracle(cuda, graph, n, bf16):
    """EXACT: bitwise the oracle's round; FMA: bitwise K1-FMA on three rows and, on bf16, the
    oracle's fused round.  Signed weights, specials, a payload NaN in member 1 (bf16: stored as
    0xFFFF by every row reading it), -0.0 and +-inf columns, output rows permuted and shifted by
    2, a padded odd stride, and nothing else written."""
    orders, ws = _round_of(graph, n)
    rows = len(orders)
    csr = ra.round_csr(orders, ws)
    out_rows = (np.random.default_rng(rows).permutation(rows) + 2).astype(np.int32)
    plan = ops.build_clique_plan(*csr, out_rows, bf16=bf16, max_members=128)
    assert plan is not None and plan.n_col >= 1
    assert (plan.n_cliques > 0) == (graph == "mixed") and (plan.rest is not None) == (graph in ("mixed", "barbell66"))
    pool, nan_col = inputs(rows, n, rows + n, bf16)
    pin = _padded(pool, bf16, cuda, odd=plan.n_cliques == 0)
    for mode in MODES:
        pout = _sentinel_pool(rows + 2, pin.shape[1], bf16, cuda)
        run(pin, pout, plan, n, mode)
        got = bits(pout)
        if mode == ops.MODE_EXACT or bf16:
            ref = oracle_round(pool, csr, out_rows - 2, bf16, exact=(mode == ops.MODE_EXACT))
            assert _same(got[2:, :n], ref, bf16), (graph, n, mode)
        if mode == ops.MODE_FMA:
            for r in (0, rows // 2, rows - 1):
                assert _same(got[out_rows[r], :n], k1_fma(pin, orders, ws, r, n), bf16), (graph, n, r)
        for r in range(rows):
            if 1 in orders[r]:
                assert is_nan(got[out_rows[r], nan_col], bf16), (r, mode)
        assert np.all(got[:2] == SENTINEL[bf16]) and np.all(got[:, n:] == SENTINEL[bf16])  # nothing else written


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_partial_participation(cuda, bf16):
    """complete(100) with output rows for 37 members: those rows are the oracle's, the other 63
    rows of the output pool keep their sentinel."""
    n = 259
    who = sorted(np.random.default_rng(5).choice(100, 37, replace=False).tolist())
    orders, ws = _round_of(nx.complete_graph(100), n, who=who)
    csr = ra.round_csr(orders, ws)
    out_rows = np.array(who, dtype=np.int32)
    plan = ops.build_clique_plan(*csr, out_rows, bf16=bf16, max_members=128)
    assert (plan.n_cliques, plan.n_col, plan.col_mmax) == (0, 1, 100) and plan.rest is None
    pool, _ = inputs(100, n, 11, bf16)
    pin = _padded(pool, bf16, cuda)
    for mode in MODES:
        pout = _sentinel_pool(100, pin.shape[1], bf16, cuda)
        run(pin, pout, plan, n, mode)
        got = bits(pout)
        if mode == ops.MODE_EXACT or bf16:
            ref = oracle_round(pool, csr, out_rows, bf16, exact=(mode == ops.MODE_EXACT),
                          pool_out=np.full((100, n), SENTINEL[bf16], np_dtype(bf16)))
            assert _same(got[:, :n], ref, bf16), mode
        else:
            for k in (0, 18, 36):
                assert _same(got[who[k], :n], k1_fma(pin, orders, ws, k, n), bf16), k
        idle = np.setdiff1d(np.arange(100), who)
        assert len(idle) == 63 and np.all(got[idle] == SENTINEL[bf16]) and np.all(got[:, n:] == SENTINEL[bf16])


def _col_table_of(plan64):
    """The K3c records of a plan (no attached rows) as K3c1 records."""
    t = plan64.table.reshape(plan64.n_cliques, ops.CLIQUE_WORDS)
    assert np.all(t[:, 2] == 0)
    c = np.zeros((plan64.n_cliques, ops.CLIQUE_COL_WORDS), np.int32)
    c[:, :2] = t[:, :2]
    c[:, 4 + ops.CLIQUE_COL_MAX:] = -1
    c[:, 4: 4 + ops.CLIQUE_MAX] = t[:, 4: 4 + ops.CLIQUE_MAX]
    c[:, 4 + ops.CLIQUE_COL_MAX: 4 + ops.CLIQUE_COL_MAX + ops.CLIQUE_MAX] = t[:, 4 + ops.CLIQUE_MAX: 4 + 2 * ops.CLIQUE_MAX]
    return c


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [7, 259])
def test_small_block_equals_k3c(cuda, bf16, n):
    """Blocks of <= 64 members are legal input: complete(40) through the column entry gives K3c's
    bits in both modes."""
    orders, ws = _round_of(nx.complete_graph(40), n)
    csr = ra.round_csr(orders, ws)
    out_rows = np.arange(40, dtype=np.int32)
    plan = ops.build_clique_plan(*csr, out_rows, bf16=bf16)
    assert plan.n_cliques == 1 and plan.mmax == 40 and plan.rest is None
    pool, _ = inputs(40, n, 40 + n, bf16)
    pin = _padded(pool, bf16, cuda, odd=False)
    table = torch.from_numpy(_col_table_of(plan).reshape(-1)).to(cuda)
    L = _lib.load()
    fn = getattr(L, "tal_agg_round_clique_col_bf16" if bf16 else "tal_agg_round_clique_col_f32")
    for mode in MODES:
        want = _sentinel_pool(40, pin.shape[1], bf16, cuda)
        run(pin, want, plan, n, mode)
        pout = _sentinel_pool(40, pin.shape[1], bf16, cuda)
        ops.check(fn(ctypes.c_void_p(pin.data_ptr()), pin.stride(0), ctypes.c_void_p(pout.data_ptr()), pout.stride(0),
                     n, ctypes.c_void_p(table.data_ptr()), 1, 40, int(mode), ops._stream(cuda, None)))
        torch.cuda.synchronize()
        assert np.array_equal(bits(pout), bits(want)), mode
        if mode == ops.MODE_EXACT:
            assert _same(bits(want)[:, :n], oracle_round(pool, csr, out_rows, bf16), bf16)


def _entries(monkeypatch, bf16):
    t = "bf16" if bf16 else "f32"
    return (count(monkeypatch, f"tal_agg_round_clique_col_{t}"), count(monkeypatch, f"tal_agg_round_clique_{t}"),
            count(monkeypatch, f"tal_agg_round_{t}"))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
def test_dispatch_counts(cuda, monkeypatch, bf16, mode):
    """complete(100): the column entry once, K3c's entry and the regular round entry never; a round
    with a 20-block, a 100-block and other rows: each of the three once.  In place is refused."""
    n = 259
    col, k3c, regular = _entries(monkeypatch, bf16)
    for graph, want in (("complete100", (1, 0, 0)), ("mixed", (1, 1, 1))):
        orders, ws = _round_of(graph, n)
        rows = len(orders)
        csr = ra.round_csr(orders, ws)
        out_rows = np.arange(rows, dtype=np.int32)
        plan = ops.plan_from_spec(*csr, out_rows, {"clique": 1, "members": 128, "rest": None})
        pool, _ = inputs(rows, n, 3, bf16)
        pin = _padded(pool, bf16, cuda, odd=False)
        pout = torch.zeros_like(pin)
        before = (col.calls, k3c.calls, regular.calls)
        run(pin, pout, plan, n, mode)
        assert (col.calls - before[0], k3c.calls - before[1], regular.calls - before[2]) == want, graph
        if mode == ops.MODE_EXACT or bf16:
            assert _same(bits(pout)[:, :n], oracle_round(pool, csr, out_rows, bf16, exact=(mode == ops.MODE_EXACT)), bf16)
        with pytest.raises(ValueError):
            run(pin, pin, plan, n, mode)
        assert (col.calls - before[0], k3c.calls - before[1], regular.calls - before[2]) == want


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
def test_unaligned_pools_stay_on_the_clique_path(cuda, monkeypatch, bf16, mode):
    """An odd row stride and pools that start one element (4 B / 2 B) into an aligned buffer: the
    column entry runs (no fallback to plan.full, whose entry is never called) and gives the
    aligned run's bits."""
    n = 259
    orders, ws = _round_of("complete100", n)
    csr = ra.round_csr(orders, ws)
    out_rows = np.arange(100, dtype=np.int32)
    plan = ops.build_clique_plan(*csr, out_rows, bf16=bf16, max_members=128)
    pool, _ = inputs(100, n, 9, bf16)
    aligned = _padded(pool, bf16, cuda, odd=False)
    want = torch.zeros_like(aligned)
    run(aligned, want, plan, n, mode)
    want = bits(want)[:, :n]
    if mode == ops.MODE_EXACT or bf16:
        assert _same(want, oracle_round(pool, csr, out_rows, bf16, exact=(mode == ops.MODE_EXACT)), bf16)
    col, k3c, regular = _entries(monkeypatch, bf16)
    ld = aligned.shape[1] + 1  # odd
    assert ld % 2 == 1
    esize = aligned.element_size()
    src = torch.zeros(100 * ld + 1, dtype=aligned.dtype, device=cuda)[1:].view(100, ld)
    dst = torch.zeros(100 * ld + 1, dtype=aligned.dtype, device=cuda)[1:].view(100, ld)
    assert src.data_ptr() % (2 * esize) == esize and dst.data_ptr() % (2 * esize) == esize
    src[:, : aligned.shape[1]] = aligned
    run(src, dst, plan, n, mode)
    assert np.array_equal(bits(dst)[:, :n], want)
    assert (col.calls, k3c.calls, regular.calls) == (1, 0, 0)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_plan_rows_beyond_a_pool_raise_before_any_launch(cuda, monkeypatch, bf16):
    """A plan that reads a row pool_in lacks, or writes one pool_out lacks, is a ValueError of
    ops.round_* for the 64-member record (complete 9) and the column record (complete 65) alike,
    and none of the five round entries is called."""
    n = 8
    t = "bf16" if bf16 else "f32"
    cs = [count(monkeypatch, f"tal_agg_round_{k}{t}") for k in ("clique_col_w_", "clique_w_", "", "clique_col_", "clique_")]
    for m, blocks in ((9, (1, 0)), (65, (0, 1))):
        orders, ws = _round_of(nx.complete_graph(m), n)
        plan = ops.build_clique_plan(*ra.round_csr(orders, ws), np.arange(m, dtype=np.int32), bf16=bf16, max_members=128)
        assert (plan.n_cliques, plan.n_col) == blocks and plan.rest is None
        whole = torch.zeros(m, n, dtype=tdtype(bf16), device=cuda)
        short = torch.zeros(m - 1, n, dtype=tdtype(bf16), device=cuda)
        with pytest.raises(ValueError, match="beyond pool_in"):
            run(short, whole, plan, n, ops.MODE_EXACT)
        with pytest.raises(ValueError, match="beyond pool_out"):
            run(whole, short, plan, n, ops.MODE_EXACT)
    assert [c.calls for c in cs] == [0] * 5
