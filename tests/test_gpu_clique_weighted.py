"""K3c with per-source weights (tal_agg_round_clique_w_f32 / _bf16): clique blocks whose source j
carries the same fp32 weight w_j in every row (the weighted and centrality apps), bit for bit
against
  fp32 EXACT   oracle.round_f32
  fp32 FMA     ops.agg_f32(mode=FMA), one K1 call per row
  bf16         oracle.round_bf16 of the mode (NaN stored as 0xFFFF)
over every MMAX instantiation, odd widths (the tail kernels), n below one block and several blocks,
attached rows with their own per-operand weights, the uniform entries' output on a uniform round,
the alignment fallback and RoundExecutor."""
import networkx as nx
import numpy as np
import pytest
import torch

import oracle
from oracle import reference_alg as ra
from topology_aware_learning_amd import ops
from topology_aware_learning_amd import weights as tw
from topology_aware_learning_amd.arena import ModelPool, StateLayout
from topology_aware_learning_amd.round import RoundExecutor

from _clique import MODES, bits, count, inputs, padded, round_of, run, same, sentinel_pool, to_dev

pytestmark = pytest.mark.gpu

F32, BF16 = "f32", "bf16"
SENTINEL = {F32: 0x12345678, BF16: 0x1234}

_GRAPHS = {
    "complete9": lambda: nx.complete_graph(9),      # m = 9: the 16-member instantiation
    "barbell20": lambda: nx.barbell_graph(20, 3),   # m = 20: the 32-member instantiation, rest rows
    "complete37": lambda: nx.complete_graph(37),    # m = 37: the 40-member instantiation, a partial row group
    "barbell45": lambda: nx.barbell_graph(45, 2),   # m = 45: the 48-member instantiation, bridges attached
    "complete53": lambda: nx.complete_graph(53),    # m = 53: the 56-member instantiation
    "barbell60": lambda: nx.barbell_graph(60, 8),   # BASELINE config 4's topology (m = 60)
    "complete64": lambda: nx.complete_graph(64),    # m = 64: the largest block
    "mixed": lambda: nx.disjoint_union(nx.complete_graph(12), nx.random_regular_graph(4, 30, seed=1)),
}
_WEIGHTS = ["datasize", "degcent", "signed"]
_CASES = [(g, n) for g in _GRAPHS for n in (1, 7, 4098)] + [("barbell60", 20003), ("complete64", 20003)]


def _round_of(graph, kind):
    return round_of(_GRAPHS[graph](), kind)


def _to_bits(x, dt):
    return x.view(np.uint32) if dt == F32 else oracle.f32_to_bf16(x)


def _inputs(rows, n, seed, dt):
    return inputs(rows, n, seed, dt == BF16)


def _as_torch(bits_, dt, dev):
    return to_dev(bits_, dt == BF16, dev)


def _sentinel_pool(rows, ld, dt, dev):
    return sentinel_pool(rows, ld, dt == BF16, dev, SENTINEL[dt])


def _padded(pool, dt, dev):
    return padded(pool, dt == BF16, dev)  # even, padded stride


def _k1_rows_fma(pin, orders, ws, n, dev):
    """fp32 FMA reference: one K1 call per row on the device pool."""
    out = torch.empty(len(orders), n, dtype=torch.float32, device=dev)
    for r, (o, w) in enumerate(zip(orders, ws)):
        ops.agg_f32([pin[j, :n] for j in o], w, out[r], mode=ops.MODE_FMA)
    return bits(out)


def _same(got, ref, dt, mode):
    """Bit for bit; fp32 EXACT is held against the C oracle on the CPU, whose NaN payloads differ."""
    return same(got, ref, nan_payloads_free=(dt == F32 and mode == ops.MODE_EXACT))


def _reference(dt, mode, pool, pin, csr, orders, ws, n, dev):
    """Rows in CSR order."""
    row_ptr, col, w = csr
    ident = np.arange(len(orders), dtype=np.int32)
    if dt == BF16:
        return oracle.round_bf16(pool, row_ptr, col, w, ident, pool_out=np.zeros((len(orders), n), np.uint16),
                                 exact=(mode == ops.MODE_EXACT))
    if mode == ops.MODE_EXACT:
        return oracle.round_f32(pool.view(np.float32), row_ptr, col, w, ident,
                                pool_out=np.zeros((len(orders), n), np.float32)).view(np.uint32)
    return _k1_rows_fma(pin, orders, ws, n, dev)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("kind", _WEIGHTS)
@pytest.mark.parametrize("graph,n", _CASES)
def test_round_clique_weighted(cuda, graph, n, kind, dt):
    """Both modes against the references above: per-source weights of three kinds, denormals, 3e38,
    a payload NaN (bf16: every reading row stores 0xFFFF), -0.0 and +-inf columns, odd n, output rows
    permuted and shifted by 2 with a padded even stride, nothing else written."""
    orders, ws = _round_of(graph, kind)
    rows = len(orders)
    csr = ra.round_csr(orders, ws)
    out_rows = (np.random.default_rng(rows).permutation(rows) + 2).astype(np.int32)
    plan = ops.build_clique_plan(*csr, out_rows, per_source=True)
    assert plan is not None and plan.n_cliques >= 1 and plan.wtable is not None
    if kind != "degcent":  # (a complete graph's centralities are all equal: uniform weights)
        assert ops.build_clique_plan(*csr, out_rows) is None  # no uniform block: only this form takes the round
    pool, nan_col = _inputs(rows, n, rows + n, dt)
    pin = _padded(pool, dt, cuda)
    for mode in MODES:
        ref = _reference(dt, mode, pool, pin, csr, orders, ws, n, cuda)
        pout = _sentinel_pool(rows + 2, pin.shape[1], dt, cuda)
        run(pin, pout, plan, n, mode)
        got = bits(pout)
        assert _same(got[out_rows, :n], ref, dt, mode), (graph, n, kind, dt, mode)
        if dt == BF16:
            for r in range(rows):
                if 1 in orders[r]:
                    assert got[out_rows[r], nan_col] == 0xFFFF, (r, mode)
        assert np.all(got[:2] == SENTINEL[dt]) and np.all(got[:, n:] == SENTINEL[dt])  # nothing else written


def _attached_round():
    """20 members on the even pool rows 0..38 with per-source weights, and two attached rows whose
    per-operand weights are their own: member self (10) with externals 5 and 31 interleaved among
    twelve members; non-member self (41) with one external above every member (45)."""
    members = list(range(0, 40, 2))
    w_of = {j: (0.01 + 0.003 * k) * (-1.0 if k % 5 == 2 else 1.0) for k, j in enumerate(members)}
    orders, ws = [], []
    for i in members:
        orders.append([j for j in members if j != i] + [i])
        ws.append([w_of[j] for j in orders[-1]])
    orders.append(sorted([j for j in members if j != 10][:12] + [5, 31]) + [10])
    ws.append([-0.3 + 0.021 * k for k in range(len(orders[-1]))])
    orders.append(sorted(members[3:15] + [45]) + [41])
    ws.append([0.07 - 0.009 * k for k in range(len(orders[-1]))])
    return orders, ws


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("n", [5, 4097])
def test_round_clique_weighted_attached_rows(cuda, n, dt):
    orders, ws = _attached_round()
    rows = len(orders)
    csr = ra.round_csr(orders, ws)
    out_rows = np.arange(rows, dtype=np.int32)
    cliques, rest = ops.find_cliques(*csr, out_rows, per_source=True)
    assert len(cliques) == 1 and len(cliques[0][3]) == 2 and rest == []
    plan = ops.build_clique_plan(*csr, out_rows, per_source=True)
    rng = np.random.default_rng(n)
    pool = _to_bits((rng.standard_normal((48, n)) * 3.0).astype(np.float32), dt)
    pin = _padded(pool, dt, cuda)
    for mode in MODES:
        ref = _reference(dt, mode, pool, pin, csr, orders, ws, n, cuda)
        pout = _sentinel_pool(rows, pin.shape[1], dt, cuda)
        run(pin, pout, plan, n, mode)
        assert _same(bits(pout)[:, :n], ref, dt, mode), (dt, mode)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("graph,n", [("barbell45", 4097), ("complete64", 1002), ("mixed", 7)])
def test_uniform_round_through_weighted_entries(cuda, graph, n, dt):
    """A uniform-weight round: the per-source entries give the uniform entries' bits (signed
    weights on odd n, so FMA's padding differs between the two forms and must not show)."""
    g = _GRAPHS[graph]()
    orders = [sorted(g.neighbors(i)) + [i] for i in sorted(g.nodes)]
    sign = -1.0 if n % 2 else 1.0
    ws = [[sign / len(o)] * len(o) for o in orders]
    rows = len(orders)
    csr = ra.round_csr(orders, ws)
    out_rows = np.arange(rows, dtype=np.int32)
    uni = ops.build_clique_plan(*csr, out_rows)
    per = ops.build_clique_plan(*csr, out_rows, per_source=True)
    assert uni.wtable is None and per.wtable is not None and per.clique_rows == uni.clique_rows
    pool, _ = _inputs(rows, n, 3, dt)
    pin = _padded(pool, dt, cuda)
    for mode in MODES:
        a = _sentinel_pool(rows, pin.shape[1], dt, cuda)
        b = _sentinel_pool(rows, pin.shape[1], dt, cuda)
        run(pin, a, uni, n, mode)
        run(pin, b, per, n, mode)
        assert np.array_equal(bits(a), bits(b)), (graph, dt, mode)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("mode", MODES)
def test_weighted_clique_dispatch_and_alignment_fallback(cuda, monkeypatch, mode, dt):
    """A per-source CliquePlan: one call of the weighted entry (never the uniform one), the rest rows
    through the regular entry, in place refused; pools the entry cannot take - rows starting half a
    column pair in, an odd row stride - run `plan.full` with the aligned run's bits."""
    n = 1002
    orders, ws = _round_of("barbell20", "datasize")
    rows = len(orders)
    csr = ra.round_csr(orders, ws)
    plan = ops.build_clique_plan(*csr, np.arange(rows, dtype=np.int32), per_source=True)
    assert plan.rest is not None
    pool, _ = _inputs(rows, n, 7, dt)
    pin = _padded(pool, dt, cuda)
    weighted = count(monkeypatch, f"tal_agg_round_clique_w_{dt}")
    uniform = count(monkeypatch, f"tal_agg_round_clique_{dt}")
    regular = count(monkeypatch, f"tal_agg_round_{dt}")
    want = torch.zeros_like(pin)
    run(pin, want, plan, n, mode)
    assert (weighted.calls, uniform.calls, regular.calls) == (1, 0, 1)
    want = bits(want)[:, :n]
    assert _same(want, _reference(dt, mode, pool, pin, csr, orders, ws, n, cuda), dt, mode)
    with pytest.raises(ValueError):
        run(pin, pin, plan, n, mode)
    ld, tdt = pin.shape[1], pin.dtype
    src = torch.zeros(rows * ld + 1, dtype=tdt, device=cuda)[1:].view(rows, ld)  # half a column pair in
    dst = torch.zeros(rows * ld + 1, dtype=tdt, device=cuda)[1:].view(rows, ld)
    assert src.data_ptr() % (2 * src.element_size()) == src.element_size()
    src.copy_(pin)
    run(src, dst, plan, n, mode)
    assert np.array_equal(bits(dst)[:, :n], want)
    src = torch.zeros(rows, ld + 1, dtype=tdt, device=cuda)  # an odd row stride
    dst = torch.zeros(rows, ld + 1, dtype=tdt, device=cuda)
    src[:, :ld] = pin
    run(src, dst, plan, n, mode)
    assert np.array_equal(bits(dst)[:, :n], want)
    assert (weighted.calls, uniform.calls) == (1, 0)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_round_executor_weighted_barbell(cuda, monkeypatch, dt):
    """RoundExecutor on a small ModelPool, barbell(12, 4) under weights.weighted, with the weighted
    clique plan as the round's default: every row equals the oracle round on the pre-round snapshot
    and exactly one weighted clique call ran."""
    n = 3001
    layout = StateLayout.from_layout([("w", (n,), "float32" if dt == F32 else "bfloat16")])
    g = nx.barbell_graph(12, 4)
    rows = g.number_of_nodes()
    orders = [sorted(g.neighbors(i)) + [i] for i in range(rows)]
    lens = np.random.default_rng(2).integers(100, 5000, rows).tolist()
    ws = [tw.weighted([lens[j] for j in o]) for o in orders]
    csr = ra.round_csr(orders, ws)
    monkeypatch.setitem(ops.WCLIQUE_DEFAULT, (dt == BF16, ops.MODE_EXACT), True)
    default = ops.default_plan(*csr, np.arange(rows, dtype=np.int32), bf16=(dt == BF16), mode=ops.MODE_EXACT)
    assert isinstance(default, ops.CliquePlan) and default.wtable is not None and default.n_cliques == 2
    pool = ModelPool(layout, rows, cuda)
    seg = pool.f32 if dt == F32 else pool.b16
    before = _to_bits((np.random.default_rng(4).standard_normal((rows, n)) * 3.0).astype(np.float32), dt)
    seg[:, :n].copy_(_as_torch(before, dt, cuda))
    weighted = count(monkeypatch, f"tal_agg_round_clique_w_{dt}")
    ex = RoundExecutor(pool, mode=ops.MODE_EXACT, placement_trials=1)  # no placement runs: the round alone
    ex.run(orders, ws)
    ref = _reference(dt, ops.MODE_EXACT, before, None, csr, orders, ws, n, cuda)
    seg = pool.f32 if dt == F32 else pool.b16
    assert _same(bits(seg[:, :n]), ref, dt, ops.MODE_EXACT)
    assert weighted.calls == 1
