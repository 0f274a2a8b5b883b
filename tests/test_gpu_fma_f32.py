"""fp32 TAL_MODE_FMA on the GPU, bit for bit against the fused oracle.

FMA mode is one deterministic chain per element, acc = fl(w_0 * x_0), acc = fma(w_i, x_i, acc)
in operand order (include/tal_agg.h), and oracle.agg_f32 / oracle.round_f32 with exact=False
restate it (pinned against exact rational arithmetic by tests/test_oracle_fma.py).  Every fp32
entry point that takes the mode is compared with that oracle directly, all bits, NaN positions
equal and payloads not compared.  The inputs (tests/_fma_cases.py) carry subnormals, both zeros,
3e38, 65504, an inf and a NaN, cancelling operands, columns of -0.0 and of mixed zeros, and for
rounds an inf / NaN source that only some rows name (rows that do not must stay finite).  Each
test also asserts on the reference alone that the fused chain differs from the EXACT one in at
least 10 % of the finite elements, so a kernel running EXACT arithmetic in FMA mode fails.

Entry point / kernel -> test
  tal_agg_f32: k_agg<M> 1..17, run-time count 18+, passes past 256 operands, the scalar kernel,
    out aliasing the first / last operand (k_agg_chain scratch past 256)
                                              test_agg_f32_fma_vs_oracle
  tal_agg_model_f32 (K1m): fused launch, last-block tail, two launches past 64 operands
                                              test_agg_model_f32_fma_vs_oracle
  k_round_f32_persistent (c4 64 / 128, sparse / dense, 1 / several groups, in place)
                                              test_round_persistent
  k_round_f32_tiled (sparse / dense)          test_round_tiled
  k_round_tiled_scalar (odd ld; the tail of an in-place round)
                                              test_round_tiled_scalar, test_round_persistent
  k_round_direct (<= 256 columns out of place: odd ld, every n % 4 tail)
                                              test_round_direct and the tails of the others
  k_round_f32_narrow, pairs form              test_round_narrow_pairs
  k_round_f32_narrow, ROWW form (+1/m, -1/m)  test_round_narrow_roww
  k_round_f32_narrow, 8 / 12 staging loads    test_round_narrow_wide_groups
  k_round_f32_narrow, broadcast form          test_round_narrow_bcast
  k_round_stream, k_round_stream_scalar       test_round_stream, test_round_stream_scalar
  k_round_clique (K3c), uniform weights       test_round_clique
  k_round_clique (K3c), per-source weights    test_round_clique_weighted
  k_round_clique_col (K3c1)                   test_round_clique_col
  RoundExecutor(mode=MODE_FMA), fp32 + int64  test_round_executor_fma
Not reachable in fp32 FMA mode
  k_round_wide: bf16 only - round_vec_form() returns kWide for a streamed plan only when bf16,
    an fp32 pool gets kStream (tal_agg.hip, `if (in.stream_cs != 0) return bf16 ? kWide : kStream`)
  the bf16 EXACT chains (bf16x_first4 / bf16x_next4): first4t / next4t take them only for
    uint16_t storage in EXACT mode
  the int64 kernels: one arithmetic in both modes (`EXACT || kIsI64<T>`); tal_agg_round_i64 has
    no mode argument
"""
import networkx as nx
import numpy as np
import pytest
import torch

import oracle
from _fma_cases import (WEIGHT_KINDS, RoundCase, assert_bits, fused_differs, k1_operands, k1_weights,
                        products_exact)
from _pools import dev_rows
from oracle import reference_alg as ra
from topology_aware_learning_amd import ops
from topology_aware_learning_amd import weights as tw
from topology_aware_learning_amd.arena import ModelPool, StateLayout
from topology_aware_learning_amd.round import RoundExecutor

pytestmark = pytest.mark.gpu

FMA = ops.MODE_FMA

# ---- K1 ----------------------------------------------------------------------------------------
K1_M = [1, 2, 8, 9, 16, 17, 18, 25, 33, 256, 257, 300, 513]
K1_N = [1, 3, 4, 5, 1027, 4 * 257 + 2]  # 1030: a block of 256 float4 chunks, one more, a 2-element tail
K1_LAYOUTS = ["apart", "offset4", "out_last", "out_first"]


def _k1_buffers(xs, n, off, cuda):
    """One [m + 1, ld] device buffer: operand i in row i at element `off` (0: 16-B aligned rows,
    1: every pointer 4 bytes into its row - the scalar kernel), row m for an output apart."""
    m = len(xs)
    ld = (n + 3) // 4 * 4 + 4
    buf = np.full((m + 1, ld), 7.0, np.float32)
    for i, x in enumerate(xs):
        buf[i, off:off + n] = x
    base = torch.from_numpy(buf).to(cuda)
    return buf, base, [base[i, off:off + n] for i in range(m + 1)]


@pytest.mark.parametrize("kind", WEIGHT_KINDS)
@pytest.mark.parametrize("layout", K1_LAYOUTS)
@pytest.mark.parametrize("m", K1_M)
def test_agg_f32_fma_vs_oracle(cuda, m, layout, kind):
    for n in K1_N:
        rng = np.random.default_rng(7919 * m + n)
        xs = k1_operands(rng, m, n)
        w = k1_weights(rng, m, kind)
        ref = oracle.agg_f32(xs, w, exact=False)
        if m >= 2 and n > 1000 and not products_exact(w):
            fused_differs(ref, oracle.agg_f32(xs, w))
        off = 1 if layout == "offset4" else 0
        buf, base, rows = _k1_buffers(xs, n, off, cuda)
        o = {"apart": m, "offset4": m, "out_last": m - 1, "out_first": 0}[layout]
        assert rows[o].data_ptr() % 16 == 4 * off
        ops.agg_f32(rows[:m], w, rows[o], mode=FMA)
        got = base.cpu().numpy()
        assert_bits(got[o, off:off + n], ref, (n,))
        got[o, off:off + n] = buf[o, off:off + n]  # nothing else was written
        assert np.array_equal(got.view(np.uint32), buf.view(np.uint32)), (n, "stray write")


@pytest.mark.parametrize("n_i", [0, 53])
@pytest.mark.parametrize("m", [1, 9, 17, 18, 64, 65])
def test_agg_model_f32_fma_vs_oracle(cuda, m, n_i):
    """K1m: n = 3 (no whole chunk), 1024 (the last block holds no fp32 chunk) and 1026 (its
    tail); m = 65 is past kModelOps: the two segment launches."""
    for n in (3, 1024, 1026):
        rng = np.random.default_rng(104729 * m + n + n_i)
        xs = k1_operands(rng, m, n)
        w = k1_weights(rng, m, "random")
        xis = [rng.integers(-(2 ** 40), 2 ** 40, size=n_i).astype(np.int64) for _ in range(m)]
        for x in xis:
            x[:min(n_i, 3)] = [1000, 2 ** 31 + 5, -999][:min(n_i, 3)]
        ref = oracle.agg_f32(xs, w, exact=False)
        if m >= 2 and n > 1000:
            fused_differs(ref, oracle.agg_f32(xs, w))
        dx = [torch.from_numpy(x).to(cuda) for x in xs]
        dxi = [torch.from_numpy(x).to(cuda) for x in xis]
        out = torch.full((n,), 7.0, dtype=torch.float32, device=cuda)
        out_i = torch.zeros(n_i, dtype=torch.int64, device=cuda)
        ops.agg_model_f32(dx, dxi, w, out, out_i, mode=FMA)
        assert_bits(out.cpu().numpy(), ref, (n,))
        if n_i:
            assert np.array_equal(out_i.cpu().numpy(), oracle.agg_i64(xis, w)), n


# ---- rounds ------------------------------------------------------------------------------------
def _tile_n(c4):
    return 4 * (2 * c4 + 1) + 3  # two full tiles, a partial tile and a 3-element tail


def _graph_round(g, weights):
    """Rows in reference order (sorted neighbors, then self) with unweighted, softmax-of-degree-
    centrality, or signed uniform weights."""
    cent = nx.degree_centrality(g)
    orders = [sorted(g.neighbors(i)) + [i] for i in sorted(g.nodes)]
    if weights == "unweighted":
        ws = [ra.unweighted_weights(len(o)) for o in orders]
    elif weights == "softmax":
        ws = [ra.centrality_weights(o, cent, True, 10.0) for o in orders]
    else:
        ws = [[float(weights) / len(o)] * len(o) for o in orders]
    return orders, ws


def _regular64():
    return nx.random_regular_graph(8, 64, seed=0)


def _gnp150():
    return nx.gnp_random_graph(150, 0.08, seed=2)


def _run(cuda, case, plan, pad=True, in_place=False, what=None):
    """The round in FMA mode into a copy of the input pool (so rows and padding the round must
    not write are compared too), every element against the fused oracle."""
    pin = dev_rows(case.pool, cuda, pad)
    pout = pin.clone()
    ops.round_f32(pin, pout, plan, n=case.n, mode=FMA)
    got = pout.cpu().numpy()
    case.check(got, what)
    assert np.array_equal(got[:, case.n:].view(np.uint32), pin[:, case.n:].cpu().numpy().view(np.uint32)), "padding written"
    if in_place:
        ops.round_f32(pin, pin, plan, n=case.n, mode=FMA)
        case.check(pin.cpu().numpy(), (what, "in place"))
    return pin, pout


@pytest.mark.parametrize("dense", [0, 8], ids=["sparse", "dense"])
@pytest.mark.parametrize("c4,lds,multi", [(64, 80 * 1024, False), (128, 160 * 1024, False),
                                          (64, 24 * 1024, True), (128, 40 * 1024, True)])
def test_round_persistent(cuda, c4, lds, multi, dense):
    orders, ws = _graph_round(_regular64(), "softmax")
    n = 4099 if multi else _tile_n(c4)
    case = RoundCase(orders, ws, np.arange(64), 64, n, seed=c4 + dense)
    plan = ops.build_plan(*case.csr, c4=c4, lds_bytes=lds, dense=dense)
    assert ops.round_kernel_name(plan) == "k_round_f32_persistent"
    assert plan.info.c4 == c4 and plan.info.dense_rb == dense and (plan.info.n_groups > 1) == multi
    assert case.spared > 0
    _run(cuda, case, plan, in_place=plan.single_group)  # in place: the tail by k_round_tiled_scalar


@pytest.mark.parametrize("dense", [0, 8], ids=["sparse", "dense"])
def test_round_tiled(cuda, dense):
    """A group of 150 sources at c4 = 64, past what the persistent kernel stages."""
    rows, c4 = 4, 64
    orders = [[s for s in range(rows, 154) if (s + r) % 31] + [r] for r in range(rows)]
    case = RoundCase(orders, [ra.unweighted_weights(len(o)) for o in orders], np.arange(rows), 154, _tile_n(c4),
                     seed=154 + dense)
    plan = ops.build_plan(*case.csr, c4=c4, lds_bytes=160 * 1024, dense=dense)
    assert plan.info.dense_rb == dense and ops.round_kernel_name(plan) == "k_round_f32_tiled"
    assert case.spared > 0
    _run(cuda, case, plan)


def _scalar_case(n, seed):
    g = nx.random_regular_graph(4, 20, seed=1)
    orders, ws = _graph_round(g, "softmax")
    ws = [[w * (1 + 0.01 * k) for k, w in enumerate(row)] for row in ws]  # (a regular graph: make them per-operand)
    return RoundCase(orders, ws, np.arange(20), 20, n, seed)


def test_round_tiled_scalar(cuda):
    """Contiguous rows of odd length: no vector kernel (agg_round needs ld % 4 == 0), and more
    than kDirectMaxCols = 256 columns, so every column runs k_round_tiled_scalar."""
    case = _scalar_case(1031, 3)
    plan = ops.build_plan(*case.csr)
    assert plan.info.stream_cs == 0
    pin, _ = _run(cuda, case, plan, pad=False)
    assert pin.stride(0) % 4 != 0 and case.n > 256


def test_round_direct(cuda):
    """Odd rows and at most 256 columns out of place: every column by k_round_direct (use_direct)."""
    case = _scalar_case(135, 4)
    plan = ops.build_plan(*case.csr)
    pin, pout = _run(cuda, case, plan, pad=False)
    assert pin.stride(0) % 4 != 0 and case.n <= 256 and pin.data_ptr() != pout.data_ptr()


@pytest.mark.parametrize("graph", ["regular", "gnp"])
@pytest.mark.parametrize("c4", [16, 32])
def test_round_narrow_pairs(cuda, c4, graph):
    """Per-operand weights (softmax of the degree centrality), permuted output rows."""
    g = _regular64() if graph == "regular" else _gnp150()
    orders, ws = _graph_round(g, "softmax")
    if graph == "regular":  # equal degrees give equal weights: make them per-operand
        ws = [[w * (1 + 0.01 * k) for k, w in enumerate(row)] for row in ws]
    rows = len(orders)
    case = RoundCase(orders, ws, np.random.default_rng(rows).permutation(rows), rows, _tile_n(c4), seed=rows + c4)
    plan = ops.build_plan(*case.csr, c4=c4, lds_bytes=160 * 1024)
    assert ops.round_kernel_name(plan) == "k_round_f32_narrow"
    assert plan.info.c4 == c4 and plan.info.narrow_roww == 0 and plan.info.narrow_bcast == 0
    assert case.spared > 0
    _run(cuda, case, plan, in_place=plan.single_group)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus", "minus"])
@pytest.mark.parametrize("c4", [16, 32])
def test_round_narrow_roww(cuda, c4, sign):
    """One weight per row, +1/m and -1/m: padding reads the zero tile of the weight's sign."""
    g = nx.random_regular_graph(6, 40, seed=3)
    orders, ws = _graph_round(g, sign)
    case = RoundCase(orders, ws, np.arange(40), 40, _tile_n(c4), seed=7 + c4)
    plan = ops.build_plan(*case.csr, c4=c4, lds_bytes=80 * 1024)
    assert ops.round_kernel_name(plan) == "k_round_f32_narrow" and plan.info.narrow_roww == 1 and plan.info.c4 == c4
    assert case.spared > 0
    _run(cuda, case, plan, in_place=plan.single_group)


@pytest.mark.parametrize("uniform", [True, False], ids=["roww", "pairs"])
@pytest.mark.parametrize("c4,sources,j", [(16, 300, 8), (16, 600, 12), (32, 300, 12)])
def test_round_narrow_wide_groups(cuda, c4, sources, j, uniform):
    """Groups past 256 sources at c4 = 16 (128 at c4 = 32): 8 and 12 staging loads per lane."""
    rows = 6
    orders = [[s for s in range(rows, sources) if (s + r) % 29] + [r] for r in range(rows)]
    rng = np.random.default_rng(sources + c4)
    ws = [ra.unweighted_weights(len(o)) if uniform else list(rng.uniform(0.05, 1.0, len(o)) / len(o)) for o in orders]
    case = RoundCase(orders, ws, np.arange(rows), sources, _tile_n(c4), seed=sources + c4)
    plan = ops.build_plan(*case.csr, c4=c4, lds_bytes=160 * 1024)
    lo, hi = {8: (4, 8), 12: (8, 12)}[j]
    assert ops.round_kernel_name(plan) == "k_round_f32_narrow"
    assert lo * 1024 < plan.info.max_src * c4 <= hi * 1024 and plan.info.narrow_roww == int(uniform)
    assert case.spared > 0
    _run(cuda, case, plan)


@pytest.mark.parametrize("waves,wg", [(8, 2), (12, 2), (16, 2), (16, 1)])
@pytest.mark.parametrize("c4", [16, 32])
@pytest.mark.parametrize("graph", ["gnp", "star"])
def test_round_narrow_bcast(cuda, graph, c4, waves, wg):
    """The broadcast form: operand records in VGPRs, the accumulator starts at -0.0."""
    g = _gnp150() if graph == "gnp" else nx.star_graph(70)  # star: a row of 71 operands, five records
    orders, ws = _graph_round(g, "softmax")
    if graph == "star":  # (its softmax weights leave the leaves ~5e-5 of a row: both modes round alike)
        rng = np.random.default_rng(70)
        ws = [list(rng.uniform(0.05, 1.0, len(o)) / len(o)) for o in orders]
    rows = len(orders)
    case = RoundCase(orders, ws, np.random.default_rng(rows).permutation(rows), rows, _tile_n(c4), seed=rows + c4 + waves)
    plan = ops.build_plan(*case.csr, c4=c4, lds_bytes=80 * 1024, bcast=waves, bcast_wg=wg)
    assert ops.round_kernel_name(plan) == "k_round_f32_narrow"
    assert plan.info.narrow_bcast == waves and plan.info.bc_wg_per_cu == wg and plan.info.c4 == c4
    assert case.spared > 0
    _run(cuda, case, plan, in_place=plan.single_group)


@pytest.mark.parametrize("grouping", [(64, 0), (16, 24)])
@pytest.mark.parametrize("graph", ["gnp", "barbell"])
def test_round_stream(cuda, graph, grouping):
    """Sources streamed through the LDS ring, dense row blocks under a row mask; permuted output
    rows; the 3-element tail out of place by k_round_direct."""
    g = _gnp150() if graph == "gnp" else nx.barbell_graph(30, 4)
    orders, ws = _graph_round(g, "softmax" if graph == "gnp" else "unweighted")
    rows = len(orders)
    case = RoundCase(orders, ws, np.random.default_rng(rows).permutation(rows), rows, 4099, seed=rows + grouping[0])
    plan = ops.build_stream_plan(*case.csr, *grouping)
    assert ops.round_kernel_name(plan) == "k_round_stream" and plan.info.stream_cs in (16, 32)
    assert case.spared > 0
    _run(cuda, case, plan, in_place=plan.single_group)


def test_round_stream_scalar(cuda):
    """A streamed plan on contiguous odd rows of more than 256 columns: k_round_stream_scalar."""
    g = nx.barbell_graph(9, 2)
    orders, ws = _graph_round(g, "unweighted")
    rows = len(orders)
    case = RoundCase(orders, ws, np.arange(rows)[::-1].copy(), rows, 1031, seed=4)
    plan = ops.build_stream_plan(*case.csr, 8, 0)
    assert plan.info.stream_cs > 0 and plan.info.n_groups > 1
    pin, _ = _run(cuda, case, plan, pad=False)
    assert pin.stride(0) % 4 != 0 and case.n > 256


def _clique_run(cuda, case, plan):
    pin, pout = _run(cuda, case, plan)
    assert pin.stride(0) % 2 == 0 and pin.data_ptr() % 8 == 0 and pout.data_ptr() % 8 == 0  # not plan.full


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus", "minus"])
@pytest.mark.parametrize("n", [259, 1030])
def test_round_clique(cuda, n, sign):
    """K3c on barbell(20, 3): two blocks of 20, the bridge rows attached or through the rest plan."""
    orders, ws = _graph_round(nx.barbell_graph(20, 3), sign)
    rows = len(orders)
    case = RoundCase(orders, ws, np.random.default_rng(rows).permutation(rows), rows, n, seed=rows + n)
    plan = ops.build_clique_plan(*case.csr)
    assert plan is not None and plan.n_cliques == 2 and plan.wtable is None and plan.n_col == 0
    assert ops.round_kernel_name(plan) == "k_round_clique" and case.spared > 0
    _clique_run(cuda, case, plan)


@pytest.mark.parametrize("kind", ["degcent", "signed"])
@pytest.mark.parametrize("n", [259, 1030])
def test_round_clique_weighted(cuda, n, kind):
    """K3c with one weight per source: softmax of the degree centrality, and signed weights with
    zeros among them."""
    g = nx.barbell_graph(20, 3)
    nodes = sorted(g.nodes)
    orders = [sorted(g.neighbors(i)) + [i] for i in nodes]
    if kind == "degcent":
        cent = nx.degree_centrality(g)
        ws = [tw.centrality(o, cent, True, 10.0) for o in orders]
    else:
        per = [0.0 if j % 7 == 3 else ((-1.0) ** j) * (0.013 * (j % 11) + 0.002) for j in nodes]
        ws = [[per[j] for j in o] for o in orders]
    rows = len(orders)
    case = RoundCase(orders, ws, np.arange(rows), rows, n, seed=rows + n + len(kind))
    plan = ops.build_clique_plan(*case.csr, per_source=True)
    assert plan is not None and plan.n_cliques >= 1 and plan.wtable is not None
    assert ops.round_kernel_name(plan) == "k_round_clique" and case.spared > 0
    _clique_run(cuda, case, plan)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus", "minus"])
@pytest.mark.parametrize("n", [259, 1030])
def test_round_clique_col(cuda, n, sign):
    """K3c1 on barbell(66, 3): two blocks of 66 members, one column per lane."""
    orders, ws = _graph_round(nx.barbell_graph(66, 3), sign)
    rows = len(orders)
    case = RoundCase(orders, ws, np.random.default_rng(rows).permutation(rows), rows, n, seed=rows + n)
    plan = ops.build_clique_plan(*case.csr, max_members=128)
    assert plan is not None and plan.n_col == 2 and plan.n_cliques == 0
    assert ops.round_kernel_name(plan) == "k_round_clique_col" and case.spared > 0
    _run(cuda, case, plan)


def test_round_executor_fma(cuda):
    """RoundExecutor(mode=MODE_FMA) on an fp32 + int64 layout, double-buffered, with the plan
    default_plan picks: fp32 against the fused oracle, int64 against oracle.round_i64, over two
    rounds (the second reads the exchanged pool)."""
    orders, ws = _graph_round(nx.random_regular_graph(4, 20, seed=1), "unweighted")
    n, n_i = 1031, 5
    case = RoundCase(orders, ws, np.arange(20), 20, n, seed=11)
    lay = StateLayout.from_layout([("w", (n,), "float32"), ("nbt", (n_i,), "int64")])
    pool = ModelPool(lay, 20, cuda)
    xi = np.random.default_rng(12).integers(0, 10 ** 6, (20, n_i))
    xi[:, 0] = 1000
    pool.f32[:, :n] = torch.from_numpy(case.pool).to(cuda)
    pool.i64[:, :n_i] = torch.from_numpy(xi).to(cuda)
    ex = RoundExecutor(pool, mode=FMA, placement_trials=1)
    assert ex.double_buffer
    x = case.pool
    for k in range(2):
        x = oracle.round_f32(x, *case.csr, exact=False)
        xi = oracle.round_i64(xi, *case.csr)
        ex.run(orders, ws)
        assert_bits(pool.f32[:, :n].cpu().numpy(), x, k)
        assert np.array_equal(pool.i64[:, :n_i].cpu().numpy(), xi), k
    assert ex.swaps == 2
