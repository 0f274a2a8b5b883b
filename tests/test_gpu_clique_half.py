"""K3c2 on the GPU (tal_agg_round_clique_half_f32 / _bf16): clique blocks of 129..256 members, two
lanes per column, bit for bit against the C oracle's round of the mode (fp32 and bf16, EXACT and
FMA; bf16 NaN stored as 0xFFFF) through ops.round_* on plans of max_members=256, plus the
cross-check against K3c1 on a block both take and a round through RoundExecutor."""
import ctypes

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import reference_alg as ra
from topology_aware_learning_amd import _lib, ops
from topology_aware_learning_amd.arena import ModelPool, StateLayout
from topology_aware_learning_amd.round import RoundExecutor

from _clique import MODES, bits, count, inputs, np_dtype, oracle_round, round_of, run, same, tdtype, to_dev

pytestmark = pytest.mark.gpu

SENTINEL = {False: 0x40E01234, True: 0x1234}  # fp32 / bf16 bits of an untouched output element
DENORMAL = {False: 0x00000003, True: 0x0003}


# graph, the nodes that aggregate (None: all), (K3c blocks, K3c1 blocks, K3c2 blocks, a rest plan)
_GRAPHS = {
    "complete129": (lambda: nx.complete_graph(129), None, (0, 0, 1, False)),  # MMAX 160: one member past H, padding in the high half
    "complete160": (lambda: nx.complete_graph(160), None, (0, 0, 1, False)),  # no padding
    "complete161": (lambda: nx.complete_graph(161), None, (0, 0, 1, False)),  # the next rung
    "complete256": (lambda: nx.complete_graph(256), None, (0, 0, 1, False)),  # the largest block
    "partial200": (lambda: nx.complete_graph(200), [i for i in range(200) if i % 3 != 1], (0, 0, 1, False)),
    "three_forms": (lambda: nx.disjoint_union_all([nx.complete_graph(m) for m in (40, 100, 200)]), None, (1, 1, 1, False)),
    "beside_ring": (lambda: nx.disjoint_union(nx.complete_graph(200), nx.cycle_graph(12)), None, (0, 0, 1, True)),
}
# width -> layout (_place): a partial wavefront, 31 columns, one wavefront and a column, several wavefronts
_WIDTHS = {1: "even", 31: "odd", 33: "offset", 97: "even"}


def _place(host_bits, bf16, dev, layout):
    """Zero-padded device pool: "even" / "odd" row stride, "offset": odd and one element into its buffer."""
    rows, n = host_bits.shape
    ld = n + 2 + (n + (layout != "even")) % 2
    buf = torch.zeros(rows * ld + 1, dtype=tdtype(bf16), device=dev)
    t = buf[int(layout == "offset"):][: rows * ld].view(rows, ld)
    t[:, :n] = to_dev(host_bits, bf16, dev)
    return t


def _inputs(rows, n, seed, bf16):
    """_clique.inputs (NaN, -0.0 and +-inf columns, the specials) and a column of denormals."""
    pool, _ = inputs(rows, n, seed, bf16)
    if n > 7:
        pool[:, 7] = DENORMAL[bf16]
        pool[1::2, 7] |= 0x8000 if bf16 else 0x80000000
    return pool


def _check(cuda, pool, csr, out_rows, plan, n, bf16, layout):
    """Both modes: the output pool is the oracle's round on a pool of sentinels, bit for bit."""
    pin = _place(pool, bf16, cuda, layout)
    blank = np.full(pool.shape, SENTINEL[bf16], np_dtype(bf16))
    for mode in MODES:
        pout = _place(blank, bf16, cuda, layout)
        run(pin, pout, plan, n, mode)
        ref = oracle_round(pool, csr, out_rows, bf16, exact=(mode == ops.MODE_EXACT), pool_out=blank.copy())
        got = bits(pout)
        assert same(got[:, :n], ref, nan_payloads_free=not bf16), mode
        assert not got[:, n:].any()  # nothing written past the round's width


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", list(_WIDTHS))
@pytest.mark.parametrize("graph", list(_GRAPHS))
def test_round_clique_half_vs_oracle(cuda, graph, n, bf16):
    """Uniform weights 1 / m (negative at n = 31), output row = node id; rows that do not aggregate
    keep their sentinel."""
    make, who, blocks = _GRAPHS[graph]
    g = make()
    orders, ws = round_of(g, "uniform", who=who, n=n // 16)
    csr = ra.round_csr(orders, ws)
    out_rows = np.array(sorted(g.nodes) if who is None else who, dtype=np.int32)
    plan = ops.build_clique_plan(*csr, out_rows, bf16=bf16, max_members=256)
    assert (plan.n_cliques, plan.n_col, plan.n_half, plan.rest is not None) == blocks
    # K3c's column pairs need the even stride; every other plan here has no alignment rule
    layout = "even" if plan.n_cliques else _WIDTHS[n]
    _check(cuda, _inputs(g.number_of_nodes(), n, len(orders) + n, bf16), csr, out_rows, plan, n, bf16, layout)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
def test_block_of_100_equals_k3c1(cuda, bf16, mode):
    """Blocks of <= 128 members are legal input: complete(100) as a hand-built record (MMAX 160:
    20 members in the high half) gives K3c1's bits."""
    n = 97
    orders, ws = round_of(nx.complete_graph(100), "uniform", n=1)
    plan = ops.build_clique_plan(*ra.round_csr(orders, ws), np.arange(100, dtype=np.int32), bf16=bf16, max_members=128)
    c = plan.col_table.reshape(1, ops.CLIQUE_COL_WORDS)[0]
    h = np.full(ops.CLIQUE_HALF_WORDS, -1, np.int32)
    h[:4], h[4: 4 + ops.CLIQUE_HALF_MAX] = c[:4], 0
    h[4: 4 + 128], h[4 + 256: 4 + 256 + 128] = c[4: 4 + 128], c[4 + 128:]
    table = torch.from_numpy(h).to(cuda)
    pin = _place(_inputs(100, n, 7, bf16), bf16, cuda, "odd")
    want, pout = torch.zeros_like(pin), torch.zeros_like(pin)
    run(pin, want, plan, n, mode)
    fn = getattr(_lib.load(), "tal_agg_round_clique_half_" + ("bf16" if bf16 else "f32"))
    ops.check(fn(ctypes.c_void_p(pin.data_ptr()), pin.stride(0), ctypes.c_void_p(pout.data_ptr()), pout.stride(0), n,
                 ctypes.c_void_p(table.data_ptr()), 1, 100, int(mode), ops._stream(cuda, None)))
    torch.cuda.synchronize()
    assert np.array_equal(bits(pout), bits(want))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_round_executor_complete129(cuda, monkeypatch, bf16):
    """RoundExecutor on a small ModelPool with the plan of spec {"clique": 1, "members": 256} passed
    in: every row is the oracle round of the pre-round snapshot, by one call of the new entry."""
    n = 97
    layout = StateLayout.from_layout([("w", (n,), "bfloat16" if bf16 else "float32")])
    orders, ws = round_of(nx.complete_graph(129), "uniform")
    csr = ra.round_csr(orders, ws)
    out_rows = np.arange(129, dtype=np.int32)
    plan = ops.plan_from_spec(*csr, out_rows, {"clique": 1, "members": 256, "rest": None}).to(cuda)
    assert (plan.n_cliques, plan.n_col, plan.n_half, plan.half_mmax) == (0, 0, 1, 129)
    plan.rest_rows = None  # every row aggregates: nothing to carry into the spare (RoundExecutor.plan's form)
    pool = ModelPool(layout, 129, cuda)
    before = _inputs(129, n, 4, bf16)
    (pool.b16 if bf16 else pool.f32)[:, :n].copy_(to_dev(before, bf16, cuda))
    new = count(monkeypatch, "tal_agg_round_clique_half_" + ("bf16" if bf16 else "f32"))
    RoundExecutor(pool, mode=ops.MODE_EXACT, placement_trials=1).run(orders, ws, plan=plan)
    assert same(bits((pool.b16 if bf16 else pool.f32)[:, :n]), oracle_round(before, csr, out_rows, bf16), nan_payloads_free=not bf16)
    assert new.calls == 1
