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

pytestmark = pytest.mark.gpu

MODES = [ops.MODE_EXACT, ops.MODE_FMA]
SENTINEL = {False: 0x40E01234, True: 0x1234}  # fp32 / bf16 bits of an untouched output element
SPECIALS = [1e-40, -0.0, 3.3e38, -1e-45, 65504.0, 1.17e-38, -3.3e38, 2.0 ** -133, 0.0, 1.0, -1.0, 3.0e38]

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


def _np_dtype(bf16):
    return np.uint16 if bf16 else np.uint32


def _tdtype(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _to_dev(bits, bf16, dev):
    """Host bit array -> device tensor of the storage type."""
    a = np.ascontiguousarray(bits)
    return torch.from_numpy(a.view(np.int16 if bf16 else np.int32)).view(_tdtype(bf16)).to(dev)


def _bits(t):
    bf16 = t.dtype == torch.bfloat16
    return t.cpu().contiguous().view(torch.int16 if bf16 else torch.int32).numpy().view(_np_dtype(bf16))


def _sentinel_pool(rows, ld, bf16, dev):
    return _to_dev(np.full((rows, ld), SENTINEL[bf16], _np_dtype(bf16)), bf16, dev)


def _round_of(graph, n, who=None):
    g = _GRAPHS[graph]() if isinstance(graph, str) else graph
    nodes = sorted(g.nodes) if who is None else who
    orders = [sorted(g.neighbors(i)) + [i] for i in nodes]
    sign = -1.0 if n % 2 else 1.0  # signed weights: negative for odd n
    ws = [[sign / len(o)] * len(o) for o in orders]
    return orders, ws


def _inputs(rows, n, seed, bf16):
    """Pool bits [rows, n].  Row 0: the specials (n > 12); member 1 holds a payload NaN in one
    column; a column of -0.0; +inf / -inf in every third row of another."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, n)) * 3.0).astype(np.float32)
    if n > 12:
        x[0, :12] = SPECIALS
    pool = oracle.f32_to_bf16(x) if bf16 else x.view(np.uint32).copy()
    nan_col = 3 if n > 3 else 0
    pool[1, nan_col] = 0x7FC1 if bf16 else 0x7FC00001
    if n > 5:
        pool[:, 5] = 0x8000 if bf16 else 0x80000000
    if n > 6:
        pool[::3, 6] = 0x7F80 if bf16 else 0x7F800000
        pool[3::6, 6] = 0xFF80 if bf16 else 0xFF800000
    return pool, nan_col


def _padded(pool, bf16, dev, odd=True):
    """Device copy with a padded row stride: odd on purpose (no column-pair rule here), even for
    plans that also hold K3c blocks."""
    rows, n = pool.shape
    ld = n + 2 + ((n + odd) % 2)
    assert ld % 2 == int(odd)
    pin = torch.zeros(rows, ld, dtype=_tdtype(bf16), device=dev)
    pin[:, :n] = _to_dev(pool, bf16, dev)
    return pin


def _oracle(pool, csr, out_rows, bf16, exact=True, pool_out=None):
    row_ptr, col, w = csr
    if bf16:
        return oracle.round_bf16(pool, row_ptr, col, w, out_rows, pool_out=pool_out, exact=exact)
    out = oracle.round_f32(pool.view(np.float32), row_ptr, col, w, out_rows,
                           pool_out=None if pool_out is None else pool_out.view(np.float32))
    return out.view(np.uint32)


def _same(got, ref, bf16):
    """Bit for bit; on fp32 a NaN matches a NaN (payloads are not the oracle's to pin)."""
    if bf16:
        return np.array_equal(got, ref)
    ng, nr = np.isnan(got.view(np.float32)), np.isnan(ref.view(np.float32))
    return np.array_equal(ng, nr) and np.array_equal(got[~ng], ref[~nr])


def _is_nan(bits, bf16):
    return bits == 0xFFFF if bf16 else np.isnan(np.array([bits], np.uint32).view(np.float32))[0]


def _run(pin, pout, plan, n, mode):
    (ops.round_bf16 if pin.dtype == torch.bfloat16 else ops.round_f32)(pin, pout, plan, n=n, mode=mode)


def _k1_fma(pin, orders, ws, r, n):
    bf16 = pin.dtype == torch.bfloat16
    chk = torch.empty(n, dtype=pin.dtype, device=pin.device)
    (ops.agg_bf16 if bf16 else ops.agg_f32)([pin[j, :n] for j in orders[r]], ws[r], chk, mode=ops.MODE_FMA)
    return _bits(chk)


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
    pool, nan_col = _inputs(rows, n, rows + n, bf16)
    pin = _padded(pool, bf16, cuda, odd=plan.n_cliques == 0)
    for mode in MODES:
        pout = _sentinel_pool(rows + 2, pin.shape[1], bf16, cuda)
        _run(pin, pout, plan, n, mode)
        got = _bits(pout)
        if mode == ops.MODE_EXACT or bf16:
            ref = _oracle(pool, csr, out_rows - 2, bf16, exact=(mode == ops.MODE_EXACT))
            assert _same(got[2:, :n], ref, bf16), (graph, n, mode)
        if mode == ops.MODE_FMA:
            for r in (0, rows // 2, rows - 1):
                assert _same(got[out_rows[r], :n], _k1_fma(pin, orders, ws, r, n), bf16), (graph, n, r)
        for r in range(rows):
            if 1 in orders[r]:
                assert _is_nan(got[out_rows[r], nan_col], bf16), (r, mode)
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
    pool, _ = _inputs(100, n, 11, bf16)
    pin = _padded(pool, bf16, cuda)
    for mode in MODES:
        pout = _sentinel_pool(100, pin.shape[1], bf16, cuda)
        _run(pin, pout, plan, n, mode)
        got = _bits(pout)
        if mode == ops.MODE_EXACT or bf16:
            ref = _oracle(pool, csr, out_rows, bf16, exact=(mode == ops.MODE_EXACT),
                          pool_out=np.full((100, n), SENTINEL[bf16], _np_dtype(bf16)))
            assert _same(got[:, :n], ref, bf16), mode
        else:
            for k in (0, 18, 36):
                assert _same(got[who[k], :n], _k1_fma(pin, orders, ws, k, n), bf16), k
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
    pool, _ = _inputs(40, n, 40 + n, bf16)
    pin = _padded(pool, bf16, cuda, odd=False)
    table = torch.from_numpy(_col_table_of(plan).reshape(-1)).to(cuda)
    L = _lib.load()
    fn = getattr(L, "tal_agg_round_clique_col_bf16" if bf16 else "tal_agg_round_clique_col_f32")
    for mode in MODES:
        want = _sentinel_pool(40, pin.shape[1], bf16, cuda)
        _run(pin, want, plan, n, mode)
        pout = _sentinel_pool(40, pin.shape[1], bf16, cuda)
        ops.check(fn(ctypes.c_void_p(pin.data_ptr()), pin.stride(0), ctypes.c_void_p(pout.data_ptr()), pout.stride(0),
                     n, ctypes.c_void_p(table.data_ptr()), 1, 40, int(mode), ops._stream(cuda, None)))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(pout), _bits(want)), mode
        if mode == ops.MODE_EXACT:
            assert _same(_bits(want)[:, :n], _oracle(pool, csr, out_rows, bf16), bf16)


class _Counter:
    """A library entry point wrapped in a counting Python callable."""

    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *args):
        self.calls += 1
        return self.fn(*args)


def _count(monkeypatch, name):
    L = _lib.load()
    c = _Counter(getattr(L, name))
    monkeypatch.setattr(L, name, c)
    return c


def _entries(monkeypatch, bf16):
    t = "bf16" if bf16 else "f32"
    return (_count(monkeypatch, f"tal_agg_round_clique_col_{t}"), _count(monkeypatch, f"tal_agg_round_clique_{t}"),
            _count(monkeypatch, f"tal_agg_round_{t}"))


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
        pool, _ = _inputs(rows, n, 3, bf16)
        pin = _padded(pool, bf16, cuda, odd=False)
        pout = torch.zeros_like(pin)
        before = (col.calls, k3c.calls, regular.calls)
        _run(pin, pout, plan, n, mode)
        assert (col.calls - before[0], k3c.calls - before[1], regular.calls - before[2]) == want, graph
        if mode == ops.MODE_EXACT or bf16:
            assert _same(_bits(pout)[:, :n], _oracle(pool, csr, out_rows, bf16, exact=(mode == ops.MODE_EXACT)), bf16)
        with pytest.raises(ValueError):
            _run(pin, pin, plan, n, mode)
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
    pool, _ = _inputs(100, n, 9, bf16)
    aligned = _padded(pool, bf16, cuda, odd=False)
    want = torch.zeros_like(aligned)
    _run(aligned, want, plan, n, mode)
    want = _bits(want)[:, :n]
    if mode == ops.MODE_EXACT or bf16:
        assert _same(want, _oracle(pool, csr, out_rows, bf16, exact=(mode == ops.MODE_EXACT)), bf16)
    col, k3c, regular = _entries(monkeypatch, bf16)
    ld = aligned.shape[1] + 1  # odd
    assert ld % 2 == 1
    esize = aligned.element_size()
    src = torch.zeros(100 * ld + 1, dtype=aligned.dtype, device=cuda)[1:].view(100, ld)
    dst = torch.zeros(100 * ld + 1, dtype=aligned.dtype, device=cuda)[1:].view(100, ld)
    assert src.data_ptr() % (2 * esize) == esize and dst.data_ptr() % (2 * esize) == esize
    src[:, : aligned.shape[1]] = aligned
    _run(src, dst, plan, n, mode)
    assert np.array_equal(_bits(dst)[:, :n], want)
    assert (col.calls, k3c.calls, regular.calls) == (1, 0, 0)
