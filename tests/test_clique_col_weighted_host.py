"""K3c1 with per-source weights, host side (no GPU): per-source clique blocks of 65..128 members
(tal_agg_round_clique_col_w_*).  The planner's `wide_per_source` keyword - what it admits, where
the blocks and their weights go (CliquePlan.col_table / col_wtable), and that nothing changes
without it - the spec, the tuner's candidate, default_plan against WCLIQUE_COL_DEFAULT, and the
C-ABI entries' declarations and argument errors."""
import ctypes
import re

import networkx as nx
import numpy as np
import pytest

import bench
from topology_aware_learning_amd import _lib, ops
from topology_aware_learning_amd import weights as tw
from topology_aware_learning_amd.build import HDR
from topology_aware_learning_amd.round import csr_from_lists

NAMES = ("tal_agg_round_clique_col_w_f32", "tal_agg_round_clique_col_w_bf16")
MODES = (ops.MODE_EXACT, ops.MODE_FMA)
WIDE = dict(per_source=True, max_members=128, wide_per_source=True)

_GRAPHS = {
    "complete65": lambda: nx.complete_graph(65),
    "complete100": lambda: nx.complete_graph(100),
    "complete128": lambda: nx.complete_graph(128),
    "two_blocks": lambda: nx.disjoint_union(nx.complete_graph(70), nx.complete_graph(100)),
    "mixed": lambda: nx.disjoint_union(nx.disjoint_union(nx.complete_graph(20), nx.complete_graph(100)),
                                       nx.random_regular_graph(4, 30, seed=1)),
    "barbell66": lambda: nx.barbell_graph(66, 3),
}


def _lists(g, kind="datasize"):
    """(orders, weights) of graph g: data-size weights (all distinct), softmax of 10 x the degree
    centrality, or uniform 1 / len."""
    g = _GRAPHS[g]() if isinstance(g, str) else g
    nodes = sorted(g.nodes)
    orders = [sorted(g.neighbors(i)) + [i] for i in nodes]
    if kind == "datasize":
        lens = (np.random.default_rng(5).permutation(len(nodes)) * 37 + 101).tolist()
        return orders, [tw.weighted([lens[j] for j in o]) for o in orders]
    if kind == "degcent":
        cent = nx.degree_centrality(g)
        return orders, [tw.centrality(o, cent, True, 10.0) for o in orders]
    return orders, [[1.0 / len(o)] * len(o) for o in orders]


def _csr_of(g, kind="datasize"):
    orders, ws = _lists(g, kind)
    rp, col, w = csr_from_lists(orders, ws)
    return rp, col, w, np.arange(len(orders), dtype=np.int32)


def _w32(ws_row):
    return np.asarray(ws_row, np.float64).astype(np.float32)


def _col(plan):
    return plan.col_table.reshape(plan.n_col, ops.CLIQUE_COL_WORDS)


def _colw(plan):
    return plan.col_wtable.reshape(plan.n_col, ops.CLIQUE_COL_WWORDS)


@pytest.mark.parametrize("graph,blocks,n64,rest_rows", [
    ("complete65", [(65, 65)], 0, []),
    ("complete100", [(100, 100)], 0, []),
    ("complete128", [(128, 128)], 0, []),
    ("two_blocks", [(70, 70), (100, 100)], 0, []),
    ("mixed", [(100, 100)], 1, list(range(120, 150))),
    ("barbell66", [(66, 65), (66, 65)], 0, [65, 66, 67, 68, 69]),
])
def test_blocks_found(graph, blocks, n64, rest_rows):
    """(sources, rows) of every block above 64 members, the <= 64 blocks beside them and the rest
    rows, under data-size weights; a block above 64 attaches nothing."""
    csr = _csr_of(graph)
    cliques, rest = ops.find_cliques(*csr, **WIDE)
    wide = [c for c in cliques if len(c[0]) > 64]
    assert [(len(c[0]), len(c[2])) for c in wide] == blocks and all(c[3] == [] for c in wide)
    assert len(cliques) - len(wide) == n64 and rest == rest_rows
    p = ops.build_clique_plan(*csr, **WIDE)
    assert (p.n_cliques, p.n_col, p.col_mmax) == (n64, len(blocks), max(b[0] for b in blocks))
    assert p.rest_rows == rest_rows and (p.rest is None) == (not rest_rows)
    assert p.wtable is not None and p.col_wtable is not None and p.spec_key == "wclique"
    assert p.clique_rows == sum(b[1] for b in blocks) + (20 if n64 else 0)
    assert ops.round_kernel_name(p) == ("k_round_clique" if n64 else "k_round_clique_col")
    assert ops.build_clique_plan(*csr, max_members=128) is None  # no uniform block in these rounds


def test_barbell66_degree_centrality_blocks():
    """barbell(66, 3) under degree-centrality softmax weights: two weights per block (the bridge
    member's and the others'), the same two blocks, bridges and path rows in the rest plan."""
    csr = _csr_of("barbell66", "degcent")
    cliques, rest = ops.find_cliques(*csr, **WIDE)
    assert [(len(c[0]), len(c[2])) for c in cliques] == [(66, 65), (66, 65)] and rest == [65, 66, 67, 68, 69]
    assert all(len(set(c[1].view(np.uint32).tolist())) == 2 for c in cliques)


@pytest.mark.parametrize("graph", ["complete65", "two_blocks", "barbell66"])
def test_col_wtable_contents(graph):
    """col_wtable: w[j] = the fp32 bits source j carries in the block's rows, 1.0 in unused slots;
    col_table is the uniform form's record with a zero weight word."""
    orders, ws = _lists(graph)
    csr = _csr_of(graph)
    p = ops.build_clique_plan(*csr, **WIDE)
    assert ops.CLIQUE_COL_WWORDS == 128
    assert p.col_wtable.dtype == np.float32 and p.col_wtable.shape == (p.n_col * 128,)
    for rec, wrec in zip(_col(p), _colw(p)):
        m = int(rec[0])
        srcs = rec[4: 4 + m].tolist()
        assert rec[1] == 0 and rec[2] == 0 and rec[3] == 0
        member = next(i for i in range(m) if rec[4 + 128 + i] >= 0)
        r = int(rec[4 + 128 + member])  # out_row == CSR row here
        w_of = dict(zip(orders[r], _w32(ws[r]).view(np.uint32).tolist()))
        assert wrec[:m].view(np.uint32).tolist() == [w_of[s] for s in srcs]
        assert np.all(wrec[m:].view(np.uint32) == np.float32(1.0).view(np.uint32))
        assert np.all(rec[4 + m: 4 + 128] == 0) and np.all(rec[4 + 128 + m:] == -1)


def test_one_ulp_and_non_finite_rows_stay_out():
    """A row whose weight for one source differs by one ulp, and rows with an inf or NaN weight,
    are not in the block: they go to the rest plan, the other 97 rows keep their block."""
    orders, ws = _lists("complete100")
    ws = [list(_w32(r).astype(np.float64)) for r in ws]
    ws[7][3] = float(np.nextafter(np.float32(ws[7][3]), np.float32(1.0)))
    ws[11][0] = float("inf")
    ws[50][20] = float("nan")
    rp, col, w = csr_from_lists(orders, ws)
    out = np.arange(100, dtype=np.int32)
    cliques, rest = ops.find_cliques(rp, col, w, out, **WIDE)
    assert len(cliques) == 1 and len(cliques[0][0]) == 100 and len(cliques[0][2]) == 97
    assert rest == [7, 11, 50]
    p = ops.build_clique_plan(rp, col, w, out, **WIDE)
    rows = _col(p)[0, 4 + 128:]
    assert int((rows >= 0).sum()) == 97 and all(rows[i] == -1 for i in (7, 11, 50))


def test_blocks_of_129_go_to_rest():
    csr = _csr_of(nx.complete_graph(129))
    assert ops.find_cliques(*csr, **WIDE) == ([], list(range(129)))
    assert ops.build_clique_plan(*csr, **WIDE) is None
    csr = _csr_of(nx.disjoint_union(nx.complete_graph(100), nx.complete_graph(129)))
    p = ops.build_clique_plan(*csr, **WIDE)
    assert p.n_col == 1 and p.rest_rows == list(range(100, 229)) and p.rest.info.rows == 129
    for fn in (ops.find_cliques, ops.build_clique_plan):
        with pytest.raises(ValueError):
            fn(*csr, per_source=True, max_members=129, wide_per_source=True)


def test_small_and_wide_block_in_one_plan():
    """complete(20) u complete(100): the K3c record and wtable are byte for byte those of the <= 64
    plan of the same round; the 100 block is the col record."""
    csr = _csr_of(nx.disjoint_union(nx.complete_graph(20), nx.complete_graph(100)))
    p = ops.build_clique_plan(*csr, **WIDE)
    q = ops.build_clique_plan(*csr, per_source=True)
    assert (p.n_cliques, p.mmax, p.n_col, p.col_mmax) == (1, 20, 1, 100) and p.rest is None
    assert q.n_cliques == 1 and q.col_table is None and q.col_wtable is None and q.rest_rows == list(range(20, 120))
    assert p.table.tobytes() == q.table.tobytes() and p.wtable.tobytes() == q.wtable.tobytes()
    assert _col(p)[0, 4: 104].tolist() == list(range(20, 120))
    assert p.clique_sources == 120 and p.clique_rows == 120
    moved = p.to("cpu")
    assert moved.col_wdevice.numpy().tobytes() == p.col_wtable.tobytes()
    assert moved.col_device.numpy().tobytes() == p.col_table.tobytes()


def _default_rounds():
    yield "complete65", _csr_of("complete65", "uniform")
    yield "complete100", _csr_of("complete100", "uniform")
    yield "barbell60_8", _csr_of(nx.barbell_graph(60, 8), "uniform")
    for kind, n, deg in (("ring", 32, 2), ("random", 64, 8), ("barbell", 128, 0), ("sbm", 256, 0)):  # configs 2-5
        orders, ws = bench.round_spec(n, deg, kind=kind)
        rp, col, w = csr_from_lists(orders, ws)
        yield kind, (rp, col, w, np.arange(len(orders), dtype=np.int32))
    yield "complete100_datasize", _csr_of("complete100")
    yield "barbell60_8_datasize", _csr_of(nx.barbell_graph(60, 8))


@pytest.mark.parametrize("name,csr", list(_default_rounds()), ids=[n for n, _ in _default_rounds()])
def test_without_the_keyword_nothing_changes(name, csr):
    """Default calls, and calls with wide_per_source=False spelled out, give the tables of a call
    with wide_per_source=True held to 64 members (the keyword alone admits nothing), no block above
    64 under per_source, and no col_wtable."""
    for per_source in (False, True):
        for mm in (None, 64):
            kw = dict(per_source=per_source, **({} if mm is None else {"max_members": mm}))
            c0, r0 = ops.find_cliques(*csr, **kw)
            c1, r1 = ops.find_cliques(*csr, wide_per_source=True, **kw)
            assert r0 == r1 and [c[0] for c in c0] == [c[0] for c in c1] and all(len(c[0]) <= 64 for c in c0)
            p = ops.build_clique_plan(*csr, **kw)
            q = ops.build_clique_plan(*csr, wide_per_source=True, **kw)
            assert (p is None) == (q is None)
            if p is not None:
                assert p.col_table is None and p.col_wtable is None and p.col_wdevice is None
                assert p.table.tobytes() == q.table.tobytes() and p.rest_rows == q.rest_rows
                assert (p.wtable is None) == (not per_source)
                if per_source:
                    assert p.wtable.tobytes() == q.wtable.tobytes()
    # the uniform 128-member plan carries no weight table either
    u = ops.build_clique_plan(*csr, max_members=128)
    if u is not None:
        assert u.col_wtable is None and u.wtable is None
        v = ops.build_clique_plan(*csr, max_members=128, wide_per_source=True)
        assert v.col_wtable is None and (v.col_table is None) == (u.col_table is None)
        assert u.col_table is None or u.col_table.tobytes() == v.col_table.tobytes()


def test_limit_errors_without_the_keyword():
    small = _csr_of(nx.complete_graph(70), "uniform")
    for fn in (ops.find_cliques, ops.build_clique_plan):
        with pytest.raises(ValueError):
            fn(*small, max_members=129)
        with pytest.raises(ValueError):
            fn(*small, per_source=True, max_members=128)
        with pytest.raises(ValueError):
            fn(*small, per_source=True, max_members=65)
        with pytest.raises(ValueError):
            fn(*small, per_source=True, max_members=128, wide_per_source=False)
    assert ops.find_cliques(*small, per_source=True, max_members=64)[0] == []
    assert len(ops.find_cliques(*small, per_source=True, max_members=128, wide_per_source=True)[0]) == 1


def test_spec_round_trip():
    csr = _csr_of("mixed")
    p = ops.build_clique_plan(*csr, **WIDE)
    spec = {"wclique": 1, "members": 128, "rest": p.rest.spec}
    q = ops.plan_from_spec(*csr, spec)
    assert q.spec == spec and (q.n_cliques, q.n_col) == (1, 1)
    assert q.col_table.tobytes() == p.col_table.tobytes() and q.col_wtable.tobytes() == p.col_wtable.tobytes()
    assert q.table.tobytes() == p.table.tobytes() and q.wtable.tobytes() == p.wtable.tobytes()
    assert q.rest.spec == p.rest.spec and q.rest_rows == p.rest_rows
    # {"wclique": 1} keeps meaning 64: the 20 block alone, and on complete(100) no block at all
    q64 = ops.plan_from_spec(*csr, {"wclique": 1, "rest": None})
    assert q64.n_col == 0 and q64.col_wtable is None and q64.table.tobytes() == p.table.tobytes()
    with pytest.raises(ValueError):
        ops.plan_from_spec(*_csr_of("complete100"), {"wclique": 1})
    # "clique" with members 128 stays the uniform form: a ValueError on a round without uniform blocks
    with pytest.raises(ValueError):
        ops.plan_from_spec(*_csr_of("complete100"), {"clique": 1, "members": 128})


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_tuner_candidate_and_default(bf16, mode, monkeypatch):
    """tune_candidates offers ("wclique128",) exactly once for complete(100) under data-size
    weights (where WCLIQUE_COL_DEFAULT makes that plan the default it is candidate 0 instead, as
    with "clique128"), never for complete(40) under data-size weights nor for the unweighted
    complete(100); default_plan follows WCLIQUE_COL_DEFAULT, and rounds without a per-source block
    above 64 members keep their plan under either setting."""
    big = _csr_of("complete100")
    for on in (False, True):
        monkeypatch.setitem(ops.WCLIQUE_COL_DEFAULT, (bf16, mode), on)
        cands = ops.tune_candidates(*big, bf16=bf16, mode=mode)
        keys = [k for k, _ in cands]
        d = ops.default_plan(*big, bf16=bf16, mode=mode)
        if on:
            assert isinstance(d, ops.CliquePlan) and (d.n_cliques, d.n_col, d.col_mmax) == (0, 1, 100)
            assert d.col_wtable is not None and d.spec == {"wclique": 1, "members": 128, "rest": None}
            assert ("wclique128",) not in keys  # it is the default, candidate 0
            assert isinstance(cands[0][1], ops.CliquePlan) and cands[0][1].col_wtable is not None
        else:
            assert isinstance(d, ops.RoundPlan) and d.info.dense_rb == 0 and d.info.stream_cs == 0
            assert keys.count(("wclique128",)) == 1
            yp = dict(cands)[("wclique128",)]
            assert yp.n_col == 1 and yp.col_wtable is not None
            assert yp.spec == {"wclique": 1, "members": 128, "rest": None}
        for other, kind in (("complete100", "uniform"), (nx.complete_graph(40), "datasize"),
                            (nx.barbell_graph(60, 8), "degcent")):
            csr = _csr_of(other, kind)
            ks = [k for k, _ in ops.tune_candidates(*csr, bf16=bf16, mode=mode)]
            assert ("wclique128",) not in ks, (other, kind)
            dd = ops.default_plan(*csr, bf16=bf16, mode=mode)
            monkeypatch.setitem(ops.WCLIQUE_COL_DEFAULT, (bf16, mode), False)
            d0 = ops.default_plan(*csr, bf16=bf16, mode=mode)
            monkeypatch.setitem(ops.WCLIQUE_COL_DEFAULT, (bf16, mode), on)
            assert type(dd) is type(d0) and dd.spec == d0.spec
            if isinstance(dd, ops.CliquePlan):
                assert dd.col_wtable is None and dd.table.tobytes() == d0.table.tobytes()
                assert (dd.col_table is None) == (d0.col_table is None)


def test_default_table_covers_every_dtype_and_mode():
    assert set(ops.WCLIQUE_COL_DEFAULT) == {(b, m) for b in (False, True) for m in MODES}
    assert all(isinstance(v, bool) for v in ops.WCLIQUE_COL_DEFAULT.values())


def test_symbols_declared_exported_bound():
    L = _lib.load()
    assert L.tal_abi_version() == _lib.ABI_VERSION >= 34
    header = HDR.read_text()
    assert re.search(r"#define\s+TAL_CLIQUE_COL_WWORDS\s+128\b", header)
    assert re.search(r"#define\s+TAL_CLIQUE_COL_WORDS\s+260\b", header)
    assert re.search(r"static_assert\(TAL_CLIQUE_COL_WWORDS\s*==", header)
    for name, ctype in zip(NAMES, ("float", "uint16_t")):
        assert name in _lib.EXPORTED and _lib._SIGS[name] == _lib._SIGS["tal_agg_round_clique_w_f32"]
        assert getattr(L, name).argtypes == _lib._SIGS[name][1]
        decl = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl is not None
        assert re.sub(r"\s+", " ", decl.group(1)).strip() == (
            f"const {ctype}* pool_in, int64_t ld_in, {ctype}* pool_out, int64_t ld_out, int64_t n, "
            "const int32_t* table_dev, int32_t n_cliques, int32_t mmax, int32_t mode, void* stream, "
            "const float* wtab_dev")


@pytest.mark.parametrize("case,args,message", [
    ("null pool_in", (None, 64, 0x2000, 64, 64, 0x3000, 1, 100, 0x4000), b"null"),
    ("null pool_out", (0x1000, 64, None, 64, 64, 0x3000, 1, 100, 0x4000), b"null"),
    ("null table", (0x1000, 64, 0x2000, 64, 64, None, 1, 100, 0x4000), b"null"),
    ("null wtab", (0x1000, 64, 0x2000, 64, 64, 0x3000, 1, 100, None), b"null"),
    ("in place", (0x1000, 64, 0x1000, 64, 64, 0x3000, 1, 100, 0x4000), b"out of place"),
    ("mmax 0", (0x1000, 64, 0x2000, 64, 64, 0x3000, 1, 0, 0x4000), b"mmax"),
    ("mmax 129", (0x1000, 64, 0x2000, 64, 64, 0x3000, 1, 129, 0x4000), b"mmax"),
    ("65536 blocks", (0x1000, 64, 0x2000, 64, 64, 0x3000, 65536, 100, 0x4000), b"n_cliques"),
    ("ld_in < n", (0x1000, 63, 0x2000, 64, 64, 0x3000, 1, 100, 0x4000), b"ld"),
    ("ld_out < n", (0x1000, 64, 0x2000, 63, 64, 0x3000, 1, 100, 0x4000), b"ld"),
])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_argument_errors(name, case, args, message, mode):
    """Each is TAL_ERR_INVALID with a message naming the entry, found before any GPU work (the
    pointers are not memory)."""
    L = _lib.load()
    pin, ld_in, pout, ld_out, n, table, n_cliques, mmax, wtab = args
    rc = getattr(L, name)(ctypes.c_void_p(pin), ld_in, ctypes.c_void_p(pout), ld_out, n, ctypes.c_void_p(table),
                          n_cliques, mmax, mode, None, ctypes.c_void_p(wtab))
    err = L.tal_last_error()
    assert rc == _lib.TAL_ERR_INVALID, case
    assert name.encode() in err and message in err, (case, err)


@pytest.mark.parametrize("name", NAMES)
def test_odd_ld_and_element_offsets_are_not_errors(name):
    """No column-pair rule here either: an odd ld and element-aligned pools pass the argument
    checks, for any mmax <= 128 (n = 0: accepted with nothing to launch)."""
    L = _lib.load()
    for mmax in (1, 40, 128):
        rc = getattr(L, name)(ctypes.c_void_p(0x1002), 65, ctypes.c_void_p(0x2006), 67, 0, ctypes.c_void_p(0x3000),
                              1, mmax, ops.MODE_EXACT, None, ctypes.c_void_p(0x4000))
        assert rc == 0, L.tal_last_error()
