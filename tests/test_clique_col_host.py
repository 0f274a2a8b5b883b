"""K3c1, host side (no GPU): clique blocks of 65..128 members (one column per lane,
tal_agg_round_clique_col_*).  The planner's `max_members` parameter - what it admits, where the
blocks go (CliquePlan.col_table), and that nothing changes without it - the spec, the tuner's
candidate, default_plan against CLIQUE_COL_DEFAULT, and the C-ABI entries' argument errors."""
import ctypes
import re

import networkx as nx
import numpy as np
import pytest

import bench
from topology_aware_learning_amd import _lib, ops
from topology_aware_learning_amd.build import HDR
from topology_aware_learning_amd.round import csr_from_lists

NAMES = ("tal_agg_round_clique_col_f32", "tal_agg_round_clique_col_bf16")
MODES = (ops.MODE_EXACT, ops.MODE_FMA)


def _csr_of(g, rows=None):
    """Unweighted round of graph g (neighbors ascending, then self), output rows = node ids;
    rows: the nodes that aggregate (default all)."""
    nodes = sorted(g.nodes) if rows is None else list(rows)
    orders = [sorted(g.neighbors(i)) + [i] for i in nodes]
    ws = [[1.0 / len(o)] * len(o) for o in orders]
    rp, col, w = csr_from_lists(orders, ws)
    return rp, col, w, np.array(nodes, dtype=np.int32)


def _col_records(plan):
    return plan.col_table.reshape(plan.n_col, ops.CLIQUE_COL_WORDS)


def test_complete100_plan_record():
    csr = _csr_of(nx.complete_graph(100))
    p = ops.build_clique_plan(*csr, max_members=128)
    assert p is not None
    assert (p.n_cliques, p.n_col, p.col_mmax) == (0, 1, 100) and p.rest is None and p.rest_rows == []
    assert p.table.size == 0 and p.wtable is None
    assert ops.CLIQUE_COL_MAX == 128 and ops.CLIQUE_COL_WORDS == 4 + 2 * 128
    want = np.zeros(ops.CLIQUE_COL_WORDS, np.int32)
    want[0] = 100
    want[1] = np.array([1.0 / 100], np.float64).astype(np.float32).view(np.int32)[0]
    want[4: 4 + 100] = np.arange(100)             # sources ascending
    want[4 + 128:] = -1
    want[4 + 128: 4 + 128 + 100] = np.arange(100)  # out_row by member
    assert p.col_table.dtype == np.int32 and np.array_equal(_col_records(p)[0], want)
    assert p.clique_sources == 100 and p.clique_rows == 100 and p.staged_rows() == 100
    assert ops.round_kernel_name(p) == "k_round_clique_col"


def _default_rounds():
    yield "complete65", _csr_of(nx.complete_graph(65))
    yield "complete100", _csr_of(nx.complete_graph(100))
    yield "barbell60_8", _csr_of(nx.barbell_graph(60, 8))
    for kind, n, deg in (("ring", 32, 2), ("random", 64, 8), ("barbell", 128, 0), ("sbm", 256, 0)):  # configs 2-5
        orders, ws = bench.round_spec(n, deg, kind=kind)
        rp, col, w = csr_from_lists(orders, ws)
        yield kind, (rp, col, w, np.arange(len(orders), dtype=np.int32))


@pytest.mark.parametrize("name,csr", list(_default_rounds()), ids=[n for n, _ in _default_rounds()])
def test_default_max_members_is_unchanged(name, csr):
    """Without max_members: no block above 64 members, no col_table, and the table's bytes those
    of a plan built with an explicit max_members=64."""
    for per_source in (False, True):
        cliques, rest = ops.find_cliques(*csr, per_source=per_source)
        assert all(len(c[0]) <= 64 for c in cliques)
        c64, r64 = ops.find_cliques(*csr, per_source=per_source, max_members=64)
        assert rest == r64 and [c[0] for c in cliques] == [c[0] for c in c64]
        p = ops.build_clique_plan(*csr, per_source=per_source)
        q = ops.build_clique_plan(*csr, per_source=per_source, max_members=64)
        assert (p is None) == (q is None) == (not cliques)
        if p is not None:
            assert p.col_table is None and p.n_col == 0 and p.col_mmax == 0
            assert p.table.tobytes() == q.table.tobytes() and (p.n_cliques, p.mmax) == (q.n_cliques, q.mmax)
            assert p.rest_rows == q.rest_rows
    if name in ("complete65", "complete100"):
        assert ops.find_cliques(*csr)[0] == [] and ops.build_clique_plan(*csr) is None


def test_limits():
    p = ops.build_clique_plan(*_csr_of(nx.complete_graph(128)), max_members=128)
    assert p is not None and (p.n_cliques, p.n_col, p.col_mmax) == (0, 1, 128) and p.rest is None
    csr = _csr_of(nx.complete_graph(129))
    cliques, rest = ops.find_cliques(*csr, max_members=128)
    assert cliques == [] and rest == list(range(129))
    assert ops.build_clique_plan(*csr, max_members=128) is None
    # beside a block, the rows of a 129-member one land in the rest plan
    csr = _csr_of(nx.disjoint_union(nx.complete_graph(100), nx.complete_graph(129)))
    p = ops.build_clique_plan(*csr, max_members=128)
    assert p.n_col == 1 and p.rest_rows == list(range(100, 229)) and p.rest is not None and p.rest.info.rows == 129
    small = _csr_of(nx.complete_graph(70))
    for fn in (ops.find_cliques, ops.build_clique_plan):
        with pytest.raises(ValueError):
            fn(*small, max_members=129)
        with pytest.raises(ValueError):
            fn(*small, per_source=True, max_members=128)
        with pytest.raises(ValueError):
            fn(*small, per_source=True, max_members=65)
    assert ops.find_cliques(*small, per_source=True, max_members=64)[0] == []


def test_small_and_large_block_in_one_round():
    csr = _csr_of(nx.disjoint_union(nx.complete_graph(20), nx.complete_graph(100)))
    p = ops.build_clique_plan(*csr, max_members=128)
    assert (p.n_cliques, p.mmax, p.n_col, p.col_mmax) == (1, 20, 1, 100) and p.rest is None and p.rest_rows == []
    t = p.table.reshape(1, ops.CLIQUE_WORDS)
    assert t[0, 0] == 20 and t[0, 4: 24].tolist() == list(range(20))
    only20 = ops.build_clique_plan(*_csr_of(nx.complete_graph(20)))
    assert p.table.tobytes() == only20.table.tobytes()  # the K3c record, byte for byte
    c = _col_records(p)
    assert c[0, 0] == 100 and c[0, 4: 104].tolist() == list(range(20, 120))
    assert c[0, 4 + 128: 4 + 228].tolist() == list(range(20, 120))
    assert p.clique_sources == 120 and p.clique_rows == 120


def test_barbell66_bridges_go_to_rest():
    """barbell(66, 3): each clique's 65 non-bridge rows share 66 sources (a col block); the two
    bridge rows and the three path rows are rest rows - a block above 64 attaches nothing."""
    csr = _csr_of(nx.barbell_graph(66, 3))
    cliques, rest = ops.find_cliques(*csr, max_members=128)
    assert [len(c[0]) for c in cliques] == [66, 66] and all(c[3] == [] for c in cliques)
    assert rest == [65, 66, 67, 68, 69]
    p = ops.build_clique_plan(*csr, max_members=128)
    assert (p.n_cliques, p.n_col, p.col_mmax) == (0, 2, 66) and p.rest_rows == [65, 66, 67, 68, 69]
    c = _col_records(p)
    assert c[0, 4: 70].tolist() == list(range(66)) and c[1, 4: 70].tolist() == list(range(69, 135))
    assert c[0, 4 + 128 + 65] == -1 and c[1, 4 + 128] == -1  # the bridge members have no row here
    assert int((c[:, 4 + 128:] >= 0).sum()) == 130 and p.clique_rows == 130
    assert p.rest.info.rows == 5


def test_partial_participation():
    """complete(100) with 37 aggregating members: one block of 100 sources, 37 output rows."""
    rng = np.random.default_rng(5)
    who = sorted(rng.choice(100, 37, replace=False).tolist())
    rp, col, w, _ = _csr_of(nx.complete_graph(100), rows=who)
    out = (np.arange(37) + 3).astype(np.int32)
    p = ops.build_clique_plan(rp, col, w, out, max_members=128)
    assert (p.n_cliques, p.n_col, p.col_mmax) == (0, 1, 100) and p.rest is None
    c = _col_records(p)[0]
    assert c[0] == 100 and c[4: 104].tolist() == list(range(100))
    rows = c[4 + 128:]
    assert int((rows >= 0).sum()) == 37 and np.all(rows[100:] == -1)
    assert [int(rows[i]) for i in who] == out.tolist()
    assert np.all(np.delete(rows[:100], who) == -1)


def test_spec_round_trip():
    csr = _csr_of(nx.disjoint_union(nx.complete_graph(100), nx.random_regular_graph(4, 30, seed=1)))
    p = ops.build_clique_plan(*csr, max_members=128)
    spec = {"clique": 1, "members": 128, "rest": p.rest.spec}
    q = ops.plan_from_spec(*csr, spec)
    assert q.spec == spec and q.n_col == 1 and q.col_table.tobytes() == p.col_table.tobytes()
    assert q.rest.spec == p.rest.spec and q.rest_rows == p.rest_rows
    # a spec without `members` means 64: this round then has no block at all
    with pytest.raises(ValueError):
        ops.plan_from_spec(*csr, {"clique": 1, "rest": None})
    b = _csr_of(nx.barbell_graph(60, 8))
    q64 = ops.plan_from_spec(*b, {"clique": 1, "rest": None})
    assert q64.n_col == 0 and q64.table.tobytes() == ops.build_clique_plan(*b).table.tobytes()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_tuner_candidate_and_default(bf16, mode):
    """tune_candidates offers ("clique128",) for complete(100), not for complete(40); default_plan
    takes the 128-member plan exactly where CLIQUE_COL_DEFAULT says so, and rounds whose blocks
    are all <= 64 members keep their plan."""
    big = _csr_of(nx.complete_graph(100))
    keys = [k for k, _ in ops.tune_candidates(*big, bf16=bf16, mode=mode)]
    d = ops.default_plan(*big, bf16=bf16, mode=mode)
    if ops.CLIQUE_COL_DEFAULT[bf16, mode]:
        assert isinstance(d, ops.CliquePlan) and (d.n_cliques, d.n_col, d.col_mmax) == (0, 1, 100)
        assert d.spec == {"clique": 1, "members": 128, "rest": None}
        assert ("clique128",) not in keys  # it is the default, candidate 0
    else:
        assert isinstance(d, ops.RoundPlan) and d.info.dense_rb == 0 and d.info.stream_cs == 0
        assert keys.count(("clique128",)) == 1
        xp = dict(ops.tune_candidates(*big, bf16=bf16, mode=mode))[("clique128",)]
        assert xp.n_col == 1 and xp.spec == {"clique": 1, "members": 128, "rest": None}
    small = _csr_of(nx.complete_graph(40))
    assert ("clique128",) not in [k for k, _ in ops.tune_candidates(*small, bf16=bf16, mode=mode)]
    d40 = ops.default_plan(*small, bf16=bf16, mode=mode)
    ref = ops.build_clique_plan(*small, bf16=bf16)
    assert isinstance(d40, ops.CliquePlan) and d40.n_col == 0 and d40.col_table is None
    assert d40.table.tobytes() == ref.table.tobytes() and d40.spec == {"clique": 1, "rest": None}


def test_default_table_covers_every_dtype_and_mode():
    assert set(ops.CLIQUE_COL_DEFAULT) == {(b, m) for b in (False, True) for m in MODES}
    assert all(isinstance(v, bool) for v in ops.CLIQUE_COL_DEFAULT.values())


def test_symbols_declared_exported_bound():
    L = _lib.load()
    assert L.tal_abi_version() == _lib.ABI_VERSION >= 32
    header = HDR.read_text()
    assert re.search(r"#define\s+TAL_CLIQUE_COL_MAX\s+128\b", header)
    assert re.search(r"#define\s+TAL_CLIQUE_COL_WORDS\s+260\b", header)
    assert re.search(r"#define\s+TAL_CLIQUE_WORDS\s+180\b", header)  # the K3c record is untouched
    for name, ctype in zip(NAMES, ("float", "uint16_t")):
        assert name in _lib.EXPORTED and _lib._SIGS[name] == _lib._SIGS["tal_agg_round_clique_f32"]
        assert getattr(L, name).argtypes == _lib._SIGS[name][1]
        decl = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl is not None
        assert re.sub(r"\s+", " ", decl.group(1)).strip() == (
            f"const {ctype}* pool_in, int64_t ld_in, {ctype}* pool_out, int64_t ld_out, int64_t n, "
            "const int32_t* table_dev, int32_t n_cliques, int32_t mmax, int32_t mode, void* stream")


@pytest.mark.parametrize("case,args,message", [
    ("null pool_in", (None, 64, 0x2000, 64, 64, 0x3000, 1, 100), b"null"),
    ("null pool_out", (0x1000, 64, None, 64, 64, 0x3000, 1, 100), b"null"),
    ("null table", (0x1000, 64, 0x2000, 64, 64, None, 1, 100), b"null"),
    ("in place", (0x1000, 64, 0x1000, 64, 64, 0x3000, 1, 100), b"out of place"),
    ("mmax 0", (0x1000, 64, 0x2000, 64, 64, 0x3000, 1, 0), b"mmax"),
    ("mmax 129", (0x1000, 64, 0x2000, 64, 64, 0x3000, 1, 129), b"mmax"),
    ("65536 blocks", (0x1000, 64, 0x2000, 64, 64, 0x3000, 65536, 100), b"n_cliques"),
    ("ld_in < n", (0x1000, 63, 0x2000, 64, 64, 0x3000, 1, 100), b"ld"),
])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_argument_errors(name, case, args, message, mode):
    """Each is TAL_ERR_INVALID with a message naming the entry, found before any GPU work (the
    pointers are not memory)."""
    L = _lib.load()
    pin, ld_in, pout, ld_out, n, table, n_cliques, mmax = args
    rc = getattr(L, name)(ctypes.c_void_p(pin), ld_in, ctypes.c_void_p(pout), ld_out, n, ctypes.c_void_p(table),
                          n_cliques, mmax, mode, None)
    err = L.tal_last_error()
    assert rc == _lib.TAL_ERR_INVALID, case
    assert name.encode() in err and message in err, (case, err)


@pytest.mark.parametrize("name", NAMES)
def test_odd_ld_and_element_offsets_are_not_errors(name):
    """One column per lane has no column-pair rule: an odd ld and element-aligned pools pass the
    argument checks (n = 0: accepted with nothing to launch)."""
    L = _lib.load()
    rc = getattr(L, name)(ctypes.c_void_p(0x1002), 65, ctypes.c_void_p(0x2006), 67, 0, ctypes.c_void_p(0x3000),
                          1, 128, ops.MODE_EXACT, None)
    assert rc == 0, L.tal_last_error()
