"""K3q, host side (no GPU): the sequential plan's blob (tal_seq_plan_build), its capacity and
argument errors, the three tal_agg_round_seq_* entries' argument checks on pointers that are not
memory, the ABI, and that the snapshot planner (default_plan, tune_candidates) is untouched."""
import ctypes
import re

import networkx as nx
import numpy as np
import pytest

from topology_aware_learning_amd import _lib, ops
from topology_aware_learning_amd.build import HDR
from topology_aware_learning_amd.round import csr_from_lists

ENTRIES = ("tal_agg_round_seq_f32", "tal_agg_round_seq_bf16", "tal_agg_round_seq_i64")
MODES = (ops.MODE_EXACT, ops.MODE_FMA)
HEADER = 8


def _round(g, rows=None, reverse=False):
    nodes = sorted(g.nodes) if rows is None else list(rows)
    if reverse:
        nodes = nodes[::-1]
    orders = [sorted(g.neighbors(i)) + [i] for i in nodes]
    ws = [[(0.25 + 0.5 * ((i + k) % 3)) / len(o) for k in range(len(o))] for i, o in zip(nodes, orders)]
    return orders, ws, nodes


def _rounds():
    yield "ring8", _round(nx.cycle_graph(8))
    yield "star17", _round(nx.star_graph(16))
    yield "ba33", _round(nx.barabasi_albert_graph(33, 2, seed=0))
    yield "rr64", _round(nx.random_regular_graph(8, 64, seed=1))
    yield "ring8 reversed", _round(nx.cycle_graph(8), reverse=True)
    yield "rr64 subset", _round(nx.random_regular_graph(8, 64, seed=1), rows=[i for i in range(64) if i % 3])
    yield "duplicate operand", ([[1, 2, 1, 0], [0, 1]], [[0.1, 0.2, 0.3, 0.4], [0.5, 0.5]], [0, 1])
    yield "single operands", ([[3], [0], [5]], [[1.0], [-2.0], [0.0]], [0, 3, 7])


@pytest.mark.parametrize("name,spec", list(_rounds()), ids=[n for n, _ in _rounds()])
def test_plan_decodes_to_the_csr(name, spec):
    orders, ws, out_rows = spec
    rp, col, w = csr_from_lists(orders, ws)
    p = ops.build_seq_plan(rp, col, w, np.asarray(out_rows, np.int32))
    assert isinstance(p, ops.SeqPlan) and p.spec == {"seq": 1} and p.rows == len(orders) and p.nnz == len(col)
    i, b = p.info, p.host
    assert b.dtype == np.int32 and len(b) == i.words <= _lib.load().tal_seq_plan_words(len(orders), len(col))
    srcs = sorted(set(col.tolist()))
    assert b[:HEADER].tolist() == [len(orders), len(col), len(srcs), i.words, max(max(srcs), max(out_rows)),
                                   max(len(o) for o in orders), 0, 0]
    assert (i.rows, i.nnz, i.n_src, i.max_row, i.max_ops) == tuple(b[[0, 1, 2, 4, 5]].tolist())
    # the arrays follow the header in the documented order
    offs = [HEADER, HEADER + len(srcs)]
    offs += [offs[-1] + len(orders) + 1]
    offs += [offs[-1] + len(col)]
    offs += [offs[-1] + len(col)]
    offs += [offs[-1] + len(orders)]
    assert [i.off_src_row, i.off_row_ptr, i.off_op_slot, i.off_op_w, i.off_out_row, i.off_out_slot] == offs
    assert i.words == offs[-1] + len(orders) + 8 and not b[offs[-1] + len(orders):].any()  # eight words of padding
    src_row = b[i.off_src_row: i.off_row_ptr]
    assert src_row.tolist() == srcs  # ascending, distinct: a row's slot is its index
    assert np.array_equal(b[i.off_row_ptr: i.off_op_slot], rp)
    slots = b[i.off_op_slot: i.off_op_w]
    assert np.array_equal(src_row[slots], col)  # operands in the caller's order
    assert np.array_equal(b[i.off_op_w: i.off_out_row].view(np.float32), w.astype(np.float32))
    assert b[i.off_out_row: i.off_out_slot].tolist() == list(out_rows)  # rows in the caller's order
    out_slot = b[i.off_out_slot: i.off_out_slot + len(orders)]
    for r, s in zip(out_rows, out_slot):
        assert s == (srcs.index(r) if r in srcs else -1)
    assert p.staged_rows() == len(srcs)


def _complete(m):
    orders = [[j for j in range(m) if j != i] + [i] for i in range(m)]
    return csr_from_lists(orders, [[1.0 / m] * m] * m) + (np.arange(m, dtype=np.int32),)


def test_capacity_256_sources_build_257_do_not():
    assert ops.SEQ_MAX_SRC == 256 and re.search(r"#define\s+TAL_SEQ_MAX_SRC\s+256\b", HDR.read_text())
    p = ops.build_seq_plan(*_complete(256))
    assert p.info.n_src == 256 and p.info.max_ops == 256
    with pytest.raises(_lib.TalError) as e:
        ops.build_seq_plan(*_complete(257))
    assert e.value.code == _lib.TAL_ERR_CAPACITY and "257" in str(e.value)
    # sources, not rows, are what is counted: 300 rows over 256 sources fit
    orders = [[(r + k) % 256 for k in range(3)] for r in range(300)]
    rp, col, w = csr_from_lists(orders, [[0.5, 0.25, 0.25]] * 300)
    assert ops.build_seq_plan(rp, col, w, np.arange(300, dtype=np.int32)).info.n_src == 256


def _build_raw(rows, rp, col, w, out, cap=None, null=()):
    L = _lib.load()
    P32, PD = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    arrs = dict(rp=np.asarray(rp, np.int32), col=np.asarray(col, np.int32), w=np.asarray(w, np.float64),
                out=np.asarray(out, np.int32))
    size = int(L.tal_seq_plan_words(max(rows, 0), len(arrs["col"]))) if cap is None else cap
    blob = np.zeros(max(size, 1), np.int32)
    info = _lib.SeqPlanInfo()
    arg = lambda k, t: None if k in null else arrs[k].ctypes.data_as(t)  # noqa: E731
    rc = L.tal_seq_plan_build(rows, arg("rp", P32), arg("col", P32), arg("w", PD), arg("out", P32),
                              None if "blob" in null else blob.ctypes.data_as(P32), size, ctypes.byref(info))
    return rc, info, L.tal_last_error()


@pytest.mark.parametrize("case,args,kw", [
    ("duplicate out_row", (2, [0, 2, 4], [0, 1, 1, 0], [.5, .5, .5, .5], [1, 1]), {}),
    ("empty row", (2, [0, 2, 2], [0, 1], [.5, .5], [0, 1]), {}),
    ("rows 0", (0, [0], [], [], []), {}),
    ("negative source", (1, [0, 2], [0, -1], [.5, .5], [0]), {}),
    ("negative out_row", (1, [0, 2], [0, 1], [.5, .5], [-1]), {}),
    ("null row_ptr", (1, [0, 2], [0, 1], [.5, .5], [0]), dict(null=("rp",))),
    ("null col", (1, [0, 2], [0, 1], [.5, .5], [0]), dict(null=("col",))),
    ("null w", (1, [0, 2], [0, 1], [.5, .5], [0]), dict(null=("w",))),
    ("null out_row", (1, [0, 2], [0, 1], [.5, .5], [0]), dict(null=("out",))),
])
def test_build_errors(case, args, kw):
    rc, _, err = _build_raw(*args, **kw)
    assert rc == _lib.TAL_ERR_INVALID and b"tal_seq_plan_build" in err, (case, err)


def test_small_capacity_reports_the_words_needed():
    args = (2, [0, 2, 4], [0, 1, 1, 0], [.5, .5, .5, .5], [0, 1])
    rc, info, _ = _build_raw(*args)
    assert rc == _lib.TAL_OK
    need = info.words
    assert need == HEADER + 2 + 3 + 4 + 4 + 2 + 2 + 8
    for kw in (dict(cap=need - 1), dict(cap=0), dict(null=("blob",))):
        rc, info, err = _build_raw(*args, **kw)
        assert rc == _lib.TAL_ERR_CAPACITY and info.words == need and b"tal_seq_plan_build" in err
    assert _build_raw(*args, cap=need)[0] == _lib.TAL_OK


def _info(max_row=7, n_src=8, rows=8, nnz=24):
    i = _lib.SeqPlanInfo()
    i.rows, i.nnz, i.n_src, i.max_row, i.max_ops = rows, nnz, n_src, max_row, 3
    return i


def _call(name, pool, ld, pool_rows, n, plan, info, mode=ops.MODE_EXACT):
    L = _lib.load()
    args = [ctypes.c_void_p(pool), ld, pool_rows, n, ctypes.c_void_p(plan),
            None if info is None else ctypes.byref(info)]
    if not name.endswith("_i64"):
        args.append(mode)
    args.append(None)
    return getattr(L, name)(*args), L.tal_last_error()


@pytest.mark.parametrize("case,args,message", [
    ("null pool", (None, 64, 8, 64, 0x3000, "info"), b"null pool"),
    ("null plan", (0x1000, 64, 8, 64, None, "info"), b"null plan_dev"),
    ("null info", (0x1000, 64, 8, 64, 0x3000, None), b"null info"),
    ("ld < n", (0x1000, 63, 8, 64, 0x3000, "info"), b"ld < n"),
    ("n < 0", (0x1000, 64, 8, -1, 0x3000, "info"), b"n < 0"),
    ("plan row beyond the pool", (0x1000, 64, 7, 64, 0x3000, "info"), b"pool_rows"),
])
@pytest.mark.parametrize("name", ENTRIES)
def test_entry_argument_errors(name, case, args, message):
    """Each is TAL_ERR_INVALID naming the entry and the argument, found before any GPU work (the
    pointers are not memory)."""
    pool, ld, pool_rows, n, plan, info = args
    rc, err = _call(name, pool, ld, pool_rows, n, plan, _info() if info else None)
    assert rc == _lib.TAL_ERR_INVALID, case
    assert name.encode() in err and message in err, (case, err)


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_accept_any_ld_and_element_offsets(name):
    """No alignment rule: an odd ld and an element-aligned pool pass the checks, in both modes
    (n = 0: accepted with nothing to launch)."""
    for mode in MODES:
        rc, err = _call(name, 0x1000 + 8 * 3, 67, 8, 0, 0x3000, _info(), mode)
        assert rc == _lib.TAL_OK and err == b""
        rc, err = _call(name, 0x1008, 0, 8, 0, 0x3000, _info(n_src=256), mode)
        assert rc == _lib.TAL_OK and err == b""
    rc, err = _call(name, 0x1000, 64, 8, 0, 0x3000, _info(n_src=257))
    assert rc == _lib.TAL_ERR_INVALID and b"n_src" in err


def test_symbols_declared_exported_bound():
    L = _lib.load()
    assert L.tal_abi_version() == _lib.ABI_VERSION >= 35
    header = HDR.read_text()
    for name, ctype in zip(ENTRIES, ("float", "uint16_t", "int64_t")):
        assert name in _lib.EXPORTED and getattr(L, name).argtypes == _lib._SIGS[name][1]
        decl = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl is not None
        want = (f"{ctype}* pool, int64_t ld, int64_t pool_rows, int64_t n, const int32_t* plan_dev, "
                "const tal_seq_plan_info* info, " + ("" if ctype == "int64_t" else "int32_t mode, ") + "void* stream")
        assert re.sub(r"\s+", " ", decl.group(1)).strip() == want
    for name in ("tal_seq_plan_words", "tal_seq_plan_build"):
        assert name in _lib.EXPORTED and hasattr(L, name)
    # the ctypes struct is the header's, field for field
    body = re.search(r"typedef struct tal_seq_plan_info \{(.*?)\} tal_seq_plan_info;", header, re.S).group(1)
    fields = re.findall(r"\b(int32_t|int64_t)\s+(\w+);", body)
    ctype_of = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    assert [(n, ctype_of[t]) for t, n in fields] == list(_lib.SeqPlanInfo._fields_)


def test_gate_table_covers_every_dtype_and_mode():
    assert set(ops.SEQ_DEFAULT) == {(b, m) for b in (False, True) for m in MODES}
    assert all(isinstance(v, bool) for v in ops.SEQ_DEFAULT.values())


def _unweighted(g):
    orders = [sorted(g.neighbors(i)) + [i] for i in sorted(g.nodes)]
    return csr_from_lists(orders, [[1.0 / len(o)] * len(o) for o in orders]) + (
        np.arange(len(orders), dtype=np.int32),)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_snapshot_planner_untouched(bf16, mode):
    """default_plan and tune_candidates return what they returned before the sequential plan
    existed: ring 32 the narrow regular plan build_plan finds, complete 100 the one-block K3c1
    plan build_clique_plan(max_members=128) builds - spec and blob bytes - and no candidate is a
    sequential plan."""
    ring = _unweighted(nx.cycle_graph(32))
    d = ops.default_plan(*ring, bf16=bf16, mode=mode)
    want = ops.build_plan(*ring)
    assert isinstance(d, ops.RoundPlan) and d.spec == want.spec and d.host.tobytes() == want.host.tobytes()
    comp = _unweighted(nx.complete_graph(100))
    d = ops.default_plan(*comp, bf16=bf16, mode=mode)
    want = ops.build_clique_plan(*comp, bf16=bf16, max_members=128)
    assert isinstance(d, ops.CliquePlan) and d.spec == want.make_spec() and d.spec.get("members") == 128
    assert d.col_table.tobytes() == want.col_table.tobytes() and d.table.tobytes() == want.table.tobytes()
    assert (d.rest is None) and (want.rest is None)
    for csr in (ring, comp):
        cands = ops.tune_candidates(*csr, bf16=bf16, mode=mode)
        assert cands and not any(isinstance(c, ops.SeqPlan) or (c.spec or {}).get("seq") for _, c in cands)
