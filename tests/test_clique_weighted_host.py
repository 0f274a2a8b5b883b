"""K3c with per-source weights, host side (no GPU): the C-ABI entries tal_agg_round_clique_w_f32 /
_bf16 - declared, exported, bound, their argument errors reported before any launch - and the
plan logic: per-source block detection on the weighted and centrality apps' barbell rounds, the
weight table (every entry the fp32 cast of the CSR weight it stands for, 1.0 elsewhere, each block
decoded back to its CSR rows), the rows detection must leave out, the `wclique` spec, and the
uniform-weight plans unchanged."""
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

NAMES = {"tal_agg_round_clique_w_f32": "float", "tal_agg_round_clique_w_bf16": "uint16_t"}
M, XW = ops.CLIQUE_MAX, ops.CLIQUE_MAX + 3


def test_symbols_declared_exported_bound():
    L = _lib.load()
    assert L.tal_abi_version() == _lib.ABI_VERSION >= 31
    header = HDR.read_text()
    assert re.search(r"#define\s+TAL_CLIQUE_WWORDS\s+332\b", header) and ops.CLIQUE_WWORDS == 332
    for name, ctype in NAMES.items():
        assert name in _lib.EXPORTED and name in _lib._SIGS and hasattr(L, name)
        uniform = _lib._SIGS[name.replace("_w_", "_")]
        assert _lib._SIGS[name] == (uniform[0], uniform[1] + [ctypes.c_void_p])
        assert getattr(L, name).argtypes == _lib._SIGS[name][1]
        decl = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl is not None
        assert re.sub(r"\s+", " ", decl.group(1)).strip() == (
            f"const {ctype}* pool_in, int64_t ld_in, {ctype}* pool_out, int64_t ld_out, int64_t n, "
            "const int32_t* table_dev, int32_t n_cliques, int32_t mmax, int32_t mode, void* stream, "
            "const float* wtab_dev")


@pytest.mark.parametrize("case,args,message", [
    ("null wtab_dev", (0x1000, 64, 0x2000, 64, 64, 0x3000, 1, 16, None), b"null"),
    ("null pool_in", (None, 64, 0x2000, 64, 64, 0x3000, 1, 16, 0x4000), b"null"),
    ("null table", (0x1000, 64, 0x2000, 64, 64, None, 1, 16, 0x4000), b"null"),
    ("in place", (0x1000, 64, 0x1000, 64, 64, 0x3000, 1, 16, 0x4000), b"out of place"),
    ("mmax 65", (0x1000, 64, 0x2000, 64, 64, 0x3000, 1, 65, 0x4000), b"mmax"),
    ("odd ld_in", (0x1000, 65, 0x2000, 64, 64, 0x3000, 1, 16, 0x4000), b"aligned"),
    ("odd ld_out", (0x1000, 64, 0x2000, 65, 64, 0x3000, 1, 16, 0x4000), b"aligned"),
    ("pool_in at a 2-byte offset", (0x1002, 64, 0x2000, 64, 64, 0x3000, 1, 16, 0x4000), b"aligned"),
    ("pool_out at a 2-byte offset", (0x1000, 64, 0x2002, 64, 64, 0x3000, 1, 16, 0x4000), b"aligned"),
])
@pytest.mark.parametrize("name", list(NAMES))
@pytest.mark.parametrize("mode", [ops.MODE_EXACT, ops.MODE_FMA])
def test_argument_errors(case, args, message, name, mode):
    """Each is TAL_ERR_INVALID with a message naming the entry, found before any launch (the
    pointers are not memory)."""
    L = _lib.load()
    pin, ld_in, pout, ld_out, n, table, n_cliques, mmax, wtab = args
    rc = getattr(L, name)(ctypes.c_void_p(pin), ld_in, ctypes.c_void_p(pout), ld_out, n, ctypes.c_void_p(table),
                          n_cliques, mmax, mode, None, ctypes.c_void_p(wtab))
    err = L.tal_last_error()
    assert rc == _lib.TAL_ERR_INVALID, case
    assert name.encode() in err and message in err, (case, err)


def _orders(g):
    return [sorted(g.neighbors(i)) + [i] for i in sorted(g.nodes)]


def _weights(kind, g, orders):
    if kind == "datasize":  # weighted_module_avg over seeded training-set lengths
        lens = np.random.default_rng(11).integers(100, 5000, g.number_of_nodes()).tolist()
        return [tw.weighted([lens[j] for j in o]) for o in orders]
    cent = nx.degree_centrality(g)
    return [tw.centrality(o, cent, kind == "degcent_softmax", 10.0) for o in orders]


def _csr(orders, ws):
    rp, col, w = csr_from_lists(orders, ws)
    return rp, col, w, np.arange(len(orders), dtype=np.int32)


def _decode(plan):
    """{out_row: (operands in the kernel's order, their fp32 weights)} of a per-source clique plan's
    blocks, read from the two tables alone (tal_agg.h)."""
    t = plan.table.reshape(plan.n_cliques, ops.CLIQUE_WORDS)
    wt = plan.wtable.reshape(plan.n_cliques, ops.CLIQUE_WWORDS)
    rows = {}
    for k in range(plan.n_cliques):
        m, n_att = int(t[k, 0]), int(t[k, 2])
        src, out = t[k, 4: 4 + M], t[k, 4 + M: 4 + 2 * M]
        for i in range(m):
            if out[i] >= 0:
                order = [j for j in range(m) if j != i] + [i]
                rows[int(out[i])] = ([int(src[j]) for j in order], [wt[k, j] for j in order])
        for q in range(n_att):
            rec = t[k, 4 + 2 * M + q * ops.CLIQUE_EXTRA_WORDS:][: ops.CLIQUE_EXTRA_WORDS]
            xw = wt[k, M + q * XW:][:XW]
            mask = (int(rec[2]) & 0xFFFFFFFF) | ((int(rec[3]) & 0xFFFFFFFF) << 32)
            ops_, ws = [], []
            for j in range(M + 1):
                for e in range(int(rec[6])):
                    if rec[9 + e] == j:
                        ops_.append(int(rec[7 + e])), ws.append(xw[M + e])
                if j < M and (mask >> j) & 1:
                    ops_.append(int(src[j])), ws.append(xw[j])
            ops_.append(int(src[rec[4]]) if rec[4] >= 0 else int(rec[5])), ws.append(xw[M + 2])
            rows[int(rec[0])] = (ops_, ws)
    return rows


def _used_weight_slots(plan):
    """Boolean [n_cliques, CLIQUE_WWORDS]: the weight slots a kernel multiplies a real operand by."""
    t = plan.table.reshape(plan.n_cliques, ops.CLIQUE_WORDS)
    used = np.zeros((plan.n_cliques, ops.CLIQUE_WWORDS), bool)
    for k in range(plan.n_cliques):
        used[k, : t[k, 0]] = True
        for q in range(int(t[k, 2])):
            rec = t[k, 4 + 2 * M + q * ops.CLIQUE_EXTRA_WORDS:][: ops.CLIQUE_EXTRA_WORDS]
            mask = (int(rec[2]) & 0xFFFFFFFF) | ((int(rec[3]) & 0xFFFFFFFF) << 32)
            base = M + q * XW
            used[k, base: base + M] = [(mask >> j) & 1 for j in range(M)]
            used[k, base + M: base + M + int(rec[6])] = True
            used[k, base + M + 2] = True
    return used


@pytest.mark.parametrize("kind", ["datasize", "degcent_softmax", "degcent_normalised"])
@pytest.mark.parametrize("m1,m2", [(60, 8), (12, 4)])
def test_detection_on_barbells(m1, m2, kind):
    """barbell(m1, m2) under the weighted / centrality apps: two blocks, one per clique, every member
    but the bridge with a row, the bridge rows attached with their own weights, the path rows in
    `rest`; the tables decode back to exactly the CSR rows, fp32 weight bits included; the uniform
    detection finds nothing on these rounds."""
    g = nx.barbell_graph(m1, m2)
    orders = _orders(g)
    rp, col, w, out = _csr(orders, _weights(kind, g, orders))
    assert ops.find_cliques(rp, col, w, out)[0] == []
    cliques, rest = ops.find_cliques(rp, col, w, out, per_source=True)
    assert len(cliques) == 2
    bridges = {m1 - 1, m1 + m2}
    for srcs, w32, outs, att in cliques:
        assert len(srcs) == m1 and len(outs) == m1 - 1 and w32.dtype == np.float32 and len(w32) == m1
        assert len(att) == 1 and att[0]["out"] in bridges and len(att[0]["ext"]) == 1
        assert not bridges.intersection(outs.values())
    assert sorted(rest) == list(range(m1, m1 + m2))  # the path
    plan = ops.build_clique_plan(rp, col, w, out, per_source=True)
    assert plan.n_cliques == 2 and plan.mmax == m1 and plan.clique_rows == 2 * m1
    assert plan.wtable.dtype == np.float32 and plan.wtable.size == 2 * ops.CLIQUE_WWORDS
    assert plan.rest is not None and plan.rest.rows == m2 and plan.full.rows == len(orders)
    assert plan.staged_rows() == 2 * m1 + 2 + plan.rest.staged_rows()
    t = plan.table.reshape(2, ops.CLIQUE_WORDS)
    assert not t[:, 1].any() and not t[:, 4 + 2 * M + 1].any()  # the uniform weight words: unused
    decoded = _decode(plan)
    assert sorted(decoded) == [r for r in range(len(orders)) if r not in rest]
    for r, (ops_, ws) in decoded.items():
        assert ops_ == list(col[rp[r]: rp[r + 1]]), r
        want = w[rp[r]: rp[r + 1]].astype(np.float32)
        assert np.array_equal(np.array(ws, np.float32).view(np.uint32), want.view(np.uint32)), r
    unused = ~_used_weight_slots(plan)
    assert np.all(plan.wtable.reshape(2, -1)[unused] == np.float32(1.0)) and unused.sum() > 0
    if kind != "datasize":  # two distinct weights per block: the bridge's and everyone else's
        assert all(len(set(c[1].view(np.uint32).tolist())) == 2 for c in cliques)
    else:
        assert all(len(set(c[1].view(np.uint32).tolist())) > m1 // 2 for c in cliques)


def _complete(m):
    g = nx.complete_graph(m)
    orders = _orders(g)
    lens = np.random.default_rng(m).integers(100, 5000, m).tolist()
    return orders, [tw.weighted([lens[j] for j in o]) for o in orders]


def test_rows_left_out():
    """One ulp of difference in one source's weight, a sign-flipped (`*_sim`-style) row, self not
    last and a non-finite weight each keep that row out of the block (and out of its attached
    rows when it is not in reference order); the other rows still form it."""
    m = 20
    orders, ws = _complete(m)
    ulp = [list(x) for x in ws]
    w32 = np.float32(ulp[3][5])
    ulp[3][5] = float(np.nextafter(w32, np.float32(2.0)))
    flipped = [list(x) for x in ws]
    flipped[4] = [-x for x in flipped[4]]
    nonfinite = [list(x) for x in ws]
    nonfinite[6][2] = float("inf")
    for bad, wsx in ((3, ulp), (4, flipped), (6, nonfinite)):
        rp, col, w, out = _csr(orders, wsx)
        cliques, rest = ops.find_cliques(rp, col, w, out, per_source=True)
        assert len(cliques) == 1 and sorted(cliques[0][2].values()) == [r for r in range(m) if r != bad]
        att = cliques[0][3]
        if bad == 6:  # a non-finite weight is in no block at all
            assert att == [] and rest == [bad]
        else:  # in reference order with finite weights of its own: attached, with those weights
            assert [a["out"] for a in att] == [bad] and rest == []
            plan = ops.build_clique_plan(rp, col, w, out, per_source=True)
            ops_, wts = _decode(plan)[bad]
            assert ops_ == orders[bad]
            assert np.array_equal(np.array(wts, np.float32), np.array(wsx[bad], np.float32))
    shuffled = [list(o) for o in orders]
    shuffled[7] = shuffled[7][-1:] + shuffled[7][:-1]  # self first
    wsh = [list(x) for x in ws]
    wsh[7] = wsh[7][-1:] + wsh[7][:-1]
    rp, col, w, out = _csr(shuffled, wsh)
    cliques, rest = ops.find_cliques(rp, col, w, out, per_source=True)
    assert len(cliques) == 1 and 7 not in cliques[0][2].values() and cliques[0][3] == [] and rest == [7]


def test_block_size_limits():
    """Fewer than CLIQUE_MIN_ROWS rows or more than 64 sources: no block."""
    orders, ws = _complete(ops.CLIQUE_MIN_ROWS - 1)
    assert ops.find_cliques(*_csr(orders, ws), per_source=True)[0] == []
    assert ops.build_clique_plan(*_csr(orders, ws), per_source=True) is None
    orders, ws = _complete(ops.CLIQUE_MIN_ROWS)
    assert len(ops.find_cliques(*_csr(orders, ws), per_source=True)[0]) == 1
    orders, ws = _complete(64)
    assert len(ops.find_cliques(*_csr(orders, ws), per_source=True)[0]) == 1
    orders, ws = _complete(65)
    assert ops.find_cliques(*_csr(orders, ws), per_source=True)[0] == []
    # 20 rows over the same 20 sources but only 7 with one set of weights: no block of 7
    orders, ws = _complete(20)
    for r in range(7, 20):
        ws[r] = [x * (1.0 + (r + 1) * 2.0 ** -10) for x in ws[r]]
    assert ops.find_cliques(*_csr(orders, ws), per_source=True)[0] == []


@pytest.mark.parametrize("kind,n,deg", [("ring", 32, 2), ("random", 64, 8), ("barbell", 128, 0), ("sbm", 256, 0)])
def test_unweighted_rounds_unchanged(kind, n, deg):
    """The unweighted rounds of test_default_plan_forms: default_plan and build_clique_plan() give
    the default call's tables, with no weight table; the per-source flag changes nothing for a
    caller that does not pass it."""
    orders, ws = bench.round_spec(n, deg, kind=kind)
    rp, col, w, out = _csr(orders, ws)
    base = ops.build_clique_plan(rp, col, w, out)
    assert ops.find_cliques(rp, col, w, out) == ops.find_cliques(rp, col, w, out, per_source=False)
    for bf16 in (False, True):
        for mode in (ops.MODE_EXACT, ops.MODE_FMA):
            p = ops.default_plan(rp, col, w, out, bf16=bf16, mode=mode)
            if base is None:
                assert not isinstance(p, ops.CliquePlan)
                continue
            assert isinstance(p, ops.CliquePlan) and p.wtable is None and p.spec_key == "clique"
            assert p.table.tobytes() == base.table.tobytes() and p.spec["clique"] == 1 and "wclique" not in p.spec
    if base is not None:
        assert base.wtable is None
        t = base.table.reshape(base.n_cliques, ops.CLIQUE_WORDS)
        assert (t[:, 1].view(np.float32) == np.float32(1 / 60)).all()
        # the tuner does not offer per-source blocks that cover no more rows than the uniform ones
        assert not any(c.wtable is not None for _, c in ops.tune_candidates(rp, col, w, out) if isinstance(c, ops.CliquePlan))


def test_spec_round_trip_and_candidates():
    """{"wclique": 1} rebuilds the per-source plan (rest spec included); {"clique": 1} still means
    the uniform form and is a ValueError on a round without uniform blocks; the tuner offers the
    weighted plan on such a round, bf16 rest rows keep the sparse / narrow restriction."""
    orders, ws = bench.round_spec(128, 0, kind="barbell", weights="degcent")
    rp, col, w, out = _csr(orders, ws)
    p = ops.build_clique_plan(rp, col, w, out, per_source=True)
    q = ops.plan_from_spec(rp, col, w, out, {"wclique": 1})
    assert q.wtable is not None and q.table.tobytes() == p.table.tobytes() and q.wtable.tobytes() == p.wtable.tobytes()
    assert q.spec == {"wclique": 1} and q.spec_key == "wclique"
    q = ops.plan_from_spec(rp, col, w, out, {"wclique": 1, "rest": p.rest.spec})
    assert q.rest.spec == p.rest.spec and q.wtable.tobytes() == p.wtable.tobytes()
    with pytest.raises(ValueError):
        ops.plan_from_spec(rp, col, w, out, {"clique": 1})
    for bf16 in (False, True):
        for mode in (ops.MODE_EXACT, ops.MODE_FMA):
            cands = ops.tune_candidates(rp, col, w, out, bf16=bf16, mode=mode)
            wc = [c for _, c in cands if isinstance(c, ops.CliquePlan)]
            assert len(wc) == 1 and wc[0].wtable is not None and wc[0].spec["wclique"] == 1
            assert wc[0].rest.info.dense_rb == 0 and wc[0].rest.info.stream_cs == 0
            d = ops.default_plan(rp, col, w, out, bf16=bf16, mode=mode)
            assert isinstance(d, ops.CliquePlan) == ops.WCLIQUE_DEFAULT[bf16, mode]
    spec = {"c4": 64, "lds": ops.LDS_BUDGETS[-1], "dense": 8}
    assert ops.build_clique_plan(rp, col, w, out, rest_spec=spec, per_source=True).rest.info.dense_rb != 0
    with pytest.raises(ValueError):
        ops.build_clique_plan(rp, col, w, out, rest_spec=spec, bf16=True, per_source=True)
