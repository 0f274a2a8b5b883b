"""K3ms on the host (tal_agg.h): the plan's classes and rest decode back to the CSR; the ABI entry's errors."""
import ctypes

import networkx as nx
import numpy as np
import pytest

import _matrix as mx
from topology_aware_learning_amd import _lib, ops

CASES = ("complete33", "per_source", "barbell", "outside")


def case(name):
    """(row_ptr, col, w, out_row, pool rows, the classes' row indices, the rest's)."""
    if name == "complete33":
        rp, col, w = mx.round_csr("complete33", "unweighted")
        return rp, col, w, np.arange(33, dtype=np.int32), 33, [list(range(33))], []
    if name == "per_source":  # one weight per SOURCE shared by all rows: signed, zeros among them, sum |w| <= 1
        rp, col, _ = mx.round_csr("complete_chunk+1", "unweighted")
        m = len(rp) - 1
        ws = np.random.default_rng(7).standard_normal(m)
        ws[::7] = 0.0
        ws /= np.abs(ws).sum() * (1 + 2.0 ** -20)
        return rp, col, ws[col], np.arange(m, dtype=np.int32), m, [list(range(m))], []
    if name == "barbell":  # two cliques of 12 whose node 11 / 14 also lists the path 12 - 13
        g = nx.barbell_graph(12, 2)
        orders = [sorted(g.neighbors(i)) + [i] for i in range(26)]
        rp = np.cumsum([0] + [len(o) for o in orders]).astype(np.int32)
        w = np.concatenate([[1.0 / len(o)] * len(o) for o in orders])
        return (rp, np.concatenate(orders).astype(np.int32), w, np.arange(26, dtype=np.int32), 26,
                [list(range(11)), list(range(15, 26))], [11, 12, 13, 14])
    # a permuted out_row into 40 pool rows; rows 0..5: sources 30..37, rotated; 6 and 8: source 2 twice; 7: one weight off
    orders = [list(np.roll(np.arange(30, 38), r)) for r in range(6)] + [[2, 31, 2], [2, 2, 31], [2, 2, 31]]
    ws = [[(1 + (s - 30)) / 64 for s in o] for o in orders[:6]] + [[0.25, 0.5, 0.25], [0.25, 0.125, 0.5], [0.25, 0.25, 0.5]]
    rp = np.cumsum([0] + [len(o) for o in orders]).astype(np.int32)
    out_row = np.random.default_rng(5).permutation(40)[:9].astype(np.int32)
    return rp, np.concatenate(orders).astype(np.int32), np.concatenate(ws), out_row, 40, [list(range(6)), [6, 8]], [7]


def _key(col, w):
    return sorted(zip(col.tolist(), np.asarray(w, np.float32).view(np.uint32).tolist()))


@pytest.mark.parametrize("name", CASES)
def test_classes_and_rest_decode_to_the_csr(name):
    rp, col, w, out_row, pool_rows, classes, rest = case(name)
    plan = ops.build_matrix_plan(rp, col, w, out_row, shared=True)
    assert isinstance(plan, ops.SharedPlan) and plan.spec == {"matrix": 1, "shared": 1} and not plan.single_group
    i, h = plan.info, plan.host
    assert plan.class_index == classes and plan.rest_index == rest and i.n_classes == len(classes)
    assert i.words == len(h) and i.off_src % 2 == 0 and i.max_row == max(col.max(), out_row.max()) < pool_rows
    cls = h[i.off_cls: i.off_cls + 4 * i.n_classes].reshape(-1, 4)
    src = h[i.off_src: i.off_src + 2 * i.n_src].reshape(-1, 2)
    outs, m_rp = h[i.off_out_row: i.off_out_row + i.n_out], h[i.off_row_ptr: i.off_row_ptr + i.n_out + 1]
    for (s0, ns, m0, nm), rows in zip(cls, classes):
        rec = list(zip(src[s0: s0 + ns, 0].tolist(), src[s0: s0 + ns, 1].view(np.uint32).tolist()))
        assert rec == sorted(rec) and nm == len(rows) and np.array_equal(outs[m0: m0 + nm], out_row[rows])
        for m, r in zip(range(m0, m0 + nm), rows):  # the class is the row's multiset; the member CSR is the row
            a, b, qa, qb = rp[r], rp[r + 1], m_rp[m], m_rp[m + 1]
            assert rec == _key(col[a:b], w[a:b])
            assert np.array_equal(h[i.off_col + qa: i.off_col + qb], col[a:b])
            assert np.array_equal(h[i.off_w + qa: i.off_w + qb].view(np.float32), w[a:b].astype(np.float32))
    assert i.n_src == cls[:, 1].sum() and i.n_out == cls[:, 3].sum() and i.max_src == cls[:, 1].max()
    keys = [_key(col[rp[r]: rp[r + 1]], w[rp[r]: rp[r + 1]]) for r in rest]
    assert all(keys.count(k) == 1 for k in keys)  # no two rest rows share their operands
    assert (plan.rest is None) == (not rest)
    if rest:
        ri = plan.rest.info
        assert sorted(plan.rest.host[ri.off_out_row: ri.off_out_row + ri.rows]) == sorted(out_row[rest])
        assert plan.staged_rows() == i.n_src + plan.rest.staged_rows()


def test_no_class_gives_the_matrix_plan():
    rp, col, w = mx.round_csr("ring8", "unweighted")
    out_row = np.arange(8, dtype=np.int32)
    a, b = (ops.build_matrix_plan(rp, col, w, out_row, shared=s) for s in (True, False))
    assert type(a) is type(b) is ops.MatrixPlan and np.array_equal(a.host, b.host) and a.spec == {"matrix": 1}
    assert type(ops.default_plan(rp, col, w, out_row, bf16=True, mode=ops.MODE_MATRIX, shared=True)) is ops.MatrixPlan
    with pytest.raises(ValueError, match="MODE_MATRIX"):
        ops.default_plan(rp, col, w, out_row, bf16=True, mode=ops.MODE_FMA, shared=True)


@pytest.mark.parametrize("bump,kind", [(0.0, ops.SharedPlan), (1.0, ops.MatrixPlan), (np.inf, ops.MatrixPlan)])
def test_a_repeated_source_counts_twice_and_one_ulp_separates(bump, kind):
    """[3, 3, 5] and [5, 3, 3]: one class; not with a weight one fp32 ulp apart or a non-finite one in both."""
    w = np.array([0.25, 0.5, 0.125, 0.125, 0.5, 0.25])
    if bump == 1.0:
        w[4] = np.nextafter(np.float32(0.5), np.float32(1.0))
    elif bump:
        w[[2, 3]] = bump
    plan = ops.build_matrix_plan([0, 3, 6], [3, 3, 5, 5, 3, 3], w, [0, 1], shared=True)
    assert type(plan) is kind
    assert bump or plan.host[plan.info.off_src:][:6].tolist() == [3, 0x3E800000, 3, 0x3F000000, 5, 0x3E000000]


def test_abi_38_entry_and_argument_errors():
    L = _lib.load()
    assert L.tal_abi_version() == _lib.ABI_VERSION == 38 and "tal_agg_round_shared_bf16" in _lib.EXPORTED
    rp, col, w, out_row, pool_rows = case("barbell")[:5]
    info = ops.build_matrix_plan(rp, col, w, out_row, shared=True).info
    a, b, t, f = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000), L.tal_agg_round_shared_bf16
    ok = dict(pin=a, ld_in=64, pout=b, ld_out=64, rows=pool_rows, n=64, table=t, info=ctypes.byref(info))
    for change, word in ((dict(pin=None), b"null"), (dict(pout=None), b"null"), (dict(table=None), b"null"),
                         (dict(info=None), b"null"), (dict(pout=a), b"pool_out == pool_in"), (dict(n=-1), b"n < 0"),
                         (dict(ld_in=63), b"ld < n"), (dict(ld_out=63), b"ld < n"), (dict(rows=25), b"pool_rows"),
                         (dict(table=ctypes.c_void_p(0x3004)), b"aligned"),
                         (dict(info=ctypes.byref(_lib.SharedPlanInfo())), b"not a shared plan")):
        assert f(*{**ok, **change}.values(), None) == _lib.TAL_ERR_INVALID and word in L.tal_last_error(), change
    assert f(*{**ok, "n": 0}.values(), None) == _lib.TAL_OK  # nothing to do: no launch
