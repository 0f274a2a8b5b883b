"""K3c on bf16 pools, host side (no GPU): the C-ABI entry tal_agg_round_clique_bf16 - declared,
exported, bound, its argument errors reported before any GPU work - and the plan logic that
routes bf16 rounds to it (default_plan per mode, tune_candidates, plan_from_spec, the rest plan's
form), with the fp32 plans unchanged."""
import ctypes
import re

import networkx as nx
import numpy as np
import pytest

import bench
from topology_aware_learning_amd import _lib, ops
from topology_aware_learning_amd.build import HDR
from topology_aware_learning_amd.round import csr_from_lists

NAME = "tal_agg_round_clique_bf16"

# default_plan(bf16=True) per mode, as measured on MI355X (ops.default_plan's docstring, DESIGN §4
# "K3c on bf16 pools"): the clique plan where it beat the sparse form by more than the tuner's margin
# on config 4 and was not slower on the complete graph of 64
CLIQUE_IS_DEFAULT = {ops.MODE_EXACT: True, ops.MODE_FMA: True}


def test_symbol_declared_exported_bound():
    L = _lib.load()
    assert L.tal_abi_version() == _lib.ABI_VERSION >= 30
    assert NAME in _lib.EXPORTED and NAME in _lib._SIGS
    assert _lib._SIGS[NAME] == _lib._SIGS["tal_agg_round_clique_f32"]
    assert getattr(L, NAME).argtypes == _lib._SIGS[NAME][1]
    header = HDR.read_text()
    decl = re.search(r"int32_t\s+" + NAME + r"\s*\(([^)]*)\)\s*;", header)
    assert decl is not None
    assert re.sub(r"\s+", " ", decl.group(1)).strip() == (
        "const uint16_t* pool_in, int64_t ld_in, uint16_t* pool_out, int64_t ld_out, int64_t n, "
        "const int32_t* table_dev, int32_t n_cliques, int32_t mmax, int32_t mode, void* stream")


@pytest.mark.parametrize("case,args,message", [
    ("null pool_in", (None, 64, 0x2000, 64, 64, 0x3000, 1, 16), b"null"),
    ("null pool_out", (0x1000, 64, None, 64, 64, 0x3000, 1, 16), b"null"),
    ("in place", (0x1000, 64, 0x1000, 64, 64, 0x3000, 1, 16), b"out of place"),
    ("mmax 0", (0x1000, 64, 0x2000, 64, 64, 0x3000, 1, 0), b"mmax"),
    ("mmax 65", (0x1000, 64, 0x2000, 64, 64, 0x3000, 1, 65), b"mmax"),
    ("odd ld_in", (0x1000, 65, 0x2000, 64, 64, 0x3000, 1, 16), b"aligned"),
    ("odd ld_out", (0x1000, 64, 0x2000, 65, 64, 0x3000, 1, 16), b"aligned"),
    ("pool_in at a 2-byte offset", (0x1002, 64, 0x2000, 64, 64, 0x3000, 1, 16), b"aligned"),
    ("pool_out at a 2-byte offset", (0x1000, 64, 0x2002, 64, 64, 0x3000, 1, 16), b"aligned"),
])
@pytest.mark.parametrize("mode", [ops.MODE_EXACT, ops.MODE_FMA])
def test_argument_errors(case, args, message, mode):
    """Each is TAL_ERR_INVALID with a message naming the entry, found before any GPU work (the
    pointers are not memory)."""
    L = _lib.load()
    pin, ld_in, pout, ld_out, n, table, n_cliques, mmax = args
    rc = getattr(L, NAME)(ctypes.c_void_p(pin), ld_in, ctypes.c_void_p(pout), ld_out, n, ctypes.c_void_p(table),
                          n_cliques, mmax, mode, None)
    err = L.tal_last_error()
    assert rc == _lib.TAL_ERR_INVALID, case
    assert NAME.encode() in err and message in err, (case, err)


def _rounds():
    orders, ws = bench.round_spec(128, 0, kind="barbell")
    yield "barbell", orders, ws, 2
    g = nx.complete_graph(64)
    orders = [sorted(g.neighbors(i)) + [i] for i in range(64)]
    yield "complete64", orders, [[1.0 / 64] * 64 for _ in orders], 1


@pytest.mark.parametrize("name,orders,ws,n_cliques", list(_rounds()), ids=["barbell", "complete64"])
def test_plan_logic(name, orders, ws, n_cliques):
    """Config 4's round and `unweighted_fl` over 64 clients on bf16: default_plan takes the clique
    plan in both modes (medians of 20 interleaved runs on MI355X, profiles/r12: config 4 7.38 ms
    against 19.05 for the sparse form in EXACT mode, 6.11 against 8.48 in FMA mode; complete 64
    0.869 against 5.23 and 0.729 against 2.26), the tuner offers it, its spec rebuilds it, its
    rest plan is a form tal_agg_round_bf16 takes, and the fp32 plan of the round is unchanged."""
    rp, col, w = csr_from_lists(orders, ws)
    rows = np.arange(len(orders), dtype=np.int32)
    fp32 = ops.build_clique_plan(rp, col, w, rows)
    assert fp32 is not None and fp32.n_cliques == n_cliques
    for mode in (ops.MODE_EXACT, ops.MODE_FMA):
        p = ops.default_plan(rp, col, w, rows, bf16=True, mode=mode)
        if CLIQUE_IS_DEFAULT[mode]:
            assert isinstance(p, ops.CliquePlan) and p.n_cliques == n_cliques and p.spec["clique"] == 1
        else:  # today's form: the sparse plan
            assert isinstance(p, ops.RoundPlan) and p.info.dense_rb == 0 and p.info.stream_cs == 0
        cands = ops.tune_candidates(rp, col, w, rows, bf16=True, mode=mode)
        cliques = [c for _, c in cands if isinstance(c, ops.CliquePlan)]
        assert len(cliques) == 1 and cliques[0].spec["clique"] == 1
        for cp in cliques + [ops.plan_from_spec(rp, col, w, rows, {"clique": 1}),
                             ops.build_clique_plan(rp, col, w, rows, bf16=True)]:
            assert np.array_equal(cp.table, fp32.table) and cp.mmax == fp32.mmax
            assert (cp.rest is None) == (name == "complete64")
            if cp.rest is not None:  # a form tal_agg_round_bf16 takes
                assert isinstance(cp.rest, ops.RoundPlan) and cp.rest.info.dense_rb == 0 and cp.rest.info.stream_cs == 0
            assert cp.full.info.dense_rb == 0 and cp.full.info.stream_cs == 0
        # the fp32 default of the same round is still build_clique_plan's plan
        for kw in (dict(), dict(mode=mode), dict(bf16=False, mode=mode)):
            q = ops.default_plan(rp, col, w, rows, **kw)
            assert isinstance(q, ops.CliquePlan)
            assert q.table.tobytes() == fp32.table.tobytes() and (q.n_cliques, q.mmax) == (fp32.n_cliques, fp32.mmax)
            assert (q.rest.spec if q.rest is not None else None) == (fp32.rest.spec if fp32.rest is not None else None)
            assert q.spec == dict(clique=1, rest=fp32.rest.spec if fp32.rest is not None else None)


def test_bf16_rest_plan_must_be_sparse_or_narrow():
    """A rest spec asking for a form tal_agg_round_bf16 refuses (dense row blocks) is an error for a
    bf16 clique plan; the fp32 plan takes it as before."""
    orders, ws = bench.round_spec(128, 0, kind="barbell")
    rp, col, w = csr_from_lists(orders, ws)
    rows = np.arange(len(orders), dtype=np.int32)
    spec = {"c4": 64, "lds": ops.LDS_BUDGETS[-1], "dense": 8}
    p = ops.build_clique_plan(rp, col, w, rows, rest_spec=spec)
    assert p.rest.info.dense_rb != 0
    with pytest.raises(ValueError):
        ops.build_clique_plan(rp, col, w, rows, rest_spec=spec, bf16=True)
