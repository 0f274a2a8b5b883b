"""K3c2, host side (no GPU): clique blocks of 129..256 members (two lanes per column,
tal_agg_round_clique_half_*): what `max_members=256` admits, CliquePlan.half_table, nothing changed
below it, the spec, the tuner's opt-in candidate, the ABI and the entries' argument errors."""
import ctypes
import re

import networkx as nx
import numpy as np
import pytest

from topology_aware_learning_amd import _lib, ops
from topology_aware_learning_amd.build import HDR
from topology_aware_learning_amd.round import csr_from_lists

NAMES = ("tal_agg_round_clique_half_f32", "tal_agg_round_clique_half_bf16")


def _csr_of(g):
    orders = [sorted(g.neighbors(i)) + [i] for i in sorted(g.nodes)]
    rp, col, w = csr_from_lists(orders, [[1.0 / len(o)] * len(o) for o in orders])
    return rp, col, w, np.arange(len(orders), dtype=np.int32)


@pytest.mark.parametrize("m", [129, 200, 256])
def test_record_decodes_to_the_csr(m):
    rp, col, w, out = csr = _csr_of(nx.complete_graph(m))
    p = ops.build_clique_plan(*csr, max_members=256)
    assert (p.n_cliques, p.n_col, p.n_half, p.half_mmax) == (0, 0, 1, m) and p.rest is None and p.rest_rows == []
    assert p.table.size == 0 and p.col_table is None and p.half_table.dtype == np.int32
    rec = p.half_table.reshape(1, ops.CLIQUE_HALF_WORDS)[0]
    srcs, outs = rec[4: 4 + 256], rec[4 + 256:]
    assert rec[0] == m and rec[2] == rec[3] == 0 and np.all(srcs[m:] == 0) and np.all(outs[m:] == -1)
    wbits = np.array([1.0 / m], np.float64).astype(np.float32).view(np.int32)[0]
    assert rec[1] == wbits
    for i in range(m):  # member i's row: every other member ascending, then itself, all under w
        r = int(np.flatnonzero(out == outs[i])[0])
        want = [int(s) for k, s in enumerate(srcs[:m]) if k != i] + [int(srcs[i])]
        assert col[rp[r]: rp[r + 1]].tolist() == want
        assert np.all(w[rp[r]: rp[r + 1]].astype(np.float32).view(np.int32) == wbits)
    assert (p.clique_sources, p.clique_rows, p.staged_rows(), p.row_bounds) == (m, m, m, (m - 1, m - 1))
    assert ops.round_kernel_name(p) == "k_round_clique_half"


def test_limits():
    small = _csr_of(nx.complete_graph(70))
    for fn in (ops.find_cliques, ops.build_clique_plan):
        for bad in (dict(max_members=130), dict(max_members=257), dict(max_members=256, per_source=True),
                    dict(max_members=256, per_source=True, wide_per_source=True)):
            with pytest.raises(ValueError):
                fn(*small, **bad)
    # beside a 200-block, the rows of a 257-member one land in the rest plan
    csr = _csr_of(nx.disjoint_union(nx.complete_graph(200), nx.complete_graph(257)))
    p = ops.build_clique_plan(*csr, max_members=256)
    assert (p.n_half, p.half_mmax) == (1, 200) and p.rest_rows == list(range(200, 457)) and p.rest.info.rows == 257


def test_blocks_up_to_128_are_unchanged():
    csr = _csr_of(nx.disjoint_union(nx.disjoint_union(nx.complete_graph(20), nx.complete_graph(100)), nx.cycle_graph(9)))
    p, q = ops.build_clique_plan(*csr, max_members=256), ops.build_clique_plan(*csr, max_members=128)
    assert p.half_table is None and (p.n_half, p.half_mmax) == (0, 0)
    assert p.table.tobytes() == q.table.tobytes() and p.col_table.tobytes() == q.col_table.tobytes()
    assert p.rest_rows == q.rest_rows and p.rest.host.tobytes() == q.rest.host.tobytes()
    assert p.make_spec() == q.make_spec() == {"clique": 1, "members": 128, "rest": q.rest.spec}
    # and the three forms in one plan, each block in its own table
    csr = _csr_of(nx.disjoint_union(nx.disjoint_union(nx.complete_graph(40), nx.complete_graph(100)), nx.complete_graph(200)))
    p = ops.build_clique_plan(*csr, max_members=256)
    assert (p.n_cliques, p.mmax, p.n_col, p.col_mmax, p.n_half, p.half_mmax) == (1, 40, 1, 100, 1, 200) and p.rest is None
    assert p.table.tobytes() == ops.build_clique_plan(*_csr_of(nx.complete_graph(40))).table.tobytes()
    assert p.half_table[4: 204].tolist() == list(range(140, 340)) and ops.round_kernel_name(p) == "k_round_clique"


def test_spec_gate_and_candidate():
    csr = _csr_of(nx.disjoint_union(nx.complete_graph(200), nx.cycle_graph(12)))
    p = ops.build_clique_plan(*csr, max_members=256)
    spec = p.make_spec()
    assert spec == {"clique": 1, "members": 256, "rest": p.rest.spec}
    q = ops.plan_from_spec(*csr, spec)
    assert q.spec == spec and q.half_table.tobytes() == p.half_table.tobytes() and q.rest_rows == p.rest_rows
    assert set(ops.CLIQUE_HALF_DEFAULT) == {(b, m) for b in (False, True) for m in (ops.MODE_EXACT, ops.MODE_FMA)}
    assert not any(ops.CLIQUE_HALF_DEFAULT.values())  # the default stays what it was
    assert not isinstance(ops.default_plan(*csr), ops.CliquePlan)
    assert all(k != ("clique256",) for k, _ in ops.tune_candidates(*csr))
    offered = [c for k, c in ops.tune_candidates(*csr, clique_half=True) if k == ("clique256",)]
    assert len(offered) == 1 and offered[0].spec == spec and offered[0].n_half == 1
    small = _csr_of(nx.complete_graph(100))  # no such block: not offered
    assert all(k != ("clique256",) for k, _ in ops.tune_candidates(*small, clique_half=True))


def test_abi_and_header_constants():
    L = _lib.load()
    assert L.tal_abi_version() == _lib.ABI_VERSION >= 37 and set(NAMES) <= set(_lib.EXPORTED)
    hdr = HDR.read_text()
    assert int(re.search(r"#define TAL_CLIQUE_HALF_MAX (\d+)", hdr).group(1)) == ops.CLIQUE_HALF_MAX == 256
    assert int(re.search(r"#define TAL_CLIQUE_HALF_WORDS (\d+)", hdr).group(1)) == ops.CLIQUE_HALF_WORDS == 4 + 2 * 256


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors(name):
    """Every argument error is answered before any GPU call (the pointers are not memory)."""
    fn = getattr(_lib.load(), name)
    good = dict(pin=0x1000, ld_in=64, pout=0x2000, ld_out=64, n=64, table=0x3000, blocks=1, mmax=200)
    for bad in (dict(pin=None), dict(pout=None), dict(table=None), dict(pout=0x1000), dict(mmax=0), dict(mmax=257),
                dict(blocks=-1), dict(blocks=65536), dict(ld_in=63), dict(ld_out=63), dict(n=-1)):
        a = {**good, **bad}
        for mode in (ops.MODE_EXACT, ops.MODE_FMA):
            rc = fn(ctypes.c_void_p(a["pin"]), a["ld_in"], ctypes.c_void_p(a["pout"]), a["ld_out"], a["n"],
                    ctypes.c_void_p(a["table"]), a["blocks"], a["mmax"], mode, None)
            assert rc == _lib.TAL_ERR_INVALID and name in _lib.load().tal_last_error().decode(), bad
