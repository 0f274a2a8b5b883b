"""K3m, host side: ABI 36, the planner's route, the capacity protocol, the round entry's argument
checks, the plan blob decoded back to the CSR, and the FMA oracle inside K3m's bound."""
import ctypes
from collections import defaultdict

import numpy as np
import pytest

import _matrix as mx
import oracle
from topology_aware_learning_amd import _lib, ops
from topology_aware_learning_amd.build import HDR

def test_abi_36_declares_the_matrix_entries():
    L = _lib.load()
    assert L.tal_abi_version() == _lib.ABI_VERSION >= 36 and ops.MODE_MATRIX == _lib.TAL_MODE_MATRIX == 2
    hdr = HDR.read_text()
    assert "#define TAL_MODE_MATRIX 2" in hdr and f"#define TAL_MATRIX_CHUNK {ops.MATRIX_CHUNK}\n" in hdr
    for name in ("tal_matrix_plan_words", "tal_matrix_plan_build", "tal_agg_round_matrix_bf16"):
        assert name in _lib.EXPORTED and name + "(" in hdr and getattr(L, name).argtypes == _lib._SIGS[name][1]
    # the planner's route, and the capacity protocol: without a buffer the build reports the words needed
    rp, col, w, p = _plan("ring8", "unweighted")
    routed = ops.default_plan(rp, col, w, np.arange(8), bf16=True, mode=ops.MODE_MATRIX)
    assert isinstance(routed, ops.MatrixPlan) and isinstance(routed.full, ops.RoundPlan)
    with pytest.raises(ValueError, match="bf16"):
        ops.default_plan(rp, col, w, np.arange(8), bf16=False, mode=ops.MODE_MATRIX)
    P32, info = ctypes.POINTER(ctypes.c_int32), _lib.MatrixPlanInfo()
    rc = L.tal_matrix_plan_build(8, rp.ctypes.data_as(P32), col.ctypes.data_as(P32), w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                 np.arange(8, dtype=np.int32).ctypes.data_as(P32), None, 0, ctypes.byref(info))
    assert rc == _lib.TAL_ERR_CAPACITY and info.words == len(p.host) <= L.tal_matrix_plan_words(8, len(col))


def _plan(gname, wname):
    rp, col, w = mx.round_csr(gname, wname)
    return rp, col, w, ops.build_matrix_plan(rp, col, w, np.arange(len(rp) - 1, dtype=np.int32)[::-1].copy())


@pytest.mark.parametrize("case,kw,rc", [
    ("valid, n == 0: no launch", dict(n=0), _lib.TAL_OK),
    ("null pool_in", dict(pin=None), _lib.TAL_ERR_INVALID),
    ("null pool_out", dict(pout=None), _lib.TAL_ERR_INVALID),
    ("null plan", dict(plan=None), _lib.TAL_ERR_INVALID),
    ("null info", dict(info=None), _lib.TAL_ERR_INVALID),
    ("pool_out == pool_in", dict(pout=4096), _lib.TAL_ERR_INVALID),
    ("ld_in < n", dict(ld_in=99), _lib.TAL_ERR_INVALID),
    ("ld_out < n", dict(ld_out=99), _lib.TAL_ERR_INVALID),
    ("n < 0", dict(n=-1), _lib.TAL_ERR_INVALID),
    ("a plan row beyond the pools", dict(rows=7), _lib.TAL_ERR_INVALID),  # ring8 reads and writes row 7
    ("an empty info", dict(info=_lib.MatrixPlanInfo()), _lib.TAL_ERR_INVALID),
])
def test_round_entry_checks_its_arguments_before_any_launch(case, kw, rc):
    info = _plan("ring8", "unweighted")[3].info
    a = dict(pin=4096, ld_in=100, pout=8192, ld_out=100, rows=8, n=100, plan=12288, info=info)
    a.update(kw)
    got = _lib.load().tal_agg_round_matrix_bf16(a["pin"], a["ld_in"], a["pout"], a["ld_out"], a["rows"], a["n"], a["plan"],
                                                None if a["info"] is None else ctypes.byref(a["info"]), None)
    assert got == rc, (case, _lib.load().tal_last_error())


def _decode(p):
    """({(round row, source row): sum over planes of A x epilogue scale}, planes per tile, padding slots)."""
    i, b = p.info, p.host
    arr = lambda off, n: b[off: off + n]  # noqa: E731
    gt, gc = arr(i.off_grp_tile_ptr, i.n_groups + 1), arr(i.off_grp_chunk_ptr, i.n_groups + 1)
    cs, src = arr(i.off_chunk_src_ptr, i.n_chunks + 1), arr(i.off_src_row, i.n_src)
    tkb, kbp = arr(i.off_tile_kb_ptr, i.n_tiles), b[i.off_kb_ptr: i.off_tile_info]
    tinfo = arr(i.off_tile_info, 4 * i.n_tiles).reshape(-1, 4)
    tw = arr(i.off_tile_w, 32 * i.n_tiles).view(np.float32).reshape(-1, 32).astype(np.float64)
    slots = arr(i.off_kb_slots, 4 * i.n_kblocks).view(np.uint8).reshape(-1, 16)
    a = oracle.bf16_to_f32(arr(i.off_a_tiles, 256 * i.n_kblocks).view(np.uint16)).astype(np.float64).reshape(-1, 64, 8)
    assert i.off_a_tiles % 4 == 0 and np.diff(cs).max() <= ops.MATRIX_CHUNK and np.diff(gt).max() <= ops.MATRIX_GROUP_TILES
    weights, pads, seen = defaultdict(float), 0, 0
    for g in range(i.n_groups):
        for t in range(gt[g], gt[g + 1]):
            r0, nr = tinfo[t, :2]
            for c in range(gc[g + 1] - gc[g]):
                for kb in range(kbp[tkb[t] + c], kbp[tkb[t] + c + 1]):
                    seen += 1
                    for k in range(16):
                        column = a[kb, 32 * (k // 8): 32 * (k // 8) + 32, k % 8]  # A[row 0..31][k]
                        assert not column[nr:].any()
                        if slots[kb, k] == ops.MATRIX_PAD:
                            pads += 1
                            assert not column.any()
                            continue
                        assert slots[kb, k] < cs[gc[g] + c + 1] - cs[gc[g] + c]
                        for r in range(nr):
                            if column[r]:
                                weights[r0 + r, src[cs[gc[g] + c] + slots[kb, k]]] += column[r] * tw[t, r]
    assert seen == i.n_kblocks
    return dict(weights), tinfo[:, 2].tolist(), pads


@pytest.mark.parametrize("gname,wname,planes,kblocks,pads", [
    ("ring8", "unweighted", [1], 1, 8),                  # 8 sources in one k-block of 16
    ("rr40x5", "positive", [3, 3], 3 * (3 + 3), None),   # per-operand weights: every k-block three times
    ("complete33", "unweighted", [1, 1], 3 + 3, 2 * 15),  # 33 sources -> 48 slots, in both tiles
])
def test_plan_decodes_to_the_csr(gname, wname, planes, kblocks, pads):
    rp, col, w, p = _plan(gname, wname)
    rows = len(rp) - 1
    assert isinstance(p, ops.MatrixPlan) and p.spec == {"matrix": 1} and not p.single_group and p.full is not None
    assert p.host[:9].tolist() == [rows, len(col), p.info.n_groups, (rows + 31) // 32, p.info.n_chunks,
                                   p.info.n_kblocks, p.info.n_src, rows - 1, len(p.host)]
    i = p.info
    assert np.array_equal(p.host[i.off_row_ptr: i.off_col], rp) and np.array_equal(p.host[i.off_col: i.off_w], col)
    assert np.array_equal(p.host[i.off_w: i.off_out_row].view(np.float32), w.astype(np.float32))
    assert p.host[i.off_out_row:].tolist() == list(range(rows))[::-1]
    got, got_planes, got_pads = _decode(p)
    want = {(r, int(col[k])): float(np.float32(w[k])) for r in range(rows) for k in range(rp[r], rp[r + 1])}
    assert got == want  # every weight exactly fp32(w): the planes lose nothing
    assert got_planes == planes and (pads is None or got_pads == pads)
    assert i.n_kblocks == kblocks if wname == "unweighted" else i.n_kblocks <= kblocks


@pytest.mark.parametrize("wname", mx.WEIGHTS)
@pytest.mark.parametrize("gname", mx.GRAPHS)
def test_fma_oracle_stays_inside_the_matrix_bound(gname, wname):
    """The GPU test's inputs do not break the bound by themselves: FMA mode's own result is inside it."""
    rp, col, w = mx.round_csr(gname, wname)
    bits = mx.pool_bits(len(rp) - 1, 389, seed=7, correlated=wname == "signed")
    got = oracle.round_bf16(bits, rp, col, w, np.arange(len(rp) - 1, dtype=np.int32), exact=False)
    assert mx.check_bound(got, *mx.reference(bits, rp, col, w)) <= 1.0
