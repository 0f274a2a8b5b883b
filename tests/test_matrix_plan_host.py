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


def _kb_counts(p):
    """Per tile, the k-blocks it visits in each chunk of its group."""
    i, b = p.info, p.host
    gt, gc = (b[off: off + i.n_groups + 1] for off in (i.off_grp_tile_ptr, i.off_grp_chunk_ptr))
    tkb, kbp = b[i.off_tile_kb_ptr: i.off_tile_kb_ptr + i.n_tiles], b[i.off_kb_ptr: i.off_tile_info]
    return [np.diff(kbp[tkb[t]: tkb[t] + gc[g + 1] - gc[g] + 1]).tolist()
            for g in range(i.n_groups) for t in range(gt[g], gt[g + 1])]


def _csr_weights(rp, col, w):
    """{(row, source): fp32 weight}, a source a row lists twice summed in float64."""
    want = defaultdict(float)
    for r in range(len(rp) - 1):
        for k in range(rp[r], rp[r + 1]):
            want[r, int(col[k])] += float(np.float32(w[k]))
    return dict(want)


# chunks per group; per tile the k-blocks per chunk (None: not pinned)
_RING300_KB = [[3, 0, 0, 0, 1], [3, 1, 0, 0, 0], [1, 3, 0, 0, 0], [0, 3, 1, 0, 0], [0, 1, 3, 0, 0], [0, 0, 3, 1, 0],
               [0, 0, 1, 3, 0], [0, 0, 0, 3, 1], [3], [1]]
_BIG_PLANS = [
    # tile t of group 0 lists the 34 sources 32 t - 1 .. 32 t + 32, 33 of them in one chunk and one in
    # a neighbouring one (tile 0: 0..32, and 299, the 258th source: chunks 0 and 4); group 1 lists 0
    # and 255..299, 46 sources: tile 8 34 of them (255..288), tile 9 0 and 287..299
    ("ring300", "unweighted", [5, 1], _RING300_KB),
    ("ring300", "positive", [5, 1], [[3 * k for k in t] for t in _RING300_KB]),
    ("rr300x7", "unweighted", [5, 4], None),
    ("rr300x7", "positive", [5, 4], None),
    # 300 sources for every row: 4 x 64 + 44, so 4 k-blocks per tile and chunk and 3 in the last
    ("complete300", "unweighted", [5, 5], [[4, 4, 4, 4, 3]] * 10),
    ("complete300", "positive", [5, 5], [[12, 12, 12, 12, 9]] * 10),
    ("hand", "own", [2], [[3, 2], [10, 5], [1, 3]]),
]


@pytest.mark.parametrize("gname,wname,chunks,kblocks", _BIG_PLANS, ids=[f"{g}-{w}" for g, w, _, _ in _BIG_PLANS])
def test_big_plans_decode_to_the_csr(gname, wname, chunks, kblocks):
    """Rounds of more than one group and more than two chunks, and the hand-made round (sources outside
    the round, repeated sources, a uniform and two general tiles in one group): the blob decodes to
    the CSR exactly, through chunk, source and k-block offsets that do not start at zero."""
    if gname == "hand":
        rp, col, w, out_row = mx.hand_round()
    else:
        rp, col, w = mx.round_csr(gname, wname)
        out_row = np.arange(len(rp) - 1, dtype=np.int32)[::-1].copy()
    p = ops.build_matrix_plan(rp, col, w, out_row)
    i = p.info
    assert i.words == len(p.host) <= _lib.load().tal_matrix_plan_words(len(rp) - 1, len(col))
    assert i.n_groups == len(chunks) == (1 if gname == "hand" else 2)
    assert np.diff(p.host[i.off_grp_chunk_ptr: i.off_grp_chunk_ptr + i.n_groups + 1]).tolist() == chunks
    tiles = [3] if gname == "hand" else [8, 2]
    assert np.diff(p.host[i.off_grp_tile_ptr: i.off_grp_tile_ptr + i.n_groups + 1]).tolist() == tiles
    got, planes, _ = _decode(p)
    assert got == _csr_weights(rp, col, w)
    assert planes == ([1, 3, 3] if gname == "hand" else [1 if wname == "unweighted" else 3] * 10)
    counts = _kb_counts(p)
    assert sum(map(sum, counts)) == i.n_kblocks
    assert [len(c) for c in counts] == [chunks[g] for g, nt in enumerate(tiles) for _ in range(nt)]
    if kblocks is not None:
        assert counts == kblocks
    if gname == "ring300":  # five chunks of 64, 64, 64, 64 and 2 sources, then one of 46
        assert np.diff(p.host[i.off_chunk_src_ptr: i.off_chunk_src_ptr + 7]).tolist() == [64, 64, 64, 64, 2, 46]
    if gname == "hand":
        assert i.n_kblocks == mx.HAND_KBLOCKS and i.n_src == mx.HAND_POOL_ROWS and i.max_row == mx.HAND_POOL_ROWS - 1
        assert col.max() >= len(rp) - 1 and sorted(out_row) != list(range(len(rp) - 1))


def test_two_pass_build_equals_the_one_pass_build():
    """complete300's size bound passes MATRIX_PLAN_ONE_PASS, so build_matrix_plan asks for the size
    first; its blob is the one a single pass writes into a buffer of exactly info.words."""
    rp, col, w = mx.round_csr("complete300", "positive")
    rows, L = len(rp) - 1, _lib.load()
    assert L.tal_matrix_plan_words(rows, len(col)) > ops.MATRIX_PLAN_ONE_PASS
    assert L.tal_matrix_plan_words(rows, len(mx.round_csr("rr300x7", "positive")[1])) <= ops.MATRIX_PLAN_ONE_PASS
    out_row = np.arange(rows, dtype=np.int32)
    p = ops.build_matrix_plan(rp, col, w, out_row)
    P32, info = ctypes.POINTER(ctypes.c_int32), _lib.MatrixPlanInfo()
    blob = np.full(p.info.words, -1, np.int32)
    rc = L.tal_matrix_plan_build(rows, rp.ctypes.data_as(P32), col.ctypes.data_as(P32), w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                 out_row.ctypes.data_as(P32), blob.ctypes.data_as(P32), len(blob), ctypes.byref(info))
    assert rc == _lib.TAL_OK and info.words == p.info.words == len(p.host) and np.array_equal(blob, p.host)
    assert bytes(info) == bytes(p.info)


def test_tiny_weights_split_exactly_into_normal_planes():
    """Weights of 2^-124 .. 2^-119: split as they are, their second plane is a bf16 subnormal of a few
    bits and the third is lost (the planes then miss fp32(w) by up to 2^-10.6 of it).  The planner takes
    a power of two out of such a row into its epilogue scale: the planes are exact and normal."""
    _, rp, col, w = mx.tiny_weight_round(8)
    p = ops.build_matrix_plan(rp, col, w, np.arange(len(rp) - 1, dtype=np.int32))
    got, planes, _ = _decode(p)
    assert got == _csr_weights(rp, col, w) and planes == [3, 3]
    i = p.info
    a = np.abs(oracle.bf16_to_f32(p.host[i.off_a_tiles: i.off_a_tiles + 256 * i.n_kblocks].view(np.uint16)))
    assert a[a != 0].min() >= 2.0 ** -126
    tw = p.host[i.off_tile_w: i.off_tile_w + 64].view(np.float32)[: len(rp) - 1]
    assert (np.frexp(tw)[0] == 0.5).all() and (tw < 2.0 ** -10).all()  # powers of two
    # a row without such a weight keeps the scale 1.0, and a huge weight its infinite first plane
    _, rp, col, w = mx.huge_weight_round(8)[:4]
    p = ops.build_matrix_plan(rp, col, w, np.arange(len(rp) - 1, dtype=np.int32))
    i = p.info
    assert (p.host[i.off_tile_w: i.off_tile_w + 64].view(np.float32)[: len(rp) - 1] == 1.0).all()
    assert np.isinf(oracle.bf16_to_f32(p.host[i.off_a_tiles: i.off_a_tiles + 256 * i.n_kblocks].view(np.uint16))).sum() == 6


@pytest.mark.parametrize("gname,wname", [(g, w) for g in mx.GRAPHS for w in mx.WEIGHTS] + list(mx.NEW_BOUND_CASES))
def test_fma_oracle_stays_inside_the_matrix_bound(gname, wname):
    """The GPU test's inputs do not break the bound by themselves: FMA mode's own result is inside it."""
    if (gname, wname) in mx.NEW_BOUND_CASES:
        bits, rp, col, w, out_row = mx.bound_case(gname, wname)
    else:
        rp, col, w = mx.round_csr(gname, wname)
        bits = mx.pool_bits(len(rp) - 1, 389, seed=7, correlated=wname == "signed")
        out_row = np.arange(len(rp) - 1, dtype=np.int32)
    got = oracle.round_bf16(bits, rp, col, w, out_row, exact=False)[out_row]
    assert mx.check_bound(got, *mx.reference(bits, rp, col, w)) <= 1.0


@pytest.mark.parametrize("gname,variant", mx.EXACT_CASES)
def test_exact_sum_rounds_are_exact_and_land_on_ties(gname, variant):
    """The inputs of the GPU's bit-for-bit test, judged by the reference alone: mx.exact_case asserts
    that every sum is exact in any order, that FMA mode's oracle is the sum rounded once, and the ties."""
    mx.exact_case(gname, variant)
