"""Shared by the matrix-round tests (tests/test_matrix_plan_host.py, tests/test_gpu_matrix_round.py):
the rounds, their bf16 inputs, the float64 reference and tal_agg.h's K3m error bound."""
import networkx as nx
import numpy as np

import oracle
from topology_aware_learning_amd import ops

GRAPHS = ("ring8", "rr40x5", "sbm3x24", "complete33", "complete_chunk+1")
# 300 rows = 256 + 32 + 12: a full group of eight tiles, then a group of a full and a partial tile
BIG_GRAPHS = ("ring300", "rr300x7", "complete300")
WEIGHTS = ("unweighted", "positive", "signed")
BF16_OVERFLOW = 2.0 ** 128 - 2.0 ** 119  # from here on a value rounds to a bf16 infinity


def graph(name):
    return {"ring8": lambda: nx.cycle_graph(8),  # a partial row tile and a partial k-block
            "rr40x5": lambda: nx.random_regular_graph(5, 40, seed=2),  # two row tiles
            "sbm3x24": lambda: nx.stochastic_block_model(  # three tiles, more than 64 sources: two chunks
                [24] * 3, np.full((3, 3), 0.05) + np.eye(3) * 0.5, seed=3),
            "complete33": lambda: nx.complete_graph(33),  # k padding 33 -> 48
            # one source more than an LDS chunk: the accumulators cross a chunk boundary
            "complete_chunk+1": lambda: nx.complete_graph(ops.MATRIX_CHUNK + 1),
            # group 0: sources 0..256 and 299, five chunks, the last of two sources; a tile has k-blocks
            # in two of them (tile 0: the first and the last); group 1: every offset non-zero
            "ring300": lambda: nx.cycle_graph(300),
            # nearly every (tile, chunk) pair with a partially filled k-block
            "rr300x7": lambda: nx.random_regular_graph(7, 300, seed=4),
            # five chunks in both groups: each LDS buffer is overwritten twice; 90,000 operands
            "complete300": lambda: nx.complete_graph(300)}[name]()


def round_csr(gname, wname, seed=0):
    """(row_ptr, col, w), operands in reference order; sum |w| <= 1 per row, so no partial sum overflows
    where its terms do not.  "signed": zero-sum weights of distinct magnitudes with zeros among them."""
    g = graph(gname)
    rng = np.random.default_rng(seed)
    orders = [sorted(g.neighbors(i)) + [i] for i in sorted(g.nodes)]
    ws = []
    for o in orders:
        m = len(o)
        if wname == "unweighted":
            w = np.full(m, 1.0 / m)
        elif wname == "positive":
            w = rng.uniform(0.1, 1.0, m)
            w /= w.sum() * (1 + 2.0 ** -20)
        else:
            w = rng.standard_normal(m)
            w[rng.random(m) < 0.25] = 0.0
            nz = w != 0
            w[nz] -= w[nz].mean() if nz.sum() > 1 else 0.0
            w /= max(np.abs(w).sum(), 1e-3) * (1 + 2.0 ** -20)
        ws.append(w)
    row_ptr = np.cumsum([0] + [len(o) for o in orders]).astype(np.int32)
    return row_ptr, np.concatenate(orders).astype(np.int32), np.concatenate(ws).astype(np.float64)


def pool_bits(rows, n, seed, correlated=False):
    """[rows, n] bf16 bits as tests/test_gpu_bf16.py::_bf16_bits (subnormals and +-3.3e38 when n > 12).
    correlated: one base row with bf16-ulp noise, so zero-sum weights cancel: |ref| << sum |w x|."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, n)) * 3.0).astype(np.float32)
    if correlated:
        x = x[:1] * (1.0 + 2.0 ** -7 * rng.standard_normal((rows, n))).astype(np.float32)
    if n > 12:
        x[:, :12] = [1e-40, -0.0, 3.3e38, -1e-45, 65504.0, 1.17e-38, -3.3e38, 2.0 ** -133, 0.0, 1.0, -1.0, 3.0e38]
    return oracle.f32_to_bf16(x)


def reference(bits, row_ptr, col, w):
    """(float64 sum of fp32(w_k) x_k, 2^-8 |ref| + (3M + 2) 2^-23 sum |w x| + (3M + 1) 2^-126) per row."""
    x = oracle.bf16_to_f32(bits).astype(np.float64)
    w32 = np.asarray(w, np.float32).astype(np.float64)
    ref, bound = [], []
    for r in range(len(row_ptr) - 1):
        a, b = row_ptr[r], row_ptr[r + 1]
        terms = w32[a:b, None] * x[col[a:b]]
        ref.append(terms.sum(0))
        m = b - a
        bound.append(2.0 ** -8 * np.abs(ref[-1]) + (3 * m + 2) * 2.0 ** -23 * np.abs(terms).sum(0)
                     + (3 * m + 1) * 2.0 ** -126)
    return np.array(ref), np.array(bound)


def check_bound(got_bits, ref, bound):
    """got (bf16 bits) within the bound; returns the largest |error| / bound.  Left out, beyond the
    non-finite references: elements whose bound itself admits a bf16 infinity (|ref| + bound past
    the overflow threshold: only +-3.3e38 columns), so at least 95 % of the elements are checked."""
    got = oracle.bf16_to_f32(got_bits).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(ref) & (np.abs(ref) + bound < BF16_OVERFLOW)
        assert ok.mean() > 0.95
        frac = np.abs(got[ok] - ref[ok]) / bound[ok]
    worst = float(frac.max())
    assert np.isfinite(got[ok]).all() and worst <= 1.0, worst
    return worst


HAND_POOL_ROWS = 90
# the k-blocks of hand_round(), from which planes vanish (pool row == source index: all 90 are listed).
# Tile 0 (uniform, one plane): 33 sources + (5, second occurrence) in chunk 0 -> 3, 70..89 in chunk 1 -> 2.
# Tile 1, chunk 0: 64 sources + (8, 2nd), (8, 3rd), (51, 2nd) = 67 entries in five k-blocks; in entry order
# the blocks end at sources 13, 29, 45, 60, 63, so their widest weights need 1, 1, 2, 3, 3 planes -> 10;
# chunk 1: sources 64..79 (two planes) and 80..89 (three) -> 5.
# Tile 2: sources 4..9 (one plane) -> 1; 64..69 + (66, 2nd) + 84..89 in one k-block of three planes -> 3.
HAND_KBLOCKS = (3 + 2) + (10 + 5) + (1 + 3)


def hand_round():
    """(row_ptr, col, w, out_row): 70 rows over a pool of HAND_POOL_ROWS, one group of three tiles and two
    chunks.  Pool rows 70..89 are sources and no rows of the round; out_row is a permutation into the
    pool; rows 5, 40, 50 and 66 list a source two or three times (40 and 66: as the first and the last
    operand), 40, 50 and 66 with different weights.  Rows 0..31 carry one weight per row (a uniform tile),
    the others a weight per operand whose planes depend on the source: exact in bf16 (planes 2 and 3
    vanish) below source 32, two planes for 32..47 and 64..79, three for 48..63 and 80..89.  Every weight
    is a short dyadic number, so the repeated sources' sums and, on small integers, every round sum are exact."""
    def weight(s, pos):
        if s < 32:
            return (8 + pos) / 16
        return (1 + 2.0 ** -9 + (2.0 ** -17 if 48 <= s < 64 or s >= 80 else 0.0)) * 2.0 ** -(pos % 2)
    orders, ws = [], []
    for r in range(70):
        if r < 32:
            o = [5, 6, 75, 5] if r == 5 else [r + 1, 70 + r % 20, r]
            w = [2.0 ** -(r % 4)] * len(o)
        else:
            o = {40: [8, 40, 8, 41, 72, 8], 50: [18, 50, 51, 51, 82], 66: [66, 6, 86, 66]}.get(
                r, [r - 32, r, r + 1, 64 + (r - 32) % 26] if r < 64 else [r - 60, r, r + 20])
            w = [weight(s, pos) for pos, s in enumerate(o)]
        orders.append(o)
        ws.append(w)
    row_ptr = np.cumsum([0] + [len(o) for o in orders]).astype(np.int32)
    out_row = np.random.default_rng(5).permutation(HAND_POOL_ROWS)[:70].astype(np.int32)
    return row_ptr, np.concatenate(orders).astype(np.int32), np.concatenate(ws).astype(np.float64), out_row


# ---- rounds whose sums are exact: the only rounding is the store's, so K3m is pinned bit for bit ----
EXACT_VARIANTS = ("row", "operand", "planes")


def exact_weights(row_ptr, variant, seed=0):
    """Positive weights with few bits.  "row": one power of two per row (uniform tiles); "operand":
    2^-j per operand, j in 0..7 (general tiles, planes 2 and 3 vanish); "planes": (1 + 2^-9 + 2^-17) 2^-j,
    j <= 1, which needs all three planes (bf16(w) = 2^-j, then 2^-9-j, then 2^-17-j)."""
    rng = np.random.default_rng(seed)
    m = np.diff(row_ptr)
    if variant == "row":
        return np.repeat(2.0 ** -rng.integers(0, 8, len(m)), m)
    if variant == "operand":
        return 2.0 ** -rng.integers(0, 8, int(m.sum())).astype(np.float64)
    return (1 + 2.0 ** -9 + 2.0 ** -17) * 2.0 ** -rng.integers(0, 2, int(m.sum())).astype(np.float64)


def int_pool_bits(rows, n, seed, lo=-3, hi=8):
    """[rows, n] bf16 bits of integers lo..hi: off centre, so that the sums of a wide row pass 256,
    where every odd integer is a bf16 tie."""
    return oracle.f32_to_bf16(np.random.default_rng(seed).integers(lo, hi + 1, (rows, n)).astype(np.float32))


def exact_sums(bits, row_ptr, col, w):
    """The round's sums in float64, after asserting that they are exact in fp32 in ANY order: the inputs
    are integers, so every product and partial sum is a multiple of q = the smallest unit (lowest set
    bit) among the row's weights, and sum_k |w_k x_k| < 2^24 q bounds every partial sum."""
    x = oracle.bf16_to_f32(bits).astype(np.float64)
    w32 = np.asarray(w, np.float32).astype(np.float64)
    assert (x == np.rint(x)).all() and (w32 == w).all() and (w32 > 0).all()
    mant, exp = np.frexp(w32)
    mant = (mant * 2.0 ** 53).astype(np.int64)
    unit = (mant & -mant).astype(np.float64) * 2.0 ** (exp - 53)
    sums = []
    for r in range(len(row_ptr) - 1):
        a, b = row_ptr[r], row_ptr[r + 1]
        terms = w32[a:b, None] * x[col[a:b]]
        assert (np.abs(terms).sum(0) < 2.0 ** 24 * unit[a:b].min()).all()
        sums.append(terms.sum(0))
    return np.array(sums)


def round_once(sums):
    """(bf16 bits of the exact sums rounded once to nearest even, ties that round down, ties that round
    up), in integer arithmetic on the sums' fp32 bits (the sums are exact in fp32: exact_sums)."""
    assert (sums.astype(np.float32).astype(np.float64) == sums).all()
    u = sums.astype(np.float32).view(np.uint32)
    tie, odd = (u & 0xFFFF) == 0x8000, (u >> 16) & 1 == 1
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16), tie & ~odd, tie & odd


EXACT_CASES = tuple((g, v) for g in BIG_GRAPHS for v in ("row", "operand")) + (
    ("ring300", "planes"), ("rr300x7", "planes"), ("hand", "own"))  # "planes": M <= 8 keeps the sums exact
# where a sum needs more than 8 bits often enough to land on ties: every weight a power of two, and
# either weights that differ within a row or a row wide enough for integer sums past 256
_EXACT_WITH_TIES = tuple((g, "operand") for g in BIG_GRAPHS) + (("complete300", "row"),)
# where the reference's own bf16 arithmetic (every product and partial sum rounded to bf16) is exact
# too: one weight per row and at most 8 operands of at most 8, so no partial sum needs more than 7 bits
_EXACT_IN_BF16 = (("ring300", "row"), ("rr300x7", "row"))
_exact_cache = {}


def exact_case(gname, variant, n=389):
    """(bits, row_ptr, col, w, out_row, the output rows' bf16 bits) of a round on small integers whose
    every sum is exact in fp32 in any order (exact_sums asserts it), so that the store's rounding is the
    only one and K3m must give FMA mode's bits.  The expected bits are oracle.round_bf16(exact=False),
    asserted equal to the exact sums rounded once in integer arithmetic; oracle.round_bf16(exact=True)
    gives the same bits where its bf16 partial sums are exact too (_EXACT_IN_BF16), and cannot
    elsewhere.  _EXACT_WITH_TIES: ties rounding down and up are asserted among the sums, so a store
    that rounds half up (or truncates) differs from the expected bits.  Computed once per case."""
    if (gname, variant, n) in _exact_cache:
        return _exact_cache[gname, variant, n]
    if gname == "hand":
        rp, col, w, out_row = hand_round()
        bits = int_pool_bits(HAND_POOL_ROWS, n, seed=31)
    else:
        rp, col, _ = round_csr(gname, "unweighted")
        w = exact_weights(rp, variant, seed=3)
        out_row = np.arange(len(rp) - 1, dtype=np.int32)
        bits = int_pool_bits(len(rp) - 1, n, seed=37, **(dict(lo=-2, hi=4) if variant == "planes" else {}))
    want, down, up = round_once(exact_sums(bits, rp, col, w))
    assert np.array_equal(oracle.round_bf16(bits, rp, col, w, out_row, exact=False)[out_row], want)
    if (gname, variant) in _EXACT_IN_BF16:
        assert np.array_equal(oracle.round_bf16(bits, rp, col, w, out_row, exact=True)[out_row], want)
    if (gname, variant) in _EXACT_WITH_TIES:
        assert down.sum() >= 8 and up.sum() >= 8, (down.sum(), up.sum())
    for a in (bits, want):
        a.setflags(write=False)
    _exact_cache[gname, variant, n] = bits, rp, col, w, out_row, want
    return _exact_cache[gname, variant, n]


# ---- weight edges on rr40x5(tests/test_gpu_matrix_round.py, "weight edges") ----
HUGE = 3.4e38  # finite in fp32; its first bf16 plane is infinite
HUGE_SOURCE = 7


def huge_weight_round(n, seed=19):
    """(bits, row_ptr, col, w, w with the huge weight set to 1.0, rows that list HUGE_SOURCE): rr40x5,
    "positive", where every operand HUGE_SOURCE weighs HUGE; that source holds 0 in the even columns
    and 2^-120 in the odd ones, so every fp32 term and FMA mode's result are finite."""
    rp, col, w = round_csr("rr40x5", "positive")
    rows = len(rp) - 1
    x = oracle.bf16_to_f32(pool_bits(rows, n, seed)).copy()
    x[HUGE_SOURCE] = np.where(np.arange(n) % 2 == 0, 0.0, 2.0 ** -120)
    w1 = w.copy()
    w1[col == HUGE_SOURCE] = 1.0
    w = w.copy()
    w[col == HUGE_SOURCE] = HUGE
    lists = np.array([HUGE_SOURCE in col[rp[r]: rp[r + 1]] for r in range(rows)])
    return oracle.f32_to_bf16(x), rp, col, w, w1, lists


NEW_BOUND_CASES = tuple((g, w) for g in BIG_GRAPHS for w in WEIGHTS) + (("hand", "own"), ("rr40x5", "huge"), ("rr40x5", "tiny"))


def bound_case(gname, wname, n=389):
    """(bits, row_ptr, col, w, out_row) of one of NEW_BOUND_CASES, the same on the host (where FMA mode's
    own result shows the inputs fair) and on the GPU."""
    if gname == "hand":
        rp, col, w, out_row = hand_round()
        return pool_bits(HAND_POOL_ROWS, n, seed=29), rp, col, w, out_row
    if wname == "huge":
        bits, rp, col, w = huge_weight_round(n)[:4]
    elif wname == "tiny":
        bits, rp, col, w = tiny_weight_round(n)
    else:
        rp, col, w = round_csr(gname, wname)
        bits = pool_bits(len(rp) - 1, n, seed=n, correlated=wname == "signed")
    return bits, rp, col, w, np.arange(len(rp) - 1, dtype=np.int32)


def tiny_weight_round(n, seed=23):
    """(bits, row_ptr, col, w): rr40x5, "positive" scaled by 2^-118 - every fp32(w) is normal, while
    bf16(w - bf16(w)) and what it leaves are below the bf16 normals - on inputs around 2^100, so that the
    outputs (around 2^-20) are normal."""
    rp, col, w = round_csr("rr40x5", "positive")
    w = w * 2.0 ** -118
    assert (np.abs(w.astype(np.float32)) >= 2.0 ** -126).all() and (np.abs(w) < 2.0 ** -118).all()
    x = np.random.default_rng(seed).standard_normal((len(rp) - 1, n)) * 3.0 * 2.0 ** 100
    return oracle.f32_to_bf16(x.astype(np.float32)), rp, col, w
