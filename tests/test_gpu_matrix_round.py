"""K3m on the GPU (tal_agg.h): the float64 bound, the non-finite rule, RoundExecutor(mode=MODE_MATRIX)."""
import numpy as np
import pytest
import torch

import _matrix as mx
import oracle
from topology_aware_learning_amd import ops
from topology_aware_learning_amd.arena import ModelPool, StateLayout
from topology_aware_learning_amd.round import RoundExecutor

pytestmark = pytest.mark.gpu
SENTINEL = 0x4D4D  # bf16 bits no round writes by chance: rows and columns a round must not touch


def _dev(bits, dev):
    return torch.from_numpy(np.array(bits).view(np.int16)).view(torch.bfloat16).to(dev)  # (a copy: shared inputs are read-only)


def _run(dev, bits, rp, col, w, out_row, n, ld=None, offset=0, ld_out=None, plan=None, stream=None):
    """pool_out's bits [rows, ld_out], SENTINEL where the round did not write; ld defaults to n rounded
    up to 4 (8-B rows, as a ModelPool's) and ld_out to ld; the pools start `offset` elements into their
    allocation.  plan: the round's plan, built here if None; stream: the round's, after the current one."""
    rows, ld = bits.shape[0], ld or -(-bits.shape[1] // 4) * 4
    ld_out = ld_out or ld
    flat_in = torch.zeros(rows * ld + offset, dtype=torch.bfloat16, device=dev)
    flat_out = _dev(np.full(rows * ld_out + offset, SENTINEL, np.uint16), dev)
    pin, pout = flat_in[offset:].view(rows, ld), flat_out[offset:].view(rows, ld_out)
    pin[:, :bits.shape[1]] = _dev(bits, dev)
    plan = plan or ops.build_matrix_plan(rp, col, w, out_row)
    if stream is not None:
        plan.to(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
    ops.round_matrix_bf16(pin, pout, plan, n, stream)
    if stream is not None:
        stream.synchronize()
    return pout.cpu().view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("n", [3, 128, 389])  # tail only; exactly one strip; strips, a partial one, an odd tail
@pytest.mark.parametrize("wname", mx.WEIGHTS)
@pytest.mark.parametrize("gname", mx.GRAPHS)
def test_round_within_the_bound(cuda, gname, wname, n):
    rp, col, w = mx.round_csr(gname, wname)
    rows = len(rp) - 1
    bits = mx.pool_bits(rows, n, seed=n, correlated=wname == "signed")
    got = _run(cuda, bits, rp, col, w, np.arange(rows, dtype=np.int32), n)
    assert (got[:, n:] == SENTINEL).all()
    mx.check_bound(got[:, :n], *mx.reference(bits, rp, col, w))


@pytest.mark.parametrize("layout", ["ld > n, permuted out_row", "pools offset by one element"])
def test_round_layouts(cuda, layout):
    """Nothing outside [out_row, :n] is touched; misaligned pools run the whole round as the chain."""
    rp, col, w = mx.round_csr("rr40x5", "positive")
    n, rows = 389, len(rp) - 1
    bits = mx.pool_bits(rows + 2, n, seed=11)
    out_row = np.random.default_rng(5).permutation(rows + 2)[:rows].astype(np.int32)
    got = _run(cuda, bits, rp, col, w, out_row, n, ld=400, offset=int(layout.startswith("pools offset")))
    mx.check_bound(got[out_row, :n], *mx.reference(bits, rp, col, w))
    untouched = np.ones(got.shape, bool)
    untouched[out_row, :n] = False
    assert (got[untouched] == SENTINEL).all()


@pytest.mark.parametrize("wname", ["ones", "positive"])
def test_non_finite_sources_reach_only_the_rows_that_list_them(cuda, wname):
    """Source s carries +inf, a NaN and 3e38 where a neighbor has 3e38 too: rows that list s are FMA
    mode's wherever that is not finite, the others bit for bit the round with s zeroed."""
    rp, col, w = mx.round_csr("rr40x5", "positive")
    if wname == "ones":
        w = np.ones_like(w)  # scale_agg without normalisation: the pair of 3e38 overflows
    rows, n, s = len(rp) - 1, 260, 7
    out_row = np.arange(rows, dtype=np.int32)
    bits = mx.pool_bits(rows, n, seed=13)
    nbr = int(col[rp[s]])
    poisoned = oracle.bf16_to_f32(bits).copy()
    poisoned[s, [20, 150, 257]] = [np.inf, np.nan, 3e38]  # a strip, the next strip, the strip's last group
    poisoned[nbr, 257] = 3e38
    poisoned = oracle.f32_to_bf16(poisoned)
    zeroed = poisoned.copy()
    zeroed[s] = 0
    got, got0 = (_run(cuda, b, rp, col, w, out_row, n)[:, :n] for b in (poisoned, zeroed))
    fma = oracle.bf16_to_f32(oracle.round_bf16(poisoned, rp, col, w, out_row, exact=False))
    lists = np.array([s in col[rp[r]: rp[r + 1]] for r in range(rows)])
    bad = ~np.isfinite(fma)
    assert lists.sum() == 6 and bad[lists][:, [20, 150]].all() and not bad[~lists][:, 12:].any()
    assert bad[s, 257] == (wname == "ones")
    assert np.array_equal(got[bad], oracle.f32_to_bf16(fma)[bad])
    assert np.array_equal(got[~lists], got0[~lists])


N_BIG = 389  # four strips, the last one partial, and an n % 4 tail


@pytest.mark.parametrize("wname", mx.WEIGHTS)
@pytest.mark.parametrize("gname", mx.BIG_GRAPHS)
def test_big_round_within_the_bound_and_deterministic(cuda, gname, wname):
    """Two groups, the first of eight tiles, three to five chunks: the bound, and the same bits from
    a second run of the same plan, on another stream."""
    bits, rp, col, w, out_row = mx.bound_case(gname, wname, N_BIG)
    plan = ops.build_matrix_plan(rp, col, w, out_row)
    got = _run(cuda, bits, rp, col, w, out_row, N_BIG, plan=plan)
    again = _run(cuda, bits, rp, col, w, out_row, N_BIG, plan=plan, stream=torch.cuda.Stream(cuda))
    assert (got[:, N_BIG:] == SENTINEL).all()
    print("error / bound:", mx.check_bound(got[:, :N_BIG], *mx.reference(bits, rp, col, w)))
    assert np.array_equal(got, again)


@pytest.mark.parametrize("gname,variant", mx.EXACT_CASES)
def test_exact_sums_bit_for_bit(cuda, gname, variant):
    """Small integers times powers of two (or short dyadic weights): every partial sum is exact in fp32 in
    any order, so the store's nearest-even rounding is the only one and the bits are FMA mode's
    (mx.exact_case).  A dropped, doubled or misplaced operand changes every element it touches."""
    bits, rp, col, w, out_row, want = mx.exact_case(gname, variant, N_BIG)
    got = _run(cuda, bits, rp, col, w, out_row, N_BIG)
    wrong = got[out_row, :N_BIG] != want
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:8].tolist())


def test_hand_round_with_two_leading_dimensions(cuda):
    """The hand-made round (sources outside the round, a permuted out_row into a larger pool, repeated
    sources, a uniform and two general tiles in one group) with ld_in = 400 and ld_out = 392."""
    bits, rp, col, w, out_row = mx.bound_case("hand", "own", N_BIG)
    got = _run(cuda, bits, rp, col, w, out_row, N_BIG, ld=400, ld_out=392)
    assert got.shape == (mx.HAND_POOL_ROWS, 392)
    print("error / bound:", mx.check_bound(got[out_row, :N_BIG], *mx.reference(bits, rp, col, w)))
    untouched = np.ones(got.shape, bool)
    untouched[out_row, :N_BIG] = False
    assert (got[untouched] == SENTINEL).all()
    bits, rp, col, w, out_row, want = mx.exact_case("hand", "own", N_BIG)
    got = _run(cuda, bits, rp, col, w, out_row, N_BIG, ld=400, ld_out=392)
    assert np.array_equal(got[out_row, :N_BIG], want) and (got[untouched] == SENTINEL).all()


def test_huge_weight_is_fma_modes_in_its_rows_and_reaches_no_other(cuda):
    """3.4e38 is finite in fp32 and infinite as a bf16 plane: times the source's 0 and 2^-120 the matrix
    cores give NaN and inf in every element of the six rows that list the source, which are therefore
    FMA mode's (finite) bits; the other rows are bit for bit the round with that weight set to 1.0."""
    bits, rp, col, w, w1, lists = mx.huge_weight_round(N_BIG)
    out_row = np.arange(len(rp) - 1, dtype=np.int32)
    got, got1 = (_run(cuda, bits, rp, col, ww, out_row, N_BIG)[:, :N_BIG] for ww in (w, w1))
    fma = oracle.round_bf16(bits, rp, col, w, out_row, exact=False)
    assert lists.sum() == 6 and np.isfinite(oracle.bf16_to_f32(fma[lists][:, 12:])).all()
    assert np.array_equal(got[lists], fma[lists])
    assert np.array_equal(got[~lists], got1[~lists])
    mx.check_bound(got, *mx.reference(bits, rp, col, w))


def test_tiny_weights_within_the_unchanged_bound(cuda):
    """Normal weights of 2^-124 .. 2^-119, whose lower planes would be bf16 subnormals, on inputs around
    2^100: the header's bound as it stands (the planner scales such rows, tests/test_matrix_plan_host.py)."""
    bits, rp, col, w, out_row = mx.bound_case("rr40x5", "tiny", N_BIG)
    got = _run(cuda, bits, rp, col, w, out_row, N_BIG)[:, :N_BIG]
    ref, bound = mx.reference(bits, rp, col, w)
    assert (np.abs(ref) > 2.0 ** -40).mean() > 0.99  # outputs far above the subnormals
    print("error / bound:", mx.check_bound(got, ref, bound))


def test_executor_mode_matrix_two_groups(cuda):
    """RoundExecutor(mode=MODE_MATRIX) on ring300: two groups; b16 within the bound, int64 the oracle's."""
    rp, col, w = mx.round_csr("ring300", "positive")
    rows, n = len(rp) - 1, 200
    orders = [col[rp[r]: rp[r + 1]].tolist() for r in range(rows)]
    weights = [w[rp[r]: rp[r + 1]].tolist() for r in range(rows)]
    bits = mx.pool_bits(rows, n, seed=41)
    counts = np.arange(1000, 1000 + rows, dtype=np.int64).reshape(rows, 1)
    pool = ModelPool(StateLayout.from_layout([("w", (n,), "bfloat16"), ("count", (), "int64")]), rows, cuda)
    pool.b16[:, :n] = _dev(bits, cuda)
    pool.i64[:, :1] = torch.from_numpy(counts).to(cuda)
    ex = RoundExecutor(pool, mode=ops.MODE_MATRIX, placement_trials=1)
    ex.run(orders, weights)
    plan = ex.plan(orders, weights, list(range(rows)))
    assert isinstance(plan, ops.MatrixPlan) and plan.info.n_groups == 2
    mx.check_bound(pool.b16[:, :n].cpu().view(torch.int16).numpy().view(np.uint16), *mx.reference(bits, rp, col, w))
    want = oracle.round_i64(counts, rp, col, w, np.arange(rows, dtype=np.int32))
    assert np.array_equal(pool.i64[:, :1].cpu().numpy(), want)


def test_executor_mode_matrix(cuda):
    """b16 through K3m, int64 through the full plan (bitwise the oracle); what the mode refuses."""
    rp, col, w = mx.round_csr("rr40x5", "positive")
    rows, n = len(rp) - 1, 200
    orders = [col[rp[r]: rp[r + 1]].tolist() for r in range(rows)]
    weights = [w[rp[r]: rp[r + 1]].tolist() for r in range(rows)]
    bits = mx.pool_bits(rows, n, seed=17)
    counts = np.arange(1000, 1000 + rows, dtype=np.int64).reshape(rows, 1)
    pool = ModelPool(StateLayout.from_layout([("w", (n,), "bfloat16"), ("count", (), "int64")]), rows, cuda)
    pool.b16[:, :n] = _dev(bits, cuda)
    pool.i64[:, :1] = torch.from_numpy(counts).to(cuda)
    ex = RoundExecutor(pool, mode=ops.MODE_MATRIX, placement_trials=1)
    ex.run(orders, weights)
    assert isinstance(ex.plan(orders, weights, list(range(rows))), ops.MatrixPlan)
    mx.check_bound(pool.b16[:, :n].cpu().view(torch.int16).numpy().view(np.uint16), *mx.reference(bits, rp, col, w))
    want = oracle.round_i64(counts, rp, col, w, np.arange(rows, dtype=np.int32))
    assert np.array_equal(pool.i64[:, :1].cpu().numpy(), want)
    with pytest.raises(ValueError, match="sequential"):
        ex.run(orders, weights, sequential=True)
    f32 = ModelPool(StateLayout.from_layout([("w", (8,), "float32")]), rows, cuda)
    with pytest.raises(ValueError, match="bf16"):
        RoundExecutor(f32, mode=ops.MODE_MATRIX)
    with pytest.raises(ValueError, match="MatrixPlan"):  # no quiet FMA round under MODE_MATRIX
        ops.round_bf16(pool.b16, torch.empty_like(pool.b16), ops.build_plan(rp, col, w, np.arange(rows)), n,
                       ops.MODE_MATRIX)
    short = pool.b16[: rows - 1].contiguous()  # the plan reads and writes row rows - 1
    for pin, pout in ((short, torch.empty_like(pool.b16)), (pool.b16, torch.empty_like(short))):
        with pytest.raises(ValueError, match="beyond the pools"):
            ops.round_matrix_bf16(pin, pout, ex.plan(orders, weights, list(range(rows))), n)
