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
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).to(dev)


def _run(dev, bits, rp, col, w, out_row, n, ld=None, offset=0):
    """pool_out's bits [rows, ld], SENTINEL where the round did not write; ld defaults to n rounded
    up to 4 (8-B rows, as a ModelPool's); the pools start `offset` elements into their allocation."""
    rows, ld = bits.shape[0], ld or -(-bits.shape[1] // 4) * 4
    flat_in = torch.zeros(rows * ld + offset, dtype=torch.bfloat16, device=dev)
    flat_out = _dev(np.full(rows * ld + offset, SENTINEL, np.uint16), dev)
    pin, pout = (f[offset:].view(rows, ld) for f in (flat_in, flat_out))
    pin[:, :bits.shape[1]] = _dev(bits, dev)
    ops.round_matrix_bf16(pin, pout, ops.build_matrix_plan(rp, col, w, out_row), n)
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
