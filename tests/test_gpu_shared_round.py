"""K3ms on the GPU (tal_agg.h): the matrix mode's float64 bound, the lane ladder, exact sums bit for bit,
the non-finite rule and RoundExecutor(mode=MODE_MATRIX, shared=True)."""
import numpy as np
import pytest
import torch

import _matrix as mx
import oracle
from test_shared_plan_host import CASES, case
from topology_aware_learning_amd import ops
from topology_aware_learning_amd.arena import ModelPool, StateLayout
from topology_aware_learning_amd.round import RoundExecutor

pytestmark = pytest.mark.gpu
SENTINEL = 0x4D4D  # bf16 bits no round writes by chance
N = 389  # 48 16-B lanes + 5 columns, 97 8-B lanes + 1: body and tail both run
# (offset, ld_in, ld_out) in elements: a ModelPool's 64-element stride; 8-B rows; odd, 2-B rows
LAYOUTS = {"16-B lanes": (0, 448, 456), "8-B lanes": (4, 392, 396), "element lanes": (1, 391, 393)}


def _dev(bits, dev):
    return torch.from_numpy(np.array(bits).view(np.int16)).view(torch.bfloat16).to(dev)


def _run(dev, bits, rp, col, w, out_row, layout="16-B lanes", kind=ops.SharedPlan):
    """The first N columns of pool_out after the round; nothing outside [out_row, :N] may be written."""
    offset, ld_in, ld_out = LAYOUTS[layout]
    rows = bits.shape[0]
    flat_in = torch.zeros(rows * ld_in + offset, dtype=torch.bfloat16, device=dev)
    flat_out = _dev(np.full(rows * ld_out + offset, SENTINEL, np.uint16), dev)
    pin, pout = flat_in[offset:].view(rows, ld_in), flat_out[offset:].view(rows, ld_out)
    pin[:, :N] = _dev(bits, dev)
    plan = ops.build_matrix_plan(rp, col, w, out_row, shared=True)
    assert isinstance(plan, kind)
    ops.round_bf16(pin, pout, plan, N, ops.MODE_MATRIX)
    got = pout.cpu().view(torch.int16).numpy().view(np.uint16)
    untouched = np.ones(got.shape, bool)
    untouched[out_row, :N] = False
    assert (got[untouched] == SENTINEL).all()
    return got[:, :N]


@pytest.mark.parametrize("name,layout", [(c, "16-B lanes") for c in CASES] + [("complete33", k) for k in list(LAYOUTS)[1:]])
def test_round_within_the_bound(cuda, name, layout):
    """Class rows in the bound and bit-identical, rest rows FMA mode's bits; complete33 on every lane width."""
    rp, col, w, out_row, pool_rows, classes, rest = case(name)
    bits = mx.pool_bits(pool_rows, N, seed=43, correlated=name == "per_source")
    got = _run(cuda, bits, rp, col, w, out_row, layout)
    print("error / bound:", mx.check_bound(got[out_row], *mx.reference(bits, rp, col, w)))
    for rows in classes:
        assert (got[out_row[rows]] == got[out_row[rows[0]]]).all()
    fma = oracle.round_bf16(bits, rp, col, w, out_row, exact=False)
    assert np.array_equal(got[out_row[rest]], fma[out_row[rest]])


@pytest.mark.parametrize("variant,kind", [("row", ops.SharedPlan), ("operand", object)])
def test_exact_sums_bit_for_bit(cuda, variant, kind):
    """complete300 on small integers: the store's rounding is the only one (mx.exact_case), ties included."""
    bits, rp, col, w, out_row, want = mx.exact_case("complete300", variant, N)
    got = _run(cuda, bits, rp, col, w, out_row, kind=kind)
    wrong = got[out_row] != want
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:8].tolist())


def test_non_finite_elements_are_fma_modes(cuda):
    """One class of three rows, weight 1.0.  Source 1 holds +inf, NaN and -inf; in column 257 the canonical
    chain 3e38 + 3e38 - 3e38 overflows while rows 0 and 1, in their own order, stay finite."""
    rp, col, w, out_row = [0, 3, 6, 9], np.array([1, 2, 0, 0, 2, 1, 0, 1, 2]), np.ones(9), np.arange(3, dtype=np.int32)
    x = oracle.bf16_to_f32(mx.pool_bits(3, N, seed=53)).copy()
    special = [20, 150, 257, 300]
    x[1, [20, 150, 300]] = [np.inf, np.nan, -np.inf]
    x[:, 257] = [3e38, 3e38, -3e38]
    bits = oracle.f32_to_bf16(x)
    got = _run(cuda, bits, rp, col, w, out_row)
    fma = oracle.round_bf16(bits, rp, col, w, out_row, exact=False)
    assert np.isfinite(oracle.bf16_to_f32(fma[:, 257])).tolist() == [True, True, False]
    assert np.array_equal(got[:, special], fma[:, special])  # FMA mode's bits in every row
    keep = np.setdiff1d(np.arange(N), special)
    mx.check_bound(*(a[:, keep] for a in (got, *mx.reference(bits, rp, col, w))))


def test_executor_shared(cuda):
    """The barbell: b16 within the bound, int64 the oracle's; shared=False still builds a MatrixPlan."""
    rp, col, w, out_row, rows, _, _ = case("barbell")
    orders = [col[rp[r]: rp[r + 1]].tolist() for r in range(rows)]
    weights = [w[rp[r]: rp[r + 1]].tolist() for r in range(rows)]
    bits = mx.pool_bits(rows, N, seed=59)
    counts = np.arange(1000, 1000 + rows, dtype=np.int64).reshape(rows, 1)
    pool = ModelPool(StateLayout.from_layout([("w", (N,), "bfloat16"), ("count", (), "int64")]), rows, cuda)
    pool.b16[:, :N] = _dev(bits, cuda)
    pool.i64[:, :1] = torch.from_numpy(counts).to(cuda)
    ex = RoundExecutor(pool, mode=ops.MODE_MATRIX, shared=True, placement_trials=1)
    ex.run(orders, weights)
    assert isinstance(ex.plan(orders, weights, list(range(rows))), ops.SharedPlan)
    mx.check_bound(pool.b16[:, :N].cpu().view(torch.int16).numpy().view(np.uint16), *mx.reference(bits, rp, col, w))
    assert np.array_equal(pool.i64[:, :1].cpu().numpy(), oracle.round_i64(counts, rp, col, w, out_row))
    plain = RoundExecutor(pool, mode=ops.MODE_MATRIX, placement_trials=1)
    assert isinstance(plain.plan(orders, weights, list(range(rows))), ops.MatrixPlan)
    with pytest.raises(ValueError, match="MODE_MATRIX"):
        RoundExecutor(pool, mode=ops.MODE_FMA, shared=True)
