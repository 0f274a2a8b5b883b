"""The launch layer's compile-time choices on the GPU, at their edges: every step of the MMAX
ladders of K3c (16 .. 64) and K3c1 (68 .. 128) from the block size just below and just above it,
and the tail kernels' EXACT choice (k_round_direct, k_round_stream_scalar, k_round_tiled_scalar)
on every storage type.  Bit for bit against the C oracle (EXACT) and K1 in FMA mode."""
import networkx as nx
import numpy as np
import pytest
import torch

import oracle
from oracle import reference_alg as ra
from topology_aware_learning_amd import ops

from _clique import MODES, bits, inputs, k1_fma, oracle_round, padded, round_of, run, same, sentinel_pool

pytestmark = pytest.mark.gpu

SENTINEL = {False: 0x40E01234, True: 0x1234}  # fp32 / bf16 bits of an untouched output element
N = 259  # odd: K3c's pair kernel, both last-column tails, and a second 256-thread workgroup

_K3C = (16, 17, 32, 33, 40, 41, 48, 49, 56, 57, 60, 61, 64)
_K3C1 = (65, 68, 69, 84, 85, 100, 101, 116, 117, 128)
_KINDS = {"uniform": dict(max_members=128),
          "datasize": dict(per_source=True, max_members=128, wide_per_source=True)}  # one weight per source


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", list(_KINDS))
@pytest.mark.parametrize("m", _K3C + _K3C1)
def test_mmax_ladder_edges(cuda, m, kind, bf16):
    """The complete graph on m clients as one block whose mmax is m: EXACT is the oracle's round,
    FMA is K1's chain on the first, a middle and the last row, and nothing but the round's rows
    and columns is written (output rows permuted and shifted by 2, a padded stride)."""
    orders, ws = round_of(nx.complete_graph(m), kind, n=N)
    csr = ra.round_csr(orders, ws)
    out_rows = (np.random.default_rng(m).permutation(m) + 2).astype(np.int32)
    plan = ops.build_clique_plan(*csr, out_rows, bf16=bf16, **_KINDS[kind])
    assert plan is not None and plan.rest is None
    wide = m > ops.CLIQUE_MAX
    assert (plan.n_cliques, plan.n_col) == ((0, 1) if wide else (1, 0))
    assert (plan.col_mmax if wide else plan.mmax) == m
    assert ((plan.col_wtable if wide else plan.wtable) is not None) == (kind == "datasize")
    pool, _ = inputs(m, N, m + N, bf16)
    pin = padded(pool, bf16, cuda, odd=wide)
    for mode in MODES:
        pout = sentinel_pool(m + 2, pin.shape[1], bf16, cuda, SENTINEL[bf16])
        run(pin, pout, plan, N, mode)
        got = bits(pout)
        if mode == ops.MODE_EXACT:
            assert same(got[2:, :N], oracle_round(pool, csr, out_rows - 2, bf16), not bf16), mode
        else:
            for r in (0, m // 2, m - 1):
                assert same(got[out_rows[r], :N], k1_fma(pin, orders, ws, r, N), not bf16), r
        assert np.all(got[:2] == SENTINEL[bf16]) and np.all(got[:, N:] == SENTINEL[bf16])  # nothing else written


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", ["f32", "bf16", "i64"])
def test_tail_kernels_of_a_streamed_plan(cuda, dt, mode):
    """n = 7 under a row stride of 10 elements: no float4 column, every column is the tail
    kernels'.  Out of place (3 groups of 4 rows): k_round_direct.  In place (one group): fp32 and
    int64 run k_round_stream_scalar, bf16 (which has no streamed kernels) k_round_tiled_scalar.
    All against the oracle's round of the mode (int64 has one)."""
    n, bf16 = 7, dt == "bf16"
    orders, ws = round_of(nx.cycle_graph(12), "signed")
    csr = ra.round_csr(orders, ws)
    out_rows = np.arange(12, dtype=np.int32)
    if dt == "i64":
        pool = np.random.default_rng(7).integers(-10 ** 6, 10 ** 6, size=(12, n)).astype(np.int64)
        ref = oracle.round_i64(pool, *csr, out_rows)
        pin = torch.zeros(12, 10, dtype=torch.int64, device=cuda)
        pin[:, :n] = torch.from_numpy(pool).to(cuda)
        rnd, host, nan_free = (lambda a, b, p: ops.round_i64(a, b, p, n=n)), (lambda t: t.cpu().numpy()), False
    else:
        pool, _ = inputs(12, n, 12 + n, bf16)
        ref = oracle_round(pool, csr, out_rows, bf16, exact=(mode == ops.MODE_EXACT))
        pin = padded(pool, bf16, cuda)
        rnd, host, nan_free = (lambda a, b, p: run(a, b, p, n, mode)), bits, not bf16
    assert pin.shape[1] == 10
    grouped = ops.build_stream_plan(*csr, out_rows, 4, 0)
    assert grouped.info.n_groups == 3 and grouped.info.max_rows == 4 and grouped.info.stream_cs > 0
    pout = torch.full_like(pin, 77)
    untouched = host(pout)
    rnd(pin, pout, grouped)
    got = host(pout)
    assert same(got[:, :n], ref, nan_free) and np.array_equal(got[:, n:], untouched[:, n:])
    single = ops.build_stream_plan(*csr, out_rows, 64, 0)
    assert single.single_group and single.info.stream_cs > 0
    rnd(pin, pin, single)
    got = host(pin)
    assert same(got[:, :n], ref, nan_free) and not got[:, n:].any()
