"""Shared by the matrix-round tests (tests/test_matrix_plan_host.py, tests/test_gpu_matrix_round.py):
the rounds, their bf16 inputs, the float64 reference and tal_agg.h's K3m error bound."""
import networkx as nx
import numpy as np

import oracle
from topology_aware_learning_amd import ops

GRAPHS = ("ring8", "rr40x5", "sbm3x24", "complete33", "complete_chunk+1")
WEIGHTS = ("unweighted", "positive", "signed")
BF16_OVERFLOW = 2.0 ** 128 - 2.0 ** 119  # from here on a value rounds to a bf16 infinity


def graph(name):
    return {"ring8": lambda: nx.cycle_graph(8),  # a partial row tile and a partial k-block
            "rr40x5": lambda: nx.random_regular_graph(5, 40, seed=2),  # two row tiles
            "sbm3x24": lambda: nx.stochastic_block_model(  # three tiles, more than 64 sources: two chunks
                [24] * 3, np.full((3, 3), 0.05) + np.eye(3) * 0.5, seed=3),
            "complete33": lambda: nx.complete_graph(33),  # k padding 33 -> 48
            # one source more than an LDS chunk: the accumulators cross a chunk boundary
            "complete_chunk+1": lambda: nx.complete_graph(ops.MATRIX_CHUNK + 1)}[name]()


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
