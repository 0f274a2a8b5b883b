"""tests/_prox_oracle.py pinned on the CPU: the float32 gradient chain against float64 within the
rounding it is allowed, against torch's CPU autograd of the reference's loop, its deliberate
properties (identical neighbor, zero norm, sign of the scale), and that the order of the sum
shows in the bits - so a kernel that sums in another order cannot match it by accident."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from _prox_oracle import grad_chain, norms64, to_bf16_bits

U = 2.0 ** -24  # unit roundoff of float32


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _case(k, segs, n, seed, wide=False, identical=True):
    """Client row and k neighbor rows (float32, randn; `wide`: scaled by 2^e, e in [-20, 20]);
    with `identical`, neighbor 1 equals the client."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((k + 1, n)).astype(np.float32)
    if wide:
        x = x * np.exp2(rng.integers(-20, 21, (k + 1, n))).astype(np.float32)
    if identical and k >= 2:
        x[2] = x[0]
    return x[0], [x[1 + t] for t in range(k)]


SEGS = [(1, 1), (5, 3), (11, 257), (271, 1030)]
N = 1305
INSIDE = np.zeros(N, dtype=bool)
for _o, _n in SEGS:
    INSIDE[_o: _o + _n] = True


@pytest.mark.parametrize("wide", [False, True], ids=["randn", "wide"])
@pytest.mark.parametrize("k", [1, 2, 9, 65])
@pytest.mark.parametrize("scale", [0.37, -2.5])
def test_grad_chain_against_float64(k, scale, wide):
    """gw: |err| <= (k + 2) u sum_t |d_t| (one rounding each for the subtraction, the division and
    the product, plus k - 1 additions); gwt_t: |err| <= 3 u |d_t|; d_t in float64 from the same
    float32 norms."""
    w, wts = _case(k, SEGS, N, seed=100 * k + int(wide), wide=wide)
    norms = norms64(w, wts, SEGS).astype(np.float32)
    s = np.float32(scale)
    gw, gwt = grad_chain(w, wts, SEGS, norms, s, [True] * k, sentinel=7.0)
    sum_d, sum_abs = np.zeros(N), np.zeros(N)
    for t in range(k):
        d = np.zeros(N)
        for p, (o, n) in enumerate(SEGS):
            c = float(s) / float(norms[t, p]) if norms[t, p] > 0 else 0.0
            d[o: o + n] = (w[o: o + n].astype(np.float64) - wts[t][o: o + n].astype(np.float64)) * c
        err = np.abs(gwt[t].astype(np.float64) + d)[INSIDE]
        assert (err <= 3 * U * np.abs(d)[INSIDE]).all(), t
        sum_d += d
        sum_abs += np.abs(d)
    err = np.abs(gw.astype(np.float64) - sum_d)[INSIDE]
    assert (err <= (k + 2) * U * sum_abs[INSIDE]).all()
    assert sum_abs[INSIDE].min() > 0
    for x in [gw] + gwt:  # outside the segments: the sentinel
        assert (_bits(x)[~INSIDE] == _bits(np.float32(7.0))).all()


@pytest.mark.parametrize("k,segs,n", [(1, [(0, 7)], 7), (3, [(1, 5), (8, 130)], 140), (70, SEGS, N)],
                         ids=["k1", "k3", "k70"])
def test_against_torch_cpu_autograd(k, segs, n):
    """The reference's loop ((w - wt).norm(2) summed, .backward()) with test_prox_term_matches_
    torch_loop's bounds: value 1e-5 relative + 1e-6, gradients rtol 1e-4, atol 1e-6."""
    w, wts = _case(k, segs, n, seed=7 + k)
    leaves = [[torch.from_numpy(r[o: o + m].copy()).requires_grad_() for o, m in segs] for r in [w] + wts]
    ref = 0.0
    for nb in leaves[1:]:
        for a, b in zip(leaves[0], nb):
            ref = ref + (a - b).norm(2)
    ref.backward()
    n64 = norms64(w, wts, segs)
    ref_v = float(ref.detach())
    assert abs(float(n64.sum()) - ref_v) <= 1e-5 * abs(ref_v) + 1e-6
    gw, gwt = grad_chain(w, wts, segs, n64.astype(np.float32), np.float32(1.0), [True] * k)
    for row, got in zip(leaves, [gw] + gwt):
        for (o, m), leaf in zip(segs, row):
            assert torch.allclose(torch.from_numpy(got[o: o + m]), leaf.grad, rtol=1e-4, atol=1e-6)


def test_identical_neighbor_adds_nothing():
    w, wts = _case(5, SEGS, N, seed=3)
    norms = norms64(w, wts, SEGS).astype(np.float32)
    assert (norms[1] == 0).all() and (np.delete(norms, 1, axis=0) > 0).all()
    gw, gwt = grad_chain(w, wts, SEGS, norms, 0.37, [True] * 5)
    assert (gwt[1][INSIDE] == 0).all()
    without = [t for t in range(5) if t != 1]
    gw4, _ = grad_chain(w, [wts[t] for t in without], SEGS, norms[without], 0.37, [False] * 4)
    assert np.array_equal(_bits(gw)[INSIDE], _bits(gw4)[INSIDE])


def test_zero_norm_means_zero_coefficient():
    """norm == 0 gives c == 0 whatever s is - even where the rows differ (squares that all
    underflowed): no inf, no NaN, zero-valued gradients."""
    w, wts = _case(2, SEGS, N, seed=4, identical=False)
    norms = norms64(w, wts, SEGS).astype(np.float32)
    norms[0, :] = 0.0
    gw, gwt = grad_chain(w, wts, SEGS, norms, -2.5, [True, True])
    assert (gwt[0][INSIDE] == 0).all() and np.isfinite(gw[INSIDE]).all()
    only1, _ = grad_chain(w, wts[1:], SEGS, norms[1:], -2.5, [False])
    assert np.array_equal(_bits(gw)[INSIDE], _bits(only1)[INSIDE])


def test_negative_scale_flips_every_sign_bit():
    w, wts = _case(4, SEGS, N, seed=5, identical=False)  # (a zero norm's c is +0 for either sign)
    norms = norms64(w, wts, SEGS).astype(np.float32)
    gw_pos, pos = grad_chain(w, wts, SEGS, norms, 2.5, [True] * 4)
    gw_neg, neg = grad_chain(w, wts, SEGS, norms, -2.5, [True] * 4)
    for a, b in zip(pos, neg):
        assert ((_bits(a) ^ _bits(b))[INSIDE] == 0x80000000).all()
    assert np.array_equal(gw_neg[INSIDE], -gw_pos[INSIDE])


@pytest.mark.parametrize("k", [3, 9, 65])
def test_order_of_the_sum_shows_in_the_bits(k):
    """The sum begun at d_1, with d_0 one step later ((d_1 + d_2) + d_0 + d_3 + ...; exchanging
    d_0 and d_1 alone is the same sum, addition being commutative), changes bits of gw on inputs
    like the GPU tests': a kernel that sums in another order does not pass them by accident.
    With k = 3 the roundings that differ are the last ones and land elsewhere about every other
    time: a twentieth of the elements is asked for.  With more neighbors the later additions
    absorb most of that difference, so there only some element has to change; the whole sum taken
    downwards from d_{k-1} again ends on other roundings, and a twentieth is asked for."""
    w, wts = _case(k, SEGS, N, seed=6 + k, identical=False)
    norms = norms64(w, wts, SEGS).astype(np.float32)
    gw, gwt = grad_chain(w, wts, SEGS, norms, 0.37, [True] * k)
    gw_c, _ = grad_chain(w, wts, SEGS, norms, 0.37, [True] * k, order=[1, 0] + list(range(2, k)))
    assert np.array_equal(_bits(gw), _bits(gw_c))
    order = [1, 2, 0] + list(range(3, k))
    gw_r, gwt_r = grad_chain(w, wts, SEGS, norms, 0.37, [True] * k, order=order)
    changed = int((_bits(gw) != _bits(gw_r))[INSIDE].sum())
    print(f"k={k}: {changed} of {int(INSIDE.sum())} elements change")
    assert changed >= (INSIDE.sum() // 20 if k == 3 else 1)
    gw_d, _ = grad_chain(w, wts, SEGS, norms, 0.37, [True] * k, order=list(range(k - 1, -1, -1)))
    down = int((_bits(gw) != _bits(gw_d))[INSIDE].sum())
    print(f"k={k}: {down} of {int(INSIDE.sum())} elements change with the sum taken downwards")
    assert down >= INSIDE.sum() // 20
    for a, b in zip(gwt, gwt_r):  # the per-neighbor gradients do not depend on the order
        assert np.array_equal(_bits(a)[INSIDE], _bits(b)[INSIDE])


def test_to_bf16_bits_rounds_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.0], dtype=np.float32)
    assert to_bf16_bits(x).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0x8000]
