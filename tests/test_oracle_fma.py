"""The fp32 FMA-mode oracle (oracle.agg_f32 / round_f32 with exact=False) pinned on the CPU.

The reference has no FMA mode, so there is no golden file to pin it with.  The definition in
include/tal_agg.h is pinned by exact arithmetic instead: per element
    acc = fl(w_0 * x_0);  acc = fma(w_i, x_i, acc)  for i = 1..m-1, in operand order,
each step computed here with fractions.Fraction and rounded to the nearest-even fp32 by integer
arithmetic (never through float64: that would round twice), subnormals kept, overflow to inf,
and an exactly zero sum signed by the IEEE rule (equal signs keep theirs, otherwise +0).
"""
from fractions import Fraction

import numpy as np
import pytest

import oracle

_INF = 0x7F800000
_SIGN = 0x80000000


def _decode(bits: int):
    """fp32 bits of a finite value -> (Fraction, sign bit)."""
    s, e, f = bits >> 31, (bits >> 23) & 0xFF, bits & 0x7FFFFF
    assert e != 0xFF
    mag = Fraction(f, 1 << 149) if e == 0 else Fraction((1 << 23) | f, 1) * Fraction(2) ** (e - 150)
    return (-mag if s else mag), s


def _round_f32(q: Fraction) -> int:
    """Nearest-even fp32 bits of a nonzero exact value."""
    s = _SIGN if q < 0 else 0
    a = -q if q < 0 else q
    e = a.numerator.bit_length() - a.denominator.bit_length()  # 2^(e-1) < a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    e = max(e, -126)  # subnormals share the smallest normal's quantum
    k = a / Fraction(2) ** (e - 23)
    fl = k.numerator // k.denominator
    rem = k - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl & 1):
        fl += 1
    if fl == 1 << 24:
        fl, e = 1 << 23, e + 1
    if fl == 0:
        return s  # underflow to a zero of the value's sign
    if fl < 1 << 23:
        assert e == -126
        return s | fl  # subnormal
    if e + 127 >= 255:
        return s | _INF
    return s | ((e + 127) << 23) | (fl - (1 << 23))


def _chain(wbits, xbits, seen):
    """The fused chain on fp32 bit patterns of finite weights and operands; records in `seen`
    the classes of arithmetic it went through."""
    acc = None
    for i, (wb, xb) in enumerate(zip(wbits, xbits)):
        (w, ws), (x, xs) = _decode(wb), _decode(xb)
        if ws and w != 0:
            seen.add("negative weight")
        if w == 0:
            seen.add("zero weight")
        p, ps = w * x, ws ^ xs
        if p != 0 and abs(p) < Fraction(1, 1 << 126):
            seen.add("subnormal product")
        if i == 0:
            acc = _round_f32(p) if p != 0 else (_SIGN if ps else 0)
            continue
        if acc & 0x7FFFFFFF == _INF:  # finite w * x never moves an infinity
            continue
        a, asg = _decode(acc)
        t = p + a
        if t != 0:
            acc = _round_f32(t)
        else:
            if p != 0:
                seen.add("exact cancellation")
            acc = (_SIGN if ps else 0) if (p == 0 and a == 0 and ps == asg) else 0
    if acc & 0x7FFFFFFF == _INF:
        seen.add("overflow")
    elif acc == 0:
        seen.add("+0 result")
    elif acc == _SIGN:
        seen.add("-0 result")
    elif acc & 0x7F800000 == 0:
        seen.add("subnormal sum")
    return acc


def _inputs(m, rng):
    """(xs [m, n] fp32, w [m] float64): column blocks that drive the chain through ordinary
    values, subnormal products and sums, overflow, exact cancellation, both zeros, and negative
    and zero weights."""
    blk = 48
    cols = []
    w = rng.random(m)
    w = w / w.sum() * (2.5 if m % 2 else 1.0)  # odd m: weights past 1, so sums of large operands overflow
    if m >= 2:
        w[1] = -w[1]
    if m >= 3:
        w[2] = 0.0
    if m >= 4:
        w[0] = w[3] = 0.25  # a power of two: its products are exact, so x and -x cancel exactly
    cols.append(rng.standard_normal((m, blk)) * 3)                                  # ordinary
    cols.append(rng.standard_normal((m, blk)) * 3e-38)                              # subnormal products and sums
    cols.append(rng.standard_normal((m, blk)) * 1e-42)                              # subnormal operands
    cols.append(np.abs(rng.standard_normal((m, blk))) * 1e38 + 2.5e38)              # large: sums overflow
    cols.append(rng.standard_normal((m, blk)) * 3e38)                               # large, mixed signs
    c = rng.standard_normal((m, blk)) * 3
    if m >= 4:  # operand 3 cancels operand 0 (equal weights 0.25); the rest contribute zeros
        c[1:] = 0.0
        c[3] = -c[0]
        c[1, ::2] = -0.0
    cols.append(c)
    z = np.zeros((m, blk))
    z[:, : blk // 2] = -0.0                                                         # every product a signed zero
    z[rng.random((m, blk)) < 0.3] *= -1
    cols.append(z)
    t = np.where(rng.random((m, blk)) < 0.5, -1e-45, 1e-45)                         # products underflow to +-0
    cols.append(t)
    x = np.clip(np.concatenate(cols, axis=1), -3.4e38, 3.4e38).astype(np.float32)  # operands stay finite
    if m == 1:
        w[0] = -0.75
    return x, w


_M = list(range(1, 10))


@pytest.fixture(scope="module")
def chains():
    """For every m: inputs, the oracle's two fused results and the exact-arithmetic bits."""
    rng = np.random.default_rng(2024)
    out, seen = {}, set()
    for m in _M:
        x, w = _inputs(m, rng)
        wbits = [int(b) for b in w.astype(np.float32).view(np.uint32)]
        xb = x.view(np.uint32)
        want = np.array([_chain(wbits, [int(b) for b in xb[:, e]], seen) for e in range(x.shape[1])], np.uint32)
        agg = oracle.agg_f32(list(x), w, exact=False)
        rnd = oracle.round_f32(x, [0, m], np.arange(m), w, [0], pool_out=np.zeros((1, x.shape[1]), np.float32),
                               exact=False)[0]
        out[m] = (x, w, want, agg, rnd)
    return out, seen


def test_fused_chain_is_the_exact_definition(chains):
    out, _ = chains
    total = 0
    for m, (x, w, want, agg, rnd) in out.items():
        bad = np.flatnonzero(agg.view(np.uint32) != want)
        assert bad.size == 0, (m, bad[:8], agg.view(np.uint32)[bad[:8]], want[bad[:8]])
        total += want.size
    assert total >= 3000


def test_inputs_reach_every_class(chains):
    _, seen = chains
    assert seen >= {"subnormal product", "subnormal sum", "overflow", "exact cancellation", "+0 result",
                    "-0 result", "negative weight", "zero weight"}, seen


def test_agg_and_round_agree(chains):
    out, _ = chains
    for m, (x, w, want, agg, rnd) in out.items():
        assert np.array_equal(agg.view(np.uint32), rnd.view(np.uint32)), m


def test_default_stays_exact():
    """exact defaults to True: callers that pass nothing keep the reference's arithmetic."""
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((5, 1000)) * 3).astype(np.float32)
    w = rng.random(5)
    a, b = oracle.agg_f32(list(x), w), oracle.agg_f32(list(x), w, exact=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    acc = np.float32(w[0]) * x[0]
    for i in range(1, 5):
        acc = acc + np.float32(w[i]) * x[i]
    assert np.array_equal(a.view(np.uint32), acc.view(np.uint32))
    r = oracle.round_f32(x, [0, 5], np.arange(5), w, [2])
    assert np.array_equal(r[2].view(np.uint32), a.view(np.uint32))


@pytest.mark.parametrize("m", [2, 3, 5, 9, 65])
def test_fused_differs_from_exact_on_ordinary_inputs(m):
    """The two modes are different functions: on standard-normal x 3 operands and normalised
    random weights at least 10 % of the elements differ in a bit (two operands: about 17 %)."""
    rng = np.random.default_rng(m)
    x = (rng.standard_normal((m, 20000)) * 3).astype(np.float32)
    w = rng.random(m)
    w /= w.sum()
    ex = oracle.agg_f32(list(x), w)
    fu = oracle.agg_f32(list(x), w, exact=False)
    share = np.mean(ex.view(np.uint32) != fu.view(np.uint32))
    assert share >= 0.10, share
    rex = oracle.round_f32(x, [0, m], np.arange(m), w, [0])[0]
    rfu = oracle.round_f32(x, [0, m], np.arange(m), w, [0], exact=False)[0]
    assert np.array_equal(rex.view(np.uint32), ex.view(np.uint32))
    assert np.array_equal(rfu.view(np.uint32), fu.view(np.uint32))
