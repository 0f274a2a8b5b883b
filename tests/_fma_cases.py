"""Inputs and reference-side checks shared by the fp32 FMA-mode tests (tests/test_host_fma.py,
tests/test_gpu_fma_f32.py).  Everything here is host-side numpy; the reference is
oracle.agg_f32 / oracle.round_f32 with exact=False (pinned by tests/test_oracle_fma.py)."""
import numpy as np

import oracle

# subnormals of either sign (one the smallest), both zeros, a value whose average stays finite
# but whose sum does not, and the largest fp16
SPECIALS = np.array([1e-40, -1e-45, -0.0, 0.0, 3e38, 65504.0], np.float32)
WEIGHT_KINDS = ["random", "uniform", "signed"]


def assert_bits(got, ref, what=None):
    """All bits equal; NaNs at equal positions, their payloads not compared."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ng, nr = np.isnan(got), np.isnan(ref)
    assert np.array_equal(ng, nr), (what, "NaN positions", np.argwhere(ng != nr)[:8].tolist())
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~ng
    if bad.any():
        at = np.argwhere(bad)
        i = tuple(at[0])
        raise AssertionError((what, f"{len(at)} of {bad.size} elements differ, first at {at[:6].tolist()}: "
                                    f"got {got[i]!r} ({got.view(np.uint32)[i]:#010x}), "
                                    f"reference {ref[i]!r} ({ref.view(np.uint32)[i]:#010x})"))


def fused_differs(fused, exact, least=0.10):
    """The condition on the reference alone: over finite elements the fused chain differs from
    the EXACT one in at least `least` of them, so a kernel running EXACT arithmetic in FMA mode
    cannot match the fused reference."""
    fin = np.isfinite(fused) & np.isfinite(exact)
    share = float(np.mean(fused.view(np.uint32)[fin] != exact.view(np.uint32)[fin]))
    assert share >= least, share
    return share


def products_exact(w):
    """Every fp32 weight is 0 or a power of two: each product is then exact unless it is
    subnormal, the fused and the unfused chain agree on ordinary values, and fused_differs has
    nothing to separate (uniform weights 1/m at m = 2, 8, 16, 256)."""
    mant, _ = np.frexp(np.asarray(w, np.float64).astype(np.float32))
    return bool(np.all((np.abs(mant) == 0.5) | (mant == 0)))


def k1_weights(rng, m, kind):
    """normalised random; 1/m; or random with negative and zero entries.  The middle operand
    shares operand 0's weight (the cancelling columns of k1_operands)."""
    if kind == "uniform":
        return [1.0 / m] * m
    w = rng.random(m) + 0.05
    w /= w.sum()
    if kind == "signed":
        w[1::3] *= -1.0
        w[2::5] = 0.0
    w[m // 2] = w[0]
    return [float(v) for v in w]


def k1_operands(rng, m, n):
    """m operands of n elements.  Operand 0 and the middle one carry the special values, an inf
    and a NaN each, and a block of columns where the two cancel (x_mid = -x_0): on powers of two
    against signed zeros from everyone else (an exactly zero sum), and on random values.  Sixteen
    columns hold a small subnormal in every operand.  The last elements (the n % 4 tail) carry a
    -0.0 and two subnormals.  n < 56: only the special values, cycled."""
    x = (rng.standard_normal((m, n)) * 3).astype(np.float32)
    mid = m // 2
    if n < 56:
        e = np.arange(n)
        x[0] = SPECIALS[e % 6]
        x[mid] = SPECIALS[(e + 3) % 6]  # (m = 1: operand 0 again)
        return list(x)
    x[0, 0:6] = SPECIALS
    x[mid, 6:12] = SPECIALS
    x[0, 6:8] = [-0.0, 1e-40]
    x[0, 12], x[mid, 13], x[mid, 14], x[0, 15] = np.inf, np.nan, -np.inf, np.nan
    if m >= 2:
        x[:, 16:24] = np.where((np.arange(m)[:, None] + np.arange(8)[None, :]) % 2, -0.0, 0.0)
        x[0, 16:24] = 2.0 ** np.arange(-4, 4)
        x[0, 24:32] = rng.standard_normal(8) * 3
        x[mid, 16:32] = -x[0, 16:32]
    # every operand a small subnormal k * 2^-149, k an odd number times 2^t: with a weight 2^-(t+1)
    # the product lies halfway between two subnormals, the unfused chain rounds it to even on its
    # own and the fused one together with the accumulator, so the two modes differ here even
    # with power-of-two weights (1/m at m = 2, 8, 16, 256)
    k = (2 * rng.integers(0, 50, (m, 16)) + 1) << rng.integers(0, 9, (m, 16))
    x[:, 32:48] = (k * rng.choice([-1, 1], (m, 16)) * 2.0 ** -149).astype(np.float32)
    x[0, n - 1], x[mid, n - 2], x[m - 1, n - 3] = -0.0, 1e-40, -1e-45
    return list(x)


def round_pool(rng, n_src, n, orders):
    """[n_src, n] pool for a round over `orders` (n >= 48) and the source that carries the
    non-finite values.
      columns 0-5    every source a special value, rotated by its row
      columns 6-11   every third source the same special value, the others ordinary
      columns 12-13  -0.0 in every source;  14-15 +0 / -0 mixed by row
      columns 16-21  sources cancel in pairs (even rows v, odd rows -v; 16-19 powers of two)
      columns 22-24  +inf, NaN, -inf in ONE source that only some rows name (the one named by
                     the fewest rows): a masked or padded slot that multiplied it in would
                     leak 0 * inf = NaN into rows that do not name it
      the last seven columns (a partial tile's end and the n % 4 tail): -0.0 in every source,
      mixed zeros, a subnormal."""
    assert n >= 48
    x = (rng.standard_normal((n_src, n)) * 3).astype(np.float32)
    r = np.arange(n_src)
    x[:, 0:6] = SPECIALS[(r[:, None] + np.arange(6)[None, :]) % 6]
    x[0::3, 6:12] = SPECIALS
    x[:, 12:14] = -0.0
    x[:, 14] = np.where(r % 2, -0.0, 0.0)
    x[:, 15] = np.where(r % 3, 0.0, -0.0)
    v = np.concatenate([2.0 ** np.arange(-2, 2), rng.standard_normal(2) * 3]).astype(np.float32)
    x[:, 16:22] = np.where(r[:, None] % 2, -v, v)
    uses = np.zeros(n_src, np.int64)
    for o in orders:
        uses[np.unique(o)] += 1
    named = np.flatnonzero(uses > 0)
    hot = int(named[np.argmin(uses[named])])
    x[hot, 22:25] = [np.inf, np.nan, -np.inf]
    x[:, n - 7] = 1e-40
    x[:, n - 6:n - 4] = -0.0
    x[:, n - 4] = np.where(r % 2, 0.0, -0.0)
    x[:, n - 3] = np.where(r % 3, -0.0, 0.0)
    x[:, n - 2:] = -0.0
    return x, hot


class RoundCase:
    """A round (orders, weights, output rows), its pool and the fused reference; built once per
    test, with the conditions that hold on the reference alone asserted here."""

    def __init__(self, orders, ws, out_rows, n_src, n, seed):
        from oracle import reference_alg as ra

        self.orders, self.ws, self.n = orders, ws, n
        self.row_ptr, self.col, self.w = ra.round_csr(orders, ws)
        self.out_rows = np.asarray(out_rows, np.int32)
        self.pool, self.hot = round_pool(np.random.default_rng(seed), n_src, n, orders)
        self.csr = (self.row_ptr, self.col, self.w, self.out_rows)
        self.ref = oracle.round_f32(self.pool, *self.csr, exact=False)
        exact = oracle.round_f32(self.pool, *self.csr)
        multi = [int(self.out_rows[i]) for i, o in enumerate(orders) if len(o) >= 2]
        self.share = fused_differs(self.ref[multi], exact[multi])
        # the non-finite source reaches exactly the rows that name it
        names = np.array([self.hot in o for o in orders])
        hit = self.ref[self.out_rows][:, 22:25]
        assert np.isfinite(hit[~names]).all()
        if names.any():
            assert np.isnan(hit[names][:, 1]).all()
        self.spared = int((~names).sum())

    def check(self, got, what=None):
        """got: [n_src, >= n] pool after the round (started as a copy of the input pool)."""
        got = np.asarray(got)
        assert_bits(got[:, :self.n], self.ref, what)
        names = np.array([self.hot in o for o in self.orders])
        assert np.isfinite(got[self.out_rows[~names]][:, 22:25]).all(), (what, "0 * inf leaked into a row")
