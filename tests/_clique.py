"""Helpers shared by the GPU clique tests (tests/test_gpu_clique_*.py): pools as storage bits
(uint32 for fp32, uint16 for bf16), the per-source weight kinds, the oracle round of either
storage type, bitwise comparison, and counters on the library's entries."""
import networkx as nx
import numpy as np
import torch

import oracle
from topology_aware_learning_amd import _lib, ops
from topology_aware_learning_amd import weights as tw

MODES = [ops.MODE_EXACT, ops.MODE_FMA]
SPECIALS = [1e-40, -0.0, 3.3e38, -1e-45, 65504.0, 1.17e-38, -3.3e38, 2.0 ** -133, 0.0, 1.0, -1.0, 3.0e38]


def np_dtype(bf16):
    return np.uint16 if bf16 else np.uint32


def tdtype(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def to_dev(bits, bf16, dev):
    """Host bit array -> device tensor of the storage type."""
    a = np.ascontiguousarray(bits)
    return torch.from_numpy(a.view(np.int16 if bf16 else np.int32)).view(tdtype(bf16)).to(dev)


def bits(t):
    """Device tensor of either storage type -> host bit array."""
    bf16 = t.dtype == torch.bfloat16
    return t.cpu().contiguous().view(torch.int16 if bf16 else torch.int32).numpy().view(np_dtype(bf16))


def sentinel_pool(rows, ld, bf16, dev, sentinel):
    """An output pool whose every element holds the bits `sentinel`."""
    return to_dev(np.full((rows, ld), sentinel, np_dtype(bf16)), bf16, dev)


def inputs(rows, n, seed, bf16, by_row=False):
    """Pool bits [rows, n].  Row 0: the specials (n > 12); member 1 holds a payload NaN in one
    column; a column of -0.0; +inf / -inf in every third row of another.  by_row: the values
    drawn one row at a time (a row's specials then replace its first twelve draws) instead of
    the matrix at once."""
    rng = np.random.default_rng(seed)
    if by_row:
        x = np.stack([(rng.standard_normal(n) * 3.0).astype(np.float32) for _ in range(rows)])
    else:
        x = (rng.standard_normal((rows, n)) * 3.0).astype(np.float32)
    if n > 12:
        x[0, :12] = SPECIALS
    pool = oracle.f32_to_bf16(x) if bf16 else x.view(np.uint32).copy()
    nan_col = 3 if n > 3 else 0
    pool[1, nan_col] = 0x7FC1 if bf16 else 0x7FC00001
    if n > 5:
        pool[:, 5] = 0x8000 if bf16 else 0x80000000
    if n > 6:
        pool[::3, 6] = 0x7F80 if bf16 else 0x7F800000
        pool[3::6, 6] = 0xFF80 if bf16 else 0xFF800000
    return pool, nan_col


def padded(pool, bf16, dev, odd=False):
    """Device copy with a padded row stride: even for K3c's column pairs, odd on purpose where a
    plan holds K3c1 blocks alone (no column-pair rule there)."""
    rows, n = pool.shape
    ld = n + 2 + ((n + odd) % 2)
    assert ld % 2 == int(odd)
    pin = torch.zeros(rows, ld, dtype=tdtype(bf16), device=dev)
    pin[:, :n] = to_dev(pool, bf16, dev)
    return pin


def oracle_round(pool, csr, out_rows, bf16, exact=True, pool_out=None):
    """The C oracle's round of the mode on pool bits, as bits."""
    row_ptr, col, w = csr
    if bf16:
        return oracle.round_bf16(pool, row_ptr, col, w, out_rows, pool_out=pool_out, exact=exact)
    out = oracle.round_f32(pool.view(np.float32), row_ptr, col, w, out_rows,
                           pool_out=None if pool_out is None else pool_out.view(np.float32), exact=exact)
    return out.view(np.uint32)


def same(got, ref, nan_payloads_free):
    """Bit for bit.  nan_payloads_free: NaNs must sit in the same places and every other value
    agree in every bit - for fp32 results held against the C oracle on the CPU, whose NaNs carry
    x86's payloads (inf - inf is 0xFFC00000 there, 0x7FC00000 on the GPU)."""
    if not nan_payloads_free:
        return np.array_equal(got, ref)
    ng, nr = np.isnan(got.view(np.float32)), np.isnan(ref.view(np.float32))
    return np.array_equal(ng, nr) and np.array_equal(got[~ng], ref[~nr])


def is_nan(b, bf16):
    return b == 0xFFFF if bf16 else np.isnan(np.array([b], np.uint32).view(np.float32))[0]


def run(pin, pout, plan, n, mode):
    (ops.round_bf16 if pin.dtype == torch.bfloat16 else ops.round_f32)(pin, pout, plan, n=n, mode=mode)


def k1_fma(pin, orders, ws, r, n):
    """Row r of the round by one K1 call in FMA mode on the device pool, as bits."""
    chk = torch.empty(n, dtype=pin.dtype, device=pin.device)
    (ops.agg_bf16 if pin.dtype == torch.bfloat16 else ops.agg_f32)([pin[j, :n] for j in orders[r]], ws[r], chk,
                                                                  mode=ops.MODE_FMA)
    return bits(chk)


def round_of(g, kind, who=None, n=0):
    """(orders, weights) of graph g for the rows `who` (default: every node).  "uniform": 1 / len,
    negative for odd n; "datasize": data-size weights, every source distinct; "degcent": softmax
    of 10 x the degree centrality; "signed": hand-made signed weights per source, some exactly 0.
    The last three are the same for a source in every row that reads it, so the clique rows form
    per-source blocks."""
    nodes = sorted(g.nodes)
    orders = [sorted(g.neighbors(i)) + [i] for i in (nodes if who is None else who)]
    if kind == "uniform":
        sign = -1.0 if n % 2 else 1.0
        return orders, [[sign / len(o)] * len(o) for o in orders]
    if kind == "datasize":
        lens = (np.random.default_rng(5).permutation(len(nodes)) * 37 + 101).tolist()  # all distinct
        return orders, [tw.weighted([lens[j] for j in o]) for o in orders]
    if kind == "degcent":
        cent = nx.degree_centrality(g)
        return orders, [tw.centrality(o, cent, True, 10.0) for o in orders]
    per = [0.0 if j % 7 == 3 else ((-1.0) ** j) * (0.013 * (j % 11) + 0.002) for j in nodes]
    return orders, [[per[j] for j in o] for o in orders]


class Counter:
    """A library entry point wrapped in a counting Python callable."""

    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *args):
        self.calls += 1
        return self.fn(*args)


def count(monkeypatch, name):
    L = _lib.load()
    c = Counter(getattr(L, name))
    monkeypatch.setattr(L, name, c)
    return c
