"""TEST INFRASTRUCTURE - a plain restatement of the K4 (FedProx) arithmetic, numpy only.

include/tal_agg.h fixes what tal_prox_norms / tal_prox_grad and their bf16 twins compute on flat
rows cut into (offset, length) segments, one per parameter tensor p, against k neighbor rows t:

    norm[t, p] = sqrt(sum_e (w[e] - wt_t[e])^2)
    c[t, p]    = norm[t, p] > 0 ? s / norm[t, p] : 0
    d_t[e]     = (w[e] - wt_t[e]) * c[t, p]
    gw[e]      = ((0 + d_0[e]) + d_1[e]) + ...          gwt_t[e] = -d_t[e]

`norms64` is the high-precision truth of the first line.  `grad_chain` is the other three in
np.float32, one IEEE operation per step (numpy never fuses a multiply into an add), so for the
norms a kernel itself produced its result is what the kernel must write, all 32 bits.  Nothing
here imports the package under test; tests/test_prox_oracle.py pins this file on the CPU.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np


def norms64(w, wts, segs) -> np.ndarray:
    """float64 [k, n_seg]: sqrt(sum((w - wt_t)^2)) over each (offset, length) segment."""
    w = np.asarray(w, dtype=np.float64)
    out = np.empty((len(wts), len(segs)), dtype=np.float64)
    for t, wt in enumerate(wts):
        d = w - np.asarray(wt, dtype=np.float64)
        for p, (o, n) in enumerate(segs):
            out[t, p] = np.sqrt(np.sum(d[o: o + n] ** 2))
    return out


def grad_chain(w, wts, segs, norms_f32, scale_f32, want_t, sentinel=np.nan,
               order: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, List[Optional[np.ndarray]]]:
    """The header's gradient chain in float32.  w: float32 row, wts: k float32 rows, norms_f32:
    [k, n_seg], want_t: k booleans.  Returns (gw, gwt): float32 rows of w's length, gwt[t] None
    where want_t[t] is false; every position outside the segments holds `sentinel`.  `order`
    (a permutation of range(k), default 0, 1, ..., k - 1) is the order of the sum: only the
    sensitivity check of tests/test_prox_oracle.py passes another one."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    wts = [np.ascontiguousarray(x, dtype=np.float32) for x in wts]
    k = len(wts)
    norms = np.asarray(norms_f32, dtype=np.float32).reshape(k, len(segs))
    s = np.float32(scale_f32)
    assert len(want_t) == k and all(x.shape == w.shape for x in wts)
    order = list(range(k)) if order is None else list(order)
    assert sorted(order) == list(range(k))
    gw = np.full(w.shape, sentinel, dtype=np.float32)
    gwt = [np.full(w.shape, sentinel, dtype=np.float32) if wnt else None for wnt in want_t]
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        for p, (o, n) in enumerate(segs):
            ws = w[o: o + n]
            g = np.zeros(n, dtype=np.float32)  # +0.0f
            for t in order:
                nrm = norms[t, p]
                c = s / nrm if nrm > zero else zero  # np.float32 / np.float32: one IEEE division
                assert isinstance(c, np.float32)
                d = (ws - wts[t][o: o + n]) * c
                g = g + d
                if gwt[t] is not None:
                    gwt[t][o: o + n] = -d
            gw[o: o + n] = g
    assert gw.dtype == np.float32
    return gw, gwt


def to_bf16_bits(x) -> np.ndarray:
    """The bf16 twins' round-once store: float32 -> bf16 bit patterns (uint16), to nearest even."""
    import oracle

    return oracle.f32_to_bf16(x)
