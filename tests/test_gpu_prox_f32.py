"""K4 on fp32 rows (tal_prox_norms, tal_prox_grad) on the GPU, against tests/_prox_oracle.py.

Kernel level, through ctypes on flat float32 rows with a plan of explicit (offset, length)
segments at odd offsets with gaps: one element, one 256-lane stride and its neighbors, one
8192-element chunk and its neighbors, three chunks of one segment; 1 to 129 neighbors (the
8-neighbor tile, the 64-neighbor launch and a third launch), with some neighbor gradients not
asked for in every launch.

The norms against float64, relative 32 * 2^-24.  With u = 2^-24: the subtraction puts 2u on
d^2; a lane's chain is at most 32 fmaf of non-negative terms, 32u; lanes, wavefronts and chunks
are summed in double; the sqrt halves the error, 17u; the cast to fp32 adds u: 18u to first
order, the rest is margin for second-order terms and the double sqrt.  An identical neighbor's
norms are exactly 0, a second call gives the same bits, and the scratch is exactly
tal_prox_scratch_bytes long between two guard regions.

The gradient, for the kernel's own norms, all 32 bits of grad_chain (include/tal_agg.h's chain:
c_t = norm_t > 0 ? s / norm_t : 0, d_t = (w - wt_t) * c_t, g = ((0 + d_0) + d_1) + ...,
gwt_t = -d_t; the library is built with -ffp-contract=off and IEEE fp32 division), for s = 0.37,
-2.5 and 0; nothing written outside the segments or for a neighbor not asked for; gw pre-filled,
so the first launch has to overwrite it.  The same with rows 4 bytes into their buffers, with
a segment whose squares all underflow (norm exactly 0, zero-valued gradients) and with products
that are subnormal (kept, not flushed).

Interface level: prox_term on fp32 pool-bound models with a parameter past one chunk against the
torch loop, and prox_norms plus one backward against grad_chain bit for bit on the pool rows.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import test_gpu_prox_bf16 as pb
from _models import TinyNet
from _prox_oracle import grad_chain, norms64
from topology_aware_learning_amd import _lib
from topology_aware_learning_amd.prox import _plan_for, prox_norms, prox_term

pytestmark = pytest.mark.gpu

CHUNK, BLOCK = 8192, 256
_LENS = [1, BLOCK - 1, BLOCK, BLOCK + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7]


def _segments(lens):
    segs, off = [], 1
    for n in lens:
        off += 2  # a gap, then on to an odd offset
        off += 1 - off % 2
        segs.append((off, n))
        off += n
    return segs


SEGS = _segments(_LENS)
N = SEGS[-1][0] + SEGS[-1][1] + 5
KS = [1, 7, 8, 9, 16, 17, 64, 65, 128, 129]
SCALES = [0.37, -2.5, 0.0]
SENTINEL = 7.0
NORM_BOUND = 32 * 2.0 ** -24
GUARD = 256  # bytes on either side of the scratch, elements after norms_out


def test_segment_list_reaches_every_edge():
    assert [n for _, n in SEGS] == _LENS
    assert all(o % 2 == 1 for o, _ in SEGS)
    assert all(b[0] >= a[0] + a[1] + 2 for a, b in zip(SEGS, SEGS[1:]))  # gaps
    assert SEGS[0][0] >= 2 and N >= SEGS[-1][0] + SEGS[-1][1] + 2


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Plan:
    def __init__(self, device, segs):
        L = _lib.load()
        seg = np.array([x for s in segs for x in s], dtype=np.int64)
        P64 = ctypes.POINTER(ctypes.c_int64)
        words = L.tal_prox_plan_words(seg.ctypes.data_as(P64), len(segs))
        blob = np.zeros(words, dtype=np.int64)
        nc = ctypes.c_int32()
        _lib.check(L.tal_prox_plan_build(seg.ctypes.data_as(P64), len(segs), blob.ctypes.data_as(P64), words,
                                         ctypes.byref(nc)))
        self.segs, self.n_seg, self.n_chunks = list(segs), len(segs), int(nc.value)
        assert self.n_chunks == sum((n + CHUNK - 1) // CHUNK for _, n in segs)
        self.n = max(o + n for o, n in segs)
        self.inside = np.zeros(self.n, dtype=bool)
        for o, n in segs:
            assert not self.inside[o: o + n].any()
            self.inside[o: o + n] = True
        self.dev = torch.from_numpy(blob).to(device)


_cache = {}


def _plan(device):
    if "plan" not in _cache:
        _cache["plan"] = _Plan(device, SEGS)
    return _cache["plan"]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _place(x, device, mis):
    """The rows of the float32 array x on the device, each `mis` elements into its own 16-byte
    aligned buffer row."""
    rows_n, n = x.shape
    buf = torch.zeros(rows_n, n + 8 - n % 4, dtype=torch.float32, device=device)
    assert buf.data_ptr() % 16 == 0 and buf.stride(0) % 4 == 0
    rows = buf[:, mis: mis + n]
    rows.copy_(torch.from_numpy(x))
    assert all(rows[i].data_ptr() % 16 == 4 * mis for i in range(rows_n))
    return rows


def _host_rows(k, n, wide, seed):
    """k + 1 float32 rows of n elements (randn; `wide`: each scaled by 2^e, e in [-20, 20]);
    row 0 is the client, neighbor 1 (where there is one) equals it."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    x = torch.randn(k + 1, n, generator=g)
    if wide:
        x = x * torch.exp2(torch.randint(-20, 21, (k + 1, n), generator=g).float())
    if k >= 2:
        x[2] = x[0]
    return x.numpy()


def _norms(rows, plan):
    """tal_prox_norms with a scratch of exactly tal_prox_scratch_bytes between two guard regions
    and guard elements behind norms_out; the guards must keep their bytes."""
    L = _lib.load()
    k = rows.shape[0] - 1
    nbytes = int(L.tal_prox_scratch_bytes(plan.n_chunks, k))
    assert nbytes == 8 * plan.n_chunks * min(k, 64)
    sbuf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=rows.device)
    scratch = sbuf[GUARD: GUARD + nbytes]
    assert scratch.data_ptr() % 8 == 0
    obuf = torch.full((k * plan.n_seg + GUARD,), float("nan"), dtype=torch.float32, device=rows.device)
    wt = _lib.ptr_array([rows[1 + t].data_ptr() for t in range(k)])
    _lib.check(L.tal_prox_norms(_ptr(rows[0]), wt, k, _ptr(plan.dev), plan.n_chunks, plan.n_seg, _ptr(scratch),
                                _ptr(obuf), _stream()))
    torch.cuda.synchronize()
    assert (sbuf[:GUARD] == 0xA5).all() and (sbuf[GUARD + nbytes:] == 0xA5).all(), "written outside the scratch"
    assert torch.isnan(obuf[k * plan.n_seg:]).all(), "written behind norms_out"
    return obuf[: k * plan.n_seg].view(k, plan.n_seg).clone()


def _case(device, k, mis=0, wide=False):
    key = (k, mis, wide)
    if key not in _cache:
        x = _host_rows(k, N, wide, seed=2000 * k + 10 * mis + int(wide))
        rows = _place(x, device, mis)
        _cache[key] = (x, rows, _norms(rows, _plan(device)))
    return _cache[key]


def _check_norms(x, rows, norms, plan, what):
    k = x.shape[0] - 1
    again = _norms(rows, plan)
    assert torch.equal(_bits(norms), _bits(again))  # deterministic, scratch re-used
    want = norms64(x[0], list(x[1:]), plan.segs)
    got = norms.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    rel = float((err / np.maximum(want, 1e-300)).max())
    print(f"{what}: largest relative norm error {rel:.3e} = {rel * 2 ** 24:.2f} * 2^-24")
    assert (err <= NORM_BOUND * want).all()
    if k >= 2:
        assert (got[1] == 0).all()  # the identical neighbor: exactly 0
        assert (np.delete(got, 1, axis=0) > 0).all()


def _want_t(k):
    """Neighbors whose gradient is asked for: the identical one, every third one and the last."""
    return [t == 1 or t % 3 == 0 or t == k - 1 for t in range(k)]


def _grad(rows, norms, plan, scale, want_t, mis):
    """tal_prox_grad into sentinel-filled buffers: gw `mis` elements into its buffer like the
    rows, one gwt row per neighbor, the rows of neighbors not asked for passed as null."""
    L = _lib.load()
    k, n = rows.shape[0] - 1, rows.shape[1]
    device = rows.device
    s = torch.tensor([scale], dtype=torch.float32, device=device)
    gbuf = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=device)
    gw = gbuf[mis: mis + n]
    tbuf = torch.full((k, n + 8 - n % 4), SENTINEL, dtype=torch.float32, device=device)
    gwt = tbuf[:, mis: mis + n]
    wt = _lib.ptr_array([rows[1 + t].data_ptr() for t in range(k)])
    gwt_p = _lib.ptr_array([gwt[t].data_ptr() if want_t[t] else 0 for t in range(k)])
    _lib.check(L.tal_prox_grad(_ptr(rows[0]), wt, k, _ptr(plan.dev), plan.n_chunks, plan.n_seg, _ptr(norms), _ptr(s),
                               _ptr(gw), gwt_p, _stream()))
    torch.cuda.synchronize()
    return gbuf.cpu().numpy(), tbuf.cpu().numpy()


def _check_grad(x, rows, norms, plan, scale, mis, what, want_t=None):
    k, n = x.shape[0] - 1, x.shape[1]
    identical = want_t is None and k >= 2  # _case's rows: neighbor 1 equals the client
    if want_t is None:
        want_t = _want_t(k)
        assert (not all(want_t) or k == 1) and any(want_t)
    gbuf, tbuf = _grad(rows, norms, plan, scale, want_t, mis)
    ref_gw, ref_gwt = grad_chain(x[0], list(x[1:]), plan.segs, norms.cpu().numpy(), np.float32(scale), want_t,
                                 sentinel=SENTINEL)
    inside = np.zeros(n, dtype=bool)
    inside[: plan.n] = plan.inside
    sentinel = _np_bits(np.float32(SENTINEL))

    def same(buf, ref, name):
        got = buf[mis: mis + n]
        assert not np.isnan(got[inside]).any(), (what, name)
        bad = (_np_bits(got) != _np_bits(ref)) & inside
        assert not bad.any(), (what, name, int(bad.sum()), int(bad.nonzero()[0][0]))
        outside = np.ones(buf.shape, dtype=bool)
        outside[mis: mis + n] = ~inside
        assert (_np_bits(buf)[outside] == sentinel).all(), (what, name, "written outside the segments")

    same(gbuf, ref_gw, "gw")
    for t in range(k):
        if want_t[t]:
            same(tbuf[t], ref_gwt[t], f"gwt[{t}]")
        else:
            assert (_np_bits(tbuf[t]) == sentinel).all(), (what, f"gwt[{t}] was not asked for")
    if identical:  # contributes exactly nothing
        assert want_t[1] and (tbuf[1][mis: mis + n][inside] == 0).all()
    if scale != 0.0:
        assert (gbuf[mis: mis + n][inside] != 0).any()


@pytest.mark.parametrize("k", KS)
def test_norms_vs_float64(cuda, k):
    x, rows, norms = _case(cuda, k)
    _check_norms(x, rows, norms, _plan(cuda), f"k={k}")


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("k", KS)
def test_grad_is_the_chain_bit_for_bit(cuda, k, scale):
    x, rows, norms = _case(cuda, k)
    _check_grad(x, rows, norms, _plan(cuda), scale, 0, f"k={k} scale={scale}")


@pytest.mark.parametrize("k", [9, 65])
def test_wide_range_values(cuda, k):
    x, rows, norms = _case(cuda, k, wide=True)
    d = np.abs(x[0:1] - x[1:])[:, : _plan(cuda).n][:, _plan(cuda).inside]
    nz = d[d > 0]
    assert nz.min() >= 2.0 ** -40 and nz.max() <= 2.0 ** 40  # the float64 truth applies
    _check_norms(x, rows, norms, _plan(cuda), f"k={k} wide")
    for scale in SCALES[:2]:
        _check_grad(x, rows, norms, _plan(cuda), scale, 0, f"k={k} wide scale={scale}")


@pytest.mark.parametrize("k", [1, 9, 65, 129])
def test_unaligned_rows(cuda, k):
    """Every row and gw one element (4 bytes) into its buffer: no access may assume 16 bytes."""
    x, rows, norms = _case(cuda, k, mis=1)
    _check_norms(x, rows, norms, _plan(cuda), f"k={k} mis=1")
    _check_grad(x, rows, norms, _plan(cuda), 0.37, 1, f"k={k} mis=1")
    # the same values at aligned addresses: the same bits
    aligned = _place(x, cuda, 0)
    assert torch.equal(_bits(_norms(aligned, _plan(cuda))), _bits(norms))


EDGE_SEGS = [(3, 300), (311, 8192 + 100)]


def _edge_plan(device):
    if "edge" not in _cache:
        _cache["edge"] = _Plan(device, EDGE_SEGS)
    return _cache["edge"]


def test_squares_that_all_underflow(cuda):
    """Segment 0's differences are all below 2^-76: every square is below 2^-152 and rounds to 0
    in fp32, so the norm is exactly 0 (not the float64 truth) and, by the header's rule "0 where
    a norm is 0", gw and gwt are zero-valued there; nothing is inf or NaN.  Segment 1 is ordinary."""
    plan = _edge_plan(cuda)
    k, n = 3, plan.n + 3
    x = _host_rows(k, n, False, seed=77)
    x[2] = _host_rows(k, n, False, seed=78)[2]  # no identical neighbor here
    o, m = EDGE_SEGS[0]
    x[:, o: o + m] *= np.float32(2.0 ** -82)
    diff = np.abs(x[0:1, o: o + m] - x[1:, o: o + m])
    assert diff.max() < 2.0 ** -76 and diff.min() > 2.0 ** -126  # normal numbers, squares below 2^-152
    rows = _place(x, cuda, 0)
    norms = _norms(rows, plan)
    got = norms.cpu().numpy()
    assert (got[:, 0] == 0).all() and (got[:, 1] > 0).all() and np.isfinite(got).all()
    want = norms64(x[0], list(x[1:]), plan.segs)
    assert (np.abs(got[:, 1] - want[:, 1]) <= NORM_BOUND * want[:, 1]).all()
    for scale in SCALES:
        gbuf, tbuf = _grad(rows, norms, plan, scale, [True] * k, 0)
        assert np.isfinite(gbuf).all() and np.isfinite(tbuf).all()
        assert (gbuf[o: o + m] == 0).all() and (tbuf[:, o: o + m] == 0).all()
        _check_grad(x, rows, norms, plan, scale, 0, f"underflow scale={scale}", want_t=[True, False, True])


def test_subnormal_products_are_kept(cuda):
    """Segment 0 holds one difference near 2^20 and otherwise differences near 2^-120: c is near
    2^-21 and the products d are subnormal.  The chain keeps them (the oracle runs with gradual
    underflow), so a kernel that flushed subnormals to zero would differ in these bits."""
    plan = _edge_plan(cuda)
    k, n = 3, plan.n + 3
    x = _host_rows(k, n, False, seed=79)
    x[2] = _host_rows(k, n, False, seed=80)[2]
    o, m = EDGE_SEGS[0]
    x[:, o: o + m] *= np.float32(2.0 ** -120)
    x[0, o + 17] = np.float32(2.0 ** 20)
    rows = _place(x, cuda, 0)
    norms = _norms(rows, plan)
    want = norms64(x[0], list(x[1:]), plan.segs)
    assert (np.abs(norms.cpu().numpy() - want) <= NORM_BOUND * want).all()
    ref_gw, ref_gwt = grad_chain(x[0], list(x[1:]), plan.segs, norms.cpu().numpy(), np.float32(0.37), [True] * k)
    tiny = 2.0 ** -126
    for r in [ref_gw] + ref_gwt:  # the case is what it says: non-zero subnormals in the expected result
        sub = (np.abs(r[o: o + m]) < tiny) & (r[o: o + m] != 0)
        assert sub.sum() >= m - 1 - m // 10
    _check_grad(x, rows, norms, plan, 0.37, 0, "subnormal products", want_t=[True, False, True])


# ---- interface level ------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 9, 70])
def test_prox_term_past_one_chunk_matches_torch_loop(cuda, k):
    """prox_term on fp32 pool-bound models with a 130 x 127 parameter (three chunks) against the
    reference's loop, with test_prox_term_matches_torch_loop's bounds."""
    models, pool = pb._bound(cuda, pb._past_one_chunk, k + 1, seed=80 + k, dtype=torch.float32, identical=k >= 2)
    names = [n for n, _ in models[0].named_parameters()]
    plan = _plan_for(pool.layout, names, pool.device)
    assert plan.kind == "f32" and max(plan.numels) == 130 * 127 and plan.n_chunks == 3 + 3
    fused = prox_term(models[0], models[1:])
    assert fused is not None and fused.dtype == torch.float32
    fused.backward()
    ref_v, ref_g = pb._torch_loop(models)
    v = float(fused.detach())
    print(f"k={k}: value {v!r} reference {ref_v!r}")
    assert abs(v - ref_v) <= 1e-5 * abs(ref_v) + 1e-6
    for m, gs in zip(models, ref_g):
        for p, r in zip(m.parameters(), gs):
            assert p.grad is not None and p.grad.dtype == torch.float32 and p.grad.shape == p.shape
            assert torch.allclose(p.grad, r, rtol=1e-4, atol=1e-6)
    if k >= 2:
        assert all((p.grad == 0).all() for p in models[1].parameters())


@pytest.mark.parametrize("make", [TinyNet, pb._past_one_chunk], ids=["tinynet", "past_one_chunk"])
@pytest.mark.parametrize("k", [1, 9, 70])
def test_backward_is_the_chain_on_the_pool_rows(cuda, make, k):
    """The Python glue (pointer arrays in the models' row order, `views`, `needs`): prox_norms and
    one backward of 0.37 * prox_term equal grad_chain bit for bit on the pool rows; a neighbor
    whose parameters do not require grad gets none, and changes no one else's."""
    models, pool = pb._bound(cuda, make, k + 1, seed=90 + k, dtype=torch.float32, identical=k >= 2)
    frozen = 2 if k >= 3 else None  # the model that is neighbor 1
    if frozen is not None:
        for p in models[frozen].parameters():
            p.requires_grad_(False)
    names = [n for n, _ in models[0].named_parameters()]
    plan = _plan_for(pool.layout, names, pool.device)
    segs = list(zip(plan.offsets, plan.numels))
    rows = [pool.row_of(m) for m in models]
    assert rows == list(range(k, -1, -1))
    norms = prox_norms(pool, rows[0], rows[1:], plan)
    host = [pool.row_f32(r).cpu().numpy() for r in rows]
    want = norms64(host[0], host[1:], segs)
    got = norms.cpu().numpy()
    assert got.shape == (k, len(segs)) and (np.abs(got - want) <= NORM_BOUND * want).all()
    (prox_term(models[0], models[1:]) * 0.37).backward()
    want_t = [frozen is None or t != frozen - 1 for t in range(k)]
    ref_gw, ref_gwt = grad_chain(host[0], host[1:], segs, got, np.float32(0.37), want_t)
    for m, ref in zip(models, [ref_gw] + ref_gwt):
        for p, o, cnt in zip(m.parameters(), plan.offsets, plan.numels):
            if ref is None:
                assert p.grad is None
                continue
            assert p.grad is not None and p.grad.shape == p.shape
            g = p.grad.detach().reshape(-1).cpu().numpy()
            assert np.array_equal(_np_bits(g), _np_bits(ref[o: o + cnt])), (k, o)
