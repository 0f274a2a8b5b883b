"""Device operations: thin, checked wrappers over the C-ABI (include/tal_agg.h).

Every function takes torch tensors that already live on the GPU and launches on the current
torch stream of their device.  Nothing here falls back to the CPU: without the HIP library
the first call raises ``TalLibraryError``; with a CPU tensor it raises ``ValueError``.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import RoundPlanInfo, SeqPlanInfo, check

MODE_EXACT = _lib.TAL_MODE_EXACT
MODE_FMA = _lib.TAL_MODE_FMA


def _stream(device: torch.device, stream: Optional[torch.cuda.Stream] = None) -> ctypes.c_void_p:
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return ctypes.c_void_p(s.cuda_stream)


def _require_gpu(t: torch.Tensor, name: str, dtype: torch.dtype) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be a GPU tensor (got {t.device}); the aggregation has no CPU path")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _ptrs_and_weights(xs, weights, n, dtype, out):
    if len(xs) == 0:
        raise ValueError("at least one operand is required")
    if len(weights) != len(xs):
        raise ValueError(f"{len(xs)} operands but {len(weights)} weights")
    for i, x in enumerate(xs):
        _require_gpu(x, f"operand {i}", dtype)
        if x.numel() != n:
            raise ValueError(f"operand {i} has {x.numel()} elements, expected {n}")
        if x.device != out.device:
            raise ValueError(f"operand {i} is on {x.device}, out on {out.device}")
    return _lib.ptr_array([x.data_ptr() for x in xs]), _lib.double_array(weights)


def agg_f32(xs: Sequence[torch.Tensor], weights: Sequence[float], out: torch.Tensor,
            mode: int = MODE_EXACT, stream=None) -> torch.Tensor:
    """K1: out = sum_i fp32(w_i) * xs[i] (reference order; decentralized_client.py:399-411)."""
    _require_gpu(out, "out", torch.float32)
    n = out.numel()
    P, W = _ptrs_and_weights(xs, weights, n, torch.float32, out)
    L = _lib.load()
    check(L.tal_agg_f32(P, W, len(xs), ctypes.c_void_p(out.data_ptr()), n, int(mode),
                        _stream(out.device, stream)))
    return out


def agg_i64(xs: Sequence[torch.Tensor], weights: Sequence[float], out: torch.Tensor,
            stream=None) -> torch.Tensor:
    """K1 on int64 buffers: fp32 accumulate, truncation (decentralized_client.py:407-413)."""
    _require_gpu(out, "out", torch.int64)
    n = out.numel()
    P, W = _ptrs_and_weights(xs, weights, n, torch.int64, out)
    L = _lib.load()
    check(L.tal_agg_i64(P, W, len(xs), ctypes.c_void_p(out.data_ptr()), n, _stream(out.device, stream)))
    return out


def agg_model_f32(xs: Sequence[torch.Tensor], xis: Sequence[torch.Tensor], weights: Sequence[float],
                  out: torch.Tensor, out_i: torch.Tensor, mode: int = MODE_EXACT, stream=None) -> None:
    """K1 over a whole model in one launch: out = sum_i fp32(w_i) * xs[i] (fp32 segment) and
    out_i = trunc(sum_i fp32(w_i) * fp32(xis[i])) (int64 segment), the arithmetic of agg_f32 and
    agg_i64 bit for bit (decentralized_client.py:406-413 over every state_dict entry)."""
    _require_gpu(out, "out", torch.float32)
    _require_gpu(out_i, "out_i", torch.int64)
    n, n_i = out.numel(), out_i.numel()
    P, W = _ptrs_and_weights(xs, weights, n, torch.float32, out)
    PI, _ = _ptrs_and_weights(xis, weights, n_i, torch.int64, out)
    L = _lib.load()
    check(L.tal_agg_model_f32(P, PI, W, len(xs), ctypes.c_void_p(out.data_ptr()), n,
                              ctypes.c_void_p(out_i.data_ptr()), n_i, int(mode), _stream(out.device, stream)))


def agg_pool_rows(pool, rows: Sequence[int], weights: Sequence[float], out_row: int,
                  mode: int = MODE_EXACT, stream=None) -> None:
    """K1 on rows of one device-resident ModelPool: row out_row <- sum_i fp32(w_i) * row rows[i],
    every segment of the layout (fp32 + int64 in one launch, as agg_model_f32; otherwise one
    launch per segment), out_row may be one of the operands (the app's own model, in place).
    The arithmetic of agg_model_f32 / agg_f32 / agg_bf16 / agg_i64 on the rows' views, with the
    operand addresses computed from the pool (the pool's tensors are checked once per call, not
    each row view): the per-call app path on pool-bound models (decentralized_client.py:399-413)."""
    if pool.device.type != "cuda":
        raise ValueError(f"agg_pool_rows needs a device pool (got {pool.device}); the aggregation has no CPU path")
    m = len(rows)
    if m == 0:
        raise ValueError("at least one operand is required")
    if len(weights) != m:
        raise ValueError(f"{m} operands but {len(weights)} weights")
    for r in (*rows, out_row):
        if not 0 <= int(r) < pool.rows:
            raise IndexError(f"row {r} outside the pool's {pool.rows} rows")
    lay = pool.layout
    for seg, t, n in pool.segments():
        if t.dim() != 2 or t.stride(1) != 1 or t.shape[1] < n:
            raise ValueError(f"pool segment {seg} must be [rows, ld] with unit column stride")
    W = _lib.double_array(weights)
    s = _stream(pool.device, stream)
    L = _lib.load()
    rows = [int(r) for r in rows]
    if lay.n_f32 and lay.n_i64 and not lay.n_b16:
        check(L.tal_agg_model_f32(_lib.ptr_array(pool.row_ptrs("f32", rows)), _lib.ptr_array(pool.row_ptrs("i64", rows)),
                                  W, m, ctypes.c_void_p(pool.row_ptrs("f32", [out_row])[0]), lay.n_f32,
                                  ctypes.c_void_p(pool.row_ptrs("i64", [out_row])[0]), lay.n_i64, int(mode), s))
        return
    for seg, n in (("f32", lay.n_f32), ("b16", lay.n_b16), ("i64", lay.n_i64)):
        if not n:
            continue
        P = _lib.ptr_array(pool.row_ptrs(seg, rows))
        out = ctypes.c_void_p(pool.row_ptrs(seg, [out_row])[0])
        if seg == "i64":
            check(L.tal_agg_i64(P, W, m, out, n, s))
        else:
            fn = L.tal_agg_f32 if seg == "f32" else L.tal_agg_bf16
            check(fn(P, W, m, out, n, int(mode), s))


def agg_bf16(xs: Sequence[torch.Tensor], weights: Sequence[float], out: torch.Tensor,
             mode: int = MODE_EXACT, stream=None) -> torch.Tensor:
    """K1 on bf16 buffers.  MODE_EXACT: the reference's torch ops on bf16 tensors (every product
    and partial sum rounded to bf16; decentralized_client.py:407-411); MODE_FMA: fp32 fused
    accumulation rounded once."""
    _require_gpu(out, "out", torch.bfloat16)
    n = out.numel()
    P, W = _ptrs_and_weights(xs, weights, n, torch.bfloat16, out)
    L = _lib.load()
    check(L.tal_agg_bf16(P, W, len(xs), ctypes.c_void_p(out.data_ptr()), n, int(mode),
                         _stream(out.device, stream)))
    return out


# ------------------------------------------------------------------------------------------
# Host reduction (a process that sees no GPU: BASELINE config 1)
# ------------------------------------------------------------------------------------------
_HOST_FN = {torch.float32: "tal_host_agg_f32", torch.int64: "tal_host_agg_i64",
            torch.bfloat16: "tal_host_agg_bf16"}


def host_agg(xs: Sequence[torch.Tensor], weights: Sequence[float], out: torch.Tensor,
             mode: int = MODE_EXACT) -> torch.Tensor:
    """The library's host reduction (tal_host_agg_*) on contiguous CPU tensors of one dtype:
    out = sum_i fp32(w_i) * xs[i] with the kernels' arithmetic (fp32 / int64 / bf16, modes as
    agg_f32 / agg_i64 / agg_bf16).  For processes without a GPU only (aggregate.py dispatches
    on torch.cuda.is_available()); GPU tensors are refused."""
    if out.device.type != "cpu" or not out.is_contiguous() or out.dtype not in _HOST_FN:
        raise ValueError("host_agg: out must be a contiguous CPU float32 / int64 / bfloat16 tensor")
    if len(xs) == 0 or len(weights) != len(xs):
        raise ValueError("host_agg: one weight per operand, at least one operand")
    n = out.numel()
    for i, x in enumerate(xs):
        if x.device.type != "cpu" or x.dtype != out.dtype or not x.is_contiguous() or x.numel() != n:
            raise ValueError(f"host_agg: operand {i} must be a contiguous CPU {out.dtype} tensor of {n} elements")
    L = _lib.load()
    P, W = _lib.ptr_array([x.data_ptr() for x in xs]), _lib.double_array(weights)
    args = [P, W, len(xs), ctypes.c_void_p(out.data_ptr()), n]
    if out.dtype != torch.int64:
        args.append(int(mode))
    check(getattr(L, _HOST_FN[out.dtype])(*args))
    return out


# ------------------------------------------------------------------------------------------
# K3 round plans
# ------------------------------------------------------------------------------------------
LDS_BUDGET = 80 * 1024  # two workgroups per CU overlap one's HBM staging with the other's math
LDS_BUDGETS = (80 * 1024, 160 * 1024)  # candidates: 2 workgroups / CU, or 1 with bigger groups
TILE_WIDTHS = (64, 128, 32, 16)  # float4 per staged source per tile (ties keep the earlier)
# the narrow kernel's broadcast form (build_plan(bcast=...)): (c4, wavefronts per workgroup,
# workgroups per CU) of the forms that won a measured round - per-operand weights on a
# community graph (config 5 degree-centrality: fp32 16/8/2, bf16 32/16/1 and 16/16/2).
# The form is a candidate only for rounds with per-operand weights: on uniform-weight rows it
# never won (config 3: 6.2-9.9 ms against 2.0 in BENCH_r05; config 5 bf16 unweighted: 23.6-103
# against 22.3, profiles/r06/r06a)
BCAST_CANDIDATES = ((16, 8, 2), (16, 16, 2), (32, 16, 1), (32, 8, 2))
TUNE_DROP = 1.5  # a candidate whose first timed run exceeds the default's by this factor is dropped


@dataclass
class RoundPlan:
    info: RoundPlanInfo
    host: np.ndarray           # int32 blob
    device: Optional[torch.Tensor] = None
    rows: int = 0
    nnz: int = 0
    tuned_ms: Optional[float] = None
    candidates: Optional[list] = None  # tune_plan's measured candidates
    spec: Optional[dict] = None        # how it was built (plan_from_spec rebuilds it)

    @property
    def single_group(self) -> bool:
        return self.info.n_groups == 1

    def to(self, device) -> "RoundPlan":
        self.device = torch.from_numpy(self.host).to(device, non_blocking=False)
        return self

    def staged_rows(self) -> int:
        """Source rows read from HBM per column tile (sum over groups)."""
        return int(self.info.total_src)


@dataclass
class RowCallPlan:
    """A round as one K1 call per row, out of place (snapshot semantics): the fallback for a
    round with a row of more distinct sources than any LDS-tiled form stages in one tile
    (> ~620 at c4 = 16) on a bf16 pool, where the streamed form (fp32 only) cannot take it
    either - e.g. the reference's `unweighted_fl` strategy (every other client a neighbor,
    decentralized_app.py:386-389) with many clients under the batched round.  K1 chains any
    operand count in reference order, so every row is bitwise its per-call aggregation."""
    row_ptr: np.ndarray
    col: np.ndarray
    w: np.ndarray
    out_row: np.ndarray
    device: Optional[torch.device] = None
    tuned_ms: Optional[float] = None
    candidates: Optional[list] = None
    spec: Optional[dict] = None

    @property
    def rows(self) -> int:
        return len(self.out_row)

    @property
    def single_group(self) -> bool:
        return False  # rows read other rows' pre-round values: never in place

    def staged_rows(self) -> int:
        """Source rows read from HBM per column: every operand of every row."""
        return int(len(self.col))

    def to(self, device) -> "RowCallPlan":
        self.device = torch.device(device)
        return self


def row_call_plan(row_ptr, col, w, out_row) -> RowCallPlan:
    rp, cl, ww, orow = _csr(row_ptr, col, w, out_row)
    return RowCallPlan(rp, cl, ww, orow, spec={"rows_k1": 1})


def _round_rows(pool_in, pool_out, plan: RowCallPlan, n, dtype, mode, stream):
    _require_gpu(pool_in, "pool_in", dtype)
    _require_gpu(pool_out, "pool_out", dtype)
    if pool_in.dim() != 2 or pool_out.dim() != 2:
        raise ValueError("pools must be 2-D [models, ld]")
    if pool_in.data_ptr() == pool_out.data_ptr():
        raise ValueError("a per-row round runs out of place (snapshot semantics)")
    n = pool_in.shape[1] if n is None else int(n)
    if plan.col.max(initial=-1) >= pool_in.shape[0] or plan.out_row.max(initial=-1) >= pool_out.shape[0]:
        raise ValueError("plan rows beyond the pools")
    for r in range(plan.rows):
        a, b = int(plan.row_ptr[r]), int(plan.row_ptr[r + 1])
        xs = [pool_in[int(j), :n] for j in plan.col[a:b]]
        out = pool_out[int(plan.out_row[r]), :n]
        ws = plan.w[a:b].tolist()
        if dtype == torch.int64:
            agg_i64(xs, ws, out, stream=stream)
        elif dtype == torch.bfloat16:
            agg_bf16(xs, ws, out, mode=mode, stream=stream)
        else:
            agg_f32(xs, ws, out, mode=mode, stream=stream)
    return pool_out


def build_plan(row_ptr, col, w, out_row, c4: int = 0, lds_bytes: int = 0, dense: int = 0,
               bcast: int = 0, bcast_wg: int = 2) -> RoundPlan:
    """Tile plan for a round given as CSR (row r: operands col[row_ptr[r]:row_ptr[r+1]] with
    float64 weights w, written to pool row out_row[r]).

    c4 = 0 / lds_bytes = 0 search the float4 tile width (16, 32, 64 or 128 float4 per source;
    16 / 32 are the narrow-tile kernel: up to 256 / 128 sources in one group, sparse form) and
    the LDS budget (LDS_BUDGETS) for the plan with the lowest estimated time per element:
      HBM  = 4 B x (staged sources + rows)                     at ~5.5 TB/s
      LDS  = 4 B x operands (one LDS read per operand)         at ~150 TB/s x eff(workgroups/CU)
    (eff = 0.33 / 0.6 / 0.8 for 1 / 2 / >= 3 resident workgroups, halved at c4 = 64; fitted to
    tools/tune/round_variants.hip on MI355X); ties go to more resident workgroups.
    dense: 0 (default) = the sparse form; 8 requests dense row blocks; -1 lets the library
    pick dense when one LDS read serves >= 4 operands on average.  The dense form lost every
    measured A/B outside cliques (config 3: 6.2 vs 2.45 ms, config 5: 171 vs 83 ms; round-1
    tuner candidates), and clique rounds take the K3c plan (default_plan).
    bcast = 8 / 16: the narrow kernel's broadcast form (tal_round_plan_build_bcast) with that
    many wavefronts per workgroup: per-lane operand records in VGPRs, handed to a row's lanes
    by DPP row broadcasts, so per-operand weights cost no LDS reads (c4 16 / 32 only);
    bcast_wg = resident workgroups per CU it is compiled for (1: 128 VGPRs at 1024 threads and
    8 LDS reads in flight per wavefront; 2: 64 VGPRs, two groups' tiles per CU)."""
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    w = np.ascontiguousarray(w, dtype=np.float64)
    out_row = np.ascontiguousarray(out_row, dtype=np.int32)
    rows = len(out_row)
    if len(row_ptr) != rows + 1 or row_ptr[-1] != len(col) or len(w) != len(col):
        raise ValueError("inconsistent CSR arrays")
    L = _lib.load()
    cap = L.tal_round_plan_words(rows, len(col))
    best = None
    last_err = None
    widths = [c4] if c4 else ((16, 32) if bcast else TILE_WIDTHS)
    cands = [(c, b) for b in ([lds_bytes] if lds_bytes else LDS_BUDGETS) for c in widths]
    for cand, budget in cands:
        info = RoundPlanInfo()
        P32 = ctypes.POINTER(ctypes.c_int32)
        size = cap
        for _ in range(2):  # the dense tables' size is known only after grouping: retry once
            blob = np.zeros(size, dtype=np.int32)
            args = (rows, row_ptr.ctypes.data_as(P32), col.ctypes.data_as(P32),
                    w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out_row.ctypes.data_as(P32), cand, int(budget))
            if bcast:
                rc = L.tal_round_plan_build_bcast(*args, int(bcast), int(bcast_wg), blob.ctypes.data_as(P32), size,
                                                  ctypes.byref(info))
            else:
                rc = L.tal_round_plan_build(*args, int(dense), blob.ctypes.data_as(P32), size, ctypes.byref(info))
            if rc == _lib.TAL_ERR_CAPACITY and info.words > size:
                size = int(info.words)
                continue
            break
        if rc != _lib.TAL_OK:
            last_err = _lib.TalError(rc, L.tal_last_error().decode())
            continue
        spec = dict(c4=int(cand), lds=int(budget), dense=int(dense))
        if bcast:
            spec["bcast"] = int(bcast)
            spec["bcwg"] = int(bcast_wg)
        plan = RoundPlan(info=info, host=blob[: info.words].copy(), rows=rows, nnz=len(col), spec=spec)
        key = (_plan_cost(plan.info), -_blocks_per_cu(plan.info))
        if best is None or key < best[0]:
            best = (key, plan)
    if best is None:
        raise last_err
    return best[1]


CLIQUE_MAX = 64
CLIQUE_EXTRA = 4          # attached rows per clique block
CLIQUE_EXTRA_WORDS = 12
CLIQUE_WORDS = 4 + 2 * CLIQUE_MAX + CLIQUE_EXTRA * CLIQUE_EXTRA_WORDS  # TAL_CLIQUE_WORDS (180)
CLIQUE_MIN_ROWS = 8       # smaller blocks stay in the regular plan
CLIQUE_MIN_SHARED = 8     # an attached row takes at least this many operands from the block
# (bf16, mode): whether default_plan takes the per-source clique plan where the round has such
# blocks and no uniform ones: where it beat the earlier default by more than tune_plan's margin on
# both measured config-4 rounds (default_plan's docstring; profiles/r13) - all four
WCLIQUE_DEFAULT = {(False, MODE_EXACT): True, (False, MODE_FMA): True,
                   (True, MODE_EXACT): True, (True, MODE_FMA): True}
CLIQUE_COL_MAX = 128      # TAL_CLIQUE_COL_MAX: members of a block of the one-column-per-lane form (K3c1)
CLIQUE_COL_WORDS = 4 + 2 * CLIQUE_COL_MAX  # TAL_CLIQUE_COL_WORDS (260)
# (bf16, mode): whether default_plan admits blocks of 65..128 members (K3c1): where the 128-member
# plan beat the earlier default by more than tune_plan's margin on both the 66- and the
# 100-client round (default_plan's docstring; profiles/r14) - all four, by 2.5x to 5.1x
CLIQUE_COL_DEFAULT = {(False, MODE_EXACT): True, (False, MODE_FMA): True,
                      (True, MODE_EXACT): True, (True, MODE_FMA): True}
CLIQUE_COL_WWORDS = CLIQUE_COL_MAX  # TAL_CLIQUE_COL_WWORDS (128): one weight per member of a K3c1 block
# (bf16, mode): whether default_plan takes the per-source plan with blocks of 65..128 members
# (K3c1 with per-source weights, spec {"wclique": 1, "members": 128}) where the round has such a
# block: True only where that plan beat the plan default_plan returned before by more than
# tune_plan's margin on every round of tools/clique_col_weighted_rate.py (profiles/r17; medians
# of 20 interleaved runs, ms, new plan / earlier default on complete 66 and complete 100 at
# CIFAR-CNN width, complete 100 at ResNet-50 width under data-size weights, barbell(66, 3) at
# CIFAR-CNN width under degree-centrality softmax weights):
#   fp32 EXACT  0.576 / 2.354   0.985 / 3.731   4.226 / 15.172   1.889 / 4.655
#   fp32 FMA    0.579 / 1.914   1.068 / 2.894   4.437 / 12.153   1.864 / 3.797
#   bf16 EXACT  0.818 / 4.248   1.938 / 7.777   7.589 / 31.380   2.365 / 8.447
#   bf16 FMA    0.521 / 1.754   0.950 / 2.609   4.023 / 11.033   1.568 / 3.484
# - all four, by 2.0x to 5.2x, the forms agreeing bit for bit
WCLIQUE_COL_DEFAULT = {(False, MODE_EXACT): True, (False, MODE_FMA): True,
                       (True, MODE_EXACT): True, (True, MODE_FMA): True}


def find_cliques(row_ptr, col, w, out_row, min_rows: int = CLIQUE_MIN_ROWS, per_source: bool = False,
                 max_members: int = CLIQUE_MAX, wide_per_source: bool = False):
    """Uniform-weight clique blocks of a round (the K3c kernel's rows, tal_agg.h): rows whose
    operands are strictly ascending sources and then their own model (not among them), all with
    one finite fp32 weight, grouped by (operand set, weight); a group of >= min_rows rows with
    distinct own models and <= 64 sources is a clique block.  Other such rows that take at
    least CLIQUE_MIN_SHARED neighbors from a block and have at most two more are attached to it
    (up to CLIQUE_EXTRA per block).  Returns (cliques, rest): cliques = [(sources ascending, fp32
    weight, {member index: out_row}, [attached row records])], rest = the other row indices.

    per_source: blocks with one weight per source instead (the weighted and centrality apps on a
    clique; tal_agg_round_clique_w_*).  Rows are in the same reference order with all-finite fp32
    weights, grouped by operand set and by the fp32 bits every source carries: two rows share a
    block only when each source has the same weight in both.  The second element of a block is
    then the float32 array of its sources' weights, and an attached row's record carries its own
    per-operand weights: wm = {member index: weight}, wext = [weights of ext], wself.

    max_members: the largest block, 64 (K3c) or up to 128: uniform-weight blocks of 65..128
    sources run the one-column-per-lane form (K3c1, tal_agg_round_clique_col_*), which has no
    attached rows - rows beside such a block stay in rest.

    wide_per_source: with per_source, lifts the per-source limit from 64 to 128 members too
    (K3c1 with per-source weights, tal_agg_round_clique_col_w_*); without it per_source with
    max_members > 64 is a ValueError, as it was before that form existed."""
    if max_members > CLIQUE_COL_MAX:
        raise ValueError(f"clique blocks have at most {CLIQUE_COL_MAX} members")
    if per_source and max_members > CLIQUE_MAX and not wide_per_source:
        raise ValueError(f"per-source clique blocks have at most {CLIQUE_MAX} members")
    row_ptr, col, w, out_row = _csr(row_ptr, col, w, out_row)

    def reference_row(r):
        """(operands, fp32 weights) of row r when a block can carry it, else None."""
        ops_ = col[row_ptr[r]: row_ptr[r + 1]]
        if len(ops_) < 2:
            return None
        w32 = w[row_ptr[r]: row_ptr[r + 1]].astype(np.float32)
        if per_source:
            if not np.all(np.isfinite(w32)):
                return None
        elif not np.isfinite(w32[0]) or np.any(w32.view(np.uint32) != w32[:1].view(np.uint32)):
            return None
        nb, own = ops_[:-1], int(ops_[-1])
        if np.any(np.diff(nb) <= 0) or own in nb:
            return None
        return ops_, w32

    groups: dict = {}
    for r in range(len(out_row)):
        row = reference_row(r)
        if row is None or len(row[0]) > max_members:
            continue
        ops_, w32 = row
        by_src = np.argsort(ops_)
        wkey = tuple(w32[by_src].view(np.uint32).tolist()) if per_source else int(w32[:1].view(np.uint32)[0])
        groups.setdefault((tuple(ops_[by_src].tolist()), wkey), []).append(r)
    cliques, used = [], set()
    for (srcs, wbits), rows in groups.items():
        owns = [int(col[row_ptr[r + 1] - 1]) for r in rows]
        if len(rows) < min_rows or len(set(owns)) != len(rows):
            continue
        idx = {s: i for i, s in enumerate(srcs)}
        w32 = np.array(wbits if per_source else [wbits], np.uint32).view(np.float32)
        cliques.append((list(srcs), w32 if per_source else w32[0],
                        {idx[o]: int(out_row[r]) for o, r in zip(owns, rows)}, []))
        used.update(rows)
    # attached rows: rows in reference order that take most operands from one block (a barbell's
    # bridge nodes) - at most two other neighbors, own model anywhere; K3c blocks only
    attachable = [c for c in range(len(cliques)) if len(cliques[c][0]) <= CLIQUE_MAX]
    for r in range(len(out_row)):
        if r in used or not attachable:
            continue
        row = reference_row(r)
        if row is None:
            continue
        ops_, w32 = row
        nb, own = ops_[:-1], int(ops_[-1])
        best = max(attachable, key=lambda c: len(set(cliques[c][0]).intersection(nb.tolist())))
        srcs, _, _, att = cliques[best]
        idx = {s: i for i, s in enumerate(srcs)}
        mem = [int(x) for x in nb if int(x) in idx]
        ext = [int(x) for x in nb if int(x) not in idx]
        if len(mem) < CLIQUE_MIN_SHARED or len(ext) > 2 or len(att) >= CLIQUE_EXTRA:
            continue
        mask = 0
        for x in mem:
            mask |= 1 << idx[x]
        rec = dict(out=int(out_row[r]), w=w32[0], mask=mask, self_member=idx.get(own, -1),
                   self_row=-1 if own in idx else own,
                   ext=[(x, sum(1 for s_ in srcs if s_ < x)) for x in ext])
        if per_source:
            w_of = {int(x): w32[k] for k, x in enumerate(nb)}
            rec.update(wm={idx[x]: w_of[x] for x in mem}, wext=[w_of[x] for x in ext], wself=w32[-1])
        att.append(rec)
        used.add(r)
    return cliques, [r for r in range(len(out_row)) if r not in used]


CLIQUE_EXTRA_W = CLIQUE_MAX + 3                            # an attached row's weights: 64 member positions, 2 ext, self
CLIQUE_WWORDS = CLIQUE_MAX + CLIQUE_EXTRA * CLIQUE_EXTRA_W  # TAL_CLIQUE_WWORDS (332)


@dataclass
class CliquePlan:
    """A round split into clique blocks (K3c, one launch) and the remaining rows (a regular
    RoundPlan, None if there are none).  The clique kernel takes fp32 and bf16 pools; `full` is a
    sparse plan over all rows, used for the int64 segment and for pools that miss K3c's
    column-pair alignment (8 B fp32, 4 B bf16, even row stride).  `wtable` (per-source blocks:
    CLIQUE_WWORDS float32 per block, tal_agg.h) selects the tal_agg_round_clique_w_* entries.
    Blocks of 65..128 members (build_clique_plan(max_members=128)) are `col_table`: n_col records
    of CLIQUE_COL_WORDS for K3c1 (tal_agg_round_clique_col_*, one column per lane: no alignment
    rule), launched after the K3c blocks of `table`; clique_sources and clique_rows count both.
    A plan is per-source as a whole: built with wide_per_source, its blocks of 65..128 members
    carry `col_wtable` (CLIQUE_COL_WWORDS float32 per block beside `col_table`, whose weight word
    is then 0) and run tal_agg_round_clique_col_w_*."""
    table: np.ndarray
    n_cliques: int
    mmax: int
    clique_sources: int
    clique_rows: int
    rest: Optional[RoundPlan]
    full: RoundPlan
    rows: int
    rest_rows: Optional[list] = None
    device: Optional[torch.Tensor] = None
    tuned_ms: Optional[float] = None
    candidates: Optional[list] = None
    spec: Optional[dict] = None
    wtable: Optional[np.ndarray] = None
    wdevice: Optional[torch.Tensor] = None
    col_table: Optional[np.ndarray] = None
    n_col: int = 0
    col_mmax: int = 0
    col_device: Optional[torch.Tensor] = None
    col_wtable: Optional[np.ndarray] = None
    col_wdevice: Optional[torch.Tensor] = None
    on: Optional[torch.device] = None  # where the device copies are (to)

    @property
    def info(self) -> RoundPlanInfo:
        return self.full.info

    @property
    def single_group(self) -> bool:
        return False  # clique blocks read other blocks' sources: never in place

    @property
    def spec_key(self) -> str:
        """The plan's name in a spec: "wclique" with per-source weights, else "clique"."""
        return "wclique" if self.wtable is not None else "clique"

    def staged_rows(self) -> int:
        """Source rows read from HBM per column (clique sources + the rest plan's)."""
        return self.clique_sources + (self.rest.staged_rows() if self.rest is not None else 0)

    def make_spec(self) -> dict:
        """The spec plan_from_spec rebuilds this plan from: its name, "members": 128 when it has
        blocks of 65..128 members, and its rest plan's spec."""
        return {self.spec_key: 1, **({"members": CLIQUE_COL_MAX} if self.n_col else {}),
                "rest": self.rest.spec if self.rest is not None else None}

    def to(self, device) -> "CliquePlan":
        for host, attr in ((self.table, "device"), (self.wtable, "wdevice"), (self.col_table, "col_device"),
                           (self.col_wtable, "col_wdevice")):
            if host is not None:
                setattr(self, attr, torch.from_numpy(host).to(device))
        self.on = self.device.device
        if self.rest is not None:
            self.rest.to(device)
        self.full.to(device)
        return self

    def row_bounds(self):
        """(largest pool row the clique blocks read, largest they write); -1 for none."""
        t = self.table.reshape(self.n_cliques, CLIQUE_WORDS)
        att = t[:, 4 + 2 * CLIQUE_MAX:].reshape(self.n_cliques, CLIQUE_EXTRA, CLIQUE_EXTRA_WORDS)
        att = att[np.arange(CLIQUE_EXTRA)[None, :] < t[:, 2:3]]  # attached records in use
        ct = (self.col_table if self.col_table is not None else np.zeros(0, np.int32)).reshape(self.n_col, CLIQUE_COL_WORDS)
        return (max(t[:, 4: 4 + CLIQUE_MAX].max(initial=-1), att[:, [5, 7, 8]].max(initial=-1),
                    ct[:, 4: 4 + CLIQUE_COL_MAX].max(initial=-1)),
                max(t[:, 4 + CLIQUE_MAX: 4 + 2 * CLIQUE_MAX].max(initial=-1), att[:, 0].max(initial=-1),
                    ct[:, 4 + CLIQUE_COL_MAX:].max(initial=-1)))


def _clique_head(rec, wrec, cap, srcs, w32, outs):
    """A block's head in a record of either layout (cap = CLIQUE_MAX or CLIQUE_COL_MAX members):
    member count, weight - per source into wrec where the plan has a weight table, else the
    record's weight word - sources, and output rows (-1: none)."""
    rec[0] = len(srcs)
    if wrec is not None:
        wrec[: len(srcs)] = w32
    else:
        rec[1] = np.array([w32], np.float32).view(np.int32)[0]
    rec[4: 4 + len(srcs)] = srcs
    rec[4 + cap: 4 + 2 * cap] = -1
    for i, o in outs.items():
        rec[4 + cap + i] = o


def build_clique_plan(row_ptr, col, w, out_row, min_rows: int = CLIQUE_MIN_ROWS,
                      rest_spec: Optional[dict] = None, bf16: bool = False,
                      per_source: bool = False, max_members: int = CLIQUE_MAX,
                      wide_per_source: bool = False) -> Optional[CliquePlan]:
    """CliquePlan of a round, or None when it has no clique block (find_cliques).  bf16: the
    plan runs on bf16 pools, so its rest plan must be a form tal_agg_round_bf16 takes (sparse or
    narrow: dense_rb 0, stream_cs 0); a rest_spec that asks for another form is a ValueError.
    per_source: blocks with one weight per source (find_cliques(per_source=True)); the plan then
    carries `wtable`, and the table's two weight words stay 0.
    max_members (find_cliques): up to 128 admits uniform-weight blocks of 65..128 sources, which
    go to `col_table` (K3c1); blocks of <= 64 stay in `table` with their attached rows.
    wide_per_source (find_cliques): per-source blocks of 65..128 sources too; they go to
    `col_table` + `col_wtable` (no attached rows: rows beside them go to the rest plan)."""
    row_ptr, col, w, out_row = _csr(row_ptr, col, w, out_row)
    cliques, rest = find_cliques(row_ptr, col, w, out_row, min_rows, per_source=per_source,
                                 max_members=max_members, wide_per_source=wide_per_source)
    if not cliques:
        return None
    wide = [c for c in cliques if len(c[0]) > CLIQUE_MAX]
    cliques = [c for c in cliques if len(c[0]) <= CLIQUE_MAX]
    col_table = np.zeros((len(wide), CLIQUE_COL_WORDS), np.int32) if wide else None
    col_wtable = np.ones((len(wide), CLIQUE_COL_WWORDS), np.float32) if wide and per_source else None
    for k, (srcs, w32, outs, _) in enumerate(wide):
        _clique_head(col_table[k], col_wtable[k] if per_source else None, CLIQUE_COL_MAX, srcs, w32, outs)
    table = np.zeros((len(cliques), CLIQUE_WORDS), np.int32)
    wtable = np.ones((len(cliques), CLIQUE_WWORDS), np.float32) if per_source else None
    n_ext_loads = 0
    for k, (srcs, w32, outs, att) in enumerate(cliques):
        _clique_head(table[k], wtable[k] if per_source else None, CLIQUE_MAX, srcs, w32, outs)
        table[k, 2] = len(att)
        for q, a in enumerate(att):
            rec = table[k, 4 + 2 * CLIQUE_MAX + q * CLIQUE_EXTRA_WORDS:][:CLIQUE_EXTRA_WORDS]
            rec[0] = a["out"]
            if per_source:
                wrec = wtable[k, CLIQUE_MAX + q * CLIQUE_EXTRA_W:][:CLIQUE_EXTRA_W]
                for i, v in a["wm"].items():
                    wrec[i] = v
                wrec[CLIQUE_MAX: CLIQUE_MAX + len(a["wext"])] = a["wext"]
                wrec[CLIQUE_MAX + 2] = a["wself"]
            else:
                rec[1] = np.array([a["w"]], np.float32).view(np.int32)[0]
            rec[2:4] = np.array([a["mask"] & 0xFFFFFFFF, a["mask"] >> 32], np.uint32).view(np.int32)
            rec[4], rec[5], rec[6] = a["self_member"], a["self_row"], len(a["ext"])
            for e_, (row, pos) in enumerate(a["ext"]):
                rec[7 + e_], rec[9 + e_] = row, pos
            n_ext_loads += len(a["ext"]) + (a["self_row"] >= 0)
    rest_plan = None
    if rest:
        sub = _sub_csr(row_ptr, col, w, out_row, rest)
        rest_plan = plan_from_spec(*sub, rest_spec) if rest_spec else build_plan(*sub)
        if bf16 and (not isinstance(rest_plan, RoundPlan) or rest_plan.info.dense_rb or rest_plan.info.stream_cs):
            raise ValueError("a bf16 clique plan's other rows take a sparse or narrow plan (dense_rb 0, stream_cs 0)")
    mmax = max((len(c[0]) for c in cliques), default=0)
    return CliquePlan(table=table.reshape(-1), n_cliques=len(cliques), mmax=mmax,
                      clique_sources=sum(len(c[0]) for c in cliques + wide) + n_ext_loads,
                      clique_rows=sum(len(c[2]) + len(c[3]) for c in cliques + wide), rest=rest_plan,
                      full=build_plan(row_ptr, col, w, out_row, dense=0), rows=len(out_row), rest_rows=rest,
                      wtable=wtable.reshape(-1) if per_source else None,
                      col_table=col_table.reshape(-1) if wide else None, n_col=len(wide),
                      col_mmax=max((len(c[0]) for c in wide), default=0),
                      col_wtable=col_wtable.reshape(-1) if col_wtable is not None else None)


def _sub_csr(row_ptr, col, w, out_row, rows):
    """The CSR of a subset of a round's rows."""
    rp = np.concatenate([[0], np.cumsum([row_ptr[r + 1] - row_ptr[r] for r in rows])]).astype(np.int32)
    sel = np.concatenate([np.arange(row_ptr[r], row_ptr[r + 1]) for r in rows])
    return rp, col[sel], w[sel], np.asarray(out_row)[rows]




def _csr(row_ptr, col, w, out_row):
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    w = np.ascontiguousarray(w, dtype=np.float64)
    out_row = np.ascontiguousarray(out_row, dtype=np.int32)
    if len(row_ptr) != len(out_row) + 1 or row_ptr[-1] != len(col) or len(w) != len(col):
        raise ValueError("inconsistent CSR arrays")
    return row_ptr, col, w, out_row


def build_stream_plan(row_ptr, col, w, out_row, max_group_rows: int = 64, max_group_src: int = 0) -> RoundPlan:
    """Streamed-form plan (tal_round_plan_build_stream): groups of <= max_group_rows
    consecutive rows (and <= max_group_src distinct sources if > 0) whose sources stream through
    an LDS ring, so cliques and other dense neighborhoods of any size run without the LDS bound
    of build_plan.  Needs every row in reference order (sorted neighbors, then self)."""
    row_ptr, col, w, out_row = _csr(row_ptr, col, w, out_row)
    rows = len(out_row)
    L = _lib.load()
    P32 = ctypes.POINTER(ctypes.c_int32)
    size = L.tal_round_plan_words(rows, len(col))
    info = RoundPlanInfo()
    for _ in range(2):
        blob = np.zeros(size, dtype=np.int32)
        rc = L.tal_round_plan_build_stream(rows, row_ptr.ctypes.data_as(P32), col.ctypes.data_as(P32),
                                           w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                           out_row.ctypes.data_as(P32), int(max_group_rows),
                                           int(max_group_src), blob.ctypes.data_as(P32), size,
                                           ctypes.byref(info))
        if rc == _lib.TAL_ERR_CAPACITY and info.words > size:
            size = int(info.words)
            continue
        break
    check(rc)
    return RoundPlan(info=info, host=blob[: info.words].copy(), rows=rows, nnz=len(col))


def rows_uniform(row_ptr, w) -> bool:
    """Every row's operands share one fp32 weight (unweighted_module_avg, scale_agg): the
    narrow plans' row-weight form, on which the broadcast form never won."""
    w32 = np.asarray(w, dtype=np.float64).astype(np.float32)
    rp = np.asarray(row_ptr)
    first = np.repeat(w32[rp[:-1]], np.diff(rp))
    return bool(np.array_equal(w32, first))


# The clique variants by candidate key: build_clique_plan's keywords, the table that gates the
# variant as a default (None: not gated), and whether a plan has the blocks the variant exists for
_CLIQUE_VARIANTS = {
    "clique": (dict(), None, lambda p: True),
    "wclique": (dict(per_source=True), WCLIQUE_DEFAULT, lambda p: True),
    "clique128": (dict(max_members=CLIQUE_COL_MAX), CLIQUE_COL_DEFAULT, lambda p: p.n_col > 0),
    "wclique128": (dict(per_source=True, max_members=CLIQUE_COL_MAX, wide_per_source=True), WCLIQUE_COL_DEFAULT,
                   lambda p: p.col_wtable is not None),
}


def _clique_variant(name, row_ptr, col, w, out_row, bf16) -> Optional[CliquePlan]:
    """The variant's plan with its spec, or None where the round has no block of its kind."""
    kw, _, has_blocks = _CLIQUE_VARIANTS[name]
    p = build_clique_plan(row_ptr, col, w, out_row, bf16=bf16, **kw)
    if p is None or not has_blocks(p):
        return None
    p.spec = p.make_spec()
    return p


def tune_candidates(row_ptr, col, w, out_row, bf16: bool = False, mode: int = MODE_EXACT):
    """tune_plan's candidates [(key, plan)], the default plan first (host-side plans)."""
    base = default_plan(row_ptr, col, w, out_row, bf16=bf16, mode=mode)
    if base.spec is None:
        base.spec = {}
    cands = [(("default",), base)]
    sparse = []
    for c4 in TILE_WIDTHS:
        for budget in LDS_BUDGETS:
            try:
                p = build_plan(row_ptr, col, w, out_row, c4=c4, lds_bytes=budget, dense=0)
            except _lib.TalError:
                continue
            sparse.append(p)
    if sparse:
        fewest = min(p.staged_rows() for p in sparse)
        for p in sparse:
            key = (p.info.c4, p.info.n_groups, p.info.total_src, p.info.max_src)
            if p.staged_rows() <= 1.25 * fewest and all(key != k for k, _ in cands) and p.spec != base.spec:
                cands.append((key, p))
    for c4, waves, wg in (BCAST_CANDIDATES if not rows_uniform(row_ptr, w) else ()):
        try:
            p = build_plan(row_ptr, col, w, out_row, c4=c4, lds_bytes=LDS_BUDGETS[-1], bcast=waves, bcast_wg=wg)
        except _lib.TalError:
            continue
        key = ("bcast", c4, waves, wg)
        if all(key != k for k, _ in cands) and p.spec != base.spec:
            cands.append((key, p))
    for name, (kw, _, _) in _CLIQUE_VARIANTS.items():
        # a clique variant is offered when no clique plan already among the candidates is of its
        # kind (per-source weights, blocks of 65..128 members) and it takes rows none of them
        # takes; per-source plans (weighted / centrality apps on cliques) do not count against a
        # uniform-weight variant
        have = [c for _, c in cands if isinstance(c, CliquePlan)]
        per, wide = kw.get("per_source", False), "max_members" in kw
        if any((c.wtable is not None or not per) and (c.n_col > 0 or not wide) for c in have):
            continue
        p = _clique_variant(name, row_ptr, col, w, out_row, bf16)
        if p is not None and p.clique_rows > max((c.clique_rows for c in have if per or c.wtable is None), default=0):
            cands.append(((name,), p))
    return cands


def tune_plan(row_ptr, col, w, out_row, pool_in: torch.Tensor, pool_out: torch.Tensor,
              n: Optional[int] = None, reps: int = 5, mode: int = MODE_EXACT,
              margin: float = 0.01) -> RoundPlan:
    """Pick the plan by measurement, anchored on the untimed default (default_plan).

    Candidates are the forms that have won a measured round on some BASELINE config (DESIGN §4
    "Plan forms and their selection"): the sparse form at every tile width and LDS budget whose
    staging stays within 1.25 x the fewest staged sources of any candidate (multi-group plans
    that re-read sources - config 3's 80 KiB c4 = 128 plan stages 3.7x - never won), the
    broadcast forms that won (BCAST_CANDIDATES) on rounds with per-operand weights, and the
    clique plan (tune_candidates).  Dense row blocks and the streamed form lost every measured
    A/B outside their probes (BENCH_r04: 5.9 and 7.0 ms against 2.0 ms on config 3) and are
    built only on request (plan_from_spec); the register-resident groups (K3r: 8.5-16 ms on
    that round) lost too and were removed.

    Each candidate runs `reps` times, interleaved rep by rep with the others, and is judged by
    its median; one slower than TUNE_DROP x the default on its first timed run is not timed
    again (its median comes from that run).  A candidate replaces the default only when its
    median beats the default's by more than `margin` (round 4: the tuner's single short timings
    once kept a plan slower than the default - 23.74 vs 22.89 ms).  pool_out must not alias
    pool_in."""
    if pool_in.data_ptr() == pool_out.data_ptr():
        raise ValueError("tune_plan needs distinct input / output pools")
    bf16 = pool_in.dtype == torch.bfloat16  # bf16 rounds: sparse, narrow and clique plans
    run = round_bf16 if bf16 else round_f32
    cands = tune_candidates(row_ptr, col, w, out_row, bf16=bf16, mode=mode)
    base = cands[0][1]
    if isinstance(base, CliquePlan) and base.rest is not None:  # the rows outside the cliques: tuned too
        r_rp, r_col, r_w, r_out = _sub_csr(row_ptr, col, w, out_row, base.rest_rows)
        base.rest = tune_plan(r_rp, r_col, r_w, r_out, pool_in, pool_out, n=n, reps=reps, mode=mode, margin=margin)
        base.spec = base.make_spec()
    if len(cands) == 1:
        return base.to(pool_in.device)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _, p in cands:
        p.to(pool_in.device)
        run(pool_in, pool_out, p, n=n, mode=mode)  # warm (LDS attribute, code load)
    # candidates interleaved rep by rep, so a clock or thermal drift during tuning does not
    # favour the ones timed first
    ts = [[] for _ in cands]
    live = list(range(len(cands)))
    for rep in range(reps):
        for k in live:
            s.record()
            run(pool_in, pool_out, cands[k][1], n=n, mode=mode)
            e.record()
            e.synchronize()
            ts[k].append(s.elapsed_time(e))
        if rep == 0:  # far slower than the default on its first timed run: not timed again
            live = [k for k in live if k == 0 or ts[k][0] <= TUNE_DROP * ts[0][0]]
    med = [float(np.median(tk)) for tk in ts]
    timings = [{"form": "/".join(map(str, key)), "ms": round(t, 4), "all_ms": [round(x, 4) for x in tk], "spec": p.spec}
               for (key, p), t, tk in zip(cands, med, ts)]
    k_best = int(np.argmin(med))
    if med[k_best] >= (1.0 - margin) * med[0]:
        k_best = 0  # not clearly faster than the default: keep the default
    best = cands[k_best][1]
    best.tuned_ms = med[k_best]
    best.candidates = timings
    return best


def plan_from_spec(row_ptr, col, w, out_row, spec: dict) -> RoundPlan:
    """Rebuild a plan tune_plan chose (its `spec`): profiling runs then time the same plan
    without re-tuning."""
    if spec.get("clique") or spec.get("wclique"):
        p = build_clique_plan(row_ptr, col, w, out_row, rest_spec=spec.get("rest"),
                              per_source=not spec.get("clique"),
                              max_members=int(spec.get("members", CLIQUE_MAX)),  # "members": 128 admits K3c1 blocks
                              wide_per_source=not spec.get("clique"))
        if p is None:
            raise ValueError("plan spec asks for clique blocks but the round has none")
        p.spec = dict(spec)
        return p
    if spec.get("reg"):
        raise ValueError('plan spec asks for "reg": the register-resident form (K3r) was removed; a spec can ask '
                         'for "clique" / "wclique", "rows_k1", "stream_rows" with "stream_src", or "c4", "lds" and '
                         '"dense" (with "bcast" and "bcwg" for the broadcast form)')
    if "rows_k1" in spec:
        return row_call_plan(row_ptr, col, w, out_row)
    if "stream_rows" in spec:
        p = build_stream_plan(row_ptr, col, w, out_row, int(spec["stream_rows"]), int(spec["stream_src"]))
    else:
        p = build_plan(row_ptr, col, w, out_row, c4=int(spec["c4"]), lds_bytes=int(spec["lds"]),
                       dense=int(spec["dense"]), bcast=int(spec.get("bcast", 0)), bcast_wg=int(spec.get("bcwg", 2)))
    p.spec = dict(spec)
    return p


def default_plan(row_ptr, col, w, out_row, bf16: bool = False, mode: int = MODE_EXACT):
    """The plan the round components build when they do not time candidates (tune=False).
    A round with clique blocks takes the first clique variant (_CLIQUE_VARIANTS) that finds
    blocks of its kind, in this order of preference:
      clique128   a uniform-weight block of 65..128 members (`unweighted_fl` over 66 or 100
                  clients): K3c1, spec {"clique": 1, "members": 128}; gated by CLIQUE_COL_DEFAULT
      clique      uniform-weight blocks of <= 64 members: K3c, spec {"clique": 1}; never gated
      wclique128  no uniform block, a per-source block of 65..128 members (`weighted_module_avg`,
                  `centrality_module_avg` past 64 clients): K3c1 with per-source weights, spec
                  {"wclique": 1, "members": 128}; gated by WCLIQUE_COL_DEFAULT
      wclique     no uniform block, per-source blocks of <= 64 members: K3c with per-source
                  weights, spec {"wclique": 1}; gated by WCLIQUE_DEFAULT
    with the other rows in a sparse plan of their own; a round that lacks a variant's blocks, or
    whose (bf16, mode) the variant's table switches off, keeps exactly the plan of the lines below
    it.  Each table is True where the variant beat the plan returned before it by more than
    tune_plan's 1 % margin on every measured round, the forms agreeing bit for bit: the
    measurements are in DESIGN §4 and beside the *_DEFAULT tables (tools/clique_*_rate.py;
    profiles/r12, r13, r14 and r17).  A round without clique blocks takes
    build_plan's sparse form at the tile width and LDS budget its cost model picks; on the round-1
    A/B tables this is the measured winner's form for configs 2-5
    (tests/test_host_logic.py::test_default_plan_forms).  One exception, from round 4's
    measurements: a round whose narrow plan needs per-operand weights (the pairs
    form: centrality weights on a graph whose degrees differ) runs the narrow kernel's
    broadcast form with the whole source set in one LDS tile — for bf16 in FMA mode the
    two-chunk form (c4 = 32, 16 wavefronts, one workgroup per CU; config 5 with
    degree-centrality weights: 23.0-23.3 ms against 23.7-24.4 for the 16 x 2 form, 32.1-32.6 for
    the pairs form and 29.8-30.1 for the register-resident K3r, which round 3 picked and which
    has since been removed; profiles/r04/r04j, profiles/r04/pmc), for fp32 8 wavefronts x 2 (38.2-42.2 ms against 46.0
    for the cost model's two-group pairs plan; profiles/r04/r04f).  The broadcast plan is taken
    only when it has no more groups than the sparse plan; RoundExecutor runs a single-group
    plan (config 5's: every source in one tile) in place and a multi-group one through its
    scratch pool.  A round with a row of more distinct sources than one LDS tile holds (e.g.
    `unweighted_fl` over > ~620 clients) gets a streamed plan - the fp32 streamed kernel, or for
    bf16 pools the wide-row kernel - or, rows out of reference order, one K1 call per row
    (RowCallPlan)."""
    try:
        for name in ("clique128", "clique", "wclique128", "wclique"):
            gate = _CLIQUE_VARIANTS[name][1]
            if gate is None or gate[bool(bf16), int(mode)]:
                cp = _clique_variant(name, row_ptr, col, w, out_row, bf16)
                if cp is not None:  # a round without the variant's blocks keeps the plans below
                    return cp
        p = build_plan(row_ptr, col, w, out_row, dense=0)
    except _lib.TalError as exc:
        if exc.code != _lib.TAL_ERR_CAPACITY:
            raise
        # a row with more distinct sources than one LDS tile holds: fp32 rounds stream their
        # sources through an LDS ring (k_round_stream), bf16 rounds through LDS chunks in groups
        # of 16 rows (k_round_wide); rows in reference order either way; other operand orders
        # run one K1 call per row
        try:  # fp32: the streamed kernel's groups of 64 rows; bf16: the wide-row form's 16
            rows = 64 if not bf16 else WIDE_ROWS
            p = build_stream_plan(row_ptr, col, w, out_row, max_group_rows=rows)
            p.spec = {"stream_rows": rows, "stream_src": 0}
            return p
        except _lib.TalError:
            pass
        return row_call_plan(row_ptr, col, w, out_row)
    if p.info.c4 < 64 and not p.info.narrow_roww and (not bf16 or mode == MODE_FMA):
        # per-operand weights on a narrow plan: the broadcast form with every source in one LDS
        # tile - bf16 FMA: the two-chunk form (c4 = 32, one workgroup per CU) when its 512-B
        # tiles hold the group, else 16 wavefronts x 2; fp32: 8 wavefronts x 2 (its 1024-thread
        # two-workgroup form spills; the two-chunk form ran alike)
        forms = [(32, 16, 1), (16, 16, 2)] if bf16 else [(16, 8, 2)]
        for c4, waves, wg in forms:
            try:
                bp = build_plan(row_ptr, col, w, out_row, c4=c4, lds_bytes=LDS_BUDGETS[-1], bcast=waves, bcast_wg=wg)
            except _lib.TalError:  # a row past 128 / waves records: no broadcast form
                continue
            if bp.info.n_groups <= p.info.n_groups:
                return bp
    return p


WIDE_ROWS = 16  # rows per group of the bf16 wide-row form (k_round_wide, kWideRows)


def round_kernel_name(plan, bf16: bool = False) -> str:
    """Which K3 kernel tal_agg_round_f32 (bf16: tal_agg_round_bf16) launches for this plan or plan
    info, asked from the library (tal_round_kernel_name: the function its launch dispatches on);
    clique plans name the K3c kernel (their rest rows run a second one)."""
    if isinstance(plan, CliquePlan):
        return "k_round_clique" if plan.n_cliques > 0 else "k_round_clique_col"
    if isinstance(plan, RowCallPlan):
        return "k_agg (one call per row)"
    info = plan.info if isinstance(plan, RoundPlan) else plan
    return _lib.load().tal_round_kernel_name(ctypes.byref(info), int(bf16)).decode()


def _blocks_per_cu(info: RoundPlanInfo) -> int:
    if info.c4 < 64:  # narrow kernel: 1024 threads, data tile + plan slice
        return max(1, min(2, (160 * 1024) // max(1, info.lds_bytes)))
    lds = max(1, info.max_src * info.c4 * 16)
    return max(1, min(4, (160 * 1024) // lds))


def _plan_cost(info: RoundPlanInfo) -> float:
    """Estimated seconds per element column of the round (see build_plan)."""
    eff = {1: 0.33, 2: 0.6}.get(_blocks_per_cu(info), 0.8)
    if info.c4 <= 64:
        eff *= 0.5  # one float4 column per lane: half the LDS reads in flight of the c4=128 form
    hbm = 4.0 * (info.total_src + info.rows) / 5.5e12
    lds = 4.0 * info.dense_reads / (150e12 * eff)
    return max(hbm, lds)


def round_f32(pool_in: torch.Tensor, pool_out: torch.Tensor, plan, n: Optional[int] = None,
              mode: int = MODE_EXACT, stream=None) -> torch.Tensor:
    """K3 on [models, ld] fp32 pools (snapshot semantics; see tal_agg.h).  A CliquePlan runs
    its clique blocks with K3c and its other rows with their regular plan (out of place)."""
    if isinstance(plan, CliquePlan):
        return _round_clique(pool_in, pool_out, plan, n, torch.float32, mode, stream)
    if isinstance(plan, RowCallPlan):
        return _round_rows(pool_in, pool_out, plan, n, torch.float32, mode, stream)
    return _round(pool_in, pool_out, plan, n, torch.float32, mode, stream)


_CLIQUE_SUFFIX = {torch.float32: "_f32", torch.bfloat16: "_bf16"}


def _round_clique(pool_in, pool_out, plan: CliquePlan, n, dtype, mode, stream):
    _require_gpu(pool_in, "pool_in", dtype)
    _require_gpu(pool_out, "pool_out", dtype)
    if pool_in.dim() != 2 or pool_out.dim() != 2:
        raise ValueError("pools must be 2-D [models, ld]")
    if pool_in.device != pool_out.device:
        raise ValueError("pools on different devices")
    if pool_in.data_ptr() == pool_out.data_ptr():
        raise ValueError("a clique round runs out of place (snapshot semantics)")
    if plan.on != pool_in.device:
        plan.to(pool_in.device)
    n = pool_in.shape[1] if n is None else int(n)
    pair = 2 * pool_in.element_size()
    if plan.n_cliques > 0 and ((pool_in.stride(0) | pool_out.stride(0)) % 2
                               or (pool_in.data_ptr() | pool_out.data_ptr()) % pair):
        # K3c reads and writes column pairs (8 B fp32, 4 B bf16): rows not aligned to one take the full plan
        # (K3c1 has no such rule: a plan of 65..128-member blocks alone never gets here)
        return _round(pool_in, pool_out, plan.full, n, dtype, mode, stream)
    reads, writes = plan.row_bounds()
    if reads >= pool_in.shape[0]:
        raise ValueError("plan reads a pool row beyond pool_in")
    if writes >= pool_out.shape[0]:
        raise ValueError("plan writes a pool row beyond pool_out")
    L = _lib.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    # K3c for the blocks of <= 64 members, then K3c1 for those of 65..128, each with per-source
    # weights where the plan carries them; the entry is looked up by name at every call
    for col_form, table, blocks, mmax, wtab in (
            (False, plan.device, plan.n_cliques, plan.mmax, plan.wdevice if plan.wtable is not None else None),
            (True, plan.col_device, plan.n_col, plan.col_mmax, plan.col_wdevice if plan.col_wtable is not None else None)):
        if blocks > 0:
            fn = getattr(L, "tal_agg_round_clique" + "_col" * col_form + "_w" * (wtab is not None) + _CLIQUE_SUFFIX[dtype])
            check(fn(ptr(pool_in), pool_in.stride(0), ptr(pool_out), pool_out.stride(0), n, ptr(table), blocks, mmax,
                     int(mode), _stream(pool_in.device, stream), *((ptr(wtab),) if wtab is not None else ())))
    if plan.rest is not None:
        _round(pool_in, pool_out, plan.rest, n, dtype, mode, stream)
    return pool_out


def round_i64(pool_in: torch.Tensor, pool_out: torch.Tensor, plan: RoundPlan, n: Optional[int] = None,
              stream=None) -> torch.Tensor:
    if isinstance(plan, CliquePlan):
        plan = plan.full
    if isinstance(plan, RowCallPlan):
        return _round_rows(pool_in, pool_out, plan, n, torch.int64, MODE_EXACT, stream)
    return _round(pool_in, pool_out, plan, n, torch.int64, MODE_EXACT, stream)


def round_bf16(pool_in: torch.Tensor, pool_out: torch.Tensor, plan: RoundPlan, n: Optional[int] = None,
               mode: int = MODE_EXACT, stream=None) -> torch.Tensor:
    """K3 on [models, ld] bf16 pools (sparse, narrow or - rows wider than one LDS tile - streamed
    plans of at most 16 rows per group, the wide-row kernel; modes as agg_bf16).  A CliquePlan
    runs its clique blocks with K3c on bf16 (tal_agg_round_clique_bf16) and its other rows with
    their regular plan, out of place; pools that miss the 4-B column-pair alignment take
    `plan.full`.  Blocks of 65..128 members (`col_table`) run K3c1 (tal_agg_round_clique_col_bf16),
    which has no alignment rule."""
    if isinstance(plan, CliquePlan):
        return _round_clique(pool_in, pool_out, plan, n, torch.bfloat16, mode, stream)
    if isinstance(plan, RowCallPlan):
        return _round_rows(pool_in, pool_out, plan, n, torch.bfloat16, mode, stream)
    return _round(pool_in, pool_out, plan, n, torch.bfloat16, mode, stream)


_ROUND_FN = {torch.float32: "tal_agg_round_f32", torch.int64: "tal_agg_round_i64",
             torch.bfloat16: "tal_agg_round_bf16"}


def _round(pool_in, pool_out, plan, n, dtype, mode, stream):
    _require_gpu(pool_in, "pool_in", dtype)
    _require_gpu(pool_out, "pool_out", dtype)
    if pool_in.dim() != 2 or pool_out.dim() != 2:
        raise ValueError("pools must be 2-D [models, ld]")
    if pool_in.device != pool_out.device:
        raise ValueError("pools on different devices")
    if plan.device is None or plan.device.device != pool_in.device:
        plan.to(pool_in.device)
    n = pool_in.shape[1] if n is None else int(n)
    rows_in = pool_in.shape[0]
    rows_out = pool_out.shape[0]
    h = plan.host
    i = plan.info
    if h[i.off_src_row: i.off_src_row + i.total_src].max(initial=-1) >= rows_in:
        raise ValueError("plan reads a pool row beyond pool_in")
    if h[i.off_out_row: i.off_out_row + i.rows].max(initial=-1) >= rows_out:
        raise ValueError("plan writes a pool row beyond pool_out")
    L = _lib.load()
    fn = getattr(L, _ROUND_FN[dtype])
    args = [ctypes.c_void_p(pool_in.data_ptr()), pool_in.stride(0), ctypes.c_void_p(pool_out.data_ptr()),
            pool_out.stride(0), n, ctypes.c_void_p(plan.device.data_ptr()), ctypes.byref(plan.info)]
    if dtype != torch.int64:
        args.append(int(mode))
    args.append(_stream(pool_in.device, stream))
    check(fn(*args))
    return pool_out


# ------------------------------------------------------------------------------------------
# K3q: a sequential round in one launch
# ------------------------------------------------------------------------------------------
SEQ_MAX_SRC = 256  # TAL_SEQ_MAX_SRC: distinct source rows of one sequential plan
# (bf16, mode): whether RoundExecutor.run(sequential=True) runs the round as one K3q launch per
# segment instead of one K1 call per client: True only where the kernel's median beat the K1
# loop's by more than tune_plan's 1 % margin on every round of tools/seq_round_rate.py
# (profiles/r18; medians of 20 interleaved runs, ms, kernel / K1 loop on ring 32 at ResNet-18
# width, random-regular(8, 64) and barbell(60, 8) at ResNet-50 width, BA(33, 2) at CIFAR-CNN width):
#   fp32 EXACT  0.842 / 1.037   5.672 / 11.136   136.09 / 119.05   0.505 / 0.898
#   fp32 FMA    0.793 / 1.032   5.365 / 11.130   128.39 / 119.00   0.476 / 0.898
#   bf16 EXACT  0.702 / 0.732   3.810 /  5.989    67.27 /  64.40   0.410 / 0.705
#   bf16 FMA    0.682 / 0.722   3.488 /  5.844    61.38 /  62.77   0.398 / 0.709
# - bf16 FMA alone, by 1.02x (the barbell) to 1.78x.  The others lose the barbell round (its
# 61-operand rows are one dependent chain per lane with few waves resident on a CU) while winning
# the sparse rounds by 1.04x to 2.07x, the forms agreeing bit for bit; DESIGN §4 "K3q"
SEQ_DEFAULT = {(False, MODE_EXACT): False, (False, MODE_FMA): False,
               (True, MODE_EXACT): False, (True, MODE_FMA): True}


@dataclass
class SeqPlan:
    """A sequential round (tal_agg.h K3q): rows in the caller's order, each reading the pool as
    the rows before it left it."""
    info: SeqPlanInfo
    host: np.ndarray           # int32 blob
    device: Optional[torch.Tensor] = None
    rows: int = 0
    nnz: int = 0
    spec: Optional[dict] = None

    def to(self, device) -> "SeqPlan":
        self.device = torch.from_numpy(self.host).to(device, non_blocking=False)
        return self

    def staged_rows(self) -> int:
        """Source rows read from HBM per column tile."""
        return int(self.info.n_src)


def build_seq_plan(row_ptr, col, w, out_row) -> SeqPlan:
    """The plan of a sequential round given as CSR (row r: operands col[row_ptr[r]:row_ptr[r+1]]
    with float64 weights w, written to pool row out_row[r]; rows run in this order).  Raises
    TalError with TAL_ERR_CAPACITY for more than SEQ_MAX_SRC distinct source rows."""
    row_ptr, col, w, out_row = _csr(row_ptr, col, w, out_row)
    rows = len(out_row)
    L = _lib.load()
    P32 = ctypes.POINTER(ctypes.c_int32)
    size = int(L.tal_seq_plan_words(rows, len(col)))
    info = SeqPlanInfo()
    blob = np.zeros(size, dtype=np.int32)
    check(L.tal_seq_plan_build(rows, row_ptr.ctypes.data_as(P32), col.ctypes.data_as(P32),
                               w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out_row.ctypes.data_as(P32),
                               blob.ctypes.data_as(P32), size, ctypes.byref(info)))
    return SeqPlan(info=info, host=blob[: info.words].copy(), rows=rows, nnz=len(col), spec={"seq": 1})


_ROUND_SEQ_FN = {torch.float32: "tal_agg_round_seq_f32", torch.int64: "tal_agg_round_seq_i64",
                 torch.bfloat16: "tal_agg_round_seq_bf16"}


def _round_seq(pool, plan: SeqPlan, n, dtype, mode, stream):
    if not isinstance(plan, SeqPlan):
        raise TypeError("a sequential round takes a SeqPlan (build_seq_plan)")
    if not isinstance(pool, torch.Tensor):
        raise TypeError("pool must be a torch.Tensor")
    if pool.device.type != "cuda":
        raise ValueError(f"pool must be a GPU tensor (got {pool.device}); the aggregation has no CPU path")
    if pool.dtype != dtype:
        raise ValueError(f"pool must be {dtype} (got {pool.dtype})")
    if pool.dim() != 2 or pool.stride(1) != 1:
        raise ValueError("pool must be 2-D [models, ld] with unit column stride")
    n = pool.shape[1] if n is None else int(n)
    if not 0 <= n <= pool.shape[1]:
        raise ValueError(f"n = {n} outside the pool's {pool.shape[1]} columns")
    if plan.info.max_row >= pool.shape[0]:
        raise ValueError("plan reads or writes a pool row beyond the pool")
    if plan.device is None or plan.device.device != pool.device:
        plan.to(pool.device)
    L = _lib.load()
    args = [ctypes.c_void_p(pool.data_ptr()), pool.stride(0), pool.shape[0], n,
            ctypes.c_void_p(plan.device.data_ptr()), ctypes.byref(plan.info)]
    if dtype != torch.int64:
        args.append(int(mode))
    args.append(_stream(pool.device, stream))
    check(getattr(L, _ROUND_SEQ_FN[dtype])(*args))
    return pool


def round_seq_f32(pool: torch.Tensor, plan: SeqPlan, n: Optional[int] = None, mode: int = MODE_EXACT,
                  stream=None) -> torch.Tensor:
    """K3q on a [models, ld] fp32 pool, in place: the plan's rows in order, each the chain of
    agg_f32 on the pool as the rows before it left it (any row stride, element-aligned)."""
    return _round_seq(pool, plan, n, torch.float32, mode, stream)


def round_seq_bf16(pool: torch.Tensor, plan: SeqPlan, n: Optional[int] = None, mode: int = MODE_EXACT,
                   stream=None) -> torch.Tensor:
    """K3q on a bf16 pool (chains as agg_bf16 per mode; later rows read the stored bf16 value)."""
    return _round_seq(pool, plan, n, torch.bfloat16, mode, stream)


def round_seq_i64(pool: torch.Tensor, plan: SeqPlan, n: Optional[int] = None, stream=None) -> torch.Tensor:
    """K3q on an int64 pool (chains as agg_i64; later rows read the truncated integer)."""
    return _round_seq(pool, plan, n, torch.int64, MODE_EXACT, stream)


# ------------------------------------------------------------------------------------------
# K2 cosine similarity
# ------------------------------------------------------------------------------------------
@dataclass
class CosinePlan:
    n_seg: int
    n_chunks: int
    host: np.ndarray
    device: Optional[torch.Tensor] = None
    threads: int = 1


def build_cosine_plan(segments: Sequence[Sequence[int]], threads: int = 1) -> CosinePlan:
    """segments: (offset, A, I, B) per parameter tensor (see tal_agg.h K2).  threads: the torch
    intra-op thread count whose reduction order a tensor mean over >= 32768 outputs follows
    (the reference's process's torch.get_num_threads(); 1 = torch's serial order)."""
    seg = np.ascontiguousarray(np.asarray(segments, dtype=np.int64).reshape(-1, 4))
    L = _lib.load()
    P64 = ctypes.POINTER(ctypes.c_int64)
    words = L.tal_cosine_plan_words(seg.ctypes.data_as(P64), len(seg))
    if words < 0:
        raise ValueError("bad cosine segments")
    blob = np.zeros(words, dtype=np.int64)
    nch = ctypes.c_int32()
    check(L.tal_cosine_plan_build(seg.ctypes.data_as(P64), len(seg), blob.ctypes.data_as(P64), words,
                                  ctypes.byref(nch)))
    check(L.tal_cosine_plan_set_threads(blob.ctypes.data_as(P64), int(threads)))
    return CosinePlan(n_seg=len(seg), n_chunks=nch.value, host=blob, threads=int(threads))


# element types of the cosine entry points: fp32, or bf16 models widened exactly to fp32 by the
# loads (tal_agg.h "K2 on bf16 models"); the suffix of the *_bf16 twins
_COSINE_SUFFIX = {torch.float32: "", torch.bfloat16: "_bf16"}


def _cosine_dtype(first: torch.Tensor, what: str) -> torch.dtype:
    """The dtype of a cosine call, float32 or bfloat16: its first operand's (every operand is then
    checked against it)."""
    if not isinstance(first, torch.Tensor):
        raise TypeError(f"{what}: model 0 must be a torch.Tensor")
    if first.dtype not in _COSINE_SUFFIX:
        raise ValueError(f"{what}: models must be float32 or bfloat16 (got {first.dtype})")
    return first.dtype


def _one_dtype(what: str, dtype: torch.dtype, i: int, t: torch.Tensor) -> ValueError:
    return ValueError(f"{what}: every operand must have one dtype (model 0 is {dtype}, model {i} is {t.dtype})")


def cosine(a_list: Sequence[torch.Tensor], b_list: Sequence[torch.Tensor], plan: CosinePlan,
           stream=None) -> torch.Tensor:
    """K2: cosine_similarity(a_j, b_j) for every pair (flat parameter arenas, all float32 or all
    bfloat16), the reference's fp32 value bit for bit; for bfloat16 models that of the models
    widened to fp32 (tal_agg.h "K2 on bf16 models")."""
    if len(a_list) != len(b_list) or not a_list:
        raise ValueError("need matching, non-empty a/b lists")
    dev = a_list[0].device
    dtype = _cosine_dtype(a_list[0], "cosine")
    for i, t in enumerate(list(a_list) + list(b_list)):
        if isinstance(t, torch.Tensor) and t.dtype != dtype:
            raise _one_dtype("cosine", dtype, i, t)
        _require_gpu(t, f"model {i}", dtype)
        if t.device != dev:
            raise ValueError("models on different devices")
    if plan.device is None or plan.device.device != dev:
        plan.device = torch.from_numpy(plan.host).to(dev)
    L = _lib.load()
    P64 = ctypes.POINTER(ctypes.c_int64)
    hp = plan.host.ctypes.data_as(P64)
    scratch = torch.empty(int(L.tal_cosine_scratch_bytes(hp, len(a_list))), dtype=torch.uint8, device=dev)
    out = torch.empty(len(a_list), dtype=torch.float32, device=dev)
    fn = getattr(L, "tal_cosine_params" + _COSINE_SUFFIX[dtype])
    check(fn(_lib.ptr_array([t.data_ptr() for t in a_list]), _lib.ptr_array([t.data_ptr() for t in b_list]),
             len(a_list), ctypes.c_void_p(plan.device.data_ptr()), hp, plan.n_chunks,
             ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(out.data_ptr()), _stream(dev, stream)))
    return out


def host_cosine(a_list: Sequence[torch.Tensor], b_list: Sequence[torch.Tensor], plan: CosinePlan) -> torch.Tensor:
    """K2's arithmetic on the host (tal_host_cosine / tal_host_cosine_bf16): cosine_similarity(a_j,
    b_j) for flat contiguous CPU parameter arenas, all float32 or all bfloat16, the reference's
    fp32 value bit for bit (bfloat16: of the widened models, as `cosine`), in a process that sees
    no GPU (similarity.cosine_pairs dispatches on torch.cuda.is_available())."""
    if len(a_list) != len(b_list) or not a_list:
        raise ValueError("need matching, non-empty a/b lists")
    dtype = _cosine_dtype(a_list[0], "host_cosine")
    for i, t in enumerate(list(a_list) + list(b_list)):
        if t.dtype != dtype:
            raise _one_dtype("host_cosine", dtype, i, t)
        if t.device.type != "cpu" or not t.is_contiguous():
            raise ValueError(f"host_cosine: model {i} must be a contiguous CPU float32 or bfloat16 tensor")
    out = torch.empty(len(a_list), dtype=torch.float32)
    L = _lib.load()
    fn = getattr(L, "tal_host_cosine" + _COSINE_SUFFIX[dtype])
    check(fn(_lib.ptr_array([t.data_ptr() for t in a_list]), _lib.ptr_array([t.data_ptr() for t in b_list]),
             len(a_list), plan.host.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.c_void_p(out.data_ptr())))
    return out


# K2r: the cosine similarities of a whole round in one call (tal_agg.h K2r)
COSINE_ROUND_BUDGET = 256 << 20  # default scratch budget in bytes: config 3's round takes 141 MB, one batch


@dataclass
class CosineRound:
    """A round's ordered pairs of pool rows as tal_cosine_round_build's table."""
    n_pairs: int
    pool_rows: int
    host: np.ndarray
    info: "_lib.CosineRoundInfo"
    device: Optional[torch.Tensor] = None


def build_cosine_round(pairs: Sequence[Sequence[int]], pool_rows: int) -> CosineRound:
    """pairs: (row_a, row_b) per ordered pair, rows of a pool of `pool_rows` rows.  The table holds
    the distinct rows, the distinct unordered pairs in groups that share a row, and the map from
    each ordered pair to its unordered pair."""
    arr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(arr) == 0:
        raise ValueError("cosine round: no pairs")
    if arr.min() < 0 or arr.max() >= int(pool_rows):
        raise ValueError(f"cosine round: a row outside [0, {int(pool_rows)})")
    ra = np.ascontiguousarray(arr[:, 0], dtype=np.int32)
    rb = np.ascontiguousarray(arr[:, 1], dtype=np.int32)
    L = _lib.load()
    P32 = ctypes.POINTER(ctypes.c_int32)
    words = L.tal_cosine_round_words(len(arr))
    blob = np.zeros(words, dtype=np.int32)
    info = _lib.CosineRoundInfo()
    check(L.tal_cosine_round_build(ra.ctypes.data_as(P32), rb.ctypes.data_as(P32), len(arr), int(pool_rows),
                                   blob.ctypes.data_as(P32), words, ctypes.byref(info)))
    return CosineRound(n_pairs=len(arr), pool_rows=int(pool_rows), host=np.ascontiguousarray(blob[: info.words]),
                       info=info)


def _cosine_round_args(pool_f32: torch.Tensor, pairs_or_table, plan: CosinePlan, what: str):
    if not isinstance(pool_f32, torch.Tensor):
        raise TypeError(f"{what}: the pool must be a torch.Tensor")
    if pool_f32.dtype not in _COSINE_SUFFIX or pool_f32.dim() != 2 or pool_f32.shape[0] < 1 or (
            pool_f32.shape[1] > 1 and pool_f32.stride(1) != 1):
        raise ValueError(f"{what}: the pool must be a 2-D float32 or bfloat16 tensor with unit column stride")
    ld = int(pool_f32.stride(0)) if pool_f32.shape[0] > 1 else int(pool_f32.shape[1])
    seg = plan.host[4: 4 + 7 * plan.n_seg].reshape(-1, 7)
    extent = int((seg[:, 0] + seg[:, 1] * seg[:, 2] * seg[:, 3]).max())
    if pool_f32.shape[1] < extent or ld < pool_f32.shape[1]:
        raise ValueError(f"{what}: the pool's rows ({pool_f32.shape[1]} elements, pitch {ld}) are shorter than the "
                         f"plan's parameters ({extent})")
    table = pairs_or_table if isinstance(pairs_or_table, CosineRound) else build_cosine_round(
        pairs_or_table, pool_f32.shape[0])
    if table.pool_rows > pool_f32.shape[0]:
        raise ValueError(f"{what}: the table was built for {table.pool_rows} rows, the pool has {pool_f32.shape[0]}")
    return ld, table


def cosine_round(pool_f32: torch.Tensor, pairs_or_table, plan: CosinePlan, budget_bytes: int = COSINE_ROUND_BUDGET,
                 stream=None) -> torch.Tensor:
    """K2r: cosine_similarity(pool[a_j], pool[b_j]) for every ordered pair of a round, rows of one
    device pool segment f32[rows, ld] or b16[rows, ld] (float32 or bfloat16; the name is
    historical): every norm once per model, every unordered pair once, one launch sequence on the
    current (or given) stream.  Bit for bit `cosine` on the same pairs.
    pairs_or_table: (row_a, row_b) pairs, or a CosineRound of build_cosine_round.  budget_bytes
    bounds the scratch (the unique pairs run in batches under it)."""
    if pool_f32.device.type != "cuda":
        raise ValueError(f"cosine_round: the pool must be a GPU tensor (got {pool_f32.device}); "
                         "host_cosine_round is the host form")
    ld, table = _cosine_round_args(pool_f32, pairs_or_table, plan, "cosine_round")
    dev = pool_f32.device
    if plan.device is None or plan.device.device != dev:
        plan.device = torch.from_numpy(plan.host).to(dev)
    if table.device is None or table.device.device != dev:
        table.device = torch.from_numpy(table.host).to(dev)
    L = _lib.load()
    hp = plan.host.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    ht = table.host.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    need = int(L.tal_cosine_round_scratch_bytes(hp, ht, ctypes.byref(table.info), int(budget_bytes)))
    if need < 0:
        raise ValueError(f"cosine_round: budget_bytes={int(budget_bytes)} does not hold the norm table and one pair group")
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(table.n_pairs, dtype=torch.float32, device=dev)
    fn = getattr(L, "tal_cosine_round" + _COSINE_SUFFIX[pool_f32.dtype])
    check(fn(ctypes.c_void_p(pool_f32.data_ptr()), ld, ctypes.c_void_p(plan.device.data_ptr()), hp, plan.n_chunks,
             ctypes.c_void_p(table.device.data_ptr()), ht, ctypes.byref(table.info),
             ctypes.c_void_p(scratch.data_ptr()), need, ctypes.c_void_p(out.data_ptr()), _stream(dev, stream)))
    if stream is not None:  # the scratch is released to the current stream's allocator pool
        scratch.record_stream(stream)
    return out


def host_cosine_round(pool_f32: torch.Tensor, pairs_or_table, plan: CosinePlan) -> torch.Tensor:
    """cosine_round on a CPU pool, float32 or bfloat16 (tal_host_cosine_round[_bf16]:
    tal_host_cosine's arithmetic, every unordered pair once), for a process that sees no GPU."""
    if pool_f32.device.type != "cpu":
        raise ValueError("host_cosine_round: the pool must be a CPU tensor")
    ld, table = _cosine_round_args(pool_f32, pairs_or_table, plan, "host_cosine_round")
    out = torch.empty(table.n_pairs, dtype=torch.float32)
    L = _lib.load()
    fn = getattr(L, "tal_host_cosine_round" + _COSINE_SUFFIX[pool_f32.dtype])
    check(fn(ctypes.c_void_p(pool_f32.data_ptr()), ld, plan.host.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
             table.host.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(table.info),
             ctypes.c_void_p(out.data_ptr())))
    return out


# ------------------------------------------------------------------------------------------
# Synthetic pool rows (benchmark / full-size test inputs)
# ------------------------------------------------------------------------------------------
_FILL_TORCH = {0: torch.float32, 1: torch.bfloat16, 2: torch.int64}


def fill_counter(seg: torch.Tensor, table: np.ndarray, dtype_code: int, stream=None) -> torch.Tensor:
    """tal_fill_counter: rows 0..n_rows-1 of the [rows, ld] segment `seg` = synth's counter
    generator per `table` (synth.fill_table), one launch for all rows."""
    if seg.device.type != "cuda" or seg.dtype != _FILL_TORCH[int(dtype_code)]:
        raise ValueError(f"fill_counter needs a GPU {_FILL_TORCH[int(dtype_code)]} segment (got {seg.device} {seg.dtype})")
    tab = np.ascontiguousarray(table, dtype=np.int64)
    n_rows, n = int(tab[0]), int(tab[1])
    if seg.dim() != 2 or seg.stride(1) != 1 or seg.shape[0] < n_rows or seg.shape[1] < n:
        raise ValueError(f"seg must be [>= {n_rows}, >= {n}] with unit column stride (got {tuple(seg.shape)})")
    dev_tab = torch.from_numpy(tab).to(seg.device)
    L = _lib.load()
    check(L.tal_fill_counter(ctypes.c_void_p(seg.data_ptr()), seg.stride(0), int(dtype_code),
                             ctypes.c_void_p(dev_tab.data_ptr()), tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                             _stream(seg.device, stream)))
    return seg
