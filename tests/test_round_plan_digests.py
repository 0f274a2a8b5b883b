"""The K3 planner's output, pinned byte for byte (no GPU).

Every case builds a round plan through the C entry points and compares
sha256(bytes(info) + blob[:info.words]), n_groups, words and the kernel name
(ops.round_kernel_name, fp32 and bf16) with tests/golden/round_plan_digests.json; a failing
build is pinned by its status, its message and the info.words it leaves.  The fixture was
recorded before the planner's host code was cut into per-form encoders, so a host-side
refactor that keeps this test green kept every plan byte.

Run as a script (`python tests/test_round_plan_digests.py`) the file REWRITES its fixture from
the library in the tree.  Do that only for a deliberate planner change (a new field, another
grouping rule): the diff of the fixture is then part of that change's review.

Graphs (deterministic; the random ones from a fixed linear congruential generator, their CSR
hashed into the fixture as well): a 40-row ring with neighbours -1, +1 and +5 (uniform weights;
uniform with every third row's weight negative - the ROWW form's second zero tile; per-operand
random), a random 8-regular graph of 96 rows (uniform, per-operand random), a 20-row clique
(uniform), four rows of 150 sources (the tiled kernel's plan), and one small CSR whose operands
are out of reference order.  Rows list their
neighbours ascending and then themselves, as the reference does.

Forms: tal_round_plan_build at c4 16/32/64/128 x dense 0/8/-1 (dense at c4 >= 64) with the
whole 160 KiB and with a small budget per width that forces many groups (8/16/40/80 KiB),
tal_round_plan_build_bcast at c4 16/32 x 8/12/16 wavefronts x 1/2 workgroups per CU at 160 and
8 KiB, tal_round_plan_build_stream at 3/16/64/128 rows per group with and without a 24-source
cap (both chunk sizes, stream_cs 16 and 32, occur).  Error paths: a null plan buffer (capacity,
info.words filled), a row wider than its tile (16 KiB at c4 128 for every graph, 16 KiB at
c4 64 for the clique), and the out-of-order CSR under the stream builder; the forced-dense
request on that CSR answers with a sparse plan.
"""
import ctypes
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))

from topology_aware_learning_amd import _lib, ops  # noqa: E402

FIXTURE = Path(__file__).resolve().parent / "golden" / "round_plan_digests.json"
KIB = 1024
SMALL_BUDGET = {16: 8 * KIB, 32: 16 * KIB, 64: 40 * KIB, 128: 80 * KIB}
P32 = ctypes.POINTER(ctypes.c_int32)
PD = ctypes.POINTER(ctypes.c_double)


class _Lcg:
    """Knuth's MMIX generator: the graphs must not depend on a library's random streams."""

    def __init__(self, seed):
        self.s = seed

    def next(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return self.s >> 33

    def below(self, n):
        return self.next() % n

    def unit(self):
        return (self.next() + 1) / float((1 << 31) + 1)


def _csr_of(adj, weight):
    """Rows in reference order: neighbours ascending, then the row itself; weight(r, k, m)."""
    row_ptr, col, w = [0], [], []
    for r, nb in enumerate(adj):
        ops_ = sorted(set(nb) - {r}) + [r]
        col += ops_
        w += [weight(r, k, len(ops_)) for k in range(len(ops_))]
        row_ptr.append(len(col))
    return (np.asarray(row_ptr, np.int32), np.asarray(col, np.int32), np.asarray(w, np.float64),
            np.arange(len(adj), dtype=np.int32))


def _ring():
    return [[(r - 1) % 40, (r + 1) % 40, (r + 5) % 40] for r in range(40)]


def _regular8():
    """Four edge-disjoint random Hamiltonian cycles on 96 nodes."""
    rng, n = _Lcg(20240607), 96
    edges, adj = set(), [[] for _ in range(n)]
    cycles = 0
    while cycles < 4:
        perm = list(range(n))
        for i in range(n - 1, 0, -1):
            j = rng.below(i + 1)
            perm[i], perm[j] = perm[j], perm[i]
        cyc = {frozenset((perm[i], perm[(i + 1) % n])) for i in range(n)}
        if cyc & edges:
            continue
        edges |= cyc
        cycles += 1
    for e in edges:
        a, b = tuple(e)
        adj[a].append(b)
        adj[b].append(a)
    assert all(len(set(x)) == 8 for x in adj)
    return adj


def _graphs():
    uniform = lambda r, k, m: 1.0 / m  # noqa: E731
    third_neg = lambda r, k, m: (-1.0 if r % 3 == 0 else 1.0) / m  # noqa: E731

    def rand(seed):
        rng = _Lcg(seed)
        return lambda r, k, m: 0.05 + 0.9 * rng.unit()

    clique = [[c for c in range(20) if c != r] for r in range(20)]
    return {
        "ring40_uniform": _csr_of(_ring(), uniform),
        "ring40_third_negative": _csr_of(_ring(), third_neg),
        "ring40_random": _csr_of(_ring(), rand(7)),
        "reg8x96_uniform": _csr_of(_regular8(), uniform),
        "reg8x96_random": _csr_of(_regular8(), rand(11)),
        "clique20_uniform": _csr_of(clique, uniform),
    }


def _wide150():
    """Four rows of 150 sources each: past the persistent kernel's staging at c4 = 64 (the tiled
    kernel), more than a c4 = 128 tile holds."""
    return _csr_of([[c for c in range(4, 154) if (c + r) % 31] for r in range(4)], lambda r, k, m: 1.0 / m)


def _out_of_order():
    """Six rows of a ring whose operands start with the row itself and then descend."""
    row_ptr, col, w = [0], [], []
    for r in range(6):
        col += [r, (r + 1) % 6, (r - 1) % 6] if r % 2 else [r, max((r + 1) % 6, (r - 1) % 6), min((r + 1) % 6, (r - 1) % 6)]
        w += [0.5, 0.25, 0.25]
        row_ptr.append(len(col))
    return (np.asarray(row_ptr, np.int32), np.asarray(col, np.int32), np.asarray(w, np.float64),
            np.arange(6, dtype=np.int32))


def _cases():
    """[(case id, graph name, builder, builder arguments, null plan buffer)]"""
    out = []
    for g in _graphs():
        for c4 in (16, 32, 64, 128):
            for dense in ((0, 8, -1) if c4 >= 64 else (0,)):
                for budget in (160 * KIB, SMALL_BUDGET[c4]):
                    out.append((f"{g}/build/c4={c4}/dense={dense}/lds={budget // KIB}K", g, "build", (c4, budget, dense), False))
        for c4 in (16, 32):
            for waves in (8, 12, 16):
                for wg in (1, 2):
                    for budget in (160 * KIB, 8 * KIB):
                        out.append((f"{g}/bcast/c4={c4}/waves={waves}/wg={wg}/lds={budget // KIB}K", g, "bcast",
                                    (c4, budget, waves, wg), False))
        for mgr in (3, 16, 64, 128):
            for mgs in (0, 24):
                out.append((f"{g}/stream/rows={mgr}/src={mgs}", g, "stream", (mgr, mgs), False))
        # error paths: a row wider than its tile, a null plan buffer
        out.append((f"{g}/build/c4=128/dense=0/lds=16K", g, "build", (128, 16 * KIB, 0), False))
        out.append((f"{g}/build/c4=64/dense=0/lds=160K/null", g, "build", (64, 160 * KIB, 0), True))
        out.append((f"{g}/bcast/c4=16/waves=8/wg=2/lds=160K/null", g, "bcast", (16, 160 * KIB, 8, 2), True))
        out.append((f"{g}/stream/rows=16/src=0/null", g, "stream", (16, 0), True))
    out.append((f"clique20_uniform/build/c4=64/dense=0/lds=16K", "clique20_uniform", "build", (64, 16 * KIB, 0), False))
    g = "out_of_order"
    out.append((f"{g}/stream/rows=16/src=0", g, "stream", (16, 0), False))
    for c4 in (64, 128):
        for dense in (8, -1):
            out.append((f"{g}/build/c4={c4}/dense={dense}/lds=160K", g, "build", (c4, 160 * KIB, dense), False))
    out.append((f"{g}/build/c4=16/dense=0/lds=160K", g, "build", (16, 160 * KIB, 0), False))
    for c4 in (16, 64, 128):
        out.append((f"wide150/build/c4={c4}/dense=0/lds=160K", "wide150", "build", (c4, 160 * KIB, 0), False))
    return out


def _run(L, csr, kind, args, null):
    row_ptr, col, w, out_row = csr
    rows = len(out_row)
    head = (rows, row_ptr.ctypes.data_as(P32), col.ctypes.data_as(P32), w.ctypes.data_as(PD), out_row.ctypes.data_as(P32))
    fn = {"build": L.tal_round_plan_build, "bcast": L.tal_round_plan_build_bcast,
          "stream": L.tal_round_plan_build_stream}[kind]
    size = int(L.tal_round_plan_words(rows, len(col)))
    for _ in range(2):  # as ops.build_plan: the form's tables may need more than the first estimate
        info = _lib.RoundPlanInfo()
        blob = np.zeros(size, dtype=np.int32)
        rc = fn(*head, *args, None if null else blob.ctypes.data_as(P32), size, ctypes.byref(info))
        if null or not (rc == _lib.TAL_ERR_CAPACITY and info.words > size):
            break
        size = int(info.words)
    if rc != _lib.TAL_OK:
        return dict(rc=int(rc), error=L.tal_last_error().decode(), words=int(info.words))
    return dict(rc=0, sha256=hashlib.sha256(bytes(info) + blob[: info.words].tobytes()).hexdigest(),
                n_groups=int(info.n_groups), words=int(info.words), stream_cs=int(info.stream_cs),
                kernel_f32=ops.round_kernel_name(info), kernel_bf16=ops.round_kernel_name(info, bf16=True))


def _record():
    L = _lib.load()
    graphs = dict(_graphs(), out_of_order=_out_of_order(), wide150=_wide150())
    csr_sha = {name: hashlib.sha256(b"".join(a.tobytes() for a in csr)).hexdigest() for name, csr in graphs.items()}
    cases = {cid: _run(L, graphs[g], kind, args, null) for cid, g, kind, args, null in _cases()}
    return dict(graphs=csr_sha, cases=cases)


@pytest.fixture(scope="module")
def recorded():
    return _record()


_OK_FIELDS = ("sha256", "n_groups", "words", "stream_cs", "kernel_f32", "kernel_bf16")


def _dump(rec):
    """The fixture's text: one case per line, a built plan as [sha256, n_groups, words, stream_cs,
    kernel fp32, kernel bf16 (both without "k_round_")], a failed build as [status, info.words, message]."""
    def row(v):
        if v["rc"] != 0:
            return [v["rc"], v["words"], v["error"]]
        return [v[k].replace("k_round_", "") if k.startswith("kernel") else v[k] for k in _OK_FIELDS]
    lines = [f' {json.dumps(cid)}: {json.dumps(row(v))}' for cid, v in sorted(rec["cases"].items())]
    return ('{"graphs": ' + json.dumps(rec["graphs"], indent=1, sort_keys=True) + ',\n"cases": {\n'
            + ",\n".join(lines) + "\n}}\n")


def _load(text):
    raw = json.loads(text)
    cases = {cid: dict(zip(_OK_FIELDS, v[:4] + ["k_round_" + k for k in v[4:]]), rc=0) if len(v) == len(_OK_FIELDS)
             else dict(rc=v[0], words=v[1], error=v[2]) for cid, v in raw["cases"].items()}
    return dict(graphs=raw["graphs"], cases=cases)


@pytest.fixture(scope="module")
def golden():
    return _load(FIXTURE.read_text())


def test_graphs_are_the_recorded_ones(recorded, golden):
    assert recorded["graphs"] == golden["graphs"]


def test_plan_digests(recorded, golden):
    assert sorted(recorded["cases"]) == sorted(golden["cases"])
    bad = {cid: (got, golden["cases"][cid]) for cid, got in recorded["cases"].items() if got != golden["cases"][cid]}
    assert not bad, f"{len(bad)} of {len(recorded['cases'])} plans changed, first: {sorted(bad.items())[0]}"


def test_grid_reaches_what_it_is_meant_to(golden):
    """The fixture itself: many-group plans, both stream chunk sizes, the error paths."""
    c = golden["cases"]
    for c4, budget in SMALL_BUDGET.items():
        assert c[f"reg8x96_random/build/c4={c4}/dense=0/lds={budget // KIB}K"]["n_groups"] >= 8
    assert c[f"reg8x96_random/bcast/c4=16/waves=8/wg=2/lds=8K"]["n_groups"] >= 8
    assert {v["stream_cs"] for k, v in c.items() if "/stream/" in k and v["rc"] == 0} == {16, 32}
    nulls = [v for k, v in c.items() if k.endswith("/null")]
    assert nulls and all(v["rc"] == _lib.TAL_ERR_CAPACITY and v["words"] > 0 and "too small" in v["error"] for v in nulls)
    wide = [c[f"{g}/build/c4={c4}/dense=0/lds=16K"] for g, c4 in (
        ("reg8x96_uniform", 128), ("reg8x96_random", 128), ("clique20_uniform", 128), ("clique20_uniform", 64))]
    assert all(v["rc"] == _lib.TAL_ERR_CAPACITY and "more distinct sources" in v["error"] for v in wide)
    assert c["out_of_order/stream/rows=16/src=0"]["rc"] == _lib.TAL_ERR_INVALID
    assert {v["kernel_f32"] for v in c.values() if v["rc"] == 0} >= {
        "k_round_stream", "k_round_f32_narrow", "k_round_f32_persistent", "k_round_f32_tiled"}
    assert "k_round_wide" in {v["kernel_bf16"] for v in c.values() if v["rc"] == 0}


if __name__ == "__main__":
    FIXTURE.write_text(_dump(_record()))
    print(f"rewrote {FIXTURE}")
