"""The clique planner's output, the variant selection and the clique entries' argument errors,
pinned (no GPU), in the manner of tests/test_round_plan_digests.py for the C-built plans.

Run as a script (`python tests/test_clique_plan_digests.py`) the file REWRITES
tests/golden/clique_plan_digests.json from the code in the tree and writes the commit it ran at
into it.  Do that only for a deliberate change of the planner or of which plan is the default:
the diff of the fixture is then part of that change's review.  The fixture was recorded before the
clique host path (ops.py's variant ladders, CliquePlan, tal_agg.hip's argument checkers) was folded
into one table and one path, so a refactor that keeps this test green kept every table byte,
every default and candidate, and every error text.

Graphs (networkx; their CSR hashed into the fixture): complete 8, 9, 64, 65, 100, 128, 129,
barbell(12, 4), (45, 2), (60, 8), (66, 3), complete 70 + complete 100, complete 20 + complete 100
+ random-regular(4, 30), ring 32 and random-regular(8, 64), each under uniform, data-size,
degree-centrality-softmax and hand-made signed per-source weights.

The fixture holds digests only (_condensed): per graph and weight kind the sha256 of the CSR and
of the entries of each section below, per bad-argument case the sha256 of the eight entries'
answers.  Recorded per graph and weight kind:
  build     ops.build_clique_plan for the four variants x bf16: "None", the exception's text, or
            [digest, n_cliques, mmax, n_col, col_mmax, clique_sources, clique_rows]; the digest is
            sha256 over the four tables, those six numbers, rest_rows and the rest and full plans'
            info + words and spec
  default   ops.default_plan for every (bf16, mode) with each of WCLIQUE_DEFAULT,
            CLIQUE_COL_DEFAULT and WCLIQUE_COL_DEFAULT wholly on and wholly off ("101": in that
            order): [plan type, spec, digest], equal results under one key (_grouped)
  cands     ops.tune_candidates likewise: [[key, spec, digest], ...] in order
  specs     ops.plan_from_spec of every clique spec that occurred: the rebuilt plan
and, for the eight tal_agg_round_clique* entries, `errors`: [rc, tal_last_error(), n passed] over
a grid of bad arguments - every argument error the four host test files try, at mmax 16 and 100,
plus n == 0 and n_cliques == 0 on misaligned pools.  The pointers are not memory and nothing may
launch: arguments an entry would accept go to it with n = 0 (_accepted)."""
import ctypes
import hashlib
import itertools
import json
import subprocess
import sys
from pathlib import Path

import networkx as nx
import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))

from topology_aware_learning_amd import _lib, ops  # noqa: E402
from topology_aware_learning_amd import weights as tw  # noqa: E402
from topology_aware_learning_amd.round import csr_from_lists  # noqa: E402

FIXTURE = Path(__file__).resolve().parent / "golden" / "clique_plan_digests.json"
MODES = {"exact": ops.MODE_EXACT, "fma": ops.MODE_FMA}
KINDS = ("uniform", "datasize", "degcent", "signed")
VARIANTS = {
    "clique": dict(),
    "wclique": dict(per_source=True),
    "clique128": dict(max_members=128),
    "wclique128": dict(per_source=True, max_members=128, wide_per_source=True),
}
DEFAULT_TABLES = ("WCLIQUE_DEFAULT", "CLIQUE_COL_DEFAULT", "WCLIQUE_COL_DEFAULT")

_GRAPHS = {
    **{f"complete{m}": (lambda m=m: nx.complete_graph(m)) for m in (8, 9, 64, 65, 100, 128, 129)},
    **{f"barbell{a}_{b}": (lambda a=a, b=b: nx.barbell_graph(a, b)) for a, b in ((12, 4), (45, 2), (60, 8), (66, 3))},
    "two_blocks": lambda: nx.disjoint_union(nx.complete_graph(70), nx.complete_graph(100)),
    "mixed": lambda: nx.disjoint_union(nx.disjoint_union(nx.complete_graph(20), nx.complete_graph(100)),
                                       nx.random_regular_graph(4, 30, seed=1)),
    "ring32": lambda: nx.cycle_graph(32),
    "regular8x64": lambda: nx.random_regular_graph(8, 64, seed=1),
}


def _csr_of(g, kind):
    """The round of graph g (neighbours ascending, then the row itself) under one weight kind;
    data-size, degree-centrality and signed weights as _round_of in the GPU clique tests."""
    nodes = sorted(g.nodes)
    orders = [sorted(g.neighbors(i)) + [i] for i in nodes]
    if kind == "uniform":
        ws = [[1.0 / len(o)] * len(o) for o in orders]
    elif kind == "datasize":
        lens = (np.random.default_rng(5).permutation(len(nodes)) * 37 + 101).tolist()
        ws = [tw.weighted([lens[j] for j in o]) for o in orders]
    elif kind == "degcent":
        cent = nx.degree_centrality(g)
        ws = [tw.centrality(o, cent, True, 10.0) for o in orders]
    else:
        per = [0.0 if j % 7 == 3 else ((-1.0) ** j) * (0.013 * (j % 11) + 0.002) for j in nodes]
        ws = [[per[j] for j in o] for o in orders]
    return (*csr_from_lists(orders, ws), np.arange(len(orders), dtype=np.int32))


def _rounds():
    out = {}
    for name, make in _GRAPHS.items():
        g = make()
        for kind in KINDS:
            out[f"{name}/{kind}"] = _csr_of(g, kind)
    return out


def _spec(p):
    return None if p.spec is None else json.dumps(p.spec)  # as text: the keys' order is pinned too


def _digest(p):
    """sha256 of everything a plan holds but its own spec (recorded beside it)."""
    if p is None:
        return None
    h = hashlib.sha256()
    if isinstance(p, ops.CliquePlan):
        for t in (p.table, p.wtable, p.col_table, p.col_wtable):
            h.update(b"none" if t is None else t.dtype.str.encode() + t.tobytes())
        h.update(json.dumps([p.n_cliques, p.mmax, p.n_col, p.col_mmax, p.clique_sources, p.clique_rows, p.rows,
                             None if p.rest_rows is None else [int(r) for r in p.rest_rows]]).encode())
        for sub in (p.rest, p.full):
            h.update(repr((_digest(sub), None if sub is None else _spec(sub))).encode())
    elif isinstance(p, ops.RoundPlan):
        h.update(bytes(p.info) + p.host[: p.info.words].tobytes())
    else:
        h.update(b"".join(np.ascontiguousarray(a).tobytes() for a in (p.row_ptr, p.col, p.w, p.out_row)))
    return h.hexdigest()


def _attempt(fn):
    try:
        return fn()
    except Exception as exc:  # noqa: BLE001 - the text is what is pinned
        return f"{type(exc).__name__}: {exc}"


def _build(csr, kw, bf16):
    p = _attempt(lambda: ops.build_clique_plan(*csr, bf16=bf16, **kw))
    if p is None or isinstance(p, str):
        return str(p)
    return [_digest(p), p.n_cliques, p.mmax, p.n_col, p.col_mmax, p.clique_sources, p.clique_rows]


def _plan_row(p):
    return p if isinstance(p, str) else [type(p).__name__, _spec(p), _digest(p)]


def _grouped(by_tag):
    """{tag: result} -> {"tag tag ...": result}, equal results under one key; a dtype and mode
    whose eight table settings agree are written "f32/exact/*", a round where all agree "*"."""
    groups = {}
    for tag, res in by_tag.items():
        groups.setdefault(json.dumps(res), []).append(tag)
    out = {}
    for res, tags in groups.items():
        if len(tags) == len(by_tag):
            out["*"] = json.loads(res)
            continue
        heads = sorted({t.rsplit("/", 1)[0] for t in tags})
        full = [h for h in heads if sum(t.startswith(h + "/") for t in tags) == 8]
        out[" ".join([h + "/*" for h in full] + [t for t in tags if t.rsplit("/", 1)[0] not in full])] = json.loads(res)
    return out


def _record_plans():
    rounds = _rounds()
    rec = dict(graphs={k: hashlib.sha256(b"".join(a.tobytes() for a in csr)).hexdigest() for k, csr in rounds.items()},
               build={}, default={}, cands={}, specs={})
    for rid, csr in rounds.items():
        for (v, kw), bf16 in itertools.product(VARIANTS.items(), (False, True)):
            rec["build"][f"{rid}/{v}/{'bf16' if bf16 else 'f32'}"] = _build(csr, kw, bf16)
    saved = {t: dict(getattr(ops, t)) for t in DEFAULT_TABLES}
    clique_specs = set()
    default = {rid: {} for rid in rounds}
    cands = {rid: {} for rid in rounds}
    try:
        for combo in itertools.product((0, 1), repeat=3):
            for t, on in zip(DEFAULT_TABLES, combo):
                for k in getattr(ops, t):
                    getattr(ops, t)[k] = bool(on)
            for rid, csr in rounds.items():
                for bf16, (mname, mode) in itertools.product((False, True), MODES.items()):
                    tag = f"{'bf16' if bf16 else 'f32'}/{mname}/{''.join(map(str, combo))}"
                    d = _attempt(lambda: ops.default_plan(*csr, bf16=bf16, mode=mode))
                    default[rid][tag] = _plan_row(d)
                    c = _attempt(lambda: ops.tune_candidates(*csr, bf16=bf16, mode=mode))
                    cands[rid][tag] = c if isinstance(c, str) else [["/".join(map(str, k)), *_plan_row(p)[1:]]
                                                                    for k, p in c]
                    found = ([] if isinstance(d, str) else [d]) + ([] if isinstance(c, str) else [p for _, p in c])
                    clique_specs.update((rid, _spec(p)) for p in found if isinstance(p, ops.CliquePlan))
    finally:
        for t, v in saved.items():
            getattr(ops, t).update(v)
    rec["default"] = {rid: _grouped(v) for rid, v in default.items()}
    rec["cands"] = {rid: _grouped(v) for rid, v in cands.items()}
    for rid, spec in sorted(clique_specs):
        rec["specs"][f"{rid}|{spec}"] = _plan_row(_attempt(lambda: ops.plan_from_spec(*rounds[rid], json.loads(spec))))
    return rec


# ---- the eight entries' argument errors ----

ENTRIES = [(f"tal_agg_round_clique{form}_{t}", "_col" in form, form.endswith("_w"), esize)
           for form in ("", "_w", "_col", "_col_w") for t, esize in (("f32", 4), ("bf16", 2))]
# (pool_in, ld_in, pool_out, ld_out, n, table_dev, n_cliques, mmax, wtab_dev)
_FIELDS = ("pin", "ld_in", "pout", "ld_out", "n", "table", "n_cliques", "mmax", "wtab")
_BASE = dict(pin=0x1000, ld_in=64, pout=0x2000, ld_out=64, n=64, table=0x3000, n_cliques=1, wtab=0x4000)
_BAD = {
    "null pool_in": dict(pin=None), "null pool_out": dict(pout=None), "null table": dict(table=None),
    "null wtab": dict(wtab=None), "in place": dict(pout=0x1000), "mmax 0": dict(mmax=0), "mmax 65": dict(mmax=65),
    "mmax 129": dict(mmax=129), "65536 blocks": dict(n_cliques=65536), "ld_in < n": dict(ld_in=63),
    "ld_out < n": dict(ld_out=63), "odd ld_in": dict(ld_in=65), "odd ld_out": dict(ld_out=65),
    "pool_in at a 2-byte offset": dict(pin=0x1002), "pool_out at a 2-byte offset": dict(pout=0x2002),
    "n 0, misaligned": dict(pin=0x1002, ld_in=65, pout=0x2006, ld_out=67, n=0),
    "no blocks, misaligned": dict(pin=0x1002, ld_in=65, pout=0x2006, ld_out=67, n_cliques=0),
}


def _error_cases():
    return {f"{label} (mmax {mmax})": tuple({**_BASE, "mmax": mmax, **bad}[f] for f in _FIELDS)
            for mmax in (16, 100) for label, bad in _BAD.items()}


def _accepted(col, wsrc, esize, args):
    """Whether the entry's documented argument rules (tal_agg.h) admit these arguments: such a
    call would launch on pointers that are not memory, so it is made with n = 0 instead."""
    pin, ld_in, pout, ld_out, n, table, n_cliques, mmax, wtab = args
    if not pin or not pout or not table or (wsrc and not wtab) or pin == pout or not 0 <= n <= min(ld_in, ld_out):
        return False
    if not 0 <= n_cliques <= 65535 or not 1 <= mmax <= (128 if col else 64):
        return False
    return col or not ((pin | pout) % (2 * esize) or ld_in % 2 or ld_out % 2)


def _record_errors():
    L = _lib.load()
    out = {}
    for cid, args in _error_cases().items():
        for name, col, wsrc, esize in ENTRIES:
            a = list(args)
            if _accepted(col, wsrc, esize, args):
                a[4] = 0
            got = []
            for mode in MODES.values():
                head = (ctypes.c_void_p(a[0]), a[1], ctypes.c_void_p(a[2]), a[3], a[4], ctypes.c_void_p(a[5]), a[6], a[7])
                rc = getattr(L, name)(*head, mode, None, *((ctypes.c_void_p(a[8]),) if wsrc else ()))
                got.append([int(rc), L.tal_last_error().decode(), a[4]])
            assert got[0] == got[1], (cid, name, got)  # the mode plays no part before the launch
            out[f"{cid}/{name}"] = got[0]
    return out


def _record():
    return dict(_record_plans(), errors=_record_errors())


def _sha(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()


def _condensed(rec):
    """What the fixture holds of a record: per round the sha256 of its CSR and of its entries in
    each of the four sections, per bad-argument case the sha256 of the eight entries' answers."""
    def of(sec, rid, sep):
        return _sha({k: v for k, v in rec[sec].items() if k == rid or k.startswith(rid + sep)})
    return dict(rounds={rid: [csr, of("build", rid, "/"), of("default", rid, "/"), of("cands", rid, "/"), of("specs", rid, "|")]
                        for rid, csr in rec["graphs"].items()},
                errors={cid: _sha({k: v for k, v in rec["errors"].items() if k.startswith(cid + "/")})
                        for cid in _error_cases()})


def _dump(rec, commit):
    """The fixture's text: one round or case per line."""
    parts = [f'"recorded_at": {json.dumps(commit)}']
    for sec, val in _condensed(rec).items():
        lines = [f" {json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(val.items())]
        parts.append(f'"{sec}": {{\n' + ",\n".join(lines) + "\n}")
    return "{" + ",\n".join(parts) + "}\n"


@pytest.fixture(scope="module")
def recorded():
    return json.loads(json.dumps(_record()))


@pytest.fixture(scope="module")
def golden():
    return json.loads(FIXTURE.read_text())


def test_graphs_are_the_recorded_ones(recorded, golden):
    got = _condensed(recorded)["rounds"]
    assert sorted(got) == sorted(golden["rounds"]) and all(v[0] == golden["rounds"][k][0] for k, v in got.items())


@pytest.mark.parametrize("section", ["build", "default", "cands", "specs", "errors"])
def test_clique_plan_digests(recorded, golden, section):
    """A mismatch names the rounds (or cases) that changed; `--full FILE` of the script writes
    every entry, to be compared between the commit the fixture was recorded at and the tree."""
    if section == "errors":
        got, want = _condensed(recorded)["errors"], golden["errors"]
    else:
        k = ("build", "default", "cands", "specs").index(section) + 1
        got = {rid: v[k] for rid, v in _condensed(recorded)["rounds"].items()}
        want = {rid: v[k] for rid, v in golden["rounds"].items()}
    assert sorted(got) == sorted(want)
    bad = sorted(k for k, v in got.items() if v != want[k])
    assert not bad, f"{section}: {len(bad)} of {len(got)} changed: {bad}"


def test_grid_reaches_what_it_is_meant_to(recorded):
    """The grid itself, as recorded from the tree (the digests tie it to the fixture): all four
    variants build somewhere and return None somewhere, default_plan reaches its six families, tune_candidates the three
    reachable clique keys, every spec that occurred round-trips, and no call of the error grid
    can have launched."""
    b = recorded["build"]
    for v in VARIANTS:
        got = [x for k, x in b.items() if f"/{v}/" in k]
        assert any(isinstance(x, list) for x in got) and "None" in got, v
    assert any(isinstance(x, list) and x[1] > 0 and x[3] > 0 for x in b.values())  # K3c and K3c1 blocks in one plan
    specs = [json.loads(v[1]) if v[1] else {} for by_tag in recorded["default"].values() for v in by_tag.values()]
    families = {("clique" if "clique" in s else "wclique" if "wclique" in s else "bcast" if s.get("bcast") else "sparse",
                 "members" in s) for s in specs}
    assert families == {("sparse", False), ("bcast", False), ("clique", False), ("clique", True),
                        ("wclique", False), ("wclique", True)}
    keys = {c[0] for by_tag in recorded["cands"].values() for v in by_tag.values() for c in v}
    # ("clique",) cannot occur: tune_candidates builds it only when default_plan's identical,
    # ungated build_clique_plan call returned None
    assert keys >= {"default", "wclique", "clique128", "wclique128"} and "clique" not in keys
    assert recorded["specs"] and all(v[0] == "CliquePlan" and json.dumps(json.loads(k.split("|", 1)[1])) == v[1]
                                   for k, v in recorded["specs"].items())
    e = recorded["errors"]
    assert all(rc == _lib.TAL_ERR_INVALID for name, (rc, _, n) in e.items() if n > 0 and "no blocks" not in name)
    assert {rc for rc, _, _ in e.values()} == {0, _lib.TAL_ERR_INVALID}
    # the asymmetry: K3c finds 65536 blocks at its launch, the column form up front
    assert "grid too large" in e["65536 blocks (mmax 16)/tal_agg_round_clique_f32"][1]
    assert "n_cliques <= 65535" in e["65536 blocks (mmax 100)/tal_agg_round_clique_col_f32"][1]


if __name__ == "__main__":
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    rec = _record()
    if "--full" in sys.argv:  # every entry, for comparing two commits; the fixture is left alone
        Path(sys.argv[sys.argv.index("--full") + 1]).write_text(json.dumps(rec, indent=0, sort_keys=True))
    else:
        FIXTURE.write_text(_dump(rec, commit))
        print(f"rewrote {FIXTURE} at {commit}")
