"""The host-call contract of K1, the four round paths, RoundExecutor and aggregate_models.

What the Python layer hands the library is pinned here: for each case the sequence of C-ABI
entries it calls with their integer arguments (pointers as "p", a plan info as its `words`), the
sha256 of the result, and for every argument error of K1 and the round paths its exception type
and text, with one call per path that breaks two rules at once to pin which check fires first.
The expected values are tests/golden/round_calls.json, written by

    python tests/test_gpu_round_calls.py --record

on an MI355X; a change of the host layer that is meant to leave behaviour alone passes against
the fixture unchanged.  Cases that need a second GPU are run where one is visible and listed
under "skipped" in a fixture recorded without one.
"""
import hashlib
import json
import sys
from pathlib import Path

import networkx as nx
import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
for _p in (str(ROOT), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from topology_aware_learning_amd import _lib, arena, ops  # noqa: E402
from topology_aware_learning_amd.aggregate import aggregate_models  # noqa: E402
from topology_aware_learning_amd.arena import ModelPool, StateLayout  # noqa: E402
from topology_aware_learning_amd.round import RoundExecutor, csr_from_lists  # noqa: E402

FIXTURE = ROOT / "tests" / "golden" / "round_calls.json"
GOLDEN = json.loads(FIXTURE.read_text()) if FIXTURE.exists() else {"cases": {}, "errors": {}, "skipped": []}

N, LD, ROWS = 70, 72, 12  # whole float4 columns and a 2-column tail; a 12-row ring
DTYPES = {"f32": torch.float32, "b16": torch.bfloat16, "i64": torch.int64}
ROUND = {"f32": ops.round_f32, "b16": ops.round_bf16, "i64": ops.round_i64}
SEQ = {"f32": ops.round_seq_f32, "b16": ops.round_seq_bf16, "i64": ops.round_seq_i64}


# ---------------------------------------------------------------------------------------------
# recording
# ---------------------------------------------------------------------------------------------
def _arg(a):
    if isinstance(a, (bool, int)):
        return int(a)
    info = getattr(a, "_obj", None)  # ctypes.byref(...)
    if isinstance(info, (_lib.RoundPlanInfo, _lib.SeqPlanInfo)):
        return int(info.words)
    return "p"


class _Proxy:
    """The loaded library with every call (but tal_last_error) appended to `log`."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name == "tal_last_error":
            return fn

        def call(*args):
            self._log.append([name] + [_arg(a) for a in args])
            return fn(*args)

        return call


def _sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _mode_kw(dt, mode):
    return {} if dt == "i64" else {"mode": mode}


def _pool(dt, rows, ld, dev, seed=0):
    rng = np.random.default_rng(seed)
    if dt == "i64":
        return torch.from_numpy(rng.integers(-1000, 1000, (rows, ld))).to(dev)
    return torch.from_numpy(rng.standard_normal((rows, ld)).astype(np.float32)).to(DTYPES[dt]).to(dev)


def _ring(rows=ROWS):
    orders = [sorted([(i - 1) % rows, (i + 1) % rows]) + [i] for i in range(rows)]
    return orders, [[1.0 / 3] * 3 for _ in orders]


def _csr(orders, weights):
    return (*csr_from_lists(orders, weights), np.arange(len(orders), dtype=np.int32))


def _clique_graph(members):
    """A complete graph of `members` nodes and, for 8, a 4-ring beside it (the rest rows)."""
    g = nx.complete_graph(members)
    if members == 8:
        g.add_edges_from((8 + i, 8 + (i + 1) % 4) for i in range(4))
    return g


def _clique_pool(dt, rows, ld, dev):
    import _clique

    if dt == "i64":
        return _pool(dt, rows, ld, dev, seed=3)
    bits, _ = _clique.inputs(rows, N, 3, dt == "b16")
    pin = torch.zeros(rows, ld, dtype=DTYPES[dt], device=dev)
    pin[:, :N] = _clique.to_dev(bits, dt == "b16", dev)
    return pin


def _bn_modules(dev, k=3):
    torch.manual_seed(7)
    return [torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.BatchNorm1d(5)).to(dev) for _ in range(k)]


def _bf16_modules(dev, k=3):
    torch.manual_seed(8)
    return [torch.nn.Linear(6, 5).to(torch.bfloat16).to(dev) for _ in range(k)]


def _call_cases(dev):
    """(case id, thunk -> tensors to hash); plans are built before the log starts where the case
    is about a launch, inside it where the case is about the executor or the app call."""
    import _clique

    cases = []
    orders, weights = _ring()
    csr = _csr(orders, weights)
    for dt in DTYPES:
        kw = _mode_kw(dt, ops.MODE_EXACT)

        def out_of_place(plan, dt=dt, kw=kw):
            pin, pout = _pool(dt, ROWS, LD, dev), torch.zeros(ROWS, LD, dtype=DTYPES[dt], device=dev)
            return lambda: [ROUND[dt](pin, pout, plan, n=N, **kw)]

        cases.append((f"sparse/{dt}", out_of_place(ops.build_plan(*csr, dense=0))))
        cases.append((f"rowcall/{dt}", out_of_place(ops.row_call_plan(*csr))))

        def seq(dt=dt, kw=kw, view=False):
            pool = _pool(dt, ROWS, LD + 8 * view, dev)[:, :LD]
            plan = ops.build_seq_plan(*csr)
            return lambda: [SEQ[dt](pool, plan, n=N, **kw)]

        cases.append((f"seq/{dt}", seq()))
        if dt == "f32":
            cases.append((f"seq_row_view/{dt}", seq(view=True)))
        for members, kind, ld in ((8, "uniform", LD), (8, "datasize", LD), (65, "uniform", LD), (65, "datasize", LD),
                                  (8, "uniform", 71)):
            g = _clique_graph(members)
            c_orders, c_w = _clique.round_of(g, kind, n=N)
            per = kind == "datasize"
            wide = dict(max_members=128, wide_per_source=per) if members > 64 else {}
            plan = ops.build_clique_plan(*_csr(c_orders, c_w), bf16=dt == "b16", per_source=per, **wide)
            assert plan is not None and (plan.n_col if members > 64 else plan.n_cliques) == 1
            assert (plan.rest is not None) == (members == 8) and (plan.wtable is not None) == per

            def clique(plan=plan, rows=g.number_of_nodes(), ld=ld, dt=dt):
                pin = _clique_pool(dt, rows, ld, dev)
                pout = torch.zeros_like(pin)
                out = []
                for mode in _clique.MODES if dt != "i64" else [None]:
                    out.append(ROUND[dt](pin, pout, plan, n=N, **_mode_kw(dt, mode)).clone())
                return out

            cases.append((f"clique{members}/{kind}/ld{ld}/{dt}", lambda c=clique: c()))

    layouts = {"f32+i64": (StateLayout.from_state_dict(_bn_modules("cpu", 1)[0].state_dict()), ops.MODE_EXACT),
               "b16": (StateLayout.from_layout([("w", (N,), "bfloat16")]), ops.MODE_FMA)}
    c_orders, c_w = _clique.round_of(_clique_graph(8), "uniform", n=N)
    for lname, (lay, mode) in layouts.items():
        for ename, kw, run_kw, rnd in (
                ("double_buffered", dict(placement_trials=1), {}, (orders, weights)),
                ("in_place", dict(placement_trials=1, double_buffer=False), {}, (orders, weights)),
                ("scratch_copy_back", dict(placement_trials=1, double_buffer=False), {}, (c_orders, c_w)),
                ("sequential", dict(), dict(sequential=True), (orders, weights)),
                ("sequential_calls", dict(), dict(sequential="calls"), (orders, weights))):

            def executor(lay=lay, mode=mode, kw=kw, run_kw=run_kw, rnd=rnd):
                pool = ModelPool(lay, ROWS, dev)
                for k, (g, t, n) in enumerate(pool.segments()):
                    t[:, :n] = _pool(g, ROWS, n, dev, seed=10 + k)
                ex = RoundExecutor(pool, mode=mode, **kw)
                for _ in range(2):  # the second round finds the plan and the spare in place
                    ex.run(*rnd, **run_kw)
                return [t for _, t, _ in pool.segments()]

            cases.append((f"executor/{ename}/{lname}", executor))

    def app(make, bound):
        def run():
            mods = make(dev)
            if bound:
                pool = ModelPool(StateLayout.from_state_dict(mods[0].state_dict()), len(mods), dev)
                for r, m in enumerate(mods):
                    pool.bind(m, r)
            aggregate_models(mods, [0.5, 0.25, 0.25], mods[-1])
            return list(mods[-1].state_dict().values())
        return run

    cases += [("app/pool_bound/f32+i64", app(_bn_modules, True)), ("app/unbound/f32+i64", app(_bn_modules, False)),
              ("app/pool_bound/b16", app(_bf16_modules, True)), ("app/unbound/b16", app(_bf16_modules, False))]
    return cases


def _error_cases(dev):
    """(case id, thunk that raises).  Every thunk fails its argument checks: none launches."""
    orders, weights = _ring()
    csr = _csr(orders, weights)
    two = torch.cuda.device_count() >= 2
    other = torch.device("cuda", 1) if two else None
    cases, need_two = [], []

    def t(dt="f32", shape=(N,), device=dev):
        return torch.zeros(shape, dtype=DTYPES[dt], device=device)

    def k1(fn, xs, ws, out):
        return lambda: fn(xs, ws, out)

    f = ops.agg_f32
    cases += [
        ("k1/out_not_tensor", k1(f, [t()], [1.0], None)),
        ("k1/out_cpu", k1(f, [t()], [1.0], t(device="cpu"))),
        ("k1/out_dtype/f32", k1(f, [t()], [1.0], t("i64"))),
        ("k1/out_dtype/b16", k1(ops.agg_bf16, [t()], [1.0], t("f32"))),
        ("k1/out_dtype/i64", k1(ops.agg_i64, [t()], [1.0], t("f32"))),
        ("k1/out_noncontiguous", k1(f, [t()], [1.0], t(shape=(2 * N,))[::2])),
        ("k1/no_operands", k1(f, [], [], t())),
        ("k1/weight_count", k1(f, [t(), t()], [1.0], t())),
        ("k1/operand_not_tensor", k1(f, [t(), None], [0.5, 0.5], t())),
        ("k1/operand_cpu", k1(f, [t(), t(device="cpu")], [0.5, 0.5], t())),
        ("k1/operand_dtype/f32", k1(f, [t(), t("b16")], [0.5, 0.5], t())),
        ("k1/operand_dtype/b16", k1(ops.agg_bf16, [t("f32")], [1.0], t("b16"))),
        ("k1/operand_dtype/i64", k1(ops.agg_i64, [t("f32")], [1.0], t("i64"))),
        ("k1/operand_noncontiguous", k1(f, [t(shape=(2 * N,))[::2]], [1.0], t())),
        ("k1/operand_length", k1(f, [t(), t(shape=(N + 1,))], [0.5, 0.5], t())),
        ("k1/two_rules/out_dtype+no_operands", k1(f, [], [], t("i64"))),
        ("k1/two_rules/weight_count+operand_cpu", k1(f, [t(device="cpu")], [], t())),
    ]
    if two:
        cases.append(("k1/two_devices", k1(f, [t(device=other)], [1.0], t())))
    need_two.append("k1/two_devices")

    def p(dt="f32", rows=ROWS, device=dev):
        return torch.zeros(rows, LD, dtype=DTYPES[dt], device=device)

    plans = {"sparse": ops.build_plan(*csr, dense=0), "rowcall": ops.row_call_plan(*csr)}
    import _clique

    plans["clique"] = ops.build_clique_plan(*_csr(*_clique.round_of(_clique_graph(8), "uniform", n=N)))
    for path, plan in plans.items():
        def rnd(pin, pout, fn=ops.round_f32, plan=plan, **kw):
            return lambda: fn(pin, pout, plan, n=N, **kw)

        same = p()
        cases += [
            (f"{path}/pool_in_not_tensor", rnd(None, p())),
            (f"{path}/pool_in_cpu", rnd(p(device="cpu"), p())),
            (f"{path}/pool_out_cpu", rnd(p(), p(device="cpu"))),
            (f"{path}/dtype/f32", rnd(p("b16"), p("b16"))),
            (f"{path}/dtype/b16", rnd(p(), p(), fn=ops.round_bf16)),
            (f"{path}/dtype/i64", rnd(p(), p(), fn=ops.round_i64)),
            (f"{path}/pool_out_dtype", rnd(p(), p("i64"))),
            (f"{path}/pool_in_noncontiguous", rnd(p()[:, :N], p())),
            (f"{path}/pool_out_noncontiguous", rnd(p(), p()[:, :N])),
            (f"{path}/pool_in_1d", rnd(t(), p())),
            (f"{path}/pool_out_1d", rnd(p(), t())),
            (f"{path}/reads_beyond", rnd(p(rows=6), p())),
            (f"{path}/writes_beyond", rnd(p(), p(rows=6))),
            (f"{path}/two_rules/pool_in_1d+pool_out_dtype", rnd(t(), p("i64"))),
            (f"{path}/two_rules/pool_in_cpu+pool_out_1d", rnd(p(device="cpu"), t())),
        ]
        if path != "sparse":  # a sparse single-group round may run in place
            small = p(rows=6)
            oned = t()
            cases += [(f"{path}/aliased", rnd(same, same)),
                      (f"{path}/two_rules/aliased+rows_beyond", rnd(small, small)),
                      (f"{path}/two_rules/aliased+1d", rnd(oned, oned))]
        if two:
            cases.append((f"{path}/two_devices", rnd(p(), p(device=other))))
            cases.append((f"{path}/two_rules/two_devices+writes_beyond", rnd(p(), p(rows=6, device=other))))
        need_two += [f"{path}/two_devices", f"{path}/two_rules/two_devices+writes_beyond"]

    sp = ops.build_seq_plan(*csr)

    def seq(pool, plan=sp, fn=ops.round_seq_f32, n=N):
        return lambda: fn(pool, plan, n=n)

    cases += [
        ("seq/not_a_seq_plan", seq(p(), plan=plans["sparse"])),
        ("seq/pool_not_tensor", seq(None)),
        ("seq/pool_cpu", seq(p(device="cpu"))),
        ("seq/dtype/f32", seq(p("b16"))),
        ("seq/dtype/b16", seq(p(), fn=ops.round_seq_bf16)),
        ("seq/dtype/i64", seq(p(), fn=ops.round_seq_i64)),
        ("seq/pool_1d", seq(t())),
        ("seq/column_stride", seq(torch.zeros(LD, ROWS, device=dev).t())),
        ("seq/n_above", seq(p(), n=LD + 1)),
        ("seq/n_negative", seq(p(), n=-1)),
        ("seq/rows_beyond", seq(p(rows=6))),
        ("seq/two_rules/not_a_seq_plan+pool_cpu", seq(p(device="cpu"), plan=plans["sparse"])),
        ("seq/two_rules/dtype+1d", seq(t("b16"))),
        ("seq/two_rules/n_above+rows_beyond", seq(p(rows=6), n=LD + 1)),
    ]
    return cases, ([] if two else need_two)


def collect(dev) -> dict:
    """Every case run once: {"cases": {id: {"calls", "sha256"}}, "errors": {id: [type, text]},
    "skipped": [ids that need a second GPU]}."""
    real = _lib.load()
    log: list = []
    proxy = _Proxy(real, log)
    orig = _lib.load
    out = {"cases": {}, "errors": {}, "skipped": []}
    call_cases = _call_cases(dev)
    error_cases, out["skipped"] = _error_cases(dev)
    _lib.load = lambda path=None: proxy
    try:
        for cid, thunk in call_cases:
            log.clear()
            got = thunk()
            torch.cuda.synchronize(dev)
            out["cases"][cid] = {"calls": [list(c) for c in log], "sha256": _sha(*got)}
        for cid, thunk in error_cases:
            log.clear()
            try:
                thunk()
            except (ValueError, TypeError) as exc:
                out["errors"][cid] = [type(exc).__name__, str(exc)]
            else:
                out["errors"][cid] = ["no error", ""]
            assert not log, f"{cid}: an argument error after a library call {log}"
    finally:
        _lib.load = orig
        arena.uninstall_hooks()  # (the pool-bound app cases installed them)
    return out


# ---------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def observed(cuda):
    return collect(cuda)


@pytest.mark.gpu
def test_fixture_covers_every_case(observed):
    assert GOLDEN["cases"], f"{FIXTURE} is missing: record it with --record"
    assert sorted(observed["cases"]) == sorted(GOLDEN["cases"])
    want = set(GOLDEN["errors"]) | set(GOLDEN["skipped"])
    assert set(observed["errors"]) | set(observed["skipped"]) == want
    assert not [c for c, (kind, _) in GOLDEN["errors"].items() if kind == "no error"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(GOLDEN["cases"]))
def test_calls_and_result(observed, case):
    got, want = observed["cases"][case], GOLDEN["cases"][case]
    print(case, got["calls"], got["sha256"])
    assert got["calls"] == want["calls"]
    assert got["sha256"] == want["sha256"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(GOLDEN["errors"]))
def test_argument_error(observed, case):
    if case not in observed["errors"]:
        assert case in observed["skipped"]  # recorded with two GPUs, run with one
        return
    print(case, observed["errors"][case])
    assert observed["errors"][case] == GOLDEN["errors"][case]


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_round_calls.py --record")
    _lib.load()
    FIXTURE.write_text(json.dumps(collect(torch.device("cuda", 0)), indent=1, sort_keys=True) + "\n")
    print(f"wrote {FIXTURE}")
