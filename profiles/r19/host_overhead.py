"""Host overhead of the per-call paths: the parent commit's package against the working tree's,
alternating rep by rep in one process; parent against parent gives the spread.

    python profiles/r19/host_overhead.py PARENT_DIR OUT.json

PARENT_DIR holds the parent commit's topology_aware_learning_amd directory (with its built
libraries) renamed to tal_parent, so both packages load side by side."""
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import networkx as nx
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, sys.argv[1])

REPS, CALLS = 30, 20
dev = torch.device("cuda", 0)


def load(name):
    m = {k: importlib.import_module(f"{name}.{k}") for k in ("arena", "aggregate", "round", "ops")}
    m["ops"]._lib.load()
    return m


def modules(k):
    torch.manual_seed(1)
    return [torch.nn.Sequential(torch.nn.Conv2d(3, 64, 3), torch.nn.BatchNorm2d(64), torch.nn.Conv2d(64, 128, 3),
                                torch.nn.BatchNorm2d(128), torch.nn.Flatten(), torch.nn.Linear(128, 256)).to(dev)
            for _ in range(k)]


def setup(pkg):
    A, G, R = pkg["arena"], pkg["aggregate"], pkg["round"]
    w9 = [1.0 / 9] * 9
    bound = modules(9)
    lay = A.StateLayout.from_state_dict(bound[0].state_dict())
    pool = A.ModelPool(lay, 9, dev)
    for r, m in enumerate(bound):
        pool.bind(m, r)
    unbound = modules(9)
    g = nx.random_regular_graph(8, 64, seed=0)
    orders = [sorted(g.neighbors(i)) + [i] for i in range(64)]
    ws = [[1.0 / 9] * 9 for _ in orders]
    rpool = A.ModelPool(lay, 64, dev)
    ex = R.RoundExecutor(rpool, placement_trials=1)
    plan = ex.plan(orders, ws, list(range(64)))
    ring = [sorted([(i - 1) % 12, (i + 1) % 12]) + [i] for i in range(12)]
    rw = [[1.0 / 3] * 3 for _ in ring]
    spool = A.ModelPool(lay, 12, dev)
    sx = R.RoundExecutor(spool)
    return {
        "app_pool_bound": lambda: G.aggregate_models(bound, w9, bound[-1]),
        "app_unbound_gpu": lambda: G.aggregate_models(unbound, w9, unbound[-1]),
        "executor_prebuilt_plan": lambda: ex.run(orders, ws, plan=plan),
        "executor_sequential_calls": lambda: sx.run(ring, rw, sequential="calls"),
    }


def timed(fn):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize(dev)
    return 1e6 * (time.perf_counter() - t) / CALLS


def main():
    variants = {"parent_a": setup(load("tal_parent")), "new": setup(load("topology_aware_learning_amd"))}
    variants["parent_b"] = variants["parent_a"]
    order = ["parent_a", "new", "parent_b"]
    out = {}
    for path in variants["new"]:
        for v in ("parent_a", "new"):
            for _ in range(3):
                variants[v][path]()  # warm
        ts = {v: [] for v in order}
        for rep in range(REPS):
            for v in order[rep % 3:] + order[:rep % 3]:
                ts[v].append(timed(variants[v][path]))
        med = {v: statistics.median(x) for v, x in ts.items()}
        parent = statistics.median(ts["parent_a"] + ts["parent_b"])
        out[path] = dict(us_per_call=dict({k: round(x, 2) for k, x in med.items()}, parent=round(parent, 2)),
                         spread_us=round(abs(med["parent_a"] - med["parent_b"]), 2),
                         new_minus_parent_us=round(med["new"] - parent, 2), reps=REPS, calls_per_rep=CALLS)
        print(path, json.dumps(out[path]), flush=True)
    Path(sys.argv[2]).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
