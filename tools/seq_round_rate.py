"""K3q (the sequential round in one launch) against the K1 loop it replaces (not part of the
product).  Four rounds, every client aggregating in index order under `unweighted` weights:
  (a) ring 32 at ResNet-18's width (11,183,562 elements)
  (b) random-regular(8, 64, seed 0) at ResNet-50's width (23,573,962 elements): config 3's graph
  (c) barbell(60, 8) at ResNet-50's width: 128 clients, 61 operands in a clique row
  (d) Barabasi-Albert(33, 2, seed 0) at the CIFAR-CNN width (5,851,338 elements)
each on a ModelPool of one fp32 or one bf16 entry, in both modes.  Two forms of
RoundExecutor.run in one process: sequential=True with ops.SEQ_DEFAULT switched on for the pool's
dtype and mode (one tal_agg_round_seq_* launch) and sequential="calls" (one K1 call per client:
what sequential=True ran before K3q).  Both are warmed, then timed `--reps` times (default 20)
with HIP events, the forms alternating repetition by repetition, in place on the pool as the
repetitions before left it.  The forms' results from one common start are compared bit for bit;
a difference ends the run with status 1.  One JSON line per round, dtype and mode: median / min /
max per form, the algorithmic bytes elem n (sources + rows written) and each form's share of
8 TB/s at its median, the K1 loop's operand bytes, and whether the kernel's median beats the
loop's by more than tune_plan's 1 % margin (what sets ops.SEQ_DEFAULT).
  --round a|b|c|d (any subset, default abcd)   --dtype f32|bf16|both (default both)   --reps N"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import networkx as nx  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

from topology_aware_learning_amd import ops  # noqa: E402
from topology_aware_learning_amd.arena import ModelPool, StateLayout  # noqa: E402
from topology_aware_learning_amd.round import RoundExecutor  # noqa: E402

ROUNDS = {
    "a": ("ring32_resnet18", lambda: nx.cycle_graph(32), 11_183_562),
    "b": ("rr8_64_resnet50", lambda: nx.random_regular_graph(8, 64, seed=0), 23_573_962),
    "c": ("barbell60_8_resnet50", lambda: nx.barbell_graph(60, 8), 23_573_962),
    "d": ("ba33_2_cifar_cnn", lambda: nx.barabasi_albert_graph(33, 2, seed=0), 5_851_338),
}
HBM_PEAK = 8e12
MARGIN = 0.01  # tune_plan's
FORMS = (("seq_kernel", True), ("k1_calls", "calls"))


def measure(dev, name, make_graph, n, bf16, reps) -> bool:
    g = make_graph()
    m = g.number_of_nodes()
    orders = [sorted(g.neighbors(i)) + [i] for i in range(m)]
    ws = [[1.0 / len(o)] * len(o) for o in orders]
    layout = StateLayout.from_layout([("w", (n,), "bfloat16" if bf16 else "float32")])
    pool = ModelPool(layout, m, dev)
    seg = pool.b16 if bf16 else pool.f32
    start = torch.empty_like(seg).normal_()
    bits = torch.int16 if bf16 else torch.int32
    nnz = sum(len(o) for o in orders)
    n_src = len({j for o in orders for j in o})
    nbytes = seg.element_size() * n * (n_src + m)  # every source once, every row once
    k1_bytes = seg.element_size() * n * (nnz + m)  # every operand of every call, every row once
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ok = True
    for mode, mname in ((ops.MODE_EXACT, "exact"), (ops.MODE_FMA, "fma")):
        ops.SEQ_DEFAULT[(bf16, mode)] = True  # this process only: the form under test
        ex = RoundExecutor(pool, mode=mode)
        ref, same = None, True
        for _, sequential in FORMS:  # warm (code load, LDS attribute) and compare the results
            seg.copy_(start)
            ex.run(orders, ws, sequential=sequential)
            torch.cuda.synchronize()
            if ref is None:
                ref = seg.clone()
            else:
                same = bool(torch.equal(ref.view(bits), seg.view(bits)))
        del ref
        ts = {k: [] for k, _ in FORMS}
        for _ in range(reps):  # forms alternate rep by rep: a clock drift does not favour one
            for k, sequential in FORMS:
                s.record()
                ex.run(orders, ws, sequential=sequential)
                e.record()
                e.synchronize()
                ts[k].append(s.elapsed_time(e))
        plan = ex.seq_plan(orders, ws, list(range(m)))
        res = dict(round=name, dtype="bf16" if bf16 else "f32", mode=mname, rows=m, operands=nnz, sources=n_src,
                   max_ops=int(plan.info.max_ops), elements=n, reps=reps, bitwise_equal=same,
                   algorithmic_bytes=nbytes, k1_bytes=k1_bytes)
        for k, _ in FORMS:
            med = float(np.median(ts[k]))
            res[k] = dict(median_ms=round(med, 4), min_ms=round(min(ts[k]), 4), max_ms=round(max(ts[k]), 4),
                          hbm_share=round(nbytes / (med * 1e-3) / HBM_PEAK, 4))
        res["k1_calls_vs_seq_kernel"] = round(res["k1_calls"]["median_ms"] / res["seq_kernel"]["median_ms"], 3)
        res["kernel_wins"] = res["seq_kernel"]["median_ms"] < (1.0 - MARGIN) * res["k1_calls"]["median_ms"]
        print(json.dumps(res), flush=True)
        ok = ok and same
    return ok


def main() -> int:
    dev = torch.device("cuda", 0)
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    which = sys.argv[sys.argv.index("--round") + 1] if "--round" in sys.argv else "abcd"
    dtypes = sys.argv[sys.argv.index("--dtype") + 1] if "--dtype" in sys.argv else "both"
    ok = True
    for key in which:
        for bf16 in (False, True):
            if dtypes in ("both", "bf16" if bf16 else "f32"):
                ok = measure(dev, *ROUNDS[key], bf16, reps) and ok
                torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
