"""K3c1 (clique blocks of 65..128 members, one column per lane) against the forms such a round
ran before it (not part of the product).  Three rounds of `unweighted_fl`, a complete graph and
so one clique block: (a) 66 clients and (b) 100 clients at the CIFAR-CNN width (5,851,338
elements), (c) 100 clients at ResNet-50's width (23,573,962 elements; 9.4 GB per fp32 pool), the
row stride padded to 64.  Three forms in one process: the 128-member clique plan
(build_clique_plan(max_members=128): tal_agg_round_clique_col_*), its `full` plan, and the sparse
default (build_plan(dense=0): what default_plan returned for these rounds).  Every form is warmed,
then timed `--reps` times (default 20) with HIP events, the forms alternating repetition by
repetition.  One JSON line per round, dtype and mode: median / min / max per form, whether the
forms' outputs agree bit for bit, the algorithmic bytes elem n (m + rows) (every source read
once, every row written once) and each form's share of 8 TB/s at its median.
  --round a|b|c (any subset, default abc)   --dtype f32|bf16|both (default both)   --reps N
One round's pools of one dtype are resident at a time."""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import networkx as nx  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

from topology_aware_learning_amd import ops  # noqa: E402
from topology_aware_learning_amd.round import csr_from_lists  # noqa: E402

ROUNDS = {
    "a": ("complete66_cifar_cnn", 66, 5_851_338),
    "b": ("complete100_cifar_cnn", 100, 5_851_338),
    "c": ("complete100_resnet50", 100, 23_573_962),
}
HBM_PEAK = 8e12


def measure(dev, name, m, n, bf16, reps):
    g = nx.complete_graph(m)
    orders = [sorted(g.neighbors(i)) + [i] for i in range(m)]
    ws = [[1.0 / len(o)] * len(o) for o in orders]
    rp, col, w = csr_from_lists(orders, ws)
    out_rows = np.arange(m, dtype=np.int32)
    ld = (n + 63) // 64 * 64
    dtype = torch.bfloat16 if bf16 else torch.float32
    run = ops.round_bf16 if bf16 else ops.round_f32
    pin = torch.empty(m, ld, dtype=dtype, device=dev).normal_()
    pout = torch.empty_like(pin)
    clique = ops.build_clique_plan(rp, col, w, out_rows, bf16=bf16, max_members=ops.CLIQUE_COL_MAX)
    assert clique.n_col == 1 and clique.n_cliques == 0 and clique.rest is None
    forms = [("clique128", clique), ("full", clique.full), ("sparse_default", ops.build_plan(rp, col, w, out_rows, dense=0))]
    for _, p in forms:
        p.to(dev)
    nbytes = pin.element_size() * n * (m + m)  # every source once, every row once
    bits = torch.int16 if bf16 else torch.int32
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for mode, mname in ((ops.MODE_EXACT, "exact"), (ops.MODE_FMA, "fma")):
        ref, same = None, True
        for _, p in forms:  # warm (code load, LDS attribute) and compare the outputs
            run(pin, pout, p, n=n, mode=mode)
            torch.cuda.synchronize()
            if ref is None:
                ref = pout.clone()
            else:
                same = same and bool(torch.equal(ref.view(bits), pout.view(bits)))
        del ref
        ts = {k: [] for k, _ in forms}
        for _ in range(reps):  # forms alternate rep by rep: a clock drift does not favour one
            for k, p in forms:
                s.record()
                run(pin, pout, p, n=n, mode=mode)
                e.record()
                e.synchronize()
                ts[k].append(s.elapsed_time(e))
        res = dict(round=name, dtype="bf16" if bf16 else "f32", mode=mname, rows=m, elements=n, reps=reps,
                   n_col=clique.n_col, col_mmax=clique.col_mmax, bitwise_equal=same, algorithmic_bytes=nbytes)
        for k, _ in forms:
            med = float(np.median(ts[k]))
            res[k] = dict(median_ms=round(med, 4), min_ms=round(min(ts[k]), 4), max_ms=round(max(ts[k]), 4),
                          hbm_share=round(nbytes / (med * 1e-3) / HBM_PEAK, 4))
        res["clique128_vs_sparse_default"] = round(res["sparse_default"]["median_ms"] / res["clique128"]["median_ms"], 3)
        res["clique128_vs_full"] = round(res["full"]["median_ms"] / res["clique128"]["median_ms"], 3)
        print(json.dumps(res), flush=True)


def main():
    dev = torch.device("cuda", 0)
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    which = sys.argv[sys.argv.index("--round") + 1] if "--round" in sys.argv else "abc"
    dtypes = sys.argv[sys.argv.index("--dtype") + 1] if "--dtype" in sys.argv else "both"
    for key in which:
        for bf16 in (False, True):
            if dtypes in ("both", "bf16" if bf16 else "f32"):
                measure(dev, *ROUNDS[key], bf16, reps)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
