"""K3c on bf16 pools against the forms a bf16 clique round ran before it (not part of the product).
Two rounds: (a) BASELINE config 4 on bf16 - barbell(60, 8), 128 rows of ResNet-50's width
(23,573,962 elements, row stride padded to 64) - and (b) `unweighted_fl` over 64 clients, a
complete graph and so one clique block, at the CIFAR-CNN width (5,851,338 elements).  Three
forms, EXACT and FMA, in one process: the clique plan (tal_agg_round_clique_bf16 + the rest rows'
plan), its `full` plan (what round_bf16 ran when handed a CliquePlan before) and the sparse
default (build_plan(dense=0): what default_plan(bf16=True) returned).  Every form is warmed, then
timed `--reps` times (default 20) with HIP events, the forms alternating repetition by
repetition.  One JSON line per mode and round: median / min / max per form, whether the forms'
outputs agree bit for bit, the algorithmic bytes 2 n (sources read + rows written) and each
form's share of 8 TB/s at its median.  FMA is an HBM-bound form and is judged by that share;
EXACT is bound by its vector instructions per column pair."""
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
    "a": ("config4_barbell60_8_resnet50", lambda: nx.barbell_graph(60, 8), 23_573_962),
    "b": ("complete64_cifar_cnn", lambda: nx.complete_graph(64), 5_851_338),
}
HBM_PEAK = 8e12


def measure(dev, name, graph, n, reps):
    g = graph()
    rows = g.number_of_nodes()
    orders = [sorted(g.neighbors(i)) + [i] for i in range(rows)]
    ws = [[1.0 / len(o)] * len(o) for o in orders]
    rp, col, w = csr_from_lists(orders, ws)
    out_rows = np.arange(rows, dtype=np.int32)
    ld = (n + 63) // 64 * 64
    pin = torch.empty(rows, ld, dtype=torch.bfloat16, device=dev).normal_()
    pout = torch.empty_like(pin)
    clique = ops.build_clique_plan(rp, col, w, out_rows, bf16=True)
    forms = [("clique", clique), ("full", clique.full), ("sparse_default", ops.build_plan(rp, col, w, out_rows, dense=0))]
    for _, p in forms:
        p.to(dev)
    nbytes = 2 * n * (len(set(col.tolist())) + rows)  # every source once, every row once
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for mode, mname in ((ops.MODE_EXACT, "exact"), (ops.MODE_FMA, "fma")):
        ref, same = None, True
        for _, p in forms:  # warm (code load, LDS attribute) and compare the outputs
            ops.round_bf16(pin, pout, p, n=n, mode=mode)
            torch.cuda.synchronize()
            if ref is None:
                ref = pout.clone()
            else:
                same = same and bool(torch.equal(ref.view(torch.int16), pout.view(torch.int16)))
        del ref
        ts = {k: [] for k, _ in forms}
        for _ in range(reps):  # forms alternate rep by rep: a clock drift does not favour one
            for k, p in forms:
                s.record()
                ops.round_bf16(pin, pout, p, n=n, mode=mode)
                e.record()
                e.synchronize()
                ts[k].append(s.elapsed_time(e))
        res = dict(round=name, mode=mname, rows=rows, elements=n, reps=reps, n_cliques=clique.n_cliques,
                   mmax=clique.mmax, bitwise_equal=same, algorithmic_bytes=nbytes)
        for k, _ in forms:
            med = float(np.median(ts[k]))
            res[k] = dict(median_ms=round(med, 4), min_ms=round(min(ts[k]), 4), max_ms=round(max(ts[k]), 4),
                          hbm_share=round(nbytes / (med * 1e-3) / HBM_PEAK, 4))
        res["clique_vs_sparse_default"] = round(res["sparse_default"]["median_ms"] / res["clique"]["median_ms"], 3)
        res["clique_vs_full"] = round(res["full"]["median_ms"] / res["clique"]["median_ms"], 3)
        print(json.dumps(res), flush=True)


def main():
    dev = torch.device("cuda", 0)
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    which = sys.argv[sys.argv.index("--round") + 1] if "--round" in sys.argv else "ab"
    for key in which:
        measure(dev, *ROUNDS[key], reps)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
