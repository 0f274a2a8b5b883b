"""K3c with per-source weights against the forms such a round ran before it (not part of the product).
Three rounds: (a) BASELINE config 4 - barbell(60, 8), 128 rows of ResNet-50's width (23,573,962
elements, row stride padded to 64) - under `centrality_module_avg`'s softmax of 10 x the degree
centrality (bench.round_spec(128, 0, kind="barbell", weights="degcent")), (b) the same graph under
`weighted_module_avg`'s data-size weights (seeded lengths), and (c) a complete graph of 64 clients
at the CIFAR-CNN width (5,851,338 elements) under data-size weights.  fp32 and bf16 pools, EXACT
and FMA, three forms in one process: the weighted clique plan (tal_agg_round_clique_w_* + the rest
rows' plan), the plan default_plan returned before the weighted form existed (every
ops.WCLIQUE_DEFAULT entry off), and the clique plan's `full` sparse plan; for scale, the uniform
K3c plan of the same graph under unweighted weights (other arithmetic: timed, not compared).
Every form is warmed,
then timed `--reps` times (default 20) with HIP events, the forms alternating repetition by
repetition.  One JSON line per round, dtype and mode: median / min / max per form, whether the
forms' outputs agree bit for bit (asserted), the algorithmic bytes (sources read + rows written) and
each form's share of 8 TB/s at its median.  --out FILE also appends the lines to FILE."""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import networkx as nx  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from topology_aware_learning_amd import ops  # noqa: E402
from topology_aware_learning_amd import weights as tw  # noqa: E402
from topology_aware_learning_amd.round import csr_from_lists  # noqa: E402

RESNET50, CIFAR_CNN = 23_573_962, 5_851_338
HBM_PEAK = 8e12


def _datasize(g):
    rows = g.number_of_nodes()
    orders = [sorted(g.neighbors(i)) + [i] for i in range(rows)]
    lens = np.random.default_rng(0).integers(200, 2000, rows).tolist()
    return orders, [tw.weighted([lens[j] for j in o]) for o in orders]


ROUNDS = {
    "a": ("config4_barbell60_8_resnet50_degcent", lambda: bench.round_spec(128, 0, kind="barbell", weights="degcent"),
          RESNET50),
    "b": ("config4_barbell60_8_resnet50_datasize", lambda: _datasize(nx.barbell_graph(60, 8)), RESNET50),
    "c": ("complete64_cifar_cnn_datasize", lambda: _datasize(nx.complete_graph(64)), CIFAR_CNN),
}


def _parent_default(rp, col, w, out_rows, bf16, mode):
    """default_plan with the weighted clique form switched off: what it returned before."""
    saved = dict(ops.WCLIQUE_DEFAULT)
    try:
        for k in ops.WCLIQUE_DEFAULT:
            ops.WCLIQUE_DEFAULT[k] = False
        return ops.default_plan(rp, col, w, out_rows, bf16=bf16, mode=mode)
    finally:
        ops.WCLIQUE_DEFAULT.update(saved)


def measure(dev, name, spec, n, reps, dtype, out):
    orders, ws = spec()
    rows = len(orders)
    rp, col, w = csr_from_lists(orders, ws)
    out_rows = np.arange(rows, dtype=np.int32)
    bf16 = dtype == torch.bfloat16
    run = ops.round_bf16 if bf16 else ops.round_f32
    view = torch.int16 if bf16 else torch.int32
    ld = (n + 63) // 64 * 64
    pin = torch.empty(rows, ld, dtype=dtype, device=dev).normal_()
    pout = torch.empty_like(pin)
    wclique = ops.build_clique_plan(rp, col, w, out_rows, bf16=bf16, per_source=True)
    assert wclique is not None and ops.build_clique_plan(rp, col, w, out_rows, bf16=bf16) is None
    urp, ucol, uw = csr_from_lists(orders, [tw.unweighted(len(o)) for o in orders])
    uniform = ops.build_clique_plan(urp, ucol, uw, out_rows, bf16=bf16)
    nbytes = pin.element_size() * n * (len(set(col.tolist())) + rows)  # every source once, every row once
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for mode, mname in ((ops.MODE_EXACT, "exact"), (ops.MODE_FMA, "fma")):
        parent = _parent_default(rp, col, w, out_rows, bf16, mode)
        forms = [("wclique", wclique), ("parent_default", parent), ("full", wclique.full)]
        ref, same = None, True
        for _, p in forms:  # warm (code load, LDS attribute) and compare the outputs
            p.to(dev)
            run(pin, pout, p, n=n, mode=mode)
            torch.cuda.synchronize()
            if ref is None:
                ref = pout.clone()
            else:
                same = same and bool(torch.equal(ref.view(view), pout.view(view)))
        del ref
        forms.append(("unweighted_clique", uniform.to(dev)))
        run(pin, pout, uniform, n=n, mode=mode)
        ts = {k: [] for k, _ in forms}
        for _ in range(reps):  # forms alternate rep by rep: a clock drift does not favour one
            for k, p in forms:
                s.record()
                run(pin, pout, p, n=n, mode=mode)
                e.record()
                e.synchronize()
                ts[k].append(s.elapsed_time(e))
        res = dict(round=name, dtype="bf16" if bf16 else "f32", mode=mname, rows=rows, elements=n, reps=reps,
                   n_cliques=wclique.n_cliques, mmax=wclique.mmax, bitwise_equal=same, algorithmic_bytes=nbytes,
                   parent_default_kernel=ops.round_kernel_name(parent, bf16=bf16), parent_default_spec=parent.spec)
        for k, _ in forms:
            med = float(np.median(ts[k]))
            res[k] = dict(median_ms=round(med, 4), min_ms=round(min(ts[k]), 4), max_ms=round(max(ts[k]), 4),
                          hbm_share=round(nbytes / (med * 1e-3) / HBM_PEAK, 4))
        res["wclique_vs_parent_default"] = round(res["parent_default"]["median_ms"] / res["wclique"]["median_ms"], 3)
        res["wclique_vs_unweighted_clique"] = round(res["unweighted_clique"]["median_ms"] / res["wclique"]["median_ms"], 3)
        res["wclique_vs_full"] = round(res["full"]["median_ms"] / res["wclique"]["median_ms"], 3)
        line = json.dumps(res)
        print(line, flush=True)
        if out is not None:
            with open(out, "a") as f:
                f.write(line + "\n")
        assert same, f"{name} {res['dtype']} {mname}: the forms' outputs differ"


def main():
    dev = torch.device("cuda", 0)
    arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d  # noqa: E731
    reps, which, out = int(arg("--reps", 20)), arg("--round", "abc"), arg("--out", None)
    for key in which:
        for dtype in (torch.float32, torch.bfloat16):
            measure(dev, *ROUNDS[key], reps, dtype, out)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
