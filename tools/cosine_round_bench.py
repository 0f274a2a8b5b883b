"""K2r timing (not part of the product): a round's cosine similarities on BASELINE config 3's
setting - 64 ResNet-50 rows, nx.random_regular_graph(8, 64, seed=0), all 512 ordered pairs - two
ways, alternating in one process after a warm-up, ten repetitions each:
  (A) what the batched `*_sim` round did before the round form: 64 ops.cosine calls of 8 pairs
      sharing `a`, each followed by .cpu() (a device synchronise);
  (B) one ops.cosine_round and one .cpu().
Host clock around the synchronised work, device events for the GPU time, and the 512 values of A
and B compared bit for bit.  One JSON line.

usage: cosine_round_bench.py [layout [degree [clients [dtype]]]]   (default resnet50 8 64 float32;
e.g. vit_b16 2 16; dtype bfloat16: the layout of model.to(torch.bfloat16), synth.as_bf16, through
the bf16 entry points)
"""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import networkx as nx  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

from topology_aware_learning_amd import ops, synth  # noqa: E402
from topology_aware_learning_amd.arena import ModelPool, StateLayout  # noqa: E402

REPS = 10


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "resnet50"
    degree = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    dtype = sys.argv[4] if len(sys.argv) > 4 else "float32"
    if dtype not in ("float32", "bfloat16"):
        sys.exit(f"dtype must be float32 or bfloat16, not {dtype}")
    dev = torch.device("cuda", 0)
    lay = synth.get_layout(name)
    if dtype == "bfloat16":
        lay = synth.as_bf16(lay)
    layout = StateLayout.from_layout(lay)
    segs = layout.param_segments(synth.param_names(lay))
    plan = ops.build_cosine_plan(segs, threads=max(1, min(torch.get_num_threads(), 1024)))
    pool = ModelPool(layout, n, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    seg, row, n_el = ((pool.f32, pool.row_f32, layout.n_f32) if dtype == "float32" else
                      (pool.b16, pool.row_b16, layout.n_b16))
    seg.normal_(generator=g)
    seg[1:].mul_(0.3).add_(seg[0:1])  # models similar to one another, as after training
    graph = nx.random_regular_graph(degree, n, seed=0)
    nbrs = [sorted(graph.neighbors(i)) for i in range(n)]
    pairs = [(i, j) for i in range(n) for j in nbrs[i]]
    table = ops.build_cosine_round(pairs, n)
    rows = [row(i) for i in range(n)]
    view = seg[:, :n_el]

    def form_a():
        vals = []
        for i in range(n):
            vals += ops.cosine([rows[i]] * len(nbrs[i]), [rows[j] for j in nbrs[i]], plan).cpu().tolist()
        return vals

    def form_b():
        return ops.cosine_round(view, table, plan).cpu().tolist()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        s.record()
        vals = fn()
        e.record()
        e.synchronize()
        return (time.perf_counter() - t0) * 1e3, s.elapsed_time(e), vals

    va, vb = form_a(), form_b()  # warm-up
    form_a(), form_b()
    ta, tb, ga, gb = [], [], [], []
    for _ in range(REPS):
        h, d, va = timed(form_a)
        ta.append(h)
        ga.append(d)
        h, d, vb = timed(form_b)
        tb.append(h)
        gb.append(d)
    bits = lambda v: np.asarray(v, dtype=np.float32).view(np.uint32)  # noqa: E731
    same = bool(np.array_equal(bits(va), bits(vb)))
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    print(json.dumps(dict(
        layout=name, dtype=dtype, clients=n, degree=degree, ordered_pairs=len(pairs), unique_pairs=int(table.info.n_unique),
        groups=int(table.info.n_groups), batches=int(table.info.n_batches), threads=plan.threads,
        a_host_ms=[round(x, 4) for x in ta], b_host_ms=[round(x, 4) for x in tb],
        a_host_ms_median=med(ta), a_host_ms_min=round(min(ta), 4), b_host_ms_median=med(tb),
        a_gpu_ms_median=med(ga), b_gpu_ms_median=med(gb), ratio_of_medians=round(float(np.median(ta) / np.median(tb)), 3),
        bitwise_a_equals_b=same, b_median_below_a_min=bool(np.median(tb) < min(ta)),
        params=n_el, tensors=len(segs), n_outputs=int(plan.host[1]))), flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
