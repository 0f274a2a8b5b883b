"""K3m (TAL_MODE_MATRIX, the round on the matrix cores) against the FMA-mode default plan of the
same round on bf16 pools (not part of the product).  Five rounds:
  (a) config 5: SBM 8 x 32 at ViT-B/16's width (86,567,656 elements), unweighted
  (b) config 5 with degree-centrality weights (per-operand weights: three A planes)
  (c) config 4: barbell(60, 8) at ResNet-50's width (23,573,962 elements), unweighted
  (d) complete 100 at ResNet-50's width, unweighted (`unweighted_fl` over 100 clients)
  (e) complete 700 at the CIFAR-CNN width (5,851,338 elements), unweighted (`unweighted_fl`, 700 clients)
A third form where the round has rows with identical operands: the matrix mode's shared plan
(K3ms, default_plan(mode=MODE_MATRIX, shared=True): one sum per row class, the other rows in FMA
mode); a round without a class has no such plan and prints no "shared" figures.
All forms run ops.round_pool out of place between the same two pools; each is warmed, then timed
`--reps` times (default 10) with HIP events, the forms alternating repetition by repetition.  One
JSON line per round: median / min / max per form, the algorithmic bytes (every distinct source
read once, every row written once) and each form's share of 8 TB/s at its median, the FMA form's
kernel, and the largest |matrix - fma| over the output in units of the matrix mode's rounding step
2^-8 |fma| (the two modes are not bit-comparable; this is a sanity figure, the bound is tested in
tests/test_gpu_matrix_round.py).
  --round a|b|c|d|e (any subset, default abcde)   --reps N"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import networkx as nx  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from topology_aware_learning_amd import ops  # noqa: E402
from topology_aware_learning_amd.round import csr_from_lists  # noqa: E402

VIT_B16, RESNET50, CIFAR_CNN = 86_567_656, 23_573_962, 5_851_338
HBM_PEAK = 8e12


def _complete(m):
    g = nx.complete_graph(m)
    orders = [sorted(g.neighbors(i)) + [i] for i in range(m)]
    return orders, [[1.0 / m] * m for _ in orders]


ROUNDS = {
    "a": ("c5_sbm256_vit_unweighted", lambda: bench.round_spec(256, 0, kind="sbm"), VIT_B16),
    "b": ("c5_sbm256_vit_degcent", lambda: bench.round_spec(256, 0, kind="sbm", weights="degcent"), VIT_B16),
    "c": ("c4_barbell60_8_resnet50", lambda: bench.round_spec(128, 0, kind="barbell"), RESNET50),
    "d": ("complete100_resnet50", lambda: _complete(100), RESNET50),
    "e": ("complete700_cifar_cnn", lambda: _complete(700), CIFAR_CNN),
}


def measure(dev, name, spec, n, reps) -> None:
    orders, ws = spec()
    m = len(orders)
    rp, col, w = csr_from_lists(orders, ws)
    out = np.arange(m, dtype=np.int32)
    plans = {"fma": ops.default_plan(rp, col, w, out, bf16=True, mode=ops.MODE_FMA).to(dev),
             "matrix": ops.default_plan(rp, col, w, out, bf16=True, mode=ops.MODE_MATRIX).to(dev)}
    modes = {"fma": ops.MODE_FMA, "matrix": ops.MODE_MATRIX, "shared": ops.MODE_MATRIX}
    sp = ops.default_plan(rp, col, w, out, bf16=True, mode=ops.MODE_MATRIX, shared=True)
    if isinstance(sp, ops.SharedPlan):  # a round without a class: the same MatrixPlan, not timed twice
        plans["shared"] = sp.to(dev)
    ld = -(-n // 64) * 64
    pin = torch.empty((m, ld), dtype=torch.bfloat16, device=dev).normal_()
    pout = torch.empty_like(pin)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = dict(round=name, rows=m, operands=len(col), sources=len(set(col.tolist())), elements=n, reps=reps,
               fma_kernel=ops.round_kernel_name(plans["fma"], bf16=True),
               matrix_kblocks=int(plans["matrix"].info.n_kblocks), matrix_groups=int(plans["matrix"].info.n_groups))
    if "shared" in plans:
        i = plans["shared"].info
        res.update(shared_classes=int(i.n_classes), shared_class_rows=int(i.n_out), shared_class_sources=int(i.n_src),
                   shared_rest_rows=len(plans["shared"].rest_index))
    nbytes = 2 * n * (res["sources"] + m)
    ref = None
    for k in plans:  # warm (code load) and compare with the FMA form
        pout.zero_()
        ops.round_pool(pin, pout, plans[k], n, modes[k])
        torch.cuda.synchronize()
        head = pout[:, : min(n, 1 << 20)].float()
        if ref is None:
            ref = head
        else:
            step = ref.abs() * 2.0 ** -8
            ok = step > 0
            key = "max_diff_in_rounding_steps" + "_shared" * (k == "shared")
            res[key] = round(float(((head - ref).abs()[ok] / step[ok]).max()), 3)
    del ref, head
    ts = {k: [] for k in plans}
    for _ in range(reps):  # forms alternate rep by rep: a clock drift does not favour one
        for k in plans:
            s.record()
            ops.round_pool(pin, pout, plans[k], n, modes[k])
            e.record()
            e.synchronize()
            ts[k].append(s.elapsed_time(e))
    for k in plans:
        med = float(np.median(ts[k]))
        res[k] = dict(median_ms=round(med, 4), min_ms=round(min(ts[k]), 4), max_ms=round(max(ts[k]), 4),
                      hbm_share=round(nbytes / (med * 1e-3) / HBM_PEAK, 4))
    res["algorithmic_bytes"] = nbytes
    res["fma_vs_matrix"] = round(res["fma"]["median_ms"] / res["matrix"]["median_ms"], 3)
    if "shared" in plans:
        res["fma_vs_shared"] = round(res["fma"]["median_ms"] / res["shared"]["median_ms"], 3)
    print(json.dumps(res), flush=True)


def main() -> int:
    dev = torch.device("cuda", 0)
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    which = sys.argv[sys.argv.index("--round") + 1] if "--round" in sys.argv else "abcde"
    for key in which:
        measure(dev, *ROUNDS[key], reps)
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
