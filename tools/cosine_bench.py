"""K2 (exact-order cosine) timing on BASELINE config 3's layout (not part of the product):
ResNet-50, one client vs its 8 neighbors (sim_centrality_module_avg's K2 launch), checked bit
for bit against the C oracle on the first pair at full size.  One JSON line.

usage: cosine_bench.py [layout [dtype]]   (default resnet50 float32; dtype bfloat16: the layout of
model.to(torch.bfloat16), synth.as_bf16, through the bf16 entry point; the oracle then runs on
the widened rows)
"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle  # noqa: E402  (the checker)
from topology_aware_learning_amd import ops, synth  # noqa: E402
from topology_aware_learning_amd.arena import ModelPool, StateLayout  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    lay = synth.get_layout(sys.argv[1] if len(sys.argv) > 1 else "resnet50")
    dtype = sys.argv[2] if len(sys.argv) > 2 else "float32"
    if dtype not in ("float32", "bfloat16"):
        sys.exit(f"dtype must be float32 or bfloat16, not {dtype}")
    if dtype == "bfloat16":
        lay = synth.as_bf16(lay)
    layout = StateLayout.from_layout(lay)
    segs = layout.param_segments(synth.param_names(lay))
    plan = ops.build_cosine_plan(segs)
    pool = ModelPool(layout, 9, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    seg, row = (pool.f32, pool.row_f32) if dtype == "float32" else (pool.b16, pool.row_b16)
    seg.normal_(generator=g)
    seg[1:].mul_(0.3).add_(seg[0:1])  # neighbors similar to the client
    a = [row(0)] * 8
    b = [row(j) for j in range(1, 9)]
    out = ops.cosine(a, b, plan)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(10):
        s.record()
        ops.cosine(a, b, plan)
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    ref = oracle.cosine_model(row(0).float().cpu().numpy(), row(1).float().cpu().numpy(), segs)
    got = out[0].cpu().numpy()
    print(json.dumps(dict(layout=sys.argv[1] if len(sys.argv) > 1 else "resnet50", dtype=dtype, pairs=8,
                          ms=round(float(np.median(ts)), 4), values=[float(x) for x in out.cpu()],
                          bitwise_vs_oracle_pair0=bool(got.view(np.uint32) == ref.view(np.uint32)),
                          params=layout.n_f32 + layout.n_b16, tensors=len(segs), n_chunks=plan.n_chunks)), flush=True)


if __name__ == "__main__":
    main()
