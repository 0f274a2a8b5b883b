"""K4 (fused FedProx term) timing, fp32 and bf16 (not part of the product): one client against
its K = 8 neighbors, synthetic pool rows of the ResNet-50 layout (synth.py), the norms pass
(tal_prox_norms / _bf16) and the gradient pass (tal_prox_grad / _bf16) each timed alone with
device events around the C-ABI call, buffers allocated before; the cases alternate in one
process, median of `reps` (>= 20) after warm-up.  One JSON line per case: ms, the minimum
traffic of the pass in bytes - P (K + 1) elements read, plus P written for gw in the gradient
pass (and K P more for the `grad_gwt` cases, which also write every neighbor's gradient, as
local_train's neighbors ask) - and that minimum over the time.

usage: prox_bench.py [layout [K [reps]]]   (default resnet50 8 25)
"""
import ctypes
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from topology_aware_learning_amd import _lib, synth  # noqa: E402
from topology_aware_learning_amd.arena import ModelPool, StateLayout  # noqa: E402
from topology_aware_learning_amd.prox import ProxPlan  # noqa: E402


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


class Case:
    def __init__(self, name, dtype, dev, k):
        lay = synth.get_layout(name)
        if dtype == "bfloat16":
            lay = synth.as_bf16(lay)
        self.dtype, self.k = dtype, k
        layout = StateLayout.from_layout(lay)
        names = synth.param_names(lay)
        self.plan = ProxPlan(layout, names, dev)
        pool = ModelPool(layout, k + 1, dev)
        b16 = self.plan.kind == "b16"
        assert b16 == (dtype == "bfloat16")
        seg, row, n, tdt = ((pool.b16, pool.row_b16, layout.ld_b16, torch.bfloat16) if b16 else
                            (pool.f32, pool.row_f32, layout.ld_f32, torch.float32))
        synth.fill_rows_torch(seg, lay, list(range(40, 41 + k)), dtype)
        seg[1:].mul_(0.3).add_(seg[0:1])  # neighbors near the client
        self.pool = pool
        self.elems = sum(self.plan.numels)
        self.esize = 2 if b16 else 4
        L = self.L = _lib.load()
        self.w = row(0)
        self.wt_t = [row(r) for r in range(1, k + 1)]
        self.wt = _lib.ptr_array([t.data_ptr() for t in self.wt_t])
        self.scratch = torch.empty(int(L.tal_prox_scratch_bytes(self.plan.n_chunks, k)), dtype=torch.uint8, device=dev)
        self.norms = torch.empty((k, self.plan.n_seg), dtype=torch.float32, device=dev)
        self.scale = torch.ones(1, dtype=torch.float32, device=dev)
        self.gw = torch.zeros(n, dtype=tdt, device=dev)
        self.gwt_t = [torch.zeros(n, dtype=tdt, device=dev) for _ in range(k)]
        self.gwt = _lib.ptr_array([t.data_ptr() for t in self.gwt_t])
        self.no_gwt = _lib.ptr_array([0] * k)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.b16 = b16

    def run_norms(self):
        fn = self.L.tal_prox_norms_bf16 if self.b16 else self.L.tal_prox_norms
        pl = self.plan
        _lib.check(fn(_p(self.w), self.wt, self.k, _p(pl.plan), pl.n_chunks, pl.n_seg, _p(self.scratch),
                      _p(self.norms), self.stream))

    def run_grad(self, gwt=False):
        pl = self.plan
        args = [_p(self.w), self.wt, self.k, _p(pl.plan), pl.n_chunks, pl.n_seg, _p(self.norms), _p(self.scale),
                _p(self.gw), self.gwt if gwt else self.no_gwt]
        if self.b16:
            _lib.check(self.L.tal_prox_grad_bf16(*args, None, 0, self.stream))
        else:
            _lib.check(self.L.tal_prox_grad(*args, self.stream))

    def run_grad_gwt(self):
        self.run_grad(True)

    def min_bytes(self, what):
        p, k = self.elems, self.k
        return self.esize * p * {"norms": k + 1, "grad": k + 2, "grad_gwt": 2 * k + 2}[what]


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "resnet50"
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    reps = max(20, int(sys.argv[3]) if len(sys.argv) > 3 else 25)
    if not 1 <= k <= 64:
        sys.exit("K must be 1..64 (one launch per pass)")
    dev = torch.device("cuda", 0)
    cases = [Case(name, dt, dev, k) for dt in ("float32", "bfloat16")]
    runs = [(c, what) for what in ("norms", "grad", "grad_gwt") for c in cases]
    for c in cases:
        c.run_norms()  # the gradient passes read these norms
    ts = {(c.dtype, what): [] for c, what in runs}
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(3 + reps):
        for c, what in runs:  # alternating: the cases share the machine's state
            fn = getattr(c, "run_" + what)
            s.record()
            fn()
            e.record()
            e.synchronize()
            if rep >= 3:
                ts[(c.dtype, what)].append(s.elapsed_time(e))
    for c, what in runs:
        t = ts[(c.dtype, what)]
        ms = float(np.median(t))
        mb = c.min_bytes(what)
        print(json.dumps(dict(tool="prox_bench", layout=name, dtype=c.dtype, K=k, what=what, ms=round(ms, 4),
                              ms_min=round(float(np.min(t)), 4), ms_max=round(float(np.max(t)), 4), reps=len(t),
                              params=c.elems, tensors=c.plan.n_seg, n_chunks=c.plan.n_chunks, min_bytes=mb,
                              min_bytes_per_s=round(mb / (ms * 1e-3), 1),
                              value=float(c.norms.double().sum()))), flush=True)


if __name__ == "__main__":
    main()
