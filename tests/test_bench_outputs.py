"""bench.py's plain run, --full and --dump-outputs.

The dump is the output pool of the last timed step.  The inputs are synth's seeded models, so the
expected dump is the C oracle's round applied warmup + steps times to the same models built on
the host: a plain run and a --full run (which spends one more round on its parity check, into the
pool the first step overwrites) must both write exactly that."""
import json
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle
from conftest import ROOT
from topology_aware_learning_amd import rowcheck, synth
from topology_aware_learning_amd.arena import ModelPool, StateLayout


def test_dump_outputs_whole_segments(tmp_path):
    """Small segments are written whole: f32 as float32, bf16 widened exactly, int64 as float64."""
    lay = [("w", (37,), "float32"), ("h", (11,), "bfloat16"), ("count", (3,), "int64")]
    pool = ModelPool(StateLayout.from_layout(lay), 5, "cpu")
    rowcheck.fill_owned(pool, lay, range(5), 40)
    got = bench.dump_outputs(tmp_path / "d", pool, 4)
    assert got == {"f32.npy": [[4, 37], 37], "b16.npy": [[4, 11], 11], "i64.npy": [[4, 3], 3]}
    f32, b16, i64 = (np.load(tmp_path / "d" / f"{k}.npy") for k in ("f32", "b16", "i64"))
    assert f32.dtype == np.float32 and b16.dtype == np.float32 and i64.dtype == np.float64
    assert np.array_equal(f32.view(np.uint32), pool.f32[:4, :37].numpy().view(np.uint32))
    assert np.array_equal(b16, pool.b16[:4, :11].float().numpy())
    assert np.array_equal(i64.astype(np.int64), pool.i64[:4, :3].numpy())


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """A segment over the budget is cut to the same sorted, seeded draw of distinct columns on
    every call, shared among the float segments and the writing ranks."""
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 4 * 3 * 64)  # 64 fp32 columns of 3 rows
    lay = [("w", (1000,), "float32"), ("count", (2,), "int64")]
    pool = ModelPool(StateLayout.from_layout(lay), 3, "cpu")
    rowcheck.fill_owned(pool, lay, range(3), 7)
    a = bench.dump_outputs(tmp_path / "a", pool, 3)
    b = bench.dump_outputs(tmp_path / "b", pool, 3)
    assert a == b == {"f32.npy": [[3, 64], 1000], "i64.npy": [[3, 2], 2]}
    fa, fb = np.load(tmp_path / "a" / "f32.npy"), np.load(tmp_path / "b" / "f32.npy")
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    cols = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(1000, size=64, replace=False))
    assert len(set(cols.tolist())) == 64
    assert np.array_equal(fa.view(np.uint32), pool.f32[:3, :1000].numpy()[:, cols].view(np.uint32))
    half = bench.dump_outputs(tmp_path / "c", pool, 3, suffix="_rank1", writers=2)
    assert half == {"f32_rank1.npy": [[3, 32], 1000], "i64_rank1.npy": [[3, 2], 2]}


def test_host_path_needs_full(monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--host-path"])
    with pytest.raises(SystemExit):
        bench.parse()
    assert "--full" in capsys.readouterr().err
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs == ""


STEPS, WARMUP, DEVICES, DEGREE, MAX_PARAMS = 3, 2, 16, 4, 1_000_000


@pytest.fixture(scope="module")
def expected_rounds():
    """(f32, i64) of 16 devices with ResNet-50's first MAX_PARAMS float parameters and all its
    int64 counters after WARMUP + STEPS oracle rounds."""
    lay = synth.truncate_layout(synth.get_layout("resnet50"), MAX_PARAMS)
    layout = StateLayout.from_layout(lay)
    orders, weights = bench.round_spec(DEVICES, DEGREE)
    rp, col, w = bench._round_csr(orders, weights)
    pool = ModelPool(layout, DEVICES, "cpu")
    rowcheck.fill_owned(pool, lay, range(DEVICES), bench.SEED_BASE)
    f32 = pool.f32[:, :layout.n_f32].contiguous().numpy()
    i64 = pool.i64[:, :layout.n_i64].contiguous().numpy()
    rows = np.arange(DEVICES, dtype=np.int32)
    for _ in range(WARMUP + STEPS):
        f32 = oracle.round_f32(f32, rp, col, w, rows)
        i64 = oracle.round_i64(i64, rp, col, w, rows)
    return f32, i64


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
def test_bench_dumps_the_last_timed_step(cuda, tmp_path, expected_rounds, full):
    """One GPU, 16 cut-down ResNet-50 models: the plain run's line carries the headline fields and
    nothing it did not measure; --full adds the checks and side measurements; both dump the
    oracle's models after warmup + steps rounds, bit for bit."""
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--model", "resnet50", "--max-params", str(MAX_PARAMS), "--devices-per-gpu", str(DEVICES), "--degree", str(DEGREE),
           "--placement-trials", "2", "--dump-outputs", str(tmp_path / "out")]
    if full:
        cmd += ["--full", "--cpu-seconds", "0.5"]
    out = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, out.stdout[-2000:]
    d = json.loads(line[0])
    assert d["metric"] == "device-resident aggregated params/s at K=8 neighbors" and d["unit"] == "params/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == STEPS and d["warmup"] == WARMUP
    assert d["ms_per_step"] > 0
    params = d["config"]["devices"] * d["config"]["params_per_model"]
    assert d["value"] == pytest.approx(params / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["full"] is full
    if full:
        assert d["parity"] is True and d["parity_k3_vs_k1"]["rows_checked"] == DEVICES
        assert d["parity_k3_vs_k1"]["rows_differing"] == 0
        assert d["cpu_baseline"]["value"] > 0 and d["k1_per_call"]["ms"] > 0
    else:
        assert d["parity"] is None and d["parity_k3_vs_k1"] is None and d["parity_vs_reference"] is None
        assert d["cpu_baseline"] is None and "k1_per_call" not in d
    f32, i64 = expected_rounds
    n = f32.shape[1]  # 16 rows of 1 M columns: over the budget, so the dump is the seeded sample
    k = bench.DUMP_SAMPLE_BYTES // (4 * DEVICES)
    assert k < n
    cols = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(n, size=k, replace=False))
    want = {"f32.npy": [[DEVICES, k], n], "i64.npy": [[DEVICES, 53], 53]}
    assert d["dumped_outputs"] == want
    got_i = np.load(tmp_path / "out" / "i64.npy")
    assert got_i.dtype == np.float64 and np.array_equal(got_i.astype(np.int64), i64)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(want)
    got = np.load(tmp_path / "out" / "f32.npy")
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), f32[:, cols].view(np.uint32))
