"""TAL_BATCHED_ROUND=seq in the driver: decentralized_main.py runs each round's aggregations as one
RoundExecutor.run(sequential=True) - clients in the order of the batch, each reading the models
the earlier ones left - checked segment by segment against the row-by-row oracle; `*_sim`
strategies keep the per-call apps, and =1 keeps its snapshot round."""
import networkx as nx
import numpy as np
import pytest

from topology_aware_learning_amd import ops
from topology_aware_learning_amd.round import RoundExecutor

from _clique import bits, same
from _seq import sequential_oracle

pytestmark = pytest.mark.gpu


def _main(tmp_path, strategy, rounds=2):
    topo = tmp_path / "ring8.txt"
    np.savetxt(topo, nx.to_numpy_array(nx.cycle_graph(8)), fmt="%d")
    from src.experiments import decentralized_main

    return decentralized_main.main(["--dataset", "cifar10", "--aggregation_strategy", *strategy, "--rounds",
                                    str(rounds), "--epochs", "1", "--topology_file", str(topo), "--out_dir",
                                    str(tmp_path / "logs"), "--batch_size", "32"])


def _synthetic(monkeypatch, batched):
    monkeypatch.setenv("TAL_SYNTHETIC_DATA", "1")
    monkeypatch.setenv("TAL_SYNTHETIC_SAMPLES", "64")
    monkeypatch.setenv("TAL_BATCHED_ROUND", batched)


@pytest.mark.parametrize("kernel", [True, False], ids=["kernel", "k1 loop"])
@pytest.mark.parametrize("strategy", [("unweighted",), ("degCent", "--softmax")], ids=["unweighted", "degCent"])
def test_driver_sequential_round(cuda, tmp_path, monkeypatch, strategy, kernel):
    """Two rounds, each one run(sequential=True) over all eight clients; the pool after it is the
    oracle's sequential sweep of the pool before it, fp32 and int64 segments, whichever form the
    executor takes (the kernel switched on or off for every dtype and mode)."""
    _synthetic(monkeypatch, "seq")
    for key in list(ops.SEQ_DEFAULT):
        monkeypatch.setitem(ops.SEQ_DEFAULT, key, kernel)
    real_run = RoundExecutor.run
    runs = []

    def checked_run(self, orders, weights, out_rows=None, sequential=False, plan=None):
        lay = self.pool.layout
        f_in = bits(self.pool.f32[:, : lay.n_f32]).copy()
        i_in = self.pool.i64[:, : lay.n_i64].cpu().numpy().copy()
        assert sequential is True and plan is None
        real_run(self, orders, weights, out_rows, sequential, plan)
        ref = sequential_oracle(f_in, orders, weights, out_rows, "f32")
        iref = sequential_oracle(i_in, orders, weights, out_rows, "i64")
        assert same(bits(self.pool.f32[:, : lay.n_f32]), ref, nan_payloads_free=True)
        assert np.array_equal(self.pool.i64[:, : lay.n_i64].cpu().numpy(), iref)
        runs.append(list(out_rows))

    monkeypatch.setattr(RoundExecutor, "run", checked_run)
    seq_calls = []
    real_seq = ops.round_seq_f32
    monkeypatch.setattr(ops, "round_seq_f32", lambda *a, **k: (seq_calls.append(1), real_seq(*a, **k))[1])
    assert _main(tmp_path, strategy) == 0
    assert runs == [list(range(8))] * 2  # client order is the order of the batch
    assert len(seq_calls) == (2 if kernel else 0)


def test_sim_strategy_keeps_the_per_call_apps(cuda, tmp_path, monkeypatch, capsys):
    _synthetic(monkeypatch, "seq")
    called = []
    monkeypatch.setattr(RoundExecutor, "run", lambda self, *a, **k: called.append(1))
    import src.decentralized_client as dc
    from topology_aware_learning_amd.aggregate import aggregate_models as real

    apps = []
    monkeypatch.setattr(dc, "aggregate_models", lambda *a, **k: (apps.append(1), real(*a, **k))[1])
    assert _main(tmp_path, ("degCent_sim", "--softmax")) == 0
    assert not called and len(apps) == 16  # 8 clients x 2 rounds, one app call each
    out = capsys.readouterr().out
    assert out.count("TAL_BATCHED_ROUND=seq:") == 1 and "one app call per client" in out


def test_batched_round_1_is_still_the_snapshot_round(cuda, tmp_path, monkeypatch):
    _synthetic(monkeypatch, "1")
    real_run = RoundExecutor.run
    seen = []

    def spy(self, orders, weights, out_rows=None, sequential=False, plan=None):
        seen.append((sequential, plan is not None))
        return real_run(self, orders, weights, out_rows, sequential, plan)

    monkeypatch.setattr(RoundExecutor, "run", spy)
    assert _main(tmp_path, ("unweighted",)) == 0
    assert seen == [(False, True)] * 2
