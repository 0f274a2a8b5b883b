"""K2r on the host: the round table (tal_cosine_round_build: distinct rows, distinct unordered
pairs in groups of at most 8 that share one row, the map from each ordered pair), its
refusals, the host form (ops.host_cosine_round) bitwise the oracle for every ordered pair, and
_sim_centrality_weights taking a round's similarities instead of calling cosine_pairs.
Reference: cosine_similarity / sim_centrality_module_avg, src/decentralized_client.py:452-550,
661-681 of the reference.
"""
from __future__ import annotations

import ctypes

import networkx as nx
import numpy as np
import pytest
import torch
from torch.utils.data import Subset, TensorDataset

import oracle
from topology_aware_learning_amd import _lib, ops

from _models import TinyNet

P32 = ctypes.POINTER(ctypes.c_int32)
P64 = ctypes.POINTER(ctypes.c_int64)


def _parse(table):
    """(models, unique [n, 2] slots, groups [n, 3], map) of a CosineRound's host words."""
    t = table.host
    n_pairs, n_unique, n_models, n_groups = (int(x) for x in t[:4])
    o = 8
    models = t[o: o + n_models]
    o += n_models
    uniq = t[o: o + 2 * n_unique].reshape(-1, 2)
    o += 2 * n_unique
    groups = t[o: o + 3 * n_groups].reshape(-1, 3)
    o += 3 * n_groups
    mp = t[o: o + n_pairs]
    assert o + n_pairs == len(t) == table.info.words == t[6]
    return models, uniq, groups, mp


def _round_pairs():
    g = nx.random_regular_graph(3, 12, seed=2)
    pairs = []
    for u, v in g.edges():  # rows 4 .. 15, both directions
        pairs += [(u + 4, v + 4), (v + 4, u + 4)]
    pairs.append(pairs[5])          # a repeated pair
    pairs.append((7, 7))            # a self pair
    pairs += [(0, r) for r in range(4, 16)]  # a star: 12 partners of row 0
    return pairs


def test_table_invariants():
    pairs = _round_pairs()
    table = ops.build_cosine_round(pairs, 16)
    models, uniq, groups, mp = _parse(table)
    info = table.info
    want_models = sorted({r for p in pairs for r in p})
    assert want_models == [0] + list(range(4, 16))  # rows 1 .. 3 are not referenced
    assert models.tolist() == want_models
    want_unique = sorted({(min(a, b), max(a, b)) for a, b in pairs})
    got_unique = [(int(min(models[a], models[b])), int(max(models[a], models[b]))) for a, b in uniq]
    assert sorted(got_unique) == want_unique and len(set(got_unique)) == len(got_unique)
    assert (7, 7) in got_unique
    for j, (a, b) in enumerate(pairs):  # every ordered pair maps to the unique pair with its rows
        assert got_unique[mp[j]] == (min(a, b), max(a, b)), j
    covered = []
    for slot_a, first, count in groups:
        assert 1 <= count <= 8
        for u in range(first, first + count):
            assert uniq[u][0] == slot_a  # the group's pairs share the group's row, listed first
        covered += list(range(first, first + count))
    assert covered == list(range(len(want_unique)))  # every unique pair in exactly one group, in order
    assert len(want_unique) == 31 and len(groups) >= 4  # 8 pairs to a group at most
    # a star alone: its centre has 12 partners, more than one group holds
    star = ops.build_cosine_round([(0, r) for r in range(1, 13)] + [(5, 0)], 13)
    _, s_uniq, s_groups, s_map = _parse(star)
    assert s_groups.tolist() == [[0, 0, 8], [0, 8, 4]] and (s_uniq[:, 0] == 0).all()
    assert s_map[12] == s_map[4] and star.info.n_unique == 12
    assert (info.n_pairs, info.n_unique, info.n_models, info.n_groups) == (
        len(pairs), len(want_unique), len(want_models), len(groups))
    assert info.max_group == 8 and info.pool_rows == 16
    assert table.host[:7].tolist() == [info.n_pairs, info.n_unique, info.n_models, info.n_groups, info.max_group,
                                       info.pool_rows, info.words]


def test_refusals():
    L = _lib.load()
    ra = np.array([0, 1, 2], dtype=np.int32)
    rb = np.array([1, 2, 0], dtype=np.int32)
    words = int(L.tal_cosine_round_words(3))
    assert words > 0 and L.tal_cosine_round_words(0) == -1
    buf = np.zeros(words, dtype=np.int32)
    info = _lib.CosineRoundInfo()

    def build(a, b, n, rows, out, cap):
        return L.tal_cosine_round_build(a.ctypes.data_as(P32) if a is not None else None,
                                        b.ctypes.data_as(P32) if b is not None else None, n, rows,
                                        out.ctypes.data_as(P32) if out is not None else None, cap, ctypes.byref(info))

    assert build(ra, rb, 0, 3, buf, words) == _lib.TAL_ERR_INVALID and L.tal_last_error()
    assert b"n_pairs" in L.tal_last_error()
    assert build(None, rb, 3, 3, buf, words) == _lib.TAL_ERR_INVALID and b"null" in L.tal_last_error()
    assert build(ra, None, 3, 3, buf, words) == _lib.TAL_ERR_INVALID and b"null" in L.tal_last_error()
    bad = np.array([0, 3, 2], dtype=np.int32)  # a row equal to pool_rows
    assert build(bad, rb, 3, 3, buf, words) == _lib.TAL_ERR_INVALID and b"row" in L.tal_last_error()
    assert build(ra, bad, 3, 3, buf, words) == _lib.TAL_ERR_INVALID
    neg = np.array([0, -1, 2], dtype=np.int32)
    assert build(neg, rb, 3, 3, buf, words) == _lib.TAL_ERR_INVALID
    assert build(ra, rb, 3, 3, buf, 4) == _lib.TAL_ERR_CAPACITY and L.tal_last_error()
    need = int(info.words)
    assert need == 8 + 3 + 2 * 3 + 3 * 2 + 3  # header, models, unique pairs, groups {0: 2 pairs}, {1: 1}, map
    assert build(ra, rb, 3, 3, buf, need) == _lib.TAL_OK
    assert build(ra, rb, 3, 3, buf, need - 1) == _lib.TAL_ERR_CAPACITY and info.words == need

    # the scratch: norms per model, one batch of pairs, a result per unique pair
    plan = ops.build_cosine_plan([(0, 8, 64, 9), (4608, 16, 72, 1)])
    table = ops.build_cosine_round([(0, r) for r in range(1, 13)], 13)
    hp, ht = plan.host.ctypes.data_as(P64), table.host.ctypes.data_as(P32)
    n_out, n_seg = int(plan.host[1]), plan.n_seg
    fixed = 4 * (13 * n_out + 12)
    per = 4 * (n_out + n_seg)
    assert L.tal_cosine_round_scratch_bytes(hp, ht, ctypes.byref(table.info), fixed + 8 * per - 1) == -1
    assert L.tal_cosine_round_scratch_bytes(hp, ht, ctypes.byref(table.info), 0) == -1
    assert L.tal_cosine_round_scratch_bytes(None, ht, ctypes.byref(table.info), 1 << 30) == -1
    assert L.tal_cosine_round_scratch_bytes(hp, ht, ctypes.byref(table.info), fixed + 8 * per) == fixed + 8 * per
    assert (table.info.batch_pairs, table.info.n_batches) == (8, 2)
    assert L.tal_cosine_round_scratch_bytes(hp, ht, ctypes.byref(table.info), 1 << 30) == fixed + 12 * per
    assert (table.info.batch_pairs, table.info.n_batches) == (12, 1)
    # the launcher refuses before touching a GPU: an info that does not describe the table, no scratch
    fake = ctypes.c_void_p(0x1000)
    other = _lib.CosineRoundInfo()
    assert L.tal_cosine_round(fake, 1 << 20, fake, hp, plan.n_chunks, fake, ht, ctypes.byref(other), fake, 1 << 30,
                              fake, None) == _lib.TAL_ERR_INVALID
    assert L.tal_cosine_round(fake, 1 << 20, fake, hp, plan.n_chunks, fake, ht, ctypes.byref(table.info), fake, 16,
                              fake, None) == _lib.TAL_ERR_INVALID and b"scratch" in L.tal_last_error()
    assert L.tal_cosine_round(fake, 100, fake, hp, plan.n_chunks, fake, ht, ctypes.byref(table.info), fake, 1 << 30,
                              fake, None) == _lib.TAL_ERR_INVALID and b"pitch" in L.tal_last_error()


def _segments():
    segs, off = [], 5
    for a, i, b in [(8, 64, 9), (16, 72, 1), (30, 1, 1), (3, 50, 32), (4, 2, 7)]:
        segs.append((off, a, i, b))
        off += a * i * b + 3
    return segs, off


def test_host_cosine_round_vs_oracle():
    """A CPU pool whose row pitch exceeds the row, rows used out of order: every ordered pair is
    bitwise the oracle; the oracle itself is symmetric on these inputs (the deduplication rests
    on it)."""
    segs, n = _segments()
    rng = np.random.default_rng(17)
    pool = torch.zeros(7, n + 37)
    pool[:, :n] = torch.from_numpy(rng.standard_normal((7, n)).astype(np.float32))
    view = pool[:, :n]
    rows = view.numpy()
    pairs = [(5, 1), (1, 5), (5, 0), (2, 6), (6, 2), (3, 3), (0, 2), (5, 1), (6, 5), (4, 0)]
    plan = ops.build_cosine_plan(segs)
    got = ops.host_cosine_round(view, pairs, plan).numpy()
    table = ops.build_cosine_round(pairs, 7)
    assert table.info.n_unique == 7
    again = ops.host_cosine_round(view, table, plan).numpy()
    for j, (a, b) in enumerate(pairs):
        ref = np.float32(oracle.cosine_model(rows[a], rows[b], segs))
        sym = np.float32(oracle.cosine_model(rows[b], rows[a], segs))
        assert ref.view(np.uint32) == sym.view(np.uint32), (a, b)
        assert got[j].view(np.uint32) == ref.view(np.uint32), (j, a, b, got[j], ref)
        assert again[j].view(np.uint32) == ref.view(np.uint32)
    # argument checks: a row too short for the plan, a table for more rows than the pool has
    with pytest.raises(ValueError, match="shorter"):
        ops.host_cosine_round(pool[:, : n - 4], pairs, plan)
    with pytest.raises(ValueError, match="rows"):
        ops.host_cosine_round(view[:6], table, plan)
    with pytest.raises(ValueError, match="row outside"):
        ops.build_cosine_round([(0, 7)], 7)


def _client(idx, model):
    from src.decentralized_client import DecentralClient

    data = TensorDataset(torch.zeros(4, 1), torch.zeros(4, dtype=torch.long))
    return DecentralClient(idx=idx, prox_coeff=0.0, model=model, train_data=Subset(data, [0, 1, 2, 3]), test_data=None,
                           valid_data=None, global_test_data=data, global_backdoor_test_data=None, neighbors=[],
                           neighbor_probs=[])


def test_sim_weights_take_round_similarities(monkeypatch, capsys):
    """_sim_centrality_weights(sims=...) returns the weights and prints the text of the call that
    gets the same values from cosine_pairs, and does not call cosine_pairs."""
    import src.decentralized_client as dc

    torch.manual_seed(4)
    order = [3, 0, 7, 5]  # self (5) last, as the driver passes it
    futures = [(["r"], _client(i, TinyNet())) for i in order]
    cent = {"degree": {0: 0.2, 3: 0.5, 5: 0.4, 7: 0.1}}
    sims = {3: 0.25, 0: -0.5, 7: 0.125}
    calls = []

    def fake_pairs(model, others):
        calls.append(len(others))
        return [sims[i] for i in order[:-1]]

    monkeypatch.setattr(dc, "cosine_pairs", fake_pairs)
    for softmax in (True, False):
        kw = dict(centrality_metric="degree", centrality_dict=cent, softmax=softmax, softmax_coeff=10.0)
        calls.clear()
        models_a, w_a = dc._sim_centrality_weights(futures[-1], futures, **kw)
        text_a = capsys.readouterr().out
        assert calls == [3]
        models_b, w_b = dc._sim_centrality_weights(futures[-1], futures, sims=dict(sims), **kw)
        text_b = capsys.readouterr().out
        assert calls == [3]  # not called again
        assert text_a == text_b and text_a
        assert [float(x) for x in w_a] == [float(x) for x in w_b]
        assert all(x is y for x, y in zip(models_a, models_b)) and len(models_a) == 4
