"""Experiment driver — mirror of the reference's src/decentralized_app.py.

Round structure, operand order, RNG draws, strategy dispatch, scheduler stepping and the
checkpoint/resume protocol follow the reference (decentralized_app.py:96-644).  MI355X
difference: when a GPU is visible every client's model is bound to one device-resident
ModelPool row (topology_aware_learning_amd.arena), so local training and the aggregation
kernels work on the same HBM bytes and no model crosses PCIe between rounds
(TAL_DEVICE_POOL=0 keeps the reference's CPU-resident models).  TAL_BATCHED_ROUND=1 (opt-in;
=seq: the same batch as a sequential round, clients in order, one K3q launch per segment)
runs each round's aggregations as one K3 launch over that pool, with snapshot semantics.
"""
from __future__ import annotations

import contextlib
import glob
import io
import json
import logging
import os
import pathlib
import shutil
import sys
import threading
from concurrent.futures import Future
from pathlib import Path

import numpy
import torch

from src.aggregation_scheduler import (BaseScheduler, CosineAnnealingWarmRestarts, ExponentialScheduler,
                                       OscilateScheduler)
from src.decentralized_client import (DecentralClient, centrality_module_avg, create_centrality_dict, draw_neighbors,  # noqa: F401
                                      create_clients, scale_agg, sim_centrality_module_avg, test_agg,
                                      unweighted_module_avg, update_random_agg_coeffs, weighted_module_avg)
from src.modules import create_model, load_data
from src.tasks import local_train, no_local_train
from src.types import DataChoices, Result
from src.utils import load_checkpoint, process_futures_and_ckpt, set_file_logger

APP_LOG_LEVEL = 21
logger = logging.getLogger("decentral_app")

# strategy string -> (aggregation app, centrality metric); reference :318-353
STRATEGIES = {
    "betCent_sim": (sim_centrality_module_avg, "betweenness"),
    "degCent_sim": (sim_centrality_module_avg, "degree"),
    "random": (centrality_module_avg, "random"),
    "betCent": (centrality_module_avg, "betweenness"),
    "degCent": (centrality_module_avg, "degree"),
    "weighted": (weighted_module_avg, None),
    "unweighted": (unweighted_module_avg, None),
    "unweighted_fl": (unweighted_module_avg, None),
    "test_agg": (test_agg, None),
    "scale_agg": (scale_agg, None),
}

_DATASETS = {
    "mnist": (DataChoices.MNIST, 10), "fmnist": (DataChoices.FMNIST, 10), "cifar10": (DataChoices.CIFAR10, 10),
    "cifar10_mobile": (DataChoices.CIFAR10_MOBILE, 10), "cifar10_vit": (DataChoices.CIFAR10_VIT, 10),
    "cifar10_resnet18": (DataChoices.CIFAR10_RESTNET18, 10), "cifar10_resnet50": (DataChoices.CIFAR10_RESTNET50, 10),
    "cifar10_augment": (DataChoices.CIFAR10_AUGMENT, 10), "cifar10_augment_vgg": (DataChoices.CIFAR10_AUGMENT_VGG, 10),
    "cifar10_vgg": (DataChoices.CIFAR10_VGG, 10), "cifar100_vgg": (DataChoices.CIFAR100_VGG, 100),
    "cifar10_dropout": (DataChoices.CIFAR10_DROPOUT, 10),
    "cifar10_augment_dropout": (DataChoices.CIFAR10_AUGMENT_DROPOUT, 10),
}


class _Resolved(Future):
    """A future created already resolved (the batched round's aggregation results): the
    concurrent.futures.Future interface (result(), done(), add_done_callback, ...) without a
    condition variable and lock per future - they never wait, so one shared condition serves."""

    _cond = threading.Condition()

    def __init__(self, result):  # noqa: D107 - Future.__init__ replaced on purpose
        self._condition = _Resolved._cond
        self._state = "FINISHED"
        self._result = result
        self._exception = None
        self._waiters = []
        self._done_callbacks = []


class DecentrallearnApp:
    """Decentralized learning experiment (reference :58-454)."""

    sequential_round = False  # TAL_BATCHED_ROUND=seq (set in __init__): the batch as a sequential round

    def __init__(self, data_dir: str = "../data", topology_path: str = "topology/topo_1.txt",
                 dataset: str = "mnist", rounds: int = 5, batch_size: int = 16, epochs: int = 2,
                 lr: float = 1e-3, download: bool = False, train: bool = True, label_alpha: float = 100,
                 sample_alpha: float = 100, participation: float = 1.0, seed: int | None = 0,
                 log_dir: str = "./logs", aggregation_strategy: str = "weighted", prox_coeff: float = 0.1,
                 train_test_val: tuple = None, backdoor: bool = False, backdoor_proportion: float = 0.1,
                 backdoor_node_idx: int = 0, random_bd: bool = False, many_to_one: bool = True,
                 offset_clients_data_placement: int = 0, centrality_metric_data_placement: str = "degree",
                 random_data_placement: bool = True, softmax: bool = False, tiny_mem_num_labels: int = 50,
                 momentum: float = 0, softmax_coeff: float = 10, optimizer: str = "sgd",
                 weight_decay: float = 0, beta_1: float = 0.9, beta_2: float = 0.98, scheduler: str = None,
                 gamma: float = 0.95, T_0: float = 66, T_mult: float = 1, eta_min: float = 1,
                 trigger: int = 100, num_test: int = 1000, num_example: int = 5000, modulo: int = 16381,
                 length: int = 20, max_ctx: int = 150, n_layer: int = 4, task_type: str = "multiply",
                 data_dis: str = "evens", checkpoint_every: int = 5) -> None:
        args = dict(locals())
        args.pop("self", None)
        args["topology_path"] = os.path.basename(args["topology_path"])
        for k in ("log_dir", "rounds", "checkpoint_every"):
            args.pop(k, None)
        # run dir = every other ctor argument joined with "_" (reference :151-162)
        arg_path = "_".join(map(str, args.values())).replace(".", "").replace("/", "")
        self.run_dir = Path(f"{log_dir}/{arg_path}/")
        os.makedirs(self.run_dir, exist_ok=True)
        with open(f"{self.run_dir}/args.txt", "w") as f:
            json.dump(args, f)

        if dataset not in _DATASETS and "tiny_mem" not in dataset:
            raise ValueError(f"unknown dataset {dataset}")
        self.dataset, self.num_labels = _DATASETS.get(dataset, (None, tiny_mem_num_labels))
        set_file_logger(filename=f"{self.run_dir}/experiment.log", name="decentral_app")

        self.rng = numpy.random.default_rng(seed)
        self.seed = seed
        self.train_test_val = train_test_val
        if seed is not None:
            torch.manual_seed(seed)
        self.max_ctx, self.n_layer = max_ctx, n_layer
        self.global_model = create_model(data=self.dataset, n_layer=n_layer, max_ctx=max_ctx)
        self.checkpoint_every = checkpoint_every
        self.train = train
        root = pathlib.Path(data_dir)
        self.train_data = load_data(self.dataset, root, train=True, download=True)
        self.test_data = load_data(self.dataset, root, train=False, download=True)

        self.topology = numpy.loadtxt(topology_path, dtype=float)
        num_clients = self.topology.shape[0]
        self.backdoor = backdoor
        if backdoor:
            raise NotImplementedError("backdoor experiments are outside the accelerated path")

        self.aggregation_strategy = aggregation_strategy
        self.softmax = softmax
        self.softmax_coeff = softmax_coeff
        self.aggregation_scheduler = BaseScheduler(self.softmax_coeff)
        if aggregation_strategy not in STRATEGIES:
            raise ValueError(f"unknown aggregation strategy {aggregation_strategy}")
        self.aggregation_function, self.centrality_metric = STRATEGIES[aggregation_strategy]
        if scheduler == "CA":
            self.aggregation_scheduler = CosineAnnealingWarmRestarts(T_0=T_0, T_mult=T_mult, eta_min=eta_min,
                                                                     last_round=-1, softmax_coeff=self.softmax_coeff)
        if scheduler == "exp":
            self.aggregation_scheduler = ExponentialScheduler(gamma=gamma, softmax_coeff=self.softmax_coeff)
        if scheduler == "osc":
            self.aggregation_scheduler = OscilateScheduler(T_0=T_0, softmax_coeff=self.softmax_coeff)

        self.epochs, self.batch_size, self.lr = epochs, batch_size, lr
        self.momentum, self.optimizer, self.weight_decay = momentum, optimizer, weight_decay
        self.beta_1, self.beta_2 = beta_1, beta_2
        self.prox_coeff = prox_coeff
        self.participation = participation
        if aggregation_strategy == "unweighted_fl":  # fully connected, no self loops (:386-389)
            self.topology = numpy.ones(self.topology.shape)
            numpy.fill_diagonal(self.topology, 0)
        self.rounds = rounds
        self.start_round = 0
        if sample_alpha <= 0 or label_alpha <= 0:
            raise ValueError("Argument `alpha` must be greater than 0.")
        self.label_alpha, self.sample_alpha = label_alpha, sample_alpha
        if backdoor_node_idx >= num_clients:
            raise ValueError("Backdoor node index must be less than the # of clients.")

        self.clients = create_clients(num_clients, self.dataset, self.train_data, self.num_labels, self.test_data,
                                      label_alpha, sample_alpha, self.rng, self.topology, prox_coeff, self.run_dir,
                                      train_test_val)
        self.pool = self._bind_device_pool()
        # opt-in (no CLI change): the round's aggregations as one K3 launch with snapshot
        # semantics instead of one app call per client (the reference's form, the default)
        # =seq: the same batch as a sequential round (RoundExecutor.run(sequential=True)): clients in
        # the order of the batch, each reading the models the earlier ones left - the reference's
        # round under one aggregation thread
        batched = os.environ.get("TAL_BATCHED_ROUND", "0")
        self.batched_round = batched in ("1", "seq") and self.pool is not None
        self.sequential_round = self.batched_round and batched == "seq"
        if self.sequential_round:
            why = self._seq_round_per_call()
            if why:
                print(f"TAL_BATCHED_ROUND=seq: {why}; the round runs as one app call per client")
                self.batched_round = self.sequential_round = False
        self._executor = None
        self._round_cache: dict = {}  # _round_key -> the round's rows, weights and printout
        self.round_cache_hits = 0
        self.centrality_dict = create_centrality_dict(self.topology, self.rng)
        logger.log(APP_LOG_LEVEL, f"Created {len(self.clients)} clients")
        self.client_results: list[Result] = []

        ckpts = glob.glob(f"{self.run_dir}/*.pth")
        if ckpts:
            path = max(ckpts, key=os.path.getctime)
            logger.log(APP_LOG_LEVEL, f"Loading lastest checkpoint from:  {path}")
            try:
                (self.start_round, self.clients, self.client_results,
                 self.aggregation_scheduler) = load_checkpoint(path, self.clients, self.aggregation_scheduler)
            except Exception as exc:  # corrupt checkpoint: the reference deletes the run dir (:449-452)
                shutil.rmtree(self.run_dir, ignore_errors=True)
                raise RuntimeError(f"corrupt checkpoint {path}: run directory removed") from exc
            self.start_round += 1
            print(f"loaded latest ckpt from: {path}")

    def _bind_device_pool(self):
        if os.environ.get("TAL_DEVICE_POOL", "1") == "0" or not torch.cuda.is_available():
            return None
        from topology_aware_learning_amd.aggregate import layout_of_module
        from topology_aware_learning_amd.multipool import MultiPool, devices_from_env
        from topology_aware_learning_amd.round import calibrated_pool

        layout = layout_of_module(self.clients[0].model)
        trials = int(os.environ.get("TAL_POOL_PLACEMENT_TRIALS", "8"))
        devs = devices_from_env()
        if devs is not None:
            # TAL_GPUS=N: the clients in contiguous blocks over N GPUs of this one process, each
            # GPU's pool with ghost rows for the other GPUs' clients its clients can draw
            # (the topology's non-zero entries); see topology_aware_learning_amd/multipool.py
            mp = MultiPool(layout, len(self.clients), devs, adjacency=self.topology,
                           make_pool=lambda rows, dev: calibrated_pool(layout, rows, dev, trials=trials))
            for c in self.clients:
                mp.bind(c.model, c.idx)
            return mp
        # the pool the models live in for the whole run, placed where in-place rounds are fast
        pool = calibrated_pool(layout, len(self.clients), torch.device("cuda", torch.cuda.current_device()),
                               trials=trials)
        for c in self.clients:
            c.model.to(pool.device)
            pool.bind(c.model, c.idx)
        return pool

    def _seq_round_per_call(self) -> str:
        """Why TAL_BATCHED_ROUND=seq takes the per-call app path ("" when it does not): a `*_sim`
        strategy's similarities must be taken at each client's turn, on the models the earlier
        clients left; a MultiPool's clients are spread over several pools."""
        from topology_aware_learning_amd.multipool import MultiPool

        from src.decentralized_client import weight_rule

        rule = weight_rule(self.aggregation_function)
        if rule is not None and rule.__name__ == "_sim_centrality_weights":
            return "a *_sim strategy takes its similarities at each client's turn"
        if isinstance(self.pool, MultiPool):
            return "the models are spread over several GPUs (TAL_GPUS)"
        return ""

    def close(self) -> None:
        pass

    def run(self):
        """Round loop with periodic checkpoints (reference :460-518)."""
        self.round_states = {self.start_round: {i: {"agg": ([{}], self.clients[i])} for i in range(len(self.clients))}}
        train_result_futures = []
        if self.start_round >= self.rounds:
            return 0
        for round_idx in range(self.start_round, self.rounds):
            train_result_futures.extend(self._federated_round(round_idx))
            if round_idx % self.checkpoint_every == 0 and round_idx != 0:
                process_futures_and_ckpt(self.client_results, train_result_futures, self.round_states, round_idx,
                                         self.run_dir)
            self.round_states.pop(round_idx - 1, None)
        process_futures_and_ckpt(self.client_results, train_result_futures, self.round_states, self.rounds,
                                 self.run_dir)
        return 0

    def _federated_round(self, round_idx: int):
        """Client selection, local training, aggregation (reference :520-644)."""
        print("round idx: ", round_idx)
        job = local_train if self.train else no_local_train
        size = int(max(1, len(self.clients) * self.participation))
        selected = self.rng.choice(list(range(len(self.clients))), size=size, replace=False).tolist()
        print(f"{selected=}")
        futures = []
        batch = [] if self.batched_round else None
        nxt = self.round_states[round_idx + 1] = {}
        cur = self.round_states[round_idx]
        sel = set(selected)
        # both loops' neighbor draws (one get_neighbors() per selected client in client order,
        # loop 1 then loop 2: nothing between them draws from NumPy's global RNG) in one RNG call
        # made before any app is submitted: the same stream (draw_neighbors), and no GIL
        # hand-off to the app threads in the middle of the round
        picked = [c for c in self.clients if c.idx in sel]
        both = draw_neighbors(picked + picked)
        draws, draws2 = iter(both[:len(picked)]), iter(both[len(picked):])
        for client in self.clients:
            train_input = cur[client.idx]["agg"]
            if client.idx not in sel:
                nxt[client.idx] = {"train": train_input}
                continue
            prox_neighbors = [cur[i]["agg"] for i in next(draws)]
            nxt[client.idx] = {"train": job(train_input, round_idx, self.epochs, self.batch_size, self.lr,
                                            self.momentum, self.prox_coeff, self.seed, self.backdoor, self.dataset,
                                            self.optimizer, self.weight_decay, self.beta_1, self.beta_2,
                                            *prox_neighbors)}
        if self.centrality_metric == "random":
            self.centrality_dict = update_random_agg_coeffs(seed=self.seed, round_idx=round_idx,
                                                            num_clients=len(self.clients),
                                                            centrality_dict=self.centrality_dict)
        kwargs = None
        for client in self.clients:
            agg_client = nxt[client.idx]["train"]
            if client.idx not in sel:
                nxt[client.idx]["agg"] = agg_client
                futures.append(agg_client)
                continue
            neighbor_idxs = next(draws2)  # second, independent draw (:616)
            if len(neighbor_idxs) == 0:
                nxt[client.idx]["agg"] = agg_client
                futures.append(agg_client)
                continue
            neighbor_idxs.append(client.idx)  # self is the last operand (:625)
            if kwargs is None:  # the same for every call of the round (the scheduler steps after it)
                kwargs = dict(centrality_metric=self.centrality_metric, centrality_dict=self.centrality_dict,
                              softmax=self.softmax, softmax_coeff=self.aggregation_scheduler.get_softmax_coeff())
            if batch is not None:  # collected; the whole round runs below as one K3 launch
                # (the operand futures are nxt[i]["train"] for i in the drawn tuple: looked up
                # only when the round's weights are computed, not on a cached round)
                batch.append((len(futures), client.idx, agg_client, tuple(neighbor_idxs), kwargs))
                futures.append(None)  # its future is made after the launch (below)
                continue
            agg_neighbors = [nxt[i]["train"] for i in neighbor_idxs]
            future = self.aggregation_function(agg_client, self.seed, *agg_neighbors, **kwargs)
            futures.append(future)
            nxt[client.idx]["agg"] = future
        if batch:
            # the launch first, then the round's futures (already resolved: the aggregation is
            # stream-ordered behind the launch), so their setup runs under the kernel
            for (pos, idx, *_), me in zip(batch, self._batched_aggregation(batch, nxt)):
                futures[pos] = nxt[idx]["agg"] = _Resolved(me)
        self.aggregation_scheduler.step(round_idx)
        return futures

    def _batched_aggregation(self, batch, nxt) -> list:
        """The round's aggregations as ONE K3 launch over the device pool (RoundExecutor):
        every aggregation reads the models as they were after training (snapshot semantics,
        SURVEY §8(a)).  The reference's per-call apps instead read neighbors that an earlier
        call of the same round may already have overwritten, in an order its 2-thread pool
        decides; per call each result is the same arithmetic (same operands in the same order,
        same fp32 weights).  batch: (future position, client, its training future, drawn
        operand ids with self last, kwargs) per aggregation; nxt: the round's
        {client: {"train": future}}.  Returns each entry's aggregated (results, client) tuple,
        in order.  The `*_sim` strategies' similarities for the whole round come from one
        similarity.cosine_round call before the launch (_round_similarities)."""
        from topology_aware_learning_amd import arena
        from topology_aware_learning_amd.arena import bound_row
        from topology_aware_learning_amd.multipool import MultiPool
        from topology_aware_learning_amd.round import RoundExecutor

        from src.decentralized_client import manual_seed, weight_rule

        if isinstance(self.pool, MultiPool):
            return self._batched_aggregation_multi(batch, nxt)

        # every operand is some client's training future (nxt[i]["train"]): each resolved once
        # (64 futures behind 640 operand references at config 3), each model's row checked once
        memo = self._resolve_round(nxt)
        rule = weight_rule(self.aggregation_function)  # None for test_agg: a no-op
        key = self._round_key(batch, rule)
        hit = self._round_cache.get(key) if key is not None else None
        if hit is not None and not (hit["gen"] == arena._GEN[0] and arena._HOOKS):
            # a binding hook fired since (e.g. training's module.to()): every client of the round
            # still bound to the row it had, or the round is computed afresh
            if all(bound_row(self.clients[i].model) == (self.pool, r) for i, r in hit["rows"]):
                hit["gen"] = arena._GEN[0]
            else:
                hit = None
        if hit is not None:
            # the same drawn neighbor sets and weight inputs as a round before, and every model
            # where it was: its operand rows and weights as they were, and its weight rules'
            # printout
            sys.stdout.write(hit["text"])
            self.round_cache_hits += 1
            if self.seed is not None:
                manual_seed(self.seed)
            if self.sequential_round:
                self._executor.run(hit["orders"], hit["weights"], hit["out_rows"], sequential=True)
            else:
                self._executor.run(hit["orders"], hit["weights"], hit["out_rows"], plan=hit["plan"])
            return [memo[id(e[2])] for e in batch]
        row_of: dict = {}  # id(model) -> pool row

        def pool_row(m) -> int:
            b = bound_row(m)
            if b is None or b[0] is not self.pool:
                raise RuntimeError("TAL_BATCHED_ROUND needs every model bound to the device pool")
            row_of[id(m)] = b[1]
            return b[1]

        round_sims = None
        if rule is not None and rule.__name__ == "_sim_centrality_weights":
            round_sims = self._round_similarities(batch, nxt, memo, pool_row)
        orders, weights, out_rows, done = [], [], [], []
        text = io.StringIO()
        with contextlib.redirect_stdout(text) if key is not None else contextlib.nullcontext():
            for pos, (_, _, agg_client, idxs, kwargs) in enumerate(batch):
                me = memo[id(agg_client)]
                done.append(me)
                if rule is None:
                    continue
                if round_sims is not None:
                    kwargs = dict(kwargs, sims=round_sims[pos])
                got = rule(me, [memo[id(nxt[i]["train"])] for i in idxs], **kwargs)
                orders.append([row_of[id(m)] if id(m) in row_of else pool_row(m) for m in got[0]])
                weights.append(list(map(float, got[1])))
                m = me[1].model
                out_rows.append(row_of[id(m)] if id(m) in row_of else pool_row(m))
        if key is not None:
            sys.stdout.write(text.getvalue())
        if self.seed is not None:  # the apps seed torch per call (reference :395); same end state
            manual_seed(self.seed)
        if orders:
            if self._executor is None:
                self._executor = RoundExecutor(self.pool)
            if self.sequential_round:  # the executor keeps the sequential plan of these lists itself
                plan = None
                self._executor.run(orders, weights, out_rows, sequential=True)
            else:
                plan = self._executor.plan(orders, weights, out_rows)
                self._executor.run(orders, weights, out_rows, plan=plan)
            if key is not None:
                if len(self._round_cache) > 16:
                    self._round_cache.clear()
                rows = {v[1].idx: row_of[id(v[1].model)] for v in memo.values() if id(v[1].model) in row_of}
                self._round_cache[key] = dict(orders=orders, weights=weights, out_rows=out_rows, plan=plan,
                                              text=text.getvalue(), gen=arena._GEN[0], rows=sorted(rows.items()))
        return done

    def _round_similarities(self, batch, nxt, memo, pool_row) -> list:
        """The `*_sim` strategies' cosine similarities for a whole batched round in ONE call
        (similarity.cosine_round: every model's norms once, every edge once, one copy to the
        host) on the pool as it is after training, before the round's K3 launch: per batch
        entry {neighbor idx: similarity with the entry's client}, self excluded - what
        _sim_centrality_weights otherwise gets from one K2 launch and one synchronisation per
        client, bit for bit."""
        from topology_aware_learning_amd.similarity import cosine_round

        pairs, spans = [], []
        for _, _, agg_client, idxs, _ in batch:
            me = memo[id(agg_client)][1]
            others = [memo[id(nxt[i]["train"])][1] for i in idxs]
            others = [c for c in others if c.idx != me.idx]
            r = pool_row(me.model)
            spans.append((len(pairs), [c.idx for c in others]))
            pairs.extend((r, pool_row(c.model)) for c in others)
        vals = cosine_round(self.pool, pairs, memo[id(batch[0][2])][1].model) if pairs else []
        return [dict(zip(ids, vals[p0: p0 + len(ids)])) for p0, ids in spans]

    def _round_key(self, batch, rule):
        """A round's operand rows and weights are a function of its drawn neighbor sets and the
        weight rule's inputs for every strategy whose weights do not read the models (all but the
        *_sim strategies' cosine similarities) and whose centrality does not change per round
        (all but "random", redrawn every round: reference decentralized_app.py:596-598).  With
        `%d` topology files every link probability is 1, so the sets repeat round after round
        (SURVEY §5): the key is (rule, softmax, coefficient, metric, (client, neighbors) per
        entry), None when the round must be computed."""
        if rule is None or rule.__name__ == "_sim_centrality_weights" or self.centrality_metric == "random":
            return None
        kw = batch[0][4]
        return (rule.__name__, kw.get("softmax"), float(kw.get("softmax_coeff") or 0.0), kw.get("centrality_metric"),
                tuple((e[1], e[3]) for e in batch))

    @staticmethod
    def _resolve_round(nxt) -> dict:
        """id(future) -> its result, for every client's training future of the round."""
        memo: dict = {}
        for v in nxt.values():
            x = v["train"]
            if id(x) not in memo:
                memo[id(x)] = x.result() if isinstance(x, Future) else x
        return memo

    def _batched_aggregation_multi(self, batch, nxt) -> list:
        """_batched_aggregation over a MultiPool (TAL_GPUS): the same weights and operand order;
        the whole halo moves first (every GPU's ghost rows from their owners: RCCL sends /
        receives between this process's per-device communicators), then each GPU's share of the
        round runs as one K3 launch on its pool (own and ghost rows in, own rows out in place),
        each on its device's stream behind that device's messages.  The `*_sim` strategies keep
        the per-client cosine here (cosine_pairs over the ghost rows, one K2 launch per client):
        the round form (similarity.cosine_round) reads rows of one pool."""
        from topology_aware_learning_amd.arena import bound_row
        from topology_aware_learning_amd.round import RoundExecutor

        from src.decentralized_client import manual_seed, weight_rule

        mp = self.pool
        memo = self._resolve_round(nxt)
        gid_of: dict = {}  # id(model) -> global client id

        def gid(m) -> int:
            k = gid_of.get(id(m))
            if k is None:
                b = bound_row(m)
                if b is None or mp.member(b[0]) is None:
                    raise RuntimeError("TAL_BATCHED_ROUND needs every model bound to the device pools")
                k = gid_of[id(m)] = mp.global_id(b[0], b[1])
            return k

        per_gpu = [([], [], []) for _ in range(mp.world)]  # (orders, weights, out rows) in local rows
        done = []
        rule = weight_rule(self.aggregation_function)  # None for test_agg: a no-op
        for _, _, agg_client, idxs, kwargs in batch:
            me = memo[id(agg_client)]
            done.append(me)
            if rule is None:
                continue
            got = rule(me, [memo[id(nxt[i]["train"])] for i in idxs], **kwargs)
            g, out_row = mp.home(gid(me[1].model))
            loc = mp.local[g]
            per_gpu[g][0].append([loc[gid(m)] for m in got[0]])
            per_gpu[g][1].append(list(map(float, got[1])))
            per_gpu[g][2].append(out_row)
        if self.seed is not None:  # the apps seed torch per call (reference :395); same end state
            manual_seed(self.seed)
        if any(o for o, _, _ in per_gpu):
            if self._executor is None:
                # double-buffered per GPU pool; the ghost rows are not carried into the spare (the
                # next halo, or a per-call read, refreshes every ghost row before it is read)
                self._executor = [RoundExecutor(p, carried_rows=len(mp.own[g])) for g, p in enumerate(mp.pools)]
            mp.exchange_halo()
            for g, (orders, weights, out_rows) in enumerate(per_gpu):
                if orders:
                    with torch.cuda.device(mp.devices[g]):
                        self._executor[g].run(orders, weights, out_rows)
        return done
