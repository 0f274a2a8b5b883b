"""The reference of the sequential round tests (tests/test_gpu_seq_*.py): rows in order, each one
oracle K1 call on the running pool - oracle.reference_alg.sequential_round_f32 extended to bf16,
int64 and the FMA mode.  Pools are storage bits as in tests/_clique.py (uint32 for fp32, uint16
for bf16, int64 for int64)."""
import networkx as nx
import numpy as np

import oracle


def sequential_oracle(pool_bits, orders, weights, out_rows, dtype, exact=True):
    """pool_bits [rows, n] after the round `out_rows[r] <- chain(weights[r], pool[orders[r]])` run
    row by row in the order given, every row reading what the rows before it wrote.
    dtype: "f32" (uint32 bits), "bf16" (uint16 bits) or "i64" (int64 values)."""
    pool = np.ascontiguousarray(pool_bits).copy()
    for r, order, w in zip(out_rows, orders, weights):
        if dtype == "f32":
            xs = [pool[j].view(np.float32) for j in order]
            pool[r] = oracle.agg_f32(xs, w, exact=exact).view(np.uint32)
        elif dtype == "bf16":
            pool[r] = oracle.agg_bf16([pool[j] for j in order], w, exact=exact)
        else:
            pool[r] = oracle.agg_i64([pool[j] for j in order], w)
    return pool


def csr(orders, weights):
    row_ptr = np.cumsum([0] + [len(o) for o in orders]).astype(np.int32)
    return row_ptr, np.concatenate(orders).astype(np.int32), np.concatenate(weights).astype(np.float64)


def graph(name):
    """The tests' graphs by name."""
    if name.startswith("ring"):
        return nx.cycle_graph(int(name[4:]))
    if name.startswith("star"):
        return nx.star_graph(int(name[4:]) - 1)  # node 0 is the hub
    if name == "ba33":
        return nx.barabasi_albert_graph(33, 2, seed=0)
    if name == "rr64":
        return nx.random_regular_graph(8, 64, seed=1)
    if name == "barbell12_4":
        return nx.barbell_graph(12, 4)
    if name.startswith("complete"):
        return nx.complete_graph(int(name[8:]))
    raise KeyError(name)
