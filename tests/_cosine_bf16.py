"""Helpers shared by the bf16 cosine tests (test_cosine_bf16_host.py, test_gpu_cosine_bf16.py):
bf16 rows as uint16 bit patterns, their torch form, and the expected value - the existing fp32
oracle (oracle.cosine_model, unchanged) on the rows widened exactly to fp32, which is the
definition of the bf16 cosine similarity (include/tal_agg.h "K2 on bf16 models")."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

import oracle

# (A, I, B): streamed column, direct column, row and 1-D kinds, with partial steps, partial runs
# and remainders (the families of test_gpu_cosine_staged.py at their smallest)
HOST_SHAPES = [(64, 3, 9), (3, 511, 9), (3, 37, 31), (1, 16400, 3), (2, 513, 9), (3, 50, 32), (3, 4609, 1),
               (40, 7, 1), (11, 13, 1), (3, 1030, 1), (30, 1, 1)]


def extent(segs) -> int:
    return max(o + a * i * b for o, a, i, b in segs)


def bf16_rows(rng, segs, n):
    """n models as bf16 bit patterns: standard normals rounded to bf16."""
    total = extent(segs)
    return [oracle.f32_to_bf16(rng.standard_normal(total).astype(np.float32)) for _ in range(n)]


def as_torch(bits, device="cpu") -> torch.Tensor:
    """uint16 bit patterns -> a bfloat16 tensor of the same shape."""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).to(device)


def torch_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def ref(a_bits, b_bits, segs, threads: int = 1) -> np.float32:
    """The oracle on the widened rows."""
    return np.float32(oracle.cosine_model(oracle.bf16_to_f32(a_bits).astype(np.float32),
                                          oracle.bf16_to_f32(b_bits).astype(np.float32), segs, threads=threads))


def refs(rows, segs, pairs, threads: int = 1):
    """ref of every ordered pair (rows[a], rows[b]), each ordered pair evaluated once."""
    memo = {}
    for p in pairs:
        if p not in memo:
            memo[p] = ref(rows[p[0]], rows[p[1]], segs, threads)
    return [memo[p] for p in pairs]


def bits(v):
    return [int(np.float32(x).view(np.uint32)) for x in v]


def same(got, want) -> bool:
    """Bitwise equal, a NaN matching any NaN (payloads are unspecified)."""
    g, w = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    if g.shape != w.shape:
        return False
    nan = np.isnan(w)
    return bool(np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan]))


class SmallNet(nn.Module):
    """A 3 x 3 conv (streamed column kind), a 1 x 1 conv (row kind) and a linear layer, with
    biases (1-D kind) and odd sizes."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 7, 3)
        self.pw = nn.Conv2d(7, 5, 1)
        self.fc = nn.Linear(45, 11)


def small_bf16(seed: int) -> nn.Module:
    torch.manual_seed(seed)
    return SmallNet().to(torch.bfloat16)


def module_row(model: nn.Module, layout) -> np.ndarray:
    """A bf16 module's b16 segment as bit patterns (state_dict order)."""
    sd = model.state_dict()
    return np.concatenate([torch_bits(t.reshape(-1)) for t in layout.flatten_cat(sd, "b16")])
