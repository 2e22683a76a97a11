"""Reference math for the KV-cache decode tests (test_decode_ref.py,
test_gpu_decode.py). Plain torch, any device."""
from __future__ import annotations

import math

import torch

from kernel_edge_util import rbf


def decode_math(q, k_cache, v_cache, kv_len: int, dt, rnd: bool):
    """End-aligned causal attention of q (B,H,Tq,C) over cache[:, :, :kv_len]
    in dtype ``dt``: row i sees keys [0, kv_len - Tq + i]. Scale 1/sqrt(C).
    rnd=True rounds where the kernel's contract rounds: the output to bf16,
    nothing else (P stays in ``dt``). Rows >= kv_len of the caches are never
    touched. Returns o (B,Tq,H,C), the kernel's layout."""
    B, H, Tq, C = q.shape
    k = k_cache[:, :, :kv_len].to(dt)
    v = v_cache[:, :, :kv_len].to(dt)
    s = torch.matmul(q.to(dt), k.transpose(-1, -2)) * (1.0 / math.sqrt(C))
    qpos = torch.arange(kv_len - Tq, kv_len, device=q.device)[:, None]
    kpos = torch.arange(kv_len, device=q.device)[None, :]
    s = s.masked_fill(kpos > qpos, float("-inf"))
    o = torch.matmul(torch.softmax(s, dim=-1), v)
    if rnd:
        o = rbf(o)
    return o.transpose(1, 2).contiguous()
