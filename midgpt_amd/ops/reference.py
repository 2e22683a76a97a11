"""Pure-PyTorch reference implementations of the hot ops.

These define the numerics contract (fp32 internal math) that the HIP
kernels in ``csrc/`` are tested against, and serve as the CPU execution
path. Semantics follow the reference implementation:

- RMSNorm: ``x * rsqrt(mean(x^2) + eps)``, optional weight
  (reference src/layers.py:60-75; block norms weightless).
- QK-LayerNorm: LayerNorm over head dim, weight, no bias, eps 1e-6
  (reference src/model.py:52-53).
- RoPE: GPT-J interleaved pairing — ``rotate_every_two`` =
  ``[a b c d] -> [-b a -d c]`` (reference src/layers.py:85-99).
- Attention: causal, fp32 softmax with 1/sqrt(C) scale folded in
  (reference src/model.py:71-77).
- Cross-entropy: fp32 logits, mean over tokens (reference src/train.py:76-77).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F


def rmsnorm(x: torch.Tensor, weight=None, eps: float = 1e-6) -> torch.Tensor:
    """Row-wise RMS normalization over the last dim. fp32 internal math."""
    xf = x.float()
    out = xf * torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + eps)
    if weight is not None:
        out = out * weight.float()
    return out.to(x.dtype)


def qk_layernorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """LayerNorm over the last (head) dim with weight, no bias."""
    xf = x.float()
    mu = xf.mean(dim=-1, keepdim=True)
    var = xf.var(dim=-1, unbiased=False, keepdim=True)
    out = (xf - mu) * torch.rsqrt(var + eps) * weight.float()
    return out.to(x.dtype)


def rope_tables(head_dim: int, seq_len: int, base: float = 10000.0,
                device=None, dtype=torch.float32):
    """sin/cos tables of shape (T, C/2). inv_freq = base^(-2i/C)
    (reference src/layers.py:79-82, host-precomputed)."""
    inv_freq = 1.0 / (base ** (torch.arange(0, head_dim, 2, device=device,
                                            dtype=torch.float64) / head_dim))
    t = torch.arange(seq_len, device=device, dtype=torch.float64)
    freqs = torch.outer(t, inv_freq)  # (T, C/2)
    return freqs.sin().to(dtype), freqs.cos().to(dtype)


def rotate_every_two(x: torch.Tensor) -> torch.Tensor:
    """[a b c d] -> [-b a -d c] (GPT-J interleaved; reference src/layers.py:85-89)."""
    x1 = x[..., ::2]
    x2 = x[..., 1::2]
    out = torch.stack((-x2, x1), dim=-1)
    return out.flatten(-2)


def apply_rope(x: torch.Tensor, sin: torch.Tensor, cos: torch.Tensor) -> torch.Tensor:
    """x: (..., T, C); sin/cos: (T, C/2). Duplicates sin/cos to C interleaved
    and returns x*cos + rotate_every_two(x)*sin (reference src/layers.py:92-99)."""
    sin2 = torch.repeat_interleave(sin, 2, dim=-1).to(torch.float32)
    cos2 = torch.repeat_interleave(cos, 2, dim=-1).to(torch.float32)
    xf = x.float()
    out = xf * cos2 + rotate_every_two(xf) * sin2
    return out.to(x.dtype)


_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def _philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 on numpy uint64 arrays holding 32-bit values (a 32x32
    product fits in 64 bits, so mulhi is ``>> 32``). Mirrors csrc/philox.h."""
    lo32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    m0, m1 = np.uint64(_PHILOX_M0), np.uint64(_PHILOX_M1)
    for _ in range(10):
        p0 = m0 * c0
        p1 = m1 * c2
        n0 = (p1 >> s32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> s32) ^ c3 ^ np.uint64(k1)
        c1 = p1 & lo32
        c3 = p0 & lo32
        c0, c2 = n0, n2
        k0 = (k0 + _PHILOX_W0) & 0xFFFFFFFF
        k1 = (k1 + _PHILOX_W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def attn_dropout_threshold(p: float) -> int:
    """(uint32)(p * 2^32): an element is kept iff its word >= this."""
    return int(p * 4294967296.0)


def attn_dropout_keep(seed: int, B: int, H: int, T: int, p: float) -> torch.Tensor:
    """Bit-exact host mirror of the attention kernels' dropout keep-mask
    (csrc/philox.h): bool (B, H, T, T), True = kept. Key = 64-bit seed,
    counter = (k, q >> 2, b*H + h, 0), element (q, k) takes word q & 3."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    q4 = np.arange((T + 3) // 4, dtype=np.uint64)[None, :, None]
    kk = np.arange(T, dtype=np.uint64)[None, None, :]
    shape = (B * H, (T + 3) // 4, T)
    c0 = np.broadcast_to(kk, shape)
    c1 = np.broadcast_to(q4, shape)
    c2 = np.broadcast_to(bh, shape)
    c3 = np.zeros(shape, dtype=np.uint64)
    words = np.stack(_philox4x32_10(c0, c1, c2, c3, k0, k1), axis=2)  # (BH,T/4,4,T)
    keep = words.reshape(B * H, -1, T)[:, :T] >= np.uint64(attn_dropout_threshold(p))
    return torch.from_numpy(np.ascontiguousarray(keep)).view(B, H, T, T)


SAMPLE_DOMAIN = 0x53414D50  # "SAMP": counter word c3 of the sampling stream


def sample_words(B: int, V: int, seed: int, step: int, row0: int = 0) -> np.ndarray:
    """Bit-exact host mirror of csrc/philox.h:sample_words: uint32 (B, V),
    the word of vocabulary entry v of logits row b at token ``step``.
    Key = 64-bit seed, counter = (v >> 2, row0 + b, step, SAMPLE_DOMAIN),
    entry v takes word v & 3."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    step = int(step)
    if not 0 <= step < 1 << 32:
        raise ValueError(f"sample_words: step must be in [0, 2^32), got {step}")
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    n4 = (V + 3) // 4
    shape = (B, n4)
    c0 = np.broadcast_to(np.arange(n4, dtype=np.uint64)[None, :], shape)
    c1 = np.broadcast_to(np.arange(row0, row0 + B, dtype=np.uint64)[:, None], shape)
    c2 = np.full(shape, step, dtype=np.uint64)
    c3 = np.full(shape, SAMPLE_DOMAIN, dtype=np.uint64)
    words = np.stack(_philox4x32_10(c0, c1, c2, c3, k0, k1), axis=2)  # (B,n4,4)
    return np.ascontiguousarray(words.reshape(B, n4 * 4)[:, :V]).astype(np.uint32)


def sample_scores(logits: torch.Tensor, inv_t: float, seed: int, step: int) -> np.ndarray:
    """The sampling definition's scores in float64, (B, V):
    ``logit * inv_t - log(-log(t))`` with ``t = (2 * (word >> 9) + 1) * 2^-24``
    (23 bits, strictly inside (0, 1)). The token of row b is the lowest index
    among its candidates (``sample_candidates``) of maximal score."""
    B, V = logits.shape
    w = sample_words(B, V, seed, step)
    t = (2.0 * (w >> 9).astype(np.float64) + 1.0) * 2.0 ** -24
    noise = -np.log(-np.log(t))
    lf = logits.detach().double().cpu().numpy()
    return lf * float(inv_t) + noise


def sample_candidates(logits: torch.Tensor, top_k) -> np.ndarray:
    """bool (B, V): every entry, or with 1 <= top_k < V those whose logit is
    >= the row's k-th largest (entries tied with the k-th are all kept)."""
    lf = logits.detach().double().cpu().numpy()
    B, V = lf.shape
    if top_k is None or top_k <= 0 or top_k >= V:
        return np.ones((B, V), dtype=bool)
    kth = np.sort(lf, axis=1)[:, V - int(top_k)][:, None]
    return lf >= kth


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                     dropout_p: float = 0.0, training: bool = False,
                     keep: torch.Tensor | None = None) -> torch.Tensor:
    """q,k,v: (B, H, T, C). Materialized reference (O(T^2) memory):
    scores = QK^T masked, softmax((scores)/sqrt(C)) in fp32, then @V.
    With ``keep`` (bool, broadcastable to (B,H,T,T), e.g. from
    ``attn_dropout_keep``) that mask replaces ``F.dropout``: kept
    probabilities are scaled by 1/(1-dropout_p), the rest zeroed."""
    B, H, T, C = q.shape
    s = torch.matmul(q.float(), k.float().transpose(-1, -2))
    mask = torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
    s = s.masked_fill(~mask, float("-inf"))
    a = torch.softmax(s / math.sqrt(C), dim=-1)
    if keep is not None:
        a = a * keep.to(device=a.device, dtype=a.dtype) / (1.0 - dropout_p)
    elif dropout_p > 0.0 and training:
        a = F.dropout(a, p=dropout_p, training=True)
    return torch.matmul(a.to(v.dtype), v)


def cross_entropy(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """logits (N, V) any float dtype, targets (N,) int64. fp32 math, mean."""
    return F.cross_entropy(logits.float(), targets.reshape(-1))
