"""Op dispatch and autograd plumbing: hand-written HIP/CDNA4 kernels on GPU,
the same interface in fp32 PyTorch (``ops/ref_backend.py``) on CPU.

The HIP extension is built IN-TREE as ``midgpt_amd/ops/_C*.so`` (see
``setup.py`` / ``__graft_entry__.build``). On a GPU box the
extension is REQUIRED: ops raise if it is missing so that a silent eager
fallback can never masquerade as the native path. Set ``MIDGPT_FORCE_REF=1``
to explicitly run the reference path on GPU (debugging only).
"""
from __future__ import annotations

import math
import os

import torch

from midgpt_amd.ops import ref_backend

_C = None
_C_ERR: str | None = None

# The entry points that the extension and ref_backend both implement, with
# the same positional arguments and the same results (count, shapes, dtypes).
# Every op below that has a torch fallback is one call through _backend().
BACKEND_API = (
    "rmsnorm_fwd", "rmsnorm_bwd", "qkv_prep_fwd", "qkv_prep_bwd",
    "attn_fwd", "attn_bwd", "attn_fwd_dropout", "attn_bwd_dropout",
    "gelu_fwd", "gelu_bwd", "embedding_bwd", "ce_fwd", "ce_bwd",
    "adamw_step", "kv_append", "attn_decode",
)
# The ragged decode pair (per-sequence positions / lengths), implemented by
# both backends under the same rule as BACKEND_API.
RAGGED_API = ("kv_append_ragged", "attn_decode_ragged")
# Seeded token sampling, under the same rule.
SAMPLING_API = ("sample_tokens",)
# Slot-mapped decode and per-row sampling (continuous batching), under the
# same rule.
SLOT_API = ("kv_append_slots", "attn_decode_slots", "sample_tokens_rows")
# Paged decode (block-table caches), under the same rule.
PAGED_API = ("kv_append_paged", "attn_decode_paged", "kv_store_paged")
# Batched transpose of matrices inside a flat buffer, under the same rule.
TRANSPOSE_API = ("transpose_batched",)


def _try_load_ext():
    global _C, _C_ERR
    if _C is not None:
        return _C
    try:
        import importlib
        _C = importlib.import_module("midgpt_amd.ops._C")
    except Exception as e:  # pragma: no cover
        _C_ERR = repr(e)
        _C = None
    return _C


_try_load_ext()


def have_ext() -> bool:
    return _C is not None


def _use_hip(*tensors) -> bool:
    """True iff tensors live on a GPU. Raises loudly if the extension is
    missing on GPU (unless MIDGPT_FORCE_REF=1)."""
    on_gpu = any(t.is_cuda for t in tensors if isinstance(t, torch.Tensor))
    if not on_gpu:
        return False
    if os.environ.get("MIDGPT_FORCE_REF") == "1":
        return False
    if _C is None:
        raise RuntimeError(
            "midgpt_amd HIP extension (midgpt_amd/ops/_C) is not built but a GPU "
            f"tensor reached a hot op. Build it with __graft_entry__.build(). "
            f"Import error: {_C_ERR}")
    return True


def _backend(*tensors):
    """The implementation of BACKEND_API for these tensors: the extension
    where ``_use_hip`` says so, ref_backend otherwise."""
    return _C if _use_hip(*tensors) else ref_backend


# ----------------------------------------------------------------------------
# RMSNorm (reference src/layers.py:60-75; plan K5)
# ----------------------------------------------------------------------------
class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        shp = x.shape
        x2d = x.reshape(-1, shp[-1])
        y, invrms = _backend(x).rmsnorm_fwd(x2d.contiguous(), weight, eps)
        ctx.save_for_backward(x2d, invrms, *( [weight] if weight is not None else [] ))
        ctx.eps = eps
        ctx.has_w = weight is not None
        return y.reshape(shp)

    @staticmethod
    def backward(ctx, dy):
        saved = ctx.saved_tensors
        x2d, invrms = saved[0], saved[1]
        weight = saved[2] if ctx.has_w else None
        dy2d = dy.reshape(x2d.shape)
        dx, dw = _backend(x2d).rmsnorm_bwd(dy2d.contiguous(), x2d.contiguous(),
                                           weight, invrms, ctx.eps)
        return dx.reshape(dy.shape), dw, None


def rmsnorm(x, weight=None, eps: float = 1e-6):
    return _RMSNorm.apply(x, weight, eps)


def glue_unfused() -> bool:
    """MIDGPT_GLUE_UNFUSED=1 (read at call time) restores the composition of
    separate add, rmsnorm, qkv_prep, flash_attention and transpose kernels:
    the A/B handle for ``add_rmsnorm`` / ``qkv_attention`` and the path the
    tests compare them against, bit for bit."""
    return os.environ.get("MIDGPT_GLUE_UNFUSED") == "1"


# ----------------------------------------------------------------------------
# Fused residual add + weightless RMSNorm: s = x + r, y = rmsnorm(s).
# One kernel each way instead of add + norm (forward) and norm-backward +
# gradient-accumulation add (backward); results are bit-identical to those.
# ----------------------------------------------------------------------------
class _AddRMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, eps):
        shp = x.shape
        D = shp[-1]
        s, y, invrms = _C.add_rmsnorm_fwd(x.reshape(-1, D).contiguous(),
                                          r.reshape(-1, D).contiguous(), eps)
        ctx.save_for_backward(s, invrms)
        ctx.set_materialize_grads(False)
        return s.view(shp), y.view(shp)

    @staticmethod
    def backward(ctx, ds, dy):
        s, invrms = ctx.saved_tensors
        if dy is None:  # only the sum was used
            return ds, ds, None
        shp = dy.shape
        if ds is not None:
            ds = ds.reshape(s.shape).contiguous()
        dx = _C.add_rmsnorm_bwd(ds, dy.reshape(s.shape).contiguous(), s,
                                invrms).view(shp)
        # d(x + r) flows to both addends unchanged: one tensor serves both
        return dx, dx, None


def add_rmsnorm(x, r, eps: float = 1e-6):
    """(s, y) with s = x + r and y = rmsnorm(s) (weightless). On GPU in bf16
    with D % 8 == 0 this is one fused kernel per direction; otherwise (CPU,
    other dtypes or widths) the composition of the existing ops."""
    if (_use_hip(x, r) and x.dtype == torch.bfloat16 and r.dtype == torch.bfloat16
            and x.shape == r.shape and x.shape[-1] % 8 == 0
            and not glue_unfused()):
        return _AddRMSNorm.apply(x, r, eps)
    s = x + r
    return s, rmsnorm(s, None, eps)


# ----------------------------------------------------------------------------
# Fused QK-LayerNorm + RoPE over the packed QKV projection
# (reference src/model.py:59-69; plan K3+K4). Input qkv: (B, T, 3, H, C)
# produced by the c_attn GEMM; outputs q,k,v: (B, H, T, C), with LayerNorm
# (weight, no bias, eps 1e-6) and GPT-J interleaved RoPE applied to q,k.
# ----------------------------------------------------------------------------
class _QKVPrep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, qw, kw, sin, cos, eps):
        assert qkv.shape[2] == 3
        q, k, v, qstats, kstats = _backend(qkv).qkv_prep_fwd(
            qkv.contiguous(), qw, kw, sin, cos, eps)
        ctx.save_for_backward(qkv, qw, kw, sin, cos, qstats, kstats)
        ctx.eps = eps
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        qkv, qw, kw, sin, cos, qstats, kstats = ctx.saved_tensors
        dqkv, dqw, dkw = _backend(qkv).qkv_prep_bwd(
            dq.contiguous(), dk.contiguous(), dv.contiguous(), qkv.contiguous(),
            qw, kw, sin, cos, qstats, kstats, ctx.eps)
        return dqkv, dqw, dkw, None, None, None


def qkv_prep(qkv, q_ln_weight, k_ln_weight, sin, cos, eps: float = 1e-6):
    return _QKVPrep.apply(qkv, q_ln_weight, k_ln_weight, sin, cos, eps)


# ----------------------------------------------------------------------------
# Flash-style causal attention (reference src/model.py:71-79; plan K1/K2)
# ----------------------------------------------------------------------------
class _Attention(torch.autograd.Function):
    """dropout_p > 0: attention-matrix dropout with the stateless Philox
    keep-mask of csrc/philox.h, a pure function of (seed, b*H+h, q, k).
    Nothing is stored: the backward (and an activation-remat replay)
    regenerates the mask from the seed. ref_backend applies the bit-exact
    host mirror, so one seed gives one mask on CPU and on GPU. LSE is that of
    the undropped softmax on both backends."""

    @staticmethod
    def forward(ctx, q, k, v, dropout_p=0.0, seed=0):
        ctx.dropout_p, ctx.seed = dropout_p, seed
        impl = _backend(q)
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        if dropout_p > 0.0:
            o, lse = impl.attn_fwd_dropout(q, k, v, dropout_p, seed)
        else:
            o, lse = impl.attn_fwd(q, k, v)
        ctx.save_for_backward(q, k, v, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        impl = _backend(q)
        if ctx.dropout_p > 0.0:
            dq, dk, dv = impl.attn_bwd_dropout(do.contiguous(), q, k, v, o, lse,
                                               ctx.dropout_p, ctx.seed)
        else:
            dq, dk, dv = impl.attn_bwd(do.contiguous(), q, k, v, o, lse)
        return dq, dk, dv, None, None


def draw_dropout_seed() -> int:
    """63-bit seed from torch's default CPU generator: no device sync,
    reproducible under torch.manual_seed, replayed by torch.utils.checkpoint
    (which preserves RNG state), and sequential draws give successive
    layers different seeds."""
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())


def flash_attention(q, k, v, dropout_p: float = 0.0, seed: int | None = None):
    """Causal attention, q/k/v (B,H,T,C). Softmax scale 1/sqrt(C) in fp32.

    ``dropout_p > 0`` drops attention probabilities inside the kernels
    (fwd + bwd) with a counter-based mask keyed by ``seed``; with
    ``seed=None`` the seed is drawn by ``draw_dropout_seed``.
    ``dropout_p == 0`` is exactly the undropped path."""
    dropout_p, seed = _resolve_dropout(dropout_p, seed, "flash_attention")
    if dropout_p == 0.0:
        return _Attention.apply(q, k, v)
    return _Attention.apply(q, k, v, dropout_p, seed)


def _resolve_dropout(dropout_p, seed, who):
    """(p, seed as the int64 the bindings take); seed drawn if p > 0 and
    none was given."""
    dropout_p = float(dropout_p)
    if dropout_p == 0.0:
        return 0.0, 0
    if not 0.0 < dropout_p < 1.0:
        raise ValueError(f"{who}: dropout_p must be in [0, 1), got {dropout_p}")
    if seed is None:
        seed = draw_dropout_seed()
    return dropout_p, _seed_i64(seed)


def _seed_i64(seed) -> int:
    """The low 64 bits of ``seed`` as the int64 the bindings take."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if seed >= 1 << 63:
        seed -= 1 << 64
    return seed


# ----------------------------------------------------------------------------
# QK-LayerNorm + RoPE + causal attention over the packed projection with the
# layout copies around attention removed: qkv (B,T,3,H,C) -> o (B,T,H*C).
# The forward kernels write O as (B,T,H,C), what the output projection reads;
# the backward's delta kernel reads dO in that layout and re-lays it out for
# the dkv/dq kernels on the way; dkv writes dV into slot 2 of dqkv and the Q/K
# prep backward fills slots 0 and 1. Same arithmetic, bit for bit, as
# qkv_prep + flash_attention + transpose.
# MIDGPT_ATTN_PACKED_V=1 (read at call time) trades time for memory: no V copy
# at all, the kernels read V in place from slot 2 of qkv (one (B,T,H,C)
# activation less per layer, slower attention kernels).
# ----------------------------------------------------------------------------
class _QKVAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, qw, kw, sin, cos, dropout_p, seed, eps):
        B, T, three, H, C = qkv.shape
        assert three == 3
        qkv = qkv.contiguous()
        if os.environ.get("MIDGPT_ATTN_PACKED_V") == "1":
            q, k, qstats, kstats = _C.qk_prep_fwd(qkv, qw, kw, sin, cos, eps)
            v = qkv
        else:
            q, k, v, qstats, kstats = _C.qkv_prep_fwd(qkv, qw, kw, sin, cos, eps)
        o, lse = _C.attn_fwd_packed(q, k, v, dropout_p, seed)
        ctx.save_for_backward(qkv, qw, kw, sin, cos, q, k, v, o, lse, qstats, kstats)
        ctx.dropout_p, ctx.seed = dropout_p, seed
        return o.view(B, T, H * C)

    @staticmethod
    def backward(ctx, do):
        qkv, qw, kw, sin, cos, q, k, v, o, lse, qstats, kstats = ctx.saved_tensors
        B, T, _, H, C = qkv.shape
        dqkv = torch.empty_like(qkv)
        dq, dk = _C.attn_bwd_packed(do.reshape(B, T, H, C).contiguous(), q, k,
                                    v, o, lse, dqkv, ctx.dropout_p, ctx.seed)
        dqw, dkw = _C.qk_prep_bwd(dq, dk, qkv, qw, kw, sin, cos, qstats,
                                  kstats, dqkv)
        return dqkv, dqw, dkw, None, None, None, None, None


def qkv_attention(qkv, q_ln_weight, k_ln_weight, sin, cos,
                  dropout_p: float = 0.0, seed: int | None = None,
                  eps: float = 1e-6):
    """qkv (B,T,3,H,C) -> causal attention output (B,T,H*C).

    Dropout and seed as in ``flash_attention``: the seed is drawn on the
    host, so a ``torch.utils.checkpoint`` replay regenerates the same mask.
    Off the GPU (and under MIDGPT_GLUE_UNFUSED=1) this is the composition
    qkv_prep -> flash_attention -> transpose."""
    B, T, _, H, C = qkv.shape
    if _use_hip(qkv) and not glue_unfused():
        dropout_p, seed = _resolve_dropout(dropout_p, seed, "qkv_attention")
        return _QKVAttention.apply(qkv, q_ln_weight, k_ln_weight, sin, cos,
                                   dropout_p, seed, eps)
    q, k, v = qkv_prep(qkv, q_ln_weight, k_ln_weight, sin, cos, eps)
    o = flash_attention(q, k, v, dropout_p, seed)
    return o.transpose(1, 2).reshape(B, T, H * C)


# ----------------------------------------------------------------------------
# KV-cache decode (inference only, no autograd). Caches are (B,H,Tmax,C) and
# are written in place. GPU: csrc/decode.hip; CPU or MIDGPT_FORCE_REF=1: the
# same semantics in fp32 torch.
# ----------------------------------------------------------------------------
def _check_append(qkv, sin, cos, k_cache, v_cache, pos):
    B, Tn, three, H, C = qkv.shape
    if three != 3 or k_cache.shape != v_cache.shape or \
            tuple(k_cache.shape[:2]) + (k_cache.shape[3],) != (B, H, C):
        raise RuntimeError("kv_append: qkv must be (B,Tn,3,H,C) and the caches (B,H,Tmax,C)")
    Tmax = k_cache.shape[2]
    if Tn < 1 or pos < 0 or pos + Tn > Tmax:
        raise RuntimeError(f"kv_append: rows [{pos}, {pos + Tn}) do not fit a "
                           f"cache of {Tmax} rows")
    if sin.shape[0] < pos + Tn or cos.shape[0] < pos + Tn:
        raise RuntimeError(f"kv_append: sin/cos tables have {sin.shape[0]} rows, "
                           f"position {pos + Tn - 1} needed")


def kv_append(qkv, q_ln_weight, k_ln_weight, sin, cos, k_cache, v_cache,
              pos: int, eps: float = 1e-6):
    """QK-LayerNorm + RoPE of Tn new tokens at absolute positions
    pos .. pos+Tn-1. qkv (B,Tn,3,H,C); sin/cos are the FULL tables
    (rows >= pos+Tn, C/2). Writes K and V rows [pos, pos+Tn) of the caches in
    place (nothing else) and returns q (B,H,Tn,C)."""
    pos = int(pos)
    _check_append(qkv, sin, cos, k_cache, v_cache, pos)
    return _backend(qkv).kv_append(qkv.contiguous(), q_ln_weight, k_ln_weight,
                                   sin, cos, k_cache, v_cache, pos, eps)


def decode_attention(q, k_cache, v_cache, kv_len: int, num_splits: int = 0):
    """q (B,H,Tq,C), 1 <= Tq <= 16: the last Tq of the cache's first kv_len
    positions. Causal, end-aligned, scale 1/sqrt(C), fp32 softmax. Returns o
    (B,Tq,H*C). ``num_splits`` cuts the key range into that many slices over
    the grid (0: chosen from the sizes and the CU count; <= 64)."""
    B, H, Tq, C = q.shape
    return _backend(q).attn_decode(q.contiguous(), k_cache, v_cache, int(kv_len),
                                   int(num_splits)).view(B, Tq, H * C)


# Ragged decode: sequence b of the batch at its own position / length. The
# host values (``pos`` / ``kv_lens``: Python ints or a CPU integer tensor) are
# the truth and are validated; the kernels read an int32 GPU copy, which a
# caller may pass (``*_dev``) to upload once per step instead of once per
# layer and must then keep equal to the host values. fp32 caches select
# ref_backend on any device: that is how the eager A/B path of
# ``generate_ragged`` (MIDGPT_DECODE_REF=1) asks for it. bf16 caches on the
# GPU run the kernels, and what they do not take raises.
def _host_lens(vals, B, who):
    t = vals if isinstance(vals, torch.Tensor) else torch.tensor(list(vals))
    if t.is_cuda or t.dim() != 1 or t.shape[0] != B or t.dtype.is_floating_point \
            or t.dtype == torch.bool:
        raise RuntimeError(f"{who}: expected {B} integer positions on the host, "
                           f"got {tuple(t.shape)} {t.dtype} on {t.device}")
    return t.to(torch.int64)


def _ragged_backend(qkv, k_cache):
    return ref_backend if k_cache.dtype == torch.float32 else _backend(qkv)


def _dev_lens(host, dev, like):
    if dev is None and like.is_cuda:
        dev = host.to(device=like.device, dtype=torch.int32)
    return host if dev is None else dev


def kv_append_ragged(qkv, q_ln_weight, k_ln_weight, sin, cos, k_cache, v_cache,
                     pos, pos_dev=None, eps: float = 1e-6):
    """``kv_append`` with sequence b at positions pos[b] .. pos[b]+Tn-1 (RoPE
    rows and cache rows); Tn is uniform. Returns q (B,H,Tn,C)."""
    B, Tn = qkv.shape[:2]
    pos = _host_lens(pos, B, "kv_append_ragged")
    for p in pos.tolist():
        _check_append(qkv, sin, cos, k_cache, v_cache, p)
    return _ragged_backend(qkv, k_cache).kv_append_ragged(
        qkv.contiguous(), q_ln_weight, k_ln_weight, sin, cos, k_cache, v_cache,
        _dev_lens(pos, pos_dev, qkv), pos, eps)


def decode_attention_ragged(q, k_cache, v_cache, kv_lens, kv_lens_dev=None,
                            num_splits: int = 0):
    """``decode_attention`` with sequence b holding kv_lens[b] positions: row
    i of Tq sees keys [0, kv_lens[b] - Tq + i] of sequence b. Returns o
    (B,Tq,H*C). ``num_splits`` = 0 applies the uniform rule to the longest
    sequence; every row cuts its own range into that many slices."""
    B, H, Tq, C = q.shape
    kv_lens = _host_lens(kv_lens, B, "decode_attention_ragged")
    Tmax = k_cache.shape[2]
    for n in kv_lens.tolist():
        if n > Tmax or not 1 <= Tq <= min(16, n):
            raise RuntimeError(f"decode_attention_ragged: Tq {Tq} <= kv_len {n} <= "
                               f"{Tmax} (the cache) required, Tq <= 16")
    return _ragged_backend(q, k_cache).attn_decode_ragged(
        q.contiguous(), k_cache, v_cache, _dev_lens(kv_lens, kv_lens_dev, q),
        kv_lens, int(num_splits)).view(B, Tq, H * C)


# Slotted decode: the caches are a pool (S,H,Tmax,C) of S >= B slots and batch
# row b lives in slot slots[b], so a batch can change from step to step
# without moving a cache. ``slots`` (host: Python ints or a CPU integer
# tensor) is B distinct slots in [0, S) and is validated like the positions;
# ``slots_dev`` is the optional int32 GPU copy, under the same contract as
# ``pos_dev``. Row b has the bits of the ragged op on the gathered cache[slots].
def _host_slots(slots, B, S, who):
    slots = _host_lens(slots, B, who)
    vals = slots.tolist()
    if S < B or not all(0 <= s < S for s in vals):
        raise RuntimeError(f"{who}: {B} slots in [0, {S}) expected, got {vals}")
    if len(set(vals)) != B:
        raise RuntimeError(f"{who}: a slot is named twice in {vals} (two rows "
                           "would race on one cache)")
    return slots


def kv_append_slots(qkv, q_ln_weight, k_ln_weight, sin, cos, k_cache, v_cache,
                    pos, slots, pos_dev=None, slots_dev=None, eps: float = 1e-6):
    """``kv_append_ragged`` into a pool: qkv (B,Tn,3,H,C), caches
    (S,H,Tmax,C) with S >= B. Writes rows [pos[b], pos[b]+Tn) of slot slots[b]
    and nothing else; returns q (B,H,Tn,C)."""
    who = "kv_append_slots"
    B, Tn = qkv.shape[:2]
    pos = _host_lens(pos, B, who)
    if k_cache.dim() != 4:
        raise RuntimeError(f"{who}: the caches must be (S,H,Tmax,C)")
    slots = _host_slots(slots, B, k_cache.shape[0], who)
    for p in pos.tolist():
        _check_append(qkv, sin, cos, k_cache[:B], v_cache[:B], p)
    return _ragged_backend(qkv, k_cache).kv_append_slots(
        qkv.contiguous(), q_ln_weight, k_ln_weight, sin, cos, k_cache, v_cache,
        _dev_lens(pos, pos_dev, qkv), pos, _dev_lens(slots, slots_dev, qkv), slots, eps)


def decode_attention_slots(q, k_cache, v_cache, kv_lens, slots, kv_lens_dev=None,
                           slots_dev=None, num_splits: int = 0):
    """``decode_attention_ragged`` on a pool: sequence b holds kv_lens[b]
    positions in slot slots[b] of the caches (S,H,Tmax,C). Returns o
    (B,Tq,H*C). ``num_splits`` = 0 applies the uniform rule to the longest
    sequence, as the ragged op does."""
    who = "decode_attention_slots"
    B, H, Tq, C = q.shape
    kv_lens = _host_lens(kv_lens, B, who)
    if k_cache.dim() != 4:
        raise RuntimeError(f"{who}: the caches must be (S,H,Tmax,C)")
    slots = _host_slots(slots, B, k_cache.shape[0], who)
    Tmax = k_cache.shape[2]
    for n in kv_lens.tolist():
        if n > Tmax or not 1 <= Tq <= min(16, n):
            raise RuntimeError(f"{who}: Tq {Tq} <= kv_len {n} <= "
                               f"{Tmax} (the cache) required, Tq <= 16")
    return _ragged_backend(q, k_cache).attn_decode_slots(
        q.contiguous(), k_cache, v_cache, _dev_lens(kv_lens, kv_lens_dev, q), kv_lens,
        _dev_lens(slots, slots_dev, q), slots, int(num_splits)).view(B, Tq, H * C)


def prefill_attention(qkv, q_ln_weight, k_ln_weight, sin, cos, k_cache, v_cache,
                      eps: float = 1e-6):
    """A whole prompt at position 0: qkv (B,Tn,3,H,C) -> o (B,Tn,H*C), with
    K and V rows [0, Tn) of the caches written in place.

    On GPU the prompt runs on the MFMA flash kernel, not row by row: qkv is
    zero-padded along T to the next multiple of 128 (which must fit the
    cache), qkv_prep_fwd and attn_fwd_packed run unchanged, and rows [0, Tn)
    are kept. Padding rows are harmless: LN of a zero row is finite and
    causality hides them from the real rows."""
    B, Tn, _, H, C = qkv.shape
    if _backend(qkv) is ref_backend:
        # append, then attn_decode's math without its 16-row limit
        q = kv_append(qkv, q_ln_weight, k_ln_weight, sin, cos, k_cache, v_cache, 0, eps)
        return ref_backend._decode_attention_ref(q, k_cache, v_cache, Tn).view(B, Tn, H * C)
    _check_append(qkv, sin, cos, k_cache, v_cache, 0)
    Tp = -(-Tn // 128) * 128
    if Tp > k_cache.shape[2]:
        raise RuntimeError(f"prefill_attention: {Tn} rows pad to {Tp}, over the "
                           f"cache's {k_cache.shape[2]}")
    pad = Tp - Tn
    if pad:
        qkv = torch.nn.functional.pad(qkv, (0, 0, 0, 0, 0, 0, 0, pad))
    sin, cos = sin[:Tp], cos[:Tp]
    if sin.shape[0] < Tp:  # tables end inside the padding: any finite row does
        extra = (0, 0, 0, Tp - sin.shape[0])
        sin = torch.nn.functional.pad(sin, extra)
        cos = torch.nn.functional.pad(cos, extra)
    q, k, v, _, _ = _C.qkv_prep_fwd(qkv.contiguous(), q_ln_weight, k_ln_weight,
                                    sin, cos, eps)
    o, _ = _C.attn_fwd_packed(q, k, v)          # (B,Tp,H,C)
    k_cache[:, :, :Tn].copy_(k[:, :, :Tn])
    v_cache[:, :, :Tn].copy_(v[:, :, :Tn])
    return o[:, :Tn].reshape(B, Tn, H * C)


# Paged decode: the caches are pools (P,H,PS,C) of P pages of PS positions (a
# power of two in [16, 128]) and position p of batch row b lives at row p % PS
# of page block_table[b][p // PS]; MP*PS stands where Tmax stands above and
# unassigned entries are -1. ``block_table`` (host: nested ints or a CPU
# integer tensor (B,MP)) is the truth and is validated by the backend: every
# entry that covers the positions a call touches lies in [0, P), and the pages
# that receive writes are distinct (attention may name one page in several
# rows). ``block_table_dev`` is the optional int32 GPU copy, under the same
# contract as ``pos_dev``. Row b has the bits of the ragged op on the cache
# gathered through the table.
def _host_table(table, B, who):
    t = table if isinstance(table, torch.Tensor) else torch.tensor(table)
    if t.is_cuda or t.dim() != 2 or t.shape[0] != B or t.shape[1] < 1 \
            or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise RuntimeError(f"{who}: expected a ({B}, MP) integer block table on the "
                           f"host, got {tuple(t.shape)} {t.dtype} on {t.device}")
    return t.to(torch.int64)


def _check_pools(k_pool, v_pool, H, C, who):
    if k_pool.dim() != 4 or k_pool.shape != v_pool.shape or \
            (k_pool.shape[1], k_pool.shape[3]) != (H, C):
        raise RuntimeError(f"{who}: the pools must be (P,{H},PS,{C}), got "
                           f"{tuple(k_pool.shape)} and {tuple(v_pool.shape)}")


def kv_append_paged(qkv, q_ln_weight, k_ln_weight, sin, cos, k_pool, v_pool,
                    pos, block_table, pos_dev=None, block_table_dev=None,
                    eps: float = 1e-6):
    """``kv_append_ragged`` into paged pools: qkv (B,Tn,3,H,C), pools
    (P,H,PS,C). Writes positions [pos[b], pos[b]+Tn) of sequence b into the
    pages its table row names and nothing else; returns q (B,H,Tn,C)."""
    who = "kv_append_paged"
    B, Tn, three, H, C = qkv.shape
    if three != 3 or Tn < 1:
        raise RuntimeError(f"{who}: qkv must be (B,Tn,3,H,C) with Tn >= 1")
    pos = _host_lens(pos, B, who)
    table = _host_table(block_table, B, who)
    _check_pools(k_pool, v_pool, H, C, who)
    return _ragged_backend(qkv, k_pool).kv_append_paged(
        qkv.contiguous(), q_ln_weight, k_ln_weight, sin, cos, k_pool, v_pool,
        _dev_lens(pos, pos_dev, qkv), pos, _dev_lens(table, block_table_dev, qkv), table,
        eps)


def decode_attention_paged(q, k_pool, v_pool, kv_lens, block_table, kv_lens_dev=None,
                           block_table_dev=None, num_splits: int = 0):
    """``decode_attention_ragged`` on paged pools: sequence b holds kv_lens[b]
    positions in the pages of its table row. Returns o (B,Tq,H*C).
    ``num_splits`` = 0 applies the uniform rule to the longest sequence, as
    the ragged op does."""
    who = "decode_attention_paged"
    B, H, Tq, C = q.shape
    kv_lens = _host_lens(kv_lens, B, who)
    table = _host_table(block_table, B, who)
    _check_pools(k_pool, v_pool, H, C, who)
    return _ragged_backend(q, k_pool).attn_decode_paged(
        q.contiguous(), k_pool, v_pool, _dev_lens(kv_lens, kv_lens_dev, q), kv_lens,
        _dev_lens(table, block_table_dev, q), table, int(num_splits)).view(B, Tq, H * C)


def kv_store_paged(k, v, k_pool, v_pool, lens, block_table, block_table_dev=None):
    """Rows [0, lens[b]) of contiguous k, v (B,H,T,C) into the pages of
    sequence b's table row, in place; nothing else is written."""
    who = "kv_store_paged"
    B, H, T, C = k.shape
    lens = _host_lens(lens, B, who)
    table = _host_table(block_table, B, who)
    _check_pools(k_pool, v_pool, H, C, who)
    _ragged_backend(k, k_pool).kv_store_paged(
        k.contiguous(), v.contiguous(), k_pool, v_pool, _dev_lens(lens, None, k), lens,
        _dev_lens(table, block_table_dev, k), table)


def prefill_attention_paged(qkv, q_ln_weight, k_ln_weight, sin, cos, k_pool, v_pool,
                            block_table, block_table_dev=None, eps: float = 1e-6):
    """``prefill_attention`` into paged pools: whole prompts at position 0,
    qkv (B,Tn,3,H,C) -> o (B,Tn,H*C), with positions [0, Tn) of every sequence
    written into the pages of its table row. On GPU: the same qkv_prep_fwd +
    attn_fwd_packed on the prompt padded to a multiple of 128 rows, then
    ``kv_store_paged`` of rows [0, Tn) where the contiguous caches take a
    copy. On ref_backend (the CPU, fp32 pools): the paged append, then
    attn_decode's math on the gathered cache without its 16-row limit."""
    who = "prefill_attention_paged"
    B, Tn, _, H, C = qkv.shape
    table = _host_table(block_table, B, who)
    _check_pools(k_pool, v_pool, H, C, who)
    PS = k_pool.shape[2]
    if Tn > table.shape[1] * PS:
        raise RuntimeError(f"{who}: {Tn} rows do not fit the table's {table.shape[1] * PS}")
    if _ragged_backend(qkv, k_pool) is ref_backend:
        q = kv_append_paged(qkv, q_ln_weight, k_ln_weight, sin, cos, k_pool, v_pool,
                            [0] * B, table, None, block_table_dev, eps)
        return torch.cat([ref_backend._decode_attention_ref(
            q[b:b + 1], ref_backend._gather_pages(k_pool, table, b, Tn, PS),
            ref_backend._gather_pages(v_pool, table, b, Tn, PS), Tn)
            for b in range(B)], dim=0).view(B, Tn, H * C)
    if sin.shape[0] < Tn or cos.shape[0] < Tn:
        raise RuntimeError(f"{who}: sin/cos tables have {sin.shape[0]} rows, "
                           f"position {Tn - 1} needed")
    Tp = -(-Tn // 128) * 128
    pad = Tp - Tn
    if pad:
        qkv = torch.nn.functional.pad(qkv, (0, 0, 0, 0, 0, 0, 0, pad))
    sin, cos = sin[:Tp], cos[:Tp]
    if sin.shape[0] < Tp:  # tables end inside the padding: any finite row does
        extra = (0, 0, 0, Tp - sin.shape[0])
        sin = torch.nn.functional.pad(sin, extra)
        cos = torch.nn.functional.pad(cos, extra)
    q, k, v, _, _ = _C.qkv_prep_fwd(qkv.contiguous(), q_ln_weight, k_ln_weight,
                                    sin, cos, eps)
    o, _ = _C.attn_fwd_packed(q, k, v)          # (B,Tp,H,C)
    kv_store_paged(k, v, k_pool, v_pool, [Tn] * B, table, block_table_dev)
    return o[:, :Tn].reshape(B, Tn, H * C)


# ----------------------------------------------------------------------------
# Seeded token sampling (inference only): one token per row of logits, a pure
# function of (seed, step, row, logits), so the same seed gives the same draw
# on the CPU and on the GPU and nothing crosses to the host. GPU, contiguous
# bf16: csrc/sampling.hip, one launch. Everything else (fp32 logits, strided
# logits, the CPU, MIDGPT_FORCE_REF=1): ref_backend, the same definition.
# ----------------------------------------------------------------------------
def sample_tokens(logits, temperature: float, top_k: int | None = None, *,
                  seed: int, step: int):
    """logits (B, V) -> tokens (B,) int64 drawn from
    softmax(logits / temperature), restricted with ``top_k`` to the entries
    >= the row's k-th largest logit (ties with it kept; None, 0 or >= V: all).

    Gumbel-max with counter-based noise: entry v of row b at token ``step``
    (in [0, 2^32)) takes a Philox word keyed by the 64-bit ``seed`` at counter
    (v >> 2, b, step), see csrc/philox.h. The draw of a row therefore depends
    on its index in the batch. ``temperature`` must be > 0: greedy decoding is
    ``argmax``, not a mode of this op."""
    temperature = float(temperature)
    if not temperature > 0.0:
        raise ValueError(f"sample_tokens: temperature must be > 0, got {temperature}")
    # fp32(1/T), computed once, is what every backend multiplies by
    inv_t = torch.tensor(1.0 / temperature, dtype=torch.float32).item()
    if not (math.isfinite(inv_t) and inv_t > 0.0):
        raise ValueError(f"sample_tokens: 1/temperature is {inv_t} in fp32")
    top_k = 0 if top_k is None else int(top_k)
    if top_k < 0:
        raise ValueError(f"sample_tokens: top_k must be >= 0, got {top_k}")
    step = int(step)
    if not 0 <= step < 1 << 32:
        raise ValueError(f"sample_tokens: step must be in [0, 2^32), got {step}")
    if logits.dim() != 2:
        raise ValueError(f"sample_tokens: logits must be (B, V), got {tuple(logits.shape)}")
    impl = _backend(logits)
    if logits.dtype != torch.bfloat16 or not logits.is_contiguous():
        impl = ref_backend
    return impl.sample_tokens(logits, inv_t, top_k, _seed_i64(seed), step)


def sample_row_params(temperature, top_k, seeds, steps, rows, B: int):
    """The per-row arguments of ``sample_tokens_rows`` as the five validated
    host tensors a backend takes: (inv_t float32, top_k, seeds, steps, rows
    int64), each (B,). ``temperature`` and ``top_k`` may be one value for every
    row; temperature <= 0 marks a greedy row (inv_t 0); top_k None or 0: all."""
    def seq(x, name):
        x = list(x) if hasattr(x, "__len__") else [x] * B
        if len(x) != B:
            raise RuntimeError(f"sample_tokens_rows: {B} values of {name} expected, "
                               f"got {len(x)}")
        return x
    inv_t = []
    for t in seq(temperature, "temperature"):
        t, it = float(t), 0.0
        if t > 0.0:
            # fp32(1/T), computed once, is what every backend multiplies by
            it = torch.tensor(1.0 / t, dtype=torch.float32).item()
            if not (math.isfinite(it) and it > 0.0):
                raise RuntimeError(f"sample_tokens_rows: 1/temperature is {it} in fp32")
        inv_t.append(it)
    ks = [0 if k is None else int(k) for k in seq(top_k, "top_k")]
    if min(ks, default=0) < 0:
        raise RuntimeError(f"sample_tokens_rows: top_k must be >= 0, got {ks}")
    seeds = [_seed_i64(x) for x in seq(seeds, "seeds")]
    steps = [int(x) for x in seq(steps, "steps")]
    rows = [int(x) for x in seq(rows, "rows")]
    for name, vals in (("step", steps), ("row", rows)):
        if not all(0 <= x < 1 << 32 for x in vals):
            raise RuntimeError(f"sample_tokens_rows: {name} must be in [0, 2^32), got {vals}")
    i64 = lambda x: torch.tensor(x, dtype=torch.int64)
    return (torch.tensor(inv_t, dtype=torch.float32), i64(ks), i64(seeds), i64(steps),
            i64(rows))


def pack_sample_params(inv_t, top_k, seeds, steps, rows, device=None):
    """What the kernel reads of ``sample_row_params``' tensors: (B, 6) int32,
    row b = {seed low word, seed high word, step, row, bits of fp32 inv_t,
    top_k clamped to int32} (csrc/sampling.hip). Column 2 is the step: a
    caller that keeps the tensor advances it there."""
    # the low 32 bits of an int64 as the int32 of the same bit pattern
    u32 = lambda x: ((x & 0xFFFFFFFF) - ((x & 0x80000000) << 1)).to(torch.int32)
    p = torch.stack([u32(seeds), u32(seeds >> 32), u32(steps), u32(rows),
                     inv_t.view(torch.int32),
                     top_k.clamp(max=2 ** 31 - 1).to(torch.int32)], dim=1).contiguous()
    return p if device is None else p.to(device)


def sample_tokens_rows(logits, temperature, top_k=None, *, seeds, steps, rows,
                       params_dev=None):
    """``sample_tokens`` with per-row parameters: logits (B, V) -> tokens (B,)
    int64, row b drawn with its own temperature[b], top_k[b], seeds[b] and
    steps[b], and with rows[b] as the Philox counter word that
    ``sample_tokens`` fills with the batch index. So
    ``out[b] == sample_tokens(X, T_b, k_b, seed=s_b, step=t_b)[r_b]`` for any X
    whose row r_b is logits[b]: what a request draws does not depend on who
    shares its batch. The per-row arguments are host sequences of length B
    (temperature and top_k may be one value); they are the truth and are
    validated. A row with temperature <= 0 is greedy: the lowest index of the
    largest logit, ``top_k`` ignored.

    ``params_dev``: the optional GPU copy, ``pack_sample_params(...)``, which a
    caller uploads once and keeps equal to the host values (advancing the step
    column on the device). Contiguous bf16 logits on the GPU run
    csrc/sampling.hip; everything else goes to ref_backend."""
    if logits.dim() != 2:
        raise ValueError(f"sample_tokens_rows: logits must be (B, V), got {tuple(logits.shape)}")
    B = logits.shape[0]
    host = sample_row_params(temperature, top_k, seeds, steps, rows, B)
    impl = _backend(logits)
    if logits.dtype != torch.bfloat16 or not logits.is_contiguous():
        impl = ref_backend
    if params_dev is None:
        params_dev = pack_sample_params(*host, device=logits.device)
    return impl.sample_tokens_rows(logits, params_dev, *host)


def draw_sample_seed() -> int:
    """A seed for ``sample_tokens`` from torch's default CPU generator, as
    ``draw_dropout_seed`` draws one: no device sync, reproducible under
    torch.manual_seed."""
    return draw_dropout_seed()


# ----------------------------------------------------------------------------
# GELU (tanh approx) fwd/bwd (reference src/model.py:30; plan K7): a
# hand-written u16x8 elementwise pair replacing the torch library kernels
# (same numerics as F.gelu(approximate="tanh"); fp32 internal). The pair is
# bf16 with numel % 8 == 0; ref_backend takes everything else on the GPU too.
# ----------------------------------------------------------------------------
class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        impl = _backend(x)
        if x.dtype != torch.bfloat16 or x.numel() % 8:
            impl = ref_backend
        return impl.gelu_fwd(x.contiguous())

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        impl = _backend(x)
        if x.dtype != torch.bfloat16 or x.numel() % 8:
            impl = ref_backend
        return impl.gelu_bwd(dy.contiguous(), x.contiguous())


def gelu(x):
    return _Gelu.apply(x)


# ----------------------------------------------------------------------------
# Embedding: gather fwd, scatter-add bwd (reference src/layers.py:13-34;
# plan K8). The forward gather is a plain coalesced index_select (torch);
# the backward is the hand-written HIP fp32-accurate scatter-add (bf16).
# ----------------------------------------------------------------------------
class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, weight):
        ctx.save_for_backward(idx)
        ctx.V = weight.shape[0]
        return weight[idx]

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        dy2d = dy.reshape(-1, dy.shape[-1])
        impl = _backend(dy)
        if dy.dtype != torch.bfloat16:
            impl = ref_backend
        return None, impl.embedding_bwd(dy2d.contiguous(), idx.reshape(-1), ctx.V)


def embedding(idx, weight):
    """idx (...,) int64, weight (V, D) -> (..., D)."""
    return _Embedding.apply(idx, weight)


# ----------------------------------------------------------------------------
# Fused softmax cross-entropy over the vocab (reference src/train.py:76-77;
# plan K9). Never materializes the fp32 softmax over V on the HIP path.
# ----------------------------------------------------------------------------
class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets):
        loss_sum, lse = _backend(logits).ce_fwd(logits, targets)
        ctx.save_for_backward(logits, targets, lse)
        return loss_sum / logits.shape[0]

    @staticmethod
    def backward(ctx, dloss):
        logits, targets, lse = ctx.saved_tensors
        dlogits = _backend(logits).ce_bwd(logits, targets, lse,
                                          dloss.float().reshape(1))
        return dlogits, None


def cross_entropy(logits, targets):
    """logits (N,V), targets (N,) int64 -> scalar mean loss (fp32)."""
    return _CrossEntropy.apply(logits, targets)


# ----------------------------------------------------------------------------
# hipBLASLt DGELU-fused MLP backward: the gelu backward lives in the dgrad
# GEMM epilogue — no separate elementwise gelu-backward kernel (plan K7).
# (GELU_AUX forward fusion has no gfx950 hipblaslt algorithms on ROCm 7.2 —
# probed via _C.lt_probe — so the forward keeps torch's GEMM + gelu;
# numerics: hipBLASLt GELU is the tanh approximation, matching the
# reference jax.nn.gelu default.)
# ----------------------------------------------------------------------------
class _FusedMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2d, w1, w2):
        h = torch.mm(x2d, w1.t())
        g = torch.nn.functional.gelu(h, approximate="tanh")
        y = torch.mm(g, w2.t())
        ctx.save_for_backward(x2d, w1, w2, h, g)
        return y

    @staticmethod
    def backward(ctx, dy):
        x2d, w1, w2, h, g = ctx.saved_tensors
        dy = dy.contiguous()
        dh = _C.matmul_dgelu(dy, w2, h)      # dgrad GEMM + dgelu epilogue
        dw2 = torch.mm(dy.t(), g)
        dx = torch.mm(dh, w1)
        dw1 = torch.mm(dh.t(), x2d)
        return dx, dw1, dw2


def fused_mlp(x, w1, w2):
    """x (..., D) -> gelu(x @ w1.T) @ w2.T with GEMM-epilogue GELU."""
    shp = x.shape
    y = _FusedMLP.apply(x.reshape(-1, shp[-1]).contiguous(), w1, w2)
    return y.reshape(*shp[:-1], w2.shape[0])


# ----------------------------------------------------------------------------
# Linear with a transposed weight image. The forward is F.linear, unchanged.
# The backward reads dx from ``wt`` = w.t() stored (in, out): dx = dy wt^T is
# then the forward's TN GEMM layout, which hipBLASLt runs 11-16 % faster on
# gfx950 than the NN layout of dx = dy w at the model's shapes
# (profiles/dgrad_wt.md). dW is the NT call autograd issues for F.linear.
# ``wt`` is a cache the caller keeps equal to w.t(); it gets no gradient.
# ----------------------------------------------------------------------------
class _LinearWt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, wt):
        ctx.save_for_backward(x, wt)
        return torch.nn.functional.linear(x, w)

    @staticmethod
    def backward(ctx, dy):
        x, wt = ctx.saved_tensors
        dy2d = dy.reshape(-1, dy.shape[-1])
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = dy2d.mm(wt.t()).view(x.shape)
        if ctx.needs_input_grad[1]:
            dw = dy2d.t().mm(x.reshape(-1, x.shape[-1]))
        return dx, dw, None


def linear_wt(x, w, wt):
    """x (..., in) @ w(out, in)^T with the dgrad read from wt (in, out), which
    must hold w.t() (the training engine refreshes it after every write of
    the weights). x, w and wt share one dtype."""
    if wt.shape != (w.shape[1], w.shape[0]) or not (x.dtype == w.dtype == wt.dtype):
        raise RuntimeError(f"linear_wt: w {tuple(w.shape)} {w.dtype} needs an image "
                           f"{(w.shape[1], w.shape[0])} of its dtype and x's "
                           f"({x.dtype}), got {tuple(wt.shape)} {wt.dtype}")
    return _LinearWt.apply(x, w, wt)


# ----------------------------------------------------------------------------
# Batched transpose: every matrix of a table, from offsets of one flat buffer
# to offsets of another, in one launch (csrc/transpose.hip; any dtype on
# ref_backend, bf16 on the GPU).
# ----------------------------------------------------------------------------
TRANSPOSE_TILE = ref_backend.TRANSPOSE_TILE


def transpose_table(entries, device=None):
    """(table_dev, table_host) for ``transpose_batched`` from (src_off,
    dst_off, rows, cols) per matrix: int64 (n, 5), the fifth column the count
    of 64x64 tiles before the matrix."""
    rows5, tiles = [], 0
    for (so, do, r, c) in entries:
        rows5.append([int(so), int(do), int(r), int(c), tiles])
        tiles += -(-int(r) // TRANSPOSE_TILE) * -(-int(c) // TRANSPOSE_TILE)
    host = torch.tensor(rows5, dtype=torch.int64).reshape(-1, 5)
    return (host if device is None else host.to(device)), host


def transpose_batched(src, dst, table_dev, table_host, max_blocks: int = 0):
    """dst[dst_off : dst_off + rows*cols] viewed (cols, rows) becomes the
    transpose of src[src_off : src_off + rows*cols] viewed (rows, cols), for
    every row of the table (``transpose_table``). Nothing else of dst is
    written. ``table_host`` is the truth and is validated; ``table_dev`` is
    the copy the kernel reads, under the same contract as ``pos_dev``.
    ``max_blocks`` caps the grid (0: sized for the device)."""
    _backend(src).transpose_batched(src, dst, table_dev, table_host, int(max_blocks))


# ----------------------------------------------------------------------------
# Fused AdamW step on flat buffers (plan K10/K13). Semantics match the optax
# chain clip_by_global_norm(1.0) -> scale_by_adam -> add_decayed_weights(
# wd/lr_peak) -> scale_by_schedule -> scale(-1)  (reference src/train.py:153-159).
# ----------------------------------------------------------------------------
def adamw_step(master: torch.Tensor, grad: torch.Tensor, m: torch.Tensor,
               v: torch.Tensor, out_bf16: torch.Tensor | None,
               *, lr: float, beta1: float, beta2: float, eps: float,
               wd_over_peak_lr: float, grad_scale: float, clip_norm: float,
               sq_sum: torch.Tensor, step: int):
    """In-place AdamW on flat fp32 buffers; optionally writes the bf16
    working copy. ``step`` is 1-indexed (bias correction t).

    The effective gradient is ``grad * grad_scale * clip`` where
    ``clip = min(1, clip_norm / (grad_scale * sqrt(sq_sum)))`` — computed
    ON DEVICE from the (already all-reduced) squared-norm scalar ``sq_sum``
    so the step path never syncs to host (ref_backend does sync).
    """
    _backend(master).adamw_step(master, grad, m, v,
                                out_bf16 if out_bf16 is not None
                                else master.new_empty(0, dtype=torch.bfloat16),
                                out_bf16 is not None, sq_sum,
                                lr, beta1, beta2, eps, wd_over_peak_lr,
                                grad_scale, clip_norm, step)
