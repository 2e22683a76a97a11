"""Autoregressive generation with incremental KV-cache decode.

Functional parity with the reference generate() (sample.py:68-95):
temperature-scaled categorical sampling from the last position's logits,
cropping to block_size. Improvement: an incremental KV cache while the
sequence fits in block_size (the reference re-runs the full forward per
token). Once the window slides past block_size we fall back to the
reference's recompute-from-cropped-window behavior so RoPE positions
match exactly.

Two decode paths. The native one (``KVCache`` + ``decode_step``) keeps K and V
in one preallocated buffer and runs the step on the HIP decode kernels
(``ops.kv_append`` / ``ops.decode_attention`` / ``ops.prefill_attention``);
``generate`` takes it for a bf16 model on the GPU with head dim 64 or 128 and
block_size % 128 == 0. Everything else (CPU, other dtypes and shapes, or
``MIDGPT_DECODE_REF=1``, read at call time, for A/B) runs the eager path
below, built from the fp32 reference ops.

``generate_ragged`` decodes a batch of prompts of different lengths in one
step per token (``prefill_ragged`` + ``decode_step_ragged`` on
``ops.kv_append_ragged`` / ``ops.decode_attention_ragged``): per-sequence
lengths in the ``KVCache``, every sequence advancing by the same number of
tokens per step. It has no sliding window (a sequence whose cache is full is
finished) and does not compact the batch when sequences finish.

``DecodeScheduler`` / ``generate_continuous`` do: the ``KVCache`` is a pool of
slots, a step runs the rows named by a slot map (``decode_step_slots`` on
``ops.kv_append_slots`` / ``ops.decode_attention_slots``), requests join and
leave between steps, and every request samples with its own parameters
(``ops.sample_tokens_rows``), so its text does not depend on its batch. With
``num_pages`` the pool is a ``PagedKVCache``: a request holds only the pages
it can write, found through a block table (``decode_step_paged`` on
``ops.kv_append_paged`` / ``ops.decode_attention_paged``).
"""
from __future__ import annotations

import collections
import math
import os

import torch
import torch.nn.functional as F

from midgpt_amd import ops
from midgpt_amd.ops import reference as ref


def _attn_cached(q, k, v):
    """q: (B,H,Tq,C) attends to k,v: (B,H,Tk,C) with causal alignment at the
    END (the Tq new positions are the last Tq of Tk). fp32 softmax."""
    B, H, Tq, C = q.shape
    Tk = k.shape[2]
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) / math.sqrt(C)
    if Tq > 1:
        qpos = torch.arange(Tk - Tq, Tk, device=q.device)[:, None]
        kpos = torch.arange(Tk, device=q.device)[None, :]
        s = s.masked_fill(kpos > qpos, float("-inf"))
    a = torch.softmax(s, dim=-1).to(v.dtype)
    return torch.matmul(a, v)


def _eager_step(model, idx_new: torch.Tensor, cache: list, pos: int):
    """Run idx_new (B, Tnew) through the model appending to cache; returns
    last-position logits (B, V)."""
    cfg = model.config
    H, C = cfg.n_head, cfg.head_dim
    B, Tn = idx_new.shape
    sin = model.rope_sin[pos:pos + Tn]
    cos = model.rope_cos[pos:pos + Tn]
    x = F.embedding(idx_new, model.wte)
    for li, blk in enumerate(model.blocks):
        h = ref.rmsnorm(x, None, 1e-6)
        qkv = blk.attn.c_attn(h).view(B, Tn, 3, H, C)
        q = qkv[:, :, 0].permute(0, 2, 1, 3)
        k = qkv[:, :, 1].permute(0, 2, 1, 3)
        v = qkv[:, :, 2].permute(0, 2, 1, 3)
        q = ref.qk_layernorm(q, blk.attn.q_ln_weight)
        k = ref.qk_layernorm(k, blk.attn.k_ln_weight)
        q = ref.apply_rope(q, sin, cos)
        k = ref.apply_rope(k, sin, cos)
        if cache[li] is None:
            cache[li] = (k, v)
        else:
            pk, pv = cache[li]
            cache[li] = (torch.cat([pk, k], dim=2), torch.cat([pv, v], dim=2))
        k, v = cache[li]
        o = _attn_cached(q, k, v)
        o = o.transpose(1, 2).reshape(B, Tn, cfg.n_embd)
        x = x + blk.attn.c_proj(o)
        x = x + blk.mlp(ref.rmsnorm(x, None, 1e-6))
    x = ref.rmsnorm(x[:, -1:], None, 1e-5)
    return model.lm_head(x)[:, -1]


class KVCache:
    """Preallocated K/V of every layer for ``batch_size`` sequences of up to
    block_size positions: one buffer (n_layer, 2, B, H, block_size, C), with
    per-layer views ``k[l]`` / ``v[l]`` of shape (B, H, block_size, C) and the
    number of valid positions ``pos`` kept on the host. Rows >= pos hold
    stale or uninitialised data and are never read.

    The ragged path keeps per-sequence lengths instead of ``pos``: the host
    list ``lens`` and its int32 device mirror ``lens_dev``, uploaded by
    ``set_lens`` and from then on advanced on the device by the same rule as
    on the host (``decode_step_ragged``), so no step uploads or syncs."""

    def __init__(self, model, batch_size: int, device=None, dtype=None):
        cfg = model.config
        device = model.wte.device if device is None else device
        dtype = model.wte.dtype if dtype is None else dtype
        self.block_size = cfg.block_size
        self.buf = torch.empty(cfg.n_layer, 2, batch_size, cfg.n_head,
                               cfg.block_size, cfg.head_dim, device=device,
                               dtype=dtype)
        self.k = [self.buf[li, 0] for li in range(cfg.n_layer)]
        self.v = [self.buf[li, 1] for li in range(cfg.n_layer)]
        # the kernels take fp32 LN weights: convert once, not per token
        self.ln_w = [(blk.attn.q_ln_weight.detach().float(),
                      blk.attn.k_ln_weight.detach().float())
                     for blk in model.blocks]
        self.pos = 0
        self.lens = [0] * batch_size
        self.lens_dev = torch.zeros(batch_size, dtype=torch.int32, device=device)

    def reset(self):
        self.pos = 0
        self.lens = [0] * len(self.lens)
        self.lens_dev.zero_()

    def set_lens(self, lens):
        """Per-sequence valid positions: host list and device mirror."""
        lens = [int(n) for n in lens]
        if len(lens) != len(self.lens) or not all(0 <= n <= self.block_size for n in lens):
            raise RuntimeError(f"KVCache.set_lens: {len(self.lens)} lengths in "
                               f"[0, {self.block_size}] expected, got {lens}")
        self.lens = lens
        self.lens_dev.copy_(torch.tensor(lens, dtype=torch.int32))


def _attend_cached(qkv, qw, kw, sin, cos, k_cache, v_cache, pos):
    """Append qkv (B,Tn,3,H,C) at pos and attend: -> o (B,Tn,H*C)."""
    Tn = qkv.shape[1]
    fits = not qkv.is_cuda or -(-Tn // 128) * 128 <= k_cache.shape[2]
    if pos == 0 and Tn > 16 and fits:
        return ops.prefill_attention(qkv, qw, kw, sin, cos, k_cache, v_cache)
    outs = []
    for s in range(0, Tn, 16):  # decode_attention takes at most 16 rows
        chunk = qkv[:, s:s + 16]
        q = ops.kv_append(chunk, qw, kw, sin, cos, k_cache, v_cache, pos + s)
        outs.append(ops.decode_attention(q, k_cache, v_cache,
                                         pos + s + chunk.shape[1]))
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)


@torch.no_grad()
def decode_step(model, idx_new: torch.Tensor, cache: KVCache) -> torch.Tensor:
    """Run idx_new (B, Tn) at positions cache.pos .. cache.pos+Tn-1, appending
    their K/V to the cache; returns the last position's logits (B, V)."""
    cfg = model.config
    H, C = cfg.n_head, cfg.head_dim
    B, Tn = idx_new.shape
    pos = cache.pos
    if pos + Tn > cache.block_size:
        raise RuntimeError(f"decode_step: positions [{pos}, {pos + Tn}) exceed "
                           f"block_size {cache.block_size}")
    sin, cos = model.rope_sin, model.rope_cos
    x = F.embedding(idx_new, model.wte)
    pending = None  # residual-pending form of GPT.forward
    for li, blk in enumerate(model.blocks):
        if pending is None:
            h = ops.rmsnorm(x, None, 1e-6)
        else:
            x, h = ops.add_rmsnorm(x, pending, 1e-6)
        qkv = blk.attn.c_attn(h).view(B, Tn, 3, H, C)
        qw, kw = cache.ln_w[li]
        o = _attend_cached(qkv, qw, kw, sin, cos, cache.k[li], cache.v[li], pos)
        x, h = ops.add_rmsnorm(x, blk.attn.c_proj(o), 1e-6)
        pending = blk.mlp(h)
    cache.pos = pos + Tn
    if pending is None:  # no blocks
        h = ops.rmsnorm(x[:, -1:], None, 1e-5)
    else:
        _, h = ops.add_rmsnorm(x[:, -1:], pending[:, -1:], 1e-5)
    return model.lm_head(h)[:, -1]


def decode_ref() -> bool:
    """MIDGPT_DECODE_REF=1 (read at call time) keeps ``generate`` on the
    eager decode path: the A/B handle for the native one."""
    return os.environ.get("MIDGPT_DECODE_REF") == "1"


def native_decode(model) -> bool:
    """Whether ``generate`` decodes this model on the HIP decode kernels."""
    cfg = model.config
    return (model.wte.is_cuda and model.wte.dtype == torch.bfloat16
            and model.rope_sin.dtype == torch.float32
            and cfg.head_dim in (64, 128) and cfg.block_size % 128 == 0
            and not decode_ref())


def decode_stepper(model, batch_size: int):
    """step(tokens (B,Tn), pos) -> last-position logits (B,V) on the path
    ``generate`` takes for this model: native (``KVCache`` + ``decode_step``)
    or eager. pos is the absolute position of tokens[:, 0]; pos == 0 starts a
    new sequence, otherwise it must continue the previous call."""
    if native_decode(model):
        kv = KVCache(model, batch_size)

        def step(tokens, pos):
            if pos == 0:
                kv.reset()
            assert pos == kv.pos, (pos, kv.pos)
            return decode_step(model, tokens, kv)
    else:
        cache = [None] * model.config.n_layer

        @torch.no_grad()
        def step(tokens, pos):
            if pos == 0:
                cache[:] = [None] * model.config.n_layer
            return _eager_step(model, tokens, cache, pos)
    return step


@torch.no_grad()
def generate(model, idx: torch.Tensor, max_new_tokens: int,
             temperature: float = 1.0, top_k: int | None = None,
             generator: torch.Generator | None = None,
             seed: int | None = None) -> torch.Tensor:
    """idx (B, T0) int64 -> (B, T0 + max_new_tokens).

    With ``seed`` (and temperature > 0) token t of the call, counted from 0
    through a slid window too, is ``ops.sample_tokens(logits, temperature,
    top_k, seed=seed, step=t)`` with row = batch index: one launch per token
    on the native path, no host round trip, the same text on the CPU and on
    the GPU wherever the logits agree. Without it the draw is
    ``torch.multinomial`` from ``generator`` or the global RNG."""
    _check_seed(seed, generator)
    model.eval()
    block = model.config.block_size
    step = decode_stepper(model, idx.shape[0])
    # prompts longer than block_size condition on the last block_size tokens
    # (reference sample.py:74-81 crops to the trailing window)
    logits = step(idx[:, -block:], 0)
    for t in range(max_new_tokens):
        nxt = _next_token(logits, temperature, top_k, generator, seed, t)
        idx = torch.cat([idx, nxt[:, None]], dim=1)
        if idx.shape[1] <= block:
            logits = step(nxt[:, None], idx.shape[1] - 1)
        else:
            # window slid: reference behavior — recompute the cropped window
            # from position 0 (the cached positions are invalid from here on)
            logits = step(idx[:, -block:], 0)
    return idx


def _ragged_layers(model, idx, attend):
    """The layer loop of ``decode_step`` with attention left to
    ``attend(li, qkv (B,Tn,3,H,C)) -> o (B,Tn,H*C)``. Returns (x, pending):
    the residual stream before the last MLP's output is added."""
    cfg = model.config
    H, C = cfg.n_head, cfg.head_dim
    B, Tn = idx.shape
    x = F.embedding(idx, model.wte)
    pending = None  # residual-pending form of GPT.forward
    for li, blk in enumerate(model.blocks):
        if pending is None:
            h = ops.rmsnorm(x, None, 1e-6)
        else:
            x, h = ops.add_rmsnorm(x, pending, 1e-6)
        qkv = blk.attn.c_attn(h).view(B, Tn, 3, H, C)
        x, h = ops.add_rmsnorm(x, blk.attn.c_proj(attend(li, qkv)), 1e-6)
        pending = blk.mlp(h)
    return x, pending


def _ragged_logits(model, x, pending):
    """Final norm + lm_head of one row per sequence: x, pending (B,1,D)."""
    if pending is None:  # no blocks
        h = ops.rmsnorm(x, None, 1e-5)
    else:
        _, h = ops.add_rmsnorm(x, pending, 1e-5)
    return model.lm_head(h)[:, -1]


def _native_cache(cache: KVCache) -> bool:
    return cache.buf.is_cuda and cache.buf.dtype == torch.bfloat16


def _prefill_attend(model, cache: KVCache, ks, vs, B, Lmax):
    """``attend`` of ``_ragged_layers`` for B prompts run from position 0 into
    the per-layer caches ``ks`` / ``vs`` (B,H,block_size,C): ``cache``'s own
    views, or one slot of them."""
    sin, cos = model.rope_sin, model.rope_cos
    if _native_cache(cache) or not cache.buf.is_cuda:
        def attend(li, qkv):
            qw, kw = cache.ln_w[li]
            return _attend_cached(qkv, qw, kw, sin, cos, ks[li], vs[li], 0)
    else:
        # ref_backend on the GPU (fp32 caches): the uniform ops would pick the
        # kernels there, so the 16-row chunks go through the ragged pair
        def attend(li, qkv):
            qw, kw = cache.ln_w[li]
            outs = []
            for s in range(0, Lmax, 16):
                chunk = qkv[:, s:s + 16]
                q = ops.kv_append_ragged(chunk, qw, kw, sin, cos, ks[li], vs[li], [s] * B)
                outs.append(ops.decode_attention_ragged(
                    q, ks[li], vs[li], [s + chunk.shape[1]] * B))
            return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)
    return attend


@torch.no_grad()
def prefill_ragged(model, prompts, cache: KVCache) -> torch.Tensor:
    """Start a batch of prompts of different lengths: ``prompts`` is a list of
    1-D int64 tensors (L_b >= 1 tokens, cropped to their last block_size).
    Right-padded with token 0 to the longest, the batch runs once from
    position 0; attention is causal, so the padding cannot reach a sequence's
    real tokens. Cache rows [L_b, Lmax) of sequence b then hold padding K/V:
    never read, since ``cache.lens[b] = L_b``, and overwritten by later
    appends. Returns each sequence's logits at its last real token (B, V)."""
    block = cache.block_size
    prompts = [p.reshape(-1)[-block:] for p in prompts]
    B = len(prompts)
    lens = [int(p.numel()) for p in prompts]
    if B != len(cache.lens) or min(lens, default=0) < 1:
        raise RuntimeError(f"prefill_ragged: {len(cache.lens)} non-empty prompts "
                           f"expected, got lengths {lens}")
    dev = model.wte.device
    Lmax = max(lens)
    idx = torch.zeros(B, Lmax, dtype=torch.int64)
    for b, p in enumerate(prompts):
        idx[b, :lens[b]] = p
    idx = idx.to(dev)
    cache.set_lens([0] * B)
    x, pending = _ragged_layers(model, idx,
                                _prefill_attend(model, cache, cache.k, cache.v, B, Lmax))
    last = torch.tensor(lens, device=dev) - 1
    rows = torch.arange(B, device=dev)
    x = x[rows, last][:, None]
    if pending is not None:
        pending = pending[rows, last][:, None]
    cache.set_lens(lens)
    return _ragged_logits(model, x, pending)


@torch.no_grad()
def decode_step_ragged(model, idx_new: torch.Tensor, cache: KVCache) -> torch.Tensor:
    """Run idx_new (B, Tn), Tn <= 16, with sequence b at positions
    cache.lens[b] .. cache.lens[b]+Tn-1, appending to the cache; returns the
    last position's logits (B, V).

    A sequence whose cache is full (lens[b] == block_size) is retired: its
    position stays frozen at the last Tn rows, which it goes on rewriting, its
    length does not advance and its logits mean nothing. That keeps the batch
    rectangular without a host decision per step. The device mirror of the
    lengths follows the same rule on the device: two small launches per step,
    no upload and no sync, however many layers read it."""
    B, Tn = idx_new.shape
    block = cache.block_size
    if not 1 <= Tn <= 16:
        raise RuntimeError(f"decode_step_ragged: 1 <= Tn <= 16 required, got {Tn}")
    if B != len(cache.lens):
        raise RuntimeError(f"decode_step_ragged: batch {B}, cache {len(cache.lens)}")
    for n in cache.lens:
        if n < block and n + Tn > block:
            raise RuntimeError(f"decode_step_ragged: positions [{n}, {n + Tn}) "
                               f"exceed block_size {block}")
    pos = [min(n, block - Tn) for n in cache.lens]
    kv_lens = [p + Tn for p in pos]
    pos_dev = cache.lens_dev.clamp(max=block - Tn)
    kv_lens_dev = pos_dev + Tn
    sin, cos = model.rope_sin, model.rope_cos

    def attend(li, qkv):
        qw, kw = cache.ln_w[li]
        q = ops.kv_append_ragged(qkv, qw, kw, sin, cos, cache.k[li], cache.v[li],
                                 pos, pos_dev)
        return ops.decode_attention_ragged(q, cache.k[li], cache.v[li], kv_lens,
                                           kv_lens_dev)

    x, pending = _ragged_layers(model, idx_new, attend)
    cache.lens = kv_lens
    cache.lens_dev = kv_lens_dev
    return _ragged_logits(model, x[:, -1:],
                          None if pending is None else pending[:, -1:])


@torch.no_grad()
def generate_ragged(model, prompts, max_new_tokens: int, temperature: float = 1.0,
                    top_k: int | None = None, eos_id: int | None = None,
                    generator: torch.Generator | None = None,
                    stop_check_every: int = 16, seed: int | None = None) -> list:
    """Decode a batch of prompts of different lengths together: ``prompts`` is
    a list of 1-D int64 tensors; returns, per prompt, the prompt plus what it
    generated, cut after its first ``eos_id`` if that is set.

    Limits. Every sequence takes one token per step. There is no sliding
    window: a prompt is cropped to its last block_size tokens, and a sequence
    emits at most min(max_new_tokens, block_size - L_b + 1) tokens (the last
    one is sampled and never fed), after which it is finished. The batch is
    not compacted: a finished sequence goes on stepping (retired, see
    ``decode_step_ragged``) until the loop ends, and its surplus tokens are
    dropped from the result. The loop ends when the longest budget is spent
    or, with ``eos_id``, when a check of the device-side done-mask (one sync
    every ``stop_check_every`` steps; a parameter, not a measured optimum)
    finds every sequence done.

    ``seed`` as in ``generate``: step t of the loop draws with
    ``ops.sample_tokens(..., seed=seed, step=t)``, row = index of the prompt.

    Native under ``native_decode(model)``; otherwise the same code runs on
    ``ops.ref_backend`` with fp32 caches."""
    _check_seed(seed, generator)
    model.eval()
    block = model.config.block_size
    dev = model.wte.device
    prompts = [p.reshape(-1) for p in prompts]
    B = len(prompts)
    if B == 0:
        return []
    cache = KVCache(model, B, dtype=None if native_decode(model) else torch.float32)
    lens = [min(int(p.numel()), block) for p in prompts]
    budget = [max(0, min(int(max_new_tokens), block - n + 1)) for n in lens]
    n_steps = max(budget)
    if n_steps == 0:
        return [p.clone() for p in prompts]
    logits = prefill_ragged(model, prompts, cache)
    toks = torch.zeros(B, n_steps, dtype=torch.int64, device=dev)
    budget_dev = torch.tensor(budget, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    for t in range(n_steps):
        nxt = _next_token(logits, temperature, top_k, generator, seed, t)
        toks[:, t] = nxt
        if t + 1 == n_steps:
            break
        if eos_id is not None:
            done |= (nxt == eos_id) | (budget_dev <= t + 1)
            if (t + 1) % stop_check_every == 0 and bool(done.all()):
                break
        logits = decode_step_ragged(model, nxt[:, None], cache)
    toks = toks.cpu()
    out = []
    for b, p in enumerate(prompts):
        new = toks[b, :budget[b]]
        if eos_id is not None:
            hit = (new == eos_id).nonzero()
            if hit.numel():
                new = new[:int(hit[0]) + 1]
        out.append(torch.cat([p, new.to(p.device)]))
    return out


@torch.no_grad()
def decode_step_slots(model, idx_new: torch.Tensor, cache: KVCache, slots,
                      slots_dev=None) -> torch.Tensor:
    """``decode_step_ragged`` for the rows named by ``slots`` in a pool
    ``cache`` of S >= B slots: idx_new (B, Tn), Tn <= 16, with row b at
    positions cache.lens[slots[b]] .. +Tn-1 of slot slots[b]; returns the last
    position's logits (B, V). ``slots`` is B distinct host integers;
    ``slots_dev`` their int32 device copy (uploaded here when absent).

    The per-slot lengths ``cache.lens`` / ``cache.lens_dev`` are indexed by
    slot and advance for the named slots only, by the retire-when-full rule of
    ``decode_step_ragged``, on the device without upload or sync (a gather, a
    clamp, an add and a scatter per step, however many layers read them)."""
    B, Tn = idx_new.shape
    block = cache.block_size
    slots = [int(s) for s in slots]
    S = len(cache.lens)
    if not 1 <= Tn <= 16:
        raise RuntimeError(f"decode_step_slots: 1 <= Tn <= 16 required, got {Tn}")
    if len(slots) != B or len(set(slots)) != B or not all(0 <= s < S for s in slots):
        raise RuntimeError(f"decode_step_slots: {B} distinct slots in [0, {S}) "
                           f"expected, got {slots}")
    lens = [cache.lens[s] for s in slots]
    for n in lens:
        if n < block and n + Tn > block:
            raise RuntimeError(f"decode_step_slots: positions [{n}, {n + Tn}) "
                               f"exceed block_size {block}")
    if slots_dev is None:
        slots_dev = torch.tensor(slots, dtype=torch.int32, device=cache.lens_dev.device)
    pos = [min(n, block - Tn) for n in lens]
    kv_lens = [p + Tn for p in pos]
    pos_dev = cache.lens_dev[slots_dev].clamp(max=block - Tn)
    kv_lens_dev = pos_dev + Tn
    sin, cos = model.rope_sin, model.rope_cos

    def attend(li, qkv):
        qw, kw = cache.ln_w[li]
        q = ops.kv_append_slots(qkv, qw, kw, sin, cos, cache.k[li], cache.v[li],
                                pos, slots, pos_dev, slots_dev)
        return ops.decode_attention_slots(q, cache.k[li], cache.v[li], kv_lens, slots,
                                          kv_lens_dev, slots_dev)

    x, pending = _ragged_layers(model, idx_new, attend)
    for s, n in zip(slots, kv_lens):
        cache.lens[s] = n
    cache.lens_dev[slots_dev] = kv_lens_dev
    return _ragged_logits(model, x[:, -1:],
                          None if pending is None else pending[:, -1:])


class PagedKVCache:
    """K/V of every layer in ``num_pages`` pages of ``page_size`` positions,
    shared by ``num_seats`` sequences: one buffer (n_layer, 2, num_pages, H,
    page_size, C) with per-layer pool views ``k[l]`` / ``v[l]`` of shape
    (num_pages, H, page_size, C). Position p of the sequence in seat s lives at
    row p % page_size of page ``table[s][p // page_size]``.

    Kept on the host, per seat: the page list ``pages[s]``, the length
    ``lens[s]`` and the capacity ``cap[s]`` = pages * page_size (at most
    block_size), with the (num_seats, MP) block table ``table`` (int32, -1
    where no page is assigned; MP = block_size / page_size). ``alloc`` hands
    out the lowest free page numbers first, so a run is deterministic;
    ``free`` returns a seat's pages. Both change the host side only:
    ``upload`` (or a caller that folds ``host_state()`` into an upload of its
    own and calls ``set_dev``) refreshes the int32 device mirrors
    ``table_dev``, ``lens_dev`` and ``cap_dev`` that the kernels and
    ``decode_step_paged`` read. Rows at and past a length, and free pages,
    hold stale or uninitialised data and are never read."""

    def __init__(self, model, num_seats: int, num_pages: int, page_size: int = 16,
                 device=None, dtype=None):
        cfg = model.config
        page_size = int(page_size)
        if not 16 <= page_size <= 128 or page_size & (page_size - 1):
            raise ValueError("PagedKVCache: page_size must be a power of two in "
                             f"[16, 128], got {page_size}")
        if cfg.block_size % page_size:
            raise ValueError(f"PagedKVCache: page_size {page_size} does not divide "
                             f"block_size {cfg.block_size}")
        if num_seats < 1 or num_pages < 1:
            raise ValueError("PagedKVCache: num_seats >= 1 and num_pages >= 1 required")
        device = model.wte.device if device is None else device
        dtype = model.wte.dtype if dtype is None else dtype
        self.block_size = cfg.block_size
        self.page_size = page_size
        self.num_pages = int(num_pages)
        self.max_pages = cfg.block_size // page_size       # MP
        self.buf = torch.empty(cfg.n_layer, 2, num_pages, cfg.n_head, page_size,
                               cfg.head_dim, device=device, dtype=dtype)
        self.k = [self.buf[li, 0] for li in range(cfg.n_layer)]
        self.v = [self.buf[li, 1] for li in range(cfg.n_layer)]
        # the kernels take fp32 LN weights: convert once, not per token
        self.ln_w = [(blk.attn.q_ln_weight.detach().float(),
                      blk.attn.k_ln_weight.detach().float())
                     for blk in model.blocks]
        self.free_pages = list(range(num_pages))            # kept sorted
        self.pages = [[] for _ in range(num_seats)]
        self.lens = [0] * num_seats
        self.cap = [0] * num_seats
        self.table = torch.full((num_seats, self.max_pages), -1, dtype=torch.int32)
        self.upload()

    def pages_for(self, n_positions: int) -> int:
        return -(-int(n_positions) // self.page_size)

    def alloc(self, seat: int, n_positions: int) -> list:
        """Give the (empty) seat the pages for ``n_positions`` positions, lowest
        page numbers first; returns them. Host side only."""
        n = self.pages_for(n_positions)
        if self.pages[seat]:
            raise RuntimeError(f"PagedKVCache.alloc: seat {seat} already holds pages")
        if not 1 <= n <= self.max_pages:
            raise RuntimeError(f"PagedKVCache.alloc: {n_positions} positions need {n} "
                               f"pages, 1..{self.max_pages} allowed")
        if n > len(self.free_pages):
            raise RuntimeError(f"PagedKVCache.alloc: {n} pages wanted, "
                               f"{len(self.free_pages)} free")
        got, self.free_pages = self.free_pages[:n], self.free_pages[n:]
        self.pages[seat] = got
        self.cap[seat] = n * self.page_size
        self.lens[seat] = 0
        self.table[seat, :n] = torch.tensor(got, dtype=torch.int32)
        return got

    def free(self, seat: int):
        """Return the seat's pages to the free list. Host side only."""
        self.free_pages = sorted(self.free_pages + self.pages[seat])
        self.pages[seat] = []
        self.cap[seat] = self.lens[seat] = 0
        self.table[seat] = -1

    def host_state(self) -> torch.Tensor:
        """lens | cap | table as one int32 vector, the layout of ``set_dev``."""
        return torch.cat([torch.tensor(self.lens + self.cap, dtype=torch.int32),
                          self.table.reshape(-1)])

    def set_dev(self, state_dev: torch.Tensor):
        """Take the device copy of ``host_state()`` as the mirrors."""
        S = len(self.lens)
        self.lens_dev = state_dev[:S]
        self.cap_dev = state_dev[S:2 * S]
        self.table_dev = state_dev[2 * S:2 * S + S * self.max_pages].view(S, self.max_pages)

    def upload(self):
        self.set_dev(self.host_state().to(self.buf.device))


@torch.no_grad()
def decode_step_paged(model, idx_new: torch.Tensor, cache: PagedKVCache, seats,
                      seats_dev=None) -> torch.Tensor:
    """``decode_step_slots`` on a ``PagedKVCache``: idx_new (B, Tn), Tn <= 16,
    with row b at positions cache.lens[seats[b]] .. +Tn-1 of the pages of seat
    seats[b]; returns the last position's logits (B, V). ``seats`` is B
    distinct host integers, ``seats_dev`` their int32 device copy (uploaded
    here when absent). The device mirrors of the cache must be current
    (``cache.upload``).

    The (B, MP) table rows of the step are gathered from the seat-indexed
    mirror once, not once per layer. Lengths advance, on the host and on the
    device, by the retire-when-full rule of ``decode_step_ragged`` with the
    seat's capacity where that has block_size: a row that is full goes on
    rewriting the last Tn rows of its own last page and never writes outside
    its pages."""
    B, Tn = idx_new.shape
    seats = [int(s) for s in seats]
    S = len(cache.lens)
    if not 1 <= Tn <= 16:
        raise RuntimeError(f"decode_step_paged: 1 <= Tn <= 16 required, got {Tn}")
    if len(seats) != B or len(set(seats)) != B or not all(0 <= s < S for s in seats):
        raise RuntimeError(f"decode_step_paged: {B} distinct seats in [0, {S}) "
                           f"expected, got {seats}")
    lens = [cache.lens[s] for s in seats]
    caps = [cache.cap[s] for s in seats]
    for n, cap in zip(lens, caps):
        if cap < Tn or (n < cap and n + Tn > cap):
            raise RuntimeError(f"decode_step_paged: positions [{n}, {n + Tn}) exceed "
                               f"the seat's {cap}")
    if seats_dev is None:
        seats_dev = torch.tensor(seats, dtype=torch.int32, device=cache.lens_dev.device)
    pos = [min(n, cap - Tn) for n, cap in zip(lens, caps)]
    kv_lens = [p + Tn for p in pos]
    pos_dev = torch.minimum(cache.lens_dev[seats_dev], cache.cap_dev[seats_dev] - Tn)
    kv_lens_dev = pos_dev + Tn
    table = cache.table[seats]
    table_dev = cache.table_dev[seats_dev]
    sin, cos = model.rope_sin, model.rope_cos

    def attend(li, qkv):
        qw, kw = cache.ln_w[li]
        q = ops.kv_append_paged(qkv, qw, kw, sin, cos, cache.k[li], cache.v[li],
                                pos, table, pos_dev, table_dev)
        return ops.decode_attention_paged(q, cache.k[li], cache.v[li], kv_lens, table,
                                          kv_lens_dev, table_dev)

    x, pending = _ragged_layers(model, idx_new, attend)
    for s, n in zip(seats, kv_lens):
        cache.lens[s] = n
    cache.lens_dev[seats_dev] = kv_lens_dev
    return _ragged_logits(model, x[:, -1:],
                          None if pending is None else pending[:, -1:])


def _prefill_paged(model, cache: PagedKVCache, idx, seat):
    """Run one prompt idx (1, L) from position 0 into the pages of ``seat``
    (already allocated) on the paths ``_attend_cached`` takes for a contiguous
    cache: the flash prefill for L > 16 where the padded prompt fits
    block_size, 16-row chunks on the paged pair otherwise. The seat's table row
    and the chunk positions go to the device once, not once per layer.
    Returns (x, pending) of ``_ragged_layers``."""
    L = idx.shape[1]
    dev = cache.buf.device
    sin, cos = model.rope_sin, model.rope_cos
    table = cache.table[seat:seat + 1]
    table_dev = table.to(dev)
    fits = not idx.is_cuda or -(-L // 128) * 128 <= cache.block_size
    starts = list(range(0, L, 16))
    ends = [min(s + 16, L) for s in starts]
    # ref_backend on the GPU (fp32 pools) takes the chunks, as _prefill_attend does
    chunked = not (L > 16 and fits) or (cache.buf.is_cuda and not _native_cache(cache))
    if chunked:
        marks = torch.tensor(starts + ends, dtype=torch.int32).to(dev)

    def attend(li, qkv):
        qw, kw = cache.ln_w[li]
        if not chunked:
            return ops.prefill_attention_paged(qkv, qw, kw, sin, cos, cache.k[li],
                                               cache.v[li], table, table_dev)
        outs = []
        for i, (s, e) in enumerate(zip(starts, ends)):
            q = ops.kv_append_paged(qkv[:, s:e], qw, kw, sin, cos, cache.k[li], cache.v[li],
                                    [s], table, marks[i:i + 1], table_dev)
            outs.append(ops.decode_attention_paged(
                q, cache.k[li], cache.v[li], [e], table,
                marks[len(starts) + i:len(starts) + i + 1], table_dev))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)

    return _ragged_layers(model, idx, attend)


class Request:
    """Handle of one ``DecodeScheduler.submit``: ``done`` once the request has
    left the scheduler, and then ``tokens`` = the prompt plus what it
    generated (1-D int64, on the prompt's device)."""

    def __init__(self, prompt, budget, temperature, top_k, seed, row, eos_id):
        self.prompt = prompt
        self.budget = budget
        self.temperature = float(temperature)
        self.top_k = top_k
        self.seed = seed
        self.row = int(row)
        self.eos_id = eos_id
        self.done = False
        self.tokens = None
        self._new = []        # generated tokens the host has seen
        self._drawn = 0       # tokens sampled on the device so far
        self._slot = None

    def _finish(self):
        new = torch.tensor(self._new, dtype=torch.int64)
        self.tokens = torch.cat([self.prompt, new.to(self.prompt.device)])
        self.done = True


class DecodeScheduler:
    """Continuous batching over a pool of ``num_slots`` full-length caches:
    requests are queued by ``submit``, admitted into free slots, decoded
    together one token per ``step`` and retired as they finish, while the
    others go on. Synchronous, no threads: the caller drives ``step`` (or
    ``run``).

    Every ``tick_every`` steps (and at once when nothing is active and the
    queue is not empty, or when every active row has spent its budget) a step
    ends with a tick: one device-to-host copy of the tokens drawn since the
    last one; rows that hit their ``eos_id`` or spent their budget are retired,
    their surplus tokens dropped as in ``generate_ragged``, and their slots
    freed; queued requests are admitted into free slots in FIFO order, each
    prompt prefilled alone at B=1 into its slot and its first token drawn at
    step 0 with its own parameters; then the slot map, the per-slot lengths
    and the per-row sampling parameters go to the device in one upload.
    Between ticks the active set is fixed, finished rows keep stepping (as
    retired rows do in ``decode_step_ragged``), nothing is uploaded and nothing
    syncs. ``tick_every`` is a parameter, not a measured optimum: a small value
    frees slots sooner, a large one syncs less often.

    Token t of a request is drawn by ``ops.sample_tokens_rows`` with the
    request's own (seed, step=t, row), whatever else shares the step: a
    request with (seed=s, row=r) reproduces row r of ``generate(..., seed=s)``
    wherever the logits agree. temperature <= 0 is greedy.

    With ``num_pages`` the cache is a ``PagedKVCache`` of that many pages of
    ``page_size`` positions, ``num_slots`` is the number of seats (the largest
    batch) and a step runs ``decode_step_paged``. A request holds the pages of
    the positions it can ever write, ceil(min(L + budget - 1, block_size) /
    page_size) of them, allocated at admission (lowest free page first) and
    freed at retirement, so the table only changes at a tick and travels in
    the tick's upload (an admitted request's own table row goes up once more,
    ahead of it, for its prefill). Admission stays strictly FIFO: the head of
    the queue is admitted when a seat is free and its pages are; while it does
    not fit it waits and nothing overtakes it. ``submit`` raises for a request
    that needs more pages than the pool has. A request's tokens do not depend
    on ``num_pages``, on ``page_size`` or on which pages it got: the paged
    kernels have the bits of the slotted ones. ``page_size`` = 16 is a
    parameter, not a measured optimum. Out of scope: page growth on demand,
    preemption, prefix sharing, and paging for ``generate`` and
    ``generate_ragged``.

    Limits: without ``num_pages`` no paging (a slot is a whole block_size
    cache); no sliding window (budget = min(max_new_tokens, block_size - L +
    1) as in ``generate_ragged``); admitted prompts are prefilled one at a
    time, not as a batch, and a prefill is not interleaved with decode steps.

    Native under ``native_decode(model)``; otherwise the same code runs on
    ``ops.ref_backend`` with fp32 caches."""

    def __init__(self, model, num_slots: int, tick_every: int = 8, *,
                 num_pages: int | None = None, page_size: int = 16):
        if num_slots < 1 or tick_every < 1:
            raise ValueError("DecodeScheduler: num_slots >= 1 and tick_every >= 1 required")
        model.eval()
        self.model = model
        self.tick_every = int(tick_every)
        dtype = None if native_decode(model) else torch.float32
        self.paged = num_pages is not None
        if self.paged:
            self.cache = PagedKVCache(model, num_slots, num_pages, page_size, dtype=dtype)
        else:
            self.cache = KVCache(model, num_slots, dtype=dtype)
        self.queue = collections.deque()
        self.free = list(range(num_slots))
        self.active = []          # requests, in batch-row order
        self._finished = []       # retired since the last step() returned
        self._since_tick = 0
        self._nxt = None          # (B,) last token of every active row, on the device
        self._cols = []           # (B,) token columns since the last tick
        self._fresh = []          # per active row: column 0 has not been read yet
        self._slots_dev = self._params_dev = None

    def submit(self, prompt, max_new_tokens: int, temperature: float = 1.0,
               top_k: int | None = None, seed: int | None = None, row: int = 0,
               eos_id: int | None = None) -> Request:
        """Queue a request; returns its handle. The prompt (1-D int64, at least
        one token) conditions on its last block_size tokens. Without ``seed``
        one is drawn by ``ops.draw_sample_seed``."""
        block = self.cache.block_size
        prompt = prompt.reshape(-1)
        if prompt.numel() < 1:
            raise RuntimeError("DecodeScheduler.submit: empty prompt")
        L = min(int(prompt.numel()), block)
        budget = max(0, min(int(max_new_tokens), block - L + 1))
        if seed is None:
            seed = ops.draw_sample_seed()
        req = Request(prompt, budget, temperature, top_k, seed, row, eos_id)
        # validates the sampling parameters now, not at admission
        ops.sample_row_params(req.temperature, top_k, [seed], [0], [req.row], 1)
        if self.paged and budget > 0:
            # the positions it can ever write: the last token is never fed
            req._positions = min(L + budget - 1, block)
            need = self.cache.pages_for(req._positions)
            if need > self.cache.num_pages:
                raise RuntimeError(f"DecodeScheduler.submit: the request needs {need} "
                                   f"pages, the pool has {self.cache.num_pages}")
        if budget == 0:
            req._finish()
            self._finished.append(req)
        else:
            self.queue.append(req)
        return req

    def pending(self) -> bool:
        """Whether a request is queued or active."""
        return bool(self.queue or self.active)

    @torch.no_grad()
    def step(self) -> list:
        """One decode step for the active rows, with a tick where one is due;
        returns the handles that finished."""
        if not self.active and self.queue:
            self._tick()
        if self.active:
            slots = [r._slot for r in self.active]
            step = decode_step_paged if self.paged else decode_step_slots
            logits = step(self.model, self._nxt[:, None], self.cache, slots, self._slots_dev)
            self._draw(logits)
            self._since_tick += 1
            if self._since_tick >= self.tick_every or \
                    all(r._drawn >= r.budget for r in self.active):
                self._tick()
        done, self._finished = self._finished, []
        return done

    def run(self) -> list:
        """Step until queue and pool are empty; returns the finished handles."""
        done = []
        while True:
            done += self.step()
            if not self.pending():
                return done

    def _draw(self, logits):
        act = self.active
        self._nxt = ops.sample_tokens_rows(
            logits, [r.temperature for r in act], [r.top_k for r in act],
            seeds=[r.seed for r in act], steps=[r._drawn for r in act],
            rows=[r.row for r in act], params_dev=self._params_dev)
        self._cols.append(self._nxt)
        self._params_dev[:, 2] += 1   # the step column, as on the host
        for r in act:
            r._drawn += 1

    def _admit(self, req, slot):
        """Prefill the prompt alone into its slot; its first token, on the
        device, drawn at step 0 with its own parameters."""
        model, cache = self.model, self.cache
        idx = req.prompt[-cache.block_size:][None].to(model.wte.device)
        L = idx.shape[1]
        if self.paged:
            cache.alloc(slot, req._positions)
            x, pending = _prefill_paged(model, cache, idx, slot)
        else:
            ks = [k[slot:slot + 1] for k in cache.k]
            vs = [v[slot:slot + 1] for v in cache.v]
            x, pending = _ragged_layers(model, idx,
                                        _prefill_attend(model, cache, ks, vs, 1, L))
        logits = _ragged_logits(model, x[:, -1:],
                                None if pending is None else pending[:, -1:])
        req._slot = slot
        req._drawn = 1
        cache.lens[slot] = L
        return ops.sample_tokens_rows(logits, req.temperature, [req.top_k],
                                      seeds=[req.seed], steps=[0], rows=[req.row])

    def _tick(self):
        dev = self.model.wte.device
        keep = []                 # index into the old rows of those that stay
        if self.active:
            toks = torch.stack(self._cols, dim=1).cpu()   # the one copy of a tick
            for b, req in enumerate(self.active):
                for tok in toks[b, 0 if self._fresh[b] else 1:].tolist():
                    if len(req._new) == req.budget:
                        break
                    req._new.append(tok)
                    if tok == req.eos_id:
                        break
                if len(req._new) == req.budget or req._new[-1:] == [req.eos_id]:
                    req._finish()
                    self.free.append(req._slot)
                    if self.paged:
                        self.cache.free(req._slot)
                    self._finished.append(req)
                else:
                    keep.append(b)
        stay = [self.active[b] for b in keep]
        firsts = []
        self.free.sort()
        while self.queue and self.free:
            if self.paged and self.cache.pages_for(self.queue[0]._positions) > \
                    len(self.cache.free_pages):
                break             # the head waits for pages; nothing overtakes it
            req = self.queue.popleft()
            firsts.append(self._admit(req, self.free.pop(0)))
            stay.append(req)
        n_old = len(self.active)
        self._fresh = [False] * len(keep) + [True] * len(firsts)
        self.active = stay
        self._since_tick = 0
        if not stay:
            self._nxt, self._cols = None, []
            return
        # one upload: per-slot lengths | slot map | rows kept | sampling parameters
        # (paged: | per-seat lengths, capacities and block table, at the end)
        S, B = len(self.cache.lens), len(stay)
        host = ops.sample_row_params(
            [r.temperature for r in stay], [r.top_k for r in stay], [r.seed for r in stay],
            [r._drawn for r in stay], [r.row for r in stay], B)
        meta = torch.tensor(self.cache.lens + [r._slot for r in stay]
                            + keep + list(range(n_old, n_old + len(firsts))),
                            dtype=torch.int32)
        parts = [meta, ops.pack_sample_params(*host).reshape(-1)]
        if self.paged:
            parts.append(self.cache.host_state())
        buf = torch.cat(parts).to(dev)
        if self.paged:
            n_state = parts[2].numel()
            self.cache.set_dev(buf[-n_state:])
            buf = buf[:-n_state]
        self.cache.lens_dev = buf[:S]
        self._slots_dev = buf[S:S + B]
        self._params_dev = buf[S + 2 * B:].view(B, 6)
        src = torch.cat(([self._nxt] if n_old else []) + firsts)
        self._nxt = src[buf[S + B:S + 2 * B]]
        self._cols = [self._nxt]


@torch.no_grad()
def generate_continuous(model, prompts, max_new_tokens: int, temperature: float = 1.0,
                        top_k: int | None = None, eos_id: int | None = None,
                        num_slots: int = 8, tick_every: int = 8,
                        seed: int | None = None, num_pages: int | None = None,
                        page_size: int = 16) -> list:
    """``generate_ragged`` on a ``DecodeScheduler`` of ``num_slots`` slots:
    every prompt is submitted (prompt i with ``row=i`` and the one ``seed``,
    drawn when None), the scheduler runs until all are done, and the results
    come back in order. There may be more prompts than slots: the rest wait
    for a slot. With a seed, prompt i gets the tokens row i of
    ``generate(..., seed=seed)`` gets wherever the logits agree. With
    ``num_pages`` the scheduler's cache is paged (``num_slots`` seats over
    ``num_pages`` pages of ``page_size`` positions); the tokens are the same."""
    if seed is None:
        seed = ops.draw_sample_seed()
    sched = DecodeScheduler(model, num_slots, tick_every, num_pages=num_pages,
                            page_size=page_size)
    handles = [sched.submit(p, max_new_tokens, temperature, top_k, seed=seed, row=i,
                            eos_id=eos_id) for i, p in enumerate(prompts)]
    sched.run()
    return [h.tokens for h in handles]


def _check_seed(seed, generator):
    if seed is not None and generator is not None:
        raise ValueError("pass seed= (counter-based sampling) or generator= "
                         "(torch.multinomial), not both")


def _next_token(logits, temperature, top_k, generator, seed, t):
    """Token t of a call: seeded sampling where a seed is given, ``_sample``
    otherwise; greedy (temperature <= 0) is argmax either way."""
    if seed is None or temperature <= 0:
        return _sample(logits, temperature, top_k, generator)
    return ops.sample_tokens(logits, temperature, top_k, seed=seed, step=t)


def _sample(logits, temperature, top_k, generator):
    if temperature <= 0:
        return logits.argmax(dim=-1)
    lf = logits.float() / temperature
    if top_k is not None:
        kth = torch.topk(lf, top_k, dim=-1).values[:, -1:]
        lf = lf.masked_fill(lf < kth, float("-inf"))
    p = torch.softmax(lf, dim=-1)
    return torch.multinomial(p.cpu() if generator is not None and
                             generator.device.type == "cpu" and p.is_cuda else p,
                             1, generator=generator).squeeze(-1).to(logits.device)
