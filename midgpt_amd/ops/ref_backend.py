"""The extension's interface in fp32 torch: one plain function (no autograd)
per entry point in ``ops.BACKEND_API``, ``ops.RAGGED_API``,
``ops.SAMPLING_API``, ``ops.SLOT_API``, ``ops.PAGED_API`` and
``ops.TRANSPOSE_API``, taking the same positional arguments
as the ``_C`` binding of that name and returning as many results with the
same shapes and dtypes. ``ops._backend`` hands out this module wherever the
HIP extension does not run: on the CPU and under ``MIDGPT_FORCE_REF=1``.

Written apart from ``ops/reference.py`` on purpose: that module is the
oracle of the tests, this one the code under test (hand-derived backward
passes included). Only its RoPE / LayerNorm / keep-mask helpers are shared.
"""
from __future__ import annotations

import math

import torch

from midgpt_amd.ops import reference as ref


# RMSNorm over (N, D) rows
def rmsnorm_fwd(x2d, weight, eps):
    xf = x2d.float()
    invrms = torch.rsqrt(xf.pow(2).mean(dim=-1) + eps)
    y = xf * invrms[:, None]
    if weight is not None:
        y = y * weight.float()
    return y.to(x2d.dtype), invrms


def rmsnorm_bwd(dy2d, x2d, weight, invrms, eps):
    xf = x2d.float()
    dyf = dy2d.float()
    g = dyf * weight.float() if weight is not None else dyf
    # y = x * r, r = (mean(x^2)+eps)^-1/2
    # dx = r*g - x * r^3 * mean(x*g)
    r = invrms[:, None]
    mean_xg = (xf * g).mean(dim=-1, keepdim=True)
    dx = (r * g - xf * r.pow(3) * mean_xg).to(x2d.dtype)
    dw = (dyf * xf * r).sum(dim=0).to(weight.dtype) if weight is not None else None
    return dx, dw


# QK-LayerNorm + RoPE over the packed projection (B, T, 3, H, C)
def _ln_fwd_stats(x, w, eps):
    """LayerNorm fwd returning (y, stats) with stats = (mean, invstd) fp32
    stacked on last dim -> shape (*x.shape[:-1], 2)."""
    xf = x.float()
    mu = xf.mean(dim=-1, keepdim=True)
    var = xf.var(dim=-1, unbiased=False, keepdim=True)
    invstd = torch.rsqrt(var + eps)
    y = ((xf - mu) * invstd * w.float()).to(x.dtype)
    stats = torch.cat([mu, invstd], dim=-1)  # (..., 2)
    return y, stats


def _ln_bwd(dyf, x, w, stats):
    """LayerNorm bwd (no bias). dyf fp32, x input tensor, stats (...,2)."""
    xf = x.float()
    mu = stats[..., 0:1]
    invstd = stats[..., 1:2]
    xhat = (xf - mu) * invstd
    g = dyf * w.float()
    mean_g = g.mean(dim=-1, keepdim=True)
    mean_gx = (g * xhat).mean(dim=-1, keepdim=True)
    dx = invstd * (g - mean_g - xhat * mean_gx)
    dw = (dyf * xhat).sum(dim=tuple(range(dyf.dim() - 1))).to(w.dtype)
    return dx, dw


def qkv_prep_fwd(qkv, qw, kw, sin, cos, eps):
    qr = qkv[:, :, 0].permute(0, 2, 1, 3)  # (B,H,T,C)
    kr = qkv[:, :, 1].permute(0, 2, 1, 3)
    v = qkv[:, :, 2].permute(0, 2, 1, 3).contiguous()
    qn, qstats = _ln_fwd_stats(qr, qw, eps)
    kn, kstats = _ln_fwd_stats(kr, kw, eps)
    q = ref.apply_rope(qn, sin, cos).contiguous()
    k = ref.apply_rope(kn, sin, cos).contiguous()
    return q, k, v, qstats, kstats


def qkv_prep_bwd(dq, dk, dv, qkv, qw, kw, sin, cos, qstats, kstats, eps):
    # rope(x) = x*cos + rot(x)*sin with rot = rotate_every_two.
    # d/dx: dx = dy*cos + rot^T(dy*sin); rot^T = inverse rotation
    # rot([a,b]) = [-b, a]  =>  rot^T([a,b]) = [b, -a] = -rot
    sin2 = torch.repeat_interleave(sin, 2, dim=-1)
    cos2 = torch.repeat_interleave(cos, 2, dim=-1)
    dqn = (dq.float() * cos2 - ref.rotate_every_two(dq.float() * sin2))
    dkn = (dk.float() * cos2 - ref.rotate_every_two(dk.float() * sin2))
    qr = qkv[:, :, 0].permute(0, 2, 1, 3)
    kr = qkv[:, :, 1].permute(0, 2, 1, 3)
    dqr, dqw = _ln_bwd(dqn, qr, qw, qstats)
    dkr, dkw = _ln_bwd(dkn, kr, kw, kstats)
    dqkv = torch.empty_like(qkv)
    dqkv[:, :, 0] = dqr.permute(0, 2, 1, 3).to(qkv.dtype)
    dqkv[:, :, 1] = dkr.permute(0, 2, 1, 3).to(qkv.dtype)
    dqkv[:, :, 2] = dv.permute(0, 2, 1, 3).to(qkv.dtype)
    return dqkv, dqw, dkw


# Causal attention, (B,H,T,C) throughout. Dropout applies the bit-exact host
# mirror of the kernels' keep-mask, so one seed gives one mask on either
# backend. LSE is that of the undropped softmax.
def _cpu_dropout_scale(seed, B, H, T, p, like):
    """Z = keep/(1-p) from the host mirror of the kernels' keep-mask."""
    keep = ref.attn_dropout_keep(seed, B, H, T, p)
    return keep.to(device=like.device, dtype=like.dtype) / (1.0 - p)


def attn_fwd_dropout(q, k, v, dropout_p, seed):
    B, H, T, C = q.shape
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) / math.sqrt(C)
    mask = torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
    s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)  # (B,H,T) fp32
    a = torch.exp(s - lse[..., None])
    if dropout_p > 0.0:
        a = a * _cpu_dropout_scale(seed, B, H, T, dropout_p, a)
    o = torch.matmul(a.to(v.dtype), v)
    return o, lse


def attn_bwd_dropout(do, q, k, v, o, lse, dropout_p, seed):
    B, H, T, C = q.shape
    scale = 1.0 / math.sqrt(C)
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    mask = torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
    s = s.masked_fill(~mask, float("-inf"))
    p = torch.exp(s - lse[..., None])          # undropped P (B,H,T,T) fp32
    dof = do.float()
    dp = torch.matmul(dof, v.float().transpose(-1, -2))
    if dropout_p > 0.0:
        z = _cpu_dropout_scale(seed, B, H, T, dropout_p, p)
        dv = torch.matmul((p * z).transpose(-1, -2), dof)
        dp = dp * z
    else:
        dv = torch.matmul(p.transpose(-1, -2), dof)
    # rowsum(dO*O) = sum_j P_ij dP_ij also holds for the dropped O
    delta = (dof * o.float()).sum(dim=-1, keepdim=True)
    ds = p * (dp - delta)
    dq = torch.matmul(ds, k.float()) * scale
    dk = torch.matmul(ds.transpose(-1, -2), q.float()) * scale
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


def attn_fwd(q, k, v):
    return attn_fwd_dropout(q, k, v, 0.0, 0)


def attn_bwd(do, q, k, v, o, lse):
    return attn_bwd_dropout(do, q, k, v, o, lse, 0.0, 0)


# KV-cache decode. Caches are (B,H,Tmax,C), written in place.
def kv_append(qkv, qw, kw, sin, cos, k_cache, v_cache, pos, eps):
    Tn = qkv.shape[1]
    s, c = sin[pos:pos + Tn], cos[pos:pos + Tn]
    q = ref.qk_layernorm(qkv[:, :, 0].permute(0, 2, 1, 3), qw, eps)
    k = ref.qk_layernorm(qkv[:, :, 1].permute(0, 2, 1, 3), kw, eps)
    k_cache[:, :, pos:pos + Tn] = ref.apply_rope(k, s, c)
    v_cache[:, :, pos:pos + Tn] = qkv[:, :, 2].permute(0, 2, 1, 3)
    return ref.apply_rope(q, s, c).contiguous()


def _decode_attention_ref(q, k_cache, v_cache, kv_len):
    """End-aligned causal attention in fp32: row i of Tq sees keys
    [0, kv_len - Tq + i]. Any Tq. -> (B,Tq,H,C) in q's dtype."""
    B, H, Tq, C = q.shape
    k = k_cache[:, :, :kv_len].float()
    v = v_cache[:, :, :kv_len].float()
    s = torch.matmul(q.float(), k.transpose(-1, -2)) / math.sqrt(C)
    qpos = torch.arange(kv_len - Tq, kv_len, device=q.device)[:, None]
    kpos = torch.arange(kv_len, device=q.device)[None, :]
    s = s.masked_fill(kpos > qpos, float("-inf"))
    o = torch.matmul(torch.softmax(s, dim=-1), v).to(q.dtype)
    return o.transpose(1, 2).contiguous()


def attn_decode(q, k_cache, v_cache, kv_len, num_splits):
    """The binding's argument checks, then the math (num_splits only cuts
    the kernel's grid: nothing to do with it here)."""
    Tq = q.shape[2]
    if kv_len > k_cache.shape[2]:
        raise RuntimeError(f"decode_attention: kv_len {kv_len} exceeds the cache "
                           f"({k_cache.shape[2]})")
    if not 1 <= Tq <= min(16, kv_len):
        raise RuntimeError("decode_attention: 1 <= Tq <= min(16, kv_len) required "
                           f"(Tq {Tq}, kv_len {kv_len})")
    if not 0 <= num_splits <= 64:
        raise RuntimeError("decode_attention: num_splits must be in [0, 64]")
    return _decode_attention_ref(q, k_cache, v_cache, kv_len)


# Ragged decode (ops.RAGGED_API): sequence b at its own position / length.
# pos_host / kv_lens_host are the (B,) CPU integer tensors the bindings
# validate; the device copies are what the kernels read and are unused here.
def _host_lens(t, B, who):
    if t.is_cuda or t.dim() != 1 or t.shape[0] != B or t.dtype.is_floating_point:
        raise RuntimeError(f"{who}: the host copy must be a CPU integer tensor "
                           f"of {B} values")
    return [int(x) for x in t.tolist()]


def kv_append_ragged(qkv, qw, kw, sin, cos, k_cache, v_cache, pos_dev, pos_host, eps):
    B, Tn = qkv.shape[:2]
    pos = _host_lens(pos_host, B, "kv_append_ragged")
    Tmax = k_cache.shape[2]
    for p in pos:  # all of them before the first write, as the binding does
        if p < 0 or p + Tn > Tmax:
            raise RuntimeError(f"kv_append: rows [{p}, {p + Tn}) do not fit a "
                               f"cache of {Tmax} rows")
        if sin.shape[0] < p + Tn or cos.shape[0] < p + Tn:
            raise RuntimeError(f"kv_append: sin/cos tables have {sin.shape[0]} rows, "
                               f"position {p + Tn - 1} needed")
    return torch.cat([kv_append(qkv[b:b + 1], qw, kw, sin, cos, k_cache[b:b + 1],
                                v_cache[b:b + 1], pos[b], eps)
                      for b in range(B)], dim=0)


def attn_decode_ragged(q, k_cache, v_cache, kv_lens_dev, kv_lens_host, num_splits):
    B = q.shape[0]
    lens = _host_lens(kv_lens_host, B, "attn_decode_ragged")
    return torch.cat([attn_decode(q[b:b + 1], k_cache[b:b + 1], v_cache[b:b + 1],
                                  lens[b], num_splits)
                      for b in range(B)], dim=0)


# Slotted decode (ops.SLOT_API): batch row b lives in cache slot slots[b] of a
# pool (S,H,Tmax,C), S >= B. The ragged op on the one-slot view of each row,
# so row b has the bits of the ragged call on the gathered cache[slots].
def _host_slots(t, B, S, who):
    slots = _host_lens(t, B, who)
    if S < B:
        raise RuntimeError(f"{who}: a pool of {S} slots cannot hold {B} rows")
    for s in slots:
        if not 0 <= s < S:
            raise RuntimeError(f"{who}: slot {s} is outside the pool of {S}")
    if len(set(slots)) != B:
        raise RuntimeError(f"{who}: a slot is named twice in {slots}")
    return slots


def kv_append_slots(qkv, qw, kw, sin, cos, k_cache, v_cache, pos_dev, pos_host,
                    slots_dev, slots_host, eps):
    B = qkv.shape[0]
    pos = _host_lens(pos_host, B, "kv_append_slots")
    slots = _host_slots(slots_host, B, k_cache.shape[0], "kv_append_slots")
    Tn, Tmax = qkv.shape[1], k_cache.shape[2]
    for p in pos:  # every position before the first write, as the binding does
        if p < 0 or p + Tn > Tmax:
            raise RuntimeError(f"kv_append: rows [{p}, {p + Tn}) do not fit a "
                               f"cache of {Tmax} rows")
    return torch.cat([kv_append_ragged(qkv[b:b + 1], qw, kw, sin, cos,
                                       k_cache[s:s + 1], v_cache[s:s + 1], None,
                                       torch.tensor([pos[b]]), eps)
                      for b, s in enumerate(slots)], dim=0)


def attn_decode_slots(q, k_cache, v_cache, kv_lens_dev, kv_lens_host, slots_dev,
                      slots_host, num_splits):
    B = q.shape[0]
    lens = _host_lens(kv_lens_host, B, "attn_decode_slots")
    slots = _host_slots(slots_host, B, k_cache.shape[0], "attn_decode_slots")
    return torch.cat([attn_decode_ragged(q[b:b + 1], k_cache[s:s + 1], v_cache[s:s + 1],
                                         None, torch.tensor([lens[b]]), num_splits)
                      for b, s in enumerate(slots)], dim=0)


# Paged decode (ops.PAGED_API): the caches are pools (P,H,PS,C) of P pages of
# PS positions and position p of batch row b lives at row p % PS of page
# table[b][p // PS] of a (B,MP) table. The ragged op on the cache gathered
# through the table; what append and store write is scattered back, row by
# row, so nothing else in the pool changes.
def _host_table(t, B, k_pool, who):
    """(table rows as lists, P, PS) after the binding's checks of the shapes."""
    if k_pool.dim() != 4:
        raise RuntimeError(f"{who}: the pools must be (P,H,PS,C)")
    P, PS = k_pool.shape[0], k_pool.shape[2]
    if not 16 <= PS <= 128 or PS & (PS - 1):
        raise RuntimeError(f"{who}: the page size must be a power of two in "
                           f"[16, 128], got {PS}")
    if t.is_cuda or t.dim() != 2 or t.shape[0] != B or t.shape[1] < 1 \
            or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise RuntimeError(f"{who}: the host block table must be a CPU integer "
                           f"tensor ({B}, MP)")
    return t.to(torch.int64), P, PS


def _check_table_dev(dev, host, who):
    """What the binding asks of the device copy, wherever one is given."""
    if dev is not None and dev.is_cuda and \
            (dev.dtype != torch.int32 or dev.shape != host.shape):
        raise RuntimeError(f"{who}: block_table_dev must be int32 of shape "
                           f"{tuple(host.shape)}")


def _cover(table, b, lo, hi, P, PS, written, who):
    """The binding's check of the entries that cover positions [lo, hi) of row
    b; ``written``: the set of pages that receive writes (None: a read)."""
    for j in range(lo // PS, -(-hi // PS)):
        pg = int(table[b, j])
        if not 0 <= pg < P:
            raise RuntimeError(f"{who}: block_table[{b}][{j}] = {pg} is outside "
                               f"the pool of {P} pages")
        if written is not None:
            if pg in written:
                raise RuntimeError(f"{who}: page {pg} receives writes twice")
            written.add(pg)


def _page_rows(table, b, lo, hi, PS):
    """Index tensors (page, row in page) of positions [lo, hi) of row b."""
    p = torch.arange(lo, hi)
    return table[b, p // PS], p % PS


def kv_append_paged(qkv, qw, kw, sin, cos, k_pool, v_pool, pos_dev, pos_host,
                    table_dev, table_host, eps):
    who = "kv_append_paged"
    B, Tn = qkv.shape[:2]
    pos = _host_lens(pos_host, B, who)
    table, P, PS = _host_table(table_host, B, k_pool, who)
    _check_table_dev(table_dev, table, who)
    Tmax = table.shape[1] * PS
    written = set()
    for b, p in enumerate(pos):  # everything before the first write
        if p < 0 or p + Tn > Tmax:
            raise RuntimeError(f"kv_append: rows [{p}, {p + Tn}) do not fit a "
                               f"cache of {Tmax} rows")
        if sin.shape[0] < p + Tn or cos.shape[0] < p + Tn:
            raise RuntimeError(f"kv_append: sin/cos tables have {sin.shape[0]} rows, "
                               f"position {p + Tn - 1} needed")
        _cover(table, b, p, p + Tn, P, PS, written, who)
    H, C = qkv.shape[3], qkv.shape[4]
    qs = []
    for b, p in enumerate(pos):
        # rows [p, p+Tn) of the gathered cache are all the append touches
        kg = k_pool.new_empty(1, H, Tmax, C)
        vg = v_pool.new_empty(1, H, Tmax, C)
        qs.append(kv_append_ragged(qkv[b:b + 1], qw, kw, sin, cos, kg, vg, None,
                                   torch.tensor([p]), eps))
        pg, r = _page_rows(table, b, p, p + Tn, PS)
        k_pool[pg, :, r] = kg[0, :, p:p + Tn].transpose(0, 1)
        v_pool[pg, :, r] = vg[0, :, p:p + Tn].transpose(0, 1)
    return torch.cat(qs, dim=0)


def _gather_pages(pool, table, b, n, PS):
    """Positions [0, ceil(n / PS) * PS) of row b as a cache (1,H,*,C)."""
    pages = pool[table[b, :-(-n // PS)]]                  # (n_pages,H,PS,C)
    H, C = pool.shape[1], pool.shape[3]
    return pages.permute(1, 0, 2, 3).reshape(1, H, -1, C)


def attn_decode_paged(q, k_pool, v_pool, kv_lens_dev, kv_lens_host, table_dev,
                      table_host, num_splits):
    who = "attn_decode_paged"
    B, Tq = q.shape[0], q.shape[2]
    lens = _host_lens(kv_lens_host, B, who)
    table, P, PS = _host_table(table_host, B, k_pool, who)
    _check_table_dev(table_dev, table, who)
    Tmax = table.shape[1] * PS
    for b, n in enumerate(lens):
        if n > Tmax:
            raise RuntimeError(f"decode_attention: kv_len {n} exceeds the cache ({Tmax})")
        if not 1 <= Tq <= min(16, n):
            raise RuntimeError("decode_attention: 1 <= Tq <= min(16, kv_len) required "
                               f"(Tq {Tq}, kv_len {n})")
        _cover(table, b, 0, n, P, PS, None, who)   # shared pages are legal to read
    return torch.cat([attn_decode_ragged(q[b:b + 1], _gather_pages(k_pool, table, b, n, PS),
                                         _gather_pages(v_pool, table, b, n, PS), None,
                                         torch.tensor([n]), num_splits)
                      for b, n in enumerate(lens)], dim=0)


def kv_store_paged(k, v, k_pool, v_pool, lens_dev, lens_host, table_dev, table_host):
    who = "kv_store_paged"
    B, H, T, C = k.shape
    lens = _host_lens(lens_host, B, who)
    table, P, PS = _host_table(table_host, B, k_pool, who)
    _check_table_dev(table_dev, table, who)
    if v.shape != k.shape or k_pool.shape != v_pool.shape or \
            (k_pool.shape[1], k_pool.shape[3]) != (H, C):
        raise RuntimeError(f"{who}: k, v must be (B,H,T,C) and the pools (P,H,PS,C)")
    written = set()
    for b, n in enumerate(lens):
        if not 0 <= n <= min(T, table.shape[1] * PS):
            raise RuntimeError(f"{who}: length {n} exceeds the {T} rows given or "
                               f"the table's {table.shape[1] * PS}")
        _cover(table, b, 0, n, P, PS, written, who)
    for b, n in enumerate(lens):
        pg, r = _page_rows(table, b, 0, n, PS)
        k_pool[pg, :, r] = k[b, :, :n].transpose(0, 1).to(k_pool.dtype)
        v_pool[pg, :, r] = v[b, :, :n].transpose(0, 1).to(v_pool.dtype)


# Seeded token sampling (ops.SAMPLING_API): top-k + Gumbel-max, the
# definition of csrc/sampling.hip in fp32 on the logits' device. The Philox
# words come from the host mirror, so one (seed, step) gives one stream on
# either backend; the tokens agree wherever the top two scores are further
# apart than fp32 rounding.
def sample_tokens(logits, inv_t, top_k, seed, step):
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise RuntimeError(f"sample_tokens: logits must be (B, V), got {tuple(logits.shape)}")
    inv_t, top_k = float(inv_t), int(top_k)
    if not (math.isfinite(inv_t) and inv_t > 0):
        raise RuntimeError(f"sample_tokens: inv_t must be finite and > 0, got {inv_t}")
    if top_k < 0:
        raise RuntimeError(f"sample_tokens: top_k >= 0 required (0: all), got {top_k}")
    B, V = logits.shape
    return _sample_from_words(logits, inv_t, top_k, ref.sample_words(B, V, seed, step))


def _sample_from_words(logits, inv_t, top_k, words):
    """The draw of every row of logits (B, V) from its Philox words, uint32
    (B, V); words None: greedy, the score is the logit alone."""
    B, V = logits.shape
    lf = logits.float()
    if words is None:
        score = lf.clone()
    else:
        m = torch.from_numpy((words >> 9).astype("int32"))
        t = (2 * m + 1).to(torch.float32) * 2.0 ** -24   # exact: < 2^24
        noise = -torch.log(-torch.log(t))
        score = lf * inv_t + noise.to(logits.device)
    if 1 <= top_k < V:
        kth = torch.topk(lf, top_k, dim=-1).values[:, -1:]
        score = score.masked_fill(lf < kth, float("-inf"))
    # lowest index of the maximal score, spelled out: argmax's tie order is
    # not defined on the GPU
    best = score.max(dim=-1, keepdim=True).values
    idx = torch.arange(V, device=logits.device).expand(B, V)
    tok = torch.where(score == best, idx, V).min(dim=-1).values
    return tok.clamp_(max=V - 1)   # a NaN row (outside the contract) has no maximum


def sample_tokens_rows(logits, params_dev, inv_t, top_k, seeds, steps, rows):
    """Row b by the definition of ``sample_tokens`` with its own (inv_t[b],
    top_k[b], seeds[b], steps[b]) and Philox row word rows[b]; inv_t[b] == 0:
    greedy (the logit alone, top_k ignored, lowest index of the maximum). The
    five host tensors are validated as the binding does; params_dev is what
    the kernel reads and is unused here."""
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise RuntimeError(f"sample_tokens_rows: logits must be (B, V), got {tuple(logits.shape)}")
    B, V = logits.shape
    who = "sample_tokens_rows"
    if inv_t.is_cuda or inv_t.shape != (B,) or inv_t.dtype != torch.float32:
        raise RuntimeError(f"{who}: inv_t must be a CPU float32 tensor of {B} values")
    inv_t = [float(x) for x in inv_t.tolist()]
    top_k, seeds = _host_lens(top_k, B, who), _host_lens(seeds, B, who)
    steps, rows = _host_lens(steps, B, who), _host_lens(rows, B, who)
    for b in range(B):
        if not (math.isfinite(inv_t[b]) and inv_t[b] >= 0):
            raise RuntimeError(f"{who}: inv_t must be finite and > 0, or 0 for a "
                               f"greedy row, got {inv_t[b]}")
        if top_k[b] < 0:
            raise RuntimeError(f"{who}: top_k >= 0 required (0: all), got {top_k[b]}")
        if not (0 <= steps[b] < 1 << 32 and 0 <= rows[b] < 1 << 32):
            raise RuntimeError(f"{who}: step and row must be in [0, 2^32), got "
                               f"{steps[b]}, {rows[b]}")
    out = []
    for b in range(B):
        if inv_t[b] == 0:
            out.append(_sample_from_words(logits[b:b + 1], 1.0, 0, None))
        else:
            words = ref.sample_words(1, V, seeds[b], steps[b], row0=rows[b])
            out.append(_sample_from_words(logits[b:b + 1], inv_t[b], top_k[b], words))
    return torch.cat(out) if out else torch.empty(0, dtype=torch.int64, device=logits.device)


# GELU (tanh approximation)
def gelu_fwd(x):
    return torch.nn.functional.gelu(x, approximate="tanh")


def gelu_bwd(dy, x):
    xf = x.float()
    c0, c1 = 0.7978845608028654, 0.044715
    inner = c0 * (xf + c1 * xf ** 3)
    t = torch.tanh(inner)
    dg = 0.5 * (1 + t) + 0.5 * xf * (1 - t * t) * c0 * (1 + 3 * c1 * xf ** 2)
    return (dy.float() * dg).to(x.dtype)


# Embedding backward: fp32 scatter-add of dy (N, D) into (V, D)
def embedding_bwd(dy2d, idx, V):
    dw32 = torch.zeros(V, dy2d.shape[-1], dtype=torch.float32, device=dy2d.device)
    dw32.index_add_(0, idx, dy2d.float())
    return dw32.to(dy2d.dtype)


# Cross-entropy over (N, V) logits: (sum of the row losses, lse); the
# backward takes dloss as a (1,) tensor and divides by N itself.
def ce_fwd(logits, targets):
    lf = logits.float()
    lse = torch.logsumexp(lf, dim=-1)
    picked = lf.gather(1, targets[:, None]).squeeze(1)
    return (lse - picked).sum(), lse


def ce_bwd(logits, targets, lse, gscale):
    N = logits.shape[0]
    lf = logits.float()
    p = torch.exp(lf - lse[:, None])
    p.scatter_add_(1, targets[:, None],
                   -torch.ones(N, 1, device=p.device, dtype=p.dtype))
    return (p * (gscale / N)).to(logits.dtype)


# AdamW on flat fp32 buffers, in place (semantics: ops.adamw_step)
def adamw_step(master, grad, m, v, out_bf16, write_bf16, sq_sum, lr, beta1, beta2,
               eps, wd_over_peak_lr, grad_scale, clip_norm, step):
    gnorm = float(sq_sum.float().sqrt()) * grad_scale
    clip_coef = grad_scale * min(1.0, clip_norm / (gnorm + 1e-12))
    g = grad * clip_coef
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    mhat = m / (1 - beta1 ** step)
    vhat = v / (1 - beta2 ** step)
    update = mhat / (vhat.sqrt() + eps) + wd_over_peak_lr * master
    master.add_(update, alpha=-lr)
    if write_bf16:
        out_bf16.copy_(master.to(torch.bfloat16))


# Batched transpose (ops.TRANSPOSE_API): matrix m of the table, rows x cols
# at src[src_off:], lands transposed at dst[dst_off:]. The host table (n, 5)
# int64 {src_off, dst_off, rows, cols, tile prefix} is the truth and is
# validated as the binding validates it; any dtype goes.
TRANSPOSE_TILE = 64


def transpose_batched(src, dst, table_dev, table_host, max_blocks=0):
    who = "transpose_batched"
    if src.dim() != 1 or dst.dim() != 1 or src.dtype != dst.dtype:
        raise RuntimeError(f"{who}: src and dst must be flat buffers of one dtype")
    t = table_host
    if t.is_cuda or t.dim() != 2 or t.shape[1] != 5 or t.dtype != torch.int64:
        raise RuntimeError(f"{who}: the host table must be a CPU int64 tensor (n, 5)")
    if tuple(table_dev.shape) != tuple(t.shape):
        raise RuntimeError(f"{who}: the device table must be {tuple(t.shape)}")
    tiles = 0
    for m, (so, do, rows, cols, prefix) in enumerate(t.tolist()):
        if rows < 1 or cols < 1 or so < 0 or so + rows * cols > src.numel():
            raise RuntimeError(f"{who}: matrix {m} ({rows} x {cols} at {so}) leaves src")
        if do < 0 or do + rows * cols > dst.numel():
            raise RuntimeError(f"{who}: image {m} at {do} leaves dst")
        if prefix != tiles:
            raise RuntimeError(f"{who}: tile prefix of matrix {m} is {prefix}, "
                               f"expected {tiles}")
        tiles += -(-rows // TRANSPOSE_TILE) * -(-cols // TRANSPOSE_TILE)
        dst[do:do + rows * cols].view(cols, rows).copy_(
            src[so:so + rows * cols].view(rows, cols).t())
