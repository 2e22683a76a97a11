"""KV-cache decode on the CPU: the fp32 torch references of ops.kv_append /
ops.decode_attention / ops.prefill_attention, KVCache bookkeeping and
decode_step against one full forward."""
import pytest
import torch

from midgpt_amd import ops
from midgpt_amd.config import GPTConfig
from midgpt_amd.generate import KVCache, decode_step
from midgpt_amd.models.gpt import GPT
from midgpt_amd.ops import reference as ref

TINY = GPTConfig(block_size=16, vocab_size=37, n_layer=2, n_head=2, n_embd=16,
                 dropout=0.0)
B, H, C, T, TMAX = 2, 3, 8, 16, 32
SENTINEL = 777.0


@pytest.fixture(scope="module")
def seq():
    """One 16-token sequence and its full-sequence reference (read-only)."""
    g = torch.Generator().manual_seed(21)
    qkv = torch.randn(B, T, 3, H, C, generator=g)
    qw = 1.0 + 0.1 * torch.randn(C, generator=g)
    kw = 1.0 + 0.1 * torch.randn(C, generator=g)
    sin, cos = ref.rope_tables(C, TMAX)
    q = ref.apply_rope(ref.qk_layernorm(qkv[:, :, 0].permute(0, 2, 1, 3), qw), sin[:T], cos[:T])
    k = ref.apply_rope(ref.qk_layernorm(qkv[:, :, 1].permute(0, 2, 1, 3), kw), sin[:T], cos[:T])
    v = qkv[:, :, 2].permute(0, 2, 1, 3)
    o = ref.causal_attention(q, k, v).transpose(1, 2).reshape(B, T, H * C)
    return dict(qkv=qkv, qw=qw, kw=kw, sin=sin, cos=cos, k=k, v=v, o=o)


def _caches():
    return (torch.full((B, H, TMAX, C), SENTINEL),
            torch.full((B, H, TMAX, C), SENTINEL))


def test_chunked_append_and_decode_match_full_attention(seq):
    kc, vc = _caches()
    pos = 0
    for n in (5, 1, 1, 9):
        q = ops.kv_append(seq["qkv"][:, pos:pos + n], seq["qw"], seq["kw"],
                          seq["sin"], seq["cos"], kc, vc, pos)
        assert q.shape == (B, H, n, C)
        o = ops.decode_attention(q, kc, vc, pos + n)
        assert o.shape == (B, n, H * C)
        assert torch.allclose(o, seq["o"][:, pos:pos + n], atol=1e-5, rtol=1e-5)
        pos += n
        # rows beyond pos untouched after every chunk
        assert bool((kc[:, :, pos:] == SENTINEL).all())
        assert bool((vc[:, :, pos:] == SENTINEL).all())
    assert pos == T
    assert torch.allclose(kc[:, :, :T], seq["k"], atol=1e-5, rtol=1e-5)
    assert torch.equal(vc[:, :, :T], seq["v"])


@pytest.mark.parametrize("num_splits", [1, 5])
def test_decode_attention_num_splits_is_semantics_free(seq, num_splits):
    kc, vc = _caches()
    q = ops.kv_append(seq["qkv"], seq["qw"], seq["kw"], seq["sin"], seq["cos"],
                      kc, vc, 0)
    o = ops.decode_attention(q[:, :, -3:].contiguous(), kc, vc, T, num_splits)
    assert torch.allclose(o, seq["o"][:, -3:], atol=1e-5, rtol=1e-5)


def test_prefill_attention_fills_cache_and_matches(seq):
    kc, vc = _caches()
    o = ops.prefill_attention(seq["qkv"], seq["qw"], seq["kw"], seq["sin"],
                              seq["cos"], kc, vc)
    assert o.shape == (B, T, H * C)
    assert torch.allclose(o, seq["o"], atol=1e-5, rtol=1e-5)
    assert torch.allclose(kc[:, :, :T], seq["k"], atol=1e-5, rtol=1e-5)
    assert torch.equal(vc[:, :, :T], seq["v"])
    assert bool((kc[:, :, T:] == SENTINEL).all())
    assert bool((vc[:, :, T:] == SENTINEL).all())


def test_append_and_decode_guards(seq):
    kc, vc = _caches()
    a = (seq["qw"], seq["kw"], seq["sin"], seq["cos"], kc, vc)
    with pytest.raises(RuntimeError):
        ops.kv_append(seq["qkv"][:, :4], *a, TMAX - 3)      # pos + Tn > Tmax
    with pytest.raises(RuntimeError):
        ops.kv_append(seq["qkv"][:, :4], *a, -1)
    with pytest.raises(RuntimeError):                        # table too short
        ops.kv_append(seq["qkv"][:, :4], seq["qw"], seq["kw"], seq["sin"][:8],
                      seq["cos"][:8], kc, vc, 6)
    assert bool((kc == SENTINEL).all()) and bool((vc == SENTINEL).all())
    q = torch.zeros(B, H, 17, C)
    with pytest.raises(RuntimeError):
        ops.decode_attention(q, kc, vc, 20)                  # Tq = 17
    with pytest.raises(RuntimeError):
        ops.decode_attention(q[:, :, :4], kc, vc, 3)         # Tq > kv_len
    with pytest.raises(RuntimeError):
        ops.decode_attention(q[:, :, :4], kc, vc, TMAX + 1)  # kv_len > Tmax
    with pytest.raises(RuntimeError):
        ops.decode_attention(q[:, :, :4], kc, vc, 8, 65)     # num_splits > 64


def test_kvcache_bookkeeping():
    torch.manual_seed(22)
    model = GPT(TINY).eval()
    cache = KVCache(model, 2, torch.device("cpu"), torch.float32)
    assert cache.buf.shape == (2, 2, 2, 2, 16, 8)
    assert cache.pos == 0 and len(cache.k) == 2 and len(cache.v) == 2
    assert cache.k[1].shape == (2, 2, 16, 8)
    assert cache.k[1].data_ptr() == cache.buf[1, 0].data_ptr()   # views, no copies
    assert cache.v[0].data_ptr() == cache.buf[0, 1].data_ptr()
    idx = torch.randint(0, 37, (2, 16))
    decode_step(model, idx[:, :6], cache)
    assert cache.pos == 6
    decode_step(model, idx[:, 6:7], cache)
    assert cache.pos == 7
    ptr = cache.buf.data_ptr()
    cache.reset()
    assert cache.pos == 0 and cache.buf.data_ptr() == ptr
    decode_step(model, idx[:, :15], cache)
    assert cache.pos == 15
    with pytest.raises(RuntimeError):
        decode_step(model, idx[:, :2], cache)                # 15 + 2 > block_size
    assert cache.pos == 15
    decode_step(model, idx[:, 15:], cache)
    assert cache.pos == 16
    with pytest.raises(RuntimeError):
        decode_step(model, idx[:, :1], cache)


def test_decode_step_teacher_forced_matches_full_forward():
    torch.manual_seed(23)
    model = GPT(TINY).eval()
    idx = torch.randint(0, 37, (2, 16))
    with torch.no_grad():
        full = model(idx)                                    # (2,16,V)
    cache = KVCache(model, 2, torch.device("cpu"), torch.float32)
    logits = decode_step(model, idx[:, :6], cache)
    assert logits.shape == (2, 37)
    assert torch.allclose(logits, full[:, 5], atol=1e-4, rtol=1e-4)
    for t in range(6, 16):
        logits = decode_step(model, idx[:, t:t + 1], cache)
        assert torch.allclose(logits, full[:, t], atol=1e-4, rtol=1e-4), t


def test_decode_step_long_prefill_on_cpu():
    """A prompt of more than 16 tokens at position 0 goes through
    prefill_attention; same logits as the full forward."""
    torch.manual_seed(24)
    cfg = GPTConfig(block_size=32, vocab_size=37, n_layer=2, n_head=2, n_embd=16,
                    dropout=0.0)
    model = GPT(cfg).eval()
    idx = torch.randint(0, 37, (1, 24))
    with torch.no_grad():
        full = model(idx)
    cache = KVCache(model, 1, torch.device("cpu"), torch.float32)
    logits = decode_step(model, idx[:, :20], cache)
    assert torch.allclose(logits, full[:, 19], atol=1e-4, rtol=1e-4)
    for t in range(20, 24):
        logits = decode_step(model, idx[:, t:t + 1], cache)
        assert torch.allclose(logits, full[:, t], atol=1e-4, rtol=1e-4), t
