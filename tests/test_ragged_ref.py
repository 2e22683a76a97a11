"""Ragged batched decode on the CPU: ``ops.RAGGED_API`` on ref_backend against
the uniform ops sequence by sequence, the host guards, and
``prefill_ragged`` / ``decode_step_ragged`` / ``generate_ragged`` on a tiny
fp32 model against the full forward and ``generate`` of each prompt alone."""
import pytest
import torch

from midgpt_amd import ops
from midgpt_amd.config import GPTConfig
from midgpt_amd.generate import (KVCache, decode_step_ragged, generate,
                                 generate_ragged, prefill_ragged)
from midgpt_amd.models.gpt import GPT
from midgpt_amd.ops import ref_backend
from midgpt_amd.ops import reference as ref

B, H, C, TMAX = 3, 2, 64, 64
NAN = float("nan")


def nan_equal(a, b):
    return torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)) \
        and torch.equal(torch.isnan(a), torch.isnan(b))


def test_ragged_api_names():
    assert ops.RAGGED_API == ("kv_append_ragged", "attn_decode_ragged")
    for name in ops.RAGGED_API:
        assert callable(getattr(ref_backend, name, None)), name
        assert name not in ops.BACKEND_API
        if ops.have_ext():
            assert callable(getattr(ops._C, name, None)), name
    assert ops.BACKEND_API == (
        "rmsnorm_fwd", "rmsnorm_bwd", "qkv_prep_fwd", "qkv_prep_bwd",
        "attn_fwd", "attn_bwd", "attn_fwd_dropout", "attn_bwd_dropout",
        "gelu_fwd", "gelu_bwd", "embedding_bwd", "ce_fwd", "ce_bwd",
        "adamw_step", "kv_append", "attn_decode")


def _append_inputs(Tn, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, Tn, 3, H, C, generator=g)
    qw = 1.0 + 0.1 * torch.randn(C, generator=g)
    kw = 1.0 + 0.1 * torch.randn(C, generator=g)
    sin, cos = ref.rope_tables(C, TMAX)
    return qkv, qw, kw, sin.contiguous(), cos.contiguous()


def _nan_caches():
    return torch.full((B, H, TMAX, C), NAN), torch.full((B, H, TMAX, C), NAN)


@pytest.mark.parametrize("Tn,pos", [(1, (0, 5, 63)), (16, (0, 5, 48))])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_kv_append_ragged_equals_uniform_per_sequence(Tn, pos, as_tensor):
    qkv, qw, kw, sin, cos = _append_inputs(Tn, 51)
    kc, vc = _nan_caches()
    q = ops.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc,
                             torch.tensor(pos) if as_tensor else pos)
    assert q.shape == (B, H, Tn, C)
    for b in range(B):
        kc1, vc1 = (t[b:b + 1].clone() for t in _nan_caches())
        q1 = ops.kv_append(qkv[b:b + 1], qw, kw, sin, cos, kc1, vc1, pos[b])
        assert torch.equal(q[b:b + 1], q1), b
        # the written rows agree and every other row is still NaN
        assert nan_equal(kc[b:b + 1], kc1), b
        assert nan_equal(vc[b:b + 1], vc1), b
        written = torch.zeros(TMAX, dtype=torch.bool)
        written[pos[b]:pos[b] + Tn] = True
        assert bool(torch.isnan(kc[b][:, ~written]).all()), b
        assert bool(torch.isnan(vc[b][:, ~written]).all()), b
        assert not bool(torch.isnan(kc[b][:, written]).any()), b
        assert not bool(torch.isnan(vc[b][:, written]).any()), b


@pytest.mark.parametrize("Tq,kv_lens", [(1, (1, 9, 64)), (3, (3, 10, 64))])
def test_decode_attention_ragged_equals_uniform_per_sequence(Tq, kv_lens):
    g = torch.Generator().manual_seed(52)
    q = torch.randn(B, H, Tq, C, generator=g)
    kc = torch.randn(B, H, TMAX, C, generator=g)
    vc = torch.randn(B, H, TMAX, C, generator=g)
    for b, n in enumerate(kv_lens):        # rows past a sequence's length
        kc[b, :, n:] = NAN
        vc[b, :, n:] = NAN
    kc0, vc0 = kc.clone(), vc.clone()
    o = ops.decode_attention_ragged(q, kc, vc, kv_lens)
    assert o.shape == (B, Tq, H * C)
    assert not bool(torch.isnan(o).any())
    assert nan_equal(kc, kc0) and nan_equal(vc, vc0)
    for b, n in enumerate(kv_lens):
        o1 = ops.decode_attention(q[b:b + 1], kc[b:b + 1], vc[b:b + 1], n)
        assert torch.equal(o[b:b + 1], o1), b


def test_ragged_guards():
    qkv, qw, kw, sin, cos = _append_inputs(4, 53)
    kc, vc = _nan_caches()
    with pytest.raises(RuntimeError):      # pos + Tn > Tmax for one sequence
        ops.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc, (0, 5, TMAX - 3))
    with pytest.raises(RuntimeError):      # negative position
        ops.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc, (0, -1, 5))
    with pytest.raises(RuntimeError):      # tables shorter than pos + Tn
        ops.kv_append_ragged(qkv, qw, kw, sin[:16], cos[:16], kc, vc, (0, 5, 13))
    with pytest.raises(RuntimeError):      # wrong length of pos
        ops.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc, (0, 5))
    with pytest.raises(RuntimeError):
        ops.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc, torch.zeros(B + 1, dtype=torch.int64))
    with pytest.raises(RuntimeError):      # the backend checks too
        ref_backend.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc,
                                     torch.tensor([0, 5, TMAX - 3]),
                                     torch.tensor([0, 5, TMAX - 3]), 1e-6)
    assert bool(torch.isnan(kc).all()) and bool(torch.isnan(vc).all())
    q = torch.zeros(B, H, 3, C)
    kc, vc = torch.zeros(B, H, TMAX, C), torch.zeros(B, H, TMAX, C)
    with pytest.raises(RuntimeError):      # kv_len < Tq
        ops.decode_attention_ragged(q, kc, vc, (3, 2, 10))
    with pytest.raises(RuntimeError):      # kv_len > Tmax
        ops.decode_attention_ragged(q, kc, vc, (3, TMAX + 1, 10))
    with pytest.raises(RuntimeError):      # wrong length of kv_lens
        ops.decode_attention_ragged(q, kc, vc, (3, 10))
    with pytest.raises(RuntimeError):
        ref_backend.attn_decode_ragged(q, kc, vc, torch.tensor([3, 2, 10]),
                                       torch.tensor([3, 2, 10]), 0)
    with pytest.raises(RuntimeError):      # Tq = 17
        ops.decode_attention_ragged(torch.zeros(B, H, 17, C), kc, vc, (20, 20, 20))


# ---------------------------------------------------------------------------
# generation on a tiny fp32 CPU model
# ---------------------------------------------------------------------------
BLOCK, VOCAB = 32, 96
LENS = (1, 5, 17)
N_NEW = 8


@pytest.fixture(scope="module")
def tiny():
    cfg = GPTConfig(block_size=BLOCK, vocab_size=VOCAB, n_layer=2, n_head=2,
                    n_embd=64, dropout=0.0)
    torch.manual_seed(61)
    model = GPT(cfg).eval()
    g = torch.Generator().manual_seed(62)
    prompts = [torch.randint(0, VOCAB, (n,), generator=g) for n in LENS]
    return model, prompts


def test_teacher_forced_logits_match_full_forward(tiny):
    model, prompts = tiny
    g = torch.Generator().manual_seed(63)
    steps = 6
    cont = torch.randint(0, VOCAB, (len(LENS), steps), generator=g)
    cache = KVCache(model, len(LENS))
    rows = [prefill_ragged(model, prompts, cache)]
    assert cache.lens == list(LENS)
    for t in range(steps):
        rows.append(decode_step_ragged(model, cont[:, t:t + 1], cache))
        assert cache.lens == [n + t + 1 for n in LENS]
        assert cache.lens_dev.tolist() == cache.lens
    got = torch.stack(rows, dim=1)                      # (B, steps + 1, V)
    worst = 0.0
    for b, p in enumerate(prompts):
        full = torch.cat([p, cont[b]])[None]
        with torch.no_grad():
            want = model(full)[0, LENS[b] - 1:]
        worst = max(worst, float((got[b] - want).abs().max()))
        assert torch.allclose(got[b], want, atol=1e-4, rtol=0), (b, worst)
    print(f"RAGGED teacher-forced cpu fp32 max abs logit diff {worst:.3e}")


def _alone(model, p, n):
    """generate() of one prompt at B=1 with the top-2 logit gap of each step."""
    out = generate(model, p[None], n, temperature=0)[0]
    gaps = []
    with torch.no_grad():
        for t in range(n):
            top = model(out[None, :p.numel() + t])[0, -1].topk(2).values
            gaps.append(float(top[0] - top[1]))
    return out, gaps


def test_generate_ragged_greedy_equals_generate_per_prompt(tiny):
    model, prompts = tiny
    alone = [_alone(model, p, N_NEW) for p in prompts]
    for _, gaps in alone:                  # precondition: no near-tie
        assert min(gaps) > 1e-3, gaps
    outs = generate_ragged(model, prompts, N_NEW, temperature=0)
    assert len(outs) == len(prompts)
    for (want, _), got in zip(alone, outs):
        assert torch.equal(got, want)


def test_generate_ragged_eos(tiny):
    model, prompts = tiny
    plain = generate_ragged(model, prompts, N_NEW, temperature=0)
    eos = int(plain[1][LENS[1] + 2])       # what sequence 1 emits at step 3
    first = {b: (plain[b][LENS[b]:] == eos).nonzero() for b in range(3)}
    assert int(first[1][0]) <= 2
    for every in (1, 16):
        outs = generate_ragged(model, prompts, N_NEW, temperature=0, eos_id=eos,
                               stop_check_every=every)
        for b in range(3):
            if first[b].numel():           # cut after its first eos
                want = plain[b][:LENS[b] + int(first[b][0]) + 1]
                assert int(want[-1]) == eos
            else:                          # unaffected
                want = plain[b]
            assert torch.equal(outs[b], want), (every, b)
    assert outs[1].numel() <= LENS[1] + 3


def test_generate_ragged_full_and_nearly_full_prompts(tiny):
    model, _ = tiny
    g = torch.Generator().manual_seed(64)
    prompts = [torch.randint(0, VOCAB, (n,), generator=g)
               for n in (BLOCK, BLOCK - 2, 4, BLOCK + 5)]
    outs = generate_ragged(model, prompts, 6, temperature=0)
    assert [o.numel() - p.numel() for o, p in zip(outs, prompts)] == [1, 3, 6, 1]
    for o, p in zip(outs, prompts):
        assert torch.equal(o[:p.numel()], p)
    # the short sequence is not disturbed by its retired neighbours
    alone = generate(model, prompts[2][None], 6, temperature=0)[0]
    assert torch.equal(outs[2], alone)
    # sampling: budgets and token range hold as well
    outs = generate_ragged(model, prompts, 6, temperature=0.9, top_k=5,
                           generator=torch.Generator().manual_seed(65))
    assert [o.numel() - p.numel() for o, p in zip(outs, prompts)] == [1, 3, 6, 1]
    assert all(0 <= int(o.min()) and int(o.max()) < VOCAB for o in outs)
    assert generate_ragged(model, [], 4) == []
