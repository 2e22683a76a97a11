"""Seeded token sampling on the CPU: ``ref_backend.sample_tokens`` and
``ops.sample_tokens`` against the float64 oracle of ops/reference.py, the
counter's contract, and ``generate`` / ``generate_ragged`` with ``seed=``."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import sampling_util as S
from midgpt_amd import generate as G
from midgpt_amd import ops
from midgpt_amd.config import GPTConfig
from midgpt_amd.models.gpt import GPT
from midgpt_amd.ops import ref_backend


def test_sampling_api():
    assert ops.SAMPLING_API == ("sample_tokens",)
    for name in ops.SAMPLING_API:
        assert callable(getattr(ref_backend, name))
    assert ops.BACKEND_API == (
        "rmsnorm_fwd", "rmsnorm_bwd", "qkv_prep_fwd", "qkv_prep_bwd",
        "attn_fwd", "attn_bwd", "attn_fwd_dropout", "attn_bwd_dropout",
        "gelu_fwd", "gelu_bwd", "embedding_bwd", "ce_fwd", "ce_bwd",
        "adamw_step", "kv_append", "attn_decode")
    assert ops.RAGGED_API == ("kv_append_ragged", "attn_decode_ragged")


def test_per_row_optimality():
    decided = rows = 0
    for i, (V, B, T, k) in enumerate(S.OPT_CASES):
        logits = S.bf16_logits(V, B, 4.0, 300 + i)
        inv_t = S.inv_t_of(T)
        for step in (0, 7):
            tok = ref_backend.sample_tokens(logits, inv_t, k or 0, 41 + i, step)
            d, n = S.check_optimal(tok, logits, inv_t, k, 41 + i, step)
            decided, rows = decided + d, rows + n
    print(f"SAMPLING ref rows decided by > 2 eps: {decided}/{rows}")
    assert decided >= 0.99 * rows


def test_candidate_sets():
    S.check_candidate_sets(ref_backend.sample_tokens, 37)


@pytest.mark.parametrize("V,top_k,temperature,bound", S.CHI2_CASES)
def test_distribution(V, top_k, temperature, bound):
    S.check_chi2(ref_backend.sample_tokens, V, top_k, temperature, bound)


def test_counter_contract():
    logits = S.bf16_logits(37, 1, 1.5, 17).repeat(4096, 1)
    a = ops.sample_tokens(logits, 0.9, 8, seed=3, step=2)
    assert a.dtype == torch.int64 and a.shape == (4096,)
    assert torch.equal(a, ops.sample_tokens(logits, 0.9, 8, seed=3, step=2))
    assert len(set(a.tolist())) > 1                       # rows differ
    steps = [ops.sample_tokens(logits[:4], 0.9, 8, seed=3, step=t) for t in range(8)]
    assert len({tuple(s.tolist()) for s in steps}) > 1    # steps differ
    assert not torch.equal(a, ops.sample_tokens(logits, 0.9, 8, seed=4, step=2))
    # seeds are 64-bit: the high word counts, and 2^64 wraps
    assert not torch.equal(a, ops.sample_tokens(logits, 0.9, 8, seed=3 + (1 << 32), step=2))
    assert torch.equal(a, ops.sample_tokens(logits, 0.9, 8, seed=3 + (1 << 64), step=2))
    # the row index is part of the counter: a row called alone is row 0, so
    # it repeats the batch's draw only for row 0
    alone = [int(ops.sample_tokens(logits[b:b + 1], 0.9, 8, seed=3, step=2)) for b in range(64)]
    assert alone[0] == int(a[0]) and len(set(alone)) == 1
    assert alone != a[:64].tolist()


def test_op_arguments():
    logits = S.bf16_logits(37, 2, 1.0, 5)
    for bad in (0.0, -1.0, float("nan"), 1e-60):
        with pytest.raises(ValueError):
            ops.sample_tokens(logits, bad, seed=1, step=0)
    with pytest.raises(ValueError):
        ops.sample_tokens(logits, 1.0, -1, seed=1, step=0)
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError):
            ops.sample_tokens(logits, 1.0, seed=1, step=bad)
    with pytest.raises(ValueError):
        ops.sample_tokens(logits[0], 1.0, seed=1, step=0)
    # fp32 logits take the same definition; top_k None, 0 and >= V mean all
    a = ops.sample_tokens(logits.float(), 0.8, None, seed=9, step=1)
    assert torch.equal(a, ops.sample_tokens(logits, 0.8, 0, seed=9, step=1))
    assert torch.equal(a, ops.sample_tokens(logits, 0.8, 37, seed=9, step=1))
    assert torch.equal(a, ref_backend.sample_tokens(logits, S.inv_t_of(0.8), 40, 9, 1))


# ---------------------------------------------------------------------------
# generate / generate_ragged
# ---------------------------------------------------------------------------
def _tiny():
    cfg = GPTConfig(block_size=16, vocab_size=37, n_layer=2, n_head=2, n_embd=16,
                    dropout=0.0)
    torch.manual_seed(23)
    return GPT(cfg).eval()


def _no_multinomial(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("torch.multinomial called on the seed= path")
    monkeypatch.setattr(torch, "multinomial", boom)


def test_generate_seeded(monkeypatch):
    model = _tiny()
    idx = torch.randint(0, 37, (3, 5), generator=torch.Generator().manual_seed(1))
    n_new = 14                               # 5 + 14 > 16: the window slides
    _no_multinomial(monkeypatch)
    out = G.generate(model, idx, n_new, temperature=0.8, top_k=6, seed=77)
    assert out.shape == (3, 5 + n_new)
    assert torch.equal(out, G.generate(model, idx, n_new, temperature=0.8, top_k=6, seed=77))
    assert not torch.equal(out, G.generate(model, idx, n_new, temperature=0.8, top_k=6, seed=78))
    # the hand loop: token t is sample_tokens(step=t) of the stepper's logits
    step = G.decode_stepper(model, 3)
    seq = idx
    logits = step(seq, 0)
    for t in range(n_new):
        nxt = ops.sample_tokens(logits, 0.8, 6, seed=77, step=t)
        seq = torch.cat([seq, nxt[:, None]], dim=1)
        logits = step(seq[:, -1:], seq.shape[1] - 1) if seq.shape[1] <= 16 \
            else step(seq[:, -16:], 0)
    assert torch.equal(out, seq)
    # greedy stays argmax whatever else is passed
    assert torch.equal(G.generate(model, idx, 4, temperature=0.0, seed=77),
                       G.generate(model, idx, 4, temperature=0.0))
    with pytest.raises(ValueError):
        G.generate(model, idx, 2, seed=1, generator=torch.Generator())


def test_generate_ragged_seeded(monkeypatch):
    model = _tiny()
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, 37, (n,), generator=g) for n in (2, 7, 13)]
    _no_multinomial(monkeypatch)
    outs = G.generate_ragged(model, prompts, 6, temperature=0.9, top_k=5, seed=31)
    assert [o.numel() - p.numel() for o, p in zip(outs, prompts)] == [6, 6, 4]
    again = G.generate_ragged(model, prompts, 6, temperature=0.9, top_k=5, seed=31)
    assert all(torch.equal(a, b) for a, b in zip(outs, again))
    # the hand loop over the ragged steps
    cache = G.KVCache(model, 3, dtype=torch.float32)
    logits = G.prefill_ragged(model, prompts, cache)
    toks = []
    for t in range(6):
        nxt = ops.sample_tokens(logits, 0.9, 5, seed=31, step=t)
        toks.append(nxt)
        if t < 5:
            logits = G.decode_step_ragged(model, nxt[:, None], cache)
    toks = torch.stack(toks, dim=1)
    for b, (o, p) in enumerate(zip(outs, prompts)):
        assert torch.equal(o[p.numel():], toks[b, :o.numel() - p.numel()]), b
    with pytest.raises(ValueError):
        G.generate_ragged(model, prompts, 2, seed=1, generator=torch.Generator())


def _sample_before(logits, temperature, top_k, generator):
    """generate._sample as it was before seed= existed, verbatim."""
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


def test_generator_path_unchanged():
    model = _tiny()
    idx = torch.randint(0, 37, (2, 4), generator=torch.Generator().manual_seed(3))
    out = G.generate(model, idx, 8, temperature=0.8, top_k=6,
                     generator=torch.Generator().manual_seed(55))
    gen = torch.Generator().manual_seed(55)
    step = G.decode_stepper(model, 2)
    seq = idx
    logits = step(seq, 0)
    for _ in range(8):
        nxt = _sample_before(logits, 0.8, 6, gen)
        seq = torch.cat([seq, nxt[:, None]], dim=1)
        logits = step(seq[:, -1:], seq.shape[1] - 1)
    assert torch.equal(out, seq)
    # and the global-RNG path
    torch.manual_seed(56)
    a = G.generate(model, idx, 8, temperature=0.8)
    torch.manual_seed(56)
    seq = idx
    logits = step(seq, 0)
    for _ in range(8):
        nxt = _sample_before(logits, 0.8, None, None)
        seq = torch.cat([seq, nxt[:, None]], dim=1)
        logits = step(seq[:, -1:], seq.shape[1] - 1)
    assert torch.equal(a, seq)
