"""CPU: ops.add_rmsnorm / ops.qkv_attention are exactly the compositions they
stand for off the GPU, and the model computes the same loss and gradients
with the fused routing as with MIDGPT_GLUE_UNFUSED=1."""

import pytest
import torch

from midgpt_amd import ops
from midgpt_amd.config import GPTConfig
from midgpt_amd.models.gpt import GPT
from midgpt_amd.ops import reference as ref


def test_add_rmsnorm_cpu_is_add_then_rmsnorm():
    torch.manual_seed(0)
    x, r = torch.randn(2, 5, 24), torch.randn(2, 5, 24)
    gs, gy = torch.randn(2, 5, 24), torch.randn(2, 5, 24)
    xa, ra = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    s, y = ops.add_rmsnorm(xa, ra, 1e-5)
    torch.autograd.backward([s, y], [gs, gy])
    xb, rb = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    s2 = xb + rb
    y2 = ops.rmsnorm(s2, None, 1e-5)
    torch.autograd.backward([s2, y2], [gs, gy])
    assert torch.equal(s, s2) and torch.equal(y, y2)
    assert torch.equal(xa.grad, xb.grad) and torch.equal(ra.grad, rb.grad)


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_qkv_attention_cpu_is_prep_attention_transpose(p):
    torch.manual_seed(1)
    B, T, H, C = 2, 12, 3, 8
    qkv = torch.randn(B, T, 3, H, C)
    qw, kw = torch.randn(C), torch.randn(C)
    sin, cos = ref.rope_tables(C, T)
    go = torch.randn(B, T, H * C)

    def grads(fn):
        a = [t.clone().requires_grad_(True) for t in (qkv, qw, kw)]
        o = fn(*a)
        o.backward(go)
        return [o.detach()] + [t.grad for t in a]

    def fused(a, b, c):
        return ops.qkv_attention(a, b, c, sin, cos, p, 1234)

    def composed(a, b, c):
        q, k, v = ops.qkv_prep(a, b, c, sin, cos)
        o = ops.flash_attention(q, k, v, p, 1234)
        return o.transpose(1, 2).reshape(B, T, H * C)

    for name, g, w in zip(("o", "dqkv", "dqw", "dkw"), grads(fused), grads(composed)):
        assert torch.equal(g, w), name


def test_qkv_attention_draws_seed_like_flash_attention():
    torch.manual_seed(2)
    B, T, H, C = 1, 8, 2, 8
    qkv = torch.randn(B, T, 3, H, C)
    w = torch.ones(C)
    sin, cos = ref.rope_tables(C, T)
    torch.manual_seed(5)
    a = ops.qkv_attention(qkv, w, w, sin, cos, 0.5)
    torch.manual_seed(5)
    q, k, v = ops.qkv_prep(qkv, w, w, sin, cos)
    b = ops.flash_attention(q, k, v, 0.5).transpose(1, 2).reshape(B, T, H * C)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        ops.qkv_attention(qkv, w, w, sin, cos, 1.0)


def _run(cfg, remat, fused, monkeypatch):
    if fused:
        monkeypatch.delenv("MIDGPT_GLUE_UNFUSED", raising=False)
    else:
        monkeypatch.setenv("MIDGPT_GLUE_UNFUSED", "1")
    torch.manual_seed(0)
    model = GPT(cfg)
    model.remat = remat
    model.train()
    x = torch.randint(0, cfg.vocab_size, (2, cfg.block_size))
    y = torch.randint(0, cfg.vocab_size, (2, cfg.block_size))
    torch.manual_seed(7)
    loss = model.loss(x, y)
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in model.named_parameters()}


@pytest.mark.parametrize("remat,dropout", [(False, 0.0), (True, 0.0), (False, 0.1),
                                           (True, 0.1)])
def test_model_cpu_fused_routing_equals_unfused(monkeypatch, remat, dropout):
    cfg = GPTConfig(block_size=16, vocab_size=64, n_layer=3, n_head=2, n_embd=32,
                    dropout=dropout)
    loss_f, grads_f = _run(cfg, remat, True, monkeypatch)
    loss_u, grads_u = _run(cfg, remat, False, monkeypatch)
    assert torch.equal(loss_f, loss_u)
    assert grads_f.keys() == grads_u.keys()
    for n in grads_u:
        assert torch.equal(grads_f[n], grads_u[n]), n


def test_model_without_blocks_and_eval_path(monkeypatch):
    cfg = GPTConfig(block_size=8, vocab_size=32, n_layer=0, n_head=2, n_embd=16,
                    dropout=0.0)
    torch.manual_seed(0)
    model = GPT(cfg).eval()
    idx = torch.randint(0, 32, (1, 8))
    monkeypatch.delenv("MIDGPT_GLUE_UNFUSED", raising=False)
    a = model(idx)
    monkeypatch.setenv("MIDGPT_GLUE_UNFUSED", "1")
    assert torch.equal(a, model(idx))
