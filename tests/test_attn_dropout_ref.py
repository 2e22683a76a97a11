"""Attention dropout, CPU side: the Philox host mirror (known answers,
statistics), ops.flash_attention(dropout_p=...) on the CPU branch against
the materialized reference with the mirror mask, determinism, passthrough,
and the model wiring (no materialized fallback, remat replay)."""
import math

import numpy as np
import pytest
import torch

from midgpt_amd import ops
from midgpt_amd.config import GPTConfig
from midgpt_amd.models.gpt import GPT
from midgpt_amd.ops import reference as ref


# ---------------------------------------------------------------------------
# Philox4x32-10 known answers (Random123 kat_vectors: zeros, all-ones, pi)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,expect", [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, expect):
    c = [np.array([x], dtype=np.uint64) for x in ctr]
    out = ref._philox4x32_10(*c, key[0], key[1])
    assert tuple(int(w[0]) for w in out) == expect


def test_mirror_layout_matches_definition():
    """Element (bh, q, k) takes word q&3 of counter (k, q>>2, bh, 0), key =
    (seed lo, seed hi), kept iff word >= (uint32)(p * 2^32)."""
    seed, B, H, T, p = (0x1234567 << 32) | 0x89abcdef, 2, 3, 12, 0.3
    keep = ref.attn_dropout_keep(seed, B, H, T, p)
    assert keep.shape == (B, H, T, T) and keep.dtype == torch.bool
    thr = int(p * 2 ** 32)
    for (b, h, q, k) in [(0, 0, 0, 0), (1, 2, 11, 5), (0, 1, 6, 11), (1, 0, 3, 3)]:
        c = [np.array([x], dtype=np.uint64) for x in (k, q >> 2, b * H + h, 0)]
        w = ref._philox4x32_10(*c, seed & 0xffffffff, seed >> 32)[q & 3]
        assert bool(keep[b, h, q, k]) == (int(w[0]) >= thr)


# ---------------------------------------------------------------------------
# Mirror statistics: B=2, H=2, T=256 over the causal entries
# ---------------------------------------------------------------------------
B_, H_, T_ = 2, 2, 256
N_CAUSAL = B_ * H_ * T_ * (T_ + 1) // 2  # 131 584


def _corr(a, b, valid):
    a = a[valid].double()
    b = b[valid].double()
    a = a - a.mean()
    b = b - b.mean()
    return float((a * b).sum() / (a.norm() * b.norm()))


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_mirror_keep_rate(p):
    keep = ref.attn_dropout_keep(11, B_, H_, T_, p)
    tril = torch.ones(T_, T_, dtype=torch.bool).tril().expand(B_, H_, T_, T_)
    assert int(tril.sum()) == N_CAUSAL
    rate = float(keep[tril].double().mean())
    bound = 5 * math.sqrt(p * (1 - p) / N_CAUSAL)
    print(f"p={p}: keep rate {rate:.5f} (bound +-{bound:.5f})")
    assert abs(rate - (1 - p)) < bound, rate


def test_mirror_keep_decorrelated():
    p = 0.2
    keep = ref.attn_dropout_keep(11, B_, H_, T_, p)
    keep2 = ref.attn_dropout_keep(12, B_, H_, T_, p)
    tril = torch.ones(T_, T_, dtype=torch.bool).tril().expand(B_, H_, T_, T_)
    bound = 5 / math.sqrt(N_CAUSAL)
    pairs = {
        "k,k+1": (keep[..., :, :-1], keep[..., :, 1:],
                  tril[..., :, :-1] & tril[..., :, 1:]),
        "q,q+1": (keep[..., :-1, :], keep[..., 1:, :],
                  tril[..., :-1, :] & tril[..., 1:, :]),
        "h,h+1": (keep[:, :-1], keep[:, 1:], tril[:, :-1]),
        "seed,seed+1": (keep, keep2, tril),
    }
    for name, (a, b, valid) in pairs.items():
        c = _corr(a, b, valid)
        print(f"corr {name}: {c:+.5f} (bound {bound:.5f})")
        assert abs(c) < bound, (name, c)


# ---------------------------------------------------------------------------
# CPU ops.flash_attention(dropout_p=0.2, seed=7) vs reference + mirror mask
# ---------------------------------------------------------------------------
SHAPE = (2, 2, 64, 16)


def _qkv(seed=0, requires_grad=False):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*SHAPE, generator=g).requires_grad_(requires_grad)
            for _ in range(3)]


def test_cpu_forward_backward_match_reference_with_mirror():
    B, H, T, C = SHAPE
    p, seed = 0.2, 7
    q, k, v = _qkv(0, True)
    o = ops.flash_attention(q, k, v, dropout_p=p, seed=seed)
    do = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(1))
    (o * do).sum().backward()

    keep = ref.attn_dropout_keep(seed, B, H, T, p)
    assert not bool(keep.all()) and bool(keep.any())
    q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o2 = ref.causal_attention(q2, k2, v2, dropout_p=p, keep=keep)
    (o2 * do).sum().backward()
    # fp32 round-off only: same math, different association
    assert torch.allclose(o, o2, rtol=1e-5, atol=1e-6), float((o - o2).abs().max())
    for name, a, b in [("dq", q.grad, q2.grad), ("dk", k.grad, k2.grad),
                       ("dv", v.grad, v2.grad)]:
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5), \
            (name, float((a - b).abs().max()))


def test_reference_default_unchanged_by_keep_argument():
    q, k, v = _qkv(2)
    a = ref.causal_attention(q, k, v)
    b = ref.causal_attention(q, k, v, 0.2, False)  # training=False: no dropout
    assert torch.equal(a, b)


def test_cpu_determinism_and_passthrough():
    q, k, v = _qkv(3)
    a = ops.flash_attention(q, k, v, dropout_p=0.2, seed=7)
    b = ops.flash_attention(q, k, v, dropout_p=0.2, seed=7)
    c = ops.flash_attention(q, k, v, dropout_p=0.2, seed=8)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    base = ops.flash_attention(q, k, v)
    assert torch.equal(ops.flash_attention(q, k, v, dropout_p=0.0), base)
    assert torch.equal(ops.flash_attention(q, k, v, 0.0, 123), base)
    assert not torch.equal(a, base)


def test_seed_drawn_from_cpu_generator_is_reproducible():
    q, k, v = _qkv(4)
    torch.manual_seed(5)
    a1 = ops.flash_attention(q, k, v, dropout_p=0.2)
    a2 = ops.flash_attention(q, k, v, dropout_p=0.2)  # next draw: new mask
    torch.manual_seed(5)
    b1 = ops.flash_attention(q, k, v, dropout_p=0.2)
    assert torch.equal(a1, b1)
    assert not torch.equal(a1, a2)


def test_dropout_p_out_of_range_raises():
    q, k, v = _qkv(4)
    with pytest.raises(ValueError):
        ops.flash_attention(q, k, v, dropout_p=1.0, seed=1)
    with pytest.raises(ValueError):
        ops.flash_attention(q, k, v, dropout_p=-0.1, seed=1)


# ---------------------------------------------------------------------------
# Model level
# ---------------------------------------------------------------------------
TINY_DROP = GPTConfig(block_size=16, vocab_size=37, n_layer=2, n_head=2,
                      n_embd=32, dropout=0.2)


def _model_run(remat, state=None):
    torch.manual_seed(0)
    model = GPT(TINY_DROP)
    if state is not None:
        model.load_state_dict(state)
    model.train()
    model.remat = remat
    g = torch.Generator().manual_seed(9)
    x = torch.randint(0, 37, (3, 16), generator=g)
    y = torch.randint(0, 37, (3, 16), generator=g)
    torch.manual_seed(0)
    loss = model.loss(x, y)
    loss.backward()
    return model, float(loss.detach()), {n: p.grad.clone()
                                         for n, p in model.named_parameters()}


def test_model_dropout_uses_flash_path_and_remat_replays(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("materialized attention reached with dropout > 0")
    monkeypatch.setattr(ref, "causal_attention", boom)
    monkeypatch.delenv("MIDGPT_ATTN_DROPOUT_REF", raising=False)

    model, loss1, g1 = _model_run(remat=False)
    assert math.isfinite(loss1)
    _, loss2, g2 = _model_run(remat=False, state=model.state_dict())
    assert loss1 == loss2
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    # activation remat replays the same seeds (checkpoint preserves RNG state)
    _, loss3, g3 = _model_run(remat=True, state=model.state_dict())
    assert loss3 == loss1
    for n in g1:
        assert torch.allclose(g1[n], g3[n], rtol=1e-5, atol=1e-7), \
            (n, float((g1[n] - g3[n]).abs().max()))

    # dropout is really on: eval() (p=0 path) gives a different loss
    model.eval()
    g = torch.Generator().manual_seed(9)
    x = torch.randint(0, 37, (3, 16), generator=g)
    y = torch.randint(0, 37, (3, 16), generator=g)
    assert float(model.loss(x, y).detach()) != loss1
