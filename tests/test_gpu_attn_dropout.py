"""Attention dropout inside the flash kernels (fwd + dkv + dq), on the GPU:
the exact keep-mask read back from the forward kernel, numerics against the
fp32 reference with the host-mirror mask, determinism, p=0 passthrough, and
the model wiring under activation remat.

Measured on MI355X at p=0.2, seed 7, over the four shapes below (bounds
1e-3 / 2e-2 / 4e-2 are those of test_attention_fwd / test_attention_bwd):
mask mismatches 0; relative errors LSE <= 5.1e-8, O <= 2.0e-3, dq <= 2.7e-3,
dk <= 2.7e-3, dv <= 2.4e-3. Per-shape figures: profiles/attn_dropout.md."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from midgpt_amd import ops
    assert ops.have_ext(), f"HIP extension must be built: {ops._C_ERR}"

from midgpt_amd.config import GPTConfig
from midgpt_amd.models.gpt import GPT
from midgpt_amd.ops import reference as ref

DEV = "cuda:0"
P, SEED = 0.2, 7
# 4-wave path; shakespeare head geometry on the 8-wave path; C=128; more
# than one q-block per head
SHAPES = [(2, 2, 128, 64), (2, 3, 256, 64), (1, 2, 256, 128), (1, 1, 512, 128)]


def relerr(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / (b.norm() + 1e-12))


_KEEP = {}


def mirror(B, H, T, p=P, seed=SEED):
    """Host-mirror mask on the device; computed once per shape, never mutated."""
    key = (seed, B, H, T, p)
    if key not in _KEEP:
        _KEEP[key] = ref.attn_dropout_keep(seed, B, H, T, p).to(DEV)
    return _KEEP[key]


@pytest.mark.parametrize("B,H,T,C", SHAPES)
def test_forward_kernel_mask_is_the_mirror_exactly(B, H, T, C):
    """q = k = 0 makes P uniform on each row; with V[j] = e_{j mod C} inside
    column block blk (0 outside), O[i, c] > 0 iff (i, blk*C + c) is causal
    and kept. Reassembled over the T/C passes this is the kernel's mask."""
    q = torch.zeros(B, H, T, C, device=DEV, dtype=torch.bfloat16)
    got = torch.zeros(B, H, T, T, device=DEV, dtype=torch.bool)
    eye = torch.eye(C, device=DEV, dtype=torch.bfloat16)
    for blk in range(T // C):
        v = torch.zeros(B, H, T, C, device=DEV, dtype=torch.bfloat16)
        v[:, :, blk * C:(blk + 1) * C] = eye
        o, _ = ops._C.attn_fwd_dropout(q, q, v, P, SEED)
        got[..., blk * C:(blk + 1) * C] = o > 0
    tril = torch.ones(T, T, dtype=torch.bool, device=DEV).tril()
    want = mirror(B, H, T) & tril
    nbad = int((got != want).sum())
    print(f"mask mismatches {nbad} of {want.numel()}")
    assert nbad == 0


@pytest.mark.parametrize("B,H,T,C", SHAPES)
def test_forward_backward_vs_fp32_reference_with_mirror_mask(B, H, T, C):
    torch.manual_seed(4)
    q, k, v = (torch.randn(B, H, T, C, device=DEV, dtype=torch.bfloat16,
                           requires_grad=True) for _ in range(3))
    o = ops.flash_attention(q, k, v, dropout_p=P, seed=SEED)
    do = torch.randn_like(o)
    (o.float() * do.float()).sum().backward()
    _, lse = ops._C.attn_fwd_dropout(q.detach(), k.detach(), v.detach(), P, SEED)

    # fp32 reference on the same (bf16-rounded) inputs, mirror mask
    q2, k2, v2 = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    o2 = ref.causal_attention(q2, k2, v2, dropout_p=P, keep=mirror(B, H, T))
    (o2 * do.float()).sum().backward()
    s = torch.matmul(q2.detach(), k2.detach().transpose(-1, -2)) / math.sqrt(C)
    tril = torch.ones(T, T, dtype=torch.bool, device=DEV).tril()
    lse_ref = torch.logsumexp(s.masked_fill(~tril, float("-inf")), dim=-1)

    errs = {"lse": relerr(lse, lse_ref), "o": relerr(o, o2),
            "dq": relerr(q.grad, q2.grad), "dk": relerr(k.grad, k2.grad),
            "dv": relerr(v.grad, v2.grad)}
    print(f"B{B} H{H} T{T} C{C}: " +
          " ".join(f"{n}={e:.3e}" for n, e in errs.items()))
    assert errs["lse"] < 1e-3, errs   # LSE is that of the UNDROPPED softmax
    assert errs["o"] < 2e-2, errs
    assert errs["dq"] < 4e-2, errs
    assert errs["dk"] < 4e-2, errs
    assert errs["dv"] < 4e-2, errs


@pytest.mark.parametrize("B,H,T,C", [(2, 3, 256, 64), (1, 2, 256, 128)])
def test_same_seed_is_bit_identical_and_seeds_differ(B, H, T, C):
    torch.manual_seed(5)
    q, k, v, do = (torch.randn(B, H, T, C, device=DEV, dtype=torch.bfloat16)
                   for _ in range(4))
    o1, lse1 = ops._C.attn_fwd_dropout(q, k, v, P, SEED)
    o2, lse2 = ops._C.attn_fwd_dropout(q, k, v, P, SEED)
    assert torch.equal(o1, o2) and torch.equal(lse1, lse2)
    g1 = ops._C.attn_bwd_dropout(do, q, k, v, o1, lse1, P, SEED)
    g2 = ops._C.attn_bwd_dropout(do, q, k, v, o1, lse1, P, SEED)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    o3, lse3 = ops._C.attn_fwd_dropout(q, k, v, P, SEED + 1)
    assert not torch.equal(o1, o3)
    assert torch.equal(lse1, lse3)  # LSE does not see the mask
    # a seed above 2^32 reaches the key's high word
    o4, _ = ops._C.attn_fwd_dropout(q, k, v, P, SEED + (1 << 32))
    assert not torch.equal(o1, o4)


@pytest.mark.parametrize("B,H,T,C", [(2, 2, 128, 64), (1, 2, 256, 128)])
def test_p_zero_is_todays_path_bit_for_bit(B, H, T, C):
    torch.manual_seed(6)
    q, k, v = (torch.randn(B, H, T, C, device=DEV, dtype=torch.bfloat16,
                           requires_grad=True) for _ in range(3))
    o = ops.flash_attention(q, k, v, dropout_p=0.0, seed=SEED)
    do = torch.randn_like(o)
    o.backward(do)
    o_ref, lse_ref = ops._C.attn_fwd(q.detach(), k.detach(), v.detach())
    dq, dk, dv = ops._C.attn_bwd(do, q.detach(), k.detach(), v.detach(),
                                 o_ref, lse_ref)
    assert torch.equal(o.detach(), o_ref)
    assert torch.equal(q.grad, dq)
    assert torch.equal(k.grad, dk)
    assert torch.equal(v.grad, dv)


def test_binding_rejects_bad_p():
    q = torch.zeros(1, 1, 128, 64, device=DEV, dtype=torch.bfloat16)
    for bad in (0.0, 1.0, -0.5):
        with pytest.raises(RuntimeError):
            ops._C.attn_fwd_dropout(q, q, q, bad, SEED)


# ---------------------------------------------------------------------------
# Model on GPU
# ---------------------------------------------------------------------------
DROP_CFG = GPTConfig(block_size=128, vocab_size=512, n_layer=2, n_head=2,
                     n_embd=128, dropout=0.2)


def _gpu_model_run(state, remat):
    gm = GPT(DROP_CFG)
    gm.load_state_dict(state)
    gm = gm.to("cuda").to(torch.bfloat16)
    gm.rope_sin = gm.rope_sin.float()
    gm.rope_cos = gm.rope_cos.float()
    gm.train()
    gm.remat = remat
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, 512, (2, 128), generator=g).cuda()
    y = torch.randint(0, 512, (2, 128), generator=g).cuda()
    torch.manual_seed(0)
    loss = gm.loss(x, y)
    loss.backward()
    return float(loss.detach()), {n: p.grad.detach().clone()
                                  for n, p in gm.named_parameters()}


def test_model_gpu_dropout_in_kernel_and_remat_bit_identical(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("materialized attention reached with dropout > 0")
    monkeypatch.setattr(ref, "causal_attention", boom)
    monkeypatch.delenv("MIDGPT_ATTN_DROPOUT_REF", raising=False)
    torch.manual_seed(0)
    state = GPT(DROP_CFG).state_dict()
    loss_a, ga = _gpu_model_run(state, remat=False)
    assert math.isfinite(loss_a), loss_a
    loss_b, gb = _gpu_model_run(state, remat=True)
    diffs = {n: float((ga[n].float() - gb[n].float()).abs().max()) for n in ga}
    print(f"loss {loss_a} / {loss_b}; max |grad diff| "
          f"{max(diffs.values()):.3e} ({[n for n, d in diffs.items() if d > 0]})")
    assert math.isfinite(loss_b), loss_b
    for n in ga:
        assert torch.isfinite(ga[n].float()).all(), n
        assert torch.equal(ga[n], gb[n]), (n, diffs[n])
