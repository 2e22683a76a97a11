"""GPU: the copy-free attention path (strided O/dO/V/dV, Q/K-only prep) and
the fused residual-add + RMSNorm kernels against the kernels they replace.

The arithmetic is unchanged and only addresses (or the number of passes)
move, so the criterion is torch.equal against the existing entry points fed
explicit copies, not a tolerance. Every reference is computed twice: should
the existing path itself not repeat bit for bit on identical inputs, the new
path's difference from it is bounded by that existing-vs-existing difference
instead (``same``)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from midgpt_amd import ops
    assert ops.have_ext()

from midgpt_amd.config import GPTConfig
from midgpt_amd.models.gpt import GPT
from midgpt_amd.ops import reference as ref
from test_gpu_model import SMALL

DEV = "cuda"
BF = torch.bfloat16
SENTINEL = -77.0          # exact in bf16
SEED = 0x1234_5678_9ABC


def randbf(*shape):
    return torch.randn(*shape, device=DEV).to(BF)


def same(name, got, want, want_again):
    """got == want bit for bit; if the reference does not repeat itself,
    |got - want| <= |want - want_again| (max-abs) instead."""
    assert got.shape == want.shape and got.dtype == want.dtype, name
    if torch.equal(want, want_again):
        assert torch.equal(got, want), name
        return
    noise = float((want.float() - want_again.float()).abs().max())
    diff = float((got.float() - want.float()).abs().max())
    print(f"{name}: reference repeats only to {noise:.3e}; new differs by {diff:.3e}")
    assert diff <= noise, (name, diff, noise)


def _qkv_inputs(B, T, H, C):
    qkv = randbf(B, T, 3, H, C)
    qw = torch.randn(C, device=DEV)
    kw = torch.randn(C, device=DEV)
    sin, cos = ref.rope_tables(C, T, device=DEV)
    return qkv, qw, kw, sin, cos


# ---------------------------------------------------------------------------
# Copy-free attention layouts: O/dO as (B,T,H,C), dV into slot 2 of dqkv, and
# V either as the (B,H,T,C) copy or read in place from slot 2 of qkv; dO
# either re-laid out by the delta kernel (stage_do) or read in place.
# ---------------------------------------------------------------------------
def _old_attention(q, k, v, do_bhtc, p):
    if p > 0.0:
        o, lse = ops._C.attn_fwd_dropout(q, k, v, p, SEED)
        dq, dk, dv = ops._C.attn_bwd_dropout(do_bhtc, q, k, v, o, lse, p, SEED)
    else:
        o, lse = ops._C.attn_fwd(q, k, v)
        dq, dk, dv = ops._C.attn_bwd(do_bhtc, q, k, v, o, lse)
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("packed_v,stage_do", [(False, True), (True, False)])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("C", [64, 128])
# NW=4 one block, NW=8 one block, NW=4 several, NW=8 several (q0 > 0)
@pytest.mark.parametrize("T", [128, 256, 384, 512])
def test_packed_attention_equals_contiguous(T, C, p, packed_v, stage_do):
    B, H = 2, 3                                   # odd H: catches b/h stride mix-ups
    torch.manual_seed(T + C)
    qkv, qw, kw, sin, cos = _qkv_inputs(B, T, H, C)
    q, k, v, qs, ks = ops._C.qkv_prep_fwd(qkv, qw, kw, sin, cos, 1e-6)
    do = randbf(B, T, H, C)                       # the layout c_proj's backward gives
    do_bhtc = do.transpose(1, 2).contiguous()

    want = _old_attention(q, k, v, do_bhtc, p)
    again = _old_attention(q, k, v, do_bhtc, p)
    o_w, lse_w, dq_w, dk_w, dv_w = want

    vin = qkv if packed_v else v
    o, lse = ops._C.attn_fwd_packed(q, k, vin, p, SEED)
    assert o.shape == (B, T, H, C) and o.is_contiguous()
    same("o", o, o_w.transpose(1, 2).contiguous(), again[0].transpose(1, 2).contiguous())
    same("lse", lse, lse_w, again[1])

    dqkv = torch.full_like(qkv, SENTINEL)
    # o_w in the new layout, so that only the backward kernels are compared
    dq, dk = ops._C.attn_bwd_packed(do, q, k, vin, o_w.transpose(1, 2).contiguous(),
                                    lse_w, dqkv, p, SEED, stage_do)
    same("dq", dq, dq_w, again[2])
    same("dk", dk, dk_w, again[3])
    same("dv", dqkv[:, :, 2].contiguous(), dv_w.permute(0, 2, 1, 3).contiguous(),
         again[4].permute(0, 2, 1, 3).contiguous())
    assert bool((dqkv[:, :, :2] == SENTINEL).all()), "attention bwd wrote slots 0/1"

    # the Q/K prep backward then fills slots 0 and 1 and leaves slot 2 alone
    dqw, dkw = ops._C.qk_prep_bwd(dq_w, dk_w, qkv, qw, kw, sin, cos, qs, ks, dqkv)
    dqkv_w, dqw_w, dkw_w = ops._C.qkv_prep_bwd(dq_w, dk_w, dv_w, qkv, qw, kw, sin, cos,
                                               qs, ks, 1e-6)
    dqkv_a, dqw_a, dkw_a = ops._C.qkv_prep_bwd(dq_w, dk_w, dv_w, qkv, qw, kw, sin, cos,
                                               qs, ks, 1e-6)
    same("dqkv slots 0,1", dqkv[:, :, :2].contiguous(), dqkv_w[:, :, :2].contiguous(),
         dqkv_a[:, :, :2].contiguous())
    same("dqw", dqw, dqw_w, dqw_a)
    same("dkw", dkw, dkw_w, dkw_a)
    if torch.equal(dv_w, again[4]):
        assert torch.equal(dqkv, dqkv_w)


def test_packed_attention_rejects_wrong_shapes():
    B, T, H, C = 1, 128, 2, 64
    qkv, qw, kw, sin, cos = _qkv_inputs(B, T, H, C)
    q, k, _, _ = ops._C.qk_prep_fwd(qkv, qw, kw, sin, cos, 1e-6)
    o, lse = ops._C.attn_fwd_packed(q, k, qkv)
    with pytest.raises(RuntimeError):             # (B,H,T,C) where (B,T,H,C) is due
        ops._C.attn_bwd_packed(o.transpose(1, 2).contiguous(), q, k, qkv, o, lse,
                               torch.empty_like(qkv))
    with pytest.raises(RuntimeError):             # qkv of another batch size
        ops._C.attn_fwd_packed(q, k, randbf(B + 1, T, 3, H, C))
    with pytest.raises(RuntimeError):             # v that is neither layout
        ops._C.attn_fwd_packed(q, k, randbf(B, T, H, C))
    with pytest.raises(RuntimeError):             # dqkv not shaped like qkv
        ops._C.attn_bwd_packed(o, q, k, qkv, o, lse, randbf(B, T, 3, H, C // 2))

    # the plain (B,H,T,C) entry points run the same checks
    B, H, T, C = 1, 1, 128, 64
    q, k, v, do = (randbf(B, H, T, C) for _ in range(4))
    o, lse = ops._C.attn_fwd(q, k, v)
    with pytest.raises(RuntimeError):             # k of another length
        ops._C.attn_bwd(do, q, randbf(1, 1, 256, 64), v, o, lse)
    with pytest.raises(RuntimeError):             # fp32 v
        ops._C.attn_bwd(do, q, k, v.float(), o, lse)
    with pytest.raises(RuntimeError):             # lse of the wrong length
        ops._C.attn_bwd(do, q, k, v, o, lse[..., :-1].contiguous())
    with pytest.raises(RuntimeError):             # k of another length
        ops._C.attn_fwd(q, randbf(1, 1, 256, 64), v)
    qkv, qw, kw, sin, cos = _qkv_inputs(B, T, H, C)
    with pytest.raises(RuntimeError):             # sin one row short
        ops._C.qkv_prep_fwd(qkv, qw, kw, sin[:T - 1].contiguous(), cos, 1e-6)
    torch.cuda.synchronize()                      # nothing was launched: no fault to report


# ---------------------------------------------------------------------------
# Q/K-only prep (no T constraint; 131 rows/head: not a multiple of rows/wave)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("T", [128, 131])
def test_qk_prep_equals_qkv_prep(T, C):
    B, H = 2, 3
    torch.manual_seed(T * C)
    qkv, qw, kw, sin, cos = _qkv_inputs(B, T, H, C)
    q_w, k_w, _, qs_w, ks_w = ops._C.qkv_prep_fwd(qkv, qw, kw, sin, cos, 1e-6)
    q, k, qs, ks = ops._C.qk_prep_fwd(qkv, qw, kw, sin, cos, 1e-6)
    for name, a, b in (("q", q, q_w), ("k", k, k_w), ("qstats", qs, qs_w),
                       ("kstats", ks, ks_w)):
        assert torch.equal(a, b), name
    dq, dk, dv = randbf(B, H, T, C), randbf(B, H, T, C), randbf(B, H, T, C)
    ref1 = ops._C.qkv_prep_bwd(dq, dk, dv, qkv, qw, kw, sin, cos, qs, ks, 1e-6)
    ref2 = ops._C.qkv_prep_bwd(dq, dk, dv, qkv, qw, kw, sin, cos, qs, ks, 1e-6)
    dqkv = torch.full_like(qkv, SENTINEL)
    dqw, dkw = ops._C.qk_prep_bwd(dq, dk, qkv, qw, kw, sin, cos, qs, ks, dqkv)
    same("dqkv slots 0,1", dqkv[:, :, :2].contiguous(), ref1[0][:, :, :2].contiguous(),
         ref2[0][:, :, :2].contiguous())
    assert bool((dqkv[:, :, 2] == SENTINEL).all()), "prep bwd wrote slot 2"
    same("dqw", dqw, ref1[1], ref2[1])
    same("dkw", dkw, ref1[2], ref2[2])


# ---------------------------------------------------------------------------
# Fused residual add + RMSNorm. The launch is one wave per row, 4 rows per
# block, at most 8192 blocks: 32773 rows take a second grid-stride trip with
# a ragged last block. D = 8: one active lane; 136: a partial sweep; 2048 and
# 4096: the row held in registers (4 and 8 sweeps); 4104: the re-read path.
# ---------------------------------------------------------------------------
ADDNORM_CASES = [(N, D) for N in (1, 5, 1021, 32773) for D in (8, 136, 2048)] + \
                [(5, 4096), (5, 4104)]


@pytest.mark.parametrize("N,D", ADDNORM_CASES)
def test_add_rmsnorm_equals_add_then_norm(N, D):
    torch.manual_seed(N + D)
    x, r = randbf(N, D), randbf(N, D)
    x[0] = 0.0
    r[0] = 0.0                                    # zero row: eps keeps it finite
    if N > 1:
        x[1] *= 1e3
    eps = 1e-6
    s_w = x + r
    y_w, inv_w = ops._C.rmsnorm_fwd(s_w, None, eps)
    s, y, inv = ops._C.add_rmsnorm_fwd(x, r, eps)
    assert torch.equal(s, s_w), "s"
    assert torch.equal(inv, inv_w), "invrms"
    assert torch.equal(y, y_w), "y"

    dy, ds = randbf(N, D), randbf(N, D)
    dn_w, _ = ops._C.rmsnorm_bwd(dy, s_w, None, inv_w, eps)
    dx = ops._C.add_rmsnorm_bwd(ds, dy, s, inv)
    assert torch.equal(dx, ds + dn_w), "dx"
    dx0 = ops._C.add_rmsnorm_bwd(None, dy, s, inv)
    assert torch.equal(dx0, dn_w), "dx without ds"


def test_add_rmsnorm_autograd_wrapper(monkeypatch):
    torch.manual_seed(9)
    x, r = randbf(3, 7, 136), randbf(3, 7, 136)
    gs, gy = randbf(3, 7, 136), randbf(3, 7, 136)

    def run(use_s):
        xa, ra = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
        s, y = ops.add_rmsnorm(xa, ra, 1e-5)
        if use_s:
            torch.autograd.backward([s, y], [gs, gy])
        else:
            y.backward(gy)
        return s.detach(), y.detach(), xa.grad, ra.grad

    for use_s in (True, False):
        monkeypatch.delenv("MIDGPT_GLUE_UNFUSED", raising=False)
        got = run(use_s)
        monkeypatch.setenv("MIDGPT_GLUE_UNFUSED", "1")
        want = run(use_s)
        for name, a, b in zip(("s", "y", "dx", "dr"), got, want):
            assert torch.equal(a, b), (name, use_s)

    # other dtypes and widths take the composition, on the GPU too
    monkeypatch.delenv("MIDGPT_GLUE_UNFUSED", raising=False)
    xf = torch.randn(4, 100, device=DEV)
    s, y = ops.add_rmsnorm(xf, xf, 1e-6)
    assert torch.equal(s, xf + xf) and torch.equal(y, ops.rmsnorm(xf + xf, None, 1e-6))


def test_add_rmsnorm_rejects_unsupported():
    with pytest.raises(RuntimeError):
        ops._C.add_rmsnorm_fwd(randbf(4, 65), randbf(4, 65), 1e-6)
    with pytest.raises(RuntimeError):
        ops._C.add_rmsnorm_fwd(randbf(4, 64), randbf(5, 64), 1e-6)
    with pytest.raises(RuntimeError):
        ops._C.add_rmsnorm_fwd(randbf(4, 64).float(), randbf(4, 64).float(), 1e-6)


# ---------------------------------------------------------------------------
# Whole model: fused routing vs MIDGPT_GLUE_UNFUSED=1
# ---------------------------------------------------------------------------
def _model_run(cfg, remat, seed):
    """One forward and backward. The loss is taken exactly as ``GPT.loss``
    takes it, but through the logits of that same forward, which are
    returned too."""
    torch.manual_seed(0)
    model = GPT(cfg).to(DEV).to(BF)
    model.rope_sin = model.rope_sin.float()
    model.rope_cos = model.rope_cos.float()
    model.remat = remat
    model.train()
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (2, cfg.block_size), generator=g).to(DEV)
    y = torch.randint(0, cfg.vocab_size, (2, cfg.block_size), generator=g).to(DEV)
    torch.manual_seed(seed)                       # dropout masks and attention seeds
    logits = model(x)
    loss = ops.cross_entropy(logits.reshape(-1, logits.shape[-1]), y.reshape(-1))
    loss.backward()
    out = {"logits": logits.detach(), "loss": loss.detach().reshape(1)}
    out.update({n: p.grad.detach() for n, p in model.named_parameters()})
    return out, y


def _fixed_order_loss(logits, y):
    """Mean cross-entropy summed in one fixed order (no atomics)."""
    lf = logits.reshape(-1, logits.shape[-1]).double()
    return (torch.logsumexp(lf, -1) - lf.gather(1, y.reshape(-1, 1)).squeeze(1)).cpu().sum()


@pytest.mark.parametrize("remat,dropout,inplace", [(False, 0.0, False), (True, 0.0, False),
                                                   (False, 0.1, False), (False, 0.0, True)])
def test_model_fused_equals_unfused(monkeypatch, remat, dropout, inplace):
    """inplace: the variant that reads V where it lies."""
    cfg = GPTConfig(block_size=SMALL.block_size, vocab_size=SMALL.vocab_size,
                    n_layer=SMALL.n_layer, n_head=SMALL.n_head,
                    n_embd=SMALL.n_embd, dropout=dropout)
    monkeypatch.setenv("MIDGPT_GLUE_UNFUSED", "1")
    want, y = _model_run(cfg, remat, 7)
    again, _ = _model_run(cfg, remat, 7)
    monkeypatch.delenv("MIDGPT_GLUE_UNFUSED")
    if inplace:
        monkeypatch.setenv("MIDGPT_ATTN_PACKED_V", "1")
    got, _ = _model_run(cfg, remat, 7)
    assert got.keys() == want.keys()
    for name in want:
        if name != "loss":                        # logits of the loss's own forward included
            same(name, got[name], want[name], again[name])
    # The loss. Summed in a fixed order from those logits it is equal outright.
    assert torch.equal(_fixed_order_loss(got["logits"], y),
                       _fixed_order_loss(want["logits"], y))
    # What the model returns is the cross-entropy kernel's sum over the rows
    # with float atomics, which does not repeat bit for bit on identical
    # input. It is held to the existing-vs-existing difference measured here:
    # the spread of that kernel's loss over repeated runs on the unfused
    # path's logits (the two whole unfused runs included).
    if not torch.equal(got["loss"], want["loss"]):
        lg = want["logits"].reshape(-1, want["logits"].shape[-1])
        reps = [float(ops.cross_entropy(lg, y.reshape(-1))) for _ in range(64)]
        reps += [float(want["loss"]), float(again["loss"])]
        noise = max(reps) - min(reps)
        diff = abs(float(got["loss"]) - float(want["loss"]))
        print(f"loss: new-vs-unfused {diff:.3e}, unfused-vs-unfused spread {noise:.3e}")
        assert diff <= noise, (diff, noise)
