"""CPU self-check of the kernel-edge metric (kernel_edge_util): the clean CPU
reference path of midgpt_amd.ops passes every new check, and each planted
fault below is caught by the new check -- where it is true, while the suite's
older whole-tensor bound would have let it through."""
import math

import torch

import kernel_edge_util as U
from midgpt_amd import ops

BF = torch.bfloat16


def _names(bad):
    return {f.name for f in bad}


# ---------------------------------------------------------------------------
def _ce_case():
    """The distribution of test_cross_entropy_fwd_bwd (V=50304, randn*2)."""
    torch.manual_seed(6)
    N, V = 32, 50304
    logits = (torch.randn(N, V) * 2).to(BF).requires_grad_(True)
    targets = torch.randint(0, V, (N,))
    loss = ops.cross_entropy(logits, targets)
    (loss * 3.5).backward()
    lse = torch.logsumexp(logits.detach().float(), dim=-1)
    return logits.detach(), targets, lse, loss.detach(), logits.grad


def test_ce_clean_passes_and_halved_softmax_is_caught():
    logits, targets, lse, loss, d = _ce_case()
    N, V = logits.shape
    assert not U.report("cpu ce clean", U.ce_figures(logits, targets, 3.5, lse, loss, d))

    # plant: the softmax part of dlogits scaled by 0.5, the one-hot part kept
    gs = 3.5 / N
    onehot = torch.zeros(N, V).scatter_(1, targets[:, None], 1.0)
    soft = d.float() + onehot * gs
    planted = (0.5 * soft - onehot * gs).to(BF)
    _, _, d32 = U.ce_math(logits, targets, 3.5, torch.float32)
    old = U.whole_relerr(planted, d32)
    print(f"old whole-tensor relerr of the planted fault: {old:.4f} (bound 2e-2)")
    assert old < 2e-2                      # the old check passes it
    bad = U.report("cpu ce halved", U.ce_figures(logits, targets, 3.5, lse, loss, planted))
    assert "ce.dlogits_offtarget" in _names(bad)


def test_ce_wrong_lse_row_is_caught():
    logits, targets, lse, loss, d = _ce_case()
    lse = lse.clone()
    lse[5] += 1e-3                          # 1e-4 relative: invisible in the mean loss
    bad = U.report("cpu ce lse", U.ce_figures(logits, targets, 3.5, lse, loss, d))
    assert "ce.lse" in _names(bad)


# ---------------------------------------------------------------------------
def _attn_case():
    torch.manual_seed(4)
    B, H, T, C = 1, 2, 1024, 64
    q, k, v = (torch.randn(B, H, T, C).to(BF) for _ in range(3))
    o = ops.flash_attention(q, k, v)
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) / math.sqrt(C)
    tril = torch.ones(T, T, dtype=torch.bool).tril()
    s = s.masked_fill(~tril, float("-inf"))
    o32 = torch.matmul(torch.softmax(s, -1), v.float())
    return q, k, v, o, s, o32


def test_attention_clean_passes_and_one_row_mask_off_by_one_is_caught():
    """Row 40 of one head also sees key 41. One extra key among t+1 moves a
    row by about 1/sqrt(t), so the early rows are where a mask off-by-one
    shows; late rows approach the rounding noise of any metric (the GPU file
    checks causality exactly, bit for bit, instead)."""
    q, k, v, o, s, o32 = _attn_case()
    assert not U.report("cpu attn clean", U.attn_figures(q, k, v, None, {"o": o}))
    C = q.shape[-1]
    i = 40
    srow = (q[0, 1, i].float() @ k[0, 1, :i + 2].float().t()) / math.sqrt(C)
    planted = o.clone()
    planted[0, 1, i] = (torch.softmax(srow, -1).to(BF).float() @ v[0, 1, :i + 2].float()).to(BF)
    old = U.whole_relerr(planted, o32)
    print(f"old whole-tensor relerr of the planted fault: {old:.4f} (bound 2e-2)")
    assert old < 2e-2
    bad = U.report("cpu attn mask", U.attn_figures(q, k, v, None, {"o": planted}))
    assert "attn.o" in _names(bad)


def test_attention_zeroed_output_tile_is_caught():
    q, k, v, o, s, o32 = _attn_case()
    planted = o.clone()
    planted[0, 0, 512:544] = 0              # one 32-row q tile never written
    print(f"old whole-tensor relerr of the planted fault: "
          f"{U.whole_relerr(planted, o32):.4f} (bound 2e-2)")
    bad = U.report("cpu attn tile", U.attn_figures(q, k, v, None, {"o": planted}))
    assert "attn.o" in _names(bad)


def test_attention_backward_clean_passes():
    torch.manual_seed(5)
    B, H, T, C = 1, 1, 256, 64
    q, k, v = (torch.randn(B, H, T, C).to(BF).requires_grad_(True) for _ in range(3))
    o = ops.flash_attention(q, k, v)
    do = torch.randn(B, H, T, C).to(BF)
    o.backward(do)
    got = {"o": o.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
    figs = U.attn_figures(q.detach(), k.detach(), v.detach(), do, got)
    assert not U.report("cpu attn bwd clean", figs)


# ---------------------------------------------------------------------------
# the paired-tile 8-wave forward, emulated
# ---------------------------------------------------------------------------
def _paired_fwd(q, k, v, fault=None):
    """Plain fp32 torch emulation of the paired-tile forward: rounds of 64
    keys (sub-tiles A and B), one merged max, sum and rescale per round, P
    rounded to bf16 before PV, o rounded to bf16. Rows are handled alone, in
    strips of 32 like the kernel's waves. Returns (o, lse, times the fault
    changed a row's arithmetic).

    fault="needB": on their diagonal round, odd strips treat sub-tile B -- the
    keys of their own strip -- as wholly masked.
    fault="rescale": a row's O is not rescaled on a round in which its max
    grew in sub-tile B only (the decision looks at A's max alone). lsum and m
    are updated as they should be."""
    B, H, T, C = q.shape
    scale = 1.0 / math.sqrt(C)
    qf, kf, vf = q.float(), k.float(), v.float()
    rows = torch.arange(T)
    qw0 = (rows // 32) * 32
    odd = (rows // 32) % 2 == 1
    m = torch.full((B, H, T), -1e30)
    lsum = torch.zeros(B, H, T)
    acc = torch.zeros(B, H, T, C)
    fired = 0
    for k0 in range(0, T, 64):
        need_b = (k0 + 32) <= qw0 + 31
        if fault == "needB":
            wrong = odd & (k0 + 32 == qw0)
            fired += int(wrong.sum()) * B * H
            need_b = need_b & ~wrong
        keys = k0 + torch.arange(64)
        vis = keys[None, :] <= rows[:, None]
        vis[:, 32:] &= need_b[:, None]
        s = torch.matmul(qf, kf[:, :, k0:k0 + 64].transpose(-1, -2))
        s = torch.where(vis, s, torch.tensor(-1e30))
        mt_a, mt = s[..., :32].amax(-1), s.amax(-1)
        mn = torch.maximum(m, mt)
        alpha = torch.exp((m - mn) * scale)
        p = torch.exp((s - mn[..., None]) * scale) * vis     # rows not yet started: 0
        lsum = lsum * alpha + p.sum(-1)
        alpha_o = alpha
        if fault == "rescale":
            skipped = (mt_a <= m) & (mt > m)
            fired += int(skipped.sum())
            alpha_o = torch.where(skipped, torch.ones_like(alpha), alpha)
        acc = acc * alpha_o[..., None] + torch.matmul(U.rbf(p), vf[:, :, k0:k0 + 64])
        m = mn
    return (acc / lsum[..., None]).to(BF), m * scale + torch.log(lsum), fired


def _old_o_err(q, k, v, o):
    r32 = U.attn_math(q, k, v, None, torch.float32, False)
    return U.whole_relerr(o, r32["o"])


def test_paired_forward_emulation_clean_passes():
    """The emulation without a fault meets the bounds of the GPU tests, on
    random inputs and on every constructed case of section 3."""
    B, H, T, C = 1, 2, 512, 64
    torch.manual_seed(4)
    cases = {"random": tuple(torch.randn(B, H, T, C).to(BF) for _ in range(3))}
    for case in U.SOFTMAX_PATHS:
        cases[case] = U.attn_softmax_path_inputs(case, B, H, T, C)[:3]
        print(f"cpu attn paired {case}: {U.attn_check_path(case, *cases[case][:2])}")
    for case, (q, k, v) in cases.items():
        o, lse, _ = _paired_fwd(q, k, v)
        assert not U.report(f"cpu attn paired clean {case}",
                            U.attn_figures(q, k, v, None, {"o": o, "lse": lse}))


def test_attention_odd_strips_missing_their_own_keys_is_caught():
    """needB wrongly false on the diagonal round: rows of odd 32-row strips
    never see the 32 keys of their own strip.

    This fault is NOT hidden from the older metric: half of all rows lose up
    to 32 of their keys, and the whole-tensor error is 0.27 against the 2e-2
    bound (printed below). It is kept as the issue states it, untuned. The
    per-row figures flag both o and lse."""
    B, H, T, C = 1, 2, 512, 64
    torch.manual_seed(4)
    q, k, v = (torch.randn(B, H, T, C).to(BF) for _ in range(3))
    o, lse, fired = _paired_fwd(q, k, v, "needB")
    assert fired == B * H * T // 2
    old = _old_o_err(q, k, v, o)
    print(f"old whole-tensor relerr of the planted fault: {old:.4f} (bound 2e-2)")
    bad = U.report("cpu attn needB", U.attn_figures(q, k, v, None, {"o": o, "lse": lse}))
    assert {"attn.o", "attn.lse"} <= _names(bad)


def test_attention_missed_rescale_after_subtile_b_is_caught():
    """O is not rescaled on a round whose max grew in sub-tile B only, on the
    'growing' inputs of the online-softmax GPU cases. The emulation decides
    per row; the kernel decides per wave, where A's max grows for some row on
    every round of these inputs, so only a per-row fault can fire on them.
    lse is untouched by the fault; attn.o must flag it.

    This fault is NOT hidden from the older metric either, at these inputs:
    75 missed rescales change 73 of 1024 rows by up to 63% of their norm, a
    whole-tensor error of 0.045 against the 2e-2 bound (the per-row figure is
    58 x its bound). The older tests had no input of this kind, though. Kept
    as the issue states it, untuned."""
    B, H, T, C = 1, 2, 512, 64
    q, k, v, _ = U.attn_softmax_path_inputs("growing", B, H, T, C)
    o, lse, fired = _paired_fwd(q, k, v, "rescale")
    clean, _, _ = _paired_fwd(q, k, v)
    nrows = int((o.float() != clean.float()).any(-1).sum())
    assert fired > 0 and nrows > 0
    old = _old_o_err(q, k, v, o)
    print(f"missed rescales: {fired}, rows changed: {nrows} of {B * H * T}")
    print(f"old whole-tensor relerr of the planted fault: {old:.4f} (bound 2e-2)")
    bad = U.report("cpu attn rescale", U.attn_figures(q, k, v, None, {"o": o, "lse": lse}))
    assert "attn.o" in _names(bad) and "attn.lse" not in _names(bad)


# ---------------------------------------------------------------------------
def test_embedding_clean_passes_and_missing_contribution_is_caught():
    torch.manual_seed(8)
    N, V, D = 16384, 4096, 64
    idx = torch.randint(0, V, (N,))
    idx[idx == 17] = 18                     # row 17 is never indexed
    w = torch.zeros(V, D, dtype=BF, requires_grad=True)
    dy = torch.randn(N, D).to(BF)
    ops.embedding(idx, w).backward(dy)
    dw = w.grad
    assert not U.report("cpu embed clean", U.embedding_figures(dy, idx, V, dw))

    tok = int(idx[100])
    assert int((idx == tok).sum()) >= 2
    ref32 = torch.zeros(V, D).index_add_(0, idx, dy.float())
    planted = dw.clone()
    planted[tok] = (ref32[tok] - dy[100].float()).to(BF)   # one contribution lost
    old = U.whole_relerr(planted, ref32.to(BF))
    print(f"old whole-tensor relerr of the planted fault: {old:.4f} (bound 1e-2)")
    assert old < 1e-2
    bad = U.report("cpu embed missing", U.embedding_figures(dy, idx, V, planted))
    assert "embed.touched_err_over_tol" in _names(bad)

    stray = dw.clone()
    stray[17, 3] = 1e-3                     # a write into a never-indexed row
    bad = U.report("cpu embed stray", U.embedding_figures(dy, idx, V, stray))
    assert "embed.untouched_nonzero" in _names(bad)


# ---------------------------------------------------------------------------
def test_row_err_scales():
    ref = torch.zeros(4, 8, dtype=torch.float64)
    ref[1:] = 1.0
    got = ref.clone()
    assert U.row_err(got, ref) == 0.0       # a zero reference row does not divide by zero
    got[0, 0] = 0.1                         # judged on the typical row norm
    typical = math.sqrt(3 * 8 / 4)
    assert abs(U.row_err(got, ref) - 0.1 / typical) < 1e-12
    got[2, 0] = float("nan")
    assert math.isnan(U.row_err(got, ref))
    big = ref.clone()
    big[3] *= 100
    g2 = big.clone()
    g2[3, 0] += 1.0                         # judged on its own, larger norm
    assert abs(U.row_err(g2, big) - 1.0 / (100 * math.sqrt(8))) < 1e-12


def test_gelu_and_adamw_and_norm_cpu_paths_pass():
    x = U.gelu_all_inputs("cpu")
    assert x.numel() % 8 == 0 and bool(torch.isfinite(x.float()).all())
    assert float(x.float().abs().max()) == 64.0
    xr = x.clone().requires_grad_(True)
    y = ops.gelu(xr)
    torch.manual_seed(1)
    dy = torch.randn(x.numel()).to(BF)
    y.backward(dy)
    assert not U.report("cpu gelu", U.gelu_figures(x, dy, y.detach(), xr.grad))

    torch.manual_seed(7)
    n = 1027
    before = (torch.randn(n), torch.randn(n), torch.randn(n).abs() * 0.1,
              torch.randn(n).abs() * 0.01)
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, wd_over_peak_lr=0.1,
              grad_scale=0.125, clip_norm=1.0, step=3)
    master, grad, m, v = (t.clone() for t in before)
    sq = torch.tensor(1e4)
    ops.adamw_step(master, grad, m, v, None, sq_sum=sq, **hp)
    assert not U.report("cpu adamw", U.adamw_figures(before, sq, hp, (master, m, v)))

    x = torch.randn(37, 72).to(BF).requires_grad_(True)
    y = ops.rmsnorm(x, None, 1e-6)
    g = torch.randn(37, 72).to(BF)
    y.backward(g)
    r = torch.rsqrt(x.detach().float().pow(2).mean(-1) + 1e-6)
    assert not U.report("cpu rmsnorm",
                        U.rmsnorm_figures(x.detach(), None, g, 1e-6, y.detach(), r, x.grad))
