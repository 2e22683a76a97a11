"""Per-row error metric, fp64 references and fp32 "yardsticks" for the
kernel edge tests (test_kernel_edge_metrics.py, test_gpu_kernel_edges.py,
_edge_variant_worker.py). Plain torch; runs on whatever device the inputs
live on.

Three things per op:

- ``*_ref64``: the operation in fp64 on the same (bf16-rounded) inputs.
- ``*_yard``: the same operation in plain fp32 torch, rounding only where the
  kernel's documented contract rounds (one rounding to the output dtype for
  elementwise/rowwise ops; P and dS to bf16 before their matmuls and bf16
  outputs for attention; fp32 LSE and bf16 dlogits for cross-entropy).
- ``*_figures``: compares a result with the fp64 reference and bounds its
  ``row_err`` by FACTOR x the yardstick's ``row_err`` at the same inputs. The
  bound therefore never comes from the kernel under test.

fp32 per-row statistics (LSE, invrms, mean/invstd, loss) get FACTOR x the
yardstick plus STAT_ULPS fp32 ulp of the reference value: the hardware
exp/log/rsqrt are 1-ulp instructions and ``__expf``/``__logf`` add one
argument-scaling rounding each, which a correctly rounded library call in
the yardstick does not have.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

FACTOR = 3.0
STAT_ULPS = 4
F32_ULP = 2.0 ** -23


# ---------------------------------------------------------------------------
# metric
# ---------------------------------------------------------------------------
def row_err(got: torch.Tensor, ref64: torch.Tensor) -> float:
    """max over rows (last dim) of |got_r - ref_r|_2 / max(|ref_r|_2, rms_r |ref_r|_2).

    Rows smaller than typical (exactly-zero reference rows included) are
    judged on the typical row scale, larger rows on their own. NaN/Inf in
    ``got`` gives NaN, which fails every ``<=`` bound."""
    r = ref64.double()
    g = got.double().reshape(r.shape)
    r2 = r.reshape(-1, r.shape[-1])
    g2 = g.reshape(-1, r.shape[-1])
    rn = r2.norm(dim=-1)
    typical = rn.pow(2).mean().sqrt()
    den = torch.maximum(rn, typical).clamp_min(1e-300)
    e = (g2 - r2).norm(dim=-1) / den
    if not bool(torch.isfinite(g2).all()):
        return float("nan")
    return float(e.max())


def elem_err(got, ref64) -> float:
    """row_err with rows of length 1: per-element error on the larger of the
    element's own magnitude and the tensor's rms."""
    return row_err(got.reshape(-1, 1), ref64.reshape(-1, 1))


def whole_relerr(a, b) -> float:
    """The suite's older whole-tensor relative L2 error."""
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def bf16_ulp(x64: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 numbers at |x| (8 significant bits), fp64 tensor."""
    a = x64.double().abs().clamp_min(2.0 ** -126)
    _, e = torch.frexp(a)                      # a = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(a), e - 8)


def rbf(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16, keep the dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


@dataclass
class Figure:
    name: str
    kernel: float
    yard: float
    bound: float

    @property
    def ok(self) -> bool:
        return self.kernel <= self.bound      # NaN fails

    def __str__(self):
        return (f"{self.name}: kernel={self.kernel:.3e} yardstick={self.yard:.3e} "
                f"bound={self.bound:.3e} {'ok' if self.ok else 'OVER'}")


def fig_rows(name, got, yard, ref64) -> Figure:
    y = row_err(yard, ref64)
    return Figure(name, row_err(got, ref64), y, FACTOR * y)


def fig_elems(name, got, yard, ref64) -> Figure:
    y = elem_err(yard, ref64)
    return Figure(name, elem_err(got, ref64), y, FACTOR * y)


def fig_stat(name, got, yard, ref64) -> Figure:
    """fp32 per-row statistic: FACTOR x yardstick + STAT_ULPS fp32 ulp."""
    y = elem_err(yard, ref64)
    return Figure(name, elem_err(got, ref64), y, FACTOR * y + STAT_ULPS * F32_ULP)


def report(tag: str, figs) -> list:
    """Print every figure; return the ones over their bound."""
    for f in figs:
        print(f"EDGE {tag} {f}")
    return [f for f in figs if not f.ok]


def check(tag: str, figs):
    bad = report(tag, figs)
    assert not bad, f"{tag}: " + "; ".join(str(f) for f in bad)


# ---------------------------------------------------------------------------
# cross-entropy
# ---------------------------------------------------------------------------
def ce_math(logits, targets, dloss: float, dt):
    """(lse, loss, dlogits) of mean cross-entropy in dtype ``dt``."""
    N, V = logits.shape
    lf = logits.to(dt)
    lse = torch.logsumexp(lf, dim=-1)
    loss = (lse - lf.gather(1, targets[:, None]).squeeze(1)).mean()
    p = torch.exp(lf - lse[:, None])
    p.scatter_add_(1, targets[:, None], -torch.ones(N, 1, device=p.device, dtype=dt))
    gs = torch.tensor(dloss, dtype=dt, device=p.device) / N
    return lse, loss, p * gs


def ce_figures(logits, targets, dloss, got_lse, got_loss, got_dlogits):
    lse64, loss64, d64 = ce_math(logits, targets, dloss, torch.float64)
    lse32, loss32, d32 = ce_math(logits, targets, dloss, torch.float32)
    d32 = d32.to(torch.bfloat16)
    tcol = targets[:, None]

    def off_target(d):
        return d.double().scatter(1, tcol, 0.0)

    def on_target(d):
        return d.double().gather(1, tcol)

    # The kernel adds the N row losses (all >= 0) into one fp32 scalar with
    # atomics, in no fixed order: worst case N * 2^-24 relative, on top of the
    # statistic's allowance. The per-row check is ce.lse; this one is for the
    # target gather and the sum.
    loss = fig_stat("ce.loss", got_loss.reshape(1), loss32.reshape(1), loss64.reshape(1))
    loss.bound += logits.shape[0] * 2.0 ** -24
    return [
        fig_stat("ce.lse", got_lse, lse32, lse64),
        loss,
        fig_rows("ce.dlogits_offtarget", off_target(got_dlogits), off_target(d32),
                 off_target(d64)),
        fig_elems("ce.dlogits_target", on_target(got_dlogits), on_target(d32),
                  on_target(d64)),
    ]


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------
def rmsnorm_math(x, w, dy, eps, dt):
    """(y, invrms, dx) in dtype dt; dx is of the weightless norm (None if
    dy is None)."""
    xf = x.to(dt)
    r = torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + eps)
    y = xf * r
    if w is not None:
        y = y * w.to(dt)
    dx = None
    if dy is not None:
        g = dy.to(dt)
        dx = r * g - xf * r.pow(3) * (xf * g).mean(dim=-1, keepdim=True)
    return y, r.squeeze(-1), dx


def rmsnorm_figures(x, w, dy, eps, got_y, got_invrms, got_dx):
    y64, r64, dx64 = rmsnorm_math(x, w, dy, eps, torch.float64)
    y32, r32, dx32 = rmsnorm_math(x, w, dy, eps, torch.float32)
    figs = [fig_rows("rmsnorm.y", got_y, y32.to(x.dtype), y64),
            fig_stat("rmsnorm.invrms", got_invrms, r32, r64)]
    if dy is not None:
        figs.append(fig_rows("rmsnorm.dx", got_dx, dx32.to(x.dtype), dx64))
    return figs


# ---------------------------------------------------------------------------
# QK-LayerNorm + RoPE over packed qkv (B, T, 3, H, C)
# ---------------------------------------------------------------------------
def _rot2(x):
    return torch.stack((-x[..., 1::2], x[..., ::2]), dim=-1).flatten(-2)


def qkv_prep_math(qkv, qw, kw, sin, cos, eps, dt, grads=None):
    """Returns dict with q, k (B,H,T,C), qstats/kstats (B,H,T,2) and, with
    grads=(gq, gk, gv), dqkv, dqw, dkw -- all in dtype dt (autograd)."""
    x = qkv.detach().to(dt).requires_grad_(grads is not None)
    qw_ = qw.detach().to(dt).requires_grad_(grads is not None)
    kw_ = kw.detach().to(dt).requires_grad_(grads is not None)
    sin2 = torch.repeat_interleave(sin.to(dt), 2, dim=-1)
    cos2 = torch.repeat_interleave(cos.to(dt), 2, dim=-1)
    out = {}

    def ln_rope(xr, w, key):
        mu = xr.mean(dim=-1, keepdim=True)
        var = (xr - mu).pow(2).mean(dim=-1, keepdim=True)
        invstd = torch.rsqrt(var + eps)
        out[key] = torch.cat([mu, invstd], dim=-1).detach()
        n = (xr - mu) * invstd * w
        return n * cos2 + _rot2(n) * sin2

    q = ln_rope(x[:, :, 0].permute(0, 2, 1, 3), qw_, "qstats")
    k = ln_rope(x[:, :, 1].permute(0, 2, 1, 3), kw_, "kstats")
    v = x[:, :, 2].permute(0, 2, 1, 3)
    out["q"], out["k"] = q.detach(), k.detach()
    if grads is not None:
        gq, gk, gv = (g.to(dt) for g in grads)
        (q * gq).sum().add((k * gk).sum()).add((v * gv).sum()).backward()
        out["dqkv"], out["dqw"], out["dkw"] = x.grad, qw_.grad, kw_.grad
    return out


def qkv_prep_figures(qkv, qw, kw, sin, cos, eps, grads, got):
    """got: dict with the kernel's q, k, qstats, kstats, dqkv, dqw, dkw."""
    r = qkv_prep_math(qkv, qw, kw, sin, cos, eps, torch.float64, grads)
    y = qkv_prep_math(qkv, qw, kw, sin, cos, eps, torch.float32, grads)
    bf = torch.bfloat16
    figs = [fig_rows("qkv.q", got["q"], y["q"].to(bf), r["q"]),
            fig_rows("qkv.k", got["k"], y["k"].to(bf), r["k"])]
    for s in ("qstats", "kstats"):
        figs.append(fig_stat(f"qkv.{s}.mean", got[s][..., 0], y[s][..., 0], r[s][..., 0]))
        figs.append(fig_stat(f"qkv.{s}.invstd", got[s][..., 1], y[s][..., 1], r[s][..., 1]))
    if grads is not None:
        figs.append(fig_rows("qkv.dqkv", got["dqkv"], y["dqkv"].to(bf), r["dqkv"]))
        figs.append(fig_rows("qkv.dqw", got["dqw"], y["dqw"], r["dqw"]))
        figs.append(fig_rows("qkv.dkw", got["dkw"], y["dkw"], r["dkw"]))
    return figs


# ---------------------------------------------------------------------------
# causal attention
# ---------------------------------------------------------------------------
def attn_math(q, k, v, do, dt, rnd: bool, keep=None, p: float = 0.0):
    """Causal attention forward (+ backward if ``do`` is given) in dtype dt.
    rnd=True rounds where the kernels' contract rounds: P (after dropout
    scaling) and dS to bf16 before their matmuls, every output to bf16.
    ``keep``: bool (B,H,T,T) dropout keep-mask, kept entries scaled 1/(1-p).
    LSE is that of the undropped softmax. Returns dict o, lse[, dq, dk, dv]."""
    B, H, T, C = q.shape
    scale = 1.0 / math.sqrt(C)
    r = rbf if rnd else (lambda t: t)
    qf, kf, vf = q.to(dt), k.to(dt), v.to(dt)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    tril = torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
    s = s.masked_fill(~tril, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    pm = torch.exp(s - lse[..., None])
    del s
    z = None if keep is None else keep.to(device=q.device, dtype=dt) / (1.0 - p)
    pd = pm if z is None else pm * z
    o = r(torch.matmul(r(pd), vf))
    out = {"o": o, "lse": lse}
    if do is None:
        return out
    dof = do.to(dt)
    out["dv"] = r(torch.matmul(r(pd).transpose(-1, -2), dof))
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    if z is not None:
        dp = dp * z
    delta = (dof * o).sum(dim=-1, keepdim=True)
    ds = r(pm * (dp - delta))
    out["dq"] = r(torch.matmul(ds, kf) * scale)
    out["dk"] = r(torch.matmul(ds.transpose(-1, -2), qf) * scale)
    return out


def attn_figures(q, k, v, do, got, keep=None, p=0.0, names=None):
    """got: dict of the kernel's o, lse[, dq, dk, dv]; only the keys present
    are judged."""
    r = attn_math(q, k, v, do, torch.float64, False, keep, p)
    y = attn_math(q, k, v, do, torch.float32, True, keep, p)
    figs = []
    for n in names or ("o", "lse", "dq", "dk", "dv"):
        if n not in got or n not in r:
            continue
        if n == "lse":
            figs.append(fig_stat("attn.lse", got[n], y[n], r[n]))
        else:
            figs.append(fig_rows(f"attn.{n}", got[n], y[n], r[n]))
    return figs


SOFTMAX_PATHS = ("first", "growing", "lastB", "lastA")


def attn_softmax_path_inputs(case: str, B, H, T, C, device="cpu", seed=15):
    """(q, k, v, do) in bf16 with keys constructed to drive one path of the
    online softmax. Drawn on the CPU from a fixed seed, so the GPU tests and
    the CPU emulation see the same numbers. u is a fixed unit vector.

    - ``first`` / ``lastB`` / ``lastA``: q = sqrt(C) u + noise, k = noise/2,
      and one spiked key 8 u at position 0 / T-3 / T-40. Its score is
      8 +- 8/sqrt(C) against N(0, 1/2) for the others, so it is the maximum of
      every row that sees it (attn_check_path asserts that) and takes 80% or
      more of the row's weight. No larger on purpose: once P is one-hot, o is
      a copy of one v row, dq and dk are the rounding noise of delta alone
      (yardstick row_err > 1), and their figures check nothing.
    - ``growing``: q = sqrt(C) u + noise/2, k_j = (16 j / T) u + noise/2: the
      score rises by 1 per 32-key tile, under key noise of std 0.56."""
    g = torch.Generator().manual_seed(seed + C)
    u = torch.randn(C, generator=g)
    u = u / u.norm()
    rc = math.sqrt(C)

    def noise(s=1.0):
        return torch.randn(B, H, T, C, generator=g) * s

    if case == "growing":
        j = torch.arange(T, dtype=torch.float32)[:, None]
        q = rc * u + noise(0.5)
        k = (16.0 * j / T) * u + noise(0.5)
    else:
        pos = {"first": 0, "lastB": T - 3, "lastA": T - 40}[case]
        q = rc * u + noise()
        k = noise(0.5)
        k[:, :, pos] = 8.0 * u
    v, do = noise(), noise()
    return tuple(t.to(torch.bfloat16).to(device) for t in (q, k, v, do))


def attn_check_path(case: str, q, k) -> str:
    """Asserts that the inputs (never the kernel) take the path they were
    built for, from the fp32 scores; returns a line for the EDGE output."""
    B, H, T, C = q.shape
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) / math.sqrt(C)
    tril = torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
    top = float(s[tril.expand_as(s)].abs().max())
    s = s.masked_fill(~tril, float("-inf"))
    if case != "growing":
        pos = {"first": 0, "lastB": T - 3, "lastA": T - 40}[case]
        assert bool((s[..., pos:, :].argmax(-1) == pos).all()), "the spike is not every row's max"
        return f"max |score| {top:.1f}, key {pos} is the max of rows {pos}..{T - 1}"
    nt = T // 32
    tm = s.reshape(B, H, T, nt, 32).amax(-1)                    # (B,H,T,tile), -inf if unseen
    grows = tm[..., 1:] > tm.cummax(-1).values[..., :-1]        # a later tile's max is -inf: False
    strip_grows = grows.reshape(B, H, nt, 32, nt - 1).any(3)    # the kernels decide per wave
    seen = torch.ones(nt, nt, dtype=torch.bool, device=q.device).tril()[:, 1:]
    assert bool(strip_grows[..., seen].all()), "a strip has a tile in which no row's max grows"
    pa, pb = tm[..., 0::2], tm[..., 1::2]
    both = torch.isfinite(pb)
    b_over_a = float((pb > pa)[both].float().mean())
    rows = float(grows[torch.isfinite(tm[..., 1:])].float().mean())
    assert b_over_a > 0.5 and rows > 0.5
    return (f"max |score| {top:.1f}, max grows in every tile of every strip "
            f"({100 * rows:.0f}% of rows x tiles), B over A in {100 * b_over_a:.0f}% of pairs")


# ---------------------------------------------------------------------------
# embedding backward
# ---------------------------------------------------------------------------
def embedding_figures(dy, idx, V, got):
    """Derived bound, no measured tolerance. Per element of a touched row:
    one final bf16 rounding (<= 1 bf16 ulp of the fp64 sum, which allows a
    rounding-boundary flip) plus the fp32 accumulation error of an n_run-term
    sum in any order, n_run * 2^-24 * sum|dy|. Rows never indexed: exactly 0.
    Figures are max |err| / tolerance (bound 1) and the count of nonzero
    elements in untouched rows (bound 0)."""
    D = dy.shape[1]
    idx = idx.reshape(-1)
    ref = torch.zeros(V, D, dtype=torch.float64, device=dy.device)
    ref.index_add_(0, idx, dy.double())
    sabs = torch.zeros_like(ref).index_add_(0, idx, dy.double().abs())
    cnt = torch.bincount(idx, minlength=V).double()[:, None]
    tol = bf16_ulp(ref) + cnt * 2.0 ** -24 * sabs
    touched = (cnt > 0).expand(V, D)
    y32 = torch.zeros(V, D, dtype=torch.float32, device=dy.device)
    y32.index_add_(0, idx, dy.float())
    yard = y32.to(torch.bfloat16)

    def ratio(t):
        if not bool(torch.isfinite(t.float()).all()):
            return float("nan")
        e = (t.double() - ref).abs() / tol
        return float(e[touched].max()) if bool(touched.any()) else 0.0

    def stray(t):
        return float((t[~touched[:, 0]] != 0).sum())

    return [Figure("embed.touched_err_over_tol", ratio(got), ratio(yard), 1.0),
            Figure("embed.untouched_nonzero", stray(got), stray(yard), 0.0)]


# ---------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------
def adamw_math(master, grad, m, v, sq_sum, dt, *, lr, beta1, beta2, eps,
               wd_over_peak_lr, grad_scale, clip_norm, step):
    """The documented update (csrc/adamw.hip header), out of place, in dt."""
    th, g, m, v = (t.to(dt) for t in (master, grad, m, v))
    gnorm = sq_sum.to(dt).sqrt() * grad_scale + 1e-12
    coef = grad_scale * torch.clamp(clip_norm / gnorm, max=1.0)
    g = g * coef
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    mhat = m / (1 - beta1 ** step)
    vhat = v / (1 - beta2 ** step)
    th = th - lr * (mhat / (vhat.sqrt() + eps) + wd_over_peak_lr * th)
    return th, m, v


def adamw_figures(before, sq_sum, hp, got):
    """before/got: (master, grad, m, v) before and (master, m, v) after."""
    r = adamw_math(*before, sq_sum, torch.float64, **hp)
    y = adamw_math(*before, sq_sum, torch.float32, **hp)
    return [fig_elems(f"adamw.{n}", got[i], y[i], r[i])
            for i, n in enumerate(("master", "m", "v"))]


# ---------------------------------------------------------------------------
# GELU (tanh approximation)
# ---------------------------------------------------------------------------
GELU_C0, GELU_C1 = 0.7978845608028654, 0.044715


def gelu_all_inputs(device) -> torch.Tensor:
    """Every finite bf16 value with |x| <= 64 (both zeros, subnormals):
    2 * 0x4281 = 34050 values, zero-padded to a multiple of 8."""
    pos = torch.arange(0, 0x4281, dtype=torch.int32)
    bits = torch.cat([pos, pos + 0x8000]).to(torch.int16)   # wraps to the sign bit
    x = bits.view(torch.bfloat16)
    assert x.numel() == 34050
    pad = (-x.numel()) % 8
    return torch.cat([x, torch.zeros(pad, dtype=torch.bfloat16)]).to(device)


def gelu_math(x, dy, dt):
    xf = x.to(dt)
    inner = GELU_C0 * (xf + GELU_C1 * xf ** 3)
    t = torch.tanh(inner)
    y = 0.5 * xf * (1 + t)
    if dy is None:
        return y, None
    dg = 0.5 * (1 + t) + 0.5 * xf * (1 - t * t) * GELU_C0 * (1 + 3 * GELU_C1 * xf ** 2)
    return y, dy.to(dt) * dg


def gelu_figures(x, dy, got_y, got_dx):
    """Per element. Forward: |err| <= 1 bf16 ulp(ref) + |x| 2^-22 + |ref| 2^-23;
    the last two terms are the fp32 cancellation in 1 + tanh, inherent to the
    formula. Backward: dgelu = (1+t)/2 + x (1-t^2) d / 2 with d = c0 (1 + 3 c1
    x^2); an absolute error dt <= 2^-21 on t (three fp32 roundings at
    magnitude <= 2 plus the exp2 argument rounding) moves it by at most
    (1/2 + |x| d) dt, so |err| <= 1 bf16 ulp(ref) + |dy| (1/2 + |x| d) 2^-21
    + |ref| 2^-22. Figures: max |err|/tol (bound 1) and the number of inputs
    whose result differs from the bf16-rounded fp64 result, capped at FACTOR x
    the yardstick's number."""
    y64, dx64 = gelu_math(x, dy, torch.float64)
    y32, dx32 = gelu_math(x, dy, torch.float32)
    xa = x.double().abs()
    figs = []

    def pair(name, got, yard, ref, tol):
        yard = yard.to(torch.bfloat16)

        def ratio(t):
            if not bool(torch.isfinite(t.float()).all()):
                return float("nan")
            return float(((t.double() - ref).abs() / tol).max())

        def flips(t):
            return float((t.double() != ref.to(torch.bfloat16).double()).sum())

        figs.append(Figure(f"{name}.err_over_tol", ratio(got), ratio(yard), 1.0))
        figs.append(Figure(f"{name}.off_by_ulp_count", flips(got), flips(yard),
                           FACTOR * flips(yard)))

    if got_y is not None:
        tol = bf16_ulp(y64) + xa * 2.0 ** -22 + y64.abs() * 2.0 ** -23
        pair("gelu.y", got_y, y32, y64, tol)
    if got_dx is not None:
        d = GELU_C0 * (1 + 3 * GELU_C1 * xa ** 2)
        tol = (bf16_ulp(dx64) + dy.double().abs() * (0.5 + xa * d) * 2.0 ** -21
               + dx64.abs() * 2.0 ** -22)
        pair("gelu.dx", got_dx, dx32, dx64, tol)
    return figs
