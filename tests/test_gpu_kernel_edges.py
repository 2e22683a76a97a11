"""GPU kernel edge tests: per-row error against fp64 references with bounds
taken from an fp32 yardstick (kernel_edge_util), at the smallest shapes that
reach a grid-stride second trip, a ragged tail, an unpadded vocab, the 4-wave
attention kernels with more than one q/k block, the embedding-bwd variants,
and the environment-gated kernels. Exact properties (causality, head
independence, pass-through, untouched buffers) are compared bit for bit.

Attention, what is covered where (main process, default launch path):

- 4 waves (T % 256 == 128): T=384 and 640 in test_attention_rows and every
  exact test.
- 8 waves (T % 256 == 0), per row: test_attention_rows at T=256, 512, 768
  (o, lse, dq, dk, dv; C=64 and 128; with and without dropout) and at 1024
  (backward, C=64); test_attention_online_softmax_paths_at_8_waves and
  test_attention_large_scores at T=512 (no dropout).
- 8 waves, exact: first row and forward causality, backward causality of dq,
  head independence, zero upstream rows; all at T=512, C=64 and 128, with and
  without dropout.
- Kernels behind those cases: no dropout, C=128 forward is the paired-tile
  attn_fwd2_kernel<128,8>, C=64 attn_fwd_kernel<64,8,1,false>; dropout takes
  attn_fwd_kernel<C,8,1,true>; backward attn_bwd_dkv_kernel<C,8,DROP> and
  attn_bwd_dq_kernel<C,8,1,DROP>.
- The child process (_edge_variant_worker.py) swaps the undropped backward to
  4 waves at T=512; its forward is the 8-wave one again.

Every test prints ``EDGE <case> <tensor>: kernel=.. yardstick=.. bound=..``;
the figures measured on MI355X are in profiles/kernel_edge_errors.md."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import kernel_edge_util as U

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from midgpt_amd import ops
    from midgpt_amd.ops import reference as ref
    assert ops.have_ext(), f"HIP extension must be built: {ops._C_ERR}"

DEV = "cuda:0"
BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))


def randbf(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(BF)


# ---------------------------------------------------------------------------
# cross-entropy
# ---------------------------------------------------------------------------
def _ce_targets(N, V):
    """Rows 0..3: target at 0, at V-1, at the last element the vector loop
    covers, and inside the scalar tail (V-1 again when V % 8 == 0)."""
    t = torch.randint(0, V, (N,), device=DEV)
    vec_end = (V // 8) * 8
    t[0], t[1], t[2] = 0, V - 1, vec_end - 1
    t[3] = vec_end + (V % 8) // 2 if V % 8 else V - 1
    return t


@pytest.mark.parametrize("N,V", [(37, 65), (8, 2056), (8, 4099), (8269, 65), (8, 50304)])
def test_cross_entropy_rows(N, V):
    torch.manual_seed(6)
    logits = randbf(N, V, scale=2.0)
    targets = _ce_targets(N, V)
    # adversarial rows 4..7
    logits[4] = 1.5                                   # all equal: LSE = x + log V
    logits[5, targets[5]] = 64.0                      # dominant logit at the target
    other = (int(targets[6]) + V // 2) % V
    logits[6, other] = 64.0                           # dominant logit elsewhere
    logits[7] = -100.0                                # all far below zero
    lg = logits.clone().requires_grad_(True)
    loss = ops.cross_entropy(lg, targets)
    (loss * 3.5).backward()                           # non-unit upstream gradient
    _, lse = ops._C.ce_fwd(logits, targets)
    U.check(f"ce N{N} V{V}", U.ce_figures(logits, targets, 3.5, lse, loss.detach(), lg.grad))
    assert abs(float(lse[4]) - (1.5 + math.log(V))) <= 4 * U.F32_ULP * (1.5 + math.log(V))
    assert abs(float(lse[7]) - (-100 + math.log(V))) <= 4 * U.F32_ULP * 100
    # the older whole-tensor check, kept
    _, _, d32 = U.ce_math(logits, targets, 3.5, torch.float32)
    assert U.whole_relerr(lg.grad, d32) < 2e-2


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------
def _rms_input(N, D, dtype):
    x = torch.randn(N, D, device=DEV)
    x[0] = 0.0                     # with eps: finite y and dx
    if N > 1:
        x[1] *= 1e3
    return x.to(dtype)


@pytest.mark.parametrize("N,D", [(32773, 72), (5, 520), (3, 8)])
def test_rmsnorm_bf16_rows(N, D):
    torch.manual_seed(2)
    x = _rms_input(N, D, BF)
    dy = randbf(N, D)
    y, invrms = ops._C.rmsnorm_fwd(x, None, 1e-6)
    dx, _ = ops._C.rmsnorm_bwd(dy, x, None, invrms, 1e-6)
    assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(dx.float()).all())
    assert bool((y[0] == 0).all())
    U.check(f"rmsnorm bf16 N{N} D{D}", U.rmsnorm_figures(x, None, dy, 1e-6, y, invrms, dx))
    # the autograd wrapper takes the same kernels
    xr = x.clone().requires_grad_(True)
    yr = ops.rmsnorm(xr, None, 1e-6)
    yr.backward(dy)
    assert torch.equal(yr.detach(), y) and torch.equal(xr.grad, dx)


@pytest.mark.parametrize("dtype,N,D,weighted", [(torch.float32, 7, 100, False),
                                               (torch.float32, 7, 100, True),
                                               (BF, 5, 520, True)])
def test_rmsnorm_fp32_kernel_and_weighted_forward(dtype, N, D, weighted):
    torch.manual_seed(3)
    x = _rms_input(N, D, dtype)
    w = torch.randn(D, device=DEV) if weighted else None
    y, invrms = ops._C.rmsnorm_fwd(x, w, 1e-6)
    assert y.dtype == dtype
    U.check(f"rmsnorm {str(dtype)[6:]} N{N} D{D} w{int(weighted)}",
            U.rmsnorm_figures(x, w, None, 1e-6, y, invrms, None))


def test_rmsnorm_unsupported_raises():
    x = randbf(4, 64)
    w = torch.ones(64, device=DEV)
    y, invrms = ops._C.rmsnorm_fwd(x, w, 1e-6)
    with pytest.raises(RuntimeError):          # weighted backward is unimplemented
        ops._C.rmsnorm_bwd(x, x, w, invrms, 1e-6)
    with pytest.raises(RuntimeError):          # bf16 rows that are no multiple of 8
        ops._C.rmsnorm_fwd(randbf(4, 65), None, 1e-6)


# ---------------------------------------------------------------------------
# qkv_prep
# ---------------------------------------------------------------------------
def _qkv_case(B, T, H, C, bwd=True):
    torch.manual_seed(3)
    qkv = randbf(B, T, 3, H, C)
    qkv[0, 0, 0, 0] *= 50.0                      # one row at a larger scale
    qw = torch.randn(C, device=DEV)
    kw = torch.randn(C, device=DEV)
    sin, cos = ref.rope_tables(C, T, device=DEV)
    q, k, v, qs, ks = ops._C.qkv_prep_fwd(qkv, qw, kw, sin, cos, 1e-6)
    got = {"q": q, "k": k, "qstats": qs, "kstats": ks}
    assert torch.equal(v, qkv[:, :, 2].permute(0, 2, 1, 3))      # V passes through
    grads = None
    if bwd:
        grads = (randbf(B, H, T, C), randbf(B, H, T, C), randbf(B, H, T, C))
        dqkv, dqw, dkw = ops._C.qkv_prep_bwd(*grads, qkv, qw, kw, sin, cos, qs, ks, 1e-6)
        assert torch.equal(dqkv[:, :, 2], grads[2].permute(0, 2, 1, 3))
        got.update(dqkv=dqkv, dqw=dqw, dkw=dkw)
    return U.qkv_prep_figures(qkv, qw, kw, sin, cos, 1e-6, grads, got)


@pytest.mark.parametrize("C", [8, 16, 32, 64, 128])
def test_qkv_prep_head_dims_odd_heads(C):
    U.check(f"qkv B2 T24 H5 C{C}", _qkv_case(2, 24, 5, C))


def test_qkv_prep_bwd_grid_stride():
    U.check("qkv B3 T256 H29 C128", _qkv_case(3, 256, 29, 128))       # 66816 rows


def test_qkv_prep_fwd_grid_stride():
    U.check("qkv B3 T1024 H29 C128", _qkv_case(3, 1024, 29, 128, bwd=False))  # 267264 rows


@pytest.mark.parametrize("B,T,H,C", [(2, 128, 2, 64), (2, 24, 5, 8), (3, 256, 29, 128)])
def test_qkv_prep_bwd_weight_grads_are_bit_reproducible(B, T, H, C):
    """dqw/dkw are reduced over all rows; the reduction order is fixed, so a
    replay (activation remat) gives the same bits. With float atomics in the
    block reduction, test_model_gpu_dropout_in_kernel_and_remat_bit_identical
    was seen to differ by one ulp in k_ln_weight.grad."""
    torch.manual_seed(3)
    qkv = randbf(B, T, 3, H, C)
    qw, kw = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    sin, cos = ref.rope_tables(C, T, device=DEV)
    _, _, _, qs, ks = ops._C.qkv_prep_fwd(qkv, qw, kw, sin, cos, 1e-6)
    g = [randbf(B, H, T, C) for _ in range(3)]
    first = ops._C.qkv_prep_bwd(*g, qkv, qw, kw, sin, cos, qs, ks, 1e-6)
    for _ in range(4):
        again = ops._C.qkv_prep_bwd(*g, qkv, qw, kw, sin, cos, qs, ks, 1e-6)
        for a, b in zip(first, again):
            assert torch.equal(a, b)


@pytest.mark.parametrize("C", [96, 24])
def test_qkv_prep_rejects_head_dims_the_kernel_cannot_reduce(C):
    B, T, H = 1, 8, 2
    qkv = randbf(B, T, 3, H, C)
    w = torch.ones(C, device=DEV)
    sin, cos = ref.rope_tables(C, T, device=DEV)
    with pytest.raises(RuntimeError):
        ops._C.qkv_prep_fwd(qkv, w, w, sin, cos, 1e-6)
    g = randbf(B, H, T, C)
    st = torch.zeros(B, H, T, 2, device=DEV)
    with pytest.raises(RuntimeError):
        ops._C.qkv_prep_bwd(g, g, g, qkv, w, w, sin, cos, st, st, 1e-6)


def test_qkv_prep_bwd_rejects_wrong_dtype():
    B, T, H, C = 1, 8, 2, 64
    qkv = randbf(B, T, 3, H, C)
    w = torch.ones(C, device=DEV)
    sin, cos = ref.rope_tables(C, T, device=DEV)
    g = randbf(B, H, T, C)
    st = torch.zeros(B, H, T, 2, device=DEV)
    with pytest.raises(RuntimeError):
        ops._C.qkv_prep_bwd(g.float(), g, g, qkv, w, w, sin, cos, st, st, 1e-6)
    with pytest.raises(RuntimeError):
        ops._C.qkv_prep_bwd(g, g, g, qkv.float(), w, w, sin, cos, st, st, 1e-6)


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------
P, SEED = 0.2, 7
_KEEP = {}


def mirror(B, H, T):
    """Host-mirror dropout mask on the device, once per shape, never mutated."""
    key = (B, H, T)
    if key not in _KEEP:
        _KEEP[key] = ref.attn_dropout_keep(SEED, B, H, T, P).to(DEV)
    return _KEEP[key]


def _attn_run(q, k, v, do, drop, fwd=True):
    if drop:
        o, lse = ops._C.attn_fwd_dropout(q, k, v, P, SEED)
    else:
        o, lse = ops._C.attn_fwd(q, k, v)
    got = {"o": o, "lse": lse}
    if do is not None:
        if drop:
            dq, dk, dv = ops._C.attn_bwd_dropout(do, q, k, v, o, lse, P, SEED)
        else:
            dq, dk, dv = ops._C.attn_bwd(do, q, k, v, o, lse)
        got.update(dq=dq, dk=dk, dv=dv)
    return got


ATTN_SHAPES = [(1, 3, 384, 64), (1, 3, 384, 128), (3, 5, 640, 64), (3, 11, 1024, 64)]
# T % 256 == 0: the 8-wave kernels of the default path. 256: one workgroup per
# head, every wave on its own diagonal. 512: two q/k blocks, unmasked rounds
# before the diagonal, 16 q tiles in the first dkv workgroup. 768: an odd
# block count, B=2 for the batch stride, 24 and 8 q tiles in the first and
# last dkv workgroup.
ATTN8_SHAPES = [(1, 3, 256, 64), (1, 3, 256, 128), (1, 3, 512, 64), (1, 3, 512, 128),
                (2, 3, 768, 64), (2, 3, 768, 128)]
ATTN8_EXACT = [(1, 3, 512, 64), (1, 3, 512, 128)]


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "p0.2"])
@pytest.mark.parametrize("B,H,T,C", ATTN_SHAPES + ATTN8_SHAPES)
def test_attention_rows(B, H, T, C, drop):
    """NW=4 with more than one q/k block and odd B*H; (3,11,1024,64) is there
    for the delta kernel's grid-stride second trip (33792 rows). ATTN8_SHAPES:
    all five tensors of the 8-wave kernels, both head dims, both DROP values."""
    torch.manual_seed(4)
    q, k, v, do = (randbf(B, H, T, C) for _ in range(4))
    got = _attn_run(q, k, v, do, drop)
    keep = mirror(B, H, T) if drop else None
    names = ("dq", "dk", "dv") if T == 1024 else None        # bwd only
    U.check(f"attn {'p0.2' if drop else 'nodrop'} B{B} H{H} T{T} C{C}",
            U.attn_figures(q, k, v, do, got, keep, P if drop else 0.0, names))


@pytest.mark.parametrize("B,H,T,C", ATTN_SHAPES[:2])
def test_attention_dropout_mask_is_the_mirror_at_4_waves(B, H, T, C):
    """The construction of test_forward_kernel_mask_is_the_mirror_exactly:
    q = k = 0, V one-hot per column block, O > 0 iff causal and kept."""
    q = torch.zeros(B, H, T, C, device=DEV, dtype=BF)
    got = torch.zeros(B, H, T, T, device=DEV, dtype=torch.bool)
    eye = torch.eye(C, device=DEV, dtype=BF)
    for blk in range(T // C):
        v = torch.zeros(B, H, T, C, device=DEV, dtype=BF)
        v[:, :, blk * C:(blk + 1) * C] = eye
        o, _ = ops._C.attn_fwd_dropout(q, q, v, P, SEED)
        got[..., blk * C:(blk + 1) * C] = o > 0
    tril = torch.ones(T, T, dtype=torch.bool, device=DEV).tril()
    nbad = int((got != (mirror(B, H, T) & tril)).sum())
    print(f"EDGE attn mask B{B} H{H} T{T} C{C}: mismatches {nbad} of {got.numel()}")
    assert nbad == 0


def _t0s(T):
    """Perturbation starts: inside a 32-key tile and on a workgroup edge; at 8
    waves also where sub-tile B of a 64-key pair starts, in both q-blocks."""
    return (200, 256) if T % 256 else (200, 224, 256, 288)


@pytest.mark.parametrize("B,H,T,C", ATTN_SHAPES[:2] + ATTN8_EXACT)
def test_attention_first_row_and_causality_exact(B, H, T, C):
    torch.manual_seed(11)
    q, k, v = (randbf(B, H, T, C) for _ in range(3))
    o, lse = ops._C.attn_fwd(q, k, v)
    assert torch.equal(o[..., 0, :], v[..., 0, :])           # P = 1 on row 0
    q0, k0 = q[..., 0, :].double(), k[..., 0, :].double()
    s0 = (q0 * k0).sum(-1) / math.sqrt(C)
    # fp32 accumulation of C products plus STAT_ULPS ulp on the result
    tol = C * 2.0 ** -24 * (q0 * k0).abs().sum(-1) / math.sqrt(C) + U.STAT_ULPS * U.F32_ULP * s0.abs()
    assert bool(((lse[..., 0].double() - s0).abs() <= tol).all())
    for t0 in _t0s(T):
        q2, k2, v2 = q.clone(), k.clone(), v.clone()
        for t in (q2, k2, v2):
            t[..., t0:, :] = randbf(B, H, T - t0, C, scale=3.0)
        for drop in (False, True):
            a = _attn_run(q, k, v, None, drop)
            b = _attn_run(q2, k2, v2, None, drop)
            assert torch.equal(a["o"][..., :t0, :], b["o"][..., :t0, :]), (t0, drop)
            assert torch.equal(a["lse"][..., :t0], b["lse"][..., :t0]), (t0, drop)
            assert not torch.equal(a["o"][..., t0:, :], b["o"][..., t0:, :]), (t0, drop)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "p0.2"])
@pytest.mark.parametrize("B,H,T,C", ATTN_SHAPES[:2] + ATTN8_EXACT)
def test_attention_bwd_causality_exact(B, H, T, C, drop):
    """dq of a row depends on nothing at or after t0 > row: later rows of q,
    k, v and dO (with o and lse of the matching forward) must leave dq on rows
    < t0 bit-identical. Masked entries have P = 0 exactly, so dS = 0 x finite;
    the perturbation is finite for that reason (0 x NaN would fail a correct
    kernel). Pins the dq kernel's tile loop and mask and the delta kernel."""
    torch.manual_seed(16)
    q, k, v, do = (randbf(B, H, T, C) for _ in range(4))
    a = _attn_run(q, k, v, do, drop)
    for t0 in _t0s(T):
        pert = [t.clone() for t in (q, k, v, do)]
        for t in pert:
            t[..., t0:, :] = randbf(B, H, T - t0, C, scale=3.0)
        b = _attn_run(*pert, drop)
        assert bool(torch.isfinite(b["dq"].float()).all()), t0
        assert torch.equal(a["dq"][..., :t0, :], b["dq"][..., :t0, :]), t0
        assert not torch.equal(a["dq"][..., t0:, :], b["dq"][..., t0:, :]), t0


def _heads_are_independent(B, H, T, C, drop):
    torch.manual_seed(12)
    q, k, v, do = (randbf(B, H, T, C) for _ in range(4))
    a = _attn_run(q, k, v, do, drop)
    q2, k2, v2, do2 = q.clone(), k.clone(), v.clone(), do.clone()
    for t in (q2, k2, v2, do2):
        t[1, 1] = randbf(T, C, scale=2.0)
    b = _attn_run(q2, k2, v2, do2, drop)
    others = torch.ones(B, H, dtype=torch.bool, device=DEV)
    others[1, 1] = False
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(a[n][others], b[n][others]), n
        assert not torch.equal(a[n][1, 1], b[n][1, 1]), n


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "p0.2"])
def test_attention_heads_are_independent_exact(drop):
    _heads_are_independent(2, 3, 384, 64, drop)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "p0.2"])
@pytest.mark.parametrize("C", [64, 128])
def test_attention_heads_are_independent_exact_at_8_waves(C, drop):
    _heads_are_independent(2, 3, 512, C, drop)


def _zero_upstream_rows(B, H, T, C, t0, drop):
    torch.manual_seed(13)
    q, k, v, do = (randbf(B, H, T, C) for _ in range(4))
    do[..., t0:, :] = 0
    g = _attn_run(q, k, v, do, drop)
    for n in ("dq", "dk", "dv"):
        assert bool((g[n][..., t0:, :] == 0).all()), n
        assert bool((g[n][..., :t0, :] != 0).any()), n


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "p0.2"])
@pytest.mark.parametrize("t0", [200, 256])
def test_attention_zero_upstream_rows_give_exact_zero_grads(t0, drop):
    _zero_upstream_rows(1, 3, 384, 64, t0, drop)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "p0.2"])
@pytest.mark.parametrize("t0", [200, 224, 256])
@pytest.mark.parametrize("B,H,T,C", ATTN8_EXACT)
def test_attention_zero_upstream_rows_give_exact_zero_grads_at_8_waves(B, H, T, C, t0, drop):
    _zero_upstream_rows(B, H, T, C, t0, drop)


@pytest.mark.parametrize("B,H,T,C", ATTN_SHAPES[:2] + ATTN8_EXACT)
def test_attention_large_scores(B, H, T, C):
    """q, k at scale 4: scores q.k/sqrt(C) have std 16 and reach about +-80,
    the running max moving from tile to tile. At T=512 this is the large-score
    case of the 8-wave kernels' online softmax."""
    torch.manual_seed(14)
    q, k = randbf(B, H, T, C, scale=4.0), randbf(B, H, T, C, scale=4.0)
    v, do = randbf(B, H, T, C), randbf(B, H, T, C)
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) / math.sqrt(C)
    print(f"EDGE attn big B{B} H{H} T{T} C{C}: max |score| {float(s.abs().max()):.1f}")
    got = _attn_run(q, k, v, do, False)
    for n, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), n
    U.check(f"attn big B{B} H{H} T{T} C{C}", U.attn_figures(q, k, v, do, got))


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("case", U.SOFTMAX_PATHS)
def test_attention_online_softmax_paths_at_8_waves(case, C):
    """Constructed keys (kernel_edge_util.attn_softmax_path_inputs) for the
    paired (C=128) and single-tile (C=64) 8-wave forward:
    first   -- key 0 is every row's max: no tile after the first rescales;
    growing -- the max grows in every tile and sub-tile B's exceeds A's: a
               rescale on every round, alpha from the merged max;
    lastB   -- spike at T-3, in sub-tile B of the last pair (the per-row
               counterpart of test_attention_fwd_spiked_max);
    lastA   -- spike at T-40, in sub-tile A of the last pair.
    o and lse, and dq, dk, dv of the matching backward, per row."""
    B, H, T = 1, 2, 512
    q, k, v, do = U.attn_softmax_path_inputs(case, B, H, T, C, DEV)
    print(f"EDGE attn {case} B{B} H{H} T{T} C{C}: {U.attn_check_path(case, q, k)}")
    got = _attn_run(q, k, v, do, False)
    for n, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), n
    U.check(f"attn {case} B{B} H{H} T{T} C{C}", U.attn_figures(q, k, v, do, got))


# ---------------------------------------------------------------------------
# embedding backward
# ---------------------------------------------------------------------------
def _embed_idx(kind, N, V):
    if kind == "runs":
        idx = torch.randint(0, V, (N,), device=DEV)
        idx[idx == V // 2] = V // 2 + 1          # a row that is never indexed
        idx[:5] = 0                              # runs at token 0 and at V-1
        idx[5:9] = V - 1
        return idx
    if kind == "same":
        return torch.full((N,), 13, device=DEV, dtype=torch.long)
    return torch.randperm(V, device=DEV)[:N]     # "distinct"


@pytest.mark.parametrize("kind", ["runs", "same", "distinct"])
@pytest.mark.parametrize("D", [64, 384, 768, 2112, 4096])
def test_embedding_bwd_sorted_path(D, kind):
    torch.manual_seed(8)
    N = 1021                                     # N % 4 != 0
    V = 97 if kind != "distinct" else N + 3
    idx = _embed_idx(kind, N, V)
    dy = randbf(N, D)
    dw = ops._C.embedding_bwd(dy, idx, V)
    U.check(f"embed sorted {kind} N{N} V{V} D{D}", U.embedding_figures(dy, idx, V, dw))


@pytest.mark.parametrize("D", [8, 72])
def test_embedding_bwd_atomic_path(D):
    torch.manual_seed(8)
    N, V = 4100, 97                              # N over the 4096-block cap
    idx = _embed_idx("runs", N, V)
    dy = randbf(N, D)
    dw = ops._C.embedding_bwd(dy, idx, V)
    U.check(f"embed atomic N{N} V{V} D{D}", U.embedding_figures(dy, idx, V, dw))


# ---------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------
HP = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, wd_over_peak_lr=0.1,
          grad_scale=0.125, clip_norm=1.0)


@pytest.mark.parametrize("n", [3, 1027, 4194327])
@pytest.mark.parametrize("case,sq,step,write", [("clip", 1e4, 3, True),
                                                ("noclip", 1e-8, 1, True),
                                                ("sq0", 0.0, 1, False)])
def test_adamw_elements(n, case, sq, step, write):
    torch.manual_seed(7)
    before = (torch.randn(n, device=DEV), torch.randn(n, device=DEV),
              torch.randn(n, device=DEV).abs() * 0.1,
              torch.randn(n, device=DEV).abs() * 0.01)
    master, grad, m, v = (t.clone() for t in before)
    sq_sum = torch.tensor(sq, device=DEV)
    hp = dict(HP, step=step)
    SENT = -7.0
    out16 = torch.full((n,), SENT, device=DEV, dtype=BF)
    if write:
        ops.adamw_step(master, grad, m, v, out16, sq_sum=sq_sum, **hp)
        assert torch.equal(out16, master.to(BF))
    else:
        # a real buffer with write_bf16=False must stay untouched
        ops._C.adamw_step(master, grad, m, v, out16, False, sq_sum,
                          hp["lr"], hp["beta1"], hp["beta2"], hp["eps"],
                          hp["wd_over_peak_lr"], hp["grad_scale"], hp["clip_norm"], step)
        assert bool((out16 == SENT).all())
        # and the wrapper with out_bf16=None computes the same update
        m2, g2, mm2, v2 = (t.clone() for t in before)
        ops.adamw_step(m2, g2, mm2, v2, None, sq_sum=sq_sum, **hp)
        assert torch.equal(m2, master) and torch.equal(mm2, m) and torch.equal(v2, v)
    assert torch.equal(grad, before[1])
    U.check(f"adamw {case} n{n}", U.adamw_figures(before, sq_sum, hp, (master, m, v)))


# ---------------------------------------------------------------------------
# GELU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dyk", ["ones", "random"])
def test_gelu_every_bf16_input(dyk):
    torch.manual_seed(10)
    x = U.gelu_all_inputs(DEV)
    dy = torch.ones_like(x) if dyk == "ones" else randbf(x.numel())
    y = ops._C.gelu_fwd(x)
    dx = ops._C.gelu_bwd(dy, x)
    U.check(f"gelu exhaustive dy={dyk}", U.gelu_figures(x, dy, y, dx))


def test_gelu_grid_stride_and_fallback():
    torch.manual_seed(10)
    n = 16777216 + 24                            # one trip is 8192*256*8 elements
    x = randbf(n, scale=3.0)
    dy = randbf(n)
    y = ops._C.gelu_fwd(x)
    dx = ops._C.gelu_bwd(dy, x)
    figs = U.gelu_figures(x, dy, y, dx)
    # the flip-count cap is set on the exhaustive sweep; here only the tolerance
    U.check(f"gelu n{n}", [f for f in figs if f.name.endswith("err_over_tol")])
    del x, dy, y, dx, figs
    xs = randbf(1003, scale=3.0).requires_grad_(True)      # numel % 8 != 0
    ys = ops.gelu(xs)
    dys = randbf(1003)
    ys.backward(dys)
    figs = U.gelu_figures(xs.detach(), dys, ys.detach(), xs.grad)
    U.check("gelu n1003 fallback", [f for f in figs if f.name.endswith("err_over_tol")])


# ---------------------------------------------------------------------------
# environment-gated kernel variants: one fresh child process per group
# ---------------------------------------------------------------------------
VARIANT_GROUPS = [
    ("MIDGPT_ATTN_DKV_NW4",),
]
ALL_SWITCHES = sorted({s for g in VARIANT_GROUPS for s in g})


_CHILD_DIED = []     # groups whose worker died by signal or timed out


@pytest.mark.parametrize("group", VARIANT_GROUPS, ids=lambda g: "+".join(s[7:] for s in g))
def test_env_gated_variants_meet_the_default_bounds(group):
    """The switches are read once into statics, so each group needs a fresh
    process. One child at a time, each with its own time limit; once a child
    has died by signal or timed out, the remaining groups fail without
    starting theirs."""
    if _CHILD_DIED:
        pytest.fail(f"not started: the worker of {_CHILD_DIED[0]} died or timed out")
    worker = os.path.join(HERE, "_edge_variant_worker.py")
    env = {k: v for k, v in os.environ.items() if k not in ALL_SWITCHES}
    env.update({s: "1" for s in group})
    try:
        r = subprocess.run([sys.executable, worker], env=env, capture_output=True,
                           text=True, timeout=180)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append(group)
        pytest.fail(f"{group}: worker timed out")
    if r.returncode != 0:      # a figure over its bound still exits 0: this is a crash
        _CHILD_DIED.append(group)
        how = f"signal {-r.returncode}" if r.returncode < 0 else f"exit {r.returncode}"
        pytest.fail(f"{group}: worker died ({how})\n{r.stderr[-2000:]}")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for line in res["lines"]:
        print(f"EDGE [{'+'.join(s[7:] for s in group)}] {line}")
    assert set(group) <= set(res["env"])
    assert not res["over"], f"{group}: {res['over']}"
