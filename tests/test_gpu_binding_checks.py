"""Argument checks of the ``ops._C`` entry points (csrc/bindings.cpp).

Every pointer a kernel gets comes from one helper family that checks device,
contiguity, dtype and the exact shape or element count the kernel addresses.
For each argument that used to reach a kernel unchecked there is one call
here that must raise ``RuntimeError``. Every bad argument is wrong in a
harmless direction (a longer buffer, a wider dtype, a strided view of a
larger buffer, more dimensions over the same memory), so that no call could
read or write out of bounds even with the check missing. After the rejections
the same tensors make one valid call, compared with ``ref_backend`` under the
bound test_gpu_backend_parity.py uses for that entry point: they were
acceptable apart from the one flaw. Nothing else here launches a kernel.

The device, contiguity and dtype branches of each helper are taken once each
through an argument that was already rejected before the helpers existed.
``f32_out`` serves only adamw_step, whose first tensor is also the device
anchor and whose other buffers are new checks (no host tensors there): its
device branch is the shared ``ptr`` code the other helpers exercise."""
import pytest
import torch

import kernel_edge_util as U

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from midgpt_amd import ops
    from midgpt_amd.ops import ref_backend
    from midgpt_amd.ops import reference as ref
    assert ops.have_ext(), f"HIP extension must be built: {ops._C_ERR}"

DEV = "cuda:0"
BF = torch.bfloat16
EPS = 1e-6
N = 5
# test_gpu_backend_parity.py (which names the test each constant comes from)
RMS_Y, RMS_DX = 1e-2, 2e-2
GELU_Y, GELU_DX = 1e-2, 2e-2
EMBED = 1e-2
CE_LOSS, CE_DLOGITS = 1e-3, 2e-2
ADAMW = 1e-6
PROBE = 2e-2        # test_gpu_kernels.py::test_mfma_layout_probe / _pack_probe
MLP_GRAD = 3e-2     # test_gpu_kernels.py::test_fused_mlp_matches_reference


def randbf(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(BF)


def strided(t):
    """t's values as every other element of a buffer twice as long."""
    big = torch.zeros(2 * t.numel(), device=t.device, dtype=t.dtype)
    view = big[::2]
    view.copy_(t.reshape(-1))
    assert not view.is_contiguous() or t.numel() <= 1
    return view


def rejects(fn, *args):
    with pytest.raises(RuntimeError):
        fn(*args)


def close(case, got, want, bound):
    assert got.shape == want.shape and got.dtype == want.dtype, (case, got.shape, want.shape)
    e = U.whole_relerr(got, want)
    print(f"BINDING {case}: relerr={e:.3e} bound={bound:.0e}")
    assert e < bound, (case, e, bound)


# ---------------------------------------------------------------------------
# Arguments that gained a shape or numel check
# ---------------------------------------------------------------------------
def test_rmsnorm():
    torch.manual_seed(2)
    C = ops._C
    D = 64
    x, dy = randbf(N, D), randbf(N, D)
    w = torch.randn(D, device=DEV)
    rejects(C.rmsnorm_fwd, x.view(N, 8, 8), None, EPS)                # x.dim()
    rejects(C.rmsnorm_fwd, x, torch.randn(D + 8, device=DEV), EPS)    # w longer than D
    y, invrms = C.rmsnorm_fwd(x, None, EPS)
    yr, invr = ref_backend.rmsnorm_fwd(x, None, EPS)
    close("rmsnorm_fwd y", y, yr, RMS_Y)
    close("rmsnorm_fwd invrms", invrms, invr, RMS_Y)
    close("rmsnorm_fwd weighted", C.rmsnorm_fwd(x, w, EPS)[0],
          ref_backend.rmsnorm_fwd(x, w, EPS)[0], RMS_Y)
    rejects(C.rmsnorm_bwd, randbf(N + 1, D), x, None, invrms, EPS)    # dy: one more row
    rejects(C.rmsnorm_bwd, dy.float(), x, None, invrms, EPS)          # dy: fp32 for bf16
    rejects(C.rmsnorm_bwd, dy, x, None, torch.ones(N + 1, device=DEV), EPS)
    rejects(C.rmsnorm_bwd, dy, x, None, strided(invrms), EPS)
    dx, none = C.rmsnorm_bwd(dy, x, None, invrms, EPS)
    assert none is None
    close("rmsnorm_bwd", dx, ref_backend.rmsnorm_bwd(dy, x, None, invrms, EPS)[0], RMS_DX)


def test_cross_entropy():
    torch.manual_seed(6)
    C = ops._C
    V = 72                                           # vector body and scalar tail
    logits = randbf(N, V, scale=2.0)
    targets = torch.tensor([0, V - 1, 63, 64, 7], device=DEV)
    longer = torch.cat([targets, targets[:1]])
    rejects(C.ce_fwd, logits.view(1, N, V), targets)                  # logits.dim()
    rejects(C.ce_fwd, logits, longer)                                 # targets of N + 1
    loss, lse = C.ce_fwd(logits, targets)
    loss_r, lse_r = ref_backend.ce_fwd(logits, targets)
    close("ce_fwd loss", loss, loss_r, CE_LOSS)
    close("ce_fwd lse", lse, lse_r, CE_LOSS)
    gscale = torch.tensor([3.5], device=DEV)
    rejects(C.ce_bwd, logits, longer, lse, gscale)
    rejects(C.ce_bwd, logits, strided(targets), lse, gscale)
    rejects(C.ce_bwd, logits, targets, torch.ones(N + 1, device=DEV), gscale)
    rejects(C.ce_bwd, logits, targets, lse.double(), gscale)          # fp64 for fp32
    rejects(C.ce_bwd, logits, targets, strided(lse), gscale)
    rejects(C.ce_bwd, logits, targets, lse, torch.ones(2, device=DEV))
    close("ce_bwd", C.ce_bwd(logits, targets, lse, gscale),
          ref_backend.ce_bwd(logits, targets, lse, gscale), CE_DLOGITS)


HP = (1e-3, 0.9, 0.95, 1e-8, 0.1, 0.125, 1.0, 3)    # test_gpu_backend_parity.py
SENT = -7.0


def _adamw_buffers(n):
    torch.manual_seed(7)
    return [torch.randn(n, device=DEV), torch.randn(n, device=DEV),
            torch.randn(n, device=DEV).abs() * 0.1, torch.randn(n, device=DEV).abs() * 0.01,
            torch.full((n,), SENT, device=DEV, dtype=BF)]


def test_adamw_step():
    n = 1032
    before = _adamw_buffers(n)
    bufs = [t.clone() for t in before]
    sq = (before[1] * before[1]).sum()
    step = ops._C.adamw_step
    for i in (1, 2, 3, 4):                           # grad, m, v, out_bf16
        for bad in (torch.zeros(n + 8, device=DEV, dtype=bufs[i].dtype),   # longer
                    strided(bufs[i])):
            args = list(bufs)
            args[i] = bad
            rejects(step, *args, True, sq, *HP)
    args = list(bufs)
    args[4] = torch.zeros(n, device=DEV)                                   # fp32 for bf16
    rejects(step, *args, True, sq, *HP)
    rejects(step, *bufs, True, torch.ones(2, device=DEV), *HP)             # sq_sum of 2
    torch.cuda.synchronize()
    for got, was in zip(bufs, before):                                     # nothing written
        assert torch.equal(got, was)
    want = [t.clone() for t in before]
    assert step(*bufs, True, sq, *HP) is None
    ref_backend.adamw_step(*want, True, sq, *HP)
    for name, g, w in zip(("master", "grad", "m", "v"), bufs, want):
        close(f"adamw_step {name}", g, w, ADAMW)
    assert torch.equal(bufs[4], want[4]) and torch.equal(bufs[4], bufs[0].to(BF))


def test_gelu():
    torch.manual_seed(10)
    C = ops._C
    x, dy = randbf(N, 64, scale=3.0), randbf(N, 64)
    close("gelu_fwd", C.gelu_fwd(x), ref_backend.gelu_fwd(x), GELU_Y)
    rejects(C.gelu_bwd, dy.float(), x)                                # dy: fp32 for bf16
    rejects(C.gelu_bwd, dy, x.float())                                # x: fp32 for bf16
    rejects(C.gelu_bwd, randbf(N * 64 + 8), x)                        # dy longer than x
    rejects(C.gelu_bwd, strided(dy).view(N, 64), x)
    close("gelu_bwd", C.gelu_bwd(dy, x), ref_backend.gelu_bwd(dy, x), GELU_DX)


@pytest.mark.parametrize("D", [64, 24], ids=["sorted", "atomic"])
def test_embedding_bwd(D):
    torch.manual_seed(8)
    V = 11
    dy = randbf(N, D)
    idx = torch.tensor([0, V - 1, 3, 3, 0], device=DEV)
    rejects(ops._C.embedding_bwd, dy, torch.cat([idx, idx[:1]]), V)   # idx of N + 1
    rejects(ops._C.embedding_bwd, dy.view(N, D // 8, 8), idx, V)      # dy.dim()
    rejects(ops._C.embedding_bwd, dy, strided(idx), V)
    close(f"embedding_bwd D{D}", ops._C.embedding_bwd(dy, idx, V),
          ref_backend.embedding_bwd(dy, idx, V), EMBED)


def test_probes():
    torch.manual_seed(0)
    C = ops._C
    A, B = torch.randn(32, 16, device=DEV), torch.randn(16, 32, device=DEV)
    M, B2 = torch.randn(32, 32, device=DEV), torch.randn(32, 32, device=DEV)
    rejects(C.probe_mfma, M, B)                                       # A of 32x32, longer
    rejects(C.probe_mfma, A, B2)                                      # B of 32x32, longer
    rejects(C.probe_mfma, A.double(), B)
    rejects(C.probe_pack, torch.randn(33, 32, device=DEV), B2)
    rejects(C.probe_pack, M, B2.double())
    rejects(C.probe_pack, M, strided(B2).view(32, 32))
    rnd = lambda t: t.to(BF).float()
    close("probe_mfma", C.probe_mfma(A, B), rnd(A) @ rnd(B), PROBE)
    close("probe_pack", C.probe_pack(M, B2), rnd(M.t()) @ rnd(B2), PROBE)


def test_matmul_dgelu():
    torch.manual_seed(8)
    M, N2, NN = 128, 128, 256
    dy, w2, h = randbf(M, N2), randbf(N2, NN, scale=0.05), randbf(M, NN)
    f = ops._C.matmul_dgelu
    rejects(f, dy.float(), w2, h)                                     # fp32 for bf16
    rejects(f, dy, w2.float(), h)
    rejects(f, dy, w2, h.float())
    rejects(f, dy, w2, h.view(M, NN, 1))                              # dim() == 2
    rejects(f, dy.view(1, M, N2), w2, h)
    want = ref_backend.gelu_bwd(dy.float() @ w2.float(), h)
    close("matmul_dgelu", f(dy, w2, h), want, MLP_GRAD)


# ---------------------------------------------------------------------------
# Device, contiguity and dtype branch of each helper, through arguments that
# were rejected before the helpers existed
# ---------------------------------------------------------------------------
def test_helper_branches_bf16_and_f32():
    """bf16: add_rmsnorm_fwd's r. Optional bf16: add_rmsnorm_bwd's ds.
    f32: add_rmsnorm_bwd's invrms. The first tensor: gelu_fwd's x."""
    torch.manual_seed(11)
    C = ops._C
    x, r, dy, ds = (randbf(N, 64) for _ in range(4))
    rejects(C.gelu_fwd, x.cpu())
    rejects(C.add_rmsnorm_fwd, x, r.cpu(), EPS)
    rejects(C.add_rmsnorm_fwd, x, strided(r).view(N, 64), EPS)
    rejects(C.add_rmsnorm_fwd, x, r.float(), EPS)
    s, y, invrms = C.add_rmsnorm_fwd(x, r, EPS)
    assert s.shape == y.shape == (N, 64) and invrms.shape == (N,)
    for bad in (ds.cpu(), strided(ds).view(N, 64), ds.float()):
        rejects(C.add_rmsnorm_bwd, bad, dy, s, invrms)
    for bad in (invrms.cpu(), strided(invrms), invrms.double()):
        rejects(C.add_rmsnorm_bwd, ds, dy, s, bad)
    assert C.add_rmsnorm_bwd(ds, dy, s, invrms).shape == (N, 64)
    assert C.add_rmsnorm_bwd(None, dy, s, invrms).shape == (N, 64)


def test_helper_branches_out_i64_i32():
    """bf16_out: attn_decode's caches. f32_out: adamw_step's master. i64:
    ce_fwd's targets (fp64 zeros stand in for a wrong dtype: as int64 they are
    index 0). i32: kv_append_ragged's pos_dev."""
    torch.manual_seed(12)
    C = ops._C
    B, H, TMAX, HD = 2, 1, 8, 64
    q = randbf(B, H, 1, HD)
    kc, vc = randbf(B, H, TMAX, HD), randbf(B, H, TMAX, HD)
    big = randbf(B, H, 2 * TMAX, HD)
    rejects(C.attn_decode, q, kc.cpu(), vc, 4, 1)
    rejects(C.attn_decode, q, big[:, :, ::2], vc, 4, 1)
    rejects(C.attn_decode, q, kc.float(), vc, 4, 1)
    assert C.attn_decode(q, kc, vc, 4, 1).shape == (B, 1, H, HD)

    n = 16
    bufs = _adamw_buffers(n)
    sq = torch.ones((), device=DEV)
    rejects(C.adamw_step, strided(bufs[0]), *bufs[1:], True, sq, *HP)
    rejects(C.adamw_step, bufs[0].double(), *bufs[1:], True, sq, *HP)

    logits = randbf(N, 72)
    targets = torch.zeros(N, dtype=torch.long, device=DEV)
    rejects(C.ce_fwd, logits, targets.cpu())
    rejects(C.ce_fwd, logits, strided(targets))
    rejects(C.ce_fwd, logits, targets.double())

    qkv = randbf(B, 1, 3, H, HD)
    qw, kw = torch.ones(HD, device=DEV), torch.ones(HD, device=DEV)
    sin, cos = (t.contiguous() for t in ref.rope_tables(HD, TMAX, device=DEV))
    pos_host = torch.tensor([2, 3])
    pos_dev = pos_host.to(device=DEV, dtype=torch.int32)
    for bad in (pos_dev.cpu(), pos_dev.long(), strided(pos_dev)):
        rejects(C.kv_append_ragged, qkv, qw, kw, sin, cos, kc, vc, bad, pos_host, EPS)
    kc0, vc0 = kc.clone(), vc.clone()
    out = C.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc, pos_dev, pos_host, EPS)
    assert out.shape == (B, H, 1, HD)
    for b, p in enumerate(pos_host.tolist()):          # only row pos[b] was written
        keep = [t for t in range(TMAX) if t != p]
        assert torch.equal(kc[b, :, keep], kc0[b, :, keep])
        assert torch.equal(vc[b, :, keep], vc0[b, :, keep])
        assert torch.equal(vc[b, :, p], qkv[b, 0, 2])


# ---------------------------------------------------------------------------
def test_zero_rows():
    """An empty grid launches nothing: empty results of the right shape and
    dtype where the launch used to fail."""
    C = ops._C
    x = torch.empty(0, 64, device=DEV, dtype=BF)
    y, invrms = C.rmsnorm_fwd(x, None, EPS)
    assert (y.shape, y.dtype, invrms.shape, invrms.dtype) == ((0, 64), BF, (0,), torch.float32)
    dx, _ = C.rmsnorm_bwd(x, x, None, invrms, EPS)
    assert dx.shape == (0, 64) and dx.dtype == BF
    g = C.gelu_fwd(x)
    assert g.shape == (0, 64) and g.dtype == BF
    assert C.gelu_bwd(x, x).shape == (0, 64)
    logits = torch.empty(0, 72, device=DEV, dtype=BF)
    targets = torch.empty(0, device=DEV, dtype=torch.long)
    loss, lse = C.ce_fwd(logits, targets)
    assert loss.shape == () and loss.dtype == torch.float32 and float(loss) == 0.0
    assert lse.shape == (0,) and lse.dtype == torch.float32
    dl = C.ce_bwd(logits, targets, lse, torch.ones(1, device=DEV))
    assert dl.shape == (0, 72) and dl.dtype == BF
    s, y, invrms = C.add_rmsnorm_fwd(x, x, EPS)
    assert s.shape == y.shape == (0, 64) and s.dtype == y.dtype == BF
    assert invrms.shape == (0,) and invrms.dtype == torch.float32
    assert C.add_rmsnorm_bwd(None, x, s, invrms).shape == (0, 64)


def test_rejected_adamw_step_writes_nothing():
    """The end check: after everything above, a rejected call has left the
    sentinel-filled output (and the state) as it was."""
    n = 1032
    before = _adamw_buffers(n)
    bufs = [t.clone() for t in before]
    sq = torch.ones((), device=DEV)
    rejects(ops._C.adamw_step, *bufs, True, torch.ones(2, device=DEV), *HP)
    rejects(ops._C.adamw_step, *bufs[:3], torch.zeros(n + 8, device=DEV), bufs[4], True, sq, *HP)
    torch.cuda.synchronize()
    assert bool((bufs[4] == SENT).all())
    for got, was in zip(bufs, before):
        assert torch.equal(got, was)
