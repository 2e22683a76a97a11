"""The two implementations of ``ops.BACKEND_API`` side by side on the GPU:
every entry point is called as ``_C.name(*args)`` and as
``ref_backend.name(*args)`` with the same tensors (in-place buffers cloned)
and must give the same number of results with the same shapes and dtypes,
and values within the threshold that the existing GPU test of that entry
point uses (sources named at each constant; the fp32 per-row statistics that
rmsnorm_fwd, qkv_prep_fwd and ce_fwd return have no whole-tensor constant of
their own there and take that of the result they are statistics of).

Shapes are the smallest at which each kernel can still go wrong. Every
figure is printed as ``PARITY <case> [i]: relerr=.. bound=..``."""
import pytest
import torch

import kernel_edge_util as U
from decode_util import decode_math

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from midgpt_amd import ops
    from midgpt_amd.ops import ref_backend
    from midgpt_amd.ops import reference as ref
    assert ops.have_ext(), f"HIP extension must be built: {ops._C_ERR}"

DEV = "cuda:0"
BF = torch.bfloat16
EPS = 1e-6
P, SEED = 0.2, 7          # test_gpu_attn_dropout.py
NAN = float("nan")

# test_gpu_kernels.py, whole-tensor relative L2 error (``relerr`` there)
RMS_Y, RMS_DX = 1e-2, 2e-2                    # test_rmsnorm_fwd_bwd
PREP_QK, PREP_V, PREP_BWD = 1e-2, 1e-3, 2e-2  # test_qkv_prep_fwd_bwd
ATTN_O, ATTN_LSE, ATTN_BWD = 2e-2, 1e-3, 4e-2  # test_attention_fwd / _bwd; the same
#                               three in test_gpu_attn_dropout.py under dropout
GELU_Y, GELU_DX = 1e-2, 2e-2                  # test_gelu_fwd_bwd
EMBED = 1e-2                                  # test_embedding_bwd
CE_LOSS, CE_DLOGITS = 1e-3, 2e-2              # test_cross_entropy_fwd_bwd
ADAMW = 1e-6                                  # test_adamw_step_gpu_matches_cpu;
#                               the bf16 copy is compared with torch.equal there
# kv_append: test_gpu_decode.py::test_kv_append_bit_exact_with_qkv_prep holds it
# to qkv_prep_fwd's bits, so qkv_prep_fwd's constants are its constants.
# attn_decode: test_gpu_decode.py judges it by U.check(fig_rows(...)) against
# fp64, bound FACTOR x the fp32 yardstick; the same here, for both backends.

COMPARED = set()


def compares(*names):
    """Declares, at import, which entry points a test puts side by side."""
    COMPARED.update(names)
    return lambda f: f


def randbf(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(BF)


def _results(r):
    if r is None:
        return []
    return [r] if isinstance(r, torch.Tensor) else list(r)


def both(name, *args):
    """(_C results, ref_backend results) of one entry point, as lists."""
    assert name in COMPARED, name
    return (_results(getattr(ops._C, name)(*args)),
            _results(getattr(ref_backend, name)(*args)))


def same(case, got, want, bounds):
    assert len(got) == len(want) == len(bounds), (case, len(got), len(want))
    for i, (g, w, bound) in enumerate(zip(got, want, bounds)):
        if g is None or w is None:
            assert g is None and w is None, (case, i)
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, \
            (case, i, g.shape, w.shape, g.dtype, w.dtype)
        e = U.whole_relerr(g, w)
        print(f"PARITY {case} [{i}]: relerr={e:.3e} bound={bound:.0e}")
        assert e < bound, (case, i, e, bound)


# ---------------------------------------------------------------------------
@compares("rmsnorm_fwd", "rmsnorm_bwd")
def test_rmsnorm():
    """(3, 8): test_gpu_kernel_edges.py::test_rmsnorm_bf16_rows, with its
    zero row and its row at 1e3."""
    torch.manual_seed(2)
    x = torch.randn(3, 8, device=DEV)
    x[0] = 0.0
    x[1] *= 1e3
    x, dy = x.to(BF), randbf(3, 8)
    got, want = both("rmsnorm_fwd", x, None, EPS)
    same("rmsnorm_fwd", got, want, [RMS_Y, RMS_Y])
    invrms = got[1]
    same("rmsnorm_bwd", *both("rmsnorm_bwd", dy, x, None, invrms, EPS), [RMS_DX, None])


@pytest.mark.parametrize("B,T,H,C", [(1, 5, 2, 64), (1, 3, 1, 128)])
@compares("qkv_prep_fwd", "qkv_prep_bwd")
def test_qkv_prep(B, T, H, C):
    torch.manual_seed(3)
    qkv = randbf(B, T, 3, H, C)
    qw, kw = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    sin, cos = ref.rope_tables(C, T, device=DEV)
    got, want = both("qkv_prep_fwd", qkv, qw, kw, sin, cos, EPS)
    same(f"qkv_prep_fwd C{C}", got, want, [PREP_QK, PREP_QK, PREP_V, PREP_QK, PREP_QK])
    assert torch.equal(got[2], want[2])                      # V passes through
    grads = [randbf(B, H, T, C) for _ in range(3)]
    same(f"qkv_prep_bwd C{C}",
         *both("qkv_prep_bwd", *grads, qkv, qw, kw, sin, cos, got[3], got[4], EPS),
         [PREP_BWD] * 3)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "p0.2"])
@pytest.mark.parametrize("B,H,T,C", [(1, 2, 128, 64), (1, 1, 256, 128)])
@compares("attn_fwd", "attn_bwd", "attn_fwd_dropout", "attn_bwd_dropout")
def test_attention(B, H, T, C, drop):
    """4-wave path and the 8-wave paired-tile forward. Under dropout the
    host mask is the bit-exact mirror of the kernels', so the dropped
    outputs are comparable element for element."""
    torch.manual_seed(4)
    q, k, v, do = (randbf(B, H, T, C) for _ in range(4))
    tail = (P, SEED) if drop else ()
    sfx = "_dropout" if drop else ""
    got, want = both("attn_fwd" + sfx, q, k, v, *tail)
    same(f"attn_fwd{sfx} T{T} C{C}", got, want, [ATTN_O, ATTN_LSE])
    o, lse = got
    same(f"attn_bwd{sfx} T{T} C{C}",
         *both("attn_bwd" + sfx, do, q, k, v, o, lse, *tail), [ATTN_BWD] * 3)


@compares("gelu_fwd", "gelu_bwd")
def test_gelu():
    """Every finite bf16 |x| <= 64: test_gpu_kernel_edges.py::
    test_gelu_every_bf16_input, that file's smallest gelu case."""
    torch.manual_seed(10)
    x = U.gelu_all_inputs(DEV)
    dy = randbf(x.numel())
    same("gelu_fwd", *both("gelu_fwd", x), [GELU_Y])
    same("gelu_bwd", *both("gelu_bwd", dy, x), [GELU_DX])


@pytest.mark.parametrize("N,V,D", [(4100, 97, 8), (1021, 97, 64)])
@compares("embedding_bwd")
def test_embedding_bwd(N, V, D):
    """test_gpu_kernel_edges.py's smallest case of the atomic path and of
    the sorted path (D % 64 == 0), with runs of one token and an unused row."""
    torch.manual_seed(8)
    idx = torch.randint(0, V, (N,), device=DEV)
    idx[idx == V // 2] = V // 2 + 1
    idx[:5] = 0
    idx[5:9] = V - 1
    dy = randbf(N, D)
    got, want = both("embedding_bwd", dy, idx, V)
    same(f"embedding_bwd D{D}", got, want, [EMBED])
    assert bool((got[0][V // 2] == 0).all()) and bool((want[0][V // 2] == 0).all())


@compares("ce_fwd", "ce_bwd")
def test_cross_entropy():
    """(37, 65): test_gpu_kernel_edges.py::test_cross_entropy_rows, an
    unpadded vocab with targets at both ends and in the scalar tail."""
    torch.manual_seed(6)
    N, V = 37, 65
    logits = randbf(N, V, scale=2.0)
    targets = torch.randint(0, V, (N,), device=DEV)
    targets[0], targets[1], targets[2], targets[3] = 0, V - 1, 63, 64
    got, want = both("ce_fwd", logits, targets)
    same("ce_fwd", got, want, [CE_LOSS, CE_LOSS])
    gscale = torch.tensor([3.5], device=DEV)
    same("ce_bwd", *both("ce_bwd", logits, targets, got[1], gscale), [CE_DLOGITS])


@pytest.mark.parametrize("write", [True, False])
@compares("adamw_step")
def test_adamw_step(write):
    """n = 1027: the 4-wide body and a tail of 3. Hyperparameters of
    test_adamw_step_gpu_matches_cpu."""
    torch.manual_seed(7)
    n = 1027
    before = [torch.randn(n, device=DEV), torch.randn(n, device=DEV),
              torch.randn(n, device=DEV).abs() * 0.1,
              torch.randn(n, device=DEV).abs() * 0.01,
              torch.full((n,), -7.0, device=DEV, dtype=BF)]
    sq = (before[1] * before[1]).sum()
    hp = (1e-3, 0.9, 0.95, 1e-8, 0.1, 0.125, 1.0, 3)
    bufs_c = [t.clone() for t in before]
    bufs_r = [t.clone() for t in before]
    got, want = (_results(getattr(impl, "adamw_step")(*bufs, write, sq, *hp))
                 for impl, bufs in ((ops._C, bufs_c), (ref_backend, bufs_r)))
    assert got == [] and want == []
    same(f"adamw_step write{int(write)}", bufs_c[:4], bufs_r[:4], [ADAMW] * 4)
    assert torch.equal(bufs_c[1], before[1]) and torch.equal(bufs_r[1], before[1])
    assert torch.equal(bufs_c[4], bufs_r[4])
    assert torch.equal(bufs_c[4], bufs_c[0].to(BF) if write else before[4])


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("Tn", [1, 3])
@compares("kv_append")
def test_kv_append(Tn, C):
    torch.manual_seed(31)
    B, H, TMAX, pos = 1, 2, 128, 5
    qkv = randbf(B, Tn, 3, H, C)
    qw = 1.0 + 0.1 * torch.randn(C, device=DEV)
    kw = 1.0 + 0.1 * torch.randn(C, device=DEV)
    sin, cos = ref.rope_tables(C, TMAX, device=DEV)
    kc, vc = randbf(B, H, TMAX, C), randbf(B, H, TMAX, C)
    caches_c, caches_r = (kc.clone(), vc.clone()), (kc.clone(), vc.clone())
    got = _results(ops._C.kv_append(qkv, qw, kw, sin, cos, *caches_c, pos, EPS))
    want = _results(ref_backend.kv_append(qkv, qw, kw, sin, cos, *caches_r, pos, EPS))
    rows = slice(pos, pos + Tn)
    same(f"kv_append Tn{Tn} C{C}",
         got + [caches_c[0][:, :, rows], caches_c[1][:, :, rows]],
         want + [caches_r[0][:, :, rows], caches_r[1][:, :, rows]],
         [PREP_QK, PREP_QK, PREP_V])
    for c in (caches_c, caches_r):                 # nothing else was written
        for new, old in zip(c, (kc, vc)):
            assert torch.equal(new[:, :, :pos], old[:, :, :pos])
            assert torch.equal(new[:, :, pos + Tn:], old[:, :, pos + Tn:])


@pytest.fixture(scope="module")
def decode_inputs():
    """Per head dim: q (1,2,16,C) and caches of 320 rows; read-only."""
    out = {}
    for C in (64, 128):
        g = torch.Generator().manual_seed(32 + C)
        out[C] = tuple((torch.randn(1, 2, t, C, generator=g)).to(BF).to(DEV)
                       for t in (16, 320, 320))
    return out


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("num_splits", [0, 2])
@pytest.mark.parametrize("kv_len", [33, 300])
@pytest.mark.parametrize("Tq", [1, 16])
@compares("attn_decode")
def test_attn_decode(decode_inputs, Tq, kv_len, num_splits, C):
    q_all, k_all, v_all = decode_inputs[C]
    q = q_all[:, :, :Tq].contiguous()
    kc, vc = k_all.clone(), v_all.clone()
    kc[:, :, kv_len:] = NAN                        # rows no backend may read
    vc[:, :, kv_len:] = NAN
    got, want = both("attn_decode", q, kc, vc, kv_len, num_splits)
    assert len(got) == len(want) == 1
    assert got[0].shape == want[0].shape == (1, Tq, 2, C)
    assert got[0].dtype == want[0].dtype == BF
    ref64 = decode_math(q, kc, vc, kv_len, torch.float64, False)
    yard = decode_math(q, kc, vc, kv_len, torch.float32, True)
    case = f"C{C} Tq{Tq} kv{kv_len} s{num_splits}"
    U.check("parity decode", [U.fig_rows(f"decode.o _C {case}", got[0], yard, ref64),
                              U.fig_rows(f"decode.o ref_backend {case}", want[0], yard, ref64)])


def test_every_entry_point_is_compared():
    assert COMPARED == set(ops.BACKEND_API), set(ops.BACKEND_API) ^ COMPARED


def test_routing(monkeypatch):
    x = torch.zeros(8, device=DEV)
    monkeypatch.setenv("MIDGPT_FORCE_REF", "1")
    assert ops._backend(x) is ref_backend
    monkeypatch.delenv("MIDGPT_FORCE_REF")
    assert ops._backend(x) is ops._C
