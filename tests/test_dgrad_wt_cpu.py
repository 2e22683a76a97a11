"""CPU: the ref_backend mirror of the batched transpose, and ``ops.linear_wt``
with an image bound by hand against ``F.linear`` under autograd."""

import pytest
import torch
import torch.nn.functional as F

from midgpt_amd import ops
from midgpt_amd.config import GPTConfig
from midgpt_amd.models.gpt import GPT, Linear
from midgpt_amd.ops import ref_backend
from midgpt_amd.parallel.engine import ShardedAdamW

# The table of tests/test_gpu_dgrad_wt.py: (rows, cols, src offset off
# alignment by, dst offset off alignment by).
MATRICES = [(64, 64, 0, 0), (1, 8, 0, 0), (72, 200, 0, 0), (130, 65, 0, 0),
            (128, 192, 0, 0), (256, 192, 3, 0), (64, 128, 0, 5)]
GUARD = 8
POISON = -77.0


def _layout():
    entries, so, do = [], 0, GUARD
    for rows, cols, s_odd, d_odd in MATRICES:
        so = -(-so // 8) * 8 + s_odd
        do = -(-do // 8) * 8 + d_odd
        entries.append((so, do, rows, cols))
        so += rows * cols + 1
        do += rows * cols + GUARD
    return entries, so, do


def test_api_lists():
    assert ops.TRANSPOSE_API == ("transpose_batched",)
    for name in ops.TRANSPOSE_API:
        assert callable(getattr(ref_backend, name))
        assert name not in (ops.BACKEND_API + ops.RAGGED_API + ops.SAMPLING_API
                            + ops.SLOT_API + ops.PAGED_API)
    if ops.have_ext():
        assert callable(ops._C.transpose_batched)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64])
def test_ref_transpose_table(dtype):
    entries, ns, nd = _layout()
    g = torch.Generator().manual_seed(7)
    src = torch.randn(ns, generator=g).to(dtype)
    dst = torch.full((nd,), POISON, dtype=dtype)
    tdev, thost = ops.transpose_table(entries)
    assert thost.shape == (len(entries), 5) and thost.dtype == torch.int64
    assert thost[:, 4].tolist() == [0, 1, 2, 10, 16, 22, 34]
    ops.transpose_batched(src, dst, tdev, thost)
    inside = torch.zeros(nd, dtype=torch.bool)
    for so, do, rows, cols in entries:
        want = src[so:so + rows * cols].view(rows, cols).t().contiguous()
        assert torch.equal(dst[do:do + rows * cols].view(cols, rows), want)
        inside[do:do + rows * cols] = True
    assert bool((dst[~inside] == POISON).all())


def test_ref_transpose_rejects_bad_tables():
    src, dst = torch.zeros(4096), torch.zeros(4096)
    for entries in ([(1, 0, 64, 64)], [(0, 1, 64, 64)], [(0, 0, 0, 8)]):
        t, h = ops.transpose_table(entries)
        with pytest.raises(RuntimeError):
            ops.transpose_batched(src, dst, t, h)
    t, h = ops.transpose_table([(0, 0, 8, 8), (64, 64, 8, 8)])
    h = h.clone()
    h[1, 4] = 5
    with pytest.raises(RuntimeError):
        ops.transpose_batched(src, dst, t, h)


@pytest.mark.parametrize("shape_x", [(256, 192), (4, 64, 192)])
@pytest.mark.parametrize("x_grad", [True, False])
def test_linear_wt_fp64_matches_autograd(shape_x, x_grad):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(*shape_x, generator=g, dtype=torch.float64)
    w = torch.randn(320, 192, generator=g, dtype=torch.float64) / 192 ** 0.5
    dy = torch.randn(*shape_x[:-1], 320, generator=g, dtype=torch.float64)

    def run(fn):
        xa = x.clone().requires_grad_(x_grad)
        wa = w.clone().requires_grad_(True)
        y = fn(xa, wa)
        y.backward(dy)
        return y.detach(), xa.grad, wa.grad

    y0, dx0, dw0 = run(F.linear)
    wt = w.t().contiguous()
    y1, dx1, dw1 = run(lambda xa, wa: ops.linear_wt(xa, wa, wt))
    torch.testing.assert_close(y1, y0, rtol=1e-12, atol=0)
    torch.testing.assert_close(dw1, dw0, rtol=1e-12, atol=1e-12)
    if x_grad:
        torch.testing.assert_close(dx1, dx0, rtol=1e-12, atol=1e-12)
    else:
        assert dx1 is None and dx0 is None


def test_cpu_engine_and_bare_model_bind_no_image():
    cfg = GPTConfig(block_size=16, vocab_size=37, n_layer=1, n_head=2, n_embd=32,
                    dropout=0.0)
    torch.manual_seed(0)
    model = GPT(cfg)
    linears = [m for m in model.modules() if isinstance(m, Linear)]
    assert linears and all(m.weight_t is None for m in linears)
    assert "weight_t" not in "".join(model.state_dict().keys())
    engine = ShardedAdamW(model, compute_dtype=torch.float32, zero=False)
    assert engine.flat_wt is None
    assert all(m.weight_t is None for m in linears)
    engine.refresh_dgrad_images()        # nothing to do, no error
