"""GPU: the transposed weight images behind the dgrad GEMMs.

- ``ops.transpose_batched`` (csrc/transpose.hip): bit-equal to
  ``.t().contiguous()`` for one table of matrices that takes every path of the
  kernel, with a poisoned destination and guard elements around the images.
- ``ops.linear_wt``: y and dW bit-equal to ``F.linear`` under autograd (with
  the repeat guard of test_gpu_glue_fusion.py); dx, whose summation order
  differs, within twice autograd's own per-row error against fp64.
- ``ShardedAdamW``: every bound image equals ``weight.t()`` after every writer
  of the weights; MIDGPT_DGRAD_WT=0 binds none; cache on and off train alike.

The engine model is the issue's 2-layer GPT with D=64 and V=65, but with one
head and T=128: the attention kernels take head dim 64 or 128 and T % 128 == 0
only, so H=2 (head dim 32) and T=32 cannot run on the GPU path at all. D and V
fix the shapes that are transposed (65 x 64 is ragged and lands on a buffer
offset that is no multiple of 8 elements further on), and they are kept."""

import pytest
import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from midgpt_amd import ops
    assert ops.have_ext()

from kernel_edge_util import row_err
from midgpt_amd.config import GPTConfig
from midgpt_amd.models.gpt import GPT, Linear
from midgpt_amd.parallel.engine import ShardedAdamW
from test_gpu_glue_fusion import same

DEV = "cuda"
BF = torch.bfloat16
POISON = -77.0            # exact in bf16

# (rows, cols, src offset alignment, dst offset alignment): offsets are made
# multiples of 8 elements (16 bytes) or pushed off by the given odd amount.
#   64x64 aligned: one full tile on the vector path
#   1x8, 72x200, 130x65: ragged tiles, scalar path, rows or cols of 1 tile + tail
#   128x192 aligned: several full tiles on the vector path
#   256x192 at a source offset that is no multiple of 8: scalar path forced
#   64x128 with only the image off alignment: scalar path forced by dst
MATRICES = [(64, 64, 0, 0), (1, 8, 0, 0), (72, 200, 0, 0), (130, 65, 0, 0),
            (128, 192, 0, 0), (256, 192, 3, 0), (64, 128, 0, 5)]
GUARD = 8


def _layout():
    """entries (src_off, dst_off, rows, cols), src size, dst size; GUARD or
    more elements before, between and after the images."""
    entries, so, do = [], 0, GUARD
    for rows, cols, s_odd, d_odd in MATRICES:
        so = -(-so // 8) * 8 + s_odd
        do = -(-do // 8) * 8 + d_odd
        entries.append((so, do, rows, cols))
        so += rows * cols + 1
        do += rows * cols + GUARD
    return entries, so, do


def _check_images(src, dst, entries):
    inside = torch.zeros(dst.numel(), dtype=torch.bool, device=DEV)
    for so, do, rows, cols in entries:
        want = src[so:so + rows * cols].view(rows, cols).t().contiguous()
        got = dst[do:do + rows * cols].view(cols, rows)
        assert torch.equal(got, want), (rows, cols, so, do)
        inside[do:do + rows * cols] = True
    assert bool((dst[~inside] == POISON).all()), "a write outside the images"
    assert int((~inside).sum()) >= GUARD * (len(entries) + 1)


# 0: the default grid, one trip; 3: 36 tiles on 3 workgroups, 12 trips
@pytest.mark.parametrize("max_blocks", [0, 3])
def test_transpose_batched_table(max_blocks):
    entries, ns, nd = _layout()
    assert entries[5][0] % 8 != 0 and entries[6][1] % 8 != 0
    tiles = sum(-(-r // 64) * -(-c // 64) for _, _, r, c in entries)
    assert tiles == 36
    g = torch.Generator().manual_seed(7)
    src = torch.randn(ns, generator=g).to(BF).to(DEV)
    dst = torch.full((nd,), POISON, dtype=BF, device=DEV)
    tdev, thost = ops.transpose_table(entries, DEV)
    ops.transpose_batched(src, dst, tdev, thost, max_blocks)
    _check_images(src, dst, entries)


def test_transpose_batched_rejects_bad_tables():
    src = torch.zeros(4096, dtype=BF, device=DEV)
    dst = torch.zeros(4096, dtype=BF, device=DEV)
    for entries in ([(1, 0, 64, 64)], [(0, 1, 64, 64)], [(0, 0, 0, 8)]):
        tdev, thost = ops.transpose_table(entries, DEV)
        with pytest.raises(RuntimeError):
            ops.transpose_batched(src, dst, tdev, thost)
    tdev, thost = ops.transpose_table([(0, 0, 8, 8), (64, 64, 8, 8)], DEV)
    thost[1, 4] = 5      # a wrong tile prefix
    with pytest.raises(RuntimeError):
        ops.transpose_batched(src, dst, tdev, thost)
    with pytest.raises(RuntimeError):
        ops.transpose_batched(src, src, tdev, ops.transpose_table([(0, 0, 8, 8)])[1])


# ---------------------------------------------------------------------------
# linear_wt at M=256, in=192, out=320
# ---------------------------------------------------------------------------
M, IN, OUT = 256, 192, 320


@pytest.fixture(scope="module")
def lin():
    """Inputs, autograd's F.linear results (twice, for the repeat guard) and
    the fp64 dx of the same bf16 inputs. Computed once, never modified."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, IN, generator=g).to(BF).to(DEV)
    w = (torch.randn(OUT, IN, generator=g) / IN ** 0.5).to(BF).to(DEV)
    dy = torch.randn(M, OUT, generator=g).to(BF).to(DEV)

    def autograd(shape_x, x_grad=True):
        xa = x.view(shape_x).clone().requires_grad_(x_grad)
        wa = w.clone().requires_grad_(True)
        y = F.linear(xa, wa)
        y.backward(dy.view(*shape_x[:-1], OUT))
        return y.detach(), xa.grad, wa.grad

    ref = {"x": x, "w": w, "dy": dy, "wt": w.t().contiguous(),
           "dx64": dy.double() @ w.double()}
    for name, shp in (("2d", (M, IN)), ("3d", (4, M // 4, IN))):
        ref[name] = (autograd(shp), autograd(shp))
    ref["err_auto"] = row_err(ref["2d"][0][1], ref["dx64"])
    return ref


def _run_linear_wt(lin, shape_x, x_grad=True, remat=False):
    xa = lin["x"].view(shape_x).clone().requires_grad_(x_grad)
    wa = lin["w"].clone().requires_grad_(True)
    if remat:
        y = checkpoint(ops.linear_wt, xa, wa, lin["wt"], use_reentrant=False)
    else:
        y = ops.linear_wt(xa, wa, lin["wt"])
    y.backward(lin["dy"].view(*shape_x[:-1], OUT))
    return y.detach(), xa.grad, wa.grad


def _check_linear(lin, tag, key, got):
    (y0, dx0, dw0), (y1, dx1, dw1) = lin[key]
    y, dx, dw = got
    assert torch.equal(y, y0), tag
    same(f"{tag}.dW", dw, dw0, dw1)
    if dx is None:
        return
    assert dx.shape == dx0.shape
    e_new = row_err(dx.reshape(M, IN), lin["dx64"])
    e_auto = row_err(dx0.reshape(M, IN), lin["dx64"])
    print(f"DGRAD_WT {tag}: dx row_err vs fp64: linear_wt {e_new:.3e}, "
          f"autograd {e_auto:.3e}, bound {2 * e_auto:.3e}")
    # both are fp32-accumulated sums rounded once to bf16: at most twice
    assert e_new <= 2 * e_auto, (tag, e_new, e_auto)


def test_linear_wt_2d(lin):
    _check_linear(lin, "2d", "2d", _run_linear_wt(lin, (M, IN)))


def test_linear_wt_3d(lin):
    _check_linear(lin, "3d", "3d", _run_linear_wt(lin, (4, M // 4, IN)))


@pytest.mark.parametrize("key,shape_x", [("2d", (M, IN)), ("3d", (4, M // 4, IN))])
def test_linear_wt_under_checkpoint(lin, key, shape_x):
    _check_linear(lin, f"remat.{key}", key, _run_linear_wt(lin, shape_x, remat=True))


@pytest.mark.parametrize("key,shape_x", [("2d", (M, IN)), ("3d", (4, M // 4, IN))])
def test_linear_wt_without_input_grad(lin, key, shape_x):
    y, dx, dw = _run_linear_wt(lin, shape_x, x_grad=False)
    assert dx is None
    _check_linear(lin, f"no_dx.{key}", key, (y, None, dw))


def test_linear_wt_rejects_a_wrong_image(lin):
    with pytest.raises(RuntimeError):
        ops.linear_wt(lin["x"], lin["w"], lin["w"])
    with pytest.raises(RuntimeError):
        ops.linear_wt(lin["x"], lin["w"], lin["wt"].float())


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------
TINY = GPTConfig(block_size=128, vocab_size=65, n_layer=2, n_head=1,
                 n_embd=64, dropout=0.0)
G_ACCUM = 2


def _engine(seed=0):
    torch.manual_seed(seed)
    model = GPT(TINY).to(DEV)
    return model, ShardedAdamW(model, compute_dtype=BF, zero=False, peak_lr=1e-2)


def _batches(n):
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, 65, (n, 4, 128), generator=g).to(DEV)
    y = torch.randint(0, 65, (n, 4, 128), generator=g).to(DEV)
    return x, y


def _train_step(model, engine, x, y):
    for i in range(G_ACCUM):
        model.loss(x[i], y[i]).backward()
        engine.microstep_end()
    engine.step(5e-3, G_ACCUM)


def _linears(model):
    mods = [m for m in model.modules() if isinstance(m, Linear)]
    assert len(mods) == 4 * TINY.n_layer + 1
    return mods


def _assert_images(model, when):
    for m in _linears(model):
        assert m.weight_t is not None, when
        assert m.weight_t.shape == (m.weight.shape[1], m.weight.shape[0])
        assert torch.equal(m.weight_t, m.weight.t()), (when, tuple(m.weight.shape))


def test_engine_images_follow_every_writer(monkeypatch):
    monkeypatch.delenv("MIDGPT_DGRAD_WT", raising=False)
    model, engine = _engine()
    _assert_images(model, "construction")
    x, y = _batches(G_ACCUM)
    for s in range(2):
        before = engine.flat_w.clone()
        _train_step(model, engine, x, y)
        assert not torch.equal(before, engine.flat_w)
        _assert_images(model, f"step {s}")
    before = engine.flat_w.clone()
    engine.master.mul_(1.5)
    engine.refresh_weights()
    assert not torch.equal(before, engine.flat_w)
    _assert_images(model, "refresh_weights")
    g = torch.Generator().manual_seed(5)
    full = [torch.randn(engine.total, generator=g) for _ in range(3)]
    engine.load_state_full(full[0], full[1].abs(), full[2].abs(), 7)
    assert torch.equal(engine.flat_w[:engine.total], full[0].to(BF).to(DEV))
    _assert_images(model, "load_state_full")


def test_engine_cache_off_binds_nothing(monkeypatch):
    monkeypatch.setenv("MIDGPT_DGRAD_WT", "0")
    model, engine = _engine()
    assert engine.flat_wt is None
    assert all(m.weight_t is None for m in _linears(model))
    x, y = _batches(G_ACCUM)
    _train_step(model, engine, x, y)
    assert all(m.weight_t is None for m in _linears(model))


def test_engine_cache_on_and_off_give_the_same_loss(monkeypatch, lin):
    x, y = _batches(G_ACCUM + 1)
    losses = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("MIDGPT_DGRAD_WT", flag)
        model, engine = _engine(seed=1)
        assert (engine.flat_wt is not None) == (flag == "1")
        _train_step(model, engine, x, y)
        with torch.no_grad():
            losses[flag] = float(model.loss(x[G_ACCUM], y[G_ACCUM]))
    # the bound of the dx checks above: twice autograd's own relative error
    tol = 2 * lin["err_auto"] * abs(losses["0"])
    print(f"DGRAD_WT loss after one step: on {losses['1']:.6f} off {losses['0']:.6f} "
          f"tol {tol:.3e}")
    assert abs(losses["1"] - losses["0"]) <= tol, (losses, tol)


def _zero_worker(rank, init_file, out_q):
    import os
    import torch.distributed as dist
    os.environ["WORLD_SIZE"] = "2"
    os.environ["RANK"] = str(rank)
    os.environ.pop("MIDGPT_DGRAD_WT", None)
    dist.init_process_group("gloo", init_method=f"file://{init_file}",
                            rank=rank, world_size=2)
    torch.manual_seed(0)
    model = GPT(TINY).to("cuda:0")  # both ranks share the one GPU
    engine = ShardedAdamW(model, compute_dtype=BF, zero=True)
    ok = engine.zero and engine.flat_wt is not None
    x, y = _batches(2)
    for _ in range(2):
        model.loss(x[rank], y[rank]).backward()
        engine.microstep_end()
        engine.step(5e-3)
        ok = ok and all(torch.equal(m.weight_t, m.weight.t()) for m in _linears(model))
    torch.cuda.synchronize()
    out_q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_zero_two_ranks_one_gpu_images(tmp_path):
    """ZeRO on 2 ranks sharing cuda:0 over gloo (as test_gpu_model.py does):
    after the all-gather of a step every image equals weight.t() on both
    ranks. The RCCL twin is tests/test_multigpu_dgrad_wt.py."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_zero_worker, args=(r, str(tmp_path / "pg"), q))
             for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get() for _ in range(2))
    for p in procs:
        p.join(timeout=240)
        assert p.exitcode == 0
    assert res == {0: True, 1: True}
