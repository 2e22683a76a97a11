"""KV-cache decode kernels on the GPU (csrc/decode.hip) and the native decode
path built on them.

kv_append is compared bit for bit with qkv_prep_fwd (one row body serves
both). attn_decode is judged by ``row_err`` against fp64 with the bound taken
from an fp32 yardstick at the same inputs (kernel_edge_util); cache rows at
and beyond every key limit hold NaN, so a row that is loaded and multiplied
by zero instead of skipped fails the case. The model-level yardstick is the
eager decode path (MIDGPT_DECODE_REF=1), never the new code.

Every figure is printed as ``EDGE <case> ...`` / ``DECODE ...``; the values
measured on MI355X are in profiles/decode.md."""
import pytest
import torch

import kernel_edge_util as U
from decode_util import decode_math

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from midgpt_amd import ops
    from midgpt_amd.ops import reference as ref
    assert ops.have_ext(), f"HIP extension must be built: {ops._C_ERR}"

from midgpt_amd.config import GPTConfig
from midgpt_amd.models.gpt import GPT

DEV = "cuda:0"
BF = torch.bfloat16
B, H, TMAX = 2, 3, 256
NAN = float("nan")


def _randbf(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def _nan_caches(C):
    return (torch.full((B, H, TMAX, C), NAN, device=DEV, dtype=BF),
            torch.full((B, H, TMAX, C), NAN, device=DEV, dtype=BF))


def _prep_inputs(C, T, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = _randbf(g, B, T, 3, H, C)
    qw = (1.0 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    kw = (1.0 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    sin, cos = ref.rope_tables(C, TMAX, device=DEV)
    return qkv, qw, kw, sin.contiguous(), cos.contiguous()


# ---------------------------------------------------------------------------
# kv_append
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 128])
def test_kv_append_bit_exact_with_qkv_prep(C):
    qkv, qw, kw, sin, cos = _prep_inputs(C, 128, 31)
    q, k, v, _, _ = ops._C.qkv_prep_fwd(qkv, qw, kw, sin[:128].contiguous(),
                                        cos[:128].contiguous(), 1e-6)
    kc, vc = _nan_caches(C)
    pos = 0
    for n in (5, 1, 1, 64, 57):
        qc = ops.kv_append(qkv[:, pos:pos + n], qw, kw, sin, cos, kc, vc, pos)
        assert qc.shape == (B, H, n, C)
        assert torch.equal(qc, q[:, :, pos:pos + n]), (pos, n)
        pos += n
        assert bool(torch.isnan(kc[:, :, pos:]).all()), pos
        assert bool(torch.isnan(vc[:, :, pos:]).all()), pos
    assert pos == 128
    assert torch.equal(kc[:, :, :128], k)
    assert torch.equal(vc[:, :, :128], v)


# ---------------------------------------------------------------------------
# attn_decode
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attn_inputs():
    """Per head dim: q (B,H,16,C) and full K/V caches; read-only."""
    out = {}
    for C in (64, 128):
        g = torch.Generator().manual_seed(32 + C)
        out[C] = (_randbf(g, B, H, 16, C), _randbf(g, B, H, TMAX, C),
                  _randbf(g, B, H, TMAX, C))
    return out


def _decode_case(inputs, C, Tq, kv_len, num_splits, qscale=1.0):
    """Kernel output, its figure against fp64, and the poisoned caches."""
    q_all, k_all, v_all = inputs[C]
    q = (q_all[:, :, :Tq].float() * qscale).to(BF).contiguous()
    kc, vc = k_all.clone(), v_all.clone()
    kc[:, :, kv_len:] = NAN
    vc[:, :, kv_len:] = NAN
    got = ops._C.attn_decode(q, kc, vc, kv_len, num_splits)
    assert got.shape == (B, Tq, H, C) and got.dtype == BF
    ref64 = decode_math(q, kc, vc, kv_len, torch.float64, False)
    yard = decode_math(q, kc, vc, kv_len, torch.float32, True)
    fig = U.fig_rows(f"decode.o C{C} Tq{Tq} kv{kv_len} s{num_splits} x{qscale:g}",
                     got, yard, ref64)
    return got, fig, (q, kc, vc)


CASES = [(1, 2, 1), (1, 7, 1), (1, 8, 1), (1, 9, 2), (1, 63, 1), (1, 64, 2),
         (1, 65, 5), (1, 3, 5), (1, 255, 0), (1, 256, 4), (3, 10, 2), (5, 5, 3),
         (16, 200, 0)]


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("Tq,kv_len,num_splits", CASES)
def test_attn_decode_rows(attn_inputs, C, Tq, kv_len, num_splits):
    _, fig, _ = _decode_case(attn_inputs, C, Tq, kv_len, num_splits)
    U.check("decode", [fig])


@pytest.mark.parametrize("C", [64, 128])
def test_attn_decode_rows_see_only_their_own_keys(attn_inputs, C):
    """Tq > 1: keys above a row's own limit (but below kv_len) hold finite
    data. Row i must equal the single-row call at kv_len - Tq + i + 1 with
    everything above poisoned, bit for bit (same slices need the same
    num_splits = 1 arithmetic)."""
    Tq, kv_len = 5, 37
    got, _, (q, kc, vc) = _decode_case(attn_inputs, C, Tq, kv_len, 1)
    for i in range(Tq):
        lim = kv_len - Tq + i + 1
        kci, vci = kc.clone(), vc.clone()
        kci[:, :, lim:] = NAN
        vci[:, :, lim:] = NAN
        one = ops._C.attn_decode(q[:, :, i:i + 1].contiguous(), kci, vci, lim, 1)
        assert torch.equal(one[:, 0], got[:, i]), i


@pytest.mark.parametrize("C", [64, 128])
def test_attn_decode_large_scores(attn_inputs, C):
    """q x20: scores of a few hundred, the running maximum moves a lot and
    every rescale matters."""
    _, fig, _ = _decode_case(attn_inputs, C, 1, 65, 2, qscale=20.0)
    U.check("decode", [fig])


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("num_splits", [0, 1, 3])
def test_attn_decode_single_key_returns_v(attn_inputs, C, num_splits):
    got, _, (_, _, vc) = _decode_case(attn_inputs, C, 1, 1, num_splits)
    assert torch.equal(got[:, 0], vc[:, :, 0])


@pytest.mark.parametrize("C", [64, 128])
def test_attn_decode_splits_agree(attn_inputs, C):
    """num_splits 1, 2 and 5 at one shape: each within the bound of the fp64
    result (so within twice the bound of each other)."""
    figs = [_decode_case(attn_inputs, C, 3, 200, s)[1] for s in (1, 2, 5)]
    U.check("decode splits", figs)


def test_auto_splits_rule():
    f = ops._C.attn_decode_auto_splits
    assert f(16, 128, 256) == 1            # under two slices' worth of keys
    assert f(16, 511, 256) == 1 and f(16, 512, 256) == 2
    assert f(4096, 4096, 256) == 1         # rows alone fill the chip
    assert f(1, 1 << 20, 256) == 64        # capped
    for rows, kv, cus in [(16, 1024, 256), (32, 4096, 256), (6, 255, 256)]:
        s = f(rows, kv, cus)
        assert 1 <= s <= 64 and kv // s >= 128, (rows, kv, s)


def test_attn_decode_auto_follows_rule():
    """num_splits = 0 where the rule cuts the range: same bits as asking for
    the rule's count, and within the bound."""
    C, kv_len = 128, 512
    g = torch.Generator().manual_seed(41)
    q, kc, vc = _randbf(g, 1, 2, 1, C), _randbf(g, 1, 2, 600, C), _randbf(g, 1, 2, 600, C)
    kc[:, :, kv_len:] = NAN
    vc[:, :, kv_len:] = NAN
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    s = ops._C.attn_decode_auto_splits(2, kv_len, cus)
    assert s == 2
    got = ops._C.attn_decode(q, kc, vc, kv_len, 0)
    assert torch.equal(got, ops._C.attn_decode(q, kc, vc, kv_len, s))
    U.check("decode auto", [U.fig_rows(
        "decode.o C128 Tq1 kv512 s0", got,
        decode_math(q, kc, vc, kv_len, torch.float32, True),
        decode_math(q, kc, vc, kv_len, torch.float64, False))])


def test_binding_guards():
    C = 64
    qkv, qw, kw, sin, cos = _prep_inputs(C, 8, 33)
    kc, vc = _nan_caches(C)
    q = torch.zeros(B, H, 4, C, device=DEV, dtype=BF)
    w32 = torch.ones(32, device=DEV)
    s32, c32 = (t.contiguous() for t in ref.rope_tables(32, TMAX, device=DEV))
    kc32 = torch.zeros(B, H, TMAX, 32, device=DEV, dtype=BF)
    vc32 = torch.zeros_like(kc32)
    with pytest.raises(RuntimeError):      # C = 32
        ops._C.attn_decode(torch.zeros(B, H, 1, 32, device=DEV, dtype=BF), kc32, vc32, 8, 1)
    with pytest.raises(RuntimeError):
        ops._C.kv_append(torch.zeros(B, 1, 3, H, 32, device=DEV, dtype=BF), w32, w32,
                         s32, c32, kc32, vc32, 0, 1e-6)
    with pytest.raises(RuntimeError):      # pos + Tn > Tmax
        ops._C.kv_append(qkv, qw, kw, sin, cos, kc, vc, TMAX - 7, 1e-6)
    with pytest.raises(RuntimeError):
        ops.kv_append(qkv, qw, kw, sin, cos, kc, vc, TMAX - 7)
    with pytest.raises(RuntimeError):      # negative position
        ops._C.kv_append(qkv, qw, kw, sin, cos, kc, vc, -1, 1e-6)
    with pytest.raises(RuntimeError):      # tables shorter than pos + Tn
        ops._C.kv_append(qkv, qw, kw, sin[:16].contiguous(), cos[:16].contiguous(),
                         kc, vc, 12, 1e-6)
    with pytest.raises(RuntimeError):      # Tq = 17
        ops._C.attn_decode(torch.zeros(B, H, 17, C, device=DEV, dtype=BF), kc, vc, 32, 1)
    with pytest.raises(RuntimeError):      # Tq > kv_len
        ops._C.attn_decode(q, kc, vc, 3, 1)
    with pytest.raises(RuntimeError):      # kv_len > Tmax
        ops._C.attn_decode(q, kc, vc, TMAX + 1, 1)
    with pytest.raises(RuntimeError):      # num_splits > 64
        ops._C.attn_decode(q, kc, vc, 8, 65)
    with pytest.raises(RuntimeError):      # fp16
        ops._C.attn_decode(q.half(), kc.half(), vc.half(), 8, 1)
    with pytest.raises(RuntimeError):
        ops._C.kv_append(qkv.half(), qw, kw, sin, cos, kc, vc, 0, 1e-6)
    with pytest.raises(RuntimeError):      # non-contiguous cache view
        ops._C.attn_decode(q, kc[:, :, ::2], vc[:, :, ::2], 8, 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(kc).all()) and bool(torch.isnan(vc).all())


# ---------------------------------------------------------------------------
# prefill_attention
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 128])
def test_prefill_attention_padded_prompt(C):
    Tn = 100                               # pads to 128
    qkv, qw, kw, sin, cos = _prep_inputs(C, Tn, 34)
    kc, vc = _nan_caches(C)
    o = ops.prefill_attention(qkv, qw, kw, sin, cos, kc, vc)
    assert o.shape == (B, Tn, H * C)
    q, k, v, _, _ = ops._C.qkv_prep_fwd(qkv, qw, kw, sin[:Tn].contiguous(),
                                        cos[:Tn].contiguous(), 1e-6)
    assert torch.equal(kc[:, :, :Tn], k)
    assert torch.equal(vc[:, :, :Tn], v)
    assert bool(torch.isnan(kc[:, :, Tn:]).all())
    assert bool(torch.isnan(vc[:, :, Tn:]).all())
    got = {"o": o.view(B, Tn, H, C).transpose(1, 2)}
    U.check(f"prefill C{C}", U.attn_figures(q, k, v, None, got, names=("o",)))
    # and the next token decodes against what the prefill left in the cache
    g = torch.Generator().manual_seed(35)
    q1 = _randbf(g, B, H, 1, C)
    kc[:, :, Tn] = k[:, :, 0]
    vc[:, :, Tn] = v[:, :, 0]
    got1 = ops._C.attn_decode(q1, kc, vc, Tn + 1, 0)
    U.check(f"prefill+decode C{C}", [U.fig_rows(
        "decode.o", got1, decode_math(q1, kc, vc, Tn + 1, torch.float32, True),
        decode_math(q1, kc, vc, Tn + 1, torch.float64, False))])
    with pytest.raises(RuntimeError):      # 100 rows pad to 128 > a 120-row cache
        ops.prefill_attention(qkv, qw, kw, sin, cos, kc[:, :, :120].contiguous(),
                              vc[:, :, :120].contiguous())


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
def _models(n_embd, seed):
    cfg = GPTConfig(block_size=128, vocab_size=512, n_layer=2, n_head=2,
                    n_embd=n_embd, dropout=0.0)
    torch.manual_seed(seed)
    cpu = GPT(cfg).eval()
    gm = GPT(cfg)
    gm.load_state_dict(cpu.state_dict())
    gm = gm.to(DEV).to(BF).eval()
    gm.rope_sin = gm.rope_sin.float()
    gm.rope_cos = gm.rope_cos.float()
    return cpu, gm


def _teacher_forced(gm, idx, n_prefill):
    """Logit rows at positions n_prefill-1 .. T-1 on the path generate takes."""
    from midgpt_amd.generate import decode_stepper
    step = decode_stepper(gm, idx.shape[0])
    rows = [step(idx[:, :n_prefill], 0)]
    for t in range(n_prefill, idx.shape[1]):
        rows.append(step(idx[:, t:t + 1], t))
    return torch.stack(rows, dim=1)        # (B, T - n_prefill + 1, V)


@pytest.mark.parametrize("n_embd", [128, 256])   # head dim 64, 128
def test_decode_step_teacher_forced_vs_eager(n_embd, monkeypatch):
    from midgpt_amd import generate as G
    cpu, gm = _models(n_embd, 37)
    idx = torch.randint(0, 512, (2, 128), generator=torch.Generator().manual_seed(38))
    with torch.no_grad():
        ref_logits = cpu(idx)[:, 99:].double()           # 29 rows per sequence
    monkeypatch.delenv("MIDGPT_DECODE_REF", raising=False)
    assert G.native_decode(gm)
    native = _teacher_forced(gm, idx.to(DEV), 100)
    monkeypatch.setenv("MIDGPT_DECODE_REF", "1")
    assert not G.native_decode(gm)
    eager = _teacher_forced(gm, idx.to(DEV), 100)
    assert native.shape == eager.shape == (2, 29, 512)
    e_native = U.row_err(native.cpu(), ref_logits)
    e_eager = U.row_err(eager.cpu(), ref_logits)
    print(f"DECODE teacher-forced n_embd{n_embd}: native={e_native:.3e} "
          f"eager={e_eager:.3e} bound={3 * e_eager:.3e}")
    assert e_native <= 3 * e_eager, (e_native, e_eager)


def _generate_counting(gm, idx, n_new, temperature):
    """generate() with a counting wrapper around the attn_decode binding."""
    from midgpt_amd.generate import generate
    calls = [0]
    real = ops._C.attn_decode

    def counting(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    ops._C.attn_decode = counting
    try:
        out = generate(gm, idx, n_new, temperature=temperature)
    finally:
        ops._C.attn_decode = real
    return out, calls[0]


@pytest.mark.parametrize("prompt,temperature", [((2, 8), 0.8), ((1, 120), 0.0)])
def test_generate_native_path(prompt, temperature, monkeypatch):
    """(2,8) stays inside block_size; (1,120) + 16 crosses the 128-token
    window and recomputes the slid window through prefill_attention."""
    _, gm = _models(128, 39)
    torch.manual_seed(40)
    idx = torch.randint(0, 512, prompt, device=DEV)
    monkeypatch.delenv("MIDGPT_DECODE_REF", raising=False)
    out, calls = _generate_counting(gm, idx, 16, temperature)
    assert out.shape == (prompt[0], prompt[1] + 16)
    assert torch.equal(out[:, :prompt[1]], idx)
    assert 0 <= int(out.min()) and int(out.max()) < 512
    assert calls > 0
    monkeypatch.setenv("MIDGPT_DECODE_REF", "1")
    out, calls = _generate_counting(gm, idx, 16, temperature)
    assert out.shape == (prompt[0], prompt[1] + 16)
    assert 0 <= int(out.min()) and int(out.max()) < 512
    assert calls == 0
