"""Ragged decode kernels on the GPU (csrc/decode.hip, RAGGED instantiations)
and the ragged generation path built on them.

The contract is bit-exactness with the uniform kernels sequence by sequence:
``kv_append_ragged`` / ``attn_decode_ragged`` of a batch equal ``kv_append`` /
``attn_decode`` on each sequence's slice under ``torch.equal`` (explicit
num_splits). Cache rows at and beyond each sequence's own length hold NaN, so
a row loaded past it shows in the output. With num_splits = 0 the rule is
that of test_gpu_decode.py: ``row_err`` against fp64, bound from the fp32
yardstick at the same inputs. The model-level yardstick is the existing
uniform native path on each sequence alone, never the new code.

Figures are printed as ``EDGE ...`` / ``RAGGED ...``; the values measured on
MI355X are in profiles/decode.md."""
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

from midgpt_amd.config import GPTConfig
from midgpt_amd.models.gpt import GPT

DEV = "cuda:0"
BF = torch.bfloat16
B, H, TMAX = 3, 2, 256
NAN = float("nan")


def _randbf(g, *shape):
    return torch.randn(*shape, generator=g).to(BF).to(DEV)


def _nan_caches(C):
    return (torch.full((B, H, TMAX, C), NAN, device=DEV, dtype=BF),
            torch.full((B, H, TMAX, C), NAN, device=DEV, dtype=BF))


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


def _prep_inputs(C, T, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = _randbf(g, B, T, 3, H, C)
    qw = (1.0 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    kw = (1.0 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    sin, cos = ref.rope_tables(C, TMAX, device=DEV)
    return qkv, qw, kw, sin.contiguous(), cos.contiguous()


# ---------------------------------------------------------------------------
# kv_append_ragged
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("Tn,pos", [(1, (0, 7, 255)), (16, (0, 100, 240))])
def test_kv_append_ragged_bit_exact_per_sequence(C, Tn, pos):
    qkv, qw, kw, sin, cos = _prep_inputs(C, Tn, 71)
    kc, vc = _nan_caches(C)
    q = ops.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc, pos)
    assert q.shape == (B, H, Tn, C) and q.dtype == BF
    for b in range(B):
        kc1, vc1 = (t[b:b + 1].contiguous() for t in _nan_caches(C))
        q1 = ops.kv_append(qkv[b:b + 1].contiguous(), qw, kw, sin, cos, kc1, vc1, pos[b])
        rows = slice(pos[b], pos[b] + Tn)
        assert torch.equal(q[b], q1[0]), b
        assert torch.equal(kc[b, :, rows], kc1[0, :, rows]), b
        assert torch.equal(vc[b, :, rows], vc1[0, :, rows]), b
        assert not bool(torch.isnan(kc[b, :, rows]).any()), b
        assert bool(torch.isnan(kc[b, :, :pos[b]]).all()), b
        assert bool(torch.isnan(vc[b, :, :pos[b]]).all()), b
        assert bool(torch.isnan(kc[b, :, pos[b] + Tn:]).all()), b
        assert bool(torch.isnan(vc[b, :, pos[b] + Tn:]).all()), b
    # a device copy handed in by the caller is the same call
    kc2, vc2 = _nan_caches(C)
    q2 = ops.kv_append_ragged(qkv, qw, kw, sin, cos, kc2, vc2, torch.tensor(pos),
                              pos_dev=_i32(pos))
    assert torch.equal(q2, q)
    assert torch.equal(torch.nan_to_num(kc2), torch.nan_to_num(kc))
    assert torch.equal(torch.nan_to_num(vc2), torch.nan_to_num(vc))


# ---------------------------------------------------------------------------
# attn_decode_ragged
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attn_inputs():
    """Per head dim: q (B,H,16,C) and full K/V caches; read-only."""
    out = {}
    for C in (64, 128):
        g = torch.Generator().manual_seed(72 + C)
        out[C] = (_randbf(g, B, H, 16, C), _randbf(g, B, H, TMAX, C),
                  _randbf(g, B, H, TMAX, C))
    return out


def _poisoned(inputs, C, Tq, kv_lens):
    q_all, k_all, v_all = inputs[C]
    q = q_all[:, :, :Tq].contiguous()
    kc, vc = k_all.clone(), v_all.clone()
    for b, n in enumerate(kv_lens):
        kc[b, :, n:] = NAN
        vc[b, :, n:] = NAN
    return q, kc, vc


CASES = [(1, (1, 9, 256), 1), (1, (2, 65, 200), 2), (1, (3, 64, 255), 5),
         (3, (3, 10, 200), 2), (16, (16, 17, 256), 0)]


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("Tq,kv_lens,num_splits", CASES)
def test_attn_decode_ragged_per_sequence(attn_inputs, C, Tq, kv_lens, num_splits):
    q, kc, vc = _poisoned(attn_inputs, C, Tq, kv_lens)
    got = ops._C.attn_decode_ragged(q, kc, vc, _i32(kv_lens), torch.tensor(kv_lens),
                                    num_splits)
    assert got.shape == (B, Tq, H, C) and got.dtype == BF
    assert not bool(torch.isnan(got).any())
    figs = []
    for b, n in enumerate(kv_lens):
        qb, kb, vb = (t[b:b + 1].contiguous() for t in (q, kc, vc))
        if num_splits >= 1:
            one = ops._C.attn_decode(qb, kb, vb, n, num_splits)
            assert torch.equal(got[b], one[0]), b
        figs.append(U.fig_rows(
            f"ragged.o C{C} Tq{Tq} kv{n} of {kv_lens} s{num_splits}", got[b:b + 1],
            decode_math(qb, kb, vb, n, torch.float32, True),
            decode_math(qb, kb, vb, n, torch.float64, False)))
    U.check("ragged decode", figs)
    # the op: same bits, (B,Tq,H*C), with and without the caller's device copy
    o = ops.decode_attention_ragged(q, kc, vc, kv_lens, num_splits=num_splits)
    assert torch.equal(o, got.view(B, Tq, H * C))
    o = ops.decode_attention_ragged(q, kc, vc, torch.tensor(kv_lens), _i32(kv_lens),
                                    num_splits)
    assert torch.equal(o, got.view(B, Tq, H * C))


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("num_splits", [0, 1, 3])
def test_attn_decode_ragged_equal_lengths_is_the_uniform_call(attn_inputs, C, num_splits):
    kv_lens = (200, 200, 200)
    q, kc, vc = _poisoned(attn_inputs, C, 1, kv_lens)
    got = ops._C.attn_decode_ragged(q, kc, vc, _i32(kv_lens), torch.tensor(kv_lens),
                                    num_splits)
    assert torch.equal(got, ops._C.attn_decode(q, kc, vc, 200, num_splits))


# ---------------------------------------------------------------------------
# both backends side by side, guards
# ---------------------------------------------------------------------------
def test_ragged_api_parity_with_ref_backend(attn_inputs):
    C, Tn, pos = 64, 4, (0, 9, 200)
    qkv, qw, kw, sin, cos = _prep_inputs(C, Tn, 73)
    res = {}
    for name, impl in (("_C", ops._C), ("ref", ref_backend)):
        kc, vc = _nan_caches(C)
        out = impl.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc, _i32(pos),
                                    torch.tensor(pos), 1e-6)
        res[name] = (out, kc, vc)
    (qa, kca, vca), (qb, kcb, vcb) = res["_C"], res["ref"]
    assert isinstance(qa, torch.Tensor) and isinstance(qb, torch.Tensor)
    assert qa.shape == qb.shape and qa.dtype == qb.dtype
    assert torch.equal(torch.isnan(kca), torch.isnan(kcb))
    assert torch.equal(torch.isnan(vca), torch.isnan(vcb))
    assert torch.equal(torch.nan_to_num(vca), torch.nan_to_num(vcb))
    sl = [(b, slice(p, p + Tn)) for b, p in enumerate(pos)]
    figs = []
    for b, rows in sl:                     # per sequence: its own RoPE rows
        r = U.qkv_prep_math(qkv[b:b + 1], qw, kw, sin[rows], cos[rows], 1e-6, torch.float64)
        y = U.qkv_prep_math(qkv[b:b + 1], qw, kw, sin[rows], cos[rows], 1e-6, torch.float32)
        for tag, q_, kc_ in (("_C", qa, kca), ("ref", qb, kcb)):
            figs.append(U.fig_rows(f"{tag} append.q b{b}", q_[b:b + 1], y["q"].to(BF), r["q"]))
            figs.append(U.fig_rows(f"{tag} append.k b{b}", kc_[b:b + 1, :, rows],
                                   y["k"].to(BF), r["k"]))
    U.check("ragged parity append", figs)

    Tq, kv_lens = 3, (3, 10, 200)
    q, kc, vc = _poisoned(attn_inputs, C, Tq, kv_lens)
    oa = ops._C.attn_decode_ragged(q, kc, vc, _i32(kv_lens), torch.tensor(kv_lens), 2)
    ob = ref_backend.attn_decode_ragged(q, kc, vc, _i32(kv_lens), torch.tensor(kv_lens), 2)
    assert oa.shape == ob.shape == (B, Tq, H, C) and oa.dtype == ob.dtype == BF
    figs = []
    for b, n in enumerate(kv_lens):
        args = (q[b:b + 1], kc[b:b + 1], vc[b:b + 1], n)
        yard = decode_math(*args, torch.float32, True)
        ref64 = decode_math(*args, torch.float64, False)
        figs.append(U.fig_rows(f"_C decode.o b{b}", oa[b:b + 1], yard, ref64))
        figs.append(U.fig_rows(f"ref decode.o b{b}", ob[b:b + 1], yard, ref64))
    U.check("ragged parity decode", figs)


def test_ragged_guards_on_the_gpu():
    C = 64
    qkv, qw, kw, sin, cos = _prep_inputs(C, 8, 74)
    kc, vc = _nan_caches(C)
    ok = (0, 5, 100)

    def both(pos, **kw_):
        a = dict(sin=sin, cos=cos, dev=_i32(ok))
        a.update(kw_)
        with pytest.raises(RuntimeError):
            ops._C.kv_append_ragged(qkv, qw, kw, a["sin"], a["cos"], kc, vc, a["dev"],
                                    torch.tensor(pos), 1e-6)
        with pytest.raises(RuntimeError):
            ops.kv_append_ragged(qkv, qw, kw, a["sin"], a["cos"], kc, vc, pos)

    both((0, 5, TMAX - 7))                 # pos + Tn > Tmax for one sequence
    both((0, -1, 5))                       # negative position
    both((0, 5))                           # wrong length
    both((0, 5, 12), sin=sin[:16].contiguous(), cos=cos[:16].contiguous())
    with pytest.raises(RuntimeError):      # host copy on the GPU
        ops._C.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc, _i32(ok), _i32(ok), 1e-6)
    with pytest.raises(RuntimeError):      # device copy on the CPU
        ops._C.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc, torch.tensor(ok),
                                torch.tensor(ok), 1e-6)
    with pytest.raises(RuntimeError):      # device copy int64
        ops._C.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc,
                                torch.tensor(ok, device=DEV), torch.tensor(ok), 1e-6)
    q = torch.zeros(B, H, 4, C, device=DEV, dtype=BF)
    for lens in ((4, 3, 10), (4, TMAX + 1, 10), (4, 10)):   # < Tq, > Tmax, length
        with pytest.raises(RuntimeError):
            ops._C.attn_decode_ragged(q, kc, vc, _i32((4, 4, 4)), torch.tensor(lens), 1)
        with pytest.raises(RuntimeError):
            ops.decode_attention_ragged(q, kc, vc, lens)
    with pytest.raises(RuntimeError):      # num_splits > 64
        ops._C.attn_decode_ragged(q, kc, vc, _i32((4, 4, 4)), torch.tensor((4, 4, 4)), 65)
    with pytest.raises(RuntimeError):      # Tq = 17
        ops._C.attn_decode_ragged(torch.zeros(B, H, 17, C, device=DEV, dtype=BF), kc, vc,
                                  _i32((32, 32, 32)), torch.tensor((32, 32, 32)), 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(kc).all()) and bool(torch.isnan(vc).all())


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
LENS = (3, 40, 100)
STEPS = 20


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


@pytest.mark.parametrize("n_embd", [128, 256])   # head dim 64, 128
def test_ragged_teacher_forced_vs_uniform_native(n_embd, monkeypatch):
    from midgpt_amd import generate as G
    monkeypatch.delenv("MIDGPT_DECODE_REF", raising=False)
    cpu, gm = _models(n_embd, 75)
    assert G.native_decode(gm)
    g = torch.Generator().manual_seed(76)
    seqs = [torch.randint(0, 512, (n + STEPS,), generator=g) for n in LENS]
    cache = G.KVCache(gm, len(LENS))
    rows = [G.prefill_ragged(gm, [s[:n] for s, n in zip(seqs, LENS)], cache)]
    for t in range(STEPS):
        nxt = torch.stack([s[n + t] for s, n in zip(seqs, LENS)]).to(DEV)
        rows.append(G.decode_step_ragged(gm, nxt[:, None], cache))
    assert cache.lens == [n + STEPS for n in LENS]
    assert cache.lens_dev.tolist() == cache.lens
    ragged = torch.stack(rows, dim=1).cpu()              # (B, STEPS + 1, V)
    for b, (s, n) in enumerate(zip(seqs, LENS)):
        with torch.no_grad():
            ref_logits = cpu(s[None])[:, n - 1:].double()
        step = G.decode_stepper(gm, 1)                   # the existing native path
        sd = s.to(DEV)[None]
        alone = [step(sd[:, :n], 0)]
        for t in range(n, n + STEPS):
            alone.append(step(sd[:, t:t + 1], t))
        e_alone = U.row_err(torch.stack(alone, dim=1).cpu(), ref_logits)
        e_ragged = U.row_err(ragged[b:b + 1], ref_logits)
        print(f"RAGGED teacher-forced n_embd{n_embd} L{n}: ragged={e_ragged:.3e} "
              f"uniform B=1={e_alone:.3e} bound={U.FACTOR * e_alone:.3e}")
        assert e_ragged <= U.FACTOR * e_alone, (b, e_ragged, e_alone)


def _generate_ragged_counting(gm, prompts, n_new, **kw):
    from midgpt_amd.generate import generate_ragged
    calls = [0]
    real = ops._C.attn_decode_ragged

    def counting(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    ops._C.attn_decode_ragged = counting
    try:
        out = generate_ragged(gm, prompts, n_new, **kw)
    finally:
        ops._C.attn_decode_ragged = real
    return out, calls[0]


def test_generate_ragged_native_path(monkeypatch):
    _, gm = _models(128, 77)
    g = torch.Generator().manual_seed(78)
    lens = (3, 40, 120)                    # 120 + 12 crosses block_size 128
    prompts = [torch.randint(0, 512, (n,), generator=g).to(DEV) for n in lens]
    want = [n + min(12, 128 - n + 1) for n in lens]
    monkeypatch.delenv("MIDGPT_DECODE_REF", raising=False)
    plain, calls = _generate_ragged_counting(gm, prompts, 12, temperature=0.0)
    assert calls > 0
    assert [o.numel() for o in plain] == want
    for o, p in zip(plain, prompts):
        assert torch.equal(o[:p.numel()], p)
        assert 0 <= int(o.min()) and int(o.max()) < 512
    # EOS: the token sequence 1 emits at step 3 ends it there
    eos = int(plain[1][lens[1] + 2])
    outs, _ = _generate_ragged_counting(gm, prompts, 12, temperature=0.0, eos_id=eos,
                                        stop_check_every=4)
    for b, (o, p) in enumerate(zip(outs, plain)):
        hit = (p[lens[b]:] == eos).nonzero()
        cut = p if not hit.numel() else p[:lens[b] + int(hit[0]) + 1]
        assert torch.equal(o, cut), b
    assert outs[1].numel() <= lens[1] + 3 and int(outs[1][-1]) == eos
    # sampling keeps the budgets
    outs, _ = _generate_ragged_counting(gm, prompts, 12, temperature=0.8, top_k=20)
    assert [o.numel() for o in outs] == want
    # the same code on ref_backend
    monkeypatch.setenv("MIDGPT_DECODE_REF", "1")
    outs, calls = _generate_ragged_counting(gm, prompts, 12, temperature=0.0)
    assert calls == 0
    assert [o.numel() for o in outs] == want
    for o, p in zip(outs, prompts):
        assert torch.equal(o[:p.numel()], p)
        assert 0 <= int(o.min()) and int(o.max()) < 512
