"""Seeded token sampling on the GPU: the ``_C.sample_tokens`` kernel against
the float64 oracle of ops/reference.py (the judge of the kernel and of
ref_backend alike), its binding checks, and ``generate`` / ``generate_ragged``
with ``seed=`` on the native decode path.

Every kernel input is a (B, V) view cut from the middle of a larger bf16
buffer filled with +3e38: a read outside the rows wins the argmax or shifts
the k-th value and shows as a wrong token. Odd V puts every row but the first
off the 16-byte grid, so a vector load across a row edge shows the same way."""
from __future__ import annotations

import pytest
import torch

import sampling_util as S

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from midgpt_amd import ops
    from midgpt_amd.ops import ref_backend
    assert ops.have_ext(), f"HIP extension must be built: {ops._C_ERR}"

from midgpt_amd.config import GPTConfig
from midgpt_amd.models.gpt import GPT

DEV = "cuda:0"
BF = torch.bfloat16


def _place(logits):
    """The CPU (B, V) bf16 logits as a contiguous view inside a +3e38 buffer."""
    B, V = logits.shape
    pad = 64                                  # elements: keeps row 0 16-byte aligned
    buf = torch.full((pad + B * V + pad,), 3e38, dtype=BF, device=DEV)
    view = buf[pad:pad + B * V].view(B, V)
    view.copy_(logits)
    assert view.is_contiguous()
    return view


def _kernel(logits, inv_t, top_k, seed, step):
    return ops._C.sample_tokens(logits, inv_t, top_k, seed, step)


OPT_CASES = S.OPT_CASES + [(65, 64, 0.7, 5), (65, 64, 1.0, None),
                           (520, 1, 1.0, 20), (37, 3, 0.7, None), (2056, 3, 0.1, 1)]


def test_per_row_optimality():
    decided = rows = 0
    for i, (V, B, T, k) in enumerate(OPT_CASES):
        logits = S.bf16_logits(V, B, 4.0, 300 + i)
        dev = _place(logits)
        inv_t = S.inv_t_of(T)
        for step in (0, 7):
            tok = _kernel(dev, inv_t, k or 0, 41 + i, step)
            d, n = S.check_optimal(tok, logits, inv_t, k, 41 + i, step)
            decided, rows = decided + d, rows + n
            same = int((tok == ref_backend.sample_tokens(dev, inv_t, k or 0, 41 + i,
                                                         step)).sum())
            print(f"SAMPLING kernel V{V} B{B} T{T} k{k} step{step}: decided {d}/{n}, "
                  f"equal to ref_backend {same}/{n}")
    assert decided >= 0.99 * rows


@pytest.mark.parametrize("V", [37, 65])
def test_candidate_sets(V):
    S.check_candidate_sets(_kernel, V, _place)


@pytest.mark.parametrize("V,top_k,temperature,bound", S.CHI2_CASES)
def test_distribution(V, top_k, temperature, bound):
    S.check_chi2(_kernel, V, top_k, temperature, bound, _place)


def test_binding_checks():
    logits = _place(S.bf16_logits(40, 4, 1.0, 5))
    ok = _kernel(logits, 1.25, 0, 1, 0)
    assert ok.dtype == torch.int64 and ok.shape == (4,) and ok.device == logits.device
    for bad in (logits.float(), logits[:, ::2], logits.t(), logits[0], logits[None]):
        with pytest.raises(RuntimeError):
            _kernel(bad, 1.25, 0, 1, 0)
    with pytest.raises(RuntimeError):
        _kernel(logits.cpu(), 1.25, 0, 1, 0)
    for inv_t in (0.0, -1.0, float("inf"), float("nan"), 1e60):
        with pytest.raises(RuntimeError):
            _kernel(logits, inv_t, 0, 1, 0)
    with pytest.raises(RuntimeError):
        _kernel(logits, 1.25, -1, 1, 0)
    for step in (-1, 1 << 32):
        with pytest.raises(RuntimeError):
            _kernel(logits, 1.25, 0, 1, step)
    assert torch.equal(_kernel(logits, 1.25, 0, 1, (1 << 32) - 1),
                       _kernel(logits, 1.25, 40, 1, (1 << 32) - 1))
    assert _kernel(logits[:0], 1.25, 0, 1, 0).shape == (0,)


def test_op_routing(monkeypatch):
    logits = _place(S.bf16_logits(520, 8, 4.0, 6))
    calls = []
    real = ops._C.sample_tokens
    monkeypatch.setattr(ops._C, "sample_tokens",
                        lambda *a: calls.append(a[1:]) or real(*a))
    a = ops.sample_tokens(logits, 0.8, 20, seed=-3, step=4)
    assert calls == [(S.inv_t_of(0.8), 20, -3, 4)]
    # fp32 and strided logits, and MIDGPT_FORCE_REF=1, go to ref_backend
    b = ops.sample_tokens(logits.float(), 0.8, 20, seed=-3, step=4)
    ops.sample_tokens(logits[:, :519], 0.8, 20, seed=-3, step=4)
    monkeypatch.setenv("MIDGPT_FORCE_REF", "1")
    c = ops.sample_tokens(logits, 0.8, 20, seed=-3, step=4)
    assert len(calls) == 1
    assert b.device == a.device and torch.equal(b, c)
    S.check_optimal(a, logits.cpu(), S.inv_t_of(0.8), 20, -3, 4)
    S.check_optimal(b, logits.cpu(), S.inv_t_of(0.8), 20, -3, 4)
    with pytest.raises(ValueError):
        ops.sample_tokens(logits, 0.0, seed=1, step=0)


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
def _model(seed):
    cfg = GPTConfig(block_size=128, vocab_size=512, n_layer=2, n_head=2,
                    n_embd=128, dropout=0.0)
    torch.manual_seed(seed)
    gm = GPT(cfg).to(DEV).to(BF).eval()
    gm.rope_sin = gm.rope_sin.float()
    gm.rope_cos = gm.rope_cos.float()
    return gm


def _counting(monkeypatch):
    calls = [0]
    real = ops._C.sample_tokens

    def counting(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    def boom(*a, **kw):
        raise AssertionError("torch.multinomial called on the seed= path")

    monkeypatch.setattr(ops._C, "sample_tokens", counting)
    monkeypatch.setattr(torch, "multinomial", boom)
    return calls


def test_generate_seeded_native(monkeypatch):
    from midgpt_amd import generate as G
    gm = _model(91)
    monkeypatch.delenv("MIDGPT_DECODE_REF", raising=False)
    assert G.native_decode(gm)
    idx = torch.randint(0, 512, (2, 120), generator=torch.Generator().manual_seed(92)).to(DEV)
    n_new = 12                               # 120 + 12 crosses the 128-token window
    calls = _counting(monkeypatch)
    out = G.generate(gm, idx, n_new, temperature=0.8, top_k=20, seed=5)
    assert calls[0] == n_new
    assert out.shape == (2, 120 + n_new) and torch.equal(out[:, :120], idx)
    assert torch.equal(out, G.generate(gm, idx, n_new, temperature=0.8, top_k=20, seed=5))
    step = G.decode_stepper(gm, 2)
    seq = idx
    logits = step(seq, 0)
    for t in range(n_new):
        nxt = ops.sample_tokens(logits, 0.8, 20, seed=5, step=t)
        seq = torch.cat([seq, nxt[:, None]], dim=1)
        logits = step(seq[:, -1:], seq.shape[1] - 1) if seq.shape[1] <= 128 \
            else step(seq[:, -128:], 0)
    assert torch.equal(out, seq)


def test_generate_ragged_seeded_native(monkeypatch):
    from midgpt_amd import generate as G
    gm = _model(77)
    monkeypatch.delenv("MIDGPT_DECODE_REF", raising=False)
    g = torch.Generator().manual_seed(78)
    lens = (3, 40, 120)                    # 120 + 12 crosses block_size 128
    prompts = [torch.randint(0, 512, (n,), generator=g).to(DEV) for n in lens]
    want = [n + min(12, 128 - n + 1) for n in lens]
    calls = _counting(monkeypatch)
    outs = G.generate_ragged(gm, prompts, 12, temperature=0.8, top_k=20, seed=5)
    assert calls[0] == 12
    assert [o.numel() for o in outs] == want
    for o, p in zip(outs, prompts):
        assert torch.equal(o[:p.numel()], p)
        assert 0 <= int(o.min()) and int(o.max()) < 512
    again = G.generate_ragged(gm, prompts, 12, temperature=0.8, top_k=20, seed=5)
    assert all(torch.equal(a, b) for a, b in zip(outs, again))
