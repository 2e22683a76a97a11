"""Slot-mapped decode kernels and per-row sampling on the GPU (csrc/decode.hip
SLOTS instantiations, ``sample_tokens_rows_kernel``), and the scheduler built
on them.

The contract of the slotted kernels is bit-exactness with the ragged kernels on
the gathered cache ``cache[slots]`` under ``torch.equal``, for every
num_splits. Unused slots, and rows at and beyond each sequence's own length,
hold NaN: a load through the wrong slot or past a length shows in the output,
a store anywhere else as a row that is no longer NaN. ``sample_tokens_rows``
is judged as tests/test_gpu_sampling.py judges the uniform kernel (the fp64
oracle and the 2 eps rule of sampling_util), row by row through the identity
``rows(...)[b] == sample_tokens(X, ...)[r_b]``."""
import pytest
import torch

import sampling_util as SU

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
S, B, H, TMAX = 5, 3, 2, 256
SLOTS = (4, 0, 2)
NAN = float("nan")


def _randbf(g, *shape):
    return torch.randn(*shape, generator=g).to(BF).to(DEV)


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


def _nan_pool(C, n=S):
    return (torch.full((n, H, TMAX, C), NAN, device=DEV, dtype=BF),
            torch.full((n, H, TMAX, C), NAN, device=DEV, dtype=BF))


# ---------------------------------------------------------------------------
# attn_decode_slots
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attn_inputs():
    """Per head dim: q (B,H,16,C) and B full K/V caches; read-only."""
    out = {}
    for C in (64, 128):
        g = torch.Generator().manual_seed(172 + C)
        out[C] = (_randbf(g, B, H, 16, C), _randbf(g, B, H, TMAX, C),
                  _randbf(g, B, H, TMAX, C))
    return out


def _pool(inputs, C, Tq, kv_lens, slots, n_slots):
    """q, the compact (gathered) caches with NaN past each length, and a pool
    of n_slots that holds sequence b in slot slots[b] and NaN everywhere else."""
    q_all, k_all, v_all = inputs[C]
    q = q_all[:, :, :Tq].contiguous()
    kg, vg = k_all.clone(), v_all.clone()
    for b, n in enumerate(kv_lens):
        kg[b, :, n:] = NAN
        vg[b, :, n:] = NAN
    kp, vp = _nan_pool(C, n_slots)
    kp[list(slots)] = kg
    vp[list(slots)] = vg
    return q, kg, vg, kp, vp


CASES = [(1, (1, 9, 256)), (1, (2, 65, 200)), (1, (3, 64, 255)), (3, (3, 10, 200)),
         (16, (16, 17, 256))]


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("Tq,kv_lens", CASES)
def test_attn_decode_slots_equals_ragged_on_gathered_cache(attn_inputs, C, Tq, kv_lens):
    q, kg, vg, kp, vp = _pool(attn_inputs, C, Tq, kv_lens, SLOTS, S)
    qi, _, _, kpi, vpi = _pool(attn_inputs, C, Tq, kv_lens, (0, 1, 2), 3)
    lens_h = torch.tensor(kv_lens)
    for num_splits in (0, 1, 2, 5):
        want = ops._C.attn_decode_ragged(q, kg, vg, _i32(kv_lens), lens_h, num_splits)
        got = ops._C.attn_decode_slots(q, kp, vp, _i32(kv_lens), lens_h, _i32(SLOTS),
                                       torch.tensor(SLOTS), num_splits)
        assert got.shape == (B, Tq, H, C) and got.dtype == BF
        assert not bool(torch.isnan(got).any()), num_splits
        assert torch.equal(got, want), num_splits
        # the identity map in a pool of 3: the ragged call on the pool itself
        ident = ops._C.attn_decode_slots(qi, kpi, vpi, _i32(kv_lens), lens_h, _i32((0, 1, 2)),
                                         torch.tensor((0, 1, 2)), num_splits)
        assert torch.equal(ident, ops._C.attn_decode_ragged(qi, kpi, vpi, _i32(kv_lens),
                                                            lens_h, num_splits)), num_splits
        assert torch.equal(ident, want), num_splits
        # the op: same bits, (B,Tq,H*C), with and without the caller's device copies
        o = ops.decode_attention_slots(q, kp, vp, kv_lens, SLOTS, num_splits=num_splits)
        assert torch.equal(o, want.view(B, Tq, H * C))
        o = ops.decode_attention_slots(q, kp, vp, lens_h, torch.tensor(SLOTS), _i32(kv_lens),
                                       _i32(SLOTS), num_splits)
        assert torch.equal(o, want.view(B, Tq, H * C))


# ---------------------------------------------------------------------------
# kv_append_slots
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("Tn,pos", [(1, (0, 7, 255)), (16, (0, 100, 240))])
def test_kv_append_slots_equals_ragged_on_gathered_cache(C, Tn, pos):
    g = torch.Generator().manual_seed(171)
    qkv = _randbf(g, B, Tn, 3, H, C)
    qw = (1.0 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    kw = (1.0 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    sin, cos = (t.contiguous() for t in ref.rope_tables(C, TMAX, device=DEV))
    kg, vg = _nan_pool(C, B)
    want = ops.kv_append_ragged(qkv, qw, kw, sin, cos, kg, vg, pos)
    for dev_copies in (False, True):
        kp, vp = _nan_pool(C)
        extra = dict(pos_dev=_i32(pos), slots_dev=_i32(SLOTS)) if dev_copies else {}
        q = ops.kv_append_slots(qkv, qw, kw, sin, cos, kp, vp, pos, SLOTS, **extra)
        assert q.shape == (B, H, Tn, C) and q.dtype == BF
        assert torch.equal(q, want)
        for b, s in enumerate(SLOTS):
            rows = slice(pos[b], pos[b] + Tn)
            assert torch.equal(kp[s, :, rows], kg[b, :, rows]), b
            assert torch.equal(vp[s, :, rows], vg[b, :, rows]), b
            assert not bool(torch.isnan(kp[s, :, rows]).any()), b
            for t in (kp, vp):             # every other row of the slot
                assert bool(torch.isnan(t[s, :, :pos[b]]).all()), b
                assert bool(torch.isnan(t[s, :, pos[b] + Tn:]).all()), b
        for s in (1, 3):                   # the two unused slots
            assert bool(torch.isnan(kp[s]).all()) and bool(torch.isnan(vp[s]).all())


# ---------------------------------------------------------------------------
# sample_tokens_rows_kernel
# ---------------------------------------------------------------------------
def _place(logits):
    """The CPU (B, V) bf16 logits as a contiguous view inside a +3e38 buffer."""
    n, V = logits.shape
    pad = 64                                  # elements: keeps row 0 16-byte aligned
    buf = torch.full((pad + n * V + pad,), 3e38, dtype=BF, device=DEV)
    view = buf[pad:pad + n * V].view(n, V)
    view.copy_(logits)
    return view


@pytest.mark.parametrize("V", [37, 2056, 50304])
def test_sample_tokens_rows_kernel(V):
    n = 8
    logits = SU.bf16_logits(V, n, 4.0, 400 + V)
    temps = [0.7, 1.0, 0.1, 0.8, 0.0, 0.9, 1.3, 0.5]
    top_k = [None, 1, 50, V, 50, 50, None, 1]
    seeds = [41, -3, 1 << 40, 7, 8, (1 << 63) + 5, 12, 13]
    steps = [0, 7, 1, (1 << 32) - 1, 3, 2, 100, 6]
    rows = [0, 3, 1, 2, 5, 6, 2, 1]
    logits[4, [V - 2, 9, 20]] = 300.0          # the greedy row: a tied maximum
    dev = _place(logits)
    calls = []
    real = ops._C.sample_tokens_rows
    ops._C.sample_tokens_rows = lambda *a: calls.append(1) or real(*a)
    try:
        got = ops.sample_tokens_rows(dev, temps, top_k, seeds=seeds, steps=steps, rows=rows)
    finally:
        ops._C.sample_tokens_rows = real
    assert calls == [1]
    assert got.dtype == torch.int64 and got.shape == (n,) and got.device == dev.device
    host = ops.sample_row_params(temps, top_k, seeds, steps, rows, n)
    want_ref = ref_backend.sample_tokens_rows(dev, ops.pack_sample_params(*host), *host)
    assert torch.equal(got, want_ref)
    assert int(got[4]) == 9
    for b in range(n):
        if temps[b] <= 0:
            continue
        inv_t, k = SU.inv_t_of(temps[b]), top_k[b] or 0
        X = torch.zeros(rows[b] + 1, V, dtype=BF)
        X[rows[b]] = logits[b]
        # the uniform kernel on a batch that holds these logits in row r_b
        uni = ops._C.sample_tokens(_place(X), inv_t, k, ops._seed_i64(seeds[b]), steps[b])
        assert int(got[b]) == int(uni[rows[b]]), b
        # the oracle judges that batch with this kernel's token in row r_b
        # (the other rows, all zeros, carry the uniform kernel's draws)
        tok = uni.clone()
        tok[rows[b]] = got[b]
        SU.check_optimal(tok, X, inv_t, top_k[b], seeds[b], steps[b])


def test_slot_binding_checks():
    C = 64
    g = torch.Generator().manual_seed(174)
    qkv = _randbf(g, B, 2, 3, H, C)
    qw = torch.ones(C, device=DEV)
    sin, cos = (t.contiguous() for t in ref.rope_tables(C, TMAX, device=DEV))
    kp, vp = _nan_pool(C)
    q = torch.zeros(B, H, 1, C, device=DEV, dtype=BF)
    pos, lens = (0, 1, 2), (3, 3, 3)
    bad_maps = [(4, 0, 4), (4, 0, S), (4, -1, 2), (4, 0), torch.tensor([4.0, 0.0, 2.0])]
    for bad in bad_maps:
        t = bad if isinstance(bad, torch.Tensor) else torch.tensor(bad)
        with pytest.raises(RuntimeError):
            ops._C.kv_append_slots(qkv, qw, qw, sin, cos, kp, vp, _i32(pos), torch.tensor(pos),
                                   _i32(SLOTS), t, 1e-6)
        with pytest.raises(RuntimeError):
            ops._C.attn_decode_slots(q, kp, vp, _i32(lens), torch.tensor(lens), _i32(SLOTS),
                                     t, 1)
        with pytest.raises(RuntimeError):
            ops.kv_append_slots(qkv, qw, qw, sin, cos, kp, vp, pos, bad)
        with pytest.raises(RuntimeError):
            ops.decode_attention_slots(q, kp, vp, lens, bad)
    ok = torch.tensor(SLOTS)
    with pytest.raises(RuntimeError):      # device copy on the CPU / int64
        ops._C.attn_decode_slots(q, kp, vp, _i32(lens), torch.tensor(lens), ok, ok, 1)
    with pytest.raises(RuntimeError):
        ops._C.attn_decode_slots(q, kp, vp, _i32(lens), torch.tensor(lens), ok.to(DEV), ok, 1)
    with pytest.raises(RuntimeError):      # fewer slots than rows
        ops._C.attn_decode_slots(q, kp[:2], vp[:2], _i32(lens), torch.tensor(lens),
                                 _i32((0, 1, 2)), torch.tensor((0, 1, 2)), 1)
    with pytest.raises(RuntimeError):      # positions follow the ragged checks
        ops._C.kv_append_slots(qkv, qw, qw, sin, cos, kp, vp, _i32(pos),
                               torch.tensor((0, 1, TMAX - 1)), _i32(SLOTS), ok, 1e-6)
    # the existing entry points still want cache dim 0 == B
    with pytest.raises(RuntimeError):
        ops._C.attn_decode_ragged(q, kp, vp, _i32(lens), torch.tensor(lens), 1)
    logits = _place(SU.bf16_logits(40, 2, 1.0, 5))
    host = list(ops.sample_row_params(1.0, None, [1, 2], [0, 0], [0, 1], 2))
    packed = ops.pack_sample_params(*host, device=DEV)
    assert ops._C.sample_tokens_rows(logits, packed, *host).shape == (2,)
    for i, bad in ((0, torch.tensor([1.0, -1.0])), (0, torch.tensor([1.0, float("inf")])),
                   (0, torch.tensor([1.0])), (1, torch.tensor([0, -1])),
                   (3, torch.tensor([0, 1 << 32])), (4, torch.tensor([-1, 0])),
                   (2, torch.tensor([1.0, 2.0]))):
        args = list(host)
        args[i] = bad
        with pytest.raises(RuntimeError):
            ops._C.sample_tokens_rows(logits, packed, *args)
    for bad in (packed.cpu(), packed[:, :5].contiguous(), packed.long()):
        with pytest.raises(RuntimeError):
            ops._C.sample_tokens_rows(logits, bad, *host)
    torch.cuda.synchronize()
    assert bool(torch.isnan(kp).all()) and bool(torch.isnan(vp).all())


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
def _model(n_embd, seed):
    cfg = GPTConfig(block_size=128, vocab_size=512, n_layer=2, n_head=2,
                    n_embd=n_embd, dropout=0.0)
    torch.manual_seed(seed)
    gm = GPT(cfg).to(DEV).to(BF).eval()
    gm.rope_sin = gm.rope_sin.float()
    gm.rope_cos = gm.rope_cos.float()
    return gm


@pytest.mark.parametrize("n_embd", [128, 256])   # head dim 64, 128
def test_decode_step_slots_equals_ragged_on_compact_cache(n_embd, monkeypatch):
    from midgpt_amd import generate as G
    monkeypatch.delenv("MIDGPT_DECODE_REF", raising=False)
    gm = _model(n_embd, 175)
    assert G.native_decode(gm)
    g = torch.Generator().manual_seed(176)
    lens, steps, slots = (40, 100), 4, (3, 1)
    seqs = [torch.randint(0, 512, (n + steps,), generator=g) for n in lens]
    compact = G.KVCache(gm, 2)
    G.prefill_ragged(gm, [s[:n] for s, n in zip(seqs, lens)], compact)
    pool = G.KVCache(gm, 4)
    pool.buf.fill_(NAN)
    pool.buf[:, :, list(slots)] = compact.buf
    pool.set_lens([0, lens[1], 0, lens[0]])
    for t in range(steps):
        nxt = torch.stack([s[n + t] for s, n in zip(seqs, lens)]).to(DEV)[:, None]
        want = G.decode_step_ragged(gm, nxt, compact)
        got = G.decode_step_slots(gm, nxt, pool, slots)
        assert torch.equal(got, want), t
        assert not bool(torch.isnan(got).any())
    assert pool.lens == [0, lens[1] + steps, 0, lens[0] + steps]
    assert pool.lens_dev.tolist() == pool.lens
    assert bool(torch.isnan(pool.buf[:, :, [0, 2]]).all())


def test_scheduler_slot_hygiene_native(monkeypatch):
    from midgpt_amd import generate as G
    monkeypatch.delenv("MIDGPT_DECODE_REF", raising=False)
    gm = _model(128, 177)
    g = torch.Generator().manual_seed(178)
    X = torch.randint(0, 512, (90,), generator=g).to(DEV)
    A = torch.randint(0, 512, (33,), generator=g).to(DEV)
    calls = [0]
    real = ops._C.attn_decode_slots

    def counting(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(ops._C, "attn_decode_slots", counting)
    sched = G.DecodeScheduler(gm, 1, tick_every=4)
    hx = sched.submit(X, 30, temperature=0.8, top_k=20, seed=3)   # dirties the slot
    ha = sched.submit(A, 12, temperature=0)
    done = sched.run()
    assert [id(h) for h in done] == [id(hx), id(ha)] and calls[0] > 0
    assert hx.tokens.numel() == 90 + 30 and torch.equal(hx.tokens[:90], X)
    want = G.generate_ragged(gm, [A], 12, temperature=0)[0]
    assert torch.equal(ha.tokens, want)
