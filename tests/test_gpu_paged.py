"""Paged decode kernels on the GPU (csrc/decode.hip PAGED instantiations,
``kv_store_paged_kernel``), ``decode_step_paged`` and the scheduler on a
``PagedKVCache``.

The contract of the paged kernels is bit-exactness with the ragged kernels on
the cache gathered through the block table, under ``torch.equal``, for every
num_splits: only the address of a cache row differs. B=3, H=2, C in {64, 128},
page size in {16, 64}, MP*PS = 256, a pool with spare pages, the pages dealt to
the sequences in a fixed scrambled, interleaved order (paged_util). Unused
pages, the rows past a sequence's length inside its last page and the unused
rows of the gathered cache hold NaN, and unused table entries are -1: a load
through the wrong page or past a length shows in the output, a store anywhere
else as a row that is no longer NaN."""
import pytest
import torch

import paged_util as PU
from paged_util import B, H, NAN, TMAX

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from midgpt_amd import ops
    from midgpt_amd.ops import reference as ref
    assert ops.have_ext(), f"HIP extension must be built: {ops._C_ERR}"

from midgpt_amd.config import GPTConfig
from midgpt_amd.models.gpt import GPT

DEV = "cuda:0"
BF = torch.bfloat16


def _randbf(g, *shape):
    return torch.randn(*shape, generator=g).to(BF).to(DEV)


def _i32(vals):
    return torch.as_tensor(vals).to(device=DEV, dtype=torch.int32)


# ---------------------------------------------------------------------------
# attn_decode_paged
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attn_inputs():
    """Per head dim: q (B,H,16,C) and B full K/V caches; read-only."""
    out = {}
    for C in (64, 128):
        g = torch.Generator().manual_seed(372 + C)
        out[C] = (_randbf(g, B, H, 16, C), _randbf(g, B, H, TMAX, C),
                  _randbf(g, B, H, TMAX, C))
    return out


CASES = [(1, (1, 9, 256)), (1, (2, 65, 200)), (1, (3, 64, 255)), (3, (3, 10, 200)),
         (16, (16, 17, 256))]


@pytest.mark.parametrize("PS", [16, 64])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("Tq,kv_lens", CASES)
def test_attn_decode_paged_equals_ragged_on_gathered_cache(attn_inputs, C, PS, Tq, kv_lens):
    q_all, k_all, v_all = attn_inputs[C]
    q = q_all[:, :, :Tq].contiguous()
    kg, vg, kp, vp, table, _ = PU.paged(k_all, v_all, kv_lens, PS)
    assert PU.nan_equal(PU.gather(kp, table, PS), kg)    # the set-up itself
    lens_h = torch.tensor(kv_lens)
    for num_splits in (0, 1, 2, 5):
        want = ops._C.attn_decode_ragged(q, kg, vg, _i32(kv_lens), lens_h, num_splits)
        got = ops._C.attn_decode_paged(q, kp, vp, _i32(kv_lens), lens_h, _i32(table), table,
                                       num_splits)
        assert got.shape == (B, Tq, H, C) and got.dtype == BF
        assert not bool(torch.isnan(got).any()), num_splits
        assert torch.equal(got, want), num_splits
        # the op: same bits, (B,Tq,H*C), with and without the caller's device copies
        o = ops.decode_attention_paged(q, kp, vp, kv_lens, table.tolist(),
                                       num_splits=num_splits)
        assert torch.equal(o, want.view(B, Tq, H * C))
        o = ops.decode_attention_paged(q, kp, vp, lens_h, table, _i32(kv_lens), _i32(table),
                                       num_splits)
        assert torch.equal(o, want.view(B, Tq, H * C))


@pytest.mark.parametrize("PS", [16, 64])
def test_attn_decode_paged_shared_page(attn_inputs, PS):
    C, kv_lens = 128, (PS + 4, 3 * PS, PS)
    q_all, k_all, v_all = attn_inputs[C]
    k_all, v_all = k_all.clone(), v_all.clone()
    k_all[1, :, :PS] = k_all[0, :, :PS]                  # one first page of data
    v_all[1, :, :PS] = v_all[0, :, :PS]
    kg, vg, kp, vp, table, _ = PU.paged(k_all, v_all, kv_lens, PS)
    kp[table[1, 0]] = NAN                                # row 1 loses its own first page
    vp[table[1, 0]] = NAN
    table[1, 0] = table[0, 0]                            # and reads row 0's
    q = q_all[:, :, :1].contiguous()
    for num_splits in (0, 2):
        got = ops.decode_attention_paged(q, kp, vp, kv_lens, table, num_splits=num_splits)
        assert not bool(torch.isnan(got).any())
        assert torch.equal(got, ops.decode_attention_ragged(q, kg, vg, kv_lens,
                                                            num_splits=num_splits))


# ---------------------------------------------------------------------------
# kv_append_paged, kv_store_paged
# ---------------------------------------------------------------------------
def _only_rows_written(pool_k, pool_v, kg, vg, table, PS, rows):
    """Positions ``rows[b]`` of sequence b equal the gathered result and are
    not NaN; every other row of every page is still NaN."""
    written = torch.zeros(pool_k.shape[0], PS, dtype=torch.bool)
    for b, rng in enumerate(rows):
        p = torch.tensor(list(rng))
        pg, r = table[b, p // PS], p % PS
        written[pg, r] = True
        for pool, g in ((pool_k, kg), (pool_v, vg)):
            got = pool[pg.to(DEV), :, r.to(DEV)]         # (n,H,C)
            assert torch.equal(got, g[b, :, rng.start:rng.stop].transpose(0, 1)), b
            assert not bool(torch.isnan(got).any()), b
    for pool in (pool_k, pool_v):
        rest = pool.permute(0, 2, 1, 3)[(~written).to(DEV)]
        assert bool(torch.isnan(rest).all())


@pytest.mark.parametrize("PS", [16, 64])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("Tn,pos", [(1, (0, 7, 255)), (16, (0, 7, 240))])
def test_kv_append_paged_equals_ragged_on_gathered_cache(C, PS, Tn, pos):
    g = torch.Generator().manual_seed(371)
    qkv = _randbf(g, B, Tn, 3, H, C)
    qw = (1.0 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    kw = (1.0 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    sin, cos = (t.contiguous() for t in ref.rope_tables(C, TMAX, device=DEV))
    kg = torch.full((B, H, TMAX, C), NAN, device=DEV, dtype=BF)
    vg = kg.clone()
    want = ops.kv_append_ragged(qkv, qw, kw, sin, cos, kg, vg, pos)
    table, P = PU.deal(PS)
    for j in range(TMAX // PS):                          # -1 where no row is written
        for b in range(B):
            if not (pos[b] // PS <= j <= (pos[b] + Tn - 1) // PS):
                table[b, j] = -1
    for dev_copies in (False, True):
        kp, vp = PU.nan_pool(P, PS, C, DEV, BF)
        extra = dict(pos_dev=_i32(pos), block_table_dev=_i32(table)) if dev_copies else {}
        q = ops.kv_append_paged(qkv, qw, kw, sin, cos, kp, vp, pos, table, **extra)
        assert q.shape == (B, H, Tn, C) and q.dtype == BF
        assert torch.equal(q, want)
        _only_rows_written(kp, vp, kg, vg, table, PS, [range(p, p + Tn) for p in pos])


@pytest.mark.parametrize("PS", [16, 64])
@pytest.mark.parametrize("C", [64, 128])
def test_kv_store_paged(C, PS):
    lens = (1, 17, 200)
    g = torch.Generator().manual_seed(373)
    k, v = _randbf(g, B, H, TMAX, C), _randbf(g, B, H, TMAX, C)
    table = PU.trim(PU.deal(PS)[0], PS, lens)
    P = PU.deal(PS)[1]
    for dev_copy in (False, True):
        kp, vp = PU.nan_pool(P, PS, C, DEV, BF)
        ops.kv_store_paged(k, v, kp, vp, lens, table,
                           **(dict(block_table_dev=_i32(table)) if dev_copy else {}))
        _only_rows_written(kp, vp, k, v, table, PS, [range(n) for n in lens])


def test_paged_binding_checks():
    C, PS = 64, 16
    g = torch.Generator().manual_seed(374)
    qkv = _randbf(g, B, 16, 3, H, C)
    qw = torch.ones(C, device=DEV)
    sin, cos = (t.contiguous() for t in ref.rope_tables(C, TMAX, device=DEV))
    table, P = PU.deal(PS)
    kp, vp = PU.nan_pool(P, PS, C, DEV, BF)
    q = torch.zeros(B, H, 1, C, device=DEV, dtype=BF)
    kv = torch.zeros(B, H, 32, C, device=DEV, dtype=BF)
    pos, lens, slens = (0, 7, 240), (3, 17, 256), (3, 17, 32)
    pos_h, lens_h, slens_h = torch.tensor(pos), torch.tensor(lens), torch.tensor(slens)

    def all_raise(t_dev, t_host, kpool=kp, vpool=vp):
        with pytest.raises(RuntimeError):
            ops._C.kv_append_paged(qkv, qw, qw, sin, cos, kpool, vpool, _i32(pos), pos_h,
                                   t_dev, t_host, 1e-6)
        with pytest.raises(RuntimeError):
            ops._C.attn_decode_paged(q, kpool, vpool, _i32(lens), lens_h, t_dev, t_host, 1)
        with pytest.raises(RuntimeError):
            ops._C.kv_store_paged(kv, kv, kpool, vpool, _i32(slens), slens_h, t_dev, t_host)

    for val in (-1, P):                                  # an entry inside the needed range
        t = table.clone()
        t[1, 1] = val
        all_raise(_i32(t), t)
        with pytest.raises(RuntimeError):
            ops.kv_append_paged(qkv, qw, qw, sin, cos, kp, vp, pos, t)
        with pytest.raises(RuntimeError):
            ops.decode_attention_paged(q, kp, vp, lens, t)
        with pytest.raises(RuntimeError):
            ops.kv_store_paged(kv, kv, kp, vp, slens, t)
    all_raise(table.clone(), table)                      # the device table on the CPU
    all_raise(table.to(DEV), table)                      # ... as int64
    all_raise(_i32(table[:, :8]), table)                 # the wrong MP
    all_raise(_i32(table), table.float())                # a host table that is no integer
    kp48, vp48 = PU.nan_pool(P, 48, C, DEV, BF)          # PS not a power of two
    all_raise(_i32(table), table, kp48, vp48)
    dup = table.clone()
    dup[2, 15] = dup[0, 0]                               # a written page named by two rows
    with pytest.raises(RuntimeError):
        ops._C.kv_append_paged(qkv, qw, qw, sin, cos, kp, vp, _i32(pos), pos_h, _i32(dup),
                               dup, 1e-6)
    dup = table.clone()
    dup[2, 0] = dup[1, 1]
    with pytest.raises(RuntimeError):
        ops._C.kv_store_paged(kv, kv, kp, vp, _i32(slens), slens_h, _i32(dup), dup)
    with pytest.raises(RuntimeError):                    # kv_len > MP*PS
        ops._C.attn_decode_paged(q, kp, vp, _i32((3, 17, 257)), torch.tensor((3, 17, 257)),
                                 _i32(table), table, 1)
    with pytest.raises(RuntimeError):                    # Tq > 16
        ops._C.attn_decode_paged(torch.zeros(B, H, 17, C, device=DEV, dtype=BF), kp, vp,
                                 _i32((100,) * 3), torch.tensor((100,) * 3), _i32(table),
                                 table, 1)
    with pytest.raises(RuntimeError):                    # rows past MP*PS
        ops._C.kv_append_paged(qkv, qw, qw, sin, cos, kp, vp, _i32(pos),
                               torch.tensor((0, 7, 241)), _i32(table), table, 1e-6)
    with pytest.raises(RuntimeError):                    # more rows than were given
        ops._C.kv_store_paged(kv, kv, kp, vp, _i32(slens), torch.tensor((3, 17, 33)),
                              _i32(table), table)
    # the existing entry points do not take a pool of pages
    with pytest.raises(RuntimeError):
        ops._C.attn_decode_ragged(q, kp, vp, _i32(lens), lens_h, 1)
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
def test_decode_step_paged_equals_ragged_on_compact_cache(n_embd, monkeypatch):
    from midgpt_amd import generate as G
    monkeypatch.delenv("MIDGPT_DECODE_REF", raising=False)
    gm = _model(n_embd, 375)
    assert G.native_decode(gm)
    g = torch.Generator().manual_seed(376)
    PS = 16
    lens, steps, seats = (46, 100), 4, (3, 1)     # 46 -> 50 crosses the boundary at 48
    seqs = [torch.randint(0, 512, (n + steps,), generator=g) for n in lens]
    compact = G.KVCache(gm, 2)
    G.prefill_ragged(gm, [s[:n] for s, n in zip(seqs, lens)], compact)
    pool = G.PagedKVCache(gm, 4, 20, page_size=PS)
    pool.buf.fill_(NAN)
    pool.alloc(0, 16)                             # page 0: a seat that does not step
    pool.alloc(1, lens[1] + steps)                # pages 1..7
    pool.alloc(2, 16)                             # page 8
    pool.alloc(3, lens[0] + steps)                # pages 9..12
    pool.free(0)
    pool.free(2)
    for b, s in enumerate(seats):                 # the prompts' K/V through the table
        for li in range(2):
            ops.kv_store_paged(compact.k[li][b:b + 1], compact.v[li][b:b + 1], pool.k[li],
                               pool.v[li], [lens[b]], pool.table[s:s + 1])
        pool.lens[s] = lens[b]
    pool.upload()
    for t in range(steps):
        nxt = torch.stack([s[n + t] for s, n in zip(seqs, lens)]).to(DEV)[:, None]
        want = G.decode_step_ragged(gm, nxt, compact)
        got = G.decode_step_paged(gm, nxt, pool, seats)
        assert torch.equal(got, want), t
        assert not bool(torch.isnan(got).any())
    assert pool.lens == [0, lens[1] + steps, 0, lens[0] + steps]
    assert pool.lens_dev.tolist() == pool.lens
    used = pool.pages[1] + pool.pages[3]
    assert used == list(range(1, 8)) + list(range(9, 13))
    untouched = [p for p in range(20) if p not in used]
    assert bool(torch.isnan(pool.buf[:, :, untouched]).all())
    for b, s in enumerate(seats):                 # and the rows past each length
        n = lens[b] + steps
        last = pool.pages[s][-1]
        assert bool(torch.isnan(pool.buf[:, :, last, :, n % PS:]).all()) or n % PS == 0
        assert not bool(torch.isnan(pool.buf[:, :, last, :, :n % PS]).any())


def test_scheduler_paged_equals_unpaged_native(monkeypatch):
    from midgpt_amd import generate as G
    monkeypatch.delenv("MIDGPT_DECODE_REF", raising=False)
    gm = _model(128, 377)
    g = torch.Generator().manual_seed(378)
    X = torch.randint(0, 512, (90,), generator=g).to(DEV)    # flash prefill, dirties pages
    A = torch.randint(0, 512, (33,), generator=g).to(DEV)
    Z = torch.randint(0, 512, (9,), generator=g).to(DEV)     # the 16-row paged pair
    calls = [0]
    real = ops._C.attn_decode_paged

    def counting(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(ops._C, "attn_decode_paged", counting)

    def run(**pages):
        sched = G.DecodeScheduler(gm, 1, tick_every=4, **pages)   # one seat, reused
        hs = [sched.submit(X, 30, temperature=0.8, top_k=20, seed=3),
              sched.submit(A, 12, temperature=0),
              sched.submit(Z, 20, temperature=0.9, top_k=50, seed=5, row=2)]
        done = sched.run()
        assert [id(h) for h in done] == [id(h) for h in hs]
        return sched, [h.tokens for h in hs]

    _, want = run()
    assert calls[0] == 0
    for PS, P in ((16, 8), (64, 3)):
        before = calls[0]
        sched, got = run(num_pages=P, page_size=PS)
        assert calls[0] > before
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert sched.cache.free_pages == list(range(P))
    assert got[0].numel() == 90 + 30 and torch.equal(got[0][:90], X)
    assert torch.equal(got[1], G.generate_ragged(gm, [A], 12, temperature=0)[0])
