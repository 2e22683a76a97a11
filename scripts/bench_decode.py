"""Decode benchmarks (run on the GPU box; fails without a GPU).

  --which kernels   attn_decode (+ combine) and kv_append microbench: time and
                    achieved bytes/s against the HBM peak. The byte count is
                    the algorithmic one, K and V read once:
                    2 * B*H*kv_len*C * 2 bytes. Each call reads a different
                    cache out of a ring of >= 1 GiB, so the 256 MiB Infinity
                    Cache cannot hold the working set (in a real decode step
                    the other layers' caches evict it in the same way).
  --sweep           with kernels: every num_splits in 1,2,4,..,64 next to the
                    automatic choice (the measurements behind the split rule).
                    Then the ragged rows: attn_decode_ragged with all lengths
                    equal next to attn_decode at the same shape (B=8 and B=64),
                    and skewed batches (B=8, lengths spread over 128..4096) at
                    the automatic split count (the rule on the longest
                    sequence) and at every column of the sweep.
  --which ragged    openwebtext_xl architecture, random weights, 8 prompts of
                    16..512 tokens, 128 new tokens each, greedy:
                    generate_ragged on the batch against generate() once per
                    prompt at B=1, alternating in this process, each warmed up.
  --which e2e       generate() on the openwebtext_xl architecture, random
                    weights, 128-token prompt + 256 new tokens, greedy: native
                    path and MIDGPT_DECODE_REF=1 alternating in this process,
                    each warmed up, host clock around a final synchronise.
  --which count     one generate() of --new tokens on the path the
                    environment selects and nothing else: run it under
                    ``rocprofv3 --kernel-trace --stats`` at two values of
                    --new; the difference in dispatches is launches per token.
                    Greedy, or with --sampled at temperature 0.8, top_k 50,
                    seed= (the sample_tokens kernel).
  --which sampling  the last step of a token. Kernel: ops.sample_tokens at
                    B = 1, 8, 64, V = 50304, top_k none and 50, against
                    generate._sample (the torch chain) on the same logits with
                    the device multinomial and with a CPU generator (the
                    probability matrix copied to the host), the three
                    alternating over a ring of 4 logit tensors: hot in cache,
                    as the lm_head has just written them in a real step. End
                    to end: the --which ragged set-up at temperature 0.8,
                    top_k 50 with seed=, the same with a CPU generator, and
                    greedy, alternating.
  --which slots     attn_decode_slots and kv_append_slots with the identity map
                    and with a permuted map against the ragged ops on the same
                    ring of caches (a cache of the ring is the pool, S = B),
                    the three alternating x 3, at the B8 / B64 shapes of the
                    ragged table.
  --which continuous  openwebtext_xl architecture, random weights, greedy: 32
                    requests, prompt lengths cycling through the eight of the
                    ragged case, budgets cycling through 16, 64, 128, 256 new
                    tokens. DecodeScheduler with 8 slots against
                    generate_ragged on the requests in arrival order, four
                    batches of 8 (each batch runs to its longest budget), the
                    two alternating in this process, each warmed up. Tokens/s =
                    tokens requested / wall time.
                    With --pages: the same 32 requests on the unpaged
                    DecodeScheduler with 8 slots against DecodeScheduler on a
                    PagedKVCache of the same byte size (8 * block_size /
                    page_size pages of --page_size positions) with 8, 16 and
                    32 seats, the four alternating.
  --which paged     attn_decode_paged and kv_append_paged with the pages in
                    order and scrambled, page sizes 16, 64 and 128, against the
                    slotted ops with the identity map on caches of the same
                    byte size, all alternating x 3, at the --which slots
                    shapes.
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import statistics
import time

import torch

from midgpt_amd import ops
from midgpt_amd.ops import reference as ref

assert torch.cuda.is_available(), "bench_decode.py needs a GPU"
assert ops.have_ext(), f"HIP extension missing: {ops._C_ERR}"
DEV = "cuda:0"
BF = torch.bfloat16
HBM_PEAK = 8.0e12       # bytes/s, MI355X HBM3E spec
HBM_COPY = 6.29e12      # bytes/s, measured float4 copy
RING_BYTES = 1 << 30


def time_ring(fns, iters, warmup=10):
    """Mean seconds per call, cycling through fns (one per ring slot)."""
    n = len(fns)
    for i in range(max(warmup, n)):
        fns[i % n]()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fns[i % n]()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_attn_decode(B, H, C, kv_len, sweep):
    nbytes = 2 * B * H * kv_len * C * 2          # K and V once, bf16
    ring = max(1, min(32, -(-RING_BYTES // nbytes)))
    caches = [(torch.randn(B, H, kv_len, C, device=DEV, dtype=BF),
               torch.randn(B, H, kv_len, C, device=DEV, dtype=BF))
              for _ in range(ring)]
    q = torch.randn(B, H, 1, C, device=DEV, dtype=BF)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    auto = ops._C.attn_decode_auto_splits(B * H, kv_len, cus)
    iters = 200 if nbytes < (64 << 20) else 50
    splits = [0] + ([s for s in (1, 2, 4, 8, 16, 32, 64)] if sweep else [])
    for s in splits:
        fns = [(lambda k=k, v=v: ops._C.attn_decode(q, k, v, kv_len, s))
               for k, v in caches]
        reps = [time_ring(fns, iters) for _ in range(3)]
        t = statistics.median(reps)
        tag = f"auto={auto}" if s == 0 else f"{s:4d}"
        print(f"attn_decode B{B} H{H} C{C} kv{kv_len} splits {tag:>7}: "
              f"{t*1e6:9.1f} us (min {min(reps)*1e6:.1f} max {max(reps)*1e6:.1f})  "
              f"{nbytes/1e6:8.1f} MB  {nbytes/t/1e12:5.2f} TB/s  "
              f"{100*nbytes/t/HBM_PEAK:5.1f}% of 8.0 TB/s peak, "
              f"{100*nbytes/t/HBM_COPY:5.1f}% of 6.29 TB/s copy", flush=True)
    del caches


def bench_kv_append(B, H=16, C=128, Tmax=1024):
    qkv = torch.randn(B, 1, 3, H, C, device=DEV, dtype=BF)
    qw = torch.ones(C, device=DEV)
    kw = torch.ones(C, device=DEV)
    sin, cos = (t.contiguous() for t in ref.rope_tables(C, Tmax, device=DEV))
    kc = torch.zeros(B, H, Tmax, C, device=DEV, dtype=BF)
    vc = torch.zeros_like(kc)
    fn = lambda: ops._C.kv_append(qkv, qw, kw, sin, cos, kc, vc, 500, 1e-6)
    reps = [time_ring([fn], 500) for _ in range(3)]
    nbytes = 2 * qkv.numel() * 2
    print(f"kv_append   B{B} H{H} C{C} Tn1: {statistics.median(reps)*1e6:9.1f} us "
          f"(min {min(reps)*1e6:.1f} max {max(reps)*1e6:.1f})  {nbytes/1e3:.1f} kB "
          f"moved: launch-bound, back-to-back enqueue time", flush=True)
    pos_host = torch.full((B,), 500, dtype=torch.int64)
    pos_dev = pos_host.to(device=DEV, dtype=torch.int32)
    fn = lambda: ops._C.kv_append_ragged(qkv, qw, kw, sin, cos, kc, vc, pos_dev,
                                         pos_host, 1e-6)
    reps = [time_ring([fn], 500) for _ in range(3)]
    print(f"kv_append_ragged B{B} H{H} C{C} Tn1: {statistics.median(reps)*1e6:6.1f} us "
          f"(min {min(reps)*1e6:.1f} max {max(reps)*1e6:.1f})", flush=True)


def _reps_us(fns, iters):
    reps = [time_ring(fns, iters) * 1e6 for _ in range(3)]
    return statistics.median(reps), min(reps), max(reps)


def bench_ragged_equal(B, H, C, kv_len):
    """attn_decode_ragged with all lengths equal against attn_decode, the two
    alternating (uniform, ragged, uniform, ragged ...) over the same ring."""
    nbytes = 2 * B * H * kv_len * C * 2
    ring = max(1, min(32, -(-RING_BYTES // nbytes)))
    caches = [(torch.randn(B, H, kv_len, C, device=DEV, dtype=BF),
               torch.randn(B, H, kv_len, C, device=DEV, dtype=BF))
              for _ in range(ring)]
    q = torch.randn(B, H, 1, C, device=DEV, dtype=BF)
    lens_host = torch.full((B,), kv_len, dtype=torch.int64)
    lens_dev = lens_host.to(device=DEV, dtype=torch.int32)
    iters = 200 if nbytes < (64 << 20) else 50
    uni = [(lambda k=k, v=v: ops._C.attn_decode(q, k, v, kv_len, 0)) for k, v in caches]
    rag = [(lambda k=k, v=v: ops._C.attn_decode_ragged(q, k, v, lens_dev, lens_host, 0))
           for k, v in caches]
    res = {"uniform": [], "ragged": []}
    for _ in range(3):
        res["uniform"].append(time_ring(uni, iters) * 1e6)
        res["ragged"].append(time_ring(rag, iters) * 1e6)
    for name, r in res.items():
        print(f"attn_decode {name:7s} B{B} H{H} C{C} kv{kv_len} auto: "
              f"{statistics.median(r):9.1f} us (min {min(r):.1f} max {max(r):.1f})",
              flush=True)
    del caches


def bench_ragged_skewed(B, H, C, lens, sweep):
    """A skewed batch: bytes are the keys the sequences actually hold."""
    Tmax = max(lens)
    nbytes = 2 * H * sum(lens) * C * 2
    alloc = 2 * B * H * Tmax * C * 2
    ring = max(1, min(32, -(-RING_BYTES // alloc)))
    caches = [(torch.randn(B, H, Tmax, C, device=DEV, dtype=BF),
               torch.randn(B, H, Tmax, C, device=DEV, dtype=BF))
              for _ in range(ring)]
    q = torch.randn(B, H, 1, C, device=DEV, dtype=BF)
    lens_host = torch.tensor(lens, dtype=torch.int64)
    lens_dev = lens_host.to(device=DEV, dtype=torch.int32)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    auto = ops._C.attn_decode_auto_splits(B * H, Tmax, cus)
    for s in [0] + ([1, 2, 4, 8, 16, 32, 64] if sweep else []):
        fns = [(lambda k=k, v=v: ops._C.attn_decode_ragged(q, k, v, lens_dev, lens_host, s))
               for k, v in caches]
        med, lo, hi = _reps_us(fns, 100)
        tag = f"auto={auto}" if s == 0 else f"{s:4d}"
        print(f"attn_decode ragged  B{B} H{H} C{C} lens {list(lens)} splits {tag:>7}: "
              f"{med:9.1f} us (min {lo:.1f} max {hi:.1f})  {nbytes/1e6:8.1f} MB  "
              f"{nbytes/(med*1e-6)/1e12:5.2f} TB/s", flush=True)
    # the same keys as a uniform batch padded to the longest: what a caller
    # without the ragged kernel would have to read
    fns = [(lambda k=k, v=v: ops._C.attn_decode(q, k, v, Tmax, 0)) for k, v in caches]
    med, lo, hi = _reps_us(fns, 100)
    print(f"attn_decode uniform B{B} H{H} C{C} all at kv{Tmax} auto={auto}: "
          f"{med:9.1f} us (min {lo:.1f} max {hi:.1f})", flush=True)
    del caches


def bench_ragged_e2e(reps, n_new=128):
    from midgpt_amd.generate import generate, generate_ragged
    model, cfg = xl_model()
    lens = [16, 48, 96, 160, 240, 320, 416, 512]
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).to(DEV) for n in lens]
    print(f"ragged e2e: openwebtext_xl, prompts {lens}, {n_new} new tokens each, greedy; "
          "time includes the prompts", flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def batch(n):
        outs = generate_ragged(model, prompts, n, temperature=0.0)
        assert [o.numel() for o in outs] == [m + n for m in lens]

    def one_by_one(n):
        for p in prompts:
            assert generate(model, p[None], n, temperature=0.0).shape == (1, p.numel() + n)

    for fn in (batch, one_by_one):                        # warm up both
        fn(8)
    res = {"generate_ragged B=8": [], "generate x8 at B=1": []}
    for _ in range(reps):                                 # alternating
        res["generate_ragged B=8"].append(timed(lambda: batch(n_new)))
        res["generate x8 at B=1"].append(timed(lambda: one_by_one(n_new)))
    for name, ts in res.items():
        tps = sorted(len(lens) * n_new / t for t in ts)
        print(f"ragged e2e {name:20s}: tokens/s median {statistics.median(tps):8.1f} "
              f"min {tps[0]:8.1f} max {tps[-1]:8.1f}  (wall median "
              f"{statistics.median(ts)*1e3:8.1f} ms) over {reps} runs", flush=True)
    a, b = (statistics.median(res[k]) for k in res)
    print(f"ragged e2e speed ratio of medians (batch over one-by-one): {b/a:.2f}x",
          flush=True)


def bench_slots(B, H, C, kv_len):
    """attn_decode_slots (identity map, permuted map) against
    attn_decode_ragged, the three alternating over the same ring; then the
    same for kv_append at Tn = 1."""
    nbytes = 2 * B * H * kv_len * C * 2
    ring = max(1, min(32, -(-RING_BYTES // nbytes)))
    caches = [(torch.randn(B, H, kv_len, C, device=DEV, dtype=BF),
               torch.randn(B, H, kv_len, C, device=DEV, dtype=BF))
              for _ in range(ring)]
    q = torch.randn(B, H, 1, C, device=DEV, dtype=BF)
    lens_host = torch.full((B,), kv_len, dtype=torch.int64)
    lens_dev = lens_host.to(device=DEV, dtype=torch.int32)
    ident = torch.arange(B)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(0))
    maps = {"slots identity": (ident.to(device=DEV, dtype=torch.int32), ident),
            "slots permuted": (perm.to(device=DEV, dtype=torch.int32), perm)}
    iters = 200 if nbytes < (64 << 20) else 50
    paths = {"ragged": [(lambda k=k, v=v: ops._C.attn_decode_ragged(
        q, k, v, lens_dev, lens_host, 0)) for k, v in caches]}
    for name, (sd, sh) in maps.items():
        paths[name] = [(lambda k=k, v=v, sd=sd, sh=sh: ops._C.attn_decode_slots(
            q, k, v, lens_dev, lens_host, sd, sh, 0)) for k, v in caches]
    res = {name: [] for name in paths}
    for _ in range(3):                                    # alternating
        for name, fns in paths.items():
            res[name].append(time_ring(fns, iters) * 1e6)
    for name, r in res.items():
        print(f"attn_decode {name:14s} B{B} H{H} C{C} kv{kv_len} auto: "
              f"{statistics.median(r):9.1f} us (min {min(r):.1f} max {max(r):.1f})",
              flush=True)
    qkv = torch.randn(B, 1, 3, H, C, device=DEV, dtype=BF)
    qw = torch.ones(C, device=DEV)
    sin, cos = (t.contiguous() for t in ref.rope_tables(C, kv_len, device=DEV))
    pos_host = torch.full((B,), kv_len - 1, dtype=torch.int64)
    pos_dev = pos_host.to(device=DEV, dtype=torch.int32)
    kc, vc = caches[0]
    paths = {"ragged": [lambda: ops._C.kv_append_ragged(qkv, qw, qw, sin, cos, kc, vc, pos_dev,
                                                        pos_host, 1e-6)]}
    for name, (sd, sh) in maps.items():
        paths[name] = [lambda sd=sd, sh=sh: ops._C.kv_append_slots(
            qkv, qw, qw, sin, cos, kc, vc, pos_dev, pos_host, sd, sh, 1e-6)]
    res = {name: [] for name in paths}
    for _ in range(3):
        for name, fns in paths.items():
            res[name].append(time_ring(fns, 500) * 1e6)
    for name, r in res.items():
        print(f"kv_append   {name:14s} B{B} H{H} C{C} Tn1: "
              f"{statistics.median(r):9.1f} us (min {min(r):.1f} max {max(r):.1f})",
              flush=True)
    del caches


def bench_paged(B, H, C, kv_len, page_sizes=(16, 64, 128)):
    """attn_decode_paged (pages in order, pages scrambled; every page size)
    against attn_decode_slots with the identity map, all alternating over
    rings of the same byte size; then the same for kv_append at Tn = 1."""
    nbytes = 2 * B * H * kv_len * C * 2
    ring = max(1, min(32, -(-RING_BYTES // nbytes)))
    q = torch.randn(B, H, 1, C, device=DEV, dtype=BF)
    lens_host = torch.full((B,), kv_len, dtype=torch.int64)
    lens_dev = lens_host.to(device=DEV, dtype=torch.int32)
    ident = torch.arange(B)
    ident_dev = ident.to(device=DEV, dtype=torch.int32)
    caches = [(torch.randn(B, H, kv_len, C, device=DEV, dtype=BF),
               torch.randn(B, H, kv_len, C, device=DEV, dtype=BF))
              for _ in range(ring)]
    iters = 200 if nbytes < (64 << 20) else 50
    paths = {"slots identity": [(lambda k=k, v=v: ops._C.attn_decode_slots(
        q, k, v, lens_dev, lens_host, ident_dev, ident, 0)) for k, v in caches]}
    qkv = torch.randn(B, 1, 3, H, C, device=DEV, dtype=BF)
    qw = torch.ones(C, device=DEV)
    sin, cos = (t.contiguous() for t in ref.rope_tables(C, kv_len, device=DEV))
    pos_host = torch.full((B,), kv_len - 1, dtype=torch.int64)
    pos_dev = pos_host.to(device=DEV, dtype=torch.int32)
    kc, vc = caches[0]
    appends = {"slots identity": [lambda: ops._C.kv_append_slots(
        qkv, qw, qw, sin, cos, kc, vc, pos_dev, pos_host, ident_dev, ident, 1e-6)]}
    for PS in page_sizes:
        MP = kv_len // PS
        P = B * MP
        pools = [(torch.randn(P, H, PS, C, device=DEV, dtype=BF),
                  torch.randn(P, H, PS, C, device=DEV, dtype=BF)) for _ in range(ring)]
        order = torch.arange(P).view(B, MP)
        mixed = torch.randperm(P, generator=torch.Generator().manual_seed(PS)).view(B, MP)
        for tag, th in (("in order", order), ("scrambled", mixed)):
            td = th.to(device=DEV, dtype=torch.int32)
            paths[f"paged PS{PS} {tag}"] = [
                (lambda k=k, v=v, td=td, th=th: ops._C.attn_decode_paged(
                    q, k, v, lens_dev, lens_host, td, th, 0)) for k, v in pools]
            kp, vp = pools[0]
            appends[f"paged PS{PS} {tag}"] = [
                lambda kp=kp, vp=vp, td=td, th=th: ops._C.kv_append_paged(
                    qkv, qw, qw, sin, cos, kp, vp, pos_dev, pos_host, td, th, 1e-6)]
    for what, group, n in (("attn_decode", paths, iters), ("kv_append  ", appends, 500)):
        res = {name: [] for name in group}
        for _ in range(3):                                # alternating
            for name, fns in group.items():
                res[name].append(time_ring(fns, n) * 1e6)
        base = statistics.median(res["slots identity"])
        for name, r in res.items():
            print(f"{what} {name:22s} B{B} H{H} C{C} kv{kv_len}: "
                  f"{statistics.median(r):9.1f} us (min {min(r):.1f} max {max(r):.1f})  "
                  f"{statistics.median(r)/base:5.3f}x slots", flush=True)
    del caches, paths, appends


def bench_continuous_paged(reps, page_size, n_req=32, num_slots=8, seats=(8, 16, 32)):
    from midgpt_amd.generate import DecodeScheduler
    model, cfg = xl_model()
    lens = [16, 48, 96, 160, 240, 320, 416, 512]
    budgets = [16, 64, 128, 256]
    g = torch.Generator().manual_seed(0)
    reqs = [(torch.randint(0, cfg.vocab_size, (lens[i % 8],), generator=g).to(DEV),
             budgets[i % 4]) for i in range(n_req)]
    asked = sum(n for _, n in reqs)
    num_pages = num_slots * cfg.block_size // page_size
    print(f"continuous paged: openwebtext_xl, {n_req} requests, prompts cycling {lens}, "
          f"budgets cycling {budgets} ({asked} tokens requested), greedy; unpaged with "
          f"{num_slots} slots against {num_pages} pages of {page_size} (the same bytes) "
          f"with {list(seats)} seats; time includes the prompts", flush=True)

    def run(rs, n, **pages):
        sched = DecodeScheduler(model, n, **pages)
        hs = [sched.submit(p, m, temperature=0.0) for p, m in rs]
        sched.run()
        assert [h.tokens.numel() for h in hs] == [p.numel() + m for p, m in rs]
        return [h.tokens for h in hs]

    paths = {f"unpaged {num_slots} slots": lambda rs: run(rs, num_slots)}
    for n in seats:
        paths[f"paged PS{page_size} {n} seats"] = \
            lambda rs, n=n: run(rs, n, num_pages=num_pages, page_size=page_size)
    warm = [(p, 8) for p, _ in reqs[:2 * num_slots]]
    for fn in paths.values():                             # warm up all
        fn(warm)
    res = {name: [] for name in paths}
    texts = {}
    for _ in range(reps):                                 # alternating
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            texts[name] = fn(reqs)
            torch.cuda.synchronize()
            res[name].append(time.perf_counter() - t0)
    base_name = f"unpaged {num_slots} slots"
    base = statistics.median(res[base_name])
    for name, ts in res.items():
        tps = sorted(asked / t for t in ts)
        same = sum(torch.equal(a, b) for a, b in zip(texts[name], texts[base_name]))
        print(f"continuous {name:24s}: tokens/s median {statistics.median(tps):8.1f} "
              f"min {tps[0]:8.1f} max {tps[-1]:8.1f}  (wall median "
              f"{statistics.median(ts)*1e3:8.1f} ms) over {reps} runs, "
              f"{base/statistics.median(ts):.2f}x unpaged, {same}/{n_req} texts equal "
              "to unpaged", flush=True)


def bench_continuous(reps, n_req=32, num_slots=8):
    from midgpt_amd.generate import DecodeScheduler, generate_ragged
    model, cfg = xl_model()
    lens = [16, 48, 96, 160, 240, 320, 416, 512]
    budgets = [16, 64, 128, 256]
    g = torch.Generator().manual_seed(0)
    reqs = [(torch.randint(0, cfg.vocab_size, (lens[i % 8],), generator=g).to(DEV),
             budgets[i % 4]) for i in range(n_req)]
    asked = sum(n for _, n in reqs)
    print(f"continuous: openwebtext_xl, {n_req} requests, prompts cycling {lens}, budgets "
          f"cycling {budgets} ({asked} tokens requested), greedy, {num_slots} slots; time "
          "includes the prompts", flush=True)

    def continuous(rs):
        sched = DecodeScheduler(model, num_slots)
        hs = [sched.submit(p, n, temperature=0.0) for p, n in rs]
        sched.run()
        assert [h.tokens.numel() for h in hs] == [p.numel() + n for p, n in rs]

    def ragged_batches(rs):
        for i in range(0, len(rs), num_slots):
            batch = rs[i:i + num_slots]
            outs = generate_ragged(model, [p for p, _ in batch], max(n for _, n in batch),
                                   temperature=0.0)
            outs = [o[:p.numel() + n] for o, (p, n) in zip(outs, batch)]
            assert [o.numel() for o in outs] == [p.numel() + n for p, n in batch]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(reqs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    paths = {"DecodeScheduler 8 slots": continuous, "generate_ragged 4 x B=8": ragged_batches}
    warm = [(p, 8) for p, _ in reqs[:2 * num_slots]]
    for fn in paths.values():                             # warm up both
        fn(warm)
    res = {name: [] for name in paths}
    for _ in range(reps):                                 # alternating
        for name, fn in paths.items():
            res[name].append(timed(fn))
    for name, ts in res.items():
        tps = sorted(asked / t for t in ts)
        print(f"continuous {name:24s}: tokens/s median {statistics.median(tps):8.1f} "
              f"min {tps[0]:8.1f} max {tps[-1]:8.1f}  (wall median "
              f"{statistics.median(ts)*1e3:8.1f} ms) over {reps} runs", flush=True)
    a, b = (statistics.median(res[k]) for k in res)
    print(f"continuous speed ratio of medians (scheduler over ragged batches): {b/a:.2f}x",
          flush=True)


def bench_sample_kernel(B, V, top_k):
    from midgpt_amd.generate import _sample
    ring = [(4.0 * torch.randn(B, V, device=DEV)).to(BF) for _ in range(4)]
    gen = torch.Generator(device="cpu").manual_seed(0)
    step = [0]

    def seeded(lg):
        step[0] += 1
        return ops.sample_tokens(lg, 0.8, top_k, seed=1, step=step[0])

    paths = {
        "sample_tokens (seed=)": [(lambda lg=lg: seeded(lg)) for lg in ring],
        "_sample device multinomial": [(lambda lg=lg: _sample(lg, 0.8, top_k, None))
                                       for lg in ring],
        "_sample CPU generator": [(lambda lg=lg: _sample(lg, 0.8, top_k, gen))
                                  for lg in ring],
    }
    res = {name: [] for name in paths}
    for _ in range(3):                                    # alternating
        for name, fns in paths.items():
            res[name].append(time_ring(fns, 200) * 1e6)
    for name, r in res.items():
        print(f"sampling B{B} V{V} top_k {top_k}: {name:27s} "
              f"{statistics.median(r):9.1f} us (min {min(r):.1f} max {max(r):.1f})",
              flush=True)


def bench_sample_e2e(reps, n_new=128):
    from midgpt_amd.generate import generate_ragged
    model, cfg = xl_model()
    lens = [16, 48, 96, 160, 240, 320, 416, 512]
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).to(DEV) for n in lens]
    print(f"sampling e2e: openwebtext_xl, generate_ragged, prompts {lens}, {n_new} new "
          "tokens each; time includes the prompts", flush=True)
    paths = {
        "T=0.8 top_k=50 seed=": lambda n: generate_ragged(
            model, prompts, n, temperature=0.8, top_k=50, seed=1),
        "T=0.8 top_k=50 CPU generator": lambda n: generate_ragged(
            model, prompts, n, temperature=0.8, top_k=50,
            generator=torch.Generator(device="cpu").manual_seed(1)),
        "greedy": lambda n: generate_ragged(model, prompts, n, temperature=0.0),
    }

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = fn(n_new)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert [o.numel() for o in outs] == [m + n_new for m in lens]
        return dt

    for fn in paths.values():                             # warm up all
        fn(8)
    res = {name: [] for name in paths}
    for _ in range(reps):                                 # alternating
        for name, fn in paths.items():
            res[name].append(timed(fn))
    for name, ts in res.items():
        tps = sorted(len(lens) * n_new / t for t in ts)
        print(f"sampling e2e {name:29s}: tokens/s median {statistics.median(tps):8.1f} "
              f"min {tps[0]:8.1f} max {tps[-1]:8.1f}  (wall median "
              f"{statistics.median(ts)*1e3:8.1f} ms) over {reps} runs", flush=True)


def xl_model():
    from midgpt_amd.config import load_config
    from midgpt_amd.models.gpt import GPT
    cfg = load_config("openwebtext_xl").model_config
    torch.manual_seed(0)
    with torch.device(DEV):
        model = GPT(cfg)
    model = model.to(BF).eval()
    model.rope_sin = model.rope_sin.float()
    model.rope_cos = model.rope_cos.float()
    return model, cfg


def timed_generate(model, idx, n_new, eager):
    from midgpt_amd.generate import generate
    if eager:
        os.environ["MIDGPT_DECODE_REF"] = "1"
    else:
        os.environ.pop("MIDGPT_DECODE_REF", None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = generate(model, idx, n_new, temperature=0.0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    os.environ.pop("MIDGPT_DECODE_REF", None)
    assert out.shape == (idx.shape[0], idx.shape[1] + n_new)
    return dt


def bench_e2e(reps, n_prompt=128, n_new=256):
    model, cfg = xl_model()
    print(f"e2e generate: openwebtext_xl ({cfg.n_layer} layers, {cfg.n_head} heads, "
          f"head dim {cfg.head_dim}), prompt {n_prompt}, {n_new} new tokens, greedy; "
          "time includes the prompt", flush=True)
    for B in (1, 8):
        idx = torch.randint(0, cfg.vocab_size, (B, n_prompt), device=DEV)
        for eager in (False, True):                       # warm up both paths
            timed_generate(model, idx, 16, eager)
        res = {False: [], True: []}
        for _ in range(reps):
            for eager in (False, True):                   # alternating
                res[eager].append(timed_generate(model, idx, n_new, eager))
        for eager, name in ((False, "native"), (True, "eager (MIDGPT_DECODE_REF=1)")):
            tps = sorted(B * n_new / t for t in res[eager])
            print(f"e2e B{B} {name:28s}: tokens/s median {statistics.median(tps):8.1f} "
                  f"min {tps[0]:8.1f} max {tps[-1]:8.1f}  "
                  f"({statistics.median(res[eager])*1e3/n_new:6.2f} ms/step) over {reps} runs",
                  flush=True)
        med = {e: statistics.median(res[e]) for e in res}
        print(f"e2e B{B} native/eager speed ratio (median): {med[True]/med[False]:.2f}x",
              flush=True)


def run_count(n_new, sampled):
    model, cfg = xl_model()
    idx = torch.randint(0, cfg.vocab_size, (1, 128), device=DEV)
    from midgpt_amd.generate import generate, native_decode
    print(f"count: native={native_decode(model)} new={n_new} sampled={sampled}", flush=True)
    if sampled:
        generate(model, idx, n_new, temperature=0.8, top_k=50, seed=1)
    else:
        generate(model, idx, n_new, temperature=0.0)
    torch.cuda.synchronize()


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--which", default="all", choices=["all", "kernels", "ragged", "e2e", "count", "sampling", "slots",
                            "continuous", "paged"])
    p.add_argument("--sweep", action="store_true")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--new", type=int, default=32)
    p.add_argument("--sampled", action="store_true")
    p.add_argument("--pages", action="store_true",
                   help="with --which continuous: the paged scheduler against the unpaged")
    p.add_argument("--page_size", type=int, default=16)
    args = p.parse_args()
    if args.which in ("all", "kernels"):
        for B in (1, 8, 64):
            for kv in (128, 1024):
                bench_attn_decode(B, 16, 128, kv, args.sweep)
        for B in (1, 8, 64):
            bench_attn_decode(B, 32, 128, 4096, args.sweep)   # 7B shape
        for B in (1, 8, 64):
            bench_kv_append(B)
        for B in (8, 64):
            for kv in (128, 1024):
                bench_ragged_equal(B, 16, 128, kv)
            bench_ragged_equal(B, 32, 128, 4096)
        skew = [128, 256, 512, 768, 1024, 2048, 3072, 4096]
        bench_ragged_skewed(8, 16, 128, skew, args.sweep)
        bench_ragged_skewed(8, 32, 128, skew, args.sweep)
    if args.which in ("all", "ragged"):
        bench_ragged_e2e(max(3, args.reps))
    if args.which in ("all", "e2e"):
        bench_e2e(max(3, args.reps))
    if args.which in ("all", "sampling"):
        for B in (1, 8, 64):
            for top_k in (None, 50):
                bench_sample_kernel(B, 50304, top_k)
        bench_sample_e2e(max(3, args.reps))
    if args.which in ("all", "slots"):
        for B in (8, 64):
            for kv in (128, 1024):
                bench_slots(B, 16, 128, kv)
            bench_slots(B, 32, 128, 4096)
    if args.which == "continuous" and args.pages:
        bench_continuous_paged(max(3, args.reps), args.page_size)
    elif args.which in ("all", "continuous"):
        bench_continuous(max(3, args.reps))
    if args.which in ("all", "paged"):
        for B in (8, 64):
            for kv in (128, 1024):
                bench_paged(B, 16, 128, kv)
            bench_paged(B, 32, 128, 4096)
    if args.which == "count":
        run_count(args.new, args.sampled)
