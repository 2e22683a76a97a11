"""Microbenchmarks for the HIP hot kernels (run on the GPU box).
Prints per-kernel time and effective TF/s or TB/s."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import time

import torch

from midgpt_amd import ops
from midgpt_amd.ops import reference as ref

assert torch.cuda.is_available()
DEV = "cuda:0"


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_attn(B=32, H=16, T=1024, C=128, dropout_p=0.0):
    q = torch.randn(B, H, T, C, device=DEV, dtype=torch.bfloat16)
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    if dropout_p > 0.0:  # in-kernel Philox dropout (fixed seed)
        fwd = lambda: ops._C.attn_fwd_dropout(q, k, v, dropout_p, 1234)
        o, lse = fwd()
        do = torch.randn_like(o)
        bwd = lambda: ops._C.attn_bwd_dropout(do, q, k, v, o, lse, dropout_p, 1234)
    else:
        fwd = lambda: ops._C.attn_fwd(q, k, v)
        o, lse = fwd()
        do = torch.randn_like(o)
        bwd = lambda: ops._C.attn_bwd(do, q, k, v, o, lse)
    t_fwd = timeit(fwd)
    t_bwd = timeit(bwd)
    flops_fwd = 4 * B * H * T * T * C / 2  # causal
    flops_bwd = flops_fwd * 2.5
    tag = f" p{dropout_p}" if dropout_p > 0.0 else ""
    print(f"attn_fwd  B{B} H{H} T{T} C{C}{tag}: {t_fwd*1e3:8.3f} ms  "
          f"{flops_fwd/t_fwd/1e12:7.1f} TF/s (causal-effective)")
    print(f"attn_bwd  B{B} H{H} T{T} C{C}{tag}: {t_bwd*1e3:8.3f} ms  "
          f"{flops_bwd/t_bwd/1e12:7.1f} TF/s (causal-effective)")


def bench_gelu(N=131072, D=8192):
    x = torch.randn(N, D, device=DEV).to(torch.bfloat16)
    dy = torch.randn_like(x)
    t = timeit(lambda: ops._C.gelu_fwd(x))
    print(f"gelu_fwd N{N} D{D}: {t*1e3:8.3f} ms  {2*N*D*2/t/1e12:6.2f} TB/s")
    t = timeit(lambda: ops._C.gelu_bwd(dy, x))
    print(f"gelu_bwd N{N} D{D}: {t*1e3:8.3f} ms  {3*N*D*2/t/1e12:6.2f} TB/s")


def bench_embedding(N=131072, V=50304, D=2048):
    idx = torch.randint(0, V, (N,), device=DEV)
    dy = torch.randn(N, D, device=DEV).to(torch.bfloat16)
    t = timeit(lambda: ops._C.embedding_bwd(dy, idx, V), iters=10)
    print(f"embedding_bwd N{N} V{V} D{D}: {t*1e3:8.3f} ms")


def bench_rmsnorm(N=131072, D=2048):
    x = torch.randn(N, D, device=DEV, dtype=torch.bfloat16)
    y, invr = ops._C.rmsnorm_fwd(x, None, 1e-6)
    t = timeit(lambda: ops._C.rmsnorm_fwd(x, None, 1e-6))
    gb = 2 * N * D * 2 / 1e9
    print(f"rmsnorm_fwd N{N} D{D}: {t*1e3:8.3f} ms  {gb/t/1e3:6.2f} TB/s")
    dy = torch.randn_like(x)
    t = timeit(lambda: ops._C.rmsnorm_bwd(dy, x, None, invr, 1e-6))
    gb = 5 * N * D * 2 / 1e9
    print(f"rmsnorm_bwd N{N} D{D}: {t*1e3:8.3f} ms  {gb/t/1e3:6.2f} TB/s")


def bench_qkv_prep(B=32, T=1024, H=16, C=128):
    qkv = torch.randn(B, T, 3, H, C, device=DEV, dtype=torch.bfloat16)
    qw = torch.ones(C, device=DEV)
    kw = torch.ones(C, device=DEV)
    sin, cos = ref.rope_tables(C, T, device=DEV)
    sin, cos = sin.contiguous(), cos.contiguous()
    t = timeit(lambda: ops._C.qkv_prep_fwd(qkv, qw, kw, sin, cos, 1e-6))
    gb = 2 * B * T * 3 * H * C * 2 / 1e9
    print(f"qkv_prep_fwd: {t*1e3:8.3f} ms  {gb/t/1e3:6.2f} TB/s")


def bench_ce(N=131072, V=50304):
    logits = torch.randn(N, V, device=DEV, dtype=torch.bfloat16)
    targets = torch.randint(0, V, (N,), device=DEV)
    loss, lse = ops._C.ce_fwd(logits, targets)
    t = timeit(lambda: ops._C.ce_fwd(logits, targets), iters=5)
    gb = N * V * 2 / 1e9
    print(f"ce_fwd N{N} V{V}: {t*1e3:8.3f} ms  {gb/t/1e3:6.2f} TB/s")
    gs = torch.ones(1, device=DEV)
    t = timeit(lambda: ops._C.ce_bwd(logits, targets, lse, gs), iters=5)
    print(f"ce_bwd N{N} V{V}: {t*1e3:8.3f} ms  {2*gb/t/1e3:6.2f} TB/s")


def bench_adamw(n=1_600_000_000 // 8):
    master = torch.randn(n, device=DEV)
    grad = torch.randn(n, device=DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    out = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    sq = (grad * grad).sum()
    t = timeit(lambda: ops._C.adamw_step(master, grad, m, v, out, True, sq,
                                         1e-3, 0.9, 0.95, 1e-8, 0.1, 1.0, 1.0, 5),
               iters=5)
    gb = n * (4 * 4 + 3 * 4 + 2) / 1e9  # r: m,v,g,master; w: m,v,master; bf16
    print(f"adamw n{n}: {t*1e3:8.3f} ms  {gb/t/1e3:6.2f} TB/s")


def bench_gemm():
    for (M, K, N, tag) in [(32768, 2048, 6144, "c_attn"),
                           (32768, 2048, 8192, "c_fc"),
                           (32768, 8192, 2048, "mlp_proj"),
                           (32768, 2048, 50304, "lm_head")]:
        a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
        b = torch.randn(N, K, device=DEV, dtype=torch.bfloat16)
        t = timeit(lambda: a @ b.t(), iters=10)
        fl = 2 * M * K * N
        print(f"gemm {tag} {M}x{K}x{N}: {t*1e3:8.3f} ms  {fl/t/1e12:7.1f} TF/s")


def bench_dgrad(M=65536, rounds=5, iters=8):
    """dgrad dx = dy W as torch issues it today (NN, W stored (out, in))
    against the same product from a transposed image Wt (in, out), which is
    the forward's TN layout. The two run interleaved, round by round, in this
    one process; the figure per variant is the median round. Weighted by
    launches per microstep it predicts the step's saving."""
    shapes = [("c_attn", 2048, 6144, 24), ("attn_proj", 2048, 2048, 24),
              ("c_fc", 2048, 8192, 24), ("mlp_proj", 8192, 2048, 24),
              ("lm_head", 2048, 50304, 1)]

    def window(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    total_nn = total_tn = 0.0
    print(f"dgrad M={M}: NN (dy @ W) vs TN (dy @ Wt.t()), ms per call, "
          f"median of {rounds} interleaved rounds of {iters}")
    print("| shape | in | out | NN ms | NN TF/s | TN ms | TN TF/s | TN/NN | "
          "launches | saved ms/microstep |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for tag, n_in, n_out, launches in shapes:
        dy = torch.randn(M, n_out, device=DEV, dtype=torch.bfloat16)
        w = (torch.randn(n_out, n_in, device=DEV) / n_in ** 0.5).to(torch.bfloat16)
        wt = w.t().contiguous()
        nn_fn = lambda: torch.mm(dy, w)
        tn_fn = lambda: torch.mm(dy, wt.t())
        for _ in range(3):
            nn_fn()
            tn_fn()
        torch.cuda.synchronize()
        t_nn, t_tn = [], []
        for _ in range(rounds):
            t_nn.append(window(nn_fn))
            t_tn.append(window(tn_fn))
        a = sorted(t_nn)[rounds // 2]
        b = sorted(t_tn)[rounds // 2]
        fl = 2.0 * M * n_in * n_out
        saved = (a - b) * launches
        total_nn += a * launches
        total_tn += b * launches
        print(f"| {tag} | {n_in} | {n_out} | {a:.3f} | {fl/a/1e9:.0f} | {b:.3f} | "
              f"{fl/b/1e9:.0f} | {b/a:.3f} | {launches} | {saved:+.2f} |")
        del dy, w, wt
    print(f"weighted per microstep: NN {total_nn:.2f} ms, TN {total_tn:.2f} ms, "
          f"saved {total_nn - total_tn:+.2f} ms")


def bench_transpose(D=2048, L=24, V=50304):
    """The engine's one launch at openwebtext_xl: every Linear weight of the
    model transposed from a flat buffer into the image buffer, beside a torch
    copy_ of the same byte count (the yardstick: read + write once)."""
    shapes = [(3 * D, D), (D, D), (4 * D, D), (D, 4 * D)] * L + [(V, D)]
    entries, off = [], 0
    for r, c in shapes:
        entries.append((off, off, r, c))
        off += r * c
    src = torch.randn(off, device=DEV, dtype=torch.bfloat16)
    dst = torch.empty_like(src)
    tdev, thost = ops.transpose_table(entries, DEV)
    t = timeit(lambda: ops.transpose_batched(src, dst, tdev, thost), iters=10, warmup=3)
    tc = timeit(lambda: dst.copy_(src), iters=10, warmup=3)
    gb = 2 * off * 2 / 1e9
    print(f"transpose_batched {len(shapes)} matrices, {off/1e9:.3f}e9 elements: "
          f"{t*1e3:8.3f} ms  {gb/t/1e3:6.2f} TB/s   | copy_ {tc*1e3:8.3f} ms  "
          f"{gb/tc/1e3:6.2f} TB/s   | ratio {t/tc:.2f}")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--which", default="all")
    args = p.parse_args()
    w = args.which
    if w == "dgrad":  # a decision measurement of its own, not part of "all"
        bench_dgrad()
    if w in ("all", "transpose"):
        bench_transpose()
    if w in ("all", "attn"):
        bench_attn()
        bench_attn(B=32, H=12, T=1024, C=64)
        bench_attn(B=4, H=32, T=4096, C=128)  # 7B shape
        bench_attn(B=64, H=6, T=256, C=64)  # shakespeare_char shape
        bench_attn(B=64, H=6, T=256, C=64, dropout_p=0.2)
    if w in ("all", "gelu"):
        bench_gelu()
    if w in ("all", "embed"):
        bench_embedding()
    if w in ("all", "norm"):
        bench_rmsnorm()
        bench_qkv_prep()
    if w in ("all", "ce"):
        bench_ce()
    if w in ("all", "adamw"):
        bench_adamw()
    if w in ("all", "gemm"):
        bench_gemm()
