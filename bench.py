"""Benchmark harness — the driver contract.

``python bench.py --gpus N --steps K --warmup W`` runs the flagship
training step (openwebtext_xl 1.5B GPT, bf16, synthetic data, random
init — BASELINE.json headline) on N GPUs of one node, one rank per GPU
over RCCL, and prints ONE JSON line from rank 0.

Weak scaling: per-GPU work is fixed at 128 seq x 1024 tok = 131072
tokens/GPU/step, so N=8 reproduces the reference's global batch 1024
(reference src/configs/openwebtext_xl.py; BASELINE.md 444K tok/s).

A plain run sets up, warms up, times ``--steps`` steps and prints the
result line; nothing else is measured. ``--dump-outputs DIR`` also writes
what the last timed step computed (see ``_dump_outputs``) so two builds
can be compared output for output. ``--full`` is reserved for secondary
measurements; this benchmark has none today, so it changes nothing.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np
import torch

from midgpt_amd.config import load_config
from midgpt_amd.data import synthetic_batch
from midgpt_amd.parallel import dist as pdist
from midgpt_amd.train import build_engine
from midgpt_amd.utils.lr import warmup_cosine_lr


def _self_launch(n: int):
    """Re-exec under torch.distributed.run with one rank per GPU.

    The driver may invoke ``python bench.py --gpus 8`` directly; without
    this, WORLD_SIZE is unset and the run would silently measure 1 GPU.
    """
    import subprocess
    import sys
    cmd = [sys.executable, "-m", "torch.distributed.run",
           "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr=127.0.0.1", "--master-port=29771",
           sys.argv[0], *sys.argv[1:]]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    raise SystemExit(subprocess.call(cmd))


# weights written by --dump-outputs: a fixed seeded sample, 16 MB as fp32
_DUMP_SAMPLE = 1 << 22


def _dump_outputs(outdir: str, losses, sq, engine):
    """Write the last timed step's results as float32 ``<name>.npy``:

    loss          (g_accum,) the loss each microbatch's forward returned
    grad_sq_sum   (1,) what ``engine.step`` returned (pre-clip sum of squares)
    weights       the working weights the step left behind, all of them if
                  they fit in the sample size, else a seeded sample in flat
                  parameter order
    """
    os.makedirs(outdir, exist_ok=True)
    flat = engine.flat_w[:engine.total]
    if engine.total > _DUMP_SAMPLE:
        g = torch.Generator().manual_seed(4321)
        idx = torch.randint(0, engine.total, (_DUMP_SAMPLE,), generator=g)
        flat = flat[idx.sort().values.to(flat.device)]
    out = {
        "loss": torch.stack([l.detach().float().reshape(()) for l in losses]),
        "grad_sq_sum": sq.detach().float().reshape(1),
        "weights": flat.detach().float(),
    }
    for name, t in out.items():
        np.save(os.path.join(outdir, name + ".npy"), t.cpu().numpy())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--config", default="openwebtext_xl")
    p.add_argument("--local-batch", type=int, default=128,
                   help="sequences per GPU per optimizer step")
    p.add_argument("--micro-batch", type=int, default=None,
                   help="microbatch size (default: the whole local batch "
                        "for <=1024-dim models, 64 for larger at T<=1024, "
                        "4 at long seq — all measured optima; 7B@4096 "
                        "no-remat micro=4 fits 224 GB)")
    p.add_argument("--remat", action="store_true",
                   help="per-block activation recompute (default OFF: 288 GB "
                        "HBM fits stored activations at the default "
                        "microbatch for every config incl. 7B@4096)")
    p.add_argument("--no-remat", action="store_true",
                   help="force remat OFF even at seq > 1024 (memory permitting)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last one "
                        "computed as DIR/<name>.npy (rank 0)")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements (none today)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")

    if args.gpus > 1 and int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        _self_launch(args.gpus)  # re-exec under torchrun; does not return

    rank, world, device = pdist.init_distributed()
    assert world == args.gpus, f"WORLD_SIZE={world} != --gpus {args.gpus}"
    n = max(world, 1)

    config = load_config(args.config)
    config.synthetic_data = True
    config.rundir = ""
    config.remat = args.remat and not args.no_remat
    mc = config.model_config
    # micro default: whole local batch for small models (124M at micro
    # 128/g1 measured +1% over 64/g2); 64 for >=1.5B at T<=1024 (memory
    # headroom for the 8-GPU run); 4 for long-seq (7B@4096 fits 224 GB)
    micro = args.micro_batch or min(
        args.local_batch,
        (args.local_batch if mc.n_embd <= 1024 else 64)
        if mc.block_size <= 1024 else 4)
    assert args.local_batch % micro == 0
    g_accum = args.local_batch // micro
    config.batch_size = micro * n
    config.g_accum_iters = g_accum
    # ZeRO sharding active whenever world > 1 (headline config shard_model=True)

    # identical seed for model init on EVERY rank (data-parallel replicas
    # must start from the same weights); per-rank seed afterwards for data
    torch.manual_seed(1234)
    model, engine = build_engine(config, device)
    torch.manual_seed(1234 + rank)
    tokens_per_step_per_gpu = args.local_batch * mc.block_size

    # pre-generate a couple of synthetic batches on device (data pipeline is
    # not the measured quantity; the reference benches with real data cached
    # in RAM — synthetic per the driver contract, no network)
    batches = []
    for i in range(2):
        x, y = synthetic_batch(mc.vocab_size, mc.block_size, micro, g_accum,
                               device=device)
        batches.append((x, y))

    def one_step(it):
        lr = warmup_cosine_lr(it, peak_lr=config.learning_rate,
                              warmup_steps=config.warmup_steps,
                              decay_steps=config.lr_decay_steps,
                              min_lr=config.min_lr)
        x, y = batches[it % len(batches)]
        losses = []
        for g in range(g_accum):
            loss = model.loss(x[g], y[g])
            loss.backward()
            engine.microstep_end()
            losses.append(loss)
        sq = engine.step(lr, g_accum)
        return losses, sq

    for w in range(args.warmup):
        one_step(w)

    pdist.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(args.steps):
        losses, sq = one_step(args.warmup + it)
    pdist.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    loss = losses[-1]

    if args.dump_outputs and rank == 0:
        _dump_outputs(args.dump_outputs, losses, sq, engine)

    # MAX over ranks
    t = torch.tensor([elapsed], dtype=torch.float64)
    if world > 1:
        import torch.distributed as dist
        td = t.to(device) if device.type == "cuda" else t
        dist.all_reduce(td, op=dist.ReduceOp.MAX)
        elapsed = float(td[0])

    ms_per_step = elapsed / args.steps * 1000.0
    tokens_per_sec = n * tokens_per_step_per_gpu * args.steps / elapsed
    # model FLOPs/token = 6*(matmul params incl. the UNTIED lm_head, which
    # is compute-bearing even though count_params excludes it for reference
    # parity) + 12*L*D*T attention term; MFU vs 2.5 PF dense bf16 per GPU.
    from midgpt_amd.models.gpt import count_params
    n_params = count_params(model)
    n_matmul = n_params + model.lm_head.weight.numel()
    flops_per_token = 6 * n_matmul + 12 * mc.n_layer * mc.n_embd * mc.block_size
    mfu = tokens_per_sec * flops_per_token / (n * 2.5e15)

    if rank == 0:
        print(json.dumps({
            "metric": "tokens_per_sec",
            "value": round(tokens_per_sec, 1),
            "unit": "tokens/s",
            "n_gpus": n,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(tokens_per_sec / 444000.0, 4),
            "dtype": "bf16" if device.type == "cuda" else "fp32",
            "data": "synthetic",
            "config": {
                "model": f"{args.config}-gpt-{round(n_params/1e6)}M",
                "global_batch": args.local_batch * n,
                "seq_len": mc.block_size,
                "parallelism": (f"zero-dp{n}" if engine.zero else f"dp{n}"),
                "g_accum_iters": g_accum,
                "remat": config.remat,
                "mfu_vs_2.5pf_dense": round(mfu, 4),
                "last_loss": round(float(loss.detach()), 4),
                "max_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30,
                                    1) if device.type == "cuda" else 0,
            },
        }), flush=True)


if __name__ == "__main__":
    main()
