"""torchrun worker of tests/test_multigpu_dgrad_wt.py: 2 ranks, ZeRO over
RCCL, the bf16 HIP path. After construction and after each of two steps every
``Linear.weight_t`` must equal ``weight.t()`` on this rank. Exit code 0 and a
DGRAD-WT-ZERO-OK line per rank = pass."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from midgpt_amd.config import GPTConfig  # noqa: E402
from midgpt_amd.models.gpt import GPT, Linear  # noqa: E402
from midgpt_amd.parallel import dist as pdist  # noqa: E402
from midgpt_amd.parallel.engine import ShardedAdamW  # noqa: E402

TINY = GPTConfig(block_size=128, vocab_size=65, n_layer=2, n_head=1,
                 n_embd=64, dropout=0.0)


def check(model, when):
    mods = [m for m in model.modules() if isinstance(m, Linear)]
    assert len(mods) == 4 * TINY.n_layer + 1
    for m in mods:
        assert m.weight_t is not None, when
        assert torch.equal(m.weight_t, m.weight.t()), (when, tuple(m.weight.shape))


def main():
    rank, world, device = pdist.init_distributed()
    assert world == 2, "run under torchrun with 2 processes"
    torch.manual_seed(0)
    model = GPT(TINY).to(device)
    engine = ShardedAdamW(model, compute_dtype=torch.bfloat16, zero=True,
                          device=device)
    assert engine.zero and engine.flat_wt is not None
    check(model, "construction")
    g = torch.Generator().manual_seed(42)
    x = torch.randint(0, 65, (2, 4, 128), generator=g)[rank].to(device)
    y = torch.randint(0, 65, (2, 4, 128), generator=g)[rank].to(device)
    for s in range(2):
        before = engine.flat_w.clone()
        model.loss(x, y).backward()
        engine.microstep_end()
        engine.step(5e-3)
        assert not torch.equal(before, engine.flat_w)
        check(model, f"step {s}")
    torch.cuda.synchronize()
    print(f"DGRAD-WT-ZERO-OK rank={rank}")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
