"""Child process of test_env_gated_variants_meet_the_default_bounds.

The MIDGPT_ATTN_DKV_NW4 switch is read once into a static by the bindings,
so the test starts this script afresh with it set. It runs the attention,
embedding-bwd and gelu checks of test_gpu_kernel_edges.py and prints one JSON
line: {"env": [switches set], "lines": [figures], "over": [figures over their
bound]}. The bounds are those of the default path.

What the attention part covers: T=512, C=64 and 128, no dropout, one seed.
With the switch set the backward is attn_bwd_dkv_kernel<C,4,false> and
attn_bwd_dq_kernel<C,4,1,false> at a T where the default path takes 8 waves;
the forward stays the default 8-wave one. The 8-wave backward, the dropout
kernels and every exact property of the default path are checked in the main
process (test_attention_rows and the *_exact / *_at_8_waves tests), not here."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import kernel_edge_util as U  # noqa: E402
from midgpt_amd import ops  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16


def randbf(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(BF)


def main():
    assert torch.cuda.is_available() and ops.have_ext(), ops._C_ERR
    figs = []

    def add(tag, fs):
        figs.extend(U.Figure(f"{tag} {f.name}", f.kernel, f.yard, f.bound) for f in fs)

    for (B, H, T, C) in [(1, 2, 512, 64), (1, 2, 512, 128)]:
        torch.manual_seed(4)
        q, k, v, do = (randbf(B, H, T, C) for _ in range(4))
        o, lse = ops._C.attn_fwd(q, k, v)
        dq, dk, dv = ops._C.attn_bwd(do, q, k, v, o, lse)
        got = {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
        add(f"attn B{B} H{H} T{T} C{C}", U.attn_figures(q, k, v, do, got))

    torch.manual_seed(8)
    for (N, V, D) in [(1021, 97, 64), (4100, 97, 8)]:
        idx = torch.randint(0, V, (N,), device=DEV)
        idx[idx == V // 2] = V // 2 + 1
        idx[:5] = 0
        idx[5:9] = V - 1
        dy = randbf(N, D)
        dw = ops._C.embedding_bwd(dy, idx, V)
        add(f"embed N{N} V{V} D{D}", U.embedding_figures(dy, idx, V, dw))

    torch.manual_seed(10)
    x = U.gelu_all_inputs(DEV)
    dy = randbf(x.numel())
    add("gelu exhaustive", U.gelu_figures(x, dy, ops._C.gelu_fwd(x), ops._C.gelu_bwd(dy, x)))

    torch.cuda.synchronize()
    env = sorted(k for k in os.environ
                 if k.startswith(("MIDGPT_ATTN_", "MIDGPT_EMBED_", "MIDGPT_GELU_")))
    print(json.dumps({"env": env, "lines": [str(f) for f in figs],
                      "over": [str(f) for f in figs if not f.ok]}))


if __name__ == "__main__":
    main()
