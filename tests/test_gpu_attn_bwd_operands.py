"""Attention backward with its loop-invariant operands resident in LDS, the
key in the dq kernel's registers (LSE and delta per lane), the transposed
images in accumulator order and the delta kernel's several rows per wave.

Every bound is kernel_edge_util's FACTOR x the fp32 yardstick at the same
inputs. What is here and not in test_gpu_kernel_edges.py:

- the shortest tile loops (T=128: 4 waves, one workgroup per head; T=256: 8
  waves, one workgroup) and B*H = 6 with two blocks, both head dims, with and
  without dropout;
- constructed rows that differ within one 32-row strip (LSE, delta per lane);
- two backward calls on the same inputs, bit for bit (a missing barrier around
  the resident LDS operands would show here or in the row figures);
- delta and the packed dO copy on their own (ops._C.attn_delta), in both
  visiting orders, with row counts that do and do not fill the last block.

That the packed entry point ((B,T,H,C) dO, V and dV inside the projection)
gives dq, dk, dv bit for bit equal to the (B,H,T,C) one is asserted by
test_gpu_glue_fusion.py::test_packed_attention_equals_contiguous at T=128..512,
both head dims, with and without dropout, and is not repeated."""
import pytest
import torch

import kernel_edge_util as U

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from midgpt_amd import ops
    from midgpt_amd.ops import reference as ref
    assert ops.have_ext(), f"HIP extension must be built: {ops._C_ERR}"

DEV = "cuda:0"
BF = torch.bfloat16
P, SEED = 0.25, 7
_KEEP = {}


def randbf(*shape):
    return torch.randn(*shape, device=DEV).to(BF)


def mirror(B, H, T):
    """Host-mirror dropout mask on the device, once per shape, never mutated."""
    key = (B, H, T)
    if key not in _KEEP:
        _KEEP[key] = ref.attn_dropout_keep(SEED, B, H, T, P).to(DEV)
    return _KEEP[key]


def backward(q, k, v, do, drop):
    if drop:
        o, lse = ops._C.attn_fwd_dropout(q, k, v, P, SEED)
        dq, dk, dv = ops._C.attn_bwd_dropout(do, q, k, v, o, lse, P, SEED)
    else:
        o, lse = ops._C.attn_fwd(q, k, v)
        dq, dk, dv = ops._C.attn_bwd(do, q, k, v, o, lse)
    return {"dq": dq, "dk": dk, "dv": dv}


BWD = ("dq", "dk", "dv")


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "p0.25"])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("B,H,T", [(1, 2, 128), (1, 2, 256), (2, 3, 512)])
def test_shortest_loops_and_odd_batch(B, H, T, C, drop):
    """T=128: 4 tiles at most, the prefetch pipeline's shortest trip count.
    T=256: the 8-wave kernels with one block. (2,3,512): two blocks."""
    torch.manual_seed(T + C)
    q, k, v, do = (randbf(B, H, T, C) for _ in range(4))
    got = backward(q, k, v, do, drop)
    keep = mirror(B, H, T) if drop else None
    U.check(f"attn operands {'p0.25' if drop else 'nodrop'} B{B} H{H} T{T} C{C}",
            U.attn_figures(q, k, v, do, got, keep, P if drop else 0.0, BWD))


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("case", ["growing", "lastA"])
def test_rows_that_differ_within_a_strip(case, C):
    """growing: LSE rises by about 2 per 32-key tile, so the 32 rows of a
    strip have 32 different LSE and delta. lastA: rows before and after key
    T-40 sit in one strip with LSE some 7 apart."""
    B, H, T = 1, 2, 256
    q, k, v, do = U.attn_softmax_path_inputs(case, B, H, T, C, DEV)
    print(f"EDGE attn operands {case} C{C}: {U.attn_check_path(case, q, k)}")
    got = backward(q, k, v, do, False)
    U.check(f"attn operands {case} B{B} H{H} T{T} C{C}",
            U.attn_figures(q, k, v, do, got, names=BWD))


@pytest.mark.parametrize("B,H,T,C", [(2, 3, 512, 128), (1, 2, 128, 64)])
def test_backward_repeats_bit_for_bit(B, H, T, C):
    torch.manual_seed(T)
    q, k, v, do = (randbf(B, H, T, C) for _ in range(4))
    first = backward(q, k, v, do, False)
    again = backward(q, k, v, do, False)
    for n in BWD:
        assert torch.equal(first[n], again[n]), n


# Rows per 4-wave block: 32 at C=64, 16 at C=128. The first two shapes fill
# their last block; 15 rows leave the second half of one wave's row groups
# idle, 129 = 8 blocks + 1 row.
@pytest.mark.parametrize("bthc", [False, True], ids=["bhtc", "bthc"])
@pytest.mark.parametrize("B,H,T,C", [(1, 3, 128, 64), (2, 2, 256, 128),
                                     (1, 3, 5, 64), (1, 3, 43, 128)])
def test_delta_rows_per_wave(B, H, T, C, bthc):
    torch.manual_seed(C + T)
    shape = (B, T, H, C) if bthc else (B, H, T, C)
    do, o = randbf(*shape), randbf(*shape)
    out = ops._C.attn_delta(do, o, bthc)
    bhtc = (lambda t: t.transpose(1, 2)) if bthc else (lambda t: t)
    want64 = bhtc((do.double() * o.double()).sum(-1))
    yard = bhtc((do.float() * o.float()).sum(-1))
    assert out[0].shape == (B, H, T)
    U.check(f"attn delta {'bthc' if bthc else 'bhtc'} B{B} H{H} T{T} C{C}",
            [U.fig_stat("attn.delta", out[0], yard, want64)])
    if bthc:
        assert torch.equal(out[1], do.transpose(1, 2).contiguous()), "do_copy"
