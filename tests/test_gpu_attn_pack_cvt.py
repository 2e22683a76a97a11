"""Attention with the packed hardware bf16 conversion in its tile loops
(mfma.h pack_bf16), the forward kernels' prefetch kept clear of waits, and
the heaviest q-block first.

- The conversion itself: ops._C.probe_bf16_pack sweeps all 2^32 fp32 bit
  patterns, in both element positions, against the software f2b. Required: no
  difference for any input that is not a NaN (signed zeros, infinities and
  denormals are among them), and a NaN for every NaN.
- Forward and full backward against the fp64 reference at the smallest shapes
  that reach each path, every bound kernel_edge_util's FACTOR x the fp32
  yardstick at the same inputs:
    paired forward (C=128, 8 waves): T=256 (1,1) is a single block whose
      rounds all touch the diagonal; T=512 (3,1) has rounds wholly below the
      diagonal, two block classes and an odd B*H; T=768 (1,2) has three
      classes, so the reversed block order is seen at an odd count;
    single-tile 8-wave forward (C=64; C=128 under dropout): T=256 and 512,
      (2,3), p = 0 and p = 0.25;
    4-wave kernels: C=64 and 128 at T=128 and 384, (1,2).
- Two calls of forward and backward on the same inputs, bit for bit."""
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
P, SEED = 0.25, 11


def randbf(*shape):
    return torch.randn(*shape, device=DEV).to(BF)


def fwd_bwd(q, k, v, do, drop):
    if drop:
        o, lse = ops._C.attn_fwd_dropout(q, k, v, P, SEED)
        dq, dk, dv = ops._C.attn_bwd_dropout(do, q, k, v, o, lse, P, SEED)
    else:
        o, lse = ops._C.attn_fwd(q, k, v)
        dq, dk, dv = ops._C.attn_bwd(do, q, k, v, o, lse)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def test_pack_equals_f2b_for_every_fp32():
    counts = torch.zeros(3, dtype=torch.int64, device=DEV)
    chunk = 1 << 28
    for start in range(0, 1 << 32, chunk):
        ops._C.probe_bf16_pack(counts, start, chunk)
    differ, nan_differ, nan_lost = (int(c) for c in counts.cpu())
    print(f"EDGE bf16 pack sweep: non-NaN inputs that differ from f2b {differ}, "
          f"NaN inputs that differ {nan_differ}, NaN inputs that give no NaN {nan_lost}")
    assert differ == 0, f"{differ} non-NaN fp32 inputs convert differently from f2b"
    assert nan_lost == 0, f"{nan_lost} NaN inputs do not give a NaN"


def test_pack_probe_counts_a_chunk_with_its_tail():
    """The probe's own counting, on the 2^24 patterns from 0x7f000000 (large
    finite values, +inf and every positive NaN): a count that is no multiple
    of the block is swept to its end and no further, so a sweep split at an
    odd place gives the sums of the whole."""
    whole = torch.zeros(3, dtype=torch.int64, device=DEV)
    ops._C.probe_bf16_pack(whole, 0x7f000000, 1 << 24)
    parts = torch.zeros(3, dtype=torch.int64, device=DEV)
    ops._C.probe_bf16_pack(parts, 0x7f000000, 12345)
    ops._C.probe_bf16_pack(parts, 0x7f000000 + 12345, (1 << 24) - 12345)
    assert torch.equal(whole, parts), (whole, parts)
    assert int(whole[0]) == 0 and int(whole[2]) == 0, whole


def check(tag, B, H, T, C, drop):
    torch.manual_seed(T + C + B)
    q, k, v, do = (randbf(B, H, T, C) for _ in range(4))
    got = fwd_bwd(q, k, v, do, drop)
    keep = ref.attn_dropout_keep(SEED, B, H, T, P).to(DEV) if drop else None
    U.check(f"attn pack_cvt {tag} {'p0.25' if drop else 'nodrop'} B{B} H{H} T{T} C{C}",
            U.attn_figures(q, k, v, do, got, keep, P if drop else 0.0))


@pytest.mark.parametrize("B,H,T", [(1, 1, 256), (3, 1, 512), (1, 2, 768)])
def test_paired_forward(B, H, T):
    check("paired", B, H, T, 128, False)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "p0.25"])
@pytest.mark.parametrize("T", [256, 512])
def test_single_tile_8wave_forward(T, drop):
    check("single8", 2, 3, T, 64, drop)


def test_single_tile_8wave_forward_c128_dropout():
    check("single8", 2, 3, 512, 128, True)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("T", [128, 384])
def test_4wave_kernels(T, C):
    check("4wave", 1, 2, T, C, False)


def test_forward_backward_repeat_bit_for_bit():
    torch.manual_seed(512)
    q, k, v, do = (randbf(3, 1, 512, 128) for _ in range(4))
    first = fwd_bwd(q, k, v, do, False)
    again = fwd_bwd(q, k, v, do, False)
    for n, t in first.items():
        assert torch.equal(t, again[n]), n
