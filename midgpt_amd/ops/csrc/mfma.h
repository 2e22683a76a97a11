// MFMA fragment-layout helpers for v_mfma_f32_32x32x16_bf16 (gfx950).
//
// Layouts (verified on hardware by tests/test_gpu_kernels.py::
// test_mfma_layout_probe and ::test_mfma_pack_probe):
//   D/C: lane l, reg r  ->  row = (r&3) + 8*(r>>2) + 4*(l>>5), col = l&31
//   A  : lane l, j      ->  A[row = l&31][k = 8*(l>>5) + j],  j = 0..7
//   B  : lane l, j      ->  B[k = 8*(l>>5) + j][col = l&31]
// (guide cdna_hip_programming.md section 3; A/B extrapolated from the CDNA
//  32x32x8 pattern with K doubled — the probe test guards this assumption.)
#pragma once
#include "common.h"

using bf16x8_t = __attribute__((ext_vector_type(8))) __bf16;

DEVINL f32x16 mfma_32x32x16_bf16(bf16x8_t a, bf16x8_t b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

DEVINL int mfma_d_row(int lane, int r) {
  return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}

// pack two f32 into one dword of two bf16 (lo = first): the vector conversion
// compiles to one v_cvt_pk_bf16_f32. Bit for bit f2b for every input that is
// not a NaN, and a NaN for every NaN (probe_bf16_pack sweeps all 2^32).
using bf16x2_t = __attribute__((ext_vector_type(2))) __bf16;
DEVINL unsigned pack_bf16(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}

// Position of row i (0..31) of a k axis in an image that an accumulator tile
// reads as the other operand of its next MFMA: bits 2 and 3 exchanged (an
// involution). Element j of lane half h of a 16-byte read at positions
// 16s + 8h + j is then row 16s + 8(j>>2) + 4h + (j&3), which is what
// dlayout_pack puts into element j of that half.
DEVINL int acc_k_pos(int i) {
  return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1);
}

// 8 f32 D-layout registers (regs 8s..8s+7 of a 32x32 accumulator X) packed
// pairwise into the bf16x8 fragment of k-step s of a product that sums over
// X's row index (X^T·B as the A operand, A·X as the B operand): no lane
// movement. The k order inside the step is permuted, see acc_k_pos. keep8:
// bit i clear zeroes s[i] (applied to the packed pairs).
DEVINL bf16x8_t dlayout_pack(const float* s /*8 vals*/, unsigned keep8 = 0xffu) {
  union { unsigned u[4]; bf16x8_t v; } out;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned mk = (((keep8 >> (2 * i)) & 1u) ? 0x0000ffffu : 0u) |
                        (((keep8 >> (2 * i + 1)) & 1u) ? 0xffff0000u : 0u);
    out.u[i] = pack_bf16(s[2 * i], s[2 * i + 1]) & mk;
  }
  return out.v;
}

// Convert 8 f32 D-layout registers (regs rb..rb+7 of a 32x32 accumulator,
// holding rows {0..3, 8..11} + 4*(lane>>5) of some logical axis) into ONE
// bf16x8 A-fragment covering rows 0..15 of that axis (k-chunk), using
// v_permlane32_swap half exchanges (guide T12/T21 pattern).
DEVINL bf16x8_t dlayout_to_afrag(const float* s /*8 vals*/) {
  unsigned x0 = pack_bf16(s[0], s[1]);
  unsigned x1 = pack_bf16(s[2], s[3]);
  unsigned x2 = pack_bf16(s[4], s[5]);
  unsigned x3 = pack_bf16(s[6], s[7]);
  {
    auto r = __builtin_amdgcn_permlane32_swap(x0, x2, false, false);
    x0 = r[0]; x2 = r[1];
  }
  {
    auto r = __builtin_amdgcn_permlane32_swap(x1, x3, false, false);
    x1 = r[0]; x3 = r[1];
  }
  union { unsigned u[4]; bf16x8_t v; } out;
  out.u[0] = x0; out.u[1] = x1; out.u[2] = x2; out.u[3] = x3;
  return out.v;
}
