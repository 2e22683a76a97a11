// MFMA layout probes: verify on hardware the fragment-layout assumptions in
// mfma.h (tests/test_gpu_kernels.py::test_mfma_layout_probe and
// ::test_mfma_pack_probe). Asymmetric inputs catch transposes
// (guide section 3 "Always A=I-check with ASYMMETRIC B").
// probe_bf16_pack_kernel: mfma.h's packed conversion against common.h's f2b
// over fp32 bit patterns (tests/test_gpu_attn_pack_cvt.py sweeps all 2^32).
#include "common.h"
#include "mfma.h"

// D = A(32x16) @ B(16x32) with fragments loaded per mfma.h's layout maps.
__global__ void probe_mfma_kernel(const float* __restrict__ A,
                                  const float* __restrict__ B,
                                  float* __restrict__ D) {
  const int lane = threadIdx.x;  // 64 threads
  bf16x8_t a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    // A[row = lane&31][k = 8*(lane>>5) + j]
    a[j] = (__bf16)A[(lane & 31) * 16 + 8 * (lane >> 5) + j];
    // B[k = 8*(lane>>5) + j][col = lane&31]
    b[j] = (__bf16)B[(8 * (lane >> 5) + j) * 32 + (lane & 31)];
  }
  f32x16 d = (f32x16)(0.f);
  d = mfma_32x32x16_bf16(a, b, d);
#pragma unroll
  for (int r = 0; r < 16; ++r)
    D[mfma_d_row(lane, r) * 32 + (lane & 31)] = d[r];
}

// D = M^T @ B where M (32x32) enters via D-layout registers and is packed to
// A-fragments by dlayout_to_afrag (the fwd P->PV path). Expected: M^T @ B.
__global__ void probe_pack_kernel(const float* __restrict__ M,
                                  const float* __restrict__ B,
                                  float* __restrict__ D) {
  const int lane = threadIdx.x;
  float m[16];
#pragma unroll
  for (int r = 0; r < 16; ++r)
    m[r] = M[mfma_d_row(lane, r) * 32 + (lane & 31)];
  bf16x8_t a0 = dlayout_to_afrag(m);
  bf16x8_t a1 = dlayout_to_afrag(m + 8);
  bf16x8_t b0, b1;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    b0[j] = (__bf16)B[(8 * (lane >> 5) + j) * 32 + (lane & 31)];
    b1[j] = (__bf16)B[(16 + 8 * (lane >> 5) + j) * 32 + (lane & 31)];
  }
  f32x16 d = (f32x16)(0.f);
  d = mfma_32x32x16_bf16(a0, b0, d);
  d = mfma_32x32x16_bf16(a1, b1, d);
#pragma unroll
  for (int r = 0; r < 16; ++r)
    D[mfma_d_row(lane, r) * 32 + (lane & 31)] = d[r];
}

// pack_bf16 against f2b for the n fp32 bit patterns start, start + 1, ...
// (n <= 2^32; the pattern wraps). Pattern x is converted in both element
// positions, beside its complement ~x in the other one, and all four halves
// are compared with f2b. Added into counts:
//   [0] patterns that are no NaN with a half that differs from f2b,
//   [1] NaN patterns with a half that differs from f2b,
//   [2] NaN patterns whose conversion is not a NaN (either position).
// A pattern counts for itself only: ~x is judged when its own turn comes.
__global__ void probe_bf16_pack_kernel(uint32_t start, unsigned long long n,
                                       unsigned long long* __restrict__ counts) {
  auto bits = [](uint32_t u) { return __builtin_bit_cast(float, u); };
  auto is_nan16 = [](uint32_t h) { return (h & 0x7fffu) > 0x7f80u; };
  unsigned long long bad = 0, bad_nan = 0, lost_nan = 0;
  const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < n; i += step) {
    const uint32_t x = start + (uint32_t)i;
    const unsigned lo = pack_bf16(bits(x), bits(~x));  // x in the low half
    const unsigned hi = pack_bf16(bits(~x), bits(x));  // x in the high half
    const uint32_t want = f2b(bits(x));
    const bool same = (lo & 0xffffu) == want && (hi >> 16) == want;
    if ((x & 0x7fffffffu) > 0x7f800000u) {
      bad_nan += !same;
      lost_nan += !(is_nan16(lo & 0xffffu) && is_nan16(hi >> 16));
    } else {
      bad += !same;
    }
  }
  if (bad) atomicAdd(&counts[0], bad);
  if (bad_nan) atomicAdd(&counts[1], bad_nan);
  if (lost_nan) atomicAdd(&counts[2], lost_nan);
}
