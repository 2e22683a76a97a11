// Stateless attention-dropout keep-mask: Philox4x32-10 (Salmon et al.,
// "Parallel Random Numbers: As Easy as 1, 2, 3", SC'11) in plain C++ —
// mulhi, mullo and xor only, so the same text compiles for the device and
// for the host. ops/reference.py:attn_dropout_keep is the bit-exact numpy
// mirror; the forward and both backward attention kernels call the
// functions below and nothing else, so the mask is defined in ONE place.
//
// Definition. For attention element (bh = b*H + h, q, k):
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (k, q >> 2, bh, 0)
//   word    = philox4x32_10(counter, key)[q & 3]
//   keep    = word >= thr,   thr = (uint32)(p * 2^32)
// i.e. the four words of one Philox call cover four consecutive q at one k.
//
// Why along q: in attn_bwd_dkv_kernel and attn_bwd_dq_kernel a lane's four
// consecutive accumulator registers are four consecutive q (4-aligned) at
// one k, so one call yields exactly the four words that lane needs. In the
// forward's swapped-QK^T layout the registers run along k at one q; there
// the four lanes of a quad (q = 4g..4g+3, same 16 k) each evaluate a
// quarter of the quad's calls and exchange the keep bits (see
// attn_fwd_kernel), which keeps the forward at one call per four elements
// too.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PHILOX_INL __host__ __device__ __forceinline__
#else
#define PHILOX_INL inline
#endif

struct PhiloxWords { uint32_t w[4]; };

PHILOX_INL PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                                     uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    // one 32x32->64 product gives mulhi (>> 32) and mullo (low word)
    const uint64_t p0 = (uint64_t)M0 * c0;
    const uint64_t p1 = (uint64_t)M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += W0;
    k1 += W1;
  }
  PhiloxWords r;
  r.w[0] = c0; r.w[1] = c1; r.w[2] = c2; r.w[3] = c3;
  return r;
}

// The four words for q = 4*q4 .. 4*q4+3 at column k of head-batch bh.
PHILOX_INL PhiloxWords attn_drop_words(uint32_t seed_lo, uint32_t seed_hi,
                                       uint32_t bh, uint32_t q4, uint32_t k) {
  return philox4x32_10(k, q4, bh, 0u, seed_lo, seed_hi);
}

// Token sampling (sampling.hip) draws from the same generator in a domain of
// its own: counter = (v >> 2, row, step, 0x53414D50 "SAMP"), so c3 != 0 keeps
// it apart from the dropout mask under one seed. The four words are those of
// vocabulary entries v = 4*v4 .. 4*v4+3 of logits row `row` at token `step`.
PHILOX_INL PhiloxWords sample_words(uint32_t seed_lo, uint32_t seed_hi,
                                    uint32_t row, uint32_t step, uint32_t v4) {
  return philox4x32_10(v4, row, step, 0x53414D50u, seed_lo, seed_hi);
}

// 4-bit keep mask of one call: bit i set iff element q = 4*q4 + i is kept.
PHILOX_INL uint32_t attn_drop_keep4(uint32_t seed_lo, uint32_t seed_hi,
                                    uint32_t bh, uint32_t q4, uint32_t k,
                                    uint32_t thr) {
  const PhiloxWords r = attn_drop_words(seed_lo, seed_hi, bh, q4, k);
  return (uint32_t)(r.w[0] >= thr) | ((uint32_t)(r.w[1] >= thr) << 1) |
         ((uint32_t)(r.w[2] >= thr) << 2) | ((uint32_t)(r.w[3] >= thr) << 3);
}

// Scalar form of the definition (tests / host tools).
PHILOX_INL bool attn_drop_keep(uint64_t seed, uint32_t bh, uint32_t q,
                               uint32_t k, uint32_t thr) {
  const uint32_t m = attn_drop_keep4((uint32_t)seed, (uint32_t)(seed >> 32),
                                     bh, q >> 2, k, thr);
  return (m >> (q & 3)) & 1u;
}

// thr = (uint32)(p * 2^32), 0 < p < 1 (exact in double).
inline uint32_t attn_drop_threshold(double p) {
  return (uint32_t)(p * 4294967296.0);
}
