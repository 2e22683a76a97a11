// KV-cache decode kernels for gfx950 (bf16, head dim C in {64, 128}).
//
//   kv_append_kernel     QK-LayerNorm + RoPE of Tn new tokens at absolute
//                        position pos; q goes to (B,H,Tn,C), the K and V rows
//                        straight into the (B,H,Tmax,C) caches.
//   attn_decode_kernel   Tq <= 16 query rows against the cache, split-KV.
//   attn_decode_combine_kernel   merges the per-slice partials.
//   kv_store_paged_kernel   contiguous (B,H,T,C) K/V rows into a paged pool.
//
// The first two have a RAGGED instantiation that reads the position / length
// of sequence b from an int32 array instead of one value for the batch: the
// same body, so sequence b of a ragged call has the bits of the uniform call
// on its slice. The uniform instantiations compile to the same resource
// figures as before the flag (profiles/decode.md).
//
// SLOTS (implies RAGGED) adds one level of indirection for a pool of S cache
// slots: batch row b lives in slot slots[b], so its cache base is
// (slots[b]*H + h)*Tmax*C instead of (b*H + h)*Tmax*C. One more 4-byte load
// per row / block and nothing else: row b of a slotted call has the bits of
// the ragged call on the gathered cache[slots].
//
// PAGED (implies RAGGED, exclusive with SLOTS) takes that indirection per
// block of keys: the caches are pools of P pages, (P,H,PS,C) with PS a power of
// two, and position p of sequence b lives at row p % PS of page
// block_table[b][p / PS] of a (B,MP) int32 table; MP*PS plays the role of Tmax.
// Only the address of a cache row changes, so row b of a paged call has the
// bits of the ragged call on the cache gathered through the table.
// kv_store_paged_kernel copies contiguous K/V rows into the pages (prefill).
//
// Decode attention is a memory-bound stream over K and V with one query row
// per head: no MFMA, no LDS staging. K/V rows go straight to VGPRs with
// 16-byte loads, C/8 lanes per key row.
#pragma once
#include "common.h"

// Same row sequence as qkv_prep_fwd_kernel<3> (row = ((b*Tn + t)*3 + role)*H
// + h) and the same row body (qk_ln_rope_row, norms.hip); only the position
// (pos + t) and the destinations differ. RAGGED: sequence b starts at
// pos_b[b] instead of pos (one more 4-byte load per row, nothing else).
// SLOTS: the cache rows are those of slot slots[b] of S. The binding validated
// the host copy of the map; a device copy that names a slot outside [0, S)
// writes nothing for that row (neither cache nor q).
// PAGED: the caches are (P,H,PS,C) pools with PS = 1 << ps_shift and Tmax =
// MP*PS; row pos + t goes to the page block_table[b][(pos + t) >> ps_shift].
// An entry outside [0, P) (a device table that disagrees with the validated
// host copy) writes nothing for that row, neither cache nor q.
template <bool RAGGED, bool SLOTS = false, bool PAGED = false>
__global__ void kv_append_kernel(const u16* __restrict__ qkv,
                                 const float* __restrict__ qw,
                                 const float* __restrict__ kw,
                                 const float* __restrict__ sin_t,
                                 const float* __restrict__ cos_t,
                                 u16* __restrict__ q, u16* __restrict__ k_cache,
                                 u16* __restrict__ v_cache,
                                 int B, int Tn, int H, int C, long Tmax, long pos,
                                 const int* __restrict__ pos_b, float eps,
                                 const int* __restrict__ slots, int S,
                                 const int* __restrict__ block_table, int P,
                                 int MP, int ps_shift) {
  static_assert(RAGGED || !SLOTS, "SLOTS implies RAGGED");
  static_assert(!PAGED || (RAGGED && !SLOTS), "PAGED implies RAGGED, excludes SLOTS");
  const int LPR = C / 8;                 // lanes per row (8 or 16)
  const int RPW = WAVE / LPR;            // rows per wave
  const int sub = lane_id() % LPR;
  const int rsub = lane_id() / LPR;
  const long nrows = (long)B * Tn * H * 3;
  const long row0 = ((long)blockIdx.x * (blockDim.x / WAVE) + wave_id()) * RPW + rsub;
  const long rstep = (long)gridDim.x * (blockDim.x / WAVE) * RPW;
  for (long row = row0; row < nrows; row += rstep) {
    const long h = row % H;
    const long rest = row / H;
    const int role = (int)(rest % 3);
    const long bt = rest / 3;            // = b*Tn + t
    const long t = bt % Tn;
    const long b = bt / Tn;
    if constexpr (RAGGED) {
      pos = pos_b[b];
      // the binding validated the host copy; a device copy that disagrees
      // must not write outside the cache
      if (pos < 0 || pos + Tn > Tmax) continue;
    }
    long cb = b;                         // cache row of the batch
    if constexpr (SLOTS) {
      cb = slots[b];
      if (cb < 0 || cb >= S) continue;
    }
    long crow = pos + t;                 // row inside the cache of (cb, h)
    long cstride = Tmax;                 // rows per (cb, h)
    if constexpr (PAGED) {
      cb = block_table[b * MP + (crow >> ps_shift)];
      if (cb < 0 || cb >= P) continue;
      cstride = 1L << ps_shift;
      crow &= cstride - 1;
    }
    const u16x8 raw = *(const u16x8*)(qkv + ((bt * 3 + role) * H + h) * C + sub * 8);
    const long cache_off = ((cb * H + h) * cstride + crow) * C + sub * 8;
    if (role == 2) {
      *(u16x8*)(v_cache + cache_off) = raw;
      continue;
    }
    float mu, invstd;
    const u16x8 out = qk_ln_rope_row(raw, role == 0 ? qw : kw,
                                     sin_t + (pos + t) * (C / 2) + sub * 4,
                                     cos_t + (pos + t) * (C / 2) + sub * 4, C, LPR,
                                     sub, eps, mu, invstd);
    if (role == 0)
      *(u16x8*)(q + ((b * H + h) * Tn + t) * C + sub * 8) = out;
    else
      *(u16x8*)(k_cache + cache_off) = out;
  }
}

#define DECODE_NEG_INF (-__builtin_inff())

// exp(m - m_ref) as the weight of a partial with running max m when merged
// under m_ref >= m. A partial that saw no key has m = -inf (and l = acc = 0):
// its weight is 0, not exp(-inf - -inf) = NaN.
DEVINL float decode_weight(float m, float m_ref) {
  return m == DECODE_NEG_INF ? 0.f : __expf(m - m_ref);
}

// One block = one query row (b, h, i) x one slice of its keys. Row i of Tq
// sees keys [0, limit) with limit = kv_len - Tq + i + 1; the slice is
// [k0, k1) = the split-th of num_splits equal parts of that range, possibly
// empty. No cache row >= limit is ever loaded (the cache tail is
// uninitialised memory). RAGGED: kv_len is read per sequence from
// kv_lens[b]; a short sequence next to a long one has short, possibly empty,
// slices, and everything else is the same code. SLOTS: the keys of sequence b
// are those of cache slot slots[b] of S. The host copy of the map is the
// truth; for a device copy that names a slot outside [0, S) the block treats
// its row as kv_len = Tq in slot 0: it reads rows [0, Tq) of a cache that
// exists, never anything outside it, and slice 0 still writes its output or
// partials (whatever those rows hold). PAGED: key k of sequence b is row
// k % PS of page block_table[b][k / PS] of a (P,H,PS,C) pool, Tmax = MP*PS.
// The table entries of a batch of U keys are loaded ahead of its K/V loads,
// one batch early, so a batch still has 2*U 16-byte loads in flight and an
// iteration does not wait for two dependent loads. For an entry outside [0, P)
// (a device table that disagrees with the host copy) the key is read from
// page 0: in bounds, the values unspecified.
//
// 256 threads form G = 256/(C/8) lane groups; group g takes keys k0+g,
// k0+g+G, ... in batches of U keys whose K and V loads (2*U 16-byte loads per
// lane) are all issued before the first use. Scores, online softmax and the
// P.V accumulation are fp32; every lane of a group carries the group's (m, l)
// and its own 8 columns of acc. Groups merge by shuffles, waves through LDS.
// num_splits == 1: writes o (B,Tq,H,C) bf16. Otherwise writes the slice's
// fp32 (m, l) to ws_ml[row][split][2] and acc to ws_acc[row][split][C].
template <int C, bool RAGGED, bool SLOTS = false, bool PAGED = false>
__global__ __launch_bounds__(256) void attn_decode_kernel(
    const u16* __restrict__ q, const u16* __restrict__ k_cache,
    const u16* __restrict__ v_cache, u16* __restrict__ o,
    float* __restrict__ ws_acc, float* __restrict__ ws_ml,
    int H, int Tq, long Tmax, int kv_len, const int* __restrict__ kv_lens,
    int num_splits, float scale, const int* __restrict__ slots, int S,
    const int* __restrict__ block_table, int P, int MP, int ps_shift) {
  static_assert(RAGGED || !SLOTS, "SLOTS implies RAGGED");
  static_assert(!PAGED || (RAGGED && !SLOTS), "PAGED implies RAGGED, excludes SLOTS");
  constexpr int LPR = C / 8;
  constexpr int G = 256 / LPR;
  constexpr int U = 4;
  constexpr int NWAVE = 256 / WAVE;
  const int row = blockIdx.x;            // (b*H + h)*Tq + i
  const int split = blockIdx.y;
  const int i = row % Tq;
  const int bh = row / Tq;
  int cbh = bh;                          // (cache row of the batch)*H + h
  // min: a device copy that disagrees with the validated host one must not
  // read past the cache
  if constexpr (SLOTS) {
    const int slot = slots[bh / H];
    const bool ok = (unsigned)slot < (unsigned)S;
    // the length load inside the guard: written after it, the same code
    // takes 15 more VGPRs (profiles/decode.md)
    kv_len = ok ? min(kv_lens[bh / H], (int)Tmax) : Tq;
    cbh = (ok ? slot : 0) * H + bh % H;
  } else if constexpr (PAGED) {
    // max: nor must it make a slice start below key 0 (Tq <= Tmax on the host)
    kv_len = max(Tq, min(kv_lens[bh / H], (int)Tmax));
  } else if constexpr (RAGGED) {
    kv_len = min(kv_lens[bh / H], (int)Tmax);
  }
  const int limit = kv_len - Tq + i + 1;
  const int per = (limit + num_splits - 1) / num_splits;
  const int k0 = split * per;
  const int k1 = min(limit, k0 + per);
  const int sub = threadIdx.x % LPR;
  const int g = threadIdx.x / LPR;
  // PAGED: the page is part of the row offset, not of the base
  const u16* kb = k_cache + (PAGED ? 0 : (long)cbh * Tmax * C) + sub * 8;
  const u16* vb = v_cache + (PAGED ? 0 : (long)cbh * Tmax * C) + sub * 8;
  const int* tb = PAGED ? block_table + (long)(bh / H) * MP : nullptr;

  float qf[8];
  {
    const u16x8 qr = *(const u16x8*)(q + (long)row * C + sub * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] = b2f(qr[j]);
  }
  float m = DECODE_NEG_INF, l = 0.f;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;

  // The first key of a batch (kk) is always inside the slice, so every batch
  // has a finite maximum.
  // PAGED: the table entries of a batch, loaded while the batch before it is
  // in flight, so that an iteration waits for one memory latency, not two.
  [[maybe_unused]] int page[U];
  if constexpr (PAGED) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = k0 + g + u * G;
      page[u] = key < k1 ? tb[key >> ps_shift] : 0;
    }
  }
  for (int kk = k0 + g; kk < k1; kk += G * U) {
    u16x8 kr[U], vr[U];
    bool ok[U];
    [[maybe_unused]] int page_next[U];
    if constexpr (PAGED) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long key = (long)kk + G * U + u * G;
        page_next[u] = key < k1 ? tb[key >> ps_shift] : 0;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = kk + u * G;
      ok[u] = key < k1;
      kr[u] = 0;
      vr[u] = 0;
      if (ok[u]) {
        long crow = key;                 // row of the key from kb / vb
        if constexpr (PAGED) {
          const long pg = (unsigned)page[u] < (unsigned)P ? page[u] : 0;
          crow = ((pg * H + bh % H) << ps_shift) + (key & ((1 << ps_shift) - 1));
        }
        kr[u] = *(const u16x8*)(kb + crow * C);
        vr[u] = *(const u16x8*)(vb + crow * C);
      }
    }
    float s[U];
    float mb = DECODE_NEG_INF;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) d += qf[j] * b2f(kr[u][j]);
      d = group_sum<LPR>(d) * scale;
      s[u] = ok[u] ? d : DECODE_NEG_INF;
      mb = fmaxf(mb, s[u]);
    }
    const float mn = fmaxf(m, mb);
    const float corr = __expf(m - mn);   // m = -inf on the first batch: 0
    l *= corr;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= corr;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float p = __expf(s[u] - mn); // 0 for a key outside the slice
      l += p;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += p * b2f(vr[u][j]);
    }
    m = mn;
    if constexpr (PAGED) {
#pragma unroll
      for (int u = 0; u < U; ++u) page[u] = page_next[u];
    }
  }

  // merge the lane groups of a wave
#pragma unroll
  for (int off = LPR; off < WAVE; off <<= 1) {
    const float m2 = __shfl_xor(m, off);
    const float l2 = __shfl_xor(l, off);
    const float mn = fmaxf(m, m2);
    const float f1 = decode_weight(m, mn), f2 = decode_weight(m2, mn);
    l = l * f1 + l2 * f2;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = acc[j] * f1 + __shfl_xor(acc[j], off) * f2;
    m = mn;
  }

  // merge the waves
  __shared__ float sm_acc[NWAVE][C];
  __shared__ float sm_ml[NWAVE][2];
  if (lane_id() < LPR) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sm_acc[wave_id()][sub * 8 + j] = acc[j];
    if (lane_id() == 0) {
      sm_ml[wave_id()][0] = m;
      sm_ml[wave_id()][1] = l;
    }
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < C) {
    float M = sm_ml[0][0];
#pragma unroll
    for (int w = 1; w < NWAVE; ++w) M = fmaxf(M, sm_ml[w][0]);
    float L = 0.f, A = 0.f;
#pragma unroll
    for (int w = 0; w < NWAVE; ++w) {
      const float f = decode_weight(sm_ml[w][0], M);
      L += sm_ml[w][1] * f;
      A += sm_acc[w][c] * f;
    }
    if (num_splits == 1) {
      // split 0 of 1 holds key 0 at least: L > 0
      const int b = bh / H, h = bh % H;
      o[(((long)b * Tq + i) * H + h) * C + c] = f2b(A / L);
    } else {
      const long part = (long)row * num_splits + split;
      ws_acc[part * C + c] = A;          // empty slice: M = -inf, L = A = 0
      if (c == 0) {
        ws_ml[part * 2] = M;
        ws_ml[part * 2 + 1] = L;
      }
    }
  }
}

// One block of C threads per query row: o = sum_s acc_s w_s / sum_s l_s w_s
// with w_s = exp(m_s - max m). Slice 0 is never empty, so the sum of l is > 0.
__global__ void attn_decode_combine_kernel(const float* __restrict__ ws_acc,
                                           const float* __restrict__ ws_ml,
                                           u16* __restrict__ o, int H, int Tq,
                                           int C, int num_splits) {
  const int row = blockIdx.x;
  const int c = threadIdx.x;
  const float* ml = ws_ml + (long)row * num_splits * 2;
  const float* ac = ws_acc + (long)row * num_splits * C + c;
  float M = DECODE_NEG_INF;
  for (int s = 0; s < num_splits; ++s) M = fmaxf(M, ml[2 * s]);
  float L = 0.f, A = 0.f;
  for (int s = 0; s < num_splits; ++s) {
    const float f = decode_weight(ml[2 * s], M);
    L += ml[2 * s + 1] * f;
    A += ac[(long)s * C] * f;
  }
  const int i = row % Tq, bh = row / Tq;
  const int b = bh / H, h = bh % H;
  o[(((long)b * Tq + i) * H + h) * C + c] = f2b(A / L);
}

// Rows [0, lens[b]) of contiguous k, v (B,H,T,C) into the pages block_table
// names: row t of sequence b goes to row t % PS of page block_table[b][t / PS]
// of the (P,H,PS,C) pools. One 16-byte unit of K and of V per lane and
// iteration, grid-stride; nothing else is written. A device length above
// min(T, MP*PS) is cut to it and a table entry outside [0, P) writes nothing:
// no access leaves the pools (the binding validated the host copies).
__global__ void kv_store_paged_kernel(const u16* __restrict__ k,
                                      const u16* __restrict__ v,
                                      u16* __restrict__ k_pool, u16* __restrict__ v_pool,
                                      const int* __restrict__ lens,
                                      const int* __restrict__ block_table, int B, int H,
                                      int T, int C, int P, int MP, int ps_shift) {
  const int LPR = C / 8;
  const long nunits = (long)B * H * T * LPR;
  const long step = (long)gridDim.x * blockDim.x;
  const long tcap = min((long)T, (long)MP << ps_shift);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nunits; i += step) {
    const int sub = (int)(i % LPR);
    const long row = i / LPR;            // (b*H + h)*T + t
    const long t = row % T;
    const long bh = row / T;
    const long h = bh % H, b = bh / H;
    if (t >= min((long)lens[b], tcap)) continue;
    const long pg = block_table[b * MP + (t >> ps_shift)];
    if (pg < 0 || pg >= P) continue;
    const long dst = (((pg * H + h) << ps_shift) + (t & ((1L << ps_shift) - 1))) * C + sub * 8;
    *(u16x8*)(k_pool + dst) = *(const u16x8*)(k + row * C + sub * 8);
    *(u16x8*)(v_pool + dst) = *(const u16x8*)(v + row * C + sub * 8);
  }
}
