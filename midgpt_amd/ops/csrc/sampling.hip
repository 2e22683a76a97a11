// Seeded token sampling from one row of logits: top-k by exact radix select,
// then Gumbel-max over the candidates. One 256-thread workgroup per row, one
// launch per token, no host round trip.
//
// Definition (ops/reference.py:sample_scores / sample_candidates are the
// host mirror): for row b, element v,
//   word  = sample_words(seed, b, step, v >> 2)[v & 3]      (philox.h)
//   t     = (2 * (word >> 9) + 1) * 2^-24                   23 bits, in (0,1)
//   score = float(logit[v]) * inv_t - log(-log(t))          standard Gumbel
//   cand  = all v, or { v : logit[v] >= k-th largest logit of the row }
//   token = the lowest v among the candidates of maximal score
// which draws from softmax(logits / T) restricted to cand.
//
// Shape of the work. A bf16 maps to a 16-bit key of the same order, so the
// k-th largest value falls out of two 256-bin histogram passes (high byte,
// then low byte within the chosen high-byte bin), each followed by a suffix
// scan that finds the bin holding rank k. Integer LDS atomics: the counts, and
// so the result, do not depend on the order of arrival. (The high byte of a
// bf16 is its sign and 7 exponent bits, so a row of logits lands in a handful
// of bins; 16 interleaved copies of the histogram to spread a wave's atomics
// measured 51.5 us against 54.2 us for the whole kernel at V = 50304, k = 50,
// and were not kept: see profiles/decode.md.) The last
// pass scores candidates only; one Philox call serves four consecutive v, so
// a unit of 8 elements costs at most two calls and none where it holds no
// candidate. Rows are read from global memory each pass (the lm_head GEMM
// has just written them; 100 KB at V = 50304 sits in L2).
//
// Loads: a unit is 8 consecutive elements at a multiple of 8 in v. Where the
// row starts on a 16-byte boundary a full unit is one 16-byte load; the tail
// unit, and every unit of a row that starts elsewhere (V odd), loads its
// elements one by one, each checked against V.
#include <climits>

#include "common.h"
#include "philox.h"

constexpr int SAMPLE_THREADS = 256;

// Order-preserving key: a > b as floats <=> key(a) > key(b); -0 keys as +0,
// since -0 >= +0 holds for the values.
DEVINL unsigned sample_key(u16 h) {
  if (h == 0x8000u) h = 0;
  return (h & 0x8000u) ? (~(unsigned)h & 0xffffu) : ((unsigned)h | 0x8000u);
}

// The unit at element i of a row of V: h[j] = row[i + j] for i + j < V.
// Returns how many are valid.
DEVINL int sample_load8(const u16* __restrict__ row, int i, int V, bool vec, u16 (&h)[8]) {
  if (vec && i + 8 <= V) {
    const u16x8 x = *(const u16x8*)(row + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = x[j];
    return 8;
  }
  const int n = min(8, V - i);
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = j < n ? row[i + j] : (u16)0;
  return n;
}

// hist: 256 counters. Finds the bin that holds rank k from
// the top (1 <= k <= total count): sel[0] = bin, sel[1] = rank within it.
DEVINL void sample_select_bin(const int* hist, int k, int* wtot, int* sel) {
  const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
  const int h = hist[tid];
  int s = h;  // becomes the count of bins >= tid
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const int y = __shfl_down(s, o);
    if (lane + o < WAVE) s += y;
  }
  if (lane == 0) wtot[wid] = s;
  __syncthreads();
  for (int w = wid + 1; w < SAMPLE_THREADS / WAVE; ++w) s += wtot[w];
  if (s >= k && s - h < k) {
    sel[0] = tid;
    sel[1] = k - (s - h);
  }
  __syncthreads();
}

DEVINL bool sample_better(float s2, int v2, float s, int v) {
  return s2 > s || (s2 == s && v2 < v);
}

// The key of the row's k-th largest logit, 1 <= top_k < V: two histogram
// passes, block-uniform. hist (one bin per thread), wtot and sel are the
// kernel's LDS (a kernel that never selects gets none).
DEVINL unsigned sample_kth_key(const u16* __restrict__ row, int V, bool vec, int top_k,
                               int* hist, int* wtot, int* sel) {
  const int tid = threadIdx.x;
  constexpr int STRIDE = SAMPLE_THREADS * 8;
  unsigned kth = 0;
  int k = top_k;
  unsigned hi = 0;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    if (tid < 2) sel[tid] = tid;  // overwritten below: the counts total at least k
    hist[tid] = 0;
    __syncthreads();
    for (int i = tid * 8; i < V; i += STRIDE) {
      u16 h[8];
      const int n = sample_load8(row, i, V, vec, h);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned key = sample_key(h[j]);
        if (j < n && (pass == 0 || (key >> 8) == hi))
          atomicAdd(&hist[pass == 0 ? key >> 8 : key & 0xffu], 1);
      }
    }
    __syncthreads();
    sample_select_bin(hist, k, wtot, sel);
    if (pass == 0) hi = (unsigned)sel[0];
    else kth = (hi << 8) | (unsigned)sel[0];
    k = sel[1];
    __syncthreads();
  }
  return kth;
}

// Scores the candidates (key >= kth where HAS_K, else all) of the row with
// the noise of Philox row word `b`, reduces over the workgroup and returns the
// token in thread 0. GREEDY_OPT: with greedy set (block-uniform) the score is
// the logit alone and no noise is drawn.
template <bool HAS_K, bool GREEDY_OPT>
DEVINL int sample_pick(const u16* __restrict__ row, int V, bool vec, unsigned kth, float inv_t,
                       uint32_t seed_lo, uint32_t seed_hi, uint32_t b, uint32_t step,
                       bool greedy, float* red_s, int* red_v) {
  const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
  constexpr int STRIDE = SAMPLE_THREADS * 8;
  float best_s = -INFINITY;
  int best_v = INT_MAX;
  for (int i = tid * 8; i < V; i += STRIDE) {
    u16 h[8];
    const int n = sample_load8(row, i, V, vec, h);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      bool any = false;
      bool cand[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cand[j] = half * 4 + j < n && (!HAS_K || sample_key(h[half * 4 + j]) >= kth);
        any |= cand[j];
      }
      if (!any) continue;
      if (GREEDY_OPT && greedy) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!cand[j]) continue;
          const float s = b2f(h[half * 4 + j]);
          const int v = i + half * 4 + j;
          if (sample_better(s, v, best_s, best_v)) { best_s = s; best_v = v; }
        }
        continue;
      }
      const PhiloxWords r =
          sample_words(seed_lo, seed_hi, b, step, (uint32_t)(i >> 2) + half);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!cand[j]) continue;
        // logf, not __logf: -log(t) for t near 1 must be accurate relative
        // to its own size, that is where the largest noise comes from
        const float t = (float)(2u * (r.w[j] >> 9) + 1u) * 0x1p-24f;
        const float s = b2f(h[half * 4 + j]) * inv_t - logf(-logf(t));
        const int v = i + half * 4 + j;
        if (sample_better(s, v, best_s, best_v)) { best_s = s; best_v = v; }
      }
    }
  }
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const float s2 = __shfl_xor(best_s, o);
    const int v2 = __shfl_xor(best_v, o);
    if (sample_better(s2, v2, best_s, best_v)) { best_s = s2; best_v = v2; }
  }
  if (lane == 0) { red_s[wid] = best_s; red_v[wid] = best_v; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < SAMPLE_THREADS / WAVE; ++w)
      if (sample_better(red_s[w], red_v[w], best_s, best_v)) {
        best_s = red_s[w];
        best_v = red_v[w];
      }
  }
  // a row of NaN (outside the contract) leaves no winner: still an index
  return best_v < V ? best_v : 0;
}

// top_k: 1 <= top_k < V where HAS_K (the binding sees to it).
template <bool HAS_K>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_tokens_kernel(
    const u16* __restrict__ logits, long* __restrict__ out, int V, float inv_t, int top_k,
    uint32_t seed_lo, uint32_t seed_hi, uint32_t step) {
  const uint32_t b = blockIdx.x;
  const u16* __restrict__ row = logits + (long)b * V;
  const bool vec = ((uintptr_t)row & 15) == 0;
  __shared__ int hist[SAMPLE_THREADS];
  __shared__ int wtot[SAMPLE_THREADS / WAVE];
  __shared__ int sel[2];
  __shared__ float red_s[SAMPLE_THREADS / WAVE];
  __shared__ int red_v[SAMPLE_THREADS / WAVE];
  unsigned kth = 0;  // candidates: key >= kth
  if (HAS_K) kth = sample_kth_key(row, V, vec, top_k, hist, wtot, sel);
  const int tok = sample_pick<HAS_K, false>(row, V, vec, kth, inv_t, seed_lo, seed_hi, b, step,
                                            false, red_s, red_v);
  if (threadIdx.x == 0) out[b] = tok;
}

// Per-row parameters: row b of the launch draws by the definition above with
// its own values, params[b] = SAMPLE_ROW_WORDS int32 words
//   {seed_lo, seed_hi, step, row, bits of fp32 inv_t, top_k}
// where `row` is the Philox counter word that sample_tokens_kernel fills with
// the batch index, so out[b] is what sample_tokens_kernel gives row `row` of a
// batch whose row `row` holds these logits. top_k outside [1, V): all entries
// (the choice is block-uniform: one workgroup per row). inv_t <= 0 marks a
// greedy row: score = logit, top_k ignored, lowest index of the maximum.
constexpr int SAMPLE_ROW_WORDS = 6;

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_tokens_rows_kernel(
    const u16* __restrict__ logits, long* __restrict__ out, int V,
    const int* __restrict__ params) {
  const uint32_t b = blockIdx.x;
  const u16* __restrict__ row = logits + (long)b * V;
  const bool vec = ((uintptr_t)row & 15) == 0;
  const int* __restrict__ p = params + (long)b * SAMPLE_ROW_WORDS;
  const uint32_t seed_lo = (uint32_t)p[0], seed_hi = (uint32_t)p[1];
  const uint32_t step = (uint32_t)p[2], rowctr = (uint32_t)p[3];
  const float inv_t = __int_as_float(p[4]);
  const int top_k = p[5];
  const bool greedy = !(inv_t > 0.f);
  __shared__ int hist[SAMPLE_THREADS];
  __shared__ int wtot[SAMPLE_THREADS / WAVE];
  __shared__ int sel[2];
  __shared__ float red_s[SAMPLE_THREADS / WAVE];
  __shared__ int red_v[SAMPLE_THREADS / WAVE];
  unsigned kth = 0;  // key >= 0: every entry is a candidate
  if (!greedy && top_k >= 1 && top_k < V)
    kth = sample_kth_key(row, V, vec, top_k, hist, wtot, sel);
  const int tok = sample_pick<true, true>(row, V, vec, kth, inv_t, seed_lo, seed_hi, rowctr,
                                          step, greedy, red_s, red_v);
  if (threadIdx.x == 0) out[b] = tok;
}
