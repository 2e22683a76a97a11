// Flash-style causal attention, forward + backward (plans K1/K2).
// MI355X-native: MFMA v_mfma_f32_32x32x16_bf16 tiles, LDS-staged K/V with
// XOR swizzles (guide T2/G4), online fp32 softmax held IN REGISTERS via the
// swapped-QK^T layout + permlane32_swap half exchanges (guide T12), fp32
// LSE saved for the recompute-based backward.
//
// Reference numerics: softmax(mask(QK^T)/sqrt(C)) in fp32, bf16 elsewhere
// (reference src/model.py:71-79). The T x T score matrix is never
// materialized.
//
// Geometry (fwd): one workgroup = NW waves (8 at T%256==0, else 4), each
// wave owning 32 q rows; KV tiles of 32 rows double-buffered in LDS with
// T14 load-early/write-late staging; grid = B*H*(T/(NW*32)), ordered so
// one (b,h)'s q-blocks share an XCD's L2.
// Geometry (bwd): TWO kernels — dkv (workgroup = NW*32 k rows, iterates
// q tiles >= its diagonal; dK/dV accumulate in registers) and dq
// (workgroup = NW*32 q rows, iterates k tiles; dQ in registers, no
// atomics), both with double-buffered T14 staging. A delta kernel
// (rowsum(dO*O)) runs first.
#include "common.h"
#include "mfma.h"
#include "philox.h"

// ---------------------------------------------------------------------------
// Operand addressing. Q, K, dQ, dK, LSE and delta are always (B,H,T,*)
// packed. O, dO, V and dV carry explicit strides in elements (the head dim
// is contiguous), so the same kernels serve the (B,H,T,C) layout, O/dO kept
// as (B,T,H,C) — what the output projection consumes, no transpose copy —
// and V/dV living in slot 2 of the packed (B,T,3,H,C) projection.
// ---------------------------------------------------------------------------
struct AttnStrides {
  long b, h;  // batch and head stride
  int r;      // row (t) stride
};
DEVINL long bh_base(const AttnStrides& s, long bh, int H) {
  return (bh / H) * s.b + (bh % H) * s.h;
}

// ---------------------------------------------------------------------------
// LDS swizzles
// ---------------------------------------------------------------------------
// Row-major [R][C] bf16 tile, rows of C*2 bytes, read by ds_read_b128 at
// per-lane rows: XOR byte bits 4..7 with row (C=128: row&15 -> conflict-free;
// C=64 rows are 128 B: row&7).
template <int C> DEVINL int swz_rm(int row, int byte_in_row) {
  constexpr int M = (C == 128) ? 15 : 7;
  return byte_in_row ^ ((row & M) << 4);
}
// Transposed [C][32] bf16 tile (rows of 64 B): XOR byte bits 4..5 with
// (row>>2)&3 (see analysis: removes the 4-way conflict of the 64-B stride).
DEVINL int swz_tr(int row, int byte_in_row) {
  return byte_in_row ^ (((row >> 2) & 3) << 4);
}

// ---------------------------------------------------------------------------
// Cooperative staging (T14 async split: issue global loads EARLY, hold the
// tile in registers through the compute phase, ds_write late — the HBM
// latency hides under the MFMA phase instead of stalling the wave at a
// vmcnt before its LDS writes).
// ---------------------------------------------------------------------------
// ld = row stride of the global tile, in elements. The per-thread offset
// row*ld + col is 32-bit and loop-invariant; only the wave-uniform tile base g
// advances from tile to tile.
// Single-row loader -> row-major swizzled image only.
template <int C, int NT>
struct RmStage {
  static constexpr int NV = (32 * C + NT * 8 - 1) / (NT * 8);
  // The first NF passes take every thread. Only a last, partial pass is
  // predicated: a run-time exec branch around a load hides from the compiler
  // which loads are outstanding, and the waits it then places for safety
  // land in the tile loop's MFMA phase.
  static constexpr int NF = (32 * C) / (NT * 8);
  u16x8 v[NV];
  DEVINL void load1(const u16* __restrict__ g, int ld, unsigned boff, int i) {
    v[i] = *(const u16x8*)((const char*)(g + (long)(i * (NT * 8 / C)) * ld) + boff);
  }
  DEVINL void load(const u16* __restrict__ g, int ld = C) {
    static_assert((NT * 8) % C == 0, "a thread keeps its column across loads");
    const int idx0 = threadIdx.x * 8;
    const unsigned boff = 2u * (unsigned)((idx0 / C) * ld + idx0 % C);  // bytes
#pragma unroll
    for (int i = 0; i < NF; ++i) load1(g, ld, boff, i);
    if constexpr (NV > NF) {
      if (idx0 + NF * NT * 8 < 32 * C) load1(g, ld, boff, NF);
    }
  }
  DEVINL void write1(u16* lds, int i) const {
    const int idx = threadIdx.x * 8 + i * NT * 8;
    const int row = idx / C, col = idx % C;
    *(u16x8*)((char*)lds + row * C * 2 + swz_rm<C>(row, col * 2)) = v[i];
  }
  DEVINL void write(u16* lds) const {
#pragma unroll
    for (int i = 0; i < NF; ++i) write1(lds, i);
    if constexpr (NV > NF) {
      if ((int)threadIdx.x * 8 + NF * NT * 8 < 32 * C) write1(lds, NF);
    }
  }
};
// Row-pair loader -> transposed image (u16x2 pair writes), and optionally
// also the row-major image (both from ONE set of global loads).
// ACCK (the backward kernels): the transposed image has its 32 rows at
// acc_k_pos (mfma.h) inside each image row, for a reader whose other operand
// is a dlayout_pack'ed accumulator.
template <int C, int NT, bool ACCK = false>
struct TrStage {
  static constexpr int NP = (32 * C + NT * 16 - 1) / (NT * 16);
  static constexpr int NF = (32 * C) / (NT * 16);  // unpredicated, as in RmStage
  // Whether this thread has a part in pass i: known at compile time but for
  // a last, partial pass.
  static DEVINL bool mine(int i) { return (int)threadIdx.x * 16 + i * NT * 16 < 32 * C; }
  u16x8 a[NP], b[NP];  // rows 2p and 2p+1 at an 8-col span
  DEVINL void load1(const u16* __restrict__ g, int ld, unsigned boff, int i) {
    // row pair i of this thread: 2 * (NT * 8 / C) rows further down
    const u16* gi = g + (long)(i * 2 * (NT * 8 / C)) * ld;
    // Row 2p+1 sits one (wave-uniform, runtime) row stride after row 2p.
    // Kept opaque so that the second address is formed from the first at
    // issue time, not carried through the tile loop as a pointer of its own.
    int ldb = 2 * ld;
    asm volatile("" : "+s"(ldb));
    if constexpr (ACCK) {
      // Wave-uniform base plus a 32-bit lane offset, opaque so that the
      // loop keeps no 64-bit per-lane pointer alive from tile to tile.
      unsigned off = boff;
      asm volatile("" : "+v"(off));
      a[i] = *(const u16x8*)((const char*)gi + off);
      b[i] = *(const u16x8*)((const char*)gi + ldb + off);
    } else {
      const char* pa = (const char*)gi + boff;
      a[i] = *(const u16x8*)pa;
      b[i] = *(const u16x8*)(pa + ldb);
    }
  }
  DEVINL void load(const u16* __restrict__ g, int ld = C) {
    static_assert((NT * 8) % C == 0, "a thread keeps its column across loads");
    const int idx0 = threadIdx.x * 16;
    const unsigned boff =  // bytes
        2u * (unsigned)(2 * (idx0 / (2 * C)) * ld + (idx0 / 2) % C);
#pragma unroll
    for (int i = 0; i < NF; ++i) load1(g, ld, boff, i);
    if constexpr (NP > NF) {
      if (mine(NF)) load1(g, ld, boff, NF);
    }
  }
  // A row pair (2p, 2p+1) stays a pair under acc_k_pos.
  DEVINL void write_tr1(u16* lds, int i) const {
    const int idx = threadIdx.x * 16 + i * NT * 16;
    const int row0 = 2 * (idx / (2 * C));
    const int row = ACCK ? acc_k_pos(row0) : row0;
    const int col = (idx / 2) % C;
    // The pairs are cut out of the loaded dwords with integer ops.
    // Element-wise u16 extraction (pv.x = a[i][j]; pv.y = b[i][j]) makes the
    // compiler keep a and b in a stack slot: every tile's loads are then
    // waited for and stored to scratch where they are issued, and the
    // prefetch hides nothing.
    const u32x4 aw = __builtin_bit_cast(u32x4, a[i]);
    const u32x4 bw = __builtin_bit_cast(u32x4, b[i]);
    // col is a multiple of 8, so swz_tr(col + j, x) is
    // x ^ 32*((col>>3)&1) ^ 16*(j>>2): two bases per thread and the
    // rest in the store's offset field, not eight address registers.
    const int x = (row * 2) ^ (((col >> 3) & 1) << 5);
    char* const p0 = (char*)lds + col * 64 + x;
    char* const p1 = (char*)lds + col * 64 + (x ^ 16);
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // LDS row = col + j
      const unsigned pv = (j & 1)
          ? (aw[j >> 1] >> 16) | (bw[j >> 1] & 0xffff0000u)
          : (aw[j >> 1] & 0xffffu) | (bw[j >> 1] << 16);
      *(unsigned*)((j < 4 ? p0 : p1) + j * 64) = pv;
    }
  }
  DEVINL void write_tr(u16* lds) const {
#pragma unroll
    for (int i = 0; i < NF; ++i) write_tr1(lds, i);
    if constexpr (NP > NF) {
      if (mine(NF)) write_tr1(lds, NF);
    }
  }
  DEVINL void write_rm1(u16* lds, int i) const {
    const int idx = threadIdx.x * 16 + i * NT * 16;
    const int row = 2 * (idx / (2 * C));
    const int col = (idx / 2) % C;
    *(u16x8*)((char*)lds + row * C * 2 + swz_rm<C>(row, col * 2)) = a[i];
    *(u16x8*)((char*)lds + (row + 1) * C * 2 + swz_rm<C>(row + 1, col * 2)) = b[i];
  }
  DEVINL void write_rm(u16* lds) const {
#pragma unroll
    for (int i = 0; i < NF; ++i) write_rm1(lds, i);
    if constexpr (NP > NF) {
      if (mine(NF)) write_rm1(lds, NF);
    }
  }
};
// Synchronous convenience wrappers (prologue use).
template <int C, int NT>
DEVINL void stage_rm(const u16* __restrict__ g, u16* lds, int ld = C) {
  RmStage<C, NT> st; st.load(g, ld); st.write(lds);
}
template <int C, int NT, bool ACCK = false>
DEVINL void stage_tr(const u16* __restrict__ g, u16* lds, int ld = C) {
  TrStage<C, NT, ACCK> st; st.load(g, ld); st.write_tr(lds);
}

// Read one A/B fragment (bf16x8) from a swizzled row-major [R][C] tile:
// lane l -> row (l&31)+row0, bytes 16*chunk32? caller passes byte base.
template <int C>
DEVINL bf16x8_t read_rm_frag(const u16* lds, int row, int cbyte) {
  return *(const bf16x8_t*)((const char*)lds + row * C * 2 + swz_rm<C>(row, cbyte));
}
DEVINL bf16x8_t read_tr_frag(const u16* lds, int row, int kbyte) {
  return *(const bf16x8_t*)((const char*)lds + row * 64 + swz_tr(row, kbyte));
}

DEVINL float shfl32(float v, int src) { return __shfl(v, src, 32); }

// ===========================================================================
// Forward. SPW strips per wave: with SPW=2 each wave owns MIRRORED strips
// (w and NW*SPW-1-w), so causal work per wave is exactly equal and the
// staging barriers park nobody (the measured 50% SQ_WAIT_ANY at SPW=1 came
// from low-diagonal waves waiting on high-diagonal ones).
// ===========================================================================
//
// DROP: attention dropout (philox.h). m, lsum and the saved LSE come from
// the UNDROPPED P; only the P fragments fed to the PV MFMA are masked, and
// 1/(1-p) is folded into the epilogue's 1/lsum.
template <int C, int NW, int SPW, bool DROP = false>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_kernel(const u16* __restrict__ q,
                                const u16* __restrict__ k,
                                const u16* __restrict__ v,
                                u16* __restrict__ o, float* __restrict__ lse,
                                int B, int H, int T,
                                AttnStrides sv, AttnStrides so,
                                uint32_t seed_lo = 0, uint32_t seed_hi = 0,
                                uint32_t drop_thr = 0, float inv_keep = 1.f) {
  constexpr int NCB = C / 32;   // 32-col c-blocks
  constexpr int NCH = C / 16;   // 16-deep mfma chunks
  constexpr int NSTRIP = NW * SPW;
  const float scale = rsqrtf((float)C);
  // qb-outermost grid order: all q-blocks of one (b,h) land on the same
  // XCD (b%8 dispatch) for K/V L2 reuse (guide T1).
  const long bh = blockIdx.x % ((long)B * H);
  const int qb = blockIdx.x / (B * H);
  const int q0 = qb * (NSTRIP * 32);
  const int lane = lane_id();
  const int w = wave_id();
  int strip[SPW];
  strip[0] = w;
  if (SPW == 2) strip[1] = NSTRIP - 1 - w;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  u16* ldsK = (u16*)smem;                       // [2][32*C]
  u16* ldsVt = (u16*)(smem + 2 * 32 * C * 2);   // [2][C*32]
  float* obuf = (float*)smem;                   // epilogue reuse: [NW][32*32]

  const u16* qg = q + (bh * T) * C;
  const u16* kg = k + (bh * T) * C;
  const u16* vg = v + bh_base(sv, bh, H);

  // Q B-fragments in registers for the LAST (busiest) strip only; earlier
  // strips re-read their Q rows from global per tile (L2-resident, few
  // tiles) to stay under the 256-VGPR cap at 2 waves/SIMD.
  bf16x8_t qf[NCH];
  f32x16 oacc[SPW][NCB];
  float m[SPW], lsum[SPW];
  {
    const u16* qrow = qg + (long)(q0 + 32 * strip[SPW - 1] + (lane & 31)) * C;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
      qf[ch] = *(const bf16x8_t*)(qrow + 16 * ch + 8 * (lane >> 5));
  }
#pragma unroll
  for (int sp = 0; sp < SPW; ++sp) {
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) oacc[sp][cb] = (f32x16)(0.f);
    m[sp] = -1e30f;
    lsum[sp] = 0.f;
  }

  const int nkt = (q0 + NSTRIP * 32) / 32;
  stage_rm<C, NW * 64>(kg, ldsK);
  stage_tr<C, NW * 64>(vg, ldsVt, sv.r);
  __syncthreads();
  // Every prologue load (Q fragments, staging) has landed, as in the backward
  // kernels: the vmcnt waits inside the loop then count its own prefetch alone
  // and stand in front of the staged tile's ds_write, not among the S MFMAs.
  __builtin_amdgcn_s_waitcnt(0);

  RmStage<C, NW * 64> kst;
  TrStage<C, NW * 64> vst;
  for (int kt = 0; kt < nkt; ++kt) {
    const int buf = kt & 1;
    const bool pre = kt + 1 < nkt;
    if (pre) {  // T14: issue next tile's loads before this tile's compute
      kst.load(kg + (long)(kt + 1) * 32 * C);
      vst.load(vg + (long)(kt + 1) * 32 * sv.r, sv.r);
    }
    const int k0 = kt * 32;
#pragma unroll
    for (int sp = 0; sp < SPW; ++sp) {
      const int qw0 = q0 + 32 * strip[sp];
      const int myq = qw0 + (lane & 31);
      if (k0 > qw0 + 31) continue;  // wave-uniform per strip
      // S = K x Q^T  (swapped: D rows = k, cols = q)
      f32x16 s = (f32x16)(0.f);
      const u16* kb = ldsK + buf * 32 * C;
      const u16* qrow = qg + (long)myq * C;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        bf16x8_t a = read_rm_frag<C>(kb, lane & 31, 16 * ch * 2 + 16 * (lane >> 5));
        bf16x8_t qfr = (sp == SPW - 1) ? qf[ch]
            : *(const bf16x8_t*)(qrow + 16 * ch + 8 * (lane >> 5));
        s = mfma_32x32x16_bf16(a, qfr, s);
      }
      // mask + tile row-max (per q = lane&31; halves merged via xor 32)
      float sv[16];
      float mt = -1e30f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sv[r] = (k0 + mfma_d_row(lane, r) > myq) ? -1e30f : s[r];
        mt = fmaxf(mt, sv[r]);
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32));
      const float mn = fmaxf(m[sp], mt);
      const float alpha = __expf((m[sp] - mn) * scale);
      const bool need_rescale = !__all(mt <= m[sp]);  // EXACT: alpha==1 otherwise
      m[sp] = mn;
      float p[16], psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = __expf((sv[r] - mn) * scale);
        psum += p[r];
      }
      psum += __shfl_xor(psum, 32);
      lsum[sp] = lsum[sp] * alpha + psum;
      // rescale O by alpha[q_of_reg] — skipped (exactly) when no row's max
      // grew this tile, which is most tiles once the running max settles
      if (need_rescale) {
        float arow[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) arow[r] = shfl32(alpha, mfma_d_row(lane, r));
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[sp][cb][r] *= arow[r];
      }
      if constexpr (DROP) {
        // The mask groups four consecutive q at one k into one Philox
        // call; here registers run along k at ONE q, but the four lanes of
        // a quad hold q = 4g..4g+3 at the same 16 k. Lane j = lane&3 of
        // the quad evaluates the calls of registers 4j..4j+3 (bit 4c+i of
        // its mask = keep(q = 4g+i, k of reg 4j+c)); every lane then reads
        // the four quad masks and picks its own q's bit.
        const int j = lane & 3;
        const uint32_t q4 = (uint32_t)myq >> 2;
        uint32_t mine = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          mine |= attn_drop_keep4(seed_lo, seed_hi, (uint32_t)bh, q4,
                                  (uint32_t)(k0 + c + 8 * j + 4 * (lane >> 5)),
                                  drop_thr) << (4 * c);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint32_t mg = (uint32_t)__shfl((int)mine, g, 4);
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (!((mg >> (4 * c + j)) & 1u)) p[4 * g + c] = 0.f;
        }
      }
      // P -> bf16 A-fragments; PV
      bf16x8_t pf0 = dlayout_to_afrag(p);
      bf16x8_t pf1 = dlayout_to_afrag(p + 8);
      const u16* vb = ldsVt + buf * C * 32;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        bf16x8_t b0 = read_tr_frag(vb, 32 * cb + (lane & 31), 16 * (lane >> 5));
        bf16x8_t b1 = read_tr_frag(vb, 32 * cb + (lane & 31), 32 + 16 * (lane >> 5));
        oacc[sp][cb] = mfma_32x32x16_bf16(pf0, b0, oacc[sp][cb]);
        oacc[sp][cb] = mfma_32x32x16_bf16(pf1, b1, oacc[sp][cb]);
      }
    }
    if (pre) {  // T14: LDS writes after compute (loads have landed by now)
      kst.write(ldsK + (1 - buf) * 32 * C);
      vst.write_tr(ldsVt + (1 - buf) * C * 32);
    }
    __syncthreads();
  }

  // epilogue: normalize, bounce through LDS, wide stores (per strip)
#pragma unroll
  for (int sp = 0; sp < SPW; ++sp) {
    const int qw0 = q0 + 32 * strip[sp];
    const int myq = qw0 + (lane & 31);
    float rec = 1.f / lsum[sp];
    if constexpr (DROP) rec *= inv_keep;  // Z = keep/(1-p): scale applied once
    float rrow[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rrow[r] = shfl32(rec, mfma_d_row(lane, r));
    if (lane < 32) lse[bh * T + myq] = m[sp] * scale + __logf(lsum[sp]);
    float* ob = obuf + w * 32 * 32;
    u16* og = o + bh_base(so, bh, H) + (long)qw0 * so.r;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mfma_d_row(lane, r);
        *(float*)((char*)ob + row * 128 + (((lane & 31) * 4) ^ ((row & 7) << 4))) =
            oacc[sp][cb][r] * rrow[r];
      }
      __builtin_amdgcn_s_waitcnt(0);  // lgkmcnt: LDS writes land (same wave)
      const int row = lane & 31;
      const int c16 = 16 * (lane >> 5);
      float tmp[16];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 t = *(const f32x4*)((char*)ob + row * 128 + (((c16 + 4 * i) * 4) ^ ((row & 7) << 4)));
        tmp[4 * i] = t[0]; tmp[4 * i + 1] = t[1]; tmp[4 * i + 2] = t[2]; tmp[4 * i + 3] = t[3];
      }
      u16x8 out0, out1;
#pragma unroll
      for (int j = 0; j < 8; ++j) { out0[j] = f2b(tmp[j]); out1[j] = f2b(tmp[8 + j]); }
      *(u16x8*)(og + (long)row * so.r + 32 * cb + c16) = out0;
      *(u16x8*)(og + (long)row * so.r + 32 * cb + c16 + 8) = out1;
      __builtin_amdgcn_s_waitcnt(0);
    }
  }
}

// ===========================================================================
// Forward, PAIRED variant: two 32-row KV tiles per barrier round with ONE
// merged online-softmax rescale — halves barrier rounds and O-rescale
// passes vs the single-tile loop. nkt is always even (multiple of NW).
// Launched for C=128 at NW=8 only (+4% there, -4% at C=64).
// ===========================================================================
template <int C, int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd2_kernel(
    const u16* __restrict__ q, const u16* __restrict__ k,
    const u16* __restrict__ v, u16* __restrict__ o, float* __restrict__ lse,
    int B, int H, int T, AttnStrides sv, AttnStrides so) {
  constexpr int NCB = C / 32;
  constexpr int NCH = C / 16;
  const float scale = rsqrtf((float)C);
  const long bh = blockIdx.x % ((long)B * H);
  // The last q-block has the most rounds: heaviest first, so that the grid's
  // tail is made of the short blocks (-1.4 % per call at T=1024; the same
  // order measured +1.0 % in the dq kernel, which keeps the ascending one).
  const int qb = T / (NW * 32) - 1 - blockIdx.x / (B * H);
  const int q0 = qb * (NW * 32);
  const int lane = lane_id();
  const int w = wave_id();
  const int qw0 = q0 + 32 * w;
  const int myq = qw0 + (lane & 31);

  extern __shared__ __attribute__((aligned(16))) char smem[];
  u16* ldsK = (u16*)smem;                       // [2][2][32*C]
  u16* ldsVt = (u16*)(smem + 2 * 64 * C * 2);   // [2][2][C*32]
  float* obuf = (float*)smem;                   // epilogue reuse

  const u16* qg = q + (bh * T) * C;
  const u16* kg = k + (bh * T) * C;
  const u16* vg = v + bh_base(sv, bh, H);

  bf16x8_t qf[NCH];
  {
    const u16* qrow = qg + (long)myq * C;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
      qf[ch] = *(const bf16x8_t*)(qrow + 16 * ch + 8 * (lane >> 5));
  }
  f32x16 oacc[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) oacc[cb] = (f32x16)(0.f);
  float m = -1e30f, lsum = 0.f;

  const int nrounds = (q0 + NW * 32) / 64;  // nkt/2, nkt always even
  // prologue: stage round 0 (two tiles) synchronously
  stage_rm<C, NW * 64>(kg, ldsK);
  stage_rm<C, NW * 64>(kg + 32 * C, ldsK + 32 * C);
  stage_tr<C, NW * 64>(vg, ldsVt, sv.r);
  stage_tr<C, NW * 64>(vg + (long)32 * sv.r, ldsVt + C * 32, sv.r);
  __syncthreads();
  __builtin_amdgcn_s_waitcnt(0);  // as in attn_fwd_kernel

  RmStage<C, NW * 64> kstA, kstB;
  TrStage<C, NW * 64> vstA, vstB;
  for (int rd = 0; rd < nrounds; ++rd) {
    const int buf = rd & 1;
    const bool pre = rd + 1 < nrounds;
    if (pre) {
      const long nb = (long)(rd + 1) * 64;
      kstA.load(kg + nb * C);
      kstB.load(kg + (nb + 32) * C);
      vstA.load(vg + nb * sv.r, sv.r);
      vstB.load(vg + (nb + 32) * sv.r, sv.r);
    }
    const int k0 = rd * 64;
    if (k0 <= qw0 + 31) {  // at least sub-tile A needed by this wave
      const u16* kbuf = ldsK + buf * 64 * C;
      const u16* vbuf = ldsVt + buf * 64 * C;  // (C*32 per sub-tile) x 2
      const bool needB = (k0 + 32) <= qw0 + 31;
      // S for both sub-tiles (independent MFMA chains)
      f32x16 s0 = (f32x16)(0.f), s1 = (f32x16)(0.f);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        bf16x8_t a0 = read_rm_frag<C>(kbuf, lane & 31, 16 * ch * 2 + 16 * (lane >> 5));
        s0 = mfma_32x32x16_bf16(a0, qf[ch], s0);
      }
      if (needB) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          bf16x8_t a1 = read_rm_frag<C>(kbuf + 32 * C, lane & 31,
                                        16 * ch * 2 + 16 * (lane >> 5));
          s1 = mfma_32x32x16_bf16(a1, qf[ch], s1);
        }
      }
      // merged mask + stats over up to 64 k
      float sv0[16], sv1[16];
      float mt = -1e30f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sv0[r] = (k0 + mfma_d_row(lane, r) > myq) ? -1e30f : s0[r];
        mt = fmaxf(mt, sv0[r]);
        sv1[r] = (!needB || k0 + 32 + mfma_d_row(lane, r) > myq) ? -1e30f : s1[r];
        mt = fmaxf(mt, sv1[r]);
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32));
      const float mn = fmaxf(m, mt);
      const float alpha = __expf((m - mn) * scale);
      const bool need_rescale = !__all(mt <= m);
      m = mn;
      float p0[16], p1[16], psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p0[r] = __expf((sv0[r] - mn) * scale);
        p1[r] = __expf((sv1[r] - mn) * scale);
        psum += p0[r] + p1[r];
      }
      psum += __shfl_xor(psum, 32);
      lsum = lsum * alpha + psum;
      if (need_rescale) {  // ONE rescale per 64 k
        float arow[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) arow[r] = shfl32(alpha, mfma_d_row(lane, r));
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[cb][r] *= arow[r];
      }
      // PV for both sub-tiles
      bf16x8_t pA0 = dlayout_to_afrag(p0);
      bf16x8_t pA1 = dlayout_to_afrag(p0 + 8);
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        bf16x8_t b0 = read_tr_frag(vbuf, 32 * cb + (lane & 31), 16 * (lane >> 5));
        bf16x8_t b1 = read_tr_frag(vbuf, 32 * cb + (lane & 31), 32 + 16 * (lane >> 5));
        oacc[cb] = mfma_32x32x16_bf16(pA0, b0, oacc[cb]);
        oacc[cb] = mfma_32x32x16_bf16(pA1, b1, oacc[cb]);
      }
      if (needB) {
        bf16x8_t pB0 = dlayout_to_afrag(p1);
        bf16x8_t pB1 = dlayout_to_afrag(p1 + 8);
        const u16* vbufB = vbuf + C * 32;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          bf16x8_t b0 = read_tr_frag(vbufB, 32 * cb + (lane & 31), 16 * (lane >> 5));
          bf16x8_t b1 = read_tr_frag(vbufB, 32 * cb + (lane & 31), 32 + 16 * (lane >> 5));
          oacc[cb] = mfma_32x32x16_bf16(pB0, b0, oacc[cb]);
          oacc[cb] = mfma_32x32x16_bf16(pB1, b1, oacc[cb]);
        }
      }
    }
    if (pre) {
      u16* kd = ldsK + (1 - buf) * 64 * C;
      u16* vd = ldsVt + (1 - buf) * 64 * C;
      kstA.write(kd);
      kstB.write(kd + 32 * C);
      vstA.write_tr(vd);
      vstB.write_tr(vd + C * 32);
    }
    __syncthreads();
  }

  // epilogue: identical to the single-tile kernel
  const float rec = 1.f / lsum;
  float rrow[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) rrow[r] = shfl32(rec, mfma_d_row(lane, r));
  if (lane < 32) lse[bh * T + myq] = m * scale + __logf(lsum);
  float* ob = obuf + w * 32 * 32;
  u16* og = o + bh_base(so, bh, H) + (long)qw0 * so.r;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mfma_d_row(lane, r);
      *(float*)((char*)ob + row * 128 + (((lane & 31) * 4) ^ ((row & 7) << 4))) =
          oacc[cb][r] * rrow[r];
    }
    __builtin_amdgcn_s_waitcnt(0);
    const int row = lane & 31;
    const int c16 = 16 * (lane >> 5);
    float tmp[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 t = *(const f32x4*)((char*)ob + row * 128 + (((c16 + 4 * i) * 4) ^ ((row & 7) << 4)));
      tmp[4 * i] = t[0]; tmp[4 * i + 1] = t[1]; tmp[4 * i + 2] = t[2]; tmp[4 * i + 3] = t[3];
    }
    u16x8 out0, out1;
#pragma unroll
    for (int j = 0; j < 8; ++j) { out0[j] = f2b(tmp[j]); out1[j] = f2b(tmp[8 + j]); }
    *(u16x8*)(og + (long)row * so.r + 32 * cb + c16) = out0;
    *(u16x8*)(og + (long)row * so.r + 32 * cb + c16 + 8) = out1;
    __builtin_amdgcn_s_waitcnt(0);
  }
}

// ===========================================================================
// delta = rowsum(dO * O) — 64/(C/8) rows per wave (prologue of backward)
// Unchanged under dropout: with O_i = sum_j P_ij Z_ij V_j (Z = keep/(1-p)),
// dO_i.O_i = sum_j P_ij Z_ij (dO_i.V_j) = sum_j P_ij dP_ij, dP = (dO V^T)oZ.
// ===========================================================================
// delta is (B,H,T) packed; dO and O are strided. bth_order: the rows are
// visited in (b,t,h) order, the memory order of (B,T,H,C) operands, instead
// of (b,h,t). do_copy != nullptr: dO is also written out as packed (B,H,T,C)
// on the way, for the dkv and dq kernels to stage from (their per-head tiles
// are then contiguous; read in place from (B,T,H,C), whose rows of one head
// lie H*C elements apart, both kernels measured 8-12% slower).
// A row is C/8 lanes of 16 bytes, so a wave takes 64/(C/8) consecutive rows
// at once and sums each within its own lane group.
template <int C>
__global__ void attn_delta_kernel(const u16* __restrict__ dO,
                                  const u16* __restrict__ O,
                                  float* __restrict__ delta, long N,
                                  int H, int T, AttnStrides sdo, AttnStrides so,
                                  u16* __restrict__ do_copy, int bth_order) {
  constexpr int LPR = C / 8;      // lanes per row
  constexpr int RPW = WAVE / LPR;  // rows per wave
  static_assert(LPR * 8 == C && RPW * LPR == WAVE, "C/8 must divide the wave");
  const int lane = lane_id();
  const int i = (lane % LPR) * 8;
  const long row0 =
      ((long)blockIdx.x * (blockDim.x / WAVE) + wave_id()) * RPW + lane / LPR;
  const long rstep = (long)gridDim.x * (blockDim.x / WAVE) * RPW;
  for (long row = row0; row < N; row += rstep) {
    // N < 2^31 (checked by the launcher): 32-bit divisions
    const unsigned urow = (unsigned)row;
    long bh, t;
    if (bth_order) {
      const unsigned bt = urow / (unsigned)H;
      t = bt % (unsigned)T;
      bh = (long)(bt / (unsigned)T) * H + urow % (unsigned)H;
    } else {
      bh = urow / (unsigned)T;
      t = urow % (unsigned)T;
    }
    const u16* dor = dO + bh_base(sdo, bh, H) + t * sdo.r;
    const u16* orow = O + bh_base(so, bh, H) + t * so.r;
    float acc = 0.f;
    const u16x8 a = *(const u16x8*)(dor + i);
    const u16x8 b = *(const u16x8*)(orow + i);
    if (do_copy) *(u16x8*)(do_copy + (bh * T + t) * C + i) = a;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += b2f(a[j]) * b2f(b[j]);
    // a row's lanes leave the loop together, so its group is whole here
    acc = group_sum<LPR>(acc);
    if (lane % LPR == 0) delta[bh * T + t] = acc;
  }
}

// ===========================================================================
// Backward, kernel A (dK/dV): one WG = NW*32 k rows (32/wave); iterates q
// tiles >= its diagonal with DOUBLE-BUFFERED staging (the tile qt+1 is
// staged while qt is computed, hiding the HBM load latency that a
// stage-barrier-compute structure exposes). dK/dV accumulate in registers.
// S and dS are recomputed from Q,K,LSE (standard flash recompute).
// ===========================================================================
//
// DROP (Z = keep/(1-p), philox.h): dV += (PoZ)^T dO, dP = (dO V^T)oZ,
// dS = P o (dP - delta) * scale. Registers 4g..4g+3 are four consecutive q
// (4-aligned) at this lane's k: one Philox call per register group. The
// 1/(1-p) of dV is applied once, in the epilogue.
// Whether the dkv kernel keeps its V fragments in LDS (NW*32*C bf16 behind
// the staging buffers). Not at C=128 with 4 waves: two such workgroups share
// a CU, and 96.5 KB each would leave room for one. There V is re-read from
// global (L2) in every tile.
template <int C, int NW>
constexpr bool attn_dkv_vf_lds = !(C == 128 && NW == 4);
// How many of a lane's C/16 K fragments sit in LDS behind them (the DROP
// kernel at C=128 keeps none resident and uses none of it).
template <int C, int NW>
constexpr int attn_dkv_kf_lds = C == 128 ? 3 : 0;

template <int C, int NW, bool DROP = false>
__global__ __launch_bounds__(NW * 64, 2) void attn_bwd_dkv_kernel(
    const u16* __restrict__ dO, const u16* __restrict__ q,
    const u16* __restrict__ k, const u16* __restrict__ v,
    const float* __restrict__ lse, const float* __restrict__ delta,
    u16* __restrict__ dk, u16* __restrict__ dv, int B, int H, int T,
    AttnStrides sdo, AttnStrides sv, AttnStrides sdv,
    uint32_t seed_lo = 0, uint32_t seed_hi = 0, uint32_t drop_thr = 0,
    float inv_keep = 1.f) {
  constexpr int NCB = C / 32;
  constexpr int NCH = C / 16;
  constexpr int TILE = 4 * 32 * C;  // u16 elems per buffer set (Q,Qt,dO,dOt)
  const float scale = rsqrtf((float)C);
  const long bh = blockIdx.x % ((long)B * H);
  const int kb = blockIdx.x / (B * H);
  const int lane = lane_id();
  const int w = wave_id();
  const int kw0 = kb * (NW * 32) + 32 * w;
  const int myk = kw0 + (lane & 31);

  extern __shared__ __attribute__((aligned(16))) char smem[];
  u16* base = (u16*)smem;                       // [2][TILE]
  float* ldsLse = (float*)(base + 2 * TILE);    // [2][32]
  float* ldsDelta = ldsLse + 64;                // [2][32]
  // V fragments of this wave's 32 keys, constant over the q loop: each lane
  // parks its own NCH fragments here once and reads back only those, so no
  // barrier guards them and a 16-byte read per lane is conflict-free.
  constexpr bool VF_LDS = attn_dkv_vf_lds<C, NW>;
  bf16x8_t* ldsVf = (bf16x8_t*)(ldsDelta + 64) + w * (NCH * 64) + lane;

  const u16* qg = q + (bh * T) * C;
  const u16* kg = k + (bh * T) * C;
  const u16* vg = v + bh_base(sv, bh, H);
  const u16* dog = dO + bh_base(sdo, bh, H);
  const u16* krow = kg + (long)myk * C;
  const unsigned vrow_off = 2u * (unsigned)(myk * sv.r + 8 * (lane >> 5));  // bytes
  if constexpr (VF_LDS) {
    const u16* vrow = vg + (long)myk * sv.r;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
      ldsVf[ch * 64] = *(const bf16x8_t*)(vrow + 16 * ch + 8 * (lane >> 5));
  }

  // K row fragments resident in registers (the L2 re-read variant was
  // measured -20% on dkv C=128 in a full-step profile despite removing
  // the 2-VGPR spill — the per-tile global loads add latency the spill
  // never cost).
  // Under DROP at C=128 the keep mask and its select/scale code do not
  // fit beside 32 VGPRs of resident K (the DROP=false kernel sits at the
  // 256 cap), so that variant re-reads K too.
  constexpr bool KF_RES = !(DROP && C == 128);
  // At C=128 the last NKL of them are parked in LDS behind V in the same
  // way: with the next tile's Q and dO held in registers across the compute
  // phase, all NCH beside the 128 accumulators spill, and a scratch reload
  // in the loop waits for the prefetch with it.
  constexpr int NKL = KF_RES ? attn_dkv_kf_lds<C, NW> : 0;
  constexpr int NKR = KF_RES ? NCH - NKL : 0;
  bf16x8_t kf[NKR ? NKR : 1];
  bf16x8_t* ldsKf = (bf16x8_t*)(ldsDelta + 64) + (VF_LDS ? NW * (NCH * 64) : 0) +
                    w * (NKL * 64) + lane;
  if (KF_RES) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const bf16x8_t f = *(const bf16x8_t*)(krow + 16 * ch + 8 * (lane >> 5));
      if (ch < NKR) kf[ch < NKR ? ch : 0] = f;
      else ldsKf[(ch - NKR) * 64] = f;
    }
  }

  f32x16 dvacc[NCB], dkacc[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) { dvacc[cb] = (f32x16)(0.f); dkacc[cb] = (f32x16)(0.f); }

  const int qt0 = kb * NW;  // diagonal q tile
  const int nqt = T / 32;

  auto stage_set = [&](int qt, int buf) {
    const long qbase = (long)qt * 32;
    u16* bq = base + buf * TILE;
    stage_rm<C, NW * 64>(qg + qbase * C, bq);
    stage_tr<C, NW * 64, true>(qg + qbase * C, bq + 32 * C);
    stage_rm<C, NW * 64>(dog + qbase * sdo.r, bq + 2 * 32 * C, sdo.r);
    stage_tr<C, NW * 64, true>(dog + qbase * sdo.r, bq + 3 * 32 * C, sdo.r);
    if (threadIdx.x < 32) {
      ldsLse[buf * 32 + threadIdx.x] = lse[bh * T + qbase + threadIdx.x];
      ldsDelta[buf * 32 + threadIdx.x] = delta[bh * T + qbase + threadIdx.x];
    }
  };

  stage_set(qt0, 0);
  __syncthreads();
  // Every prologue load has landed: said outright, so that the vmcnt waits
  // inside the loop count its own prefetch alone and none of them stands
  // before the compute phase on account of a load from up here.
  __builtin_amdgcn_s_waitcnt(0);
  TrStage<C, NW * 64, true> qst, dost;  // ONE load feeds both rm and tr images
  float lse_r = 0.f, del_r = 0.f;
  for (int qt = qt0; qt < nqt; ++qt) {
    const int buf = (qt - qt0) & 1;
    const bool pre = qt + 1 < nqt;
    if (pre) {  // T14 split: loads early
      const long nb = (long)(qt + 1) * 32;
      qst.load(qg + nb * C);
      dost.load(dog + nb * sdo.r, sdo.r);
      if (threadIdx.x < 32) {
        unsigned off = 4u * threadIdx.x;  // opaque, as in TrStage::load
        asm volatile("" : "+v"(off));
        lse_r = *(const float*)((const char*)(lse + bh * T + nb) + off);
        del_r = *(const float*)((const char*)(delta + bh * T + nb) + off);
      }
    }
    const int qbase = qt * 32;
    if (qbase + 31 >= kw0) {  // not fully masked for this wave
      const u16* ldsQ = base + buf * TILE;
      const u16* ldsQt = ldsQ + 32 * C;
      const u16* ldsDO = ldsQt + C * 32;
      const u16* ldsDOt = ldsDO + 32 * C;
      const float* lseb = ldsLse + buf * 32;
      const float* deltab = ldsDelta + buf * 32;
      // DROP: bit r = keep(q of reg r, myk). Evaluated before the MFMA
      // phase, while s/dp/p/ds are dead, and fenced so the Philox
      // temporaries never overlap them (the kernel sits at the VGPR cap).
      uint32_t keep = 0;
      if constexpr (DROP) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          keep |= attn_drop_keep4(seed_lo, seed_hi, (uint32_t)bh,
                                  (uint32_t)(qbase + 8 * g + 4 * (lane >> 5)) >> 2,
                                  (uint32_t)myk, drop_thr) << (4 * g);
        __builtin_amdgcn_sched_barrier(0);
      }
      // Registers 4g..4g+3 are q rows 8g + 4h .. +3 (h = lane>>5): the
      // tile's LSE and delta come as four 16-byte reads each.
      // S = Q x K^T (D rows = q regs, cols = k lanes)
      f32x16 s = (f32x16)(0.f);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        bf16x8_t a = read_rm_frag<C>(ldsQ, lane & 31, 16 * ch * 2 + 16 * (lane >> 5));
        bf16x8_t kfr;
        if constexpr (!KF_RES) kfr = *(const bf16x8_t*)(krow + 16 * ch + 8 * (lane >> 5));
        else if (ch < NKR) kfr = kf[ch < NKR ? ch : 0];
        else kfr = ldsKf[(ch - NKR) * 64];
        s = mfma_32x32x16_bf16(a, kfr, s);
      }
      float p[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 l4 = *(const f32x4*)(lseb + 8 * g + 4 * (lane >> 5));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * g + i;
          const int qrow = qbase + mfma_d_row(lane, r);
          p[r] = (myk > qrow) ? 0.f : __expf(s[r] * scale - l4[i]);
        }
      }
      // dV += P^T x dO. P^T x B sums over P's register (q) index: packed
      // pairwise P is the A operand as it stands, against a dOt image whose
      // q positions follow acc_k_pos. The same holds for dS and Qt below.
      bf16x8_t pf0 = dlayout_pack(p, DROP ? keep : 0xffu);
      bf16x8_t pf1 = dlayout_pack(p + 8, DROP ? keep >> 8 : 0xffu);
      // Formed here, and the phases kept in this order: the pack is a few
      // pure instructions that would otherwise be placed behind the dP
      // phase with all dOt fragments read ahead of it, and at C=128 the
      // resident K fragments then spill into the loop (a sched_barrier
      // alone does not hold a pure value). Likewise for dS below.
      asm volatile("" : "+v"(pf0), "+v"(pf1));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        bf16x8_t b0 = read_tr_frag(ldsDOt, 32 * cb + (lane & 31), 16 * (lane >> 5));
        bf16x8_t b1 = read_tr_frag(ldsDOt, 32 * cb + (lane & 31), 32 + 16 * (lane >> 5));
        dvacc[cb] = mfma_32x32x16_bf16(pf0, b0, dvacc[cb]);
        dvacc[cb] = mfma_32x32x16_bf16(pf1, b1, dvacc[cb]);
      }
      // dP = dO x V^T
      f32x16 dp = (f32x16)(0.f);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        bf16x8_t a = read_rm_frag<C>(ldsDO, lane & 31, 16 * ch * 2 + 16 * (lane >> 5));
        bf16x8_t vf;
        if constexpr (VF_LDS) {
          vf = ldsVf[ch * 64];
        } else {
          // wave-uniform base plus a 32-bit lane offset, as in TrStage::load
          unsigned off = vrow_off;
          asm volatile("" : "+v"(off));
          vf = *(const bf16x8_t*)((const char*)vg + off + 32 * ch);
        }
        dp = mfma_32x32x16_bf16(a, vf, dp);
      }
      // dS = P * (dP - delta[q]) * scale
      float ds[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 d4 = *(const f32x4*)(deltab + 8 * g + 4 * (lane >> 5));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * g + i;
          float dpr = dp[r];
          if constexpr (DROP) dpr = ((keep >> r) & 1u) ? dpr * inv_keep : 0.f;
          ds[r] = p[r] * (dpr - d4[i]) * scale;
        }
      }
      bf16x8_t df0 = dlayout_pack(ds);
      bf16x8_t df1 = dlayout_pack(ds + 8);
      asm volatile("" : "+v"(df0), "+v"(df1));
      __builtin_amdgcn_sched_barrier(0);
      // dK += dS^T x Q
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        bf16x8_t b0 = read_tr_frag(ldsQt, 32 * cb + (lane & 31), 16 * (lane >> 5));
        bf16x8_t b1 = read_tr_frag(ldsQt, 32 * cb + (lane & 31), 32 + 16 * (lane >> 5));
        dkacc[cb] = mfma_32x32x16_bf16(df0, b0, dkacc[cb]);
        dkacc[cb] = mfma_32x32x16_bf16(df1, b1, dkacc[cb]);
      }
    }
    if (pre) {  // writes late
      u16* bq = base + (buf ^ 1) * TILE;
      qst.write_rm(bq);
      qst.write_tr(bq + 32 * C);
      dost.write_rm(bq + 2 * 32 * C);
      dost.write_tr(bq + 3 * 32 * C);
      if (threadIdx.x < 32) {
        ldsLse[(buf ^ 1) * 32 + threadIdx.x] = lse_r;
        ldsDelta[(buf ^ 1) * 32 + threadIdx.x] = del_r;
      }
    }
    __syncthreads();
  }

  // epilogue: LDS bounce -> wide bf16 stores (reuses the staging region)
  float* ob = (float*)smem + w * 32 * 32;
  u16* dkg = dk + (bh * T + kw0) * C;
  u16* dvg = dv + bh_base(sdv, bh, H) + (long)kw0 * sdv.r;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    f32x16* acc = which == 0 ? dkacc : dvacc;
    u16* out = which == 0 ? dkg : dvg;
    const int old = which == 0 ? C : sdv.r;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mfma_d_row(lane, r);
        float a = acc[cb][r];
        if constexpr (DROP) { if (which == 1) a *= inv_keep; }
        *(float*)((char*)ob + row * 128 + (((lane & 31) * 4) ^ ((row & 7) << 4))) = a;
      }
      __builtin_amdgcn_s_waitcnt(0);
      const int row = lane & 31;
      const int c16 = 16 * (lane >> 5);
      float tmp[16];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 t = *(const f32x4*)((char*)ob + row * 128 +
                                  (((c16 + 4 * i) * 4) ^ ((row & 7) << 4)));
        tmp[4 * i] = t[0]; tmp[4 * i + 1] = t[1];
        tmp[4 * i + 2] = t[2]; tmp[4 * i + 3] = t[3];
      }
      u16x8 o0, o1;
#pragma unroll
      for (int j = 0; j < 8; ++j) { o0[j] = f2b(tmp[j]); o1[j] = f2b(tmp[8 + j]); }
      *(u16x8*)(out + (long)row * old + 32 * cb + c16) = o0;
      *(u16x8*)(out + (long)row * old + 32 * cb + c16 + 8) = o1;
      __builtin_amdgcn_s_waitcnt(0);
    }
  }
}

// ===========================================================================
// Backward, kernel B (dQ): SPW mirrored q strips per wave (work balance,
// see forward); iterates k tiles up to the max diagonal, DOUBLE-BUFFERED.
// dQ accumulates in registers — no atomics.
// ===========================================================================
// DROP: same dP = (dO V^T)oZ and dS as the dkv kernel; registers 4g..4g+3
// are four consecutive q at this lane's k, one Philox call per group.
template <int C, int NW, int SPW, bool DROP = false>
__global__ __launch_bounds__(NW * 64, 2) void attn_bwd_dq_kernel(
    const u16* __restrict__ dO, const u16* __restrict__ q,
    const u16* __restrict__ k, const u16* __restrict__ v,
    const float* __restrict__ lse, const float* __restrict__ delta,
    u16* __restrict__ dq, int B, int H, int T,
    AttnStrides sdo, AttnStrides sv,
    uint32_t seed_lo = 0, uint32_t seed_hi = 0, uint32_t drop_thr = 0,
    float inv_keep = 1.f) {
  constexpr int NCB = C / 32;
  constexpr int NCH = C / 16;
  constexpr int NSTRIP = NW * SPW;
  constexpr int TILE = 3 * 32 * C;  // u16 elems per buffer set (K, V, Kt)
  const float scale = rsqrtf((float)C);
  const long bh = blockIdx.x % ((long)B * H);
  const int qb = blockIdx.x / (B * H);
  const int q0 = qb * (NSTRIP * 32);
  const int lane = lane_id();
  const int w = wave_id();
  int strip[SPW];
  strip[0] = w;
  if (SPW == 2) strip[1] = NSTRIP - 1 - w;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  u16* base = (u16*)smem;               // [2][TILE] = K rm | V rm | Kt
  // dO fragments of this wave's strips, constant over the k loop: each lane
  // parks its own SPW*NCH fragments here once and reads back only those, so
  // no barrier guards them and a 16-byte read per lane is conflict-free.
  bf16x8_t* ldsDOf = (bf16x8_t*)(base + 2 * TILE) + w * (SPW * NCH * 64) + lane;

  const u16* qg = q + (bh * T) * C;
  const u16* kg = k + (bh * T) * C;
  const u16* vg = v + bh_base(sv, bh, H);
  const u16* dog = dO + bh_base(sdo, bh, H);

  // Under DROP at C=128 that variant re-reads Q from global (L2-resident)
  // like the non-last strips do. (Decided when the DROP=false kernel used
  // 255 of 256 VGPRs; it uses 193 now, so resident Q may fit there too.)
  constexpr bool QF_RES = !(DROP && C == 128);
  bf16x8_t qf[QF_RES ? NCH : 1];  // registers only for the last (busiest) strip
  f32x16 dqacc[SPW][NCB];
  float mylse[SPW], mydelta[SPW];
#pragma unroll
  for (int sp = 0; sp < SPW; ++sp) {
    const long myq = q0 + 32 * strip[sp] + (lane & 31);
    if (QF_RES && sp == SPW - 1) {
      const u16* qrow = qg + myq * C;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
        qf[ch] = *(const bf16x8_t*)(qrow + 16 * ch + 8 * (lane >> 5));
    }
    const u16* dorow = dog + myq * sdo.r;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
      ldsDOf[(sp * NCH + ch) * 64] = *(const bf16x8_t*)(dorow + 16 * ch + 8 * (lane >> 5));
    mylse[sp] = lse[bh * T + myq];
    mydelta[sp] = delta[bh * T + myq];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) dqacc[sp][cb] = (f32x16)(0.f);
  }

  const int nkt = (q0 + NSTRIP * 32) / 32;
  auto stage_set = [&](int kt, int buf) {
    const long k0 = (long)kt * 32;
    u16* bk = base + buf * TILE;
    stage_rm<C, NW * 64>(kg + k0 * C, bk);
    stage_rm<C, NW * 64>(vg + k0 * sv.r, bk + 32 * C, sv.r);
    stage_tr<C, NW * 64, true>(kg + k0 * C, bk + 2 * 32 * C);
  };
  stage_set(0, 0);
  __syncthreads();
  __builtin_amdgcn_s_waitcnt(0);  // as in the dkv kernel
  TrStage<C, NW * 64, true> kst;  // ONE load feeds K rm + Kt images
  RmStage<C, NW * 64> vst;
  for (int kt = 0; kt < nkt; ++kt) {
    const int buf = kt & 1;
    const bool pre = kt + 1 < nkt;
    if (pre) {
      kst.load(kg + (long)(kt + 1) * 32 * C);
      vst.load(vg + (long)(kt + 1) * 32 * sv.r, sv.r);
    }
    const int k0 = kt * 32;
    const u16* ldsK = base + buf * TILE;
    const u16* ldsV = ldsK + 32 * C;
    const u16* ldsKt = ldsV + 32 * C;
#pragma unroll
    for (int sp = 0; sp < SPW; ++sp) {
      const int qw0 = q0 + 32 * strip[sp];
      if (k0 > qw0 + 31) continue;
      const int myq = qw0 + (lane & 31);
      const u16* qrow = qg + (long)myq * C;
      // DROP: bit r = keep(myq, k of reg r). The mask groups four
      // consecutive q at one k into one Philox call; here registers run
      // along k at ONE q, and the four lanes of a quad hold q = 4g..4g+3
      // at the same 16 k (as in attn_fwd_kernel): quad lane j evaluates the
      // calls of registers 4j..4j+3, and every lane picks its own q's bit
      // out of the four quad masks. Evaluated before the MFMA phase, while
      // s/dp/ds are dead, and fenced so the Philox temporaries never
      // overlap them.
      uint32_t keep = 0;
      if constexpr (DROP) {
        const int j = lane & 3;
        uint32_t mine = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          mine |= attn_drop_keep4(seed_lo, seed_hi, (uint32_t)bh, (uint32_t)myq >> 2,
                                  (uint32_t)(k0 + c + 8 * j + 4 * (lane >> 5)),
                                  drop_thr) << (4 * c);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint32_t mg = (uint32_t)__shfl((int)mine, g, 4);
#pragma unroll
          for (int c = 0; c < 4; ++c) keep |= ((mg >> (4 * c + j)) & 1u) << (4 * g + c);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // S^T = K x Q^T and dP^T = V x dO^T in one pass: the key in the
      // registers (mfma_d_row), the query on the lane.
      f32x16 s = (f32x16)(0.f);
      f32x16 dp = (f32x16)(0.f);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        bf16x8_t kfrag = read_rm_frag<C>(ldsK, lane & 31, 16 * ch * 2 + 16 * (lane >> 5));
        bf16x8_t qfr = (QF_RES && sp == SPW - 1) ? qf[QF_RES ? ch : 0]
            : *(const bf16x8_t*)(qrow + 16 * ch + 8 * (lane >> 5));
        s = mfma_32x32x16_bf16(kfrag, qfr, s);
        bf16x8_t vfrag = read_rm_frag<C>(ldsV, lane & 31, 16 * ch * 2 + 16 * (lane >> 5));
        dp = mfma_32x32x16_bf16(vfrag, ldsDOf[(sp * NCH + ch) * 64], dp);
      }
      // LSE and delta of this lane's q are its own scalars.
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int krow = k0 + mfma_d_row(lane, r);
        float pv = (krow > myq) ? 0.f : __expf(s[r] * scale - mylse[sp]);
        float dpr = dp[r];
        if constexpr (DROP) dpr = ((keep >> r) & 1u) ? dpr * inv_keep : 0.f;
        ds[r] = pv * (dpr - mydelta[sp]) * scale;
      }
      // dQ += dS x K sums over dS^T's register (k) index: packed pairwise
      // it is the A operand as it stands, against a Kt image whose k
      // positions follow acc_k_pos.
      const bf16x8_t a0 = dlayout_pack(ds), a1 = dlayout_pack(ds + 8);
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        bf16x8_t b0 = read_tr_frag(ldsKt, 32 * cb + (lane & 31), 16 * (lane >> 5));
        bf16x8_t b1 = read_tr_frag(ldsKt, 32 * cb + (lane & 31), 32 + 16 * (lane >> 5));
        dqacc[sp][cb] = mfma_32x32x16_bf16(a0, b0, dqacc[sp][cb]);
        dqacc[sp][cb] = mfma_32x32x16_bf16(a1, b1, dqacc[sp][cb]);
      }
    }
    if (pre) {
      u16* bk = base + (buf ^ 1) * TILE;
      kst.write_rm(bk);
      vst.write(bk + 32 * C);
      kst.write_tr(bk + 2 * 32 * C);
    }
    __syncthreads();
  }

  // epilogue: LDS bounce -> wide stores (per strip)
#pragma unroll
  for (int sp = 0; sp < SPW; ++sp) {
    const int qw0 = q0 + 32 * strip[sp];
    float* ob = (float*)smem + w * 32 * 32;
    u16* dqg = dq + (bh * T + qw0) * C;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mfma_d_row(lane, r);
        *(float*)((char*)ob + row * 128 + (((lane & 31) * 4) ^ ((row & 7) << 4))) =
            dqacc[sp][cb][r];
      }
      __builtin_amdgcn_s_waitcnt(0);
      const int row = lane & 31;
      const int c16 = 16 * (lane >> 5);
      float tmp[16];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 t = *(const f32x4*)((char*)ob + row * 128 +
                                  (((c16 + 4 * i) * 4) ^ ((row & 7) << 4)));
        tmp[4 * i] = t[0]; tmp[4 * i + 1] = t[1];
        tmp[4 * i + 2] = t[2]; tmp[4 * i + 3] = t[3];
      }
      u16x8 o0, o1;
#pragma unroll
      for (int j = 0; j < 8; ++j) { o0[j] = f2b(tmp[j]); o1[j] = f2b(tmp[8 + j]); }
      *(u16x8*)(dqg + (long)row * C + 32 * cb + c16) = o0;
      *(u16x8*)(dqg + (long)row * C + 32 * cb + c16 + 8) = o1;
      __builtin_amdgcn_s_waitcnt(0);
    }
  }
}
