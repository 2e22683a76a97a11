// Batched 2-D transpose of bf16 matrices that live at offsets of one flat
// buffer, into images at offsets of another: one launch for every matrix of a
// table. The training engine keeps W^T beside each Linear's W this way, so
// that the dgrad GEMM dx = dy W runs in the forward's TN layout.
//
// Table: n_mat rows of 5 int64 {src offset, dst offset, rows, cols, tiles
// before this matrix}, offsets in elements. Matrix m is rows x cols row-major
// at src + src offset; its image is cols x rows row-major at dst + dst offset.
// A workgroup of 256 takes 64x64 tiles, grid-stride over the tiles of all the
// matrices, and finds a tile's matrix by bisection on the prefix column.
//
// LDS tile: 64 rows of 33 dwords (66 bf16). The odd dword stride makes both
// sides conflict-free under the 32-bank rule of the dword writes (the compiler
// pairs them into ds_write2_b32) and of ds_read_u16:
//   write: lane -> (row = lane/8, 16-byte chunk v = lane%8), four dwords at
//     row*33 + 4v + k. A 32-lane group holds 4 rows x 8 chunks: banks
//     (row + 4v + k) % 32 are 32 different ones.
//   read:  lane -> (image row c, chunk j of 8 source rows); element i comes
//     from dword (8j+i)*33 + c/2. A 32-lane group holds 8 image rows x 4
//     chunks j0..j0+3: banks 8j + c/2 + const, 16 different ones, each read by
//     the two lanes of one dword (a broadcast).
// The vector path (16-byte global loads and stores) needs a full tile and
// every row start of tile and image 16-byte aligned; ragged edge tiles and
// unaligned offsets take the scalar path through the same LDS tile.
#include "common.h"

#define TR_TILE 64
#define TR_STRIDE_W 33              // dwords per LDS row
#define TR_STRIDE (2 * TR_STRIDE_W) // bf16 per LDS row
#define TR_COLS 5                   // int64 per table row

__global__ __launch_bounds__(256) void transpose_batched_kernel(
    const u16* __restrict__ src, u16* __restrict__ dst, const long* __restrict__ tab,
    int n_mat, long n_tiles) {
  __shared__ unsigned tile_w[TR_TILE * TR_STRIDE_W];
  u16* tile = reinterpret_cast<u16*>(tile_w);
  const int tid = threadIdx.x;

  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    // the last matrix whose first tile is <= t
    int lo = 0, hi = n_mat - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tab[mid * TR_COLS + 4] <= t) lo = mid;
      else hi = mid - 1;
    }
    const long* e = tab + lo * TR_COLS;
    const long rows = e[2], cols = e[3];
    const long local = t - e[4];
    const long tiles_c = (cols + TR_TILE - 1) / TR_TILE;
    const long r0 = (local / tiles_c) * TR_TILE, c0 = (local % tiles_c) * TR_TILE;
    const u16* s = src + e[0] + r0 * cols + c0;  // tile origin in the matrix
    u16* d = dst + e[1] + c0 * rows + r0;        // and in the image
    const bool vec = r0 + TR_TILE <= rows && c0 + TR_TILE <= cols && rows % 8 == 0 &&
                     cols % 8 == 0 && reinterpret_cast<uintptr_t>(s) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(d) % 16 == 0;
    if (vec) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int idx = tid + p * 256;
        const int r = idx >> 3, v = idx & 7;
        const u16x8 x = *reinterpret_cast<const u16x8*>(s + r * cols + v * 8);
        unsigned* w = tile_w + r * TR_STRIDE_W + v * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = (unsigned)x[2 * k] | ((unsigned)x[2 * k + 1] << 16);
      }
      __syncthreads();
      const int lane = tid & 63, wave = tid >> 6;
      const int j = (lane >> 5) * 4 + (lane & 3);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int c = p * 32 + wave * 8 + ((lane >> 2) & 7);
        u16x8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = tile[(8 * j + i) * TR_STRIDE + c];
        *reinterpret_cast<u16x8*>(d + c * rows + 8 * j) = o;
      }
    } else {
      const int nr = (int)min((long)TR_TILE, rows - r0), nc = (int)min((long)TR_TILE, cols - c0);
      for (int idx = tid; idx < TR_TILE * TR_TILE; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        if (r < nr && c < nc) tile[r * TR_STRIDE + c] = s[r * cols + c];
      }
      __syncthreads();
      for (int idx = tid; idx < TR_TILE * TR_TILE; idx += 256) {
        const int c = idx >> 6, r = idx & 63;
        if (r < nr && c < nc) d[c * rows + r] = tile[r * TR_STRIDE + c];
      }
    }
    __syncthreads();  // the tile is free for the next trip
  }
}
