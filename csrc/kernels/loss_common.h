// The scaffold of the label-free loss kernels (unsup.hip, census.hip, selfsup.hip): a block handles
// ITERS iterations (grid.y over the groups), every thread carries Q accumulators, and the block's
// sums leave as one 16-byte row part[block][i][4] per iteration.  No atomics: the order of every sum
// is fixed (thread -> wave by shuffles -> the block's 4 waves in LDS, added as ((r0 + r1) + r2) + r3),
// so the partials are bitwise repeatable.
//
// A file's floating-point contraction state holds for what it includes from here: selfsup.hip
// switches contraction off *above* this header, unsup.hip and census.hip compile it contracted.
#pragma once
#include "common.h"

namespace loss {

constexpr int ITERS = 4;      // iterations per block
constexpr int MAX_N = 32;     // iterations per call
constexpr int BLOCK = 256;    // threads per block: 4 waves
constexpr int GRID_X = 1024;  // blocks per iteration group of a grid-stride loss kernel

// What every host entry refuses: P = B * H * W pixels must fit an int32 (a block then counts at most
// 2^31 / GRID_X pixels, which fp32 holds exactly).
inline bool sizes_ok(int B, int H, int W, int N) {
  return B >= 1 && H >= 1 && W >= 1 && N >= 1 && N <= MAX_N && (long)B * H * W <= 0x7fffffffL;
}
inline unsigned iter_groups(int N) { return (unsigned)((N + ITERS - 1) / ITERS); }

// The robust penalty and its derivative; e2 = eps^2.
JR_DEVICE float rho(float d, float e2) { return sqrtf(d * d + e2); }
JR_DEVICE float drho(float d, float e2) { return d / sqrtf(d * d + e2); }

// The landing point (px, py) lies in the frame; NaN fails.  A macro: a function is simplified to four
// unconditional compares before it is inlined, and the early return of unsup.hip's landing then
// compiles to other code than the expression written in place.
#define JR_INSIDE_FRAME(px, py, H, W) \
  ((px) >= 0.f && (px) <= (float)((W) - 1) && (py) >= 0.f && (py) <= (float)((H) - 1))

// Every accumulator summed over each wave into red[q][wave]; ends in the barrier.  Rows may be wider
// than the 4 words used.
template <int Q, int RW>
JR_DEVICE void block_sums(const float (&acc)[Q], float (&red)[Q][RW]) {
  static_assert(RW >= BLOCK / 64, "one word per wave");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    float v = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[k][wave] = v;
  }
  __syncthreads();
}
template <int RW>
JR_DEVICE float row_total(const float (&r)[RW]) { return ((r[0] + r[1]) + r[2]) + r[3]; }

// The epilogue of an iteration group that starts at i0: thread k < ITERS owns iteration i = i0 + k (where
// that is below N) and stores its four sums as the 16-byte row part[blockIdx.x][i].
JR_DEVICE bool owns_row(int i0, int N, int& k, int& i) {
  if (!(threadIdx.x < ITERS && i0 + (int)threadIdx.x < N)) return false;
  k = threadIdx.x;
  i = i0 + k;
  return true;
}
JR_DEVICE void store_row(float* part, int N, int i, float x, float y, float z, float w) {
  *(float4*)(part + 4 * ((long)blockIdx.x * N + i)) = make_float4(x, y, z, w);
}

}  // namespace loss
