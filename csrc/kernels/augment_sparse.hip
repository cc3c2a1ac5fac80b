// RAFT's sparse flow augmentation (KITTI / HD1K: photometric jitter, eraser, one scale, flips,
// crop) over frames of several sizes: every sample sits in the top-left corner of a
// [Hb][Wb] buffer and carries its own size (Hs, Ws) in its record.  The semantics are the
// golden op's (train/augment.py:augment_pairs_sparse) and the kernels equal it bit for bit;
// contraction is off, there are no float atomics.
// The images are the dense gather (augment_common.h) with per-sample sizes and the buffer's
// pitch.  The flow cannot be interpolated: the golden op moves it point by point, a forward
// scatter in which the source pixel with the largest linear index wins a cell.  The kernel
// inverts that map per output cell: it scans the candidate source rows from the highest down
// and in each the candidate columns from the highest down, evaluates the forward predicate
// rint(fp32(xs) * isx) == X itself on each, and takes the first candidate whose valid byte is
// set -- the largest linear index, so no atomics, no memset and no winner plane.
// Two launches:
//   1. colour sums over each sample's own region (padding bytes never enter);
//   2. the gather: grid (runs of a row, rows, samples), one thread per 4 consecutive pixels of a
//      row, the sample's 52-word record wave-uniform, 16-byte stores.
#include "augment_common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

using namespace augment_dev;

// record layout (train/augment.py:SparseAugmentParams): the dense record's 16 ints, the sample's
// own size, two spare words, then the dense record's 32 floats
constexpr int REC_WORDS = 52, I_HS = 16, I_WS = 17, F_BASE = 20;
constexpr int SUM_PIX = 16;     // pixels per thread of the sums kernel

// The sample's size as the kernels use it: inside the buffer whatever the record says.
JR_DEVICE void sample_size(const int* __restrict__ rec, int Hb, int Wb, int& Hs, int& Ws) {
  Hs = min(max(rec[I_HS], 1), Hb);
  Ws = min(max(rec[I_WS], 1), Wb);
}

// sums int32 [2][B][3]; grid (blocks per buffer, 2 * B).  Pixel p of a sample is (p / Ws, p % Ws).
__global__ __launch_bounds__(256) void augment_sparse_sums_kernel(const unsigned char* __restrict__ i1,
                                                                  const unsigned char* __restrict__ i2,
                                                                  const int* __restrict__ params, int B, int Hb, int Wb,
                                                                  int* __restrict__ sums) {
  __shared__ int part[4][3];
  const int n = blockIdx.y, smp = n < B ? n : n - B;
  int Hs, Ws;
  sample_size(params + smp * REC_WORDS, Hb, Wb, Hs, Ws);
  const int npix = Hs * Ws;
  if ((int)blockIdx.x * (256 * SUM_PIX) >= npix) return;   // block-uniform: a sample smaller than the buffer
  const unsigned char* img = (n < B ? i1 : i2) + (long)smp * Hb * Wb * 3;
  const int base = blockIdx.x * (256 * SUM_PIX) + threadIdx.x;
  int s[3] = {0, 0, 0};
#pragma unroll 4
  for (int k = 0; k < SUM_PIX; ++k) {
    const int p = base + k * 256;
    if (p < npix) {
      const int row = (int)((unsigned)p / (unsigned)Ws);
      const unsigned char* px = img + ((long)row * Wb + (p - row * Ws)) * 3;
      s[0] += px[0]; s[1] += px[1]; s[2] += px[2];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[c] += __shfl_down(s[c], off, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[wave][0] = s[0]; part[wave][1] = s[1]; part[wave][2] = s[2]; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    atomicAdd(sums + n * 3 + c, (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]));
  }
}

// grid: (ceil(ceil(w / 4) / 64), ceil(h / 4), B), block (64, 4): thread = 4 pixels of one row
__global__ __launch_bounds__(256) void augment_sparse_kernel(
    const unsigned char* __restrict__ i1, const unsigned char* __restrict__ i2, const float* __restrict__ flow,
    const unsigned char* __restrict__ valid, const int* __restrict__ params, const int* __restrict__ sums,
    float* __restrict__ o1, float* __restrict__ o2, float* __restrict__ oflow, float* __restrict__ ovalid, int B, int Hb,
    int Wb, int h, int w) {
  const int n = blockIdx.z;
  const int y = blockIdx.y * 4 + threadIdx.y;
  const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4;
  if (y >= h || x4 >= w) return;
  const int* rec = params + n * REC_WORDS;                  // wave-uniform: scalar loads
  const float* recf = (const float*)(rec + F_BASE);
  int Hs, Ws;
  sample_size(rec, Hb, Wb, Hs, Ws);
  const int npix = Hs * Ws;
  const int Hr = rec[I_HR], Wr = rec[I_WR], y0 = rec[I_Y0], x0 = rec[I_X0];
  const bool hflip = rec[I_HFLIP] != 0, vflip = rec[I_VFLIP] != 0;
  const int nrect = rec[I_NRECT];
  const float sx = recf[F_SX], sy = recf[F_SY], isx = recf[F_ISX], isy = recf[F_ISY];
  const Colour c1 = load_colour(recf + F_COL1, sums + n * 3, npix);
  const Colour c2 = load_colour(recf + F_COL2, sums + (B + n) * 3, npix);

  int v = y + y0, y_lo, y_hi;                               // v: the cell's row Y before flips
  if (vflip) v = Hr - 1 - v;
  float wy;
  source_pos(v, sy, Hs, y_lo, y_hi, wy);
  const long frame = (long)n * Hb * Wb;
  const unsigned char* p1 = i1 + frame * 3;
  const unsigned char* p2 = i2 + frame * 3;
  const float* pf = flow + frame * 2;
  const unsigned char* pv = valid + frame;
  int ys_lo, ys_hi;
  scan_window(v, sy, Hs, ys_lo, ys_hi);

  float a1[12], a2[12], fl[8], va[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = min(x4 + k, w - 1);   // the tail of a width that is no multiple of 4 repeats its last pixel (not stored)
    int u = x + x0, x_lo, x_hi;         // u: the cell's column X before flips
    if (hflip) u = Wr - 1 - u;
    float wx;
    source_pos(u, sx, Ws, x_lo, x_hi, wx);
    const int ty[4] = {y_lo, y_lo, y_hi, y_hi}, tx[4] = {x_lo, x_hi, x_lo, x_hi};
    image_pixel(p1, p2, Wb, ty, tx, wx, wy, rec, nrect, c1, c2, a1 + 3 * k, a2 + 3 * k);

    // the winner of cell (v, u): the valid source pixel with the largest ys * Ws + xs that lands on it
    const long win = sparse_winner(pv, Wb, v, u, ys_lo, ys_hi, sx, isx, isy, Ws);
    float2 f = make_float2(0.f, 0.f);
    if (win >= 0) f = *(const float2*)(pf + win * 2);
    flow_pixel(f.x, f.y, win >= 0, isx, isy, hflip, vflip, fl + 2 * k, va + k);
  }

  const long px = ((long)n * h + y) * w + x4;   // first output pixel of the run
  store_run(o1, o2, oflow, ovalid, px, x4, w, a1, a2, fl, va);
}

}  // namespace

extern "C" int jr_augment_sparse_sums(const void* img1, const void* img2, const int* params, int B, int Hb, int Wb,
                                      int* sums, hipStream_t stream) {
  // a frame's sum plus the rounding term of the mean must fit an int32
  if (B < 1 || B > 32767 || Hb < 1 || Wb < 1 || (long)Hb * Wb * 255 + (long)Hb * Wb / 2 > 0x7fffffffL || !img1 || !img2 ||
      !params || !sums)
    return (int)hipErrorInvalidValue;
  const int npix = Hb * Wb;
  hipError_t e = hipMemsetAsync(sums, 0, sizeof(int) * 6 * (size_t)B, stream);   // ordered before the adds
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)((npix + 256 * SUM_PIX - 1) / (256 * SUM_PIX)), (unsigned)(2 * B));
  hipLaunchKernelGGL(augment_sparse_sums_kernel, grid, dim3(256), 0, stream, (const unsigned char*)img1,
                     (const unsigned char*)img2, params, B, Hb, Wb, sums);
  return (int)hipGetLastError();
}

extern "C" int jr_augment_sparse(const void* img1, const void* img2, const float* flow, const void* valid_in,
                                 const int* params, const int* sums, float* out1, float* out2, float* out_flow,
                                 float* valid, int B, int Hb, int Wb, int h, int w, hipStream_t stream) {
  if (B < 1 || B > 65535 || Hb < 1 || Wb < 1 || h < 1 || w < 1 || h > 65535 * 4 || (long)Hb * Wb > 0x7fffffffL / 256 ||
      (long)h * w > 0x3fffffffL || !img1 || !img2 || !flow || !valid_in || !params || !sums || !out1 || !out2 ||
      !out_flow || !valid)
    return (int)hipErrorInvalidValue;
  const int runs = (w + 3) / 4;
  const dim3 grid((unsigned)((runs + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)B);
  hipLaunchKernelGGL(augment_sparse_kernel, grid, dim3(64, 4), 0, stream, (const unsigned char*)img1,
                     (const unsigned char*)img2, flow, (const unsigned char*)valid_in, params, sums, out1, out2, out_flow,
                     valid, B, Hb, Wb, h, w);
  return (int)hipGetLastError();
}
