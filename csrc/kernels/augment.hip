// RAFT's dense flow augmentation (photometric jitter, eraser, scale + stretch, flips, crop) as
// ONE gather over the uint8 frames as they were uploaded, writing the fp32 NHWC tensors the
// training step consumes.  The semantics are the golden op's (train/augment.py:augment_pairs)
// and the kernels equal it bit for bit: the same fp32 operations in the same order, every
// product and sum rounded on its own (contraction is off for this file, below), no operation
// that is not correctly rounded on both sides (the host supplies every ratio, reciprocal and
// the hue matrix; the only division is the IEEE x / 255).
// Two launches, no LDS in the gather, no float atomics:
//   1. colour sums: per image and channel the integer sum of the source frame (wave reductions,
//      one integer atomic add per block and channel: order-independent, bitwise repeatable);
//   2. the gather: grid (runs of a row, rows, samples) -- the sample's 48-word record is
//      wave-uniform; one thread per 4 consecutive pixels of a row, 16-byte stores.
#include "augment_common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

using namespace augment_dev;   // the record words, texel, blend, source_pos, image_pixel, flow_blend, flow_pixel, store_run

// record layout (train/augment.py:AugmentParams): 16 ints, then 32 floats
constexpr int REC_WORDS = 48, F_BASE = 16;
constexpr int SUM_PIX = 16;   // pixels per thread of the sums kernel

// sums int32 [2][B][3] (image 1 frames, then image 2 frames); grid (blocks per frame, 2 * B)
__global__ __launch_bounds__(256) void augment_sums_kernel(const unsigned char* __restrict__ i1,
                                                           const unsigned char* __restrict__ i2, int B, int npix,
                                                           int* __restrict__ sums) {
  __shared__ int part[4][3];
  const int n = blockIdx.y;
  const unsigned char* img = (n < B ? i1 + (long)n * npix * 3 : i2 + (long)(n - B) * npix * 3);
  const int base = blockIdx.x * (256 * SUM_PIX) + threadIdx.x;
  int s[3] = {0, 0, 0};
#pragma unroll 4
  for (int k = 0; k < SUM_PIX; ++k) {
    const int p = base + k * 256;
    if (p < npix) {
      const unsigned char* px = img + (long)p * 3;
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
__global__ __launch_bounds__(256) void augment_kernel(const unsigned char* __restrict__ i1,
                                                      const unsigned char* __restrict__ i2,
                                                      const float* __restrict__ flow, const int* __restrict__ params,
                                                      const int* __restrict__ sums, float* __restrict__ o1,
                                                      float* __restrict__ o2, float* __restrict__ oflow,
                                                      float* __restrict__ ovalid, int B, int Hs, int Ws, int h, int w) {
  const int n = blockIdx.z;
  const int y = blockIdx.y * 4 + threadIdx.y;
  const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4;
  if (y >= h || x4 >= w) return;
  const int* rec = params + n * REC_WORDS;                  // wave-uniform: scalar loads
  const float* recf = (const float*)(rec + F_BASE);
  const int npix = Hs * Ws;
  const int Hr = rec[I_HR], Wr = rec[I_WR], y0 = rec[I_Y0], x0 = rec[I_X0];
  const bool hflip = rec[I_HFLIP] != 0, vflip = rec[I_VFLIP] != 0;
  const int nrect = rec[I_NRECT];
  const float sx = recf[F_SX], sy = recf[F_SY], isx = recf[F_ISX], isy = recf[F_ISY];
  const Colour c1 = load_colour(recf + F_COL1, sums + n * 3, npix);
  const Colour c2 = load_colour(recf + F_COL2, sums + (B + n) * 3, npix);

  int v = y + y0, y_lo, y_hi;
  if (vflip) v = Hr - 1 - v;
  float wy;
  source_pos(v, sy, Hs, y_lo, y_hi, wy);
  const long frame = (long)n * npix;
  const unsigned char* p1 = i1 + frame * 3;
  const unsigned char* p2 = i2 + frame * 3;
  const float* pf = flow + frame * 2;

  float a1[12], a2[12], fl[8], va[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = min(x4 + k, w - 1);   // the tail of a width that is no multiple of 4 repeats its last pixel (not stored)
    int u = x + x0, x_lo, x_hi;
    if (hflip) u = Wr - 1 - u;
    float wx;
    source_pos(u, sx, Ws, x_lo, x_hi, wx);
    const int ty[4] = {y_lo, y_lo, y_hi, y_hi}, tx[4] = {x_lo, x_hi, x_lo, x_hi};
    image_pixel(p1, p2, Ws, ty, tx, wx, wy, rec, nrect, c1, c2, a1 + 3 * k, a2 + 3 * k);
    float fx, fy;
    flow_blend(pf, Ws, ty, tx, wx, wy, fx, fy);
    flow_pixel(fx, fy, true, isx, isy, hflip, vflip, fl + 2 * k, va + k);
  }

  const long px = ((long)n * h + y) * w + x4;   // first output pixel of the run
  store_run(o1, o2, oflow, ovalid, px, x4, w, a1, a2, fl, va);
}

}  // namespace

extern "C" int jr_augment_sums(const void* img1, const void* img2, int B, int Hs, int Ws, int* sums,
                               hipStream_t stream) {
  // a frame's sum plus the rounding term of the mean must fit an int32
  if (B < 1 || B > 32767 || Hs < 1 || Ws < 1 || (long)Hs * Ws * 255 + (long)Hs * Ws / 2 > 0x7fffffffL || !img1 || !img2 ||
      !sums)
    return (int)hipErrorInvalidValue;
  const int npix = Hs * Ws;
  hipError_t e = hipMemsetAsync(sums, 0, sizeof(int) * 6 * (size_t)B, stream);   // ordered before the adds
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)((npix + 256 * SUM_PIX - 1) / (256 * SUM_PIX)), (unsigned)(2 * B));
  hipLaunchKernelGGL(augment_sums_kernel, grid, dim3(256), 0, stream, (const unsigned char*)img1,
                     (const unsigned char*)img2, B, npix, sums);
  return (int)hipGetLastError();
}

extern "C" int jr_augment(const void* img1, const void* img2, const float* flow, const int* params, const int* sums,
                          float* out1, float* out2, float* out_flow, float* valid, int B, int Hs, int Ws, int h, int w,
                          hipStream_t stream) {
  if (B < 1 || B > 65535 || Hs < 1 || Ws < 1 || h < 1 || w < 1 || h > 65535 * 4 || (long)Hs * Ws > 0x7fffffffL / 256 ||
      (long)h * w > 0x3fffffffL || !img1 || !img2 || !flow || !params || !sums || !out1 || !out2 || !out_flow || !valid)
    return (int)hipErrorInvalidValue;
  const int runs = (w + 3) / 4;
  const dim3 grid((unsigned)((runs + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)B);
  hipLaunchKernelGGL(augment_kernel, grid, dim3(64, 4), 0, stream, (const unsigned char*)img1,
                     (const unsigned char*)img2, flow, params, sums, out1, out2, out_flow, valid, B, Hs, Ws, h, w);
  return (int)hipGetLastError();
}
