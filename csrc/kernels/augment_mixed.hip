// Dense and sparse samples in one batch (RAFT's Sintel stage: Sintel and FlyingThings next to KITTI
// and HD1K), each of its own size, in PACKED SLOTS: slot n of the [B][S] buffers holds sample n in its
// first Hs * Ws pixels with row pitch Ws, S the largest Hs * Ws of the list.  The record is the sparse
// one (52 words) with word 18 saying which ground truth the sample has.  The semantics are the golden
// op's (train/augment.py:augment_pairs_mixed), a composition of the dense and the sparse op with no
// arithmetic of its own, and so are the kernels: the images, the four-tap flow blend and the sparse
// scan are the functions of augment_common.h that augment.hip and augment_sparse.hip call, here with
// the sample's own pitch.  Bitwise equal to the golden op; contraction is off, no float atomics.
// Nothing past Hs * Ws in a slot is read, nor the valid bytes of a dense sample.
// Two launches, shaped as the sparse pair's:
//   1. colour sums over each sample's Hs * Ws packed pixels (pixel p is at 3 p);
//   2. the gather: grid (runs of a row, rows, samples), block (64, 4): the sample's record and with it
//      the dense / sparse branch are wave-uniform, one thread per 4 consecutive pixels, 16-byte stores.
#include "augment_common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

using namespace augment_dev;

// record layout (train/augment.py:MixedAugmentParams): the sparse record, word 18 = 1 for a dense sample
constexpr int REC_WORDS = 52, I_HS = 16, I_WS = 17, I_DENSE = 18, F_BASE = 20;
constexpr int SUM_PIX = 16;     // pixels per thread of the sums kernel

// The sample's size as the kernels use it: Hs * Ws inside the slot whatever the record says.
JR_DEVICE void sample_size(const int* __restrict__ rec, int S, int& Hs, int& Ws) {
  Ws = min(max(rec[I_WS], 1), S);
  Hs = min(max(rec[I_HS], 1), S / Ws);
}

// sums int32 [2][B][3]; grid (blocks per slot, 2 * B)
__global__ __launch_bounds__(256) void augment_mixed_sums_kernel(const unsigned char* __restrict__ i1,
                                                                 const unsigned char* __restrict__ i2,
                                                                 const int* __restrict__ params, int B, int S,
                                                                 int* __restrict__ sums) {
  __shared__ int part[4][3];
  const int n = blockIdx.y, smp = n < B ? n : n - B;
  int Hs, Ws;
  sample_size(params + smp * REC_WORDS, S, Hs, Ws);
  const int npix = Hs * Ws;
  if ((int)blockIdx.x * (256 * SUM_PIX) >= npix) return;   // block-uniform: a sample smaller than the slot
  const unsigned char* img = (n < B ? i1 : i2) + (long)smp * S * 3;
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
__global__ __launch_bounds__(256) void augment_mixed_kernel(
    const unsigned char* __restrict__ i1, const unsigned char* __restrict__ i2, const float* __restrict__ flow,
    const unsigned char* __restrict__ valid, const int* __restrict__ params, const int* __restrict__ sums,
    float* __restrict__ o1, float* __restrict__ o2, float* __restrict__ oflow, float* __restrict__ ovalid, int B, int S,
    int h, int w) {
  const int n = blockIdx.z;
  const int y = blockIdx.y * 4 + threadIdx.y;
  const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4;
  if (y >= h || x4 >= w) return;
  const int* rec = params + n * REC_WORDS;                  // wave-uniform: scalar loads
  const float* recf = (const float*)(rec + F_BASE);
  int Hs, Ws;
  sample_size(rec, S, Hs, Ws);
  const int npix = Hs * Ws;
  const bool dense = rec[I_DENSE] != 0;                     // wave-uniform: the branch below does not diverge
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
  const long slot = (long)n * S;                            // 64-bit: B * S * 3 can pass 2^31
  const unsigned char* p1 = i1 + slot * 3;
  const unsigned char* p2 = i2 + slot * 3;
  const float* pf = flow + slot * 2;
  const unsigned char* pv = valid + slot;
  int ys_lo = 0, ys_hi = -1;
  if (!dense) scan_window(v, sy, Hs, ys_lo, ys_hi);

  float a1[12], a2[12], fl[8], va[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = min(x4 + k, w - 1);   // the tail of a width that is no multiple of 4 repeats its last pixel (not stored)
    int u = x + x0, x_lo, x_hi;         // u: the cell's column X before flips
    if (hflip) u = Wr - 1 - u;
    float wx;
    source_pos(u, sx, Ws, x_lo, x_hi, wx);
    const int ty[4] = {y_lo, y_lo, y_hi, y_hi}, tx[4] = {x_lo, x_hi, x_lo, x_hi};
    image_pixel(p1, p2, Ws, ty, tx, wx, wy, rec, nrect, c1, c2, a1 + 3 * k, a2 + 3 * k);
    if (dense) {
      float fx, fy;
      flow_blend(pf, Ws, ty, tx, wx, wy, fx, fy);
      flow_pixel(fx, fy, true, isx, isy, hflip, vflip, fl + 2 * k, va + k);
    } else {
      const long win = sparse_winner(pv, Ws, v, u, ys_lo, ys_hi, sx, isx, isy, Ws);
      float2 f = make_float2(0.f, 0.f);
      if (win >= 0) f = *(const float2*)(pf + win * 2);
      flow_pixel(f.x, f.y, win >= 0, isx, isy, hflip, vflip, fl + 2 * k, va + k);
    }
  }

  const long px = ((long)n * h + y) * w + x4;   // first output pixel of the run
  store_run(o1, o2, oflow, ovalid, px, x4, w, a1, a2, fl, va);
}

}  // namespace

extern "C" int jr_augment_mixed_sums(const void* img1, const void* img2, const int* params, int B, long S, int* sums,
                                     hipStream_t stream) {
  // a sample's sum plus the rounding term of the mean must fit an int32
  if (B < 1 || B > 32767 || S < 1 || S * 255 + S / 2 > 0x7fffffffL || !img1 || !img2 || !params || !sums)
    return (int)hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(sums, 0, sizeof(int) * 6 * (size_t)B, stream);   // ordered before the adds
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)((S + 256 * SUM_PIX - 1) / (256 * SUM_PIX)), (unsigned)(2 * B));
  hipLaunchKernelGGL(augment_mixed_sums_kernel, grid, dim3(256), 0, stream, (const unsigned char*)img1,
                     (const unsigned char*)img2, params, B, (int)S, sums);
  return (int)hipGetLastError();
}

extern "C" int jr_augment_mixed(const void* img1, const void* img2, const float* flow, const void* valid_in,
                                const int* params, const int* sums, float* out1, float* out2, float* out_flow,
                                float* valid, int B, long S, int h, int w, hipStream_t stream) {
  if (B < 1 || B > 65535 || S < 1 || h < 1 || w < 1 || h > 65535 * 4 || S > 0x7fffffffL / 256 ||
      (long)h * w > 0x3fffffffL || !img1 || !img2 || !flow || !valid_in || !params || !sums || !out1 || !out2 ||
      !out_flow || !valid)
    return (int)hipErrorInvalidValue;
  const int runs = (w + 3) / 4;
  const dim3 grid((unsigned)((runs + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)B);
  hipLaunchKernelGGL(augment_mixed_kernel, grid, dim3(64, 4), 0, stream, (const unsigned char*)img1,
                     (const unsigned char*)img2, flow, (const unsigned char*)valid_in, params, sums, out1, out2, out_flow,
                     valid, B, (int)S, h, w);
  return (int)hipGetLastError();
}
