// RAFT's flow augmentation (photometric jitter, eraser, scale + stretch, flips, crop) as ONE gather
// over the uint8 frames as they were uploaded, writing the fp32 NHWC tensors the training step
// consumes -- for the three layouts a batch can have (kernels.h: JR_AUGMENT_*):
//   DENSE   frames [B][Hs][Ws] of one size with dense ground truth (train/augment.py:augment_pairs);
//   SPARSE  KITTI / HD1K: every sample in the top-left corner of a [Hb][Wb] buffer, its own size
//           (Hs, Ws) in its record, sparse ground truth with a valid plane (augment_pairs_sparse);
//   MIXED   RAFT's Sintel stage: packed slots [B][S], sample n in the first Hs * Ws pixels of slot n
//           with row pitch Ws, record word 18 saying which ground truth it has (augment_pairs_mixed).
// The semantics are the golden ops' and the kernels equal them bit for bit: the same fp32 operations
// in the same order, every product and sum rounded on its own (contraction is off for this file,
// below), no operation that is not correctly rounded on both sides (the host supplies every ratio,
// reciprocal and the hue matrix; the only division is the IEEE x / 255).
// Dense flow is the four-tap blend.  Sparse flow cannot be interpolated: the golden op moves it point
// by point, a forward scatter in which the source pixel with the largest linear index wins a cell.
// The kernel inverts that map per output cell: it scans the candidate source rows from the highest
// down and in each the candidate columns from the highest down, evaluates the forward predicate
// rint(fp32(xs) * isx) == X itself on each, and takes the first candidate whose valid byte is set --
// the largest linear index, so no atomics, no memset and no winner plane.
// One body per launch, the layout a template parameter: each instantiation carries only its own
// geometry and flow code.  Two launches, no LDS in the gather, no float atomics:
//   1. colour sums: per image and channel the integer sum of each sample's own pixels (padding never
//      enters; wave reductions, one integer atomic add per block and channel: order-independent,
//      bitwise repeatable);
//   2. the gather: grid (runs of a row, rows, samples) -- the sample's record, and with it MIXED's
//      dense / sparse branch, is wave-uniform; one thread per 4 consecutive pixels of a row, 16-byte
//      stores.
// Nothing outside a sample's Hs x Ws pixels is read, nor the valid bytes of a dense sample.
#include "augment_common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

using namespace augment_dev;   // the record words, texel, blend, source_pos, image_pixel, flow_blend, sparse_winner, flow_pixel, store_run

constexpr int SUM_PIX = 16;   // pixels per thread of the sums kernel

struct Sample {
  int Hs, Ws, pitch;          // the sample's size and the pixels from one of its rows to the next
};

// What a layout is to the kernels.  g0, g1: the two geometry arguments, (Hs, Ws) for DENSE, (Hb, Wb)
// for SPARSE, (1, S) for MIXED.
template <int L> struct Layout {
  static constexpr bool sized = L != JR_AUGMENT_DENSE;     // the record carries (Hs, Ws), and there is a valid plane
  static constexpr bool padded = L == JR_AUGMENT_SPARSE;   // rows of Ws pixels at a pitch that can be larger
  // record layout (train/augment.py): 16 ints, for a sized layout (Hs, Ws, dense flag, one spare word), then 32 floats
  static constexpr int REC_WORDS = sized ? 52 : 48, F_BASE = sized ? 20 : 16;

  // The pixels from one frame (buffer, slot) to the next.  MIXED reads no g0: the host entries insist on 1.
  static JR_DEVICE int frame(int g0, int g1) {
    if constexpr (L == JR_AUGMENT_MIXED) return g1;
    else return g0 * g1;
  }

  // The sample's size as the kernels use it: inside its buffer or slot whatever the record says.
  static JR_DEVICE Sample sample(const int* __restrict__ rec, int g0, int g1) {
    if constexpr (L == JR_AUGMENT_DENSE) {
      return {g0, g1, g1};                                 // rec is not read
    } else if constexpr (L == JR_AUGMENT_SPARSE) {
      return {min(max(rec[I_HS], 1), g0), min(max(rec[I_WS], 1), g1), g1};
    } else {
      const int Ws = min(max(rec[I_WS], 1), g1);
      return {min(max(rec[I_HS], 1), g1 / Ws), Ws, Ws};
    }
  }

  // Dense ground truth (the four-tap blend) or sparse (the scan)?  Wave-uniform where it is not a constant.
  static JR_DEVICE bool dense_flow(const int* __restrict__ rec) {
    if constexpr (L == JR_AUGMENT_MIXED) return rec[I_DENSE] != 0;
    else return L == JR_AUGMENT_DENSE;
  }
};

// sums int32 [2][B][3] (image 1 frames, then image 2 frames); grid (blocks per frame, 2 * B)
template <int L>
__global__ __launch_bounds__(256) void sums_kernel(const unsigned char* __restrict__ i1,
                                                   const unsigned char* __restrict__ i2,
                                                   const int* __restrict__ params, int B, int g0, int g1,
                                                   int* __restrict__ sums) {
  __shared__ int part[4][3];
  const int n = blockIdx.y, smp = n < B ? n : n - B;
  const int frame = Layout<L>::frame(g0, g1);
  Sample s0 = {g0, g1, g1};
  if constexpr (Layout<L>::sized) s0 = Layout<L>::sample(params + smp * Layout<L>::REC_WORDS, g0, g1);
  const int npix = s0.Hs * s0.Ws;
  if constexpr (Layout<L>::sized)
    if ((int)blockIdx.x * (256 * SUM_PIX) >= npix) return;   // block-uniform: a sample smaller than its frame
  const unsigned char* img = (n < B ? i1 : i2) + (long)smp * frame * 3;
  const int base = blockIdx.x * (256 * SUM_PIX) + threadIdx.x;
  int s[3] = {0, 0, 0};
#pragma unroll 4
  for (int k = 0; k < SUM_PIX; ++k) {
    const int p = base + k * 256;   // pixel p of a sample is (p / Ws, p % Ws)
    if (p < npix) {
      long at = p;
      if constexpr (Layout<L>::padded) {
        const int row = (int)((unsigned)p / (unsigned)s0.Ws);
        at = (long)row * s0.pitch + (p - row * s0.Ws);
      }
      const unsigned char* px = img + at * 3;
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
template <int L>
__global__ __launch_bounds__(256) void gather_kernel(
    const unsigned char* __restrict__ i1, const unsigned char* __restrict__ i2, const float* __restrict__ flow,
    const unsigned char* __restrict__ valid, const int* __restrict__ params, const int* __restrict__ sums,
    float* __restrict__ o1, float* __restrict__ o2, float* __restrict__ oflow, float* __restrict__ ovalid, int B, int g0,
    int g1, int h, int w) {
  const int n = blockIdx.z;
  const int y = blockIdx.y * 4 + threadIdx.y;
  const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4;
  if (y >= h || x4 >= w) return;
  const int* rec = params + n * Layout<L>::REC_WORDS;       // wave-uniform: scalar loads
  const float* recf = (const float*)(rec + Layout<L>::F_BASE);
  const Sample sm = Layout<L>::sample(rec, g0, g1);
  const int Hs = sm.Hs, Ws = sm.Ws, pitch = sm.pitch, npix = Hs * Ws;
  const bool dense = Layout<L>::dense_flow(rec);            // wave-uniform: the branch below does not diverge
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
  const long frame = (long)n * Layout<L>::frame(g0, g1);    // 64-bit: B * frame * 3 can pass 2^31
  const unsigned char* p1 = i1 + frame * 3;
  const unsigned char* p2 = i2 + frame * 3;
  const float* pf = flow + frame * 2;
  const unsigned char* pv = nullptr;
  if constexpr (Layout<L>::sized) pv = valid + frame;       // DENSE has no valid plane: no pointer is formed from it
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
    image_pixel(p1, p2, pitch, ty, tx, wx, wy, rec, nrect, c1, c2, a1 + 3 * k, a2 + 3 * k);
    if (dense) {
      float fx, fy;
      flow_blend(pf, pitch, ty, tx, wx, wy, fx, fy);
      flow_pixel(fx, fy, true, isx, isy, hflip, vflip, fl + 2 * k, va + k);
    } else if constexpr (Layout<L>::sized) {
      // the winner of cell (v, u): the valid source pixel with the largest ys * Ws + xs that lands on it
      const long win = sparse_winner(pv, pitch, v, u, ys_lo, ys_hi, sx, isx, isy, Ws);
      float2 f = make_float2(0.f, 0.f);
      if (win >= 0) f = *(const float2*)(pf + win * 2);
      flow_pixel(f.x, f.y, win >= 0, isx, isy, hflip, vflip, fl + 2 * k, va + k);
    }
  }

  const long px = ((long)n * h + y) * w + x4;   // first output pixel of the run
  store_run(o1, o2, oflow, ovalid, px, x4, w, a1, a2, fl, va);
}

}  // namespace

extern "C" int jr_augment_sums(int layout, const void* img1, const void* img2, const int* params, int B, int g0, int g1,
                               int* sums, hipStream_t stream) {
  void (*kernel)(const unsigned char*, const unsigned char*, const int*, int, int, int, int*) = nullptr;
  switch (layout) {
    case JR_AUGMENT_DENSE: kernel = sums_kernel<JR_AUGMENT_DENSE>; break;
    case JR_AUGMENT_SPARSE: kernel = sums_kernel<JR_AUGMENT_SPARSE>; break;
    case JR_AUGMENT_MIXED: kernel = sums_kernel<JR_AUGMENT_MIXED>; break;
  }
  const long P = (long)g0 * g1;   // a frame's sum plus the rounding term of the mean must fit an int32
  if (!kernel || B < 1 || B > 32767 || g0 < 1 || g1 < 1 || (layout == JR_AUGMENT_MIXED && g0 != 1) || P * 255 + P / 2 > 0x7fffffffL || !img1 || !img2 ||
      (layout != JR_AUGMENT_DENSE && !params) || !sums)
    return (int)hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(sums, 0, sizeof(int) * 6 * (size_t)B, stream);   // ordered before the adds
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)((P + 256 * SUM_PIX - 1) / (256 * SUM_PIX)), (unsigned)(2 * B));
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, (const unsigned char*)img1, (const unsigned char*)img2, params, B,
                     g0, g1, sums);
  return (int)hipGetLastError();
}

extern "C" int jr_augment_gather(int layout, const void* img1, const void* img2, const float* flow, const void* valid_in,
                                 const int* params, const int* sums, float* out1, float* out2, float* out_flow,
                                 float* valid, int B, int g0, int g1, int h, int w, hipStream_t stream) {
  void (*kernel)(const unsigned char*, const unsigned char*, const float*, const unsigned char*, const int*, const int*,
                 float*, float*, float*, float*, int, int, int, int, int) = nullptr;
  switch (layout) {
    case JR_AUGMENT_DENSE: kernel = gather_kernel<JR_AUGMENT_DENSE>; break;
    case JR_AUGMENT_SPARSE: kernel = gather_kernel<JR_AUGMENT_SPARSE>; break;
    case JR_AUGMENT_MIXED: kernel = gather_kernel<JR_AUGMENT_MIXED>; break;
  }
  if (!kernel || B < 1 || B > 65535 || g0 < 1 || g1 < 1 || (layout == JR_AUGMENT_MIXED && g0 != 1) || h < 1 || w < 1 || h > 65535 * 4 ||
      (long)g0 * g1 > 0x7fffffffL / 256 || (long)h * w > 0x3fffffffL || !img1 || !img2 || !flow ||
      (layout != JR_AUGMENT_DENSE && !valid_in) || !params || !sums || !out1 || !out2 || !out_flow || !valid)
    return (int)hipErrorInvalidValue;
  const int runs = (w + 3) / 4;
  const dim3 grid((unsigned)((runs + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)B);
  hipLaunchKernelGGL(kernel, grid, dim3(64, 4), 0, stream, (const unsigned char*)img1, (const unsigned char*)img2, flow,
                     (const unsigned char*)valid_in, params, sums, out1, out2, out_flow, valid, B, g0, g1, h, w);
  return (int)hipGetLastError();
}
