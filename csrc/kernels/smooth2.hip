// Second-order edge-aware smoothness of the label-free loss (train/unsup.py, step 4b; smooth2_sums): the
// penalty on the second difference of every iteration's prediction that UFlow / SMURF use on KITTI, where
// a first-order penalty pulls slanted surfaces towards piecewise-constant flow.  Two bandwidth kernels on
// the scaffold of loss_common.h, the shape of unsup.hip's two: no LDS image, no atomics, no memset,
// bitwise repeatable.
//
// pred fp32 [N][B][H][W][2] (channel 0 = x), image1 fp32 [B][H][W][3], prm fp32 [4] = (eps, eps_s,
// edge_kappa, out_penalty) on the device, of which words 1 and 2 are read.  Per pixel (y, x) and
// iteration i, with f = pred[i][b]:
//   a2_x(y, x) = exp(-kappa mean_c |image1(y, x+2) - image1(y, x)|) for x < W-2: the stride-2 image
//   difference across the triple; a2_y alike between rows y and y+2;
//   D2x_k(y, x) = (f_k(y, x+2) - f_k(y, x+1)) - (f_k(y, x+1) - f_k(y, x)), D2y_k alike down a column;
//   the pixel owns the triple that starts at it to the right and the one that starts at it downwards:
//   a2_x sum_k rho_s(D2x_k) and a2_y sum_k rho_s(D2y_k), rho_s(d) = sqrt(d^2 + eps_s^2).
// A triple never leaves its row (x < W-2) or its frame (y < H-2): W < 3 has none on the x axis, H < 3 none
// on the y axis.
//
// Both kernels: one thread per pixel, grid.y over groups of ITERS iterations, the edge weights computed once
// per group.  The neighbours' flows are coalesced re-reads of rows that the neighbouring threads read as
// their own.
//   1. smooth2_loss_kernel: grid-stride over the pixels (GRID_X blocks at most); per iteration five 8-byte
//      flow loads (the pixel's own, +1, +2, +W, +2W); one row part[block][i][4] = (x-axis sum, y-axis sum,
//      0, 0) per iteration.
//   2. smooth2_loss_bwd_kernel: grad fp32 [N][B][H][W][2] as a gather.  A pixel is the left end, the centre
//      and the right end of up to three triples per axis; with psi(d) = d / sqrt(d^2 + eps_s^2)
//        g_k(y, x) = scale[i] [a2_x(x) psi(D2x_k(x)) - 2 a2_x(x-1) psi(D2x_k(x-1)) + a2_x(x-2) psi(D2x_k(x-2))
//                              + the same three terms down the column],
//      each term only where its triple exists: six edge weights per group, nine flows per iteration.
//      add = 0 writes every element of grad, add = 1 adds into it.
#include <algorithm>

#include "kernels.h"
#include "loss_common.h"

namespace {

using namespace loss;

__device__ __forceinline__ float2 ld2(const float* p) { return *(const float2*)p; }

// exp(-kappa * mean_c |b_c - a_c|) of two image1 texels
__device__ __forceinline__ float edge_weight(const float* __restrict__ a, const float* __restrict__ b, float kappa) {
  const float m = ((fabsf(b[0] - a[0]) + fabsf(b[1] - a[1])) + fabsf(b[2] - a[2])) / 3.f;
  return expf(-kappa * m);
}

// the second difference of a triple (f0, f1, f2), per component
__device__ __forceinline__ float2 diff2(float2 f0, float2 f1, float2 f2) {
  return make_float2((f2.x - f1.x) - (f1.x - f0.x), (f2.y - f1.y) - (f1.y - f0.y));
}

// part fp32 [gridDim.x][N][4]
__global__ __launch_bounds__(BLOCK) void smooth2_loss_kernel(const float* __restrict__ pred, const float* __restrict__ img1,
                                                             const float* __restrict__ prm, float* __restrict__ part,
                                                             int H, int W, long P, int N) {
  constexpr int Q = 2 * ITERS;
  __shared__ float red[Q][BLOCK / 64];
  const float eps_s = prm[1], kappa = prm[2];
  const float es2 = eps_s * eps_s;
  const int i0 = (int)blockIdx.y * ITERS;                    // block-uniform
  float acc[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) acc[k] = 0.f;
  const long stride = (long)gridDim.x * BLOCK;
  for (long p = (long)blockIdx.x * BLOCK + threadIdx.x; p < P; p += stride) {
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const float* c1 = img1 + 3 * p;
    const bool tx = x < W - 2, ty = y < H - 2;               // the triple stays in its row / its frame
    const float ax = tx ? edge_weight(c1, c1 + 6, kappa) : 0.f;
    const float ay = ty ? edge_weight(c1, c1 + 6 * (long)W, kappa) : 0.f;
#pragma unroll
    for (int k = 0; k < ITERS; ++k) {
      const int i = i0 + k;
      if (i >= N) break;
      const float* fp = pred + 2 * ((long)i * P + p);
      const float2 f = ld2(fp);
      if (tx) {
        const float2 d = diff2(f, ld2(fp + 2), ld2(fp + 4));
        acc[k] += ax * (rho(d.x, es2) + rho(d.y, es2));
      }
      if (ty) {
        const float2 d = diff2(f, ld2(fp + 2 * (long)W), ld2(fp + 4 * (long)W));
        acc[ITERS + k] += ay * (rho(d.x, es2) + rho(d.y, es2));
      }
    }
  }
  block_sums(acc, red);
  int k, i;
  if (owns_row(i0, N, k, i)) store_row(part, N, i, row_total(red[k]), row_total(red[ITERS + k]), 0.f, 0.f);
}

// One axis of the gather at a pixel with `lo` pixels before it and `hi` after it on that axis (each counted up
// to 2); s = the flow offset of one step; a0, a1, a2 = the edge weights of the triples that start at the pixel,
// one step and two steps before it (0 where there is none).
__device__ __forceinline__ void axis_bwd(const float* __restrict__ fp, float2 f, long s, int lo, int hi, float a0, float a1,
                                         float a2, float es2, float& gx, float& gy) {
  float2 m1 = f, m2 = f, p1 = f, p2 = f;
  if (lo >= 1) m1 = ld2(fp - s);
  if (lo >= 2) m2 = ld2(fp - 2 * s);
  if (hi >= 1) p1 = ld2(fp + s);
  if (hi >= 2) p2 = ld2(fp + 2 * s);
  if (hi >= 2) {                                            // the left end of (f, p1, p2)
    const float2 d = diff2(f, p1, p2);
    gx += a0 * drho(d.x, es2);
    gy += a0 * drho(d.y, es2);
  }
  if (lo >= 1 && hi >= 1) {                                 // the centre of (m1, f, p1)
    const float2 d = diff2(m1, f, p1);
    gx -= 2.f * (a1 * drho(d.x, es2));
    gy -= 2.f * (a1 * drho(d.y, es2));
  }
  if (lo >= 2) {                                            // the right end of (m2, m1, f)
    const float2 d = diff2(m2, m1, f);
    gx += a2 * drho(d.x, es2);
    gy += a2 * drho(d.y, es2);
  }
}

// scale fp32 [N]; grad fp32 [N][P][2]
template <bool ADD>
__global__ __launch_bounds__(BLOCK) void smooth2_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ img1,
                                                                 const float* __restrict__ prm, const float* __restrict__ scale,
                                                                 float* __restrict__ grad, int H, int W, long P, int N) {
  const long p = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (p >= P) return;
  const float eps_s = prm[1], kappa = prm[2];
  const float es2 = eps_s * eps_s;
  const int i0 = (int)blockIdx.y * ITERS;
  const int x = (int)(p % W), y = (int)((p / W) % H);
  const float* c1 = img1 + 3 * p;
  const long row = 3 * (long)W;
  // pixels before and after this one in its row and in its column, up to 2
  const int xl = min(x, 2), xh = min(W - 1 - x, 2), yl = min(y, 2), yh = min(H - 1 - y, 2);
  const float ax0 = xh >= 2 ? edge_weight(c1, c1 + 6, kappa) : 0.f;
  const float ax1 = (xl >= 1 && xh >= 1) ? edge_weight(c1 - 3, c1 + 3, kappa) : 0.f;
  const float ax2 = xl >= 2 ? edge_weight(c1 - 6, c1, kappa) : 0.f;
  const float ay0 = yh >= 2 ? edge_weight(c1, c1 + 2 * row, kappa) : 0.f;
  const float ay1 = (yl >= 1 && yh >= 1) ? edge_weight(c1 - row, c1 + row, kappa) : 0.f;
  const float ay2 = yl >= 2 ? edge_weight(c1 - 2 * row, c1, kappa) : 0.f;
#pragma unroll
  for (int k = 0; k < ITERS; ++k) {
    const int i = i0 + k;
    if (i >= N) break;
    const long at = 2 * ((long)i * P + p);
    const float* fp = pred + at;
    const float2 f = ld2(fp);
    float sx = 0.f, sy = 0.f;
    axis_bwd(fp, f, 2, xl, xh, ax0, ax1, ax2, es2, sx, sy);
    axis_bwd(fp, f, 2 * (long)W, yl, yh, ay0, ay1, ay2, es2, sx, sy);
    const float s = scale[i];
    {
      // the product rounded on its own: adding into grad is then writing and adding afterwards, bit for bit
#pragma clang fp contract(off)
      float2 g = make_float2(s * sx, s * sy);
      if (ADD) {
        const float2 o = ld2(grad + at);
        g = make_float2(o.x + g.x, o.y + g.y);
      }
      *(float2*)(grad + at) = g;
    }
  }
}

}  // namespace

extern "C" int jr_smooth2_loss_blocks(long P) { return (int)std::min<long>(GRID_X, (P + BLOCK - 1) / BLOCK); }

extern "C" int jr_smooth2_loss(const float* pred, const float* img1, const float* prm, float* part, int B, int H, int W,
                               int N, hipStream_t stream) {
  const long P = (long)B * H * W;
  if (!sizes_ok(B, H, W, N) || !pred || !img1 || !prm || !part) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(smooth2_loss_kernel, dim3((unsigned)jr_smooth2_loss_blocks(P), iter_groups(N)), dim3(BLOCK), 0,
                     stream, pred, img1, prm, part, H, W, P, N);
  return (int)hipGetLastError();
}

extern "C" int jr_smooth2_loss_bwd(const float* pred, const float* img1, const float* prm, const float* scale, float* grad,
                                   int B, int H, int W, int N, int add, hipStream_t stream) {
  const long P = (long)B * H * W;
  if (!sizes_ok(B, H, W, N) || !pred || !img1 || !prm || !scale || !grad || (add != 0 && add != 1))
    return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((P + BLOCK - 1) / BLOCK), iter_groups(N));
  if (add)
    hipLaunchKernelGGL(smooth2_loss_bwd_kernel<true>, grid, dim3(BLOCK), 0, stream, pred, img1, prm, scale, grad, H, W, P, N);
  else
    hipLaunchKernelGGL(smooth2_loss_bwd_kernel<false>, grid, dim3(BLOCK), 0, stream, pred, img1, prm, scale, grad, H, W, P, N);
  return (int)hipGetLastError();
}
