// Label-free training loss (train/unsup.py:unsup_loss_reference): a robust photometric term on
// image 2 sampled at x + flow(x) and an edge-aware first-order smoothness term, for every
// iteration's prediction.  Two bandwidth kernels, no atomics, bitwise repeatable.
//
// pred fp32 [N][B][H][W][2] (channel 0 = x), image1 / image2 fp32 [B][H][W][3], mask (optional)
// fp32 [B][H][W], used where >= 0.5, prm fp32 [4] = (eps, eps_s, edge_kappa, out_penalty) on the
// device.  Per pixel (y, x) and iteration i, with f = pred[i][b][y][x]:
//   px = float(x) + f.x, py = float(y) + f.y; inside iff 0 <= px <= W-1 and 0 <= py <= H-1 (NaN
//   fails); x0 = floor(px), x1 = min(x0+1, W-1), wx = px - x0, y alike (framewarp.hip's steps);
//   v_c = t + wy (b - t), t = c00 + wx (c01 - c00), b = c10 + wx (c11 - c10) on image 2;
//   pix = mean_c sqrt((v_c - image1_c)^2 + eps^2) inside, out_penalty outside (+ 0 * (f.x + f.y),
//   so a non-finite flow poisons its iteration's sum whatever the mask says);
//   a_x(y, x) = exp(-kappa mean_c |image1(y, x+1) - image1(y, x)|) for x < W-1, a_y alike;
//   the pixel owns the pairs to its right and below: a_x sum_k rho_s(f_k(y, x+1) - f_k(y, x)) + the
//   same in y, rho_s(d) = sqrt(d^2 + eps_s^2).
//
// Both kernels: one thread per pixel, grid.y over groups of ITERS iterations, so that the
// iteration-independent work of a pixel (image1 and its neighbours, the edge weights' exp, the
// mask) is done once per ITERS iterations and a thread carries 3 * ITERS + 1 accumulators, not
// 3 * 32 + 1.  The flow of the right / lower (and, backward, left / upper) neighbour is a
// coalesced read of rows that the neighbouring threads read as their own; the four texels of
// image 2 are 12-byte gathers through the caches.
//   1. unsup_loss_kernel: grid-stride over the pixels (GRID_X blocks at most), reduced by
//      loss_common.h to one row part[block][i][4] per iteration: (sum of mask * pix, smoothness sum,
//      masked pixels that are not inside, sum of pix over the inside masked pixels -- the last
//      iteration only, 0 elsewhere).
//   2. unsup_loss_bwd_kernel: grad fp32 [N][B][H][W][2] as a gather: scale[i][0] * mask *
//      sum_c rho'(d_c) / 3 * (dv_c/dpx, dv_c/dpy) inside, plus scale[i][1] times the
//      four-neighbour stencil -a_x(y,x) rho_s'(D at x) + a_x(y,x-1) rho_s'(D at x-1) and the same
//      in y; rho'(d) = d / sqrt(d^2 + eps^2).
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

// Steps 1 and 2 at pixel (y, x) with flow f: false where the landing point is outside the frame
// (nothing else is written then); o[4] are the float offsets of the texels 00, 01, 10, 11 inside
// one [H][W][3] image.
__device__ __forceinline__ bool landing(float2 f, int y, int x, int H, int W, float& wx, float& wy, long* o) {
  const float px = (float)x + f.x, py = (float)y + f.y;
  if (!JR_INSIDE_FRAME(px, py, H, W)) return false;
  const float x0f = floorf(px), y0f = floorf(py);
  wx = px - x0f;
  wy = py - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;                  // in [0, W-1] x [0, H-1]: inside
  const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
  o[0] = 3 * ((long)y0 * W + x0);
  o[1] = 3 * ((long)y0 * W + x1);
  o[2] = 3 * ((long)y1 * W + x0);
  o[3] = 3 * ((long)y1 * W + x1);
  return true;
}

// part fp32 [gridDim.x][N][4]
__global__ __launch_bounds__(BLOCK) void unsup_loss_kernel(const float* __restrict__ pred, const float* __restrict__ img1,
                                                           const float* __restrict__ img2, const float* __restrict__ mask,
                                                           const float* __restrict__ prm, float* __restrict__ part,
                                                           int H, int W, long P, int N) {
  constexpr int Q = 3 * ITERS + 1;
  __shared__ float red[Q][BLOCK / 64];
  const float eps = prm[0], eps_s = prm[1], kappa = prm[2], out_pen = prm[3];
  const float e2 = eps * eps, es2 = eps_s * eps_s;
  const int i0 = (int)blockIdx.y * ITERS;                    // block-uniform
  float acc[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) acc[k] = 0.f;
  const long HW = (long)H * W;
  const long stride = (long)gridDim.x * BLOCK;
  for (long p = (long)blockIdx.x * BLOCK + threadIdx.x; p < P; p += stride) {
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const long b = p / HW;
    const float* c1 = img1 + 3 * p;
    const float own[3] = {c1[0], c1[1], c1[2]};
    const bool right = x < W - 1, below = y < H - 1;
    const float ax = right ? edge_weight(c1, c1 + 3, kappa) : 0.f;
    const float ay = below ? edge_weight(c1, c1 + 3 * (long)W, kappa) : 0.f;
    const bool on = mask == nullptr || mask[p] >= 0.5f;
    const float m = on ? 1.f : 0.f;
    const float* src = img2 + 3 * b * HW;
#pragma unroll
    for (int k = 0; k < ITERS; ++k) {
      const int i = i0 + k;
      if (i >= N) break;
      const float* fp = pred + 2 * ((long)i * P + p);
      const float2 f = ld2(fp);
      float sm = 0.f;
      if (right) {
        const float2 r = ld2(fp + 2);
        sm += ax * (rho(r.x - f.x, es2) + rho(r.y - f.y, es2));
      }
      if (below) {
        const float2 d = ld2(fp + 2 * (long)W);
        sm += ay * (rho(d.x - f.x, es2) + rho(d.y - f.y, es2));
      }
      acc[ITERS + k] += sm;
      float wx, wy, pix;
      long o[4];
      const bool in = landing(f, y, x, H, W, wx, wy, o);
      if (in) {
        float s3 = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float c00 = src[o[0] + c], c01 = src[o[1] + c], c10 = src[o[2] + c], c11 = src[o[3] + c];
          const float t = c00 + wx * (c01 - c00);
          const float bt = c10 + wx * (c11 - c10);
          const float v = t + wy * (bt - t);
          s3 += rho(v - own[c], e2);
        }
        pix = s3 / 3.f;
      } else {
        pix = out_pen + 0.f * (f.x + f.y);                 // NaN for a non-finite flow
      }
      acc[k] += m * pix;                                    // 0 * NaN = NaN: not masked away
      acc[2 * ITERS + k] += (on && !in) ? 1.f : 0.f;
      if (i == N - 1 && on && in) acc[3 * ITERS] += pix;
    }
  }
  block_sums(acc, red);
  int k, i;
  if (owns_row(i0, N, k, i))
    store_row(part, N, i, row_total(red[k]), row_total(red[ITERS + k]), row_total(red[2 * ITERS + k]),
              i == N - 1 ? row_total(red[3 * ITERS]) : 0.f);
}

// scale fp32 [N][2] = (photometric, smoothness); grad fp32 [N][P][2]
__global__ __launch_bounds__(BLOCK) void unsup_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ img1,
                                                               const float* __restrict__ img2, const float* __restrict__ mask,
                                                               const float* __restrict__ prm, const float* __restrict__ scale,
                                                               float* __restrict__ grad, int H, int W, long P, int N) {
  const long p = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (p >= P) return;
  const float eps = prm[0], eps_s = prm[1], kappa = prm[2];
  const float e2 = eps * eps, es2 = eps_s * eps_s;
  const int i0 = (int)blockIdx.y * ITERS;
  const long HW = (long)H * W;
  const int x = (int)(p % W), y = (int)((p / W) % H);
  const long b = p / HW;
  const float* c1 = img1 + 3 * p;
  const float own[3] = {c1[0], c1[1], c1[2]};
  const bool right = x < W - 1, left = x > 0, below = y < H - 1, above = y > 0;
  const float a_r = right ? edge_weight(c1, c1 + 3, kappa) : 0.f;
  const float a_l = left ? edge_weight(c1 - 3, c1, kappa) : 0.f;
  const float a_d = below ? edge_weight(c1, c1 + 3 * (long)W, kappa) : 0.f;
  const float a_u = above ? edge_weight(c1 - 3 * (long)W, c1, kappa) : 0.f;
  const bool on = mask == nullptr || mask[p] >= 0.5f;
  const float* src = img2 + 3 * b * HW;
#pragma unroll
  for (int k = 0; k < ITERS; ++k) {
    const int i = i0 + k;
    if (i >= N) break;
    const long at = 2 * ((long)i * P + p);
    const float* fp = pred + at;
    const float2 f = ld2(fp);
    float sx = 0.f, sy = 0.f;
    if (right) {
      const float2 r = ld2(fp + 2);
      sx -= a_r * drho(r.x - f.x, es2);
      sy -= a_r * drho(r.y - f.y, es2);
    }
    if (left) {
      const float2 l = ld2(fp - 2);
      sx += a_l * drho(f.x - l.x, es2);
      sy += a_l * drho(f.y - l.y, es2);
    }
    if (below) {
      const float2 d = ld2(fp + 2 * (long)W);
      sx -= a_d * drho(d.x - f.x, es2);
      sy -= a_d * drho(d.y - f.y, es2);
    }
    if (above) {
      const float2 u = ld2(fp - 2 * (long)W);
      sx += a_u * drho(f.x - u.x, es2);
      sy += a_u * drho(f.y - u.y, es2);
    }
    const float s_photo = scale[2 * i], s_smooth = scale[2 * i + 1];
    float gx = s_smooth * sx, gy = s_smooth * sy;
    float wx, wy;
    long o[4];
    if (on && landing(f, y, x, H, W, wx, wy, o)) {
      float px = 0.f, py = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float c00 = src[o[0] + c], c01 = src[o[1] + c], c10 = src[o[2] + c], c11 = src[o[3] + c];
        const float t = c00 + wx * (c01 - c00);
        const float bt = c10 + wx * (c11 - c10);
        const float v = t + wy * (bt - t);
        const float r = drho(v - own[c], e2);
        px += r * ((1.f - wy) * (c01 - c00) + wy * (c11 - c10));
        py += r * (bt - t);
      }
      gx += s_photo * (px / 3.f);
      gy += s_photo * (py / 3.f);
    }
    *(float2*)(grad + at) = make_float2(gx, gy);
  }
}

}  // namespace

extern "C" int jr_unsup_loss_blocks(long P) { return (int)std::min<long>(GRID_X, (P + BLOCK - 1) / BLOCK); }

extern "C" int jr_unsup_loss(const float* pred, const float* img1, const float* img2, const float* mask,
                             const float* prm, float* part, int B, int H, int W, int N, hipStream_t stream) {
  const long P = (long)B * H * W;
  if (!sizes_ok(B, H, W, N) || !pred || !img1 || !img2 || !prm || !part) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(unsup_loss_kernel, dim3((unsigned)jr_unsup_loss_blocks(P), iter_groups(N)),
                     dim3(BLOCK), 0, stream, pred, img1, img2, mask, prm, part, H, W, P, N);
  return (int)hipGetLastError();
}

extern "C" int jr_unsup_loss_bwd(const float* pred, const float* img1, const float* img2, const float* mask,
                                 const float* prm, const float* scale, float* grad, int B, int H, int W, int N,
                                 hipStream_t stream) {
  const long P = (long)B * H * W;
  if (!sizes_ok(B, H, W, N) || !pred || !img1 || !img2 || !prm || !scale || !grad) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(unsup_loss_bwd_kernel, dim3((unsigned)((P + BLOCK - 1) / BLOCK), iter_groups(N)),
                     dim3(BLOCK), 0, stream, pred, img1, img2, mask, prm, scale, grad, H, W, P, N);
  return (int)hipGetLastError();
}
