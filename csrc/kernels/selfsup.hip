// Self-supervision for label-free training (train/selfsup.py): the student's views and the teacher's
// target as a centre crop resampled back to the frame, and the loss of every student iteration against
// that target with its gradient.  Three bandwidth kernels: no LDS beyond the block reduction's 4 words
// per quantity, no atomics, no memset, bitwise repeatable.
//
//   crop_resize (train/selfsup.py:crop_resize, bit for bit; contraction is off for this file, below):
//     x, out fp32 [B][H][W][C], C = 1, 2, 3; prm fp32 [6] = (rx, ry, scale[0..3]) on the device, the
//     ratios rx = fp32(Wc / W), ry = fp32(Hc / H) rounded once by the host (the kernel never divides).
//     Output column u: xs = (float(u) + 0.5) * rx - 0.5, clamped to [0, Wc - 1], x0 = floor(xs),
//     x1 = min(x0 + 1, Wc - 1), wx = xs - x0, taps at c + x0 and c + x1; rows alike;
//     v = t + wy (b - t), t = c00 + wx (c01 - c00), b = c10 + wx (c11 - c10); channel k times scale[k].
//     Grid (blocks over a row's groups of 4 pixels, rows, B); one thread writes 4 pixels of a row:
//     16-byte stores when the width is a multiple of 4 and out is 16-byte aligned, element stores with
//     a row tail otherwise.  The taps are cached gathers of C floats; nothing outside the crop is read.
//
//   selfsup_loss / selfsup_loss_bwd (train/selfsup.py:selfsup_sums): pred fp32 [N][Btot][H][W][2], of
//     which the batches [B0, B0 + B) are read in place; target fp32 [B][H][W][2]; weight (optional)
//     fp32 [B][H][W]; prm fp32 [1] = eps.  Per iteration and pixel d = pred - target,
//     e = sqrt(d.x^2 + eps^2) + sqrt(d.y^2 + eps^2); the term is weight * e where weight > 0 and
//     0 * (pred.x + pred.y) elsewhere (a non-finite prediction poisons the sum whatever the weight, a
//     non-finite target under weight 0 is never touched).  One thread per 2 pixels, two instantiations:
//     one 16-byte load of pred and of target, one 8-byte load of the weights (and, backward, one 16-byte
//     store of grad) when every iteration's window is 16-byte aligned and holds an even number of
//     pixels; 8-byte loads and stores with a tail pixel otherwise,
//     grid.y over groups of ITERS iterations so that target and weight are read once per group.
//     Loss: grid-stride, reduced by loss_common.h to one row part[block][i][4]:
//     (sum of term, the same for i = N - 1 else 0, sum of weight for i = N - 1, count of weight > 0
//     for i = N - 1).  Backward: grad fp32 [N][B][H][W][2] (contiguous, every element written) =
//     scale[i] * weight * d / sqrt(d^2 + eps^2) per component where weight > 0, 0 * pred elsewhere.
#include <algorithm>

#include "kernels.h"

// above loss_common.h: its rho and drho stay uncontracted here, as everything below
#pragma clang fp contract(off)

#include "loss_common.h"

namespace {

using namespace loss;

constexpr int CR_BLOCK = 64;  // threads per block of crop_resize: 256 pixels of a row

// One axis of crop_resize: the two tap indices inside the crop and the weight of the second.
__device__ __forceinline__ void axis(int u, float r, int nc, int& i0, int& i1, float& w) {
  float s = ((float)u + 0.5f) * r - 0.5f;
  s = fminf(fmaxf(s, 0.f), (float)(nc - 1));
  const float f = floorf(s);
  w = s - f;
  i0 = (int)f;                                            // in [0, nc - 1]
  i1 = min(i0 + 1, nc - 1);
}

template <int C>
__global__ __launch_bounds__(CR_BLOCK) void crop_resize_kernel(const float* __restrict__ x, const float* __restrict__ prm,
                                                               float* __restrict__ out, int H, int W, int c, int vec) {
  const int u4 = ((int)blockIdx.x * CR_BLOCK + (int)threadIdx.x) * 4;
  if (u4 >= W) return;
  const int y = (int)blockIdx.y;
  const long img = (long)blockIdx.z * H * W;
  const int Wc = W - 2 * c, Hc = H - 2 * c;
  const float rx = prm[0], ry = prm[1];
  int y0, y1;
  float wy;
  axis(y, ry, Hc, y0, y1, wy);
  const float* r0 = x + C * (img + (long)(c + y0) * W + c);
  const float* r1 = x + C * (img + (long)(c + y1) * W + c);
  float* o = out + C * (img + (long)y * W + u4);
  const int n = min(4, W - u4);
  float v[4 * C];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= n) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) v[C * k + ch] = 0.f;
      continue;
    }
    int x0, x1;
    float wx;
    axis(u4 + k, rx, Wc, x0, x1, wx);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const float c00 = r0[C * x0 + ch], c01 = r0[C * x1 + ch], c10 = r1[C * x0 + ch], c11 = r1[C * x1 + ch];
      const float t = c00 + wx * (c01 - c00);
      const float b = c10 + wx * (c11 - c10);
      v[C * k + ch] = (t + wy * (b - t)) * prm[2 + ch];
    }
  }
  if (vec) {                                              // W % 4 == 0 and out 16-byte aligned: n == 4
#pragma unroll
    for (int q = 0; q < C; ++q) ((float4*)o)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    return;
  }
  for (int k = 0; k < C * n; ++k) o[k] = v[k];
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// Pixels p, p + 1 of the window (p even).  VEC: one 16-byte load through a native vector type (the window holds
// an even number of pixels, so there are always two); else 8-byte loads, the second only when there are two.
template <bool VEC>
__device__ __forceinline__ void load2(const float* __restrict__ a, bool two, float2& u, float2& v) {
  if constexpr (VEC) {
    const f32x4 q = *(const f32x4*)a;
    u = make_float2(q.x, q.y);
    v = make_float2(q.z, q.w);
  } else {
    const f32x2 q = *(const f32x2*)a;
    u = make_float2(q.x, q.y);
    v = make_float2(0.f, 0.f);
    if (two) {
      const f32x2 r = *(const f32x2*)(a + 2);
      v = make_float2(r.x, r.y);
    }
  }
}

// The weights of pixels p, p + 1 (1 without a weight plane; 0 for a second pixel that does not exist).
template <bool VEC>
__device__ __forceinline__ void weights2(const float* __restrict__ weight, long p, bool two, float* w) {
  w[0] = 1.f;
  w[1] = two ? 1.f : 0.f;
  if (weight == nullptr) return;
  if constexpr (VEC) {
    const f32x2 q = *(const f32x2*)(weight + p);
    w[0] = q.x;
    w[1] = q.y;
  } else {
    w[0] = weight[p];
    if (two) w[1] = weight[p + 1];
  }
}

// pred points at batch B0 of iteration 0; it_stride = Btot * H * W pixels.  part fp32 [gridDim.x][N][4]
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void selfsup_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             const float* __restrict__ weight, const float* __restrict__ prm,
                                                             float* __restrict__ part, long P, long it_stride, int N) {
  constexpr int Q = ITERS + 2;
  __shared__ float red[Q][BLOCK / 64];
  const float eps = prm[0];
  const float e2 = eps * eps;
  const int i0 = (int)blockIdx.y * ITERS;                   // block-uniform
  float acc[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) acc[k] = 0.f;
  const long stride = 2L * gridDim.x * BLOCK;
  for (long p = 2 * ((long)blockIdx.x * BLOCK + threadIdx.x); p < P; p += stride) {
    const bool two = VEC || p + 1 < P;
    float w[2];
    weights2<VEC>(weight, p, two, w);
    const bool on[2] = {w[0] > 0.f, w[1] > 0.f};
    float2 t[2];
    load2<VEC>(target + 2 * p, two, t[0], t[1]);
#pragma unroll
    for (int k = 0; k < ITERS; ++k) {
      const int i = i0 + k;
      if (i >= N) break;
      float2 f[2];
      load2<VEC>(pred + 2 * ((long)i * it_stride + p), two, f[0], f[1]);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j == 1 && !two) break;
        // the target of a pixel without weight is not used: it may be non-finite
        const float term = on[j] ? w[j] * (rho(f[j].x - t[j].x, e2) + rho(f[j].y - t[j].y, e2))
                                 : 0.f * (f[j].x + f[j].y);
        acc[k] += term;
      }
    }
    if (i0 + ITERS >= N) {                                  // the group of the last iteration
      acc[ITERS] += (on[0] ? w[0] : 0.f) + (on[1] ? w[1] : 0.f);
      acc[ITERS + 1] += (on[0] ? 1.f : 0.f) + (on[1] ? 1.f : 0.f);
    }
  }
  block_sums(acc, red);
  int k, i;
  if (owns_row(i0, N, k, i)) {
    const bool last = i == N - 1;
    const float sum = row_total(red[k]);
    store_row(part, N, i, sum, last ? sum : 0.f, last ? row_total(red[ITERS]) : 0.f, last ? row_total(red[ITERS + 1]) : 0.f);
  }
}

// scale fp32 [N]; grad fp32 [N][P][2].  VEC: 16-byte loads as above and 16-byte stores of grad.
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void selfsup_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                 const float* __restrict__ weight, const float* __restrict__ prm,
                                                                 const float* __restrict__ scale, float* __restrict__ grad,
                                                                 long P, long it_stride, int N) {
  const long p = 2 * ((long)blockIdx.x * BLOCK + threadIdx.x);
  if (p >= P) return;
  const float eps = prm[0];
  const float e2 = eps * eps;
  const int i0 = (int)blockIdx.y * ITERS;
  const bool two = VEC || p + 1 < P;
  float w[2];
  weights2<VEC>(weight, p, two, w);
  const bool on[2] = {w[0] > 0.f, w[1] > 0.f};
  float2 t[2];
  load2<VEC>(target + 2 * p, two, t[0], t[1]);
#pragma unroll
  for (int k = 0; k < ITERS; ++k) {
    const int i = i0 + k;
    if (i >= N) break;
    float2 f[2], g[2];
    load2<VEC>(pred + 2 * ((long)i * it_stride + p), two, f[0], f[1]);
    const float s = scale[i];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (on[j]) {
        const float sw = s * w[j];
        g[j] = make_float2(sw * drho(f[j].x - t[j].x, e2), sw * drho(f[j].y - t[j].y, e2));
      } else {
        g[j] = make_float2(0.f * f[j].x, 0.f * f[j].y);    // exactly 0, NaN at a non-finite prediction
      }
    }
    float* o = grad + 2 * ((long)i * P + p);
    if constexpr (VEC) {
      f32x4 q;
      q.x = g[0].x; q.y = g[0].y; q.z = g[1].x; q.w = g[1].y;
      *(f32x4*)o = q;
    } else {
      f32x2 q;
      q.x = g[0].x; q.y = g[0].y;
      *(f32x2*)o = q;
      if (two) {
        q.x = g[1].x; q.y = g[1].y;
        *(f32x2*)(o + 2) = q;
      }
    }
  }
}

inline bool loss_sizes_ok(int B, int H, int W, int N, int Btot, int B0) {
  return sizes_ok(Btot, H, W, N) && B >= 1 && B0 >= 0 && B0 <= Btot - B;
}

// The 16-byte form: every iteration's window starts 16-byte aligned and holds an even number of pixels (no
// thread's second pixel lies past the window); the weight plane, read 8 bytes at a time, is 8-byte aligned;
// grad (backward; nullptr in the forward) is 16-byte aligned.
inline bool loss_vec(const float* pred, const float* target, const float* weight, const float* grad, long P, long it_stride,
                     long off) {
  return P % 2 == 0 && it_stride % 2 == 0 && off % 2 == 0 && (uintptr_t)pred % 16 == 0 && (uintptr_t)target % 16 == 0 &&
         (uintptr_t)weight % 8 == 0 && (uintptr_t)grad % 16 == 0;
}

}  // namespace

extern "C" int jr_crop_resize(const float* x, const float* prm, float* out, int B, int H, int W, int C, int c,
                              hipStream_t stream) {
  if (B < 1 || B > 65535 || H < 1 || H > 65535 || W < 1 || C < 1 || C > 3 || c < 1 || 2L * c >= std::min(H, W) ||
      (long)B * H * W * C > 0x7fffffffL || !x || !prm || !out)
    return (int)hipErrorInvalidValue;
  const int vec = W % 4 == 0 && (uintptr_t)out % 16 == 0;
  const dim3 grid((unsigned)(((W + 3) / 4 + CR_BLOCK - 1) / CR_BLOCK), (unsigned)H, (unsigned)B);
  if (C == 1) hipLaunchKernelGGL(crop_resize_kernel<1>, grid, dim3(CR_BLOCK), 0, stream, x, prm, out, H, W, c, vec);
  else if (C == 2) hipLaunchKernelGGL(crop_resize_kernel<2>, grid, dim3(CR_BLOCK), 0, stream, x, prm, out, H, W, c, vec);
  else hipLaunchKernelGGL(crop_resize_kernel<3>, grid, dim3(CR_BLOCK), 0, stream, x, prm, out, H, W, c, vec);
  return (int)hipGetLastError();
}

extern "C" int jr_selfsup_loss_blocks(long P) { return (int)std::min<long>(GRID_X, ((P + 1) / 2 + BLOCK - 1) / BLOCK); }

extern "C" int jr_selfsup_loss(const float* pred, const float* target, const float* weight, const float* prm, float* part,
                               int N, int B, int H, int W, int Btot, int B0, hipStream_t stream) {
  if (!loss_sizes_ok(B, H, W, N, Btot, B0) || !pred || !target || !prm || !part) return (int)hipErrorInvalidValue;
  const long HW = (long)H * W, P = B * HW, it_stride = Btot * HW, off = B0 * HW;
  const float* win = pred + 2 * off;
  const dim3 grid((unsigned)jr_selfsup_loss_blocks(P), iter_groups(N));
  if (loss_vec(pred, target, weight, nullptr, P, it_stride, off))
    hipLaunchKernelGGL(selfsup_loss_kernel<true>, grid, dim3(BLOCK), 0, stream, win, target, weight, prm, part, P, it_stride, N);
  else
    hipLaunchKernelGGL(selfsup_loss_kernel<false>, grid, dim3(BLOCK), 0, stream, win, target, weight, prm, part, P, it_stride, N);
  return (int)hipGetLastError();
}

extern "C" int jr_selfsup_loss_bwd(const float* pred, const float* target, const float* weight, const float* prm,
                                   const float* scale, float* grad, int N, int B, int H, int W, int Btot, int B0,
                                   hipStream_t stream) {
  if (!loss_sizes_ok(B, H, W, N, Btot, B0) || !pred || !target || !prm || !scale || !grad) return (int)hipErrorInvalidValue;
  const long HW = (long)H * W, P = B * HW, it_stride = Btot * HW, off = B0 * HW;
  const float* win = pred + 2 * off;
  const dim3 grid((unsigned)(((P + 1) / 2 + BLOCK - 1) / BLOCK), iter_groups(N));
  if (loss_vec(pred, target, weight, grad, P, it_stride, off))
    hipLaunchKernelGGL(selfsup_loss_bwd_kernel<true>, grid, dim3(BLOCK), 0, stream, win, target, weight, prm, scale, grad, P,
                       it_stride, N);
  else
    hipLaunchKernelGGL(selfsup_loss_bwd_kernel<false>, grid, dim3(BLOCK), 0, stream, win, target, weight, prm, scale, grad, P,
                       it_stride, N);
  return (int)hipGetLastError();
}
