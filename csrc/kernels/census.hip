// Soft census photometric term of the label-free loss (train/unsup.py:census_sums; the census
// loss of UnFlow / SMURF with SMURF's constants): a 7x7 stencil over image 1's grey plane and over
// image 2's grey plane *warped* by every iteration's prediction.  Three kernels, no atomics,
// bitwise repeatable.
//
// pred fp32 [N][B][H][W][2] (channel 0 = x), gray fp32 [2][B][H][W] (G1, G2), mask (optional) fp32
// [B][H][W], used where >= 0.5, prm fp32 [4] = (eps, eps_s, edge_kappa, out_penalty) on the device
// (only out_penalty is read).  Per pixel q and iteration i, with f = pred[i][b][q]:
//   px = float(x) + f.x, py = float(y) + f.y; inside iff 0 <= px <= W-1 and 0 <= py <= H-1 (NaN
//   fails); pxc = min(px >= 0 ? px : 0, W-1) (NaN -> 0), x0 = floor(pxc), x1 = min(x0+1, W-1),
//   wx = pxc - x0, y alike; w(q) = t + wy (b - t), t = c00 + wx (c01 - c00), b = c10 + wx (c11 - c10)
//   on G2: a pixel that lands outside has the border's grey (and no derivative);
//   tau(D) = D / sqrt(0.81 + D^2) (as D * rsq); for the 48 offsets d != 0 of the 7x7 patch
//   e_d = (tau(G1(p+d) - G1(p)) - tau(w(p+d) - w(p)))^2, h(p) = sum_d e_d / (0.1 + e_d),
//   cen(p) = (h(p) + 0.01)^0.4;
//   valid(p) = inside(p) and 3 <= x < W-3 and 3 <= y < H-3; term(p) = cen(p) where valid,
//   out_penalty where not inside, 0 in the border band; + 0 * (f.x + f.y), so that a non-finite flow
//   poisons its iteration's sum whatever the mask says.
//
//   1. census_gray_kernel: G = 127.5 ((0.299 r + 0.587 g) + 0.114 b) of both images, once per call.
//   2. census_loss_kernel: a block owns a TX x TY pixel tile of one batch sample for ITERS
//      iterations.  It stages G1 and the *computed* w of every iteration of the group for the tile
//      plus a 3-pixel halo in LDS (a halo pixel recomputes its bilinear sample: four cached 4-byte
//      gathers; positions outside the frame hold 0 and are read only by pixels that are not valid),
//      then every thread walks the 48 offsets of its pixel out of LDS: tau of the G1 difference once
//      per offset, the warped part once per offset and iteration.  TX = 32: one 32-lane half of a
//      wave reads 32 consecutive words of one LDS row, whatever the offset, so the shifted reads
//      (ds_read_b32: banks modulo 32 per half) have no bank conflict and the rows need no padding.
//      Output: one row part[tile][i][4] per tile and iteration (loss_common.h's reduction):
//      (sum of mask * term, masked pixels that are not inside, masked pixels inside but in
//      the band, sum of cen over the valid masked pixels -- the last iteration only, 0 elsewhere),
//      and the plane coef[i][q] = mask valid 0.4 (h + 0.01)^-0.6 for the backward.  Counts are at
//      most TX * TY per row: exact.
//   3. census_loss_bwd_kernel: the same tile, with coef staged too.  With D1, D2, e of pixel q and
//      offset d as in the forward, kappa(q, d) = k'(e) 2 (tau(D2) - tau(D1)) tau'(D2),
//      k'(e) = 0.1 / (0.1 + e)^2, tau'(D) = 0.81 / (0.81 + D^2)^1.5, the derivative of the sum in
//      w(q) is sum_d [coef(q-d) kappa_(q-d)(q) - coef(q) kappa(q, d)].  tau is odd and tau' even, so
//      kappa_(q+d)(q) = -kappa(q, d) exactly, in fp32 too, and the gather is
//      A(q) = -sum_d (coef(q) + coef(q+d)) kappa(q, d): 48 evaluations, not 96.  coef is 0 outside
//      the frame and wherever a pixel is not valid, so every product is finite.  The thread then
//      writes (add = 0) or adds (add = 1) scale[i] A(q) (dw/dwx, dw/dwy)(q) where inside(q), 0
//      elsewhere, to grad[i][q]: each element is owned by one thread.
//   The per-element order of products and sums depends on neither the tile nor the block.
#include "kernels.h"
#include "loss_common.h"

namespace {

using namespace loss;

constexpr int TX = 32, TY = 8;            // the pixel tile of a block; TX * TY threads
constexpr int R = 3;                      // patch radius
constexpr int LW = TX + 2 * R, LH = TY + 2 * R;
constexpr int LN = LW * LH;
static_assert(TX * TY == BLOCK, "one thread per pixel of the tile");
constexpr float C_TAU = 0.81f, C_K = 0.1f, C_H = 0.01f;

// The hardware's reciprocal and reciprocal square root (1 ulp; the arguments are at least 0.1 and
// 0.81, far from any denormal): the 48 x ITERS inner loop is arithmetic bound, and IEEE division
// and square root cost it about three times as many instructions.
__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float tau(float d) { return d * rsq(C_TAU + d * d); }

// The warped grey value at pixel (y, x) with flow f; g2 is the sample's G2 plane.  dwx / dwy are
// the derivatives in wx / wy.
__device__ __forceinline__ float warp_gray(float2 f, int y, int x, int H, int W, const float* __restrict__ g2, bool& inside,
                                           float& dwx, float& dwy) {
  const float px = (float)x + f.x, py = (float)y + f.y;
  inside = JR_INSIDE_FRAME(px, py, H, W);
  const float pxc = fminf(px >= 0.f ? px : 0.f, (float)(W - 1));    // NaN -> 0
  const float pyc = fminf(py >= 0.f ? py : 0.f, (float)(H - 1));
  const float x0f = floorf(pxc), y0f = floorf(pyc);
  const float wx = pxc - x0f, wy = pyc - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;                            // in [0, W-1] x [0, H-1]
  const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
  const float c00 = g2[(long)y0 * W + x0], c01 = g2[(long)y0 * W + x1];
  const float c10 = g2[(long)y1 * W + x0], c11 = g2[(long)y1 * W + x1];
  const float t = c00 + wx * (c01 - c00);
  const float b = c10 + wx * (c11 - c10);
  dwx = (1.f - wy) * (c01 - c00) + wy * (c11 - c10);
  dwy = b - t;
  return t + wy * (b - t);
}

// gray fp32 [2][P]
__global__ __launch_bounds__(256) void census_gray_kernel(const float* __restrict__ img1, const float* __restrict__ img2,
                                                          float* __restrict__ gray, long P) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const float* a = img1 + 3 * p;
  const float* b = img2 + 3 * p;
  gray[p] = 127.5f * ((0.299f * a[0] + 0.587f * a[1]) + 0.114f * a[2]);
  gray[P + p] = 127.5f * ((0.299f * b[0] + 0.587f * b[1]) + 0.114f * b[2]);
}

// The tile of a block: sample b, origin (ty0, tx0).
__device__ __forceinline__ void tile_of(int tiles_x, int tiles_y, int& b, int& ty0, int& tx0) {
  const int t = (int)blockIdx.x;
  tx0 = (t % tiles_x) * TX;
  ty0 = ((t / tiles_x) % tiles_y) * TY;
  b = t / (tiles_x * tiles_y);
}

// Stages G1 (and, backward, coef) and the warped planes of iterations i0 .. i0 + ITERS - 1 for the
// tile plus halo; 0 outside the frame.
template <bool BWD>
__device__ __forceinline__ void stage(float (*sw)[LN], float* sg, float (*sc)[LN], const float* __restrict__ pred,
                                      const float* __restrict__ g1, const float* __restrict__ g2,
                                      const float* __restrict__ coef, int b, int ty0, int tx0, int H, int W, long P, int N,
                                      int i0) {
  const long HW = (long)H * W;
  for (int j = threadIdx.x; j < LN; j += BLOCK) {
    const int ly = j / LW, lx = j - ly * LW;
    const int y = ty0 + ly - R, x = tx0 + lx - R;
    const bool in_frame = y >= 0 && y < H && x >= 0 && x < W;
    const long p = b * HW + (long)y * W + x;
    sg[j] = in_frame ? g1[p] : 0.f;
#pragma unroll
    for (int k = 0; k < ITERS; ++k) {
      const int i = i0 + k;
      float w = 0.f, c = 0.f;
      if (in_frame && i < N) {
        bool inside;
        float dwx, dwy;
        w = warp_gray(*(const float2*)(pred + 2 * ((long)i * P + p)), y, x, H, W, g2 + b * HW, inside, dwx, dwy);
        if (BWD) c = coef[(long)i * P + p];
      }
      sw[k][j] = w;
      if (BWD) sc[k][j] = c;
    }
  }
}

// part fp32 [tiles][N][4], coef fp32 [N][P]
__global__ __launch_bounds__(BLOCK) void census_loss_kernel(const float* __restrict__ pred, const float* __restrict__ gray,
                                                            const float* __restrict__ mask, const float* __restrict__ prm,
                                                            float* __restrict__ part, float* __restrict__ coef, int H, int W,
                                                            long P, int N, int tiles_x, int tiles_y) {
  constexpr int Q = 3 * ITERS + 1;
  __shared__ float sw[ITERS][LN];
  __shared__ float sg[LN];
  __shared__ float red[Q][BLOCK / 64];
  const float out_pen = prm[3];
  const int i0 = (int)blockIdx.y * ITERS;                    // block-uniform
  int b, ty0, tx0;
  tile_of(tiles_x, tiles_y, b, ty0, tx0);
  const long HW = (long)H * W;
  stage<false>(sw, sg, nullptr, pred, gray, gray + P, nullptr, b, ty0, tx0, H, W, P, N, i0);
  __syncthreads();
  const int lx = threadIdx.x % TX, ly = threadIdx.x / TX;
  const int x = tx0 + lx, y = ty0 + ly;
  float acc[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) acc[k] = 0.f;
  if (x < W && y < H) {
    const long p = b * HW + (long)y * W + x;
    const int c = (ly + R) * LW + lx + R;
    const float gc = sg[c];
    float wc[ITERS], h[ITERS];
#pragma unroll
    for (int k = 0; k < ITERS; ++k) {
      wc[k] = sw[k][c];
      h[k] = 0.f;
    }
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
      for (int dx = -R; dx <= R; ++dx) {
        if (dx == 0 && dy == 0) continue;
        const int n = c + dy * LW + dx;
        const float t1 = tau(sg[n] - gc);
#pragma unroll
        for (int k = 0; k < ITERS; ++k) {
          const float d = t1 - tau(sw[k][n] - wc[k]);
          const float e = d * d;
          h[k] += e * rcp(C_K + e);
        }
      }
    }
    const bool on = mask == nullptr || mask[p] >= 0.5f;
    const float m = on ? 1.f : 0.f;
    const bool geom = x >= R && x < W - R && y >= R && y < H - R;
#pragma unroll
    for (int k = 0; k < ITERS; ++k) {
      const int i = i0 + k;
      if (i >= N) break;
      const float2 f = *(const float2*)(pred + 2 * ((long)i * P + p));
      const float px = (float)x + f.x, py = (float)y + f.y;
      const bool inside = JR_INSIDE_FRAME(px, py, H, W);
      const bool valid = inside && geom;
      const float hh = h[k] + C_H;
      const float cen = powf(hh, 0.4f);
      const float term = valid ? cen : (inside ? 0.f : out_pen);
      acc[k] += m * term + 0.f * (f.x + f.y);               // NaN for a non-finite flow, whatever the mask
      acc[ITERS + k] += (on && !inside) ? 1.f : 0.f;
      acc[2 * ITERS + k] += (on && inside && !geom) ? 1.f : 0.f;
      if (i == N - 1 && on && valid) acc[3 * ITERS] += cen;
      coef[(long)i * P + p] = (on && valid) ? 0.4f * cen / hh : 0.f;
    }
  }
  block_sums(acc, red);
  int k, i;
  if (owns_row(i0, N, k, i))
    store_row(part, N, i, row_total(red[k]), row_total(red[ITERS + k]), row_total(red[2 * ITERS + k]),
              i == N - 1 ? row_total(red[3 * ITERS]) : 0.f);
}

// scale fp32 [N]; grad fp32 [N][P][2]
__global__ __launch_bounds__(BLOCK) void census_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gray,
                                                                const float* __restrict__ coef, const float* __restrict__ scale,
                                                                float* __restrict__ grad, int H, int W, long P, int N,
                                                                int tiles_x, int tiles_y, int add) {
  __shared__ float sw[ITERS][LN];
  __shared__ float sc[ITERS][LN];
  __shared__ float sg[LN];
  const int i0 = (int)blockIdx.y * ITERS;
  int b, ty0, tx0;
  tile_of(tiles_x, tiles_y, b, ty0, tx0);
  const long HW = (long)H * W;
  stage<true>(sw, sg, sc, pred, gray, gray + P, coef, b, ty0, tx0, H, W, P, N, i0);
  __syncthreads();
  const int lx = threadIdx.x % TX, ly = threadIdx.x / TX;
  const int x = tx0 + lx, y = ty0 + ly;
  if (x >= W || y >= H) return;
  const long p = b * HW + (long)y * W + x;
  const int c = (ly + R) * LW + lx + R;
  const float gc = sg[c];
  float wc[ITERS], cc[ITERS], a[ITERS];
#pragma unroll
  for (int k = 0; k < ITERS; ++k) {
    wc[k] = sw[k][c];
    cc[k] = sc[k][c];
    a[k] = 0.f;
  }
  for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      if (dx == 0 && dy == 0) continue;
      const int n = c + dy * LW + dx;
      const float t1 = tau(sg[n] - gc);
#pragma unroll
      for (int k = 0; k < ITERS; ++k) {
        const float d2 = sw[k][n] - wc[k];
        const float ri = rsq(C_TAU + d2 * d2);
        const float df = d2 * ri - t1;                      // tau(D2) - tau(D1)
        const float ki = rcp(C_K + df * df);
        const float kappa = (C_K * (ki * ki)) * (2.f * df) * (C_TAU * (ri * ri * ri));
        a[k] -= (cc[k] + sc[k][n]) * kappa;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < ITERS; ++k) {
    const int i = i0 + k;
    if (i >= N) break;
    const long at = 2 * ((long)i * P + p);
    bool inside;
    float dwx, dwy;
    warp_gray(*(const float2*)(pred + at), y, x, H, W, gray + P + b * HW, inside, dwx, dwy);
    const float s = scale[i] * a[k];
    // (rounded products: add = 1 is then bitwise the written gradient added to what grad holds)
    float2 g = inside ? make_float2(__fmul_rn(s, dwx), __fmul_rn(s, dwy)) : make_float2(0.f, 0.f);
    if (add) {
      const float2 o = *(const float2*)(grad + at);
      g.x += o.x;
      g.y += o.y;
    }
    *(float2*)(grad + at) = g;
  }
}

}  // namespace

extern "C" long jr_census_tiles(int B, int H, int W) { return (long)B * ((H + TY - 1) / TY) * ((W + TX - 1) / TX); }

extern "C" int jr_census_gray(const float* img1, const float* img2, float* gray, int B, int H, int W, hipStream_t stream) {
  if (!sizes_ok(B, H, W, 1) || !img1 || !img2 || !gray) return (int)hipErrorInvalidValue;
  const long P = (long)B * H * W;
  hipLaunchKernelGGL(census_gray_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, img1, img2, gray, P);
  return (int)hipGetLastError();
}

extern "C" int jr_census_loss(const float* pred, const float* gray, const float* mask, const float* prm, float* part,
                              float* coef, int B, int H, int W, int N, hipStream_t stream) {
  if (!sizes_ok(B, H, W, N) || !pred || !gray || !prm || !part || !coef) return (int)hipErrorInvalidValue;
  const int tiles_x = (W + TX - 1) / TX, tiles_y = (H + TY - 1) / TY;
  hipLaunchKernelGGL(census_loss_kernel, dim3((unsigned)jr_census_tiles(B, H, W), iter_groups(N)),
                     dim3(BLOCK), 0, stream, pred, gray, mask, prm, part, coef, H, W, (long)B * H * W, N, tiles_x, tiles_y);
  return (int)hipGetLastError();
}

extern "C" int jr_census_loss_bwd(const float* pred, const float* gray, const float* coef, const float* scale, float* grad,
                                  int B, int H, int W, int N, int add, hipStream_t stream) {
  if (!sizes_ok(B, H, W, N) || !pred || !gray || !coef || !scale || !grad) return (int)hipErrorInvalidValue;
  const int tiles_x = (W + TX - 1) / TX, tiles_y = (H + TY - 1) / TY;
  hipLaunchKernelGGL(census_loss_bwd_kernel, dim3((unsigned)jr_census_tiles(B, H, W), iter_groups(N)),
                     dim3(BLOCK), 0, stream, pred, gray, coef, scale, grad, H, W, (long)B * H * W, N, tiles_x, tiles_y, add);
  return (int)hipGetLastError();
}
