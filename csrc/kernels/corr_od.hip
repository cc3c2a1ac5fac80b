// On-demand correlation lookup (gfx950): the lookup op's output computed from the two
// feature maps, without the all-pairs volume (original RAFT's alternate_corr).  Memory is
// O(P * C) instead of O(P^2).
//
// Golden op: models/reference.py:index_on_demand.  Pooling is linear, so the correlation of a
// query with a level-l cell of the pooled volume equals its correlation with the level-l pooled
// target features.
//
// feat_pool_kernel (prologue, once per call): levels 1 .. L-1 of the target features, each the
// 2x2 VALID mean of the level below, accumulated and stored in fp32 (floor sizes: a cell exists
// iff its whole footprint is inside the map).  One thread per (8x8 level-0 block, channel)
// forms the block's 4x4 / 2x2 / 1 cells of levels 1 / 2 / 3 in registers.
//
// lookup_od_kernel (loop): one wave per query pixel.  Per level the (2r+2)^2 integer cells
// around floor(coords / 2^l) - r; a group of 16 lanes forms one cell's dot product over C
// (lane `sub` owns the 8-channel chunks sub, sub + 16, ..; fp32 FMAs, then an xor tree over
// the 16 lanes), four cells per step.  The scaled values go to an LDS window image, from which
// the (2r+1)^2 samples are blended as corr_lookup_kernel blends them (vertical, then
// horizontal) and written as bf16 rows in the reference channel order l*S^2 + i*S + j,
// zero-padded to the consumer's channel stride.  No atomics: every output element has one
// writer and a fixed summation order, so runs are bitwise repeatable.
#include <cstdint>

#include "common.h"
#include "kernels.h"
#include "lookup_coords.h"

namespace {

struct PoolPtrs {
  float* p[3];   // levels 1, 2, 3
};

__global__ __launch_bounds__(128) void feat_pool_kernel(const bf16* __restrict__ f2, int h, int w, int C, int cs,
                                                        PoolPtrs pp, int nlev, int nby, int nbx) {
  const int bx = blockIdx.x % nbx, by = (blockIdx.x / nbx) % nby, b = blockIdx.x / (nbx * nby);
  const int h1 = h >> 1, w1 = w >> 1, h2 = h1 >> 1, w2 = w1 >> 1, h3 = h2 >> 1, w3 = w2 >> 1;
  const bf16* src = f2 + (long)b * h * w * cs;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float v1[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int Y = 4 * by + a, X = 4 * bx + d;
        float v = 0.f;
        if (Y < h1 && X < w1) {   // 2Y + 1 <= h - 1, 2X + 1 <= w - 1
          const bf16* s = src + ((long)(2 * Y) * w + 2 * X) * cs + c;
          v = 0.25f * ((bf2f(s[0]) + bf2f(s[cs])) + (bf2f(s[(long)w * cs]) + bf2f(s[(long)(w + 1) * cs])));
          pp.p[0][(((long)b * h1 + Y) * w1 + X) * C + c] = v;
        }
        v1[a][d] = v;
      }
    if (nlev < 3) continue;
    float v2[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const int Y = 2 * by + a, X = 2 * bx + d;
        float v = 0.f;
        if (Y < h2 && X < w2) {   // its four level-1 cells exist: 2 * h2 <= h1
          v = 0.25f * ((v1[2 * a][2 * d] + v1[2 * a][2 * d + 1]) + (v1[2 * a + 1][2 * d] + v1[2 * a + 1][2 * d + 1]));
          pp.p[1][(((long)b * h2 + Y) * w2 + X) * C + c] = v;
        }
        v2[a][d] = v;
      }
    if (nlev < 4) continue;
    if (by < h3 && bx < w3)
      pp.p[2][(((long)b * h3 + by) * w3 + bx) * C + c] = 0.25f * ((v2[0][0] + v2[0][1]) + (v2[1][0] + v2[1][1]));
  }
}

struct PoolCPtrs {
  const float* p[3];
};

// The integer window base of a coordinate.  Any float (far outside, inf, NaN) is clamped HERE,
// before the conversion to int and before anything is added to it, so the window indices below
// are small integers; a cell index is used in address arithmetic only after it has been checked
// against the level size.
JR_DEVICE int window_base(float fl, int R) { return (int)fminf(fmaxf(fl, -1048576.f), 1048576.f) - R; }

// blockDim = 256: 4 waves, one query each.  NCH: 8-channel chunks per lane (C <= 128 * NCH).
template <int R, int NCH>
__global__ __launch_bounds__(256) void lookup_od_kernel(const bf16* __restrict__ f1, const bf16* __restrict__ f2,
                                                        int fcs, PoolCPtrs pl, int nlev, int total, int h, int w, int C,
                                                        float scale, const float* coords, bf16* __restrict__ out,
                                                        int ocs, TapsUpd upd) {
  constexpr int S = 2 * R + 1, W1 = S + 1, NC = W1 * W1, NSTEP = (NC + 3) / 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x * 4 + wave;
  float* wn = (float*)dyn_smem + wave * 4 * NC;                        // [4 levels][W1][W1]
  bf16* st = (bf16*)(dyn_smem + 16 * NC * sizeof(float)) + wave * ocs;   // [ocs]
  for (int c = lane; c < ocs; c += 64) st[c] = f2bf(0.f);
  float qcx[1], qcy[1];
  lookup_coords<1>(upd, coords, q, total, h, w, lane, qcx, qcy);
  const bool qok = q < total;
  const int g = lane >> 4, sub = lane & 15;
  const int nchunk = C >> 3;
  const int hw = h * w;
  const int b = qok ? q / hw : 0;
  float a[NCH][8];
#pragma unroll
  for (int n = 0; n < NCH; ++n) {
    const int ch = sub + 16 * n;
    bf16x8 v = {};
    if (qok && ch < nchunk) v = *(const bf16x8*)(f1 + (long)q * fcs + ch * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[n][e] = bf2f(v[e]);
  }
  for (int l = 0; l < nlev; ++l) {
    const int hl = h >> l, wl = w >> l;
    const float sc = 1.0f / (float)(1 << l);
    const int col0 = window_base(floorf(qcx[0] * sc), R);
    const int row0 = window_base(floorf(qcy[0] * sc), R);
    const float* lvf = l ? pl.p[l - 1] + (long)b * hl * wl * C : nullptr;
    // not unrolled: 58 VGPRs at r = 4, C = 256 (8 waves per SIMD, the whole 440 x 1024 grid resident
    // at once) measured 77 us per launch against 110 us for the 5-fold unrolled loop at 84 VGPRs
#pragma unroll 1
    for (int s = 0; s < NSTEP; ++s) {
      const int cell = s * 4 + g;
      const int j = cell / W1, i = cell - j * W1;   // window row (y), column (x)
      const int y = row0 + j, x = col0 + i;
      const bool ok = qok && cell < NC && (unsigned)y < (unsigned)hl && (unsigned)x < (unsigned)wl;
      float acc = 0.f;
      if (ok) {   // (y, x) is a cell of the level map: the only place an address is formed from it
        if (l == 0) {
          const bf16* src = f2 + ((long)b * hw + y * w + x) * fcs;
#pragma unroll
          for (int n = 0; n < NCH; ++n) {
            const int ch = sub + 16 * n;
            if (ch < nchunk) {
              const bf16x8 v = *(const bf16x8*)(src + ch * 8);
#pragma unroll
              for (int e = 0; e < 8; ++e) acc = fmaf(a[n][e], bf2f(v[e]), acc);
            }
          }
        } else {
          const float* src = lvf + (long)(y * wl + x) * C;
#pragma unroll
          for (int n = 0; n < NCH; ++n) {
            const int ch = sub + 16 * n;
            if (ch < nchunk) {
              const f32x4 v0 = *(const f32x4*)(src + ch * 8), v1 = *(const f32x4*)(src + ch * 8 + 4);
#pragma unroll
              for (int e = 0; e < 4; ++e) acc = fmaf(a[n][e], v0[e], acc);
#pragma unroll
              for (int e = 0; e < 4; ++e) acc = fmaf(a[n][4 + e], v1[e], acc);
            }
          }
        }
      }
      acc += __shfl_xor(acc, 8);
      acc += __shfl_xor(acc, 4);
      acc += __shfl_xor(acc, 2);
      acc += __shfl_xor(acc, 1);
      if (sub == 0 && cell < NC) wn[l * NC + cell] = acc * scale;
    }
  }
  __syncthreads();   // window images written, staging row zeroed
  if (qok) {
    for (int o = lane; o < nlev * S * S; o += 64) {
      const int l = o / (S * S), r = o - l * S * S;
      const int i = r / S, j = r - i * S;   // x offset i - R is the slow index
      const float sc = 1.0f / (float)(1 << l);
      const float cx = qcx[0] * sc, cy = qcy[0] * sc;
      const float fx = cx - floorf(cx), fy = cy - floorf(cy);
      const float* c = wn + l * NC + j * W1 + i;
      const float v0 = (1.f - fy) * c[0] + fy * c[W1];
      const float v1 = (1.f - fy) * c[1] + fy * c[W1 + 1];
      st[o] = f2bf((1.f - fx) * v0 + fx * v1);
    }
  }
  __syncthreads();
  if (qok) {
    bf16* dst = out + (long)q * ocs;
    for (int c = lane * 8; c < ocs; c += 64 * 8) *(u32x4*)(dst + c) = *(const u32x4*)(st + c);
  }
}

template <int NCH>
int launch_od(const bf16* f1, const bf16* f2, int fcs, const PoolCPtrs& pl, int L, int total, int h, int w, int C,
              int r, float scale, const float* coords, bf16* out, int ocs, const TapsUpd& upd, hipStream_t stream) {
  dim3 grid((total + 3) / 4);
  const int W1 = 2 * r + 2;
  const size_t smem = 16 * W1 * W1 * sizeof(float) + 4 * (size_t)ocs * sizeof(bf16);
  switch (r) {
#define JR_OD(RR)                                                                                                    \
  case RR:                                                                                                           \
    hipLaunchKernelGGL((lookup_od_kernel<RR, NCH>), grid, dim3(256), smem, stream, f1, f2, fcs, pl, L, total, h, w, C, \
                       scale, coords, out, ocs, upd);                                                                \
    break;
    JR_OD(1) JR_OD(2) JR_OD(3) JR_OD(4)
#undef JR_OD
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" int jr_feat_pool(const void* f2, int B, int h, int w, int C, int cs, float* p1, float* p2, float* p3,
                            int num_levels, hipStream_t stream) {
  if (num_levels < 1 || num_levels > 4 || C < 64 || C % 64 != 0 || cs < C || B < 1) return (int)hipErrorInvalidValue;
  if ((h >> (num_levels - 1)) < 2 || (w >> (num_levels - 1)) < 2) return (int)hipErrorInvalidValue;
  if (num_levels == 1) return (int)hipSuccess;
  PoolPtrs pp{{p1, p2, p3}};
  for (int l = 1; l < num_levels; ++l)
    if (!pp.p[l - 1]) return (int)hipErrorInvalidValue;
  const int nby = ((h >> 1) + 3) / 4, nbx = ((w >> 1) + 3) / 4;
  hipLaunchKernelGGL(feat_pool_kernel, dim3(B * nby * nbx), dim3(C < 128 ? 64 : 128), 0, stream, (const bf16*)f2, h, w,
                     C, cs, pp, num_levels, nby, nbx);
  return (int)hipGetLastError();
}

extern "C" int jr_lookup_od(const void* f1, const void* f2, int fcs, const float* p1, const float* p2, const float* p3,
                            int num_levels, int B, int h, int w, int C, int radius, float scale, const float* coords,
                            void* out, int out_cstride, hipStream_t stream, const TapsUpd* upd) {
  const int S = 2 * radius + 1;
  if (num_levels < 1 || num_levels > 4 || radius < 1 || radius > 4 || out_cstride % 8 != 0 ||
      out_cstride < num_levels * S * S || C < 64 || C % 64 != 0 || C > 512 || fcs % 8 != 0 || fcs < C || B < 1)
    return (int)hipErrorInvalidValue;
  if ((h >> (num_levels - 1)) < 2 || (w >> (num_levels - 1)) < 2) return (int)hipErrorInvalidValue;
  PoolCPtrs pl{{p1, p2, p3}};
  if (!aligned16(f1) || !aligned16(f2) || !aligned16(out)) return (int)hipErrorInvalidValue;
  for (int l = 1; l < num_levels; ++l)
    if (!pl.p[l - 1] || !aligned16(pl.p[l - 1])) return (int)hipErrorInvalidValue;
  TapsUpd u{};
  if (upd && upd->on) {
    if (!upd->taps || upd->tcs < 18 || !upd->bias || upd->coords != coords || !upd->flow32 || !upd->hx)
      return (int)hipErrorInvalidValue;
    u = *upd;
  }
  const int total = B * h * w;
  if (C <= 128)
    return launch_od<1>((const bf16*)f1, (const bf16*)f2, fcs, pl, num_levels, total, h, w, C, radius, scale, coords,
                        (bf16*)out, out_cstride, u, stream);
  if (C <= 256)
    return launch_od<2>((const bf16*)f1, (const bf16*)f2, fcs, pl, num_levels, total, h, w, C, radius, scale, coords,
                        (bf16*)out, out_cstride, u, stream);
  return launch_od<4>((const bf16*)f1, (const bf16*)f2, fcs, pl, num_levels, total, h, w, C, radius, scale, coords,
                      (bf16*)out, out_cstride, u, stream);
}
