// Flow validation metrics (eval/metrics.py:flow_metrics): a batch of predictions against ground
// truth -> per sample [sum of epe, valid pixels, epe < 1, < 3, < 5, outliers] in fp64, added to
// the running total of a split on the device.  The per-pixel arithmetic is the golden op's: the
// same fp32 operations in the same order, every product and sum rounded on its own (contraction
// is off for this file, below), so every count equals the golden op's bit for bit; the fp64 sums
// differ from it only in the order of their additions.
//
// sqrtf here is the correctly rounded one: clang compiles HIP with
// -fhip-fp32-correctly-rounded-divide-sqrt by default, and the code of this file shows it when it
// is compiled for gfx950 -- each square root is v_sqrt_f32 followed by the fix-up (two v_fma_f32
// residuals against the +-1 ulp neighbours and v_cndmask selects, with the scaling of small
// arguments around it); under -fno-hip-fp32-correctly-rounded-divide-sqrt no v_fma_f32 is left and
// the bare v_sqrt_f32 (1 ulp) is all that remains.  The fp64 division of the outlier test is IEEE
// (v_div_scale_f64 / v_div_fmas_f64 / v_div_fixup_f64).  tests/test_validation_gpu.py holds the
// boundary pixels, where a root that is one ulp off changes a count.
//
// Two launches, no atomics, no memset, bitwise repeatable:
//   1. partials: grid (blocks, samples), one thread per 4 consecutive pixels of a row of the
//      sample's own Hs x Ws rectangle; pred and gt have pitches of their own and are read with two
//      16-byte loads where the run starts on a 16-byte boundary, with 8-byte loads elsewhere; valid
//      bytes are read only when the plane is given (one 32-bit load where the run is aligned).
//      The fp64 epe sum goes thread -> wave (shuffles) -> block (4 LDS words); the five counts
//      travel in one 64-bit word of 12-bit fields (a block counts at most 1024 of each).  Every
//      block writes its own partial: [sum, packed counts].
//   2. finish: one block, a wave per sample; the wave loads 64 partials at a time (one coalesced
//      16-byte load per lane) and adds their sums in lane order, i.e. the sample's partials in block
//      order, into rows[n]; then thread 0 folds the samples in order into acc.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int RUN = 4;        // pixels per thread
constexpr int BLOCK = 256;    // threads per block of the partials kernel
constexpr int FIELD = 12;     // bits per packed count: BLOCK * RUN = 1024 < 4096
constexpr int FINISH = 256;   // threads of the finish kernel: a wave per sample, four at a time

// blocks that sample (Hs, Ws) occupies
__device__ __forceinline__ int sample_blocks(int Hs, int Ws) {
  const long items = (long)Hs * ((Ws + RUN - 1) / RUN);
  return (int)((items + BLOCK - 1) / BLOCK);
}

// the sample's rectangle, clamped into both maps whatever the device-side list says
__device__ __forceinline__ void sample_size(const int* __restrict__ sizes, int n, int Hp, int Wp, int Hg, int Wg,
                                            int& Hs, int& Ws) {
  Hs = max(0, min(sizes[2 * n], min(Hp, Hg)));
  Ws = max(0, min(sizes[2 * n + 1], min(Wp, Wg)));
}

// 4 consecutive pixels starting at p (8-byte aligned); only the first `count` are read
__device__ __forceinline__ void load_run(const float* __restrict__ p, int count, float2* v) {
  if (count == RUN && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    v[0] = make_float2(a.x, a.y); v[1] = make_float2(a.z, a.w);
    v[2] = make_float2(b.x, b.y); v[3] = make_float2(b.z, b.w);
    return;
  }
#pragma unroll
  for (int k = 0; k < RUN; ++k) v[k] = k < count ? *(const float2*)(p + 2 * k) : make_float2(0.f, 0.f);
}

// part: [B][gridDim.x][2] 8-byte words
__global__ __launch_bounds__(BLOCK) void flow_metrics_partial_kernel(const float* __restrict__ pred,
                                                                     const float* __restrict__ gt,
                                                                     const unsigned char* __restrict__ valid,
                                                                     const int* __restrict__ sizes,
                                                                     double* __restrict__ part, int Hp, int Wp, int Hg,
                                                                     int Wg) {
  __shared__ double psum[BLOCK / 64];
  __shared__ unsigned long long pcnt[BLOCK / 64];
  const int n = blockIdx.y;
  int Hs, Ws;
  sample_size(sizes, n, Hp, Wp, Hg, Wg, Hs, Ws);             // block-uniform
  if ((int)blockIdx.x >= sample_blocks(Hs, Ws)) return;     // the whole block: no barrier is skipped by a part of it
  const int runs = (Ws + RUN - 1) / RUN;
  const long item = (long)blockIdx.x * BLOCK + threadIdx.x;
  double sum = 0.0;
  unsigned long long cnt = 0;
  if (item < (long)Hs * runs) {
    const int y = (int)(item / runs);
    const int x = (int)(item % runs) * RUN;
    const int count = min(RUN, Ws - x);
    float2 p[RUN], g[RUN];
    load_run(pred + 2 * (((long)n * Hp + y) * Wp + x), count, p);
    load_run(gt + 2 * (((long)n * Hg + y) * Wg + x), count, g);
    unsigned on = 0x01010101u;
    if (valid) {
      const unsigned char* v = valid + ((long)n * Hg + y) * Wg + x;
      if (count == RUN && (reinterpret_cast<uintptr_t>(v) & 3) == 0) {
        on = *(const unsigned*)v;
      } else {
        on = 0;
        for (int k = 0; k < count; ++k) on |= (unsigned)v[k] << (8 * k);
      }
    }
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
      if (k >= count || ((on >> (8 * k)) & 0xffu) == 0) continue;
      const float dx = p[k].x - g[k].x, dy = p[k].y - g[k].y;
      const float d2 = dx * dx + dy * dy;
      const float epe = sqrtf(d2);
      const float m2 = g[k].x * g[k].x + g[k].y * g[k].y;
      const float mag = sqrtf(m2);
      sum += (double)epe;
      cnt += 1ull;
      if (epe < 1.f) cnt += 1ull << FIELD;
      if (epe < 3.f) cnt += 1ull << (2 * FIELD);
      if (epe < 5.f) cnt += 1ull << (3 * FIELD);
      if (epe > 3.f && (double)epe / (double)mag > 0.05) cnt += 1ull << (4 * FIELD);   // x / 0 = inf: an outlier
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, 64);
    cnt += __shfl_down(cnt, off, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { psum[wave] = sum; pcnt[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* out = part + 2 * ((long)n * gridDim.x + blockIdx.x);
    out[0] = (psum[0] + psum[1]) + (psum[2] + psum[3]);
    out[1] = __longlong_as_double((long long)((pcnt[0] + pcnt[1]) + (pcnt[2] + pcnt[3])));
  }
}

// v of lane l (a constant after unrolling), broadcast to the wave through scalar registers
__device__ __forceinline__ double lane_value(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// rows fp64 [B][6], acc fp64 [8]; NB: the partials kernel's gridDim.x
__global__ __launch_bounds__(FINISH) void flow_metrics_finish_kernel(const double* __restrict__ part,
                                                                     const int* __restrict__ sizes,
                                                                     double* __restrict__ rows, double* __restrict__ acc,
                                                                     int B, int NB, int Hp, int Wp, int Hg, int Wg) {
  const int lane = threadIdx.x & 63;
  for (int n = threadIdx.x >> 6; n < B; n += FINISH / 64) {   // a wave per sample
    int Hs, Ws;
    sample_size(sizes, n, Hp, Wp, Hg, Wg, Hs, Ws);
    const int nb = min(sample_blocks(Hs, Ws), NB);
    const double2* p = (const double2*)part + (long)n * NB;
    double sum = 0.0;
    long long c[5] = {0, 0, 0, 0, 0};
    for (int b0 = 0; b0 < nb; b0 += 64) {                   // 64 partials per coalesced load
      const bool in = b0 + lane < nb;
      const double2 v = in ? p[b0 + lane] : make_double2(0.0, 0.0);
      // block order: every lane adds the 64 sums in lane order (x + 0.0 == x past the end), so the
      // sum is a function of the inputs alone
#pragma unroll
      for (int l = 0; l < 64; ++l) sum += lane_value(v.x, l);
      const unsigned long long w = in ? (unsigned long long)__double_as_longlong(v.y) : 0ull;
#pragma unroll
      for (int k = 0; k < 5; ++k) c[k] += (long long)((w >> (FIELD * k)) & ((1u << FIELD) - 1));
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) c[k] += __shfl_down(c[k], off, 64);
    if (lane == 0) {
      double* r = rows + 6 * n;
      r[0] = sum;
#pragma unroll
      for (int k = 0; k < 5; ++k) r[1 + k] = (double)c[k];
    }
  }
  __syncthreads();                                          // rows, written by this block, are read back by thread 0
  if (threadIdx.x != 0) return;
  double tot[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int n = 0; n < B; ++n) {                             // the samples in order
    const double* r = rows + 6 * n;
#pragma unroll
    for (int k = 0; k < 6; ++k) tot[k] += r[k];
    tot[6] += r[0] / fmax(r[1], 1.0);
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) acc[k] += tot[k];
  acc[7] += (double)B;
}

}  // namespace

extern "C" int jr_flow_metrics(const float* pred, const float* gt, const void* valid, const int* sizes, double* part,
                               double* rows, double* acc, int B, int Hp, int Wp, int Hg, int Wg, int NB,
                               hipStream_t stream) {
  if (B < 1 || B > 65535 || Hp < 1 || Wp < 1 || Hg < 1 || Wg < 1 || NB < 1 || (long)Hp * Wp > 0x3fffffffL ||
      (long)Hg * Wg > 0x3fffffffL || !pred || !gt || !sizes || !part || !rows || !acc)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(flow_metrics_partial_kernel, dim3((unsigned)NB, (unsigned)B), dim3(BLOCK), 0, stream, pred, gt,
                     (const unsigned char*)valid, sizes, part, Hp, Wp, Hg, Wg);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(flow_metrics_finish_kernel, dim3(1), dim3(FINISH), 0, stream, (const double*)part, sizes, rows,
                     acc, B, NB, Hp, Wp, Hg, Wg);
  return (int)hipGetLastError();
}
