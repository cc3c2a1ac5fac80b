// Frame interpolation from a bidirectional flow pair by forward splatting: every pixel of both frames
// is pushed along a fraction of its own flow, and what meets in a cell of the frame at time t is
// normalised.  The semantics are the golden op's (models/reference.py:interpolate_frames) and the
// kernels equal it bit for bit, the accumulator included: the landing point is one fp32 product and
// one fp32 sum per axis, each rounded on its own (contraction is off for this file, below), its
// fraction is quantised to 1/16 per axis (occlusion.hip's steps), and everything after that is
// INTEGER arithmetic, so the sums do not depend on the order of the atomics.  No float atomics, no
// LDS, no host synchronisation; they ride at the end of a bidirectional plan after fb_check.
//   interp_splat:   both directions in one launch, grid (blocks of 64 source pixels, 2 B), FOUR
//                   neighbouring lanes per source pixel of the FRAME (not of the padded map), lane q
//                   adding quantity q of (w k, w k R, w k G, w k B): the 8-byte load of the pixel's
//                   flow and its mask byte (the same address in the four lanes: one access), one
//                   colour byte, the range test in float before any conversion; per tap of weight
//                   != 0 inside the frame one 64-bit integer atomic add per lane, so ONE wave
//                   instruction adds the 32 contiguous bytes of a cell of acc [2][B][H0][W0][4] int64
//                   for 16 sources (one thread per source issuing the four adds one after the other
//                   touches 64 cells with 8 bytes each per instruction: measured slower, see
//                   profiles/interp_splat_lanes_ab.txt).  No address is formed for a tap outside the
//                   frame.  The caller clears acc (a plan: its memset op, recorded just before).
//   interp_resolve: grid (blocks, B) over the frame, one thread per pixel: two 16-byte loads per
//                   direction, the integer blend D = a0 acc0.w + a1 acc1.w, N_c likewise,
//                   v_c = (2 N_c + D) / (2 D), the hole test D < Dmin; the fallback texel is read only
//                   where the pixel is a hole.  Byte stores, so any W0 works without a padded copy.
// (tq, Dmin) of the time are read from an int32 device tensor par [K][2], row k: another t or
// min_cover changes no kernel argument, so a captured plan serves every time.
// Bound: one contribution is below 2^20 (256 * 16 * 255) and H0 * W0 <= 2^30, so a cell stays below
// 2^50 and 2 N + D below 2^61, whatever the flow.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr unsigned long long CONSISTENT = 16;   // models/reference.py:CONSISTENT (an occluded source: 1)

typedef unsigned long long u64;

// grid (ceil(4 * H0 * W0 / 256), 2 B): map m = d * B + b splats frame d with flow d into acc[m];
// thread t serves source pixel t / 4 and quantity t % 4
__global__ __launch_bounds__(BLOCK) void interp_splat_kernel(
    const unsigned char* __restrict__ frame0, const unsigned char* __restrict__ frame1, const float* __restrict__ flow0,
    const float* __restrict__ flow1, const long long* __restrict__ slot, long off0, long off1,
    const unsigned char* __restrict__ occ, u64* __restrict__ acc, const int* __restrict__ par, int B, int H, int W, int H0,
    int W0, int top, int left) {
  const long t = (long)blockIdx.x * BLOCK + threadIdx.x;
  const long p = t >> 2;
  const int q = (int)(t & 3);                          // 0 = weight, 1..3 = R, G, B
  if (p >= (long)H0 * W0) return;
  if (slot) {   // the flows where the plan's upsampling kernels wrote them (address supplied at run time)
    const float* base = (const float*)(*slot);
    flow0 = base + off0;
    flow1 = base + off1;
  }
  const int m = (int)blockIdx.y;
  const int dir = m >= B, b = m - dir * B;             // block-uniform
  const int tq = par[0];
  const float s = (float)(dir ? 256 - tq : tq) / 256.f;   // exact
  const int y = (int)(p / W0), x = (int)(p - (long)y * W0);
  const long mp = ((long)b * H + top + y) * W + left + x;   // the pixel in the map
  const float2 f = *(const float2*)((dir ? flow1 : flow0) + 2 * mp);
  const float px = (float)x + s * f.x, py = (float)y + s * f.y;
  // float comparisons before any conversion: NaN, +-inf and far landings contribute nothing
  if (!(px > -1.f && px < (float)W0 && py > -1.f && py < (float)H0)) return;
  const u64 k = (occ && occ[(long)dir * B * H * W + mp]) ? 1ull : CONSISTENT;
  const unsigned char* c = (dir ? frame1 : frame0) + 3 * ((long)b * H0 * W0 + p);
  const u64 kv = k * (q ? (u64)c[q - 1] : 1ull);       // what this lane multiplies a tap's weight by: < 2^12
  const float x0f = floorf(px), y0f = floorf(py);
  const int qx = (int)rintf((px - x0f) * 16.f), qy = (int)rintf((py - y0f) * 16.f);   // ties to even, [0, 16]
  const int x0 = (int)x0f, y0 = (int)y0f;              // in [-1, W0-1] x [-1, H0-1]
  const int wx[2] = {16 - qx, qx}, wy[2] = {16 - qy, qy};
  u64* a = acc + 4 * ((long)m * H0 * W0) + q;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int tx = x0 + dx, ty = y0 + dy, w = wx[dx] * wy[dy];
      // no address is formed for a tap outside the frame
      if (w != 0 && (unsigned)tx < (unsigned)W0 && (unsigned)ty < (unsigned)H0)
        atomicAdd(a + 4 * ((long)ty * W0 + tx), (u64)w * kv);
    }
  }
}

// floor(num / den) for 0 < den, num <= 256 * den, num < 2^62: a float estimate (relative error below
// 2^-22, so off by at most one) and one exact integer correction -- the bits of the 64-bit division
__device__ __forceinline__ unsigned div_small(u64 num, u64 den) {
  unsigned q = (unsigned)((float)num / (float)den);
  const long long rem = (long long)(num - (u64)q * den);
  if (rem < 0) q -= 1;
  else if ((u64)rem >= den) q += 1;
  return q;
}

// grid (ceil(H0 * W0 / 256), B)
__global__ __launch_bounds__(BLOCK) void interp_resolve_kernel(const unsigned char* __restrict__ frame0,
                                                               const unsigned char* __restrict__ frame1,
                                                               const u64* __restrict__ acc, const int* __restrict__ par,
                                                               unsigned char* __restrict__ out,
                                                               unsigned char* __restrict__ holes, int B, long P) {
  const long p = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (p >= P) return;
  const int b = (int)blockIdx.y;
  const int tq = par[0];
  const u64 dmin = (u64)par[1], a0 = (u64)(256 - tq), a1 = (u64)tq;
  const long cell = (long)b * P + p;
  const ulonglong2* c0 = (const ulonglong2*)(acc + 4 * cell);
  const ulonglong2* c1 = (const ulonglong2*)(acc + 4 * ((long)B * P + cell));
  const ulonglong2 u0 = c0[0], u1 = c0[1], v0 = c1[0], v1 = c1[1];
  const u64 D = a0 * u0.x + a1 * v0.x;
  const bool hole = D < dmin;                          // dmin >= 1: D > 0 where the quotient is taken
  unsigned char* o = out + 3 * cell;
  if (hole) {
    const unsigned char* fb = (tq <= 128 ? frame0 : frame1) + 3 * cell;
    o[0] = fb[0]; o[1] = fb[1]; o[2] = fb[2];
  } else {
    const u64 n[3] = {a0 * u0.y + a1 * v0.y, a0 * u1.x + a1 * v1.x, a0 * u1.y + a1 * v1.y};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) o[ch] = (unsigned char)div_small(2 * n[ch] + D, 2 * D);   // N <= 255 D: in [0, 255]
  }
  holes[cell] = hole ? 1 : 0;
}

inline bool sizes_ok(int B, int H0, int W0, int maps) {
  return B >= 1 && H0 >= 1 && W0 >= 1 && (long)H0 * W0 <= JR_INTERP_MAX_PIXELS && maps >= 1 && maps <= 65535;
}

}  // namespace

extern "C" int jr_interp_splat(const void* frame0, const void* frame1, const float* flow0, const float* flow1,
                               const void* slot, long off0, long off1, const void* occ, long long* acc, const int* par,
                               int B, int H, int W, int H0, int W0, int top, int left, hipStream_t stream) {
  if (!sizes_ok(B, H0, W0, 2 * B) || H < 1 || W < 1 || top < 0 || left < 0 || top + H0 > H || left + W0 > W ||
      (long)H * W > 0x3fffffffL || !frame0 || !frame1 || !acc || !par || (!slot && (!flow0 || !flow1)))
    return (int)hipErrorInvalidValue;
  const unsigned gx = (unsigned)((4 * (long)H0 * W0 + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL(interp_splat_kernel, dim3(gx, (unsigned)(2 * B)), dim3(BLOCK), 0, stream,
                     (const unsigned char*)frame0, (const unsigned char*)frame1, flow0, flow1, (const long long*)slot, off0,
                     off1, (const unsigned char*)occ, (u64*)acc, par, B, H, W, H0, W0, top, left);
  return (int)hipGetLastError();
}

extern "C" int jr_interp_resolve(const void* frame0, const void* frame1, const long long* acc, const int* par, void* out,
                                 void* holes, int B, int H0, int W0, hipStream_t stream) {
  if (!sizes_ok(B, H0, W0, B) || !frame0 || !frame1 || !acc || !par || !out || !holes) return (int)hipErrorInvalidValue;
  const long P = (long)H0 * W0;
  const unsigned gx = (unsigned)((P + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL(interp_resolve_kernel, dim3(gx, (unsigned)B), dim3(BLOCK), 0, stream, (const unsigned char*)frame0,
                     (const unsigned char*)frame1, (const u64*)acc, par, (unsigned char*)out, (unsigned char*)holes, B, P);
  return (int)hipGetLastError();
}
