// Motion-compensated frames and the masked photometric error of a bidirectional flow pair: the
// other frame sampled at x + flow(x), the pixels the forward-backward check calls occluded (or
// that land outside the frame) replaced by the frame's own, and the exact integer sum of
// |warped - own| over the kept pixels -- for one or both directions in ONE launch, at the end of
// a bidirectional plan's epilogue after fb_check.  The semantics are the golden op's
// (models/reference.py:warp_frames) and the kernel equals it bit for bit: the same fp32 operations
// in the same order, every product and sum rounded on its own (contraction is off for this file,
// below); steps 1 and 2 are fbcheck.hip's, so both agree on what "outside" means.
// A bandwidth kernel over the frame (not the padded map): grid (blocks, dirs * B), one thread per
// 4 consecutive pixels of a frame row (the last thread of a row takes the tail) -- 8-byte loads of
// its own flows (an odd `left` leaves no 16-byte alignment), its 4 mask bytes, four cached 3-byte
// gathers per pixel from the sampled frame, the 12 bytes of its own frame, and 12 output bytes as
// three 32-bit stores where every row starts 4-byte aligned ((W0 * 3) % 4 == 0), as bytes
// elsewhere.  No LDS for the gather.  The sums are integers (any order of addition gives the same
// bits): thread -> wave (shuffles) -> block (4 LDS words) -> one 64-bit atomic add per block and
// quantity.  The caller clears them (a plan: its memset op, recorded just before this one).
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int RUN = 4;        // pixels per thread
constexpr int BLOCK = 256;    // threads per block

// One pixel (y, x) of the H0 x W0 frame: f its flow, s the sampled frame of this sample.
// Returns false where the landing point is outside the frame (w is then not written).
__device__ __forceinline__ bool warp_pixel(float2 f, const unsigned char* __restrict__ s, int y, int x, int H0, int W0,
                                           unsigned* w) {
  const float px = (float)x + f.x, py = (float)y + f.y;
  // float comparisons: a NaN landing point is outside
  if (!(px >= 0.f && px <= (float)(W0 - 1) && py >= 0.f && py <= (float)(H0 - 1))) return false;
  const float x0f = floorf(px), y0f = floorf(py);
  const float wx = px - x0f, wy = py - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;             // in [0, W0-1] x [0, H0-1]: inside
  const int x1 = min(x0 + 1, W0 - 1), y1 = min(y0 + 1, H0 - 1);
  const unsigned char* p00 = s + 3 * ((long)y0 * W0 + x0);
  const unsigned char* p01 = s + 3 * ((long)y0 * W0 + x1);
  const unsigned char* p10 = s + 3 * ((long)y1 * W0 + x0);
  const unsigned char* p11 = s + 3 * ((long)y1 * W0 + x1);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float c00 = (float)p00[c], c01 = (float)p01[c], c10 = (float)p10[c], c11 = (float)p11[c];
    const float t = c00 + wx * (c01 - c00);
    const float b = c10 + wx * (c11 - c10);
    const float v = t + wy * (b - t);                 // in [0, 255]: every step is monotone
    w[c] = (unsigned)rintf(v);                        // ties to even
  }
  return true;
}

// grid (blocks over H0 * ceil(W0 / 4) threads, dirs * B); vec_out / vec_own: every full run of
// warped / own starts 4-byte aligned
__global__ __launch_bounds__(BLOCK) void warp_frames_kernel(
    const unsigned char* __restrict__ src0, const unsigned char* __restrict__ src1,
    const unsigned char* __restrict__ own0, const unsigned char* __restrict__ own1, const float* __restrict__ flow0,
    const float* __restrict__ flow1, const long long* __restrict__ slot, long off0, long off1,
    const unsigned char* __restrict__ occ, unsigned char* __restrict__ warped, unsigned long long* __restrict__ photo,
    int B, int H, int W, int H0, int W0, int top, int left, int vec_out, int vec_own) {
  __shared__ unsigned long long psum[BLOCK / 64], pcnt[BLOCK / 64];
  if (slot) {   // the flows where the plan's upsampling kernels wrote them (address supplied at run time)
    const float* base = (const float*)(*slot);
    flow0 = base + off0;
    flow1 = base + off1;
  }
  const int dir = (int)blockIdx.y / B;                // block-uniform
  const int b = (int)blockIdx.y - dir * B;
  const unsigned char* src = (dir ? src1 : src0) + 3 * (long)b * H0 * W0;
  const unsigned char* own = dir ? own1 : own0;
  const float* flow = dir ? flow1 : flow0;
  const int runs = (W0 + RUN - 1) / RUN;
  const long item = (long)blockIdx.x * BLOCK + threadIdx.x;
  int sum = 0, cnt = 0;                               // per thread: at most 4 * 3 * 255 and 4
  if (item < (long)H0 * runs) {
    const int y = (int)(item / runs);
    const int x = (int)(item % runs) * RUN;
    const int count = min(RUN, W0 - x);
    const long mp = ((long)b * H + top + y) * W + left + x;          // the run's first pixel in the map
    const long fp = 3 * (((long)b * H0 + y) * W0 + x);               // ... its first byte in a frame
    const float* f = flow + 2 * mp;
    float2 fl[RUN];
#pragma unroll
    for (int k = 0; k < RUN; ++k) fl[k] = k < count ? *(const float2*)(f + 2 * k) : make_float2(0.f, 0.f);
    unsigned m = 0;                                   // the run's mask bytes
    if (occ) {
      const unsigned char* o = occ + (long)dir * B * H * W + mp;
      if (count == RUN && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        m = *(const unsigned*)o;
      } else {
        for (int k = 0; k < count; ++k) m |= (unsigned)o[k] << (8 * k);
      }
    }
    unsigned char q[3 * RUN];                         // what fills a masked pixel: own, else 0
    if (own) {
      const unsigned char* op = own + fp;
      if (count == RUN && vec_own) {
        const unsigned* o4 = (const unsigned*)op;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const unsigned v = o4[j];
#pragma unroll
          for (int i = 0; i < 4; ++i) q[4 * j + i] = (unsigned char)(v >> (8 * i));
        }
      } else {
#pragma unroll
        for (int i = 0; i < 3 * RUN; ++i) q[i] = i < 3 * count ? op[i] : (unsigned char)0;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 3 * RUN; ++i) q[i] = 0;
    }
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
      if (k >= count) continue;
      unsigned w[3];
      if (((m >> (8 * k)) & 0xffu) != 0 || !warp_pixel(fl[k], src, y, x + k, H0, W0, w)) continue;
      cnt += 1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int d = (int)w[c] - (int)q[3 * k + c];
        sum += d < 0 ? -d : d;
        q[3 * k + c] = (unsigned char)w[c];
      }
    }
    unsigned char* out = warped + 3 * (long)dir * B * H0 * W0 + fp;
    if (count == RUN && vec_out) {
      unsigned* o4 = (unsigned*)out;
#pragma unroll
      for (int j = 0; j < 3; ++j)
        o4[j] = (unsigned)q[4 * j] | ((unsigned)q[4 * j + 1] << 8) | ((unsigned)q[4 * j + 2] << 16) |
                ((unsigned)q[4 * j + 3] << 24);
    } else {
#pragma unroll
      for (int i = 0; i < 3 * RUN; ++i)
        if (i < 3 * count) out[i] = q[i];
    }
  }
  if (!photo) return;                                 // kernel-uniform: no barrier is skipped by a part of a block
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, 64);
    cnt += __shfl_down(cnt, off, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { psum[wave] = (unsigned long long)sum; pcnt[wave] = (unsigned long long)cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* p = photo + 2 * (long)blockIdx.y;
    atomicAdd(p, (psum[0] + psum[1]) + (psum[2] + psum[3]));
    atomicAdd(p + 1, (pcnt[0] + pcnt[1]) + (pcnt[2] + pcnt[3]));
  }
}

}  // namespace

extern "C" int jr_warp_frames(const void* src0, const void* src1, const void* own0, const void* own1,
                              const float* flow0, const float* flow1, const void* slot, long off0, long off1,
                              const void* occ, void* warped, long long* photo, int B, int H, int W, int H0, int W0,
                              int top, int left, int dirs, hipStream_t stream) {
  if (B < 1 || H < 1 || W < 1 || H0 < 1 || W0 < 1 || top < 0 || left < 0 || top + H0 > H || left + W0 > W ||
      (long)H * W > 0x3fffffffL || dirs < 1 || dirs > 2 || (long)dirs * B > 65535 || !src0 || !warped ||
      (!slot && !flow0) || (dirs == 2 && (!src1 || (!slot && !flow1) || !own0 != !own1)) || (dirs == 1 && own1) ||
      (photo && !own0))
    return (int)hipErrorInvalidValue;
  const long items = (long)H0 * ((W0 + RUN - 1) / RUN);
  const long blocks = (items + BLOCK - 1) / BLOCK;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const bool rows4 = (W0 * 3L) % 4 == 0;              // every frame row starts on a multiple of 4 bytes
  const int vec_out = rows4 && (reinterpret_cast<uintptr_t>(warped) & 3) == 0;
  const int vec_own = rows4 && (reinterpret_cast<uintptr_t>(own0) & 3) == 0 && (reinterpret_cast<uintptr_t>(own1) & 3) == 0;
  hipLaunchKernelGGL(warp_frames_kernel, dim3((unsigned)blocks, (unsigned)(dirs * B)), dim3(BLOCK), 0, stream,
                     (const unsigned char*)src0, (const unsigned char*)src1, (const unsigned char*)own0,
                     (const unsigned char*)own1, flow0, flow1, (const long long*)slot, off0, off1,
                     (const unsigned char*)occ, (unsigned char*)warped, (unsigned long long*)photo, B, H, W, H0, W0, top,
                     left, vec_out, vec_own);
  return (int)hipGetLastError();
}
