// Range-map occlusion estimate of a bidirectional flow pair (Wang et al. 2018; UFlow / SMURF use it
// early in training): how much of the other frame maps onto each pixel, and the visibility masks
// derived from it, both directions in one launch each.  The semantics are the golden ops'
// (train/occlusion.py:range_map, visibility_masks) and the kernels equal them bit for bit: the
// landing point is one fp32 add per axis, its fraction is quantised to 1/16 per axis, and the
// splat adds INTEGER weights (four taps, 256 per source), so the sums do not depend on the order
// of the atomics.  No float atomics, no LDS, no host synchronisation.
//   range_splat:   one thread per source pixel: one 8-byte load of its flow, up to four 32-bit
//                  integer atomic adds (a tap of weight 0 is not issued).  The caller clears acc.
//   range_visible: one thread per 4 pixels of a row: its own flow for the inside test, the
//                  opposite direction's acc, one fp32 mask per pixel (16-byte accesses when the
//                  width and the addresses allow, element accesses with a row tail otherwise).
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

// grid: (ceil(H * W / 256), maps), map m = d * B + b reads flow d, adds into acc[m]
__global__ __launch_bounds__(256) void range_splat_kernel(const float* __restrict__ fw, const float* __restrict__ bw,
                                                          int* __restrict__ acc, int B, int H, int W) {
  const int HW = H * W;                                  // <= 2^23 (checked by the host)
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (p >= HW) return;
  const int m = (int)blockIdx.y;
  const int dir = m >= B;
  const float* f = (dir ? bw : fw) + 2 * ((long)(m - dir * B) * HW);
  int* a = acc + (long)m * HW;
  const int y = p / W, x = p - y * W;
  const float2 v = *(const float2*)(f + 2 * (long)p);
  const float px = (float)x + v.x, py = (float)y + v.y;
  // float comparisons before any conversion: NaN, +-inf and far landings contribute nothing
  if (!(px > -1.f && px < (float)W && py > -1.f && py < (float)H)) return;
  const float x0f = floorf(px), y0f = floorf(py);
  const int qx = (int)rintf((px - x0f) * 16.f), qy = (int)rintf((py - y0f) * 16.f);   // ties to even, [0, 16]
  const int x0 = (int)x0f, y0 = (int)y0f;                // in [-1, W-1] x [-1, H-1]
  const int wx[2] = {16 - qx, qx}, wy[2] = {16 - qy, qy};
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int tx = x0 + dx, ty = y0 + dy, w = wx[dx] * wy[dy];
      // no address is formed for a tap outside the map
      if (w != 0 && (unsigned)tx < (unsigned)W && (unsigned)ty < (unsigned)H) atomicAdd(a + ty * W + tx, w);
    }
  }
}

__device__ __forceinline__ float visible(float2 f, int a, int x, int y, int H, int W, int T) {
  const float px = (float)x + f.x, py = (float)y + f.y;
  const bool inside = px >= 0.f && px <= (float)(W - 1) && py >= 0.f && py <= (float)(H - 1);   // NaN: not inside
  return (!inside || a >= T) ? 1.f : 0.f;
}

// grid: (ceil(H * ceil(W / 4) / 256), 2 B), map m = d * B + b reads flow d and acc[1 - d], writes vis[m]
__global__ __launch_bounds__(256) void range_visible_kernel(const float* __restrict__ fw, const float* __restrict__ bw,
                                                            const int* __restrict__ acc, float* __restrict__ vis, int B,
                                                            int H, int W, int T, int vec) {
  const int W4 = (W + 3) >> 2, HW = H * W;
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= H * W4) return;
  const int y = t / W4, x4 = (t - y * W4) * 4;
  const int m = (int)blockIdx.y;
  const int dir = m >= B, b = m - dir * B;
  const float* f = (dir ? bw : fw) + 2 * ((long)b * HW + (long)y * W + x4);
  const int* a = acc + ((long)((1 - dir) * B + b) * HW + (long)y * W + x4);
  float* o = vis + ((long)m * HW + (long)y * W + x4);
  if (vec) {                                             // W % 4 == 0, every base 16-byte aligned
    const float4 v0 = *(const float4*)f, v1 = *(const float4*)(f + 4);
    const int4 c = *(const int4*)a;
    *(float4*)o = make_float4(visible(make_float2(v0.x, v0.y), c.x, x4, y, H, W, T),
                              visible(make_float2(v0.z, v0.w), c.y, x4 + 1, y, H, W, T),
                              visible(make_float2(v1.x, v1.y), c.z, x4 + 2, y, H, W, T),
                              visible(make_float2(v1.z, v1.w), c.w, x4 + 3, y, H, W, T));
    return;
  }
  const int n = min(4, W - x4);                          // the row's tail
  for (int k = 0; k < n; ++k) o[k] = visible(*(const float2*)(f + 2 * k), a[k], x4 + k, y, H, W, T);
}

inline bool sizes_ok(int B, int H, int W, int maps) {
  return B >= 1 && H >= 1 && W >= 1 && (long)H * W <= JR_RANGE_MAX_PIXELS && maps >= 1 && maps <= 65535;
}

}  // namespace

extern "C" int jr_range_splat(const float* flow_fw, const float* flow_bw, int* acc, int B, int H, int W,
                              hipStream_t stream) {
  const int maps = flow_bw ? 2 * B : B;
  if (!sizes_ok(B, H, W, maps) || !flow_fw || !acc) return (int)hipErrorInvalidValue;
  const unsigned gx = (unsigned)(((long)H * W + 255) / 256);
  hipLaunchKernelGGL(range_splat_kernel, dim3(gx, (unsigned)maps), dim3(256), 0, stream, flow_fw, flow_bw, acc, B, H, W);
  return (int)hipGetLastError();
}

extern "C" int jr_range_visible(const float* flow_fw, const float* flow_bw, const int* acc, float* vis, int B, int H,
                                int W, int T, hipStream_t stream) {
  if (!sizes_ok(B, H, W, 2 * B) || !flow_fw || !flow_bw || !acc || !vis) return (int)hipErrorInvalidValue;
  const uintptr_t bits = (uintptr_t)flow_fw | (uintptr_t)flow_bw | (uintptr_t)acc | (uintptr_t)vis;
  const int vec = W % 4 == 0 && bits % 16 == 0;
  const unsigned gx = (unsigned)(((long)H * ((W + 3) / 4) + 255) / 256);
  hipLaunchKernelGGL(range_visible_kernel, dim3(gx, (unsigned)(2 * B)), dim3(256), 0, stream, flow_fw, flow_bw, acc, vis, B,
                     H, W, T, vec);
  return (int)hipGetLastError();
}
