// Forward-backward consistency check of a bidirectional flow pair (UnFlow, Meister et al. 2018):
// the occlusion masks of flow 1->2 and flow 2->1 in ONE launch, at the end of a bidirectional
// plan's epilogue.  The semantics are the golden op's (models/reference.py:fb_consistency) and the
// kernel equals it bit for bit: the same fp32 operations in the same order, every product and
// sum rounded on its own (contraction is off for this file, below).
// A bandwidth kernel: one thread per 4 consecutive pixels of a row -- two 16-byte loads of its
// own flow, four cached gathers per pixel from the opposite flow, one 32-bit store of 4 mask
// bytes (+ one 16-byte store of 4 errors).  No atomics, no LDS.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

// One pixel (y, x) of the H0 x W0 frame: f its own flow, b the opposite flow's frame origin
// (row stride W pixels).  Returns the mask byte, *err the error (inf where the landing point
// is outside the frame).
__device__ __forceinline__ unsigned fb_pixel(float2 f, const float* __restrict__ b, int W, int y, int x, int H0,
                                             int W0, float alpha, float beta, float* err) {
  const float px = (float)x + f.x, py = (float)y + f.y;
  // float comparisons: a NaN landing point is outside
  if (!(px >= 0.f && px <= (float)(W0 - 1) && py >= 0.f && py <= (float)(H0 - 1))) {
    *err = __builtin_inff();
    return 1u;
  }
  const float x0f = floorf(px), y0f = floorf(py);
  const float wx = px - x0f, wy = py - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;             // in [0, W0-1] x [0, H0-1]: inside
  const int x1 = min(x0 + 1, W0 - 1), y1 = min(y0 + 1, H0 - 1);
  const float2 b00 = *(const float2*)(b + 2 * ((long)y0 * W + x0));
  const float2 b01 = *(const float2*)(b + 2 * ((long)y0 * W + x1));
  const float2 b10 = *(const float2*)(b + 2 * ((long)y1 * W + x0));
  const float2 b11 = *(const float2*)(b + 2 * ((long)y1 * W + x1));
  const float tx = b00.x + wx * (b01.x - b00.x), ty = b00.y + wx * (b01.y - b00.y);
  const float bx = b10.x + wx * (b11.x - b10.x), by = b10.y + wx * (b11.y - b10.y);
  const float gx = tx + wy * (bx - tx), gy = ty + wy * (by - ty);
  const float dx = f.x + gx, dy = f.y + gy;
  const float e = dx * dx + dy * dy;
  const float mag = (f.x * f.x + f.y * f.y) + (gx * gx + gy * gy);
  const float thr = alpha * mag + beta;
  *err = e;
  return (e <= thr) ? 0u : 1u;                        // a NaN error is occluded
}

// grid: 2 * B * H * (W / 4) threads, direction-major like occ / err [2][B][H][W]
__global__ __launch_bounds__(256) void fb_check_kernel(const float* __restrict__ fw, const float* __restrict__ bw,
                                                       const long long* __restrict__ slot, long off_fw, long off_bw,
                                                       const float* __restrict__ thr, unsigned* __restrict__ occ,
                                                       float* __restrict__ err, int B, int H, int W, int H0, int W0,
                                                       int top, int left) {
  const int W4 = W >> 2;
  const long n = (long)B * H * W4;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * n) return;
  if (slot) {   // the flows where the plan's upsampling kernels wrote them (address supplied at run time)
    const float* base = (const float*)(*slot);
    fw = base + off_fw;
    bw = base + off_bw;
  }
  const int dir = t >= n;
  const long r = dir ? t - n : t;
  const int x4 = (int)(r % W4) * 4;
  const long row = r / W4;              // b * H + Y
  const int Y = (int)(row % H);
  const long img = (row - Y) * W;       // pixel index of the image's origin
  const float* a = dir ? bw : fw;
  const float* b = dir ? fw : bw;
  const float alpha = thr[0], beta = thr[1];
  const float4 v0 = *(const float4*)(a + 2 * (row * W + x4));
  const float4 v1 = *(const float4*)(a + 2 * (row * W + x4) + 4);
  const float2 f[4] = {make_float2(v0.x, v0.y), make_float2(v0.z, v0.w), make_float2(v1.x, v1.y),
                       make_float2(v1.z, v1.w)};
  const float* bo = b + 2 * (img + (long)top * W + left);   // the frame's origin in the opposite flow
  const int y = Y - top;
  unsigned m = 0;
  float e[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = x4 + k - left;
    e[k] = 0.f;
    if ((unsigned)y < (unsigned)H0 && (unsigned)x < (unsigned)W0)   // outside the frame window: not occluded
      m |= fb_pixel(f[k], bo, W, y, x, H0, W0, alpha, beta, &e[k]) << (8 * k);
  }
  occ[t] = m;
  if (err) *(float4*)(err + 4 * t) = make_float4(e[0], e[1], e[2], e[3]);
}

}  // namespace

extern "C" int jr_fb_check(const float* flow_fw, const float* flow_bw, const void* slot, long off_fw, long off_bw,
                           const float* thr, void* occ, float* err, int B, int H, int W, int H0, int W0, int top,
                           int left, hipStream_t stream) {
  if (B < 1 || H < 1 || W < 4 || W % 4 || H0 < 1 || W0 < 1 || top < 0 || left < 0 || top + H0 > H || left + W0 > W ||
      (long)H * W > 0x3fffffffL || (!slot && (!flow_fw || !flow_bw)))
    return (int)hipErrorInvalidValue;
  const long n = 2L * B * H * (W / 4);
  if ((n + 255) / 256 > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(fb_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, flow_fw, flow_bw,
                     (const long long*)slot, off_fw, off_bw, thr, (unsigned*)occ, err, B, H, W, H0, W0, top, left);
  return (int)hipGetLastError();
}
