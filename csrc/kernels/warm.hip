// Warm start of the refinement loop (video): seeding a plan's flow state from
// an initial 1/8-resolution flow, and projecting the flow of pair t forward in
// time into the initial flow of pair t + 1 (original RAFT's `flow_init` +
// `forward_interpolate`, there a host-side scipy.griddata per frame).  The
// semantics are the golden ops' (models/reference.py:forward_project,
// models/raft.py:forward_reference with flow_init); both kernels match them bit
// for bit.  Latency kernels: 7 k - 33 k threads, one thread per cell, no MFMA.
#include "common.h"
#include "kernels.h"

namespace {

constexpr unsigned long long KEY_EMPTY = ~0ull;
constexpr int MAX_FILL_RADIUS = 8;
constexpr int N_OFFSETS = (2 * MAX_FILL_RADIUS + 1) * (2 * MAX_FILL_RADIUS + 1);

// The hole search's neighbour offsets, ascending by (dy*dy + dx*dx, dy, dx), for the largest
// radius; a smaller radius walks the same table and skips the offsets outside its box (a
// subsequence of a sorted sequence is sorted).
struct Offsets {
  signed char dy[N_OFFSETS], dx[N_OFFSETS];
};
constexpr Offsets make_offsets() {
  Offsets t{};
  int n = 0;
  for (int d2 = 0; d2 <= 2 * MAX_FILL_RADIUS * MAX_FILL_RADIUS; ++d2)
    for (int dy = -MAX_FILL_RADIUS; dy <= MAX_FILL_RADIUS; ++dy)
      for (int dx = -MAX_FILL_RADIUS; dx <= MAX_FILL_RADIUS; ++dx)
        if (dy * dy + dx * dx == d2) {
          t.dy[n] = (signed char)dy;
          t.dx[n] = (signed char)dx;
          ++n;
        }
  return t;
}
__constant__ Offsets kOffsets = make_offsets();

// ---------------------------------------------------------------------------
// Key buffer: [2][B*h*w] 64-bit keys + 2 control words, allocated all ones.
//
// Pass 2 reads the keys of a cell's neighbours (hole filling), so it cannot
// put a cell's key back to "empty" in place: a neighbouring thread could read
// the cell after the reset and see a hit cell as a hole.  The reset is
// therefore done where no thread of the same launch reads: the buffer holds
// two key planes, a call splats into and resolves from plane p and pass 2
// resets the cell of plane 1 - p, which the PREVIOUS call used and nothing
// reads now.  Every plane is thus all ones on entry to the call that splats
// into it, with no memset launch.
//
// p lives on the device (a replayed or repeated launch sequence alternates by
// itself): ctl[0] is written only by pass 2 and read only by pass 1, ctl[1] is
// written only by pass 1 and read only by pass 2, so no launch reads a word
// that one of its own threads writes.  Pass 1 takes p = ctl[0] & 1 and hands it
// on in ctl[1]; pass 2 takes p = ctl[1] & 1 and leaves ctl[0] = 1 - p for the
// next call.  (All ones on allocation: the first call uses plane 1.)
// ---------------------------------------------------------------------------

// Pass 1, one thread per source cell: the cell's landing point, its target cell and the
// 64-bit key (squared landing distance in 1/256 cells << 32 | source index), atomic-min'ed
// into the target's key.  An integer min is commutative and associative, so the winner
// does not depend on the order the threads run in: eager and replayed runs, and any two
// runs, are bitwise identical.  The distance is integer arithmetic on two rounded fp32
// values (no float multiply-add that contraction could change).
__global__ __launch_bounds__(256) void project_splat_kernel(const float* __restrict__ flow,
                                                            unsigned long long* __restrict__ keys,
                                                            unsigned long long* __restrict__ ctl, int B, int h, int w) {
  const int hw = h * w;
  const long M = (long)B * hw;
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  const int p = (int)(ctl[0] & 1ull);
  if (m == 0) ctl[1] = (unsigned long long)p;
  if (m >= M) return;
  const int rem = (int)(m % hw);
  const int y = rem / w, x = rem - y * w;
  const float2 f = *(const float2*)(flow + 2 * m);
  const float x1 = (float)x + f.x, y1 = (float)y + f.y;
  const float tx = floorf(x1 + 0.5f), ty = floorf(y1 + 0.5f);
  // float comparisons: NaN and +-inf landing points are invalid
  if (!(tx >= 0.f && tx <= (float)(w - 1) && ty >= 0.f && ty <= (float)(h - 1))) return;
  const int ix = (int)rintf((x1 - tx) * 256.f), iy = (int)rintf((y1 - ty) * 256.f);
  const unsigned d2 = (unsigned)(ix * ix + iy * iy);
  const unsigned long long key = ((unsigned long long)d2 << 32) | (unsigned)rem;
  const int tgt = (int)ty * w + (int)tx;
  atomicMin(keys + (long)p * M + (m - rem) + tgt, key);
}

// Pass 2, one thread per target cell: a hit cell takes its winning source's flow; a hole the
// value of the first hit cell in sorted-offset order within the radius (read from the keys, so
// holes are filled from splat-hit cells only), else zero.  Then the reset of the other plane.
__global__ __launch_bounds__(256) void project_resolve_kernel(const float* __restrict__ flow,
                                                              unsigned long long* __restrict__ keys,
                                                              unsigned long long* __restrict__ ctl,
                                                              float* __restrict__ out, int B, int h, int w, int R) {
  const int hw = h * w;
  const long M = (long)B * hw;
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  const int p = (int)(ctl[1] & 1ull);
  if (m == 0) ctl[0] = (unsigned long long)(1 - p);
  if (m >= M) return;
  const int rem = (int)(m % hw);
  const int y = rem / w, x = rem - y * w;
  const long img0 = m - rem;
  const unsigned long long* kp = keys + (long)p * M + img0;
  float2 v = make_float2(0.f, 0.f);
  const int d2max = 2 * R * R;
  for (int k = 0; k < N_OFFSETS; ++k) {
    const int dy = kOffsets.dy[k], dx = kOffsets.dx[k];
    if (dy * dy + dx * dx > d2max) break;
    if (abs(dy) > R || abs(dx) > R) continue;
    const int yy = y + dy, xx = x + dx;
    if ((unsigned)yy >= (unsigned)h || (unsigned)xx >= (unsigned)w) continue;
    const unsigned long long key = kp[yy * w + xx];
    if (key != KEY_EMPTY) {
      const unsigned src = (unsigned)(key & 0xffffffffull);
      if (src < (unsigned)hw) v = *(const float2*)(flow + 2 * (img0 + src));   // (a foreign buffer's bits: no wild read)
      break;
    }
  }
  *(float2*)(out + 2 * m) = v;
  keys[(long)(1 - p) * M + m] = KEY_EMPTY;
}

// The seed of a warm plan (replaces init_coords): what flow_taps_kernel (flowhead.hip)
// leaves behind after an update whose result is flow_init.
template <typename T>
__global__ __launch_bounds__(256) void init_flow_kernel(const float* __restrict__ fi, long M, int h, int w,
                                                        float* __restrict__ coords, float* __restrict__ flow32,
                                                        T* __restrict__ hx, int hx_cs, int hx_off, T* __restrict__ qx,
                                                        int qx_cs, int qx_off, T* __restrict__ fz, int fz_cs) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int rem = (int)(m % ((long)h * w));
  const int y = rem / w, x = rem - y * w;
  const float2 f = *(const float2*)(fi + 2 * m);
  *(float2*)(coords + 2 * m) = make_float2((float)x + f.x, (float)y + f.y);
  *(float2*)(flow32 + 2 * m) = f;
  const T vx = (T)f.x, vy = (T)f.y;
  hx[m * hx_cs + hx_off] = vx;
  hx[m * hx_cs + hx_off + 1] = vy;
  if (qx) {
    qx[m * qx_cs + qx_off] = vx;
    qx[m * qx_cs + qx_off + 1] = vy;
  }
  if (fz) {
    fz[m * fz_cs] = vx;
    fz[m * fz_cs + 1] = vy;
    // fp32 engine: flow4 rows are (fx, fy, 0, 0), as jr_flow_update_f32 writes them
    if (sizeof(T) == 4)
      for (int c = 2; c < fz_cs; ++c) fz[m * fz_cs + c] = (T)0.f;
  }
}

}  // namespace

extern "C" int jr_forward_project(const float* flow, void* keys, float* out, int B, int h, int w, int fill_radius,
                                  hipStream_t stream) {
  if (B < 1 || h < 1 || w < 1 || (long)h * w > 0x7fffffffL || fill_radius < 0 || fill_radius > MAX_FILL_RADIUS)
    return (int)hipErrorInvalidValue;
  const long M = (long)B * h * w;
  unsigned long long* kp = (unsigned long long*)keys;
  unsigned long long* ctl = kp + 2 * M;
  const dim3 grid((unsigned)((M + 255) / 256));
  hipLaunchKernelGGL(project_splat_kernel, grid, dim3(256), 0, stream, flow, kp, ctl, B, h, w);
  hipLaunchKernelGGL(project_resolve_kernel, grid, dim3(256), 0, stream, flow, kp, ctl, out, B, h, w, fill_radius);
  return (int)hipGetLastError();
}

extern "C" int jr_init_flow(const float* flow_init, int N, int h, int w, float* coords, float* flow32, void* hx,
                            int hx_cs, int hx_off, void* qx, int qx_cs, int qx_off, void* f8, int f8_cs,
                            hipStream_t stream) {
  const long M = (long)N * h * w;
  hipLaunchKernelGGL(init_flow_kernel<bf16>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, flow_init, M, h,
                     w, coords, flow32, (bf16*)hx, hx_cs, hx_off, (bf16*)qx, qx_cs, qx_off, (bf16*)f8, f8_cs);
  return (int)hipGetLastError();
}

extern "C" int jr_init_flow_f32(const float* flow_init, int N, int h, int w, float* coords, float* flow32, float* hx,
                                int hx_cs, int hx_off, float* qx, int qx_cs, int qx_off, float* flow4,
                                hipStream_t stream) {
  const long M = (long)N * h * w;
  hipLaunchKernelGGL(init_flow_kernel<float>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, flow_init, M, h,
                     w, coords, flow32, hx, hx_cs, hx_off, qx, qx_cs, qx_off, flow4, 4);
  return (int)hipGetLastError();
}
