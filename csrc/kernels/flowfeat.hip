// The motion encoder's flow branch in one launch: convflow1 (7x7, 2 -> 128, relu) and convflow2
// (3x3 / pad 1, 128 -> 64, relu), jax_raft/model.py:282-285, run every refinement iteration on the
// lane schedule's mask lane (runtime/lowering.py:schedule_lanes).
//
// As two launches (conv_direct.hip, then conv_halo.hip in the config <128, 2, 2, 2, 8, 16>) the
// 128-channel intermediate f1 goes to memory and comes back with halos, and the first launch is
// mostly latency (8 us at 2 % MFMA busy, profiles/r6_pmc_b4.txt).  Here the halo conv's workgroup
// (8 x 16 output pixels, 4 waves) does not load its (8 + 2) x (16 + 2) footprint of f1: it computes
// those 180 pixels' 128 channels from the 2-channel flow with the 7x7 conv's MFMA body
// (conv_direct.h: K = 7 x 8 x 2 in 4 k-chunks of 16x16x32, kc = 0..3), applies bias + relu, rounds
// to bf16 as f1 is stored, and writes the result into the footprint image (halo.h: key_x layout).
// Footprint pixels outside the image are ZERO -- the 3x3 conv's padding -- not convflow1 evaluated
// there.  The flow patch the 7x7 windows read, (10 + 6) x (18 + 7) pixels, is staged in LDS once
// (zero outside the image: the 7x7 conv's padding), so a B fragment is four 4-B LDS reads.  The
// halo main loop (halo.h:pipe_gemm; tap-major, k16 steps, one accumulator chain) and the bias /
// relu / bf16 store of conv_halo.hip's epilogue follow unchanged, so every output is bitwise what
// the two launches write.  Recompute: 180 / 128 of a conv whose MFMA work is under 1 us.
#include "halo.h"

namespace {

constexpr int C1 = 128, COUT = 64;                       // convflow1 / convflow2 output channels
constexpr int WCO = 2, WPX = 2, TN = 2, TR = 8, TC = 16; // the halo tile config
constexpr int NT = 64 * WCO * WPX;
constexpr int P = pitch_of<C1>();
constexpr int SPT = C1 / 16, S = 9 * SPT, PD = 16;       // k-steps per tap, in all; weight ring depth
constexpr int FW = TC + 2, FH = TR + 2, NFP = FH * FW;   // footprint
constexpr int RB = P * 16;                               // footprint row bytes
constexpr int KH = 7, KWP = 8, NKC = 4, PAD7 = 3;        // 7x7 conv: kw padded to 8, K = 7 * 8 * 2 -> 4 k-chunks
// flow patch: rows fy + kh (kh up to 7: the k-chunks' padding row, zero weights), columns fx + kw
constexpr int PR = FH + KH, PC = FW + KWP - 1;
constexpr int PATCH_OFF = NFP * RB;
constexpr int LDS_BYTES = PATCH_OFF + (PR * PC * 4 + 15) / 16 * 16;
constexpr int NPT = (NFP + 15) / 16;                     // 16-pixel tiles of the footprint
static_assert(NT % 64 == 0 && NT / 64 * 32 == C1, "one 32-channel block of convflow1 per wave");
static_assert(TR * TC == 32 * WPX * TN && COUT == 32 * WCO, "tile");

__global__ __launch_bounds__(NT, 1) void flow_features_kernel(const FlowFeatParams p) {
  extern __shared__ __attribute__((aligned(16))) bf16 lds[];
  char* const lds_b = (char*)lds;
  unsigned* const patch = (unsigned*)(lds_b + PATCH_OFF);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rho = lane & 31, hh = lane >> 5;
  const int wc = wave % WCO, wp = wave / WCO;

  const int per_img = p.tiles_y * p.tiles_x;
  const int n = blockIdx.x / per_img;
  const int rem = blockIdx.x - n * per_img;
  const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
  const int y0 = ty * TR, x0 = tx * TC;

  // convflow2's weight ring first (its latency overlaps the footprint's computation)
  const __amdgpu_buffer_rsrc_t ws = __builtin_amdgcn_make_buffer_rsrc((void*)p.w2, (short)0, (int)p.w2_bytes, 0x00020000);
  const unsigned w_base = (unsigned)(wc * S * 64 + lane) * 16u;
  bf16x8 ring[PD];
#pragma unroll
  for (int d = 0; d < PD; ++d) ring[d] = __builtin_bit_cast(bf16x8, bload(ws, w_base + (unsigned)d * 1024u));

  // flow patch -> LDS: pixel (y0 - 1 - 3 + pr, x0 - 1 - 3 + pc), both channels in 4 bytes
  {
    const unsigned* fl = (const unsigned*)p.flow + (long)n * p.H * p.W;
    for (int e = tid; e < PR * PC; e += NT) {
      const int pr = e / PC, pc = e - pr * PC;
      const int iy = y0 - 1 - PAD7 + pr, ix = x0 - 1 - PAD7 + pc;
      const bool in = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      patch[e] = in ? fl[iy * p.W + ix] : 0u;
    }
  }
  // convflow1: wave = channels 32 wave + [0, 32) (two 16-row A tiles) of every footprint pixel
  const int li = lane & 15, kg = lane >> 4;
  const int co0 = wave * 32;
  bf16x8 a[2][NKC];
  float bv1[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) a[t][kc] = ((const bf16x8*)p.w1)[((co0 / 16 + t) * NKC + kc) * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) bv1[t][r] = p.b1[co0 + 16 * t + 4 * kg + r];
  }
  __syncthreads();
#pragma unroll 4
  for (int pt = 0; pt < NPT; ++pt) {
    const int f = pt * 16 + li;
    const bool live = f < NFP;
    const int ff = live ? f : 0;
    const int fy = ff / FW, fx = ff - fy * FW;
    u32x4 u[NKC];
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      const int tt0 = kc * 16 + 4 * kg;   // first of this lane's 4 taps (conv_direct.h)
      const unsigned* q = patch + (fy + tt0 / KWP) * PC + fx + tt0 % KWP;
#pragma unroll
      for (int e = 0; e < 4; ++e) u[kc][e] = q[e];
    }
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      const bf16x8 b = __builtin_bit_cast(bf16x8, u[kc]);
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t][kc], b, acc[t], 0, 0, 0);
    }
    if (!live) continue;
    const bool in = (unsigned)(y0 - 1 + fy) < (unsigned)p.H && (unsigned)(x0 - 1 + fx) < (unsigned)p.W;
    const int kx = key_x<P>(fx + TC * fy);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = f2bf(in ? fmaxf(acc[t][r] + bv1[t][r], 0.f) : 0.f);
      // channels co0 + 16 t + 4 kg + [0, 4): half (kg & 1) of the 16-B chunk 4 wave + 2 t + (kg >> 1)
      *(bf16x4*)(lds_b + ff * RB + (((4 * wave + 2 * t + (kg >> 1)) ^ kx) << 4) + 8 * (kg & 1)) = o;
    }
  }

  // convflow2: conv_halo.hip's main loop and EPI_STD epilogue (bias, relu, bf16 store) for this config
  int rb0[TN], key0[TN], om[TN];
#pragma unroll
  for (int b = 0; b < TN; ++b) {
    const int q = 32 * (wp * TN + b) + lane_px(rho);
    const int i = q / TC, j = q - i * TC;
    const bool ok = i < TR && y0 + i < p.H && x0 + j < p.W;
    rb0[b] = ok ? (i * FW + j) * RB : 0;
    key0[b] = ok ? j + TC * i : 0;
    om[b] = ok ? (n * p.H + y0 + i) * p.W + x0 + j : -1;
  }
  __syncthreads();

  f32x16 acc[TN];
  pipe_gemm<TN, S, PD>(
      acc, ring,
      [&](int s) { return __builtin_bit_cast(bf16x8, bload(ws, w_base + (unsigned)s * 1024u)); },
      [&](int s, int b) {
        const int tap = s / SPT, kc = s - tap * SPT;
        const int u = tap / 3, v = tap % 3;
        const int kxh = (key_x<P>(key0[b] + v + TC * u) ^ hh) << 4;
        return *(const bf16x8*)(lds_b + (rb0[b] + (((2 * kc) << 4) ^ kxh)) + (u * FW + v) * RB);
      });
  const int c0 = 32 * wc + 16 * hh;
  float bv[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) bv[k] = p.b2[c0 + k];
#pragma unroll
  for (int b = 0; b < TN; ++b) {
    const int m = om[b];
    if (m < 0) continue;
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = fmaxf(acc[b][k] + bv[k], 0.f);
    store_bf16<16>((bf16*)p.y + (long)m * p.ycs + p.yoff + c0, v);
  }
}

}  // namespace

extern "C" int jr_flow_features_tile(int* out2) {
  out2[0] = TR; out2[1] = TC;
  return LDS_BYTES;
}

extern "C" int jr_flow_features_fused(const FlowFeatParams* p, hipStream_t stream) {
  if (p->ntiles <= 0 || p->ycs % 8 != 0 || p->yoff % 8 != 0 || p->yoff + COUT > p->ycs) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(flow_features_kernel, dim3(p->ntiles), dim3(NT), LDS_BYTES, stream, *p);
  return (int)hipGetLastError();
}
