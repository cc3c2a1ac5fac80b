// The query coordinates of a lookup wave and the flow update fused ahead of the lookup
// (TapsUpd, kernels.h): shared by the pyramid lookup (corr.hip) and the on-demand lookup
// (corr_od.hip), so both apply the update with the same operations in the same order.
#pragma once
#include "common.h"
#include "kernels.h"

// Query coordinates of a lookup wave (QPW queries q0 ..), with the optional
// fused flow update (TapsUpd): lane 18 k + 2 t + c loads tap t, component c of
// query k's 3x3 neighbour (zero outside the image); lanes 18 k + c sum bias[c]
// and the nine taps in jr_flow_taps' order, store the new coords / flow, and
// every lane receives the new coords by shuffle.  All lanes take part.
template <int QPW>
JR_DEVICE void lookup_coords(const TapsUpd& u, const float* coords, int q0, int total, int h, int w, int lane,
                             float (&cx)[QPW], float (&cy)[QPW]) {
  static_assert(QPW * 18 <= 64, "QPW");
  if (!u.on) {
#pragma unroll
    for (int k = 0; k < QPW; ++k) {
      const int q = q0 + k;
      cx[k] = q < total ? coords[2 * (long)q] : 0.f;
      cy[k] = q < total ? coords[2 * (long)q + 1] : 0.f;
    }
    return;
  }
  const int uq = lane / 18, k = lane - uq * 18;
  const int tap = k >> 1, c = k & 1;
  const long q = (long)q0 + uq;
  const bool own = uq < QPW && q < total;
  const int hw = h * w;
  int y = 0, x = 0;
  float val = 0.f;
  if (own) {
    const int rem = (int)(q % hw);
    y = rem / w;
    x = rem - y * w;
    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    if ((unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w)
      val = u.taps[(q - rem + (long)yy * w + xx) * u.tcs + k];
  }
  float d = u.bias[c];
#pragma unroll
  for (int t = 0; t < 9; ++t) d += __shfl(val, min(uq * 18 + 2 * t + c, 63));
  float cn = 0.f;
  if (own && k < 2) {
    cn = coords[2 * q + k] + d;
    u.coords[2 * q + k] = cn;
    const float f = cn - (float)(k == 0 ? x : y);
    u.flow32[2 * q + k] = f;
    const bf16 fb = f2bf(f);
    ((bf16*)u.hx)[q * u.hx_cs + u.hx_off + k] = fb;
    if (u.qx) ((bf16*)u.qx)[q * u.qx_cs + u.qx_off + k] = fb;
    if (u.f8) ((bf16*)u.f8)[q * u.f8_cs + k] = fb;
  }
#pragma unroll
  for (int kk = 0; kk < QPW; ++kk) {
    cx[kk] = __shfl(cn, kk * 18);
    cy[kk] = __shfl(cn, kk * 18 + 1);
  }
}
