// The per-pixel functions of the augmentation gather (augment.hip), the same for its three layouts:
// the record words, the texel transform, the bilinear blend, the source position of a resized
// coordinate, one output pixel of both images, the flow of one output pixel from dense ground truth
// (the four-tap blend) and from sparse ground truth (the scan for the winner), and the stores of a
// thread's run of 4 pixels.
// augment.hip switches contraction off; the pragma below covers the functions defined here.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace augment_dev {

// words 0..15 of a record's ints and 0..31 of its floats (train/augment.py), dense and sparse alike
constexpr int I_HR = 0, I_WR = 1, I_Y0 = 2, I_X0 = 3, I_HFLIP = 4, I_VFLIP = 5, I_NRECT = 6, I_RECT = 8;
constexpr int F_SX = 0, F_SY = 1, F_ISX = 2, F_ISY = 3, F_COL1 = 4, F_COL2 = 16;
// words 16..18 of the ints of a sparse or mixed record: the sample's own size; 1 for dense ground truth (mixed)
constexpr int I_HS = 16, I_WS = 17, I_DENSE = 18;

struct Colour {
  float b, k, s, m[9], mean[3], cm;   // cm: the contrast pivot min(255, b * luma(mean))
};

JR_DEVICE float clamp255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }
JR_DEVICE float luma(float r, float g, float b) { return (0.299f * r + 0.587f * g) + 0.114f * b; }

JR_DEVICE Colour load_colour(const float* __restrict__ f, const int* __restrict__ sum, int npix) {
  Colour c;
  c.b = f[0]; c.k = f[1]; c.s = f[2];
#pragma unroll
  for (int j = 0; j < 9; ++j) c.m[j] = f[3 + j];
#pragma unroll
  for (int j = 0; j < 3; ++j) c.mean[j] = (float)(((unsigned)sum[j] + (unsigned)(npix / 2)) / (unsigned)npix);
  c.cm = fminf(c.b * luma(c.mean[0], c.mean[1], c.mean[2]), 255.f);
  return c;
}

// brightness, contrast, saturation, hue of one texel, clamped to [0, 255] after every step
JR_DEVICE void texel(float& r, float& g, float& b, const Colour& c) {
  r = clamp255(r * c.b); g = clamp255(g * c.b); b = clamp255(b * c.b);
  if (c.k != 1.f) {
    r = clamp255((r - c.cm) * c.k + c.cm); g = clamp255((g - c.cm) * c.k + c.cm); b = clamp255((b - c.cm) * c.k + c.cm);
  }
  if (c.s != 1.f) {
    const float l = luma(r, g, b);
    r = clamp255((r - l) * c.s + l); g = clamp255((g - l) * c.s + l); b = clamp255((b - l) * c.s + l);
  }
  const float hr = clamp255((r * c.m[0] + g * c.m[1]) + b * c.m[2]);
  const float hg = clamp255((r * c.m[3] + g * c.m[4]) + b * c.m[5]);
  const float hb = clamp255((r * c.m[6] + g * c.m[7]) + b * c.m[8]);
  r = hr; g = hg; b = hb;
}

JR_DEVICE float blend(float t00, float t01, float t10, float t11, float wx, float wy) {
  const float top = t00 + wx * (t01 - t00);
  const float bot = t10 + wx * (t11 - t10);
  return top + wy * (bot - top);
}

// source position of resized coordinate u: taps lo / hi in [0, size - 1] and the weight of hi
JR_DEVICE void source_pos(int u, float ratio, int size, int& lo, int& hi, float& wgt) {
  const float s = fminf(fmaxf(((float)u + 0.5f) * ratio - 0.5f, 0.f), (float)(size - 1));
  const float f = floorf(s);
  wgt = s - f;
  lo = min(max((int)f, 0), size - 1);   // clamped whatever the record says: never an out-of-bounds read
  hi = min(lo + 1, size - 1);
}

// One output pixel of both images from its 4 taps (ty[q], tx[q]) of frames p1 / p2 with rows of
// `pitch` pixels: a1 / a2 receive the 3 channels in [-1, 1].  rec: the record's ints (the eraser
// rectangles of image 2).
JR_DEVICE void image_pixel(const unsigned char* __restrict__ p1, const unsigned char* __restrict__ p2, int pitch,
                           const int ty[4], const int tx[4], float wx, float wy, const int* __restrict__ rec, int nrect,
                           const Colour& c1, const Colour& c2, float* a1, float* a2) {
  float t1[4][3], t2[4][3];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long o = (long)ty[q] * pitch + tx[q];
    t1[q][0] = (float)p1[o * 3]; t1[q][1] = (float)p1[o * 3 + 1]; t1[q][2] = (float)p1[o * 3 + 2];
    texel(t1[q][0], t1[q][1], t1[q][2], c1);
    bool erased = false;
#pragma unroll
    for (int j = 0; j < 2; ++j)
      erased |= j < nrect && tx[q] >= rec[I_RECT + 4 * j] && tx[q] < rec[I_RECT + 4 * j + 2] &&
                ty[q] >= rec[I_RECT + 4 * j + 1] && ty[q] < rec[I_RECT + 4 * j + 3];
    t2[q][0] = erased ? c2.mean[0] : (float)p2[o * 3];
    t2[q][1] = erased ? c2.mean[1] : (float)p2[o * 3 + 1];
    t2[q][2] = erased ? c2.mean[2] : (float)p2[o * 3 + 2];
    texel(t2[q][0], t2[q][1], t2[q][2], c2);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a1[c] = blend(t1[0][c], t1[1][c], t1[2][c], t1[3][c], wx, wy) / 255.0f * 2.0f - 1.0f;
    a2[c] = blend(t2[0][c], t2[1][c], t2[2][c], t2[3][c], wx, wy) / 255.0f * 2.0f - 1.0f;
  }
}

// Dense ground truth: the blend of the 4 flow taps of a frame pf with rows of `pitch` pixels (before the scale).
JR_DEVICE void flow_blend(const float* __restrict__ pf, int pitch, const int ty[4], const int tx[4], float wx, float wy,
                          float& fx, float& fy) {
  float tf[4][2];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float2 f = *(const float2*)(pf + ((long)ty[q] * pitch + tx[q]) * 2);
    tf[q][0] = f.x; tf[q][1] = f.y;
  }
  fx = blend(tf[0][0], tf[1][0], tf[2][0], tf[3][0], wx, wy);
  fy = blend(tf[0][1], tf[1][1], tf[2][1], tf[3][1], wx, wy);
}

constexpr int MAX_SCAN = 16;    // candidates per axis at most (a valid sparse record needs sx + 5 <= 9)

// Source indices that can land on target T (train/augment.py:scan_window is the same formula):
// rint(fp32(s) * inv) == T needs |s * inv - T| <= 0.5 up to rounding, i.e. s within
// (T -+ 0.5) * ratio; fp32(s) * inv is monotone in s, and the rounding of the two products and
// of ratio and inv (sizes below 2^18: a few 2^-6 in source pixels) is far inside the margin of 1.
JR_DEVICE void scan_window(int T, float ratio, int size, int& lo, int& hi) {
  lo = max((int)floorf(((float)T - 0.5f) * ratio) - 1, 0);
  hi = min((int)ceilf(((float)T + 0.5f) * ratio) + 1, size - 1);
  lo = max(lo, hi - (MAX_SCAN - 1));
}

// Sparse ground truth: the winner of cell (v, u), i.e. the source pixel with the largest linear index
// whose valid byte is set and that lands on the cell, as an offset ys * pitch + xs into a frame with
// rows of `pitch` pixels, or -1.  ys_lo .. ys_hi: the row window of v; Ws: the sample's width.
JR_DEVICE long sparse_winner(const unsigned char* __restrict__ pv, int pitch, int v, int u, int ys_lo, int ys_hi, float sx,
                             float isx, float isy, int Ws) {
  int xs_lo, xs_hi;
  scan_window(u, sx, Ws, xs_lo, xs_hi);
  long win = -1;
  for (int ys = ys_hi; ys >= ys_lo && win < 0; --ys) {
    if (rintf((float)ys * isy) != (float)v) continue;
    for (int xs = xs_hi; xs >= xs_lo; --xs)
      if (rintf((float)xs * isx) == (float)u && pv[(long)ys * pitch + xs] != 0) {
        win = (long)ys * pitch + xs;
        break;
      }
  }
  return win;
}

// The flow of one output pixel from its source value (fx, fy): the scale, the flips, the range check
// (false for NaN; `landed`: a sparse cell without a winner is not valid), 0 where not valid.
JR_DEVICE void flow_pixel(float fx, float fy, bool landed, float isx, float isy, bool hflip, bool vflip, float* fl,
                          float* va) {
  fx = fx * isx;
  fy = fy * isy;
  if (hflip) fx = -fx;
  if (vflip) fy = -fy;
  const bool ok = landed && fabsf(fx) < 1000.f && fabsf(fy) < 1000.f;
  fl[0] = ok ? fx : 0.f;
  fl[1] = ok ? fy : 0.f;
  *va = ok ? 1.f : 0.f;
}

// The run of 4 pixels that starts at output pixel px (column x4 of a row of w): a1 / a2 [12],
// fl [8], va [4].
JR_DEVICE void store_run(float* __restrict__ o1, float* __restrict__ o2, float* __restrict__ oflow,
                         float* __restrict__ ovalid, long px, int x4, int w, const float* a1, const float* a2,
                         const float* fl, const float* va) {
  if ((w & 3) == 0) {                           // every run starts at a multiple of 4 pixels: 16-byte stores
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      *(float4*)(o1 + px * 3 + 4 * j) = make_float4(a1[4 * j], a1[4 * j + 1], a1[4 * j + 2], a1[4 * j + 3]);
      *(float4*)(o2 + px * 3 + 4 * j) = make_float4(a2[4 * j], a2[4 * j + 1], a2[4 * j + 2], a2[4 * j + 3]);
    }
    *(float4*)(oflow + px * 2) = make_float4(fl[0], fl[1], fl[2], fl[3]);
    *(float4*)(oflow + px * 2 + 4) = make_float4(fl[4], fl[5], fl[6], fl[7]);
    *(float4*)(ovalid + px) = make_float4(va[0], va[1], va[2], va[3]);
  } else {                                      // rows start at any pixel: scalar stores, the tail cut off
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x4 + k < w) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { o1[(px + k) * 3 + c] = a1[3 * k + c]; o2[(px + k) * 3 + c] = a2[3 * k + c]; }
        oflow[(px + k) * 2] = fl[2 * k];
        oflow[(px + k) * 2 + 1] = fl[2 * k + 1];
        ovalid[px + k] = va[k];
      }
  }
}

}  // namespace augment_dev
