// The per-coordinate sampler of scipy.ndimage.map_coordinates(mode='constant') shared by mt_affine_sample (prep.hip: affine
// coordinate field) and mt_warp_sample (warp.hip: affine field of a displaced mesh).  The caller computes the input coordinate
// (xd, xh, xw) of one output voxel in double; everything after that — range check, stencil, mirror rule, the four modes — is here,
// so both kernels give the same bits for the same coordinate.
#pragma once
#include "mt_common.h"

struct AffineParams {
  const float* src; float* dst; const float* mats;     // mats: per sample 12 floats = 3x3 matrix M (row-major) + centre (3)
  int planar;                                           // 1: "dummy 2D" — D is a stack of independent slices (xd = od), M acts on (h, w) only
  int N, C, D, H, W, OD, OH, OW, mode;                  // mode 0 nearest, 1 linear, 3 cubic (src = prefiltered coefficients), 11 per-label linear
  float cval;
};
__device__ __forceinline__ int mt_mirror(int i, int n) {
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  i = i < 0 ? -i : i;
  i %= period;
  return i > n - 1 ? period - i : i;
}
// output voxel r = (od, oh, ow) of sample n reads the input at (xd, xh, xw).  The coordinate is range-checked in double BEFORE any
// conversion to an integer index; the comparisons are written so that a NaN (or an infinity) fails them and yields cval.
__device__ __forceinline__ void mt_sample_point(const AffineParams& P, int n, long r, int od, double xd, double xh, double xw) {
  const long ovol = (long)P.OD * P.OH * P.OW;
  const size_t V = (size_t)P.D * P.H * P.W;
  const bool inside = xd >= 0.0 && xd <= (double)(P.D - 1) && xh >= 0.0 && xh <= (double)(P.H - 1) && xw >= 0.0 && xw <= (double)(P.W - 1);
  const float* sn = P.src + (size_t)n * P.C * V;
  float* dn = P.dst + (size_t)n * P.C * ovol + r;
  if (!inside) {
    for (int c = 0; c < P.C; ++c) dn[(size_t)c * ovol] = (P.mode == 11) ? 0.f : P.cval;      // per-label rule: nothing reaches 0.5
    return;
  }
  if (P.mode == 0) {
    const int a = (int)floor(xd + 0.5), b = (int)floor(xh + 0.5), e = (int)floor(xw + 0.5);
    const size_t o = ((size_t)(a > P.D - 1 ? P.D - 1 : a) * P.H + (b > P.H - 1 ? P.H - 1 : b)) * P.W + (e > P.W - 1 ? P.W - 1 : e);
    for (int c = 0; c < P.C; ++c) dn[(size_t)c * ovol] = sn[(size_t)c * V + o];
    return;
  }
  if (P.mode == 1 || P.mode == 11) {
    const int d0 = (int)floor(xd), h0 = (int)floor(xh), w0 = (int)floor(xw);
    const float fd = (float)(xd - d0), fh = (float)(xh - h0), fw = (float)(xw - w0);
    const int d1 = mt_mirror(d0 + 1, P.D), h1 = mt_mirror(h0 + 1, P.H), w1 = mt_mirror(w0 + 1, P.W);
    size_t off[8]; float wt[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int a = (k & 4) ? d1 : d0, b = (k & 2) ? h1 : h0, e = (k & 1) ? w1 : w0;
      off[k] = ((size_t)a * P.H + b) * P.W + e;
      wt[k] = ((k & 4) ? fd : 1.f - fd) * ((k & 2) ? fh : 1.f - fh) * ((k & 1) ? fw : 1.f - fw);
    }
    for (int c = 0; c < P.C; ++c) {
      const float* s = sn + (size_t)c * V;
      if (P.mode == 1) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) v += wt[k] * s[off[k]];
        dn[(size_t)c * ovol] = v;
      } else {                       // per-label: the largest label whose indicator interpolates to >= 0.5 (ascending override)
        float lab[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) lab[k] = s[off[k]];
        float best = 0.f; bool any = false;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float sum = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) sum += (lab[j] == lab[k]) ? wt[j] : 0.f;
          if (sum >= 0.5f && (!any || lab[k] > best)) { best = lab[k]; any = true; }
        }
        dn[(size_t)c * ovol] = any ? best : 0.f;
      }
    }
    return;
  }
  // cubic B-spline on prefiltered coefficients
  int id[4], ih[4], iw[4]; float wd[4], wh[4], ww[4];
  {
    const double x[3] = {xd, xh, xw};
    const int dims[3] = {P.D, P.H, P.W};
    int* idx[3] = {id, ih, iw}; float* wgt[3] = {wd, wh, ww};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int i0 = (int)floor(x[a]) - 1;
      const double t = x[a] - floor(x[a]);
      wgt[a][0] = (float)((1.0 - t) * (1.0 - t) * (1.0 - t) / 6.0);
      wgt[a][1] = (float)((4.0 - 6.0 * t * t + 3.0 * t * t * t) / 6.0);
      wgt[a][2] = (float)((1.0 + 3.0 * t + 3.0 * t * t - 3.0 * t * t * t) / 6.0);
      wgt[a][3] = (float)(t * t * t / 6.0);
#pragma unroll
      for (int k = 0; k < 4; ++k) idx[a][k] = mt_mirror(i0 + k, dims[a]);
    }
  }
  if (P.planar) { wd[0] = 0.f; wd[1] = 1.f; wd[2] = 0.f; wd[3] = 0.f; id[1] = od; }      // slices are independent images: no D stencil
  for (int c = 0; c < P.C; ++c) {
    const float* s = sn + (size_t)c * V;
    float v = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float va = 0.f;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float* row = s + ((size_t)id[a] * P.H + ih[b]) * P.W;
        va += wh[b] * (ww[0] * row[iw[0]] + ww[1] * row[iw[1]] + ww[2] * row[iw[2]] + ww[3] * row[iw[3]]);
      }
      v += wd[a] * va;
    }
    dn[(size_t)c * ovol] = v;
  }
}
