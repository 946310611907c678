// Per-line arithmetic of the resize unit (resize.hip): mt_resize_prefilter3, mt_resize, mt_resize_labels, mt_resize_labels_axis.
// The semantics are the reference's resample_data_or_seg (preprocessing/preprocessing.py:109-197) with the project's standing
// delegate for the absent skimage: skimage.transform.resize(order, mode='edge', anti_aliasing=False) is
// scipy.ndimage.zoom(order, mode='nearest', grid_mode=True); the z pass is scipy.ndimage.map_coordinates(order_z, mode='nearest').
// Both sample output index o of an axis resized from n_in to n_out at  x = (o + 0.5) * n_in / n_out - 0.5.
//
// scipy's 'nearest' rule is the line extended by its edge values to infinity on both sides.  Nothing is padded here: everything the
// extension contributes has a closed form in the line's own elements (z = sqrt(3) - 2, the pole of the cubic B-spline filter):
//   prefilter   c+[k] = 6 x[k] + z c+[k-1],  c[k] = z (c[k+1] - c+[k]);
//               causal start      c+[-1] = 6 x[0] / (1 - z)          (the steady state of a constant input; hence c+[0] = c+[-1]);
//               anticausal start  c[n-1] = -(s z / (1 - z) + (c+[n-1] - s) z / (1 - z^2)),  s = 6 x[n-1] / (1 - z)
//               (to the right of the line c+[n-1+m] = s + (c+[n-1] - s) z^m, and c[n-1] = -z sum_m z^m c+[n-1+m]);
//   extension   on the constant part the coefficients obey c[k-1] + 4 c[k] + c[k+1] = 6 x0 and decay towards x0:
//               c[-m] = x0 + (c[0] - x0) z^m,  x0 = ((4 + z) c[0] + c[1]) / (5 + z)   (x0 is the edge value, recovered from the STORED
//               coefficients alone); the end of the line is the mirror image (c[n-1], c[n-2]); for n == 1 every coefficient is the
//               value itself.  c[-m] is linear in (c[0], c[1]), so a tap that falls off the line is folded into the weights of the
//               two taps next to the edge: the sampler reads stored elements only and its loops do not depend on where it is.
//   order 3     four taps floor(x) - 1 .. floor(x) + 2, the coordinate is NOT clamped (with x in [-0.5, n - 0.5) they span -2 .. n + 1);
//   order 1     the coordinate is clamped to [0, n - 1];   order 0   floor(x + 0.5), clamped;
//   n_in == n_out   x = o exactly and every order returns the input: one tap of weight 1 (the axis must NOT be prefiltered).
// Plain C++ that the device kernels and a host program compile alike (tests/test_resampling_cases_cpu.py builds
// tests/resize_line_host.cpp with the address and undefined-behaviour sanitizers); tests/resampling_cases.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MT_HD __host__ __device__
#else
#define MT_HD
#endif

#define MT_RS_POLE (-0.26794919243112270647)        /* sqrt(3) - 2 */

// The coordinate is scipy's own sequence of double operations, each rounded: at order 0 an output index whose coordinate lies exactly
// between two source elements (in/out = 4/3: every third one) then picks the neighbour scipy picks.  A fused multiply-add would not
// round the product and falls on the other side there, so contraction is switched off for this function.
static inline MT_HD double mt_rs_coord(int o, int n_in, int n_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double scale = (double)n_in / (double)n_out;
  const double p = ((double)o + 0.5) * scale;
  return p - 0.5;
}

// ---- prefilter
static inline MT_HD double mt_rs_causal_start(double x_first) { return 6.0 * x_first / (1.0 - MT_RS_POLE); }      // c+[-1] = c+[0]
static inline MT_HD double mt_rs_anticausal_start(double cp_last, double x_last) {                                   // c[n-1]
  const double z = MT_RS_POLE, s = 6.0 * x_last / (1.0 - z);
  return -(s * z / (1.0 - z) + (cp_last - s) * z / (1.0 - z * z));
}

// ---- extension: c[-m] = a c[0] + b c[1]  (m = 1, 2; the same pair serves c[n-1+m] with c[n-1], c[n-2])
static inline MT_HD void mt_rs_fold(int m, double* a, double* b) {
  const double z = MT_RS_POLE, zm = m == 1 ? z : z * z;
  *b = (1.0 - zm) / (5.0 + z);
  *a = (4.0 + z) * *b + zm;
}
static inline MT_HD double mt_rs_extend(double c0, double c1, int m) {
  double a, b;
  mt_rs_fold(m, &a, &b);
  return a * c0 + b * c1;
}

// ---- cubic B-spline weights of the taps floor(x) - 1 .. floor(x) + 2 for t = x - floor(x)
static inline MT_HD void mt_rs_weights3(double t, double w[4]) {
  const double u = 1.0 - t;
  w[0] = u * u * u / 6.0;
  w[1] = (3.0 * t * t * t - 6.0 * t * t + 4.0) / 6.0;
  w[2] = (3.0 * u * u * u - 6.0 * u * u + 4.0) / 6.0;
  w[3] = t * t * t / 6.0;
}

// first tap of output index o at order 3 (floor(x) - 1, -2 .. n_in - 2) — the tap range the tests walk
static inline MT_HD int mt_rs_tap_base3(int o, int n_in, int n_out) { return (int)floor(mt_rs_coord(o, n_in, n_out)) - 1; }

// number of taps per output index: fixed by the arguments of a call, never by data or position
static inline MT_HD int mt_rs_ntaps(int order, int n_in, int n_out) { return n_in == n_out || order == 0 ? 1 : order == 1 ? 2 : 4; }

// The taps of output index o: idx[k] in [0, n_in) and w[k], k < mt_rs_ntaps(...); out[o] = sum_k w[k] line[idx[k]].
static inline MT_HD int mt_rs_taps(int order, int o, int n_in, int n_out, int idx[4], double w[4]) {
  if (n_in == n_out) { idx[0] = o; w[0] = 1.0; return 1; }
  const double x = mt_rs_coord(o, n_in, n_out);         // in [-0.5, n_in - 0.5): every conversion below is defined
  if (order == 0) {
    int i = (int)floor(x + 0.5);
    idx[0] = i < 0 ? 0 : i > n_in - 1 ? n_in - 1 : i; w[0] = 1.0;
    return 1;
  }
  if (order == 1) {
    const double xc = x < 0.0 ? 0.0 : x > (double)(n_in - 1) ? (double)(n_in - 1) : x;
    const int i = (int)floor(xc);
    const double t = xc - (double)i;
    idx[0] = i; idx[1] = i + 1 < n_in ? i + 1 : n_in - 1;
    w[0] = 1.0 - t; w[1] = t;
    return 2;
  }
  const double fl = floor(x);
  const int base = (int)fl - 1;
  mt_rs_weights3(x - fl, w);
  if (n_in == 1) {                                       // every coefficient of the extended line is the value
    w[0] = w[0] + w[1] + w[2] + w[3]; w[1] = w[2] = w[3] = 0.0;
    idx[0] = idx[1] = idx[2] = idx[3] = 0;
    return 4;
  }
  double a1, b1, a2, b2;
  mt_rs_fold(1, &a1, &b1);
  mt_rs_fold(2, &a2, &b2);
  // Written out per case (no indexing by position, so the four weights stay in registers on the device).
  // Start: base == -2 drops taps -2, -1 (elements 0, 1 sit in slots 2, 3); base == -1 drops tap -1 (elements 0, 1 in slots 1, 2).
  if (base == -2) { w[2] += w[0] * a2 + w[1] * a1; w[3] += w[0] * b2 + w[1] * b1; w[0] = 0.0; w[1] = 0.0; }
  else if (base == -1) { w[1] += w[0] * a1; w[2] += w[0] * b1; w[0] = 0.0; }
  // End: `over` taps lie beyond element n_in - 1.  over == 2: elements n_in - 1, n_in - 2 sit in slots 1, 0; over == 1: in slots 2, 1.
  const int over = base + 3 - (n_in - 1);
  if (over == 2) { w[1] += w[2] * a1 + w[3] * a2; w[0] += w[2] * b1 + w[3] * b2; w[2] = 0.0; w[3] = 0.0; }
  else if (over == 1) { w[2] += w[3] * a1; w[1] += w[3] * b1; w[3] = 0.0; }
  for (int k = 0; k < 4; ++k) { const int i = base + k; idx[k] = i < 0 ? 0 : i > n_in - 1 ? n_in - 1 : i; }
  return 4;
}

// ---- the label rule: among `n` taps (label, weight) the LARGEST label whose summed weight reaches one half wins (the labels apply
// in ascending order, a later one overwrites); 0 where none does — 0, not -1, and -1 is a label like any other.
//   strict == 0: weight >= 0.5 (batchgenerators' resize_segmentation, the in-plane / 3D rule);
//   strict == 1: weight >  0.5 (the z pass, preprocessing.py:176-184: np.round sends 0.5 to 0 and the test is `> 0.5`).
// A slot with a negative weight is unused (the kernel keeps eight slots whatever the number of axes that change).
static inline MT_HD float mt_rs_label_vote(const float* lab, const double* w, int n, int strict) {
  float res = 0.f; int found = 0;
  for (int k = 0; k < n; ++k) {
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += (w[j] >= 0.0 && lab[j] == lab[k]) ? w[j] : 0.0;
    const int wins = w[k] >= 0.0 && (strict ? s > 0.5 : s >= 0.5);
    if (wins && (!found || lab[k] > res)) { res = lab[k]; found = 1; }
  }
  return res;
}
