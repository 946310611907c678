// Intensity augmentation of the moreDA chain on the device (data_augmentation_moreDA.py:90-106: BrightnessMultiplicativeTransform,
// ContrastAugmentationTransform and the two GammaTransforms) without a device-to-host read:
//   mt_channel_stats     min, max, mean and population sd of every requested channel of a batch x[NC][V] in ONE streaming pass
//                        (4 bytes per element), left in device memory as doubles;
//   mt_intensity_apply   one fused in-place pass (8 bytes per element) over the batch: per channel one op record that travels in
//                        the kernel arguments, its statistics read from the device arrays mt_channel_stats wrote.
// Both are HBM-bound streams of 16-byte, dword-aligned loads (a channel starts at x + c * V) with a scalar tail.  The op of a
// channel is uniform per workgroup (grid.y = channel): the loop is instantiated per op, so a channel that is only scaled never
// pays for the power of its neighbour.  Sums are formed in a fixed order without atomics: bit-identical from run to run.
#include "stream_common.h"
#include <math.h>

#define IA_THREADS 256
#define IA_WAVES (IA_THREADS / MT_WAVE)
#define IA_CHUNK 64              // channels per launch: their activity mask / op records travel in the kernel arguments

#define IA_STAT_QUADS 4          // 16-byte loads per thread of the statistics pass before the grid-stride loop wraps: its reduction
                                 // epilogue (shuffles, LDS, one partial per workgroup) is paid once per 4096 elements

static int ia_blocks(long V) { return mt_stream_blocks((V + 3) / 4, IA_THREADS); }
static int ia_stat_blocks(long V) { return mt_stream_blocks((V + 3) / 4, IA_THREADS * IA_STAT_QUADS); }

// ---- statistics ----------------------------------------------------------------------------------------------------------------
// One pass, shifted: with K = x[0] of the channel, every thread accumulates sum(d) and sum(d * d) of d = x - K in double.  K is a
// sample of the channel, so (K - mean)^2 <= V * variance: the cancellation in  s2 - s1^2 / V  costs at most log2(V) <= 31 of the 53
// bits, whatever the ratio of mean to sd (a channel of mean 100 and sd 1 has d of order 1).  Min and max are exact in float32.
// Non-finite elements follow numpy.  The shift is 0 when x[0] is not finite, so d is NaN exactly where x is: sum(d * d) - a sum of
// non-negative terms, infinite ones included - is NaN exactly when the channel holds a NaN, and then all four statistics are NaN
// (fminf / fmaxf alone would drop it).  The streaming loop pays nothing for this.  With an infinite element and no NaN, min and
// max are exact, the mean is numpy's (+-inf, or NaN with both signs) and the sd is NaN.
struct StatParams { const float* x; long V; int c0, nblk; uint64_t active; double* part; /* [NC][nblk][4]: min, max, s1, s2 */ };
__device__ __forceinline__ float ia_shift(float x0) { return fabsf(x0) < __builtin_huge_valf() ? x0 : 0.f; }

__global__ __launch_bounds__(IA_THREADS) void channel_stats_kernel(const StatParams P) {
  if (!(P.active >> blockIdx.y & 1ull)) return;
  const int c = P.c0 + (int)blockIdx.y;
  const float* x = P.x + (size_t)c * P.V;
  const float x0 = x[0], k = ia_shift(x0);
  const long nquad = P.V / 4;
  const long gtid = (long)blockIdx.x * IA_THREADS + threadIdx.x, gstride = (long)gridDim.x * IA_THREADS;
  float lo = x0, hi = x0;
  double a1[4] = {0.0, 0.0, 0.0, 0.0}, a2[4] = {0.0, 0.0, 0.0, 0.0};      // one pair of sums per quad component: four short chains
#pragma unroll 4                 // = IA_STAT_QUADS: the loads of a thread's quads are issued together
  for (long q = gtid; q < nquad; q += gstride) {
    const mt_f4 a = *(const mt_f4*)(x + 4 * q);
    const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lo = fminf(lo, av[j]); hi = fmaxf(hi, av[j]);
      const double d = (double)av[j] - (double)k;
      a1[j] += d; a2[j] += d * d;
    }
  }
  for (long v = 4 * nquad + gtid; v < P.V; v += gstride) {
    const float a = x[v];
    lo = fminf(lo, a); hi = fmaxf(hi, a);
    const double d = (double)a - (double)k;
    a1[0] += d; a2[0] += d * d;
  }
  double s1 = (a1[0] + a1[1]) + (a1[2] + a1[3]), s2 = (a2[0] + a2[1]) + (a2[2] + a2[3]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { lo = fminf(lo, __shfl_xor(lo, off, MT_WAVE)); hi = fmaxf(hi, __shfl_xor(hi, off, MT_WAVE)); }
  s1 = mt_wave_sum_d(s1);
  s2 = mt_wave_sum_d(s2);
  __shared__ double sh[IA_WAVES][4];
  const int wave = threadIdx.x / MT_WAVE, lane = threadIdx.x % MT_WAVE;
  if (lane == 0) { sh[wave][0] = lo; sh[wave][1] = hi; sh[wave][2] = s1; sh[wave][3] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double l = sh[0][0], h = sh[0][1], t1 = sh[0][2], t2 = sh[0][3];
    for (int w = 1; w < IA_WAVES; ++w) { l = fmin(l, sh[w][0]); h = fmax(h, sh[w][1]); t1 += sh[w][2]; t2 += sh[w][3]; }
    double* o = P.part + ((size_t)c * P.nblk + blockIdx.x) * 4;
    o[0] = l; o[1] = h; o[2] = t1; o[3] = t2;
  }
}

// One wave per channel: lane l combines partials l, l + 64, ... in that order, then the butterfly (a fixed tree).
__global__ __launch_bounds__(MT_WAVE) void channel_stats_finalize_kernel(const StatParams P, double* __restrict__ stats) {
  if (!(P.active >> blockIdx.x & 1ull)) return;
  const int c = P.c0 + (int)blockIdx.x;
  const double* p = P.part + (size_t)c * P.nblk * 4;
  const double k = (double)ia_shift(P.x[(size_t)c * P.V]);
  double lo = __builtin_huge_val(), hi = -__builtin_huge_val(), s1 = 0.0, s2 = 0.0;
  for (int b = threadIdx.x; b < P.nblk; b += MT_WAVE) { lo = fmin(lo, p[4 * b]); hi = fmax(hi, p[4 * b + 1]); s1 += p[4 * b + 2]; s2 += p[4 * b + 3]; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { lo = fmin(lo, __shfl_xor(lo, off, MT_WAVE)); hi = fmax(hi, __shfl_xor(hi, off, MT_WAVE)); }
  s1 = mt_wave_sum_d(s1);
  s2 = mt_wave_sum_d(s2);
  if (threadIdx.x == 0) {
    const double n = (double)P.V, var = (s2 - s1 * s1 / n) / n;
    double* o = stats + (size_t)c * 4;
    if (s2 != s2) lo = hi = s2;                                   // a NaN element
    o[0] = lo; o[1] = hi; o[2] = k + s1 / n; o[3] = var > 0.0 ? sqrt(var) : (var != var ? var : 0.0);
  }
}

extern "C" size_t mt_channel_stats_workspace(int NC, long V) {
  if (NC < 1 || V < 1 || V > (long)INT32_MAX) return 0;
  return (size_t)NC * ia_stat_blocks(V) * 4 * sizeof(double);
}

extern "C" int mt_channel_stats(const float* x, int NC, long V, const uint8_t* active, double* stats, void* ws, size_t ws_bytes,
                                mt_stream_t stream) {
  MT_REQUIRE(x && stats && ws, "channel_stats: null pointer");
  MT_REQUIRE(NC >= 1 && V >= 1, "channel_stats: bad shape %d x %ld", NC, V);
  MT_REQUIRE(V <= (long)INT32_MAX, "channel_stats: %ld elements per channel exceed the int32 index range", V);
  MT_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)stats & 7) == 0 && ((uintptr_t)ws & 7) == 0, "channel_stats: misaligned pointer");
  MT_REQUIRE(ws_bytes >= mt_channel_stats_workspace(NC, V), "channel_stats: workspace of %zu bytes, %zu needed", ws_bytes,
             mt_channel_stats_workspace(NC, V));
  StatParams P;
  P.x = x; P.V = V; P.nblk = ia_stat_blocks(V); P.part = (double*)ws;
  hipStream_t s = (hipStream_t)stream;
  for (int c0 = 0; c0 < NC; c0 += IA_CHUNK) {
    const int n = NC - c0 < IA_CHUNK ? NC - c0 : IA_CHUNK;
    P.c0 = c0; P.active = 0;
    for (int c = 0; c < n; ++c) if (!active || active[c0 + c]) P.active |= 1ull << c;
    if (!P.active) continue;
    hipLaunchKernelGGL(channel_stats_kernel, dim3(P.nblk, n), dim3(IA_THREADS), 0, s, P);
    hipLaunchKernelGGL(channel_stats_finalize_kernel, dim3(n), dim3(MT_WAVE), 0, s, P, stats);
    MT_CHECK_LAUNCH("channel_stats");
  }
  return MT_OK;
}

// ---- apply -----------------------------------------------------------------------------------------------------------------------
// Float32 throughout, every product and sum rounded on its own (no contraction into an FMA: numpy and torch do not fuse either),
// true divisions.  The statistics are rounded to float32 once, before the loop.
struct ApplyParams { float* x; long V; int c0; const double* stats; const double* stats2; mt_intensity_op_t rec[IA_CHUNK]; };
struct IaCoef { float a, b, lo, hi, p, q; int flag; };

template <int OP> __device__ __forceinline__ float ia_one(float x, const IaCoef& K) {
#pragma clang fp contract(off)
  if (OP == MT_INTENSITY_SCALE) return x * K.a;
  if (OP == MT_INTENSITY_CONTRAST) {                    // a = factor, p = mean, [lo, hi] = [min, max]
    float y = (x - K.p) * K.a + K.p;
    if (K.flag) y = fminf(fmaxf(y, K.lo), K.hi);
    return y;
  }
  const float y = K.flag ? -x : x;
  float r;
  if (OP == MT_INTENSITY_GAMMA)                         // a = gamma, lo = min, p = max - min, q = max - min + eps
    r = powf((y - K.lo) / K.q, K.a) * K.p + K.lo;
  else                                                  // RESTORE: p = mean1, q = sd1 + 1e-8, a = sd0, b = mean0
    r = (y - K.p) / K.q * K.a + K.b;
  return K.flag ? -r : r;
}

template <int OP> __device__ __forceinline__ void ia_run(float* __restrict__ x, long V, const IaCoef K) {
  const long nquad = V / 4;
  const long gtid = (long)blockIdx.x * IA_THREADS + threadIdx.x, gstride = (long)gridDim.x * IA_THREADS;
  for (long q = gtid; q < nquad; q += gstride) {
    mt_f4 a = *(const mt_f4*)(x + 4 * q);
    a.x = ia_one<OP>(a.x, K); a.y = ia_one<OP>(a.y, K); a.z = ia_one<OP>(a.z, K); a.w = ia_one<OP>(a.w, K);
    *(mt_f4*)(x + 4 * q) = a;
  }
  for (long v = 4 * nquad + gtid; v < V; v += gstride) x[v] = ia_one<OP>(x[v], K);
}

__global__ __launch_bounds__(IA_THREADS) void intensity_apply_kernel(const ApplyParams P) {
#pragma clang fp contract(off)
  const mt_intensity_op_t R = P.rec[blockIdx.y];
  if (R.op == MT_INTENSITY_NONE) return;
  const int c = P.c0 + (int)blockIdx.y;
  float* x = P.x + (size_t)c * P.V;
  const int neg = R.op >= MT_INTENSITY_GAMMA && (R.flags & MT_INTENSITY_NEGATE) != 0;
  IaCoef K;
  K.a = R.a; K.b = 0.f; K.lo = 0.f; K.hi = 0.f; K.p = 0.f; K.q = 1.f; K.flag = 0;
  float mn = 0.f, mx = 0.f, mean = 0.f, sd = 0.f;
  if (R.op != MT_INTENSITY_SCALE) {                     // the statistics of y = -x from those of x: min <-> -max, mean -> -mean
    const double* s = P.stats + (size_t)c * 4;
    const float m0 = (float)s[0], m1 = (float)s[1];
    mn = neg ? -m1 : m0; mx = neg ? -m0 : m1; mean = neg ? -(float)s[2] : (float)s[2]; sd = (float)s[3];
  }
  switch (R.op) {
    case MT_INTENSITY_SCALE: ia_run<MT_INTENSITY_SCALE>(x, P.V, K); break;
    case MT_INTENSITY_CONTRAST:
      K.p = mean; K.lo = mn; K.hi = mx;
      K.flag = (R.flags & MT_INTENSITY_PRESERVE_RANGE) != 0;
      ia_run<MT_INTENSITY_CONTRAST>(x, P.V, K); break;
    case MT_INTENSITY_GAMMA:
      K.lo = mn; K.p = mx - mn; K.q = K.p + R.b; K.flag = neg;
      ia_run<MT_INTENSITY_GAMMA>(x, P.V, K); break;
    case MT_INTENSITY_RESTORE: {
      const double* s2 = P.stats2 + (size_t)c * 4;
      K.p = neg ? -(float)s2[2] : (float)s2[2]; K.q = (float)s2[3] + 1e-8f; K.a = sd; K.b = mean; K.flag = neg;
      ia_run<MT_INTENSITY_RESTORE>(x, P.V, K); break;
    }
    default: break;
  }
}

extern "C" int mt_intensity_apply(float* x, int NC, long V, const mt_intensity_op_t* records, const double* stats, const double* stats2,
                                  mt_stream_t stream) {
  MT_REQUIRE(x && records, "intensity_apply: null pointer");
  MT_REQUIRE(NC >= 1 && V >= 1, "intensity_apply: bad shape %d x %ld", NC, V);
  MT_REQUIRE(V <= (long)INT32_MAX, "intensity_apply: %ld elements per channel exceed the int32 index range", V);
  MT_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)stats & 7) == 0 && ((uintptr_t)stats2 & 7) == 0, "intensity_apply: misaligned pointer");
  for (int c = 0; c < NC; ++c) {
    const int op = records[c].op;
    MT_REQUIRE(op >= MT_INTENSITY_NONE && op <= MT_INTENSITY_RESTORE, "intensity_apply: record %d has the unknown op %d", c, op);
    MT_REQUIRE(op <= MT_INTENSITY_SCALE || stats, "intensity_apply: record %d (op %d) needs the statistics of mt_channel_stats", c, op);
    MT_REQUIRE(op != MT_INTENSITY_RESTORE || stats2, "intensity_apply: record %d (RESTORE) needs the second statistics", c);
  }
  ApplyParams P;
  P.x = x; P.V = V; P.stats = stats; P.stats2 = stats2;
  const int nblk = ia_blocks(V);
  for (int c0 = 0; c0 < NC; c0 += IA_CHUNK) {
    const int n = NC - c0 < IA_CHUNK ? NC - c0 : IA_CHUNK;
    bool any = false;
    for (int c = 0; c < IA_CHUNK; ++c) {
      if (c < n) P.rec[c] = records[c0 + c];
      else { P.rec[c].op = MT_INTENSITY_NONE; P.rec[c].flags = 0; P.rec[c].a = 0.f; P.rec[c].b = 0.f; }
      any = any || P.rec[c].op != MT_INTENSITY_NONE;
    }
    if (!any) continue;
    P.c0 = c0;
    hipLaunchKernelGGL(intensity_apply_kernel, dim3(nblk, n), dim3(IA_THREADS), 0, (hipStream_t)stream, P);
    MT_CHECK_LAUNCH("intensity_apply");
  }
  return MT_OK;
}
