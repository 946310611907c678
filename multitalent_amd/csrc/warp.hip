// warp.hip — elastic deformation of batchgenerators' SpatialTransform on the device (augment_spatial with do_elastic_deform,
// data_augmentation_moreDA.py:66-80 as nnUNetTrainerV2_DA3 / _insaneDA / the BraTS trainers configure it).
//
// elastic_deform_coordinates adds, per mesh axis, offsets = gaussian_filter(uniform(-1, 1), sigma, mode='constant', cval=0) * alpha
// to the zero-centred output mesh BEFORE rotation and scaling, so output voxel o of sample n reads the input at
//     x = M_n (g(o) + alpha_n f_n(o)) + centre_n.
// Two kernels:
//  * mt_gaussian_blur_axis_zero: one axis pass of that zero-padded Gaussian.  sigma is 9..13 in the reference's defaults, so the
//    radius int(4 sigma + 0.5) reaches 52 (105 taps): a workgroup stages its tile and the r-wide halo in LDS once (taps that fall
//    off the axis are staged as 0) and every output takes its taps from LDS — one global read (halo rows of neighbouring tiles
//    come from L2) and one write per element and pass.  Lanes run along W for every axis.  No atomics.
//  * mt_warp_sample: mt_affine_sample's kernel with the displaced mesh coordinate; the sampler itself is sample_common.h's.
#include "mt_common.h"
#include "sample_common.h"

#define MT_ZB_MAXR 64            // largest supported radius: sigma < 16.125
#define MT_ZB_CHUNK 32           // channels per launch (their sigmas travel in the kernel arguments)
#define MT_ZB_TL 64              // D / H passes: tile = 64 outputs along the axis x 64 lanes along the contiguous inner index
#define MT_ZB_RB 4               // D / H passes: outputs along the axis per thread and tap-loop (MT_ZB_TL = 4 waves x 4 groups of them)
#define MT_ZB_TW 256             // W pass: tile = 8 rows x 256 outputs along W
#define MT_ZB_RW 8
#define MT_ZB_PITCH (MT_ZB_TW + 2 * MT_ZB_MAXR)

struct ZeroBlurParams { const float* src; float* dst; int D, H, W, axis; float sigma[MT_ZB_CHUNK]; };

// w[k] = exp(-k^2 / 2 sigma^2) / sum for k = -r..r in double (scipy's _gaussian_kernel1d), left in wsh[0 .. 2r]; returns r.
// Called by every thread of a 256-thread workgroup with the same sigma > 0.
__device__ __forceinline__ int zero_blur_weights(float sg, double* wsh) {
  const int r = (int)(4.0 * (double)sg + 0.5);
  const int t = threadIdx.x;
  if (t <= 2 * r) { const double k = (double)(t - r); wsh[t] = exp(-0.5 * k * k / ((double)sg * sg)); }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int k = 0; k <= 2 * r; ++k) s += wsh[k];
    wsh[2 * MT_ZB_MAXR + 1] = s;
  }
  __syncthreads();
  if (t <= 2 * r) wsh[t] = wsh[t] / wsh[2 * MT_ZB_MAXR + 1];
  __syncthreads();
  return r;
}

// axis 0 (D) and 1 (H): the channel is [outer][L][inner] with inner contiguous (axis 0: outer 1, inner H*W; axis 1: outer D, inner W)
__global__ __launch_bounds__(256) void zero_blur_strided_kernel(const ZeroBlurParams P) {
  __shared__ double wsh[2 * MT_ZB_MAXR + 2];
  __shared__ float tile[(MT_ZB_TL + 2 * MT_ZB_MAXR) * 64];
  const float sg = P.sigma[blockIdx.y];
  const size_t V = (size_t)P.D * P.H * P.W;
  const float* src = P.src + (size_t)blockIdx.y * V;
  float* dst = P.dst + (size_t)blockIdx.y * V;
  const int L = P.axis == 0 ? P.D : P.H;
  const long inner = P.axis == 0 ? (long)P.H * P.W : (long)P.W;
  const long nit = (inner + 63) / 64, nlt = (L + MT_ZB_TL - 1) / MT_ZB_TL;
  long b = blockIdx.x;
  const long it = b % nit; b /= nit;
  const long lt = b % nlt, o = b / nlt;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long col = it * 64 + lane;
  const bool colok = col < inner;
  const int l0 = (int)lt * MT_ZB_TL;
  const int nl = L - l0 < MT_ZB_TL ? L - l0 : MT_ZB_TL;
  const size_t base = (size_t)o * L * inner + (size_t)(colok ? col : 0);
  if (sg <= 0.f) {
    if (colok) for (int j = wv; j < nl; j += 4) dst[base + (size_t)(l0 + j) * inner] = src[base + (size_t)(l0 + j) * inner];
    return;
  }
  const int r = zero_blur_weights(sg, wsh);
  for (int j = wv; j < nl + 2 * r; j += 4) {
    const int l = l0 - r + j;
    tile[j * 64 + lane] = (colok && l >= 0 && l < L) ? src[base + (size_t)l * inner] : 0.f;
  }
  __syncthreads();
  if (!colok) return;
  // a thread takes MT_ZB_RB consecutive outputs along the axis at a time: one weight read serves all of them (the tap loop is bound
  // by the double-precision FMAs, not by LDS).  Taps k = 0..2r of output pos read axis position pos - r + k; the loop runs over the
  // union of the on-axis taps of the group, the others were staged as 0.  Outputs past nl read unstaged LDS and are not stored.
  for (int j0 = wv * MT_ZB_RB; j0 < nl; j0 += 4 * MT_ZB_RB) {
    const int pos = l0 + j0;
    const int klo = r - (pos + MT_ZB_RB - 1) > 0 ? r - (pos + MT_ZB_RB - 1) : 0, khi = L - 1 - pos + r < 2 * r ? L - 1 - pos + r : 2 * r;
    const float* t = tile + j0 * 64 + lane;
    double acc[MT_ZB_RB];                                 // scipy's correlate1d accumulates in double
#pragma unroll
    for (int i = 0; i < MT_ZB_RB; ++i) acc[i] = 0.0;
    for (int k = klo; k <= khi; ++k) {
      const double w = wsh[k];
#pragma unroll
      for (int i = 0; i < MT_ZB_RB; ++i) acc[i] += w * (double)t[(k + i) * 64];
    }
#pragma unroll
    for (int i = 0; i < MT_ZB_RB; ++i)
      if (j0 + i < nl) dst[base + (size_t)(pos + i) * inner] = (float)acc[i];
  }
}

// axis 2 (W): the channel is D*H rows of W; a workgroup takes 8 rows x 256 outputs, lanes along W
__global__ __launch_bounds__(256) void zero_blur_w_kernel(const ZeroBlurParams P) {
  __shared__ double wsh[2 * MT_ZB_MAXR + 2];
  __shared__ float tile[MT_ZB_RW * MT_ZB_PITCH];
  const float sg = P.sigma[blockIdx.y];
  const size_t V = (size_t)P.D * P.H * P.W;
  const float* src = P.src + (size_t)blockIdx.y * V;
  float* dst = P.dst + (size_t)blockIdx.y * V;
  const int W = P.W;
  const long rows = (long)P.D * P.H, nwt = (W + MT_ZB_TW - 1) / MT_ZB_TW;
  const long wt = blockIdx.x % nwt, rt = blockIdx.x / nwt;
  const int w0 = (int)wt * MT_ZB_TW;
  const long row0 = rt * MT_ZB_RW;
  const int nr = rows - row0 < MT_ZB_RW ? (int)(rows - row0) : MT_ZB_RW;
  const int w = w0 + (int)threadIdx.x;
  if (sg <= 0.f) {
    if (w < W) for (int j = 0; j < nr; ++j) dst[(size_t)(row0 + j) * W + w] = src[(size_t)(row0 + j) * W + w];
    return;
  }
  const int r = zero_blur_weights(sg, wsh);
  const int span = MT_ZB_TW + 2 * r;
  for (int idx = threadIdx.x; idx < nr * span; idx += 256) {
    const int j = idx / span, q = idx % span;
    const int ws = w0 - r + q;
    tile[j * MT_ZB_PITCH + q] = (ws >= 0 && ws < W) ? src[(size_t)(row0 + j) * W + ws] : 0.f;
  }
  __syncthreads();
  if (w >= W) return;
  const int klo = r - w > 0 ? r - w : 0, khi = W - 1 - w + r < 2 * r ? W - 1 - w + r : 2 * r;
  // the tap loop is outermost so that one weight read serves all 8 rows; rows past nr read unstaged LDS and are not stored
  const float* t = tile + threadIdx.x;
  double acc[MT_ZB_RW];
#pragma unroll
  for (int j = 0; j < MT_ZB_RW; ++j) acc[j] = 0.0;
  for (int k = klo; k <= khi; ++k) {
    const double wk = wsh[k];
#pragma unroll
    for (int j = 0; j < MT_ZB_RW; ++j) acc[j] += wk * (double)t[j * MT_ZB_PITCH + k];
  }
#pragma unroll
  for (int j = 0; j < MT_ZB_RW; ++j)
    if (j < nr) dst[(size_t)(row0 + j) * W + w] = (float)acc[j];
}

extern "C" int mt_gaussian_blur_axis_zero(const float* src, float* dst, int NC, int D, int H, int W, int axis, const float* sigma,
                                          mt_stream_t stream) {
  MT_REQUIRE(src != nullptr && dst != nullptr && sigma != nullptr && src != dst, "gaussian_blur_axis_zero: null or aliased pointers");
  MT_REQUIRE(NC > 0 && D > 0 && H > 0 && W > 0 && axis >= 0 && axis <= 2, "gaussian_blur_axis_zero: bad geometry");
  for (int c = 0; c < NC; ++c)          // refused, never clamped: a clamped radius is a different filter
    MT_REQUIRE(sigma[c] <= 0.f || 4.0 * (double)sigma[c] + 0.5 < (double)(MT_ZB_MAXR + 1),
               "gaussian_blur_axis_zero: sigma[%d] = %g needs a radius above %d", c, (double)sigma[c], MT_ZB_MAXR);
  long tiles;
  if (axis == 2) tiles = (((long)D * H + MT_ZB_RW - 1) / MT_ZB_RW) * ((W + MT_ZB_TW - 1) / MT_ZB_TW);
  else {
    const long inner = axis == 0 ? (long)H * W : (long)W, outer = axis == 0 ? 1 : D;
    const int L = axis == 0 ? D : H;
    tiles = outer * ((L + MT_ZB_TL - 1) / MT_ZB_TL) * ((inner + 63) / 64);
  }
  MT_REQUIRE(tiles < (1L << 24), "gaussian_blur_axis_zero: %ld tiles per channel exceed the grid (256 threads each, 2^32 in all)", tiles);
  const size_t V = (size_t)D * H * W;
  for (int c0 = 0; c0 < NC; c0 += MT_ZB_CHUNK) {
    const int n = NC - c0 < MT_ZB_CHUNK ? NC - c0 : MT_ZB_CHUNK;
    ZeroBlurParams P;
    P.src = src + (size_t)c0 * V; P.dst = dst + (size_t)c0 * V; P.D = D; P.H = H; P.W = W; P.axis = axis;
    for (int c = 0; c < MT_ZB_CHUNK; ++c) P.sigma[c] = c < n ? sigma[c0 + c] : 0.f;
    if (axis == 2) hipLaunchKernelGGL(zero_blur_w_kernel, dim3((unsigned)tiles, n), dim3(256), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(zero_blur_strided_kernel, dim3((unsigned)tiles, n), dim3(256), 0, (hipStream_t)stream, P);
    MT_CHECK_LAUNCH("gaussian_blur_axis_zero");
  }
  return MT_OK;
}

struct WarpParams { AffineParams A; const float* field; const float* alpha; };
__global__ __launch_bounds__(256) void warp_sample_kernel(const WarpParams Q) {
  const AffineParams& P = Q.A;
  const long ohw = (long)P.OH * P.OW, ovol = (long)P.OD * ohw, total = (long)P.N * ovol;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int n = (int)(i / ovol);
    long r = i % ovol;
    const int ow = (int)(r % P.OW), oh = (int)((r / P.OW) % P.OH), od = (int)(r / ohw);
    const float* M = P.mats + n * 12;
    double gd = od - 0.5 * (P.OD - 1), gh = oh - 0.5 * (P.OH - 1), gw = ow - 0.5 * (P.OW - 1);
    const float al = Q.alpha[n];
    if (al != 0.f) {                    // alpha 0: the sample's field is never read (it may be uninitialised)
      if (P.planar) {                   // one 2-component field over (OH, OW) for all slices
        const float* f = Q.field + (size_t)n * 2 * ohw + (size_t)(r % ohw);
        gh += (double)al * (double)f[0]; gw += (double)al * (double)f[ohw];
      } else {                          // the field element has the output voxel's own index: coalesced like the store
        const float* f = Q.field + (size_t)n * 3 * ovol + (size_t)r;
        gd += (double)al * (double)f[0]; gh += (double)al * (double)f[ovol]; gw += (double)al * (double)f[2 * ovol];
      }
    }
    const double xd = P.planar ? (double)od : (double)M[0] * gd + (double)M[1] * gh + (double)M[2] * gw + (double)M[9];
    const double xh = (P.planar ? 0.0 : (double)M[3] * gd) + (double)M[4] * gh + (double)M[5] * gw + (double)M[10];
    const double xw = (P.planar ? 0.0 : (double)M[6] * gd) + (double)M[7] * gh + (double)M[8] * gw + (double)M[11];
    mt_sample_point(P, n, r, od, xd, xh, xw);      // range-checks the coordinate in double; NaN and infinities give cval
  }
}

extern "C" int mt_warp_sample(const float* src, int N, int C, int D, int H, int W, float* dst, int OD, int OH, int OW,
                              const float* mats, const float* field, const float* alpha, int mode, float cval, int planar,
                              mt_stream_t stream) {
  MT_REQUIRE(!planar || OD == D, "warp_sample: planar sampling keeps the slice axis (OD == D)");
  MT_REQUIRE(src && dst && mats && field && alpha && N > 0 && C > 0 && D > 0 && H > 0 && W > 0 && OD > 0 && OH > 0 && OW > 0,
             "warp_sample: bad arguments");
  MT_REQUIRE(mode == 0 || mode == 1 || mode == 3 || mode == 11, "warp_sample: mode must be 0, 1, 3 or 11 (got %d)", mode);
  WarpParams Q;
  AffineParams& P = Q.A;
  P.src = src; P.dst = dst; P.mats = mats; P.N = N; P.C = C; P.D = D; P.H = H; P.W = W; P.OD = OD; P.OH = OH; P.OW = OW;
  P.mode = mode; P.cval = cval; P.planar = planar ? 1 : 0;
  Q.field = field; Q.alpha = alpha;
  const long total = (long)N * OD * OH * OW;
  int blocks = mt_cdiv(total, 256); if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(warp_sample_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, Q);
  MT_CHECK_LAUNCH("warp_sample");
  return MT_OK;
}
