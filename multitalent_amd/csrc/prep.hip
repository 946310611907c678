// prep.hip — device-side target preparation: the deep-supervision label pyramid.
//
// Replaces: DownsampleSegForDSTransform2 / downsample_seg_for_ds_transform2 (downsampling.py:70-104, order 0) and
// RemoveLabelTransform(-1, 0) (data_augmentation_moreDA.py:117), which the reference runs in CPU augmentation workers.
// resize_segmentation(order 0) is batchgenerators -> skimage.transform.resize(order=0, mode="edge", anti_aliasing=False),
// which delegates to scipy.ndimage.zoom(order=0, grid_mode=True): output voxel o samples input coordinate
// (o + 0.5) * in/out - 0.5 and order 0 takes floor(coord + 0.5) = floor((o + 0.5) * in/out), clamped to the volume.
// HBM-bound: every level reads |out| scattered labels and writes |out| floats.
#include "mt_common.h"
#include "sample_common.h"

struct DsParams {
  const float* src; float* dst;
  int NC, Di, Hi, Wi, Do, Ho, Wo;
  double fd, fh, fw;       // in/out per axis
  int remove_minus_one;
};
__global__ __launch_bounds__(256) void downsample_seg_kernel(const DsParams P) {
  const long total = (long)P.NC * P.Do * P.Ho * P.Wo;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    long r = i;
    const int ow = (int)(r % P.Wo); r /= P.Wo;
    const int oh = (int)(r % P.Ho); r /= P.Ho;
    const int od = (int)(r % P.Do);
    const long nc = r / P.Do;
    int sd = (int)floor((od + 0.5) * P.fd), sh = (int)floor((oh + 0.5) * P.fh), sw = (int)floor((ow + 0.5) * P.fw);
    sd = sd < 0 ? 0 : (sd >= P.Di ? P.Di - 1 : sd);
    sh = sh < 0 ? 0 : (sh >= P.Hi ? P.Hi - 1 : sh);
    sw = sw < 0 ? 0 : (sw >= P.Wi ? P.Wi - 1 : sw);
    float v = P.src[((size_t)((size_t)nc * P.Di + sd) * P.Hi + sh) * P.Wi + sw];
    if (P.remove_minus_one && v == -1.f) v = 0.f;
    P.dst[i] = v;
  }
}

extern "C" int mt_downsample_seg_nearest(const float* src, int NC, int Di, int Hi, int Wi, float* dst, int Do, int Ho, int Wo,
                                         int remove_minus_one, mt_stream_t stream) {
  MT_REQUIRE(src != nullptr && dst != nullptr, "downsample_seg: null pointers");
  MT_REQUIRE(NC > 0 && Di > 0 && Hi > 0 && Wi > 0 && Do > 0 && Ho > 0 && Wo > 0, "downsample_seg: empty problem");
  DsParams P;
  P.src = src; P.dst = dst; P.NC = NC; P.Di = Di; P.Hi = Hi; P.Wi = Wi; P.Do = Do; P.Ho = Ho; P.Wo = Wo;
  P.fd = (double)Di / Do; P.fh = (double)Hi / Ho; P.fw = (double)Wi / Wo;
  P.remove_minus_one = remove_minus_one;
  const long total = (long)NC * Do * Ho * Wo;
  int blocks = mt_cdiv(total, 256); if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(downsample_seg_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P);
  MT_CHECK_LAUNCH("downsample_seg");
  return MT_OK;
}

// ================================================================================================
// Spatial augmentation on the device (second half): batchgenerators' SpatialTransform as nnU-Net configures it
// (data_augmentation_moreDA.py:66-80: rotation + scaling, no elastic deformation, order_data 3 / order_seg 1, constant borders)
// is, per sample, scipy.ndimage.map_coordinates over an AFFINE coordinate field x = M (o - (O-1)/2) + centre.  Two kernels:
//  * mt_spline_prefilter3: the cubic B-spline prefilter map_coordinates(order=3) applies first — per axis the recursive filter with
//    pole z = sqrt(3) - 2, gain 6 and scipy's exact mirror boundary initialisation (mode 'constant' filters with mirror
//    boundaries); one thread per line, double-precision recursion, in place, three passes (W, H, D);
//  * mt_affine_sample: output voxel -> coordinate -> 64-tap cubic B-spline (order 3), 8-tap linear (order 1), nearest (order 0) or
//    the per-label rule batchgenerators uses for segmentations with order 1 (label c wins where the order-1 interpolation of the
//    indicator (seg == c) is >= 0.5, later = larger labels override).  scipy's 'constant' mode: a coordinate outside [0, n-1]
//    on any axis yields cval; inside, stencil taps that fall off the array read the MIRRORED coefficient.
struct PrefilterParams { float* vol; long nlines; int len; long line_stride_outer, line_stride_inner; int inner; long elem_stride; };
// line index l -> base offset: (l / inner) * line_stride_outer + (l % inner) * line_stride_inner; elements at + k * elem_stride
#define MT_PF_CHUNK 32           // causal values a thread keeps in registers for the anticausal pass
#define MT_PF_WARM 40            // inputs in front of a chunk from which its causal values are rebuilt: |z|^40 = 1.3e-23
__global__ __launch_bounds__(256) void spline_prefilter_kernel(const PrefilterParams P) {
  const double z = -0.26794919243112270647;       // sqrt(3) - 2
  const int n = P.len;
  for (long l = (long)blockIdx.x * 256 + threadIdx.x; l < P.nlines; l += (long)gridDim.x * 256) {
    float* p = P.vol + (l / P.inner) * P.line_stride_outer + (l % P.inner) * P.line_stride_inner;
    const long es = P.elem_stride;
    if (n == 1) continue;
    // causal initialisation, exact for mirror boundaries: sum_{k=0}^{2n-3} z^k s_mirror[k] / (1 - z^(2n-2)), gain 6 folded in
    const double zn = pow(z, (double)(n - 1));
    double sum = 6.0 * ((double)p[0] + zn * (double)p[(long)(n - 1) * es]);
    double z1 = z, z2 = zn * zn / z;
    for (int k = 1; k < n - 1; ++k) { sum += 6.0 * (z1 + z2) * (double)p[(long)k * es]; z1 *= z; z2 /= z; }
    const double c0 = sum / (1.0 - zn * zn);
    // Both recursions run in double and the line is rounded to float32 ONCE, when the result is stored (float storage between the
    // passes over the axes only).  The anticausal pass needs the causal values c+[k] = 6 s[k] + z c+[k-1] from the back, and a line
    // does not fit in registers, so it goes chunk by chunk from the end: the causal values of a chunk are recomputed from the inputs
    // in front of it — from c+[0] where the chunk starts within MT_PF_WARM elements of the line's start, else from MT_PF_WARM elements
    // before it with c+ = 0 there (what that drops is below |z|^40 = 1.3e-23 of the line) — and kept in registers while the
    // anticausal pass  c[n-1] = z/(z^2-1) (z c+[n-2] + c+[n-1]);  c[k] = z (c[k+1] - c+[k])  overwrites the chunk.  Only elements of
    // the chunk are written, and every read of an input lies in front of a chunk not yet written.
    const double g = z / (z * z - 1.0);
    double next = 0.0;
    for (int a = ((n - 1) / MT_PF_CHUNK) * MT_PF_CHUNK; a >= 0; a -= MT_PF_CHUNK) {
      const int len = n - a < MT_PF_CHUNK ? n - a : MT_PF_CHUNK;
      int j = a - MT_PF_WARM;
      double prev = 0.0;
      if (j <= 0) { prev = c0; j = 1; }
      for (int k = j; k < a; ++k) prev = 6.0 * (double)p[(long)k * es] + z * prev;
      const double before = prev;                   // c+[a-1] (a > 0)
      double cp[MT_PF_CHUNK];
#pragma unroll
      for (int i = 0; i < MT_PF_CHUNK; ++i) {
        if (i < len) { prev = (a + i == 0) ? c0 : 6.0 * (double)p[(long)(a + i) * es] + z * prev; }
        cp[i] = prev;
      }
#pragma unroll
      for (int i = MT_PF_CHUNK - 1; i >= 0; --i) {
        if (i < len) {
          if (a + i == n - 1) next = g * (z * (i > 0 ? cp[i > 0 ? i - 1 : 0] : before) + cp[i]);
          else next = z * (next - cp[i]);
          p[(long)(a + i) * es] = (float)next;
        }
      }
    }
  }
}
extern "C" int mt_spline_prefilter3(float* vol, int NC, int D, int H, int W, int axes, mt_stream_t stream) {
  MT_REQUIRE(vol != nullptr && NC > 0 && D > 0 && H > 0 && W > 0 && axes > 0 && axes < 8, "spline_prefilter3: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  PrefilterParams P; P.vol = vol;
  const long HW = (long)H * W, V = (long)D * HW;
  // along W: lines (nc, d, h)
  P.nlines = (long)NC * D * H; P.len = W; P.inner = 1; P.line_stride_outer = W; P.line_stride_inner = 0; P.elem_stride = 1;
  if (axes & 1) hipLaunchKernelGGL(spline_prefilter_kernel, dim3((unsigned)mt_cdiv(P.nlines, 256)), dim3(256), 0, st, P);
  // along H: lines (nc*d, w)
  P.nlines = (long)NC * D * W; P.len = H; P.inner = W; P.line_stride_outer = HW; P.line_stride_inner = 1; P.elem_stride = W;
  if (axes & 2) hipLaunchKernelGGL(spline_prefilter_kernel, dim3((unsigned)mt_cdiv(P.nlines, 256)), dim3(256), 0, st, P);
  // along D: lines (nc, h*w)
  P.nlines = (long)NC * HW; P.len = D; P.inner = (int)HW; P.line_stride_outer = V; P.line_stride_inner = 1; P.elem_stride = HW;
  if (axes & 4) hipLaunchKernelGGL(spline_prefilter_kernel, dim3((unsigned)mt_cdiv(P.nlines, 256)), dim3(256), 0, st, P);
  MT_CHECK_LAUNCH("spline_prefilter3");
  return MT_OK;
}

// AffineParams, the mirror rule and the per-coordinate sampler live in sample_common.h (shared with warp.hip's mt_warp_sample).
__global__ __launch_bounds__(256) void affine_sample_kernel(const AffineParams P) {
  const long ovol = (long)P.OD * P.OH * P.OW, total = (long)P.N * ovol;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int n = (int)(i / ovol);
    long r = i % ovol;
    const int ow = (int)(r % P.OW), oh = (int)((r / P.OW) % P.OH), od = (int)(r / ((long)P.OW * P.OH));
    const float* M = P.mats + n * 12;
    const double gd = od - 0.5 * (P.OD - 1), gh = oh - 0.5 * (P.OH - 1), gw = ow - 0.5 * (P.OW - 1);
    const double xd = P.planar ? (double)od : (double)M[0] * gd + (double)M[1] * gh + (double)M[2] * gw + (double)M[9];
    const double xh = (P.planar ? 0.0 : (double)M[3] * gd) + (double)M[4] * gh + (double)M[5] * gw + (double)M[10];
    const double xw = (P.planar ? 0.0 : (double)M[6] * gd) + (double)M[7] * gh + (double)M[8] * gw + (double)M[11];
    mt_sample_point(P, n, r, od, xd, xh, xw);
  }
}
extern "C" int mt_affine_sample(const float* src, int N, int C, int D, int H, int W, float* dst, int OD, int OH, int OW,
                                const float* mats, int mode, float cval, int planar, mt_stream_t stream) {
  MT_REQUIRE(!planar || OD == D, "affine_sample: planar sampling keeps the slice axis (OD == D)");
  MT_REQUIRE(src && dst && mats && N > 0 && C > 0 && D > 0 && H > 0 && W > 0 && OD > 0 && OH > 0 && OW > 0, "affine_sample: bad arguments");
  MT_REQUIRE(mode == 0 || mode == 1 || mode == 3 || mode == 11, "affine_sample: mode must be 0, 1, 3 or 11 (got %d)", mode);
  AffineParams P;
  P.src = src; P.dst = dst; P.mats = mats; P.N = N; P.C = C; P.D = D; P.H = H; P.W = W; P.OD = OD; P.OH = OH; P.OW = OW;
  P.mode = mode; P.cval = cval; P.planar = planar ? 1 : 0;
  const long total = (long)N * OD * OH * OW;
  int blocks = mt_cdiv(total, 256); if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(affine_sample_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P);
  MT_CHECK_LAUNCH("affine_sample");
  return MT_OK;
}

// ================================================================================================
// GaussianBlurTransform of nnU-Net's moreDA chain (data_augmentation_moreDA.py:87-88; batchgenerators' augment_gaussian_blur =
// scipy.ndimage.gaussian_filter(channel, sigma, order=0) per chosen channel): separable, per axis a correlation with
// w[k] = exp(-k^2 / (2 sigma^2)) / sum, k = -r..r, r = int(4 sigma + 0.5) (truncate = 4) and scipy's default 'reflect' boundary
// (half-sample symmetric: d c b a | a b c d | d c b a).  One launch per axis; sigma per (sample, channel) — sigma <= 0 copies the
// channel (the transform blurs only some channels of some samples).  HBM-bound: one read (the 2r+1 taps of neighbouring threads
// overlap in L1/L2) and one write per element and pass.  The radius is never clamped (a clamped radius is a different filter): sigma
// lives on the device, so a channel whose sigma needs a radius above MT_BLUR_MAXR (sigma >= 8.125) or is NaN cannot be refused on the
// host — every element of that channel is written as NaN instead.
struct BlurParams { const float* src; float* dst; const float* sigma; int NC, D, H, W, axis; };
#define MT_BLUR_MAXR 32
__global__ __launch_bounds__(256) void gaussian_blur_axis_kernel(const BlurParams P) {
  __shared__ float wsh[2 * MT_BLUR_MAXR + 1];
  const int nc = blockIdx.y;
  const float sg = P.sigma[nc];
  const long V = (long)P.D * P.H * P.W;
  const float* src = P.src + (size_t)nc * V;
  float* dst = P.dst + (size_t)nc * V;
  int r = 0;
  // written so that a NaN sigma is refused as well: it fails both comparisons
  const bool refused = !(sg <= 0.f) && !(4.0 * (double)sg + 0.5 < (double)(MT_BLUR_MAXR + 1));
  if (sg > 0.f && !refused) {
    r = (int)(4.0 * (double)sg + 0.5);
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int k = -r; k <= r; ++k) s += exp(-0.5 * (double)k * k / ((double)sg * sg));
      for (int k = -r; k <= r; ++k) wsh[k + r] = (float)(exp(-0.5 * (double)k * k / ((double)sg * sg)) / s);
    }
  }
  __syncthreads();
  const int len = P.axis == 0 ? P.D : (P.axis == 1 ? P.H : P.W);
  const long stride = P.axis == 0 ? (long)P.H * P.W : (P.axis == 1 ? P.W : 1);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long)gridDim.x * 256) {
    if (sg <= 0.f) { dst[i] = src[i]; continue; }
    if (refused) { dst[i] = __builtin_nanf(""); continue; }
    const int pos = (int)((i / stride) % len);
    const long base = i - (long)pos * stride;
    double acc = 0.0;                                     // scipy's correlate1d accumulates in double
    for (int k = -r; k <= r; ++k) {
      int q = pos + k;
      // 'reflect': period 2 len, q -> q mod 2 len, mirrored in the upper half
      if (q < 0 || q >= len) {
        const int p2 = 2 * len;
        q %= p2; if (q < 0) q += p2;
        if (q >= len) q = p2 - 1 - q;
      }
      acc += (double)wsh[k + r] * (double)src[base + (long)q * stride];
    }
    dst[i] = (float)acc;
  }
}

extern "C" int mt_gaussian_blur_axis(const float* src, float* dst, int NC, int D, int H, int W, int axis, const float* sigma, mt_stream_t stream) {
  MT_REQUIRE(src != nullptr && dst != nullptr && sigma != nullptr && src != dst, "gaussian_blur_axis: null or aliased pointers");
  MT_REQUIRE(NC > 0 && NC <= 65535 && D > 0 && H > 0 && W > 0 && axis >= 0 && axis <= 2, "gaussian_blur_axis: bad geometry");
  BlurParams P;
  P.src = src; P.dst = dst; P.sigma = sigma; P.NC = NC; P.D = D; P.H = H; P.W = W; P.axis = axis;
  const long V = (long)D * H * W;
  int blocks = mt_cdiv(V, 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(gaussian_blur_axis_kernel, dim3(blocks, NC), dim3(256), 0, (hipStream_t)stream, P);
  MT_CHECK_LAUNCH("gaussian_blur_axis");
  return MT_OK;
}
