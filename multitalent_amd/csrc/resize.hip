// resize.hip — the resize unit of the preprocessing front: resample_data_or_seg (preprocessing/preprocessing.py:109-197) at every
// order the reference's preprocessors use.  skimage.transform.resize(order, mode='edge', anti_aliasing=False) is
// scipy.ndimage.zoom(order, mode='nearest', grid_mode=True), the z pass is scipy.ndimage.map_coordinates(order_z, mode='nearest');
// resize_line.h holds the per-line arithmetic (closed-form edge rule, weights, taps) that these kernels share with a host program.
//   mt_resize_prefilter3   cubic B-spline prefilter along any subset of axes, src -> dst (in place allowed), no padded copy;
//   mt_resize              one order (0, 1, 3) per axis; an axis with in == out is addressed by its stride and copied, so a per-slice
//                          resize works for whichever axis is the anisotropic one without a permuted copy;
//   mt_resize_labels       the per-label order-1 rule of resize_segmentation on the axes that change;
//   mt_resize_labels_axis  the z pass of a label map (strictly above one half).
// All loop bounds come from the arguments.  HBM-bound: 4 B read per input element and 4 B written per output element, per pass.
#include "mt_common.h"
#include "resize_line.h"
#include <limits.h>

// ---- prefilter: one thread per line, both recursions in double, one rounding to float32 when the result is stored --------------------
struct RsPrefilterParams { const float* src; float* dst; long nlines; int len; long line_stride_outer, line_stride_inner; int inner; long elem_stride; };
#define MT_RS_CHUNK 32           // causal values a thread keeps in registers for the anticausal pass
#define MT_RS_WARM 40            // inputs in front of a chunk from which its causal values are rebuilt: |z|^40 = 1.3e-23
__global__ __launch_bounds__(256) void resize_prefilter_kernel(const RsPrefilterParams P) {
  const double z = MT_RS_POLE;
  const int n = P.len;
  for (long l = (long)blockIdx.x * 256 + threadIdx.x; l < P.nlines; l += (long)gridDim.x * 256) {
    const long off = (l / P.inner) * P.line_stride_outer + (l % P.inner) * P.line_stride_inner;
    const float* p = P.src + off;
    float* q = P.dst + off;
    const long es = P.elem_stride;
    if (n == 1) { q[0] = p[0]; continue; }
    const double c0 = mt_rs_causal_start((double)p[0]);              // c+[0] = c+[-1]
    const double x_last = (double)p[(long)(n - 1) * es];
    // As in spline_prefilter_kernel (prep.hip): the anticausal pass needs the causal values from the back and a line does not fit in
    // registers, so it goes chunk by chunk from the end; the causal values of a chunk are rebuilt from the inputs in front of it (from
    // c+[0] where the chunk starts within MT_RS_WARM elements of the start, else from MT_RS_WARM elements before it with c+ = 0 there).
    // Only elements of the chunk are written and every read of an input lies in the chunk or in front of it, so src == dst is allowed.
    double next = 0.0;
    for (int a = ((n - 1) / MT_RS_CHUNK) * MT_RS_CHUNK; a >= 0; a -= MT_RS_CHUNK) {
      const int len = n - a < MT_RS_CHUNK ? n - a : MT_RS_CHUNK;
      int j = a - MT_RS_WARM;
      double prev = 0.0;
      if (j <= 0) { prev = c0; j = 1; }
      for (int k = j; k < a; ++k) prev = 6.0 * (double)p[(long)k * es] + z * prev;
      double cp[MT_RS_CHUNK];
#pragma unroll
      for (int i = 0; i < MT_RS_CHUNK; ++i) {
        if (i < len) { prev = (a + i == 0) ? c0 : 6.0 * (double)p[(long)(a + i) * es] + z * prev; }
        cp[i] = prev;
      }
#pragma unroll
      for (int i = MT_RS_CHUNK - 1; i >= 0; --i) {
        if (i < len) {
          if (a + i == n - 1) next = mt_rs_anticausal_start(cp[i], x_last);
          else next = z * (next - cp[i]);
          q[(long)(a + i) * es] = (float)next;
        }
      }
    }
  }
}

static bool rs_count_ok(int NC, int D, int H, int W) { return (long)NC * D <= INT_MAX && (long)NC * D * H <= INT_MAX && (long)NC * D * H * W <= INT_MAX; }

extern "C" int mt_resize_prefilter3(const float* src, float* dst, int NC, int D, int H, int W, int axes, mt_stream_t stream) {
  MT_REQUIRE(src != nullptr && dst != nullptr, "resize_prefilter3: null pointers");
  MT_REQUIRE(NC > 0 && D > 0 && H > 0 && W > 0, "resize_prefilter3: a non-positive extent");
  MT_REQUIRE(axes > 0 && axes < 8, "resize_prefilter3: axes is a mask of bit 0 W, bit 1 H, bit 2 D");
  MT_REQUIRE(rs_count_ok(NC, D, H, W), "resize_prefilter3: more than INT32_MAX elements");
  hipStream_t st = (hipStream_t)stream;
  RsPrefilterParams P; P.src = src; P.dst = dst;
  const long HW = (long)H * W, V = (long)D * HW;
  bool first = true;                                   // the first pass reads src, the later ones run in place on dst
  for (int bit = 0; bit < 3; ++bit) {
    if (!(axes >> bit & 1)) continue;
    if (bit == 0) { P.nlines = (long)NC * D * H; P.len = W; P.inner = 1; P.line_stride_outer = W; P.line_stride_inner = 0; P.elem_stride = 1; }
    else if (bit == 1) { P.nlines = (long)NC * D * W; P.len = H; P.inner = W; P.line_stride_outer = HW; P.line_stride_inner = 1; P.elem_stride = W; }
    else { P.nlines = (long)NC * HW; P.len = D; P.inner = (int)HW; P.line_stride_outer = V; P.line_stride_inner = 1; P.elem_stride = HW; }
    P.src = first ? src : dst;
    hipLaunchKernelGGL(resize_prefilter_kernel, dim3((unsigned)mt_cdiv(P.nlines, 256)), dim3(256), 0, st, P);
    first = false;
  }
  MT_CHECK_LAUNCH("resize_prefilter3");
  return MT_OK;
}

// ---- sampler: one output voxel per thread; up to 4 x 4 x 4 taps, fewer where an axis is order 0 / 1 or unchanged ----------------------
struct RsParams {
  const float* src; float* dst;
  int NC, D, H, W, OD, OH, OW;
  int ord[3];              // per axis D, H, W
  int nt[3];               // taps per axis (mt_rs_ntaps): uniform over the launch
  int strict;              // label kernels
};
__global__ __launch_bounds__(256) void resize_kernel(const RsParams P) {
  const unsigned total = (unsigned)P.NC * P.OD * P.OH * P.OW;
  const int nd = P.nt[0], nh = P.nt[1], nw = P.nt[2];
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    unsigned r = i;
    const int ow = (int)(r % P.OW); r /= P.OW;
    const int oh = (int)(r % P.OH); r /= P.OH;
    const int od = (int)(r % P.OD);
    const unsigned nc = r / P.OD;
    int id[4], ih[4], iw[4];
    double wd[4], wh[4], ww[4];
    mt_rs_taps(P.ord[0], od, P.D, P.OD, id, wd);
    mt_rs_taps(P.ord[1], oh, P.H, P.OH, ih, wh);
    mt_rs_taps(P.ord[2], ow, P.W, P.OW, iw, ww);
    const float* vol = P.src + (size_t)nc * P.D * P.H * P.W;
    double acc = 0.0;
    // fixed trip counts with uniform guards: the tap arrays stay in registers
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (a >= nd) break;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (b >= nh) break;
        const float* row = vol + ((size_t)id[a] * P.H + ih[b]) * P.W;
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < nw) s += ww[c] * (double)row[iw[c]];
        acc += wd[a] * wh[b] * s;
      }
    }
    P.dst[i] = (float)acc;
  }
}

__global__ __launch_bounds__(256) void resize_labels_kernel(const RsParams P) {
  const unsigned total = (unsigned)P.NC * P.OD * P.OH * P.OW;
  const int nd = P.nt[0], nh = P.nt[1], nw = P.nt[2];
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    unsigned r = i;
    const int ow = (int)(r % P.OW); r /= P.OW;
    const int oh = (int)(r % P.OH); r /= P.OH;
    const int od = (int)(r % P.OD);
    const unsigned nc = r / P.OD;
    int id[4], ih[4], iw[4];
    double wd[4], wh[4], ww[4];
    mt_rs_taps(1, od, P.D, P.OD, id, wd);
    mt_rs_taps(1, oh, P.H, P.OH, ih, wh);
    mt_rs_taps(1, ow, P.W, P.OW, iw, ww);
    const float* vol = P.src + (size_t)nc * P.D * P.H * P.W;
    float lab[8]; double w[8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const bool on = a < nd && b < nh && c < nw;          // uniform over the launch
          const int k = (a * 2 + b) * 2 + c;
          lab[k] = on ? vol[((size_t)id[a < nd ? a : 0] * P.H + ih[b < nh ? b : 0]) * P.W + iw[c < nw ? c : 0]] : 0.f;
          w[k] = on ? wd[a] * wh[b] * ww[c] : -1.0;            // an unused slot: the sums below skip it
        }
    P.dst[i] = mt_rs_label_vote(lab, w, 8, P.strict);
  }
}

static int rs_fill(RsParams& P, const char* who, const float* src, int NC, int D, int H, int W, float* dst, int OD, int OH, int OW,
                   int ordD, int ordH, int ordW) {
  MT_REQUIRE(src != nullptr && dst != nullptr, "%s: null pointers", who);
  MT_REQUIRE(NC > 0 && D > 0 && H > 0 && W > 0 && OD > 0 && OH > 0 && OW > 0, "%s: a non-positive extent", who);
  MT_REQUIRE((ordD == 0 || ordD == 1 || ordD == 3) && (ordH == 0 || ordH == 1 || ordH == 3) && (ordW == 0 || ordW == 1 || ordW == 3),
             "%s: orders are 0, 1 or 3, got (%d, %d, %d)", who, ordD, ordH, ordW);
  MT_REQUIRE(rs_count_ok(NC, D, H, W) && rs_count_ok(NC, OD, OH, OW), "%s: more than INT32_MAX input or output elements", who);
  P.src = src; P.dst = dst; P.NC = NC; P.D = D; P.H = H; P.W = W; P.OD = OD; P.OH = OH; P.OW = OW;
  P.ord[0] = ordD; P.ord[1] = ordH; P.ord[2] = ordW;
  P.nt[0] = mt_rs_ntaps(ordD, D, OD); P.nt[1] = mt_rs_ntaps(ordH, H, OH); P.nt[2] = mt_rs_ntaps(ordW, W, OW);
  P.strict = 0;
  return MT_OK;
}
static unsigned rs_blocks(const RsParams& P) {
  const long total = (long)P.NC * P.OD * P.OH * P.OW;
  const long b = (total + 255) / 256;
  return (unsigned)(b > 65536 ? 65536 : b);
}

extern "C" int mt_resize(const float* src, int NC, int D, int H, int W, float* dst, int OD, int OH, int OW, int order_d, int order_h,
                         int order_w, mt_stream_t stream) {
  RsParams P;
  const int rc = rs_fill(P, "resize", src, NC, D, H, W, dst, OD, OH, OW, order_d, order_h, order_w);
  if (rc != MT_OK) return rc;
  hipLaunchKernelGGL(resize_kernel, dim3(rs_blocks(P)), dim3(256), 0, (hipStream_t)stream, P);
  MT_CHECK_LAUNCH("resize");
  return MT_OK;
}

extern "C" int mt_resize_labels(const float* src, int NC, int D, int H, int W, float* dst, int OD, int OH, int OW, mt_stream_t stream) {
  RsParams P;
  const int rc = rs_fill(P, "resize_labels", src, NC, D, H, W, dst, OD, OH, OW, 1, 1, 1);
  if (rc != MT_OK) return rc;
  hipLaunchKernelGGL(resize_labels_kernel, dim3(rs_blocks(P)), dim3(256), 0, (hipStream_t)stream, P);
  MT_CHECK_LAUNCH("resize_labels");
  return MT_OK;
}

extern "C" int mt_resize_labels_axis(const float* src, int NC, int D, int H, int W, int axis, int out_n, float* dst, mt_stream_t stream) {
  MT_REQUIRE(axis >= 0 && axis <= 2, "resize_labels_axis: axis is 0 (D), 1 (H) or 2 (W), got %d", axis);
  RsParams P;
  const int rc = rs_fill(P, "resize_labels_axis", src, NC, D, H, W, dst, axis == 0 ? out_n : D, axis == 1 ? out_n : H, axis == 2 ? out_n : W, 1, 1, 1);
  if (rc != MT_OK) return rc;
  P.strict = 1;
  hipLaunchKernelGGL(resize_labels_kernel, dim3(rs_blocks(P)), dim3(256), 0, (hipStream_t)stream, P);
  MT_CHECK_LAUNCH("resize_labels_axis");
  return MT_OK;
}
