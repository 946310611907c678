// Training batches from device-resident cases (training/dataloading/device_loading.py; reference dataset_loading.py:224-380).
//   mt_patch_gather   the crop + np.pad of generate_train_batch (:338-372) for up to MT_PATCH_MAX_SRC samples in one launch: every
//                     sample has its own source (a whole case, or a staged sub-box), patch corner and shape, handed over in the
//                     kernel arguments;
//   mt_seg_narrow     the label channel of a case as int16 (its storage on the device), with a check that nothing was lost.
// Both stream (HBM-bound): the gather reads (4C + 2) bytes and writes 4(C + 1) bytes per patch voxel, the narrowing reads 4 and
// writes 2 per voxel.  No LDS, no atomics; a copy, so the results are bit-identical from run to run.
#include "stream_common.h"
#include "patch_index.h"

#define LD_THREADS 256

struct GatherParams {
  mt_patch_src_t src[MT_PATCH_MAX_SRC];
  int C, PH, PW, QW, pad_mode;
  long nquad;                // quads of one sample and channel: PD * PH * QW
  float seg_fill;
  float* data_out; float* seg_out;
};

// grid (blocks, n): blockIdx.y is the sample, so its descriptor is wave-uniform.  A thread owns 4 consecutive w of one patch row, for
// all channels and the label map.  The 4 source voxels are one dword-aligned 16-byte load when the run lies inside the source (lb
// makes its alignment arbitrary), single loads under the pad rule at the borders; label voxels are 2-byte loads.  A full quad is one
// 16-byte store (16-byte aligned when PW % 4 == 0 and the output is), the tail of a row single stores.
__global__ __launch_bounds__(LD_THREADS) void patch_gather_kernel(const GatherParams P) {
  const mt_patch_src_t& S = P.src[blockIdx.y];
  const long V = (long)S.shape[0] * S.shape[1] * S.shape[2];
  const size_t PV = (size_t)(P.nquad / P.QW) * P.PW;
  float* __restrict__ dout = P.data_out + (size_t)blockIdx.y * P.C * PV;
  float* __restrict__ sout = P.seg_out + (size_t)blockIdx.y * PV;
  for (long q = (long)blockIdx.x * LD_THREADS + threadIdx.x; q < P.nquad; q += (long)gridDim.x * LD_THREADS) {
    const int row = (int)(q / P.QW), w0 = 4 * (int)(q - (long)row * P.QW);
    const int d = row / P.PH, h = row - d * P.PH;
    const int nw = P.PW - w0 < 4 ? P.PW - w0 : 4;
    const size_t o = (size_t)row * P.PW + w0;
    const int z0 = S.lb[2] + w0;
    const bool run_inside = z0 >= 0 && z0 + 3 < S.shape[2];
    float v[4];
    // image channels
    const long s0 = mt_patch_source(S.shape, S.lb, d, h, w0, P.pad_mode);
    for (int c = 0; c < P.C; ++c) {
      const float* __restrict__ x = S.data + (size_t)c * V;
      if (run_inside && s0 >= 0) {
        const mt_f4 a = *(const mt_f4*)(x + s0);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const long s = k < nw ? mt_patch_source(S.shape, S.lb, d, h, w0 + k, P.pad_mode) : MT_PATCH_FILL;
          v[k] = s >= 0 ? x[s] : 0.f;
        }
      }
      float* __restrict__ y = dout + (size_t)c * PV + o;
      if (nw == 4) { mt_f4 a; a.x = v[0]; a.y = v[1]; a.z = v[2]; a.w = v[3]; *(mt_f4*)y = a; }
      else for (int k = 0; k < nw; ++k) y[k] = v[k];
    }
    // label map: seg_fill outside the source in either pad mode
    const long t0 = mt_patch_source(S.shape, S.lb, d, h, w0, MT_PAD_CONSTANT);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long s = (run_inside && t0 >= 0) ? t0 + k : k < nw ? mt_patch_source(S.shape, S.lb, d, h, w0 + k, MT_PAD_CONSTANT) : MT_PATCH_FILL;
      v[k] = s >= 0 ? (float)S.seg[s] : P.seg_fill;
    }
    float* __restrict__ y = sout + o;
    if (nw == 4) { mt_f4 a; a.x = v[0]; a.y = v[1]; a.z = v[2]; a.w = v[3]; *(mt_f4*)y = a; }
    else for (int k = 0; k < nw; ++k) y[k] = v[k];
  }
}

extern "C" int mt_patch_gather(const mt_patch_src_t* srcs, int n, int C, int PD, int PH, int PW, int pad_mode, float seg_fill,
                               float* data_out, float* seg_out, mt_stream_t stream) {
  MT_REQUIRE(srcs && data_out && seg_out, "patch_gather: null pointer");
  MT_REQUIRE(n >= 1 && n <= MT_PATCH_MAX_SRC, "patch_gather: %d samples in one call (1..%d)", n, MT_PATCH_MAX_SRC);
  MT_REQUIRE(C >= 1 && PD >= 1 && PH >= 1 && PW >= 1, "patch_gather: bad shape %d x %d x %d x %d", C, PD, PH, PW);
  MT_REQUIRE((long)PD * PH * PW <= (long)INT32_MAX, "patch_gather: a patch of %d x %d x %d exceeds the int32 index range", PD, PH, PW);
  MT_REQUIRE(pad_mode == MT_PAD_CONSTANT || pad_mode == MT_PAD_EDGE, "patch_gather: pad mode %d", pad_mode);
  MT_REQUIRE(((uintptr_t)data_out & 3) == 0 && ((uintptr_t)seg_out & 3) == 0, "patch_gather: misaligned output");
  GatherParams P;
  for (int j = 0; j < MT_PATCH_MAX_SRC; ++j) {
    const mt_patch_src_t& s = srcs[j < n ? j : 0];
    if (j < n) {
      MT_REQUIRE(s.data && s.seg && ((uintptr_t)s.data & 3) == 0 && ((uintptr_t)s.seg & 1) == 0, "patch_gather: source %d: null or misaligned pointer", j);
      for (int a = 0; a < 3; ++a)
        MT_REQUIRE(s.shape[a] >= 1 && s.lb[a] > -(1 << 30) && s.lb[a] < (1 << 30), "patch_gather: source %d: axis %d has %d voxels, corner %d",
                   j, a, s.shape[a], s.lb[a]);
    }
    P.src[j] = s;
  }
  P.C = C; P.PH = PH; P.PW = PW; P.QW = (PW + 3) / 4; P.pad_mode = pad_mode; P.nquad = (long)PD * PH * P.QW;
  P.seg_fill = seg_fill; P.data_out = data_out; P.seg_out = seg_out;
  const int blocks = mt_stream_blocks(P.nquad * n, LD_THREADS) / n;
  hipLaunchKernelGGL(patch_gather_kernel, dim3(blocks > 1 ? blocks : 1, n), dim3(LD_THREADS), 0, (hipStream_t)stream, P);
  MT_CHECK_LAUNCH("patch_gather");
  return MT_OK;
}

// ---- float32 labels -> int16 --------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ld_narrow1(float f, bool& bad) {
  if (!(f >= -32768.f && f <= 32767.f)) { bad = true; return 0u; }         // NaN fails both comparisons
  const int i = (int)f;
  if ((float)i != f) bad = true;
  return (uint32_t)i & 0xffffu;
}

__global__ __launch_bounds__(LD_THREADS) void seg_narrow_kernel(const float* __restrict__ seg, long V, int16_t* __restrict__ out,
                                                                int32_t* __restrict__ flag) {
  bool bad = false;
  const long nquad = V / 4;
  const long gtid = (long)blockIdx.x * LD_THREADS + threadIdx.x, gstride = (long)gridDim.x * LD_THREADS;
  for (long q = gtid; q < nquad; q += gstride) {
    const mt_f4 a = *(const mt_f4*)(seg + 4 * q);
    uint2 t;
    t.x = ld_narrow1(a.x, bad) | ld_narrow1(a.y, bad) << 16;
    t.y = ld_narrow1(a.z, bad) | ld_narrow1(a.w, bad) << 16;
    ((uint2*)out)[q] = t;
  }
  for (long v = 4 * nquad + gtid; v < V; v += gstride) out[v] = (int16_t)ld_narrow1(seg[v], bad);
  if (bad) *flag = 1;                      // every writer stores the same value
}

extern "C" int mt_seg_narrow(const float* seg, long V, int16_t* out, int32_t* flag, mt_stream_t stream) {
  MT_REQUIRE(seg && out && flag && V > 0, "seg_narrow: bad arguments");
  MT_REQUIRE(((uintptr_t)seg & 3) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)flag & 3) == 0, "seg_narrow: misaligned pointer");
  hipLaunchKernelGGL(seg_narrow_kernel, dim3(mt_stream_blocks((V + 3) / 4, LD_THREADS)), dim3(LD_THREADS), 0, (hipStream_t)stream, seg, V, out, flag);
  MT_CHECK_LAUNCH("seg_narrow");
  return MT_OK;
}
