// ensemble.hip — the ensemble merge of stored probabilities (inference/ensemble_predictions.py:25-53 merge_files,
// evaluation/model_selection/ensemble.py:26-40 merge).  The reference loads K float16 arrays [C, X, Y, Z], copies them with
// np.vstack, reduces with np.mean, takes the argmax (or paints the region thresholds) and inserts the result into the uncropped
// volume: four passes over K*C*V elements on the host.  Here it is one stream: every member element is read once, the label and
// (when asked for) the float16 mean are written once.
#include "stream_common.h"

// K member pointers travel by value in the kernel arguments: no device-side pointer table per call.
struct EnsembleParams {
  const _Float16* m[MT_ENSEMBLE_MAX_MEMBERS];
  const int32_t* order; uint8_t* out; _Float16* mean;
  long V, cs, ms;           // voxels of the box, channel strides of the members and of the mean (elements)
  long FH, FW;              // the uncropped volume's inner dims
  int K, C, H, W, use_regions;
  int bD, bH, bW;           // insertion offset
  int cD, cH, cW;           // voxels actually written per dim (clipped to the volume)
};

typedef _Float16 mt_h8 __attribute__((ext_vector_type(8)));
#define MT_ENS_VOX 8        // voxels per lane: 16 bytes of float16

// numpy's np.mean of float16 members: float32 sum in member order, one IEEE division, one RNE rounding to float16 (subnormals
// kept: the f16 denormal mode of the code object is on, and float32 denormals are not flushed either).  The label is decided on
// the rounded value widened back.  A NaN mean follows numpy: the argmax takes the first NaN channel, `> 0.5` never holds for it.
// A class_order entry above 255 is stored as its low byte on every store path (the packed `& 255`, the bytewise cast).
template <bool WIDE> __global__ __launch_bounds__(256) void ensemble_classify_kernel(const EnsembleParams P) {
  const long groups = (P.V + MT_ENS_VOX - 1) / MT_ENS_VOX;
  const float fk = (float)P.K;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
    const long v0 = g * MT_ENS_VOX;
    const int n = P.V - v0 < MT_ENS_VOX ? (int)(P.V - v0) : MT_ENS_VOX;
    const bool wide = WIDE && n == MT_ENS_VOX;          // the last, partial group of a channel goes element by element
    float best[MT_ENS_VOX];
    int lab[MT_ENS_VOX];
#pragma unroll
    for (int j = 0; j < MT_ENS_VOX; ++j) { best[j] = 0.f; lab[j] = 0; }
    for (int c = 0; c < P.C; ++c) {
      const size_t off = (size_t)c * P.cs + v0;
      float s[MT_ENS_VOX];
      if (wide) {
        const mt_h8 t = *(const mt_h8*)(P.m[0] + off);
#pragma unroll
        for (int j = 0; j < MT_ENS_VOX; ++j) s[j] = (float)t[j];
#pragma unroll 4
        for (int k = 1; k < P.K; ++k) {
          const mt_h8 u = *(const mt_h8*)(P.m[k] + off);
#pragma unroll
          for (int j = 0; j < MT_ENS_VOX; ++j) s[j] += (float)u[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < MT_ENS_VOX; ++j) s[j] = j < n ? (float)P.m[0][off + j] : 0.f;
        for (int k = 1; k < P.K; ++k) {
          const _Float16* p = P.m[k] + off;
#pragma unroll
          for (int j = 0; j < MT_ENS_VOX; ++j) if (j < n) s[j] += (float)p[j];
        }
      }
      mt_h8 h;
#pragma unroll
      for (int j = 0; j < MT_ENS_VOX; ++j) h[j] = (_Float16)(s[j] / fk);
      if (P.mean) {
        _Float16* q = P.mean + (size_t)c * P.ms + v0;
        if (wide) *(mt_h8*)q = h;
        else {
#pragma unroll
          for (int j = 0; j < MT_ENS_VOX; ++j) if (j < n) q[j] = h[j];
        }
      }
      if (P.use_regions) {
        const int oc = P.order[c];
#pragma unroll
        for (int j = 0; j < MT_ENS_VOX; ++j) if ((float)h[j] > 0.5f) lab[j] = oc;
      } else {
#pragma unroll
        for (int j = 0; j < MT_ENS_VOX; ++j) {
          const float m = (float)h[j];
          if (c == 0 || m > best[j] || (m != m && best[j] == best[j])) { best[j] = m; lab[j] = c; }     // np.argmax: the first NaN wins
        }
      }
    }
    // re-insertion: voxel v of the box = (d, h, w) -> out[bD + d][bH + h][bW + w], clipped to the volume
    const int w0 = (int)(v0 % P.W);
    const long r0 = v0 / P.W;
    if (w0 + n <= P.W) {                                // the group lies in one row
      const int hh = (int)(r0 % P.H), d = (int)(r0 / P.H);
      int nw = P.cW - w0 < n ? P.cW - w0 : n;
      if (d < P.cD && hh < P.cH && nw > 0) {
        uint8_t* o = P.out + ((size_t)(P.bD + d) * P.FH + (P.bH + hh)) * P.FW + (P.bW + w0);
        if (nw == MT_ENS_VOX && ((uintptr_t)o & 3) == 0) {           // eight labels as one 8-byte or two 4-byte stores
          uint2 t;
          t.x = (uint32_t)(lab[0] & 255) | (uint32_t)(lab[1] & 255) << 8 | (uint32_t)(lab[2] & 255) << 16 | (uint32_t)(lab[3] & 255) << 24;
          t.y = (uint32_t)(lab[4] & 255) | (uint32_t)(lab[5] & 255) << 8 | (uint32_t)(lab[6] & 255) << 16 | (uint32_t)(lab[7] & 255) << 24;
          if (((uintptr_t)o & 7) == 0) *(uint2*)o = t;
          else { ((uint32_t*)o)[0] = t.x; ((uint32_t*)o)[1] = t.y; }
        } else {
#pragma unroll
          for (int j = 0; j < MT_ENS_VOX; ++j) if (j < nw) o[j] = (uint8_t)lab[j];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < MT_ENS_VOX; ++j) {
        if (j < n) {
          const long v = v0 + j;
          const int w = (int)(v % P.W), hh = (int)((v / P.W) % P.H), d = (int)(v / ((long)P.W * P.H));
          if (d < P.cD && hh < P.cH && w < P.cW)
            P.out[((size_t)(P.bD + d) * P.FH + (P.bH + hh)) * P.FW + (P.bW + w)] = (uint8_t)lab[j];
        }
      }
    }
  }
}

extern "C" int mt_ensemble_classify(const void* const* members, int K, int C, int D, int H, int W, long chan_stride,
                                    const int32_t* class_order, int use_regions, uint8_t* out, long FD, long FH, long FW,
                                    int bD, int bH, int bW, void* mean, long mean_stride, mt_stream_t stream) {
  MT_REQUIRE(members && K >= 1 && K <= MT_ENSEMBLE_MAX_MEMBERS, "ensemble_classify: %d members (1 .. %d)", K, MT_ENSEMBLE_MAX_MEMBERS);
  MT_REQUIRE(C >= 1 && C <= 255, "ensemble_classify: %d channels (1 .. 255: the label is a uint8)", C);
  MT_REQUIRE(out && D > 0 && H > 0 && W > 0 && FD > 0 && FH > 0 && FW > 0, "ensemble_classify: bad sizes");
  MT_REQUIRE(!use_regions || class_order, "ensemble_classify: regions need class_order");
  const long V = (long)D * H * W;
  MT_REQUIRE(chan_stride >= V && (!mean || mean_stride >= V), "ensemble_classify: channel stride below the %ld voxels of the box", V);
  MT_REQUIRE(bD >= 0 && bH >= 0 && bW >= 0 && bD < FD && bH < FH && bW < FW, "ensemble_classify: insertion offset outside the volume");
  EnsembleParams P;
  bool wide = chan_stride % MT_ENS_VOX == 0 && (!mean || (mean_stride % MT_ENS_VOX == 0 && ((uintptr_t)mean & 15) == 0));
  for (int k = 0; k < MT_ENSEMBLE_MAX_MEMBERS; ++k) {
    P.m[k] = (const _Float16*)members[k < K ? k : 0];
    MT_REQUIRE(P.m[k] && ((uintptr_t)P.m[k] & 1) == 0, "ensemble_classify: member %d is NULL or not float16 aligned", k);
    wide = wide && ((uintptr_t)P.m[k] & 15) == 0;
  }
  MT_REQUIRE(!mean || ((uintptr_t)mean & 1) == 0, "ensemble_classify: mean is not float16 aligned");
  P.order = class_order; P.out = out; P.mean = (_Float16*)mean; P.V = V; P.cs = chan_stride; P.ms = mean ? mean_stride : 0;
  P.FH = FH; P.FW = FW; P.K = K; P.C = C; P.H = H; P.W = W; P.use_regions = use_regions ? 1 : 0; P.bD = bD; P.bH = bH; P.bW = bW;
  P.cD = (int)((bD + (long)D <= FD) ? D : FD - bD); P.cH = (int)((bH + (long)H <= FH) ? H : FH - bH);
  P.cW = (int)((bW + (long)W <= FW) ? W : FW - bW);
  const int blocks = mt_stream_blocks((V + MT_ENS_VOX - 1) / MT_ENS_VOX, 256);
  if (wide) hipLaunchKernelGGL(ensemble_classify_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P);
  else hipLaunchKernelGGL(ensemble_classify_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P);
  MT_CHECK_LAUNCH("ensemble_classify");
  return MT_OK;
}
