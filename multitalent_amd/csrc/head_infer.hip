// head_infer.hip — the fused inference heads: 1x1x1 segmentation head + nonlinearity + un-flip + accumulation in one kernel
// (mt_head_flip_accumulate: one mirror combination into a tile accumulator; mt_head_mirror_accumulate: all combinations of a tile
// straight into the volume aggregate).
#include "pw_common.h"
#include <type_traits>

// ------------------------------------------------------------------------------------------------
// Inference: segmentation head + nonlinearity + un-flip + accumulation in ONE kernel (neural_network.py:502-591 does
// pred = nonlin(net(flip(x))); result += flip^-1(pred) / num_results per mirror combination).  The 1x1x1 head is computed with the
// MFMA operand roles SWAPPED (weights as the row operand), so a lane owns a VOXEL and its registers are output channels: the
// channel-major accumulator acc[C][D][H][W] is then written with 32 consecutive voxels per channel row — 128-byte aligned runs —
// instead of 47-channel NDHWC rows of 188 bytes, and the logits never exist in HBM (the separate head wrote 2.7 GB per batch of
// eight tiles at 0.9 TB/s and flip_accumulate read them back).  The register contents of both operands are exactly those of
// pw_fast_kernel; only their order in the MFMA changes.
struct HeadAccParams {
  mt_pointwise_t c;
  int nchunks, nsb, sample, fD, fH, fW, nonlin, first;
  long V;
  float weight;
  float* acc;
};
// XS: storage type of the source (fp32, or 16-bit activations of the mixed mode: a lane's 8 channels are ONE 16-byte load)
template <int VEC, int XS = MT_F32>
__global__ __launch_bounds__(256) void head_flip_accumulate_kernel(const HeadAccParams P) {
  constexpr int XE = mt_ebytes<XS>();
  const mt_pointwise_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  const int sb = mt_xcd_remap(blockIdx.x, gridDim.x);
  const int nb = P.sample;
  const long m0 = (long)sb * 128 + wave * 32;
  const mt_src_t& S = c.src;
  const long bv = m0 + li;
  const bool vok = bv < P.V;
  const size_t in_sample = (size_t)P.V * S.cs;
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)S.ptr + (size_t)nb * in_sample * XE), 0, (int)(in_sample * XE), 0x00020000);
  const int aoff = vok ? (int)((bv * S.cs + 8 * lhalf) * XE) : (int)0x80000000;
  const bool aff = S.scale != nullptr;
  const float slope = S.slope;
  const bool lrelu_ok = (slope >= 0.f) && (slope <= 1.f);
  __shared__ __attribute__((aligned(16))) float ssc[PW_MAXC], ssh[PW_MAXC];
  if (aff) {
    for (int i = tid; i < P.nchunks * PW_CK; i += 256) {
      ssc[i] = i < S.C ? S.scale[(size_t)nb * S.C + i] : 0.f;
      ssh[i] = i < S.C ? S.shift[(size_t)nb * S.C + i] : 0.f;
    }
    __syncthreads();
  }
  auto load_a = [&](int ch, float (&x)[8]) {        // (16-bit: raw dwords in x[0..3], widened in finish_a — a conversion here would wait for the prefetch)
    const int o = aoff + ch * (PW_CK * XE);
    if constexpr (XS != MT_F32) {
      const uint4 t = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ra, o, 0, 0));
      x[0] = __builtin_bit_cast(float, t.x); x[1] = __builtin_bit_cast(float, t.y); x[2] = __builtin_bit_cast(float, t.z); x[3] = __builtin_bit_cast(float, t.w);
    } else if constexpr (VEC == 2) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float2 t = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(ra, o + g * 8, 0, 0));
        x[2 * g] = t.x; x[2 * g + 1] = t.y;
      }
    } else {
#pragma unroll
      for (int g = 0; g < 8; ++g) x[g] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, o + g * 4, 0, 0));
    }
  };
  auto finish_a = [&](int ch, float (&x)[8]) {
    const int cb = ch * PW_CK + 8 * lhalf;
    if constexpr (XS != MT_F32) {
      const unsigned r0 = __builtin_bit_cast(unsigned, x[0]), r1 = __builtin_bit_cast(unsigned, x[1]), r2 = __builtin_bit_cast(unsigned, x[2]), r3 = __builtin_bit_cast(unsigned, x[3]);
      x[0] = mt_lo16<XS>(r0); x[1] = mt_hi16<XS>(r0); x[2] = mt_lo16<XS>(r1); x[3] = mt_hi16<XS>(r1);
      x[4] = mt_lo16<XS>(r2); x[5] = mt_hi16<XS>(r2); x[6] = mt_lo16<XS>(r3); x[7] = mt_hi16<XS>(r3);
    }
    if (aff) {
      const f32x4 sc0 = *(const f32x4*)(ssc + cb), sc1 = *(const f32x4*)(ssc + cb + 4);
      const f32x4 sh0 = *(const f32x4*)(ssh + cb), sh1 = *(const f32x4*)(ssh + cb + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float t = fmaf(x[e], e < 4 ? sc0[e & 3] : sc1[e & 3], e < 4 ? sh0[e & 3] : sh1[e & 3]);
        x[e] = lrelu_ok ? fmaxf(t, t * slope) : mt_lrelu(t, slope);
      }
    }
    if (cb + 8 > c.Cin || !vok) {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = (vok && cb + e < c.Cin) ? x[e] : 0.f;
    }
  };
  f32x16 acc[2];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[n][j] = 0.f;
  const bool two = c.Cout > 32;                      // block-uniform
  float xa[8], xn[8];
  load_a(0, xa);
  for (int ch = 0; ch < P.nchunks; ++ch) {
    if (ch + 1 < P.nchunks) load_a(ch + 1, xn);
    finish_a(ch, xa);
    const float* wq = c.wpack + (size_t)ch * 512 + lane * 4;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      if (n == 1 && !two) break;
      const float* wn = wq + (size_t)n * P.nchunks * 512;
      const f32x4 b0 = *(const f32x4*)(wn), b1 = *(const f32x4*)(wn + 256);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0[e], xa[e], acc[n], 0, 0, 0);      // rows = channels
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1[e], xa[4 + e], acc[n], 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < (XS != MT_F32 ? 4 : 8); ++e) xa[e] = xn[e];
  }
  // ---- epilogue: this lane's voxel, channels n*32 + (j&3) + 8*(j>>2) + 4*lhalf
  if (c.bias != nullptr) {
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int cj = n * 32 + (j & 3) + 8 * (j >> 2) + 4 * lhalf;
        acc[n][j] += cj < c.Cout ? c.bias[cj] : 0.f;
      }
  }
  if (P.nonlin == 2) {                                // softmax over ALL channels of the voxel: own registers + the partner lane's
    float mx = -3.0e38f;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (n * 32 + (j & 3) + 8 * (j >> 2) + 4 * lhalf < c.Cout) mx = fmaxf(mx, acc[n][j]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float se = 0.f;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const bool cv = n * 32 + (j & 3) + 8 * (j >> 2) + 4 * lhalf < c.Cout;
        acc[n][j] = cv ? expf(acc[n][j] - mx) : 0.f;
        se += acc[n][j];
      }
    se += __shfl_xor(se, 32, 64);
    const float inv = 1.f / se;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[n][j] *= inv;
  } else if (P.nonlin == 1) {
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[n][j] = 1.f / (1.f + expf(-acc[n][j]));
  }
  if (!vok) return;
  const int w = (int)(bv % c.Wb), h = (int)((bv / c.Wb) % c.Hb), d = (int)(bv / ((long)c.Wb * c.Hb));
  const long dv = ((long)(P.fD ? c.Db - 1 - d : d) * c.Hb + (P.fH ? c.Hb - 1 - h : h)) * c.Wb + (P.fW ? c.Wb - 1 - w : w);
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    if (n == 1 && !two) break;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int cj = n * 32 + (j & 3) + 8 * (j >> 2) + 4 * lhalf;
      if (cj < c.Cout) {
        float* a = P.acc + (size_t)cj * P.V + dv;
        const float v = acc[n][j] * P.weight;
        *a = P.first ? v : *a + v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// All mirror combinations of a tile in ONE kernel, straight into the volume aggregate: for output voxel v of the tile
//   agg[c][tile + v] += gauss[v] * weight * sum_k nonlin(head(features_k[flip_k(v)]))_c ,   nb[tile + v] += gauss[v]
// (neural_network.py:531-586 result += flip^-1(pred) / num_results per combination, then :384-394 result *= gaussian and the
// overlap-add).  The sum over the samples k stays in registers, so the per-tile accumulator and its 2 x 333 MB read-modify-write
// per mirror combination (plus the separate tile_accumulate pass) disappear: 8 x 212 MB of features in, one update of the
// aggregate out.
struct HeadMirParams {
  mt_pointwise_t c;
  int nchunks, nsb, sample0, nsamples, nonlin;
  int flips[8];                 // bit 0: D, bit 1: H, bit 2: W
  long V;
  float weight;
  const float* gauss;           // [D][H][W] or NULL (= 1)
  float* agg; float* nb;        // agg[C][aX][aY][aZ], nb[aX][aY][aZ] (nb may be NULL)
  long aX, aY, aZ; int x0, y0, z0;
};
template <int VEC, int XS = MT_F32>
__global__ __launch_bounds__(256) void head_mirror_accumulate_kernel(const HeadMirParams P) {
  constexpr int XE = mt_ebytes<XS>();
  const mt_pointwise_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  const int sb = mt_xcd_remap(blockIdx.x, gridDim.x);
  const long bv = (long)sb * 128 + wave * 32 + li;
  const bool vok = bv < P.V;
  const int w = (int)(bv % c.Wb), h = (int)((bv / c.Wb) % c.Hb), d = (int)(bv / ((long)c.Wb * c.Hb));
  const mt_src_t& S = c.src;
  const size_t in_sample = (size_t)P.V * S.cs;
  const bool aff = S.scale != nullptr;
  const float slope = S.slope;
  const bool lrelu_ok = (slope >= 0.f) && (slope <= 1.f);
  const bool two = c.Cout > 32;                      // block-uniform
  __shared__ __attribute__((aligned(16))) float ssc[PW_MAXC], ssh[PW_MAXC];
  f32x16 sum[2];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int j = 0; j < 16; ++j) sum[n][j] = 0.f;
  float bias[2][16];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int cj = n * 32 + (j & 3) + 8 * (j >> 2) + 4 * lhalf;
      bias[n][j] = (c.bias != nullptr && cj < c.Cout) ? c.bias[cj] : 0.f;
    }

  for (int k = 0; k < P.nsamples; ++k) {
    const int nb_ = P.sample0 + k, f = P.flips[k];
    __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)S.ptr + (size_t)nb_ * in_sample * XE), 0, (int)(in_sample * XE), 0x00020000);
    const long sv = ((long)((f & 1) ? c.Db - 1 - d : d) * c.Hb + ((f & 2) ? c.Hb - 1 - h : h)) * c.Wb + ((f & 4) ? c.Wb - 1 - w : w);
    const int aoff = vok ? (int)((sv * S.cs + 8 * lhalf) * XE) : (int)0x80000000;
    if (aff) {
      __syncthreads();
      for (int i = tid; i < P.nchunks * PW_CK; i += 256) {
        ssc[i] = i < S.C ? S.scale[(size_t)nb_ * S.C + i] : 0.f;
        ssh[i] = i < S.C ? S.shift[(size_t)nb_ * S.C + i] : 0.f;
      }
      __syncthreads();
    }
    f32x16 acc[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[n][j] = bias[n][j];
    for (int ch = 0; ch < P.nchunks; ++ch) {
      float x[8];
      const int o = aoff + ch * (PW_CK * XE);
      if constexpr (XS != MT_F32) {
        const uint4 t = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ra, o, 0, 0));
        x[0] = mt_lo16<XS>(t.x); x[1] = mt_hi16<XS>(t.x); x[2] = mt_lo16<XS>(t.y); x[3] = mt_hi16<XS>(t.y);
        x[4] = mt_lo16<XS>(t.z); x[5] = mt_hi16<XS>(t.z); x[6] = mt_lo16<XS>(t.w); x[7] = mt_hi16<XS>(t.w);
      } else if constexpr (VEC == 2) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float2 t = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(ra, o + g * 8, 0, 0));
          x[2 * g] = t.x; x[2 * g + 1] = t.y;
        }
      } else {
#pragma unroll
        for (int g = 0; g < 8; ++g) x[g] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, o + g * 4, 0, 0));
      }
      const int cb = ch * PW_CK + 8 * lhalf;
      if (aff) {
        const f32x4 sc0 = *(const f32x4*)(ssc + cb), sc1 = *(const f32x4*)(ssc + cb + 4);
        const f32x4 sh0 = *(const f32x4*)(ssh + cb), sh1 = *(const f32x4*)(ssh + cb + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = fmaf(x[e], e < 4 ? sc0[e & 3] : sc1[e & 3], e < 4 ? sh0[e & 3] : sh1[e & 3]);
          x[e] = lrelu_ok ? fmaxf(t, t * slope) : mt_lrelu(t, slope);
        }
      }
      if (cb + 8 > c.Cin || !vok) {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = (vok && cb + e < c.Cin) ? x[e] : 0.f;
      }
      const float* wq = c.wpack + (size_t)ch * 512 + lane * 4;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        if (n == 1 && !two) break;
        const float* wn = wq + (size_t)n * P.nchunks * 512;
        const f32x4 b0 = *(const f32x4*)(wn), b1 = *(const f32x4*)(wn + 256);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0[e], x[e], acc[n], 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1[e], x[4 + e], acc[n], 0, 0, 0);
      }
    }
    if (P.nonlin == 2) {
      float mx = -3.0e38f;
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (n * 32 + (j & 3) + 8 * (j >> 2) + 4 * lhalf < c.Cout) mx = fmaxf(mx, acc[n][j]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      float se = 0.f;
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const bool cv = n * 32 + (j & 3) + 8 * (j >> 2) + 4 * lhalf < c.Cout;
          acc[n][j] = cv ? expf(acc[n][j] - mx) : 0.f;
          se += acc[n][j];
        }
      se += __shfl_xor(se, 32, 64);
      const float inv = 1.f / se;
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int j = 0; j < 16; ++j) sum[n][j] += acc[n][j] * inv;
    } else {
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int j = 0; j < 16; ++j) sum[n][j] += P.nonlin == 1 ? 1.f / (1.f + expf(-acc[n][j])) : acc[n][j];
    }
  }
  if (!vok) return;
  const float g = P.gauss ? P.gauss[bv] : 1.f;
  const float wg = P.weight * g;
  const size_t av = ((size_t)(P.x0 + d) * P.aY + (P.y0 + h)) * P.aZ + (P.z0 + w);
  const size_t AV = (size_t)P.aX * P.aY * P.aZ;
  if (P.nb != nullptr && lhalf == 0) P.nb[av] += g;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    if (n == 1 && !two) break;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int cj = n * 32 + (j & 3) + 8 * (j >> 2) + 4 * lhalf;
      if (cj < c.Cout) P.agg[(size_t)cj * AV + av] += sum[n][j] * wg;
    }
  }
}

// ---- entry points: one validation-and-fill and one instance pick for both kernels
// The instance both kernels run for a source — the ONE place that decides it (the launches and mt_head_infer_kernel_name read it):
// a 16-bit source is one 16-byte load per lane and chunk (<2, XS>; a raw 16-byte buffer load only needs dword alignment); an fp32
// source goes by 8-byte loads where channel stride and base allow them (<2, MT_F32>), else by dwords (<1, MT_F32>)
struct HeadInferPick { int vec, xs; };
static HeadInferPick head_infer_pick(int dtype, int cs, const void* base) {
  if (dtype != MT_F32) return {2, dtype};
  return {((cs % 2) == 0 && (((uintptr_t)base) & 7) == 0) ? 2 : 1, MT_F32};
}
// calls f(VEC, XS) with the pick as compile-time constants
template <class F>
static void head_infer_instance(const HeadInferPick k, F&& f) {
  if (k.xs == MT_F16) f(std::integral_constant<int, 2>(), std::integral_constant<int, MT_F16>());
  else if (k.xs == MT_BF16) f(std::integral_constant<int, 2>(), std::integral_constant<int, MT_BF16>());
  else if (k.vec == 2) f(std::integral_constant<int, 2>(), std::integral_constant<int, MT_F32>());
  else f(std::integral_constant<int, 1>(), std::integral_constant<int, MT_F32>());
}
// what both kernels need of the head alone (p non-null): everything mt_head_infer_kernel_name can see
static int head_infer_head_ok(const char* who, const mt_pointwise_t* p) {
  MT_REQUIRE(mt_dtype_ok(p->src.dtype), "%s: bad source storage type %d", who, p->src.dtype);
  MT_REQUIRE(p->src.dtype == MT_F32 || (!(p->src.cs & 1) && !(((uintptr_t)p->src.ptr) & 3)), "%s: a 16-bit source needs an even channel stride", who);
  MT_REQUIRE(p->siD == 1 && p->siH == 1 && p->siW == 1 && p->soD == 1 && p->soH == 1 && p->soW == 1 && p->Db == p->Di && p->Hb == p->Hi &&
             p->Wb == p->Wi, "%s: 1x1x1 stride-1 head only", who);
  MT_REQUIRE(p->Cout >= 1 && p->Cout <= 64 && p->src.C == p->Cin, "%s: needs 1..64 output channels", who);
  MT_REQUIRE(mt_cdiv(p->Cin, PW_CK) * PW_CK <= PW_MAXC && (double)p->Db * p->Hb * p->Wb * p->src.cs * 4.0 < 2147483648.0, "%s: sample too large", who);
  return MT_OK;
}
// the part of the kernels' parameters that has the same meaning in both
template <class Params>
static int head_infer_fill(const char* who, const mt_pointwise_t* p, int sample0, int nsamples, int nonlin, float weight, Params& P) {
  if (int rc = head_infer_head_ok(who, p)) return rc;
  MT_REQUIRE(nsamples >= 1 && nsamples <= 8 && sample0 >= 0 && sample0 + nsamples <= p->N, "%s: bad sample range", who);
  MT_REQUIRE(nonlin >= 0 && nonlin <= 2, "%s: nonlin must be 0 (none), 1 (sigmoid) or 2 (softmax)", who);
  P.c = *p; P.nchunks = mt_cdiv(p->Cin, PW_CK); P.V = (long)p->Db * p->Hb * p->Wb; P.nsb = mt_cdiv(P.V, 128);
  P.nonlin = nonlin; P.weight = weight;
  return MT_OK;
}
extern "C" int mt_head_infer_kernel_name(const mt_pointwise_t* p, int mirror, char* buf, size_t n) {
  MT_REQUIRE(p != nullptr && buf != nullptr && n > 0, "head_infer_kernel_name: null pointers");
  if (int rc = head_infer_head_ok("head_infer_kernel_name", p)) return rc;
  const HeadInferPick k = head_infer_pick(p->src.dtype, p->src.cs, p->src.ptr);
  snprintf(buf, n, "head_%s_accumulate_kernel<%d, %d>", mirror ? "mirror" : "flip", k.vec, k.xs);
  return MT_OK;
}
extern "C" int mt_head_flip_accumulate(const mt_pointwise_t* p, int sample, int flipD, int flipH, int flipW, int nonlin, float weight,
                                       float* acc, int first, mt_stream_t stream) {
  MT_REQUIRE(p != nullptr && acc != nullptr, "head_flip_accumulate: null pointers");
  HeadAccParams P;
  if (int rc = head_infer_fill("head_flip_accumulate", p, sample, 1, nonlin, weight, P)) return rc;
  P.sample = sample; P.fD = flipD; P.fH = flipH; P.fW = flipW; P.first = first; P.acc = acc;
  head_infer_instance(head_infer_pick(p->src.dtype, p->src.cs, p->src.ptr), [&](auto vec, auto xs) {
    hipLaunchKernelGGL((head_flip_accumulate_kernel<decltype(vec)::value, decltype(xs)::value>), dim3((unsigned)P.nsb), dim3(256), 0, (hipStream_t)stream, P);
  });
  MT_CHECK_LAUNCH("head_flip_accumulate");
  return MT_OK;
}
extern "C" int mt_head_mirror_accumulate(const mt_pointwise_t* p, int sample0, int nsamples, const int32_t* flips, int nonlin, float weight,
                                         const float* gauss, float* agg, float* nb, long aX, long aY, long aZ, int x0, int y0, int z0,
                                         mt_stream_t stream) {
  MT_REQUIRE(p != nullptr && agg != nullptr && flips != nullptr, "head_mirror_accumulate: null pointers");
  HeadMirParams P;
  if (int rc = head_infer_fill("head_mirror_accumulate", p, sample0, nsamples, nonlin, weight, P)) return rc;
  MT_REQUIRE(x0 >= 0 && y0 >= 0 && z0 >= 0 && x0 + p->Db <= aX && y0 + p->Hb <= aY && z0 + p->Wb <= aZ, "head_mirror_accumulate: tile outside the aggregate");
  P.sample0 = sample0; P.nsamples = nsamples; P.gauss = gauss; P.agg = agg; P.nb = nb;
  for (int k = 0; k < 8; ++k) P.flips[k] = k < nsamples ? flips[k] : 0;
  P.aX = aX; P.aY = aY; P.aZ = aZ; P.x0 = x0; P.y0 = y0; P.z0 = z0;
  head_infer_instance(head_infer_pick(p->src.dtype, p->src.cs, p->src.ptr), [&](auto vec, auto xs) {
    hipLaunchKernelGGL((head_mirror_accumulate_kernel<decltype(vec)::value, decltype(xs)::value>), dim3((unsigned)P.nsb), dim3(256), 0, (hipStream_t)stream, P);
  });
  MT_CHECK_LAUNCH("head_mirror_accumulate");
  return MT_OK;
}
