// head_bwd.hip — backward of a 1x1x1 segmentation head in one pass over (x, dY): dX, dW and dbias (mt_head_bwd), the fp64 reduces
// of its partials and the dispatch decision head_bwd_resolve that the launch, the name query and the workspace query read.
#include "pw_common.h"
#include <stdio.h>

// ================================================================================================
// Backward of a 1x1x1 segmentation head in ONE pass over (x, dY) — generic_UNet.py:349-351 / generic_modular_UNet.py:244,251:
//   dX[n,v,ci] (+)= sum_co dY[n,v,co] W[co,ci]                 (gradient w.r.t. the ACTIVATED head input a = lrelu(x*scale+shift))
//   dW[co,ci]  (+)= sum_{n,v} a[n,v,ci] dY[n,v,co],   dbias[co] (+)= sum_{n,v} dY[n,v,co]
// The separate kernels (pointwise backward-data + tiled backward-weight) moved 2 x |x| + 3 x |dY| + |dX| at 1.2-2.5 TB/s: with 47
// output channels at full resolution the heads cost 3.2 ms of a 74 ms Task100 step.  Here a wave walks over 32-voxel tiles:
//   * dX tile = dY tile (A operand: the lane's voxel row, 8 contiguous channels per 16-chunk, 16-byte loads) x W^T (packed B
//     fragments, held in registers for the whole kernel);
//   * dW += a^T dY with the VOXELS as the contraction index: both operands are then "lane = channel" rows of one voxel (coalesced
//     120 / 188-byte reads that hit the lines the dX part just fetched), two voxels per MFMA; row 31 of the last input-channel tile,
//     when free, carries 1.0 so that the same MFMAs produce dbias;
//   * every wave keeps its dW partial (NCI x 2 accumulator tiles) in registers and writes it once; head_bwd_reduce_kernel sums the
//     partials in fp64 in a fixed order (deterministic, no atomics).
struct HeadBwdParams {
  mt_src_t x; const float* dy; int dycs; int N; long V; int Cin, Cout;
  const float* wpack; float* dx; int dxcs; int accumulate_dx;
  float* part; int nwaves; long ntiles;
};
// XS: storage type of the head's input x (fp32 | fp16 | bf16); OS: of dX (fp32 | bf16).  dY (the loss gradient) is fp32.
// ST (round 5, dense tensors: x.cs == dxcs == Cin, dycs == Cout): the tile's dY block [32][Cout] and x block [32][Cin] are ONE
// contiguous run each — staged into a wave-private LDS image as coalesced 16-byte pieces, operands read from there, dX leaves the
// same way.  Without it a tile costs 70 vector-memory instructions (6 row-per-lane b128 loads, 48 two-voxel gathers of 128-376
// bytes, 16 two-row stores) for 56 MFMAs: 10.5 k cycles per tile against 3.6 k of matrix time.
template <int NCI, int XS = MT_F32, int OS = MT_F32, bool ST = false>
__global__ __launch_bounds__(256) void head_bwd_kernel(const HeadBwdParams P) {
  constexpr int XE = mt_ebytes<XS>(), OE = mt_ebytes<OS>();
  constexpr int HB_WF = 2048 + 1024 * NCI;                   // floats of a wave's image: dY [32][<= 64], x / dX [32][<= 32 NCI]
  __shared__ __attribute__((aligned(16))) float hb_img[ST ? 4 * HB_WF : 4];
  static_assert(!ST || 4 * HB_WF * sizeof(float) <= 65536, "head_bwd_kernel: the four wave images must fit the 64 KiB of static LDS (NCI <= 2)");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* const idy = hb_img + (ST ? wave * HB_WF : 0);
  float* const ixf = idy + (ST ? 2048 : 0);                  // x block (storage type XS), afterwards the dX tile in fp32
  const int li = lane & 31, lhalf = lane >> 5;
  const int gw = blockIdx.x * 4 + wave;
  const mt_src_t& S = P.x;
  const bool aff = S.scale != nullptr;
  const float slope = aff ? S.slope : 1.f;
  const int nchunks = (P.Cout + 15) / 16;                          // K chunks of the dX product (K = Cout <= 64)
  // packed W^T fragments: [ci tile][co chunk][2][64 lanes][4] — constant for the whole kernel
  f32x4 wb[NCI][4][2];
#pragma unroll
  for (int t = 0; t < NCI; ++t)
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      const float* wq = P.wpack + (size_t)(t * nchunks + ch) * 512 + lane * 4;
      wb[t][ch][0] = ch < nchunks ? *(const f32x4*)(wq) : f32x4{0.f, 0.f, 0.f, 0.f};
      wb[t][ch][1] = ch < nchunks ? *(const f32x4*)(wq + 256) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  f32x16 aw[NCI][2];
#pragma unroll
  for (int t = 0; t < NCI; ++t)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) aw[t][n][j] = 0.f;
  // the ones row (dbias): the last row of the last ci tile, when no input channel lives there
  const bool ones_free = (P.Cin % 32) != 0;
  const long tiles_per_sample = (P.V + 31) / 32;
  int cur_nb = -1;
  float xsc[NCI], xsh[NCI];
#pragma unroll
  for (int t = 0; t < NCI; ++t) { xsc[t] = 0.f; xsh[t] = 0.f; }
  for (long tile = gw; tile < P.ntiles; tile += P.nwaves) {
    const int nb = (int)(tile / tiles_per_sample);
    const long m0 = (tile - (long)nb * tiles_per_sample) * 32;
    if (nb != cur_nb) {                                            // (wave-uniform) per-(sample, channel) lazy-activation constants
      cur_nb = nb;
#pragma unroll
      for (int t = 0; t < NCI; ++t) {
        const int ci = t * 32 + li;
        const bool cv = ci < P.Cin;
        xsc[t] = cv ? (aff ? S.scale[(size_t)nb * S.C + ci] : 1.f) : 0.f;
        xsh[t] = (cv && aff) ? S.shift[(size_t)nb * S.C + ci] : 0.f;
      }
    }
    const size_t ysample = (size_t)P.V * P.dycs, xsample = (size_t)P.V * S.cs, dsample = (size_t)P.V * P.dxcs;
    __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)(P.dy + (size_t)nb * ysample), 0, (int)(ysample * 4), 0x00020000);
    __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)S.ptr + (size_t)nb * xsample * XE), 0, (int)(xsample * XE), 0x00020000);
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)P.dx + (size_t)nb * dsample * OE), 0, (int)(dsample * OE), 0x00020000);
    // ---- dX = dY W^T: A operand = this lane's voxel row of dY, channels 16 ch + 8 lhalf .. +7
    const long bv = m0 + li;
    const bool vok = bv < P.V;
    const int yoff = vok ? (int)((bv * P.dycs + 8 * lhalf) * 4) : (int)0x80000000;
    if constexpr (ST) {
      const int ybytes = 32 * P.Cout * 4, xbytes = 32 * P.Cin * XE;
      const int ybase = (int)(m0 * P.Cout * 4), xbase = (int)(m0 * P.Cin * XE);
      uint4 py[8], px[4 * NCI];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int o = (k * 64 + lane) * 16;
        py[k] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ry, o < ybytes ? ybase + o : (int)0x80000000, 0, 0));
      }
#pragma unroll
      for (int k = 0; k < 4 * NCI; ++k) {
        const int o = (k * 64 + lane) * 16;
        px[k] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, o < xbytes ? xbase + o : (int)0x80000000, 0, 0));
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();                         // the previous tile's dX pieces have left the image
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int o = (k * 64 + lane) * 16;
        if (o < ybytes) *(uint4*)((char*)idy + o) = py[k];
      }
#pragma unroll
      for (int k = 0; k < 4 * NCI; ++k) {
        const int o = (k * 64 + lane) * 16;
        if (o < xbytes) *(uint4*)((char*)ixf + o) = px[k];
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
    }
    f32x16 ax[NCI];
#pragma unroll
    for (int t = 0; t < NCI; ++t)
#pragma unroll
      for (int j = 0; j < 16; ++j) ax[t][j] = 0.f;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      if (ch < nchunks) {
        float xa[8];
        if constexpr (ST) {
#pragma unroll
          for (int e = 0; e < 8; ++e) xa[e] = idy[li * P.Cout + ch * 16 + 8 * lhalf + e];      // (rows past the sample were staged as zeros)
        } else {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ry, yoff + (ch * 16 + g * 4) * 4, 0, 0));
          xa[4 * g] = v[0]; xa[4 * g + 1] = v[1]; xa[4 * g + 2] = v[2]; xa[4 * g + 3] = v[3];
        }
        }
        const int cb = ch * 16 + 8 * lhalf;                        // a row's tail runs into the next voxel's first channels: zero them
        if (cb + 8 > P.Cout) {
#pragma unroll
          for (int e = 0; e < 8; ++e) xa[e] = (cb + e < P.Cout) ? xa[e] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < NCI; ++t) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ax[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[e], wb[t][ch][0][e], ax[t], 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 4; ++e) ax[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[4 + e], wb[t][ch][1][e], ax[t], 0, 0, 0);
        }
      }
    }
    // ---- dW += a^T dY, two voxels per MFMA (k = lhalf): operands are channel rows of voxel m0 + 2 s + lhalf
#pragma unroll 4
    for (int s2 = 0; s2 < 16; ++s2) {
      const long v = m0 + 2 * s2 + lhalf;
      const bool in = v < P.V;
      const int vo = in ? (int)(v * 4) : (int)0x80000000;          // (scaled below; bit 31 survives the multiplications as a mask)
      float av[NCI], bvv[2];
#pragma unroll
      for (int t = 0; t < NCI; ++t) {
        const int ci = t * 32 + li;
        const int o = (in && ci < P.Cin) ? (int)((v * S.cs + ci) * XE) : (int)0x80000000;
        float raw;
        if constexpr (ST) {
          const int ei = (2 * s2 + lhalf) * P.Cin + ci;
          if constexpr (XS == MT_F32) raw = (ci < P.Cin) ? ixf[ei] : 0.f;
          else raw = (ci < P.Cin) ? mt_from16<XS>(((const unsigned short*)ixf)[ei]) : 0.f;
        } else if constexpr (XS == MT_F32) raw = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, o, 0, 0));
        else raw = mt_from16<XS>(__builtin_amdgcn_raw_buffer_load_b16(rx, o, 0, 0));
        const float tt = fmaf(raw, xsc[t], xsh[t]);
        av[t] = in ? (tt > 0.f ? tt : tt * slope) : 0.f;          // (not max(t, slope t): any slope, as mt_src_t defines it)
        if (ones_free && t == NCI - 1 && li == 31) av[t] = in ? 1.f : 0.f;
      }
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int co = n * 32 + li;
        const int o = (in && co < P.Cout) ? (int)((v * P.dycs + co) * 4) : (int)0x80000000;
        if constexpr (ST) bvv[n] = (in && co < P.Cout) ? idy[(2 * s2 + lhalf) * P.Cout + co] : 0.f;
        else bvv[n] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, o, 0, 0));
      }
      (void)vo;
#pragma unroll
      for (int t = 0; t < NCI; ++t)
#pragma unroll
        for (int n = 0; n < 2; ++n) aw[t][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bvv[n], aw[t][n], 0, 0, 0);
    }
    // ---- store dX (C layout: lane = input channel column, registers = voxel rows)
    if constexpr (ST) {
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();                         // every lane has read its x operands: the region becomes the fp32 dX tile
#pragma unroll
      for (int t = 0; t < NCI; ++t) {
        const int ci = t * 32 + li;
        if (ci < P.Cin) {
#pragma unroll
          for (int j = 0; j < 16; ++j) ixf[((j & 3) + 8 * (j >> 2) + 4 * lhalf) * P.Cin + ci] = ax[t][j];
        }
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      const int dbytes = 32 * P.Cin * OE, dbase = (int)(m0 * P.Cin * OE);
#pragma unroll
      for (int k = 0; k < 4 * NCI; ++k) {
        const int o = (k * 64 + lane) * 16;                    // byte offset of this lane's 16-byte piece inside the tile's dX block
        if (o < dbytes) {
          if constexpr (OS == MT_F32) {
            f32x4 v = *(const f32x4*)((const char*)ixf + o);
            if (P.accumulate_dx) {
              const f32x4 old = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rd, dbase + o, 0, 0));
              v[0] += old[0]; v[1] += old[1]; v[2] += old[2]; v[3] += old[3];
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), rd, dbase + o, 0, 0);
          } else {
            const f32x4 v0 = *(const f32x4*)((const char*)ixf + 2 * o), v1 = *(const f32x4*)((const char*)ixf + 2 * o + 16);
            float e[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
            if (P.accumulate_dx) {
              const uint4 old = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rd, dbase + o, 0, 0));
              e[0] += mt_lo16<OS>(old.x); e[1] += mt_hi16<OS>(old.x); e[2] += mt_lo16<OS>(old.y); e[3] += mt_hi16<OS>(old.y);
              e[4] += mt_lo16<OS>(old.z); e[5] += mt_hi16<OS>(old.z); e[6] += mt_lo16<OS>(old.w); e[7] += mt_hi16<OS>(old.w);
            }
            uint4 q; q.x = mt_pk16<OS>(e[0], e[1]); q.y = mt_pk16<OS>(e[2], e[3]); q.z = mt_pk16<OS>(e[4], e[5]); q.w = mt_pk16<OS>(e[6], e[7]);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, q), rd, dbase + o, 0, 0);
          }
        }
      }
    } else
#pragma unroll
    for (int t = 0; t < NCI; ++t) {
      const int ci = t * 32 + li;
      if constexpr (OS != MT_F32) {          // channel-pair dwords (pw_pair_exchange): even lanes row j, odd lanes row j + 1; Cin, dxcs even
        const bool odd = li & 1;
        const int cie = ci & ~1;
#pragma unroll
        for (int j = 0; j < 16; j += 2) {
          const long v = m0 + (j & 3) + 8 * (j >> 2) + 4 * lhalf + (odd ? 1 : 0);
          const int o = (cie + 1 < P.Cin && v < P.V) ? (int)((v * P.dxcs + cie) * 2) : (int)0x80000000;
          float a, b;
          pw_pair_exchange(ax[t][j], ax[t][j + 1], odd, a, b);
          if (P.accumulate_dx) { const unsigned pv = __builtin_amdgcn_raw_buffer_load_b32(rd, o, 0, 0); a += mt_lo16<OS>(pv); b += mt_hi16<OS>(pv); }
          __builtin_amdgcn_raw_buffer_store_b32(mt_pk16<OS>(a, b), rd, o, 0, 0);
        }
      } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const long v = m0 + (j & 3) + 8 * (j >> 2) + 4 * lhalf;
        const int o = (ci < P.Cin && v < P.V) ? (int)((v * P.dxcs + ci) * 4) : (int)0x80000000;
        float val = ax[t][j];
        if (P.accumulate_dx) val += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, o, 0, 0));
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), rd, o, 0, 0);
      }
      }
    }
  }
  // ---- this wave's dW partial: [wave][t][n][j 16][lane 64]
  float* pp = P.part + (size_t)gw * (NCI * 2 * 1024);
#pragma unroll
  for (int t = 0; t < NCI; ++t)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) pp[((t * 2 + n) * 16 + j) * 64 + lane] = aw[t][n][j];
}

#define HB_SLICES 32
struct HeadBwdReduce { const float* part; double* tmp; int nwaves, nci, Cin, Cout; float* dw; long s_ci, s_co; float* dbias; int accumulate; };
// stage A: tmp[slice][e] = sum over the slice's partials (fp64, fixed order) — 32 x fewer dependent loads per thread than one pass
__global__ __launch_bounds__(256) void head_bwd_reduce_a_kernel(const HeadBwdReduce R) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int per = R.nci * 2 * 1024;
  if (e >= per) return;
  const int sl = blockIdx.y;
  const int w0 = (int)((long)R.nwaves * sl / HB_SLICES), w1 = (int)((long)R.nwaves * (sl + 1) / HB_SLICES);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;                   // four fixed chains: loads in flight, order independent of timing
  int w = w0;
  for (; w + 4 <= w1; w += 4) {
    s0 += (double)R.part[(size_t)w * per + e];
    s1 += (double)R.part[(size_t)(w + 1) * per + e];
    s2 += (double)R.part[(size_t)(w + 2) * per + e];
    s3 += (double)R.part[(size_t)(w + 3) * per + e];
  }
  for (; w < w1; ++w) s0 += (double)R.part[(size_t)w * per + e];
  R.tmp[(size_t)sl * per + e] = (s0 + s1) + (s2 + s3);
}
// stage B: element e = ((t*2 + n)*16 + j)*64 + lane of the accumulator layout -> dW[co][ci] / dbias[co]
__global__ __launch_bounds__(256) void head_bwd_reduce_b_kernel(const HeadBwdReduce R) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int per = R.nci * 2 * 1024;
  if (e >= per) return;
  const int lane = e & 63, j = (e >> 6) & 15, tn = e >> 10, n = tn & 1, t = tn >> 1;
  const int row = (j & 3) + 8 * (j >> 2) + 4 * (lane >> 5), col = lane & 31;
  const int ci = t * 32 + row, co = n * 32 + col;
  const bool is_bias = (R.Cin % 32) != 0 && t == R.nci - 1 && row == 31;
  if (co >= R.Cout || (ci >= R.Cin && !is_bias)) return;
  double a = 0.0;
  for (int sl = 0; sl < HB_SLICES; ++sl) a += R.tmp[(size_t)sl * per + e];
  const float s = (float)a;
  if (is_bias) { if (R.dbias != nullptr) R.dbias[co] = R.accumulate ? R.dbias[co] + s : s; return; }
  float* o = R.dw + (long)ci * R.s_ci + (long)co * R.s_co;
  *o = R.accumulate ? *o + s : s;
}

// ---- narrow heads (Cout <= 4, 30 / 32 dense input channels; see pw_narrow_kernel): the same three results from one streaming pass
// with a thread per voxel — dX[v][ci] (+)= sum_co dY[v][co] W[co][ci]; per-thread partial sums of dW[co][ci] = sum_v act(x)[v][ci]
// dY[v][co] and dbias[co] = sum_v dY[v][co] in registers over the thread's voxels, reduced over the wave by DPP shuffles and over
// the workgroup through LDS in a fixed order; one partial row per workgroup, summed in fp64 by head_narrow_reduce_kernel.
#define HN_BLOCKS 1024
// a lane's row of CIN channels in the wave's LDS image (rows are only 8- / 4-byte aligned: 120 / 60 bytes apart)
template <int CIN, int ST>
__device__ __forceinline__ void hn_row_from_lds(const char* row, float (&x)[CIN + 2]) {
  if constexpr (ST == MT_F32) {
#pragma unroll
    for (int q = 0; q < CIN / 2; ++q) { const float2 t = *(const float2*)(row + q * 8); x[2 * q] = t.x; x[2 * q + 1] = t.y; }
  } else {
#pragma unroll
    for (int q = 0; q < CIN / 2; ++q) { const unsigned d = *(const unsigned*)(row + q * 4); x[2 * q] = mt_lo16<ST>(d); x[2 * q + 1] = mt_hi16<ST>(d); }
  }
}
template <int CIN, int ST>
__device__ __forceinline__ void hn_row_to_lds(char* row, const float (&x)[CIN + 2]) {
  if constexpr (ST == MT_F32) {
#pragma unroll
    for (int q = 0; q < CIN / 2; ++q) { float2 t; t.x = x[2 * q]; t.y = x[2 * q + 1]; *(float2*)(row + q * 8) = t; }
  } else {
#pragma unroll
    for (int q = 0; q < CIN / 2; ++q) *(unsigned*)(row + q * 4) = mt_pk16<ST>(x[2 * q], x[2 * q + 1]);
  }
}
template <int CIN, int NCO, int XS = MT_F32, int OS = MT_F32>
__global__ __launch_bounds__(256) void head_bwd_narrow_kernel(const HeadBwdParams P) {
  static_assert(CIN % 2 == 0, "channel pairs");
  __shared__ __attribute__((aligned(16))) float hn_img[4 * 64 * CIN];          // one [64 voxels][CIN] image per wave (fp32-sized)
  constexpr int XE = mt_ebytes<XS>(), OE = mt_ebytes<OS>();
  constexpr int NP = NCO * CIN + NCO;                       // partial sums per thread: dW rows, then dbias
  __shared__ __attribute__((aligned(16))) float sw[NCO][CIN + 2], ssc[CIN + 2], ssh[CIN + 2];
  __shared__ float red[4][NP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const mt_src_t& S = P.x;
  const bool aff = S.scale != nullptr;
  const float slope = aff ? S.slope : 1.f;
  for (int i = tid; i < NCO * CIN; i += 256) {
    const int co = i / CIN, ci = i - co * CIN;
    sw[co][ci] = co < P.Cout ? P.wpack[ci * 4 + co] : 0.f;   // packed W^T (K = Cout in one chunk, co < 4: [lane = ci][e = co])
  }
  float part[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) part[k] = 0.f;
  const long per_sample_blocks = HN_BLOCKS / P.N > 0 ? HN_BLOCKS / P.N : 1;
  const int nb = (int)(blockIdx.x / per_sample_blocks);      // a workgroup stays inside one sample (its scale / shift)
  if (nb < P.N) {
    const long b = blockIdx.x - (long)nb * per_sample_blocks;
    for (int i = tid; i < CIN; i += 256) {
      ssc[i] = aff ? S.scale[(size_t)nb * S.C + i] : 1.f;
      ssh[i] = aff ? S.shift[(size_t)nb * S.C + i] : 0.f;
    }
    __syncthreads();
    const size_t xs = (size_t)P.V * CIN;
    __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)S.ptr + (size_t)nb * xs * XE), 0, (int)(xs * XE), 0x00020000);
    __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)P.dx + (size_t)nb * xs * OE), 0, (int)(xs * OE), 0x00020000);
    const float* dyp = P.dy + (size_t)nb * P.V * P.dycs;
    // Rows through LDS (round 5).  A thread owns a voxel and needs its CIN channels as registers, but a row-per-lane access is 64
    // pieces at 120-byte (60-byte) strides per instruction: 3.3 TB/s.  The rows of a wave's 64 consecutive voxels are ONE contiguous
    // block of 64 * CIN elements, so the wave moves it as 16-byte pieces (lane l: pieces l, l + 64, ...) through a wave-private LDS
    // image of the same linear layout, and every lane reads / writes its own row there.
    constexpr int ROWX = CIN * XE, ROWO = CIN * OE;            // bytes per row
    constexpr int NPX = 64 * ROWX / 16, NPO = 64 * ROWO / 16;  // 16-byte pieces of a wave's block
    char* const img = (char*)hn_img + wave * (64 * CIN * 4);
    for (long v0 = b * 256 + wave * 64; v0 < P.V; v0 += per_sample_blocks * 256) {
      const long v = v0 + lane;
      const bool vok = v < P.V;
      float x[CIN + 2], old[CIN + 2], dy[NCO];
      {
        uint4 pc[(NPX + 63) / 64];
#pragma unroll
        for (int k = 0; k < (NPX + 63) / 64; ++k) {
          const int p = k * 64 + lane;
          pc[k] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ra, p < NPX ? (int)(v0 * ROWX) + p * 16 : (int)0x80000000, 0, 0));
        }
#pragma unroll
        for (int k = 0; k < (NPX + 63) / 64; ++k) {
          const int p = k * 64 + lane;
          if (p < NPX) *(uint4*)(img + p * 16) = pc[k];
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        hn_row_from_lds<CIN, XS>(img + lane * ROWX, x);
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
      }
      if (P.accumulate_dx) {
        uint4 pc[(NPO + 63) / 64];
#pragma unroll
        for (int k = 0; k < (NPO + 63) / 64; ++k) {
          const int p = k * 64 + lane;
          pc[k] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, p < NPO ? (int)(v0 * ROWO) + p * 16 : (int)0x80000000, 0, 0));
        }
#pragma unroll
        for (int k = 0; k < (NPO + 63) / 64; ++k) {
          const int p = k * 64 + lane;
          if (p < NPO) *(uint4*)(img + p * 16) = pc[k];
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        hn_row_from_lds<CIN, OS>(img + lane * ROWO, old);
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
      }
#pragma unroll
      for (int co = 0; co < NCO; ++co) dy[co] = (vok && co < P.Cout) ? dyp[v * P.dycs + co] : 0.f;      // (a lane past the sample adds nothing)
      float dx[CIN + 2];
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) {
        const float t = fmaf(x[ci], ssc[ci], ssh[ci]);
        const float a = fmaxf(t, t * slope);
        float g = P.accumulate_dx ? old[ci] : 0.f;
#pragma unroll
        for (int co = 0; co < NCO; ++co) {
          g = fmaf(dy[co], sw[co][ci], g);
          part[co * CIN + ci] = fmaf(a, dy[co], part[co * CIN + ci]);
        }
        dx[ci] = g;
      }
#pragma unroll
      for (int co = 0; co < NCO; ++co) part[NCO * CIN + co] += dy[co];
      hn_row_to_lds<CIN, OS>(img + lane * ROWO, dx);
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int k = 0; k < (NPO + 63) / 64; ++k) {
        const int p = k * 64 + lane;
        if (p < NPO) {                                         // (pieces past the sample's last row: beyond num_records, dropped)
          const uint4 q = *(const uint4*)(img + p * 16);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, q), rx, (int)(v0 * ROWO) + p * 16, 0, 0);
        }
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
    }
  }
  // wave reduction (fixed butterfly), then the four waves through LDS in wave order
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    float s = part[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  for (int k = tid; k < NP; k += 256) P.part[(size_t)blockIdx.x * NP + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}
// dW[co][ci] / dbias[co] (+)= sum over the workgroups' partial rows, in block order, fp64
__global__ __launch_bounds__(64) void head_narrow_reduce_kernel(const float* part, int nblocks, int np, int Cin, int Cout, int nco, float* dw, long s_ci,
                                                               long s_co, float* dbias, int accumulate) {
  const int k = blockIdx.x;                                 // one partial column per workgroup, 64 lanes over the rows
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) s += (double)part[(size_t)b * np + k];
  s = mt_wave_sum_d(s);
  if (threadIdx.x != 0) return;
  const int co = k < nco * Cin ? k / Cin : k - nco * Cin, ci = k < nco * Cin ? k - co * Cin : -1;
  if (co >= Cout) return;
  if (ci >= 0) { float* o = dw + (long)ci * s_ci + (long)co * s_co; *o = accumulate ? *o + (float)s : (float)s; }
  else if (dbias != nullptr) dbias[co] = accumulate ? dbias[co] + (float)s : (float)s;
}

// ---- dispatch: ONE decision per launch (head_bwd_resolve); the launch and the kernel name read it, the workspace query shares
// its size functions
// Cin <= 32 only: the two-input-tile instantiation (Cin <= 64) needs 182 VGPRs (one wave per SIMD) and measured 0.70 ms on the
// 24x96x96 level — slower than the generic kernels there, so callers are told to keep those on the separate kernels; mt_head_bwd
// itself serves Cin <= 64
extern "C" int mt_head_bwd_supported(int Cin, int Cout) { return Cin >= 1 && Cin <= 32 && Cout >= 1 && Cout <= 64; }
// storage types mt_head_bwd takes natively: x fp32 with dX fp32; x fp16 or bf16 with dX bf16 (even Cin and channel strides, dword-aligned
// bases); dY is the fp32 loss gradient
extern "C" int mt_head_bwd_io_supported(int xdtype, int xcs, int dxdtype, int dxcs, int Cin, int Cout) {
  if (xdtype == MT_F32 && dxdtype == MT_F32) return 1;
  if (!(mt_is16(xdtype) && dxdtype == MT_BF16)) return 0;
  return ((Cin & 1) || (xcs & 1) || (dxcs & 1)) ? 0 : 1;
}
static inline int head_bwd_waves(int N, long V) {
  const long ntiles = (long)N * ((V + 31) / 32);
  long w = ntiles / 32;                                            // >= 32 tiles per wave: the 8 - 16 KiB partial of a wave is written once
  if (w > 256 * 4 * 4) w = 256 * 4 * 4;                            // at most 4 workgroups of 4 waves per CU
  if (w < 4) w = 4;
  return (int)((w + 3) / 4 * 4);
}
// workspace of the two forms: per-wave partials of nci x 2 accumulator tiles plus the fp64 slices of the first reduce | one partial
// row of np floats per workgroup
static inline size_t head_bwd_per(int Cin) { return (size_t)((Cin + 31) / 32) * 2 * 1024; }
static inline size_t head_bwd_tiled_bytes(int nwaves, size_t per) { return (size_t)nwaves * per * sizeof(float) + HB_SLICES * per * sizeof(double) + 64; }
static inline size_t head_bwd_narrow_bytes(int nblocks, int np) { return (size_t)nblocks * np * sizeof(float); }
struct HeadBwdChoice {
  bool narrow, staged;     // head_bwd_narrow_kernel<tiles, nco, ..> | head_bwd_kernel<tiles, .., ST = staged>
  int tiles;               // narrow: CIN (30 | 32); else NCI, the 32-channel input tiles (1 | 2)
  int nco, np, nblocks;    // narrow: output channels a thread keeps (2 | 4), floats per partial row, workgroups
  int nwaves; size_t per;  // else: waves and floats per wave partial
  int xs, os;              // storage types of x and dX
  int dbias_done;          // 0: the caller sums dY itself (mt_channel_sum)
};
// dx may be NULL (the name query has none)
static int head_bwd_resolve(const mt_src_t* x, int dycs, int N, long V, int Cin, int Cout, const void* dx, int dxcs, int dxdtype, HeadBwdChoice& c) {
  MT_REQUIRE(x && x->ptr && N > 0 && V > 0, "head_bwd: null / empty argument");
  MT_REQUIRE(mt_head_bwd_io_supported(x->dtype, x->cs, dxdtype, dxcs, Cin, Cout) && !(((uintptr_t)x->ptr) & 3) && !(((uintptr_t)dx) & 3),
             "head_bwd: storage types (x %d, dX %d) not taken (ask mt_head_bwd_io_supported, convert with mt_cast)", x->dtype, dxdtype);
  MT_REQUIRE(Cin >= 1 && Cin <= 64 && Cout >= 1 && Cout <= 64, "head_bwd: Cin (%d) and Cout (%d) must be <= 64", Cin, Cout);
  MT_REQUIRE(x->C == Cin, "head_bwd: x->C != Cin");
  MT_REQUIRE((double)V * x->cs * 4.0 < 2147483648.0 && (double)V * dycs * 4.0 < 2147483648.0 && (double)V * dxcs * 4.0 < 2147483648.0, "head_bwd: sample larger than 2 GiB");
  c.xs = x->dtype; c.os = mt_is16(c.xs) ? MT_BF16 : MT_F32;
  c.narrow = Cout <= 4 && (Cin == 30 || Cin == 32) && x->cs == Cin && dxcs == Cin && N <= HN_BLOCKS &&
             (x->scale == nullptr || (x->slope >= 0.f && x->slope <= 1.f)) && (double)V * Cin * 4.0 < 2147483648.0;
  c.staged = false; c.nco = c.np = c.nblocks = c.nwaves = 0; c.per = 0;
  if (c.narrow) {
    c.tiles = Cin; c.nco = Cout <= 2 ? 2 : 4; c.np = c.nco * Cin + c.nco;
    c.nblocks = (HN_BLOCKS / N > 0 ? HN_BLOCKS / N : 1) * N;
    c.dbias_done = 1;
    return MT_OK;
  }
  c.tiles = (Cin + 31) / 32;
  // dense tensors: the tile's dY and x blocks are one contiguous run each, staged through LDS (see head_bwd_kernel, ST)
  c.staged = x->cs == Cin && dxcs == Cin && dycs == Cout && (mt_is16(c.xs) ? (Cin % 2) == 0 : true);
  c.nwaves = head_bwd_waves(N, V); c.per = head_bwd_per(Cin);
  c.dbias_done = ((Cin % 32) != 0) ? 1 : 0;      // a spare MFMA row of the last input tile carries 1.0
  return MT_OK;
}
// The query knows neither strides nor storage types: the maximum over the forms a launch with these sizes could choose
extern "C" size_t mt_head_bwd_workspace(int N, long V, int Cin, int Cout) {
  if (!(Cin >= 1 && Cin <= 64 && Cout >= 1 && Cout <= 64)) return 0;
  const size_t tiled = head_bwd_tiled_bytes(head_bwd_waves(N, V), head_bwd_per(Cin));
  const size_t narrow = (Cout <= 4) ? head_bwd_narrow_bytes(HN_BLOCKS, 4 * 32 + 4) : 0;      // head_bwd_narrow_kernel: one partial row per workgroup
  return tiled > narrow ? tiled : narrow;
}
extern "C" int mt_head_bwd_kernel_name(const mt_src_t* x, int dycs, int N, long V, int Cin, int Cout, int dxcs, int dxdtype, char* buf, size_t n,
                                       int* dbias_done) {
  MT_REQUIRE(buf != nullptr && n > 0, "head_bwd_kernel_name: no buffer");
  HeadBwdChoice c;
  if (int rc = head_bwd_resolve(x, dycs, N, V, Cin, Cout, nullptr, dxcs, dxdtype, c)) return rc;
  if (c.narrow) snprintf(buf, n, "head_bwd_narrow_kernel<%d, %d, %d, %d>", c.tiles, c.nco, c.xs, c.os);
  else snprintf(buf, n, "head_bwd_kernel<%d, %d, %d, %s>", c.tiles, c.xs, c.os, c.staged ? "true" : "false");
  if (dbias_done != nullptr) *dbias_done = c.dbias_done;
  return MT_OK;
}

template <int CIN, int NCO>
static void head_bwd_launch_narrow(const HeadBwdChoice& c, const HeadBwdParams& P, hipStream_t st) {
  const dim3 g(c.nblocks);
  if (c.xs == MT_F16) hipLaunchKernelGGL((head_bwd_narrow_kernel<CIN, NCO, MT_F16, MT_BF16>), g, dim3(256), 0, st, P);
  else if (c.xs == MT_BF16) hipLaunchKernelGGL((head_bwd_narrow_kernel<CIN, NCO, MT_BF16, MT_BF16>), g, dim3(256), 0, st, P);
  else hipLaunchKernelGGL((head_bwd_narrow_kernel<CIN, NCO>), g, dim3(256), 0, st, P);
}
template <int NCI, bool ST>
static void head_bwd_launch_tiled(const HeadBwdChoice& c, const HeadBwdParams& P, hipStream_t st) {
  const dim3 g(c.nwaves / 4);
  if (c.xs == MT_F16) hipLaunchKernelGGL((head_bwd_kernel<NCI, MT_F16, MT_BF16, ST>), g, dim3(256), 0, st, P);
  else if (c.xs == MT_BF16) hipLaunchKernelGGL((head_bwd_kernel<NCI, MT_BF16, MT_BF16, ST>), g, dim3(256), 0, st, P);
  else hipLaunchKernelGGL((head_bwd_kernel<NCI, MT_F32, MT_F32, ST>), g, dim3(256), 0, st, P);
}
extern "C" int mt_head_bwd(const mt_src_t* x, const float* dy, int dycs, int N, long V, int Cin, int Cout, const float* wpack_bwd,
                           float* dx, int dxcs, int dxdtype, int accumulate_dx, float* dw, long s_ci, long s_co, float* dbias, int accumulate_dw,
                           int* dbias_done, void* ws, size_t ws_bytes, mt_stream_t stream) {
  MT_REQUIRE(dy && wpack_bwd && dx && dw, "head_bwd: null / empty argument");
  HeadBwdChoice c;
  if (int rc = head_bwd_resolve(x, dycs, N, V, Cin, Cout, dx, dxcs, dxdtype, c)) return rc;
  if (ws == nullptr || ws_bytes < mt_head_bwd_workspace(N, V, Cin, Cout)) { mt_set_error("head_bwd: workspace too small"); return MT_EWORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  HeadBwdParams P;
  P.x = *x; P.dy = dy; P.dycs = dycs; P.N = N; P.V = V; P.Cin = Cin; P.Cout = Cout; P.wpack = wpack_bwd;
  P.dx = dx; P.dxcs = dxcs; P.accumulate_dx = accumulate_dx; P.part = (float*)ws;
  if (c.narrow) {
    MT_REQUIRE(head_bwd_narrow_bytes(c.nblocks, c.np) <= ws_bytes, "head_bwd: workspace too small for the narrow form");
    if (c.tiles == 30 && c.nco == 2) head_bwd_launch_narrow<30, 2>(c, P, st);
    else if (c.tiles == 30) head_bwd_launch_narrow<30, 4>(c, P, st);
    else if (c.nco == 2) head_bwd_launch_narrow<32, 2>(c, P, st);
    else head_bwd_launch_narrow<32, 4>(c, P, st);
    hipLaunchKernelGGL(head_narrow_reduce_kernel, dim3(c.np), dim3(64), 0, st, (const float*)ws, c.nblocks, c.np, Cin, Cout, c.nco, dw, s_ci, s_co, dbias, accumulate_dw);
    MT_CHECK_LAUNCH("head_bwd_narrow");
  } else {
    P.nwaves = c.nwaves; P.ntiles = (long)N * ((V + 31) / 32);
    if (c.staged) { if (c.tiles == 1) head_bwd_launch_tiled<1, true>(c, P, st); else head_bwd_launch_tiled<2, true>(c, P, st); }
    else { if (c.tiles == 1) head_bwd_launch_tiled<1, false>(c, P, st); else head_bwd_launch_tiled<2, false>(c, P, st); }
    MT_CHECK_LAUNCH("head_bwd");
    HeadBwdReduce R;
    R.part = (const float*)ws; R.nwaves = c.nwaves; R.nci = c.tiles; R.Cin = Cin; R.Cout = Cout; R.dw = dw; R.s_ci = s_ci; R.s_co = s_co;
    R.dbias = dbias; R.accumulate = accumulate_dw;
    R.tmp = (double*)(((uintptr_t)((float*)ws + (size_t)c.nwaves * c.per) + 7) & ~(uintptr_t)7);
    hipLaunchKernelGGL(head_bwd_reduce_a_kernel, dim3(mt_cdiv((long)c.per, 256), HB_SLICES), dim3(256), 0, st, R);
    hipLaunchKernelGGL(head_bwd_reduce_b_kernel, dim3(mt_cdiv((long)c.per, 256)), dim3(256), 0, st, R);
    MT_CHECK_LAUNCH("head_bwd_reduce");
  }
  if (dbias_done != nullptr) *dbias_done = c.dbias_done;
  return MT_OK;
}
