// pointwise.hip — 1x1x1 convolutions and kernel==stride transposed convolutions on fp32 MFMA.
//
// Replaces: seg heads nn.Conv3d(C, num_classes, 1) (generic_UNet.py:349-351; generic_modular_UNet.py:244,251),
// strided 1x1x1 skip projections (conv_blocks.py:192-197), nn.ConvTranspose3d(k == stride, bias=False)
// (generic_UNet.py:335-336; generic_modular_UNet.py:236-237) and, with transposed packed weights,
// the backward-data of the 1x1x1 convs.
//
// For a transposed conv every tap is an independent GEMM whose rows are scattered to out[base*so + tap] — written
// directly into the first half of the skip-concat buffer (ocs).  Weights: mt_pack_conv_weights(layout 1, ck 16).
//
// The fused inference heads live in head_infer.hip, the fused head backward in head_bwd.hip, the device probe in probe.hip;
// pw_common.h holds what they share with this unit.
#include "pw_common.h"
#include <stdio.h>

// One wave = 32 base voxels x 32 output channels x NT taps.  Lane (i, h) holds channels 8h..8h+7 of voxel i for the current
// 16-channel chunk (one 32-byte vector straight from global memory, lazy InstanceNorm+LeakyReLU applied in registers), so a
// chunk costs 8 MFMAs per tap with no LDS traffic at all; every tap of a transposed conv accumulates into its own
// accumulator tile (NT*16 AGPRs) and the input is read exactly once.  Outputs leave through buffer stores whose per-row
// offsets are computed once (out-of-range rows carry the hardware-masked offset).
#ifndef PW_ABL
#define PW_ABL 0      // timing ablations of pw_fast_kernel: 1 no stores, 2 no weight-fragment loads, 4 no MFMAs
#endif
// M16 (mixed precision, fp16 source, mt_pointwise_t.mma == 1): the activated fragment is rounded to fp16 and multiplied by pack-layout-4
// weights — one v_mfma_f32_32x32x16_f16 per (chunk, tap) instead of eight fp32 MFMAs (the forward transposed convs ran AT the fp32 matrix rate)
template <int NT, int XS = MT_F32, int OS = MT_F32, bool M16 = false>
__global__ __launch_bounds__(256) void pw_fast_kernel(const PwKParams P) {
  constexpr int XE = mt_ebytes<XS>(), OE = mt_ebytes<OS>();     // bytes per stored element
  const mt_pointwise_t& c = P.c;
  __shared__ float red[4 * 32 * 2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  const int bx = mt_xcd_remap(blockIdx.x, gridDim.x);
  const int nb = bx / P.nsb, sb = bx % P.nsb;
  const int ntile = blockIdx.y;
  const long m0 = (long)sb * 128 + wave * 32;
  const mt_src_t& S = c.src;

  // ---- A operand: this lane's base voxel, channels 8*lhalf .. +7 of each chunk
  const long bv = m0 + li;
  const bool vok = bv < P.Vb;
  // (d, h, w) of the wave's first voxel by ONE wave-uniform division; a row 0..31 further only carries once into h and once into
  // d when the rows are at least 32 voxels long (otherwise: the general division per lane).  The per-row divisions of the first
  // version (1 + 16 of them per lane, ~40 VALU each) cost more than the 16 MFMAs of the tile.
  const int w0 = (int)(m0 % c.Wb), h0 = (int)((m0 / c.Wb) % c.Hb), d0 = (int)(m0 / ((long)c.Wb * c.Hb));
  const bool longrows = c.Wb >= 32;
  auto row_dhw = [&](int iv, int& d, int& h, int& w) {
    if (longrows) {
      w = w0 + iv; h = h0; d = d0;
      const bool cw = w >= c.Wb;
      w = cw ? w - c.Wb : w; h = cw ? h + 1 : h;
      const bool chh = h >= c.Hb;
      h = chh ? h - c.Hb : h; d = chh ? d + 1 : d;
    } else {
      const long v = m0 + iv;
      w = (int)(v % c.Wb); h = (int)((v / c.Wb) % c.Hb); d = (int)(v / ((long)c.Wb * c.Hb));
    }
  };
  int wb, hb, db;
  row_dhw(li, db, hb, wb);
  const size_t in_sample = (size_t)c.Di * c.Hi * c.Wi * S.cs;
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)S.ptr + (size_t)nb * in_sample * XE), 0,
                                                                (int)(in_sample * XE), 0x00020000);
  const int aoff = vok ? ((((db * c.siD) * c.Hi + hb * c.siH) * c.Wi + wb * c.siW) * S.cs + 8 * lhalf) * XE : (int)0x80000000;
  const bool aff = S.scale != nullptr;
  const float slope = S.slope;
  const bool lrelu_ok = (slope >= 0.f) && (slope <= 1.f);
  // the producer's per-(sample, channel) scale / shift once per workgroup in LDS: fetching them per element through the vector
  // memory path cost 16 extra VMEM instructions per chunk and lane (measured: 30 -> 47 head 3.1 ms)
  __shared__ __attribute__((aligned(16))) float ssc[PW_MAXC], ssh[PW_MAXC];
  if (aff) {
    for (int i = tid; i < P.nchunks * PW_CK; i += 256) {
      ssc[i] = i < S.C ? S.scale[(size_t)nb * S.C + i] : 0.f;
      ssh[i] = i < S.C ? S.shift[(size_t)nb * S.C + i] : 0.f;
    }
    __syncthreads();
  }

  auto load_a = [&](int ch, float (&x)[8]) { pw_load8<XS>(ra, aoff + ch * (PW_CK * XE), x); };
  // channels beyond Cin inside the last chunk may hold neighbouring data: zero them (and apply the lazy activation)
  auto finish_a = [&](int ch, float (&x)[8]) {
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
  };

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[t][j] = 0.f;
  // blockIdx.z: which NT of the P.ntaps taps this workgroup computes (8 taps as two workgroups of 4: half the accumulator
  // registers, twice the resident workgroups — their store phases overlap the others' multiplications)
  const int tap0 = (int)blockIdx.z * NT;

  float xa[8], xn[8];
  load_a(0, xa);
  for (int ch = 0; ch < P.nchunks; ++ch) {
    if (ch + 1 < P.nchunks) load_a(ch + 1, xn);
    finish_a(ch, xa);
    if constexpr (M16) {
      typedef _Float16 pw_f16x8 __attribute__((ext_vector_type(8)));
      uint4 af;
      af.x = mt_pk16<MT_F16>(xa[0], xa[1]); af.y = mt_pk16<MT_F16>(xa[2], xa[3]); af.z = mt_pk16<MT_F16>(xa[4], xa[5]); af.w = mt_pk16<MT_F16>(xa[6], xa[7]);
      const unsigned* wq16 = (const unsigned*)c.wpack + ((size_t)(ntile * P.nchunks + ch) * P.ntaps + tap0) * 256 + lane * 4;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const uint4 b = *(const uint4*)(wq16 + t * 256);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(pw_f16x8, af), __builtin_bit_cast(pw_f16x8, b), acc[t], 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) xa[e] = xn[e];
      continue;
    }
    const float* wq = c.wpack + ((size_t)(ntile * P.nchunks + ch) * P.ntaps + tap0) * 512 + lane * 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4 b0, b1;
      if (PW_ABL & 2) { b0 = f32x4{xa[0], xa[1], xa[2], xa[3]}; b1 = f32x4{xa[4], xa[5], xa[6], xa[7]}; }
      else { b0 = *(const f32x4*)(wq + t * 512); b1 = *(const f32x4*)(wq + t * 512 + 256); }
      if (PW_ABL & 4) { acc[t][0] += xa[t & 7] * b0[0] + b1[1]; continue; }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[e], b0[e], acc[t], 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[4 + e], b1[e], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) xa[e] = xn[e];
  }
  if (PW_ABL & 1) {
    float sacc = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 16; ++j) sacc += acc[t][j];
    if (sacc == 1234.5678f) c.out[0] = sacc;
    return;
  }

  // ---- epilogue
  const int co = ntile * 32 + li;
  const bool covalid = co < c.Cout;
  const float bias = (c.bias != nullptr && covalid) ? c.bias[co] : 0.f;
  const int Ho = c.Hb * c.soH, Wo = c.Wb * c.soW, Do = c.Db * c.soD;
  const size_t out_sample = (size_t)Do * Ho * Wo * c.ocs;
  __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)c.out + (size_t)nb * out_sample * OE), 0,
                                                                (int)(out_sample * OE), 0x00020000);
  if constexpr (NT >= 4) {
    // Wide epilogue of the transposed convolutions (soW == 2, the wave's 32 base voxels in one row, <= 32 even output channels):
    // the two kw taps of a (kd, kh) pair are 64 CONSECUTIVE output voxels.  The dword stores of the plain epilogue (one per
    // accumulator element: 128 store instructions per wave, each two 120-byte runs) were 300 of the 460 us of the 60 -> 30
    // launch (PW_ABL=1); here the pair goes through a wave-private LDS tile [64 voxels][32] and leaves as 16-byte stores.
    if (P.wide) {
      __shared__ __attribute__((aligned(16))) float wst[4][64 * 32];
      float* sg = wst[wave];
      int wb0, hb0, db0;
      row_dhw(0, db0, hb0, wb0);                             // the row of the wave's first voxel (the whole wave is in it)
      const bool wok = m0 < P.Vb;
      const int pv = lane >> 3, pc = (lane & 7) * 4;         // piece (lane & 7) of output voxel pv + 8 k
#pragma unroll
      for (int pr = 0; pr < NT / 2; ++pr) {                  // (kd, kh) pairs: taps 2 pr (kw = 0) and 2 pr + 1 (kw = 1)
        const int prg = pr + tap0 / 2;
        const int th = prg % c.soH, tdd = prg / c.soH;
#pragma unroll
        for (int tw = 0; tw < 2; ++tw)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int iv = (j & 3) + 8 * (j >> 2) + 4 * lhalf;
            sg[(2 * iv + tw) * 32 + li] = acc[2 * pr + tw][j] + bias;
          }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        if (wok && P.wide == 2) {
          // dense output (channel stride == Cout): the pair's 64 voxels are ONE run of 64 * Cout floats
          const int rowbase = ((((db0 * c.soD + tdd) * Ho + hb0 * c.soH + th) * Wo + wb0 * 2) * c.Cout) * OE;
          const int n2 = 32 * c.Cout;                        // channel pairs: 8-byte units (fp32) / dwords (16-bit)
          for (int u = lane; u < n2; u += 64) {
            const int e = 2 * u, ov = e / c.Cout, cc = e - ov * c.Cout;      // (Cout even: a unit never straddles two voxels)
            const float2 h = *(const float2*)(sg + ov * 32 + cc);
            if constexpr (OS == MT_F32) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, h), ro, rowbase + u * 8, 0, 0);
            else __builtin_amdgcn_raw_buffer_store_b32(mt_pk16<OS>(h.x, h.y), ro, rowbase + u * 4, 0, 0);
          }
        } else if (wok) {
          const int rowbase = ((((db0 * c.soD + tdd) * Ho + hb0 * c.soH + th) * Wo + wb0 * 2) * c.ocs) * OE;      // bytes
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int ov = pv + 8 * k;
            const f32x4 v = *(const f32x4*)(sg + ov * 32 + pc);
            const int o = rowbase + (ov * c.ocs + pc) * OE;
            if constexpr (OS == MT_F32) {
              if (pc + 4 <= c.Cout)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), ro, o, 0, 0);
              else if (pc + 2 <= c.Cout) {
                float2 h; h.x = v[0]; h.y = v[1];
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, h), ro, o, 0, 0);
              }
            } else {
              if (pc + 4 <= c.Cout) {
                uint2 h; h.x = mt_pk16<OS>(v[0], v[1]); h.y = mt_pk16<OS>(v[2], v[3]);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, h), ro, o, 0, 0);
              } else if (pc + 2 <= c.Cout) {
                __builtin_amdgcn_raw_buffer_store_b32(mt_pk16<OS>(v[0], v[1]), ro, o, 0, 0);
              }
            }
          }
        }
        __builtin_amdgcn_wave_barrier();                     // the tile is rewritten by the next pair
      }
      return;
    }
  }
  float s1 = 0.f, s2 = 0.f;
  if constexpr (OS != MT_F32) {
    // 16-bit destination: channel-pair dwords (pw_pair_exchange) — even lanes store accumulator row j, odd lanes row j + 1
    const bool odd = li & 1;
    const int coe = co & ~1;
    const bool pvalid = coe + 1 < c.Cout;                 // (Cout, ocs even: mt_pointwise_io_supported)
    int pbase[8];
#pragma unroll
    for (int jp = 0; jp < 8; ++jp) {
      const int j = 2 * jp;
      const int iv = (j & 3) + 8 * (j >> 2) + 4 * lhalf + (odd ? 1 : 0);
      const long v = m0 + iv;
      int w2, h2, d2;
      row_dhw(iv, d2, h2, w2);
      const bool ok = pvalid && v < P.Vb;
      pbase[jp] = ok ? ((((d2 * c.soD) * Ho + h2 * c.soH) * Wo + w2 * c.soW) * c.ocs + coe) * 2 : (int)0x80000000;
    }
    float q1[2] = {0.f, 0.f}, q2[2] = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int tg = tap0 + t;
      const int tw = tg % c.soW, th = (tg / c.soW) % c.soH, tdd = tg / (c.soW * c.soH);
      const int toff = ((tdd * Ho + th) * Wo + tw) * c.ocs * 2;
#pragma unroll
      for (int jp = 0; jp < 8; ++jp) {
        float a, b;
        pw_pair_exchange(acc[t][2 * jp] + bias, acc[t][2 * jp + 1] + bias, odd, a, b);
        if (c.accumulate) { const unsigned pv = __builtin_amdgcn_raw_buffer_load_b32(ro, pbase[jp], toff, 0); a += mt_lo16<OS>(pv); b += mt_hi16<OS>(pv); }
        const unsigned pk = mt_pk16<OS>(a, b);
        __builtin_amdgcn_raw_buffer_store_b32(pk, ro, pbase[jp], toff, 0);
        if (c.stats_part != nullptr && pbase[jp] >= 0) {
          const float ar = mt_lo16<OS>(pk), br = mt_hi16<OS>(pk);
          q1[0] += ar; q2[0] = fmaf(ar, ar, q2[0]); q1[1] += br; q2[1] = fmaf(br, br, q2[1]);
        }
      }
    }
    s1 = pw_pair_combine(q1[0], q1[1], odd);
    s2 = pw_pair_combine(q2[0], q2[1], odd);
  } else {
  int obase[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int iv = (j & 3) + 8 * (j >> 2) + 4 * lhalf;
    const long v = m0 + iv;
    int w2, h2, d2;
    row_dhw(iv, d2, h2, w2);
    const bool ok = covalid && v < P.Vb;
    obase[j] = ok ? ((((d2 * c.soD) * Ho + h2 * c.soH) * Wo + w2 * c.soW) * c.ocs + co) * 4 : (int)0x80000000;
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tg = tap0 + t;
    const int tw = tg % c.soW, th = (tg / c.soW) % c.soH, tdd = tg / (c.soW * c.soH);
    const int toff = ((tdd * Ho + th) * Wo + tw) * c.ocs * 4;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float val = acc[t][j] + bias;
      if (c.accumulate) val += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ro, obase[j], toff, 0));
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), ro, obase[j], toff, 0);
      if (c.stats_part != nullptr && obase[j] >= 0) { s1 += val; s2 = fmaf(val, val, s2); }
    }
  }
  }
  if (c.stats_part != nullptr) {
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    if (lhalf == 0) { red[(wave * 32 + li) * 2] = s1; red[(wave * 32 + li) * 2 + 1] = s2; }
    __syncthreads();
    if (tid < 32 && (ntile * 32 + tid) < c.Cout) {
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) { t1 += red[(w * 32 + tid) * 2]; t2 += red[(w * 32 + tid) * 2 + 1]; }
      float* sp = c.stats_part + ((size_t)((size_t)nb * P.nsb + sb) * c.Cout + ntile * 32 + tid) * 2;
      sp[0] = t1; sp[1] = t2;
    }
  }
}

// ---- 1x1x1 head with 33..64 output channels into a DENSE [V][Cout] tensor (the 47 MultiTalent logits, generic_UNet.py:349-351) ----
// pw_fast_kernel serves it with two workgroups per 128 voxels (channels 0-31 and 32-46): the input is read twice and every voxel's
// 188-byte row is written as a 128-byte and a 60-byte piece, neither aligned to anything (measured 1.8 TB/s).  Here one workgroup
// computes both channel tiles from one read of the input, transposes its 128 x Cout block through LDS and writes it as ONE linear run
// of 16-byte stores (128 * 47 * 4 = 24 064 contiguous bytes).  Requires V % 32 == 0, unit strides, no accumulation / statistics.
#define PWH_MAXCO 64
template <int XS = MT_F32, bool M16 = false>
__global__ __launch_bounds__(256) void pw_head_kernel(const PwKParams P) {
  constexpr int XE = mt_ebytes<XS>();
  const mt_pointwise_t& c = P.c;
  __shared__ __attribute__((aligned(16))) float ssc[PW_MAXC], ssh[PW_MAXC];
  __shared__ __attribute__((aligned(16))) float stage[4][32 * PWH_MAXCO];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  const int bx = mt_xcd_remap(blockIdx.x, gridDim.x);
  const int nb = bx / P.nsb, sb = bx % P.nsb;
  const long m0 = (long)sb * 128 + wave * 32;
  const mt_src_t& S = c.src;
  const bool wok = m0 < P.Vb;                              // (whole waves: V % 32 == 0)
  const size_t in_sample = (size_t)P.Vb * S.cs;
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)S.ptr + (size_t)nb * in_sample * XE), 0, (int)(in_sample * XE), 0x00020000);
  const int aoff = wok ? (int)(((m0 + li) * S.cs + 8 * lhalf) * XE) : (int)0x80000000;
  const bool aff = S.scale != nullptr;
  const float slope = S.slope;
  if (aff) {
    for (int i = tid; i < P.nchunks * PW_CK; i += 256) {
      ssc[i] = i < S.C ? S.scale[(size_t)nb * S.C + i] : 0.f;
      ssh[i] = i < S.C ? S.shift[(size_t)nb * S.C + i] : 0.f;
    }
    __syncthreads();
  }
  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[t][j] = 0.f;
  float xa[8], xn[8];
  auto load_a = [&](int ch, float (&x)[8]) { pw_load8<XS>(ra, aoff + ch * (PW_CK * XE), x); };
  load_a(0, xa);
  for (int ch = 0; ch < P.nchunks; ++ch) {
    if (ch + 1 < P.nchunks) load_a(ch + 1, xn);
    const int cb = ch * PW_CK + 8 * lhalf;
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = xa[e];
    if (aff) {
      const f32x4 sc0 = *(const f32x4*)(ssc + cb), sc1 = *(const f32x4*)(ssc + cb + 4);
      const f32x4 sh0 = *(const f32x4*)(ssh + cb), sh1 = *(const f32x4*)(ssh + cb + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float t = fmaf(x[e], e < 4 ? sc0[e & 3] : sc1[e & 3], e < 4 ? sh0[e & 3] : sh1[e & 3]);
        x[e] = mt_lrelu(t, slope);
      }
    }
    if (cb + 8 > c.Cin) {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = (cb + e < c.Cin) ? x[e] : 0.f;
    }
    if constexpr (M16) {
      typedef _Float16 pw_f16x8 __attribute__((ext_vector_type(8)));
      uint4 af;
      af.x = mt_pk16<MT_F16>(x[0], x[1]); af.y = mt_pk16<MT_F16>(x[2], x[3]); af.z = mt_pk16<MT_F16>(x[4], x[5]); af.w = mt_pk16<MT_F16>(x[6], x[7]);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const uint4 b = *(const uint4*)((const unsigned*)c.wpack + (size_t)(t * P.nchunks + ch) * 256 + lane * 4);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(pw_f16x8, af), __builtin_bit_cast(pw_f16x8, b), acc[t], 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) xa[e] = xn[e];
      continue;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float* wq = c.wpack + (size_t)(t * P.nchunks + ch) * 512 + lane * 4;
      const f32x4 b0 = *(const f32x4*)(wq);
      const f32x4 b1 = *(const f32x4*)(wq + 256);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[e], b0[e], acc[t], 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[4 + e], b1[e], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) xa[e] = xn[e];
  }
  // ---- epilogue: [32 voxels][Cout] of this wave through LDS, then a linear run of 16-byte stores
  float* sg = stage[wave];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int co = t * 32 + li;
    const float bias = (c.bias != nullptr && co < c.Cout) ? c.bias[co] : 0.f;
    if (co < c.Cout) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int iv = (j & 3) + 8 * (j >> 2) + 4 * lhalf;
        sg[iv * c.Cout + co] = acc[t][j] + bias;
      }
    }
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);                     // lgkmcnt(0): this wave's own LDS writes (no other wave touches stage[wave])
  __builtin_amdgcn_wave_barrier();
  if (wok) {
    const size_t out_sample = (size_t)P.Vb * c.Cout;
    __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)(c.out + (size_t)nb * out_sample), 0, (int)(out_sample * 4), 0x00020000);
    const int n4 = 8 * c.Cout;                             // float4 per wave block (32 * Cout / 4)
    const int obase = (int)(m0 * c.Cout * 4);
    for (int i = lane; i < n4; i += 64) {
      const f32x4 v = *(const f32x4*)(sg + 4 * i);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), ro, obase + i * 16, 0, 0);
    }
  }
}

// ---- narrow heads: 1x1x1 convolution to <= 4 output channels (the heads of the few-class single-dataset trainers: 2 logits for
// Task009) from a dense CIN-channel tensor.  The MFMA forms spend a 32-wide output tile on 2 channels and fetch their A fragments as
// 32-byte pieces of 120-byte rows (2.7 TB/s); here a thread owns a voxel: its row is one contiguous run (consecutive lanes = consecutive
// rows: the wave reads 7.5 KiB linearly), the lazy InstanceNorm+LeakyReLU and CIN x Cout multiply-adds run on the vector ALU
// (60 FMAs per 120 bytes: far below the bandwidth bound), W / scale / shift come from LDS as broadcast reads.
// a dense CIN-channel row (byte offset o) as 16-byte loads + tail; CIN % 2 == 0
template <int CIN, int XS>
__device__ __forceinline__ void pw_load_row(__amdgpu_buffer_rsrc_t r, int o, float (&x)[CIN + 2]) {
  if constexpr (XS == MT_F32) {
#pragma unroll
    for (int q = 0; q < CIN / 4; ++q) {
      const f32x4 t = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, o + q * 16, 0, 0));
      x[4 * q] = t[0]; x[4 * q + 1] = t[1]; x[4 * q + 2] = t[2]; x[4 * q + 3] = t[3];
    }
    if constexpr ((CIN % 4) != 0) {
      const float2 t = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(r, o + (CIN / 4) * 16, 0, 0));
      x[CIN - 2] = t.x; x[CIN - 1] = t.y;
    }
  } else {
    constexpr int ND = CIN / 2;            // dwords of the row
    unsigned d[ND + 3];
#pragma unroll
    for (int q = 0; q < ND / 4; ++q) {
      const uint4 t = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, o + q * 16, 0, 0));
      d[4 * q] = t.x; d[4 * q + 1] = t.y; d[4 * q + 2] = t.z; d[4 * q + 3] = t.w;
    }
#pragma unroll
    for (int q = (ND / 4) * 4; q < ND; ++q) d[q] = __builtin_amdgcn_raw_buffer_load_b32(r, o + q * 4, 0, 0);
#pragma unroll
    for (int q = 0; q < ND; ++q) { x[2 * q] = mt_lo16<XS>(d[q]); x[2 * q + 1] = mt_hi16<XS>(d[q]); }
  }
}
template <int CIN, int OS>
__device__ __forceinline__ void pw_store_row(__amdgpu_buffer_rsrc_t r, int o, const float (&x)[CIN + 2]) {
  if constexpr (OS == MT_F32) {
#pragma unroll
    for (int q = 0; q < CIN / 4; ++q) {
      f32x4 t; t[0] = x[4 * q]; t[1] = x[4 * q + 1]; t[2] = x[4 * q + 2]; t[3] = x[4 * q + 3];
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, t), r, o + q * 16, 0, 0);
    }
    if constexpr ((CIN % 4) != 0) {
      float2 t; t.x = x[CIN - 2]; t.y = x[CIN - 1];
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, t), r, o + (CIN / 4) * 16, 0, 0);
    }
  } else {
    constexpr int ND = CIN / 2;
    unsigned d[ND + 3];
#pragma unroll
    for (int q = 0; q < ND; ++q) d[q] = mt_pk16<OS>(x[2 * q], x[2 * q + 1]);
#pragma unroll
    for (int q = 0; q < ND / 4; ++q) {
      uint4 t; t.x = d[4 * q]; t.y = d[4 * q + 1]; t.z = d[4 * q + 2]; t.w = d[4 * q + 3];
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, t), r, o + q * 16, 0, 0);
    }
#pragma unroll
    for (int q = (ND / 4) * 4; q < ND; ++q) __builtin_amdgcn_raw_buffer_store_b32(d[q], r, o + q * 4, 0, 0);
  }
}
template <int CIN, int XS = MT_F32>
__global__ __launch_bounds__(256) void pw_narrow_kernel(const PwKParams P) {
  constexpr int XE = mt_ebytes<XS>();
  const mt_pointwise_t& c = P.c;
  __shared__ __attribute__((aligned(16))) float sw[4][CIN + 2], ssc[CIN + 2], ssh[CIN + 2];
  const int tid = threadIdx.x;
  const int nb = blockIdx.y;
  const mt_src_t& S = c.src;
  const bool aff = S.scale != nullptr;
  for (int i = tid; i < 4 * CIN; i += 256) {
    const int co = i / CIN, ci = i - co * CIN;
    // packed layout 1 (ck = 16): channel ci = 16 ch + 8 half + 4 q + e of output co sits at [ch][q][lane = 32 half + co][e]
    const int ch = ci >> 4, cl = ci & 15, half = cl >> 3, kp = cl & 7;
    sw[co][ci] = co < c.Cout ? c.wpack[(size_t)ch * 512 + ((kp >> 2) * 64 + half * 32 + co) * 4 + (kp & 3)] : 0.f;
  }
  for (int i = tid; i < CIN; i += 256) {
    ssc[i] = aff ? S.scale[(size_t)nb * S.C + i] : 1.f;
    ssh[i] = aff ? S.shift[(size_t)nb * S.C + i] : 0.f;
  }
  __syncthreads();
  const float slope = aff ? S.slope : 1.f;
  float bias[4];
#pragma unroll
  for (int co = 0; co < 4; ++co) bias[co] = (c.bias != nullptr && co < c.Cout) ? c.bias[co] : 0.f;
  const size_t in_sample = (size_t)P.Vb * CIN;
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)S.ptr + (size_t)nb * in_sample * XE), 0, (int)(in_sample * XE), 0x00020000);
  float* outp = c.out + (size_t)nb * P.Vb * c.Cout;
  for (long v = (long)blockIdx.x * 256 + tid; v < P.Vb; v += (long)gridDim.x * 256) {
    float x[CIN + 2];
    pw_load_row<CIN, XS>(ra, (int)(v * (CIN * XE)), x);
    float y[4] = {bias[0], bias[1], bias[2], bias[3]};
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) {
      const float t = fmaf(x[ci], ssc[ci], ssh[ci]);
      const float a = fmaxf(t, t * slope);                   // LeakyReLU for slope in [0, 1]
#pragma unroll
      for (int co = 0; co < 4; ++co) y[co] = fmaf(a, sw[co][ci], y[co]);
    }
    float* q = outp + v * c.Cout;
#pragma unroll
    for (int co = 0; co < 4; ++co)
      if (co < c.Cout) q[co] = y[co];
  }
}

// ---- dispatch: ONE decision per problem (pw_resolve).  The launch, the kernel name, the launch shape and the pack layout read it;
// the eligibility predicates below are called from pw_resolve only.
extern "C" int mt_pointwise_stats_blocks(const mt_pointwise_t* p) {
  if (p == nullptr) return -1;
  return mt_cdiv((long)p->Db * p->Hb * p->Wb, 128);
}
// Storage types mt_pointwise_fwd takes natively (mt_pointwise_t.src.dtype -> odtype): fp32 -> fp32 always; a 16-bit source needs an even
// channel stride and a dword-aligned base (its 8-channel groups are 16-byte loads on dword boundaries), a 16-bit destination even Cout /
// channel stride and a dword-aligned base (channel-pair dwords).  Combinations: fp16 -> fp16 | fp32 (forward over activations),
// bf16 -> bf16 | fp32 and fp32 -> bf16 (backward-data over gradients).
extern "C" int mt_pointwise_io_supported(const mt_pointwise_t* p) {
  if (p == nullptr) return 0;
  const int xs = p->src.dtype, os = p->odtype;
  if (!mt_dtype_ok(xs) || !mt_dtype_ok(os)) return 0;
  if (xs == MT_F32 && os == MT_F32) return 1;
  if (mt_is16(xs) && ((p->src.cs & 1) || (((uintptr_t)p->src.ptr) & 3))) return 0;
  if (mt_is16(os) && ((p->Cout & 1) || (p->ocs & 1) || (((uintptr_t)p->out) & 3))) return 0;
  if (xs == MT_F16) return os == MT_F16 || os == MT_F32;
  if (xs == MT_BF16) return os == MT_BF16 || os == MT_F32;
  return os == MT_BF16;                       // fp32 source (the loss gradient) into a bf16 gradient
}
// the narrow form (pw_narrow_kernel): 1x1x1, unit strides, <= 4 output channels from a dense 30- or 32-channel tensor
static bool pw_narrow_ok(const mt_pointwise_t* p, const PwKParams& P) {
  return P.ntaps == 1 && p->soD * p->soH * p->soW == 1 && p->siD == 1 && p->siH == 1 && p->siW == 1 && p->Cout <= 4 && (p->Cin == 30 || p->Cin == 32) && p->src.cs == p->Cin &&
         p->ocs == p->Cout && !p->accumulate && p->stats_part == nullptr && p->Di == p->Db && p->Hi == p->Hb && p->Wi == p->Wb &&
         (p->src.slope >= 0.f && p->src.slope <= 1.f) && ((((uintptr_t)p->out) & 15) == 0);
}
// the dense-output head form (pw_head_kernel): 1x1x1, unit strides, 33..64 output channels written densely, whole waves of voxels
static bool pw_head_ok(const mt_pointwise_t* p, const PwKParams& P) {
  return P.ntaps == 1 && p->soD * p->soH * p->soW == 1 && p->siD == 1 && p->siH == 1 && p->siW == 1 && p->Cout > 32 && p->Cout <= PWH_MAXCO && p->ocs == p->Cout &&
         !p->accumulate && p->stats_part == nullptr && (P.Vb % 32) == 0 && p->Di == p->Db && p->Hi == p->Hb && p->Wi == p->Wb &&
         ((((uintptr_t)p->out) & 15) == 0) && ((P.Vb * p->Cout) % 4 == 0);
}
// 16-bit products (mt_pointwise_t.mma == 1): fp16 source; pw_head_kernel (fp32 logits) or pw_fast_kernel writing fp16 (transposed convs)
static bool pw_m16(const mt_pointwise_t* p, const PwKParams& P, bool head) {
  if (p->mma != 1 || p->src.dtype != MT_F16 || p->scatter) return false;
  if ((p->src.cs & 1) || (((uintptr_t)p->src.ptr) & 3)) return false;
  return head ? true : (p->odtype == MT_F16 && P.ntaps >= 2);
}
enum PwFamily { PW_FAST = 0, PW_HEAD, PW_NARROW };
struct PwChoice {
  PwFamily family;
  int nt;            // pw_fast_kernel: taps per workgroup (eight taps without statistics run as 4 with grid.z = 2); pw_narrow_kernel: CIN
  int xs, os;        // storage types of the source and the destination
  bool m16;          // fp16 products: the weights are in pack layout 4
  dim3 grid;
  PwKParams P;       // P.wide: the store form of pw_fast_kernel
};
// The decision is pure arithmetic on the descriptor and comes first; the requirements on the problem follow in the order the launch
// always checked them, so that mt_pointwise_pack_layout keeps answering for a problem the launch refuses.  `require` = false is that
// query's path: the decision alone, no requirement checked and the library's last-error text left as it is.
static int pw_resolve(const mt_pointwise_t* p, PwChoice& c, bool require = true) {
  c.m16 = false;
  if (!require && (p == nullptr || !mt_pointwise_io_supported(p))) return MT_EINVAL;
  MT_REQUIRE(p != nullptr, "pointwise: null params");
  MT_REQUIRE(mt_pointwise_io_supported(p), "pointwise: storage types (src %d, out %d) not taken (ask mt_pointwise_io_supported, convert with mt_cast)", p->src.dtype, p->odtype);
  PwKParams& P = c.P;
  P.c = *p;
  P.ntaps = p->scatter ? 1 : p->soD * p->soH * p->soW;       // scatter: only tap (0,0,0) exists (one packed tap)
  P.nchunks = mt_cdiv(p->Cin, PW_CK);
  P.Vb = (long)p->Db * p->Hb * p->Wb;
  P.nsb = mt_cdiv(P.Vb, 128);
  {
    const bool shape_ok = P.ntaps >= 4 && p->soW == 2 && p->soH == 2 && (p->Wb % 32) == 0 && p->Cout <= 32 && (p->Cout % 2) == 0 &&
                          !p->accumulate && p->stats_part == nullptr && p->siD == 1 && p->siH == 1 && p->siW == 1;
    P.wide = 0;
    if (shape_ok && p->ocs == p->Cout && ((((uintptr_t)p->out) & 7) == 0)) P.wide = 2;                       // dense output: linear 8-byte (fp32) / 4-byte (16-bit) stores
    else if (shape_ok && (p->ocs % 4) == 0 && ((((uintptr_t)p->out) & 15) == 0)) P.wide = 1;                 // concat slot: 16 / 8-byte pieces per voxel
  }
  c.xs = p->src.dtype; c.os = p->odtype;
  if (c.os == MT_F32 && pw_narrow_ok(p, P)) {
    long blocks = (P.Vb + 255) / 256; if (blocks > 4096) blocks = 4096;
    c.family = PW_NARROW; c.nt = p->Cin; c.grid = dim3((unsigned)blocks, (unsigned)p->N);
  } else if (c.os == MT_F32 && pw_head_ok(p, P)) {
    c.family = PW_HEAD; c.nt = 1; c.grid = dim3((unsigned)(P.nsb * p->N));
    c.m16 = pw_m16(p, P, true);
  } else {
    // the source is read with 16-byte loads whatever its alignment: a raw buffer_load_dwordx4 only needs dword alignment and
    // range-checks per dword (tools/ubench/oob128.hip, verified on the device by mt_probe_device)
    c.family = PW_FAST;
    const bool split8 = P.ntaps == 8 && p->stats_part == nullptr;      // two workgroups of four taps (see pw_fast_kernel)
    c.nt = split8 ? 4 : P.ntaps;
    c.grid = dim3((unsigned)(P.nsb * p->N), (unsigned)mt_cdiv(p->Cout, 32), split8 ? 2 : 1);
    c.m16 = pw_m16(p, P, false);
  }
  if (!require) return MT_OK;
  MT_REQUIRE(p->N > 0 && p->Db > 0 && p->Hb > 0 && p->Wb > 0 && p->Cin > 0 && p->Cout > 0, "pointwise: empty problem");
  MT_REQUIRE(p->siD >= 1 && p->siD <= 2 && p->siH >= 1 && p->siH <= 2 && p->siW >= 1 && p->siW <= 2, "pointwise: input stride must be 1 or 2");
  MT_REQUIRE(p->soD >= 1 && p->soD <= 2 && p->soH >= 1 && p->soH <= 2 && p->soW >= 1 && p->soW <= 2, "pointwise: output stride must be 1 or 2");
  MT_REQUIRE((p->Db - 1) * p->siD < p->Di && (p->Hb - 1) * p->siH < p->Hi && (p->Wb - 1) * p->siW < p->Wi, "pointwise: base grid exceeds stored input");
  MT_REQUIRE(p->src.C == p->Cin, "pointwise: src.C != Cin");
  MT_REQUIRE(p->src.ptr && p->wpack && p->out, "pointwise: null pointers");
  MT_REQUIRE((double)p->Di * p->Hi * p->Wi * p->src.cs * 4.0 < 2147483648.0 &&
             (double)P.Vb * (p->soD * p->soH * p->soW) * p->ocs * 4.0 < 2147483648.0, "pointwise: sample larger than 2 GiB");
  MT_REQUIRE(P.ntaps == 1 || P.ntaps == 2 || P.ntaps == 4 || P.ntaps == 8, "pointwise: unsupported tap count %d", P.ntaps);
  MT_REQUIRE(P.nchunks * PW_CK <= PW_MAXC, "pointwise: Cin = %d exceeds %d", p->Cin, PW_MAXC);
  return MT_OK;
}
// pack layout 1 where the launch refuses the storage types (the caller converts with mt_cast and asks again)
extern "C" int mt_pointwise_pack_layout(const mt_pointwise_t* p) {
  PwChoice c;
  pw_resolve(p, c, false);
  return c.m16 ? 4 : 1;
}
extern "C" int mt_pointwise_kernel_name(const mt_pointwise_t* p, char* buf, size_t n) {
  MT_REQUIRE(buf != nullptr && n > 0, "pointwise_kernel_name: no buffer");
  PwChoice c;
  if (int rc = pw_resolve(p, c)) return rc;
  if (c.family == PW_NARROW) snprintf(buf, n, "pw_narrow_kernel<%d, %d>", c.nt, c.xs);
  else if (c.family == PW_HEAD) snprintf(buf, n, "pw_head_kernel<%d, %s>", c.xs, c.m16 ? "true" : "false");
  else snprintf(buf, n, "pw_fast_kernel<%d, %d, %d, %s>", c.nt, c.xs, c.os, c.m16 ? "true" : "false");
  return MT_OK;
}
extern "C" int mt_pointwise_launch_shape(const mt_pointwise_t* p, int32_t shape[4]) {
  MT_REQUIRE(shape != nullptr, "pointwise_launch_shape: no output");
  PwChoice c;
  if (int rc = pw_resolve(p, c)) return rc;
  shape[0] = (int32_t)c.grid.x; shape[1] = (int32_t)c.grid.y; shape[2] = (int32_t)c.grid.z; shape[3] = c.P.wide;
  return MT_OK;
}

#define PW_FAST(NT_, XS_, OS_, M16_) hipLaunchKernelGGL((pw_fast_kernel<NT_, XS_, OS_, M16_>), c.grid, dim3(256), 0, st, c.P)
template <int NT>
static void pw_launch_fast(const PwChoice& c, hipStream_t st) {
  if constexpr (NT >= 2) {
    if (c.m16) { PW_FAST(NT, MT_F16, MT_F16, true); return; }
  }
  if (c.xs == MT_F16 && c.os == MT_F16) PW_FAST(NT, MT_F16, MT_F16, false);
  else if (c.xs == MT_F16) PW_FAST(NT, MT_F16, MT_F32, false);
  else if (c.xs == MT_BF16 && c.os == MT_BF16) PW_FAST(NT, MT_BF16, MT_BF16, false);
  else if (c.xs == MT_BF16) PW_FAST(NT, MT_BF16, MT_F32, false);
  else if (c.os == MT_BF16) PW_FAST(NT, MT_F32, MT_BF16, false);
  else PW_FAST(NT, MT_F32, MT_F32, false);
}
#undef PW_FAST
template <int CIN>
static void pw_launch_narrow(const PwChoice& c, hipStream_t st) {
  if (c.xs == MT_F16) hipLaunchKernelGGL((pw_narrow_kernel<CIN, MT_F16>), c.grid, dim3(256), 0, st, c.P);
  else if (c.xs == MT_BF16) hipLaunchKernelGGL((pw_narrow_kernel<CIN, MT_BF16>), c.grid, dim3(256), 0, st, c.P);
  else hipLaunchKernelGGL((pw_narrow_kernel<CIN, MT_F32>), c.grid, dim3(256), 0, st, c.P);
}
extern "C" int mt_pointwise_fwd(const mt_pointwise_t* p, mt_stream_t stream) {
  PwChoice c;
  if (int rc = pw_resolve(p, c)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (c.family == PW_NARROW) {
    if (c.nt == 30) pw_launch_narrow<30>(c, st); else pw_launch_narrow<32>(c, st);
    MT_CHECK_LAUNCH("pointwise_narrow");
  } else if (c.family == PW_HEAD) {
    if (c.m16) hipLaunchKernelGGL((pw_head_kernel<MT_F16, true>), c.grid, dim3(256), 0, st, c.P);
    else if (c.xs == MT_F16) hipLaunchKernelGGL((pw_head_kernel<MT_F16>), c.grid, dim3(256), 0, st, c.P);
    else if (c.xs == MT_BF16) hipLaunchKernelGGL((pw_head_kernel<MT_BF16>), c.grid, dim3(256), 0, st, c.P);
    else hipLaunchKernelGGL((pw_head_kernel<MT_F32>), c.grid, dim3(256), 0, st, c.P);
    MT_CHECK_LAUNCH("pointwise_head");
  } else {
    switch (c.nt) {
      case 1: pw_launch_fast<1>(c, st); break;
      case 2: pw_launch_fast<2>(c, st); break;
      case 4: pw_launch_fast<4>(c, st); break;
      default: pw_launch_fast<8>(c, st); break;
    }
    MT_CHECK_LAUNCH("pointwise");
  }
  return MT_OK;
}
