// conv_stage.h — input-tile staging shared by the convolution units: conv_lds.hip (forward / backward-data) and conv_bwdw.hip
// (backward-weight) stage the same haloed X tile into LDS, with InstanceNorm + LeakyReLU applied on load.
#pragma once
#include "mt_common.h"
#include "bwdw_common.h"

// ------------------------------------------------------------------------------------------------
// Input-tile staging shared by forward and backward-weight kernels.
// Tile origin (ud0,uh0,uw0) in VIRTUAL input coordinates, extent LD x LH x LW, channel slots CK.
// Each wave owns rows wave, wave+4, ... of the (LD*LH)-row tile; a row is walked in steps of VPS = 64/CK
// voxels x CK channels (64 lanes = CK contiguous channels of VPS consecutive voxels).  Lean addressing:
// global address = wave-uniform row base + per-lane constant + step * (VPS*cs); LDS address likewise, so a
// staged element costs ~1 load, a bounds select, the fused InstanceNorm+LeakyReLU and 1 ds_write.
// Two rows x STAGE_NI steps are issued back-to-back before the LDS stores (deep memory-level parallelism).
// LDS image: voxel lv (linear index in the LD x LH x LW tile) x CK channel slots, channel c stored at slot
// c ^ ((lv >> 1) & (CK-1)): with an even CK-dword voxel stride this XOR swizzle makes the A-fragment reads
// (32 consecutive voxels, one channel) bank-conflict free WITHOUT padding the voxel stride, which is what lets
// three 52 KiB workgroups share a CU's 160 KiB LDS.
#define STAGE_NI 9
__device__ __forceinline__ int mt_swz(int lv, int c, int ckmask) { return c ^ ((lv >> 1) & ckmask); }
template <int CK>
__device__ __forceinline__ void mt_stage_input(float* __restrict__ lds, const mt_conv3d_t& c,
                                               const ConvChunk ch, int nb, int ud0, int uh0, int uw0,
                                               int LD, int LH, int LW, int lane, int wave) {
  constexpr int VPS = 64 / CK;  // voxels per 64-lane step
  const mt_src_t& S = c.src[ch.src];
  const int cl = lane % CK, vl = lane / CK;
  const bool cvalid = cl < ch.ck;
  const bool has_aff = S.scale != nullptr;
  float sc = 1.f, sh = 0.f;
  if (has_aff && cvalid) {
    sc = S.scale[(size_t)nb * S.C + ch.c0 + cl];
    sh = S.shift[(size_t)nb * S.C + ch.c0 + cl];
  }
  const float slope = S.slope;
  const int nrows = LD * LH;
  const int NI = (LW + VPS - 1) / VPS;
  const int dilW = c.dilW;
  // per-lane constants: first virtual w of this lane, its stored-w offset (elements) and LDS offset
  const int uwl = uw0 + vl;
  const float* lanep = S.ptr + ch.c0 + cl;
  const int cs = S.cs;
  for (int row0 = wave; row0 < nrows; row0 += 8) {
    for (int i0 = 0; i0 < NI; i0 += STAGE_NI) {
      float v[2][STAGE_NI];
      bool okv[2][STAGE_NI];
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const int row = row0 + 4 * rr;
        const int ld = row / LH, lhh = row - ld * LH;
        const int ud = ud0 + ld, uh = uh0 + lhh;
        int sd = ud, shh = uh;
        bool rvalid = (row < nrows) && (ud >= 0) && (uh >= 0);
        if (c.dilD == 2) { rvalid = rvalid && !(ud & 1); sd = ud >> 1; }
        if (c.dilH == 2) { rvalid = rvalid && !(uh & 1); shh = uh >> 1; }
        rvalid = rvalid && (sd < c.Di) && (shh < c.Hi) && cvalid;
        const float* rowp = lanep + ((size_t)((size_t)nb * c.Di + sd) * c.Hi + shh) * c.Wi * cs;  // wave-uniform part + lane const
#pragma unroll
        for (int u = 0; u < STAGE_NI; ++u) {
          const int i = i0 + u;
          const int lw = i * VPS + vl;
          const int uw = uwl + i * VPS;
          int sw = uw;
          bool ok = rvalid && (i < NI) && (lw < LW) && (uw >= 0);
          if (dilW == 2) { ok = ok && !(uw & 1); sw = uw >> 1; }
          ok = ok && (sw < c.Wi);
          float x = 0.f;
          if (ok) x = rowp[(long)sw * cs];
          v[rr][u] = x;
          okv[rr][u] = ok;
        }
      }
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const int row = row0 + 4 * rr;
        if (row < nrows) {
          const int lv0 = row * LW + vl;
#pragma unroll
          for (int u = 0; u < STAGE_NI; ++u) {
            const int i = i0 + u;
            const int lw = i * VPS + vl;
            if (i < NI && lw < LW) {
              float x = v[rr][u];
              if (has_aff && okv[rr][u]) x = mt_lrelu(fmaf(x, sc, sh), slope);
              const int lv = lv0 + i * VPS;
              lds[lv * CK + mt_swz(lv, cl, CK - 1)] = x;
            }
          }
        }
      }
    }
  }
}

// LDS image of the lean staging: 16 channel slots per voxel, padded to a pitch of 20 dwords (see conv_fast_kernel in conv_lds.hip)
#define FCK 16
#define FCKP 20
// LDS rows are padded to a multiple of 4 (stage_rows) so that every wave stores the same number of rows; a row is padded to whole
// staging steps where that still fits 80 KiB (stage_lwp)
template <int VEC> __host__ __device__ constexpr int stage_vps() { return 64 / (FCK / VEC); }
template <int LD, int LH> __host__ __device__ constexpr int stage_rows() { return ((LD * LH + 3) / 4) * 4; }
template <int LD, int LH, int LW, int VEC> __host__ __device__ constexpr int stage_lwp() {
  constexpr int padded = ((LW + stage_vps<VEC>() - 1) / stage_vps<VEC>()) * stage_vps<VEC>();
  return ((size_t)stage_rows<LD, LH>() * padded * FCKP * 4 <= 80 * 1024) ? padded : LW;
}
template <int LD, int LH, int LW, int VEC> __host__ __device__ constexpr size_t stage_lds_bytes() {
  return (size_t)stage_rows<LD, LH>() * stage_lwp<LD, LH, LW, VEC>() * FCKP * sizeof(float);
}

// ------------------------------------------------------------------------------------------------
// Split form of mt_stage_fast2 for software pipelining across tiles: stage2_load issues all global loads of a wave's
// share of the tile into registers (no wait), stage2_store applies InstanceNorm+LeakyReLU and writes LDS later.
template <int LD, int LH, int LW, int VEC>
struct Stage2Regs {
  static constexpr int LPV = FCK / VEC, VPS = 64 / LPV, NI = (LW + VPS - 1) / VPS, R = LD * LH, RPW = (R + 3) / 4;
  float v[RPW][NI][VEC];
  int voff[NI];
  unsigned rvmask;     // bit r: row r of this wave is inside the volume
  int nb;
  bool nosel;
};

// XS: storage type of the source.  A 16-bit source (VEC == 2 only) leaves the RAW dword — two elements — in v[r][i][0]; stage2_store
// widens it (a conversion right behind the load would put a wait between the loads and drain the prefetch).
template <int LD, int LH, int LW, int VEC, int XS = MT_F32>
__device__ __forceinline__ void stage2_load(Stage2Regs<LD, LH, LW, VEC>& g, const mt_conv3d_t& c, const ConvChunk ch, int nb,
                                            int ud0, int uh0, int uw0, int lane, int wave) {
  typedef Stage2Regs<LD, LH, LW, VEC> RG_;
  constexpr int LPV = RG_::LPV, VPS = RG_::VPS, NI = RG_::NI, R = RG_::R, RPW = RG_::RPW;
  constexpr int XE = mt_ebytes<XS>();
  static_assert(XS == MT_F32 || VEC == 2, "16-bit sources are staged as channel pairs");
  const mt_src_t& S = c.src[ch.src];
  const int cl = (lane % LPV) * VEC, vl = lane / LPV;
  const bool cval0 = cl < ch.ck;
  const int cs = S.cs;
  const size_t sample_elems = (size_t)c.Di * c.Hi * c.Wi * cs;
  __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)S.ptr + (size_t)nb * sample_elems * XE), 0, (int)(sample_elems * XE), 0x00020000);
  g.nb = nb;
  g.nosel = (ud0 >= 0) && (uh0 >= 0) && (uw0 >= 0) && (ud0 + LD <= c.Di) && (uh0 + LH <= c.Hi) && (uw0 + LW <= c.Wi) &&
            (S.slope >= 0.f) && (S.slope <= 1.f);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int lw = vl + i * VPS;
    const int uw = uw0 + lw;
    const bool ok = cval0 && (lw < LW) && ((unsigned)uw < (unsigned)c.Wi);
    g.voff[i] = ok ? (uw * cs + ch.c0 + cl) * XE : (int)0x80000000;
  }
  g.rvmask = 0;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int row = wave + 4 * r;
    const int ld = row / LH, lhh = row % LH;
    const int ud = ud0 + ld, uh = uh0 + lhh;
    const bool rv = (row < R) && ((unsigned)ud < (unsigned)c.Di) && ((unsigned)uh < (unsigned)c.Hi);
    if (rv) {
      g.rvmask |= 1u << r;
      const int srow = (ud * c.Hi + uh) * c.Wi * cs * XE;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        if constexpr (XS != MT_F32) {
          g.v[r][i][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, g.voff[i] + srow, 0, 0));
          g.v[r][i][1] = 0.f;
        } else if constexpr (VEC == 2) {
          const float2 t = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, g.voff[i] + srow, 0, 0));
          g.v[r][i][0] = t.x; g.v[r][i][1] = t.y;
        } else {
          g.v[r][i][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, g.voff[i] + srow, 0, 0));
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int e = 0; e < VEC; ++e) g.v[r][i][e] = 0.f;
    }
  }
}

template <int LD, int LH, int LW, int VEC, int PITCH = FCKP, int XS = MT_F32>
__device__ __forceinline__ void stage2_store(const Stage2Regs<LD, LH, LW, VEC>& g, float* __restrict__ lds, const mt_conv3d_t& c,
                                             const ConvChunk ch, int lane, int wave) {
  typedef Stage2Regs<LD, LH, LW, VEC> RG_;
  constexpr int LPV = RG_::LPV, VPS = RG_::VPS, NI = RG_::NI, R = RG_::R, RPW = RG_::RPW;
  const mt_src_t& S = c.src[ch.src];
  const int cl = (lane % LPV) * VEC, vl = lane / LPV;
  const bool has_aff = S.scale != nullptr;
  float sc[VEC], sh[VEC];
  bool cval[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    cval[e] = (cl + e) < ch.ck;
    sc[e] = 1.f; sh[e] = 0.f;
    if (has_aff && cval[e]) {
      sc[e] = S.scale[(size_t)g.nb * S.C + ch.c0 + cl + e];
      sh[e] = S.shift[(size_t)g.nb * S.C + ch.c0 + cl + e];
    }
  }
  const float slope = S.slope;
  float* lbase = lds + vl * PITCH + cl + wave * (LW * PITCH);
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int row = wave + 4 * r;
    if (row < R) {
      const bool rv = (g.rvmask >> r) & 1u;
      float* lrow = lbase + 4 * r * (LW * PITCH);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int lw = vl + i * VPS;
        if ((i + 1) * VPS <= LW || lw < LW) {
          float x[VEC];
          const bool ok = rv && g.voff[i] >= 0;
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            if constexpr (XS != MT_F32) { const unsigned raw = __builtin_bit_cast(unsigned, g.v[r][i][0]); x[e] = e ? mt_hi16<XS>(raw) : mt_lo16<XS>(raw); }
            else x[e] = g.v[r][i][e];
            if (has_aff) {
              const float t = fmaf(x[e], sc[e], sh[e]);
              const float a = mt_lrelu(t, slope);          // any slope: the backward-weight dispatch does not restrict it
              x[e] = g.nosel ? a : ((ok && cval[e]) ? a : 0.f);
            } else if (VEC == 2 && e == 1) x[e] = cval[e] ? x[e] : 0.f;
          }
          if constexpr (VEC == 2) {
            float2 t; t.x = x[0]; t.y = x[1];
            *(float2*)(lrow + i * VPS * PITCH) = t;
          } else {
            lrow[i * VPS * PITCH] = x[0];
          }
        }
      }
    }
  }
}

// Stem kernels (one input channel): the haloed (TD + 2) x (TH + 2) x (TW + 2) tile as a scalar LDS image, activated on load
template <int TD, int TH, int TW>
__device__ __forceinline__ void stem_stage(float* __restrict__ xs, const mt_conv3d_t& c, int nb, int od0, int oh0, int ow0, int tid) {
  constexpr int LD = TD + 2, LH = TH + 2, LW = TW + 2;
  const mt_src_t& S = c.src[0];
  const bool aff = S.scale != nullptr;
  const float sc = aff ? S.scale[(size_t)nb * S.C] : 1.f, sh = aff ? S.shift[(size_t)nb * S.C] : 0.f;
  const float slope = aff ? S.slope : 1.f;
  for (int e = tid; e < LD * LH * LW; e += 256) {
    const int lw = e % LW, lh = (e / LW) % LH, ld = e / (LW * LH);
    const int ud = od0 - 1 + ld, uh = oh0 - 1 + lh, uw = ow0 - 1 + lw;
    float x = 0.f;
    if ((unsigned)ud < (unsigned)c.Di && (unsigned)uh < (unsigned)c.Hi && (unsigned)uw < (unsigned)c.Wi) {
      x = S.ptr[((size_t)((size_t)((size_t)nb * c.Di + ud) * c.Hi + uh) * c.Wi + uw) * S.cs];
      x = mt_lrelu(fmaf(x, sc, sh), slope);
    }
    xs[e] = x;
  }
}
