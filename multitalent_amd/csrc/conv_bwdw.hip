// conv_bwdw.hip — backward-weight of the 3D convolutions on gfx950, NDHWC (replaces the autograd backward-weight of nn.Conv3d /
// nn.ConvTranspose3d on the hot path of the reference).
//
// This unit holds the backward-weight kernel families (conv_bwdw_kernel, conv_bwdw_fast_kernel, conv_bwdw_march_kernel,
// conv_bwdw_stem_kernel here; the Winograd, im2col + GEMM and 16-bit families in bwdw_wino.inc / bwdw_gemm.inc / bwdw_fast16.inc;
// conv_bwdw_tr16_kernel is its own unit, bwdw_tr16.hip), bwdw_reduce_kernel, their plans and launchers, and the four extern "C"
// entry points.  Which family serves a problem is decided ONCE, in bwdw_resolve; the kernel name, io_supported and the launch all
// read that one choice.  The X staging shared with the forward kernels is conv_stage.h.
#include "mt_common.h"
#include "bwdw_common.h"
#include "conv_stage.h"
#include "conv16_common.h"
#include <cstring>
#include <stdlib.h>
#include <type_traits>

// ------------------------------------------------------------------------------------------------
// Backward-weight:  dW[tap][ci][co] = sum_{n,o} X[n, o*S + t - P, ci] * Y[n, o, co]
// v_mfma_f32_16x16x4_f32: M = 16 input channels (one chunk), N = 16 output channels, K = 4 voxels.
// A workgroup owns (ci chunk, 32 couts) and walks a strided list of spatial tiles, keeping all taps'
// accumulators in registers (taps are dealt round-robin to the 4 waves); it writes ONE partial per
// workgroup, reduced deterministically by bwdw_reduce_kernel straight into the torch weight layout.

#ifndef BW_ABL
#define BW_ABL 0   // compile-time timing ablations of the fast backward-weight kernel: 1 skip X staging, 2 skip Y, 8 skip MFMA
#endif
#define BW_YP 48
#define BW_MAXT 7
#define BW_YU 16

// MFMA phase of one backward-weight tile: K = voxels (4 per v_mfma_f32_16x16x4_f32), NT taps of this wave x
// 2 halves of 16 couts; operands of k-step i+1 are fetched from LDS while the MFMAs of k-step i issue.
struct BwdwWalk { int wsteps, TH, dx_w, dx_h, dx_d, nsteps; };

template <int NT>
__device__ __forceinline__ void bwdw_tile_compute(const float* __restrict__ xl, const float* __restrict__ yl,
                                                  const int (&tapoff)[BW_MAXT], int xb, int yb, const BwdwWalk wk,
                                                  int li, f32x4 (&acc)[BW_MAXT][2]) {
  float acur[NT], anxt[NT], b0c, b1c, b0n, b1n;
  auto xaddr = [&](int lv) { return lv * BW_CK + (li ^ ((lv >> 1) & (BW_CK - 1))); };   // swizzled X tile (see mt_swz)
#pragma unroll
  for (int t = 0; t < NT; ++t) acur[t] = xl[xaddr(xb + tapoff[t])];
  b0c = yl[yb]; b1c = yl[yb + 16];
  int ws = 0, hs = 0;
  for (int st = 0; st < wk.nsteps; ++st) {
    int xn = xb, yn = yb;
    if (st + 1 < wk.nsteps) {
      xn += wk.dx_w; yn += 4 * BW_YP;
      if (++ws == wk.wsteps) { ws = 0; xn += wk.dx_h; if (++hs == wk.TH) { hs = 0; xn += wk.dx_d; } }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) anxt[t] = xl[xaddr(xn + tapoff[t])];
    b0n = yl[yn]; b1n = yl[yn + 16];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(acur[t], b0c, acc[t][0], 0, 0, 0);
      acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(acur[t], b1c, acc[t][1], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) acur[t] = anxt[t];
    b0c = b0n; b1c = b1n;
    xb = xn; yb = yn;
  }
}

__global__ __launch_bounds__(256) void conv_bwdw_kernel(const BwdWParams P) {
  constexpr int CK = BW_CK, YP = BW_YP;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int sg = blockIdx.x, cot = blockIdx.y, chi = blockIdx.z;
  const ConvChunk cc = P.chunk[chi];
  const int TD = P.TD, TH = P.TH, TW = P.TW, TV = TD * TH * TW;
  const int LD = (TD - 1) * c.SD + c.KD, LH = (TH - 1) * c.SH + c.KH, LW = (TW - 1) * c.SW + c.KW;
  float* xl = lds;
  float* yl = lds + (size_t)LD * LH * LW * CK;

  // taps handled by this wave: wave, wave+4, ...
  int tapoff[BW_MAXT];
  int mytaps = 0;
#pragma unroll
  for (int t = 0; t < BW_MAXT; ++t) {
    const int tap = wave + 4 * t;
    tapoff[t] = 0;
    if (tap < P.ntaps) {
      const int kw = tap % c.KW, kh = (tap / c.KW) % c.KH, kd = tap / (c.KW * c.KH);
      tapoff[t] = (kd * LH + kh) * LW + kw;   // in voxels
      mytaps = t + 1;
    }
  }
  f32x4 acc[BW_MAXT][2];
#pragma unroll
  for (int t = 0; t < BW_MAXT; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t][h][j] = 0.f;

  const mt_src_t& Y = P.y;
  for (int tile = sg; tile < P.ntiles_total; tile += P.nsg) {
    int r = tile;
    const int tw = r % P.tilesW; r /= P.tilesW;
    const int th = r % P.tilesH; r /= P.tilesH;
    const int td = r % P.tilesD;
    const int nb = r / P.tilesD;
    const int od0 = td * TD, oh0 = th * TH, ow0 = tw * TW;
    __syncthreads();
    mt_stage_input<CK>(xl, c, cc, nb, od0 * c.SD - c.PD, oh0 * c.SH - c.PH, ow0 * c.SW - c.PW, LD, LH, LW, lane, wave);
    // stage Y tile: [TV][32 couts]; thread = (co = tid&31, voxel lane tid>>5), 8 voxels of a row per pass,
    // BW_YU loads in flight before the LDS stores
    {
      const int col = tid & 31, wv = tid >> 5;
      const int co = cot * 32 + col;
      const bool cok = co < c.Cout;
      float ysc = 1.f, ysh = 0.f;
      const bool yaff = Y.scale != nullptr;
      if (yaff && cok) { ysc = Y.scale[(size_t)nb * Y.C + co]; ysh = Y.shift[(size_t)nb * Y.C + co]; }
      const int nrowsY = TD * TH, NP = (TW + 7) >> 3;
      int rowy = 0, pass = 0;
      while (rowy < nrowsY) {
        float yv[BW_YU];
        int yo[BW_YU];
#pragma unroll
        for (int u = 0; u < BW_YU; ++u) {
          yo[u] = -1;
          if (rowy < nrowsY) {
            const int d = rowy / TH, h = rowy - d * TH;
            const int w = pass * 8 + wv;
            const int od = od0 + d, oh = oh0 + h, ow = ow0 + w;
            const bool ok = cok && (w < TW) && od < c.Do && oh < c.Ho && ow < c.Wo;
            float x = 0.f;
            if (ok) x = Y.ptr[((size_t)((size_t)((size_t)nb * c.Do + od) * c.Ho + oh) * c.Wo + ow) * Y.cs + co];
            yv[u] = x;
            if (w < TW) yo[u] = ((rowy * TW + w) * YP + col) | (ok ? 0x40000000 : 0);
            if (++pass == NP) { pass = 0; ++rowy; }
          }
        }
#pragma unroll
        for (int u = 0; u < BW_YU; ++u) {
          if (yo[u] >= 0) {
            float x = yv[u];
            if (yaff && (yo[u] & 0x40000000)) x = mt_lrelu(fmaf(x, ysc, ysh), Y.slope);
            yl[yo[u] & 0x3fffffff] = x;
          }
        }
      }
    }
    __syncthreads();
    {
      const int xb0 = lk * c.SW, yb0 = lk * YP + li;   // X walk in voxels
      const BwdwWalk wk{TW / 4, TH, 4 * c.SW, c.SH * LW - TW * c.SW, (c.SD * LH - TH * c.SH) * LW, TV / 4};
      switch (mytaps) {
        case 7: bwdw_tile_compute<7>(xl, yl, tapoff, xb0, yb0, wk, li, acc); break;
        case 6: bwdw_tile_compute<6>(xl, yl, tapoff, xb0, yb0, wk, li, acc); break;
        case 5: bwdw_tile_compute<5>(xl, yl, tapoff, xb0, yb0, wk, li, acc); break;
        case 4: bwdw_tile_compute<4>(xl, yl, tapoff, xb0, yb0, wk, li, acc); break;
        case 3: bwdw_tile_compute<3>(xl, yl, tapoff, xb0, yb0, wk, li, acc); break;
        case 2: bwdw_tile_compute<2>(xl, yl, tapoff, xb0, yb0, wk, li, acc); break;
        case 1: bwdw_tile_compute<1>(xl, yl, tapoff, xb0, yb0, wk, li, acc); break;
        default: break;
      }
    }
  }
  // write partial: D layout of 16x16x4: row (ci) = (lane>>4)*4 + j, col (co) = lane&15
  float* pp = P.part + ((size_t)((size_t)(chi * P.ncot + cot) * P.nsg + sg) * P.ntaps) * (16 * 32);
#pragma unroll
  for (int t = 0; t < BW_MAXT; ++t) {
    const int tap = wave + 4 * t;
    if (tap < P.ntaps) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) pp[(size_t)tap * 512 + (lk * 4 + j) * 32 + h * 16 + li] = acc[t][h][j];
    }
  }
}

struct BwdWReduceParams {
  const float* part; float* dw;
  int Cin, Cout, KD, KH, KW, nchunks, ncot, nsg, ntaps, accumulate;
  long s_ci, s_co, s_kd, s_kh, s_kw;
  ConvChunk chunk[MT_MAX_CHUNKS];
};
__global__ void bwdw_reduce_kernel(const BwdWReduceParams P) {
  // one thread per (chunk, cot, tap, ci16, co32)
  const long total = (long)P.nchunks * P.ncot * P.ntaps * 512;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long r = i;
    const int col = (int)(r % 32); r /= 32;
    const int cil = (int)(r % 16); r /= 16;
    const int tap = (int)(r % P.ntaps); r /= P.ntaps;
    const int cot = (int)(r % P.ncot); r /= P.ncot;
    const int chi = (int)r;
    const ConvChunk cc = P.chunk[chi];
    const int co = cot * 32 + col;
    if (cil >= cc.ck || co >= P.Cout) continue;
    const float* pp = P.part + ((size_t)(chi * P.ncot + cot) * P.nsg * P.ntaps + tap) * 512 + cil * 32 + col;
    // four independent chains keep several loads in flight (the order is fixed, so the result stays deterministic)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const size_t gs = (size_t)P.ntaps * 512;
    int g = 0;
    for (; g + 4 <= P.nsg; g += 4) {
      s0 += (double)pp[(size_t)g * gs];
      s1 += (double)pp[(size_t)(g + 1) * gs];
      s2 += (double)pp[(size_t)(g + 2) * gs];
      s3 += (double)pp[(size_t)(g + 3) * gs];
    }
    for (; g < P.nsg; ++g) s0 += (double)pp[(size_t)g * gs];
    const double s = (s0 + s1) + (s2 + s3);
    const int kw = tap % P.KW, kh = (tap / P.KW) % P.KH, kd = tap / (P.KW * P.KH);
    const long o = (long)(cc.cglob + cil) * P.s_ci + (long)co * P.s_co + kd * P.s_kd + kh * P.s_kh + kw * P.s_kw;
    if (P.accumulate) P.dw[o] += (float)s; else P.dw[o] = (float)s;
  }
}

// Deterministic in-workgroup reduction of the four waves' accumulator tiles through LDS (waves 2,3 -> 0,1, then 1 -> 0) and
// ONE partial per workgroup in global memory: [chunk][cot][sg][tap][16 ci][32 co].  Needs 2 * NT * 512 floats of LDS.
#define BW_RED_LDS(NT_) ((size_t)2 * (NT_) * 512 * sizeof(float))
template <int NT, bool NPERM = false, int CW = 1>
__device__ __forceinline__ void bwdw_wg_reduce_store(f32x4 (&acc)[NT][2], float* __restrict__ lds, float* __restrict__ pp,
                                                     int wave, int lane, bool valid = true) {
  const int li = lane & 15, lk = lane >> 4;
  // CW cout tiles per workgroup (wave = kq * CW + cw): only the 4 / CW waves of one cout tile are summed — CW = 4: every wave
  // stores its own tile, CW = 2: waves 2, 3 -> 0, 1 and both store.  pp / valid belong to THIS wave's cout tile.
  auto store = [&](const float* b) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          pp[(size_t)t * 512 + (lk * 4 + j) * 32 + (NPERM ? 2 * li + h : h * 16 + li)] = acc[t][h][j] + (b ? b[((t * 2 + h) * 4 + j) * 64] : 0.f);
  };
  if constexpr (CW == 4) {
    if (valid) store(nullptr);
    return;
  }
  __syncthreads();                     // every wave is done with the X tiles
  if (wave >= 2) {
    float* b = lds + (wave - 2) * (NT * 512) + lane;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[((t * 2 + h) * 4 + j) * 64] = acc[t][h][j];
  }
  __syncthreads();
  if constexpr (CW == 2) {
    if (wave < 2 && valid) store(lds + wave * (NT * 512) + lane);
    return;
  }
  if (wave < 2) {
    const float* b = lds + wave * (NT * 512) + lane;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][h][j] += b[((t * 2 + h) * 4 + j) * 64];
  }
  __syncthreads();
  if (wave == 1) {
    float* b = lds + lane;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[((t * 2 + h) * 4 + j) * 64] = acc[t][h][j];
  }
  __syncthreads();
  if (wave == 0) store(lds + lane);
}

// ================================================================================================
// FAST backward-weight kernel (3x3x3, stride 1, pad 1):  dW[tap][ci16][co32] += X(tile + tap)^T * Y(tile)
// K (= voxels) is split across the 4 waves, every wave accumulates ALL 27 taps for its quarter of the tile
// (216 accumulator registers), so all waves run the same straight-line code with compile-time LDS offsets:
// ZERO vector-ALU instructions between the v_mfma_f32_16x16x4_f32 (see conv_fast_kernel for why that matters).
// X tile: LDS [voxel][20] (same staging as the forward kernel).  Y fragments are wave-private, so they bypass LDS:
// buffer loads straight into registers in B-fragment order.  A workgroup walks a strided list of tiles and writes
// one partial per WAVE; bwdw_reduce_kernel sums them deterministically.
// XS / YS: storage types of X (p->src) and dY (ysrc)
template <int KD, int KH, int KW, int SD, int SH, int SW, int TH, int TW, int VEC, int XS = MT_F32, int YS = MT_F32, int CW = 1>
__global__ __launch_bounds__(256) void conv_bwdw_fast_kernel(const BwdWParams P) {
  constexpr int YE = mt_ebytes<YS>();
  // compile-time geometry: kernel K, stride S, pad (K-1)/2 for odd K and 0 for K = 2 (transposed-conv weights); tile 1 x TH x TW
  constexpr int NT = KD * KH * KW;
  constexpr int PD = (KD == 3) ? 1 : 0, PH = (KH == 3) ? 1 : 0, PW = (KW == 3) ? 1 : 0;
  constexpr int LD = KD, LH = (TH - 1) * SH + KH, LW = (TW - 1) * SW + KW, TV = TH * TW;
  constexpr int KS = TV / 16;            // k-steps (4 voxels each) per wave
  constexpr int SPR = TW / 4;            // k-steps per tile row
  static_assert(TV == 128, "tile must hold 128 voxels");
  // CW cout tiles per workgroup: wave = kq * CW + cw takes cout tile cw and the blocks kq * CW ... kq * CW + CW - 1 of the tile's four
  // blocks of KS k-steps (CW = 1: one block per wave and a four-wave reduction at the end, the original form).  The staged X tile
  // then feeds CW times the MFMAs: staging (texture path + vector ALU, as long as the matrix phase at CW = 1) is amortised CW-fold.
  static_assert((CW == 1 || CW == 2 || CW == 4) && KS % SPR == 0, "cout tiles per workgroup");
  constexpr int GOFF = (KS / SPR) * SH * LW * FCKP;      // LDS distance between consecutive blocks
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int cw = wave & (CW - 1), kq = wave / CW;
  const int sg = blockIdx.x, cot = blockIdx.y * CW + cw, chi = blockIdx.z;
  const ConvChunk cc = P.chunk[chi];
  const mt_src_t& Y = P.y;

  f32x4 acc[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t][h][j] = 0.f;

  // this wave's first voxel inside the tile: k-step ks = wave*KS + s -> (row, w0) = (ks / SPR, 4*(ks % SPR))
  const int row0 = (kq * CW * KS) / SPR;
  const int xbase0 = ((row0 * SH * LW) + lk * SW) * FCKP + li;     // + block * GOFF + compile-time (step voxel + tap voxel) * FCKP
  const int co = cot * 32 + li;
  const bool yaff = Y.scale != nullptr;
  const size_t ysample = (size_t)c.Do * c.Ho * c.Wo * Y.cs;

  // tile -> coordinates
  auto tile_coords = [&](int tile, int& nb, int& od0, int& oh0, int& ow0) {
    int r = tile;
    const int tw = r % P.tilesW; r /= P.tilesW;
    const int th = r % P.tilesH; r /= P.tilesH;
    od0 = r % P.tilesD; nb = r / P.tilesD;
    oh0 = th * TH; ow0 = tw * TW;
  };
  // Y fragments of this wave's KS k-steps (2 cout halves each), straight from global in B-fragment order.
  // ISSUE ONLY: the optional lazy-activation transform is applied when the fragments are rotated in (finish_y), never
  // right behind the loads — otherwise hipcc parks an s_waitcnt vmcnt(0) after every load pair and drains the prefetch.
  auto issue_y = [&](float (&yb)[KS][2], unsigned& okmask, int nb, int od0, int oh0, int ow0, int kb) {
    __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)Y.ptr + (size_t)nb * ysample * YE), 0, (int)(ysample * YE), 0x00020000);
    okmask = 0;
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
      const int ks = kb * KS + s2;                      // wave-uniform
      const int oh = oh0 + ks / SPR, ow = ow0 + 4 * (ks % SPR) + lk;
      const bool vok = (oh < c.Ho) && (ow < c.Wo);
      const int base = ((od0 * c.Ho + oh) * c.Wo + ow) * Y.cs + co;
      const bool k0 = vok && co < c.Cout, k1 = vok && co + 16 < c.Cout;
      okmask |= (k0 ? 1u : 0u) << (2 * s2);
      okmask |= (k1 ? 1u : 0u) << (2 * s2 + 1);
      if constexpr (YS == MT_F32) {
        yb[s2][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(yr, k0 ? base * 4 : (int)0x80000000, 0, 0));
        yb[s2][1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(yr, k1 ? (base + 16) * 4 : (int)0x80000000, 0, 0));
      } else {         // raw 16-bit elements; widened in finish_y
        yb[s2][0] = __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b16(yr, k0 ? base * 2 : (int)0x80000000, 0, 0));
        yb[s2][1] = __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b16(yr, k1 ? (base + 16) * 2 : (int)0x80000000, 0, 0));
      }
    }
  };
  auto widen_y = [&](float raw) -> float {
    if constexpr (YS == MT_F32) return raw;
    else return mt_from16<YS>((unsigned short)__builtin_bit_cast(unsigned, raw));
  };
  auto finish_y = [&](float (&dst)[KS][2], const float (&src)[KS][2], unsigned okmask, int nb) {
    if (yaff) {
      float ysc0 = 1.f, ysh0 = 0.f, ysc1 = 1.f, ysh1 = 0.f;
      if (co < c.Cout) { ysc0 = Y.scale[(size_t)nb * Y.C + co]; ysh0 = Y.shift[(size_t)nb * Y.C + co]; }
      if (co + 16 < c.Cout) { ysc1 = Y.scale[(size_t)nb * Y.C + co + 16]; ysh1 = Y.shift[(size_t)nb * Y.C + co + 16]; }
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) {
        dst[s2][0] = ((okmask >> (2 * s2)) & 1u) ? mt_lrelu(fmaf(widen_y(src[s2][0]), ysc0, ysh0), Y.slope) : 0.f;
        dst[s2][1] = ((okmask >> (2 * s2 + 1)) & 1u) ? mt_lrelu(fmaf(widen_y(src[s2][1]), ysc1, ysh1), Y.slope) : 0.f;
      }
    } else {
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) { dst[s2][0] = widen_y(src[s2][0]); dst[s2][1] = widen_y(src[s2][1]); }
    }
  };

  // Software pipeline over tiles: while the MFMAs of tile i run, the global loads of tile i+1 (X share of this wave into
  // registers, Y fragments) are in flight; between tiles only the register->LDS pass and two barriers are exposed.
  Stage2Regs<LD, LH, LW, VEC> xr;
  float ycur[KS][2], ynxt[KS][2];
  unsigned yok = 0;
  int ynb = 0;
  int tile = sg;
  int cnb = 0, cod0 = 0, coh0 = 0, cow0 = 0;       // coordinates of the tile in LDS
  if (tile < P.ntiles_total) {
    tile_coords(tile, cnb, cod0, coh0, cow0);
    stage2_load<LD, LH, LW, VEC, XS>(xr, c, cc, cnb, cod0 * SD - PD, coh0 * SH - PH, cow0 * SW - PW, lane, wave);
    issue_y(ynxt, yok, cnb, cod0, coh0, cow0, kq * CW);
    ynb = cnb;
  }
  for (; tile < P.ntiles_total; tile += P.nsg) {
    __syncthreads();     // previous tile's X reads are done
    if (!(BW_ABL & 1)) stage2_store<LD, LH, LW, VEC, FCKP, XS>(xr, lds, c, cc, lane, wave);
    if (!(BW_ABL & 2)) finish_y(ycur, ynxt, yok, ynb);
    __syncthreads();
    const int tnext = tile + P.nsg;
    const bool more = tnext < P.ntiles_total;
    int nnb = 0, nod0 = 0, noh0 = 0, now0 = 0;
    if (more) {
      tile_coords(tnext, nnb, nod0, noh0, now0);
      if (!(BW_ABL & 1)) stage2_load<LD, LH, LW, VEC, XS>(xr, c, cc, nnb, nod0 * SD - PD, noh0 * SH - PH, now0 * SW - PW, lane, wave);
    }
#pragma unroll 1
    for (int g = 0; g < CW; ++g) {
      if (CW > 1 && g > 0 && !(BW_ABL & 2)) finish_y(ycur, ynxt, yok, ynb);
      // dY fragments of the next block: the same tile's block g + 1, or block 0 of the next tile
      if (!(BW_ABL & 2)) {
        if (CW > 1 && g + 1 < CW) issue_y(ynxt, yok, cnb, cod0, coh0, cow0, kq * CW + g + 1);
        else if (more) { issue_y(ynxt, yok, nnb, nod0, noh0, now0, kq * CW); ynb = nnb; }
      }
      if (BW_ABL & 8) continue;
      const int xbase = xbase0 + g * GOFF;
      __builtin_amdgcn_sched_barrier(0);
      // ---- MFMA phase: KS k-steps x 27 taps x 2 cout halves; all LDS offsets are immediates and the A fragments of
      // k-step s+1 are fetched (ping-pong register sets) while the 54 MFMAs of k-step s issue
      float a0[NT], a1[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) a0[t] = lds[xbase + (((t / (KH * KW)) * LH + (t / KW) % KH) * LW + (t % KW)) * FCKP];
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) {
        float (&ac)[NT] = (s2 & 1) ? a1 : a0;
        float (&an)[NT] = (s2 & 1) ? a0 : a1;
        // one A read of the next k-step rides behind every MFMA pair: the LDS queue never fills, so MFMA issue never waits
        // on a burst of reads
        const int svox = ((s2 + 1) / SPR) * SH * LW + 4 * ((s2 + 1) % SPR) * SW;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (s2 + 1 < KS) an[t] = lds[xbase + (svox + ((t / (KH * KW)) * LH + (t / KW) % KH) * LW + (t % KW)) * FCKP];
          acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[t], ycur[s2][0], acc[t][0], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[t], ycur[s2][1], acc[t][1], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    cnb = nnb; cod0 = nod0; coh0 = noh0; cow0 = now0;
  }
  bwdw_wg_reduce_store<NT, false, CW>(acc, lds, P.part + ((size_t)((size_t)(chi * P.ncot + cot) * P.nsg + sg) * NT) * 512, wave, lane, cot < P.ncot);
}


// ================================================================================================
// Marching backward-weight kernel (KD = 3, SD = 1): a workgroup owns a column (sample, h-tile, w-tile) and walks it plane by
// plane along D.  The X planes live in a ring of 4 LDS slots, so every input plane is fetched from memory and transformed ONCE
// per column instead of once per output plane (the tile kernel above re-stages all three planes of every tile); one barrier per
// plane.  While the 432 MFMAs of plane d issue, plane d+2 of X and the Y fragments of plane d+1 are in flight.
// Voxel pitch 16 (SW = 1) / 24 (SW = 2) dwords makes the four k-groups of an A-fragment ds_read_b32 land on disjoint banks.
template <int KH, int KW, int SH, int SW, int TH, int TW, int VEC, int YV>
__global__ __launch_bounds__(256) void conv_bwdw_march_kernel(const BwdWParams P) {
  constexpr int KD = 3, NT = KD * KH * KW;
  constexpr int PH = (KH == 3) ? 1 : 0, PW = (KW == 3) ? 1 : 0;
  constexpr int LH = (TH - 1) * SH + KH, LW = (TW - 1) * SW + KW, TV = TH * TW;
  constexpr int KS = TV / 16, SPR = TW / 4;      // k-steps (4 voxels each) per wave and per tile row
  constexpr int PITCH = (SW == 1) ? 16 : 24;
  // staging geometry: 64 lanes = VPS voxels x LPV channel groups; NI steps cover a row, RPW rows per wave.  Rows are padded to
  // LWP = NI*VPS voxels in LDS so that every lane of every step may store unconditionally.
  constexpr int LPV = FCK / VEC, VPS = 64 / LPV, NI = (LW + VPS - 1) / VPS, RPW = (LH + 3) / 4, LWP = NI * VPS;
  constexpr int LHP = RPW * 4;                 // rows padded likewise: every wave stores RPW rows unconditionally
  constexpr int PLANE = LHP * LWP * PITCH;
  static_assert(TV % 64 == 0 && (KS % SPR == 0 || SPR % KS == 0), "tile must split evenly over 4 waves");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int sg = blockIdx.x, cot = blockIdx.y, chi = blockIdx.z;
  const ConvChunk cc = P.chunk[chi];
  const mt_src_t& Y = P.y;
  const mt_src_t& S = c.src[cc.src];

  f32x4 acc[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t][h][j] = 0.f;

  const int row0 = (wave * KS) / SPR, col0 = 4 * ((wave * KS) % SPR);
  const int xlane = ((row0 * SH * LWP) + (col0 + lk) * SW) * PITCH + li;
  // N permutation: column li of the MFMA for half h is output channel 2*li + h, so a lane's two B operands are ADJACENT in
  // memory (one 8-byte load) — bwdw_wg_reduce_store<NT, true> undoes it when the partial is written
  const int co0 = cot * 32 + 2 * li;
  const bool yaff = Y.scale != nullptr;
  const size_t ysample = (size_t)c.Do * c.Ho * c.Wo * Y.cs;
  const size_t xsample = (size_t)c.Di * c.Hi * c.Wi * S.cs;
  const int xplane_bytes = __builtin_amdgcn_readfirstlane(c.Hi * c.Wi * S.cs * 4);
  const int yplane_bytes = __builtin_amdgcn_readfirstlane(c.Ho * c.Wo * Y.cs * 4);

  // staging lane constants
  const int cl = (lane % LPV) * VEC, vl = lane / LPV;
  const bool xaff = S.scale != nullptr;
  const float xslope = xaff ? S.slope : 1.f;
  const int swlane = vl * PITCH + cl + wave * (LWP * PITCH);      // this lane's LDS store offset inside a plane (row r: + 4r rows)
  const int yoob1 = (co0 + 1 < c.Cout) ? 0 : (int)0x80000000;      // second channel of the pair exists?

  float xv[RPW][NI][VEC];      // the X plane in flight
  float ycur[KS][2];           // dY fragments of the current plane; refilled in place for the next plane

  for (int unit = sg; unit < P.nunits; unit += P.nsg) {
    int r = unit;
    const int seg = r % P.nseg; r /= P.nseg;
    const int tw = r % P.tilesW; r /= P.tilesW;
    const int th = r % P.tilesH;
    const int nb = r / P.tilesH;
    const int oh0 = th * TH, ow0 = tw * TW;
    const int uh0 = oh0 * SH - PH, uw0 = ow0 * SW - PW;
    const int d0 = seg * P.dseg;
    const int d1 = (d0 + P.dseg < c.Do) ? d0 + P.dseg : c.Do;

    // ---- per-unit constants: every per-plane load below is (constant VGPR offset, scalar plane/row offset).  Validity is
    // carried as data (masks / out-of-range offsets), never as control flow: uniform conditions would otherwise become dozens
    // of scalar branches around single loads and stores
    __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)(S.ptr + (size_t)nb * xsample), 0, (int)(xsample * 4), 0x00020000);
    __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)(Y.ptr + (size_t)nb * ysample), 0, (int)(ysample * 4), 0x00020000);
    int xvo[NI];
    unsigned mval[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int lw = vl + i * VPS, uw = uw0 + lw;
      const bool ok = (lw < LW) && ((unsigned)uw < (unsigned)c.Wi);
      xvo[i] = ok ? (uw * S.cs + cc.c0 + cl) * 4 : (int)0x80000000;
      mval[i] = ok ? 0xffffffffu : 0u;
    }
    int rowm[RPW], rowoff[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
      const int row = wave + 4 * q, uh = uh0 + row;
      const bool ok = (row < LH) && ((unsigned)uh < (unsigned)c.Hi);
      rowm[q] = ok ? -1 : 0;
      rowoff[q] = ok ? uh * c.Wi * S.cs * 4 : 0;
    }
    float sc[VEC], sh[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const bool cv = (cl + e) < cc.ck;
      sc[e] = cv ? 1.f : 0.f; sh[e] = 0.f;                    // channel slots beyond the chunk stage as zeros
      if (xaff && cv) { sc[e] = S.scale[(size_t)nb * S.C + cc.c0 + cl + e]; sh[e] = S.shift[(size_t)nb * S.C + cc.c0 + cl + e]; }
    }
    int yvo[KS];
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
      const int ks = wave * KS + s2;
      const int oh = oh0 + ks / SPR, ow = ow0 + 4 * (ks % SPR) + lk;
      const bool vok = (oh < c.Ho) && (ow < c.Wo) && (co0 < c.Cout);
      yvo[s2] = vok ? ((oh * c.Wo + ow) * Y.cs + co0) * 4 : (int)0x80000000;
    }
    float ysc0 = 1.f, ysh0 = 0.f, ysc1 = 1.f, ysh1 = 0.f;
    if (yaff) {
      if (co0 < c.Cout) { ysc0 = Y.scale[(size_t)nb * Y.C + co0]; ysh0 = Y.shift[(size_t)nb * Y.C + co0]; }
      if (co0 + 1 < c.Cout) { ysc1 = Y.scale[(size_t)nb * Y.C + co0 + 1]; ysh1 = Y.shift[(size_t)nb * Y.C + co0 + 1]; }
    }

    auto load_x = [&](int ud) {            // issue only
      const int pvm = ((unsigned)ud < (unsigned)c.Di) ? -1 : 0;
      const int poff = (ud & pvm) * xplane_bytes;
#pragma unroll
      for (int q = 0; q < RPW; ++q) {
        const int oob = ~(pvm & rowm[q]) & (int)0x80000000;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int vo = xvo[i] | oob;
          if constexpr (VEC == 2) {
            const float2 t = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(xrs, vo, poff + rowoff[q], 0));
            xv[q][i][0] = t.x; xv[q][i][1] = t.y;
          } else {
            xv[q][i][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, vo, poff + rowoff[q], 0));
          }
        }
      }
    };
    auto store_x = [&](int ud, int slot) {
      const int pvm = ((unsigned)ud < (unsigned)c.Di) ? -1 : 0;
      float* lp = lds + slot * PLANE + swlane;
#pragma unroll
      for (int q = 0; q < RPW; ++q) {
        const unsigned rvm = (unsigned)(pvm & rowm[q]);
        float scq[VEC], shq[VEC];      // a row outside the volume gets scale = shift = 0: its voxels stage as exact zeros
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          scq[e] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, sc[e]) & rvm);
          shq[e] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, sh[e]) & rvm);
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          float x[VEC];
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const float t = fmaf(xv[q][i][e], scq[e], shq[e]);
            const float a = mt_lrelu(t, xslope);
            x[e] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, a) & mval[i]);
          }
          float* d = lp + (4 * q * LWP + i * VPS) * PITCH;
          if constexpr (VEC == 2) { float2 t; t.x = x[0]; t.y = x[1]; *(float2*)d = t; }
          else *d = x[0];
        }
      }
    };
    auto load_y1 = [&](int s2, int poff, int oob) {      // the two dY operands of one k-step (oob masks a finished segment)
      if constexpr (YV == 2) {
        const float2 t = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(yrs, yvo[s2] | oob, poff, 0));
        ycur[s2][0] = t.x; ycur[s2][1] = t.y;
      } else {
        ycur[s2][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(yrs, yvo[s2] | oob, poff, 0));
        ycur[s2][1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(yrs, yvo[s2] | oob | yoob1, poff + 4, 0));
      }
    };
    auto activate_y = [&]() {          // lazy InstanceNorm+LeakyReLU of the dY fragments, in place; invalid lanes stay zero
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) {
        ycur[s2][0] = (yvo[s2] >= 0) ? mt_lrelu(fmaf(ycur[s2][0], ysc0, ysh0), Y.slope) : 0.f;
        ycur[s2][1] = (yvo[s2] >= 0 && yoob1 == 0) ? mt_lrelu(fmaf(ycur[s2][1], ysc1, ysh1), Y.slope) : 0.f;
      }
    };

    // ---- prologue: planes d0-1 and d0 into the ring, plane d0+1 and the dY fragments of plane d0 in flight
    __syncthreads();       // the previous unit's A reads are done
    load_x(d0 - 1); store_x(d0 - 1, (d0 + 3) & 3); load_x(d0); store_x(d0, d0 & 3); load_x(d0 + 1);
    {
      const int p0 = __builtin_amdgcn_readfirstlane(d0 * yplane_bytes);
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) load_y1(s2, p0, 0);
    }

    for (int d = d0; d < d1; ++d) {
      // slot (d+1)&3 last held plane d-3, read no later than step d-2: every wave has passed the barrier of step d-1 since
      store_x(d + 1, (d + 1) & 3);
      if (yaff) activate_y();
      __syncthreads();
      const bool more = d + 1 < d1;
      if (more) load_x(d + 2);
      const int ynext = __builtin_amdgcn_readfirstlane(more ? (d + 1) * yplane_bytes : 0);
      const int yoob = __builtin_amdgcn_readfirstlane(more ? 0 : (int)0x80000000);
      int xb[3];
#pragma unroll
      for (int kd = 0; kd < 3; ++kd) xb[kd] = ((d + 3 + kd) & 3) * PLANE + xlane;      // plane d-1+kd
      __builtin_amdgcn_sched_barrier(0);
      float a0[NT], a1[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) a0[t] = lds[xb[t / (KH * KW)] + (((t / KW) % KH) * LWP + (t % KW)) * PITCH];
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) {
        float (&ac)[NT] = (s2 & 1) ? a1 : a0;
        float (&an)[NT] = (s2 & 1) ? a0 : a1;
        // voxel offset of k-step s2+1 relative to this wave's first k-step (rows advance every SPR k-steps)
        const int ksn = s2 + 1;
        const int svox = (ksn / SPR) * SH * LWP + 4 * (ksn % SPR) * SW;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (s2 + 1 < KS) an[t] = lds[xb[t / (KH * KW)] + (svox + ((t / KW) % KH) * LWP + (t % KW)) * PITCH];
          acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[t], ycur[s2][0], acc[t][0], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[t], ycur[s2][1], acc[t][1], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
        load_y1(s2, ynext, yoob);          // this k-step's operands are consumed: fetch the next plane's in place
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  bwdw_wg_reduce_store<NT, true>(acc, lds, P.part + ((size_t)((size_t)(chi * P.ncot + cot) * P.nsg + sg) * NT) * 512, wave, lane);
}

// Stem backward-weight (Cin = 1): dW[tap][cout] = sum over voxels of x[voxel + tap] * dY[voxel][cout] as a GEMM with
// M = taps (27 of 32 rows), N = cout, K = voxels: per MFMA one scalar LDS read (lane = tap, voxel parity) and one coalesced
// dY load (lane = cout, voxel parity).  dY is streamed exactly once; persistent workgroups, fixed-order reduction.
// YS: storage type of dY (fp32 | bf16)
template <int YS = MT_F32>
__global__ __launch_bounds__(256) void conv_bwdw_stem_kernel(const BwdWParams P) {
  constexpr int TD = 2, TH = 4, TW = 32, LH = TH + 2, LW = TW + 2, YE = mt_ebytes<YS>();
  __shared__ float xs[(TD + 2) * LH * LW];
  __shared__ float red[3 * 16 * 64];
  const mt_conv3d_t& c = P.c;
  const mt_src_t& Y = P.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  const int sg = blockIdx.x, cot = blockIdx.y;
  const int co = cot * 32 + li;
  const int tap = li < 27 ? li : 26;
  const int dm = wave >> 1, r0 = (wave & 1) * 2;
  const int xlane = ((dm + tap / 9) * LH + r0 + (tap / 3) % 3) * LW + tap % 3 + lhalf;
  const int ylane = (co < c.Cout) ? (lhalf * Y.cs + co) * YE : (int)0x80000000;
  const size_t ysample = (size_t)c.Do * c.Ho * c.Wo * Y.cs;
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  // Staged dY (voxel stride a multiple of 4 bytes): the tile's 256 voxels x 32 channels arrive as
  // cooperative 16-byte pieces (4 per thread for 16-bit dY, 8 for fp32, requested one tile ahead) in an LDS image [voxel][YSP dwords];
  // the B operands are LDS reads.  The per-lane form below issues 32 gathers per wave and tile: 442 us (bf16) / 197 us (fp32) for the
  // 30-channel full-resolution gradient.
  constexpr int EPP = 16 / YE, PPV = 32 / EPP;                     // elements per piece, pieces per voxel (= pieces per thread)
  constexpr int YSP = 32 * YE / 4 + 1;                             // dwords per voxel of the image (odd: the two voxel parities on disjoint banks)
  __shared__ unsigned ysl[TD * TH * TW * YSP];
  const bool staged = ((Y.cs * YE) & 3) == 0 && !((uintptr_t)Y.ptr & 3);       // block-uniform: dword-aligned 16-byte loads
  uint4 yq[PPV];
  auto tile_of = [&](int tile, int& nb, int& od0, int& oh0, int& ow0) {
    int r = tile;
    const int tw = r % P.tilesW; r /= P.tilesW;
    const int th = r % P.tilesH; r /= P.tilesH;
    const int td = r % P.tilesD;
    nb = r / P.tilesD;
    od0 = td * TD; oh0 = th * TH; ow0 = tw * TW;
  };
  auto fetch_tile = [&](int tile) {        // issue only
    int nb, od0, oh0, ow0; tile_of(tile, nb, od0, oh0, ow0);
    __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)Y.ptr + (size_t)nb * ysample * YE), 0, (int)(ysample * YE), 0x00020000);
#pragma unroll
    for (int j = 0; j < PPV; ++j) {
      const int pc = tid + 256 * j;
      const int vox = pc / PPV, q = pc % PPV;
      const int od = od0 + (vox >> 7), oh = oh0 + ((vox >> 5) & 3), ow = ow0 + (vox & 31);
      const bool ok = (tile < P.ntiles_total) && od < c.Do && oh < c.Ho && ow < c.Wo && (cot * 32 + EPP * q < c.Cout);
      const int off = ok ? (((od * c.Ho + oh) * c.Wo + ow) * Y.cs + cot * 32 + EPP * q) * YE : (int)0x80000000;
      yq[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(yr, off, 0, 0));
    }
  };
  if (staged && sg < P.ntiles_total) fetch_tile(sg);
  for (int tile = sg; tile < P.ntiles_total; tile += P.nsg) {
    int nb, od0, oh0, ow0; tile_of(tile, nb, od0, oh0, ow0);
    __syncthreads();
    stem_stage<TD, TH, TW>(xs, c, nb, od0, oh0, ow0, tid);
    if (staged) {
#pragma unroll
      for (int j = 0; j < PPV; ++j) {
        const int pc = tid + 256 * j;
        unsigned* d = ysl + (pc / PPV) * YSP + 4 * (pc % PPV);
        d[0] = yq[j].x; d[1] = yq[j].y; d[2] = yq[j].z; d[3] = yq[j].w;
      }
      __syncthreads();
      fetch_tile(tile + P.nsg);
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        float b[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int vox = ((dm * TH + r0 + m) * TW) + 2 * v + lhalf;
          if constexpr (YS == MT_F32) b[v] = __builtin_bit_cast(float, ysl[vox * YSP + li]);
          else b[v] = mt_from16<YS>(((const unsigned short*)ysl)[vox * (2 * YSP) + li]);
        }
#pragma unroll
        for (int v = 0; v < 16; ++v)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[xlane + m * LW + 2 * v], b[v], acc, 0, 0, 0);
      }
      continue;
    }
    __syncthreads();
    __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)Y.ptr + (size_t)nb * ysample * YE), 0, (int)(ysample * YE), 0x00020000);
    const int od = od0 + dm;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int oh = oh0 + r0 + m;
      const bool rowok = od < c.Do && oh < c.Ho;                         // wave-uniform
      const int rowoff = rowok ? ((od * c.Ho + oh) * c.Wo + ow0) * Y.cs * YE : 0;
      float b[16];
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const bool ok = rowok && (ow0 + 2 * v + lhalf < c.Wo);
        if constexpr (YS == MT_F32) b[v] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(yr, ok ? ylane : (int)0x80000000, rowoff + v * 2 * Y.cs * 4, 0));
        else b[v] = mt_from16<YS>(__builtin_amdgcn_raw_buffer_load_b16(yr, ok ? ylane : (int)0x80000000, rowoff + v * 2 * Y.cs * YE, 0));
      }
#pragma unroll
      for (int v = 0; v < 16; ++v)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[xlane + m * LW + 2 * v], b[v], acc, 0, 0, 0);
    }
  }
  // fixed-order reduction of the four waves, then one partial per workgroup: [cot][sg][tap][ci slot 0][cout]
  __syncthreads();
  if (wave > 0) {
#pragma unroll
    for (int q = 0; q < 16; ++q) red[((wave - 1) * 16 + q) * 64 + lane] = acc[q];
  }
  __syncthreads();
  if (wave == 0) {
    float* pp = P.part + ((size_t)((size_t)cot * P.nsg + sg) * 27) * 512;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float t = ((acc[q] + red[q * 64 + lane]) + red[(16 + q) * 64 + lane]) + red[(32 + q) * 64 + lane];
      const int row = (q & 3) + 8 * (q >> 2) + 4 * lhalf;      // tap
      if (row < 27) pp[(size_t)row * 512 + li] = t;
    }
  }
}


// Launch a backward-weight kernel with LDSB_ bytes of dynamic LDS; more than the default 64 KiB is asked for first.  Returns from the
// calling function when that fails.
#define MT_BWDW_LAUNCH(KFN_, GRID_, LDSB_, ST_, P_)                                                           \
  do {                                                                                                        \
    auto kfn = KFN_;                                                                                          \
    if ((LDSB_) > 64 * 1024) {                                                                                \
      hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDSB_)); \
      if (e != hipSuccess) { mt_set_error("bwd_weight: cannot raise dynamic LDS: %s", hipGetErrorString(e)); return MT_EHIP; } \
    }                                                                                                         \
    hipLaunchKernelGGL(kfn, GRID_, dim3(256), LDSB_, ST_, P_);                                                \
  } while (0)

#include "bwdw_wino.inc"
#include "bwdw_gemm.inc"
#include "bwdw_fast16.inc"

// compile-time geometries of the fast backward-weight kernel: (K, S) with pad (K-1)/2 for K=3/1 and 0 for K=2
struct BwGeo { int KD, KH, KW, SD, SH, SW; };
static const BwGeo kBwGeos[] = {
  {3, 3, 3, 1, 1, 1},   // 0: all stride-1 3x3x3 convs
  {3, 3, 3, 2, 2, 2},   // 1: strided stage convs (generic_UNet.py:263-278)
  {3, 3, 3, 1, 2, 2},   // 2: anisotropic pooling stage
  {2, 2, 2, 2, 2, 2},   // 3: ConvTranspose3d(k = s = 2) weights (X = dOut, Y = tconv input)
  {1, 2, 2, 1, 2, 2},   // 4: ConvTranspose3d(k = s = (1,2,2))
  {1, 1, 1, 1, 1, 1},   // 5: 1x1x1 heads
  {1, 3, 3, 1, 1, 1},   // 6: residual-encoder stage 0
  {1, 1, 1, 2, 2, 2},   // 7: strided 1x1x1 skip convs of the residual blocks (conv_blocks.py:159-165)
  {1, 1, 1, 1, 2, 2},   // 8: ... of the anisotropic stages
};
static int bwdw_fast_geo(const mt_conv3d_t* p, const mt_src_t* y) {
  if (!(p->dilD == 1 && p->dilH == 1 && p->dilW == 1)) return -1;
  for (int i = 0; i < p->nsrc; ++i)
    if ((double)p->Di * p->Hi * p->Wi * p->src[i].cs * 4.0 >= 2147483648.0) return -1;
  if ((double)p->Do * p->Ho * p->Wo * y->cs * 4.0 >= 2147483648.0) return -1;
  for (int g = 0; g < (int)(sizeof(kBwGeos) / sizeof(kBwGeos[0])); ++g) {
    const BwGeo& b = kBwGeos[g];
    if (p->KD == b.KD && p->KH == b.KH && p->KW == b.KW && p->SD == b.SD && p->SH == b.SH && p->SW == b.SW &&
        p->PD == (b.KD == 3 ? 1 : 0) && p->PH == (b.KH == 3 ? 1 : 0) && p->PW == (b.KW == 3 ? 1 : 0)) return g;
  }
  return -1;
}
#define BW_STEM_WGS 512
static bool bwdw_is_stem(const mt_conv3d_t* p, const mt_src_t* y) {
  if (p->nsrc != 1 || p->Cin != 1 || p->src[0].C != 1) return false;
  if (!(p->KD == 3 && p->KH == 3 && p->KW == 3 && p->SD == 1 && p->SH == 1 && p->SW == 1 && p->PD == 1 && p->PH == 1 && p->PW == 1)) return false;
  if (!(p->dilD == 1 && p->dilH == 1 && p->dilW == 1)) return false;
  if (y != nullptr && y->scale != nullptr) return false;                 // lazily activated dY takes the general kernel
  if ((double)p->Do * p->Ho * p->Wo * (y ? y->cs : p->Cout) * 4.0 >= 2147483648.0) return false;
  return true;
}
static bool bwdw_use_march(const mt_conv3d_t* p) {
  return p->KD == 3 && p->KH == 3 && p->KW == 3 && p->SD == 1 && p->SH == 1 && p->SW == 1 && p->PD == 1 && p->Do >= 3;
}
// the same kernel with KD = 1: the 1x3x3 stride-1 layers of the residual encoder's first stage (no depth halo, any Do)
static bool bwdw_use_wino133(const mt_conv3d_t* p) {
  const int g_bwdw_wino = mt_sel3(p, MT_SEL_BWDW_WINO);
  for (int i = 0; i < p->nsrc; ++i)
    if (p->src[i].scale != nullptr && !(p->src[i].slope >= 0.f && p->src[i].slope <= 1.f)) return false;
  return g_bwdw_wino && p->KD == 1 && p->KH == 3 && p->KW == 3 && p->SD == 1 && p->SH == 1 && p->SW == 1 && p->PD == 0 && p->PH == 1 &&
         p->PW == 1 && p->Wo > 16 && p->Ho >= 2 && conv_fast_vec(p) == 2 && conv_src_dtype(p) == MT_F32;
}
static bool bwdw_use_wino(const mt_conv3d_t* p) {
  const int g_bwdw_wino = mt_sel3(p, MT_SEL_BWDW_WINO);
  // (its X path applies LeakyReLU as max(t, slope * t): lazy sources need 0 <= slope <= 1)
  for (int i = 0; i < p->nsrc; ++i)
    if (p->src[i].scale != nullptr && !(p->src[i].slope >= 0.f && p->src[i].slope <= 1.f)) return false;
  return g_bwdw_wino && bwdw_use_march(p) && p->Wo > 16 && p->Ho >= 2 && conv_fast_vec(p) == 2;
}
// conv_bwdw_tr16_kernel (bwdw_tr16.hip): 3x3x3 / 1x3x3 stride-1, 16-bit X (lazy activations or plain), bf16 dY without affine, Wo > 16.
// ysrc == nullptr: geometry + X only (workspace query).
static bool bwdw_use_tr16(const mt_conv3d_t* p, const mt_src_t* ysrc) {
  const int g_bwdw_tr16 = mt_sel3(p, MT_SEL_BWDW_TR16);
  if (!g_bwdw_tr16 || p->mma != 1 || p->N > 16) return false;                 // (BWT_MAXN samples in the kernel's activation table)
  const bool g333 = bwdw_use_march(p) && p->PH == 1 && p->PW == 1;
  const bool g133 = p->KD == 1 && p->KH == 3 && p->KW == 3 && p->SD == 1 && p->SH == 1 && p->SW == 1 && p->PD == 0 && p->PH == 1 && p->PW == 1 && p->Do >= 1;
  if (!(g333 || g133) || !(p->dilD == 1 && p->dilH == 1 && p->dilW == 1) || !(p->Wo > 16 && p->Ho >= 2) || conv_fast_vec(p) != 2) return false;
  for (int i = 0; i < p->nsrc; ++i)          // (its X path applies LeakyReLU as max(t, slope * t))
    if (p->src[i].scale != nullptr && !(p->src[i].slope >= 0.f && p->src[i].slope <= 1.f)) return false;
  const int xdt = conv_src_dtype(p);
  if (xdt != MT_F16 && xdt != MT_BF16) return false;
  if (ysrc != nullptr && (ysrc->dtype != MT_BF16 || ysrc->scale != nullptr || (ysrc->cs & 1) || (((uintptr_t)ysrc->ptr) & 3))) return false;
  for (int i = 0; i < p->nsrc; ++i)
    if ((double)p->Di * p->Hi * p->Wi * p->src[i].cs * 2.0 >= 2147483648.0) return false;
  if ((double)p->Do * p->Ho * p->Wo * (ysrc ? ysrc->cs : p->Cout) * 2.0 >= 2147483648.0) return false;
  return true;
}
static inline int mt_bwdw_cw(const mt_conv3d_t* p) { const unsigned v = MT_SEL_GET(p->select, MT_SEL_BWDW_CW); return v == 1 ? 1 : v == 2 ? 2 : v == 3 ? 104 : 4; }
// the two halves every plan starts from: the spatial tiling, and the (tap, channel chunk, cout tile) decomposition
static void bwdw_set_tiles(const mt_conv3d_t* p, BwdWParams* P, int TD, int TH, int TW) {
  P->TD = TD; P->TH = TH; P->TW = TW;
  P->tilesD = mt_cdiv(p->Do, TD); P->tilesH = mt_cdiv(p->Ho, TH); P->tilesW = mt_cdiv(p->Wo, TW);
  P->ntiles_total = P->tilesD * P->tilesH * P->tilesW * p->N;
}
static void bwdw_set_channels(const mt_conv3d_t* p, BwdWParams* P) {
  P->ntaps = p->KD * p->KH * p->KW;
  P->nchunks = mt_build_chunks(p->src[0].C, p->nsrc == 2 ? p->src[1].C : 0, BW_CK, P->chunk);
  P->ncot = mt_cdiv(p->Cout, 32);
}
// workgroups per (cout tile, chunk pair): one per CU over all pairs, never more than (column, plane) pairs
static int bwdw_tr16_nsg(const mt_conv3d_t* p, int nchunks) {
  const int pairs = mt_cdiv(p->Cout, 32) * ((nchunks + 1) / 2);
  const long T = (long)p->N * mt_cdiv(p->Ho, 4) * mt_cdiv(p->Wo, 32) * p->Do;
  // (rounded DOWN: one workgroup fits a CU, so 8 pairs x ceil(256 / 120) = 360 workgroups were two rounds for 104 of them — twice a
  // workgroup's time — where 240 workgroups of 1.5x the work take 1.5x)
  long nsg = mt_device_cus(mt_current_device()) / pairs;
  if (nsg > T) nsg = T;
  if (p->max_workgroups > 0 && nsg > p->max_workgroups) nsg = p->max_workgroups;      // tests: few workgroups, so that a range spans columns on small volumes
  return nsg < 1 ? 1 : (int)nsg;
}
static void bwdw_tr16_plan(const mt_conv3d_t* p, BwdWParams* P) {
  bwdw_set_tiles(p, P, 1, 4, 32);
  bwdw_set_channels(p, P);                  // (KH = KW = 3: KD * 9 taps)
  P->cw = 1;
  P->nsg = P->nsg_cap = P->nchunks > 0 ? bwdw_tr16_nsg(p, P->nchunks) : 1;
  P->nunits = 0; P->nseg = 1; P->dseg = p->Do;
}
// conv_bwdw_fast_kernel (fp32 storage on both sides) / conv_bwdw_fast16_kernel with several cout tiles per workgroup (channel-pair
// staging; the geometries launch_bwdw_fast / launch_bwdw_fast16 instantiate them for): 4 when the cout tiles divide by 4, else 2, else 1.  The MT_SEL_BWDW_CW field of mt_conv3d_t.select limits it.
static int bwdw_fast_cw(const mt_conv3d_t* p, int ntiles_total, int nchunks) {
  const int g_bwdw_cw = mt_bwdw_cw(p);
  const int cap = g_bwdw_cw % 100;
  const bool force = g_bwdw_cw >= 100;          // 104 / 102: without the tiles-per-workgroup condition below (tests on small volumes)
  if (cap < 2 || conv_src_dtype(p) < 0 || conv_fast_vec(p) != 2) return 1;
  const bool g333 = p->KD == 3 && p->KH == 3 && p->KW == 3 && p->SH == 2 && p->SW == 2 && (p->SD == 1 || p->SD == 2);      // strided stage convs
  const bool g222 = p->KH == 2 && p->KW == 2 && p->SH == 2 && p->SW == 2 && ((p->KD == 2 && p->SD == 2) || (p->KD == 1 && p->SD == 1));   // transposed-conv weights
  const bool g133 = p->KD == 1 && p->KH == 3 && p->KW == 3 && p->SD == 1 && p->SH == 1 && p->SW == 1;                      // residual-encoder stage 0
  if (!(g333 || g222 || g133)) return 1;
  const int ncot = mt_cdiv(p->Cout, 32);
  int cw = (ncot % 4 == 0) ? 4 : ((ncot % 2 == 0) ? 2 : 1);
  if (cw > cap) cw = cap;
  // every workgroup should still walk >= 6 tiles: below that its fixed costs (prologue, CW partials of ntaps x 512 floats) outweigh the
  // saved staging (the 3 x 6 x 6 layers measured 102 -> 111 us with two tiles per workgroup)
  while (!force && cw > 1 && (long)ntiles_total * nchunks * (ncot / cw) < 1536) cw >>= 1;
  return cw;
}

// marching plan: columns x D segments; the segment count balances the units over the workgroups of a (chunk, cout tile) pair
static void bwdw_march_plan(const mt_conv3d_t* p, BwdWParams* P) {
  const int cols = p->N * P->tilesH * P->tilesW;
  int best = 1; double bestcost = 1e300;
  for (int nseg = 1; nseg <= p->Do; ++nseg) {
    const int dseg = mt_cdiv(p->Do, nseg);
    if (mt_cdiv(p->Do, dseg) != nseg) continue;
    const long units = (long)cols * nseg;
    const double cost = (double)mt_cdiv(units, P->nsg_cap) * (dseg + 2.0);   // +2: prologue planes of every unit
    if (cost < bestcost - 1e-9) { bestcost = cost; best = nseg; }
  }
  P->nseg = best; P->dseg = mt_cdiv(p->Do, best);
  P->nunits = cols * best;
  P->nsg = P->nsg_cap < P->nunits ? P->nsg_cap : P->nunits;
}
// plan for the fast kernel: tile 1 x TH x TW with (TH,TW) = (4,32) or (8,16)
static void bwdw_fast_plan(const mt_conv3d_t* p, BwdWParams* P, bool allow_cw = false, bool f32_both = false) {
  const bool wide = p->Wo > 16;
  bwdw_set_tiles(p, P, 1, wide ? 4 : 8, wide ? 32 : 16);
  bwdw_set_channels(p, P);
  P->cw = allow_cw ? bwdw_fast_cw(p, P->ntiles_total, P->nchunks) : 1;
  // fp32 Winograd marching kernel: two cout tiles per workgroup where the cout tiles pair up and a workgroup still gets >= 12 planes
  if (allow_cw && (bwdw_use_wino(p) || (f32_both && bwdw_use_wino133(p))) && conv_src_dtype(p) == MT_F32) {
    const int g_bwdw_cw = mt_bwdw_cw(p);
    const long planes = (long)p->N * mt_cdiv(p->Ho, 4) * mt_cdiv(p->Wo, 32) * p->Do;
    P->cw = 1;                              // (bwdw_fast_cw answers for conv_bwdw_fast_kernel)
    if ((g_bwdw_cw % 100) >= 2 && P->ncot % 2 == 0 && (g_bwdw_cw >= 100 || planes * P->nchunks * (P->ncot / 2) >= 3072)) P->cw = 2;
  }
  int pairs = P->nchunks * mt_cdiv(P->ncot, P->cw); if (pairs < 1) pairs = 1;
  // one workgroup per CU (up to 216 accumulator registers per wave), rounded DOWN: 60 pairs x ceil(256 / 60) = 300 workgroups are two
  // rounds for 44 of them (240 -> 240 @ 6x24x24), 60 x 4 = 240 are one round of 1.25x the work
  int nsg = 256 / pairs;
  // conv_bwdw_fast16_kernel with few taps (transposed-conv weights, 1x1x1): <= 180 registers and <= 49 KiB of LDS — two workgroups per CU
  if (p->mma == 1 && p->src[0].dtype != MT_F32 && P->ntaps <= 8 && !bwdw_use_march(p)) nsg = 512 / pairs;
  if (allow_cw && f32_both && bwdw_use_wino133(p)) nsg = 512 / pairs;       // conv_bwdw_wino_kernel<2, CW, 1>: 64 KiB of LDS, two per CU
  if (nsg < 1) nsg = 1;
  P->nsg_cap = nsg;
  if (nsg > P->ntiles_total) nsg = P->ntiles_total;
  if (nsg < 1) nsg = 1;
  P->nsg = nsg;
  P->nunits = 0; P->nseg = 1; P->dseg = p->Do;
  if (bwdw_march16_geo(p)) bwdw_march_plan(p, P);      // conv_bwdw_march16_kernel: columns x D segments (tile 4 x 32: Wo > 16)
  if (allow_cw && f32_both && bwdw_use_wino133(p)) {   // conv_bwdw_wino_kernel<2, CW, 1>: columns x D segments
    bwdw_set_tiles(p, P, 1, 4, 32);
    bwdw_march_plan(p, P);
  }
  if (bwdw_use_march(p)) {
    if (bwdw_use_wino(p)) bwdw_set_tiles(p, P, 1, 4, 32);
    else if (wide && p->Ho >= 8) bwdw_set_tiles(p, P, 1, 8, 32);
    bwdw_march_plan(p, P);
  }
}

static void bwdw_plan(const mt_conv3d_t* p, BwdWParams* P) {
  // tile: rows of up to 32 voxels in W (multiple of 4), ~128 voxels per tile
  int TW = p->Wo >= 32 ? 32 : ((p->Wo + 3) / 4) * 4;
  int TH = 128 / TW; if (TH > p->Ho) TH = p->Ho; if (TH < 1) TH = 1;
  int TD = 128 / (TW * TH); if (TD > p->Do) TD = p->Do; if (TD < 1) TD = 1;
  // keep the haloed X tile within ~48 KiB for strided convs
  for (;;) {
    const size_t LD = (TD - 1) * p->SD + p->KD, LH = (TH - 1) * p->SH + p->KH, LW = (TW - 1) * p->SW + p->KW;
    const size_t b = (LD * LH * LW * BW_CK + (size_t)TD * TH * TW * BW_YP) * sizeof(float);
    if (b <= 72 * 1024 || (TD == 1 && TH == 1)) break;
    if (TD > 1) TD = (TD + 1) / 2; else TH = (TH + 1) / 2;
  }
  bwdw_set_tiles(p, P, TD, TH, TW);
  bwdw_set_channels(p, P);
  // spatial groups: fill ~2 workgroups per CU over all (chunk, cot) pairs
  int pairs = P->nchunks * P->ncot; if (pairs < 1) pairs = 1;
  int nsg = (512 + pairs - 1) / pairs;
  if (nsg > P->ntiles_total) nsg = P->ntiles_total;
  if (nsg < 1) nsg = 1;
  P->nsg = nsg;
}

template <int KH, int KW, int SH, int SW>
static int launch_bwdw_march(const BwdWParams& P, int vec, int yv, hipStream_t st) {
  constexpr int PITCH = (SW == 1) ? 16 : 24;
  const int vps = vec == 2 ? 8 : 4;                                 // voxels per staging step; rows are padded to a multiple
  const int LH = (P.TH - 1) * SH + KH, LW = (P.TW - 1) * SW + KW;
  size_t ldsb = (size_t)4 * (mt_cdiv(LH, 4) * 4) * (mt_cdiv(LW, vps) * vps) * PITCH * sizeof(float);
  if (ldsb < BW_RED_LDS(3 * KH * KW)) ldsb = BW_RED_LDS(3 * KH * KW);
  MT_REQUIRE(ldsb <= 160 * 1024, "bwd_weight: LDS ring too large (%zu)", ldsb);
  dim3 grid(P.nsg, P.ncot, P.nchunks);
#define MT_BW_LAUNCH(TH_, TW_, VEC_, YV_) MT_BWDW_LAUNCH((conv_bwdw_march_kernel<KH, KW, SH, SW, TH_, TW_, VEC_, YV_>), grid, ldsb, st, P)
#define MT_BW_LAUNCH_T(TH_, TW_)                                                                              \
  do {                                                                                                        \
    if (vec == 2) { if (yv == 2) MT_BW_LAUNCH(TH_, TW_, 2, 2); else MT_BW_LAUNCH(TH_, TW_, 2, 1); }           \
    else          { if (yv == 2) MT_BW_LAUNCH(TH_, TW_, 1, 2); else MT_BW_LAUNCH(TH_, TW_, 1, 1); }           \
  } while (0)
  if (P.TW == 32 && P.TH == 8) MT_BW_LAUNCH_T(8, 32);
  else if (P.TW == 32)         MT_BW_LAUNCH_T(4, 32);
  else                         MT_BW_LAUNCH_T(8, 16);
#undef MT_BW_LAUNCH_T
#undef MT_BW_LAUNCH
  MT_CHECK_LAUNCH("conv_bwdw_march");
  return MT_OK;
}

// conv_bwdw_wino_kernel<2, CW, KD>: one or two cout tiles per workgroup (BwdWParams::cw), KD = 3 | 1
template <int CW, int KD>
static int launch_bwdw_wino_cw(const BwdWParams& P, hipStream_t st) {
  const size_t ldsb = (size_t)BWW_LDS_FLOATS * sizeof(float) / (KD == 3 ? 1 : 2);      // ring of 4 (KD = 3) / 2 (KD = 1) planes
  const int devid = mt_current_device();
  static std::atomic<uint64_t> attr{0};          // (one per instantiation: the attribute is set once per kernel and device)
  if (mt_device_pending(attr, devid)) {
    hipError_t e = hipFuncSetAttribute((const void*)conv_bwdw_wino_kernel<2, CW, KD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb);
    if (e != hipSuccess) { mt_set_error("bwd_weight: cannot raise dynamic LDS: %s", hipGetErrorString(e)); return MT_EHIP; }
    mt_mark_device_done(attr, devid);
  }
  hipLaunchKernelGGL((conv_bwdw_wino_kernel<2, CW, KD>), dim3(P.nsg, P.ncot / CW, P.nchunks), dim3(256), ldsb, st, P);
  MT_CHECK_LAUNCH("conv_bwdw_wino");
  return MT_OK;
}
template <int KD>
static int launch_bwdw_wino(const BwdWParams& P, hipStream_t st) {
  MT_REQUIRE(P.cw == 1 || P.cw == 2, "bwd_weight: %d cout tiles per workgroup in the Winograd kernel", P.cw);
  return P.cw == 2 ? launch_bwdw_wino_cw<2, KD>(P, st) : launch_bwdw_wino_cw<1, KD>(P, st);
}

// conv_bwdw_fast_kernel (fp32 products; the 16-bit forms are launch_bwdw_fast16 / launch_bwdw_march16 of bwdw_fast16.inc)
template <int KD, int KH, int KW, int SD, int SH, int SW>
static int launch_bwdw_fast(const BwdWParams& P, int vec, hipStream_t st) {
  constexpr int LHa = 3 * SH + KH, LWa = 31 * SW + KW, LHb = 7 * SH + KH, LWb = 15 * SW + KW;
  size_t ldsb = (size_t)KD * (P.TW == 32 ? LHa * LWa : LHb * LWb) * FCKP * sizeof(float);
  if (ldsb < BW_RED_LDS(KD * KH * KW)) ldsb = BW_RED_LDS(KD * KH * KW);
  MT_REQUIRE(ldsb <= 160 * 1024, "bwd_weight: LDS tile too large (%zu)", ldsb);
  dim3 grid(P.nsg, mt_cdiv(P.ncot, P.cw), P.nchunks);
#define MT_BW_LAUNCH_K(KFN_) MT_BWDW_LAUNCH(KFN_, grid, ldsb, st, P)
  // storage types: X fp32 | fp16 | bf16 (16-bit: channel pairs, vec == 2), dY fp32 | bf16 — the combinations the engine produces
  const int xs = P.c.src[0].dtype, ys = P.y.dtype;
#define MT_BW_LAUNCH(TH_, TW_, VEC_)                                                                          \
  do {                                                                                                        \
    if (xs == MT_F32 && ys == MT_F32) MT_BW_LAUNCH_K((conv_bwdw_fast_kernel<KD, KH, KW, SD, SH, SW, TH_, TW_, VEC_>)); \
    else if (VEC_ == 2 && xs == MT_F16 && ys == MT_BF16) MT_BW_LAUNCH_K((conv_bwdw_fast_kernel<KD, KH, KW, SD, SH, SW, TH_, TW_, 2, MT_F16, MT_BF16>)); \
    else if (VEC_ == 2 && xs == MT_F16 && ys == MT_F32) MT_BW_LAUNCH_K((conv_bwdw_fast_kernel<KD, KH, KW, SD, SH, SW, TH_, TW_, 2, MT_F16, MT_F32>)); \
    else if (VEC_ == 2 && xs == MT_BF16 && ys == MT_F16) MT_BW_LAUNCH_K((conv_bwdw_fast_kernel<KD, KH, KW, SD, SH, SW, TH_, TW_, 2, MT_BF16, MT_F16>)); \
    else if (VEC_ == 2 && xs == MT_BF16 && ys == MT_BF16) MT_BW_LAUNCH_K((conv_bwdw_fast_kernel<KD, KH, KW, SD, SH, SW, TH_, TW_, 2, MT_BF16, MT_BF16>)); \
    else { mt_set_error("bwd_weight: storage types (X %d, dY %d) not compiled into conv_bwdw_fast_kernel", xs, ys); return MT_EINVAL; } \
  } while (0)
  // several cout tiles per workgroup (bwdw_fast_cw: fp32 storage, channel pairs, these geometries)
  constexpr bool CWG = (KD == 3 && KH == 3 && KW == 3 && SH == 2 && SW == 2) || (KH == 2 && KW == 2 && SH == 2 && SW == 2) ||
                       (KD == 1 && KH == 3 && KW == 3 && SD == 1 && SH == 1 && SW == 1);
  if (P.cw > 1) {
    if constexpr (CWG) {
      MT_REQUIRE(vec == 2 && xs == MT_F32 && ys == MT_F32 && (P.cw == 2 || P.cw == 4), "bwd_weight: cout tiles per workgroup (%d) on a problem the kernel is not compiled for", P.cw);
      if (P.TW == 32) { if (P.cw == 4) MT_BW_LAUNCH_K((conv_bwdw_fast_kernel<KD, KH, KW, SD, SH, SW, 4, 32, 2, MT_F32, MT_F32, 4>));
                        else           MT_BW_LAUNCH_K((conv_bwdw_fast_kernel<KD, KH, KW, SD, SH, SW, 4, 32, 2, MT_F32, MT_F32, 2>)); }
      else            { if (P.cw == 4) MT_BW_LAUNCH_K((conv_bwdw_fast_kernel<KD, KH, KW, SD, SH, SW, 8, 16, 2, MT_F32, MT_F32, 4>));
                        else           MT_BW_LAUNCH_K((conv_bwdw_fast_kernel<KD, KH, KW, SD, SH, SW, 8, 16, 2, MT_F32, MT_F32, 2>)); }
      MT_CHECK_LAUNCH("conv_bwdw_fast (cout tiles per workgroup)");
      return MT_OK;
    } else {
      mt_set_error("bwd_weight: cout tiles per workgroup (%d) on a geometry the kernel is not compiled for", P.cw); return MT_EINVAL;
    }
  }
  if (P.TW == 32) { if (vec == 2) MT_BW_LAUNCH(4, 32, 2); else MT_BW_LAUNCH(4, 32, 1); }
  else            { if (vec == 2) MT_BW_LAUNCH(8, 16, 2); else MT_BW_LAUNCH(8, 16, 1); }
#undef MT_BW_LAUNCH
#undef MT_BW_LAUNCH_K
  MT_CHECK_LAUNCH("conv_bwdw_fast");
  return MT_OK;
}

// conv_bwdw_stem_kernel: the single-channel network input, tile 2 x 4 x 32, at most BW_STEM_WGS workgroups per cout tile
static void bwdw_stem_plan(const mt_conv3d_t* p, BwdWParams* P) {
  bwdw_set_tiles(p, P, 2, 4, 32);
  bwdw_set_channels(p, P);                  // (27 taps, one chunk of one channel)
  P->nsg = P->ntiles_total < BW_STEM_WGS ? P->ntiles_total : BW_STEM_WGS;
}
static int launch_bwdw_stem(const BwdWParams& P, hipStream_t st) {
  if (P.y.dtype == MT_BF16) hipLaunchKernelGGL((conv_bwdw_stem_kernel<MT_BF16>), dim3(P.nsg, P.ncot, 1), dim3(256), 0, st, P);
  else hipLaunchKernelGGL((conv_bwdw_stem_kernel<MT_F32>), dim3(P.nsg, P.ncot, 1), dim3(256), 0, st, P);
  MT_CHECK_LAUNCH("conv_bwdw_stem");
  return MT_OK;
}

// conv_bwdw_kernel: any kernel size up to 3, any stride
static int launch_bwdw_generic(const BwdWParams& P, hipStream_t st) {
  const mt_conv3d_t* p = &P.c;
  MT_REQUIRE(P.ntaps <= 4 * BW_MAXT, "bwd_weight: too many taps");
  const size_t LD = (P.TD - 1) * p->SD + p->KD, LH = (P.TH - 1) * p->SH + p->KH, LW = (P.TW - 1) * p->SW + p->KW;
  const size_t ldsb = (LD * LH * LW * BW_CK + (size_t)P.TD * P.TH * P.TW * BW_YP) * sizeof(float);
  MT_REQUIRE(ldsb <= 160 * 1024, "bwd_weight: LDS tile too large (%zu)", ldsb);
  MT_BWDW_LAUNCH(conv_bwdw_kernel, dim3(P.nsg, P.ncot, P.nchunks), ldsb, st, P);
  MT_CHECK_LAUNCH("conv_bwdw");
  return MT_OK;
}

// the tiled launchers instantiated for kBwGeos, in its order
#define MT_BW_GEOS(FN_) FN_<3, 3, 3, 1, 1, 1>, FN_<3, 3, 3, 2, 2, 2>, FN_<3, 3, 3, 1, 2, 2>, FN_<2, 2, 2, 2, 2, 2>, FN_<1, 2, 2, 1, 2, 2>, \
                        FN_<1, 1, 1, 1, 1, 1>, FN_<1, 3, 3, 1, 1, 1>, FN_<1, 1, 1, 2, 2, 2>, FN_<1, 1, 1, 1, 2, 2>
static int (*const kLaunchFast[9])(const BwdWParams&, int, hipStream_t) = {MT_BW_GEOS(launch_bwdw_fast)};
static int (*const kLaunchFast16[9])(const BwdWParams&, hipStream_t) = {MT_BW_GEOS(launch_bwdw_fast16)};
#undef MT_BW_GEOS

// partial sums of a plan: one [tap][16 ci][32 co] block per (chunk, cout tile, workgroup)
static size_t bwdw_partials_bytes(const BwdWParams& P) { return (size_t)P.nchunks * P.ncot * P.nsg * P.ntaps * 512 * sizeof(float); }

// bwdw_reduce_kernel: the workgroups' partials -> dW in the caller's layout (grid-stride: the grid does not change the sums)
static int bwdw_launch_reduce(const BwdWParams& P, float* dw, long s_ci, long s_co, long s_kd, long s_kh, long s_kw, int accumulate, hipStream_t st) {
  BwdWReduceParams R;
  R.part = P.part; R.dw = dw; R.Cin = P.c.Cin; R.Cout = P.c.Cout; R.KD = P.c.KD; R.KH = P.c.KH; R.KW = P.c.KW;
  R.nchunks = P.nchunks; R.ncot = P.ncot; R.nsg = P.nsg; R.ntaps = P.ntaps; R.accumulate = accumulate;
  R.s_ci = s_ci; R.s_co = s_co; R.s_kd = s_kd; R.s_kh = s_kh; R.s_kw = s_kw;
  for (int i = 0; i < P.nchunks; ++i) R.chunk[i] = P.chunk[i];
  const long total = (long)P.nchunks * P.ncot * P.ntaps * 512;
  int blocks = mt_cdiv(total, 256); if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(bwdw_reduce_kernel, dim3(blocks), dim3(256), 0, st, R);
  MT_CHECK_LAUNCH("bwdw_reduce");
  return MT_OK;
}

// ------------------------------------------------------------------------------------------------
// THE dispatch decision: which kernel family serves (p, ysrc), in the order the launch tries them.  The kernel name, io_supported and
// the launch read this choice; mt_conv3d_bwd_weight_workspace has no dY and takes the maximum over what a launch could choose.
enum BwdwKind { BWDW_GENERIC, BWDW_STEM, BWDW_GEMM, BWDW_TR16, BWDW_WINO, BWDW_WINO133, BWDW_MARCH, BWDW_MARCH16, BWDW_FAST16, BWDW_FAST };
struct BwdwChoice {
  int kind, geo;      // BwdwKind; index into kBwGeos (-1: none)
  bool cw_ok;         // the plan may put several cout tiles into a workgroup (bwdw_fast_plan's allow_cw)
  bool f32_both;      // fp32 storage of X and dY
};
static BwdwChoice bwdw_resolve(const mt_conv3d_t* p, const mt_src_t* ysrc) {
  BwdwChoice c = {BWDW_GENERIC, -1, false, false};
  if (bwdw_is_stem(p, ysrc)) { c.kind = BWDW_STEM; return c; }
  const int geo = c.geo = bwdw_fast_geo(p, ysrc);
  if (geo < 0) return c;
  if (bwdw_use_gemm(p, ysrc)) { c.kind = BWDW_GEMM; return c; }
  const bool fast16 = bwdw_fast16_ok(p, ysrc);
  c.f32_both = conv_src_dtype(p) == MT_F32 && ysrc->dtype == MT_F32;
  // several cout tiles per workgroup: conv_bwdw_fast_kernel with fp32 storage on both sides, conv_bwdw_fast16_kernel and its marching
  // form, the fp32 Winograd kernels — not conv_bwdw_march_kernel
  c.cw_ok = (fast16 || c.f32_both) && !(geo == 0 && bwdw_use_march(p) && !(bwdw_use_wino(p) && c.f32_both));
  if ((geo == 0 || geo == 6) && bwdw_use_tr16(p, ysrc)) c.kind = BWDW_TR16;
  else if (geo == 0 && bwdw_use_wino(p)) c.kind = BWDW_WINO;
  else if (geo == 0 && bwdw_use_march(p)) c.kind = BWDW_MARCH;
  else if (geo == 6 && c.f32_both && bwdw_use_wino133(p)) c.kind = BWDW_WINO133;
  else if ((geo == 1 || geo == 2) && bwdw_march16_ok(p, ysrc)) c.kind = BWDW_MARCH16;      // marching form of the strided stage convs
  else c.kind = fast16 ? BWDW_FAST16 : BWDW_FAST;                                         // mixed precision: bf16 products
  return c;
}

extern "C" size_t mt_conv3d_bwd_weight_workspace(const mt_conv3d_t* p) {
  if (p == nullptr) return 0;
  BwdWParams P; bwdw_plan(p, &P);
  if (P.nchunks <= 0) return 0;
  size_t bytes = bwdw_partials_bytes(P);
  auto take = [&bytes](const BwdWParams& F) { if (F.nchunks > 0 && bwdw_partials_bytes(F) > bytes) bytes = bwdw_partials_bytes(F); };
  for (int cwp = 0; cwp < 4; ++cwp) {          // every (cw_ok, f32_both) bwdw_resolve can answer (decided with dY's type there)
    BwdWParams F; bwdw_fast_plan(p, &F, (cwp & 1) != 0, (cwp & 2) != 0);
    take(F);
  }
  if (bwdw_use_tr16(p, nullptr)) { BwdWParams F; bwdw_tr16_plan(p, &F); take(F); }
  if (bwdw_is_stem(p, nullptr)) { BwdWParams F; bwdw_stem_plan(p, &F); F.nsg = BW_STEM_WGS; take(F); }      // (the cap, whatever the tile count)
  mt_src_t ys; std::memset(&ys, 0, sizeof(ys));
  if (bwdw_use_gemm(p, &ys) && bwdw_gemm_workspace(p) > bytes) bytes = bwdw_gemm_workspace(p);
  return bytes;
}

extern "C" int mt_conv3d_bwd_weight_kernel_name(const mt_conv3d_t* p, const mt_src_t* ysrc, char* buf, size_t n) {
  if (p == nullptr || ysrc == nullptr || buf == nullptr || n == 0) return MT_EINVAL;
  const BwdwChoice c = bwdw_resolve(p, ysrc);
  const BwGeo g = kBwGeos[c.geo < 0 ? 0 : c.geo];
  switch (c.kind) {
    case BWDW_STEM:    snprintf(buf, n, "conv_bwdw_stem_kernel<%d>", ysrc->dtype); break;
    case BWDW_GENERIC: snprintf(buf, n, "conv_bwdw_kernel"); break;
    case BWDW_GEMM:    snprintf(buf, n, "bwdw_gemm_kernel"); break;
    case BWDW_TR16:    snprintf(buf, n, "conv_bwdw_tr16_kernel<%d, %d>", p->KD, conv_src_dtype(p)); break;
    case BWDW_WINO:    snprintf(buf, n, "conv_bwdw_wino_kernel<2>"); break;
    case BWDW_WINO133: snprintf(buf, n, "conv_bwdw_wino_kernel<2, KD = 1>"); break;
    case BWDW_MARCH:   snprintf(buf, n, "conv_bwdw_march_kernel<3, 3, 1, 1>"); break;
    case BWDW_MARCH16: snprintf(buf, n, "conv_bwdw_march16_kernel<%d, %d, %d>", p->SD, p->src[0].dtype, ysrc->dtype); break;
    case BWDW_FAST16:  snprintf(buf, n, "conv_bwdw_fast16_kernel<%d, %d, %d, %d, %d, %d>", g.KD, g.KH, g.KW, g.SD, g.SH, g.SW); break;
    case BWDW_FAST:    snprintf(buf, n, "conv_bwdw_fast_kernel<%d, %d, %d, %d, %d, %d>", g.KD, g.KH, g.KW, g.SD, g.SH, g.SW); break;
    default: return MT_EINVAL;
  }
  return MT_OK;
}

// storage types of a backward-weight problem: X = p->src (common type), dY = ysrc.  fp32 on both sides is taken by every kernel;
// otherwise it depends on the family that serves the problem (convert with mt_cast).
extern "C" int mt_conv3d_bwd_weight_io_supported(const mt_conv3d_t* p, const mt_src_t* ysrc) {
  if (p == nullptr || ysrc == nullptr) return 0;
  const int xdt = conv_src_dtype(p), ydt = ysrc->dtype;
  if (xdt < 0 || !mt_dtype_ok(ydt)) return 0;
  if (xdt == MT_F32 && ydt == MT_F32) return 1;
  const BwdwChoice c = bwdw_resolve(p, ysrc);
  switch (c.kind) {
    case BWDW_STEM: return (xdt == MT_F32 && ydt != MT_F16) ? 1 : 0;       // fp32 network input, fp32 | bf16 gradient
    case BWDW_GEMM:                                                         // im2col + GEMM: every storage type on either side
    case BWDW_TR16:                                                         // 16-bit X, bf16 dY (part of its eligibility)
    case BWDW_MARCH16:
    case BWDW_FAST16: return 1;                                             // mixed precision, bf16 products (part of their eligibility)
    case BWDW_FAST:                                                         // 16-bit X as channel pairs, the combinations launch_bwdw_fast
      if (c.geo == 0 || conv_fast_vec(p) != 2) return 0;                    // compiles (not for the stride-1 3x3x3 geometry)
      return ((xdt == MT_F16 && (ydt == MT_BF16 || ydt == MT_F32)) || (xdt == MT_BF16 && (ydt == MT_F16 || ydt == MT_BF16))) ? 1 : 0;
    default: return 0;                                                      // generic, fp32 Winograd / marching kernels: fp32 storage only
  }
}

extern "C" int mt_conv3d_bwd_weight(const mt_conv3d_t* p, const mt_src_t* ysrc, float* dw, long s_ci, long s_co,
                                    long s_kd, long s_kh, long s_kw, int accumulate, void* workspace,
                                    size_t workspace_bytes, mt_stream_t stream) {
  MT_REQUIRE(p != nullptr && ysrc != nullptr && dw != nullptr, "bwd_weight: null argument");
  MT_REQUIRE(mt_conv3d_bwd_weight_io_supported(p, ysrc), "bwd_weight: storage types (X %d/%d, dY %d) not taken by the kernel that serves this problem "
             "(ask mt_conv3d_bwd_weight_io_supported, convert with mt_cast)", p->src[0].dtype, p->nsrc == 2 ? p->src[1].dtype : -1, ysrc->dtype);
  MT_REQUIRE(p->nsrc == 1 || p->nsrc == 2, "bwd_weight: nsrc must be 1 or 2");
  MT_REQUIRE(p->KD >= 1 && p->KD <= 3 && p->KH >= 1 && p->KH <= 3 && p->KW >= 1 && p->KW <= 3, "bwd_weight: kernel size must be 1..3");
  MT_REQUIRE(p->dilD == 1 && p->dilH == 1 && p->dilW == 1, "bwd_weight: dilation unsupported");
  MT_REQUIRE(ysrc->C == p->Cout, "bwd_weight: ysrc.C (%d) != Cout (%d)", ysrc->C, p->Cout);
  hipStream_t st = (hipStream_t)stream;
  const BwdwChoice c = bwdw_resolve(p, ysrc);
  if (c.kind == BWDW_GEMM) return launch_bwdw_gemm(p, ysrc, dw, s_ci, s_co, s_kd, s_kh, s_kw, accumulate, workspace, workspace_bytes, st);
  BwdWParams P;
  P.c = *p;
  if (P.c.nsrc == 1) { P.c.src[1] = P.c.src[0]; P.c.src[1].C = 0; }
  P.y = *ysrc;
  switch (c.kind) {
    case BWDW_STEM:    bwdw_stem_plan(p, &P); break;
    case BWDW_GENERIC: bwdw_plan(p, &P); break;
    case BWDW_TR16:    bwdw_tr16_plan(p, &P); break;
    default:           bwdw_fast_plan(p, &P, c.cw_ok, c.f32_both); break;
  }
  MT_REQUIRE(P.nchunks > 0, "bwd_weight: too many channel chunks");
  const size_t need = bwdw_partials_bytes(P);
  if (workspace == nullptr || workspace_bytes < need) { mt_set_error("bwd_weight: workspace %zu < %zu", workspace_bytes, need); return MT_EWORKSPACE; }
  P.part = (float*)workspace;
  const int vec = conv_fast_vec(p);
  int rc = MT_EINVAL;
  switch (c.kind) {
    case BWDW_STEM:    rc = launch_bwdw_stem(P, st); break;
    case BWDW_GENERIC: rc = launch_bwdw_generic(P, st); break;
    case BWDW_TR16:    rc = mt_launch_bwdw_tr16(P, p->KD, conv_src_dtype(p), st); break;
    case BWDW_WINO:    rc = launch_bwdw_wino<3>(P, st); break;
    case BWDW_WINO133: rc = launch_bwdw_wino<1>(P, st); break;
    case BWDW_MARCH: {
      const int yv = ((ysrc->cs & 1) || (p->Cout & 1) || (((uintptr_t)ysrc->ptr) & 7)) ? 1 : 2;
      rc = launch_bwdw_march<3, 3, 1, 1>(P, vec, yv, st);
      break;
    }
    case BWDW_MARCH16:
      MT_REQUIRE(P.nunits > 0 && P.TW == 32, "bwd_weight: the marching kernel needs the column plan of a 4 x 32 tile");
      rc = p->SD == 2 ? launch_bwdw_march16<2>(P, st) : launch_bwdw_march16<1>(P, st);
      break;
    case BWDW_FAST16:  rc = kLaunchFast16[c.geo](P, st); break;
    case BWDW_FAST:    rc = kLaunchFast[c.geo](P, vec, st); break;
  }
  if (rc != MT_OK) return rc;
  return bwdw_launch_reduce(P, dw, s_ci, s_co, s_kd, s_kh, s_kw, accumulate, st);
}
