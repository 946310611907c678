// conv_lds.hip — direct (im2col-free) 3D convolution on fp32 MFMA for gfx950, NDHWC.
//
// Replaces nn.Conv3d on the hot path of the reference (generic_UNet.py:57,67 ConvDropoutNormNonlin,
// conv_blocks.py:49-85,116-213) and, through flipped/transposed packed weights, its autograd
// backward-data.  This unit holds the forward / backward-data kernels with their dispatch, strided
// backward-data and weight packing; backward-weight is conv_bwdw.hip, and the input staging both
// share is conv_stage.h.
//
// Design (MI355X_MICROARCH.md: fp32 MFMA = 64 FLOP/clk/SIMD, 64-cycle v_mfma_f32_32x32x2_f32):
//  * a workgroup (4 waves) owns a TD x TH x TW block of output voxels and 32 output channels;
//  * per <=CK input channels it stages the haloed input tile into LDS once (zero padding,
//    zero-insertion for transposed convs, and InstanceNorm+LeakyReLU applied ON LOAD so the
//    normalised activation never round-trips through HBM), channel stride CK+1 (odd) so the
//    per-voxel A-fragment reads are bank-conflict free;
//  * every (tap, channel pair) is one v_mfma_f32_32x32x2_f32: A = 32 voxels x 2 channels from LDS,
//    B = 2 channels x 32 couts straight from the L2-resident pre-packed weights (256 B coalesced,
//    prefetched one tap ahead), accumulating MT 32x32 tiles per wave in registers;
//  * epilogue adds bias, writes NDHWC (optionally into two destinations = split of a concat
//    gradient, optionally accumulating) and emits per-block (sum, sumsq) partials for InstanceNorm.
#include "mt_common.h"
#include "bwdw_common.h"
#include "conv_stage.h"
#include <cstring>
#include <stdlib.h>
#include <type_traits>


// Block -> (spatial tile, output-channel tile).  Workgroups are dispatched in linear order (x fastest, then y) round-robin over the
// eight XCDs, each with its own L2.  An XCD walks a CONTIGUOUS range of (spatial tile, channel tile) pairs with
// the channel tile fastest — all channel tiles of a spatial tile read the same input patch while it is in that L2 — and the
// spatial tiles in the order D, H, W (W slowest): the tiles resident on an XCD at one time then form a compact D x H block at one
// w position, so the halo rows (TH + 2 rows fetched for TH outputs: the expensive direction) are shared in L2 instead of being
// fetched again a whole D x W plane later.
__device__ __forceinline__ int mt_block_decode(int& ntile) {
  const int ny = (int)gridDim.y;
  const int b = mt_xcd_remap((int)(blockIdx.x + gridDim.x * blockIdx.y), (int)(gridDim.x * ny));
  const int t = b / ny;
  ntile = b - t * ny;
  return t;
}
// spatial tile index -> (td, th, tw, sample)
__device__ __forceinline__ void mt_tile_coords(int tile, int tilesD, int tilesH, int tilesW, int& td, int& th, int& tw, int& nb) {
  td = tile % tilesD; tile /= tilesD;
  th = tile % tilesH; tile /= tilesH;
  tw = tile % tilesW;
  nb = tile / tilesW;
}

// ------------------------------------------------------------------------------------------------
// FAST staging: compile-time tile geometry (3x3x3 / stride 1 / no zero insertion).  Buffer loads with hardware
// bounds checking return 0 for out-of-range lanes (zero padding costs no branch): a lane whose w or channel is
// out of range carries byte offset 0x80000000, which stays >= num_records after adding the row offset.  All
// RPW x NI loads of a wave are in flight before the first LDS store.
template <int CK, int LD, int LH, int LW>
__device__ __forceinline__ void mt_stage_fast(float* __restrict__ lds, const mt_conv3d_t& c, const ConvChunk ch,
                                              int nb, int ud0, int uh0, int uw0, int lane, int wave) {
  constexpr int VPS = 64 / CK, NI = (LW + VPS - 1) / VPS, R = LD * LH, RPW = (R + 3) / 4;
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
  const int cs = S.cs;
  const size_t sample_elems = (size_t)c.Di * c.Hi * c.Wi * cs;
  __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)(S.ptr + (size_t)nb * sample_elems), 0, (int)(sample_elems * 4), 0x00020000);
  int voff[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int lw = vl + i * VPS;
    const int uw = uw0 + lw;
    const bool ok = cvalid && (lw < LW) && ((unsigned)uw < (unsigned)c.Wi);
    voff[i] = ok ? (uw * cs + ch.c0 + cl) * 4 : (int)0x80000000;
  }
  constexpr int RG = (RPW > 3) ? 3 : RPW;       // rows per batch: RG*NI loads in flight, bounded register use
#pragma unroll
  for (int r0 = 0; r0 < RPW; r0 += RG) {
    float v[RG][NI];
    bool rv[RG];
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      const int row = wave + 4 * (r0 + q);
      const int ld = row / LH, lhh = row % LH;
      const int ud = ud0 + ld, uh = uh0 + lhh;
      rv[q] = (r0 + q < RPW) && (row < R) && ((unsigned)ud < (unsigned)c.Di) && ((unsigned)uh < (unsigned)c.Hi);
      if (rv[q]) {
        const int srow = (ud * c.Hi + uh) * c.Wi * cs * 4;
#pragma unroll
        for (int i = 0; i < NI; ++i) v[q][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff[i] + srow, 0, 0));
      } else {
#pragma unroll
        for (int i = 0; i < NI; ++i) v[q][i] = 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      const int row = wave + 4 * (r0 + q);
      if (r0 + q < RPW && row < R) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int lw = vl + i * VPS;
          if ((i + 1) * VPS <= LW || lw < LW) {
            float x = v[q][i];
            if (has_aff) x = (rv[q] && voff[i] >= 0) ? mt_lrelu(fmaf(x, sc, sh), slope) : 0.f;
            const int lv = row * LW + lw;
            lds[lv * CK + (cl ^ ((lv >> 1) & (CK - 1)))] = x;
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// MFMA phase of one staged channel chunk: for every tap, NK channel pairs x MT voxel tiles of
// v_mfma_f32_32x32x2_f32.  Straight-line per tap (NK is a compile-time constant, no branches), and the
// A fragments (LDS) and B fragments (packed weights, L2) of tap t+1 are fetched into a second register
// set while the MFMAs of tap t issue, so neither LDS nor L2 latency sits in front of the matrix pipe.
struct TapWalk { int KH, KW, step_w, step_h, step_d; };

template <int MT, int NK>
struct ConvFrag { float a[MT][NK]; float b[NK]; };

// swizzled LDS dword index of channel lhalf*NK of voxel lv; channel lhalf*NK + kp is this value ^ kp
template <int CK>
__device__ __forceinline__ int conv_a0(int lv, int lhalf) { return lv * CK + ((lhalf * (CK / 2)) ^ ((lv >> 1) & (CK - 1))); }
// weights: layout 1 of mt_pack_conv_weights, wq points at this lane's float4 of (tap, q = 0)
template <int NK>
__device__ __forceinline__ void conv_load_b(float (&b)[NK], const float* __restrict__ wq) {
#pragma unroll
  for (int q = 0; q < NK / 4; ++q) {
    const f32x4 v = *(const f32x4*)(wq + q * 256);
#pragma unroll
    for (int e = 0; e < 4; ++e) b[q * 4 + e] = v[e];
  }
}

// One tap = NK steps; step kp issues the loads of channel pair kp of the NEXT tap (1 weight load, MT LDS reads with
// their XOR) and then the MT MFMAs of channel pair kp of the CURRENT tap.  sched_barrier(0) between steps pins this
// even interleave: non-matrix instructions sit one-per-gap behind 64-cycle MFMAs instead of in a ~70-instruction bunch
// that idles the matrix pipe (tools/ubench/mfma_peak.hip: interleaved fillers are free, bunched ones are not).
template <int MT, int NK>
__device__ __forceinline__ void conv_tap_step(ConvFrag<MT, NK>& nxt, const ConvFrag<MT, NK>& cur,
                                              const float* __restrict__ lds, const int (&abase)[MT], int off,
                                              const float* __restrict__ wq, int lhalf, f32x16 (&acc)[MT]) {
  int a0[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) a0[m] = conv_a0<2 * NK>(abase[m] + off, lhalf);
  conv_load_b<NK>(nxt.b, wq);
#pragma unroll
  for (int kp = 0; kp < NK; ++kp) {
#pragma unroll
    for (int m = 0; m < MT; ++m) nxt.a[m][kp] = lds[a0[m] ^ kp];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[m][kp], cur.b[kp], acc[m], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int MT, int NK>
__device__ __forceinline__ void conv_chunk_compute(const float* __restrict__ lds, const int (&abase)[MT],
                                                   const float* __restrict__ wq, int ntaps, int wstride,
                                                   const TapWalk tw, int lhalf, f32x16 (&acc)[MT]) {
  ConvFrag<MT, NK> f0, f1;
  int off = 0, kw = 0, kh = 0, tap = 0;
  auto advance = [&]() {   // move (off, wq) to the next tap; stays on the last tap at the end
    if (tap + 1 < ntaps) {
      off += tw.step_w;
      if (++kw == tw.KW) { kw = 0; off += tw.step_h; if (++kh == tw.KH) { kh = 0; off += tw.step_d; } }
      wq += wstride;
    }
    ++tap;
  };
  {  // prologue: fragments of tap 0
    conv_load_b<NK>(f0.b, wq);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int a0 = conv_a0<2 * NK>(abase[m], lhalf);
#pragma unroll
      for (int kp = 0; kp < NK; ++kp) f0.a[m][kp] = lds[a0 ^ kp];
    }
  }
  while (tap + 2 <= ntaps) {
    advance();
    __builtin_amdgcn_sched_barrier(0);
    conv_tap_step<MT, NK>(f1, f0, lds, abase, off, wq, lhalf, acc);
    advance();
    __builtin_amdgcn_sched_barrier(0);
    conv_tap_step<MT, NK>(f0, f1, lds, abase, off, wq, lhalf, acc);
  }
  if (tap < ntaps) {
#pragma unroll
    for (int kp = 0; kp < NK; ++kp)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(f0.a[m][kp], f0.b[kp], acc[m], 0, 0, 0);
  }
}

// ------------------------------------------------------------------------------------------------
template <int MW, int RH, int TD, int CK, bool FAST>
__global__ __launch_bounds__(256) void conv_fwd_kernel(const ConvKParams P) {
  constexpr int MH = 32 / MW;
  constexpr int TH = MH * RH;
  constexpr int TW = MW;
  constexpr int NMT = TD * RH;
  static_assert(NMT % 4 == 0, "M tiles must split over 4 waves");
  constexpr int MT = NMT / 4;
  constexpr int NKP = CK / 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;

  int ntile, td, th, tw, nb;
  mt_tile_coords(mt_block_decode(ntile), P.tilesD, P.tilesH, P.tilesW, td, th, tw, nb);
  const int sb = (td * P.tilesH + th) * P.tilesW + tw;

  // FAST: 3x3x3, stride 1, pad 1, no zero insertion -> the whole tile geometry is compile-time
  const int KD = FAST ? 3 : c.KD, KH = FAST ? 3 : c.KH, KW = FAST ? 3 : c.KW;
  const int SD = FAST ? 1 : c.SD, SH = FAST ? 1 : c.SH, SW = FAST ? 1 : c.SW;
  const int LD = (TD - 1) * SD + KD, LH = (TH - 1) * SH + KH, LW = (TW - 1) * SW + KW;
  const int od0 = td * TD, oh0 = th * TH, ow0 = tw * TW;
  const int ud0 = od0 * SD - (FAST ? 1 : c.PD), uh0 = oh0 * SH - (FAST ? 1 : c.PH), uw0 = ow0 * SW - (FAST ? 1 : c.PW);

  // per-lane LDS base of each M tile: voxel (dm, row, col) of the tile, channel half lhalf
  int abase[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mt = wave * MT + m;
    const int dm = mt / RH, rh = mt % RH;
    const int r = li / MW, col = li % MW;
    const int row = rh * MH + r;
    abase[m] = (dm * SD * LH + row * SH) * LW + col * SW;   // voxel index inside the LDS tile
  }

  f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[m][j] = 0.f;

  // De-phase the workgroups that share a CU: all workgroups have identical duration, so without this they stage
  // together and then contend for the matrix pipe together.  The k-th initially resident workgroup of a CU (blocks
  // are dealt round-robin: slot = blockIdx / 256) starts k*stagger later; later workgroups inherit the offset.
  // Pure performance heuristic — correctness never depends on placement or timing.
  if (P.stagger > 0 && blockIdx.y == 0) {
    const int slot = blockIdx.x >> 8;
    if (slot > 0 && slot < 4)
      for (int i = 0; i < slot * P.stagger; ++i) __builtin_amdgcn_s_sleep(100);
  }

  long long* tsbuf = (P.dbg & 16) ? ((long long*)c.out1 + ((size_t)blockIdx.x * 4 + wave) * 16) : nullptr;
  int tsn = 0;
#define MT_STAMP() do { if (tsbuf && lane == 0 && tsn < 16) tsbuf[tsn++] = __builtin_readcyclecounter(); } while (0)
  MT_STAMP();
  const int ntaps = FAST ? 27 : P.ntaps;
  for (int ch = 0; ch < P.nchunks; ++ch) {
    const ConvChunk cc = P.chunk[ch];
    const float* wq = c.wpack + ((size_t)(ntile * P.nchunks + ch) * ntaps) * (NKP * 64) + lane * 4;
    __syncthreads();  // previous chunk's LDS reads are done
    MT_STAMP();
    if (!(P.dbg & 1)) {
      if constexpr (FAST) mt_stage_fast<CK, TD + 2, TH + 2, TW + 2>(lds, c, cc, nb, ud0, uh0, uw0, lane, wave);
      else mt_stage_input<CK>(lds, c, cc, nb, ud0, uh0, uw0, LD, LH, LW, lane, wave);
    }
    MT_STAMP();
    __syncthreads();
    MT_STAMP();

    // channels beyond cc.ck are zero both in LDS and in the packed weights: always run all NKP pairs (one
    // straight-line code path keeps the register allocation small; <= 1/16 padded work for C = 30, 60, 120)
    const TapWalk tw0{KH, KW, 1, LW - KW, (LH - KH) * LW};   // tap walk in voxels
    if (!(P.dbg & 8)) conv_chunk_compute<MT, NKP>(lds, abase, wq, ntaps, (P.dbg & 2) ? 0 : NKP * 64, tw0, lhalf, acc);
    MT_STAMP();
  }

  // ---- epilogue: bias, store, InstanceNorm partial statistics
  const int co = ntile * 32 + li;
  const bool covalid = co < c.Cout;
  const float bv = (c.bias != nullptr && covalid) ? c.bias[co] : 0.f;
  float* optr;
  int ocs, cofs;
  if (co < c.csplit) { optr = c.out0; ocs = c.ocs0; cofs = co; }
  else               { optr = c.out1; ocs = c.ocs1; cofs = co - c.csplit; }
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mt = wave * MT + m;
    const int dm = mt / RH, rh = mt % RH;
    const int od = od0 + dm;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int iv = (j & 3) + 8 * (j >> 2) + 4 * lhalf;
      const int r = iv / MW, col = iv % MW;
      const int oh = oh0 + rh * MH + r, ow = ow0 + col;
      const bool ok = covalid && (od < c.Do) && (oh < c.Ho) && (ow < c.Wo) && !(P.dbg & 4);
      if (ok) {
        const size_t idx = ((size_t)((size_t)((size_t)nb * c.Do + od) * c.Ho + oh) * c.Wo + ow) * ocs + cofs;
        float v = acc[m][j] + bv;
        if (c.accumulate) v += optr[idx];
        optr[idx] = v;
        s1 += v;
        s2 += v * v;
      }
    }
  }
  MT_STAMP();
  if (c.stats_part != nullptr) {
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    __syncthreads();  // LDS tile no longer needed
    if (lhalf == 0) { lds[(wave * 32 + li) * 2] = s1; lds[(wave * 32 + li) * 2 + 1] = s2; }
    __syncthreads();
    if (tid < 32 && (ntile * 32 + tid) < c.Cout) {
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) { t1 += lds[(w * 32 + tid) * 2]; t2 += lds[(w * 32 + tid) * 2 + 1]; }
      float* sp = c.stats_part + ((size_t)((size_t)nb * P.nsb + sb) * c.Cout + ntile * 32 + tid) * 2;
      sp[0] = t1; sp[1] = t2;
    }
  }
  MT_STAMP();
#undef MT_STAMP
}

// ================================================================================================
// FAST v2 forward kernel (3x3x3, stride 1, pad 1): ZERO vector-ALU instructions inside the MFMA loop.
//
// Measured on gfx950 (tools/ubench/mfma_fill.hip): v_mfma_f32_32x32x2_f32 runs on the FP32 vector datapath, so every
// VALU instruction interleaved with it costs matrix time (+15 cycles for the first, ~6 per further one), while LDS
// reads (~1 cycle), scalar ALU and s_waitcnt are free.  Hence:
//   * LDS image [voxel][20 dwords] (16 channel slots + 4 pad): 16-byte aligned voxels, and the 80-byte stride makes
//     ds_read_b128 over 16 consecutive voxels bank-conflict free (slot = 5*lv mod 16 is a bijection) without any XOR;
//   * K-permutation (weight layout 1): lane half h contracts channels 8h..8h+7, i.e. 8 CONTIGUOUS floats of its voxel
//     = two ds_read_b128 per M tile per tap;
//   * the 27 taps are fully unrolled: every LDS address is (per-lane base) + compile-time immediate;
//   * weights arrive as two global_load_dwordx4 per tap from a wave-uniform pointer + lane offset.
// The staging pass uses 8-byte buffer loads (2 channels) with hardware bounds checking and ds_write_b64.
__device__ __constant__ float kWinoG[4][3] = {{1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.f, 0.f, 1.f}};
#ifndef CF_ABL
#define CF_ABL 0   // compile-time timing ablations of conv_fast_kernel: 1 skip staging, 4 skip epilogue, 8 skip MFMA
#endif

// Lean staging of a haloed input tile (LD x LH x LW voxels x 16 channels) into the LDS image [row][LWP voxels][20 dwords].
// 64 lanes = VPS voxels x LPV channel groups; a wave owns rows wave, wave+4, ...; NI steps cover a row.  Validity is carried as
// DATA, never as control flow: out-of-volume rows/voxels load through the buffer descriptor's bounds check (offset
// 0x80000000 -> 0) and are zeroed by scale = shift = 0 (rows, channel slots) or an AND mask (voxels); every load is
// (per-lane constant offset, scalar row offset) and every store (one base VGPR + immediate).  All loads of a batch are issued
// before the first store.  The staging VALU work matters twice: it delays this wave AND it steals issue cycles from the
// other workgroup's MFMAs on the same SIMD.
// LDS rows are padded to a multiple of 4 (stage_rows) so that every wave stores RPW rows; LWP >= NI*VPS makes the last step
// of a row unconditional, otherwise (LDS too small for the padding) it is predicated.
template <int LD, int LH, int LW, int VEC>
__device__ __forceinline__ void mt_stage_fast2(float* __restrict__ lds, const mt_conv3d_t& c, const ConvChunk ch,
                                               int nb, int ud0, int uh0, int uw0, int lane, int wave) {
  constexpr int LPV = FCK / VEC, VPS = 64 / LPV, NI = (LW + VPS - 1) / VPS, R = LD * LH, RPW = (R + 3) / 4;
  constexpr int LWP = stage_lwp<LD, LH, LW, VEC>();
  constexpr bool PADW = LWP >= NI * VPS;
  constexpr int RG = (RPW * NI * VEC > 64) ? (RPW + 1) / 2 : RPW;      // rows per batch (<= ~64 registers in flight)
  const mt_src_t& S = c.src[ch.src];
  const int cl = (lane % LPV) * VEC, vl = lane / LPV;
  const bool has_aff = S.scale != nullptr;
  float sc[VEC], sh[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const bool cv = (cl + e) < ch.ck;
    sc[e] = cv ? 1.f : 0.f; sh[e] = 0.f;                    // channel slots beyond the chunk stage as zeros
    if (has_aff && cv) {
      sc[e] = S.scale[(size_t)nb * S.C + ch.c0 + cl + e];
      sh[e] = S.shift[(size_t)nb * S.C + ch.c0 + cl + e];
    }
  }
  const float slope = has_aff ? S.slope : 1.f;
  const int cs = S.cs;
  const size_t sample_elems = (size_t)c.Di * c.Hi * c.Wi * cs;
  __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)(S.ptr + (size_t)nb * sample_elems), 0, (int)(sample_elems * 4), 0x00020000);
  int voff[NI];
  unsigned mval[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int lw = vl + i * VPS;
    const int uw = uw0 + lw;
    const bool ok = (lw < LW) && ((unsigned)uw < (unsigned)c.Wi);
    voff[i] = ok ? (uw * cs + ch.c0 + cl) * 4 : (int)0x80000000;
    mval[i] = ok ? 0xffffffffu : 0u;
  }
  float* lbase = lds + (wave * LWP + vl) * FCKP + cl;
  const int rowbytes = c.Wi * cs * 4;
#pragma unroll
  for (int r0 = 0; r0 < RPW; r0 += RG) {
    float v[RG][NI][VEC];
    int rowm[RG];
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      if (r0 + q < RPW) {
        const int row = wave + 4 * (r0 + q);
        const int ld = row / LH, lhh = row - ld * LH;
        const int ud = ud0 + ld, uh = uh0 + lhh;
        rowm[q] = ((row < R) && ((unsigned)ud < (unsigned)c.Di) && ((unsigned)uh < (unsigned)c.Hi)) ? -1 : 0;
        const int srow = ((ud * c.Hi + uh) & rowm[q]) * rowbytes;
        const int oob = ~rowm[q] & (int)0x80000000;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          if constexpr (VEC == 2) {
            // NB: bit_cast the WHOLE 64-bit result; indexing the builtin's return type yields the first dword twice
            const float2 t = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff[i] | oob, srow, 0));
            v[q][i][0] = t.x;
            v[q][i][1] = t.y;
          } else {
            v[q][i][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff[i] | oob, srow, 0));
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      if (r0 + q < RPW) {
        float scq[VEC], shq[VEC];        // a row outside the volume: scale = shift = 0 -> exact zeros
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          scq[e] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, sc[e]) & (unsigned)rowm[q]);
          shq[e] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, sh[e]) & (unsigned)rowm[q]);
        }
        float* lrow = lbase + 4 * (r0 + q) * (LWP * FCKP);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          float x[VEC];
          if constexpr (VEC == 2) {       // packed fp32 math: one v_pk_fma_f32 + one v_pk_mul_f32 per two channels
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            f32x2 xv2, sc2, sh2, sl2;
            xv2[0] = v[q][i][0]; xv2[1] = v[q][i][1]; sc2[0] = scq[0]; sc2[1] = scq[1]; sh2[0] = shq[0]; sh2[1] = shq[1];
            sl2[0] = slope; sl2[1] = slope;
            const f32x2 t = __builtin_elementwise_fma(xv2, sc2, sh2);
            const f32x2 u = t * sl2;
            // LeakyReLU with 0 <= slope <= 1 (checked on the host for these kernels) is max(t, slope*t)
            x[0] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, fmaxf(t[0], u[0])) & mval[i]);
            x[1] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, fmaxf(t[1], u[1])) & mval[i]);
          } else {
            const float t = fmaf(v[q][i][0], scq[0], shq[0]);
            x[0] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, fmaxf(t, t * slope)) & mval[i]);
          }
          if (PADW || (i + 1) * VPS <= LW || vl + i * VPS < LW) {
            if constexpr (VEC == 2) {
              float2 t; t.x = x[0]; t.y = x[1];
              *(float2*)(lrow + i * VPS * FCKP) = t;
            } else {
              lrow[i * VPS * FCKP] = x[0];
            }
          }
        }
      }
    }
  }
}


template <int MT>
struct FastFrag { f32x4 a[MT][2]; f32x4 b[2]; };

template <int MT>
__device__ __forceinline__ void fast_frag_mfma(const FastFrag<MT>& f, f32x16 (&acc)[MT]) {
#pragma unroll
  for (int kp = 0; kp < 8; ++kp)
#pragma unroll
    for (int m = 0; m < MT; ++m)
      acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[m][kp >> 2][kp & 3], f.b[kp >> 2][kp & 3], acc[m], 0, 0, 0);
}
// One 16-channel chunk of a 3x3x3 conv, all 27 taps unrolled with compile-time LDS offsets.  The weight (B) fragments come from
// L2 with a latency of more than one tap's worth of MFMAs, so they are prefetched BPF taps ahead through a small register ring;
// the A fragments (LDS) one tap ahead.
#ifndef CF_BPF
#define CF_BPF 3
#endif
template <int MT, int LH, int LW, int KD = 3>
__device__ __forceinline__ void fast_chunk(const float* __restrict__ lds, const int (&abase)[MT], const float* __restrict__ wlane,
                                           f32x16 (&acc)[MT]) {
  constexpr int NB = CF_BPF + 1, NTAP = KD * 9;       // KD = 1: the 1x3x3 convolutions of the residual encoder's first stage
  f32x4 b[NB][2];
  f32x4 a[2][MT][2];
#pragma unroll
  for (int t = 0; t < CF_BPF; ++t) {
    b[t][0] = *(const f32x4*)(wlane + t * 512);
    b[t][1] = *(const f32x4*)(wlane + t * 512 + 256);
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    a[0][m][0] = *(const f32x4*)(lds + abase[m]);
    a[0][m][1] = *(const f32x4*)(lds + abase[m] + 4);
  }
#pragma unroll
  for (int t = 0; t < NTAP; ++t) {
    if (t + CF_BPF < NTAP && !(CF_ABL & 64)) {
      b[(t + CF_BPF) % NB][0] = *(const f32x4*)(wlane + (t + CF_BPF) * 512);
      b[(t + CF_BPF) % NB][1] = *(const f32x4*)(wlane + (t + CF_BPF) * 512 + 256);
    }
    if (t + 1 < NTAP && !(CF_ABL & 32)) {
      const int t1 = t + 1;
      const int toff = (((t1 / 9) * LH + (t1 / 3) % 3) * LW + t1 % 3) * FCKP;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        a[t1 & 1][m][0] = *(const f32x4*)(lds + abase[m] + toff);
        a[t1 & 1][m][1] = *(const f32x4*)(lds + abase[m] + toff + 4);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kp = 0; kp < 8; ++kp)
#pragma unroll
      for (int m = 0; m < MT; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[(CF_ABL & 32) ? 0 : (t & 1)][m][kp >> 2][kp & 3], b[(CF_ABL & 64) ? 0 : (t % NB)][kp >> 2][kp & 3], acc[m], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int MW, int RH, int TD, int VEC, int KD = 3>
__global__ __launch_bounds__(256) void conv_fast_kernel(const ConvKParams P) {
  constexpr int MH = 32 / MW, TH = MH * RH, TW = MW, NMT = TD * RH, MT = NMT / 4;
  constexpr int LD = TD + KD - 1, LH = TH + 2, LW = TW + 2, LWP = stage_lwp<LD, LH, LW, VEC>();
  static_assert(NMT % 4 == 0, "M tiles must split over 4 waves");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  int ntile, td, th, tw, nb;
  mt_tile_coords(mt_block_decode(ntile), P.tilesD, P.tilesH, P.tilesW, td, th, tw, nb);
  const int sb = (td * P.tilesH + th) * P.tilesW + tw;
  const int od0 = td * TD, oh0 = th * TH, ow0 = tw * TW;

  int abase[MT];   // dword index of (voxel of this lane in M tile m, channel 8*lhalf)
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mt = wave * MT + m;
    const int dm = mt / RH, rh = mt % RH;
    const int r = li / MW, col = li % MW;
    abase[m] = ((dm * LH + rh * MH + r) * LWP + col) * FCKP + lhalf * 8;
  }
  f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[m][j] = 0.f;

  for (int ch = 0; ch < P.nchunks; ++ch) {
    const ConvChunk cc = P.chunk[ch];
    const float* wlane = c.wpack + (size_t)(ntile * P.nchunks + ch) * (KD * 9 * 512) + lane * 4;
    if (!(CF_ABL & 16)) __syncthreads();
    if (!(CF_ABL & 1)) mt_stage_fast2<LD, LH, LW, VEC>(lds, c, cc, nb, od0 - (KD - 1) / 2, oh0 - 1, ow0 - 1, lane, wave);
    if (!(CF_ABL & 16)) __syncthreads();
    if (!(CF_ABL & 8)) fast_chunk<MT, LH, LWP, KD>(lds, abase, wlane, acc);
  }

  // ---- epilogue: bias, store, statistics.  Stores go through a buffer descriptor: per-lane byte offset (column part)
  // + wave-uniform scalar offset per (M tile, register) -> no vector address arithmetic; out-of-volume lanes of
  // boundary tiles get offset 0x80000000 (dropped by the hardware bounds check).
  if (CF_ABL & 4) { if (acc[0][0] == 12345.678f) c.out0[0] = acc[MT - 1][3]; return; }
  const int co = ntile * 32 + li;
  const bool covalid = co < c.Cout;
  const float bv = (c.bias != nullptr && covalid) ? c.bias[co] : 0.f;
  float* optr; int ocs, cofs;
  if (co < c.csplit) { optr = c.out0; ocs = c.ocs0; cofs = co; }
  else               { optr = c.out1; ocs = c.ocs1; cofs = co - c.csplit; }
  float s1 = 0.f, s2 = 0.f;
  const bool interior = (od0 + TD <= c.Do) && (oh0 + TH <= c.Ho) && (ow0 + TW <= c.Wo);   // block-uniform
  const size_t out_sample = (size_t)c.Do * c.Ho * c.Wo;
  // two descriptors (out0 / out1 when the output is a split concat gradient); each lane uses the one of its channel
  __amdgpu_buffer_rsrc_t r0d = __builtin_amdgcn_make_buffer_rsrc((void*)(c.out0 + (size_t)nb * out_sample * c.ocs0), 0,
                                                                 (int)(out_sample * c.ocs0 * 4), 0x00020000);
  const bool split = c.csplit < c.Cout;
  __amdgpu_buffer_rsrc_t r1d = r0d;
  if (split) r1d = __builtin_amdgcn_make_buffer_rsrc((void*)(c.out1 + (size_t)nb * out_sample * c.ocs1), 0,
                                                     (int)(out_sample * c.ocs1 * 4), 0x00020000);
  const bool use1 = split && !(co < c.csplit);
  (void)optr;
  const int lane_col = 4 * lhalf;    // column part of iv that depends on the lane
  const int loff = covalid ? (lane_col * ocs + cofs) * 4 : (int)0x80000000;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mt = wave * MT + m;
    const int dm = mt / RH, rh = mt % RH;
    const int od = od0 + dm;
    const int vox0 = ((od * c.Ho) + (oh0 + rh * MH)) * c.Wo + ow0;    // within the sample, wave-uniform
    auto jgeom = [&](int j, int& off, int& so0, int& so1) {
      const int ivj = (j & 3) + 8 * (j >> 2);           // lane-independent part of the voxel index in the M tile
      const int r = ivj / MW, colj = ivj % MW;          // (4*lhalf never crosses an MW boundary: MW >= 8)
      off = loff;
      if (!interior) {
        const bool ok = (od < c.Do) && (oh0 + rh * MH + r < c.Ho) && (ow0 + colj + lane_col < c.Wo);
        off = ok ? loff : (int)0x80000000;
      }
      // scalar offsets differ per destination only through ocs: compute both (SALU) and select per lane once
      so0 = (vox0 + r * c.Wo + colj) * c.ocs0 * 4;
      so1 = (vox0 + r * c.Wo + colj) * c.ocs1 * 4;
    };
    // accumulate: the 16 old values of this M tile are requested together, before the first store (one load -> add -> store
    // round trip per element otherwise: the residual encoder's 30 -> 30 backward-data at full resolution)
    float prev[16];
    if (c.accumulate) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        int off, so0, so1; jgeom(j, off, so0, so1);
        if (!split) prev[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r0d, off, so0, 0));
        else {
          const int offa = use1 ? (int)0x80000000 : off, offb = use1 ? off : (int)0x80000000;
          prev[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r0d, offa, so0, 0)) +
                    __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r1d, offb, so1, 0));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      int off, so0, so1; jgeom(j, off, so0, so1);
      float v = acc[m][j] + bv;
      if (c.accumulate) v += prev[j];
      if (!split) {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r0d, off, so0, 0);
      } else {
        // lanes of the two destinations take different descriptors: predicate by offset (OOB = no-op)
        const int offa = use1 ? (int)0x80000000 : off, offb = use1 ? off : (int)0x80000000;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r0d, offa, so0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r1d, offb, so1, 0);
      }
      if (interior) { s1 += v; s2 = fmaf(v, v, s2); }
      else if (off >= 0) { s1 += v; s2 = fmaf(v, v, s2); }
    }
  }
  if (!covalid) { s1 = 0.f; s2 = 0.f; }
  if (c.stats_part != nullptr) {
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    __syncthreads();
    if (lhalf == 0) { lds[(wave * 32 + li) * 2] = s1; lds[(wave * 32 + li) * 2 + 1] = s2; }
    __syncthreads();
    if (tid < 32 && (ntile * 32 + tid) < c.Cout) {
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) { t1 += lds[(w * 32 + tid) * 2]; t2 += lds[(w * 32 + tid) * 2 + 1]; }
      float* sp = c.stats_part + ((size_t)((size_t)nb * P.nsb + sb) * c.Cout + ntile * 32 + tid) * 2;
      sp[0] = t1; sp[1] = t2;
    }
  }
}

#include "conv_bf16.inc"

// ================================================================================================
// Forward 3x3x3 convolution with stride (2,2,2) or (1,2,2), pad 1 (the first conv of every encoder stage,
// generic_UNet.py:263-278) on the FAST design with compile-time taps.  Tile = 2 x 4 x 8 outputs x 64 output channels:
// the haloed input tile ((TD-1)*SD+3) x 9 x 17 voxels x 16 channels stays under 64 KiB so two workgroups share a CU; the four
// waves are 2 M tiles (one output plane each) x 2 N tiles, so every staged voxel feeds 64 output channels.
// BF = true (mixed precision, mt_conv3d_t.mma == 1): bf16 LDS image and v_mfma_f32_32x32x16_bf16 through mt_stage_bf16 / bf16_chunk.
// XS / OS (BF only): storage types of the source / destination (mt_src_t.dtype, mt_conv3d_t.odtype); MTY: matrix type (mt_stage_bf16).
#ifndef FS_ABL
#define FS_ABL 0   // compile-time timing ablations of conv_fast_strided_kernel (fp32): 1 no staging, 4 no epilogue, 8 no MFMAs
#endif
template <int SD, int SH, int SW, int VEC, bool BF = false, int XS = MT_F32, int OS = MT_F32, int MTY = MT_BF16>
__global__ __launch_bounds__(256) void conv_fast_strided_kernel(const ConvKParams P) {
  static_assert(BF || (XS == MT_F32 && OS == MT_F32), "16-bit storage is served by the 16-bit matrix path");
  constexpr bool OB = OS != MT_F32;
  constexpr int TD = 2, TH = 4, TW = 8;
  constexpr int LD = (TD - 1) * SD + 3, LH = (TH - 1) * SH + 3, LW = (TW - 1) * SW + 3;
  constexpr int LWP = BF ? bstage_lwp<LD, LH, LW, VEC, 4>() : stage_lwp<LD, LH, LW, VEC>();
  constexpr int PITCH = BF ? BFP : FCKP;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  int by, td, th, tw, nb;
  mt_tile_coords(mt_block_decode(by), P.tilesD, P.tilesH, P.tilesW, td, th, tw, nb);
  const int dm = wave & 1, nt2 = wave >> 1;
  const int ntile_raw = by * 2 + nt2;
  const bool nt_ok = ntile_raw * 32 < c.Cout;           // wave-uniform: an odd number of 32-channel tiles leaves one wave idle
  const int ntile = nt_ok ? ntile_raw : 0;
  const int sb = (td * P.tilesH + th) * P.tilesW + tw;
  const int od0 = td * TD, oh0 = th * TH, ow0 = tw * TW;

  int abase[1];
  abase[0] = ((dm * SD * LH + (li >> 3) * SH) * LWP + (li & 7) * SW) * PITCH + lhalf * (BF ? 4 : 8);
  f32x16 accb[1][1];
  f32x16 (&acc)[1] = accb[0];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[0][j] = 0.f;

  for (int ch = 0; ch < P.nchunks; ++ch) {
    const ConvChunk cc = P.chunk[ch];
    __syncthreads();
    if constexpr (BF) {
      const unsigned* wlane = (const unsigned*)c.wpack + (size_t)(ntile * P.nchunks + ch) * (27 * 256) + lane * 4;
      mt_stage_bf16<LD, LH, LW, VEC, 4, XS, MTY>((unsigned*)lds, c, cc, nb, od0 * SD - 1, oh0 * SH - 1, ow0 * SW - 1, lane, wave);
      __syncthreads();
      const int abase3[1][3] = {{abase[0], abase[0], abase[0]}};
      bf16_chunk<1, 1, LH, LWP, 3, MTY>((const unsigned*)lds, abase3, wlane, 0, accb);
    } else {
      const float* wlane = c.wpack + (size_t)(ntile * P.nchunks + ch) * (27 * 512) + lane * 4;
      if (!(FS_ABL & 1)) mt_stage_fast2<LD, LH, LW, VEC>(lds, c, cc, nb, od0 * SD - 1, oh0 * SH - 1, ow0 * SW - 1, lane, wave);
      __syncthreads();
      if (!(FS_ABL & 8)) fast_chunk<1, LH, LWP>(lds, abase, wlane, acc);
    }
  }
  if ((FS_ABL & 4) && acc[0][0] != 12345.f) return;

  const int co = ntile_raw * 32 + li;
  const bool covalid = nt_ok && co < c.Cout;
  const float bv = (c.bias != nullptr && covalid) ? c.bias[co] : 0.f;
  const int ocs = c.ocs0;
  const size_t out_sample = (size_t)c.Do * c.Ho * c.Wo;
  constexpr int OEB = mt_ebytes<OS>();
  __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)c.out0 + (size_t)nb * out_sample * ocs * OEB), 0,
                                                                (int)(out_sample * ocs * OEB), 0x00020000);
  const int od = od0 + dm;
  float s1 = 0.f, s2 = 0.f;
  if constexpr (OB) {                  // channel-pair dwords (mt_pair_exchange): even lanes store row j, odd lanes row j + 1
    const bool odd = li & 1;
    const int coe = co & ~1;
    const bool pvalid = nt_ok && coe + 1 < c.Cout;
    float q1[2] = {0.f, 0.f}, q2[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
      const int iv = (j & 3) + 8 * (j >> 2) + 4 * lhalf + (odd ? 1 : 0);
      const int oh = oh0 + (iv >> 3), ow = ow0 + (iv & 7);
      const bool ok = pvalid && (od < c.Do) && (oh < c.Ho) && (ow < c.Wo);
      const int off = ok ? (((od * c.Ho + oh) * c.Wo + ow) * ocs + coe) * 2 : (int)0x80000000;
      float a, b;
      mt_pair_exchange(acc[0][j] + bv, acc[0][j + 1] + bv, odd, a, b);
      if (c.accumulate) { const unsigned pv = __builtin_amdgcn_raw_buffer_load_b32(rd, off, 0, 0); a += mt_lo16<OS>(pv); b += mt_hi16<OS>(pv); }
      const unsigned pk = mt_pk16<OS>(a, b);
      __builtin_amdgcn_raw_buffer_store_b32(pk, rd, off, 0, 0);
      if (ok) {
        const float ar = mt_lo16<OS>(pk), br = mt_hi16<OS>(pk);
        q1[0] += ar; q2[0] = fmaf(ar, ar, q2[0]); q1[1] += br; q2[1] = fmaf(br, br, q2[1]);
      }
    }
    s1 = mt_pair_combine(q1[0], q1[1], odd);
    s2 = mt_pair_combine(q2[0], q2[1], odd);
  } else {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int iv = (j & 3) + 8 * (j >> 2) + 4 * lhalf;
    const int oh = oh0 + (iv >> 3), ow = ow0 + (iv & 7);
    const bool ok = covalid && (od < c.Do) && (oh < c.Ho) && (ow < c.Wo);
    const int off = ok ? (((od * c.Ho + oh) * c.Wo + ow) * ocs + co) * 4 : (int)0x80000000;
    float v = acc[0][j] + bv;
    if (c.accumulate) v += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, off, 0, 0));
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rd, off, 0, 0);
    if (ok) { s1 += v; s2 = fmaf(v, v, s2); }
  }
  }
  if (c.stats_part != nullptr) {
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    __syncthreads();
    if (lhalf == 0) { lds[(wave * 32 + li) * 2] = s1; lds[(wave * 32 + li) * 2 + 1] = s2; }
    __syncthreads();
    if (tid < 64) {                                      // thread t: N tile t/32 of this pair, channel t%32
      const int n2 = tid >> 5, cl = tid & 31;
      const int cg = (by * 2 + n2) * 32 + cl;
      if (cg < c.Cout) {
        const float t1 = lds[((n2 * 2) * 32 + cl) * 2] + lds[((n2 * 2 + 1) * 32 + cl) * 2];
        const float t2 = lds[((n2 * 2) * 32 + cl) * 2 + 1] + lds[((n2 * 2 + 1) * 32 + cl) * 2 + 1];
        float* sp = c.stats_part + ((size_t)((size_t)nb * P.nsb + sb) * c.Cout + cg) * 2;
        sp[0] = t1; sp[1] = t2;
      }
    }
  }
}

// ================================================================================================
// 3x3x3 stride-1 convolution for the LOW-RESOLUTION stages (<= 6x24x24 voxels, 256-320 channels): the standard tiling yields
// fewer workgroups than the chip has CUs and each wave walks Cin/16 x 27 taps serially.  Here a workgroup owns ONE 32-voxel
// M tile (2x4x4) x 32 output channels and its four waves split the 27 TAPS (t = wave, wave+4, ...), so the serial chain per wave
// is 4x shorter and the grid 4x larger; the four accumulator tiles are summed through LDS in a fixed order (deterministic).
// BF = true (mixed precision): bf16 LDS image and one v_mfma_f32_32x32x16_bf16 per tap instead of eight fp32 MFMAs.
// XS / OS / MTY (BF only): storage types of the source / destination and the matrix type, as in conv_bf16_kernel.
// SD / SH / SW (round 5): the same kernel for the strided 3x3x3 stage convs whose standard tiling (conv_fast_strided_kernel, 2x4x8
// outputs x 64 channels) yields fewer workgroups than the chip has CUs — 240 -> 320 @ 6x24x24 -> 3x12x12 is 120 workgroups of 15
// chunks x 216 MFMAs, the bottleneck's 320 -> 320 stride (1,2,2) 40 of 20 (generic_UNet.py:263-278).
#ifndef TS_ABL
#define TS_ABL 0      // timing ablations of the fp32 path: 1 skip the staging, 2 every weight fragment from the same cached 14 KiB, 4 skip the MFMAs
#endif
template <int VEC, bool BF = false, int XS = MT_F32, int OS = MT_F32, int MTY = MT_BF16, int SD = 1, int SH = 1, int SW = 1>
__global__ __launch_bounds__(256) void conv_tapsplit_kernel(const ConvKParams P) {
  static_assert(BF || (XS == MT_F32 && OS == MT_F32), "16-bit storage is served by the 16-bit matrix path");
  constexpr int TD = 2, TH = 4, TW = 4, LD = (TD - 1) * SD + 3, LH = (TH - 1) * SH + 3, LW = (TW - 1) * SW + 3;
  constexpr int LWP = BF ? bstage_lwp<LD, LH, LW, VEC, 4>() : stage_lwp<LD, LH, LW, VEC>();
  constexpr int PITCH = BF ? BFP : FCKP;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  int ntile, td, th, tw, nb;
  mt_tile_coords(mt_block_decode(ntile), P.tilesD, P.tilesH, P.tilesW, td, th, tw, nb);
  const int sb = (td * P.tilesH + th) * P.tilesW + tw;
  const int od0 = td * TD, oh0 = th * TH, ow0 = tw * TW;
  // M tile row li -> voxel (dm, r, col) = (li>>4, (li>>2)&3, li&3)
  const int abase = (((li >> 4) * SD * LH + ((li >> 2) & 3) * SH) * LWP + (li & 3) * SW) * PITCH + lhalf * (BF ? 4 : 8);

  f32x16 acc;
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;

  for (int ch = 0; ch < P.nchunks; ++ch) {
    const ConvChunk cc = P.chunk[ch];
    __syncthreads();
    if constexpr (BF) {
      mt_stage_bf16<LD, LH, LW, VEC, 4, XS, MTY>((unsigned*)lds, c, cc, nb, od0 * SD - 1, oh0 * SH - 1, ow0 * SW - 1, lane, wave);
      __syncthreads();
      const unsigned* ldsu = (const unsigned*)lds;
      const unsigned* wl = (const unsigned*)c.wpack + (size_t)(ntile * P.nchunks + ch) * (27 * 256) + lane * 4;
      bf16x8 fa[7], fb[7];                 // this wave's taps: all fragments first, then the MFMAs back to back
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        const int tt = (wave + 4 * i) < 27 ? wave + 4 * i : 26;
        fa[i] = *(const bf16x8*)(ldsu + abase + (((tt / 9) * LH + (tt / 3) % 3) * LWP + tt % 3) * PITCH);
        fb[i] = *(const bf16x8*)(wl + tt * 256);
      }
#pragma unroll
      for (int i = 0; i < 7; ++i)
        if (i < 6 || wave < 3) acc = mt_mfma16<MTY>(fa[i], fb[i], acc);
      continue;
    }
    const float* wlane = c.wpack + ((TS_ABL & 2) ? (size_t)0 : (size_t)(ntile * P.nchunks + ch) * (27 * 512)) + lane * 4;
    if (!(TS_ABL & 1)) mt_stage_fast2<LD, LH, LW, VEC>(lds, c, cc, nb, od0 * SD - 1, oh0 * SH - 1, ow0 * SW - 1, lane, wave);
    __syncthreads();
    // this wave's taps: wave, wave+4, ... (7 or 6 of them); the next tap's fragments are fetched behind the current MFMAs
    f32x4 a[2][2], b[2][2];
    {
      const int t = wave;
      const int toff = (((t / 9) * LH + (t / 3) % 3) * LWP + t % 3) * FCKP;
      a[0][0] = *(const f32x4*)(lds + abase + toff); a[0][1] = *(const f32x4*)(lds + abase + toff + 4);
      b[0][0] = *(const f32x4*)(wlane + t * 512);    b[0][1] = *(const f32x4*)(wlane + t * 512 + 256);
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const int t = wave + 4 * i, t1 = t + 4;
      if (i + 1 < 7) {
        const int tt = t1 < 27 ? t1 : 26;                 // wave 3 has 6 taps: its 7th fetch is a harmless repeat
        const int toff = (((tt / 9) * LH + (tt / 3) % 3) * LWP + tt % 3) * FCKP;
        a[(i + 1) & 1][0] = *(const f32x4*)(lds + abase + toff); a[(i + 1) & 1][1] = *(const f32x4*)(lds + abase + toff + 4);
        b[(i + 1) & 1][0] = *(const f32x4*)(wlane + tt * 512);   b[(i + 1) & 1][1] = *(const f32x4*)(wlane + tt * 512 + 256);
      }
      if (i < 6 || wave < 3) {                             // only wave 3 lacks a 7th tap (wave-uniform)
        if (TS_ABL & 4) { acc[0] += a[i & 1][0][0] + a[i & 1][1][3] + b[i & 1][0][1] + b[i & 1][1][2]; continue; }
#pragma unroll
        for (int kp = 0; kp < 8; ++kp)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i & 1][kp >> 2][kp & 3], b[i & 1][kp >> 2][kp & 3], acc, 0, 0, 0);
      }
    }
  }

  // ---- fixed-order sum of the four waves' tiles through LDS; wave w finishes accumulator registers 4w..4w+3
  __syncthreads();
  float* red = lds;                                        // [wave][16][64] floats = 16 KiB (the tile buffer is free now)
#pragma unroll
  for (int j = 0; j < 16; ++j) red[(wave * 16 + j) * 64 + lane] = acc[j];
  __syncthreads();
  float v[4];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const float* rp = red + ((wave * 4 + jj)) * 64 + lane;
    v[jj] = ((rp[0] + rp[16 * 64]) + rp[32 * 64]) + rp[48 * 64];
  }
  const int co = ntile * 32 + li;
  const bool covalid = co < c.Cout;
  const float bv = (c.bias != nullptr && covalid) ? c.bias[co] : 0.f;
  const int ocs = c.ocs0;
  const size_t out_sample = (size_t)c.Do * c.Ho * c.Wo;
  constexpr int OEB = mt_ebytes<OS>();
  __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)c.out0 + (size_t)nb * out_sample * ocs * OEB), 0,
                                                                (int)(out_sample * ocs * OEB), 0x00020000);
  float s1 = 0.f, s2 = 0.f;
  if constexpr (OS != MT_F32) {        // channel-pair dwords (mt_pair_exchange): even lanes store row jj, odd lanes row jj + 1
    const bool odd = li & 1;
    const int coe = co & ~1;
    const bool pvalid = coe + 1 < c.Cout;
    float q1[2] = {0.f, 0.f}, q2[2] = {0.f, 0.f};
#pragma unroll
    for (int jj = 0; jj < 4; jj += 2) {
      const int iv = jj + 8 * wave + 4 * lhalf + (odd ? 1 : 0);
      const int od = od0 + (iv >> 4), oh = oh0 + ((iv >> 2) & 3), ow = ow0 + (iv & 3);
      const bool ok = pvalid && od < c.Do && oh < c.Ho && ow < c.Wo;
      const int off = ok ? (((od * c.Ho + oh) * c.Wo + ow) * ocs + coe) * 2 : (int)0x80000000;
      float a, b;
      mt_pair_exchange(v[jj] + bv, v[jj + 1] + bv, odd, a, b);
      if (c.accumulate) { const unsigned pv = __builtin_amdgcn_raw_buffer_load_b32(rd, off, 0, 0); a += mt_lo16<OS>(pv); b += mt_hi16<OS>(pv); }
      const unsigned pk = mt_pk16<OS>(a, b);
      __builtin_amdgcn_raw_buffer_store_b32(pk, rd, off, 0, 0);
      if (ok) {
        const float ar = mt_lo16<OS>(pk), br = mt_hi16<OS>(pk);
        q1[0] += ar; q2[0] = fmaf(ar, ar, q2[0]); q1[1] += br; q2[1] = fmaf(br, br, q2[1]);
      }
    }
    s1 = mt_pair_combine(q1[0], q1[1], odd);
    s2 = mt_pair_combine(q2[0], q2[1], odd);
  } else
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    // accumulator register j = 4*wave + jj holds M row (j&3) + 8*(j>>2) + 4*lhalf = jj + 8*wave + 4*lhalf
    const int iv = jj + 8 * wave + 4 * lhalf;
    const int od = od0 + (iv >> 4), oh = oh0 + ((iv >> 2) & 3), ow = ow0 + (iv & 3);
    const bool ok = covalid && od < c.Do && oh < c.Ho && ow < c.Wo;
    const int off = ok ? (((od * c.Ho + oh) * c.Wo + ow) * ocs + co) * 4 : (int)0x80000000;
    float o = v[jj] + bv;
    if (c.accumulate) o += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, off, 0, 0));
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), rd, off, 0, 0);
    if (ok) { s1 += o; s2 = fmaf(o, o, s2); }
  }
  if (c.stats_part != nullptr) {
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    __syncthreads();
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

// ================================================================================================
// Stem kernels: the first convolution of the network has ONE input channel (CT), so padding Cin to a 16-channel chunk would
// spend 16x the necessary MFMAs.  Here the 27 TAPS are the contraction dimension: A[voxel][k = tap] is gathered from a scalar
// LDS image of the haloed tile, B[k = tap][cout] comes from the packed weights (channel 0 of the single chunk); one M tile of 32
// voxels costs 14 MFMAs instead of 216.  Both kernels (conv_stem_kernel here, conv_bwdw_stem_kernel in conv_bwdw.hip) are bound by
// the 32-channel output / gradient stream (HBM); stem_stage (conv_stage.h) stages the haloed tile for both.
// OS: storage type of the output (the network input is fp32)
template <int OS = MT_F32>
__global__ __launch_bounds__(256) void conv_stem_kernel(const ConvKParams P) {
  constexpr int TD = 2, TH = 4, TW = 32, LH = TH + 2, LW = TW + 2, NJ = 14;      // 14 MFMAs x k=2 cover 27 taps (+1 zero)
  __shared__ float xs[(TD + 2) * LH * LW];
  __shared__ float red[4 * 32 * 2];
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  int ntile, td, th, tw, nb;
  mt_tile_coords(mt_block_decode(ntile), P.tilesD, P.tilesH, P.tilesW, td, th, tw, nb);
  const int sb = (td * P.tilesH + th) * P.tilesW + tw;
  const int od0 = td * TD, oh0 = th * TH, ow0 = tw * TW;
  stem_stage<TD, TH, TW>(xs, c, nb, od0, oh0, ow0, tid);
  // B fragments: W[tap = 2j + lhalf][cout = li] = channel 0 of the chunk = element 0 of lane li's first float4 of the tap
  const float* wq = c.wpack + (size_t)ntile * P.nchunks * (27 * 512) + li * 4;
  float b[NJ];
  int koff[NJ];
  // this wave's two M tiles: plane dm = wave/2, rows (wave%2)*2 + {0,1}
  const int mbase = (((wave >> 1)) * LH + (wave & 1) * 2) * LW + li;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int k = 2 * j + lhalf;
    const bool kv = k < 27;
    b[j] = kv ? wq[(kv ? k : 0) * 512] : 0.f;
    const int kk = kv ? k : 0;
    koff[j] = mbase + ((kk / 9) * LH + (kk / 3) % 3) * LW + kk % 3;
  }
  __syncthreads();
  f32x16 acc[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[m][q] = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[koff[j] + m * LW], b[j], acc[m], 0, 0, 0);
  }
  const int co = ntile * 32 + li;
  const bool covalid = co < c.Cout;
  const float bv = (c.bias != nullptr && covalid) ? c.bias[co] : 0.f;
  const int ocs = c.ocs0;
  const size_t out_sample = (size_t)c.Do * c.Ho * c.Wo;
  constexpr int OEB = mt_ebytes<OS>();
  __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)c.out0 + (size_t)nb * out_sample * ocs * OEB), 0,
                                                                (int)(out_sample * ocs * OEB), 0x00020000);
  float s1 = 0.f, s2 = 0.f;
  const int od = od0 + (wave >> 1);
  if constexpr (OS != MT_F32) {        // channel-pair dwords (mt_pair_exchange): even lanes store voxel q, odd lanes voxel q + 1
    const bool odd = li & 1;
    const int coe = co & ~1;
    const bool pvalid = coe + 1 < c.Cout;
    float q1[2] = {0.f, 0.f}, q2[2] = {0.f, 0.f};
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int oh = oh0 + (wave & 1) * 2 + m;
#pragma unroll
      for (int q = 0; q < 16; q += 2) {
        const int ow = ow0 + (q & 3) + 8 * (q >> 2) + 4 * lhalf + (odd ? 1 : 0);
        const bool ok = pvalid && od < c.Do && oh < c.Ho && ow < c.Wo;
        const int off = ok ? (((od * c.Ho + oh) * c.Wo + ow) * ocs + coe) * 2 : (int)0x80000000;
        float a, b;
        mt_pair_exchange(acc[m][q] + bv, acc[m][q + 1] + bv, odd, a, b);
        if (c.accumulate) { const unsigned pv = __builtin_amdgcn_raw_buffer_load_b32(rd, off, 0, 0); a += mt_lo16<OS>(pv); b += mt_hi16<OS>(pv); }
        const unsigned pk = mt_pk16<OS>(a, b);
        __builtin_amdgcn_raw_buffer_store_b32(pk, rd, off, 0, 0);
        if (ok) {
          const float ar = mt_lo16<OS>(pk), br = mt_hi16<OS>(pk);
          q1[0] += ar; q2[0] = fmaf(ar, ar, q2[0]); q1[1] += br; q2[1] = fmaf(br, br, q2[1]);
        }
      }
    }
    s1 = mt_pair_combine(q1[0], q1[1], odd);
    s2 = mt_pair_combine(q2[0], q2[1], odd);
  } else
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int oh = oh0 + (wave & 1) * 2 + m;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int ow = ow0 + (q & 3) + 8 * (q >> 2) + 4 * lhalf;
      const bool ok = covalid && od < c.Do && oh < c.Ho && ow < c.Wo;
      const int off = ok ? (((od * c.Ho + oh) * c.Wo + ow) * ocs + co) * 4 : (int)0x80000000;
      float v = acc[m][q] + bv;
      if (c.accumulate) v += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, off, 0, 0));
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rd, off, 0, 0);
      if (ok) { s1 += v; s2 = fmaf(v, v, s2); }
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

// ================================================================================================
// Non-overlapping convolution (kernel == stride in every dim, pad 0): the backward-data of ConvTranspose3d(k = s)
// (generic_UNet.py:335-336) — every output voxel reads its own kD*kH*kW block, nothing is shared between outputs, so there is
// no halo to stage: A fragments come straight from global memory (32-byte per-lane vectors, lazy activation in registers) as in
// the pointwise kernel, one accumulator tile per wave of 32 output voxels x 32 channels.
// BF (mixed precision, bf16 source without a lazy activation = a gradient): the lane's 16-byte load IS the A fragment of
// v_mfma_f32_32x32x16_bf16 (8 channels of its voxel), the weights are pack layout 3 — one MFMA per (chunk, tap) instead of eight fp32
// ones.  (In fp32 this kernel is AT the fp32 matrix rate: 29 padded GFLOP in 185 us for the 60 -> 30 transposed conv of Task009.)
// NT (fp32 only): cout tiles per wave.  The A fragments are a GATHER (32 bytes of every second 120 / 240-byte voxel per lane and tap): with one
// tile per wave every cout tile re-requests them, and the L2 -> L1 line rate of that gather, not the matrix pipe, paces the kernel.
template <int VEC, int XS = MT_F32, int OS = MT_F32, bool BF = false, int NT = 1>
__global__ __launch_bounds__(256) void conv_gather_kernel(const ConvKParams P) {
  static_assert(NT == 1 || (!BF && XS == MT_F32 && OS == MT_F32), "several cout tiles per wave: the fp32 form");
  constexpr int XE = mt_ebytes<XS>(), OE = mt_ebytes<OS>();
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  const long V = (long)c.Do * c.Ho * c.Wo;
  const int nsb = (int)((V + 127) / 128);
  int ntile;
  const int bx = mt_block_decode(ntile);
  const int nb = bx / nsb, sb = bx % nsb;
  const long m0 = (long)sb * 128 + wave * 32;
  const mt_src_t& S = c.src[0];
  const long mv = m0 + li;
  const bool vok = mv < V;
  const int ow = (int)(mv % c.Wo), oh = (int)((mv / c.Wo) % c.Ho), od = (int)(mv / ((long)c.Wo * c.Ho));
  const size_t in_sample = (size_t)c.Di * c.Hi * c.Wi * S.cs;
  __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)S.ptr + (size_t)nb * in_sample * XE), 0, (int)(in_sample * XE), 0x00020000);
  const int abase = vok ? ((((od * c.SD) * c.Hi + oh * c.SH) * c.Wi + ow * c.SW) * S.cs + 8 * lhalf) * XE : (int)0x80000000;
  const bool aff = S.scale != nullptr;
  const float slope = aff ? S.slope : 1.f;
  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(aff ? S.scale + (size_t)nb * S.C : S.ptr), 0, aff ? S.C * 4 : 0, 0x00020000);
  __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc((void*)(aff ? S.shift + (size_t)nb * S.C : S.ptr), 0, aff ? S.C * 4 : 0, 0x00020000);
  const int ntaps = P.ntaps, total = P.nchunks * ntaps;

  // (chunk, kd, kh, kw) of the NEXT load advance as counters: `it / ntaps`, `tap % KW` ... with run-time divisors are ~40
  // instructions each on this hardware (no integer divider), three of them per 8 MFMAs in the first version
  int l_ch = 0, l_kd = 0, l_kh = 0, l_kw = 0;
  auto load_a = [&](float (&x)[8]) {
    const int so = __builtin_amdgcn_readfirstlane((((l_kd * c.Hi + l_kh) * c.Wi + l_kw) * S.cs + l_ch * FCK) * XE);
    if (++l_kw == c.KW) { l_kw = 0; if (++l_kh == c.KH) { l_kh = 0; if (++l_kd == c.KD) { l_kd = 0; ++l_ch; } } }
    if constexpr (XS != MT_F32) {         // 8 channels of a 16-bit source: one 16-byte load
      const uint4 t = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ra, abase, so, 0));
      x[0] = mt_lo16<XS>(t.x); x[1] = mt_hi16<XS>(t.x); x[2] = mt_lo16<XS>(t.y); x[3] = mt_hi16<XS>(t.y);
      x[4] = mt_lo16<XS>(t.z); x[5] = mt_hi16<XS>(t.z); x[6] = mt_lo16<XS>(t.w); x[7] = mt_hi16<XS>(t.w);
    } else if constexpr (VEC == 4) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const f32x4 t = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, abase + g * 16, so, 0));
        x[4 * g] = t[0]; x[4 * g + 1] = t[1]; x[4 * g + 2] = t[2]; x[4 * g + 3] = t[3];
      }
    } else if constexpr (VEC == 2) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float2 t = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(ra, abase + g * 8, so, 0));
        x[2 * g] = t.x; x[2 * g + 1] = t.y;
      }
    } else {
#pragma unroll
      for (int g = 0; g < 8; ++g) x[g] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, abase + g * 4, so, 0));
    }
  };

  f32x16 accn[NT];
  f32x16& acc = accn[0];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int j = 0; j < 16; ++j) accn[nt][j] = 0.f;
  const int ntiles = (c.Cout + 31) >> 5;
  if constexpr (BF) {
    static_assert(XS == MT_BF16, "the bf16 matrix path reads a bf16 source");
    const unsigned* wq = (const unsigned*)c.wpack + (size_t)ntile * P.nchunks * ntaps * 256 + lane * 4;
    // channel tail of the last chunk as AND masks on the fragment's dwords (the bytes belong to the next voxel)
    int g_kd = 0, g_kh = 0, g_kw = 0, g_ch = 0;
    auto load_raw = [&]() -> uint4 {
      const int so = __builtin_amdgcn_readfirstlane((((g_kd * c.Hi + g_kh) * c.Wi + g_kw) * S.cs + g_ch * FCK) * XE);
      if (++g_kw == c.KW) { g_kw = 0; if (++g_kh == c.KH) { g_kh = 0; if (++g_kd == c.KD) { g_kd = 0; ++g_ch; } } }
      return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ra, abase, so, 0));
    };
    constexpr int PF = 4;                      // fragments in flight
    uint4 ar[PF], br[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) if (u < total) { ar[u] = load_raw(); br[u] = *(const uint4*)(wq + (size_t)u * 256); }
    int ch = 0, tap = 0;
    for (int it0 = 0; it0 < total; it0 += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int it = it0 + u;
        if (it < total) {
          uint4 a = ar[u]; const uint4 b = br[u];
          const int cb = ch * FCK + 8 * lhalf;           // first channel of this lane's fragment
          if (cb + 8 > c.Cin) {
            const unsigned m0 = (cb + 0 < c.Cin ? 0xffffu : 0u) | (cb + 1 < c.Cin ? 0xffff0000u : 0u), m1 = (cb + 2 < c.Cin ? 0xffffu : 0u) | (cb + 3 < c.Cin ? 0xffff0000u : 0u);
            const unsigned m2 = (cb + 4 < c.Cin ? 0xffffu : 0u) | (cb + 5 < c.Cin ? 0xffff0000u : 0u), m3 = (cb + 6 < c.Cin ? 0xffffu : 0u) | (cb + 7 < c.Cin ? 0xffff0000u : 0u);
            a.x &= m0; a.y &= m1; a.z &= m2; a.w &= m3;
          }
          if (it + PF < total) { ar[u] = load_raw(); br[u] = *(const uint4*)(wq + (size_t)(it + PF) * 256); }
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
          if (++tap == ntaps) { tap = 0; ++ch; }
        }
      }
    }
  } else {
  if constexpr (NT > 1) {
    // Chunk PAIRS: the two 16-channel chunks of a voxel's 32 channels (128 bytes) are requested back to back, tap-major inside the pair - the second
    // request finds the line the first one brought in (one L2 -> L1 fill per voxel and tap instead of two).
    const int npairs = (P.nchunks + 1) >> 1, totalp = npairs * ntaps;
    int p_pr = 0, p_kd = 0, p_kh = 0, p_kw = 0;
    auto load_pair = [&](float (&x)[2][8]) __attribute__((always_inline)) {
      const int so = __builtin_amdgcn_readfirstlane((((p_kd * c.Hi + p_kh) * c.Wi + p_kw) * S.cs + 2 * p_pr * FCK) * 4);
      const bool two = 2 * p_pr + 1 < P.nchunks;
      if (++p_kw == c.KW) { p_kw = 0; if (++p_kh == c.KH) { p_kh = 0; if (++p_kd == c.KD) { p_kd = 0; ++p_pr; } } }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h == 0 || two) {
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            const f32x4 t = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, abase + g * 16, so + h * FCK * 4, 0));
            x[h][4 * g] = t[0]; x[h][4 * g + 1] = t[1]; x[h][4 * g + 2] = t[2]; x[h][4 * g + 3] = t[3];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) x[h][e] = 0.f;
        }
      }
    };
    float xa[2][8], xn[2][8], sc[2][8], sh[2][8];
    load_pair(xa);
    for (int it = 0, pr = 0, tap = 0; it < totalp; ++it) {
      if (it + 1 < totalp) load_pair(xn);
      const bool two = 2 * pr + 1 < P.nchunks;
      if (tap == 0) {                                    // per-chunk lazy-activation constants (0 for channels beyond Cin)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int cb = (2 * pr + h) * FCK + 8 * lhalf;
            const bool cv = cb + e < c.Cin;
            sc[h][e] = aff ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, cv ? (cb + e) * 4 : (int)0x80000000, 0, 0)) : (cv ? 1.f : 0.f);
            sh[h][e] = aff ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rh, cv ? (cb + e) * 4 : (int)0x80000000, 0, 0)) : 0.f;
          }
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h == 0 || two) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float t = fmaf(xa[h][e], sc[h][e], sh[h][e]);
            xa[h][e] = vok ? mt_lrelu(t, slope) : 0.f;
          }
          f32x4 b0[NT], b1[NT];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {  // (a cout tile behind the last one: tile 0's weights, its outputs are never stored)
            const int tl = ntile * NT + nt < ntiles ? ntile * NT + nt : 0;
            const float* wq = c.wpack + ((size_t)(tl * P.nchunks + 2 * pr + h) * ntaps + tap) * 512 + lane * 4;
            b0[nt] = *(const f32x4*)(wq);
            b1[nt] = *(const f32x4*)(wq + 256);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) accn[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[h][e], b0[nt][e], accn[nt], 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) accn[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[h][4 + e], b1[nt][e], accn[nt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) xa[h][e] = xn[h][e];
      if (++tap == ntaps) { tap = 0; ++pr; }
    }
  } else {
  float xa[8], xn[8], sc[8], sh[8];
  load_a(xa);
  for (int it = 0, ch = 0, tap = 0; it < total; ++it) {
    if (it + 1 < total) load_a(xn);
    const int cb = ch * FCK + 8 * lhalf;
    if (tap == 0) {                                      // per-chunk lazy-activation constants (0 for channels beyond Cin)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool cv = cb + e < c.Cin;
        sc[e] = aff ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, cv ? (cb + e) * 4 : (int)0x80000000, 0, 0)) : (cv ? 1.f : 0.f);
        sh[e] = aff ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rh, cv ? (cb + e) * 4 : (int)0x80000000, 0, 0)) : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = fmaf(xa[e], sc[e], sh[e]);
      xa[e] = vok ? mt_lrelu(t, slope) : 0.f;
    }
    f32x4 b0[NT], b1[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {      // (a cout tile behind the last one: tile 0's weights, its outputs are never stored)
      const int tl = ntile * NT + nt < ntiles ? ntile * NT + nt : 0;
      const float* wq = c.wpack + ((size_t)(tl * P.nchunks + ch) * ntaps + tap) * 512 + lane * 4;
      b0[nt] = *(const f32x4*)(wq);
      b1[nt] = *(const f32x4*)(wq + 256);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) accn[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[e], b0[nt][e], accn[nt], 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) accn[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[4 + e], b1[nt][e], accn[nt], 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 8; ++e) xa[e] = xn[e];
    if (++tap == ntaps) { tap = 0; ++ch; }
  }
  }
  }

  const size_t out_sample = (size_t)V * c.ocs0;
  __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)c.out0 + (size_t)nb * out_sample * OE), 0, (int)(out_sample * OE), 0x00020000);
  if constexpr (NT > 1) {
    static_assert(NT == 2, "the wide epilogue stages 32 voxels x 64 channels per wave");
    // Wide epilogue: the accumulator layout gives a lane ONE channel of 16 voxels (32 dword stores per lane and wave tile, each 2 x 128 bytes);
    // through a wave-private LDS image [32 voxels][64 channels] a lane leaves with 4 channels of a voxel per 16-byte store - 8 stores of 1 KB.
    if ((c.ocs0 & 3) == 0 && (c.Cout & 3) == 0 && ((((uintptr_t)c.out0) & 15) == 0)) {
      __shared__ __attribute__((aligned(16))) float stg[4][32 * 64];
      float* const sw = stg[wave];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int co = (ntile * NT + nt) * 32 + li;
        const float bv = (c.bias != nullptr && co < c.Cout) ? c.bias[co] : 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) sw[((j & 3) + 8 * (j >> 2) + 4 * lhalf) * 64 + nt * 32 + li] = accn[nt][j] + bv;
      }
      const int c4 = (lane & 15) * 4, vq = lane >> 4;               // this lane's 4 channels of the 64 | its voxel of each group of four
      const int cg = ntile * 64 + c4;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int vl = k * 4 + vq;
        f32x4 val = *(const f32x4*)(sw + vl * 64 + c4);              // (same wave: LDS operations retire in order)
        const long v = m0 + vl;
        const int off = (cg < c.Cout && v < V) ? (int)((v * c.ocs0 + cg) * 4) : (int)0x80000000;
        if (c.accumulate) val += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ro, off, 0, 0));
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, val), ro, off, 0, 0);
      }
      return;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int co = (ntile * NT + nt) * 32 + li;
      const bool covalid = co < c.Cout;
      const float bv = (c.bias != nullptr && covalid) ? c.bias[co] : 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const long v = m0 + (j & 3) + 8 * (j >> 2) + 4 * lhalf;
        const int off = (covalid && v < V) ? (int)((v * c.ocs0 + co) * 4) : (int)0x80000000;
        float val = accn[nt][j] + bv;
        if (c.accumulate) val += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ro, off, 0, 0));
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), ro, off, 0, 0);
      }
    }
    return;
  }
  const int co = ntile * 32 + li;
  const bool covalid = co < c.Cout;
  const float bv = (c.bias != nullptr && covalid) ? c.bias[co] : 0.f;
  if constexpr (OS != MT_F32) {          // channel-pair dwords (mt_pair_exchange)
    const bool odd = li & 1;
    const int coe = co & ~1;
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
      const long v = m0 + (j & 3) + 8 * (j >> 2) + 4 * lhalf + (odd ? 1 : 0);
      const int off = (coe + 1 < c.Cout && v < V) ? (int)((v * c.ocs0 + coe) * 2) : (int)0x80000000;
      float a, b;
      mt_pair_exchange(acc[j] + bv, acc[j + 1] + bv, odd, a, b);
      if (c.accumulate) { const unsigned pv = __builtin_amdgcn_raw_buffer_load_b32(ro, off, 0, 0); a += mt_lo16<OS>(pv); b += mt_hi16<OS>(pv); }
      __builtin_amdgcn_raw_buffer_store_b32(mt_pk16<OS>(a, b), ro, off, 0, 0);
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const long v = m0 + (j & 3) + 8 * (j >> 2) + 4 * lhalf;
    const int off = (covalid && v < V) ? (int)((v * c.ocs0 + co) * 4) : (int)0x80000000;
    float val = acc[j] + bv;
    if (c.accumulate) val += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ro, off, 0, 0));
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), ro, off, 0, 0);
  }
}

// ================================================================================================
// Runtime-geometry forward kernel on the FAST design (any kernel size 1..3, stride 1..2, pad, strided output placement):
// LDS image [voxel][20], ds_read_b128 operands, float4 weights, buffer loads/stores.  The tap loop is a runtime loop
// (unrolled by two with ping-pong fragments); the only vector-ALU work inside it is one address add per M tile and tap
// (1 VALU per 16 MFMAs).  Serves strided stage convs, 1x3x3 and 1x1x1(strided) convs, the backward-data of transposed
// convs (a k = s conv) and of strided convs (one launch per parity class with a sub-kernel and os = stride, oo = parity).
template <int VEC>
__device__ __forceinline__ void mt_stage_rt(float* __restrict__ lds, const mt_conv3d_t& c, const ConvChunk ch, int nb,
                                            int ud0, int uh0, int uw0, int LD, int LH, int LW, int lane, int wave) {
  constexpr int LPV = FCK / VEC, VPS = 64 / LPV, NIMAX = (66 + VPS - 1) / VPS;
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
      sc[e] = S.scale[(size_t)nb * S.C + ch.c0 + cl + e];
      sh[e] = S.shift[(size_t)nb * S.C + ch.c0 + cl + e];
    }
  }
  const float slope = S.slope;
  const int cs = S.cs;
  const size_t sample_elems = (size_t)c.Di * c.Hi * c.Wi * cs;
  __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)(S.ptr + (size_t)nb * sample_elems), 0, (int)(sample_elems * 4), 0x00020000);
  const int NI = (LW + VPS - 1) / VPS;
  int voff[NIMAX];
#pragma unroll
  for (int i = 0; i < NIMAX; ++i) {
    const int lw = vl + i * VPS;
    const int uw = uw0 + lw;
    const bool ok = cval[0] && (i < NI) && (lw < LW) && ((unsigned)uw < (unsigned)c.Wi);
    voff[i] = ok ? (uw * cs + ch.c0 + cl) * 4 : (int)0x80000000;
  }
  const bool lrelu_ok = (slope >= 0.f) && (slope <= 1.f);
  const int nrows = LD * LH;
  float* lbase = lds + vl * FCKP + cl;
  for (int row = wave; row < nrows; row += 4) {
    const int ld = row / LH, lhh = row - ld * LH;
    const int ud = ud0 + ld, uh = uh0 + lhh;
    const bool rv = ((unsigned)ud < (unsigned)c.Di) && ((unsigned)uh < (unsigned)c.Hi);
    const int srow = rv ? (ud * c.Hi + uh) * c.Wi * cs * 4 : 0;
    float v[NIMAX][VEC];
#pragma unroll
    for (int i = 0; i < NIMAX; ++i) {
      if (i < NI && rv) {
        if constexpr (VEC == 2) {
          const float2 t = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff[i] + srow, 0, 0));
          v[i][0] = t.x; v[i][1] = t.y;
        } else {
          v[i][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff[i] + srow, 0, 0));
        }
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[i][e] = 0.f;
      }
    }
    float* lrow = lbase + row * LW * FCKP;
#pragma unroll
    for (int i = 0; i < NIMAX; ++i) {
      const int lw = vl + i * VPS;
      if (i < NI && lw < LW) {
        float x[VEC];
        const bool ok = rv && voff[i] >= 0;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          x[e] = v[i][e];
          if (has_aff) {
            const float t = fmaf(x[e], sc[e], sh[e]);
            const float a = lrelu_ok ? fmaxf(t, t * slope) : mt_lrelu(t, slope);
            x[e] = (ok && cval[e]) ? a : 0.f;
          } else if (VEC == 2 && e == 1) x[e] = cval[e] ? x[e] : 0.f;
        }
        if constexpr (VEC == 2) {
          float2 t; t.x = x[0]; t.y = x[1];
          *(float2*)(lrow + i * VPS * FCKP) = t;
        } else {
          lrow[i * VPS * FCKP] = x[0];
        }
      }
    }
  }
}

template <int MT>
__device__ __forceinline__ void rt_frag_load(FastFrag<MT>& f, const float* __restrict__ lds, const int (&abase)[MT], int off,
                                             const float* __restrict__ wq) {
  f.b[0] = *(const f32x4*)(wq);
  f.b[1] = *(const f32x4*)(wq + 256);
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const float* a = lds + abase[m] + off;
    f.a[m][0] = *(const f32x4*)(a);
    f.a[m][1] = *(const f32x4*)(a + 4);
  }
}

template <int MW, int RH, int TD, int VEC>
__global__ __launch_bounds__(256) void conv_rt_kernel(const ConvKParams P) {
  constexpr int MH = 32 / MW, TH = MH * RH, TW = MW, NMT = TD * RH, MT = NMT / 4;
  static_assert(NMT % 4 == 0, "M tiles must split over 4 waves");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  int ntile, td, th, tw, nb;
  mt_tile_coords(mt_block_decode(ntile), P.tilesD, P.tilesH, P.tilesW, td, th, tw, nb);
  const int sb = (td * P.tilesH + th) * P.tilesW + tw;
  const int LD = (TD - 1) * c.SD + c.KD, LH = (TH - 1) * c.SH + c.KH, LW = (TW - 1) * c.SW + c.KW;
  const int od0 = td * TD, oh0 = th * TH, ow0 = tw * TW;

  int abase[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mt = wave * MT + m;
    const int dm = mt / RH, rh = mt % RH;
    const int r = li / MW, col = li % MW;
    abase[m] = ((dm * c.SD * LH + (rh * MH + r) * c.SH) * LW + col * c.SW) * FCKP + lhalf * 8;
  }
  f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[m][j] = 0.f;

  const int ntaps = P.ntaps;
  const int step_w = FCKP, step_h = (LW - c.KW) * FCKP, step_d = (LH - c.KH) * LW * FCKP;
  for (int ch = 0; ch < P.nchunks; ++ch) {
    const ConvChunk cc = P.chunk[ch];
    const float* wq = c.wpack + (size_t)(ntile * P.nchunks + ch) * ntaps * 512 + lane * 4;
    __syncthreads();
    mt_stage_rt<VEC>(lds, c, cc, nb, od0 * c.SD - c.PD, oh0 * c.SH - c.PH, ow0 * c.SW - c.PW, LD, LH, LW, lane, wave);
    __syncthreads();
    FastFrag<MT> f0, f1;
    int off = 0, kw = 0, kh = 0, tap = 0;
    auto advance = [&]() {
      if (tap + 1 < ntaps) {
        off += step_w;
        if (++kw == c.KW) { kw = 0; off += step_h; if (++kh == c.KH) { kh = 0; off += step_d; } }
        wq += 512;
      }
      ++tap;
    };
    rt_frag_load<MT>(f0, lds, abase, off, wq);
    while (tap + 2 <= ntaps) {
      advance();
      __builtin_amdgcn_sched_barrier(0);
      rt_frag_load<MT>(f1, lds, abase, off, wq);
      __builtin_amdgcn_sched_barrier(0);
      fast_frag_mfma<MT>(f0, acc);
      __builtin_amdgcn_sched_barrier(0);
      advance();
      __builtin_amdgcn_sched_barrier(0);
      rt_frag_load<MT>(f0, lds, abase, off, wq);
      __builtin_amdgcn_sched_barrier(0);
      fast_frag_mfma<MT>(f1, acc);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (tap < ntaps) fast_frag_mfma<MT>(f0, acc);
  }

  // ---- epilogue (strided placement; one or two destinations: each lane stores through the descriptor of its channel, the other
  // store of a split launch carries the hardware-masked offset)
  const int co = ntile * 32 + li;
  const bool covalid = co < c.Cout;
  const float bv = (c.bias != nullptr && covalid) ? c.bias[co] : 0.f;
  const int osD = c.osD > 0 ? c.osD : 1, osH = c.osH > 0 ? c.osH : 1, osW = c.osW > 0 ? c.osW : 1;
  const int OD = c.osD > 0 ? c.OD : c.Do, OH = c.osD > 0 ? c.OH : c.Ho, OW = c.osD > 0 ? c.OW : c.Wo;
  const int ooD = c.osD > 0 ? c.ooD : 0, ooH = c.osD > 0 ? c.ooH : 0, ooW = c.osD > 0 ? c.ooW : 0;
  const bool split = c.csplit < c.Cout;
  const bool use1 = split && co >= c.csplit;
  const int ocs = use1 ? c.ocs1 : c.ocs0;
  const int cofs = use1 ? co - c.csplit : co;
  const size_t out_sample = (size_t)OD * OH * OW;
  __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(c.out0 + (size_t)nb * out_sample * c.ocs0), 0,
                                                                (int)(out_sample * c.ocs0 * 4), 0x00020000);
  __amdgpu_buffer_rsrc_t rd1 = rd;
  if (split) rd1 = __builtin_amdgcn_make_buffer_rsrc((void*)(c.out1 + (size_t)nb * out_sample * c.ocs1), 0,
                                                     (int)(out_sample * c.ocs1 * 4), 0x00020000);
  const int m0 = use1 ? (int)0x80000000 : 0, m1 = use1 ? 0 : (int)0x80000000;
  const int lane_col = 4 * lhalf;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mt = wave * MT + m;
    const int dm = mt / RH, rh = mt % RH;
    const int od = od0 + dm;
    auto jgeom = [&](int j, bool& ok) -> int {
      const int ivj = (j & 3) + 8 * (j >> 2);
      const int r = ivj / MW, colj = ivj % MW;
      const int oh = oh0 + rh * MH + r, ow = ow0 + colj + lane_col;
      ok = covalid && (od < c.Do) && (oh < c.Ho) && (ow < c.Wo);
      const int vox = ((od * osD + ooD) * OH + (oh * osH + ooH)) * OW + (ow * osW + ooW);
      return ok ? (vox * ocs + cofs) * 4 : (int)0x80000000;
    };
    float prev[16];                                    // accumulate: the 16 old values are requested together, before the first store
    if (c.accumulate) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        bool ok; const int off = jgeom(j, ok);
        prev[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, off | m0, 0, 0));
        if (split) prev[j] += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd1, off | m1, 0, 0));
      }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      bool ok; const int off = jgeom(j, ok);
      float v = acc[m][j] + bv;
      if (c.accumulate) v += prev[j];
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rd, off | m0, 0, 0);
      if (split) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rd1, off | m1, 0, 0);
      if (ok) { s1 += v; s2 = fmaf(v, v, s2); }
    }
  }
  if (c.stats_part != nullptr) {
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    __syncthreads();
    if (lhalf == 0) { lds[(wave * 32 + li) * 2] = s1; lds[(wave * 32 + li) * 2 + 1] = s2; }
    __syncthreads();
    if (tid < 32 && (ntile * 32 + tid) < c.Cout) {
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) { t1 += lds[(w * 32 + tid) * 2]; t2 += lds[(w * 32 + tid) * 2 + 1]; }
      float* sp = c.stats_part + ((size_t)((size_t)nb * P.nsb + sb) * c.Cout + ntile * 32 + tid) * 2;
      sp[0] = t1; sp[1] = t2;
    }
  }
}

// ================================================================================================
// Backward-data of a strided 3x3x3 convolution (stride 2 in the dims given by SD/SH/SW, pad 1) in ONE launch:
//   dX[S*m + par] = sum over the taps k congruent to par+1 (mod S) of dY[m + j(k)] * W[k]
// A workgroup stages one dY tile (with a +1 halo in strided dims, +-1 in stride-1 dims) and keeps one accumulator tile per
// parity class (8 for stride (2,2,2), 4 for (1,2,2)): every one of the 27 taps is exactly one 16-channel MFMA block into the
// class it belongs to, so the MFMA work equals the algorithmic FLOPs — no multiplication of inserted zeros, no re-staging
// of dY per class.  Per dim:  S = 2: k=1 -> (par 0, j 0), k=2 -> (par 1, j 0), k=0 -> (par 1, j 1);   S = 1: (par 0, j 2-k)
// with the tile origin at m0-1.
template <int S> __host__ __device__ constexpr int bd_par(int k) { return S == 2 ? (k == 1 ? 0 : 1) : 0; }
template <int S> __host__ __device__ constexpr int bd_off(int k) { return S == 2 ? (k == 0 ? 1 : 0) : 2 - k; }

// BF = true (mixed precision): bf16 LDS image (mt_stage_bf16) and one v_mfma_f32_32x32x16_bf16 per tap.
#ifndef BDS_ABL
#define BDS_ABL 0      // timing ablations: 1 skip the dY staging, 2 skip the weight-fragment loads, 4 skip the epilogue, 8 skip the MFMAs
#endif
template <int SD, int SH, int SW, int VEC, bool BF = false, int XS = MT_F32, int OS = MT_F32>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void conv_bwdd_strided_kernel(const ConvKParams P) {
  static_assert(BF || (XS == MT_F32 && OS == MT_F32), "16-bit storage is served by the bf16 matrix path");
  constexpr bool OB = OS != MT_F32;
  constexpr int TD = 2, TH = 4, TW = 16;                       // dY positions per workgroup: 4 waves x 32
  constexpr int LD = TD + (SD == 2 ? 1 : 2), LH = TH + (SH == 2 ? 1 : 2), LW = TW + (SW == 2 ? 1 : 2);
  constexpr int NC = SD * SH * SW, LWP = BF ? bstage_lwp<LD, LH, LW, VEC, 4>() : stage_lwp<LD, LH, LW, VEC>();
  constexpr int PITCH = BF ? BFP : FCKP;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  int ntile, td, th, tw, nb;
  mt_tile_coords(mt_block_decode(ntile), P.tilesD, P.tilesH, P.tilesW, td, th, tw, nb);
  const int md0 = td * TD, mh0 = th * TH, mw0 = tw * TW;

  // this wave's M tile: dm = wave/2, rows (wave%2)*2 + {0,1}, 16 columns
  const int dm = wave >> 1, rbase = (wave & 1) * 2;
  const int abase = ((dm * LH + rbase + (li >> 4)) * LWP + (li & 15)) * PITCH + lhalf * (BF ? 4 : 8);

  f32x16 acc[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[q][j] = 0.f;

  for (int ch = 0; ch < P.nchunks; ++ch) {
    const ConvChunk cc = P.chunk[ch];
    const float* wlane = c.wpack + (size_t)(ntile * P.nchunks + ch) * (27 * 512) + lane * 4;
    __syncthreads();
    if constexpr (BF) {
      mt_stage_bf16<LD, LH, LW, VEC, 4, XS, MT_BF16>((unsigned*)lds, c, cc, nb, md0 - (SD == 1 ? 1 : 0), mh0 - (SH == 1 ? 1 : 0), mw0 - (SW == 1 ? 1 : 0), lane, wave);
      __syncthreads();
      const unsigned* ldsu = (const unsigned*)lds;
      const unsigned* wl = (const unsigned*)c.wpack + (size_t)(ntile * P.nchunks + ch) * (27 * 256) + lane * 4;
      constexpr int BPF = 5, NB = BPF + 1;
      bf16x8 b[NB], a[2];
#pragma unroll
      for (int t = 0; t < BPF; ++t) b[t] = *(const bf16x8*)(wl + t * 256);
      {
        constexpr int o0 = ((bd_off<SD>(0) * LH + bd_off<SH>(0)) * LWP + bd_off<SW>(0)) * PITCH;
        a[0] = *(const bf16x8*)(ldsu + abase + o0);
      }
#pragma unroll
      for (int t = 0; t < 27; ++t) {
        if (t + BPF < 27) b[(t + BPF) % NB] = *(const bf16x8*)(wl + (t + BPF) * 256);
        if (t + 1 < 27) {
          const int t1 = t + 1;
          const int o1 = ((bd_off<SD>(t1 / 9) * LH + bd_off<SH>((t1 / 3) % 3)) * LWP + bd_off<SW>(t1 % 3)) * PITCH;
          a[t1 & 1] = *(const bf16x8*)(ldsu + abase + o1);
        }
        __builtin_amdgcn_sched_barrier(0);
        const int q = (bd_par<SD>(t / 9) * SH + bd_par<SH>((t / 3) % 3)) * SW + bd_par<SW>(t % 3);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[t & 1], b[t % NB], acc[q], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      continue;
    }
    if (!(BDS_ABL & 1)) mt_stage_fast2<LD, LH, LW, VEC>(lds, c, cc, nb, md0 - (SD == 1 ? 1 : 0), mh0 - (SH == 1 ? 1 : 0), mw0 - (SW == 1 ? 1 : 0), lane, wave);
    __syncthreads();
    if (BDS_ABL & 2) wlane = c.wpack + lane * 4;       // (every fragment from the same cached 8 KiB)
    // all 27 taps unrolled in natural order; tap t reads the A fragment at its compile-time offset (jd, jh, jw) and accumulates
    // into the tile of its parity class.  Weight fragments are prefetched 3 taps ahead through a register ring, A fragments
    // one tap ahead (same software pipeline as fast_chunk — the plain loop nest left every L2 round trip exposed).
    {
      constexpr int NB = 4;
      f32x4 b[NB][2];
      f32x4 a[2][2];
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        b[t][0] = *(const f32x4*)(wlane + t * 512);
        b[t][1] = *(const f32x4*)(wlane + t * 512 + 256);
      }
      {
        constexpr int o0 = ((bd_off<SD>(0) * LH + bd_off<SH>(0)) * LWP + bd_off<SW>(0)) * FCKP;
        a[0][0] = *(const f32x4*)(lds + abase + o0);
        a[0][1] = *(const f32x4*)(lds + abase + o0 + 4);
      }
#pragma unroll
      for (int t = 0; t < 27; ++t) {
        if (t + 3 < 27 && !(BDS_ABL & 2)) {
          b[(t + 3) % NB][0] = *(const f32x4*)(wlane + (t + 3) * 512);
          b[(t + 3) % NB][1] = *(const f32x4*)(wlane + (t + 3) * 512 + 256);
        }
        if (t + 1 < 27) {
          const int t1 = t + 1;
          const int o1 = ((bd_off<SD>(t1 / 9) * LH + bd_off<SH>((t1 / 3) % 3)) * LWP + bd_off<SW>(t1 % 3)) * FCKP;
          a[t1 & 1][0] = *(const f32x4*)(lds + abase + o1);
          a[t1 & 1][1] = *(const f32x4*)(lds + abase + o1 + 4);
        }
        __builtin_amdgcn_sched_barrier(0);
        const int q = (bd_par<SD>(t / 9) * SH + bd_par<SH>((t / 3) % 3)) * SW + bd_par<SW>(t % 3);
        if (BDS_ABL & 8) { acc[q][0] += a[t & 1][0][0] + a[t & 1][1][3] + b[t % NB][0][1] + b[t % NB][1][2]; continue; }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t & 1][0][e], b[t % NB][0][e], acc[q], 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t & 1][1][e], b[t % NB][1][e], acc[q], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // ---- epilogue: class (pd,ph,pw) of dY position m lands at dX[S*m + par]
  const int co = ntile * 32 + li;
  const bool covalid = co < c.Cout;
  const int ocs = c.ocs0;
  const size_t out_sample = (size_t)c.OD * c.OH * c.OW;
  constexpr int OEB = mt_ebytes<OS>();
  __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)c.out0 + (size_t)nb * out_sample * ocs * OEB), 0,
                                                                (int)(out_sample * ocs * OEB), 0x00020000);
  const int md = md0 + dm;
  if (BDS_ABL & 4) { float t = 0.f; for (int q = 0; q < NC; ++q) t += acc[q][3] + acc[q][9]; if (t == 1234.5f) c.out0[0] = t; return; }
  if constexpr (OB) {
    // bf16 dX: channel-pair dwords (mt_pair_exchange) — even lanes own accumulator row j, odd lanes row j + 1; the read-modify-write of
    // an accumulating launch is pipelined one row pair ahead like the fp32 form below
    const bool odd = li & 1;
    const int coe = co & ~1;
    const bool pvalid = coe + 1 < c.Cout;
    auto pair_off = [&](int j, int (&off)[NC]) {
      const int iv = (j & 3) + 8 * (j >> 2) + 4 * lhalf + (odd ? 1 : 0);
      const int mh = mh0 + rbase + (iv >> 4), mw = mw0 + (iv & 15);
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        const int pd = q / (SH * SW), ph = (q / SW) % SH, pw = q % SW;
        const int xd = md * SD + pd, xh = mh * SH + ph, xw = mw * SW + pw;
        const bool ok = pvalid && xd < c.OD && xh < c.OH && xw < c.OW;
        off[q] = ok ? (((xd * c.OH + xh) * c.OW + xw) * ocs + coe) * 2 : (int)0x80000000;
      }
    };
    int poff[2][NC];
    unsigned pprev[2][NC];
    pair_off(0, poff[0]);
    if (c.accumulate) {
#pragma unroll
      for (int q = 0; q < NC; ++q) pprev[0][q] = __builtin_amdgcn_raw_buffer_load_b32(rd, poff[0][q], 0, 0);
    }
#pragma unroll
    for (int jp = 0; jp < 8; ++jp) {
      const int j = 2 * jp;
      if (jp + 1 < 8) {
        pair_off(j + 2, poff[(jp + 1) & 1]);
        if (c.accumulate) {
#pragma unroll
          for (int q = 0; q < NC; ++q) pprev[(jp + 1) & 1][q] = __builtin_amdgcn_raw_buffer_load_b32(rd, poff[(jp + 1) & 1][q], 0, 0);
        }
      }
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        float a, b;
        mt_pair_exchange(acc[q][j], acc[q][j + 1], odd, a, b);
        if (c.accumulate) { a += mt_lo16<OS>(pprev[jp & 1][q]); b += mt_hi16<OS>(pprev[jp & 1][q]); }
        __builtin_amdgcn_raw_buffer_store_b32(mt_pk16<OS>(a, b), rd, poff[jp & 1][q], 0, 0);
      }
    }
    return;
  }
  // Accumulating into dX (the skip connection wrote it first) is a read-modify-write of 16 x NC scattered dwords per lane: the
  // NC loads of accumulator row j+1 are requested before the NC stores of row j go out, so a row's round trip hides behind the
  // previous row's stores (one load -> add -> store chain per element cost 0.26 of 0.81 ms on 30 <- 60 @ 48x192x192)
  auto row_off = [&](int j, int (&off)[NC]) {
    const int iv = (j & 3) + 8 * (j >> 2) + 4 * lhalf;
    const int mh = mh0 + rbase + (iv >> 4), mw = mw0 + (iv & 15);
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const int pd = q / (SH * SW), ph = (q / SW) % SH, pw = q % SW;
      const int xd = md * SD + pd, xh = mh * SH + ph, xw = mw * SW + pw;
      const bool ok = covalid && xd < c.OD && xh < c.OH && xw < c.OW;
      off[q] = ok ? (((xd * c.OH + xh) * c.OW + xw) * ocs + co) * 4 : (int)0x80000000;
    }
  };
  int off[2][NC];
  float prev[2][NC];
  row_off(0, off[0]);
  if (c.accumulate) {
#pragma unroll
    for (int q = 0; q < NC; ++q) prev[0][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, off[0][q], 0, 0));
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j + 1 < 16) {
      row_off(j + 1, off[(j + 1) & 1]);
      if (c.accumulate) {
#pragma unroll
        for (int q = 0; q < NC; ++q)
          prev[(j + 1) & 1][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, off[(j + 1) & 1][q], 0, 0));
      }
    }
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      float v = acc[q][j];
      if (c.accumulate) v += prev[j & 1][q];
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rd, off[j & 1][q], 0, 0);
    }
  }
}

// The same backward-data on UNDER-FILLED grids (round 5): dY of 3x12x12 or 3x6x6 positions is 96 / 80 workgroups of 20 serial
// chunks x 216 MFMAs in the tiling above.  Here a workgroup owns ONE 32-position M tile (2 x 4 x 4 dY positions) x 32 dX channels
// and its four waves split the K of every chunk — wave w multiplies the channel pairs 2w, 2w + 1 of the chunk's eight, for all 27
// taps into all NC class tiles —, so the grid is 3-4 x larger and a wave's chain 4 x shorter; the four partial tiles of a class are
// summed through LDS in a fixed order (deterministic), class by class.  fp32 storage, 8-byte channel pairs.
template <int SD, int SH, int SW>
__global__ __launch_bounds__(256) void conv_bwdd_strided_ks_kernel(const ConvKParams P) {
  constexpr int TD = 2, TH = 4, TW = 4;
  constexpr int LD = TD + (SD == 2 ? 1 : 2), LH = TH + (SH == 2 ? 1 : 2), LW = TW + (SW == 2 ? 1 : 2);
  constexpr int NC = SD * SH * SW, LWP = stage_lwp<LD, LH, LW, 2>();
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  int ntile, td, th, tw, nb;
  mt_tile_coords(mt_block_decode(ntile), P.tilesD, P.tilesH, P.tilesW, td, th, tw, nb);
  const int md0 = td * TD, mh0 = th * TH, mw0 = tw * TW;
  // M row li -> dY position (li >> 4, (li >> 2) & 3, li & 3); the lane's eight channels of a chunk start at lhalf * 8, this wave's two
  // at + 2 wave (the MFMA pairs channel lhalf * 8 + k of both lane halves)
  const int abase = (((li >> 4) * LH + ((li >> 2) & 3)) * LWP + (li & 3)) * FCKP + lhalf * 8 + 2 * wave;

  f32x16 acc[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[q][j] = 0.f;

  for (int ch = 0; ch < P.nchunks; ++ch) {
    const ConvChunk cc = P.chunk[ch];
    // this wave's share of the chunk's weight fragments ([tap][group 2][lane 64][4]: group wave >> 1, floats 2 (wave & 1), + 1): all 27
    // requested before the staging, consumed behind its barrier
    const float* wl = c.wpack + (size_t)(ntile * P.nchunks + ch) * (27 * 512) + (wave >> 1) * 256 + lane * 4 + 2 * (wave & 1);
    float2 b[27];
#pragma unroll
    for (int t = 0; t < 27; ++t) b[t] = *(const float2*)(wl + t * 512);
    __syncthreads();
    mt_stage_fast2<LD, LH, LW, 2>(lds, c, cc, nb, md0 - (SD == 1 ? 1 : 0), mh0 - (SH == 1 ? 1 : 0), mw0 - (SW == 1 ? 1 : 0), lane, wave);
    __syncthreads();
    float2 a[2];
    {
      constexpr int o0 = ((bd_off<SD>(0) * LH + bd_off<SH>(0)) * LWP + bd_off<SW>(0)) * FCKP;
      a[0] = *(const float2*)(lds + abase + o0);
    }
#pragma unroll
    for (int t = 0; t < 27; ++t) {
      if (t + 1 < 27) {
        const int t1 = t + 1;
        const int o1 = ((bd_off<SD>(t1 / 9) * LH + bd_off<SH>((t1 / 3) % 3)) * LWP + bd_off<SW>(t1 % 3)) * FCKP;
        a[t1 & 1] = *(const float2*)(lds + abase + o1);
      }
      const int q = (bd_par<SD>(t / 9) * SH + bd_par<SH>((t / 3) % 3)) * SW + bd_par<SW>(t % 3);
      acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t & 1].x, b[t].x, acc[q], 0, 0, 0);
      acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t & 1].y, b[t].y, acc[q], 0, 0, 0);
    }
  }

  // ---- epilogue: class by class, the four waves' tiles summed in a fixed order; wave w finishes accumulator registers 4w .. 4w + 3
  // = M rows jj + 8 w + 4 lhalf; class (pd, ph, pw) of dY position m lands at dX[S m + par]
  const int co = ntile * 32 + li;
  const bool covalid = co < c.Cout;
  const int ocs = c.ocs0;
  const size_t out_sample = (size_t)c.OD * c.OH * c.OW;
  __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(c.out0 + (size_t)nb * out_sample * ocs), 0, (int)(out_sample * ocs * 4), 0x00020000);
  float* red = lds;                                        // [wave][16][64] floats = 16 KiB
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    const int pd = q / (SH * SW), ph = (q / SW) % SH, pw = q % SW;
    int off[4];
    float prev[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int iv = jj + 8 * wave + 4 * lhalf;
      const int xd = (md0 + (iv >> 4)) * SD + pd, xh = (mh0 + ((iv >> 2) & 3)) * SH + ph, xw = (mw0 + (iv & 3)) * SW + pw;
      const bool ok = covalid && xd < c.OD && xh < c.OH && xw < c.OW;
      off[jj] = ok ? (((xd * c.OH + xh) * c.OW + xw) * ocs + co) * 4 : (int)0x80000000;
      prev[jj] = 0.f;
      if (c.accumulate) prev[jj] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, off[jj], 0, 0));
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) red[(wave * 16 + j) * 64 + lane] = acc[q][j];
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const float* rp = red + (wave * 4 + jj) * 64 + lane;
      const float v = (((rp[0] + rp[16 * 64]) + rp[32 * 64]) + rp[48 * 64]) + prev[jj];
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rd, off[jj], 0, 0);
    }
    __syncthreads();
  }
}

#include "conv_wino.inc"

// ------------------------------------------------------------------------------------------------
// host side of mt_conv3d_fwd
struct ConvCfg { int MW, RH, TD, CK; };
static const ConvCfg kCfgs[] = {
  {32, 4, 2, 16}, {16, 2, 2, 16}, {8, 2, 2, 16}, {32, 4, 2, 8}, {16, 2, 2, 8}, {8, 2, 2, 8}, {32, 4, 4, 16},
};

static const ConvCfg kBfCfgs[] = { {32, 4, 4, 16}, {32, 4, 2, 16}, {16, 4, 2, 16} };    // tiles of conv_bf16_kernel: 4x4x32, 2x4x32, 2x8x16

static void cfg_tile(const ConvCfg& g, int* TD, int* TH, int* TW) {
  *TD = g.TD; *TH = (32 / g.MW) * g.RH; *TW = g.MW;
}
static size_t cfg_lds(const ConvCfg& g, const mt_conv3d_t* p) {
  int TD, TH, TW; cfg_tile(g, &TD, &TH, &TW);
  const size_t LD = (TD - 1) * p->SD + p->KD, LH = (TH - 1) * p->SH + p->KH, LW = (TW - 1) * p->SW + p->KW;
  size_t b = LD * LH * LW * g.CK * sizeof(float);
  return b < 1024 ? 1024 : b;
}
// choose the tile shape with the least padded work that fits LDS; prefer >=2 workgroups per CU
static int pick_cfg(const mt_conv3d_t* p) {
  int best = -1; double bestcost = 1e300;
  for (int i = 0; i < (int)(sizeof(kCfgs) / sizeof(kCfgs[0])); ++i) {
    const ConvCfg& g = kCfgs[i];
    const size_t l = cfg_lds(g, p);
    if (l > 160 * 1024) continue;
    int TD, TH, TW; cfg_tile(g, &TD, &TH, &TW);
    double vol = (double)mt_cdiv(p->Do, TD) * TD * mt_cdiv(p->Ho, TH) * TH * mt_cdiv(p->Wo, TW) * TW;
    double cost = vol;
    if (l > 80 * 1024) cost *= 1.25;       // one workgroup per CU: no load/compute overlap
    if (g.CK == 8) cost *= 1.10;           // more staging passes
    if (cost < bestcost - 1e-9) { bestcost = cost; best = i; }
  }
  return best;
}

static int conv_validate(const mt_conv3d_t* p) {
  MT_REQUIRE(p != nullptr, "conv3d: null params");
  MT_REQUIRE(p->nsrc == 1 || p->nsrc == 2, "conv3d: nsrc must be 1 or 2 (got %d)", p->nsrc);
  MT_REQUIRE(p->KD >= 1 && p->KD <= 3 && p->KH >= 1 && p->KH <= 3 && p->KW >= 1 && p->KW <= 3, "conv3d: kernel size must be 1..3");
  MT_REQUIRE(p->SD >= 1 && p->SD <= 2 && p->SH >= 1 && p->SH <= 2 && p->SW >= 1 && p->SW <= 2, "conv3d: stride must be 1 or 2");
  MT_REQUIRE((p->dilD == 1 || p->dilD == 2) && (p->dilH == 1 || p->dilH == 2) && (p->dilW == 1 || p->dilW == 2), "conv3d: dilation (zero insertion) must be 1 or 2");
  int csum = p->src[0].C + (p->nsrc == 2 ? p->src[1].C : 0);
  MT_REQUIRE(csum == p->Cin, "conv3d: source channels (%d) != Cin (%d)", csum, p->Cin);
  MT_REQUIRE(p->N > 0 && p->Do > 0 && p->Ho > 0 && p->Wo > 0 && p->Cout > 0 && p->Cin > 0, "conv3d: empty problem");
  MT_REQUIRE(p->wpack != nullptr && p->out0 != nullptr, "conv3d: null pointers");
  MT_REQUIRE(p->csplit >= p->Cout || p->out1 != nullptr, "conv3d: out1 required when csplit < Cout");
  return MT_OK;
}

// ---- eligibility of the kernel families (read by conv_resolve alone)
static bool conv_slopes_ok(const mt_conv3d_t* p) {     // the lean staging computes LeakyReLU as max(t, slope*t)
  for (int i = 0; i < p->nsrc; ++i)
    if (p->src[i].scale != nullptr && !(p->src[i].slope >= 0.f && p->src[i].slope <= 1.f)) return false;
  return true;
}
static bool conv_is_fast(const mt_conv3d_t* p) {
  if (!conv_slopes_ok(p)) return false;
  if (!(p->KD == 3 && p->KH == 3 && p->KW == 3 && p->SD == 1 && p->SH == 1 && p->SW == 1 && p->PD == 1 && p->PH == 1 &&
        p->PW == 1 && p->dilD == 1 && p->dilH == 1 && p->dilW == 1)) return false;
  for (int i = 0; i < p->nsrc; ++i)
    if ((double)p->Di * p->Hi * p->Wi * p->src[i].cs * 4.0 >= 2147483648.0) return false;  // 31-bit buffer offsets per sample
  return true;
}
// 1x3x3, stride 1, pad (0,1,1): the first stage of the residual encoder (generic_modular_residual_UNet.py:28-118, plan kernels)
static bool conv_is_133(const mt_conv3d_t* p) {
  if (!conv_slopes_ok(p)) return false;
  if (!(p->KD == 1 && p->KH == 3 && p->KW == 3 && p->SD == 1 && p->SH == 1 && p->SW == 1 && p->PD == 0 && p->PH == 1 &&
        p->PW == 1 && p->dilD == 1 && p->dilH == 1 && p->dilW == 1)) return false;
  for (int i = 0; i < p->nsrc; ++i)
    if ((double)p->Di * p->Hi * p->Wi * p->src[i].cs * 4.0 >= 2147483648.0) return false;
  return true;
}
// whether the destination(s) can be written as bf16 dwords (channel pairs: even channel counts / strides / split, dword-aligned bases)
static bool out_pairs_aligned(const mt_conv3d_t* p) {
  if ((p->Cout & 1) || (p->ocs0 & 1) || (((uintptr_t)p->out0) & 3)) return false;
  if (p->csplit < p->Cout && ((p->csplit & 1) || (p->ocs1 & 1) || (((uintptr_t)p->out1) & 3))) return false;
  return true;
}
static bool conv_fast_strided_ok(const mt_conv3d_t* p) {
  if (!conv_slopes_ok(p)) return false;
  if (!(p->KD == 3 && p->KH == 3 && p->KW == 3 && p->PD == 1 && p->PH == 1 && p->PW == 1)) return false;
  if (!(p->dilD == 1 && p->dilH == 1 && p->dilW == 1 && p->SH == 2 && p->SW == 2 && (p->SD == 1 || p->SD == 2))) return false;
  if (p->csplit < p->Cout || p->osD > 0) return false;
  for (int i = 0; i < p->nsrc; ++i)
    if ((double)p->Di * p->Hi * p->Wi * p->src[i].cs * 4.0 >= 2147483648.0) return false;
  if ((double)p->Do * p->Ho * p->Wo * p->ocs0 * 4.0 >= 2147483648.0) return false;
  return true;
}
// ---- bf16 matrix inputs (conv_bf16.inc)
static int conv_bf16_cfg(const mt_conv3d_t* p) {
  const int use = mt_sel3(p, MT_SEL_M16);       // 0 never; 1 where the grid fills the chip; 2 wherever eligible
  if (!use || !(conv_is_fast(p) || conv_is_133(p)) || p->osD > 0 || p->Cin < 16 || conv_fast_vec(p) != 2) return -1;
  if ((double)p->Do * p->Ho * p->Wo * p->ocs0 * 4.0 >= 2147483648.0) return -1;            // 31-bit store offsets per sample
  if (p->csplit < p->Cout && (double)p->Do * p->Ho * p->Wo * p->ocs1 * 4.0 >= 2147483648.0) return -1;
  if (mt_cdiv(p->src[0].C, FCK) + (p->nsrc == 2 ? mt_cdiv(p->src[1].C, FCK) : 0) > MT_MAX_CHUNKS) return -1;
  int best = -1; double bestcost = 1e300;
  for (int i = 0; i < (int)(sizeof(kBfCfgs) / sizeof(kBfCfgs[0])); ++i) {
    int TD, TH, TW; cfg_tile(kBfCfgs[i], &TD, &TH, &TW);
    const double vol = (double)mt_cdiv(p->Do, TD) * TD * mt_cdiv(p->Ho, TH) * TH * mt_cdiv(p->Wo, TW) * TW;
    const double halo = (double)(TD + 2) * (TH + 2) * (TW + 2) / ((double)TD * TH * TW);
    const double cost = vol * (0.5 + 0.5 * halo / 2.0);
    if (cost < bestcost - 1e-9) { bestcost = cost; best = i; }
  }
  if (best < 0) return -1;
  int TD, TH, TW; cfg_tile(kBfCfgs[best], &TD, &TH, &TW);
  const long wgs = (long)p->N * mt_cdiv(p->Do, TD) * mt_cdiv(p->Ho, TH) * mt_cdiv(p->Wo, TW) * mt_cdiv(p->Cout, 32);
  if (wgs < 256 && use != 2) return -1;          // low-resolution stages stay on the fp32 latency-oriented kernels
  return best;
}
static bool strided_use_bf16(const mt_conv3d_t* p) {      // forward strided stage convs (and the tap-split kernel) in mixed precision
  return mt_sel3(p, MT_SEL_M16) && p->mma == 1 && p->Cin >= 16 && conv_fast_vec(p) == 2;
}

// conv_x16_kernel (conv_x16.hip): the conv_bf16_kernel problems on the 4 x 4 x 32 tile with ONE 16-bit storage type on all operands and one
// destination — persistent workgroups, weight fragments in LDS, register prefetch of the next (tile, chunk) step, 16-byte stores.
// mt_conv3d_t.select MT_SEL_X16: default = where it measured faster than conv_bf16_kernel (one cout tile, or >= 8 channel chunks:
// tools/bench_fwd16.py) | OFF = conv_bf16_kernel everywhere | FORCE: wherever eligible; max_workgroups caps the persistent grid
// (tests: several tiles per workgroup)
static bool conv_x16_geometry_ok(const mt_conv3d_t* p, int cfg) {
  if (cfg != 0 || p->mma != 1) return false;
  const int sd = conv_src_dtype(p);
  if (!mt_is16(sd) || p->odtype != sd || !out_pairs_aligned(p)) return false;
  if (p->csplit < p->Cout || p->osD > 0 || p->bstats.y != nullptr) return false;
  if (!(p->KH == 3 && p->KW == 3 && (p->KD == 3 || p->KD == 1) && p->SD == 1 && p->SH == 1 && p->SW == 1 && p->PH == 1 && p->PW == 1 &&
        p->PD == (p->KD == 3 ? 1 : 0) && p->dilD == 1 && p->dilH == 1 && p->dilW == 1)) return false;
  for (int i = 0; i < p->nsrc; ++i) {
    if ((double)p->Di * p->Hi * p->Wi * p->src[i].cs * 2.0 >= 2147483648.0) return false;
    if ((p->src[i].cs & 1) || (((uintptr_t)p->src[i].ptr) & 3)) return false;
    if (p->src[i].scale != nullptr && !(p->src[i].slope >= 0.f && p->src[i].slope <= 1.f)) return false;
  }
  if ((double)p->Do * p->Ho * p->Wo * p->ocs0 * 2.0 >= 2147483648.0) return false;
  if ((long)p->N * mt_cdiv(p->Do, 4) * mt_cdiv(p->Ho, 4) * mt_cdiv(p->Wo, 32) * mt_cdiv(p->Cout, 32) >= 2147483647L) return false;
  return true;
}
static bool conv_x16_ok(const mt_conv3d_t* p, int cfg) {
  const int g_x16 = mt_sel3(p, MT_SEL_X16);
  if (!g_x16) return false;
  if (g_x16 == 1) {
    const int nch = mt_cdiv(p->src[0].C, FCK) + (p->nsrc == 2 ? mt_cdiv(p->src[1].C, FCK) : 0);
    if (p->Cout > 32 && nch < 8) return false;
  }
  return conv_x16_geometry_ok(p, cfg);
}

// Packed patch geometry of the persistent kernel: a task's linear offset (ld*Hi + lh)*Wi + lw with ld, lh <= 5 and lw <= 17 lives
// in bits 0-19 of a table entry, so its maximum (5*Hi + 5)*Wi + 17 must stay below 2^20 (beyond that the offset would spill into
// the ld bits); larger planes take the direct kernels.
static bool wino_persist_geometry_ok(const mt_conv3d_t* p) { return (5.0 * p->Hi + 5.0) * p->Wi + 17.0 < 1048576.0; }
// Winograd eligibility: FAST geometry, 8-byte channel pairs in every source, one destination, enough workgroups to fill
// the chip with 4x4x16 tiles and enough input channels to amortise the transforms
static bool conv_wino_ok(const mt_conv3d_t* p) {
  const int use = mt_sel3(p, MT_SEL_WINO);
  if (!use) return false;
  if (p->Cin < 16 || conv_fast_vec(p) != 2 || !wino_persist_geometry_ok(p)) return false;
  if (p->csplit < p->Cout && (double)p->Do * p->Ho * p->Wo * p->ocs1 * 4.0 >= 2147483648.0) return false;
  if (mt_cdiv(p->src[0].C, WCK) + (p->nsrc == 2 ? mt_cdiv(p->src[1].C, WCK) : 0) > MT_MAX_CHUNKS) return false;
  if ((double)p->Do * p->Ho * p->Wo * p->ocs0 * 4.0 >= 2147483648.0) return false;
  const long wgs = (long)p->N * mt_cdiv(p->Do, 4) * mt_cdiv(p->Ho, 4) * mt_cdiv(p->Wo, 16) * mt_cdiv(p->Cout, 32);
  return wgs >= 256 || use == 2;          // MT_SEL_FORCE in the MT_SEL_WINO field forces it (tests on small shapes)
}
// mt_bwd_stats_t is implemented in the epilogue of the persistent register-staged Winograd kernel (conv_wino8pb_kernel)
static bool wino_serves_bwd_stats(const mt_conv3d_t* p) {
  return wino_persist_geometry_ok(p);
}

// kernel == stride, pad 0, one plain destination, no statistics: every output owns its input block (conv_gather_kernel)
static bool conv_gather_ok(const mt_conv3d_t* p) {
  if (p->nsrc != 1 || p->csplit < p->Cout || p->osD > 0 || p->stats_part != nullptr) return false;
  if (!(p->KD == p->SD && p->KH == p->SH && p->KW == p->SW && p->PD == 0 && p->PH == 0 && p->PW == 0)) return false;
  if (!(p->dilD == 1 && p->dilH == 1 && p->dilW == 1)) return false;
  if ((double)p->Do * p->Ho * p->Wo * p->ocs0 * 4.0 >= 2147483648.0) return false;
  return true;
}
static bool gather_use_bf16(const mt_conv3d_t* p) {          // mixed precision: a bf16 gradient without a lazy activation
  return p->mma == 1 && p->src[0].dtype == MT_BF16 && p->src[0].scale == nullptr && !(p->src[0].cs & 1) && !(((uintptr_t)p->src[0].ptr) & 3);
}
// two cout tiles per wave: fp32 on both sides, at least two tiles, and a grid that still fills the chip four times over (measured, tools/bench_gather.py:
// 30 -> 60 @ 2x24x96x96 outputs 280 -> 231 us (218 with the chunk pairs and the wide epilogue), 60 -> 120 @ 12x48x48 97 -> 99, 120 -> 240 @ 6x24x24 70 -> 83 -
// the smaller levels need the workgroups more than the halved gather).  GATHER_NT2 0: the one-tile form everywhere.
#ifndef GATHER_NT2
#define GATHER_NT2 1
#endif
static bool gather_nt2(const mt_conv3d_t* p) {
  if (!(GATHER_NT2 && !gather_use_bf16(p) && p->src[0].dtype == MT_F32 && p->odtype == MT_F32 && p->Cout > 32)) return false;
  const long wgs = (((long)p->Do * p->Ho * p->Wo + 127) / 128) * p->N * mt_cdiv(mt_cdiv(p->Cout, 32), 2);
  return wgs >= 4L * mt_device_cus(mt_current_device());
}

static size_t rt_lds(const ConvCfg& g, const mt_conv3d_t* p) {
  int TD, TH, TW; cfg_tile(g, &TD, &TH, &TW);
  const size_t LD = (TD - 1) * p->SD + p->KD, LH = (TH - 1) * p->SH + p->KH, LW = (TW - 1) * p->SW + p->KW;
  size_t b = LD * LH * LW * FCKP * sizeof(float);
  return b < 1024 ? 1024 : b;
}
static bool conv_rt_ok(const mt_conv3d_t* p) {
  if (!(p->dilD == 1 && p->dilH == 1 && p->dilW == 1)) return false;
  if (p->csplit < p->Cout && (p->osD > 0 || (double)p->Do * p->Ho * p->Wo * p->ocs1 * 4.0 >= 2147483648.0)) return false;
  for (int i = 0; i < p->nsrc; ++i)
    if ((double)p->Di * p->Hi * p->Wi * p->src[i].cs * 4.0 >= 2147483648.0) return false;
  const double od = p->osD > 0 ? (double)p->OD * p->OH * p->OW : (double)p->Do * p->Ho * p->Wo;
  if (od * p->ocs0 * 4.0 >= 2147483648.0) return false;
  return true;
}
// tile shape for the runtime kernel: least padded work among the shapes whose LDS tile fits (prefer two workgroups per CU)
static int pick_rt_cfg(const mt_conv3d_t* p) {
  int best = -1; double bestcost = 1e300;
  for (int i = 0; i < 3; ++i) {
    const ConvCfg& g = kCfgs[i];
    const size_t l = rt_lds(g, p);
    if (l > 160 * 1024) continue;
    int TD, TH, TW; cfg_tile(g, &TD, &TH, &TW);
    double cost = (double)mt_cdiv(p->Do, TD) * TD * mt_cdiv(p->Ho, TH) * TH * mt_cdiv(p->Wo, TW) * TW;
    if (l > 80 * 1024) cost *= 1.15;
    if (cost < bestcost - 1e-9) { bestcost = cost; best = i; }
  }
  return best;
}

// ---- the one dispatch decision of mt_conv3d_fwd.  conv_resolve is the only reader of the eligibility predicates above; the queries, the
// kernel name and the launchers are functions of the ConvChoice it returns (and of plain fields of p).
enum ConvFamily { CONV_NONE = 0, CONV_STEM, CONV_WINO, CONV_WINO_B, CONV_FAST, CONV_TAPSPLIT, CONV_FAST_STRIDED, CONV_BF16, CONV_X16, CONV_GATHER,
                  CONV_RT, CONV_GENERIC };
struct ConvChoice {
  int family;        // CONV_NONE: no tile configuration of the generic kernel fits LDS
  ConvCfg g;         // tile configuration of the tiled kernels (conv_tile for the spatial tile of every family)
  int ck;            // channels per chunk = the ck argument of mt_pack_conv_weights
  // the template instance: staging width, storage types of sources and destination, matrix type, 16-bit matrix inputs
  int vec, xs, os, mty;
  bool m16;
  bool nt2;          // conv_gather_kernel: two cout tiles per wave
  bool bstats;       // the Winograd families: mt_bwd_stats_t is served (CONV_WINO_B computes it)
  bool fast;         // FAST flag of conv_fwd_kernel
};
static ConvChoice conv_resolve(const mt_conv3d_t* p) {
  ConvChoice c = {};
  const int cfg = pick_cfg(p), sd = conv_src_dtype(p);
  c.family = cfg < 0 ? CONV_NONE : CONV_GENERIC;
  if (cfg >= 0) c.g = kCfgs[cfg];
  c.ck = c.g.CK; c.vec = conv_fast_vec(p); c.xs = MT_F32; c.os = MT_F32; c.mty = MT_BF16;
  // the strided and tap-split kernels in mixed precision: a 16-bit source multiplies as its own type (fp16 activations: the forward pass;
  // bf16: gradients) and the destination has the source's type, or fp32 (a level the engine keeps in fp32); fp32 sources round to bf16
  auto strided_instance = [&] {
    c.m16 = strided_use_bf16(p);
    if (c.m16 && sd > 0) { c.vec = 4; c.xs = sd; c.os = p->odtype == sd ? sd : MT_F32; c.mty = sd == MT_F16 ? MT_F16 : MT_BF16; }
  };
  if (p->mma == 1) {                      // 16-bit matrix inputs where the bf16 kernel serves the problem; fp32 kernels elsewhere
    const int bc = conv_bf16_cfg(p);
    if (bc >= 0) {
      // storage: all fp32 (bf16 matrix type), all bf16 (backward-data over gradients) or all fp16 (forward over activations: fp16 matrix
      // type); 16-bit sources are read as 8-byte groups of four channels (fp32: 16-byte staging loads measured slower, 0.409 vs 0.372 ms
      // on 32->32), 16-bit destinations written as channel-pair dwords
      c.family = conv_x16_ok(p, bc) ? CONV_X16 : CONV_BF16;
      c.g = kBfCfgs[bc]; c.ck = FCK; c.m16 = true;
      c.vec = sd > 0 ? 4 : 2; c.xs = c.os = sd > 0 ? sd : MT_F32; c.mty = sd == MT_F16 ? MT_F16 : MT_BF16;
      return c;
    }
  }
  const bool fast = conv_is_fast(p), small = cfg >= 0 && cfg <= 2 && p->osD <= 0;
  const bool out31 = (double)p->Do * p->Ho * p->Wo * p->ocs0 * 4.0 < 2147483648.0;         // 31-bit store offsets per sample
  if (fast && p->osD <= 0 && p->nsrc == 1 && p->Cin == 1 && p->csplit >= p->Cout && out31) {
    c.family = CONV_STEM; c.g = kCfgs[0]; c.ck = c.g.CK; c.os = p->odtype;
    return c;
  }
  if (fast && small && conv_wino_ok(p)) {
    c.bstats = wino_serves_bwd_stats(p);
    c.family = p->bstats.y != nullptr ? CONV_WINO_B : CONV_WINO; c.ck = WCK;
    return c;
  }
  if (fast && small) {
    c.family = CONV_FAST;
    // low-resolution stages: fewer than two workgroups per CU -> split the taps over the waves instead
    int TD, TH, TW; cfg_tile(c.g, &TD, &TH, &TW);
    const long wgs = (long)p->N * mt_cdiv(p->Do, TD) * mt_cdiv(p->Ho, TH) * mt_cdiv(p->Wo, TW) * mt_cdiv(p->Cout, 32);
    if (mt_sel3(p, MT_SEL_TAPSPLIT) && wgs < 300 && p->csplit >= p->Cout && out31) { c.family = CONV_TAPSPLIT; strided_instance(); }
    return c;
  }
  if (conv_is_133(p) && small && p->Cin >= 8) { c.family = CONV_FAST; return c; }      // compile-time taps instead of conv_rt
  if (conv_fast_strided_ok(p)) {
    c.family = CONV_FAST_STRIDED; c.g = kCfgs[0]; c.ck = c.g.CK;
    strided_instance();
    // fewer workgroups than CUs in the 2x4x8 x 64-channel tiling: one 32-voxel tile x 32 channels per workgroup, taps over the waves
    // (instances: fp32 with 8-byte channel pairs, or 16-bit storage)
    const int g_tapsplit = mt_sel3(p, MT_SEL_TAPSPLIT);
    const long wgs = (long)p->N * mt_cdiv(p->Do, 2) * mt_cdiv(p->Ho, 4) * mt_cdiv(p->Wo, 8) * mt_cdiv(p->Cout, 64);
    const bool inst = c.m16 ? mt_is16(sd) && (p->odtype == sd || p->odtype == MT_F32) : (sd == MT_F32 && p->odtype == MT_F32 && c.vec == 2);
    if (g_tapsplit && (wgs < 256 || g_tapsplit >= 2) && inst) c.family = CONV_TAPSPLIT;
    return c;
  }
  if (conv_rt_ok(p)) {
    const int i = pick_rt_cfg(p);
    if (i >= 0) {
      c.family = CONV_RT; c.g = kCfgs[i]; c.ck = c.g.CK;
      if (conv_gather_ok(p)) {           // gradients: bf16 -> bf16 (backward-data of a transposed convolution between two 16-bit levels), bf16 -> fp32, fp32 -> bf16
        // 16-byte loads at any alignment (dword-aligned dwordx4 buffer loads are legal and range-checked per dword: tools/ubench/oob128.hip)
        c.family = CONV_GATHER; c.ck = FCK; c.vec = 4; c.xs = p->src[0].dtype; c.os = p->odtype;
        c.m16 = gather_use_bf16(p); c.nt2 = gather_nt2(p);
      }
      return c;
    }
  }
  c.fast = fast && (cfg <= 3 || cfg == 6);
  return c;
}
struct ConvTile { int D, H, W; };
// spatial output tile of a workgroup (conv_gather_kernel walks 128 voxels in linear order and takes no statistics: the tile of its
// conv_rt configuration only sizes mt_conv3d_stats_blocks, as before)
static ConvTile conv_tile(const ConvChoice& c) {
  switch (c.family) {
    case CONV_FAST_STRIDED: return {2, 4, 8};
    case CONV_TAPSPLIT: return {2, 4, 4};
    case CONV_WINO: case CONV_WINO_B: return {4, 4, 16};
    default: { ConvTile t; cfg_tile(c.g, &t.D, &t.H, &t.W); return t; }
  }
}

extern "C" int mt_conv3d_ck(const mt_conv3d_t* p) {
  const ConvChoice c = conv_resolve(p);
  return c.family == CONV_NONE ? -1 : c.ck;
}
extern "C" int mt_conv3d_pack_layout(const mt_conv3d_t* p) {      // layout argument of mt_pack_conv_weights for this problem
  const ConvChoice c = conv_resolve(p);
  if (c.m16) return c.mty == MT_F16 ? 4 : 3;         // fp16 sources multiply as fp16, everything else as bf16
  return (c.family == CONV_WINO || c.family == CONV_WINO_B) ? 2 : 1;
}
extern "C" int mt_conv3d_stats_blocks(const mt_conv3d_t* p) {
  const ConvChoice c = conv_resolve(p);
  if (c.family == CONV_NONE) return -1;
  const ConvTile t = conv_tile(c);
  return mt_cdiv(p->Do, t.D) * mt_cdiv(p->Ho, t.H) * mt_cdiv(p->Wo, t.W);
}
extern "C" int mt_conv3d_bwd_stats_supported(const mt_conv3d_t* p) {
  if (p == nullptr || conv_validate(p) != MT_OK) return 0;
  return conv_resolve(p).bstats ? 1 : 0;
}

// Storage types (mt_src_t.dtype, mt_conv3d_t.odtype): 1 when the kernel that serves p reads / writes them natively.  All-fp32 is
// always supported; 16-bit storage is taken by the 16-bit matrix kernels (p->mma == 1): conv_bf16_kernel with ONE 16-bit type on all
// operands (fp16: the forward pass, fp16 products; bf16: backward-data, bf16 products), the strided stage kernel with 16-bit sources
// (destination of the same type, or fp32).  Elsewhere the caller converts with mt_cast.
static int conv_io_served(const mt_conv3d_t* p, const ConvChoice& c) {
  const int sd = conv_src_dtype(p);
  if (sd < 0 || !mt_dtype_ok(p->odtype)) return 0;
  if (sd == MT_F32 && p->odtype == MT_F32) return 1;
  if (p->bstats.y != nullptr) return 0;
  switch (c.family) {
    case CONV_BF16: case CONV_X16: return (mt_is16(sd) && p->odtype == sd && out_pairs_aligned(p)) ? 1 : 0;
    case CONV_FAST_STRIDED: case CONV_TAPSPLIT:
      return (c.m16 && mt_is16(sd) && (p->odtype == MT_F32 || (p->odtype == sd && out_pairs_aligned(p)))) ? 1 : 0;
    case CONV_STEM: return (sd == MT_F32 && out_pairs_aligned(p)) ? 1 : 0;          // fp32 network input, any output type
    case CONV_GATHER:                                                                // gradients: fp32 / bf16 on either side
      if (sd == MT_F16 || p->odtype == MT_F16) return 0;
      if (sd == MT_BF16 && ((p->src[0].cs & 1) || (((uintptr_t)p->src[0].ptr) & 3))) return 0;
      return (p->odtype == MT_F32 || out_pairs_aligned(p)) ? 1 : 0;
    default: return 0;
  }
}
extern "C" int mt_conv3d_io_supported(const mt_conv3d_t* p) {
  if (p == nullptr) return 0;
  return conv_io_served(p, conv_resolve(p));
}

// name of the device kernel mt_conv3d_fwd will launch for this problem (as rocprofv3 prints it) — lets the benchmark
// attribute per-launch timings to the same kernel names the profiler reports
extern "C" int mt_conv3d_kernel_name(const mt_conv3d_t* p, char* buf, size_t n) {
  if (p == nullptr || buf == nullptr || n == 0) return MT_EINVAL;
  const ConvChoice c = conv_resolve(p);
  const ConvCfg& g = c.g;
  const char* b = c.m16 ? "true" : "false";
  switch (c.family) {
    case CONV_STEM: snprintf(buf, n, "conv_stem_kernel<%d>", c.os); break;
    case CONV_WINO: snprintf(buf, n, "conv_wino8p_kernel"); break;
    case CONV_WINO_B: snprintf(buf, n, "conv_wino8pb_kernel"); break;
    case CONV_FAST: snprintf(buf, n, "conv_fast_kernel<%d, %d, %d, %d, %d>", g.MW, g.RH, g.TD, c.vec, p->KD); break;
    case CONV_TAPSPLIT:
      if (p->SH == 2) snprintf(buf, n, "conv_tapsplit_kernel<%d, %s, %d, %d, %d, %d, 2, 2>", c.vec, b, c.xs, c.os, c.mty, p->SD);
      else snprintf(buf, n, "conv_tapsplit_kernel<%d, %s, %d, %d, %d>", c.vec, b, c.xs, c.os, c.mty);
      break;
    case CONV_FAST_STRIDED: snprintf(buf, n, "conv_fast_strided_kernel<%d, %d, %d, %d, %s, %d, %d, %d>", p->SD, p->SH, p->SW, c.vec, b, c.xs, c.os, c.mty); break;
    case CONV_BF16: snprintf(buf, n, "conv_bf16_kernel<%d, %d, %d, %d, 1, 4, %d, %d, %d, %d>", g.MW, g.RH, g.TD, c.vec, p->KD, c.xs, c.os, c.mty); break;   // <MW, RH, TD, VEC, NT, NW, KD, XS, OS, MTY>
    case CONV_X16: snprintf(buf, n, "conv_x16_kernel<%d, %d>", p->KD, c.xs); break;
    case CONV_GATHER: snprintf(buf, n, c.m16 ? "conv_gather_kernel<%d, %d, %d, true>" : c.nt2 ? "conv_gather_kernel<%d, %d, %d, false, 2>" : "conv_gather_kernel<%d, %d, %d>", c.vec, c.xs, c.os); break;
    case CONV_RT: snprintf(buf, n, "conv_rt_kernel<%d, %d, %d, %d>", g.MW, g.RH, g.TD, c.vec); break;
    case CONV_GENERIC: snprintf(buf, n, "conv_fwd_kernel<%d, %d, %d, %d, %s>", g.MW, g.RH, g.TD, g.CK, c.fast ? "true" : "false"); break;
    default: return MT_EINVAL;
  }
  return MT_OK;
}

// ---- launchers: each switches from the choice's runtime values to the template instance
// kernel arguments of a tiled launch: the problem (a single source aliased into the empty second slot), the tile counts over the output and the channel chunks
static int conv_fill(ConvKParams& P, const mt_conv3d_t* p, const ConvTile& t, int ntaps, int ck) {
  P.c = *p;
  if (P.c.nsrc == 1) { P.c.src[1] = P.c.src[0]; P.c.src[1].C = 0; }
  P.tilesD = mt_cdiv(p->Do, t.D); P.tilesH = mt_cdiv(p->Ho, t.H); P.tilesW = mt_cdiv(p->Wo, t.W);
  P.nsb = P.tilesD * P.tilesH * P.tilesW;
  P.ntaps = ntaps; P.dbg = 0; P.stagger = 0;
  P.nchunks = mt_build_chunks(p->src[0].C, p->nsrc == 2 ? p->src[1].C : 0, ck, P.chunk);
  MT_REQUIRE(P.nchunks > 0, "conv3d: too many channel chunks (Cin=%d, ck=%d)", p->Cin, ck);
  return MT_OK;
}
// launch with `ldsb` bytes of dynamic LDS, raising the kernel's limit where that exceeds the default 64 KiB
template <class K>
static int conv_launch_lds(K kfn, dim3 grid, dim3 block, size_t ldsb, hipStream_t st, const ConvKParams& P, const char* what) {
  if (ldsb > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb);
    if (e != hipSuccess) { mt_set_error("conv3d: cannot raise dynamic LDS to %zu: %s", ldsb, hipGetErrorString(e)); return MT_EHIP; }
  }
  hipLaunchKernelGGL(kfn, grid, block, ldsb, st, P);
  MT_CHECK_LAUNCH(what);
  return MT_OK;
}
static dim3 conv_grid(const ConvKParams& P, int cout_per_wg) {
  return dim3((unsigned)(P.nsb * P.c.N), (unsigned)mt_cdiv(P.c.Cout, cout_per_wg), 1);
}

static int launch_fast(const mt_conv3d_t* p, const ConvChoice& c, hipStream_t st) {
  ConvKParams P;
  if (int rc = conv_fill(P, p, conv_tile(c), p->KD * 9, FCK)) return rc;
#define MT_F_INST(MW_, RH_, TD_, VEC_, KD_) \
  conv_launch_lds(conv_fast_kernel<MW_, RH_, TD_, VEC_, KD_>, conv_grid(P, 32), dim3(256), stage_lds_bytes<TD_ + KD_ - 1, (32 / MW_) * RH_ + 2, MW_ + 2, VEC_>(), st, P, "conv3d_fast")
#define MT_F_CASE(MW_, RH_, TD_)                                                                                           \
  if (c.g.MW == MW_) {                                                                                                     \
    if (p->KD == 1) return c.vec == 2 ? MT_F_INST(MW_, RH_, TD_, 2, 1) : MT_F_INST(MW_, RH_, TD_, 1, 1);                   \
    return c.vec == 2 ? MT_F_INST(MW_, RH_, TD_, 2, 3) : MT_F_INST(MW_, RH_, TD_, 1, 3);                                   \
  }
  MT_F_CASE(32, 4, 2)
  MT_F_CASE(16, 2, 2)
  MT_F_CASE(8, 2, 2)
#undef MT_F_CASE
#undef MT_F_INST
  return MT_EINVAL;
}

// the 16-bit instances of the strided and tap-split kernels: (source, destination, matrix type) = (fp16, fp16 | fp32, fp16), (bf16, bf16 | fp32, bf16)
#define MT_IO16_SWITCH(c_, LAUNCH_)                                                        \
  do {                                                                                     \
    if (c_.xs == MT_F16 && c_.os == MT_F16) LAUNCH_(MT_F16, MT_F16, MT_F16);               \
    else if (c_.xs == MT_F16) LAUNCH_(MT_F16, MT_F32, MT_F16);                             \
    else if (c_.os == MT_BF16) LAUNCH_(MT_BF16, MT_BF16, MT_BF16);                         \
    else LAUNCH_(MT_BF16, MT_F32, MT_BF16);                                                \
  } while (0)

template <int SD>
static int launch_fast_strided_t(const mt_conv3d_t* p, const ConvChoice& c, hipStream_t st) {
  constexpr int TD = 2, TH = 4, TW = 8, LD = (TD - 1) * SD + 3, LH = (TH - 1) * 2 + 3, LW = (TW - 1) * 2 + 3;
  ConvKParams P;
  if (int rc = conv_fill(P, p, conv_tile(c), 27, FCK)) return rc;
  const dim3 grid = conv_grid(P, 64);
#define MT_FS_LAUNCH(XS_, OS_, MTY_) hipLaunchKernelGGL((conv_fast_strided_kernel<SD, 2, 2, 4, true, XS_, OS_, MTY_>), grid, dim3(256), (bstage_lds_bytes<LD, LH, LW, 4, 4>()), st, P)
  if (c.m16 && c.vec == 4) MT_IO16_SWITCH(c, MT_FS_LAUNCH);
  else if (c.m16) hipLaunchKernelGGL((conv_fast_strided_kernel<SD, 2, 2, 2, true, MT_F32, MT_F32, MT_BF16>), grid, dim3(256), (bstage_lds_bytes<LD, LH, LW, 2, 4>()), st, P);
  else if (c.vec == 2) hipLaunchKernelGGL((conv_fast_strided_kernel<SD, 2, 2, 2>), grid, dim3(256), (stage_lds_bytes<LD, LH, LW, 2>()), st, P);
  else return conv_launch_lds(conv_fast_strided_kernel<SD, 2, 2, 1>, grid, dim3(256), stage_lds_bytes<LD, LH, LW, 1>(), st, P, "conv3d_fast_strided");
#undef MT_FS_LAUNCH
  MT_CHECK_LAUNCH("conv3d_fast_strided");
  return MT_OK;
}

// SD, S2: depth and in-plane stride.  The strided forms exist as the 16-bit instances and as fp32 with 8-byte channel pairs (conv_resolve
// takes the tap-split kernel only there); stride 1 also stages fp32 as bf16 and single channels.
template <int SD, int S2>
static void launch_tapsplit_t(const ConvChoice& c, dim3 grid, hipStream_t st, const ConvKParams& P) {
  constexpr int LD = SD + 3, LH = 3 * S2 + 3;        // staged extent of the 2 x 4 x 4 tile
  size_t l = (size_t)4 * 16 * 64 * sizeof(float);    // at least the cross-wave reduction buffer
#define MT_TS_LAUNCH(VEC_, BF_, XS_, OS_, MTY_) hipLaunchKernelGGL((conv_tapsplit_kernel<VEC_, BF_, XS_, OS_, MTY_, SD, S2, S2>), grid, dim3(256), l, st, P)
#define MT_TS_LAUNCH16(XS_, OS_, MTY_) MT_TS_LAUNCH(4, true, XS_, OS_, MTY_)
  if (c.m16 && c.vec == 4) {
    l = std::max(l, bstage_lds_bytes<LD, LH, LH, 4, 4>());
    MT_IO16_SWITCH(c, MT_TS_LAUNCH16);
  } else if (!c.m16 && c.vec == 2) {
    l = std::max(l, stage_lds_bytes<LD, LH, LH, 2>());
    MT_TS_LAUNCH(2, false, MT_F32, MT_F32, MT_BF16);
  } else if constexpr (S2 == 1) {
    if (c.m16) {                                     // fp32 sources rounded to bf16 in the staging
      l = std::max(l, bstage_lds_bytes<LD, LH, LH, 2, 4>());
      MT_TS_LAUNCH(2, true, MT_F32, MT_F32, MT_BF16);
    } else {
      l = std::max(l, stage_lds_bytes<LD, LH, LH, 1>());
      MT_TS_LAUNCH(1, false, MT_F32, MT_F32, MT_BF16);
    }
  }
#undef MT_TS_LAUNCH16
#undef MT_TS_LAUNCH
}
static int launch_tapsplit(const mt_conv3d_t* p, const ConvChoice& c, hipStream_t st) {
  ConvKParams P;
  if (int rc = conv_fill(P, p, conv_tile(c), 27, FCK)) return rc;
  const dim3 grid = conv_grid(P, 32);
  if (p->SH != 2) launch_tapsplit_t<1, 1>(c, grid, st, P);
  else if (p->SD == 2) launch_tapsplit_t<2, 2>(c, grid, st, P);
  else launch_tapsplit_t<1, 2>(c, grid, st, P);
  MT_CHECK_LAUNCH("conv3d_tapsplit");
  return MT_OK;
}

static int launch_stem(const mt_conv3d_t* p, const ConvChoice& c, hipStream_t st) {
  ConvKParams P;
  if (int rc = conv_fill(P, p, conv_tile(c), 27, FCK)) return rc;
  const dim3 grid = conv_grid(P, 32);
  if (c.os == MT_F16) hipLaunchKernelGGL((conv_stem_kernel<MT_F16>), grid, dim3(256), 0, st, P);
  else if (c.os == MT_BF16) hipLaunchKernelGGL((conv_stem_kernel<MT_BF16>), grid, dim3(256), 0, st, P);
  else hipLaunchKernelGGL((conv_stem_kernel<MT_F32>), grid, dim3(256), 0, st, P);
  MT_CHECK_LAUNCH("conv3d_stem");
  return MT_OK;
}

template <int MW, int RH, int TD, int VEC, int NT, int NW, int KD = 3, int XS = MT_F32, int OS = MT_F32, int MTY = MT_BF16>
static int launch_bf16_t(const mt_conv3d_t* p, const ConvChoice& c, hipStream_t st) {
  ConvKParams P;
  if (int rc = conv_fill(P, p, conv_tile(c), KD * 9, FCK)) return rc;
  constexpr int TH = (32 / MW) * RH, TW = MW;
  const size_t ldsb = bstage_lds_bytes<TD + KD - 1, TH + 2, TW + 2, VEC, NW, (BF_SWZ ? BFP_SWZ : BFP)>();
  dim3 grid((unsigned)(P.nsb * p->N), (unsigned)mt_cdiv(mt_cdiv(p->Cout, 32), NT), 1);
  return conv_launch_lds(conv_bf16_kernel<MW, RH, TD, VEC, NT, NW, KD, XS, OS, MTY>, grid, dim3(64 * NW), ldsb, st, P, "conv3d_bf16");
}
static int launch_bf16(const mt_conv3d_t* p, const ConvChoice& c, hipStream_t st) {
  // NT = 2 (64 output channels per workgroup) measured slower: 0.197 vs 0.179 ms on 64->64 @ 24x96x96; 8 waves: no gain
  MT_REQUIRE(c.xs == conv_src_dtype(p) && c.xs == p->odtype, "conv3d: conv_bf16_kernel takes ONE storage type on all operands (ask mt_conv3d_io_supported)");
#define MT_BF_CASE(MW_, RH_, TD_, NW_)                                                       \
  if (c.g.MW == MW_ && c.g.TD == TD_) {                                                      \
    if (c.xs == MT_F16) return p->KD == 1 ? launch_bf16_t<MW_, RH_, TD_, 4, 1, NW_, 1, MT_F16, MT_F16, MT_F16>(p, c, st) : launch_bf16_t<MW_, RH_, TD_, 4, 1, NW_, 3, MT_F16, MT_F16, MT_F16>(p, c, st); \
    if (c.xs == MT_BF16) return p->KD == 1 ? launch_bf16_t<MW_, RH_, TD_, 4, 1, NW_, 1, MT_BF16, MT_BF16, MT_BF16>(p, c, st) : launch_bf16_t<MW_, RH_, TD_, 4, 1, NW_, 3, MT_BF16, MT_BF16, MT_BF16>(p, c, st); \
    return p->KD == 1 ? launch_bf16_t<MW_, RH_, TD_, 2, 1, NW_, 1>(p, c, st) : launch_bf16_t<MW_, RH_, TD_, 2, 1, NW_>(p, c, st); \
  }
  MT_BF_CASE(32, 4, 4, 4)
  MT_BF_CASE(32, 4, 2, 4)
  MT_BF_CASE(16, 4, 2, 4)
#undef MT_BF_CASE
  mt_set_error("conv3d bf16: bad tile configuration %d x %d x %d", c.g.MW, c.g.RH, c.g.TD);
  return MT_EINVAL;
}

static int launch_x16(const mt_conv3d_t* p, const ConvChoice& c, hipStream_t st) {
  const ConvTile t = conv_tile(c);
  X16Params P;
  P.c = *p;
  if (P.c.nsrc == 1) { P.c.src[1] = P.c.src[0]; P.c.src[1].C = 0; }
  P.tilesD = mt_cdiv(p->Do, t.D); P.tilesH = mt_cdiv(p->Ho, t.H); P.tilesW = mt_cdiv(p->Wo, t.W);
  P.nsb = P.tilesD * P.tilesH * P.tilesW;
  P.ncot = mt_cdiv(p->Cout, 32);
  P.nitems = p->N * P.nsb * P.ncot;
  P.nchunks = mt_build_chunks(p->src[0].C, p->nsrc == 2 ? p->src[1].C : 0, FCK, P.chunk);
  MT_REQUIRE(P.nchunks > 0, "conv3d (x16): too many channel chunks (Cin=%d)", p->Cin);
  P.npairs = 0;
  for (int i = 0; i < P.nchunks; ++P.npairs) {
    const bool two = i + 1 < P.nchunks && P.chunk[i + 1].src == P.chunk[i].src && P.chunk[i + 1].c0 == P.chunk[i].c0 + 16;
    P.pair[P.npairs][0] = (short)i; P.pair[P.npairs][1] = (short)(two ? i + 1 : -1);
    i += two ? 2 : 1;
  }
  P.nwg = mt_conv_x16_workgroups(P.nitems);
  if (p->max_workgroups > 0 && P.nwg > p->max_workgroups) P.nwg = p->max_workgroups;
  return mt_launch_conv_x16(P, p->KD, c.xs, st);
}

static int launch_wino(const mt_conv3d_t* p, const ConvChoice& c, hipStream_t st) {
  MT_REQUIRE(p->bstats.y == nullptr || (c.bstats && p->stats_part != nullptr && p->bstats.mean && p->bstats.rstd &&
                                        p->bstats.c0 >= 0 && p->bstats.C > 0 && p->bstats.c0 + p->bstats.C <= p->Cout),
             "conv3d: bstats set on a problem this kernel does not compute them for (ask mt_conv3d_bwd_stats_supported)");
  ConvKParams P;
  if (int rc = conv_fill(P, p, conv_tile(c), 27, WCK)) return rc;
  const int devid = mt_current_device();
  const size_t l8 = (size_t)(2 * W_RAWF + W_VF) * sizeof(float) + 11 * 256 * 4;          // two raw patches + V + the patch-geometry table
  // one resident workgroup per CU (126 KiB of LDS each): NW workers per output-channel tile walk over the spatial tiles
  const int T = P.nsb * p->N, nct = mt_cdiv(p->Cout, 32);
  int nw = mt_device_cus(devid) / nct; if (nw < 1) nw = 1; if (nw > T) nw = T;
  if (p->max_workgroups > 0 && nw > p->max_workgroups) nw = p->max_workgroups;       // tests: few workers, many tiles each
  const bool b = c.family == CONV_WINO_B;
  static std::atomic<uint64_t> attrb{0}, attrp{0};
  std::atomic<uint64_t>& attr = b ? attrb : attrp;
  if (mt_device_pending(attr, devid)) {
    hipError_t e = hipFuncSetAttribute(b ? (const void*)conv_wino8pb_kernel : (const void*)conv_wino8p_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l8);
    if (e != hipSuccess) { mt_set_error("conv3d: cannot raise dynamic LDS to %zu: %s", l8, hipGetErrorString(e)); return MT_EHIP; }
    mt_mark_device_done(attr, devid);
  }
  if (b) hipLaunchKernelGGL(conv_wino8pb_kernel, dim3((unsigned)nw, (unsigned)nct, 1), dim3(512), l8, st, P);
  else hipLaunchKernelGGL(conv_wino8p_kernel, dim3((unsigned)nw, (unsigned)nct, 1), dim3(512), l8, st, P);
  MT_CHECK_LAUNCH(b ? "conv3d_wino8pb" : "conv3d_wino8p");
  return MT_OK;
}

static int launch_gather(const mt_conv3d_t* p, const ConvChoice& c, hipStream_t st) {
  ConvKParams P;
  if (int rc = conv_fill(P, p, {1, 1, 1}, p->KD * p->KH * p->KW, FCK)) return rc;
  const long V = (long)p->Do * p->Ho * p->Wo;
  P.tilesD = P.tilesH = P.tilesW = 1; P.nsb = (int)((V + 127) / 128);
  dim3 grid = conv_grid(P, 32);
  // (the <2> and <1> instances below are unreachable; they stay until the device code itself is cleaned up)
  if (c.m16 && c.os == MT_BF16) hipLaunchKernelGGL((conv_gather_kernel<4, MT_BF16, MT_BF16, true>), grid, dim3(256), 0, st, P);
  else if (c.m16) hipLaunchKernelGGL((conv_gather_kernel<4, MT_BF16, MT_F32, true>), grid, dim3(256), 0, st, P);
  else if (c.xs == MT_BF16 && c.os == MT_BF16) hipLaunchKernelGGL((conv_gather_kernel<4, MT_BF16, MT_BF16>), grid, dim3(256), 0, st, P);
  else if (c.xs == MT_BF16) hipLaunchKernelGGL((conv_gather_kernel<4, MT_BF16, MT_F32>), grid, dim3(256), 0, st, P);
  else if (c.os == MT_BF16) hipLaunchKernelGGL((conv_gather_kernel<4, MT_F32, MT_BF16>), grid, dim3(256), 0, st, P);
  else if (c.vec == 4 && c.nt2) {
    grid.y = (unsigned)mt_cdiv(mt_cdiv(p->Cout, 32), 2);
    hipLaunchKernelGGL((conv_gather_kernel<4, MT_F32, MT_F32, false, 2>), grid, dim3(256), 0, st, P);
  }
  else if (c.vec == 4) hipLaunchKernelGGL(conv_gather_kernel<4>, grid, dim3(256), 0, st, P);
  else if (c.vec == 2) hipLaunchKernelGGL(conv_gather_kernel<2>, grid, dim3(256), 0, st, P);
  else hipLaunchKernelGGL(conv_gather_kernel<1>, grid, dim3(256), 0, st, P);
  MT_CHECK_LAUNCH("conv3d_gather");
  return MT_OK;
}

static int launch_rt(const mt_conv3d_t* p, const ConvChoice& c, hipStream_t st) {
  ConvKParams P;
  if (int rc = conv_fill(P, p, conv_tile(c), p->KD * p->KH * p->KW, FCK)) return rc;
  const size_t ldsb = rt_lds(c.g, p);
#define MT_RT_CASE(MW_, RH_, TD_)                                                                                              \
  if (c.g.MW == MW_) return c.vec == 2 ? conv_launch_lds(conv_rt_kernel<MW_, RH_, TD_, 2>, conv_grid(P, 32), dim3(256), ldsb, st, P, "conv3d_rt") \
                                       : conv_launch_lds(conv_rt_kernel<MW_, RH_, TD_, 1>, conv_grid(P, 32), dim3(256), ldsb, st, P, "conv3d_rt");
  MT_RT_CASE(32, 4, 2)
  MT_RT_CASE(16, 2, 2)
  MT_RT_CASE(8, 2, 2)
#undef MT_RT_CASE
  return MT_EINVAL;
}

static int launch_generic(const mt_conv3d_t* p, const ConvChoice& c, hipStream_t st) {
  ConvKParams P;
  if (int rc = conv_fill(P, p, conv_tile(c), p->KD * p->KH * p->KW, c.g.CK)) return rc;
  const size_t ldsb = cfg_lds(c.g, p);
#define MT_G_INST(MW_, RH_, TD_, CK_, FAST_) conv_launch_lds(conv_fwd_kernel<MW_, RH_, TD_, CK_, FAST_>, conv_grid(P, 32), dim3(256), ldsb, st, P, "conv3d_fwd")
#define MT_G_IS(MW_, TD_, CK_) (c.g.MW == MW_ && c.g.TD == TD_ && c.g.CK == CK_)
#define MT_G_CASE(MW_, RH_, TD_, CK_) if (MT_G_IS(MW_, TD_, CK_)) return c.fast ? MT_G_INST(MW_, RH_, TD_, CK_, true) : MT_G_INST(MW_, RH_, TD_, CK_, false);
  MT_G_CASE(32, 4, 2, 16)
  MT_G_CASE(16, 2, 2, 16)
  MT_G_CASE(8, 2, 2, 16)
  MT_G_CASE(32, 4, 2, 8)
  if (MT_G_IS(16, 2, 8)) return MT_G_INST(16, 2, 2, 8, false);
  if (MT_G_IS(8, 2, 8)) return MT_G_INST(8, 2, 2, 8, false);
  MT_G_CASE(32, 4, 4, 16)
#undef MT_G_CASE
#undef MT_G_IS
#undef MT_G_INST
  return MT_EINVAL;
}

extern "C" int mt_conv3d_fwd(const mt_conv3d_t* p, mt_stream_t stream) {
  int rc = conv_validate(p);
  if (rc != MT_OK) return rc;
  const ConvChoice c = conv_resolve(p);
  MT_REQUIRE(c.family != CONV_NONE, "conv3d: no tile configuration fits LDS");
  MT_REQUIRE(conv_io_served(p, c), "conv3d: storage types (src %d/%d, out %d) not taken by the kernel that serves this problem "
             "(ask mt_conv3d_io_supported, convert with mt_cast)", p->src[0].dtype, p->nsrc == 2 ? p->src[1].dtype : -1, p->odtype);
  MT_REQUIRE(p->bstats.y == nullptr || c.family == CONV_WINO_B, "conv3d: bstats set on a problem whose kernel does not compute them "
             "(ask mt_conv3d_bwd_stats_supported)");
  MT_REQUIRE(p->osD <= 0 || c.family == CONV_RT, "conv3d: strided output placement needs the runtime-geometry kernel");
  MT_REQUIRE(p->osD <= 0 || (p->stats_part == nullptr && p->osH > 0 && p->osW > 0 &&
             (p->Do - 1) * p->osD + p->ooD < p->OD && (p->Ho - 1) * p->osH + p->ooH < p->OH && (p->Wo - 1) * p->osW + p->ooW < p->OW),
             "conv3d: bad strided output placement");
  hipStream_t st = (hipStream_t)stream;
  switch (c.family) {
    case CONV_STEM: return launch_stem(p, c, st);
    case CONV_WINO: case CONV_WINO_B: return launch_wino(p, c, st);
    case CONV_FAST: return launch_fast(p, c, st);
    case CONV_TAPSPLIT: return launch_tapsplit(p, c, st);
    case CONV_FAST_STRIDED: return p->SD == 2 ? launch_fast_strided_t<2>(p, c, st) : launch_fast_strided_t<1>(p, c, st);
    case CONV_BF16: return launch_bf16(p, c, st);
    case CONV_X16: return launch_x16(p, c, st);
    case CONV_GATHER: return launch_gather(p, c, st);
    case CONV_RT: return launch_rt(p, c, st);
    default: return launch_generic(p, c, st);
  }
}


// ------------------------------------------------------------------------------------------------
// mt_conv3d_bwd_data_strided: see include/mtseg.h.  p carries the FORWARD geometry (Di.. = X dims, Do.. = Y dims, K = 3,
// S in {(2,2,2), (1,2,2)}, P = 1); src[0] = dY (C = Cout of the conv), out0 = dX (Cin channels).
// The one decision: conv_bwdd_strided_ks_kernel (fp32 on both sides, 8-byte channel pairs, fewer workgroups than CUs in the 2 x 4 x 16
// tiling; MT_SEL_TAPSPLIT OFF: never, FORCE: wherever the types fit), else conv_bwdd_strided_kernel with 16-bit matrix inputs and the
// storage pair (dY, dX), or in fp32 with staging width 2 (channel pairs) or 1.
struct BwddChoice { bool ks, m16; int vec, xs, os; };
static BwddChoice bwdd_resolve(const mt_conv3d_t* p) {
  const mt_src_t& s0 = p->src[0];
  const bool pairs = !((s0.cs & 1) || (s0.C & 1));
  BwddChoice c = {};
  c.m16 = mt_sel3(p, MT_SEL_M16) && p->mma == 1 && p->Cout >= 16 && pairs && !(((uintptr_t)s0.ptr) & (mt_is16(s0.dtype) ? 3 : 7));
  c.vec = (pairs && !(((uintptr_t)s0.ptr) & 7)) ? 2 : 1;
  if (c.m16) {
    const bool yb = s0.dtype == MT_BF16 && p->odtype == MT_BF16;        // dY and dX bf16; else dY read as fp32, dX bf16 or fp32
    c.vec = yb ? 4 : 2; c.xs = yb ? MT_BF16 : MT_F32; c.os = p->odtype == MT_BF16 ? MT_BF16 : MT_F32;
    return c;
  }
  const int g_tapsplit = mt_sel3(p, MT_SEL_TAPSPLIT);
  if (g_tapsplit && s0.dtype == MT_F32 && p->odtype == MT_F32 && c.vec == 2) {
    const long wgs = (long)p->N * mt_cdiv(mt_cdiv(p->Di, p->SD), 2) * mt_cdiv(mt_cdiv(p->Hi, 2), 4) * mt_cdiv(mt_cdiv(p->Wi, 2), 16) * mt_cdiv(p->Cin, 32);
    c.ks = wgs < 256 || g_tapsplit >= 2;
  }
  return c;
}
extern "C" int mt_conv3d_bwd_data_strided_pack_layout(const mt_conv3d_t* p) { return (p != nullptr && bwdd_resolve(p).m16) ? 3 : 1; }
static int bwdd_io_served(const mt_conv3d_t* p, const BwddChoice& c) {
  if (!mt_dtype_ok(p->src[0].dtype) || !mt_dtype_ok(p->odtype)) return 0;
  if (p->src[0].dtype == MT_F32 && p->odtype == MT_F32) return 1;
  if (!c.m16 || p->src[0].dtype == MT_F16) return 0;        // gradients are fp32 or bf16
  // dX bf16 (channel-pair dwords: even Cin / stride, dword-aligned base) from dY bf16 or fp32
  return (p->odtype == MT_BF16 && !(p->Cin & 1) && !(p->ocs0 & 1) && !(((uintptr_t)p->out0) & 3)) ? 1 : 0;
}
extern "C" int mt_conv3d_bwd_data_strided_io_supported(const mt_conv3d_t* p) { return p == nullptr ? 0 : bwdd_io_served(p, bwdd_resolve(p)); }
template <int SD, int SH, int SW>
static int launch_bwdd_strided(const mt_conv3d_t* p, hipStream_t st) {
  constexpr int TD = 2, TH = 4, TW = 16;
  constexpr int LD = TD + (SD == 2 ? 1 : 2), LH = TH + (SH == 2 ? 1 : 2), LW = TW + (SW == 2 ? 1 : 2);
  const BwddChoice c = bwdd_resolve(p);
  MT_REQUIRE(bwdd_io_served(p, c), "bwd_data_strided: storage types not taken by the kernel that serves this problem (ask mt_conv3d_bwd_data_strided_io_supported)");
  const ConvTile t = c.ks ? ConvTile{TD, 4, 4} : ConvTile{TD, TH, TW};   // ks: one 2 x 4 x 4 tile per workgroup, the chunk's K split over the waves
  ConvKParams P;
  if (int rc = conv_fill(P, p, t, 27, FCK)) return rc;
  // the kernel sees a stride-1 problem over the dY grid: input = dY (dims Do,Ho,Wo), channels Cout -> Cin
  P.c.Di = p->Do; P.c.Hi = p->Ho; P.c.Wi = p->Wo;
  P.c.OD = p->Di; P.c.OH = p->Hi; P.c.OW = p->Wi;
  P.c.Cin = p->Cout; P.c.Cout = p->Cin;
  // the tiles cover the dY positions that reach some dX
  P.tilesD = mt_cdiv(mt_cdiv(p->Di, SD), t.D); P.tilesH = mt_cdiv(mt_cdiv(p->Hi, SH), t.H); P.tilesW = mt_cdiv(mt_cdiv(p->Wi, SW), t.W);
  P.nsb = P.tilesD * P.tilesH * P.tilesW;
  const dim3 grid = conv_grid(P, 32);
  if (c.ks) {
    constexpr int KLD = 2 + (SD == 2 ? 1 : 2), KLH = 4 + 1, KLW = 4 + 1;
    size_t l = stage_lds_bytes<KLD, KLH, KLW, 2>(); if (l < (size_t)4 * 16 * 64 * sizeof(float)) l = (size_t)4 * 16 * 64 * sizeof(float);
    hipLaunchKernelGGL((conv_bwdd_strided_ks_kernel<SD, SH, SW>), grid, dim3(256), l, st, P);
    MT_CHECK_LAUNCH("conv_bwdd_strided_ks");
    return MT_OK;
  }
  if (c.m16 && c.vec == 4) hipLaunchKernelGGL((conv_bwdd_strided_kernel<SD, SH, SW, 4, true, MT_BF16, MT_BF16>), grid, dim3(256), (bstage_lds_bytes<LD, LH, LW, 4, 4>()), st, P);
  else if (c.m16 && c.os == MT_BF16) hipLaunchKernelGGL((conv_bwdd_strided_kernel<SD, SH, SW, 2, true, MT_F32, MT_BF16>), grid, dim3(256), (bstage_lds_bytes<LD, LH, LW, 2, 4>()), st, P);
  else if (c.m16) hipLaunchKernelGGL((conv_bwdd_strided_kernel<SD, SH, SW, 2, true>), grid, dim3(256), (bstage_lds_bytes<LD, LH, LW, 2, 4>()), st, P);
  else if (c.vec == 2) hipLaunchKernelGGL((conv_bwdd_strided_kernel<SD, SH, SW, 2>), grid, dim3(256), (stage_lds_bytes<LD, LH, LW, 2>()), st, P);
  else hipLaunchKernelGGL((conv_bwdd_strided_kernel<SD, SH, SW, 1>), grid, dim3(256), (stage_lds_bytes<LD, LH, LW, 1>()), st, P);
  MT_CHECK_LAUNCH("conv_bwdd_strided");
  return MT_OK;
}
extern "C" int mt_conv3d_bwd_data_strided_supported(const mt_conv3d_t* p) {
  if (p == nullptr || p->nsrc != 1) return 0;
  if (p->src[0].scale != nullptr && !(p->src[0].slope >= 0.f && p->src[0].slope <= 1.f)) return 0;
  if (!(p->KD == 3 && p->KH == 3 && p->KW == 3 && p->PD == 1 && p->PH == 1 && p->PW == 1)) return 0;
  if (!(p->dilD == 1 && p->dilH == 1 && p->dilW == 1)) return 0;
  if (!(p->SH == 2 && p->SW == 2 && (p->SD == 1 || p->SD == 2))) return 0;
  if ((double)p->Do * p->Ho * p->Wo * p->src[0].cs * 4.0 >= 2147483648.0) return 0;
  if ((double)p->Di * p->Hi * p->Wi * p->ocs0 * 4.0 >= 2147483648.0) return 0;
  return 1;
}
extern "C" int mt_conv3d_bwd_data_strided_kernel_name(const mt_conv3d_t* p, char* buf, size_t n) {
  if (p == nullptr || buf == nullptr || n == 0 || !mt_conv3d_bwd_data_strided_supported(p)) return MT_EINVAL;
  const BwddChoice c = bwdd_resolve(p);
  if (c.ks) snprintf(buf, n, "conv_bwdd_strided_ks_kernel<%d, 2, 2>", p->SD);
  else snprintf(buf, n, "conv_bwdd_strided_kernel<%d, 2, 2, %d, %s, %d, %d>", p->SD, c.vec, c.m16 ? "true" : "false", c.xs, c.os);
  return MT_OK;
}
extern "C" int mt_conv3d_bwd_data_strided(const mt_conv3d_t* p, mt_stream_t stream) {
  MT_REQUIRE(p != nullptr, "bwd_data_strided: null params");
  MT_REQUIRE(mt_conv3d_bwd_data_strided_supported(p), "bwd_data_strided: unsupported geometry (needs 3x3x3, pad 1, stride (1|2,2,2), one source)");
  MT_REQUIRE(p->src[0].C == p->Cout, "bwd_data_strided: src[0].C (%d) != Cout (%d)", p->src[0].C, p->Cout);
  MT_REQUIRE(p->wpack != nullptr && p->out0 != nullptr && p->src[0].ptr != nullptr, "bwd_data_strided: null pointers");
  hipStream_t st = (hipStream_t)stream;
  return p->SD == 2 ? launch_bwdd_strided<2, 2, 2>(p, st) : launch_bwdd_strided<1, 2, 2>(p, st);
}

// ------------------------------------------------------------------------------------------------
// Weight packing into B-fragment order [ntile][chunk][tap][ck/2][64]:
//   lane l holds W_eff[tap][ci = chunk.cglob + 2*kp + (l>>5)][co = ntile*32 + (l&31)]
struct PackParams {
  const float* w; float* dst;
  int Cout, KD, KH, KW, nkp, nchunks, ntiles, flip, layout;
  int has_tm, tb[3], ts[3];
  int contig;          // the K3 taps of a (cin, cout) pair and the cin of a cout are contiguous (torch Conv3d weight): LDS-transposed path
  long s_ci, s_co, s_kd, s_kh, s_kw;
  ConvChunk chunk[MT_MAX_CHUNKS];
};
#define PACK_TP (16 * 27 + 1)       // floats per cout row of the LDS tile
#define PACK_LDS_BYTES (32 * PACK_TP * 4)
// Layouts 1 / 3 / 4 over a contiguous torch weight: a workgroup takes one (cout tile, chunk) block — 32 rows of ck * K3 CONTIGUOUS floats,
// read as linear runs into an LDS tile — and writes the block's K3 x per_tap packed dwords as linear runs.  (The per-item form below
// reads 108-byte runs at 64 different addresses per instruction: texture-path bound, 255 us for 124 MB of weights.)
__device__ __forceinline__ void pack_weights_tiled(const PackParams& P, float* __restrict__ tile, int blk, int nblk) {
  const int K3 = P.KD * P.KH * P.KW;
  const int nq = P.layout == 1 ? P.nkp / 4 : 1;
  const int per_tap = nq * 256;
  const int tid = threadIdx.x;
  for (int g = blk; g < P.ntiles * P.nchunks; g += nblk) {
    const int nt = g / P.nchunks, ch = g - nt * P.nchunks;
    const ConvChunk cc = P.chunk[ch];
    const int rowlen = cc.ck * K3;
    __syncthreads();                         // the previous block's reads of the tile are done
    {   // all 64 loads of a thread (32 rows x 2 pieces of <= 432 floats) are requested before the first LDS store: one round trip per block
      float v0[32], v1[32];
      const float* src0 = P.w + (long)(nt * 32) * P.s_co + (long)cc.cglob * K3;
      const int nrow = P.Cout - nt * 32;              // valid rows of this cout tile
#pragma unroll
      for (int co = 0; co < 32; ++co) {
        const float* src = src0 + (long)co * P.s_co;
        v0[co] = (co < nrow && tid < rowlen) ? src[tid] : 0.f;
        v1[co] = (co < nrow && tid + 256 < rowlen) ? src[tid + 256] : 0.f;
      }
#pragma unroll
      for (int co = 0; co < 32; ++co) {
        if (tid < rowlen) tile[co * PACK_TP + tid] = v0[co];
        if (tid + 256 < rowlen) tile[co * PACK_TP + tid + 256] = v1[co];
      }
    }
    __syncthreads();
    float* dst = P.dst + (size_t)g * K3 * per_tap;
    for (int i = tid; i < per_tap; i += 256) {
      const int e = i & 3, l = (i >> 2) & 63, qq = i >> 8;
      const int co = l & 31;
      const int c0 = P.layout == 1 ? (l >> 5) * P.nkp + qq * 4 + e : (l >> 5) * 8 + 2 * e;
      const bool v0 = c0 < cc.ck, v1 = P.layout >= 3 && (c0 + 1) < cc.ck;
      const float* tp = tile + co * PACK_TP + c0 * K3;
      for (int tap = 0; tap < K3; ++tap) {
        const int zt = P.flip ? K3 - 1 - tap : tap;
        const float a0 = v0 ? tp[zt] : 0.f;
        if (P.layout == 1) dst[(size_t)tap * per_tap + i] = a0;
        else {
          const float a1 = v1 ? tp[K3 + zt] : 0.f;
          ((unsigned*)dst)[(size_t)tap * per_tap + i] = P.layout == 3 ? mt_pk16<MT_BF16>(a0, a1) : mt_pk16<MT_F16>(a0, a1);
        }
      }
    }
  }
}
__device__ __forceinline__ void pack_weights_body(const PackParams& P, long first, long stride) {
  if (P.layout == 2) {     // Winograd F(2x2x2, 3x3x3): U = G g G^T (3D) in B-fragment order [ntile][chunk of 8][xi 64][lane][4]
    // one work item per (cin, cout) pair: the 27 weights are read once and transformed separably into the 64 xi values
    const long total = (long)P.ntiles * P.nchunks * 256;
    for (long i = first; i < total; i += stride) {
      long r = i;
      const int e = (int)(r % 4); r /= 4;
      const int l = (int)(r % 64); r /= 64;
      const int ch = (int)(r % P.nchunks); r /= P.nchunks;
      const int nt = (int)r;
      const ConvChunk cc = P.chunk[ch];
      const int cin_local = 4 * (l >> 5) + e, co = nt * 32 + (l & 31);
      float u[4][4][4];
      if (cin_local < cc.ck && co < P.Cout) {
        const float* wp = P.w + (cc.cglob + cin_local) * P.s_ci + co * P.s_co;
        float g[3][3][3];
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
          for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
              const int zd = P.flip ? 2 - kd : kd, zh = P.flip ? 2 - kh : kh, zw = P.flip ? 2 - kw : kw;
              g[kd][kh][kw] = wp[zd * P.s_kd + zh * P.s_kh + zw * P.s_kw];
            }
        float t1[3][3][4], t2[3][4][4];
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
          for (int kh = 0; kh < 3; ++kh) {
            const float g0 = g[kd][kh][0], g1 = g[kd][kh][1], g2 = g[kd][kh][2];
            t1[kd][kh][0] = g0; t1[kd][kh][1] = 0.5f * (g0 + g1 + g2); t1[kd][kh][2] = 0.5f * (g0 - g1 + g2); t1[kd][kh][3] = g2;
          }
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float g0 = t1[kd][0][k], g1 = t1[kd][1][k], g2 = t1[kd][2][k];
            t2[kd][0][k] = g0; t2[kd][1][k] = 0.5f * (g0 + g1 + g2); t2[kd][2][k] = 0.5f * (g0 - g1 + g2); t2[kd][3][k] = g2;
          }
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float g0 = t2[0][b][k], g1 = t2[1][b][k], g2 = t2[2][b][k];
            u[0][b][k] = g0; u[1][b][k] = 0.5f * (g0 + g1 + g2); u[2][b][k] = 0.5f * (g0 - g1 + g2); u[3][b][k] = g2;
          }
      } else {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int k = 0; k < 4; ++k) u[a][b][k] = 0.f;
      }
      float* dp = P.dst + ((size_t)(nt * P.nchunks + ch) * 64) * 256 + l * 4 + e;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int k = 0; k < 4; ++k) dp[((a * 4 + b) * 4 + k) * 256] = u[a][b][k];
    }
    return;
  }
  if (P.layout == 1 || P.layout == 3 || P.layout == 4) {
    // One work item per (lane slot, channel group) of a fragment, looping over the taps: the K taps of a (cin, cout) pair are
    // contiguous in the torch weight (one 108-byte run, read once), and for a fixed tap consecutive work items write consecutive
    // dwords.  (The previous one-item-per-element mapping fetched 837 MB for 117 MB of weights: profiles/r01_pmc_per_kernel.json.)
    //   layout 1: [ntile][chunk][tap][kp/4][lane][4]: lane half h owns channels h*nkp .. h*nkp+nkp-1, float4 = 4 consecutive
    //   layout 3: [ntile][chunk][tap][lane][4 dwords]: lane half h owns channels 8h .. 8h+7 as bf16 pairs (RNE); layout 4: as fp16 pairs
    const int K3 = P.KD * P.KH * P.KW;
    const int nq = P.layout == 1 ? P.nkp / 4 : 1;
    const int per_tap = nq * 256;
    const long items = (long)P.ntiles * P.nchunks * per_tap;
    for (long i = first; i < items; i += stride) {
      long r = i;
      const int e = (int)(r % 4); r /= 4;
      const int l = (int)(r % 64); r /= 64;
      const int q = (int)(r % nq); r /= nq;
      const int ch = (int)(r % P.nchunks); r /= P.nchunks;
      const int nt = (int)r;
      const ConvChunk cc = P.chunk[ch];
      const int co = nt * 32 + (l & 31);
      const int c0 = P.layout == 1 ? (l >> 5) * P.nkp + q * 4 + e : (l >> 5) * 8 + 2 * e;
      const bool v0 = c0 < cc.ck && co < P.Cout, v1 = P.layout >= 3 && (c0 + 1) < cc.ck && co < P.Cout;
      const float* w0 = P.w + (long)(cc.cglob + c0) * P.s_ci + (long)co * P.s_co;
      float* dp = P.dst + ((size_t)(nt * P.nchunks + ch) * K3) * per_tap + (q * 64 + l) * 4 + e;
      // all taps of the item's (cin, cout) pair(s) are requested BEFORE the first store (the compiler may not move a load over a
      // store to dst): the 108-byte run of a pair is one or two cache lines, and 27 dependent round trips through a thrashing L2
      // fetched 2.4 GB for 124 MB of weights (profiles/r04_pmc_per_kernel.json)
      if (K3 <= 27) {
        float a0[27], a1[27];
#pragma unroll
        for (int tap = 0; tap < 27; ++tap) {
          a0[tap] = 0.f; a1[tap] = 0.f;
          if (tap < K3) {
            const int kw = tap % P.KW, kh = (tap / P.KW) % P.KH, kd = tap / (P.KW * P.KH);
            int zd = P.flip ? P.KD - 1 - kd : kd, zh = P.flip ? P.KH - 1 - kh : kh, zw = P.flip ? P.KW - 1 - kw : kw;
            if (P.has_tm) { zd = P.tb[0] + P.ts[0] * kd; zh = P.tb[1] + P.ts[1] * kh; zw = P.tb[2] + P.ts[2] * kw; }
            const long o = zd * P.s_kd + zh * P.s_kh + zw * P.s_kw;
            if (v0) a0[tap] = w0[o];
            if (v1) a1[tap] = w0[o + P.s_ci];
          }
        }
#pragma unroll
        for (int tap = 0; tap < 27; ++tap)
          if (tap < K3) {
            if (P.layout == 1) dp[(size_t)tap * per_tap] = a0[tap];
            else if (P.layout == 3) ((unsigned*)dp)[(size_t)tap * per_tap] = mt_pk16<MT_BF16>(a0[tap], a1[tap]);
            else ((unsigned*)dp)[(size_t)tap * per_tap] = mt_pk16<MT_F16>(a0[tap], a1[tap]);
          }
        continue;
      }
      int tap = 0;
      for (int kd = 0; kd < P.KD; ++kd)
        for (int kh = 0; kh < P.KH; ++kh)
          for (int kw = 0; kw < P.KW; ++kw, ++tap) {
            int zd = P.flip ? P.KD - 1 - kd : kd, zh = P.flip ? P.KH - 1 - kh : kh, zw = P.flip ? P.KW - 1 - kw : kw;
            if (P.has_tm) { zd = P.tb[0] + P.ts[0] * kd; zh = P.tb[1] + P.ts[1] * kh; zw = P.tb[2] + P.ts[2] * kw; }
            const long o = zd * P.s_kd + zh * P.s_kh + zw * P.s_kw;
            const float a0 = v0 ? w0[o] : 0.f;
            if (P.layout == 1) dp[(size_t)tap * per_tap] = a0;
            else if (P.layout == 3) ((unsigned*)dp)[(size_t)tap * per_tap] = mt_pk16<MT_BF16>(a0, v1 ? w0[o + P.s_ci] : 0.f);
            else ((unsigned*)dp)[(size_t)tap * per_tap] = mt_pk16<MT_F16>(a0, v1 ? w0[o + P.s_ci] : 0.f);
          }
    }
    return;
  }
  const long total = (long)P.ntiles * P.nchunks * P.KD * P.KH * P.KW * P.nkp * 64;
  for (long i = first; i < total; i += stride) {
    long r = i;
    int l, kp;
    if (P.layout == 1) {      // [.. tap][kp/4][lane][4]: one float4 per lane carries 4 consecutive channel pairs
      const int e = (int)(r % 4); r /= 4;
      l = (int)(r % 64); r /= 64;
      const int q = (int)(r % (P.nkp / 4)); r /= (P.nkp / 4);
      kp = q * 4 + e;
    } else {                  // [.. tap][kp][lane]
      l = (int)(r % 64); r /= 64;
      kp = (int)(r % P.nkp); r /= P.nkp;
    }
    const int kw = (int)(r % P.KW); r /= P.KW;
    const int kh = (int)(r % P.KH); r /= P.KH;
    const int kd = (int)(r % P.KD); r /= P.KD;
    const int ch = (int)(r % P.nchunks); r /= P.nchunks;
    const int nt = (int)r;
    const ConvChunk cc = P.chunk[ch];
    // layout 0: MFMA step kp contracts channels (2kp, 2kp+1); layout 1: channels (kp, nkp + kp) — each lane half
    // then owns nkp CONTIGUOUS channels of a voxel, which the conv kernels fetch with two ds_read_b128
    const int cin_local = (P.layout == 1) ? (l >> 5) * P.nkp + kp : 2 * kp + (l >> 5);
    const int co = nt * 32 + (l & 31);
    float v = 0.f;
    if (cin_local < cc.ck && co < P.Cout) {
      const int ci = cc.cglob + cin_local;
      int zd = P.flip ? P.KD - 1 - kd : kd, zh = P.flip ? P.KH - 1 - kh : kh, zw = P.flip ? P.KW - 1 - kw : kw;
      if (P.has_tm) { zd = P.tb[0] + P.ts[0] * kd; zh = P.tb[1] + P.ts[1] * kh; zw = P.tb[2] + P.ts[2] * kw; }
      v = P.w[ci * P.s_ci + co * P.s_co + zd * P.s_kd + zh * P.s_kh + zw * P.s_kw];
    }
    P.dst[i] = v;
  }
}
__global__ void pack_weights_kernel(const PackParams P) {
  pack_weights_body(P, (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
}
// every layer's packing of one optimizer step in ONE launch: blockIdx.y selects the descriptor (table in device memory)
__global__ __launch_bounds__(256) void pack_weights_batched_kernel(const PackParams* __restrict__ tab) {
  extern __shared__ __attribute__((aligned(16))) float pack_tile[];
  const PackParams& P = tab[blockIdx.y];
  if (P.contig && (P.layout == 1 || P.layout >= 3)) { pack_weights_tiled(P, pack_tile, (int)blockIdx.x, (int)gridDim.x); return; }   // block-uniform
  pack_weights_body(P, (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
}

static int pack_fill(PackParams& P, size_t* packed_floats, const float* w, float* dst, int C0, int C1, int Cout, int KD, int KH,
                     int KW, long s_ci, long s_co, long s_kd, long s_kh, long s_kw, int flip, int ck, int layout,
                     const int32_t* tapmap) {
  MT_REQUIRE(ck >= 2 && (ck % 2) == 0, "pack: ck must be even (got %d)", ck);
  MT_REQUIRE(layout == 0 || (layout == 1 && (ck % 8) == 0) || (layout == 2 && ck == 8 && KD == 3 && KH == 3 && KW == 3 && tapmap == nullptr) ||
             ((layout == 3 || layout == 4) && ck == 16),
             "pack: layout 1 needs ck %% 8 == 0; layout 2 (Winograd) needs ck == 8 and a 3x3x3 kernel; layouts 3 / 4 (bf16 / fp16) need ck == 16");
  std::memset((void*)&P, 0, sizeof(P));
  P.nchunks = mt_build_chunks(C0, C1, ck, P.chunk);
  MT_REQUIRE(P.nchunks > 0, "pack: too many chunks");
  P.ntiles = mt_cdiv(Cout, 32);
  P.nkp = ck / 2;
  if (packed_floats) *packed_floats = layout == 2 ? (size_t)P.ntiles * P.nchunks * 64 * 256
                                    : layout >= 3 ? (size_t)P.ntiles * P.nchunks * KD * KH * KW * 256
                                                  : (size_t)P.ntiles * P.nchunks * KD * KH * KW * P.nkp * 64;
  P.w = w; P.dst = dst; P.Cout = Cout; P.KD = KD; P.KH = KH; P.KW = KW; P.flip = flip; P.layout = layout;
  P.has_tm = tapmap != nullptr;
  for (int d = 0; d < 3; ++d) { P.tb[d] = tapmap ? tapmap[2 * d] : 0; P.ts[d] = tapmap ? tapmap[2 * d + 1] : 1; }
  P.s_ci = s_ci; P.s_co = s_co; P.s_kd = s_kd; P.s_kh = s_kh; P.s_kw = s_kw;
  P.contig = (tapmap == nullptr && ck <= 16 && KD * KH * KW <= 27 && s_kw == 1 && s_kh == KW && s_kd == (long)KH * KW && s_ci == (long)KD * KH * KW) ? 1 : 0;
  return MT_OK;
}
extern "C" size_t mt_pack_desc_size(void) { return sizeof(PackParams); }
extern "C" int mt_pack_desc_fill(void* desc, const float* w, float* dst, int C0, int C1, int Cout, int KD, int KH, int KW,
                                 long s_ci, long s_co, long s_kd, long s_kh, long s_kw, int flip, int ck, int layout,
                                 const int32_t* tapmap) {
  MT_REQUIRE(desc != nullptr && w != nullptr && dst != nullptr, "pack_desc_fill: null pointers");
  return pack_fill(*(PackParams*)desc, nullptr, w, dst, C0, C1, Cout, KD, KH, KW, s_ci, s_co, s_kd, s_kh, s_kw, flip, ck, layout, tapmap);
}
// workgroups per descriptor of the batched packing: the launch lasts as long as its LARGEST descriptor (a 320 x 320 x 27 layer is 2.8 M
// scattered 4-byte reads), so that one needs the whole chip; the small descriptors' surplus workgroups exit at once
static unsigned g_pack_blocks() {
  constexpr int v = 1024;
  return (unsigned)v;
}
extern "C" int mt_pack_batched(const void* descs_device, int n, mt_stream_t stream) {
  MT_REQUIRE(descs_device != nullptr && n > 0, "pack_batched: empty table");
  hipLaunchKernelGGL(pack_weights_batched_kernel, dim3(g_pack_blocks(), (unsigned)n, 1), dim3(256), PACK_LDS_BYTES, (hipStream_t)stream,
                     (const PackParams*)descs_device);
  MT_CHECK_LAUNCH("pack_weights_batched");
  return MT_OK;
}

extern "C" int mt_pack_conv_weights(const float* w, float* dst, size_t* packed_floats, int C0, int C1, int Cout,
                                    int KD, int KH, int KW, long s_ci, long s_co, long s_kd, long s_kh, long s_kw,
                                    int flip, int ck, int layout, const int32_t* tapmap, mt_stream_t stream) {
  PackParams P;
  size_t total = 0;
  int rc = pack_fill(P, &total, w, dst, C0, C1, Cout, KD, KH, KW, s_ci, s_co, s_kd, s_kh, s_kw, flip, ck, layout, tapmap);
  if (rc != MT_OK) return rc;
  if (packed_floats) *packed_floats = total;
  if (dst == nullptr) return MT_OK;
  MT_REQUIRE(w != nullptr, "pack: null weights");
  int blocks = mt_cdiv((long)total, 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P);
  MT_CHECK_LAUNCH("pack_weights");
  return MT_OK;
}
