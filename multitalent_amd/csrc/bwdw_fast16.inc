// bwdw_fast16.inc — backward-weight of the tiled geometries (strided 3x3x3 stage convs, 2x2x2 / 1x2x2 transposed-conv weights, 1x1x1
// projections, 1x3x3) in mixed precision: 16-bit X and dY in HBM, bf16 products, fp32 accumulation (VERDICT r3 item 7 for the
// mixed mode).  conv_bwdw_fast_kernel, which served these launches, multiplies in fp32: 8 k-steps of 4 voxels x 27 taps x 2 cout halves
// = 432 v_mfma_f32_16x16x4_f32 per wave and tile, fully serialised with a staging pass of 63 four-byte gathers per thread (round-2
// ablation: 0.45 + 0.45 ms of 0.84).  Same decomposition here — tile of 128 voxels, K (= voxels) split over the four waves, every wave
// holds all taps' 16 ci x 32 co accumulators, one partial per workgroup, bwdw_reduce_kernel sums them — with
//   * ONE v_mfma_f32_16x16x32_bf16 per (tap, cout half): the wave's 32 voxels are the K of one instruction.  K index 8*lk + j of lane
//     group lk is voxel (k-step j, position lk) — the SAME (lane, step) -> voxel map as the fp32 kernel, so dY arrives with the same
//     loads and the X fragment is the same LDS gather, eight 2-byte reads instead of eight dwords;
//   * a bf16 LDS image [voxel][12 dwords] (16 channels + pad: the four k-groups of a gather land on disjoint banks for SW = 1 and 2),
//     activation (fp32) + ONE rounding to bf16 in the staging pass;
//   * 8-byte staging loads (4 channels per lane): 35 instead of 63 gathers per thread and tile for the 3 x 9 x 65 halo.
#define BW16_P 12      // dwords per voxel of the LDS image

template <int LD, int LH, int LW>
struct Bw16Regs {
  static constexpr int VPS = 16, NI = (LW + VPS - 1) / VPS, R = LD * LH, RPW = (R + 3) / 4;
  uint2 v[RPW][NI];    // raw 8-byte groups (4 channels of one voxel)
  int voff[NI];
  unsigned rvmask;     // bit r: row r of this wave is inside the volume
  int nb;
};
template <int LD, int LH, int LW>
__host__ __device__ constexpr size_t bw16_lds_bytes() { return (size_t)LD * LH * LW * BW16_P * 4; }

template <int LD, int LH, int LW, int XS>
__device__ __forceinline__ void bw16_load(Bw16Regs<LD, LH, LW>& g, const mt_conv3d_t& c, const ConvChunk ch, int nb,
                                          int ud0, int uh0, int uw0, int lane, int wave) {
  typedef Bw16Regs<LD, LH, LW> RG_;
  constexpr int VPS = RG_::VPS, NI = RG_::NI, R = RG_::R, RPW = RG_::RPW;
  const mt_src_t& S = c.src[ch.src];
  const int cl = (lane & 3) * 4, vl = lane >> 2;
  const int cs = S.cs;
  const size_t sample_elems = (size_t)c.Di * c.Hi * c.Wi * cs;
  __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)S.ptr + (size_t)nb * sample_elems * 2), 0, (int)(sample_elems * 2), 0x00020000);
  g.nb = nb;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int lw = vl + i * VPS;
    const int uw = uw0 + lw;
    const bool ok = (cl < ch.ck) && (lw < LW) && ((unsigned)uw < (unsigned)c.Wi);
    g.voff[i] = ok ? (uw * cs + ch.c0 + cl) * 2 : (int)0x80000000;
  }
  g.rvmask = 0;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int row = wave + 4 * r;
    const int ld = row / LH, lhh = row % LH;
    const int ud = ud0 + ld, uh = uh0 + lhh;
    const bool rv = (row < R) && ((unsigned)ud < (unsigned)c.Di) && ((unsigned)uh < (unsigned)c.Hi);     // wave-uniform
    const int srow = rv ? (ud * c.Hi + uh) * c.Wi * cs * 2 : 0;
    const int oob = rv ? 0 : (int)0x80000000;
    g.rvmask |= (rv ? 1u : 0u) << r;
#pragma unroll
    for (int i = 0; i < NI; ++i)
      g.v[r][i] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, g.voff[i] | oob, srow, 0));
  }
}

template <int LD, int LH, int LW, int XS>
__device__ __forceinline__ void bw16_store(const Bw16Regs<LD, LH, LW>& g, unsigned* __restrict__ lds, const mt_conv3d_t& c,
                                           const ConvChunk ch, int lane, int wave) {
  typedef Bw16Regs<LD, LH, LW> RG_;
  constexpr int VPS = RG_::VPS, NI = RG_::NI, R = RG_::R, RPW = RG_::RPW;
  const mt_src_t& S = c.src[ch.src];
  const int cl = (lane & 3) * 4, vl = lane >> 2;
  const bool has_aff = S.scale != nullptr;
  float sc[4], sh[4];
  unsigned cm[2];          // channel validity of the lane's two pairs, as AND masks on the packed dwords
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool cv = (cl + e) < ch.ck;
    sc[e] = cv ? 1.f : 0.f; sh[e] = 0.f;
    if (has_aff && cv) {
      sc[e] = S.scale[(size_t)g.nb * S.C + ch.c0 + cl + e];
      sh[e] = S.shift[(size_t)g.nb * S.C + ch.c0 + cl + e];
    }
  }
  cm[0] = ((cl < ch.ck) ? 0x0000ffffu : 0u) | ((cl + 1 < ch.ck) ? 0xffff0000u : 0u);
  cm[1] = ((cl + 2 < ch.ck) ? 0x0000ffffu : 0u) | ((cl + 3 < ch.ck) ? 0xffff0000u : 0u);
  const float slope = has_aff ? S.slope : 1.f;
  unsigned* lbase = lds + (wave * LW + vl) * BW16_P + cl / 2;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int row = wave + 4 * r;
    if (row < R) {
      const unsigned rm = ((g.rvmask >> r) & 1u) ? 0xffffffffu : 0u;
      unsigned* lrow = lbase + 4 * r * (LW * BW16_P);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int lw = vl + i * VPS;
        if ((i + 1) * VPS <= LW || lw < LW) {
          const unsigned m = g.voff[i] >= 0 ? rm : 0u;            // voxel inside the volume (zero padding applies AFTER the activation)
          const unsigned raw[2] = {g.v[r][i].x, g.v[r][i].y};
          uint2 pk;
          unsigned out[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (XS == MT_BF16 && !has_aff) out[h] = raw[h] & cm[h] & m;       // a bf16 gradient as X (transposed-conv weights): exact copy
            else {
              const float t0 = fmaf(mt_lo16<XS>(raw[h]), sc[2 * h], sh[2 * h]), t1 = fmaf(mt_hi16<XS>(raw[h]), sc[2 * h + 1], sh[2 * h + 1]);
              out[h] = mt_pk16<MT_BF16>(fmaxf(t0, t0 * slope), fmaxf(t1, t1 * slope)) & m;
            }
          }
          pk.x = out[0]; pk.y = out[1];
          *(uint2*)(lrow + i * VPS * BW16_P) = pk;
        }
      }
    }
  }
}

// XS: storage type of X (MT_F16 | MT_BF16), YS: of dY (MT_F32 | MT_BF16 | MT_F16); CW: cout tiles per workgroup (as in conv_bwdw_fast_kernel:
// wave = kq * CW + cw takes cout tile cw and CW of the tile's four 32-voxel blocks — here the staging pass is several times the MFMA phase)
template <int KD, int KH, int KW, int SD, int SH, int SW, int TH, int TW, int XS, int YS, int CW = 1>
__global__ __launch_bounds__(256) void conv_bwdw_fast16_kernel(const BwdWParams P) {
  constexpr int YE = mt_ebytes<YS>();
  constexpr int NT = KD * KH * KW;
  constexpr int PD = (KD == 3) ? 1 : 0, PH = (KH == 3) ? 1 : 0, PW = (KW == 3) ? 1 : 0;
  constexpr int LD = KD, LH = (TH - 1) * SH + KH, LW = (TW - 1) * SW + KW, TV = TH * TW;
  constexpr int KS = TV / 16;            // k-steps (4 voxels each) per wave = 8: the K = 32 of one MFMA
  constexpr int SPR = TW / 4;            // k-steps per tile row
  static_assert(TV == 128 && KS == 8, "tile must hold 128 voxels");
  static_assert((CW == 1 || CW == 2 || CW == 4) && KS % SPR == 0, "cout tiles per workgroup");
  constexpr int GOFF = (KS / SPR) * SH * LW * (2 * BW16_P);      // 2-byte distance between consecutive blocks in the image
  extern __shared__ __attribute__((aligned(16))) unsigned ldsw[];
  const unsigned short* ldsh = (const unsigned short*)ldsw;
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

  const int row0 = (kq * CW * KS) / SPR;
  // 2-byte index of (voxel of k-step 0 at position lk, channel li) in the image; + block * GOFF + compile-time (step voxel + tap voxel) * 2 * BW16_P
  const int xbase0 = ((row0 * SH * LW) + lk * SW) * (2 * BW16_P) + li;
  const int co = cot * 32 + li;
  const bool yaff = Y.scale != nullptr;
  const size_t ysample = (size_t)c.Do * c.Ho * c.Wo * Y.cs;

  auto tile_coords = [&](int tile, int& nb, int& od0, int& oh0, int& ow0) {
    int r = tile;
    const int tw = r % P.tilesW; r /= P.tilesW;
    const int th = r % P.tilesH; r /= P.tilesH;
    od0 = r % P.tilesD; nb = r / P.tilesD;
    oh0 = th * TH; ow0 = tw * TW;
  };
  // dY of this wave's 8 k-steps (2 cout halves each), straight from global, raw; widened / activated / packed in finish_y
  auto issue_y = [&](unsigned (&yb)[KS][2], unsigned& okmask, int nb, int od0, int oh0, int ow0, int kb) {
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
        yb[s2][0] = __builtin_amdgcn_raw_buffer_load_b32(yr, k0 ? base * 4 : (int)0x80000000, 0, 0);
        yb[s2][1] = __builtin_amdgcn_raw_buffer_load_b32(yr, k1 ? (base + 16) * 4 : (int)0x80000000, 0, 0);
      } else {
        yb[s2][0] = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(yr, k0 ? base * 2 : (int)0x80000000, 0, 0);
        yb[s2][1] = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(yr, k1 ? (base + 16) * 2 : (int)0x80000000, 0, 0);
      }
    }
  };
  auto widen_y = [&](unsigned raw) -> float {
    if constexpr (YS == MT_F32) return __builtin_bit_cast(float, raw);
    else return mt_from16<YS>((unsigned short)raw);
  };
  auto finish_y = [&](bf16x8 (&dst)[2], const unsigned (&src)[KS][2], unsigned okmask, int nb) {
    float f[KS][2];
    if (yaff) {
      float ysc0 = 1.f, ysh0 = 0.f, ysc1 = 1.f, ysh1 = 0.f;
      if (co < c.Cout) { ysc0 = Y.scale[(size_t)nb * Y.C + co]; ysh0 = Y.shift[(size_t)nb * Y.C + co]; }
      if (co + 16 < c.Cout) { ysc1 = Y.scale[(size_t)nb * Y.C + co + 16]; ysh1 = Y.shift[(size_t)nb * Y.C + co + 16]; }
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) {
        f[s2][0] = ((okmask >> (2 * s2)) & 1u) ? mt_lrelu(fmaf(widen_y(src[s2][0]), ysc0, ysh0), Y.slope) : 0.f;
        f[s2][1] = ((okmask >> (2 * s2 + 1)) & 1u) ? mt_lrelu(fmaf(widen_y(src[s2][1]), ysc1, ysh1), Y.slope) : 0.f;
      }
    } else {
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) { f[s2][0] = widen_y(src[s2][0]); f[s2][1] = widen_y(src[s2][1]); }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      u32x4 pk;
#pragma unroll
      for (int q = 0; q < 4; ++q) pk[q] = mt_pk16<MT_BF16>(f[2 * q][h], f[2 * q + 1][h]);
      dst[h] = __builtin_bit_cast(bf16x8, pk);
    }
  };
  // the lane's X fragment of one tap: K value j = voxel of k-step j — eight 2-byte reads with immediate offsets
  auto gather = [&](int xbase, int t) -> bf16x8 {
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
    u16x8 a;
    const int toff = ((t / (KH * KW)) * LH + (t / KW) % KH) * LW + (t % KW);
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int svox = (j / SPR) * SH * LW + 4 * (j % SPR) * SW;
      a[j] = ldsh[xbase + (svox + toff) * (2 * BW16_P)];
    }
    return __builtin_bit_cast(bf16x8, a);
  };

  Bw16Regs<LD, LH, LW> xr;
  unsigned ynxt[KS][2];
  bf16x8 ycur[2];
  unsigned yok = 0;
  int ynb = 0;
  int tile = sg;
  int cnb = 0, cod0 = 0, coh0 = 0, cow0 = 0;       // coordinates of the tile in LDS
  if (tile < P.ntiles_total) {
    tile_coords(tile, cnb, cod0, coh0, cow0);
    bw16_load<LD, LH, LW, XS>(xr, c, cc, cnb, cod0 * SD - PD, coh0 * SH - PH, cow0 * SW - PW, lane, wave);
    issue_y(ynxt, yok, cnb, cod0, coh0, cow0, kq * CW);
    ynb = cnb;
  }
  for (; tile < P.ntiles_total; tile += P.nsg) {
    __syncthreads();     // previous tile's X reads are done
    bw16_store<LD, LH, LW, XS>(xr, ldsw, c, cc, lane, wave);
    finish_y(ycur, ynxt, yok, ynb);
    __syncthreads();
    const int tnext = tile + P.nsg;
    const bool more = tnext < P.ntiles_total;
    int nnb = 0, nod0 = 0, noh0 = 0, now0 = 0;
    if (more) {
      tile_coords(tnext, nnb, nod0, noh0, now0);
      bw16_load<LD, LH, LW, XS>(xr, c, cc, nnb, nod0 * SD - PD, noh0 * SH - PH, now0 * SW - PW, lane, wave);
    }
#pragma unroll 1
    for (int g = 0; g < CW; ++g) {
      if (CW > 1 && g > 0) finish_y(ycur, ynxt, yok, ynb);
      if (CW > 1 && g + 1 < CW) issue_y(ynxt, yok, cnb, cod0, coh0, cow0, kq * CW + g + 1);       // dY of the next block: same tile ...
      else if (more) { issue_y(ynxt, yok, nnb, nod0, noh0, now0, kq * CW); ynb = nnb; }          // ... or block 0 of the next one
      const int xbase = xbase0 + g * GOFF;
      __builtin_amdgcn_sched_barrier(0);
      bf16x8 a = gather(xbase, 0);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        bf16x8 an = a;
        if (t + 1 < NT) an = gather(xbase, t + 1);
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, ycur[0], acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, ycur[1], acc[t][1], 0, 0, 0);
        a = an;
      }
    }
    cnb = nnb; cod0 = nod0; coh0 = noh0; cow0 = now0;
  }
  bwdw_wg_reduce_store<NT, false, CW>(acc, (float*)ldsw, P.part + ((size_t)((size_t)(chi * P.ncot + cot) * P.nsg + sg) * NT) * 512, wave, lane, cot < P.ncot);
}

static bool bwdw_fast16_ok(const mt_conv3d_t* p, const mt_src_t* y) {
  if (p->mma != 1 || y == nullptr) return false;
  const int xs = p->src[0].dtype;
  if (!(xs == MT_F16 || xs == MT_BF16)) return false;
  for (int i = 0; i < p->nsrc; ++i) {
    if (p->src[i].dtype != xs || (p->src[i].cs & 1) || (p->src[i].C & 1) || (((uintptr_t)p->src[i].ptr) & 3)) return false;
    if (p->src[i].scale != nullptr && !(p->src[i].slope >= 0.f && p->src[i].slope <= 1.f)) return false;
  }
  // the two combinations the engine produces: fp16 activations x bf16 gradients (convolutions), bf16 gradient x fp16 activations
  // (transposed-conv weights: X = dOut, Y = the layer's input); others keep conv_bwdw_fast_kernel (fp32 products)
  return (xs == MT_F16 && y->dtype == MT_BF16) || (xs == MT_BF16 && y->dtype == MT_F16);
}

template <int KD, int KH, int KW, int SD, int SH, int SW>
static int launch_bwdw_fast16(const BwdWParams& P, hipStream_t st) {
  constexpr int LHa = 3 * SH + KH, LWa = 31 * SW + KW, LHb = 7 * SH + KH, LWb = 15 * SW + KW;
  size_t ldsb = P.TW == 32 ? bw16_lds_bytes<KD, LHa, LWa>() : bw16_lds_bytes<KD, LHb, LWb>();
  if (ldsb < BW_RED_LDS(KD * KH * KW)) ldsb = BW_RED_LDS(KD * KH * KW);
  MT_REQUIRE(ldsb <= 160 * 1024, "bwd_weight: LDS tile too large (%zu)", ldsb);
  dim3 grid(P.nsg, mt_cdiv(P.ncot, P.cw), P.nchunks);
  const int xs = P.c.src[0].dtype, ys = P.y.dtype;
#define MT_BW16_K(KFN_) MT_BWDW_LAUNCH(KFN_, grid, ldsb, st, P)
#define MT_BW16(TH_, TW_)                                                                                     \
  do {                                                                                                        \
    if (xs == MT_F16 && ys == MT_BF16) MT_BW16_K((conv_bwdw_fast16_kernel<KD, KH, KW, SD, SH, SW, TH_, TW_, MT_F16, MT_BF16>)); \
    else if (xs == MT_BF16 && ys == MT_F16) MT_BW16_K((conv_bwdw_fast16_kernel<KD, KH, KW, SD, SH, SW, TH_, TW_, MT_BF16, MT_F16>)); \
    else { mt_set_error("bwd_weight: storage types (X %d, dY %d) not compiled into conv_bwdw_fast16_kernel", xs, ys); return MT_EINVAL; } \
  } while (0)
  // several cout tiles per workgroup (bwdw_fast_cw): the geometries conv_bwdw_fast_kernel has them for
  constexpr bool CWG = (KD == 3 && KH == 3 && KW == 3 && SH == 2 && SW == 2) || (KH == 2 && KW == 2 && SH == 2 && SW == 2) ||
                       (KD == 1 && KH == 3 && KW == 3 && SD == 1 && SH == 1 && SW == 1);
#define MT_BW16C(TH_, TW_, CW_)                                                                               \
  do {                                                                                                        \
    if (xs == MT_F16 && ys == MT_BF16) MT_BW16_K((conv_bwdw_fast16_kernel<KD, KH, KW, SD, SH, SW, TH_, TW_, MT_F16, MT_BF16, CW_>)); \
    else if (xs == MT_BF16 && ys == MT_F16) MT_BW16_K((conv_bwdw_fast16_kernel<KD, KH, KW, SD, SH, SW, TH_, TW_, MT_BF16, MT_F16, CW_>)); \
    else { mt_set_error("bwd_weight: storage types (X %d, dY %d) not compiled into conv_bwdw_fast16_kernel", xs, ys); return MT_EINVAL; } \
  } while (0)
  if (P.cw > 1) {
    if constexpr (CWG) {
      MT_REQUIRE(P.cw == 2 || P.cw == 4, "bwd_weight: %d cout tiles per workgroup", P.cw);
      if (P.TW == 32) { if (P.cw == 4) MT_BW16C(4, 32, 4); else MT_BW16C(4, 32, 2); }
      else            { if (P.cw == 4) MT_BW16C(8, 16, 4); else MT_BW16C(8, 16, 2); }
    } else {
      mt_set_error("bwd_weight: cout tiles per workgroup (%d) on a geometry conv_bwdw_fast16_kernel is not compiled for", P.cw); return MT_EINVAL;
    }
  } else if (P.TW == 32) MT_BW16(4, 32); else MT_BW16(8, 16);
#undef MT_BW16C
#undef MT_BW16
#undef MT_BW16_K
  MT_CHECK_LAUNCH("conv_bwdw_fast16");
  return MT_OK;
}

// ================================================================================================
// conv_bwdw_march16_kernel — the MARCHING form for the strided 3x3x3 stage convs (stride (SD, 2, 2), SD = 1 | 2; VERDICT r3 item 7).
// conv_bwdw_fast16_kernel stages the three input planes of EVERY output plane: a plane is fetched, activated and written to LDS three
// times (SD = 1) or 1.5 times (SD = 2) — for 32 -> 64 @ 48 x 192 x 192 -> 48 x 96 x 96 that is 1.5 GB through the texture path, 620 us.
// Here a workgroup owns a column (sample, h-tile, w-tile) x D segment and walks it plane by plane: the input planes live in a ring of
// four LDS slots (plane u in slot u & 3), each output plane stages only its SD NEW planes (one plane ahead in registers, as before);
// the taps' plane base is a scalar per kd.  Same MFMA phase, dY path, accumulators and reduction as the tiled kernel.
template <int LH, int LW, int NP>
struct Bm16Regs {
  static constexpr int VPS = 16, NI = (LW + VPS - 1) / VPS, R = NP * LH, RPW = (R + 3) / 4;
  uint2 v[RPW][NI];
  int voff[NI];
  unsigned rvmask;
};
// planes up0 .. up0 + NP - 1 (rows uh0 .. uh0 + LH - 1) of sample nb: issue only
template <int LH, int LW, int NP>
__device__ __forceinline__ void bm16_load(Bm16Regs<LH, LW, NP>& g, const mt_conv3d_t& c, const ConvChunk ch, int nb, int up0, int uh0, int uw0,
                                          int lane, int wave) {
  typedef Bm16Regs<LH, LW, NP> RG_;
  constexpr int VPS = RG_::VPS, NI = RG_::NI, R = RG_::R, RPW = RG_::RPW;
  const mt_src_t& S = c.src[ch.src];
  const int cl = (lane & 3) * 4, vl = lane >> 2;
  const int cs = S.cs;
  const size_t sample_elems = (size_t)c.Di * c.Hi * c.Wi * cs;
  __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)S.ptr + (size_t)nb * sample_elems * 2), 0, (int)(sample_elems * 2), 0x00020000);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int lw = vl + i * VPS;
    const int uw = uw0 + lw;
    const bool ok = (cl < ch.ck) && (lw < LW) && ((unsigned)uw < (unsigned)c.Wi);
    g.voff[i] = ok ? (uw * cs + ch.c0 + cl) * 2 : (int)0x80000000;
  }
  g.rvmask = 0;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int row = wave + 4 * r;
    const int lp = row / LH, lhh = row % LH;
    const int ud = up0 + lp, uh = uh0 + lhh;
    const bool rv = (row < R) && ((unsigned)ud < (unsigned)c.Di) && ((unsigned)uh < (unsigned)c.Hi);     // wave-uniform
    const int srow = rv ? (ud * c.Hi + uh) * c.Wi * cs * 2 : 0;
    const int oob = rv ? 0 : (int)0x80000000;
    g.rvmask |= (rv ? 1u : 0u) << r;
#pragma unroll
    for (int i = 0; i < NI; ++i)
      g.v[r][i] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, g.voff[i] | oob, srow, 0));
  }
}
// activation + rounding + store of the planes into their ring slots (plane up0 + lp -> slot (up0 + lp) & 3)
template <int LH, int LW, int NP, int XS>
__device__ __forceinline__ void bm16_store(const Bm16Regs<LH, LW, NP>& g, unsigned* __restrict__ ring, const mt_conv3d_t& c, const ConvChunk ch,
                                           int nb, int up0, int lane, int wave) {
  typedef Bm16Regs<LH, LW, NP> RG_;
  constexpr int VPS = RG_::VPS, NI = RG_::NI, R = RG_::R, RPW = RG_::RPW, PLANE = LH * LW * BW16_P;
  const mt_src_t& S = c.src[ch.src];
  const int cl = (lane & 3) * 4, vl = lane >> 2;
  const bool has_aff = S.scale != nullptr;
  float sc[4], sh[4];
  unsigned cm[2];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool cv = (cl + e) < ch.ck;
    sc[e] = cv ? 1.f : 0.f; sh[e] = 0.f;
    if (has_aff && cv) {
      sc[e] = S.scale[(size_t)nb * S.C + ch.c0 + cl + e];
      sh[e] = S.shift[(size_t)nb * S.C + ch.c0 + cl + e];
    }
  }
  cm[0] = ((cl < ch.ck) ? 0x0000ffffu : 0u) | ((cl + 1 < ch.ck) ? 0xffff0000u : 0u);
  cm[1] = ((cl + 2 < ch.ck) ? 0x0000ffffu : 0u) | ((cl + 3 < ch.ck) ? 0xffff0000u : 0u);
  const float slope = has_aff ? S.slope : 1.f;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int row = wave + 4 * r;
    if (row < R) {
      const int lp = row / LH, lhh = row % LH;
      const unsigned rm = ((g.rvmask >> r) & 1u) ? 0xffffffffu : 0u;
      unsigned* lrow = ring + ((up0 + lp) & 3) * PLANE + (lhh * LW + vl) * BW16_P + cl / 2;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int lw = vl + i * VPS;
        if ((i + 1) * VPS <= LW || lw < LW) {
          const unsigned m = g.voff[i] >= 0 ? rm : 0u;
          const unsigned raw[2] = {g.v[r][i].x, g.v[r][i].y};
          unsigned out[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (XS == MT_BF16 && !has_aff) out[h] = raw[h] & cm[h] & m;
            else {
              const float t0 = fmaf(mt_lo16<XS>(raw[h]), sc[2 * h], sh[2 * h]), t1 = fmaf(mt_hi16<XS>(raw[h]), sc[2 * h + 1], sh[2 * h + 1]);
              out[h] = mt_pk16<MT_BF16>(fmaxf(t0, t0 * slope), fmaxf(t1, t1 * slope)) & m;
            }
          }
          uint2 pk; pk.x = out[0]; pk.y = out[1];
          *(uint2*)(lrow + i * VPS * BW16_P) = pk;
        }
      }
    }
  }
}
#define BM16_LDS_BYTES(LH_, LW_) ((size_t)4 * (LH_) * (LW_) * BW16_P * 4)

// CW: cout tiles per workgroup (wave = kq * CW + cw: cout tile cw, tile rows kq * CW ... kq * CW + CW - 1 of every output plane)
template <int SD, int XS, int YS, int CW = 1>
__global__ __launch_bounds__(256) void conv_bwdw_march16_kernel(const BwdWParams P) {
  constexpr int KD = 3, KH = 3, KW = 3, SH = 2, SW = 2, TH = 4, TW = 32, NT = 27;
  constexpr int YE = mt_ebytes<YS>();
  constexpr int LH = (TH - 1) * SH + KH, LW = (TW - 1) * SW + KW, PLANE = LH * LW * BW16_P;
  constexpr int KS = 8, SPR = TW / 4;
  static_assert(CW == 1 || CW == 2 || CW == 4, "cout tiles per workgroup");
  constexpr int GOFF = SH * LW * (2 * BW16_P);           // 2-byte distance between consecutive tile rows in a plane
  extern __shared__ __attribute__((aligned(16))) unsigned ldsw[];
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

  const int row0 = kq * CW;                              // this wave's first tile row (TW = 32: one row of 32 voxels = 8 k-steps)
  const int xlane = ((row0 * SH * LW) + lk * SW) * (2 * BW16_P) + li;      // 2-byte index inside a plane
  const int co = cot * 32 + li;
  const bool yaff = Y.scale != nullptr;
  const size_t ysample = (size_t)c.Do * c.Ho * c.Wo * Y.cs;
  const unsigned short* ldsh = (const unsigned short*)ldsw;

  auto issue_y = [&](unsigned (&yb)[KS][2], unsigned& okmask, int nb, int od, int oh0, int ow0, int kb) {
    __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)Y.ptr + (size_t)nb * ysample * YE), 0, (int)(ysample * YE), 0x00020000);
    okmask = 0;
    const bool pok = od < c.Do;
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
      const int ks = kb * KS + s2;
      const int oh = oh0 + ks / SPR, ow = ow0 + 4 * (ks % SPR) + lk;
      const bool vok = pok && (oh < c.Ho) && (ow < c.Wo);
      const int base = ((od * c.Ho + oh) * c.Wo + ow) * Y.cs + co;
      const bool k0 = vok && co < c.Cout, k1 = vok && co + 16 < c.Cout;
      okmask |= (k0 ? 1u : 0u) << (2 * s2);
      okmask |= (k1 ? 1u : 0u) << (2 * s2 + 1);
      if constexpr (YS == MT_F32) {
        yb[s2][0] = __builtin_amdgcn_raw_buffer_load_b32(yr, k0 ? base * 4 : (int)0x80000000, 0, 0);
        yb[s2][1] = __builtin_amdgcn_raw_buffer_load_b32(yr, k1 ? (base + 16) * 4 : (int)0x80000000, 0, 0);
      } else {
        yb[s2][0] = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(yr, k0 ? base * 2 : (int)0x80000000, 0, 0);
        yb[s2][1] = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(yr, k1 ? (base + 16) * 2 : (int)0x80000000, 0, 0);
      }
    }
  };
  auto widen_y = [&](unsigned raw) -> float {
    if constexpr (YS == MT_F32) return __builtin_bit_cast(float, raw);
    else return mt_from16<YS>((unsigned short)raw);
  };
  auto finish_y = [&](bf16x8 (&dst)[2], const unsigned (&src)[KS][2], unsigned okmask, int nb) {
    float f[KS][2];
    if (yaff) {
      float ysc0 = 1.f, ysh0 = 0.f, ysc1 = 1.f, ysh1 = 0.f;
      if (co < c.Cout) { ysc0 = Y.scale[(size_t)nb * Y.C + co]; ysh0 = Y.shift[(size_t)nb * Y.C + co]; }
      if (co + 16 < c.Cout) { ysc1 = Y.scale[(size_t)nb * Y.C + co + 16]; ysh1 = Y.shift[(size_t)nb * Y.C + co + 16]; }
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) {
        f[s2][0] = ((okmask >> (2 * s2)) & 1u) ? mt_lrelu(fmaf(widen_y(src[s2][0]), ysc0, ysh0), Y.slope) : 0.f;
        f[s2][1] = ((okmask >> (2 * s2 + 1)) & 1u) ? mt_lrelu(fmaf(widen_y(src[s2][1]), ysc1, ysh1), Y.slope) : 0.f;
      }
    } else {
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) { f[s2][0] = widen_y(src[s2][0]); f[s2][1] = widen_y(src[s2][1]); }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      u32x4 pk;
#pragma unroll
      for (int q = 0; q < 4; ++q) pk[q] = mt_pk16<MT_BF16>(f[2 * q][h], f[2 * q + 1][h]);
      dst[h] = __builtin_bit_cast(bf16x8, pk);
    }
  };

  Bm16Regs<LH, LW, SD> xr;
  unsigned ynxt[KS][2];
  bf16x8 ycur[2];
  unsigned yok = 0;

  for (int unit = sg; unit < P.nunits; unit += P.nsg) {
    int r_ = unit;
    const int seg = r_ % P.nseg; r_ /= P.nseg;
    const int tw = r_ % P.tilesW; r_ /= P.tilesW;
    const int th = r_ % P.tilesH;
    const int nb = r_ / P.tilesH;
    const int oh0 = th * TH, ow0 = tw * TW;
    const int uh0 = oh0 * SH - 1, uw0 = ow0 * SW - 1;
    const int d0 = seg * P.dseg;
    const int d1 = (d0 + P.dseg < c.Do) ? d0 + P.dseg : c.Do;
    // ---- prologue: the planes output plane d0 needs that are not "new" for it: u = d0 * SD - 1 (and, SD == 1, u = d0)
    __syncthreads();                        // the previous unit's ring readers are done
    {
      Bm16Regs<LH, LW, 1> pr;
      bm16_load<LH, LW, 1>(pr, c, cc, nb, d0 * SD - 1, uh0, uw0, lane, wave);
      bm16_store<LH, LW, 1, XS>(pr, ldsw, c, cc, nb, d0 * SD - 1, lane, wave);
      if (SD == 1) {
        bm16_load<LH, LW, 1>(pr, c, cc, nb, d0, uh0, uw0, lane, wave);
        bm16_store<LH, LW, 1, XS>(pr, ldsw, c, cc, nb, d0, lane, wave);
      }
    }
    // new planes of output plane d: u = d * SD + (SD == 1 ? 1 : 0) .. (SD planes)
    bm16_load<LH, LW, SD>(xr, c, cc, nb, d0 * SD + (SD == 1 ? 1 : 0), uh0, uw0, lane, wave);
    issue_y(ynxt, yok, nb, d0, oh0, ow0, kq * CW);
    for (int d = d0; d < d1; ++d) {
      __syncthreads();                      // plane d - 1's MFMA phase is done: its oldest slots may be overwritten
      bm16_store<LH, LW, SD, XS>(xr, ldsw, c, cc, nb, d * SD + (SD == 1 ? 1 : 0), lane, wave);
      finish_y(ycur, ynxt, yok, nb);
      __syncthreads();
      if (d + 1 < d1) bm16_load<LH, LW, SD>(xr, c, cc, nb, (d + 1) * SD + (SD == 1 ? 1 : 0), uh0, uw0, lane, wave);
      int xb[3];                            // 2-byte index of plane d * SD - 1 + kd in the ring
#pragma unroll
      for (int kd = 0; kd < 3; ++kd) xb[kd] = __builtin_amdgcn_readfirstlane(((d * SD - 1 + kd) & 3) * (2 * PLANE)) + xlane;
#pragma unroll 1
      for (int g = 0; g < CW; ++g) {
        if (CW > 1 && g > 0) finish_y(ycur, ynxt, yok, nb);
        if (CW > 1 && g + 1 < CW) issue_y(ynxt, yok, nb, d, oh0, ow0, kq * CW + g + 1);       // dY of the next row of this plane ...
        else if (d + 1 < d1) issue_y(ynxt, yok, nb, d + 1, oh0, ow0, kq * CW);                // ... or of the first row of the next plane
        __builtin_amdgcn_sched_barrier(0);
        const int goff = g * GOFF;
        auto gather = [&](int t) -> bf16x8 {
          typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
          u16x8 a;
          const int toff = ((t / KW) % KH) * LW + (t % KW);
#pragma unroll
          for (int j = 0; j < KS; ++j) {
            const int svox = (j / SPR) * SH * LW + 4 * (j % SPR) * SW;
            a[j] = ldsh[xb[t / (KH * KW)] + goff + (svox + toff) * (2 * BW16_P)];
          }
          return __builtin_bit_cast(bf16x8, a);
        };
        bf16x8 a = gather(0);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          bf16x8 an = a;
          if (t + 1 < NT) an = gather(t + 1);
          acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, ycur[0], acc[t][0], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, ycur[1], acc[t][1], 0, 0, 0);
          a = an;
        }
      }
    }
  }
  bwdw_wg_reduce_store<NT, false, CW>(acc, (float*)ldsw, P.part + ((size_t)((size_t)(chi * P.ncot + cot) * P.nsg + sg) * NT) * 512, wave, lane, cot < P.ncot);
}

static bool bwdw_march16_geo(const mt_conv3d_t* p) {       // (the plan needs it without the dY descriptor)
  return p->mma == 1 && (p->src[0].dtype == MT_F16 || p->src[0].dtype == MT_BF16) && p->KD == 3 && p->KH == 3 && p->KW == 3 && p->SH == 2 &&
         p->SW == 2 && (p->SD == 1 || p->SD == 2) && p->PD == 1 && p->PH == 1 && p->PW == 1 && p->dilD == 1 && p->dilH == 1 && p->dilW == 1 &&
         p->Wo > 16 && p->Do >= 3;
}
static bool bwdw_march16_ok(const mt_conv3d_t* p, const mt_src_t* y) {
  return bwdw_fast16_ok(p, y) && p->src[0].dtype == MT_F16 && y->dtype == MT_BF16 && bwdw_march16_geo(p);
}
template <int SD>
static int launch_bwdw_march16(const BwdWParams& P, hipStream_t st) {
  constexpr int LH = 3 * 2 + 3, LW = 31 * 2 + 3;
  size_t ldsb = BM16_LDS_BYTES(LH, LW);
  if (ldsb < BW_RED_LDS(27)) ldsb = BW_RED_LDS(27);
  dim3 grid(P.nsg, mt_cdiv(P.ncot, P.cw), P.nchunks);
  const int xs = P.c.src[0].dtype, ys = P.y.dtype;
#define MT_BM16_K(KFN_) MT_BWDW_LAUNCH(KFN_, grid, ldsb, st, P)       // (110 KiB: always above the default)
  if (xs == MT_F16 && ys == MT_BF16) {
    if (P.cw == 4) MT_BM16_K((conv_bwdw_march16_kernel<SD, MT_F16, MT_BF16, 4>));
    else if (P.cw == 2) MT_BM16_K((conv_bwdw_march16_kernel<SD, MT_F16, MT_BF16, 2>));
    else MT_BM16_K((conv_bwdw_march16_kernel<SD, MT_F16, MT_BF16>));
  } else { mt_set_error("bwd_weight: storage types (X %d, dY %d) not compiled into conv_bwdw_march16_kernel", xs, ys); return MT_EINVAL; }
#undef MT_BM16_K
  MT_CHECK_LAUNCH("conv_bwdw_march16");
  return MT_OK;
}
