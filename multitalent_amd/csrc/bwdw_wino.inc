// bwdw_wino.inc — backward-weight of 3x3x3 stride-1 convolutions with a 2D Winograd transform (included by conv_bwdw.hip).
//
// dW[kd][kh][kw] = sum over output voxels of X[o + k - 1] * dY[o].  Group the outputs of a plane into 2x2 (h, w) tiles: per tile
// the (kh, kw) part is F(3x3, 2x2) — 3x3 results from a 4x4 X block and the 2x2 dY block with 16 instead of 36 products:
//   V = B^T X B (4x4),  W = A dY A^T (4x4, A = [[1,0],[1,1],[1,-1],[0,-1]]),  M_xi += V_xi * W_xi over ALL tiles (the GEMM K),
//   dW = G^T M G once at the very end (G^T = [[1,.5,.5,0],[0,.5,-.5,0],[0,.5,.5,1]]);  kd stays a direct sum over three planes.
// 48 virtual taps (3 kd x 16 xi) on 4-tile k-steps replace 27 taps on 4-voxel k-steps: 2.25x fewer MFMAs.
// Structure = the marching kernel: a workgroup owns a column (4 x 32 outputs) and marches along D.  Thread (tile column, cin)
// fetches the 6x4 X block of its two tiles straight from global memory (no raw LDS image, no extra barrier), applies the lazy
// activation, transforms both tiles in registers and writes V[xi][tile][cin] into a ring of 4 planes; ONE barrier per plane.
// dY fragments are loaded straight into registers and transformed there (18 VALU per 48 MFMAs).  Waves = (tile row kq) x (cout half nh): 48 accumulator tiles of 16x16 each.
#ifndef BWW_ABL
#define BWW_ABL 0      // timing ablations: 1 skip X load+transform, 2 skip dY loads, 8 skip MFMA loop
#endif
#ifndef BWW_PIPE
#define BWW_PIPE 1     // 1: the X transform of plane d+2 is interleaved with the MFMAs of step d (0: plane d+1 before the barrier)
#endif
#define BWW_RP 20                       // dword pitch of a voxel in the raw plane (16 used): 2-way worst case in the transform gathers
#define BWW_VPL (16 * 32 * 16)          // floats of one transformed plane: [xi 16][tile 32][cin 16]
#define BWW_RAWF (8 * 40 * BWW_RP)      // raw plane: 8 padded rows x 40 padded voxels
#define BWW_LDS_FLOATS (4 * BWW_VPL)

// CW = 2 (round 4): two cout tiles per workgroup.  Wave w owns the 16 output channels 64 * blockIdx.y + 16 w ... and BOTH tile rows
// (two MFMA passes per plane) instead of one tile row of one cout half: the same 48 accumulator tiles per wave, but a transformed X plane
// — the load + activation + B^T X B path is ~22 % of the kernel at CW = 1 — feeds twice the MFMAs, its 14 slices sit in the first
// pass, and the two-wave reduction at the end disappears.
// KD = 1 (round 5): the 1x3x3 convolutions of the residual encoder's first stage (generic_modular_residual_UNet.py:69-71, plan
// conv_kernel_sizes[0] = [1, 3, 3]) — the same march with ONE plane per step (no depth halo): 16 virtual taps, a third of the MFMAs
// for the same X / dY stream, the 14 transform slices after every fourth MFMA.
template <int VEC, int CW = 1, int KD = 3>
__global__ __launch_bounds__(256) void conv_bwdw_wino_kernel(const BwdWParams P) {
  static_assert(VEC == 2 && (CW == 1 || CW == 2) && (KD == 3 || KD == 1), "8-byte channel pairs only");
  constexpr int NKQ = CW;                // tile rows (K halves) a wave multiplies per plane
  constexpr int TH = 4, TW = 32, LH = TH + 2, LW = TW + 2;
  constexpr int NVT = KD * 16;           // virtual taps: kd * 16 + b * 4 + c
  constexpr int NT = KD * 9;             // taps of the result
  constexpr int RING = (KD == 3) ? 4 : 2;   // transformed planes in LDS; KD = 1: 64 KiB, two workgroups per CU hide each other's latencies
  constexpr int TA = (KD == 3) ? 2 : 1;     // the transform runs TA planes ahead of the MFMAs, the loads TA + 1
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* VR = lds;                       // ring of 4 transformed planes
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int kq = (CW == 1) ? (wave >> 1) : 0, nh = wave & 1;      // (first) tile row and cout half of this wave
  const int sg = blockIdx.x, cot = (CW == 1) ? blockIdx.y : blockIdx.y * 2 + (wave >> 1), chi = blockIdx.z;
  const ConvChunk cc = P.chunk[chi];
  const mt_src_t& Y = P.y;
  const mt_src_t& S = c.src[cc.src];

  f32x4 acc[NVT];
#pragma unroll
  for (int t = 0; t < NVT; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = 0.f;

  const int co = cot * 32 + nh * 16 + li;
  const bool yaff = Y.scale != nullptr;
  const size_t ysample = (size_t)c.Do * c.Ho * c.Wo * Y.cs;
  const size_t xsample = (size_t)c.Di * c.Hi * c.Wi * S.cs;
  const int xplane_bytes = __builtin_amdgcn_readfirstlane(c.Hi * c.Wi * S.cs * 4);
  const int yplane_bytes = __builtin_amdgcn_readfirstlane(c.Ho * c.Wo * Y.cs * 4);
  const bool xaff = S.scale != nullptr;
  const float xslope = xaff ? S.slope : 1.f;
  // transform thread = (tile column tcol = tid>>4, cin tci = tid&15): X block rows 0..5 (both tile rows), columns 2*tcol..+3
  const int tcol = tid >> 4, tci = tid & 15;
  const bool tcv = tci < cc.ck;
  // MFMA A operand: V[xi][tile = kq*16 + 4s + lk][cin li]
  const int alane = (kq * 16 + lk) * 16 + li;

  float xv[6][4];                        // X block in flight: rows 0..5 of the column's halo, 4 columns
  float yr[NKQ][4][4];                   // dY 2x2 blocks of this lane's tile in each of the 4 k-steps: [tile row][s][r*2+c]

  for (int unit = sg; unit < P.nunits; unit += P.nsg) {
    int r_ = unit;
    const int seg = r_ % P.nseg; r_ /= P.nseg;
    const int tw = r_ % P.tilesW; r_ /= P.tilesW;
    const int th = r_ % P.tilesH;
    const int nb = r_ / P.tilesH;
    const int oh0 = th * TH, ow0 = tw * TW;
    const int uh0 = oh0 - 1, uw0 = ow0 - 1;
    const int d0 = seg * P.dseg;
    const int d1 = (d0 + P.dseg < c.Do) ? d0 + P.dseg : c.Do;
    __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)(S.ptr + (size_t)nb * xsample), 0, (int)(xsample * 4), 0x00020000);
    __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)(Y.ptr + (size_t)nb * ysample), 0, (int)(ysample * 4), 0x00020000);
    __amdgpu_buffer_rsrc_t nullrs = __builtin_amdgcn_make_buffer_rsrc((void*)Y.ptr, 0, 0, 0x00020000);     // num_records = 0
    int xco[4];                          // byte offset of this thread's 4 columns inside a row (or the masked offset)
    unsigned xcm[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int uw = uw0 + 2 * tcol + k;
      const bool ok = tcv && ((unsigned)uw < (unsigned)c.Wi);
      xco[k] = ok ? (uw * S.cs + cc.c0 + tci) * 4 : (int)0x80000000;
      xcm[k] = ok ? 0xffffffffu : 0u;
    }
    int rowm[6], rowoff[6];               // wave-uniform: the six halo rows of this column
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const int uh = uh0 + r;
      const bool ok = (unsigned)uh < (unsigned)c.Hi;
      rowm[r] = ok ? -1 : 0;
      rowoff[r] = ok ? uh * c.Wi * S.cs * 4 : 0;
    }
    float sc = tcv ? 1.f : 0.f, sh = 0.f;
    if (xaff && tcv) { sc = S.scale[(size_t)nb * S.C + cc.c0 + tci]; sh = S.shift[(size_t)nb * S.C + cc.c0 + tci]; }
    float sck[4], shk[4];                 // per column: the lazy affine, 0 / 0 where the column lies outside the tensor
#pragma unroll
    for (int k = 0; k < 4; ++k) { sck[k] = xcm[k] ? sc : 0.f; shk[k] = xcm[k] ? sh : 0.f; }
    // dY offsets: k-step s, tile column 4s + lk, tile row kq; block element (r, c2)
    int yvo[NKQ][4][4];
#pragma unroll
    for (int q = 0; q < NKQ; ++q)
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int oh = oh0 + 2 * (kq + q) + (e >> 1), ow = ow0 + 2 * (4 * s + lk) + (e & 1);
          const bool ok = (oh < c.Ho) && (ow < c.Wo) && (co < c.Cout);
          yvo[q][s][e] = ok ? ((oh * c.Wo + ow) * Y.cs + co) * 4 : (int)0x80000000;
        }
    float ysc = 1.f, ysh = 0.f;
    if (yaff && co < c.Cout) { ysc = Y.scale[(size_t)nb * Y.C + co]; ysh = Y.shift[(size_t)nb * Y.C + co]; }

    auto load_x = [&](int ud) {            // issue only: 24 scalar loads, cin-contiguous across lanes
      const int pvm = ((unsigned)ud < (unsigned)c.Di) ? -1 : 0;
      const int poff = (ud & pvm) * xplane_bytes;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        const int oob = ~(pvm & rowm[r]) & (int)0x80000000;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          xv[r][k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, xco[k] | oob, poff + rowoff[r], 0));
      }
    };
    auto transform_x = [&](int ud, int slot) {   // registers -> V[slot][xi][tile][cin] for the tiles (row 0, tcol) and (row 1, tcol)
      const int pvm = ((unsigned)ud < (unsigned)c.Di) ? -1 : 0;
      float a[6][4];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        const unsigned rvm = (unsigned)(pvm & rowm[r]);
        const float scq = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, sc) & rvm);
        const float shq = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, sh) & rvm);
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          x[k] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, mt_lrelu(fmaf(xv[r][k], scq, shq), xslope)) & xcm[k]);
        a[r][0] = x[0] - x[2]; a[r][1] = x[1] + x[2]; a[r][2] = x[2] - x[1]; a[r][3] = x[1] - x[3];      // B^T along w
      }
      float* vp = VR + slot * BWW_VPL + tid;
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float x0 = a[2 * q][k], x1 = a[2 * q + 1][k], x2 = a[2 * q + 2][k], x3 = a[2 * q + 3][k];             // B^T along h
          vp[(0 * 4 + k) * 512 + q * 256] = x0 - x2;
          vp[(1 * 4 + k) * 512 + q * 256] = x1 + x2;
          vp[(2 * 4 + k) * 512 + q * 256] = x2 - x1;
          vp[(3 * 4 + k) * 512 + q * 256] = x1 - x3;
        }
    };
    auto load_y = [&](int q, int s, int poff, int oob) {       // oob != 0 (past the last plane of the unit): the empty descriptor
      const __amdgpu_buffer_rsrc_t rr = oob ? nullrs : yrs;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        yr[q][s][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, yvo[q][s][e], poff, 0));
    };

    // ---- prologue: planes d0-1, d0 and d0+1 transformed into the ring, plane d0+2 and the dY blocks of plane d0 in flight
    __syncthreads();                     // the previous unit's MFMAs (ring readers) are done
    if (!BWW_PIPE) {
      load_x(d0 - 1);
      transform_x(d0 - 1, (d0 + 3) & 3);
      load_x(d0);
      transform_x(d0, d0 & 3);
      load_x(d0 + 1);
    } else {
      if constexpr (KD == 3) {
        load_x(d0 - 1);
        transform_x(d0 - 1, (d0 + 3) & 3);
        load_x(d0);
        transform_x(d0, d0 & 3);
        load_x(d0 + 1);
        transform_x(d0 + 1, (d0 + 1) & 3);
        load_x(d0 + 2);
      } else {
        load_x(d0);
        transform_x(d0, d0 & 1);
        load_x(d0 + 1);
      }
    }
    {
      const int p0 = __builtin_amdgcn_readfirstlane(d0 * yplane_bytes);
#pragma unroll
      for (int q = 0; q < NKQ; ++q)
#pragma unroll
        for (int s = 0; s < 4; ++s) load_y(q, s, p0, 0);
    }

    for (int d = d0; d < d1; ++d) {
      // !BWW_PIPE: plane d+1 is transformed here, before the barrier (slot (d+1)&3 last held plane d-3, read no later than the
      // MFMAs of step d-2: every wave has passed the barrier of step d-1 since then)
      if (!BWW_PIPE && !(BWW_ABL & 1)) transform_x(d + 1, (d + 1) & 3);
      __syncthreads();
      const bool more = d + 1 < d1;
      if (!BWW_PIPE && more && !(BWW_ABL & 1)) load_x(d + 2);
      const int ynext = __builtin_amdgcn_readfirstlane(more ? (d + 1) * yplane_bytes : 0);
      const int yoob = __builtin_amdgcn_readfirstlane(more ? 0 : (int)0x80000000);
      int xb[KD];
#pragma unroll
      for (int kd = 0; kd < KD; ++kd) xb[kd] = ((d + (KD == 3 ? 3 + kd : 0)) & (RING - 1)) * BWW_VPL + alane;       // plane d-1+kd (KD = 1: plane d)
      if (BWW_ABL & 8) continue;
      // BWW_PIPE: with one wave per SIMD nothing hides a latency, so the transform of plane d+2 (registers xv, fetched during
      // step d-1) is cut into 14 slices that sit BETWEEN the MFMAs of this step: six rows (activation + B^T along w; the row's
      // registers are refilled with plane d+3 at once) and eight (tile row, column) pieces (B^T along h + the LDS stores into
      // slot (d+2)&3 = the slot of plane d-2, whose last readers were the MFMAs of step d-1, before this step's barrier).
      // The planes d1+1, d1+2 transformed / fetched by the last two steps of a unit are not used (masked loads past Di).
      const int t_ud = d + TA, l_ud = d + TA + 1;
      const int t_pvm = ((unsigned)t_ud < (unsigned)c.Di) ? -1 : 0;
      const int l_pvm = (((unsigned)l_ud < (unsigned)c.Di) && (d + 2 < d1)) ? -1 : 0;
      const int l_poff = __builtin_amdgcn_readfirstlane((l_ud & l_pvm) * xplane_bytes);
      float* const t_vp = VR + ((d + TA) & (RING - 1)) * BWW_VPL + tid;
      float xa[6][4];
      auto x_row = [&](int r) {
        // column validity is folded into the per-column scale / shift (an invalid column loads 0 and has scale = shift = 0); a row
        // outside the tensor (wave-uniform, rare) is a scalar branch instead of a mask per element: every instruction between
        // the MFMAs costs matrix time
        if (t_pvm & rowm[r]) {
          float x[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) { const float t = fmaf(xv[r][k], sck[k], shk[k]); x[k] = fmaxf(t, t * xslope); }   // 0 <= slope <= 1 (host check)
          xa[r][0] = x[0] - x[2]; xa[r][1] = x[1] + x[2]; xa[r][2] = x[2] - x[1]; xa[r][3] = x[1] - x[3];      // B^T along w
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) xa[r][k] = 0.f;
        }
      };
      auto x_refill = [&](int r, int k) {
        // a row / plane outside the tensor reads through an EMPTY descriptor (every load returns 0): a scalar select instead of
        // one v_or per load
        const __amdgpu_buffer_rsrc_t rr = (l_pvm & rowm[r]) ? xrs : nullrs;
        xv[r][k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, xco[k], l_poff + rowoff[r], 0));
      };
      auto x_col = [&](int q, int k) {
        const float x0 = xa[2 * q][k], x1 = xa[2 * q + 1][k], x2 = xa[2 * q + 2][k], x3 = xa[2 * q + 3][k];             // B^T along h
        t_vp[(0 * 4 + k) * 512 + q * 256] = x0 - x2;
        t_vp[(1 * 4 + k) * 512 + q * 256] = x1 + x2;
        t_vp[(2 * 4 + k) * 512 + q * 256] = x2 - x1;
        t_vp[(3 * 4 + k) * 512 + q * 256] = x1 - x3;
      };
      // slice i = 0..13 follows MFMA t = 5 + 12 (i & 3) of k-step s = i >> 2: rows 0-3 (each followed by its four refills, plane d+3),
      // tile row 0, rows 4-5, tile row 1.  (Spreading the 24 + 16 loads of a plane one by one over the 192 MFMAs instead was measured
      // slower, 1.074 vs 1.052 ms: a load costs the issuing wave ~35 cycles wherever it sits.)
      auto events = [&](const int m) {     // (m is a constant after unrolling)
        if (BWW_ABL & 1) return;
        if ((m % (NVT / 4)) != (KD == 3 ? 5 : 1)) return;
        const int i = m / (NVT / 4);
        if (i < 4) { x_row(i); for (int k = 0; k < 4; ++k) x_refill(i, k); }
        else if (i < 8) x_col(0, i - 4);
        else if (i < 10) { x_row(i - 4); for (int k = 0; k < 4; ++k) x_refill(i - 4, k); }
        else if (i < 14) x_col(1, i - 10);
      };
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < NKQ; ++q) {
      float a0[NVT], a1[NVT];
#pragma unroll
      for (int t = 0; t < NVT; ++t) a0[t] = VR[xb[t >> 4] + q * 256 + (t & 15) * 512];        // tile row q: tiles 16 q ... 16 q + 15 (x 16 cin)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float (&ac)[NVT] = (s & 1) ? a1 : a0;
        float (&an)[NVT] = (s & 1) ? a0 : a1;
        // W = A g A^T of this lane's 2x2 dY block
        float g0 = yr[q][s][0], g1 = yr[q][s][1], g2 = yr[q][s][2], g3 = yr[q][s][3];
        if (yaff) {
          g0 = (yvo[q][s][0] >= 0) ? mt_lrelu(fmaf(g0, ysc, ysh), Y.slope) : 0.f;
          g1 = (yvo[q][s][1] >= 0) ? mt_lrelu(fmaf(g1, ysc, ysh), Y.slope) : 0.f;
          g2 = (yvo[q][s][2] >= 0) ? mt_lrelu(fmaf(g2, ysc, ysh), Y.slope) : 0.f;
          g3 = (yvo[q][s][3] >= 0) ? mt_lrelu(fmaf(g3, ysc, ysh), Y.slope) : 0.f;
        }
        if (!(BWW_ABL & 2)) load_y(q, s, ynext, yoob);         // the raw block is consumed: fetch the next plane's in place
        float w[16];
        {
          const float t00 = g0, t01 = g0 + g1, t02 = g0 - g1, t03 = -g1;     // row 0 along w
          const float t10 = g2, t11 = g2 + g3, t12 = g2 - g3, t13 = -g3;     // row 1
          w[0] = t00; w[1] = t01; w[2] = t02; w[3] = t03;
          w[4] = t00 + t10; w[5] = t01 + t11; w[6] = t02 + t12; w[7] = t03 + t13;
          w[8] = t00 - t10; w[9] = t01 - t11; w[10] = t02 - t12; w[11] = t03 - t13;
          w[12] = -t10; w[13] = -t11; w[14] = -t12; w[15] = -t13;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NVT; ++t) {
          if (s + 1 < 4) an[t] = VR[xb[t >> 4] + q * 256 + (t & 15) * 512 + (s + 1) * 64];
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[t], w[t & 15], acc[t], 0, 0, 0);
          if (BWW_PIPE && q == 0) events(s * NVT + t);
          if ((t & 1) == 1) __builtin_amdgcn_sched_barrier(0);
        }
      }
      }
    }
  }

  // ---- output transform dW = G^T M G per (kd, accumulator register), then the two tile rows (K halves) are summed through LDS
  f32x4 o[NT];
#pragma unroll
  for (int kd = 0; kd < KD; ++kd)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float u[4][3];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float m0 = acc[kd * 16 + b * 4 + 0][j], m1 = acc[kd * 16 + b * 4 + 1][j], m2 = acc[kd * 16 + b * 4 + 2][j], m3 = acc[kd * 16 + b * 4 + 3][j];
        const float hs = 0.5f * (m1 + m2), hd = 0.5f * (m1 - m2);
        u[b][0] = m0 + hs; u[b][1] = hd; u[b][2] = hs + m3;
      }
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const float hs = 0.5f * (u[1][kw] + u[2][kw]), hd = 0.5f * (u[1][kw] - u[2][kw]);
        o[kd * 9 + 0 * 3 + kw][j] = u[0][kw] + hs;
        o[kd * 9 + 1 * 3 + kw][j] = hd;
        o[kd * 9 + 2 * 3 + kw][j] = hs + u[3][kw];
      }
    }
  if constexpr (CW == 2) {               // every wave holds the complete sums of its 16 channels: one partial per (workgroup, cout tile)
    if (cot < P.ncot) {
      float* pp = P.part + ((size_t)((size_t)(chi * P.ncot + cot) * P.nsg + sg) * NT) * 512;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          pp[(size_t)t * 512 + (lk * 4 + j) * 32 + nh * 16 + li] = o[t][j];
    }
    return;
  }
  __syncthreads();
  float* red = lds;                      // [nh][tap NT][j 4][lane 64]
  if (kq == 1) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[((nh * NT + t) * 4 + j) * 64 + lane] = o[t][j];
  }
  __syncthreads();
  if (kq == 0) {
    float* pp = P.part + ((size_t)((size_t)(chi * P.ncot + cot) * P.nsg + sg) * NT) * 512;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        pp[(size_t)t * 512 + (lk * 4 + j) * 32 + nh * 16 + li] = o[t][j] + red[((nh * NT + t) * 4 + j) * 64 + lane];
  }
}
