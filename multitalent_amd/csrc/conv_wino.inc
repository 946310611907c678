// conv_wino.inc — 3D Winograd F(2x2x2, 3x3x3) convolution (included by conv_lds.hip).
//
// The fp32 matrix rate (157 TFLOP/s) bounds every direct 3x3x3 convolution; the only way past it is fewer multiplications.
// F(2x2x2, 3x3x3) computes a 2x2x2 output block from a 4x4x4 input block with 64 instead of 216 multiply-accumulates per
// (cin, cout) pair: 3.375x less MFMA work, paid with additions in the input/output transforms (VALU) and LDS traffic.
//   V = B^T d B (3D, per tile and input channel),  U = G g G^T (3D, per cin/cout, done by the packing kernel),
//   M_xi = V_xi . U_xi (64 independent GEMMs over cin),  Y = A^T M A (3D).
// Workgroup = 4x4x16 outputs = 32 Winograd tiles (one MFMA M tile) x 32 output channels; input channels in chunks of 8.
// Per chunk:  A) the haloed 6x6x18 patch goes to LDS (lazy InstanceNorm+LeakyReLU applied),  B) thread (tile, channel)
// transforms its 4x4x4 block in registers and writes V[xi][tile][channel],  C) wave w accumulates the 16 GEMMs xi = 16w..16w+15
// (a = w in xi = (a,b,c)) into 16 accumulator tiles (256 registers).  D) after the last chunk every wave contracts (b, c) of
// its tiles in registers, the four waves exchange the a-partials through LDS and each finishes one (od, oh) quarter.
// Numerics: transforms use +-1 and 0.5 only; relative error vs the direct fp32 sum ~1e-7 (tools/wino/check_transforms.py).
#ifndef WN_ABL
#define WN_ABL 0     // timing ablations: 1 skip phase A (patch staging), 2 skip phase B (input transform), 4 skip phase C (MFMA), 8 skip phase D
#endif
#ifndef WN_OPT
#define WN_OPT 0
#endif
#ifndef WN_BPF
#define WN_BPF 5      // weight-fragment prefetch distance (xi) in the 8-wave kernel
#endif
#ifndef WN_TPF
#define WN_TPF 6      // persistent kernel, transformer waves: weight fragments requested before the transform (the rest 2 xi ahead)
#endif
#ifndef WN_TS
#define WN_TS 0       // 1: per-wave cycle totals per phase (s_memtime) written to c.out1[wave][16] (tools/bench_conv.py --ts)
#endif
#ifndef WN_SRING
#define WN_SRING 0      // persistent kernel, stager waves: weight-fragment ring inside the MFMA phase
#endif
#ifndef WN_SPRIO
#define WN_SPRIO 1      // persistent kernel: static issue priority of the stager waves (see wino8p_body)
#endif
#define WCK 8            // input channels per chunk
#define WRP 12           // dword pitch of a voxel in the RAW patch (8 used): makes the phase-B gathers 2-way at worst
#define W_RAWF (648 * WRP)
#define W_VF (64 * 256)


// ================================================================================================
// Persistent form of the 8-wave kernel (default): one workgroup per CU walks over spatial tiles t = lw, lw + NW, ... of one
// output-channel tile, and the (tile, chunk) pairs form ONE continuous software pipeline — the stager waves fetch and store the
// first patches of the NEXT tile while the last chunk of the current tile is multiplied and its outputs are transformed.  In the
// one-tile-per-workgroup kernel every tile began with an exposed HBM round trip (0.26 of 1.21 ms on 30 -> 30 @ 48x192x192,
// profiles/r01_pmc_conv_wino.txt); here only the first tile of a CU pays it.  Differences from conv_wino8_kernel:
//   * RAW double-buffer parity follows the global step g = iteration * nchunks + chunk;
//   * validity of the patch in flight is a bit mask fetched with it (the stagers' tile coordinates run ahead of the tile that is
//     being multiplied), the per-thread patch geometry (linear offsets, local coordinates) is computed once per kernel;
//   * the output transform exchanges its partials through the V region (dead after the last MFMA phase of a tile) instead of
//     the RAW region (which already holds the next tile's first patch).
// Role-specialised body: STAGER = waves 4-7 (fetch / activate / store patches), !STAGER = waves 0-3 (input transform).  Both roles
// run the same MFMA phases, output transform and the SAME sequence of barriers; compiling them as separate code paths keeps the
// patch-in-flight registers out of the transformers' live ranges and the 64-value transform block out of the stagers'
// (one merged path needs > 256 VGPRs and spills).
template <bool STAGER, bool BSTK>
__device__ __forceinline__ void wino8p_body(const ConvKParams& P) {
  constexpr int TD = 4, TH = 4, TW = 16, LH = 6, LW = 18, NTASK = 648 * 2, NJ = (NTASK + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* V = lds + 2 * W_RAWF;
  const mt_conv3d_t& c = P.c;
  const int tid = threadIdx.x, lane = tid & 63, tl = tid & 255;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lhalf = lane >> 5;
  const int ntile = blockIdx.y;
  const int T = P.nsb * c.N;
  // The workers of one group (= one XCD whenever gridDim.x is a multiple of 8: workgroups go round-robin over the XCDs in
  // dispatch order) share a CONTIGUOUS range of the tile sequence and walk it side by side, NWK tiles per iteration, in the order
  // D, H, W: what the group holds at one time is a compact D x H block of tiles whose halo rows are fetched into that XCD's L2
  // once; the workers of the other output-channel tiles (blockIdx.y) walk the same range at the same time.
  const int ngrp = (int)gridDim.x < 8 ? (int)gridDim.x : 8;
  const int grp = (int)blockIdx.x % ngrp;
  const int NWK = ((int)gridDim.x - grp + ngrp - 1) / ngrp;             // workers of this group
  const int tbase = (int)(((long)T * grp) / ngrp);
  const int lw = tbase + (int)blockIdx.x / ngrp;
  const int tend = (int)(((long)T * (grp + 1)) / ngrp);
  if (lw >= tend) return;                                // (workgroup-uniform)
  const int niter = (tend - lw + NWK - 1) / NWK;
  const int G = niter * P.nchunks;

  // tile index -> coordinates
  auto decode = [&](int t, int& nb, int& od0, int& oh0, int& ow0, int& sb) {
    int td_, th_, tw_;
    mt_tile_coords(t, P.tilesD, P.tilesH, P.tilesW, td_, th_, tw_, nb);
    sb = (td_ * P.tilesH + th_) * P.tilesW + tw_;
    od0 = td_ * TD; oh0 = th_ * TH; ow0 = tw_ * TW;
  };

  // ---- per-thread patch geometry, tile independent: task e = tl + 256 j -> (voxel e>>1 of the 6x6x18 patch, channel quad e&1):
  // 16-byte loads, two lanes per voxel — a gather costs the issuing wave ~130 cycles whatever it fetches (measured: neither the
  // bytes nor the number of distinct lines per instruction matter), so the patch is 6 instructions instead of 11 and the
  // scale / shift of the lane's four channels are one 16-byte load each (per-dword range check: channels beyond C read 0)
  // packed per task: bits 0-19 linear offset (ld*Hi + lh)*Wi + lw inside the sample (the dispatcher guarantees 5*Hi*Wi < 2^20),
  // bits 20-22 ld, 23-25 lh, 26-30 lw.  Kept in LDS ([j][thread], 11 KiB behind V): eleven registers less across the whole loop
  int* const PCO = (int*)(lds + 2 * W_RAWF + W_VF) + tl;
  if constexpr (STAGER) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = tl + 256 * j, vox = e >> 1;
      const int lw_ = vox % LW, lh = (vox / LW) % LH, ld = vox / (LW * LH);
      PCO[j * 256] = (e < NTASK) ? (((ld * c.Hi + lh) * c.Wi + lw_) | (ld << 20) | (lh << 23) | (lw_ << 26)) : (7 << 20);   // ld = 7: never valid
    }
  }
  const int cg4 = (tl & 1) * 4;
  const int rawst = (tl >> 1) * WRP + cg4;
  const int tB = tl >> 3, cB = tl & 7;
  const int rawrd = ((((tB >> 4) * 2) * LH + ((tB >> 3) & 1) * 2) * LW + (tB & 7) * 2) * WRP + cB;
  const int wa = wave >> 1, wh = wave & 1;              // this wave's a and c-half
  const int xi0 = wa * 16 + 2 * wh;                     // xi of accumulator j = (b = j>>1, cl = j&1): xi0 + b*4 + cl
  const float* va = V + xi0 * 256 + li * 8 + 4 * lhalf;

  __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)c.wpack, 0, 0x7fffffff, 0x00020000);

  // ---- stager state: the patch in flight (registers) belongs to global step gi - 1; gi = next step to issue
  f32x4 pv[NJ];
  f32x4 psc, psh;
  float pcv[4], pslope = 1.f;
  unsigned pmask = 0;                                    // validity bits of the patch in flight
  int gi = 0, gs = 0, i_ch = 0, i_k = 0;                 // next step to issue (= iteration i_k, chunk i_ch) / next step to store
  int i_nb = 0, i_base = 0, i_od = 0, i_oh = 0, i_ow = 0;  // tile of step gi (stagers only)
  unsigned i_mask = 0;
  auto stager_tile = [&](int k) {                        // coordinates + validity mask of the tile of iteration k
    int sbx;
    decode(lw + k * NWK, i_nb, i_od, i_oh, i_ow, sbx);
    i_base = ((i_od - 1) * c.Hi + (i_oh - 1)) * c.Wi + (i_ow - 1);
    // all table reads first (one LDS round trip), then branch-free bit arithmetic: hipcc turns `a && b` on loaded values into an
    // exec-masked branch per task with its own ds_read + s_waitcnt inside
    int pc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) pc[j] = PCO[j * 256];
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ld = (pc[j] >> 20) & 7, ud = i_od - 1 + ld, uh = i_oh - 1 + ((pc[j] >> 23) & 7), uw = i_ow - 1 + (pc[j] >> 26);
      const unsigned ok = (unsigned)(ld < 6) & (unsigned)((unsigned)ud < (unsigned)c.Di) & (unsigned)((unsigned)uh < (unsigned)c.Hi) &
                          (unsigned)((unsigned)uw < (unsigned)c.Wi);
      m |= ok << j;
    }
    i_mask = m;
  };
  // The request of a patch: issue_prepare (which (tile, chunk) comes next, validity mask of a new tile) and issue_loads(part) (the
  // 4 + 11 loads in NPART groups).  The texture path needs ~2 cycles per distinct 128-B line of these gathers (16 lines per
  // instruction, ~2000 cycles per patch and CU, profiles/r02_wino_phase_cycles.txt).  !live (past the last step): the same loads with every offset masked
  // — the instruction stream must not branch around vector-memory operations, or the waitcnt pass has to assume on every path that
  // the weight fragments are the youngest loads (and drains the patch in flight).
  // The descriptors the request needs were a chain of dependent scalar loads in the middle of the staging (chunk -> source index ->
  // source fields -> scale/shift pointers: six s_load + s_waitcnt lgkmcnt(0) round trips per patch).  The two sources' fields are
  // read once (SGPRs, selected by the chunk's source index), the chunk entry of the NEXT request at the top of the step.
  constexpr int NPART = 6;
  const float* const sp_ptr0 = c.src[0].ptr;   const float* const sp_ptr1 = c.src[1].ptr;
  const float* const sp_sc0 = c.src[0].scale;  const float* const sp_sc1 = c.src[1].scale;
  const float* const sp_sh0 = c.src[0].shift;  const float* const sp_sh1 = c.src[1].shift;
  const int sp_C0 = c.src[0].C, sp_C1 = c.src[1].C, sp_cs0 = c.src[0].cs, sp_cs1 = c.src[1].cs;
  const float sp_sl0 = c.src[0].slope, sp_sl1 = c.src[1].slope;
  bool q_live = false; ConvChunk q_cc = P.chunk[0];
  auto issue_prepare = [&](bool live, const ConvChunk cc) {
    q_live = live; q_cc = cc;
    if (live && i_ch == 0) stager_tile(i_k);
    if (live) { ++gi; if (++i_ch == P.nchunks) { i_ch = 0; ++i_k; } }
  };
  auto issue_loads = [&](int part) {
    const int dead = q_live ? 0 : (int)0x80000000;
    const ConvChunk cc = q_cc;
    const bool s1 = cc.src != 0;
    const float* const S_ptr = s1 ? sp_ptr1 : sp_ptr0;
    const float* const S_scale = s1 ? sp_sc1 : sp_sc0;
    const float* const S_shift = s1 ? sp_sh1 : sp_sh0;
    const int S_C = s1 ? sp_C1 : sp_C0, S_cs = s1 ? sp_cs1 : sp_cs0;
    if (part == 0) {
      const bool aff = S_scale != nullptr;
      __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc((void*)(aff ? S_scale + (size_t)i_nb * S_C : S_ptr), 0, aff ? S_C * 4 : 0, 0x00020000);
      __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc((void*)(aff ? S_shift + (size_t)i_nb * S_C : S_ptr), 0, aff ? S_C * 4 : 0, 0x00020000);
      const int o = ((cc.c0 + cg4) * 4) | dead;            // channels beyond the source's C (or a plain source: num_records 0) read 0
      psc = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r1, o, 0, 0));
      psh = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r2, o, 0, 0));
#pragma unroll
      for (int e = 0; e < 4; ++e) pcv[e] = ((cg4 + e) < cc.ck && !aff) ? 1.f : 0.f;
      pslope = aff ? (s1 ? sp_sl1 : sp_sl0) : 1.f;
      pmask = q_live ? i_mask : 0u;
    }
    const size_t sample_elems = (size_t)c.Di * c.Hi * c.Wi * S_cs;
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(S_ptr + (size_t)i_nb * sample_elems), 0, (int)(sample_elems * 4), 0x00020000);
    const int cofs = cc.c0 + cg4;
    const unsigned mk = q_live ? i_mask : 0u;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (j * NPART / NJ != part) continue;                          // (compile-time after unrolling: part and j are constants)
      // the address is formed unconditionally; an invalid task only sets bit 31 (beyond num_records: the load returns 0)
      const int off = (((i_base + (PCO[j * 256] & 0xfffff)) * S_cs + cofs) * 4) | (int)((((mk >> j) & 1u) ^ 1u) << 31);
      pv[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
    }
  };
  auto issue_patch = [&](bool live, const ConvChunk cc) {
    issue_prepare(live, cc);
#pragma unroll
    for (int part = 0; part < NPART; ++part) issue_loads(part);
  };
  auto store_patch = [&]() {                             // patch in flight (step gs) -> RAW[gs & 1], lazy InstanceNorm+LeakyReLU applied
    // a channel slot beyond the chunk's ck has scale = shift = 0 (a lazy source: the range-checked loads; a plain one: pcv = 0),
    // so whatever finite neighbour data its dwords hold becomes 0
    float sc[4], sh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { sc[e] = psc[e] + pcv[e]; sh[e] = psh[e]; }
    float* dst = lds + (gs & 1) * W_RAWF + rawst;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const bool ok = (pmask >> j) & 1u;
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = fmaf(pv[j][e], sc[e], sh[e]);
        o[e] = ok ? fmaxf(t, t * pslope) : 0.f;
      }
      if (j < NJ - 1 || tl + 256 * j < NTASK) *(f32x4*)(dst + j * 128 * WRP) = o;
    }
    ++gs;
  };

  // Issue priority.  The stager waves are the YOUNGER wave of every SIMD (waves 4-7) and lose every arbitration against the dense
  // VALU / LDS stream of the transformer wave: their chain of long-latency steps (wait for the patch, store it, request the next)
  // only started once the transformer had finished, and phase 1 lasted the SUM of the two (r3 stamps: 2 700 + 1 950 cycles).  With
  // the stagers prioritised their waits are filled by the transformer's instructions instead.
  if constexpr (STAGER) { if (WN_SPRIO) __builtin_amdgcn_s_setprio(WN_SPRIO); }
  if constexpr (STAGER) {
    if (!(WN_ABL & 1)) {
      issue_patch(true, P.chunk[0]);
      store_patch();
      issue_patch(G > 1, P.chunk[i_ch]);
    }
  }
  __syncthreads();

  unsigned long long ts_prev = 0, ts_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  auto TS = [&](int cat) {                               // time since the previous stamp is charged to `cat`
    if (WN_TS) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      ts_acc[cat] += t - ts_prev;
      ts_prev = t;
    }
  };
  if (WN_TS) ts_prev = __builtin_amdgcn_s_memtime();
  f32x16 acc[8];
  f32x4 fbs[10];                                         // weight fragments of the current step (see phase 1); [8..9]: transformers' ring
  if constexpr (STAGER) {
    if (WN_SRING && !(WN_ABL & 4)) {
      const int wq0 = (((ntile * P.nchunks + 0) * 64 + xi0) * 256 + lane * 4) * 4;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        fbs[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, wq0 + ((j >> 1) * 4 + (j & 1)) * 1024, 0, 0));
    }
  }
  int nb = 0, od0 = 0, oh0 = 0, ow0 = 0, sb = 0;
  for (int g = 0, ch = 0, k = 0; g < G; ++g) {
    if (ch == 0) {
      decode(lw + k * NWK, nb, od0, oh0, ow0, sb);
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    }
    // ---------------- phase 1: waves 0-3 transform step g, waves 4-7 store step g+1 and request step g+2 (possibly of the next tile)
    if constexpr (!STAGER) {
      // the first weight fragments of this step's MFMA phase are requested before the transform: their L2 latency is hidden
      // behind it instead of opening the MFMA phase
      if (!(WN_ABL & 4)) {
        const int wqo = (((ntile * P.nchunks + ch) * 64 + xi0) * 256 + lane * 4) * 4;
#pragma unroll
        for (int j = 0; j < WN_TPF; ++j)
          fbs[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, wqo + ((j >> 1) * 4 + (j & 1)) * 1024, 0, 0));
      }
      const float* rr = lds + (g & 1) * W_RAWF + rawrd;
      float d[4][4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) d[a][b][kk] = rr[((a * LH + b) * LW + kk) * WRP];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float x0 = d[a][b][0], x1 = d[a][b][1], x2 = d[a][b][2], x3 = d[a][b][3];
          d[a][b][0] = x0 - x2; d[a][b][1] = x1 + x2; d[a][b][2] = x2 - x1; d[a][b][3] = x1 - x3;
        }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const float x0 = d[a][0][kk], x1 = d[a][1][kk], x2 = d[a][2][kk], x3 = d[a][3][kk];
          d[a][0][kk] = x0 - x2; d[a][1][kk] = x1 + x2; d[a][2][kk] = x2 - x1; d[a][3][kk] = x1 - x3;
        }
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const float x0 = d[0][b][kk], x1 = d[1][b][kk], x2 = d[2][b][kk], x3 = d[3][b][kk];
          d[0][b][kk] = x0 - x2; d[1][b][kk] = x1 + x2; d[2][b][kk] = x2 - x1; d[3][b][kk] = x1 - x3;
        }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) V[((a * 4 + b) * 4 + kk) * 256 + tl] = d[a][b][kk];
    } else {
      // vmcnt completes IN ORDER: a weight-fragment load issued after the patch request cannot be waited for without waiting
      // for the whole patch (an HBM round trip at the start of every MFMA phase, with the other seven waves held at the next
      // barrier).  So this step's eight weight fragments are requested FIRST, the patch of step g+2 after them: the MFMA phase
      // then waits for loads that are older than the patch in flight and never for the patch itself.
      const ConvChunk ncc = P.chunk[i_ch];               // (scalar load: in flight during the wait and the store below)
      if (!(WN_ABL & 4) && !WN_SRING) {
        const int wqo = (((ntile * P.nchunks + ch) * 64 + xi0) * 256 + lane * 4) * 4;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          fbs[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, wqo + ((j >> 1) * 4 + (j & 1)) * 1024, 0, 0));
      }
      if (!(WN_ABL & 1)) {
        if (WN_TS) { asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); TS(9); }    // (timing build: arrival of the patch in flight)
        if (g + 1 < G) store_patch();                    // (LDS stores only)
        if (WN_TS) TS(10);
        // (interleaving these loads with the MFMAs of phase 2 was measured SLOWER, 1.148 vs 1.131 ms: a wave stalls ~130 cycles on
        // the issue of every gather — 16 distinct lines per instruction — and in phase 2 that stall delays its own MFMAs)
        issue_patch(g + 2 < G, ncc);
      }
    }
    TS(0);
    __syncthreads();
    TS(1);
    // ---------------- phase 2: 8 GEMMs per wave, K = 8 channels = 4 MFMAs each
    if constexpr (STAGER) {
      if (!(WN_ABL & 4)) {
        // WN_SRING: fragment j of the NEXT step replaces fragment j as soon as its MFMAs are issued (the patch request of phase 1 is
        // then older than every fragment load the MFMA phase waits for, and phase 1 does not open with eight loads per wave)
        const int chn = (ch + 1 == P.nchunks) ? 0 : ch + 1;
        const int wqn = ((((ntile * P.nchunks + chn) * 64 + xi0) * 256 + lane * 4) * 4) | ((g + 1 < G) ? 0 : (int)0x80000000);
        f32x4 fa[2];
        fa[0] = *(const f32x4*)(va);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (j + 1 < 8) fa[(j + 1) & 1] = *(const f32x4*)(va + (((j + 1) >> 1) * 4 + ((j + 1) & 1)) * 256);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[j & 1][e], fbs[j][e], acc[j], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (WN_SRING) fbs[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, wqn + ((j >> 1) * 4 + (j & 1)) * 1024, 0, 0));
        }
      }
    } else
    if (!(WN_ABL & 4)) {
      const int wqo = (((ntile * P.nchunks + ch) * 64 + xi0) * 256 + lane * 4) * 4;
      f32x4 fa[2];
      fa[0] = *(const f32x4*)(va);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (j + 1 < 8) fa[(j + 1) & 1] = *(const f32x4*)(va + (((j + 1) >> 1) * 4 + ((j + 1) & 1)) * 256);
        if (j + WN_TPF < 8) {                            // ring: fragment j + WN_TPF goes into the slot fragment j leaves after this step
          const int jn = j + WN_TPF;
          fbs[8 + (j & 1)] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, wqo + ((jn >> 1) * 4 + (jn & 1)) * 1024, 0, 0));
        }
        __builtin_amdgcn_sched_barrier(0);
        const f32x4 fbj = (j < WN_TPF) ? fbs[j] : fbs[8 + ((j - WN_TPF) & 1)];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[j & 1][e], fbj[e], acc[j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    TS(2);
    __syncthreads();
    TS(3);
    if (++ch < P.nchunks) continue;
    ch = 0; ++k;

    // ---------------- output transform of the finished tile (partials through the V region)
    if (WN_ABL & 8) { if (acc[0][0] == 1234.5f) c.out0[0] = acc[7][3] + acc[3][1]; continue; }
    const int co = ntile * 32 + li;
    const bool covalid = co < c.Cout;
    const float bv = (c.bias != nullptr && covalid) ? c.bias[co] : 0.f;
    const bool split = c.csplit < c.Cout;
    const bool use1 = split && co >= c.csplit;
    const int ocs = use1 ? c.ocs1 : c.ocs0;
    const int cofs = use1 ? co - c.csplit : co;
    const size_t out_sample = (size_t)c.Do * c.Ho * c.Wo;
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(c.out0 + (size_t)nb * out_sample * c.ocs0), 0,
                                                                  (int)(out_sample * c.ocs0 * 4), 0x00020000);
    __amdgpu_buffer_rsrc_t rd1 = rd;
    if (split) rd1 = __builtin_amdgcn_make_buffer_rsrc((void*)(c.out1 + (size_t)nb * out_sample * c.ocs1), 0,
                                                       (int)(out_sample * c.ocs1 * 4), 0x00020000);
    const int od = wave >> 2, oh = (wave >> 1) & 1, ow = wave & 1;
    const float sgn = od ? -1.f : 1.f;
    float* PL = V;                                       // [wave 8][r 8][q 4][lane 64] = 64 KiB per round
    float s1 = 0.f, s2 = 0.f;
    // Output addresses.  Accumulator row r of this wave is the output voxel (xd0 + 2 (r>>3), xh0 + 2 ((r>>2)&1), xw0 + 2 (r&3)) with
    // xw0 = ow0 + ow + 8 lhalf the only lane-dependent coordinate: the four lane offsets (k = r & 3, masked where the column or the
    // channel is outside) are computed once per tile, the (d, h) part of a row is a SCALAR offset of the store, and a row outside
    // the tensor stores through an empty descriptor (scalar select).  The output transform is bound by its vector instructions
    // (~1 000 per tile and wave, half of the kernel's, profiles/r02_pmc_conv_wino8p.txt); the per-output address arithmetic
    // (two integer multiplications, four compares, shifts) was 35 of its 45 per output.
    const int xd0 = od0 + od, xh0 = oh0 + oh, xw0 = ow0 + ow + 8 * lhalf;
    int vo0[4], vo1[4];                                  // byte offsets into destination 0 / 1 (bit 31: this lane does not store there)
    unsigned lm[4];                                      // all ones where the lane's output of column k exists
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool okl = covalid && (xw0 + 2 * k < c.Wo);
      const int vox = (xd0 * c.Ho + xh0) * c.Wo + xw0 + 2 * k;
      vo0[k] = (okl && !use1) ? (vox * c.ocs0 + co) * 4 : (int)0x80000000;
      vo1[k] = (okl && use1) ? (vox * c.ocs1 + (co - c.csplit)) * 4 : (int)0x80000000;
      lm[k] = okl ? 0xffffffffu : 0u;
    }
    __amdgpu_buffer_rsrc_t rnull = __builtin_amdgcn_make_buffer_rsrc((void*)c.out0, 0, 0, 0x00020000);      // num_records = 0
    // Fused first pass of the InstanceNorm backward that consumes this gradient (mt_bwd_stats_t): the lane's channel constants and
    // the offsets of the layer's raw forward output y at the lane's four columns
    const bool bst = BSTK && c.bstats.y != nullptr;       // (BSTK: the kernel instance that carries the statistics code)
    const int yc = co - c.bstats.c0;
    const bool bch = bst && covalid && yc >= 0 && yc < c.bstats.C;
    float b_mu = 0.f, b_rs = 0.f, b_ga = 1.f, b_be = 0.f;
    int vy[4] = {(int)0x80000000, (int)0x80000000, (int)0x80000000, (int)0x80000000};
    __amdgpu_buffer_rsrc_t ry = rnull;
    if (bst) {
      if (bch) {
        b_mu = c.bstats.mean[(size_t)nb * c.bstats.C + yc]; b_rs = c.bstats.rstd[(size_t)nb * c.bstats.C + yc];
        if (c.bstats.gamma != nullptr) b_ga = c.bstats.gamma[yc];
        if (c.bstats.beta != nullptr) b_be = c.bstats.beta[yc];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (xw0 + 2 * k < c.Wo) vy[k] = (((xd0 * c.Ho + xh0) * c.Wo + xw0 + 2 * k) * c.bstats.ycs + yc) * 4;
      }
      ry = __builtin_amdgcn_make_buffer_rsrc((void*)(c.bstats.y + (size_t)nb * out_sample * c.bstats.ycs), 0,
                                             (int)(out_sample * c.bstats.ycs * 4), 0x00020000);
    }
    // (BST) the layer's forward output at the lane's sixteen outputs: requested now, consumed after the exchange rounds' barriers
    float yr16[BSTK ? 16 : 1];
    if constexpr (BSTK) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = r & 3, dh = 2 * ((r >> 2) & 1), dd = 2 * (r >> 3);
        const bool rok = (xd0 + dd < c.Do) && (xh0 + dh < c.Ho);
        yr16[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rok ? ry : rnull, vy[k], (dd * c.Ho + dh) * c.Wo * 4 * c.bstats.ycs, 0));
      }
    }
#pragma unroll
    for (int round = 0; round < 2; ++round) {
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const int r = round * 8 + rr;
        float t[2][2];                                   // [oh][cl]: contraction over b
#pragma unroll
        for (int cl = 0; cl < 2; ++cl) {
          const float q0 = acc[0 + cl][r], q1 = acc[2 + cl][r], q2 = acc[4 + cl][r], q3 = acc[6 + cl][r];
          t[0][cl] = q0 + q1 + q2;
          t[1][cl] = q1 - q2 - q3;
        }
#pragma unroll
        for (int o2 = 0; o2 < 2; ++o2) {
          const float w0 = wh ? t[o2][0] : (t[o2][0] + t[o2][1]);              // ow = 0: c0 + c1 | c2
          const float w1 = wh ? (-t[o2][0] - t[o2][1]) : t[o2][1];             // ow = 1: c1 | -c2 - c3
          PL[((wave * 8 + rr) * 4 + o2 * 2 + 0) * 64 + lane] = w0;
          PL[((wave * 8 + rr) * 4 + o2 * 2 + 1) * 64 + lane] = w1;
        }
      }
      TS(4);
      __syncthreads();
      TS(5);
      // straight-line code per (accumulate, split) case: with run-time branches on those flags every output was its own chain
      // of basic blocks — LDS read, wait, add, store, eight times per round — instead of one batch of reads
      auto stage2 = [&](auto acc_c, auto split_c, auto bst_c) {
        constexpr bool ACC = decltype(acc_c)::value, SPLIT = decltype(split_c)::value, BST = decltype(bst_c)::value;
        const int q = oh * 2 + ow;
        float yv[8];
        const float* yraw = yr16 + (BSTK ? round * 8 : 0);    // (BST) requested before the first exchange round
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
          auto part = [&](int a) { return PL[(((a * 2) * 8 + rr) * 4 + q) * 64 + lane] + PL[(((a * 2 + 1) * 8 + rr) * 4 + q) * 64 + lane]; };
          const float pa = part(od ? 3 : 0), p1 = part(1), p2 = part(2);
          yv[rr] = fmaf(sgn, pa + p2, p1) + bv;
        }
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
          const int r = round * 8 + rr;
          const int k = r & 3, dh = 2 * ((r >> 2) & 1), dd = 2 * (r >> 3);              // (compile-time)
          const bool rok = (xd0 + dd < c.Do) && (xh0 + dh < c.Ho);                      // wave-uniform
          const int srow = (dd * c.Ho + dh) * c.Wo * 4;                                 // scalar: bytes per channel-stride unit
          const __amdgpu_buffer_rsrc_t r0 = rok ? rd : rnull;
          const __amdgpu_buffer_rsrc_t r1 = rok ? rd1 : rnull;
          float y = yv[rr];
          if constexpr (ACC) {
            y += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r0, vo0[k], srow * c.ocs0, 0));
            if constexpr (SPLIT) y += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r1, vo1[k], srow * c.ocs1, 0));
          }
          if (!(WN_ABL & 16) || y == 1234.5f) {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y), r0, vo0[k], srow * c.ocs0, 0);
            if constexpr (SPLIT) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y), r1, vo1[k], srow * c.ocs1, 0);
          }
          const float m = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, y) & lm[k] & (rok ? 0xffffffffu : 0u));
          if constexpr (BST) {
            // m = the finished gradient g of lrelu(IN(yraw)) at this voxel (0 where the lane has no output): dz = g lrelu'(z)
            const float zh = (yraw[rr] - b_mu) * b_rs;
            const float z = fmaf(zh, b_ga, b_be);
            const float mb = bch ? m : 0.f;                  // channels of the other destination: no statistics
            const float dz = z > 0.f ? mb : mb * c.bstats.slope;
            s1 += dz; s2 = fmaf(dz, zh, s2);
          } else {
            s1 += m; s2 = fmaf(m, m, s2);
          }
        }
      };
      using bst_t = std::integral_constant<bool, BSTK>;
      if (!c.accumulate && !split) stage2(std::false_type{}, std::false_type{}, bst_t{});
      else if (!c.accumulate) stage2(std::false_type{}, std::true_type{}, bst_t{});
      else if (!split) stage2(std::true_type{}, std::false_type{}, bst_t{});
      else stage2(std::true_type{}, std::true_type{}, bst_t{});
      TS(6);
      __syncthreads();
      TS(7);
    }
    if (c.stats_part != nullptr) {
      s1 += __shfl_xor(s1, 32, 64);
      s2 += __shfl_xor(s2, 32, 64);
      if (lhalf == 0) { PL[(wave * 32 + li) * 2] = s1; PL[(wave * 32 + li) * 2 + 1] = s2; }
      __syncthreads();
      if (tid < 32 && (ntile * 32 + tid) < c.Cout) {
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) { t1 += PL[(w * 32 + tid) * 2]; t2 += PL[(w * 32 + tid) * 2 + 1]; }
        float* sp = c.stats_part + ((size_t)((size_t)nb * P.nsb + sb) * c.Cout + ntile * 32 + tid) * 2;
        sp[0] = t1; sp[1] = t2;
      }
      __syncthreads();                                   // the next tile's transform overwrites V
    }
    TS(8);
  }
  if (WN_TS && lane == 0 && blockIdx.y == 0) {
    unsigned long long* o = (unsigned long long*)c.out1 + ((size_t)blockIdx.x * 8 + wave) * 16;
#pragma unroll
    for (int q = 0; q < 12; ++q) o[q] = ts_acc[q];
  }
}

__global__ __launch_bounds__(512) void conv_wino8p_kernel(const ConvKParams P) {
  if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >= 4) wino8p_body<true, false>(P);
  else wino8p_body<false, false>(P);
}
// the same kernel with the fused InstanceNorm-backward statistics in its epilogue (mt_bwd_stats_t): a separate instance, so that the
// launches without statistics do not carry its registers
__global__ __launch_bounds__(512) void conv_wino8pb_kernel(const ConvKParams P) {
  if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >= 4) wino8p_body<true, true>(P);
  else wino8p_body<false, true>(P);
}
