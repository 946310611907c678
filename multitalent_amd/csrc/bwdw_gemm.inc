// bwdw_gemm.inc — backward-weight of the LOW-RESOLUTION convolutions in mixed precision (mt_conv3d_t.mma == 1) as im2col + one GEMM
// with bf16 products (included by conv_bwdw.hip).
//
// dW[tap][ci][co] = sum over output voxels o of act(X)[o*S + tap - P][ci] * dY[o][co]  (autograd of nn.Conv3d weights; reference ops
// conv_blocks.py:116-213, generic_UNet.py:57,67) is a GEMM whose contraction index is the VOXEL: C[m = (tap, ci)][n = co] = A[m][k] B[n][k].
// A bf16 MFMA wants both operands with the contraction index fastest — the opposite of NDHWC — which is why the full-resolution kernels
// stay in the Winograd domain (bwdw_bf16.inc).  At the low-resolution stages (<= 6x12x12 voxels, 320 channels) the tensors are small
// enough (0.5 MB) to be REWRITTEN: one kernel builds A = im2col(act(X)) as [tap][ci][K] bf16 (zero rows where a tap leaves the volume,
// K = all output voxels of the batch, padded to 32), a second transposes dY to B = [co][K] bf16, and the GEMM reads both as 16-byte
// fragments straight from L2.  The fp32 marching kernel these launches took (conv_bwdw_march_kernel, W <= 16) spends 160 us on 9.5 GFLOP;
// this path: ~30 us.  Deterministic: every output element is one wave's ordered sum.
#define BG_KPAD 32

struct BgParams {
  mt_conv3d_t c;
  mt_src_t y;
  unsigned short* A;      // [Cin][ntaps][Kp]: row m = ci * ntaps + tap (the torch weight layout's order within an output channel)
  unsigned short* B;      // [Cout][Kp]
  int Kp, Vo;             // padded / real contraction length per launch (N * Do * Ho * Wo)
  float* dw; long s_ci, s_co, s_kd, s_kh, s_kw; int accumulate;
};

// A[tap][ci][k]: one workgroup = (tap, 64 voxels, 64 channels) through an LDS tile: reads run along channels, writes along voxels
template <int XS>
__global__ __launch_bounds__(256) void bwdw_im2col_kernel(const BgParams P) {
  __shared__ unsigned short tile[64][66];
  const mt_conv3d_t& c = P.c;
  const int tap = blockIdx.z, k0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int kw = tap % c.KW, kh = (tap / c.KW) % c.KH, kd = tap / (c.KW * c.KH);
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;           // tx: channel (read) / voxel (write)
  // which source holds channel c0 + tx (torch.cat of two sources)
  const int C0 = c.src[0].C;
  const int ci = c0 + tx;
  const bool second = c.nsrc == 2 && ci >= C0;
  const mt_src_t& S = second ? c.src[1] : c.src[0];
  const int cl = second ? ci - C0 : ci;
  const bool cv = ci < c.Cin;
  const bool aff = S.scale != nullptr;
  const long vper = (long)c.Do * c.Ho * c.Wo;
  const int wv = __builtin_amdgcn_readfirstlane(ty);
  for (int r = wv; r < 64; r += 4) {
    // the row's voxel is the same for the whole wave: its decode (integer divisions by run-time values, ~40 instructions each on the
    // vector ALU) runs on the scalar unit
    const int k = __builtin_amdgcn_readfirstlane(k0 + r);
    float v = 0.f;
    if (k < P.Vo) {
      const int n = (int)(k / vper);
      int o = k - n * (int)vper;
      const int ow = o % c.Wo; o /= c.Wo;
      const int oh = o % c.Ho, od = o / c.Ho;
      const int ud = od * c.SD + kd - c.PD, uh = oh * c.SH + kh - c.PH, uw = ow * c.SW + kw - c.PW;
      if (cv && (unsigned)ud < (unsigned)c.Di && (unsigned)uh < (unsigned)c.Hi && (unsigned)uw < (unsigned)c.Wi) {
        const size_t e = ((((size_t)n * c.Di + ud) * c.Hi + uh) * c.Wi + uw) * S.cs + cl;
        v = mt_ld<XS>(S.ptr, e);
        if (aff) v = mt_lrelu(fmaf(v, S.scale[(size_t)n * S.C + cl], S.shift[(size_t)n * S.C + cl]), S.slope);
      }
    }
    tile[r][tx] = (unsigned short)(mt_pk_bf16(v, v) & 0xffffu);
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {                                 // r: channel, tx: voxel
    const int cc = c0 + r, k = k0 + tx;
    if (cc < c.Cin && k < P.Kp) P.A[((size_t)cc * gridDim.z + tap) * P.Kp + k] = tile[tx][r];       // row m = ci * ntaps + tap
  }
}
// B[co][k] = dY[k][co]
template <int YS>
__global__ __launch_bounds__(256) void bwdw_ytrans_kernel(const BgParams P) {
  __shared__ unsigned short tile[64][66];
  const int k0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const mt_src_t& Y = P.y;
  const bool aff = Y.scale != nullptr;
  const long vper = (long)P.c.Do * P.c.Ho * P.c.Wo;
  for (int r = ty; r < 64; r += 4) {
    const int k = k0 + r, co = c0 + tx;
    float v = 0.f;
    if (k < P.Vo && co < P.c.Cout) {
      v = mt_ld<YS>(Y.ptr, (size_t)k * Y.cs + co);
      if (aff) { const int n = (int)(k / vper); v = mt_lrelu(fmaf(v, Y.scale[(size_t)n * Y.C + co], Y.shift[(size_t)n * Y.C + co]), Y.slope); }
    }
    tile[r][tx] = (unsigned short)(mt_pk_bf16(v, v) & 0xffffu);
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int co = c0 + r, k = k0 + tx;
    if (co < P.c.Cout && k < P.Kp) P.B[(size_t)co * P.Kp + k] = tile[tx][r];
  }
}
// C[co][m] = sum_k B[co][k] A[m][k]: a wave owns a 64 (co) x 32 (m) output block — the A fragment of a k-step feeds two MFMAs —,
// fragments come as 16-byte loads straight from global memory (both operands stay in L2: A is re-read by the Cout / 64 row blocks),
// eight k-steps in flight.  The m index is the MFMA's COLUMN (= lane): consecutive lanes store consecutive weights of one output channel
// (128-byte runs in the torch layout [co][ci][kd][kh][kw]).
typedef __bf16 bg_bf16x8 __attribute__((ext_vector_type(8)));
__global__ __launch_bounds__(256) void bwdw_gemm_kernel(const BgParams P) {
  const mt_conv3d_t& c = P.c;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int ntaps = c.KD * c.KH * c.KW;
  const int M = ntaps * c.Cin;
  const int mblk = (blockIdx.x * 4 + wave) * 32, nblk = blockIdx.y * 64;
  if (mblk >= M) return;
  const int m = mblk + li;
  const int am = m < M ? m : M - 1;                                  // (columns beyond M repeat the last one; their results are not stored)
  const int bn0 = nblk + li < c.Cout ? nblk + li : c.Cout - 1, bn1 = nblk + 32 + li < c.Cout ? nblk + 32 + li : c.Cout - 1;
  const uint4* ap = (const uint4*)(P.A + (size_t)am * P.Kp) + lh;    // k-block lh of every 16: 8 consecutive k = one uint4
  const uint4* bp0 = (const uint4*)(P.B + (size_t)bn0 * P.Kp) + lh;
  const uint4* bp1 = (const uint4*)(P.B + (size_t)bn1 * P.Kp) + lh;
  f32x16 acc0, acc1;
#pragma unroll
  for (int j = 0; j < 16; ++j) { acc0[j] = 0.f; acc1[j] = 0.f; }
  const int nk = P.Kp / 16;
  constexpr int PF = 8;
  uint4 ra[PF], rb0[PF], rb1[PF];
#pragma unroll
  for (int s = 0; s < PF; ++s) {
    const int kk = s < nk ? s : nk - 1;
    ra[s] = ap[kk * 2]; rb0[s] = bp0[kk * 2]; rb1[s] = bp1[kk * 2];
  }
  for (int k = 0; k < nk; k += PF) {
#pragma unroll
    for (int s = 0; s < PF; ++s) {
      const uint4 a = ra[s], b0 = rb0[s], b1 = rb1[s];
      const int kn = k + s + PF;
      const int kk = kn < nk ? kn : nk - 1;
      ra[s] = ap[kk * 2]; rb0[s] = bp0[kk * 2]; rb1[s] = bp1[kk * 2];
      if (k + s < nk) {                                               // rows = output channels (dY^T), columns = (ci, tap)
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bg_bf16x8, b0), __builtin_bit_cast(bg_bf16x8, a), acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bg_bf16x8, b1), __builtin_bit_cast(bg_bf16x8, a), acc1, 0, 0, 0);
      }
    }
  }
  if (m >= M) return;
  const int ci = m / ntaps, tap = m - ci * ntaps;
  const int kw = tap % c.KW, kh = (tap / c.KW) % c.KH, kd = tap / (c.KW * c.KH);
  float* ob = P.dw + (long)ci * P.s_ci + kd * P.s_kd + kh * P.s_kh + kw * P.s_kw;
  // C layout: lane (column li, row group lh): rows (j & 3) + 8 * (j >> 2) + 4 * lh
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int co = nblk + 32 * t + (j & 3) + 8 * (j >> 2) + 4 * lh;
      if (co >= c.Cout) continue;
      float* o = ob + (long)co * P.s_co;
      const float v = t ? acc1[j] : acc0[j];
      *o = P.accumulate ? *o + v : v;
    }
}

// eligibility: mixed precision, stride-1 3x3x3 / 1x3x3 convolutions whose output rows are too short for the Winograd marching kernels
// (W <= 16), contraction and operands small enough to stay in L2 (A <= 96 MB)
static bool bwdw_use_gemm(const mt_conv3d_t* p, const mt_src_t* y) {
  if (p->mma != 1 || y == nullptr) return false;
  if (!(p->dilD == 1 && p->dilH == 1 && p->dilW == 1 && p->SD == 1 && p->SH == 1 && p->SW == 1 && p->KH == 3 && p->KW == 3 && (p->KD == 3 || p->KD == 1))) return false;
  if (p->Wo > 16 || p->Cin < 16 || p->Cout < 16) return false;
  const double V = (double)p->N * p->Do * p->Ho * p->Wo;
  const double abytes = (double)p->KD * 9.0 * p->Cin * (V + BG_KPAD) * 2.0;
  return V >= 64 && abytes <= 96.0 * 1024 * 1024;
}
static size_t bwdw_gemm_workspace(const mt_conv3d_t* p) {
  const long V = (long)p->N * p->Do * p->Ho * p->Wo;
  const long Kp = (V + BG_KPAD - 1) / BG_KPAD * BG_KPAD;
  return ((size_t)p->KD * p->KH * p->KW * p->Cin + (size_t)p->Cout) * Kp * 2 + 256;
}
static int launch_bwdw_gemm(const mt_conv3d_t* p, const mt_src_t* ysrc, float* dw, long s_ci, long s_co, long s_kd, long s_kh, long s_kw,
                            int accumulate, void* ws, size_t ws_bytes, hipStream_t st) {
  BgParams P;
  P.c = *p;
  if (P.c.nsrc == 1) { P.c.src[1] = P.c.src[0]; P.c.src[1].C = 0; }
  P.y = *ysrc;
  P.Vo = (int)((long)p->N * p->Do * p->Ho * p->Wo);
  P.Kp = (P.Vo + BG_KPAD - 1) / BG_KPAD * BG_KPAD;
  const int ntaps = p->KD * p->KH * p->KW;
  if (ws == nullptr || ws_bytes < bwdw_gemm_workspace(p)) { mt_set_error("bwd_weight (gemm): workspace %zu < %zu", ws_bytes, bwdw_gemm_workspace(p)); return MT_EWORKSPACE; }
  P.A = (unsigned short*)(((uintptr_t)ws + 127) & ~(uintptr_t)127);
  P.B = P.A + (size_t)ntaps * p->Cin * P.Kp;
  P.dw = dw; P.s_ci = s_ci; P.s_co = s_co; P.s_kd = s_kd; P.s_kh = s_kh; P.s_kw = s_kw; P.accumulate = accumulate;
  const int xs = conv_src_dtype(p);
  const dim3 gi((unsigned)mt_cdiv(P.Kp, 64), (unsigned)mt_cdiv(p->Cin, 64), (unsigned)ntaps);       // (gridDim.z = ntaps: used by the kernel)
  if (xs == MT_F16) hipLaunchKernelGGL((bwdw_im2col_kernel<MT_F16>), gi, dim3(256), 0, st, P);
  else if (xs == MT_BF16) hipLaunchKernelGGL((bwdw_im2col_kernel<MT_BF16>), gi, dim3(256), 0, st, P);
  else hipLaunchKernelGGL((bwdw_im2col_kernel<MT_F32>), gi, dim3(256), 0, st, P);
  const dim3 gy((unsigned)mt_cdiv(P.Kp, 64), (unsigned)mt_cdiv(p->Cout, 64), 1);
  if (ysrc->dtype == MT_BF16) hipLaunchKernelGGL((bwdw_ytrans_kernel<MT_BF16>), gy, dim3(256), 0, st, P);
  else if (ysrc->dtype == MT_F16) hipLaunchKernelGGL((bwdw_ytrans_kernel<MT_F16>), gy, dim3(256), 0, st, P);
  else hipLaunchKernelGGL((bwdw_ytrans_kernel<MT_F32>), gy, dim3(256), 0, st, P);
  const int M = ntaps * p->Cin;
  const dim3 gg((unsigned)mt_cdiv(mt_cdiv(M, 32), 4), (unsigned)mt_cdiv(p->Cout, 64), 1);
  hipLaunchKernelGGL(bwdw_gemm_kernel, gg, dim3(256), 0, st, P);
  MT_CHECK_LAUNCH("bwdw_gemm");
  return MT_OK;
}
