// Parameter blocks and host helpers shared by the convolution translation units: conv_lds.hip (forward, backward-data: one dispatch decision each, conv_resolve / bwdd_resolve; weight packing),
// conv_bwdw.hip (backward-weight: plans, the one dispatch decision, the reduce), and the single-family units bwdw_tr16.hip and conv_x16.hip,
// whose launchers are declared here and whose dispatch stays with the caller.
#pragma once
#include "mt_common.h"

struct ConvChunk { short src, c0, ck, cglob; };

// Split the concatenated input channels (C0 | C1) into chunks of <= ck channels that never straddle
// the two sources.  Shared by packing and kernels so the packed order always matches.
static inline int mt_build_chunks(int C0, int C1, int ck, ConvChunk* out) {
  int n = 0;
  const int Cs[2] = {C0, C1};
  int cglob = 0;
  for (int s = 0; s < 2; ++s) {
    for (int c0 = 0; c0 < Cs[s]; c0 += ck) {
      if (n >= MT_MAX_CHUNKS) return -1;
      const int k = (Cs[s] - c0 < ck) ? (Cs[s] - c0) : ck;
      out[n].src = (short)s; out[n].c0 = (short)c0; out[n].ck = (short)k; out[n].cglob = (short)(cglob + c0);
      ++n;
    }
    cglob += Cs[s];
  }
  return n;
}
// 2 when every source can be staged as channel pairs (one 8 / 4-byte load: even channel count and stride, aligned base), else 1
static inline int conv_fast_vec(const mt_conv3d_t* p) {
  for (int i = 0; i < p->nsrc; ++i) {
    const mt_src_t& s = p->src[i];
    if ((s.cs & 1) || (s.C & 1) || (((uintptr_t)s.ptr) & (mt_is16(s.dtype) ? 3 : 7))) return 1;   // a channel pair = one 8 / 4-byte load
  }
  return 2;
}
// storage type of a problem's sources: their common type (-1: mixed or unknown)
static inline int conv_src_dtype(const mt_conv3d_t* p) {
  const int d = p->src[0].dtype;
  if (p->nsrc == 2 && p->src[1].dtype != d) return -1;
  return mt_dtype_ok(d) ? d : -1;
}
// a 2-bit MT_SEL_* field of p->select: 0 off, 1 the library's policy, 2 forced
static inline int mt_sel3(const mt_conv3d_t* p, int shift) { const unsigned v = MT_SEL_GET(p->select, shift); return v == MT_SEL_OFF ? 0 : v == MT_SEL_FORCE ? 2 : 1; }

struct ConvKParams {
  mt_conv3d_t c;
  int tilesD, tilesH, tilesW, nsb;
  int nchunks, ntaps;
  int dbg;       // 0 (timing ablations of conv_fwd_kernel when set by hand: 1 skip staging, 2 skip weight loads, 4 skip epilogue, 8 skip MFMA, 16 stamps)
  int stagger;   // 0 (one-time start delay per residency slot of the first block wave: measured without effect, rounds 3 and 6)
  ConvChunk chunk[MT_MAX_CHUNKS];
};

#define BW_CK 16
struct BwdWParams {
  mt_conv3d_t c;      // X geometry (src), conv geometry; Do/Ho/Wo = Y dims
  mt_src_t y;         // Y source (C = Cout)
  int TD, TH, TW;     // spatial tile (TW % 4 == 0)
  int tilesD, tilesH, tilesW, ntiles_total;
  int nchunks, ntaps, ncot, nsg;
  int nsg_cap, nunits, nseg, dseg;   // marching kernel: units = (sample, h-tile, w-tile, D segment of dseg planes)
  int cw;             // conv_bwdw_fast_kernel: cout tiles per workgroup (1 | 2 | 4; grid.y = ceil(ncot / cw))
  float* part;        // [chunk][cot][sg][tap][16][32]
  ConvChunk chunk[MT_MAX_CHUNKS];
};

typedef __bf16 bwb_bf16x8 __attribute__((ext_vector_type(8)));

// bwdw_tr16.hip: direct bf16 backward-weight of 3x3x3 (KD = 3) / 1x3x3 (KD = 1) stride-1 convolutions fed by LDS transpose reads
int mt_launch_bwdw_tr16(const BwdWParams& P, int KD, int xdt, hipStream_t st);

// conv_x16.hip: persistent stride-1 3x3x3 (KD = 3) / 1x3x3 (KD = 1) convolution with ONE 16-bit storage type on all operands (fp16 forward,
// bf16 backward-data); weights in pack layout 4 / 3; items = (spatial 4x4x32 tile, 32-channel cout tile), nwg persistent workgroups
struct X16Params {
  mt_conv3d_t c;
  int tilesD, tilesH, tilesW, nsb;
  int nchunks, ncot, nitems, nwg;
  int npairs;                         // chunk pairs: two consecutive 16-channel chunks of one source (64 bytes of a voxel), or a single chunk (-1)
  short pair[MT_MAX_CHUNKS][2];
  ConvChunk chunk[MT_MAX_CHUNKS];
};
int mt_conv_x16_workgroups(int nitems);
int mt_launch_conv_x16(const X16Params& P, int KD, int dt, hipStream_t st);
