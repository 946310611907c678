// pw_common.h — shared by pointwise.hip, head_infer.hip and head_bwd.hip: the kernel parameters of mt_pointwise_fwd, the K-chunk constants
// and the load / channel-pair helpers of the pointwise kernels.
#pragma once
#include "mt_common.h"

struct PwKParams {
  mt_pointwise_t c;
  int ntaps, nchunks, nsb;
  long Vb;
  int wide;      // pw_fast_kernel: transposed-conv outputs leave through LDS as 16-byte stores (see the wide epilogue)
};

#define PW_MAXC 1024   // largest Cin (rounded up to a chunk) whose scale/shift fit the LDS copy
#define PW_CK 16   // channels per K chunk (packed weight layout 1, ck = 16 — the conv kernels' layout)

// ---- storage types (mt_src_t.dtype, odtype; mt_common.h).  The matrix arithmetic of the kernels that include this header is fp32 whatever the storage type (the M16 forms apart): a 16-bit source
// is widened on load (8 channels = ONE 16-byte load instead of two), a 16-bit destination rounded on store.
// 16-bit output of a 32x32 accumulator tile as channel-pair dwords: the lanes of a channel pair (li even, li odd) trade one value per
// two accumulator rows, so the EVEN lane holds both channels of voxel row j and the ODD lane both channels of row j + 1.
__device__ __forceinline__ void pw_pair_exchange(float vj, float vj1, bool odd, float& a, float& b) {
  const float send = odd ? vj : vj1;
  const float recv = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send), 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, true));
  a = odd ? recv : vj;
  b = odd ? vj1 : recv;
}
__device__ __forceinline__ float pw_pair_combine(float s0, float s1, bool odd) {       // per-channel total of sums kept per pair member
  const float t0 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s0), 0xB1, 0xF, 0xF, true));
  const float t1 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s1), 0xB1, 0xF, 0xF, true));
  return odd ? s1 + t1 : s0 + t0;
}
// 8 consecutive channels of one voxel (byte offset o inside the buffer): two 16-byte loads (fp32) or one (16-bit)
template <int XS>
__device__ __forceinline__ void pw_load8(__amdgpu_buffer_rsrc_t r, int o, float (&x)[8]) {
  if constexpr (XS == MT_F32) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const f32x4 t = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, o + g * 16, 0, 0));
      x[4 * g] = t[0]; x[4 * g + 1] = t[1]; x[4 * g + 2] = t[2]; x[4 * g + 3] = t[3];
    }
  } else {
    const uint4 t = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, o, 0, 0));
    x[0] = mt_lo16<XS>(t.x); x[1] = mt_hi16<XS>(t.x); x[2] = mt_lo16<XS>(t.y); x[3] = mt_hi16<XS>(t.y);
    x[4] = mt_lo16<XS>(t.z); x[5] = mt_hi16<XS>(t.z); x[6] = mt_lo16<XS>(t.w); x[7] = mt_hi16<XS>(t.w);
  }
}
