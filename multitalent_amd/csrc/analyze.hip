// The dataset fingerprint on the device (experiment_planning/DatasetAnalyzer.py of the reference, :161-224, and the np.unique of
// preprocessing/cropping.py:146 and DatasetAnalyzer.py:83).
//   mt_fg_sample_count / _gather   data[c][seg > 0][::stride] for all channels at once: an ordered compaction built like
//                                  mt_label_locations (units of MT_PP_UNIT voxels, one wave each, ballot ranks on a running counter,
//                                  exclusive scan over the units), of which only every stride-th element is ever written;
//   mt_label_presence              np.unique of an integer label map as a bitmap over -1..1022.
// All of them stream their input (HBM-bound) and use integer counts and integer atomics only: results are bit-identical from run to
// run, whatever the block scheduling.
#include "stream_common.h"

#define AN_THREADS 256
#define AN_WAVES (AN_THREADS / MT_WAVE)
#define AN_MAX_CHANNELS 16

// ---- ordered strided foreground sampling -------------------------------------------------------------------------------------
// One wave per unit: the number of voxels with seg > 0 (a float comparison: -1, 0 and NaN are not selected).
__global__ __launch_bounds__(AN_THREADS) void fg_count_kernel(const float* __restrict__ seg, long V, long nunits, int32_t* __restrict__ off) {
  const int lane = threadIdx.x % MT_WAVE;
  for (long unit = (long)blockIdx.x * AN_WAVES + threadIdx.x / MT_WAVE; unit < nunits; unit += (long)gridDim.x * AN_WAVES) {
    const long v0 = unit * MT_PP_UNIT, vend = mt_unit_end(v0, V);
    const long nquad = (vend - v0) / 4;
    int cnt = 0;
#pragma unroll 4
    for (long q = lane; q < nquad; q += MT_WAVE) {
      const mt_f4 s = *(const mt_f4*)(seg + v0 + 4 * q);
      cnt += (s.x > 0.f) + (s.y > 0.f) + (s.z > 0.f) + (s.w > 0.f);
    }
    for (long v = v0 + 4 * nquad + lane; v < vend; v += MT_WAVE) cnt += seg[v] > 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, MT_WAVE);
    if (lane == 0) off[unit] = cnt;
  }
}

// One block: counts of the units -> exclusive offsets in place, total -> *count.
__global__ __launch_bounds__(MT_SCAN_THREADS) void fg_scan_kernel(int32_t* __restrict__ off, long nunits, int64_t* __restrict__ count) {
  const int64_t total = mt_scan_units(off, nunits);
  if (threadIdx.x == 0) *count = total;
}

struct FgParams {
  const uint32_t* data; const float* seg; long V, nunits; int C; uint32_t stride;
  const int32_t* off; uint32_t* out; long out_cs; unsigned long long* nan;
};

// One wave per unit, 64 voxels a round in order: rank = offset of the unit + selected voxels of the earlier rounds + selected lower
// lanes.  A voxel whose rank is a multiple of the stride is copied, all channels, as a bit pattern.
__global__ __launch_bounds__(AN_THREADS) void fg_gather_kernel(const FgParams P) {
  const int lane = threadIdx.x % MT_WAVE;
  const uint64_t lower = (1ull << lane) - 1ull;
  for (long unit = (long)blockIdx.x * AN_WAVES + threadIdx.x / MT_WAVE; unit < P.nunits; unit += (long)gridDim.x * AN_WAVES) {
    const long v0 = unit * MT_PP_UNIT, vend = mt_unit_end(v0, P.V);
    uint32_t run = (uint32_t)P.off[unit];
    for (long vb = v0; vb < vend; vb += 4 * MT_WAVE) {
      float f[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {                          // four independent loads in flight, then four ordered rounds
        const long v = vb + r * MT_WAVE + lane;
        f[r] = v < vend ? P.seg[v] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long v = vb + r * MT_WAVE + lane;
        const bool sel = f[r] > 0.f;
        const uint64_t m = __ballot(sel);
        if (sel) {
          const uint32_t rank = run + (uint32_t)__popcll(m & lower);
          const uint32_t j = rank / P.stride;
          if (j * P.stride == rank && (long)j < P.out_cs) {
            for (int c = 0; c < P.C; ++c) {
              const uint32_t bits = P.data[(size_t)c * P.V + v];
              P.out[(size_t)c * P.out_cs + j] = bits;
              if ((bits & 0x7fffffffu) > 0x7f800000u) atomicAdd(&P.nan[c], 1ull);
            }
          }
        }
        run += (uint32_t)__popcll(m);
      }
    }
  }
}

extern "C" size_t mt_fg_sample_workspace(long V) {
  if (V < 1) return 0;
  return (((size_t)mt_units(V) * sizeof(int32_t)) + 7) & ~(size_t)7;
}

static int fg_args(const char* who, const float* seg, long V, const void* ws, size_t ws_bytes) {
  MT_REQUIRE(seg && ws, "%s: null pointer", who);
  MT_REQUIRE(V > 0, "%s: bad voxel count %ld", who, V);
  MT_REQUIRE(V <= (long)INT32_MAX, "%s: %ld voxels exceed the int32 index range", who, V);
  MT_REQUIRE(((uintptr_t)seg & 3) == 0 && ((uintptr_t)ws & 7) == 0, "%s: misaligned pointer", who);
  MT_REQUIRE_WORKSPACE(who, ws_bytes, mt_fg_sample_workspace(V));
  return MT_OK;
}

extern "C" int mt_fg_sample_count(const float* seg, long V, int64_t* count, void* ws, size_t ws_bytes, mt_stream_t stream) {
  const int rc = fg_args("fg_sample_count", seg, V, ws, ws_bytes);
  if (rc != MT_OK) return rc;
  MT_REQUIRE(count && ((uintptr_t)count & 7) == 0, "fg_sample_count: count must be an 8-byte aligned device pointer");
  const long nunits = mt_units(V);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fg_count_kernel, dim3(mt_stream_blocks(nunits, AN_WAVES)), dim3(AN_THREADS), 0, s, seg, V, nunits, (int32_t*)ws);
  hipLaunchKernelGGL(fg_scan_kernel, dim3(1), dim3(MT_SCAN_THREADS), 0, s, (int32_t*)ws, nunits, count);
  MT_CHECK_LAUNCH("fg_sample_count");
  return MT_OK;
}

extern "C" int mt_fg_sample_gather(const float* data, int C, long V, const float* seg, long stride, const void* ws, size_t ws_bytes,
                                   float* out, long out_cs, int64_t* nan_counts, mt_stream_t stream) {
  MT_REQUIRE(C >= 1 && C <= AN_MAX_CHANNELS, "fg_sample_gather: %d channels (1..%d)", C, AN_MAX_CHANNELS);
  MT_REQUIRE(stride >= 1, "fg_sample_gather: stride %ld", stride);
  const int rc = fg_args("fg_sample_gather", seg, V, ws, ws_bytes);
  if (rc != MT_OK) return rc;
  MT_REQUIRE(data && out && nan_counts && out_cs >= 1, "fg_sample_gather: bad arguments");
  MT_REQUIRE(((uintptr_t)data & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)nan_counts & 7) == 0, "fg_sample_gather: misaligned pointer");
  FgParams P;
  P.data = (const uint32_t*)data; P.seg = seg; P.V = V; P.nunits = mt_units(V); P.C = C;
  P.stride = stride > (long)INT32_MAX ? (uint32_t)INT32_MAX : (uint32_t)stride;      // ranks stay below 2^31: the same selection
  P.off = (const int32_t*)ws; P.out = (uint32_t*)out; P.out_cs = out_cs; P.nan = (unsigned long long*)nan_counts;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(nan_counts, 0, (size_t)C * sizeof(int64_t), s) != hipSuccess) { mt_set_error("fg_sample_gather: memset failed"); return MT_EHIP; }
  hipLaunchKernelGGL(fg_gather_kernel, dim3(mt_stream_blocks(P.nunits, AN_WAVES)), dim3(AN_THREADS), 0, s, P);
  MT_CHECK_LAUNCH("fg_sample_gather");
  return MT_OK;
}

// ---- label presence ----------------------------------------------------------------------------------------------------------------
#define LP_WORDS 32                        // labels -1..1022 -> bits 0..1023

__global__ __launch_bounds__(AN_THREADS) void label_presence_kernel(const float* __restrict__ seg, long V, uint32_t* __restrict__ bitmap,
                                                                    int32_t* __restrict__ flag) {
  __shared__ uint32_t lb[LP_WORDS + 1];
  if (threadIdx.x <= LP_WORDS) lb[threadIdx.x] = 0;
  __syncthreads();
  int last = -2;                           // the label this thread saw last: runs of one label cost no LDS access
  bool bad = false;
  auto see = [&](float f) {
    if (!(f >= -1.f && f <= 1022.f)) { bad = true; return; }            // NaN fails both comparisons
    const int lab = (int)f;
    if ((float)lab != f) { bad = true; return; }
    if (lab == last) return;
    last = lab;
    const uint32_t b = (uint32_t)(lab + 1), bit = 1u << (b & 31);
    if (!(lb[b >> 5] & bit)) atomicOr(&lb[b >> 5], bit);
  };
  const long nquad = V / 4;
  const long gtid = (long)blockIdx.x * AN_THREADS + threadIdx.x, gstride = (long)gridDim.x * AN_THREADS;
  for (long q = gtid; q < nquad; q += gstride) {
    const mt_f4 a = *(const mt_f4*)(seg + 4 * q);
    see(a.x); see(a.y); see(a.z); see(a.w);
  }
  for (long v = 4 * nquad + gtid; v < V; v += gstride) see(seg[v]);
  if (bad) lb[LP_WORDS] = 1;
  __syncthreads();
  if (threadIdx.x < LP_WORDS) { if (lb[threadIdx.x]) atomicOr(&bitmap[threadIdx.x], lb[threadIdx.x]); }
  else if (threadIdx.x == LP_WORDS) { if (lb[LP_WORDS]) atomicOr((uint32_t*)flag, 1u); }
}

extern "C" int mt_label_presence(const float* seg, long V, uint32_t* bitmap, int32_t* flag, mt_stream_t stream) {
  MT_REQUIRE(seg && bitmap && flag && V > 0, "label_presence: bad arguments");
  MT_REQUIRE(((uintptr_t)seg & 3) == 0 && ((uintptr_t)bitmap & 3) == 0 && ((uintptr_t)flag & 3) == 0, "label_presence: misaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(bitmap, 0, LP_WORDS * sizeof(uint32_t), s) != hipSuccess || hipMemsetAsync(flag, 0, sizeof(int32_t), s) != hipSuccess) {
    mt_set_error("label_presence: memset failed");
    return MT_EHIP;
  }
  hipLaunchKernelGGL(label_presence_kernel, dim3(mt_stream_blocks((V + 3) / 4, AN_THREADS)), dim3(AN_THREADS), 0, s, seg, V, bitmap, flag);
  MT_CHECK_LAUNCH("label_presence");
  return MT_OK;
}
