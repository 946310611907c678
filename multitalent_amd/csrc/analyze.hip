// The dataset fingerprint on the device (experiment_planning/DatasetAnalyzer.py of the reference, :161-224, and the np.unique of
// preprocessing/cropping.py:146 and DatasetAnalyzer.py:83).
//   mt_fg_sample_count / _gather   data[c][seg > 0][::stride] for all channels at once: an ordered compaction built like
//                                  mt_label_locations (units of MT_PP_UNIT voxels, one wave each, ballot ranks on a running counter,
//                                  exclusive scan over the units), of which only every stride-th element is ever written;
//   mt_label_presence              np.unique of an integer label map as a bitmap over -1..1022;
//   mt_label_convert               copy_and_convert_segmentation of the dataset conversion: a stored label volume of any of eight
//                                  types -> uint8 through a table, with the count and the minimum of the unexpected values.
// All of them stream their input (HBM-bound) and use integer counts and integer atomics only: results are bit-identical from run to
// run, whatever the block scheduling.
#include "stream_common.h"
#include "label_class.h"

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

// ---- label conversion ----------------------------------------------------------------------------------------------------------------
// One pass in the stored type: itemsize bytes read and 1 byte written per voxel, no LDS.  The body starts where the INPUT is 16-byte
// aligned (the larger stream): a thread owns LC_VT consecutive voxels, 16 (8 for float64), which are 1, 2 or 4 aligned 16-byte loads
// and one 16-byte (8-byte) store; the store has whatever alignment the output has there, the same for every thread.  The voxels before
// the body and after its last whole chunk, fewer than 32, are scalar accesses of block 0.  The table travels by value in the kernel
// arguments.  Unexpected voxels are counted and their smallest key kept per thread, reduced over the wave with shuffles, and leave
// the wave as one 64-bit add and one 64-bit min: integer atomics, the same result in any order.
struct LcTable { uint16_t t[MT_LABEL_SLOTS + 1]; };
struct __attribute__((packed, aligned(1))) lc_out16 { uint32_t x, y, z, w; };
struct __attribute__((packed, aligned(1))) lc_out8 { uint32_t x, y; };

template <typename T> __device__ __forceinline__ uint32_t lc_one(T v, const LcTable& tab, unsigned long long& cnt, unsigned long long& key) {
  const int s = mt_label_slot(v);
  if (s == MT_LABEL_ZERO) return 0u;
  if (s > 0) {
    const uint32_t m = tab.t[s];
    if (m != MT_LABEL_UNLISTED) return m;
  }
  const unsigned long long k = mt_label_key(v);
  ++cnt;
  key = k < key ? k : key;
  return 0u;
}

template <typename T>
__global__ __launch_bounds__(AN_THREADS) void label_convert_kernel(const T* __restrict__ in, long V, long head, long nchunks, const LcTable tab,
                                                                   uint8_t* __restrict__ out, unsigned long long* __restrict__ report) {
  constexpr int VT = sizeof(T) == 8 ? 8 : 16, NL = VT * (int)sizeof(T) / 16;
  unsigned long long cnt = 0, key = MT_LABEL_KEY_NONE;
  const long gtid = (long)blockIdx.x * AN_THREADS + threadIdx.x, gstride = (long)gridDim.x * AN_THREADS;
  for (long c = gtid; c < nchunks; c += gstride) {
    const long v0 = head + c * VT;
    uint4 raw[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) raw[k] = ((const uint4*)(in + v0))[k];
    T val[VT];
    __builtin_memcpy(val, raw, sizeof(val));
    uint32_t w[VT / 4];
#pragma unroll
    for (int k = 0; k < VT / 4; ++k) {
      w[k] = lc_one(val[4 * k], tab, cnt, key) | lc_one(val[4 * k + 1], tab, cnt, key) << 8 | lc_one(val[4 * k + 2], tab, cnt, key) << 16 |
             lc_one(val[4 * k + 3], tab, cnt, key) << 24;
    }
    if constexpr (VT == 16) { lc_out16 o; o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3]; *(lc_out16*)(out + v0) = o; }
    else { lc_out8 o; o.x = w[0]; o.y = w[1]; *(lc_out8*)(out + v0) = o; }
  }
  if (blockIdx.x == 0) {                                   // head [0, head) and tail [head + nchunks * VT, V): fewer than 2 * 16 voxels
    const long tail0 = head + nchunks * VT;
    long v = threadIdx.x < head ? (long)threadIdx.x : tail0 + ((long)threadIdx.x - head);
    if (v < V) out[v] = (uint8_t)lc_one(in[v], tab, cnt, key);
  }
  if (__any(cnt != 0)) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cnt += __shfl_xor(cnt, o, MT_WAVE);
      const unsigned long long other = __shfl_xor(key, o, MT_WAVE);
      key = other < key ? other : key;
    }
    if (threadIdx.x % MT_WAVE == 0) { atomicAdd(&report[0], cnt); atomicMin(&report[1], key); }
  }
}

static inline int lc_itemsize(int dtype) {
  switch (dtype) {
    case MT_LABEL_U8: case MT_LABEL_I8: return 1;
    case MT_LABEL_I16: case MT_LABEL_U16: return 2;
    case MT_LABEL_I32: case MT_LABEL_U32: case MT_LABEL_F32: return 4;
    case MT_LABEL_F64: return 8;
  }
  return 0;
}
static inline long lc_chunk(int dtype) { return dtype == MT_LABEL_F64 ? 8 : 16; }

extern "C" long mt_label_convert_round(int dtype) {
  if (!lc_itemsize(dtype)) return 0;
  return mt_stream_cap() * AN_THREADS * lc_chunk(dtype);
}

template <typename T>
static void lc_launch(const void* in, long V, long head, long nchunks, const LcTable& tab, uint8_t* out, uint64_t* report, hipStream_t s) {
  hipLaunchKernelGGL(label_convert_kernel<T>, dim3(mt_stream_blocks(nchunks, AN_THREADS)), dim3(AN_THREADS), 0, s, (const T*)in, V, head, nchunks,
                     tab, out, (unsigned long long*)report);
}

extern "C" int mt_label_convert(const void* in, int dtype, long V, const uint16_t* table, uint8_t* out, uint64_t* report, mt_stream_t stream) {
  const int isz = lc_itemsize(dtype);
  MT_REQUIRE(isz != 0, "label_convert: unknown label type %d", dtype);
  MT_REQUIRE(in && table && out && report, "label_convert: null pointer");
  MT_REQUIRE(V > 0, "label_convert: bad voxel count %ld", V);
  MT_REQUIRE(((uintptr_t)in & (uintptr_t)(isz - 1)) == 0, "label_convert: the input is not aligned to its %d-byte elements", isz);
  MT_REQUIRE(((uintptr_t)report & 7) == 0, "label_convert: report must be an 8-byte aligned device pointer");
  LcTable tab;
  for (int l = 0; l < MT_LABEL_SLOTS; ++l) {
    MT_REQUIRE(table[l] <= 255 || table[l] == MT_LABEL_UNLISTED, "label_convert: label %d maps to %d, which is no uint8 value", l, (int)table[l]);
    tab.t[l] = table[l];
  }
  tab.t[MT_LABEL_SLOTS] = MT_LABEL_UNLISTED;
  long head = (long)(((16 - ((uintptr_t)in & 15)) & 15) / (uintptr_t)isz);
  if (head > V) head = V;
  const long nchunks = (V - head) / lc_chunk(dtype);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(report, 0, sizeof(uint64_t), s) != hipSuccess || hipMemsetAsync(report + 1, 0xff, sizeof(uint64_t), s) != hipSuccess) {
    mt_set_error("label_convert: memset failed");
    return MT_EHIP;
  }
  switch (dtype) {
    case MT_LABEL_U8: lc_launch<uint8_t>(in, V, head, nchunks, tab, out, report, s); break;
    case MT_LABEL_I8: lc_launch<int8_t>(in, V, head, nchunks, tab, out, report, s); break;
    case MT_LABEL_I16: lc_launch<int16_t>(in, V, head, nchunks, tab, out, report, s); break;
    case MT_LABEL_U16: lc_launch<uint16_t>(in, V, head, nchunks, tab, out, report, s); break;
    case MT_LABEL_I32: lc_launch<int32_t>(in, V, head, nchunks, tab, out, report, s); break;
    case MT_LABEL_U32: lc_launch<uint32_t>(in, V, head, nchunks, tab, out, report, s); break;
    case MT_LABEL_F32: lc_launch<float>(in, V, head, nchunks, tab, out, report, s); break;
    default: lc_launch<double>(in, V, head, nchunks, tab, out, report, s); break;
  }
  MT_CHECK_LAUNCH("label_convert");
  return MT_OK;
}
