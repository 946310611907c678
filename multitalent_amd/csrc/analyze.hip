// The dataset fingerprint on the device (experiment_planning/DatasetAnalyzer.py of the reference, :161-224, and the np.unique of
// preprocessing/cropping.py:146 and DatasetAnalyzer.py:83).
//   mt_fg_sample_count / _gather   data[c][seg > 0][::stride] for all channels at once: an ordered compaction built like
//                                  mt_label_locations (units of MT_PP_UNIT voxels, one wave each, ballot ranks on a running counter,
//                                  exclusive scan over the units), of which only every stride-th element is ever written;
//   mt_select_kth_f32              order statistics of signed float32: radix select, 4 passes of 8 bits, on the order-preserving key;
//   mt_label_presence              np.unique of an integer label map as a bitmap over -1..1022.
// All of them stream their input (HBM-bound) and use integer counts and integer atomics only: results are bit-identical from run to
// run, whatever the block scheduling.
#include "mt_common.h"

#define AN_THREADS 256
#define AN_WAVES (AN_THREADS / MT_WAVE)
#define AN_MAX_CHANNELS 16

static int an_cap_blocks() {
  const int cap = mt_device_cus(mt_current_device()) * 8;
  return cap > 0 ? cap : 1;
}

// 16 bytes that are only dword aligned (the label map of a case is the last channel of its array): gfx950 serves a dword-aligned
// global_load_dwordx4.
struct __attribute__((packed, aligned(4))) an_f4 { float x, y, z, w; };

// ---- ordered strided foreground sampling -------------------------------------------------------------------------------------
static long an_units(long V) { return (V + MT_PP_UNIT - 1) / MT_PP_UNIT; }

// One wave per unit: the number of voxels with seg > 0 (a float comparison: -1, 0 and NaN are not selected).
__global__ __launch_bounds__(AN_THREADS) void fg_count_kernel(const float* __restrict__ seg, long V, long nunits, int32_t* __restrict__ off) {
  const int lane = threadIdx.x % MT_WAVE;
  for (long unit = (long)blockIdx.x * AN_WAVES + threadIdx.x / MT_WAVE; unit < nunits; unit += (long)gridDim.x * AN_WAVES) {
    const long v0 = unit * MT_PP_UNIT, vend = (v0 + MT_PP_UNIT < V) ? v0 + MT_PP_UNIT : V;
    const long nquad = (vend - v0) / 4;
    int cnt = 0;
#pragma unroll 4
    for (long q = lane; q < nquad; q += MT_WAVE) {
      const an_f4 s = *(const an_f4*)(seg + v0 + 4 * q);
      cnt += (s.x > 0.f) + (s.y > 0.f) + (s.z > 0.f) + (s.w > 0.f);
    }
    for (long v = v0 + 4 * nquad + lane; v < vend; v += MT_WAVE) cnt += seg[v] > 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, MT_WAVE);
    if (lane == 0) off[unit] = cnt;
  }
}

// One block: counts of the units -> exclusive offsets in place, total -> *count.
__global__ __launch_bounds__(AN_THREADS) void fg_scan_kernel(int32_t* __restrict__ off, long nunits, int64_t* __restrict__ count) {
  const long per = (nunits + AN_THREADS - 1) / AN_THREADS;
  const long b = threadIdx.x * per, e = b + per < nunits ? b + per : nunits;
  long sum = 0;
  for (long u = b; u < e; ++u) sum += off[u];
  __shared__ long sh[AN_THREADS];
  sh[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    long run = 0;
    for (int t = 0; t < AN_THREADS; ++t) { const long n = sh[t]; sh[t] = run; run += n; }
    *count = run;
  }
  __syncthreads();
  long run = sh[threadIdx.x];
  for (long u = b; u < e; ++u) { const int32_t n = off[u]; off[u] = (int32_t)run; run += n; }
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
    const long v0 = unit * MT_PP_UNIT, vend = (v0 + MT_PP_UNIT < P.V) ? v0 + MT_PP_UNIT : P.V;
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

static int an_unit_blocks(long nunits) {
  const int cap = an_cap_blocks();
  const int b = mt_cdiv(nunits, AN_WAVES);
  return b < cap ? b : cap;
}

extern "C" size_t mt_fg_sample_workspace(long V) {
  if (V < 1) return 0;
  return (((size_t)an_units(V) * sizeof(int32_t)) + 7) & ~(size_t)7;
}

static int fg_args(const char* who, const float* seg, long V, const void* ws, size_t ws_bytes) {
  MT_REQUIRE(seg && ws, "%s: null pointer", who);
  MT_REQUIRE(V > 0, "%s: bad voxel count %ld", who, V);
  MT_REQUIRE(V <= (long)INT32_MAX, "%s: %ld voxels exceed the int32 index range", who, V);
  MT_REQUIRE(((uintptr_t)seg & 3) == 0 && ((uintptr_t)ws & 7) == 0, "%s: misaligned pointer", who);
  if (ws_bytes < mt_fg_sample_workspace(V)) {
    mt_set_error("%s: workspace of %zu bytes, %zu needed", who, ws_bytes, mt_fg_sample_workspace(V));
    return MT_EWORKSPACE;
  }
  return MT_OK;
}

extern "C" int mt_fg_sample_count(const float* seg, long V, int64_t* count, void* ws, size_t ws_bytes, mt_stream_t stream) {
  const int rc = fg_args("fg_sample_count", seg, V, ws, ws_bytes);
  if (rc != MT_OK) return rc;
  MT_REQUIRE(count && ((uintptr_t)count & 7) == 0, "fg_sample_count: count must be an 8-byte aligned device pointer");
  const long nunits = an_units(V);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fg_count_kernel, dim3(an_unit_blocks(nunits)), dim3(AN_THREADS), 0, s, seg, V, nunits, (int32_t*)ws);
  hipLaunchKernelGGL(fg_scan_kernel, dim3(1), dim3(AN_THREADS), 0, s, (int32_t*)ws, nunits, count);
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
  P.data = (const uint32_t*)data; P.seg = seg; P.V = V; P.nunits = an_units(V); P.C = C;
  P.stride = stride > (long)INT32_MAX ? (uint32_t)INT32_MAX : (uint32_t)stride;      // ranks stay below 2^31: the same selection
  P.off = (const int32_t*)ws; P.out = (uint32_t*)out; P.out_cs = out_cs; P.nan = (unsigned long long*)nan_counts;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(nan_counts, 0, (size_t)C * sizeof(int64_t), s) != hipSuccess) { mt_set_error("fg_sample_gather: memset failed"); return MT_EHIP; }
  hipLaunchKernelGGL(fg_gather_kernel, dim3(an_unit_blocks(P.nunits)), dim3(AN_THREADS), 0, s, P);
  MT_CHECK_LAUNCH("fg_sample_gather");
  return MT_OK;
}

// ---- order statistics of float32 (radix select) ------------------------------------------------------------------------------
// key = bits ^ (sign ? 0xffffffff : 0x80000000) orders as the numbers do (-0.0 before +0.0, NaNs by bit pattern at both ends).
// Four passes of 8 bits, most significant first.  Ranks whose prefixes agree so far form one group and share one histogram; a pass
// reads x once for all groups.
#define SF_MAXRANKS 8
#define SF_BINS 256
#define SF_FLUSH_ITERS (1L << 20)          // x 256 threads x 4 elements = 2^30 additions to a workgroup's 32-bit LDS bins per flush
struct SelF32Ranks { unsigned long long k[SF_MAXRANKS]; };
struct SelF32State {                        // the workspace
  unsigned long long k[SF_MAXRANKS];        // rank among the elements that share the prefix
  unsigned long long hist[SF_MAXRANKS][SF_BINS];      // per group
  uint32_t prefix[SF_MAXRANKS];             // the digits found so far (high bits of the key)
  uint32_t gprefix[SF_MAXRANKS];            // the distinct prefixes
  int32_t group[SF_MAXRANKS];               // rank -> group
  int32_t ngroups, pad;
};

__device__ __forceinline__ uint32_t sf_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ uint32_t sf_bits(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu); }

__global__ void self32_init_kernel(SelF32State* __restrict__ st, const SelF32Ranks ranks) {
  if (threadIdx.x < SF_MAXRANKS) {
    st->k[threadIdx.x] = ranks.k[threadIdx.x]; st->prefix[threadIdx.x] = 0; st->gprefix[threadIdx.x] = 0; st->group[threadIdx.x] = 0;
  }
  if (threadIdx.x == 0) { st->ngroups = 1; st->pad = 0; }
  for (int i = threadIdx.x; i < SF_MAXRANKS * SF_BINS; i += blockDim.x) st->hist[i / SF_BINS][i % SF_BINS] = 0;
}

__device__ __forceinline__ void sf_add(uint32_t bits, int pass, int shift, int ng, const uint32_t* gp, uint32_t (*lh)[SF_BINS]) {
  const uint32_t key = sf_key(bits);
  const uint32_t hi = pass ? key >> (shift + 8) : 0u;
  const uint32_t digit = (key >> shift) & (SF_BINS - 1);
  for (int g = 0; g < ng; ++g)
    if (hi == gp[g]) { atomicAdd(&lh[g][digit], 1u); break; }          // the group prefixes are distinct
}

// 16-byte loads from the first 16-byte aligned element on; block 0 takes the (at most 3 + 3) elements before and after.
__global__ __launch_bounds__(AN_THREADS) void self32_hist_kernel(const uint32_t* __restrict__ x, long n, int pass, SelF32State* __restrict__ st) {
  __shared__ uint32_t lh[SF_MAXRANKS][SF_BINS];
  __shared__ uint32_t gp[SF_MAXRANKS];
  const int ng = st->ngroups;
  for (int i = threadIdx.x; i < ng * SF_BINS; i += AN_THREADS) lh[i / SF_BINS][i % SF_BINS] = 0;
  if ((int)threadIdx.x < SF_MAXRANKS) gp[threadIdx.x] = st->gprefix[threadIdx.x];
  __syncthreads();
  const int shift = 24 - 8 * pass;
  long head = (long)(((16 - ((uintptr_t)x & 15)) & 15) / 4);
  if (head > n) head = n;
  const long nquad = (n - head) / 4;
  const uint4* xq = (const uint4*)(x + head);
  const long gtid = (long)blockIdx.x * AN_THREADS + threadIdx.x, gstride = (long)gridDim.x * AN_THREADS;
  const long iters = (nquad + gstride - 1) / gstride;                   // the same for every thread
  long it0 = 0;
  do {
    const long it1 = it0 + SF_FLUSH_ITERS < iters ? it0 + SF_FLUSH_ITERS : iters;
    for (long it = it0; it < it1; ++it) {
      const long q = it * gstride + gtid;
      if (q < nquad) {
        const uint4 a = xq[q];
        sf_add(a.x, pass, shift, ng, gp, lh); sf_add(a.y, pass, shift, ng, gp, lh);
        sf_add(a.z, pass, shift, ng, gp, lh); sf_add(a.w, pass, shift, ng, gp, lh);
      }
    }
    if (it0 == 0 && blockIdx.x == 0) {
      for (long i = threadIdx.x; i < head; i += AN_THREADS) sf_add(x[i], pass, shift, ng, gp, lh);
      for (long i = head + 4 * nquad + threadIdx.x; i < n; i += AN_THREADS) sf_add(x[i], pass, shift, ng, gp, lh);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ng * SF_BINS; i += AN_THREADS) {
      const uint32_t h = lh[i / SF_BINS][i % SF_BINS];
      if (h) { atomicAdd(&st->hist[i / SF_BINS][i % SF_BINS], (unsigned long long)h); lh[i / SF_BINS][i % SF_BINS] = 0; }
    }
    __syncthreads();
    it0 = it1;
  } while (it0 < iters);
}

// One wave.  Per rank: lane l sums bins 4l..4l+3 of the rank's group, an inclusive scan over the lanes finds the lane, that lane the
// bin, that holds the rank.  Then the ranks are regrouped by their new prefixes and the bins are cleared for the next pass.
__global__ __launch_bounds__(MT_WAVE) void self32_pick_kernel(SelF32State* __restrict__ st, int nr, int last, uint32_t* __restrict__ out) {
  const int lane = threadIdx.x;
  __shared__ uint32_t sp[SF_MAXRANKS];
  for (int r = 0; r < nr; ++r) {
    const int g = st->group[r];
    const unsigned long long k = st->k[r];
    unsigned long long h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = st->hist[g][4 * lane + j];
    const unsigned long long s = h[0] + h[1] + h[2] + h[3];
    unsigned long long incl = s;
#pragma unroll
    for (int d = 1; d < MT_WAVE; d <<= 1) {
      const unsigned long long t = __shfl_up(incl, d, MT_WAVE);
      if (lane >= d) incl += t;
    }
    const uint64_t m = __ballot(incl > k);
    const int owner = m ? __ffsll((unsigned long long)m) - 1 : MT_WAVE - 1;       // the entry point checked rank < n: m != 0
    if (lane == owner) {
      unsigned long long cum = incl - s;
      int j = 0;
      for (; j < 3; ++j) { if (cum + h[j] > k) break; cum += h[j]; }
      sp[r] = (st->prefix[r] << 8) | (uint32_t)(4 * lane + j);
      st->k[r] = k - cum;
    }
  }
  __syncthreads();
  if (lane == 0) {
    int ng = 0;
    for (int r = 0; r < nr; ++r) {
      int g = -1;
      for (int q = 0; q < r; ++q) if (sp[q] == sp[r]) { g = st->group[q]; break; }
      if (g < 0) { g = ng; st->gprefix[ng] = sp[r]; ++ng; }
      st->group[r] = g; st->prefix[r] = sp[r];
      if (last) out[r] = sf_bits(sp[r]);
    }
    st->ngroups = ng;
  }
  __syncthreads();
  for (int i = lane; i < SF_MAXRANKS * SF_BINS; i += MT_WAVE) st->hist[i / SF_BINS][i % SF_BINS] = 0;
}

extern "C" size_t mt_select_kth_f32_workspace(int nranks) {
  return nranks >= 1 && nranks <= SF_MAXRANKS ? sizeof(SelF32State) : 0;
}

extern "C" int mt_select_kth_f32(const float* x, long n, const long* ranks, int nranks, float* out, void* ws, size_t ws_bytes,
                                 mt_stream_t stream) {
  MT_REQUIRE(x && ranks && out && ws, "select_kth_f32: null pointer");
  MT_REQUIRE(n >= 1, "select_kth_f32: bad element count %ld", n);
  MT_REQUIRE(nranks >= 1 && nranks <= SF_MAXRANKS, "select_kth_f32: %d ranks (1..%d)", nranks, SF_MAXRANKS);
  SelF32Ranks rk;
  for (int r = 0; r < SF_MAXRANKS; ++r) rk.k[r] = 0;
  for (int r = 0; r < nranks; ++r) {
    MT_REQUIRE(ranks[r] >= 0 && ranks[r] < n, "select_kth_f32: rank %ld outside 0..%ld", ranks[r], n - 1);
    rk.k[r] = (unsigned long long)ranks[r];
  }
  MT_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)ws & 7) == 0, "select_kth_f32: misaligned pointer");
  if (ws_bytes < sizeof(SelF32State)) {
    mt_set_error("select_kth_f32: workspace of %zu bytes, %zu needed", ws_bytes, sizeof(SelF32State));
    return MT_EWORKSPACE;
  }
  SelF32State* st = (SelF32State*)ws;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(self32_init_kernel, dim3(1), dim3(AN_THREADS), 0, s, st, rk);
  MT_CHECK_LAUNCH("select_kth_f32 (init)");
  long grid = (n / 4 + AN_THREADS - 1) / AN_THREADS;
  const long cap = an_cap_blocks();
  if (grid > cap) grid = cap;
  if (grid < 1) grid = 1;
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(self32_hist_kernel, dim3((unsigned)grid), dim3(AN_THREADS), 0, s, (const uint32_t*)x, n, pass, st);
    MT_CHECK_LAUNCH("select_kth_f32 (histogram)");
    hipLaunchKernelGGL(self32_pick_kernel, dim3(1), dim3(MT_WAVE), 0, s, st, nranks, pass == 3 ? 1 : 0, (uint32_t*)out);
    MT_CHECK_LAUNCH("select_kth_f32 (pick)");
  }
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
    const an_f4 a = *(const an_f4*)(seg + 4 * q);
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
  long grid = ((V + 3) / 4 + AN_THREADS - 1) / AN_THREADS;
  const long cap = an_cap_blocks();
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL(label_presence_kernel, dim3((unsigned)grid), dim3(AN_THREADS), 0, s, seg, V, bitmap, flag);
  MT_CHECK_LAUNCH("label_presence");
  return MT_OK;
}
