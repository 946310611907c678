// Order statistics on the device: mt_select_kth (float64, the hd95 of evaluation/evaluator.py) and mt_select_kth_f32 (float32, the
// median and percentiles of experiment_planning/DatasetAnalyzer.py) are the two widths of one radix select.
// key = bits ^ (sign ? all ones : sign bit) orders as the numbers do (-0.0 before +0.0, NaNs by bit pattern at both ends).
// sizeof(K) passes of 8 bits, most significant first.  Ranks whose prefixes agree so far form one group and share one histogram; a pass
// reads x once for all groups and adds one LDS atomic per element.  Integer counts only: bit-identical from run to run.
#include "stream_common.h"

#define SEL_THREADS 256
#define SEL_MAXRANKS 8
#define SEL_BINS 256
#define SEL_FLUSH_ITERS (1L << 20)         // x 256 threads x at most 4 elements = 2^30 additions to a workgroup's 32-bit LDS bins per flush
struct SelRanks { unsigned long long k[SEL_MAXRANKS]; };
template <typename K> struct SelState {     // the workspace; K = uint32_t or uint64_t, the key
  unsigned long long k[SEL_MAXRANKS];       // rank among the elements that share the prefix
  unsigned long long hist[SEL_MAXRANKS][SEL_BINS];    // per group
  K prefix[SEL_MAXRANKS];                   // the digits found so far (high bits of the key)
  K gprefix[SEL_MAXRANKS];                  // the distinct prefixes
  int32_t group[SEL_MAXRANKS];              // rank -> group
  int32_t ngroups, pad;
};

template <typename K> __device__ __forceinline__ K sel_key(K bits) {
  constexpr K sign = (K)1 << (8 * sizeof(K) - 1);
  return bits ^ ((bits & sign) ? ~(K)0 : sign);
}
template <typename K> __device__ __forceinline__ K sel_bits(K key) {
  constexpr K sign = (K)1 << (8 * sizeof(K) - 1);
  return key ^ ((key & sign) ? sign : ~(K)0);
}

template <typename K> __global__ void sel_init_kernel(SelState<K>* __restrict__ st, const SelRanks ranks) {
  if (threadIdx.x < SEL_MAXRANKS) {
    st->k[threadIdx.x] = ranks.k[threadIdx.x]; st->prefix[threadIdx.x] = 0; st->gprefix[threadIdx.x] = 0; st->group[threadIdx.x] = 0;
  }
  if (threadIdx.x == 0) { st->ngroups = 1; st->pad = 0; }
  for (int i = threadIdx.x; i < SEL_MAXRANKS * SEL_BINS; i += blockDim.x) st->hist[i / SEL_BINS][i % SEL_BINS] = 0;
}

template <typename K> __device__ __forceinline__ void sel_add(K bits, int pass, int shift, int ng, const K* gp, uint32_t (*lh)[SEL_BINS]) {
  const K key = sel_key<K>(bits);
  const K hi = pass ? key >> (shift + 8) : (K)0;
  const uint32_t digit = (uint32_t)(key >> shift) & (SEL_BINS - 1);
  for (int g = 0; g < ng; ++g)
    if (hi == gp[g]) { atomicAdd(&lh[g][digit], 1u); break; }          // the group prefixes are distinct
}

// 16-byte loads from the first 16-byte aligned element on; block 0 takes the elements before and after (fewer than 16 bytes each).
template <typename K>
__global__ __launch_bounds__(SEL_THREADS) void sel_hist_kernel(const K* __restrict__ x, long n, int pass, SelState<K>* __restrict__ st) {
  constexpr int PER = 16 / sizeof(K);                                   // elements per load
  __shared__ uint32_t lh[SEL_MAXRANKS][SEL_BINS];
  __shared__ K gp[SEL_MAXRANKS];
  const int ng = st->ngroups;
  for (int i = threadIdx.x; i < ng * SEL_BINS; i += SEL_THREADS) lh[i / SEL_BINS][i % SEL_BINS] = 0;
  if ((int)threadIdx.x < SEL_MAXRANKS) gp[threadIdx.x] = st->gprefix[threadIdx.x];
  __syncthreads();
  const int shift = 8 * ((int)sizeof(K) - 1 - pass);
  long head = (long)(((16 - ((uintptr_t)x & 15)) & 15) / sizeof(K));
  if (head > n) head = n;
  const long nvec = (n - head) / PER;
  const uint4* xv = (const uint4*)(x + head);
  const long gtid = (long)blockIdx.x * SEL_THREADS + threadIdx.x, gstride = (long)gridDim.x * SEL_THREADS;
  const long iters = (nvec + gstride - 1) / gstride;                    // the same for every thread
  long it0 = 0;
  do {
    const long it1 = it0 + SEL_FLUSH_ITERS < iters ? it0 + SEL_FLUSH_ITERS : iters;
    for (long it = it0; it < it1; ++it) {
      const long q = it * gstride + gtid;
      if (q < nvec) {
        const uint4 a = xv[q];
        if constexpr (sizeof(K) == 4) {
          sel_add<K>(a.x, pass, shift, ng, gp, lh); sel_add<K>(a.y, pass, shift, ng, gp, lh);
          sel_add<K>(a.z, pass, shift, ng, gp, lh); sel_add<K>(a.w, pass, shift, ng, gp, lh);
        } else {
          sel_add<K>((K)a.x | (K)a.y << 32, pass, shift, ng, gp, lh); sel_add<K>((K)a.z | (K)a.w << 32, pass, shift, ng, gp, lh);
        }
      }
    }
    if (it0 == 0 && blockIdx.x == 0) {
      for (long i = threadIdx.x; i < head; i += SEL_THREADS) sel_add<K>(x[i], pass, shift, ng, gp, lh);
      for (long i = head + PER * nvec + threadIdx.x; i < n; i += SEL_THREADS) sel_add<K>(x[i], pass, shift, ng, gp, lh);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ng * SEL_BINS; i += SEL_THREADS) {
      const uint32_t h = lh[i / SEL_BINS][i % SEL_BINS];
      if (h) { atomicAdd(&st->hist[i / SEL_BINS][i % SEL_BINS], (unsigned long long)h); lh[i / SEL_BINS][i % SEL_BINS] = 0; }
    }
    __syncthreads();
    it0 = it1;
  } while (it0 < iters);
}

// One wave.  Per rank: lane l sums bins 4l..4l+3 of the rank's group, an inclusive scan over the lanes finds the lane, that lane the
// bin, that holds the rank.  Then the ranks are regrouped by their new prefixes and the bins are cleared for the next pass.
template <typename K>
__global__ __launch_bounds__(MT_WAVE) void sel_pick_kernel(SelState<K>* __restrict__ st, int nr, int last, K* __restrict__ out) {
  const int lane = threadIdx.x;
  __shared__ K sp[SEL_MAXRANKS];
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
      sp[r] = (st->prefix[r] << 8) | (K)(4 * lane + j);
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
      if (last) out[r] = sel_bits<K>(sp[r]);
    }
    st->ngroups = ng;
  }
  __syncthreads();
  for (int i = lane; i < SEL_MAXRANKS * SEL_BINS; i += MT_WAVE) st->hist[i / SEL_BINS][i % SEL_BINS] = 0;
}

template <typename K> static size_t sel_workspace(int nranks) { return nranks >= 1 && nranks <= SEL_MAXRANKS ? sizeof(SelState<K>) : 0; }

template <typename K>
static int sel_launch(const char* who, const void* x, long n, const long* ranks, int nranks, void* out, void* ws, size_t ws_bytes,
                      mt_stream_t stream) {
  MT_REQUIRE(x && ranks && out && ws, "%s: null pointer", who);
  MT_REQUIRE(n >= 1, "%s: bad element count %ld", who, n);
  MT_REQUIRE(nranks >= 1 && nranks <= SEL_MAXRANKS, "%s: %d ranks (1..%d)", who, nranks, SEL_MAXRANKS);
  SelRanks rk;
  for (int r = 0; r < SEL_MAXRANKS; ++r) rk.k[r] = 0;
  for (int r = 0; r < nranks; ++r) {
    MT_REQUIRE(ranks[r] >= 0 && ranks[r] < n, "%s: rank %ld outside 0..%ld", who, ranks[r], n - 1);
    rk.k[r] = (unsigned long long)ranks[r];
  }
  MT_REQUIRE(((uintptr_t)x & (sizeof(K) - 1)) == 0 && ((uintptr_t)out & (sizeof(K) - 1)) == 0 && ((uintptr_t)ws & 7) == 0,
             "%s: misaligned pointer", who);
  MT_REQUIRE_WORKSPACE(who, ws_bytes, sizeof(SelState<K>));
  SelState<K>* st = (SelState<K>*)ws;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sel_init_kernel<K>, dim3(1), dim3(SEL_THREADS), 0, s, st, rk);
  MT_CHECK_LAUNCH(who);
  const int grid = mt_stream_blocks(n / (16 / sizeof(K)), SEL_THREADS);
  const int npass = (int)sizeof(K);
  for (int pass = 0; pass < npass; ++pass) {
    hipLaunchKernelGGL(sel_hist_kernel<K>, dim3(grid), dim3(SEL_THREADS), 0, s, (const K*)x, n, pass, st);
    MT_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(sel_pick_kernel<K>, dim3(1), dim3(MT_WAVE), 0, s, st, nranks, pass == npass - 1 ? 1 : 0, (K*)out);
    MT_CHECK_LAUNCH(who);
  }
  return MT_OK;
}

extern "C" size_t mt_select_kth_workspace(int nranks) { return sel_workspace<uint64_t>(nranks); }
extern "C" int mt_select_kth(const double* x, long n, const long* ranks, int nranks, double* out, void* ws, size_t ws_bytes,
                             mt_stream_t stream) {
  return sel_launch<uint64_t>("select_kth", x, n, ranks, nranks, out, ws, ws_bytes, stream);
}

extern "C" size_t mt_select_kth_f32_workspace(int nranks) { return sel_workspace<uint32_t>(nranks); }
extern "C" int mt_select_kth_f32(const float* x, long n, const long* ranks, int nranks, float* out, void* ws, size_t ws_bytes,
                                 mt_stream_t stream) {
  return sel_launch<uint32_t>("select_kth_f32", x, n, ranks, nranks, out, ws, ws_bytes, stream);
}
