// Preprocessing a training case on the device (preprocessing/preprocessing.py of the reference, :273-353): the intensity
// normalisation schemes with their per-case moments, and the sampled class locations of `_run_internal`.
//   mt_masked_moments        count, mean and population sd per channel over a predicate, in double, two passes (mean, then the
//                            centred squares: nothing cancels for a CT volume of mean -900 and sd 5);
//   mt_intensity_normalize   one in-place pass: clip, (x - mean) / (sd + eps) in the reference's float32 order, masked zeroing;
//   mt_label_counts          voxels per class, and per (class, unit of MT_PP_UNIT voxels) the exclusive offsets of an ordered compaction;
//   mt_label_locations       np.argwhere(seg == c)[rank] for a list of (class, rank) queries, through that compaction.
// All of them stream the volume once per pass (HBM-bound).  Every sum is formed in a fixed order and the compaction uses integer
// counts only: results are bit-identical from run to run, whatever the block scheduling.
#include "stream_common.h"
#include <math.h>

#define PP_THREADS 256
#define PP_WAVES (PP_THREADS / MT_WAVE)
#define PP_MAX_CHANNELS 16

// ---- masked moments ----------------------------------------------------------------------------------------------------------
struct MomParams {
  const float* data; const float* seg; long V; int pred, pass, nblk;
  double lo[PP_MAX_CHANNELS], hi[PP_MAX_CHANNELS];
  double* part;            // [C][nblk][2]: (count, sum) of pass 0, (unused, centred sum of squares) of pass 1
  const double* stats;     // [C][3], pass 1 reads the mean
};

template <int PRED> __device__ __forceinline__ bool pp_selected(float x, float s, double lo, double hi) {
  if (PRED == MT_MOMENTS_ALL) return true;
  if (PRED == MT_MOMENTS_SEG_GE0) return s >= 0.f;
  return (double)x > lo && (double)x < hi;
}

// grid (nblk, C).  Per thread a double sum and a count over a grid-stride loop of 16-byte quads; per block the four wave sums are
// added in wave order.  The partial of a block depends on the grid size only, which the host derives from V.
template <int PRED, int PASS>
__global__ __launch_bounds__(PP_THREADS) void moments_kernel(const MomParams P) {
  const int c = blockIdx.y;
  const float* x = P.data + (size_t)c * P.V;
  const double lo = P.lo[c], hi = P.hi[c];
  const double mean = PASS ? P.stats[c * 3 + 1] : 0.0;
  const long nquad = P.V / 4;
  const long gtid = (long)blockIdx.x * PP_THREADS + threadIdx.x, gstride = (long)gridDim.x * PP_THREADS;
  double sum = 0.0, cnt = 0.0;
  for (long q = gtid; q < nquad; q += gstride) {
    const mt_f4 a = *(const mt_f4*)(x + 4 * q);
    mt_f4 s = {0.f, 0.f, 0.f, 0.f};
    if (PRED == MT_MOMENTS_SEG_GE0) s = *(const mt_f4*)(P.seg + 4 * q);
    const float av[4] = {a.x, a.y, a.z, a.w}, sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (pp_selected<PRED>(av[k], sv[k], lo, hi)) {
        const double d = (double)av[k] - mean;
        sum += PASS ? d * d : d;
        cnt += 1.0;
      }
  }
  for (long v = 4 * nquad + gtid; v < P.V; v += gstride) {
    const float a = x[v], s = PRED == MT_MOMENTS_SEG_GE0 ? P.seg[v] : 0.f;
    if (pp_selected<PRED>(a, s, lo, hi)) {
      const double d = (double)a - mean;
      sum += PASS ? d * d : d;
      cnt += 1.0;
    }
  }
  sum = mt_wave_sum_d(sum);
  cnt = mt_wave_sum_d(cnt);               // counts below 2^53: exact in double
  __shared__ double sh[PP_WAVES][2];
  const int wave = threadIdx.x / MT_WAVE, lane = threadIdx.x % MT_WAVE;
  if (lane == 0) { sh[wave][0] = cnt; sh[wave][1] = sum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double c0 = 0.0, s0 = 0.0;
    for (int w = 0; w < PP_WAVES; ++w) { c0 += sh[w][0]; s0 += sh[w][1]; }
    double* o = P.part + ((size_t)c * P.nblk + blockIdx.x) * 2;
    o[0] = c0; o[1] = s0;
  }
}

// One wave per channel: lane l adds partials l, l + 64, ... in that order, then the butterfly (a fixed tree).
__global__ __launch_bounds__(MT_WAVE) void moments_finalize_kernel(const double* __restrict__ part, int nblk, int pass, double* __restrict__ stats) {
  const int c = blockIdx.x;
  const double* p = part + (size_t)c * nblk * 2;
  double cnt = 0.0, sum = 0.0;
  for (int b = threadIdx.x; b < nblk; b += MT_WAVE) { cnt += p[2 * b]; sum += p[2 * b + 1]; }
  cnt = mt_wave_sum_d(cnt);
  sum = mt_wave_sum_d(sum);
  if (threadIdx.x == 0) {
    double* o = stats + c * 3;
    if (pass == 0) { o[0] = cnt; o[1] = cnt > 0.0 ? sum / cnt : (double)NAN; }
    else o[2] = cnt > 0.0 ? sqrt(sum / cnt) : (double)NAN;          // numpy: mean and std of an empty selection are nan
  }
}

static int pp_moment_blocks(long V) { return mt_stream_blocks((V + 3) / 4, PP_THREADS); }

extern "C" size_t mt_masked_moments_workspace(int C, long V) {
  if (C < 1 || V < 1) return 0;
  return (size_t)C * pp_moment_blocks(V) * 2 * sizeof(double);
}

extern "C" int mt_masked_moments(const float* data, int C, long V, int pred, const float* seg, const double* lo, const double* hi,
                                 double* stats, void* ws, size_t ws_bytes, mt_stream_t stream) {
  MT_REQUIRE(data && stats && ws, "masked_moments: null pointer");
  MT_REQUIRE(C >= 1 && C <= PP_MAX_CHANNELS && V > 0, "masked_moments: bad shape %d x %ld (at most %d channels)", C, V, PP_MAX_CHANNELS);
  MT_REQUIRE(pred == MT_MOMENTS_ALL || pred == MT_MOMENTS_SEG_GE0 || pred == MT_MOMENTS_OPEN_RANGE, "masked_moments: predicate %d", pred);
  MT_REQUIRE(pred != MT_MOMENTS_SEG_GE0 || seg, "masked_moments: the seg >= 0 predicate needs seg");
  MT_REQUIRE(pred != MT_MOMENTS_OPEN_RANGE || (lo && hi), "masked_moments: the range predicate needs lo and hi");
  MT_REQUIRE(((uintptr_t)data & 3) == 0 && ((uintptr_t)seg & 3) == 0 && ((uintptr_t)stats & 7) == 0 && ((uintptr_t)ws & 7) == 0,
             "masked_moments: misaligned pointer");
  MT_REQUIRE_WORKSPACE("masked_moments", ws_bytes, mt_masked_moments_workspace(C, V));
  MomParams P;
  P.data = data; P.seg = seg; P.V = V; P.pred = pred; P.nblk = pp_moment_blocks(V); P.part = (double*)ws; P.stats = stats;
  for (int c = 0; c < PP_MAX_CHANNELS; ++c) {
    P.lo[c] = (pred == MT_MOMENTS_OPEN_RANGE && c < C) ? lo[c] : 0.0;
    P.hi[c] = (pred == MT_MOMENTS_OPEN_RANGE && c < C) ? hi[c] : 0.0;
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(P.nblk, C), blk(PP_THREADS);
  for (int pass = 0; pass < 2; ++pass) {
    P.pass = pass;
#define PP_LAUNCH(PRED)                                                                               \
    if (pass == 0) hipLaunchKernelGGL((moments_kernel<PRED, 0>), grid, blk, 0, s, P);                 \
    else hipLaunchKernelGGL((moments_kernel<PRED, 1>), grid, blk, 0, s, P)
    if (pred == MT_MOMENTS_ALL) { PP_LAUNCH(MT_MOMENTS_ALL); }
    else if (pred == MT_MOMENTS_SEG_GE0) { PP_LAUNCH(MT_MOMENTS_SEG_GE0); }
    else { PP_LAUNCH(MT_MOMENTS_OPEN_RANGE); }
#undef PP_LAUNCH
    hipLaunchKernelGGL(moments_finalize_kernel, dim3(C), dim3(MT_WAVE), 0, s, (const double*)ws, P.nblk, pass, stats);
  }
  MT_CHECK_LAUNCH("masked_moments");
  return MT_OK;
}

// ---- normalise -----------------------------------------------------------------------------------------------------------------
struct NormParams { float* x; const float* seg; long V; int clip, masked; float lo, hi, mean, sd, eps; const double* stats; };

__device__ __forceinline__ float pp_norm1(float x, float s, const NormParams& P, float mean, float den) {
  if (P.masked && s < 0.f) return 0.f;      // numpy's data[seg < 0] = 0: a NaN in seg zeroes nothing
  if (P.clip) {                             // np.clip as two comparisons: a NaN voxel fails both and passes unchanged
    x = x < P.lo ? P.lo : x;
    x = x > P.hi ? P.hi : x;
  }
  return (x - mean) / den;                 // a true float32 division, as numpy's (x - m) / s: no reciprocal
}

__global__ __launch_bounds__(PP_THREADS) void normalize_kernel(const NormParams P) {
  const float mean = P.stats ? (float)P.stats[1] : P.mean;
  const float den = (P.stats ? (float)P.stats[2] : P.sd) + P.eps;           // float32 sum, numpy's `std + 1e-8` on a float32 std
  const long nquad = P.V / 4;
  const long gtid = (long)blockIdx.x * PP_THREADS + threadIdx.x, gstride = (long)gridDim.x * PP_THREADS;
  for (long q = gtid; q < nquad; q += gstride) {
    mt_f4 a = *(const mt_f4*)(P.x + 4 * q);
    mt_f4 s = {0.f, 0.f, 0.f, 0.f};
    if (P.masked) s = *(const mt_f4*)(P.seg + 4 * q);
    a.x = pp_norm1(a.x, s.x, P, mean, den); a.y = pp_norm1(a.y, s.y, P, mean, den);
    a.z = pp_norm1(a.z, s.z, P, mean, den); a.w = pp_norm1(a.w, s.w, P, mean, den);
    *(mt_f4*)(P.x + 4 * q) = a;
  }
  for (long v = 4 * nquad + gtid; v < P.V; v += gstride) P.x[v] = pp_norm1(P.x[v], P.masked ? P.seg[v] : 0.f, P, mean, den);
}

extern "C" int mt_intensity_normalize(float* x, long V, int clip, float lo, float hi, float mean, float sd, const double* stats, float eps,
                                      const float* seg, mt_stream_t stream) {
  MT_REQUIRE(x && V > 0, "intensity_normalize: bad arguments");
  MT_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)seg & 3) == 0 && ((uintptr_t)stats & 7) == 0, "intensity_normalize: misaligned pointer");
  MT_REQUIRE(!clip || lo <= hi, "intensity_normalize: clip bounds %g > %g", (double)lo, (double)hi);
  NormParams P;
  P.x = x; P.seg = seg; P.V = V; P.clip = clip ? 1 : 0; P.masked = seg ? 1 : 0; P.lo = lo; P.hi = hi; P.mean = mean; P.sd = sd; P.eps = eps;
  P.stats = stats;
  hipLaunchKernelGGL(normalize_kernel, dim3(pp_moment_blocks(V)), dim3(PP_THREADS), 0, (hipStream_t)stream, P);
  MT_CHECK_LAUNCH("intensity_normalize");
  return MT_OK;
}

// ---- class counts and locations ---------------------------------------------------------------------------------------------------
// The volume is cut into units of MT_PP_UNIT consecutive voxels, one wave per unit.  A wave walks its unit 64 voxels at a time, in
// order; the voxels of one slot within such a round are ranked with a ballot (lower lanes first), so that a running counter per
// slot gives every voxel its position among the voxels of its class in C order.  The counters live in registers: slot s in lane
// s % 64, register s / 64.  Pass 0 (WRITE = false) leaves the per-unit counts, the scan turns them into exclusive offsets, pass 1
// starts each counter at base[slot] + offset[slot][unit] and writes the linear indices.  Workspace: int64 base[257], then
// int32 off[nslots][nunits].
#define PP_NOSLOT 255
#define PP_BASE_ENTRIES 257

__device__ __forceinline__ int pp_slot(float f, const uint8_t* __restrict__ table, int L, int nslots) {
  if (!(f >= 0.f && f < (float)L)) return PP_NOSLOT;
  const int lab = (int)f;
  if ((float)lab != f) return PP_NOSLOT;
  const int s = table[lab];
  return s < nslots ? s : PP_NOSLOT;
}

struct LabelParams {
  const float* seg; long V; const uint8_t* table; int L, nslots; long nunits;
  int64_t* base; int32_t* off; int32_t* idx; long cap;
};

template <bool WRITE>
__global__ __launch_bounds__(PP_THREADS) void label_units_kernel(const LabelParams P) {
  const int lane = threadIdx.x % MT_WAVE;
  const uint64_t lower = (1ull << lane) - 1ull;
  for (long unit = (long)blockIdx.x * PP_WAVES + threadIdx.x / MT_WAVE; unit < P.nunits; unit += (long)gridDim.x * PP_WAVES) {
    int32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = WRITE ? -1 : 0;
    const long v0 = unit * MT_PP_UNIT, vend = mt_unit_end(v0, P.V);
    for (long vb = v0; vb < vend; vb += 4 * MT_WAVE) {
      float f[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {                          // four independent loads in flight, then four ordered rounds
        const long v = vb + r * MT_WAVE + lane;
        f[r] = v < vend ? P.seg[v] : -1.f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long v = vb + r * MT_WAVE + lane;
        const int slot = pp_slot(f[r], P.table, P.L, P.nslots);
        uint64_t todo = __ballot(slot != PP_NOSLOT);
        while (todo) {
          const int s = __shfl(slot, __ffsll((unsigned long long)todo) - 1, MT_WAVE);      // uniform: the first pending lane's slot
          const uint64_t m = __ballot(slot == s);
          const int hi = s >> 6, owner = s & 63;
          const int32_t mine = hi == 0 ? c[0] : hi == 1 ? c[1] : hi == 2 ? c[2] : c[3];
          int32_t cur = __shfl(mine, owner, MT_WAVE);
          if (WRITE) {
            if (cur < 0) cur = (int32_t)P.base[s] + P.off[(size_t)s * P.nunits + unit];
            if (slot == s) {
              const long pos = (long)cur + __popcll(m & lower);
              if (pos < P.cap) P.idx[pos] = (int32_t)v;
            }
          }
          const int32_t next = cur + (int32_t)__popcll(m);
          // four selects, no branches: the if / else chain on the uniform `hi` was compiled (ROCm 7 hipcc, -O3) so that hi == 3
          // stored into c[0] and left c[3] alone, and slots 192..254 were never counted (tests/test_datapath_kernels_gpu.py)
          const bool own = lane == owner;
#pragma unroll
          for (int k = 0; k < 4; ++k) c[k] = (own && hi == k) ? next : c[k];
          todo &= ~m;
        }
      }
    }
    if (!WRITE) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int s = k * MT_WAVE + lane;
        if (s < P.nslots) P.off[(size_t)s * P.nunits + unit] = c[k];
      }
    }
  }
}

// One block per slot: counts of the units -> exclusive offsets in place, total -> counts[slot].
__global__ __launch_bounds__(MT_SCAN_THREADS) void label_scan_kernel(int32_t* __restrict__ off, long nunits, int64_t* __restrict__ counts) {
  const int64_t total = mt_scan_units(off + (size_t)blockIdx.x * nunits, nunits);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ void label_base_kernel(const int64_t* __restrict__ counts, int nslots, int64_t* __restrict__ base) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int64_t run = 0;
    for (int s = 0; s < nslots; ++s) { base[s] = run; run += counts[s]; }
    base[nslots] = run;
  }
}

__global__ __launch_bounds__(PP_THREADS) void label_gather_kernel(const int32_t* __restrict__ idx, long cap, const int64_t* __restrict__ base,
                                                                  int nslots, const int32_t* __restrict__ qslot, const int64_t* __restrict__ qrank,
                                                                  long nq, int H, int W, int64_t* __restrict__ out) {
  for (long i = (long)blockIdx.x * PP_THREADS + threadIdx.x; i < nq; i += (long)gridDim.x * PP_THREADS) {
    const int s = qslot[i];
    const int64_t r = qrank[i];
    int64_t x = -1, y = -1, z = -1;
    if (s >= 0 && s < nslots && r >= 0 && base[s] + r < base[s + 1] && base[s] + r < cap) {
      const uint32_t p = (uint32_t)idx[base[s] + r], hw = (uint32_t)H * (uint32_t)W;
      x = p / hw;
      const uint32_t rem = p - (uint32_t)x * hw;
      y = rem / (uint32_t)W;
      z = rem - (uint32_t)y * (uint32_t)W;
    }
    out[3 * i] = x; out[3 * i + 1] = y; out[3 * i + 2] = z;
  }
}

extern "C" size_t mt_label_counts_workspace(long V, int nslots) {
  if (V < 1 || nslots < 1) return 0;
  return PP_BASE_ENTRIES * sizeof(int64_t) + (size_t)nslots * mt_units(V) * sizeof(int32_t);
}

static int pp_label_args(const char* who, const float* seg, long V, const uint8_t* table, int L, int nslots, void* ws, size_t ws_bytes) {
  MT_REQUIRE(seg && table && ws, "%s: null pointer", who);
  MT_REQUIRE(V > 0 && L >= 1 && nslots >= 1 && nslots <= 255, "%s: bad arguments (V %ld, table of %d, %d classes; at most 255)", who, V, L, nslots);
  MT_REQUIRE(V <= (long)INT32_MAX, "%s: %ld voxels exceed the int32 index range", who, V);
  MT_REQUIRE(((uintptr_t)seg & 3) == 0 && ((uintptr_t)ws & 7) == 0, "%s: misaligned pointer", who);
  MT_REQUIRE_WORKSPACE(who, ws_bytes, mt_label_counts_workspace(V, nslots));
  return MT_OK;
}

extern "C" int mt_label_counts(const float* seg, long V, const uint8_t* table, int L, int nslots, int64_t* counts, void* ws, size_t ws_bytes,
                               mt_stream_t stream) {
  const int rc = pp_label_args("label_counts", seg, V, table, L, nslots, ws, ws_bytes);
  if (rc != MT_OK) return rc;
  MT_REQUIRE(counts && ((uintptr_t)counts & 7) == 0, "label_counts: counts must be an 8-byte aligned device pointer");
  LabelParams P;
  P.seg = seg; P.V = V; P.table = table; P.L = L; P.nslots = nslots; P.nunits = mt_units(V);
  P.base = (int64_t*)ws; P.off = (int32_t*)((int64_t*)ws + PP_BASE_ENTRIES); P.idx = nullptr; P.cap = 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(label_units_kernel<false>, dim3(mt_stream_blocks(P.nunits, PP_WAVES)), dim3(PP_THREADS), 0, s, P);
  hipLaunchKernelGGL(label_scan_kernel, dim3(nslots), dim3(MT_SCAN_THREADS), 0, s, P.off, P.nunits, counts);
  hipLaunchKernelGGL(label_base_kernel, dim3(1), dim3(1), 0, s, (const int64_t*)counts, nslots, P.base);
  MT_CHECK_LAUNCH("label_counts");
  return MT_OK;
}

extern "C" int mt_label_locations(const float* seg, int D, int H, int W, const uint8_t* table, int L, int nslots, void* ws, size_t ws_bytes,
                                  int32_t* idx, long idx_capacity, const int32_t* qslot, const int64_t* qrank, long nq, int64_t* out,
                                  mt_stream_t stream) {
  MT_REQUIRE(D > 0 && H > 0 && W > 0, "label_locations: bad shape %d x %d x %d", D, H, W);
  const long V = (long)D * H * W;
  const int rc = pp_label_args("label_locations", seg, V, table, L, nslots, ws, ws_bytes);
  if (rc != MT_OK) return rc;
  MT_REQUIRE(idx && qslot && qrank && out && nq > 0 && idx_capacity > 0 && idx_capacity <= V, "label_locations: bad arguments");
  MT_REQUIRE(((uintptr_t)idx & 3) == 0 && ((uintptr_t)qslot & 3) == 0 && ((uintptr_t)qrank & 7) == 0 && ((uintptr_t)out & 7) == 0,
             "label_locations: misaligned pointer");
  LabelParams P;
  P.seg = seg; P.V = V; P.table = table; P.L = L; P.nslots = nslots; P.nunits = mt_units(V);
  P.base = (int64_t*)ws; P.off = (int32_t*)((int64_t*)ws + PP_BASE_ENTRIES); P.idx = idx; P.cap = idx_capacity;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(label_units_kernel<true>, dim3(mt_stream_blocks(P.nunits, PP_WAVES)), dim3(PP_THREADS), 0, s, P);
  hipLaunchKernelGGL(label_gather_kernel, dim3(mt_stream_blocks(nq, PP_THREADS)), dim3(PP_THREADS), 0, s, (const int32_t*)idx, idx_capacity,
                     (const int64_t*)P.base, nslots, qslot, qrank, nq, H, W, out);
  MT_CHECK_LAUNCH("label_locations");
  return MT_OK;
}
