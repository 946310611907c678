// Normalized surface Dice on the device (evaluation/surface_dice.py of the reference): the distances mt_surface_distances (metrics.hip)
// left in device memory, counted against up to 8 tolerances where they lie.  The metric itself is host arithmetic on the counts.
#include "stream_common.h"

#define SDC_THREADS 256

// mt_sd_count_within: counts[s][t] = #{i in segment s : x[i] <= tol[t]} over the array mt_surface_distances wrote, segment 0 =
// [0, n_tr), segment 1 = [n_tr, n_tr + n_rt).  One pass, 8 bytes read per element and nothing else.  A segment's body is read as
// 16-byte pairs from its first 16-byte aligned element on (n_tr may be odd: the second segment can start 8 bytes off), the element
// before and the element after the pairs are single loads of global threads 0 and 1.  Counts stay in registers, are summed over the
// wave with shuffles, over the workgroup's four waves through 32 T bytes of LDS, and leave as one 64-bit atomicAdd per workgroup,
// segment and tolerance that counted anything: integer sums, the same from run to run.  (One atomicAdd per WAVE was measured
// first: every add of a segment goes to one address, and 16 384 of them took 0.20 ms whatever the length of the array.)
#define SDC_MAXTOL 8
struct SdcTols { double t[SDC_MAXTOL]; };

template <int T>
__global__ __launch_bounds__(SDC_THREADS) void sd_count_within_kernel(const double* __restrict__ x, long n_tr, long n, const SdcTols tol,
                                                                     unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long part[SDC_THREADS / MT_WAVE][T];
  const long gtid = (long)blockIdx.x * SDC_THREADS + threadIdx.x, gstride = (long)gridDim.x * SDC_THREADS;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const long lo = s ? n_tr : 0, hi = s ? n : n_tr;
    if (lo >= hi) continue;                                            // uniform over the grid
    const long head = ((uintptr_t)(x + lo) & 15) ? 1 : 0;              // x is 8-byte aligned; hi - lo >= 1 >= head
    const long nvec = (hi - lo - head) >> 1, tail = (hi - lo - head) & 1;
    unsigned long long c[T];
#pragma unroll
    for (int k = 0; k < T; ++k) c[k] = 0;
    const double2* xv = (const double2*)(x + lo + head);               // pair i = elements lo + head + 2 i, + 1 <= hi - 1 - tail
    for (long i = gtid; i < nvec; i += gstride) {
      const double2 a = xv[i];
#pragma unroll
      for (int k = 0; k < T; ++k) c[k] += (a.x <= tol.t[k] ? 1u : 0u) + (a.y <= tol.t[k] ? 1u : 0u);
    }
    if ((gtid == 0 && head) || (gtid == 1 && tail)) {
      const double v = x[gtid == 0 ? lo : hi - 1];
#pragma unroll
      for (int k = 0; k < T; ++k) c[k] += v <= tol.t[k] ? 1u : 0u;
    }
#pragma unroll
    for (int k = 0; k < T; ++k) {
      unsigned long long sum = c[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, MT_WAVE);
      if (threadIdx.x % MT_WAVE == 0) part[threadIdx.x / MT_WAVE][k] = sum;
    }
    __syncthreads();
    if ((int)threadIdx.x < T) {
      unsigned long long sum = 0;
#pragma unroll
      for (int w = 0; w < SDC_THREADS / MT_WAVE; ++w) sum += part[w][threadIdx.x];
      if (sum) atomicAdd(counts + s * T + threadIdx.x, sum);
    }
    __syncthreads();                                                   // part is written again for the second segment
  }
}

template <int T>
static void sdc_launch(const double* x, long n_tr, long n, const SdcTols& tol, int64_t* counts, hipStream_t s) {
  hipLaunchKernelGGL(sd_count_within_kernel<T>, dim3(mt_stream_blocks(n / 2, SDC_THREADS)), dim3(SDC_THREADS), 0, s, x, n_tr, n, tol,
                     (unsigned long long*)counts);
}

extern "C" int mt_sd_count_within(const double* sds, long n_tr, long n_rt, const double* tols, int T, int64_t* counts, mt_stream_t stream) {
  MT_REQUIRE(sds && tols && counts, "sd_count_within: null pointer");
  MT_REQUIRE(T >= 1 && T <= SDC_MAXTOL, "sd_count_within: %d tolerances (1..%d)", T, SDC_MAXTOL);
  MT_REQUIRE(n_tr >= 0 && n_rt >= 0 && n_tr <= INT64_MAX - n_rt && n_tr + n_rt >= 1, "sd_count_within: bad segment lengths %ld, %ld", n_tr,
             n_rt);
  SdcTols tol;
  for (int k = 0; k < SDC_MAXTOL; ++k) tol.t[k] = 0.0;
  for (int k = 0; k < T; ++k) {
    MT_REQUIRE(tols[k] >= 0.0, "sd_count_within: tolerance %d is %g (a number >= 0 or +inf)", k, tols[k]);       // false for NaN
    tol.t[k] = tols[k];
  }
  MT_REQUIRE(((uintptr_t)sds & 7) == 0 && ((uintptr_t)counts & 7) == 0, "sd_count_within: misaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, sizeof(int64_t) * 2 * T, s) != hipSuccess) {
    mt_set_error("sd_count_within: hipMemsetAsync failed");
    return MT_EHIP;
  }
  const long n = n_tr + n_rt;
  switch (T) {
    case 1: sdc_launch<1>(sds, n_tr, n, tol, counts, s); break;
    case 2: sdc_launch<2>(sds, n_tr, n, tol, counts, s); break;
    case 3: sdc_launch<3>(sds, n_tr, n, tol, counts, s); break;
    case 4: sdc_launch<4>(sds, n_tr, n, tol, counts, s); break;
    case 5: sdc_launch<5>(sds, n_tr, n, tol, counts, s); break;
    case 6: sdc_launch<6>(sds, n_tr, n, tol, counts, s); break;
    case 7: sdc_launch<7>(sds, n_tr, n, tol, counts, s); break;
    default: sdc_launch<8>(sds, n_tr, n, tol, counts, s); break;
  }
  MT_CHECK_LAUNCH("sd_count_within");
  return MT_OK;
}
