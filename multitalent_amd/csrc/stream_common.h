// What the data-path units (postproc, metrics, crop, preproc, analyze, select) share: the grid of a streaming launch, the 256-bit
// label membership, the dword-aligned 16-byte load type and the bookkeeping of the MT_PP_UNIT compactions.
#pragma once
#include "mt_common.h"

// ---- grid of a streaming launch: one block per `per_block` items until the chip holds 8 blocks per CU, a grid-stride loop beyond ----
static inline long mt_stream_cap() { return mt_device_cus(mt_current_device()) * 8; }
static inline int mt_stream_blocks(long items, int per_block) {
  const long cap = mt_stream_cap(), b = mt_cdiv(items, per_block);
  return (int)(b < cap ? (b > 1 ? b : 1) : cap);
}

// ---- 256-bit membership of the uint8 labels ----
struct MtMember { uint32_t bits[8]; };
__device__ __forceinline__ bool mt_member(const MtMember& m, uint8_t v) { return (m.bits[v >> 5] >> (v & 31)) & 1u; }
static inline MtMember mt_member_from_bytes(const uint8_t member[256]) {      // non-zero byte = in the set
  MtMember m;
  for (int k = 0; k < 8; ++k) m.bits[k] = 0;
  for (int k = 0; k < 256; ++k) if (member[k]) m.bits[k >> 5] |= 1u << (k & 31);
  return m;
}

// 16 bytes that are only dword aligned (channel c of a case starts at data + c * V, its label map is the last channel): gfx950 serves
// a dword-aligned global_load_dwordx4.
struct __attribute__((packed, aligned(4))) mt_f4 { float x, y, z, w; };

// ---- units of MT_PP_UNIT consecutive voxels (ordered compactions: per-unit counts, exclusive scan, ranks inside a unit) ----
static inline long mt_units(long V) { return (V + MT_PP_UNIT - 1) / MT_PP_UNIT; }
__device__ __forceinline__ long mt_unit_end(long v0, long V) { return v0 + MT_PP_UNIT < V ? v0 + MT_PP_UNIT : V; }

// One workgroup of MT_SCAN_THREADS: the counts p[0 .. nunits) become their exclusive prefix sums in place; thread 0 gets the total
// (the others 0).  Thread t owns a contiguous run of units; the runs are combined in thread order.
#define MT_SCAN_THREADS 256
__device__ __forceinline__ int64_t mt_scan_units(int32_t* __restrict__ p, long nunits) {
  const long per = (nunits + MT_SCAN_THREADS - 1) / MT_SCAN_THREADS;
  const long b = threadIdx.x * per, e = b + per < nunits ? b + per : nunits;
  long sum = 0, total = 0;
  for (long u = b; u < e; ++u) sum += p[u];
  __shared__ long sh[MT_SCAN_THREADS];
  sh[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 0; t < MT_SCAN_THREADS; ++t) { const long n = sh[t]; sh[t] = total; total += n; }
  }
  __syncthreads();
  long run = sh[threadIdx.x];
  for (long u = b; u < e; ++u) { const int32_t n = p[u]; p[u] = (int32_t)run; run += n; }
  return total;
}
