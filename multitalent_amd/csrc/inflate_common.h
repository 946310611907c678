// inflate_common.h — what the INFLATE units (inflate.hip, inflate_spec.hip) share: statuses, the code tables of one decoding wave,
// canonical decoding, the wave-uniform bit reader and the reading of a block's two codes.  See inflate.hip for the decoding wave.
#pragma once
#include "stream_common.h"

#define IF_WAVE 64
#define IF_FASTL 10                                  // bits that index the literal/length table; longer codes walk the counts
#define IF_FASTD 8

enum { IF_OK = 0, IF_FOREIGN = 1, IF_TOO_LONG = 2, IF_BAD = 3, IF_CORRUPT = 4, IF_SIZE = 5 };

struct IfTables {
  uint16_t fastl[1 << IF_FASTL];    // low bits of the stream -> symbol | code length << 9; 0: a longer code (or none)
  uint16_t fastd[1 << IF_FASTD];
  uint16_t syml[288], symd[32], symc[20];          // symbols ordered by (code length, symbol)
  uint16_t cntl[16], cntd[16], cntc[16], offs[16]; // codes of each length
  uint8_t lens[320];
  int ok;
};

__device__ static const uint8_t IF_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// canonical decoding of the code whose bits arrive lowest first in v: -> symbol (its length in len), -1 when no code of at most
// maxlen bits matches
__device__ __forceinline__ int if_walk(const uint16_t* cnt, const uint16_t* sym, uint64_t v, int maxlen, int& len) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= maxlen; ++l) {
    code |= (int)(v & 1u);
    v >>= 1;
    const int c = cnt[l];
    if (code - c < first) { len = l; return sym[index + (code - first)]; }
    index += c; first += c; first <<= 1; code <<= 1;
  }
  len = 0;
  return -1;
}

// lens[0, n) -> cnt, sym and (fastbits > 0) the table; false when the lengths are over-subscribed.  All lanes call it.
__device__ __forceinline__ bool if_build(IfTables& T, const uint8_t* lens, int n, uint16_t* cnt, uint16_t* sym, uint16_t* fast,
                                         int fastbits, int lane) {
  __syncthreads();
  if (lane == 0) {
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int s = 0; s < n; ++s) ++cnt[lens[s] & 15];
    int left = 1, o = 0;
    bool ok = true;
    for (int l = 1; l < 16; ++l) { left = (left << 1) - cnt[l]; if (left < 0) { ok = false; break; } }
    for (int l = 1; l < 16; ++l) { T.offs[l] = (uint16_t)o; o += cnt[l]; }
    if (ok)
      for (int s = 0; s < n; ++s) { const int l = lens[s] & 15; if (l) sym[T.offs[l]++] = (uint16_t)s; }
    T.ok = ok ? 1 : 0;
  }
  __syncthreads();
  const bool ok = T.ok != 0;
  if (ok && fastbits)
    for (int e = lane; e < (1 << fastbits); e += IF_WAVE) {
      int len;
      const int s = if_walk(cnt, sym, (uint64_t)e, fastbits, len);
      fast[e] = s < 0 ? (uint16_t)0 : (uint16_t)(s | (len << 9));
    }
  __syncthreads();
  return ok;
}

// The input as every lane sees it: a bit buffer of up to 64 bits in front of byte `ip`; bytes behind the end read as zero and
// `used()` tells when they were consumed.
struct IfIn {
  const uint8_t* in; long n, ip, wbase; uint64_t bb; int nb, lane; uint32_t w;
  __device__ __forceinline__ void open(const uint8_t* p, long n_, long at, int lane_) {
    in = p; n = n_; ip = at; bb = 0; nb = 0; lane = lane_; w = 0; wbase = -(1l << 40);
  }
  __device__ __forceinline__ void window(long at) {                   // 64 aligned dwords from the one that holds byte `at`
    wbase = at - (long)(((uintptr_t)in + (uintptr_t)at) & 3);
    const long p = wbase + 4 * lane;
    uint32_t v = 0;
    if (p >= 0 && p + 4 <= n) v = *(const uint32_t*)(in + p);
    else {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (p + k >= 0 && p + k < n) v |= (uint32_t)in[p + k] << (8 * k);
    }
    w = v;
  }
  __device__ __forceinline__ uint32_t word32(long at) {
    if (at >= n) return 0;
    long a = at - wbase;
    if (a < 0 || a + 8 > 4 * IF_WAVE) { window(at); a = at - wbase; }
    const int i = (int)(a >> 2), sh = (int)(a & 3) * 8;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)w, i), hi = (uint32_t)__builtin_amdgcn_readlane((int)w, i + 1);
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
  }
  __device__ __forceinline__ void refill() { if (nb <= 32) { bb |= (uint64_t)word32(ip) << nb; ip += 4; nb += 32; } }
  __device__ __forceinline__ uint32_t take(int k) { const uint32_t v = (uint32_t)bb & ((1u << k) - 1u); bb >>= k; nb -= k; return v; }
  __device__ __forceinline__ uint32_t get(int k) { refill(); return take(k); }                  // k <= 16
  __device__ __forceinline__ void align() { const int k = nb & 7; bb >>= k; nb -= k; }
  __device__ __forceinline__ long byte_pos() const { return ip - (nb >> 3); }                   // after align()
  __device__ __forceinline__ void seek(long at) { ip = at; bb = 0; nb = 0; }
  __device__ __forceinline__ bool overrun() const { return 8 * ip - nb > 8 * n; }
};
