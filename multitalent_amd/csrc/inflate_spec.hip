// inflate_spec.hip — INFLATE of a raw DEFLATE stream that has no restart points (a file of another writer: zlib, numpy, gzip, pigz),
// parallel over block starts that are FOUND in the stream.  The byte-aligned decoder (inflate.hip) refuses such a stream; this one
// is what the readers try next.
//
// A UNIT starts at a BIT position that is a candidate, decodes consecutive blocks and ends at the first block end that is a
// candidate's position, or at a block with BFINAL (the stream ends at the next byte boundary).  Matches may reach up to 32 768 bytes
// in front of their unit: the unit is first decoded into 16-bit SYMBOLS (a byte, or a marker 0x8000 | index into the window of
// the 32 768 bytes in front of the unit), the windows are then resolved one after the other, and the symbols last.
//   mt_inflate_spec_scan   search: bit 0, and per chunk of compressed bytes the first bit position at which the header of a
//                          non-final dynamic block is accepted (as strictly as zlib accepts one), 64 positions per wave step;
//                          size pass: one wave per candidate decodes without output -> end, bytes, stored blocks, reach, status;
//                          chain: one wave follows end -> start from bit 0 (64 candidates per step where each ends at the next
//                          one), which by induction holds true units only, and takes the exclusive scan of their sizes.
//   mt_inflate_spec_write  the stored blocks of the chained units are listed as spans and copied (widened) by the whole grid; one wave
//                          per unit decodes into its range of symbols through an LDS ring; one workgroup walks the units and keeps
//                          every unit's closing window; the whole grid resolves symbols to bytes in 16-byte stores.
// The result never depends on what the search proposes: bit 0 starts a unit, a true unit ends where the next true unit starts, and
// candidates the chain does not reach are ignored.  Restated in tests/inflate_spec_host.py.
#include "inflate_common.h"

#define SP_RB 4096                                   // ring symbols (a power of two)
#define SP_FLUSH 2048                                // unflushed symbols at which the ring is written out; SP_FLUSH + 258 <= SP_RB
#define SP_WIN 32768                                 // the window: the farthest a match reaches
#define SP_HEAD_BYTES 64
#define SP_MAX_UNIT_LIMIT (1l << 30)
#define SP_MIN_CHUNK 64
#define SP_MAX_CHUNK (1 << 20)
#define SP_WIN_THREADS 1024
#define SP_WIN_PER (SP_WIN / SP_WIN_THREADS)         // window bytes per thread: 32

enum { SP_MODE_SIZE = 0, SP_MODE_SPANS = 1, SP_MODE_WRITE = 2 };
enum { SP_STEP_SEARCH = 1, SP_STEP_SIZE = 2, SP_STEP_CHAIN = 4, SP_STEP_SYMBOLS = 1, SP_STEP_WINDOWS = 2, SP_STEP_RESOLVE = 4 };

struct SpHead { int32_t status, n_units; int64_t total; int32_t n_cand, n_spans, max_reach; uint32_t shortest; };
struct SpRes { int64_t end; uint32_t out; int32_t nspans, flags, reach; };     // end: a bit position; flags: status | final << 3
struct SpSpan { int64_t dst; int32_t src, len; };

// scan workspace: [head 64][index i32 x nch][first i64 x nch][cand i64 x cap][res 24 x cap][unit_cand i32 x cap][unit_span i32 x cap]
//                 [unit_out i64 x cap], every part 16-byte aligned.  nch = chunks of the input, cap = nch + 1 (bit 0 and one per chunk).
struct SpLayout {
  long nch, cap;
  int lg;
  size_t index, first, cand, res, ucand, uspan, uout, bytes;
};
static inline size_t sp_al(size_t v) { return (v + 15) & ~(size_t)15; }
static inline bool sp_n_ok(long n) { return n >= 1 && n <= 2147483647l - 64; }
static inline bool sp_chunk_ok(int chunk) { return chunk >= SP_MIN_CHUNK && chunk <= SP_MAX_CHUNK && (chunk & (chunk - 1)) == 0; }
static inline SpLayout sp_layout(long n, int chunk) {
  SpLayout L;
  L.lg = 0;
  while ((1 << L.lg) < chunk) ++L.lg;
  L.nch = (n + chunk - 1) >> L.lg;
  L.cap = L.nch + 1;
  L.index = SP_HEAD_BYTES;
  L.first = L.index + sp_al(4 * (size_t)L.nch);
  L.cand = L.first + sp_al(8 * (size_t)L.nch);
  L.res = L.cand + sp_al(8 * (size_t)L.cap);
  L.ucand = L.res + sp_al(sizeof(SpRes) * (size_t)L.cap);
  L.uspan = L.ucand + sp_al(4 * (size_t)L.cap);
  L.uout = L.uspan + sp_al(4 * (size_t)L.cap);
  L.bytes = L.uout + sp_al(8 * (size_t)L.cap);
  return L;
}
// write workspace: [symbols u16 x n_out][windows SP_WIN x n_units][spans 16 x n_spans]
struct SpWriteLayout { size_t win, spans, bytes; };
static inline SpWriteLayout sp_write_layout(long n_units, long n_spans, long n_out) {
  SpWriteLayout L;
  L.win = sp_al(2 * (size_t)n_out);
  L.spans = L.win + (size_t)SP_WIN * (size_t)n_units;
  L.bytes = L.spans + 16 * (size_t)n_spans;
  return L;
}

// ------------------------------------------------------------------------------------------------ search
// at least 57 bits of the stream from bit position `bit`, lowest first; bytes behind the input read as zero.  Every lane on its own.
__device__ __forceinline__ uint64_t sp_bits(const uint8_t* __restrict__ comp, long n, int64_t bit) {
  const long b = (long)(bit >> 3);
  uint64_t v = 0;
  if (b + 8 <= n) __builtin_memcpy(&v, comp + b, 8);
  else {
#pragma unroll
    for (int k = 0; k < 8; ++k) if (b + k < n) v |= (uint64_t)comp[b + k] << (8 * k);
  }
  return v >> (bit & 7);
}

// Kraft sums in units of 2^-15 of the two codes while their lengths arrive: `rep` lengths of value `val` from index i on
struct SpSums {
  uint32_t kl, kd; int bigl, bigd, eob, hlit;
  __device__ __forceinline__ void add(int i, int val, int rep) {
    if (val == 0) return;
    int nl = hlit - i;
    nl = nl < 0 ? 0 : nl > rep ? rep : nl;
    kl += (uint32_t)nl << (15 - val);
    kd += (uint32_t)(rep - nl) << (15 - val);
    if (val > 1) { if (nl) bigl = 1; if (rep - nl) bigd = 1; }
    if (i <= 256 && 256 < i + rep) eob = 1;
  }
};
// complete, or all codes at most one bit long and not over-subscribed (what zlib's inflate_table lets pass)
__device__ __forceinline__ bool sp_code_ok(uint32_t k, int big) { return k == 32768u || (!big && k < 32768u); }

// Is bit position p the header of a non-final dynamic block that zlib's inflate would accept?  Everything in registers: the 19 lengths
// of the code-length code are 3 bits each in one word, its symbols in (length, symbol) order 5 bits each in two, its counts 8 bits each.
__device__ __forceinline__ bool sp_accept(const uint8_t* __restrict__ comp, long n, int64_t p) {
  const int64_t nbits = 8 * (int64_t)n;
  uint64_t v = sp_bits(comp, n, p);
  if ((v & 7u) != 4u) return false;                                    // BFINAL 0, BTYPE 2
  const int hlit = (int)((v >> 3) & 31u) + 257, hdist = (int)((v >> 8) & 31u) + 1, hclen = (int)((v >> 13) & 15u) + 4;
  if (hlit > 286 || hdist > 30) return false;
  int64_t q = p + 17;
  if (q + 3 * hclen > nbits) return false;
  v = sp_bits(comp, n, q);
  uint64_t cl = 0;
  int kraft = 0;
  for (int k = 0; k < hclen; ++k) {
    const uint32_t l = (uint32_t)(v >> (3 * k)) & 7u;
    cl |= (uint64_t)l << (3 * IF_ORDER[k]);
    if (l) kraft += 128 >> l;
  }
  if (kraft != 128) return false;                                      // the code-length code is complete
  q += 3 * hclen;
  uint64_t cnt = 0, s0 = 0, s1 = 0;
  int m = 0;
  for (int l = 1; l <= 7; ++l)
    for (int s = 0; s < 19; ++s)
      if (((uint32_t)(cl >> (3 * s)) & 7u) == (uint32_t)l) {
        if (m < 12) s0 |= (uint64_t)s << (5 * m); else s1 |= (uint64_t)s << (5 * (m - 12));
        ++m;
        cnt += 1ull << (8 * l);
      }
  SpSums S; S.kl = 0; S.kd = 0; S.bigl = 0; S.bigd = 0; S.eob = 0; S.hlit = hlit;
  const int total = hlit + hdist;
  int i = 0, prev = 0;
  while (i < total) {
    v = sp_bits(comp, n, q);
    int code = 0, first = 0, index = 0, len = 0, sym = -1;
    for (int l = 1; l <= 7; ++l) {
      code |= (int)(v & 1u);
      v >>= 1;
      const int c = (int)(cnt >> (8 * l)) & 255;
      if (code - c < first) {
        const int at = index + (code - first);
        sym = at < 12 ? (int)(s0 >> (5 * at)) & 31 : (int)(s1 >> (5 * (at - 12))) & 31;
        len = l;
        break;
      }
      index += c; first += c; first <<= 1; code <<= 1;
    }
    if (sym < 0) return false;
    q += len;
    if (sym < 16) { S.add(i, sym, 1); prev = sym; ++i; }
    else {
      int rep, val = 0;
      if (sym == 16) { if (i == 0) return false; val = prev; rep = 3 + (int)(v & 3u); q += 2; }
      else if (sym == 17) { rep = 3 + (int)(v & 7u); q += 3; }
      else { rep = 11 + (int)(v & 127u); q += 7; }
      if (i + rep > total) return false;
      S.add(i, val, rep);
      prev = val; i += rep;
    }
    if (q > nbits) return false;                                       // a header bit behind the input
  }
  return S.eob && sp_code_ok(S.kl, S.bigl) && sp_code_ok(S.kd, S.bigd);
}

// One wave per chunk: first[k] = the first accepted bit position p > 0 in chunk k (-1: none), index[k] = whether there is one
__global__ __launch_bounds__(IF_WAVE) void inflate_spec_search_kernel(const uint8_t* __restrict__ comp, long n, int lg, long nch,
                                                                      int64_t* __restrict__ first, int32_t* __restrict__ index) {
  const int lane = threadIdx.x;
  const int64_t nbits = 8 * (int64_t)n;
  for (long k = blockIdx.x; k < nch; k += gridDim.x) {
    const int64_t b0 = 8 * ((int64_t)k << lg);
    int64_t b1 = 8 * ((int64_t)(k + 1) << lg);
    if (b1 > nbits) b1 = nbits;
    int64_t found = -1;
    for (int64_t p = b0; p < b1 && found < 0; p += IF_WAVE) {
      const int64_t me = p + lane;
      const bool a = me > 0 && me < b1 && sp_accept(comp, n, me);
      const unsigned long long m = __ballot(a);
      if (m) found = p + (__ffsll((long long)m) - 1);
    }
    if (lane == 0) { first[k] = found; index[k] = found >= 0 ? 1 : 0; }
  }
}

__global__ __launch_bounds__(MT_SCAN_THREADS) void inflate_spec_scan_kernel(int32_t* __restrict__ index, long nch, SpHead* __restrict__ head) {
  const int64_t total = mt_scan_units(index, nch);
  if (threadIdx.x == 0) {
    head->status = IF_OK; head->n_cand = (int32_t)(total + 1);
    head->n_units = 0; head->total = 0; head->n_spans = 0; head->max_reach = 0; head->shortest = 0;
  }
}

__global__ __launch_bounds__(256) void inflate_spec_compact_kernel(const int64_t* __restrict__ first, const int32_t* __restrict__ index,
                                                                   long nch, int64_t* __restrict__ cand) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k == 0) cand[0] = 0;
  if (k < nch && first[k] >= 0) cand[1 + index[k]] = first[k];
}

// the candidate that starts at bit position e > 0: its index, or -1
__device__ __forceinline__ int sp_lookup(const int64_t* __restrict__ first, const int32_t* __restrict__ index, int lg, long nch, int64_t e) {
  const long k = (long)((e >> 3) >> lg);
  return k < nch && first[k] == e ? 1 + index[k] : -1;
}

// ------------------------------------------------------------------------------------------------ one unit
struct SpSharedSize { IfTables T; };
struct SpSharedWrite { uint16_t ring[SP_RB] __attribute__((aligned(16))); IfTables T; };

// The ring of a unit that is written: symbol q of the unit lives in ring[(bias + q) & (SP_RB - 1)], bias = the low bits of its index
// in the symbol array (which is 16-byte aligned), so that 8 symbols of the ring are 16 bytes of memory.
struct SpOut {
  uint16_t* ring; uint16_t* obase; uint32_t bias, pos, flushed, ring_lo; int lane;
  __device__ __forceinline__ uint32_t slot(uint32_t q) const { return (bias + q) & (SP_RB - 1); }
  __device__ __forceinline__ void flush(bool all) {
    __syncthreads();
    uint32_t a1 = pos;
    if (!all) {
      const uint32_t tail = (bias + pos) & 7u;
      if (pos < flushed + tail) return;
      a1 = pos - tail;
    }
    uint32_t q = flushed;
    uint32_t head = (8u - ((bias + q) & 7u)) & 7u;
    if (head > a1 - q) head = a1 - q;
    if ((uint32_t)lane < head) obase[q + lane] = ring[slot(q + lane)];
    q += head;
    const uint32_t nv = (a1 - q) >> 3;
    for (uint32_t k = lane; k < nv; k += IF_WAVE) *(uint4*)(obase + q + 8 * k) = *(const uint4*)(ring + slot(q + 8 * k));
    q += 8 * nv;
    if ((uint32_t)lane < a1 - q) obase[q + lane] = ring[slot(q + lane)];
    flushed = a1;
    __threadfence();                                                  // far matches read these symbols back
    __syncthreads();
  }
};

// Decodes the unit that starts at bit `start`.  SIZE: no output.  SPANS: its first `want` non-empty stored blocks go to spans[] (dst
// from out0), then it stops.  WRITE: the Huffman-coded symbols go to obase[0, limit), the stored blocks are skipped (they are copied
// as spans beforehand).  All lanes run the same path.  Every iteration of every loop consumes at least one bit and stops behind the
// input, so a false candidate, which decodes garbage, ends too.
template <int MODE>
__device__ __forceinline__ SpRes sp_unit(IfTables& T, uint16_t* ring, const uint8_t* __restrict__ comp, long n, int64_t start,
                                         uint32_t unit_limit, int64_t span_bits, int lg, long nch, const int64_t* __restrict__ first,
                                         SpSpan* __restrict__ spans, int want, int64_t out0, uint16_t* obase, uint32_t limit) {
  const int lane = threadIdx.x;
  IfIn I; I.open(comp, n, (long)(start >> 3), lane);
  if (start & 7) I.get((int)(start & 7));
  SpOut O;
  O.ring = ring; O.obase = obase; O.bias = (uint32_t)out0 & (SP_RB - 1); O.pos = 0; O.flushed = 0; O.ring_lo = 0; O.lane = lane;
  uint32_t pos = 0;
  int nspans = 0, status = IF_OK, final = 0, reach = 0;
  int64_t end = start;
  for (;;) {                                                           // blocks
    final = (int)I.get(1);
    const int type = (int)I.get(2);
    if (type == 3 || I.overrun()) { status = IF_BAD; break; }
    if (type == 0) {
      I.align();
      I.refill();
      const uint32_t len = I.take(16);
      I.refill();
      const uint32_t nlen = I.take(16);
      const long data = I.byte_pos();
      if ((len ^ nlen) != 0xffffu || I.overrun() || data + (long)len > n) { status = IF_BAD; break; }
      if (len) {
        if (MODE == SP_MODE_SPANS) {
          if (lane == 0) { SpSpan s; s.dst = out0 + pos; s.src = (int32_t)data; s.len = (int32_t)len; spans[nspans] = s; }
          if (nspans + 1 == want) { ++nspans; break; }
        }
        if (MODE == SP_MODE_WRITE) {
          O.flush(true);
          if (pos + len > limit) { status = IF_CORRUPT; break; }
          O.pos = O.flushed = O.ring_lo = pos + len;
        }
        ++nspans;
        pos += len;
      }
      I.seek(data + len);
      end = 8 * (int64_t)(data + (long)len);
    } else {
#include "inflate_codes.inc"
      // ---- tokens
      for (;;) {
        I.refill();
        int len, sym;
        {
          const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)T.fastl[(uint32_t)I.bb & ((1u << IF_FASTL) - 1u)]);
          if (e) { sym = (int)(e & 511u); len = (int)(e >> 9); }
          else {
            sym = __builtin_amdgcn_readfirstlane(if_walk(T.cntl, T.syml, I.bb, 15, len));
            len = __builtin_amdgcn_readfirstlane(len);
          }
        }
        if (sym < 0 || sym > 285) { status = IF_BAD; break; }
        I.take(len);
        if (sym < 256) {
          if (MODE == SP_MODE_WRITE) {
            if (pos + 1 > limit) { status = IF_CORRUPT; break; }
            if (lane == 0) ring[O.slot(pos)] = (uint16_t)sym;
          }
          ++pos;
        } else if (sym == 256) {
          if (I.overrun()) status = IF_BAD;
          break;
        } else {
          uint32_t L, dist;
          if (sym < 265) L = (uint32_t)sym - 254u;
          else if (sym == 285) L = 258u;
          else { const int eb = (sym - 261) >> 2; L = 3u + ((4u + ((uint32_t)(sym - 265) & 3u)) << eb) + I.take(eb); }
          I.refill();
          int dsym;
          {
            const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)T.fastd[(uint32_t)I.bb & ((1u << IF_FASTD) - 1u)]);
            if (e) { dsym = (int)(e & 511u); len = (int)(e >> 9); }
            else {
              dsym = __builtin_amdgcn_readfirstlane(if_walk(T.cntd, T.symd, I.bb, 15, len));
              len = __builtin_amdgcn_readfirstlane(len);
            }
          }
          if (dsym < 0 || dsym > 29) { status = IF_BAD; break; }
          I.take(len);
          if (dsym < 4) dist = (uint32_t)dsym + 1u;
          else { const int eb = (dsym >> 1) - 1; dist = 1u + ((2u + ((uint32_t)dsym & 1u)) << eb) + I.take(eb); }
          if (dist > pos) {                                            // it reaches in front of the unit: nothing is there in front of bit 0
            if (start == 0) { status = IF_CORRUPT; break; }
            if ((int)(dist - pos) > reach) reach = (int)(dist - pos);
          }
          if (MODE == SP_MODE_WRITE) {
            if (pos + L > limit) { status = IF_CORRUPT; break; }
            __syncthreads();
            for (uint32_t k = lane; k < L; k += IF_WAVE) {
              const int32_t q = (int32_t)pos - (int32_t)dist + (int32_t)(k < dist ? k : k % dist);
              uint16_t s;
              if (q < 0) s = (uint16_t)(0x8000 | (SP_WIN + q));       // -q bytes in front of the unit: index into the window
              else if ((uint32_t)q >= O.ring_lo && pos + L - (uint32_t)q <= SP_RB) s = ring[O.slot((uint32_t)q)];
              else s = obase[q];                                       // flushed, or a stored block: q < O.flushed
              ring[O.slot(pos + k)] = s;
            }
          }
          pos += L;
        }
        if (I.overrun()) { status = IF_BAD; break; }
        if (pos > unit_limit || 8 * (int64_t)I.ip - I.nb - start > span_bits) { status = IF_TOO_LONG; break; }
        if (MODE == SP_MODE_WRITE) {
          O.pos = pos;
          if (pos - O.flushed >= SP_FLUSH) O.flush(false);
        }
      }
      if (status != IF_OK) break;
      end = 8 * (int64_t)I.ip - I.nb;
    }
    if (pos > unit_limit || end - start > span_bits) { status = IF_TOO_LONG; break; }
    if (final) { end = (end + 7) & ~(int64_t)7; break; }
    const long k = (long)((end >> 3) >> lg);                           // the unit ends where a candidate starts
    if (k < nch && first[k] == end) break;
  }
  if (MODE == SP_MODE_WRITE) { O.pos = pos < limit ? pos : limit; if (O.pos >= O.flushed) O.flush(true); }
  SpRes r;
  r.end = end; r.out = pos; r.nspans = nspans; r.flags = status | (final << 3); r.reach = reach;
  return r;
}

__global__ __launch_bounds__(IF_WAVE) void inflate_spec_size_kernel(const uint8_t* __restrict__ comp, long n, uint32_t unit_limit,
                                                                    int64_t span_bits, int lg, long nch, const SpHead* __restrict__ head,
                                                                    const int64_t* __restrict__ first, const int64_t* __restrict__ cand,
                                                                    SpRes* __restrict__ res) {
  __shared__ SpSharedSize S;
  if (head->status != IF_OK) return;
  const int ncand = head->n_cand;
  for (int c = blockIdx.x; c < ncand; c += gridDim.x) {
    const SpRes r = sp_unit<SP_MODE_SIZE>(S.T, nullptr, comp, n, cand[c], unit_limit, span_bits, lg, nch, first, nullptr, 0, 0, nullptr, 0u);
    if (threadIdx.x == 0) res[c] = r;
    __syncthreads();
  }
}

// One wave.  Lane j looks at candidate c + j: it LINKS when it decoded, is not final and ends where candidate c + j + 1 starts.
// The lanes in front of the first that does not link, and that lane, are units; the candidate at its end is looked up through the
// chunk the end falls in.
__global__ __launch_bounds__(IF_WAVE) void inflate_spec_chain_kernel(SpHead* __restrict__ head, const int64_t* __restrict__ first,
                                                                     const int32_t* __restrict__ index, int lg, long nch,
                                                                     const int64_t* __restrict__ cand, const SpRes* __restrict__ res,
                                                                     int32_t* __restrict__ ucand, int32_t* __restrict__ uspan,
                                                                     int64_t* __restrict__ uout, long n, long n_expect) {
  if (head->status != IF_OK) return;
  const int lane = threadIdx.x, ncand = head->n_cand;
  const int64_t nbits = 8 * (int64_t)n;
  int c = 0, k = 0, status = -1, reach = 0;
  uint32_t shortest = 0xffffffffu;
  int64_t total = 0;
  long spans = 0;
  while (status < 0) {
    const int ci = c + lane;
    const bool have = ci < ncand;
    SpRes r; r.end = 0; r.out = 0; r.nspans = 0; r.flags = IF_CORRUPT; r.reach = 0;
    if (have) r = res[ci];
    const int st = r.flags & 7, fin = (r.flags >> 3) & 1;
    const bool link = have && st == IF_OK && !fin && ci + 1 < ncand && cand[ci + 1] == r.end;
    const unsigned long long lm = __ballot(link);
    const int f = ~lm ? __ffsll((long long)~lm) - 1 : IF_WAVE;       // the first lane that does not link
    const int st_f = __shfl(st, f < IF_WAVE ? f : 0, IF_WAVE), fin_f = __shfl(fin, f < IF_WAVE ? f : 0, IF_WAVE);
    const int64_t end_f = __shfl(r.end, f < IF_WAVE ? f : 0, IF_WAVE);
    int take = f;                                                      // lanes [0, take) are units
    if (f < IF_WAVE && st_f == IF_OK) take = f + 1;
    {
      const bool in = lane < take;
      int64_t o = in ? (int64_t)r.out : 0;
      int s = in ? r.nspans : 0;
      int64_t oi = o; int si = s;
      int rc = in ? r.reach : 0;
      uint32_t sh = in ? r.out : 0xffffffffu;
#pragma unroll
      for (int d = 1; d < IF_WAVE; d <<= 1) {
        const int64_t oo = __shfl_up(oi, d, IF_WAVE); const int so = __shfl_up(si, d, IF_WAVE);
        if (lane >= d) { oi += oo; si += so; }
        const int ro = __shfl_xor(rc, d, IF_WAVE); const uint32_t ho = (uint32_t)__shfl_xor((int)sh, d, IF_WAVE);
        rc = ro > rc ? ro : rc; sh = ho < sh ? ho : sh;
      }
      if (in) { ucand[k + lane] = ci; uout[k + lane] = total + oi - o; uspan[k + lane] = (int32_t)(spans + si - s); }
      total += __shfl(oi, IF_WAVE - 1, IF_WAVE);
      spans += __shfl(si, IF_WAVE - 1, IF_WAVE);
      reach = rc > reach ? rc : reach; shortest = sh < shortest ? sh : shortest;
      k += take;
    }
    if (f == IF_WAVE) { c += IF_WAVE; continue; }
    if (st_f != IF_OK) { status = st_f; break; }
    if (fin_f) { status = end_f == nbits ? IF_OK : IF_CORRUPT; break; }
    const int next = end_f > 0 ? sp_lookup(first, index, lg, nch, end_f) : -1;
    if (next <= c + f || next >= ncand) { status = IF_CORRUPT; break; }  // (a unit ends at a candidate behind it, or is final)
    c = next;
  }
  if (status == IF_OK && n_expect >= 0 && total != n_expect) status = IF_SIZE;
  if (lane == 0) {
    head->status = status; head->n_units = k; head->total = total; head->n_spans = (int32_t)spans;
    head->max_reach = reach; head->shortest = k ? shortest : 0u;
  }
}

// ------------------------------------------------------------------------------------------------ symbols
__global__ __launch_bounds__(IF_WAVE) void inflate_spec_spans_kernel(const uint8_t* __restrict__ comp, long n, int lg, long nch,
                                                                     const SpHead* __restrict__ head, int n_units, int n_spans,
                                                                     const int64_t* __restrict__ first, const int64_t* __restrict__ cand,
                                                                     const SpRes* __restrict__ res, const int32_t* __restrict__ ucand,
                                                                     const int32_t* __restrict__ uspan, const int64_t* __restrict__ uout,
                                                                     SpSpan* __restrict__ spans) {
  __shared__ SpSharedSize S;
  if (head->status != IF_OK || head->n_units != n_units || head->n_spans != n_spans) return;
  for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int c = ucand[u], want = res[c].nspans, at = uspan[u];
    if (want > 0 && at >= 0 && at + want <= n_spans)
      sp_unit<SP_MODE_SPANS>(S.T, nullptr, comp, n, cand[c], 0xffffffffu, 8 * (int64_t)n + 64, lg, nch, first, spans + at, want, uout[u],
                             nullptr, 0u);
    __syncthreads();
  }
}

// the stored bytes become symbols: one block per span, 8 bytes -> 16 bytes per lane and step
__global__ __launch_bounds__(256) void inflate_spec_copy_kernel(const uint8_t* __restrict__ comp, long n, const SpHead* __restrict__ head,
                                                                int n_spans, const SpSpan* __restrict__ spans, uint16_t* __restrict__ sym,
                                                                long n_out) {
  if (head->status != IF_OK || head->n_spans != n_spans || head->total != n_out) return;
  for (int s = blockIdx.x; s < n_spans; s += gridDim.x) {
    const SpSpan sp = spans[s];
    if (sp.len <= 0 || sp.src < 0 || (long)sp.src + sp.len > n || sp.dst < 0 || sp.dst + sp.len > n_out) continue;
    const uint8_t* src = comp + sp.src;
    uint16_t* dst = sym + sp.dst;
    int head_s = (int)((8u - ((uint32_t)sp.dst & 7u)) & 7u);
    if (head_s > sp.len) head_s = sp.len;
    if ((int)threadIdx.x < head_s) dst[threadIdx.x] = src[threadIdx.x];
    const int nv = (sp.len - head_s) >> 3;
    for (int k = threadIdx.x; k < nv; k += 256) {
      uint2 v;
      __builtin_memcpy(&v, src + head_s + 8 * k, 8);
      uint4 w;
      w.x = (v.x & 0xffu) | ((v.x & 0xff00u) << 8); w.y = ((v.x >> 16) & 0xffu) | ((v.x >> 24) << 16);
      w.z = (v.y & 0xffu) | ((v.y & 0xff00u) << 8); w.w = ((v.y >> 16) & 0xffu) | ((v.y >> 24) << 16);
      *(uint4*)(dst + head_s + 8 * k) = w;
    }
    const int done = head_s + 8 * nv;
    if ((int)threadIdx.x < sp.len - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
  }
}

__global__ __launch_bounds__(IF_WAVE) void inflate_spec_symbols_kernel(const uint8_t* __restrict__ comp, long n, int lg, long nch,
                                                                       const SpHead* __restrict__ head, int n_units,
                                                                       const int64_t* __restrict__ first, const int64_t* __restrict__ cand,
                                                                       const SpRes* __restrict__ res, const int32_t* __restrict__ ucand,
                                                                       const int64_t* __restrict__ uout, uint16_t* sym, long n_out) {
  __shared__ SpSharedWrite S;
  if (head->status != IF_OK || head->n_units != n_units || head->total != n_out) return;
  const int u = blockIdx.x;
  const int c = ucand[u];
  const SpRes r = res[c];
  const int64_t o = uout[u];
  if (o < 0 || o + (int64_t)r.out > n_out) return;
  sp_unit<SP_MODE_WRITE>(S.T, S.ring, comp, n, cand[c], 0xffffffffu, 8 * (int64_t)n + 64, lg, nch, first, nullptr, 0, o, sym + o, r.out);
}

// ------------------------------------------------------------------------------------------------ windows and bytes
// One workgroup walks the units.  W holds the SP_WIN bytes in front of the unit at hand (byte i of it is stream byte start - SP_WIN
// + i; bytes in front of the stream are invalid); every thread resolves SP_WIN_PER bytes of the next window, which is stored.
__global__ __launch_bounds__(SP_WIN_THREADS) void inflate_spec_window_kernel(SpHead* __restrict__ head, int n_units,
                                                                             const int32_t* __restrict__ ucand, const SpRes* __restrict__ res,
                                                                             const int64_t* __restrict__ uout, const uint16_t* __restrict__ sym,
                                                                             long n_out, uint8_t* __restrict__ win) {
  __shared__ uint8_t W[SP_WIN] __attribute__((aligned(16)));
  if (head->status != IF_OK || head->n_units != n_units || head->total != n_out) return;
  const int t = threadIdx.x;
  int bad = 0;
  for (int u = 0; u + 1 < n_units; ++u) {                              // (nobody reads the window behind the last unit)
    const int64_t s0 = uout[u], len = (int64_t)res[ucand[u]].out, e = s0 + len;
    if (s0 < 0 || e > n_out) { bad = 1; break; }                       // the same values in every thread
    uint32_t w[SP_WIN_PER / 4];
#pragma unroll
    for (int j = 0; j < SP_WIN_PER / 4; ++j) w[j] = 0;
    const int64_t g0 = e - SP_WIN + SP_WIN_PER * t;
    if (g0 >= s0) {                                                    // all of this thread's bytes are the unit's: 64 bytes of symbols
      uint32_t raw[SP_WIN_PER / 2];
      __builtin_memcpy(raw, sym + g0, 2 * SP_WIN_PER);
#pragma unroll
      for (int j = 0; j < SP_WIN_PER; ++j) {
        const uint32_t s = (raw[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        uint32_t b = s;
        if (s >= 0x8000u) { const uint32_t m = s & 0x7fffu; b = 0; if ((int64_t)m + s0 < SP_WIN) bad = 1; else b = W[m]; }
        w[j >> 2] |= b << (8 * (j & 3));
      }
    } else {
#pragma unroll
      for (int j = 0; j < SP_WIN_PER; ++j) {
        const int i = SP_WIN_PER * t + j;
        const int64_t g = g0 + j;
        uint32_t b = 0;
        if (g >= s0) {
          const uint32_t s = sym[g];
          if (s < 0x8000u) b = s;
          else { const uint32_t m = s & 0x7fffu; if ((int64_t)m + s0 < SP_WIN) bad = 1; else b = W[m]; }
        } else if (g >= 0) b = W[i + (int)len];                        // g < s0: i + len < SP_WIN
        w[j >> 2] |= b << (8 * (j & 3));
      }
    }
    __syncthreads();
    uint8_t* gw = win + (size_t)u * SP_WIN + SP_WIN_PER * t;
#pragma unroll
    for (int j = 0; j < SP_WIN_PER / 16; ++j) {
      const uint4 v = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
      *(uint4*)(W + SP_WIN_PER * t + 16 * j) = v;
      *(uint4*)(gw + 16 * j) = v;
    }
    __syncthreads();
  }
  if (bad) head->status = IF_CORRUPT;                                  // a marker that points in front of the stream
}

// out[i] = sym[i], or the byte of the window in front of i's unit that the marker names; 16 bytes of `out` per thread and step
__global__ __launch_bounds__(256) void inflate_spec_resolve_kernel(SpHead* __restrict__ head, int n_units, const int64_t* __restrict__ uout,
                                                                   const uint16_t* __restrict__ sym, const uint8_t* __restrict__ win,
                                                                   uint8_t* __restrict__ out, long n_out) {
  if (head->status != IF_OK || head->n_units != n_units || head->total != n_out || n_units < 1) return;
  const long a = (long)((uintptr_t)out & 15);
  const long groups = (n_out + a + 15) >> 4;
  int bad = 0;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
    const long i0 = 16 * g - a, lo = i0 < 0 ? 0 : i0, hi = i0 + 16 < n_out ? i0 + 16 : n_out;
    int k = 0, kh = n_units;                                           // the last unit that starts at or in front of lo
    while (kh - k > 1) { const int mid = (k + kh) >> 1; if (uout[mid] <= lo) k = mid; else kh = mid; }
    int64_t uk = uout[k], next = k + 1 < n_units ? uout[k + 1] : (int64_t)n_out;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const long i = i0 + j;
      if (i >= lo && i < hi) {
        while (i >= next && k + 1 < n_units) { ++k; uk = next; next = k + 1 < n_units ? uout[k + 1] : (int64_t)n_out; }
        const uint32_t s = sym[i];
        uint32_t b = s;
        if (s >= 0x8000u) {
          const uint32_t m = s & 0x7fffu;
          if (k < 1 || (int64_t)m + uk < SP_WIN) { bad = 1; b = 0; }
          else b = win[(size_t)(k - 1) * SP_WIN + m];
        }
        w[j >> 2] |= b << (8 * (j & 3));
      }
    }
    if (hi - lo == 16) *(uint4*)(out + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    else
      for (int j = 0; j < 16; ++j) if (i0 + j >= lo && i0 + j < hi) out[i0 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  }
  if (bad) head->status = IF_CORRUPT;
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" size_t mt_inflate_spec_workspace(long n_comp, int chunk) {
  if (!sp_n_ok(n_comp) || !sp_chunk_ok(chunk)) return 0;
  return sp_layout(n_comp, chunk).bytes;
}

extern "C" size_t mt_inflate_spec_workspace_part(long n_comp, int chunk, int part) {
  if (!sp_n_ok(n_comp) || !sp_chunk_ok(chunk)) return 0;
  const SpLayout L = sp_layout(n_comp, chunk);
  return part == 0 ? L.cand : part == 1 ? L.ucand : part == 2 ? (size_t)L.cap : 0;
}

extern "C" size_t mt_inflate_spec_write_workspace(int n_units, int n_spans, long n_out) {
  if (n_units < 0 || n_spans < 0 || n_out < 0) return 0;
  const size_t b = sp_write_layout(n_units, n_spans, n_out).bytes;
  return b ? b : 16;
}

extern "C" int mt_inflate_spec_scan(const uint8_t* comp, long n_comp, int chunk, long unit_limit, long span_limit, long n_expect,
                                    int steps, void* ws, size_t ws_bytes, mt_stream_t stream) {
  MT_REQUIRE(sp_n_ok(n_comp), "inflate_spec_scan: %ld compressed bytes (1 .. INT32_MAX - 64)", n_comp);
  MT_REQUIRE(sp_chunk_ok(chunk), "inflate_spec_scan: a chunk of %d bytes (a power of two, 64 .. 2^20)", chunk);
  MT_REQUIRE(unit_limit >= 1 && unit_limit <= SP_MAX_UNIT_LIMIT, "inflate_spec_scan: a unit limit of %ld bytes (1 .. 2^30)", unit_limit);
  MT_REQUIRE(span_limit >= 1, "inflate_spec_scan: a span limit of %ld bytes (at least 1)", span_limit);
  MT_REQUIRE(steps >= 1 && steps <= 7, "inflate_spec_scan: steps %d (a mask of 1 search, 2 size, 4 chain)", steps);
  MT_REQUIRE(comp && ws, "inflate_spec_scan: NULL argument");
  MT_REQUIRE(((uintptr_t)ws & 15) == 0, "inflate_spec_scan: the workspace must be 16-byte aligned");
  const SpLayout L = sp_layout(n_comp, chunk);
  MT_REQUIRE_WORKSPACE("inflate_spec_scan", ws_bytes, L.bytes);
  hipStream_t s = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)ws;
  SpHead* head = (SpHead*)w;
  int32_t* index = (int32_t*)(w + L.index);
  int64_t* first = (int64_t*)(w + L.first);
  int64_t* cand = (int64_t*)(w + L.cand);
  SpRes* res = (SpRes*)(w + L.res);
  const long waves = (long)mt_device_cus(mt_current_device()) * 32;
  if (steps & SP_STEP_SEARCH) {
    hipLaunchKernelGGL(inflate_spec_search_kernel, dim3((unsigned)(L.nch < waves ? L.nch : waves)), dim3(IF_WAVE), 0, s, comp, n_comp, L.lg,
                       L.nch, first, index);
    MT_CHECK_LAUNCH("inflate_spec_scan (search)");
    hipLaunchKernelGGL(inflate_spec_scan_kernel, dim3(1), dim3(MT_SCAN_THREADS), 0, s, index, L.nch, head);
    MT_CHECK_LAUNCH("inflate_spec_scan (scan)");
    hipLaunchKernelGGL(inflate_spec_compact_kernel, dim3((unsigned)((L.nch + 255) / 256)), dim3(256), 0, s, first, index, L.nch, cand);
    MT_CHECK_LAUNCH("inflate_spec_scan (compact)");
  }
  if (steps & SP_STEP_SIZE) {
    const int64_t span_bits = span_limit > n_comp ? 8 * (int64_t)n_comp + 64 : 8 * (int64_t)span_limit;
    hipLaunchKernelGGL(inflate_spec_size_kernel, dim3((unsigned)(L.cap < waves ? L.cap : waves)), dim3(IF_WAVE), 0, s, comp, n_comp,
                       (uint32_t)unit_limit, span_bits, L.lg, L.nch, head, first, cand, res);
    MT_CHECK_LAUNCH("inflate_spec_scan (size)");
  }
  if (steps & SP_STEP_CHAIN) {
    hipLaunchKernelGGL(inflate_spec_chain_kernel, dim3(1), dim3(IF_WAVE), 0, s, head, first, index, L.lg, L.nch, cand, res,
                       (int32_t*)(w + L.ucand), (int32_t*)(w + L.uspan), (int64_t*)(w + L.uout), n_comp, n_expect);
    MT_CHECK_LAUNCH("inflate_spec_scan (chain)");
  }
  return MT_OK;
}

extern "C" int mt_inflate_spec_write(const uint8_t* comp, long n_comp, int chunk, void* ws, size_t ws_bytes, int n_units, int n_spans,
                                     void* ws2, size_t ws2_bytes, uint8_t* out, long n_out, int steps, mt_stream_t stream) {
  MT_REQUIRE(sp_n_ok(n_comp), "inflate_spec_write: %ld compressed bytes (1 .. INT32_MAX - 64)", n_comp);
  MT_REQUIRE(sp_chunk_ok(chunk), "inflate_spec_write: a chunk of %d bytes (a power of two, 64 .. 2^20)", chunk);
  MT_REQUIRE(steps >= 1 && steps <= 7, "inflate_spec_write: steps %d (a mask of 1 symbols, 2 windows, 4 resolve)", steps);
  MT_REQUIRE(comp && ws && ws2 && (out || n_out == 0), "inflate_spec_write: NULL argument");
  MT_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)ws2 & 15) == 0, "inflate_spec_write: the workspaces must be 16-byte aligned");
  const SpLayout L = sp_layout(n_comp, chunk);
  MT_REQUIRE(n_units >= 0 && n_units <= L.cap && n_spans >= 0 && (long)n_spans <= n_comp / 5 + 1 && n_out >= 0,
             "inflate_spec_write: %d units, %d spans, %ld bytes for a stream of %ld bytes", n_units, n_spans, n_out, n_comp);
  MT_REQUIRE_WORKSPACE("inflate_spec_write", ws_bytes, L.bytes);
  const SpWriteLayout K = sp_write_layout(n_units, n_spans, n_out);
  MT_REQUIRE_WORKSPACE("inflate_spec_write", ws2_bytes, K.bytes);
  if (n_units == 0 || n_out == 0) return MT_OK;
  hipStream_t s = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)ws;
  uint8_t* w2 = (uint8_t*)ws2;
  SpHead* head = (SpHead*)w;
  const int64_t* first = (const int64_t*)(w + L.first);
  const int64_t* cand = (const int64_t*)(w + L.cand);
  const SpRes* res = (const SpRes*)(w + L.res);
  const int32_t* ucand = (const int32_t*)(w + L.ucand);
  const int32_t* uspan = (const int32_t*)(w + L.uspan);
  const int64_t* uout = (const int64_t*)(w + L.uout);
  uint16_t* sym = (uint16_t*)w2;
  uint8_t* win = w2 + K.win;
  SpSpan* spans = (SpSpan*)(w2 + K.spans);
  if (steps & SP_STEP_SYMBOLS) {
    if (n_spans) {
      const long waves = (long)mt_device_cus(mt_current_device()) * 32;
      hipLaunchKernelGGL(inflate_spec_spans_kernel, dim3((unsigned)(n_units < waves ? n_units : waves)), dim3(IF_WAVE), 0, s, comp, n_comp,
                         L.lg, L.nch, head, n_units, n_spans, first, cand, res, ucand, uspan, uout, spans);
      MT_CHECK_LAUNCH("inflate_spec_write (spans)");
      const long cap = mt_stream_cap() * 4;
      hipLaunchKernelGGL(inflate_spec_copy_kernel, dim3((unsigned)(n_spans < cap ? n_spans : cap)), dim3(256), 0, s, comp, n_comp, head,
                         n_spans, spans, sym, n_out);
      MT_CHECK_LAUNCH("inflate_spec_write (copy)");
    }
    hipLaunchKernelGGL(inflate_spec_symbols_kernel, dim3((unsigned)n_units), dim3(IF_WAVE), 0, s, comp, n_comp, L.lg, L.nch, head, n_units,
                       first, cand, res, ucand, uout, sym, n_out);
    MT_CHECK_LAUNCH("inflate_spec_write (symbols)");
  }
  if ((steps & SP_STEP_WINDOWS) && n_units > 1) {
    hipLaunchKernelGGL(inflate_spec_window_kernel, dim3(1), dim3(SP_WIN_THREADS), 0, s, head, n_units, ucand, res, uout, sym, n_out, win);
    MT_CHECK_LAUNCH("inflate_spec_write (windows)");
  }
  if (steps & SP_STEP_RESOLVE) {
    hipLaunchKernelGGL(inflate_spec_resolve_kernel, dim3((unsigned)mt_stream_blocks((n_out + 31) / 16, 256)), dim3(256), 0, s, head, n_units,
                       uout, sym, win, out, n_out);
    MT_CHECK_LAUNCH("inflate_spec_write (resolve)");
  }
  return MT_OK;
}
