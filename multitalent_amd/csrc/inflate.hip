// inflate.hip — INFLATE (RFC 1951: stored, fixed and dynamic blocks, every length and distance code) for a raw DEFLATE stream in
// device memory, parallel over the byte-aligned restart points that the device writers (deflate.hip) and zlib's Z_FULL_FLUSH leave
// in a stream.  The reference inflates every .npz member and .nii.gz file on one host thread (np.load, gzip.open).
//
// A UNIT starts at a byte position, decodes consecutive blocks and ends behind an EMPTY stored block (the next unit starts at the
// following byte) or at a block with BFINAL (the stream ends at the next byte boundary).  Non-empty stored blocks belong to the unit
// they occur in.  No match reaches in front of its unit: a unit that holds one is BAD.
//   mt_inflate_scan   candidates = position 0 and every position behind an occurrence of 00 00 ff ff, compacted in order;
//                     size pass: one wave per candidate decodes without output -> end, bytes, stored blocks, status;
//                     chain: one wave follows end -> start from position 0 (64 candidates per step where each ends at the next
//                     one), which by induction holds true units only, and takes the exclusive scan of their sizes.
//   mt_inflate_write  the stored blocks of the chained units are listed as spans and copied by the whole grid; then one wave per
//                     unit decodes again into its own range: the output is staged in an LDS ring of IF_RB bytes, which serves
//                     every match nearer than IF_RB - 258 bytes, and leaves in 16-byte stores.
//   mt_inflate_crc    CRC-32 of fixed-size pieces of the result; the host joins them.
// Decoding is wave-uniform: every lane holds the same bit buffer (fed from a 256-byte window of the input that the lanes hold one
// dword each), the lanes share table construction, match copies and the stores.  Restated in tests/inflate_host.py.  The tables,
// the bit reader and the reading of a block's two codes live in inflate_common.h / inflate_codes.inc, shared with inflate_spec.hip.
#include "inflate_common.h"
#include "crc32_common.h"

#define IF_RB 4096                                   // ring bytes (a power of two)
#define IF_FLUSH 2048                                // unflushed bytes at which the ring is written out; IF_FLUSH + 258 <= IF_RB
#define IF_SCAN_THREADS 256
#define IF_SCAN_PER 16
#define IF_SCAN_TILE (IF_SCAN_THREADS * IF_SCAN_PER)
#define IF_MIN_UNIT 5                                // an empty stored block on a byte boundary: 1 + 4 bytes
#define IF_MIN_SPAN 6                                // a stored block of one byte
#define IF_HEAD_BYTES 64
#define IF_MAX_UNIT_LIMIT (1l << 30)

enum { IF_MODE_SIZE = 0, IF_MODE_SPANS = 1, IF_MODE_WRITE = 2 };

struct IfHead { int32_t status, n_units; int64_t total; int32_t n_cand, n_spans; };
struct IfRes { int32_t end; uint32_t out; int32_t nspans, flags; };            // flags: status | final << 3
struct IfSpan { int64_t dst; int32_t src, len; };

// workspace: [head 64][block counts i32 x nblk][cand_pos i32 x cap][res 16 x cap][unit_cand i32 x cap][unit_span i32 x cap]
//            [unit_out i64 x cap][spans 16 x span_cap], every part 16-byte aligned.
// cap = n / IF_MIN_UNIT + 2: true units are at least IF_MIN_UNIT bytes apart, so a stream with more candidates than that holds
// markers that are no restart points; span_cap = n / IF_MIN_SPAN + 2: the chained units are disjoint.
struct IfLayout {
  long nblk, cap, span_cap;
  size_t counts, cand, res, ucand, uspan, uout, spans, bytes;
};
static inline size_t if_al(size_t v) { return (v + 15) & ~(size_t)15; }
static inline IfLayout if_layout(long n) {
  IfLayout L;
  L.nblk = (n + IF_SCAN_TILE - 1) / IF_SCAN_TILE;
  L.cap = n / IF_MIN_UNIT + 2;
  L.span_cap = n / IF_MIN_SPAN + 2;
  L.counts = IF_HEAD_BYTES;
  L.cand = L.counts + if_al(4 * (size_t)L.nblk);
  L.res = L.cand + if_al(4 * (size_t)L.cap);
  L.ucand = L.res + 16 * (size_t)L.cap;
  L.uspan = L.ucand + if_al(4 * (size_t)L.cap);
  L.uout = L.uspan + if_al(4 * (size_t)L.cap);
  L.spans = L.uout + if_al(8 * (size_t)L.cap);
  L.bytes = L.spans + 16 * (size_t)L.span_cap;
  return L;
}
static inline bool if_n_ok(long n) { return n >= 1 && n <= 2147483647l - 64; }

// ------------------------------------------------------------------------------------------------ candidates
__device__ __forceinline__ uint32_t if_marker_mask(const uint8_t* __restrict__ comp, long n, long p0) {
  // bit i: bytes p0 + i .. p0 + i + 3 are 00 00 ff ff and a unit could start behind them (p0 + i + 4 < n)
  uint32_t b[IF_SCAN_PER + 3];
#pragma unroll
  for (int k = 0; k < IF_SCAN_PER + 3; ++k) b[k] = p0 + k < n ? comp[p0 + k] : 1u;
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < IF_SCAN_PER; ++i)
    if (p0 + i + 4 < n && b[i] == 0 && b[i + 1] == 0 && b[i + 2] == 0xffu && b[i + 3] == 0xffu) m |= 1u << i;
  return m;
}

__device__ __forceinline__ uint32_t if_block_scan(uint32_t v, uint32_t* red, uint32_t& total) {       // exclusive, thread order
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
  if (lane == 63) red[wv] = inc;
  __syncthreads();
  uint32_t base = 0; total = 0;
#pragma unroll
  for (int k = 0; k < IF_SCAN_THREADS / 64; ++k) { const uint32_t r = red[k]; if (k < wv) base += r; total += r; }
  __syncthreads();
  return base + inc - v;
}

__global__ __launch_bounds__(IF_SCAN_THREADS) void inflate_cand_count_kernel(const uint8_t* __restrict__ comp, long n,
                                                                             int32_t* __restrict__ counts) {
  __shared__ uint32_t red[IF_SCAN_THREADS / 64];
  const long p0 = (long)blockIdx.x * IF_SCAN_TILE + (long)threadIdx.x * IF_SCAN_PER;
  uint32_t total;
  if_block_scan((uint32_t)__popc(if_marker_mask(comp, n, p0)), red, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = (int32_t)total;
}

__global__ __launch_bounds__(MT_SCAN_THREADS) void inflate_cand_scan_kernel(int32_t* __restrict__ counts, long nblk, long cap,
                                                                            IfHead* __restrict__ head) {
  const int64_t total = mt_scan_units(counts, nblk);
  if (threadIdx.x == 0) {
    const bool fits = total + 1 <= cap;
    head->status = fits ? IF_OK : IF_FOREIGN;
    head->n_cand = fits ? (int32_t)(total + 1) : 0;
    head->n_units = 0; head->total = 0; head->n_spans = 0;
  }
}

__global__ __launch_bounds__(IF_SCAN_THREADS) void inflate_cand_write_kernel(const uint8_t* __restrict__ comp, long n,
                                                                             const int32_t* __restrict__ offs,
                                                                             const IfHead* __restrict__ head, int32_t* __restrict__ cand) {
  __shared__ uint32_t red[IF_SCAN_THREADS / 64];
  if (head->status != IF_OK) return;
  const long p0 = (long)blockIdx.x * IF_SCAN_TILE + (long)threadIdx.x * IF_SCAN_PER;
  uint32_t m = if_marker_mask(comp, n, p0), total;
  uint32_t at = 1u + (uint32_t)offs[blockIdx.x] + if_block_scan((uint32_t)__popc(m), red, total);
  while (m) { const int i = __ffs(m) - 1; m &= m - 1; cand[at++] = (int32_t)(p0 + i + 4); }
  if (blockIdx.x == 0 && threadIdx.x == 0) cand[0] = 0;
}

// ------------------------------------------------------------------------------------------------ one unit
struct IfSharedSize { IfTables T; };
struct IfSharedWrite { uint8_t ring[IF_RB] __attribute__((aligned(16))); IfTables T; };


// The ring of a unit that is written: position q of the unit's output lives in ring[(bias + q) & (IF_RB - 1)], bias = the low bits
// of its global address, so that 16-byte pieces of the ring are 16-byte pieces of memory.
struct IfOut {
  uint8_t* ring; uint8_t* obase; uint32_t bias, pos, flushed, ring_lo, limit; int lane;
  __device__ __forceinline__ uint32_t slot(uint32_t q) const { return (bias + q) & (IF_RB - 1); }
  __device__ __forceinline__ void flush(bool all) {
    __syncthreads();
    uint32_t a1 = pos;
    if (!all) {
      const uint32_t tail = (uint32_t)((uintptr_t)obase + pos) & 15u;
      if (pos < flushed + tail) return;
      a1 = pos - tail;
    }
    uint32_t q = flushed;
    uint32_t head = (16u - ((uint32_t)((uintptr_t)obase + q) & 15u)) & 15u;
    if (head > a1 - q) head = a1 - q;
    if ((uint32_t)lane < head) obase[q + lane] = ring[slot(q + lane)];
    q += head;
    const uint32_t nv = (a1 - q) >> 4;
    for (uint32_t k = lane; k < nv; k += IF_WAVE) *(uint4*)(obase + q + 16 * k) = *(const uint4*)(ring + slot(q + 16 * k));
    q += 16 * nv;
    if ((uint32_t)lane < a1 - q) obase[q + lane] = ring[slot(q + lane)];
    flushed = a1;
    __threadfence();                                                  // far matches read these bytes back
    __syncthreads();
  }
};

// Decodes the unit that starts at byte `start`.  SIZE: no output.  SPANS: its first `want` stored blocks go to spans[] (dst from
// out0), then it stops.  WRITE: the Huffman-coded bytes go to out0 + [0, limit), the stored blocks are skipped (they are copied
// as spans beforehand).  All lanes run the same path.
template <int MODE>
__device__ __forceinline__ IfRes if_unit(IfTables& T, uint8_t* ring, const uint8_t* __restrict__ comp, long n, long start,
                                         uint32_t unit_limit, IfSpan* __restrict__ spans, int want, int64_t out0,
                                         uint8_t* __restrict__ obase, uint32_t limit) {
  const int lane = threadIdx.x;
  IfIn I; I.open(comp, n, start, lane);
  IfOut O;
  O.ring = ring; O.obase = obase; O.bias = (uint32_t)((uintptr_t)obase) & (IF_RB - 1); O.pos = 0; O.flushed = 0; O.ring_lo = 0;
  O.limit = limit; O.lane = lane;
  uint32_t pos = 0, huff = 0;
  int nspans = 0, status = IF_OK, final = 0;
  long end = start;
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
      if (len == 0) {
        end = data;
        break;                                                         // the marker (or an empty last block): the unit ends
      }
      if (MODE == IF_MODE_SPANS) {
        if (lane == 0) { IfSpan s; s.dst = out0 + pos; s.src = (int32_t)data; s.len = (int32_t)len; spans[nspans] = s; }
        if (nspans + 1 == want) { ++nspans; break; }
      }
      if (MODE == IF_MODE_WRITE) {
        O.flush(true);
        if (pos + len > limit) { status = IF_CORRUPT; break; }
        O.pos = O.flushed = O.ring_lo = pos + len;
      }
      ++nspans;
      pos += len;
      I.seek(data + len);
      if (final) { end = data + len; break; }
      continue;
    }
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
        if (MODE == IF_MODE_WRITE) {
          if (pos + 1 > limit) { status = IF_CORRUPT; break; }
          if (lane == 0) ring[O.slot(pos)] = (uint8_t)sym;
        }
        ++pos; ++huff;
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
        if (dist > pos) { status = IF_BAD; break; }                   // it would reach in front of the unit
        if (MODE == IF_MODE_WRITE) {
          if (pos + L > limit) { status = IF_CORRUPT; break; }
          __syncthreads();
          for (uint32_t k = lane; k < L; k += IF_WAVE) {
            const uint32_t q = pos - dist + (k < dist ? k : k % dist);
            uint8_t b;
            if (q >= O.ring_lo && pos + L - q <= IF_RB) b = ring[O.slot(q)];
            else b = obase[q];                                        // flushed, or a stored block: q < O.flushed
            ring[O.slot(pos + k)] = b;
          }
        }
        pos += L; huff += L;
      }
      if (I.overrun()) { status = IF_BAD; break; }
      if (huff > unit_limit) { status = IF_TOO_LONG; break; }
      if (MODE == IF_MODE_WRITE) {
        O.pos = pos;
        if (pos - O.flushed >= IF_FLUSH) O.flush(false);
      }
    }
    if (status != IF_OK) break;
    if (final) { I.align(); end = I.byte_pos(); break; }
  }
  if (MODE == IF_MODE_WRITE) { O.pos = pos < limit ? pos : limit; if (O.pos >= O.flushed) O.flush(true); }
  IfRes r;
  r.end = (int32_t)end; r.out = pos; r.nspans = nspans; r.flags = status | (final << 3);
  return r;
}

__global__ __launch_bounds__(IF_WAVE) void inflate_size_kernel(const uint8_t* __restrict__ comp, long n, uint32_t unit_limit,
                                                               const IfHead* __restrict__ head, const int32_t* __restrict__ cand,
                                                               IfRes* __restrict__ res) {
  __shared__ IfSharedSize S;
  if (head->status != IF_OK) return;
  const int ncand = head->n_cand;
  for (int c = blockIdx.x; c < ncand; c += gridDim.x) {
    const IfRes r = if_unit<IF_MODE_SIZE>(S.T, nullptr, comp, n, (long)cand[c], unit_limit, nullptr, 0, 0, nullptr, 0u);
    if (threadIdx.x == 0) res[c] = r;
    __syncthreads();
  }
}

// One wave.  Lane j looks at candidate c + j: it LINKS when it decoded, is not final and ends where candidate c + j + 1 starts.
// The lanes in front of the first that does not link, and that lane, are units; from its end the next start is searched.
__global__ __launch_bounds__(IF_WAVE) void inflate_chain_kernel(IfHead* __restrict__ head, const int32_t* __restrict__ cand,
                                                                const IfRes* __restrict__ res, int32_t* __restrict__ ucand,
                                                                int32_t* __restrict__ uspan, int64_t* __restrict__ uout, long n,
                                                                int need_final, long n_expect) {
  if (head->status != IF_OK) return;
  const int lane = threadIdx.x, ncand = head->n_cand;
  int c = 0, k = 0, status = -1;
  int64_t total = 0;
  long spans = 0;
  while (status < 0) {
    const int ci = c + lane;
    const bool have = ci < ncand;
    IfRes r; r.end = 0; r.out = 0; r.nspans = 0; r.flags = IF_CORRUPT;
    if (have) r = res[ci];
    const int st = r.flags & 7, fin = (r.flags >> 3) & 1;
    const bool link = have && st == IF_OK && !fin && ci + 1 < ncand && cand[ci + 1] == r.end;
    const unsigned long long lm = __ballot(link);
    const int f = ~lm ? __ffsll((long long)~lm) - 1 : IF_WAVE;       // the first lane that does not link
    const int st_f = __shfl(st, f < IF_WAVE ? f : 0, IF_WAVE), fin_f = __shfl(fin, f < IF_WAVE ? f : 0, IF_WAVE);
    const int end_f = __shfl(r.end, f < IF_WAVE ? f : 0, IF_WAVE);
    int take = f;                                                      // lanes [0, take) are units
    if (f < IF_WAVE && st_f == IF_OK) take = f + 1;
    {
      const bool in = lane < take;
      int64_t o = in ? (int64_t)r.out : 0;
      int s = in ? r.nspans : 0;
      int64_t oi = o; int si = s;
#pragma unroll
      for (int d = 1; d < IF_WAVE; d <<= 1) {
        const int64_t oo = __shfl_up(oi, d, IF_WAVE); const int so = __shfl_up(si, d, IF_WAVE);
        if (lane >= d) { oi += oo; si += so; }
      }
      if (in) { ucand[k + lane] = ci; uout[k + lane] = total + oi - o; uspan[k + lane] = (int32_t)(spans + si - s); }
      total += __shfl(oi, IF_WAVE - 1, IF_WAVE);
      spans += __shfl(si, IF_WAVE - 1, IF_WAVE);
      k += take;
    }
    if (f == IF_WAVE) { c += IF_WAVE; continue; }
    if (st_f != IF_OK) { status = st_f; break; }
    if (fin_f) { status = end_f == n ? IF_OK : IF_CORRUPT; break; }
    if (end_f == n) { status = need_final ? IF_CORRUPT : IF_OK; break; }
    int lo = c + f + 1, hi = ncand;                                    // the candidate that starts at end_f
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cand[mid] < end_f) lo = mid + 1; else hi = mid; }
    if (lo >= ncand || cand[lo] != end_f) { status = IF_CORRUPT; break; }
    c = lo;
  }
  if (status == IF_OK && n_expect >= 0 && total != n_expect) status = IF_SIZE;
  if (lane == 0) { head->status = status; head->n_units = k; head->total = total; head->n_spans = (int32_t)spans; }
}

__global__ __launch_bounds__(IF_WAVE) void inflate_spans_kernel(const uint8_t* __restrict__ comp, long n, const IfHead* __restrict__ head,
                                                                int n_units, const int32_t* __restrict__ cand, const IfRes* __restrict__ res,
                                                                const int32_t* __restrict__ ucand, const int32_t* __restrict__ uspan,
                                                                const int64_t* __restrict__ uout, IfSpan* __restrict__ spans) {
  __shared__ IfSharedSize S;
  if (head->status != IF_OK || head->n_units != n_units) return;
  for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int c = ucand[u], want = res[c].nspans;
    if (want > 0) if_unit<IF_MODE_SPANS>(S.T, nullptr, comp, n, (long)cand[c], 0xffffffffu, spans + uspan[u], want, uout[u], nullptr, 0u);
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void inflate_copy_kernel(const uint8_t* __restrict__ comp, long n, const IfHead* __restrict__ head,
                                                           int n_spans, const IfSpan* __restrict__ spans, uint8_t* __restrict__ out,
                                                           long n_out) {
  if (head->status != IF_OK || head->n_spans != n_spans || head->total != n_out) return;
  for (int s = blockIdx.x; s < n_spans; s += gridDim.x) {
    const IfSpan sp = spans[s];
    if (sp.len <= 0 || sp.src < 0 || (long)sp.src + sp.len > n || sp.dst < 0 || sp.dst + sp.len > n_out) continue;
    const uint8_t* src = comp + sp.src;
    uint8_t* dst = out + sp.dst;
    int head_b = (int)((16u - ((uint32_t)(uintptr_t)dst & 15u)) & 15u);
    if (head_b > sp.len) head_b = sp.len;
    if ((int)threadIdx.x < head_b) dst[threadIdx.x] = src[threadIdx.x];
    const int nv = (sp.len - head_b) >> 4;
    for (int k = threadIdx.x; k < nv; k += 256) {
      uint4 v;
      __builtin_memcpy(&v, src + head_b + 16 * k, 16);
      *(uint4*)(dst + head_b + 16 * k) = v;
    }
    const int done = head_b + 16 * nv;
    if ((int)threadIdx.x < sp.len - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
  }
}

__global__ __launch_bounds__(IF_WAVE) void inflate_write_kernel(const uint8_t* __restrict__ comp, long n, const IfHead* __restrict__ head,
                                                                int n_units, const int32_t* __restrict__ cand, const IfRes* __restrict__ res,
                                                                const int32_t* __restrict__ ucand, const int64_t* __restrict__ uout,
                                                                uint8_t* __restrict__ out, long n_out) {
  __shared__ IfSharedWrite S;
  if (head->status != IF_OK || head->n_units != n_units || head->total != n_out) return;
  const int u = blockIdx.x;
  const int c = ucand[u];
  const IfRes r = res[c];
  const int64_t o = uout[u];
  if (o < 0 || o + (int64_t)r.out > n_out) return;
  if_unit<IF_MODE_WRITE>(S.T, S.ring, comp, n, (long)cand[c], 0xffffffffu, nullptr, 0, o, out + o, r.out);
}

// ------------------------------------------------------------------------------------------------ CRC-32 of pieces
__global__ __launch_bounds__(256) void inflate_crc_kernel(const uint8_t* __restrict__ data, long n, int piece, uint32_t* __restrict__ crcs) {
  __shared__ uint32_t crctab[256], pow128[256], red[8];
  const int t = threadIdx.x;
  df_crc_tables(crctab, pow128, t);
  __syncthreads();
  const long ps = (long)blockIdx.x * piece;
  const int plen = (int)(n - ps < piece ? n - ps : piece);
  uint32_t acc = 0xffffffffu;
  for (int ts = 0; ts < plen; ts += 4096) {
    const int m = plen - ts < 4096 ? plen - ts : 4096;
    const int q = m >> 4, r = m & 15;
    const uint8_t* p = data + ps + ts;
    uint32_t reg = t == 0 ? acc : 0u;
    if (t < q) {
      uint4 v;
      __builtin_memcpy(&v, p + 16 * t, 16);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 16; ++i) reg = crctab[(reg ^ (w[i >> 2] >> (8 * (i & 3)))) & 0xffu] ^ (reg >> 8);
      reg = df_mulmod(reg, pow128[q - 1 - t]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) reg ^= __shfl_xor(reg, off, 64);
    if ((t & 63) == 0) red[t >> 6] = reg;
    __syncthreads();
    uint32_t x = red[0] ^ red[1] ^ red[2] ^ red[3];
    if (r) {
      if (t == q) {
        uint32_t g = x;
        for (int i = 0; i < r; ++i) g = crctab[(g ^ p[16 * q + i]) & 0xffu] ^ (g >> 8);
        red[4] = g;
      }
      __syncthreads();
      x = red[4];
    }
    __syncthreads();
    acc = x;
  }
  if (t == 0) crcs[blockIdx.x] = ~acc;
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" size_t mt_inflate_workspace(long n_comp) {
  if (!if_n_ok(n_comp)) return 0;
  return if_layout(n_comp).bytes;
}

extern "C" size_t mt_inflate_workspace_part(long n_comp, int part) {
  if (!if_n_ok(n_comp)) return 0;
  const IfLayout L = if_layout(n_comp);
  return part == 0 ? L.cand : part == 1 ? L.ucand : part == 2 ? (size_t)L.cap : 0;
}

extern "C" int mt_inflate_scan(const uint8_t* comp, long n_comp, long unit_limit, int final, long n_expect, void* ws, size_t ws_bytes,
                               mt_stream_t stream) {
  MT_REQUIRE(if_n_ok(n_comp), "inflate_scan: %ld compressed bytes (1 .. INT32_MAX - 64)", n_comp);
  MT_REQUIRE(unit_limit >= 1 && unit_limit <= IF_MAX_UNIT_LIMIT, "inflate_scan: a unit limit of %ld bytes (1 .. 2^30)", unit_limit);
  MT_REQUIRE(comp && ws, "inflate_scan: NULL argument");
  MT_REQUIRE(((uintptr_t)ws & 15) == 0, "inflate_scan: the workspace must be 16-byte aligned");
  const IfLayout L = if_layout(n_comp);
  MT_REQUIRE_WORKSPACE("inflate_scan", ws_bytes, L.bytes);
  hipStream_t s = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)ws;
  IfHead* head = (IfHead*)w;
  int32_t* counts = (int32_t*)(w + L.counts);
  int32_t* cand = (int32_t*)(w + L.cand);
  IfRes* res = (IfRes*)(w + L.res);
  hipLaunchKernelGGL(inflate_cand_count_kernel, dim3((unsigned)L.nblk), dim3(IF_SCAN_THREADS), 0, s, comp, n_comp, counts);
  MT_CHECK_LAUNCH("inflate_scan (count)");
  hipLaunchKernelGGL(inflate_cand_scan_kernel, dim3(1), dim3(MT_SCAN_THREADS), 0, s, counts, L.nblk, L.cap, head);
  MT_CHECK_LAUNCH("inflate_scan (scan)");
  hipLaunchKernelGGL(inflate_cand_write_kernel, dim3((unsigned)L.nblk), dim3(IF_SCAN_THREADS), 0, s, comp, n_comp, counts, head, cand);
  MT_CHECK_LAUNCH("inflate_scan (candidates)");
  const long waves = (long)mt_device_cus(mt_current_device()) * 32;
  const unsigned grid = (unsigned)(L.cap < waves ? L.cap : waves);
  hipLaunchKernelGGL(inflate_size_kernel, dim3(grid), dim3(IF_WAVE), 0, s, comp, n_comp, (uint32_t)unit_limit, head, cand, res);
  MT_CHECK_LAUNCH("inflate_scan (size)");
  hipLaunchKernelGGL(inflate_chain_kernel, dim3(1), dim3(IF_WAVE), 0, s, head, cand, res, (int32_t*)(w + L.ucand), (int32_t*)(w + L.uspan),
                     (int64_t*)(w + L.uout), n_comp, final ? 1 : 0, n_expect);
  MT_CHECK_LAUNCH("inflate_scan (chain)");
  return MT_OK;
}

extern "C" int mt_inflate_write(const uint8_t* comp, long n_comp, void* ws, size_t ws_bytes, int n_units, int n_spans, uint8_t* out,
                                long n_out, mt_stream_t stream) {
  MT_REQUIRE(if_n_ok(n_comp), "inflate_write: %ld compressed bytes (1 .. INT32_MAX - 64)", n_comp);
  MT_REQUIRE(comp && ws && (out || n_out == 0), "inflate_write: NULL argument");
  MT_REQUIRE(((uintptr_t)ws & 15) == 0, "inflate_write: the workspace must be 16-byte aligned");
  const IfLayout L = if_layout(n_comp);
  MT_REQUIRE(n_units >= 0 && n_units <= L.cap && n_spans >= 0 && n_spans <= L.span_cap && n_out >= 0,
             "inflate_write: %d units, %d spans, %ld bytes for a stream of %ld bytes", n_units, n_spans, n_out, n_comp);
  MT_REQUIRE_WORKSPACE("inflate_write", ws_bytes, L.bytes);
  if (n_units == 0 || n_out == 0) return MT_OK;
  hipStream_t s = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)ws;
  const IfHead* head = (const IfHead*)w;
  const int32_t* cand = (const int32_t*)(w + L.cand);
  const IfRes* res = (const IfRes*)(w + L.res);
  const int32_t* ucand = (const int32_t*)(w + L.ucand);
  const int32_t* uspan = (const int32_t*)(w + L.uspan);
  const int64_t* uout = (const int64_t*)(w + L.uout);
  IfSpan* spans = (IfSpan*)(w + L.spans);
  if (n_spans) {
    const long waves = (long)mt_device_cus(mt_current_device()) * 32;
    hipLaunchKernelGGL(inflate_spans_kernel, dim3((unsigned)(n_units < waves ? n_units : waves)), dim3(IF_WAVE), 0, s, comp, n_comp, head,
                       n_units, cand, res, ucand, uspan, uout, spans);
    MT_CHECK_LAUNCH("inflate_write (spans)");
    const long cap = mt_stream_cap() * 4;
    hipLaunchKernelGGL(inflate_copy_kernel, dim3((unsigned)(n_spans < cap ? n_spans : cap)), dim3(256), 0, s, comp, n_comp, head, n_spans,
                       spans, out, n_out);
    MT_CHECK_LAUNCH("inflate_write (copy)");
  }
  hipLaunchKernelGGL(inflate_write_kernel, dim3((unsigned)n_units), dim3(IF_WAVE), 0, s, comp, n_comp, head, n_units, cand, res, ucand, uout,
                     out, n_out);
  MT_CHECK_LAUNCH("inflate_write (decode)");
  return MT_OK;
}

extern "C" int mt_inflate_crc(const uint8_t* data, long n, int piece, uint32_t* crcs, mt_stream_t stream) {
  MT_REQUIRE(n >= 0 && piece >= 16 && piece <= (1 << 24), "inflate_crc: %ld bytes in pieces of %d (16 .. 2^24)", n, piece);
  MT_REQUIRE((data || n == 0) && crcs, "inflate_crc: NULL argument");
  const long pieces = n > 0 ? (n + piece - 1) / piece : 1;
  MT_REQUIRE(pieces <= 2147483647l, "inflate_crc: %ld pieces", pieces);
  hipLaunchKernelGGL(inflate_crc_kernel, dim3((unsigned)pieces), dim3(256), 0, (hipStream_t)stream, data, n, piece, crcs);
  MT_CHECK_LAUNCH("inflate_crc");
  return MT_OK;
}
