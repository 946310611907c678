// deflate.hip — a gzip / DEFLATE encoder for byte streams in device memory (label maps written as .nii.gz; the reference hands
// the raw voxels to SimpleITK / Python's gzip on one host thread, segmentation_export.py:148-160; stored probabilities and training
// cases written as .npz, where it calls np.savez_compressed).  The stream is a short HOST prefix (the NIfTI or .npy header) followed
// by the device payload, cut into chunks that are encoded independently, one workgroup each:
//   mt_deflate_tokenize  tokenises every chunk (run-length matches at distance `period`: 1, or the element size of the payload),
//                        counts the 286 + 30 DEFLATE symbols of the whole call and leaves each chunk's CRC-32 in the workspace;
//   (host)               builds ONE length-limited Huffman code from the counts, the dynamic-block header and the token table;
//   mt_deflate_emit      sizes each chunk under that code, writes it as one dynamic block (or as stored blocks where those are
//                        smaller) into the chunk's own zeroed region — a lane packs its consecutive tokens in registers and stores
//                        whole words, only the first and last word of its bit range go through atomicOr; lanes own disjoint bit
//                        ranges, so the bytes do not depend on the order — and compacts the regions by the prefix sum of their sizes.
// Tokeniser and framing are restated in tests/deflate_host.py (period 1) and tests/deflate_period_host.py; the device output equals
// them byte for byte.
#include "stream_common.h"
#include "crc32_common.h"

#define DF_THREADS 256
#define DF_PER 16                                   // bytes per lane and tile: one ds_read_b128
#define DF_BACK 8                                   // bytes a lane sees behind its own: the largest period
#define DF_TILE (DF_THREADS * DF_PER)
#define DF_NONE (-2147483647 - 1)
#define DF_LL 286
#define DF_HIST (DF_LL + 30)
#define DF_TOK_MATCH0 256
#define DF_TOK_EOB 512
#define DF_TOK_SLOTS 513
#define DF_HDR_WORDS 256                            // 8192 bits; a dynamic header has at most 14 + 3 + 19*3 + 316*14 = 4498
#define DF_NOBYTE 256u                              // what stands for a byte in front of the chunk: equal to no byte

// workspace: [prefix 512][token table 513 x 8, padded to 4608][header words 1024][crc u32 x nchunks][size i32 x nchunks][pad 16][regions]
#define DF_WS_TAB MT_DEFLATE_MAX_PREFIX
#define DF_WS_HDR (DF_WS_TAB + 4608)
#define DF_WS_CRC (DF_WS_HDR + DF_HDR_WORDS * 4)

static inline long df_chunks(long n, int chunk) { const long c = (n + chunk - 1) / chunk; return c > 0 ? c : 1; }
__host__ __device__ static inline long df_stored_size(long len) { const long b = (len + 65534) / 65535; return len + 5 * (b > 0 ? b : 1); }
static inline long df_region(int chunk) { return (df_stored_size(chunk) + 3) & ~3l; }
static inline size_t df_ws_regions(long nchunks) { return ((size_t)DF_WS_CRC + 8 * (size_t)nchunks + 15) & ~(size_t)15; }
static inline size_t df_out_data(long nchunks) { return 8 + (((size_t)nchunks * 4 + 7) & ~(size_t)7); }
static inline bool df_args_ok(long n, int chunk) { return n >= 0 && n <= 2147483647l && chunk >= MT_DEFLATE_MIN_CHUNK && chunk <= MT_DEFLATE_MAX_CHUNK; }
static inline bool df_period_ok(int period) { return period == 1 || period == 2 || period == 4 || period == 8; }

struct DfShared {
  uint32_t w[DF_TILE / 4 + 4] __attribute__((aligned(16)));      // the tile as an aligned dword copy of global memory, + 1 byte of lookahead
  uint64_t tab[DF_TOK_SLOTS];       // token -> bits | nbits << 48   (emit)
  uint32_t hist[DF_HIST];           // (tokenize)
  uint32_t crctab[256];             // bytewise CRC-32 table (tokenize)
  uint32_t pow128[DF_THREADS];      // x^(128 k) mod P: what k later 16-byte pieces shift a piece's CRC by (tokenize)
  int red[8];
};

struct DfStream {
  const uint8_t* pre; const uint8_t* pay;   // prefix (device copy) and payload
  long npre, n;                              // stream = pre[0, npre) ++ pay[0, n - npre)
  __device__ __forceinline__ uint32_t byte(long i) const { return i < npre ? pre[i] : pay[i - npre]; }
};

__device__ __forceinline__ int df_length_symbol(int len) {            // RFC 1951 §3.2.5
  if (len == 258) return 285;
  const int v = len - 3;
  if (v < 8) return 257 + v;
  const int e = 29 - __clz(v);
  return 261 + 4 * e + ((v >> e) & 3);
}

// exclusive max-scan over the block's threads in thread order; `total` = the maximum over all threads.  Two barriers.
__device__ __forceinline__ int df_scan_max(int v, int* red, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d, 64); if (lane >= d) inc = inc > o ? inc : o; }
  if (lane == 63) red[wv] = inc;
  __syncthreads();
  int base = DF_NONE; total = DF_NONE;
#pragma unroll
  for (int k = 0; k < DF_THREADS / 64; ++k) { const int r = red[k]; if (k < wv) base = base > r ? base : r; total = total > r ? total : r; }
  int ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = DF_NONE;
  __syncthreads();
  return ex > base ? ex : base;
}
__device__ __forceinline__ uint32_t df_scan_sum(uint32_t v, int* red, uint32_t& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
  if (lane == 63) red[wv] = (int)inc;
  __syncthreads();
  uint32_t base = 0; total = 0;
#pragma unroll
  for (int k = 0; k < DF_THREADS / 64; ++k) { const uint32_t r = (uint32_t)red[k]; if (k < wv) base += r; total += r; }
  __syncthreads();
  return base + inc - v;
}
__device__ __forceinline__ uint32_t df_reduce_xor(uint32_t v, int* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (int)v;
  __syncthreads();
  uint32_t x = 0;
#pragma unroll
  for (int k = 0; k < DF_THREADS / 64; ++k) x ^= (uint32_t)red[k];
  __syncthreads();
  return x;
}

// nbits (<= 48) bits of v at bit position pos of a zeroed word array: OR is order independent (header and end of block)
__device__ __forceinline__ void df_put(uint32_t* out, uint32_t pos, uint64_t v) {
  const uint32_t wd = pos >> 5, sh = pos & 31;
  const uint32_t a = (uint32_t)(v << sh);
  const uint64_t r = v >> (32 - sh);                                  // shift 1..32
  if (a) atomicOr(out + wd, a);
  if ((uint32_t)r) atomicOr(out + wd + 1, (uint32_t)r);
  if (r >> 32) atomicOr(out + wd + 2, (uint32_t)(r >> 32));
}

// One lane's consecutive tokens, packed in a register pair and written a word at a time.  The lane owns the bits [pos, pos + its
// bits) of a zeroed array and nobody else writes inside that range, so every word that lies wholly inside it is a plain store; the
// word the range starts in (unless it starts on a word boundary) and the word it ends in are shared with the neighbours and go
// through atomicOr.
struct DfPack {
  uint32_t* out; uint64_t acc; uint32_t wd, fill; bool shared;
  __device__ __forceinline__ void open(uint32_t* o, uint32_t pos) { out = o; acc = 0; wd = pos >> 5; fill = pos & 31; shared = fill != 0; }
  __device__ __forceinline__ void put32(uint32_t v, uint32_t nb) {     // nb <= 32 bits of v, fill <= 31 in front of them
    acc |= (uint64_t)v << fill;
    fill += nb;
    if (fill >= 32) {
      const uint32_t w = (uint32_t)acc;
      if (shared) { if (w) atomicOr(out + wd, w); shared = false; } else out[wd] = w;
      acc >>= 32; fill -= 32; ++wd;
    }
  }
  __device__ __forceinline__ void put(uint64_t e) {                    // a token table entry: bits | nbits << 48
    const uint32_t nb = (uint32_t)(e >> 48);
    if (nb <= 32) put32((uint32_t)e, nb);
    else { put32((uint32_t)e, 32); put32((uint32_t)(e >> 32) & 0xffffu, nb - 32); }
  }
  __device__ __forceinline__ void close() { if (fill && (uint32_t)acc) atomicOr(out + wd, (uint32_t)acc); }
};

// One lane's symbol counts: equal consecutive symbols (a literal-dense payload repeats its sign / exponent bytes, a run its
// 258-matches) are added up in a register and reach the LDS histogram as one atomicAdd; the matches' distance symbol as one per lane.
struct DfCount {
  uint32_t* hist; int sym; uint32_t cnt, matches;
  __device__ __forceinline__ void open(uint32_t* h) { hist = h; sym = 0; cnt = 0; matches = 0; }
  __device__ __forceinline__ void add(int s, uint32_t k) {
    if (s == sym) cnt += k;
    else { if (cnt) atomicAdd(hist + sym, cnt); sym = s; cnt = k; }
  }
  __device__ __forceinline__ void close(int dsym) {
    if (cnt) atomicAdd(hist + sym, cnt);
    if (matches) atomicAdd(hist + DF_LL + dsym, matches);
  }
};

enum { DF_MODE_HIST = 0, DF_MODE_COUNT = 1, DF_MODE_WRITE = 2 };

// One lane's DF_PER positions p0 .. of a tile of m bytes.  e[DF_BACK + i] is its byte i (i = DF_PER: the byte behind them),
// e[DF_BACK - k] the byte k in front of them (DF_NOBYTE where the chunk has not begun).  Position p is IN A RUN when its byte equals
// the one P in front of it.  vs = tile position of the last position in front of p0 that is not in a run (negative: in an earlier
// tile).  Position p, at offset j from that start, emits
//   j == 0: the literal;   j % 258 == 0: a match of 258;   else, at the stretch's last byte: a match of j % 258 when that is >= 3,
//   else the j % 258 literals that end here
// which is "literal, then 258-matches while they fit, then the remainder" seen from where each token ENDS, so that the tokens of
// a tile come out in stream order with no knowledge of the bytes behind the tile but one.
template <int MODE, int P>
__device__ __forceinline__ uint32_t df_walk(const uint32_t (&e)[DF_BACK + DF_PER + 1], int p0, int m, bool chunk_ends, int vs,
                                             DfShared& S, uint32_t* out, uint32_t pos) {
  uint32_t bits = 0;
  int jm = p0 - 1 < vs ? 0 : (p0 - 1 - vs) % 258;                     // j % 258 of the position in front of p0
  DfPack pk; DfCount ct;
  if (MODE == DF_MODE_WRITE) pk.open(out, pos);
  if (MODE == DF_MODE_HIST) ct.open(S.hist);
#pragma unroll
  for (int i = 0; i < DF_PER; ++i) {
    const int p = p0 + i;
    if (p < m) {
      const uint32_t b = e[DF_BACK + i];
      const bool st = b != e[DF_BACK + i - P];
      const bool en = (p == m - 1 && chunk_ends) || e[DF_BACK + i + 1] != e[DF_BACK + i + 1 - P];
      jm = st ? 0 : (jm == 257 ? 0 : jm + 1);
      int tok = -1, lit2 = -1;                                         // lit2: a literal in front of tok (a remainder of 2)
      if (st) tok = (int)b;
      else if (jm == 0) tok = DF_TOK_MATCH0 + 255;
      else if (en) { if (jm >= 3) tok = DF_TOK_MATCH0 + jm - 3; else { tok = (int)b; if (jm == 2) lit2 = (int)e[DF_BACK + i - 1]; } }
      if (tok >= 0) {
        if (MODE == DF_MODE_HIST) {
          if (lit2 >= 0) ct.add(lit2, 1u);
          if (tok < 256) ct.add(tok, 1u);
          else { ct.add(df_length_symbol(tok - DF_TOK_MATCH0 + 3), 1u); ++ct.matches; }
        } else {
          const uint64_t t1 = S.tab[tok];
          bits += (uint32_t)(t1 >> 48);
          if (lit2 >= 0) {
            const uint64_t t0 = S.tab[lit2];
            bits += (uint32_t)(t0 >> 48);
            if (MODE == DF_MODE_WRITE) pk.put(t0);
          }
          if (MODE == DF_MODE_WRITE) pk.put(t1);
        }
      }
    }
  }
  if (MODE == DF_MODE_WRITE) pk.close();
  if (MODE == DF_MODE_HIST) ct.close(P == 8 ? 5 : P - 1);
  return bits;
}

// All tiles of one chunk [cs, cs + clen) of the stream.  HIST: counts into S.hist, returns the chunk's CRC-32.  COUNT: returns the
// bits of the chunk's tokens.  WRITE: writes them from bit `bit0` of `out`.  The value is returned to every thread.
template <int MODE, int P>
__device__ __forceinline__ uint32_t df_sweep(const DfStream& X, long cs, int clen, DfShared& S, uint32_t* out, uint32_t bit0) {
  const int t = threadIdx.x, p0 = t * DF_PER;
  int carry = 0;                    // distance from the last position that is not in a run to the tile's first byte
  uint64_t last8 = 0;               // the DF_BACK bytes in front of the tile, the nearest in the top byte
  uint32_t acc = MODE == DF_MODE_HIST ? 0xffffffffu : 0u;            // running CRC register / bit count
  for (int ts = 0; ts < clen; ts += DF_TILE) {
    const int m = clen - ts < DF_TILE ? clen - ts : DF_TILE;
    const bool ends = ts + m == clen;
    const int L = ends ? m : m + 1;                                   // with one byte of lookahead
    const long s = cs + ts;
    int a = 0;
    if (s >= X.npre) {                                                // aligned dwords of the payload; edge words byte by byte
      const uint8_t* g = X.pay + (s - X.npre);
      const uint8_t* pend = X.pay + (X.n - X.npre);
      a = (int)((uintptr_t)g & 3);
      const uint8_t* wb = g - a;
      const int nw = (a + L + 3) >> 2;
      for (int w = t; w < nw; w += DF_THREADS) {
        const uint8_t* p = wb + 4 * (long)w;
        uint32_t v = 0;
        if (p >= X.pay && p + 4 <= pend) v = *(const uint32_t*)p;
        else {
#pragma unroll
          for (int k = 0; k < 4; ++k) if (p + k >= X.pay && p + k < pend) v |= (uint32_t)p[k] << (8 * k);
        }
        S.w[w] = v;
      }
    } else {                                                          // the tile touches the prefix
      for (int k = t; k < L; k += DF_THREADS) ((uint8_t*)S.w)[k] = (uint8_t)X.byte(s + k);
    }
    __syncthreads();
    uint32_t e[DF_BACK + DF_PER + 1];
    {
      const uint4 q = ((const uint4*)S.w)[t];
      const uint32_t w4 = S.w[4 * t + 4];
      const uint32_t wv[5] = {q.x, q.y, q.z, q.w, w4};
      uint32_t al[5];
#pragma unroll
      for (int k = 0; k < 4; ++k) al[k] = (uint32_t)((((uint64_t)wv[k + 1] << 32) | wv[k]) >> (8 * a));
      al[4] = w4 >> (8 * a);
#pragma unroll
      for (int i = 0; i <= DF_PER; ++i) e[DF_BACK + i] = (al[i >> 2] >> (8 * (i & 3))) & 0xffu;
      // the P bytes in front: from the two words in front of the lane's own, for lane 0 from the previous tile
      uint64_t behind = last8;
      if (t > 0) {
        const uint64_t lo = ((uint64_t)S.w[4 * t - 1] << 32) | S.w[4 * t - 2];
        behind = a ? (lo >> (8 * a)) | ((uint64_t)q.x << (64 - 8 * a)) : lo;
      }
      const int have = ts + p0;                                       // positions of the chunk in front of the lane
#pragma unroll
      for (int k = 1; k <= DF_BACK; ++k)
        if (k <= P) e[DF_BACK - k] = k <= have ? (uint32_t)(behind >> (8 * (DF_BACK - k))) & 0xffu : DF_NOBYTE;
    }
    // the last position in front of this lane that is not in a run: in an earlier lane of the tile, else the carry
    int ls = DF_NONE;
#pragma unroll
    for (int i = 0; i < DF_PER; ++i)
      if (p0 + i < m && e[DF_BACK + i] != e[DF_BACK + i - P]) ls = p0 + i;
    int any;
    const int before = df_scan_max(ls, S.red, any);
    const int vs = before != DF_NONE ? before : -carry;
    if (MODE == DF_MODE_HIST) {
      df_walk<DF_MODE_HIST, P>(e, p0, m, ends, vs, S, nullptr, 0);
      // CRC: lane t's 16 bytes from a zero register (lane 0: from the running one), shifted past the full pieces behind it
      const int q = m >> 4, r = m & 15;
      uint32_t reg = t == 0 ? acc : 0u;                               // (with no full piece the register passes through)
      if (t < q) {
#pragma unroll
        for (int i = 0; i < DF_PER; ++i) reg = S.crctab[(reg ^ e[DF_BACK + i]) & 0xffu] ^ (reg >> 8);
        reg = df_mulmod(reg, S.pow128[q - 1 - t]);
      }
      uint32_t x = df_reduce_xor(reg, S.red);
      if (r) {                                                        // the partial last piece continues from the joined register
        if (t == q) {
          uint32_t g = x;
          for (int i = 0; i < r; ++i) g = S.crctab[(g ^ e[DF_BACK + i]) & 0xffu] ^ (g >> 8);
          S.red[4] = (int)g;
        }
        __syncthreads();
        x = (uint32_t)S.red[4];
      }
      acc = x;
    } else if (MODE == DF_MODE_COUNT) {
      acc += df_walk<DF_MODE_COUNT, P>(e, p0, m, ends, vs, S, nullptr, 0);
    } else {
      const uint32_t mine = df_walk<DF_MODE_COUNT, P>(e, p0, m, ends, vs, S, nullptr, 0);
      uint32_t total;
      const uint32_t off = df_scan_sum(mine, S.red, total);
      if (mine) df_walk<DF_MODE_WRITE, P>(e, p0, m, ends, vs, S, out, bit0 + acc + off);
      acc += total;
    }
    carry = any != DF_NONE ? m - any : carry + m;
    if (!ends) {                                                      // (a tile that does not end the chunk is full)
      last8 = 0;
#pragma unroll
      for (int k = 0; k < DF_BACK; ++k) last8 |= (uint64_t)((const uint8_t*)S.w)[a + m - DF_BACK + k] << (8 * k);
    }
    __syncthreads();                                                  // the tile is overwritten next
  }
  if (MODE == DF_MODE_HIST) return ~acc;
  if (MODE == DF_MODE_COUNT) {
    uint32_t total;
    df_scan_sum(acc, S.red, total);
    return total;
  }
  return 0;
}

template <int P>
__global__ __launch_bounds__(DF_THREADS) void deflate_tokenize_kernel(DfStream X, int chunk, uint32_t* __restrict__ hist, uint32_t* __restrict__ crc) {
  __shared__ DfShared S;
  const int t = threadIdx.x;
  for (int k = t; k < DF_HIST; k += DF_THREADS) S.hist[k] = 0;
  df_crc_tables(S.crctab, S.pow128, t);
  __syncthreads();
  const long cs = (long)blockIdx.x * chunk;
  const int clen = (int)(X.n - cs < chunk ? X.n - cs : chunk);
  const uint32_t c = df_sweep<DF_MODE_HIST, P>(X, cs, clen, S, nullptr, 0);
  if (t == 0) { crc[blockIdx.x] = c; atomicAdd(&S.hist[256], 1u); }    // one end-of-block per chunk
  __syncthreads();
  for (int k = t; k < DF_HIST; k += DF_THREADS) if (S.hist[k]) atomicAdd(hist + k, S.hist[k]);
}

// byte q of a chunk written as stored blocks of at most 65535 bytes: [BFINAL, LEN lo, LEN hi, ~LEN lo, ~LEN hi, data ...] each
__device__ __forceinline__ uint32_t df_stored_byte(const DfStream& X, long cs, int clen, bool final, long q) {
  const long blk = q / 65540, r = q % 65540;
  const long rest = (long)clen - blk * 65535;
  const uint32_t len = (uint32_t)(rest < 65535 ? rest : 65535);
  if (r == 0) return final && rest <= 65535 ? 1u : 0u;
  if (r == 1) return len & 0xffu;
  if (r == 2) return len >> 8;
  if (r == 3) return ~len & 0xffu;
  if (r == 4) return (~len >> 8) & 0xffu;
  return X.byte(cs + blk * 65535 + (r - 5));
}

template <int P>
__global__ __launch_bounds__(DF_THREADS) void deflate_emit_kernel(DfStream X, int chunk, long nchunks, int ends_stream, const uint64_t* __restrict__ tab,
                                                                  const uint32_t* __restrict__ hdr, int hdr_bits, uint8_t* __restrict__ regions,
                                                                  long region, int32_t* __restrict__ sizes) {
  __shared__ DfShared S;
  const int t = threadIdx.x;
  for (int k = t; k < DF_TOK_SLOTS; k += DF_THREADS) S.tab[k] = tab[k];
  __syncthreads();
  const long c = blockIdx.x, cs = c * chunk;
  const int clen = (int)(X.n - cs < chunk ? X.n - cs : chunk);
  const bool final = ends_stream && c == nchunks - 1;
  uint32_t* out = (uint32_t*)(regions + c * region);
  const uint32_t tok_bits = df_sweep<DF_MODE_COUNT, P>(X, cs, clen, S, nullptr, 0);
  const uint64_t eob = S.tab[DF_TOK_EOB];
  // BFINAL, header, tokens, end of block; every chunk but the stream's last is closed by an empty stored block: 3 bits, pad, 00 00 ff ff
  const long bits = 1 + (long)hdr_bits + tok_bits + (long)(eob >> 48) + (final ? 0 : 3);
  const long huff = ((bits + 7) >> 3) + (final ? 0 : 4);
  const long stored = df_stored_size(clen);
  if (stored < huff) {
    for (long w = t; w < (stored + 3) >> 2; w += DF_THREADS) {
      uint32_t v = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) if (4 * w + k < stored) v |= df_stored_byte(X, cs, clen, final, 4 * w + k) << (8 * k);
      out[w] = v;
    }
    if (t == 0) sizes[c] = (int32_t)stored;
    return;
  }
  if (t == 0 && final) atomicOr(out, 1u);
  for (int k = t; 32 * k < hdr_bits; k += DF_THREADS) df_put(out, 1 + 32 * k, hdr[k]);
  df_sweep<DF_MODE_WRITE, P>(X, cs, clen, S, out, 1 + hdr_bits);
  if (t == 0) {
    df_put(out, 1 + hdr_bits + tok_bits, eob & 0xffffffffffffull);
    if (!final) df_put(out, (uint32_t)(8 * (((bits + 7) >> 3) + 2)), 0xffffull);
    sizes[c] = (int32_t)huff;
  }
}

// sizes -> exclusive offsets in place; the total and the chunk CRCs go to the head of `dst`
__global__ __launch_bounds__(MT_SCAN_THREADS) void deflate_scan_kernel(int32_t* __restrict__ sizes, long nchunks, int64_t* __restrict__ total) {
  const int64_t s = mt_scan_units(sizes, nchunks);
  if (threadIdx.x == 0) *total = s;
}
__global__ __launch_bounds__(DF_THREADS) void deflate_compact_kernel(const uint8_t* __restrict__ regions, long region, const int32_t* __restrict__ offs,
                                                                     long nchunks, const uint32_t* __restrict__ crc, uint8_t* __restrict__ dst,
                                                                     size_t data) {
  const long c = blockIdx.x;
  const int64_t total = *(const int64_t*)dst;
  const long o = (uint32_t)offs[c], e = c + 1 < nchunks ? (long)(uint32_t)offs[c + 1] : (long)total;      // (the offsets are kept mod 2^32)
  const uint8_t* src = regions + c * region;
  for (long k = threadIdx.x; k < e - o; k += DF_THREADS) dst[data + o + k] = src[k];
  if (threadIdx.x == 0) ((uint32_t*)(dst + 8))[c] = crc[c];
}

extern "C" size_t mt_deflate_workspace(long n, int chunk) {
  if (!df_args_ok(n, chunk)) return 0;
  const long nchunks = df_chunks(n, chunk);
  return df_ws_regions(nchunks) + (size_t)nchunks * df_region(chunk);
}

extern "C" size_t mt_deflate_bound(long n, int chunk) {
  if (!df_args_ok(n, chunk)) return 0;
  const long nchunks = df_chunks(n, chunk);
  return df_out_data(nchunks) + (size_t)nchunks * df_region(chunk);
}

#define DF_CHECK_ARGS(who)                                                                                                            \
  MT_REQUIRE(n_payload >= 0 && n_prefix >= 0 && n_prefix <= MT_DEFLATE_MAX_PREFIX, who ": %ld payload and %d prefix bytes (prefix 0 .. %d)", \
             n_payload, n_prefix, MT_DEFLATE_MAX_PREFIX);                                                                             \
  MT_REQUIRE(n_payload + n_prefix <= 2147483647l, who ": %ld bytes; at most INT32_MAX are encoded as one member", n_payload + n_prefix); \
  MT_REQUIRE(chunk >= MT_DEFLATE_MIN_CHUNK && chunk <= MT_DEFLATE_MAX_CHUNK, who ": chunk of %d bytes (%d .. %d)", chunk,            \
             MT_DEFLATE_MIN_CHUNK, MT_DEFLATE_MAX_CHUNK);                                                                             \
  MT_REQUIRE(df_period_ok(period), who ": a period of %d bytes (1, 2, 4 or 8)", period);                                              \
  MT_REQUIRE(ws && (n_payload == 0 || payload) && (n_prefix == 0 || prefix), who ": NULL argument");                                  \
  MT_REQUIRE(((uintptr_t)ws & 15) == 0, who ": the workspace must be 16-byte aligned")

#define DF_LAUNCH_PERIOD(kernel, ...)                                                                      \
  switch (period) {                                                                                        \
    case 1: hipLaunchKernelGGL(kernel<1>, dim3((unsigned)nchunks), dim3(DF_THREADS), 0, s, __VA_ARGS__); break; \
    case 2: hipLaunchKernelGGL(kernel<2>, dim3((unsigned)nchunks), dim3(DF_THREADS), 0, s, __VA_ARGS__); break; \
    case 4: hipLaunchKernelGGL(kernel<4>, dim3((unsigned)nchunks), dim3(DF_THREADS), 0, s, __VA_ARGS__); break; \
    default: hipLaunchKernelGGL(kernel<8>, dim3((unsigned)nchunks), dim3(DF_THREADS), 0, s, __VA_ARGS__); break; \
  }

extern "C" int mt_deflate_tokenize_period(const uint8_t* payload, long n_payload, const uint8_t* prefix, int n_prefix, int chunk, int period,
                                          void* ws, size_t ws_bytes, uint32_t* hist, mt_stream_t stream) {
  DF_CHECK_ARGS("deflate_tokenize");
  MT_REQUIRE(hist, "deflate_tokenize: NULL argument");
  const long n = n_payload + n_prefix, nchunks = df_chunks(n, chunk);
  MT_REQUIRE_WORKSPACE("deflate_tokenize", ws_bytes, mt_deflate_workspace(n, chunk));
  hipStream_t s = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)ws;
  if (hipMemsetAsync(hist, 0, DF_HIST * sizeof(uint32_t), s) != hipSuccess ||
      (n_prefix && hipMemcpyAsync(w, prefix, (size_t)n_prefix, hipMemcpyHostToDevice, s) != hipSuccess)) {
    mt_set_error("deflate_tokenize: memset / prefix copy failed");
    return MT_EHIP;
  }
  DfStream X; X.pre = w; X.pay = payload; X.npre = n_prefix; X.n = n;
  DF_LAUNCH_PERIOD(deflate_tokenize_kernel, X, chunk, hist, (uint32_t*)(w + DF_WS_CRC));
  MT_CHECK_LAUNCH("deflate_tokenize");
  return MT_OK;
}

extern "C" int mt_deflate_emit_period(const uint8_t* payload, long n_payload, const uint8_t* prefix, int n_prefix, int chunk, int period,
                                      int final, const uint64_t* table, const uint32_t* header, int header_bits,
                                      void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes, mt_stream_t stream) {
  DF_CHECK_ARGS("deflate_emit");
  MT_REQUIRE(table && header && out, "deflate_emit: NULL argument");
  MT_REQUIRE(header_bits >= 17 && header_bits <= DF_HDR_WORDS * 32, "deflate_emit: a dynamic block header of %d bits", header_bits);
  MT_REQUIRE(((uintptr_t)out & 7) == 0, "deflate_emit: out must be 8-byte aligned");
  for (int k = 0; k < DF_TOK_SLOTS; ++k)
    MT_REQUIRE((table[k] >> 48) <= 48, "deflate_emit: token %d of %d bits", k, (int)(table[k] >> 48));
  MT_REQUIRE((table[DF_TOK_EOB] >> 48) >= 1, "deflate_emit: the end-of-block symbol has no code");
  const long n = n_payload + n_prefix, nchunks = df_chunks(n, chunk), region = df_region(chunk);
  MT_REQUIRE_WORKSPACE("deflate_emit", ws_bytes, mt_deflate_workspace(n, chunk));
  MT_REQUIRE(out_bytes >= mt_deflate_bound(n, chunk), "deflate_emit: out of %zu bytes, %zu needed", out_bytes, mt_deflate_bound(n, chunk));
  hipStream_t s = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)ws;
  uint8_t* regions = w + df_ws_regions(nchunks);
  uint32_t* crc = (uint32_t*)(w + DF_WS_CRC);
  int32_t* sizes = (int32_t*)(crc + nchunks);
  if ((n_prefix && hipMemcpyAsync(w, prefix, (size_t)n_prefix, hipMemcpyHostToDevice, s) != hipSuccess) ||
      hipMemcpyAsync(w + DF_WS_TAB, table, DF_TOK_SLOTS * sizeof(uint64_t), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(w + DF_WS_HDR, header, (size_t)((header_bits + 31) / 32) * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemsetAsync(regions, 0, (size_t)nchunks * region, s) != hipSuccess) {
    mt_set_error("deflate_emit: table copy / memset failed");
    return MT_EHIP;
  }
  DfStream X; X.pre = w; X.pay = payload; X.npre = n_prefix; X.n = n;
  DF_LAUNCH_PERIOD(deflate_emit_kernel, X, chunk, nchunks, final ? 1 : 0, (const uint64_t*)(w + DF_WS_TAB), (const uint32_t*)(w + DF_WS_HDR),
                   header_bits, regions, region, sizes);
  MT_CHECK_LAUNCH("deflate_emit");
  hipLaunchKernelGGL(deflate_scan_kernel, dim3(1), dim3(MT_SCAN_THREADS), 0, s, sizes, nchunks, (int64_t*)out);
  MT_CHECK_LAUNCH("deflate_emit (scan)");
  hipLaunchKernelGGL(deflate_compact_kernel, dim3((unsigned)nchunks), dim3(DF_THREADS), 0, s, regions, region, sizes, nchunks, crc, out,
                     df_out_data(nchunks));
  MT_CHECK_LAUNCH("deflate_emit (compact)");
  return MT_OK;
}

extern "C" int mt_deflate_tokenize(const uint8_t* payload, long n_payload, const uint8_t* prefix, int n_prefix, int chunk,
                                   void* ws, size_t ws_bytes, uint32_t* hist, mt_stream_t stream) {
  return mt_deflate_tokenize_period(payload, n_payload, prefix, n_prefix, chunk, 1, ws, ws_bytes, hist, stream);
}

extern "C" int mt_deflate_emit(const uint8_t* payload, long n_payload, const uint8_t* prefix, int n_prefix, int chunk,
                               const uint64_t* table, const uint32_t* header, int header_bits,
                               void* ws, size_t ws_bytes, uint8_t* out, size_t out_bytes, mt_stream_t stream) {
  return mt_deflate_emit_period(payload, n_payload, prefix, n_prefix, chunk, 1, 1, table, header, header_bits, ws, ws_bytes, out, out_bytes,
                                stream);
}
