// Evaluation on the device (evaluation/evaluator.py, evaluation/metrics.py of the reference).
//   mt_seg_joint_hist      one pass over two uint8 label volumes -> exact 64-bit joint histogram of the remapped labels; every
//                          label entry's tp / fp / fn / tn is a sum of its cells.
//   mt_surface_distances   medpy's __surface_distances in both directions: border = mask ^ erosion(mask), exact anisotropic
//                          Euclidean distance transform of the other mask's border, read at this mask's border voxels.
//                          Seven launches:
//     sd_border_kernel     bm[v] = bit 0 border(test), bit 1 border(ref); border voxels counted per 2048-voxel chunk;
//     sd_scan_kernel       exclusive scan of the chunk counts (one workgroup, fixed order);
//     sd_compact_kernel    q[rank] = v: the border voxels in linear order, test's first, then ref's;
//     sd_rows_kernel       g1[v] = signed x offset of the nearest border voxel of the same row, per mask (bit scans), and which
//                          rows and planes hold a border voxel at all;
//     sd_query_kernel      for each border voxel the nearest border voxel of the other mask: the rows around it, nearest first,
//                          each row's candidate from g1, until no unvisited row can be nearer; the distance is
//                          sqrt((dz sz)^2 + (dy sy)^2 + (dx sx)^2) in fp64 of the integer offsets to the site found;
//     sd_reduce_kernel x2  count, maximum and sum per direction: fixed 4096-element chunks, fixed tree, no atomics.
// (mt_sd_count_within, which counts those distances against tolerances, is surface_dice.hip.)
// Every floating-point result is a function of the inputs alone (integer atomics only): two runs are bit-identical.
#include "stream_common.h"

#define MX_THREADS 256

// ---- joint label histogram -------------------------------------------------------------------------------------------------
struct SegRemap { uint32_t w[64]; };     // remap[v] = byte v
#define SH_LDS_MAXC 64

// Voxels [0, head) and [head + 16 nvec, V) are read bytewise, the 16-byte vectors between them as uint4 (test + head and
// ref + head are 16-byte aligned).  The (0, 0) pair - more than 90 % of a label map - is counted in a register and added
// once per wave; every other pair is one LDS atomic (C <= 64) or one global atomic.
template <bool LDSH>
__global__ __launch_bounds__(MX_THREADS) void seg_hist_kernel(const uint8_t* __restrict__ t, const uint8_t* __restrict__ r, long V,
                                                              long head, long nvec, const SegRemap remap, int C,
                                                              unsigned long long* __restrict__ hist) {
  __shared__ uint32_t rmw[64];
  __shared__ int lh[LDSH ? SH_LDS_MAXC * SH_LDS_MAXC : 1];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 64; ++k) rmw[k] = remap.w[k];
  }
  if (LDSH)
    for (int i = threadIdx.x; i < C * C; i += MX_THREADS) lh[i] = 0;
  __syncthreads();
  const uint8_t* rm = (const uint8_t*)rmw;
  long bg = 0;
  auto add = [&](unsigned a, unsigned b) {
    if ((a | b) == 0) { ++bg; return; }
    const int cell = (int)rm[a] * C + (int)rm[b];
    if (LDSH) atomicAdd(lh + cell, 1);
    else atomicAdd(hist + cell, 1ull);
  };
  const long gtid = (long)blockIdx.x * MX_THREADS + threadIdx.x, gstride = (long)gridDim.x * MX_THREADS;
  const uint4* tv = (const uint4*)(t + head);
  const uint4* rv = (const uint4*)(r + head);
  for (long i = gtid; i < nvec; i += gstride) {
    const uint4 a = tv[i], b = rv[i];
    if ((a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0) { bg += 16; continue; }
    const unsigned aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if ((aw[k] | bw[k]) == 0) { bg += 4; continue; }
#pragma unroll
      for (int j = 0; j < 4; ++j) add((aw[k] >> (8 * j)) & 255u, (bw[k] >> (8 * j)) & 255u);
    }
  }
  for (long i = gtid; i < head; i += gstride) add(t[i], r[i]);
  for (long i = head + nvec * 16 + gtid; i < V; i += gstride) add(t[i], r[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bg += __shfl_xor(bg, off, 64);
  if ((threadIdx.x & 63) == 0 && bg) atomicAdd(hist + ((int)rm[0] * C + (int)rm[0]), (unsigned long long)bg);
  if (LDSH) {
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += MX_THREADS)
      if (lh[i]) atomicAdd(hist + i, (unsigned long long)lh[i]);
  }
}

extern "C" int mt_seg_joint_hist(const uint8_t* test, const uint8_t* ref, long V, const uint8_t* remap, int C, int64_t* hist,
                                 mt_stream_t stream) {
  MT_REQUIRE(test && ref && remap && hist, "seg_joint_hist: null pointer");
  MT_REQUIRE(V > 0, "seg_joint_hist: bad voxel count %ld", V);
  MT_REQUIRE(C >= 1 && C <= 256, "seg_joint_hist: %d classes (1..256)", C);
  SegRemap rm;
  for (int k = 0; k < 64; ++k) rm.w[k] = 0;
  for (int k = 0; k < 256; ++k) {
    MT_REQUIRE(remap[k] < C, "seg_joint_hist: remap[%d] = %d is not below C = %d", k, (int)remap[k], C);
    rm.w[k >> 2] |= (uint32_t)remap[k] << (8 * (k & 3));
  }
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(hist, 0, sizeof(int64_t) * C * C, s) != hipSuccess) {
    mt_set_error("seg_joint_hist: hipMemsetAsync failed");
    return MT_EHIP;
  }
  long head = (16 - (long)((uintptr_t)test & 15)) & 15, nvec = 0;
  if (head > V) head = V;
  if ((((uintptr_t)ref + head) & 15) == 0) nvec = (V - head) / 16;
  else head = 0;                                      // different misalignment: everything bytewise
  const long items = nvec ? nvec : V;
  long grid = (items + MX_THREADS - 1) / MX_THREADS;
  const long cap = mt_stream_cap(), need = (V >> 30) + 1;     // a workgroup's int32 LDS counts stay below 2^31
  if (grid > cap) grid = cap > need ? cap : need;
  if (C <= SH_LDS_MAXC)
    hipLaunchKernelGGL(seg_hist_kernel<true>, dim3((unsigned)grid), dim3(MX_THREADS), 0, s, test, ref, V, head, nvec, rm, C,
                       (unsigned long long*)hist);
  else
    hipLaunchKernelGGL(seg_hist_kernel<false>, dim3((unsigned)grid), dim3(MX_THREADS), 0, s, test, ref, V, head, nvec, rm, C,
                       (unsigned long long*)hist);
  MT_CHECK_LAUNCH("seg_joint_hist");
  return MT_OK;
}

// ---- surface distances -----------------------------------------------------------------------------------------------------
#define SD_CHUNK 2048                     // voxels per workgroup of the border / compaction launches (8 per thread)
#define SD_IT (SD_CHUNK / MX_THREADS)
#define SD_INF 32767                      // "no border voxel" in the int16 offset arrays
#define SD_MAXDIM 32766
#define SD_RCHUNK 4096                    // elements per partial of the reduction
#define SD_ROWWORDS 512                   // 64-bit words of one row's border bits (W <= 32766)

struct SDGeom { int D, H, W; double sz, sy, sx; };

// border(X) = X ^ binary_erosion(X, generate_binary_structure(3, conn)), border_value 0: a mask voxel is a border voxel when a
// neighbour of the structure (city-block distance <= conn inside the 3x3x3 cube) is outside the mask or outside the volume.
__global__ __launch_bounds__(MX_THREADS) void sd_border_kernel(const uint8_t* __restrict__ test, const uint8_t* __restrict__ ref,
                                                               const MtMember m, const SDGeom g, int conn, long V,
                                                               uint8_t* __restrict__ bm, int32_t* __restrict__ cnt) {
  __shared__ int red[4][2];
  int na = 0, nb = 0;                                         // wave-uniform
  const long base = (long)blockIdx.x * SD_CHUNK;
  for (int j = 0; j < SD_IT; ++j) {
    const long v = base + j * MX_THREADS + threadIdx.x;
    bool ba = false, bb = false;
    if (v < V) {
      const bool a = mt_member(m, test[v]), b = mt_member(m, ref[v]);
      if (a | b) {
        const int w = (int)(v % g.W), h = (int)((v / g.W) % g.H), d = (int)(v / ((long)g.W * g.H));
        bool ea = a, eb = b;
        for (int dz = -1; dz <= 1; ++dz)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int nz = (dz != 0) + (dy != 0) + (dx != 0);
              if (nz == 0 || nz > conn) continue;
              const int zz = d + dz, yy = h + dy, xx = w + dx;
              if (zz < 0 || zz >= g.D || yy < 0 || yy >= g.H || xx < 0 || xx >= g.W) { ea = false; eb = false; continue; }
              const long nv = ((long)zz * g.H + yy) * g.W + xx;
              if (ea) ea = mt_member(m, test[nv]);
              if (eb) eb = mt_member(m, ref[nv]);
            }
        ba = a && !ea;
        bb = b && !eb;
      }
      bm[v] = (uint8_t)((ba ? 1 : 0) | (bb ? 2 : 0));
    }
    na += __popcll(__ballot(ba));
    nb += __popcll(__ballot(bb));
  }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = na; red[threadIdx.x >> 6][1] = nb; }
  __syncthreads();
  if (threadIdx.x < 2) cnt[2 * (long)blockIdx.x + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// off[b] = sum of cnt[< b] per mask, tot = the two totals.  One workgroup; thread t owns a contiguous run of chunks.
__global__ __launch_bounds__(MX_THREADS) void sd_scan_kernel(const int32_t* __restrict__ cnt, int nblk, int32_t* __restrict__ off,
                                                             int32_t* __restrict__ tot) {
  __shared__ int part[MX_THREADS][2];
  const int per = (nblk + MX_THREADS - 1) / MX_THREADS;
  const int b0 = min(nblk, (int)threadIdx.x * per), b1 = min(nblk, b0 + per);
  int sa = 0, sb = 0;
  for (int b = b0; b < b1; ++b) { sa += cnt[2 * b]; sb += cnt[2 * b + 1]; }
  part[threadIdx.x][0] = sa; part[threadIdx.x][1] = sb;
  __syncthreads();
  int ea = 0, eb = 0;
  for (int k = 0; k < (int)threadIdx.x; ++k) { ea += part[k][0]; eb += part[k][1]; }
  for (int b = b0; b < b1; ++b) {
    off[2 * b] = ea; off[2 * b + 1] = eb;
    ea += cnt[2 * b]; eb += cnt[2 * b + 1];
  }
  if (threadIdx.x == MX_THREADS - 1) { tot[0] = ea; tot[1] = eb; }
}

// q[rank] = v in linear order: test's border voxels at [0, nA), ref's at [nA, nA + nB); ranks at or beyond cap are dropped.
__global__ __launch_bounds__(MX_THREADS) void sd_compact_kernel(const uint8_t* __restrict__ bm, long V, const int32_t* __restrict__ off,
                                                                const int32_t* __restrict__ tot, long cap, int32_t* __restrict__ q) {
  __shared__ int wc[SD_IT][4][2];
  const long base = (long)blockIdx.x * SD_CHUNK;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint8_t b[SD_IT];
  int ra[SD_IT], rb[SD_IT];
#pragma unroll
  for (int j = 0; j < SD_IT; ++j) {
    const long v = base + j * MX_THREADS + threadIdx.x;
    b[j] = v < V ? bm[v] : 0;
    const uint64_t ma = __ballot(b[j] & 1), mb = __ballot(b[j] & 2);
    ra[j] = __popcll(ma & below); rb[j] = __popcll(mb & below);
    if (lane == 0) { wc[j][wave][0] = __popcll(ma); wc[j][wave][1] = __popcll(mb); }
  }
  __syncthreads();
  long pa = off[2 * (long)blockIdx.x], pb = (long)tot[0] + off[2 * (long)blockIdx.x + 1];
#pragma unroll
  for (int j = 0; j < SD_IT; ++j) {
    for (int k = 0; k < 4; ++k) {
      if (k == wave) {
        const long v = base + j * MX_THREADS + threadIdx.x;
        if ((b[j] & 1) && pa + ra[j] < cap) q[pa + ra[j]] = (int32_t)v;
        if ((b[j] & 2) && pb + rb[j] < cap) q[pb + rb[j]] = (int32_t)v;
      }
      pa += wc[j][k][0]; pb += wc[j][k][1];
    }
  }
}

__device__ __forceinline__ int sd_nearest_bit(const uint64_t* wd, int nw, int x) {
  // signed offset of the nearest set bit of wd[0 .. nw) to position x, SD_INF when there is none (left wins a tie)
  const int wi = x >> 6, bit = x & 63;
  int right = SD_INF, left = SD_INF;
  uint64_t r = wd[wi] >> bit;
  if (r) right = __ffsll((unsigned long long)r) - 1;
  else
    for (int k = wi + 1; k < nw; ++k)
      if (wd[k]) { right = (k << 6) + __ffsll((unsigned long long)wd[k]) - 1 - x; break; }
  uint64_t l = wd[wi] << (63 - bit);
  if (l) left = __clzll((long long)l);
  else
    for (int k = wi - 1; k >= 0; --k)
      if (wd[k]) { left = x - ((k << 6) + 63 - __clzll((long long)wd[k])); break; }
  if (left == SD_INF && right == SD_INF) return SD_INF;
  return left <= right ? -left : right;
}

// One wave per row (z, y): the row's border bits of both masks as 64-bit words in LDS, then the nearest set bit for every x.
// pflag[z] / rflag[row] get bit 0 / 1 when the plane / the row holds a border voxel of test / ref.
__global__ __launch_bounds__(MX_THREADS) void sd_rows_kernel(const uint8_t* __restrict__ bm, const SDGeom g, long nrows,
                                                             short2* __restrict__ g1, int32_t* __restrict__ pflag,
                                                             uint8_t* __restrict__ rflag) {
  __shared__ uint64_t bits[4][2][SD_ROWWORDS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nw = (g.W + 63) >> 6;
  uint64_t* wa = bits[wave][0];
  uint64_t* wb = bits[wave][1];
  for (long row = (long)blockIdx.x * 4 + wave; row < nrows; row += (long)gridDim.x * 4) {
    const uint8_t* src = bm + row * g.W;
    uint64_t anya = 0, anyb = 0;
    for (int k = 0; k < nw; ++k) {
      const int x = (k << 6) + lane;
      const uint8_t b = x < g.W ? src[x] : 0;
      const uint64_t ma = __ballot(b & 1), mb = __ballot(b & 2);
      if (lane == 0) { wa[k] = ma; wb[k] = mb; }
      anya |= ma; anyb |= mb;
    }
    // the words were written by lane 0 of this wave only: make them visible to the other lanes of the wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane == 0) {
      rflag[row] = (uint8_t)((anya ? 1 : 0) | (anyb ? 2 : 0));
      if (anya | anyb) atomicOr(pflag + row / g.H, (anya ? 1 : 0) | (anyb ? 2 : 0));
    }
    short2* dst = g1 + row * g.W;
    for (int x = lane; x < g.W; x += 64) {
      short2 o;
      o.x = (short)(anya ? sd_nearest_bit(wa, nw, x) : SD_INF);
      o.y = (short)(anyb ? sd_nearest_bit(wb, nw, x) : SD_INF);
      dst[x] = o;
    }
    __builtin_amdgcn_wave_barrier();                          // the words are rewritten for the next row
  }
}

// One thread per border voxel: test's query the ref border (mask 1 of g1), ref's the test border (mask 0).  Exhaustive search
// over the rows (z', y') around the voxel, nearest first: planes outwards from z until (dz sz)^2 alone reaches the best squared
// distance so far, inside a plane rows outwards from y until (dz sz)^2 + (dy sy)^2 does; a row's only candidate is its border
// voxel nearest to x (g1).  Every row that could hold a nearer site is visited, so the minimum is exact; planes and rows without
// a border voxel (pflag, rflag) cost one cached byte.
__global__ __launch_bounds__(MX_THREADS) void sd_query_kernel(const int32_t* __restrict__ q, const int32_t* __restrict__ tot, long cap,
                                                              const short* __restrict__ g1, const int32_t* __restrict__ pflag,
                                                              const uint8_t* __restrict__ rflag, const SDGeom g,
                                                              double* __restrict__ out) {
  const long na = tot[0];
  long n = na + tot[1];
  if (n > cap) n = cap;
  const long HW = (long)g.H * g.W;
  for (long i = (long)blockIdx.x * MX_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * MX_THREADS) {
    const int mask = i < na ? 1 : 0;
    const long v = q[i];
    const int z = (int)(v / HW), y = (int)((v - (long)z * HW) / g.W), x = (int)(v - (long)z * HW - (long)y * g.W);
    double best = __builtin_huge_val();
    int bz = 0, by = 0, bx = 0;
    const int kzmax = max(z, g.D - 1 - z), kymax = max(y, g.H - 1 - y);
    for (int kz = 0; kz <= kzmax; ++kz) {
      const double tz = (double)kz * g.sz, kz2 = tz * tz;
      if (kz2 >= best) break;
      for (int sgz = 0; sgz < (kz ? 2 : 1); ++sgz) {
        const int zz = sgz ? z + kz : z - kz;
        if (zz < 0 || zz >= g.D || !((pflag[zz] >> mask) & 1)) continue;
        const uint8_t* rf = rflag + (long)zz * g.H;
        const short* pl = g1 + ((long)zz * HW + x) * 2 + mask;                 // + y' * W * 2
        for (int ky = 0; ky <= kymax; ++ky) {
          const double ty = (double)ky * g.sy, zy2 = kz2 + ty * ty;
          if (zy2 >= best) break;
          for (int sgy = 0; sgy < (ky ? 2 : 1); ++sgy) {
            const int yy = sgy ? y + ky : y - ky;
            if (yy < 0 || yy >= g.H || !((rf[yy] >> mask) & 1)) continue;
            const int dx = pl[(long)yy * g.W * 2];
            const double tx = (double)dx * g.sx, d2 = zy2 + tx * tx;
            if (d2 < best) { best = d2; bz = zz - z; by = yy - y; bx = dx; }
          }
        }
      }
    }
    double d = __builtin_huge_val();                                        // the other mask has no border voxel
    if (best < __builtin_huge_val()) {
      const double tz = (double)bz * g.sz, ty = (double)by * g.sy, tx = (double)bx * g.sx;
      d = sqrt(tz * tz + ty * ty + tx * tx);
    }
    out[i] = d;
  }
}

// Fixed-order sum and maximum of one workgroup's values (shuffle butterfly, then the four waves in order).
__device__ __forceinline__ void sd_block_sum_max(double& s, double& m, double (*red)[2]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    m = fmax(m, __shfl_xor(m, off, 64));
  }
  __syncthreads();                                             // red may still be read from the previous use
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s; red[threadIdx.x >> 6][1] = m; }
  __syncthreads();
  s = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
  m = fmax(fmax(red[0][1], red[1][1]), fmax(red[2][1], red[3][1]));
}

__device__ __forceinline__ void sd_ranges(const int32_t* tot, long cap, long (&lo)[2], long (&hi)[2]) {
  const long na = tot[0], nb = tot[1];
  lo[0] = 0; hi[0] = na < cap ? na : cap;
  lo[1] = hi[0]; hi[1] = na + nb < cap ? na + nb : cap;
  if (na > cap) hi[1] = lo[1];
}

// partial[dir][c] = (sum, max) of elements [lo + 4096 c, lo + 4096 (c + 1)) of direction dir; thread t adds elements
// t, t + 256, ... of the chunk in that order.
__global__ __launch_bounds__(MX_THREADS) void sd_reduce1_kernel(const double* __restrict__ x, const int32_t* __restrict__ tot, long cap,
                                                                long maxchunks, double* __restrict__ partial) {
  __shared__ double red[4][2];
  long lo[2], hi[2];
  sd_ranges(tot, cap, lo, hi);
  for (int dir = 0; dir < 2; ++dir) {
    const long nch = (hi[dir] - lo[dir] + SD_RCHUNK - 1) / SD_RCHUNK;
    for (long c = blockIdx.x; c < nch && c < maxchunks; c += gridDim.x) {
      double s = 0.0, m = 0.0;
      for (int j = 0; j < SD_RCHUNK / MX_THREADS; ++j) {
        const long i = lo[dir] + c * SD_RCHUNK + j * MX_THREADS + threadIdx.x;
        if (i < hi[dir]) { const double v = x[i]; s += v; m = fmax(m, v); }
      }
      sd_block_sum_max(s, m, red);
      if (threadIdx.x == 0) { partial[(dir * maxchunks + c) * 2] = s; partial[(dir * maxchunks + c) * 2 + 1] = m; }
    }
  }
}

// stats = (count, max, sum) of test -> ref, then of ref -> test.  One workgroup.
__global__ __launch_bounds__(MX_THREADS) void sd_reduce2_kernel(const double* __restrict__ partial, const int32_t* __restrict__ tot,
                                                                long cap, long maxchunks, double* __restrict__ stats) {
  __shared__ double red[4][2];
  long lo[2], hi[2];
  sd_ranges(tot, cap, lo, hi);
  for (int dir = 0; dir < 2; ++dir) {
    long nch = (hi[dir] - lo[dir] + SD_RCHUNK - 1) / SD_RCHUNK;
    if (nch > maxchunks) nch = maxchunks;
    double s = 0.0, m = 0.0;
    for (long c = threadIdx.x; c < nch; c += MX_THREADS) {
      s += partial[(dir * maxchunks + c) * 2];
      m = fmax(m, partial[(dir * maxchunks + c) * 2 + 1]);
    }
    sd_block_sum_max(s, m, red);
    if (threadIdx.x == 0) {
      stats[3 * dir] = (double)tot[dir];
      stats[3 * dir + 1] = m;
      stats[3 * dir + 2] = s;
    }
  }
}

static size_t sd_align(size_t n) { return (n + 255) & ~(size_t)255; }

struct SDLayout { size_t bm, g1, rflag, cnt, off, tot, pflag, q, partial, total; long nblk, maxchunks; };

static SDLayout sd_layout(long V, int D, int H, long cap) {
  SDLayout L;
  L.nblk = (V + SD_CHUNK - 1) / SD_CHUNK;
  L.maxchunks = (cap + SD_RCHUNK - 1) / SD_RCHUNK + 1;
  size_t p = 0;
  L.bm = p; p += sd_align((size_t)V);
  L.g1 = p; p += sd_align((size_t)V * 4);
  L.rflag = p; p += sd_align((size_t)D * H);
  L.cnt = p; p += sd_align((size_t)L.nblk * 8);
  L.off = p; p += sd_align((size_t)L.nblk * 8);
  L.tot = p; p += sd_align(8);
  L.pflag = p; p += sd_align((size_t)D * 4);
  L.q = p; p += sd_align((size_t)cap * 4);
  L.partial = p; p += sd_align((size_t)L.maxchunks * 2 * 2 * 8);
  L.total = p;
  return L;
}

static bool sd_shape_ok(int D, int H, int W) {
  return D > 0 && H > 0 && W > 0 && (long)D * H * W <= (long)INT32_MAX && D <= SD_MAXDIM && H <= SD_MAXDIM && W <= SD_MAXDIM;
}

extern "C" size_t mt_surface_distances_workspace(int D, int H, int W, long capacity) {
  if (!sd_shape_ok(D, H, W) || capacity < 1) return 0;
  return sd_layout((long)D * H * W, D, H, capacity).total;
}

extern "C" int mt_surface_distances(const uint8_t* test, const uint8_t* ref, int D, int H, int W, const uint8_t* member,
                                    const double* spacing, int connectivity, double* out, long capacity, double* stats, void* ws,
                                    size_t ws_bytes, mt_stream_t stream) {
  MT_REQUIRE(test && ref && member && out && stats && ws, "surface_distances: null pointer");
  MT_REQUIRE(D > 0 && H > 0 && W > 0, "surface_distances: bad shape %d x %d x %d", D, H, W);
  const long V = (long)D * H * W;
  MT_REQUIRE(V <= (long)INT32_MAX, "surface_distances: %ld voxels exceed the int32 index range", V);
  MT_REQUIRE(sd_shape_ok(D, H, W), "surface_distances: an axis of %d x %d x %d exceeds %d (int16 offsets)", D, H, W, SD_MAXDIM);
  MT_REQUIRE(connectivity >= 1 && connectivity <= 3, "surface_distances: connectivity %d (1..3)", connectivity);
  MT_REQUIRE(capacity >= 1, "surface_distances: capacity %ld", capacity);
  SDGeom g;
  g.D = D; g.H = H; g.W = W;
  g.sz = spacing ? spacing[0] : 1.0; g.sy = spacing ? spacing[1] : 1.0; g.sx = spacing ? spacing[2] : 1.0;
  MT_REQUIRE(g.sz > 0 && g.sy > 0 && g.sx > 0 && g.sz < 1e100 && g.sy < 1e100 && g.sx < 1e100,
             "surface_distances: spacing (%g, %g, %g) must be positive and finite", g.sz, g.sy, g.sx);
  const SDLayout L = sd_layout(V, D, H, capacity);
  MT_REQUIRE(ws_bytes >= L.total, "surface_distances: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
  MT_REQUIRE(((uintptr_t)ws & 15) == 0, "surface_distances: workspace must be 16-byte aligned");
  const MtMember m = mt_member_from_bytes(member);
  char* base = (char*)ws;
  uint8_t* bm = (uint8_t*)(base + L.bm);
  short* g1 = (short*)(base + L.g1);
  uint8_t* rflag = (uint8_t*)(base + L.rflag);
  int32_t* cnt = (int32_t*)(base + L.cnt);
  int32_t* off = (int32_t*)(base + L.off);
  int32_t* tot = (int32_t*)(base + L.tot);
  int32_t* pflag = (int32_t*)(base + L.pflag);
  int32_t* q = (int32_t*)(base + L.q);
  double* partial = (double*)(base + L.partial);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(pflag, 0, sizeof(int32_t) * D, s) != hipSuccess) {
    mt_set_error("surface_distances: hipMemsetAsync failed");
    return MT_EHIP;
  }
  const int nblk = (int)L.nblk;                                 // <= 2^20
  hipLaunchKernelGGL(sd_border_kernel, dim3(nblk), dim3(MX_THREADS), 0, s, test, ref, m, g, connectivity, V, bm, cnt);
  MT_CHECK_LAUNCH("surface_distances (border)");
  hipLaunchKernelGGL(sd_scan_kernel, dim3(1), dim3(MX_THREADS), 0, s, cnt, nblk, off, tot);
  MT_CHECK_LAUNCH("surface_distances (scan)");
  hipLaunchKernelGGL(sd_compact_kernel, dim3(nblk), dim3(MX_THREADS), 0, s, bm, V, off, tot, capacity, q);
  MT_CHECK_LAUNCH("surface_distances (compact)");
  const long nrows = (long)D * H;
  const long cap_blocks = mt_stream_cap();
  long rgrid = (nrows + 3) / 4;
  if (rgrid > cap_blocks * 4) rgrid = cap_blocks * 4;
  hipLaunchKernelGGL(sd_rows_kernel, dim3((unsigned)rgrid), dim3(MX_THREADS), 0, s, bm, g, nrows, (short2*)g1, pflag, rflag);
  MT_CHECK_LAUNCH("surface_distances (rows)");
  long qgrid = (capacity + MX_THREADS - 1) / MX_THREADS;
  if (qgrid > cap_blocks * 4) qgrid = cap_blocks * 4;
  hipLaunchKernelGGL(sd_query_kernel, dim3((unsigned)qgrid), dim3(MX_THREADS), 0, s, q, tot, capacity, g1, pflag, rflag, g, out);
  MT_CHECK_LAUNCH("surface_distances (query)");
  long pgrid = L.maxchunks < cap_blocks ? L.maxchunks : cap_blocks;
  hipLaunchKernelGGL(sd_reduce1_kernel, dim3((unsigned)pgrid), dim3(MX_THREADS), 0, s, out, tot, capacity, L.maxchunks, partial);
  MT_CHECK_LAUNCH("surface_distances (reduce 1)");
  hipLaunchKernelGGL(sd_reduce2_kernel, dim3(1), dim3(MX_THREADS), 0, s, partial, tot, capacity, L.maxchunks, stats);
  MT_CHECK_LAUNCH("surface_distances (reduce 2)");
  return MT_OK;
}
