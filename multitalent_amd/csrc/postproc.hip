// Connected-component post-processing on the device: "keep only the largest connected component" of
// postprocessing/connected_components.py:48-101 (scipy.ndimage.label with its default 3-D structure = 6-connectivity, :76,
// then the removal loop :85-100).  Union-find labelling in four launches:
//   1. cc_local_kernel   one 8x16x16 brick per 256-thread workgroup: union-find in LDS (atomicMin links the larger root under
//                        the smaller); a run along w starts out linked to its first voxel (a ballot, no atomics) and runs of
//                        neighbouring rows are united once per overlap.  labels[v] = global linear index of the brick-local
//                        root, sizes[brick-local root] = voxel count of the brick-local piece, every other sizes[] entry 0;
//   2. cc_merge_kernel   the low faces of every brick against the neighbouring brick: union in global memory (atomicMin), once
//                        per distinct pair of roots among neighbouring lanes;
//   3. cc_flatten_kernel labels[v] = final root = the smallest linear index of the component; roots are counted;
//   4. cc_count_kernel   every non-final brick-local root adds its piece count to its final root (one atomic per
//                        (brick, component) pair, not per voxel) and clears its own entry.
// cc_remove_kernel then zeroes, in place, the voxels of the components that are not kept.
//
// mt_fill_holes3d (scipy.ndimage.binary_fill_holes, default structure, for preprocessing/device_cropping.py) labels the BACKGROUND
// with launches 1 - 3 (no piece counts), then
//   fh_mark_kernel       every background voxel on one of the six faces of the volume stores -2 over its root's own label;
//   fh_fill_kernel       mask[v] = 1 where v is foreground or its component's root is unmarked (a cavity), else 0, and the
//                        bounding box and count of the result: wave shuffles, then one integer atomic per workgroup and value.
#include "stream_common.h"

#define CC_BD 8
#define CC_BH 16
#define CC_BW 16
#define CC_BV (CC_BD * CC_BH * CC_BW)   // 2048 voxels per brick, 8 per thread
#define CC_THREADS 256

// ---- LDS union-find (one workgroup) ----------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_lds_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int cc_lfind(int* par, int x) {
  int p;
  while ((p = cc_lds_load(par + x)) != x) x = p;
  return x;
}
// Links the larger root under the smaller.  If the atomicMin finds `a` already linked (old != a), par[a] now holds min(old, b)
// and the pair (old, b) is united in the next turn: no equivalence is lost, and a parent pointer only ever decreases.
__device__ __forceinline__ void cc_lunion(int* par, int a, int b) {
  while (true) {
    a = cc_lfind(par, a);
    b = cc_lfind(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + a, b);
    if (old == a) return;
    a = old;
  }
}

// ---- global union-find (merge launch) -------------------------------------------------------------------------------------
// Parent pointers are read with agent-scope atomic loads: another workgroup's link may have been made on another XCD within
// this launch, and a plain load could return a line this CU's L1 or this XCD's L2 still holds.
__device__ __forceinline__ int cc_gload(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_gfind(int* L, int x) {
  int p;
  while ((p = cc_gload(L + x)) != x) x = p;
  return x;
}
__device__ __forceinline__ void cc_gunion(int* L, int a, int b) {
  while (true) {
    a = cc_gfind(L, a);
    b = cc_gfind(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
}

struct CCGeom { int D, H, W, nbh, nbw; };

__device__ __forceinline__ void cc_brick_origin(const CCGeom& g, int b, int& d0, int& h0, int& w0) {
  const int bw = b % g.nbw, bh = (b / g.nbw) % g.nbh, bd = b / (g.nbw * g.nbh);
  d0 = bd * CC_BD; h0 = bh * CC_BH; w0 = bw * CC_BW;
}

// COUNT = false (mt_fill_holes3d): no piece counts, S is not touched and may be NULL.
template <bool COUNT>
__global__ __launch_bounds__(CC_THREADS) void cc_local_kernel(const uint8_t* __restrict__ seg, const MtMember m, const CCGeom g,
                                                              int nb, int32_t* __restrict__ L, int32_t* __restrict__ S,
                                                              int32_t* __restrict__ stats) {
  __shared__ int par[CC_BV];
  __shared__ int cnt[COUNT ? CC_BV : 1];
  if (blockIdx.x == 0 && threadIdx.x < 2) stats[threadIdx.x] = 0;
  const int t = threadIdx.x, lh = t >> 4, lw = t & 15;
  for (int b = blockIdx.x; b < nb; b += gridDim.x) {
    int d0, h0, w0;
    cc_brick_origin(g, b, d0, h0, w0);
    const int h = h0 + lh, w = w0 + lw;
    const bool hw_in = h < g.H && w < g.W;
    unsigned fg = 0;                                 // bit ld: this thread's voxel of slice ld is in the mask
    unsigned fgl = 0;                                // bit ld: so is its neighbour at w - 1
    unsigned rs = 0;                                 // bit ld: it is the first voxel of its run along w
    // Runs along w need no atomics: a row is 16 lanes of one wave, so a ballot gives every voxel the start of its run, and
    // that is its parent from the beginning.
#pragma unroll
    for (int ld = 0; ld < CC_BD; ++ld) {
      const int d = d0 + ld, i = ld * (CC_BH * CC_BW) + t;
      bool f = false;
      if (hw_in && d < g.D) f = mt_member(m, seg[((size_t)d * g.H + h) * g.W + w]);
      const unsigned row = (unsigned)(__ballot(f) >> (t & 48)) & 0xffffu;
      const unsigned below = ~row & ((1u << lw) - 1u);               // voxels before lw that are not in the mask
      const int start = below ? 32 - __clz((int)below) : 0;
      fg |= (unsigned)f << ld;
      fgl |= (lw > 0 ? (row >> (lw - 1)) & 1u : 0u) << ld;
      rs |= (unsigned)(start == lw) << ld;
      par[i] = f ? i - (lw - start) : -1;
      if (COUNT) cnt[i] = 0;
    }
    __syncthreads();
    // Runs of neighbouring rows (h - 1, then d - 1) are united once per overlap, at its first voxel: where this run starts, or
    // where the other one does (its voxel at w - 1 is outside the mask).  A neighbour's entry is >= 0 exactly when it is in the
    // mask, whatever links other threads are making meanwhile.
#pragma unroll
    for (int ld = 0; ld < CC_BD; ++ld) {
      if (!((fg >> ld) & 1)) continue;
      const int i = ld * (CC_BH * CC_BW) + t;
      const bool first = (rs >> ld) & 1;
      if (lh > 0 && cc_lds_load(par + i - CC_BW) >= 0 && (first || cc_lds_load(par + i - CC_BW - 1) < 0)) cc_lunion(par, i, i - CC_BW);
      if (ld > 0 && ((fg >> (ld - 1)) & 1) && (first || !((fgl >> (ld - 1)) & 1))) cc_lunion(par, i, i - CC_BH * CC_BW);
    }
    __syncthreads();
    int root[CC_BD];
#pragma unroll
    for (int ld = 0; ld < CC_BD; ++ld) {
      const int i = ld * (CC_BH * CC_BW) + t;
      const bool f = (fg >> ld) & 1;
      root[ld] = f ? cc_lfind(par, i) : -1;
      if (!COUNT) continue;
      // per-wave aggregation of the piece counts: one LDS atomic per distinct root of the wave, not one per voxel
      uint64_t active = __ballot(f);
      while (active) {
        const int leader = __ffsll((unsigned long long)active) - 1;
        const int rl = __shfl(root[ld], leader, 64);
        const uint64_t same = __ballot(f && root[ld] == rl);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(cnt + rl, __popcll(same));
        active &= ~same;
      }
    }
    if (COUNT) __syncthreads();
    if (hw_in) {
#pragma unroll
      for (int ld = 0; ld < CC_BD; ++ld) {
        const int d = d0 + ld;
        if (d >= g.D) break;
        const int i = ld * (CC_BH * CC_BW) + t;
        const size_t v = ((size_t)d * g.H + h) * g.W + w;
        int lab = -1;
        if (root[ld] >= 0) {
          const int r = root[ld];
          // local index order (ld, lh, lw) is the linear order inside the brick: the local root is the piece's smallest index
          lab = (int)(((size_t)(d0 + (r >> 8)) * g.H + (h0 + ((r >> 4) & 15))) * g.W + (w0 + (r & 15)));
        }
        L[v] = lab;
        if (COUNT) S[v] = (root[ld] == i) ? cnt[i] : 0;
      }
    }
    __syncthreads();                                 // LDS is reused by the next brick
  }
}

// Faces d = d0, h = h0, w = w0 of every brick against the voxel before it.  Threads 0..255: the D face (one (h, w) each);
// threads 0..127 also the H face (ld, lw), threads 128..255 the W face (ld, lh).  Where a component crosses a face with many
// voxels, most pairs of a wave name the same two brick-local roots: a pair is united by the lowest lane that holds it (lane - 1
// and lane - 16 are the face's two neighbours), the others skip it.
__device__ __forceinline__ void cc_merge_pairs(int32_t* L, int a, int b) {
  const int lane = threadIdx.x & 63;
  const int pa = __shfl_up(a, 1, 64), pb = __shfl_up(b, 1, 64), qa = __shfl_up(a, 16, 64), qb = __shfl_up(b, 16, 64);
  const bool dup = (lane >= 1 && pa == a && pb == b) || (lane >= 16 && qa == a && qb == b);
  if (a >= 0 && b >= 0 && !dup) cc_gunion(L, a, b);
}

__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const CCGeom g, int nb, int32_t* __restrict__ L) {
  const int t = threadIdx.x;
  const size_t HW = (size_t)g.H * g.W;
  for (int blk = blockIdx.x; blk < nb; blk += gridDim.x) {
    int d0, h0, w0;
    cc_brick_origin(g, blk, d0, h0, w0);
    int a = -1, b = -1;                              // >= 0 <=> in the mask: fixed since the previous launch
    if (d0 > 0) {
      const int h = h0 + (t >> 4), w = w0 + (t & 15);
      if (h < g.H && w < g.W) {
        const size_t v = ((size_t)d0 * g.H + h) * g.W + w;
        a = L[v]; b = L[v - HW];
      }
    }
    cc_merge_pairs(L, a, b);
    a = -1; b = -1;
    if (t < 128) {
      const int d = d0 + (t >> 4), w = w0 + (t & 15);
      if (h0 > 0 && d < g.D && w < g.W) {
        const size_t v = ((size_t)d * g.H + h0) * g.W + w;
        a = L[v]; b = L[v - g.W];
      }
    } else {
      const int d = d0 + ((t - 128) >> 4), h = h0 + ((t - 128) & 15);
      if (w0 > 0 && d < g.D && h < g.H) {
        const size_t v = ((size_t)d * g.H + h) * g.W + w0;
        a = L[v]; b = L[v - 1];
      }
    }
    cc_merge_pairs(L, a, b);
  }
}

__device__ __forceinline__ int cc_block_sum(int v, int* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ int cc_block_max(int v, int* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return max(max(red[0], red[1]), max(red[2], red[3]));
}

// labels[v] = root.  Plain loads suffice here: the links are final since the merge launch, and a value another thread of
// THIS launch stores (a final root) is an ancestor of what was there before, so any mix of old and new values walks to the
// same root.
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int32_t* __restrict__ L, long V, int32_t* __restrict__ stats) {
  __shared__ int red[4];
  int nroots = 0;
  for (long v = (long)blockIdx.x * CC_THREADS + threadIdx.x; v < V; v += (long)gridDim.x * CC_THREADS) {
    int x = L[v];
    if (x < 0) continue;
    int p;
    while ((p = L[x]) != x) x = p;
    L[v] = x;
    nroots += (x == (int)v);
  }
  const int n = cc_block_sum(nroots, red);
  if (threadIdx.x == 0 && n) atomicAdd(stats, n);
}

// sizes[root] += piece count of every brick-local root that is not a final root; sizes[v] of such a v is read and cleared by
// its own thread only (nothing adds to an entry that is not a final root).  The running totals returned by the atomics bound
// each component's final count from below and reach it at the last add: their maximum is the largest component.
__global__ __launch_bounds__(CC_THREADS) void cc_count_kernel(const int32_t* __restrict__ L, int32_t* __restrict__ S, long V,
                                                              int32_t* __restrict__ stats) {
  __shared__ int red[4];
  int mx = 0;
  for (long v = (long)blockIdx.x * CC_THREADS + threadIdx.x; v < V; v += (long)gridDim.x * CC_THREADS) {
    const int c = S[v];
    if (c <= 0) continue;
    const int r = L[v];
    if (r == (int)v) { mx = max(mx, c); continue; }
    mx = max(mx, atomicAdd(S + r, c) + c);
    S[v] = 0;
  }
  const int m = cc_block_max(mx, red);
  if (threadIdx.x == 0 && m) atomicMax(stats + 1, m);
}

// Removal rule of connected_components.py:92-99: a component is removed when its size differs from the largest size (every
// component tied for the largest is kept) and, with a minimum given, its size is below it.  Sizes are (double)count * vpv, the
// same IEEE product as the reference's np.int64 * float.
__global__ __launch_bounds__(CC_THREADS) void cc_remove_kernel(uint8_t* __restrict__ seg, const int32_t* __restrict__ L,
                                                               const int32_t* __restrict__ S, long V,
                                                               const int32_t* __restrict__ stats, double vpv, double min_size,
                                                               int use_min, int32_t* __restrict__ removed) {
  __shared__ int red[4];
  const double max_size = (double)stats[1] * vpv;
  int mx = 0;
  for (long v = (long)blockIdx.x * CC_THREADS + threadIdx.x; v < V; v += (long)gridDim.x * CC_THREADS) {
    const int r = L[v];
    if (r < 0) continue;
    const int c = S[r];
    const double size = (double)c * vpv;
    if (size != max_size && (!use_min || size < min_size)) {
      seg[v] = 0;
      mx = max(mx, c);
    }
  }
  const int m = cc_block_max(mx, red);
  if (threadIdx.x == 0 && m) atomicMax(removed, m);
}

// The labelling launches shared by mt_cc_label3d and mt_fill_holes3d: local, merge, flatten (labels[v] = root, stats[0] = number
// of components, stats[1] = 0).  COUNT: the local kernel also writes the brick-local piece counts into sizes.
template <bool COUNT>
static int cc_label_launches(const uint8_t* seg, int D, int H, int W, const MtMember& m, int32_t* labels, int32_t* sizes,
                             int32_t* stats, hipStream_t s, const char* who) {
  const long V = (long)D * H * W;
  CCGeom g;
  g.D = D; g.H = H; g.W = W; g.nbh = mt_cdiv(H, CC_BH); g.nbw = mt_cdiv(W, CC_BW);
  const long nb = (long)mt_cdiv(D, CC_BD) * g.nbh * g.nbw;     // <= V: fits in int
  const int grid = nb < (1L << 20) ? (int)nb : (1 << 20);          // bricks beyond the grid: block-stride loop
  hipLaunchKernelGGL(cc_local_kernel<COUNT>, dim3(grid), dim3(CC_THREADS), 0, s, seg, m, g, (int)nb, labels, sizes, stats);
  MT_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(cc_merge_kernel, dim3(grid), dim3(CC_THREADS), 0, s, g, (int)nb, labels);
  MT_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(mt_stream_blocks(V, CC_THREADS)), dim3(CC_THREADS), 0, s, labels, V, stats);
  MT_CHECK_LAUNCH(who);
  return MT_OK;
}

extern "C" int mt_cc_label3d(const uint8_t* seg, int D, int H, int W, const uint8_t* member, int32_t* labels, int32_t* sizes,
                             int32_t* stats, mt_stream_t stream) {
  MT_REQUIRE(seg && member && labels && sizes && stats, "cc_label3d: null pointer");
  MT_REQUIRE(D > 0 && H > 0 && W > 0, "cc_label3d: bad shape %d x %d x %d", D, H, W);
  const long V = (long)D * H * W;
  MT_REQUIRE(V <= (long)INT32_MAX, "cc_label3d: %ld voxels exceed the int32 index range", V);
  const MtMember m = mt_member_from_bytes(member);
  hipStream_t s = (hipStream_t)stream;
  const int rc = cc_label_launches<true>(seg, D, H, W, m, labels, sizes, stats, s, "cc_label3d (labelling)");
  if (rc != MT_OK) return rc;
  hipLaunchKernelGGL(cc_count_kernel, dim3(mt_stream_blocks(V, CC_THREADS)), dim3(CC_THREADS), 0, s, labels, sizes, V, stats);
  MT_CHECK_LAUNCH("cc_label3d (count)");
  return MT_OK;
}

extern "C" int mt_cc_remove(uint8_t* seg, int D, int H, int W, const int32_t* labels, const int32_t* sizes, const int32_t* stats,
                            double volume_per_voxel, int use_min_size, double min_size, int32_t* removed, mt_stream_t stream) {
  MT_REQUIRE(seg && labels && sizes && stats && removed, "cc_remove: null pointer");
  MT_REQUIRE(D > 0 && H > 0 && W > 0, "cc_remove: bad shape %d x %d x %d", D, H, W);
  const long V = (long)D * H * W;
  MT_REQUIRE(V <= (long)INT32_MAX, "cc_remove: %ld voxels exceed the int32 index range", V);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(removed, 0, sizeof(int32_t), s) != hipSuccess) {
    mt_set_error("cc_remove: hipMemsetAsync failed");
    return MT_EHIP;
  }
  hipLaunchKernelGGL(cc_remove_kernel, dim3(mt_stream_blocks(V, CC_THREADS)), dim3(CC_THREADS), 0, s, seg, labels, sizes, V, stats,
                     volume_per_voxel, min_size, use_min_size, removed);
  MT_CHECK_LAUNCH("cc_remove");
  return MT_OK;
}

// ---- binary_fill_holes ------------------------------------------------------------------------------------------------------
#define FH_OUTSIDE (-2)

// One thread per face voxel (edges and corners are visited more than once).  Every store of this launch writes the same value
// and nothing in it depends on another thread's store: a label read here is -1 (foreground), a root, or FH_OUTSIDE where the
// voxel is itself a root that was marked a moment ago.  Block 0 also resets the box for the fill launch.
__global__ __launch_bounds__(CC_THREADS) void fh_mark_kernel(int32_t* __restrict__ L, int D, int H, int W, int32_t* __restrict__ bbox) {
  if (blockIdx.x == 0 && threadIdx.x < 7) bbox[threadIdx.x] = (threadIdx.x < 6 && !(threadIdx.x & 1)) ? INT32_MAX : 0;
  const long nD = (long)H * W, nH = (long)D * W, nW = (long)D * H, total = 2 * (nD + nH + nW);
  for (long i = (long)blockIdx.x * CC_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * CC_THREADS) {
    long v, r = i;
    if (r < 2 * nD) {
      v = (r < nD ? 0 : (long)(D - 1) * nD) + r % nD;
    } else if ((r -= 2 * nD) < 2 * nH) {
      const long q = r % nH;
      v = ((q / W) * H + (r < nH ? 0 : H - 1)) * W + q % W;
    } else {
      r -= 2 * nH;
      v = (r % nW) * W + (r < nW ? 0 : W - 1);
    }
    const int x = L[v];
    if (x >= 0) L[x] = FH_OUTSIDE;
  }
}

// 16 consecutive voxels per thread and step: four 16-byte loads of labels, one 16-byte store of mask bytes (bytewise when the
// mask is not 16-byte aligned, and in the last, partial chunk).  The mask itself is not read: labels[v] == -1 is "foreground".
__global__ __launch_bounds__(CC_THREADS) void fh_fill_kernel(uint8_t* __restrict__ mask, const int32_t* __restrict__ L, int H, int W,
                                                             long V, int vec, int32_t* __restrict__ bbox) {
  __shared__ int red[7][CC_THREADS / 64];
  int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {0, 0, 0}, count = 0;
  int last = -1, last_set = 1;                     // the previous label looked up and its answer
  const long nchunk = (V + 15) / 16;
  for (long c = (long)blockIdx.x * CC_THREADS + threadIdx.x; c < nchunk; c += (long)gridDim.x * CC_THREADS) {
    const long base = c * 16;
    const int n = V - base < 16 ? (int)(V - base) : 16;
    int x[16];
    if (n == 16) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int4 t = ((const int4*)(L + base))[k];
        x[4 * k] = t.x; x[4 * k + 1] = t.y; x[4 * k + 2] = t.z; x[4 * k + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) x[k] = k < n ? L[base + k] : FH_OUTSIDE;
    }
    int w = (int)(base % W), h = (int)((base / W) % H), d = (int)(base / ((long)W * H));
    uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (x[k] != last) {
        last = x[k];
        last_set = last == -1 || (last != FH_OUTSIDE && L[last] != FH_OUTSIDE);
      }
      if (last_set && k < n) {
        out[k >> 2] |= 1u << (8 * (k & 3));
        ++count;
        lo[0] = min(lo[0], d); hi[0] = max(hi[0], d + 1);
        lo[1] = min(lo[1], h); hi[1] = max(hi[1], h + 1);
        lo[2] = min(lo[2], w); hi[2] = max(hi[2], w + 1);
      }
      if (++w == W) { w = 0; if (++h == H) { h = 0; ++d; } }
    }
    if (n == 16 && vec) {
      uint4 t; t.x = out[0]; t.y = out[1]; t.z = out[2]; t.w = out[3];
      *(uint4*)(mask + base) = t;
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) if (k < n) mask[base + k] = (uint8_t)((out[k >> 2] >> (8 * (k & 3))) & 1u);
    }
  }
  int val[7] = {lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], count};
#pragma unroll
  for (int j = 0; j < 7; ++j) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(val[j], off, 64);
      val[j] = j == 6 ? val[j] + o : (j & 1) ? max(val[j], o) : min(val[j], o);
    }
    if ((threadIdx.x & 63) == 0) red[j][threadIdx.x >> 6] = val[j];
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int j = threadIdx.x;
    int v = red[j][0];
    for (int k = 1; k < CC_THREADS / 64; ++k) v = j == 6 ? v + red[j][k] : (j & 1) ? max(v, red[j][k]) : min(v, red[j][k]);
    int total = 0;
    for (int k = 0; k < CC_THREADS / 64; ++k) total += red[6][k];
    if (total) {
      if (j == 6) atomicAdd(bbox + 6, v);
      else if (j & 1) atomicMax(bbox + j, v);
      else atomicMin(bbox + j, v);
    }
  }
}

static size_t fh_label_bytes(long V) { return ((size_t)V * sizeof(int32_t) + 15) & ~(size_t)15; }

extern "C" size_t mt_fill_holes3d_workspace(int D, int H, int W) {
  if (D <= 0 || H <= 0 || W <= 0) return 0;
  return fh_label_bytes((long)D * H * W) + 16;                       // labels, then the two labelling statistics
}

extern "C" int mt_fill_holes3d(uint8_t* mask, int D, int H, int W, int32_t* bbox, void* ws, size_t ws_bytes, mt_stream_t stream) {
  MT_REQUIRE(mask && bbox && ws, "fill_holes3d: null pointer");
  MT_REQUIRE(D > 0 && H > 0 && W > 0, "fill_holes3d: bad shape %d x %d x %d", D, H, W);
  const long V = (long)D * H * W;
  MT_REQUIRE(V <= (long)INT32_MAX, "fill_holes3d: %ld voxels exceed the int32 index range", V);
  MT_REQUIRE(((uintptr_t)ws & 15) == 0, "fill_holes3d: the workspace must be 16-byte aligned");
  MT_REQUIRE_WORKSPACE("fill_holes3d", ws_bytes, mt_fill_holes3d_workspace(D, H, W));
  int32_t* labels = (int32_t*)ws;
  int32_t* stats = (int32_t*)((char*)ws + fh_label_bytes(V));
  const uint8_t background[256] = {1};                               // mask == 0 only
  const MtMember m = mt_member_from_bytes(background);
  hipStream_t s = (hipStream_t)stream;
  const int rc = cc_label_launches<false>(mask, D, H, W, m, labels, nullptr, stats, s, "fill_holes3d (labelling)");
  if (rc != MT_OK) return rc;
  const long faces = 2 * ((long)H * W + (long)D * W + (long)D * H);
  hipLaunchKernelGGL(fh_mark_kernel, dim3(mt_stream_blocks(faces, CC_THREADS)), dim3(CC_THREADS), 0, s, labels, D, H, W, bbox);
  MT_CHECK_LAUNCH("fill_holes3d (mark)");
  hipLaunchKernelGGL(fh_fill_kernel, dim3(mt_stream_blocks((V + 15) / 16, CC_THREADS)), dim3(CC_THREADS), 0, s, mask, labels, H, W, V,
                     (int)(((uintptr_t)mask & 15) == 0), bbox);
  MT_CHECK_LAUNCH("fill_holes3d (fill)");
  return MT_OK;
}
