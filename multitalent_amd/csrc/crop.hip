// Cropping a case to its non-zero region on the device (preprocessing/cropping.py of the reference, :23-116).
//   mt_nonzero_mask   mask[v] = any channel != 0 at v, decided on the bit pattern (numpy's rule whatever the denormal mode);
//   mt_crop_nonzero   one pass over the crop box: the data channels bit for bit, and the segmentation with `nonzero_label`
//                     outside the mask.
// The hole filling between the two is mt_fill_holes3d (postproc.hip: it shares the union-find labelling).
#include "stream_common.h"

#define CR_THREADS 256

__device__ __forceinline__ uint32_t cr_nz(uint32_t bits) { return (bits & 0x7fffffffu) != 0 ? 1u : 0u; }

// 16 bytes that are only dword aligned: a channel starts at data + c * V, so at most one channel in four shares the
// alignment of the mask.  gfx950 serves a dword-aligned global_load_dwordx4 (mt_probe_device checks the buffer form).
struct __attribute__((packed, aligned(4))) cr_u4 { uint32_t x, y, z, w; };

// Voxels [0, head) and [head + 4 nquad, V) bytewise; between them one 16-byte load per lane and channel and one dword store of
// four mask bytes (mask + head is dword aligned), two quads per lane and step.
__global__ __launch_bounds__(CR_THREADS) void nz_mask_kernel(const uint32_t* __restrict__ data, int C, long V, long head, long nquad,
                                                             uint8_t* __restrict__ mask) {
  const long gtid = (long)blockIdx.x * CR_THREADS + threadIdx.x, gstride = (long)gridDim.x * CR_THREADS;
  uint32_t* mq = (uint32_t*)(mask + head);
  for (long q = gtid; q < nquad; q += 2 * gstride) {
    const long q1 = q + gstride;
    const bool two = q1 < nquad;
    uint32_t m0 = 0, m1 = 0;
    for (int c = 0; c < C; ++c) {
      const uint32_t* p = data + (size_t)c * V + head;
      const cr_u4 a = *(const cr_u4*)(p + 4 * q);
      cr_u4 b = {0, 0, 0, 0};
      if (two) b = *(const cr_u4*)(p + 4 * q1);
      m0 |= cr_nz(a.x) | cr_nz(a.y) << 8 | cr_nz(a.z) << 16 | cr_nz(a.w) << 24;
      m1 |= cr_nz(b.x) | cr_nz(b.y) << 8 | cr_nz(b.z) << 16 | cr_nz(b.w) << 24;
    }
    mq[q] = m0;
    if (two) mq[q1] = m1;
  }
  const long tail0 = head + 4 * nquad, nscalar = head + (V - tail0);
  for (long i = gtid; i < nscalar; i += gstride) {
    const long v = i < head ? i : tail0 + (i - head);
    uint32_t m = 0;
    for (int c = 0; c < C; ++c) m |= cr_nz(data[(size_t)c * V + v]);
    mask[v] = (uint8_t)m;
  }
}

extern "C" int mt_nonzero_mask(const float* data, int C, long V, uint8_t* mask, mt_stream_t stream) {
  MT_REQUIRE(data && mask, "nonzero_mask: null pointer");
  MT_REQUIRE(C >= 1 && V > 0, "nonzero_mask: bad shape %d x %ld", C, V);
  MT_REQUIRE(((uintptr_t)data & 3) == 0, "nonzero_mask: data must be 4-byte aligned");
  long head = (4 - (long)((uintptr_t)mask & 3)) & 3;
  if (head > V) head = V;
  const long nquad = (V - head) / 4;
  const long items = nquad ? (nquad + 1) / 2 : V;
  hipLaunchKernelGGL(nz_mask_kernel, dim3(mt_stream_blocks(items, CR_THREADS)), dim3(CR_THREADS), 0, (hipStream_t)stream, (const uint32_t*)data, C, V,
                     head, nquad, mask);
  MT_CHECK_LAUNCH("nonzero_mask");
  return MT_OK;
}

struct CropGeom { int H, W, bd, bh, bw, lo_d, lo_h, lo_w; };

// One thread per voxel of the box (consecutive lanes along w).  SEG: 0 = no seg_in, int8 seg_out[0]; 1 = float32 seg_in / seg_out
// with CS channels.  Everything moves as uint32: NaN payloads survive, and `seg == 0` is the bit test of cr_nz.
template <int SEG>
__global__ __launch_bounds__(CR_THREADS) void crop_kernel(const uint32_t* __restrict__ data, int C, size_t V, const uint8_t* __restrict__ mask,
                                                          const CropGeom g, uint32_t* __restrict__ out, const uint32_t* __restrict__ seg_in,
                                                          int CS, void* __restrict__ seg_out, uint32_t label_bits, int label_i8) {
  const uint32_t Vo = (uint32_t)g.bd * g.bh * g.bw, bhw = (uint32_t)g.bh * g.bw;          // V <= INT32_MAX: 32-bit divisions
  for (uint32_t o = blockIdx.x * CR_THREADS + threadIdx.x; o < Vo; o += gridDim.x * CR_THREADS) {
    const uint32_t d = o / bhw, r = o - d * bhw, h = r / g.bw, w = r - h * g.bw;
    const size_t v = ((size_t)(g.lo_d + d) * g.H + (g.lo_h + h)) * g.W + (g.lo_w + w);
    for (int c = 0; c < C; ++c) out[(size_t)c * Vo + o] = data[(size_t)c * V + v];
    const bool in = mask[v] != 0;
    if (SEG == 0) {
      ((int8_t*)seg_out)[o] = in ? (int8_t)0 : (int8_t)label_i8;
    } else {
      for (int c = 0; c < CS; ++c) {
        const uint32_t s = seg_in[(size_t)c * V + v];
        ((uint32_t*)seg_out)[(size_t)c * Vo + o] = (!cr_nz(s) && !in) ? label_bits : s;
      }
    }
  }
}

extern "C" int mt_crop_nonzero(const float* data, int C, int D, int H, int W, const uint8_t* mask, const int32_t* box, float* out,
                               const float* seg_in, int CS, void* seg_out, float nonzero_label, mt_stream_t stream) {
  MT_REQUIRE(data && mask && box && out && seg_out, "crop_nonzero: null pointer");
  MT_REQUIRE(C >= 1 && D > 0 && H > 0 && W > 0, "crop_nonzero: bad shape %d x %d x %d x %d", C, D, H, W);
  MT_REQUIRE((long)D * H * W <= (long)INT32_MAX, "crop_nonzero: %ld voxels exceed the int32 index range", (long)D * H * W);
  MT_REQUIRE(box[0] >= 0 && box[0] < box[1] && box[1] <= D && box[2] >= 0 && box[2] < box[3] && box[3] <= H && box[4] >= 0 &&
             box[4] < box[5] && box[5] <= W, "crop_nonzero: box [%d, %d) x [%d, %d) x [%d, %d) outside %d x %d x %d", box[0], box[1],
             box[2], box[3], box[4], box[5], D, H, W);
  MT_REQUIRE(!seg_in || CS >= 1, "crop_nonzero: %d segmentation channels", CS);
  CropGeom g;
  g.H = H; g.W = W; g.bd = box[1] - box[0]; g.bh = box[3] - box[2]; g.bw = box[5] - box[4];
  g.lo_d = box[0]; g.lo_h = box[2]; g.lo_w = box[4];
  const size_t V = (size_t)D * H * W;
  const long Vo = (long)g.bd * g.bh * g.bw;
  const uint32_t bits = __builtin_bit_cast(uint32_t, nonzero_label);
  hipStream_t s = (hipStream_t)stream;
  if (seg_in) {
    hipLaunchKernelGGL(crop_kernel<1>, dim3(mt_stream_blocks(Vo, CR_THREADS)), dim3(CR_THREADS), 0, s, (const uint32_t*)data, C, V, mask, g,
                       (uint32_t*)out, (const uint32_t*)seg_in, CS, seg_out, bits, 0);
  } else {
    MT_REQUIRE(nonzero_label >= -128.f && nonzero_label <= 127.f && nonzero_label == (float)(int)nonzero_label,
               "crop_nonzero: nonzero_label %g is not an int8 value", (double)nonzero_label);
    hipLaunchKernelGGL(crop_kernel<0>, dim3(mt_stream_blocks(Vo, CR_THREADS)), dim3(CR_THREADS), 0, s, (const uint32_t*)data, C, V, mask, g,
                       (uint32_t*)out, (const uint32_t*)nullptr, 0, seg_out, bits, (int)nonzero_label);
  }
  MT_CHECK_LAUNCH("crop_nonzero");
  return MT_OK;
}
