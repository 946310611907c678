// Index and pad arithmetic of the patch gather (loader.hip): output coordinate of a patch -> coordinate in its source, or "fill".
// This is np.pad's meaning for the box that is the intersection of patch and case (reference dataset_loading.py:338-372): outside
// the source `constant` fills, `edge` repeats the nearest voxel of the source, axis by axis.  Plain C++ that the device kernel and a
// host program compile alike (tests/test_device_loading_cpu.py builds it with the host compiler and its sanitizers).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MT_HD __host__ __device__
#else
#define MT_HD
#endif

#define MT_PATCH_FILL (-1)

// Coordinate i of a patch whose lower corner sits at lb (may be negative) in a source axis of n voxels -> source coordinate in
// [0, n), or MT_PATCH_FILL.  pad_mode: MT_PAD_CONSTANT (0) or MT_PAD_EDGE (1).
static inline MT_HD int mt_patch_axis(int i, int lb, int n, int pad_mode) {
  const int s = lb + i;
  if (s >= 0 && s < n) return s;
  if (pad_mode == 1) return s < 0 ? 0 : n - 1;
  return MT_PATCH_FILL;
}

// Linear index into the [sx, sy, sz] source of patch voxel (d, h, w), or MT_PATCH_FILL when any axis fills.
static inline MT_HD long mt_patch_source(const int shape[3], const int lb[3], int d, int h, int w, int pad_mode) {
  const int x = mt_patch_axis(d, lb[0], shape[0], pad_mode);
  const int y = mt_patch_axis(h, lb[1], shape[1], pad_mode);
  const int z = mt_patch_axis(w, lb[2], shape[2], pad_mode);
  if (x < 0 || y < 0 || z < 0) return MT_PATCH_FILL;
  return ((long)x * shape[1] + y) * shape[2] + z;
}
