// Classification of one voxel of a stored label volume for mt_label_convert (analyze.hip): "which table slot, zero, or unexpected".
// This is the per-voxel meaning of the reference's copy_and_convert_segmentation (dataset_conversion/Task100_MultiTalent.py:229-275)
// on the float64 array that get_fdata returns: np.unique, `uniques > 1e-20`, `u not in labels`, `seg == label`.
//   not (v > 1e-20)            zero: the output is 0 and the voxel is never an error (zero, negatives, 1e-20 itself, NaN);
//   an integer 1..1022         that slot of the table (whether the table lists it is the caller's question);
//   anything else above 1e-20  unexpected (a fraction, +inf, an integer beyond the table).
// Every stored type widens to double exactly (int64 / uint64 files are cast on the host, as get_fdata does), so the float32 and
// integer forms below are the double form applied to the widened value.  Plain C++ that the device kernel and a host program
// compile alike (tests/test_label_convert_cpu.py builds it as a stand-alone program with the address and undefined-behaviour
// sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MT_HD __host__ __device__
#else
#define MT_HD
#endif

#define MT_LABEL_ZERO (-1)
#define MT_LABEL_UNEXPECTED (-2)
#ifndef MT_LABEL_SLOTS
#define MT_LABEL_SLOTS 1023               /* labels 0..1022, the range of mt_label_presence (include/mtseg.h has the same line) */
#endif

static inline MT_HD int mt_label_slot(double v) {
  if (!(v > 1e-20)) return MT_LABEL_ZERO;                         // NaN fails the comparison
  if (!(v <= (double)(MT_LABEL_SLOTS - 1))) return MT_LABEL_UNEXPECTED;   // +inf and everything beyond the table
  const int l = (int)v;                                           // 1e-20 < v <= 1022: the conversion is defined
  return (double)l == v ? (l > 0 ? l : MT_LABEL_UNEXPECTED) : MT_LABEL_UNEXPECTED;   // 0 < v < 1 truncates to 0: a fraction
}
static inline MT_HD int mt_label_slot(float v) { return mt_label_slot((double)v); }
static inline MT_HD int mt_label_slot(int32_t v) { return v <= 0 ? MT_LABEL_ZERO : v <= MT_LABEL_SLOTS - 1 ? (int)v : MT_LABEL_UNEXPECTED; }
static inline MT_HD int mt_label_slot(uint32_t v) { return v == 0 ? MT_LABEL_ZERO : v <= (uint32_t)(MT_LABEL_SLOTS - 1) ? (int)v : MT_LABEL_UNEXPECTED; }
static inline MT_HD int mt_label_slot(int16_t v) { return mt_label_slot((int32_t)v); }
static inline MT_HD int mt_label_slot(uint16_t v) { return mt_label_slot((uint32_t)v); }
static inline MT_HD int mt_label_slot(int8_t v) { return mt_label_slot((int32_t)v); }
static inline MT_HD int mt_label_slot(uint8_t v) { return mt_label_slot((uint32_t)v); }

// Order-preserving key of a value above 1e-20 (+inf included): the bits of the positive double it widens to.  A 64-bit integer
// minimum over the keys of the unexpected voxels is the smallest unexpected value, whatever the order the voxels are met in.
#define MT_LABEL_KEY_NONE 0xffffffffffffffffull
template <typename T> static inline MT_HD uint64_t mt_label_key(T v) { return __builtin_bit_cast(uint64_t, (double)v); }
