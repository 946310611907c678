// CRC-32 (IEEE, reflected) pieces that the DEFLATE encoder (deflate.hip) and the INFLATE decoder (inflate.hip) share: a piece of 16
// bytes is run through the bytewise table from a zero register and shifted past the pieces behind it by a multiplication mod P.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define DF_POLY 0xedb88320u

// product of two reflected 32-bit polynomials mod the CRC polynomial (bit 31 is x^0)
__device__ __forceinline__ uint32_t df_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 8
  for (int k = 0; k < 32; ++k) {
    p ^= b & (0u - ((a >> (31 - k)) & 1u));
    b = (b >> 1) ^ (DF_POLY & (0u - (b & 1u)));
  }
  return p;
}

// Thread t of 256 fills crctab[t] (the bytewise table) and pow128[t] = x^(128 t) mod P (what t later 16-byte pieces shift a
// piece's CRC by).  The caller synchronises.
__device__ __forceinline__ void df_crc_tables(uint32_t* crctab, uint32_t* pow128, int t) {
  uint32_t c = (uint32_t)t;
#pragma unroll
  for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (DF_POLY & (0u - (c & 1u)));
  crctab[t] = c;
  uint32_t sq = 1u << 30;                                            // x^1 -> x^128 by 7 squarings
#pragma unroll 1
  for (int k = 0; k < 7; ++k) sq = df_mulmod(sq, sq);
  uint32_t r = 1u << 31;                                             // x^0
#pragma unroll 1
  for (int e = t; e; e >>= 1) { if (e & 1) r = df_mulmod(r, sq); sq = df_mulmod(sq, sq); }
  pow128[t] = r;
}
