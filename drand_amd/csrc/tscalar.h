// The sealing scalar (include/blsverify.h "timelock"): 32 big-endian bytes reduced mod r and read as 64
// four-bit digits. One host/device form for every user -- the batch kernels (tseal.h, tsealr.h), the
// latency engine's item (wseal.h) and the host tools -- so that they agree by construction.
#pragma once
#include "bls_constants.h"
#include "fp.h"

namespace bls {

constexpr int TSEAL_WINDOWS = 64;  // four-bit windows of a 256-bit scalar
constexpr int TSEAL_ENTRIES = 15;  // the non-zero digits
constexpr int TSEAL_SCALAR_LEN = 32;

// 32 bytes big-endian -> k mod r as eight little-endian words; 2^256 < 3r, so at most two
// subtractions. Returns false for k == 0 (mod r).
DI bool tseal_scalar(const uint8_t* be32, uint32_t (&k)[8]) {
#pragma unroll
  for (int w = 0; w < 8; w++) {
    const uint8_t* p = be32 + 4 * (7 - w);
    k[w] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
  }
#pragma unroll 1
  for (int pass = 0; pass < 2; pass++) {
    uint32_t d[8];
    uint32_t borrow = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) {
      const uint64_t t = (uint64_t)k[w] - R_ORDER[w] - borrow;
      d[w] = (uint32_t)t;
      borrow = (uint32_t)(t >> 63);
    }
    if (!borrow) {
#pragma unroll
      for (int w = 0; w < 8; w++) k[w] = d[w];
    }
  }
  uint32_t any = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) any |= k[w];
  return any != 0;
}

DI int tseal_digit(const uint32_t (&k)[8], int w) { return (int)((k[w >> 3] >> ((w & 7) * 4)) & 15u); }

// entry (w, j), j = 1..15, of a table of 64 x 15 entries
DI int tseal_entry(int w, int j) { return w * TSEAL_ENTRIES + (j - 1); }

}  // namespace bls
