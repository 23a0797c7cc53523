// Timelock encrypt / decrypt, the fused tail (include/blsverify.h "timelock in one call"): the key stream of
// BLSV_KDF_SHA256_CTR over an item's Gt value and the XOR with its message bytes, one lane per item, so that
// the 576 encoded bytes never leave the lane.
//   key stream = SHA-256(gt576 || BE32(0)) || SHA-256(gt576 || BE32(1)) || ...   truncated to mlen bytes
// gt576 is tlock.h's encoding: twelve canonical Fp values, 48 bytes big-endian each. A coefficient's twelve
// big-endian words are SHA-256's message words as they stand, four coefficients are three 64-byte blocks
// and the nine blocks of the twelve do not depend on the counter: their midstate is computed once, and
// every 32 bytes of key stream cost one more compression of the block {j, 0x80 pad, 0 x 13, 4640 bits}.
// 9 + ceil(mlen / 32) compressions per item.
// The shared host/device forms below are what tools/opcount tmask runs; k_tmask.hip holds the kernel.
#pragma once
#include "hash.h"
#include "soa.h"

namespace bls {

constexpr int TMASK_GT_LEN = 576;
constexpr int TMASK_MSG_MAX = 256;
constexpr uint32_t TMASK_BITS = 8 * (TMASK_GT_LEN + 4);  // the hashed length: the encoding and the counter

// blk[DST .. DST + N) = the big-endian words SRC .. SRC + N of v (word 0 holds the highest limb)
template <int DST, int SRC, int N>
DI void tmask_words(uint32_t (&blk)[16], const fp& v) {
#pragma unroll
  for (int w = 0; w < N; w++) blk[DST + w] = v.l[11 - SRC - w];
}

// coef(k): coefficient k of the encoding (0 = c1.c2.c1 ... 11 = c0.c0.c0), canonical, limb 11 the highest
template <typename Coef>
DI void tmask_midstate(uint32_t (&st)[8], Coef coef) {
  sha256_init(st);
#pragma unroll 1
  for (int g = 0; g < 3; g++) {  // four coefficients = 48 words = three blocks: 12 + 4, 8 + 8, 4 + 12
    uint32_t blk[16];
    fp a = coef(4 * g), b = coef(4 * g + 1);
    tmask_words<0, 0, 12>(blk, a);
    tmask_words<12, 0, 4>(blk, b);
    sha256_compress_batch(st, blk);
    a = coef(4 * g + 2);
    tmask_words<0, 4, 8>(blk, b);
    tmask_words<8, 0, 8>(blk, a);
    sha256_compress_batch(st, blk);
    b = coef(4 * g + 3);
    tmask_words<0, 8, 4>(blk, a);
    tmask_words<4, 0, 12>(blk, b);
    sha256_compress_batch(st, blk);
  }
}

// the captured Fp12 of item i (SoA of stride n, Montgomery form): coefficient k is slot 11 - k
DI fp tmask_coef_soa(const uint32_t* E, size_t n, size_t i, int k) { return fp_from_mont(ld_fp_v(E, n, i, 11 - k)); }
// the item's 576 encoded bytes as 144 words in memory order (4-byte aligned)
DI fp tmask_coef_enc(const uint32_t* enc, int k) {
  fp v;
#pragma unroll
  for (int w = 0; w < 12; w++) v.l[11 - w] = __builtin_bswap32(enc[12 * k + w]);
  return v;
}

// key stream block j (eight big-endian words) from the midstate
DI void tmask_block(uint32_t (&ks)[8], const uint32_t (&mid)[8], uint32_t j) {
  uint32_t blk[16];
#pragma unroll
  for (int w = 0; w < 16; w++) blk[w] = 0;
  blk[0] = j;
  blk[1] = 0x80000000u;
  blk[15] = TMASK_BITS;
#pragma unroll
  for (int w = 0; w < 8; w++) ks[w] = mid[w];
  sha256_compress_batch(ks, blk);
}

// out[0 .. mlen) = in[0 .. mlen) XOR key stream, or mlen zero bytes for an item that is not good (mid is
// then not read). Every byte is read before it is written, so out == in is allowed; nothing outside
// [0, mlen) is touched. WORDS: in, out and mlen are multiples of 4 and the bytes move as dwords; otherwise
// byte by byte (a neighbouring lane owns the neighbouring bytes: no word-granular read-modify-write).
template <bool WORDS>
DI void tmask_apply(const uint32_t (&mid)[8], bool good, const uint8_t* in, uint8_t* out, uint32_t mlen) {
#pragma unroll 1
  for (uint32_t j = 0; 32 * j < mlen; j++) {
    uint32_t ks[8];
#pragma unroll
    for (int w = 0; w < 8; w++) ks[w] = 0;
    if (good) tmask_block(ks, mid, j);
    const uint32_t m = mlen - 32 * j < 32 ? mlen - 32 * j : 32;
    if constexpr (WORDS) {
      const uint32_t* in32 = (const uint32_t*)(in + 32 * j);
      uint32_t* out32 = (uint32_t*)(out + 32 * j);
#pragma unroll
      for (int w = 0; w < 8; w++)
        if (4u * w < m) out32[w] = good ? in32[w] ^ __builtin_bswap32(ks[w]) : 0u;
    } else {
#pragma unroll
      for (int b = 0; b < 32; b++)
        if ((uint32_t)b < m)
          out[32 * j + b] = good ? (uint8_t)(in[32 * j + b] ^ (uint8_t)(ks[b >> 2] >> (24 - 8 * (b & 3)))) : (uint8_t)0;
    }
  }
}

}  // namespace bls
