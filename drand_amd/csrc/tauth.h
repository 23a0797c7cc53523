// Authenticated timelock (include/blsverify.h "authenticated timelock", blsv_tlock_encrypt_auth* /
// blsv_tlock_decrypt_auth*): the Fujisaki-Okamoto transform over the timelock of tseal.h / tlock.h, one lane
// per item. A ciphertext of an mlen-byte message M under the 32-byte seed s is (U, V, W):
//   k = H3(s, M)                                 the sealing scalar is derived, not drawn
//   U = compress(k G1),  K = B^k                 as blsv_tlock_seal computes them for that scalar
//   V = s XOR H2(encode(K)),  W = M XOR H4(s, mlen)
// and the opener, with E = e(U, sigma)^3, takes s' = V XOR H2(encode(E)), M' = W XOR H4(s', mlen),
// k' = H3(s', M') and accepts iff k' != 0 and k' G1 is the decoded U. This project's own instantiation:
//   H2(G)       = SHA-256(G || BE32(0)) over the 576 encoded bytes: block 0 of tmask.h's key stream
//   H3(s, M)    = (SHA-256(TAG3 || s || M || BE32(0)) || the first 16 bytes of SHA-256(TAG3 || s || M || BE32(1)))
//                 as a 384-bit big-endian integer, mod r (48 bytes: RFC 9380's L for this r, bias < 2^-128)
//   H4(s, mlen) = SHA-256(TAG4 || s || BE32(0)) || SHA-256(TAG4 || s || BE32(1)) || ...  truncated to mlen
// TAG3 || s is 48 bytes, so M starts on a SHA word; the counter comes last, so H3's two hashes share every
// block that is full before it. Not kyber's hashes and not wire-compatible with kyber or tlock.
// The shared host/device forms below are what tools/opcount tauth runs; k_tauth.hip holds the kernels.
#pragma once
#include "tmask.h"
#include "tseal.h"

namespace bls {

constexpr int TAUTH_SEED_LEN = 32;
constexpr int TAUTH_V_LEN = 32;
constexpr uint8_t TAUTH_REJ_AUTH = 10;  // BLSV_REJ_TLOCK_AUTH
// "BLSV-TLOCK-FO-H3" / "BLSV-TLOCK-FO-H4" as big-endian words: the two differ in their last byte
constexpr uint32_t TAUTH_TAG_W0 = 0x424c5356u, TAUTH_TAG_W1 = 0x2d544c4fu, TAUTH_TAG_W2 = 0x434b2d46u;
constexpr uint32_t TAUTH_TAG3_W3 = 0x4f2d4833u, TAUTH_TAG4_W3 = 0x4f2d4834u;

// 384 bits (be[0] the highest word) -> k = value mod r as eight little-endian words, the form tseal_digit
// reads; false for k == 0. Horner over the low 256 bits behind the top 128 (below r as they stand): one
// doubling with the next bit and one conditional subtraction of r per bit (2 k + 1 < 2 r < 2^256).
DI bool tauth_reduce384(const uint32_t (&be)[12], uint32_t (&k)[8]) {
#pragma unroll
  for (int w = 0; w < 8; w++) k[w] = w < 4 ? be[3 - w] : 0u;
#pragma unroll
  for (int word = 4; word < 12; word++) {
    const uint32_t bits = be[word];
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      uint32_t carry = (bits >> b) & 1u;
#pragma unroll
      for (int w = 0; w < 8; w++) {
        const uint32_t top = k[w] >> 31;
        k[w] = (k[w] << 1) | carry;
        carry = top;
      }
      uint32_t d[8];
      uint32_t borrow = 0;
#pragma unroll
      for (int w = 0; w < 8; w++) {
        const uint64_t t = (uint64_t)k[w] - R_ORDER[w] - borrow;
        d[w] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
      }
#pragma unroll
      for (int w = 0; w < 8; w++) k[w] = borrow ? k[w] : d[w];
    }
  }
  uint32_t any = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) any |= k[w];
  return any != 0;
}

// k (eight little-endian words) as the 32 big-endian bytes blsv_tlock_seal's scalars are
DI void tauth_scalar_bytes(uint8_t* be32, const uint32_t (&k)[8]) {
#pragma unroll
  for (int w = 0; w < 8; w++) {
    const uint32_t v = k[7 - w];
    be32[4 * w] = (uint8_t)(v >> 24);
    be32[4 * w + 1] = (uint8_t)(v >> 16);
    be32[4 * w + 2] = (uint8_t)(v >> 8);
    be32[4 * w + 3] = (uint8_t)v;
  }
}

// A SHA-256 stream: the state, the open block (zero behind the bytes it holds) and the bytes taken so far.
// The block is written through a select over its words, so that it stays in registers whatever the position.
struct tauth_sha {
  uint32_t st[8];
  uint32_t blk[16];
  uint32_t n;
};

DI void tauth_sha_or(tauth_sha& s, uint32_t idx, uint32_t v) {
#pragma unroll
  for (uint32_t w = 0; w < 16; w++) s.blk[w] |= w == idx ? v : 0u;
}

// the stream behind TAG || s: 48 bytes, twelve words of block 0
DI void tauth_sha_begin(tauth_sha& s, uint32_t tag_w3, const uint32_t (&seed)[8]) {
  sha256_init(s.st);
#pragma unroll
  for (int w = 0; w < 16; w++) s.blk[w] = 0;
  s.blk[0] = TAUTH_TAG_W0;
  s.blk[1] = TAUTH_TAG_W1;
  s.blk[2] = TAUTH_TAG_W2;
  s.blk[3] = tag_w3;
#pragma unroll
  for (int w = 0; w < 8; w++) s.blk[4 + w] = seed[w];
  s.n = 48;
}

// H3 as a stream: begin with the seed, take M in pieces of up to 32 bytes (eight big-endian words, the bytes
// behind the piece's length zero; every piece but the last is whole), finish into k. A piece starts on a
// multiple of 16 bytes (48 + 32 j), so each of its halves lies in one block and a block can only fill up at
// the end of a half: one compression site.
DI void tauth_h3_begin(tauth_sha& s, const uint32_t (&seed)[8]) { tauth_sha_begin(s, TAUTH_TAG3_W3, seed); }
DI void tauth_h3_piece(tauth_sha& s, const uint32_t (&m)[8], uint32_t len) {
#pragma unroll 1
  for (uint32_t h = 0; h < 2 && 16 * h < len; h++) {
    const uint32_t hl = len - 16 * h < 16 ? len - 16 * h : 16;
    const uint32_t base = (s.n >> 2) & 15u;
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
      const uint32_t v = h ? m[4 + w] : m[w];
      if (4 * w < hl) tauth_sha_or(s, base + w, v);
    }
    s.n += hl;
    if ((s.n & 63u) == 0) {
      sha256_compress_batch(s.st, s.blk);
#pragma unroll
      for (int w = 0; w < 16; w++) s.blk[w] = 0;
    }
  }
}

// ... BE32(ctr), the 0x80 byte and the bit length behind the stream: the digest. The stream may end on any
// byte, so the five bytes go into a pair of blocks -- the open one and the one behind it -- through a select
// over their 32 words; the second block is hashed only when the length did not fit the first.
DI void tauth_sha_end(const tauth_sha& s, uint32_t ctr, uint32_t (&dig)[8]) {
  uint32_t ab[32];
#pragma unroll
  for (int w = 0; w < 32; w++) ab[w] = w < 16 ? s.blk[w] : 0u;
  auto put = [&](uint32_t idx, uint32_t v) {
#pragma unroll
    for (uint32_t w = 0; w < 32; w++) ab[w] |= w == idx ? v : 0u;
  };
  const uint32_t pos = s.n & 63u, sh = 8u * (pos & 3u);
  put(pos >> 2, ctr >> sh);
  if (sh) put((pos >> 2) + 1, ctr << (32u - sh));
  put((pos + 4) >> 2, 0x80000000u >> sh);
  const bool two = pos + 5 > 56;
  const uint32_t bits = 8u * (s.n + 4);
  put(two ? 31u : 15u, bits);
#pragma unroll
  for (int w = 0; w < 8; w++) dig[w] = s.st[w];
#pragma unroll 1
  for (int b = 0; b < (two ? 2 : 1); b++) {
    uint32_t blk[16];
#pragma unroll
    for (int w = 0; w < 16; w++) blk[w] = b ? ab[16 + w] : ab[w];
    sha256_compress_batch(dig, blk);
  }
}
DI bool tauth_h3_end(const tauth_sha& s, uint32_t (&k)[8]) {
  uint32_t be[12];
#pragma unroll 1
  for (uint32_t c = 0; c < 2; c++) {
    uint32_t dig[8];
    tauth_sha_end(s, c, dig);
#pragma unroll
    for (int w = 0; w < 8; w++) {
      if (c == 0) be[w] = dig[w];
      else if (w < 4) be[8 + w] = dig[w];
    }
  }
  return tauth_reduce384(be, k);
}

// block j of H4's stream: SHA-256(TAG4 || s || BE32(j)), 52 bytes, one compression
DI void tauth_h4_block(uint32_t (&ks)[8], const uint32_t (&seed)[8], uint32_t j) {
  uint32_t blk[16];
  blk[0] = TAUTH_TAG_W0;
  blk[1] = TAUTH_TAG_W1;
  blk[2] = TAUTH_TAG_W2;
  blk[3] = TAUTH_TAG4_W3;
#pragma unroll
  for (int w = 0; w < 8; w++) blk[4 + w] = seed[w];
  blk[12] = j;
  blk[13] = 0x80000000u;
  blk[14] = 0;
  blk[15] = 8u * 52u;
  sha256_init(ks);
  sha256_compress_batch(ks, blk);
}

// the piece j of an item's mlen bytes as eight big-endian words, zero behind its length m (1..32)
template <bool WORDS>
DI void tauth_load_piece(uint32_t (&p)[8], const uint8_t* in, uint32_t j, uint32_t m) {
  if constexpr (WORDS) {
    const uint32_t* in32 = (const uint32_t*)(in + 32 * j);
#pragma unroll
    for (int w = 0; w < 8; w++) p[w] = 4u * w < m ? __builtin_bswap32(in32[w]) : 0u;
  } else {
#pragma unroll
    for (int w = 0; w < 8; w++) p[w] = 0;
#pragma unroll
    for (int b = 0; b < 32; b++)
      if ((uint32_t)b < m) p[b >> 2] |= (uint32_t)in[32 * j + b] << (24 - 8 * (b & 3));
  }
}
// ... and its store; zero == true stores m zero bytes. tmask_apply's split: dwords only when in, out and
// mlen are multiples of 4, else byte by byte (a neighbouring lane owns the neighbouring bytes)
template <bool WORDS>
DI void tauth_store_piece(uint8_t* out, uint32_t j, uint32_t m, const uint32_t (&p)[8], bool zero) {
  if constexpr (WORDS) {
    uint32_t* out32 = (uint32_t*)(out + 32 * j);
#pragma unroll
    for (int w = 0; w < 8; w++)
      if (4u * w < m) out32[w] = zero ? 0u : __builtin_bswap32(p[w]);
  } else {
#pragma unroll
    for (int b = 0; b < 32; b++)
      if ((uint32_t)b < m) out[32 * j + b] = zero ? (uint8_t)0 : (uint8_t)(p[b >> 2] >> (24 - 8 * (b & 3)));
  }
}
DI uint32_t tauth_piece_len(uint32_t mlen, uint32_t j) { return mlen - 32 * j < 32 ? mlen - 32 * j : 32; }
// the bytes of a word that lie inside a piece of m bytes
DI uint32_t tauth_word_mask(uint32_t m, int w) {
  if (4u * w + 4u <= m) return 0xffffffffu;
  if (4u * w >= m) return 0u;
  return 0xffffffffu << (8u * (4u - (m - 4u * w)));
}

// in[0 .. mlen) XOR H4(seed) piece by piece: take(j, m, piece) gets every piece with the bytes behind m zero
template <bool WORDS, typename Take>
DI void tauth_h4_xor(const uint32_t (&seed)[8], const uint8_t* in, uint32_t mlen, Take take) {
#pragma unroll 1
  for (uint32_t j = 0; 32 * j < mlen; j++) {
    const uint32_t m = tauth_piece_len(mlen, j);
    uint32_t ks[8], p[8];
    tauth_h4_block(ks, seed, j);
    tauth_load_piece<WORDS>(p, in, j, m);
#pragma unroll
    for (int w = 0; w < 8; w++) p[w] = (p[w] ^ ks[w]) & tauth_word_mask(m, w);
    take(j, m, p);
  }
}

// Where item i of a pass lies in the pass's packed message bytes. Uniform (blsv_tlock_*_auth*): every item has
// mlen bytes, item i from byte i * mlen. Ragged (blsv_tlock_*_auth*_var): a table of cnt + 1 prefix offsets the
// host staged, item i in [offs[i], offs[i + 1]), its length 1 .. TMASK_MSG_MAX (the host has checked it). The
// kernels of k_tauth.hip take either; the per-item forms below take the pointer and the length as ever.
struct tauth_span_uniform {
  uint32_t mlen;
  DI size_t off(size_t i) const { return i * mlen; }
  DI uint32_t len(size_t) const { return mlen; }
};
struct tauth_span_ragged {
  const uint32_t* offs;
  DI size_t off(size_t i) const { return offs[i]; }
  DI uint32_t len(size_t i) const { return offs[i + 1] - offs[i]; }
};

// k = H3(seed, msg[0 .. mlen)): what k_tauth_derive runs. seed32: the 32 bytes as they are in memory.
DI void tauth_seed_words(uint32_t (&seed)[8], const uint8_t* seed32) {
#pragma unroll
  for (int w = 0; w < 8; w++) seed[w] = load_be32(seed32 + 4 * w);
}
template <bool WORDS>
DI bool tauth_derive(const uint32_t (&seed)[8], const uint8_t* msg, uint32_t mlen, uint32_t (&k)[8]) {
  tauth_sha s;
  tauth_h3_begin(s, seed);
#pragma unroll 1
  for (uint32_t j = 0; 32 * j < mlen; j++) {
    const uint32_t m = tauth_piece_len(mlen, j);
    uint32_t p[8];
    tauth_load_piece<WORDS>(p, msg, j, m);
    tauth_h3_piece(s, p, m);
  }
  return tauth_h3_end(s, k);
}

// The sealing tail of one item: V = seed XOR H2(K), W = M XOR H4(seed), or zeros for a refused item
// (sealed == false; mid, the midstate of K's encoding (tmask_midstate), is then not read). out_w == msg is
// allowed: every piece is read before it is written.
template <bool WORDS>
DI void tauth_seal_tail(const uint32_t (&mid)[8], bool sealed, const uint32_t (&seed)[8], const uint8_t* msg,
                        uint32_t mlen, uint8_t* out_v, uint8_t* out_w) {
  uint32_t h2[8];
#pragma unroll
  for (int w = 0; w < 8; w++) h2[w] = 0;
  if (sealed) tmask_block(h2, mid, 0);
#pragma unroll
  for (int w = 0; w < 8; w++) {
    const uint32_t v = sealed ? seed[w] ^ h2[w] : 0u;
    out_v[4 * w] = (uint8_t)(v >> 24);
    out_v[4 * w + 1] = (uint8_t)(v >> 16);
    out_v[4 * w + 2] = (uint8_t)(v >> 8);
    out_v[4 * w + 3] = (uint8_t)v;
  }
  tauth_h4_xor<WORDS>(seed, msg, mlen,
                      [&](uint32_t j, uint32_t m, const uint32_t (&p)[8]) { tauth_store_piece<WORDS>(out_w, j, m, p, !sealed); });
}

// The re-encryption check: k G1 == U for the decoded affine U (Montgomery form), by a walk of T1 (entry(w, j)
// as tseal_u takes it) and a projective comparison -- for the Jacobian sum (X, Y, Z), X == xU Z^2 and
// Y == yU Z^3: no inversion, no square root, no compression. Infinity on either side is "not equal" (no
// non-zero k < r maps to infinity, and a U at infinity is the key everyone knows).
// Every value here lies in the redundant range [0, 2p), where one residue has two representatives, so no
// limbs are compared: fp_eq takes the difference (fp_sub keeps [0, 2p)) and tests it for 0 or p.
// ucoord(0) / ucoord(1): U's x / y, fetched at their one use so that they are not live across the walk.
template <typename Entry, typename UCoord>
DI bool tauth_check(const uint32_t (&k)[8], UCoord ucoord, bool u_inf, Entry entry) {
  const g1j a = tseal_u(k, entry);
  if (u_inf | jac_is_inf(a)) return false;
  const fp zz = fp_sqr(a.z);
  const bool ex = fp_eq(a.x, fp_mul(ucoord(0), zz));
  const bool ey = fp_eq(a.y, fp_mul(fp_mul(ucoord(1), zz), a.z));
  return ex & ey;
}

// The opening tail of one item whose class is 0: s' = V XOR H2(E), M' = W XOR H4(s') streamed into H3, the
// check, and only then the store -- a failing item's candidate plaintext never reaches memory: a good item
// recomputes W XOR H4(s') piece by piece (at most 8 more compressions) and stores it, any other gets mlen
// zero bytes. Returns the item's class: 0, or TAUTH_REJ_AUTH. out == ws is allowed (every piece is read
// before it is written, and all of W is read before the first store).
template <bool WORDS, typename Entry, typename UCoord>
DI uint8_t tauth_open_tail(const uint32_t (&mid)[8], const uint8_t* v32, const uint8_t* ws, uint32_t mlen, UCoord ucoord,
                           bool u_inf, Entry entry, uint8_t* out) {
  uint32_t seed[8], h2[8];
  tmask_block(h2, mid, 0);
#pragma unroll
  for (int w = 0; w < 8; w++) seed[w] = load_be32(v32 + 4 * w) ^ h2[w];
  tauth_sha s;
  tauth_h3_begin(s, seed);
  bool good = false;
#pragma unroll 1
  for (int pass = 0; pass < 2; pass++) {  // the check, then the store: one body, so one copy of the hashing
    tauth_h4_xor<WORDS>(seed, ws, mlen, [&](uint32_t j, uint32_t m, const uint32_t (&p)[8]) {
      if (pass == 0)
        tauth_h3_piece(s, p, m);
      else
        tauth_store_piece<WORDS>(out, j, m, p, !good);
    });
    if (pass == 0) {
      uint32_t k[8];
      good = tauth_h3_end(s, k);
      if (good) good = tauth_check(k, ucoord, u_inf, entry);
    }
  }
  return good ? (uint8_t)0 : TAUTH_REJ_AUTH;
}

}  // namespace bls
