// One signature on the latency engine (k_lat_sign.hip; include/blsverify.h "Signing on the latency path",
// DESIGN.md 9.1): for a key sk reduced mod r and a message's b_0,
//   sigma = compress([sk] H(m))
// byte for byte what the batch kernel (k_sign.hip: curve.h jac_mul_scalar, g2_compress) returns. The scalar
// multiplication is wrecover.h's x-adic form: sk = sum_j d_j |x|^j with four 64-bit digits, and on G2
// [|x|] P = -psi(P), so [sk] H = sum_j [d_j] P_j with P_j = (-psi)^j (H) -- four independent ladders of 63
// doublings on four waves instead of one of 254.
//
// H(m) lies in G2 after the cofactor clearing, so psi(H) = [x] H holds and every P_j has order r (or H is
// the point at infinity, which skips the ladders). A ladder's intermediate multiples [k] P_j, 2 <= k < 2^64 < r,
// therefore never equal +-P_j: the condition of wcurve.h g2_madd_noexc.
//
// The key is wave-uniform data, as xmd_b0_* is: every wave reads it and decomposes it itself (scalar work),
// so neither the key nor a digit sits in LDS. A partial product [d_j] P_j does, and next to the public P_j
// it is a 64-bit discrete logarithm -- breakable, unlike the signature: its slots are overwritten before the
// workgroup exits. Nothing here is constant-time: g2_mul_digit branches on the digit's bits, as
// jac_mul_scalar branches on the key's.
#pragma once
#include "wrecover.h"
#include "wvteam.h"

namespace wv {

// H affine in the hash's hand-off slots; the partial products of waves 1 .. 3 in the signature pair's area
// (three slots each), which this item does not use otherwise
constexpr int S_GX = S_HX, S_GY = S_HY;
constexpr int SIGN_LADDERS = 4;
constexpr int SIGN_PART = TB1, SIGN_PART_END = SIGN_PART + 3 * (SIGN_LADDERS - 1);
static_assert(SIGN_PART_END <= TB1 + TA_SIZE, "the partial products fit the signature pair's area");

// [d_j] P_j for ladder j of the key sk (eight little-endian words below r) on the affine point (x, y) of G2
WVI G2J sign_ladder(const F& x, const F& y, const uint32_t (&sk)[8], int j) {
  uint64_t d[4];
  decompose_xabs(sk, d);
  const uint64_t dj = j == 0 ? d[0] : j == 1 ? d[1] : j == 2 ? d[2] : d[3];
  F px, py;
  lambda_base(x, y, j, px, py);
  return g2_mul_digit(px, py, dj);
}

// the 24 words of a signature to out (4-byte aligned) by plain masked vector stores: curve.h g2_compress of
// the point, the infinity encoding 0xc0 00.. included
WVI void sign_store(uint32_t* out, const G2J& s) {
  const V l = lane_id();
  const V be = g2_compress_words(s);  // word j, most significant byte first; one inversion for a finite point
  const V mem = (be >> 24) | ((be >> 8) & 0xff00u) | ((be << 8) & 0xff0000u) | (be << 24);
  gst_if(l < 24u, out, l, mem);
}

// ------------------------------------------------------------------ the item, one wave
// The specification of sign_team: the hash, then the four digit ladders in turn.
WVI void sign_item(const uint32_t (&b0)[8], const uint32_t (&sk)[8], uint32_t* out) {
  F hx, hy;
  G2J s = g2_infinity();
  if (hash_to_g2(b0, hx, hy))
    for (int j = 0; j < SIGN_LADDERS; j++) s = g2_add(s, sign_ladder(hx, hy, sk, j));
  sign_store(out, s);
}

// ------------------------------------------------------------------ the item, eight waves
// sign_item run by the eight waves of a workgroup (each wave calls it):
//
//   phase A  waves 0, 4, 5 (+ 3 as aff_serve): hash-to-G2 of the message, team_hash_key's branch as it stands;
//            wave 0 then converts H to affine (the item's one extra inversion, so that the ladders run mixed
//            additions) and hands x, y and the finite flag over
//   phase B  waves 0 .. 3: ladder j on wave j, one per SIMD; waves 1 .. 3 leave their product in LDS
//            waves 4 .. 7: idle
//   phase C  wave 0: the sum of the four, the conversion to affine, the compression and the 24 stores;
//            waves 1 .. 3 overwrite their slots once wave 0 has read them
//
// sk_words: the key reduced mod r (the host's scalar_mod_r), a wave-uniform pointer. A key == 0 has four
// zero digits: every ladder returns the point at infinity and so does the sum.
WVI void sign_team(const uint32_t (&b0)[8], const uint32_t* sk_words, uint32_t* out_words) {
  const int w = wave_id();
  Team all = make_team(ALL_WAVES, CTR_ALL);
  uint32_t sk[8];  // every wave alike, as seal_team reads its scalar: scalar work on uniform data
  for (int i = 0; i < 8; i++) sk[i] = sk_words[i];
  if ((HASH_TEAM >> w) & 1u) {
    Team th = make_team(HASH_TEAM, CTR_HASH);
    RingCounts rc;
    G2J q = g2_infinity();
    if (w == 0) q = team_hash_to_curve_sum(b0, rc);
    if (w == 5) {
      for (int i = 0; i < SSWU_POWS; i++) ring_pow_consume(HASH_RING, bls::EXP_P_MINUS_3_DIV_4, rc);
      iso_serve();
    }
    const G2J h = team_clear_cofactor(th, q);
    if (w == 0) {
      const bool fin = !g2_is_inf(h);
      if (fin) {
        F hx, hy;
        g2_to_affine(h, hx, hy);
        xst(S_GX, hx);
        xst(S_GY, hy);
      }
      xst_word(XW_HFIN, fin);
    }
  } else if (w == 3) {
    aff_serve();
  }
  team_sync(all);
  G2J s = g2_infinity();
  if (w < SIGN_LADDERS) {
    // (H at infinity is not reachable by a test: no message is known to hash there)
    if (xld_word(XW_HFIN) != 0u) s = sign_ladder(xld(S_GX), xld(S_GY), sk, w);
    if (w > 0) xst_g2(SIGN_PART + 3 * (w - 1), s);
  }
  team_sync(all);
  if (w == 0)
    for (int j = 1; j < SIGN_LADDERS; j++) s = g2_add(s, xld_g2(SIGN_PART + 3 * (j - 1)));
  team_sync(all);  // wave 0 holds the sum: the partial products go
  if (w > 0 && w < SIGN_LADDERS)
    for (int i = 0; i < 3; i++) xst(SIGN_PART + 3 * (w - 1) + i, zero());
  if (w == 0) sign_store(out_words, s);
}

}  // namespace wv
