// One timelock seal with its own round on the latency engine (k_lat_tseal.hip; include/blsverify.h
// "timelock"): for a 32-byte scalar k and a round,
//   U = k G1,   K = e(k pk, H(MessageV2(round)))^3
// -- one hash-to-G2, one single-pair Miller loop, one final exponentiation: the bilinearity form of
// tsealr.h, byte for byte what the batch kernels (k_tseal.hip, k_tsealr.hip) return. The two scalar
// multiplications are walks over the batch engine's tables of multiples (tseal.h T1, the key table TK of
// k_tsealr.hip: 64 windows x 15 affine entries of 24 words), one mixed addition per non-zero four-bit
// digit, on G1 points embedded in the G2 types (whash.h "G1 decompression").
//
// The scalar is wave-uniform data, as xmd_b0_* is: one item per workgroup, every lane sees the same
// digits and every table pointer is wave-uniform. Its reduction and digits are tscalar.h's, the batch
// kernels' own. Table indices depend on the digits: nothing here is constant-time (tseal.h).
#pragma once
#include "tscalar.h"
#include "wvteam.h"

namespace wv {

// ------------------------------------------------------------------ table walk
// [x | y] of one 24-word table entry (x, y: 12 words each, Montgomery R = 2^392, < 2p; a wave-uniform
// pointer) in Montgomery R = 2^400: wverify.h g1_coord with y's words in half 1, one product for both
WVI F g1_entry_xy(const uint32_t* e) {
  const V l = lane_id(), k = l & 15u, base = (l >> 5) * 12u;
  const V bit = k * 25u, wi = bit >> 5, sh = bit & 31u;
  const V lo = gld(e, base + sel(wi < 12u, wi, vsplat(11))), hi = gld(e, base + sel(wi < 11u, wi + 1u, vsplat(11)));
  const V v = ((lo >> sh) | sel((sh == 0u) | (wi >= 11u), vsplat(0), hi << ((32u - sh) & 31u))) & M25;  // (sh == 0: discarded)
  const V limbs = sel((l & 16u) == 0u, v, vsplat(0));
  return mulp(mkF(limbs, 2.0), cst(WC_C408_DUP));  // x 2^392 -> x 2^400
}

// sum over the windows w of tab[w][digit w of k] for k = eight little-endian words, 0 < k < r, and tab the
// table of a point A of order r (tab[w][j] = j 16^w A): k A, Jacobian, embedded.
// tseal.h tseal_u's argument carries over: before window w the accumulator is s A with s the scalar's
// windows below w, s < 16^w, and the addend is j 16^w A with j 16^w <= s + j 16^w <= k < r. So the
// accumulator is the point at infinity only before the first non-zero digit (s = 0: the entry is copied),
// and otherwise s != +-j 16^w (mod r): s < j 16^w, and s + j 16^w < r. Of the addition's exceptional
// cases only "accumulator at infinity" is ever taken, and every other step is the mixed addition without
// them (wcurve.h g2_madd_noexc, whose formulas never touch the curve constant).
WVI G2J seal_walk(const uint32_t* tab, const uint32_t (&k)[8]) {
  uint32_t q[8];
  for (int i = 0; i < 8; i++) q[i] = k[i];
  G2J acc = g2_infinity();
  bool started = false;
#pragma unroll 1
  for (int w = 0; w < bls::TSEAL_WINDOWS; w++) {
    const int d = (int)(q[0] & 15u);
    for (int i = 0; i < 7; i++) q[i] = (q[i] >> 4) | (q[i + 1] << 28);  // the next digit moves down
    q[7] >>= 4;
    if (!d) continue;
    const F xy = g1_entry_xy(tab + (size_t)bls::tseal_entry(w, d) * 24);
    const F qx = lo_only(xy), qy = lo_only(swap_halves(xy));  // [x | 0], [y | 0]
    if (started) acc = g2_madd_noexc(acc, qx, qy);
    else acc = {qx, qy, cst(WC_ONE2)};
    started = true;
  }
  return acc;
}

// ------------------------------------------------------------------ G1 compression
// curve.h g1_compress of an embedded point, the 48 bytes written to out (4-byte aligned) as 12 words by
// plain masked vector stores: the infinity encoding 0xc0 00.., else x canonical out of Montgomery form,
// big-endian, with the compression flag and the sign bit y > (p - 1) / 2. x, y: the point's affine form
// (ignored for the point at infinity).
WVI void g1_compress_store(uint32_t* out, bool inf, const F& x, const F& y) {
  const V l = lane_id();
  V be = sel(l == 0u, vsplat(0xc0000000u), vsplat(0));  // word j, most significant byte first
  if (!inf) {
    uint32_t w0[12];
    limbs_to_words(raw_canon(x), 0, w0);
    const bool largest = (ge_halves(raw_canon(y), cword(WC_PP1H_DUP)) & 1u) != 0;
    be = vsplat(0);
    for (int j = 0; j < 12; j++) be = sel(l == (uint32_t)j, vsplat(w0[11 - j]), be);
    be = be | sel(l == 0u, vsplat(0x80000000u | (largest ? 0x20000000u : 0u)), vsplat(0));
  }
  const V mem = (be >> 24) | ((be >> 8) & 0xff00u) | ((be << 8) & 0xff0000u) | (be << 24);
  gst_if(l < 12u, out, l, mem);
}
WVI void g1_compress_store(uint32_t* out, const G2J& p) {
  const bool inf = g2_is_inf(p);
  F x = zero(), y = zero();
  if (!inf) g2_to_affine(p, x, y);  // one inversion (wfield.h inv_gcd_lanes)
  g1_compress_store(out, inf, x, y);
}

// the outputs of a refused item (k == 0 mod r): 48 + 576 zero bytes, the stores shared out as the
// encoding's are (wave `id` of `n`)
WVI void seal_store_refused(uint32_t* out_u, uint32_t* out_gt, int id, int n) {
  if (id == 0) gst_if(lane_id() < 12u, out_u, lane_id(), vsplat(0));
  for (int c = id; c < 6; c += n) gt_store_words(out_gt, c, vsplat(0));
}

// ------------------------------------------------------------------ the item, one wave
// k32: the scalar's 32 big-endian bytes; b0: expand_message_xmd's b_0 of MessageV2(round); T1, TK: the
// generator's and the key's tables; out_u: the item's 48 bytes as 12 words, out_gt: its 576 bytes as 144
// words. Returns ok; a refused scalar writes zeros. H at infinity skips the pair: K = 1, the rule of
// wvteam.h team_hash_key's a0 (no message is known to hash there). The specification of seal_team.
WVI bool seal_item(const uint8_t* k32, const uint32_t (&b0)[8], const uint32_t* T1, const uint32_t* TK,
                   uint32_t* out_u, uint32_t* out_gt) {
  uint32_t k[8];
  if (!bls::tseal_scalar(k32, k)) {
    seal_store_refused(out_u, out_gt, 0, 1);
    return false;
  }
  g1_compress_store(out_u, seal_walk(T1, k));
  F px, py, hx, hy;
  g2_to_affine(seal_walk(TK, k), px, py);  // k pk: never the point at infinity (0 < k < r)
  W12 e = w12_one();
  if (hash_to_g2(b0, hx, hy)) {
    MPair pr[2];
    const bool active[2] = {true, false};
    pr[0] = mpair(dup0(px), dup0(py), hx, hy);
    e = final_exp(miller_loop(pr, active));
  }
  for (int c = 0; c < 6; c++) gt_encode_c(out_gt, c, e.c[c]);
  return true;
}

// ------------------------------------------------------------------ the item, eight waves
// seal_item run by the eight waves of a workgroup (each wave calls it; every wave returns the same ok):
//
//   phase A  waves 0, 4, 5 (+ 3 as aff_serve): hash-to-G2 of the message, team_hash_key's branch as it
//            stands
//            wave 6: the walk over T1, U to affine, compressed and stored
//            wave 7: the walk over TK, P = k pk to affine, its x and y into the slots S_PX, S_PY
//            waves 1, 2: idle (on the SIMDs of waves 5 and 6: the hash keeps SIMDs 0 and 1 to itself)
//   phase B  all eight: the Miller loop of the one pair e(P, H)
//   phase C  all eight: the final exponentiation; six waves encode
//
// Every wave reduces the scalar itself (scalar work on uniform data), so the digits never sit in LDS; P
// does, in the decoded signature's slots, which this item does not use, and those are overwritten once
// every wave has read them: P is as good as K to whoever reads it.
constexpr int S_PX = S_SX, S_PY = S_SY;
constexpr int SEAL_WAVE_U = 6, SEAL_WAVE_P = 7;

WVI bool seal_team(const uint8_t* k32, const uint32_t (&b0)[8], const uint32_t* T1, const uint32_t* TK,
                   uint32_t* out_u, uint32_t* out_gt) {
  const int w = wave_id();
  Team all = make_team(ALL_WAVES, CTR_ALL);
  uint32_t k[8];
  if (!bls::tseal_scalar(k32, k)) {  // every wave alike: no sync is pending
    seal_store_refused(out_u, out_gt, all.id, all.n);
    return false;
  }
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
      if (fin) {  // Jacobian (X, Y, Z) -> homogeneous (X Z : Y : Z^3), as verify_team
        xst(S_HX, dot(h.x, h.z));
        xst(S_HY, h.y);
        xst(S_HZ, dot(h.z, sqr2(h.z)));
      }
      xst_word(XW_HFIN, fin);
    }
  } else if (w == 3) {
    aff_serve();
  } else if (w == SEAL_WAVE_U) {
    g1_compress_store(out_u, seal_walk(T1, k));
  } else if (w == SEAL_WAVE_P) {
    F px, py;
    g2_to_affine(seal_walk(TK, k), px, py);
    xst(S_PX, dup0(px));
    xst(S_PY, dup0(py));
  }
  team_sync(all);
  const F px = xld(S_PX), py = xld(S_PY);
  const bool a0 = xld_word(XW_HFIN) != 0u;
  team_sync(all);  // every wave holds P: its slots go
  if (w == SEAL_WAVE_P) {
    xst(S_PX, zero());
    xst(S_PY, zero());
  }
  if (!a0) {  // the pair is skipped: K = 1 (not reachable by a test: no message is known to hash to infinity)
    for (int c = all.id; c < 6; c += all.n) gt_encode_c(out_gt, c, c == 0 ? cst(WC_ONE2) : zero());
    return true;
  }
  const MPair m0 = mpair_proj(px, py, xld(S_HX), xld(S_HY), xld(S_HZ));
  const int f = team_miller(all, m0, TB0);
  team_final_exp(all, f);
  for (int c = all.id; c < 6; c += all.n) gt_encode_c(out_gt, c, xld(W_A + c));
  return true;
}

// seal_team's schedule up to and including the final exponentiation, for an item whose scalar is derived
// and whose tail is not the encoding (wauth.h). k: the reduced scalar, eight little-endian words below r,
// k_ok: k != 0, as tseal_scalar or tauth_derive leaves them -- so no k32 in memory is needed; all: the
// whole-workgroup team, fresh from make_team. U is stored; K is not: SEAL_K leaves it in the slots
// W_A .. W_A + 5, SEAL_ONE in no slot (the pair is skipped: K = 1), and SEAL_REFUSED (k == 0) returns before
// anything is stored or synced. seal_team keeps its own text: k_lat_tseal is held to compile to what it
// compiled to.
constexpr int SEAL_REFUSED = 0, SEAL_ONE = 1, SEAL_K = 2;
WVI int seal_team_core(Team& all, const uint32_t (&k)[8], bool k_ok, const uint32_t (&b0)[8], const uint32_t* T1,
                       const uint32_t* TK, uint32_t* out_u) {
  const int w = wave_id();
  if (!k_ok) return SEAL_REFUSED;  // every wave alike: no sync is pending
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
      if (fin) {  // Jacobian (X, Y, Z) -> homogeneous (X Z : Y : Z^3), as verify_team
        xst(S_HX, dot(h.x, h.z));
        xst(S_HY, h.y);
        xst(S_HZ, dot(h.z, sqr2(h.z)));
      }
      xst_word(XW_HFIN, fin);
    }
  } else if (w == 3) {
    aff_serve();
  } else if (w == SEAL_WAVE_U) {
    g1_compress_store(out_u, seal_walk(T1, k));
  } else if (w == SEAL_WAVE_P) {
    F px, py;
    g2_to_affine(seal_walk(TK, k), px, py);
    xst(S_PX, dup0(px));
    xst(S_PY, dup0(py));
  }
  team_sync(all);
  const F px = xld(S_PX), py = xld(S_PY);
  const bool a0 = xld_word(XW_HFIN) != 0u;
  team_sync(all);  // every wave holds P: its slots go
  if (w == SEAL_WAVE_P) {
    xst(S_PX, zero());
    xst(S_PY, zero());
  }
  if (!a0) return SEAL_ONE;  // not reachable by a test: no message is known to hash to infinity
  const MPair m0 = mpair_proj(px, py, xld(S_HX), xld(S_HY), xld(S_HZ));
  const int f = team_miller(all, m0, TB0);
  team_final_exp(all, f);
  return SEAL_K;
}


}  // namespace wv
