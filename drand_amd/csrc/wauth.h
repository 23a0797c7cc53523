// The authenticated timelock on the latency engine (k_lat_tauth_open.hip, k_lat_tauth_seal.hip; tauth.h,
// include/blsverify.h "authenticated timelock"): one ciphertext (U, V, W) opened, or one
// message sealed, by one workgroup end to end. The pairing side is wvteam.h tlock_team / wseal.h seal_team
// up to the final exponentiation; what follows is tauth.h's tail with the Gt value taken from the lanes:
//   open   s' = V XOR H2(E), M' = W XOR H4(s') streamed into H3, k' = H3(s', M'), accept iff k' != 0 and
//          k' G1 is the decoded U -- a walk over T1 on the critical path, shared out over the eight waves
//   seal   k = H3(s, M) in front, V = s XOR H2(K) and W = M XOR H4(s) behind
// The hashing is tauth.h's and tmask.h's own uint32_t code, run as wave-uniform work (one item per
// workgroup, every lane the same values), as xmd_b0_* and tseal_scalar are. The 576 encoded bytes of E / K
// are never written anywhere: their SHA-256 midstate is computed from the lane form (gt_midstate).
// Nothing here is constant-time (tseal.h).
#pragma once
#include "wseal.h"
#include "tauth.h"

namespace wv {

// byte stores are one lane's (a neighbouring item owns the neighbouring bytes: no word-granular
// read-modify-write; item i's bytes start at i mlen, so odd lengths are unaligned)
WVI bool lane0() {
#ifdef WV_HOST
  return true;
#else
  return threadIdx.x % 64 == 0;
#endif
}

// ------------------------------------------------------------------ midstate of a Gt value
// tmask.h tmask_midstate over the twelve Fp coefficients of the value whose w-power coefficient c is
// load(c), in the encoding's order (wpairing.h gt_encode_c: the w-powers 5, 3, 1, 4, 2, 0, each as imaginary
// then real part), out of Montgomery form as wseal.h g1_compress_store takes its words. Equal to
// tmask_midstate over tmask_coef_enc of the 576 bytes gt_encode_c would have written. Wave-uniform.
template <class Load>
WVI void gt_midstate(uint32_t (&mid)[8], Load load) {
  V cur = vsplat(0);
  bls::tmask_midstate(mid, [&](int j) {  // called for j = 0 .. 11 in order: the imaginary part loads the pair
    const int pos = j >> 1, c = pos < 3 ? 5 - 2 * pos : 10 - 2 * pos;
    if (!(j & 1)) cur = raw_canon(load(c));
    uint32_t w[12];
    limbs_to_words(cur, (j & 1) ? 0 : 1, w);
    bls::fp v;
    for (int i = 0; i < 12; i++) v.l[i] = w[i];
    return v;
  });
}

// ------------------------------------------------------------------ the walk for the check
// The windows [w0, w0 + nw) of wseal.h seal_walk: (the part of k in those windows) A, Jacobian, embedded; the
// point at infinity when every digit there is zero. seal_walk's argument holds for a part as it does for
// the whole: before window w the accumulator is s A with s the part's digits below w, s < 16^w, and the
// addend is j 16^w A with s < j 16^w and s + j 16^w <= k < r, so s != +-j 16^w (mod r).
WVI G2J auth_walk_part(const uint32_t* tab, const uint32_t (&k)[8], int w0, int nw) {
  G2J acc = g2_infinity();
  bool started = false;
#pragma unroll 1
  for (int w = w0; w < w0 + nw; w++) {
    const int d = bls::tseal_digit(k, w);
    if (!d) continue;
    const F xy = g1_entry_xy(tab + (size_t)bls::tseal_entry(w, d) * 24);
    const F qx = lo_only(xy), qy = lo_only(swap_halves(xy));
    if (started) acc = g2_madd_noexc(acc, qx, qy);
    else acc = {qx, qy, cst(WC_ONE2)};
    started = true;
  }
  return acc;
}

// seal_walk(tab, k) by the whole team (every wave calls it with the same k; every wave returns the sum):
// wave w walks its own eight windows, at most eight additions, and posts its partial sum to the slots
// AW_SLOT + 3 w; three rounds of the complete addition (wcurve.h g2_add) combine them. The slots are the key
// pair's Miller area, free behind the final exponentiation.
// Two partial sums over disjoint windows are a A and b A with a + b <= k < r, so a = +-b (mod r) only when
// both are 0: of g2_add's exceptional cases only "either operand at infinity" is ever taken -- and those
// are taken, by every wave whose windows are all zero. The caller clears the slots (auth_walk_clear) once
// every wave has read the sum: a partial sum is as good as its part of the scalar.
// The one-wave seal_walk stays the specification, and the form walk_waves == 1 runs (wave 0 walks all 64
// windows while the others wait: what DESIGN.md 8.9 measures the shared walk against; a wave-uniform choice).
constexpr int AW_SLOT = TB0;
static_assert(AW_SLOT + 3 * TEAM_WAVES <= TB1 && bls::TSEAL_WINDOWS == 8 * TEAM_WAVES, "eight windows and a G2 slot per wave");

WVI G2J auth_walk_team(Team& all, const uint32_t* tab, const uint32_t (&k)[8], int walk_waves = TEAM_WAVES) {
  const int w = all.id;
  if (walk_waves == 1) {
    if (w == 0) xst_g2(AW_SLOT, seal_walk(tab, k));
    team_sync(all);
    return xld_g2(AW_SLOT);
  }
  xst_g2(AW_SLOT + 3 * w, auth_walk_part(tab, k, 8 * w, 8));
  team_sync(all);
#pragma unroll 1
  for (int s = 1; s < TEAM_WAVES; s *= 2) {
    if ((w & (2 * s - 1)) == 0) xst_g2(AW_SLOT + 3 * w, g2_add(xld_g2(AW_SLOT + 3 * w), xld_g2(AW_SLOT + 3 * (w + s))));
    team_sync(all);
  }
  return xld_g2(AW_SLOT);
}
// behind a whole-team sync that follows every wave's read of the sum
WVI void auth_walk_clear(const Team& all) {
  for (int j = 0; j < 3; j++) xst(AW_SLOT + 3 * all.id + j, zero());
}

// ------------------------------------------------------------------ the opening tail
// tauth.h tauth_open_tail with the check left to the caller: check(k') says whether k' G1 is the decoded U
// (called by every wave alike, for k' != 0 only). Every wave of the n computes the same verdict; the
// store is shared out piece by piece (wave `id` of `n`, one lane writing bytes): a good item recomputes
// W XOR H4(s') for its pieces, any other gets mlen zero bytes -- the candidate plaintext never reaches memory.
// The hashing is out of line, one body per code object: its arguments and results travel in vector
// registers, so the device build keeps SHA-256's working set out of the scalar file (uni() brings the results,
// the same in every lane, back to scalars).
struct AuthWords {
  uint32_t w[8];
};
struct AuthOpened {
  uint32_t seed[8], k[8];
  uint32_t good;
};
WVI uint32_t uni(uint32_t v) {
#ifdef WV_HOST
  return v;
#else
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#endif
}
// s' = V XOR H2 (mid: the midstate of E's encoding), M' = W XOR H4(s') streamed into H3, k' = H3(s', M') reduced
WV_NOINL AuthOpened auth_open_hash(AuthWords mid, const uint8_t* v32, const uint8_t* ws, uint32_t mlen) {
  AuthOpened r;
  uint32_t h2[8];
  bls::tmask_block(h2, mid.w, 0);
  for (int w = 0; w < 8; w++) r.seed[w] = bls::load_be32(v32 + 4 * w) ^ h2[w];
  bls::tauth_sha s;
  bls::tauth_h3_begin(s, r.seed);
  bls::tauth_h4_xor<false>(r.seed, ws, mlen, [&](uint32_t, uint32_t m, const uint32_t (&p)[8]) { bls::tauth_h3_piece(s, p, m); });
  r.good = bls::tauth_h3_end(s, r.k) ? 1u : 0u;
  return r;
}
// piece j (m bytes) of W XOR H4(seed), the bytes behind m zero
WV_NOINL AuthWords auth_open_piece(AuthWords seed, const uint8_t* ws, uint32_t j, uint32_t m) {
  AuthWords p;
  uint32_t ks[8];
  bls::tauth_h4_block(ks, seed.w, j);
  bls::tauth_load_piece<false>(p.w, ws, j, m);
  for (int w = 0; w < 8; w++) p.w[w] = (p.w[w] ^ ks[w]) & bls::tauth_word_mask(m, w);
  return p;
}

template <class Check>
WVI uint8_t auth_open_tail(const uint32_t (&mid)[8], const uint8_t* v32, const uint8_t* ws, uint32_t mlen, uint8_t* out,
                           int id, int n, Check check) {
  AuthWords m8, seed;
  for (int w = 0; w < 8; w++) m8.w[w] = mid[w];
  const AuthOpened h = auth_open_hash(m8, v32, ws, mlen);
  uint32_t k[8];
  for (int w = 0; w < 8; w++) k[w] = uni(h.k[w]), seed.w[w] = h.seed[w];
  bool good = uni(h.good) != 0u;
  if (good) good = check(k);
#pragma unroll 1
  for (uint32_t j = (uint32_t)id; 32 * j < mlen; j += (uint32_t)n) {
    const uint32_t m = bls::tauth_piece_len(mlen, j);
    AuthWords p = {{0, 0, 0, 0, 0, 0, 0, 0}};
    if (good) p = auth_open_piece(seed, ws, j, m);
    if (lane0()) bls::tauth_store_piece<false>(out, j, m, p.w, !good);
  }
  return good ? (uint8_t)0 : bls::TAUTH_REJ_AUTH;
}
// mlen zero bytes, shared out as the tail's stores are
WVI void auth_store_zero(uint8_t* out, uint32_t mlen, int id, int n) {
  const uint32_t p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t j = (uint32_t)id; 32 * j < mlen; j += (uint32_t)n)
    if (lane0()) bls::tauth_store_piece<false>(out, j, bls::tauth_piece_len(mlen, j), p, true);
}

// ------------------------------------------------------------------ the opening item, one wave
// sig: the 96-byte compressed signature, u48 / v32 / ws: the ciphertext (ws: mlen bytes, 1 .. 256), T1: the
// generator's table; out: mlen bytes, the message or zeros. Returns the item's class and sets sig_cls, the
// signature's own decode class. Precedence as on the batch path (wverify.h tlock_class): U's decode class
// 2 .. 6, then a signature that does not decode, then TAUTH_REJ_AUTH. U or sigma at infinity: E = 1 as
// tlock_item takes it, and the check then fails as it fails for any wrong E (a U at infinity equals no k' G1).
// The specification of auth_open_team.
WVI uint8_t auth_open_item(const uint8_t* sig, const uint8_t* u48, const uint8_t* v32, const uint8_t* ws, uint32_t mlen,
                           const uint32_t* T1, uint8_t* out, uint8_t& sig_cls) {
  F sx, sy, ux, uy;
  bool s_inf, u_inf;
  sig_cls = g2_decompress(sig, sx, sy, s_inf);
  const uint8_t cls = tlock_class(g1_decompress(u48, ux, uy, u_inf), sig_cls);
  if (cls != bls::REJ_OK) {
    auth_store_zero(out, mlen, 0, 1);
    return cls;
  }
  W12 e = w12_one();
  if (!u_inf && !s_inf) {
    MPair pr[2];
    const bool active[2] = {true, false};
    pr[0] = mpair(dup0(ux), dup0(uy), sx, sy);
    e = final_exp(miller_loop(pr, active));
  }
  uint32_t mid[8];
  gt_midstate(mid, [&](int c) { return e.c[c]; });
  return auth_open_tail(mid, v32, ws, mlen, out, 0, 1, [&](const uint32_t (&k)[8]) {
    return !u_inf && g2_eq(seal_walk(T1, k), {ux, uy, cst(WC_ONE2)});
  });
}

// ------------------------------------------------------------------ the opening item, eight waves
// auth_open_item run by the eight waves of a workgroup (each wave calls it; every wave returns the same
// class and sets the same sig_cls): tlock_team's schedule as it stands up to the final exponentiation, then
//   all eight  the midstate of E from its slots, s', the stream into H3 and k' (uniform work, the same in
//              every wave: neither s' nor k' sits in LDS)
//   all eight  the walk (auth_walk_team), then the comparison of the sum with the decoded U, by every wave
//   all eight  the stores, a piece per wave
// U's affine coordinates stay where tlock_team's decode left them: S_UX, S_UY are the two slots behind the
// final exponentiation's last value (W_C) and outside both Miller areas, the subgroup check's slots (HS_*)
// and the walk's (AW_SLOT ..), so nothing between the decode and the comparison writes them.
static_assert(S_UX >= W_C + 6 && S_UY >= W_C + 6 && S_UX >= 2 * TA_SIZE, "U survives to the comparison");

WVI uint8_t auth_open_team(const uint8_t* sig, const uint8_t* u48, const uint8_t* v32, const uint8_t* ws, uint32_t mlen,
                           const uint32_t* T1, uint8_t* out, uint8_t& sig_cls, int walk_waves = TEAM_WAVES) {
  Team all = make_team(ALL_WAVES, CTR_ALL);
  bool e_one = false;
  const uint8_t cls = tlock_team_core(all, sig, u48, sig_cls, e_one);
  if (cls != bls::REJ_OK) {
    auth_store_zero(out, mlen, all.id, all.n);
    return cls;
  }
  if (e_one) {  // the pair was skipped: E = 1 into the slots the final exponentiation would have left it in
    for (int c = all.id; c < 6; c += all.n) xst(W_A + c, c == 0 ? cst(WC_ONE2) : zero());
    team_sync(all);
  }
  const bool u_inf = xld_word(XW_UINF) != 0u;
  uint32_t mid[8];
  gt_midstate(mid, [&](int c) { return xld(W_A + c); });
  return auth_open_tail(mid, v32, ws, mlen, out, all.id, all.n, [&](const uint32_t (&k)[8]) {
    const G2J a = auth_walk_team(all, T1, k, walk_waves);
    const bool eq = !u_inf && g2_eq(a, {xld(S_UX), xld(S_UY), cst(WC_ONE2)});
    team_sync(all);  // every wave has read the sum
    auth_walk_clear(all);
    return eq;
  });
}

// k = H3(seed, M) reduced (tauth.h tauth_derive), out of line as the opening's hashing is: the seed's words,
// the scalar's, and whether it is non-zero
WV_NOINL AuthOpened auth_derive(const uint8_t* seed32, const uint8_t* msg, uint32_t mlen) {
  AuthOpened r;
  bls::tauth_seed_words(r.seed, seed32);
  r.good = bls::tauth_derive<false>(r.seed, msg, mlen, r.k) ? 1u : 0u;
  return r;
}

// ------------------------------------------------------------------ the sealing tail
// tauth.h tauth_seal_tail as it stands, by one lane of the calling wave: V = seed XOR H2(K) and
// W = M XOR H4(seed), or 32 + mlen zero bytes for a refused item (mid is then not read)
WVI void auth_seal_tail(const uint32_t (&mid)[8], bool sealed, const uint32_t (&seed)[8], const uint8_t* msg, uint32_t mlen,
                        uint8_t* out_v, uint8_t* out_w) {
  if (lane0()) bls::tauth_seal_tail<false>(mid, sealed, seed, msg, mlen, out_v, out_w);
}

// ------------------------------------------------------------------ the sealing item, one wave
// seed: the item's 32 bytes as eight big-endian words (tauth_seed_words), msg: its mlen bytes (1 .. 256);
// k = H3(seed, msg) reduced, k_ok: k != 0 (tauth_derive; auth_seal_item below derives them). b0, T1, TK as
// seal_item. out_u: 48 bytes as 12 words; out_v: 32 bytes; out_w: mlen bytes. Returns ok; k == 0 writes
// zeros (no SHA-256 input is known to reach that branch: the host tool feeds it a directed value). K never
// leaves the wave. The specification of auth_seal_team_k.
WVI bool auth_seal_item_k(const uint32_t (&seed)[8], const uint32_t (&k)[8], bool k_ok, const uint8_t* msg, uint32_t mlen,
                          const uint32_t (&b0)[8], const uint32_t* T1, const uint32_t* TK, uint32_t* out_u, uint8_t* out_v,
                          uint8_t* out_w) {
  uint32_t mid[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!k_ok) {
    gst_if(lane_id() < 12u, out_u, lane_id(), vsplat(0));
    auth_seal_tail(mid, false, seed, msg, mlen, out_v, out_w);
    return false;
  }
  g1_compress_store(out_u, seal_walk(T1, k));
  F px, py, hx, hy;
  g2_to_affine(seal_walk(TK, k), px, py);
  W12 e = w12_one();
  if (hash_to_g2(b0, hx, hy)) {
    MPair pr[2];
    const bool active[2] = {true, false};
    pr[0] = mpair(dup0(px), dup0(py), hx, hy);
    e = final_exp(miller_loop(pr, active));
  }
  gt_midstate(mid, [&](int c) { return e.c[c]; });
  auth_seal_tail(mid, true, seed, msg, mlen, out_v, out_w);
  return true;
}
WVI bool auth_seal_item(const uint8_t* seed32, const uint8_t* msg, uint32_t mlen, const uint32_t (&b0)[8], const uint32_t* T1,
                        const uint32_t* TK, uint32_t* out_u, uint8_t* out_v, uint8_t* out_w) {
  const AuthOpened d = auth_derive(seed32, msg, mlen);
  uint32_t seed[8], k[8];
  for (int w = 0; w < 8; w++) seed[w] = uni(d.seed[w]), k[w] = uni(d.k[w]);
  const bool k_ok = uni(d.good) != 0u;
  return auth_seal_item_k(seed, k, k_ok, msg, mlen, b0, T1, TK, out_u, out_v, out_w);
}

// ------------------------------------------------------------------ the sealing item, eight waves
// auth_seal_item run by the eight waves of a workgroup (each wave calls it; every wave returns the same ok).
// Every wave derives k = H3(seed, M) itself (uniform work), so the scalar sits neither in LDS nor in global
// memory; then seal_team's schedule as it stands up to the final exponentiation (seal_team_core), the
// midstate of K from its slots and the tail by wave 0. K is never encoded: nothing of it reaches global
// memory. What it leaves in LDS -- K in W_A and the final exponentiation's intermediate values around it --
// is cleared before the workgroup exits: every block slot, shared out over the waves.
WVI bool auth_seal_team_k(const uint32_t (&seed)[8], const uint32_t (&k)[8], bool k_ok, const uint8_t* msg, uint32_t mlen,
                          const uint32_t (&b0)[8], const uint32_t* T1, const uint32_t* TK, uint32_t* out_u, uint8_t* out_v,
                          uint8_t* out_w) {
  Team all = make_team(ALL_WAVES, CTR_ALL);
  uint32_t mid[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int st = seal_team_core(all, k, k_ok, b0, T1, TK, out_u);
  if (st == SEAL_REFUSED) {  // every wave alike: no sync is pending
    if (all.id == 0) {
      gst_if(lane_id() < 12u, out_u, lane_id(), vsplat(0));
      auth_seal_tail(mid, false, seed, msg, mlen, out_v, out_w);
    }
    return false;
  }
  if (st == SEAL_ONE) {  // the pair was skipped: K = 1 into the slots the final exponentiation would have left it in
    for (int c = all.id; c < 6; c += all.n) xst(W_A + c, c == 0 ? cst(WC_ONE2) : zero());
    team_sync(all);
  }
  if (all.id == 0) {
    gt_midstate(mid, [&](int c) { return xld(W_A + c); });
    auth_seal_tail(mid, true, seed, msg, mlen, out_v, out_w);
  }
  team_sync(all);  // wave 0 has read K
  for (int s = all.id; s < BLK_SLOTS; s += all.n) xst(s, zero());
  return true;
}
WVI bool auth_seal_team(const uint8_t* seed32, const uint8_t* msg, uint32_t mlen, const uint32_t (&b0)[8], const uint32_t* T1,
                        const uint32_t* TK, uint32_t* out_u, uint8_t* out_v, uint8_t* out_w) {
  const AuthOpened d = auth_derive(seed32, msg, mlen);
  uint32_t seed[8], k[8];
  for (int w = 0; w < 8; w++) seed[w] = uni(d.seed[w]), k[w] = uni(d.k[w]);
  const bool k_ok = uni(d.good) != 0u;
  return auth_seal_team_k(seed, k, k_ok, msg, mlen, b0, T1, TK, out_u, out_v, out_w);
}

}  // namespace wv
