// Op counter + CPU run of the engine's own device algorithms (drand_amd/csrc/*.h compiled for the host
// with -DBLS_HOST). Counts Montgomery multiplications (fp_mul_u12 calls; 288 32x32->64 limb products
// each: 144 for a*b + 144 for m*p in CIOS) per pipeline stage for ONE chained beacon, and checks that
// the beacon verifies. The stages are the batch path's: decompression is the decoding alone, and the
// signature's subgroup check is the closing test on the Miller lines' own [|x|]sigma, counted under
// Miller (`subgroup` runs that check on points from stdin beside g2_decompress's own).
// The counts are the algorithmic work figures used for bench.py's roofline
// (DESIGN.md §Roofline). Build + run: make -C tools opcount && tools/opcount <pk48hex> <round> <prevhex> <sighex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "../drand_amd/csrc/pairing.h"
#include "../drand_amd/csrc/hash.h"
#include "../drand_amd/csrc/tri.h"
#include "../drand_amd/csrc/testops.h"
#include "../drand_amd/csrc/rlc.h"
#include "../drand_amd/csrc/tlock.h"
#include "../drand_amd/csrc/tlockr.h"
#include "../drand_amd/csrc/hostlogic.h"
#include "../drand_amd/csrc/tseal.h"
#include "../drand_amd/csrc/tsealr.h"
#include "../drand_amd/csrc/tmask.h"
#include "../drand_amd/csrc/tauth.h"

namespace bls {
unsigned long long g_fp_mul_count = 0;
}
using namespace bls;

static std::vector<uint8_t> unhex(const char* s) {
  std::vector<uint8_t> v;
  size_t n = strlen(s);
  for (size_t i = 0; i + 1 < n; i += 2) {
    unsigned x;
    sscanf(s + i, "%2x", &x);
    v.push_back((uint8_t)x);
  }
  return v;
}

static void print_fp(const fp& a) {
  fp r = fp_from_mont(a);
  printf("\"");
  for (int i = 11; i >= 0; i--) printf("%08x", r.l[i]);
  printf("\"");
}

// hash <msghex>: KyberG2.Hash of an arbitrary message (xmd_b0_bytes path), affine raw coordinates
static int cmd_hash(const char* msghex) {
  auto msg = unhex(msghex);
  uint32_t b0[8];
  xmd_b0_bytes(b0, msg.data(), (uint32_t)msg.size(), DST);
  fp2 u0, u1;
  xmd_tail_to_field(b0, u0, u1);
  g2a h = g2_to_aff(hash_field_to_g2(u0, u1));
  printf("{\"x\": [");
  print_fp(h.x.c0);
  printf(", ");
  print_fp(h.x.c1);
  printf("], \"y\": [");
  print_fp(h.y.c0);
  printf(", ");
  print_fp(h.y.c1);
  printf("]}\n");
  return 0;
}

// fp_inv (binary GCD) against a^(p-2) on n seeded inputs in [0, 2p) plus edge values; prints the
// number of mismatches or out-of-range results as JSON
static int cmd_invfuzz(unsigned long n) {
  using namespace bls;
  unsigned long long s = 0x9e3779b97f4a7c15ull;
  auto next = [&]() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return (uint32_t)(s >> 11);
  };
  // structured inputs (the shapes that stress the 64-bit approximations: long runs of equal top bits,
  // values just around p and its halvings): 2^k, 2^k - 1, p - 2^k, (p + 1) / 2^k, (p - 1) / 2^k,
  // p +- d and 2p - d for small d
  std::vector<fp> st;
  auto pow2 = [](int k) {
    fp r = {};
    if (k < 384) r.l[k / 32] = 1u << (k % 32);
    return r;
  };
  auto sub = [](const fp& a, const fp& b) {
    fp r;
    unsigned br = 0;
    for (int i = 0; i < 12; i++) r.l[i] = __builtin_subc(a.l[i], b.l[i], br, &br);
    return r;
  };
  auto shr = [](fp a, int k) {
    for (; k > 0; k--) {
      for (int i = 0; i < 11; i++) a.l[i] = (a.l[i] >> 1) | (a.l[i + 1] << 31);
      a.l[11] >>= 1;
    }
    return a;
  };
  fp P, P1, Pm1, one = pow2(0);
  for (int i = 0; i < 12; i++) P.l[i] = P_RAW[i];
  Pm1 = sub(P, one);
  P1 = sub(P, sub(pow2(0), pow2(1)));  // p + 1 (p - (1 - 2) wraps to p + 1)
  for (int k = 0; k <= 381; k++) {
    st.push_back(pow2(k));
    st.push_back(sub(pow2(k), one));
    if (k < 381) st.push_back(sub(P, pow2(k)));
    st.push_back(shr(P1, k));
    st.push_back(shr(Pm1, k));
  }
  for (uint32_t d = 1; d < 64; d++) {
    fp dd = {};
    dd.l[0] = d;
    st.push_back(sub(P, dd));
    fp p2;
    for (int i = 0; i < 12; i++) p2.l[i] = P2_RAW[i];
    st.push_back(sub(p2, dd));
    st.push_back(sub(P, sub(fp{}, dd)));  // p + d
  }
  unsigned long bad = 0, unconverged = 0;
  const unsigned long total = n + st.size();
  for (unsigned long t = 0; t < total; t++) {
    fp x;
    for (int i = 0; i < 12; i++) x.l[i] = next();
    x.l[11] &= 0x1fffffffu;
    if (t < 6) {
      for (int i = 0; i < 12; i++) x.l[i] = (t == 2 || t == 3 || t == 5) ? P_RAW[i] : (t == 4 ? P2_RAW[i] : 0u);
      if (t == 1) x.l[0] = 1;
      if (t == 3) x.l[0] -= 1;  // p - 1
      if (t == 4) x.l[0] -= 1;  // 2p - 1
      if (t == 5) x.l[0] += 1;  // p + 1
    } else if (t >= n) {
      x = st[t - n];
    }
    uint32_t d[12];
    unsigned br = 0;
    for (int i = 0; i < 12; i++) d[i] = __builtin_subc(x.l[i], P2_RAW[i], br, &br);
    if (!br) for (int i = 0; i < 12; i++) x.l[i] = d[i];  // into [0, 2p)
    bool conv;
    const fp a = fp_from_u12(fp_inv_bingcd_raw(fp_to_u12(x), conv));  // the GCD alone, no fallback
    const fp b = fp_from_u12(fp_pow_p_minus_2(fp_to_u12(x)));
    br = 0;
    for (int i = 0; i < 12; i++) (void)__builtin_subc(a.l[i], P2_RAW[i], br, &br);
    bad += !fp_eq(a, b) || !br;
    unconverged += !conv;
  }
  printf("{\"inputs\": %lu, \"structured\": %zu, \"bad\": %lu, \"unconverged\": %lu}\n", total, st.size(), bad,
         unconverged);
  return bad != 0 || unconverged != 0;
}

// The square-root exponentiation (4-bit window, radix-2^28 running value) against the generic fixed-
// window one, and the Fp2 square (radix-2^28 sums) against Fp products, on random inputs including
// lazy sums (< 4p) as the callers pass them. Prints the mismatch count.
static int cmd_powfuzz(unsigned long n) {
  using namespace bls;
  unsigned long long s = 0x2545f4914f6cdd1dull;
  auto next = [&]() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return (uint32_t)(s >> 11);
  };
  auto rnd2p = [&]() {  // a value < 2^381 < 2p (2p's top word is 0x340223d4)
    fp x;
    for (int i = 0; i < 12; i++) x.l[i] = next();
    x.l[11] &= 0x1fffffffu;
    return x;
  };
  unsigned long bad_pow = 0, bad_sqr = 0, bad_mul = 0, bad_fp4 = 0;
  for (unsigned long t = 0; t < n; t++) {
    fp x = rnd2p();
    if (t == 0) x = fp_zero();
    if (t == 1) x = fp_one();
    const fp w = fp_from_u12(fp_pow_p_minus_3_div_4(fp_to_u12(x)));
    const fp ref = fp_pow_words<12>(x, EXP_P_MINUS_3_DIV_4);
    bad_pow += !fp_eq(w, ref);
    // Fp2 square of a reduced value and of a lazy sum
    const fp2 a = {rnd2p(), rnd2p()}, b = {rnd2p(), rnd2p()};
    for (int lazy = 0; lazy < 2; lazy++) {
      const fp2 in = lazy ? fp2_add_lazy(a, b) : a;
      const fp2 red = lazy ? fp2_add(a, b) : a;
      const fp2 got = fp2_sqr(in);
      const fp2 want = {fp_mul(fp_add(red.c0, red.c1), fp_sub(red.c0, red.c1)), fp_dbl(fp_mul(red.c0, red.c1))};
      bad_sqr += !fp2_eq(got, want);
    }
    // Fp2 product (fp.h: three products per column) on operands of every lazy level up to < 8p,
    // against the two-term dot-product body and Fp products; the result must also be < 2p
    auto lvl = [&](int l) {
      fp v = rnd2p();
      if (l >= 1) v = fp_add_lazy(v, rnd2p());
      if (l >= 2) v = fp_add_lazy(v, fp_add_lazy(rnd2p(), rnd2p()));
      if (l == 3) {  // the largest 12-word value below 8p
        for (int i = 0; i < 12; i++) v.l[i] = P2_RAW[i];
        v = fp_add_lazy(fp_add_lazy(v, v), fp_add_lazy(v, v));
        v.l[0] -= 1;
      }
      return v;
    };
    for (int l = 0; l < 16; l++) {
      const fp2 x = {lvl(l & 3), lvl((l >> 2) & 3)}, y = {lvl((l + 1) & 3), lvl((l >> 1) & 3)};
      const u24 k = fp2_mul_body_kara(fp2_to_u24(x), fp_to_u12(y.c0), fp_to_u12(y.c1));
      uint32_t x0[14], x1[14], y0[14], y1[14], yn[14];
      fp_split28(fp_to_u12(x.c0), x0);
      fp_split28(fp_to_u12(x.c1), x1);
      fp_split28(fp_to_u12(y.c0), y0);
      fp_split28(fp_to_u12(y.c1), y1);
      fp_neg28(y1, yn);
      const fp2 d = {fp_from_u12(fp_mont_dot<true>(x0, y0, x1, yn)), fp_from_u12(fp_mont_dot<true>(x0, y1, x1, y0))};
      const fp2 got = fp2_from_u24(k);
      bool in_range = true;
      for (const fp* c : {&got.c0, &got.c1}) {
        unsigned br = 0;
        for (int i = 0; i < 12; i++) (void)__builtin_subc(c->l[i], P2_RAW[i], br, &br);
        in_range = in_range && br;
      }
      bad_mul += !fp2_eq(got, d) || !in_range;
    }
    // the cyclotomic squaring's Fp4 square (tri.h fp4_sqr_k7: seven product columns, signed Y.a)
    // against Fp2 squares and products, on reduced inputs including 0, p - 1 and 2p - 1 limbs
    {
      fp4 x = {{rnd2p(), rnd2p()}, {rnd2p(), rnd2p()}};
      if (t % 7 == 1) x.a.c0 = fp_zero();
      if (t % 7 == 2) for (int i = 0; i < 12; i++) x.b.c1.l[i] = P2_RAW[i] - (i == 0);
      if (t % 7 == 3) for (int i = 0; i < 12; i++) x.a.c1.l[i] = P2_RAW[i] - (i == 0), x.b.c0.l[i] = 0;
      if (t % 7 == 4) x.a = fp2_zero();
      const fp4 y = fp4_sqr_k7(x);
      const fp2 want_a = fp2_add(fp2_sqr(x.a), fp2_mul_xi(fp2_sqr(x.b)));
      const fp2 want_b = fp2_dbl(fp2_mul(x.a, x.b));
      bool in_range = true;
      for (const fp* c : {&y.a.c0, &y.a.c1, &y.b.c0, &y.b.c1}) {
        unsigned br = 0;
        for (int i = 0; i < 12; i++) (void)__builtin_subc(c->l[i], P2_RAW[i], br, &br);
        in_range = in_range && br;
      }
      bad_fp4 += !fp2_eq(y.a, want_a) || !fp2_eq(y.b, want_b) || !in_range;
      // the interleaved Fp2 additive operations (tower.h) against the per-component fp.h ones
      const fp2 u = {rnd2p(), rnd2p()}, v = x.b;
      for (int sub = 0; sub < 2; sub++) {
        const fp2 g = fp2_addsub(u, v, sub != 0), w = sub ? fp2_sub(u, v) : fp2_add(u, v);
        const fp2 wr = sub ? fp2{fp_sub(u.c0, v.c0), fp_sub(u.c1, v.c1)} : fp2{fp_add(u.c0, v.c0), fp_add(u.c1, v.c1)};
        bad_fp4 += !fp2_eq(g, wr) || !fp2_eq(w, wr) || memcmp(&g, &wr, sizeof g) != 0 || memcmp(&w, &wr, sizeof w) != 0;
      }
      const fp2 xi = fp2_mul_xi(u), xr = {fp_sub(u.c0, u.c1), fp_add(u.c0, u.c1)};
      bad_fp4 += memcmp(&xi, &xr, sizeof xi) != 0;
      const fp2 ng = fp2_neg(u), nr = {fp_neg(u.c0), fp_neg(u.c1)};
      bad_fp4 += memcmp(&ng, &nr, sizeof ng) != 0;
    }
  }
  printf("{\"inputs\": %lu, \"pow_mismatch\": %lu, \"fp2_sqr_mismatch\": %lu, \"fp2_mul_mismatch\": %lu,"
         " \"fp4_sqr_mismatch\": %lu}\n", n, bad_pow, bad_sqr, bad_mul, bad_fp4);
  return (bad_pow || bad_sqr || bad_mul || bad_fp4) ? 1 : 0;
}

// The cofactor chains' addition (curve.h g2_add_inl_exc: no exceptional branch, a flag instead) and
// the subgroup check's mixed addition (g2_madd_inl_exc) against jac_add on curve points from the SSWU map, each also in a second Jacobian representation
// (X z^2, Y z^3, Z z): for distinct points the sums agree projectively and the flag stays clear; for
// P + P, P + (-P) and a point at infinity on either side the flag is set. Prints the mismatch count.
static int cmd_addfuzz(unsigned long n) {
  using namespace bls;
  unsigned long long s = 0x5851f42d4c957f2dull;
  auto next = [&]() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return (uint32_t)(s >> 11);
  };
  auto rnd = [&]() {
    fp x;
    for (int i = 0; i < 12; i++) x.l[i] = next();
    x.l[11] &= 0x0fffffffu;
    return fp_to_mont(x);
  };
  auto point = [&]() { return hash_field_to_q1(fp2{rnd(), rnd()}); };
  auto rescale = [&](const g2j& p) {
    const fp2 z = {rnd(), rnd()}, z2 = fp2_sqr(z);
    return g2j{fp2_mul(p.x, z2), fp2_mul(p.y, fp2_mul(z2, z)), fp2_mul(p.z, z)};
  };
  fp2 slots[3];
  const LdsFp2Slots park = {slots};
  unsigned long bad = 0;
  auto add = [&](const g2j& p, const g2j& q, bool& exc) {
    exc = false;
    return g2_add_inl_exc(p, [&]() { return q.x; }, [&]() { return q.y; }, [&]() { return q.z; }, park, exc);
  };
  auto madd = [&](const g2j& p, const g2a& q, bool& exc) {
    exc = false;
    return g2_madd_inl_exc(p, [&]() { return q.x; }, [&]() { return q.y; }, park, exc);
  };
  for (unsigned long t = 0; t < n; t++) {
    const g2j p = point(), q = point(), q2 = rescale(q), p2 = rescale(p);
    bool exc;
    // mixed addition (the subgroup check's): q affine
    const g2a qa = g2_to_aff(q), pa = g2_to_aff(p);
    const g2j m = madd(p2, qa, exc);
    bad += exc || !jac_eq(m, jac_add(p, q));
    (void)madd(p2, pa, exc);
    bad += !exc;
    (void)madd(p2, g2a{pa.x, fp2_neg(pa.y)}, exc);
    bad += !exc;
    (void)madd(jac_infinity<fp2>(), qa, exc);
    bad += !exc;
    const g2j r = add(p, q2, exc);
    bad += exc || !jac_eq(r, jac_add(p, q));
    (void)add(p, p2, exc);
    bad += !exc;
    (void)add(p, jac_neg(p2), exc);
    bad += !exc;
    (void)add(jac_infinity<fp2>(), q, exc);
    bad += !exc;
    (void)add(p, jac_infinity<fp2>(), exc);
    bad += !exc;
  }
  printf("{\"inputs\": %lu, \"add_mismatch\": %lu}\n", n, bad);
  return bad != 0;
}

// tower.h fp2_3u_pm_2x (the cyclotomic square's fused 3u +- 2x) against fp2_addsub + fp2_dbl +
// fp2_add on random operands in [0, 2p), the edges 0 and 2p - 1, and top words placed so that the
// quotient estimate sits on each boundary k D (k = 1..10) of its correction step; every result must
// equal the reference mod p and lie in [0, 2p).
static int cmd_linfuzz(unsigned long n) {
  using namespace bls;
  unsigned long long s = 0x9e3779b97f4a7c15ull;
  auto next = [&]() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return (uint32_t)(s >> 11);
  };
  auto below2p = [&](uint32_t top) {  // top word < P2_RAW[11]: the value is < 2p
    fp x;
    for (int i = 0; i < 11; i++) x.l[i] = next();
    x.l[11] = top;
    return x;
  };
  auto rnd = [&]() { return below2p(next() % P2_RAW[11]); };
  fp zero = fp_zero(), max2p;
  {
    unsigned br = 0;
    for (int i = 0; i < 12; i++) max2p.l[i] = __builtin_subc(P2_RAW[i], i == 0 ? 1u : 0u, br, &br);
  }
  auto lt2p = [](const fp& a) {
    unsigned br = 0;
    for (int i = 0; i < 12; i++) (void)__builtin_subc(a.l[i], P2_RAW[i], br, &br);
    return br != 0;
  };
  unsigned long bad = 0, cases = 0, edges = 0;
  auto check = [&](const fp2& u, const fp2& x, bool sub) {
    const fp2 got = fp2_3u_pm_2x(u, x, sub);
    const fp2 want = fp2_add(fp2_dbl(fp2_addsub(u, x, sub)), u);
    bad += !(fp_eq(got.c0, want.c0) && fp_eq(got.c1, want.c1) && lt2p(got.c0) && lt2p(got.c1));
    cases++;
  };
  const uint32_t D = P_RAW[11] + 1u;
  for (unsigned long t = 0; t < n; t++) {
    for (int sub = 0; sub < 2; sub++) {
      check({rnd(), rnd()}, {rnd(), rnd()}, sub);
      check({zero, max2p}, {max2p, zero}, sub);
      check({max2p, max2p}, {max2p, max2p}, sub);
      check({zero, zero}, {zero, zero}, sub);
    }
    // T = t >> 352 ~ 3 u11 + 2 y11 (+ carries), y = x or 2p - x: aim it at k D - 1, k D, k D + 1
    for (uint32_t k = 1; k <= 10; k++) {
      for (int d = -1; d <= 1; d++) {
        const int64_t T = (int64_t)k * D + d;
        const uint32_t a = next() % P2_RAW[11];  // u's top word
        const int64_t b = (T - 3 * (int64_t)a) / 2;  // y's top word
        if (b < 0 || b >= (int64_t)P2_RAW[11]) continue;
        // sub = false: y = x
        check({below2p(a), rnd()}, {below2p((uint32_t)b), rnd()}, false);
        // sub = true: y = 2p - x, so x's top word ~ P2_11 - b
        const int64_t bx = (int64_t)P2_RAW[11] - 1 - b;
        if (bx >= 0) check({below2p(a), rnd()}, {below2p((uint32_t)bx), rnd()}, true);
        edges++;
      }
    }
  }
  printf("{\"cases\": %lu, \"boundary_cases\": %lu, \"lin_mismatch\": %lu}\n", cases, edges, bad);
  return bad ? 1 : 0;
}

// tower.h fp6_mul_lin / fp12_sqr_lin (one reduction per output component, q p by KpMad) against
// fp6_mul / fp12_sqr: random operands in [0, 2p), operands at 2p - 1, and the lazily added operands
// (< 4p) fp12_sqr feeds its second product; results equal mod p and in [0, 2p).
static int cmd_f6fuzz(unsigned long n) {
  using namespace bls;
  unsigned long long s = 0x2545f4914f6cdd1dull;
  auto next = [&]() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return (uint32_t)(s >> 11);
  };
  auto rnd = [&]() {
    fp x;
    for (int i = 0; i < 11; i++) x.l[i] = next();
    x.l[11] = next() % P2_RAW[11];
    return x;
  };
  fp max2p;
  {
    unsigned br = 0;
    for (int i = 0; i < 12; i++) max2p.l[i] = __builtin_subc(P2_RAW[i], i == 0 ? 1u : 0u, br, &br);
  }
  auto lt2p = [](const fp& a) {
    unsigned br = 0;
    for (int i = 0; i < 12; i++) (void)__builtin_subc(a.l[i], P2_RAW[i], br, &br);
    return br != 0;
  };
  auto r6 = [&](bool edge) {
    fp6 a;
    fp2* c[3] = {&a.c0, &a.c1, &a.c2};
    for (auto* x : c) *x = edge ? fp2{max2p, (next() & 1) ? max2p : rnd()} : fp2{rnd(), rnd()};
    return a;
  };
  auto eq6 = [&](const fp6& x, const fp6& y) {
    const fp2* a[3] = {&x.c0, &x.c1, &x.c2};
    const fp2* b[3] = {&y.c0, &y.c1, &y.c2};
    bool ok = true;
    for (int k = 0; k < 3; k++)
      ok &= fp_eq(a[k]->c0, b[k]->c0) && fp_eq(a[k]->c1, b[k]->c1) && lt2p(a[k]->c0) && lt2p(a[k]->c1);
    return ok;
  };
  unsigned long bad = 0, cases = 0;
  for (unsigned long t = 0; t < n; t++) {
    for (int e = 0; e < 3; e++) {
      const fp6 a = r6(e == 1), b = r6(e == 2);
      bad += !eq6(fp6_mul_lin(a, b), fp6_mul(a, b));
      const fp6 la = fp6_add_lazy(a, r6(e == 1)), lb = fp6_add_lazy(b, r6(e != 0));  // < 4p
      bad += !eq6(fp6_mul_lin(la, lb), fp6_mul(la, lb));
      const fp12 f = {a, b}, g = fp12_sqr_lin(f, KpMad()), h = fp12_sqr(f);
      bad += !(eq6(g.c0, h.c0) && eq6(g.c1, h.c1));
      cases += 3;
    }
  }
  printf("{\"cases\": %lu, \"f6_mismatch\": %lu}\n", cases, bad);
  return bad ? 1 : 0;
}

// tri.h fp4_sqr_k6 (six product columns, four reductions, one body; wrap-around accumulators) against
// fp4_sqr_dot, fp4_sqr_k7 and three fp2_sqr / fp2_mul; every output must lie in [0, 2p). Inputs: random
// operands in [0, 2p); 0, p - 1, p and 2p - 1 in every component (all 256 combinations); operands whose
// limbs below the top one are all 2^28 - 1 (the largest columns: the partial sums of Y.b pass 2^63);
// the operands that make Y.b.c0 and Y.a.c0 as negative and as large as they get; operands built so that
// Y.b.c0 is exactly -2^k before its + p, each of which must take that branch. Then the whole
// Granger-Scott square of the three-lane layout (three Fp4 squares by the form this build selects,
// tri.h fp4_sqr_cyc, and the role combinations of tri_cyclotomic_sqr) against tower.h
// fp12_cyclotomic_sqr on cyclotomic values, 63 squares in a row per value.
static int cmd_sq6fuzz(unsigned long n) {
  using namespace bls;
  unsigned long long s = 0x6a09e667f3bcc909ull;
  auto next = [&]() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return (uint32_t)(s >> 11);
  };
  auto rnd = [&]() {  // uniform top word below 2p's: the value is < 2p
    fp x;
    for (int i = 0; i < 11; i++) x.l[i] = next();
    x.l[11] = next() % P2_RAW[11];
    return x;
  };
  auto lt2p = [](const fp& a) {
    unsigned br = 0;
    for (int i = 0; i < 12; i++) (void)__builtin_subc(a.l[i], P2_RAW[i], br, &br);
    return br != 0;
  };
  fp edge[4];  // 0, p - 1, p, 2p - 1
  edge[0] = fp_zero();
  for (int i = 0; i < 12; i++) edge[1].l[i] = P_RAW[i] - (i == 0), edge[2].l[i] = P_RAW[i], edge[3].l[i] = P2_RAW[i] - (i == 0);
  // every limb below the top one 2^28 - 1 (bits 0 .. 363 set), the top limb `top` (< 2p's top limb)
  auto full = [&](uint32_t top) {
    fp x;
    for (int i = 0; i < 11; i++) x.l[i] = 0xffffffffu;
    x.l[11] = (top << 12) | 0xfffu;
    return x;
  };
  const uint32_t top2p = P2_RAW[11] >> 12;  // 2p's top limb; full(top2p - 1) < 2p
  unsigned long bad = 0, cases = 0, negfix = 0;
  auto check = [&](const fp4& x) -> bool {
    const fp4 y = fp4_sqr_k6(x), d = fp4_sqr_dot(x), k7 = fp4_sqr_k7(x);
    const fp2 want_a = fp2_add(fp2_sqr(x.a), fp2_mul_xi(fp2_sqr(x.b)));
    const fp2 want_b = fp2_dbl(fp2_mul(x.a, x.b));
    bool ok = fp2_eq(y.a, want_a) && fp2_eq(y.b, want_b) && fp2_eq(y.a, d.a) && fp2_eq(y.b, d.b) && fp2_eq(y.a, k7.a) && fp2_eq(y.b, k7.b);
    for (const fp* c : {&y.a.c0, &y.a.c1, &y.b.c0, &y.b.c1}) ok = ok && lt2p(*c);
    bad += !ok;
    cases++;
    // how often the signed Y.b.c0 took its + p (a diagnostic: the branch is exercised)
    uint32_t a0[14], a1[14], b0[14], b1[14], t0[14], t1[14], t2[14], t3[14];
    fp_split28(fp_to_u12(x.a.c0), a0);
    fp_split28(fp_to_u12(x.a.c1), a1);
    fp_split28(fp_to_u12(x.b.c0), b0);
    fp_split28(fp_to_u12(x.b.c1), b1);
    bool n0, n1, n2;
    fp4_sqr_k6_t(a0, a1, b0, b1, t0, t1, t2, t3, n0, n1, n2);
    negfix += n2;
    return n2;
  };
  for (unsigned long t = 0; t < n; t++) check(fp4{{rnd(), rnd()}, {rnd(), rnd()}});
  for (int e = 0; e < 256; e++) check(fp4{{edge[e & 3], edge[(e >> 2) & 3]}, {edge[(e >> 4) & 3], edge[(e >> 6) & 3]}});
  for (int e = 0; e < 16; e++) {  // full limbs in every subset of the components, random elsewhere, and all tops
    auto pick = [&](int bit) { return ((e >> bit) & 1) ? full(top2p - 1) : rnd(); };
    check(fp4{{pick(0), pick(1)}, {pick(2), pick(3)}});
  }
  check(fp4{{full(top2p - 1), full(top2p - 1)}, {full(top2p - 1), full(top2p - 1)}});
  check(fp4{{full(0), full(top2p - 1)}, {full(top2p - 1), full(0)}});
  check(fp4{{full(top2p - 1), full(0)}, {full(top2p - 1), full(0)}});
  // Y.b.c0 = 2 (a0 b0 - a1 b1): most negative, largest; Y.b.c1 = 2 (a0 b1 + a1 b0): largest;
  // Y.a.c0 = a0^2 - a1^2 + b0^2 - b1^2 - 2 b0 b1: most negative, largest
  check(fp4{{edge[0], edge[3]}, {edge[0], edge[3]}});
  check(fp4{{edge[3], edge[0]}, {edge[3], edge[0]}});
  check(fp4{{edge[3], edge[3]}, {edge[3], edge[3]}});
  check(fp4{{edge[0], edge[3]}, {edge[3], edge[3]}});
  check(fp4{{edge[3], edge[0]}, {edge[3], edge[0]}});
  // Y.b.c0 negative before its + p, by construction: a0 b0 = 0, a1 = 2^(196 + i), b1 = 2^(195 + j) give
  // 2 (a0 b0 - a1 b1) = -R 2^(i + j), so m = 0 and the signed result is exactly -2^(i + j) (down to -2^371 at
  // a1 = b1 = 2^381, inside (-p/315, 0)); every one must take the fix-up and come out as p - 2^(i + j)
  unsigned long forced = 0, forced_neg = 0;
  auto pow2 = [](int k) {
    fp r = fp_zero();
    r.l[k / 32] = 1u << (k % 32);
    return r;
  };
  for (int i = 0; i <= 185; i += 37)
    for (int j = 0; j <= 186; j += 62) {
      forced_neg += check(fp4{{edge[0], pow2(196 + i)}, {edge[0], pow2(195 + j)}});
      forced_neg += check(fp4{{rnd(), pow2(196 + i)}, {edge[0], pow2(195 + j)}});  // a0 b0 = 0 still
      forced_neg += check(fp4{{edge[0], pow2(196 + i)}, {rnd(), pow2(195 + j)}});
      forced += 3;
    }
  // near the extremes, the low words random: about one in 315 of the first kind comes out negative
  // before its + p (m p < 8 p^2), against next to none of uniform operands
  for (unsigned long t = 0; t < n; t++) {
    auto near = [&](bool big) {
      fp x = big ? edge[3] : edge[0];
      for (int i = 0; i < 6; i++) x.l[i] = big ? x.l[i] - (next() & 0xffffu) - 1u : next();
      return x;
    };
    check(fp4{{near(false), near(true)}, {near(false), near(true)}});
    check(fp4{{near(true), near(false)}, {near(true), near(false)}});
  }

  // the three-lane Granger-Scott square (tri.h tri_cyclotomic_sqr without its lane exchange)
  unsigned long bad_cyc = 0, cyc = 0;
  for (unsigned long t = 0; t < n / 64 + 2; t++) {
    fp12 f;
    fp2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
    for (auto* x : c) *x = fp2{rnd(), rnd()};
    fp12 g = fexp_easy(f);  // cyclotomic
    for (int it = 0; it < 63; it++) {  // as many squares as one x-power takes
      const fp4 A[3] = {{g.c0.c0, g.c1.c1}, {g.c1.c0, g.c0.c2}, {g.c0.c1, g.c1.c2}};
      const fp4 S[3] = {fp4_sqr_cyc(A[0]), fp4_sqr_cyc(A[1]), fp4_sqr_cyc(A[2])};
      auto three = [](const fp2& u) { return fp2_add(fp2_dbl(u), u); };
      // role 0, 2: (3 Y.a - 2 a, 3 Y.b + 2 b), Y = own square (role 0), role 1's (role 2)
      // role 1:    (3 xi Y.b + 2 a, 3 Y.a - 2 b), Y = role 2's square
      const fp4 R0 = {fp2_sub(three(S[0].a), fp2_dbl(A[0].a)), fp2_add(three(S[0].b), fp2_dbl(A[0].b))};
      const fp4 R2 = {fp2_sub(three(S[1].a), fp2_dbl(A[2].a)), fp2_add(three(S[1].b), fp2_dbl(A[2].b))};
      const fp4 R1 = {fp2_add(three(fp2_mul_xi(S[2].b)), fp2_dbl(A[1].a)), fp2_sub(three(S[2].a), fp2_dbl(A[1].b))};
      fp12 h;
      h.c0.c0 = R0.a, h.c1.c1 = R0.b, h.c1.c0 = R1.a, h.c0.c2 = R1.b, h.c0.c1 = R2.a, h.c1.c2 = R2.b;
      const fp12 want = fp12_cyclotomic_sqr(g);
      bad_cyc += !fp12_eq(h, want) || !fp12_eq(want, fp12_sqr(g));
      cyc++;
      g = h;
    }
  }
  printf("{\"k6_selected\": %d, \"cases\": %lu, \"k6_mismatch\": %lu, \"yb_c0_negative\": %lu, \"yb_c0_forced_cases\": %lu, \"yb_c0_forced_negative\": %lu, \"cyclotomic_cases\": %lu, \"cyclotomic_mismatch\": %lu}\n",
         (int)BLS_FP4_SQR_K6, cases, bad, negfix, forced, forced_neg, cyc, bad_cyc);
  return (bad || bad_cyc) ? 1 : 0;
}

// ops: the raw operation hooks of drand_amd/csrc/testops.h on the host build (kind 0: the forms this
// build contains, KpMad in place of the LDS tables of k p). Reads one item per line from stdin: the op's
// name, then its operands, each Fp element as 96 hex digits (its twelve 32-bit words, most significant
// first), raw: nothing is converted or reduced. Prints the raw result elements of each item on one line.
// `ops list` prints name, Fp in, Fp out, kind of every op instead.
template <int OP, int NIN, int NOUT, int KIND>
static bool ops_run_t(const fp* x, fp* r) {
  if constexpr (KIND == 0) {
    test_op_run<OP, KpMad>(x, r);
    return true;
  } else {
    return false;
  }
}
static bool ops_run(int op, const fp* x, fp* r) {
  switch (op) {
#define X(name, nin, nout, kind) \
  case TOP_##name:               \
    return ops_run_t<TOP_##name, nin, nout, kind>(x, r);
    BLS_TEST_OPS(X)
#undef X
  }
  return false;
}
static int cmd_ops(bool list) {
  const TestOpInfo* tab = test_op_table();
  if (list) {
    for (int k = 0; k < TOP_COUNT; k++) printf("%s %d %d %d\n", tab[k].name, tab[k].nin, tab[k].nout, tab[k].kind);
    return 0;
  }
  static char line[64 + 24 * 97 + 8];
  unsigned long lineno = 0;
  while (fgets(line, sizeof line, stdin)) {
    lineno++;
    char* save = nullptr;
    const char* name = strtok_r(line, " \n", &save);
    if (!name) continue;
    int op = -1;
    for (int k = 0; k < TOP_COUNT; k++)
      if (!strcmp(tab[k].name, name)) op = k;
    if (op < 0 || tab[op].kind != 0) {
      fprintf(stderr, "ops: line %lu: no host op '%s'\n", lineno, name);
      return 2;
    }
    fp x[24], r[12];
    for (int k = 0; k < tab[op].nin; k++) {
      const char* tok = strtok_r(nullptr, " \n", &save);
      if (!tok || strlen(tok) != 96) {
        fprintf(stderr, "ops: line %lu: operand %d is not 96 hex digits\n", lineno, k);
        return 2;
      }
      for (int w = 0; w < 12; w++) {
        char b[9];
        memcpy(b, tok + 8 * (11 - w), 8);
        b[8] = 0;
        x[k].l[w] = (uint32_t)strtoul(b, nullptr, 16);
      }
    }
    if (!ops_run(op, x, r)) return 2;
    for (int k = 0; k < tab[op].nout; k++) {
      if (k) putchar(' ');
      for (int w = 11; w >= 0; w--) printf("%08x", r[k].l[w]);
    }
    putchar('\n');
  }
  return 0;
}

// rlc <seed32hex> <G>: the randomized batch verification's combination stage (drand_amd/csrc/rlc.h) as
// the device runs it -- lanes of RLC_LANE_ITEMS consecutive items, a group's lanes summed, to affine --
// on the (message, signature) pairs read from stdin, one "msghex sighex" per line, item i = line i. A
// message is hashed as KyberG2.Hash does, a signature decoded with the subgroup check; a decode reject
// enters neither sum, a point at infinity not its own. Prints every group's sums A = sum r_i H_i and
// B = sum r_i sigma_i compressed, and the Fp products of the stage per item, every predicated
// addition counted as executed (the select form runs it whatever the bit).
static int cmd_rlc(const char* seedhex, unsigned long G) {
  const auto sb = unhex(seedhex);
  if (sb.size() != 32 || G < (unsigned long)RLC_LANE_ITEMS || (G & (G - 1))) {
    fprintf(stderr, "rlc: a 32-byte seed and a power-of-two group size >= %d\n", RLC_LANE_ITEMS);
    return 2;
  }
  uint32_t seed[8];
  for (int k = 0; k < 8; k++) seed[k] = load_be32(sb.data() + 4 * k);
  std::vector<g2a> P[2];
  std::vector<uint64_t> r[2];
  static char line[8192];
  while (fgets(line, sizeof line, stdin)) {
    char* save = nullptr;
    const char* mh = strtok_r(line, " \n", &save);
    const char* sh = mh ? strtok_r(nullptr, " \n", &save) : nullptr;
    if (!mh) continue;
    if (!sh) return 2;
    const auto msg = unhex(strcmp(mh, "-") ? mh : ""), sig = unhex(sh);
    if (sig.size() != 96) return 2;
    uint32_t b0[8];
    xmd_b0_bytes(b0, msg.data(), (uint32_t)msg.size(), DST);
    fp2 u0, u1;
    xmd_tail_to_field(b0, u0, u1);
    const g2j hj = hash_field_to_g2(u0, u1);
    const bool hinf = jac_is_inf(hj);
    g2a s;
    bool sinf;
    const uint8_t cls = g2_decompress(sig.data(), s, sinf, true);
    const uint64_t ri = rlc_scalar(seed, P[0].size());
    P[0].push_back(hinf ? g2a{fp2_zero(), fp2_zero()} : g2_to_aff(hj));
    P[1].push_back(s);
    r[0].push_back(cls == REJ_OK && !hinf ? ri : 0);
    r[1].push_back(cls == REJ_OK && !sinf ? ri : 0);
  }
  const size_t n = P[0].size(), ng = (n + G - 1) / G, L = RLC_LANE_ITEMS;
  if (!n) return 2;
  const unsigned long long c0 = g_fp_mul_count;
  std::vector<g2j> sums[2];
  for (int w = 0; w < 2; w++) {
    for (size_t g = 0; g < ng; g++) {
      const size_t lo = g * G, hi = std::min(n, lo + G);
      std::vector<g2j> part;
      for (size_t i0 = lo; i0 < hi; i0 += L)
        part.push_back(rlc_accumulate(
            (int)std::min(L, hi - i0), [&](int k) { return P[w][i0 + k].x; }, [&](int k) { return P[w][i0 + k].y; },
            [&](int k, int b) { return ((r[w][i0 + k] >> b) & 1u) != 0; }));
      g2j sum = rlc_sum(part.size(), [&](size_t q) { return part[q]; });
      if (!jac_is_inf(sum)) sum = jac_from_aff(g2_to_aff(sum));  // the device stores the affine form
      sums[w].push_back(sum);
    }
  }
  const unsigned long long total = g_fp_mul_count - c0;
  printf("{\"items\": %zu, \"group\": %lu, \"groups\": %zu, ", n, G, ng);
  for (int w = 0; w < 2; w++) {
    printf("\"%s\": [", w ? "b" : "a");
    for (size_t g = 0; g < ng; g++) {
      uint8_t out[96];
      g2_compress(out, sums[w][g]);
      printf("%s\"", g ? ", " : "");
      for (int k = 0; k < 96; k++) printf("%02x", out[k]);
      printf("\"");
    }
    printf("], ");
  }
  printf("\"fp_mul\": %llu, \"fp_mul_per_item\": %.1f}\n", total, (double)total / (double)n);
  return 0;
}

// tlock <sig96hex>: the timelock opening (drand_amd/csrc/tlock.h) as the device runs it -- sigma
// decoded with the subgroup check and prepared once into the table of P-independent line coefficients,
// then per U (stdin, one 48-byte compressed G1 point in hex per line) the f pass against the table, the
// final exponentiation and the 576-byte Gt encoding. A U that does not decode prints null and its
// class; a pair with a point at infinity is skipped (E = 1). "lines_match": every table line times
// (xU, yU) equals, as field elements, the line miller_lines (miller_dbl_step / miller_add_step) emits
// for the same pair, and the f pass equals miller_loop_multi<1>. Prints the Fp products of the
// preparation (once per sigma) and of one item's f pass and final exponentiation.
static int cmd_tlock(const char* sighex) {
  const auto sig = unhex(sighex);
  if (sig.size() != 96) return 2;
  g2a Q;
  bool qinf;
  const uint8_t scls = g2_decompress(sig.data(), Q, qinf, true);
  if (scls != REJ_OK) {
    printf("{\"sig_class\": %d}\n", scls);
    return 1;
  }
  static fp2 tab[MILLER_STEPS][3];
  unsigned long long n_prepare = 0, n_f = 0, n_fexp = 0;
  if (!qinf) {
    const unsigned long long c0 = g_fp_mul_count;
    tlock_prepare(Q, [&](int step, int c, const fp2& v) { tab[step][c] = v; });
    n_prepare = g_fp_mul_count - c0;
  }
  auto coef = [&](int step, int c) { return tab[step][c]; };
  bool lines_match = true;
  std::vector<std::string> enc;
  std::vector<int> classes;
  static char line_buf[256];
  while (fgets(line_buf, sizeof line_buf, stdin)) {
    char* save = nullptr;
    const char* uh = strtok_r(line_buf, " \n", &save);
    if (!uh) continue;
    const auto ub = unhex(uh);
    if (ub.size() != 48) return 2;
    g1a U;
    bool uinf;
    const uint8_t cls = g1_decompress(ub.data(), U, uinf);
    classes.push_back(cls);
    if (cls != REJ_OK) {
      enc.push_back("");
      continue;
    }
    fp12 f = fp12_one();
    if (!uinf && !qinf) {
      unsigned long long c0 = g_fp_mul_count;
      f = tlock_f(coef, U.x, U.y);
      n_f = g_fp_mul_count - c0;
      // the lines and the value of the two-pass Miller loop for the same pair
      miller_lines(U, [&]() { return Q; }, [&](int step, const line& l) {
        const line t = tlock_line(coef, step, U.x, U.y);
        lines_match &= fp2_eq(t.a0, l.a0) && fp2_eq(t.a1, l.a1) && fp2_eq(t.a4, l.a4);
      });
      const g1a Ps[1] = {U};
      const g2a Qs[1] = {Q};
      const bool act[1] = {true};
      lines_match &= fp12_eq(f, miller_loop_multi<1>(Ps, Qs, act));
    }
    const unsigned long long c1 = g_fp_mul_count;
    const fp12 e = final_exponentiation(f);
    n_fexp = g_fp_mul_count - c1;
    uint8_t out[TLOCK_GT_LEN];
    tlock_encode(out, e);
    std::string h;
    char b[3];
    for (int k = 0; k < TLOCK_GT_LEN; k++) {
      snprintf(b, sizeof b, "%02x", out[k]);
      h += b;
    }
    enc.push_back(h);
  }
  printf("{\"sig_class\": 0, \"sig_inf\": %s, \"lines_match\": %s, \"class\": [", qinf ? "true" : "false",
         lines_match ? "true" : "false");
  for (size_t i = 0; i < classes.size(); i++) printf("%s%d", i ? ", " : "", classes[i]);
  printf("], \"e\": [");
  for (size_t i = 0; i < enc.size(); i++) {
    if (enc[i].empty())
      printf("%snull", i ? ", " : "");
    else
      printf("%s\"%s\"", i ? ", " : "", enc[i].c_str());
  }
  printf("], \"fp_mul\": {\"tlock_prepare\": %llu, \"tlock_f\": %llu, \"final_exp\": %llu}}\n", n_prepare, n_f, n_fexp);
  return lines_match ? 0 : 1;
}

static std::string hex_of(const uint8_t* b, size_t n) {
  std::string h;
  char t[3];
  for (size_t k = 0; k < n; k++) {
    snprintf(t, sizeof t, "%02x", b[k]);
    h += t;
  }
  return h;
}

// tmask: the fused tail of timelock encrypt / decrypt (drand_amd/csrc/tmask.h) as the device runs it. stdin:
// the first line is mlen (1 .. 256), then one item per line, "gt576hex msghex [class]" (class defaults to 0;
// an item whose class is not 0 gets mlen zero bytes). Prints the masked bytes of every item. "forms_match":
// the two input forms (the SoA capture in Montgomery form and the encoded bytes), the dword and the byte
// stores, and the in-place run all give the same bytes, and the guard bytes around every output are intact.
static int cmd_tmask() {
  static char buf[4096];
  if (!fgets(buf, sizeof buf, stdin)) return 2;
  const unsigned long mlen = strtoul(buf, nullptr, 10);
  if (mlen < 1 || mlen > (unsigned long)TMASK_MSG_MAX) return 2;
  std::vector<std::vector<uint8_t>> gts, msgs;
  std::vector<int> classes;
  while (fgets(buf, sizeof buf, stdin)) {
    char* save = nullptr;
    const char* gh = strtok_r(buf, " \n", &save);
    if (!gh) continue;
    const char* mh = strtok_r(nullptr, " \n", &save);
    const char* ch = strtok_r(nullptr, " \n", &save);
    if (!mh) return 2;
    gts.push_back(unhex(gh));
    msgs.push_back(unhex(mh));
    classes.push_back(ch ? atoi(ch) : 0);
    if (gts.back().size() != (size_t)TMASK_GT_LEN || msgs.back().size() != mlen) return 2;
  }
  const size_t n = gts.size();
  if (!n) return 2;
  // the SoA capture as the final exponentiation leaves it: slot 11 - k holds coefficient k, Montgomery form
  std::vector<uint32_t> E(144 * n), enc(144 * n);
  for (size_t i = 0; i < n; i++) {
    for (int k = 0; k < 12; k++) st_fp(E.data(), n, i, 11 - k, fp_to_mont(fp_raw_from_be48(gts[i].data() + 48 * k)));
    memcpy(enc.data() + 144 * i, gts[i].data(), TMASK_GT_LEN);
  }
  constexpr size_t G = 8;  // guard bytes (a multiple of 4: the dword runs stay aligned)
  auto run = [&](int form, bool words, bool in_place) {
    // items with their guards, 4-byte aligned through the uint32 backing
    const size_t stride = mlen;
    std::vector<uint32_t> back((2 * G + n * stride) / 4 + 2);
    uint8_t* base = (uint8_t*)back.data();
    memset(base, 0xAA, 2 * G + n * stride);
    std::vector<uint32_t> inb((n * stride) / 4 + 2);
    uint8_t* in = in_place ? base + G : (uint8_t*)inb.data();
    for (size_t i = 0; i < n; i++) memcpy(in + i * stride, msgs[i].data(), mlen);
    for (size_t i = 0; i < n; i++) {
      const bool good = classes[i] == 0;
      uint32_t mid[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (good) {
        if (form == 0)
          tmask_midstate(mid, [&](int k) { return tmask_coef_soa(E.data(), n, i, k); });
        else
          tmask_midstate(mid, [&](int k) { return tmask_coef_enc(enc.data() + 144 * i, k); });
      }
      if (words)
        tmask_apply<true>(mid, good, in + i * stride, base + G + i * stride, (uint32_t)mlen);
      else
        tmask_apply<false>(mid, good, in + i * stride, base + G + i * stride, (uint32_t)mlen);
    }
    std::vector<uint8_t> out(base + G, base + G + n * stride);
    for (size_t g = 0; g < G; g++)
      if (base[g] != 0xAA || base[G + n * stride + g] != 0xAA) out.clear();  // a guard was written
    return out;
  };
  const std::vector<uint8_t> out = run(0, false, false);
  bool match = !out.empty() && run(1, false, false) == out && run(0, false, true) == out;
  if (mlen % 4 == 0) match &= run(0, true, false) == out && run(1, true, true) == out;
  printf("{\"mlen\": %lu, \"forms_match\": %s, \"out\": [", mlen, match ? "true" : "false");
  for (size_t i = 0; i < n && !out.empty(); i++)
    printf("%s\"%s\"", i ? ", " : "", hex_of(out.data() + i * mlen, mlen).c_str());
  printf("]}\n");
  return match ? 0 : 1;
}

// tauth: the authenticated timelock's forms (drand_amd/csrc/tauth.h) as the device runs them. stdin: the first
// line is mlen (1 .. 256), then one line per case:
//   reduce <hex96>                           tauth_reduce384 of 48 big-endian bytes
//   seal <seed32hex> <msghex> <gt576hex>     k = H3, then V and W from the given K (zeros when k == 0)
//   open <gt576hex> <u48hex> <v32hex> <whex> [class]
//                                            the opening tail over the given E; u48 is decoded here, an
//                                            undecodable one gives its class, a class other than 0 is kept
// The seal cases run as one packed batch and so do the open cases, each with guard bytes around every
// output. "forms_match": the byte stores, the dword stores (mlen a multiple of 4) and the in-place run all
// give the same bytes, classes and scalars, and every guard is intact. "fp_mul_open": the Fp products of the
// last good item's check (the T1 walk and the comparison).
// tauthv: the same with a length per case (the first line is 0): every seal case has its own message length and
// every open case its own W length, 1 .. 256, and the packed batches take their spans from a table of prefix
// offsets through tauth_span_ragged, as the kernels' ragged forms do. The dword form runs when every length of
// the batch is a multiple of 4; "dword_forms": how many of the two batches ran it.
static int cmd_tauth(bool ragged) {
  static char buf[8192];
  if (!fgets(buf, sizeof buf, stdin)) return 2;
  const unsigned long mlen = strtoul(buf, nullptr, 10);
  if (ragged ? mlen != 0 : (mlen < 1 || mlen > (unsigned long)TMASK_MSG_MAX)) return 2;
  auto len_ok = [&](size_t v) { return ragged ? v >= 1 && v <= (size_t)TMASK_MSG_MAX : v == mlen; };
  struct SealIn {
    std::vector<uint8_t> seed, msg, gt;
  };
  struct OpenIn {
    std::vector<uint8_t> gt, u, v, w;
    int cls;
  };
  std::vector<std::vector<uint8_t>> reds;
  std::vector<SealIn> seals;
  std::vector<OpenIn> opens;
  while (fgets(buf, sizeof buf, stdin)) {
    char* save = nullptr;
    const char* cmd = strtok_r(buf, " \n", &save);
    if (!cmd) continue;
    std::vector<const char*> a;
    while (const char* t = strtok_r(nullptr, " \n", &save)) a.push_back(t);
    if (!strcmp(cmd, "reduce") && a.size() == 1) {
      reds.push_back(unhex(a[0]));
      if (reds.back().size() != 48) return 2;
    } else if (!strcmp(cmd, "seal") && a.size() == 3) {
      seals.push_back({unhex(a[0]), unhex(a[1]), unhex(a[2])});
      const SealIn& x = seals.back();
      if (x.seed.size() != 32 || !len_ok(x.msg.size()) || x.gt.size() != (size_t)TMASK_GT_LEN) return 2;
    } else if (!strcmp(cmd, "open") && (a.size() == 4 || a.size() == 5)) {
      opens.push_back({unhex(a[0]), unhex(a[1]), unhex(a[2]), unhex(a[3]), a.size() == 5 ? atoi(a[4]) : 0});
      const OpenIn& x = opens.back();
      if (x.gt.size() != (size_t)TMASK_GT_LEN || x.u.size() != 48 || x.v.size() != 32 || !len_ok(x.w.size())) return 2;
    } else {
      return 2;
    }
  }
  constexpr size_t G = 8;  // guard bytes (a multiple of 4: the dword runs stay aligned)
  auto guarded = [&](std::vector<uint32_t>& back, size_t bytes) {
    back.assign((2 * G + bytes) / 4 + 2, 0);
    memset(back.data(), 0xAA, 2 * G + bytes);
    return (uint8_t*)back.data() + G;
  };
  auto guards_ok = [&](const uint8_t* p, size_t bytes) {
    for (size_t g = 0; g < G; g++)
      if ((p - G)[g] != 0xAA || p[bytes + g] != 0xAA) return false;
    return true;
  };
  auto gt_mid = [&](const std::vector<uint8_t>& gt, uint32_t (&mid)[8]) {
    std::vector<uint32_t> E(144);
    for (int k = 0; k < 12; k++) st_fp(E.data(), 1, 0, 11 - k, fp_to_mont(fp_raw_from_be48(gt.data() + 48 * k)));
    tmask_midstate(mid, [&](int k) { return tmask_coef_soa(E.data(), 1, 0, k); });
  };
  bool match = true;
  // the spans of a packed batch: the prefix offsets of its items, read through the form under test
  auto offsets = [](size_t n, auto len_of) {
    std::vector<uint32_t> o(n + 1, 0);
    for (size_t i = 0; i < n; i++) o[i + 1] = o[i] + (uint32_t)len_of(i);
    return o;
  };
  auto all_dwords = [](const std::vector<uint32_t>& o) {
    uint32_t low = 0;
    for (uint32_t v : o) low |= v;
    return (low & 3) == 0;
  };
  int dword_forms = 0;

  printf("{\"mlen\": %lu, \"reduce\": [", mlen);
  for (size_t i = 0; i < reds.size(); i++) {
    uint32_t be[12], k[8];
    for (int w = 0; w < 12; w++) be[w] = load_be32(reds[i].data() + 4 * w);
    const bool nz = tauth_reduce384(be, k);
    uint8_t kb[32];
    tauth_scalar_bytes(kb, k);
    printf("%s{\"k\": \"%s\", \"nonzero\": %s}", i ? ", " : "", hex_of(kb, 32).c_str(), nz ? "true" : "false");
  }

  // ---- the sealing side: derive, then the tail from the given K
  struct SealOut {
    std::vector<uint8_t> k, v, w;
    std::vector<int> ok;
    bool operator==(const SealOut& o) const { return k == o.k && v == o.v && w == o.w && ok == o.ok; }
  };
  const size_t ns = seals.size();
  const std::vector<uint32_t> soffs = offsets(ns, [&](size_t i) { return seals[i].msg.size(); });
  const size_t sbytes = soffs[ns];
  auto s_off = [&](size_t i) { return ragged ? tauth_span_ragged{soffs.data()}.off(i) : tauth_span_uniform{(uint32_t)mlen}.off(i); };
  auto s_len = [&](size_t i) { return ragged ? tauth_span_ragged{soffs.data()}.len(i) : tauth_span_uniform{(uint32_t)mlen}.len(i); };
  auto run_seal = [&](bool words, bool in_place) {
    SealOut o;
    std::vector<uint32_t> bv, bw, bm;
    uint8_t* V = guarded(bv, 32 * ns);
    uint8_t* W = guarded(bw, sbytes);
    bm.assign(sbytes / 4 + 2, 0);
    uint8_t* M = in_place ? W : (uint8_t*)bm.data();
    for (size_t i = 0; i < ns; i++) memcpy(M + s_off(i), seals[i].msg.data(), s_len(i));
    o.k.resize(32 * ns);
    for (size_t i = 0; i < ns; i++) {
      uint32_t seed[8], k[8], mid[8] = {0};
      tauth_seed_words(seed, seals[i].seed.data());
      bool sealed = words ? tauth_derive<true>(seed, M + s_off(i), s_len(i), k)
                          : tauth_derive<false>(seed, M + s_off(i), s_len(i), k);
      tauth_scalar_bytes(o.k.data() + 32 * i, k);
      uint32_t k2[8];
      sealed = tseal_scalar(o.k.data() + 32 * i, k2);  // what k_tseal_u reads back from the staging row
      for (int w = 0; w < 8; w++) match &= k2[w] == k[w];
      o.ok.push_back(sealed);
      if (sealed) gt_mid(seals[i].gt, mid);
      if (words)
        tauth_seal_tail<true>(mid, sealed, seed, M + s_off(i), s_len(i), V + 32 * i, W + s_off(i));
      else
        tauth_seal_tail<false>(mid, sealed, seed, M + s_off(i), s_len(i), V + 32 * i, W + s_off(i));
    }
    if (!guards_ok(V, 32 * ns) || !guards_ok(W, sbytes)) match = false;
    o.v.assign(V, V + 32 * ns);
    o.w.assign(W, W + sbytes);
    return o;
  };
  printf("], \"seal\": [");
  if (ns) {
    const SealOut o = run_seal(false, false);
    match &= run_seal(false, true) == o;
    if (all_dwords(soffs)) {
      match &= run_seal(true, false) == o && run_seal(true, true) == o;
      dword_forms++;
    }
    for (size_t i = 0; i < ns; i++)
      printf("%s{\"k\": \"%s\", \"ok\": %d, \"v\": \"%s\", \"w\": \"%s\"}", i ? ", " : "", hex_of(o.k.data() + 32 * i, 32).c_str(),
             o.ok[i], hex_of(o.v.data() + 32 * i, 32).c_str(), hex_of(o.w.data() + s_off(i), s_len(i)).c_str());
  }

  // ---- the opening side
  static g1a T1[TSEAL_WINDOWS * TSEAL_ENTRIES];
  const size_t no = opens.size();
  if (no)
    for (int w = 0; w < TSEAL_WINDOWS; w++) tseal_g1_row(w, [&](int j, const g1a& p) { T1[tseal_entry(w, j)] = p; });
  unsigned long long n_check = 0;
  struct OpenOut {
    std::vector<uint8_t> msg, cls;
    bool operator==(const OpenOut& o) const { return msg == o.msg && cls == o.cls; }
  };
  const std::vector<uint32_t> ooffs = offsets(no, [&](size_t i) { return opens[i].w.size(); });
  const size_t obytes = ooffs[no];
  auto o_off = [&](size_t i) { return ragged ? tauth_span_ragged{ooffs.data()}.off(i) : tauth_span_uniform{(uint32_t)mlen}.off(i); };
  auto o_len = [&](size_t i) { return ragged ? tauth_span_ragged{ooffs.data()}.len(i) : tauth_span_uniform{(uint32_t)mlen}.len(i); };
  auto run_open = [&](bool words, bool in_place) {
    OpenOut o;
    std::vector<uint32_t> bo, bw, bv;
    uint8_t* out = guarded(bo, obytes);
    bw.assign(obytes / 4 + 2, 0);
    bv.assign(8 * no + 2, 0);
    uint8_t* W = in_place ? out : (uint8_t*)bw.data();
    uint8_t* V = (uint8_t*)bv.data();
    for (size_t i = 0; i < no; i++) {
      memcpy(W + o_off(i), opens[i].w.data(), o_len(i));
      memcpy(V + 32 * i, opens[i].v.data(), 32);
    }
    for (size_t i = 0; i < no; i++) {
      g1a U;
      bool uinf = false;
      uint8_t cls = g1_decompress(opens[i].u.data(), U, uinf);
      if (cls == REJ_OK && opens[i].cls) cls = (uint8_t)opens[i].cls;
      if (cls != REJ_OK) {
        const uint32_t zero[8] = {0};
        for (uint32_t j = 0; 32 * j < o_len(i); j++) {
          if (words)
            tauth_store_piece<true>(out + o_off(i), j, tauth_piece_len(o_len(i), j), zero, true);
          else
            tauth_store_piece<false>(out + o_off(i), j, tauth_piece_len(o_len(i), j), zero, true);
        }
      } else {
        uint32_t mid[8];
        gt_mid(opens[i].gt, mid);
        const unsigned long long c0 = g_fp_mul_count;
        auto entry = [&](int w, int j) { return T1[tseal_entry(w, j)]; };
        auto ucoord = [&](int c) { return c ? U.y : U.x; };
        cls = words ? tauth_open_tail<true>(mid, V + 32 * i, W + o_off(i), o_len(i), ucoord, uinf, entry, out + o_off(i))
                    : tauth_open_tail<false>(mid, V + 32 * i, W + o_off(i), o_len(i), ucoord, uinf, entry, out + o_off(i));
        if (cls == REJ_OK) n_check = g_fp_mul_count - c0;
      }
      o.cls.push_back(cls);
    }
    if (!guards_ok(out, obytes)) match = false;
    o.msg.assign(out, out + obytes);
    return o;
  };
  printf("], \"open\": [");
  if (no) {
    const OpenOut o = run_open(false, false);
    match &= run_open(false, true) == o;
    if (all_dwords(ooffs)) {
      match &= run_open(true, false) == o && run_open(true, true) == o;
      dword_forms++;
    }
    for (size_t i = 0; i < no; i++)
      printf("%s{\"cls\": %d, \"msg\": \"%s\"}", i ? ", " : "", (int)o.cls[i], hex_of(o.msg.data() + o_off(i), o_len(i)).c_str());
  }
  if (ragged)
    printf("], \"fp_mul_open\": %llu, \"dword_forms\": %d, \"forms_match\": %s}\n", n_check, dword_forms, match ? "true" : "false");
  else
    printf("], \"fp_mul_open\": %llu, \"forms_match\": %s}\n", n_check, match ? "true" : "false");
  return match ? 0 : 1;
}

// tseal <pk48hex> <round>: the timelock sealing (drand_amd/csrc/tseal.h) as the device runs it -- the base
// B = e(pk, H(MessageV2(round)))^3 through the opening's own forms (hash, prepared line table, f pass,
// final exponentiation), the tables T1 (multiples of G1) and T2 (powers of B), then per scalar (stdin, 32
// bytes big-endian in hex per line) U = k G1 and K = B^k by table walks. "tables_match": every T1 entry
// equals jac_mul_scalar of the generator and every T2 entry a plain power of B (generic Fp12 squares and
// products). "u_plain" / "k_plain": the same outputs by a second implementation, jac_mul_scalar and 255
// cyclotomic squarings with multiplies. A scalar == 0 (mod r) is refused: ok 0 and zero bytes. Prints
// the Fp products of the base and the tables (once each) and of the last sealed item's four forms.
static int cmd_tseal(const char* pkhex, unsigned long long round) {
  const auto pkb = unhex(pkhex);
  if (pkb.size() != 48) return 2;
  g1a P;
  bool pinf;
  const uint8_t pcls = g1_decompress(pkb.data(), P, pinf);
  if (pcls != REJ_OK || pinf) {
    printf("{\"pk_class\": %d, \"pk_inf\": %s}\n", pcls, pinf ? "true" : "false");
    return 1;
  }
  unsigned long long c0 = g_fp_mul_count;
  fp12 B;
  {
    uint32_t msg[8];
    drand_message_v2(msg, round);
    const g2a h = g2_to_aff(hash_to_g2(msg));
    static fp2 lines[MILLER_STEPS][3];
    tlock_prepare(h, [&](int step, int c, const fp2& v) { lines[step][c] = v; });
    B = final_exponentiation(tlock_f([&](int step, int c) { return lines[step][c]; }, P.x, P.y));
  }
  const unsigned long long n_base = g_fp_mul_count - c0;

  static g1a T1[TSEAL_WINDOWS * TSEAL_ENTRIES];
  static fp12 T2[TSEAL_WINDOWS * TSEAL_ENTRIES];
  c0 = g_fp_mul_count;
  for (int w = 0; w < TSEAL_WINDOWS; w++) tseal_g1_row(w, [&](int j, const g1a& p) { T1[tseal_entry(w, j)] = p; });
  const unsigned long long n_t1 = g_fp_mul_count - c0;
  c0 = g_fp_mul_count;
  tseal_gt_chain(B, [&](int w, const fp12& v) { T2[tseal_entry(w, 1)] = v; });
  for (int w = 0; w < TSEAL_WINDOWS; w++)
    tseal_gt_row(T2[tseal_entry(w, 1)], [&](int j, const fp12& v) { T2[tseal_entry(w, j)] = v; });
  const unsigned long long n_t2 = g_fp_mul_count - c0;

  const g1j G = jac_from_aff(g1a{fp_load_const(G1_GEN_X), fp_load_const(G1_GEN_Y)});
  bool tables_match = true;
  {
    fp12 pw = B;  // B^(16^w) by generic squares
    for (int w = 0; w < TSEAL_WINDOWS; w++) {
      if (w)
        for (int k = 0; k < 4; k++) pw = fp12_sqr(pw);
      for (int j = 1; j <= TSEAL_ENTRIES; j++) {
        uint32_t e[8] = {0};
        e[w >> 3] = (uint32_t)j << ((w & 7) * 4);
        tables_match &= jac_eq(jac_from_aff(T1[tseal_entry(w, j)]), jac_mul_scalar(G, e));
        fp12 x = fp12_one();  // pw^j, square and multiply over j's four bits
        for (int b = 3; b >= 0; b--) {
          x = fp12_sqr(x);
          if ((j >> b) & 1) x = fp12_mul(x, pw);
        }
        tables_match &= fp12_eq(T2[tseal_entry(w, j)], x);
      }
    }
  }

  std::vector<std::string> us, ks, up, kp;
  std::vector<int> oks;
  unsigned long long n_uf = 0, n_gf = 0, n_up = 0, n_gp = 0;
  static char line_buf[256];
  while (fgets(line_buf, sizeof line_buf, stdin)) {
    char* save = nullptr;
    const char* sh = strtok_r(line_buf, " \n", &save);
    if (!sh) continue;
    const auto sb = unhex(sh);
    if (sb.size() != TSEAL_SCALAR_LEN) return 2;
    uint32_t k[8];
    const bool sealed = tseal_scalar(sb.data(), k);
    oks.push_back(sealed);
    uint8_t u[48] = {0}, e[TLOCK_GT_LEN] = {0}, u2[48] = {0}, e2[TLOCK_GT_LEN] = {0};
    if (sealed) {
      c0 = g_fp_mul_count;
      g1_compress(u, tseal_u(k, [&](int w, int j) { return T1[tseal_entry(w, j)]; }));
      n_uf = g_fp_mul_count - c0;
      c0 = g_fp_mul_count;
      const fp12 K = tseal_gt(k, [&](int w, int j, int h) {
        const fp12& t = T2[tseal_entry(w, j)];
        return h ? t.c1 : t.c0;
      });
      n_gf = g_fp_mul_count - c0;
      tlock_encode(e, K);
      // the plain way
      c0 = g_fp_mul_count;
      g1_compress(u2, jac_mul_scalar(G, k));
      n_up = g_fp_mul_count - c0;
      c0 = g_fp_mul_count;
      fp12 acc = (k[7] >> 31) ? B : fp12_one();
      for (int b = 254; b >= 0; b--) {
        acc = fp12_cyclotomic_sqr(acc);
        if ((k[b >> 5] >> (b & 31)) & 1u) acc = fp12_mul(acc, B);
      }
      n_gp = g_fp_mul_count - c0;
      tlock_encode(e2, acc);
    }
    us.push_back(hex_of(u, 48));
    ks.push_back(hex_of(e, TLOCK_GT_LEN));
    up.push_back(hex_of(u2, 48));
    kp.push_back(hex_of(e2, TLOCK_GT_LEN));
  }
  auto list = [](const char* name, const std::vector<std::string>& v) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) printf("%s\"%s\"", i ? ", " : "", v[i].c_str());
    printf("], ");
  };
  printf("{\"tables_match\": %s, \"ok\": [", tables_match ? "true" : "false");
  for (size_t i = 0; i < oks.size(); i++) printf("%s%d", i ? ", " : "", oks[i]);
  printf("], ");
  list("u", us);
  list("k", ks);
  list("u_plain", up);
  list("k_plain", kp);
  printf("\"fp_mul\": {\"base\": %llu, \"g1_table\": %llu, \"gt_table\": %llu, \"u_fixed\": %llu, \"gt_fixed\": %llu,"
         " \"u_plain\": %llu, \"gt_plain\": %llu}}\n", n_base, n_t1, n_t2, n_uf, n_gf, n_up, n_gp);
  return tables_match ? 0 : 1;
}

// tsealr <pk48hex>: the timelock sealing to many rounds (drand_amd/csrc/tsealr.h) as the device runs it.
// Per line of stdin, "round scalarhex" (the round in decimal, 32 bytes big-endian in hex): U = k G1 from
// T1, P = k pk by the walk over the key table TK, H = H(MessageV2(round)), the single-pair lines of
// (P, H), the single-pair f pass over them, the final exponentiation and the Gt encoding. "table_match":
// every TK entry equals jac_mul_scalar of pk. "u_plain" / "k_plain": the same outputs by a second
// implementation, jac_mul_scalar for both points and miller_loop_multi<1> with the register final
// exponentiation. A scalar == 0 (mod r) is refused: ok 0 and zero bytes.
// Prints the Fp products of the key table (once) and of the last sealed item's stages, and beside them
// what the two-pair passes cost for the same item: "lines2" walks a second chain next to (P, H) -- the
// pair (-G1, H) as a stand-in, what a pass with a live second pair pays -- and "f2" is
// miller_f_from_lines with the second pair inactive (its lines 1), which must give the single-pair f
// ("two_pair_match").
static int cmd_tsealr(const char* pkhex) {
  const auto pkb = unhex(pkhex);
  if (pkb.size() != 48) return 2;
  g1a PK;
  bool pinf;
  const uint8_t pcls = g1_decompress(pkb.data(), PK, pinf);
  if (pcls != REJ_OK || pinf) {
    printf("{\"pk_class\": %d, \"pk_inf\": %s}\n", pcls, pinf ? "true" : "false");
    return 1;
  }
  static g1a T1[TSEAL_WINDOWS * TSEAL_ENTRIES], TK[TSEAL_WINDOWS * TSEAL_ENTRIES];
  for (int w = 0; w < TSEAL_WINDOWS; w++) tseal_g1_row(w, [&](int j, const g1a& p) { T1[tseal_entry(w, j)] = p; });
  unsigned long long c0 = g_fp_mul_count;
  for (int w = 0; w < TSEAL_WINDOWS; w++)
    tseal_g1_row_of(PK, w, [&](int j, const g1a& p) { TK[tseal_entry(w, j)] = p; });
  const unsigned long long n_tk = g_fp_mul_count - c0;
  const g1j G = jac_from_aff(g1a{fp_load_const(G1_GEN_X), fp_load_const(G1_GEN_Y)}), PKJ = jac_from_aff(PK);
  bool table_match = true;
  for (int w = 0; w < TSEAL_WINDOWS; w++)
    for (int j = 1; j <= TSEAL_ENTRIES; j++) {
      uint32_t e[8] = {0};
      e[w >> 3] = (uint32_t)j << ((w & 7) * 4);
      table_match &= jac_eq(jac_from_aff(TK[tseal_entry(w, j)]), jac_mul_scalar(PKJ, e));
    }

  std::vector<std::string> us, ks, up, kp;
  std::vector<int> oks;
  bool two_pair_match = true;
  unsigned long long n_u = 0, n_p = 0, n_l1 = 0, n_f1 = 0, n_fexp = 0, n_l2 = 0, n_f2 = 0;
  static char line_buf[256];
  while (fgets(line_buf, sizeof line_buf, stdin)) {
    char* save = nullptr;
    const char* rh = strtok_r(line_buf, " \n", &save);
    const char* sh = rh ? strtok_r(nullptr, " \n", &save) : nullptr;
    if (!rh) continue;
    if (!sh) return 2;
    const unsigned long long round = strtoull(rh, nullptr, 10);
    const auto sb = unhex(sh);
    if (sb.size() != TSEAL_SCALAR_LEN) return 2;
    uint32_t k[8];
    const bool sealed = tseal_scalar(sb.data(), k);
    oks.push_back(sealed);
    uint8_t u[48] = {0}, e[TLOCK_GT_LEN] = {0}, u2[48] = {0}, e2[TLOCK_GT_LEN] = {0};
    if (sealed) {
      c0 = g_fp_mul_count;
      g1_compress(u, tseal_u(k, [&](int w, int j) { return T1[tseal_entry(w, j)]; }));
      n_u = g_fp_mul_count - c0;
      c0 = g_fp_mul_count;
      const g1a P = tsealr_point(k, [&](int w, int j) { return TK[tseal_entry(w, j)]; });
      n_p = g_fp_mul_count - c0;
      uint32_t msg[8];
      drand_message_v2(msg, round);
      const g2a H = g2_to_aff(hash_to_g2(msg));
      auto load_h = [&]() { return H; };
      static fp2 L[MILLER_STEPS][3];
      g2proj T;
      c0 = g_fp_mul_count;
      tsealr_lines(g2proj_reg{T}, load_h, [&](int step, int c, const fp2& v) { L[step][c] = v; },
                   [&]() { return P.x; }, [&]() { return P.y; });
      n_l1 = g_fp_mul_count - c0;
      c0 = g_fp_mul_count;
      const fp12 f = tsealr_f([&](int step, int c) { return L[step][c]; }, [](const fp12& a) { return fp12_sqr(a); });
      n_f1 = g_fp_mul_count - c0;
      c0 = g_fp_mul_count;
      const fp12 K = final_exponentiation(f);
      n_fexp = g_fp_mul_count - c0;
      tlock_encode(e, K);
      // the two-pair passes for the same item
      c0 = g_fp_mul_count;
      g2proj T2;
      tsealr_lines(g2proj_reg{T2}, load_h, [](int, int, const fp2&) {}, []() { return fp_load_const(G1_GEN_X); },
                   []() { return fp_load_const(G1_GEN_NEG_Y); });
      n_l2 = n_l1 + (g_fp_mul_count - c0);
      c0 = g_fp_mul_count;
      const fp12 f2 = miller_f_from_lines(
          [&](int step, int pair) { return pair == 0 ? line{L[step][0], L[step][1], L[step][2]} : line_one(); });
      n_f2 = g_fp_mul_count - c0;
      two_pair_match &= fp12_eq(f, f2);
      // the plain way
      g1_compress(u2, jac_mul_scalar(G, k));
      const g1a Ps[1] = {g1_to_aff(jac_mul_scalar(PKJ, k))};
      const g2a Qs[1] = {H};
      const bool act[1] = {true};
      tlock_encode(e2, final_exponentiation(miller_loop_multi<1>(Ps, Qs, act)));
    }
    us.push_back(hex_of(u, 48));
    ks.push_back(hex_of(e, TLOCK_GT_LEN));
    up.push_back(hex_of(u2, 48));
    kp.push_back(hex_of(e2, TLOCK_GT_LEN));
  }
  auto list = [](const char* name, const std::vector<std::string>& v) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) printf("%s\"%s\"", i ? ", " : "", v[i].c_str());
    printf("], ");
  };
  printf("{\"table_match\": %s, \"two_pair_match\": %s, \"ok\": [", table_match ? "true" : "false",
         two_pair_match ? "true" : "false");
  for (size_t i = 0; i < oks.size(); i++) printf("%s%d", i ? ", " : "", oks[i]);
  printf("], ");
  list("u", us);
  list("k", ks);
  list("u_plain", up);
  list("k_plain", kp);
  printf("\"fp_mul\": {\"key_table\": %llu, \"u_fixed\": %llu, \"p_fixed\": %llu, \"lines1\": %llu, \"f1\": %llu,"
         " \"final_exp\": %llu, \"lines2\": %llu, \"f2\": %llu}}\n", n_tk, n_u, n_p, n_l1, n_f1, n_fexp, n_l2, n_f2);
  return table_match && two_pair_match ? 0 : 1;
}

// tlockr <cap> <dense_min> (<sig96hex> <count>)...: the timelock opening across many rounds
// (drand_amd/csrc/tlockr.h) as the device runs it -- the host's plan of every pass of at most cap items
// (hostlogic.h open_rounds_next_pass), per pass the signatures it touches decoded and prepared into one
// word-major table, then every tile's items through tlockr_f in the tile's form: a uniform tile reads a
// copy of its signature's column (the device's LDS copy), a mixed tile's items read the table itself. Every
// item also runs the other form ("forms_match"). The U values come on stdin, one 48-byte compressed G1
// point in hex per line, in packed order. Prints sig_class per signature, class and e (null where the item
// did not open) per item and the tiles of every pass as [first, len, sig] (sig -1 = mixed).
static int cmd_tlockr(int argc, char** argv) {
  using namespace blsv_detail;
  if (argc < 2 || (argc - 2) % 2) return 2;
  const size_t cap = strtoull(argv[0], nullptr, 10), dense_min = strtoull(argv[1], nullptr, 10);
  const size_t m = (size_t)(argc - 2) / 2;
  if (!cap) return 2;
  std::vector<std::vector<uint8_t>> sigs;
  std::vector<uint64_t> counts;
  for (size_t j = 0; j < m; j++) {
    sigs.push_back(unhex(argv[2 + 2 * j]));
    if (sigs.back().size() != 96) return 2;
    counts.push_back(strtoull(argv[3 + 2 * j], nullptr, 10));
  }
  std::vector<std::vector<uint8_t>> us;
  static char line_buf[256];
  while (fgets(line_buf, sizeof line_buf, stdin)) {
    char* save = nullptr;
    const char* uh = strtok_r(line_buf, " \n", &save);
    if (!uh) continue;
    us.push_back(unhex(uh));
    if (us.back().size() != 48) return 2;
  }
  const size_t n = us.size();
  if (!open_rounds_fits(counts.data(), m, n)) {
    printf("{\"einval\": true}\n");
    return 1;
  }
  std::vector<int> sig_class(m), classes(n, 0);
  for (size_t j = 0; j < m; j++) {
    g2a Q;
    bool qinf;
    sig_class[j] = g2_decompress(sigs[j].data(), Q, qinf, true);
  }
  std::vector<std::string> enc(n);
  bool forms_match = true;
  std::string tiles_json;
  TlockRoundsCursor cur;
  TlockRoundsPass p;
  while (open_rounds_next_pass(counts.data(), m, cap, dense_min, cur, p)) {
    const size_t M = p.sig_j.size();
    std::vector<g2a> Q(M);
    std::vector<uint8_t> qinf(M), qcls(M);
    std::vector<uint32_t> tab((size_t)TLOCK_TAB_WORDS * M, 0xdeadbeefu);
    for (size_t j = 0; j < M; j++) {
      bool inf;
      qcls[j] = g2_decompress(sigs[p.sig_j[j]].data(), Q[j], inf, true);
      qinf[j] = inf;
      if (qcls[j] == REJ_OK && !inf) tlockr_prepare(Q[j], [&](int w, uint32_t v) { tab[tlockr_tab_at(w, M, j)] = v; });
    }
    tiles_json += std::string(tiles_json.empty() ? "" : ", ") + "[";
    for (size_t t = 0; t < p.tiles.size(); t++) {
      const TlockTile& tl = p.tiles[t];
      const bool mixed = tl.sig == kTlockTileMixed;
      tiles_json += std::string(t ? ", " : "") + "[" + std::to_string(tl.first) + ", " + std::to_string(tl.len) + ", " +
                    (mixed ? std::string("-1") : std::to_string(tl.sig)) + "]";
      std::vector<uint32_t> col(TLOCK_TAB_WORDS);  // a uniform tile's copy of its column
      if (!mixed)
        for (int w = 0; w < TLOCK_TAB_WORDS; w++) col[w] = tab[tlockr_tab_at(w, M, tl.sig)];
      for (uint32_t lane = 0; lane < tl.len; lane++) {
        const size_t i = tl.first + lane, gi = p.base + i;
        const size_t j = mixed ? p.sig_of[i] : tl.sig;
        g1a U;
        bool uinf;
        classes[gi] = g1_decompress(us[gi].data(), U, uinf);
        if (classes[gi] != REJ_OK) continue;
        if (qcls[j] != REJ_OK) {
          classes[gi] = REJ_TLOCK_SIG;
          continue;
        }
        fp12 f = fp12_one();
        if (!uinf && !qinf[j]) {
          fp2 parked[3];
          auto from_table = [&](int step, int c) {
            const size_t o = tlockr_tab_at(tlockr_coef_word(step, c), M, j);
            fp2 v;
            for (int k = 0; k < 12; k++) {
              v.c0.l[k] = tab[o + (size_t)k * M];
              v.c1.l[k] = tab[o + (size_t)(12 + k) * M];
            }
            return v;
          };
          std::vector<uint32_t> own;  // the other form of a mixed tile's item: a copy of its own column
          if (mixed) {
            own.resize(TLOCK_TAB_WORDS);
            for (int w = 0; w < TLOCK_TAB_WORDS; w++) own[w] = tab[tlockr_tab_at(w, M, j)];
          }
          const std::vector<uint32_t>& column = mixed ? own : col;
          auto from_column = [&](int step, int c) {
            const int o = tlockr_coef_word(step, c);
            fp2 v;
            for (int k = 0; k < 12; k++) {
              v.c0.l[k] = column[o + k];
              v.c1.l[k] = column[o + 12 + k];
            }
            return v;
          };
          auto ucoord = [&](int c) { return c == 0 ? U.x : U.y; };
          auto park = [&](int c, const fp2& v) { parked[c] = v; };
          auto get = [&](int c) { return parked[c]; };
          auto sqr = [](const fp12& a) { return fp12_sqr(a); };
          const fp12 fm = tlockr_f(from_table, ucoord, park, get, sqr);
          const fp12 fu = tlockr_f(from_column, ucoord, park, get, sqr);
          forms_match &= fp12_eq(fm, fu);
          f = mixed ? fm : fu;
        }
        uint8_t out[TLOCK_GT_LEN];
        tlock_encode(out, final_exponentiation(f));
        enc[gi] = hex_of(out, TLOCK_GT_LEN);
      }
    }
    tiles_json += "]";
  }
  printf("{\"sig_class\": [");
  for (size_t j = 0; j < m; j++) printf("%s%d", j ? ", " : "", sig_class[j]);
  printf("], \"forms_match\": %s, \"class\": [", forms_match ? "true" : "false");
  for (size_t i = 0; i < n; i++) printf("%s%d", i ? ", " : "", classes[i]);
  printf("], \"e\": [");
  for (size_t i = 0; i < n; i++) {
    if (enc[i].empty())
      printf("%snull", i ? ", " : "");
    else
      printf("%s\"%s\"", i ? ", " : "", enc[i].c_str());
  }
  printf("], \"tiles\": [%s]}\n", tiles_json.c_str());
  return forms_match ? 0 : 1;
}

// The batch path's subgroup check of a decoded sigma (not infinity): the call-free line steps of
// k_miller_lines over |x|'s bits (the lines themselves dropped; they do not depend on the check) and
// pairing.h miller_t_in_subgroup on the T they leave. close_muls: the Fp products of that closing test.
static bool lines_subgroup_check(const g2a& Q, unsigned long long* close_muls = nullptr) {
  g2proj T = {Q.x, Q.y, fp2_one()};
  const g2proj_reg ts{T};
  auto put = [](int, const fp2&) {};
  auto xp = []() { return fp_load_const(G1_GEN_X); };
  auto yp = []() { return fp_load_const(G1_GEN_NEG_Y); };
  auto q = [&]() { return Q; };
  for (int b = 62; b >= 0; b--) {
    miller_dbl_step_ts(ts, put, xp, yp);
    if ((BLS_X_ABS >> b) & 1ull) miller_add_step_ts(ts, q, put, xp, yp);
  }
  const unsigned long long c0 = g_fp_mul_count;
  const bool in = miller_t_in_subgroup(ts, q);
  if (close_muls) *close_muls = g_fp_mul_count - c0;
  return in;
}

// subgroup: one 96-byte compressed G2 point in hex per line on stdin. Prints per line
// "<batch> <ref>": the class the batch path gives (g2_decompress without its subgroup check, then
// lines_subgroup_check) beside the class of g2_decompress with the psi check of curve.h.
static int cmd_subgroup() {
  static char line[512];
  int differ = 0;
  while (fgets(line, sizeof line, stdin)) {
    char* save = nullptr;
    const char* sh = strtok_r(line, " \n", &save);
    if (!sh) continue;
    const auto sig = unhex(sh);
    if (sig.size() != 96) return 2;
    g2a s, r;
    bool sinf, rinf;
    uint8_t cls = g2_decompress(sig.data(), s, sinf, false);
    if (cls == REJ_OK && !sinf && !lines_subgroup_check(s)) cls = REJ_NOT_IN_SUBGROUP;
    const uint8_t ref = g2_decompress(sig.data(), r, rinf, true);
    printf("%d %d\n", (int)cls, (int)ref);
    differ |= cls != ref;
  }
  return differ;
}

// fexp: the final exponentiation's staged forms (drand_amd/csrc/pairing.h) on Fp12 values read from stdin, one
// per line: twelve Fp coefficients as hex integers below p, in the order (c_k.c0, c_k.c1) of the w-power
// k = 0 .. 5. Per line: the value e = final_exponentiation(f); g (easy part), the handed-out g3, c and
// fp12_frob4(c), and whether that equals fp12_frob2(c) fp12_conj(c); the verdict of fexp_step4_is_one with the
// compared operands (r's factors t and g3, and c) given in [0, p) and in [p, 2p), all four pairings; the
// Fp products of the value and of the verdict form.
static fp2* f12_slot(fp12& f, int k) {
  fp2* s[6] = {&f.c0.c0, &f.c1.c0, &f.c0.c1, &f.c1.c1, &f.c0.c2, &f.c1.c2};
  return s[k];
}
static fp fp_rep(const fp& a, bool hi) {  // the same value in [0, p) or in [p, 2p)
  fp r = fp_canon(a);
  unsigned c = 0;
  if (hi)
    for (int i = 0; i < 12; i++) r.l[i] = __builtin_addc(r.l[i], P_RAW[i], c, &c);
  return r;
}
static fp12 f12_rep(fp12 f, bool hi) {
  for (int k = 0; k < 6; k++) *f12_slot(f, k) = fp2{fp_rep(f12_slot(f, k)->c0, hi), fp_rep(f12_slot(f, k)->c1, hi)};
  return f;
}
static void print_f12(const char* name, fp12 f) {
  printf("\"%s\": [", name);
  for (int k = 0; k < 6; k++) {
    printf("%s", k ? ", " : "");
    print_fp(f12_slot(f, k)->c0);
    printf(", ");
    print_fp(f12_slot(f, k)->c1);
  }
  printf("]");
}
static int cmd_fexp() {
  static char line[12 * 100 + 8];
  while (fgets(line, sizeof line, stdin)) {
    char* save = nullptr;
    fp12 f;
    int got = 0;
    for (char* tok = strtok_r(line, " \n", &save); tok && got < 12; tok = strtok_r(nullptr, " \n", &save), got++) {
      char buf[97];
      const size_t len = strlen(tok);
      if (len > 96) return 2;
      memset(buf, '0', 96);
      memcpy(buf + 96 - len, tok, len);
      buf[96] = 0;
      fp raw;
      for (int w = 0; w < 12; w++) {
        char b[9];
        memcpy(b, buf + 8 * (11 - w), 8);
        b[8] = 0;
        raw.l[w] = (uint32_t)strtoul(b, nullptr, 16);
      }
      fp2* slot = f12_slot(f, got / 2);
      (got % 2 ? slot->c1 : slot->c0) = fp_to_mont(raw);
    }
    if (!got) continue;
    if (got != 12) return 2;
    unsigned long long c0 = g_fp_mul_count;
    const fp12 e = final_exponentiation(f);
    const unsigned long long n_value = g_fp_mul_count - c0;
    c0 = g_fp_mul_count;
    const bool one = final_exponentiation_is_one(f);
    const unsigned long long n_verdict = g_fp_mul_count - c0;
    const fexp_staged s = fexp_stage_to_t(f);
    const fp12 f4 = fp12_frob4(s.c);
    printf("{");
    print_f12("e", e);
    printf(", ");
    print_f12("g", s.g);
    printf(", ");
    print_f12("g3", s.g3);
    printf(", ");
    print_f12("c", s.c);
    printf(", ");
    print_f12("frob4c", f4);
    printf(", \"frob4_is_frob2_conj\": %s, \"is_one\": %s, \"verdict\": [",
           fp12_eq(f4, fp12_mul(fp12_frob2(s.c), fp12_conj(s.c))) ? "true" : "false", one ? "true" : "false");
    for (int v = 0; v < 4; v++) {
      const fp12 t = f12_rep(s.t, v & 1), g3 = f12_rep(s.g3, v & 1), c = f12_rep(s.c, (v & 2) != 0);
      printf("%s%s", v ? ", " : "", fexp_step4_is_one([&]() { return t; }, [&]() { return c; }, [&]() { return g3; }) ? "true" : "false");
    }
    printf("], \"fp_mul\": {\"value\": %llu, \"verdict\": %llu}}\n", n_value, n_verdict);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "fexp")) return cmd_fexp();
  if (argc == 2 && !strcmp(argv[1], "subgroup")) return cmd_subgroup();
  if (argc == 3 && !strcmp(argv[1], "tlock")) return cmd_tlock(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "tmask")) return cmd_tmask();
  if (argc == 2 && !strcmp(argv[1], "tauth")) return cmd_tauth(false);
  if (argc == 2 && !strcmp(argv[1], "tauthv")) return cmd_tauth(true);
  if (argc == 4 && !strcmp(argv[1], "tseal")) return cmd_tseal(argv[2], strtoull(argv[3], nullptr, 10));
  if (argc == 3 && !strcmp(argv[1], "tsealr")) return cmd_tsealr(argv[2]);
  if (argc >= 4 && !strcmp(argv[1], "tlockr")) return cmd_tlockr(argc - 2, argv + 2);
  if (argc == 4 && !strcmp(argv[1], "rlc")) return cmd_rlc(argv[2], strtoul(argv[3], nullptr, 10));
  if (argc >= 2 && !strcmp(argv[1], "ops")) return cmd_ops(argc == 3 && !strcmp(argv[2], "list"));
  if (argc == 3 && !strcmp(argv[1], "hash")) return cmd_hash(argv[2]);
  if (argc == 3 && !strcmp(argv[1], "powfuzz")) return cmd_powfuzz(strtoul(argv[2], nullptr, 10));
  if (argc == 3 && !strcmp(argv[1], "invfuzz")) return cmd_invfuzz(strtoul(argv[2], nullptr, 10));
  if (argc == 3 && !strcmp(argv[1], "addfuzz")) return cmd_addfuzz(strtoul(argv[2], nullptr, 10));
  if (argc == 3 && !strcmp(argv[1], "linfuzz")) return cmd_linfuzz(strtoul(argv[2], nullptr, 10));
  if (argc == 3 && !strcmp(argv[1], "f6fuzz")) return cmd_f6fuzz(strtoul(argv[2], nullptr, 10));
  if (argc == 3 && !strcmp(argv[1], "sq6fuzz")) return cmd_sq6fuzz(strtoul(argv[2], nullptr, 10));
  if (argc != 5) {
    fprintf(stderr, "usage: %s pk48hex round prevhex|- sig96hex   (prev '-' = unchained V2)\n       %s hash msghex\n"
            "       %s tlock sig96hex   (one compressed U in hex per line on stdin)\n"
            "       %s subgroup   (one compressed G2 point in hex per line on stdin)\n"
            "       %s tseal pk48hex round   (one 32-byte scalar in hex per line on stdin)\n"
            "       %s tsealr pk48hex   (one \"round scalarhex\" per line on stdin)\n"
            "       %s tlockr cap dense_min (sig96hex count)...   (one compressed U in hex per line on stdin)\n"
            "       %s fexp   (one Fp12 per line on stdin: twelve hex coefficients below p)\n",
            argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0]);
    return 2;
  }
  auto pk = unhex(argv[1]);
  unsigned long long round = strtoull(argv[2], nullptr, 10);
  auto prev = unhex(argv[3]);
  auto sig = unhex(argv[4]);
  unsigned long long c0;

  // group setup (once per chain, not per beacon)
  g1a P;
  bool pinf;
  if (g1_decompress(pk.data(), P, pinf) != REJ_OK) return 3;

  c0 = g_fp_mul_count;
  uint32_t msg[8];
  if (!strcmp(argv[3], "-"))
    drand_message_v2(msg, round);
  else
    drand_message(msg, prev.data(), (int)prev.size(), round);
  g2j h = hash_to_g2(msg);
  g2a ha = g2_to_aff(h);
  unsigned long long n_hash = g_fp_mul_count - c0;

  c0 = g_fp_mul_count;
  g2a s;
  bool sinf;
  // the batch path: decoding alone; the subgroup check is closed on the Miller lines' own [|x|]sigma
  // (k_miller_lines<true>), so its walk costs nothing beyond the closing test, counted under Miller
  uint8_t cls = g2_decompress(sig.data(), s, sinf, false);
  unsigned long long n_decomp = g_fp_mul_count - c0;
  unsigned long long n_close = 0;
  if (cls == REJ_OK && !sinf && !lines_subgroup_check(s, &n_close)) cls = REJ_NOT_IN_SUBGROUP;
  if (cls) {
    printf("{\"verified\": false, \"class\": %d}\n", cls);
    return 1;
  }

  c0 = g_fp_mul_count;
  g1a Ps[2] = {P, {fp_load_const(G1_GEN_X), fp_load_const(G1_GEN_NEG_Y)}};
  g2a Qs[2] = {ha, s};
  bool act[2] = {true, true};
  fp12 f = miller_loop_2(Ps, Qs, act);
  unsigned long long n_miller = g_fp_mul_count - c0;

  // the device's staged form (k_miller_lines + k_miller_f) must give the same f with the same work
  {
    static line lines[MILLER_STEPS][2];
    const unsigned long long s0 = g_fp_mul_count;
    for (int k = 0; k < 2; k++)
      miller_lines(Ps[k], [&]() { return Qs[k]; }, [&](int step, const line& l) { lines[step][k] = l; });
    fp12 fs = miller_f_from_lines([&](int step, int k) { return lines[step][k]; });
    if (!fp12_eq(fs, f) || g_fp_mul_count - s0 != n_miller) {
      printf("{\"verified\": false, \"staged_miller_mismatch\": true}\n");
      return 1;
    }
  }

  // the device's hard part (Granger-Scott squares on three lanes, k_fexp.hip) in register form
  c0 = g_fp_mul_count;
  // "final_exp" counts the value e, as every caller of final_exponentiation pays it (the timelock paths
  // capture it); a verification runs the verdict form, which compares without forming e and saves the
  // last Fp12 product: "final_exp_verdict_fp_mul". The two forms must agree.
  const fp12 fe = final_exponentiation(f);
  unsigned long long n_fexp = g_fp_mul_count - c0;
  c0 = g_fp_mul_count;
  bool ok = final_exponentiation_is_one(f);
  unsigned long long n_verdict = g_fp_mul_count - c0;
  if (ok != fp12_is_one(fe)) {
    printf("{\"verified\": false, \"verdict_form_mismatch\": true}\n");
    return 1;
  }

  printf("{\"verified\": %s, \"fp_mul\": {\"hash\": %llu, \"decompress\": %llu, \"miller\": %llu, \"final_exp\": %llu},"
         " \"final_exp_verdict_fp_mul\": %llu, \"limb_products_per_fp_mul\": 288}\n",
         ok ? "true" : "false", n_hash, n_decomp, n_miller + n_close, n_fexp, n_verdict);
  return ok ? 0 : 1;
}
