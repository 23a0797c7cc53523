// Host build of the latency engine (drand_amd/csrc/w*.h, -DWV_HOST): the same source as the device
// kernels, with wv.h emulating the 64 lanes, so tests/test_wv_host.py can check every layer against
// Python integers and the golden vectors on the CPU.
//
// usage: wvtest field   < lines "a0 a1 b0 b1" (hex, raw values < p)  -> one line of results each
//        wvtest inv     < lines "a" (hex, raw < p)                    -> raw a^-1 in both halves (lane GCD)
//        wvtest teamadd < lines "sig96 case"                          -> ok / bad (team G2 addition)
//        wvtest verify  < lines "pk48 msg sig96" (hex)                -> reject class per line
//        wvtest hash    < lines "msg" (hex)                            -> affine H(msg) raw hex
//        wvtest pair    < lines "px py qx0 qx1 qy0 qy1" (affine raw)  -> Miller loop + final exp (raw)
//        wvtest g1dec   < lines "u48" (hex)                            -> "class inf x y" (affine raw hex)
//        wvtest topen   < lines "sig96 u48" (hex)                      -> sigma's class, the item's class, 576 bytes
//        wvtest ttopen  < lines "sig96 u48", or "sig96 -"              -> the same by the eight-wave team
//        wvtest tscalar < lines "k32" (hex)                            -> "ok k-mod-r digits" (tscalar.h)
//        wvtest g1comp  < lines "x y" (affine raw hex), or "inf -"     -> the 48 compressed bytes (wseal.h)
//        wvtest tseal   < lines "pk48 round k32" (round decimal)       -> "ok u48 gt576" (wseal.h seal_item)
//        wvtest ttseal  < lines "pk48 round k32"                       -> the same by the eight-wave team
//        wvtest gtmid   < lines "gt576" (hex)                          -> "h2 ks1" from the lane-form midstate (wauth.h)
//        wvtest awalk   < lines "k" (hex, 0 < k < r)                   -> "u48 -": k G1 by the one-wave walk
//        wvtest tawalk  < lines "k"                                    -> "u48 n": by the eight waves; n partial sums at infinity
//        wvtest aopen   < lines "sig96 u48 v32 w" (hex)                -> sigma's class, the item's class, the message bytes
//        wvtest taopen  < lines "sig96 u48 v32 w"                      -> the same by the eight-wave team
//        wvtest aseal   < lines "pk48 round seed32 msg mode"           -> "ok u48 v32 w" (mode "-", or "k0": the refusal)
//        wvtest taseal  < lines "pk48 round seed32 msg mode"           -> the same by the eight-wave team
//        wvtest sign    < lines "sk32 msg" (hex; msg "-" = empty)      -> the 96 signature bytes (wsign.h sign_item)
//        wvtest tsign   < lines "sk32 msg"                             -> the same by the eight-wave team
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../drand_amd/csrc/wrecover.h"
#include "../drand_amd/csrc/wvteam.h"
#include "../drand_amd/csrc/wseal.h"
#include "../drand_amd/csrc/wauth.h"
#include "../drand_amd/csrc/wsign.h"
#include "../drand_amd/csrc/tseal.h"

#include <thread>

namespace wv {
uint32_t g_host_lds[HOST_MAX_WAVES][LDS_WORDS];
thread_local int g_host_wave = 0;
thread_local unsigned long long g_wv_ops[OPC_N];
uint32_t g_host_blk[BLK_SLOTS * 64 + BLK_WORDS_EXTRA];
double g_host_blk_b[BLK_SLOTS];
std::atomic<uint32_t> g_host_ctr[BLK_CTRS];
}
namespace bls {
unsigned long long g_fp_mul_count = 0;
}

using namespace wv;

static std::vector<uint32_t> hex_to_limbs(const std::string& h) {  // 16 x 25-bit limbs of a hex integer
  std::vector<uint32_t> bits;
  for (int i = (int)h.size() - 1; i >= 0; i--) {
    const char c = h[i];
    const int v = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
    for (int b = 0; b < 4; b++) bits.push_back((v >> b) & 1);
  }
  std::vector<uint32_t> l(16, 0);
  for (size_t i = 0; i < bits.size() && i < 400; i++) l[i / 25] |= bits[i] << (i % 25);
  return l;
}
static std::string limbs_to_hex(const V& x, int h) {  // strict limbs of half h -> hex
  std::vector<int> bits;
  for (int k = 0; k < 16; k++)
    for (int b = 0; b < 25; b++) bits.push_back((x.v[32 * h + k] >> b) & 1);
  std::string s;
  for (int i = 396; i >= 0; i -= 4) {
    int v = 0;
    for (int b = 3; b >= 0; b--) v = v * 2 + (i + b < 400 ? bits[i + b] : 0);
    s += "0123456789abcdef"[v];
  }
  size_t nz = s.find_first_not_of('0');
  return nz == std::string::npos ? "0" : s.substr(nz);
}
static F raw_fp2(const std::string& c0, const std::string& c1) {
  V x = vsplat(0);
  const auto a = hex_to_limbs(c0), b = hex_to_limbs(c1);
  for (int k = 0; k < 16; k++) x.v[k] = a[k], x.v[32 + k] = b[k];
  return mkF(x, 1.0);
}
static F to_mont(const F& raw) { return mulp(raw, cst(WC_R2_DUP)); }
static std::string out_fp2(const F& a) {
  const V r = raw_canon(a);
  return limbs_to_hex(r, 0) + " " + limbs_to_hex(r, 1);
}

static int cmd_field() {
  char a0[200], a1[200], b0[200], b1[200];
  while (scanf("%199s %199s %199s %199s", a0, a1, b0, b1) == 4) {
    wv_init();
    const F a = to_mont(raw_fp2(a0, a1)), b = to_mont(raw_fp2(b0, b1));
    printf("%s", out_fp2(mul2(a, b)).c_str());
    printf(" %s", out_fp2(sqr2(a)).c_str());
    printf(" %s", out_fp2(mulp(a, b)).c_str());
    printf(" %s", out_fp2(add(a, b)).c_str());
    printf(" %s", out_fp2(sub(a, b)).c_str());
    printf(" %s", out_fp2(mul_xi(a)).c_str());
    printf(" %s", out_fp2(conj(a)).c_str());
    printf(" %s", out_fp2(half(a)).c_str());
    printf(" %s", out_fp2(inv2(a)).c_str());
    printf(" %s", out_fp2(norm_dup(a)).c_str());
    printf(" %s", out_fp2(dot(a, b, b, a, a, a)).c_str());
    printf(" %d %d", (int)eq2(a, b), (int)is_zero2(a));
    printf("\n");
  }
  return 0;
}

// inv: "a" (hex, raw < p) -> raw a^-1 (0 -> 0) by the lane GCD, or "nc" if its divsteps did not
// reach b = 1 (the caller would take the exponentiation)
static int cmd_inv() {
  char a0[200];
  while (scanf("%199s", a0) == 1) {
    wv_init();
    const F a = to_mont(raw_fp2(a0, a0));
    F r;
    if (!inv_gcd_lanes(a, r)) {
      printf("nc\n");
      continue;
    }
    const V c = raw_canon(r);
    printf("%s %s\n", limbs_to_hex(c, 0).c_str(), limbs_to_hex(c, 1).c_str());
  }
  return 0;
}

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> b;
  for (size_t i = 0; i + 1 < h.size(); i += 2) b.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return b;
}
static void msg_b0(const std::vector<uint8_t>& m, uint32_t (&b0)[8]) {
  if (m.size() == 32) {
    uint32_t w[8];
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)m[4 * i] << 24 | (uint32_t)m[4 * i + 1] << 16 | (uint32_t)m[4 * i + 2] << 8 | m[4 * i + 3];
    xmd_b0_msg32(w, b0);
  } else {
    bls::xmd_b0_bytes(b0, m.data(), (uint32_t)m.size(), bls::DST);
  }
}

// verify: "pk48 msg sig96" -> reject class (pk that does not decode: -1)
static int cmd_verify() {
  char a[300], b[4000], c[300];
  while (scanf("%299s %3999s %299s", a, b, c) == 3) {
    wv_init();
    const auto pk = unhex(a), msg = unhex(strcmp(b, "-") ? b : ""), sig = unhex(c);
    bls::g1a P;
    bool pinf = false;
    if (bls::g1_decompress(pk.data(), P, pinf) != bls::REJ_OK) {
      printf("-1\n");
      continue;
    }
    uint32_t b0[8];
    msg_b0(msg, b0);
    F sx, sy;
    bool sinf;
    const int cls = sig.size() == 96 ? verify_item(sig.data(), b0, P.x.l, P.y.l, pinf, sx, sy, sinf) : bls::REJ_LENGTH;
    printf("%d\n", cls);
    fflush(stdout);
  }
  return 0;
}

// tverify: as verify, by the eight-wave team (wvteam.h), one host thread per wave
static int cmd_tverify() {
  char a[300], b[4000], c[300];
  while (scanf("%299s %3999s %299s", a, b, c) == 3) {
    const auto pk = unhex(a), msg = unhex(strcmp(b, "-") ? b : ""), sig = unhex(c);
    bls::g1a P;
    bool pinf = false;
    if (bls::g1_decompress(pk.data(), P, pinf) != bls::REJ_OK) {
      printf("-1\n");
      continue;
    }
    if (sig.size() != 96) {
      printf("%d\n", bls::REJ_LENGTH);
      continue;
    }
    uint32_t b0[8];
    msg_b0(msg, b0);
    for (auto& ctr : g_host_ctr) ctr.store(0);
    int cls[TEAM_WAVES];
    std::thread th[TEAM_WAVES];
    for (int w = 0; w < TEAM_WAVES; w++)
      th[w] = std::thread([&, w]() {
        g_host_wave = w;
        wv_init();
        F sx, sy;
        bool sinf = false;
        cls[w] = verify_team(sig.data(), b0, P.x.l, P.y.l, pinf, sx, sy, sinf);
      });
    for (auto& t : th) t.join();
    for (int w = 1; w < TEAM_WAVES; w++)
      if (cls[w] != cls[0]) fprintf(stderr, "waves disagree: %d vs %d\n", cls[w], cls[0]), abort();
    printf("%d\n", cls[0]);
    fflush(stdout);
  }
  return 0;
}

// tverify_pre: as tverify, through the fused round's two launches (wvteam.h team_hash_key, then
// verify_team_pre on the signature's affine point). The point is decoded by one wave and handed over
// the way k_lat_recover_sum hands over the interpolated sum: Jacobian (x z^2, y z^3, z) with z = x + 1,
// back to affine by g2_to_affine. Lines whose signature does not decode print its class (the
// speculative path never sees such a signature: its shares all verified).
static int cmd_tverify_pre() {
  char a[300], b[4000], c[300];
  static uint32_t hbuf[HOUT_WORDS], sbuf[SAFF_WORDS];
  while (scanf("%299s %3999s %299s", a, b, c) == 3) {
    const auto pk = unhex(a), msg = unhex(strcmp(b, "-") ? b : ""), sig = unhex(c);
    bls::g1a P;
    bool pinf = false;
    if (bls::g1_decompress(pk.data(), P, pinf) != bls::REJ_OK) {
      printf("-1\n");
      continue;
    }
    if (sig.size() != 96) {
      printf("%d\n", bls::REJ_LENGTH);
      continue;
    }
    uint32_t b0[8];
    msg_b0(msg, b0);
    g_host_wave = 0;
    wv_init();
    F x, y;
    bool sinf = false;
    const uint8_t dc = g2_decompress(sig.data(), x, y, sinf);
    if (dc != bls::REJ_OK) {
      printf("%d\n", dc);
      continue;
    }
    memset(sbuf, 0, sizeof sbuf);
    if (!sinf) {
      const F z = add(x, cst(WC_ONE2)), z2 = sqr2(z);
      F ax, ay;
      g2_to_affine({dot(x, z2), dot(y, dot(z2, z)), z}, ax, ay);
      gst_F(sbuf, ax);
      gst_F(sbuf + 64, ay);
    }
    gst_flag(sbuf + 128, sinf);
    memset(hbuf, 0, sizeof hbuf);
    for (int pass = 0; pass < 2; pass++) {
      for (auto& ctr : g_host_ctr) ctr.store(0);
      int cls[TEAM_WAVES];
      std::thread th[TEAM_WAVES];
      for (int w = 0; w < TEAM_WAVES; w++)
        th[w] = std::thread([&, w]() {
          g_host_wave = w;
          wv_init();
          if (pass == 0) team_hash_key(b0, P.x.l, P.y.l, pinf, hbuf);
          else cls[w] = verify_team_pre(hbuf, sbuf);
        });
      for (auto& t : th) t.join();
      if (pass == 0) continue;
      for (int w = 1; w < TEAM_WAVES; w++)
        if (cls[w] != cls[0]) fprintf(stderr, "waves disagree: %d vs %d\n", cls[w], cls[0]), abort();
      printf("%d\n", cls[0]);
    }
    fflush(stdout);
  }
  return 0;
}

// hash: "msg" -> "inf x0 x1 y0 y1" (affine raw hex)
static int cmd_hash() {
  char b[4000];
  while (scanf("%3999s", b) == 1) {
    wv_init();
    const auto msg = unhex(strcmp(b, "-") ? b : "");
    uint32_t b0[8];
    msg_b0(msg, b0);
    F hx, hy;
    const bool fin = hash_to_g2(b0, hx, hy);
    if (!fin) {
      printf("1 0 0 0 0\n");
      continue;
    }
    printf("0 %s %s\n", out_fp2(hx).c_str(), out_fp2(hy).c_str());
  }
  return 0;
}

// decompress: "sig96" -> "class x0 x1 y0 y1"
static int cmd_decompress() {
  char c[300];
  while (scanf("%299s", c) == 1) {
    wv_init();
    const auto sig = unhex(c);
    F x, y;
    bool inf;
    const int cls = g2_decompress(sig.data(), x, y, inf);
    if (cls || inf) {
      printf("%d %d 0 0 0 0\n", cls, (int)inf);
      continue;
    }
    printf("0 0 %s %s\n", out_fp2(x).c_str(), out_fp2(y).c_str());
  }
  return 0;
}

// opcount: "pk48 msg sig96" (an accepting item) -> JSON op counts per phase of verify_item
static void ops_line(const char* name, bool last) {
  static const char* nm[OPC_N] = {"dot1", "dot2", "dot3", "dot4", "dot5", "dot6", "mulp", "sqr2", "norm", "gcd"};
  printf("\"%s\": {", name);
  for (int k = 0; k < OPC_N; k++) printf("\"%s\": %llu%s", nm[k], g_wv_ops[k], k + 1 < OPC_N ? ", " : "");
  printf("}%s", last ? "}\n" : ", ");
  memset(g_wv_ops, 0, sizeof g_wv_ops);
}
static int cmd_opcount() {
  char a[300], b[4000], c[300];
  if (scanf("%299s %3999s %299s", a, b, c) != 3) return 2;
  wv_init();
  const auto pk = unhex(a), msg = unhex(strcmp(b, "-") ? b : ""), sig = unhex(c);
  bls::g1a P;
  bool pinf = false;
  if (bls::g1_decompress(pk.data(), P, pinf) != bls::REJ_OK) return 3;
  uint32_t b0[8];
  msg_b0(msg, b0);
  memset(g_wv_ops, 0, sizeof g_wv_ops);
  printf("{");
  F sx, sy, hx, hy;
  bool sinf;
  if (g2_decompress(sig.data(), sx, sy, sinf) != bls::REJ_OK) return 4;
  ops_line("decompress_subgroup", false);
  hash_to_g2(b0, hx, hy);
  ops_line("hash_to_g2", false);
  MPair pr[2];
  const bool active[2] = {true, true};
  pr[0] = mpair(g1_coord(P.x.l), g1_coord(P.y.l), hx, hy);
  pr[1] = mpair(cst(WC_NEG_G1_X), cst(WC_NEG_G1_Y), sx, sy);
  ops_line("pair_setup", false);
  const W12 f0 = miller_loop(pr, active);
  ops_line("miller", false);
  const bool ok = final_exp_is_one(f0);
  ops_line("final_exp", true);
  return ok ? 0 : 5;
}

// smul: "sig96 k" (k hex < r) -> compressed [k] S through the x-adic joint multiplication;
// "sum sig96 sig96" -> compressed S1 + S2
static int cmd_smul() {
  static uint32_t tab[15 * POINT_WORDS];
  char a[300], b[300];
  while (scanf("%299s %299s", a, b) == 2) {
    wv_init();
    const auto sig = unhex(a);
    F x, y;
    bool inf;
    if (g2_decompress(sig.data(), x, y, inf) || inf) {
      printf("-\n");
      continue;
    }
    uint32_t lam[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const std::string h(b);
    for (int i = 0; i < (int)h.size(); i++) {  // hex digit i from the right -> bits 4i..4i+3
      const char c = h[h.size() - 1 - i];
      const uint32_t v = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
      lam[i / 8] |= v << (4 * (i % 8));
    }
    const G2J r = g2_mul_lambda(x, y, lam, tab);
    const V w = g2_compress_words(r);
    for (int j = 0; j < 24; j++) printf("%08x", lane_val(w, j));
    printf("\n");
    fflush(stdout);
  }
  return 0;
}

// smul4: "sig96 k" -> "ok" when the four-wave form (wrecover.h lambda_base, g2_mul_digit per digit,
// the four partial products summed) equals g2_mul_lambda's [k] S, else "bad"
static int cmd_smul4() {
  static uint32_t tab[15 * POINT_WORDS];
  char a[300], b[300];
  while (scanf("%299s %299s", a, b) == 2) {
    wv_init();
    const auto sig = unhex(a);
    F x, y;
    bool inf;
    if (g2_decompress(sig.data(), x, y, inf) || inf) {
      printf("-\n");
      continue;
    }
    uint32_t lam[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const std::string h(b);
    for (int i = 0; i < (int)h.size(); i++) {
      const char c = h[h.size() - 1 - i];
      const uint32_t v = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
      lam[i / 8] |= v << (4 * (i % 8));
    }
    const G2J ref = g2_mul_lambda(x, y, lam, tab);
    uint64_t d[4];
    decompose_xabs(lam, d);
    G2J sum = g2_infinity();
    for (int j = 0; j < 4; j++) {
      F px, py;
      lambda_base(x, y, j, px, py);
      sum = g2_add(sum, g2_mul_digit(px, py, d[j]));
    }
    printf(g2_eq(sum, ref) ? "ok\n" : "bad\n");
    fflush(stdout);
  }
  return 0;
}

// teamadd: "sig96 case" -> ok / bad: wvteam.h team_g2_add (three host threads as the hash team's
// waves 0, 4, 5) against wcurve.h g2_add for case sum (P' + 2P), dbl (P' + P), neg (P' + (-P)),
// ainf (O + 2P), binf (P' + O), with P' = P in scaled Jacobian coordinates (Z = x_P); and "chain"
// (team_mul_x_abs against g2_mul_x_abs on P')
static int cmd_teamadd() {
  char a[300], b[32];
  while (scanf("%299s %31s", a, b) == 2) {
    wv_init();
    const auto sig = unhex(a);
    F x, y;
    bool inf;
    if (g2_decompress(sig.data(), x, y, inf) || inf) {
      printf("-\n");
      continue;
    }
    const G2J p = {x, y, cst(WC_ONE2)};
    const F l2 = sqr2(x);
    const G2J ps = {dot(p.x, l2), dot(p.y, dot(l2, x)), dot(p.z, x)};
    const G2J p2 = g2_dbl(p);
    const std::string c(b);
    G2J A = ps, B = p2;
    if (c == "dbl") B = p;
    else if (c == "neg") B = g2_neg(p);
    else if (c == "ainf") A = g2_infinity();
    else if (c == "binf") B = g2_infinity();
    const bool chain = c == "chain";
    const G2J want = chain ? g2_mul_x_abs(ps) : g2_add(A, B);
    for (auto& ctr : g_host_ctr) ctr.store(0);
    xst_g2(HS_ACC, chain ? ps : A);
    xst_g2(HS_Q2, chain ? ps : B);
    std::thread th[3];
    const int waves[3] = {0, 4, 5};
    for (int k = 0; k < 3; k++)
      th[k] = std::thread([&, k]() {
        g_host_wave = waves[k];
        wv_init();
        Team t = make_team(HASH_TEAM, CTR_HASH);
        if (chain) team_mul_x_abs(t, HS_Q2, HS_ACC);
        else team_g2_add(t, HS_ACC, HS_Q2);
      });
    for (auto& t : th) t.join();
    printf("%s\n", g2_eq(xld_g2(HS_ACC), want) ? "ok" : "bad");
    fflush(stdout);
  }
  return 0;
}

// g1dec: "u48" -> "class inf x y" (affine raw hex; zeros unless the point decodes and is finite)
static int cmd_g1dec() {
  char c[300];
  while (scanf("%299s", c) == 1) {
    wv_init();
    const auto u = unhex(c);
    if (u.size() != 48) {
      printf("%d 0 0 0\n", bls::REJ_LENGTH);
      continue;
    }
    F x, y;
    bool inf;
    const int cls = g1_decompress(u.data(), x, y, inf);
    if (cls || inf) {
      printf("%d %d 0 0\n", cls, (int)inf);
      continue;
    }
    const V rx = raw_canon(x), ry = raw_canon(y);
    // the embedded form: the imaginary halves are zero
    printf("0 0 %s %s%s\n", limbs_to_hex(rx, 0).c_str(), limbs_to_hex(ry, 0).c_str(),
           limbs_to_hex(rx, 1) == "0" && limbs_to_hex(ry, 1) == "0" ? "" : " imaginary-half-nonzero");
    fflush(stdout);
  }
  return 0;
}

static void print_topen(int sig_cls, int cls, const uint32_t (&out)[144]) {
  printf("%d %d ", sig_cls, cls);
  const uint8_t* b = (const uint8_t*)out;
  for (int i = 0; i < 576; i++) printf("%02x", b[i]);
  printf("\n");
  fflush(stdout);
}

// topen: "sig96 u48" -> "sigma's class, the item's class, the 576 bytes" through wverify.h tlock_item
static int cmd_topen() {
  char a[300], b[300];
  while (scanf("%299s %299s", a, b) == 2) {
    wv_init();
    const auto sig = unhex(a), u = unhex(b);
    if (sig.size() != 96 || u.size() != 48) {
      printf("%d %d -\n", bls::REJ_LENGTH, bls::REJ_LENGTH);
      continue;
    }
    uint32_t out[144];
    memset(out, 0xee, sizeof out);
    uint8_t sc = 0xff;
    const int cls = tlock_item(sig.data(), u.data(), out, sc);
    print_topen(sc, cls, out);
  }
  return 0;
}

// ttopen: as topen, by the eight-wave team (wvteam.h tlock_team), one host thread per wave;
// "sig96 -" classes the signature alone (sig_class_team) and prints "class - -"
static int cmd_ttopen() {
  char a[300], b[300];
  while (scanf("%299s %299s", a, b) == 2) {
    const auto sig = unhex(a), u = unhex(strcmp(b, "-") ? b : "");
    const bool alone = !strcmp(b, "-");
    if (sig.size() != 96 || (!alone && u.size() != 48)) {
      printf("%d %d -\n", bls::REJ_LENGTH, bls::REJ_LENGTH);
      continue;
    }
    for (auto& ctr : g_host_ctr) ctr.store(0);
    uint32_t out[144];
    memset(out, 0xee, sizeof out);
    int cls[TEAM_WAVES], sc[TEAM_WAVES];
    std::thread th[TEAM_WAVES];
    for (int w = 0; w < TEAM_WAVES; w++)
      th[w] = std::thread([&, w]() {
        g_host_wave = w;
        wv_init();
        uint8_t s = 0xff;
        cls[w] = alone ? 0 : tlock_team(sig.data(), u.data(), out, s);
        if (alone) s = sig_class_team(sig.data());
        sc[w] = s;
      });
    for (auto& t : th) t.join();
    for (int w = 1; w < TEAM_WAVES; w++)
      if (cls[w] != cls[0] || sc[w] != sc[0]) fprintf(stderr, "waves disagree\n"), abort();
    if (alone) printf("%d - -\n", sc[0]), fflush(stdout);
    else print_topen(sc[0], cls[0], out);
  }
  return 0;
}

// tscalar: "k32" -> "ok k digits": tscalar.h's reduction (k mod r as 64 hex digits, most significant
// first) and its 64 four-bit digits, window 0 first
static int cmd_tscalar() {
  char a[300];
  while (scanf("%299s", a) == 1) {
    const auto kb = unhex(a);
    if (kb.size() != 32) {
      printf("- - -\n");
      continue;
    }
    uint32_t k[8];
    const bool ok = bls::tseal_scalar(kb.data(), k);
    printf("%d ", (int)ok);
    for (int w = 7; w >= 0; w--) printf("%08x", k[w]);
    printf(" ");
    for (int w = 0; w < bls::TSEAL_WINDOWS; w++) printf("%x", bls::tseal_digit(k, w));
    printf("\n");
  }
  return 0;
}

static void print_hex(const uint8_t* b, int n) {
  for (int i = 0; i < n; i++) printf("%02x", b[i]);
}

// g1comp: "x y" (affine, raw hex) or "inf -" -> the 48 bytes of wseal.h g1_compress_store. The point is
// handed over in Jacobian form (x z^2, y z^3, z) with z = x + 1, so the conversion to affine runs too.
static int cmd_g1comp() {
  char a[300], b[300];
  while (scanf("%299s %299s", a, b) == 2) {
    wv_init();
    G2J p = g2_infinity();
    if (strcmp(a, "inf")) {
      const F x = to_mont(raw_fp2(a, "0")), y = to_mont(raw_fp2(b, "0"));
      const F z = lo_only(add(x, cst(WC_ONE2)));
      const F zz = sqr2(z);
      p = {dot(x, zz), dot(y, dot(zz, z)), z};
    }
    uint32_t out[12];
    memset(out, 0xee, sizeof out);
    g1_compress_store(out, p);
    print_hex((const uint8_t*)out, 48);
    printf("\n");
    fflush(stdout);
  }
  return 0;
}

// the sealing tables in the batch engine's form, built by tseal.h's own row builder: T1 once, TK per key
static std::vector<uint32_t> seal_table(const bls::g1a& A) {
  std::vector<uint32_t> t((size_t)bls::TSEAL_T1_WORDS);
  for (int w = 0; w < bls::TSEAL_WINDOWS; w++)
    bls::tseal_g1_row_of(A, w, [&](int j, const bls::g1a& p) {
      uint32_t* o = t.data() + (size_t)bls::tseal_entry(w, j) * bls::TSEAL_G1_WORDS;
      for (int i = 0; i < 12; i++) o[i] = p.x.l[i], o[12 + i] = p.y.l[i];
    });
  return t;
}
static void round_b0(uint64_t round, uint32_t (&b0)[8]) {
  uint32_t msg[8];
  bls::drand_message_v2(msg, round);
  xmd_b0_msg32(msg, b0);
}

// tseal / ttseal: "pk48 round k32" -> "ok u48 gt576" through wseal.h seal_item (one wave) or seal_team
// (one host thread per wave); a key that does not decode, or is the point at infinity, prints "-1 - -"
static int cmd_tseal(bool team) {
  char a[300], b[300], c[300];
  static const std::vector<uint32_t> T1 =
      seal_table(bls::g1a{bls::fp_load_const(bls::G1_GEN_X), bls::fp_load_const(bls::G1_GEN_Y)});
  std::string tk_key;
  std::vector<uint32_t> TK;
  while (scanf("%299s %299s %299s", a, b, c) == 3) {
    const auto pk = unhex(a), kb = unhex(c);
    const uint64_t round = strtoull(b, nullptr, 10);
    if (tk_key != a) {
      bls::g1a P;
      bool pinf = false;
      if (pk.size() != 48 || bls::g1_decompress(pk.data(), P, pinf) != bls::REJ_OK || pinf) {
        printf("-1 - -\n");
        continue;
      }
      TK = seal_table(P);
      tk_key = a;
    }
    if (kb.size() != 32) {
      printf("-1 - -\n");
      continue;
    }
    uint32_t b0[8];
    round_b0(round, b0);
    uint32_t u[12], gt[144];
    memset(u, 0xee, sizeof u);
    memset(gt, 0xee, sizeof gt);
    int ok[TEAM_WAVES];
    if (!team) {
      wv_init();
      ok[0] = seal_item(kb.data(), b0, T1.data(), TK.data(), u, gt);
    } else {
      for (auto& ctr : g_host_ctr) ctr.store(0);
      std::thread th[TEAM_WAVES];
      for (int w = 0; w < TEAM_WAVES; w++)
        th[w] = std::thread([&, w]() {
          g_host_wave = w;
          wv_init();
          ok[w] = seal_team(kb.data(), b0, T1.data(), TK.data(), u, gt);
        });
      for (auto& t : th) t.join();
      for (int w = 1; w < TEAM_WAVES; w++)
        if (ok[w] != ok[0]) fprintf(stderr, "waves disagree\n"), abort();
      // P's slots are overwritten before the workgroup exits
      for (int i = 0; i < 64; i++)
        if (g_host_blk[S_PX * 64 + i] | g_host_blk[S_PY * 64 + i]) fprintf(stderr, "P left in its slots\n"), abort();
    }
    printf("%d ", ok[0]);
    print_hex((const uint8_t*)u, 48);
    printf(" ");
    print_hex((const uint8_t*)gt, 576);
    printf("\n");
    fflush(stdout);
  }
  return 0;
}

// ------------------------------------------------------------------ authenticated timelock (wauth.h)
static const std::vector<uint32_t>& t1_table() {
  static const std::vector<uint32_t> T1 =
      seal_table(bls::g1a{bls::fp_load_const(bls::G1_GEN_X), bls::fp_load_const(bls::G1_GEN_Y)});
  return T1;
}
static void print_words_be(const uint32_t (&w)[8]) {
  for (int i = 0; i < 8; i++) printf("%08x", w[i]);
}
// a hex integer below 2^256 as eight little-endian words
static void hex_to_k(const std::string& h, uint32_t (&k)[8]) {
  for (int i = 0; i < 8; i++) k[i] = 0;
  for (int i = 0; i < (int)h.size() && i < 64; i++) {
    const char c = h[h.size() - 1 - i];
    const uint32_t v = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
    k[i / 8] |= v << (4 * (i % 8));
  }
}
// run fn(w) as the eight waves of one workgroup
template <class Fn>
static void run_team(Fn fn) {
  for (auto& ctr : g_host_ctr) ctr.store(0);
  std::thread th[TEAM_WAVES];
  for (int w = 0; w < TEAM_WAVES; w++)
    th[w] = std::thread([&, w]() {
      g_host_wave = w;
      wv_init();
      fn(w);
    });
  for (auto& t : th) t.join();
}
static bool slots_zero(int from, int to) {
  for (int i = from * 64; i < to * 64; i++)
    if (g_host_blk[i]) return false;
  return true;
}

// gtmid: "gt576" (hex, tlock.h's encoding) -> "h2 ks1": blocks 0 and 1 of tmask.h's key stream from
// wauth.h gt_midstate over the value in lane form (Montgomery). Aborts unless that midstate is
// tmask_midstate's over the bytes themselves.
static int cmd_gtmid() {
  static char a[1300];
  while (scanf("%1299s", a) == 1) {
    wv_init();
    const std::string h(a);
    if (h.size() != 1152) {
      printf("- -\n");
      continue;
    }
    W12 e;
    for (int c = 0; c < 6; c++) {  // position gt_pos(c): the imaginary part's 96 hex digits, then the real part's
      const size_t o = 192 * (size_t)gt_pos(c);
      e.c[c] = to_mont(raw_fp2(h.substr(o + 96, 96), h.substr(o, 96)));
    }
    uint32_t mid[8], ref[8], ks[8];
    gt_midstate(mid, [&](int c) { return e.c[c]; });
    const auto bytes = unhex(h);
    uint32_t enc[144];
    memcpy(enc, bytes.data(), 576);
    bls::tmask_midstate(ref, [&](int k) { return bls::tmask_coef_enc(enc, k); });
    if (memcmp(mid, ref, sizeof mid)) fprintf(stderr, "midstate differs from the bytes'\n"), abort();
    bls::tmask_block(ks, mid, 0);
    print_words_be(ks);
    printf(" ");
    bls::tmask_block(ks, mid, 1);
    print_words_be(ks);
    printf("\n");
    fflush(stdout);
  }
  return 0;
}

// awalk / tawalk: "k" (hex, 0 < k < r) -> the 48 compressed bytes of k G1 by wseal.h seal_walk (one wave)
// or wauth.h auth_walk_team (one host thread per wave), and the number of partial sums at infinity ("-" for
// awalk)
static int cmd_awalk(bool team) {
  char a[300];
  while (scanf("%299s", a) == 1) {
    uint32_t k[8];
    hex_to_k(a, k);
    uint32_t u[12];
    memset(u, 0xee, sizeof u);
    if (!team) {
      wv_init();
      g1_compress_store(u, seal_walk(t1_table().data(), k));
      print_hex((const uint8_t*)u, 48);
      printf(" -\n");
    } else {
      int n_inf = 0;
      run_team([&](int w) {
        Team all = make_team(ALL_WAVES, CTR_ALL);
        if (w == 0)
          for (int j = 0; j < TEAM_WAVES; j++) n_inf += g2_is_inf(auth_walk_part(t1_table().data(), k, 8 * j, 8));
        const G2J s = auth_walk_team(all, t1_table().data(), k);
        team_sync(all);
        auth_walk_clear(all);
        if (w == 3) g1_compress_store(u, s);  // any wave holds the sum
      });
      if (!slots_zero(AW_SLOT, AW_SLOT + 3 * TEAM_WAVES)) fprintf(stderr, "partial sums left in their slots\n"), abort();
      print_hex((const uint8_t*)u, 48);
      printf(" %d\n", n_inf);
    }
    fflush(stdout);
  }
  return 0;
}

// aopen / taopen: "sig96 u48 v32 w" (hex; w: 1 .. 256 bytes) -> "sigma's class, the item's class, the mlen
// output bytes" through wauth.h auth_open_item (one wave) or auth_open_team (one host thread per wave). The
// output buffer is guarded on both sides; taopen aborts if the walk's partial sums are left in their slots.
static int cmd_aopen(bool team) {
  static char a[300], b[300], c[300], d[600];
  while (scanf("%299s %299s %299s %599s", a, b, c, d) == 4) {
    const auto sig = unhex(a), u = unhex(b), v = unhex(c), ws = unhex(d);
    if (sig.size() != 96 || u.size() != 48 || v.size() != 32 || ws.empty() || ws.size() > 256) {
      printf("%d %d -\n", bls::REJ_LENGTH, bls::REJ_LENGTH);
      continue;
    }
    const uint32_t mlen = (uint32_t)ws.size();
    std::vector<uint8_t> out(mlen + 16, 0xee);
    int cls[TEAM_WAVES], sc[TEAM_WAVES];
    if (!team) {
      wv_init();
      uint8_t s = 0xff;
      cls[0] = auth_open_item(sig.data(), u.data(), v.data(), ws.data(), mlen, t1_table().data(), out.data() + 8, s);
      sc[0] = s;
    } else {
      run_team([&](int w) {
        uint8_t s = 0xff;
        cls[w] = auth_open_team(sig.data(), u.data(), v.data(), ws.data(), mlen, t1_table().data(), out.data() + 8, s);
        sc[w] = s;
      });
      for (int w = 1; w < TEAM_WAVES; w++)
        if (cls[w] != cls[0] || sc[w] != sc[0]) fprintf(stderr, "waves disagree\n"), abort();
      if ((cls[0] == 0 || cls[0] == bls::TAUTH_REJ_AUTH) && !slots_zero(AW_SLOT, AW_SLOT + 3 * TEAM_WAVES))
        fprintf(stderr, "partial sums of k' left in their slots\n"), abort();
    }
    for (int i = 0; i < 8; i++)
      if (out[i] != 0xee || out[8 + mlen + i] != 0xee) fprintf(stderr, "store outside the item's bytes\n"), abort();
    printf("%d %d ", sc[0], cls[0]);
    print_hex(out.data() + 8, (int)mlen);
    printf("\n");
    fflush(stdout);
  }
  return 0;
}

// aseal / taseal: "pk48 round seed32 msg mode" (round decimal, the rest hex; mode "-" or "k0") -> "ok u48 v32
// w" through wauth.h auth_seal_item (one wave) or auth_seal_team (one host thread per wave). Mode k0 enters
// behind the derivation (auth_seal_*_k) with the scalar zero and k_ok false: the refusal's stores, which no
// known SHA-256 input reaches -- the derivation itself is not part of that line. V and W are guarded on both
// sides; taseal aborts if a workgroup that sealed leaves anything in the block's LDS slots (K, k pk, ...).
static int cmd_aseal(bool team) {
  static char a[300], b[300], c[300], d[600], m[16];
  std::string tk_key;
  std::vector<uint32_t> TK;
  while (scanf("%299s %299s %299s %599s %15s", a, b, c, d, m) == 5) {
    const auto pk = unhex(a), seed = unhex(c), msg = unhex(d);
    const uint64_t round = strtoull(b, nullptr, 10);
    const bool k0 = !strcmp(m, "k0");
    if (tk_key != a) {
      bls::g1a P;
      bool pinf = false;
      if (pk.size() != 48 || bls::g1_decompress(pk.data(), P, pinf) != bls::REJ_OK || pinf) {
        printf("-1 - - -\n");
        continue;
      }
      TK = seal_table(P);
      tk_key = a;
    }
    if (seed.size() != 32 || msg.empty() || msg.size() > 256) {
      printf("-1 - - -\n");
      continue;
    }
    const uint32_t mlen = (uint32_t)msg.size();
    uint32_t b0[8], u[12];
    round_b0(round, b0);
    memset(u, 0xee, sizeof u);
    std::vector<uint8_t> v(32 + 16, 0xee), w(mlen + 16, 0xee);
    uint32_t sw[8];
    const uint32_t kz[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bls::tauth_seed_words(sw, seed.data());
    const uint32_t* T1 = t1_table().data();
    int ok[TEAM_WAVES];
    if (!team) {
      wv_init();
      ok[0] = k0 ? auth_seal_item_k(sw, kz, false, msg.data(), mlen, b0, T1, TK.data(), u, v.data() + 8, w.data() + 8)
                 : auth_seal_item(seed.data(), msg.data(), mlen, b0, T1, TK.data(), u, v.data() + 8, w.data() + 8);
    } else {
      memset(g_host_blk, 0, sizeof g_host_blk);
      run_team([&](int wv_) {
        ok[wv_] = k0 ? auth_seal_team_k(sw, kz, false, msg.data(), mlen, b0, T1, TK.data(), u, v.data() + 8, w.data() + 8)
                     : auth_seal_team(seed.data(), msg.data(), mlen, b0, T1, TK.data(), u, v.data() + 8, w.data() + 8);
      });
      for (int i = 1; i < TEAM_WAVES; i++)
        if (ok[i] != ok[0]) fprintf(stderr, "waves disagree\n"), abort();
      if (!slots_zero(0, BLK_SLOTS)) fprintf(stderr, "seed-derived values left in the block's slots\n"), abort();
    }
    for (int i = 0; i < 8; i++)
      if (v[i] != 0xee || v[40 + i] != 0xee || w[i] != 0xee || w[8 + mlen + i] != 0xee)
        fprintf(stderr, "store outside the item's bytes\n"), abort();
    printf("%d ", ok[0]);
    print_hex((const uint8_t*)u, 48);
    printf(" ");
    print_hex(v.data() + 8, 32);
    printf(" ");
    print_hex(w.data() + 8, (int)mlen);
    printf("\n");
    fflush(stdout);
  }
  return 0;
}

// ------------------------------------------------------------------ signing (wsign.h)
// sign / tsign: "sk32 msg" -> the 96 bytes of compress([sk mod r] H(msg)) through wsign.h sign_item (one wave:
// the hash, then the four digit ladders in turn) or sign_team (one host thread per wave). The key is reduced
// by tscalar.h, whose reduction is the host's scalar_mod_r (k mod r, zero kept). tsign aborts if a partial
// product is still in its LDS slots when the workgroup exits.
static int cmd_sign(bool team) {
  static char a[300], b[4000];
  while (scanf("%299s %3999s", a, b) == 2) {
    const auto kb = unhex(a), msg = unhex(strcmp(b, "-") ? b : "");
    if (kb.size() != 32) {
      printf("-\n");
      continue;
    }
    uint32_t sk[8], b0[8], out[24];
    (void)bls::tseal_scalar(kb.data(), sk);
    msg_b0(msg, b0);
    memset(out, 0xee, sizeof out);
    if (!team) {
      wv_init();
      sign_item(b0, sk, out);
    } else {
      for (int i = SIGN_PART * 64; i < SIGN_PART_END * 64; i++) g_host_blk[i] = 0xeeeeeeeeu;
      run_team([&](int) { sign_team(b0, sk, out); });
      if (!slots_zero(SIGN_PART, SIGN_PART_END)) fprintf(stderr, "a partial product left in its slots\n"), abort();
    }
    print_hex((const uint8_t*)out, 96);
    printf("\n");
    fflush(stdout);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "sign")) return cmd_sign(false);
  if (argc >= 2 && !strcmp(argv[1], "tsign")) return cmd_sign(true);
  if (argc >= 2 && !strcmp(argv[1], "gtmid")) return cmd_gtmid();
  if (argc >= 2 && !strcmp(argv[1], "awalk")) return cmd_awalk(false);
  if (argc >= 2 && !strcmp(argv[1], "tawalk")) return cmd_awalk(true);
  if (argc >= 2 && !strcmp(argv[1], "aopen")) return cmd_aopen(false);
  if (argc >= 2 && !strcmp(argv[1], "taopen")) return cmd_aopen(true);
  if (argc >= 2 && !strcmp(argv[1], "aseal")) return cmd_aseal(false);
  if (argc >= 2 && !strcmp(argv[1], "taseal")) return cmd_aseal(true);
  if (argc >= 2 && !strcmp(argv[1], "tscalar")) return cmd_tscalar();
  if (argc >= 2 && !strcmp(argv[1], "g1comp")) return cmd_g1comp();
  if (argc >= 2 && !strcmp(argv[1], "tseal")) return cmd_tseal(false);
  if (argc >= 2 && !strcmp(argv[1], "ttseal")) return cmd_tseal(true);
  if (argc >= 2 && !strcmp(argv[1], "g1dec")) return cmd_g1dec();
  if (argc >= 2 && !strcmp(argv[1], "topen")) return cmd_topen();
  if (argc >= 2 && !strcmp(argv[1], "ttopen")) return cmd_ttopen();
  if (argc >= 2 && !strcmp(argv[1], "field")) return cmd_field();
  if (argc >= 2 && !strcmp(argv[1], "inv")) return cmd_inv();
  if (argc >= 2 && !strcmp(argv[1], "teamadd")) return cmd_teamadd();
  if (argc >= 2 && !strcmp(argv[1], "verify")) return cmd_verify();
  if (argc >= 2 && !strcmp(argv[1], "tverify")) return cmd_tverify();
  if (argc >= 2 && !strcmp(argv[1], "tverify_pre")) return cmd_tverify_pre();
  if (argc >= 2 && !strcmp(argv[1], "hash")) return cmd_hash();
  if (argc >= 2 && !strcmp(argv[1], "decompress")) return cmd_decompress();
  if (argc >= 2 && !strcmp(argv[1], "opcount")) return cmd_opcount();
  if (argc >= 2 && !strcmp(argv[1], "smul")) return cmd_smul();
  if (argc >= 2 && !strcmp(argv[1], "smul4")) return cmd_smul4();
  fprintf(stderr, "usage: wvtest field|verify|hash|pair\n");
  return 2;
}
