// The host side's pure logic: bit packing, share selection, Fr / Lagrange arithmetic, layout and
// count arithmetic. Nothing here touches HIP or blsv_ctx, so tools/hosttest.cpp runs it under the
// sanitizers on a machine without a GPU (tests/test_sanitize.py). No HIP header may be included.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/blsverify.h"

#pragma GCC visibility push(hidden)  // internal to whatever links it: never part of the library's ABI
namespace blsv_detail {

// reduce a 32-byte big-endian scalar mod r -> 8 little-endian words
inline void scalar_mod_r(const uint8_t* be32, uint32_t out[8]) {
  static const uint32_t R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                                0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = be32 + 28 - 4 * i;
    out[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
  for (int rep = 0; rep < 4; rep++) {  // value < 2^256 < 3r: at most 2 subtractions
    bool ge = true;
    for (int i = 7; i >= 0; i--) {
      if (out[i] != R[i]) {
        ge = out[i] > R[i];
        break;
      }
    }
    if (!ge) break;
    uint64_t br = 0;
    for (int i = 0; i < 8; i++) {
      uint64_t d = (uint64_t)out[i] - R[i] - br;
      out[i] = (uint32_t)d;
      br = (d >> 63) & 1;
    }
  }
}

// ---------------------------------------------------------------- Lagrange coefficients on the host
// kyber share.RecoverCommit's basis at 0 ([ext] drand/kyber@d59c3367dcde share/poly.go, restated) over
// Fr for the shares x_i = index_i + 1: lambda_i = prod_{j != i} x_j / (x_j - x_i). Every factor is a
// small integer (|x_j - x_i| < 2^16), so a coefficient is ~2t small products and the t inverses share
// one Fermat inversion (Montgomery's trick): ~30 us for t = 33 against 0.56 ms for the serial
// one-lane-per-coefficient device kernel this replaced, and the recovery no longer waits on it.
namespace hfr {
typedef unsigned __int128 u128;
static const uint64_t RM[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull,
                               0x73eda753299d7d48ull};
struct E {
  uint64_t l[4];
};
inline bool geq_r(const uint64_t (&a)[5]) {
  if (a[4]) return true;
  for (int i = 3; i >= 0; i--)
    if (a[i] != RM[i]) return a[i] > RM[i];
  return true;
}
inline void sub_r(uint64_t (&a)[5]) {
  uint64_t br = 0;
  for (int i = 0; i < 4; i++) {
    const u128 d = (u128)a[i] - RM[i] - br;
    a[i] = (uint64_t)d;
    br = (uint64_t)(d >> 64) & 1u;
  }
  a[4] -= br;
}
inline uint64_t n0() {  // -r^-1 mod 2^64 (Newton)
  uint64_t inv = 1;
  for (int k = 0; k < 7; k++) inv *= 2 - RM[0] * inv;
  return (uint64_t)0 - inv;
}
// a b 2^-256 mod r (CIOS), inputs and output < r
inline E mul(const E& a, const E& b) {
  static const uint64_t N0 = n0();
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    uint64_t c = 0;
    for (int j = 0; j < 4; j++) {
      const u128 v = (u128)a.l[j] * b.l[i] + t[j] + c;
      t[j] = (uint64_t)v;
      c = (uint64_t)(v >> 64);
    }
    u128 v = (u128)t[4] + c;
    t[4] = (uint64_t)v;
    t[5] = (uint64_t)(v >> 64);
    const uint64_t m = t[0] * N0;
    v = (u128)m * RM[0] + t[0];
    c = (uint64_t)(v >> 64);
    for (int j = 1; j < 4; j++) {
      v = (u128)m * RM[j] + t[j] + c;
      t[j - 1] = (uint64_t)v;
      c = (uint64_t)(v >> 64);
    }
    v = (u128)t[4] + c;
    t[3] = (uint64_t)v;
    t[4] = t[5] + (uint64_t)(v >> 64);
  }
  uint64_t r[5] = {t[0], t[1], t[2], t[3], t[4]};
  if (geq_r(r)) sub_r(r);
  return {{r[0], r[1], r[2], r[3]}};
}
inline E add(const E& a, const E& b) {
  uint64_t r[5];
  uint64_t c = 0;
  for (int i = 0; i < 4; i++) {
    const u128 v = (u128)a.l[i] + b.l[i] + c;
    r[i] = (uint64_t)v;
    c = (uint64_t)(v >> 64);
  }
  r[4] = c;
  if (geq_r(r)) sub_r(r);
  return {{r[0], r[1], r[2], r[3]}};
}
inline const E& r2() {  // 2^512 mod r: 1 doubled 512 times
  static const E v = [] {
    E x = {{1, 0, 0, 0}};
    for (int k = 0; k < 512; k++) x = add(x, x);
    return x;
  }();
  return v;
}
// the Montgomery form of the integer v (|v| < 2^63), negative values as r - |v|
inline E from_int(int64_t v) {
  E x = {{(uint64_t)(v < 0 ? -v : v), 0, 0, 0}};
  if (v < 0) {
    uint64_t a[5] = {RM[0], RM[1], RM[2], RM[3], 0};
    uint64_t br = 0;
    for (int i = 0; i < 4; i++) {
      const u128 d = (u128)a[i] - x.l[i] - br;
      a[i] = (uint64_t)d;
      br = (uint64_t)(d >> 64) & 1u;
    }
    x = {{a[0], a[1], a[2], a[3]}};
  }
  return mul(x, r2());
}
inline E inv(const E& a) {  // a^(r - 2), Montgomery form in and out
  uint64_t e[4] = {RM[0] - 2, RM[1], RM[2], RM[3]};
  E acc = from_int(1);
  for (int i = 255; i >= 0; i--) {
    acc = mul(acc, acc);
    if ((e[i >> 6] >> (i & 63)) & 1u) acc = mul(acc, a);
  }
  return acc;
}
}  // namespace hfr

// lambda_i (plain, canonical, 8 little-endian words each) for the share indices idx[0 .. t)
inline void host_lagrange(const uint32_t* idx, size_t t, uint32_t* out) {
  std::vector<hfr::E> num(t), den(t), pre(t + 1);
  for (size_t i = 0; i < t; i++) {
    const int64_t xi = (int64_t)idx[i] + 1;
    hfr::E n = hfr::from_int(1), d = n;
    for (size_t j = 0; j < t; j++) {
      if (j == i) continue;
      const int64_t xj = (int64_t)idx[j] + 1;
      n = hfr::mul(n, hfr::from_int(xj));
      d = hfr::mul(d, hfr::from_int(xj - xi));
    }
    num[i] = n;
    den[i] = d;
  }
  // Montgomery's trick: one inversion for the t denominators (none is 0: the indices are distinct)
  pre[0] = hfr::from_int(1);
  for (size_t i = 0; i < t; i++) pre[i + 1] = hfr::mul(pre[i], den[i]);
  hfr::E run = hfr::inv(pre[t]);
  const hfr::E one_plain = {{1, 0, 0, 0}};
  for (size_t i = t; i-- > 0;) {
    const hfr::E di = hfr::mul(run, pre[i]);  // 1 / den_i
    run = hfr::mul(run, den[i]);
    const hfr::E lam = hfr::mul(hfr::mul(num[i], di), one_plain);  // out of Montgomery form
    for (int w = 0; w < 4; w++) {
      out[i * 8 + 2 * w] = (uint32_t)lam.l[w];
      out[i * 8 + 2 * w + 1] = (uint32_t)(lam.l[w] >> 32);
    }
  }
}

// ---------------------------------------------------------------- verdict bits
// the device bitmap's 64-bit words (bit i of the batch = bit i % 64 of word i / 64) -> ceil(n / 8)
// bytes, the bits past n cleared
inline void bitmap_words_to_bytes(const uint64_t* w, size_t n, uint8_t* out) {
  for (size_t i = 0; i < (n + 7) / 8; i++) {
    uint8_t b = (uint8_t)(w[i / 8] >> (8 * (i % 8)));
    if (i == (n + 7) / 8 - 1 && (n % 8)) b &= (uint8_t)((1u << (n % 8)) - 1);
    out[i] = b;
  }
}

// the latency branch's epilogue (launch_finish's rule on the host): the bitmap (optional, ceil(n / 8)
// bytes) of the n class bytes; returns the first rejected index or UINT64_MAX
inline uint64_t fold_classes(const uint8_t* cls, size_t n, uint8_t* ok_bitmap) {
  uint64_t fb = UINT64_MAX;
  for (size_t i = 0; i < n; i++) {
    if (cls[i] != BLSV_REJ_OK && fb == UINT64_MAX) fb = i;
    if (ok_bitmap) {
      if (i % 8 == 0) ok_bitmap[i / 8] = 0;
      ok_bitmap[i / 8] |= (uint8_t)((cls[i] == BLSV_REJ_OK) << (i % 8));
    }
  }
  return fb;
}

// OR the first cnt bits of src (LSB first) into dst starting at bit pos
inline void or_bits_at(uint8_t* dst, const uint8_t* src, size_t cnt, size_t pos) {
  const size_t nb = (cnt + 7) / 8, q = pos / 8, s = pos % 8;
  for (size_t j = 0; j < nb; j++) {
    uint8_t b = src[j];
    if (j == nb - 1 && (cnt % 8)) b &= (uint8_t)((1u << (cnt % 8)) - 1);
    dst[q + j] |= (uint8_t)(b << s);
    if (s && (b >> (8 - s))) dst[q + j + 1] |= (uint8_t)(b >> (8 - s));
  }
}

// ---------------------------------------------------------------- threshold shares
// the big-endian 16-bit index prefix of each of k tbls shares (0 for shares too short to hold one)
inline void share_indices(const uint8_t* partials, size_t partial_len, size_t k, std::vector<uint32_t>& index) {
  index.assign(k, 0);
  if (partial_len < 2) return;
  for (size_t i = 0; i < k; i++) index[i] = ((uint32_t)partials[i * partial_len] << 8) | partials[i * partial_len + 1];
}

// kyber tbls.Recover + share.RecoverCommit ([ext] drand/kyber@d59c3367dcde sign/tbls/tbls.go,
// share/poly.go, restated from the published source; parity unpinned by any reference test):
// walk the shares of items [lo, hi) in input order, skip invalid ones, keep appending valid ones until
// t are held -- a duplicate index counts toward t; then xyCommit keys them by index (duplicates
// collapse) and drops indices >= n. sel gets the positions and idx the indices of the shares to
// interpolate; false when fewer than t distinct remain ("not enough good public shares").
inline bool select_shares(const std::vector<uint8_t>& cls, const std::vector<uint32_t>& index, size_t lo, size_t hi,
                          size_t t, size_t n, std::vector<uint32_t>& sel, std::vector<uint32_t>& idx) {
  sel.clear();
  idx.clear();
  size_t taken = 0;
  for (size_t i = lo; i < hi && taken < t; i++) {
    if (cls[i] != BLSV_REJ_OK) continue;
    taken++;
    if (index[i] >= n || std::find(idx.begin(), idx.end(), index[i]) != idx.end()) continue;
    sel.push_back((uint32_t)i);
    idx.push_back(index[i]);
  }
  return sel.size() >= t;
}

// ---------------------------------------------------------------- counts and layouts
// randomized path: the items of a pass of cnt items in its failing groups fail[0 .. nf) (ascending
// indices of groups of G items, nf >= 1): only the last entry can be the pass's short last group
inline size_t rlc_failing_items(size_t cnt, size_t G, const uint32_t* fail, size_t nf) {
  const size_t ng = (cnt + G - 1) / G;
  return nf * G - (fail[nf - 1] == ng - 1 ? ng * G - cnt : 0);
}

// The main part of a pass of cnt items whose Miller f pass runs in rounds of q items (one single-lane
// wave on every SIMD): the whole rounds, when a partial last round follows at least one of them. The
// remainder [main, cnt) then runs its f pass beside the main part's final exponentiation (verify.cpp
// pairing_check). cnt itself means no split: q == 0, a pass of at most one round, or whole rounds only.
inline size_t tail_split_main(size_t cnt, size_t q) {
  if (q == 0 || cnt <= q || cnt % q == 0) return cnt;
  return cnt - cnt % q;
}

// svc_verify_mixed's packed upload of n items with mbytes message bytes:
// off[n + 1] | lens[n] | idx[n] | sigs[n][96] | message bytes (8-byte aligned parts)
struct SvcLayout {
  size_t o_len, o_idx, o_sig, o_msg, total;
};
inline SvcLayout svc_layout(size_t n, size_t mbytes) {
  SvcLayout l;
  l.o_len = (n + 1) * 8;
  l.o_idx = l.o_len + ((n * 4 + 7) & ~size_t(7));
  l.o_sig = l.o_idx + ((n * 4 + 7) & ~size_t(7));
  l.o_msg = l.o_sig + n * 96;
  l.total = l.o_msg + mbytes + 8;
  return l;
}

// blsv_tlock_seal_rounds*: whether the byte counts of n items (the largest array is the n x 576 bytes of
// encoded values) fit size_t
inline bool seal_rounds_fits(size_t n) { return n <= SIZE_MAX / BLSV_GT_LEN; }
// ... and what a pass of cnt items keeps in the S staging (192 bytes per item; every stage of the pass
// leaves S alone): the table of the points P_i = k_i pk (96 bytes each) first, then a host call's scalars
// (32 each), rounds (8 each; the offset is a multiple of 8), compressed U bytes (48 each) and ok bytes.
// [0, secret) is what the entry points clear behind the kernels: the points and the scalars.
struct SealRoundsLayout {
  size_t o_p, o_scalars, o_rounds, o_us, o_ok, total, secret;
};
inline SealRoundsLayout seal_rounds_layout(size_t cnt) {
  SealRoundsLayout l;
  l.o_p = 0;
  l.o_scalars = l.o_p + cnt * 96;
  l.o_rounds = l.o_scalars + cnt * BLSV_SCALAR_LEN;
  l.o_us = l.o_rounds + cnt * 8;
  l.o_ok = l.o_us + cnt * BLSV_U_LEN;
  l.total = l.o_ok + cnt;
  l.secret = l.o_rounds;
  return l;
}

// blsv_tlock_decrypt* / blsv_tlock_encrypt*: whether the call's KDF and message length are ones the fused
// tail knows, and the byte counts of n items of mlen bytes fit size_t
inline bool tcrypt_fits(int kdf, size_t mlen, size_t n) {
  return kdf == BLSV_KDF_SHA256_CTR && mlen >= 1 && mlen <= BLSV_TLOCK_MSG_MAX && n <= SIZE_MAX / BLSV_TLOCK_MSG_MAX &&
         n <= SIZE_MAX / BLSV_GT_LEN;
}

// blsv_tlock_encrypt_auth* / blsv_tlock_decrypt_auth*: tcrypt_fits, and the byte counts of the feature's own
// staging (tauth_layout, below 1 KiB per item) fit size_t
inline bool tauth_fits(int kdf, size_t mlen, size_t n) { return tcrypt_fits(kdf, mlen, n) && n <= SIZE_MAX / 1024; }
// ... and what a pass of cnt items of mlen bytes keeps in that staging (engine_ctx.h "authenticated timelock").
// [0, secret) is what an encrypting call clears behind the kernels: the seeds, the derived scalars and the
// plaintexts. A device form uses the scalar row alone. Every part starts on a multiple of 8.
struct TauthLayout {
  size_t o_seeds, o_scalars, o_in, secret, o_rounds, o_us, o_vs, o_out, o_flag, total;
  size_t o_offs;  // the ragged forms' offset table (tauth_layout_var)
};
inline TauthLayout tauth_layout(size_t cnt, size_t mlen) {
  const auto up8 = [](size_t v) { return (v + 7) & ~size_t(7); };
  TauthLayout l;
  l.o_seeds = 0;
  l.o_scalars = l.o_seeds + cnt * 32;
  l.o_in = l.o_scalars + cnt * BLSV_SCALAR_LEN;  // plaintexts (encrypt) or W bytes (decrypt)
  l.secret = up8(l.o_in + cnt * mlen);
  l.o_rounds = l.secret;
  l.o_us = l.o_rounds + cnt * 8;
  l.o_vs = l.o_us + cnt * BLSV_U_LEN;
  l.o_out = l.o_vs + cnt * 32;  // W bytes (encrypt) or messages (decrypt)
  l.o_flag = up8(l.o_out + cnt * mlen);  // ok bytes (encrypt) or class bytes (decrypt)
  l.total = l.o_flag + cnt;
  l.o_offs = l.total;  // the uniform forms stage no offsets
  return l;
}

// blsv_tlock_*_auth*_var (a length per item, the bytes packed back to back): tauth_fits' guard with every
// mlens[i] in 1 .. BLSV_TLOCK_MSG_MAX; *total gets the call's byte count, sum mlens (below 256 n, which
// tauth_fits' bound on n keeps inside size_t; the sum is checked all the same). n beyond the bound is refused
// before a length is read.
inline bool tauth_var_fits(int kdf, const uint32_t* mlens, size_t n, size_t* total) {
  if (!tauth_fits(kdf, BLSV_TLOCK_MSG_MAX, n) || (n && !mlens)) return false;
  size_t sum = 0;
  for (size_t i = 0; i < n; i++) {
    if (mlens[i] < 1 || mlens[i] > BLSV_TLOCK_MSG_MAX || mlens[i] > SIZE_MAX - sum) return false;
    sum += mlens[i];
  }
  *total = sum;
  return true;
}
// The offset table of the pass [base, base + cnt) of such a call: offs[i] = the bytes of the pass's items before
// item i, offs[cnt] = the pass's byte count (returned; cnt <= 2^20 items of at most 256 bytes: below 2^32).
// *words: every length of the pass is a multiple of 4, so with 4-byte aligned base pointers every item starts
// and ends on a dword.
inline size_t tauth_var_offsets(const uint32_t* mlens, size_t base, size_t cnt, uint32_t* offs, bool* words) {
  uint32_t at = 0, low = 0;
  for (size_t i = 0; i < cnt; i++) {
    offs[i] = at;
    at += mlens[base + i];
    low |= mlens[base + i];
  }
  offs[cnt] = at;
  *words = (low & 3) == 0;
  return at;
}
// ... and what such a pass keeps in the staging: tauth_layout with the two message regions sized by the pass's
// byte count, and the cnt + 1 offsets (a word array) behind the flags
inline TauthLayout tauth_layout_var(size_t cnt, size_t bytes) {
  const auto up8 = [](size_t v) { return (v + 7) & ~size_t(7); };
  TauthLayout l;
  l.o_seeds = 0;
  l.o_scalars = l.o_seeds + cnt * 32;
  l.o_in = l.o_scalars + cnt * BLSV_SCALAR_LEN;
  l.secret = up8(l.o_in + bytes);
  l.o_rounds = l.secret;
  l.o_us = l.o_rounds + cnt * 8;
  l.o_vs = l.o_us + cnt * BLSV_U_LEN;
  l.o_out = l.o_vs + cnt * 32;
  l.o_flag = up8(l.o_out + bytes);
  l.o_offs = up8(l.o_flag + cnt);
  l.total = l.o_offs + 4 * (cnt + 1);
  return l;
}

// ---------------------------------------------------------------- blsv_tlock_open_rounds*: the plan
// m round signatures, round j owning counts[j] consecutive items of the n packed ones. Whether the call's
// arguments are consistent and every byte count of it fits size_t: sum counts == n (the sum itself must
// not wrap), n x 576 and m x 96 fit, and a signature index fits the uint32 the tiles carry.
inline bool open_rounds_fits(const uint64_t* counts, size_t m, size_t n) {
  if (n > SIZE_MAX / BLSV_GT_LEN || m > SIZE_MAX / 96 || m >= UINT32_MAX) return false;
  uint64_t sum = 0;
  for (size_t j = 0; j < m; j++) {
    if (counts[j] > (uint64_t)n - sum) return false;  // sum <= n holds, so the difference does not wrap
    sum += counts[j];
  }
  return sum == n;
}

// The f pass runs one one-wave workgroup per tile: up to 64 consecutive items of the pass that share
// signature `sig` (an index into the pass's own signature list), or, with sig == kTlockTileMixed, items of
// several short runs whose lanes look their signature up per item.
constexpr uint32_t kTlockTileMixed = 0xffffffffu;
constexpr size_t kTlockTileItems = 64;
// A run of at least this many items gets uniform tiles (blsv_set_tlock_dense_min). The measured crossover
// (profiles/topen_rounds_bench.json; 1 Mi items, ms all-uniform / all-mixed): runs of 16
// 582.9 / 296.2, 32 389.4 / 293.7, 64 293.4 / 293.2, 128 293.6 / 293.4 -- below a full wave a uniform tile
// idles lanes and loses outright; from a full wave on the two forms are within the run-to-run spread, so
// uniform wins at no run length of the sweep and the default is the end of the swept range, not 64.
constexpr size_t kTlockDenseMinDefault = 128;
struct TlockTile {
  uint32_t first, len, sig;
};
// One pass: the items [base, base + cnt) of the call, cnt <= cap. sig_j: the call's index of every
// signature with items in the pass, ascending (at most cnt of them; zero-count rounds are not listed);
// sig_of[i]: the position in sig_j of item i's signature; tiles: every item of the pass exactly once, in
// order.
struct TlockRoundsPass {
  size_t base = 0, cnt = 0;
  std::vector<uint32_t> sig_j, sig_of;
  std::vector<TlockTile> tiles;
};
struct TlockRoundsCursor {
  size_t j = 0;       // the round the next pass starts in
  uint64_t used = 0;  // items of round j that earlier passes took
  size_t base = 0;
};
// The next pass of at most cap items, or false when no item is left. The rounds are walked in order; the
// part of a run that lies in this pass (a run cut by the pass boundary is prepared in both passes) becomes
// uniform tiles when it has at least dense_min items, and the stretches of shorter parts between them are
// cut into mixed tiles. dense_min = 1: every tile uniform; SIZE_MAX: every tile mixed.
inline bool open_rounds_next_pass(const uint64_t* counts, size_t m, size_t cap, size_t dense_min, TlockRoundsCursor& cur,
                                  TlockRoundsPass& p) {
  p.base = cur.base;
  p.cnt = 0;
  p.sig_j.clear();
  p.sig_of.clear();
  p.tiles.clear();
  size_t mixed_from = 0;  // the open stretch of short runs is [mixed_from, p.cnt)
  auto cut = [&](size_t from, size_t to, uint32_t sig) {
    for (size_t f = from; f < to; f += kTlockTileItems)
      p.tiles.push_back({(uint32_t)f, (uint32_t)std::min(kTlockTileItems, to - f), sig});
  };
  while (cur.j < m && p.cnt < cap) {
    const uint64_t left = counts[cur.j] - cur.used;
    if (left == 0) {
      cur.j++;
      cur.used = 0;
      continue;
    }
    const size_t take = (size_t)std::min<uint64_t>(left, cap - p.cnt);
    const uint32_t sig = (uint32_t)p.sig_j.size();
    p.sig_j.push_back((uint32_t)cur.j);
    p.sig_of.insert(p.sig_of.end(), take, sig);
    if (take >= dense_min) {
      cut(mixed_from, p.cnt, kTlockTileMixed);
      cut(p.cnt, p.cnt + take, sig);
      mixed_from = p.cnt + take;
    }
    p.cnt += take;
    cur.used += take;
    if (cur.used == counts[cur.j]) {
      cur.j++;
      cur.used = 0;
    }
  }
  cut(mixed_from, p.cnt, kTlockTileMixed);
  cur.base += p.cnt;
  return p.cnt != 0;
}

// What a pass keeps in the FW staging until its f pass has run (the final exponentiation then takes FW as
// its scratch), for a workspace of cap items (a multiple of 64): the class and infinity bytes of the
// pass's decoded signatures, then the three arrays the host uploads in one copy -- sig_j, sig_of and the
// tiles (at most one of each per item).
struct OpenRoundsLayout {
  size_t o_cls, o_inf, o_sigj, o_sigof, o_tiles, total;
};
inline OpenRoundsLayout open_rounds_layout(size_t cap) {
  OpenRoundsLayout l;
  l.o_cls = 0;
  l.o_inf = cap;
  l.o_sigj = 2 * cap;
  l.o_sigof = l.o_sigj + 4 * cap;
  l.o_tiles = l.o_sigof + 4 * cap;
  l.total = l.o_tiles + sizeof(TlockTile) * cap;
  return l;
}
constexpr size_t kOpenRoundsFwBytesPerItem = 2 + 4 + 4 + sizeof(TlockTile);

// ---------------------------------------------------------------- timelock opening on the latency path
// blsv_set_tlock_lat_max: a host call of 1 .. lat_max items goes to k_lat_tlock, one workgroup per item.
// A call across rounds also gives every signature without items a workgroup of its own, so it takes the
// latency path only while those are no more than lat_max either (n_idle: tlock_lat_plan's count).
inline bool tlock_lat_routes(size_t n, size_t n_idle, size_t lat_max) {
  return n >= 1 && n <= lat_max && n_idle <= lat_max;
}
// The plan of a call across rounds (counts as open_rounds_fits accepted them): sig_of[i] = the signature
// of item i, idle = the signatures without items, ascending. With max_idle, stops and returns false once
// more than max_idle signatures are idle (the call is not for the latency path; the plan is then partial).
struct TlockLatPlan {
  std::vector<uint32_t> sig_of, idle;
};
inline bool tlock_lat_plan(const uint64_t* counts, size_t m, size_t max_idle, TlockLatPlan& p) {
  p.sig_of.clear();
  p.idle.clear();
  for (size_t j = 0; j < m; j++) {
    if (counts[j]) {
      p.sig_of.insert(p.sig_of.end(), (size_t)counts[j], (uint32_t)j);
    } else {
      if (p.idle.size() == max_idle) return false;
      p.idle.push_back((uint32_t)j);
    }
  }
  return true;
}
// One device buffer per call: what the host uploads in one copy (the m signatures, the n compressed U, and
// for a call across rounds sig_of and idle), then, 64-byte aligned, what one download brings back (the n x
// 576 bytes, the n item classes, the m signature classes). Every offset of a word array is 4-byte aligned.
// A decrypting call (mbytes = n x mlen, else 0) also uploads its mbytes ciphertext bytes, behind idle, and
// keeps its mbytes output bytes between the Gt bytes and the classes: its download starts there (o_down)
// and leaves the Gt bytes on the device. With mbytes = 0 nothing moves.
struct TlockLatLayout {
  size_t o_sigs, o_us, o_sigof, o_idle, o_min, in_total, o_gt, o_mout, o_cls, o_sigcls, o_down, out_total, total;
};
inline TlockLatLayout tlock_lat_layout(size_t m, size_t n, bool rounds, size_t n_idle, size_t mbytes = 0) {
  TlockLatLayout l;
  l.o_sigs = 0;
  l.o_us = 96 * m;
  l.o_sigof = l.o_us + BLSV_U_LEN * n;
  l.o_idle = l.o_sigof + (rounds ? 4 * n : 0);
  l.o_min = l.o_idle + 4 * n_idle;
  l.in_total = l.o_min + mbytes;
  l.o_gt = (l.in_total + 63) & ~size_t(63);
  l.o_mout = l.o_gt + BLSV_GT_LEN * n;
  l.o_cls = l.o_mout + mbytes;
  l.o_sigcls = l.o_cls + n;
  l.o_down = mbytes ? l.o_mout : l.o_gt;
  l.out_total = l.o_sigcls + m - l.o_down;
  l.total = l.o_sigcls + m;
  return l;
}

// ---------------------------------------------------------------- timelock sealing on the latency path
// blsv_set_tseal_lat_max: a host call of 1 .. lat_max items goes to k_lat_tseal, one workgroup per item.
inline bool tseal_lat_routes(size_t n, size_t lat_max) { return n >= 1 && n <= lat_max; }
// One device buffer per call: what the host uploads in one copy (for a call with a round per item the n
// rounds, 8 bytes each, first: the buffer is 8-byte aligned; then the n scalars, 32 bytes each), then,
// 64-byte aligned, what one download brings back (the n x 48 U bytes, the n x 576 Gt bytes, the n ok
// bytes; both word arrays start 4-byte aligned). [o_scalars, in_total) is what the entry clears behind the
// kernel. 665 bytes per item (657 for one shared round), plus at most 63 of padding.
constexpr size_t kTsealLatBytesPerItem = 8 + BLSV_SCALAR_LEN + BLSV_U_LEN + BLSV_GT_LEN + 1;
// An encrypting call (mlen > 0, else 0) also uploads its n x mlen message bytes, behind the scalars and
// cleared with them, and keeps its n x mlen ciphertext bytes between the Gt bytes and the ok bytes: it
// downloads the U bytes, and from o_mout on, and leaves the Gt bytes on the device. With mlen = 0 nothing moves.
struct TsealLatLayout {
  size_t o_rounds, o_scalars, o_min, in_total, o_us, o_gt, o_mout, o_ok, out_total, total;
};
// false when a byte count of the n items does not fit size_t (l is then untouched)
inline bool tseal_lat_layout(size_t n, bool rounds, TsealLatLayout& l, size_t mlen = 0) {
  if (mlen > BLSV_TLOCK_MSG_MAX || n > (SIZE_MAX - 63) / (kTsealLatBytesPerItem + 2 * mlen)) return false;
  l.o_rounds = 0;
  l.o_scalars = rounds ? 8 * n : 0;
  l.o_min = l.o_scalars + BLSV_SCALAR_LEN * n;
  l.in_total = l.o_min + mlen * n;
  l.o_us = (l.in_total + 63) & ~size_t(63);
  l.o_gt = l.o_us + BLSV_U_LEN * n;
  l.o_mout = l.o_gt + BLSV_GT_LEN * n;
  l.o_ok = l.o_mout + mlen * n;
  l.out_total = l.o_ok + n - l.o_us;
  l.total = l.o_us + l.out_total;
  return true;
}

// ---------------------------------------------------------------- authenticated timelock on the latency path
// blsv_set_tauth_lat_max: a host call of 1 .. lat_max items of blsv_tlock_decrypt_auth* / blsv_tlock_encrypt_auth*
// goes to k_lat_tauth_open / k_lat_tauth_seal, one workgroup per item (the decrypting side has a switch of its
// own, the encrypting side another). The rounds decrypt also needs tlock_lat_plan's consent (no more than
// lat_max signatures without items).
inline bool tauth_lat_routes(size_t n, size_t lat_max) { return n >= 1 && n <= lat_max; }
// Decrypting: one device buffer per call. What the host uploads in one copy -- the m signatures, the n
// compressed U, the n V, for a call across rounds sig_of and idle (word arrays: every part before them is a
// multiple of 4 bytes), then the n x mlen W bytes -- and, 64-byte aligned, what one download brings back: the
// n x mlen message bytes, the n item classes, the m signature classes.
struct TauthLatOpenLayout {
  size_t o_sigs, o_us, o_vs, o_sigof, o_idle, o_ws, in_total, o_out, o_cls, o_sigcls, out_total, total;
  size_t o_offs;  // the ragged forms' n + 1 offsets, in front of the W bytes (tauth_lat_open_layout_var)
};
// false when a byte count does not fit size_t or mlen is out of range (l is then untouched). Every signature
// has an item or is idle, so m <= n + n_idle bounds the signatures.
inline bool tauth_lat_open_layout(size_t m, size_t n, bool rounds, size_t n_idle, size_t mlen, TauthLatOpenLayout& l) {
  if (mlen < 1 || mlen > BLSV_TLOCK_MSG_MAX || n_idle > SIZE_MAX - n) return false;
  const size_t q = n + n_idle;
  if (m > q || q > (SIZE_MAX - 63) / (96 + 1 + 4 + BLSV_U_LEN + 32 + 4 + 1 + 2 * mlen)) return false;
  l.o_sigs = 0;
  l.o_us = 96 * m;
  l.o_vs = l.o_us + BLSV_U_LEN * n;
  l.o_sigof = l.o_vs + 32 * n;
  l.o_idle = l.o_sigof + (rounds ? 4 * n : 0);
  l.o_ws = l.o_idle + 4 * n_idle;
  l.o_offs = l.o_ws;  // none
  l.in_total = l.o_ws + mlen * n;
  l.o_out = (l.in_total + 63) & ~size_t(63);
  l.o_cls = l.o_out + mlen * n;
  l.o_sigcls = l.o_cls + n;
  l.out_total = l.o_sigcls + m - l.o_out;
  l.total = l.o_sigcls + m;
  return true;
}
// whether `bytes` can be the byte count of n items of 1 .. BLSV_TLOCK_MSG_MAX bytes each
inline bool tauth_var_bytes_ok(size_t n, size_t bytes) {
  return bytes >= n && bytes / BLSV_TLOCK_MSG_MAX + (bytes % BLSV_TLOCK_MSG_MAX != 0) <= n;
}
// The ragged forms' (blsv_tlock_decrypt_auth*_var): the same, with the n + 1 prefix offsets of the items (a word
// array, behind idle) uploaded in front of the W bytes, and `bytes` = the call's byte count (n .. 256 n, which the
// caller has checked: tauth_var_fits) in place of mlen * n
inline bool tauth_lat_open_layout_var(size_t m, size_t n, bool rounds, size_t n_idle, size_t bytes, TauthLatOpenLayout& l) {
  if (n_idle > SIZE_MAX - n || !tauth_var_bytes_ok(n, bytes)) return false;
  const size_t q = n + n_idle;
  if (m > q || q > (SIZE_MAX - 63 - 4) / (96 + 1 + 4 + BLSV_U_LEN + 32 + 4 + 1 + 4 + 2 * BLSV_TLOCK_MSG_MAX)) return false;
  l.o_sigs = 0;
  l.o_us = 96 * m;
  l.o_vs = l.o_us + BLSV_U_LEN * n;
  l.o_sigof = l.o_vs + 32 * n;
  l.o_idle = l.o_sigof + (rounds ? 4 * n : 0);
  l.o_offs = l.o_idle + 4 * n_idle;
  l.o_ws = l.o_offs + 4 * (n + 1);
  l.in_total = l.o_ws + bytes;
  l.o_out = (l.in_total + 63) & ~size_t(63);
  l.o_cls = l.o_out + bytes;
  l.o_sigcls = l.o_cls + n;
  l.out_total = l.o_sigcls + m - l.o_out;
  l.total = l.o_sigcls + m;
  return true;
}
// Encrypting: what the host uploads in one copy -- for a call with a round per item the n rounds, 8 bytes each,
// first (the buffer is 8-byte aligned), then the n seeds and the n x mlen plaintext bytes -- and, 64-byte
// aligned, what one download brings back: the n x 48 U bytes (4-byte aligned), the n V, the n x mlen W bytes,
// the n ok bytes. [o_seeds, in_total) is what the entry clears behind the kernel, in the device and the host
// copy. No scalar, no k pk and no K is ever in this buffer.
struct TauthLatSealLayout {
  size_t o_rounds, o_seeds, o_msgs, in_total, o_us, o_vs, o_ws, o_ok, out_total, total;
  size_t o_offs;  // the ragged forms' n + 1 offsets, in front of the seeds (tauth_lat_seal_layout_var)
};
inline bool tauth_lat_seal_layout(size_t n, bool rounds, size_t mlen, TauthLatSealLayout& l) {
  if (mlen < 1 || mlen > BLSV_TLOCK_MSG_MAX || n > (SIZE_MAX - 63) / (8 + 32 + BLSV_U_LEN + 32 + 1 + 2 * mlen)) return false;
  l.o_rounds = 0;
  l.o_seeds = rounds ? 8 * n : 0;
  l.o_msgs = l.o_seeds + 32 * n;
  l.in_total = l.o_msgs + mlen * n;
  l.o_us = (l.in_total + 63) & ~size_t(63);
  l.o_vs = l.o_us + BLSV_U_LEN * n;
  l.o_ws = l.o_vs + 32 * n;
  l.o_ok = l.o_ws + mlen * n;
  l.out_total = l.o_ok + n - l.o_us;
  l.total = l.o_ok + n;
  l.o_offs = l.o_seeds;  // none
  return true;
}
// The ragged forms' (blsv_tlock_encrypt_auth*_var): the same, with the n + 1 prefix offsets of the items (a word
// array) between the rounds and the seeds -- outside [o_seeds, in_total), which holds what is secret -- and
// `bytes` = the call's byte count (tauth_var_fits has checked it) in place of mlen * n
inline bool tauth_lat_seal_layout_var(size_t n, bool rounds, size_t bytes, TauthLatSealLayout& l) {
  if (!tauth_var_bytes_ok(n, bytes) ||
      n > (SIZE_MAX - 63 - 4) / (8 + 4 + 32 + BLSV_U_LEN + 32 + 1 + 2 * BLSV_TLOCK_MSG_MAX))
    return false;
  l.o_rounds = 0;
  l.o_offs = rounds ? 8 * n : 0;
  l.o_seeds = l.o_offs + 4 * (n + 1);
  l.o_msgs = l.o_seeds + 32 * n;
  l.in_total = l.o_msgs + bytes;
  l.o_us = (l.in_total + 63) & ~size_t(63);
  l.o_vs = l.o_us + BLSV_U_LEN * n;
  l.o_ws = l.o_vs + 32 * n;
  l.o_ok = l.o_ws + bytes;
  l.out_total = l.o_ok + n - l.o_us;
  l.total = l.o_ok + n;
  return true;
}

// ---------------------------------------------------------------- signing on the latency path
// blsv_set_sign_lat_max: a blsv_sign call of 1 .. lat_max messages goes to k_lat_sign, one workgroup per message.
inline bool sign_lat_routes(size_t n, size_t lat_max) { return n >= 1 && n <= lat_max; }
// One device buffer per call: what the host uploads in one copy -- the key (eight words, reduced mod r),
// the n message offsets (8 bytes each: the buffer is 8-byte aligned), the n message lengths (4 bytes each), the
// mbytes packed message bytes -- and, 64-byte aligned, what one download brings back: the n x 96 signature
// bytes at stride 96 (a word array: the host puts a share index in front of each as it copies out).
// [o_sk, o_off) is what the entry clears behind the kernel. 108 bytes per message plus its own bytes, plus
// the 32 of the key and at most 63 of padding.
constexpr size_t kSignLatKeyBytes = 32;
constexpr size_t kSignLatBytesPerItem = 8 + 4 + 96;
struct SignLatLayout {
  size_t o_sk, o_off, o_len, o_msgs, in_total, o_out, out_total, total;
};
// false when a byte count does not fit size_t (l is then untouched)
inline bool sign_lat_layout(size_t n, size_t mbytes, SignLatLayout& l) {
  const size_t fixed = kSignLatKeyBytes + 63;
  if (mbytes > SIZE_MAX - fixed || n > (SIZE_MAX - fixed - mbytes) / kSignLatBytesPerItem) return false;
  l.o_sk = 0;
  l.o_off = kSignLatKeyBytes;
  l.o_len = l.o_off + 8 * n;
  l.o_msgs = l.o_len + 4 * n;
  l.in_total = l.o_msgs + mbytes;
  l.o_out = (l.in_total + 63) & ~size_t(63);
  l.out_total = 96 * n;
  l.total = l.o_out + l.out_total;
  return true;
}

}  // namespace blsv_detail
#pragma GCC visibility pop
