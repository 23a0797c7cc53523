// Host tests of the library's pure host logic, built with sanitizers (tools/Makefile hosttest-asan,
// hosttest-tsan; tests/test_sanitize.py runs them):
//   coalesce  the blsv_service request coalescer (drand_amd/csrc/coalesce.h) with a stand-in run():
//             64 threads x rounds of bursts, every request answered exactly once with its own
//             result, bursts coalesced, stats consistent, destruction drains; and a lone request
//             leaves after the gap; a run() that throws fails only its own batch's calls.
//   boltload  the drand.db loader (drand_amd/csrc/boltload.cpp, include/boltload.h) over the files
//             named on the command line (written by tests/support/boltwriter.py), plus truncated and
//             bit-flipped copies of each: every call must fail cleanly or succeed, never fault.
//   hostlogic the pure host logic of the HIP-side units (drand_amd/csrc/hostlogic.h: bit packing,
//             share selection, Fr / Lagrange arithmetic, counts and layouts) on fixed cases, every
//             buffer heap-allocated at the size its caller gives it; the results go out as one JSON
//             line that tests/test_sanitize.py compares with values computed in Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <new>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../drand_amd/csrc/coalesce.h"
#include "../drand_amd/csrc/hostlogic.h"
#include "../include/boltload.h"

using blsv_detail::Coalescer;

namespace {

struct Req {
  int in = 0;
  int out = -1;
  int runs = 0;
};

int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      fails++;                                                     \
    }                                                              \
  } while (0)

int test_coalesce() {
  std::atomic<uint64_t> batches{0}, seen{0};
  std::atomic<size_t> largest{0};
  {
    Coalescer<Req> co(
        [&](std::vector<Req*>& b) {
          batches++;
          seen += b.size();
          size_t cur = largest.load();
          while (b.size() > cur && !largest.compare_exchange_weak(cur, b.size())) {
          }
          std::this_thread::sleep_for(std::chrono::microseconds(300));  // the "launch"
          for (Req* r : b) {
            r->out = r->in * 3 + 1;
            r->runs++;
          }
        },
        150, 2000, 48);
    const int T = 64, R = 20;
    std::vector<std::thread> th;
    std::atomic<int> bad{0};
    std::atomic<int> go{0};
    for (int t = 0; t < T; t++)
      th.emplace_back([&, t] {
        while (!go.load()) std::this_thread::yield();
        for (int r = 0; r < R; r++) {
          Req q;
          q.in = t * 1000 + r;
          co.submit(&q);
          if (q.out != q.in * 3 + 1 || q.runs != 1) bad++;
        }
      });
    go = 1;
    for (auto& x : th) x.join();
    CHECK(bad.load() == 0);
    const auto st = co.stats();
    CHECK(st.items == (uint64_t)T * R);
    CHECK(st.launches == batches.load());
    CHECK(st.max_batch <= 48);
    CHECK(st.launches < (uint64_t)T * R / 4);  // bursts were coalesced
    // a lone request waits for the gap only, not the whole window
    Req q;
    q.in = 7;
    const auto t0 = std::chrono::steady_clock::now();
    co.submit(&q);
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    CHECK(q.out == 22);
    CHECK(us < 1900);
  }  // destructor joins
  CHECK(seen.load() == 64 * 20 + 1);
  // run() throwing (a std::bad_alloc of a large batch): every caller of that batch returns, marked
  // failed by the fail hook, and the dispatcher serves the next batch
  {
    std::atomic<int> calls{0};
    Coalescer<Req> co(
        [&](std::vector<Req*>& b) {
          if (calls++ == 0) throw std::bad_alloc();
          for (Req* r : b) r->out = r->in + 1;
        },
        100, 1000, 64, [](Req* r) { r->out = -2; });
    std::vector<std::thread> th;
    std::vector<Req> qs(16);
    for (int t = 0; t < 16; t++) {
      qs[t].in = t;
      th.emplace_back([&, t] { co.submit(&qs[t]); });
    }
    for (auto& x : th) x.join();
    int failed = 0, served = 0;
    for (int t = 0; t < 16; t++) {
      failed += qs[t].out == -2;
      served += qs[t].out == t + 1;
    }
    CHECK(failed >= 1 && failed + served == 16);
    Req q;
    q.in = 41;
    co.submit(&q);
    CHECK(q.out == 42);
    // with_idle runs between batches
    int v = co.with_idle([&] { return 5; });
    CHECK(v == 5);
  }
  printf("{\"coalesce\": {\"batches\": %llu, \"items\": %llu, \"largest\": %zu}}\n",
         (unsigned long long)batches.load(), (unsigned long long)seen.load(), largest.load());
  return 0;
}

std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

void spit(const std::string& path, const std::vector<uint8_t>& v) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return;
  fwrite(v.data(), 1, v.size(), f);
  fclose(f);
}

// one open/count/load/close cycle; returns rows loaded or -1
long long load_all(const char* path) {
  dl_db* db = nullptr;
  if (dl_open(path, &db) != 0) {
    if (db) dl_close(db);
    return -1;
  }
  const int64_t n = dl_count(db);
  long long rows = -1;
  if (n >= 0 && n < (1 << 22)) {
    const size_t m = (size_t)n + 1;
    std::vector<uint64_t> rounds(m);
    std::vector<uint8_t> prev(m * 96), sig(m * 96), v2(m * 96), plen(m), slen(m), vlen(m);
    size_t got = 0;
    if (dl_load(db, 0, (size_t)n, rounds.data(), prev.data(), plen.data(), sig.data(), slen.data(), v2.data(),
                vlen.data(), &got) == 0)
      rows = (long long)got;
  }
  dl_close(db);
  return rows;
}

int test_boltload(int argc, char** argv) {
  unsigned long long tried = 0;
  for (int a = 0; a < argc; a++) {
    const long long good = load_all(argv[a]);
    CHECK(good > 0);
    const std::vector<uint8_t> raw = slurp(argv[a]);
    const std::string tmp = std::string(argv[a]) + ".fuzz";
    uint64_t s = 0x9e3779b97f4a7c15ull ^ raw.size();
    auto rnd = [&]() {
      s ^= s << 13, s ^= s >> 7, s ^= s << 17;
      return s;
    };
    for (int k = 0; k < 200; k++) {
      std::vector<uint8_t> v = raw;
      if (k % 4 == 0) {
        v.resize(rnd() % (raw.size() + 1));  // truncated
      } else {
        const int flips = 1 + (int)(rnd() % 8);
        for (int f = 0; f < flips && !v.empty(); f++) v[rnd() % v.size()] ^= (uint8_t)(1u << (rnd() % 8));
        if (k % 4 == 1) {  // aim at the first pages (meta, freelist, root): the offsets live there
          for (int f = 0; f < 4; f++) v[rnd() % std::min<size_t>(v.size(), 3 * 4096)] = (uint8_t)rnd();
        }
      }
      spit(tmp, v);
      (void)load_all(tmp.c_str());  // may fail; must not fault (ASan/UBSan report otherwise)
      tried++;
    }
    remove(tmp.c_str());
  }
  printf("{\"boltload\": {\"files\": %d, \"mutants\": %llu}}\n", argc, tried);
  return 0;
}

std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s;
}

std::string list_of(const std::vector<uint32_t>& v) {
  std::string s = "[";
  for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
  return s + "]";
}

// The cases are fixed here and restated in tests/test_sanitize.py (test_hostlogic_asan), which computes
// every expected value itself.
int test_hostlogic() {
  using namespace blsv_detail;
  const size_t sizes[] = {1, 7, 8, 9, 63, 64, 65, 127, 128, 129};
  std::string out = "{\"hostlogic\": {\"verdicts\": [";
  bool first = true;
  for (size_t n : sizes)
    for (size_t rej : {size_t(0), n - 1, n / 2, n}) {
      // one reject at 0, n - 1 or the middle, then all three (rej == n); the device words carry garbage
      // above bit n
      std::vector<uint8_t> cls(n, BLSV_REJ_OK);
      if (rej < n)
        cls[rej] = BLSV_REJ_PAIRING;
      else
        cls[0] = cls[n - 1] = cls[n / 2] = BLSV_REJ_PAIRING;
      const size_t words = (n + 63) / 64, nb = (n + 7) / 8;
      std::vector<uint64_t> w(words + 1, 0);  // the host driver's download buffer
      for (size_t i = 0; i < 64 * words; i++)
        if (i >= n || cls[i] == BLSV_REJ_OK) w[i / 64] |= uint64_t(1) << (i % 64);
      std::vector<uint8_t> guarded(nb + 2, 0xEE), exact(nb), folded(nb + 2, 0xEE), folded_exact(nb, 0xEE);
      bitmap_words_to_bytes(w.data(), n, guarded.data());
      bitmap_words_to_bytes(w.data(), n, exact.data());
      CHECK(!memcmp(guarded.data(), exact.data(), nb));
      const uint64_t fb = fold_classes(cls.data(), n, folded.data());
      CHECK(fold_classes(cls.data(), n, folded_exact.data()) == fb && fold_classes(cls.data(), n, nullptr) == fb);
      CHECK(!memcmp(folded.data(), folded_exact.data(), nb));
      out += std::string(first ? "" : ", ") + "{\"n\": " + std::to_string(n) + ", \"bytes\": \"" +
             hex(guarded.data(), nb + 2) + "\", \"fold\": \"" + hex(folded.data(), nb + 2) +
             "\", \"first_bad\": " + std::to_string(fb) + "}";
      first = false;
    }
  out += "], \"or_bits\": [";
  first = true;
  for (size_t n : sizes)
    for (size_t s = 0; s < 8; s++) {
      const size_t pos = 8 * (n % 3) + s, nb = (n + 7) / 8, cover = (pos + n + 7) / 8;
      std::vector<uint8_t> src(nb), dst(cover + 1, 0);  // one guard byte behind the last byte a bit can reach
      for (size_t j = 0; j < nb; j++) src[j] = (uint8_t)(37 * j + 11 * n + 0x5B);
      or_bits_at(dst.data(), src.data(), n, pos);
      out += std::string(first ? "" : ", ") + "\"" + hex(dst.data(), cover + 1) + "\"";
      first = false;
    }
  out += "], \"select\": [";
  struct Sel {
    std::vector<uint8_t> cls;
    std::vector<uint32_t> index;
    size_t lo, hi, t, n;
  };
  const std::vector<Sel> sels = {
      {{0, 0, 0, 0}, {3, 3, 5, 6}, 0, 4, 3, 10},        // a duplicate counts toward t, then collapses
      {{0, 0, 0, 0}, {1, 12, 2, 4}, 0, 4, 3, 10},       // an index >= n is dropped
      {{0, 7, 0, 5, 0}, {0, 1, 2, 3, 4}, 0, 5, 3, 10},  // invalid shares are skipped
      {{0, 0, 0}, {9, 8, 7}, 0, 3, 3, 10},              // exactly t distinct
      {{0, 0}, {9, 8}, 0, 2, 3, 10},                    // t - 1 distinct
      {{0, 0, 0, 0, 0, 6, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, 4, 9, 3, 10},  // [lo, hi) of a larger round
  };
  for (size_t k = 0; k < sels.size(); k++) {
    std::vector<uint32_t> sel, idx;
    const bool ok = select_shares(sels[k].cls, sels[k].index, sels[k].lo, sels[k].hi, sels[k].t, sels[k].n, sel, idx);
    out += std::string(k ? ", " : "") + "{\"ok\": " + (ok ? "true" : "false") + ", \"sel\": " + list_of(sel) +
           ", \"idx\": " + list_of(idx) + "}";
  }
  out += "], \"share_indices\": [";
  {
    std::vector<uint8_t> parts(3 * 98, 0x11);
    const uint32_t want[3] = {0, 0x0102, 0xffff};
    for (size_t i = 0; i < 3; i++) parts[i * 98] = (uint8_t)(want[i] >> 8), parts[i * 98 + 1] = (uint8_t)want[i];
    std::vector<uint32_t> index, none;
    share_indices(parts.data(), 98, 3, index);
    std::vector<uint8_t> tiny(3, 0x22);
    share_indices(tiny.data(), 1, 3, none);
    out += list_of(index) + ", " + list_of(none);
  }
  out += "], \"lagrange\": [";
  std::vector<std::vector<uint32_t>> sets = {{0}, {0, 1}, {5, 2, 9}, {}};
  for (uint32_t i = 0; i < 33; i++) sets[3].push_back((i * 37 + 11) % 1000);
  for (size_t k = 0; k < sets.size(); k++) {
    const size_t t = sets[k].size();
    std::vector<uint32_t> lam(t * 8);
    host_lagrange(sets[k].data(), t, lam.data());
    out += std::string(k ? ", " : "") + "[";
    for (size_t i = 0; i < t; i++) {
      uint8_t be[32];  // big-endian, as an integer reads
      for (int wd = 0; wd < 8; wd++)
        for (int b = 0; b < 4; b++) be[31 - (4 * wd + b)] = (uint8_t)(lam[i * 8 + wd] >> (8 * b));
      out += std::string(i ? ", " : "") + "\"" + hex(be, 32) + "\"";
    }
    out += "]";
  }
  out += "], \"scalar_mod_r\": [";
  {
    // 0, r - 1, r, r + 1, 2^256 - 1 (big-endian)
    const char* in[5] = {"0000000000000000000000000000000000000000000000000000000000000000",
                         "73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000",
                         "73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001",
                         "73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000002",
                         "ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff"};
    for (int k = 0; k < 5; k++) {
      std::vector<uint8_t> be(32);
      for (int i = 0; i < 32; i++) be[i] = (uint8_t)strtoul(std::string(in[k] + 2 * i, 2).c_str(), nullptr, 16);
      uint32_t wd[8];
      scalar_mod_r(be.data(), wd);
      uint8_t o[32];
      for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) o[31 - (4 * i + b)] = (uint8_t)(wd[i] >> (8 * b));
      out += std::string(k ? ", " : "") + "\"" + hex(o, 32) + "\"";
    }
  }
  out += "], \"rlc_failing_items\": [";
  {
    struct Rlc {
      size_t cnt, G;
      std::vector<uint32_t> fail;
    };
    const std::vector<Rlc> cases = {{197, 64, {3}}, {197, 64, {0, 3}}, {128, 64, {1}}, {65, 8, {8}}};
    for (size_t k = 0; k < cases.size(); k++)
      out += (k ? ", " : "") +
             std::to_string(rlc_failing_items(cases[k].cnt, cases[k].G, cases[k].fail.data(), cases[k].fail.size()));
  }
  out += "], \"svc_layout\": [";
  {
    const size_t cases[4][2] = {{1, 0}, {3, 32}, {7, 100}, {64, 2048}};
    for (int k = 0; k < 4; k++) {
      const SvcLayout l = svc_layout(cases[k][0], cases[k][1]);
      out += std::string(k ? ", " : "") + "[" + std::to_string(l.o_len) + ", " + std::to_string(l.o_idx) + ", " +
             std::to_string(l.o_sig) + ", " + std::to_string(l.o_msg) + ", " + std::to_string(l.total) + "]";
    }
  }
  out += "], \"seal_rounds\": {\"fits\": [";
  {
    // blsv_tlock_seal_rounds*: the guard on n at both sides of its limit, and the S-staging layout of a pass
    const size_t lim = SIZE_MAX / BLSV_GT_LEN;
    const size_t ns[6] = {0, 1, size_t(1) << 20, lim, lim + 1, SIZE_MAX};
    for (int k = 0; k < 6; k++) {
      const bool fits = seal_rounds_fits(ns[k]);
      if (fits) CHECK(ns[k] * BLSV_GT_LEN / BLSV_GT_LEN == ns[k]);  // no byte count of the call wraps
      out += std::string(k ? ", " : "") + (fits ? "true" : "false");
    }
    out += "], \"layout\": [";
    const size_t cnts[4] = {1, 64, 16384, size_t(1) << 20};
    for (int k = 0; k < 4; k++) {
      const SealRoundsLayout l = seal_rounds_layout(cnts[k]);
      CHECK(l.o_rounds % 8 == 0 && l.o_p % 4 == 0 && l.total <= 192 * cnts[k] && l.secret == l.o_rounds);
      out += std::string(k ? ", " : "") + "[" + std::to_string(l.o_p) + ", " + std::to_string(l.o_scalars) + ", " +
             std::to_string(l.o_rounds) + ", " + std::to_string(l.o_us) + ", " + std::to_string(l.o_ok) + ", " +
             std::to_string(l.total) + ", " + std::to_string(l.secret) + "]";
    }
  }
  out += "]}, \"tauth\": {\"fits\": [";
  {
    // blsv_tlock_encrypt_auth* / blsv_tlock_decrypt_auth*: the guard on (kdf, mlen, n) at both sides of its
    // limits, and the layout of a pass in the feature's own staging
    const size_t lim = SIZE_MAX / 1024;
    struct Fit {
      int kdf;
      size_t mlen, n;
    };
    const Fit fits[10] = {{1, 1, 0},   {1, 256, 1}, {1, 32, lim},     {1, 32, lim + 1}, {1, 0, 1},
                          {1, 257, 1}, {0, 32, 1},  {2, 32, 1}, {1, 256, SIZE_MAX}, {1, 3, size_t(1) << 20}};
    for (int k = 0; k < 10; k++) {
      const bool f = tauth_fits(fits[k].kdf, fits[k].mlen, fits[k].n);
      if (f) {
        const TauthLayout l = tauth_layout(fits[k].n, fits[k].mlen);
        CHECK(l.total >= fits[k].n && l.total <= 1024 * fits[k].n + 16);  // no byte count of the call wraps
      }
      out += std::string(k ? ", " : "") + (f ? "true" : "false");
    }
    out += "], \"layout\": [";
    const size_t cases[5][2] = {{1, 1}, {64, 3}, {65, 33}, {16384, 256}, {size_t(1) << 20, 32}};
    for (int k = 0; k < 5; k++) {
      const size_t cnt = cases[k][0], mlen = cases[k][1];
      const TauthLayout l = tauth_layout(cnt, mlen);
      CHECK(l.o_seeds == 0 && l.o_scalars == 32 * cnt && l.o_in == 64 * cnt && l.secret >= l.o_in + cnt * mlen);
      CHECK(l.o_rounds == l.secret && l.o_rounds % 8 == 0 && l.o_us == l.o_rounds + 8 * cnt && l.o_vs == l.o_us + 48 * cnt);
      CHECK(l.o_out == l.o_vs + 32 * cnt && l.o_out % 8 == 0 && l.o_flag >= l.o_out + cnt * mlen && l.o_flag % 8 == 0);
      CHECK(l.total == l.o_flag + cnt && l.total <= 1024 * cnt);
      out += std::string(k ? ", " : "") + "[" + std::to_string(l.o_in) + ", " + std::to_string(l.secret) + ", " +
             std::to_string(l.o_out) + ", " + std::to_string(l.o_flag) + ", " + std::to_string(l.total) + "]";
    }
  }
  out += "]}, \"tauth_lat\": {\"routes\": [";
  {
    // the authenticated timelock's latency path: the routing predicate as [n, lat_max, routes], the two buffer
    // layouts at the edge sizes and at the largest n that fits, and the overflow guard just above it
    const size_t rt[6][2] = {{0, 4}, {1, 4}, {4, 4}, {5, 4}, {1, 0}, {0, 0}};
    for (int k = 0; k < 6; k++)
      out += std::string(k ? ", " : "") + "[" + std::to_string(rt[k][0]) + ", " + std::to_string(rt[k][1]) + ", " +
             (tauth_lat_routes(rt[k][0], rt[k][1]) ? "true" : "false") + "]";
    const size_t open_most = (SIZE_MAX - 63) / (186 + 2 * 32), seal_most = (SIZE_MAX - 63) / (121 + 2 * 32);
    const size_t cases[4][2] = {{1, 1}, {3, 33}, {64, 256}, {0, 32}};  // n = 0: the largest n that fits at mlen 32
    out += "], \"open\": [";
    bool first = true;
    for (int k = 0; k < 4; k++)
      for (int rounds = 0; rounds < 2; rounds++) {
        const size_t mlen = cases[k][1], idle = rounds && cases[k][0] ? 2 : 0;
        const size_t n = cases[k][0] ? cases[k][0] : open_most - idle, m = rounds ? n + idle : 1;
        TauthLatOpenLayout l;
        CHECK(tauth_lat_open_layout(m, n, rounds != 0, idle, mlen, l));
        CHECK(l.o_sigof % 4 == 0 && l.o_idle % 4 == 0 && l.o_out % 64 == 0 && l.o_out - l.in_total < 64);
        CHECK(l.total >= l.o_sigcls && l.total > n && l.out_total == l.total - l.o_out);
        const size_t v[16] = {m, n, (size_t)rounds, idle, mlen, l.o_us, l.o_vs, l.o_sigof, l.o_idle, l.o_ws, l.in_total,
                              l.o_out, l.o_cls, l.o_sigcls, l.out_total, l.total};
        out += std::string(first ? "" : ", ") + "[";
        first = false;
        for (int j = 0; j < 16; j++) out += std::string(j ? ", " : "") + std::to_string(v[j]);
        out += "]";
      }
    out += "], \"seal\": [";
    first = true;
    for (int k = 0; k < 4; k++)
      for (int rounds = 0; rounds < 2; rounds++) {
        const size_t mlen = cases[k][1], n = cases[k][0] ? cases[k][0] : seal_most;
        TauthLatSealLayout l;
        CHECK(tauth_lat_seal_layout(n, rounds != 0, mlen, l));
        CHECK(l.o_seeds % 8 == 0 && l.o_us % 64 == 0 && l.o_us - l.in_total < 64 && l.total > n);
        const size_t v[12] = {n, (size_t)rounds, mlen, l.o_seeds, l.o_msgs, l.in_total, l.o_us, l.o_vs, l.o_ws, l.o_ok,
                              l.out_total, l.total};
        out += std::string(first ? "" : ", ") + "[";
        first = false;
        for (int j = 0; j < 12; j++) out += std::string(j ? ", " : "") + std::to_string(v[j]);
        out += "]";
      }
    // just above the largest n, and the lengths outside 1 .. 256: refused, the layout untouched
    TauthLatOpenLayout ol, okeep;
    TauthLatSealLayout sl, skeep;
    CHECK(tauth_lat_open_layout(1, 1, false, 0, 1, ol) && tauth_lat_seal_layout(1, false, 1, sl));
    okeep = ol;
    skeep = sl;
    const bool refused[8] = {!tauth_lat_open_layout(1, open_most + 1, false, 0, 32, ol),
                             !tauth_lat_open_layout(1, open_most, true, 1, 32, ol),
                             !tauth_lat_open_layout(1, SIZE_MAX, true, 1, 32, ol),
                             !tauth_lat_open_layout(3, 1, true, 1, 32, ol),
                             !tauth_lat_open_layout(1, 1, false, 0, 0, ol) && !tauth_lat_open_layout(1, 1, false, 0, 257, ol),
                             !tauth_lat_seal_layout(seal_most + 1, true, 32, sl),
                             !tauth_lat_seal_layout(SIZE_MAX, false, 32, sl),
                             !tauth_lat_seal_layout(1, false, 0, sl) && !tauth_lat_seal_layout(1, false, 257, sl)};
    CHECK(ol.total == okeep.total && ol.o_out == okeep.o_out && sl.total == skeep.total && sl.o_us == skeep.o_us);
    out += "], \"most\": [" + std::to_string(open_most) + ", " + std::to_string(seal_most) + "], \"refused\": [";
    for (int k = 0; k < 8; k++) out += std::string(k ? ", " : "") + (refused[k] ? "true" : "false");
  }
  out += "]}, \"open_rounds\": {\"fits\": [";
  {
    // blsv_tlock_open_rounds*: the guard on (counts, m, n) -- the sum must be n without wrapping, and
    // n x 576 must fit -- then the plan of every pass: each case prints its passes as
    // [base, cnt, sig_j, tiles] with a tile [first, len, sig] (sig -1 = mixed)
    const size_t lim = SIZE_MAX / BLSV_GT_LEN;
    struct Fit {
      std::vector<uint64_t> counts;
      size_t n;
    };
    const std::vector<Fit> fits = {{{}, 0},          {{1, 2, 3}, 6},       {{1, 2, 3}, 5},          {{1, 2, 3}, 7},
                                   {{0, 0}, 0},      {{UINT64_MAX, 2}, 1}, {{lim + 1}, lim + 1},    {{}, 1},
                                   {{4, UINT64_MAX - 3, 4}, 4}};
    for (size_t k = 0; k < fits.size(); k++) {
      std::vector<uint64_t> cn(fits[k].counts);  // heap, at the caller's size
      out += std::string(k ? ", " : "") + (open_rounds_fits(cn.data(), cn.size(), fits[k].n) ? "true" : "false");
    }
    out += "], \"plans\": [";
    struct Plan {
      std::vector<uint64_t> counts;
      size_t cap, dense_min;
    };
    const std::vector<uint64_t> runs = {0, 1, 63, 0, 64, 65, 129, 0};
    const std::vector<Plan> plans = {{runs, 1024, 1},       {runs, 1024, 64}, {runs, 1024, SIZE_MAX}, {{100, 60, 3}, 128, 64},
                                     {{0, 0, 0}, 64, 64},   {{200}, 64, 64},  {{1, 1, 1, 1, 1}, 64, 2}};
    for (size_t k = 0; k < plans.size(); k++) {
      std::vector<uint64_t> cn(plans[k].counts);
      size_t n = 0;
      for (uint64_t v : cn) n += (size_t)v;
      std::vector<int> covered(n, 0);
      std::vector<size_t> owner;  // the round of every item
      for (size_t j = 0; j < cn.size(); j++) owner.insert(owner.end(), (size_t)cn[j], j);
      TlockRoundsCursor cur;
      TlockRoundsPass p;
      size_t expect_base = 0;
      out += std::string(k ? ", " : "") + "[";
      bool first_pass = true;
      while (open_rounds_next_pass(cn.data(), cn.size(), plans[k].cap, plans[k].dense_min, cur, p)) {
        CHECK(p.base == expect_base && p.cnt >= 1 && p.cnt <= plans[k].cap && p.sig_of.size() == p.cnt);
        CHECK(p.sig_j.size() <= p.cnt && open_rounds_layout(plans[k].cap).total <= kOpenRoundsFwBytesPerItem * plans[k].cap);
        expect_base += p.cnt;
        for (size_t i = 0; i < p.cnt; i++) CHECK(p.sig_of[i] < p.sig_j.size() && p.sig_j[p.sig_of[i]] == owner[p.base + i]);
        out += std::string(first_pass ? "" : ", ") + "[" + std::to_string(p.base) + ", " + std::to_string(p.cnt) + ", " +
               list_of(p.sig_j) + ", [";
        first_pass = false;
        for (size_t t = 0; t < p.tiles.size(); t++) {
          const TlockTile& tl = p.tiles[t];
          CHECK(tl.len >= 1 && tl.len <= kTlockTileItems && (size_t)tl.first + tl.len <= p.cnt);
          for (uint32_t i = tl.first; i < tl.first + tl.len && i < p.cnt; i++) {
            covered[p.base + i]++;
            CHECK(tl.sig == kTlockTileMixed || p.sig_of[i] == tl.sig);
          }
          out += std::string(t ? ", " : "") + "[" + std::to_string(tl.first) + ", " + std::to_string(tl.len) + ", " +
                 (tl.sig == kTlockTileMixed ? std::string("-1") : std::to_string(tl.sig)) + "]";
        }
        out += "]]";
      }
      CHECK(expect_base == n);
      for (size_t i = 0; i < n; i++) CHECK(covered[i] == 1);  // every item exactly once
      out += "]";
    }
  }
  {
    // the timelock opening's latency path: routing, the plan of a call across rounds, the buffer layout
    // (checked here only: nothing is added to the JSON)
    CHECK(!tlock_lat_routes(0, 0, 4) && tlock_lat_routes(1, 0, 4) && tlock_lat_routes(4, 4, 4));
    CHECK(!tlock_lat_routes(5, 0, 4) && !tlock_lat_routes(1, 5, 4) && !tlock_lat_routes(1, 0, 0));
    const uint64_t counts[6] = {2, 0, 1, 3, 0, 0};
    TlockLatPlan p;
    CHECK(tlock_lat_plan(counts, 6, 3, p));
    CHECK((p.sig_of == std::vector<uint32_t>{0, 0, 2, 3, 3, 3}) && (p.idle == std::vector<uint32_t>{1, 4, 5}));
    CHECK(!tlock_lat_plan(counts, 6, 2, p) && p.idle.size() == 2);  // stops at the third idle signature
    CHECK(tlock_lat_plan(counts, 0, 0, p) && p.sig_of.empty() && p.idle.empty());
    for (size_t m : {size_t(1), size_t(6), size_t(1000)})
      for (size_t n : {size_t(1), size_t(7), size_t(4096)})
        for (size_t idle : {size_t(0), size_t(3)})
          for (bool rounds : {false, true}) {
            const TlockLatLayout l = tlock_lat_layout(m, n, rounds, idle);
            CHECK(l.o_us == 96 * m && l.o_sigof == l.o_us + 48 * n && l.o_sigof % 4 == 0 && l.o_idle % 4 == 0);
            CHECK(l.in_total == l.o_idle + 4 * idle && l.o_gt >= l.in_total && l.o_gt % 64 == 0);
            CHECK(l.o_cls == l.o_gt + 576 * n && l.o_sigcls == l.o_cls + n && l.total == l.o_sigcls + m);
            CHECK(l.out_total == l.total - l.o_gt);
          }
  }
  {
    // the timelock sealing's latency path: routing and the buffer layout over the edge sizes, with its
    // overflow guard (checked here only: nothing is added to the JSON)
    CHECK(!tseal_lat_routes(0, 4) && tseal_lat_routes(1, 4) && tseal_lat_routes(4, 4));
    CHECK(!tseal_lat_routes(5, 4) && !tseal_lat_routes(1, 0) && !tseal_lat_routes(0, 0));
    static_assert(kTsealLatBytesPerItem == 665, "the header states the bytes per item");
    for (size_t n : {size_t(1), size_t(2), size_t(7), size_t(9), size_t(64), size_t(65), size_t(4096), size_t(262144)})
      for (bool rounds : {false, true}) {
        TsealLatLayout l;
        CHECK(tseal_lat_layout(n, rounds, l));
        CHECK(l.o_rounds == 0 && l.o_scalars == (rounds ? 8 * n : 0) && l.in_total == l.o_scalars + 32 * n);
        CHECK(l.o_us >= l.in_total && l.o_us - l.in_total < 64 && l.o_us % 64 == 0);
        CHECK(l.o_gt == l.o_us + 48 * n && l.o_gt % 4 == 0 && l.o_ok == l.o_gt + 576 * n);
        CHECK(l.out_total == 625 * n && l.total == l.o_ok + n && l.total == l.o_us + l.out_total);
        CHECK(l.total <= kTsealLatBytesPerItem * n + 63);
      }
    TsealLatLayout big, keep;
    const size_t most = (SIZE_MAX - 63) / kTsealLatBytesPerItem;
    CHECK(tseal_lat_layout(most, true, big) && big.total >= big.o_ok && big.total > most);
    keep = big;
    CHECK(!tseal_lat_layout(most + 1, true, big) && !tseal_lat_layout(SIZE_MAX, false, big));
    CHECK(big.total == keep.total && big.o_gt == keep.o_gt);  // untouched on overflow
  }
  {
    // the signing's latency path: routing and the buffer layout over the edge sizes, with its overflow guard
    // (checked here only: nothing is added to the JSON)
    CHECK(!sign_lat_routes(0, 4) && sign_lat_routes(1, 4) && sign_lat_routes(4, 4));
    CHECK(!sign_lat_routes(5, 4) && !sign_lat_routes(1, 0) && !sign_lat_routes(0, 0));
    static_assert(kSignLatBytesPerItem == 108 && kSignLatKeyBytes == 32, "the header states the bytes per message");
    for (size_t n : {size_t(1), size_t(2), size_t(9), size_t(65), size_t(4096), size_t(262144)})
      for (size_t mb : {size_t(0), size_t(1), size_t(31), size_t(32), size_t(301), size_t(1) << 33}) {
        SignLatLayout l;
        CHECK(sign_lat_layout(n, mb, l));
        CHECK(l.o_sk == 0 && l.o_off == 32 && l.o_off % 8 == 0 && l.o_len == l.o_off + 8 * n && l.o_len % 4 == 0);
        CHECK(l.o_msgs == l.o_len + 4 * n && l.in_total == l.o_msgs + mb);
        CHECK(l.o_out >= l.in_total && l.o_out - l.in_total < 64 && l.o_out % 64 == 0);
        CHECK(l.out_total == 96 * n && l.total == l.o_out + l.out_total);
        CHECK(l.total <= kSignLatBytesPerItem * n + mb + kSignLatKeyBytes + 63);
      }
    SignLatLayout big, keep;
    const size_t most = (SIZE_MAX - 95) / kSignLatBytesPerItem;
    CHECK(sign_lat_layout(most, 0, big) && big.total >= big.o_out && big.total > most);
    keep = big;
    CHECK(!sign_lat_layout(most + 1, 0, big) && !sign_lat_layout(SIZE_MAX, 0, big));
    CHECK(!sign_lat_layout(1, SIZE_MAX, big) && !sign_lat_layout(1, SIZE_MAX - 95, big));
    CHECK(!sign_lat_layout(most, kSignLatBytesPerItem, big));  // the item bytes and the message bytes together
    CHECK(sign_lat_layout(1, SIZE_MAX - 95 - kSignLatBytesPerItem, big) && big.total >= big.o_out);
    big = keep;
    CHECK(!sign_lat_layout(most + 1, 0, big) && big.total == keep.total && big.o_out == keep.o_out);  // untouched on overflow
  }
  out += "]}}}";
  puts(out.c_str());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "coalesce")) test_coalesce();
  else if (argc >= 3 && !strcmp(argv[1], "boltload")) test_boltload(argc - 2, argv + 2);
  else if (argc >= 2 && !strcmp(argv[1], "hostlogic")) test_hostlogic();
  else {
    fprintf(stderr, "usage: %s coalesce | boltload file.db... | hostlogic\n", argv[0]);
    return 2;
  }
  if (fails) fprintf(stderr, "%d checks failed\n", fails);
  return fails ? 1 : 0;
}
