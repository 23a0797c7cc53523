// The host arithmetic of the authenticated timelock's ragged forms (blsv_tlock_*_auth*_var; hostlogic.h
// tauth_var_fits, tauth_var_offsets, tauth_layout_var, tauth_lat_open_layout_var, tauth_lat_seal_layout_var) as a
// stand-alone program under ASan + UBSan (tools/Makefile tauthvar-asan; tests/test_tauth_var_host.py). No GPU.
//
//   tauthvar-asan <cap> <len> [<len> ...]
// prints one JSON line for a call of those lengths cut into passes of at most <cap> items: the guard's verdict and
// byte total, then per pass [base, cnt, at, bytes, words, offs, layout], layout = [o_in, secret, o_out, o_flag,
// o_offs, total]; then the two latency layouts of the whole call (with and without rounds; two idle signatures
// with rounds) and the guards at counts near SIZE_MAX. Every array lives on the heap at the caller's size, so a
// read or write past it is the sanitizer's to report; every CHECK that fails ends the run with status 1.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../drand_amd/csrc/hostlogic.h"

using namespace blsv_detail;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
      return 1;                                                   \
    }                                                             \
  } while (0)

static std::string list_of(const std::vector<size_t>& v) {
  std::string s = "[";
  for (size_t i = 0; i < v.size(); i++) s += std::string(i ? ", " : "") + std::to_string(v[i]);
  return s + "]";
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const size_t cap = strtoull(argv[1], nullptr, 10);
  if (!cap) return 2;
  const size_t n = (size_t)argc - 2;
  std::vector<uint32_t> mlens(n);  // exactly n entries
  for (size_t i = 0; i < n; i++) mlens[i] = (uint32_t)strtoul(argv[2 + i], nullptr, 10);

  size_t total = SIZE_MAX;
  const bool fits = tauth_var_fits(BLSV_KDF_SHA256_CTR, mlens.data(), n, &total);
  size_t keep = 12345;
  CHECK(!tauth_var_fits(0, mlens.data(), n, &keep) && !tauth_var_fits(2, mlens.data(), n, &keep) && keep == 12345);
  std::string out = std::string("{\"fits\": ") + (fits ? "true" : "false");
  if (!fits) {
    CHECK(total == SIZE_MAX);  // nothing touched
  } else {
    out += ", \"total\": " + std::to_string(total) + ", \"passes\": [";
    size_t at = 0;
    for (size_t base = 0; base < n; base += cap) {
      const size_t cnt = std::min(cap, n - base);
      std::vector<uint32_t> offs(cnt + 1);  // exactly cnt + 1 entries
      bool words = false;
      const size_t bytes = tauth_var_offsets(mlens.data(), base, cnt, offs.data(), &words);
      const TauthLayout l = tauth_layout_var(cnt, bytes);
      CHECK(offs[0] == 0 && offs[cnt] == bytes && bytes >= cnt && bytes <= cnt * BLSV_TLOCK_MSG_MAX);
      for (size_t i = 0; i < cnt; i++) CHECK(offs[i + 1] - offs[i] == mlens[base + i]);
      CHECK(l.o_seeds == 0 && l.o_scalars == 32 * cnt && l.o_in == 64 * cnt && l.secret >= l.o_in + bytes);
      CHECK(l.o_rounds == l.secret && l.o_rounds % 8 == 0 && l.o_us == l.o_rounds + 8 * cnt && l.o_vs == l.o_us + 48 * cnt);
      CHECK(l.o_out == l.o_vs + 32 * cnt && l.o_out % 8 == 0 && l.o_flag >= l.o_out + bytes && l.o_flag % 8 == 0);
      CHECK(l.o_offs >= l.o_flag + cnt && l.o_offs % 8 == 0 && l.total == l.o_offs + 4 * (cnt + 1));
      CHECK(l.total <= 1024 * cnt + 16);  // tauth_fits' bound on n covers the ragged staging too
      std::vector<size_t> o(offs.begin(), offs.end());
      out += std::string(base ? ", " : "") + "[" + std::to_string(base) + ", " + std::to_string(cnt) + ", " +
             std::to_string(at) + ", " + std::to_string(bytes) + ", " + (words ? "true" : "false") + ", " + list_of(o) + ", " +
             list_of({l.o_in, l.secret, l.o_out, l.o_flag, l.o_offs, l.total}) + "]";
      at += bytes;
    }
    CHECK(at == total);
    out += "]";
    if (n) {
      out += ", \"lat_open\": [";
      for (int rounds = 0; rounds < 2; rounds++) {
        const size_t idle = rounds ? 2 : 0, m = rounds ? n + idle : 1;
        TauthLatOpenLayout l;
        CHECK(tauth_lat_open_layout_var(m, n, rounds != 0, idle, total, l));
        CHECK(l.o_us == 96 * m && l.o_vs == l.o_us + 48 * n && l.o_sigof == l.o_vs + 32 * n && l.o_sigof % 4 == 0);
        CHECK(l.o_idle == l.o_sigof + (rounds ? 4 * n : 0) && l.o_offs == l.o_idle + 4 * idle && l.o_offs % 4 == 0);
        CHECK(l.o_ws == l.o_offs + 4 * (n + 1) && l.in_total == l.o_ws + total);
        CHECK(l.o_out % 64 == 0 && l.o_out >= l.in_total && l.o_out - l.in_total < 64 && l.o_cls == l.o_out + total);
        CHECK(l.o_sigcls == l.o_cls + n && l.total == l.o_sigcls + m && l.out_total == l.total - l.o_out);
        out += std::string(rounds ? ", " : "") + list_of({l.o_offs, l.o_ws, l.in_total, l.o_out, l.o_cls, l.o_sigcls, l.total});
      }
      out += "], \"lat_seal\": [";
      for (int rounds = 0; rounds < 2; rounds++) {
        TauthLatSealLayout l;
        CHECK(tauth_lat_seal_layout_var(n, rounds != 0, total, l));
        CHECK(l.o_rounds == 0 && l.o_offs == (rounds ? 8 * n : 0) && l.o_seeds == l.o_offs + 4 * (n + 1) && l.o_seeds % 4 == 0);
        CHECK(l.o_msgs == l.o_seeds + 32 * n && l.in_total == l.o_msgs + total);
        CHECK(l.o_us % 64 == 0 && l.o_us >= l.in_total && l.o_us - l.in_total < 64 && l.o_vs == l.o_us + 48 * n);
        CHECK(l.o_ws == l.o_vs + 32 * n && l.o_ok == l.o_ws + total && l.total == l.o_ok + n && l.out_total == l.total - l.o_us);
        out += std::string(rounds ? ", " : "") + list_of({l.o_offs, l.o_seeds, l.o_msgs, l.in_total, l.o_us, l.o_ws, l.o_ok, l.total});
      }
      out += "]";
    }
  }

  // the guards at counts near SIZE_MAX: refused before a length is read (one entry stands behind the pointer),
  // the largest n that passes is SIZE_MAX / 1024, and the latency layouts refuse a byte count their items cannot have
  {
    std::vector<uint32_t> one(1, 32);
    const size_t lim = SIZE_MAX / 1024;
    size_t t = 777;
    const bool refused[6] = {!tauth_var_fits(1, one.data(), lim + 1, &t), !tauth_var_fits(1, one.data(), SIZE_MAX, &t),
                             !tauth_var_fits(1, one.data(), SIZE_MAX / 256, &t), !tauth_var_fits(1, nullptr, 1, &t),
                             tauth_var_fits(1, nullptr, 0, &t) && t == 0, tauth_fits(1, 256, lim) && !tauth_fits(1, 256, lim + 1)};
    TauthLatOpenLayout ol, okeep;
    TauthLatSealLayout sl, skeep;
    CHECK(tauth_lat_open_layout_var(1, 1, false, 0, 1, ol) && tauth_lat_seal_layout_var(1, false, 1, sl));
    okeep = ol;
    skeep = sl;
    const size_t open_most = (SIZE_MAX - 67) / (190 + 512), seal_most = (SIZE_MAX - 67) / (125 + 512);
    const bool lat_refused[8] = {!tauth_lat_open_layout_var(1, 4, false, 0, 3, ol),        // fewer bytes than items
                                 !tauth_lat_open_layout_var(1, 4, false, 0, 1025, ol),     // more than 256 each
                                 !tauth_lat_open_layout_var(1, open_most + 1, false, 0, open_most + 1, ol),
                                 !tauth_lat_open_layout_var(1, SIZE_MAX, true, 1, SIZE_MAX, ol),
                                 !tauth_lat_open_layout_var(3, 1, true, 1, 1, ol),         // a signature without item or idle slot
                                 !tauth_lat_seal_layout_var(4, false, 3, sl) && !tauth_lat_seal_layout_var(4, true, 1025, sl),
                                 !tauth_lat_seal_layout_var(seal_most + 1, true, seal_most + 1, sl),
                                 !tauth_lat_seal_layout_var(SIZE_MAX, false, SIZE_MAX, sl)};
    CHECK(ol.total == okeep.total && ol.o_out == okeep.o_out && sl.total == skeep.total && sl.o_us == skeep.o_us);
    CHECK(tauth_lat_open_layout_var(1, open_most, false, 0, open_most, ol) && ol.total > open_most);
    CHECK(tauth_lat_seal_layout_var(seal_most, true, seal_most, sl) && sl.total > seal_most);
    CHECK(tauth_lat_open_layout_var(1, 4, false, 0, 1024, ol) && tauth_lat_open_layout_var(1, 4, false, 0, 4, ol));
    out += ", \"refused\": [";
    for (int k = 0; k < 6; k++) out += std::string(k ? ", " : "") + (refused[k] ? "true" : "false");
    out += "], \"lat_refused\": [";
    for (int k = 0; k < 8; k++) out += std::string(k ? ", " : "") + (lat_refused[k] ? "true" : "false");
    out += "]";
  }
  printf("%s}\n", out.c_str());
  return 0;
}
