// Internal to libblsverify.so (never installed, no C ABI): the context object and the helpers the
// C-ABI entry points (blsverify.cpp, verify.cpp, threshold.cpp, tlock.cpp, tlockr.cpp, tseal.cpp, tsealr.cpp, tcrypt.cpp, tauth.cpp, testhooks.cpp; their shared
// internals are host_internal.h) and the thread-safe service (service.cpp) share.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/blsverify.h"
#include "hostlogic.h"
#include "kernels.h"

namespace blsv_detail {

// Beacons per pipeline pass. The staging of one pass is at most kStagingBytesPerItem per item (~42.4 KB,
// 39 KB of it the Miller line staging): ~43 GB of the 288 GB at the full 2^20 chunk. A context's chunk is
// capped by blsv_set_chunk / BLSV_CHUNK and halves itself when an allocation fails (ensure_workspace).
constexpr size_t kMaxChunk = size_t(1) << 20;
constexpr size_t kMinChunk = size_t(1) << 14;  // the OOM fallback stops here
// Miller line staging holds a whole chunk. Same-box A/B (profiles/r04k_line_sub_ab.json): 128 Ki
// sub-chunks 216.9 ms, 256 Ki 215.8, the whole chunk 210.7 per 1M (one lines + one f launch instead of
// eight of each, so one wave tail instead of eight).
constexpr size_t kLineSub = kMaxChunk;
constexpr size_t kPkTable = 4096;  // member indices with a precomputed PK_i (drand groups are far smaller)
// HQ also holds the final exponentiation's park (below): 64 lanes of 48 words per 21 items, 146.3 words
// per item against HQ_WORDS = 144, plus one wave for the second range of a split pass
constexpr size_t kFexpParkWords(size_t items) { return blsk::FEXP_PARK_WORDS(items) + 48 * 64; }
constexpr size_t kHqWords(size_t items) { return std::max(items * blsk::HQ_WORDS, kFexpParkWords(items)); }
constexpr size_t kStagingBytesPerItem =
    4 * (blsk::H_WORDS + blsk::HQ_WORDS + 3 + blsk::S_WORDS + 4 * blsk::F_WORDS + blsk::MILLER_LINE_WORDS) + 3;
static_assert(kHqWords(kMaxChunk) <= (blsk::HQ_WORDS + 3) * kMaxChunk, "kStagingBytesPerItem: HQ with the park");
// Which stage owns which staging buffer of a pass, and when (all on the launch stream unless said):
//   H, h_inf   hash writes; the Miller lines pass reads (the randomized tail's sums and gather too)
//   HQ         hash, between its kernels; then free until the final exponentiation parks its 3-lane
//              products in it: the main range in the first FEXP_PARK_WORDS(main) words, the remainder of
//              a split pass behind them. A timelock pass captures its values in HQ and parks in LN.
//   S, s_inf   decompression (side stream, joined before the Miller stage) writes; the lines pass reads
//   cls        decompression writes; the lines pass adds REJ_NOT_IN_SUBGROUP, the final exponentiation
//              REJ_PAIRING, each to its own items' bytes; finish reads
//   LN         the lines pass writes; the f pass reads. Nothing else writes LN while a pass is in flight
//              (it used to double as the park: a split pass's remainder still reads its lines while
//              the main range is in its final exponentiation)
//   F          the f pass writes; the final exponentiation consumes and reuses as scratch
//   FW         the 3-lane f pass parks in it; then the final exponentiation's three slots (k_fexp.hip:
//              g then b, g^3, c)
// A split pass (hostlogic.h tail_split_main, verify.cpp pairing_check): after the f pass of the main
// range [0, main) the side stream runs the f pass and the final exponentiation of [main, cnt) beside the
// main range's final exponentiation on the launch stream. The two touch disjoint columns of F, FW and
// cls and disjoint park areas; the remainder alone reads LN; the launch stream joins the side stream
// before finish, so before the next pass's head writes S, H, HQ and cls.
// Every SoA staging object is reached through 32-bit buffer resources (soa.h): num_records is
// min(bytes, 2^31 - 1) and offsets are uint32. The largest object resource (soa_obj_rsrc over 12 Fp
// slots, 576 bytes per item) and the largest VGPR offset ((11 * 12 * n + i) * 4) must fit at the
// largest chunk, or a load past the clamp would silently read 0 (a false reject, never a fault).
static_assert(576ull * kMaxChunk < 0x7fffffffull, "SoA object resource exceeds its 31-bit num_records");
static_assert((133ull * kMaxChunk) * 4 < 0xffffffffull, "SoA VGPR byte offset exceeds 32 bits");
static_assert(48ull * 4 * kMaxChunk < 0x7fffffffull, "3-lane park slot resource exceeds 31 bits");  // park_n < 3.05 n
// Timelock opening (blsv_tlock_open*, k_tlock.hip) runs in the pipeline staging as it is: the decoded
// U table (G1_WORDS per item, AoS) with its flags and classes in H / h_inf / s_inf, f in F, the captured
// final-exponentiation values in HQ (SoA, read by k_tlock_encode through one 12-slot object resource,
// covered by the 576-byte assert above), and the encoded bytes of a host call back in F.
static_assert(blsk::G1_WORDS <= blsk::H_WORDS, "timelock: the U table does not fit the H staging");
static_assert(blsk::F_WORDS <= blsk::HQ_WORDS, "timelock: the captured Fp12 does not fit the HQ staging");
static_assert(BLSV_GT_LEN == 4 * blsk::F_WORDS, "timelock: the Gt encoding is one F staging row per item");
static_assert(BLSV_U_LEN <= 4 * blsk::S_WORDS, "timelock: a host call's compressed U bytes do not fit the S staging");
// Timelock sealing (blsv_tlock_seal*, k_tseal.hip, tseal.cpp) runs in the same staging. A pass of cnt items:
// a host call's scalars (32 bytes each) in S, cleared before the call returns; the compressed U bytes in H
// and the ok bytes in h_inf (a device call writes the caller's buffers instead); the class bytes in s_inf;
// K in HQ (SoA, as the opening captures it) and a host call's encoded bytes in F. The base of a new
// (key, round), one item through the opening's kernels before the first pass: H(MessageV2(round)) in H /
// h_inf (HQ between the hash kernels), the decoded key in S / s_inf with its class in cls[0] (cls[1] is
// the zero class byte launch_tlock_prepare wants beside a hash output), the line table in LN behind the
// one-item park of the final exponentiation, f in F, B captured in HQ, from where k_tseal_gt_table reads
// it. The only storage of its own is the two tables (tseal_state).
static_assert(BLSV_SCALAR_LEN <= 4 * blsk::S_WORDS, "sealing: a host call's scalars do not fit the S staging");
static_assert(BLSV_U_LEN <= 4 * blsk::H_WORDS, "sealing: the compressed U bytes do not fit the H staging");
static_assert(blsk::G1_WORDS <= blsk::S_WORDS, "sealing: the decoded key does not fit the S staging");
static_assert(blsk::FEXP_PARK_WORDS(1) + blsk::kTlockTabWords <= 64 * blsk::MILLER_LINE_WORDS,
              "sealing: the base's line table does not fit LN behind the park (the smallest workspace is 64 items)");

// Timelock sealing to many rounds (blsv_tlock_seal_rounds*, tsealr.cpp, tsealr.h) runs in the same staging,
// but H holds the hash output H_i until the lines pass has read it, so the one-round seal's plan (U bytes
// in H, ok bytes in h_inf) does not carry over. A pass of cnt items:
//   S          no stage of this pass touches it, so it holds everything that is not a stage's own
//              (hostlogic.h seal_rounds_layout): the table of the points P_i = k_i pk (G1_WORDS each, AoS)
//              that k_tsealr_point writes and the lines pass reads, and behind it a host call's scalars,
//              rounds, compressed U bytes and ok bytes (a device call uses the caller's buffers). The points
//              and the scalars are cleared behind the kernels that read them
//   s_inf      the class bytes launch_tseal_u writes (0, or TSEAL_REFUSED): read by every later stage
//   cls        their copy for the final exponentiation, which marks values other than 1 in it
//   H, h_inf   the hash writes (HQ between its kernels); the lines pass reads, the f pass reads h_inf
//   LN         the single-pair lines (kMillerLine1Words per item, half the staging) until the f pass has
//              read them; then the final exponentiation's park, as in a timelock opening
//   F, FW, HQ  as in a timelock opening: f, the exponentiation's scratch, the captured K_i; a host call's
//              encoded bytes back in F
// A new key is decoded into the first entry of S with its flag in s_inf[0] and its class in cls[0], before
// the first pass; k_tseal_key_table reads it from there. The only storage of its own is the key table.
static_assert(96 + BLSV_SCALAR_LEN + 8 + BLSV_U_LEN + 1 <= 4 * blsk::S_WORDS,
              "sealing to many rounds: the P table, scalars, rounds, U and ok bytes do not fit the S staging");
static_assert(96 == 4 * blsk::G1_WORDS && (96 + BLSV_SCALAR_LEN) % 8 == 0,
              "sealing to many rounds: seal_rounds_layout's P entry, and the alignment of the rounds behind the scalars");
static_assert(blsk::kMillerLine1Words <= blsk::MILLER_LINE_WORDS &&
                  blsk::FEXP_PARK_WORDS(kMaxChunk) <= blsk::MILLER_LINE_WORDS * kMaxChunk,
              "sealing to many rounds: the single-pair lines, then the park, do not fit LN");

// Timelock opening across many rounds (blsv_tlock_open_rounds*, tlockr.cpp, tlockr.h) runs in the same
// staging with the plan of a one-signature opening, plus what its many signatures need. A pass of cnt items
// that touches M <= cnt signatures with items:
//   S          a host call's compressed U bytes until launch_decompress_g1 has read them; then the M
//              decoded signatures (SoA of stride M), read by k_tlock_prepare_many
//   H, h_inf   the decoded U table with its flags; s_inf: the items' class bytes (the f pass adds
//              BLSV_REJ_TLOCK_SIG); cls: their copy for the final exponentiation, taken behind the f pass
//   LN         the word-major table of the M signatures (kTlockTabWords words each: the first half of LN
//              at most) until the f pass has read it; then the final exponentiation's park, as in an opening
//   FW         until the final exponentiation takes it as scratch (hostlogic.h open_rounds_layout, 22 bytes
//              per item of the workspace): the signatures' class and infinity bytes, and the host's plan
//              of the pass -- sig_j, sig_of and the tiles
//   F, HQ      as in a timelock opening: f, the captured E_i; a host call's encoded bytes back in F
// The pass's compressed signatures travel in in_sigs, and a host call's m class bytes wait in misc for one
// download at the end. Signatures of rounds without items are decoded in batches of their own (S, FW).
// No table outlives its pass; the only storage of its own is the 8-byte counter of prepared signatures.
static_assert(2 * blsk::kTlockTabWords <= blsk::MILLER_LINE_WORDS,
              "opening across rounds: the tables of a pass's signatures (at most one per item) exceed half of LN");
static_assert(blsk::FEXP_PARK_WORDS(kMaxChunk) <= blsk::MILLER_LINE_WORDS * kMaxChunk,
              "opening across rounds: the park does not fit LN behind the f pass");
static_assert(2 + 4 + 4 + 4 * blsk::kTlockTileWords <= 4 * 3 * blsk::F_WORDS,
              "opening across rounds: the signatures' flags and the plan of a pass do not fit the FW staging");

// Timelock in one call (blsv_tlock_decrypt* / blsv_tlock_encrypt*, tcrypt.cpp, k_tmask.hip): each of the four
// timelock passes above with its last stage swapped -- k_tmask reads the captured values in HQ where
// k_tlock_encode read them, and nothing else in the pass moves. What a host form stages for a pass of cnt items
// of mlen bytes:
//   F          free behind the final exponentiation (the encoded bytes used to come back through it): the
//              cnt x mlen input bytes (ciphertexts, or plaintexts) at its start, uploaded behind the
//              exponentiation, and the cnt x mlen output bytes behind them, from where the download takes them
//              with the class / ok bytes of the pass it runs. An encrypting pass clears the input part behind
//              the kernel
//   HQ         the captured values, as ever; an encrypting pass (host or device form) clears the cnt x 576
//              bytes of K behind the mask kernel, also when the pass failed
// A device form reads and writes the caller's buffers in place. No storage of its own.
static_assert(2 * BLSV_TLOCK_MSG_MAX <= 4 * blsk::F_WORDS,
              "timelock in one call: a pass's input and output bytes do not fit the F staging");

// Authenticated timelock (blsv_tlock_encrypt_auth* / blsv_tlock_decrypt_auth*, tauth.cpp, k_tauth.hip): each of
// the four timelock passes above with its last stage swapped once more -- k_tauth_seal_tail / k_tauth_open_tail
// read the captured values in HQ where k_tmask read them. Nothing else in a pass moves, and the opening tail
// also reads what the pass left behind the final exponentiation: the decoded U table in H / h_inf and the
// class bytes in s_inf (it writes BLSV_REJ_TLOCK_AUTH there). The passes always run on device pointers. What
// is not a stage's own lives in ONE device buffer of the feature's (tauth_state::buf, hostlogic.h
// tauth_layout), sized for a pass of cnt <= cap items and allocated at the first authenticated call -- the
// pipeline staging is not used for it: S holds the P table in a pass across rounds and U bytes or signatures
// in an opening, and F is the exponentiation's in three of the four passes, so no one buffer is free in all:
//   a device form, encrypting    the derived scalars (32 bytes per item) that k_tauth_derive writes and the
//                                sealing kernels read, cleared behind them, also when the pass failed
//   a host form, encrypting      the seeds, the derived scalars and the plaintexts ([0, secret): cleared behind
//                                the kernels, also when the pass failed; seeds and plaintexts are uploaded
//                                straight from the caller's memory), the rounds, and the pass's U, V, W and ok
//                                bytes, from where the download takes them
//   a host form, decrypting      the pass's U, V and W bytes, its message bytes and its class bytes
// A device form that decrypts stages nothing. HQ's captured K is cleared as in blsv_tlock_encrypt (mask_wipe).
// A ragged host form (blsv_tlock_*_auth*_var, hostlogic.h tauth_layout_var) keeps the same parts with the two
// message regions sized by the pass's byte count, and the pass's cnt + 1 prefix offsets behind the flags.
// T1 is the sealing's (tseal_state::t1), built on first use by whichever call needs it first.
static_assert(BLSV_SEED_LEN == 32 && BLSV_V_LEN == 32 && BLSV_SCALAR_LEN == 32,
              "authenticated timelock: tauth_layout's rows of seeds, V bytes and scalars");
static_assert(blsk::kTauthSeedLen == BLSV_SEED_LEN && blsk::kTauthVLen == BLSV_V_LEN,
              "authenticated timelock: the header's sizes are the kernels'");
static_assert(32 + 32 + 8 + BLSV_U_LEN + 32 + 2 * BLSV_TLOCK_MSG_MAX + 1 + 16 <= 1024,
              "authenticated timelock: tauth_fits bounds a pass's staging by 1 KiB per item");
static_assert(blsk::G1_WORDS <= blsk::H_WORDS, "authenticated timelock: the U table the opening tail reads is the pass's own in H");

struct DBuf {
  void* p = nullptr;
  size_t sz = 0;
  ~DBuf() {
    if (p) (void)hipFree(p);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    sz = 0;
  }
  hipError_t ensure(size_t need) {
    if (need <= sz) return hipSuccess;
    if (p) {
      (void)hipFree(p);
      p = nullptr;
      sz = 0;
    }
    size_t want = std::max(need, size_t(256));
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) sz = want;
    return e;
  }
  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

// Page-locked host staging (hipHostMalloc): copies from it are truly asynchronous.
struct PinBuf {
  void* p = nullptr;
  size_t sz = 0;
  ~PinBuf() {
    if (p) (void)hipHostFree(p);
  }
  hipError_t ensure(size_t need) {
    if (need <= sz) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    sz = 0;
    const size_t want = std::max(need + need / 2, size_t(4096));
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) sz = want;
    return e;
  }
  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

}  // namespace blsv_detail
using namespace blsv_detail;

// Stage timing (blsv_profile_*): HIP events recorded around every stage launch on the launch stream.
// ST_RLC: the randomized path's combination stage with its gather / scatter (blsv_verify_*_rlc); that
// path's group checks and exact fallback are timed as ST_MILLER / ST_FEXP launches of their own.
enum Stage {
  ST_HASH = 0,
  ST_DECOMP = 1,
  ST_MILLER = 2,
  ST_FEXP = 3,
  ST_FINISH = 4,
  ST_LAT = 5,
  ST_RLC = 6,
  ST_TLOCK = 7,  // timelock opening: sigma's preparation and the f pass (its final exponentiation is ST_FEXP)
  ST_N = 8
};
// One record is one launch of a stage over `items` items. A split pass's Miller and final-exponentiation
// records carry a second span (a2, b2: the remainder on the side stream); blsv_profile_read adds the two,
// so time in which the spans overlap counts twice and a pass's stage times may exceed its wall time.
struct ProfRec {
  int stage;
  size_t items;
  hipEvent_t a, b;
  hipEvent_t a2 = nullptr, b2 = nullptr;
};

// Cutover between the latency path (one workgroup per item, k_lat.hip) and the batch pipeline: a batch
// of at most this many items runs on the latency path. BLSV_LAT_MAX overrides it (0 = batch pipeline
// only). Any value is clamped to kMaxChunk: the latency kernels write one class byte per item into the
// chunk-sized class buffer, so a larger batch always takes the chunked pipeline.
// Randomized batch verification (rlc.h): items per shared pairing check. blsv_set_rlc_group rounds to a
// power of two in [kRlcGroupMin, kRlcGroupMax]. Default from profiles/rlc_bench.json (1M rounds, ms per
// step at G = 32 / 64 / 256 / 1024): all valid 219 / 212 / 212 / 217, one bad round 229 / 222 / 223 / 227,
// 0.1% bad rounds 236 / 244 / 301 / 433 -- a smaller group's checks cost little, its fallback much less.
constexpr size_t kRlcGroupDefault = 64;
constexpr size_t kRlcGroupMin = 8, kRlcGroupMax = 4096;
constexpr size_t kLatMaxDefault = 1536;  // profiles/r04zk_latency_sweep.json: the paths cross near 1,750
// Default chunk: BLSV_CHUNK (items, rounded up to a multiple of 64, clamped to [kMinChunk, kMaxChunk]),
// else kMaxChunk.
inline size_t chunk_env() {
  static const size_t v = [] {
    const char* e = getenv("BLSV_CHUNK");
    if (!e) return kMaxChunk;
    char* end = nullptr;
    errno = 0;
    const unsigned long long x = strtoull(e, &end, 10);
    if (end == e || *end != '\0' || errno == ERANGE || e[0] == '-' || x == 0) {
      fprintf(stderr, "blsverify: ignoring BLSV_CHUNK=\"%s\" (not a positive integer); chunk stays %zu\n", e, kMaxChunk);
      return kMaxChunk;
    }
    const size_t c = (size_t)std::min<unsigned long long>(std::max<unsigned long long>(x, kMinChunk), kMaxChunk);
    return (c + 63) & ~size_t(63);
  }();
  return v;
}

inline size_t lat_max_env() {
  static const size_t v = [] {
    const char* e = getenv("BLSV_LAT_MAX");
    if (!e) return kLatMaxDefault;
    char* end = nullptr;
    errno = 0;
    const unsigned long long x = strtoull(e, &end, 10);
    if (end == e || *end != '\0' || errno == ERANGE || e[0] == '-') {
      fprintf(stderr, "blsverify: ignoring BLSV_LAT_MAX=\"%s\" (not a non-negative integer); cutover stays %zu\n", e,
              kLatMaxDefault);
      return kLatMaxDefault;
    }
    return (size_t)std::min<unsigned long long>(x, kMaxChunk);
  }();
  return v;
}

// Cutover of the timelock opening's latency path (blsv_set_tlock_lat_max): BLSV_TLOCK_LAT_MAX, parsed as
// BLSV_LAT_MAX is, else 0 = off.
inline size_t tlock_lat_max_env() {
  static const size_t v = [] {
    const char* e = getenv("BLSV_TLOCK_LAT_MAX");
    if (!e) return size_t(0);
    char* end = nullptr;
    errno = 0;
    const unsigned long long x = strtoull(e, &end, 10);
    if (end == e || *end != '\0' || errno == ERANGE || e[0] == '-') {
      fprintf(stderr, "blsverify: ignoring BLSV_TLOCK_LAT_MAX=\"%s\" (not a non-negative integer); it stays 0\n", e);
      return size_t(0);
    }
    return (size_t)std::min<unsigned long long>(x, kMaxChunk);
  }();
  return v;
}

// Cutover of the timelock sealing's latency path (blsv_set_tseal_lat_max): BLSV_TSEAL_LAT_MAX, parsed as
// BLSV_TLOCK_LAT_MAX is, else 0 = off.
inline size_t tseal_lat_max_env() {
  static const size_t v = [] {
    const char* e = getenv("BLSV_TSEAL_LAT_MAX");
    if (!e) return size_t(0);
    char* end = nullptr;
    errno = 0;
    const unsigned long long x = strtoull(e, &end, 10);
    if (end == e || *end != '\0' || errno == ERANGE || e[0] == '-') {
      fprintf(stderr, "blsverify: ignoring BLSV_TSEAL_LAT_MAX=\"%s\" (not a non-negative integer); it stays 0\n", e);
      return size_t(0);
    }
    return (size_t)std::min<unsigned long long>(x, kMaxChunk);
  }();
  return v;
}

// Cutovers of the authenticated timelock's latency path (blsv_set_tauth_lat_max): BLSV_TAUTH_OPEN_LAT_MAX /
// BLSV_TAUTH_SEAL_LAT_MAX, parsed as BLSV_TSEAL_LAT_MAX is, else 0 = off. Read once per context.
inline size_t tauth_lat_max_env(const char* name) {
  const char* e = getenv(name);
  if (!e) return 0;
  char* end = nullptr;
  errno = 0;
  const unsigned long long x = strtoull(e, &end, 10);
  if (end == e || *end != '\0' || errno == ERANGE || e[0] == '-') {
    fprintf(stderr, "blsverify: ignoring %s=\"%s\" (not a non-negative integer); it stays 0\n", name, e);
    return 0;
  }
  return (size_t)std::min<unsigned long long>(x, kMaxChunk);
}

// Cutover of the signing's latency path (blsv_set_sign_lat_max): BLSV_SIGN_LAT_MAX, parsed as
// BLSV_TSEAL_LAT_MAX is, else 0 = off. Read once per context.
inline size_t sign_lat_max_env() { return tauth_lat_max_env("BLSV_SIGN_LAT_MAX"); }

struct rlc_state {
  size_t group = kRlcGroupDefault;
  bool seed_pinned = false;  // blsv_test_rlc_seed
  uint8_t seed[32] = {0};
  uint64_t groups = 0, groups_failed = 0, items_exact = 0;  // blsv_rlc_stats
  DBuf part, gH, gS, g_hinf, g_sinf, gcls, cH, cS, c_hinf, c_sinf, ccls, fail, out96;
  PinBuf host;  // group verdicts down, failing group indices up
};

// Timelock opening (blsv_tlock_open*): the prepared form of the LAST sigma -- its 96 bytes, decode
// class and flag, and the device table of its 68 lines' P-independent coefficients. One entry: a call
// with another sigma replaces it.
struct tlock_state {
  bool valid = false;
  uint8_t sig[96] = {0};
  uint8_t cls = 0;
  uint64_t prepared = 0, items = 0;  // blsv_tlock_stats
  DBuf d_sig, S, s_inf, s_cls, tab;
};

// Timelock sealing (blsv_tlock_seal*): the LAST base -- the 48 key bytes and the round it was built
// for, and T2, the table of its powers. T1 (the generator's multiples) is built once per context. One
// entry: a call with another key or round replaces it.
struct tseal_state {
  bool valid = false, t1_built = false;
  uint8_t pk[48] = {0};
  uint64_t round = 0;
  uint64_t bases = 0, items = 0;  // blsv_tlock_seal_stats
  DBuf t1, t2;
};

// Timelock sealing to many rounds (blsv_tlock_seal_rounds*): the LAST key -- its 48 bytes and TK, the
// table of its multiples (T1's layout). One entry: a call with another key replaces it.
struct tsealr_state {
  bool valid = false;
  uint8_t pk[48] = {0};
  uint64_t keys = 0, items = 0;  // blsv_tlock_seal_rounds_stats
  DBuf tk;
};

// Timelock opening across many rounds (blsv_tlock_open_rounds*): no cache. dense_min: the shortest run
// that gets uniform tiles (blsv_set_tlock_dense_min; hostlogic.h kTlockDenseMinDefault); prepared: the
// device counter k_tlock_prepare_many adds to (a device call reads no class back, so the host cannot count).
struct tlockr_state {
  size_t dense_min = kTlockDenseMinDefault;
  uint64_t items = 0;  // blsv_tlock_open_rounds_stats
  DBuf prepared;
};

// Timelock opening on the latency path (blsv_set_tlock_lat_max, k_lat_tlock.hip): host calls of up to
// lat_max items, one workgroup per item. It shares nothing with the batch paths: its own device buffer
// (hostlogic.h tlock_lat_layout) and host staging of a call's results, its own counters; the sigma cache
// of tlock_state, the pipeline staging and every other counter stay as they are.
struct tlock_lat_state {
  size_t lat_max = 0;                // never above the chunk
  uint64_t launches = 0, items = 0;  // blsv_tlock_lat_stats
  DBuf buf;
  std::vector<uint8_t> up, down;
  TlockLatPlan plan;
};

// Timelock sealing on the latency path (blsv_set_tseal_lat_max, k_lat_tseal.hip): host calls of up to
// lat_max items, one workgroup per item. Its own device buffer (hostlogic.h tseal_lat_layout), host staging
// and counters; it reads T1 (tseal_state) and the key table TK (tsealr_state, through the key cache, whose
// `keys` counter therefore counts a table whichever path built it). The base cache of tseal_state, the
// sigma cache, the pipeline staging and every other counter stay as they are.
struct tseal_lat_state {
  size_t lat_max = 0;                // never above the chunk
  uint64_t launches = 0, items = 0;  // blsv_tseal_lat_stats
  DBuf buf;
  std::vector<uint8_t> up, down;  // the scalars in `up` are cleared before the entry returns
};

// Authenticated timelock (blsv_tlock_encrypt_auth* / blsv_tlock_decrypt_auth*): the one buffer of its own
// (hostlogic.h tauth_layout; the plan is above). No cache and no counter: a call counts in the pass it runs.
struct tauth_state {
  DBuf buf;
  std::vector<uint32_t> offs;  // the ragged forms: a pass's prefix offsets on the host, alive until its upload has run
};

// Authenticated timelock on the latency path (blsv_set_tauth_lat_max, k_lat_tauth_open.hip /
// k_lat_tauth_seal.hip): host calls of up to open_max (decrypting) or seal_max (encrypting) items, one
// workgroup per item. Switches, device buffer (hostlogic.h tauth_lat_open_layout / tauth_lat_seal_layout),
// host staging and counters of its own: the other latency switches are not consulted, and the batch paths'
// counters, the sigma cache and the (key, round) base cache stay as they are. It reads T1 (tseal_state) and,
// encrypting, the key table TK through the key cache (tsealr_state), as tseal_lat_state does.
struct tauth_lat_state {
  size_t open_max = 0, seal_max = 0;  // never above the chunk
  uint64_t open_launches = 0, open_items = 0, seal_launches = 0, seal_items = 0;  // blsv_tauth_lat_stats
  int walk_waves = 8;  // the waves that share the check's walk: 8, or 1 (blsv_test_tauth_walk_waves)
  DBuf buf;
  std::vector<uint8_t> up, down;  // an encrypting call's seeds and plaintexts in `up` are cleared before it returns
  TlockLatPlan plan;
};

// Signing on the latency path (blsv_set_sign_lat_max, k_lat_sign.hip): blsv_sign calls of up to lat_max
// messages, one workgroup per message. Its own device buffer (hostlogic.h sign_lat_layout), host staging and
// counters; the pipeline staging, the batch signer's c->sk and every other counter stay as they are.
struct sign_lat_state {
  size_t lat_max = 0;                // never above the chunk
  uint64_t launches = 0, items = 0;  // blsv_sign_lat_stats
  DBuf buf;
  std::vector<uint8_t> up, down;  // the key in `up` is cleared before the entry returns
};

struct blsv_ctx {
  int device = 0;
  bool prof = false;
  size_t chunk = chunk_env();                      // items per pipeline pass (blsv_set_chunk)
  size_t lat_max = std::min(lat_max_env(), chunk);  // latency-path cutover, never above the chunk
  uint64_t oom_halvings = 0;                        // times ensure_workspace halved the chunk
  // one round of the single-lane Miller f pass (64 lanes x 4 SIMDs x the device's compute units, read
  // in blsv_create), and the round a pass is split by (hostlogic.h tail_split_main; blsv_test_tail_split)
  size_t tail_q_dev = 0, tail_q = 0;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> event_pool;
  hipStream_t stream = nullptr;
  // decompression runs beside hash-to-G2 (they are independent): a side stream forked from and
  // joined back into the launch stream with these two events
  hipStream_t side = nullptr;
  hipEvent_t fork_ev = nullptr, join_ev = nullptr;
  // the speculative VerifyRecovered's hash-to-G2 of its message from the start of a threshold round
  // (threshold.cpp spec_recover_launch, launch_lat_hash_key): a second side stream, joined into `side`
  // through hash_ev[slot]. Three streams in all: the boxes run 4 hardware queues per process.
  hipStream_t side2 = nullptr;
  hipEvent_t hash_ev[2] = {nullptr, nullptr};
  std::string err;
  // group
  bool has_group = false;
  size_t t = 0, n = 0;
  DBuf commits, commit_inf;
  std::vector<uint8_t> group_bytes;  // the commitments of the current group (set_group is a no-op on a repeat)
  // PubPoly.Eval(i) for every share index i < min(n, kPkTable), computed once per group on its first
// partials call; indices beyond the table are evaluated per batch
  DBuf pk_all, pk_all_inf;
  size_t pk_all_n = 0;
  bool pk_all_built = false;
  // explicit-pk override (verify_messages with pk48)
  DBuf pk_tab, pk_inf;
  uint8_t pk_cache[48];
  bool pk_cache_valid = false;
  // staging workspace (cap items, at most chunk)
  size_t cap = 0;
  DBuf H, S, F, FW, LN, h_inf, s_inf, cls;
  DBuf HQ;  // hash-to-G2 phase staging (kernels.h HQ_WORDS per item)
  // inputs / outputs
  DBuf in_sigs, in_msgs, in_off, in_len, in_rounds, seeds, bitmap, first_bad, sk, idx, lambdas, scratch, out,
      pp_tab, pp_inf, sel, g1_cls, misc;
  // one packed upload / download per service batch (svc_verify_mixed)
  PinBuf pin;
  // pinned staging of the small copies on the main stream (blsverify.cpp h2d / download_sync): uploads
  // append at io_up_off and wrap after a synchronisation of the stream
  PinBuf io_up, io_down;
  size_t io_up_off = 0;
  // speculative recovery beside a round's partial verification (threshold.cpp spec_recover_*): two
  // slots (V1, V2), each with its decoded shares, Lagrange coefficients, products and output
  struct SpecSlot {
    DBuf sig, S, s_inf, cls, sel, lam, scratch, out, vmsg, voff, vlen, vcls;
    DBuf hout, saff;  // H(msg) and the recovered signature's affine point (kernels.h kLat*Words)
    PinBuf host;  // staged sigma bytes + indices in, the 96-byte result out (async copies only)
  } spec[2];
  uint64_t spec_hits = 0, spec_misses = 0;  // speculative recoveries kept / recomputed
  DBuf arena;
  // randomized batch verification (blsv_verify_*_rlc, rlc.h): the lanes' partial sums, one H / S slot per
  // group with flags and class bytes, the compact staging of the exact fallback, the failing groups
  rlc_state rlc;
  tlock_state tlock;
  tseal_state tseal;
  tsealr_state tsealr;
  tlockr_state tlockr;
  tlock_lat_state tlock_lat;
  tseal_lat_state tseal_lat;
  tauth_lat_state tauth_lat;
  tauth_state tauth;
  sign_lat_state sign_lat;
};

#define HIPCHK(ctx, expr)                                                             \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) return fail((ctx), BLSV_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

inline int fail(blsv_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}


// Pipeline staging for min(cnt, chunk) items (rounded to 64). On an out-of-memory failure every
// staging buffer is released, the context's chunk halves (not below kMinChunk) and the allocation is
// retried, so several contexts or ranks sharing one GPU degrade to smaller passes instead of failing.
int ensure_workspace(blsv_ctx* c, size_t cnt);
// Releases the pipeline staging (the next call reallocates what it needs).
void release_workspace(blsv_ctx* c);

// One mixed batch of the thread-safe service (service.cpp): item i verifies sigs96[i] over message i
// (msgs[off[i] .. off[i] + lens[i])) against entry idx[i] of the device G1 table (d_tab, d_tab_inf).
// The latency path up to lat_max items, else the batch pipeline in chunk-sized passes. cls_out gets
// BLSV_REJ_* per item. One host-to-device copy of everything, one device-to-host copy of the classes.
int svc_verify_mixed(blsv_ctx* c, size_t n, const uint8_t* msgs, const uint64_t* off, const uint32_t* lens,
                     const uint8_t* sigs96, const uint32_t* idx, const uint32_t* d_tab, const uint8_t* d_tab_inf,
                     uint8_t* cls_out);
