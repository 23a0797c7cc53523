// Kernel launchers of the beacon-verification engine (host-callable, defined in k_*.hip).
// Stage pipeline for a batch of beacons (each stage one lane per beacon, SoA staging in HBM):
//   hash   : message derivation + hash-to-G2            -> H[i]  (affine, 4 Fp slots) + h_inf[i]
//   decomp : sigma decompression                          -> S[i]  (affine, 4 Fp slots) + s_inf[i], cls[i]
//            (+ the psi subgroup check as kernels of its own on the randomized and timelock paths)
//   miller : e(pk_i, H_i) * e(-g1, S_i) multi-Miller loop -> F[i]  (Fp12, 12 Fp slots); the per-item path
//            closes S_i's psi subgroup check on the loop's own [|x|]S_i -> cls[i]
//   fexp   : final exponentiation, == 1                  -> cls[i] (REJ_PAIRING on mismatch)
//   finish : verdict bitmap (ballot) + first bad index (atomicMin)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace blsk {

constexpr int H_WORDS = 48;   // affine G2
constexpr int S_WORDS = 48;   // affine G2
constexpr int F_WORDS = 144;  // Fp12
constexpr int G1_WORDS = 24;  // affine G1 (x, y Montgomery), AoS entry in pk tables

// Chained beacons (chain.VerifyBeacon with prev = the previous round's signature): item i has
// round first_round + i; with s = (i + seg_phase) / seg_len its prev is seeds[s] (length seed0_len
// for s == 0, else 96) when i == 0 or (i + seg_phase) % seg_len == 0, otherwise sigs[i-1].
// seg_len = n gives one continuous chain. seg_phase (< seg_len) is the position of item 0 inside
// its segment: a shard that starts mid-segment passes its halo (the true previous signature) as
// seeds[0] and the following segment seeds as seeds[1..] (shard.py, bench.py --total-rounds).
struct ChainedSrc {
  const uint8_t* sigs;   // n x 96 (global, whole batch)
  const uint8_t* seeds;  // n_seg x 96 slots
  uint64_t first_round;
  uint64_t seg_len;
  uint32_t seed0_len;  // 32 (genesis GroupHash) or 96
  uint64_t seg_phase;  // 0 for the generator and every host-buffer entry point
};

// Every hash launcher takes Q: HQ_WORDS x cnt words of SoA staging between its three kernels.
constexpr int HQ_WORDS = 144;
void launch_hash_chained(const ChainedSrc& src, size_t base, size_t cnt, uint32_t* H, uint8_t* h_inf,
                         uint32_t* Q, hipStream_t st);
// chain.VerifyBeaconV2: msg = sha256(BE64(round)); rounds == nullptr -> first_round + base + i
void launch_hash_unchained(const uint64_t* rounds, uint64_t first_round, size_t base, size_t cnt, uint32_t* H,
                           uint8_t* h_inf, uint32_t* Q, hipStream_t st);
// arbitrary messages (Scheme.VerifyRecovered / VerifyPartial / Sign): msg i = msgs[off[i] .. off[i]+len[i])
void launch_hash_messages(const uint8_t* msgs, const uint64_t* off, const uint32_t* len, size_t cnt,
                          uint32_t* H, uint8_t* h_inf, uint32_t* Q, hipStream_t st);
// 96-byte compressed signatures at sigs + (base+i)*stride + offset
void launch_decompress_g2(const uint8_t* sigs, size_t stride, size_t offset, size_t base, size_t cnt, uint32_t* S,
                          uint8_t* s_inf, uint8_t* cls, hipStream_t st);
// pk for item i: pk_tab[pk_idx ? pk_idx[i] : 0] (G1_WORDS each) with pk_inf flags
// LN: line staging for `sub` beacons (MILLER_LINE_WORDS each); the chunk runs in sub-chunks of `sub`
// (the host passes the whole chunk: engine_ctx.h kLineSub)
// check_subgroup: the lines pass also closes S_i's psi subgroup check on its own [|x|]S_i and writes
// cls[i] = REJ_NOT_IN_SUBGROUP where it fails (for S decoded by launch_decompress_g2_only); without
// it cls is only read
constexpr int MILLER_LINE_WORDS = 68 * 2 * 6 * 12;
void launch_miller(const uint32_t* pk_tab, const uint8_t* pk_inf, const uint32_t* pk_idx, const uint32_t* H,
                   const uint8_t* h_inf, const uint32_t* S, const uint8_t* s_inf, uint8_t* cls, size_t cnt,
                   uint32_t* F, uint32_t* LN, size_t sub, uint32_t* park, bool check_subgroup, hipStream_t st);
// launch_miller's two halves, for a caller that sequences them itself (cnt = the pass, the stride of
// H / S / F / cls): the lines pass of the items [base, base + m) (base a multiple of sub, m <= sub),
// and the f pass of a range [base, base + m) inside one sub-chunk whose lines are staged. single_lane
// forces k_miller_f whatever m is: the form with the least SIMD time, for a small range that runs
// beside other work instead of alone.
void launch_miller_lines(const uint32_t* pk_tab, const uint8_t* pk_inf, const uint32_t* pk_idx, const uint32_t* H,
                         const uint8_t* h_inf, const uint32_t* S, const uint8_t* s_inf, uint8_t* cls, size_t cnt,
                         size_t base, size_t m, uint32_t* LN, size_t sub, bool check_subgroup, hipStream_t st);
void launch_miller_f(const uint32_t* LN, size_t sub, const uint8_t* cls, size_t cnt, size_t base, size_t m,
                     uint32_t* F, uint32_t* park, bool single_lane, hipStream_t st);
// park: TRI_PARK_WORDS(sub) words of scratch for the 3-lane f pass (48 words per lane, 21 items per wave)
constexpr size_t TRI_PARK_WORDS(size_t items) { return 48 * 64 * ((items + 20) / 21); }
// The final exponentiation of the m items [base, base + m) of a pass whose staging has stride n: their
// columns of F are clobbered; W = 3 * n * F_WORDS words of staging (the range's columns are used); out
// (optional: test hook, timelock): the exponentiated values (SoA of stride n, the range's columns).
// cls gets REJ_PAIRING where the value is not 1; without out that is decided by a comparison and the
// value itself is never formed (pairing.h fexp_step4_is_one).
// park: FEXP_PARK_WORDS(m) words of scratch for the 3-lane products' parked partial results; ranges
// that run side by side need disjoint park areas.
constexpr size_t FEXP_PARK_WORDS(size_t items) { return TRI_PARK_WORDS(items); }
void launch_final_exp(uint32_t* F, uint32_t* W, size_t n, size_t base, size_t m, uint8_t* cls, hipStream_t st,
                      uint32_t* park, uint32_t* out = nullptr);
// bitmap bit (base+i) = (cls[i] == 0); bitmap must cover whole 64-bit words;
// first_bad = label0 + min rejected index (label0 = first_round -> ROUND numbers)
void launch_finish(const uint8_t* cls, size_t base, size_t cnt, uint64_t* bitmap, unsigned long long* first_bad,
                   uint64_t label0, hipStream_t st);

// ---- randomized batch verification (k_rlc.hip, rlc.h): the combination stage of one pass.
// Groups of `group` consecutive items (a power of two >= kRlcLaneItems; the last may be short); per
// group A = sum r_i H_i and B = sum r_i S_i over the items with cls == 0 (an item's point at infinity
// is left out of its own sum only), r_i = first 8 bytes of SHA-256(seed || BE64(index0 + i)). The sums
// land in affine form in slot g of GH / GS (H / S layout, stride rlc_groups(cnt, group)) with
// g_hinf / g_sinf. part: 2 * kRlcPartWords * rlc_lanes(cnt) words for the lanes' Jacobian partial sums.
constexpr size_t kRlcLaneItems = 8;
constexpr size_t kRlcPartWords = 72;
constexpr size_t rlc_lanes(size_t cnt) { return (cnt + kRlcLaneItems - 1) / kRlcLaneItems; }
constexpr size_t rlc_groups(size_t cnt, size_t group) { return (cnt + group - 1) / group; }
void launch_rlc_sums(const uint32_t* H, const uint8_t* h_inf, const uint32_t* S, const uint8_t* s_inf,
                     const uint8_t* cls, size_t cnt, uint64_t index0, const uint32_t* seed_words, size_t group,
                     uint32_t* part, uint32_t* GH, uint8_t* g_hinf, uint32_t* GS, uint8_t* g_sinf, hipStream_t st);
// exact fallback: the items of the failing groups fail[0 .. ) (ascending group indices) copied into m
// compact slots (H / S layout of stride m, flags, class bytes), and their classes copied back
void launch_rlc_gather(const uint32_t* fail, size_t group, size_t m, const uint32_t* H, const uint8_t* h_inf,
                       const uint32_t* S, const uint8_t* s_inf, const uint8_t* cls, size_t cnt, uint32_t* CH,
                       uint8_t* c_hinf, uint32_t* CS, uint8_t* c_sinf, uint8_t* ccls, hipStream_t st);
void launch_rlc_scatter(const uint32_t* fail, size_t group, size_t m, const uint8_t* ccls, uint8_t* cls, size_t cnt,
                        hipStream_t st);
// test hook: ng staged points (stride ng) in the 96-byte compressed form
void launch_rlc_compress(const uint32_t* GP, const uint8_t* g_inf, size_t ng, uint8_t* out96, hipStream_t st);

// ---- timelock opening (k_tlock.hip, tlock.h): E_i = e(U_i, sigma)^3 under one shared sigma.
// prepare: sigma's decoded one-entry staging (launch_decompress_g2 with cnt = 1: S of stride 1, flag,
// class) -> tab, kTlockTabWords words of P-independent line coefficients (untouched when sigma did not
// decode or is the point at infinity). f: U / u_inf / cls as launch_decompress_g1 wrote them for cnt
// items, sig_inf = sigma's device flag -> F (SoA of stride cnt; 1 for a pair with a point at infinity,
// untouched for cls != 0). encode: the captured values E (SoA of stride cnt) -> cnt x 576 bytes (out
// 4-byte aligned), zeros where cls != 0.
constexpr size_t kTlockTabWords = 68 * 3 * 24;
void launch_tlock_prepare(const uint32_t* S, const uint8_t* s_inf, const uint8_t* s_cls, uint32_t* tab, hipStream_t st);
void launch_tlock_f(const uint32_t* tab, const uint32_t* U, const uint8_t* u_inf, const uint8_t* cls,
                    const uint8_t* sig_inf, size_t cnt, uint32_t* F, hipStream_t st);
void launch_tlock_encode(const uint32_t* E, const uint8_t* cls, size_t cnt, uint8_t* out, hipStream_t st);

// ---- timelock opening across many rounds (k_tlockr.hip, tlockr.h): E_i = e(U_i, sigma_j)^3, round j owning a
// run of consecutive items. prepare_many: the staging launch_decompress_g2 filled for the pass's M
// signatures (stride M) -> tab, kTlockTabWords x M words, word w of signature j at tab[w * M + j] (a column
// is untouched when its sigma did not decode or is the point at infinity); *prepared += the sigmas that
// decoded. f_tiles: one one-wave workgroup per tile of kTlockTileWords words (first item, length <= 64,
// signature index < M or kTlockTileMixed), the n_uniform uniform tiles first and the n_mixed mixed ones
// behind them; sig_of[i] = item i's signature index (read by mixed tiles); U / u_inf / cls as
// launch_decompress_g1 wrote them for cnt items -> F as launch_tlock_f leaves it, and cls[i] = 9
// (BLSV_REJ_TLOCK_SIG) where cls[i] was 0 and the item's sigma did not decode. scatter_classes:
// dst[sig_j[k]] = src[k] for k < M.
constexpr uint32_t kTlockTileMixed = 0xffffffffu;
constexpr size_t kTlockTileWords = 3;
void launch_tlock_prepare_many(const uint32_t* S, const uint8_t* s_inf, const uint8_t* s_cls, size_t M, uint32_t* tab,
                               unsigned long long* prepared, hipStream_t st);
void launch_tlock_f_tiles(const uint32_t* tiles, size_t n_uniform, size_t n_mixed, const uint32_t* sig_of,
                          const uint32_t* tab, size_t M, const uint8_t* sig_inf, const uint8_t* sig_cls,
                          const uint32_t* U, const uint8_t* u_inf, uint8_t* cls, size_t cnt, uint32_t* F,
                          hipStream_t st);
void launch_tlock_scatter_classes(const uint8_t* src, const uint32_t* sig_j, size_t M, uint8_t* dst, hipStream_t st);

// ---- timelock sealing (k_tseal.hip, tseal.h): U_i = k_i G1, K_i = B^k_i under one shared base B.
// g1_table: T1 (kTsealT1Words words), the multiples j 16^w G1. gt_table: B = the base's Fp12 (144 words,
// Montgomery, tower order: a captured final-exponentiation value of stride 1) -> T2 (kTsealT2Words words),
// the powers B^(j 16^w). u: cnt scalars of 32 bytes big-endian -> us (cnt x 48 bytes), ok and cls (one byte
// each; a scalar == 0 mod r gets zeros, ok = 0, cls != 0). gt: the same scalars and cls -> E (SoA of stride
// cnt, what launch_tlock_encode reads; untouched where cls != 0).
constexpr size_t kTsealT1Words = 64 * 15 * 24;
constexpr size_t kTsealT2Words = 64 * 15 * 144;
void launch_tseal_g1_table(uint32_t* T1, hipStream_t st);
void launch_tseal_gt_table(const uint32_t* B, uint32_t* T2, hipStream_t st);
void launch_tseal_u(const uint32_t* T1, const uint8_t* scalars, size_t cnt, uint8_t* us, uint8_t* ok, uint8_t* cls,
                    hipStream_t st);
void launch_tseal_gt(const uint32_t* T2, const uint8_t* scalars, const uint8_t* cls, size_t cnt, uint32_t* E,
                     hipStream_t st);

// ---- timelock sealing to many rounds (k_tsealr.hip, tsealr.h): K_i = e(k_i pk, H(MessageV2(round_i)))^3, one
// single-pair pairing per item. key_table: key = a one-entry table of launch_decompress_g1 (a point of
// order r, not infinity) -> TK (kTsealT1Words words), the multiples j 16^w pk. point: the scalars and cls
// of launch_tseal_u -> P, an AoS table of G1_WORDS per item with P_i = k_i pk (untouched where cls != 0).
// miller_lines1 / miller_f1: the two Miller passes of the pairs (P_i, H_i) alone over a
// whole pass of cnt items; LN holds kMillerLine1Words per item, half of MILLER_LINE_WORDS; F as
// launch_miller leaves it (1 where h_inf, untouched where cls != 0).
constexpr size_t kMillerLine1Words = 68 * 6 * 12;
void launch_tseal_key_table(const uint32_t* key, uint32_t* TK, hipStream_t st);
void launch_tsealr_point(const uint32_t* TK, const uint8_t* scalars, const uint8_t* cls, size_t cnt, uint32_t* P,
                         hipStream_t st);
void launch_miller_lines1(const uint32_t* P, const uint32_t* H, const uint8_t* h_inf, const uint8_t* cls, size_t cnt,
                          uint32_t* LN, hipStream_t st);
void launch_miller_f1(const uint32_t* LN, const uint8_t* h_inf, const uint8_t* cls, size_t cnt, uint32_t* F,
                      hipStream_t st);

// ---- timelock encrypt / decrypt, the fused tail (k_tmask.hip, tmask.h): one lane per item,
// out[i] = in[i] XOR kdf_sha256_ctr(Gt value of item i, mlen) over cnt x mlen packed bytes (1 <= mlen <= 256, no
// alignment asked for: dwords move only when in, out and mlen are all multiples of 4), or mlen zero bytes
// where flag[i] != good (class bytes: good = 0; ok bytes: good = 1). Nothing outside [i mlen, (i + 1) mlen) is
// written; out == in is allowed. tmask: E = the captured values (SoA of stride cnt, what launch_tlock_encode
// reads). tmask_encoded: gt576 = cnt x 576 encoded bytes, 4-byte aligned (what the latency kernels write).
constexpr size_t kTmaskMsgMax = 256;
void launch_tmask(const uint32_t* E, const uint8_t* flag, uint8_t good, size_t cnt, const uint8_t* in, uint8_t* out,
                  size_t mlen, hipStream_t st);
void launch_tmask_encoded(const uint8_t* gt576, const uint8_t* flag, uint8_t good, size_t cnt, const uint8_t* in,
                          uint8_t* out, size_t mlen, hipStream_t st);

// ---- authenticated timelock (k_tauth.hip, tauth.h): one lane per item; cnt x mlen packed bytes of any
// alignment as above (dwords move only when the message pointers and mlen are all multiples of 4).
// derive: seeds (cnt x 32) and msgs -> scalars (cnt x 32 bytes big-endian, k = H3(seed, msg) mod r; zeros for a
// derived zero). seal_tail: E = the captured K (SoA of stride cnt), cls = launch_tseal_u's class bytes ->
// out_vs (cnt x 32) and out_ws, zeros where cls != 0; out_ws == msgs is allowed. open_tail: E = the captured
// values, U / u_inf = launch_decompress_g1's table of the pass, T1 = launch_tseal_g1_table's -> out = the
// messages of the items that pass the re-encryption check, zeros for every other; cls[i] becomes
// BLSV_REJ_TLOCK_AUTH where it was 0 and the check failed; out == ws is allowed.
constexpr size_t kTauthSeedLen = 32, kTauthVLen = 32;
void launch_tauth_derive(const uint8_t* seeds, const uint8_t* msgs, size_t cnt, size_t mlen, uint8_t* scalars,
                         hipStream_t st);
void launch_tauth_seal_tail(const uint32_t* E, const uint8_t* cls, size_t cnt, const uint8_t* seeds, const uint8_t* msgs,
                            size_t mlen, uint8_t* out_vs, uint8_t* out_ws, hipStream_t st);
void launch_tauth_open_tail(const uint32_t* E, const uint32_t* U, const uint8_t* u_inf, uint8_t* cls, size_t cnt,
                            const uint32_t* T1, const uint8_t* vs, const uint8_t* ws, size_t mlen, uint8_t* out,
                            hipStream_t st);
// ... and their ragged forms (blsv_tlock_*_auth*_var): item i's bytes lie at offs[i] .. offs[i + 1] of the packed
// message pointers, offs = cnt + 1 prefix offsets on the device, every length 1 .. 256 (the host has checked).
// words: every length is a multiple of 4; dwords then move when the message pointers are 4-byte aligned too.
void launch_tauth_derive_var(const uint8_t* seeds, const uint8_t* msgs, size_t cnt, const uint32_t* offs, bool words,
                             uint8_t* scalars, hipStream_t st);
void launch_tauth_seal_tail_var(const uint32_t* E, const uint8_t* cls, size_t cnt, const uint8_t* seeds, const uint8_t* msgs,
                                const uint32_t* offs, bool words, uint8_t* out_vs, uint8_t* out_ws, hipStream_t st);
void launch_tauth_open_tail_var(const uint32_t* E, const uint32_t* U, const uint8_t* u_inf, uint8_t* cls, size_t cnt,
                                const uint32_t* T1, const uint8_t* vs, const uint8_t* ws, const uint32_t* offs, bool words,
                                uint8_t* out, hipStream_t st);

// ---- latency path (k_lat.hip): one workgroup per item, the whole verification; writes cls[i] (REJ_*)
int lat_trace_read(uint64_t* out, int n, hipStream_t st);  // phase marks of item 0 (wteam.h WV_MARK)
int lat_trace_clear(hipStream_t st);
int lat_trace_enable(int on, hipStream_t st);  // the device-global flag WV_MARK tests (off by default)
extern int g_generic_chains_all;  // k_hash.hip: every lane through the generic cofactor / subgroup kernels (test hook)
// and, for the messages form with S != nullptr, the decoded sigma (H/S staging layout, stride cnt)
void launch_lat_chained(const ChainedSrc& src, size_t base, size_t cnt, const uint32_t* pk_tab, const uint8_t* pk_inf,
                        uint8_t* cls, hipStream_t st);
void launch_lat_unchained(const uint64_t* rounds, uint64_t first_round, const uint8_t* sigs, size_t base, size_t cnt,
                          const uint32_t* pk_tab, const uint8_t* pk_inf, uint8_t* cls, hipStream_t st);
void launch_lat_messages(const uint8_t* msgs, const uint64_t* off, const uint32_t* len, const uint8_t* sigs,
                         size_t stride, size_t offset, size_t cnt, const uint32_t* pk_tab, const uint8_t* pk_inf,
                         const uint32_t* pk_idx, uint8_t* cls, uint32_t* S, uint8_t* s_inf, hipStream_t st);
// timelock opening on the latency path (k_lat_tlock.hip): one workgroup per item, E_i = e(U_i, sigma_j)^3
// with j = sig_of[i] (0 when sig_of is null) -> out (n_items x 576 bytes, 4-byte aligned, zeros for a
// rejected item), cls[i] (the item's class: U's own, else BLSV_REJ_TLOCK_SIG under a rejected signature)
// and sig_cls[j]; n_idle further workgroups class the signatures idle[k], which have no item
void launch_lat_tlock(const uint8_t* sigs, const uint32_t* sig_of, const uint8_t* us, size_t n_items,
                      const uint32_t* idle, size_t n_idle, uint8_t* out, uint8_t* cls, uint8_t* sig_cls,
                      hipStream_t st);
// timelock sealing on the latency path (k_lat_tseal.hip): one workgroup per item, U_i = k_i G1 and
// K_i = e(k_i pk, H(MessageV2(round_i)))^3 with round_i = rounds[i] (the one round `round` when rounds is
// null) from the tables T1 and TK (kTsealT1Words words each: launch_tseal_g1_table, launch_tseal_key_table)
// -> us (n x 48 bytes), gts (n x 576 bytes), both 4-byte aligned, and ok (n bytes); zeros and ok = 0 for a
// scalar == 0 mod r
void launch_lat_tseal(const uint32_t* T1, const uint32_t* TK, const uint64_t* rounds, uint64_t round,
                      const uint8_t* scalars, size_t n, uint8_t* us, uint8_t* gts, uint8_t* ok, hipStream_t st);

// ---- group / threshold / signing kernels (k_misc.hip)
// decompress cnt G1 points (48 B each) -> pk table entries + inf flags + reject class
void launch_decompress_g1(const uint8_t* in, size_t cnt, uint32_t* tab, uint8_t* inf, uint8_t* cls, hipStream_t st);
// PubPoly.Eval(idx[i]) over t commits (affine table, none at infinity assumed via inf flags)
void launch_pubpoly_eval(const uint32_t* commits, const uint8_t* commit_inf, uint32_t t, const uint32_t* idx,
                         size_t cnt, uint32_t* out_tab, uint8_t* out_inf, hipStream_t st);
// authenticated timelock on the latency path (k_lat_tauth_open.hip, k_lat_tauth_seal.hip): one workgroup per
// item. Opening: launch_lat_tlock's item shape (sig_of, idle, sig_cls) with the item's V (32 bytes) and W (mlen
// bytes, 1 .. 256, packed) beside its U; out gets n_items x mlen message bytes (zeros unless cls[i] == 0) -- byte
// for byte what launch_tauth_open_tail gives behind the batch passes. T1: kTsealT1Words words (launch_tseal_g1_table).
// walk_waves: the waves that share the check's walk, 8 or 1 (the same bytes either way).
// offs (optional, the ragged forms): n_items + 1 prefix offsets on the device; item i's W and message bytes then
// lie at offs[i] .. offs[i + 1] of ws and out, and mlen is not read.
void launch_lat_tauth_open(const uint8_t* sigs, const uint32_t* sig_of, const uint8_t* us, const uint8_t* vs,
                           const uint8_t* ws, size_t mlen, size_t n_items, const uint32_t* idle, size_t n_idle,
                           const uint32_t* T1, uint8_t* out, uint8_t* cls, uint8_t* sig_cls, int walk_waves,
                           hipStream_t st, const uint32_t* offs = nullptr);
// Sealing: launch_lat_tseal's item shape with the item's seed (32 bytes) and message (mlen bytes, packed) in the
// scalar's place; us (4-byte aligned) n x 48, vs n x 32, ws n x mlen, ok n -- byte for byte what launch_tauth_derive,
// the sealing passes and launch_tauth_seal_tail give. Neither the derived scalar nor K is written anywhere.
// offs (optional, the ragged forms): n + 1 prefix offsets on the device, as above, for msgs and ws.
void launch_lat_tauth_seal(const uint32_t* T1, const uint32_t* TK, const uint64_t* rounds, uint64_t round,
                           const uint8_t* seeds, const uint8_t* msgs, size_t mlen, size_t n, uint8_t* us, uint8_t* vs,
                           uint8_t* ws, uint8_t* ok, hipStream_t st, const uint32_t* offs = nullptr);

// decode only on the latency engine (k_lat.hip; one two-wave workgroup per signature)
void launch_lat_decode(const uint8_t* sigs, size_t stride, size_t offset, size_t cnt, uint32_t* S, uint8_t* s_inf,
                       uint8_t* cls, hipStream_t st);
// decoding alone (signatures at sigs + (base+i)*stride + offset): the subgroup check is left to
// launch_miller(check_subgroup = true)
void launch_decompress_g2_only(const uint8_t* sigs, size_t stride, size_t offset, size_t base, size_t cnt,
                               uint32_t* S, uint8_t* s_inf, uint8_t* cls, hipStream_t st);
// sum_i [lambda_i] S_i over the selected affine staging entries sel[i] (S in SoA of stride n_s),
// compressed to 96 bytes
// [lambda_i] S_sel[i] summed and compressed (k_latrec.hip, lane form); scratch >= t * 192 words
// saff (optional, k_lat.hip kLatSaffWords words): the sum's affine point for launch_lat_verify_pre
void launch_lat_recover(const uint32_t* S, size_t n_s, const uint8_t* s_inf, const uint32_t* sel,
                        const uint32_t* lambdas, uint32_t t, uint32_t* scratch, uint8_t* out96, hipStream_t st,
                        uint32_t* saff = nullptr);
// the fused round's VerifyRecovered in two launches (wvteam.h team_hash_key / verify_team_pre): H of
// message 0 of (msgs, off, len) and the Miller loop of (pk_tab[0], H) into hout, then the pairing
// check of the affine signature saff (launch_lat_recover) against it -> cls[0]
constexpr size_t kLatHoutWords = 448, kLatSaffWords = 192;
void launch_lat_hash_key(const uint8_t* msgs, const uint64_t* off, const uint32_t* len, const uint32_t* pk_tab,
                         const uint8_t* pk_inf, uint32_t* hout, hipStream_t st);
void launch_lat_verify_pre(const uint32_t* hout, const uint32_t* saff, uint8_t* cls, hipStream_t st);
// signatures: out + i*out_stride (+2 index prefix when index >= 0) = compress(sk * H(msg_i))
void launch_sign(const uint32_t* sk_words, int32_t index, const uint32_t* H, const uint8_t* h_inf, size_t cnt,
                 uint8_t* out, size_t out_stride, hipStream_t st);
// signing on the latency path (k_lat_sign.hip): one workgroup per message, item i = compress(sk * H(msg_i)) for
// the message msgs[off[i] .. off[i] + len[i]) and the key sk_words (eight little-endian words, reduced mod r)
// -> out (n x 24 words: 96-byte signatures at stride 96, no index prefix), byte for byte launch_sign's
void launch_lat_sign(const uint32_t* sk_words, const uint8_t* msgs, const uint64_t* off, const uint32_t* len, size_t n,
                     uint32_t* out, hipStream_t st);
// synthetic chained history (client/test/result/mock/result.go:98-132 recipe, per segment):
// fills sigs (n x 96) for rounds first_round .. first_round+n-1 with the ChainedSrc seed rule
void launch_gen_chained(const uint32_t* sk_words, const ChainedSrc& src, size_t n, uint8_t* sigs_out, hipStream_t st);

// ---- test hooks (k_misc.hip): raw field / group / pairing building blocks
// raw operation hooks (testops.h): op = a TestOp; in / out = cnt items of nin / nout Fp (12 raw words
// each); park: TRI_PARK_WORDS(cnt) words for the 3-lane ops. Each returns false for an op it does not hold.
bool launch_test_op(int op, const uint32_t* in, size_t cnt, uint32_t* out, uint32_t* park, hipStream_t st);
bool launch_test_op_mf(int op, const uint32_t* in, size_t cnt, uint32_t* out, hipStream_t st);
void launch_test_fp_mul(const uint32_t* a, const uint32_t* b, size_t cnt, uint32_t* out, hipStream_t st);
void launch_test_pairing(const uint32_t* p_tab, const uint32_t* q_aff, size_t cnt, uint32_t* out_f, hipStream_t st);
void launch_test_unpack_g2(const uint32_t* H, size_t cnt, uint32_t* out, hipStream_t st);
// raw AoS Fp12 (144 words each, tower order) <-> Montgomery SoA staging
void launch_test_pack_fp12(const uint32_t* f, size_t cnt, uint32_t* F, hipStream_t st);
void launch_test_unpack_fp12(const uint32_t* F, size_t cnt, uint32_t* out, hipStream_t st);
// SoA F -> final_exponentiation(F) with the one-lane register form (pairing.h), SoA out
void launch_test_final_exp_ref(const uint32_t* F, size_t cnt, uint32_t* out, hipStream_t st);

}  // namespace blsk
