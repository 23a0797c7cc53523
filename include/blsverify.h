/*
 * blsverify.h -- C ABI of the MI355X-native BLS12-381 beacon-verification engine.
 *
 * This is the drop-in boundary for drand's verification hot path. The reference
 * calls five methods on the package-level `key.Scheme` (tbls.NewThresholdSchemeOnG2(Pairing),
 * key/curve.go:31) plus the chain entry points built on it; each entry point below names the
 * reference interface it replaces. A cgo package (gpu/blsverify) binds these
 * symbols one-to-one.
 *
 * Conventions
 *  - All buffers are caller-owned host memory valid only for the duration of the call (cgo rules);
 *    the library copies into HBM and never retains caller pointers. The *_dev entry points take
 *    device pointers (HBM-resident batches, used by bench.py and multi-GPU sharding).
 *  - Return value: 0 = the call succeeded (per-item verdicts are in the outputs); < 0 =
 *    infrastructure error (bad arguments, HIP failure); details from blsv_last_error().
 *  - Accept/reject and recovered signature bytes are bit-exact with the reference kyber path;
 *    the optional reject_class output explains a reject (BLSV_REJ_*), error text is not graded.
 *  - Bitmaps: bit i (byte i/8, bit i%8, LSB first) = 1 iff item i verified.
 *  - first_bad: the ROUND number (chained/unchained) or the INDEX (message batches) of the first
 *    rejected item, UINT64_MAX when every item verified.
 *  - A context owns one HIP stream and is not thread-safe: one thread calls it at a time. For
 *    concurrent single-item callers use a blsv_service (thread-safe, coalesces concurrent calls into
 *    one launch; see the end of this header); for concurrent batch callers one context per thread,
 *    each with its chunk sized so that all of them fit in HBM (memory contract below).
 *
 * Latency contract (single-item and small callers: client.Get's per-round verify,
 * client/verify.go:185-207; the gossip validator, lp2p/client/validator.go:64; per-packet
 * VerifyPartial, chain/beacon/node.go:112,125; identity checks, key/keys.go:60-63)
 *  - A call with at most lat_max items (blsv_set_lat_max, default 1536) runs on the LATENCY path: one
 *    workgroup of eight waves per item, every limb of a field element in its own lane
 *    (drand_amd/csrc/k_lat.hip). Measured on MI355X (profiles/r06e_latency.json, warm): one
 *    VerifyRecovered 1.9 ms; blsv_aggregate of an n = 64 / t = 33 round (64 VerifyPartial +
 *    Recover + VerifyRecovered) 2.2 ms, blsv_aggregate_round V1 + V2 4.4 ms (the recovery and the
 *    verification of the shares the round would select if all verify run beside the partial
 *    verification -- H(msg) and the key pair's Miller loop from the start -- and are kept when the
 *    verdicts confirm that selection). Up to 256 items the time stays ~2.1 ms (every item has its
 *    own CU), then grows ~1.9 ms per further 256 items (profiles/r05za_latency_sweep.json).
 *  - Larger calls run on the BATCH pipeline (one lane per item, staged kernels): ~14 ms floor
 *    (14.1 ms at 64 items, 15.3 ms at 2,048: profiles/r05za_latency_sweep.json), then ~0.43 us per
 *    item (about 2.3 M items/s). Both paths give
 *    identical verdicts, reject classes and
 *    recovered bytes (tests/test_gpu_lat.py runs the same vectors through both).
 *  - The first call on a context also pays allocation and module load (~10-250 ms).
 */
#ifndef DRAND_AMD_BLSVERIFY_H
#define DRAND_AMD_BLSVERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct blsv_ctx blsv_ctx;

/* return codes */
#define BLSV_OK 0
#define BLSV_EINVAL (-1)
#define BLSV_EHIP (-2)
#define BLSV_ENOGROUP (-3)
#define BLSV_ENOTENOUGH (-4) /* Recover: fewer than t valid shares */

/* reject classes (per item) -- the order of kilic G2.FromCompressed's checks, then the pairing */
#define BLSV_REJ_OK 0
#define BLSV_REJ_LENGTH 1          /* wrong byte length (host-side)                      */
#define BLSV_REJ_FLAG 2            /* compression bit 0x80 clear                          */
#define BLSV_REJ_INF_NONZERO 3     /* infinity bit set but not exactly 0xc0 || 0...       */
#define BLSV_REJ_X_GE_P 4          /* a coordinate limb >= p                              */
#define BLSV_REJ_NOT_ON_CURVE 5    /* x^3 + b has no square root                          */
#define BLSV_REJ_NOT_IN_SUBGROUP 6 /* point not in the order-r subgroup                   */
#define BLSV_REJ_PAIRING 7         /* "bls: invalid signature" (pairing check failed)     */
#define BLSV_REJ_SHARE_INDEX 8     /* tbls share shorter than its 2-byte index prefix     */

#define BLSV_SIG_LEN 96
#define BLSV_PARTIAL_LEN 98
#define BLSV_PK_LEN 48

/* Library version string. */
const char* blsv_version(void);

/* Number of GPUs this process sees (0 when none or on a HIP error): one context per GPU for
 * blsv_verify_chained_multi. */
int blsv_device_count(void);

/* Create a context on HIP device `device`. */
int blsv_create(int device, blsv_ctx** out);
void blsv_destroy(blsv_ctx* ctx);
/* Last error message of this context ("" if none). */
const char* blsv_last_error(const blsv_ctx* ctx);

/*
 * Group state: the distributed public polynomial commitments (key.Share.PubPoly /
 * DistPublic.PubPoly, key/keys.go:235-241,316-324), t commitments of 48 bytes; the group public
 * key is commits[0] (DistPublic.Key(), chain.Info.PublicKey, chain/info.go:16-21). n is the group
 * size passed to Recover. A single-key chain is t = 1. Decoding follows kilic G1.FromCompressed
 * (chain/convert.go:15-18); returns BLSV_EINVAL if any commitment fails to decode.
 */
int blsv_set_group(blsv_ctx* ctx, const uint8_t* commits48, size_t t, size_t n);

/*
 * chain.VerifyBeacon (chain/beacon.go:87-92) over a contiguous chained range: beacon i has round
 * first_round + i, signature sigs96[i], and PreviousSig = prev0 (i == 0; 32 bytes = genesis seed
 * GroupHash at round 1, client/verify.go:122-124, or 96 bytes) or sigs96[i-1]. Replaces the serial
 * walk of client/verify.go:146-163 and chain/beacon/sync.go:100-119 with one batched call.
 * reject_class (optional, n bytes) receives BLSV_REJ_* per beacon.
 */
int blsv_verify_chained(blsv_ctx* ctx, uint64_t first_round, const uint8_t* prev0, size_t prev0_len,
                        const uint8_t* sigs96, size_t n, uint8_t* ok_bitmap, uint64_t* first_bad,
                        uint8_t* reject_class);

/*
 * blsv_verify_chained over SEVERAL contexts at once -- the multi-GPU shape of a Go host: one context
 * per GPU (ctxs[k] may sit on any device; each must hold the same group, set with blsv_set_group, and
 * appear once), one host thread per context. The range is split into n_ctx contiguous shards
 * (shard_counts[k] beacons each, summing to n; NULL = an even split, the first n % n_ctx shards one
 * longer); shard k's PreviousSig halo is the signature just before it (prev0 for the first shard), so
 * a corrupted signature at a shard edge still fails its successor in the next shard. The shards run
 * concurrently and their verdicts are merged in host memory: ok_bitmap / reject_class at their
 * positions in the whole range, first_bad = the lowest rejected ROUND over the shards (UINT64_MAX =
 * none). Identical outputs to one blsv_verify_chained call over the whole range. Replaces the serial
 * loops of client/verify.go:146-163 and chain/beacon/sync.go:100-119 on a multi-GPU node without a
 * collective (the shards share the caller's address space). Contexts are used by one thread each for
 * the duration of the call. Returns the first failing shard's code (its message in
 * blsv_last_error(ctxs[k])); BLSV_EINVAL for a bad split, a repeated context or differing groups.
 */
int blsv_verify_chained_multi(blsv_ctx* const* ctxs, size_t n_ctx, const size_t* shard_counts, uint64_t first_round,
                              const uint8_t* prev0, size_t prev0_len, const uint8_t* sigs96, size_t n,
                              uint8_t* ok_bitmap, uint64_t* first_bad, uint8_t* reject_class);

/*
 * chain.VerifyBeacon (chain/beacon.go:87-92) over n consecutive rounds first_round.. where each
 * round carries its OWN PreviousSig: prevs96[i*96 ..] (row 0 uses its first prev0_len = 32 or 96
 * bytes, every other row 96). For stored or relayed ranges whose linkage is not assumed, e.g. a
 * drand.db read by include/boltload.h (chain/boltdb/store.go:109-128 per-round Get). Outputs as in
 * blsv_verify_chained; first_bad is a ROUND.
 */
int blsv_verify_prevs(blsv_ctx* ctx, uint64_t first_round, const uint8_t* prevs96, size_t prev0_len,
                      const uint8_t* sigs96, size_t n, uint8_t* ok_bitmap, uint64_t* first_bad,
                      uint8_t* reject_class);

/*
 * One aggregator round of chain/beacon/chain.go:119-166 in two verification passes instead of three:
 * every partial verified (tbls.VerifyPartial, node.go:112; ok / reject_class per partial), Recover
 * over the first t valid shares in input order (chain.go:136; the shares it would re-verify got the
 * same deterministic verdicts in this pass), then VerifyRecovered of the group signature under the
 * group key (chain.go:141) into *group_ok. Returns BLSV_ENOTENOUGH (ok[] filled) with < t valid.
 */
int blsv_aggregate(blsv_ctx* ctx, const uint8_t* msg, size_t msg_len, const uint8_t* partials, size_t partial_len,
                   size_t k, size_t t, size_t n, uint8_t* ok, uint8_t* reject_class, uint8_t* out_sig96,
                   uint8_t* group_ok);

/* blsv_aggregate_round outcomes, in the order chain/beacon/chain.go:131-166 tests them */
#define BLSV_AGG_OK 0              /* beacon made, V1 only (fewer than t V2 partials)                   */
#define BLSV_AGG_OK_V2 1           /* beacon made with SignatureV2 (*v2_valid = VerifyRecovered V2)     */
#define BLSV_AGG_V1_RECOVER_FAIL 2 /* Recover V1 failed (< t valid distinct shares): "invalid_recovery" */
#define BLSV_AGG_V1_INVALID 3      /* VerifyRecovered V1 failed: "invalid_sig", no beacon                */
#define BLSV_AGG_V2_RECOVER_FAIL 4 /* >= t V2 partials but Recover V2 failed: no beacon (chain.go:157)  */

/*
 * The whole aggregation step of chainStore.runAggregator (chain/beacon/chain.go:131-166) for one
 * round cache, V1 and V2 together, in two verification passes: pass 1 checks the k1 V1 partials
 * (roundCache.Partials(), msg1 = chain.Message(round, prev)) and the k2 V2 partials
 * (roundCache.PartialsV2(), msg2 = chain.MessageV2(round)) in one batch (ok1/ok2); Recover V1 and,
 * when k2 >= t, Recover V2 (kyber share selection, see blsv_recover) run on the staged shares; pass 2
 * runs VerifyRecovered(pub.Commit(), ...) on both group signatures. *status = BLSV_AGG_*; sig1_96 /
 * sig2_96 hold the group signatures when produced. A V2 VerifyRecovered failure does not block the
 * beacon (*v2_valid = 0, chain.go:162-164); a V2 Recover failure does (chain.go:155-160). The
 * threshold gate (roundCache.Len() >= thr) and the cache itself stay with the caller
 * (drand_amd/callers.py Aggregator restates them).
 */
int blsv_aggregate_round(blsv_ctx* ctx, const uint8_t* msg1, size_t msg1_len, const uint8_t* partials1, size_t k1,
                         const uint8_t* msg2, size_t msg2_len, const uint8_t* partials2, size_t k2,
                         size_t partial_len, size_t t, size_t n, uint8_t* ok1, uint8_t* ok2, uint8_t* sig1_96,
                         uint8_t* sig2_96, int32_t* status, uint8_t* v2_valid);

/*
 * tbls.VerifyPartial (chain/beacon/node.go:112,125) over partials of MANY rounds in one pass:
 * partial i signs msgs[off_i .. off_i + msg_lens[i]) (messages packed back to back), e.g. a catch-up
 * of cached partials across rounds (chain/beacon/cache.go:112-182). Same outputs as
 * blsv_verify_partials. At most the context's chunk capacity of partials per call.
 */
int blsv_verify_partials_multi(blsv_ctx* ctx, const uint8_t* msgs, const uint32_t* msg_lens, const uint8_t* partials,
                               size_t partial_len, size_t k, uint8_t* ok, uint8_t* reject_class);

/*
 * chain.VerifyBeaconV2 (chain/beacon.go:94-98): msg = sha256(BE64(round)) over SignatureV2.
 * rounds may be NULL (then round i = first_round + i).
 */
int blsv_verify_unchained(blsv_ctx* ctx, const uint64_t* rounds, uint64_t first_round, const uint8_t* sigs96,
                          size_t n, uint8_t* ok_bitmap, uint64_t* first_bad, uint8_t* reject_class);

/*
 * key.Scheme.VerifyRecovered(pub, msg, sig) (chain/beacon.go:91, chain/beacon/chain.go:141,162) and
 * key.AuthScheme.Verify (key/keys.go:60-63) in batch form: message i is msgs[off_i .. off_i+len_i)
 * with msg_lens[i] bytes (consecutive), verified against pk48 (NULL = group key) and sigs96[i].
 * first_bad receives the index of the first reject.
 */
int blsv_verify_messages(blsv_ctx* ctx, const uint8_t* pk48, const uint8_t* msgs, const uint32_t* msg_lens,
                         size_t n, const uint8_t* sigs96, uint8_t* ok_bitmap, uint64_t* first_bad,
                         uint8_t* reject_class);

/*
 * key.Scheme.VerifyPartial(pubPoly, msg, partial) (chain/beacon/node.go:112,125) for k partials of
 * partial_len bytes each (98 = 2-byte BE share index || 96-byte signature); all share H(msg).
 * ok[i] = 1/0; reject_class optional.
 */
int blsv_verify_partials(blsv_ctx* ctx, const uint8_t* msg, size_t msg_len, const uint8_t* partials,
                         size_t partial_len, size_t k, uint8_t* ok, uint8_t* reject_class);

/*
 * key.Scheme.Recover(pubPoly, msg, sigs, t, n) (chain/beacon/chain.go:136,155): verifies the
 * partials and takes the first t VALID ones in input order, duplicates included (kyber tbls.Recover
 * stops at len(pubShares) >= t); those are then keyed by index as share.RecoverCommit/xyCommit does
 * (a duplicate collapses, an index >= n is dropped) and fewer than t distinct shares returns
 * BLSV_ENOTENOUGH. Otherwise Lagrange-interpolates sum lambda_i sigma_i at 0 over x = index + 1 and
 * writes the compressed 96-byte group signature. The skip-invalid / duplicate rules follow the
 * published kyber source ([ext], unpinned by any reference test).
 */
int blsv_recover(blsv_ctx* ctx, const uint8_t* msg, size_t msg_len, const uint8_t* partials, size_t partial_len,
                 size_t k, size_t t, size_t n, uint8_t* out_sig96);

/*
 * key.Scheme.Sign(priShare, msg) (chain/beacon/crypto.go:58) / AuthScheme.Sign in batch form:
 * out[i] = (index >= 0 ? BE16(index) : "") || compress(sk * H(msg_i)); sk32 is the big-endian
 * scalar (kyber Scalar.MarshalBinary), reduced mod r. Output stride 98 with index, 96 without.
 */
int blsv_sign(blsv_ctx* ctx, const uint8_t* sk32, int32_t index, const uint8_t* msgs, const uint32_t* msg_lens,
              size_t n, uint8_t* out);

/*
 * Signing on the latency path (opt-in). The calls a node makes are one or two messages: its V1 and V2
 * partials once per round (chain/beacon/crypto.go:58), or one identity (key/keys.go:80-83). On the batch path
 * such a call gives ONE lane the whole job -- hash-to-G2, a 255-bit double-and-add, the inversion, the
 * compression -- with the chip idle. The latency engine has a signing item: one workgroup of eight waves per
 * message hashes it (waves 0, 3, 4, 5, as a verification's hash branch), converts H to affine once, then four
 * waves each run one 64-bit ladder [d_j] P_j of the key's digits in base |x| on P_j = (-psi)^j (H) = [|x|^j] H
 * (63 doublings and a mixed addition per set bit, instead of 254 doublings), and wave 0 adds the four, converts
 * and compresses (drand_amd/csrc/wsign.h, k_lat_sign.hip).
 *
 * blsv_set_sign_lat_max(ctx, L) returns the previous value. The default is 0 = off, or the environment
 * variable BLSV_SIGN_LAT_MAX (a non-negative integer; anything else is ignored with a note on stderr). L is
 * clamped to the context's chunk, here and whenever the chunk shrinks (blsv_set_chunk, the out-of-memory
 * halving). A setter of its own: the other *_lat_max values do not move with it. With L = 0 blsv_sign behaves
 * exactly as described above.
 *
 * With L > 0, blsv_sign sends a call of 1 .. L messages to the latency path, after its own argument
 * validation (the same BLSV_EINVAL with no output touched). A call with n = 0 or n > L takes the batch path
 * unchanged. Every output byte is what the batch path writes for the same arguments: BE16(index) in front of
 * each signature at stride 98 when index >= 0 (the kernel writes 96-byte signatures; the host puts the two
 * bytes in front as it copies out), stride 96 without, and the encoding of the point at infinity (0xc0, then
 * 95 zero bytes) for a key == 0 (mod r).
 *
 * Counters: blsv_sign_lat_stats: *launches = latency-path calls, *items = messages they signed since the
 * context's creation; either pointer may be NULL. No other counter moves on a latency-path call.
 *
 * Memory and secrecy: one device buffer of 108 bytes per message (8 offset + 4 length up, 96 down) plus the
 * message's own bytes, 32 bytes of key and at most 63 of padding, beside the pipeline staging, which this
 * path does not touch. The staged key -- device and host copies -- is cleared behind the kernel before the
 * entry returns, also when the call fails. A partial product [d_j] P_j beside the public P_j is a 64-bit
 * discrete logarithm, which is breakable where the whole signature is not: each wave overwrites the on-chip
 * slots that held one before the workgroup exits, and none is ever written to device memory. There is NO
 * constant-time claim: the ladders branch on the digits' bits, as the batch path's double-and-add branches
 * on the key's.
 *
 * Measured on one MI355X (profiles/sign_lat_bench.json; the two modes alternating call by
 * call in one run and each mode also timed twice in a row, medians, identical bytes in every round): a lone
 * blsv_sign of a 32-byte message takes 1.75 ms against 17.5 ms on the batch path (10.0 times faster; two
 * calls in a row of one mode differ by 0.01 ms on the latency path and 1.2 ms on the batch path), a node's
 * round -- two messages with a share index in one call -- 1.75 ms against 17.6 ms; the lone verify of the same
 * run takes 1.90 ms. n messages: 1.75 ms up to 2, 1.76 at 16, 1.78 at 64, 1.84 at 256 (one workgroup per compute
 * unit), 3.59 at 512, 7.07 at 1,024, 14.05 at 2,048 and 27.97 at 4,096, against 16.4 - 18.2 ms on the batch path
 * at every size. The batch path is first faster at n = 4,096 (at 2,048 the latency path still wins by 1.17).
 * Recommended: blsv_set_sign_lat_max(ctx, 2048).
 */
size_t blsv_set_sign_lat_max(blsv_ctx* ctx, size_t items); /* returns the previous value */
int blsv_sign_lat_stats(blsv_ctx* ctx, uint64_t* launches, uint64_t* items);

/* ---------------------------------------------------------------- device-resident batches */

/*
 * Chained verify over HBM-resident signatures, optionally split into independently seeded
 * segments of seg_len rounds (seg_len = 0 means one segment): with s = (i + seg_phase) / seg_len,
 * beacon i (round first_round + i) uses d_seeds96[s] as PreviousSig when i == 0 or
 * (i + seg_phase) % seg_len == 0 (length seed0_len for s = 0, else 96), else d_sigs96[i-1].
 * seg_phase (< seg_len; 0 when segments start at item 0) lets a shard that begins inside a
 * segment pass its one-signature halo as d_seeds96[0] (multi-GPU range sharding).
 * Outputs (device): d_bitmap (ceil(n/64) uint64 words, fully written), d_first_bad (one uint64:
 * the ROUND of the first reject or UINT64_MAX), d_reject_class (optional, n bytes). Asynchronous
 * on `stream` (a hipStream_t; NULL = the context stream). The context's staging buffers are shared
 * by every call: successive *_dev calls on one context must be issued on ONE stream (or the caller
 * orders them with events), never concurrently on two streams. Internally the decompression stage
 * runs on the context's side stream, forked from `stream` after the work already queued there and
 * joined back into it (events) before the pairing stage: ordering with respect to `stream` holds.
 */
int blsv_verify_chained_dev(blsv_ctx* ctx, uint64_t first_round, uint64_t seg_len, uint64_t seg_phase,
                            const uint8_t* d_seeds96, size_t seed0_len, const uint8_t* d_sigs96, size_t n,
                            uint64_t* d_bitmap, uint64_t* d_first_bad, uint8_t* d_reject_class, void* stream);

/*
 * Synthetic chained history (client/test/result/mock/result.go:98-132, per segment, on device):
 * d_sigs96[i] = compress(sk * H(Message(first_round + i, prev))) with the seed rule above
 * (seg_phase = 0). Same single-stream rule as blsv_verify_chained_dev.
 */
int blsv_generate_chained_dev(blsv_ctx* ctx, const uint8_t* sk32, uint64_t first_round, uint64_t seg_len,
                              const uint8_t* d_seeds96, size_t seed0_len, uint8_t* d_sigs96, size_t n, void* stream);

/* Wait for the context stream. */
int blsv_synchronize(blsv_ctx* ctx);

/*
 * Latency-path cutover (see the latency contract above): calls with 1..lat_max items take the latency
 * path, larger ones the batch pipeline; 0 = batch pipeline only. The default is the BLSV_LAT_MAX
 * environment variable (a non-negative decimal integer; anything else is ignored with a warning on
 * stderr), else 1536 (below where the two paths cross on MI355X, ~1,750 items). Values above 2^20 (one pipeline chunk)
 * are clamped to 2^20. Returns the previous value.
 */
size_t blsv_set_lat_max(blsv_ctx* ctx, size_t lat_max);

/*
 * Memory contract. A context allocates its pipeline staging lazily, for min(largest batch, chunk)
 * items at ~42.4 KB per item (39 KB of it the Miller line staging): a lone verify or a round of
 * partials takes a few MB, a full 2^20 chunk ~43 GB of the GPU's 288 GB. The chunk defaults to 2^20
 * (the BLSV_CHUNK environment variable overrides it); a larger batch runs in chunk-sized passes with
 * identical verdicts. When an allocation fails with out-of-memory the context frees its staging,
 * halves its chunk (not below 16,384 items) and retries, so contexts or ranks sharing one GPU degrade
 * to smaller passes instead of failing. blsv_set_chunk caps it explicitly (items, rounded up to a
 * multiple of 64 and clamped to [16384, 2^20]; 0 = the default) and releases the staging at once when
 * it shrinks; it also clamps lat_max. Returns the previous chunk.
 */
size_t blsv_set_chunk(blsv_ctx* ctx, size_t items);
/* HBM bytes of pipeline staging the context holds now (0 before its first batch). */
size_t blsv_workspace_bytes(const blsv_ctx* ctx);

/* ---------------------------------------------------------------- randomized batch verification
 *
 * Opt-in. The entry points above make the check chain.VerifyBeacon makes, once per beacon, and stay
 * the default and the source of every headline number. The *_rlc entry points below take the argument
 * lists and fill the outputs of their exact counterparts, but share one pairing check among each group
 * of G consecutive beacons of a call (all under the group key set with blsv_set_group):
 *
 *   prod_i [ e(pk, H_i) e(-g1, sigma_i) ]^{r_i} = e(pk, sum r_i H_i) e(-g1, sum r_i sigma_i)
 *
 * with 64-bit weights r_i = the first 8 bytes, big-endian, of SHA-256(seed || BE64(i)), i the item's
 * index within the call. The 32-byte seed is drawn from the OS CSPRNG (getrandom) once per call, after
 * the inputs are fixed, is never reused and never returned; if the draw fails the call returns
 * BLSV_EHIP. Decoding and the subgroup check stay exact and per item, and only items that decode
 * (class 0 after that stage) enter a group's sums. The items of every group whose check fails are then
 * run through the exact pairing stages.
 *
 * Soundness contract
 *  - A reject is always the exact pipeline's reject: bitmap, first_bad and reject classes of a call
 *    equal the exact entry point's whenever every invalid item is caught, and a valid item is never
 *    rejected.
 *  - An invalid item is accepted only if its group's check passes, which happens with probability at
 *    most 2^-64 over the seed. The bound rests on every sigma_i lying in the order-r subgroup, which
 *    the decompression stage has already checked.
 *  - Cost: an all-valid call pays the combination stage plus n / G pairing checks. An adversary who
 *    puts one bad round into every group forces the exact cost plus the combination stage.
 *
 * Routing: a call takes this path when n > lat_max and n >= 2 G; any other call is served by the exact
 * entry point (and blsv_rlc_stats does not move). Not offered for blsv_verify_chained_multi,
 * blsv_verify_prevs, message batches, the service or the latency path.
 */
int blsv_verify_chained_rlc(blsv_ctx* ctx, uint64_t first_round, const uint8_t* prev0, size_t prev0_len,
                            const uint8_t* sigs96, size_t n, uint8_t* ok_bitmap, uint64_t* first_bad,
                            uint8_t* reject_class);
int blsv_verify_unchained_rlc(blsv_ctx* ctx, const uint64_t* rounds, uint64_t first_round, const uint8_t* sigs96,
                              size_t n, uint8_t* ok_bitmap, uint64_t* first_bad, uint8_t* reject_class);
/*
 * As blsv_verify_chained_dev, with one difference: the call SYNCHRONISES `stream` once per pass (the
 * group verdicts are read back to choose the items of the exact fallback), so it is not asynchronous;
 * the outputs of the last pass are still only ordered on `stream`.
 */
int blsv_verify_chained_rlc_dev(blsv_ctx* ctx, uint64_t first_round, uint64_t seg_len, uint64_t seg_phase,
                                const uint8_t* d_seeds96, size_t seed0_len, const uint8_t* d_sigs96, size_t n,
                                uint64_t* d_bitmap, uint64_t* d_first_bad, uint8_t* d_reject_class, void* stream);
/*
 * Group size G of the randomized path: g rounded down to a power of two and clamped to [8, 4096].
 * Default 64, chosen by measurement (profiles/rlc_bench.json). Returns the previous value.
 */
size_t blsv_set_rlc_group(blsv_ctx* ctx, size_t g);
/*
 * Counters of the randomized path since the context's creation: group checks made, group checks that
 * failed, items re-run through the exact pairing stages (every item of a failing group). Any pointer
 * may be NULL.
 */
int blsv_rlc_stats(blsv_ctx* ctx, uint64_t* groups, uint64_t* groups_failed, uint64_t* items_exact);

/* ---------------------------------------------------------------- timelock
 *
 * What SignatureV2 exists for (core/timelock_test.go:43-60): a message is encrypted to a future round
 * under the group key, and that round's SignatureV2 is the IBE private key that opens it --
 * timelock.Decrypt(key.Pairing, private, ciphertext) pairs the ciphertext's ephemeral point U = rP
 * with the signature. When a round arrives everything locked to it opens at once: n pairings
 * e(U_i, sigma) with ONE shared G2 argument. blsv_tlock_open computes them in one call.
 *
 * Inputs
 *  - sig96: the round's compressed G2 signature, decoded as every signature is (kilic
 *    G2.FromCompressed with the subgroup check). A sigma that does not decode makes the call return
 *    BLSV_EINVAL with its BLSV_REJ_* class (2-6) in *sig_class; the per-item outputs are left untouched
 *    (the precedent of a key that does not decode). *sig_class = 0 otherwise. The call does NOT check
 *    that sigma is the round's signature: verify it first (blsv_verify_unchained), a wrong "private
 *    key" opens to garbage without any error.
 *  - us48: n compressed G1 points (BLSV_U_LEN bytes each), decoded per item by the rules of a public
 *    key (kilic G1.FromCompressed, subgroup check included). An item whose U does not decode gets
 *    ok[i] = 0, reject_class[i] = BLSV_REJ_* 2-6 and BLSV_GT_LEN zero bytes; its neighbours are unaffected.
 *
 * Output: out_gt576[i] = E_i = e(U_i, sigma)^3 with e the reduced pairing f^((p^12 - 1)/r), i.e. the
 * Miller value raised to (p^6 - 1)(p^2 + 1) * lambda with lambda = 3 (p^4 - p^2 + 1)/r =
 * (x-1)^2 (x+p) (x^2+p^2-1) + 3 -- the hard part every verification here runs, and the exponent of
 * kilic's finalExp as recalled. A pair with U or sigma at infinity is skipped as kilic's engine skips
 * it: E_i = 1, ok[i] = 1. ok[i] = 1 means "U decoded", nothing more.
 *
 * Encoding of E_i: twelve canonical Fp values (out of Montgomery form, fully reduced), 48 bytes
 * big-endian each, highest tower coefficient first: c1.c2.c1, c1.c2.c0, c1.c1.c1, c1.c1.c0, c1.c0.c1,
 * c1.c0.c0, c0.c2.c1, c0.c2.c0, c0.c1.c1, c0.c1.c0, c0.c0.c1, c0.c0.c0 (Fp12 = Fp6[w]/(w^2 - v),
 * Fp6 = Fp2[v]/(v^3 - (1 + i)), x.cK.cJ.cI = coefficient of w^K v^J i^I). The encoding of 1 is 575 zero
 * bytes and a final 0x01.
 *
 * PARITY UNPINNED, two items: the exponent lambda (the cube) and the coefficient order above are kilic
 * GT marshalling as recalled; the reference holds no Gt fixture (its timelock test only round-trips
 * random data), so neither is pinned against it. Both are pinned against this repository's own oracle.
 * The KDF that turns E_i into a key stream is the caller's (kyber's is BLAKE2Xs over GT.MarshalBinary); or see
 * "Timelock in one call" below, which runs this project's own KDF and the XOR on the device.
 *
 * Prepared-signature cache: the context keeps the prepared form of the LAST sigma (its 96 bytes and
 * the table of its 68 Miller lines' P-independent coefficients, 19,584 bytes on the device). A call with
 * the same 96 bytes prepares nothing; any other sigma replaces the entry (one entry: A, B, A prepares
 * three times). blsv_tlock_stats: *prepared = preparations made (a sigma that does not decode is not
 * counted), *items = U values processed (rejected ones included) since the context's creation; either
 * pointer may be NULL.
 *
 * Sizing: the pipeline staging is used as it is (memory contract above, unchanged); more than a chunk
 * of items runs in chunk-sized passes with identical outputs. One lane per item serves every n unless
 * the latency-path form below is switched on (blsv_set_tlock_lat_max; off by default); there is no
 * service entry.
 *
 * blsv_tlock_open_dev: d_us48 / d_out_gt576 (4-byte aligned) / d_reject_class (optional; 0 = opened)
 * are device pointers, sig96 is host memory. Sigma's decode class is read back (one 1-byte copy and
 * one synchronisation of `stream`) only when the signature is not the cached one; everything else is
 * asynchronous on `stream` under the single-stream rule of blsv_verify_chained_dev. Returns
 * BLSV_EINVAL for a sigma that does not decode (class in blsv_last_error's text).
 */
#define BLSV_U_LEN 48
#define BLSV_GT_LEN 576
int blsv_tlock_open(blsv_ctx* ctx, const uint8_t* sig96, const uint8_t* us48, size_t n, uint8_t* out_gt576,
                    uint8_t* ok, uint8_t* reject_class, uint8_t* sig_class);
int blsv_tlock_open_dev(blsv_ctx* ctx, const uint8_t* sig96, const uint8_t* d_us48, size_t n, uint8_t* d_out_gt576,
                        uint8_t* d_reject_class, void* stream);
int blsv_tlock_stats(blsv_ctx* ctx, uint64_t* prepared, uint64_t* items);

/*
 * Opening across many rounds: the mirror image of blsv_tlock_seal_rounds below. A vault that comes back
 * after downtime, an auditor who opens a day of a 3-second chain (28,800 rounds), an auction whose bids
 * were locked to a spread of rounds: each holds ciphertexts for many rounds at once, usually a few per
 * round. blsv_tlock_open_rounds opens them in ONE call instead of one blsv_tlock_open per round.
 *
 * Inputs
 *  - sigs96: m round signatures (96 bytes each), counts: m item counts. Round j owns counts[j] ciphertexts;
 *    the U values of round 0, round 1, ... are packed back to back in us48 (the convention of msgs /
 *    msg_lens in blsv_verify_messages). sum counts must equal n and m must be below 2^32: anything else,
 *    or a byte count that would overflow, is BLSV_EINVAL and no output is touched. A count of 0 is allowed;
 *    that signature is still decoded and classed.
 *  - Per item: for item i of round j whose sigma_j decodes, the BLSV_GT_LEN output bytes, ok[i] and
 *    reject_class[i] are byte for byte what blsv_tlock_open(ctx, sigs96 + 96 j, us48 + 48 i, 1, ...)
 *    returns, E = 1 with ok = 1 for U_i or sigma_j at infinity included.
 *  - Per signature: a sigma_j that does not decode gets its BLSV_REJ_* class (2-6) in sig_class[j]
 *    (optional, m bytes; 0 = decoded) and the call still returns BLSV_OK. Every item of round j then has
 *    ok = 0 and BLSV_GT_LEN zero bytes; its class is U_i's own decode class where that is not 0 (what the
 *    item would get under any signature), else BLSV_REJ_TLOCK_SIG. The other rounds are unaffected.
 *  - As blsv_tlock_open, the call does NOT check that sigma_j is round j's signature (it never learns the
 *    round numbers): verify the m signatures first, in one blsv_verify_unchained.
 *
 * State: no cache. The prepared tables (19,584 bytes per signature) live in the pipeline staging for the
 * duration of a pass. The one-entry sigma cache of blsv_tlock_open, the sealing caches and all their
 * counters are left alone. blsv_tlock_open_rounds_stats: *prepared = signatures prepared (each sigma that
 * decodes and has count > 0, once per pass that touches it), *items = U values processed; either pointer
 * may be NULL. *prepared is kept on the device and read back here (one synchronisation of the context's
 * stream).
 *
 * Sizing: the pipeline staging is used as it is; more than a chunk of items runs in chunk-sized passes
 * with identical outputs (a round whose run straddles a pass boundary is prepared in both passes).
 *
 * How a pass runs: one one-wave workgroup per tile of up to 64 consecutive items. A run of at least
 * dense_min items gets uniform tiles (all lanes share sigma_j: its table is read from LDS by broadcast, as
 * blsv_tlock_open reads it); the stretches of shorter runs between them are cut into mixed tiles whose
 * lanes each read their own signature's table from global memory. Both forms give the same bytes.
 * blsv_set_tlock_dense_min sets dense_min and returns the previous value: 1 makes every tile uniform,
 * SIZE_MAX every tile mixed, 0 restores the default. The default is 128, the end of the measured sweep
 * (run lengths 1 .. 128 at 1 Mi items): below a full wave of 64 a uniform tile idles lanes and loses
 * outright (16 per run: 582.9 ms against 296.2; 32: 389.4 against 293.7), and at 64 and 128 the two forms are equal within
 * the run-to-run spread (293.4 against 293.2, 293.6 against 293.4), so uniform wins at no run length up to 128.
 *
 * Measured on one MI355X (profiles/topen_rounds_bench.json): 64 items of 64 distinct rounds
 * take 16.8 ms in one call against 1,206 ms as 64 blsv_tlock_open calls (72 times faster); 1 Mi
 * distinct U values open at 3.56 M/s under 1 round, 3.57 M/s over 1 Ki rounds, 3.55 M/s over 32 Ki rounds and
 * 2.88 M/s over 1 Mi rounds, beside 3.64 M/s for blsv_tlock_open_dev on the one-round inputs in the same run.
 *
 * blsv_tlock_open_rounds_dev: sigs96 and counts are host memory (as sig96 of blsv_tlock_open_dev);
 * d_us48 / d_out_gt576 (4-byte aligned) / d_reject_class (optional, n) / d_sig_class (optional, m) are
 * device pointers. Asynchronous on `stream` under the single-stream rule of blsv_verify_chained_dev; no
 * class is read back.
 */
#define BLSV_REJ_TLOCK_SIG 9 /* the item's round signature did not decode (its class is in sig_class[j]) */
int blsv_tlock_open_rounds(blsv_ctx* ctx, const uint8_t* sigs96, const uint64_t* counts, size_t m,
                           const uint8_t* us48, size_t n, uint8_t* out_gt576, uint8_t* ok,
                           uint8_t* reject_class /*optional, n*/, uint8_t* sig_class /*optional, m*/);
int blsv_tlock_open_rounds_dev(blsv_ctx* ctx, const uint8_t* sigs96, const uint64_t* counts, size_t m,
                               const uint8_t* d_us48, size_t n, uint8_t* d_out_gt576,
                               uint8_t* d_reject_class /*optional*/, uint8_t* d_sig_class /*optional*/, void* stream);
int blsv_tlock_open_rounds_stats(blsv_ctx* ctx, uint64_t* prepared, uint64_t* items);
size_t blsv_set_tlock_dense_min(blsv_ctx* ctx, size_t items); /* returns the previous value */

/*
 * Opening on the latency path (opt-in). A client that holds one ciphertext, or a handful, when its round
 * arrives pays on the batch path a serial chain of one-lane stages with the chip idle. The latency
 * engine (latency contract above) has a timelock item too: one workgroup of eight waves per ciphertext
 * decodes sigma and U side by side, runs the one pair's Miller loop beside their subgroup checks, then
 * the final exponentiation and the encoding, in one launch (drand_amd/csrc/k_lat_tlock.hip).
 *
 * blsv_set_tlock_lat_max(ctx, L) returns the previous value. The default is 0 = off, or the environment
 * variable BLSV_TLOCK_LAT_MAX (a non-negative integer; anything else is ignored with a note on stderr).
 * L is clamped to the context's chunk, here and whenever the chunk shrinks (blsv_set_chunk, the
 * out-of-memory halving). With L = 0 every entry point behaves exactly as described above.
 *
 * With L > 0 the HOST forms blsv_tlock_open and blsv_tlock_open_rounds send a call of 1 .. L items to the
 * latency path (a call across rounds only while its signatures with a count of 0, which get a workgroup
 * each, are no more than L too). Larger calls, n = 0 and both _dev forms take the paths above unchanged.
 * Every output is byte for byte what the batch path returns for the same arguments: the BLSV_GT_LEN
 * bytes (zeros for a rejected item), ok, reject_class, *sig_class / sig_class[j] (signatures with a count
 * of 0 included), the class rule of an item under a sigma that does not decode, and for blsv_tlock_open
 * BLSV_EINVAL with *sig_class set and no per-item output touched. Argument validation is each entry
 * point's own, before the routing. Items that share a sigma each decode it again (that work runs beside
 * their U decode), so nothing is prepared and nothing cached: the one-entry sigma cache survives a
 * latency-path call under another sigma, and blsv_tlock_stats, blsv_tlock_open_rounds_stats and the
 * sealing counters do not move. blsv_tlock_lat_stats: *launches = latency-path calls, *items = U values
 * they processed (rejected ones included) since the context's creation; either pointer may be NULL.
 *
 * Memory: one device buffer of 96 m + 629 n bytes (+ 4 per item and per signature without items for a
 * call across rounds) beside the pipeline staging, which this path does not touch.
 *
 * Measured on one MI355X (profiles/tlock_lat_bench.json; host forms, the two modes
 * alternating call by call in one run, medians, identical bytes in every pair): a lone blsv_tlock_open
 * whose sigma changes every call takes 1.51 ms against 18.28 ms on the batch path (12.1 times faster);
 * under the same sigma every call, where the batch path has its cache hit, 1.50 ms against 14.33 ms (9.6
 * times); 64 items of 64 distinct rounds in one blsv_tlock_open_rounds 1.54 ms against 16.70 ms (10.9
 * times). One sigma, n items: 1.50 ms up to 16, 1.63 at 256 (one workgroup per compute unit), 3.20 at
 * 512, 6.27 at 1,024, 12.24 at 2,048 and 24.06 at 4,096, against 14.3 falling to 12.3 - 12.5 ms on the
 * batch path. The batch path is first faster at n = 4,096; at 2,048 the two are level. Recommended:
 * blsv_set_tlock_lat_max(ctx, 2048), or 1024 where a call should win by a factor of two.
 */
size_t blsv_set_tlock_lat_max(blsv_ctx* ctx, size_t items); /* returns the previous value */
int blsv_tlock_lat_stats(blsv_ctx* ctx, uint64_t* launches, uint64_t* items);

/*
 * Sealing: the producing half, timelock.Encrypt(key.Pairing, G1 base, group key, MessageV2(round), msg)
 * of the same test, for n messages locked to ONE round. With B = e(pk, H(MessageV2(round)))^3 computed
 * once, item i is
 *     out_us48[i]  = compress(k_i * G1)     (the ciphertext's ephemeral point U_i)
 *     out_gt576[i] = encode(B^k_i)          (K_i, the value the caller's KDF turns into a key stream)
 * and no item runs a pairing. B is in the convention of blsv_tlock_open -- the same exponent lambda, the
 * same BLSV_GT_LEN-byte encoding -- so the contract is: for sigma the round's signature under pk,
 * blsv_tlock_open(sigma, U_i) returns exactly K_i. The masking C = m XOR kdf(K_i) is the caller's.
 *
 * Inputs
 *  - pk48: the compressed G1 key; NULL = the group key (BLSV_ENOGROUP when no group is set). A key that
 *    does not decode (kilic G1.FromCompressed, subgroup check included) returns BLSV_EINVAL, and so does
 *    the point at infinity (a seal under it opens for anyone: B = 1); no output is touched in either case.
 *  - scalars32: n scalars of BLSV_SCALAR_LEN bytes, big-endian, as blsv_sign's sk32; k_i is the value
 *    mod r. An item with k_i == 0 (mod r) is refused (U would be the point at infinity and K = 1):
 *    ok[i] = 0 and BLSV_U_LEN + BLSV_GT_LEN zero bytes. Every other item has ok[i] = 1. The caller draws
 *    the scalars (uniformly in [1, r), fresh per item); the engine draws nothing.
 *
 * Secrecy: the scalars are secret until the round arrives. blsv_tlock_seal clears its device staging copy
 * of them before it returns (the _dev form reads the caller's buffer in place and keeps no copy). There is
 * NO constant-time claim: both operations walk tables of the base's multiples whose indices are the
 * scalar's four-bit digits, as blsv_sign's double-and-add branches on the key's bits.
 *
 * Base cache: the context keeps the LAST base -- the 48 key bytes, the round, and the table of B's
 * powers (552,960 bytes on the device; the table of G1's multiples, 92,160 bytes, is built once per
 * context at the first seal). A call with the same key bytes and round builds nothing; any other key
 * or round replaces the entry (one entry: A, B, A builds three times). The opening's prepared-signature
 * cache is separate and survives a seal. blsv_tlock_seal_stats: *bases = bases built, *items = scalars
 * processed (refused ones included) since the context's creation; either pointer may be NULL.
 * blsv_tlock_stats is not affected.
 *
 * Sizing: the pipeline staging is used as it is; more than a chunk of items runs in chunk-sized passes
 * with identical outputs. The two tables are the only device memory of its own.
 *
 * blsv_tlock_seal_dev: d_scalars32 / d_out_us48 / d_out_gt576 (4-byte aligned) / d_ok are device
 * pointers, pk48 is host memory. Asynchronous on `stream` under the single-stream rule of
 * blsv_verify_chained_dev, except that a (key, round) other than the cached one is built first, which
 * reads the key's decode class back (one synchronisation of `stream`).
 */
#define BLSV_SCALAR_LEN 32
int blsv_tlock_seal(blsv_ctx* ctx, const uint8_t* pk48, uint64_t round, const uint8_t* scalars32, size_t n,
                    uint8_t* out_us48, uint8_t* out_gt576, uint8_t* ok);
int blsv_tlock_seal_dev(blsv_ctx* ctx, const uint8_t* pk48, uint64_t round, const uint8_t* d_scalars32, size_t n,
                        uint8_t* d_out_us48, uint8_t* d_out_gt576, uint8_t* d_ok, void* stream);
int blsv_tlock_seal_stats(blsv_ctx* ctx, uint64_t* bases, uint64_t* items);

/*
 * Sealing to many rounds: n messages, item i locked to its OWN round rounds[i] under one key -- the shape
 * of a sealing service or relay, whose requests (round_i, message_i) pick their unlock times themselves.
 * Item i's outputs are byte for byte those of blsv_tlock_seal(ctx, pk48, rounds[i], scalars32 + 32 i, 1, ...):
 *     out_us48[i]  = compress(k_i * G1)
 *     out_gt576[i] = encode(e(pk, H(MessageV2(rounds[i])))^(3 k_i))
 * so blsv_tlock_open(sigma_{rounds[i]}, U_i) returns exactly K_i. No base is shared between items: each
 * runs one single-pair pairing e(k_i pk, H_i) of its own (k_i pk by a walk over a table of pk's
 * multiples), and the items of a pass run side by side. Any uint64 is a valid round.
 * Measured on one MI355X (profiles/tseal_rounds_bench.json): 64 items with 64 distinct
 * rounds take 17.7 ms in one call against 2,195 ms as 64 one-item blsv_tlock_seal calls; 1 Mi items with
 * 1 Mi distinct rounds seal at 2.80 M/s, beside 12.7 M/s for the same scalars to one round. A caller with
 * many items per round is better served by blsv_tlock_seal, which runs no pairing per item: a loop of it
 * over the rounds wins from somewhere between 65,536 and 262,144 items per distinct round.
 *
 * pk48, scalars32, ok and the refusal of k_i == 0 (mod r) -- ok[i] = 0 and BLSV_U_LEN + BLSV_GT_LEN zero
 * bytes, neighbours unaffected -- are blsv_tlock_seal's: NULL = the group key (BLSV_ENOGROUP without one);
 * a key that does not decode, or the point at infinity, returns BLSV_EINVAL and no output is touched.
 *
 * Secrecy: the host entry clears its device staging copy of the scalars before it returns, and both
 * entries clear the staged points k_i pk (each is as good as K_i to whoever holds it), behind the kernels
 * that read them and also when a pass fails. There is NO constant-time claim, as above.
 *
 * Key cache: the context keeps the table of the LAST key's multiples (92,160 bytes on the device), keyed
 * by the 48 key bytes. A call under the same key builds nothing; another key replaces the entry (A, B, A
 * builds three times). blsv_tlock_seal_rounds_stats: *keys = key tables built, *items = scalars
 * processed (refused ones included); either pointer may be NULL. blsv_tlock_seal_stats and
 * blsv_tlock_stats do not move, and the one-round base cache and the opening's prepared-signature cache
 * survive a call.
 *
 * Sizing: the pipeline staging is used as it is; more than a chunk of items runs in chunk-sized passes
 * with identical outputs. The key table is the only device memory of its own.
 *
 * blsv_tlock_seal_rounds_dev: d_rounds (8-byte aligned) / d_scalars32 / d_out_us48 / d_out_gt576 (4-byte
 * aligned) / d_ok are device pointers, pk48 is host memory. Asynchronous on `stream` under the
 * single-stream rule of blsv_verify_chained_dev, except that a key other than the cached one has its
 * decode class read back (one synchronisation of `stream`).
 */
int blsv_tlock_seal_rounds(blsv_ctx* ctx, const uint8_t* pk48, const uint64_t* rounds, const uint8_t* scalars32,
                           size_t n, uint8_t* out_us48, uint8_t* out_gt576, uint8_t* ok);
int blsv_tlock_seal_rounds_dev(blsv_ctx* ctx, const uint8_t* pk48, const uint64_t* d_rounds,
                               const uint8_t* d_scalars32, size_t n, uint8_t* d_out_us48, uint8_t* d_out_gt576,
                               uint8_t* d_ok, void* stream);
int blsv_tlock_seal_rounds_stats(blsv_ctx* ctx, uint64_t* keys, uint64_t* items);

/*
 * Sealing on the latency path (opt-in). The most common use of timelock encryption is one person locking
 * one message to a future round; on the batch path that call pays a serial chain of one-lane stages with
 * the chip idle. The latency engine has a sealing item too: one workgroup of eight waves per message
 * hashes the item's round while two of its waves walk the tables of G1's and the key's multiples
 * (U_i = k_i G1 compressed and stored, P_i = k_i pk), then runs the one pair's Miller loop e(P_i, H_i), the
 * final exponentiation and the encoding, in one launch (drand_amd/csrc/k_lat_tseal.hip).
 *
 * blsv_set_tseal_lat_max(ctx, L) returns the previous value. The default is 0 = off, or the environment
 * variable BLSV_TSEAL_LAT_MAX (a non-negative integer; anything else is ignored with a note on stderr).
 * L is clamped to the context's chunk, here and whenever the chunk shrinks (blsv_set_chunk, the
 * out-of-memory halving). It is a setter of its own, beside blsv_set_tlock_lat_max, because the two
 * crossovers differ. With L = 0 every entry point behaves exactly as described above.
 *
 * With L > 0 the HOST forms blsv_tlock_seal and blsv_tlock_seal_rounds send a call of 1 .. L items to the
 * latency path. Larger calls, n = 0 and both _dev forms take the paths above unchanged. Every output is
 * byte for byte what the batch path returns for the same arguments: the BLSV_U_LEN and BLSV_GT_LEN bytes,
 * ok, the zeros of a refused item, and BLSV_EINVAL / BLSV_ENOGROUP with no output touched. Argument
 * validation is each entry point's own, before the routing. Items that share a round each hash it again
 * (workgroups stay independent), so no base is built and none cached: the one-round base cache and the
 * opening's prepared-signature cache survive a latency-path call.
 *
 * Key and counters: the path reads the table of G1's multiples and the key table of
 * blsv_tlock_seal_rounds, through that entry's one-entry key cache (the same decode, the same BLSV_EINVAL;
 * a new key costs its one table build and class read-back, the group key is stable). So
 * blsv_tlock_seal_rounds_stats's *keys counts a table whichever path built it -- also one built for a
 * latency-path blsv_tlock_seal -- while its *items, blsv_tlock_seal_stats and blsv_tlock_stats do not move
 * on a latency-path call. blsv_tseal_lat_stats: *launches = latency-path calls, *items = scalars they
 * processed (refused ones included) since the context's creation; either pointer may be NULL.
 *
 * Memory and secrecy: one device buffer of 665 bytes per item (8 round + 32 scalar bytes up, 48 + 576 + 1
 * down; 657 for blsv_tlock_seal's one shared round; at most 63 bytes of padding) beside the pipeline
 * staging, which this path does not touch. The staged scalars -- device and host copies -- are cleared
 * behind the kernel before the entry returns, also when the call fails; a workgroup overwrites the
 * on-chip copy of k_i pk before it exits. There is NO constant-time claim, as above.
 *
 * Measured on one MI355X (profiles/tseal_lat_bench.json; host forms, the two modes
 * alternating call by call in one run, medians, identical bytes in every pair): a lone blsv_tlock_seal to a
 * new round every call takes 1.88 ms against 34.48 ms on the batch path (18.4 times faster); to the same
 * round every call, where the batch path has its cached base, 1.87 ms against 5.24 ms (2.8 times); 64 items
 * of 64 distinct rounds in one blsv_tlock_seal_rounds 1.92 ms against 17.80 ms (9.3 times). n items: 1.87
 * ms up to 16, 2.02 at 256 (one workgroup per compute unit), 3.97 at 512, 7.80 at 1,024, 15.24 at 2,048 and
 * 30.10 at 4,096, through either entry point, against 5.2 - 6.1 ms for blsv_tlock_seal on a cached base and
 * 17.8 - 20.1 ms for blsv_tlock_seal_rounds. The batch path is first faster at n = 1,024 for blsv_tlock_seal
 * (at 512 the latency path still wins, 3.97 against 5.26 ms) and at n = 4,096 for blsv_tlock_seal_rounds
 * (at 2,048 it wins by 1.2). Recommended: blsv_set_tseal_lat_max(ctx, 512), the bound that serves both
 * entry points; 2048 for a caller that only seals across rounds. The two table walks take at most 580
 * microseconds each with their conversions (measured alone), inside the hash's 926: off the critical path.
 */
size_t blsv_set_tseal_lat_max(blsv_ctx* ctx, size_t items); /* returns the previous value */
int blsv_tseal_lat_stats(blsv_ctx* ctx, uint64_t* launches, uint64_t* items);

/*
 * Timelock in one call: the entry points above hand the Gt value back raw and leave the key stream and the
 * XOR to the caller. The eight below are the same passes with that tail fused on the device: one lane per
 * item hashes the value it has just computed and masks the item's message bytes, so what crosses to the
 * host is mlen bytes per item, not BLSV_GT_LEN, and on the sealing side K_i never leaves the device.
 *
 * KDF. kdf selects the key stream. BLSV_KDF_SHA256_CTR is the only one:
 *     stream(G, mlen) = SHA-256(G || BE32(0)) || SHA-256(G || BE32(1)) || ...   truncated to mlen bytes
 * with G the BLSV_GT_LEN-byte encoding defined under blsv_tlock_open. THIS KDF IS THE PROJECT'S OWN. kyber's
 * timelock uses BLAKE2Xs over GT.MarshalBinary, which nothing here can pin; a ciphertext produced by kyber
 * does not open under BLSV_KDF_SHA256_CTR, nor the other way round. The argument exists so that kyber's can
 * be added beside it. Any other kdf value returns BLSV_EINVAL with no output touched.
 *
 * Messages. mlen is uniform per call, 1 .. BLSV_TLOCK_MSG_MAX bytes; messages and ciphertexts are packed
 * n x mlen bytes with no padding and NO alignment requirement, on the host and on the device. mlen = 0,
 * mlen > BLSV_TLOCK_MSG_MAX, or a byte count that overflows size_t is BLSV_EINVAL with no output touched.
 * Only the bytes [i mlen, (i + 1) mlen) of item i are written. In place is allowed: out_msgs == cs and
 * out_cs == msgs (each lane reads its bytes before it writes them); any other overlap is not.
 *
 * Contract. For every item, out_msgs[i] = cs[i] XOR stream(G_i, mlen) where G_i is the BLSV_GT_LEN bytes the
 * matching entry point -- blsv_tlock_open for blsv_tlock_decrypt, blsv_tlock_open_rounds for
 * blsv_tlock_decrypt_rounds -- returns for the same arguments; out_cs[i] = msgs[i] XOR stream(K_i, mlen)
 * with K_i from blsv_tlock_seal / blsv_tlock_seal_rounds, and out_us48 is byte for byte theirs. An item
 * without a value (a U that does not decode, an item under a sigma that does not decode, a refused scalar)
 * gets mlen zero bytes where the matching entry point writes BLSV_GT_LEN zero bytes (and BLSV_U_LEN zero
 * bytes of U when sealing). U or sigma at infinity is not a rejection: E = 1 and the item is masked with
 * stream(encode(1)), as any other value. Everything else is the matching entry point's, unchanged: ok,
 * reject_class, sig_class, BLSV_REJ_TLOCK_SIG, BLSV_EINVAL with *sig_class set and no per-item output touched
 * for a sigma that does not decode, BLSV_ENOGROUP, the refusal of k == 0 (mod r), the caches, and the
 * counters: each entry point counts in the *_stats of the pass it runs. As there, nothing checks that
 * sigma is the round's signature: a wrong one decrypts to garbage without any error (the authenticated forms
 * below, blsv_tlock_decrypt_auth*, do report it).
 *
 * Host forms: a pass uploads its cnt x mlen input bytes beside what it uploads today and downloads cnt x mlen
 * output bytes and the class bytes; the staging is the pipeline's (memory contract above, unchanged).
 * Secrecy (encrypt): K_i alone unmasks message i, so the pass's captured K values are cleared on the device
 * behind the mask kernel, also when the pass fails, beside the clearing of the scalars and of k_i pk that the
 * sealing passes do; the host forms clear their staged plaintexts too. No constant-time claim, as above.
 *
 * Latency path: the host forms follow the existing switches -- blsv_tlock_decrypt and _decrypt_rounds route
 * as blsv_tlock_open / _open_rounds do under blsv_set_tlock_lat_max, blsv_tlock_encrypt and _encrypt_rounds as
 * blsv_tlock_seal / _seal_rounds under blsv_set_tseal_lat_max. The latency kernel runs unchanged and the
 * mask kernel behind it on the same stream; the path's buffer grows by 2 mlen bytes per item, the download
 * is mlen bytes per item and the classes, blsv_tlock_lat_stats / blsv_tseal_lat_stats count the call, and
 * the outputs are byte for byte the batch path's. The _dev forms never route. There is no service entry.
 *
 * _dev forms: as the matching _dev entry point (host and device arguments, the stream rule, what is read
 * back); d_cs / d_msgs / d_out_msgs / d_out_cs are device pointers of any alignment.
 *
 * Measured on one MI355X (profiles/tcrypt_bench.json; 1 Mi items, mlen = 32, the fused entry and
 * the one it fuses alternating call by call, medians, outputs hashed every step): blsv_tlock_decrypt_dev 291.9 ms
 * against 291.7 ms for blsv_tlock_open_dev (3.59 M plaintexts/s), blsv_tlock_encrypt_dev 84.7 against 84.6 ms for
 * blsv_tlock_seal_dev (12.38 M plaintexts/s): the fused tail costs nothing measurable. The host form
 * blsv_tlock_decrypt takes 293.6 ms against 303.0 ms for blsv_tlock_open, which still owes its KDF. On the latency
 * path a lone decrypt takes 1.53 against 1.49 ms for a lone open, a lone encrypt 1.89 against 1.85 ms for a seal.
 */
#define BLSV_KDF_SHA256_CTR 1
#define BLSV_TLOCK_MSG_MAX 256
int blsv_tlock_decrypt(blsv_ctx* ctx, const uint8_t* sig96, const uint8_t* us48, const uint8_t* cs, size_t mlen,
                       size_t n, int kdf, uint8_t* out_msgs, uint8_t* ok, uint8_t* reject_class /*optional*/,
                       uint8_t* sig_class /*optional*/);
int blsv_tlock_decrypt_dev(blsv_ctx* ctx, const uint8_t* sig96, const uint8_t* d_us48, const uint8_t* d_cs, size_t mlen,
                           size_t n, int kdf, uint8_t* d_out_msgs, uint8_t* d_reject_class /*optional*/, void* stream);
int blsv_tlock_decrypt_rounds(blsv_ctx* ctx, const uint8_t* sigs96, const uint64_t* counts, size_t m,
                              const uint8_t* us48, const uint8_t* cs, size_t mlen, size_t n, int kdf, uint8_t* out_msgs,
                              uint8_t* ok, uint8_t* reject_class /*optional, n*/, uint8_t* sig_class /*optional, m*/);
int blsv_tlock_decrypt_rounds_dev(blsv_ctx* ctx, const uint8_t* sigs96, const uint64_t* counts, size_t m,
                                  const uint8_t* d_us48, const uint8_t* d_cs, size_t mlen, size_t n, int kdf,
                                  uint8_t* d_out_msgs, uint8_t* d_reject_class /*optional*/,
                                  uint8_t* d_sig_class /*optional*/, void* stream);
int blsv_tlock_encrypt(blsv_ctx* ctx, const uint8_t* pk48, uint64_t round, const uint8_t* scalars32,
                       const uint8_t* msgs, size_t mlen, size_t n, int kdf, uint8_t* out_us48, uint8_t* out_cs,
                       uint8_t* ok);
int blsv_tlock_encrypt_dev(blsv_ctx* ctx, const uint8_t* pk48, uint64_t round, const uint8_t* d_scalars32,
                           const uint8_t* d_msgs, size_t mlen, size_t n, int kdf, uint8_t* d_out_us48,
                           uint8_t* d_out_cs, uint8_t* d_ok, void* stream);
int blsv_tlock_encrypt_rounds(blsv_ctx* ctx, const uint8_t* pk48, const uint64_t* rounds, const uint8_t* scalars32,
                              const uint8_t* msgs, size_t mlen, size_t n, int kdf, uint8_t* out_us48, uint8_t* out_cs,
                              uint8_t* ok);
int blsv_tlock_encrypt_rounds_dev(blsv_ctx* ctx, const uint8_t* pk48, const uint64_t* d_rounds,
                                  const uint8_t* d_scalars32, const uint8_t* d_msgs, size_t mlen, size_t n, int kdf,
                                  uint8_t* d_out_us48, uint8_t* d_out_cs, uint8_t* d_ok, void* stream);

/*
 * Authenticated timelock: ciphertexts that report whether they opened. The scheme above cannot tell its
 * caller that a decryption failed: a ciphertext whose U or masked bytes were altered, one opened with the
 * wrong round's signature and one sealed under another key all come back as ok = 1 with plausible bytes. The
 * eight entry points below apply the Fujisaki-Okamoto transform (Boneh-Franklin "FullIdent"): the sealing
 * scalar is not drawn but derived from a random seed and the message, and the opener re-derives it and checks
 * that it reproduces U. A decrypt needs no separate beacon verification: under a wrong signature every item
 * fails its check.
 *
 * THIS INSTANTIATION IS THE PROJECT'S OWN, as BLSV_KDF_SHA256_CTR is: SHA-256 with this project's tags over
 * this project's Gt encoding. kyber's IBE hashes are BLAKE2-based and its Gt encoding is not pinned here. IT
 * IS NOT WIRE-COMPATIBLE WITH kyber OR tlock: neither opens the other's ciphertexts.
 *
 * The scheme. TAG3 = "BLSV-TLOCK-FO-H3", TAG4 = "BLSV-TLOCK-FO-H4" (16 ASCII bytes each). A ciphertext of an
 * mlen-byte message M is (U: BLSV_U_LEN bytes, V: BLSV_V_LEN bytes, W: mlen bytes); mlen follows
 * blsv_tlock_encrypt's rules (1 .. BLSV_TLOCK_MSG_MAX, uniform per call, packed, no alignment asked for) and
 * kdf must be BLSV_KDF_SHA256_CTR (anything else: BLSV_EINVAL, nothing touched).
 *     H3(s, M)    = (SHA-256(TAG3 || s || M || BE32(0)) || first 16 bytes of SHA-256(TAG3 || s || M || BE32(1)))
 *                   read as a 384-bit big-endian integer, mod r
 *     H2(G)       = SHA-256(G || BE32(0)) over the BLSV_GT_LEN-byte encoding: block 0 of BLSV_KDF_SHA256_CTR
 *     H4(s, mlen) = SHA-256(TAG4 || s || BE32(0)) || SHA-256(TAG4 || s || BE32(1)) || ...  truncated to mlen
 * Encrypt(pk, round, seed s, M): k = H3(s, M); U = compress(k G1); K = e(pk, H(MessageV2(round)))^(3k),
 * exactly the K of blsv_tlock_seal / _seal_rounds for the scalar k; V = s XOR H2(encode(K)); W = M XOR H4(s, mlen).
 * THE CALLER DRAWS THE SEEDS, BLSV_SEED_LEN fresh random bytes per item; the engine draws nothing. A seed
 * alone unmasks its message. If k == 0 (mod r) the item is refused as a zero scalar is: ok = 0 and U, V and W
 * all zeros (no SHA-256 input is known to reach this).
 * Decrypt(sigma, U, V, W): E = e(U, sigma)^3 as blsv_tlock_open computes it; s' = V XOR H2(encode(E));
 * M' = W XOR H4(s', mlen); k' = H3(s', M'). The item is good iff k' != 0 and k' G1 is the decoded U. A good
 * item gets ok = 1, class 0 and M'. Any other gets ok = 0, BLSV_REJ_TLOCK_AUTH and mlen zero bytes; its
 * neighbours are unaffected, and its candidate plaintext is never stored to memory (the check runs first).
 * Class precedence: a U that does not decode keeps its class 2..6; an item under a sigma that does not decode
 * keeps BLSV_REJ_TLOCK_SIG (rounds forms), or the call returns BLSV_EINVAL with *sig_class set (one-sigma
 * forms), exactly as the matching blsv_tlock_decrypt* does; BLSV_REJ_TLOCK_AUTH comes last. U at infinity and
 * sigma at infinity are no longer "a value like any other": E = 1 is a key everyone knows and no k' != 0 maps
 * to infinity, so both are BLSV_REJ_TLOCK_AUTH.
 *
 * Everything else is the matching entry point's -- blsv_tlock_encrypt for blsv_tlock_encrypt_auth, and so on:
 * the argument rules, BLSV_EINVAL / BLSV_ENOGROUP with nothing touched, chunked passes with identical outputs,
 * the caches, and the counters (a call counts in the *_stats of the pass it runs). In place is allowed:
 * out_msgs == ws and out_ws == msgs. One exception: d_reject_class is REQUIRED in the _decrypt_auth*_dev
 * forms, because the verdict is the point; NULL with n > 0 is BLSV_EINVAL.
 *
 * Staging: one device buffer of the feature's own, below 1 KiB per item of a pass, allocated at the first
 * authenticated call; a context that only decrypts also builds the 92,160-byte table of G1's multiples the
 * sealing uses. Secrecy (encrypt): the staged seeds, the derived scalars (the _dev forms stage them too) and
 * the captured K are cleared on the device behind the kernels that read them, also when a pass fails; the
 * host forms clear their staged plaintexts too and upload seeds and plaintexts straight from the caller's
 * memory. No constant-time claim, as above.
 *
 * Latency path: the host forms here take the batch path whatever blsv_set_tlock_lat_max /
 * blsv_set_tseal_lat_max say. They have a latency path and a switch of their own, blsv_set_tauth_lat_max
 * (below), off by default. There is no service entry and no multi-context form.
 *
 * Measured on one MI355X (profiles/tauth_bench.json; 1 Mi items, mlen = 32, the authenticated
 * entry and its mirror alternating call by call, medians): blsv_tlock_decrypt_auth_dev 303.0 ms against 291.2 ms
 * for blsv_tlock_decrypt_dev (+4.05%; 4.2% predicted from the check's 653 Fp products per item),
 * blsv_tlock_encrypt_auth_dev 85.0 against 84.5 ms for blsv_tlock_encrypt_dev.
 */
#define BLSV_SEED_LEN 32
#define BLSV_V_LEN 32
#define BLSV_REJ_TLOCK_AUTH 10 /* the item failed the re-encryption check of blsv_tlock_decrypt_auth* */
int blsv_tlock_encrypt_auth(blsv_ctx* ctx, const uint8_t* pk48, uint64_t round, const uint8_t* seeds32,
                            const uint8_t* msgs, size_t mlen, size_t n, int kdf, uint8_t* out_us48, uint8_t* out_vs32,
                            uint8_t* out_ws, uint8_t* ok);
int blsv_tlock_encrypt_auth_dev(blsv_ctx* ctx, const uint8_t* pk48, uint64_t round, const uint8_t* d_seeds32,
                                const uint8_t* d_msgs, size_t mlen, size_t n, int kdf, uint8_t* d_out_us48,
                                uint8_t* d_out_vs32, uint8_t* d_out_ws, uint8_t* d_ok, void* stream);
int blsv_tlock_encrypt_auth_rounds(blsv_ctx* ctx, const uint8_t* pk48, const uint64_t* rounds, const uint8_t* seeds32,
                                   const uint8_t* msgs, size_t mlen, size_t n, int kdf, uint8_t* out_us48,
                                   uint8_t* out_vs32, uint8_t* out_ws, uint8_t* ok);
int blsv_tlock_encrypt_auth_rounds_dev(blsv_ctx* ctx, const uint8_t* pk48, const uint64_t* d_rounds,
                                       const uint8_t* d_seeds32, const uint8_t* d_msgs, size_t mlen, size_t n, int kdf,
                                       uint8_t* d_out_us48, uint8_t* d_out_vs32, uint8_t* d_out_ws, uint8_t* d_ok,
                                       void* stream);
int blsv_tlock_decrypt_auth(blsv_ctx* ctx, const uint8_t* sig96, const uint8_t* us48, const uint8_t* vs32,
                            const uint8_t* ws, size_t mlen, size_t n, int kdf, uint8_t* out_msgs, uint8_t* ok,
                            uint8_t* reject_class /*optional*/, uint8_t* sig_class /*optional*/);
int blsv_tlock_decrypt_auth_dev(blsv_ctx* ctx, const uint8_t* sig96, const uint8_t* d_us48, const uint8_t* d_vs32,
                                const uint8_t* d_ws, size_t mlen, size_t n, int kdf, uint8_t* d_out_msgs,
                                uint8_t* d_reject_class /*required*/, void* stream);
int blsv_tlock_decrypt_auth_rounds(blsv_ctx* ctx, const uint8_t* sigs96, const uint64_t* counts, size_t m,
                                   const uint8_t* us48, const uint8_t* vs32, const uint8_t* ws, size_t mlen, size_t n,
                                   int kdf, uint8_t* out_msgs, uint8_t* ok, uint8_t* reject_class /*optional, n*/,
                                   uint8_t* sig_class /*optional, m*/);
int blsv_tlock_decrypt_auth_rounds_dev(blsv_ctx* ctx, const uint8_t* sigs96, const uint64_t* counts, size_t m,
                                       const uint8_t* d_us48, const uint8_t* d_vs32, const uint8_t* d_ws, size_t mlen,
                                       size_t n, int kdf, uint8_t* d_out_msgs, uint8_t* d_reject_class /*required*/,
                                       uint8_t* d_sig_class /*optional*/, void* stream);

/*
 * Authenticated timelock, mixed message lengths in one call: blsv_tlock_encrypt_auth_var, _encrypt_auth_rounds_var,
 * _decrypt_auth_var and _decrypt_auth_rounds_var take the argument lists of the four host forms above with
 * `size_t mlen` replaced by `const uint32_t* mlens` (n entries; blsv_verify_messages' msg_lens is the precedent).
 * The length enters k = H3(s, M), so a padded message is another ciphertext: these calls cannot be had by padding
 * and cutting back, as the unauthenticated forms' can, only by one call per distinct length -- or by these.
 *
 * msgs, ws, out_ws and out_msgs are packed back to back in item order: item i occupies [off_i, off_i + mlens[i])
 * with off_i = mlens[0] + ... + mlens[i - 1]. No alignment is asked for. Every mlens[i] must lie in
 * 1 .. BLSV_TLOCK_MSG_MAX: one bad length anywhere, a kdf other than BLSV_KDF_SHA256_CTR, or a byte count that
 * does not fit size_t returns BLSV_EINVAL with nothing touched. n == 0 reads no length.
 *
 * Byte identity: item i's U, V, W (or message), ok byte and class are exactly what the uniform entry point
 * produces for that item in a call of length mlens[i]. Everything else is the uniform counterpart's: the class
 * precedence, BLSV_REJ_TLOCK_AUTH with mlens[i] zero bytes for a failing item (its candidate plaintext never
 * stored), the one-sigma form's BLSV_EINVAL with *sig_class set, chunked passes (a pass slices the bytes at its
 * first item's offset), the caches and the counters, in place (out_msgs == ws, out_ws == msgs), and the
 * clearing of staged seeds, scalars, plaintexts and K behind the kernels, also on failure. They route by
 * blsv_set_tauth_lat_max (below) exactly as their counterparts do and move the same counters.
 *
 * On the device a pass stages the cnt + 1 prefix offsets of its items beside its bytes (4 bytes per item more);
 * a lane of k_tauth.hip's ragged kernels, or a workgroup of the latency kernels, takes its span from that table.
 * Dwords move only when every length of the pass is a multiple of 4, bytes otherwise. The lanes of a wave run
 * 1 .. 8 pieces of 32 bytes each; nothing is sorted by length.
 *
 * There are no _dev forms: lengths that live on the device cannot be validated without a read-back or a reject
 * class of their own. No ragged form of the unauthenticated blsv_tlock_encrypt* / blsv_tlock_decrypt* either:
 * padding works there.
 *
 * Measured on one MI355X (profiles/tauth_var_bench.json; 65,536 items, lengths uniform in
 * 1 .. 256, host forms, the two sides alternating call by call, medians of five pairs, identical bytes on both
 * sides): one blsv_tlock_decrypt_auth_var call takes 24.3 ms against 3,586 ms for the 256 per-length
 * blsv_tlock_decrypt_auth calls (148 times faster; 23.1 against 702 ms, 30 times, with those on the latency path at
 * the recommended (1024, 512)), one blsv_tlock_encrypt_auth_var call 7.0 against 1,465 ms (209 times; 6.7 against
 * 764 ms, 114 times). What raggedness costs: the mixed call against a uniform call of the same bytes 22.43 against
 * 22.48 ms decrypting and 6.21 against 6.14 ms encrypting (inside the box-to-box spread); the _var entry against
 * the uniform entry at a uniform 32 bytes 22.37 against 22.08 ms (+1.3%) and 6.50 against 6.19 ms (+5.1%: the
 * offset table's ~0.3 ms on a 6 ms call).
 */
int blsv_tlock_encrypt_auth_var(blsv_ctx* ctx, const uint8_t* pk48, uint64_t round, const uint8_t* seeds32,
                                const uint8_t* msgs, const uint32_t* mlens, size_t n, int kdf, uint8_t* out_us48,
                                uint8_t* out_vs32, uint8_t* out_ws, uint8_t* ok);
int blsv_tlock_encrypt_auth_rounds_var(blsv_ctx* ctx, const uint8_t* pk48, const uint64_t* rounds, const uint8_t* seeds32,
                                       const uint8_t* msgs, const uint32_t* mlens, size_t n, int kdf, uint8_t* out_us48,
                                       uint8_t* out_vs32, uint8_t* out_ws, uint8_t* ok);
int blsv_tlock_decrypt_auth_var(blsv_ctx* ctx, const uint8_t* sig96, const uint8_t* us48, const uint8_t* vs32,
                                const uint8_t* ws, const uint32_t* mlens, size_t n, int kdf, uint8_t* out_msgs, uint8_t* ok,
                                uint8_t* reject_class /*optional*/, uint8_t* sig_class /*optional*/);
int blsv_tlock_decrypt_auth_rounds_var(blsv_ctx* ctx, const uint8_t* sigs96, const uint64_t* counts, size_t m,
                                       const uint8_t* us48, const uint8_t* vs32, const uint8_t* ws, const uint32_t* mlens,
                                       size_t n, int kdf, uint8_t* out_msgs, uint8_t* ok,
                                       uint8_t* reject_class /*optional, n*/, uint8_t* sig_class /*optional, m*/);

/*
 * Authenticated timelock on the latency path: for the caller with ONE ciphertext to open or ONE message to
 * lock, or a handful. With blsv_set_tauth_lat_max(ctx, open_items, seal_items) the HOST forms
 * blsv_tlock_decrypt_auth and blsv_tlock_decrypt_auth_rounds run calls of 1 .. open_items ciphertexts, and
 * blsv_tlock_encrypt_auth and blsv_tlock_encrypt_auth_rounds calls of 1 .. seal_items messages, as ONE launch
 * with one workgroup of eight waves per item (drand_amd/csrc/k_lat_tauth_open.hip, k_lat_tauth_seal.hip,
 * DESIGN.md 8.9): the whole opening with its re-encryption check, or the whole sealing with the derivation of
 * its scalar, end to end in the workgroup. Outputs, ok bytes and classes are byte for byte the batch path's,
 * with the same class precedence; under a sigma that does not decode blsv_tlock_decrypt_auth returns
 * BLSV_EINVAL with *sig_class set and touches no per-item output. The rounds decrypt takes this path only
 * while no more than open_items of its signatures are without items. The _dev forms never route.
 *
 * A switch of its own: blsv_set_tlock_lat_max and blsv_set_tseal_lat_max do not move these calls, and this one
 * moves no other. 0 = off (the default, or the environment variables BLSV_TAUTH_OPEN_LAT_MAX /
 * BLSV_TAUTH_SEAL_LAT_MAX, parsed as BLSV_TSEAL_LAT_MAX is); SIZE_MAX keeps a value as it is. Both values are
 * clamped to the context's chunk, here and whenever the chunk shrinks. Returns the larger of the two values in
 * force after the call. blsv_tauth_lat_stats: latency-path calls and the items they processed since the
 * context's creation, per direction; any pointer may be NULL.
 *
 * The path has a device buffer and host staging of its own. The batch paths' counters, blsv_tlock_lat_stats
 * and blsv_tseal_lat_stats do not move on a routed call; the sigma cache and the (key, round) base cache
 * survive it; the encrypting side builds the key's table through blsv_tlock_seal_rounds' key cache, whose
 * *keys counts a table whichever path built it.
 *
 * Secrecy on the encrypting side: the derived scalar, k pk and K never leave the workgroup -- K is never
 * encoded; its SHA-256 midstate is computed from registers and on-chip memory, which the workgroup clears
 * before it exits -- and the staged seeds and plaintexts, on the device and in the host staging, are cleared
 * behind the kernel before the entry returns, also when the call fails. There is NO constant-time claim.
 *
 * Measured on one MI355X (profiles/tauth_lat_bench.json; host forms, mlen = 32, the two modes
 * alternating call by call in one run, medians, identical bytes, ok and classes in every pair): a lone
 * blsv_tlock_decrypt_auth takes 1.81 ms against 19.34 ms on the batch path under a new signature every call
 * (10.7 times faster) and against 14.64 ms under a cached one (8.1); a lone blsv_tlock_encrypt_auth 1.97 ms
 * against 34.72 ms to a new round (17.6) and 5.44 ms to a cached one (2.76); 64 items of 64 rounds 1.84 against
 * 17.69 ms decrypting and 2.00 against 17.83 ms encrypting. The batch path is first faster at n = 2,048
 * decrypting and at n = 1,024 encrypting. Recommended: blsv_set_tauth_lat_max(ctx, 1024, 512). Authentication
 * costs 0.27 ms per opening and 0.07 ms per sealing over the unauthenticated forms on their latency paths.
 */
size_t blsv_set_tauth_lat_max(blsv_ctx* ctx, size_t open_items, size_t seal_items);
int blsv_tauth_lat_stats(blsv_ctx* ctx, uint64_t* open_launches, uint64_t* open_items, uint64_t* seal_launches,
                         uint64_t* seal_items);

/* ---------------------------------------------------------------- thread-safe service
 *
 * Concurrent single-item callers: the reference verifies each arrival in its own goroutine -- one per
 * partial packet (core/drand_public.go:39 -> chain/beacon/node.go:112,125), one per gossip message
 * (lp2p/client/validator.go:64), one per client.Get (client/verify.go:185-207). A blsv_service may be
 * called from any number of threads at once. Each call blocks until its item is verified; the items of
 * calls that arrive close together are coalesced into ONE launch (the latency path up to lat_max
 * items, the batch pipeline beyond) by the service's dispatcher thread, and every caller gets its own
 * verdict. Coalescing window: after the first waiting item the dispatcher keeps gathering while new
 * items keep arriving within gap_us of the previous one, for at most max_wait_us (0, 0 = the defaults
 * 100 us and 2000 us; the BLSV_SVC_GAP_US / BLSV_SVC_MAX_WAIT_US environment variables override the
 * defaults); items that arrive while a launch runs form the next batch. The service owns one context
 * whose chunk is capped at 65,536 items (~2.7 GB of staging at most).
 */
typedef struct blsv_service blsv_service;

int blsv_service_create(int device, uint32_t gap_us, uint32_t max_wait_us, blsv_service** out);
/* Waits for the items already submitted, then stops the dispatcher. No call may be in flight or follow. */
void blsv_service_destroy(blsv_service* svc);

/*
 * key.Scheme.VerifyPartial(pubPoly, msg, partial) (chain/beacon/node.go:112,125): the group is passed
 * with every call as its t commitments (48 bytes each) and size n, like the reference's per-call
 * *share.PubPoly; the service keeps the PK_i tables of the groups it has seen (reshare transitions keep
 * two alive). *ok = 1/0, *reject_class (optional) = BLSV_REJ_*. Returns BLSV_EINVAL for a group whose
 * commitments do not decode (the call's own error, other callers are unaffected).
 */
int blsv_service_verify_partial(blsv_service* svc, const uint8_t* commits48, size_t t, size_t n, const uint8_t* msg,
                                size_t msg_len, const uint8_t* partial, size_t partial_len, uint8_t* ok,
                                uint8_t* reject_class);

/*
 * key.Scheme.VerifyRecovered(pub, msg, sig) (chain/beacon.go:91 via chain.VerifyBeacon; the gossip
 * validator and client.Get verify one beacon each) against the 48-byte compressed G1 key pk48.
 * Returns BLSV_EINVAL for a key that does not decode (kilic G1.FromCompressed).
 */
int blsv_service_verify_recovered(blsv_service* svc, const uint8_t* pk48, const uint8_t* msg, size_t msg_len,
                                  const uint8_t* sig96, uint8_t* ok, uint8_t* reject_class);

/* Counters since creation: launches, items verified, the largest batch. Any pointer may be NULL. */
int blsv_service_stats(blsv_service* svc, uint64_t* launches, uint64_t* items, uint64_t* max_batch);

#ifdef __cplusplus
}
#endif

#endif /* DRAND_AMD_BLSVERIFY_H */
