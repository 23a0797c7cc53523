// Internal to the HIP-side host units of libblsverify.so (blsverify.cpp, verify.cpp, threshold.cpp,
// tlock.cpp, tlockr.cpp, tseal.cpp, tsealr.cpp, tcrypt.cpp, tauth.cpp, testhooks.cpp): the pinned small copies, stage timing, the typed view of the pipeline
// staging with its launch wrappers, and the one pass loop every verification entry point runs.
#pragma once
#include <functional>
#include <initializer_list>

#include "engine_ctx.h"
#include "hostlogic.h"

#pragma GCC visibility push(hidden)  // shared between the host units, never exported

// ---- blsverify.cpp: pinned small copies on the main stream
constexpr size_t kIoCap = size_t(1) << 20;
hipError_t h2d(blsv_ctx* c, void* dst, const void* src, size_t len);
struct Down {
  void* user;
  const void* dev;
  size_t len;
};
// every download enqueued, one synchronisation of the main stream, then the bytes to the callers
hipError_t download_sync(blsv_ctx* c, std::initializer_list<Down> ds);

// Brackets one stage launch with events when profiling is on (no cost otherwise).
hipEvent_t take_event(blsv_ctx* c);
struct StageTimer {
  blsv_ctx* c;
  int stage;
  size_t items;
  hipStream_t st;
  hipEvent_t a = nullptr;
  StageTimer(blsv_ctx* c_, int stage_, size_t items_, hipStream_t st_) : c(c_), stage(stage_), items(items_), st(st_) {
    if (c->prof && (a = take_event(c))) (void)hipEventRecord(a, st);
  }
  ~StageTimer() {
    if (!a) return;
    hipEvent_t b = take_event(c);
    if (!b) return;
    (void)hipEventRecord(b, st);
    c->recs.push_back({stage, items, a, b});
  }
};

// ---- the pipeline staging, typed (engine_ctx.h says which stage owns which buffer)
struct Staging {
  uint32_t *H, *HQ, *S, *F, *FW, *LN;
  uint8_t *h_inf, *s_inf, *cls;
};
inline Staging staging(const blsv_ctx* c) {
  return {c->H.as<uint32_t>(),    c->HQ.as<uint32_t>(),   c->S.as<uint32_t>(),
          c->F.as<uint32_t>(),    c->FW.as<uint32_t>(),   c->LN.as<uint32_t>(),
          c->h_inf.as<uint8_t>(), c->s_inf.as<uint8_t>(), c->cls.as<uint8_t>()};
}

// 96-byte compressed signatures on the device: item i at d + i * stride + offset
struct SigSrc {
  const uint8_t* d;
  size_t stride, offset;
};
// the public key of item i: tab[idx ? idx[i] : 0]
struct PkSel {
  const uint32_t* tab;
  const uint8_t* inf;
  const uint32_t* idx;  // nullptr -> entry 0
};
inline PkSel group_pk(const blsv_ctx* c) { return {c->commits.as<uint32_t>(), c->commit_inf.as<uint8_t>(), nullptr}; }

// the hash stage of [base, base + cnt) into H (HQ between its kernels)
inline void hash_chained(blsv_ctx* c, const blsk::ChainedSrc& src, size_t base, size_t cnt, hipStream_t st) {
  const Staging w = staging(c);
  blsk::launch_hash_chained(src, base, cnt, w.H, w.h_inf, w.HQ, st);
}
inline void hash_messages(blsv_ctx* c, const uint8_t* d_msgs, const uint64_t* d_off, const uint32_t* d_len, size_t base,
                          size_t cnt, hipStream_t st) {
  const Staging w = staging(c);
  blsk::launch_hash_messages(d_msgs, d_off + base, d_len + base, cnt, w.H, w.h_inf, w.HQ, st);
}
// ... of the messages upload_messages staged (in_msgs, in_off, in_len)
inline void hash_uploaded(blsv_ctx* c, size_t base, size_t cnt, hipStream_t st) {
  hash_messages(c, c->in_msgs.as<uint8_t>(), c->in_off.as<uint64_t>(), c->in_len.as<uint32_t>(), base, cnt, st);
}
// the latency path over the uploaded messages; S / s_inf (optional) receive the decoded signatures
inline void lat_uploaded(blsv_ctx* c, const SigSrc& sig, size_t cnt, const PkSel& pk, uint8_t* cls, uint32_t* S,
                         uint8_t* s_inf, hipStream_t st) {
  blsk::launch_lat_messages(c->in_msgs.as<uint8_t>(), c->in_off.as<uint64_t>(), c->in_len.as<uint32_t>(), sig.d,
                            sig.stride, sig.offset, cnt, pk.tab, pk.inf, pk.idx, cls, S, s_inf, st);
}
// the final exponentiation of the values [base, base + m) of the cnt in F (W = FW); its 3-lane products
// park in HQ, free after the hash stage: the range from 0 first, a range from base behind the park of
// the base items before it (engine_ctx.h kHqWords holds both); out (optional) captures the values
inline void final_exp(blsv_ctx* c, size_t cnt, size_t base, size_t m, uint8_t* cls, hipStream_t st,
                      uint32_t* out = nullptr) {
  const Staging w = staging(c);
  blsk::launch_final_exp(w.F, w.FW, cnt, base, m, cls, st, w.HQ + (base ? blsk::FEXP_PARK_WORDS(base) : 0), out);
}
inline void final_exp(blsv_ctx* c, size_t cnt, uint8_t* cls, hipStream_t st, uint32_t* out = nullptr) {
  final_exp(c, cnt, 0, cnt, cls, st, out);
}

// ---- verify.cpp: the pass loop
// lat_max is clamped to the context's chunk on every path that sets it (the latency kernels write one
// class byte per item into the chunk-sized class buffer); the min keeps the bound local anyway
inline bool use_lat(const blsv_ctx* c, size_t n) { return n > 0 && n <= std::min(c->lat_max, c->cap); }
inline bool use_rlc(const blsv_ctx* c, size_t n) { return n > c->lat_max && n >= 2 * c->rlc.group; }

// Every pass of a batch of n items: f(base, cnt) with cnt <= cap (the staging holds one pass); stops
// at the first non-zero return
template <typename F>
inline int for_each_pass(const blsv_ctx* c, size_t n, F f) {
  for (size_t base = 0; base < n; base += c->cap) {
    const int rc = f(base, std::min(c->cap, n - base));
    if (rc) return rc;
  }
  return BLSV_OK;
}

// launches the hash stage of items [base, base + cnt) on st
using HashFn = std::function<void(size_t base, size_t cnt, hipStream_t st)>;
// What follows the head of a pass: the exact stages per item, or the randomized path's shared checks
// under the call's seed (rlc_draw_seed). The exact tail's Miller lines pass closes the signatures'
// subgroup check, so its head only decodes; the randomized tail sums signatures before any Miller
// loop, on the strength of the head's explicit check.
struct Tail {
  bool randomized = false;
  uint32_t seed[8] = {0};
  bool fused_subgroup() const { return !randomized; }
};
// where a pass leaves its verdicts (device): bit base + i of bitmap, first_bad = label0 + the lowest
// rejected index (atomic min), cls (optional) the class byte of every item of the batch
struct PassOut {
  uint64_t* bitmap;
  unsigned long long* first_bad;
  uint8_t* cls;
  uint64_t label0;
};
// stages 1 and 2 of one pass (hash beside decompression); the explicit subgroup kernels run unless
// the tail closes that check itself
int run_head(blsv_ctx* c, const SigSrc& sig, size_t base, size_t cnt, const Tail& tail, hipStream_t st,
             const HashFn& hash);
// all passes of n items, each the head and then the tail; pk.idx (when given) covers the batch and is
// sliced per pass here
int run_passes(blsv_ctx* c, size_t n, const SigSrc& sig, const PkSel& pk, const HashFn& hash, const Tail& tail,
               const PassOut& out, hipStream_t st);
// the context's own output buffers for n items, sized and cleared: bitmap, first_bad, misc when with_cls
int ctx_outputs(blsv_ctx* c, size_t n, bool with_cls, PassOut& out);

// the randomized path's seed as eight big-endian words, and the combination stage of one pass
int rlc_draw_seed(blsv_ctx* c, uint32_t (&w)[8]);
int rlc_sums(blsv_ctx* c, size_t base, size_t cnt, const uint32_t (&seed)[8], hipStream_t st);

// n signatures into in_sigs and their prevs into seeds: one prev0 (prev0_len bytes) of a continuous
// chain, or with prev_rows a 96-byte row per round (segments of length 1: every round hashes its own)
int stage_chain(blsv_ctx* c, uint64_t first_round, const uint8_t* prevs, size_t prev0_len, bool prev_rows,
                const uint8_t* sigs96, size_t n, blsk::ChainedSrc& src);
// decode cnt 48-byte G1 points into (tab, inf) on the device; their classes come back in cls
int decode_g1(blsv_ctx* c, const uint8_t* pk48, size_t cnt, DBuf& tab, DBuf& inf, std::vector<uint8_t>& cls);
// n messages packed back to back (msg_lens[i] bytes each) into in_msgs / in_off / in_len
int upload_messages(blsv_ctx* c, const uint8_t* msgs, const uint32_t* msg_lens, size_t n);

// ---- tcrypt.cpp: the fused tail of the four timelock passes (blsv_tlock_decrypt* / blsv_tlock_encrypt*,
// k_tmask.hip). mlen == 0: no mask tail, the pass ends in the Gt encoding as ever.
struct MaskTail {
  size_t mlen = 0;
  bool host = false;    // a host form: the pass's input and output bytes are staged in F (engine_ctx.h)
  bool secret = false;  // encrypt: the captured K and the staged plaintexts are cleared behind the kernel
};
// Where a host form's pass of cnt items leaves its output on the device: F behind the staged input with a
// mask tail, else the start of F
uint8_t* mask_host_out(const blsv_ctx* c, const MaskTail& mk, size_t cnt);
// The tail of a pass of cnt items whose values are captured in HQ: in = the pass's cnt x mlen input bytes
// (host memory for a host form, uploaded to F here; else device memory), d_out = cnt x mlen bytes on the
// device; flag[i] == good marks an item with a value
int mask_tail(blsv_ctx* c, const MaskTail& mk, const uint8_t* flag, uint8_t good, size_t cnt, const uint8_t* in,
              uint8_t* d_out, hipStream_t st);
// Behind the tail of an encrypting pass, also when it failed: clears the K capture in HQ and a host form's
// staged plaintexts in F
hipError_t mask_wipe(blsv_ctx* c, const MaskTail& mk, size_t cnt, hipStream_t st);

// ---- tauth.cpp: the authenticated tail of the four timelock passes (blsv_tlock_encrypt_auth* /
// blsv_tlock_decrypt_auth*, k_tauth.hip, tauth.h) in place of the mask tail. Off (the default): the pass is
// byte for byte what it was. On: the pass runs on device pointers (MaskTail::host is false: a host form stages
// its bytes in the feature's own buffer, engine_ctx.h) and mk.mlen is the message length.
// The ragged forms (blsv_tlock_*_auth*_var; offs != nullptr): the items' bytes lie back to back, item i of the
// call at offs[i] .. offs[i + 1] of rag_in and rag_out (offs: n + 1 prefix offsets on the device). The tail takes
// its spans from here and not from the byte pointers the pass hands it, which a pass steps by mk.mlen: such a
// call sets mk.mlen = 1, the shortest item, so that those pointers stay inside the buffers.
struct AuthTail {
  bool on = false;
  const uint8_t* vs = nullptr;     // decrypt: the call's n x 32 V bytes
  const uint8_t* seeds = nullptr;  // encrypt: the call's n x 32 seeds
  uint8_t* out_vs = nullptr;       // encrypt: the call's n x 32 V bytes
  const uint32_t* offs = nullptr;    // ragged: the offsets from this part's first item on
  const uint8_t* rag_in = nullptr;   // ragged: the call's W bytes (decrypt) or message bytes (encrypt)
  uint8_t* rag_out = nullptr;        // ragged: the call's message bytes (decrypt) or W bytes (encrypt)
  bool rag_words = false;            // ragged: every length of the call is a multiple of 4
  AuthTail at(size_t base) const {  // the part of the pass that starts at item base
    AuthTail a = *this;
    if (vs) a.vs += base * 32;
    if (seeds) a.seeds += base * 32;
    if (out_vs) a.out_vs += base * 32;
    if (offs) a.offs += base;
    return a;
  }
};
// The tail of an opening pass of cnt items: E in HQ, the decoded U table in H / h_inf, the class bytes in
// s_inf (read and written); ws = the pass's cnt x mlen W bytes, d_out = cnt x mlen message bytes
int auth_open_tail(blsv_ctx* c, const AuthTail& au, const MaskTail& mk, size_t cnt, const uint8_t* ws, uint8_t* d_out,
                   hipStream_t st);
// The tail of a sealing pass of cnt items: K in HQ, cls = launch_tseal_u's class bytes; msgs = the pass's
// cnt x mlen message bytes, d_out_ws = cnt x mlen W bytes
int auth_seal_tail(blsv_ctx* c, const AuthTail& au, const MaskTail& mk, const uint8_t* cls, size_t cnt,
                   const uint8_t* msgs, uint8_t* d_out_ws, hipStream_t st);

// ---- the passes of the four timelock units, shared with tauth.cpp (each is described where it is defined)
int tlock_prepare_sig(blsv_ctx* c, const uint8_t* sig96, hipStream_t st, uint8_t* sig_class);
int tlock_passes(blsv_ctx* c, bool host, const uint8_t* us, size_t n, uint8_t* out, uint8_t* cls, hipStream_t st,
                 const MaskTail& mk = MaskTail(), const uint8_t* mk_in = nullptr, const AuthTail& au = AuthTail());
int rounds_passes(blsv_ctx* c, bool host, const uint8_t* sigs96, const uint64_t* counts, size_t m, const uint8_t* us,
                  size_t n, uint8_t* out, uint8_t* cls, uint8_t* d_sig_class, hipStream_t st,
                  const MaskTail& mk = MaskTail(), const uint8_t* mk_in = nullptr, const AuthTail& au = AuthTail());
int seal_prepare(blsv_ctx* c, const uint8_t* pk48, uint64_t round, size_t n, hipStream_t st);
int seal_passes(blsv_ctx* c, bool host, const uint8_t* scalars, size_t n, uint8_t* us, uint8_t* gt, uint8_t* ok,
                hipStream_t st, const MaskTail& mk = MaskTail(), const uint8_t* mk_in = nullptr,
                const AuthTail& au = AuthTail());
int sealr_passes(blsv_ctx* c, bool host, const uint64_t* rounds, const uint8_t* scalars, size_t n, uint8_t* us,
                 uint8_t* gt, uint8_t* ok, hipStream_t st, const MaskTail& mk = MaskTail(),
                 const uint8_t* mk_in = nullptr, const AuthTail& au = AuthTail());

// ---- tlock.cpp: a host call of n >= 1 items on the latency path (hostlogic.h tlock_lat_routes). The m
// signatures, item i under sig_of[i] (null: all under signature 0), the n_idle signatures idle[] classed
// alone. o points into the context's host staging, valid until the next call; copy_out hands the items over.
// A decrypting call (mlen != 0) also passes its n x mlen ciphertext bytes cs: the mask kernel runs behind the
// latency kernel and o.gt points to the n x mlen masked bytes instead (copy_out's out_len = mlen).
struct TlockLatOut {
  const uint8_t *gt, *cls, *sig_cls;  // n x 576 bytes, n item classes, m signature classes
};
int tlock_lat_run(blsv_ctx* c, const uint8_t* sigs96, size_t m, const uint32_t* sig_of, const uint32_t* idle,
                  size_t n_idle, const uint8_t* us48, size_t n, TlockLatOut& o, const uint8_t* cs = nullptr,
                  size_t mlen = 0);
void tlock_lat_copy_out(const TlockLatOut& o, size_t n, uint8_t* out, uint8_t* ok, uint8_t* reject_class,
                        size_t out_len = BLSV_GT_LEN);

// ---- tsealr.cpp: T1 and the key table TK of pk48 behind the one-entry key cache (BLSV_EINVAL for a key that
// does not decode or is the point at infinity, before anything else runs; no output is touched)
int sealr_prepare(blsv_ctx* c, const uint8_t* pk48, size_t n, hipStream_t st);

// ---- tseal_lat.cpp: a host call of n >= 1 items on the latency path (hostlogic.h tseal_lat_routes) under
// the key pk48: item i to rounds[i], or every item to `round` when rounds is null
// An encrypting call (mlen != 0) also passes its n x mlen message bytes: the mask kernel runs behind the
// latency kernel and `out` receives the n x mlen ciphertext bytes instead of the n x 576 Gt bytes.
int tseal_lat_run(blsv_ctx* c, const uint8_t* pk48, const uint64_t* rounds, uint64_t round, const uint8_t* scalars32,
                  size_t n, uint8_t* out_us48, uint8_t* out, uint8_t* ok, const uint8_t* msgs = nullptr, size_t mlen = 0);

// ---- tauth.cpp: T1, the table of G1's multiples, built once per context by whoever needs it first
int auth_t1(blsv_ctx* c, hipStream_t st);

// ---- tauth_lat.cpp: a host call of n >= 1 items of the authenticated forms on the latency path (hostlogic.h
// tauth_lat_routes; blsv_set_tauth_lat_max), after the entry point's own argument checks. Decrypting: the
// arguments of tlock_lat_run with the items' V and W bytes; o.gt points to the n x mlen message bytes (zeros for
// an item whose class is not 0), so tlock_lat_copy_out with out_len = mlen hands the items over.
// mlens != nullptr (the ragged forms): item i has mlens[i] bytes, packed back to back in ws and in o.gt, `bytes`
// in all (hostlogic.h tauth_var_fits), and mlen is not read.
int tauth_lat_open_run(blsv_ctx* c, const uint8_t* sigs96, size_t m, const uint32_t* sig_of, const uint32_t* idle,
                       size_t n_idle, const uint8_t* us48, const uint8_t* vs32, const uint8_t* ws, size_t mlen, size_t n,
                       TlockLatOut& o, const uint32_t* mlens = nullptr, size_t bytes = 0);
// Encrypting under the key pk48: item i to rounds[i], or every item to `round` when rounds is null
int tauth_lat_seal_run(blsv_ctx* c, const uint8_t* pk48, const uint64_t* rounds, uint64_t round, const uint8_t* seeds32,
                       const uint8_t* msgs, size_t mlen, size_t n, uint8_t* out_us48, uint8_t* out_vs32, uint8_t* out_ws,
                       uint8_t* ok, const uint32_t* mlens = nullptr, size_t bytes = 0);

// ---- sign_lat.cpp: a blsv_sign call of n >= 1 messages on the latency path (hostlogic.h sign_lat_routes),
// after the entry point's own argument checks. sk: the key reduced mod r (hostlogic.h scalar_mod_r); index, msgs,
// msg_lens and out as blsv_sign takes them.
int sign_lat_run(blsv_ctx* c, const uint32_t (&sk)[8], int32_t index, const uint8_t* msgs, const uint32_t* msg_lens,
                 size_t n, uint8_t* out);

// ---- tseal.cpp: the key a sealing call runs under -- pk48, or the group key (BLSV_ENOGROUP without one)
int seal_key(blsv_ctx* c, const uint8_t* pk48, const uint8_t** key);

#pragma GCC visibility pop
