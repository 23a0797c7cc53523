// Timelock sealing: blsv_tlock_seal* (include/blsverify.h "timelock", tseal.h). The base B of a
// (key, round) is one item through the opening's own stages -- hash, line table, f pass, final
// exponentiation -- and is cached with the table of its powers; then per pass U_i = k_i G1 and
// K_i = B^k_i by table walks and the opening's Gt encoding, all in the pipeline staging (engine_ctx.h
// lists which buffer holds what). The opening's sigma cache (tlock.cpp) is not touched.
// With blsv_set_tseal_lat_max the host form hands calls of a few items to the latency path (tseal_lat.cpp).
#include "host_internal.h"

// The base's line table sits in LN behind the one-item park of the final exponentiation
static uint32_t* seal_line_tab(const Staging& w) { return w.LN + blsk::FEXP_PARK_WORDS(1); }

// Builds T1 once, and B with T2 unless (key, round) is the cached base. The key's class is read back
// (the one synchronisation of a call, and only on a new base); a key that does not decode or is the
// point at infinity returns BLSV_EINVAL before anything else runs.
int seal_prepare(blsv_ctx* c, const uint8_t* pk48, uint64_t round, size_t n, hipStream_t st) {
  tseal_state& t = c->tseal;
  if (t.valid && t.round == round && memcmp(t.pk, pk48, 48) == 0) return BLSV_OK;
  int rc = ensure_workspace(c, std::max(n, size_t(1)));  // the call's passes find it allocated
  if (rc) return rc;
  const Staging w = staging(c);
  uint32_t* key = w.S;
  uint8_t *key_inf = w.s_inf, *key_cls = w.cls, *zero_cls = w.cls + 1;
  HIPCHK(c, c->misc.ensure(48));
  HIPCHK(c, hipMemcpyAsync(c->misc.p, pk48, 48, hipMemcpyHostToDevice, st));
  blsk::launch_decompress_g1(c->misc.as<uint8_t>(), 1, key, key_inf, key_cls, st);
  HIPCHK(c, hipGetLastError());
  uint8_t flags[2] = {0xff, 0xff};  // class, infinity
  HIPCHK(c, hipMemcpyAsync(&flags[0], key_cls, 1, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(&flags[1], key_inf, 1, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (flags[0] != BLSV_REJ_OK) return fail(c, BLSV_EINVAL, "tlock_seal: public key rejected (class %d)", (int)flags[0]);
  if (flags[1]) return fail(c, BLSV_EINVAL, "tlock_seal: the public key is the point at infinity");
  t.valid = false;
  HIPCHK(c, t.t1.ensure(blsk::kTsealT1Words * 4));
  HIPCHK(c, t.t2.ensure(blsk::kTsealT2Words * 4));
  if (!t.t1_built) {
    blsk::launch_tseal_g1_table(t.t1.as<uint32_t>(), st);
    t.t1_built = true;
  }
  HIPCHK(c, hipMemsetAsync(zero_cls, 0, 1, st));
  {
    StageTimer tm(c, ST_HASH, 1, st);
    blsk::launch_hash_unchained(nullptr, round, 0, 1, w.H, w.h_inf, w.HQ, st);
  }
  {
    StageTimer tm(c, ST_TLOCK, 1, st);
    // a one-item hash output is the one-entry S staging the preparation reads (both SoA of stride 1)
    blsk::launch_tlock_prepare(w.H, w.h_inf, zero_cls, seal_line_tab(w), st);
    blsk::launch_tlock_f(seal_line_tab(w), key, key_inf, key_cls, w.h_inf, 1, w.F, st);
  }
  {
    StageTimer tm(c, ST_FEXP, 1, st);
    // the exponentiation marks a value other than 1 in the class byte: the key's own, no longer needed
    blsk::launch_final_exp(w.F, w.FW, 1, 0, 1, key_cls, st, w.LN, w.HQ);
  }
  blsk::launch_tseal_gt_table(w.HQ, t.t2.as<uint32_t>(), st);
  HIPCHK(c, hipGetLastError());
  memcpy(t.pk, pk48, 48);
  t.round = round;
  t.valid = true;
  t.bases++;
  return BLSV_OK;
}

// One pass of cnt <= cap items: d_scalars (cnt x 32 bytes) -> d_us (cnt x 48), d_gt (cnt x 576), d_ok (cnt). With
// a mask tail (mk.mlen != 0; blsv_tlock_encrypt*) the encoding is replaced by the mask kernel over the pass's
// message bytes mk_in: d_gt gets cnt x mlen ciphertext bytes. With an authenticated tail (au.on;
// blsv_tlock_encrypt_auth*, device pointers only) d_scalars is the derived-scalar row and d_gt gets the W bytes.
static int seal_pass(blsv_ctx* c, const uint8_t* d_scalars, size_t cnt, uint8_t* d_us, uint8_t* d_gt, uint8_t* d_ok,
                     hipStream_t st, const MaskTail& mk, const uint8_t* mk_in, const AuthTail& au = AuthTail()) {
  const tseal_state& t = c->tseal;
  const Staging w = staging(c);
  uint8_t* cls = w.s_inf;
  {
    StageTimer tm(c, ST_TLOCK, cnt, st);
    blsk::launch_tseal_u(t.t1.as<uint32_t>(), d_scalars, cnt, d_us, d_ok, cls, st);
    blsk::launch_tseal_gt(t.t2.as<uint32_t>(), d_scalars, cls, cnt, w.HQ, st);
  }
  if (au.on) {
    const int rc = auth_seal_tail(c, au, mk, cls, cnt, mk_in, d_gt, st);
    if (rc) return rc;
  } else if (mk.mlen) {
    const int rc = mask_tail(c, mk, cls, BLSV_REJ_OK, cnt, mk_in, d_gt, st);
    if (rc) return rc;
  } else {
    blsk::launch_tlock_encode(w.HQ, cls, cnt, d_gt, st);
  }
  HIPCHK(c, hipGetLastError());
  return BLSV_OK;
}

// Every pass of n items under the prepared base. Device buffers (host == false): read and written in
// place on st. Host buffers: a pass's scalars travel in S and are cleared there behind the kernels that
// read them, its U bytes come back through H, its ok bytes through h_inf and its encoded values through
// F, and each pass ends with the download's synchronisation. With a mask tail, mk_in is the call's n x mlen
// message bytes and gt receives n x mlen ciphertext bytes; a host call's pass stages both in F (mask_tail),
// and the captured K (with a host call's staged plaintexts) is cleared behind the kernel, also when the
// pass failed.
int seal_passes(blsv_ctx* c, bool host, const uint8_t* scalars, size_t n, uint8_t* us, uint8_t* gt, uint8_t* ok,
                hipStream_t st, const MaskTail& mk, const uint8_t* mk_in, const AuthTail& au) {
  int rc = ensure_workspace(c, n);
  if (rc) return rc;
  const size_t out_len = mk.mlen ? mk.mlen : BLSV_GT_LEN;
  for (size_t base = 0; base < n; base += c->cap) {
    const size_t cnt = std::min(c->cap, n - base);
    const uint8_t* pass_in = mk.mlen ? mk_in + base * mk.mlen : nullptr;
    if (host) {
      uint8_t* d_out = mask_host_out(c, mk, cnt);
      HIPCHK(c, hipMemcpyAsync(c->S.p, scalars + base * BLSV_SCALAR_LEN, cnt * BLSV_SCALAR_LEN, hipMemcpyHostToDevice, st));
      rc = seal_pass(c, c->S.as<uint8_t>(), cnt, c->H.as<uint8_t>(), d_out, c->h_inf.as<uint8_t>(), st, mk, pass_in);
      hipError_t wipe = hipMemsetAsync(c->S.p, 0, cnt * BLSV_SCALAR_LEN, st);  // also when the pass failed
      const hipError_t wipe_k = mask_wipe(c, mk, cnt, st);
      if (wipe == hipSuccess) wipe = wipe_k;
      if (rc) return rc;
      HIPCHK(c, wipe);
      HIPCHK(c, download_sync(c, {{us + base * BLSV_U_LEN, c->H.p, cnt * BLSV_U_LEN},
                                  {gt + base * out_len, d_out, cnt * out_len},
                                  {ok + base, c->h_inf.p, cnt}}));
    } else {
      rc = seal_pass(c, scalars + base * BLSV_SCALAR_LEN, cnt, us + base * BLSV_U_LEN, gt + base * out_len, ok + base,
                     st, mk, pass_in, au.at(base));
      const hipError_t wipe_k = mask_wipe(c, mk, cnt, st);
      if (rc) return rc;
      HIPCHK(c, wipe_k);
    }
  }
  c->tseal.items += n;
  return BLSV_OK;
}

// the key a call seals under: pk48, or the group key (shared with tsealr.cpp)
int seal_key(blsv_ctx* c, const uint8_t* pk48, const uint8_t** key) {
  if (pk48) {
    *key = pk48;
    return BLSV_OK;
  }
  if (!c->has_group || c->group_bytes.size() < 48) return fail(c, BLSV_ENOGROUP, "tlock_seal: no group key set");
  *key = c->group_bytes.data();
  return BLSV_OK;
}

extern "C" {

int blsv_tlock_seal(blsv_ctx* c, const uint8_t* pk48, uint64_t round, const uint8_t* scalars32, size_t n,
                    uint8_t* out_us48, uint8_t* out_gt576, uint8_t* ok) {
  if (!c) return BLSV_EINVAL;
  if (n && (!scalars32 || !out_us48 || !out_gt576 || !ok)) return fail(c, BLSV_EINVAL, "tlock_seal: bad arguments");
  (void)hipSetDevice(c->device);
  const uint8_t* key;
  int rc = seal_key(c, pk48, &key);
  if (rc) return rc;
  if (tseal_lat_routes(n, std::min(c->tseal_lat.lat_max, c->chunk)))
    return tseal_lat_run(c, key, nullptr, round, scalars32, n, out_us48, out_gt576, ok);
  rc = seal_prepare(c, key, round, n, c->stream);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  return seal_passes(c, true, scalars32, n, out_us48, out_gt576, ok, c->stream);
}

int blsv_tlock_seal_dev(blsv_ctx* c, const uint8_t* pk48, uint64_t round, const uint8_t* d_scalars32, size_t n,
                        uint8_t* d_out_us48, uint8_t* d_out_gt576, uint8_t* d_ok, void* stream) {
  if (!c) return BLSV_EINVAL;
  if ((n && (!d_scalars32 || !d_out_us48 || !d_out_gt576 || !d_ok)) || ((uintptr_t)d_out_gt576 & 3))
    return fail(c, BLSV_EINVAL, "tlock_seal_dev: bad arguments");
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  const uint8_t* key;
  int rc = seal_key(c, pk48, &key);
  if (rc) return rc;
  rc = seal_prepare(c, key, round, n, st);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  return seal_passes(c, false, d_scalars32, n, d_out_us48, d_out_gt576, d_ok, st);
}

int blsv_tlock_encrypt(blsv_ctx* c, const uint8_t* pk48, uint64_t round, const uint8_t* scalars32, const uint8_t* msgs,
                       size_t mlen, size_t n, int kdf, uint8_t* out_us48, uint8_t* out_cs, uint8_t* ok) {
  if (!c) return BLSV_EINVAL;
  if ((n && (!scalars32 || !msgs || !out_us48 || !out_cs || !ok)) || !tcrypt_fits(kdf, mlen, n))
    return fail(c, BLSV_EINVAL, "tlock_encrypt: bad arguments");
  (void)hipSetDevice(c->device);
  const uint8_t* key;
  int rc = seal_key(c, pk48, &key);
  if (rc) return rc;
  if (tseal_lat_routes(n, std::min(c->tseal_lat.lat_max, c->chunk)))
    return tseal_lat_run(c, key, nullptr, round, scalars32, n, out_us48, out_cs, ok, msgs, mlen);
  rc = seal_prepare(c, key, round, n, c->stream);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  MaskTail mk;
  mk.mlen = mlen;
  mk.host = mk.secret = true;
  return seal_passes(c, true, scalars32, n, out_us48, out_cs, ok, c->stream, mk, msgs);
}

int blsv_tlock_encrypt_dev(blsv_ctx* c, const uint8_t* pk48, uint64_t round, const uint8_t* d_scalars32,
                           const uint8_t* d_msgs, size_t mlen, size_t n, int kdf, uint8_t* d_out_us48, uint8_t* d_out_cs,
                           uint8_t* d_ok, void* stream) {
  if (!c) return BLSV_EINVAL;
  if ((n && (!d_scalars32 || !d_msgs || !d_out_us48 || !d_out_cs || !d_ok)) || !tcrypt_fits(kdf, mlen, n))
    return fail(c, BLSV_EINVAL, "tlock_encrypt_dev: bad arguments");
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  const uint8_t* key;
  int rc = seal_key(c, pk48, &key);
  if (rc) return rc;
  rc = seal_prepare(c, key, round, n, st);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  MaskTail mk;
  mk.mlen = mlen;
  mk.secret = true;
  return seal_passes(c, false, d_scalars32, n, d_out_us48, d_out_cs, d_ok, st, mk, d_msgs);
}

int blsv_tlock_seal_stats(blsv_ctx* c, uint64_t* bases, uint64_t* items) {
  if (!c) return BLSV_EINVAL;
  if (bases) *bases = c->tseal.bases;
  if (items) *items = c->tseal.items;
  return BLSV_OK;
}

}  // extern "C"
