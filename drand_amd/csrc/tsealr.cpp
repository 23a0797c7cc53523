// Timelock sealing to many rounds: blsv_tlock_seal_rounds* (include/blsverify.h "timelock", tsealr.h).
// Item i is locked to its own round, so no base is shared: per pass U_i = k_i G1 (the one-round seal's
// kernel and T1), P_i = k_i pk by a walk over the cached key table, H_i = H(MessageV2(round_i)), the
// single-pair Miller passes of (P_i, H_i), the final exponentiation with its capture output and the
// opening's Gt encoding, all in the pipeline staging (engine_ctx.h lists which buffer holds what). The
// one-round base cache (tseal.cpp) and the opening's sigma cache (tlock.cpp) are not touched.
// With blsv_set_tseal_lat_max the host form hands calls of a few items to the latency path (tseal_lat.cpp),
// which builds the key table through sealr_prepare below.
#include "host_internal.h"

// Builds T1 once, and the key table unless pk48 is the cached key. The key's class is read back (the one
// synchronisation of a call, and only on a new key); a key that does not decode or is the point at
// infinity returns BLSV_EINVAL before anything else runs. Shared with the latency path (tseal_lat.cpp).
int sealr_prepare(blsv_ctx* c, const uint8_t* pk48, size_t n, hipStream_t st) {
  tsealr_state& t = c->tsealr;
  if (t.valid && memcmp(t.pk, pk48, 48) == 0) return BLSV_OK;  // T1 was built with the entry
  int rc = ensure_workspace(c, std::max(n, size_t(1)));  // the call's passes find it allocated
  if (rc) return rc;
  const Staging w = staging(c);
  uint32_t* key = w.S;
  uint8_t *key_inf = w.s_inf, *key_cls = w.cls;
  HIPCHK(c, c->misc.ensure(48));
  HIPCHK(c, hipMemcpyAsync(c->misc.p, pk48, 48, hipMemcpyHostToDevice, st));
  blsk::launch_decompress_g1(c->misc.as<uint8_t>(), 1, key, key_inf, key_cls, st);
  HIPCHK(c, hipGetLastError());
  uint8_t flags[2] = {0xff, 0xff};  // class, infinity
  HIPCHK(c, hipMemcpyAsync(&flags[0], key_cls, 1, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(&flags[1], key_inf, 1, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (flags[0] != BLSV_REJ_OK)
    return fail(c, BLSV_EINVAL, "tlock_seal_rounds: public key rejected (class %d)", (int)flags[0]);
  if (flags[1]) return fail(c, BLSV_EINVAL, "tlock_seal_rounds: the public key is the point at infinity");
  t.valid = false;
  HIPCHK(c, c->tseal.t1.ensure(blsk::kTsealT1Words * 4));  // the generator's table is the one-round seal's
  if (!c->tseal.t1_built) {
    blsk::launch_tseal_g1_table(c->tseal.t1.as<uint32_t>(), st);
    c->tseal.t1_built = true;
  }
  HIPCHK(c, t.tk.ensure(blsk::kTsealT1Words * 4));
  blsk::launch_tseal_key_table(key, t.tk.as<uint32_t>(), st);
  HIPCHK(c, hipGetLastError());
  memcpy(t.pk, pk48, 48);
  t.valid = true;
  t.keys++;
  return BLSV_OK;
}

// One pass of cnt <= cap items: d_rounds (cnt), d_scalars (cnt x 32 bytes) -> d_us (cnt x 48), d_gt
// (cnt x 576), d_ok (cnt). The points P_i wait in S (seal_rounds_layout) for the lines pass. With a mask tail
// (mk.mlen != 0; blsv_tlock_encrypt_rounds*) the encoding is replaced by the mask kernel over the pass's message
// bytes mk_in: d_gt gets cnt x mlen ciphertext bytes. An authenticated tail (au.on) as in tseal.cpp's pass.
static int sealr_pass(blsv_ctx* c, const uint64_t* d_rounds, const uint8_t* d_scalars, size_t cnt, uint8_t* d_us,
                      uint8_t* d_gt, uint8_t* d_ok, hipStream_t st, const MaskTail& mk, const uint8_t* mk_in,
                      const AuthTail& au = AuthTail()) {
  const Staging w = staging(c);
  uint32_t* P = w.S + seal_rounds_layout(cnt).o_p / 4;
  uint8_t* cls = w.s_inf;
  {
    StageTimer tm(c, ST_TLOCK, cnt, st);
    blsk::launch_tseal_u(c->tseal.t1.as<uint32_t>(), d_scalars, cnt, d_us, d_ok, cls, st);
    // pk has order r and k_i < r: the walk never meets jac_add_aff's exceptional branches (tsealr.h)
    blsk::launch_tsealr_point(c->tsealr.tk.as<uint32_t>(), d_scalars, cls, cnt, P, st);
  }
  // the final exponentiation marks a value other than 1 in the class bytes it is given: it gets a copy
  HIPCHK(c, hipMemcpyAsync(w.cls, cls, cnt, hipMemcpyDeviceToDevice, st));
  {
    StageTimer tm(c, ST_HASH, cnt, st);
    blsk::launch_hash_unchained(d_rounds, 0, 0, cnt, w.H, w.h_inf, w.HQ, st);
  }
  {
    StageTimer tm(c, ST_MILLER, cnt, st);
    blsk::launch_miller_lines1(P, w.H, w.h_inf, cls, cnt, w.LN, st);
    blsk::launch_miller_f1(w.LN, w.h_inf, cls, cnt, w.F, st);
  }
  {
    StageTimer tm(c, ST_FEXP, cnt, st);
    // the lines are read: the park goes to LN and the values are captured in HQ, as in an opening
    blsk::launch_final_exp(w.F, w.FW, cnt, 0, cnt, w.cls, st, w.LN, w.HQ);
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

// Every pass of n items under the prepared key. Device buffers (host == false): read and written in place
// on st. Host buffers: a pass's scalars and rounds travel in S behind the P table, its U and ok bytes come
// back from there and its encoded values through F, and each pass ends with the download's
// synchronisation. Either way the P table -- and a host call's scalars with it -- is cleared behind the
// kernels that read it, also when the pass failed. With a mask tail, mk_in is the call's n x mlen message bytes
// and gt receives n x mlen ciphertext bytes; a host call's pass stages both in F (mask_tail), and the captured
// K (with a host call's staged plaintexts) is cleared with the P table.
int sealr_passes(blsv_ctx* c, bool host, const uint64_t* rounds, const uint8_t* scalars, size_t n, uint8_t* us,
                 uint8_t* gt, uint8_t* ok, hipStream_t st, const MaskTail& mk, const uint8_t* mk_in, const AuthTail& au) {
  int rc = ensure_workspace(c, n);
  if (rc) return rc;
  const size_t out_len = mk.mlen ? mk.mlen : BLSV_GT_LEN;
  for (size_t base = 0; base < n; base += c->cap) {
    const size_t cnt = std::min(c->cap, n - base);
    const SealRoundsLayout l = seal_rounds_layout(cnt);
    const uint8_t* pass_in = mk.mlen ? mk_in + base * mk.mlen : nullptr;
    uint8_t* d_out = mask_host_out(c, mk, cnt);  // a host call's
    uint8_t* S = c->S.as<uint8_t>();
    if (host) {
      hipError_t up = hipMemcpyAsync(S + l.o_scalars, scalars + base * BLSV_SCALAR_LEN, cnt * BLSV_SCALAR_LEN,
                                     hipMemcpyHostToDevice, st);
      if (up == hipSuccess) up = hipMemcpyAsync(S + l.o_rounds, rounds + base, cnt * 8, hipMemcpyHostToDevice, st);
      rc = up != hipSuccess ? fail(c, BLSV_EHIP, "tlock_seal_rounds: upload: %s", hipGetErrorString(up))
                            : sealr_pass(c, (const uint64_t*)(S + l.o_rounds), S + l.o_scalars, cnt, S + l.o_us, d_out,
                                         S + l.o_ok, st, mk, pass_in);
    } else {
      rc = sealr_pass(c, rounds + base, scalars + base * BLSV_SCALAR_LEN, cnt, us + base * BLSV_U_LEN,
                      gt + base * out_len, ok + base, st, mk, pass_in, au.at(base));
    }
    hipError_t wipe = hipMemsetAsync(S, 0, host ? l.secret : l.o_scalars, st);
    const hipError_t wipe_k = mask_wipe(c, mk, cnt, st);
    if (wipe == hipSuccess) wipe = wipe_k;
    if (rc) return rc;
    HIPCHK(c, wipe);
    if (host)
      HIPCHK(c, download_sync(c, {{us + base * BLSV_U_LEN, S + l.o_us, cnt * BLSV_U_LEN},
                                  {gt + base * out_len, d_out, cnt * out_len},
                                  {ok + base, S + l.o_ok, cnt}}));
  }
  c->tsealr.items += n;
  return BLSV_OK;
}

extern "C" {

int blsv_tlock_seal_rounds(blsv_ctx* c, const uint8_t* pk48, const uint64_t* rounds, const uint8_t* scalars32, size_t n,
                           uint8_t* out_us48, uint8_t* out_gt576, uint8_t* ok) {
  if (!c) return BLSV_EINVAL;
  if ((n && (!rounds || !scalars32 || !out_us48 || !out_gt576 || !ok)) || !seal_rounds_fits(n))
    return fail(c, BLSV_EINVAL, "tlock_seal_rounds: bad arguments");
  (void)hipSetDevice(c->device);
  const uint8_t* key;
  int rc = seal_key(c, pk48, &key);
  if (rc) return rc;
  if (tseal_lat_routes(n, std::min(c->tseal_lat.lat_max, c->chunk)))
    return tseal_lat_run(c, key, rounds, 0, scalars32, n, out_us48, out_gt576, ok);
  rc = sealr_prepare(c, key, n, c->stream);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  return sealr_passes(c, true, rounds, scalars32, n, out_us48, out_gt576, ok, c->stream);
}

int blsv_tlock_seal_rounds_dev(blsv_ctx* c, const uint8_t* pk48, const uint64_t* d_rounds, const uint8_t* d_scalars32,
                               size_t n, uint8_t* d_out_us48, uint8_t* d_out_gt576, uint8_t* d_ok, void* stream) {
  if (!c) return BLSV_EINVAL;
  if ((n && (!d_rounds || !d_scalars32 || !d_out_us48 || !d_out_gt576 || !d_ok)) || ((uintptr_t)d_out_gt576 & 3) ||
      ((uintptr_t)d_rounds & 7) || !seal_rounds_fits(n))
    return fail(c, BLSV_EINVAL, "tlock_seal_rounds_dev: bad arguments");
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  const uint8_t* key;
  int rc = seal_key(c, pk48, &key);
  if (rc) return rc;
  rc = sealr_prepare(c, key, n, st);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  return sealr_passes(c, false, d_rounds, d_scalars32, n, d_out_us48, d_out_gt576, d_ok, st);
}

int blsv_tlock_encrypt_rounds(blsv_ctx* c, const uint8_t* pk48, const uint64_t* rounds, const uint8_t* scalars32,
                              const uint8_t* msgs, size_t mlen, size_t n, int kdf, uint8_t* out_us48, uint8_t* out_cs,
                              uint8_t* ok) {
  if (!c) return BLSV_EINVAL;
  if ((n && (!rounds || !scalars32 || !msgs || !out_us48 || !out_cs || !ok)) || !tcrypt_fits(kdf, mlen, n) ||
      !seal_rounds_fits(n))
    return fail(c, BLSV_EINVAL, "tlock_encrypt_rounds: bad arguments");
  (void)hipSetDevice(c->device);
  const uint8_t* key;
  int rc = seal_key(c, pk48, &key);
  if (rc) return rc;
  if (tseal_lat_routes(n, std::min(c->tseal_lat.lat_max, c->chunk)))
    return tseal_lat_run(c, key, rounds, 0, scalars32, n, out_us48, out_cs, ok, msgs, mlen);
  rc = sealr_prepare(c, key, n, c->stream);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  MaskTail mk;
  mk.mlen = mlen;
  mk.host = mk.secret = true;
  return sealr_passes(c, true, rounds, scalars32, n, out_us48, out_cs, ok, c->stream, mk, msgs);
}

int blsv_tlock_encrypt_rounds_dev(blsv_ctx* c, const uint8_t* pk48, const uint64_t* d_rounds, const uint8_t* d_scalars32,
                                  const uint8_t* d_msgs, size_t mlen, size_t n, int kdf, uint8_t* d_out_us48,
                                  uint8_t* d_out_cs, uint8_t* d_ok, void* stream) {
  if (!c) return BLSV_EINVAL;
  if ((n && (!d_rounds || !d_scalars32 || !d_msgs || !d_out_us48 || !d_out_cs || !d_ok)) || ((uintptr_t)d_rounds & 7) ||
      !tcrypt_fits(kdf, mlen, n) || !seal_rounds_fits(n))
    return fail(c, BLSV_EINVAL, "tlock_encrypt_rounds_dev: bad arguments");
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  const uint8_t* key;
  int rc = seal_key(c, pk48, &key);
  if (rc) return rc;
  rc = sealr_prepare(c, key, n, st);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  MaskTail mk;
  mk.mlen = mlen;
  mk.secret = true;
  return sealr_passes(c, false, d_rounds, d_scalars32, n, d_out_us48, d_out_cs, d_ok, st, mk, d_msgs);
}

int blsv_tlock_seal_rounds_stats(blsv_ctx* c, uint64_t* keys, uint64_t* items) {
  if (!c) return BLSV_EINVAL;
  if (keys) *keys = c->tsealr.keys;
  if (items) *items = c->tsealr.items;
  return BLSV_OK;
}

}  // extern "C"
