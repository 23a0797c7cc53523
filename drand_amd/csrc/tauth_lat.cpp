// Authenticated timelock on the latency path (blsv_set_tauth_lat_max; include/blsverify.h "authenticated
// timelock"): a host call of a few items of blsv_tlock_decrypt_auth* / blsv_tlock_encrypt_auth*
// (tauth.cpp routes it here after its own argument checks and key handling) runs as ONE upload, ONE launch with
// a workgroup per item (k_lat_tauth_open.hip / k_lat_tauth_seal.hip) and ONE download, through a device buffer
// and host staging of the path's own: outside the pipeline staging, the sigma cache, the (key, round) base
// cache and every other path's counters. T1 is the batch path's table; the encrypting side takes it and the key
// table TK through the one-entry key cache (sealr_prepare), the decrypting side through auth_t1.
#include "host_internal.h"

// The m signatures, item i under sig_of[i] (null: all under signature 0), the n_idle signatures idle[] classed
// alone. The results stay in the path's host staging (o points into it, valid until the next call) for the
// caller to copy out: blsv_tlock_decrypt_auth hands nothing over under a rejected sigma.
int tauth_lat_open_run(blsv_ctx* c, const uint8_t* sigs96, size_t m, const uint32_t* sig_of, const uint32_t* idle,
                       size_t n_idle, const uint8_t* us48, const uint8_t* vs32, const uint8_t* ws, size_t mlen, size_t n,
                       TlockLatOut& o, const uint32_t* mlens, size_t bytes) {
  tauth_lat_state& t = c->tauth_lat;
  TauthLatOpenLayout l;
  if (!(mlens ? tauth_lat_open_layout_var(m, n, sig_of != nullptr, n_idle, bytes, l)
              : tauth_lat_open_layout(m, n, sig_of != nullptr, n_idle, mlen, l)))
    return fail(c, BLSV_EINVAL, "tlock_decrypt_auth: too many items");
  if (!mlens) bytes = mlen * n;
  int rc = auth_t1(c, c->stream);
  if (rc) return rc;
  HIPCHK(c, t.buf.ensure(l.total));
  t.up.resize(l.in_total);
  memcpy(t.up.data() + l.o_sigs, sigs96, 96 * m);
  memcpy(t.up.data() + l.o_us, us48, BLSV_U_LEN * n);
  memcpy(t.up.data() + l.o_vs, vs32, BLSV_V_LEN * n);
  if (sig_of) memcpy(t.up.data() + l.o_sigof, sig_of, 4 * n);
  if (n_idle) memcpy(t.up.data() + l.o_idle, idle, 4 * n_idle);
  if (mlens) {
    bool words;
    (void)tauth_var_offsets(mlens, 0, n, (uint32_t*)(t.up.data() + l.o_offs), &words);  // a word array: o_offs % 4 == 0
  }
  memcpy(t.up.data() + l.o_ws, ws, bytes);
  uint8_t* d = t.buf.as<uint8_t>();
  HIPCHK(c, h2d(c, d, t.up.data(), l.in_total));
  blsk::launch_lat_tauth_open(d + l.o_sigs, sig_of ? (const uint32_t*)(d + l.o_sigof) : nullptr, d + l.o_us, d + l.o_vs,
                              d + l.o_ws, mlen, n, (const uint32_t*)(d + l.o_idle), n_idle, c->tseal.t1.as<uint32_t>(),
                              d + l.o_out, d + l.o_cls, d + l.o_sigcls, t.walk_waves, c->stream,
                              mlens ? (const uint32_t*)(d + l.o_offs) : nullptr);
  HIPCHK(c, hipGetLastError());
  t.down.resize(l.out_total);
  HIPCHK(c, download_sync(c, {{t.down.data(), d + l.o_out, l.out_total}}));
  o.gt = t.down.data();  // the n x mlen message bytes (ragged: the `bytes` packed ones)
  o.cls = t.down.data() + (l.o_cls - l.o_out);
  o.sig_cls = o.cls + n;
  t.open_launches++;
  t.open_items += n;
  return BLSV_OK;
}

// One upload (rounds, seeds, plaintexts), one launch, one download (U, V, W, ok). The staged seeds and
// plaintexts -- on the device and in the host staging -- are cleared behind the kernel before this returns,
// also when the call fails. The derived scalars, k pk and K never leave their workgroups, so there is nothing
// else to clear. No constant-time claim is made (tseal.h).
int tauth_lat_seal_run(blsv_ctx* c, const uint8_t* pk48, const uint64_t* rounds, uint64_t round, const uint8_t* seeds32,
                       const uint8_t* msgs, size_t mlen, size_t n, uint8_t* out_us48, uint8_t* out_vs32, uint8_t* out_ws,
                       uint8_t* ok, const uint32_t* mlens, size_t bytes) {
  tauth_lat_state& t = c->tauth_lat;
  hipStream_t st = c->stream;
  TauthLatSealLayout l;
  if (!(mlens ? tauth_lat_seal_layout_var(n, rounds != nullptr, bytes, l) : tauth_lat_seal_layout(n, rounds != nullptr, mlen, l)))
    return fail(c, BLSV_EINVAL, "tlock_encrypt_auth: too many items");
  if (!mlens) bytes = mlen * n;
  int rc = sealr_prepare(c, pk48, n, st);  // T1 and TK; a rejected key ends the call here
  if (rc) return rc;
  HIPCHK(c, t.buf.ensure(l.total));
  t.up.resize(l.in_total);
  t.down.resize(l.out_total);
  if (rounds) memcpy(t.up.data() + l.o_rounds, rounds, 8 * n);
  memcpy(t.up.data() + l.o_seeds, seeds32, BLSV_SEED_LEN * n);
  if (mlens) {
    bool words;
    (void)tauth_var_offsets(mlens, 0, n, (uint32_t*)(t.up.data() + l.o_offs), &words);  // a word array: o_offs % 4 == 0
  }
  memcpy(t.up.data() + l.o_msgs, msgs, bytes);
  uint8_t* d = t.buf.as<uint8_t>();
  hipError_t e = hipMemcpyAsync(d, t.up.data(), l.in_total, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    blsk::launch_lat_tauth_seal(c->tseal.t1.as<uint32_t>(), c->tsealr.tk.as<uint32_t>(),
                                rounds ? (const uint64_t*)(d + l.o_rounds) : nullptr, round, d + l.o_seeds, d + l.o_msgs, mlen,
                                n, d + l.o_us, d + l.o_vs, d + l.o_ws, d + l.o_ok, st,
                                mlens ? (const uint32_t*)(d + l.o_offs) : nullptr);
    e = hipGetLastError();
  }
  const hipError_t wipe = hipMemsetAsync(d + l.o_seeds, 0, l.in_total - l.o_seeds, st);
  if (e == hipSuccess) e = wipe;
  // the download's synchronisation also ends the upload's reads of the host staging
  const hipError_t down = e != hipSuccess ? hipStreamSynchronize(st) : download_sync(c, {{t.down.data(), d + l.o_us, l.out_total}});
  memset(t.up.data() + l.o_seeds, 0, l.in_total - l.o_seeds);
  if (e == hipSuccess) e = down;
  if (e != hipSuccess) return fail(c, BLSV_EHIP, "tlock_encrypt_auth (latency path): %s", hipGetErrorString(e));
  memcpy(out_us48, t.down.data(), BLSV_U_LEN * n);
  memcpy(out_vs32, t.down.data() + (l.o_vs - l.o_us), BLSV_V_LEN * n);
  memcpy(out_ws, t.down.data() + (l.o_ws - l.o_us), bytes);
  memcpy(ok, t.down.data() + (l.o_ok - l.o_us), n);
  t.seal_launches++;
  t.seal_items += n;
  return BLSV_OK;
}
