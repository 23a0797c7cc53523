// Timelock opening: blsv_tlock_open* (include/blsverify.h "timelock", tlock.h). Sigma is prepared once
// and cached, then per pass the U decode, the f pass against sigma's line table, the final
// exponentiation with its capture output and the Gt encoding, all in the pipeline staging
// (engine_ctx.h lists which buffer holds what). It shares the staging with the verification passes
// (verify.cpp) but none of their stages, so it keeps a pass loop of its own.
// Also the latency path of the host forms (blsv_set_tlock_lat_max; tlock_lat_run, used by tlockr.cpp too):
// one workgroup per item in one launch (k_lat_tlock.hip), outside the staging, the cache and the counters.
#include "host_internal.h"

// Decodes and prepares sigma on st unless it is the cached one; its class is read back (the one
// synchronisation of a call, and only on a new sigma).
int tlock_prepare_sig(blsv_ctx* c, const uint8_t* sig96, hipStream_t st, uint8_t* sig_class) {
  tlock_state& t = c->tlock;
  if (!t.valid || memcmp(t.sig, sig96, 96) != 0) {
    t.valid = false;
    HIPCHK(c, t.d_sig.ensure(96));
    HIPCHK(c, t.S.ensure(blsk::S_WORDS * 4));
    HIPCHK(c, t.s_inf.ensure(1));
    HIPCHK(c, t.s_cls.ensure(1));
    HIPCHK(c, t.tab.ensure(blsk::kTlockTabWords * 4));
    HIPCHK(c, hipMemcpyAsync(t.d_sig.p, sig96, 96, hipMemcpyHostToDevice, st));
    {
      StageTimer tm(c, ST_TLOCK, 1, st);
      blsk::launch_decompress_g2(t.d_sig.as<uint8_t>(), 96, 0, 0, 1, t.S.as<uint32_t>(), t.s_inf.as<uint8_t>(),
                                 t.s_cls.as<uint8_t>(), st);
      blsk::launch_tlock_prepare(t.S.as<uint32_t>(), t.s_inf.as<uint8_t>(), t.s_cls.as<uint8_t>(),
                                 t.tab.as<uint32_t>(), st);
    }
    HIPCHK(c, hipGetLastError());
    uint8_t cls = 0xff;
    HIPCHK(c, hipMemcpyAsync(&cls, t.s_cls.p, 1, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(t.sig, sig96, 96);
    t.cls = cls;
    t.valid = true;
    if (cls == BLSV_REJ_OK) t.prepared++;
  }
  if (sig_class) *sig_class = t.cls;
  if (t.cls != BLSV_REJ_OK) return fail(c, BLSV_EINVAL, "tlock_open: signature rejected (class %d)", (int)t.cls);
  return BLSV_OK;
}

// One pass of cnt <= cap items: d_us (cnt x 48 bytes) -> d_out (cnt x 576 bytes), classes in s_inf. With a
// mask tail (mk.mlen != 0; blsv_tlock_decrypt*) the encoding is replaced by the mask kernel over the pass's
// input bytes mk_in: d_out gets cnt x mlen bytes. With an authenticated tail (au.on; blsv_tlock_decrypt_auth*,
// device pointers only) mk_in is the pass's W bytes and the tail also writes BLSV_REJ_TLOCK_AUTH into s_inf.
static int tlock_pass(blsv_ctx* c, const uint8_t* d_us, size_t cnt, uint8_t* d_out, uint8_t* d_cls_out, hipStream_t st,
                      const MaskTail& mk = MaskTail(), const uint8_t* mk_in = nullptr, const AuthTail& au = AuthTail()) {
  const tlock_state& t = c->tlock;
  const Staging w = staging(c);
  uint32_t* U = w.H;
  uint8_t* u_inf = w.h_inf;
  uint8_t* ucls = w.s_inf;
  {
    StageTimer tm(c, ST_DECOMP, cnt, st);
    blsk::launch_decompress_g1(d_us, cnt, U, u_inf, ucls, st);
  }
  // the final exponentiation marks a value other than 1 in the class bytes it is given: it gets a copy
  HIPCHK(c, hipMemcpyAsync(w.cls, ucls, cnt, hipMemcpyDeviceToDevice, st));
  {
    StageTimer tm(c, ST_TLOCK, cnt, st);
    blsk::launch_tlock_f(t.tab.as<uint32_t>(), U, u_inf, ucls, t.s_inf.as<uint8_t>(), cnt, w.F, st);
  }
  {
    StageTimer tm(c, ST_FEXP, cnt, st);
    // the values are captured in HQ, so the park stays in LN (a timelock pass stages no lines)
    blsk::launch_final_exp(w.F, w.FW, cnt, 0, cnt, w.cls, st, w.LN, w.HQ);
  }
  if (au.on) {  // the authenticated tail: the U table is still in H / h_inf
    const int rc = auth_open_tail(c, au, mk, cnt, mk_in, d_out, st);
    if (rc) return rc;
  } else if (mk.mlen) {
    const int rc = mask_tail(c, mk, ucls, BLSV_REJ_OK, cnt, mk_in, d_out, st);
    if (rc) return rc;
  } else {
    blsk::launch_tlock_encode(w.HQ, ucls, cnt, d_out, st);
  }
  if (d_cls_out) HIPCHK(c, hipMemcpyAsync(d_cls_out, ucls, cnt, hipMemcpyDeviceToDevice, st));
  HIPCHK(c, hipGetLastError());
  return BLSV_OK;
}

// Every pass of n items under the prepared sigma. Device buffers (host == false): us, out and cls
// (optional) are read and written in place on st. Host buffers: a pass's compressed U bytes travel in
// S, its encoded values come back through F, and each pass ends with the download's synchronisation.
// With a mask tail, mk_in is the call's n x mlen input bytes and out receives n x mlen bytes; a host call's
// pass stages both in F (mask_tail).
int tlock_passes(blsv_ctx* c, bool host, const uint8_t* us, size_t n, uint8_t* out, uint8_t* cls, hipStream_t st,
                 const MaskTail& mk, const uint8_t* mk_in, const AuthTail& au) {
  int rc = ensure_workspace(c, n);
  if (rc) return rc;
  const size_t out_len = mk.mlen ? mk.mlen : BLSV_GT_LEN;
  for (size_t base = 0; base < n; base += c->cap) {
    const size_t cnt = std::min(c->cap, n - base);
    const uint8_t* pass_us = us + base * BLSV_U_LEN;
    const uint8_t* pass_in = mk.mlen ? mk_in + base * mk.mlen : nullptr;
    uint8_t* pass_out = out + base * out_len;
    if (host) {
      uint8_t* d_out = mask_host_out(c, mk, cnt);
      HIPCHK(c, h2d(c, c->S.p, pass_us, cnt * BLSV_U_LEN));
      rc = tlock_pass(c, c->S.as<uint8_t>(), cnt, d_out, nullptr, st, mk, pass_in);
      if (rc) return rc;
      HIPCHK(c, download_sync(c, {{pass_out, d_out, cnt * out_len}, {cls + base, c->s_inf.p, cnt}}));
    } else {
      rc = tlock_pass(c, pass_us, cnt, pass_out, cls ? cls + base : nullptr, st, mk, pass_in, au.at(base));
      if (rc) return rc;
    }
  }
  c->tlock.items += n;
  return BLSV_OK;
}

// The latency path (blsv_set_tlock_lat_max, k_lat_tlock.hip): one upload of the call's inputs, one launch
// with a workgroup per item and per idle signature, one download of everything it wrote. The results stay
// in the context's host staging (o points into it) for the caller to copy out: blsv_tlock_open hands
// nothing over under a rejected sigma. sig_of == nullptr: every item under signature 0.
int tlock_lat_run(blsv_ctx* c, const uint8_t* sigs96, size_t m, const uint32_t* sig_of, const uint32_t* idle,
                  size_t n_idle, const uint8_t* us48, size_t n, TlockLatOut& o, const uint8_t* cs, size_t mlen) {
  tlock_lat_state& t = c->tlock_lat;
  const TlockLatLayout l = tlock_lat_layout(m, n, sig_of != nullptr, n_idle, n * mlen);
  HIPCHK(c, t.buf.ensure(l.total));
  t.up.resize(l.in_total);
  memcpy(t.up.data() + l.o_sigs, sigs96, 96 * m);
  memcpy(t.up.data() + l.o_us, us48, BLSV_U_LEN * n);
  if (sig_of) memcpy(t.up.data() + l.o_sigof, sig_of, 4 * n);
  if (n_idle) memcpy(t.up.data() + l.o_idle, idle, 4 * n_idle);
  if (mlen) memcpy(t.up.data() + l.o_min, cs, n * mlen);
  uint8_t* d = t.buf.as<uint8_t>();
  HIPCHK(c, h2d(c, d, t.up.data(), l.in_total));
  blsk::launch_lat_tlock(d + l.o_sigs, sig_of ? (const uint32_t*)(d + l.o_sigof) : nullptr, d + l.o_us, n,
                         (const uint32_t*)(d + l.o_idle), n_idle, d + l.o_gt, d + l.o_cls, d + l.o_sigcls, c->stream);
  // decrypting: the mask kernel behind it over the bytes it wrote, and the download starts behind them
  if (mlen) blsk::launch_tmask_encoded(d + l.o_gt, d + l.o_cls, BLSV_REJ_OK, n, d + l.o_min, d + l.o_mout, mlen, c->stream);
  HIPCHK(c, hipGetLastError());
  t.down.resize(l.out_total);
  HIPCHK(c, download_sync(c, {{t.down.data(), d + l.o_down, l.out_total}}));
  o.gt = t.down.data();  // n x 576 bytes, or the n x mlen masked bytes
  o.cls = t.down.data() + (l.o_cls - l.o_down);
  o.sig_cls = o.cls + n;
  t.launches++;
  t.items += n;
  return BLSV_OK;
}

void tlock_lat_copy_out(const TlockLatOut& o, size_t n, uint8_t* out, uint8_t* ok, uint8_t* reject_class, size_t out_len) {
  memcpy(out, o.gt, out_len * n);
  if (reject_class) memcpy(reject_class, o.cls, n);
  for (size_t i = 0; i < n; i++) ok[i] = o.cls[i] == BLSV_REJ_OK;
}

extern "C" {

int blsv_tlock_open(blsv_ctx* c, const uint8_t* sig96, const uint8_t* us48, size_t n, uint8_t* out_gt576, uint8_t* ok,
                    uint8_t* reject_class, uint8_t* sig_class) {
  if (!c) return BLSV_EINVAL;
  if (!sig96 || (n && (!us48 || !out_gt576 || !ok))) return fail(c, BLSV_EINVAL, "tlock_open: bad arguments");
  (void)hipSetDevice(c->device);
  if (tlock_lat_routes(n, 0, std::min(c->tlock_lat.lat_max, c->chunk))) {
    TlockLatOut o;
    const int rl = tlock_lat_run(c, sig96, 1, nullptr, nullptr, 0, us48, n, o);
    if (rl) return rl;
    if (sig_class) *sig_class = o.sig_cls[0];
    if (o.sig_cls[0] != BLSV_REJ_OK)
      return fail(c, BLSV_EINVAL, "tlock_open: signature rejected (class %d)", (int)o.sig_cls[0]);
    tlock_lat_copy_out(o, n, out_gt576, ok, reject_class);
    return BLSV_OK;
  }
  int rc = tlock_prepare_sig(c, sig96, c->stream, sig_class);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  std::vector<uint8_t> own;
  uint8_t* cls = reject_class;
  if (!cls) {
    own.resize(n);
    cls = own.data();
  }
  rc = tlock_passes(c, true, us48, n, out_gt576, cls, c->stream);
  if (rc) return rc;
  for (size_t i = 0; i < n; i++) ok[i] = cls[i] == BLSV_REJ_OK;
  return BLSV_OK;
}

int blsv_tlock_open_dev(blsv_ctx* c, const uint8_t* sig96, const uint8_t* d_us48, size_t n, uint8_t* d_out_gt576,
                        uint8_t* d_reject_class, void* stream) {
  if (!c) return BLSV_EINVAL;
  if (!sig96 || (n && (!d_us48 || !d_out_gt576)) || ((uintptr_t)d_out_gt576 & 3))
    return fail(c, BLSV_EINVAL, "tlock_open_dev: bad arguments");
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  int rc = tlock_prepare_sig(c, sig96, st, nullptr);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  return tlock_passes(c, false, d_us48, n, d_out_gt576, d_reject_class, st);
}

int blsv_tlock_decrypt(blsv_ctx* c, const uint8_t* sig96, const uint8_t* us48, const uint8_t* cs, size_t mlen, size_t n,
                       int kdf, uint8_t* out_msgs, uint8_t* ok, uint8_t* reject_class, uint8_t* sig_class) {
  if (!c) return BLSV_EINVAL;
  if (!sig96 || (n && (!us48 || !cs || !out_msgs || !ok)) || !tcrypt_fits(kdf, mlen, n))
    return fail(c, BLSV_EINVAL, "tlock_decrypt: bad arguments");
  (void)hipSetDevice(c->device);
  if (tlock_lat_routes(n, 0, std::min(c->tlock_lat.lat_max, c->chunk))) {
    TlockLatOut o;
    const int rl = tlock_lat_run(c, sig96, 1, nullptr, nullptr, 0, us48, n, o, cs, mlen);
    if (rl) return rl;
    if (sig_class) *sig_class = o.sig_cls[0];
    if (o.sig_cls[0] != BLSV_REJ_OK)
      return fail(c, BLSV_EINVAL, "tlock_decrypt: signature rejected (class %d)", (int)o.sig_cls[0]);
    tlock_lat_copy_out(o, n, out_msgs, ok, reject_class, mlen);
    return BLSV_OK;
  }
  int rc = tlock_prepare_sig(c, sig96, c->stream, sig_class);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  std::vector<uint8_t> own;
  uint8_t* cls = reject_class;
  if (!cls) {
    own.resize(n);
    cls = own.data();
  }
  MaskTail mk;
  mk.mlen = mlen;
  mk.host = true;
  rc = tlock_passes(c, true, us48, n, out_msgs, cls, c->stream, mk, cs);
  if (rc) return rc;
  for (size_t i = 0; i < n; i++) ok[i] = cls[i] == BLSV_REJ_OK;
  return BLSV_OK;
}

int blsv_tlock_decrypt_dev(blsv_ctx* c, const uint8_t* sig96, const uint8_t* d_us48, const uint8_t* d_cs, size_t mlen,
                           size_t n, int kdf, uint8_t* d_out_msgs, uint8_t* d_reject_class, void* stream) {
  if (!c) return BLSV_EINVAL;
  if (!sig96 || (n && (!d_us48 || !d_cs || !d_out_msgs)) || !tcrypt_fits(kdf, mlen, n))
    return fail(c, BLSV_EINVAL, "tlock_decrypt_dev: bad arguments");
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  int rc = tlock_prepare_sig(c, sig96, st, nullptr);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  MaskTail mk;
  mk.mlen = mlen;
  return tlock_passes(c, false, d_us48, n, d_out_msgs, d_reject_class, st, mk, d_cs);
}

int blsv_tlock_stats(blsv_ctx* c, uint64_t* prepared, uint64_t* items) {
  if (!c) return BLSV_EINVAL;
  if (prepared) *prepared = c->tlock.prepared;
  if (items) *items = c->tlock.items;
  return BLSV_OK;
}

}  // extern "C"
