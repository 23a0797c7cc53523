// Timelock opening across many rounds: blsv_tlock_open_rounds* (include/blsverify.h "timelock", tlockr.h).
// m round signatures, round j owning counts[j] consecutive items. Per pass the host plans the tiles
// (hostlogic.h open_rounds_next_pass), then on the device: the U decode, the decode and preparation of the
// signatures the pass touches into one word-major table, the f pass over the tiles, the final
// exponentiation with its capture output and the opening's Gt encoding, all in the pipeline staging
// (engine_ctx.h lists which buffer holds what). Nothing is cached and no class is read back before the
// end: the opening's sigma cache (tlock.cpp) and the sealing caches are not touched.
#include "host_internal.h"

static_assert(sizeof(TlockTile) == 4 * blsk::kTlockTileWords && kTlockTileMixed == blsk::kTlockTileMixed,
              "the host's tiles are what k_tlockr_f reads");
static_assert(kOpenRoundsFwBytesPerItem <= 4 * 3 * blsk::F_WORDS, "open_rounds_layout does not fit the FW staging");
static_assert(kTlockTileItems == 64, "a tile is one wave");

// a small upload on st: through the pinned staging when st is the context's own stream
static hipError_t up(blsv_ctx* c, hipStream_t st, void* dst, const void* src, size_t len) {
  if (!len) return hipSuccess;
  if (st == c->stream) return h2d(c, dst, src, len);
  return hipMemcpyAsync(dst, src, len, hipMemcpyHostToDevice, st);
}

// The FW staging's part of a pass (open_rounds_layout), typed
struct RoundsFw {
  uint8_t *sig_cls, *sig_inf;
  uint32_t *sig_j, *sig_of, *tiles;
};
static RoundsFw rounds_fw(const blsv_ctx* c) {
  const OpenRoundsLayout l = open_rounds_layout(c->cap);
  uint8_t* fw = c->FW.as<uint8_t>();
  return {fw + l.o_cls, fw + l.o_inf, (uint32_t*)(fw + l.o_sigj), (uint32_t*)(fw + l.o_sigof),
          (uint32_t*)(fw + l.o_tiles)};
}

// Workspace for a call of n items and m signatures, the staging of a pass's compressed signatures, and the
// counter of prepared signatures (cleared when it is created).
static int rounds_begin(blsv_ctx* c, size_t m, size_t n, hipStream_t st) {
  int rc = ensure_workspace(c, std::max(n, size_t(1)));
  if (rc) return rc;
  HIPCHK(c, c->in_sigs.ensure(96 * std::min(std::max(m, size_t(1)), c->cap)));
  if (!c->tlockr.prepared.p) {
    HIPCHK(c, c->tlockr.prepared.ensure(8));
    HIPCHK(c, hipMemsetAsync(c->tlockr.prepared.p, 0, 8, st));
  }
  return BLSV_OK;
}

// The M <= cap signatures sel[0 .. M) of the call into in_sigs, their indices into sig_j, and their decode
// (subgroup check included) into S with the flags in FW; their classes go to d_sig_class (optional) at
// their own indices. tmp: the gathered bytes when the selection is not one contiguous range.
static int rounds_decode(blsv_ctx* c, const uint8_t* sigs96, const std::vector<uint32_t>& sel, size_t from, size_t M,
                         uint8_t* d_sig_class, std::vector<uint8_t>& tmp, hipStream_t st) {
  const Staging w = staging(c);
  const RoundsFw fw = rounds_fw(c);
  const uint32_t* s = sel.data() + from;
  const uint8_t* src = sigs96 + 96 * (size_t)s[0];
  if ((size_t)(s[M - 1] - s[0]) != M - 1) {
    tmp.resize(96 * M);
    for (size_t k = 0; k < M; k++) memcpy(tmp.data() + 96 * k, sigs96 + 96 * (size_t)s[k], 96);
    src = tmp.data();
  }
  HIPCHK(c, up(c, st, c->in_sigs.p, src, 96 * M));
  HIPCHK(c, up(c, st, fw.sig_j, s, 4 * M));
  blsk::launch_decompress_g2(c->in_sigs.as<uint8_t>(), 96, 0, 0, M, w.S, fw.sig_inf, fw.sig_cls, st);
  if (d_sig_class) blsk::launch_tlock_scatter_classes(fw.sig_cls, fw.sig_j, M, d_sig_class, st);
  return BLSV_OK;
}

// One pass: d_us (cnt x 48 bytes) -> d_out (cnt x 576 bytes), the items' classes in s_inf. With a mask tail
// (mk.mlen != 0; blsv_tlock_decrypt_rounds*) the encoding is replaced by the mask kernel over the pass's input
// bytes mk_in: d_out gets cnt x mlen bytes. An authenticated tail (au.on; blsv_tlock_decrypt_auth_rounds*) as in
// tlock.cpp's pass.
static int rounds_pass(blsv_ctx* c, const uint8_t* sigs96, const TlockRoundsPass& p, const uint8_t* d_us, uint8_t* d_out,
                       uint8_t* d_cls_out, uint8_t* d_sig_class, std::vector<uint8_t>& tmp, hipStream_t st,
                       const MaskTail& mk, const uint8_t* mk_in, const AuthTail& au = AuthTail()) {
  const Staging w = staging(c);
  const RoundsFw fw = rounds_fw(c);
  const size_t cnt = p.cnt, M = p.sig_j.size();
  uint32_t* U = w.H;
  uint8_t* u_inf = w.h_inf;
  uint8_t* ucls = w.s_inf;
  {
    StageTimer tm(c, ST_DECOMP, cnt, st);
    blsk::launch_decompress_g1(d_us, cnt, U, u_inf, ucls, st);  // a host call's U bytes leave S here
  }
  // the uniform tiles first, the mixed ones behind them: one launch per form
  std::vector<TlockTile> tiles(p.tiles.size());
  size_t n_uniform = 0;
  for (const TlockTile& t : p.tiles)
    if (t.sig != kTlockTileMixed) tiles[n_uniform++] = t;
  size_t at = n_uniform;
  for (const TlockTile& t : p.tiles)
    if (t.sig == kTlockTileMixed) tiles[at++] = t;
  HIPCHK(c, up(c, st, fw.tiles, tiles.data(), tiles.size() * sizeof(TlockTile)));
  if (at != n_uniform) HIPCHK(c, up(c, st, fw.sig_of, p.sig_of.data(), 4 * cnt));
  {
    StageTimer tm(c, ST_TLOCK, cnt, st);
    int rc = rounds_decode(c, sigs96, p.sig_j, 0, M, d_sig_class, tmp, st);
    if (rc) return rc;
    blsk::launch_tlock_prepare_many(w.S, fw.sig_inf, fw.sig_cls, M, w.LN,
                                    c->tlockr.prepared.as<unsigned long long>(), st);
    blsk::launch_tlock_f_tiles(fw.tiles, n_uniform, at - n_uniform, fw.sig_of, w.LN, M, fw.sig_inf, fw.sig_cls, U, u_inf,
                               ucls, cnt, w.F, st);
  }
  // the final exponentiation marks a value other than 1 in the class bytes it is given: it gets a copy,
  // taken behind the f pass, which has classed the items of rejected signatures
  HIPCHK(c, hipMemcpyAsync(w.cls, ucls, cnt, hipMemcpyDeviceToDevice, st));
  {
    StageTimer tm(c, ST_FEXP, cnt, st);
    // the table is read: the park goes to LN and the values are captured in HQ, as in an opening; FW, the
    // plan in it read too, is the exponentiation's scratch again
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

// Every pass of the call, then the signatures of the rounds without items in batches of their own (only
// their classes are wanted). Device buffers (host == false): us, out and cls (optional) are read and
// written in place on st. Host buffers: a pass's compressed U bytes travel in S, its encoded values come
// back through F, and each pass ends with the download's synchronisation.
// With a mask tail, mk_in is the call's n x mlen input bytes and out receives n x mlen bytes; a host call's
// pass stages both in F (mask_tail).
int rounds_passes(blsv_ctx* c, bool host, const uint8_t* sigs96, const uint64_t* counts, size_t m, const uint8_t* us,
                  size_t n, uint8_t* out, uint8_t* cls, uint8_t* d_sig_class, hipStream_t st, const MaskTail& mk,
                  const uint8_t* mk_in, const AuthTail& au) {
  int rc = rounds_begin(c, m, n, st);
  if (rc) return rc;
  TlockRoundsCursor cur;
  TlockRoundsPass p;
  std::vector<uint8_t> tmp;
  const size_t out_len = mk.mlen ? mk.mlen : BLSV_GT_LEN;
  while (open_rounds_next_pass(counts, m, c->cap, c->tlockr.dense_min, cur, p)) {
    const uint8_t* pass_us = us + p.base * BLSV_U_LEN;
    const uint8_t* pass_in = mk.mlen ? mk_in + p.base * mk.mlen : nullptr;
    uint8_t* pass_out = out + p.base * out_len;
    if (host) {
      uint8_t* d_out = mask_host_out(c, mk, p.cnt);
      HIPCHK(c, h2d(c, c->S.p, pass_us, p.cnt * BLSV_U_LEN));
      rc = rounds_pass(c, sigs96, p, c->S.as<uint8_t>(), d_out, nullptr, d_sig_class, tmp, st, mk, pass_in);
      if (rc) return rc;
      HIPCHK(c, download_sync(c, {{pass_out, d_out, p.cnt * out_len}, {cls + p.base, c->s_inf.p, p.cnt}}));
    } else {
      rc = rounds_pass(c, sigs96, p, pass_us, pass_out, cls ? cls + p.base : nullptr, d_sig_class, tmp, st, mk, pass_in,
                       au.at(p.base));
      if (rc) return rc;
    }
  }
  if (d_sig_class) {
    std::vector<uint32_t> idle;
    for (size_t j = 0; j < m; j++)
      if (!counts[j]) idle.push_back((uint32_t)j);
    for (size_t from = 0; from < idle.size(); from += c->cap) {
      StageTimer tm(c, ST_TLOCK, 0, st);
      rc = rounds_decode(c, sigs96, idle, from, std::min(c->cap, idle.size() - from), d_sig_class, tmp, st);
      if (rc) return rc;
    }
    HIPCHK(c, hipGetLastError());
  }
  c->tlockr.items += n;
  return BLSV_OK;
}

extern "C" {

int blsv_tlock_open_rounds(blsv_ctx* c, const uint8_t* sigs96, const uint64_t* counts, size_t m, const uint8_t* us48,
                           size_t n, uint8_t* out_gt576, uint8_t* ok, uint8_t* reject_class, uint8_t* sig_class) {
  if (!c) return BLSV_EINVAL;
  if ((m && (!sigs96 || !counts)) || (n && (!us48 || !out_gt576 || !ok)) || !open_rounds_fits(counts, m, n))
    return fail(c, BLSV_EINVAL, "tlock_open_rounds: bad arguments");
  (void)hipSetDevice(c->device);
  const size_t lat_max = std::min(c->tlock_lat.lat_max, c->chunk);
  if (tlock_lat_routes(n, 0, lat_max) && tlock_lat_plan(counts, m, lat_max, c->tlock_lat.plan)) {
    const TlockLatPlan& p = c->tlock_lat.plan;
    TlockLatOut o;
    const int rl = tlock_lat_run(c, sigs96, m, p.sig_of.data(), p.idle.data(), p.idle.size(), us48, n, o);
    if (rl) return rl;
    if (sig_class) memcpy(sig_class, o.sig_cls, m);
    tlock_lat_copy_out(o, n, out_gt576, ok, reject_class);
    return BLSV_OK;
  }
  uint8_t* d_sc = nullptr;
  if (sig_class && m) {
    HIPCHK(c, c->misc.ensure(m));
    d_sc = c->misc.as<uint8_t>();
  }
  std::vector<uint8_t> own;
  uint8_t* cls = reject_class;
  if (!cls && n) {
    own.resize(n);
    cls = own.data();
  }
  int rc = rounds_passes(c, true, sigs96, counts, m, us48, n, out_gt576, cls, d_sc, c->stream);
  if (rc) return rc;
  if (d_sc) HIPCHK(c, download_sync(c, {{sig_class, d_sc, m}}));
  for (size_t i = 0; i < n; i++) ok[i] = cls[i] == BLSV_REJ_OK;
  return BLSV_OK;
}

int blsv_tlock_open_rounds_dev(blsv_ctx* c, const uint8_t* sigs96, const uint64_t* counts, size_t m,
                               const uint8_t* d_us48, size_t n, uint8_t* d_out_gt576, uint8_t* d_reject_class,
                               uint8_t* d_sig_class, void* stream) {
  if (!c) return BLSV_EINVAL;
  if ((m && (!sigs96 || !counts)) || (n && (!d_us48 || !d_out_gt576)) || ((uintptr_t)d_out_gt576 & 3) ||
      !open_rounds_fits(counts, m, n))
    return fail(c, BLSV_EINVAL, "tlock_open_rounds_dev: bad arguments");
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  return rounds_passes(c, false, sigs96, counts, m, d_us48, n, d_out_gt576, d_reject_class, d_sig_class, st);
}

int blsv_tlock_decrypt_rounds(blsv_ctx* c, const uint8_t* sigs96, const uint64_t* counts, size_t m, const uint8_t* us48,
                              const uint8_t* cs, size_t mlen, size_t n, int kdf, uint8_t* out_msgs, uint8_t* ok,
                              uint8_t* reject_class, uint8_t* sig_class) {
  if (!c) return BLSV_EINVAL;
  if ((m && (!sigs96 || !counts)) || (n && (!us48 || !cs || !out_msgs || !ok)) || !tcrypt_fits(kdf, mlen, n) ||
      !open_rounds_fits(counts, m, n))
    return fail(c, BLSV_EINVAL, "tlock_decrypt_rounds: bad arguments");
  (void)hipSetDevice(c->device);
  const size_t lat_max = std::min(c->tlock_lat.lat_max, c->chunk);
  if (tlock_lat_routes(n, 0, lat_max) && tlock_lat_plan(counts, m, lat_max, c->tlock_lat.plan)) {
    const TlockLatPlan& p = c->tlock_lat.plan;
    TlockLatOut o;
    const int rl = tlock_lat_run(c, sigs96, m, p.sig_of.data(), p.idle.data(), p.idle.size(), us48, n, o, cs, mlen);
    if (rl) return rl;
    if (sig_class) memcpy(sig_class, o.sig_cls, m);
    tlock_lat_copy_out(o, n, out_msgs, ok, reject_class, mlen);
    return BLSV_OK;
  }
  uint8_t* d_sc = nullptr;
  if (sig_class && m) {
    HIPCHK(c, c->misc.ensure(m));
    d_sc = c->misc.as<uint8_t>();
  }
  std::vector<uint8_t> own;
  uint8_t* cls = reject_class;
  if (!cls && n) {
    own.resize(n);
    cls = own.data();
  }
  MaskTail mk;
  mk.mlen = mlen;
  mk.host = true;
  int rc = rounds_passes(c, true, sigs96, counts, m, us48, n, out_msgs, cls, d_sc, c->stream, mk, cs);
  if (rc) return rc;
  if (d_sc) HIPCHK(c, download_sync(c, {{sig_class, d_sc, m}}));
  for (size_t i = 0; i < n; i++) ok[i] = cls[i] == BLSV_REJ_OK;
  return BLSV_OK;
}

int blsv_tlock_decrypt_rounds_dev(blsv_ctx* c, const uint8_t* sigs96, const uint64_t* counts, size_t m,
                                  const uint8_t* d_us48, const uint8_t* d_cs, size_t mlen, size_t n, int kdf,
                                  uint8_t* d_out_msgs, uint8_t* d_reject_class, uint8_t* d_sig_class, void* stream) {
  if (!c) return BLSV_EINVAL;
  if ((m && (!sigs96 || !counts)) || (n && (!d_us48 || !d_cs || !d_out_msgs)) || !tcrypt_fits(kdf, mlen, n) ||
      !open_rounds_fits(counts, m, n))
    return fail(c, BLSV_EINVAL, "tlock_decrypt_rounds_dev: bad arguments");
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  MaskTail mk;
  mk.mlen = mlen;
  return rounds_passes(c, false, sigs96, counts, m, d_us48, n, d_out_msgs, d_reject_class, d_sig_class, st, mk, d_cs);
}

int blsv_tlock_open_rounds_stats(blsv_ctx* c, uint64_t* prepared, uint64_t* items) {
  if (!c) return BLSV_EINVAL;
  if (prepared) {
    unsigned long long v = 0;
    if (c->tlockr.prepared.p) {
      (void)hipSetDevice(c->device);
      HIPCHK(c, hipMemcpyAsync(&v, c->tlockr.prepared.p, 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    *prepared = v;
  }
  if (items) *items = c->tlockr.items;
  return BLSV_OK;
}

size_t blsv_set_tlock_dense_min(blsv_ctx* c, size_t items) {
  if (!c) return 0;
  const size_t prev = c->tlockr.dense_min;
  c->tlockr.dense_min = items ? items : kTlockDenseMinDefault;
  return prev;
}

}  // extern "C"
