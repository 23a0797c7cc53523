// The threshold side of the C ABI (include/blsverify.h): the group and its PubPoly.Eval table,
// partial-signature verification, recovery with its speculative form, the aggregation of a round, and
// signing. The host does the reference's control-flow bookkeeping (share selection order, index
// parsing, Lagrange coefficients: hostlogic.h); every verdict and point operation is the device's.
#include <numeric>

#include "host_internal.h"

extern "C" int blsv_set_group(blsv_ctx* c, const uint8_t* commits48, size_t t, size_t n) {
  if (!c || !commits48 || t == 0 || t > 65536) return fail(c, BLSV_EINVAL, "set_group: bad arguments");
  (void)hipSetDevice(c->device);
  // the same group again (every caller sets its key per call): nothing to decode or evaluate
  if (c->has_group && c->t == t && c->n == n && c->group_bytes.size() == t * 48 &&
      memcmp(c->group_bytes.data(), commits48, t * 48) == 0)
    return BLSV_OK;
  c->has_group = false;
  c->group_bytes.clear();
  std::vector<uint8_t> cls;
  int rc = decode_g1(c, commits48, t, c->commits, c->commit_inf, cls);
  if (rc) return rc;
  for (size_t i = 0; i < t; i++)
    if (cls[i]) return fail(c, BLSV_EINVAL, "set_group: commitment %zu rejected (class %d)", i, (int)cls[i]);
  c->pk_all_n = 0;  // the PK_i table of the new group is built by the first partials call
  c->pk_all_built = false;
  c->t = t;
  c->n = n;
  c->group_bytes.assign(commits48, commits48 + t * 48);
  c->has_group = true;
  return BLSV_OK;
}

static std::vector<uint32_t> identity(size_t m) {
  std::vector<uint32_t> v(m);
  std::iota(v.begin(), v.end(), 0u);
  return v;
}

// PubPoly.Eval(d_idx[i]) for cnt indices into (tab, inf)
static void pubpoly_eval(blsv_ctx* c, const uint32_t* d_idx, size_t cnt, DBuf& tab, DBuf& inf) {
  blsk::launch_pubpoly_eval(c->commits.as<uint32_t>(), c->commit_inf.as<uint8_t>(), (uint32_t)c->t, d_idx, cnt,
                            tab.as<uint32_t>(), inf.as<uint8_t>(), c->stream);
}

// PK_i = PubPoly.Eval(i) for every member index below min(n, kPkTable) (key/keys.go:239-241; share
// x = i + 1), built once per group: the partial verifications index this table instead of running
// Horner per partial and call. Lazily, on the group's first partials call, so a set_group that is
// only used for VerifyRecovered never pays the O(t n) G1 work.
static int ensure_pk_table(blsv_ctx* c) {
  if (c->pk_all_built) return BLSV_OK;
  const size_t m = std::min(c->n, kPkTable);
  if (m) {
    const std::vector<uint32_t> ident = identity(m);
    HIPCHK(c, c->idx.ensure(m * 4));
    HIPCHK(c, c->pk_all.ensure(m * blsk::G1_WORDS * 4));
    HIPCHK(c, c->pk_all_inf.ensure(m));
    HIPCHK(c, hipMemcpyAsync(c->idx.p, ident.data(), m * 4, hipMemcpyHostToDevice, c->stream));
    pubpoly_eval(c, c->idx.as<uint32_t>(), m, c->pk_all, c->pk_all_inf);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));  // ident must outlive the copy
  }
  c->pk_all_n = m;
  c->pk_all_built = true;
  return BLSV_OK;
}

// shared by verify_partials / recover / aggregate: the per-partial class in cls and share index in
// index (host), the decoded sigmas staged in S on the device.
// msg_lens == nullptr: every partial signs the same msg[0 .. msg_len); else partial i signs its own
// message, msgs packed back to back with msg_lens[i] bytes each.
static int partials_stage(blsv_ctx* c, const uint8_t* msg, size_t msg_len, const uint8_t* partials,
                          size_t partial_len, size_t k, std::vector<uint8_t>& cls, std::vector<uint32_t>& index,
                          const uint32_t* msg_lens = nullptr) {
  cls.assign(k, BLSV_REJ_OK);
  index.assign(k, 0);
  if (!c->has_group) return fail(c, BLSV_ENOGROUP, "partials: no group set");
  if (k > c->chunk) return fail(c, BLSV_EINVAL, "partials: more than the context chunk (%zu) in one call", c->chunk);
  share_indices(partials, partial_len, k, index);
  if (partial_len != 98) {  // every share has the wrong signature length, or not even an index
    cls.assign(k, partial_len < 2 ? BLSV_REJ_SHARE_INDEX : BLSV_REJ_LENGTH);
    return BLSV_OK;
  }
  int rc = ensure_pk_table(c);
  if (rc) return rc;
  rc = ensure_workspace(c, k);
  if (rc) return rc;
  if (k > c->cap) return fail(c, BLSV_EINVAL, "partials: more than the context chunk (%zu) in one call", c->cap);
  // H(msg) once per item slot (all identical); the per-item PubPoly.Eval(index) table
  std::vector<uint32_t> lens(k, (uint32_t)msg_len);
  std::vector<uint8_t> packed;
  if (msg_lens) {
    rc = upload_messages(c, msg, msg_lens, k);
  } else {
    packed.reserve(k * msg_len);
    for (size_t i = 0; i < k; i++) packed.insert(packed.end(), msg, msg + msg_len);
    rc = upload_messages(c, packed.data(), lens.data(), k);
  }
  if (rc) return rc;
  HIPCHK(c, c->idx.ensure(k * 4));
  HIPCHK(c, h2d(c, c->idx.p, index.data(), k * 4));
  // PubPoly.Eval(index): the per-group table when every index is a member index (< n), else
  // evaluated for this batch (an index >= n still has a well-defined Eval in kyber)
  bool in_table = true;
  for (size_t i = 0; i < k; i++) in_table = in_table && index[i] < c->pk_all_n;
  std::vector<uint32_t> ident;  // a large upload reads it when it runs: alive until the download below
  PkSel pk{c->pk_all.as<uint32_t>(), c->pk_all_inf.as<uint8_t>(), c->idx.as<uint32_t>()};
  if (!in_table) {
    HIPCHK(c, c->pp_tab.ensure(k * blsk::G1_WORDS * 4));
    HIPCHK(c, c->pp_inf.ensure(k));
    HIPCHK(c, c->sel.ensure(k * 4));
    ident = identity(k);
    HIPCHK(c, h2d(c, c->sel.p, ident.data(), k * 4));
    pubpoly_eval(c, c->idx.as<uint32_t>(), k, c->pp_tab, c->pp_inf);
    pk = {c->pp_tab.as<uint32_t>(), c->pp_inf.as<uint8_t>(), c->sel.as<uint32_t>()};
  }
  HIPCHK(c, c->in_sigs.ensure(k * partial_len + 96));
  HIPCHK(c, h2d(c, c->in_sigs.p, partials, k * partial_len));
  const SigSrc sig{c->in_sigs.as<uint8_t>(), partial_len, 2};
  if (use_lat(c, k)) {
    // one workgroup per partial; the decoded sigmas land in S (stride k) for recover_from. Only the
    // class bytes are read back (below), so no bitmap pass
    StageTimer tm(c, ST_LAT, k, c->stream);
    lat_uploaded(c, sig, k, pk, c->cls.as<uint8_t>(), c->S.as<uint32_t>(), c->s_inf.as<uint8_t>(), c->stream);
    HIPCHK(c, hipGetLastError());
  } else {
    // the batch pipeline (one pass: k <= cap): only its class bytes are read back
    PassOut out;
    rc = ctx_outputs(c, k, false, out);
    if (rc) return rc;
    rc = run_passes(
        c, k, sig, pk, [&](size_t base, size_t cnt, hipStream_t st) { hash_uploaded(c, base, cnt, st); }, Tail(), out,
        c->stream);
    if (rc) return rc;
  }
  HIPCHK(c, download_sync(c, {{cls.data(), c->cls.p, k}}));
  return BLSV_OK;
}

// ok[i] / reject_class[i] (optional) of the k partials from position lo of cls
static void put_verdicts(const std::vector<uint8_t>& cls, size_t lo, size_t k, uint8_t* ok, uint8_t* reject_class) {
  for (size_t i = 0; i < k; i++) {
    ok[i] = cls[lo + i] == BLSV_REJ_OK;
    if (reject_class) reject_class[i] = cls[lo + i];
  }
}

// blsv_verify_partials (msg_lens == nullptr) and blsv_verify_partials_multi behind their argument checks
static int verify_partials(blsv_ctx* c, const uint8_t* msg, size_t msg_len, const uint32_t* msg_lens,
                           const uint8_t* partials, size_t partial_len, size_t k, uint8_t* ok, uint8_t* reject_class) {
  (void)hipSetDevice(c->device);
  std::vector<uint8_t> cls;
  std::vector<uint32_t> index;
  const int rc = partials_stage(c, msg, msg_len, partials, partial_len, k, cls, index, msg_lens);
  if (rc) return rc;
  put_verdicts(cls, 0, k, ok, reject_class);
  return BLSV_OK;
}

// Lagrange at 0 over the shares select_shares picks (x = index + 1) of the batch partials_stage just
// decompressed into c->S, then the G2 MSM and compression.
static int recover_from(blsv_ctx* c, const std::vector<uint8_t>& cls, const std::vector<uint32_t>& index, size_t lo,
                        size_t hi, size_t t, size_t n, uint8_t* out_sig96) {
  std::vector<uint32_t> sel, idx;
  if (!select_shares(cls, index, lo, hi, t, n, sel, idx))
    return fail(c, BLSV_ENOTENOUGH, "share: not enough good public shares to reconstruct secret commitment");
  HIPCHK(c, c->sel.ensure(t * 4));
  HIPCHK(c, c->idx.ensure(t * 4));
  HIPCHK(c, c->lambdas.ensure(t * 32));
  HIPCHK(c, c->scratch.ensure(t * 192 * 4));
  HIPCHK(c, c->out.ensure(96));
  HIPCHK(c, h2d(c, c->sel.p, sel.data(), t * 4));
  std::vector<uint32_t> lam(t * 8);
  host_lagrange(idx.data(), t, lam.data());
  HIPCHK(c, h2d(c, c->lambdas.p, lam.data(), t * 32));
  blsk::launch_lat_recover(c->S.as<uint32_t>(), cls.size(), c->s_inf.as<uint8_t>(), c->sel.as<uint32_t>(),
                           c->lambdas.as<uint32_t>(), (uint32_t)t, c->scratch.as<uint32_t>(), c->out.as<uint8_t>(),
                           c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, download_sync(c, {{out_sig96, c->out.p, 96}}));
  return BLSV_OK;
}

// Speculative recovery. A round's partials are all verified before recover_from picks its shares,
// and the recovered signature is verified after: three latency launches in a row. The shares the
// selection would pick if every partial verified are known before any verification, so they are
// decoded (no subgroup check: validity is the partials' verdict), interpolated and compressed on the
// side stream WHILE the partials verify on the main stream. The result is kept when the verdicts
// leave the selection unchanged -- the same shares, hence the same bytes as recover_from -- and
// recomputed by recover_from otherwise (a selected share failed). Only for rounds on the latency
// path, whose partial verification leaves the side stream idle.
struct SpecRecover {
  bool launched = false;
  bool verified = false;      // VerifyRecovered of the speculative signature queued behind it too
  std::vector<uint32_t> sel;  // round positions of the shares used
};

static int spec_recover_launch(blsv_ctx* c, int slot, const uint8_t* partials, size_t partial_len,
                               const std::vector<uint32_t>& index, size_t lo, size_t hi, size_t t, size_t n,
                               SpecRecover& sr, const uint8_t* vmsg = nullptr, size_t vmsg_len = 0) {
  sr.launched = false;
  sr.verified = false;
  std::vector<uint8_t> all_ok(index.size(), BLSV_REJ_OK);
  std::vector<uint32_t> idx;
  if (!select_shares(all_ok, index, lo, hi, t, n, sr.sel, idx)) return BLSV_OK;  // recover_from will say so
  auto& sp = c->spec[slot];
  const size_t tt = sr.sel.size();
  // host staging: sigmas | indices | selection | 96-byte result | verify class | message, offsets,
  // length | Lagrange coefficients
  const size_t v_off = tt * 96 + tt * 8 + 96, m_off = v_off + 64;
  const bool verify = vmsg != nullptr && vmsg_len <= kIoCap / 4;
  const size_t lam_off = (m_off + (verify ? vmsg_len + 64 : 0) + 7) & ~size_t(7);
  const size_t host_need = lam_off + tt * 32 + 64;
  if (sp.host.sz < host_need) {  // no copy may be pending on it
    HIPCHK(c, hipStreamSynchronize(c->side));
    HIPCHK(c, hipStreamSynchronize(c->side2));
  }
  HIPCHK(c, sp.host.ensure(host_need));
  uint8_t* h_sig = sp.host.as<uint8_t>();
  uint32_t* h_idx = reinterpret_cast<uint32_t*>(h_sig + tt * 96);
  uint32_t* h_sel = h_idx + tt;
  uint32_t* h_lam = reinterpret_cast<uint32_t*>(h_sig + lam_off);
  for (size_t j = 0; j < tt; j++) {
    std::memcpy(h_sig + j * 96, partials + (size_t)sr.sel[j] * partial_len + 2, 96);
    h_idx[j] = idx[j];
    h_sel[j] = (uint32_t)j;
  }
  HIPCHK(c, sp.sig.ensure(tt * 96));
  HIPCHK(c, sp.S.ensure(tt * blsk::S_WORDS * 4));
  HIPCHK(c, sp.s_inf.ensure(tt));
  HIPCHK(c, sp.cls.ensure(tt));
  HIPCHK(c, sp.sel.ensure(tt * 4));
  HIPCHK(c, sp.lam.ensure(tt * 32));
  HIPCHK(c, sp.scratch.ensure(tt * 192 * 4));
  HIPCHK(c, sp.out.ensure(96));
  if (verify) {
    // VerifyRecovered's message and key do not depend on the recovery: its hash-to-G2 and the key
    // pair's Miller loop start now, on the second side stream, beside the partial verification and
    // the recovery (wvteam.h team_hash_key)
    uint8_t* h_msg = h_sig + m_off;
    std::memcpy(h_msg, vmsg, vmsg_len);
    uint64_t* h_off = reinterpret_cast<uint64_t*>(h_msg + ((vmsg_len + 7) & ~size_t(7)));
    h_off[0] = 0;
    h_off[1] = vmsg_len;
    uint32_t* h_len = reinterpret_cast<uint32_t*>(h_off + 2);
    h_len[0] = (uint32_t)vmsg_len;
    HIPCHK(c, sp.vmsg.ensure(vmsg_len + 1));
    HIPCHK(c, sp.voff.ensure(16));
    HIPCHK(c, sp.vlen.ensure(4));
    HIPCHK(c, sp.vcls.ensure(64));
    HIPCHK(c, sp.hout.ensure(blsk::kLatHoutWords * 4));
    HIPCHK(c, sp.saff.ensure(blsk::kLatSaffWords * 4));
    if (vmsg_len) HIPCHK(c, hipMemcpyAsync(sp.vmsg.p, h_msg, vmsg_len, hipMemcpyHostToDevice, c->side2));
    HIPCHK(c, hipMemcpyAsync(sp.voff.p, h_off, 16, hipMemcpyHostToDevice, c->side2));
    HIPCHK(c, hipMemcpyAsync(sp.vlen.p, h_len, 4, hipMemcpyHostToDevice, c->side2));
    const PkSel pk = group_pk(c);
    blsk::launch_lat_hash_key(sp.vmsg.as<uint8_t>(), sp.voff.as<uint64_t>(), sp.vlen.as<uint32_t>(), pk.tab, pk.inf,
                              sp.hout.as<uint32_t>(), c->side2);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->hash_ev[slot], c->side2));
  }
  // the shares' decoding first, then the Lagrange coefficients on the host (host_lagrange, ~30 us)
  // while it runs; the interpolation follows on the same stream
  hipStream_t st = c->side;
  HIPCHK(c, hipMemcpyAsync(sp.sig.p, h_sig, tt * 96, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(sp.sel.p, h_sel, tt * 4, hipMemcpyHostToDevice, st));
  blsk::launch_lat_decode(sp.sig.as<uint8_t>(), 96, 0, tt, sp.S.as<uint32_t>(), sp.s_inf.as<uint8_t>(),
                          sp.cls.as<uint8_t>(), st);
  host_lagrange(h_idx, tt, h_lam);
  HIPCHK(c, hipMemcpyAsync(sp.lam.p, h_lam, tt * 32, hipMemcpyHostToDevice, st));
  blsk::launch_lat_recover(sp.S.as<uint32_t>(), tt, sp.s_inf.as<uint8_t>(), sp.sel.as<uint32_t>(),
                           sp.lam.as<uint32_t>(), (uint32_t)tt, sp.scratch.as<uint32_t>(), sp.out.as<uint8_t>(), st,
                           verify ? sp.saff.as<uint32_t>() : nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(h_sig + tt * 96 + tt * 8, sp.out.p, 96, hipMemcpyDeviceToHost, st));
  if (verify) {
    // VerifyRecovered(group key, msg, speculative signature) right behind the recovery: the signature
    // pair of the sum's affine point, the product with the key pair's Miller value computed above and
    // the final exponentiation (wvteam.h verify_team_pre: the class verify_messages would give the
    // compressed bytes; kept on a hit)
    HIPCHK(c, hipStreamWaitEvent(st, c->hash_ev[slot], 0));
    blsk::launch_lat_verify_pre(sp.hout.as<uint32_t>(), sp.saff.as<uint32_t>(), sp.vcls.as<uint8_t>(), st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_sig + v_off, sp.vcls.p, 1, hipMemcpyDeviceToHost, st));
    sr.verified = true;
  }
  sr.launched = true;
  return BLSV_OK;
}

// after the partials' verdicts (cls): the speculative result if its selection stands, else
// recover_from; the side stream is drained either way
static int spec_recover_finish(blsv_ctx* c, int slot, const SpecRecover& sr, const std::vector<uint8_t>& cls,
                               const std::vector<uint32_t>& index, size_t lo, size_t hi, size_t t, size_t n,
                               uint8_t* out_sig96, int* vcls = nullptr) {
  if (vcls) *vcls = -1;  // no speculative VerifyRecovered verdict
  if (sr.launched) {
    HIPCHK(c, hipStreamSynchronize(c->side));
    std::vector<uint32_t> sel, idx;
    if (select_shares(cls, index, lo, hi, t, n, sel, idx) && sel == sr.sel) {
      const size_t tt = sr.sel.size();
      const uint8_t* h = c->spec[slot].host.as<uint8_t>();
      std::memcpy(out_sig96, h + tt * 96 + tt * 8, 96);
      if (vcls && sr.verified) *vcls = h[tt * 96 + tt * 8 + 96];
      c->spec_hits++;
      return BLSV_OK;
    }
    c->spec_misses++;
  }
  return recover_from(c, cls, index, lo, hi, t, n, out_sig96);
}

// Drains both side streams when a call that launched speculative work returns, on every path: an
// early error return must not leave async copies into the slots' pinned staging in flight (the next
// call's spec_recover_launch writes that staging without a synchronisation when it is large enough).
// On the normal path spec_recover_finish has drained `side` already and this costs two idle syncs.
struct SideDrain {
  blsv_ctx* c;
  bool armed = false;
  ~SideDrain() {
    if (!armed) return;
    (void)hipStreamSynchronize(c->side);
    (void)hipStreamSynchronize(c->side2);
  }
};

// partial_len == 98 and the round small enough for the latency path (partials_stage's choice)
static bool spec_applies(const blsv_ctx* c, size_t k, size_t partial_len) {
  return partial_len == 98 && c->has_group && k > 0 && k <= std::min(c->lat_max, c->chunk);
}

extern "C" {

int blsv_verify_partials(blsv_ctx* c, const uint8_t* msg, size_t msg_len, const uint8_t* partials, size_t partial_len,
                         size_t k, uint8_t* ok, uint8_t* reject_class) {
  if (!c) return BLSV_EINVAL;
  if ((k && (!partials || !ok)) || (msg_len && !msg)) return fail(c, BLSV_EINVAL, "verify_partials: null arguments");
  return verify_partials(c, msg, msg_len, nullptr, partials, partial_len, k, ok, reject_class);
}

int blsv_verify_partials_multi(blsv_ctx* c, const uint8_t* msgs, const uint32_t* msg_lens, const uint8_t* partials,
                               size_t partial_len, size_t k, uint8_t* ok, uint8_t* reject_class) {
  if (!c) return BLSV_EINVAL;
  if (k && (!partials || !ok || !msgs || !msg_lens)) return fail(c, BLSV_EINVAL, "verify_partials_multi: null arguments");
  return verify_partials(c, msgs, 0, msg_lens, partials, partial_len, k, ok, reject_class);
}

int blsv_recover(blsv_ctx* c, const uint8_t* msg, size_t msg_len, const uint8_t* partials, size_t partial_len,
                 size_t k, size_t t, size_t n, uint8_t* out_sig96) {
  if (!c) return BLSV_EINVAL;
  if (!out_sig96 || t == 0 || (k && !partials) || (msg_len && !msg)) return fail(c, BLSV_EINVAL, "recover: bad arguments");
  (void)hipSetDevice(c->device);
  std::vector<uint8_t> cls;
  std::vector<uint32_t> index;
  int rc = partials_stage(c, msg, msg_len, partials, partial_len, k, cls, index);
  if (rc) return rc;
  return recover_from(c, cls, index, 0, k, t, n, out_sig96);
}

int blsv_aggregate(blsv_ctx* c, const uint8_t* msg, size_t msg_len, const uint8_t* partials, size_t partial_len,
                   size_t k, size_t t, size_t n, uint8_t* ok, uint8_t* reject_class, uint8_t* out_sig96,
                   uint8_t* group_ok) {
  if (!c) return BLSV_EINVAL;
  if (!out_sig96 || !ok || !group_ok || t == 0 || (k && !partials) || (msg_len && !msg))
    return fail(c, BLSV_EINVAL, "aggregate: bad arguments");
  (void)hipSetDevice(c->device);
  std::vector<uint8_t> cls;
  std::vector<uint32_t> index;
  SpecRecover sr;
  SideDrain drain{c};
  if (spec_applies(c, k, partial_len)) {
    share_indices(partials, partial_len, k, index);
    drain.armed = true;
    int rc0 = spec_recover_launch(c, 0, partials, partial_len, index, 0, k, t, n, sr, msg, msg_len);
    if (rc0) return rc0;
  }
  int rc = partials_stage(c, msg, msg_len, partials, partial_len, k, cls, index);
  if (rc) return rc;
  put_verdicts(cls, 0, k, ok, reject_class);
  *group_ok = 0;
  int vcls = -1;
  rc = spec_recover_finish(c, 0, sr, cls, index, 0, k, t, n, out_sig96, &vcls);
  if (rc) return rc;
  if (vcls >= 0) {  // the speculative VerifyRecovered of this very signature
    *group_ok = vcls == BLSV_REJ_OK;
    return BLSV_OK;
  }
  // VerifyRecovered(group key, msg, sig) (chain/beacon/chain.go:141)
  const uint32_t len = (uint32_t)msg_len;
  uint8_t bm = 0, cls1 = 0;
  uint64_t fb = 0;
  rc = blsv_verify_messages(c, nullptr, msg, &len, 1, out_sig96, &bm, &fb, &cls1);
  if (rc) return rc;
  *group_ok = bm & 1;
  return BLSV_OK;
}

int blsv_aggregate_round(blsv_ctx* c, const uint8_t* msg1, size_t msg1_len, const uint8_t* partials1, size_t k1,
                         const uint8_t* msg2, size_t msg2_len, const uint8_t* partials2, size_t k2,
                         size_t partial_len, size_t t, size_t n, uint8_t* ok1, uint8_t* ok2, uint8_t* sig1_96,
                         uint8_t* sig2_96, int32_t* status, uint8_t* v2_valid) {
  if (!c) return BLSV_EINVAL;
  if (!sig1_96 || !sig2_96 || !status || !v2_valid || t == 0 || (k1 && (!partials1 || !ok1)) ||
      (k2 && (!partials2 || !ok2 || !msg2)) || (msg1_len && !msg1))
    return fail(c, BLSV_EINVAL, "aggregate_round: bad arguments");
  (void)hipSetDevice(c->device);
  *status = BLSV_AGG_V1_RECOVER_FAIL;
  *v2_valid = 0;
  const size_t k = k1 + k2;
  // pass 1: every V1 and V2 partial in ONE verification pass (per-item message)
  std::vector<uint8_t> msgs, parts;
  std::vector<uint32_t> lens(k);
  msgs.reserve(k1 * msg1_len + k2 * msg2_len);
  parts.reserve(k * partial_len);
  for (size_t i = 0; i < k1; i++) {
    msgs.insert(msgs.end(), msg1, msg1 + msg1_len);
    lens[i] = (uint32_t)msg1_len;
  }
  for (size_t i = 0; i < k2; i++) {
    msgs.insert(msgs.end(), msg2, msg2 + msg2_len);
    lens[k1 + i] = (uint32_t)msg2_len;
  }
  if (k1) parts.insert(parts.end(), partials1, partials1 + k1 * partial_len);
  if (k2) parts.insert(parts.end(), partials2, partials2 + k2 * partial_len);
  std::vector<uint8_t> cls;
  std::vector<uint32_t> index;
  const bool try_v2 = k2 >= t;
  SpecRecover sr1, sr2;  // both recoveries speculated on the side stream (see spec_recover_launch)
  SideDrain drain{c};
  if (spec_applies(c, k, partial_len)) {
    share_indices(parts.data(), partial_len, k, index);
    drain.armed = true;
    int rc0 = spec_recover_launch(c, 0, parts.data(), partial_len, index, 0, k1, t, n, sr1, msg1 ? msg1 : parts.data(),
                                  msg1_len);
    if (!rc0 && try_v2)
      rc0 = spec_recover_launch(c, 1, parts.data(), partial_len, index, k1, k, t, n, sr2, msg2, msg2_len);
    if (rc0) return rc0;
  }
  int rc = partials_stage(c, msgs.data(), 0, parts.data(), partial_len, k, cls, index, lens.data());
  if (rc) return rc;
  put_verdicts(cls, 0, k1, ok1, nullptr);
  put_verdicts(cls, k1, k2, ok2, nullptr);
  // Recover V1 (chain.go:136) and, with LenV2 >= thr, V2 (chain.go:153-155) from the staged shares
  int vc1 = -1, vc2 = -1;
  rc = spec_recover_finish(c, 0, sr1, cls, index, 0, k1, t, n, sig1_96, &vc1);
  if (rc == BLSV_ENOTENOUGH) return BLSV_OK;  // "invalid_recovery": no beacon this time (drain syncs sr2)
  if (rc) return rc;
  bool v2_recovered = false;
  if (try_v2) {
    rc = spec_recover_finish(c, 1, sr2, cls, index, k1, k, t, n, sig2_96, &vc2);
    if (rc && rc != BLSV_ENOTENOUGH) return rc;
    v2_recovered = rc == BLSV_OK;
  }
  // pass 2: VerifyRecovered(pub.Commit(), msg, sig) for both group signatures in one pass
  const uint32_t vlens[2] = {(uint32_t)msg1_len, (uint32_t)msg2_len};
  std::vector<uint8_t> vmsg(msg1, msg1 + msg1_len), vsig(sig1_96, sig1_96 + 96);
  if (v2_recovered) {
    vmsg.insert(vmsg.end(), msg2, msg2 + msg2_len);
    vsig.insert(vsig.end(), sig2_96, sig2_96 + 96);
  }
  uint8_t bm = 0, vcls[2] = {0, 0};
  uint64_t fb = 0;
  if (vc1 >= 0 && (!v2_recovered || vc2 >= 0)) {  // both verdicts already computed speculatively
    bm = (uint8_t)((vc1 == BLSV_REJ_OK) | ((v2_recovered && vc2 == BLSV_REJ_OK) << 1));
  } else {
    rc = blsv_verify_messages(c, nullptr, vmsg.data(), vlens, v2_recovered ? 2 : 1, vsig.data(), &bm, &fb, vcls);
    if (rc) return rc;
  }
  if (!(bm & 1)) {
    *status = BLSV_AGG_V1_INVALID;  // chain.go:141-144 "invalid_sig": no beacon
    return BLSV_OK;
  }
  if (try_v2 && !v2_recovered) {
    *status = BLSV_AGG_V2_RECOVER_FAIL;  // chain.go:155-160: never accept a beacon with an invalid v2
    return BLSV_OK;
  }
  *v2_valid = v2_recovered ? (uint8_t)((bm >> 1) & 1) : 0;  // chain.go:162-164: a failure only logs
  *status = v2_recovered ? BLSV_AGG_OK_V2 : BLSV_AGG_OK;
  return BLSV_OK;
}

int blsv_sign(blsv_ctx* c, const uint8_t* sk32, int32_t index, const uint8_t* msgs, const uint32_t* msg_lens, size_t n,
              uint8_t* out) {
  if (!c) return BLSV_EINVAL;
  if (!sk32 || (n && (!msg_lens || !out)) || index > 65535) return fail(c, BLSV_EINVAL, "sign: bad arguments");
  if (n > kMaxChunk) return fail(c, BLSV_EINVAL, "sign: batch larger than %zu", kMaxChunk);
  (void)hipSetDevice(c->device);
  if (!n) return BLSV_OK;
  uint32_t sk[8];
  scalar_mod_r(sk32, sk);
  // a call of a few messages: one workgroup per message (sign_lat.cpp; blsv_set_sign_lat_max, 0 = off)
  if (sign_lat_routes(n, std::min(c->sign_lat.lat_max, c->chunk)))
    return sign_lat_run(c, sk, index, msgs, msg_lens, n, out);
  int rc = ensure_workspace(c, n);
  if (rc) return rc;
  rc = upload_messages(c, msgs, msg_lens, n);
  if (rc) return rc;
  const size_t stride = index >= 0 ? 98 : 96;
  HIPCHK(c, c->sk.ensure(32));
  HIPCHK(c, c->out.ensure(n * stride));
  HIPCHK(c, hipMemcpyAsync(c->sk.p, sk, 32, hipMemcpyHostToDevice, c->stream));
  (void)for_each_pass(c, n, [&](size_t base, size_t cnt) {  // H staging holds one chunk
    hash_uploaded(c, base, cnt, c->stream);
    blsk::launch_sign(c->sk.as<uint32_t>(), index, c->H.as<uint32_t>(), c->h_inf.as<uint8_t>(), cnt,
                      c->out.as<uint8_t>() + base * stride, stride, c->stream);
    return BLSV_OK;
  });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, c->out.p, n * stride, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BLSV_OK;
}

}  // extern "C"
