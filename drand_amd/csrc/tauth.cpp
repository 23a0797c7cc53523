// Authenticated timelock: blsv_tlock_encrypt_auth* / blsv_tlock_decrypt_auth* (include/blsverify.h
// "authenticated timelock", tauth.h). Each is a thin sibling of its blsv_tlock_encrypt* / blsv_tlock_decrypt*
// mirror: the same preparation and the same passes (tlock.cpp, tlockr.cpp, tseal.cpp, tsealr.cpp) with the
// authenticated tail in place of the mask tail, and on the encrypting side k_tauth_derive in front, which
// turns seeds and messages into the scalars the sealing kernels read. The passes run on device pointers; a
// host form stages a pass of at most cap items in the feature's own buffer (engine_ctx.h has the plan). The
// switches of the unauthenticated latency paths (blsv_set_tlock_lat_max, blsv_set_tseal_lat_max) are not
// consulted; with blsv_set_tauth_lat_max the four host forms hand calls of a few items to the latency path of
// their own (tauth_lat.cpp). The _dev forms always take the batch path.
// The ragged host forms (blsv_tlock_*_auth*_var: a length per item, the bytes packed back to back) share every
// line of this with their uniform counterparts: mlens != nullptr below means ragged, a pass then stages its
// cnt + 1 prefix offsets beside its bytes (hostlogic.h tauth_layout_var) and slices the call's bytes by the
// running byte count instead of base * mlen, and the tails run their ragged kernels (AuthTail::offs).
#include "host_internal.h"

static_assert(BLSV_REJ_TLOCK_AUTH == 10 && BLSV_REJ_TLOCK_AUTH == BLSV_REJ_TLOCK_SIG + 1, "the next free class");
static_assert((unsigned long long)kMaxChunk * BLSV_TLOCK_MSG_MAX < 0xffffffffull, "a pass's prefix offsets are uint32");

// T1, the table of G1's multiples the check walks: the sealing's, built once per context by whoever needs it first
int auth_t1(blsv_ctx* c, hipStream_t st) {
  tseal_state& t = c->tseal;
  HIPCHK(c, t.t1.ensure(blsk::kTsealT1Words * 4));
  if (!t.t1_built) {
    blsk::launch_tseal_g1_table(t.t1.as<uint32_t>(), st);
    HIPCHK(c, hipGetLastError());
    t.t1_built = true;
  }
  return BLSV_OK;
}

int auth_open_tail(blsv_ctx* c, const AuthTail& au, const MaskTail& mk, size_t cnt, const uint8_t* ws, uint8_t* d_out,
                   hipStream_t st) {
  const Staging w = staging(c);
  if (au.offs)
    blsk::launch_tauth_open_tail_var(w.HQ, w.H, w.h_inf, w.s_inf, cnt, c->tseal.t1.as<uint32_t>(), au.vs, au.rag_in, au.offs,
                                     au.rag_words, au.rag_out, st);
  else
    blsk::launch_tauth_open_tail(w.HQ, w.H, w.h_inf, w.s_inf, cnt, c->tseal.t1.as<uint32_t>(), au.vs, ws, mk.mlen, d_out, st);
  return BLSV_OK;
}

int auth_seal_tail(blsv_ctx* c, const AuthTail& au, const MaskTail& mk, const uint8_t* cls, size_t cnt,
                   const uint8_t* msgs, uint8_t* d_out_ws, hipStream_t st) {
  const Staging w = staging(c);
  if (au.offs)
    blsk::launch_tauth_seal_tail_var(w.HQ, cls, cnt, au.seeds, au.rag_in, au.offs, au.rag_words, au.out_vs, au.rag_out, st);
  else
    blsk::launch_tauth_seal_tail(w.HQ, cls, cnt, au.seeds, msgs, mk.mlen, au.out_vs, d_out_ws, st);
  return BLSV_OK;
}

// Every pass of an encrypting call under the prepared base (rounds == nullptr) or key. Device buffers
// (host == false): read and written in place on st, the derived scalars alone staged. Host buffers: a pass's
// inputs go up into the feature's buffer and its outputs come back from there, and each pass ends with the
// download's synchronisation. Either way what is secret in the buffer is cleared behind the kernels, also
// when the pass failed; the pass itself clears the captured K (and k_i pk across rounds).
// mlens (a host form only): the ragged form, mlen is then not read.
static int encrypt_passes(blsv_ctx* c, bool host, const uint64_t* rounds, const uint8_t* seeds, const uint8_t* msgs,
                          size_t mlen, const uint32_t* mlens, size_t n, uint8_t* us, uint8_t* vs, uint8_t* ws, uint8_t* ok,
                          hipStream_t st) {
  int rc = ensure_workspace(c, n);
  if (rc) return rc;
  MaskTail mk;
  mk.mlen = mlens ? 1 : mlen;
  mk.secret = true;
  std::vector<uint32_t>& offs = c->tauth.offs;
  size_t at = 0;  // the call's bytes before this pass
  for (size_t base = 0; base < n; base += c->cap) {
    const size_t cnt = std::min(c->cap, n - base);
    bool words = false;
    size_t bytes = cnt * mlen;
    if (mlens) {
      offs.resize(cnt + 1);
      bytes = tauth_var_offsets(mlens, base, cnt, offs.data(), &words);
    }
    const TauthLayout l = mlens ? tauth_layout_var(cnt, bytes) : tauth_layout(cnt, mlen);
    HIPCHK(c, c->tauth.buf.ensure(host ? l.total : l.o_in));
    uint8_t* B = c->tauth.buf.as<uint8_t>();
    const uint8_t *d_seeds = seeds + base * BLSV_SEED_LEN, *d_msgs = msgs + at;
    const uint64_t* d_rounds = rounds ? rounds + base : nullptr;
    uint8_t *d_us = us + base * BLSV_U_LEN, *d_vs = vs + base * BLSV_V_LEN, *d_ws = ws + at, *d_ok = ok + base;
    uint8_t* const pass_ws = d_ws;  // the caller's
    const uint32_t* d_offs = (const uint32_t*)(B + l.o_offs);
    hipError_t up = hipSuccess;
    if (host) {
      // seeds and plaintexts straight from the caller's memory: the pinned staging of the small uploads would
      // keep a copy of them
      up = hipMemcpyAsync(B + l.o_seeds, d_seeds, cnt * BLSV_SEED_LEN, hipMemcpyHostToDevice, st);
      if (up == hipSuccess) up = hipMemcpyAsync(B + l.o_in, d_msgs, bytes, hipMemcpyHostToDevice, st);
      if (up == hipSuccess && rounds) up = hipMemcpyAsync(B + l.o_rounds, d_rounds, cnt * 8, hipMemcpyHostToDevice, st);
      if (up == hipSuccess && mlens) up = hipMemcpyAsync(B + l.o_offs, offs.data(), 4 * (cnt + 1), hipMemcpyHostToDevice, st);
      d_seeds = B + l.o_seeds;
      d_msgs = B + l.o_in;
      d_rounds = (const uint64_t*)(B + l.o_rounds);
      d_us = B + l.o_us;
      d_vs = B + l.o_vs;
      d_ws = B + l.o_out;
      d_ok = B + l.o_flag;
    }
    if (up != hipSuccess) {
      rc = fail(c, BLSV_EHIP, "tlock_encrypt_auth: upload: %s", hipGetErrorString(up));
    } else {
      uint8_t* d_k = B + l.o_scalars;
      if (mlens)
        blsk::launch_tauth_derive_var(d_seeds, d_msgs, cnt, d_offs, words, d_k, st);
      else
        blsk::launch_tauth_derive(d_seeds, d_msgs, cnt, mlen, d_k, st);
      AuthTail au;
      au.on = true;
      au.seeds = d_seeds;
      au.out_vs = d_vs;
      if (mlens) {
        au.offs = d_offs;
        au.rag_in = d_msgs;
        au.rag_out = d_ws;
        au.rag_words = words;
      }
      rc = rounds ? sealr_passes(c, false, d_rounds, d_k, cnt, d_us, d_ws, d_ok, st, mk, d_msgs, au)
                  : seal_passes(c, false, d_k, cnt, d_us, d_ws, d_ok, st, mk, d_msgs, au);
    }
    const hipError_t wipe = host ? hipMemsetAsync(B, 0, l.secret, st)
                                 : hipMemsetAsync(B + l.o_scalars, 0, cnt * BLSV_SCALAR_LEN, st);
    if (rc) return rc;
    HIPCHK(c, wipe);
    if (host)
      HIPCHK(c, download_sync(c, {{us + base * BLSV_U_LEN, d_us, cnt * BLSV_U_LEN},
                                  {vs + base * BLSV_V_LEN, d_vs, cnt * BLSV_V_LEN},
                                  {pass_ws, d_ws, bytes},
                                  {ok + base, d_ok, cnt}}));
    at += bytes;
  }
  return BLSV_OK;
}

static int encrypt_auth(blsv_ctx* c, const char* what, bool host, const uint8_t* pk48, bool many, const uint64_t* rounds,
                        uint64_t round, const uint8_t* seeds, const uint8_t* msgs, size_t mlen, size_t n, int kdf,
                        uint8_t* us, uint8_t* vs, uint8_t* ws, uint8_t* ok, void* stream, bool var = false,
                        const uint32_t* mlens = nullptr) {
  if (!c) return BLSV_EINVAL;
  size_t bytes = 0;
  if (!n) mlens = nullptr;  // a ragged call without items: nothing left that a length could shape
  if ((n && ((many && !rounds) || !seeds || !msgs || !us || !vs || !ws || !ok)) ||
      !(var ? tauth_var_fits(kdf, mlens, n, &bytes) : tauth_fits(kdf, mlen, n)) ||
      (many && (!seal_rounds_fits(n) || (!host && ((uintptr_t)rounds & 7)))))
    return fail(c, BLSV_EINVAL, "%s: bad arguments", what);
  (void)hipSetDevice(c->device);
  hipStream_t st = !host && stream ? (hipStream_t)stream : c->stream;
  const uint8_t* key;
  int rc = seal_key(c, pk48, &key);
  if (rc) return rc;
  if (host && tauth_lat_routes(n, std::min(c->tauth_lat.seal_max, c->chunk)))
    return tauth_lat_seal_run(c, key, many ? rounds : nullptr, round, seeds, msgs, mlen, n, us, vs, ws, ok, mlens, bytes);
  rc = many ? sealr_prepare(c, key, n, st) : seal_prepare(c, key, round, n, st);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  return encrypt_passes(c, host, many ? rounds : nullptr, seeds, msgs, mlen, mlens, n, us, vs, ws, ok, st);
}

// One pass-sized part of a decrypting host call: [base, base + cnt) of the call's items up into the feature's
// buffer, the device passes over it (run(l, B, mk, au)), and the messages and classes back down. mlens: the
// ragged form (mlen is then not read); at: the call's bytes before this part, moved past it.
static AuthTail open_tail_of(const uint8_t* d_vs) {
  AuthTail au;
  au.on = true;
  au.vs = d_vs;
  return au;
}

template <typename Run>
static int decrypt_host_part(blsv_ctx* c, const uint8_t* us, const uint8_t* vs, const uint8_t* ws, size_t mlen,
                             const uint32_t* mlens, size_t base, size_t cnt, size_t& at, uint8_t* out_msgs, uint8_t* cls,
                             Run run) {
  std::vector<uint32_t>& offs = c->tauth.offs;
  bool words = false;
  size_t bytes = cnt * mlen;
  if (mlens) {
    offs.resize(cnt + 1);
    bytes = tauth_var_offsets(mlens, base, cnt, offs.data(), &words);
  }
  const TauthLayout l = mlens ? tauth_layout_var(cnt, bytes) : tauth_layout(cnt, mlen);
  HIPCHK(c, c->tauth.buf.ensure(l.total));
  uint8_t* B = c->tauth.buf.as<uint8_t>();
  HIPCHK(c, h2d(c, B + l.o_us, us + base * BLSV_U_LEN, cnt * BLSV_U_LEN));
  HIPCHK(c, h2d(c, B + l.o_vs, vs + base * BLSV_V_LEN, cnt * BLSV_V_LEN));
  HIPCHK(c, h2d(c, B + l.o_in, ws + at, bytes));
  MaskTail mk;
  mk.mlen = mlens ? 1 : mlen;
  AuthTail au = open_tail_of(B + l.o_vs);
  if (mlens) {
    HIPCHK(c, h2d(c, B + l.o_offs, offs.data(), 4 * (cnt + 1)));
    au.offs = (const uint32_t*)(B + l.o_offs);
    au.rag_in = B + l.o_in;
    au.rag_out = B + l.o_out;
    au.rag_words = words;
  }
  const int rc = run(l, B, mk, au);
  if (rc) return rc;
  HIPCHK(c, download_sync(c, {{out_msgs + at, B + l.o_out, bytes}, {cls + base, B + l.o_flag, cnt}}));
  at += bytes;
  return BLSV_OK;
}

extern "C" {

int blsv_tlock_encrypt_auth(blsv_ctx* c, const uint8_t* pk48, uint64_t round, const uint8_t* seeds32, const uint8_t* msgs,
                            size_t mlen, size_t n, int kdf, uint8_t* out_us48, uint8_t* out_vs32, uint8_t* out_ws,
                            uint8_t* ok) {
  return encrypt_auth(c, "tlock_encrypt_auth", true, pk48, false, nullptr, round, seeds32, msgs, mlen, n, kdf, out_us48,
                      out_vs32, out_ws, ok, nullptr);
}

int blsv_tlock_encrypt_auth_dev(blsv_ctx* c, const uint8_t* pk48, uint64_t round, const uint8_t* d_seeds32,
                                const uint8_t* d_msgs, size_t mlen, size_t n, int kdf, uint8_t* d_out_us48,
                                uint8_t* d_out_vs32, uint8_t* d_out_ws, uint8_t* d_ok, void* stream) {
  return encrypt_auth(c, "tlock_encrypt_auth_dev", false, pk48, false, nullptr, round, d_seeds32, d_msgs, mlen, n, kdf,
                      d_out_us48, d_out_vs32, d_out_ws, d_ok, stream);
}

int blsv_tlock_encrypt_auth_rounds(blsv_ctx* c, const uint8_t* pk48, const uint64_t* rounds, const uint8_t* seeds32,
                                   const uint8_t* msgs, size_t mlen, size_t n, int kdf, uint8_t* out_us48,
                                   uint8_t* out_vs32, uint8_t* out_ws, uint8_t* ok) {
  return encrypt_auth(c, "tlock_encrypt_auth_rounds", true, pk48, true, rounds, 0, seeds32, msgs, mlen, n, kdf, out_us48,
                      out_vs32, out_ws, ok, nullptr);
}

int blsv_tlock_encrypt_auth_rounds_dev(blsv_ctx* c, const uint8_t* pk48, const uint64_t* d_rounds, const uint8_t* d_seeds32,
                                       const uint8_t* d_msgs, size_t mlen, size_t n, int kdf, uint8_t* d_out_us48,
                                       uint8_t* d_out_vs32, uint8_t* d_out_ws, uint8_t* d_ok, void* stream) {
  return encrypt_auth(c, "tlock_encrypt_auth_rounds_dev", false, pk48, true, d_rounds, 0, d_seeds32, d_msgs, mlen, n, kdf,
                      d_out_us48, d_out_vs32, d_out_ws, d_ok, stream);
}

// blsv_tlock_decrypt_auth and, with var, blsv_tlock_decrypt_auth_var (mlens in mlen's place)
static int decrypt_auth(blsv_ctx* c, const char* what, const uint8_t* sig96, const uint8_t* us48, const uint8_t* vs32,
                        const uint8_t* ws, size_t mlen, bool var, const uint32_t* mlens, size_t n, int kdf, uint8_t* out_msgs,
                        uint8_t* ok, uint8_t* reject_class, uint8_t* sig_class) {
  if (!c) return BLSV_EINVAL;
  size_t bytes = 0;
  if (!n) mlens = nullptr;
  if (!sig96 || (n && (!us48 || !vs32 || !ws || !out_msgs || !ok)) ||
      !(var ? tauth_var_fits(kdf, mlens, n, &bytes) : tauth_fits(kdf, mlen, n)))
    return fail(c, BLSV_EINVAL, "%s: bad arguments", what);
  (void)hipSetDevice(c->device);
  hipStream_t st = c->stream;
  if (tauth_lat_routes(n, std::min(c->tauth_lat.open_max, c->chunk))) {
    TlockLatOut o;
    const int rl = tauth_lat_open_run(c, sig96, 1, nullptr, nullptr, 0, us48, vs32, ws, mlen, n, o, mlens, bytes);
    if (rl) return rl;
    if (sig_class) *sig_class = o.sig_cls[0];
    if (o.sig_cls[0] != BLSV_REJ_OK)
      return fail(c, BLSV_EINVAL, "%s: signature rejected (class %d)", what, (int)o.sig_cls[0]);
    tlock_lat_copy_out(o, n, out_msgs, ok, reject_class, mlens ? 0 : mlen);
    if (mlens) memcpy(out_msgs, o.gt, bytes);
    return BLSV_OK;
  }
  int rc = tlock_prepare_sig(c, sig96, st, sig_class);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  if ((rc = auth_t1(c, st)) || (rc = ensure_workspace(c, n))) return rc;
  std::vector<uint8_t> own;
  uint8_t* cls = reject_class;
  if (!cls) {
    own.resize(n);
    cls = own.data();
  }
  size_t at = 0;
  for (size_t base = 0; base < n; base += c->cap) {
    const size_t cnt = std::min(c->cap, n - base);
    rc = decrypt_host_part(c, us48, vs32, ws, mlen, mlens, base, cnt, at, out_msgs, cls,
                           [&](const TauthLayout& l, uint8_t* B, const MaskTail& mk, const AuthTail& au) {
                             return tlock_passes(c, false, B + l.o_us, cnt, B + l.o_out, B + l.o_flag, st, mk, B + l.o_in, au);
                           });
    if (rc) return rc;
  }
  for (size_t i = 0; i < n; i++) ok[i] = cls[i] == BLSV_REJ_OK;
  return BLSV_OK;
}

int blsv_tlock_decrypt_auth_dev(blsv_ctx* c, const uint8_t* sig96, const uint8_t* d_us48, const uint8_t* d_vs32,
                                const uint8_t* d_ws, size_t mlen, size_t n, int kdf, uint8_t* d_out_msgs,
                                uint8_t* d_reject_class, void* stream) {
  if (!c) return BLSV_EINVAL;
  if (!sig96 || (n && (!d_us48 || !d_vs32 || !d_ws || !d_out_msgs || !d_reject_class)) || !tauth_fits(kdf, mlen, n))
    return fail(c, BLSV_EINVAL, "tlock_decrypt_auth_dev: bad arguments");
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  int rc = tlock_prepare_sig(c, sig96, st, nullptr);
  if (rc) return rc;
  if (!n) return BLSV_OK;
  if ((rc = auth_t1(c, st))) return rc;
  MaskTail mk;
  mk.mlen = mlen;
  return tlock_passes(c, false, d_us48, n, d_out_msgs, d_reject_class, st, mk, d_ws, open_tail_of(d_vs32));
}

// blsv_tlock_decrypt_auth_rounds and, with var, blsv_tlock_decrypt_auth_rounds_var (mlens in mlen's place)
static int decrypt_auth_rounds(blsv_ctx* c, const char* what, const uint8_t* sigs96, const uint64_t* counts, size_t m,
                               const uint8_t* us48, const uint8_t* vs32, const uint8_t* ws, size_t mlen, bool var,
                               const uint32_t* mlens, size_t n, int kdf, uint8_t* out_msgs, uint8_t* ok, uint8_t* reject_class,
                               uint8_t* sig_class) {
  if (!c) return BLSV_EINVAL;
  size_t bytes = 0;
  if (!n) mlens = nullptr;
  if ((m && (!sigs96 || !counts)) || (n && (!us48 || !vs32 || !ws || !out_msgs || !ok)) ||
      !(var ? tauth_var_fits(kdf, mlens, n, &bytes) : tauth_fits(kdf, mlen, n)) || !open_rounds_fits(counts, m, n))
    return fail(c, BLSV_EINVAL, "%s: bad arguments", what);
  (void)hipSetDevice(c->device);
  hipStream_t st = c->stream;
  int rc;
  const size_t lat_max = std::min(c->tauth_lat.open_max, c->chunk);
  if (tauth_lat_routes(n, lat_max) && tlock_lat_plan(counts, m, lat_max, c->tauth_lat.plan)) {
    const TlockLatPlan& p = c->tauth_lat.plan;
    TlockLatOut o;
    rc = tauth_lat_open_run(c, sigs96, m, p.sig_of.data(), p.idle.data(), p.idle.size(), us48, vs32, ws, mlen, n, o, mlens,
                            bytes);
    if (rc) return rc;
    if (sig_class) memcpy(sig_class, o.sig_cls, m);
    tlock_lat_copy_out(o, n, out_msgs, ok, reject_class, mlens ? 0 : mlen);
    if (mlens) memcpy(out_msgs, o.gt, bytes);
    return BLSV_OK;
  }
  if ((rc = auth_t1(c, st)) || (rc = ensure_workspace(c, std::max(n, size_t(1))))) return rc;
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
  // A part is at most cap items: the signatures [j0, j) with the items of theirs that fall into it (a run cut
  // by the boundary appears in both parts, as it does in two passes of blsv_tlock_decrypt_rounds); a round
  // without items goes with the part that reaches it.
  size_t j = 0, used = 0, base = 0, at = 0;
  std::vector<uint64_t> part;
  do {
    const size_t cnt = std::min(c->cap, n - base);
    const size_t j0 = j;
    size_t left = cnt;
    part.clear();
    while (j < m && (left || counts[j] == used)) {
      const size_t take = (size_t)std::min<uint64_t>(left, counts[j] - used);
      part.push_back(take);
      left -= take;
      used += take;
      if (used != counts[j]) break;
      j++;
      used = 0;
    }
    const size_t pm = part.size();
    auto run = [&](const uint8_t* d_us, const uint8_t* d_ws, uint8_t* d_out, uint8_t* d_cls, const MaskTail& mk,
                   const AuthTail& au) {
      return rounds_passes(c, false, sigs96 + 96 * j0, part.data(), pm, d_us, cnt, d_out, d_cls, d_sc ? d_sc + j0 : nullptr,
                           st, mk, d_ws, au);
    };
    if (cnt) {
      rc = decrypt_host_part(c, us48, vs32, ws, mlen, mlens, base, cnt, at, out_msgs, cls,
                             [&](const TauthLayout& l, uint8_t* B, const MaskTail& mk, const AuthTail& au) {
                               return run(B + l.o_us, B + l.o_in, B + l.o_out, B + l.o_flag, mk, au);
                             });
    } else {  // signatures without items: no tail runs
      MaskTail mk;
      mk.mlen = 1;
      rc = pm ? run(nullptr, nullptr, nullptr, nullptr, mk, open_tail_of(nullptr)) : BLSV_OK;
    }
    if (rc) return rc;
    base += cnt;
  } while (base < n || j < m);
  if (d_sc) HIPCHK(c, download_sync(c, {{sig_class, d_sc, m}}));
  for (size_t i = 0; i < n; i++) ok[i] = cls[i] == BLSV_REJ_OK;
  return BLSV_OK;
}

int blsv_tlock_decrypt_auth(blsv_ctx* c, const uint8_t* sig96, const uint8_t* us48, const uint8_t* vs32, const uint8_t* ws,
                            size_t mlen, size_t n, int kdf, uint8_t* out_msgs, uint8_t* ok, uint8_t* reject_class,
                            uint8_t* sig_class) {
  return decrypt_auth(c, "tlock_decrypt_auth", sig96, us48, vs32, ws, mlen, false, nullptr, n, kdf, out_msgs, ok, reject_class,
                      sig_class);
}

int blsv_tlock_decrypt_auth_rounds(blsv_ctx* c, const uint8_t* sigs96, const uint64_t* counts, size_t m, const uint8_t* us48,
                                   const uint8_t* vs32, const uint8_t* ws, size_t mlen, size_t n, int kdf, uint8_t* out_msgs,
                                   uint8_t* ok, uint8_t* reject_class, uint8_t* sig_class) {
  return decrypt_auth_rounds(c, "tlock_decrypt_auth_rounds", sigs96, counts, m, us48, vs32, ws, mlen, false, nullptr, n, kdf,
                             out_msgs, ok, reject_class, sig_class);
}

// ---- the ragged forms: mlens[i] bytes for item i, packed back to back (host forms only)
int blsv_tlock_encrypt_auth_var(blsv_ctx* c, const uint8_t* pk48, uint64_t round, const uint8_t* seeds32, const uint8_t* msgs,
                                const uint32_t* mlens, size_t n, int kdf, uint8_t* out_us48, uint8_t* out_vs32,
                                uint8_t* out_ws, uint8_t* ok) {
  return encrypt_auth(c, "tlock_encrypt_auth_var", true, pk48, false, nullptr, round, seeds32, msgs, 1, n, kdf, out_us48,
                      out_vs32, out_ws, ok, nullptr, true, mlens);
}

int blsv_tlock_encrypt_auth_rounds_var(blsv_ctx* c, const uint8_t* pk48, const uint64_t* rounds, const uint8_t* seeds32,
                                       const uint8_t* msgs, const uint32_t* mlens, size_t n, int kdf, uint8_t* out_us48,
                                       uint8_t* out_vs32, uint8_t* out_ws, uint8_t* ok) {
  return encrypt_auth(c, "tlock_encrypt_auth_rounds_var", true, pk48, true, rounds, 0, seeds32, msgs, 1, n, kdf, out_us48,
                      out_vs32, out_ws, ok, nullptr, true, mlens);
}

int blsv_tlock_decrypt_auth_var(blsv_ctx* c, const uint8_t* sig96, const uint8_t* us48, const uint8_t* vs32,
                                const uint8_t* ws, const uint32_t* mlens, size_t n, int kdf, uint8_t* out_msgs, uint8_t* ok,
                                uint8_t* reject_class, uint8_t* sig_class) {
  return decrypt_auth(c, "tlock_decrypt_auth_var", sig96, us48, vs32, ws, 1, true, mlens, n, kdf, out_msgs, ok, reject_class,
                      sig_class);
}

int blsv_tlock_decrypt_auth_rounds_var(blsv_ctx* c, const uint8_t* sigs96, const uint64_t* counts, size_t m,
                                       const uint8_t* us48, const uint8_t* vs32, const uint8_t* ws, const uint32_t* mlens,
                                       size_t n, int kdf, uint8_t* out_msgs, uint8_t* ok, uint8_t* reject_class,
                                       uint8_t* sig_class) {
  return decrypt_auth_rounds(c, "tlock_decrypt_auth_rounds_var", sigs96, counts, m, us48, vs32, ws, 1, true, mlens, n, kdf,
                             out_msgs, ok, reject_class, sig_class);
}

int blsv_tlock_decrypt_auth_rounds_dev(blsv_ctx* c, const uint8_t* sigs96, const uint64_t* counts, size_t m,
                                       const uint8_t* d_us48, const uint8_t* d_vs32, const uint8_t* d_ws, size_t mlen,
                                       size_t n, int kdf, uint8_t* d_out_msgs, uint8_t* d_reject_class, uint8_t* d_sig_class,
                                       void* stream) {
  if (!c) return BLSV_EINVAL;
  if ((m && (!sigs96 || !counts)) || (n && (!d_us48 || !d_vs32 || !d_ws || !d_out_msgs || !d_reject_class)) ||
      !tauth_fits(kdf, mlen, n) || !open_rounds_fits(counts, m, n))
    return fail(c, BLSV_EINVAL, "tlock_decrypt_auth_rounds_dev: bad arguments");
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  int rc;
  if ((rc = auth_t1(c, st))) return rc;
  MaskTail mk;
  mk.mlen = mlen;
  return rounds_passes(c, false, sigs96, counts, m, d_us48, n, d_out_msgs, d_reject_class, d_sig_class, st, mk, d_ws,
                       open_tail_of(d_vs32));
}

}  // extern "C"
