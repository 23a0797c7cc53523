// Verification: the one pass loop of the batch pipeline with its two tails (exact, randomized), the
// host driver, and the verify entry points of the C ABI (include/blsverify.h) built on them, the
// service's mixed batch and the chain generator. Every verdict is computed by the device kernels
// (kernels.h); this file only moves bytes and sequences launches.
#include <sys/random.h>

#include <thread>

#include "host_internal.h"

// Stage 1 (hash-to-G2, `hash` launches it on st) and stage 2 (decompression) side by side: the
// decompression goes to the side stream after everything already queued on st (the previous chunk
// reads S and cls), and st waits for it before the Miller stage. The two stages fill each other's
// wave-round tails, and a small batch pays max(hash, decompress) instead of the sum.
// BLSV_SERIAL_STAGES=1 in the environment runs the two on the launch stream one after the other
// (profiling: per-kernel durations without the overlap).
static bool serial_stages() {
  static const bool on = [] {
    const char* e = getenv("BLSV_SERIAL_STAGES");
    return e && e[0] == '1';
  }();
  return on;
}

// Stage 2. With a tail that closes the psi subgroup check on its Miller lines pass's own [|x|]sigma
// (k_miller.hip) the head only decodes. The explicit subgroup kernels stay for the randomized tail and
// under blsv_test_generic_chains (the hook exists to exercise them).
static void head_decompress(blsv_ctx* c, const SigSrc& sig, size_t base, size_t cnt, const Tail& tail, hipStream_t st) {
  const Staging w = staging(c);
  if (tail.fused_subgroup() && !blsk::g_generic_chains_all)
    blsk::launch_decompress_g2_only(sig.d, sig.stride, sig.offset, base, cnt, w.S, w.s_inf, w.cls, st);
  else
    blsk::launch_decompress_g2(sig.d, sig.stride, sig.offset, base, cnt, w.S, w.s_inf, w.cls, st);
}

int run_head(blsv_ctx* c, const SigSrc& sig, size_t base, size_t cnt, const Tail& tail, hipStream_t st,
             const HashFn& hash) {
  if (serial_stages()) {
    {
      StageTimer tm(c, ST_DECOMP, cnt, st);
      head_decompress(c, sig, base, cnt, tail, st);
    }
    StageTimer tm(c, ST_HASH, cnt, st);
    hash(base, cnt, st);
    return BLSV_OK;
  }
  HIPCHK(c, hipEventRecord(c->fork_ev, st));
  HIPCHK(c, hipStreamWaitEvent(c->side, c->fork_ev, 0));
  {
    StageTimer tm(c, ST_DECOMP, cnt, c->side);
    head_decompress(c, sig, base, cnt, tail, c->side);
  }
  HIPCHK(c, hipEventRecord(c->join_ev, c->side));
  {
    StageTimer tm(c, ST_HASH, cnt, st);
    hash(base, cnt, st);
  }
  HIPCHK(c, hipStreamWaitEvent(st, c->join_ev, 0));
  return BLSV_OK;
}

// Drains the side stream when a split pass returns before the launch stream has joined it (an error
// between the fork and the join): nothing of the pass may still run when the caller sees the error.
struct SplitDrain {
  blsv_ctx* c;
  bool armed = false;
  ~SplitDrain() {
    if (armed) (void)hipStreamSynchronize(c->side);
  }
};

// Miller + final exponentiation of cnt staged items into their class bytes (F, FW, LN, HQ are the pass's).
// The single-lane f pass runs one wave per SIMD, so a pass of r = cnt / tail_q rounds keeps only the
// fraction r - floor(r) of the GPU busy for the whole of its last round. A pass with such a partial
// last round (hostlogic.h tail_split_main) is split after the lines pass: the launch stream runs the f
// pass and the final exponentiation of the whole rounds [0, main), the side stream (idle since the
// head) the single-lane f pass and the final exponentiation of [main, cnt) once f(main) is done, so the
// remainder's waves share the GPU with the main range's final exponentiation instead of running alone.
// The stages are element-wise; engine_ctx.h says which columns and park areas each range owns. The
// launch stream joins the side stream before it returns to the caller's finish. BLSV_SERIAL_STAGES=1
// keeps every pass whole, like the head.
// One profile record per stage and pass either way; a split pass's records carry both spans.
static int pairing_check(blsv_ctx* c, const PkSel& pk, const uint32_t* H, const uint8_t* h_inf, const uint32_t* S,
                         const uint8_t* s_inf, uint8_t* cls, size_t cnt, bool check_subgroup, hipStream_t st) {
  const Staging w = staging(c);
  const size_t mn = serial_stages() || cnt > kLineSub ? cnt : tail_split_main(cnt, c->tail_q);
  if (mn == cnt) {
    {
      StageTimer tm(c, ST_MILLER, cnt, st);
      blsk::launch_miller(pk.tab, pk.inf, pk.idx, H, h_inf, S, s_inf, cls, cnt, w.F, w.LN, std::min(cnt, kLineSub),
                          w.FW, check_subgroup, st);
    }
    StageTimer tm(c, ST_FEXP, cnt, st);
    final_exp(c, cnt, cls, st);
    return BLSV_OK;
  }
  auto mark = [&](hipStream_t s) {
    hipEvent_t e = c->prof ? take_event(c) : nullptr;
    if (e) (void)hipEventRecord(e, s);
    return e;
  };
  auto keep = [&](ProfRec r) {
    if (!c->prof) return;
    if (!r.a2 || !r.b2) {
      for (hipEvent_t e : {r.a2, r.b2})
        if (e) c->event_pool.push_back(e);
      r.a2 = r.b2 = nullptr;
    }
    if (r.a && r.b) {
      c->recs.push_back(r);
    } else {
      for (hipEvent_t e : {r.a, r.b, r.a2, r.b2})
        if (e) c->event_pool.push_back(e);
    }
  };
  ProfRec rm{ST_MILLER, cnt, nullptr, nullptr}, rf{ST_FEXP, cnt, nullptr, nullptr};
  SplitDrain drain{c};
  const size_t rem = cnt - mn;  // [0, mn) main range, [mn, cnt) remainder
  rm.a = mark(st);
  blsk::launch_miller_lines(pk.tab, pk.inf, pk.idx, H, h_inf, S, s_inf, cls, cnt, 0, cnt, w.LN, cnt, check_subgroup, st);
  blsk::launch_miller_f(w.LN, cnt, cls, cnt, 0, mn, w.F, w.FW, false, st);
  rm.b = mark(st);
  int rc = BLSV_OK;
  auto chk = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && rc == BLSV_OK) rc = fail(c, BLSV_EHIP, "%s: %s", what, hipGetErrorString(e));
    return e == hipSuccess;
  };
  if (chk(hipEventRecord(c->fork_ev, st), "split fork") && chk(hipStreamWaitEvent(c->side, c->fork_ev, 0), "split fork")) {
    drain.armed = true;
    rm.a2 = mark(c->side);
    blsk::launch_miller_f(w.LN, cnt, cls, cnt, mn, rem, w.F, nullptr, true, c->side);
    rm.b2 = mark(c->side);
    rf.a2 = mark(c->side);
    final_exp(c, cnt, mn, rem, cls, c->side);
    rf.b2 = mark(c->side);
    rf.a = mark(st);
    final_exp(c, cnt, 0, mn, cls, st);
    rf.b = mark(st);
    if (chk(hipEventRecord(c->join_ev, c->side), "split join") && chk(hipStreamWaitEvent(st, c->join_ev, 0), "split join"))
      drain.armed = false;
  }
  keep(rm);
  keep(rf);
  return rc;
}

// the last stage of either tail: the pass's class bytes into the call's outputs
static int finish_pass(blsv_ctx* c, size_t base, size_t cnt, const PassOut& out, hipStream_t st) {
  {
    StageTimer tm(c, ST_FINISH, cnt, st);
    blsk::launch_finish(c->cls.as<uint8_t>(), base, cnt, out.bitmap, out.first_bad, out.label0, st);
  }
  if (out.cls) HIPCHK(c, hipMemcpyAsync(out.cls + base, c->cls.p, cnt, hipMemcpyDeviceToDevice, st));
  HIPCHK(c, hipGetLastError());
  return BLSV_OK;
}

// Stages 3..5 (Miller, final exponentiation, finish) of the exact tail: the Miller lines pass rejects
// the signatures outside G2 (REJ_NOT_IN_SUBGROUP; lanes the decoding already rejected return early)
static int run_tail(blsv_ctx* c, size_t base, size_t cnt, const PkSel& pk, const PassOut& out, hipStream_t st) {
  const Staging w = staging(c);
  const int rc = pairing_check(c, pk, w.H, w.h_inf, w.S, w.s_inf, w.cls, cnt, true, st);
  return rc ? rc : finish_pass(c, base, cnt, out, st);
}

// ---------------------------------------------------------------- randomized batch verification
// blsv_verify_*_rlc (include/blsverify.h, rlc.h): per pass the head as usual, then the combination
// stage, one pairing check per group with the existing Miller and final-exponentiation stages, and the
// exact stages again on the items of every group whose check failed.

// the call's seed as eight big-endian words: fresh from the OS CSPRNG unless a test pinned one
int rlc_draw_seed(blsv_ctx* c, uint32_t (&w)[8]) {
  uint8_t s[32];
  if (c->rlc.seed_pinned) {
    memcpy(s, c->rlc.seed, 32);
  } else {
    size_t got = 0;
    while (got < sizeof s) {
      const ssize_t r = getrandom(s + got, sizeof s - got, 0);
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) return fail(c, BLSV_EHIP, "rlc: getrandom failed: %s", strerror(errno));
      got += (size_t)r;
    }
  }
  for (int k = 0; k < 8; k++)
    w[k] = ((uint32_t)s[4 * k] << 24) | ((uint32_t)s[4 * k + 1] << 16) | ((uint32_t)s[4 * k + 2] << 8) | s[4 * k + 3];
  return BLSV_OK;
}

static size_t round64(size_t v) { return (std::max(v, size_t(1)) + 63) & ~size_t(63); }

// the combination stage of one pass into the group staging (ng slots)
int rlc_sums(blsv_ctx* c, size_t base, size_t cnt, const uint32_t (&seed)[8], hipStream_t st) {
  rlc_state& r = c->rlc;
  const Staging w = staging(c);
  const size_t ng = blsk::rlc_groups(cnt, r.group), cap = round64(ng);
  HIPCHK(c, r.part.ensure(2 * blsk::kRlcPartWords * blsk::rlc_lanes(cnt) * 4));
  HIPCHK(c, r.gH.ensure(cap * blsk::H_WORDS * 4));
  HIPCHK(c, r.gS.ensure(cap * blsk::S_WORDS * 4));
  HIPCHK(c, r.g_hinf.ensure(cap));
  HIPCHK(c, r.g_sinf.ensure(cap));
  HIPCHK(c, r.gcls.ensure(cap));
  StageTimer tm(c, ST_RLC, cnt, st);
  blsk::launch_rlc_sums(w.H, w.h_inf, w.S, w.s_inf, w.cls, cnt, base, seed, r.group, r.part.as<uint32_t>(),
                        r.gH.as<uint32_t>(), r.g_hinf.as<uint8_t>(), r.gS.as<uint32_t>(), r.g_sinf.as<uint8_t>(), st);
  return BLSV_OK;
}

// Stages 3..5 of one pass on the randomized path, with the group key (nothing of the pass is in F, FW
// or LN at this point, and neither check exceeds the pass). Synchronises st once: the group verdicts
// decide what the exact stages run on.
static int run_tail_rlc(blsv_ctx* c, size_t base, size_t cnt, const uint32_t (&seed)[8], const PassOut& out,
                        hipStream_t st) {
  rlc_state& r = c->rlc;
  const Staging w = staging(c);
  const PkSel pk = group_pk(c);
  const size_t G = r.group, ng = blsk::rlc_groups(cnt, G);
  int rc = rlc_sums(c, base, cnt, seed, st);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(r.gcls.p, 0, ng, st));
  // (group sums and failing items are far below one f-pass round: the split rule leaves them whole)
  rc = pairing_check(c, pk, r.gH.as<uint32_t>(), r.g_hinf.as<uint8_t>(), r.gS.as<uint32_t>(), r.g_sinf.as<uint8_t>(),
                     r.gcls.as<uint8_t>(), ng, false, st);
  if (rc) return rc;
  HIPCHK(c, hipGetLastError());
  // sized once for the largest pass and the smallest group: never reallocated under a copy in flight
  HIPCHK(c, r.host.ensure(kMaxChunk / kRlcGroupMin * 5 + 16));
  uint8_t* verdict = r.host.as<uint8_t>();
  HIPCHK(c, hipMemcpyAsync(verdict, r.gcls.p, ng, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  uint32_t* fail_list = reinterpret_cast<uint32_t*>(verdict + ((ng + 7) & ~size_t(7)));
  size_t nf = 0;
  for (size_t g = 0; g < ng; g++)
    if (verdict[g] != BLSV_REJ_OK) fail_list[nf++] = (uint32_t)g;
  r.groups += ng;
  r.groups_failed += nf;
  if (nf) {
    const size_t m = rlc_failing_items(cnt, G, fail_list, nf), cap = round64(m);
    r.items_exact += m;
    HIPCHK(c, r.fail.ensure(nf * 4));
    HIPCHK(c, r.cH.ensure(cap * blsk::H_WORDS * 4));
    HIPCHK(c, r.cS.ensure(cap * blsk::S_WORDS * 4));
    HIPCHK(c, r.c_hinf.ensure(cap));
    HIPCHK(c, r.c_sinf.ensure(cap));
    HIPCHK(c, r.ccls.ensure(cap));
    HIPCHK(c, hipMemcpyAsync(r.fail.p, fail_list, nf * 4, hipMemcpyHostToDevice, st));
    {
      StageTimer tm(c, ST_RLC, m, st);
      blsk::launch_rlc_gather(r.fail.as<uint32_t>(), G, m, w.H, w.h_inf, w.S, w.s_inf, w.cls, cnt, r.cH.as<uint32_t>(),
                              r.c_hinf.as<uint8_t>(), r.cS.as<uint32_t>(), r.c_sinf.as<uint8_t>(), r.ccls.as<uint8_t>(),
                              st);
    }
    rc = pairing_check(c, pk, r.cH.as<uint32_t>(), r.c_hinf.as<uint8_t>(), r.cS.as<uint32_t>(), r.c_sinf.as<uint8_t>(),
                       r.ccls.as<uint8_t>(), m, false, st);
    if (rc) return rc;
    StageTimer tm(c, ST_RLC, m, st);
    blsk::launch_rlc_scatter(r.fail.as<uint32_t>(), G, m, r.ccls.as<uint8_t>(), w.cls, cnt, st);
  }
  // (the next pass writes r.host's list of failing groups only after its own synchronisation of st,
  // which this pass's upload of the list precedes)
  return finish_pass(c, base, cnt, out, st);
}

// ---------------------------------------------------------------- the pass loop
int run_passes(blsv_ctx* c, size_t n, const SigSrc& sig, const PkSel& pk, const HashFn& hash, const Tail& tail,
               const PassOut& out, hipStream_t st) {
  return for_each_pass(c, n, [&](size_t base, size_t cnt) {
    // the Miller stage indexes pk.idx by the pass-local item: hand it this pass's slice of the per-item
    // key entries (a batch spans several passes once it exceeds the chunk, or an OOM halving shrank it)
    const PkSel pass_pk{pk.tab, pk.inf, pk.idx ? pk.idx + base : nullptr};
    const int rc = run_head(c, sig, base, cnt, tail, st, hash);
    if (rc) return rc;
    return tail.randomized ? run_tail_rlc(c, base, cnt, tail.seed, out, st) : run_tail(c, base, cnt, pass_pk, out, st);
  });
}

int ctx_outputs(blsv_ctx* c, size_t n, bool with_cls, PassOut& out) {
  HIPCHK(c, c->bitmap.ensure((n + 63) / 64 * 8 + 8));
  HIPCHK(c, c->first_bad.ensure(8));
  HIPCHK(c, hipMemsetAsync(c->first_bad.p, 0xff, 8, c->stream));
  if (with_cls) HIPCHK(c, c->misc.ensure(n + 64));
  out = {c->bitmap.as<uint64_t>(), c->first_bad.as<unsigned long long>(), with_cls ? c->misc.as<uint8_t>() : nullptr, 0};
  return BLSV_OK;
}

// launches the latency kernel of a whole batch writing its class bytes
using LatFn = std::function<void(uint8_t* cls)>;

// The host driver: signatures already on the device, verdicts to the caller's buffers (all optional).
// A batch small enough runs on the latency path through `lat`; else the passes with the exact tail, or
// the randomized one when `randomized`. *first_bad gets the label of the first rejected item i
// (rounds[i] when given, else first_round + i) or UINT64_MAX.
static int verify_host(blsv_ctx* c, size_t n, const SigSrc& sig, const PkSel& pk, const HashFn& hash, const LatFn& lat,
                       bool randomized, uint64_t first_round, const uint64_t* rounds, uint8_t* ok_bitmap,
                       uint64_t* first_bad, uint8_t* reject_class) {
  auto put_first_bad = [&](uint64_t fb) {
    if (first_bad) *first_bad = fb == UINT64_MAX ? fb : rounds ? rounds[fb] : first_round + fb;
  };
  int rc = ensure_workspace(c, n);
  if (rc) return rc;
  if (use_lat(c, n)) {
    // the kernel's class bytes come back in one copy and the bitmap and first bad index are read
    // off them here (launch_finish's rule): no finish kernel, memset or further copies on a call
    // whose every operation is latency
    {
      StageTimer tm(c, ST_LAT, n, c->stream);
      lat(c->cls.as<uint8_t>());
    }
    HIPCHK(c, hipGetLastError());
    std::vector<uint8_t> own;
    uint8_t* cls = reject_class;
    if (!cls) {
      own.resize(n);
      cls = own.data();
    }
    HIPCHK(c, download_sync(c, {{cls, c->cls.p, n}}));
    put_first_bad(fold_classes(cls, n, ok_bitmap));
    return BLSV_OK;
  }
  Tail tail;
  tail.randomized = randomized;
  if (randomized && (rc = rlc_draw_seed(c, tail.seed))) return rc;
  PassOut out;
  rc = ctx_outputs(c, n, reject_class != nullptr, out);
  if (rc) return rc;
  rc = run_passes(c, n, sig, pk, hash, tail, out, c->stream);
  if (rc) return rc;
  const size_t words = (n + 63) / 64;
  std::vector<uint64_t> w(words + 1, 0);
  uint64_t fb = UINT64_MAX;
  HIPCHK(c, download_sync(c, {{w.data(), c->bitmap.p, words * 8},
                              {&fb, c->first_bad.p, 8},
                              {reject_class, c->misc.p, reject_class ? n : 0}}));
  if (ok_bitmap) bitmap_words_to_bytes(w.data(), n, ok_bitmap);
  put_first_bad(fb);
  return BLSV_OK;
}

int decode_g1(blsv_ctx* c, const uint8_t* pk48, size_t cnt, DBuf& tab, DBuf& inf, std::vector<uint8_t>& cls) {
  HIPCHK(c, tab.ensure(cnt * blsk::G1_WORDS * 4));
  HIPCHK(c, inf.ensure(cnt));
  HIPCHK(c, c->g1_cls.ensure(cnt));
  HIPCHK(c, c->misc.ensure(cnt * 48));
  HIPCHK(c, hipMemcpyAsync(c->misc.p, pk48, cnt * 48, hipMemcpyHostToDevice, c->stream));
  blsk::launch_decompress_g1(c->misc.as<uint8_t>(), cnt, tab.as<uint32_t>(), inf.as<uint8_t>(),
                             c->g1_cls.as<uint8_t>(), c->stream);
  HIPCHK(c, hipGetLastError());
  cls.assign(cnt, 0);
  HIPCHK(c, hipMemcpyAsync(cls.data(), c->g1_cls.p, cnt, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BLSV_OK;
}

int upload_messages(blsv_ctx* c, const uint8_t* msgs, const uint32_t* msg_lens, size_t n) {
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + msg_lens[i];
  if (off[n] && !msgs) return fail(c, BLSV_EINVAL, "messages: %llu message bytes but no buffer",
                                   (unsigned long long)off[n]);
  HIPCHK(c, c->in_msgs.ensure(off[n] + 1));
  HIPCHK(c, c->in_off.ensure((n + 1) * 8));
  HIPCHK(c, c->in_len.ensure(n * 4 + 4));
  const size_t staged_max = kIoCap / 4;
  HIPCHK(c, h2d(c, c->in_msgs.p, msgs, off[n]));
  HIPCHK(c, h2d(c, c->in_off.p, off.data(), (n + 1) * 8));
  HIPCHK(c, h2d(c, c->in_len.p, msg_lens, n * 4));
  // a pageable copy of the offsets reads them when it runs: keep the vector alive until then
  if ((n + 1) * 8 > staged_max) HIPCHK(c, hipStreamSynchronize(c->stream));
  return BLSV_OK;
}

int svc_verify_mixed(blsv_ctx* c, size_t n, const uint8_t* msgs, const uint64_t* off, const uint32_t* lens,
                     const uint8_t* sigs96, const uint32_t* idx, const uint32_t* d_tab, const uint8_t* d_tab_inf,
                     uint8_t* cls_out) {
  if (!n) return BLSV_OK;
  if (n > kMaxChunk) return fail(c, BLSV_EINVAL, "service batch larger than %zu", kMaxChunk);
  (void)hipSetDevice(c->device);
  int rc = ensure_workspace(c, std::min(n, c->chunk));
  if (rc) return rc;
  const size_t mbytes = off[n];
  const SvcLayout l = svc_layout(n, mbytes);
  HIPCHK(c, c->pin.ensure(std::max(l.total, n + 8)));
  uint8_t* h = c->pin.as<uint8_t>();
  memcpy(h, off, (n + 1) * 8);
  memcpy(h + l.o_len, lens, n * 4);
  memcpy(h + l.o_idx, idx, n * 4);
  memcpy(h + l.o_sig, sigs96, n * 96);
  if (mbytes) memcpy(h + l.o_msg, msgs, mbytes);
  HIPCHK(c, c->arena.ensure(l.total));
  HIPCHK(c, c->misc.ensure(n + 64));
  HIPCHK(c, hipMemcpyAsync(c->arena.p, h, l.total, hipMemcpyHostToDevice, c->stream));
  uint8_t* d = c->arena.as<uint8_t>();
  const uint64_t* d_off = reinterpret_cast<const uint64_t*>(d);
  const uint32_t* d_len = reinterpret_cast<const uint32_t*>(d + l.o_len);
  const uint8_t* d_msg = d + l.o_msg;
  const SigSrc sig{d + l.o_sig, 96, 0};
  const PkSel pk{d_tab, d_tab_inf, reinterpret_cast<const uint32_t*>(d + l.o_idx)};
  if (use_lat(c, n)) {
    blsk::launch_lat_messages(d_msg, d_off, d_len, sig.d, 96, 0, n, pk.tab, pk.inf, pk.idx, c->misc.as<uint8_t>(),
                              nullptr, nullptr, c->stream);
  } else {
    PassOut out;
    rc = ctx_outputs(c, n, true, out);
    if (rc) return rc;
    rc = run_passes(
        c, n, sig, pk,
        [&](size_t base, size_t cnt, hipStream_t st) { hash_messages(c, d_msg, d_off, d_len, base, cnt, st); }, Tail(),
        out, c->stream);
    if (rc) return rc;
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(h, c->misc.p, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(cls_out, h, n);
  return BLSV_OK;
}

int stage_chain(blsv_ctx* c, uint64_t first_round, const uint8_t* prevs, size_t prev0_len, bool prev_rows,
                const uint8_t* sigs96, size_t n, blsk::ChainedSrc& src) {
  HIPCHK(c, c->in_sigs.ensure(n * 96 + 96));
  HIPCHK(c, c->seeds.ensure(prev_rows ? n * 96 + 96 : 96));
  if (n) {
    HIPCHK(c, h2d(c, c->in_sigs.p, sigs96, n * 96));
    HIPCHK(c, h2d(c, c->seeds.p, prevs, prev_rows ? n * 96 : prev0_len));
  }
  src = {c->in_sigs.as<uint8_t>(), c->seeds.as<uint8_t>(), first_round, prev_rows ? 1 : std::max<uint64_t>(n, 1),
         (uint32_t)prev0_len};
  return BLSV_OK;
}

// ---------------------------------------------------------------- chained beacons, host buffers
// blsv_verify_chained and blsv_verify_prevs (stage_chain's two forms), each exact or randomized.
// `name` prefixes the error texts.
static int chained_host(blsv_ctx* c, const char* name, bool prev_rows, bool randomized, uint64_t first_round,
                        const uint8_t* prevs, size_t prev0_len, const uint8_t* sigs96, size_t n, uint8_t* ok_bitmap,
                        uint64_t* first_bad, uint8_t* reject_class) {
  if (!c->has_group) return fail(c, BLSV_ENOGROUP, "%s: no group key set", name);
  if (n && (!sigs96 || !prevs || (prev0_len != 32 && prev0_len != 96)))
    return fail(c, BLSV_EINVAL, "%s: %s must be 32 or 96 bytes", name, prev_rows ? "row 0's prev" : "prev0");
  if (n > SIZE_MAX / 96 - 1) return fail(c, BLSV_EINVAL, "%s: %zu rounds overflow the byte count", name, n);
  (void)hipSetDevice(c->device);
  blsk::ChainedSrc src;
  const int rc = stage_chain(c, first_round, prevs, prev0_len, prev_rows, sigs96, n, src);
  if (rc) return rc;
  const PkSel pk = group_pk(c);
  return verify_host(
      c, n, {src.sigs, 96, 0}, pk, [&](size_t base, size_t cnt, hipStream_t st) { hash_chained(c, src, base, cnt, st); },
      [&](uint8_t* cls) { blsk::launch_lat_chained(src, 0, n, pk.tab, pk.inf, cls, c->stream); }, randomized,
      first_round, nullptr, ok_bitmap, first_bad, reject_class);
}

// ---------------------------------------------------------------- unchained beacons, host buffers
static int unchained_host(blsv_ctx* c, const char* name, bool randomized, const uint64_t* rounds, uint64_t first_round,
                          const uint8_t* sigs96, size_t n, uint8_t* ok_bitmap, uint64_t* first_bad,
                          uint8_t* reject_class) {
  if (!c->has_group) return fail(c, BLSV_ENOGROUP, "%s: no group key set", name);
  if (n && !sigs96) return fail(c, BLSV_EINVAL, "%s: null signatures", name);
  (void)hipSetDevice(c->device);
  HIPCHK(c, c->in_sigs.ensure(n * 96 + 96));
  if (n) HIPCHK(c, h2d(c, c->in_sigs.p, sigs96, n * 96));
  const uint64_t* d_rounds = nullptr;
  if (rounds && n) {
    HIPCHK(c, c->in_rounds.ensure(n * 8));
    HIPCHK(c, h2d(c, c->in_rounds.p, rounds, n * 8));
    d_rounds = c->in_rounds.as<uint64_t>();
  }
  const PkSel pk = group_pk(c);
  const SigSrc sig{c->in_sigs.as<uint8_t>(), 96, 0};
  return verify_host(
      c, n, sig, pk,
      [&](size_t base, size_t cnt, hipStream_t st) {
        const Staging w = staging(c);
        blsk::launch_hash_unchained(d_rounds, first_round, base, cnt, w.H, w.h_inf, w.HQ, st);
      },
      [&](uint8_t* cls) { blsk::launch_lat_unchained(d_rounds, first_round, sig.d, 0, n, pk.tab, pk.inf, cls, c->stream); },
      randomized, first_round, rounds, ok_bitmap, first_bad, reject_class);
}

// ---------------------------------------------------------------- chained beacons, device buffers
// latency path of a whole device batch (n <= lat_max): the kernel writes the classes, then the
// verdicts go through launch_finish as the pipeline's do
static int run_lat(blsv_ctx* c, size_t n, const LatFn& lat, const PassOut& out, hipStream_t st) {
  {
    StageTimer tm(c, ST_LAT, n, st);
    lat(c->cls.as<uint8_t>());
  }
  blsk::launch_finish(c->cls.as<uint8_t>(), 0, n, out.bitmap, out.first_bad, out.label0, st);
  if (out.cls) HIPCHK(c, hipMemcpyAsync(out.cls, c->cls.p, n, hipMemcpyDeviceToDevice, st));
  HIPCHK(c, hipGetLastError());
  return BLSV_OK;
}

static int chained_dev(blsv_ctx* c, const char* name, bool randomized, uint64_t first_round, uint64_t seg_len,
                       uint64_t seg_phase, const uint8_t* d_seeds96, size_t seed0_len, const uint8_t* d_sigs96, size_t n,
                       uint64_t* d_bitmap, uint64_t* d_first_bad, uint8_t* d_reject_class, void* stream) {
  if (!c->has_group) return fail(c, BLSV_ENOGROUP, "%s: no group key set", name);
  if (n && (!d_seeds96 || !d_sigs96 || !d_bitmap || !d_first_bad || (seed0_len != 32 && seed0_len != 96)))
    return fail(c, BLSV_EINVAL, "%s: bad arguments", name);
  if (seg_phase && (!seg_len || seg_phase >= seg_len))
    return fail(c, BLSV_EINVAL, "%s: seg_phase must be < seg_len", name);
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  Tail tail;
  tail.randomized = randomized;
  int rc = randomized ? rlc_draw_seed(c, tail.seed) : BLSV_OK;
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(d_first_bad, 0xff, 8, st));
  rc = ensure_workspace(c, n);
  if (rc) return rc;
  const blsk::ChainedSrc src{d_sigs96,           d_seeds96, first_round, seg_len ? seg_len : std::max<uint64_t>(n, 1),
                             (uint32_t)seed0_len, seg_phase};
  const PkSel pk = group_pk(c);
  // d_first_bad holds a ROUND (include/blsverify.h): label0 = first_round
  const PassOut out{d_bitmap, (unsigned long long*)d_first_bad, d_reject_class, first_round};
  if (use_lat(c, n))
    return run_lat(c, n, [&](uint8_t* cls) { blsk::launch_lat_chained(src, 0, n, pk.tab, pk.inf, cls, st); }, out, st);
  return run_passes(
      c, n, {d_sigs96, 96, 0}, pk, [&](size_t base, size_t cnt, hipStream_t s) { hash_chained(c, src, base, cnt, s); },
      tail, out, st);
}

extern "C" {

int blsv_verify_chained(blsv_ctx* c, uint64_t first_round, const uint8_t* prev0, size_t prev0_len,
                        const uint8_t* sigs96, size_t n, uint8_t* ok_bitmap, uint64_t* first_bad,
                        uint8_t* reject_class) {
  if (!c) return BLSV_EINVAL;
  return chained_host(c, "verify_chained", false, false, first_round, prev0, prev0_len, sigs96, n, ok_bitmap, first_bad,
                      reject_class);
}

int blsv_verify_prevs(blsv_ctx* c, uint64_t first_round, const uint8_t* prevs96, size_t prev0_len,
                      const uint8_t* sigs96, size_t n, uint8_t* ok_bitmap, uint64_t* first_bad,
                      uint8_t* reject_class) {
  if (!c) return BLSV_EINVAL;
  return chained_host(c, "verify_prevs", true, false, first_round, prevs96, prev0_len, sigs96, n, ok_bitmap, first_bad,
                      reject_class);
}

// The randomized entry points are their exact counterparts (same body, same checks, and the exact
// one's name in the error texts) whenever use_rlc says the batch is too small for shared checks.
int blsv_verify_chained_rlc(blsv_ctx* c, uint64_t first_round, const uint8_t* prev0, size_t prev0_len,
                            const uint8_t* sigs96, size_t n, uint8_t* ok_bitmap, uint64_t* first_bad,
                            uint8_t* reject_class) {
  if (!c) return BLSV_EINVAL;
  const bool rlc = use_rlc(c, n);
  return chained_host(c, rlc ? "verify_chained_rlc" : "verify_chained", false, rlc, first_round, prev0, prev0_len,
                      sigs96, n, ok_bitmap, first_bad, reject_class);
}

int blsv_verify_unchained(blsv_ctx* c, const uint64_t* rounds, uint64_t first_round, const uint8_t* sigs96, size_t n,
                          uint8_t* ok_bitmap, uint64_t* first_bad, uint8_t* reject_class) {
  if (!c) return BLSV_EINVAL;
  return unchained_host(c, "verify_unchained", false, rounds, first_round, sigs96, n, ok_bitmap, first_bad,
                        reject_class);
}

int blsv_verify_unchained_rlc(blsv_ctx* c, const uint64_t* rounds, uint64_t first_round, const uint8_t* sigs96,
                              size_t n, uint8_t* ok_bitmap, uint64_t* first_bad, uint8_t* reject_class) {
  if (!c) return BLSV_EINVAL;
  const bool rlc = use_rlc(c, n);
  return unchained_host(c, rlc ? "verify_unchained_rlc" : "verify_unchained", rlc, rounds, first_round, sigs96, n,
                        ok_bitmap, first_bad, reject_class);
}

int blsv_verify_chained_dev(blsv_ctx* c, uint64_t first_round, uint64_t seg_len, uint64_t seg_phase,
                            const uint8_t* d_seeds96, size_t seed0_len, const uint8_t* d_sigs96, size_t n,
                            uint64_t* d_bitmap, uint64_t* d_first_bad, uint8_t* d_reject_class, void* stream) {
  if (!c) return BLSV_EINVAL;
  return chained_dev(c, "verify_chained_dev", false, first_round, seg_len, seg_phase, d_seeds96, seed0_len, d_sigs96, n,
                     d_bitmap, d_first_bad, d_reject_class, stream);
}

int blsv_verify_chained_rlc_dev(blsv_ctx* c, uint64_t first_round, uint64_t seg_len, uint64_t seg_phase,
                                const uint8_t* d_seeds96, size_t seed0_len, const uint8_t* d_sigs96, size_t n,
                                uint64_t* d_bitmap, uint64_t* d_first_bad, uint8_t* d_reject_class, void* stream) {
  if (!c) return BLSV_EINVAL;
  const bool rlc = use_rlc(c, n);
  return chained_dev(c, rlc ? "verify_chained_rlc_dev" : "verify_chained_dev", rlc, first_round, seg_len, seg_phase,
                     d_seeds96, seed0_len, d_sigs96, n, d_bitmap, d_first_bad, d_reject_class, stream);
}

int blsv_verify_chained_multi(blsv_ctx* const* ctxs, size_t n_ctx, const size_t* shard_counts, uint64_t first_round,
                              const uint8_t* prev0, size_t prev0_len, const uint8_t* sigs96, size_t n,
                              uint8_t* ok_bitmap, uint64_t* first_bad, uint8_t* reject_class) {
  if (!ctxs || n_ctx == 0) return BLSV_EINVAL;
  for (size_t k = 0; k < n_ctx; k++) {
    if (!ctxs[k]) return BLSV_EINVAL;
    for (size_t j = 0; j < k; j++)
      if (ctxs[j] == ctxs[k]) return fail(ctxs[k], BLSV_EINVAL, "verify_chained_multi: context %zu repeated", k);
  }
  blsv_ctx* c0 = ctxs[0];
  for (size_t k = 0; k < n_ctx; k++) {
    if (!ctxs[k]->has_group) return fail(ctxs[k], BLSV_ENOGROUP, "verify_chained_multi: context %zu has no group", k);
    if (ctxs[k]->group_bytes != c0->group_bytes)
      return fail(ctxs[k], BLSV_EINVAL, "verify_chained_multi: context %zu holds another group", k);
  }
  if (n && (!sigs96 || !prev0 || (prev0_len != 32 && prev0_len != 96)))
    return fail(c0, BLSV_EINVAL, "verify_chained_multi: prev0 must be 32 or 96 bytes");
  std::vector<size_t> cnt(n_ctx), start(n_ctx);
  size_t sum = 0;
  for (size_t k = 0; k < n_ctx; k++) {
    cnt[k] = shard_counts ? shard_counts[k] : n / n_ctx + (k < n % n_ctx ? 1 : 0);
    start[k] = sum;
    sum += cnt[k];
  }
  if (sum != n) return fail(c0, BLSV_EINVAL, "verify_chained_multi: shard counts sum to %zu, not %zu", sum, n);
  std::vector<std::vector<uint8_t>> bms(n_ctx);
  std::vector<uint64_t> fbs(n_ctx, UINT64_MAX);
  std::vector<int> rcs(n_ctx, BLSV_OK);
  auto shard = [&](size_t k) {
    if (!cnt[k]) return;
    bms[k].assign((cnt[k] + 7) / 8, 0);
    const bool head = start[k] == 0;
    const uint8_t* halo = head ? prev0 : sigs96 + (start[k] - 1) * 96;  // the true PreviousSig of its first round
    rcs[k] = blsv_verify_chained(ctxs[k], first_round + start[k], halo, head ? prev0_len : 96, sigs96 + start[k] * 96,
                                 cnt[k], bms[k].data(), &fbs[k], reject_class ? reject_class + start[k] : nullptr);
  };
  std::vector<std::thread> th;
  for (size_t k = 1; k < n_ctx; k++)
    if (cnt[k]) th.emplace_back(shard, k);
  shard(0);
  for (auto& t : th) t.join();
  for (size_t k = 0; k < n_ctx; k++)
    if (rcs[k]) return rcs[k];
  uint64_t fb = UINT64_MAX;
  for (size_t k = 0; k < n_ctx; k++) fb = std::min(fb, fbs[k]);
  if (first_bad) *first_bad = fb;
  if (ok_bitmap && n) {
    memset(ok_bitmap, 0, (n + 7) / 8);
    for (size_t k = 0; k < n_ctx; k++)
      if (cnt[k]) or_bits_at(ok_bitmap, bms[k].data(), cnt[k], start[k]);
  }
  return BLSV_OK;
}

int blsv_verify_messages(blsv_ctx* c, const uint8_t* pk48, const uint8_t* msgs, const uint32_t* msg_lens, size_t n,
                         const uint8_t* sigs96, uint8_t* ok_bitmap, uint64_t* first_bad, uint8_t* reject_class) {
  if (!c) return BLSV_EINVAL;
  if (n && (!msg_lens || !sigs96)) return fail(c, BLSV_EINVAL, "verify_messages: null arguments");
  (void)hipSetDevice(c->device);
  PkSel pk;
  if (pk48) {
    if (!c->pk_cache_valid || memcmp(c->pk_cache, pk48, 48) != 0) {
      std::vector<uint8_t> cls;
      int rc = decode_g1(c, pk48, 1, c->pk_tab, c->pk_inf, cls);
      if (rc) return rc;
      if (cls[0]) return fail(c, BLSV_EINVAL, "verify_messages: public key rejected (class %d)", (int)cls[0]);
      memcpy(c->pk_cache, pk48, 48);
      c->pk_cache_valid = true;
    }
    pk = {c->pk_tab.as<uint32_t>(), c->pk_inf.as<uint8_t>(), nullptr};
  } else {
    if (!c->has_group) return fail(c, BLSV_ENOGROUP, "verify_messages: no group key set");
    pk = group_pk(c);
  }
  if (n > kMaxChunk) return fail(c, BLSV_EINVAL, "verify_messages: batch larger than %zu", kMaxChunk);
  int rc = upload_messages(c, msgs, msg_lens, n);
  if (rc) return rc;
  HIPCHK(c, c->in_sigs.ensure(n * 96 + 96));
  if (n) HIPCHK(c, h2d(c, c->in_sigs.p, sigs96, n * 96));
  const SigSrc sig{c->in_sigs.as<uint8_t>(), 96, 0};
  return verify_host(
      c, n, sig, pk, [&](size_t base, size_t cnt, hipStream_t st) { hash_uploaded(c, base, cnt, st); },
      [&](uint8_t* cls) { lat_uploaded(c, sig, n, pk, cls, nullptr, nullptr, c->stream); }, false, 0, nullptr, ok_bitmap,
      first_bad, reject_class);
}

int blsv_generate_chained_dev(blsv_ctx* c, const uint8_t* sk32, uint64_t first_round, uint64_t seg_len,
                              const uint8_t* d_seeds96, size_t seed0_len, uint8_t* d_sigs96, size_t n, void* stream) {
  if (!c) return BLSV_EINVAL;
  if (!sk32 || (n && (!d_seeds96 || !d_sigs96)) || (seed0_len != 32 && seed0_len != 96))
    return fail(c, BLSV_EINVAL, "generate_chained_dev: bad arguments");
  (void)hipSetDevice(c->device);
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  uint32_t sk[8];
  scalar_mod_r(sk32, sk);
  HIPCHK(c, c->sk.ensure(32));
  HIPCHK(c, hipMemcpyAsync(c->sk.p, sk, 32, hipMemcpyHostToDevice, st));
  blsk::ChainedSrc src{d_sigs96, d_seeds96, first_round, seg_len ? seg_len : std::max<uint64_t>(n, 1),
                       (uint32_t)seed0_len};
  blsk::launch_gen_chained(c->sk.as<uint32_t>(), src, n, d_sigs96, st);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(st));  // sk staging buffer is reused by later calls
  return BLSV_OK;
}

size_t blsv_set_rlc_group(blsv_ctx* c, size_t g) {
  if (!c) return 0;
  const size_t prev = c->rlc.group;
  size_t v = kRlcGroupMin;
  while (v * 2 <= g && v < kRlcGroupMax) v *= 2;
  c->rlc.group = v;
  return prev;
}

int blsv_rlc_stats(blsv_ctx* c, uint64_t* groups, uint64_t* groups_failed, uint64_t* items_exact) {
  if (!c) return BLSV_EINVAL;
  if (groups) *groups = c->rlc.groups;
  if (groups_failed) *groups_failed = c->rlc.groups_failed;
  if (items_exact) *items_exact = c->rlc.items_exact;
  return BLSV_OK;
}

}  // extern "C"
