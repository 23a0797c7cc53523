// Test hooks of the C ABI (include/blsverify_testing.h): raw building blocks of the kernels and of
// the host logic, the randomized path's pinned seed and sums, and the latency engine's phase trace.
#include "../../include/blsverify_testing.h"
#include "host_internal.h"
#include "testops_list.h"

static const bls::TestOpInfo* find_test_op(const char* name, int* op) {
  if (!name) return nullptr;
  const bls::TestOpInfo* tab = bls::test_op_table();
  for (int k = 0; k < bls::TOP_COUNT; k++)
    if (!strcmp(tab[k].name, name)) {
      if (op) *op = k;
      return &tab[k];
    }
  return nullptr;
}

extern "C" {

int blsv_test_lagrange(const uint32_t* idx, size_t t, uint32_t* out) {
  if (!idx || !out) return BLSV_EINVAL;
  for (size_t i = 0; i < t; i++)
    for (size_t j = 0; j < i; j++)
      if (idx[i] == idx[j]) return BLSV_EINVAL;
  host_lagrange(idx, t, out);
  return BLSV_OK;
}

int blsv_test_rlc_seed(blsv_ctx* c, const uint8_t* seed32) {
  if (!c) return BLSV_EINVAL;
  c->rlc.seed_pinned = seed32 != nullptr;
  if (seed32) memcpy(c->rlc.seed, seed32, 32);
  return BLSV_OK;
}

int blsv_test_rlc_sums(blsv_ctx* c, uint64_t first_round, const uint8_t* prev0, size_t prev0_len,
                       const uint8_t* sigs96, size_t n, uint8_t* out_a96, uint8_t* out_b96) {
  if (!c) return BLSV_EINVAL;
  if (!n || !sigs96 || !prev0 || !out_a96 || !out_b96 || (prev0_len != 32 && prev0_len != 96))
    return fail(c, BLSV_EINVAL, "test_rlc_sums: bad arguments");
  (void)hipSetDevice(c->device);
  Tail tail;
  tail.randomized = true;
  int rc = rlc_draw_seed(c, tail.seed);
  if (rc) return rc;
  rc = ensure_workspace(c, n);
  if (rc) return rc;
  blsk::ChainedSrc src;
  rc = stage_chain(c, first_round, prev0, prev0_len, false, sigs96, n, src);
  if (rc) return rc;
  rlc_state& r = c->rlc;
  size_t done = 0;  // groups written so far
  // the randomized pass up to its combination stage, whose sums are compressed instead of checked
  rc = for_each_pass(c, n, [&](size_t base, size_t cnt) {
    const size_t ng = blsk::rlc_groups(cnt, r.group);
    int prc = run_head(c, {src.sigs, 96, 0}, base, cnt, tail, c->stream,
                       [&](size_t b, size_t m, hipStream_t st) { hash_chained(c, src, b, m, st); });
    if (prc) return prc;
    prc = rlc_sums(c, base, cnt, tail.seed, c->stream);
    if (prc) return prc;
    HIPCHK(c, r.out96.ensure(2 * ng * 96));
    uint8_t* d_out = r.out96.as<uint8_t>();
    blsk::launch_rlc_compress(r.gH.as<uint32_t>(), r.g_hinf.as<uint8_t>(), ng, d_out, c->stream);
    blsk::launch_rlc_compress(r.gS.as<uint32_t>(), r.g_sinf.as<uint8_t>(), ng, d_out + ng * 96, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_a96 + done * 96, d_out, ng * 96, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_b96 + done * 96, d_out + ng * 96, ng * 96, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->io_up_off = 0;
    done += ng;
    return BLSV_OK;
  });
  return rc ? rc : (int)done;
}

int blsv_test_spec_stats(blsv_ctx* c, uint64_t* hits, uint64_t* misses) {
  if (!c || !hits || !misses) return BLSV_EINVAL;
  *hits = c->spec_hits;
  *misses = c->spec_misses;
  return BLSV_OK;
}

int blsv_test_tail_split(blsv_ctx* c, size_t q) {
  if (!c) return BLSV_EINVAL;
  c->tail_q = q == SIZE_MAX ? c->tail_q_dev : q;
  return BLSV_OK;
}

int blsv_test_tauth_walk_waves(blsv_ctx* c, int waves) {
  if (!c || (waves != 1 && waves != 8)) return BLSV_EINVAL;
  c->tauth_lat.walk_waves = waves;
  return BLSV_OK;
}

int blsv_test_generic_chains(blsv_ctx* c, int on) {
  if (!c) return BLSV_EINVAL;
  blsk::g_generic_chains_all = on != 0;
  return BLSV_OK;
}

int blsv_lat_trace_enable(blsv_ctx* c, int on) {
  if (!c) return BLSV_EINVAL;
  (void)hipSetDevice(c->device);
  if (blsk::lat_trace_enable(on, c->stream) != 0) return fail(c, BLSV_EHIP, "lat_trace_enable: symbol copy failed");
  return BLSV_OK;
}

int blsv_lat_trace(blsv_ctx* c, uint64_t* ticks, int n, double* ticks_per_us, int clear) {
  if (!c || n < 0 || (n && !ticks)) return BLSV_EINVAL;
  (void)hipSetDevice(c->device);
  // the marks are device-global: wait for every latency launch on the device (any stream, any context)
  HIPCHK(c, hipDeviceSynchronize());
  int got = 0;
  if (n) {
    got = blsk::lat_trace_read(ticks, n, c->stream);
    if (got < 0) return fail(c, BLSV_EHIP, "lat_trace: symbol copy failed");
  }
  if (ticks_per_us) {
    int khz = 0;
    HIPCHK(c, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
    *ticks_per_us = khz / 1000.0;
  }
  if (clear && blsk::lat_trace_clear(c->stream) != 0) return fail(c, BLSV_EHIP, "lat_trace: clear failed");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return got;
}

int blsv_test_fp_mul(blsv_ctx* c, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out) {
  if (!c || (n && (!a || !b || !out))) return BLSV_EINVAL;
  (void)hipSetDevice(c->device);
  DBuf da, db, dout;
  HIPCHK(c, da.ensure(n * 48));
  HIPCHK(c, db.ensure(n * 48));
  HIPCHK(c, dout.ensure(n * 48));
  HIPCHK(c, hipMemcpyAsync(da.p, a, n * 48, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db.p, b, n * 48, hipMemcpyHostToDevice, c->stream));
  blsk::launch_test_fp_mul(da.as<uint32_t>(), db.as<uint32_t>(), n, dout.as<uint32_t>(), c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, dout.p, n * 48, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BLSV_OK;
}

int blsv_test_pairing(blsv_ctx* c, const uint32_t* p, const uint32_t* q, size_t n, uint32_t* out_f) {
  if (!c || (n && (!p || !q || !out_f))) return BLSV_EINVAL;
  (void)hipSetDevice(c->device);
  DBuf dp, dq, dout;
  HIPCHK(c, dp.ensure(n * 96));
  HIPCHK(c, dq.ensure(n * 192));
  HIPCHK(c, dout.ensure(n * 576));
  HIPCHK(c, hipMemcpyAsync(dp.p, p, n * 96, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dq.p, q, n * 192, hipMemcpyHostToDevice, c->stream));
  blsk::launch_test_pairing(dp.as<uint32_t>(), dq.as<uint32_t>(), n, dout.as<uint32_t>(), c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out_f, dout.p, n * 576, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BLSV_OK;
}

int blsv_test_final_exp(blsv_ctx* c, const uint32_t* f, size_t n, uint32_t* out_pipeline, uint32_t* out_ref) {
  if (!c || (n && (!f || !out_pipeline || !out_ref))) return BLSV_EINVAL;
  if (n > kMaxChunk) return BLSV_EINVAL;
  (void)hipSetDevice(c->device);
  int rc = ensure_workspace(c, n);
  if (rc) return rc;
  if (n > c->cap) return fail(c, BLSV_EINVAL, "test_final_exp: more than the context chunk");
  if (!n) return BLSV_OK;
  DBuf din, dout, dref;
  HIPCHK(c, din.ensure(n * 576));
  HIPCHK(c, dout.ensure(n * 576));
  HIPCHK(c, dref.ensure(n * 576));
  const Staging w = staging(c);
  HIPCHK(c, hipMemcpyAsync(din.p, f, n * 576, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(w.cls, 0, n, c->stream));
  blsk::launch_test_pack_fp12(din.as<uint32_t>(), n, w.F, c->stream);
  blsk::launch_test_final_exp_ref(w.F, n, dref.as<uint32_t>(), c->stream);
  // the production stage (clobbers F), its final value captured into dout: whole, or as the two ranges
  // of the context's split rule (blsv_test_tail_split), one after the other with their own park areas
  const size_t mn = tail_split_main(n, c->tail_q);
  final_exp(c, n, 0, mn, w.cls, c->stream, dout.as<uint32_t>());
  final_exp(c, n, mn, n - mn, w.cls, c->stream, dout.as<uint32_t>());
  blsk::launch_test_unpack_fp12(dout.as<uint32_t>(), n, din.as<uint32_t>(), c->stream);
  HIPCHK(c, hipMemcpyAsync(out_pipeline, din.p, n * 576, hipMemcpyDeviceToHost, c->stream));
  blsk::launch_test_unpack_fp12(dref.as<uint32_t>(), n, dout.as<uint32_t>(), c->stream);
  HIPCHK(c, hipMemcpyAsync(out_ref, dout.p, n * 576, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BLSV_OK;
}

int blsv_test_op_info(int index, const char** name, int* in_fp, int* out_fp, int* lanes) {
  if (index < 0 || index >= bls::TOP_COUNT) return BLSV_EINVAL;
  const bls::TestOpInfo& t = bls::test_op_table()[index];
  if (name) *name = t.name;
  if (in_fp) *in_fp = t.nin;
  if (out_fp) *out_fp = t.nout;
  if (lanes) *lanes = t.kind == 3 ? 3 : 1;
  return BLSV_OK;
}

int blsv_test_op(blsv_ctx* c, const char* name, const uint32_t* in, size_t n, uint32_t* out) {
  int op = 0;
  const bls::TestOpInfo* t = find_test_op(name, &op);
  if (!c || !t || (n && (!in || !out))) return BLSV_EINVAL;
  if (n > kMaxChunk) return BLSV_EINVAL;
  if (!n) return BLSV_OK;
  (void)hipSetDevice(c->device);
  const size_t in_bytes = n * (size_t)t->nin * 48, out_bytes = n * (size_t)t->nout * 48;
  DBuf din, dout, dpark;
  HIPCHK(c, din.ensure(in_bytes));
  HIPCHK(c, dout.ensure(out_bytes));
  if (t->kind == 3) HIPCHK(c, dpark.ensure(blsk::TRI_PARK_WORDS(n) * 4));
  HIPCHK(c, hipMemcpyAsync(din.p, in, in_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(dout.p, 0xA5, out_bytes, c->stream));  // an item the kernel skips shows
  const bool ran = t->kind == 2
                       ? blsk::launch_test_op_mf(op, din.as<uint32_t>(), n, dout.as<uint32_t>(), c->stream)
                       : blsk::launch_test_op(op, din.as<uint32_t>(), n, dout.as<uint32_t>(),
                                              t->kind == 3 ? dpark.as<uint32_t>() : nullptr, c->stream);
  // no fall-back: an op of the list without a kernel is an error
  if (!ran) return fail(c, BLSV_EINVAL, "test_op: no kernel for this op");
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, dout.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BLSV_OK;
}

int blsv_test_hash_to_g2(blsv_ctx* c, const uint8_t* msgs, const uint32_t* msg_lens, size_t n, uint32_t* out,
                         uint8_t* inf) {
  if (!c || (n && (!msg_lens || !out || !inf))) return BLSV_EINVAL;
  if (n > kMaxChunk) return BLSV_EINVAL;
  (void)hipSetDevice(c->device);
  int rc = ensure_workspace(c, n);
  if (rc) return rc;
  if (n > c->cap) return fail(c, BLSV_EINVAL, "test_hash_to_g2: more than the context chunk");
  rc = upload_messages(c, msgs, msg_lens, n);
  if (rc) return rc;
  DBuf dout;
  HIPCHK(c, dout.ensure(n * 192));
  hash_uploaded(c, 0, n, c->stream);
  blsk::launch_test_unpack_g2(c->H.as<uint32_t>(), n, dout.as<uint32_t>(), c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, dout.p, n * 192, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(inf, c->h_inf.p, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BLSV_OK;
}

}  // extern "C"
