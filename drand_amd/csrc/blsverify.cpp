// The context of the C ABI (include/blsverify.h): lifecycle, the HBM staging workspace, the pinned
// small copies, stage profiling and the per-context limits. The entry points that verify, recover,
// open timelocks or serve tests live in verify.cpp, threshold.cpp, tlock.cpp and testhooks.cpp.
#include "host_internal.h"

void release_workspace(blsv_ctx* c) {
  for (DBuf* d : {&c->H, &c->HQ, &c->S, &c->F, &c->FW, &c->LN, &c->h_inf, &c->s_inf, &c->cls}) d->release();
  c->cap = 0;
}

int ensure_workspace(blsv_ctx* c, size_t cnt) {
  for (;;) {
    size_t want = std::min(std::max(cnt, size_t(64)), c->chunk);
    want = (want + 63) & ~size_t(63);
    if (want <= c->cap) return BLSV_OK;
    hipError_t e = hipSuccess;
    auto need = [&](DBuf& d, size_t bytes) {
      if (e == hipSuccess) e = d.ensure(bytes);
    };
    need(c->H, want * blsk::H_WORDS * 4);
    need(c->HQ, kHqWords(want) * 4);  // with the final exponentiation's park (engine_ctx.h)
    need(c->S, want * blsk::S_WORDS * 4);
    need(c->F, want * blsk::F_WORDS * 4);
    need(c->FW, 3 * want * blsk::F_WORDS * 4);
    // (a timelock pass, which stages no lines, parks its final exponentiation in LN)
    need(c->LN, std::max(std::min(want, kLineSub) * blsk::MILLER_LINE_WORDS, blsk::FEXP_PARK_WORDS(want)) * 4);
    need(c->h_inf, want);
    need(c->s_inf, want);
    need(c->cls, want);
    static_assert(3 * blsk::F_WORDS >= 48 * 64 / 21 + 1, "FW holds the Miller park of a sub-chunk");
    if (e == hipSuccess) {
      c->cap = want;
      return BLSV_OK;
    }
    release_workspace(c);
    (void)hipGetLastError();  // clear the sticky allocation error
    if (e != hipErrorOutOfMemory || want <= kMinChunk)
      return fail(c, BLSV_EHIP, "staging for %zu items: %s", want, hipGetErrorString(e));
    // out of HBM (other contexts or ranks on this GPU): halve the pass size and retry
    c->chunk = std::max(kMinChunk, ((want / 2) + 63) & ~size_t(63));
    c->lat_max = std::min(c->lat_max, c->chunk);
    c->tlock_lat.lat_max = std::min(c->tlock_lat.lat_max, c->chunk);
    c->tseal_lat.lat_max = std::min(c->tseal_lat.lat_max, c->chunk);
    c->tauth_lat.open_max = std::min(c->tauth_lat.open_max, c->chunk);
    c->tauth_lat.seal_max = std::min(c->tauth_lat.seal_max, c->chunk);
    c->sign_lat.lat_max = std::min(c->sign_lat.lat_max, c->chunk);
    c->oom_halvings++;
  }
}

// Small copies on the main stream go through pinned staging: hipMemcpyAsync from pageable memory is
// staged by the runtime and costs ~10 us per copy, which is most of a lone verify's host time.
// Uploads are copied into io_up (the caller's buffer is free on return) and DMA'd from there; the
// staging is appended to and reused from offset 0 only after a synchronisation of the stream, so no
// copy still in flight is overwritten. Downloads land in io_down and reach the caller's buffers after
// the synchronisation download_sync itself does. Larger copies take the pageable path as before.
hipError_t h2d(blsv_ctx* c, void* dst, const void* src, size_t len) {
  if (!len) return hipSuccess;
  if (len > kIoCap / 4) return hipMemcpyAsync(dst, src, len, hipMemcpyHostToDevice, c->stream);
  if (!c->io_up.p) {
    hipError_t e = c->io_up.ensure(kIoCap);
    if (e != hipSuccess) return e;
  }
  if (c->io_up_off + len > kIoCap) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return e;
    c->io_up_off = 0;
  }
  uint8_t* h = c->io_up.as<uint8_t>() + c->io_up_off;
  memcpy(h, src, len);
  c->io_up_off += (len + 63) & ~size_t(63);
  return hipMemcpyAsync(dst, h, len, hipMemcpyHostToDevice, c->stream);
}

hipError_t download_sync(blsv_ctx* c, std::initializer_list<Down> ds) {
  size_t total = 0;
  for (const Down& d : ds) total += (d.len + 63) & ~size_t(63);
  const bool staged = total <= kIoCap && (c->io_down.p || c->io_down.ensure(kIoCap) == hipSuccess);
  hipError_t e = hipSuccess;
  size_t off = 0;
  for (const Down& d : ds) {
    if (!d.len) continue;
    void* to = staged ? (void*)(c->io_down.as<uint8_t>() + off) : d.user;
    if (e == hipSuccess) e = hipMemcpyAsync(to, d.dev, d.len, hipMemcpyDeviceToHost, c->stream);
    off += (d.len + 63) & ~size_t(63);
  }
  const hipError_t es = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = es;
  if (e == hipSuccess) c->io_up_off = 0;  // every staged upload has completed too
  if (e != hipSuccess || !staged) return e;
  off = 0;
  for (const Down& d : ds) {
    if (d.len) memcpy(d.user, c->io_down.as<uint8_t>() + off, d.len);
    off += (d.len + 63) & ~size_t(63);
  }
  return hipSuccess;
}

hipEvent_t take_event(blsv_ctx* c) {
  if (!c->event_pool.empty()) {
    hipEvent_t e = c->event_pool.back();
    c->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

extern "C" {

const char* blsv_version(void) { return "drand_amd blsverify 0.1 (gfx950)"; }

int blsv_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int blsv_create(int device, blsv_ctx** out) {
  if (!out) return BLSV_EINVAL;
  *out = nullptr;
  blsv_ctx* c = new blsv_ctx();
  c->device = device;
  c->tlock_lat.lat_max = std::min(tlock_lat_max_env(), c->chunk);
  c->tseal_lat.lat_max = std::min(tseal_lat_max_env(), c->chunk);
  c->tauth_lat.open_max = std::min(tauth_lat_max_env("BLSV_TAUTH_OPEN_LAT_MAX"), c->chunk);
  c->tauth_lat.seal_max = std::min(tauth_lat_max_env("BLSV_TAUTH_SEAL_LAT_MAX"), c->chunk);
  c->sign_lat.lat_max = std::min(sign_lat_max_env(), c->chunk);
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->side2, hipStreamNonBlocking);
  for (hipEvent_t& ev : c->hash_ev)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->join_ev, hipEventDisableTiming);
  int cus = 0;
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  c->tail_q_dev = c->tail_q = size_t(64) * 4 * (size_t)std::max(cus, 0);
  if (e != hipSuccess) {
    fprintf(stderr, "blsv_create: %s\n", hipGetErrorString(e));
    blsv_destroy(c);  // releases whatever was created
    return BLSV_EHIP;
  }
  *out = c;
  return BLSV_OK;
}

void blsv_destroy(blsv_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (hipStream_t s : {c->stream, c->side, c->side2}) {
    if (!s) continue;
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
  }
  for (hipEvent_t ev : c->hash_ev)
    if (ev) (void)hipEventDestroy(ev);
  if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
  if (c->join_ev) (void)hipEventDestroy(c->join_ev);
  (void)hipDeviceSynchronize();
  for (auto& r : c->recs)
    for (hipEvent_t e : {r.a, r.b, r.a2, r.b2})
      if (e) (void)hipEventDestroy(e);
  for (auto e : c->event_pool) (void)hipEventDestroy(e);
  delete c;
}

const char* blsv_last_error(const blsv_ctx* c) { return c ? c->err.c_str() : "null context"; }

int blsv_synchronize(blsv_ctx* c) {
  if (!c) return BLSV_EINVAL;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BLSV_OK;
}

// ------------------------------------------------------------------ stage profiling
int blsv_profile_enable(blsv_ctx* c, int on) {
  if (!c) return BLSV_EINVAL;
  c->prof = on != 0;
  return BLSV_OK;
}

int blsv_profile_read(blsv_ctx* c, double* ms, uint64_t* launches, uint64_t* items, int nstages) {
  if (!c || nstages < 0) return BLSV_EINVAL;
  (void)hipSetDevice(c->device);
  for (int s = 0; s < nstages; s++) {
    if (ms) ms[s] = 0;
    if (launches) launches[s] = 0;
    if (items) items[s] = 0;
  }
  for (auto& r : c->recs) {
    HIPCHK(c, hipEventSynchronize(r.b));
    float t = 0;
    HIPCHK(c, hipEventElapsedTime(&t, r.a, r.b));
    if (r.a2 && r.b2) {  // a split pass's side span: summed, one launch
      float t2 = 0;
      HIPCHK(c, hipEventSynchronize(r.b2));
      HIPCHK(c, hipEventElapsedTime(&t2, r.a2, r.b2));
      t += t2;
    }
    if (r.stage < nstages) {
      if (ms) ms[r.stage] += t;
      if (launches) launches[r.stage] += 1;
      if (items) items[r.stage] += r.items;
    }
    for (hipEvent_t e : {r.a, r.b, r.a2, r.b2})
      if (e) c->event_pool.push_back(e);
  }
  c->recs.clear();
  return ST_N;
}

// latency-path cutover (include/blsverify.h latency contract)
size_t blsv_set_lat_max(blsv_ctx* c, size_t lat_max) {
  if (!c) return 0;
  const size_t prev = c->lat_max;
  c->lat_max = std::min(lat_max, c->chunk);  // see lat_max_env: larger batches take the pipeline
  return prev;
}

// cutover of the timelock opening's latency path (include/blsverify.h "timelock"; 0 = off)
size_t blsv_set_tlock_lat_max(blsv_ctx* c, size_t items) {
  if (!c) return 0;
  const size_t prev = c->tlock_lat.lat_max;
  c->tlock_lat.lat_max = std::min(items, c->chunk);
  return prev;
}

int blsv_tlock_lat_stats(blsv_ctx* c, uint64_t* launches, uint64_t* items) {
  if (!c) return BLSV_EINVAL;
  if (launches) *launches = c->tlock_lat.launches;
  if (items) *items = c->tlock_lat.items;
  return BLSV_OK;
}

// cutover of the timelock sealing's latency path (include/blsverify.h "timelock"; 0 = off)
size_t blsv_set_tseal_lat_max(blsv_ctx* c, size_t items) {
  if (!c) return 0;
  const size_t prev = c->tseal_lat.lat_max;
  c->tseal_lat.lat_max = std::min(items, c->chunk);
  return prev;
}

int blsv_tseal_lat_stats(blsv_ctx* c, uint64_t* launches, uint64_t* items) {
  if (!c) return BLSV_EINVAL;
  if (launches) *launches = c->tseal_lat.launches;
  if (items) *items = c->tseal_lat.items;
  return BLSV_OK;
}

// cutovers of the authenticated timelock's latency path (include/blsverify.h "authenticated timelock"; 0 =
// off, SIZE_MAX = keep); returns the larger of the two values in force
size_t blsv_set_tauth_lat_max(blsv_ctx* c, size_t open_items, size_t seal_items) {
  if (!c) return 0;
  if (open_items != SIZE_MAX) c->tauth_lat.open_max = std::min(open_items, c->chunk);
  if (seal_items != SIZE_MAX) c->tauth_lat.seal_max = std::min(seal_items, c->chunk);
  return std::max(c->tauth_lat.open_max, c->tauth_lat.seal_max);
}

int blsv_tauth_lat_stats(blsv_ctx* c, uint64_t* open_launches, uint64_t* open_items, uint64_t* seal_launches,
                         uint64_t* seal_items) {
  if (!c) return BLSV_EINVAL;
  if (open_launches) *open_launches = c->tauth_lat.open_launches;
  if (open_items) *open_items = c->tauth_lat.open_items;
  if (seal_launches) *seal_launches = c->tauth_lat.seal_launches;
  if (seal_items) *seal_items = c->tauth_lat.seal_items;
  return BLSV_OK;
}

// cutover of the signing's latency path (include/blsverify.h "Signing on the latency path"; 0 = off)
size_t blsv_set_sign_lat_max(blsv_ctx* c, size_t items) {
  if (!c) return 0;
  const size_t prev = c->sign_lat.lat_max;
  c->sign_lat.lat_max = std::min(items, c->chunk);
  return prev;
}

int blsv_sign_lat_stats(blsv_ctx* c, uint64_t* launches, uint64_t* items) {
  if (!c) return BLSV_EINVAL;
  if (launches) *launches = c->sign_lat.launches;
  if (items) *items = c->sign_lat.items;
  return BLSV_OK;
}

// per-context pass size (include/blsverify.h memory contract)
size_t blsv_set_chunk(blsv_ctx* c, size_t items) {
  if (!c) return 0;
  const size_t prev = c->chunk;
  size_t v = items ? std::min(std::max(items, kMinChunk), kMaxChunk) : chunk_env();
  v = (v + 63) & ~size_t(63);
  (void)hipSetDevice(c->device);
  if (v < c->cap) {  // give the HBM back now: the next call allocates at the new size
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->side);
    release_workspace(c);
  }
  c->chunk = v;
  c->lat_max = std::min(c->lat_max, v);
  c->tlock_lat.lat_max = std::min(c->tlock_lat.lat_max, v);
  c->tseal_lat.lat_max = std::min(c->tseal_lat.lat_max, v);
  c->tauth_lat.open_max = std::min(c->tauth_lat.open_max, v);
  c->tauth_lat.seal_max = std::min(c->tauth_lat.seal_max, v);
  c->sign_lat.lat_max = std::min(c->sign_lat.lat_max, v);
  return prev;
}

size_t blsv_workspace_bytes(const blsv_ctx* c) {
  if (!c) return 0;
  size_t b = 0;
  for (const DBuf* d : {&c->H, &c->HQ, &c->S, &c->F, &c->FW, &c->LN, &c->h_inf, &c->s_inf, &c->cls}) b += d->sz;
  return b;
}

}  // extern "C"
