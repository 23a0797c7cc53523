// Timelock sealing on the latency path (blsv_set_tseal_lat_max; include/blsverify.h "timelock", DESIGN.md
// 8.6): a host call of a few items of blsv_tlock_seal or blsv_tlock_seal_rounds (tseal.cpp / tsealr.cpp
// route it here after their own argument checks) runs as ONE launch with a workgroup per item
// (k_lat_tseal.hip), outside the pipeline staging, the base cache and the sigma cache. The generator's table
// T1 and the key's table TK are the batch path's, behind its one-entry key cache.
#include "host_internal.h"

// One upload (rounds, scalars), one launch, one download (U bytes, Gt bytes, ok) through the path's own
// device buffer. The staged scalars -- on the device and in the host staging -- are cleared behind the
// kernel before this returns, also when the call fails.
int tseal_lat_run(blsv_ctx* c, const uint8_t* pk48, const uint64_t* rounds, uint64_t round, const uint8_t* scalars32,
                  size_t n, uint8_t* out_us48, uint8_t* out_gt576, uint8_t* ok) {
  tseal_lat_state& t = c->tseal_lat;
  hipStream_t st = c->stream;
  TsealLatLayout l;
  if (!tseal_lat_layout(n, rounds != nullptr, l)) return fail(c, BLSV_EINVAL, "tlock_seal: too many items");
  int rc = sealr_prepare(c, pk48, n, st);  // T1 and TK; a rejected key ends the call here
  if (rc) return rc;
  HIPCHK(c, t.buf.ensure(l.total));
  t.up.resize(l.in_total);
  t.down.resize(l.out_total);
  if (rounds) memcpy(t.up.data() + l.o_rounds, rounds, 8 * n);
  memcpy(t.up.data() + l.o_scalars, scalars32, BLSV_SCALAR_LEN * n);
  uint8_t* d = t.buf.as<uint8_t>();
  hipError_t e = hipMemcpyAsync(d, t.up.data(), l.in_total, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    blsk::launch_lat_tseal(c->tseal.t1.as<uint32_t>(), c->tsealr.tk.as<uint32_t>(),
                           rounds ? (const uint64_t*)(d + l.o_rounds) : nullptr, round, d + l.o_scalars, n, d + l.o_us,
                           d + l.o_gt, d + l.o_ok, st);
    e = hipGetLastError();
  }
  const hipError_t wipe = hipMemsetAsync(d + l.o_scalars, 0, BLSV_SCALAR_LEN * n, st);
  if (e == hipSuccess) e = wipe;
  // the download's synchronisation also ends the upload's reads of the host staging
  const hipError_t down = e == hipSuccess ? download_sync(c, {{t.down.data(), d + l.o_us, l.out_total}})
                                          : hipStreamSynchronize(st);
  memset(t.up.data() + l.o_scalars, 0, BLSV_SCALAR_LEN * n);
  if (e == hipSuccess) e = down;
  if (e != hipSuccess) return fail(c, BLSV_EHIP, "tlock_seal (latency path): %s", hipGetErrorString(e));
  memcpy(out_us48, t.down.data(), BLSV_U_LEN * n);
  memcpy(out_gt576, t.down.data() + (l.o_gt - l.o_us), BLSV_GT_LEN * n);
  memcpy(ok, t.down.data() + (l.o_ok - l.o_us), n);
  t.launches++;
  t.items += n;
  return BLSV_OK;
}
