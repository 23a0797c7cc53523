// Timelock sealing on the latency path (blsv_set_tseal_lat_max; include/blsverify.h "timelock", DESIGN.md
// 8.6): a host call of a few items of blsv_tlock_seal or blsv_tlock_seal_rounds (tseal.cpp / tsealr.cpp
// route it here after their own argument checks) runs as ONE launch with a workgroup per item
// (k_lat_tseal.hip), outside the pipeline staging, the base cache and the sigma cache. The generator's table
// T1 and the key's table TK are the batch path's, behind its one-entry key cache.
#include "host_internal.h"

// One upload (rounds, scalars), one launch, one download (U bytes, Gt bytes, ok) through the path's own
// device buffer. The staged scalars -- on the device and in the host staging -- are cleared behind the
// kernel before this returns, also when the call fails. An encrypting call (mlen != 0; blsv_tlock_encrypt*)
// uploads its messages behind the scalars, runs the mask kernel behind the latency kernel over the Gt bytes
// it wrote, clears those bytes and the staged messages with the scalars, and downloads the U bytes, the
// n x mlen ciphertext bytes (into `out`) and ok: K_i stays on the device.
int tseal_lat_run(blsv_ctx* c, const uint8_t* pk48, const uint64_t* rounds, uint64_t round, const uint8_t* scalars32,
                  size_t n, uint8_t* out_us48, uint8_t* out, uint8_t* ok, const uint8_t* msgs, size_t mlen) {
  tseal_lat_state& t = c->tseal_lat;
  hipStream_t st = c->stream;
  TsealLatLayout l;
  if (!tseal_lat_layout(n, rounds != nullptr, l, mlen)) return fail(c, BLSV_EINVAL, "tlock_seal: too many items");
  int rc = sealr_prepare(c, pk48, n, st);  // T1 and TK; a rejected key ends the call here
  if (rc) return rc;
  HIPCHK(c, t.buf.ensure(l.total));
  t.up.resize(l.in_total);
  t.down.resize(l.out_total);
  if (rounds) memcpy(t.up.data() + l.o_rounds, rounds, 8 * n);
  memcpy(t.up.data() + l.o_scalars, scalars32, BLSV_SCALAR_LEN * n);
  if (mlen) memcpy(t.up.data() + l.o_min, msgs, mlen * n);
  uint8_t* d = t.buf.as<uint8_t>();
  hipError_t e = hipMemcpyAsync(d, t.up.data(), l.in_total, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    blsk::launch_lat_tseal(c->tseal.t1.as<uint32_t>(), c->tsealr.tk.as<uint32_t>(),
                           rounds ? (const uint64_t*)(d + l.o_rounds) : nullptr, round, d + l.o_scalars, n, d + l.o_us,
                           d + l.o_gt, d + l.o_ok, st);
    if (mlen) blsk::launch_tmask_encoded(d + l.o_gt, d + l.o_ok, 1, n, d + l.o_min, d + l.o_mout, mlen, st);
    e = hipGetLastError();
  }
  // the scalars, and an encrypting call's messages behind them and its K_i
  hipError_t wipe = hipMemsetAsync(d + l.o_scalars, 0, l.in_total - l.o_scalars, st);
  if (mlen && wipe == hipSuccess) wipe = hipMemsetAsync(d + l.o_gt, 0, BLSV_GT_LEN * n, st);
  if (e == hipSuccess) e = wipe;
  // the download's synchronisation also ends the upload's reads of the host staging
  hipError_t down;
  if (e != hipSuccess)
    down = hipStreamSynchronize(st);
  else if (mlen)
    down = download_sync(c, {{t.down.data(), d + l.o_us, BLSV_U_LEN * n},
                             {t.down.data() + (l.o_mout - l.o_us), d + l.o_mout, mlen * n + n}});
  else
    down = download_sync(c, {{t.down.data(), d + l.o_us, l.out_total}});
  memset(t.up.data() + l.o_scalars, 0, l.in_total - l.o_scalars);
  if (e == hipSuccess) e = down;
  if (e != hipSuccess) return fail(c, BLSV_EHIP, "tlock_seal (latency path): %s", hipGetErrorString(e));
  memcpy(out_us48, t.down.data(), BLSV_U_LEN * n);
  if (mlen)
    memcpy(out, t.down.data() + (l.o_mout - l.o_us), mlen * n);
  else
    memcpy(out, t.down.data() + (l.o_gt - l.o_us), BLSV_GT_LEN * n);
  memcpy(ok, t.down.data() + (l.o_ok - l.o_us), n);
  t.launches++;
  t.items += n;
  return BLSV_OK;
}
