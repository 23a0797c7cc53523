// Signing on the latency path (blsv_set_sign_lat_max; include/blsverify.h "Signing on the latency path",
// DESIGN.md 9.1): a blsv_sign call of a few messages (threshold.cpp routes it here after its own argument
// checks) runs as ONE launch with a workgroup per message (k_lat_sign.hip), outside the pipeline staging and
// the batch signer's c->sk.
#include "host_internal.h"

// One upload (key, offsets, lengths, messages), one launch, one download (the 96-byte signatures at stride
// 96) through the path's own device buffer. The staged key -- on the device and in the host staging -- is
// cleared behind the kernel before this returns, also when the call fails. The share index never reaches the
// device: the host writes BE16(index) in front of each signature as it copies out.
int sign_lat_run(blsv_ctx* c, const uint32_t (&sk)[8], int32_t index, const uint8_t* msgs, const uint32_t* msg_lens,
                 size_t n, uint8_t* out) {
  sign_lat_state& t = c->sign_lat;
  hipStream_t st = c->stream;
  size_t mbytes = 0;
  for (size_t i = 0; i < n; i++) mbytes += msg_lens[i];  // n <= kMaxChunk lengths below 2^32: no overflow
  if (mbytes && !msgs)
    return fail(c, BLSV_EINVAL, "messages: %llu message bytes but no buffer", (unsigned long long)mbytes);
  SignLatLayout l;
  if (!sign_lat_layout(n, mbytes, l)) return fail(c, BLSV_EINVAL, "sign: too many bytes");
  HIPCHK(c, t.buf.ensure(l.total));
  t.up.resize(l.in_total);
  t.down.resize(l.out_total);
  uint8_t* up = t.up.data();
  uint64_t o = 0;
  for (size_t i = 0; i < n; i++) {
    memcpy(up + l.o_off + 8 * i, &o, 8);
    o += msg_lens[i];
  }
  memcpy(up + l.o_len, msg_lens, 4 * n);
  if (mbytes) memcpy(up + l.o_msgs, msgs, mbytes);
  memcpy(up + l.o_sk, sk, kSignLatKeyBytes);
  uint8_t* d = t.buf.as<uint8_t>();
  hipError_t e = hipMemcpyAsync(d, up, l.in_total, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    blsk::launch_lat_sign((const uint32_t*)(d + l.o_sk), d + l.o_msgs, (const uint64_t*)(d + l.o_off),
                          (const uint32_t*)(d + l.o_len), n, (uint32_t*)(d + l.o_out), st);
    e = hipGetLastError();
  }
  const hipError_t wipe = hipMemsetAsync(d + l.o_sk, 0, kSignLatKeyBytes, st);
  if (e == hipSuccess) e = wipe;
  // the download's synchronisation also ends the upload's reads of the host staging
  hipError_t down;
  if (e != hipSuccess)
    down = hipStreamSynchronize(st);
  else
    down = download_sync(c, {{t.down.data(), d + l.o_out, l.out_total}});
  memset(up + l.o_sk, 0, kSignLatKeyBytes);
  if (e == hipSuccess) e = down;
  if (e != hipSuccess) return fail(c, BLSV_EHIP, "sign (latency path): %s", hipGetErrorString(e));
  if (index < 0) {
    memcpy(out, t.down.data(), 96 * n);
  } else {
    for (size_t i = 0; i < n; i++) {
      uint8_t* p = out + 98 * i;
      p[0] = (uint8_t)(index >> 8);
      p[1] = (uint8_t)index;
      memcpy(p + 2, t.down.data() + 96 * i, 96);
    }
  }
  t.launches++;
  t.items += n;
  return BLSV_OK;
}
