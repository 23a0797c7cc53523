// Timelock in one call: the fused tail blsv_tlock_decrypt* and blsv_tlock_encrypt* put where the four
// timelock passes (tlock.cpp, tlockr.cpp, tseal.cpp, tsealr.cpp) run the Gt encoding (include/blsverify.h
// "timelock in one call", tmask.h). The entry points live beside the passes they run; this is what they share.
#include "host_internal.h"

static_assert(2 * BLSV_TLOCK_MSG_MAX <= BLSV_GT_LEN,
              "a host pass's input and output bytes do not fit the F staging (one Gt row per item)");
static_assert(BLSV_TLOCK_MSG_MAX == blsk::kTmaskMsgMax, "the header's cap is the kernel's");

uint8_t* mask_host_out(const blsv_ctx* c, const MaskTail& mk, size_t cnt) {
  return c->F.as<uint8_t>() + cnt * mk.mlen;  // mlen == 0: the encoded values from the start of F
}

int mask_tail(blsv_ctx* c, const MaskTail& mk, const uint8_t* flag, uint8_t good, size_t cnt, const uint8_t* in,
              uint8_t* d_out, hipStream_t st) {
  const Staging w = staging(c);
  const uint8_t* d_in = in;
  if (mk.host) {
    // F is free behind the final exponentiation. Plaintexts go straight from the caller's memory: the
    // pinned staging of the small uploads would keep a copy of them.
    if (mk.secret)
      HIPCHK(c, hipMemcpyAsync(w.F, in, cnt * mk.mlen, hipMemcpyHostToDevice, st));
    else
      HIPCHK(c, h2d(c, w.F, in, cnt * mk.mlen));
    d_in = (const uint8_t*)w.F;
  }
  blsk::launch_tmask(w.HQ, flag, good, cnt, d_in, d_out, mk.mlen, st);
  return BLSV_OK;
}

hipError_t mask_wipe(blsv_ctx* c, const MaskTail& mk, size_t cnt, hipStream_t st) {
  if (!mk.mlen || !mk.secret) return hipSuccess;
  const Staging w = staging(c);
  hipError_t e = hipMemsetAsync(w.HQ, 0, cnt * BLSV_GT_LEN, st);  // the capture: 144 words per item
  if (mk.host) {
    const hipError_t e2 = hipMemsetAsync(w.F, 0, cnt * mk.mlen, st);
    if (e == hipSuccess) e = e2;
  }
  return e;
}
