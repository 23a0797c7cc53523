// Timelock encrypt / decrypt, the fused tail of the four timelock passes and of the two latency kernels
// (tmask.h, include/blsverify.h "timelock in one call"): one lane per item derives the item's key stream
// from its Gt value and XORs it over the item's mlen message bytes. The batch form reads the value from
// the final exponentiation's SoA capture, so the 576 encoded bytes are never stored; the latency form
// reads the bytes k_lat_tlock / k_lat_tseal wrote.
#include "kcommon.h"
#include "tmask.h"

namespace blsk {

static_assert(kTmaskMsgMax == (size_t)TMASK_MSG_MAX && TMASK_GT_LEN == 4 * F_WORDS, "kernels.h states tmask.h's sizes");

// ENC == false: src is the SoA capture of stride cnt (Montgomery form). ENC == true: src is cnt x 144 words,
// the encoded bytes. flag[i] == good marks an item with a value (class bytes: good = 0, ok bytes: good = 1);
// any other item gets mlen zero bytes. in / out: cnt x mlen packed bytes (WORDS: both 4-byte aligned and
// mlen a multiple of 4); out == in is allowed, as is any other pair that does not overlap.
// Only the occupancy the registers allow is asked for (8 words of state, 16 of schedule, 12 of Fp and the
// midstate: no scratch, DESIGN.md 8.7 quotes the figures).
template <bool ENC, bool WORDS>
__global__ void __launch_bounds__(TPB) k_tmask(const uint32_t* src, const uint8_t* flag, uint8_t good, size_t cnt,
                                               const uint8_t* in, uint8_t* out, uint32_t mlen) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  const bool has = flag[i] == good;
  uint32_t mid[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (has) {
    if constexpr (ENC)
      tmask_midstate(mid, [&](int k) { return tmask_coef_enc(src + i * (TMASK_GT_LEN / 4), k); });
    else
      tmask_midstate(mid, [&](int k) { return tmask_coef_soa(src, cnt, i, k); });
  }
  tmask_apply<WORDS>(mid, has, in + i * mlen, out + i * mlen, mlen);
}

template <bool ENC>
static void launch_tmask_form(const uint32_t* src, const uint8_t* flag, uint8_t good, size_t cnt, const uint8_t* in,
                              uint8_t* out, size_t mlen, hipStream_t st) {
  const bool words = (((uintptr_t)in | (uintptr_t)out | mlen) & 3) == 0;
  if (words)
    hipLaunchKernelGGL((k_tmask<ENC, true>), dim3(grid_for(cnt)), dim3(TPB), 0, st, src, flag, good, cnt, in, out,
                       (uint32_t)mlen);
  else
    hipLaunchKernelGGL((k_tmask<ENC, false>), dim3(grid_for(cnt)), dim3(TPB), 0, st, src, flag, good, cnt, in, out,
                       (uint32_t)mlen);
}

void launch_tmask(const uint32_t* E, const uint8_t* flag, uint8_t good, size_t cnt, const uint8_t* in, uint8_t* out,
                  size_t mlen, hipStream_t st) {
  if (!cnt || !mlen || mlen > (size_t)TMASK_MSG_MAX) return;
  launch_tmask_form<false>(E, flag, good, cnt, in, out, mlen, st);
}

void launch_tmask_encoded(const uint8_t* gt576, const uint8_t* flag, uint8_t good, size_t cnt, const uint8_t* in,
                          uint8_t* out, size_t mlen, hipStream_t st) {
  if (!cnt || !mlen || mlen > (size_t)TMASK_MSG_MAX) return;
  launch_tmask_form<true>((const uint32_t*)gt576, flag, good, cnt, in, out, mlen, st);
}

}  // namespace blsk
