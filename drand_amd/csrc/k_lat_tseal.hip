// Timelock sealing on the latency path: one workgroup of eight waves seals one message end to end
// (wseal.h seal_team: the hash of the item's round beside the two table walks U = k G1 and P = k pk, the
// one pair's Miller loop, the final exponentiation and the Gt encoding), K = e(k pk, H(MessageV2(round)))^3
// as the batch kernels of k_tseal.hip / k_tsealr.hip compute it, byte for byte. For calls of a few items
// (tseal.cpp / tsealr.cpp route calls of up to blsv_set_tseal_lat_max items here), where the batch path's
// one-lane stages leave the chip idle. A unit of its own, so that k_lat.hip and k_lat_tlock.hip compile to
// what they compiled to before; the phase trace (WV_MARK) belongs to k_lat.hip's launches and is compiled
// out here.
#define WV_WAVES 8
#define WV_NO_TRACE
#include "kcommon.h"
#include "wseal.h"

namespace wv {
static_assert(TEAM_WAVES == WV_WAVES, "one wave of the workgroup per team member");
}

namespace blsk {

static_assert(TSEAL_WINDOWS * TSEAL_ENTRIES * 24 == (int)kTsealT1Words, "wseal.h walks tables of T1's layout");

// Workgroup i < n seals item i: the scalar at scalars + 32 i to the round rounds[i] (the one round
// `round` without the array), U to us + 48 i and K to gts + 576 i (both 4-byte aligned), ok[i]; zeros
// and ok = 0 for a refused scalar. Items that share a round each hash it again.
__global__ void __launch_bounds__(64 * WV_WAVES) k_lat_tseal(const uint32_t* T1, const uint32_t* TK,
                                                            const uint64_t* rounds, uint64_t round,
                                                            const uint8_t* scalars, size_t n, uint8_t* us,
                                                            uint8_t* gts, uint8_t* ok) {
  const size_t i = blockIdx.x;
  if (i >= n) return;
  wv::team_init();
  wv::wv_init();
  __syncthreads();
  uint32_t msg[8], b0[8];
  drand_message_v2<true>(msg, rounds ? rounds[i] : round);
  wv::xmd_b0_msg32(msg, b0);
  const bool sealed = wv::seal_team(scalars + TSEAL_SCALAR_LEN * i, b0, T1, TK, (uint32_t*)(us + 48 * i),
                                    (uint32_t*)(gts + 576 * i));
  if (threadIdx.x == 0) ok[i] = sealed ? 1 : 0;
}

void launch_lat_tseal(const uint32_t* T1, const uint32_t* TK, const uint64_t* rounds, uint64_t round,
                      const uint8_t* scalars, size_t n, uint8_t* us, uint8_t* gts, uint8_t* ok, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_lat_tseal, dim3((unsigned)n), dim3(64 * WV_WAVES), 0, st, T1, TK, rounds, round, scalars, n, us,
                     gts, ok);
}

}  // namespace blsk
