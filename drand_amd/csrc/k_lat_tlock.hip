// Timelock opening on the latency path: one workgroup of eight waves opens one ciphertext end to end
// (wvteam.h tlock_team: both decodes with their subgroup checks, the one pair's Miller loop, the final
// exponentiation and the Gt encoding), E_i = e(U_i, sigma)^3 as the batch kernels of k_tlock.hip /
// k_tlockr.hip compute it, byte for byte. For calls of a few items (tlock.cpp routes calls of up to
// blsv_set_tlock_lat_max items here), where the batch path's one-lane stages leave the chip idle.
// The phase trace (WV_MARK) belongs to k_lat.hip's verification launches: this unit compiles it out.
#define WV_WAVES 8
#define WV_NO_TRACE
#include "kcommon.h"
#include "wvteam.h"

namespace wv {
static_assert(TEAM_WAVES == WV_WAVES, "one wave of the workgroup per team member");
}

namespace blsk {

// Workgroup i < n_items opens item i: U at us + 48 i under the signature sig_of[i] (0 without the table),
// its 576 bytes to out (4-byte aligned; zeros for a rejected item) and its class to cls[i]. Items that
// share a signature each decode it again, beside their U decode, and each write its class to
// sig_cls[j]: the same byte. Workgroup n_items + k classes the signature idle[k], which has no item.
__global__ void __launch_bounds__(64 * WV_WAVES) k_lat_tlock(const uint8_t* sigs, const uint32_t* sig_of,
                                                            const uint8_t* us, size_t n_items, const uint32_t* idle,
                                                            size_t n_idle, uint8_t* out, uint8_t* cls,
                                                            uint8_t* sig_cls) {
  const size_t i = blockIdx.x;
  if (i >= n_items + n_idle) return;
  wv::team_init();
  wv::wv_init();
  __syncthreads();
  if (i < n_items) {
    const size_t j = sig_of ? sig_of[i] : 0;
    uint8_t sc = 0;
    const uint8_t c = wv::tlock_team(sigs + 96 * j, us + 48 * i, (uint32_t*)(out + 576 * i), sc);
    if (threadIdx.x == 0) {
      cls[i] = c;
      sig_cls[j] = sc;
    }
  } else {
    const size_t j = idle[i - n_items];
    const uint8_t sc = wv::sig_class_team(sigs + 96 * j);
    if (threadIdx.x == 0) sig_cls[j] = sc;
  }
}

void launch_lat_tlock(const uint8_t* sigs, const uint32_t* sig_of, const uint8_t* us, size_t n_items,
                      const uint32_t* idle, size_t n_idle, uint8_t* out, uint8_t* cls, uint8_t* sig_cls,
                      hipStream_t st) {
  if (!(n_items + n_idle)) return;
  hipLaunchKernelGGL(k_lat_tlock, dim3((unsigned)(n_items + n_idle)), dim3(64 * WV_WAVES), 0, st, sigs, sig_of, us,
                     n_items, idle, n_idle, out, cls, sig_cls);
}

}  // namespace blsk
