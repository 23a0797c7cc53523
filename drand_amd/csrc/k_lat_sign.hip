// Signing on the latency path: one workgroup of eight waves signs one message end to end (wsign.h
// sign_team: the hash of the message, H to affine, the four 64-bit ladders of the key's digits in base |x|
// on four waves, their sum, the conversion and the compression), sigma = compress([sk] H(m)) as the batch
// kernel of k_sign.hip computes it, byte for byte. For calls of a few messages (threshold.cpp routes
// blsv_sign calls of up to blsv_set_sign_lat_max messages here), where the batch path's one lane per
// message leaves the chip idle. A unit of its own, so that k_lat.hip and the other latency units compile to
// what they compiled to before; the phase trace (WV_MARK) belongs to k_lat.hip's launches and is compiled
// out here.
#define WV_WAVES 8
#define WV_NO_TRACE
#include "kcommon.h"
#include "wsign.h"

namespace wv {
static_assert(TEAM_WAVES == WV_WAVES, "one wave of the workgroup per team member");
}

namespace blsk {

__constant__ uint8_t c_sign_dst[DST_LEN] = {66, 76, 83, 95, 83, 73, 71, 95, 66, 76, 83, 49, 50, 51, 56, 49, 71, 50, 95, 88,
                                            77, 68, 58, 83, 72, 65, 45, 50, 53, 54, 95, 83, 83, 87, 85, 95, 82, 79, 95,
                                            78, 85, 76, 95};

// Workgroup i < n signs message i, the len[i] bytes at msgs + off[i] (k_lat_messages's form), with the key
// sk_words (eight little-endian words, reduced mod r): 24 words to out + 24 i. No share index is written:
// the host puts it in front of each signature as it copies out.
__global__ void __launch_bounds__(64 * WV_WAVES) k_lat_sign(const uint32_t* sk_words, const uint8_t* msgs,
                                                           const uint64_t* off, const uint32_t* len, size_t n,
                                                           uint32_t* out) {
  const size_t i = blockIdx.x;
  if (i >= n) return;
  wv::team_init();
  wv::wv_init();
  __syncthreads();
  uint32_t b0[8];
  xmd_b0_bytes<true>(b0, msgs + off[i], len[i], c_sign_dst);
  wv::sign_team(b0, sk_words, out + 24 * i);
}

void launch_lat_sign(const uint32_t* sk_words, const uint8_t* msgs, const uint64_t* off, const uint32_t* len, size_t n,
                     uint32_t* out, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_lat_sign, dim3((unsigned)n), dim3(64 * WV_WAVES), 0, st, sk_words, msgs, off, len, n, out);
}

}  // namespace blsk
