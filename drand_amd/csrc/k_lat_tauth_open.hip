// Authenticated timelock opening on the latency path: one workgroup of eight waves opens one ciphertext
// (U, V, W) end to end (wauth.h auth_open_team: tlock_team's decodes, Miller loop and final exponentiation,
// then s' = V XOR H2(E), k' = H3(s', W XOR H4(s')), the walk k' G1 shared out over the waves, the comparison
// with the decoded U, and only then the store), byte for byte and class for class what the batch path's
// k_tauth_open_tail gives. For calls of a few items (tauth_lat.cpp routes the host forms' calls of up to
// blsv_set_tauth_lat_max items here). A unit of its own, so that the other latency kernels compile to what
// they compiled to before; the phase trace (WV_MARK) belongs to k_lat.hip's launches and is compiled out.
#define WV_WAVES 8
#define WV_NO_TRACE
#include "kcommon.h"
#include "wauth.h"

namespace wv {
static_assert(TEAM_WAVES == WV_WAVES, "one wave of the workgroup per team member");
}

namespace blsk {

static_assert(TSEAL_WINDOWS * TSEAL_ENTRIES * 24 == (int)kTsealT1Words, "wauth.h walks a table of T1's layout");

// k_lat_tlock's item shape: workgroup i < n_items opens item i -- U at us + 48 i, V at vs + 32 i, W at
// ws + mlen i -- under the signature sig_of[i] (0 without the table): its mlen message bytes to out + mlen i
// (zeros unless its class is 0) and its class to cls[i]. Items that share a signature each decode it again
// and each write its class to sig_cls[j]: the same byte. Workgroup n_items + k classes the signature
// idle[k], which has no item. walk_waves: the waves that share the check's walk, 8 or 1 (wauth.h).
// offs != nullptr (blsv_tlock_decrypt_auth*_var): item i's W and message bytes lie at offs[i] .. offs[i + 1] of
// ws and out instead, n_items + 1 prefix offsets; the length is one per workgroup either way.
__global__ void __launch_bounds__(64 * WV_WAVES) k_lat_tauth_open(const uint8_t* sigs, const uint32_t* sig_of,
                                                                 const uint8_t* us, const uint8_t* vs, const uint8_t* ws,
                                                                 uint32_t mlen, size_t n_items, const uint32_t* idle,
                                                                 size_t n_idle, const uint32_t* T1, uint8_t* out,
                                                                 uint8_t* cls, uint8_t* sig_cls, int walk_waves,
                                                                 const uint32_t* offs) {
  const size_t i = blockIdx.x;
  if (i >= n_items + n_idle) return;
  wv::team_init();
  wv::wv_init();
  __syncthreads();
  if (i < n_items) {
    const size_t j = sig_of ? sig_of[i] : 0;
    uint8_t sc = 0;
    const size_t off = offs ? (size_t)offs[i] : (size_t)mlen * i;
    if (offs) mlen = offs[i + 1] - offs[i];
    const uint8_t c = wv::auth_open_team(sigs + 96 * j, us + 48 * i, vs + TAUTH_V_LEN * i, ws + off, mlen, T1, out + off, sc,
                                         walk_waves);
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

void launch_lat_tauth_open(const uint8_t* sigs, const uint32_t* sig_of, const uint8_t* us, const uint8_t* vs,
                           const uint8_t* ws, size_t mlen, size_t n_items, const uint32_t* idle, size_t n_idle,
                           const uint32_t* T1, uint8_t* out, uint8_t* cls, uint8_t* sig_cls, int walk_waves,
                           hipStream_t st, const uint32_t* offs) {
  if (!(n_items + n_idle)) return;
  hipLaunchKernelGGL(k_lat_tauth_open, dim3((unsigned)(n_items + n_idle)), dim3(64 * WV_WAVES), 0, st, sigs, sig_of, us, vs,
                     ws, (uint32_t)mlen, n_items, idle, n_idle, T1, out, cls, sig_cls, walk_waves == 1 ? 1 : 8, offs);
}

}  // namespace blsk
