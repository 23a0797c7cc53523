// Authenticated timelock sealing on the latency path: one workgroup of eight waves seals one message end
// to end (wauth.h auth_seal_team: k = H3(seed, M) derived by every wave, seal_team's hash, walks, Miller loop
// and final exponentiation, then V = seed XOR H2(K) and W = M XOR H4(seed)), byte for byte what the batch
// path's k_tauth_derive / sealing kernels / k_tauth_seal_tail give. K is never encoded and never leaves the
// workgroup, and the scalar sits neither in LDS nor in global memory. For calls of a few items
// (tauth_lat.cpp routes the host forms' calls of up to blsv_set_tauth_lat_max items here). A unit of its
// own, so that the other latency kernels compile to what they compiled to before; the phase trace (WV_MARK)
// belongs to k_lat.hip's launches and is compiled out.
#define WV_WAVES 8
#define WV_NO_TRACE
#include "kcommon.h"
#include "wauth.h"

namespace wv {
static_assert(TEAM_WAVES == WV_WAVES, "one wave of the workgroup per team member");
}

namespace blsk {

static_assert(TSEAL_WINDOWS * TSEAL_ENTRIES * 24 == (int)kTsealT1Words, "wseal.h walks tables of T1's layout");

// Workgroup i < n seals item i: the seed at seeds + 32 i and the mlen message bytes at msgs + mlen i to the
// round rounds[i] (the one round `round` without the array): U to us + 48 i (4-byte aligned), V to
// vs + 32 i, W to ws + mlen i, ok[i]; zeros and ok = 0 for a derived scalar of zero. Items that share a
// round each hash it again. offs != nullptr (blsv_tlock_encrypt_auth*_var): item i's message and W bytes lie at
// offs[i] .. offs[i + 1] of msgs and ws instead, n + 1 prefix offsets; the length is one per workgroup either way.
__global__ void __launch_bounds__(64 * WV_WAVES) k_lat_tauth_seal(const uint32_t* T1, const uint32_t* TK,
                                                                 const uint64_t* rounds, uint64_t round,
                                                                 const uint8_t* seeds, const uint8_t* msgs, uint32_t mlen,
                                                                 size_t n, uint8_t* us, uint8_t* vs, uint8_t* ws,
                                                                 uint8_t* ok, const uint32_t* offs) {
  const size_t i = blockIdx.x;
  if (i >= n) return;
  wv::team_init();
  wv::wv_init();
  __syncthreads();
  uint32_t msg[8], b0[8];
  drand_message_v2<true>(msg, rounds ? rounds[i] : round);
  wv::xmd_b0_msg32(msg, b0);
  const size_t off = offs ? (size_t)offs[i] : (size_t)mlen * i;
  if (offs) mlen = offs[i + 1] - offs[i];
  const bool sealed = wv::auth_seal_team(seeds + TAUTH_SEED_LEN * i, msgs + off, mlen, b0, T1, TK, (uint32_t*)(us + 48 * i),
                                         vs + TAUTH_V_LEN * i, ws + off);
  if (threadIdx.x == 0) ok[i] = sealed ? 1 : 0;
}

void launch_lat_tauth_seal(const uint32_t* T1, const uint32_t* TK, const uint64_t* rounds, uint64_t round,
                           const uint8_t* seeds, const uint8_t* msgs, size_t mlen, size_t n, uint8_t* us, uint8_t* vs,
                           uint8_t* ws, uint8_t* ok, hipStream_t st, const uint32_t* offs) {
  if (!n) return;
  hipLaunchKernelGGL(k_lat_tauth_seal, dim3((unsigned)n), dim3(64 * WV_WAVES), 0, st, T1, TK, rounds, round, seeds, msgs,
                     (uint32_t)mlen, n, us, vs, ws, ok, offs);
}

}  // namespace blsk
