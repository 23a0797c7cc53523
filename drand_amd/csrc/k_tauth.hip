// Authenticated timelock (tauth.h, include/blsverify.h "authenticated timelock"), one lane per item:
//   k_tauth_derive     encrypt, before the sealing kernels: seeds and messages -> the derived scalars, in the
//                      32-byte big-endian form k_tseal_u / k_tseal_gt / k_tsealr_point read (a derived zero is
//                      32 zero bytes, which k_tseal_u refuses as it refuses any zero scalar)
//   k_tauth_seal_tail  encrypt, where k_tmask runs: K from the final exponentiation's SoA capture -> V and W
//   k_tauth_open_tail  decrypt, where k_tmask runs: E from the capture, the decoded U table the pass left in
//                      its staging, V and W -> the verdict and, for a good item only, the message
// The 576 encoded bytes never leave the lane, and a failing item's candidate plaintext is never stored.
// Each kernel takes the items' spans as a functor (tauth.h): tauth_span_uniform for the entry points with one
// length per call, tauth_span_ragged (the launch_*_var forms) for blsv_tlock_*_auth*_var, where the lanes of a
// wave run 1 .. 8 pieces each. The piece loops are not unrolled, so a wave leaves them with its longest item.
#include "kcommon.h"
#include "tauth.h"

namespace blsk {

static_assert(kTauthSeedLen == (size_t)TAUTH_SEED_LEN && kTauthVLen == (size_t)TAUTH_V_LEN, "kernels.h states tauth.h's sizes");

// seeds: cnt x 32 bytes, msgs: the cnt items' packed bytes (WORDS: 4-byte aligned, and every offset and length
// a multiple of 4) -> scalars: cnt x 32 bytes
template <bool WORDS, typename Span>
__global__ void __launch_bounds__(TPB) k_tauth_derive(const uint8_t* seeds, const uint8_t* msgs, size_t cnt, Span sp,
                                                      uint8_t* scalars) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  uint32_t seed[8], k[8];
  tauth_seed_words(seed, seeds + i * TAUTH_SEED_LEN);
  (void)tauth_derive<WORDS>(seed, msgs + sp.off(i), sp.len(i), k);  // k == 0 stays 0: refused downstream
  uint8_t buf[32];
  tauth_scalar_bytes(buf, k);
  uint8_t* o = scalars + i * TSEAL_SCALAR_LEN;
  for (int b = 0; b < 32; b++) o[b] = buf[b];
}

// E: the SoA capture of stride cnt (Montgomery form); cls: the class bytes launch_tseal_u wrote (an item that
// is not 0 was refused: V and W get zeros). out_ws == msgs is allowed, as is any pair that does not overlap.
template <bool WORDS, typename Span>
__global__ void __launch_bounds__(TPB) k_tauth_seal_tail(const uint32_t* E, const uint8_t* cls, size_t cnt,
                                                         const uint8_t* seeds, const uint8_t* msgs, Span sp,
                                                         uint8_t* out_vs, uint8_t* out_ws) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  const bool sealed = cls[i] == REJ_OK;
  uint32_t mid[8] = {0, 0, 0, 0, 0, 0, 0, 0}, seed[8];
  if (sealed) tmask_midstate(mid, [&](int k) { return tmask_coef_soa(E, cnt, i, k); });
  tauth_seed_words(seed, seeds + i * TAUTH_SEED_LEN);
  tauth_seal_tail<WORDS>(mid, sealed, seed, msgs + sp.off(i), sp.len(i), out_vs + i * TAUTH_V_LEN, out_ws + sp.off(i));
}

#ifndef BLS_WPE_TAUTH_OPEN
#define BLS_WPE_TAUTH_OPEN 2
#endif
// E as above; U / u_inf: the AoS table launch_decompress_g1 wrote (G1_WORDS per item), intact behind the final
// exponentiation; cls: the pass's class bytes, read and -- for an item that fails the check -- written
// (REJ_TLOCK_AUTH); an item that arrives with a class keeps it and gets zeros. T1: tseal.h's table, whole
// 96-byte entries gathered by the lane's own digits, as in k_tseal_u. out == ws is allowed.
template <bool WORDS, typename Span>
BLS_KERNEL(BLS_WPE_TAUTH_OPEN)
k_tauth_open_tail(const uint32_t* E, const uint32_t* U, const uint8_t* u_inf, uint8_t* cls, size_t cnt, const uint32_t* T1,
                  const uint8_t* vs, const uint8_t* ws, Span sp, uint8_t* out) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  const uint32_t mlen = sp.len(i);
  uint8_t* o = out + sp.off(i);
  if (cls[i] != REJ_OK) {
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
    for (uint32_t j = 0; 32 * j < mlen; j++) tauth_store_piece<WORDS>(o, j, tauth_piece_len(mlen, j), zero, true);
    return;
  }
  auto words = [](const uint32_t* p) {
    fp v;
#pragma unroll
    for (int w = 0; w < 12; w++) v.l[w] = p[w];
    return v;
  };
  uint32_t mid[8];
  tmask_midstate(mid, [&](int k) { return tmask_coef_soa(E, cnt, i, k); });
  const uint8_t c = tauth_open_tail<WORDS>(
      mid, vs + i * TAUTH_V_LEN, ws + sp.off(i), mlen, [&](int c) { return words(U + i * G1_WORDS + 12 * c); }, u_inf[i] != 0,
      [&](int w, int j) {
        const uint32_t* e = T1 + (size_t)tseal_entry(w, j) * TSEAL_G1_WORDS;
        return g1a{words(e), words(e + 12)};
      },
      o);
  if (c != REJ_OK) cls[i] = c;  // TAUTH_REJ_AUTH
}

static bool all_words(const void* a, const void* b, size_t mlen) { return (((uintptr_t)a | (uintptr_t)b | mlen) & 3) == 0; }

void launch_tauth_derive(const uint8_t* seeds, const uint8_t* msgs, size_t cnt, size_t mlen, uint8_t* scalars,
                         hipStream_t st) {
  if (!cnt || !mlen || mlen > (size_t)TMASK_MSG_MAX) return;
  if (all_words(msgs, nullptr, mlen))
    hipLaunchKernelGGL((k_tauth_derive<true, tauth_span_uniform>), dim3(grid_for(cnt)), dim3(TPB), 0, st, seeds, msgs, cnt,
                       tauth_span_uniform{(uint32_t)mlen}, scalars);
  else
    hipLaunchKernelGGL((k_tauth_derive<false, tauth_span_uniform>), dim3(grid_for(cnt)), dim3(TPB), 0, st, seeds, msgs, cnt,
                       tauth_span_uniform{(uint32_t)mlen}, scalars);
}

void launch_tauth_seal_tail(const uint32_t* E, const uint8_t* cls, size_t cnt, const uint8_t* seeds, const uint8_t* msgs,
                            size_t mlen, uint8_t* out_vs, uint8_t* out_ws, hipStream_t st) {
  if (!cnt || !mlen || mlen > (size_t)TMASK_MSG_MAX) return;
  if (all_words(msgs, out_ws, mlen))
    hipLaunchKernelGGL((k_tauth_seal_tail<true, tauth_span_uniform>), dim3(grid_for(cnt)), dim3(TPB), 0, st, E, cls, cnt,
                       seeds, msgs, tauth_span_uniform{(uint32_t)mlen}, out_vs, out_ws);
  else
    hipLaunchKernelGGL((k_tauth_seal_tail<false, tauth_span_uniform>), dim3(grid_for(cnt)), dim3(TPB), 0, st, E, cls, cnt,
                       seeds, msgs, tauth_span_uniform{(uint32_t)mlen}, out_vs, out_ws);
}

void launch_tauth_open_tail(const uint32_t* E, const uint32_t* U, const uint8_t* u_inf, uint8_t* cls, size_t cnt,
                            const uint32_t* T1, const uint8_t* vs, const uint8_t* ws, size_t mlen, uint8_t* out,
                            hipStream_t st) {
  if (!cnt || !mlen || mlen > (size_t)TMASK_MSG_MAX) return;
  if (all_words(ws, out, mlen))
    hipLaunchKernelGGL((k_tauth_open_tail<true, tauth_span_uniform>), dim3(grid_for(cnt)), dim3(TPB), 0, st, E, U, u_inf,
                       cls, cnt, T1, vs, ws, tauth_span_uniform{(uint32_t)mlen}, out);
  else
    hipLaunchKernelGGL((k_tauth_open_tail<false, tauth_span_uniform>), dim3(grid_for(cnt)), dim3(TPB), 0, st, E, U, u_inf,
                       cls, cnt, T1, vs, ws, tauth_span_uniform{(uint32_t)mlen}, out);
}

// The ragged forms: offs = the pass's cnt + 1 prefix offsets on the device, words = every length of the pass is
// a multiple of 4 (the host knows: it built the table). The dword form runs only when the base pointers are
// 4-byte aligned too; otherwise bytes, never a word-granular read-modify-write of a neighbour's bytes.
void launch_tauth_derive_var(const uint8_t* seeds, const uint8_t* msgs, size_t cnt, const uint32_t* offs, bool words,
                             uint8_t* scalars, hipStream_t st) {
  if (!cnt) return;
  if (words && all_words(msgs, nullptr, 0))
    hipLaunchKernelGGL((k_tauth_derive<true, tauth_span_ragged>), dim3(grid_for(cnt)), dim3(TPB), 0, st, seeds, msgs, cnt,
                       tauth_span_ragged{offs}, scalars);
  else
    hipLaunchKernelGGL((k_tauth_derive<false, tauth_span_ragged>), dim3(grid_for(cnt)), dim3(TPB), 0, st, seeds, msgs, cnt,
                       tauth_span_ragged{offs}, scalars);
}

void launch_tauth_seal_tail_var(const uint32_t* E, const uint8_t* cls, size_t cnt, const uint8_t* seeds, const uint8_t* msgs,
                                const uint32_t* offs, bool words, uint8_t* out_vs, uint8_t* out_ws, hipStream_t st) {
  if (!cnt) return;
  if (words && all_words(msgs, out_ws, 0))
    hipLaunchKernelGGL((k_tauth_seal_tail<true, tauth_span_ragged>), dim3(grid_for(cnt)), dim3(TPB), 0, st, E, cls, cnt,
                       seeds, msgs, tauth_span_ragged{offs}, out_vs, out_ws);
  else
    hipLaunchKernelGGL((k_tauth_seal_tail<false, tauth_span_ragged>), dim3(grid_for(cnt)), dim3(TPB), 0, st, E, cls, cnt,
                       seeds, msgs, tauth_span_ragged{offs}, out_vs, out_ws);
}

void launch_tauth_open_tail_var(const uint32_t* E, const uint32_t* U, const uint8_t* u_inf, uint8_t* cls, size_t cnt,
                                const uint32_t* T1, const uint8_t* vs, const uint8_t* ws, const uint32_t* offs, bool words,
                                uint8_t* out, hipStream_t st) {
  if (!cnt) return;
  if (words && all_words(ws, out, 0))
    hipLaunchKernelGGL((k_tauth_open_tail<true, tauth_span_ragged>), dim3(grid_for(cnt)), dim3(TPB), 0, st, E, U, u_inf,
                       cls, cnt, T1, vs, ws, tauth_span_ragged{offs}, out);
  else
    hipLaunchKernelGGL((k_tauth_open_tail<false, tauth_span_ragged>), dim3(grid_for(cnt)), dim3(TPB), 0, st, E, U, u_inf,
                       cls, cnt, T1, vs, ws, tauth_span_ragged{offs}, out);
}

}  // namespace blsk
