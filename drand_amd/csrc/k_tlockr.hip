// Timelock opening across many rounds (tlockr.h, include/blsverify.h "timelock"): E_i = e(U_i, sigma_j)^3
// where round j owns a run of consecutive items. k_tlock_prepare_many walks the 68 Miller steps of every
// signature of a pass, one lane each, into a word-major table; k_tlockr_f folds them into f, one one-wave
// workgroup per host-built tile, in two forms that share tlockr_f: a uniform tile copies its one
// signature's column to LDS and reads it by broadcast (k_tlock_f's way), a mixed tile's lanes read their
// own signature's column from global memory at each use. F is written in the pipeline's SoA layout, so
// launch_final_exp with its capture output and launch_tlock_encode run unchanged behind them.
// k_tlock.hip is not touched: the one-signature kernels compile to what they compiled to before.
#include "kcommon.h"
#include "tlockr.h"

namespace blsk {

static_assert(kTlockTabWords == (size_t)TLOCK_TAB_WORDS, "kernels.h and tlock.h agree on the table");
static_assert(kTlockTileMixed == 0xffffffffu && kTlockTileWords == 3, "a tile is (first, len, sig)");

// ------------------------------------------------------------------ prepare (one lane per signature)
// S / s_inf / s_cls: the staging launch_decompress_g2 filled for the pass's M signatures (stride M). Lane
// j writes word w of its table to tab[w * M + j]. A sigma that does not decode or is the point at
// infinity writes nothing: the f pass reads no word of its column. prepared counts the sigmas that decoded.
__global__ void __launch_bounds__(TPB) k_tlock_prepare_many(const uint32_t* S, const uint8_t* s_inf, const uint8_t* s_cls,
                                                            size_t M, uint32_t* tab, unsigned long long* prepared) {
  const size_t j = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (j >= M) return;
  if (s_cls[j] != REJ_OK) return;
  atomicAdd(prepared, 1ull);
  if (s_inf[j]) return;
  const g2a Q = {ld_fp2(S, M, j, 0), ld_fp2(S, M, j, 2)};
  tlockr_prepare(Q, [&](int w, uint32_t v) { tab[tlockr_tab_at(w, M, j)] = v; });
}

// ------------------------------------------------------------------ f pass (one workgroup per tile)
#ifndef BLS_WPE_TLOCKR_F
#define BLS_WPE_TLOCKR_F 1
#endif

// A uniform tile's table column: one LDS copy per workgroup, read by broadcast. Only the uniform
// instantiation names it, so the mixed one does not carry it.
static __shared__ uint32_t g_tr_tab[TLOCK_TAB_WORDS];
// The two U-dependent line slots (c1 xU, c2 yU) of the current step park in LDS in both forms, one
// 48-word column per lane (12 KB per workgroup).
static __shared__ uint32_t g_tr_L[48 * BLS_LANES];
// 512 VGPRs per lane leave one wave per SIMD, four one-wave workgroups per CU, in both forms; the uniform
// form's 38,784 bytes of LDS as compiled (k_tlock_f's figure; the mixed form's 19,200) fit four times into
// the CU's 160 KB.
static_assert(sizeof(uint32_t) * (TLOCK_TAB_WORDS + 48 * BLS_LANES + 24 * BLS_LANES + 16 * 12) <= 40960,
              "k_tlockr_f: four one-wave workgroups per CU share its 160 KB of LDS");
static_assert(BLS_LANES == TPB, "the parked columns are indexed by threadIdx.x");

DI void tr_park(int c, const fp2& v) {  // c = 1, 2
  const unsigned l = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    g_tr_L[((c - 1) * 24 + k) * BLS_LANES + l] = v.c0.l[k];
    g_tr_L[((c - 1) * 24 + 12 + k) * BLS_LANES + l] = v.c1.l[k];
  }
}
DI fp2 tr_parked(int c) {
  unsigned l = threadIdx.x;
  asm volatile("" : "+v"(l));
  fp2 v;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    v.c0.l[k] = g_tr_L[((c - 1) * 24 + k) * BLS_LANES + l];
    v.c1.l[k] = g_tr_L[((c - 1) * 24 + 12 + k) * BLS_LANES + l];
  }
  return v;
}

// tiles: kTlockTileWords words each, (first item, length <= 64, signature) with the signature an index
// below M, or kTlockTileMixed in the MIXED instantiation, whose lanes take theirs from sig_of[item].
// tab / sig_inf / sig_cls: the pass's M prepared signatures. U / u_inf / cls: as launch_decompress_g1
// wrote them for cnt items. An item with cls != 0 is skipped; an item whose signature was rejected takes
// class REJ_TLOCK_SIG and is skipped; a pair with a point at infinity gets F = 1.
template <bool MIXED>
BLS_KERNEL(BLS_WPE_TLOCKR_F)
k_tlockr_f(const uint32_t* tiles, const uint32_t* sig_of, const uint32_t* tab, size_t M, const uint8_t* sig_inf,
           const uint8_t* sig_cls, const uint32_t* U, const uint8_t* u_inf, uint8_t* cls, size_t cnt, uint32_t* F) {
  const uint32_t* tile = tiles + (size_t)blockIdx.x * kTlockTileWords;
  const size_t i = (size_t)tile[0] + threadIdx.x;
  const bool live = threadIdx.x < tile[1] && i < cnt;
  const size_t j = MIXED ? (live ? sig_of[i] : 0) : tile[2];
  const bool known = j < M;  // always, by the host's plan; a lane outside it reads and writes nothing
  // before the early exits: every lane of the workgroup copies its share of the tables
  if (!MIXED && known)
    for (unsigned w = threadIdx.x; w < (unsigned)TLOCK_TAB_WORDS; w += TPB) g_tr_tab[w] = tab[tlockr_tab_at(w, M, j)];
#if BLS_F6_LIN
  kp_lds_init<16>();  // ends with the barrier that also covers g_tr_tab
#else
  __syncthreads();
#endif
  if (!live || !known) return;
  if (cls[i] != REJ_OK) return;
  if (sig_cls[j] != REJ_OK) {
    cls[i] = REJ_TLOCK_SIG;
    return;
  }
  if (u_inf[i] | sig_inf[j]) {
    st_fp12(F, cnt, i, fp12_one());
    return;
  }
  auto ucoord = [&](int c) {  // U is read at its use
    size_t o = i * G1_WORDS + 12 * c;
    asm volatile("" : "+v"(o));
    fp v;
#pragma unroll
    for (int w = 0; w < 12; w++) v.l[w] = U[o + w];
    return v;
  };
  auto coef = [&](int step, int c) {  // read at the use, never kept live
    fp2 v;
    if (MIXED) {
      size_t o = tlockr_tab_at(tlockr_coef_word(step, c), M, j);
      asm volatile("" : "+v"(o));
#pragma unroll
      for (int k = 0; k < 12; k++) {
        v.c0.l[k] = tab[o + (size_t)k * M];
        v.c1.l[k] = tab[o + (size_t)(12 + k) * M];
      }
    } else {
      int o = tlockr_coef_word(step, c);
      asm volatile("" : "+s"(o));
#pragma unroll
      for (int k = 0; k < 12; k++) {
        v.c0.l[k] = g_tr_tab[o + k];
        v.c1.l[k] = g_tr_tab[o + 12 + k];
      }
    }
    return v;
  };
#if BLS_F6_LIN
  auto sqr = [](const fp12& f) { return fp12_sqr_lin(f, KpLdsK<16>()); };
#else
  auto sqr = [](const fp12& f) { return fp12_sqr(f); };
#endif
  st_fp12(F, cnt, i, tlockr_f(coef, ucoord, tr_park, tr_parked, sqr));
}

// ------------------------------------------------------------------ classes of the pass's signatures
// dst[sig_j[k]] = src[k]: the pass's list is in the call's order but skips the rounds without items
__global__ void __launch_bounds__(TPB) k_tlock_scatter_classes(const uint8_t* src, const uint32_t* sig_j, size_t M,
                                                               uint8_t* dst) {
  const size_t k = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (k < M) dst[sig_j[k]] = src[k];
}

// ------------------------------------------------------------------ launchers
void launch_tlock_prepare_many(const uint32_t* S, const uint8_t* s_inf, const uint8_t* s_cls, size_t M, uint32_t* tab,
                               unsigned long long* prepared, hipStream_t st) {
  if (!M) return;
  hipLaunchKernelGGL(k_tlock_prepare_many, dim3(grid_for(M)), dim3(TPB), 0, st, S, s_inf, s_cls, M, tab, prepared);
}

void launch_tlock_f_tiles(const uint32_t* tiles, size_t n_uniform, size_t n_mixed, const uint32_t* sig_of,
                          const uint32_t* tab, size_t M, const uint8_t* sig_inf, const uint8_t* sig_cls,
                          const uint32_t* U, const uint8_t* u_inf, uint8_t* cls, size_t cnt, uint32_t* F,
                          hipStream_t st) {
  if (n_uniform)
    hipLaunchKernelGGL(k_tlockr_f<false>, dim3((unsigned)n_uniform), dim3(TPB), 0, st, tiles, sig_of, tab, M, sig_inf,
                       sig_cls, U, u_inf, cls, cnt, F);
  if (n_mixed)
    hipLaunchKernelGGL(k_tlockr_f<true>, dim3((unsigned)n_mixed), dim3(TPB), 0, st, tiles + n_uniform * kTlockTileWords,
                       sig_of, tab, M, sig_inf, sig_cls, U, u_inf, cls, cnt, F);
}

void launch_tlock_scatter_classes(const uint8_t* src, const uint32_t* sig_j, size_t M, uint8_t* dst, hipStream_t st) {
  if (!M) return;
  hipLaunchKernelGGL(k_tlock_scatter_classes, dim3(grid_for(M)), dim3(TPB), 0, st, src, sig_j, M, dst);
}

}  // namespace blsk
