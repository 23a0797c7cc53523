// Timelock sealing (tseal.h, include/blsverify.h "timelock"): U_i = k_i G1 and K_i = B^k_i for one
// shared base B = e(pk, H(MessageV2(round)))^3. k_tseal_g1_table fills T1 once per context and
// k_tseal_gt_table T2 once per base; k_tseal_u and k_tseal_gt walk them, one lane per item, by the
// four-bit digits of k_i. K is written in the pipeline's SoA layout so that launch_tlock_encode turns it
// into the 576-byte Gt encoding unchanged. Both tables stay in global memory (645 KB together: they sit
// in L2); a lane's entry depends on its own digits, so the reads are gathers of whole 96- / 576-byte
// entries.
// The producing side of timelock.Encrypt's two group operations, as core/timelock_test.go calls it.
#include "kcommon.h"
#include "tseal.h"

namespace blsk {

static_assert(kTsealT1Words == (size_t)TSEAL_T1_WORDS && kTsealT2Words == (size_t)TSEAL_T2_WORDS, "kernels.h table sizes");
static_assert(TSEAL_WINDOWS == TPB, "the table kernels give every window a lane of one wave");

DI fp ld_words(const uint32_t* p) {
  fp v;
#pragma unroll
  for (int w = 0; w < 12; w++) v.l[w] = p[w];
  return v;
}
DI void st_words(uint32_t* p, const fp& v) {
#pragma unroll
  for (int w = 0; w < 12; w++) p[w] = v.l[w];
}
DI fp2 ld_words2(const uint32_t* p) { return {ld_words(p), ld_words(p + 12)}; }
DI fp6 ld_words6(const uint32_t* p) { return {ld_words2(p), ld_words2(p + 24), ld_words2(p + 48)}; }
DI fp12 ld_words12(const uint32_t* p) { return {ld_words6(p), ld_words6(p + 72)}; }
DI void st_words12(uint32_t* p, const fp12& v) {
  const fp2* c[6] = {&v.c0.c0, &v.c0.c1, &v.c0.c2, &v.c1.c0, &v.c1.c1, &v.c1.c2};
#pragma unroll
  for (int k = 0; k < 6; k++) {
    st_words(p + 24 * k, c[k]->c0);
    st_words(p + 24 * k + 12, c[k]->c1);
  }
}

// ------------------------------------------------------------------ T1 (once per context)
// One wave: lane w fills row w.
__global__ void __launch_bounds__(TPB) k_tseal_g1_table(uint32_t* T1) {
  const int w = (int)threadIdx.x;
  if (blockIdx.x != 0) return;
  tseal_g1_row(w, [&](int j, const g1a& p) {
    uint32_t* o = T1 + (size_t)tseal_entry(w, j) * TSEAL_G1_WORDS;
    st_words(o, p.x);
    st_words(o + 12, p.y);
  });
}

// ------------------------------------------------------------------ T2 (once per base)
// B: the captured final-exponentiation value of the one-item base pass (SoA of stride 1: the Fp12's 144
// words in tower order). One wave: lane 0 walks the chain of 252 cyclotomic squarings and leaves
// T2[w][1]; after the barrier lane w multiplies row w up.
__global__ void __launch_bounds__(TPB) k_tseal_gt_table(const uint32_t* B, uint32_t* T2) {
  const int w = (int)threadIdx.x;
  if (blockIdx.x != 0) return;
  if (w == 0)
    tseal_gt_chain(ld_words12(B), [&](int ww, const fp12& v) {
      st_words12(T2 + (size_t)tseal_entry(ww, 1) * TSEAL_GT_WORDS, v);
    });
  __threadfence_block();
  __syncthreads();
  tseal_gt_row(ld_words12(T2 + (size_t)tseal_entry(w, 1) * TSEAL_GT_WORDS), [&](int j, const fp12& v) {
    st_words12(T2 + (size_t)tseal_entry(w, j) * TSEAL_GT_WORDS, v);
  });
}

// ------------------------------------------------------------------ U (one lane per item)
#ifndef BLS_WPE_TSEAL_U
#define BLS_WPE_TSEAL_U 2
#endif
// scalars: cnt x 32 bytes big-endian. us: cnt x 48 bytes, ok / cls: one byte per item. An item with
// k == 0 (mod r) gets 48 zero bytes, ok = 0 and cls = TSEAL_REFUSED (k_tseal_gt and the encoding skip it).
BLS_KERNEL(BLS_WPE_TSEAL_U)
k_tseal_u(const uint32_t* T1, const uint8_t* scalars, size_t cnt, uint8_t* us, uint8_t* ok, uint8_t* cls) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  uint32_t k[8];
  const bool sealed = tseal_scalar(scalars + i * TSEAL_SCALAR_LEN, k);
  ok[i] = sealed ? 1 : 0;
  cls[i] = sealed ? (uint8_t)REJ_OK : TSEAL_REFUSED;
  uint8_t* o = us + i * 48;
  if (!sealed) {
    for (int b = 0; b < 48; b++) o[b] = 0;
    return;
  }
  const g1j u = tseal_u(k, [&](int w, int j) {
    const uint32_t* e = T1 + (size_t)tseal_entry(w, j) * TSEAL_G1_WORDS;
    return g1a{ld_words(e), ld_words(e + 12)};
  });
  uint8_t buf[48];
  g1_compress(buf, u);
  for (int b = 0; b < 48; b++) o[b] = buf[b];
}

// ------------------------------------------------------------------ K (one lane per item)
#ifndef BLS_WPE_TSEAL_GT
#define BLS_WPE_TSEAL_GT 1
#endif
// The accumulator alone stays in registers: the table entry is fetched by Fp6 halves at their uses
// (tseal_mul_halves), its address opaque so that no half is kept live across a product. E: SoA of
// stride cnt (what launch_tlock_encode reads); an item whose class is not 0 is left untouched.
BLS_KERNEL(BLS_WPE_TSEAL_GT)
k_tseal_gt(const uint32_t* T2, const uint8_t* scalars, const uint8_t* cls, size_t cnt, uint32_t* E) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  if (cls[i] != REJ_OK) return;
  uint32_t k[8];
  (void)tseal_scalar(scalars + i * TSEAL_SCALAR_LEN, k);
  const fp12 acc = tseal_gt(k, [&](int w, int j, int h) {
    uint32_t o = (uint32_t)(tseal_entry(w, j) * TSEAL_GT_WORDS + 72 * h);
    asm volatile("" : "+v"(o));  // read at the use, never kept live
    return ld_words6(T2 + o);
  });
  st_fp12(E, cnt, i, acc);
}

// ------------------------------------------------------------------ launchers
void launch_tseal_g1_table(uint32_t* T1, hipStream_t st) {
  hipLaunchKernelGGL(k_tseal_g1_table, dim3(1), dim3(TPB), 0, st, T1);
}

void launch_tseal_gt_table(const uint32_t* B, uint32_t* T2, hipStream_t st) {
  hipLaunchKernelGGL(k_tseal_gt_table, dim3(1), dim3(TPB), 0, st, B, T2);
}

void launch_tseal_u(const uint32_t* T1, const uint8_t* scalars, size_t cnt, uint8_t* us, uint8_t* ok, uint8_t* cls,
                    hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_tseal_u, dim3(grid_for(cnt)), dim3(TPB), 0, st, T1, scalars, cnt, us, ok, cls);
}

void launch_tseal_gt(const uint32_t* T2, const uint8_t* scalars, const uint8_t* cls, size_t cnt, uint32_t* E,
                     hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_tseal_gt, dim3(grid_for(cnt)), dim3(TPB), 0, st, T2, scalars, cls, cnt, E);
}

}  // namespace blsk
