// Timelock opening (tlock.h, include/blsverify.h "timelock"): E_i = e(U_i, sigma)^3 for one shared
// sigma. k_tlock_prepare walks sigma's 68 Miller steps once and leaves the P-independent line
// coefficients in a 19.6 KB table; k_tlock_f folds them into f, one lane per ciphertext, and writes F
// in the pipeline's SoA layout so that launch_final_exp runs unchanged; k_tlock_encode turns the
// captured Fp12 into the 576-byte Gt encoding.
// kilic Engine.AddPair(U, sigma) + Result [ext], as timelock.Decrypt calls it (core/timelock_test.go).
#include "kcommon.h"
#include "tlock.h"

namespace blsk {

// ------------------------------------------------------------------ prepare (one lane, once per sigma)
// S / s_inf / s_cls: the one-entry staging launch_decompress_g2 filled (stride 1). A sigma that does
// not decode or is the point at infinity leaves the table untouched (the host never runs the f pass
// on it).
__global__ void __launch_bounds__(TPB) k_tlock_prepare(const uint32_t* S, const uint8_t* s_inf, const uint8_t* s_cls,
                                                       uint32_t* tab) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (s_cls[0] != REJ_OK || s_inf[0]) return;
  const g2a Q = {ld_fp2(S, 1, 0, 0), ld_fp2(S, 1, 0, 2)};
  tlock_prepare(Q, [&](int step, int c, const fp2& v) {
    uint32_t* o = tab + (step * 3 + c) * 24;
#pragma unroll
    for (int w = 0; w < 12; w++) {
      o[w] = v.c0.l[w];
      o[12 + w] = v.c1.l[w];
    }
  });
}

// ------------------------------------------------------------------ f pass (one lane per ciphertext)
#ifndef BLS_WPE_TLOCK_F
#define BLS_WPE_TLOCK_F 1
#endif

// The line table is wave-uniform and read-only: one LDS copy per workgroup, read by broadcast (every
// lane of a ds_read has the same address).
static __shared__ uint32_t g_tl_tab[TLOCK_TAB_WORDS];
// The two U-dependent line slots (c1 xU, c2 yU) of the current step park in LDS, one 48-word column per
// lane (12 KB per one-wave workgroup), and are read back at each use: f and the partial products are
// all that stay in registers.
static __shared__ uint32_t g_tl_L[48 * BLS_LANES];
static_assert(sizeof(uint32_t) * (TLOCK_TAB_WORDS + 48 * BLS_LANES + 24 * BLS_LANES + 16 * 12) <= 40960,
              "k_tlock_f: four one-wave workgroups per CU share its 160 KB of LDS");
static_assert(BLS_LANES == TPB, "the parked columns are indexed by threadIdx.x");

DI void tl_put(int c, const fp2& v) {  // c = 1, 2
  const unsigned l = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    g_tl_L[((c - 1) * 24 + k) * BLS_LANES + l] = v.c0.l[k];
    g_tl_L[((c - 1) * 24 + 12 + k) * BLS_LANES + l] = v.c1.l[k];
  }
}
DI fp2 tl_coef(int step, int c) {
  int o = (step * 3 + c) * 24;
  asm volatile("" : "+s"(o));  // read at the use, never kept live
  fp2 v;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    v.c0.l[k] = g_tl_tab[o + k];
    v.c1.l[k] = g_tl_tab[o + 12 + k];
  }
  return v;
}
// slot c of the current line: 0 from the table, 1 and 2 from the lane's parked column
DI fp2 tl_get(int step, int c) {
  if (c == 0) return tl_coef(step, 0);
  unsigned l = threadIdx.x;
  asm volatile("" : "+v"(l));
  fp2 v;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    v.c0.l[k] = g_tl_L[((c - 1) * 24 + k) * BLS_LANES + l];
    v.c1.l[k] = g_tl_L[((c - 1) * 24 + 12 + k) * BLS_LANES + l];
  }
  return v;
}

using KpLds16T = KpLdsK<16>;

// U: the AoS table launch_decompress_g1 wrote (G1_WORDS per item) with u_inf / cls; F: SoA of stride cnt.
// sig_inf (device flag of the prepared sigma): a pair with a point at infinity is skipped, E = 1.
BLS_KERNEL(BLS_WPE_TLOCK_F)
k_tlock_f(const uint32_t* tab, const uint32_t* U, const uint8_t* u_inf, const uint8_t* cls, const uint8_t* sig_inf,
          size_t cnt, uint32_t* F) {
  // before the early exits: every lane of the workgroup copies its share of the tables
  for (unsigned j = threadIdx.x; j < (unsigned)TLOCK_TAB_WORDS; j += TPB) g_tl_tab[j] = tab[j];
#if BLS_F6_LIN
  kp_lds_init<16>();  // ends with the barrier that also covers g_tl_tab
#else
  __syncthreads();
#endif
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  if (cls[i] != REJ_OK) return;
  if (u_inf[i] | sig_inf[0]) {
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
  fp12 f;
  int step = 0;
#pragma unroll 1
  for (int b = 62; b >= 0; b--) {
#pragma unroll 1
    for (int rep = 0; rep < 2; rep++) {
      if (rep == 1 && !((BLS_X_ABS >> b) & 1ull)) break;
      const fp2 l1 = fp2_mul_fp(tl_coef(step, 1), ucoord(0));
      const fp2 l2 = fp2_mul_fp(tl_coef(step, 2), ucoord(1));
      if (step == 0) {  // f = 1 * l: the first line is f itself
        f = {{tl_coef(0, 0), l1, fp2_zero()}, {fp2_zero(), l2, fp2_zero()}};
        step++;
        continue;
      }
      tl_put(1, l1);
      tl_put(2, l2);
#if BLS_F6_LIN
      if (rep == 0) f = fp12_sqr_lin(f, KpLds16T());
#else
      if (rep == 0) f = fp12_sqr(f);
#endif
      f = fp12_mul_by_014_l(f, [&](int c) { return tl_get(step, c); });
      step++;
    }
  }
  st_fp12(F, cnt, i, fp12_conj(f));
}

// ------------------------------------------------------------------ encode
// One lane per (item, Fp coefficient): coefficient k of the encoding is SoA slot 11 - k (c1.c2.c1 first,
// c0.c0.c0 last), canonical and out of Montgomery form, 48 bytes big-endian. A rejected item gets zeros.
// out: 4-byte aligned, cnt x 576 bytes.
__global__ void __launch_bounds__(TPB) k_tlock_encode(const uint32_t* E, const uint8_t* cls, size_t cnt, uint32_t* out) {
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= cnt * 12) return;
  const size_t i = t / 12;
  const int k = (int)(t % 12);
  uint32_t* o = out + t * 12;
  if (cls[i] != REJ_OK) {
#pragma unroll
    for (int w = 0; w < 12; w++) o[w] = 0;
    return;
  }
  const fp v = fp_from_mont(ld_fp_v(E, cnt, i, 11 - k));
#pragma unroll
  for (int w = 0; w < 12; w++) o[w] = __builtin_bswap32(v.l[11 - w]);
}

// ------------------------------------------------------------------ launchers
void launch_tlock_prepare(const uint32_t* S, const uint8_t* s_inf, const uint8_t* s_cls, uint32_t* tab, hipStream_t st) {
  hipLaunchKernelGGL(k_tlock_prepare, dim3(1), dim3(TPB), 0, st, S, s_inf, s_cls, tab);
}

void launch_tlock_f(const uint32_t* tab, const uint32_t* U, const uint8_t* u_inf, const uint8_t* cls,
                    const uint8_t* sig_inf, size_t cnt, uint32_t* F, hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_tlock_f, dim3(grid_for(cnt)), dim3(TPB), 0, st, tab, U, u_inf, cls, sig_inf, cnt, F);
}

void launch_tlock_encode(const uint32_t* E, const uint8_t* cls, size_t cnt, uint8_t* out, hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_tlock_encode, dim3(grid_for(cnt * 12)), dim3(TPB), 0, st, E, cls, cnt, (uint32_t*)out);
}

}  // namespace blsk
