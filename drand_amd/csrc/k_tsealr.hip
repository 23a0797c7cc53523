// Timelock sealing to many rounds (tsealr.h, include/blsverify.h "timelock"): K_i = e(k_i pk, H_i)^3 with
// H_i = H(MessageV2(round_i)), one single-pair pairing per item, the items of a pass side by side.
// k_tseal_key_table fills the key's table TK once per key (T1's layout over pk instead of the generator),
// k_tsealr_point walks it for P_i = k_i pk, k_miller_lines1 and k_miller_f1 are the two Miller passes of
// the pairs (P_i, H_i) alone; U_i, the hash, the final exponentiation and the Gt encoding are the
// launchers of k_tseal.hip, k_hash.hip, k_fexp.hip and k_tlock.hip unchanged. The kernels live in a unit
// of their own so that the two-pair passes of k_miller.hip compile to what they compiled to before.
#include "kmiller.h"
#include "tsealr.h"

namespace blsk {

static_assert(TSEAL_WINDOWS == TPB, "the table kernel gives every window a lane of one wave");
static_assert(G1_WORDS == TSEAL_G1_WORDS, "a P entry is a key-table entry");
static_assert(kMillerLine1Words == (size_t)TSEALR_LINE_WORDS && 2 * TSEALR_LINE_WORDS == MILLER_LINE_WORDS,
              "a single pair uses half of the line staging");

// an affine G1 point as 24 plain words (x, y Montgomery): a table entry
DI g1a ld_g1(const uint32_t* p) {
  g1a v;
#pragma unroll
  for (int w = 0; w < 12; w++) {
    v.x.l[w] = p[w];
    v.y.l[w] = p[12 + w];
  }
  return v;
}
DI void st_g1(uint32_t* p, const g1a& v) {
#pragma unroll
  for (int w = 0; w < 12; w++) {
    p[w] = v.x.l[w];
    p[12 + w] = v.y.l[w];
  }
}

// ------------------------------------------------------------------ TK (once per key)
// key: the one-entry table launch_decompress_g1 wrote (G1_WORDS words; the host has checked that it
// decoded and is not the point at infinity). One wave: lane w fills row w.
__global__ void __launch_bounds__(TPB) k_tseal_key_table(const uint32_t* key, uint32_t* TK) {
  const int w = (int)threadIdx.x;
  if (blockIdx.x != 0) return;
  tseal_g1_row_of(ld_g1(key), w,
                  [&](int j, const g1a& p) { st_g1(TK + (size_t)tseal_entry(w, j) * TSEAL_G1_WORDS, p); });
}

// ------------------------------------------------------------------ P (one lane per item)
#ifndef BLS_WPE_TSEALR_P
#define BLS_WPE_TSEALR_P 2
#endif
// P_i = k_i pk: at most 64 mixed additions over TK and one inversion, written as entry i of an AoS table
// (G1_WORDS per item: what k_miller_lines1 reads). pk has order r and k_i < r, so the walk never meets
// jac_add_aff's exceptional branches (tsealr.h tsealr_point). An item whose class is not 0 (a refused
// scalar) is left untouched.
BLS_KERNEL(BLS_WPE_TSEALR_P)
k_tsealr_point(const uint32_t* TK, const uint8_t* scalars, const uint8_t* cls, size_t cnt, uint32_t* P) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  if (cls[i] != REJ_OK) return;
  uint32_t k[8];
  (void)tseal_scalar(scalars + i * TSEAL_SCALAR_LEN, k);
  st_g1(P + i * G1_WORDS,
        tsealr_point(k, [&](int w, int j) { return ld_g1(TK + (size_t)tseal_entry(w, j) * TSEAL_G1_WORDS); }));
}

// ------------------------------------------------------------------ lines of a single pair
// The pair (P_i, H_i) with item i's own P at entry i of the AoS table P (no index array), one workgroup
// per 64 items and none for a second pair: 3 Fp2 per step, TSEALR_LINE_WORDS per item (half of
// MILLER_LINE_WORDS), SoA of stride cnt. T parks in LDS as in k_miller_lines. A rejected item, or one
// whose H is the point at infinity, writes nothing: k_miller_f1 reads no line of it.
BLS_KERNEL(BLS_WPE_LINES)
k_miller_lines1(const uint32_t* P, const uint32_t* H, const uint8_t* h_inf, const uint8_t* cls, size_t cnt,
                uint32_t* LN) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  if (cls[i] != REJ_OK || h_inf[i]) return;
  auto load_q = [&]() {
    size_t j = i;
    asm volatile("" : "+v"(j));  // re-read at each use (5 additions), never hoisted
    return g2a{ld_fp2(H, cnt, j, 0), ld_fp2(H, cnt, j, 2)};
  };
  auto pcoord = [&](int c) {
    size_t o = i * G1_WORDS + 12 * c;
    asm volatile("" : "+v"(o));  // re-read at the use
    fp v;
#pragma unroll
    for (int w = 0; w < 12; w++) v.l[w] = P[o + w];
    return v;
  };
  tsealr_lines(
      g2proj_lds{g_ml_T + threadIdx.x}, load_q,
      [&](int step, int c, const fp2& v) { st_fp2<BLS_LN_AUX_ST>(LN, cnt, i, tsealr_line_slot(step) + 2 * c, v); },
      [&]() { return pcoord(0); }, [&]() { return pcoord(1); });
}

// ------------------------------------------------------------------ f of a single pair
// tsealr_f over the lines of k_miller_lines1: f = f^2 l(step) with the sparse 0/1/4 product, the line's
// three Fp2 read from the staging at each use (non-temporal, as k_miller_f's), so f and the partial
// products are all that stay in registers and nothing parks in LDS: no line_mul_line, no
// fp12_mul_by_line_pair. A pair whose H is the point at infinity is skipped (f = 1).
BLS_KERNEL(BLS_WPE_MILLER_F)
k_miller_f1(const uint32_t* LN, const uint8_t* h_inf, const uint8_t* cls, size_t cnt, uint32_t* F) {
#if BLS_F6_LIN
  kp_lds_init<16>();  // before the early exits: every lane of the workgroup writes its table words
#endif
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  if (cls[i] != REJ_OK) return;
  if (h_inf[i]) {
    st_fp12(F, cnt, i, fp12_one());
    return;
  }
  auto l = [&](int step, int c) {
    size_t j = i;
    asm volatile("" : "+v"(j));  // read at the use, never kept live
    return ld_fp2<BLS_LN_AUX_LD>(LN, cnt, j, tsealr_line_slot(step) + 2 * c);
  };
#if BLS_F6_LIN
  st_fp12(F, cnt, i, tsealr_f(l, [](const fp12& f) { return fp12_sqr_lin(f, KpLds16()); }));
#else
  st_fp12(F, cnt, i, tsealr_f(l, [](const fp12& f) { return fp12_sqr(f); }));
#endif
}

// ------------------------------------------------------------------ launchers
void launch_tseal_key_table(const uint32_t* key, uint32_t* TK, hipStream_t st) {
  hipLaunchKernelGGL(k_tseal_key_table, dim3(1), dim3(TPB), 0, st, key, TK);
}

void launch_tsealr_point(const uint32_t* TK, const uint8_t* scalars, const uint8_t* cls, size_t cnt, uint32_t* P,
                         hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_tsealr_point, dim3(grid_for(cnt)), dim3(TPB), 0, st, TK, scalars, cls, cnt, P);
}

void launch_miller_lines1(const uint32_t* P, const uint32_t* H, const uint8_t* h_inf, const uint8_t* cls, size_t cnt,
                          uint32_t* LN, hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_miller_lines1, dim3(grid_for(cnt)), dim3(TPB), 0, st, P, H, h_inf, cls, cnt, LN);
}

void launch_miller_f1(const uint32_t* LN, const uint8_t* h_inf, const uint8_t* cls, size_t cnt, uint32_t* F,
                      hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_miller_f1, dim3(grid_for(cnt)), dim3(TPB), 0, st, LN, h_inf, cls, cnt, F);
}

}  // namespace blsk
