// Timelock sealing to many rounds: n ciphertext heads (U_i, K_i), item i locked to its own round_i under
// one key (include/blsverify.h "timelock", blsv_tlock_seal_rounds). No base is shared between items, so
// by bilinearity each K_i is one single-pair pairing of its own,
//   K_i = e(pk, H(MessageV2(round_i)))^(3 k_i) = e(k_i pk, H_i)^3,
// and every lane does for its item what tseal.cpp's seal_prepare does for one base:
//   P_i = k_i pk   a fixed-base walk over the key table TK[w][j] = j 16^w pk (T1's layout, 92,160 bytes,
//                  built once per key by tseal_g1_row_of), then one inversion to affine;
//   lines          T = H_i through the 63 doublings and 5 additions, the pair (P_i, H_i) alone: 68 lines
//                  of 3 Fp2 per item, half of MILLER_LINE_WORDS;
//   f              f = f^2 l(step) with the sparse 0/1/4 product, the line read from the staging at each
//                  use: no line_mul_line, no fp12_mul_by_line_pair;
// then the final exponentiation and the opening's Gt encoding. U_i = k_i G1 is tseal.h's. Table indices
// depend on the scalar's digits: nothing here is constant-time.
// The shared host/device forms below are what tools/opcount tsealr runs and counts; k_tsealr.hip
// holds the device kernels.
#pragma once
#include "tseal.h"

namespace bls {

constexpr int TSEALR_LINE_SLOTS = 6;                                       // a0, a1, a4 as Fp2
constexpr int TSEALR_LINE_WORDS = MILLER_STEPS * TSEALR_LINE_SLOTS * 12;  // per item

// first Fp slot of line `step` in the single-pair staging (SoA)
DI int tsealr_line_slot(int step) { return step * TSEALR_LINE_SLOTS; }

// P = k pk in affine form from the key table: entry(w, j) returns TK[w][j]. tseal_u's argument carries
// over unchanged: pk has order r and k < r, so a partial sum (the lower windows' total times pk, below
// 16^w <= j 16^w and below r) is infinity only before the first non-zero digit and never +- the addend;
// only jac_add_aff's first branch is ever taken. k != 0, so P is never the point at infinity.
template <typename Entry>
DI g1a tsealr_point(const uint32_t (&k)[8], Entry entry) {
  return g1_to_aff(tseal_u(k, entry));
}

// The lines of the single pair (P, Q): T (an accessor as pairing.h g2proj_reg / k_miller.hip
// g2proj_lds) starts at Q and walks |x|'s bits with the call-free steps of k_miller_lines;
// put(step, c, v) receives coefficient c (0: a0, 1: a1, 2: a4) of line `step`; xp() / yp() and load_q()
// re-read their operands at each use.
template <typename TS, typename LoadQ, typename Put, typename XP, typename YP>
DI void tsealr_lines(const TS& T, LoadQ load_q, Put put, XP xp, YP yp) {
  {
    const g2a Q0 = load_q();
    T.set(0, Q0.x);
    T.set(1, Q0.y);
    T.set(2, fp2_one());
  }
  int step = 0;
  auto put_step = [&](int c, const fp2& v) { put(step, c, v); };
#pragma unroll 1
  for (int b = 62; b >= 0; b--) {
    miller_dbl_step_ts(T, put_step, xp, yp);
    step++;
    if ((BLS_X_ABS >> b) & 1ull) {
      miller_add_step_ts(T, load_q, put_step, xp, yp);
      step++;
    }
  }
}

// f of the single pair from its lines: l(step, c) returns coefficient c of line `step` and is called at
// each use (twice per coefficient and product); sqr is the Fp12 squaring (fp12_sqr, or the device's
// one-reduction form). The loop is k_tlock_f's, the value miller_loop_multi<1>'s.
template <typename L, typename Sqr>
DI fp12 tsealr_f(L l, Sqr sqr) {
  fp12 f;
  int step = 0;
#pragma unroll 1
  for (int b = 62; b >= 0; b--) {
#pragma unroll 1
    for (int rep = 0; rep < 2; rep++) {
      if (rep == 1 && !((BLS_X_ABS >> b) & 1ull)) break;
      if (step == 0) {  // f = 1 * l: the first line is f itself
        f = {{l(0, 0), l(0, 1), fp2_zero()}, {fp2_zero(), l(0, 2), fp2_zero()}};
        step++;
        continue;
      }
      if (rep == 0) f = sqr(f);
      f = fp12_mul_by_014_l(f, [&](int c) { return l(step, c); });
      step++;
    }
  }
  return fp12_conj(f);
}

}  // namespace bls
