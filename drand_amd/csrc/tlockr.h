// Timelock opening across many rounds: n pairings e(U_i, sigma_j(i)) where round j owns a run of
// consecutive items (include/blsverify.h "timelock", blsv_tlock_open_rounds). The arithmetic is tlock.h's
// -- sigma's 68 lines prepared once into a table of P-independent coefficients, then per U the f pass over
// that table -- with two differences:
//   prepare : one lane per signature of the pass. The table is word-major over the pass's M signatures,
//             word w of signature j at tab[w * M + j]: the lanes' stores coalesce, and where neighbouring
//             items hold neighbouring signatures so do the loads of the f pass.
//   f       : one tile (hostlogic.h TlockTile) per workgroup. A uniform tile shares one signature: its
//             table column is copied to LDS and read by broadcast, as k_tlock_f reads its one table. A
//             mixed tile's lanes each read their own signature's column from global memory at the use.
//             The loop is one body, tlockr_f, whose only form-specific part is the coefficient read.
// The shared host/device forms below are what tools/opcount tlockr runs; k_tlockr.hip holds the device
// kernels.
#pragma once
#include "tlock.h"

namespace bls {

// BLSV_REJ_TLOCK_SIG: the class of an item whose own U decodes but whose round's signature did not
constexpr uint8_t REJ_TLOCK_SIG = 9;

// word w (< TLOCK_TAB_WORDS) of signature j's table among the M signatures of a pass
DI size_t tlockr_tab_at(int w, size_t M, size_t j) { return (size_t)w * M + j; }
// first word of coefficient c of line `step` in one signature's table (tlock.h's order)
DI int tlockr_coef_word(int step, int c) { return (step * 3 + c) * 24; }

// tlock_prepare with every word handed to put(w, value), w < TLOCK_TAB_WORDS
template <typename Put>
DI void tlockr_prepare(const g2a& Q, Put put) {
  tlock_prepare(Q, [&](int step, int c, const fp2& v) {
    const int o = tlockr_coef_word(step, c);
#pragma unroll
    for (int w = 0; w < 12; w++) {
      put(o + w, v.c0.l[w]);
      put(o + 12 + w, v.c1.l[w]);
    }
  });
}

// The f pass of one item, the loop of k_tlock_f: coef(step, c) reads table coefficient c of line `step`
// (from LDS in a uniform tile, from global memory in a mixed one) and is called at each use; ucoord(c)
// reads xU (0) or yU (1); park(c, v) / parked(c) keep the two U-dependent slots (c = 1, 2) of the current
// line out of the registers; sqr is the Fp12 squaring.
template <typename Coef, typename UCoord, typename Park, typename Parked, typename Sqr>
DI fp12 tlockr_f(Coef coef, UCoord ucoord, Park park, Parked parked, Sqr sqr) {
  fp12 f;
  int step = 0;
#pragma unroll 1
  for (int b = 62; b >= 0; b--) {
#pragma unroll 1
    for (int rep = 0; rep < 2; rep++) {
      if (rep == 1 && !((BLS_X_ABS >> b) & 1ull)) break;
      const fp2 l1 = fp2_mul_fp(coef(step, 1), ucoord(0));
      const fp2 l2 = fp2_mul_fp(coef(step, 2), ucoord(1));
      if (step == 0) {  // f = 1 * l: the first line is f itself
        f = {{coef(0, 0), l1, fp2_zero()}, {fp2_zero(), l2, fp2_zero()}};
        step++;
        continue;
      }
      park(1, l1);
      park(2, l2);
      if (rep == 0) f = sqr(f);
      f = fp12_mul_by_014_l(f, [&](int c) { return c == 0 ? coef(step, 0) : parked(c); });
      step++;
    }
  }
  return fp12_conj(f);
}

}  // namespace bls
