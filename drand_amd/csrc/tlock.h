// Timelock opening: N pairings e(U_i, sigma) that share the G2 argument (include/blsverify.h
// "timelock"). sigma's Miller steps do not depend on U, so they run ONCE per signature:
//   prepare : T walks the 63 doublings and 5 additions of pairing.h and the P-independent
//             coefficients of every line go to a table of 68 x 3 Fp2 (19,584 bytes):
//               doubling (E - B, 3 X^2, -H),  addition (theta x2 - delta y2, -theta, delta)
//   f       : per U, f = f^2 * l_s(U) over the 68 steps with l_s(U) = (c0, c1 xU, c2 yU):
//             two Fp2-by-Fp products and one sparse 0/1/4 product per step, conjugated at the end.
// The lines are those of miller_dbl_step / miller_add_step (equal as field elements: the sign of the
// third slot is applied before the product by yU instead of after it), f is miller_loop_multi<1>'s.
// The shared host/device forms below are what tools/opcount tlock runs and counts; k_tlock.hip holds
// the device kernels.
#pragma once
#include "pairing.h"

namespace bls {

constexpr int TLOCK_TAB_WORDS = MILLER_STEPS * 3 * 24;  // 68 steps x 3 Fp2 x 24 words
constexpr int TLOCK_GT_LEN = 576;

// emit(step, c, v): coefficient c (0, 1, 2) of line `step`. The steps are miller_dbl_step /
// miller_add_step themselves, evaluated at (xP, yP) = (1, 1).
template <typename Emit>
DI void tlock_prepare(const g2a& Q, Emit emit) {
  const fp one = fp_one();
  g2proj T = {Q.x, Q.y, fp2_one()};
  int step = 0;
#pragma unroll 1
  for (int i = 62; i >= 0; i--) {
    line l;
    miller_dbl_step<false>(T, l.a0, l.a1, l.a4, one, one);
    emit(step, 0, l.a0), emit(step, 1, l.a1), emit(step, 2, l.a4);
    step++;
    if ((BLS_X_ABS >> i) & 1ull) {
      miller_add_step(T, Q, l.a0, l.a1, l.a4, one, one);
      emit(step, 0, l.a0), emit(step, 1, l.a1), emit(step, 2, l.a4);
      step++;
    }
  }
}

// line `step` at U from its table coefficients
template <typename Coef>
DI line tlock_line(Coef coef, int step, const fp& xu, const fp& yu) {
  return {coef(step, 0), fp2_mul_fp(coef(step, 1), xu), fp2_mul_fp(coef(step, 2), yu)};
}

// tower.h fp12_mul_by_014 with the line read through l(c) at each use (k_tlock_f: from LDS; the
// single-pair f pass of tsealr.h: from the line staging). (Forming c first, so that a, b and c are never
// all live with f, costs scratch instead of saving it: 320 bytes per lane against 224 in k_tlock_f.)
template <typename L>
DI fp12 fp12_mul_by_014_l(const fp12& f, L l) {
  const fp6 a = fp6_mul_by_01(f.c0, l(0), l(1));
  const fp6 b = fp6_mul_by_1(f.c1, l(2));
  const fp6 c = fp6_mul_by_01(fp6_add_lazy(f.c0, f.c1), l(0), fp2_add_lazy(l(1), l(2)));
  return {fp6_add(a, fp6_mul_v(b)), fp6_sub(fp6_sub(c, a), b)};
}

// register form of the f pass (host op counter; k_tlock_f is the device form)
template <typename Coef>
DI fp12 tlock_f(Coef coef, const fp& xu, const fp& yu) {
  fp12 f = fp12_one();
  int step = 0;
#pragma unroll 1
  for (int i = 62; i >= 0; i--) {
    const line l = tlock_line(coef, step, xu, yu);
    if (step == 0)  // f = 1 * l: the first line is f itself
      f = {{l.a0, l.a1, fp2_zero()}, {fp2_zero(), l.a4, fp2_zero()}};
    else
      f = fp12_mul_by_014(fp12_sqr(f), l.a0, l.a1, l.a4);
    step++;
    if ((BLS_X_ABS >> i) & 1ull) {
      const line a = tlock_line(coef, step, xu, yu);
      f = fp12_mul_by_014(f, a.a0, a.a1, a.a4);
      step++;
    }
  }
  return fp12_conj(f);
}

// Gt encoding: twelve canonical Fp values, 48 bytes big-endian each, highest tower coefficient first
// (c1.c2.c1, c1.c2.c0, c1.c1.c1, ..., c0.c0.c1, c0.c0.c0)
DI void tlock_encode(uint8_t* out, const fp12& e) {
  const fp2* c[6] = {&e.c1.c2, &e.c1.c1, &e.c1.c0, &e.c0.c2, &e.c0.c1, &e.c0.c0};
#pragma unroll
  for (int k = 0; k < 6; k++) {
    fp_raw_to_be48(out + 96 * k, fp_from_mont(c[k]->c1));
    fp_raw_to_be48(out + 96 * k + 48, fp_from_mont(c[k]->c0));
  }
}

}  // namespace bls
