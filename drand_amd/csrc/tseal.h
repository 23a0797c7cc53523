// Timelock sealing: n ciphertext heads (U_i, K_i) locked to one round under one key
// (include/blsverify.h "timelock", blsv_tlock_seal). With B = e(pk, H(MessageV2(round)))^3 computed once
// (the opening's own kernels, tseal.cpp), item i is U_i = k_i G1 and K_i = B^k_i: two fixed-base
// operations, so both walk a table of the base's multiples by four-bit windows of k_i,
//   T1[w][j] = j 16^w G1   (affine, Montgomery; w < 64, j = 1..15;  64 x 15 x 96 B  =  92,160 bytes)
//   T2[w][j] = B^(j 16^w)  (Fp12, Montgomery, tower order;          64 x 15 x 576 B = 552,960 bytes)
// one mixed addition / one Fp12 product per non-zero digit, no doubling and no squaring per item.
// B lies in the cyclotomic subgroup (it left the final exponentiation), so the 64 values B^(16^w) are a
// chain of 252 Granger-Scott squarings. Table indices depend on the scalar's digits: nothing here is
// constant-time (as jac_mul_scalar's branches are not for blsv_sign).
// The shared host/device forms below are what tools/opcount tseal runs and counts; k_tseal.hip holds the
// device kernels.
#pragma once
#include "tlock.h"
#include "tscalar.h"

namespace bls {

constexpr int TSEAL_G1_WORDS = 24;   // one T1 entry: x, y
constexpr int TSEAL_GT_WORDS = 144;  // one T2 entry
constexpr int TSEAL_T1_WORDS = TSEAL_WINDOWS * TSEAL_ENTRIES * TSEAL_G1_WORDS;
constexpr int TSEAL_T2_WORDS = TSEAL_WINDOWS * TSEAL_ENTRIES * TSEAL_GT_WORDS;
constexpr uint8_t TSEAL_REFUSED = 1;  // class byte of an item with k == 0 (mod r): encodes as zeros

// tscalar.h: TSEAL_WINDOWS, TSEAL_ENTRIES, TSEAL_SCALAR_LEN, tseal_entry, and the scalar's reduction and
// digits (tseal_scalar, tseal_digit), shared with the latency engine's item

// Row w of the table of a base point A of order r (T1's layout): 16^w A by 4w doublings, its multiples by
// repeated addition, each to affine. emit(j, P), j = 1..15.
template <typename Emit>
DI void tseal_g1_row_of(const g1a& A, int w, Emit emit) {
  g1j base = jac_from_aff(A);
#pragma unroll 1
  for (int k = 0; k < 4 * w; k++) base = jac_dbl(base);
  const g1a b = g1_to_aff(base);
  g1j acc = jac_from_aff(b);
  emit(1, b);
#pragma unroll 1
  for (int j = 2; j <= TSEAL_ENTRIES; j++) {
    acc = jac_add_aff(acc, b);  // j 16^w < r: never the point at infinity
    emit(j, g1_to_aff(acc));
  }
}
// Row w of T1: the generator's
template <typename Emit>
DI void tseal_g1_row(int w, Emit emit) {
  tseal_g1_row_of(g1a{fp_load_const(G1_GEN_X), fp_load_const(G1_GEN_Y)}, w, emit);
}

// The chain B^(16^w), w = 0..63: emit(w, v). B must lie in the cyclotomic subgroup.
template <typename Emit>
DI void tseal_gt_chain(const fp12& B, Emit emit) {
  fp12 v = B;
  emit(0, v);
#pragma unroll 1
  for (int w = 1; w < TSEAL_WINDOWS; w++) {
#pragma unroll 1
    for (int k = 0; k < 4; k++) v = fp12_cyclotomic_sqr(v);
    emit(w, v);
  }
}

// Row w of T2 beyond its first entry b = B^(16^w): emit(j, b^j), j = 2..15
template <typename Emit>
DI void tseal_gt_row(const fp12& b, Emit emit) {
  fp12 acc = b;
#pragma unroll 1
  for (int j = 2; j <= TSEAL_ENTRIES; j++) {
    acc = fp12_mul(acc, b);
    emit(j, acc);
  }
}

// U = k G1 from T1: one mixed addition per non-zero digit. entry(w, j) returns T1[w][j]. jac_add_aff
// carries the exceptional cases; with k < r a partial sum is infinity only before the first non-zero
// digit and never equals +- the addend (the sum of the lower windows is below 16^w <= j 16^w, and their
// total is below r), so only its first branch is ever taken.
template <typename Entry>
DI g1j tseal_u(const uint32_t (&k)[8], Entry entry) {
  g1j acc = jac_infinity<fp>();
#pragma unroll 1
  for (int w = 0; w < TSEAL_WINDOWS; w++) {
    const int d = tseal_digit(k, w);
    if (d) acc = jac_add_aff(acc, entry(w, d));
  }
  return acc;
}

// a * b with b fetched by Fp6 halves at their uses (half(0) = c0, half(1) = c1): fp12_mul's Karatsuba,
// the operand never whole in registers beside the accumulator
template <typename Half>
DI fp12 tseal_mul_halves(const fp12& a, Half half) {
  const fp6 t0 = fp6_mul(a.c0, half(0));
  const fp6 t1 = fp6_mul(a.c1, half(1));
  const fp6 c1 = fp6_sub(fp6_sub(fp6_mul(fp6_add_lazy(a.c0, a.c1), fp6_add_lazy(half(0), half(1))), t0), t1);
  return {fp6_add(t0, fp6_mul_v(t1)), c1};
}

// K = B^k from T2: the product of one entry per non-zero digit (k != 0). half(w, j, h) returns half h of
// T2[w][j].
template <typename Half>
DI fp12 tseal_gt(const uint32_t (&k)[8], Half half) {
  fp12 acc = fp12_one();
  bool first = true;
#pragma unroll 1
  for (int w = 0; w < TSEAL_WINDOWS; w++) {
    const int d = tseal_digit(k, w);
    if (!d) continue;
    if (first) {
      acc = {half(w, d, 0), half(w, d, 1)};
      first = false;
    } else {
      acc = tseal_mul_halves(acc, [&](int h) { return half(w, d, h); });
    }
  }
  return acc;
}

}  // namespace bls
