// Raw operation hooks of the field and tower arithmetic (include/blsverify_testing.h blsv_test_op,
// tools/opcount `ops`): every form of fp.h / tower.h / tri.h / pairing.h that a production kernel
// reaches, run on operands the TEST chooses. Operands and results are raw 12-word values per Fp
// element in tower order, copied in and out with no fp_to_mont / fp_from_mont / fp_canon in between,
// so the caller picks the representative (v or v + p, lazy sums, limb patterns). Booleans come back as
// word 0 of an Fp-sized result. Not used by the product path.
//
// BLS_TEST_OPS(X): X(name, Fp elements in, Fp elements out, kind)
//   kind 0  one item per lane, in the device build (k_test.hip) and the host build (tools/opcount)
//   kind 1  one item per lane, device only (the forms of tri.h that the host build does not contain,
//           and the LDS tables of k p)
//   kind 2  one item per lane, device only, in k_miller.hip (the f pass's own LDS forms)
//   kind 3  three lanes per item (tri.h), 21 items per wave, lane 63 a dummy; device only
// The one-reduction linear forms take their q p from KpLdsK<16> on the device and KpMad on the host.
#pragma once
#include "pairing.h"
#include "tri.h"
#include "testops_list.h"

namespace bls {

DI fp2 t_f2(const fp* x, int k) { return {x[k], x[k + 1]}; }
DI fp6 t_f6(const fp* x, int k) { return {t_f2(x, k), t_f2(x, k + 2), t_f2(x, k + 4)}; }
DI fp12 t_f12(const fp* x, int k) { return {t_f6(x, k), t_f6(x, k + 6)}; }
DI void t_put2(fp* r, int k, const fp2& v) { r[k] = v.c0, r[k + 1] = v.c1; }
DI void t_put6(fp* r, int k, const fp6& v) { t_put2(r, k, v.c0), t_put2(r, k + 2, v.c1), t_put2(r, k + 4, v.c2); }
DI void t_put12(fp* r, int k, const fp12& v) { t_put6(r, k, v.c0), t_put6(r, k + 6, v.c1); }
DI fp t_flag(bool b) {
  fp r = fp_zero();
  r.l[0] = b ? 1u : 0u;
  return r;
}

// the kind-0 operations: x = the item's operands, r = its results
template <int OP, typename KP16>
DI void test_op_run(const fp* x, fp* r) {
  if constexpr (OP == TOP_fp_mul) r[0] = fp_mul(x[0], x[1]);
  if constexpr (OP == TOP_fp_mul_inl) r[0] = fp_mul_inl(x[0], x[1]);
  if constexpr (OP == TOP_fp_sqr) r[0] = fp_sqr(x[0]);
  if constexpr (OP == TOP_fp_add) r[0] = fp_add(x[0], x[1]);
  if constexpr (OP == TOP_fp_sub) r[0] = fp_sub(x[0], x[1]);
  if constexpr (OP == TOP_fp_addsub_add) r[0] = fp_addsub(x[0], x[1], false);
  if constexpr (OP == TOP_fp_addsub_sub) r[0] = fp_addsub(x[0], x[1], true);
  if constexpr (OP == TOP_fp_neg) r[0] = fp_neg(x[0]);
  if constexpr (OP == TOP_fp_half) r[0] = fp_half(x[0]);
  if constexpr (OP == TOP_fp_dbl) r[0] = fp_dbl(x[0]);
  if constexpr (OP == TOP_fp_mul3) r[0] = fp_mul3(x[0]);
  if constexpr (OP == TOP_fp_add_lazy_mul) {  // one lazy level (< 4p) feeding a product
    r[0] = fp_add_lazy(x[0], x[1]);
    r[1] = fp_mul(r[0], x[2]);
  }
  if constexpr (OP == TOP_fp_add_lazy2_mul) {  // two lazy levels (< 8p) on one side, one on the other
    r[0] = fp_add_lazy(fp_add_lazy(x[0], x[1]), fp_add_lazy(x[2], x[3]));
    r[1] = fp_mul(r[0], fp_add_lazy(x[4], x[0]));
  }
  if constexpr (OP == TOP_fp_canon) r[0] = fp_canon(x[0]);
  if constexpr (OP == TOP_fp_is_zero) r[0] = t_flag(fp_is_zero(x[0]));
  if constexpr (OP == TOP_fp_eq) r[0] = t_flag(fp_eq(x[0], x[1]));
  if constexpr (OP == TOP_fp_inv_bingcd_raw) {  // the GCD alone (no exponentiation fallback) and its flag
    bool ok;
    r[0] = fp_from_u12(fp_inv_bingcd_raw(fp_to_u12(x[0]), ok));
    r[1] = t_flag(ok);
  }
  if constexpr (OP == TOP_fp_inv) r[0] = fp_inv(x[0]);
  if constexpr (OP == TOP_fp_pow_sqrt_inv) r[0] = fp_pow_sqrt_inv(x[0]);
  if constexpr (OP == TOP_fp2_mul) t_put2(r, 0, fp2_mul(t_f2(x, 0), t_f2(x, 2)));
  if constexpr (OP == TOP_fp2_mul_inl) t_put2(r, 0, fp2_mul_inl(t_f2(x, 0), t_f2(x, 2)));
  if constexpr (OP == TOP_fp2_mul_inl_kara) t_put2(r, 0, fp2_mul_inl_t<true>(t_f2(x, 0), t_f2(x, 2)));
  if constexpr (OP == TOP_fp2_sqr) t_put2(r, 0, fp2_sqr(t_f2(x, 0)));
  if constexpr (OP == TOP_fp2_sqr_inl) t_put2(r, 0, fp2_sqr_inl(t_f2(x, 0)));
  if constexpr (OP == TOP_fp2_mul_xi) t_put2(r, 0, fp2_mul_xi(t_f2(x, 0)));
  if constexpr (OP == TOP_fp2_neg) t_put2(r, 0, fp2_neg(t_f2(x, 0)));
  if constexpr (OP == TOP_fp2_inv) t_put2(r, 0, fp2_inv(t_f2(x, 0)));
  if constexpr (OP == TOP_fp2_3u_p_2x) t_put2(r, 0, fp2_3u_pm_2x(t_f2(x, 0), t_f2(x, 2), false));
  if constexpr (OP == TOP_fp2_3u_m_2x) t_put2(r, 0, fp2_3u_pm_2x(t_f2(x, 0), t_f2(x, 2), true));
  if constexpr (OP == TOP_kara6_c0) t_put2(r, 0, kara6_c0(t_f2(x, 0), t_f2(x, 2), t_f2(x, 4), t_f2(x, 6), KP16()));
  if constexpr (OP == TOP_kara6_c1) t_put2(r, 0, kara6_c1(t_f2(x, 0), t_f2(x, 2), t_f2(x, 4), t_f2(x, 6), KP16()));
  if constexpr (OP == TOP_kara6_c2) t_put2(r, 0, kara6_c2(t_f2(x, 0), t_f2(x, 2), t_f2(x, 4), t_f2(x, 6), KP16()));
  if constexpr (OP == TOP_fp6_mul_lin) t_put6(r, 0, fp6_mul_lin(t_f6(x, 0), t_f6(x, 6), KP16()));
  if constexpr (OP == TOP_fp6_mul) t_put6(r, 0, fp6_mul(t_f6(x, 0), t_f6(x, 6)));
  if constexpr (OP == TOP_fp6_sqr) t_put6(r, 0, fp6_sqr(t_f6(x, 0)));
  if constexpr (OP == TOP_fp6_mul_by_01) t_put6(r, 0, fp6_mul_by_01(t_f6(x, 0), t_f2(x, 6), t_f2(x, 8)));
  if constexpr (OP == TOP_fp6_mul_by_1) t_put6(r, 0, fp6_mul_by_1(t_f6(x, 0), t_f2(x, 6)));
  if constexpr (OP == TOP_fp6_mul_by_12) t_put6(r, 0, fp6_mul_by_12(t_f6(x, 0), t_f2(x, 6), t_f2(x, 8)));
  if constexpr (OP == TOP_fp6_inv) t_put6(r, 0, fp6_inv(t_f6(x, 0)));
  if constexpr (OP == TOP_fp4_sqr_k7) {
    const fp4 y = fp4_sqr_k7(fp4{t_f2(x, 0), t_f2(x, 2)});
    t_put2(r, 0, y.a), t_put2(r, 2, y.b);
  }
  if constexpr (OP == TOP_fp12_mul) t_put12(r, 0, fp12_mul(t_f12(x, 0), t_f12(x, 12)));
  if constexpr (OP == TOP_fp12_sqr) t_put12(r, 0, fp12_sqr(t_f12(x, 0)));
  if constexpr (OP == TOP_fp12_sqr_lin) t_put12(r, 0, fp12_sqr_lin(t_f12(x, 0), KP16()));
  if constexpr (OP == TOP_fp12_mul_by_014)
    t_put12(r, 0, fp12_mul_by_014(t_f12(x, 0), t_f2(x, 12), t_f2(x, 14), t_f2(x, 16)));
  if constexpr (OP == TOP_line_mul_line)
    t_put12(r, 0, line_mul_line(line{t_f2(x, 0), t_f2(x, 2), t_f2(x, 4)}, line{t_f2(x, 6), t_f2(x, 8), t_f2(x, 10)}));
  if constexpr (OP == TOP_fp12_cyclotomic_sqr) t_put12(r, 0, fp12_cyclotomic_sqr(t_f12(x, 0)));
  if constexpr (OP == TOP_fp12_frob) t_put12(r, 0, fp12_frob(t_f12(x, 0)));
  if constexpr (OP == TOP_fp12_frob2) t_put12(r, 0, fp12_frob2(t_f12(x, 0)));
  if constexpr (OP == TOP_fp12_conj) t_put12(r, 0, fp12_conj(t_f12(x, 0)));
  if constexpr (OP == TOP_fp12_inv) t_put12(r, 0, fp12_inv(t_f12(x, 0)));
}

}  // namespace bls
