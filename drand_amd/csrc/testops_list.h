// The list of raw operation hooks (testops.h holds the operations): BLS_TEST_OPS(X) with
// X(name, Fp elements in, Fp elements out, kind); kinds as described in testops.h. No device code here,
// so the host side of the library (testhooks.cpp) can include it.
#pragma once

#define BLS_TEST_OPS(X)                                                                              \
  X(fp_mul, 2, 1, 0) X(fp_mul_inl, 2, 1, 0) X(fp_sqr, 1, 1, 0) X(fp_add, 2, 1, 0) X(fp_sub, 2, 1, 0) \
  X(fp_addsub_add, 2, 1, 0) X(fp_addsub_sub, 2, 1, 0) X(fp_neg, 1, 1, 0) X(fp_half, 1, 1, 0)         \
  X(fp_dbl, 1, 1, 0) X(fp_mul3, 1, 1, 0) X(fp_add_lazy_mul, 3, 2, 0) X(fp_add_lazy2_mul, 5, 2, 0)   \
  X(fp_canon, 1, 1, 0) X(fp_is_zero, 1, 1, 0) X(fp_eq, 2, 1, 0) X(fp_inv_bingcd_raw, 1, 2, 0)        \
  X(fp_inv, 1, 1, 0) X(fp_pow_sqrt_inv, 1, 1, 0)                                                     \
  X(fp2_mul, 4, 2, 0) X(fp2_mul_inl, 4, 2, 0) X(fp2_mul_inl_kara, 4, 2, 0) X(fp2_sqr, 2, 2, 0)       \
  X(fp2_sqr_inl, 2, 2, 0) X(fp2_mul_xi, 2, 2, 0) X(fp2_neg, 2, 2, 0) X(fp2_inv, 2, 2, 0)             \
  X(fp2_3u_p_2x, 4, 2, 0) X(fp2_3u_m_2x, 4, 2, 0) X(fp2_3u_p_2x_lds, 4, 2, 1)                        \
  X(fp2_3u_m_2x_lds, 4, 2, 1) X(kara6_c0, 8, 2, 0) X(kara6_c1, 8, 2, 0) X(kara6_c2, 8, 2, 0)         \
  X(fp6_mul_lin, 12, 6, 0) X(fp6_mul, 12, 6, 0) X(fp6_sqr, 6, 6, 0) X(fp6_mul_by_01, 10, 6, 0)       \
  X(fp6_mul_by_1, 8, 6, 0) X(fp6_mul_by_12, 10, 6, 0) X(fp6_inv, 6, 6, 0) X(fp4_sqr_k7, 4, 4, 0)     \
  X(fp4_sqr_dot, 4, 4, 1) X(fp4_mul, 8, 4, 1) X(fp12_mul, 24, 12, 0) X(fp12_sqr, 12, 12, 0)          \
  X(fp12_sqr_lin, 12, 12, 0) X(fp12_mul_by_014, 18, 12, 0) X(line_mul_line, 12, 12, 0)               \
  X(fp12_cyclotomic_sqr, 12, 12, 0) X(fp12_frob, 12, 12, 0) X(fp12_frob2, 12, 12, 0)                 \
  X(fp12_conj, 12, 12, 0) X(fp12_inv, 12, 12, 0)                                                     \
  X(fp6_mul_lb, 12, 6, 2) X(fp12_mul_by_line_pair_lds, 22, 12, 2)                                    \
  X(tri_cyclotomic_sqr, 12, 12, 3) X(tri_mul_lp, 24, 12, 3) X(tri_sqr_lp, 12, 12, 3)                 \
  X(tri_line_pair, 12, 12, 3) X(tri_frob, 12, 12, 3) X(tri_frob2, 12, 12, 3) X(tri_conj, 12, 12, 3)  \
  X(tri_is_one, 12, 1, 3)

namespace bls {

enum TestOp : int {
#define X(name, nin, nout, kind) TOP_##name,
  BLS_TEST_OPS(X)
#undef X
      TOP_COUNT
};

struct TestOpInfo {
  const char* name;
  int nin, nout, kind;
};
inline const TestOpInfo* test_op_table() {
  static const TestOpInfo tab[TOP_COUNT] = {
#define X(name, nin, nout, kind) {#name, nin, nout, kind},
      BLS_TEST_OPS(X)
#undef X
  };
  return tab;
}

}  // namespace bls
