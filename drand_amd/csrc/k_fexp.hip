// Stage 4: final exponentiation and the == 1 test, one lane per beacon. kilic Engine.Check [ext].
// Six launches per chunk (pairing.h fexp_easy / fexp_step<0..4>, the verdict as fexp_step4_is_one), each
// holding at most two Fp12 values in registers; intermediate Fp12 values live in HBM staging buffers (SoA, 576 B per beacon)
// and are re-read at each use, which keeps every kernel free of scratch spills.
#include "kcommon.h"

namespace blsk {

// Every kernel here works on a range of m items of a pass whose SoA staging has stride n: F, G, cls (and
// X, C, OUT below) point at the range's first column, so item i of the range is column i of stride n.
BLS_KERNEL(BLS_WPE_FEXP) k_fexp_easy(const uint32_t* F, size_t n, size_t m, const uint8_t* cls, uint32_t* G) {
  size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= m || cls[i] != REJ_OK) return;
  st_fp12(G, n, i, fexp_easy(ld_fp12(F, n, i)));
}

// ------------------------------------------------------------------ 3-lane hard part (tri.h)
// Same fexp_step<MODE> sequence, each Fp12 spread over 3 lanes (Fp4 thirds): the 63 cyclotomic
// squares per exponentiation are call-free (3 in-place Fp2 squares per lane), the 5 multiplications
// use the called Fp2 product. 21 beacons per wave.
#ifndef BLS_WPE_FEXP_TRI
#define BLS_WPE_FEXP_TRI 2
#endif

// Park slot of the staged products (tri.h tri_mul_lp): 48 words per lane of the grid.
struct TriPark {
  uint32_t* p;
  size_t n, i;
};

// cube(r) receives X^3, the running value after the first square and product (pairing.h
// fp12_pow_x_abs_reload): the caller stores it at once, nothing of it stays live over the later squares
template <typename LoadX, typename Cube>
DI fp4 tri_pow_x_abs(const tri_lane& t, LoadX lx, const TriPark& pk, Cube cube) {
  constexpr uint64_t NSQ = 1ull | (2ull << 6) | (3ull << 12) | (9ull << 18) | (32ull << 24) | (16ull << 30);
  fp4 r = lx();
#pragma unroll 1
  for (int s = 0; s < 6; s++) {
    const int n = (int)((NSQ >> (6 * s)) & 63u);
#pragma unroll 1
    for (int k = 0; k < n; k++) r = tri_cyclotomic_sqr(t, r);
    if (s < 5) r = tri_mul_lp(t, r, lx(), pk.p, pk.n, pk.i);
    if (s == 0) cube(r);
  }
  return r;
}

// fexp_step<MODE> on thirds: X^|x| by 63 Granger-Scott squares and 5 products (tri_pow_x_abs), then
// the step's own products. Measured and not kept (same-box A/B, 1M beacons, profiles/r03j_*): a
// Karabina compressed squaring chain on 2 lanes + batch decompression (162.8 ms against 160.9) and
// the A0 / (A1, A2) halves of the squaring as two one-lane kernels (169.6 ms); git history holds them.
template <int MODE>
BLS_KERNEL(BLS_WPE_FEXP_TRI) k_fexp_tri(const uint32_t* X, const uint32_t* C, uint32_t* G3, size_t n, size_t m,
                                        uint8_t* cls, uint32_t* OUT, uint32_t* park) {
  const tri_lane t = tri_lane_id();
#if BLS_CSQR_LIN
  kp_lds_init<11>();
#endif
  const size_t ir = (size_t)blockIdx.x * TRI_GROUPS + t.group;
  const bool in_range = t.group < TRI_GROUPS && ir < m;
  const size_t i0 = in_range ? ir : m - 1;  // dummy lanes compute on a real row, never store
  const bool live = in_range && cls[i0] == REJ_OK;
  const TriPark pk = {park, (size_t)gridDim.x * TPB, (size_t)blockIdx.x * TPB + t.lane};
  // every lane stays active to the end (ds_bpermute reads its partners' registers)
  auto at = [&](const uint32_t* B) {
    size_t j = i0;
    asm volatile("" : "+v"(j));  // re-read at each use, never hoisted (a hoisted Fp12 pins its registers)
    return tri_load(B, n, j, t.role);
  };
  // MODE 0 (X = g) writes g^3 to G3, MODE 4 reads it there
  auto cube = [&](const fp4& g3) {
    if (MODE == 0 && live) tri_store(G3, n, i0, t.role, g3);
  };
  fp4 r = tri_conj(t, tri_pow_x_abs(t, [&]() { return at(X); }, pk, cube));
  if (MODE == 0 || MODE == 1) r = tri_mul_lp(t, r, tri_conj(t, at(X)), pk.p, pk.n, pk.i);
  if (MODE == 2) r = tri_mul_lp(t, r, tri_frob(t, at(X)), pk.p, pk.n, pk.i);
  if (MODE < 4) {
    if (live) tri_store(OUT, n, i0, t.role, r);
  }
  if (MODE == 4) {
    // e = r c^(p^4) with r = t^x g^3, and e == 1 <=> r == conj(c^(p^4)) (pairing.h fexp_step4_is_one)
    r = tri_mul_lp(t, r, at(G3), pk.p, pk.n, pk.i);
    const bool one = tri_eq(t, r, tri_conj(t, tri_frob4(t, at(C)))) & !tri_is_zero(t, r);
    if (live && t.role == 0 && !one) cls[i0] = REJ_PAIRING;
    if (OUT) {  // the final value too (blsv_test_final_exp, the timelock paths)
      r = tri_mul_lp(t, r, tri_frob4(t, at(C)), pk.p, pk.n, pk.i);
      if (live) tri_store(OUT, n, i0, t.role, r);
    }
  }
}

// ------------------------------------------------------------------ launchers
// The m items [base, base + m) of a pass whose staging has stride n. F (Miller output) is consumed by
// the easy part and then reused as scratch; W holds 3 more Fp12 staging slots of n entries each (S0,
// S1, S2). g^3 takes no slot of its own: step 0 writes it to S1, which nothing has written yet in
// this pass, and b, which used to sit there, goes to S0 once step 0 has read g for the last time:
//   easy g -> S0 | 0: a -> F, g^3 -> S1 | 1: b -> S0 | 2: c -> S2 | 3: t -> F | 4: reads F, S2, S1
// Every slot is addressed by the same base and stride, so only the range's columns of F, W, cls and
// out are touched and two disjoint ranges of one pass may run side by side on two streams, each with
// a park area of its own. park: FEXP_PARK_WORDS(m) words for the 3-lane products' parked partial
// results.
void launch_final_exp(uint32_t* F, uint32_t* W, size_t n, size_t base, size_t m, uint8_t* cls, hipStream_t st,
                      uint32_t* park, uint32_t* out) {
  if (!m) return;
  F += base;
  cls += base;
  if (out) out += base;
  uint32_t* S0 = W + base;
  uint32_t* S1 = S0 + n * F_WORDS;
  uint32_t* S2 = S0 + 2 * n * F_WORDS;
  const dim3 grid(grid_for(m)), blk(TPB);
  hipLaunchKernelGGL(k_fexp_easy, grid, blk, 0, st, F, n, m, cls, S0);
  const dim3 tgrid((unsigned)((m + TRI_GROUPS - 1) / TRI_GROUPS));
  hipLaunchKernelGGL(k_fexp_tri<0>, tgrid, blk, 0, st, S0, nullptr, S1, n, m, cls, F, park);       // a -> F, g^3 -> S1
  hipLaunchKernelGGL(k_fexp_tri<1>, tgrid, blk, 0, st, F, nullptr, nullptr, n, m, cls, S0, park);   // b -> S0
  hipLaunchKernelGGL(k_fexp_tri<2>, tgrid, blk, 0, st, S0, nullptr, nullptr, n, m, cls, S2, park);  // c -> S2
  hipLaunchKernelGGL(k_fexp_tri<3>, tgrid, blk, 0, st, S2, nullptr, nullptr, n, m, cls, F, park);   // t -> F
  hipLaunchKernelGGL(k_fexp_tri<4>, tgrid, blk, 0, st, F, S2, S1, n, m, cls, out, park);
}

}  // namespace blsk
