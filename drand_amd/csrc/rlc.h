// Randomized batch verification of beacons that share one group key (opt-in, blsv_verify_*_rlc).
//   prod_i [ e(pk, H_i) e(-g1, sigma_i) ]^{r_i} = e(pk, sum r_i H_i) e(-g1, sum r_i sigma_i)
// so a group of G consecutive items shares one two-pair pairing check on A = sum r_i H_i and
// B = sum r_i sigma_i, with 64-bit r_i the verifier draws after it has seen the items.
//
// Contract (include/blsverify.h):
//   * a reject is always the exact pipeline's reject: the items of a group whose check fails are run
//     through the exact Miller and final-exponentiation stages, decode rejects (classes 2..6) never
//     enter a sum, so verdicts, classes and first_bad of every rejected item equal the exact path's;
//   * an invalid item is accepted only if its group's check passes, with probability at most 2^-64
//     over the seed. The bound needs every sigma_i in the order-r subgroup, which the decompression
//     stage has already checked (an element of another order could cancel with probability 1/order);
//   * an adversary who puts one bad round in every group forces the exact cost plus this stage.
//
// r_i = first 8 bytes, big-endian, of SHA-256(seed || BE64(i)), i the item's index within the call;
// the 32-byte seed comes from the OS CSPRNG once per call and never leaves the library.
//
// This header holds the scalar derivation and the per-lane accumulation as DI functions that also
// compile for the host (tools/opcount rlc); k_rlc.hip holds the kernels.
// One lane accumulates RLC_LANE_ITEMS consecutive items of ONE of the two sums bit-serially: 64
// doublings shared by its items, and per bit and item one mixed addition whose result a select keeps
// or drops (a predicated addition costs a wave its full price whatever the bit). The additions are
// complete: sigma_i are the adversary's, may repeat or be negated, and an early partial sum can equal
// an input point (acc == +-P and acc at infinity take madd-2007-bl's exceptional branch, as
// g2_madd_inl). The group's lanes are then summed with jac_add (complete as well).
#pragma once
#include "hash.h"

namespace bls {

constexpr int RLC_LANE_ITEMS = 8;  // divides every group size (a power of two >= 8)

// seed as eight big-endian words
DI uint64_t rlc_scalar(const uint32_t (&seed)[8], uint64_t i) {
  uint32_t st[8], blk[16];
  sha256_init(st);
#pragma unroll
  for (int k = 0; k < 8; k++) blk[k] = seed[k];
  blk[8] = (uint32_t)(i >> 32);
  blk[9] = (uint32_t)i;
  blk[10] = 0x80000000u;
#pragma unroll
  for (int k = 11; k < 15; k++) blk[k] = 0;
  blk[15] = 40 * 8;
  sha256_compress(st, blk);
  return ((uint64_t)st[0] << 32) | st[1];
}

// p + q, q = (qx(), qy()) affine and never infinity, re-read at each use: madd-2007-bl with the
// in-place Fp2 bodies, every exceptional case handled (p at infinity, p == q, p == -q)
template <typename QX, typename QY>
DI g2j rlc_madd(const g2j& p, QX qx, QY qy) {
  const fp2 Z1Z1 = fp2_sqr_inl(p.z);
  const fp2 S2 = fp2_mul_inl(fp2_mul_inl(qy(), p.z), Z1Z1);
  const fp2 H = fp2_sub(fp2_mul_inl(qx(), Z1Z1), p.x);
  const fp2 r = fp2_dbl(fp2_sub(S2, p.y));
  const fp2 HH = fp2_sqr_inl(H);
  const fp2 I = fp2_dbl(fp2_dbl(HH));
  const fp2 J = fp2_mul_inl(H, I);
  const fp2 V = fp2_mul_inl(p.x, I);
  const fp2 X3 = fp2_sub(fp2_sub(fp2_sqr_inl(r), J), fp2_dbl(V));
  const fp2 Y3 = fp2_sub(fp2_mul_inl(r, fp2_sub(V, X3)), fp2_dbl(fp2_mul_inl(p.y, J)));
  const fp2 Z3 = fp2_sub(fp2_sub(fp2_sqr_inl(fp2_add(p.z, H)), Z1Z1), HH);
  g2j out = {X3, Y3, Z3};
  const bool pinf = jac_is_inf(p), h0 = fp2_is_zero(H);
  if (pinf | h0) {
    if (pinf)
      out = {qx(), qy(), fp2_one()};
    else if (fp2_is_zero(r))
      out = g2_dbl_inl(p);
    else
      out = jac_infinity<fp2>();
  }
  return out;
}

// sum_k r_k P_k over a lane's nk <= RLC_LANE_ITEMS items: px(k), py(k) the affine coordinates of
// item k, bit(k, b) bit b of its scalar (0 throughout for an item that does not contribute: a decode
// reject, or a point at infinity, whose coordinates are then never used)
template <typename PX, typename PY, typename Bit>
DI g2j rlc_accumulate(int nk, PX px, PY py, Bit bit) {
  g2j acc = jac_infinity<fp2>();
#pragma unroll 1
  for (int b = 63; b >= 0; b--) {
    acc = g2_dbl_inl(acc);
#pragma unroll 1
    for (int k = 0; k < nk; k++) {
      const g2j sum = rlc_madd(acc, [&]() { return px(k); }, [&]() { return py(k); });
      acc = jac_select(bit(k, b), sum, acc);
    }
  }
  return acc;
}

// the group's sum over its m lanes' partial sums
template <typename Part>
DI g2j rlc_sum(size_t m, Part part) {
  g2j acc = jac_infinity<fp2>();
#pragma unroll 1
  for (size_t q = 0; q < m; q++) acc = jac_add(acc, part(q));
  return acc;
}

}  // namespace bls
