// Stage 3: two-pair multi-Miller loop e(pk, H) * e(-g1, sigma), one lane per beacon, in two passes
// (pairing.h miller_lines / miller_f_from_lines): k_miller_lines writes the 68 x 2 sparse lines
// to HBM staging (SoA, 6 Fp slots per line), k_miller_f folds them into f. Each pass keeps only its
// own state live, which removes the scratch spills of the fused loop (13.6 KB/lane, ~160 KB of
// scratch traffic per beacon) for 2 x 39 KB of coalesced line traffic per beacon, and lets the
// lines pass run at 2 waves/SIMD (256 VGPRs).
// The lines pass of the pair (-g1, sigma) ends with T = [|x|]sigma, which is what sigma's psi subgroup
// check needs: k_miller_lines<true> closes that check on it (no [|x|]sigma walk of its own in the
// per-item batch path; k_decomp.hip keeps the explicit kernels for the paths that need the verdict first).
// kilic Engine.AddPair / AddPairInv [ext] via kyber-bls12381 ValidatePairing.
#include <type_traits>

#include "kcommon.h"
#include "kmiller.h"
#include "testops.h"

namespace blsk {

// line slot of (step, pair): 6 Fp slots (a0, a1, a4 as Fp2)
DI int line_slot(int step, int k) { return (step * 2 + k) * 6; }
// Item g = base + i of the chunk (H/S/F/cls stride cnt); its lines at LN index i (stride sub).
// The two pairs run in separate workgroups (k = blockIdx.x & 1: the pair of the whole wave), so a
// beacon's two line chains run side by side: half the latency of one lane walking both, twice the
// waves (a finer tail), and every store still one 256-byte access per wave.
// CHECK: the k == 1 workgroups (the pair (-g1, sigma)) also close sigma's psi subgroup check on their
// own T, which is [|x|]sigma when the loop ends (pairing.h miller_t_in_subgroup), and write
// cls[g] = REJ_NOT_IN_SUBGROUP on a failure: the per-item batch path, whose head then only decodes.
// k_miller_f / k_miller_f_tri and the final exponentiation launch later on the same stream and skip
// cls != REJ_OK. The k == 0 workgroup of the same items may read cls[g] before or after that byte
// store; either is correct, since nothing reads the lines of a rejected item. Without CHECK the kernel
// is the plain one (cls read-only): the randomized path's sums of points that were already checked.
template <bool CHECK>
BLS_KERNEL(BLS_WPE_LINES)
k_miller_lines(const uint32_t* pk_tab, const uint8_t* pk_inf, const uint32_t* pk_idx, const uint32_t* H,
               const uint8_t* h_inf, const uint32_t* S, const uint8_t* s_inf,
               std::conditional_t<CHECK, uint8_t*, const uint8_t*> cls, size_t cnt, size_t base, size_t m, size_t sub,
               uint32_t* LN) {
  const int k = (int)(blockIdx.x & 1u);
  const size_t i = (size_t)(blockIdx.x >> 1) * TPB + threadIdx.x;
  if (i >= m) return;
  const size_t g = base + i;
  if (cls[g] != REJ_OK) return;
  const uint32_t kk = pk_idx ? pk_idx[g] : 0u;
  const bool act[2] = {!(pk_inf[kk] | h_inf[g]), !s_inf[g]};
  {
    const uint32_t* Qb = k == 0 ? H : S;
    auto load_q = [&]() {
      size_t j = g;
      asm volatile("" : "+v"(j));  // re-read at each use (5 additions), never hoisted
      return g2a{ld_fp2(Qb, cnt, j, 0), ld_fp2(Qb, cnt, j, 2)};
    };
    auto emit = [&](int step, const line& l) {
      const int s = line_slot(step, k);
      const line o = act[k] ? l : line_one();
      st_fp2<BLS_LN_AUX_ST>(LN, sub, i, s + 0, o.a0);
      st_fp2<BLS_LN_AUX_ST>(LN, sub, i, s + 2, o.a1);
      st_fp2<BLS_LN_AUX_ST>(LN, sub, i, s + 4, o.a4);
    };
    // call-free steps (pairing.h miller_dbl_step_inl): P, Q and the lines never live across a call
    auto pcoord = [&](int c) {
      size_t o = (size_t)kk * G1_WORDS + 12 * c;
      asm volatile("" : "+v"(o));  // re-read at the use
      fp v;
#pragma unroll
      for (int w = 0; w < 12; w++) v.l[w] = pk_tab[o + w];
      return k == 0 ? v : fp_load_const(c == 0 ? G1_GEN_X : G1_GEN_NEG_Y);
    };
    if (!act[k]) {  // a skipped pair (a point at infinity) contributes the line 1 at every step
#pragma unroll 1
      for (int s = 0; s < MILLER_STEPS; s++) emit(s, line_one());
      return;
    }
    int step = 0;
    auto put = [&](int c, const fp2& v) { st_fp2<BLS_LN_AUX_ST>(LN, sub, i, line_slot(step, k) + 2 * c, v); };
    auto xp = [&]() { return pcoord(0); };
    auto yp = [&]() { return pcoord(1); };
    // T parks in LDS (72 words per lane, word-major: 18 KB per one-wave workgroup, 8 per CU at 2
    // waves/SIMD), read at each use and written back coordinate by coordinate
    const g2proj_lds T{g_ml_T + threadIdx.x};
    {
      const g2a Q0 = load_q();
      T.set(0, Q0.x);
      T.set(1, Q0.y);
      T.set(2, fp2_one());
    }
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
      miller_dbl_step_ts(T, put, xp, yp);
      step++;
      if ((BLS_X_ABS >> b) & 1ull) {
        miller_add_step_ts(T, load_q, put, xp, yp);
        step++;
      }
    }
    if constexpr (CHECK) {
      // k is uniform over the workgroup: no divergence with the other pair
      if (k == 1 && !miller_t_in_subgroup(T, load_q)) {
        size_t j = g;
        asm volatile("" : "+v"(j));  // the byte's address formed here, not kept across the loop
        cls[j] = REJ_NOT_IN_SUBGROUP;
      }
    }
  }
}

// The line-pair product L (5 Fp2: c0.c0, c0.c1, c0.c2, c1.c1, c1.c2) of the current step parks in LDS
// (one 120-word column per lane: 30 KB per one-wave workgroup, 4 per CU with g_fp2_arg) and is read
// back at each use, so f (144 words) and the partial products are all that stay in registers.
static __shared__ uint32_t g_mf_L[120 * BLS_LANES];
DI void mf_put(int c, const fp2& v) {
  const unsigned l = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    g_mf_L[(c * 24 + k) * BLS_LANES + l] = v.c0.l[k];
    g_mf_L[(c * 24 + 12 + k) * BLS_LANES + l] = v.c1.l[k];
  }
}
DI fp2 mf_get(int c) {
  unsigned l = threadIdx.x;
  asm volatile("" : "+v"(l));  // read at the use, never kept live
  fp2 v;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    v.c0.l[k] = g_mf_L[(c * 24 + k) * BLS_LANES + l];
    v.c1.l[k] = g_mf_L[(c * 24 + 12 + k) * BLS_LANES + l];
  }
  return v;
}
// fp6_mul(a, b) (tower.h, Karatsuba) with b's components read through lb
template <typename LB>
DI fp6 fp6_mul_lb(const fp6& a, LB lb) {
#if BLS_F6_LIN
  return fp6_mul_lin_lb(a, lb, KpLds16());
#else
  fp2 t0 = fp2_mul(a.c0, lb(0));
  fp2 t1 = fp2_mul(a.c1, lb(1));
  fp2 t2 = fp2_mul(a.c2, lb(2));
  fp2 c0 = fp2_add(fp2_mul_xi(fp2_sub(fp2_sub(fp2_mul(fp2_add_lazy(a.c1, a.c2), fp2_add_lazy(lb(1), lb(2))), t1), t2)), t0);
  fp2 c1 = fp2_add(fp2_sub(fp2_sub(fp2_mul(fp2_add_lazy(a.c0, a.c1), fp2_add_lazy(lb(0), lb(1))), t0), t1), fp2_mul_xi(t2));
  fp2 c2 = fp2_add(fp2_sub(fp2_sub(fp2_mul(fp2_add_lazy(a.c0, a.c2), fp2_add_lazy(lb(0), lb(2))), t0), t2), t1);
  return {c0, c1, c2};
#endif
}
// pairing.h fp12_mul_by_line_pair with L read from LDS (mf_get)
DI fp12 fp12_mul_by_line_pair_lds(const fp12& f) {
  const fp6 t0 = fp6_mul_lb(f.c0, [](int c) { return mf_get(c); });
  fp6 t1;
  {
    const fp2 b1 = mf_get(3), b2 = mf_get(4);
    t1 = fp6_mul_by_12(f.c1, b1, b2);
  }
  // Ls = (L.c0.c0, L.c0.c1 + L.c1.c1, L.c0.c2 + L.c1.c2)
  const fp6 c1 = fp6_sub(fp6_sub(fp6_mul_lb(fp6_add_lazy(f.c0, f.c1), [](int c) {
                                   return c == 0 ? mf_get(0) : fp2_add_lazy(mf_get(c), mf_get(c + 2));
                                 }),
                                 t0),
                         t1);
  return {fp6_add(t0, fp6_mul_v(t1)), c1};
}

BLS_KERNEL(BLS_WPE_MILLER_F) k_miller_f(const uint32_t* LN, const uint8_t* cls, size_t cnt, size_t base,
                                                  size_t m, size_t sub, uint32_t* F) {
#if BLS_F6_LIN
  kp_lds_init<16>();  // before the early exits: every lane of the workgroup writes its table words
#endif
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= m) return;
  const size_t g = base + i;
  if (cls[g] != REJ_OK) return;
  auto load = [&](int step, int k) {
    const int s = line_slot(step, k);
    return line{ld_fp2<BLS_LN_AUX_LD>(LN, sub, i, s + 0), ld_fp2<BLS_LN_AUX_LD>(LN, sub, i, s + 2),
                ld_fp2<BLS_LN_AUX_LD>(LN, sub, i, s + 4)};
  };
  // miller_f_from_lines (pairing.h) with the line-pair product parked in LDS
  fp12 f = fp12_one();
  int step = 0;
#pragma unroll 1
  for (int b = 62; b >= 0; b--) {
#pragma unroll 1
    for (int rep = 0; rep < 2; rep++) {
      if (rep == 1 && !((BLS_X_ABS >> b) & 1ull)) break;
#if BLS_F6_LIN
      if (rep == 0 && b != 62) f = fp12_sqr_lin(f, KpLds16());
#else
      if (rep == 0 && b != 62) f = fp12_sqr(f);
#endif
      {
        const fp12 L = line_mul_line(load(step, 0), load(step, 1));
        if (step == 0) {  // f = 1 * L: the first line pair is f itself
          f = L;
          step++;
          continue;
        }
        mf_put(0, L.c0.c0);
        mf_put(1, L.c0.c1);
        mf_put(2, L.c0.c2);
        mf_put(3, L.c1.c1);
        mf_put(4, L.c1.c2);
      }
      f = fp12_mul_by_line_pair_lds(f);
      step++;
    }
  }
  st_fp12(F, cnt, g, fp12_conj(f));
}

// ------------------------------------------------------------------ 3-lane f pass (tri.h)
// Same f as k_miller_f, each Fp12 spread over 3 lanes (Fp4 thirds), 21 beacons per wave: per step
// f = f^2 (tri_sqr_lp), L = l_0 l_1 (tri_line_pair: 2 Fp2 products per lane), f = f L (tri_mul_lp).
// Steps s = 0..67 follow miller_f_from_lines; bit s of MILLER_SQ says whether step s squares first.
constexpr uint64_t miller_sq_bits(int half) {
  uint64_t m = 0;
  int s = 0;
  for (int i = 62; i >= 0; i--) {
    if (i != 62 && s / 64 == half) m |= 1ull << (s % 64);
    s++;
    if ((BLS_X_ABS >> i) & 1ull) s++;  // addition step: no squaring
  }
  return m;
}
constexpr uint64_t MILLER_SQ_LO = miller_sq_bits(0), MILLER_SQ_HI = miller_sq_bits(1);

#ifndef BLS_MILLER_TRI_MAX
#define BLS_MILLER_TRI_MAX 65536
#endif
constexpr size_t kMillerTriMax = BLS_MILLER_TRI_MAX;

#ifndef BLS_WPE_MILLER_TRI
#define BLS_WPE_MILLER_TRI 2
#endif

BLS_KERNEL(BLS_WPE_MILLER_TRI) k_miller_f_tri(const uint32_t* LN, const uint8_t* cls, size_t cnt, size_t base,
                                              size_t m, size_t sub, uint32_t* F, uint32_t* park) {
  const tri_lane t = tri_lane_id();
  const size_t ir = (size_t)blockIdx.x * TRI_GROUPS + t.group;
  const bool in_range = t.group < TRI_GROUPS && ir < m;
  const size_t i = in_range ? ir : m - 1;  // dummy lanes compute on a real row, never store
  const bool live = in_range && cls[base + i] == REJ_OK;
  const size_t park_n = (size_t)gridDim.x * TPB, park_i = (size_t)blockIdx.x * TPB + t.lane;
  fp4 A;
#pragma unroll 1
  for (int s = 0; s < MILLER_STEPS; s++) {
    const bool sq = ((s < 64 ? MILLER_SQ_LO >> s : MILLER_SQ_HI >> (s - 64)) & 1ull) != 0;
    if (sq) A = tri_sqr_lp(t, A);
    const int s0 = line_slot(s, 0), s1 = line_slot(s, 1);
    // c is lane-role dependent: the line's 6 slots as one object, the slot in the VGPR offset
    auto la = [&](int c) {
      size_t j = i;
      asm volatile("" : "+v"(j));
      return ld_fp2_v<BLS_LN_AUX_LD>(LN + (size_t)s0 * 12 * sub, sub, j, 2 * c);
    };
    auto lb = [&](int c) {
      size_t j = i;
      asm volatile("" : "+v"(j));
      return ld_fp2_v<BLS_LN_AUX_LD>(LN + (size_t)s1 * 12 * sub, sub, j, 2 * c);
    };
    const fp4 L = tri_line_pair(t, la, lb);
    if (s == 0) {
      A = L;  // f = 1 * L
    } else {
      A = tri_mul_lp(t, A, L, park, park_n, park_i);
    }
  }
  A = tri_conj(t, A);
  if (live) tri_store(F, cnt, base + i, t.role, A);
}

// ------------------------------------------------------------------ raw operation hooks (testops.h kind 2)
// The f pass's own LDS forms on operands the test chooses (raw words, one item per lane, layout as
// k_test.hip k_test_op): fp6_mul_lb reads b through mf_get(0..2); fp12_mul_by_line_pair_lds takes f
// (12 Fp) and the five Fp2 of L (c0.c0, c0.c1, c0.c2, c1.c1, c1.c2) that k_miller_f parks with mf_put.
template <int OP, int NIN, int NOUT>
__global__ void __launch_bounds__(TPB) k_test_op_mf(const uint32_t* in, size_t cnt, uint32_t* out) {
#if BLS_F6_LIN
  kp_lds_init<16>();
#endif
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  fp x[NIN], r[NOUT];
#pragma unroll
  for (int k = 0; k < NIN; k++)
#pragma unroll
    for (int w = 0; w < 12; w++) x[k].l[w] = in[(i * NIN + k) * 12 + w];
  if constexpr (OP == TOP_fp6_mul_lb) {
#pragma unroll
    for (int c = 0; c < 3; c++) mf_put(c, t_f2(x, 6 + 2 * c));
    t_put6(r, 0, fp6_mul_lb(t_f6(x, 0), [](int c) { return mf_get(c); }));
  } else {
#pragma unroll
    for (int c = 0; c < 5; c++) mf_put(c, t_f2(x, 12 + 2 * c));
    t_put12(r, 0, fp12_mul_by_line_pair_lds(t_f12(x, 0)));
  }
#pragma unroll
  for (int k = 0; k < NOUT; k++)
#pragma unroll
    for (int w = 0; w < 12; w++) out[(i * NOUT + k) * 12 + w] = r[k].l[w];
}

bool launch_test_op_mf(int op, const uint32_t* in, size_t cnt, uint32_t* out, hipStream_t st) {
  if (op != TOP_fp6_mul_lb && op != TOP_fp12_mul_by_line_pair_lds) return false;
  if (!cnt) return true;
  if (op == TOP_fp6_mul_lb)
    hipLaunchKernelGGL((k_test_op_mf<TOP_fp6_mul_lb, 12, 6>), dim3(grid_for(cnt)), dim3(TPB), 0, st, in, cnt, out);
  else
    hipLaunchKernelGGL((k_test_op_mf<TOP_fp12_mul_by_line_pair_lds, 22, 12>), dim3(grid_for(cnt)), dim3(TPB), 0, st, in,
                       cnt, out);
  return true;
}

// ------------------------------------------------------------------ launchers
// The line staging (MILLER_LINE_WORDS per beacon) holds `sub` beacons: item g of the pass has its lines
// at LN index g % sub.
// The lines pass of the m items [base, base + m) of a pass of cnt items, base a multiple of sub and
// m <= sub.
void launch_miller_lines(const uint32_t* pk_tab, const uint8_t* pk_inf, const uint32_t* pk_idx, const uint32_t* H,
                         const uint8_t* h_inf, const uint32_t* S, const uint8_t* s_inf, uint8_t* cls, size_t cnt,
                         size_t base, size_t m, uint32_t* LN, size_t sub, bool check_subgroup, hipStream_t st) {
  if (!m) return;
  if (check_subgroup)
    hipLaunchKernelGGL(k_miller_lines<true>, dim3(2 * grid_for(m)), dim3(TPB), 0, st, pk_tab, pk_inf, pk_idx, H, h_inf,
                       S, s_inf, cls, cnt, base, m, sub, LN);
  else
    hipLaunchKernelGGL(k_miller_lines<false>, dim3(2 * grid_for(m)), dim3(TPB), 0, st, pk_tab, pk_inf, pk_idx, H,
                       h_inf, S, s_inf, (const uint8_t*)cls, cnt, base, m, sub, LN);
}

// The f pass of the m items [base, base + m), all inside one sub-chunk of the line staging: the kernels
// index the lines from 0, so LN moves to the range's first column (base % sub; the slot resources of
// soa.h then end that many words later, still inside the next slot or the buffer's own last one, and
// no lane reaches past column m).
void launch_miller_f(const uint32_t* LN, size_t sub, const uint8_t* cls, size_t cnt, size_t base, size_t m,
                     uint32_t* F, uint32_t* park, bool single_lane, hipStream_t st) {
  if (!m) return;
  LN += base % sub;
  // Below one full wave round of the single-lane pass (1 wave/SIMD x 1024 SIMDs x 64 lanes) the GPU is
  // not full and latency decides: the 3-lane pass runs 27.6 k instructions per lane-step against
  // 73.7 k. At full occupancy the single-lane pass has the higher throughput (profiles/r02_*), and so
  // it has for a small range that shares the GPU with other work (single_lane).
  if (m <= kMillerTriMax && !single_lane) {
    hipLaunchKernelGGL(k_miller_f_tri, dim3((unsigned)((m + TRI_GROUPS - 1) / TRI_GROUPS)), dim3(TPB), 0, st, LN, cls,
                       cnt, base, m, sub, F, park);
  } else {
    hipLaunchKernelGGL(k_miller_f, dim3(grid_for(m)), dim3(TPB), 0, st, LN, cls, cnt, base, m, sub, F);
  }
}

// Both passes over a whole pass, in sub-chunks of the line staging (one when sub >= cnt, which is what
// the host does: every sub-chunk adds a wave tail to both passes).
void launch_miller(const uint32_t* pk_tab, const uint8_t* pk_inf, const uint32_t* pk_idx, const uint32_t* H,
                   const uint8_t* h_inf, const uint32_t* S, const uint8_t* s_inf, uint8_t* cls, size_t cnt,
                   uint32_t* F, uint32_t* LN, size_t sub, uint32_t* park, bool check_subgroup, hipStream_t st) {
  if (!cnt) return;
  for (size_t b = 0; b < cnt; b += sub) {
    const size_t m = cnt - b < sub ? cnt - b : sub;
    launch_miller_lines(pk_tab, pk_inf, pk_idx, H, h_inf, S, s_inf, cls, cnt, b, m, LN, sub, check_subgroup, st);
    launch_miller_f(LN, sub, cls, cnt, b, m, F, park, false, st);
  }
}

}  // namespace blsk
