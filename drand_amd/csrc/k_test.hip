// Raw building-block test hooks (parity tests against the CPU oracle; not used by the product path).
#include "kcommon.h"
#include "testops.h"

namespace blsk {

// ------------------------------------------------------------------ test hooks
__global__ void k_test_fp_mul(const uint32_t* a, const uint32_t* b, size_t cnt, uint32_t* out) {
  size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  fp x, y;
#pragma unroll
  for (int w = 0; w < 12; w++) {
    x.l[w] = a[i * 12 + w];
    y.l[w] = b[i * 12 + w];
  }
  fp r = fp_from_mont(fp_mul(fp_to_mont(x), fp_to_mont(y)));
#pragma unroll
  for (int w = 0; w < 12; w++) out[i * 12 + w] = r.l[w];
}

// raw affine P (24 words: x, y) and Q (48 words: x.c0, x.c1, y.c0, y.c1) -> e(P, Q)^3 raw (144 words,
// tower order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1)
__global__ void __launch_bounds__(TPB) k_test_pairing(const uint32_t* p_tab, const uint32_t* q_aff, size_t cnt,
                                                      uint32_t* out_f) {
  size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  fp v[6];
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int w = 0; w < 12; w++) v[s].l[w] = p_tab[i * 24 + s * 12 + w];
  g1a P1[1] = {{fp_to_mont(v[0]), fp_to_mont(v[1])}};
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int w = 0; w < 12; w++) v[s].l[w] = q_aff[i * 48 + s * 12 + w];
  g2a Q1[1] = {{{fp_to_mont(v[0]), fp_to_mont(v[1])}, {fp_to_mont(v[2]), fp_to_mont(v[3])}}};
  bool act[1] = {true};
  fp12 f = final_exponentiation(miller_loop_multi<1>(P1, Q1, act));
  const fp2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
#pragma unroll
  for (int s = 0; s < 6; s++) {
    fp r0 = fp_from_mont(c[s]->c0), r1 = fp_from_mont(c[s]->c1);
#pragma unroll
    for (int w = 0; w < 12; w++) {
      out_f[i * 144 + s * 24 + w] = r0.l[w];
      out_f[i * 144 + s * 24 + 12 + w] = r1.l[w];
    }
  }
}

// SoA Montgomery affine G2 staging -> raw AoS words (x.c0, x.c1, y.c0, y.c1)
__global__ void k_test_unpack_g2(const uint32_t* H, size_t cnt, uint32_t* out) {
  size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    fp v = fp_from_mont(ld_fp(H, cnt, i, s));
#pragma unroll
    for (int w = 0; w < 12; w++) out[i * 48 + s * 12 + w] = v.l[w];
  }
}

// raw AoS Fp12 (144 words, tower order) <-> Montgomery SoA staging (soa.h slot order is the same)
__global__ void k_test_pack_fp12(const uint32_t* f, size_t cnt, uint32_t* F) {
  size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  for (int s = 0; s < 12; s++) {
    fp v;
#pragma unroll
    for (int w = 0; w < 12; w++) v.l[w] = f[i * 144 + s * 12 + w];
    st_fp(F, cnt, i, s, fp_to_mont(v));
  }
}

__global__ void k_test_unpack_fp12(const uint32_t* F, size_t cnt, uint32_t* out) {
  size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  for (int s = 0; s < 12; s++) {
    fp v = fp_from_mont(ld_fp(F, cnt, i, s));
#pragma unroll
    for (int w = 0; w < 12; w++) out[i * 144 + s * 12 + w] = v.l[w];
  }
}

// one-lane register final exponentiation (pairing.h final_exponentiation) on SoA staging
__global__ void __launch_bounds__(TPB) k_test_final_exp_ref(const uint32_t* F, size_t cnt, uint32_t* out) {
  size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  st_fp12(out, cnt, i, final_exponentiation(ld_fp12(F, cnt, i)));
}

// ------------------------------------------------------------------ raw operation hooks (testops.h)
// One item per lane: item i's NIN operands at in[(i * NIN + k) * 12], its NOUT results at
// out[(i * NOUT + k) * 12], raw words both ways. Both LDS tables of k p are written first, by every
// lane of the workgroup, as the production kernels do before their early exits.
template <int OP, int NIN, int NOUT>
__global__ void __launch_bounds__(TPB) k_test_op(const uint32_t* in, size_t cnt, uint32_t* out) {
  kp_lds_init<11>();
  kp_lds_init<16>();
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= cnt) return;
  fp x[NIN], r[NOUT];
#pragma unroll
  for (int k = 0; k < NIN; k++)
#pragma unroll
    for (int w = 0; w < 12; w++) x[k].l[w] = in[(i * NIN + k) * 12 + w];
  if constexpr (OP == TOP_fp2_3u_p_2x_lds) t_put2(r, 0, fp2_3u_pm_2x(t_f2(x, 0), t_f2(x, 2), false, KpLdsK<11>()));
  else if constexpr (OP == TOP_fp2_3u_m_2x_lds) t_put2(r, 0, fp2_3u_pm_2x(t_f2(x, 0), t_f2(x, 2), true, KpLdsK<11>()));
  else if constexpr (OP == TOP_fp4_sqr_dot) {
    const fp4 y = fp4_sqr_dot(fp4{t_f2(x, 0), t_f2(x, 2)});
    t_put2(r, 0, y.a), t_put2(r, 2, y.b);
  } else if constexpr (OP == TOP_fp4_mul) {
    const fp4 y = fp4_mul(fp4{t_f2(x, 0), t_f2(x, 2)}, fp4{t_f2(x, 4), t_f2(x, 6)});
    t_put2(r, 0, y.a), t_put2(r, 2, y.b);
  } else
    test_op_run<OP, KpLdsK<16>>(x, r);
#pragma unroll
  for (int k = 0; k < NOUT; k++)
#pragma unroll
    for (int w = 0; w < 12; w++) out[(i * NOUT + k) * 12 + w] = r[k].l[w];
}

// Three lanes per item (tri.h): item i's operands are NIN / 12 Fp12 values (or two sparse lines of 6 Fp
// for tri_line_pair) of 12 Fp in tower order, which is soa.h's slot order; the lane of role j reads and
// writes its third (tri_slot_a / tri_slot_b). Lanes without an item (lane 63, the tail of the last
// wave) compute on item cnt - 1 and never store. The LDS table and the park buffer (TRI_PARK_WORDS(cnt)
// words) are those of k_fexp_tri / k_miller_f_tri.
template <int OP, int NIN, int NOUT>
__global__ void __launch_bounds__(TPB) k_test_tri(const uint32_t* in, size_t cnt, uint32_t* out, uint32_t* park) {
  const tri_lane t = tri_lane_id();
  kp_lds_init<11>();
  const size_t ir = (size_t)blockIdx.x * TRI_GROUPS + t.group;
  const bool live = t.group < TRI_GROUPS && ir < cnt;
  const size_t i = live ? ir : cnt - 1;
  const size_t park_n = (size_t)gridDim.x * TPB, park_i = (size_t)blockIdx.x * TPB + t.lane;
  auto ld2 = [&](int base, int slot) {  // Fp2 at Fp index base + slot of item i
    fp2 v;
    const uint32_t* q = in + (i * NIN + base + slot) * 12;
#pragma unroll
    for (int w = 0; w < 12; w++) v.c0.l[w] = q[w], v.c1.l[w] = q[12 + w];
    return v;
  };
  auto ld4 = [&](int base) { return fp4{ld2(base, tri_slot_a(t.role)), ld2(base, tri_slot_b(t.role))}; };
  if constexpr (OP == TOP_tri_is_one) {
    const bool one = tri_is_one(t, ld4(0));
    if (live && t.role == 0) {
      for (int w = 0; w < 12; w++) out[i * 12 + w] = w == 0 && one ? 1u : 0u;
    }
    return;
  } else {
    fp4 y;
    if constexpr (OP == TOP_tri_cyclotomic_sqr) y = tri_cyclotomic_sqr(t, ld4(0));
    if constexpr (OP == TOP_tri_mul_lp) y = tri_mul_lp(t, ld4(0), ld4(12), park, park_n, park_i);
    if constexpr (OP == TOP_tri_sqr_lp) y = tri_sqr_lp(t, ld4(0));
    if constexpr (OP == TOP_tri_line_pair)
      y = tri_line_pair(t, [&](int c) { return ld2(0, 2 * c); }, [&](int c) { return ld2(6, 2 * c); });
    if constexpr (OP == TOP_tri_frob) y = tri_frob(t, ld4(0));
    if constexpr (OP == TOP_tri_frob2) y = tri_frob2(t, ld4(0));
    if constexpr (OP == TOP_tri_conj) y = tri_conj(t, ld4(0));
    if (live) {
      uint32_t* qa = out + (i * 12 + tri_slot_a(t.role)) * 12;
      uint32_t* qb = out + (i * 12 + tri_slot_b(t.role)) * 12;
#pragma unroll
      for (int w = 0; w < 12; w++) {
        qa[w] = y.a.c0.l[w], qa[12 + w] = y.a.c1.l[w];
        qb[w] = y.b.c0.l[w], qb[12 + w] = y.b.c1.l[w];
      }
    }
  }
}

// ------------------------------------------------------------------ launchers
// kinds 0, 1 and 3 of testops.h (kind 2 lives in k_miller.hip); false for an op that is not here
template <int OP, int NIN, int NOUT, int KIND>
static bool launch_test_op_t(const uint32_t* in, size_t cnt, uint32_t* out, uint32_t* park, hipStream_t st) {
  if constexpr (KIND == 0 || KIND == 1) {
    hipLaunchKernelGGL((k_test_op<OP, NIN, NOUT>), dim3(grid_for(cnt)), dim3(TPB), 0, st, in, cnt, out);
    return true;
  } else if constexpr (KIND == 3) {
    hipLaunchKernelGGL((k_test_tri<OP, NIN, NOUT>), dim3((unsigned)((cnt + TRI_GROUPS - 1) / TRI_GROUPS)), dim3(TPB), 0,
                       st, in, cnt, out, park);
    return true;
  } else {
    return false;
  }
}
bool launch_test_op(int op, const uint32_t* in, size_t cnt, uint32_t* out, uint32_t* park, hipStream_t st) {
  if (!cnt) return true;
  switch (op) {
#define X(name, nin, nout, kind) \
  case TOP_##name:               \
    return launch_test_op_t<TOP_##name, nin, nout, kind>(in, cnt, out, park, st);
    BLS_TEST_OPS(X)
#undef X
  }
  return false;
}

void launch_test_pack_fp12(const uint32_t* f, size_t cnt, uint32_t* F, hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_test_pack_fp12, dim3(grid_for(cnt)), dim3(TPB), 0, st, f, cnt, F);
}

void launch_test_unpack_fp12(const uint32_t* F, size_t cnt, uint32_t* out, hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_test_unpack_fp12, dim3(grid_for(cnt)), dim3(TPB), 0, st, F, cnt, out);
}

void launch_test_final_exp_ref(const uint32_t* F, size_t cnt, uint32_t* out, hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_test_final_exp_ref, dim3(grid_for(cnt)), dim3(TPB), 0, st, F, cnt, out);
}

void launch_test_fp_mul(const uint32_t* a, const uint32_t* b, size_t cnt, uint32_t* out, hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_test_fp_mul, dim3(grid_for(cnt)), dim3(TPB), 0, st, a, b, cnt, out);
}

void launch_test_pairing(const uint32_t* p_tab, const uint32_t* q_aff, size_t cnt, uint32_t* out_f, hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_test_pairing, dim3(grid_for(cnt)), dim3(TPB), 0, st, p_tab, q_aff, cnt, out_f);
}

void launch_test_unpack_g2(const uint32_t* H, size_t cnt, uint32_t* out, hipStream_t st) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_test_unpack_g2, dim3(grid_for(cnt)), dim3(TPB), 0, st, H, cnt, out);
}

}  // namespace blsk
