// Combination stage of the randomized batch verification (rlc.h): per group of G consecutive items
// of a pass, A = sum r_i H_i and B = sum r_i sigma_i over the items with cls == 0, written in affine
// form with infinity flags into one H/S staging slot per group (the layout launch_miller reads), and
// the small gather / scatter kernels of the exact fallback.
// The in-place Fp2 products use the Karatsuba body, as the other G2 chains of k_decomp.hip do.
#define BLS_FP2_KARA_INL 1
#include "kcommon.h"
#include "rlc.h"

namespace blsk {

static_assert(kRlcLaneItems == (size_t)RLC_LANE_ITEMS && kRlcPartWords == 72, "kernels.h and rlc.h disagree");

struct RlcSeed {
  uint32_t w[8];
};

// Lane j of row `which` (blockIdx.y: 0 = the H sum, 1 = the sigma sum, wave-uniform so that the SoA
// buffer resources are) accumulates items [8 j, 8 j + 8) of the pass; its Jacobian partial sum goes
// to part[which] (three Fp2 = six slots, SoA of stride nl). A group is G / 8 consecutive lanes.
// The scalars sit in LDS (each lane reads only what it wrote): the item loop is not unrolled, and a
// register array indexed by its counter would live in scratch.
// One wave per SIMD: the accumulator, a step's temporaries and the in-place Fp2 bodies take the 512
// registers without scratch (96.1 ms per 1M beacons); built for two waves the kernel keeps 256, spills
// 1,184 bytes per lane and takes 108.3 ms (same-box A/B, profiles/rlc_bench.json "wpe2_ab").
BLS_KERNEL(1) k_rlc_acc(const uint32_t* H, const uint8_t* h_inf, const uint32_t* S, const uint8_t* s_inf,
                        const uint8_t* cls, size_t cnt, uint64_t index0, RlcSeed seed, uint32_t* part, size_t nl) {
  __shared__ uint64_t sc[RLC_LANE_ITEMS * TPB];
  const size_t j = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (j >= nl) return;
  const int which = blockIdx.y;
  const uint32_t* P = which ? S : H;
  const uint8_t* inf = which ? s_inf : h_inf;
  const size_t i0 = j * RLC_LANE_ITEMS;
  const int nk = (int)(cnt - i0 < (size_t)RLC_LANE_ITEMS ? cnt - i0 : (size_t)RLC_LANE_ITEMS);
#pragma unroll 1
  for (int k = 0; k < RLC_LANE_ITEMS; k++) {
    uint64_t r = 0;
    if (k < nk && cls[i0 + k] == REJ_OK && !inf[i0 + k]) r = rlc_scalar(seed.w, index0 + i0 + k);
    sc[k * TPB + threadIdx.x] = r;
  }
  const g2j acc = rlc_accumulate(
      nk, [&](int k) { return ld_fp2(P, cnt, i0 + k, 0); }, [&](int k) { return ld_fp2(P, cnt, i0 + k, 2); },
      [&](int k, int b) { return ((sc[k * TPB + threadIdx.x] >> b) & 1u) != 0; });
  uint32_t* out = part + (size_t)which * 72 * nl;
  st_fp2(out, nl, j, 0, acc.x);
  st_fp2(out, nl, j, 2, acc.y);
  st_fp2(out, nl, j, 4, acc.z);
}

// One lane per group and row: the sum of the group's lpg = G / 8 lanes (the last group of a pass may
// have fewer), to affine, into slot g of the group staging (stride ng).
__global__ void __launch_bounds__(TPB) k_rlc_reduce(const uint32_t* part, size_t nl, size_t lpg, size_t ng,
                                                   uint32_t* GH, uint8_t* g_hinf, uint32_t* GS, uint8_t* g_sinf) {
  const size_t g = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (g >= ng) return;
  const int which = blockIdx.y;
  const uint32_t* P = part + (size_t)which * 72 * nl;
  const size_t j0 = g * lpg;
  const size_t m = nl - j0 < lpg ? nl - j0 : lpg;
  const g2j acc = rlc_sum(m, [&](size_t q) {
    return g2j{ld_fp2(P, nl, j0 + q, 0), ld_fp2(P, nl, j0 + q, 2), ld_fp2(P, nl, j0 + q, 4)};
  });
  const bool inf = jac_is_inf(acc);
  g2a a = {fp2_zero(), fp2_zero()};
  if (!inf) a = g2_to_aff(acc);
  uint32_t* out = which ? GS : GH;
  st_fp2(out, ng, g, 0, a.x);
  st_fp2(out, ng, g, 2, a.y);
  (which ? g_sinf : g_hinf)[g] = inf;
}

// Exact fallback: compact slot t holds item fail[t >> lg] * G + (t & (G - 1)) of the pass (fail: the
// failing groups in ascending order; only the last group of a pass can be short, and the host sizes m
// for it, so every slot names an item below cnt). Row 0 copies H, row 1 S and the class byte.
__global__ void __launch_bounds__(TPB) k_rlc_gather(const uint32_t* fail, int lg, size_t m, const uint32_t* H,
                                                   const uint8_t* h_inf, const uint32_t* S, const uint8_t* s_inf,
                                                   const uint8_t* cls, size_t cnt, uint32_t* CH, uint8_t* c_hinf,
                                                   uint32_t* CS, uint8_t* c_sinf, uint8_t* ccls) {
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= m) return;
  const size_t src = ((size_t)fail[t >> lg] << lg) + (t & (((size_t)1 << lg) - 1));
  if (src >= cnt) return;  // never (see above); keeps every access in bounds regardless
  const int which = blockIdx.y;
  const uint32_t* from = which ? S : H;
  uint32_t* to = which ? CS : CH;
#pragma unroll 1
  for (int slot = 0; slot < 4; slot++) st_fp(to, m, t, slot, ld_fp(from, cnt, src, slot));
  if (which) {
    c_sinf[t] = s_inf[src];
    ccls[t] = cls[src];
  } else {
    c_hinf[t] = h_inf[src];
  }
}

__global__ void __launch_bounds__(256) k_rlc_scatter(const uint32_t* fail, int lg, size_t m, const uint8_t* ccls,
                                                    uint8_t* cls, size_t cnt) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m) return;
  const size_t src = ((size_t)fail[t >> lg] << lg) + (t & (((size_t)1 << lg) - 1));
  if (src < cnt) cls[src] = ccls[t];
}

// test hook: the group staging's points in the ZCash compressed form
__global__ void __launch_bounds__(TPB) k_rlc_compress(const uint32_t* GP, const uint8_t* g_inf, size_t ng,
                                                     uint8_t* out96) {
  const size_t g = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (g >= ng) return;
  g2j p = jac_infinity<fp2>();
  if (!g_inf[g]) p = {ld_fp2(GP, ng, g, 0), ld_fp2(GP, ng, g, 2), fp2_one()};
  uint8_t buf[96];
  g2_compress(buf, p);
  for (int k = 0; k < 96; k++) out96[g * 96 + k] = buf[k];
}

// ------------------------------------------------------------------ launchers
void launch_rlc_sums(const uint32_t* H, const uint8_t* h_inf, const uint32_t* S, const uint8_t* s_inf,
                     const uint8_t* cls, size_t cnt, uint64_t index0, const uint32_t* seed_words, size_t group,
                     uint32_t* part, uint32_t* GH, uint8_t* g_hinf, uint32_t* GS, uint8_t* g_sinf, hipStream_t st) {
  if (!cnt) return;
  RlcSeed seed;
  for (int k = 0; k < 8; k++) seed.w[k] = seed_words[k];
  const size_t nl = rlc_lanes(cnt), ng = rlc_groups(cnt, group);
  hipLaunchKernelGGL(k_rlc_acc, dim3(grid_for(nl), 2), dim3(TPB), 0, st, H, h_inf, S, s_inf, cls, cnt, index0, seed,
                       part, nl);
  hipLaunchKernelGGL(k_rlc_reduce, dim3(grid_for(ng), 2), dim3(TPB), 0, st, part, nl, group / RLC_LANE_ITEMS, ng, GH,
                     g_hinf, GS, g_sinf);
}

static int log2_of(size_t group) {
  int lg = 0;
  while (((size_t)1 << lg) < group) lg++;
  return lg;
}

void launch_rlc_gather(const uint32_t* fail, size_t group, size_t m, const uint32_t* H, const uint8_t* h_inf,
                       const uint32_t* S, const uint8_t* s_inf, const uint8_t* cls, size_t cnt, uint32_t* CH,
                       uint8_t* c_hinf, uint32_t* CS, uint8_t* c_sinf, uint8_t* ccls, hipStream_t st) {
  if (!m) return;
  hipLaunchKernelGGL(k_rlc_gather, dim3(grid_for(m), 2), dim3(TPB), 0, st, fail, log2_of(group), m, H, h_inf, S,
                     s_inf, cls, cnt, CH, c_hinf, CS, c_sinf, ccls);
}

void launch_rlc_scatter(const uint32_t* fail, size_t group, size_t m, const uint8_t* ccls, uint8_t* cls, size_t cnt,
                        hipStream_t st) {
  if (!m) return;
  hipLaunchKernelGGL(k_rlc_scatter, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, fail, log2_of(group), m,
                     ccls, cls, cnt);
}

void launch_rlc_compress(const uint32_t* GP, const uint8_t* g_inf, size_t ng, uint8_t* out96, hipStream_t st) {
  if (!ng) return;
  hipLaunchKernelGGL(k_rlc_compress, dim3(grid_for(ng)), dim3(TPB), 0, st, GP, g_inf, ng, out96);
}

}  // namespace blsk
