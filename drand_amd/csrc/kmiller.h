// What the Miller-stage translation units share (k_miller.hip: the two-pair passes of the verification
// pipeline; k_tsealr.hip: the single-pair passes of the sealing to many rounds): the cache policy of the
// line staging, the LDS home of the lines pass's running point T, and the k p table of the f passes.
#pragma once
#include "kcommon.h"

namespace blsk {

// cache policy of the line staging's stores and loads (soa.h AUX; 0 = default)
// Cache policy of the line staging: written once by k_miller_lines, read once by k_miller_f, 13.8 KB
// per beacon -- nothing to keep in L2/MALL. Non-temporal (gfx950 aux 2) on both sides: Miller
// 196.2 -> 192.7 ms per 1M on one box, interleaved twice (profiles/r06s_ln_nt_ab.json); the loads
// carry the gain, the stores alone change nothing.
#ifndef BLS_LN_AUX
#define BLS_LN_AUX 2
#endif
#ifndef BLS_LN_AUX_ST
#define BLS_LN_AUX_ST BLS_LN_AUX
#endif
#ifndef BLS_LN_AUX_LD
#define BLS_LN_AUX_LD BLS_LN_AUX
#endif

static __shared__ uint32_t g_ml_T[72 * BLS_LANES];
// T = (X, Y, Z) in LDS, word w of coordinate c at [(24 c + w) * 64 + lane]: conflict-free dword access
struct g2proj_lds {
  uint32_t* base;
  DI fp2 get(int c) const {
    fp2 v;
#pragma unroll
    for (int w = 0; w < 12; w++) {
      v.c0.l[w] = base[(24 * c + w) * BLS_LANES];
      v.c1.l[w] = base[(24 * c + 12 + w) * BLS_LANES];
    }
    return v;
  }
  DI void set(int c, const fp2& v) const {
#pragma unroll
    for (int w = 0; w < 12; w++) {
      base[(24 * c + w) * BLS_LANES] = v.c0.l[w];
      base[(24 * c + 12 + w) * BLS_LANES] = v.c1.l[w];
    }
  }
};

// q p of the one-reduction linear forms (tower.h fp2_lin_reduce, T < 16p) from an LDS table of k p,
// k < 16 (768 bytes per workgroup, tower.h kp_lds_init / KpLdsK)
using KpLds16 = KpLdsK<16>;

}  // namespace blsk
