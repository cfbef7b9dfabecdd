// The query-cell arithmetic of the continuous upsampler (liif.hip, liif_variants.hip, liif_fused.hip, backward.hip), written
// once: clamp the coordinate, take grid_sample(nearest)'s index, form the cell's centre from make_coord's two constants and the
// coordinate relative to it.  The kernels agree on the cell bit for bit because they compile THESE expressions: a new kernel
// includes this header, it does not re-type them.  Scalars in and out, by value (split.h says why).  DESIGN.md "Numerics" lists
// what stays at the sites (3x3 walk, softmax, run-head mask: as helpers they change the kernels' machine code).
// Not here: eval_metrics.hip's sample_coord (bilinear sampling with border padding, a different function); csrc/scenes/, which
// restates coord_axis (that library's source hash covers its own folder only).
#pragma once
#include "common.h"
namespace as {
// ---- host: what the entry points put into the kernels' arguments ----
// clamp bounds of a query coordinate (submodule.py:366): the Python doubles -1 + 1e-6 and 1 - 1e-6, each rounded once to fp32
constexpr float kCoordLo = (float)(-1.0 + 1e-6), kCoordHi = (float)(1.0 - 1e-6);
// make_coord (liif.py:32-45) of an axis of n cells: r = 1 / n, centre(i) = -1 + r + (2 r) * i, formed in double and rounded to
// fp32 at the end: c0 + s * i.  r was also spelled 2.0 / (2.0 * n), and s 2.0 / n: the same DOUBLES for every n, because 2.0 * n
// and doubling are exact, so 2.0 / (2.0 * n) is the correctly rounded 1 / n and 2.0 * (1.0 / n) the correctly rounded 2 / n.
struct CoordAxis { float c0, s; };
inline CoordAxis coord_axis(int n) { return CoordAxis{(float)(-1.0 + 1.0 / n), (float)(2.0 * (1.0 / n))}; }
// the bounds and both sources' axes of a parameter struct with fields lo, hi, H[2], W[2], c0y[2], sy[2], c0x[2], sx[2]
template <typename P> inline void set_query_cells(P& p) {
  p.lo = kCoordLo; p.hi = kCoordHi;
  for (int s = 0; s < 2; ++s) {
    const CoordAxis ay = coord_axis(p.H[s]), ax = coord_axis(p.W[s]);
    p.c0y[s] = ay.c0; p.sy[s] = ay.s; p.c0x[s] = ax.c0; p.sx[s] = ax.s;
  }
}

// ---- device ----
__device__ __forceinline__ float clamp_coord(float c, float lo, float hi) { return fminf(fmaxf(c, lo), hi); }  // NaN -> lo
// grid_sample(mode='nearest', align_corners=False) source index of a CLAMPED coordinate, in ATen's fp32 operation order:
// nearbyint(((c + 1) * n - 1) / 2), ties to even; after clamp_coord it lies in [0, n).  The compiler contracts `(c + 1) * n - 1`
// into one v_fma_f32 (HIP's __f*_rn are plain operators), here as in every copy this replaces: see DESIGN.md "Numerics".
__device__ __forceinline__ int nearest_idx(float c, int n) {
  const float u = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(c, 1.f), (float)n), 1.f), 2.f);
  return (int)rintf(u);
}
// centre of cell i, and the UNCLAMPED coordinate relative to it in cells: rel = (c - centre) * n  (liif.py:127-129); cell_rel_to
// is the last step alone (liif_gather_kernel: centre 0 outside the map; latent_kernel: mean of two centres; liif_rel_key_kernel)
__device__ __forceinline__ float cell_centre(float c0, float s, int i) { return __fadd_rn(c0, __fmul_rn(s, (float)i)); }
__device__ __forceinline__ float cell_rel_to(float c, float centre, int n) { return __fmul_rn(__fsub_rn(c, centre), (float)n); }
__device__ __forceinline__ float cell_rel(float c, float c0, float s, int i, int n) { return cell_rel_to(c, cell_centre(c0, s, i), n); }
}  // namespace as
