// libanystereo_scenes.so: procedural stereo scenes on the device (include/anystereo_scenes.h states the model).
//
// A scene is a function of (spec, seed, index): up to 8 planar layers drawn from integer hashes.  Nothing is uploaded: the spec, the
// seed and the indices are kernel arguments, and the first n_layers threads of every block derive the layers (and the noise-lattice
// keys of their octaves) into LDS — ~40 hashes and a few dozen flops per block, against 256 pixels of ~100 hashes each.  One thread
// is one pixel or one query; no block depends on another; every store is a plain dword (byte for noc) store at consecutive
// addresses across the wave.
//
//   render_kernel   both views of scene index0 + blockIdx.y at (h, w): six values per thread
//   gt_kernel       ragged: blockIdx.y picks one of <= 8 samples carried by value; left / right disparity and noc, any of them optional
//   at_kernel       disparity (and noc) at arbitrary (row, col) queries of <= 8 scenes, times a per-sample width
//
// Arithmetic.  Every value is an fp32 add, multiply, divide, floor or compare rounded on its own, in the order written here: no FMA
// contraction in this file, no transcendental.  anystereo/harness/scenes.py restates each function below with torch ops and must
// equal it bit for bit, so an edit here is an edit there.  derive_layer is compiled for the host as well (scn_layers): the Python
// copy of the derivation is checked against it without a GPU.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/anystereo_scenes.h"
#include "../host/errstate.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr float kInv24 = 5.9604644775390625e-08f;  // 2^-24
// hash slots of a layer: slot = layer * 64 + j
constexpr int kSlotKind = 0, kSlotCu = 1, kSlotCv = 2, kSlotA = 3, kSlotB = 4, kSlotK = 5, kSlotAlpha = 6, kSlotBeta = 7, kSlotGamma = 8,
              kSlotColour = 9, kSlotOctave = 32;
constexpr int kSlotNoise = SCN_MAX_LAYERS * 64;  // the per-value noise of image2

struct Layer {
  int kind;
  float cu, cv, inv_a, k, inv_b;  // support: du = u - cu, dv = (v - cv) * aspect, p = (du + k dv) * inv_a, q = dv * inv_b
  float alpha, beta, gamma, omb;  // plane d = alpha + beta (u - cu) + gamma (v - cv); omb = 1 - beta
  float col[3];
  float a, b;
};

struct Scene {
  Layer layer[SCN_MAX_LAYERS];
  uint32_t okey[SCN_MAX_LAYERS][SCN_MAX_OCTAVES];  // lattice key of (layer, octave)
  uint32_t nkey;                                   // key of image2's noise
};

// make_coord of one axis: value(i) = c0 + step * i with c0 = fl(-1 + 1/n), step = fl(2/n), both formed in double and rounded once
// (stated in ../query.h, coord_axis: the same floats; restated because this library's source hash covers csrc/scenes/ alone)
struct Axis {
  float c0, step;
};
inline Axis axis(int n) { return Axis{(float)(-1.0 + 1.0 / (double)n), (float)(2.0 / (double)n)}; }

struct GtSample {
  float* disp;
  float* disp_right;
  unsigned char* noc;
  int h, w, index;
  Axis ah, aw;
};
struct GtTable {
  GtSample s[SCN_MAX_BATCH];
};
struct AtTable {
  float mul[SCN_MAX_BATCH];
  int index[SCN_MAX_BATCH];
};

// ---- hashes ----
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x21f0aaadu;
  x ^= x >> 15;
  x *= 0x735a2d97u;
  x ^= x >> 15;
  return x;
}

// the key of scene (seed, index)
__host__ __device__ __forceinline__ uint32_t scene_key(uint64_t seed, int index) {
  uint32_t t = mix32((uint32_t)seed + 0x9e3779b9u);
  t = mix32(t ^ (uint32_t)(seed >> 32));
  return mix32(t ^ ((uint32_t)index * 0x85ebca6bu));
}

__host__ __device__ __forceinline__ uint32_t slot_hash(uint32_t base, int slot) { return mix32(base ^ mix32((uint32_t)slot + 0x9e3779b9u)); }
__host__ __device__ __forceinline__ float uniform(uint32_t h) { return (float)(h >> 8) * kInv24; }  // [0, 1), 24 bits: exact

// ---- the layers of a scene ----
__host__ __device__ inline void derive_layer(const scn_spec& sp, uint32_t base, int l, Layer& L) {
  const int s0 = l * 64;
  const float u_alpha = uniform(slot_hash(base, s0 + kSlotAlpha));
  const float u_beta = uniform(slot_hash(base, s0 + kSlotBeta));
  const float u_gamma = uniform(slot_hash(base, s0 + kSlotGamma));
  if (l == 0) {
    L.kind = SCN_KIND_PLANE;
    L.cu = 0.5f;
    L.cv = 0.5f;
    L.a = 1.f;
    L.b = 1.f;
    L.k = 0.f;
    L.alpha = sp.bg_min + (sp.bg_max - sp.bg_min) * u_alpha;
    L.beta = (u_beta * 2.f - 1.f) * sp.bg_slope;
    L.gamma = (u_gamma * 2.f - 1.f) * sp.bg_slope;
  } else {
    L.kind = SCN_KIND_ELLIPSE + (int)(slot_hash(base, s0 + kSlotKind) & 1u);
    L.cu = 0.1f + 0.8f * uniform(slot_hash(base, s0 + kSlotCu));
    L.cv = 0.1f + 0.8f * uniform(slot_hash(base, s0 + kSlotCv));
    L.a = sp.size_min + (sp.size_max - sp.size_min) * uniform(slot_hash(base, s0 + kSlotA));
    L.b = sp.size_min + (sp.size_max - sp.size_min) * uniform(slot_hash(base, s0 + kSlotB));
    L.k = (uniform(slot_hash(base, s0 + kSlotK)) * 2.f - 1.f) * sp.shear_max;
    L.alpha = sp.d_min + (sp.d_max - sp.d_min) * u_alpha;
    L.beta = (u_beta * 2.f - 1.f) * sp.slope_max;
    L.gamma = (u_gamma * 2.f - 1.f) * sp.slope_max;
  }
  L.inv_a = 1.f / L.a;
  L.inv_b = 1.f / L.b;
  L.omb = 1.f - L.beta;
  for (int c = 0; c < 3; ++c) L.col[c] = 40.f + 170.f * uniform(slot_hash(base, s0 + kSlotColour + c));
}

// the block's first threads derive the scene into LDS; every thread of the block must call this
__device__ __forceinline__ void load_scene(Scene& sc, const scn_spec& sp, uint64_t seed, int index) {
  const int t = threadIdx.x;
  if (t <= sp.n_layers) {
    const uint32_t base = scene_key(seed, index);
    if (t < sp.n_layers) {
      derive_layer(sp, base, t, sc.layer[t]);
      for (int o = 0; o < sp.octaves; ++o) sc.okey[t][o] = slot_hash(base, t * 64 + kSlotOctave + o);
    } else {
      sc.nkey = slot_hash(base, kSlotNoise);
    }
  }
  __syncthreads();
}

// ---- geometry ----
__device__ __forceinline__ float plane(const Layer& L, float u, float v) { return (L.alpha + L.beta * (u - L.cu)) + L.gamma * (v - L.cv); }

__device__ __forceinline__ bool inside(const Layer& L, float aspect, float u, float v) {
  if (L.kind == SCN_KIND_PLANE) return true;
  const float du = u - L.cu, dv = (v - L.cv) * aspect;
  const float p = (du + L.k * dv) * L.inv_a, q = dv * L.inv_b;
  if (L.kind == SCN_KIND_ELLIPSE) return p * p + q * q <= 1.f;
  return fabsf(p) <= 1.f && fabsf(q) <= 1.f;
}

// the layer seen by the left view at (u, v) and its disparity (a fraction of the width)
__device__ __forceinline__ int seen_left(const Scene& sc, const scn_spec& sp, float u, float v, float& d_out) {
  int best = 0;
  float bd = plane(sc.layer[0], u, v);
  for (int l = 1; l < sp.n_layers; ++l) {
    const Layer& L = sc.layer[l];
    const float d = plane(L, u, v);
    if (inside(L, sp.aspect, u, v) && d > bd) {
      bd = d;
      best = l;
    }
  }
  d_out = bd;
  return best;
}

// the left-view column at which layer L is seen by the right view's pixel (ur, v): the plane inverted in closed form
__device__ __forceinline__ float left_column(const Layer& L, float ur, float v) {
  return (((ur + L.alpha) - L.beta * L.cu) + L.gamma * (v - L.cv)) / L.omb;
}

// the layer seen by the right view at (ur, v), its disparity and the left-view column of the surface point
__device__ __forceinline__ int seen_right(const Scene& sc, const scn_spec& sp, float ur, float v, float& d_out, float& ul_out) {
  int best = 0;
  float bu = left_column(sc.layer[0], ur, v);
  float bd = plane(sc.layer[0], bu, v);
  for (int l = 1; l < sp.n_layers; ++l) {
    const Layer& L = sc.layer[l];
    const float ul = left_column(L, ur, v);
    const float d = plane(L, ul, v);
    if (inside(L, sp.aspect, ul, v) && d > bd) {
      bd = d;
      bu = ul;
      best = l;
    }
  }
  d_out = bd;
  ul_out = bu;
  return best;
}

__device__ __forceinline__ unsigned char noc_of(const Scene& sc, const scn_spec& sp, float u, float v, int l, float d) {
  const float ur = u - d;
  float dr, ul;
  const int lr = seen_right(sc, sp, ur, v, dr, ul);
  return (lr == l && ur >= 0.f) ? 1 : 0;
}

// ---- texture: octaves of bilinear value noise in the layer's own frame, at the surface point (u, v) of the LEFT view ----
__device__ __forceinline__ float lattice(uint32_t key, int ix, int iy) {
  uint32_t h = mix32(key ^ ((uint32_t)ix * 0x27d4eb2fu));
  h = mix32(h ^ ((uint32_t)iy * 0x165667b1u));
  return uniform(h);
}

__device__ __forceinline__ float texture(const Scene& sc, const scn_spec& sp, int l, float u, float v) {
  const Layer& L = sc.layer[l];
  const float s = u - L.cu, t = (v - L.cv) * sp.aspect;
  float acc = 0.f, f = sp.lattice, amp = sp.contrast;
  for (int o = 0; o < sp.octaves; ++o) {
    const uint32_t key = sc.okey[l][o];
    const float xs = s * f, ys = t * f;
    const float x0 = floorf(xs), y0 = floorf(ys);
    const float fx = xs - x0, fy = ys - y0;
    const int ix = (int)x0, iy = (int)y0;
    const float a = lattice(key, ix, iy), b = lattice(key, ix + 1, iy);
    const float c = lattice(key, ix, iy + 1), d = lattice(key, ix + 1, iy + 1);
    const float top = a + fx * (b - a), bot = c + fx * (d - c);
    const float n = top + fy * (bot - top);
    acc = acc + amp * (n - 0.5f);
    f = f * 2.f;
    amp = amp * 0.5f;
  }
  return acc;
}

__device__ __forceinline__ float clamp_grey(float x) { return fminf(fmaxf(x, 0.f), 254.999f); }

// ---- kernels ----
__global__ __launch_bounds__(kThreads) void render_kernel(scn_spec sp, uint64_t seed, int index0, float* __restrict__ img1,
                                                          float* __restrict__ img2, int h, int w, Axis ah, Axis aw) {
  __shared__ Scene sc;
  const int b = blockIdx.y;
  load_scene(sc, sp, seed, index0 + b);
  const int n = h * w;
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  if (pix >= n) return;
  const int y = pix / w, x = pix - y * w;
  const float u = ((aw.c0 + aw.step * (float)x) + 1.f) * 0.5f;
  const float v = ((ah.c0 + ah.step * (float)y) + 1.f) * 0.5f;
  float d, dr, ul;
  const int l = seen_left(sc, sp, u, v, d);
  const float t1 = texture(sc, sp, l, u, v);
  const int lr = seen_right(sc, sp, u, v, dr, ul);
  const float t2 = texture(sc, sp, lr, ul, v);
  const int64_t o = (int64_t)b * 3 * n + pix;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    img1[o + (int64_t)c * n] = clamp_grey(sc.layer[l].col[c] + t1);
    const float un = uniform(mix32(sc.nkey ^ (uint32_t)(pix * 3 + c)));
    img2[o + (int64_t)c * n] = clamp_grey((sc.layer[lr].col[c] + t2) + (un * 2.f - 1.f) * sp.noise);
  }
}

__global__ __launch_bounds__(kThreads) void gt_kernel(GtTable tab, scn_spec sp, uint64_t seed) {
  __shared__ Scene sc;
  const GtSample& s = tab.s[blockIdx.y];
  const int n = s.h * s.w;
  if ((int64_t)blockIdx.x * kThreads >= n) return;  // the whole block: the grid is sized for the largest sample of the launch
  load_scene(sc, sp, seed, s.index);
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  if (pix >= n) return;
  const int y = pix / s.w, x = pix - y * s.w;
  const float u = ((s.aw.c0 + s.aw.step * (float)x) + 1.f) * 0.5f;
  const float v = ((s.ah.c0 + s.ah.step * (float)y) + 1.f) * 0.5f;
  const float wf = (float)s.w;
  if (s.disp != nullptr || s.noc != nullptr) {
    float d;
    const int l = seen_left(sc, sp, u, v, d);
    if (s.disp != nullptr) s.disp[pix] = d * wf;
    if (s.noc != nullptr) s.noc[pix] = noc_of(sc, sp, u, v, l, d);
  }
  if (s.disp_right != nullptr) {
    float dr, ul;
    seen_right(sc, sp, u, v, dr, ul);
    s.disp_right[pix] = dr * wf;
  }
}

__global__ __launch_bounds__(kThreads) void at_kernel(AtTable tab, scn_spec sp, uint64_t seed, const float2* __restrict__ coord,
                                                      float* __restrict__ out, unsigned char* __restrict__ noc, int Q, int right_view) {
  __shared__ Scene sc;
  const int b = blockIdx.y;
  load_scene(sc, sp, seed, tab.index[b]);
  const int q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= Q) return;
  const int64_t i = (int64_t)b * Q + q;
  const float2 rc = coord[i];  // (row, col)
  const float u = (rc.y + 1.f) * 0.5f;
  const float v = (rc.x + 1.f) * 0.5f;
  float d, ul;
  if (right_view) {
    seen_right(sc, sp, u, v, d, ul);
  } else {
    const int l = seen_left(sc, sp, u, v, d);
    if (noc != nullptr) noc[i] = noc_of(sc, sp, u, v, l, d);
  }
  out[i] = d * tab.mul[b];
}

// ---- host side ----
int check_spec(const char* what, const scn_spec* sp) {
  REQUIRE(sp != nullptr, SCN_ERR_BAD_ARG, "%s: null spec", what);
  REQUIRE(sp->n_layers >= 1 && sp->n_layers <= SCN_MAX_LAYERS, SCN_ERR_BAD_ARG, "%s: n_layers=%d outside [1, %d]", what, sp->n_layers,
          SCN_MAX_LAYERS);
  REQUIRE(sp->octaves >= 1 && sp->octaves <= SCN_MAX_OCTAVES, SCN_ERR_BAD_ARG, "%s: octaves=%d outside [1, %d]", what, sp->octaves,
          SCN_MAX_OCTAVES);
  REQUIRE(sp->aspect > 0.f && sp->size_min > 0.f && sp->size_max >= sp->size_min && sp->lattice > 0.f, SCN_ERR_BAD_ARG,
          "%s: aspect=%g, size_min=%g, size_max=%g, lattice=%g: positive values and size_min <= size_max expected", what,
          (double)sp->aspect, (double)sp->size_min, (double)sp->size_max, (double)sp->lattice);
  REQUIRE(fabsf(sp->slope_max) < 1.f && fabsf(sp->bg_slope) < 1.f, SCN_ERR_BAD_ARG,
          "%s: slope_max=%g, bg_slope=%g: a plane with |beta| >= 1 has no right view", what, (double)sp->slope_max, (double)sp->bg_slope);
  return SCN_OK;
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

}  // namespace

extern "C" {

int scn_abi_version(void) { return 1; }

const char* scn_last_error_string(void) { return err_buf(); }

int scn_layers(const scn_spec* spec, uint64_t seed, int index, float* out) {
  if (int rc = check_spec("scn_layers", spec)) return rc;
  REQUIRE(out != nullptr, SCN_ERR_BAD_ARG, "scn_layers: null output");
  const uint32_t base = scene_key(seed, index);
  for (int l = 0; l < spec->n_layers; ++l) {
    Layer L;
    derive_layer(*spec, base, l, L);
    float* o = out + l * SCN_LAYER_FLOATS;
    const float row[SCN_LAYER_FLOATS] = {(float)L.kind, L.cu, L.cv, L.inv_a, L.k, L.inv_b, L.alpha, L.beta, L.gamma,
                                         L.col[0], L.col[1], L.col[2], L.a, L.b, L.omb, 0.f};
    for (int j = 0; j < SCN_LAYER_FLOATS; ++j) o[j] = row[j];
  }
  return SCN_OK;
}

int scn_render_pair(float* image1, float* image2, int B, int h, int w, const scn_spec* spec, uint64_t seed, int index0, void* stream) {
  if (int rc = check_spec("scn_render_pair", spec)) return rc;
  REQUIRE(image1 != nullptr && image2 != nullptr, SCN_ERR_BAD_ARG, "scn_render_pair: null image");
  REQUIRE(aligned(image1, 4) && aligned(image2, 4), SCN_ERR_BAD_ARG, "scn_render_pair: images must be 4-byte aligned");
  REQUIRE(B >= 1 && h >= 1 && w >= 1, SCN_ERR_BAD_ARG, "scn_render_pair: B=%d h=%d w=%d must be positive", B, h, w);
  REQUIRE(B <= 65535 && 3ll * B * h * w < (1ll << 31), SCN_ERR_BAD_SHAPE, "scn_render_pair: B=%d h=%d w=%d: need B <= 65535 and 3*B*h*w < 2^31",
          B, h, w);
  hipLaunchKernelGGL(render_kernel, dim3(cdiv((int64_t)h * w, kThreads), (unsigned)B), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     *spec, seed, index0, image1, image2, h, w, axis(h), axis(w));
  return check_launch("scn_render_pair", SCN_ERR_LAUNCH);
}

int scn_ground_truth(const scn_gt_sample* table, int n, const scn_spec* spec, uint64_t seed, void* stream) {
  if (int rc = check_spec("scn_ground_truth", spec)) return rc;
  REQUIRE(table != nullptr, SCN_ERR_BAD_ARG, "scn_ground_truth: null table");
  REQUIRE(n >= 1, SCN_ERR_BAD_ARG, "scn_ground_truth: n=%d samples", n);
  for (int i = 0; i < n; ++i) {  // all samples before the first launch
    const scn_gt_sample& s = table[i];
    REQUIRE(s.h >= 1 && s.w >= 1, SCN_ERR_BAD_ARG, "scn_ground_truth: sample %d: h=%d w=%d must be positive", i, s.h, s.w);
    REQUIRE((int64_t)s.h * s.w < (1ll << 31), SCN_ERR_BAD_SHAPE, "scn_ground_truth: sample %d: h*w = %lld >= 2^31", i,
            (long long)s.h * s.w);
    REQUIRE(s.disp != nullptr || s.disp_right != nullptr || s.noc != nullptr, SCN_ERR_BAD_ARG, "scn_ground_truth: sample %d: no output", i);
    REQUIRE(aligned(s.disp, 4) && aligned(s.disp_right, 4), SCN_ERR_BAD_ARG, "scn_ground_truth: sample %d: outputs must be 4-byte aligned", i);
  }
  for (int i0 = 0; i0 < n; i0 += SCN_MAX_BATCH) {
    const int nb = n - i0 < SCN_MAX_BATCH ? n - i0 : SCN_MAX_BATCH;
    GtTable t;
    int64_t most = 0;
    for (int i = 0; i < SCN_MAX_BATCH; ++i) {
      const scn_gt_sample& s = table[i0 + (i < nb ? i : 0)];  // unused slots repeat the first sample; no block reads them
      t.s[i] = GtSample{s.disp, s.disp_right, s.noc, s.h, s.w, s.index, axis(s.h), axis(s.w)};
      if (i < nb && (int64_t)s.h * s.w > most) most = (int64_t)s.h * s.w;
    }
    hipLaunchKernelGGL(gt_kernel, dim3(cdiv(most, kThreads), (unsigned)nb), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), t, *spec,
                       seed);
    if (int rc = check_launch("scn_ground_truth", SCN_ERR_LAUNCH)) return rc;
  }
  return SCN_OK;
}

int scn_disparity_at(const float* coord, float* out, unsigned char* noc, int B, int Q, const float* mul, const int* index, int right_view,
                     const scn_spec* spec, uint64_t seed, void* stream) {
  if (int rc = check_spec("scn_disparity_at", spec)) return rc;
  REQUIRE(coord != nullptr && out != nullptr && mul != nullptr && index != nullptr, SCN_ERR_BAD_ARG, "scn_disparity_at: null pointer");
  REQUIRE(aligned(coord, 8) && aligned(out, 4), SCN_ERR_BAD_ARG, "scn_disparity_at: coord must be 8-byte and out 4-byte aligned");
  REQUIRE(B >= 1 && Q >= 1, SCN_ERR_BAD_ARG, "scn_disparity_at: B=%d Q=%d must be positive", B, Q);
  REQUIRE(2ll * B * Q < (1ll << 31), SCN_ERR_BAD_SHAPE, "scn_disparity_at: B=%d Q=%d: need 2*B*Q < 2^31", B, Q);
  REQUIRE(!(right_view && noc != nullptr), SCN_ERR_BAD_ARG, "scn_disparity_at: noc is defined for the left view only");
  for (int b0 = 0; b0 < B; b0 += SCN_MAX_BATCH) {
    const int nb = B - b0 < SCN_MAX_BATCH ? B - b0 : SCN_MAX_BATCH;
    AtTable t;
    for (int i = 0; i < SCN_MAX_BATCH; ++i) {
      t.mul[i] = mul[b0 + (i < nb ? i : 0)];
      t.index[i] = index[b0 + (i < nb ? i : 0)];
    }
    const int64_t off = (int64_t)b0 * Q;
    hipLaunchKernelGGL(at_kernel, dim3(cdiv(Q, kThreads), (unsigned)nb), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), t, *spec, seed,
                       reinterpret_cast<const float2*>(coord) + off, out + off, noc == nullptr ? nullptr : noc + off, Q, right_view ? 1 : 0);
    if (int rc = check_launch("scn_disparity_at", SCN_ERR_LAUNCH)) return rc;
  }
  return SCN_OK;
}

}  // extern "C"
