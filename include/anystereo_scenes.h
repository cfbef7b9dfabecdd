/*
 * anystereo_scenes.h — C ABI of libanystereo_scenes.so: procedural stereo scenes made on the device (gfx950).
 *
 * A scene is a function of (spec, seed, index) and nothing else: up to 8 textured planar layers (a background plane and
 * ellipses / parallelograms in front of it) seen by a rectified pair.  It renders its left / right images at any resolution
 * and gives its exact disparity, right-view disparity and occlusion mask at any pixel grid or any query coordinate.
 * This library replaces nothing of the reference (that is libanystereo_hip.so's role, include/anystereo_hip.h); it is the
 * data source of the evaluation and training harness where there are no datasets.
 *
 * Conventions
 *   - plain C: device pointers + sizes + a stream (hipStream_t as void*, NULL = the null stream); launchers never allocate,
 *     synchronise or copy: the spec travels by value as a kernel argument, every block derives the layers itself.
 *   - return value: SCN_OK (0) or a negative SCN_ERR_* code; scn_last_error_string() describes the last failure on the calling
 *     thread.  Every argument is validated on the host BEFORE any launch: a refused call launches nothing.
 *   - outputs are caller-allocated, dense, row-major, and fully overwritten.
 *
 * Coordinates are resolution-free: u runs across the width and v down the height, both in [0, 1].  A pass at size (h, w)
 * evaluates the scene at make_coord's own values, x_j = fl(-1 + 1/n) + fl(2/n) * j per axis, u = (x + 1) * 0.5 — so a dense
 * output is bit-equal to scn_disparity_at at make_coord([h, w]).  A disparity is a fraction d of the WIDTH; what is written is
 * d * w (dense) or d * mul (queries).
 *
 * The model ("Procedural scenes"): layer l has the disparity plane d_l = alpha + beta (u - cu) + gamma (v - cv) and,
 * for l >= 1, a support tested in its own left-view coordinates du = u - cu, dv = (v - cv) * aspect, p = (du + k dv) / a,
 * q = dv / b: p^2 + q^2 <= 1 (ellipse) or |p| <= 1 and |q| <= 1 (parallelogram).  Layer 0 covers everything.  Left pixel (u, v):
 * of the layers whose support holds it, the one with the largest d is seen (strict >, ascending l).  Right pixel (ur, v): per
 * layer u_l = (ur + alpha - beta cu + gamma (v - cv)) / (1 - beta), support tested at u_l, the largest d the same way; the right
 * disparity is positive, x_left = x_right + d.  noc = the layer seen at ur = u - d in the right view is the same layer and ur >= 0.
 * Every operation is an fp32 add, multiply, divide, floor or compare rounded on its own (no contraction, no transcendental), so
 * anystereo/harness/scenes.py restates the kernels bit for bit with torch ops.
 */
#ifndef ANYSTEREO_SCENES_H
#define ANYSTEREO_SCENES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCN_OK 0
#define SCN_ERR_BAD_ARG (-1)   /* null pointer, non-positive size, n_layers / octaves out of range, misaligned pointer */
#define SCN_ERR_BAD_SHAPE (-2) /* sizes above the supported maximum (2^31 elements of an output, 65535 samples of a launch) */
#define SCN_ERR_LAUNCH (-3)    /* hipGetLastError() != hipSuccess after a launch */

#define SCN_MAX_LAYERS 8
#define SCN_MAX_OCTAVES 6
#define SCN_MAX_BATCH 8     /* samples of one scn_ground_truth / scn_disparity_at launch (the table is a kernel argument) */
#define SCN_LAYER_FLOATS 16 /* scn_layers: kind, cu, cv, inv_a, k, inv_b, alpha, beta, gamma, r, g, b, a, b_ext, 0, 0 */

#define SCN_KIND_PLANE 0
#define SCN_KIND_ELLIPSE 1
#define SCN_KIND_PARALLELOGRAM 2

/* What the layers are drawn from.  All lengths are fractions of the image WIDTH. */
typedef struct scn_spec {
  int n_layers;    /* 1..SCN_MAX_LAYERS, the background included */
  int octaves;     /* 1..SCN_MAX_OCTAVES of value noise */
  float aspect;    /* height / width of the scene: v enters a support as (v - cv) * aspect, whatever size is rendered */
  float bg_min, bg_max, bg_slope;   /* background: alpha in [bg_min, bg_max], |beta|, |gamma| <= bg_slope */
  float d_min, d_max, slope_max;    /* layers 1..: alpha in [d_min, d_max], |beta|, |gamma| <= slope_max */
  float size_min, size_max;         /* half extents a, b of a support */
  float shear_max;                  /* |k| <= shear_max */
  float lattice;                    /* cells of the first noise octave per unit of u; doubles per octave */
  float contrast;                   /* amplitude of the first octave in grey levels; halves per octave */
  float noise;                      /* image2 gets +-noise per value */
} scn_spec;

/* One sample of a ragged scn_ground_truth call.  Any of the three pointers may be NULL (that output is not written). */
typedef struct scn_gt_sample {
  float* disp;         /* [h, w] left disparity in pixels of a w-wide image */
  float* disp_right;   /* [h, w] right-view disparity, the same unit */
  unsigned char* noc;  /* [h, w] 1 = seen by both views */
  int h, w;
  int index;           /* the scene is (spec, seed, index) */
} scn_gt_sample;

int scn_abi_version(void);
const char* scn_last_error_string(void);
const char* scn_source_hash(void);

/* HOST: the derived parameters of scene (spec, seed, index), out[n_layers][SCN_LAYER_FLOATS] in host memory — the very function
 * the kernels run per block, compiled for the host.  No device is touched. */
int scn_layers(const scn_spec* spec, uint64_t seed, int index, float* out);

/* image1, image2 fp32 [B, 3, h, w] in [0, 254.999]: the left and right view of scenes index0 .. index0 + B - 1.  One thread per
 * pixel writes its six values.  3 * B * h * w < 2^31, B <= 65535. */
int scn_render_pair(float* image1, float* image2, int B, int h, int w, const scn_spec* spec, uint64_t seed, int index0, void* stream);

/* Ragged ground truth: table[n] (HOST memory, any n >= 1; launches carry SCN_MAX_BATCH samples by value, blockIdx.y picks one).
 * Values are in pixels of the sample's own width.  h * w < 2^31 per sample; at least one output pointer per sample. */
int scn_ground_truth(const scn_gt_sample* table, int n, const scn_spec* spec, uint64_t seed, void* stream);

/* out fp32 [B, 1, Q] = mul[b] * d at the queries coord fp32 [B, Q, 2] = (row, col) in [-1, 1] (hr_coord's convention; values
 * outside are evaluated, not clamped) of scene index[b]; mul, index: HOST arrays of B values.  right_view != 0: the right
 * view's disparity at a right-view coordinate (noc must be NULL).  noc uint8 [B, Q] or NULL.  2 * B * Q < 2^31. */
int scn_disparity_at(const float* coord, float* out, unsigned char* noc, int B, int Q, const float* mul, const int* index,
                     int right_view, const scn_spec* spec, uint64_t seed, void* stream);

#ifdef __cplusplus
}
#endif
#endif
