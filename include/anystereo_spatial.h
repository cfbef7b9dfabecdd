/*
 * anystereo_spatial.h — C ABI of libanystereo_spatial.so: the spatial augmentation of a stereo pair on the device (gfx950), the
 * third stage of the reference's augmentor (its spatial_transform: random rescale, flips, y-jitter, crop) and the final resize to
 * (h_lr, w_lr) of its *WoCrop classes.  The photometric stages are libanystereo_augment.so's; nothing is shared but csrc/cubic.h.
 *
 * Conventions
 *   - plain C: device pointers + sizes + a stream (hipStream_t as void*, NULL = the null stream); the launcher never allocates,
 *     synchronises, copies or clears: the per-sample parameters and the ragged outputs' pointers travel by value as kernel
 *     arguments, SPT_MAX_BATCH samples per launch.  There is no workspace: the final resize is fused into the image kernel.
 *   - return value: SPT_OK (0) or a negative SPT_ERR_* code; spt_last_error_string() describes the last failure on the calling
 *     thread.  Every argument is validated on the host BEFORE any launch: a refused call launches nothing.
 *   - images are dense [B, 3, h, w], planar, row-major; uint8, or fp32 holding integers 0..255 (an fp32 input is quantised once as
 *     clamp(floor(x + 0.5), 0, 255)).  disp is fp32 [B, H, W], valid uint8 [B, H, W].  The ground-truth crops are RAGGED: disp_out /
 *     valid_out are HOST arrays of B device pointers, crop b is [ch_b, cw_b].
 *
 * The geometry (anystereo/harness/spatial.py restates it with numpy; tests/golden/spatial.npz holds the reference's own results)
 *   frame     (fh, fw) = (rint(H * scale_y), rint(W * scale_x)) in double, half to even, when `rescale`; (H, W) otherwise
 *   flip      acts on the whole frame, the crop is taken after it:
 *               HF  both images mirrored, the disparity mirrored and negated
 *               H   out1 <- mirror(image2), out2 <- mirror(image1); the ground truth untouched, NOT mirrored (as the reference)
 *               V   everything upside down, the disparity's values kept
 *             the sparse form's VALIDITY is never flipped: the reference flips flow and leaves valid as it is
 *   crop      out1 and the ground truth from (y0, x0), out2 from (y0 + dy2, x0), ch x cw
 *   rescale   per axis inv = 1.0 / f in double; s = (float)((d + 0.5) * inv - 0.5), i = floor(s), t = s - i in fp32; i < 0 -> i = 0,
 *             t = 0; i >= n - 1 -> i = n - 1, t = 0; horizontal S[i] * (1 - t) + S[i + 1] * t, then vertical likewise, every fp32
 *             operation rounded on its own; images then clamp(floor(v + 0.5), 0, 255); dense disparity (float)((double)v * scale_x)
 *   sparse    a source pixel (x, y) with valid >= 1 lands at X = rint((double)x * fx), Y = rint((double)y * fy) and is kept if
 *             0 < X < fw and 0 < Y < fh, with the value (float)((double)d * fx); of several landing on one pixel the last in raster
 *             order wins; everything else is 0 and invalid.  Computed as a gather, without atomics.
 *   resize    with out_h, out_w > 0 the (quantised) crop goes to (out_h, out_w) by csrc/cubic.h's arithmetic (A = -0.75, half-pixel
 *             centres, taps clamped into the crop, four horizontal products summed left to right, then the four vertical ones) and
 *             is quantised again.  The ground-truth crops are not resized.
 */
#ifndef ANYSTEREO_SPATIAL_H
#define ANYSTEREO_SPATIAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPT_OK 0
#define SPT_ERR_BAD_ARG (-1)    /* null or misaligned pointer, non-positive size, a parameter outside its domain */
#define SPT_ERR_BAD_SHAPE (-2)  /* 3 * B * h * w >= 2^31 for the input or the output images, or a frame of 2^31 pixels */
#define SPT_ERR_LAUNCH (-3)     /* hipGetLastError() != hipSuccess after a launch */
#define SPT_ERR_CROP (-4)       /* a crop (of image1 or, with dy2, of image2) that leaves the rescaled frame; unequal crops without out size */
#define SPT_ERR_ALIAS (-5)      /* an output overlaps an input or another output */

#define SPT_U8 0
#define SPT_F32 1

#define SPT_FLIP_NONE 0
#define SPT_FLIP_HF 1
#define SPT_FLIP_H 2
#define SPT_FLIP_V 3

#define SPT_MAX_BATCH 8     /* samples of one launch (the table is a kernel argument); a call takes any B */
#define SPT_MIN_SCALE 0.125 /* scale_x, scale_y of a rescaled sample lie in [1/8, 8] */
#define SPT_MAX_SCALE 8.0

/* One sample. */
typedef struct spt_sample {
  double scale_x, scale_y; /* read only when rescale != 0: finite, in [SPT_MIN_SCALE, SPT_MAX_SCALE] */
  int rescale;             /* 0 | 1 */
  int flip;                /* SPT_FLIP_* */
  int y0, x0;              /* crop origin in the (flipped) rescaled frame */
  int ch, cw;              /* crop size, > 0 */
  int dy2;                 /* image2's crop starts at y0 + dy2 */
  int reserved;            /* 0 */
} spt_sample;

int spt_abi_version(void);
const char* spt_last_error_string(void);
const char* spt_source_hash(void);

/* HOST: the rescaled frame of an H x W input: (rint(H * scale_y), rint(W * scale_x)), or (H, W) without rescale.  No device is
 * touched.  SPT_ERR_BAD_ARG: a NULL pointer, a non-positive size, a scale outside [1/8, 8] or not finite, an empty frame. */
int spt_frame_size(int H, int W, int rescale, double scale_x, double scale_y, int* fh, int* fw);

/* HOST: every check spt_spatial_pair makes on the parameters alone.  out_h = out_w = 0: no final resize, all crops of one size. */
int spt_validate(const spt_sample* samples, int B, int H, int W, int out_h, int out_w);

/* out1, out2 [B, 3, h_out, w_out] of out_dtype <- image1, image2 [B, 3, H, W] of in_dtype; disp_out[b] fp32 [ch_b, cw_b] <- disp; with
 * valid != NULL (the sparse form) valid_out[b] uint8 [ch_b, cw_b] as well, and disp goes through the sparse rule instead of the
 * bilinear one.  (h_out, w_out) = (out_h, out_w), or the common crop size when both are 0.  fp32 pointers must be 4-byte aligned.
 * Two launches per SPT_MAX_BATCH samples: the images, the ground truth. */
int spt_spatial_pair(const void* image1, const void* image2, int in_dtype, const float* disp, const unsigned char* valid, int B, int H, int W,
                     const spt_sample* samples, void* out1, void* out2, int out_dtype, int out_h, int out_w, float* const* disp_out,
                     unsigned char* const* valid_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
