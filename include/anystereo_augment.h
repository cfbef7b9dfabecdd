/*
 * anystereo_augment.h — C ABI of libanystereo_augment.so: the photometric augmentation and the eraser of a stereo pair on the
 * device (gfx950), byte for byte what the reference's augmentor computes with PIL and numpy (its color_transform and
 * eraser_transform; spatial_transform is no part of this library).
 *
 * Conventions
 *   - plain C: device pointers + sizes + a stream (hipStream_t as void*, NULL = the null stream); the launcher never allocates,
 *     synchronises, copies or clears: the per-sample parameters travel by value as kernel arguments, the partial sums go through
 *     a caller-provided workspace that every call fully writes before it reads it (a captured graph can hold the call).
 *   - return value: AUG_OK (0) or a negative AUG_ERR_* code; aug_last_error_string() describes the last failure on the calling
 *     thread.  Every argument is validated on the host BEFORE any launch: a refused call launches nothing.
 *   - images are dense [B, 3, h, w], planar, row-major; uint8, or fp32 holding the same integers 0..255.
 *
 * The arithmetic (anystereo/harness/augment.py restates it with numpy and is held against PIL itself)
 *   blend(x, d, f)  = d + f * (x - d) in fp32, the product rounded, then the sum; truncated for 0 <= f <= 1, clipped to [0, 255]
 *                     and truncated otherwise                                           (Image.blend)
 *   grey(R, G, B)   = (19595 R + 38470 G + 7471 B + 0x8000) >> 16                       (convert("L"))
 *   brightness      = blend(x, 0, f);   saturation = blend(x, grey of the pixel, f)
 *   contrast        = blend(x, m, f), m = (2 S + n) / (2 n) in integers, S the sum of grey over the n pixels of the image — of
 *                     BOTH images of a shared sample — in the state the image has when contrast's turn comes
 *   hue             = PIL's RGB -> HSV, H = (H + shift) & 255, HSV -> RGB, with PIL's own mix of float and double steps
 *   gamma           = out = table[value], a table the host builds
 *   eraser          = up to two rectangles of image2 filled per channel with floor(sum / n) of the jittered image2
 * All sums are integers, so no result depends on an order of summation.
 */
#ifndef ANYSTEREO_AUGMENT_H
#define ANYSTEREO_AUGMENT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AUG_OK 0
#define AUG_ERR_BAD_ARG (-1)    /* null or misaligned pointer, non-positive size, a parameter outside its domain */
#define AUG_ERR_BAD_SHAPE (-2)  /* 3 * B * h * w >= 2^31 */
#define AUG_ERR_LAUNCH (-3)     /* hipGetLastError() != hipSuccess after a launch */
#define AUG_ERR_WORKSPACE (-4)  /* workspace_bytes < aug_workspace_bytes(B, h, w) */
#define AUG_ERR_ALIAS (-5)      /* an output overlaps an input, the other output, the table or the workspace */

#define AUG_U8 0
#define AUG_F32 1

#define AUG_BRIGHTNESS 0
#define AUG_CONTRAST 1
#define AUG_SATURATION 2
#define AUG_HUE 3

#define AUG_MAX_BATCH 8    /* samples of one launch (the table is a kernel argument); a call takes any B */
#define AUG_MAX_RECTS 2
#define AUG_TILE 2048      /* pixels of one block iteration: 256 threads x 8 pixels */
#define AUG_MAX_PARTS 1024 /* blocks, and partial sums, per (sample, image) */

/* The jitter of one image. */
typedef struct aug_image_params {
  int order[4];    /* a permutation of AUG_BRIGHTNESS .. AUG_HUE: the operations in the order they are applied */
  float factor[3]; /* brightness, contrast, saturation: finite, >= 0 */
  int hue_shift;   /* 0..255, added to PIL's H byte modulo 256 */
} aug_image_params;

/* One sample.  shared != 0: the reference's symmetric branch, the pair jittered as ONE stacked image — image2 takes img[0]
 * and gamma_lut[b][0] as well, and the contrast level is the mean grey of both images together (img[1] must still be valid). */
typedef struct aug_sample {
  aug_image_params img[2];
  int shared;
  int n_rects;                /* 0..AUG_MAX_RECTS */
  int rect[AUG_MAX_RECTS][4]; /* x0, y0, dx, dy: 0 <= x0 < w, 0 <= y0 < h, dx, dy > 0; clipped at the right and bottom borders */
} aug_sample;

int aug_abi_version(void);
const char* aug_last_error_string(void);
const char* aug_source_hash(void);

/* HOST: the bytes aug_photometric_pair needs at `workspace`: B * 5 * min(ceil(h w / AUG_TILE), AUG_MAX_PARTS) uint64 partial
 * sums (two grey sums, three channel sums of image2); -1 for non-positive sizes.  No device is touched. */
int64_t aug_workspace_bytes(int B, int h, int w);

/* out1, out2 [B, 3, h, w] of out_dtype <- the jittered image1, image2 [B, 3, h, w] of in_dtype (AUG_U8 | AUG_F32; an fp32 input is
 * quantised once as clamp(floor(x + 0.5), 0, 255)), then the gamma table, then image2's rectangles.  samples: HOST array of B.
 * gamma_lut: device uint8 [B, 2, 256] or NULL (identity).  workspace: device, 8-byte aligned, need not be cleared.
 * fp32 images must be 4-byte aligned.  Up to three launches per AUG_MAX_BATCH samples: the grey sums (only if a contrast factor
 * of the chunk is not 1), the write-out, the rectangles (only if the chunk has one).  3 * B * h * w < 2^31. */
int aug_photometric_pair(const void* image1, const void* image2, int in_dtype, void* out1, void* out2, int out_dtype, int B, int h, int w,
                         const aug_sample* samples, const unsigned char* gamma_lut, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
