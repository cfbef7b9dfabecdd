// On-device evaluation (evaluation.py:389-417, metrics_utils/metrics.py:44-90, metrics_utils/experiment.py:267-296).
//
// as_disp_metrics: ONE pass over N estimates against one ground truth gives, per (estimate, image), the 19 numbers from which
// EPE, D1 and Thres-1/2/3 over the regions all / non-occluded / occluded follow:
//   row = [ all: n, sum E, n_D1, n_T1, n_T2, n_T3 | noc: ... | occ: ... | n_gt_pos ]        (fp64)
// with E = |gt - est| in fp32, an estimate of +-inf counted as 0 (evaluation.py:389), D1 = E > 3 && E / |gt| > 0.05 (IEEE fp32
// division) and Thres-k = E > thres[k].  n_gt_pos counts gt > 0 over the whole image: the `_filter` rule of metrics.py:53
// divides by it.  A pixel is either noc or occ, so the kernel keeps those two sets of accumulators and forms all = noc + occ
// when it writes the row (counts: exact; sum E: one fp64 addition).
//
// Grid (chunks, B, N), 256 threads; a chunk is 2048 pixels, or a multiple of that (up to 16 x) once an image has more than
// 2^21 pixels, so that an image is never cut into more than ~1024 chunks and the per-block reduction stays a small share.
// Per-thread accumulators (counts as integers, sum E in fp64 from the first addition) -> fixed xor tree over the wave -> the
// block's 4 waves added in order -> one row of partial [N,B,chunks,19].  A second launch sums the chunk rows of every (estimate, image) in a fixed order.  No atomics, no zero-fill, every element of partial and
// of out is written: the same bits on every run, and an empty region is a row of zeros.
// An image whose pixel count is a multiple of 4 (every real evaluation size) is read with 16-byte loads of est / gt and 4-byte
// loads of the masks: each image plane then starts 16-byte aligned.  Any other size takes coalesced scalar loads.
//
// as_lr_consistency: the non-occluded mask of occ_mask(left_disp, right_disp) (experiment.py:286-296) without its two warped
// intermediate images.  Both warps are grid_sample(bilinear, border, align_corners=False) on a linspace(0,1,n) base grid, so the
// sampling coordinate of column j under a disparity d is clamp(j*W/(W-1) + d - 0.5, 0, W-1) and row i maps to
// clamp(i*H/(H-1) - 0.5, 0, H-1).  The first warp samples the identity ramp: its value is that clamped coordinate, l2r(i,j), a
// function of dr[i,j] alone.  The second warp interpolates l2r bilinearly at (row(i), col(j, -dl[i,j])): four reads of dr and one
// of dl per output pixel.  noc = |j - l2r2l| < thr.  The coordinates are formed in the reference's order of fp32 operations
// (linspace, / W, 2 * g - 1, ((g + 1) * n - 1) / 2), each one rounded on its own.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerThread = 8;                    // pixels per thread: two 16-byte loads per operand
constexpr int kChunk = kThreads * kPerThread;    // 2048 pixels per block and loop trip
constexpr int kTargetChunks = 1024;              // above this many chunks per image a block takes several trips ...
constexpr int kMaxTrips = 16;                    // ... up to this many
constexpr int kRow = 19;                         // 3 regions x (n, sum E, n_D1, n_T1, n_T2, n_T3) + n_gt_pos
constexpr int kAcc = 13;                         // what a block accumulates: noc (6), occ (6), n_gt_pos

struct Acc {
  unsigned n[2], d1[2], t1[2], t2[2], t3[2], pos;  // [0] = noc, [1] = occ
  double e[2];
};

__device__ __forceinline__ void add_pixel(Acc& a, float est, float g, bool valid, bool noc, float gt_lo, float gt_hi, float th1, float th2,
                                          float th3) {
  a.pos += g > 0.f ? 1u : 0u;
  const bool v = valid && g > gt_lo && g < gt_hi;
  const float x = isinf(est) ? 0.f : est;
  const float err = fabsf(g - x);
  const bool d1 = err > 3.f && __fdiv_rn(err, fabsf(g)) > 0.05f;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const bool in = v && (noc == (r == 0));
    a.n[r] += in ? 1u : 0u;
    if (in) a.e[r] += (double)err;  // a select, never a product: err may be inf or NaN outside the region
    a.d1[r] += (in && d1) ? 1u : 0u;
    a.t1[r] += (in && err > th1) ? 1u : 0u;
    a.t2[r] += (in && err > th2) ? 1u : 0u;
    a.t3[r] += (in && err > th3) ? 1u : 0u;
  }
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// all = noc + occ; the row layout of the header
__device__ __forceinline__ double row_value(const double* t, int j) {
  if (j < 6) return t[j] + t[6 + j];
  if (j < 18) return t[j - 6];
  return t[12];
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void disp_metrics_kernel(const float* __restrict__ est, const float* __restrict__ gt,
                                                                const unsigned char* __restrict__ valid,
                                                                const unsigned char* __restrict__ noc, double* __restrict__ partial,
                                                                int HW, int trips, float gt_lo, float gt_hi, float th1, float th2,
                                                                float th3) {
  __shared__ double red[kWaves][kAcc];
  __shared__ double tot[kAcc];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x, b = blockIdx.y, n = blockIdx.z;
  const int B = gridDim.y, chunks = gridDim.x;
  const long long img = (long long)b * HW;
  const float* ep = est + ((long long)n * B + b) * HW;
  const float* gp = gt + img;
  const unsigned char* vp = valid ? valid + img : nullptr;
  const unsigned char* np = noc ? noc + img : nullptr;
  const int base0 = chunk * trips * kChunk;  // < HW <= INT_MAX - kMaxTrips * kChunk (checked by the host)

  Acc a;
#pragma unroll
  for (int r = 0; r < 2; ++r) a.n[r] = a.d1[r] = a.t1[r] = a.t2[r] = a.t3[r] = 0u, a.e[r] = 0.0;
  a.pos = 0u;

  for (int trip = 0; trip < trips; ++trip) {
    const int base = base0 + trip * kChunk;
    if (base >= HW) break;
    if (kVec) {  // HW % 4 == 0: a group of 4 pixels is inside the image or outside it as a whole
#pragma unroll
      for (int it = 0; it < kPerThread / 4; ++it) {
        const int p = base + it * (kThreads * 4) + tid * 4;
        if (p < HW) {
          const float4 e4 = *reinterpret_cast<const float4*>(ep + p);
          const float4 g4 = *reinterpret_cast<const float4*>(gp + p);
          const unsigned v4 = vp ? *reinterpret_cast<const unsigned*>(vp + p) : 0x01010101u;
          const unsigned n4 = np ? *reinterpret_cast<const unsigned*>(np + p) : 0x01010101u;
          const float ev[4] = {e4.x, e4.y, e4.z, e4.w}, gv[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
          for (int k = 0; k < 4; ++k)
            add_pixel(a, ev[k], gv[k], ((v4 >> (8 * k)) & 0xffu) != 0u, ((n4 >> (8 * k)) & 0xffu) != 0u, gt_lo, gt_hi, th1, th2, th3);
        }
      }
    } else {
#pragma unroll
      for (int it = 0; it < kPerThread; ++it) {
        const int p = base + it * kThreads + tid;
        if (p < HW) add_pixel(a, ep[p], gp[p], vp ? vp[p] != 0 : true, np ? np[p] != 0 : true, gt_lo, gt_hi, th1, th2, th3);
      }
    }
  }

  // ---- wave: fixed xor tree; block: the waves in order ----
  const int wave = tid >> 6, lane = tid & 63;
  double w[kAcc];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    w[6 * r + 0] = (double)wave_sum(a.n[r]);
    w[6 * r + 1] = wave_sum(a.e[r]);
    w[6 * r + 2] = (double)wave_sum(a.d1[r]);
    w[6 * r + 3] = (double)wave_sum(a.t1[r]);
    w[6 * r + 4] = (double)wave_sum(a.t2[r]);
    w[6 * r + 5] = (double)wave_sum(a.t3[r]);
  }
  w[12] = (double)wave_sum(a.pos);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < kAcc; ++j) red[wave][j] = w[j];
  }
  __syncthreads();
  if (tid < kAcc) {
    double s = red[0][tid];
    for (int k = 1; k < kWaves; ++k) s += red[k][tid];
    tot[tid] = s;
  }
  __syncthreads();
  if (tid < kRow) partial[(((long long)n * B + b) * chunks + chunk) * kRow + tid] = row_value(tot, tid);
}

// out[nb][j] = the chunk rows of image nb summed in a fixed order: thread t adds rows t, t + 256, ...; xor tree; waves in order.
__global__ __launch_bounds__(kThreads) void disp_metrics_reduce_kernel(const double* __restrict__ partial, int chunks,
                                                                       double* __restrict__ out) {
  __shared__ double red[kWaves];
  const int j = blockIdx.x, tid = threadIdx.x;
  const long long nb = blockIdx.y;
  const double* p = partial + nb * chunks * kRow + j;
  double s = 0.0;
  for (int r = tid; r < chunks; r += kThreads) s += p[(long long)r * kRow];
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
    for (int k = 1; k < kWaves; ++k) t += red[k];
    out[nb * kRow + j] = t;
  }
}

// ---- left-right consistency ----
constexpr int kLrPerThread = 4;

// linspace(0, 1, n)[i] as torch builds it: step = 1 / (n - 1) (an fp32 division, done once by the host); the first half counts up
// from 0, the second half down from 1
__device__ __forceinline__ float linspace01(int i, int n, float step) {
  return i < n / 2 ? __fmul_rn(step, (float)i) : __fsub_rn(1.f, __fmul_rn(step, (float)(n - 1 - i)));
}
// grid value g in [0,1] units -> pixel coordinate of grid_sample(align_corners=False, padding_mode='border'); * 0.5 is / 2 exactly
__device__ __forceinline__ float sample_coord(float g01, int n) {
  const float g = __fsub_rn(__fmul_rn(2.f, g01), 1.f);
  const float x = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(g, 1.f), (float)n), 1.f), 0.5f);
  return fminf((float)(n - 1), fmaxf(x, 0.f));
}
__device__ __forceinline__ float l2r_at(const float* __restrict__ dr, int i, int j, int W, float step_w) {
  return sample_coord(__fadd_rn(linspace01(j, W, step_w), __fdiv_rn(dr[(long long)i * W + j], (float)W)), W);
}

__device__ __forceinline__ unsigned lr_pixel(const float* __restrict__ drb, float d_left, int p, int H, int W, float step_h, float step_w,
                                             float thr) {
  const int i = p / W, j = p - i * W;
  const float x = sample_coord(__fadd_rn(linspace01(j, W, step_w), __fdiv_rn(-d_left, (float)W)), W);
  const float y = sample_coord(linspace01(i, H, step_h), H);
  const float xf = floorf(x), yf = floorf(y);
  const int xa = min(max((int)xf, 0), W - 1), ya = min(max((int)yf, 0), H - 1);  // x, y are inside [0, n-1]; NaN lands on 0
  const int xb = min(xa + 1, W - 1), yb = min(ya + 1, H - 1);                    // a tap outside the image carries weight 0
  const float wx1 = __fsub_rn(x, xf), wx0 = __fsub_rn(__fadd_rn(xf, 1.f), x);
  const float wy1 = __fsub_rn(y, yf), wy0 = __fsub_rn(__fadd_rn(yf, 1.f), y);
  // grid_sample's order: nw, ne, sw, se
  float v = __fmul_rn(l2r_at(drb, ya, xa, W, step_w), __fmul_rn(wx0, wy0));
  v = __fadd_rn(v, __fmul_rn(l2r_at(drb, ya, xb, W, step_w), __fmul_rn(wx1, wy0)));
  v = __fadd_rn(v, __fmul_rn(l2r_at(drb, yb, xa, W, step_w), __fmul_rn(wx0, wy1)));
  v = __fadd_rn(v, __fmul_rn(l2r_at(drb, yb, xb, W, step_w), __fmul_rn(wx1, wy1)));
  return fabsf(__fsub_rn((float)j, v)) < thr ? 1u : 0u;
}

// One thread = 4 consecutive pixels (of the flattened image).  kVec (H*W % 4 == 0, 16-byte aligned planes): one 16-byte load of dl
// and one 4-byte store of the mask; otherwise per-pixel loads and byte stores.
template <bool kVec>
__global__ __launch_bounds__(kThreads) void lr_consistency_kernel(const float* __restrict__ dl, const float* __restrict__ dr,
                                                                  unsigned char* __restrict__ noc, int H, int W, float step_h,
                                                                  float step_w, float thr) {
  const int HW = H * W;
  const int p0 = (blockIdx.x * kThreads + threadIdx.x) * kLrPerThread;  // < HW + 4 * kThreads <= INT_MAX (checked by the host)
  if (p0 >= HW) return;
  const long long img = (long long)blockIdx.y * HW;
  const float* drb = dr + img;
  if (kVec) {
    const float4 d4 = *reinterpret_cast<const float4*>(dl + img + p0);
    const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
    unsigned m = 0u;
#pragma unroll
    for (int k = 0; k < kLrPerThread; ++k) m |= lr_pixel(drb, dv[k], p0 + k, H, W, step_h, step_w, thr) << (8 * k);
    *reinterpret_cast<unsigned*>(noc + img + p0) = m;
  } else {
#pragma unroll
    for (int k = 0; k < kLrPerThread; ++k) {
      const int p = p0 + k;
      if (p < HW) noc[img + p] = (unsigned char)lr_pixel(drb, dl[img + p], p, H, W, step_h, step_w, thr);
    }
  }
}

// loop trips of a block and chunks of an image of hw pixels
inline int metrics_trips(int64_t hw) {
  const int64_t t = as::cdiv64(hw, (int64_t)kChunk * kTargetChunks);
  return (int)(t < 1 ? 1 : (t > kMaxTrips ? kMaxTrips : t));
}
inline int64_t metrics_chunks(int64_t hw) { return as::cdiv64(hw, (int64_t)kChunk * metrics_trips(hw)); }

inline bool aligned(const void* p, size_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; }

}  // namespace

extern "C" {

int64_t as_disp_metrics_partial_elems(int N, int B, int H, int W) {
  if (N <= 0 || B <= 0 || H <= 0 || W <= 0) return as::fail(AS_ERR_BAD_ARG, "disp_metrics_partial_elems: non-positive size");
  const int64_t hw = (int64_t)H * W;
  return (int64_t)N * B * metrics_chunks(hw) * kRow;
}

int as_disp_metrics(const float* est, const float* gt, const unsigned char* valid, const unsigned char* noc, double* partial,
                    double* out, int N, int B, int H, int W, float gt_lo, float gt_hi, float thres1, float thres2, float thres3,
                    void* stream) {
  AS_REQUIRE(est && gt && partial && out, AS_ERR_BAD_ARG, "disp_metrics: null pointer");
  AS_REQUIRE(N > 0 && B > 0 && H > 0 && W > 0, AS_ERR_BAD_ARG, "disp_metrics: non-positive size");
  const int64_t hw = (int64_t)H * W;
  AS_REQUIRE(hw <= 2147483647ll - (int64_t)kMaxTrips * kChunk, AS_ERR_BAD_SHAPE, "disp_metrics: image of %lld pixels too large", (long long)hw);
  AS_REQUIRE(B <= 65535 && N <= 65535 && (int64_t)N * B <= 2147483647ll, AS_ERR_BAD_SHAPE, "disp_metrics: B=%d or N=%d above 65535", B, N);
  const int trips = metrics_trips(hw);
  const int chunks = (int)metrics_chunks(hw);
  const bool vec = hw % 4 == 0 && aligned(est, 16) && aligned(gt, 16) && aligned(valid, 4) && aligned(noc, 4);
  const dim3 grid((unsigned)chunks, (unsigned)B, (unsigned)N);
  hipStream_t s = as::as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(disp_metrics_kernel<true>, grid, dim3(kThreads), 0, s, est, gt, valid, noc, partial, (int)hw, trips, gt_lo, gt_hi,
                       thres1, thres2, thres3);
  else
    hipLaunchKernelGGL(disp_metrics_kernel<false>, grid, dim3(kThreads), 0, s, est, gt, valid, noc, partial, (int)hw, trips, gt_lo, gt_hi,
                       thres1, thres2, thres3);
  int rc = as::check_launch("disp_metrics");
  if (rc != AS_OK) return rc;
  hipLaunchKernelGGL(disp_metrics_reduce_kernel, dim3(kRow, (unsigned)(N * B)), dim3(kThreads), 0, s, partial, chunks, out);
  return as::check_launch("disp_metrics_reduce");
}

int as_lr_consistency(const float* dl, const float* dr, unsigned char* noc, int B, int H, int W, float thr, void* stream) {
  AS_REQUIRE(dl && dr && noc, AS_ERR_BAD_ARG, "lr_consistency: null pointer");
  AS_REQUIRE(B > 0 && H > 0 && W > 0, AS_ERR_BAD_ARG, "lr_consistency: non-positive size");
  AS_REQUIRE(H >= 2 && W >= 2, AS_ERR_BAD_SHAPE, "lr_consistency: H=%d, W=%d (the base grid divides by n - 1)", H, W);
  const int64_t hw = (int64_t)H * W;
  AS_REQUIRE(hw <= 2147483647ll - kLrPerThread * kThreads && B <= 65535, AS_ERR_BAD_SHAPE,
             "lr_consistency: image too large or B=%d above 65535", B);
  const float step_h = 1.f / (float)(H - 1), step_w = 1.f / (float)(W - 1);  // IEEE fp32 divisions (no fast-math in this build)
  const dim3 grid((unsigned)as::cdiv64(hw, kLrPerThread * kThreads), (unsigned)B);
  if (hw % 4 == 0 && aligned(dl, 16) && aligned(noc, 4))
    hipLaunchKernelGGL(lr_consistency_kernel<true>, grid, dim3(kThreads), 0, as::as_stream(stream), dl, dr, noc, H, W, step_h, step_w, thr);
  else
    hipLaunchKernelGGL(lr_consistency_kernel<false>, grid, dim3(kThreads), 0, as::as_stream(stream), dl, dr, noc, H, W, step_h, step_w, thr);
  return as::check_launch("lr_consistency");
}

}  // extern "C"
