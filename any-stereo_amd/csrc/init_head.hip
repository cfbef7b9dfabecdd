// Backward of the IGEV init-disparity head (continuous_IGEVstereo.py:267-268, submodule.py:321-325): the classifier
// Conv3d(8 -> 1, 3x3x3, padding 1, no bias), softmax over D and the disparity regression, in the direction that
// train_continuous_IGEV.py:96-122 (--supervise_init) needs.  Per pixel, with p = softmax_d(cost), init = sum_d d * p_d and
// g = dL/d init:
//   dcost[b,d,y,x]   = g * p_d * (d - init)
//   d_geo[b,c,z,y,x] = sum_{kz,ky,kx} W[c,kz,ky,kx] * dcost[b, z-kz+1, y-ky+1, x-kx+1]          (zero outside)
//   dW[c,kz,ky,kx]   = sum_{b,z,y,x} geo[b,c,z,y,x] * dcost[b, z-kz+1, y-ky+1, x-kx+1]
// The second form of dW is the textbook sum over (b,d,y,x) of dcost * geo[.., d+kz-1, ..] with the summation index moved to
// the geo position: both gradients then read the SAME 27-value window of dcost per geo element.
//
// One block = one sample's 4 x 16 pixel tile, all D.  Phase 1: dcost of the tile plus a 1-pixel halo, every D, into LDS
// (the forward's cost gives p and init again; 4 lanes per pixel split D and combine in a fixed shuffle order).  Phase 2:
// wave c (8 waves) owns geo channel c, lane = pixel; the lane walks z with a 3-slice register window of dcost, reads each
// geo element once, writes each d_geo element once and keeps 27 dW accumulators, reduced across the wave at the end into
// the block's row of partials [nblocks, 216].  as_init_head_wgrad_reduce sums the rows in a fixed order: no atomics, no
// zero-fill, the same bits on every run.
#include "common.h"

namespace {

constexpr int kC = 8;                // geo channels (continuous_IGEVstereo.py:72: Conv3d(8, 1, 3, 1, 1))
constexpr int kTaps = 27;
constexpr int kTY = 4, kTX = 16;     // pixel tile: 64 pixels = one wave
constexpr int kHY = kTY + 2, kHX = kTX + 2, kHalo = kHY * kHX;  // 6 x 18 = 108 halo pixels
constexpr int kSplit = 4;            // lanes per halo pixel in phase 1
constexpr int kMaxD = 128;           // max_disp <= 512
constexpr int kThreads = kC * 64;

__device__ __forceinline__ float sum_xor(float v, int lanes) {
  for (int m = 1; m < lanes; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

__global__ __launch_bounds__(kThreads) void init_head_bwd_kernel(const float* __restrict__ geo, const float* __restrict__ weight,
                                                                 const float* __restrict__ cost, const float* __restrict__ gin,
                                                                 float* __restrict__ d_geo, float* __restrict__ partial, int D, int H,
                                                                 int W, int tiles_y, int tiles_x) {
  extern __shared__ float dcs[];  // [D][kHY][kHX]
  const int tid = threadIdx.x;
  const int blk = blockIdx.x;
  const int b = blk / (tiles_y * tiles_x);
  const int t = blk - b * tiles_y * tiles_x;
  const int y0 = (t / tiles_x) * kTY, x0 = (t % tiles_x) * kTX;
  const long long plane = (long long)H * W;

  // ---- phase 1a: the cost columns of the halo tile -> LDS (zero outside the image) ----
  const float* cb = cost + (long long)b * D * plane;
  for (int e = tid; e < D * kHalo; e += kThreads) {
    const int d = e / kHalo, r = e - d * kHalo;
    const int gy = y0 - 1 + r / kHX, gx = x0 - 1 + r % kHX;
    dcs[e] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? cb[(long long)d * plane + (long long)gy * W + gx] : 0.f;
  }
  __syncthreads();

  // ---- phase 1b: cost -> dcost in place, kSplit lanes per halo pixel (dispreg_bwd_kernel's arithmetic) ----
  {
    const int r = tid / kSplit, part = tid % kSplit;  // 432 of 512 lanes busy; groups of kSplit never straddle a wave
    const bool live = r < kHalo;
    const int rr = live ? r : 0;
    const int gy = y0 - 1 + rr / kHX, gx = x0 - 1 + rr % kHX;
    const bool inside = live && gy >= 0 && gy < H && gx >= 0 && gx < W;
    const int dend = live ? D : 0;  // idle lanes read nothing (their group's shuffles stay inside the group)
    float mx = -INFINITY;
    for (int d = part; d < dend; d += kSplit) mx = fmaxf(mx, dcs[d * kHalo + rr]);
    for (int m = 1; m < kSplit; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    float s = 0.f, m1 = 0.f;
    for (int d = part; d < dend; d += kSplit) {
      const float e = expf(dcs[d * kHalo + rr] - mx);
      s += e;
      m1 += e * (float)d;
    }
    s = sum_xor(s, kSplit);
    m1 = sum_xor(m1, kSplit);
    const float mean = m1 / s;
    const float g = inside ? gin[(long long)b * plane + (long long)gy * W + gx] : 0.f;
    for (int d = part; d < dend; d += kSplit) {
      const float pd = expf(dcs[d * kHalo + rr] - mx) / s;
      dcs[d * kHalo + rr] = inside ? g * pd * ((float)d - mean) : 0.f;
    }
  }
  __syncthreads();

  // ---- phase 2: wave c = geo channel c, lane = pixel of the tile ----
  const int c = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int ty = lane / kTX, tx = lane % kTX;
  const int gy = y0 + ty, gx = x0 + tx;
  const bool valid = gy < H && gx < W;
  float w[kTaps];
#pragma unroll
  for (int k = 0; k < kTaps; ++k) w[k] = weight[c * kTaps + k];
  // window slice of depth zz: s[ky*3+kx] = dcost[zz, y-ky+1, x-kx+1] = dcs[zz][ty+2-ky][tx+2-kx]
  const int base = (ty + 2) * kHX + (tx + 2);
  float sn[9], sc[9], sp[9];  // slices z+1 (kz = 0), z (kz = 1), z-1 (kz = 2)
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    sp[j] = 0.f;
    sc[j] = dcs[base - (j / 3) * kHX - (j % 3)];
    sn[j] = D > 1 ? dcs[kHalo + base - (j / 3) * kHX - (j % 3)] : 0.f;
  }
  float acc[kTaps];
#pragma unroll
  for (int k = 0; k < kTaps; ++k) acc[k] = 0.f;
  const long long off = (((long long)b * kC + c) * D) * plane + (long long)gy * W + gx;
  const float* gp = geo + off;
  float* op = d_geo + off;
  float gcur = valid ? gp[0] : 0.f;
  for (int z = 0; z < D; ++z) {
    const float gnext = (valid && z + 1 < D) ? gp[(long long)(z + 1) * plane] : 0.f;
    float o = 0.f;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      o = fmaf(w[j], sn[j], o);
      o = fmaf(w[9 + j], sc[j], o);
      o = fmaf(w[18 + j], sp[j], o);
      acc[j] = fmaf(gcur, sn[j], acc[j]);
      acc[9 + j] = fmaf(gcur, sc[j], acc[9 + j]);
      acc[18 + j] = fmaf(gcur, sp[j], acc[18 + j]);
    }
    if (valid) op[(long long)z * plane] = o;
    const int zn = z + 2;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      sp[j] = sc[j];
      sc[j] = sn[j];
      sn[j] = zn < D ? dcs[zn * kHalo + base - (j / 3) * kHX - (j % 3)] : 0.f;
    }
    gcur = gnext;
  }
  // taps are stored in the weight's order (kz, ky, kx): acc[j] holds kz = 0, acc[9 + j] kz = 1, acc[18 + j] kz = 2
  float* prow = partial + (long long)blk * (kC * kTaps) + c * kTaps;
#pragma unroll
  for (int k = 0; k < kTaps; ++k) {
    const float v = sum_xor(acc[k], 64);
    if (lane == 0) prow[k] = v;
  }
}

// dW[j] = sum over the partial rows in a fixed order: lane l adds rows l, l + 64, ...; then a fixed xor tree over the wave.
__global__ __launch_bounds__(64) void init_head_wgrad_reduce_kernel(const float* __restrict__ partial, int nrows,
                                                                    float* __restrict__ dw) {
  const int j = blockIdx.x;
  const int lane = threadIdx.x;
  float s = 0.f;
  for (int r = lane; r < nrows; r += 64) s += partial[(long long)r * (kC * kTaps) + j];
  s = sum_xor(s, 64);
  if (lane == 0) dw[j] = s;
}

inline long long init_head_blocks(int B, int H, int W) {
  return (long long)B * as::cdiv(H, kTY) * as::cdiv(W, kTX);
}

}  // namespace

extern "C" {

int64_t as_init_head_partial_elems(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return as::fail(AS_ERR_BAD_ARG, "init_head_partial_elems: non-positive size");
  return init_head_blocks(B, H, W) * (kC * kTaps);
}

int as_init_head_bwd(const float* geo, const float* weight, const float* cost, const float* g, float* d_geo, float* partial, int B,
                     int D, int H, int W, void* stream) {
  AS_REQUIRE(geo && weight && cost && g && d_geo && partial, AS_ERR_BAD_ARG, "init_head_bwd: null pointer");
  AS_REQUIRE(B > 0 && H > 0 && W > 0, AS_ERR_BAD_ARG, "init_head_bwd: non-positive size");
  AS_REQUIRE(D >= 1 && D <= kMaxD, AS_ERR_BAD_SHAPE, "init_head_bwd: D=%d outside [1,%d]", D, kMaxD);
  const long long nblk = init_head_blocks(B, H, W);
  AS_REQUIRE(nblk < 2147483647ll, AS_ERR_BAD_SHAPE, "init_head_bwd: too many tiles");
  const int ty = as::cdiv(H, kTY), tx = as::cdiv(W, kTX);
  const size_t lds = (size_t)D * kHalo * sizeof(float);  // <= 55296 B: no opt-in above 64 KB needed
  hipLaunchKernelGGL(init_head_bwd_kernel, dim3((unsigned)nblk), dim3(kThreads), lds, as::as_stream(stream), geo, weight, cost, g,
                     d_geo, partial, D, H, W, ty, tx);
  return as::check_launch("init_head_bwd");
}

int as_init_head_wgrad_reduce(const float* partial, int nrows, float* d_weight, void* stream) {
  AS_REQUIRE(partial && d_weight, AS_ERR_BAD_ARG, "init_head_wgrad_reduce: null pointer");
  AS_REQUIRE(nrows > 0, AS_ERR_BAD_ARG, "init_head_wgrad_reduce: non-positive row count");
  hipLaunchKernelGGL(init_head_wgrad_reduce_kernel, dim3(kC * kTaps), dim3(64), 0, as::as_stream(stream), partial, nrows, d_weight);
  return as::check_launch("init_head_wgrad_reduce");
}

}  // extern "C"
