// AffinityFeature with a 3x3, 5x5 or 7x7 window (liif.py:417-446 with --lsp_width / --lsp_height), forward and backward.
// n(p) = max(||x(p)||, eps), xh = x / n, aff_j(p) = max(0, xh(p)·xh(p+o_j)), o_j = (ky-R, kx-R) row-major without the centre.
//
// A per-pixel kernel that reads every neighbour through L2 (sf_affinity_kernel, csrc/liif.hip) moves win^2 times the input: fine
// for 9 taps, 1.1 GB for a 23 MB map at 7x7.  Here a block owns a 16x16 pixel tile plus its halo of R: it walks the channels in
// chunks of 8 whose NORMALISED values it stages in LDS (8 x 22 x 22 floats = 15.5 KB at 7x7; outside the map: 0; the next chunk's
// loads are in flight while a chunk is summed), and every thread keeps the n <= 48 sums of its pixel in registers.  The map is
// read (1 + 2R/16)^2 times, from LDS win^2 times.
// The backward has the same shape: the n weights w_j(p) of a pixel are gathered once into registers, then the same staged
// chunks give  sum_j w_j(p) xh_c(p+o_j)  per channel — every thread writes its own pixel, no atomics.
#include "common.h"

namespace {

constexpr int kTile = 16;  // pixels per tile side: 256 threads, one pixel each
constexpr int kChunk = 8;  // channels staged per step

template <int WIN>
struct Geo {
  static constexpr int R = WIN / 2, T = kTile + 2 * R, TT = T * T, N = WIN * WIN - 1;
  static constexpr int PER = (kChunk * TT + 255) / 256;  // staged values per thread and chunk
};

// pass 1: the clamped L2 norm over channels to ws[b,y,x]; with `out`, x is copied into out[:, :C] on the way (the concat form)
__global__ __launch_bounds__(256) void aw_norm_kernel(const float* __restrict__ x, float* __restrict__ out, long long out_bs,
                                                      float* __restrict__ ws, int C, long long plane, long long P) {
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= P) return;
  const long long b = pix / plane, rem = pix - b * plane;
  const float* xp = x + b * C * plane + rem;
  float* op = out ? out + b * out_bs + rem : nullptr;
  float ss = 0.f;
  int c = 0;
  for (; c + 8 <= C; c += 8) {  // 8 independent loads in flight per lane
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = xp[(long long)(c + i) * plane];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (op) op[(long long)(c + i) * plane] = v[i];
      ss += v[i] * v[i];
    }
  }
  for (; c < C; ++c) {
    const float v = xp[(long long)c * plane];
    if (op) op[(long long)c * plane] = v;
    ss += v * v;
  }
  ws[pix] = fmaxf(sqrtf(ss), 1e-12f);  // F.normalize: x / max(||x||_2, eps)
}

// the norms of the tile and its halo; 0 marks a pixel outside the map (a norm inside it is at least eps)
template <int WIN>
__device__ __forceinline__ void stage_norms(float* __restrict__ s_n, const float* __restrict__ np, int y0, int x0, int H, int W) {
  using G = Geo<WIN>;
  for (int e = threadIdx.x; e < G::TT; e += 256) {
    const int hy = e / G::T, hx = e - hy * G::T;
    const int gy = y0 - G::R + hy, gx = x0 - G::R + hx;
    s_n[e] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? np[(long long)gy * W + gx] : 0.f;
  }
}

// Channels [c0, c0 + kChunk) of the tile and its halo go through registers: load_chunk issues a thread's PER loads back to back
// (one memory latency per chunk, not one per element) and is called for chunk k+1 BEFORE the sums of chunk k, so that latency
// hides behind them; store_chunk normalises (IEEE division: the literal x / n of F.normalize) and parks the values in LDS, 0
// outside the map and past the last channel.
template <int WIN>
__device__ __forceinline__ void load_chunk(float (&v)[Geo<WIN>::PER], const float* __restrict__ s_n, const float* __restrict__ xb,
                                           int c0, int C, long long plane, int y0, int x0, int W) {
  using G = Geo<WIN>;
#pragma unroll
  for (int i = 0; i < G::PER; ++i) {
    const int e = threadIdx.x + 256 * i;
    const int c = e / G::TT, r = e - c * G::TT;
    const int hy = r / G::T, hx = r - hy * G::T;
    v[i] = 0.f;
    if (e < kChunk * G::TT && c0 + c < C && s_n[r] > 0.f)
      v[i] = xb[(long long)(c0 + c) * plane + (long long)(y0 - G::R + hy) * W + (x0 - G::R + hx)];
  }
}

template <int WIN>
__device__ __forceinline__ void store_chunk(float* __restrict__ s_x, const float* __restrict__ s_n, const float (&v)[Geo<WIN>::PER]) {
  using G = Geo<WIN>;
#pragma unroll
  for (int i = 0; i < G::PER; ++i) {
    const int e = threadIdx.x + 256 * i;
    if (e < kChunk * G::TT) {
      const float n = s_n[e % G::TT];
      s_x[e] = n > 0.f ? __fdiv_rn(v[i], n) : 0.f;
    }
  }
}

struct TilePos {
  int b, y0, x0;
};

__device__ __forceinline__ TilePos tile_pos(int tiles_x, int tiles_y) {
  const int blk = blockIdx.x;
  const int t = blk / tiles_x;
  TilePos p;
  p.x0 = (blk - t * tiles_x) * kTile;
  p.b = t / tiles_y;
  p.y0 = (t - p.b * tiles_y) * kTile;
  return p;
}

// pass 2: aff points at channel 0 of the affinity planes of batch element 0 (inside cat(x, aff) or alone), aff_bs floats apart
template <int WIN>
__global__ __launch_bounds__(256, 2) void aw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ ws, float* __restrict__ aff,
                                                     long long aff_bs, int C, int H, int W, int tiles_x, int tiles_y) {
  using G = Geo<WIN>;
  __shared__ float s_n[G::TT];
  __shared__ float s_x[kChunk * G::TT];
  const TilePos tp = tile_pos(tiles_x, tiles_y);
  const long long plane = (long long)H * W;
  const float* xb = x + (long long)tp.b * C * plane;
  const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
  const int y = tp.y0 + ly, xx = tp.x0 + lx;
  stage_norms<WIN>(s_n, ws + (long long)tp.b * plane, tp.y0, tp.x0, H, W);
  float acc[G::N];
#pragma unroll
  for (int j = 0; j < G::N; ++j) acc[j] = 0.f;
  __syncthreads();  // s_n
  float v[G::PER];
  load_chunk<WIN>(v, s_n, xb, 0, C, plane, tp.y0, tp.x0, W);
  for (int c0 = 0; c0 < C; c0 += kChunk) {
    if (c0) __syncthreads();  // the previous chunk has been read
    store_chunk<WIN>(s_x, s_n, v);
    __syncthreads();
    if (c0 + kChunk < C) load_chunk<WIN>(v, s_n, xb, c0 + kChunk, C, plane, tp.y0, tp.x0, W);
#pragma unroll 2  // a full unroll hoists 8 x n LDS reads: 256 registers, one wave per SIMD
    for (int c = 0; c < kChunk; ++c) {
      const float* sc = s_x + c * G::TT + ly * G::T + lx;
      const float fc = sc[G::R * G::T + G::R];
      int j = 0;
#pragma unroll
      for (int ky = 0; ky < WIN; ++ky)
#pragma unroll
        for (int kx = 0; kx < WIN; ++kx) {
          if (ky == G::R && kx == G::R) continue;
          acc[j] = fmaf(fc, sc[ky * G::T + kx], acc[j]);
          ++j;
        }
    }
  }
  if (y >= H || xx >= W) return;
  float* op = aff + (long long)tp.b * aff_bs + (long long)y * W + xx;
  int j = 0;
#pragma unroll
  for (int ky = 0; ky < WIN; ++ky)
#pragma unroll
    for (int kx = 0; kx < WIN; ++kx) {
      if (ky == G::R && kx == G::R) continue;
      const int yy = y + ky - G::R, x2 = xx + kx - G::R;
      const bool ok = yy >= 0 && yy < H && x2 >= 0 && x2 < W;
      op[(long long)j * plane] = ok ? fmaxf(acc[j], 0.f) : 0.f;
      ++j;
    }
}

// With g_j the incoming gradient and o_(n-1-j) = -o_j:  w_j(p) = [aff_j(p) > 0] g_j(p) + [aff_(n-1-j)(p+o_j) > 0] g_(n-1-j)(p+o_j),
// dx_c(p) = (sum_j w_j(p) xh_c(p+o_j) - xh_c(p) sum_j w_j(p) aff_j(p)) / n(p)   (+ the pass-through gradient of cat(x, aff));
// the formula of affinity_bwd_kernel (csrc/liif_variants.hip) for n neighbours.
template <int WIN>
__global__ __launch_bounds__(256) void aw_bwd_kernel(const float* __restrict__ x, const float* __restrict__ ws,
                                                     const float* __restrict__ aff, long long aff_bs, const float* __restrict__ g_aff,
                                                     long long g_aff_bs, const float* __restrict__ g_x, long long g_x_bs,
                                                     float* __restrict__ dx, int C, int H, int W, int tiles_x, int tiles_y) {
  using G = Geo<WIN>;
  __shared__ float s_n[G::TT];
  __shared__ float s_x[kChunk * G::TT];
  const TilePos tp = tile_pos(tiles_x, tiles_y);
  const long long plane = (long long)H * W;
  const float* xb = x + (long long)tp.b * C * plane;
  const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
  const int y = tp.y0 + ly, xx = tp.x0 + lx;
  const bool inmap = y < H && xx < W;
  const long long rem = (long long)y * W + xx;
  stage_norms<WIN>(s_n, ws + (long long)tp.b * plane, tp.y0, tp.x0, H, W);
  float w[G::N];
  float dot = 0.f;
  {
    const float* ap = aff + (long long)tp.b * aff_bs;
    const float* gp = g_aff + (long long)tp.b * g_aff_bs;
    int j = 0;
#pragma unroll
    for (int ky = 0; ky < WIN; ++ky)
#pragma unroll
      for (int kx = 0; kx < WIN; ++kx) {
        if (ky == G::R && kx == G::R) continue;
        const int yy = y + ky - G::R, x2 = xx + kx - G::R;
        float wj = 0.f;
        if (inmap && yy >= 0 && yy < H && x2 >= 0 && x2 < W) {
          const float a = ap[(long long)j * plane + rem];
          if (a > 0.f) wj = gp[(long long)j * plane + rem];
          const long long q = (long long)yy * W + x2;
          if (ap[(long long)(G::N - 1 - j) * plane + q] > 0.f) wj += gp[(long long)(G::N - 1 - j) * plane + q];
          dot = fmaf(wj, a, dot);
        }
        w[j] = wj;
        ++j;
      }
  }
  __syncthreads();  // s_n
  const float n0 = s_n[(ly + G::R) * G::T + lx + G::R];
  const float inv_n0 = inmap ? 1.f / n0 : 0.f;
  float* dxp = dx + (long long)tp.b * C * plane + rem;
  const float* gx = g_x ? g_x + (long long)tp.b * g_x_bs + rem : nullptr;
  float v[G::PER];
  load_chunk<WIN>(v, s_n, xb, 0, C, plane, tp.y0, tp.x0, W);
  for (int c0 = 0; c0 < C; c0 += kChunk) {
    if (c0) __syncthreads();  // the previous chunk has been read
    store_chunk<WIN>(s_x, s_n, v);
    __syncthreads();
    if (c0 + kChunk < C) load_chunk<WIN>(v, s_n, xb, c0 + kChunk, C, plane, tp.y0, tp.x0, W);
#pragma unroll 2  // a full unroll hoists 8 x n LDS reads: 256 registers, one wave per SIMD
    for (int c = 0; c < kChunk; ++c) {
      if (c0 + c >= C) break;
      const float* sc = s_x + c * G::TT + ly * G::T + lx;
      float acc = 0.f;
      int j = 0;
#pragma unroll
      for (int ky = 0; ky < WIN; ++ky)
#pragma unroll
        for (int kx = 0; kx < WIN; ++kx) {
          if (ky == G::R && kx == G::R) continue;
          acc = fmaf(w[j], sc[ky * G::T + kx], acc);
          ++j;
        }
      if (inmap) {
        float d = (acc - sc[G::R * G::T + G::R] * dot) * inv_n0;
        if (gx) d += gx[(long long)(c0 + c) * plane];
        dxp[(long long)(c0 + c) * plane] = d;
      }
    }
  }
}

// the checks both entries share; on success the tile grid of the launch
int check_shape(const char* what, int B, int C, int H, int W, int win, int* tiles_x, int* tiles_y, long long* blocks) {
  AS_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, AS_ERR_BAD_ARG, "%s: non-positive size (B=%d C=%d H=%d W=%d)", what, B, C, H, W);
  AS_REQUIRE(win == 3 || win == 5 || win == 7, AS_ERR_BAD_ARG, "%s: win must be 3, 5 or 7, got %d", what, win);
  const long long plane = (long long)H * W;
  AS_REQUIRE(plane < 2147483648ll, AS_ERR_BAD_SHAPE, "%s: plane of %lld pixels (2^31 or more)", what, plane);
  const long long chans = (long long)C + (long long)win * win - 1;
  AS_REQUIRE(chans <= 0x7FFFFFFFFFFFFFFFll / 4 / plane / B, AS_ERR_BAD_SHAPE, "%s: tensor of 2^63 bytes or more", what);
  *tiles_x = as::cdiv(W, kTile);
  *tiles_y = as::cdiv(H, kTile);
  *blocks = (long long)B * *tiles_x * *tiles_y;
  AS_REQUIRE(*blocks < 2147483648ll && as::cdiv64(plane * B, 256) < 2147483648ll, AS_ERR_BAD_SHAPE, "%s: more than 2^31-1 blocks", what);
  return AS_OK;
}

}  // namespace

extern "C" {

int64_t as_affinity_window_ws_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (int64_t)B * H * W * 4;
}

int as_affinity_window(const float* x, float* out, float* ws, int B, int C, int H, int W, int win, int with_x, void* stream) {
  AS_REQUIRE(x && out && ws, AS_ERR_BAD_ARG, "affinity_window: null pointer");
  int tiles_x = 0, tiles_y = 0;
  long long blocks = 0;
  const int rc = check_shape("affinity_window", B, C, H, W, win, &tiles_x, &tiles_y, &blocks);
  if (rc != AS_OK) return rc;
  const long long plane = (long long)H * W, P = plane * B;
  const int n = win * win - 1;
  const long long out_bs = (long long)(with_x ? C + n : n) * plane;
  float* aff = out + (with_x ? (long long)C * plane : 0ll);
  hipStream_t s = as::as_stream(stream);
  hipLaunchKernelGGL(aw_norm_kernel, dim3((unsigned)as::cdiv64(P, 256)), dim3(256), 0, s, x, with_x ? out : nullptr, out_bs, ws, C, plane,
                     P);
  const dim3 grid((unsigned)blocks);
  if (win == 3)
    hipLaunchKernelGGL(aw_fwd_kernel<3>, grid, dim3(256), 0, s, x, (const float*)ws, aff, out_bs, C, H, W, tiles_x, tiles_y);
  else if (win == 5)
    hipLaunchKernelGGL(aw_fwd_kernel<5>, grid, dim3(256), 0, s, x, (const float*)ws, aff, out_bs, C, H, W, tiles_x, tiles_y);
  else
    hipLaunchKernelGGL(aw_fwd_kernel<7>, grid, dim3(256), 0, s, x, (const float*)ws, aff, out_bs, C, H, W, tiles_x, tiles_y);
  return as::check_launch("affinity_window");
}

int as_affinity_window_bwd(const float* x, const float* aff, long long aff_batch_stride, const float* g_aff,
                           long long g_aff_batch_stride, const float* g_x, long long g_x_batch_stride, float* dx, float* ws, int B,
                           int C, int H, int W, int win, void* stream) {
  AS_REQUIRE(x && aff && g_aff && dx && ws, AS_ERR_BAD_ARG, "affinity_window_bwd: null pointer");
  int tiles_x = 0, tiles_y = 0;
  long long blocks = 0;
  const int rc = check_shape("affinity_window_bwd", B, C, H, W, win, &tiles_x, &tiles_y, &blocks);
  if (rc != AS_OK) return rc;
  const long long plane = (long long)H * W, P = plane * B;
  const int n = win * win - 1;
  AS_REQUIRE(aff_batch_stride >= n * plane && g_aff_batch_stride >= n * plane && (!g_x || g_x_batch_stride >= C * plane),
             AS_ERR_BAD_SHAPE, "affinity_window_bwd: batch stride smaller than the tensor");
  hipStream_t s = as::as_stream(stream);
  hipLaunchKernelGGL(aw_norm_kernel, dim3((unsigned)as::cdiv64(P, 256)), dim3(256), 0, s, x, (float*)nullptr, 0ll, ws, C, plane, P);
  const dim3 grid((unsigned)blocks);
#define AW_BWD(WIN_)                                                                                                              \
  hipLaunchKernelGGL(aw_bwd_kernel<WIN_>, grid, dim3(256), 0, s, x, (const float*)ws, aff, aff_batch_stride, g_aff, g_aff_batch_stride, \
                     g_x, g_x_batch_stride, dx, C, H, W, tiles_x, tiles_y)
  if (win == 3)
    AW_BWD(3);
  else if (win == 5)
    AW_BWD(5);
  else
    AW_BWD(7);
#undef AW_BWD
  return as::check_launch("affinity_window_bwd");
}

}  // extern "C"
