// What of a multi-scale training sample is a function of (ground-truth crop, scale, seed), on the device: the tail of
// StereoDataset.__getitem__ (models/*/stereo_datasets.py:148-212) — make_coord of the whole high-resolution crop, the
// np.random.choice(N, sample_q, replace=False) draw, the gathers, the boolean-mask splits of the sparse datasets and the 1/4-resolution
// target of --supervise_init.  A batch is ragged (every sample has its own crop size); a launch carries a table of kMaxBatch samples by
// value and blockIdx.y picks the sample, larger batches are chunked by the entry points.
//
// as_train_queries.  One thread = one query: pixel index -> (row, column) -> make_coord's two values, the crop's value (copied, never
// computed with), the index.  A random draw without replacement is pi(j) for a keyed bijection pi of [0, n): a Feistel network over
// the next power-of-two domain, walked until the value is below n.  The halves have floor(bits / 2) and ceil(bits / 2) bits and swap
// every round ((L, R) -> (R, L ^ F(R, key))), which is a bijection of the domain for every split, 0 bits included; the domain is
// below 2 n, so a walk takes under two steps on average.  Queries are independent: no sort, no table of taken pixels.
// The sparse modes need "the k-th valid / invalid pixel in raster order".  Three launches build, per sample, one list of N pixel
// indices — the valid ones first, then the invalid ones, both in raster order: count (valid pixels of every 2048-pixel tile), scan
// (one block per sample turns the tile counts into exclusive offsets and writes V), scatter (ballot ranks inside the tile).  With
// that list SPARSE_ORDERED is list[j], and SPARSE is list[j] for j < V followed by list[V + pi(j - V)], or list[pi(j)] when Q < V.
// No block waits for another block.
//
// as_low_disp.  ATen's upsample_bilinear2d(align_corners=False) of every crop to [h_out, w_out], then one division by 4 * scale.
//
// Every operation of the coordinate and the resize arithmetic is rounded on its own, as the torch ops it restates are: no FMA
// contraction in this file.
#include "common.h"
#include "query.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / as::kWave;
constexpr int kItems = 8;                    // pixels of a thread in count / scatter
constexpr int kTile = kThreads * kItems;     // pixels of a block: item k of thread t is pixel tile * kTile + k * kThreads + t
constexpr int kMaxBatch = 8;                 // samples of one launch (the table is a kernel argument)
constexpr int kRounds = 6;

struct Sample {
  const float* crop;
  int* list;       // [n] valid pixels, then invalid pixels, both in raster order (sparse modes)
  int* tile_off;   // [tiles] valid pixels in front of a tile (count writes the tile's own count, scan makes it exclusive)
  int h, w, n, tiles;
  float c0h, steph, c0w, stepw;   // make_coord (query.h: coord_axis): value(i) = c0 + step * i
  float scale;                    // copied to scale_out, so the batch's `scale` tensor needs no upload
  uint32_t key[kRounds];
};
struct Table {
  Sample s[kMaxBatch];
};

struct LowSample {
  const float* crop;
  int h, w;
  float ratio_h, ratio_w, div;
};
struct LowTable {
  LowSample s[kMaxBatch];
};

// ---- the keyed bijection ----
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x21f0aaadu;
  x ^= x >> 15;
  x *= 0x735a2d97u;
  x ^= x >> 15;
  return x;
}

__device__ __forceinline__ uint32_t feistel(uint32_t x, int bits, const uint32_t* key) {
  int lb = bits >> 1, rb = bits - lb;  // bits <= 31, so every shift below is under 32
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const uint32_t left = x >> rb, right = x & ((1u << rb) - 1u);
    const uint32_t nr = left ^ (mix32(right ^ key[r]) & ((1u << lb) - 1u));
    x = (right << lb) | nr;
    const int t = lb;
    lb = rb;
    rb = t;
  }
  return x;
}

// pi(j) over [0, n), 0 <= j < n, 1 <= n < 2^31
__device__ __forceinline__ int permute(int j, int n, const uint32_t* key) {
  const int bits = n <= 1 ? 0 : 32 - __clz(n - 1);
  uint32_t x = (uint32_t)j;
  do {
    x = feistel(x, bits, key);
  } while (x >= (uint32_t)n);  // the walk stays on the cycle of j, which re-enters [0, n) at the latest at j itself
  return (int)x;
}

inline void derive_keys(uint64_t seed, int b, int mode, uint32_t* key) {
  for (int r = 0; r < kRounds; ++r) {
    uint32_t t = mix32((uint32_t)seed + 0x9e3779b9u * (uint32_t)(r + 1));
    t = mix32(t ^ (uint32_t)(seed >> 32));
    t = mix32(t ^ ((uint32_t)b * 0x85ebca6bu));
    key[r] = mix32(t ^ (uint32_t)mode);
  }
}

// ---- the ordered pixel list of the sparse modes ----
__global__ __launch_bounds__(kThreads) void count_kernel(Table t) {
  const Sample& s = t.s[blockIdx.y];
  const int tile = blockIdx.x;
  if (tile >= s.tiles) return;
  __shared__ int wave_sum[kWaves];
  const int tid = threadIdx.x;
  const long long base = (long long)tile * kTile + tid;
  int c = 0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const long long i = base + k * kThreads;
    const bool valid = i < s.n && s.crop[i] > 0.f;
    c += __popcll(__builtin_amdgcn_ballot_w64(valid));  // the wave's count, the same in every lane
  }
  if ((tid & 63) == 0) wave_sum[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) sum += wave_sum[w];
    s.tile_off[tile] = sum;
  }
}

// one block per sample: tile counts -> exclusive offsets, in place; V -> n_valid
__global__ __launch_bounds__(kThreads) void scan_kernel(Table t, int* __restrict__ n_valid) {
  const Sample& s = t.s[blockIdx.x];
  __shared__ int wave_tot[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int base = 0; base < s.tiles; base += kThreads) {
    const int i = base + tid;
    const int v = i < s.tiles ? s.tile_off[i] : 0;
    int x = v;  // inclusive scan of the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane == 63) wave_tot[wave] = x;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int wt = wave_tot[w];
      if (w < wave) before += wt;
      total += wt;
    }
    if (i < s.tiles) s.tile_off[i] = carry + before + x - v;
    carry += total;
    __syncthreads();  // wave_tot is rewritten by the next chunk
  }
  if (tid == 0) n_valid[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kThreads) void scatter_kernel(Table t, const int* __restrict__ n_valid) {
  const Sample& s = t.s[blockIdx.y];
  const int tile = blockIdx.x;
  if (tile >= s.tiles) return;
  __shared__ int cnt[kItems * kWaves];  // valid pixels of (item k, wave w), then their exclusive prefix in (k, w) order = pixel order
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long base = (long long)tile * kTile + tid;
  const unsigned long long below = (1ull << lane) - 1ull;
  bool valid[kItems];
  int rank[kItems];
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const long long i = base + k * kThreads;
    valid[k] = i < s.n && s.crop[i] > 0.f;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(valid[k]);
    rank[k] = __popcll(bal & below);
    if (lane == 0) cnt[k * kWaves + wave] = __popcll(bal);
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int e = 0; e < kItems * kWaves; ++e) {
      const int c = cnt[e];
      cnt[e] = run;
      run += c;
    }
  }
  __syncthreads();
  const int V = n_valid[blockIdx.y];
  const int off = s.tile_off[tile];
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const long long i = base + k * kThreads;
    if (i >= s.n) continue;
    const int vb = off + cnt[k * kWaves + wave] + rank[k];  // valid pixels in front of pixel i: vb < V when i is valid,
    if (valid[k]) s.list[vb] = (int)i;                      // and i - vb = invalid pixels in front of i < n - V when it is not
    else s.list[(long long)V + (i - vb)] = (int)i;
  }
}

// ---- the queries ----
__global__ __launch_bounds__(kThreads) void queries_kernel(Table t, int Q, int mode, float* __restrict__ hr_coord,
                                                           float* __restrict__ hr_disp, int* __restrict__ index,
                                                           int* __restrict__ n_valid, float* __restrict__ scale_out) {
  const int b = blockIdx.y;
  const Sample& s = t.s[b];
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= Q) return;
  int idx;
  if (mode == AS_TQ_DENSE) {
    idx = permute(j, s.n, s.key);
  } else if (mode == AS_TQ_DENSE_ALL) {
    idx = j;
  } else if (mode == AS_TQ_SPARSE) {
    const int V = n_valid[b];
    if (Q < V) idx = s.list[permute(j, V, s.key)];
    else if (j < V) idx = s.list[j];
    else idx = s.list[(long long)V + permute(j - V, s.n - V, s.key)];  // j - V < Q - V <= n - V
  } else {
    idx = s.list[j];  // Q <= n
  }
  if ((mode == AS_TQ_DENSE || mode == AS_TQ_DENSE_ALL) && j == 0) n_valid[b] = s.n;
  if (scale_out && j == 0) scale_out[b] = s.scale;
  const int y = idx / s.w, x = idx - y * s.w;
  const long long o = (long long)b * Q + j;
  *reinterpret_cast<float2*>(hr_coord + 2 * o) = make_float2(s.c0h + s.steph * (float)y, s.c0w + s.stepw * (float)x);
  hr_disp[o] = s.crop[idx];
  index[o] = idx;
}

// ---- as_low_disp ----
constexpr int kTileX = 64;
constexpr int kTileY = kThreads / kTileX;

__device__ __forceinline__ void bilinear_axis(int d, float ratio, int n_in, int& i0, int& i1, float& l0, float& l1) {
  const float src = fmaxf(ratio * ((float)d + 0.5f) - 0.5f, 0.f);
  i0 = min((int)src, n_in - 1);
  i1 = min(i0 + 1, n_in - 1);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

__global__ __launch_bounds__(kThreads) void low_disp_kernel(LowTable t, float* __restrict__ out, int h_out, int w_out) {
  const int x = blockIdx.x * kTileX + (threadIdx.x % kTileX);
  const int y = blockIdx.y * kTileY + (threadIdx.x / kTileX);
  if (x >= w_out || y >= h_out) return;
  const LowSample& s = t.s[blockIdx.z];
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  bilinear_axis(y, s.ratio_h, s.h, y0, y1, ly0, ly1);
  bilinear_axis(x, s.ratio_w, s.w, x0, x1, lx0, lx1);
  const float* r0 = s.crop + (long long)y0 * s.w;
  const float* r1 = s.crop + (long long)y1 * s.w;
  const float v = ly0 * (lx0 * r0[x0] + lx1 * r0[x1]) + ly1 * (lx0 * r1[x0] + lx1 * r1[x1]);
  out[((long long)blockIdx.z * h_out + y) * w_out + x] = v / s.div;
}

inline bool known_mode(int mode) { return mode >= AS_TQ_DENSE && mode <= AS_TQ_SPARSE_ORDERED; }
inline bool sparse_mode(int mode) { return mode == AS_TQ_SPARSE || mode == AS_TQ_SPARSE_ORDERED; }

// the checks the entry points share; fills nothing
int check_sizes(const char* what, const int* h_hr, const int* w_hr, int B) {
  AS_REQUIRE(h_hr && w_hr, AS_ERR_BAD_ARG, "%s: null pointer", what);
  AS_REQUIRE(B > 0, AS_ERR_BAD_ARG, "%s: non-positive B=%d", what, B);
  for (int b = 0; b < B; ++b) {
    AS_REQUIRE(h_hr[b] > 0 && w_hr[b] > 0, AS_ERR_BAD_ARG, "%s: sample %d: non-positive size %dx%d", what, b, h_hr[b], w_hr[b]);
    AS_REQUIRE((int64_t)h_hr[b] * w_hr[b] <= 2147483647ll, AS_ERR_BAD_SHAPE, "%s: sample %d: %dx%d is more than 2^31-1 elements", what,
               b, h_hr[b], w_hr[b]);
  }
  return AS_OK;
}

}  // namespace

extern "C" {

int64_t as_train_queries_ws_bytes(const int* h_hr, const int* w_hr, int B, int mode) {
  AS_REQUIRE(known_mode(mode), AS_ERR_BAD_ARG, "train_queries_ws_bytes: unknown mode %d", mode);
  const int rc = check_sizes("train_queries_ws_bytes", h_hr, w_hr, B);
  if (rc != AS_OK) return rc;
  if (!sparse_mode(mode)) return 0;
  int64_t ints = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = (int64_t)h_hr[b] * w_hr[b];
    ints += n + as::cdiv64(n, kTile);
  }
  return 4 * ints;
}

int as_train_queries(const float* const* crops, const int* h_hr, const int* w_hr, int B, int Q, int mode, uint64_t seed,
                     float* hr_coord, float* hr_disp, int* index, int* n_valid, const float* scale, float* scale_out, void* ws,
                     int64_t ws_bytes, void* stream) {
  AS_REQUIRE(crops && hr_coord && hr_disp && index && n_valid, AS_ERR_BAD_ARG, "train_queries: null pointer");
  AS_REQUIRE(scale || !scale_out, AS_ERR_BAD_ARG, "train_queries: scale_out without scale");
  AS_REQUIRE(known_mode(mode), AS_ERR_BAD_ARG, "train_queries: unknown mode %d", mode);
  const int rc = check_sizes("train_queries", h_hr, w_hr, B);
  if (rc != AS_OK) return rc;
  AS_REQUIRE(Q > 0, AS_ERR_BAD_ARG, "train_queries: non-positive Q=%d", Q);
  AS_REQUIRE(reinterpret_cast<uintptr_t>(hr_coord) % 8 == 0, AS_ERR_BAD_ARG, "train_queries: hr_coord is not 8-byte aligned");
  AS_REQUIRE((int64_t)B * Q * 2 <= 2147483647ll, AS_ERR_BAD_SHAPE, "train_queries: more than 2^31-1 output elements");
  for (int b = 0; b < B; ++b) {
    AS_REQUIRE(crops[b], AS_ERR_BAD_ARG, "train_queries: sample %d: null crop pointer", b);
    AS_REQUIRE(!scale || (isfinite(scale[b]) && scale[b] > 0.f), AS_ERR_BAD_ARG,
               "train_queries: sample %d: scale %g is not finite and positive", b, (double)scale[b]);
    const int64_t n = (int64_t)h_hr[b] * w_hr[b];
    if (mode == AS_TQ_DENSE_ALL)
      AS_REQUIRE(n == Q, AS_ERR_BAD_SHAPE, "train_queries: sample %d: dense_all needs Q == N, got Q=%d, N=%lld", b, Q, (long long)n);
    else
      AS_REQUIRE(n >= Q, AS_ERR_BAD_SHAPE, "train_queries: sample %d: Q=%d distinct queries from N=%lld pixels", b, Q, (long long)n);
  }
  const bool sparse = sparse_mode(mode);
  if (sparse) {
    const int64_t need = as_train_queries_ws_bytes(h_hr, w_hr, B, mode);
    AS_REQUIRE(ws, AS_ERR_BAD_ARG, "train_queries: null workspace (the sparse modes need %lld bytes)", (long long)need);
    AS_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 4 == 0, AS_ERR_BAD_ARG, "train_queries: workspace is not 4-byte aligned");
    AS_REQUIRE(ws_bytes >= need, AS_ERR_BAD_ARG, "train_queries: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
               (long long)need);
  }
  hipStream_t s = as::as_stream(stream);
  int* wsp = static_cast<int*>(ws);
  for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
    const int nb = B - b0 < kMaxBatch ? B - b0 : kMaxBatch;
    Table t = {};
    int max_tiles = 0;
    for (int i = 0; i < nb; ++i) {
      Sample& e = t.s[i];
      const int b = b0 + i;
      e.crop = crops[b];
      e.h = h_hr[b];
      e.w = w_hr[b];
      e.n = e.h * e.w;
      e.tiles = (int)as::cdiv64(e.n, kTile);
      const as::CoordAxis ah = as::coord_axis(e.h), aw = as::coord_axis(e.w);  // make_coord (stereo_datasets.py:27-28)
      e.c0h = ah.c0; e.steph = ah.s; e.c0w = aw.c0; e.stepw = aw.s;
      derive_keys(seed, b, mode, e.key);
      e.scale = scale ? scale[b] : 0.f;
      if (sparse) {
        e.list = wsp;
        e.tile_off = wsp + e.n;
        wsp += (int64_t)e.n + e.tiles;
        if (e.tiles > max_tiles) max_tiles = e.tiles;
      }
    }
    int* nv = n_valid + b0;
    if (sparse) {
      hipLaunchKernelGGL(count_kernel, dim3(max_tiles, nb), dim3(kThreads), 0, s, t);
      hipLaunchKernelGGL(scan_kernel, dim3(nb), dim3(kThreads), 0, s, t, nv);
      hipLaunchKernelGGL(scatter_kernel, dim3(max_tiles, nb), dim3(kThreads), 0, s, t, (const int*)nv);
    }
    hipLaunchKernelGGL(queries_kernel, dim3(as::cdiv(Q, kThreads), nb), dim3(kThreads), 0, s, t, Q, mode, hr_coord + (int64_t)b0 * Q * 2,
                       hr_disp + (int64_t)b0 * Q, index + (int64_t)b0 * Q, nv, scale_out ? scale_out + b0 : nullptr);
    const int lrc = as::check_launch("train_queries");
    if (lrc != AS_OK) return lrc;
  }
  return AS_OK;
}

int as_low_disp(const float* const* crops, const int* h_hr, const int* w_hr, const float* scale, float* out, int B, int h_out,
                int w_out, void* stream) {
  AS_REQUIRE(crops && scale && out, AS_ERR_BAD_ARG, "low_disp: null pointer");
  const int rc = check_sizes("low_disp", h_hr, w_hr, B);
  if (rc != AS_OK) return rc;
  AS_REQUIRE(h_out > 0 && w_out > 0, AS_ERR_BAD_ARG, "low_disp: non-positive output size %dx%d", h_out, w_out);
  for (int b = 0; b < B; ++b) {
    AS_REQUIRE(crops[b], AS_ERR_BAD_ARG, "low_disp: sample %d: null crop pointer", b);
    AS_REQUIRE(isfinite(scale[b]) && scale[b] > 0.f, AS_ERR_BAD_ARG, "low_disp: sample %d: scale %g is not finite and positive", b,
               (double)scale[b]);
  }
  AS_REQUIRE((int64_t)B * h_out * w_out <= 2147483647ll, AS_ERR_BAD_SHAPE, "low_disp: more than 2^31-1 output elements");
  const int64_t gy = as::cdiv64(h_out, kTileY);
  AS_REQUIRE(gy <= 65535, AS_ERR_BAD_SHAPE, "low_disp: h_out=%d above %d", h_out, 65535 * kTileY);
  hipStream_t s = as::as_stream(stream);
  for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
    const int nb = B - b0 < kMaxBatch ? B - b0 : kMaxBatch;
    LowTable t = {};
    for (int i = 0; i < nb; ++i) {
      LowSample& e = t.s[i];
      const int b = b0 + i;
      e.crop = crops[b];
      e.h = h_hr[b];
      e.w = w_hr[b];
      e.ratio_h = (float)e.h / (float)h_out;
      e.ratio_w = (float)e.w / (float)w_out;
      e.div = 4.f * scale[b];
    }
    hipLaunchKernelGGL(low_disp_kernel, dim3((unsigned)as::cdiv64(w_out, kTileX), (unsigned)gy, nb), dim3(kThreads), 0, s, t,
                       out + (int64_t)b0 * h_out * w_out, h_out, w_out);
    const int lrc = as::check_launch("low_disp");
    if (lrc != AS_OK) return lrc;
  }
  return AS_OK;
}

}  // extern "C"
