// Streaming 1x1 convolution in split precision for the memory-bound pointwise layers of the pre-loop (MobileNetV2 expand /
// project, shortcuts, heads, the FeatureAtt gate, the 1x1x1 aggregation): few channels on large maps, where conv_split_kernel's
// LDS-staged 64-channel K unit, 64 | 128-channel tile padding and 8-wave, >= 100 KB blocks are all overhead.
//
// Same arithmetic as conv_split_kernel<1, ...> with the LINEAR epilogue, different data movement — results are bit-identical:
//   * operands: x = hi + lo/2048, hi = fp16(x) under MODE.FP16_OVFL, lo = fp16((x - hi) * 2048), split by the same expressions;
//   * per 16-channel chunk, ascending: acc_h += a_hi b_hi, acc_x += a_hi b_lo, acc_x += a_lo b_hi (v_mfma_f32_32x32x16_f16), with the
//     same fragment layout (lane l: channels 8 (l >> 5) .. +7 of output channel / pixel column l & 31), so every dot product sums
//     its 16 k in the same hardware order; zero chunks (padding) add exact zeros and are skipped or not, freely;
//   * epilogue: v = acc_h + acc_x / 2048, x = v + bias + add, o = act(x), with a residual h: o = max(o + h, 0).
// A dot product's value does not depend on WHICH column of the 32x32 tile holds its pixel, so the pixel <-> column map is free:
//
// A wave owns a run of 64 pixels of one batch element as TWO MFMA pixel tiles, lane column r <-> pixels 2r (tile 0) and 2r + 1
// (tile 1) of the run: a lane's operand loads, epilogue loads and result stores are 8-B accesses of two neighbouring pixels,
// 256-B runs per channel and half-wave.  Activations go from fp32 NCHW through range-checked buffer loads straight into B
// fragments (no LDS); A fragments are 16-B reads of the PackedConv split pack [chunk][comp][h][Cout_pad][8].
// Planes whose pixel pairs are not 8-B aligned (odd plane size, odd base) take dword accesses.
//
// Two register orientations, both with ascending K per accumulator:
//   RESIDENT  (pointwise_resident_kernel<NCH, OPS>):  all activation fragments of the run stay in registers (NCH chunks,
//             Cin <= 128); the block (4 waves) parks the weights and the bias in LDS once and every wave sweeps the 32-channel
//             output tiles, two accumulator pairs live at a time.  Every source plane is read once.
//   KSWEEP    (pointwise_ksweep_kernel<NT, OPS>):     the accumulators of all NT <= 2 output tiles (Cout <= 64) stay in registers;
//             the wave sweeps K in groups of four chunks (weights through L1 / L2), the next group's loads in flight under the
//             current one's MFMAs.
// OPS: the layer has an `add` tensor or a residual (pw_epilogue).  No block waits on another; the grid is a function of the shape.
#include "common.h"
#include "conv_plan.h"
#include "split.h"

namespace {

using namespace as;  // split.h: the arithmetic conv_split_kernel compiles too, which is why the two agree bit for bit

constexpr int kPwRun = 64;          // pixels per wave
constexpr int kPwWaves = 2;         // waves per block of the KSWEEP kernels
constexpr int kPwResWaves = 4;      // ... of the RESIDENT kernels (they share the weights' LDS image)
constexpr int kPwMaxLds = 80 * 1024; // RESIDENT: weights + bias image
constexpr int kPwMaxResident = 8;   // chunks the RESIDENT orientation holds (Cin <= 128)
constexpr int kPwMaxSweepCout = 64; // output channels the KSWEEP orientation accumulates
constexpr int kPwMaxPlane = 1 << 24;
constexpr unsigned kOOB = 0x7FFFFFF0u;

struct PwParams {
  const float* src[AS_MAX_SRCS];
  int src_c[AS_MAX_SRCS];
  int src_end[AS_MAX_SRCS];  // exclusive prefix end of each source's channel range
  int n_src;
  const _Float16* wpack;
  long long wpack_bytes;
  const float* bias;
  const float* add;
  int add_ctot, add_coff;
  const float* h;
  float* out;
  int out_ctot, out_coff;
  int B, Cin, Cout, Cout_pad, act;
  int plane;    // H * W
  int runs;     // blocks per batch element
  int chunks;   // 16-channel K chunks that hold channels
  int ctiles;   // 32-channel output tiles that hold channels
  int vec;      // 8-B accesses: even plane, every tensor 8-B aligned
};

__device__ unsigned g_split_overflow_pw;  // as_pointwise_split_overflow

// The two pixels of a lane in one channel plane.  o0 / o1: byte offsets of the pixels inside the descriptor's window, or kOOB.
template <bool VEC>
__device__ __forceinline__ void pw_load2(__amdgpu_buffer_rsrc_t r, unsigned o0, unsigned o1, float& a, float& b) {
  if constexpr (VEC) {  // o1 == o0 + 4, both in range or both out
    const f32x2 v = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)o0, 0, 0));  // cast the whole 8 bytes
    a = v[0];
    b = v[1];
  } else {
    a = bload(r, o0);
    b = bload(r, o1);
  }
}

// Raw fp32 operands of chunk k: v[q][j] = channel 16 k + 8 hf + j of the lane's pixel q.  Channels past the source's end
// (the padding of the last chunk; whole chunks past Cin) are outside the descriptor's range and read 0.
template <bool VEC>
__device__ __forceinline__ void pw_load_chunk(const PwParams& p, int b, int k, int hf, unsigned p0, unsigned p1, float (&v)[2][8]) {
  const int cb = k * kSplitKC;
  const float* sp = p.src[0];
  int sc = p.src_c[0], sb = 0;
  if (p.n_src > 1 && cb >= p.src_end[0]) { sp = p.src[1]; sc = p.src_c[1]; sb = p.src_end[0]; }
  if (p.n_src > 2 && cb >= p.src_end[1]) { sp = p.src[2]; sc = p.src_c[2]; sb = p.src_end[1]; }
  if (p.n_src > 3 && cb >= p.src_end[2]) { sp = p.src[3]; sc = p.src_c[3]; sb = p.src_end[2]; }
  const int left = sc - (cb - sb);  // channels of the source from this chunk on
  const float* spb = sp + ((long long)b * sc + (left > 0 ? cb - sb : 0)) * p.plane;
  const int recs = left > 0 ? (int)((long long)left * p.plane * 4) : 0;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)spb, 0, recs, 0x00020000);
  const unsigned pl4 = (unsigned)p.plane * 4u;
  // one per-lane base per pixel + a uniform channel step: kOOB + 15 planes stays below 2^32 (plane <= 2^24) and outside every window
  const unsigned b0 = p0 + (unsigned)(8 * hf) * pl4, b1 = p1 + (unsigned)(8 * hf) * pl4;
#pragma unroll
  for (int j = 0; j < 8; ++j) pw_load2<VEC>(rs, b0 + (unsigned)j * pl4, b1 + (unsigned)j * pl4, v[0][j], v[1][j]);
}

// A fragments of (chunk k, output tile ct): rows ct * 32 + r of the hi and of the lo image; chunks past the pack read 0
__device__ __forceinline__ void pw_load_a(const PwParams& p, __amdgpu_buffer_rsrc_t rw, int k, int ct, int r, int hf, half8& a_hi, half8& a_lo) {
  const unsigned row = (unsigned)(ct * 32 + r) * 16u;
  const unsigned seg = (unsigned)p.Cout_pad * 16u;  // bytes of one (chunk, comp, h) segment
  const unsigned o = (unsigned)(k * 4 + hf) * seg + row;
  a_hi = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rw, (int)o, 0, 0));
  a_lo = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(o + 2u * seg), 0, 0));
}

#define PW_MFMA(acc, a, b) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0)
// the three products of one chunk on the two pixel tiles, in conv_split_kernel's order per accumulator
#define PW_CHUNK(AH, AX, a_hi, a_lo, BH, BL)          \
  PW_MFMA(AH[0], a_hi, BH[0]);                        \
  PW_MFMA(AX[0], a_hi, BL[0]);                        \
  PW_MFMA(AH[1], a_hi, BH[1]);                        \
  PW_MFMA(AX[1], a_hi, BL[1]);                        \
  PW_MFMA(AX[0], a_lo, BH[0]);                        \
  PW_MFMA(AX[1], a_lo, BH[1]);

struct PwEpi {
  __amdgpu_buffer_rsrc_t r_out, r_add, r_h, r_bias;
  unsigned pl4;
};

__device__ __forceinline__ PwEpi pw_make_epi(const PwParams& p, int b) {
  PwEpi e;
  const long long plane = p.plane;
  const int recs = (int)((long long)p.Cout * plane * 4);
  float* outp = p.out + ((long long)b * p.out_ctot + p.out_coff) * plane;
  e.r_out = __builtin_amdgcn_make_buffer_rsrc((void*)outp, 0, recs, 0x00020000);
  const float* addp = p.add ? p.add + ((long long)b * p.add_ctot + p.add_coff) * plane : outp;
  e.r_add = __builtin_amdgcn_make_buffer_rsrc((void*)addp, 0, p.add ? recs : 0, 0x00020000);
  const float* hp = p.h ? p.h + (long long)b * p.Cout * plane : outp;
  e.r_h = __builtin_amdgcn_make_buffer_rsrc((void*)hp, 0, p.h ? recs : 0, 0x00020000);
  e.r_bias = __builtin_amdgcn_make_buffer_rsrc((void*)(p.bias ? (const void*)p.bias : (const void*)outp), 0, p.bias ? p.Cout * 4 : 0, 0x00020000);
  e.pl4 = (unsigned)plane * 4u;
  return e;
}

// The bias of the lane's 16 channels of output tile ct (0 without one; 0 past Cout).  Issued before the tile's MFMAs, the loads
// cost the epilogue no round trip.
__device__ __forceinline__ void pw_load_bias(const PwEpi& e, int ct, int hf, float (&bs)[16]) {
  const unsigned bb = (unsigned)(ct * 32 + 4 * hf) * 4u;
#pragma unroll
  for (int row = 0; row < 16; ++row) bs[row] = bload(e.r_bias, bb + (unsigned)((row & 3) + 8 * (row >> 2)) * 4u);
}

// epi_finish<AS_EPI_LINEAR> of conv.hip on output tile ct: the lane's 16 channels x 2 pixels.
// OPS: the layer has an `add` tensor or a residual `h`.  Their loads are a variant of their own because a load in the epilogue
// makes every later use wait for the memory counter, which also counts the result stores still in flight: without operands the
// stores of a tile sweep are fire and forget.  With operands, all loads of the tile go out together, before its first store.
template <bool VEC, bool OPS>
__device__ __forceinline__ void pw_epilogue(const PwParams& p, const PwEpi& e, int ct, int hf, const f32x16 (&ah)[2], const f32x16 (&ax)[2],
                                            const float (&bs)[16], unsigned p0, unsigned p1) {
  // Offsets = a per-lane base per pixel + a uniform row step.  No select: a channel >= Cout lies past the windows' Cout planes,
  // a pixel past the plane starts from kOOB, and neither sum wraps (ceil32(Cout) planes stay below 0x7FFFFFF0: pw_reject).
  const unsigned cb = (unsigned)(ct * 32 + 4 * hf);
  const unsigned b0 = p0 + cb * e.pl4, b1 = p1 + cb * e.pl4;
  float av[2][16], hv[2][16];
#pragma unroll
  for (int row = 0; row < 16; ++row) {
    av[0][row] = av[1][row] = hv[0][row] = hv[1][row] = 0.f;
    if constexpr (OPS) {
      const unsigned o0 = b0 + (unsigned)((row & 3) + 8 * (row >> 2)) * e.pl4, o1 = b1 + (unsigned)((row & 3) + 8 * (row >> 2)) * e.pl4;
      if (p.add) pw_load2<VEC>(e.r_add, o0, o1, av[0][row], av[1][row]);
      if (p.h) pw_load2<VEC>(e.r_h, o0, o1, hv[0][row], hv[1][row]);
    }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {  // rounds of 4 accumulator rows
    float x[2][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = g * 4 + i;
      const float v0 = join(ah[0][row], ax[0][row]);
      const float v1 = join(ah[1][row], ax[1][row]);
      x[0][i] = v0 + bs[row] + av[0][row];
      x[1][i] = v1 + bs[row] + av[1][row];
    }
    // the activation code is uniform: ONE switch per round, not one per element (a lone wave per SIMD pays every scalar
    // branch in full); each case is act_apply with a constant code — the same functions on the same values
#define PW_ACT_ROUND(CODE)                                                        \
  case CODE:                                                                      \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                \
      x[0][i] = act_apply(x[0][i], CODE);                                         \
      x[1][i] = act_apply(x[1][i], CODE);                                         \
    }                                                                             \
    break;
    switch (p.act) {
      PW_ACT_ROUND(AS_ACT_RELU)
      PW_ACT_ROUND(AS_ACT_SIGMOID)
      PW_ACT_ROUND(AS_ACT_TANH)
      PW_ACT_ROUND(AS_ACT_RELU6)
      PW_ACT_ROUND(AS_ACT_LEAKY)
      default: break;
    }
#undef PW_ACT_ROUND
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = g * 4 + i;
      const unsigned o0 = b0 + (unsigned)((row & 3) + 8 * (row >> 2)) * e.pl4, o1 = b1 + (unsigned)((row & 3) + 8 * (row >> 2)) * e.pl4;
      float o0v = x[0][i], o1v = x[1][i];
      if (OPS && p.h) {
        o0v = fmaxf(o0v + hv[0][row], 0.f);
        o1v = fmaxf(o1v + hv[1][row], 0.f);
      }
      if constexpr (VEC) {
        f32x2 w;
        w[0] = o0v;
        w[1] = o1v;
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, w), e.r_out, (int)o0, 0, 0);
      } else {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o0v), e.r_out, (int)o0, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o1v), e.r_out, (int)o1, 0, 0);
      }
    }
  }
}

// the wave's place: batch element, first pixel, the lane's two pixel offsets (bytes inside a plane, or kOOB).  `idle`: the
// whole run lies past the plane (the last block of a batch element); wave-uniform.
#define PW_PLACE                                                                                       \
  const int lane = threadIdx.x & 63;                                                                   \
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                                   \
  const int r = lane & 31, hf = lane >> 5;                                                             \
  const int b = blockIdx.x / p.runs;                                                                   \
  const int px0 = (blockIdx.x - b * p.runs) * (int)blockDim.x + wave * kPwRun;                         \
  const bool idle = px0 >= p.plane;                                                                    \
  const int pix = px0 + 2 * r;                                                                         \
  const unsigned p0 = pix < p.plane ? (unsigned)pix * 4u : kOOB;                                       \
  const unsigned p1 = pix + 1 < p.plane ? (unsigned)(pix + 1) * 4u : kOOB;                             \
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.wpack, 0, (int)p.wpack_bytes, 0x00020000);

// RESIDENT.  The block (4 waves, 256 pixels) parks the layer's weights — NCH chunks of the pack, in the pack's order, zeros past
// it — and the bias in LDS once, so the tile sweep issues no global load: a load behind a tile's result stores would wait for
// them (one memory counter, in order), ~4 us per tile where the stores alone are fire and forget.
template <int NCH, bool VEC, bool OPS>
__device__ __forceinline__ void pw_resident(const PwParams& p, unsigned char* lds) {
  PW_PLACE
  float amax = 0.f;
  half8 bh[NCH][2], bl[NCH][2];
  float v[NCH][2][8];
#pragma unroll
  for (int k = 0; k < NCH; ++k) pw_load_chunk<VEC>(p, b, k, hf, p0, p1, v[k]);  // every plane of the run in flight at once
  const unsigned seg = (unsigned)p.Cout_pad * 16u;  // bytes of one (chunk, comp, h) segment
  const unsigned wbytes = (unsigned)NCH * 4u * seg;
  {
    constexpr unsigned STEP = kPwResWaves * 64 * 16;
    for (unsigned o = threadIdx.x * 16u; o < wbytes; o += 4 * STEP) {
      u32x4 w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(o + i * STEP), 0, 0));
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (o + i * STEP < wbytes) *reinterpret_cast<u32x4*>(lds + o + i * STEP) = w[i];
    }
    float* bias_w = reinterpret_cast<float*>(lds + wbytes);
    for (int c = threadIdx.x; c < p.Cout_pad; c += kPwResWaves * 64) bias_w[c] = (p.bias && c < p.Cout) ? p.bias[c] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    split_mode8(v[k][0], bh[k][0], bl[k][0]);
    amax = amax8(v[k][0], amax);
    split_mode8(v[k][1], bh[k][1], bl[k][1]);
    amax = amax8(v[k][1], amax);
  }
  __syncthreads();
  if (idle) return;
  const float* bias_s = reinterpret_cast<const float*>(lds + wbytes);
  const PwEpi e = pw_make_epi(p, b);
#pragma unroll 1
  for (int ct = 0; ct < p.ctiles; ++ct) {
    const unsigned char* wa = lds + (unsigned)hf * seg + (unsigned)(ct * 32 + r) * 16u;
    half8 a_hi[NCH], a_lo[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      a_hi[k] = *reinterpret_cast<const half8*>(wa + (unsigned)(k * 4) * seg);
      a_lo[k] = *reinterpret_cast<const half8*>(wa + (unsigned)(k * 4 + 2) * seg);
    }
    float bs[16];
#pragma unroll
    for (int row = 0; row < 16; ++row) bs[row] = bias_s[ct * 32 + 4 * hf + (row & 3) + 8 * (row >> 2)];
    f32x16 ah[2], ax[2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int i = 0; i < 16; ++i) ah[q][i] = ax[q][i] = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      PW_CHUNK(ah, ax, a_hi[k], a_lo[k], bh[k], bl[k])
    }
    pw_epilogue<VEC, OPS>(p, e, ct, hf, ah, ax, bs, p0, p1);
  }
  as::note_split_overflow(amax, &g_split_overflow_pw);
}

// OPS (an `add` tensor or a residual): kernels of their own, so that the common form keeps its registers and occupancy
template <int NCH, bool OPS>
__global__ __launch_bounds__(kPwResWaves * 64, ((NCH <= 4 && !OPS) ? 2 : 1)) void pointwise_resident_kernel(PwParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pw_lds[];
  as::fp16_saturate_mode();
  if (p.vec) pw_resident<NCH, true, OPS>(p, pw_lds);
  else pw_resident<NCH, false, OPS>(p, pw_lds);
}

template <int NT, bool VEC, bool OPS>
__device__ __forceinline__ void pw_ksweep(const PwParams& p) {
  constexpr int G = 4;  // chunks per group
  PW_PLACE
  if (idle) return;  // no barrier in this kernel
  float amax = 0.f;
  f32x16 ah[NT][2], ax[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int i = 0; i < 16; ++i) ah[t][q][i] = ax[t][q][i] = 0.f;
  float cur[G][2][8];
#pragma unroll
  for (int g = 0; g < G; ++g) pw_load_chunk<VEC>(p, b, g, hf, p0, p1, cur[g]);
  const int groups = (p.chunks + G - 1) / G;
#pragma unroll 1
  for (int gi = 0; gi < groups; ++gi) {
    const int k0 = gi * G;
    float nxt[G][2][8];  // the next group (past Cin: zero records, no traffic)
#pragma unroll
    for (int g = 0; g < G; ++g) pw_load_chunk<VEC>(p, b, k0 + G + g, hf, p0, p1, nxt[g]);
    half8 a_hi[NT][G], a_lo[NT][G];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int g = 0; g < G; ++g) pw_load_a(p, rw, k0 + g, t, r, hf, a_hi[t][g], a_lo[t][g]);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      half8 bh[2], bl[2];
      split_mode8(cur[g][0], bh[0], bl[0]);
      amax = amax8(cur[g][0], amax);
      split_mode8(cur[g][1], bh[1], bl[1]);
      amax = amax8(cur[g][1], amax);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        PW_CHUNK(ah[t], ax[t], a_hi[t][g], a_lo[t][g], bh, bl)
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < 8; ++j) cur[g][q][j] = nxt[g][q][j];
  }
  const PwEpi e = pw_make_epi(p, b);
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < p.ctiles) {
      float bs[16];
      pw_load_bias(e, t, hf, bs);
      pw_epilogue<VEC, OPS>(p, e, t, hf, ah[t], ax[t], bs, p0, p1);
    }
  as::note_split_overflow(amax, &g_split_overflow_pw);
}

template <int NT, bool OPS>
__global__ __launch_bounds__(kPwRun * kPwWaves) void pointwise_ksweep_kernel(PwParams p) {
  as::fp16_saturate_mode();
  if (p.vec) pw_ksweep<NT, true, OPS>(p);
  else pw_ksweep<NT, false, OPS>(p);
}

#undef PW_PLACE
#undef PW_CHUNK
#undef PW_MFMA

// The orientation a shape runs in.  RESIDENT where the activations fit the registers (nch resident chunks: the instantiated
// count at or above the layer's) and the weights' LDS image fits; KSWEEP where the accumulators fit; by shape, the accumulators
// stay where they are few and K is long (the project layers).  AS_PW_ORIENT (A/B knob): 1 = RESIDENT, 2 = KSWEEP wherever legal.
struct PwPick {
  bool ok, sweep;
  int nch, lds;
};

int pw_orient_knob() {
  static const int v = getenv("AS_PW_ORIENT") ? atoi(getenv("AS_PW_ORIENT")) : 0;
  return v;
}

PwPick pw_pick(int Cin, int Cout) {
  PwPick k{};
  const int chunks = (Cin + kSplitKC - 1) / kSplitKC;
  k.nch = chunks <= 4 ? chunks : chunks <= 6 ? 6 : 8;
  k.lds = k.nch * 4 * conv_cout_pad(Cout) * 16 + conv_cout_pad(Cout) * 4;
  const bool can_res = chunks <= kPwMaxResident && k.lds <= kPwMaxLds, can_sweep = Cout <= kPwMaxSweepCout;
  k.sweep = can_sweep && (!can_res || chunks > 4);
  if (pw_orient_knob() == 1 && can_res) k.sweep = false;
  if (pw_orient_knob() == 2 && can_sweep) k.sweep = true;
  k.ok = can_res || can_sweep;
  return k;
}

// Why the descriptor cannot take the streaming kernel, or nullptr.  The descriptor has passed as_conv2d's validation and
// `pl` is its plan.
const char* pw_reject(const as_conv_desc& d, const as_conv_plan& pl) {
  if (d.precision != 1) return "precision is not split";
  if (d.KS != 1) return "not a 1x1 convolution";
  if (!(d.stride == 0 || d.stride == 1)) return "stride is not 1";
  if (d.epilogue != AS_EPI_LINEAR) return "epilogue is not AS_EPI_LINEAR";
  if (d.dual) return "dual launch";
  if (d.out_bs || d.bs_only) return "blocked result";
  for (int i = 0; i < d.n_src; ++i)
    if (d.src_bs[i]) return "blocked source";
  if (as::fast16_mode()) return "fast16 is on";
  for (int i = 0; i + 1 < d.n_src; ++i)
    if (d.src_c[i] % kSplitKC) return "a source but the last does not hold a multiple of 16 channels";
  if (pl.ksplit != 1) return "as_conv2d splits K for this descriptor";
  const long long plane = (long long)d.H * d.W;
  if (plane > kPwMaxPlane) return "plane above 2^24 pixels";
  if (!pw_pick(d.Cin, d.Cout).ok) return "Cout above 64 with Cin above 128 or a weight image above 80 KB";
  if ((long long)((d.Cout + 31) / 32 * 32) * plane * 4 >= 0x7FFFFFF0ll) return "result exceeds 2 GiB per batch element";
  if ((long long)d.B * conv_cdiv(plane, kPwRun * kPwWaves) >= 2147483647ll) return "grid too large";
  return nullptr;
}

template <typename K>
int pw_launch(K kernel, PwParams& p, int waves, int lds, hipStream_t s) {
  p.runs = (int)conv_cdiv(p.plane, kPwRun * waves);
  if (lds > 64 * 1024) as::lds_opt_in(reinterpret_cast<const void*>(kernel));
  hipLaunchKernelGGL(kernel, dim3((unsigned)((long long)p.B * p.runs)), dim3(kPwRun * waves), lds, s, p);
  return as::check_launch("conv1x1_stream");
}

}  // namespace

extern "C" {

int as_conv1x1_stream_ok(const as_conv_desc* d) {
  as_conv_plan pl;
  if (as_conv2d_plan(d, nullptr, &pl) != AS_OK) return 0;
  return pw_reject(*d, pl) == nullptr ? 1 : 0;
}

int as_conv1x1_stream(const as_conv_desc* d, void* stream) {
  as_conv_plan pl;
  const int rc = as_conv2d_plan(d, nullptr, &pl);  // as_conv2d's argument checks, codes and messages
  if (rc != AS_OK) return rc;
  if (const char* why = pw_reject(*d, pl)) return as::fail(AS_ERR_BAD_ARG, "conv1x1_stream: %s (as_conv1x1_stream_ok)", why);
  PwParams p{};
  int csum = 0;
  bool vec = true;
  for (int i = 0; i < d->n_src; ++i) {
    p.src[i] = d->src[i];
    p.src_c[i] = d->src_c[i];
    csum += d->src_c[i];
    p.src_end[i] = csum;
    vec = vec && (reinterpret_cast<uintptr_t>(d->src[i]) & 7) == 0;
  }
  p.n_src = d->n_src;
  p.wpack = reinterpret_cast<const _Float16*>(d->wpack);
  p.wpack_bytes = as_conv_pack_size_split(d->Cin, d->Cout, 1) * 2;
  p.bias = d->bias;
  p.add = d->add; p.add_ctot = d->add_ctot; p.add_coff = d->add_coff;
  p.h = d->h;
  p.out = d->out;
  p.out_ctot = d->out_ctot > 0 ? d->out_ctot : d->Cout;
  p.out_coff = d->out_coff;
  p.B = d->B; p.Cin = d->Cin; p.Cout = d->Cout; p.Cout_pad = conv_cout_pad(d->Cout); p.act = d->act;
  p.plane = d->H * d->W;
  p.chunks = (d->Cin + kSplitKC - 1) / kSplitKC;
  p.ctiles = (d->Cout + 31) / 32;
  vec = vec && (p.plane & 1) == 0 && (reinterpret_cast<uintptr_t>(d->out) & 7) == 0 &&
        (reinterpret_cast<uintptr_t>(d->add) & 7) == 0 && (reinterpret_cast<uintptr_t>(d->h) & 7) == 0;
  p.vec = vec ? 1 : 0;
  hipStream_t s = as::as_stream(stream);
  const PwPick k = pw_pick(d->Cin, d->Cout);
  const bool ops = d->add || d->h;
#define PW_GO(KERNEL, WAVES, LDS) (ops ? pw_launch(KERNEL, true>, p, WAVES, LDS, s) : pw_launch(KERNEL, false>, p, WAVES, LDS, s))
  if (k.sweep) return p.ctiles == 1 ? PW_GO(pointwise_ksweep_kernel<1, kPwWaves, 0) : PW_GO(pointwise_ksweep_kernel<2, kPwWaves, 0);
  switch (k.nch) {
    case 1: return PW_GO(pointwise_resident_kernel<1, kPwResWaves, k.lds);
    case 2: return PW_GO(pointwise_resident_kernel<2, kPwResWaves, k.lds);
    case 3: return PW_GO(pointwise_resident_kernel<3, kPwResWaves, k.lds);
    case 4: return PW_GO(pointwise_resident_kernel<4, kPwResWaves, k.lds);
    case 6: return PW_GO(pointwise_resident_kernel<6, kPwResWaves, k.lds);
    default: return PW_GO(pointwise_resident_kernel<8, kPwResWaves, k.lds);
  }
#undef PW_GO
}

unsigned as_pointwise_split_overflow(int reset) { return as::read_reset_counter(&g_split_overflow_pw, reset); }

}  // extern "C"
