// The schedule of as_conv2d as a value: conv_plan() maps (descriptor, knobs) to the kernel instantiation, its grid and its
// schedule parameters.  Pure host arithmetic — no HIP call, no data pointer dereferenced — so the whole decision runs on a
// machine without a GPU (as_conv2d_plan in conv_plan.hip, tests/test_conv_plan_cpu.py).
// as_conv2d (conv.hip) is validate -> plan -> launch: conv_validate() (conv_plan.hip), conv_plan(), then the launch table keyed
// by the plan's tuple, with the plan's grid, block and LDS size.  Every scheduling rule, every constant it needs and the one
// reader of the AS_CONV_* knobs are in this file; tests/golden/conv_plans.json pins the plans, and the plan is what runs.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <initializer_list>

#include "../../include/anystereo_hip.h"

namespace as {

int fail(int code, const char* fmt, ...);  // as in common.h (conv.hip and conv_plan.hip include both: a mismatch does not compile)

// conv_plan.hip.  as_conv2d's argument checks, in the order a caller meets them: AS_OK, or the code with the message set
int conv_validate(const as_conv_desc* d);
// conv_plan.hip.  The second convolution of a dual launch as a call of its own
as_conv_desc conv_dual_second(const as_conv_desc& d);
// conv.hip, beside the launch table: the plan's tuple (family, KS, TW, BN, epilogue, NSUB, S, FAST, LEAN) has an entry
bool conv_has_kernel(const as_conv_plan& pl);

// The A/B knobs of the dispatch (README: AS_CONV_*), read from the environment at first use, process-wide.  An inline function
// with external linkage: the translation units that include this header share ONE `knobs` object, so the library reads the
// environment once however many of them ask.
inline const as_conv_knobs& conv_knobs() {
  static const as_conv_knobs knobs = [] {
    as_conv_knobs k = {/*lean*/ 1, /*xcd*/ 2, /*xcd_stagger*/ 0, /*lean_offset*/ 0, /*ksplit_max*/ 8,
                       /*dma*/ 1, /*wide*/ 1, /*wide64*/ 1, /*small_dma*/ 1, /*prefer64*/ 0};
    const struct { const char* name; int* v; } env[] = {
        {"AS_CONV_LEAN", &k.lean},  // 0 off | 1 the 256-pixel blocks of the big maps | 2 every 64-channel 3x3 launch | 3 = 1 + the 128-pixel blocks
        {"AS_CONV_XCD", &k.xcd},    // 0 off | 1 channel tiles together | 2 + banded pixel tiles
        {"AS_CONV_XCD_STAGGER", &k.xcd_stagger},
        {"AS_CONV_LEAN_OFFSET", &k.lean_offset},
        {"AS_CONV_KSPLIT_MAX", &k.ksplit_max},  // 1 = never split K
        {"AS_CONV_DMA", &k.dma},
        {"AS_CONV_WIDE", &k.wide},
        {"AS_CONV_WIDE64", &k.wide64},
        {"AS_CONV_SMALL_DMA", &k.small_dma},
        {"AS_CONV_PREFER64", &k.prefer64},
    };
    for (const auto& e : env)
      if (const char* s = getenv(e.name)) *e.v = atoi(s);
    return k;
  }();
  return knobs;
}

}  // namespace as

namespace {

using ConvKnobs = as_conv_knobs;
using ConvPlan = as_conv_plan;
using as::conv_knobs;

constexpr int kNumCU = 256;     // MI355X
constexpr int kEpiPartial = 3;  // internal epilogue: store the raw partial sums of a K slice into the workspace
constexpr int kBM = 64;         // conv_igemm_kernel: pixels per block
constexpr int kBN = 64;         // conv_igemm_kernel: output channels per block; the unit Cout is padded to
constexpr int kSplitKC = 16;    // conv_split_kernel: channels per K chunk
enum { kConvIgemm = 0, kConvSplit = 1 };
enum { kDualNone = 0, kDualFused = 1, kDualSequential = 2 };

constexpr int conv_kc(int KS) { return KS == 3 ? 8 : 32; }  // conv_igemm_kernel: channels per K chunk (ConvCfg<KS>::KC)
constexpr int conv_cout_pad(int Cout) { return ((Cout + kBN - 1) / kBN) * kBN; }
constexpr long long conv_cdiv(long long a, long long b) { return (a + b - 1) / b; }

// Dynamic LDS of conv_split_kernel<KS, TW, BN, *, NSUB, S, *, LEAN>: weight images + halo patch images of one K chunk.
constexpr int conv_split_lds(int KS, int TW, int BN, int NSUB, int S, bool LEAN) {
  const int TH = 128 / TW, patch = ((TH - 1) * S + KS) * ((TW - 1) * S + KS);
  const int NSC = (KS == 1) ? 4 : 1;
  const int wimg = KS * KS * NSC * 4 * BN * 16, pimg = NSC * (4 * NSUB * patch * 16);
  // LEAN: one weight + one patch image, and room for the epilogue's staging (bias / tap weights 4 KB + the fp32 tile)
  const int staging = 4096 + BN * 128 * NSUB * 4;
  if (LEAN) return wimg + pimg > staging ? wimg + pimg : staging;
  return 2 * wimg + ((KS == 3 && 2 * wimg + 2 * pimg <= 160 * 1024) ? 2 : 1) * pimg;  // the kernel's PDB rule
}

// Small feature maps give too few blocks to pull the weight stream (each CU fills its LDS at ~35 GB/s, so a 1/16-res GRU
// conv on 36 CUs is bound by 36 x that): K is split over more blocks, one block per CU (the tile's LDS footprint: more
// blocks than CUs would just queue a second round) and at most the 8 slices conv_finish_kernel sums.
// ks_max = AS_CONV_KSPLIT_MAX (A/B knob): alone a split launch is shorter; beside the other chain's kernels the unsplit one
// costs fewer CU-microseconds (no partial slabs, no finish launch) on half the CUs.
constexpr int conv_ksplit_cap(long long blocks, int ks_max) {
  int ks = (int)(kNumCU / blocks);
  if (ks > ks_max) ks = ks_max;
  return ks > 8 ? 8 : ks;
}
// ... as far as the K chunks (two per slice at least) and the descriptor's workspace (one [B][Cout_pad][H][W] slab per slice) go
inline int conv_pick_ksplit(const as_conv_desc& d, const ConvKnobs& k, const ConvPlan& pl, int cout_pad) {
  if (!d.ws || d.ws_elems <= 0) return 1;
  const long long slab = (long long)d.B * cout_pad * pl.H * pl.W;
  int ks = conv_ksplit_cap((long long)d.B * pl.tiles_x * pl.tiles_y * pl.n_tiles, k.ksplit_max);
  while (ks > 1 && (pl.chunks / ks < 2 || slab * ks > d.ws_elems)) --ks;
  return ks > 1 ? ks : 1;
}

inline int conv_plan(const as_conv_desc& d, const ConvKnobs& k, int fast16, ConvPlan* out);

// A dual launch that cannot be fused runs as two calls of the same shape (the first convolution, then conv_dual_second): the
// plan is the first one's.
inline int conv_plan_sequential(const as_conv_desc& d, const ConvKnobs& k, int fast16, ConvPlan* out) {
  as_conv_desc first = d;
  first.dual = 0;
  const int rc = conv_plan(first, k, fast16, out);
  out->dual = kDualSequential;
  return rc;
}

// The descriptor has passed as_conv2d's validation.  AS_OK, or AS_ERR_BAD_SHAPE for a plane or a grid past 2^31.
inline int conv_plan(const as_conv_desc& d, const ConvKnobs& k, int fast16, ConvPlan* out) {
  const bool split = d.precision == 1;
  if (d.dual && !split) return conv_plan_sequential(d, k, fast16, out);
  if ((long long)d.H * d.W >= 2147483647ll) return as::fail(AS_ERR_BAD_SHAPE, "conv2d: plane too large");
  const int cout_pad = conv_cout_pad(d.Cout);
  ConvPlan pl = {};
  pl.family = split ? kConvSplit : kConvIgemm;
  pl.KS = d.KS;
  pl.BN = kBN;
  pl.NSUB = 1;
  pl.S = d.stride == 2 ? 2 : 1;  // 0 (zero-initialised descriptor) = 1
  pl.epilogue = d.epilogue;
  pl.ksplit = 1;
  pl.H = pl.Hi = d.H;
  pl.W = pl.Wi = d.W;
  pl.n_tiles = cout_pad / kBN;
  pl.tiles_y = 1;

  if (!split) {
    pl.chunks = (d.Cin + conv_kc(d.KS) - 1) / conv_kc(d.KS);
    if (d.KS == 1) {  // no halo: run on the flattened H*W plane
      pl.H = pl.Hi = 1;
      pl.W = pl.Wi = d.H * d.W;
      pl.TW = kBM;
    } else {
      // the tile shape (TH x TW = 64 pixels) that wastes the fewest pixels on this image;
      // ties prefer 4x16 (64-B store runs, least halo) over 2x32 over 8x8
      long long best = -1;
      for (const int tw : {16, 32, 8}) {
        const int th = kBM / tw;
        const long long area = conv_cdiv(pl.W, tw) * tw * conv_cdiv(pl.H, th) * th;
        if (best < 0 || area < best) { best = area; pl.TW = tw; }
      }
      pl.tiles_y = (int)conv_cdiv(pl.H, kBM / pl.TW);
    }
    pl.tiles_x = (int)conv_cdiv(pl.W, pl.TW);
    pl.grid = (int64_t)d.B * pl.tiles_x * pl.tiles_y * pl.n_tiles;
    if (pl.grid >= 2147483647ll) return as::fail(AS_ERR_BAD_SHAPE, "conv2d: grid too large");
    pl.block = 256;
    *out = pl;
    return AS_OK;
  }

  // GRU_ZR: a channel tile lies inside one half of the channels (z | r), so 128-channel tiles need Cout / 2 % 128 == 0 as well
  const int bn = (cout_pad % 128 == 0 && !(d.epilogue == AS_EPI_GRU_ZR && d.Cout % 256 != 0)) ? 128 : 64;
  pl.chunks = (d.Cin + kSplitKC - 1) / kSplitKC;
  {
    bool all = true;
    for (int i = 0; i < d.n_src; ++i) all = all && d.src_bs[i];
    if (d.dual) all = all && d.src2_bs;
    pl.all_bs = (all && k.dma) ? 1 : 0;  // every source blocked: all-DMA operand staging where it fits
  }
  if (pl.S == 2) {
    // output plane (H-1)/2+1: 8x16 output tiles x 64 channels (the 17x33 halo patch leaves LDS room for one 64-wide weight image pair)
    pl.H = (d.H - 1) / 2 + 1;
    pl.W = (d.W - 1) / 2 + 1;
    pl.TW = 16;
  } else if (d.KS == 1) {
    pl.chunks = (pl.chunks + 3) / 4;  // pipeline units of four 16-channel chunks
    pl.H = pl.Hi = 1;
    pl.W = pl.Wi = d.H * d.W;
    pl.TW = 128;
    pl.BN = bn;
  } else {
    // 128-pixel tile as 8x16 or 4x32, whichever pads the image less (ties: 8x16, smaller halo)
    const long long a16 = conv_cdiv(pl.W, 16) * 16 * conv_cdiv(pl.H, 8) * 8;
    const long long a32 = conv_cdiv(pl.W, 32) * 32 * conv_cdiv(pl.H, 4) * 4;
    pl.TW = a32 < a16 ? 32 : 16;
    pl.BN = bn;
  }
  pl.n_tiles = cout_pad / pl.BN;
  pl.tiles_x = (int)conv_cdiv(pl.W, pl.TW);
  pl.tiles_y = (int)conv_cdiv(pl.H, 128 / pl.TW);
  if ((long long)d.B * pl.tiles_x * pl.tiles_y * pl.n_tiles >= 2147483647ll) return as::fail(AS_ERR_BAD_SHAPE, "conv2d: grid too large");

  if (pl.S == 1) {
    pl.ksplit = conv_pick_ksplit(d, k, pl, cout_pad);
    if (d.dual && pl.ksplit > 1) return conv_plan_sequential(d, k, fast16, out);
  }
  if (pl.S == 1 && d.KS == 3) {
    const long long pixel_tiles = (long long)pl.tiles_x * pl.tiles_y;
    const long long wide_blocks = (long long)d.B * conv_cdiv(pixel_tiles, 2) * (cout_pad / 64);
    if (d.epilogue == AS_EPI_RELU_TAPS) {  // 64-channel tiles, whole K per block (the reduction is over a tile's channels)
      pl.ksplit = 1;
      pl.BN = 64;
      pl.NSUB = wide_blocks >= 2 * kNumCU ? 2 : 1;
    } else {
      // big maps: 256-pixel x 64-channel blocks (two sub-tiles) pull 30 % fewer bytes per MFMA through the CU's L1
      const long long now_blocks = (long long)d.B * pixel_tiles * pl.n_tiles;
      bool wide_ok = bn == 128 ? conv_cdiv(wide_blocks, kNumCU) <= conv_cdiv(now_blocks, kNumCU)
                               : wide_blocks >= 2 * kNumCU;  // bn == 64: a wide block is twice the work of a current one
      // 64-channel layers below that bar (the encoder's convc2 || convd2 dual launch: 2 x 255 narrow blocks = two rounds, or 2 x 128
      // wide blocks = exactly one): rounds x (fixed cost + chunks x chunk time) from the block-lifetime stamps of both forms
      // (narrow: 6.8 us prologue + park + finish, 1.2 us per chunk; wide: 10.8 us, 2.3 us per chunk; tools/conv_stamps.py)
      if (!wide_ok && bn == 64 && k.wide64) {
        const int mult = d.dual ? 2 : 1;
        const double t_now = (double)conv_cdiv(now_blocks * mult, kNumCU) * (6.8 + 1.2 * pl.chunks);
        const double t_wide = (double)conv_cdiv(wide_blocks * mult, kNumCU) * (10.8 + 2.3 * pl.chunks);
        wide_ok = t_wide < t_now;
      }
      if (k.wide && pl.ksplit == 1 && wide_ok) {
        pl.BN = 64;
        pl.NSUB = 2;
      } else if (k.small_dma && pl.all_bs && bn == 128 && !d.dual) {
        // small maps with every source blocked: 64-channel tiles (two patch images fit next to their weight images -> all-DMA
        // staging) with K split over the blocks that leaves, instead of 128-channel tiles on the register-staged path
        pl.BN = 64;
        pl.n_tiles = cout_pad / 64;
        pl.ksplit = conv_pick_ksplit(d, k, pl, cout_pad);
      } else if (k.prefer64 && bn == 128 && !d.dual && pl.ksplit > 1 && (long long)d.B * pixel_tiles * (cout_pad / 64) <= kNumCU) {
        // A/B knob AS_CONV_PREFER64=1 (off by default: measured slower on the cfg-4 step, 53.6 vs 52.8 ms): fp32 sources, 64-channel
        // tiles when they need NO K split where the 128-channel tiles do — one fused launch instead of partial sums + a finish launch
        pl.BN = 64;
        pl.ksplit = 1;
      }
    }
    pl.n_tiles = cout_pad / pl.BN;
  }
  if (d.dual) {  // the second convolution rides in the same grid as a second set of channel tiles
    pl.dual = kDualFused;
    pl.n_tiles *= 2;
  }
  if (pl.ksplit > 1) {  // partial sums into the workspace, then conv_finish_kernel, one lane per element of its channel walk
    pl.epilogue = kEpiPartial;
    pl.finish = 1;
    pl.finish_epilogue = d.epilogue;
    const int cwalk = (d.out_bs && d.epilogue != AS_EPI_GRU_ZR) ? (d.Cout + 7) / 8 * 8 : d.Cout;
    pl.finish_grid = conv_cdiv((long long)d.B * cwalk * pl.H * pl.W, 256);
  }
  // the one-MFMA variant exists for the stride-1 3x3 convolutions (the GRU loop, the context net)
  pl.FAST = (fast16 && d.KS == 3 && pl.S == 1) ? 1 : 0;
  pl.grid = (int64_t)d.B * conv_cdiv((long long)pl.tiles_x * pl.tiles_y, pl.NSUB) * pl.n_tiles * pl.ksplit;
  // LEAN: two 4-wave blocks per CU instead of one 8-wave block when every source is blocked.
  // measured (cfg 2): with >= 2 blocks for every CU the pair overlaps one block's staging / prologue / epilogue with the
  // other's MFMAs (gru04 z|r 149.3 -> 146.6 us, head conv1 58.9 -> 54.4); with fewer blocks a CU holds ONE single-buffered
  // block and loses (gru04 q 85.5 -> 102.8, gru08 z|r 62 -> 87), as do 128-pixel lean blocks at three per CU (156.6 vs 144.4).
  // AS_CONV_LEAN=3 (A/B knob): mode 1 + the 128-pixel blocks of the small maps (49 KB: up to three per CU, co-resident with another
  // launch's blocks) — never the big maps' 256-block launches, which run alone and need their own double buffering
  pl.LEAN = (!pl.FAST && d.KS == 3 && pl.S == 1 && pl.BN == 64 && pl.all_bs &&
             (k.lean == 2 || ((k.lean == 1 || k.lean == 3) && pl.NSUB == 2 && pl.grid >= 2 * kNumCU) || (k.lean == 3 && pl.NSUB == 1)))
                ? 1 : 0;
  pl.xcd_map = k.xcd == 2 ? 2 : ((k.xcd && pl.n_tiles > 1) ? 1 : 0);  // 2: banded pixel tiles per XCD (any channel-tile count)
  pl.stagger = k.xcd_stagger;
  pl.lean_offset = k.lean_offset;
  pl.block = pl.LEAN ? 256 : 512;
  pl.lds = conv_split_lds(pl.KS, pl.TW, pl.BN, pl.NSUB, pl.S, pl.LEAN != 0);
  *out = pl;
  return AS_OK;
}

// the error of a plan whose tuple the launch table does not hold (as::conv_has_kernel)
inline int conv_no_kernel(const ConvPlan& pl) {
  return as::fail(AS_ERR_BAD_ARG, "conv2d: no kernel of family %d with <KS %d, TW %d, BN %d, epilogue %d, NSUB %d, S %d, FAST %d, LEAN %d>",
                  pl.family, pl.KS, pl.TW, pl.BN, pl.epilogue, pl.NSUB, pl.S, pl.FAST, pl.LEAN);
}

}  // namespace
