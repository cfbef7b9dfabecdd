// The host-only half of as_conv2d: conv_validate (the argument checks: conditions, codes and messages in the order a caller
// meets them), conv_dual_second, and as_conv2d_plan — what as_conv2d launches for a descriptor, without a device.  as_conv2d
// (conv.hip) calls the same conv_validate and the same conv_plan (conv_plan.h), then launches the plan.
#include "common.h"
#include "conv_plan.h"

namespace as {

int conv_validate(const as_conv_desc* d) {
  AS_REQUIRE(d, AS_ERR_BAD_ARG, "conv2d: null descriptor");
  as_conv_desc first;
  if (d->dual) {
    AS_REQUIRE(d->n_src == 1 && d->epilogue == AS_EPI_LINEAR && !d->add && (d->stride == 0 || d->stride == 1), AS_ERR_BAD_ARG,
               "conv2d(dual): one source, LINEAR epilogue, no add, stride 1");
    AS_REQUIRE((d->h == nullptr) == (d->h2 == nullptr), AS_ERR_BAD_ARG, "conv2d(dual): a residual for both convolutions or for neither");
    AS_REQUIRE(!d->dual_act2 || (d->act2 >= AS_ACT_NONE && d->act2 <= AS_ACT_LEAKY), AS_ERR_BAD_ARG, "conv2d(dual): act2=%d", d->act2);
    AS_REQUIRE(!d->out_bs_b || (reinterpret_cast<uintptr_t>(d->out_bs_b) & 15) == 0, AS_ERR_BAD_ARG, "conv2d(dual): out_bs_b not 16-B aligned");
    AS_REQUIRE(!(d->out_b || d->out_bs_b) || ((d->out_b != nullptr) == (d->out != nullptr && !d->bs_only) && (d->out_bs_b != nullptr) == (d->out_bs != nullptr)),
               AS_ERR_BAD_ARG, "conv2d(dual): separate second outputs mirror the first convolution's (fp32 and / or blocked)");
    AS_REQUIRE(d->src2 && d->wpack2 && (reinterpret_cast<uintptr_t>(d->wpack2) & 15) == 0, AS_ERR_BAD_ARG, "conv2d(dual): null / misaligned src2 / wpack2");
    AS_REQUIRE(!d->src2_bs || (reinterpret_cast<uintptr_t>(d->src2) & 15) == 0, AS_ERR_BAD_ARG, "conv2d(dual): blocked src2 not 16-B aligned");
    AS_REQUIRE(d->out_coff2 >= 0 && d->out_bs_coff2 >= 0 && d->out_bs_coff2 % 8 == 0, AS_ERR_BAD_SHAPE, "conv2d(dual): bad second output window");
    if (d->precision != 1) {  // runs as two calls: the remaining checks are those of the first one
      first = *d;
      first.dual = 0;
      d = &first;
    }
  }
  AS_REQUIRE(d->KS == 1 || d->KS == 3, AS_ERR_BAD_ARG, "conv2d: KS=%d (supported: 1, 3)", d->KS);
  AS_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, AS_ERR_BAD_ARG, "conv2d: non-positive size");
  AS_REQUIRE(d->n_src >= 1 && d->n_src <= AS_MAX_SRCS, AS_ERR_BAD_ARG, "conv2d: n_src=%d", d->n_src);
  AS_REQUIRE(d->wpack, AS_ERR_BAD_ARG, "conv2d: null wpack");
  const bool bs_only = d->out_bs && d->bs_only;
  // the fp32 result may be omitted only where the blocked copy replaces it (LINEAR: out; GRU_ZR: out2)
  AS_REQUIRE(d->out || (bs_only && d->epilogue == AS_EPI_LINEAR), AS_ERR_BAD_ARG, "conv2d: null out");
  AS_REQUIRE((reinterpret_cast<uintptr_t>(d->wpack) & 15) == 0, AS_ERR_BAD_ARG, "conv2d: wpack not 16-B aligned");
  const bool stride1 = d->stride == 0 || d->stride == 1;  // 0 (zero-initialised descriptor) = 1
  int csum = 0;
  for (int i = 0; i < d->n_src; ++i) {
    AS_REQUIRE(d->src[i] && d->src_c[i] > 0, AS_ERR_BAD_ARG, "conv2d: source %d null or empty", i);
    csum += d->src_c[i];
    AS_REQUIRE(!d->src_bs[i] || (d->precision == 1 && stride1), AS_ERR_BAD_ARG,
               "conv2d: blocked split-fp16 sources need the split-precision kernel, stride 1");
    AS_REQUIRE(!d->src_bs[i] || (reinterpret_cast<uintptr_t>(d->src[i]) & 15) == 0, AS_ERR_BAD_ARG, "conv2d: blocked source %d not 16-B aligned", i);
  }
  if (d->out_bs) {
    AS_REQUIRE(d->precision == 1 && stride1, AS_ERR_BAD_ARG, "conv2d: out_bs needs the split-precision kernel, stride 1");
    AS_REQUIRE((reinterpret_cast<uintptr_t>(d->out_bs) & 15) == 0, AS_ERR_BAD_ARG, "conv2d: out_bs not 16-B aligned");
    const int cres = d->epilogue == AS_EPI_GRU_ZR ? d->Cout / 2 : d->Cout;
    const int ctot = d->out_bs_ctot > 0 ? d->out_bs_ctot : cres;
    AS_REQUIRE(d->out_bs_coff >= 0 && d->out_bs_coff % 8 == 0 && d->out_bs_coff + cres <= (ctot + 7) / 8 * 8, AS_ERR_BAD_SHAPE,
               "conv2d: out_bs channel window [%d,%d) must start at a multiple of 8 inside %d channels", d->out_bs_coff, d->out_bs_coff + cres, ctot);
    AS_REQUIRE(d->epilogue != AS_EPI_GRU_Q || !d->bs_only, AS_ERR_BAD_ARG, "conv2d(GRU_Q): the fp32 hidden state is always written");
  }
  AS_REQUIRE(csum == d->Cin, AS_ERR_BAD_SHAPE, "conv2d: sources hold %d channels, Cin=%d", csum, d->Cin);
  AS_REQUIRE(d->precision == 0 || d->precision == 1, AS_ERR_BAD_ARG, "conv2d: precision=%d", d->precision);
  const bool split = d->precision == 1;
  const int kc_req = split ? kSplitKC : conv_kc(d->KS);
  for (int i = 0; i + 1 < d->n_src; ++i)
    AS_REQUIRE(d->src_c[i] % kc_req == 0, AS_ERR_BAD_SHAPE,
               "conv2d: source %d has %d channels; every source but the last must hold a multiple of %d (concatenate first)",
               i, d->src_c[i], kc_req);
  AS_REQUIRE(!d->add || (d->add_coff >= 0 && d->add_coff + d->Cout <= d->add_ctot), AS_ERR_BAD_SHAPE, "conv2d: add channel window [%d,%d) outside %d", d->add_coff, d->add_coff + d->Cout, d->add_ctot);
  const int epi = d->epilogue;
  if (epi == AS_EPI_LINEAR) {
    const int out_ctot = d->out_ctot > 0 ? d->out_ctot : d->Cout;
    AS_REQUIRE(bs_only || (d->out_coff >= 0 && d->out_coff + d->Cout <= out_ctot), AS_ERR_BAD_SHAPE, "conv2d: out channel window outside out_ctot");
    AS_REQUIRE(!d->dual || bs_only || d->out_coff2 + d->Cout <= out_ctot, AS_ERR_BAD_SHAPE, "conv2d(dual): second out channel window outside out_ctot");
    AS_REQUIRE(d->act >= AS_ACT_NONE && d->act <= AS_ACT_LEAKY, AS_ERR_BAD_ARG, "conv2d: act=%d", d->act);
  } else if (epi == AS_EPI_GRU_ZR) {
    AS_REQUIRE(d->h && (d->out2 || bs_only) && (d->Cout % (2 * kBN)) == 0, AS_ERR_BAD_ARG, "conv2d(GRU_ZR): needs h, out2 and Cout %% 128 == 0");
  } else if (epi == AS_EPI_GRU_Q) {
    AS_REQUIRE(d->h && d->z, AS_ERR_BAD_ARG, "conv2d(GRU_Q): needs h and z");
  } else if (epi == AS_EPI_RELU_TAPS) {
    AS_REQUIRE(d->tap_w && d->out && !d->add && !d->h && !d->out_bs && !d->dual && d->precision == 1 && d->KS == 3 && stride1,
               AS_ERR_BAD_ARG, "conv2d(RELU_TAPS): needs tap_w and out; 3x3, split precision, stride 1, no add / residual / blocked copy / dual");
    AS_REQUIRE(d->act == AS_ACT_RELU, AS_ERR_BAD_ARG, "conv2d(RELU_TAPS): act must be AS_ACT_RELU");
  } else {
    return as::fail(AS_ERR_BAD_ARG, "conv2d: epilogue=%d", epi);
  }
  for (int i = 0; i < d->n_src; ++i)  // 32-bit buffer offsets inside one (batch, source) tensor
    AS_REQUIRE((long long)d->src_c[i] * d->H * d->W * 4 < 0x7FFFFFF0ll, AS_ERR_BAD_SHAPE,
               "conv2d: source %d exceeds 2 GiB per batch element", i);
  AS_REQUIRE(stride1 || (d->stride == 2 && split && d->KS == 3 && epi == AS_EPI_LINEAR), AS_ERR_BAD_ARG,
             "conv2d: stride=%d (stride 2: 3x3, split precision, LINEAR epilogue only)", d->stride);
  return AS_OK;
}

as_conv_desc conv_dual_second(const as_conv_desc& d) {
  as_conv_desc a = d;
  a.dual = 0;
  a.src[0] = d.src2; a.src_bs[0] = d.src2_bs; a.wpack = d.wpack2; a.bias = d.bias2;
  a.out_coff = d.out_coff2; a.out_bs_coff = d.out_bs_coff2;
  a.h = d.h2;
  if (d.dual_act2) a.act = d.act2;
  if (d.out_b || d.out_bs_b) {  // dense outputs of its own
    a.out = d.out_b; a.out_ctot = d.Cout; a.out_coff = 0;
    a.out_bs = d.out_bs_b; a.out_bs_ctot = d.Cout; a.out_bs_coff = 0;
    a.bs_only = (d.out_b == nullptr) ? 1 : 0;
  }
  a.h2 = nullptr; a.out_b = nullptr; a.out_bs_b = nullptr; a.dual_act2 = 0;
  return a;
}

}  // namespace as

extern "C" {

int as_conv2d_plan(const as_conv_desc* d, const as_conv_knobs* knobs, as_conv_plan* out) {
  AS_REQUIRE(out, AS_ERR_BAD_ARG, "conv2d_plan: null out");
  int rc = as::conv_validate(d);
  if (rc == AS_OK) rc = conv_plan(*d, knobs ? *knobs : conv_knobs(), as::fast16_mode(), out);
  if (rc == AS_OK && out->dual == kDualSequential) {  // as_conv2d checks the second call too before it launches the first
    const as_conv_desc second = as::conv_dual_second(*d);
    rc = as::conv_validate(&second);
  }
  if (rc == AS_OK && !as::conv_has_kernel(*out)) rc = conv_no_kernel(*out);
  return rc;
}

}  // extern "C"
