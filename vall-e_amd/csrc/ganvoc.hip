// HiFi-GAN / BigVGAN generator behind the C ABI (include/vallex.h, vx_gan_*): the packing of its weight table (weights_host.hpp)
// for the row GEMM, the anti-aliasing filter, the staging of a ragged call (CallStage, host.hpp), the five row buffers and the
// launches of ganvoc_kernels.hpp.  A translation unit and a handle of its own, like vocoder.hip: no other unit sees these kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>

#undef VX_STAMPS  // the in-kernel stamps write device globals of engine.hip's unit, out of this unit's reach
#include "ganvoc_kernels.hpp"
#include "weights_host.hpp"

using namespace vx;

namespace {

// One row GEMM: the packed weight [N][K] and bias [N] as offsets into the device block, and the gather rule.
struct GanConv {
  size_t w = 0, b = 0;
  bool has_bias = false;
  int C = 0, taps = 0, off0 = 0, step = 1, N = 0;
};
struct GanAct {
  size_t a = 0, invb = 0;
};
struct GanResblock {
  GanConv c1[4], c2[4];
  GanAct a1[4], a2[4];
};
struct GanStage {
  GanConv up;
  GanResblock rb[4];
};

struct GanDev {
  DevBuf<float> w;   // every packed tensor
  DevBuf<float> ws;  // five row buffers of `cap` floats each
  size_t cap = 0;
  // per call: logmel pointers | wav pointers [max_batch each] | segment tables [2 max_batch + 1 ints]
  CallStage stage;
};

constexpr long GAN_GROUP_FLOATS = 1L << 24;  // target size of a row buffer: groups of whole utterances are cut to fit it

}  // namespace

struct vx_gan : LazyDev<GanDev> {
  vx_gan_config cfg{};
  std::map<std::string, HostW> w;
  bool finalized = false;
  float filt[GAN_AA_TAPS] = {};
  int hop = 1;
  long widest = 0;  // floats per frame of the widest row buffer
  // filled by vx_gan_finalize
  std::vector<float> packed;
  GanConv pre, post;
  GanAct act_post;
  GanStage st[8];
  size_t mean = 0, scale = 0;
  bool has_norm = false;
};

namespace {

// I0 by its power series (fp64; the terms fall below 1e-17 of the sum long before 64 of them at beta ~ 6.5)
double bessel_i0(double x) {
  double sum = 1.0, term = 1.0;
  for (int k = 1; k < 64; ++k) {
    term *= (x / (2.0 * k)) * (x / (2.0 * k));
    sum += term;
  }
  return sum;
}

void kaiser_sinc12(float* out) {
  const int K = GAN_AA_TAPS;
  const double pi = 3.14159265358979323846, cutoff = 0.25, half_width = 0.3;
  const double delta_f = 4.0 * half_width, A = 2.285 * (K / 2 - 1) * pi * delta_f + 7.95;
  const double beta = A > 50.0 ? 0.1102 * (A - 8.7) : (A >= 21.0 ? 0.5842 * pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0) : 0.0);
  double f[GAN_AA_TAPS], sum = 0.0;
  for (int n = 0; n < K; ++n) {
    const double r = 2.0 * n / (K - 1) - 1.0;  // the symmetric (periodic = False) window
    const double w = bessel_i0(beta * sqrt(std::max(0.0, 1.0 - r * r))) / bessel_i0(beta);
    const double t = (double)n - K / 2 + 0.5, x = 2.0 * cutoff * t;
    f[n] = 2.0 * cutoff * w * (x == 0.0 ? 1.0 : sin(pi * x) / (pi * x));
    sum += f[n];
  }
  for (int n = 0; n < K; ++n) out[n] = (float)(f[n] / sum);
}

// Conv1d (O, C, k), dilation d, "same" zero padding: W[o][j * C + c] = w[o][c][j]; tap j reads row t + (j - (k-1)/2) d.
GanConv pack_conv(vx_gan* g, const std::string& name, int O, int Cc, int k, int d) {
  GanConv cv;
  cv.w = push(g->packed, conv_rows(g->w[name + ".weight"].data.data(), O, Cc, k));
  const HostW& b = g->w[name + ".bias"];
  cv.has_bias = b.set;
  if (b.set) cv.b = push(g->packed, b.data);
  cv.C = Cc; cv.taps = k; cv.off0 = -((k - 1) / 2) * d; cv.step = d; cv.N = O;
  return cv;
}

// ConvTranspose1d (Cin, Cout, k), stride u, padding p = (k - u) / 2.  Output sample t u + r takes x[t - q] W[.][.][q u + r + p] for
// every q with 0 <= q u + r + p < k; over the phases r that is q in [qlo, qhi].  Tap i of the GEMM is q = qhi - i (source row
// t - qhi + i), row n = r * Cout + co, zeros where a phase has no such tap.
GanConv pack_convtr(vx_gan* g, const std::string& name, int Cin, int Cout, int k, int u) {
  const HostW& w = g->w[name + ".weight"];
  const int p = (k - u) / 2;
  int qlo = 0, qhi = 0;
  for (int r = 0; r < u; ++r)
    for (int j = 0; j < k; ++j) {
      const int num = j - r - p;  // = q u
      if (num % u != 0) continue;
      qlo = std::min(qlo, num / u);
      qhi = std::max(qhi, num / u);
    }
  const int taps = qhi - qlo + 1;
  std::vector<float> pk((size_t)u * Cout * taps * Cin, 0.f);
  for (int r = 0; r < u; ++r)
    for (int co = 0; co < Cout; ++co)
      for (int i = 0; i < taps; ++i) {
        const int j = (qhi - i) * u + r + p;
        if (j < 0 || j >= k) continue;
        for (int ci = 0; ci < Cin; ++ci)
          pk[(((size_t)r * Cout + co) * taps + i) * Cin + ci] = w.data[((size_t)ci * Cout + co) * k + j];
      }
  GanConv cv;
  cv.w = push(g->packed, pk);
  const HostW& b = g->w[name + ".bias"];
  std::vector<float> bb((size_t)u * Cout);
  for (int r = 0; r < u; ++r)
    for (int co = 0; co < Cout; ++co) bb[(size_t)r * Cout + co] = b.data[co];
  cv.b = push(g->packed, bb);
  cv.has_bias = true;
  cv.C = Cin; cv.taps = taps; cv.off0 = -qhi; cv.step = 1; cv.N = u * Cout;
  return cv;
}

GanAct pack_act(vx_gan* g, const std::string& name, int Cc) {
  const vx_gan_config& c = g->cfg;
  const HostW& al = g->w[name + ".alpha"];
  const HostW& be = c.activation == VX_GAN_SNAKEBETA ? g->w[name + ".beta"] : al;
  std::vector<float> a(Cc), ib(Cc);
  for (int i = 0; i < Cc; ++i) {
    const double av = c.alpha_logscale ? exp((double)al.data[i]) : (double)al.data[i];
    const double bv = c.alpha_logscale ? exp((double)be.data[i]) : (double)be.data[i];
    a[i] = (float)av;
    ib[i] = (float)(1.0 / (bv + 1e-9));
  }
  GanAct r;
  r.a = push(g->packed, a);
  r.invb = push(g->packed, ib);
  return r;
}

int launch_gemm(const GanGemmArgs& a, hipStream_t s) {
  if (a.M <= 0) return VX_OK;
  const bool vec = a.C % 16 == 0;
  if (a.N <= 32) {
    dim3 g((unsigned)((a.M + 127) / 128), (unsigned)((a.N + 31) / 32));
    if (vec) gan_gemm_rows<4, 1, true><<<g, 256, 0, s>>>(a);
    else gan_gemm_rows<4, 1, false><<<g, 256, 0, s>>>(a);
  } else {
    dim3 g((unsigned)((a.M + 63) / 64), (unsigned)((a.N + 63) / 64));
    if (vec) gan_gemm_rows<2, 2, true><<<g, 256, 0, s>>>(a);
    else gan_gemm_rows<2, 2, false><<<g, 256, 0, s>>>(a);
  }
  HIPC(hipGetLastError());
  return VX_OK;
}

// One group of whole utterances: `frames` rows at rate 1, segment table `seg` (device, nseg + 1 frame offsets from the group's start).
struct GroupCtx {
  const vx_gan* g;
  const float* W;
  float* buf[5];
  const int* seg;
  int nseg;
  long frames;
  hipStream_t s;
};

int run_conv(const GroupCtx& x, const GanConv& cv, const float* in, float* out, int rate, bool lrelu, float slope,
             const float* res = nullptr, float* sum = nullptr, int acc = GAN_ACC_NONE, float div = 0.f) {
  GanGemmArgs a{};
  a.x = in; a.C = cv.C; a.taps = cv.taps; a.off0 = cv.off0; a.step = cv.step;
  a.lrelu = lrelu ? 1 : 0; a.slope = slope;
  a.W = x.W + cv.w; a.bias = cv.has_bias ? x.W + cv.b : nullptr;
  a.res = res; a.out = out; a.sum = sum; a.acc = acc; a.div = div;
  a.M = x.frames * rate; a.N = cv.N; a.K = cv.taps * cv.C;
  a.seg = x.seg; a.nseg = x.nseg; a.rate = rate;
  return launch_gemm(a, x.s);
}

int run_act(const GroupCtx& x, const GanAct& ac, const float* in, float* out, int Cc, int rate) {
  GanActArgs a{};
  a.x = in; a.y = out; a.a = x.W + ac.a; a.invb = x.W + ac.invb;
  a.M = x.frames * rate; a.C = Cc; a.seg = x.seg; a.nseg = x.nseg; a.rate = rate;
  memcpy(a.f, x.g->filt, sizeof(a.f));
  dim3 grid((unsigned)((a.M + GAN_AA_TT - 1) / GAN_AA_TT + x.nseg), (unsigned)((Cc + GAN_AA_CC - 1) / GAN_AA_CC));
  gan_aa_act<<<grid, 256, 0, x.s>>>(a);
  HIPC(hipGetLastError());
  return VX_OK;
}

int run_group(const GroupCtx& x, const float* const* in_ptrs, float* const* out_ptrs) {
  const vx_gan* g = x.g;
  const vx_gan_config& c = g->cfg;
  const bool lrelu = c.activation == VX_GAN_LRELU;
  float *xu = x.buf[0], *x1 = x.buf[1], *A = x.buf[2], *B = x.buf[3], *sum = x.buf[4];
  const long n_in = x.frames * c.n_mels;
  gan_pack_rows<<<(unsigned)((n_in + 255) / 256), 256, 0, x.s>>>(in_ptrs, A, g->has_norm ? x.W + g->mean : nullptr,
                                                                g->has_norm ? x.W + g->scale : nullptr, x.frames, c.n_mels, x.seg,
                                                                x.nseg);
  HIPC(hipGetLastError());
  VXC(run_conv(x, g->pre, A, sum, 1, false, 0.f));
  int rate = 1, Cc = c.initial_channels;
  for (int i = 0; i < c.n_stages; ++i) {
    const GanStage& st = g->st[i];
    VXC(run_conv(x, st.up, sum, xu, rate, lrelu, c.lrelu_slope));  // [rows][u C/2] = [rows u][C/2]
    rate *= c.rates[i];
    Cc /= 2;
    for (int r = 0; r < c.n_resblocks; ++r) {
      const GanResblock& rb = st.rb[r];
      const float* cur = xu;
      for (int m = 0; m < c.n_dilations; ++m) {
        const float* t = cur;
        if (!lrelu) { VXC(run_act(x, rb.a1[m], cur, A, Cc, rate)); t = A; }
        VXC(run_conv(x, rb.c1[m], t, B, rate, lrelu, c.lrelu_slope));
        t = B;
        if (!lrelu) { VXC(run_act(x, rb.a2[m], B, A, Cc, rate)); t = A; }
        if (m + 1 < c.n_dilations) {
          VXC(run_conv(x, rb.c2[m], t, x1, rate, lrelu, c.lrelu_slope, cur));
          cur = x1;
        } else {  // the block's result goes into the stage sum
          VXC(run_conv(x, rb.c2[m], t, nullptr, rate, lrelu, c.lrelu_slope, cur, sum, r == 0 ? GAN_ACC_FIRST : GAN_ACC_ADD,
                       r + 1 == c.n_resblocks ? (float)c.n_resblocks : 0.f));
        }
      }
    }
  }
  const float* last = sum;
  if (!lrelu) { VXC(run_act(x, g->act_post, sum, A, Cc, rate)); last = A; }
  const long M = x.frames * rate;
  gan_conv_post<<<(unsigned)((M + 255) / 256), 256, 0, x.s>>>(last, x.W + g->post.w, g->post.has_bias ? x.W + g->post.b : nullptr,
                                                              out_ptrs, M, Cc, 7, lrelu ? 1 : 0, 0.01f, x.seg, x.nseg, rate);
  HIPC(hipGetLastError());
  return VX_OK;
}

int gan_init_device(vx_gan* g) {
  VXC(open_device(g));
  GanDev& d = *g->dev;
  const size_t MB = (size_t)g->cfg.max_batch;
  VXC(d.w.alloc(g->packed.size() + 4));
  HIPC(hipMemcpy(d.w.get(), g->packed.data(), g->packed.size() * sizeof(float), hipMemcpyHostToDevice));
  VXC(d.stage.init(2 * MB * sizeof(void*) + (2 * MB + 1) * sizeof(int)));
  return VX_OK;
}

}  // namespace

extern "C" int64_t vx_gan_samples(const vx_gan* g, int64_t n_frames) { return (!g || n_frames < 0) ? 0 : n_frames * g->hop; }

extern "C" int vx_gan_create(const vx_gan_config* cfg, vx_gan** out) {
  VXC(create_head("vx_gan_create", cfg, out));
  const vx_gan_config& c = *cfg;
  if (c.max_batch < 1) return fail(VX_ERR_ARG, "vx_gan_create: max_batch = %d", c.max_batch);
  if (c.max_total_frames < 1) return fail(VX_ERR_ARG, "vx_gan_create: max_total_frames = %d", c.max_total_frames);
  if (c.n_mels < 1) return fail(VX_ERR_ARG, "vx_gan_create: n_mels = %d", c.n_mels);
  if (c.n_stages < 1 || c.n_stages > 8) return fail(VX_ERR_ARG, "vx_gan_create: n_stages = %d outside [1, 8]", c.n_stages);
  if (c.n_resblocks < 1 || c.n_resblocks > 4) return fail(VX_ERR_ARG, "vx_gan_create: n_resblocks = %d outside [1, 4]", c.n_resblocks);
  if (c.n_dilations < 1 || c.n_dilations > 4) return fail(VX_ERR_ARG, "vx_gan_create: n_dilations = %d outside [1, 4]", c.n_dilations);
  for (int i = 0; i < c.n_stages; ++i)
    if (c.rates[i] < 1 || c.kernels[i] < 1)
      return fail(VX_ERR_ARG, "vx_gan_create: stage %d: rate %d, kernel %d", i, c.rates[i], c.kernels[i]);
  for (int r = 0; r < c.n_resblocks; ++r) {
    if (c.resblock_kernels[r] < 1) return fail(VX_ERR_ARG, "vx_gan_create: resblock kernel %d = %d", r, c.resblock_kernels[r]);
    for (int m = 0; m < c.n_dilations; ++m)
      if (c.dilations[r][m] < 1) return fail(VX_ERR_ARG, "vx_gan_create: dilation [%d][%d] = %d", r, m, c.dilations[r][m]);
  }
  if (c.initial_channels < 1) return fail(VX_ERR_ARG, "vx_gan_create: initial_channels = %d", c.initial_channels);
  if (c.activation < VX_GAN_LRELU || c.activation > VX_GAN_SNAKEBETA)
    return fail(VX_ERR_ARG, "vx_gan_create: activation = %d", c.activation);
  if (c.alpha_logscale != 0 && c.alpha_logscale != 1) return fail(VX_ERR_ARG, "vx_gan_create: alpha_logscale = %d", c.alpha_logscale);
  if (!isfinite(c.lrelu_slope)) return fail(VX_ERR_ARG, "vx_gan_create: lrelu_slope = %g", c.lrelu_slope);
  long hop = 1;
  for (int i = 0; i < c.n_stages; ++i) {
    if (c.kernels[i] < c.rates[i] || (c.kernels[i] - c.rates[i]) % 2 != 0)
      return fail(VX_ERR_UNSUPPORTED, "vx_gan_create: stage %d: kernel %d with rate %d (k >= u and k - u even is served: the "
                  "symmetric padding (k - u) / 2)", i, c.kernels[i], c.rates[i]);
    hop = std::min(hop * c.rates[i], 1L << 20);
  }
  for (int r = 0; r < c.n_resblocks; ++r)
    if (c.resblock_kernels[r] % 2 == 0)
      return fail(VX_ERR_UNSUPPORTED, "vx_gan_create: resblock kernel %d = %d is even", r, c.resblock_kernels[r]);
  if (c.initial_channels % (1 << c.n_stages) != 0)
    return fail(VX_ERR_UNSUPPORTED, "vx_gan_create: initial_channels = %d is no multiple of 2^%d", c.initial_channels, c.n_stages);
  if (hop > 4096) return fail(VX_ERR_UNSUPPORTED, "vx_gan_create: the rates multiply to more than 4096 samples per frame");
  if (c.max_batch > GAN_MAX_SEG) return fail(VX_ERR_UNSUPPORTED, "vx_gan_create: max_batch = %d > %d", c.max_batch, GAN_MAX_SEG);
  if (c.max_total_frames > (1 << 21))
    return fail(VX_ERR_UNSUPPORTED, "vx_gan_create: max_total_frames = %d > %d", c.max_total_frames, 1 << 21);

  std::unique_ptr<vx_gan> g(new vx_gan());
  g->cfg = c;
  g->hop = (int)hop;
  kaiser_sinc12(g->filt);
  const bool snake = c.activation != VX_GAN_LRELU, hasb = c.activation == VX_GAN_SNAKEBETA;
  add_key(g.get(), "conv_pre.weight", {c.initial_channels, c.n_mels, 7});
  add_key(g.get(), "conv_pre.bias", {c.initial_channels});
  int Cc = c.initial_channels;
  long rate = 1, widest = std::max(c.n_mels, c.initial_channels);
  for (int i = 0; i < c.n_stages; ++i) {
    const std::string up = "ups." + std::to_string(i);
    add_key(g.get(), up + ".weight", {Cc, Cc / 2, c.kernels[i]});
    add_key(g.get(), up + ".bias", {Cc / 2});
    Cc /= 2;
    rate *= c.rates[i];
    widest = std::max(widest, rate * Cc);
    for (int r = 0; r < c.n_resblocks; ++r) {
      const std::string rb = "resblocks." + std::to_string(i * c.n_resblocks + r);
      for (int m = 0; m < c.n_dilations; ++m)
        for (const char* cv : {".convs1.", ".convs2."}) {
          add_key(g.get(), rb + cv + std::to_string(m) + ".weight", {Cc, Cc, c.resblock_kernels[r]});
          add_key(g.get(), rb + cv + std::to_string(m) + ".bias", {Cc});
        }
      if (snake)
        for (int a = 0; a < 2 * c.n_dilations; ++a) {
          add_key(g.get(), rb + ".activations." + std::to_string(a) + ".alpha", {Cc});
          if (hasb) add_key(g.get(), rb + ".activations." + std::to_string(a) + ".beta", {Cc});
        }
    }
  }
  if (snake) {
    add_key(g.get(), "activation_post.alpha", {Cc});
    if (hasb) add_key(g.get(), "activation_post.beta", {Cc});
  }
  add_key(g.get(), "conv_post.weight", {1, Cc, 7});
  add_key(g.get(), "conv_post.bias", {1}, true);
  add_key(g.get(), "mean", {c.n_mels}, true);
  add_key(g.get(), "scale", {c.n_mels}, true);
  g->widest = widest;
  *out = g.release();
  return VX_OK;
}

extern "C" void vx_gan_destroy(vx_gan* g) { destroy_handle(g); }

extern "C" int vx_gan_set_weight(vx_gan* g, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
  return set_weight(g, "vx_gan", key, data, shape, ndim);
}

extern "C" int vx_gan_set_filter(vx_gan* g, const float* taps, int32_t n_taps) {
  if (!g || !taps) return fail(VX_ERR_ARG, "vx_gan_set_filter: null argument");
  if (n_taps != GAN_AA_TAPS) return fail(VX_ERR_UNSUPPORTED, "vx_gan_set_filter: %d taps, %d are served", n_taps, GAN_AA_TAPS);
  if (g->finalized) return fail(VX_ERR_STATE, "vx_gan_set_filter after vx_gan_finalize");
  memcpy(g->filt, taps, sizeof(g->filt));
  return VX_OK;
}

extern "C" int vx_gan_get_filter(const vx_gan* g, float* taps) {
  if (!g || !taps) return fail(VX_ERR_ARG, "vx_gan_get_filter: null argument");
  memcpy(taps, g->filt, sizeof(g->filt));
  return VX_OK;
}

extern "C" int vx_gan_finalize(vx_gan* g) {
  if (!g) return fail(VX_ERR_ARG, "vx_gan_finalize: null handle");
  if (g->finalized) return VX_OK;
  VXC(missing_tensor(g));
  if (g->w["mean"].set != g->w["scale"].set)
    return fail(VX_ERR_WEIGHTS, "missing tensor %s (mean and scale come together)", g->w["mean"].set ? "scale" : "mean");
  const vx_gan_config& c = g->cfg;
  const bool snake = c.activation != VX_GAN_LRELU;
  g->packed.clear();
  g->pre = pack_conv(g, "conv_pre", c.initial_channels, c.n_mels, 7, 1);
  int Cc = c.initial_channels;
  for (int i = 0; i < c.n_stages; ++i) {
    GanStage& st = g->st[i];
    st.up = pack_convtr(g, "ups." + std::to_string(i), Cc, Cc / 2, c.kernels[i], c.rates[i]);
    Cc /= 2;
    for (int r = 0; r < c.n_resblocks; ++r) {
      const std::string rb = "resblocks." + std::to_string(i * c.n_resblocks + r);
      for (int m = 0; m < c.n_dilations; ++m) {
        st.rb[r].c1[m] = pack_conv(g, rb + ".convs1." + std::to_string(m), Cc, Cc, c.resblock_kernels[r], c.dilations[r][m]);
        st.rb[r].c2[m] = pack_conv(g, rb + ".convs2." + std::to_string(m), Cc, Cc, c.resblock_kernels[r], 1);
        if (snake) {
          st.rb[r].a1[m] = pack_act(g, rb + ".activations." + std::to_string(2 * m), Cc);
          st.rb[r].a2[m] = pack_act(g, rb + ".activations." + std::to_string(2 * m + 1), Cc);
        }
      }
    }
  }
  if (snake) g->act_post = pack_act(g, "activation_post", Cc);
  g->post = pack_conv(g, "conv_post", 1, Cc, 7, 1);
  g->has_norm = g->w["mean"].set;
  if (g->has_norm) {
    g->mean = push(g->packed, g->w["mean"].data);
    g->scale = push(g->packed, g->w["scale"].data);
  }
  for (auto& kv : g->w) std::vector<float>().swap(kv.second.data);  // the packed copy is the one that is kept
  g->finalized = true;
  return VX_OK;
}

extern "C" int vx_gan_synthesize(vx_gan* g, int32_t n, const float* const* logmel, const int32_t* n_frames, float* const* wav_out,
                                 void* stream) {
  if (!g || !logmel || !n_frames || !wav_out) return fail(VX_ERR_ARG, "vx_gan_synthesize: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_gan_synthesize: n = %d utterances", n);
  if (!g->finalized) return fail(VX_ERR_STATE, "vx_gan_synthesize before vx_gan_finalize");
  const vx_gan_config& c = g->cfg;
  if (n > c.max_batch) return fail(VX_ERR_CAPACITY, "vx_gan_synthesize: n = %d utterances > max_batch %d", n, c.max_batch);
  long total = 0;
  for (int i = 0; i < n; ++i) {
    const int T = n_frames[i];
    if (T < 0) return fail(VX_ERR_ARG, "vx_gan_synthesize: utterance %d: %d frames", i, T);
    if (T > 0 && (!logmel[i] || !wav_out[i])) return fail(VX_ERR_ARG, "vx_gan_synthesize: utterance %d: null pointer", i);
    total += T;
    if (total > c.max_total_frames)
      return fail(VX_ERR_CAPACITY, "vx_gan_synthesize: %ld frames up to utterance %d > max_total_frames %d", total, i,
                  c.max_total_frames);
  }
  if (total == 0) return VX_OK;  // no utterance has a frame: nothing to write
  // groups of whole utterances whose widest rows fit GAN_GROUP_FLOATS (an utterance that is longer goes alone)
  const long group_frames = std::max(1L, GAN_GROUP_FLOATS / g->widest);
  std::vector<int> first;  // first utterance of every group, and n at the end
  long need = 0;
  {
    long fr = 0;
    first.push_back(0);
    for (int i = 0; i < n; ++i) {
      if (fr > 0 && fr + n_frames[i] > group_frames) {
        first.push_back(i);
        fr = 0;
      }
      fr += n_frames[i];
      need = std::max(need, fr);
    }
    first.push_back(n);
  }
  VXC(ensure_device(g, gan_init_device));
  ON_DEVICE(g->device);
  GanDev& d = *g->dev;
  hipStream_t s = (hipStream_t)stream;
  const size_t cap = ((size_t)need * (size_t)g->widest + 3) / 4 * 4;
  if (cap > d.cap) {
    VXC(d.stage.drain());  // nothing uses the old workspace any more
    d.cap = 0;
    VXC(d.ws.alloc(5 * cap));
    d.cap = cap;
  }
  VXC(d.stage.begin(s));
  const size_t MB = (size_t)c.max_batch;
  const float** hin = d.stage.host<const float*>();
  float** hout = d.stage.host<float*>(MB * sizeof(void*));
  int* hseg = d.stage.host<int>(2 * MB * sizeof(void*));
  for (int i = 0; i < n; ++i) {
    hin[i] = logmel[i];
    hout[i] = wav_out[i];
  }
  std::vector<int> seg_at(first.size() - 1);
  int at = 0;
  for (size_t gi = 0; gi + 1 < first.size(); ++gi) {
    seg_at[gi] = at;
    int fr = 0;
    hseg[at++] = 0;
    for (int i = first[gi]; i < first[gi + 1]; ++i) hseg[at++] = (fr += n_frames[i]);
  }
  VXC(d.stage.upload(d.stage.bytes, s));
  for (size_t gi = 0; gi + 1 < first.size(); ++gi) {
    GroupCtx x{};
    x.g = g; x.W = d.w.get(); x.s = s;
    for (int b = 0; b < 5; ++b) x.buf[b] = d.ws.get() + (size_t)b * d.cap;
    x.seg = d.stage.dev<const int>(2 * MB * sizeof(void*)) + seg_at[gi];
    x.nseg = first[gi + 1] - first[gi];
    x.frames = hseg[seg_at[gi] + x.nseg];
    if (x.frames == 0) continue;
    VXC(run_group(x, d.stage.dev<const float* const>() + first[gi], d.stage.dev<float* const>(MB * sizeof(void*)) + first[gi]));
  }
  return d.stage.finish(s);
}
