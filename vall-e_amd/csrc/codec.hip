// EnCodec-24 kHz decoder and encoder behind the C ABI (include/vallex.h, vx_codec_*): weights, workspace and the launch
// sequences of codec_kernels.hpp.  A handle of its own: the codec has its own weights and lifetime and runs without a VALL-E engine.
// At the end of the file: the sample-rate converter in front of the encoder (vx_resampler_*), a handle without weights, its ragged
// calls staged through CallStage (host.hpp); the codec handle keeps its own stream protocol (ev_in / ev_out / ev_copy).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "host.hpp"
#include "codec_kernels.hpp"

using namespace vx;

namespace {

struct HostW {
  std::vector<int64_t> shape;
  std::vector<float> v;
  bool set = false;
};

// ---- weight packing (host): torch layouts -> the [N][K] operands of codec_gemm_rows -------------------------------------
// conv (O, C, k): k index = tap * C + c, tap 0 = oldest sample
std::vector<float> pack_conv(const float* w, int O, int Cc, int k) {
  std::vector<float> p((size_t)O * Cc * k);
  for (int o = 0; o < O; ++o)
    for (int c = 0; c < Cc; ++c)
      for (int j = 0; j < k; ++j) p[((size_t)o * k + j) * Cc + c] = w[((size_t)o * Cc + c) * k + j];
  return p;
}
// transposed conv (Cin, Cout, 2s), stride s: row n = r * Cout + co; k < Cin: x[t-1] with W[ci][co][r + s]; then x[t] with W[ci][co][r]
std::vector<float> pack_convtr(const float* w, int Cin, int Cout, int s) {
  std::vector<float> p((size_t)s * Cout * 2 * Cin);
  for (int r = 0; r < s; ++r)
    for (int co = 0; co < Cout; ++co)
      for (int ci = 0; ci < Cin; ++ci) {
        const size_t n = (size_t)r * Cout + co;
        p[n * 2 * Cin + ci] = w[((size_t)ci * Cout + co) * 2 * s + r + s];
        p[n * 2 * Cin + Cin + ci] = w[((size_t)ci * Cout + co) * 2 * s + r];
      }
  return p;
}

int upload(const std::vector<float>& h, float** d) {
  HIPC(hipMalloc((void**)d, h.size() * sizeof(float) + 16));
  HIPC(hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  return VX_OK;
}

// ---- launches --------------------------------------------------------------------------------------------------------
int launch_gemm(CodecGemmArgs a, hipStream_t s) {
  bool vec = true;
  for (int p = 0; p < a.nparts; ++p) vec = vec && (a.part[p].C % 16 == 0);
  if (a.M <= 0) return VX_OK;
  if (a.N <= 32) {
    dim3 g((unsigned)((a.M + 127) / 128), (unsigned)((a.N + 31) / 32));
    if (vec) codec_gemm_rows<4, 1, true><<<g, 256, 0, s>>>(a);
    else codec_gemm_rows<4, 1, false><<<g, 256, 0, s>>>(a);
  } else {
    dim3 g((unsigned)((a.M + 63) / 64), (unsigned)((a.N + 63) / 64));
    if (vec) codec_gemm_rows<2, 2, true><<<g, 256, 0, s>>>(a);
    else codec_gemm_rows<2, 2, false><<<g, 256, 0, s>>>(a);
  }
  HIPC(hipGetLastError());
  return VX_OK;
}

// causal k-tap convolution over rows (reflect rule); wp packed by pack_conv.  c_out == 1 runs the bandwidth kernel.
int run_conv(const float* x, const float* wp, const float* bias, float* out, long M, int cin, int cout, int k, int elu,
             const int* seg, int nseg, int rate, hipStream_t s) {
  if (cout == 1 && elu) {
    if (M > 0) codec_conv_out<<<(unsigned)((M + 255) / 256), 256, 0, s>>>(x, wp, bias, out, M, cin, k, seg, nseg, rate);
    HIPC(hipGetLastError());
    return VX_OK;
  }
  CodecGemmArgs a{};
  a.part[0] = CodecPart{x, cin, k, CODEC_PAD_REFLECT, elu};
  a.nparts = 1;
  a.W = wp; a.bias = bias; a.out = out; a.M = M; a.N = cout; a.K = cin * k; a.seg = seg; a.nseg = nseg; a.rate = rate;
  return launch_gemm(a, s);
}

// transposed convolution k = 2 stride over M input rows -> M * stride output rows; wp / bias_rep packed ([stride * cout])
int run_convtr(const float* x, const float* wp, const float* bias_rep, float* out, long M, int cin, int cout, int stride, int elu,
               const int* seg, int nseg, int rate, hipStream_t s) {
  CodecGemmArgs a{};
  a.part[0] = CodecPart{x, cin, 2, CODEC_PAD_ZERO, elu};
  a.nparts = 1;
  a.W = wp; a.bias = bias_rep; a.out = out; a.M = M; a.N = stride * cout; a.K = 2 * cin; a.seg = seg; a.nseg = nseg; a.rate = rate;
  return launch_gemm(a, s);
}

// encoder: first convolution 1 -> cout over raw samples (seg: sample offsets, rate 1)
int run_conv_in(const float* x, const float* w, const float* bias, float* out, long M, int cout, int k, const int* seg, int nseg,
                hipStream_t s) {
  const long n = M * cout;
  if (n > 0) codec_conv_in<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(x, w, bias, out, M, cout, k, seg, nseg);
  HIPC(hipGetLastError());
  return VX_OK;
}

// encoder: strided convolution k = 2 stride; M_out output rows with starts seg_out, input rows' starts seg_in (both rate 1);
// wp packed by pack_conv
int run_conv_strided(const float* x, const float* wp, const float* bias, float* out, long M_out, int cin, int cout, int stride, int elu,
                     const int* seg_out, const int* seg_in, int nseg, hipStream_t s) {
  CodecGemmArgs a{};
  a.part[0] = CodecPart{x, cin, 2 * stride, CODEC_PAD_REFLECT, elu};
  a.nparts = 1;
  a.W = wp; a.bias = bias; a.out = out; a.M = M_out; a.N = cout; a.K = 2 * stride * cin; a.seg = seg_out; a.nseg = nseg; a.rate = 1;
  a.seg_in = seg_in; a.stride = stride;
  if (M_out <= 0) return VX_OK;
  const bool vec = cin % 16 == 0;
  if (a.N <= 32) {
    dim3 g((unsigned)((a.M + 127) / 128), (unsigned)((a.N + 31) / 32));
    if (vec) codec_gemm_rows<4, 1, true, true><<<g, 256, 0, s>>>(a);
    else codec_gemm_rows<4, 1, false, true><<<g, 256, 0, s>>>(a);
  } else {
    dim3 g((unsigned)((a.M + 63) / 64), (unsigned)((a.N + 63) / 64));
    if (vec) codec_gemm_rows<2, 2, true, true><<<g, 256, 0, s>>>(a);
    else codec_gemm_rows<2, 2, false, true><<<g, 256, 0, s>>>(a);
  }
  HIPC(hipGetLastError());
  return VX_OK;
}

bool rvq_shape_ok(int S, int D) { return S >= 32 && S % 32 == 0 && D >= 8 && D % 8 == 0 && D <= CODEC_RVQ_MAX_D; }

// |e_j|^2 in fp64, rounded once
std::vector<float> codebook_sq(const float* cb, size_t n, int D) {
  std::vector<float> o(n);
  for (size_t j = 0; j < n; ++j) {
    double a = 0;
    for (int c = 0; c < D; ++c) a += (double)cb[j * D + c] * cb[j * D + c];
    o[j] = (float)a;
  }
  return o;
}

int run_rvq_encode(const float* emb, const float* cb, const float* cb_sq, int* codes, long rows, int n_q, int S, int D, hipStream_t s) {
  if (rows > 0) codec_rvq_encode<<<(unsigned)((rows + CODEC_RVQ_ROWS - 1) / CODEC_RVQ_ROWS), 256, 0, s>>>(emb, cb, cb_sq, codes, rows, n_q, S, D);
  HIPC(hipGetLastError());
  return VX_OK;
}

struct LstmDev {
  float *wih0 = nullptr, *b0 = nullptr, *whh0 = nullptr, *w1 = nullptr, *b1 = nullptr;
};

bool lstm_width_ok(int H) { return H == 64 || H == 128 || H == 256 || H == 512; }

void launch_lstm_step(const CodecLstmArgs& a, int H, unsigned grid, int st, hipStream_t s) {
  switch (H) {
    case 64: codec_lstm_step<1><<<grid, 256, 0, s>>>(a, st); break;
    case 128: codec_lstm_step<2><<<grid, 256, 0, s>>>(a, st); break;
    case 256: codec_lstm_step<4><<<grid, 256, 0, s>>>(a, st); break;
    default: codec_lstm_step<8><<<grid, 256, 0, s>>>(a, st); break;
  }
}

constexpr int CODEC_LSTM_CHAIN = 64;  // step launches per replay of the captured chain

// x [rows][H] -> y = lstm(x) + x; gin [rows][4H], h0 / h1 [rows][H], c0 / c1 [nseg][H] are workspace.  chain == nullptr: one plain
// launch per step.  Otherwise the steps are replayed as a captured LINEAR chain of CODEC_LSTM_CHAIN step launches and one
// node that advances the step counter: `meta` (device {nseg, step}) was written by the caller, *chain is captured on first use
// (s must not be the null stream) and serves every batch and length of the handle.
int run_lstm(const LstmDev& w, const float* x, float* gin, float* h0, float* h1, float* c0, float* c1, float* y, int H, int layers,
             const int* seg_dev, const int* seg_host, int nseg, hipStream_t s, hipGraphExec_t* chain = nullptr, int* meta = nullptr) {
  const long rows = seg_host[nseg];
  int Tmax = 0;
  for (int b = 0; b < nseg; ++b) Tmax = std::max(Tmax, seg_host[b + 1] - seg_host[b]);
  CodecGemmArgs g{};
  g.part[0] = CodecPart{x, H, 1, CODEC_PAD_ZERO, 0};
  g.nparts = 1;
  g.W = w.wih0; g.bias = w.b0; g.out = gin; g.M = rows; g.N = 4 * H; g.K = H; g.seg = seg_dev; g.nseg = nseg; g.rate = 1;
  VXC(launch_gemm(g, s));
  CodecLstmArgs a{};
  a.gin0 = gin; a.whh0 = w.whh0; a.w1 = w.w1; a.b1 = w.b1; a.xin = x; a.h0 = h0; a.h1 = h1; a.y = y; a.c0 = c0; a.c1 = c1;
  a.seg = seg_dev; a.nseg = nseg; a.H = H; a.layers = layers;
  const unsigned grid = (unsigned)(layers * H / 4);
  const int steps = Tmax + layers - 1;
  if (!chain) {
    for (int st = 0; st < steps; ++st) launch_lstm_step(a, H, grid, st, s);
    HIPC(hipGetLastError());
    return VX_OK;
  }
  if (!*chain) {
    a.meta = meta;
    a.nseg = 0;
    hipGraph_t graph = nullptr;
    HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    for (int st = 0; st < CODEC_LSTM_CHAIN; ++st) launch_lstm_step(a, H, grid, st, s);
    codec_lstm_advance<<<1, 64, 0, s>>>(meta, CODEC_LSTM_CHAIN);
    const hipError_t ce = hipStreamEndCapture(s, &graph);
    if (ce != hipSuccess) return fail(VX_ERR_HIP, "capturing the LSTM chain failed: %s", hipGetErrorString(ce));
    const hipError_t ie = hipGraphInstantiate(chain, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ie != hipSuccess) { *chain = nullptr; return fail(VX_ERR_HIP, "instantiating the LSTM chain failed: %s", hipGetErrorString(ie)); }
  }
  for (int st = 0; st < steps; st += CODEC_LSTM_CHAIN) HIPC(hipGraphLaunch(*chain, s));
  return VX_OK;
}

// LSTM weights (torch layouts, host) -> device operands: W_ih0, b_ih0 + b_hh0, W_hh0, [W_ih1 | W_hh1], b_ih1 + b_hh1
int pack_lstm(const float* const* wih, const float* const* whh, const float* const* bih, const float* const* bhh, int H, int layers,
              LstmDev* d) {
  std::vector<float> b0(4 * H);
  for (int i = 0; i < 4 * H; ++i) b0[i] = bih[0][i] + bhh[0][i];
  VXC(upload(std::vector<float>(wih[0], wih[0] + (size_t)4 * H * H), &d->wih0));
  VXC(upload(std::vector<float>(whh[0], whh[0] + (size_t)4 * H * H), &d->whh0));
  VXC(upload(b0, &d->b0));
  if (layers == 2) {
    std::vector<float> w1((size_t)4 * H * 2 * H), b1(4 * H);
    for (int n = 0; n < 4 * H; ++n) {
      memcpy(&w1[(size_t)n * 2 * H], wih[1] + (size_t)n * H, H * sizeof(float));
      memcpy(&w1[(size_t)n * 2 * H + H], whh[1] + (size_t)n * H, H * sizeof(float));
      b1[n] = bih[1][n] + bhh[1][n];
    }
    VXC(upload(w1, &d->w1));
    VXC(upload(b1, &d->b1));
  }
  return VX_OK;
}
void free_lstm(LstmDev& d) {
  for (float* p : {d.wih0, d.b0, d.whh0, d.w1, d.b1}) (void)hipFree(p);
  d = LstmDev{};
}

int check_segs(const int32_t* seg, int nseg) {
  if (!seg || nseg < 1 || nseg > CODEC_MAX_SEG) return fail(VX_ERR_ARG, "segments: 1..%d expected, got %d", CODEC_MAX_SEG, nseg);
  if (seg[0] != 0) return fail(VX_ERR_ARG, "segment starts begin at 0");
  for (int i = 0; i < nseg; ++i)
    if (seg[i + 1] <= seg[i]) return fail(VX_ERR_ARG, "segment %d is empty or starts are not increasing", i);
  return VX_OK;
}

struct EncStage {
  int c, stride;                             // c -> 2c at `stride`
  float *c3_w = nullptr, *c3_b = nullptr;    // block.1: c -> c / 2, k = res_kernel
  float *mix_w = nullptr, *mix_b = nullptr;  // [block.3 | shortcut]
  float *dn_w = nullptr, *dn_b = nullptr;    // strided convolution, packed by pack_conv
};

struct Stage {
  int cin, cout, stride;
  float *up_w = nullptr, *up_b = nullptr;    // packed transposed conv, bias repeated per phase
  float *c3_w = nullptr, *c3_b = nullptr;    // block.1: cout -> cout / 2, k = res_kernel
  float *mix_w = nullptr, *mix_b = nullptr;  // [block.3 | shortcut]: K = cout / 2 + cout, bias = sum of the two
};

}  // namespace

struct vx_codec {
  vx_codec_config cfg{};
  int W = 0;  // LSTM width = 16 * filters
  std::map<std::string, HostW> w;
  bool allocated = false;  // device objects may exist: vx_codec_destroy frees them
  bool finalized = false;  // every upload and allocation succeeded: set as vx_codec_finalize's last statement
  bool failed = false;     // a finalize failed half way: the handle refuses further use
  hipStream_t own = nullptr;                 // the decoder's stream (the LSTM chain cannot be captured on the null stream)
  hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_copy = nullptr;
  hipGraphExec_t chain = nullptr;
  float* cb = nullptr;  // [n_codebooks][size][dim]
  float *c0_w = nullptr, *c0_b = nullptr, *last_w = nullptr, *last_b = nullptr;
  LstmDev lstm;
  std::vector<Stage> stages;
  // workspace
  long cap_frames = 0, chunk_frames = 0, per_frame = 0;
  // int32 staging: {nseg, step} | frame offsets [max_batch + 1] | per-group relative offsets [2 (max_batch + 1)] | codes [n_q][frames]
  int *codes_dev = nullptr, *codes_host = nullptr;
  size_t stage_ints = 0;
  float *x0 = nullptr, *xc = nullptr, *gin = nullptr, *h0 = nullptr, *h1 = nullptr, *y = nullptr, *c0 = nullptr, *c1 = nullptr;
  float *bufA = nullptr, *bufH = nullptr, *bufB = nullptr;
  // encoder (VX_CODEC_ENCODER)
  bool enc = false;
  float *cb_sq = nullptr;  // [n_codebooks][size]
  float *e0_w = nullptr, *e0_b = nullptr, *elast_w = nullptr, *elast_b = nullptr, *wav = nullptr;
  LstmDev elstm;
  std::vector<EncStage> estages;
  long long **ptrs_dev = nullptr, **ptrs_host = nullptr;  // the utterances' output tensors
  long last_frames = 0;  // frames of the last vx_codec_encode (what x0 holds of it)
};

static std::map<std::string, std::vector<int64_t>> codec_expected(const vx_codec_config& c) {
  std::map<std::string, std::vector<int64_t>> s;
  const int64_t W = 16 * (int64_t)c.filters;
  char k[128];
  s["decoder.layers.0.conv.weight"] = {W, c.hidden, c.kernel};
  s["decoder.layers.0.conv.bias"] = {W};
  for (int l = 0; l < c.lstm_layers; ++l) {
    snprintf(k, sizeof k, "decoder.layers.1.lstm.weight_ih_l%d", l); s[k] = {4 * W, W};
    snprintf(k, sizeof k, "decoder.layers.1.lstm.weight_hh_l%d", l); s[k] = {4 * W, W};
    snprintf(k, sizeof k, "decoder.layers.1.lstm.bias_ih_l%d", l); s[k] = {4 * W};
    snprintf(k, sizeof k, "decoder.layers.1.lstm.bias_hh_l%d", l); s[k] = {4 * W};
  }
  int64_t ch = W;
  for (int i = 0; i < 4; ++i) {
    const int up = 3 + 3 * i, res = 4 + 3 * i;
    snprintf(k, sizeof k, "decoder.layers.%d.conv.weight", up); s[k] = {ch, ch / 2, 2 * (int64_t)c.ratios[i]};
    snprintf(k, sizeof k, "decoder.layers.%d.conv.bias", up); s[k] = {ch / 2};
    ch /= 2;
    snprintf(k, sizeof k, "decoder.layers.%d.block.1.conv.weight", res); s[k] = {ch / 2, ch, c.res_kernel};
    snprintf(k, sizeof k, "decoder.layers.%d.block.1.conv.bias", res); s[k] = {ch / 2};
    snprintf(k, sizeof k, "decoder.layers.%d.block.3.conv.weight", res); s[k] = {ch, ch / 2, 1};
    snprintf(k, sizeof k, "decoder.layers.%d.block.3.conv.bias", res); s[k] = {ch};
    snprintf(k, sizeof k, "decoder.layers.%d.shortcut.conv.weight", res); s[k] = {ch, ch, 1};
    snprintf(k, sizeof k, "decoder.layers.%d.shortcut.conv.bias", res); s[k] = {ch};
  }
  s["decoder.layers.15.conv.weight"] = {1, ch, c.last_kernel};
  s["decoder.layers.15.conv.bias"] = {1};
  for (int q = 0; q < c.n_codebooks; ++q) {
    snprintf(k, sizeof k, "quantizer.layers.%d.codebook.embed", q); s[k] = {c.codebook_size, c.codebook_dim};
  }
  if (!(c.flags & VX_CODEC_ENCODER)) return s;
  ch = c.filters;
  s["encoder.layers.0.conv.weight"] = {ch, 1, c.kernel};
  s["encoder.layers.0.conv.bias"] = {ch};
  for (int i = 0; i < 4; ++i) {
    const int res = 1 + 3 * i, dn = 3 + 3 * i;
    snprintf(k, sizeof k, "encoder.layers.%d.block.1.conv.weight", res); s[k] = {ch / 2, ch, c.res_kernel};
    snprintf(k, sizeof k, "encoder.layers.%d.block.1.conv.bias", res); s[k] = {ch / 2};
    snprintf(k, sizeof k, "encoder.layers.%d.block.3.conv.weight", res); s[k] = {ch, ch / 2, 1};
    snprintf(k, sizeof k, "encoder.layers.%d.block.3.conv.bias", res); s[k] = {ch};
    snprintf(k, sizeof k, "encoder.layers.%d.shortcut.conv.weight", res); s[k] = {ch, ch, 1};
    snprintf(k, sizeof k, "encoder.layers.%d.shortcut.conv.bias", res); s[k] = {ch};
    snprintf(k, sizeof k, "encoder.layers.%d.conv.weight", dn); s[k] = {2 * ch, ch, 2 * (int64_t)c.ratios[3 - i]};
    snprintf(k, sizeof k, "encoder.layers.%d.conv.bias", dn); s[k] = {2 * ch};
    ch *= 2;
  }
  for (int l = 0; l < c.lstm_layers; ++l) {
    snprintf(k, sizeof k, "encoder.layers.13.lstm.weight_ih_l%d", l); s[k] = {4 * W, W};
    snprintf(k, sizeof k, "encoder.layers.13.lstm.weight_hh_l%d", l); s[k] = {4 * W, W};
    snprintf(k, sizeof k, "encoder.layers.13.lstm.bias_ih_l%d", l); s[k] = {4 * W};
    snprintf(k, sizeof k, "encoder.layers.13.lstm.bias_hh_l%d", l); s[k] = {4 * W};
  }
  s["encoder.layers.15.conv.weight"] = {c.hidden, W, c.last_kernel};
  s["encoder.layers.15.conv.bias"] = {c.hidden};
  return s;
}

extern "C" int vx_codec_create(const vx_codec_config* cfg, vx_codec** out) {
  if (!cfg || !out) return fail(VX_ERR_ARG, "vx_codec_create: null argument");
  if (cfg->struct_size != (int32_t)sizeof(vx_codec_config))
    return fail(VX_ERR_ARG, "vx_codec_config.struct_size %d != %d", cfg->struct_size, (int)sizeof(vx_codec_config));
  const vx_codec_config& c = *cfg;
  if (c.hidden < 1 || c.filters < 1 || c.codebook_size < 1 || c.codebook_dim < 1 || c.n_codebooks < 1 || c.max_frames < 1 ||
      c.max_batch < 1 || c.kernel < 1 || c.last_kernel < 1 || c.res_kernel < 1 || c.lstm_layers < 0 || c.device < 0 ||
      (c.flags & ~(VX_CODEC_LSTM_GRAPH | VX_CODEC_ENCODER)))
    return fail(VX_ERR_ARG, "vx_codec_config: sizes must be positive and flags known");
  for (int i = 0; i < 4; ++i)
    if (c.ratios[i] < 1) return fail(VX_ERR_ARG, "vx_codec_config.ratios[%d] = %d", i, c.ratios[i]);
  const int W = 16 * c.filters;
  if (c.codebook_dim != c.hidden) return fail(VX_ERR_UNSUPPORTED, "codebook_dim %d != hidden %d", c.codebook_dim, c.hidden);
  if (c.lstm_layers < 1 || c.lstm_layers > 2) return fail(VX_ERR_UNSUPPORTED, "lstm_layers %d: the step kernel serves 1 or 2", c.lstm_layers);
  if (!lstm_width_ok(W)) return fail(VX_ERR_UNSUPPORTED, "LSTM width 16 * filters = %d: the step kernel serves 64, 128, 256, 512", W);
  if (c.kernel > 15 || c.last_kernel > 15 || c.res_kernel > 15) return fail(VX_ERR_UNSUPPORTED, "kernel sizes above 15");
  if (c.n_codebooks > CODEC_MAX_Q) return fail(VX_ERR_UNSUPPORTED, "n_codebooks %d > %d", c.n_codebooks, CODEC_MAX_Q);
  if (c.max_batch > CODEC_MAX_SEG) return fail(VX_ERR_UNSUPPORTED, "max_batch %d > %d", c.max_batch, CODEC_MAX_SEG);
  long hop = 1;
  for (int i = 0; i < 4; ++i) hop *= c.ratios[i];
  if (hop * (long)c.max_frames * c.max_batch >= (1L << 40)) return fail(VX_ERR_UNSUPPORTED, "capacity too large");
  if (c.flags & VX_CODEC_ENCODER) {
    if (!rvq_shape_ok(c.codebook_size, c.codebook_dim))
      return fail(VX_ERR_UNSUPPORTED, "encoder: codebook %d x %d: the search kernel serves sizes in multiples of 32 and dims in multiples of 8 up to %d",
                   c.codebook_size, c.codebook_dim, CODEC_RVQ_MAX_D);
    if (c.filters % 2) return fail(VX_ERR_UNSUPPORTED, "encoder: filters %d is odd", c.filters);
    if (hop * (long)c.max_frames >= (1L << 31)) return fail(VX_ERR_UNSUPPORTED, "encoder: max_frames * hop samples exceed int32");
  }
  vx_codec* e = new vx_codec();
  e->cfg = c;
  e->W = W;
  for (auto& kv : codec_expected(c)) e->w[kv.first].shape = kv.second;
  *out = e;
  return VX_OK;
}

static void codec_free_device(vx_codec* e) {
  for (float* p : {e->cb, e->c0_w, e->c0_b, e->last_w, e->last_b, e->x0, e->xc, e->gin, e->h0, e->h1, e->y, e->c0, e->c1, e->bufA,
                   e->bufH, e->bufB})
    (void)hipFree(p);
  free_lstm(e->lstm);
  for (float* p : {e->cb_sq, e->e0_w, e->e0_b, e->elast_w, e->elast_b, e->wav}) (void)hipFree(p);
  free_lstm(e->elstm);
  for (EncStage& st : e->estages)
    for (float* p : {st.c3_w, st.c3_b, st.mix_w, st.mix_b, st.dn_w, st.dn_b}) (void)hipFree(p);
  (void)hipFree(e->ptrs_dev);
  (void)hipHostFree(e->ptrs_host);
  for (Stage& st : e->stages)
    for (float* p : {st.up_w, st.up_b, st.c3_w, st.c3_b, st.mix_w, st.mix_b}) (void)hipFree(p);
  (void)hipFree(e->codes_dev);
  (void)hipHostFree(e->codes_host);
  if (e->chain) (void)hipGraphExecDestroy(e->chain);
  for (hipEvent_t ev : {e->ev_in, e->ev_out, e->ev_copy})
    if (ev) (void)hipEventDestroy(ev);
  if (e->own) (void)hipStreamDestroy(e->own);
}

extern "C" void vx_codec_destroy(vx_codec* e) {
  if (!e) return;
  if (e->allocated) {
    DevGuard g(e->cfg.device);
    if (e->own) (void)hipStreamSynchronize(e->own);
    codec_free_device(e);
  }
  delete e;
}

extern "C" int vx_codec_set_weight(vx_codec* e, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
  if (!e || !key || !data || !shape) return fail(VX_ERR_ARG, "vx_codec_set_weight: null argument");
  if (e->finalized) return fail(VX_ERR_STATE, "vx_codec_set_weight after vx_codec_finalize");
  auto it = e->w.find(key);
  if (it == e->w.end()) return fail(VX_ERR_WEIGHTS, "unknown key %s", key);
  HostW& t = it->second;
  bool same = (size_t)ndim == t.shape.size();
  size_t n = 1;
  for (int i = 0; same && i < ndim; ++i) { same = shape[i] == t.shape[i]; n *= (size_t)shape[i]; }
  if (!same) return fail(VX_ERR_WEIGHTS, "wrong shape for %s", key);
  t.v.assign(data, data + n);
  t.set = true;
  return VX_OK;
}

static int alloc_f(float** p, size_t n) {
  HIPC(hipMalloc((void**)p, n * sizeof(float) + 16));
  return VX_OK;
}

extern "C" int vx_codec_finalize(vx_codec* e) {
  if (!e) return fail(VX_ERR_ARG, "vx_codec_finalize: null handle");
  if (e->finalized) return VX_OK;
  if (e->failed) return fail(VX_ERR_STATE, "vx_codec_finalize failed earlier on this handle: destroy it and create a new one");
  for (auto& kv : e->w)
    if (!kv.second.set) return fail(VX_ERR_WEIGHTS, "missing tensor %s", kv.first.c_str());
  const vx_codec_config& c = e->cfg;
  e->failed = true;     // until the last statement: a finalize that stops at a HIP error leaves a handle that refuses further use
  ON_DEVICE(c.device);
  e->allocated = true;  // from here vx_codec_destroy frees what was allocated
  const int W = e->W;
  char k[128], k2[128];
  auto host = [&](const char* key) -> const std::vector<float>& { return e->w[key].v; };
  {
    std::vector<float> cb((size_t)c.n_codebooks * c.codebook_size * c.codebook_dim);
    for (int q = 0; q < c.n_codebooks; ++q) {
      snprintf(k, sizeof k, "quantizer.layers.%d.codebook.embed", q);
      memcpy(&cb[(size_t)q * c.codebook_size * c.codebook_dim], host(k).data(), host(k).size() * sizeof(float));
    }
    VXC(upload(cb, &e->cb));
  }
  VXC(upload(pack_conv(host("decoder.layers.0.conv.weight").data(), W, c.hidden, c.kernel), &e->c0_w));
  VXC(upload(host("decoder.layers.0.conv.bias"), &e->c0_b));
  {
    const float *wih[2] = {}, *whh[2] = {}, *bih[2] = {}, *bhh[2] = {};
    for (int l = 0; l < c.lstm_layers; ++l) {
      snprintf(k, sizeof k, "decoder.layers.1.lstm.weight_ih_l%d", l); wih[l] = host(k).data();
      snprintf(k, sizeof k, "decoder.layers.1.lstm.weight_hh_l%d", l); whh[l] = host(k).data();
      snprintf(k, sizeof k, "decoder.layers.1.lstm.bias_ih_l%d", l); bih[l] = host(k).data();
      snprintf(k, sizeof k, "decoder.layers.1.lstm.bias_hh_l%d", l); bhh[l] = host(k).data();
    }
    VXC(pack_lstm(wih, whh, bih, bhh, W, c.lstm_layers, &e->lstm));
  }
  int ch = W;
  long rate = 1, per_frame = 0;
  e->stages.resize(4);
  for (int i = 0; i < 4; ++i) {
    Stage& st = e->stages[i];
    const int up = 3 + 3 * i, res = 4 + 3 * i, r = c.ratios[i];
    st.cin = ch; st.cout = ch / 2; st.stride = r;
    snprintf(k, sizeof k, "decoder.layers.%d.conv.weight", up);
    VXC(upload(pack_convtr(host(k).data(), ch, ch / 2, r), &st.up_w));
    snprintf(k, sizeof k, "decoder.layers.%d.conv.bias", up);
    std::vector<float> rep((size_t)r * (ch / 2));
    for (int p = 0; p < r; ++p) memcpy(&rep[(size_t)p * (ch / 2)], host(k).data(), (ch / 2) * sizeof(float));
    VXC(upload(rep, &st.up_b));
    ch /= 2;
    rate *= r;
    per_frame = std::max(per_frame, rate * ch);
    const int hd = ch / 2;
    snprintf(k, sizeof k, "decoder.layers.%d.block.1.conv.weight", res);
    VXC(upload(pack_conv(host(k).data(), hd, ch, c.res_kernel), &st.c3_w));
    snprintf(k, sizeof k, "decoder.layers.%d.block.1.conv.bias", res);
    VXC(upload(host(k), &st.c3_b));
    snprintf(k, sizeof k, "decoder.layers.%d.block.3.conv.weight", res);
    snprintf(k2, sizeof k2, "decoder.layers.%d.shortcut.conv.weight", res);
    std::vector<float> mix((size_t)ch * (hd + ch)), mb(ch);
    for (int n = 0; n < ch; ++n) {
      memcpy(&mix[(size_t)n * (hd + ch)], host(k).data() + (size_t)n * hd, hd * sizeof(float));
      memcpy(&mix[(size_t)n * (hd + ch) + hd], host(k2).data() + (size_t)n * ch, ch * sizeof(float));
    }
    snprintf(k, sizeof k, "decoder.layers.%d.block.3.conv.bias", res);
    snprintf(k2, sizeof k2, "decoder.layers.%d.shortcut.conv.bias", res);
    for (int n = 0; n < ch; ++n) mb[n] = host(k)[n] + host(k2)[n];
    VXC(upload(mix, &st.mix_w));
    VXC(upload(mb, &st.mix_b));
  }
  VXC(upload(pack_conv(host("decoder.layers.15.conv.weight").data(), 1, ch, c.last_kernel), &e->last_w));
  VXC(upload(host("decoder.layers.15.conv.bias"), &e->last_b));
  e->enc = (c.flags & VX_CODEC_ENCODER) != 0;
  if (e->enc) {
    {
      std::vector<float> sq;
      for (int q = 0; q < c.n_codebooks; ++q) {
        snprintf(k, sizeof k, "quantizer.layers.%d.codebook.embed", q);
        const std::vector<float> one = codebook_sq(host(k).data(), (size_t)c.codebook_size, c.codebook_dim);
        sq.insert(sq.end(), one.begin(), one.end());
      }
      VXC(upload(sq, &e->cb_sq));
    }
    VXC(upload(pack_conv(host("encoder.layers.0.conv.weight").data(), c.filters, 1, c.kernel), &e->e0_w));
    VXC(upload(host("encoder.layers.0.conv.bias"), &e->e0_b));
    int ec = c.filters;
    e->estages.resize(4);
    for (int i = 0; i < 4; ++i) {
      EncStage& st = e->estages[i];
      const int res = 1 + 3 * i, dn = 3 + 3 * i, hd = ec / 2;
      st.c = ec; st.stride = c.ratios[3 - i];
      snprintf(k, sizeof k, "encoder.layers.%d.block.1.conv.weight", res);
      VXC(upload(pack_conv(host(k).data(), hd, ec, c.res_kernel), &st.c3_w));
      snprintf(k, sizeof k, "encoder.layers.%d.block.1.conv.bias", res);
      VXC(upload(host(k), &st.c3_b));
      snprintf(k, sizeof k, "encoder.layers.%d.block.3.conv.weight", res);
      snprintf(k2, sizeof k2, "encoder.layers.%d.shortcut.conv.weight", res);
      std::vector<float> mix((size_t)ec * (hd + ec)), mb(ec);
      for (int n = 0; n < ec; ++n) {
        memcpy(&mix[(size_t)n * (hd + ec)], host(k).data() + (size_t)n * hd, hd * sizeof(float));
        memcpy(&mix[(size_t)n * (hd + ec) + hd], host(k2).data() + (size_t)n * ec, ec * sizeof(float));
      }
      snprintf(k, sizeof k, "encoder.layers.%d.block.3.conv.bias", res);
      snprintf(k2, sizeof k2, "encoder.layers.%d.shortcut.conv.bias", res);
      for (int n = 0; n < ec; ++n) mb[n] = host(k)[n] + host(k2)[n];
      VXC(upload(mix, &st.mix_w));
      VXC(upload(mb, &st.mix_b));
      snprintf(k, sizeof k, "encoder.layers.%d.conv.weight", dn);
      VXC(upload(pack_conv(host(k).data(), 2 * ec, ec, 2 * st.stride), &st.dn_w));
      snprintf(k, sizeof k, "encoder.layers.%d.conv.bias", dn);
      VXC(upload(host(k), &st.dn_b));
      ec *= 2;
    }
    {
      const float *wih[2] = {}, *whh[2] = {}, *bih[2] = {}, *bhh[2] = {};
      for (int l = 0; l < c.lstm_layers; ++l) {
        snprintf(k, sizeof k, "encoder.layers.13.lstm.weight_ih_l%d", l); wih[l] = host(k).data();
        snprintf(k, sizeof k, "encoder.layers.13.lstm.weight_hh_l%d", l); whh[l] = host(k).data();
        snprintf(k, sizeof k, "encoder.layers.13.lstm.bias_ih_l%d", l); bih[l] = host(k).data();
        snprintf(k, sizeof k, "encoder.layers.13.lstm.bias_hh_l%d", l); bhh[l] = host(k).data();
      }
      VXC(pack_lstm(wih, whh, bih, bhh, W, c.lstm_layers, &e->elstm));
    }
    VXC(upload(pack_conv(host("encoder.layers.15.conv.weight").data(), c.hidden, W, c.last_kernel), &e->elast_w));
    VXC(upload(host("encoder.layers.15.conv.bias"), &e->elast_b));
  }
  for (auto& kv : e->w) std::vector<float>().swap(kv.second.v);  // the host copies are not needed any more

  // workspace: the LSTM part holds every frame of a call; the up-sampling part runs over groups of whole utterances of at
  // most chunk_frames frames (its rows are 320x as many)
  e->cap_frames = (long)c.max_frames * c.max_batch;
  e->chunk_frames = std::min(e->cap_frames, std::max<long>(c.max_frames, 8192));
  e->per_frame = std::max<long>(per_frame, 2 * rate);
  const size_t F = (size_t)e->cap_frames;
  VXC(alloc_f(&e->x0, F * c.hidden));
  VXC(alloc_f(&e->xc, F * W));
  VXC(alloc_f(&e->gin, F * 4 * W));
  VXC(alloc_f(&e->h0, F * W));
  VXC(alloc_f(&e->h1, F * W));
  VXC(alloc_f(&e->y, F * W));
  VXC(alloc_f(&e->c0, (size_t)c.max_batch * W));
  VXC(alloc_f(&e->c1, (size_t)c.max_batch * W));
  // encoder: the same three buffers hold its stages (filters channels per sample at most, as the decoder's last stage), plus one
  // row per utterance and stage for the rounded-up row counts
  const size_t slack = e->enc ? (size_t)c.max_batch * W : 0;
  VXC(alloc_f(&e->bufA, (size_t)e->chunk_frames * e->per_frame + slack));
  VXC(alloc_f(&e->bufB, (size_t)e->chunk_frames * e->per_frame + slack));
  VXC(alloc_f(&e->bufH, (size_t)e->chunk_frames * e->per_frame / 2 + slack));
  e->stage_ints = 2 + F * c.n_codebooks + 3 * (size_t)(c.max_batch + 1);
  if (e->enc) {
    e->stage_ints += 8 * (size_t)(c.max_batch + 1);  // four more row tables per utterance group
    VXC(alloc_f(&e->wav, (size_t)e->chunk_frames * rate));
    HIPC(hipMalloc((void**)&e->ptrs_dev, (size_t)c.max_batch * sizeof(void*)));
    HIPC(hipHostMalloc((void**)&e->ptrs_host, (size_t)c.max_batch * sizeof(void*)));
  }
  HIPC(hipMalloc((void**)&e->codes_dev, e->stage_ints * sizeof(int)));
  HIPC(hipHostMalloc((void**)&e->codes_host, e->stage_ints * sizeof(int)));
  HIPC(hipStreamCreateWithFlags(&e->own, hipStreamNonBlocking));
  HIPC(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
  HIPC(hipEventCreateWithFlags(&e->ev_out, hipEventDisableTiming));
  HIPC(hipEventCreateWithFlags(&e->ev_copy, hipEventDisableTiming));
  HIPC(hipEventRecord(e->ev_copy, e->own));
  e->failed = false;
  e->finalized = true;
  return VX_OK;
}

extern "C" int vx_codec_decode(vx_codec* e, int32_t n, const int64_t* const* codes, const int32_t* T, int32_t n_q,
                               float* const* wav_out, void* stream) {
  if (!e || !codes || !T || !wav_out) return fail(VX_ERR_ARG, "vx_codec_decode: null argument");
  const vx_codec_config& c = e->cfg;
  if (n < 1) return fail(VX_ERR_ARG, "n = %d utterances", n);
  if (n > c.max_batch) return fail(VX_ERR_CAPACITY, "n = %d utterances > max_batch %d", n, c.max_batch);
  if (n_q < 1 || n_q > c.n_codebooks) return fail(VX_ERR_ARG, "n_q = %d outside [1, %d]", n_q, c.n_codebooks);
  long total = 0;
  for (int i = 0; i < n; ++i) {
    if (!codes[i] || !wav_out[i]) return fail(VX_ERR_ARG, "utterance %d: null pointer", i);
    if (T[i] < 1) return fail(VX_ERR_ARG, "utterance %d: T = %d", i, T[i]);
    if (T[i] > c.max_frames) return fail(VX_ERR_CAPACITY, "utterance %d: T = %d > max_frames %d", i, T[i], c.max_frames);
    total += T[i];
  }
  for (int i = 0; i < n; ++i)
    for (long j = 0; j < (long)n_q * T[i]; ++j)
      if (codes[i][j] < 0 || codes[i][j] >= c.codebook_size)
        return fail(VX_ERR_ARG, "utterance %d: code %lld outside [0, %d)", i, (long long)codes[i][j], c.codebook_size);
  if (!e->finalized) return fail(VX_ERR_STATE, "vx_codec_decode before vx_codec_finalize");
  ON_DEVICE(c.device);
  // The work runs on the decoder's own stream, ordered after everything already enqueued on `stream`; `stream` waits for it
  // before the call returns (as the engine's entry points do).  The host waits only for the previous call's staging copy.
  hipStream_t s = e->own;
  HIPC(hipEventRecord(e->ev_in, (hipStream_t)stream));
  HIPC(hipStreamWaitEvent(s, e->ev_in, 0));
  const int W = e->W;

  HIPC(hipEventSynchronize(e->ev_copy));  // the previous call's copy out of the pinned buffer has completed
  int* hc = e->codes_host;
  const int MB1 = c.max_batch + 1;
  hc[0] = n;
  hc[1] = 0;
  int* hseg = hc + 2;
  int* hrel = hseg + MB1;
  int* hcodes = hrel + 2 * MB1;
  std::vector<int> seg(n + 1, 0);
  for (int i = 0; i < n; ++i) seg[i + 1] = seg[i] + T[i];
  for (int i = 0; i < n; ++i)
    for (int q = 0; q < n_q; ++q)
      for (int t = 0; t < T[i]; ++t) hcodes[(size_t)q * total + seg[i] + t] = (int)codes[i][(size_t)q * T[i] + t];
  memcpy(hseg, seg.data(), (n + 1) * sizeof(int));
  struct Group { int u0, u1, off; };
  std::vector<Group> groups;
  int used = 0;
  for (int u0 = 0; u0 < n;) {
    int u1 = u0 + 1;
    while (u1 < n && (long)seg[u1 + 1] - seg[u0] <= e->chunk_frames) ++u1;
    groups.push_back(Group{u0, u1, used});
    for (int u = u0; u <= u1; ++u) hrel[used++] = seg[u] - seg[u0];
    u0 = u1;
  }
  const size_t ints = 2 + 3 * (size_t)MB1 + (size_t)n_q * total;
  HIPC(hipMemcpyAsync(e->codes_dev, hc, ints * sizeof(int), hipMemcpyHostToDevice, s));
  HIPC(hipEventRecord(e->ev_copy, s));
  int* dmeta = e->codes_dev;
  const int* dseg = e->codes_dev + 2;
  const int* drel = dseg + MB1;
  const int* dcodes = drel + 2 * MB1;

  const long e0 = total * c.hidden;
  e->last_frames = 0;  // x0 no longer holds an encode's embeddings
  codec_rvq_rows<<<(unsigned)((e0 + 255) / 256), 256, 0, s>>>(dcodes, e->cb, e->x0, total, n_q, c.codebook_size, c.codebook_dim);
  HIPC(hipGetLastError());
  VXC(run_conv(e->x0, e->c0_w, e->c0_b, e->xc, total, c.hidden, W, c.kernel, 0, dseg, n, 1, s));
  VXC(run_lstm(e->lstm, e->xc, e->gin, e->h0, e->h1, e->c0, e->c1, e->y, W, c.lstm_layers, dseg, seg.data(), n, s,
                (c.flags & VX_CODEC_LSTM_GRAPH) ? &e->chain : nullptr, dmeta));

  for (const Group& gr : groups) {
    const int ns = gr.u1 - gr.u0;
    const int* sg = drel + gr.off;
    const long frames = seg[gr.u1] - seg[gr.u0];
    const float* x = e->y + (size_t)seg[gr.u0] * W;
    long rate = 1;
    for (const Stage& st : e->stages) {
      VXC(run_convtr(x, st.up_w, st.up_b, e->bufA, frames * rate, st.cin, st.cout, st.stride, 1, sg, ns, (int)rate, s));
      rate *= st.stride;
      const int ch = st.cout, hd = ch / 2;
      VXC(run_conv(e->bufA, st.c3_w, st.c3_b, e->bufH, frames * rate, ch, hd, c.res_kernel, 1, sg, ns, (int)rate, s));
      CodecGemmArgs a{};
      a.part[0] = CodecPart{e->bufH, hd, 1, CODEC_PAD_ZERO, 1};
      a.part[1] = CodecPart{e->bufA, ch, 1, CODEC_PAD_ZERO, 0};
      a.nparts = 2;
      a.W = st.mix_w; a.bias = st.mix_b; a.out = e->bufB; a.M = frames * rate; a.N = ch; a.K = hd + ch;
      a.seg = sg; a.nseg = ns; a.rate = (int)rate;
      VXC(launch_gemm(a, s));
      x = e->bufB;
    }
    const int ch = e->stages.back().cout;
    VXC(run_conv(e->bufB, e->last_w, e->last_b, e->bufH, frames * rate, ch, 1, c.last_kernel, 1, sg, ns, (int)rate, s));
    for (int u = gr.u0; u < gr.u1; ++u)
      HIPC(hipMemcpyAsync(wav_out[u], e->bufH + (size_t)(seg[u] - seg[gr.u0]) * rate, (size_t)T[u] * rate * sizeof(float),
                           hipMemcpyDeviceToDevice, s));
  }
  HIPC(hipEventRecord(e->ev_out, s));
  HIPC(hipStreamWaitEvent((hipStream_t)stream, e->ev_out, 0));
  return VX_OK;
}

extern "C" int vx_codec_encode(vx_codec* e, int32_t n, const float* const* wav, const int32_t* n_samples, int32_t n_q,
                               int64_t* const* codes_out, void* stream) {
  if (!e || !wav || !n_samples || !codes_out) return fail(VX_ERR_ARG, "vx_codec_encode: null argument");
  const vx_codec_config& c = e->cfg;
  if (!(c.flags & VX_CODEC_ENCODER)) return fail(VX_ERR_STATE, "vx_codec_encode on a handle created without VX_CODEC_ENCODER");
  if (n < 1) return fail(VX_ERR_ARG, "n = %d utterances", n);
  if (n > c.max_batch) return fail(VX_ERR_CAPACITY, "n = %d utterances > max_batch %d", n, c.max_batch);
  if (n_q < 1 || n_q > c.n_codebooks) return fail(VX_ERR_ARG, "n_q = %d outside [1, %d]", n_q, c.n_codebooks);
  long hop = 1;
  for (int i = 0; i < 4; ++i) hop *= c.ratios[i];
  const long max_samples = (long)c.max_frames * hop;
  for (int i = 0; i < n; ++i) {
    if (!wav[i] || !codes_out[i]) return fail(VX_ERR_ARG, "utterance %d: null pointer", i);
    if (n_samples[i] < 1) return fail(VX_ERR_ARG, "utterance %d: %d samples", i, n_samples[i]);
    if (n_samples[i] > max_samples)
      return fail(VX_ERR_CAPACITY, "utterance %d: %d samples > max_frames %d x %ld", i, n_samples[i], c.max_frames, hop);
  }
  if (!e->finalized) return fail(VX_ERR_STATE, "vx_codec_encode before vx_codec_finalize");
  ON_DEVICE(c.device);
  hipStream_t s = e->own;  // ordering as vx_codec_decode
  HIPC(hipEventRecord(e->ev_in, (hipStream_t)stream));
  HIPC(hipStreamWaitEvent(s, e->ev_in, 0));
  const int W = e->W;

  HIPC(hipEventSynchronize(e->ev_copy));
  int* hc = e->codes_host;
  const int MB1 = c.max_batch + 1;
  hc[0] = n;
  hc[1] = 0;
  int* hseg = hc + 2;          // frame offsets of the call
  int* hrel = hseg + MB1;      // per group: frame offsets relative to the group (stage 4 rows)
  int* hlv = hrel + 2 * MB1;   // per stage 0..3: per group row offsets, [4][2 MB1]
  std::vector<int> seg(n + 1, 0);
  auto cdiv = [](long a, long b) { return (a + b - 1) / b; };
  for (int i = 0; i < n; ++i) seg[i + 1] = seg[i] + (int)cdiv(n_samples[i], hop);
  const long total = seg[n];
  memcpy(hseg, seg.data(), (n + 1) * sizeof(int));
  struct Group { int u0, u1, off; long rows[5]; };
  std::vector<Group> groups;
  int used = 0;
  for (int u0 = 0; u0 < n;) {
    int u1 = u0 + 1;
    while (u1 < n && (long)seg[u1 + 1] - seg[u0] <= e->chunk_frames) ++u1;
    Group gr{u0, u1, used, {0, 0, 0, 0, 0}};
    long acc[5] = {0, 0, 0, 0, 0};
    for (int u = u0; u <= u1; ++u) {
      for (int l = 0; l < 4; ++l) hlv[l * 2 * MB1 + used] = (int)acc[l];
      hrel[used] = (int)acc[4];
      ++used;
      if (u == u1) break;
      long rows = n_samples[u];
      acc[0] += rows;
      for (int l = 0; l < 4; ++l) {
        rows = cdiv(rows, e->estages[l].stride);
        acc[l + 1] += rows;
      }
    }
    for (int l = 0; l < 5; ++l) gr.rows[l] = acc[l];
    groups.push_back(gr);
    u0 = u1;
  }
  for (int i = 0; i < n; ++i) e->ptrs_host[i] = (long long*)codes_out[i];
  const size_t ints = 2 + 11 * (size_t)MB1;
  HIPC(hipMemcpyAsync(e->codes_dev, hc, ints * sizeof(int), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(e->ptrs_dev, e->ptrs_host, (size_t)n * sizeof(void*), hipMemcpyHostToDevice, s));
  HIPC(hipEventRecord(e->ev_copy, s));
  const int* dseg = e->codes_dev + 2;
  const int* drel = dseg + MB1;
  const int* dlv = drel + 2 * MB1;
  int* dcodes = e->codes_dev + 2 + 11 * MB1;  // [n_q][total]

  for (const Group& gr : groups) {
    const int ns = gr.u1 - gr.u0;
    const int* sg[5] = {dlv + gr.off, dlv + 2 * MB1 + gr.off, dlv + 4 * MB1 + gr.off, dlv + 6 * MB1 + gr.off, drel + gr.off};
    long off = 0;
    for (int u = gr.u0; u < gr.u1; ++u) {
      HIPC(hipMemcpyAsync(e->wav + off, wav[u], (size_t)n_samples[u] * sizeof(float), hipMemcpyDeviceToDevice, s));
      off += n_samples[u];
    }
    VXC(run_conv_in(e->wav, e->e0_w, e->e0_b, e->bufA, gr.rows[0], c.filters, c.kernel, sg[0], ns, s));
    for (int l = 0; l < 4; ++l) {
      const EncStage& st = e->estages[l];
      const int ch = st.c, hd = ch / 2;
      VXC(run_conv(e->bufA, st.c3_w, st.c3_b, e->bufH, gr.rows[l], ch, hd, c.res_kernel, 1, sg[l], ns, 1, s));
      CodecGemmArgs a{};
      a.part[0] = CodecPart{e->bufH, hd, 1, CODEC_PAD_ZERO, 1};
      a.part[1] = CodecPart{e->bufA, ch, 1, CODEC_PAD_ZERO, 0};
      a.nparts = 2;
      a.W = st.mix_w; a.bias = st.mix_b; a.out = e->bufB; a.M = gr.rows[l]; a.N = ch; a.K = hd + ch;
      a.seg = sg[l]; a.nseg = ns; a.rate = 1;
      VXC(launch_gemm(a, s));
      float* out = l == 3 ? e->xc + (size_t)seg[gr.u0] * W : e->bufA;
      VXC(run_conv_strided(e->bufB, st.dn_w, st.dn_b, out, gr.rows[l + 1], ch, 2 * ch, st.stride, 1, sg[l + 1], sg[l], ns, s));
    }
  }
  VXC(run_lstm(e->elstm, e->xc, e->gin, e->h0, e->h1, e->c0, e->c1, e->y, W, c.lstm_layers, dseg, seg.data(), n, s));
  e->last_frames = 0;
  VXC(run_conv(e->y, e->elast_w, e->elast_b, e->x0, total, W, c.hidden, c.last_kernel, 1, dseg, n, 1, s));
  e->last_frames = total;
  VXC(run_rvq_encode(e->x0, e->cb, e->cb_sq, dcodes, total, n_q, c.codebook_size, c.codebook_dim, s));
  const long nc = total * n_q;
  codec_codes_out<<<(unsigned)((nc + 255) / 256), 256, 0, s>>>(dcodes, e->ptrs_dev, dseg, n, total, n_q);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(e->ev_out, s));
  HIPC(hipStreamWaitEvent((hipStream_t)stream, e->ev_out, 0));
  return VX_OK;
}

// The embeddings (the quantiser's input, [rows][hidden]) of the last vx_codec_encode, rows in the order of its utterances: copied to
// `out` (device) on the codec's stream, `stream` ordered after it.  For the parity tests.
extern "C" int vx_codec_last_embeddings(vx_codec* e, float* out, int64_t rows, void* stream) {
  if (!e || !out) return fail(VX_ERR_ARG, "vx_codec_last_embeddings: null argument");
  if (!(e->cfg.flags & VX_CODEC_ENCODER) || !e->finalized) return fail(VX_ERR_STATE, "vx_codec_last_embeddings: no finalised encoder");
  if (rows < 1 || rows > e->last_frames)
    return fail(VX_ERR_ARG, "vx_codec_last_embeddings: rows = %lld, the last encode had %ld frames", (long long)rows, e->last_frames);
  ON_DEVICE(e->cfg.device);
  HIPC(hipMemcpyAsync(out, e->x0, (size_t)rows * e->cfg.hidden * sizeof(float), hipMemcpyDeviceToDevice, e->own));
  HIPC(hipEventRecord(e->ev_out, e->own));
  HIPC(hipStreamWaitEvent((hipStream_t)stream, e->ev_out, 0));
  return VX_OK;
}

// ---- op-level test entries: x / out device fp32 rows, weights and biases HOST fp32 in torch's layouts (packed here exactly as
// vx_codec_finalize packs them), seg_frames HOST nseg + 1 frame offsets.  Synchronous. ----------------------------------------
namespace {
int upload_segs(const int32_t* seg, int nseg, DevBuf<int>& d) {
  VXC(d.alloc(nseg + 1));
  HIPC(hipMemcpy(d.get(), seg, (nseg + 1) * sizeof(int), hipMemcpyHostToDevice));
  return VX_OK;
}
// as upload() for the handle's own buffers: 16 spare bytes, a blocking copy
int upload(const std::vector<float>& h, DevBuf<float>& d) {
  VXC(d.alloc(h.size() + 4));
  HIPC(hipMemcpy(d.get(), h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  return VX_OK;
}
}  // namespace

extern "C" int vx_op_codec_conv(const float* x, const float* w, const float* bias, float* out, int32_t c_in, int32_t c_out, int32_t k,
                                int32_t elu, int32_t nseg, const int32_t* seg_frames, int32_t rate, void* stream) {
  if (!x || !w || !out || c_in < 1 || c_out < 1 || k < 1 || k > 15 || rate < 1) return fail(VX_ERR_ARG, "vx_op_codec_conv: bad argument");
  VXC(check_segs(seg_frames, nseg));
  hipStream_t s = (hipStream_t)stream;
  DevBuf<int> sg;
  DevBuf<float> wp, bp;
  VXC(upload_segs(seg_frames, nseg, sg));
  VXC(upload(pack_conv(w, c_out, c_in, k), wp));
  if (bias) VXC(upload(std::vector<float>(bias, bias + c_out), bp));
  VXC(run_conv(x, wp.get(), bp.get(), out, (long)seg_frames[nseg] * rate, c_in, c_out, k, elu, sg.get(), nseg, rate, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

extern "C" int vx_op_codec_convtr(const float* x, const float* w, const float* bias, float* out, int32_t c_in, int32_t c_out,
                                  int32_t stride, int32_t elu, int32_t nseg, const int32_t* seg_frames, int32_t rate, void* stream) {
  if (!x || !w || !out || c_in < 1 || c_out < 1 || stride < 1 || rate < 1) return fail(VX_ERR_ARG, "vx_op_codec_convtr: bad argument");
  VXC(check_segs(seg_frames, nseg));
  hipStream_t s = (hipStream_t)stream;
  DevBuf<int> sg;
  DevBuf<float> wp, bp;
  VXC(upload_segs(seg_frames, nseg, sg));
  VXC(upload(pack_convtr(w, c_in, c_out, stride), wp));
  if (bias) {
    std::vector<float> rep((size_t)stride * c_out);
    for (int p = 0; p < stride; ++p) memcpy(&rep[(size_t)p * c_out], bias, c_out * sizeof(float));
    VXC(upload(rep, bp));
  }
  VXC(run_convtr(x, wp.get(), bp.get(), out, (long)seg_frames[nseg] * rate, c_in, c_out, stride, elu, sg.get(), nseg, rate, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

extern "C" int vx_op_codec_lstm(const float* x, const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                                const float* const* b_hh, float* y, int32_t width, int32_t layers, int32_t nseg,
                                const int32_t* seg_frames, void* stream) {
  if (!x || !w_ih || !w_hh || !b_ih || !b_hh || !y) return fail(VX_ERR_ARG, "vx_op_codec_lstm: null argument");
  if (layers < 1 || layers > 2 || !lstm_width_ok(width)) return fail(VX_ERR_UNSUPPORTED, "vx_op_codec_lstm: width %d, layers %d", width, layers);
  VXC(check_segs(seg_frames, nseg));
  hipStream_t s = (hipStream_t)stream;
  DevBuf<int> sg;
  VXC(upload_segs(seg_frames, nseg, sg));
  LstmDev d;
  int r = pack_lstm(w_ih, w_hh, b_ih, b_hh, width, layers, &d);
  const size_t rows = seg_frames[nseg];
  DevBuf<float> gin, h0, h1, c0, c1;  // 16 spare bytes each, as alloc_f()
  if (r == VX_OK) r = gin.alloc(rows * 4 * width + 4);
  if (r == VX_OK) r = h0.alloc(rows * width + 4);
  if (r == VX_OK) r = h1.alloc(rows * width + 4);
  if (r == VX_OK) r = c0.alloc((size_t)nseg * width + 4);
  if (r == VX_OK) r = c1.alloc((size_t)nseg * width + 4);
  if (r == VX_OK) r = run_lstm(d, x, gin.get(), h0.get(), h1.get(), c0.get(), c1.get(), y, width, layers, sg.get(), seg_frames, nseg, s);
  if (r == VX_OK && hipStreamSynchronize(s) != hipSuccess) r = fail(VX_ERR_HIP, "vx_op_codec_lstm: synchronise failed");
  free_lstm(d);
  return r;
}

// Encoder convolution on caller data: x device rows [seg_rows_in[nseg]][c_in], w HOST (c_out, c_in, k), out device rows
// [sum ceil(len_i / stride)][c_out].  stride == 1: the causal convolution (c_in == 1 runs the first convolution's kernel, elu must be
// 0 there); stride > 1: k must be 2 stride.
extern "C" int vx_op_codec_conv_strided(const float* x, const float* w, const float* bias, float* out, int32_t c_in, int32_t c_out,
                                        int32_t k, int32_t stride, int32_t elu, int32_t nseg, const int32_t* seg_rows_in, void* stream) {
  if (!x || !w || !out || c_in < 1 || c_out < 1 || k < 1 || k > 32 || stride < 1) return fail(VX_ERR_ARG, "vx_op_codec_conv_strided: bad argument");
  if (stride > 1 && k != 2 * stride) return fail(VX_ERR_UNSUPPORTED, "vx_op_codec_conv_strided: k = %d, stride = %d (k = 2 stride is served)", k, stride);
  if (c_in == 1 && stride == 1 && elu) return fail(VX_ERR_UNSUPPORTED, "vx_op_codec_conv_strided: the first convolution has no ELU");
  VXC(check_segs(seg_rows_in, nseg));
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> so(nseg + 1, 0);
  for (int i = 0; i < nseg; ++i) so[i + 1] = so[i] + (seg_rows_in[i + 1] - seg_rows_in[i] + stride - 1) / stride;
  DevBuf<int> sg, sgo;
  DevBuf<float> wp, bp;
  VXC(upload_segs(seg_rows_in, nseg, sg));
  VXC(upload_segs(so.data(), nseg, sgo));
  VXC(upload(pack_conv(w, c_out, c_in, k), wp));
  if (bias) VXC(upload(std::vector<float>(bias, bias + c_out), bp));
  if (stride > 1) VXC(run_conv_strided(x, wp.get(), bp.get(), out, so[nseg], c_in, c_out, stride, elu, sgo.get(), sg.get(), nseg, s));
  else if (c_in == 1) VXC(run_conv_in(x, wp.get(), bp.get(), out, so[nseg], c_out, k, sg.get(), nseg, s));
  else VXC(run_conv(x, wp.get(), bp.get(), out, so[nseg], c_in, c_out, k, elu, sg.get(), nseg, 1, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

// The quantiser's search on caller data: emb device [rows][dim], codebooks HOST [n_q][size][dim], codes_out device int32 [n_q][rows].
extern "C" int vx_op_codec_rvq_encode(const float* emb, const float* codebooks, int32_t* codes_out, int64_t rows, int32_t n_q,
                                      int32_t size, int32_t dim, void* stream) {
  if (!emb || !codebooks || !codes_out || rows < 1 || n_q < 1 || n_q > CODEC_MAX_Q) return fail(VX_ERR_ARG, "vx_op_codec_rvq_encode: bad argument");
  if (size < 1 || dim < 1 || !rvq_shape_ok(size, dim)) return fail(VX_ERR_UNSUPPORTED, "vx_op_codec_rvq_encode: codebook %d x %d", size, dim);
  hipStream_t s = (hipStream_t)stream;
  DevBuf<float> cb, sq;
  const size_t n = (size_t)n_q * size;
  VXC(upload(std::vector<float>(codebooks, codebooks + n * dim), cb));
  VXC(upload(codebook_sq(codebooks, n, dim), sq));
  VXC(run_rvq_encode(emb, cb.get(), sq.get(), codes_out, rows, n_q, size, dim, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

// ---- sample-rate conversion and mix-down (vx_resampler_*, codec_resample) -------------------------------------------------------
namespace {
// Device side of a resampler: made on the device that is current at the first vx_resample, dropped as a whole.
struct ResamplerDev {
  DevBuf<float> coef;
  DevBuf<int> phase;  // first [n] | count [n]
  CallStage stage;  // per call: a RaggedTable of in | out pointers, tile0, len_in | chans | len_out
};

enum { COL_IN, COL_OUT, N_PTR_COLS };                         // the staged block's pointer columns
enum { COL_LEN_IN, COL_CHANS, COL_LEN_OUT, N_INT_COLS };      // and its int columns
}  // namespace

struct vx_resampler : LazyDev<ResamplerDev> {
  int orig = 0, neu = 0, max_batch = 0;
  int o = 1, n = 1, T = 1, tile_out = 256;
  std::vector<float> coef;        // [T][n], scale folded in, zero past a phase's count
  std::vector<int> first, count;  // [n]
};

namespace {

constexpr long RESAMPLE_MAX_TABLE = 1L << 24;
constexpr int RESAMPLE_WIDTH = 6;  // lowpass_filter_width; roll-off 0.99 = 99 / 100 below

long gcd_l(long a, long b) {
  while (b) { const long t = a % b; a = b; b = t; }
  return a;
}

// Input k (relative to q o) lies inside the window of phase p: |t| < 6 with t = (k n - p o) base / (o n), base = 99 min(o, n) / 100,
// in exact integers, so that a phase's taps are exactly the i with |i - j o / n| < 6 o / base and both ends move forward with j.
bool tap_inside(long k, long p, long o, long n) {
  __int128 d = (__int128)k * n - (__int128)p * o;
  if (d < 0) d = -d;
  return d * 99 * std::min(o, n) < (__int128)(100 * RESAMPLE_WIDTH) * o * n;
}

int resampler_build(vx_resampler* r) {
  const long g = gcd_l(r->orig, r->neu), o = r->orig / g, n = r->neu / g;
  r->o = (int)o;
  r->n = (int)n;
  if (o == n) {  // the same rate: the mixed-down input itself
    r->T = 1; r->tile_out = 256;
    r->coef = {1.f}; r->first = {0}; r->count = {1};
    return VX_OK;
  }
  const double base = 0.99 * (double)std::min(o, n), R = RESAMPLE_WIDTH * (double)o / base;
  if ((double)n * (2.0 * R + 2.0) > (double)RESAMPLE_MAX_TABLE)
    return fail(VX_ERR_UNSUPPORTED, "vx_resampler_create: %d -> %d Hz needs %ld phases of about %.0f taps: above %ld coefficients", r->orig,
                 r->neu, n, 2.0 * R, RESAMPLE_MAX_TABLE);
  if (2.0 * R + 4.0 > RESAMPLE_SPAN)
    return fail(VX_ERR_UNSUPPORTED, "vx_resampler_create: %d -> %d Hz: %.0f taps per sample exceed the kernel's window of %d", r->orig, r->neu,
                 2.0 * R, RESAMPLE_SPAN);
  r->first.resize(n);
  r->count.resize(n);
  int T = 1;
  for (long p = 0; p < n; ++p) {
    long k = (long)floor((double)p * o / n - R) - 1;
    while (!tap_inside(k, p, o, n)) ++k;
    int cnt = 0;
    while (tap_inside(k + cnt, p, o, n)) ++cnt;
    r->first[p] = (int)k;
    r->count[p] = cnt;
    T = std::max(T, cnt);
  }
  r->T = T;
  r->coef.assign((size_t)T * n, 0.f);
  const double pi = 3.14159265358979323846;
  for (long p = 0; p < n; ++p)
    for (int k = 0; k < r->count[p]; ++k) {
      const double t = (double)((__int128)(r->first[p] + k) * n - (__int128)p * o) * base / ((double)o * (double)n);
      const double sinc = t == 0.0 ? 1.0 : sin(pi * t) / (pi * t);
      const double win = cos(pi * t / (2.0 * RESAMPLE_WIDTH));
      r->coef[(size_t)k * n + p] = (float)(base / (double)o * sinc * win * win);
    }
  // outputs per workgroup: their input span, < (tile - 1) o / n + 2 R + 1 samples, has to fit the staged window
  auto need = [&](long t) { return (long)ceil((double)(t - 1) * o / n + 2.0 * R) + 2; };
  long t = 256;
  if (need(t) > RESAMPLE_SPAN) {
    t = std::max(1L, (long)(((double)RESAMPLE_SPAN - 2.0 - 2.0 * R) * n / o) + 1);
    while (t > 1 && need(t) > RESAMPLE_SPAN) --t;
    if (t >= 64) t &= ~63L;
  }
  if (need(t) > RESAMPLE_SPAN)
    return fail(VX_ERR_UNSUPPORTED, "vx_resampler_create: %d -> %d Hz: one sample's window exceeds %d inputs", r->orig, r->neu, RESAMPLE_SPAN);
  r->tile_out = (int)t;
  return VX_OK;
}

RaggedTable call_table(const vx_resampler* r) { return RaggedTable(r->max_batch, N_PTR_COLS, N_INT_COLS); }

// First use: the tables go to the current device.
int resampler_init_device(vx_resampler* r) {
  VXC(open_device(r));
  ResamplerDev& d = *r->dev;
  const size_t nc = r->coef.size(), n = (size_t)r->n;
  VXC(d.coef.alloc(nc));
  VXC(d.phase.alloc(2 * n));
  VXC(d.stage.init(call_table(r).bytes()));
  HIPC(hipMemcpy(d.coef.get(), r->coef.data(), nc * sizeof(float), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d.phase.get(), r->first.data(), n * sizeof(int), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(d.phase.get() + n, r->count.data(), n * sizeof(int), hipMemcpyHostToDevice));
  return VX_OK;
}

}  // namespace

extern "C" int64_t vx_resample_length(int32_t orig_hz, int32_t new_hz, int64_t n_samples) {
  if (orig_hz <= 0 || new_hz <= 0 || n_samples < 1) {
    fail(VX_ERR_ARG, "vx_resample_length: %d -> %d Hz, %lld samples", orig_hz, new_hz, (long long)n_samples);
    return -1;
  }
  const long g = gcd_l(orig_hz, new_hz), o = orig_hz / g, n = new_hz / g;
  return (int64_t)(((__int128)n * n_samples + o - 1) / o);
}

extern "C" int vx_resampler_create(int32_t orig_hz, int32_t new_hz, int32_t max_batch, vx_resampler** out) {
  if (!out) return fail(VX_ERR_ARG, "vx_resampler_create: null argument");
  if (orig_hz <= 0 || new_hz <= 0) return fail(VX_ERR_ARG, "vx_resampler_create: rates %d -> %d Hz", orig_hz, new_hz);
  if (max_batch < 1) return fail(VX_ERR_ARG, "vx_resampler_create: max_batch = %d", max_batch);
  vx_resampler* r = new vx_resampler();
  r->orig = orig_hz; r->neu = new_hz; r->max_batch = max_batch;
  const int rc = resampler_build(r);
  if (rc != VX_OK) { delete r; return rc; }
  *out = r;
  return VX_OK;
}

extern "C" void vx_resampler_destroy(vx_resampler* r) { destroy_handle(r); }

extern "C" int vx_resample(vx_resampler* r, int32_t n, const float* const* in, const int32_t* channels, const int32_t* n_samples,
                           float* const* out, void* stream) {
  if (!r || !in || !channels || !n_samples || !out) return fail(VX_ERR_ARG, "vx_resample: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_resample: n = %d utterances", n);
  if (n > r->max_batch) return fail(VX_ERR_CAPACITY, "vx_resample: n = %d utterances > max_batch %d", n, r->max_batch);
  std::vector<int> tile0(n + 1, 0), len_out(n);
  for (int i = 0; i < n; ++i) {
    if (!in[i] || !out[i]) return fail(VX_ERR_ARG, "vx_resample: utterance %d: null pointer", i);
    if (channels[i] < 1) return fail(VX_ERR_ARG, "vx_resample: utterance %d: %d channels", i, channels[i]);
    if (n_samples[i] < 1) return fail(VX_ERR_ARG, "vx_resample: utterance %d: %d samples", i, n_samples[i]);
    const long lo = ((long)r->n * n_samples[i] + r->o - 1) / r->o;
    if (lo > 0x7fffffffL) return fail(VX_ERR_UNSUPPORTED, "vx_resample: utterance %d: %ld output samples exceed int32", i, lo);
    len_out[i] = (int)lo;
    const long tiles = tile0[i] + (lo + r->tile_out - 1) / r->tile_out;
    if (tiles > 0x7fffffffL) return fail(VX_ERR_UNSUPPORTED, "vx_resample: utterance %d: the call's output tiles exceed int32", i);
    tile0[i + 1] = (int)tiles;
  }
  VXC(ensure_device(r, resampler_init_device));
  ON_DEVICE(r->device);
  ResamplerDev& d = *r->dev;
  hipStream_t s = (hipStream_t)stream;
  VXC(d.stage.begin(s));
  const RaggedTable t = call_table(r);
  memcpy(t.host_ptrs<const float*>(d.stage, COL_IN), in, n * sizeof(float*));
  memcpy(t.host_ptrs<float*>(d.stage, COL_OUT), out, n * sizeof(float*));
  memcpy(t.host_tile0(d.stage), tile0.data(), (n + 1) * sizeof(int));
  memcpy(t.host_ints(d.stage, COL_LEN_IN), n_samples, n * sizeof(int));
  memcpy(t.host_ints(d.stage, COL_CHANS), channels, n * sizeof(int));
  memcpy(t.host_ints(d.stage, COL_LEN_OUT), len_out.data(), n * sizeof(int));
  VXC(d.stage.upload(t.bytes(), s));
  ResampleArgs a{};
  a.in = t.dev_ptrs<const float* const>(d.stage, COL_IN);
  a.out = t.dev_ptrs<float* const>(d.stage, COL_OUT);
  a.tile0 = t.dev_tile0(d.stage); a.len_in = t.dev_ints(d.stage, COL_LEN_IN); a.chans = t.dev_ints(d.stage, COL_CHANS);
  a.len_out = t.dev_ints(d.stage, COL_LEN_OUT);
  a.coef = d.coef.get(); a.first = d.phase.get(); a.count = d.phase.get() + r->n;
  a.nseg = n; a.o = r->o; a.n = r->n; a.T = r->T; a.tile_out = r->tile_out;
  const unsigned grid = (unsigned)std::min(tile0[n], 2048);
  if ((long)r->T * r->n <= RESAMPLE_TAB) codec_resample<true><<<grid, 256, 0, s>>>(a);
  else codec_resample<false><<<grid, 256, 0, s>>>(a);
  HIPC(hipGetLastError());
  return d.stage.finish(s);
}
