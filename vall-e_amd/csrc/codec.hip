// EnCodec-24 kHz decoder and encoder behind the C ABI (include/vallex.h, vx_codec_*): the packing of the weight table
// (weights_host.hpp), the workspace and the launch sequences of codec_kernels.hpp.  A handle of its own: the codec has its own
// weights and lifetime and runs without a VALL-E engine.  Its device side (CodecDev: one packed weight block, one DevBuf per
// workspace buffer, the CallStage of a call's tables) is made as a whole by vx_codec_finalize on vx_codec_config.device and dropped
// as a whole; the work runs on the handle's own stream between ev_in and ev_out.
// At the end of the file: the sample-rate converter in front of the encoder (vx_resampler_*), a handle without weights on
// host.hpp's LazyDev, its ragged calls staged through CallStage too.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "weights_host.hpp"
#include "codec_kernels.hpp"

using namespace vx;

namespace {

// ---- weight packing (host): torch layouts -> the [N][K] operands of codec_gemm_rows; a convolution (O, C, k) is conv_rows -----------
// Every tensor starts at a multiple of 256 bytes of its packed block, which is what a hipMalloc of its own used to give it: the
// float4 loads and the cache-line layout of the weight rows see the alignment they always saw.
constexpr size_t CODEC_ALIGN = 64;  // floats
// Every device block ends in 16 spare bytes, as it has since the first codec.  No load of codec_kernels.hpp needs them:
// codec_gemm_rows guards every operand read by row < M, n < N and k < K, and takes float4 only where every part's C, and so K, is a
// multiple of 16; codec_lstm_step reads i * 64 + lane < ldw of whole gate rows; codec_conv_out takes float4 only when C % 4 == 0;
// codec_rvq_encode reads whole codebook rows (the host checks S % 32 == 0, D % 8 == 0); the per-element kernels leave at
// i >= rows * dim.  Kept as the margin they always were.
constexpr size_t CODEC_SPARE = 4;  // floats

// Offsets (floats) into a packed block.
struct ConvW { size_t w = 0, b = 0; };
struct ResW { ConvW c3, mix; };  // block.1: ch -> ch / 2, k = res_kernel; [block.3 | shortcut]: K = ch / 2 + ch, bias = sum of the two
struct LstmW { size_t wih0 = 0, b0 = 0, whh0 = 0, w1 = 0, b1 = 0; };

size_t put(std::vector<float>& p, const std::vector<float>& v) { return push(p, v, CODEC_ALIGN); }

// transposed conv (Cin, Cout, 2s), stride s: row n = r * Cout + co; k < Cin: x[t-1] with W[ci][co][r + s]; then x[t] with W[ci][co][r];
// the bias repeated per phase
ConvW pack_convtr(std::vector<float>& p, const float* w, const float* bias, int Cin, int Cout, int s) {
  std::vector<float> pk((size_t)s * Cout * 2 * Cin), rep;
  for (int r = 0; r < s; ++r)
    for (int co = 0; co < Cout; ++co)
      for (int ci = 0; ci < Cin; ++ci) {
        const size_t n = (size_t)r * Cout + co;
        pk[n * 2 * Cin + ci] = w[((size_t)ci * Cout + co) * 2 * s + r + s];
        pk[n * 2 * Cin + Cin + ci] = w[((size_t)ci * Cout + co) * 2 * s + r];
      }
  for (int r = 0; bias && r < s; ++r) rep.insert(rep.end(), bias, bias + Cout);
  ConvW cv;
  cv.w = put(p, pk);
  cv.b = put(p, rep);
  return cv;
}

ConvW pack_conv(std::vector<float>& p, const float* w, const float* bias, int O, int Cc, int k) {
  ConvW cv;
  cv.w = put(p, conv_rows(w, O, Cc, k));
  cv.b = put(p, bias ? std::vector<float>(bias, bias + O) : std::vector<float>());
  return cv;
}

// LSTM weights (torch layouts) -> W_ih0, W_hh0, b_ih0 + b_hh0, [W_ih1 | W_hh1], b_ih1 + b_hh1
LstmW pack_lstm(std::vector<float>& p, const float* const* wih, const float* const* whh, const float* const* bih, const float* const* bhh,
                int H, int layers) {
  LstmW d;
  std::vector<float> b0(4 * H);
  for (int i = 0; i < 4 * H; ++i) b0[i] = bih[0][i] + bhh[0][i];
  d.wih0 = put(p, std::vector<float>(wih[0], wih[0] + (size_t)4 * H * H));
  d.whh0 = put(p, std::vector<float>(whh[0], whh[0] + (size_t)4 * H * H));
  d.b0 = put(p, b0);
  if (layers == 2) {
    std::vector<float> w1((size_t)4 * H * 2 * H), b1(4 * H);
    for (int n = 0; n < 4 * H; ++n) {
      memcpy(&w1[(size_t)n * 2 * H], wih[1] + (size_t)n * H, H * sizeof(float));
      memcpy(&w1[(size_t)n * 2 * H + H], whh[1] + (size_t)n * H, H * sizeof(float));
      b1[n] = bih[1][n] + bhh[1][n];
    }
    d.w1 = put(p, w1);
    d.b1 = put(p, b1);
  }
  return d;
}

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

// A packed block goes to the device in one blocking copy.
int upload_packed(const std::vector<float>& p, DevBuf<float>& d) {
  VXC(d.alloc(p.size() + CODEC_SPARE));
  HIPC(hipMemcpy(d.get(), p.data(), p.size() * sizeof(float), hipMemcpyHostToDevice));
  return VX_OK;
}

// ---- launches --------------------------------------------------------------------------------------------------------
template <bool STRIDED = false>
int launch_gemm(const CodecGemmArgs& a, hipStream_t s) {
  bool vec = true;
  for (int p = 0; p < a.nparts; ++p) vec = vec && (a.part[p].C % 16 == 0);
  if (a.M <= 0) return VX_OK;
  if (a.N <= 32) {
    dim3 g((unsigned)((a.M + 127) / 128), (unsigned)((a.N + 31) / 32));
    if (vec) codec_gemm_rows<4, 1, true, STRIDED><<<g, 256, 0, s>>>(a);
    else codec_gemm_rows<4, 1, false, STRIDED><<<g, 256, 0, s>>>(a);
  } else {
    dim3 g((unsigned)((a.M + 63) / 64), (unsigned)((a.N + 63) / 64));
    if (vec) codec_gemm_rows<2, 2, true, STRIDED><<<g, 256, 0, s>>>(a);
    else codec_gemm_rows<2, 2, false, STRIDED><<<g, 256, 0, s>>>(a);
  }
  HIPC(hipGetLastError());
  return VX_OK;
}

// causal k-tap convolution over rows (reflect rule); wp packed by conv_rows.  c_out == 1 runs the bandwidth kernel.
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
// wp packed by conv_rows
int run_conv_strided(const float* x, const float* wp, const float* bias, float* out, long M_out, int cin, int cout, int stride, int elu,
                     const int* seg_out, const int* seg_in, int nseg, hipStream_t s) {
  CodecGemmArgs a{};
  a.part[0] = CodecPart{x, cin, 2 * stride, CODEC_PAD_REFLECT, elu};
  a.nparts = 1;
  a.W = wp; a.bias = bias; a.out = out; a.M = M_out; a.N = cout; a.K = 2 * stride * cin; a.seg = seg_out; a.nseg = nseg; a.rate = 1;
  a.seg_in = seg_in; a.stride = stride;
  return launch_gemm<true>(a, s);
}

// residual block over M rows of `x` (ch channels): h = block.1(ELU(x)); out = [block.3 | shortcut] over [ELU(h) ; x]
int run_res(const float* W, const ResW& r, const float* x, float* h, float* out, long M, int ch, int res_kernel, const int* seg, int nseg,
            int rate, hipStream_t s) {
  const int hd = ch / 2;
  VXC(run_conv(x, W + r.c3.w, W + r.c3.b, h, M, ch, hd, res_kernel, 1, seg, nseg, rate, s));
  CodecGemmArgs a{};
  a.part[0] = CodecPart{h, hd, 1, CODEC_PAD_ZERO, 1};
  a.part[1] = CodecPart{x, ch, 1, CODEC_PAD_ZERO, 0};
  a.nparts = 2;
  a.W = W + r.mix.w; a.bias = W + r.mix.b; a.out = out; a.M = M; a.N = ch; a.K = hd + ch; a.seg = seg; a.nseg = nseg; a.rate = rate;
  return launch_gemm(a, s);
}

bool rvq_shape_ok(int S, int D) { return S >= 32 && S % 32 == 0 && D >= 8 && D % 8 == 0 && D <= CODEC_RVQ_MAX_D; }

int run_rvq_encode(const float* emb, const float* cb, const float* cb_sq, int* codes, long rows, int n_q, int S, int D, hipStream_t s) {
  if (rows > 0) codec_rvq_encode<<<(unsigned)((rows + CODEC_RVQ_ROWS - 1) / CODEC_RVQ_ROWS), 256, 0, s>>>(emb, cb, cb_sq, codes, rows, n_q, S, D);
  HIPC(hipGetLastError());
  return VX_OK;
}

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

// x [rows][H] -> y = lstm(x) + x; W + w: the packed weights; gin [rows][4H], h0 / h1 [rows][H], c0 / c1 [nseg][H] are workspace.
// chain == nullptr: one plain launch per step.  Otherwise the steps are replayed as a captured LINEAR chain of CODEC_LSTM_CHAIN step
// launches and one node that advances the step counter: `meta` (device {nseg, step}) was written by the caller, *chain is captured on
// first use (s must not be the null stream) and serves every batch and length of the handle.
int run_lstm(const float* W, const LstmW& w, const float* x, float* gin, float* h0, float* h1, float* c0, float* c1, float* y, int H,
             int layers, const int* seg_dev, const int* seg_host, int nseg, hipStream_t s, hipGraphExec_t* chain = nullptr,
             int* meta = nullptr) {
  const long rows = seg_host[nseg];
  int Tmax = 0;
  for (int b = 0; b < nseg; ++b) Tmax = std::max(Tmax, seg_host[b + 1] - seg_host[b]);
  CodecGemmArgs g{};
  g.part[0] = CodecPart{x, H, 1, CODEC_PAD_ZERO, 0};
  g.nparts = 1;
  g.W = W + w.wih0; g.bias = W + w.b0; g.out = gin; g.M = rows; g.N = 4 * H; g.K = H; g.seg = seg_dev; g.nseg = nseg; g.rate = 1;
  VXC(launch_gemm(g, s));
  CodecLstmArgs a{};
  a.gin0 = gin; a.whh0 = W + w.whh0; a.xin = x; a.h0 = h0; a.h1 = h1; a.y = y; a.c0 = c0; a.c1 = c1;
  if (layers == 2) { a.w1 = W + w.w1; a.b1 = W + w.b1; }
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

int check_segs(const int32_t* seg, int nseg) {
  if (!seg || nseg < 1 || nseg > CODEC_MAX_SEG) return fail(VX_ERR_ARG, "segments: 1..%d expected, got %d", CODEC_MAX_SEG, nseg);
  if (seg[0] != 0) return fail(VX_ERR_ARG, "segment starts begin at 0");
  for (int i = 0; i < nseg; ++i)
    if (seg[i + 1] <= seg[i]) return fail(VX_ERR_ARG, "segment %d is empty or starts are not increasing", i);
  return VX_OK;
}

struct Stage {  // decoder: cin -> cout = cin / 2 at `stride`
  int cin, cout, stride;
  ConvW up;  // transposed convolution
  ResW res;
};

struct EncStage {  // encoder: c -> 2c at `stride`
  int c, stride;
  ResW res;
  ConvW dn;  // strided convolution
};

// The device side of a finalised handle: made as a whole by vx_codec_finalize, freed as a whole on every way out.
struct CodecDev {
  hipStream_t own = nullptr;  // the codec's stream (the LSTM chain cannot be captured on the null stream)
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  hipGraphExec_t chain = nullptr;
  DevBuf<float> w;  // every packed tensor
  DevBuf<float> x0, xc, gin, h0, h1, y, c0, c1, bufA, bufH, bufB, wav;  // workspace; wav: the encoder's samples of one group
  // per call: the encoder's output pointers [max_batch] (encoder handles) | int32 {nseg, step} | frame offsets [max_batch + 1] |
  // per-group relative offsets [2 (max_batch + 1)] | decode: codes [n_q][frames]; encode: four more row tables per group
  // [4][2 (max_batch + 1)], then (device only) codes [n_q][frames]
  CallStage stage;
  CodecDev() = default;
  CodecDev(const CodecDev&) = delete;
  CodecDev& operator=(const CodecDev&) = delete;
  ~CodecDev() {
    if (chain) (void)hipGraphExecDestroy(chain);
    for (hipEvent_t ev : {ev_in, ev_out})
      if (ev) (void)hipEventDestroy(ev);
    if (own) (void)hipStreamDestroy(own);
  }
};

}  // namespace

struct vx_codec {
  vx_codec_config cfg{};
  int W = 0;  // LSTM width = 16 * filters
  std::map<std::string, HostW> w;
  bool finalized = false;  // the device side is complete: set as vx_codec_finalize's last statement
  bool failed = false;     // a finalize failed half way: the handle refuses further use
  std::unique_ptr<CodecDev> dev;
  // offsets into dev->w
  size_t cb = 0;  // [n_codebooks][size][dim]
  ConvW c0, last;
  LstmW lstm;
  std::vector<Stage> stages;
  long cap_frames = 0, chunk_frames = 0, per_frame = 0;
  size_t ptr_bytes = 0;  // of the stage's pointer column
  // encoder (VX_CODEC_ENCODER)
  bool enc = false;
  size_t cb_sq = 0;  // [n_codebooks][size]
  ConvW e0, elast;
  LstmW elstm;
  std::vector<EncStage> estages;
  long last_frames = 0;  // frames of the last vx_codec_encode (what x0 holds of it)
};

namespace {

void conv_keys(vx_codec* e, const std::string& nm, int64_t O, int64_t Cc, int64_t k) {
  add_key(e, nm + ".weight", {O, Cc, k});
  add_key(e, nm + ".bias", {O});
}

void res_keys(vx_codec* e, const std::string& pre, int64_t ch) {
  conv_keys(e, pre + "block.1.conv", ch / 2, ch, e->cfg.res_kernel);
  conv_keys(e, pre + "block.3.conv", ch, ch / 2, 1);
  conv_keys(e, pre + "shortcut.conv", ch, ch, 1);
}

void lstm_keys(vx_codec* e, const std::string& pre) {
  const int64_t W = e->W;
  for (int l = 0; l < e->cfg.lstm_layers; ++l) {
    const std::string sl = "_l" + std::to_string(l);
    add_key(e, pre + "weight_ih" + sl, {4 * W, W});
    add_key(e, pre + "weight_hh" + sl, {4 * W, W});
    add_key(e, pre + "bias_ih" + sl, {4 * W});
    add_key(e, pre + "bias_hh" + sl, {4 * W});
  }
}

std::string layer(const char* side, int i) { return std::string(side) + ".layers." + std::to_string(i) + "."; }

void codec_add_keys(vx_codec* e) {
  const vx_codec_config& c = e->cfg;
  const int64_t W = e->W;
  conv_keys(e, "decoder.layers.0.conv", W, c.hidden, c.kernel);
  lstm_keys(e, "decoder.layers.1.lstm.");
  int64_t ch = W;
  for (int i = 0; i < 4; ++i) {
    add_key(e, layer("decoder", 3 + 3 * i) + "conv.weight", {ch, ch / 2, 2 * (int64_t)c.ratios[i]});
    add_key(e, layer("decoder", 3 + 3 * i) + "conv.bias", {ch / 2});
    ch /= 2;
    res_keys(e, layer("decoder", 4 + 3 * i), ch);
  }
  conv_keys(e, "decoder.layers.15.conv", 1, ch, c.last_kernel);
  for (int q = 0; q < c.n_codebooks; ++q) add_key(e, layer("quantizer", q) + "codebook.embed", {c.codebook_size, c.codebook_dim});
  if (!(c.flags & VX_CODEC_ENCODER)) return;
  ch = c.filters;
  conv_keys(e, "encoder.layers.0.conv", ch, 1, c.kernel);
  for (int i = 0; i < 4; ++i) {
    res_keys(e, layer("encoder", 1 + 3 * i), ch);
    conv_keys(e, layer("encoder", 3 + 3 * i) + "conv", 2 * ch, ch, 2 * (int64_t)c.ratios[3 - i]);
    ch *= 2;
  }
  lstm_keys(e, "encoder.layers.13.lstm.");
  conv_keys(e, "encoder.layers.15.conv", c.hidden, W, c.last_kernel);
}

const float* host(vx_codec* e, const std::string& key) { return e->w[key].data.data(); }

ConvW pack_conv(vx_codec* e, std::vector<float>& p, const std::string& nm, int O, int Cc, int k) {
  return pack_conv(p, host(e, nm + ".weight"), host(e, nm + ".bias"), O, Cc, k);
}

// One residual stage of ch channels by its key prefix ("decoder.layers.4."): block.1 and [block.3 | shortcut]
ResW pack_res(vx_codec* e, std::vector<float>& p, const std::string& pre, int ch) {
  const int hd = ch / 2;
  ResW r;
  r.c3 = pack_conv(e, p, pre + "block.1.conv", hd, ch, e->cfg.res_kernel);
  const float *w3 = host(e, pre + "block.3.conv.weight"), *ws = host(e, pre + "shortcut.conv.weight");
  const float *b3 = host(e, pre + "block.3.conv.bias"), *bs = host(e, pre + "shortcut.conv.bias");
  std::vector<float> mix((size_t)ch * (hd + ch)), mb(ch);
  for (int n = 0; n < ch; ++n) {
    memcpy(&mix[(size_t)n * (hd + ch)], w3 + (size_t)n * hd, hd * sizeof(float));
    memcpy(&mix[(size_t)n * (hd + ch) + hd], ws + (size_t)n * ch, ch * sizeof(float));
    mb[n] = b3[n] + bs[n];
  }
  r.mix.w = put(p, mix);
  r.mix.b = put(p, mb);
  return r;
}

// An LSTM's four tensors per layer by its key prefix ("decoder.layers.1.lstm.")
LstmW pack_lstm(vx_codec* e, std::vector<float>& p, const std::string& pre) {
  const float *wih[2] = {}, *whh[2] = {}, *bih[2] = {}, *bhh[2] = {};
  for (int l = 0; l < e->cfg.lstm_layers; ++l) {
    const std::string sl = "_l" + std::to_string(l);
    wih[l] = host(e, pre + "weight_ih" + sl);
    whh[l] = host(e, pre + "weight_hh" + sl);
    bih[l] = host(e, pre + "bias_ih" + sl);
    bhh[l] = host(e, pre + "bias_hh" + sl);
  }
  return pack_lstm(p, wih, whh, bih, bhh, e->W, e->cfg.lstm_layers);
}

// Every tensor of the handle into `p`; the offsets into the handle.  Returns the widest decoder stage's floats per frame.
long codec_pack(vx_codec* e, std::vector<float>& p) {
  const vx_codec_config& c = e->cfg;
  const int W = e->W;
  std::vector<float> cb, sq;
  for (int q = 0; q < c.n_codebooks; ++q) {
    const HostW& t = e->w[layer("quantizer", q) + "codebook.embed"];
    cb.insert(cb.end(), t.data.begin(), t.data.end());
    const std::vector<float> one = codebook_sq(t.data.data(), (size_t)c.codebook_size, c.codebook_dim);
    sq.insert(sq.end(), one.begin(), one.end());
  }
  e->cb = put(p, cb);
  e->c0 = pack_conv(e, p, "decoder.layers.0.conv", W, c.hidden, c.kernel);
  e->lstm = pack_lstm(e, p, "decoder.layers.1.lstm.");
  int ch = W;
  long rate = 1, per_frame = 0;
  e->stages.resize(4);
  for (int i = 0; i < 4; ++i) {
    Stage& st = e->stages[i];
    const std::string up = layer("decoder", 3 + 3 * i) + "conv";
    st.cin = ch; st.cout = ch / 2; st.stride = c.ratios[i];
    st.up = pack_convtr(p, host(e, up + ".weight"), host(e, up + ".bias"), ch, ch / 2, st.stride);
    ch /= 2;
    rate *= st.stride;
    per_frame = std::max(per_frame, rate * ch);
    st.res = pack_res(e, p, layer("decoder", 4 + 3 * i), ch);
  }
  e->last = pack_conv(e, p, "decoder.layers.15.conv", 1, ch, c.last_kernel);
  if (!e->enc) return per_frame;
  e->cb_sq = put(p, sq);
  e->e0 = pack_conv(e, p, "encoder.layers.0.conv", c.filters, 1, c.kernel);
  int ec = c.filters;
  e->estages.resize(4);
  for (int i = 0; i < 4; ++i) {
    EncStage& st = e->estages[i];
    st.c = ec; st.stride = c.ratios[3 - i];
    st.res = pack_res(e, p, layer("encoder", 1 + 3 * i), ec);
    st.dn = pack_conv(e, p, layer("encoder", 3 + 3 * i) + "conv", 2 * ec, ec, 2 * st.stride);
    ec *= 2;
  }
  e->elstm = pack_lstm(e, p, "encoder.layers.13.lstm.");
  e->elast = pack_conv(e, p, "encoder.layers.15.conv", c.hidden, W, c.last_kernel);
  return per_frame;
}

// ---- the common head of vx_codec_decode and vx_codec_encode -------------------------------------------------------------------------
struct Group { int u0, u1, off; };  // utterances [u0, u1); `off`: where the group's relative offsets start in their table

struct Call {
  hipStream_t s = nullptr;
  std::vector<int> seg;       // host: the n + 1 frame offsets of the call
  std::vector<Group> groups;  // whole utterances of at most chunk_frames frames together: the rows of the sample-rate stages
  int* meta = nullptr;        // device: {nseg, step}
  const int *dseg = nullptr, *drel = nullptr;  // device: frame offsets of the call; per group, relative to the group
  int* rest = nullptr;        // device: what `fill` wrote, and the block's unstaged end behind it
};

// The work runs on the codec's own stream, ordered after everything already enqueued on `stream`; `stream` waits for it before the
// call returns (as the engine's entry points do).  The host waits only for the previous call's staging copy.  `frames`: per utterance;
// fill(host ints behind the three tables) writes the call's own rest_ints, after seg and groups are known.
template <class Fill>
int begin_call(vx_codec* e, int n, const std::vector<int>& frames, void* stream, size_t rest_ints, Fill fill, Call& x) {
  CodecDev& d = *e->dev;
  x.s = d.own;
  HIPC(hipEventRecord(d.ev_in, (hipStream_t)stream));
  HIPC(hipStreamWaitEvent(x.s, d.ev_in, 0));
  VXC(d.stage.begin(x.s));
  const int MB1 = e->cfg.max_batch + 1;
  int* hc = d.stage.host<int>(e->ptr_bytes);
  hc[0] = n;
  hc[1] = 0;
  int *hseg = hc + 2, *hrel = hseg + MB1;
  x.seg.assign(n + 1, 0);
  for (int i = 0; i < n; ++i) x.seg[i + 1] = x.seg[i] + frames[i];
  memcpy(hseg, x.seg.data(), (n + 1) * sizeof(int));
  int used = 0;
  for (int u0 = 0; u0 < n;) {
    int u1 = u0 + 1;
    while (u1 < n && (long)x.seg[u1 + 1] - x.seg[u0] <= e->chunk_frames) ++u1;
    x.groups.push_back(Group{u0, u1, used});
    for (int u = u0; u <= u1; ++u) hrel[used++] = x.seg[u] - x.seg[u0];
    u0 = u1;
  }
  fill(hrel + 2 * MB1);
  VXC(d.stage.upload(e->ptr_bytes + (2 + 3 * (size_t)MB1 + rest_ints) * sizeof(int), x.s));
  x.meta = d.stage.dev<int>(e->ptr_bytes);
  x.dseg = x.meta + 2;
  x.drel = x.dseg + MB1;
  x.rest = x.meta + 2 + 3 * MB1;
  return VX_OK;
}

// `stream` waits for the call's work.
int end_call(vx_codec* e, const Call& x, void* stream) {
  HIPC(hipEventRecord(e->dev->ev_out, x.s));
  HIPC(hipStreamWaitEvent((hipStream_t)stream, e->dev->ev_out, 0));
  return e->dev->stage.finish(x.s);
}

}  // namespace

extern "C" int vx_codec_create(const vx_codec_config* cfg, vx_codec** out) {
  VXC(create_head("vx_codec_create", cfg, out));
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
  e->enc = (c.flags & VX_CODEC_ENCODER) != 0;
  codec_add_keys(e);
  *out = e;
  return VX_OK;
}

extern "C" void vx_codec_destroy(vx_codec* e) {
  if (!e) return;
  if (e->dev) {
    DevGuard g(e->cfg.device);
    (void)hipStreamSynchronize(e->dev->own);
    e->dev.reset();
  }
  delete e;
}

extern "C" int vx_codec_set_weight(vx_codec* e, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
  return set_weight(e, "vx_codec", key, data, shape, ndim);
}

extern "C" int vx_codec_finalize(vx_codec* e) {
  if (!e) return fail(VX_ERR_ARG, "vx_codec_finalize: null handle");
  if (e->finalized) return VX_OK;
  if (e->failed) return fail(VX_ERR_STATE, "vx_codec_finalize failed earlier on this handle: destroy it and create a new one");
  VXC(missing_tensor(e));
  const vx_codec_config& c = e->cfg;
  e->failed = true;  // until the last statement: a finalize that stops at a HIP error leaves a handle that refuses further use
  ON_DEVICE(c.device);
  std::unique_ptr<CodecDev> d(new CodecDev());  // a finalize that stops half way frees what it took
  const int W = e->W;
  long rate = 1;
  for (int i = 0; i < 4; ++i) rate *= c.ratios[i];
  {
    std::vector<float> packed;
    e->per_frame = std::max<long>(codec_pack(e, packed), 2 * rate);
    VXC(upload_packed(packed, d->w));
  }
  for (auto& kv : e->w) std::vector<float>().swap(kv.second.data);  // the host copies are not needed any more

  // workspace: the LSTM part holds every frame of a call; the up-sampling part runs over groups of whole utterances of at
  // most chunk_frames frames (its rows are 320x as many)
  e->cap_frames = (long)c.max_frames * c.max_batch;
  e->chunk_frames = std::min(e->cap_frames, std::max<long>(c.max_frames, 8192));
  const size_t F = (size_t)e->cap_frames, MB1 = (size_t)c.max_batch + 1;
  VXC(d->x0.alloc(F * c.hidden + CODEC_SPARE));
  VXC(d->xc.alloc(F * W + CODEC_SPARE));
  VXC(d->gin.alloc(F * 4 * W + CODEC_SPARE));
  VXC(d->h0.alloc(F * W + CODEC_SPARE));
  VXC(d->h1.alloc(F * W + CODEC_SPARE));
  VXC(d->y.alloc(F * W + CODEC_SPARE));
  VXC(d->c0.alloc((size_t)c.max_batch * W + CODEC_SPARE));
  VXC(d->c1.alloc((size_t)c.max_batch * W + CODEC_SPARE));
  // encoder: the same three buffers hold its stages (filters channels per sample at most, as the decoder's last stage), plus one
  // row per utterance and stage for the rounded-up row counts
  const size_t slack = e->enc ? (size_t)c.max_batch * W : 0, rows = (size_t)e->chunk_frames * e->per_frame;
  VXC(d->bufA.alloc(rows + slack + CODEC_SPARE));
  VXC(d->bufB.alloc(rows + slack + CODEC_SPARE));
  VXC(d->bufH.alloc(rows / 2 + slack + CODEC_SPARE));
  if (e->enc) VXC(d->wav.alloc((size_t)e->chunk_frames * rate + CODEC_SPARE));
  e->ptr_bytes = e->enc ? (size_t)c.max_batch * sizeof(void*) : 0;
  VXC(d->stage.init(e->ptr_bytes + (2 + 3 * MB1 + (e->enc ? 8 * MB1 : 0) + F * c.n_codebooks) * sizeof(int)));
  HIPC(hipStreamCreateWithFlags(&d->own, hipStreamNonBlocking));
  HIPC(hipEventCreateWithFlags(&d->ev_in, hipEventDisableTiming));
  HIPC(hipEventCreateWithFlags(&d->ev_out, hipEventDisableTiming));
  e->dev = std::move(d);
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
  CodecDev& d = *e->dev;
  const float* Wt = d.w.get();
  const int W = e->W;
  Call x;
  VXC(begin_call(e, n, std::vector<int>(T, T + n), stream, (size_t)n_q * total, [&](int* hcodes) {
    for (int i = 0; i < n; ++i)
      for (int q = 0; q < n_q; ++q)
        for (int t = 0; t < T[i]; ++t) hcodes[(size_t)q * total + x.seg[i] + t] = (int)codes[i][(size_t)q * T[i] + t];
  }, x));
  hipStream_t s = x.s;
  const std::vector<int>& seg = x.seg;

  const long e0 = total * c.hidden;
  e->last_frames = 0;  // x0 no longer holds an encode's embeddings
  codec_rvq_rows<<<(unsigned)((e0 + 255) / 256), 256, 0, s>>>(x.rest, Wt + e->cb, d.x0.get(), total, n_q, c.codebook_size, c.codebook_dim);
  HIPC(hipGetLastError());
  VXC(run_conv(d.x0.get(), Wt + e->c0.w, Wt + e->c0.b, d.xc.get(), total, c.hidden, W, c.kernel, 0, x.dseg, n, 1, s));
  VXC(run_lstm(Wt, e->lstm, d.xc.get(), d.gin.get(), d.h0.get(), d.h1.get(), d.c0.get(), d.c1.get(), d.y.get(), W, c.lstm_layers, x.dseg,
                seg.data(), n, s, (c.flags & VX_CODEC_LSTM_GRAPH) ? &d.chain : nullptr, x.meta));

  for (const Group& gr : x.groups) {
    const int ns = gr.u1 - gr.u0;
    const int* sg = x.drel + gr.off;
    const long frames = seg[gr.u1] - seg[gr.u0];
    const float* in = d.y.get() + (size_t)seg[gr.u0] * W;
    long rate = 1;
    for (const Stage& st : e->stages) {
      VXC(run_convtr(in, Wt + st.up.w, Wt + st.up.b, d.bufA.get(), frames * rate, st.cin, st.cout, st.stride, 1, sg, ns, (int)rate, s));
      rate *= st.stride;
      VXC(run_res(Wt, st.res, d.bufA.get(), d.bufH.get(), d.bufB.get(), frames * rate, st.cout, c.res_kernel, sg, ns, (int)rate, s));
      in = d.bufB.get();
    }
    const int ch = e->stages.back().cout;
    VXC(run_conv(d.bufB.get(), Wt + e->last.w, Wt + e->last.b, d.bufH.get(), frames * rate, ch, 1, c.last_kernel, 1, sg, ns, (int)rate, s));
    for (int u = gr.u0; u < gr.u1; ++u)
      HIPC(hipMemcpyAsync(wav_out[u], d.bufH.get() + (size_t)(seg[u] - seg[gr.u0]) * rate, (size_t)T[u] * rate * sizeof(float),
                           hipMemcpyDeviceToDevice, s));
  }
  return end_call(e, x, stream);
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
  CodecDev& d = *e->dev;
  const float* Wt = d.w.get();
  const int W = e->W, MB1 = c.max_batch + 1;
  auto cdiv = [](long a, long b) { return (a + b - 1) / b; };
  std::vector<int> frames(n);
  for (int i = 0; i < n; ++i) frames[i] = (int)cdiv(n_samples[i], hop);
  std::vector<std::array<long, 5>> rows;  // per group: its rows at stages 0..3 and its frames
  Call x;
  // behind the three tables: per stage 0..3 the groups' row offsets [4][2 MB1] (the frames' relative offsets are stage 4's)
  VXC(begin_call(e, n, frames, stream, 8 * (size_t)MB1, [&](int* hlv) {
    for (const Group& gr : x.groups) {
      std::array<long, 5> acc = {0, 0, 0, 0, 0};
      for (int u = gr.u0; u <= gr.u1; ++u) {
        for (int l = 0; l < 4; ++l) hlv[l * 2 * MB1 + gr.off + u - gr.u0] = (int)acc[l];
        if (u == gr.u1) break;
        long r = n_samples[u];
        acc[0] += r;
        for (int l = 0; l < 4; ++l) acc[l + 1] += (r = cdiv(r, e->estages[l].stride));
      }
      rows.push_back(acc);
    }
    long long** hp = d.stage.host<long long*>();  // the utterances' output tensors
    for (int i = 0; i < n; ++i) hp[i] = (long long*)codes_out[i];
  }, x));
  hipStream_t s = x.s;
  const std::vector<int>& seg = x.seg;
  const long total = seg[n];
  const int* dlv = x.rest;
  int* dcodes = x.rest + 8 * MB1;  // [n_q][total]

  for (size_t gi = 0; gi < x.groups.size(); ++gi) {
    const Group& gr = x.groups[gi];
    const int ns = gr.u1 - gr.u0;
    const int* sg[5] = {dlv + gr.off, dlv + 2 * MB1 + gr.off, dlv + 4 * MB1 + gr.off, dlv + 6 * MB1 + gr.off, x.drel + gr.off};
    long off = 0;
    for (int u = gr.u0; u < gr.u1; ++u) {
      HIPC(hipMemcpyAsync(d.wav.get() + off, wav[u], (size_t)n_samples[u] * sizeof(float), hipMemcpyDeviceToDevice, s));
      off += n_samples[u];
    }
    VXC(run_conv_in(d.wav.get(), Wt + e->e0.w, Wt + e->e0.b, d.bufA.get(), rows[gi][0], c.filters, c.kernel, sg[0], ns, s));
    for (int l = 0; l < 4; ++l) {
      const EncStage& st = e->estages[l];
      VXC(run_res(Wt, st.res, d.bufA.get(), d.bufH.get(), d.bufB.get(), rows[gi][l], st.c, c.res_kernel, sg[l], ns, 1, s));
      float* out = l == 3 ? d.xc.get() + (size_t)seg[gr.u0] * W : d.bufA.get();
      VXC(run_conv_strided(d.bufB.get(), Wt + st.dn.w, Wt + st.dn.b, out, rows[gi][l + 1], st.c, 2 * st.c, st.stride, 1, sg[l + 1], sg[l], ns, s));
    }
  }
  VXC(run_lstm(Wt, e->elstm, d.xc.get(), d.gin.get(), d.h0.get(), d.h1.get(), d.c0.get(), d.c1.get(), d.y.get(), W, c.lstm_layers, x.dseg,
                seg.data(), n, s));
  e->last_frames = 0;
  VXC(run_conv(d.y.get(), Wt + e->elast.w, Wt + e->elast.b, d.x0.get(), total, W, c.hidden, c.last_kernel, 1, x.dseg, n, 1, s));
  e->last_frames = total;
  VXC(run_rvq_encode(d.x0.get(), Wt + e->cb, Wt + e->cb_sq, dcodes, total, n_q, c.codebook_size, c.codebook_dim, s));
  const long nc = total * n_q;
  codec_codes_out<<<(unsigned)((nc + 255) / 256), 256, 0, s>>>(dcodes, d.stage.dev<long long* const>(), x.dseg, n, total, n_q);
  HIPC(hipGetLastError());
  return end_call(e, x, stream);
}

// The embeddings (the quantiser's input, [rows][hidden]) of the last vx_codec_encode, rows in the order of its utterances: copied to
// `out` (device) on the codec's stream, `stream` ordered after it.  For the parity tests.
extern "C" int vx_codec_last_embeddings(vx_codec* e, float* out, int64_t rows, void* stream) {
  if (!e || !out) return fail(VX_ERR_ARG, "vx_codec_last_embeddings: null argument");
  if (!(e->cfg.flags & VX_CODEC_ENCODER) || !e->finalized) return fail(VX_ERR_STATE, "vx_codec_last_embeddings: no finalised encoder");
  if (rows < 1 || rows > e->last_frames)
    return fail(VX_ERR_ARG, "vx_codec_last_embeddings: rows = %lld, the last encode had %ld frames", (long long)rows, e->last_frames);
  ON_DEVICE(e->cfg.device);
  CodecDev& d = *e->dev;
  HIPC(hipMemcpyAsync(out, d.x0.get(), (size_t)rows * e->cfg.hidden * sizeof(float), hipMemcpyDeviceToDevice, d.own));
  HIPC(hipEventRecord(d.ev_out, d.own));
  HIPC(hipStreamWaitEvent((hipStream_t)stream, d.ev_out, 0));
  return VX_OK;
}

// ---- op-level test entries: x / out device fp32 rows, weights and biases HOST fp32 in torch's layouts (packed here by the helpers
// vx_codec_finalize packs with), seg_frames HOST nseg + 1 frame offsets.  Synchronous. ------------------------------------------------
namespace {
int upload_segs(const int32_t* seg, int nseg, DevBuf<int>& d) {
  VXC(d.alloc(nseg + 1));
  HIPC(hipMemcpy(d.get(), seg, (nseg + 1) * sizeof(int), hipMemcpyHostToDevice));
  return VX_OK;
}
}  // namespace

extern "C" int vx_op_codec_conv(const float* x, const float* w, const float* bias, float* out, int32_t c_in, int32_t c_out, int32_t k,
                                int32_t elu, int32_t nseg, const int32_t* seg_frames, int32_t rate, void* stream) {
  if (!x || !w || !out || c_in < 1 || c_out < 1 || k < 1 || k > 15 || rate < 1) return fail(VX_ERR_ARG, "vx_op_codec_conv: bad argument");
  VXC(check_segs(seg_frames, nseg));
  hipStream_t s = (hipStream_t)stream;
  DevBuf<int> sg;
  DevBuf<float> W;
  std::vector<float> p;
  const ConvW cv = pack_conv(p, w, bias, c_out, c_in, k);
  VXC(upload_segs(seg_frames, nseg, sg));
  VXC(upload_packed(p, W));
  VXC(run_conv(x, W.get() + cv.w, bias ? W.get() + cv.b : nullptr, out, (long)seg_frames[nseg] * rate, c_in, c_out, k, elu, sg.get(), nseg, rate, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

extern "C" int vx_op_codec_convtr(const float* x, const float* w, const float* bias, float* out, int32_t c_in, int32_t c_out,
                                  int32_t stride, int32_t elu, int32_t nseg, const int32_t* seg_frames, int32_t rate, void* stream) {
  if (!x || !w || !out || c_in < 1 || c_out < 1 || stride < 1 || rate < 1) return fail(VX_ERR_ARG, "vx_op_codec_convtr: bad argument");
  VXC(check_segs(seg_frames, nseg));
  hipStream_t s = (hipStream_t)stream;
  DevBuf<int> sg;
  DevBuf<float> W;
  std::vector<float> p;
  const ConvW cv = pack_convtr(p, w, bias, c_in, c_out, stride);
  VXC(upload_segs(seg_frames, nseg, sg));
  VXC(upload_packed(p, W));
  VXC(run_convtr(x, W.get() + cv.w, bias ? W.get() + cv.b : nullptr, out, (long)seg_frames[nseg] * rate, c_in, c_out, stride, elu, sg.get(), nseg, rate, s));
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
  DevBuf<float> W, gin, h0, h1, c0, c1;
  std::vector<float> p;
  const LstmW lw = pack_lstm(p, w_ih, w_hh, b_ih, b_hh, width, layers);
  const size_t rows = seg_frames[nseg];
  VXC(upload_segs(seg_frames, nseg, sg));
  VXC(upload_packed(p, W));
  VXC(gin.alloc(rows * 4 * width + CODEC_SPARE));
  VXC(h0.alloc(rows * width + CODEC_SPARE));
  VXC(h1.alloc(rows * width + CODEC_SPARE));
  VXC(c0.alloc((size_t)nseg * width + CODEC_SPARE));
  VXC(c1.alloc((size_t)nseg * width + CODEC_SPARE));
  VXC(run_lstm(W.get(), lw, x, gin.get(), h0.get(), h1.get(), c0.get(), c1.get(), y, width, layers, sg.get(), seg_frames, nseg, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
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
  DevBuf<float> W;
  std::vector<float> p;
  const ConvW cv = pack_conv(p, w, bias, c_out, c_in, k);
  VXC(upload_segs(seg_rows_in, nseg, sg));
  VXC(upload_segs(so.data(), nseg, sgo));
  VXC(upload_packed(p, W));
  const float *wp = W.get() + cv.w, *bp = bias ? W.get() + cv.b : nullptr;
  if (stride > 1) VXC(run_conv_strided(x, wp, bp, out, so[nseg], c_in, c_out, stride, elu, sgo.get(), sg.get(), nseg, s));
  else if (c_in == 1) VXC(run_conv_in(x, wp, bp, out, so[nseg], c_out, k, sg.get(), nseg, s));
  else VXC(run_conv(x, wp, bp, out, so[nseg], c_in, c_out, k, elu, sg.get(), nseg, 1, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

// The quantiser's search on caller data: emb device [rows][dim], codebooks HOST [n_q][size][dim], codes_out device int32 [n_q][rows].
extern "C" int vx_op_codec_rvq_encode(const float* emb, const float* codebooks, int32_t* codes_out, int64_t rows, int32_t n_q,
                                      int32_t size, int32_t dim, void* stream) {
  if (!emb || !codebooks || !codes_out || rows < 1 || n_q < 1 || n_q > CODEC_MAX_Q) return fail(VX_ERR_ARG, "vx_op_codec_rvq_encode: bad argument");
  if (size < 1 || dim < 1 || !rvq_shape_ok(size, dim)) return fail(VX_ERR_UNSUPPORTED, "vx_op_codec_rvq_encode: codebook %d x %d", size, dim);
  hipStream_t s = (hipStream_t)stream;
  DevBuf<float> W;
  std::vector<float> p;
  const size_t n = (size_t)n_q * size;
  const size_t cb = put(p, std::vector<float>(codebooks, codebooks + n * dim)), sq = put(p, codebook_sq(codebooks, n, dim));
  VXC(upload_packed(p, W));
  VXC(run_rvq_encode(emb, W.get() + cb, W.get() + sq, codes_out, rows, n_q, size, dim, s));
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
