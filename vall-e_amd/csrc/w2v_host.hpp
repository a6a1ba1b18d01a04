// Host side shared by the units built on a transformer speech encoder (spk.hip, asr.hip, whisper.hip), on top of spk_host.hpp's
// leaf pieces.  Two levels:
//   - what every such handle has (SpeechHandle): the key helpers, the stacked q|k|v and encoder-layer packing (EncLayer), the
//     attention triple, the pre-norm layer loop, and the first-use / read scaffolding over host.hpp's LazyDev;
//   - the Wav2Vec2 backbone of spk.hip and asr.hip (W2vModel): its geometry, create-time checks, key table, packing, workspace
//     plan, call staging and the launches from the waveform to the positional convolution.
// Everything here has internal linkage, like spk_host.hpp.
#pragma once
#include <string.h>

#include <algorithm>
#include <memory>

#include "spk_host.hpp"
#include "asr_kernels.hpp"
#include "enc_bf16_kernels.hpp"

namespace vx {
namespace {

// ---- every handle ---------------------------------------------------------------------------------------------------------------
struct W2vCallState {  // the last call, for *_read
  std::vector<int> last_seg;  // [n_tables][n + 1]
  int last_n = 0;
  hipStream_t last_stream = nullptr;
  double last_ms = 0.0;
};

struct SpeechDev {
  DevBuf<float> w;   // every packed tensor
  DevBuf<uint16_t> w16;  // the bf16 encoder mode: the encoder layers' matrices
  DevBuf<float> ws;  // the workspace, carved by the unit's plan
  CallStage stage;   // the per-call tables
};

template <class Dev>
struct SpeechHandle : LazyDev<Dev> {
  std::map<std::string, HostW> w;
  bool finalized = false;
  std::vector<float> packed;  // filled by *_finalize
  bool bf16 = false;               // the bf16 encoder mode (set at create)
  std::vector<uint16_t> packed16;  // its encoder matrices, rounded once by *_finalize; `packed` does not hold them
  W2vCallState call;
};

template <class G>
void norm_keys(G* g, const std::string& nm, int dim) {
  add_key(g, nm + ".weight", {dim});
  add_key(g, nm + ".bias", {dim});
}

template <class G>
void lin_keys(G* g, const std::string& nm, int N, int K, bool bias = true) {
  add_key(g, nm + ".weight", {N, K});
  if (bias) add_key(g, nm + ".bias", {N});
}

template <class G>
void attn_keys(G* g, const std::string& nm, int d, bool k_has_bias) {
  lin_keys(g, nm + ".q_proj", d, d);
  lin_keys(g, nm + ".k_proj", d, d, k_has_bias);
  lin_keys(g, nm + ".v_proj", d, d);
  lin_keys(g, nm + ".out_proj", d, d);
}

// One encoder layer and the names of its parts under the layer's prefix.
struct EncLayer {
  SpkLin qkv, out, ff1, ff2;
  SpkNorm ln1, ln2;
};
struct EncNames {
  const char *attn, *ln1, *ff1, *ff2, *ln2;
};
constexpr EncNames W2V_LAYER{"attention", "layer_norm", "feed_forward.intermediate_dense", "feed_forward.output_dense", "final_layer_norm"};

template <class G>
void enc_layer_keys(G* g, const std::string& pre, const EncNames& nm, int d, int ffn, bool k_has_bias) {
  attn_keys(g, pre + nm.attn, d, k_has_bias);
  norm_keys(g, pre + nm.ln1, d);
  lin_keys(g, pre + nm.ff1, ffn, d);
  lin_keys(g, pre + nm.ff2, d, ffn);
  norm_keys(g, pre + nm.ln2, d);
}

// fp32 -> bf16 bits, round to nearest even (NaN stays NaN).
inline uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

size_t push16(std::vector<uint16_t>& p, const std::vector<float>& v) {
  while (p.size() % 8) p.push_back(0);  // every tensor starts on a 16-byte boundary
  const size_t at = p.size();
  for (float f : v) p.push_back(bf16_rne(f));
  return at;
}

// A linear of the bf16 encoder mode: the matrix rounded into `packed16` (l.w counts its elements), the bias fp32 in `packed`.
template <class G>
SpkLin pack_linear16(G* g, const std::vector<float>& w, const std::vector<float>& b, int N, int K) {
  SpkLin l;
  l.w = push16(g->packed16, w);
  l.b = push(g->packed, b);
  l.has_bias = true; l.C = K; l.N = N;
  return l;
}

// q | k | v stacked; a k without a bias (Whisper) gets zeros.
template <class G>
void stack_qkv(G* g, const std::string& prefix, int d, bool k_has_bias, std::vector<float>& wq, std::vector<float>& bq) {
  for (const char* s : {"q_proj", "k_proj", "v_proj"}) {
    const HostW& w = g->w[prefix + "." + s + ".weight"];
    wq.insert(wq.end(), w.data.begin(), w.data.end());
    if (!k_has_bias && strcmp(s, "k_proj") == 0) {
      bq.insert(bq.end(), (size_t)d, 0.f);
    } else {
      const HostW& b = g->w[prefix + "." + s + ".bias"];
      bq.insert(bq.end(), b.data.begin(), b.data.end());
    }
  }
}

// q | k | v stacked into one GEMM.
template <class G>
SpkLin pack_qkv(G* g, const std::string& prefix, int d, bool k_has_bias) {
  std::vector<float> wq, bq;
  stack_qkv(g, prefix, d, k_has_bias, wq, bq);
  SpkLin l;
  l.w = push(g->packed, wq);
  l.b = push(g->packed, bq);
  l.has_bias = true; l.C = d; l.N = 3 * d;
  return l;
}

template <class G>
EncLayer pack_enc_layer(G* g, const std::string& pre, const EncNames& nm, int d, int ffn, bool k_has_bias) {
  EncLayer ly;
  if (g->bf16) {  // the four matrices in bf16 only
    std::vector<float> wq, bq;
    stack_qkv(g, pre + nm.attn, d, k_has_bias, wq, bq);
    ly.qkv = pack_linear16(g, wq, bq, 3 * d, d);
    auto lin16 = [&](const std::string& name, int N, int K) { return pack_linear16(g, g->w[name + ".weight"].data, g->w[name + ".bias"].data, N, K); };
    ly.out = lin16(pre + nm.attn + ".out_proj", d, d);
    ly.ln1 = pack_norm(g, pre + nm.ln1);
    ly.ff1 = lin16(pre + nm.ff1, ffn, d);
    ly.ff2 = lin16(pre + nm.ff2, d, ffn);
    ly.ln2 = pack_norm(g, pre + nm.ln2);
    return ly;
  }
  ly.qkv = pack_qkv(g, pre + nm.attn, d, k_has_bias);
  ly.out = pack_linear(g, pre + nm.attn + ".out_proj", d, d);
  ly.ln1 = pack_norm(g, pre + nm.ln1);
  ly.ff1 = pack_linear(g, pre + nm.ff1, ffn, d);
  ly.ff2 = pack_linear(g, pre + nm.ff2, d, ffn);
  ly.ln2 = pack_norm(g, pre + nm.ln2);
  return ly;
}

// The start of *_finalize: every tensor is there; the packed block starts empty.
template <class G>
int finalize_begin(G* g) {
  VXC(missing_tensor(g));
  g->packed.clear();
  g->packed16.clear();
  return VX_OK;
}

template <class G>
void finalize_end(G* g) {
  for (auto& kv : g->w) std::vector<float>().swap(kv.second.data);  // the packed copy is the one that is kept
  g->finalized = true;
}

// The part of *_init_device every handle has: the device, the weights, the workspace and the stage.
template <class G>
int init_device(G* g, size_t ws_floats, size_t stage_bytes) {
  VXC(open_device(g));
  auto* fresh = g->dev.get();
  VXC(fresh->w.alloc(g->packed.size() + 4));
  HIPC(hipMemcpy(fresh->w.get(), g->packed.data(), g->packed.size() * sizeof(float), hipMemcpyHostToDevice));
  if (!g->packed16.empty()) {
    VXC(fresh->w16.alloc(g->packed16.size() + 8));
    HIPC(hipMemcpy(fresh->w16.get(), g->packed16.data(), g->packed16.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  }
  VXC(fresh->ws.alloc(ws_floats + 4));
  return fresh->stage.init(stage_bytes);
}

// The head of vx_*_read (`what` is the entry point's prefix, `call` the name of the call whose taps are read).
template <class G>
int read_check(const G* g, const char* what, const char* call, const char* name, int utt, const float* dst) {
  if (!g || !name || !dst) return fail(VX_ERR_ARG, "%s_read: null argument", what);
  if (g->device < 0 || g->call.last_n == 0) return fail(VX_ERR_STATE, "%s_read before any %s_%s", what, what, call);
  if (utt < 0 || utt >= g->call.last_n) return fail(VX_ERR_ARG, "%s_read: utterance %d of %d", what, utt, g->call.last_n);
  return VX_OK;
}

// The tail of vx_*_read: `rows` x `width` floats of the workspace from row `lo` of the buffer at `base`, once the last call is done.
template <class G>
int read_rows(G* g, const char* what, const char* name, int utt, size_t base, long lo, long rows, int width, float* dst, int64_t n_floats) {
  if (n_floats != (int64_t)rows * width)
    return fail(VX_ERR_ARG, "%s_read: %s of utterance %d is %ld x %d floats, not %lld", what, name, utt, rows, width, (long long)n_floats);
  ON_DEVICE(g->device);
  HIPC(hipStreamSynchronize(g->call.last_stream));
  HIPC(hipMemcpy(dst, g->dev->ws.get() + base + (size_t)lo * width, (size_t)rows * width * sizeof(float), hipMemcpyDeviceToHost));
  return VX_OK;
}

// "<prefix><l>" with l in [0, hi] ("hidden3", "gate0", "enc2").
bool tap_index(const std::string& nm, const char* prefix, int hi, int& l) {
  const size_t k = strlen(prefix);
  if (nm.compare(0, k, prefix) != 0 || nm.size() == k) return false;
  char* end = nullptr;
  const long v = strtol(nm.c_str() + k, &end, 10);
  if (*end != 0 || v < 0 || v > hi) return false;
  l = (int)v;
  return true;
}

// ---- the encoder layers' launches ---------------------------------------------------------------------------------------------------
// The row buffers of the encoder layers (the plan of every unit names them alike) and the shape of one call's rows.
struct EncRun {
  float *hid = nullptr, *mid = nullptr, *nrm = nullptr, *qkv = nullptr, *att = nullptr, *tmp = nullptr, *ff = nullptr;
  size_t hid_stride = 0;
  bool keep = false;  // every hidden state has a buffer of its own
  long M = 0;
  int d = 0, H = 0, hd = 0, ffn = 0, Tmax = 0;
  int table = 0;              // the rows' segment table
  const int* hseg = nullptr;  // its host copy
  // the bf16 encoder mode: its rows live where the fp32 mode's nrm / qkv / att / ff do, and its matrices in `W16`
  ebf_t *nrm16 = nullptr, *qkv16 = nullptr, *att16 = nullptr, *ff16 = nullptr;
  const ebf_t* W16 = nullptr;
  float* hidden(int l) const { return hid + hid_stride * (size_t)(keep ? l : (l & 1)); }
};

template <class Plan>
EncRun enc_run(float* ws, const Plan& p, bool keep) {
  EncRun e;
  e.hid = ws + p.hid; e.mid = ws + p.mid; e.nrm = ws + p.nrm; e.qkv = ws + p.qkv; e.att = ws + p.att; e.tmp = ws + p.tmp; e.ff = ws + p.ff;
  e.hid_stride = p.hid_stride; e.keep = keep;
  e.nrm16 = reinterpret_cast<ebf_t*>(e.nrm); e.qkv16 = reinterpret_cast<ebf_t*>(e.qkv); e.att16 = reinterpret_cast<ebf_t*>(e.att);
  e.ff16 = reinterpret_cast<ebf_t*>(e.ff);
  return e;
}

int run_add_ln(const SpkCall& x, const SpkNorm& nm, const float* a, const float* b, float* sum, float* y, long M, int d) {
  asr_add_layernorm<<<(unsigned)((M + 3) / 4), 256, 0, x.s>>>(a, b, x.W + nm.w, x.W + nm.b, sum, y, M, d, x.eps);
  HIPC(hipGetLastError());
  return VX_OK;
}

// tmp = out_proj(attention(qkv(in))); gate and table: WavLM's.
int run_attention(const SpkCall& x, const EncRun& e, const EncLayer& L, const float* in, const float* gate = nullptr, const float* table = nullptr) {
  VXC(run_lin(x, L.qkv, in, e.d, e.qkv, e.M, SPK_ACT_NONE));
  VXC(run_attn(x, x.table(e.table), e.hseg, e.qkv, gate, table, e.att, e.H, e.d, e.hd, e.Tmax));
  return run_lin(x, L.out, e.att, e.d, e.tmp, e.M, SPK_ACT_NONE);
}

// Pre-norm layers: every residual sum is stored by the LayerNorm that reads it.  The caller has written hidden(0) and its
// ln1 rows `nrm`; the last LayerNorm (`last_ln`) writes its sum to `last_sum` (may be null) and its rows to `last_out`.
int run_prenorm_layers(const SpkCall& x, const EncRun& e, const std::vector<EncLayer>& layers, const SpkNorm& last_ln, float* last_sum,
                       float* last_out) {
  const int n_layers = (int)layers.size();
  for (int l = 0; l < n_layers; ++l) {
    const EncLayer& L = layers[l];
    VXC(run_attention(x, e, L, e.nrm));
    VXC(run_add_ln(x, L.ln2, e.hidden(l), e.tmp, e.mid, e.nrm, e.M, e.d));
    VXC(run_lin(x, L.ff1, e.nrm, e.d, e.ff, e.M, SPK_ACT_GELU));
    VXC(run_lin(x, L.ff2, e.ff, e.ffn, e.tmp, e.M, SPK_ACT_NONE));
    if (l + 1 < n_layers) VXC(run_add_ln(x, layers[l + 1].ln1, e.mid, e.tmp, e.hidden(l + 1), e.nrm, e.M, e.d));
    else VXC(run_add_ln(x, last_ln, e.mid, e.tmp, last_sum, last_out, e.M, e.d));
  }
  return VX_OK;
}

// ---- the bf16 encoder mode (enc_bf16_kernels.hpp) ------------------------------------------------------------------------------------
// What the mode serves, checked at create: `what` is the entry point, the names are the config's fields.
int enc_bf16_check(const char* what, int d, int heads, int ffn, const char* heads_name, const char* ffn_name) {
  if (d % heads != 0 || d / heads != 64)
    return fail(VX_ERR_UNSUPPORTED, "%s: the bf16 encoder serves head_dim 64, not hidden / %s = %d / %d", what, heads_name, d, heads);
  if (ffn % 64 != 0) return fail(VX_ERR_UNSUPPORTED, "%s: the bf16 encoder serves %s in multiples of 64, not %d", what, ffn_name, ffn);
  return VX_OK;
}

// The launchers: every shape rule of the kernels is checked here, for the recognisers and for the vx_op_enc16_* entries alike.
int launch_ebf_gemm(int epi, const ebf_t* A, const ebf_t* W, const float* bias, const float* res, void* out, long M, int N, int K, hipStream_t s) {
  if (M <= 0) return VX_OK;
  if (N < 8 || N % 8 != 0 || K < EBF_BK || K % EBF_BK != 0) return fail(VX_ERR_ARG, "bf16 encoder GEMM: N = %d (multiples of 8), K = %d (multiples of %d)", N, K, EBF_BK);
  if (!A || !W || !bias || !out || (epi == EBF_EPI_RESID_F32 && !res)) return fail(VX_ERR_ARG, "bf16 encoder GEMM: null operand");
  const long mt = (M + EBF_BM - 1) / EBF_BM;
  if (mt > 65535) return fail(VX_ERR_CAPACITY, "bf16 encoder GEMM: M = %ld rows", M);
  EbfGemmArgs a{A, W, bias, res, out, M, N, K};
  const dim3 grid((unsigned)((N + EBF_BN - 1) / EBF_BN), (unsigned)mt);
  if (epi == EBF_EPI_BF16) ebf_gemm<EBF_EPI_BF16><<<grid, 256, 0, s>>>(a);
  else if (epi == EBF_EPI_GELU_BF16) ebf_gemm<EBF_EPI_GELU_BF16><<<grid, 256, 0, s>>>(a);
  else if (epi == EBF_EPI_RESID_F32) ebf_gemm<EBF_EPI_RESID_F32><<<grid, 256, 0, s>>>(a);
  else return fail(VX_ERR_ARG, "bf16 encoder GEMM: epilogue %d", epi);
  HIPC(hipGetLastError());
  return VX_OK;
}

int launch_ebf_add_ln(const float* a, const float* b, int bmod, const float* w, const float* beta, float* sum, ebf_t* y, long M, int d, float eps,
                      hipStream_t s) {
  if (M <= 0) return VX_OK;
  ebf_add_layernorm<<<(unsigned)((M + 3) / 4), 256, 0, s>>>(a, b, bmod, w, beta, sum, y, M, d, eps);
  HIPC(hipGetLastError());
  return VX_OK;
}

// Attention over the rows of `seg` (hseg: its host copy, n + 1 offsets), qkv rows [M][3 d] -> out rows [M][d], d = 64 H.
int launch_ebf_attn(const ebf_t* qkv, ebf_t* out, const int* seg, const int* hseg, int n, int H, hipStream_t s) {
  long tiles = 0;
  for (int i = 0; i < n; ++i) tiles += ((long)hseg[i + 1] - hseg[i] + EBF_QT - 1) / EBF_QT;
  if (tiles <= 0) return VX_OK;
  if (H < 1 || H > 65535 || tiles > 2147483647L) return fail(VX_ERR_ARG, "bf16 encoder attention: %d heads, %ld query tiles", H, tiles);
  EbfAttnArgs a{qkv, out, seg, n, H, 64 * H};
  ebf_attention<<<dim3((unsigned)tiles, (unsigned)H), 256, 0, s>>>(a);
  HIPC(hipGetLastError());
  return VX_OK;
}

int run_add_ln16(const SpkCall& x, const SpkNorm& nm, const float* a, const float* b, int bmod, float* sum, ebf_t* y, long M, int d) {
  return launch_ebf_add_ln(a, b, bmod, x.W + nm.w, x.W + nm.b, sum, y, M, d, x.eps, x.s);
}

int run_lin16(const SpkCall& x, const EncRun& e, const SpkLin& l, int epi, const ebf_t* in, const float* res, void* out) {
  return launch_ebf_gemm(epi, in, e.W16 + l.w, x.W + l.b, res, out, e.M, l.N, l.C, x.s);
}

// run_prenorm_layers in the bf16 encoder mode.  The caller has written hidden(0) and its ln1 rows `nrm16`.  out_proj and ff2 add
// their bias and the fp32 residual in the GEMM's epilogue, so the LayerNorms here read one operand; the last one is the fp32
// LayerNorm of the fp32 mode.
int run_prenorm_layers_bf16(const SpkCall& x, const EncRun& e, const std::vector<EncLayer>& layers, const SpkNorm& last_ln, float* last_sum,
                            float* last_out) {
  const int n_layers = (int)layers.size();
  for (int l = 0; l < n_layers; ++l) {
    const EncLayer& L = layers[l];
    VXC(run_lin16(x, e, L.qkv, EBF_EPI_BF16, e.nrm16, nullptr, e.qkv16));
    VXC(launch_ebf_attn(e.qkv16, e.att16, x.table(e.table), e.hseg, x.n, e.H, x.s));
    VXC(run_lin16(x, e, L.out, EBF_EPI_RESID_F32, e.att16, e.hidden(l), e.mid));
    VXC(run_add_ln16(x, L.ln2, e.mid, nullptr, 0, nullptr, e.nrm16, e.M, e.d));
    VXC(run_lin16(x, e, L.ff1, EBF_EPI_GELU_BF16, e.nrm16, nullptr, e.ff16));
    float* next = l + 1 < n_layers ? e.hidden(l + 1) : (last_sum ? last_sum : e.tmp);
    VXC(run_lin16(x, e, L.ff2, EBF_EPI_RESID_F32, e.ff16, e.mid, next));
    if (l + 1 < n_layers) VXC(run_add_ln16(x, layers[l + 1].ln1, next, nullptr, 0, nullptr, e.nrm16, e.M, e.d));
    else VXC(run_ln(x, last_ln, next, nullptr, last_out, e.M, e.d));
  }
  return VX_OK;
}

// ---- the Wav2Vec2 backbone -------------------------------------------------------------------------------------------------------------
// The geometry vx_spk_config and vx_asr_config share.
struct W2vGeom {
  int hidden = 0, layers = 0, heads = 0, ffn = 0;
  int n_conv = 0, conv_dim[8] = {}, conv_kernel[8] = {}, conv_stride[8] = {}, conv_bias = 0;
  int pos_kernel = 0, pos_groups = 0;
  int feat_extract_norm = 0, do_stable_layer_norm = 0, feat_proj_layer_norm = 1;
  float layer_norm_eps = 0.f;
  int max_batch = 0, max_samples = 0, keep_taps = 0;
  int enc_bf16 = 0;  // the bf16 encoder mode
};

template <class C>
W2vGeom w2v_geom(const C& c, int feat_proj_layer_norm, int keep_taps) {
  W2vGeom q;
  q.hidden = c.hidden; q.layers = c.layers; q.heads = c.heads; q.ffn = c.ffn;
  q.n_conv = c.n_conv; q.conv_bias = c.conv_bias;
  for (int i = 0; i < 8; ++i) {
    q.conv_dim[i] = c.conv_dim[i]; q.conv_kernel[i] = c.conv_kernel[i]; q.conv_stride[i] = c.conv_stride[i];
  }
  q.pos_kernel = c.pos_kernel; q.pos_groups = c.pos_groups;
  q.feat_extract_norm = c.feat_extract_norm; q.do_stable_layer_norm = c.do_stable_layer_norm; q.feat_proj_layer_norm = feat_proj_layer_norm;
  q.layer_norm_eps = c.layer_norm_eps;
  q.max_batch = c.max_batch; q.max_samples = c.max_samples; q.keep_taps = keep_taps;
  return q;
}

long frames_of(const W2vGeom& c, long L, int upto) {  // frames after conv layers 0 .. upto
  for (int i = 0; i <= upto; ++i) L = L >= c.conv_kernel[i] ? (L - c.conv_kernel[i]) / c.conv_stride[i] + 1 : 0;
  return L;
}

size_t conv0_ln_lds_bytes(const W2vGeom& c) {  // asr_conv0_ln's tile
  return ((size_t)(ASR_C0_TT - 1) * c.conv_stride[0] + c.conv_kernel[0] + (size_t)c.conv_kernel[0] * c.conv_dim[0]) * sizeof(float);
}

// The create-time checks both units have, in the parts between which a unit runs its own (the order of the refusals is the ABI's).
enum { W2V_CHECK_SIZES, W2V_CHECK_CONVS, W2V_CHECK_RATIOS, W2V_CHECK_SERVED, W2V_CHECK_BATCH };

int w2v_validate(const W2vGeom& c, const char* what, int part) {
  switch (part) {
    case W2V_CHECK_SIZES:
      if (c.hidden < 1 || c.layers < 1 || c.heads < 1 || c.ffn < 1 || c.layers > 256)
        return fail(VX_ERR_ARG, "%s: hidden %d, layers %d, heads %d, ffn %d", what, c.hidden, c.layers, c.heads, c.ffn);
      if (c.n_conv < 1 || c.n_conv > 8) return fail(VX_ERR_ARG, "%s: n_conv = %d outside [1, 8]", what, c.n_conv);
      break;
    case W2V_CHECK_CONVS:
      for (int i = 0; i < c.n_conv; ++i)
        if (c.conv_dim[i] < 1 || c.conv_kernel[i] < 1 || c.conv_stride[i] < 1)
          return fail(VX_ERR_ARG, "%s: conv layer %d: dim %d, kernel %d, stride %d", what, i, c.conv_dim[i], c.conv_kernel[i], c.conv_stride[i]);
      break;
    case W2V_CHECK_RATIOS:
      if (c.hidden % c.heads != 0) return fail(VX_ERR_ARG, "%s: heads = %d does not divide hidden = %d", what, c.heads, c.hidden);
      if (c.hidden % c.pos_groups != 0) return fail(VX_ERR_ARG, "%s: pos_groups = %d does not divide hidden = %d", what, c.pos_groups, c.hidden);
      if (c.max_batch < 1) return fail(VX_ERR_ARG, "%s: max_batch = %d", what, c.max_batch);
      if (!isfinite(c.layer_norm_eps) || c.layer_norm_eps < 0.f) return fail(VX_ERR_ARG, "%s: layer_norm_eps = %g", what, c.layer_norm_eps);
      break;
    case W2V_CHECK_SERVED: {
      const int hd = c.hidden / c.heads;
      if (hd != 16 && hd != 32 && hd != 64) return fail(VX_ERR_UNSUPPORTED, "%s: head_dim = %d (16, 32 and 64 are served)", what, hd);
      if (c.conv_kernel[0] > SPK_C0_MAXK || c.conv_stride[0] > 32)
        return fail(VX_ERR_UNSUPPORTED, "%s: conv layer 0: kernel %d, stride %d (up to %d and 32 are served)", what, c.conv_kernel[0],
                    c.conv_stride[0], SPK_C0_MAXK);
      break;
    }
    case W2V_CHECK_BATCH:
      if (c.max_batch > SPK_MAX_SEG) return fail(VX_ERR_UNSUPPORTED, "%s: max_batch = %d > %d", what, c.max_batch, SPK_MAX_SEG);
      break;
  }
  return VX_OK;
}

struct W2vWeights {
  size_t c0w = 0, c0b = 0, n0w = 0, n0b = 0;  // layer 0: the convolution and its GroupNorm / LayerNorm
  SpkLin conv[8], proj, pos;
  SpkNorm conv_ln[8], fp_ln, enc_ln;
  std::vector<EncLayer> layers;
};

// Offsets (floats) into the workspace: the buffers both units have.  A unit appends its own with take().
struct W2vPlan {
  size_t c0 = 0, conv[2] = {0, 0}, fpn = 0, x0 = 0, hid = 0, hid_stride = 0, mid = 0, nrm = 0, qkv = 0, att = 0, tmp = 0, ff = 0, cstats = 0,
         nstats = 0, total = 0;
  size_t partial = 0;  // doubles
  size_t take(size_t n) {
    const size_t o = total;
    total += (n + 3) / 4 * 4;
    return o;
  }
};

struct W2vModel {
  W2vGeom q;
  W2vWeights bw;
  W2vPlan p;
  int hd = 0, Tmax = 0;
  long min_samples = 0;
};

struct W2vDev : SpeechDev {
  DevBuf<double> partial;
};

template <class Dev>
struct W2vHandle : SpeechHandle<Dev> {
  W2vModel m;
};

// The sizes that follow from a checked geometry; `need` frames of the encoder make the shortest utterance served.
int w2v_size(W2vModel& m, const char* what, long need) {
  const W2vGeom& c = m.q;
  m.hd = c.hidden / c.heads;
  for (int i = c.n_conv - 1; i >= 0; --i) need = std::min((need - 1) * c.conv_stride[i] + c.conv_kernel[i], 1L << 40);
  m.min_samples = need;
  if (c.max_samples < need)
    return fail(VX_ERR_ARG, "%s: max_samples = %d below the shortest utterance served, %ld samples", what, c.max_samples, need);
  m.Tmax = (int)frames_of(c, c.max_samples, c.n_conv - 1);
  // every row buffer is indexed by rows x columns in the kernels' long arithmetic, but the segment tables are int32
  const double rows0 = (double)c.max_batch * (double)frames_of(c, c.max_samples, 0);
  if (rows0 > 2147483647.0) return fail(VX_ERR_UNSUPPORTED, "%s: max_batch x layer-0 frames = %.0f rows exceed int32", what, rows0);
  return VX_OK;
}

// The row buffers up to `ff`.  own_c0: the recogniser's layout, layer 0 in a buffer of its own (its tap "conv0") and the rows `nrm`
// of the stable flavour; else layer 0 shares the ping-pong.
void w2v_plan_rows(W2vModel& m, bool own_c0) {
  const W2vGeom& c = m.q;
  W2vPlan& p = m.p;
  const size_t B = (size_t)c.max_batch;
  if (own_c0) p.c0 = p.take(B * (size_t)frames_of(c, c.max_samples, 0) * c.conv_dim[0]);
  size_t cv[2] = {own_c0 ? 4u : 0u, own_c0 ? 4u : 0u};
  for (int i = own_c0 ? 1 : 0; i < c.n_conv; ++i) cv[i & 1] = std::max(cv[i & 1], B * (size_t)frames_of(c, c.max_samples, i) * c.conv_dim[i]);
  p.conv[0] = p.take(cv[0]);
  p.conv[1] = p.take(cv[1]);
  if (!own_c0) p.c0 = p.conv[0];
  const size_t rows = B * (size_t)m.Tmax, d = (size_t)c.hidden;
  p.fpn = p.take(rows * (size_t)c.conv_dim[c.n_conv - 1]);
  p.x0 = p.take(rows * d);
  p.hid_stride = (rows * d + 3) / 4 * 4;
  p.hid = p.take(p.hid_stride * (c.keep_taps ? (size_t)c.layers + 1 : 2));
  const size_t per = c.enc_bf16 ? 2 : 1;  // the bf16 mode's rows: two elements a float
  p.mid = p.take(rows * d);
  if (own_c0) p.nrm = p.take(rows * d / per);
  p.qkv = p.take(rows * 3 * d / per);
  p.att = p.take(rows * d / per);
  p.tmp = p.take(rows * d);
  p.ff = p.take(rows * (size_t)c.ffn / per);
}

// The statistics of the waveform and of the GroupNorm, after the unit's own buffers.
void w2v_plan_stats(W2vModel& m) {
  const W2vGeom& c = m.q;
  W2vPlan& p = m.p;
  const size_t B = (size_t)c.max_batch;
  p.cstats = p.take(B * (size_t)c.conv_dim[0] * 2);
  p.nstats = p.take(B * 2);
  const size_t t0 = (size_t)frames_of(c, c.max_samples, 0);
  p.partial = c.feat_extract_norm ? 0 : B * ((t0 + SPK_C0_TT - 1) / SPK_C0_TT) * (size_t)c.conv_dim[0] * 2;
}

std::string w2v_layer_prefix(int l) { return "encoder.layers." + std::to_string(l) + "."; }

template <class G>
void w2v_add_keys(G* g, const W2vGeom& c) {
  const int d = c.hidden;
  for (int i = 0; i < c.n_conv; ++i) {
    const std::string cl = "feature_extractor.conv_layers." + std::to_string(i);
    add_key(g, cl + ".conv.weight", {c.conv_dim[i], i == 0 ? 1 : c.conv_dim[i - 1], c.conv_kernel[i]});
    if (c.conv_bias) add_key(g, cl + ".conv.bias", {c.conv_dim[i]});
    if (i == 0 || c.feat_extract_norm) norm_keys(g, cl + ".layer_norm", c.conv_dim[i]);
  }
  const int Cl = c.conv_dim[c.n_conv - 1];
  if (c.feat_proj_layer_norm) norm_keys(g, "feature_projection.layer_norm", Cl);
  lin_keys(g, "feature_projection.projection", d, Cl);
  add_key(g, "encoder.pos_conv_embed.conv.weight", {d, d / c.pos_groups, c.pos_kernel});
  add_key(g, "encoder.pos_conv_embed.conv.bias", {d});
  norm_keys(g, "encoder.layer_norm", d);
  for (int l = 0; l < c.layers; ++l) enc_layer_keys(g, w2v_layer_prefix(l), W2V_LAYER, d, c.ffn, true);
}

// The backbone's tensors up to encoder.layer_norm, in the order that fixes their offsets; the unit packs the layers after it
// (w2v_pack_layer), each followed by what the unit keeps per layer.
template <class G>
void w2v_pack(G* g, const W2vGeom& c, W2vWeights& bw) {
  const int d = c.hidden;
  const std::string c0 = "feature_extractor.conv_layers.0.";
  if (c.feat_extract_norm) {  // asr_conv0_ln reads the weight as [k][C]
    const std::vector<float>& w = g->w[c0 + "conv.weight"].data;
    const int C0 = c.conv_dim[0], k = c.conv_kernel[0];
    std::vector<float> t((size_t)C0 * k);
    for (int ch = 0; ch < C0; ++ch)
      for (int j = 0; j < k; ++j) t[(size_t)j * C0 + ch] = w[(size_t)ch * k + j];
    bw.c0w = push(g->packed, t);
  } else {
    bw.c0w = push(g->packed, g->w[c0 + "conv.weight"].data);
  }
  if (c.conv_bias) bw.c0b = push(g->packed, g->w[c0 + "conv.bias"].data);
  bw.n0w = push(g->packed, g->w[c0 + "layer_norm.weight"].data);
  bw.n0b = push(g->packed, g->w[c0 + "layer_norm.bias"].data);
  for (int i = 1; i < c.n_conv; ++i) {
    const std::string cl = "feature_extractor.conv_layers." + std::to_string(i);
    bw.conv[i] = pack_conv(g, cl + ".conv", c.conv_dim[i], c.conv_dim[i - 1], c.conv_kernel[i], 1, c.conv_bias != 0);
    bw.conv[i].stride = c.conv_stride[i];
    if (c.feat_extract_norm) bw.conv_ln[i] = pack_norm(g, cl + ".layer_norm");
  }
  const int Cl = c.conv_dim[c.n_conv - 1];
  if (c.feat_proj_layer_norm) bw.fp_ln = pack_norm(g, "feature_projection.layer_norm");
  bw.proj = pack_linear(g, "feature_projection.projection", d, Cl);
  bw.pos = pack_conv(g, "encoder.pos_conv_embed.conv", d, d / c.pos_groups, c.pos_kernel, c.pos_groups, true);
  bw.pos.off0 = -(c.pos_kernel / 2);  // padding k / 2; outputs 0 .. T - 1 (an even k's extra last frame is never formed)
  bw.enc_ln = pack_norm(g, "encoder.layer_norm");
  bw.layers.clear();
}

template <class G>
void w2v_pack_layer(G* g, const W2vGeom& c, W2vWeights& bw, int l) {
  bw.layers.push_back(pack_enc_layer(g, w2v_layer_prefix(l), W2V_LAYER, c.hidden, c.ffn, true));
}

// wav pointers [max_batch] | n_samples [max_batch] | segment tables [n_tables][max_batch + 1]
size_t w2v_stage_bytes(const W2vGeom& c, int n_tables) {
  const size_t MB = (size_t)c.max_batch;
  return MB * sizeof(void*) + MB * sizeof(int) + (size_t)n_tables * (MB + 1) * sizeof(int);
}

template <class G>
int w2v_init_device(G* g, int n_tables) {
  VXC(init_device(g, g->m.p.total, w2v_stage_bytes(g->m.q, n_tables)));
  return g->dev->partial.alloc(g->m.p.partial + 2);
}

// One call on the backbone: the handle's device state, the staged tables and their host copy.
struct W2vRun : SpkCall {
  const W2vModel* m;
  float* ws;
  double* partial;
  const float* const* wav;  // device
  const int* n_samples;     // device
  const uint16_t* W16;      // the bf16 encoder mode's matrices, else null
  int* hseg;                // host: [n_tables][MB + 1]
  long rows_of(int t) const { return (long)hseg[(size_t)t * (MB + 1) + n]; }
};

// Waits for the stage and fills it: the pointers, the lengths and the tables of the convolution layers (the first n_conv of
// n_tables; a unit fills the others, then w2v_stage_commit).
template <class G>
int w2v_stage_begin(G* g, int n_tables, int n, const float* const* wav, const int32_t* n_samples, hipStream_t s, W2vRun& x) {
  const W2vGeom& c = g->m.q;
  auto& dv = *g->dev;
  VXC(dv.stage.begin(s));
  const size_t MB = (size_t)c.max_batch, o_ns = MB * sizeof(void*), o_seg = o_ns + MB * sizeof(int);
  const float** hwav = dv.stage.template host<const float*>();
  int* hns = dv.stage.template host<int>(o_ns);
  int* hseg = dv.stage.template host<int>(o_seg);
  for (int t = 0; t < n_tables; ++t) hseg[(size_t)t * (MB + 1)] = 0;
  for (int i = 0; i < n; ++i) {
    hwav[i] = wav[i];
    hns[i] = n_samples[i];
    for (int t = 0; t < c.n_conv; ++t) hseg[(size_t)t * (MB + 1) + i + 1] = hseg[(size_t)t * (MB + 1) + i] + (int)frames_of(c, n_samples[i], t);
  }
  x.m = &g->m; x.eps = c.layer_norm_eps; x.W = dv.w.get(); x.ws = dv.ws.get(); x.partial = dv.partial.get(); x.W16 = dv.w16.get(); x.MB = (int)MB; x.n = n; x.s = s;
  x.wav = dv.stage.template dev<const float* const>();
  x.n_samples = dv.stage.template dev<const int>(o_ns);
  x.seg = dv.stage.template dev<const int>(o_seg);
  x.hseg = hseg;
  return VX_OK;
}

template <class G>
int w2v_stage_commit(G* g, int n_tables, const W2vRun& x) {
  W2vCallState& cs = g->call;
  const int n = x.n;
  cs.last_seg.assign((size_t)n_tables * (n + 1), 0);
  for (int t = 0; t < n_tables; ++t)
    for (int i = 0; i <= n; ++i) cs.last_seg[(size_t)t * (n + 1) + i] = x.hseg[(size_t)t * (x.MB + 1) + i];
  cs.last_n = n;
  cs.last_stream = x.s;
  return g->dev->stage.upload(g->dev->stage.bytes, x.s);
}

// From the waveforms to the positional convolution: leaves the projected features in x0 and the positional term in tmp, and
// describes the encoder's rows in `e` (M, the table and its host copy, the buffers).
int w2v_run_features(const W2vRun& x, bool normalize, EncRun& e) {
  const W2vModel& m = *x.m;
  const W2vGeom& c = m.q;
  const W2vWeights& bw = m.bw;
  const W2vPlan& p = m.p;
  const int n = x.n, d = c.hidden;
  float* ws = x.ws;
  const bool layer_norm = c.feat_extract_norm != 0;
  float* nstats = nullptr;
  if (normalize) {
    nstats = ws + p.nstats;
    spk_wave_stats<<<n, 256, 0, x.s>>>(x.wav, x.n_samples, nstats);
    HIPC(hipGetLastError());
  }
  if (layer_norm) {
    AsrConv0Args a{};
    a.wav = x.wav; a.nstats = nstats; a.wt = x.W + bw.c0w; a.bias = c.conv_bias ? x.W + bw.c0b : nullptr;
    a.ln_w = x.W + bw.n0w; a.ln_b = x.W + bw.n0b; a.out = ws + p.c0;
    a.seg = x.table(0); a.nseg = n; a.C = c.conv_dim[0]; a.k = c.conv_kernel[0]; a.stride = c.conv_stride[0]; a.eps = 1e-5f;
    long tiles = 0;
    for (int i = 0; i < n; ++i) tiles += ((long)x.hseg[i + 1] - x.hseg[i] + ASR_C0_TT - 1) / ASR_C0_TT;
    asr_conv0_ln<<<(unsigned)tiles, 256, conv0_ln_lds_bytes(c), x.s>>>(a);
    HIPC(hipGetLastError());
  } else {
    SpkConv0Args a{};
    a.wav = x.wav; a.nstats = nstats; a.w = x.W + bw.c0w; a.bias = c.conv_bias ? x.W + bw.c0b : nullptr;
    a.gn_w = x.W + bw.n0w; a.gn_b = x.W + bw.n0b; a.partial = x.partial; a.cstats = ws + p.cstats; a.out = ws + p.c0;
    a.seg = x.table(0); a.nseg = n; a.C = c.conv_dim[0]; a.k = c.conv_kernel[0]; a.stride = c.conv_stride[0]; a.eps = 1e-5f;
    long tiles = 0;
    for (int i = 0; i < n; ++i) tiles += ((long)x.hseg[i + 1] - x.hseg[i] + SPK_C0_TT - 1) / SPK_C0_TT;
    const dim3 grid((unsigned)tiles, (unsigned)((a.C + 63) / 64));
    const size_t lds = ((size_t)(SPK_C0_TT - 1) * a.stride + a.k) * sizeof(float);
    spk_conv0<false><<<grid, 256, lds, x.s>>>(a);
    HIPC(hipGetLastError());
    spk_conv0_reduce<<<dim3((unsigned)((a.C + 255) / 256), (unsigned)n), 256, 0, x.s>>>(a);
    HIPC(hipGetLastError());
    spk_conv0<true><<<grid, 256, lds, x.s>>>(a);
    HIPC(hipGetLastError());
  }
  auto conv_buf = [&](int i) { return i == 0 ? ws + p.c0 : ws + p.conv[i & 1]; };
  for (int i = 1; i < c.n_conv; ++i) {
    VXC(run_lin(x, bw.conv[i], conv_buf(i - 1), c.conv_dim[i - 1], conv_buf(i), x.rows_of(i), layer_norm ? SPK_ACT_NONE : SPK_ACT_GELU, i, i - 1));
    if (layer_norm) {
      asr_ln_gelu_rows<<<(unsigned)((x.rows_of(i) + 3) / 4), 256, 0, x.s>>>(conv_buf(i), x.W + bw.conv_ln[i].w, x.W + bw.conv_ln[i].b, x.rows_of(i),
                                                                            c.conv_dim[i], 1e-5f);
      HIPC(hipGetLastError());
    }
  }
  const int te = c.n_conv - 1;  // the encoder's table
  e = enc_run(ws, p, c.keep_taps != 0);
  e.M = x.rows_of(te); e.d = d; e.H = c.heads; e.hd = m.hd; e.ffn = c.ffn; e.Tmax = m.Tmax;
  e.table = te; e.hseg = x.hseg + (size_t)te * (x.MB + 1);
  e.W16 = reinterpret_cast<const ebf_t*>(x.W16);
  const float* feats = conv_buf(te);
  const int Cl = c.conv_dim[te];
  if (c.feat_proj_layer_norm) VXC(run_ln(x, bw.fp_ln, feats, nullptr, ws + p.fpn, e.M, Cl));
  VXC(run_lin(x, bw.proj, c.feat_proj_layer_norm ? ws + p.fpn : feats, Cl, ws + p.x0, e.M, SPK_ACT_NONE));
  return run_lin(x, bw.pos, ws + p.x0, d, ws + p.tmp, e.M, SPK_ACT_GELU, te, te);
}

// The shared head of vx_spk_embed / vx_asr_recognize's checks on the utterances (`shortest` says what the minimum is made of).
template <class G>
int w2v_check_call(const G* g, const char* what, int32_t n, const float* const* wav, const int32_t* n_samples, const char* shortest) {
  const W2vGeom& c = g->m.q;
  if (n > c.max_batch) return fail(VX_ERR_CAPACITY, "%s: n = %d utterances > max_batch %d", what, n, c.max_batch);
  for (int i = 0; i < n; ++i) {
    if (!wav[i]) return fail(VX_ERR_ARG, "%s: utterance %d: null pointer", what, i);
    if (n_samples[i] < g->m.min_samples)
      return fail(VX_ERR_ARG, "%s: utterance %d: %d samples, the shortest served is %ld (%s)", what, i, n_samples[i], g->m.min_samples, shortest);
    if (n_samples[i] > c.max_samples)
      return fail(VX_ERR_CAPACITY, "%s: utterance %d: %d samples > max_samples %d", what, i, n_samples[i], c.max_samples);
  }
  return VX_OK;
}

// vx_*_get_timings: host ms, workspace bytes (`extra_bytes` on top of the plan's), weight bytes, encoder rows of the last call.
template <class G>
int w2v_timings(const G* g, const char* what, size_t extra_bytes, double* out, int32_t n) {
  if (!g || !out || n < 0 || n > 4) return fail(VX_ERR_ARG, "%s_get_timings: null argument or n outside [0, 4]", what);
  const W2vCallState& cs = g->call;
  const double v[4] = {cs.last_ms, (double)(g->m.p.total * sizeof(float) + g->m.p.partial * sizeof(double) + extra_bytes),
                       (double)(g->packed.size() * sizeof(float) + g->packed16.size() * sizeof(uint16_t)),
                       cs.last_n ? (double)cs.last_seg[(size_t)(g->m.q.n_conv - 1) * (cs.last_n + 1) + cs.last_n] : 0.0};
  for (int i = 0; i < n; ++i) out[i] = v[i];
  return VX_OK;
}

}  // namespace
}  // namespace vx
