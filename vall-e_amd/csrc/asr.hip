// CTC speech recogniser (Wav2Vec2ForCTC / HubertForCTC) behind the C ABI (include/vallex.h, vx_asr_*), the greedy CTC decode
// (vx_ctc_greedy) and the edit distance (vx_edit_distance).  The group / post-norm flavour is the speaker encoder's path up to the
// last hidden state, on the same kernels (spk_kernels.hpp through spk_host.hpp); the layer / stable flavour adds asr_kernels.hpp's
// layer 0, LayerNorm + GELU rows and residual-folding LayerNorm.  A translation unit and a handle of its own, like spk.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <memory>
#include <string>
#include <vector>

#undef VX_STAMPS  // the in-kernel stamps write device globals of engine.hip's unit, out of this unit's reach
#include "spk_host.hpp"
#include "asr_kernels.hpp"
#include "falign_kernels.hpp"

using namespace vx;

namespace {

struct AsrLayer {
  SpkLin qkv, out, ff1, ff2;
  SpkNorm ln1, ln2;
};

struct AsrDev {
  DevBuf<float> w;   // every packed tensor
  DevBuf<float> ws;  // the workspace, carved by offsets (AsrPlan)
  DevBuf<double> partial, lp;
  DevBuf<int> ids;
  // per call: wav pointers [max_batch] | n_samples [max_batch] | segment tables [n_conv][max_batch + 1]
  CallStage stage;
  DevBuf<unsigned char> fal;  // vx_falign_asr's scratch, grow-only
  size_t fal_bytes = 0;
};

// Offsets (floats) into the workspace.
struct AsrPlan {
  size_t c0 = 0, conv[2] = {0, 0}, fpn = 0, x0 = 0, hid = 0, hid_stride = 0, mid = 0, nrm = 0, qkv = 0, att = 0, tmp = 0, ff = 0, logits = 0,
         cstats = 0, nstats = 0, total = 0;
  size_t partial = 0;  // doubles
};

}  // namespace

struct vx_asr {
  vx_asr_config cfg{};
  std::map<std::string, HostW> w;
  bool finalized = false;
  int hd = 0, Tmax = 0;
  long min_samples = 0;
  AsrPlan plan;
  // filled by vx_asr_finalize
  std::vector<float> packed;
  size_t c0w = 0, c0b = 0, n0w = 0, n0b = 0;
  SpkLin conv[8], proj, pos, head;
  SpkNorm conv_ln[8], fp_ln, enc_ln;
  std::vector<AsrLayer> layers;
  int device = -1;  // >= 0: `dev` is complete
  std::unique_ptr<AsrDev> dev;
  // the last call, for vx_asr_read
  std::vector<int> last_seg;  // [n_conv][n + 1]
  int last_n = 0;
  hipStream_t last_stream = nullptr;
  double last_ms = 0.0;
};

namespace {

long frames_of(const vx_asr_config& c, long L, int upto) {  // frames after conv layers 0 .. upto
  for (int i = 0; i <= upto; ++i) L = L >= c.conv_kernel[i] ? (L - c.conv_kernel[i]) / c.conv_stride[i] + 1 : 0;
  return L;
}

size_t conv0_lds_bytes(const vx_asr_config& c) {
  return ((size_t)(ASR_C0_TT - 1) * c.conv_stride[0] + c.conv_kernel[0] + (size_t)c.conv_kernel[0] * c.conv_dim[0]) * sizeof(float);
}

void make_plan(vx_asr* g) {
  const vx_asr_config& c = g->cfg;
  AsrPlan& p = g->plan;
  const size_t B = (size_t)c.max_batch;
  size_t at = 0;
  auto take = [&](size_t n) { const size_t o = at; at += (n + 3) / 4 * 4; return o; };
  p.c0 = take(B * (size_t)frames_of(c, c.max_samples, 0) * c.conv_dim[0]);  // a buffer of its own: the tap "conv0"
  size_t cv[2] = {4, 4};
  for (int i = 1; i < c.n_conv; ++i) cv[i & 1] = std::max(cv[i & 1], B * (size_t)frames_of(c, c.max_samples, i) * c.conv_dim[i]);
  p.conv[0] = take(cv[0]);
  p.conv[1] = take(cv[1]);
  const size_t rows = B * (size_t)g->Tmax, d = (size_t)c.hidden;
  p.fpn = take(rows * (size_t)c.conv_dim[c.n_conv - 1]);
  p.x0 = take(rows * d);
  p.hid_stride = (rows * d + 3) / 4 * 4;
  p.hid = take(p.hid_stride * ((c.flags & VX_ASR_KEEP_TAPS) ? (size_t)c.layers + 1 : 2));
  p.mid = take(rows * d);
  p.nrm = take(rows * d);
  p.qkv = take(rows * 3 * d);
  p.att = take(rows * d);
  p.tmp = take(rows * d);
  p.ff = take(rows * (size_t)c.ffn);
  p.logits = take(rows * (size_t)c.vocab);
  p.cstats = take(B * (size_t)c.conv_dim[0] * 2);
  p.nstats = take(B * 2);
  p.total = at;
  const size_t t0 = (size_t)frames_of(c, c.max_samples, 0);
  p.partial = c.feat_extract_norm ? 0 : B * ((t0 + SPK_C0_TT - 1) / SPK_C0_TT) * (size_t)c.conv_dim[0] * 2;
}

int asr_init_device(vx_asr* g) {
  int dev = 0;
  HIPC(hipGetDevice(&dev));
  g->device = dev;
  g->dev.reset(new AsrDev());
  AsrDev& d = *g->dev;
  const size_t MB = (size_t)g->cfg.max_batch;
  VXC(d.w.alloc(g->packed.size() + 4));
  HIPC(hipMemcpy(d.w.get(), g->packed.data(), g->packed.size() * sizeof(float), hipMemcpyHostToDevice));
  VXC(d.ws.alloc(g->plan.total + 4));
  VXC(d.partial.alloc(g->plan.partial + 2));
  VXC(d.lp.alloc(MB * (size_t)g->Tmax));
  VXC(d.ids.alloc(MB * (size_t)g->Tmax));
  VXC(d.stage.init(MB * sizeof(void*) + MB * sizeof(int) + (size_t)g->cfg.n_conv * (MB + 1) * sizeof(int)));
  return VX_OK;
}

struct CallCtx : SpkCall {
  const vx_asr* g;
  float* ws;
};

int run_add_ln(const CallCtx& x, const SpkNorm& nm, const float* a, const float* b, float* sum, float* y, long M, int d) {
  asr_add_layernorm<<<(unsigned)((M + 3) / 4), 256, 0, x.s>>>(a, b, x.W + nm.w, x.W + nm.b, sum, y, M, d, x.eps);
  HIPC(hipGetLastError());
  return VX_OK;
}

// The frames' argmax and log-probability, then one workgroup per utterance: the shared tail of vx_asr_recognize and vx_ctc_greedy.
int launch_ctc(const float* logits, int vocab, int blank, int n, long M, const int* seg_dev, int* ids, double* lp, int* tokens,
               int* token_frames, int* counts, float* mean_lp, float* frame_lp, hipStream_t s) {
  if (M > 0) {
    ctc_frame_kernel<<<(unsigned)((M + 3) / 4), 256, 0, s>>>(logits, vocab, M, ids, lp);
    HIPC(hipGetLastError());
  }
  ctc_collapse_kernel<<<(unsigned)n, CTC_WG, 0, s>>>(ids, lp, seg_dev, blank, tokens, token_frames, counts, mean_lp, frame_lp);
  HIPC(hipGetLastError());
  return VX_OK;
}

int run_call(const CallCtx& x, const float* const* wav, const int* n_samples_dev, const int* hseg, int flags) {
  const vx_asr* g = x.g;
  const vx_asr_config& c = g->cfg;
  const AsrPlan& p = g->plan;
  const int n = x.n, MB = x.MB, d = c.hidden, H = c.heads;
  auto rows_of = [&](int t) { return (long)hseg[(size_t)t * (MB + 1) + n]; };
  float* ws = x.ws;
  const bool layer_norm = c.feat_extract_norm != 0, stable = c.do_stable_layer_norm != 0;
  // ---- feature encoder
  float* nstats = nullptr;
  if (flags & VX_ASR_NORMALIZE) {
    nstats = ws + p.nstats;
    spk_wave_stats<<<n, 256, 0, x.s>>>(wav, n_samples_dev, nstats);
    HIPC(hipGetLastError());
  }
  if (layer_norm) {
    AsrConv0Args a{};
    a.wav = wav; a.nstats = nstats; a.wt = x.W + g->c0w; a.bias = c.conv_bias ? x.W + g->c0b : nullptr;
    a.ln_w = x.W + g->n0w; a.ln_b = x.W + g->n0b; a.out = ws + p.c0;
    a.seg = x.table(0); a.nseg = n; a.C = c.conv_dim[0]; a.k = c.conv_kernel[0]; a.stride = c.conv_stride[0]; a.eps = 1e-5f;
    long tiles = 0;
    for (int i = 0; i < n; ++i) tiles += ((long)hseg[i + 1] - hseg[i] + ASR_C0_TT - 1) / ASR_C0_TT;
    asr_conv0_ln<<<(unsigned)tiles, 256, conv0_lds_bytes(c), x.s>>>(a);
    HIPC(hipGetLastError());
  } else {
    SpkConv0Args a{};
    a.wav = wav; a.nstats = nstats; a.w = x.W + g->c0w; a.bias = c.conv_bias ? x.W + g->c0b : nullptr;
    a.gn_w = x.W + g->n0w; a.gn_b = x.W + g->n0b; a.partial = g->dev->partial.get(); a.cstats = ws + p.cstats; a.out = ws + p.c0;
    a.seg = x.table(0); a.nseg = n; a.C = c.conv_dim[0]; a.k = c.conv_kernel[0]; a.stride = c.conv_stride[0]; a.eps = 1e-5f;
    long tiles = 0;
    for (int i = 0; i < n; ++i) tiles += ((long)hseg[i + 1] - hseg[i] + SPK_C0_TT - 1) / SPK_C0_TT;
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
    VXC(run_lin(x, g->conv[i], conv_buf(i - 1), c.conv_dim[i - 1], conv_buf(i), rows_of(i), layer_norm ? SPK_ACT_NONE : SPK_ACT_GELU, i, i - 1));
    if (layer_norm) {
      asr_ln_gelu_rows<<<(unsigned)((rows_of(i) + 3) / 4), 256, 0, x.s>>>(conv_buf(i), x.W + g->conv_ln[i].w, x.W + g->conv_ln[i].b, rows_of(i),
                                                                          c.conv_dim[i], 1e-5f);
      HIPC(hipGetLastError());
    }
  }
  const int te = c.n_conv - 1;  // the encoder's table
  const long M = rows_of(te);
  const float* feats = conv_buf(te);
  const int Cl = c.conv_dim[te];
  const int* et = hseg + (size_t)te * (MB + 1);
  // ---- projection, positional convolution
  if (c.feat_proj_layer_norm) VXC(run_ln(x, g->fp_ln, feats, nullptr, ws + p.fpn, M, Cl));
  VXC(run_lin(x, g->proj, c.feat_proj_layer_norm ? ws + p.fpn : feats, Cl, ws + p.x0, M, SPK_ACT_NONE));
  VXC(run_lin(x, g->pos, ws + p.x0, d, ws + p.tmp, M, SPK_ACT_GELU, te, te));
  const bool keep = (c.flags & VX_ASR_KEEP_TAPS) != 0;
  auto hid = [&](int l) { return ws + p.hid + p.hid_stride * (size_t)(keep ? l : (l & 1)); };
  auto attention = [&](const AsrLayer& L, const float* in) {
    VXC(run_lin(x, L.qkv, in, d, ws + p.qkv, M, SPK_ACT_NONE));
    VXC(run_attn(x, x.table(te), et, ws + p.qkv, nullptr, nullptr, ws + p.att, H, d, g->hd, g->Tmax));
    return run_lin(x, L.out, ws + p.att, d, ws + p.tmp, M, SPK_ACT_NONE);
  };
  if (!stable) {  // post-norm: the speaker encoder's plain mode
    VXC(run_ln(x, g->enc_ln, ws + p.x0, ws + p.tmp, hid(0), M, d));
    for (int l = 0; l < c.layers; ++l) {
      const AsrLayer& L = g->layers[l];
      VXC(attention(L, hid(l)));
      VXC(run_ln(x, L.ln1, hid(l), ws + p.tmp, ws + p.mid, M, d));
      VXC(run_lin(x, L.ff1, ws + p.mid, d, ws + p.ff, M, SPK_ACT_GELU));
      VXC(run_lin(x, L.ff2, ws + p.ff, c.ffn, ws + p.tmp, M, SPK_ACT_NONE));
      VXC(run_ln(x, L.ln2, ws + p.mid, ws + p.tmp, hid(l + 1), M, d));
    }
  } else {  // stable: every residual sum is stored by the LayerNorm that reads it
    VXC(run_add_ln(x, g->layers[0].ln1, ws + p.x0, ws + p.tmp, hid(0), ws + p.nrm, M, d));
    for (int l = 0; l < c.layers; ++l) {
      const AsrLayer& L = g->layers[l];
      VXC(attention(L, ws + p.nrm));
      VXC(run_add_ln(x, L.ln2, hid(l), ws + p.tmp, ws + p.mid, ws + p.nrm, M, d));
      VXC(run_lin(x, L.ff1, ws + p.nrm, d, ws + p.ff, M, SPK_ACT_GELU));
      VXC(run_lin(x, L.ff2, ws + p.ff, c.ffn, ws + p.tmp, M, SPK_ACT_NONE));
      if (l + 1 < c.layers) VXC(run_add_ln(x, g->layers[l + 1].ln1, ws + p.mid, ws + p.tmp, hid(l + 1), ws + p.nrm, M, d));
      else VXC(run_add_ln(x, g->enc_ln, ws + p.mid, ws + p.tmp, nullptr, hid(l + 1), M, d));
    }
  }
  // ---- head
  return run_lin(x, g->head, hid(c.layers), d, ws + p.logits, M, SPK_ACT_NONE);
}

}  // namespace

extern "C" int64_t vx_asr_frames(const vx_asr* g, int64_t n_samples) {
  return !g ? -1 : (int64_t)frames_of(g->cfg, (long)std::max<int64_t>(0, n_samples), g->cfg.n_conv - 1);
}

extern "C" int64_t vx_asr_min_samples(const vx_asr* g) { return !g ? -1 : (int64_t)g->min_samples; }

extern "C" int vx_asr_create(const vx_asr_config* cfg, vx_asr** out) {
  if (!cfg || !out) return fail(VX_ERR_ARG, "vx_asr_create: null argument");
  if (cfg->struct_size != (int32_t)sizeof(vx_asr_config))
    return fail(VX_ERR_ARG, "vx_asr_create: struct_size %d, expected %zu", cfg->struct_size, sizeof(vx_asr_config));
  const vx_asr_config& c = *cfg;
  if (c.hidden < 1 || c.layers < 1 || c.heads < 1 || c.ffn < 1 || c.layers > 256)
    return fail(VX_ERR_ARG, "vx_asr_create: hidden %d, layers %d, heads %d, ffn %d", c.hidden, c.layers, c.heads, c.ffn);
  if (c.n_conv < 1 || c.n_conv > 8) return fail(VX_ERR_ARG, "vx_asr_create: n_conv = %d outside [1, 8]", c.n_conv);
  for (int i = 0; i < c.n_conv; ++i)
    if (c.conv_dim[i] < 1 || c.conv_kernel[i] < 1 || c.conv_stride[i] < 1)
      return fail(VX_ERR_ARG, "vx_asr_create: conv layer %d: dim %d, kernel %d, stride %d", i, c.conv_dim[i], c.conv_kernel[i], c.conv_stride[i]);
  if (c.pos_kernel < 1 || c.pos_groups < 1) return fail(VX_ERR_ARG, "vx_asr_create: pos_kernel %d, pos_groups %d", c.pos_kernel, c.pos_groups);
  if (c.vocab < 1 || c.blank < 0 || c.blank >= c.vocab) return fail(VX_ERR_ARG, "vx_asr_create: vocab %d, blank %d", c.vocab, c.blank);
  if (c.hidden % c.heads != 0) return fail(VX_ERR_ARG, "vx_asr_create: heads = %d does not divide hidden = %d", c.heads, c.hidden);
  if (c.hidden % c.pos_groups != 0) return fail(VX_ERR_ARG, "vx_asr_create: pos_groups = %d does not divide hidden = %d", c.pos_groups, c.hidden);
  if (c.max_batch < 1) return fail(VX_ERR_ARG, "vx_asr_create: max_batch = %d", c.max_batch);
  if (!isfinite(c.layer_norm_eps) || c.layer_norm_eps < 0.f) return fail(VX_ERR_ARG, "vx_asr_create: layer_norm_eps = %g", c.layer_norm_eps);
  if (c.flags & ~VX_ASR_KEEP_TAPS) return fail(VX_ERR_ARG, "vx_asr_create: flags = %d", c.flags);
  if (c.add_adapter != 0) return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: add_adapter");
  if (c.conv_pos_batch_norm != 0) return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: conv_pos_batch_norm");
  if (c.activation != 0) return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: activation = %d (gelu is served)", c.activation);
  if ((c.feat_extract_norm != 0) != (c.do_stable_layer_norm != 0))
    return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: feat_extract_norm = %d with do_stable_layer_norm = %d (group / post-norm and layer / stable are served)",
                c.feat_extract_norm, c.do_stable_layer_norm);
  if (c.feat_extract_norm != 0 && !c.conv_bias)
    return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: feat_extract_norm = \"layer\" without conv_bias");
  const int hd = c.hidden / c.heads;
  if (hd != 16 && hd != 32 && hd != 64)
    return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: head_dim = %d (16, 32 and 64 are served)", hd);
  if (c.conv_kernel[0] > SPK_C0_MAXK || c.conv_stride[0] > 32)
    return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: conv layer 0: kernel %d, stride %d (up to %d and 32 are served)", c.conv_kernel[0],
                c.conv_stride[0], SPK_C0_MAXK);
  if (c.feat_extract_norm != 0 && (c.conv_dim[0] > ASR_C0_MAXC || conv0_lds_bytes(c) > (size_t)ASR_C0_LDS))
    return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: conv layer 0: dim %d x kernel %d (up to %d channels and %d bytes of tile are served)",
                c.conv_dim[0], c.conv_kernel[0], ASR_C0_MAXC, ASR_C0_LDS);
  if (c.max_batch > SPK_MAX_SEG) return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: max_batch = %d > %d", c.max_batch, SPK_MAX_SEG);

  std::unique_ptr<vx_asr> g(new vx_asr());
  g->cfg = c;
  g->hd = hd;
  long need = 1;
  for (int i = c.n_conv - 1; i >= 0; --i) need = std::min((need - 1) * c.conv_stride[i] + c.conv_kernel[i], 1L << 40);
  g->min_samples = need;
  if (c.max_samples < need)
    return fail(VX_ERR_ARG, "vx_asr_create: max_samples = %d below the shortest utterance served, %ld samples", c.max_samples, need);
  g->Tmax = (int)frames_of(c, c.max_samples, c.n_conv - 1);
  // every row buffer is indexed by rows x columns in the kernels' long arithmetic, but the segment tables are int32
  const double rows0 = (double)c.max_batch * (double)frames_of(c, c.max_samples, 0);
  if (rows0 > 2147483647.0) return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: max_batch x layer-0 frames = %.0f rows exceed int32", rows0);
  make_plan(g.get());

  const int d = c.hidden;
  auto norm_keys = [&](const std::string& nm, int dim) {
    add_key(g.get(), nm + ".weight", {dim});
    add_key(g.get(), nm + ".bias", {dim});
  };
  auto lin_keys = [&](const std::string& nm, int N, int K) {
    add_key(g.get(), nm + ".weight", {N, K});
    add_key(g.get(), nm + ".bias", {N});
  };
  for (int i = 0; i < c.n_conv; ++i) {
    const std::string cl = "feature_extractor.conv_layers." + std::to_string(i);
    add_key(g.get(), cl + ".conv.weight", {c.conv_dim[i], i == 0 ? 1 : c.conv_dim[i - 1], c.conv_kernel[i]});
    if (c.conv_bias) add_key(g.get(), cl + ".conv.bias", {c.conv_dim[i]});
    if (i == 0 || c.feat_extract_norm) norm_keys(cl + ".layer_norm", c.conv_dim[i]);
  }
  const int Cl = c.conv_dim[c.n_conv - 1];
  if (c.feat_proj_layer_norm) norm_keys("feature_projection.layer_norm", Cl);
  lin_keys("feature_projection.projection", d, Cl);
  add_key(g.get(), "encoder.pos_conv_embed.conv.weight", {d, d / c.pos_groups, c.pos_kernel});
  add_key(g.get(), "encoder.pos_conv_embed.conv.bias", {d});
  norm_keys("encoder.layer_norm", d);
  for (int l = 0; l < c.layers; ++l) {
    const std::string pre = "encoder.layers." + std::to_string(l) + ".";
    for (const char* nm : {"q_proj", "k_proj", "v_proj", "out_proj"}) lin_keys(pre + "attention." + nm, d, d);
    norm_keys(pre + "layer_norm", d);
    lin_keys(pre + "feed_forward.intermediate_dense", c.ffn, d);
    lin_keys(pre + "feed_forward.output_dense", d, c.ffn);
    norm_keys(pre + "final_layer_norm", d);
  }
  lin_keys("lm_head", c.vocab, d);
  *out = g.release();
  return VX_OK;
}

extern "C" void vx_asr_destroy(vx_asr* g) {
  if (!g) return;
  if (g->device >= 0) {
    DevGuard guard(g->device);
    (void)g->dev->stage.drain();
    g->dev.reset();
  }
  delete g;
}

extern "C" int vx_asr_set_weight(vx_asr* g, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
  return set_weight(g, "vx_asr", key, data, shape, ndim);
}

extern "C" int vx_asr_finalize(vx_asr* g) {
  if (!g) return fail(VX_ERR_ARG, "vx_asr_finalize: null handle");
  if (g->finalized) return VX_OK;
  for (auto& kv : g->w)
    if (!kv.second.set) return fail(VX_ERR_WEIGHTS, "missing tensor %s", kv.first.c_str());
  const vx_asr_config& c = g->cfg;
  const int d = c.hidden, L = c.layers;
  g->packed.clear();
  const std::string c0 = "feature_extractor.conv_layers.0.";
  if (c.feat_extract_norm) {  // asr_conv0_ln reads the weight as [k][C]
    const std::vector<float>& w = g->w[c0 + "conv.weight"].data;
    const int C0 = c.conv_dim[0], k = c.conv_kernel[0];
    std::vector<float> t((size_t)C0 * k);
    for (int ch = 0; ch < C0; ++ch)
      for (int j = 0; j < k; ++j) t[(size_t)j * C0 + ch] = w[(size_t)ch * k + j];
    g->c0w = push(g->packed, t);
  } else {
    g->c0w = push(g->packed, g->w[c0 + "conv.weight"].data);
  }
  if (c.conv_bias) g->c0b = push(g->packed, g->w[c0 + "conv.bias"].data);
  g->n0w = push(g->packed, g->w[c0 + "layer_norm.weight"].data);
  g->n0b = push(g->packed, g->w[c0 + "layer_norm.bias"].data);
  for (int i = 1; i < c.n_conv; ++i) {
    const std::string cl = "feature_extractor.conv_layers." + std::to_string(i);
    g->conv[i] = pack_conv(g, cl + ".conv", c.conv_dim[i], c.conv_dim[i - 1], c.conv_kernel[i], 1, c.conv_bias != 0);
    g->conv[i].stride = c.conv_stride[i];
    if (c.feat_extract_norm) g->conv_ln[i] = pack_norm(g, cl + ".layer_norm");
  }
  const int Cl = c.conv_dim[c.n_conv - 1];
  if (c.feat_proj_layer_norm) g->fp_ln = pack_norm(g, "feature_projection.layer_norm");
  g->proj = pack_linear(g, "feature_projection.projection", d, Cl);
  g->pos = pack_conv(g, "encoder.pos_conv_embed.conv", d, d / c.pos_groups, c.pos_kernel, c.pos_groups, true);
  g->pos.off0 = -(c.pos_kernel / 2);  // padding k / 2; outputs 0 .. T - 1 (an even k's extra last frame is never formed)
  g->enc_ln = pack_norm(g, "encoder.layer_norm");
  g->layers.assign(L, AsrLayer());
  for (int l = 0; l < L; ++l) {
    const std::string pre = "encoder.layers." + std::to_string(l) + ".";
    AsrLayer& ly = g->layers[l];
    std::vector<float> wq, bq;
    for (const char* nm : {"q_proj", "k_proj", "v_proj"}) {
      const HostW& w = g->w[pre + "attention." + nm + ".weight"];
      const HostW& b = g->w[pre + "attention." + nm + ".bias"];
      wq.insert(wq.end(), w.data.begin(), w.data.end());
      bq.insert(bq.end(), b.data.begin(), b.data.end());
    }
    ly.qkv.w = push(g->packed, wq);
    ly.qkv.b = push(g->packed, bq);
    ly.qkv.has_bias = true; ly.qkv.C = d; ly.qkv.N = 3 * d;
    ly.out = pack_linear(g, pre + "attention.out_proj", d, d);
    ly.ln1 = pack_norm(g, pre + "layer_norm");
    ly.ff1 = pack_linear(g, pre + "feed_forward.intermediate_dense", c.ffn, d);
    ly.ff2 = pack_linear(g, pre + "feed_forward.output_dense", d, c.ffn);
    ly.ln2 = pack_norm(g, pre + "final_layer_norm");
  }
  g->head = pack_linear(g, "lm_head", c.vocab, d);
  for (auto& kv : g->w) std::vector<float>().swap(kv.second.data);  // the packed copy is the one that is kept
  g->finalized = true;
  return VX_OK;
}

extern "C" int vx_asr_recognize(vx_asr* g, int32_t n, const float* const* wav, const int32_t* n_samples, int32_t flags, int32_t* tokens_out,
                                int32_t* token_frames_out, int32_t* counts_out, float* mean_logprob_out, float* logits_out, void* stream) {
  if (!g || !wav || !n_samples || !tokens_out || !token_frames_out || !counts_out || !mean_logprob_out)
    return fail(VX_ERR_ARG, "vx_asr_recognize: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_asr_recognize: n = %d utterances", n);
  if (flags & ~VX_ASR_NORMALIZE) return fail(VX_ERR_ARG, "vx_asr_recognize: flags = %d", flags);
  if (!g->finalized) return fail(VX_ERR_STATE, "vx_asr_recognize before vx_asr_finalize");
  const vx_asr_config& c = g->cfg;
  if (n > c.max_batch) return fail(VX_ERR_CAPACITY, "vx_asr_recognize: n = %d utterances > max_batch %d", n, c.max_batch);
  for (int i = 0; i < n; ++i) {
    if (!wav[i]) return fail(VX_ERR_ARG, "vx_asr_recognize: utterance %d: null pointer", i);
    if (n_samples[i] < g->min_samples)
      return fail(VX_ERR_ARG, "vx_asr_recognize: utterance %d: %d samples, the shortest served is %ld (one encoder frame)", i, n_samples[i],
                  g->min_samples);
    if (n_samples[i] > c.max_samples)
      return fail(VX_ERR_CAPACITY, "vx_asr_recognize: utterance %d: %d samples > max_samples %d", i, n_samples[i], c.max_samples);
  }
  const auto t_begin = std::chrono::steady_clock::now();
  if (g->device < 0) {
    const int rc = asr_init_device(g);
    if (rc != VX_OK) {  // a failed first use leaves the handle as it was before it
      g->dev.reset();
      g->device = -1;
      return rc;
    }
  }
  DevGuard guard(g->device);
  HIPC(guard.err);
  AsrDev& dv = *g->dev;
  hipStream_t s = (hipStream_t)stream;
  VXC(dv.stage.begin(s));
  const size_t MB = (size_t)c.max_batch;
  const float** hwav = dv.stage.host<const float*>();
  int* hns = dv.stage.host<int>(MB * sizeof(void*));
  int* hseg = dv.stage.host<int>(MB * sizeof(void*) + MB * sizeof(int));
  const int NT = c.n_conv;
  for (int t = 0; t < NT; ++t) hseg[(size_t)t * (MB + 1)] = 0;
  for (int i = 0; i < n; ++i) {
    hwav[i] = wav[i];
    hns[i] = n_samples[i];
    for (int t = 0; t < NT; ++t)
      hseg[(size_t)t * (MB + 1) + i + 1] = hseg[(size_t)t * (MB + 1) + i] + (int)frames_of(c, n_samples[i], t);
  }
  g->last_seg.assign((size_t)NT * (n + 1), 0);
  for (int t = 0; t < NT; ++t)
    for (int i = 0; i <= n; ++i) g->last_seg[(size_t)t * (n + 1) + i] = hseg[(size_t)t * (MB + 1) + i];
  g->last_n = n;
  g->last_stream = s;
  VXC(dv.stage.upload(dv.stage.bytes, s));
  CallCtx x{};
  x.g = g; x.eps = c.layer_norm_eps; x.W = dv.w.get(); x.ws = dv.ws.get(); x.MB = (int)MB; x.n = n; x.s = s;
  x.seg = dv.stage.dev<const int>(MB * sizeof(void*) + MB * sizeof(int));
  VXC(run_call(x, dv.stage.dev<const float* const>(), dv.stage.dev<const int>(MB * sizeof(void*)), hseg, flags));
  const int te = NT - 1;
  const long M = hseg[(size_t)te * (MB + 1) + n];
  const float* logits = dv.ws.get() + g->plan.logits;
  VXC(launch_ctc(logits, c.vocab, c.blank, n, M, x.table(te), dv.ids.get(), dv.lp.get(), tokens_out, token_frames_out, counts_out,
                 mean_logprob_out, nullptr, s));
  if (logits_out) HIPC(hipMemcpyAsync(logits_out, logits, (size_t)M * c.vocab * sizeof(float), hipMemcpyDeviceToDevice, s));
  const int rc = dv.stage.finish(s);
  g->last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return rc;
}

extern "C" int vx_asr_read(vx_asr* g, const char* name, int32_t utt, float* dst, int64_t n_floats) {
  if (!g || !name || !dst) return fail(VX_ERR_ARG, "vx_asr_read: null argument");
  if (g->device < 0 || g->last_n == 0) return fail(VX_ERR_STATE, "vx_asr_read before any vx_asr_recognize");
  const int n = g->last_n;
  if (utt < 0 || utt >= n) return fail(VX_ERR_ARG, "vx_asr_read: utterance %d of %d", utt, n);
  const vx_asr_config& c = g->cfg;
  const AsrPlan& p = g->plan;
  const int te = c.n_conv - 1;
  const std::string nm = name;
  size_t base = 0;
  int table = te, width = c.hidden;
  if (nm == "conv0") {
    table = 0; width = c.conv_dim[0]; base = p.c0;
  } else if (nm == "features") {
    base = te == 0 ? p.c0 : p.conv[te & 1]; width = c.conv_dim[te];
  } else if (nm == "logits") {
    base = p.logits; width = c.vocab;
  } else if (nm.compare(0, 6, "hidden") == 0 && nm.size() > 6) {
    char* end = nullptr;
    const long l = strtol(nm.c_str() + 6, &end, 10);
    if (*end != 0 || l < 0 || l > c.layers) return fail(VX_ERR_ARG, "vx_asr_read: unknown tap %s", name);
    if (!(c.flags & VX_ASR_KEEP_TAPS)) return fail(VX_ERR_STATE, "vx_asr_read: %s needs VX_ASR_KEEP_TAPS at create", name);
    base = p.hid + p.hid_stride * (size_t)l;
  } else {
    return fail(VX_ERR_ARG, "vx_asr_read: unknown tap %s", name);
  }
  const long lo = g->last_seg[(size_t)table * (n + 1) + utt], rows = (long)g->last_seg[(size_t)table * (n + 1) + utt + 1] - lo;
  if (n_floats != (int64_t)rows * width)
    return fail(VX_ERR_ARG, "vx_asr_read: %s of utterance %d is %ld x %d floats, not %lld", name, utt, rows, width, (long long)n_floats);
  DevGuard guard(g->device);
  HIPC(guard.err);
  HIPC(hipStreamSynchronize(g->last_stream));
  HIPC(hipMemcpy(dst, g->dev->ws.get() + base + (size_t)lo * width, (size_t)rows * width * sizeof(float), hipMemcpyDeviceToHost));
  return VX_OK;
}

extern "C" int vx_asr_get_timings(const vx_asr* g, double* out, int32_t n) {
  if (!g || !out || n < 0 || n > 4) return fail(VX_ERR_ARG, "vx_asr_get_timings: null argument or n outside [0, 4]");
  const double v[4] = {g->last_ms,
                       (double)(g->plan.total * sizeof(float) + g->plan.partial * sizeof(double) + (g->dev ? g->dev->fal_bytes : 0)),
                       (double)(g->packed.size() * sizeof(float)),
                       g->last_n ? (double)g->last_seg[(size_t)(g->cfg.n_conv - 1) * (g->last_n + 1) + g->last_n] : 0.0};
  for (int i = 0; i < n; ++i) out[i] = v[i];
  return VX_OK;
}

// ---- forced alignment and text likelihood -----------------------------------------------------------------------------------------
namespace {

constexpr long long FAL_MAX_BP_WORDS = 1ll << 29;  // 2 GiB of back-pointers a call

struct FalOut {
  double *nll, *path_logprob;
  int *frame_token, *tok_start, *tok_end;
  float* tok_score;
  int* feasible;
  bool any() const { return nll || path_logprob || frame_token || tok_start || tok_end || tok_score || feasible; }
  bool max_half() const { return path_logprob || frame_token || tok_start || tok_end || tok_score; }
};

// The utterance table and the layout of one call's scratch (bytes): utt | targets | lse | path | bp.
struct FalPlan {
  std::vector<FalUtt> utt;
  long rows = 0, toks = 0;
  long long bp_words = 0;
  int longest_S = 1;
  size_t o_tgt = 0, o_lse = 0, o_path = 0, o_bp = 0, bytes = 0;
};

// Every check of vx_falign / vx_falign_asr on the texts, before any HIP call.
int fal_plan(const char* what, int vocab, int blank, int n, const int* frames, const int32_t* targets, const int32_t* target_len, bool want_max,
             FalPlan& p) {
  p.utt.assign((size_t)n, FalUtt{});
  for (int i = 0; i < n; ++i) {
    if (frames[i] < 0 || target_len[i] < 0)
      return fail(VX_ERR_ARG, "%s: utterance %d: %d frames, %d targets", what, i, frames[i], target_len[i]);
    if (target_len[i] > 0 && !targets) return fail(VX_ERR_ARG, "%s: null targets", what);
    if (p.rows + frames[i] > 2147483647L || p.toks + target_len[i] > 2147483647L)
      return fail(VX_ERR_CAPACITY, "%s: more than 2^31 - 1 frames or targets", what);
    const int32_t* y = targets + p.toks;
    int repeats = 0;
    for (int k = 0; k < target_len[i]; ++k) {
      if (y[k] < 0 || y[k] >= vocab || y[k] == blank)
        return fail(VX_ERR_ARG, "%s: utterance %d: target %d is id %d (ids are in [0, %d) and not the blank %d)", what, i, k, y[k], vocab, blank);
      repeats += k > 0 && y[k] == y[k - 1];
    }
    FalUtt& u = p.utt[i];
    u.row0 = (int)p.rows; u.T = frames[i]; u.tok0 = (int)p.toks; u.L = target_len[i];
    u.feasible = (long)frames[i] >= (long)target_len[i] + repeats;
    u.bp_off = p.bp_words;
    p.rows += frames[i];
    p.toks += target_len[i];
  }
  for (int i = 0; i < n; ++i) {
    FalUtt& u = p.utt[i];
    if (!u.feasible || u.T == 0) continue;  // no lattice is walked
    if (u.L > FAL_MAX_L)
      return fail(VX_ERR_CAPACITY, "%s: utterance %d: %d targets, up to %d are served (four fp64 rows of 2 L + 3 cells in 64 KiB of LDS)", what, i,
                  u.L, FAL_MAX_L);
    p.longest_S = std::max(p.longest_S, 2 * u.L + 1);
    if (want_max) {
      u.bp_off = p.bp_words;
      p.bp_words += (long long)((u.T + 15) / 16) * (2 * u.L + 1);
      if (p.bp_words > FAL_MAX_BP_WORDS)
        return fail(VX_ERR_CAPACITY, "%s: utterance %d: the back-pointers (frames x states / 4 bytes, summed over the call) exceed the workspace limit of %lld bytes",
                    what, i, FAL_MAX_BP_WORDS * 4);
    }
  }
  auto up = [](size_t v) { return (v + 15) / 16 * 16; };
  p.o_tgt = up((size_t)n * sizeof(FalUtt));
  p.o_lse = p.o_tgt + up((size_t)(p.toks + 1) * sizeof(int));
  p.o_path = p.o_lse + up((size_t)(p.rows + 1) * sizeof(double));
  p.o_bp = p.o_path + up((size_t)(p.rows + 1) * sizeof(int));
  p.bytes = p.o_bp + up((size_t)(p.bp_words + 1) * sizeof(unsigned));
  return VX_OK;
}

// The launches: `scratch` holds p.bytes.  The host arrays are copied before the call returns (the caller waits for `s`).
int fal_launch(const float* logits, int vocab, int blank, int n, const int32_t* targets, const FalPlan& p, unsigned char* scratch,
               const FalOut& o, hipStream_t s) {
  HIPC(hipMemcpyAsync(scratch, p.utt.data(), (size_t)n * sizeof(FalUtt), hipMemcpyHostToDevice, s));
  if (p.toks > 0) HIPC(hipMemcpyAsync(scratch + p.o_tgt, targets, (size_t)p.toks * sizeof(int), hipMemcpyHostToDevice, s));
  double* lse = (double*)(scratch + p.o_lse);
  if (p.rows > 0) {
    falign_lse_kernel<<<(unsigned)((p.rows + 3) / 4), 256, 0, s>>>(logits, vocab, p.rows, lse);
    HIPC(hipGetLastError());
  }
  FalArgs a{};
  a.logits = logits; a.lse = lse; a.utt = (const FalUtt*)scratch; a.targets = (const int*)(scratch + p.o_tgt);
  a.bp = (unsigned*)(scratch + p.o_bp); a.path = (int*)(scratch + p.o_path);
  a.nll = o.nll; a.path_logprob = o.path_logprob; a.frame_token = o.frame_token; a.tok_start = o.tok_start; a.tok_end = o.tok_end;
  a.tok_score = o.tok_score; a.feasible = o.feasible;
  a.vocab = vocab; a.blank = blank; a.row_stride = p.longest_S + 2; a.do_max = o.max_half() ? 1 : 0;
  falign_kernel<<<(unsigned)n, FAL_WG, 4 * (size_t)a.row_stride * sizeof(double), s>>>(a);
  HIPC(hipGetLastError());
  return VX_OK;
}

}  // namespace

extern "C" int vx_falign(const float* logits, int32_t vocab, int32_t blank, int32_t n, const int32_t* frames, const int32_t* targets,
                         const int32_t* target_len, double* nll_out, double* path_logprob_out, int32_t* frame_token_out,
                         int32_t* tok_start_out, int32_t* tok_end_out, float* tok_score_out, int32_t* feasible_out, void* stream) {
  if (!logits || !frames || !target_len) return fail(VX_ERR_ARG, "vx_falign: null argument");
  const FalOut o{nll_out, path_logprob_out, frame_token_out, tok_start_out, tok_end_out, tok_score_out, feasible_out};
  if (!o.any()) return fail(VX_ERR_ARG, "vx_falign: no output requested");
  if (n < 1 || vocab < 1 || blank < 0 || blank >= vocab) return fail(VX_ERR_ARG, "vx_falign: n %d, vocab %d, blank %d", n, vocab, blank);
  FalPlan p;
  VXC(fal_plan("vx_falign", vocab, blank, n, frames, targets, target_len, o.max_half(), p));
  hipStream_t s = (hipStream_t)stream;
  DevBuf<unsigned char> scratch;
  VXC(scratch.alloc(p.bytes));
  VXC(fal_launch(logits, vocab, blank, n, targets, p, scratch.get(), o, s));
  HIPC(hipStreamSynchronize(s));  // the scratch and the host tables go out of scope
  return VX_OK;
}

extern "C" int vx_falign_asr(vx_asr* g, int32_t n, const int32_t* targets, const int32_t* target_len, double* nll_out,
                             double* path_logprob_out, int32_t* frame_token_out, int32_t* tok_start_out, int32_t* tok_end_out,
                             float* tok_score_out, int32_t* feasible_out, void* stream) {
  if (!g || !target_len) return fail(VX_ERR_ARG, "vx_falign_asr: null argument");
  const FalOut o{nll_out, path_logprob_out, frame_token_out, tok_start_out, tok_end_out, tok_score_out, feasible_out};
  if (!o.any()) return fail(VX_ERR_ARG, "vx_falign_asr: no output requested");
  if (n < 1) return fail(VX_ERR_ARG, "vx_falign_asr: n = %d utterances", n);
  if (g->device < 0 || g->last_n == 0) return fail(VX_ERR_STATE, "vx_falign_asr before any vx_asr_recognize");
  if (n != g->last_n) return fail(VX_ERR_STATE, "vx_falign_asr: n = %d utterances, the last vx_asr_recognize served %d", n, g->last_n);
  const vx_asr_config& c = g->cfg;
  const int* seg = g->last_seg.data() + (size_t)(c.n_conv - 1) * (n + 1);
  std::vector<int> frames((size_t)n);
  for (int i = 0; i < n; ++i) frames[i] = seg[i + 1] - seg[i];
  FalPlan p;
  VXC(fal_plan("vx_falign_asr", c.vocab, c.blank, n, frames.data(), targets, target_len, o.max_half(), p));
  DevGuard guard(g->device);
  HIPC(guard.err);
  AsrDev& dv = *g->dev;
  hipStream_t s = (hipStream_t)stream;
  HIPC(hipStreamWaitEvent(s, dv.stage.ev_done, 0));  // the logits of the last call, whatever stream it ran on
  if (p.bytes > dv.fal_bytes) {
    dv.fal_bytes = 0;
    VXC(dv.fal.alloc(p.bytes));
    dv.fal_bytes = p.bytes;
  }
  VXC(fal_launch(dv.ws.get() + g->plan.logits, c.vocab, c.blank, n, targets, p, dv.fal.get(), o, s));
  HIPC(hipStreamSynchronize(s));  // the host tables go out of scope, and the next call may replace the scratch
  return VX_OK;
}

// ---- the decode and the distance on their own -----------------------------------------------------------------------------------
extern "C" int vx_ctc_greedy(const float* logits, int32_t vocab, int32_t blank, int32_t n, const int32_t* frames, int32_t* tokens_out,
                             int32_t* token_frames_out, int32_t* counts_out, float* mean_logprob_out, float* frame_logprob_out,
                             void* stream) {
  if (!logits || !frames || !tokens_out || !token_frames_out || !counts_out || !mean_logprob_out)
    return fail(VX_ERR_ARG, "vx_ctc_greedy: null argument");
  if (n < 1 || vocab < 1 || blank < 0 || blank >= vocab) return fail(VX_ERR_ARG, "vx_ctc_greedy: n %d, vocab %d, blank %d", n, vocab, blank);
  std::vector<int> seg((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) {
    if (frames[i] < 0) return fail(VX_ERR_ARG, "vx_ctc_greedy: utterance %d: %d frames", i, frames[i]);
    if ((long)seg[i] + frames[i] > 2147483647L) return fail(VX_ERR_CAPACITY, "vx_ctc_greedy: more than 2^31 - 1 frames");
    seg[i + 1] = seg[i] + frames[i];
  }
  const long M = seg[n];
  hipStream_t s = (hipStream_t)stream;
  DevBuf<int> dseg, ids;
  DevBuf<double> lp;
  VXC(dseg.alloc((size_t)n + 1));
  VXC(ids.alloc((size_t)M + 1));
  VXC(lp.alloc((size_t)M + 1));
  HIPC(hipMemcpyAsync(dseg.get(), seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice, s));
  VXC(launch_ctc(logits, vocab, blank, n, M, dseg.get(), ids.get(), lp.get(), tokens_out, token_frames_out, counts_out, mean_logprob_out,
                 frame_logprob_out, s));
  HIPC(hipStreamSynchronize(s));  // the scratch and `seg` go out of scope
  return VX_OK;
}

extern "C" int vx_edit_distance(int32_t n, const int32_t* ref, const int32_t* ref_len, const int32_t* hyp, const int32_t* hyp_len,
                                int32_t* out, void* stream) {
  if (!ref_len || !hyp_len || !out) return fail(VX_ERR_ARG, "vx_edit_distance: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_edit_distance: n = %d pairs", n);
  std::vector<EditPair> pairs((size_t)n);
  long ro = 0, ho = 0;
  int longest = 0;
  for (int i = 0; i < n; ++i) {
    if (ref_len[i] < 0 || hyp_len[i] < 0) return fail(VX_ERR_ARG, "vx_edit_distance: pair %d: lengths %d and %d", i, ref_len[i], hyp_len[i]);
    if (ref_len[i] > EDIT_MAX_LEN || hyp_len[i] > EDIT_MAX_LEN)
      return fail(VX_ERR_ARG, "vx_edit_distance: pair %d: lengths %d and %d, up to %d tokens a side are served", i, ref_len[i], hyp_len[i],
                  EDIT_MAX_LEN);
    if (ro > 2147483647L - EDIT_MAX_LEN || ho > 2147483647L - EDIT_MAX_LEN) return fail(VX_ERR_CAPACITY, "vx_edit_distance: more than 2^31 - 1 tokens");
    pairs[i] = EditPair{(int)ro, ref_len[i], (int)ho, hyp_len[i]};
    ro += ref_len[i];
    ho += hyp_len[i];
    longest = std::max(longest, ref_len[i]);
  }
  if ((ro > 0 && !ref) || (ho > 0 && !hyp)) return fail(VX_ERR_ARG, "vx_edit_distance: null sequence");
  hipStream_t s = (hipStream_t)stream;
  DevBuf<EditPair> dp;
  VXC(dp.alloc((size_t)n));
  HIPC(hipMemcpyAsync(dp.get(), pairs.data(), pairs.size() * sizeof(EditPair), hipMemcpyHostToDevice, s));
  const int stride = longest + 1;
  edit_distance_kernel<<<(unsigned)n, EDIT_WG, 3 * (size_t)stride * sizeof(unsigned long long), s>>>(ref, hyp, dp.get(), stride, out);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));  // the pair table goes out of scope
  return VX_OK;
}
