// Speaker encoder (WavLM / Wav2Vec2 x-vector network) behind the C ABI (include/vallex.h, vx_spk_*): the weight table and its
// packing for the row GEMM, the per-head bias table, the staging of a ragged call (CallStage, host.hpp), the workspace and the
// launches of spk_kernels.hpp.  A translation unit and a handle of its own, like ganvoc.hip; the packing and the launches of the kernels
// the recogniser (asr.hip) runs too are in spk_host.hpp.
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

using namespace vx;

namespace {

struct SpkLayer {
  SpkLin qkv, out, ff1, ff2;
  SpkNorm ln1, ln2;
  size_t gw = 0, gb = 0, gc = 0;
};

struct SpkDev {
  DevBuf<float> w;   // every packed tensor
  DevBuf<float> ws;  // the workspace, carved by offsets (SpkPlan)
  DevBuf<double> partial;
  // per call: wav pointers [max_batch] | n_samples [max_batch] | segment tables [n_tables][max_batch + 1]
  CallStage stage;
};

// Offsets (floats) into the workspace.
struct SpkPlan {
  size_t conv[2] = {0, 0}, fpn = 0, x0 = 0, hid = 0, hid_stride = 0, mid = 0, qkv = 0, att = 0, tmp = 0, ff = 0, gate = 0, sum = 0, td[2] = {0, 0},
         pooled = 0, cstats = 0, nstats = 0, total = 0;
  size_t partial = 0;  // doubles
};

}  // namespace

struct vx_spk {
  vx_spk_config cfg{};
  std::map<std::string, HostW> w;
  std::vector<int32_t> buckets;
  bool finalized = false;
  int hd = 0, Tmax = 0;
  long min_samples = 0;
  SpkPlan plan;
  // filled by vx_spk_finalize
  std::vector<float> packed;
  size_t c0w = 0, c0b = 0, gnw = 0, gnb = 0, table = 0;
  SpkLin conv[8], proj, pos, projector, tdnn[8], fe, cls;
  SpkNorm fp_ln, enc_ln;
  std::vector<SpkLayer> layers;
  std::vector<float> lw;  // softmax(layer_weights)
  int device = -1;        // >= 0: `dev` is complete
  std::unique_ptr<SpkDev> dev;
  // the last call, for vx_spk_read
  std::vector<int> last_seg;  // [n_tables][n + 1]
  int last_n = 0;
  hipStream_t last_stream = nullptr;
  double last_ms = 0.0;
};

namespace {

int n_tables(const vx_spk_config& c) { return c.n_conv + c.n_tdnn; }

long frames_of(const vx_spk_config& c, long L, int upto) {  // frames after conv layers 0 .. upto
  for (int i = 0; i <= upto; ++i) L = L >= c.conv_kernel[i] ? (L - c.conv_kernel[i]) / c.conv_stride[i] + 1 : 0;
  return L;
}

long tdnn_frames(const vx_spk_config& c, long T, int upto) {
  for (int i = 0; i <= upto; ++i) T = std::max(0L, T - (long)c.tdnn_dilation[i] * (c.tdnn_kernel[i] - 1));
  return T;
}

struct CallCtx : SpkCall {
  const vx_spk* g;
  float* ws;
};

void make_plan(vx_spk* g) {
  const vx_spk_config& c = g->cfg;
  SpkPlan& p = g->plan;
  const size_t B = (size_t)c.max_batch;
  size_t at = 0;
  auto take = [&](size_t n) { const size_t o = at; at += (n + 3) / 4 * 4; return o; };
  size_t cv[2] = {0, 0};
  for (int i = 0; i < c.n_conv; ++i) cv[i & 1] = std::max(cv[i & 1], B * (size_t)frames_of(c, c.max_samples, i) * c.conv_dim[i]);
  p.conv[0] = take(cv[0]);
  p.conv[1] = take(cv[1]);
  const size_t rows = B * (size_t)g->Tmax, d = (size_t)c.hidden;
  p.fpn = take(rows * (size_t)c.conv_dim[c.n_conv - 1]);
  p.x0 = take(rows * d);
  p.hid_stride = (rows * d + 3) / 4 * 4;
  p.hid = take(p.hid_stride * ((c.flags & VX_SPK_KEEP_TAPS) ? (size_t)c.layers + 1 : 2));
  p.mid = take(rows * d);
  p.qkv = take(rows * 3 * d);
  p.att = take(rows * d);
  p.tmp = take(rows * d);
  p.ff = take(rows * (size_t)c.ffn);
  p.gate = take((size_t)c.layers * rows * c.heads);
  p.sum = take(rows * d);
  size_t widest = 0;
  for (int i = 0; i < c.n_tdnn; ++i) widest = std::max(widest, (size_t)c.tdnn_dim[i]);
  p.td[0] = take(rows * widest);
  p.td[1] = take(rows * widest);
  p.pooled = take(B * 2 * (size_t)c.tdnn_dim[c.n_tdnn - 1]);
  p.cstats = take(B * (size_t)c.conv_dim[0] * 2);
  p.nstats = take(B * 2);
  p.total = at;
  const size_t t0 = (size_t)frames_of(c, c.max_samples, 0);
  p.partial = B * ((t0 + SPK_C0_TT - 1) / SPK_C0_TT) * (size_t)c.conv_dim[0] * 2;
}

int spk_init_device(vx_spk* g) {
  int dev = 0;
  HIPC(hipGetDevice(&dev));
  g->device = dev;
  g->dev.reset(new SpkDev());
  SpkDev& d = *g->dev;
  const size_t MB = (size_t)g->cfg.max_batch;
  VXC(d.w.alloc(g->packed.size() + 4));
  HIPC(hipMemcpy(d.w.get(), g->packed.data(), g->packed.size() * sizeof(float), hipMemcpyHostToDevice));
  VXC(d.ws.alloc(g->plan.total + 4));
  VXC(d.partial.alloc(g->plan.partial + 2));
  VXC(d.stage.init(MB * sizeof(void*) + MB * sizeof(int) + (size_t)n_tables(g->cfg) * (MB + 1) * sizeof(int)));
  return VX_OK;
}

int run_call(const CallCtx& x, const float* const* wav, const int* n_samples_dev, const int* hseg, int flags, float* emb_out,
             float* logits_out) {
  const vx_spk* g = x.g;
  const vx_spk_config& c = g->cfg;
  const SpkPlan& p = g->plan;
  const int n = x.n, MB = x.MB, d = c.hidden, H = c.heads;
  auto rows_of = [&](int t) { return (long)hseg[(size_t)t * (MB + 1) + n]; };
  float* ws = x.ws;
  // ---- feature encoder
  float* nstats = nullptr;
  if (flags & VX_SPK_NORMALIZE) {
    nstats = ws + p.nstats;
    spk_wave_stats<<<n, 256, 0, x.s>>>(wav, n_samples_dev, nstats);
    HIPC(hipGetLastError());
  }
  {
    SpkConv0Args a{};
    a.wav = wav; a.nstats = nstats; a.w = x.W + g->c0w; a.bias = c.conv_bias ? x.W + g->c0b : nullptr;
    a.gn_w = x.W + g->gnw; a.gn_b = x.W + g->gnb; a.partial = g->dev->partial.get(); a.cstats = ws + p.cstats; a.out = ws + p.conv[0];
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
  for (int i = 1; i < c.n_conv; ++i)
    VXC(run_lin(x, g->conv[i], ws + p.conv[(i - 1) & 1], c.conv_dim[i - 1], ws + p.conv[i & 1], rows_of(i), SPK_ACT_GELU, i, i - 1));
  const int te = c.n_conv - 1;  // the encoder's table
  const long M = rows_of(te);
  const float* feats = ws + p.conv[te & 1];
  const int Cl = c.conv_dim[te];
  // ---- projection, positional convolution, hidden state 0
  VXC(run_ln(x, g->fp_ln, feats, nullptr, ws + p.fpn, M, Cl));
  VXC(run_lin(x, g->proj, ws + p.fpn, Cl, ws + p.x0, M, SPK_ACT_NONE));
  VXC(run_lin(x, g->pos, ws + p.x0, d, ws + p.tmp, M, SPK_ACT_GELU, te, te));
  const bool keep = (c.flags & VX_SPK_KEEP_TAPS) != 0, wsum = c.use_weighted_layer_sum != 0;
  auto hid = [&](int l) { return ws + p.hid + p.hid_stride * (size_t)(keep ? l : (l & 1)); };
  float* sum = wsum ? ws + p.sum : nullptr;
  VXC(run_ln(x, g->enc_ln, ws + p.x0, ws + p.tmp, hid(0), M, d, sum, wsum ? g->lw[0] : 0.f, 1));
  // ---- encoder layers
  const int* et = hseg + (size_t)te * (MB + 1);
  const bool wavlm = c.attention == VX_SPK_WAVLM;
  for (int l = 0; l < c.layers; ++l) {
    const SpkLayer& L = g->layers[l];
    const float* h = hid(l);
    float* gate = ws + p.gate + (size_t)l * (size_t)MB * g->Tmax * H;
    if (wavlm) {
      spk_gate<<<(unsigned)((M * H + 255) / 256), 256, 0, x.s>>>(h, x.W + L.gw, x.W + L.gb, x.W + L.gc, gate, M, H, g->hd);
      HIPC(hipGetLastError());
    }
    VXC(run_lin(x, L.qkv, h, d, ws + p.qkv, M, SPK_ACT_NONE));
    VXC(run_attn(x, x.table(te), et, ws + p.qkv, wavlm ? gate : nullptr, wavlm ? x.W + g->table : nullptr, ws + p.att, H, d, g->hd,
                 g->Tmax));
    VXC(run_lin(x, L.out, ws + p.att, d, ws + p.tmp, M, SPK_ACT_NONE));
    VXC(run_ln(x, L.ln1, h, ws + p.tmp, ws + p.mid, M, d));
    VXC(run_lin(x, L.ff1, ws + p.mid, d, ws + p.ff, M, SPK_ACT_GELU));
    VXC(run_lin(x, L.ff2, ws + p.ff, c.ffn, ws + p.tmp, M, SPK_ACT_NONE));
    VXC(run_ln(x, L.ln2, ws + p.mid, ws + p.tmp, hid(l + 1), M, d, sum, wsum ? g->lw[l + 1] : 0.f, 0));
  }
  // ---- head
  const float* top = wsum ? ws + p.sum : hid(c.layers);
  VXC(run_lin(x, g->projector, top, d, ws + p.td[0], M, SPK_ACT_NONE));
  int cur = 0, cin = c.tdnn_dim[0];
  for (int i = 0; i < c.n_tdnn; ++i) {
    VXC(run_lin(x, g->tdnn[i], ws + p.td[cur], cin, ws + p.td[cur ^ 1], rows_of(c.n_conv + i), SPK_ACT_RELU, c.n_conv + i,
                i == 0 ? te : c.n_conv + i - 1));
    cur ^= 1;
    cin = c.tdnn_dim[i];
  }
  spk_pool<<<dim3((unsigned)((cin + 255) / 256), (unsigned)n), 256, 0, x.s>>>(ws + p.td[cur], ws + p.pooled, x.table(c.n_conv + c.n_tdnn - 1), cin);
  HIPC(hipGetLastError());
  VXC(run_lin(x, g->fe, ws + p.pooled, 2 * cin, emb_out, n, SPK_ACT_NONE));
  if (logits_out) VXC(run_lin(x, g->cls, emb_out, c.xvector, logits_out, n, SPK_ACT_NONE));
  return VX_OK;
}

}  // namespace

extern "C" int64_t vx_spk_frames(const vx_spk* g, int64_t n_samples) {
  return !g ? -1 : (int64_t)frames_of(g->cfg, (long)std::max<int64_t>(0, n_samples), g->cfg.n_conv - 1);
}

extern "C" int64_t vx_spk_min_samples(const vx_spk* g) { return !g ? -1 : (int64_t)g->min_samples; }

extern "C" int vx_spk_create(const vx_spk_config* cfg, vx_spk** out) {
  if (!cfg || !out) return fail(VX_ERR_ARG, "vx_spk_create: null argument");
  if (cfg->struct_size != (int32_t)sizeof(vx_spk_config))
    return fail(VX_ERR_ARG, "vx_spk_create: struct_size %d, expected %zu", cfg->struct_size, sizeof(vx_spk_config));
  const vx_spk_config& c = *cfg;
  if (c.attention != VX_SPK_WAVLM && c.attention != VX_SPK_PLAIN) return fail(VX_ERR_ARG, "vx_spk_create: attention = %d", c.attention);
  if (c.hidden < 1 || c.layers < 1 || c.heads < 1 || c.ffn < 1 || c.layers > 256)
    return fail(VX_ERR_ARG, "vx_spk_create: hidden %d, layers %d, heads %d, ffn %d", c.hidden, c.layers, c.heads, c.ffn);
  if (c.n_conv < 1 || c.n_conv > 8) return fail(VX_ERR_ARG, "vx_spk_create: n_conv = %d outside [1, 8]", c.n_conv);
  if (c.n_tdnn < 1 || c.n_tdnn > 8) return fail(VX_ERR_ARG, "vx_spk_create: n_tdnn = %d outside [1, 8]", c.n_tdnn);
  for (int i = 0; i < c.n_conv; ++i)
    if (c.conv_dim[i] < 1 || c.conv_kernel[i] < 1 || c.conv_stride[i] < 1)
      return fail(VX_ERR_ARG, "vx_spk_create: conv layer %d: dim %d, kernel %d, stride %d", i, c.conv_dim[i], c.conv_kernel[i], c.conv_stride[i]);
  for (int i = 0; i < c.n_tdnn; ++i)
    if (c.tdnn_dim[i] < 1 || c.tdnn_kernel[i] < 1 || c.tdnn_dilation[i] < 1)
      return fail(VX_ERR_ARG, "vx_spk_create: tdnn layer %d: dim %d, kernel %d, dilation %d", i, c.tdnn_dim[i], c.tdnn_kernel[i], c.tdnn_dilation[i]);
  if (c.pos_kernel < 1 || c.pos_groups < 1 || c.xvector < 1 || c.num_buckets < 0)
    return fail(VX_ERR_ARG, "vx_spk_create: pos_kernel %d, pos_groups %d, xvector %d, num_buckets %d", c.pos_kernel, c.pos_groups, c.xvector, c.num_buckets);
  if (c.attention == VX_SPK_WAVLM && c.num_buckets < 1) return fail(VX_ERR_ARG, "vx_spk_create: num_buckets = %d", c.num_buckets);
  if (c.hidden % c.heads != 0) return fail(VX_ERR_ARG, "vx_spk_create: heads = %d does not divide hidden = %d", c.heads, c.hidden);
  if (c.hidden % c.pos_groups != 0) return fail(VX_ERR_ARG, "vx_spk_create: pos_groups = %d does not divide hidden = %d", c.pos_groups, c.hidden);
  if (c.max_batch < 1) return fail(VX_ERR_ARG, "vx_spk_create: max_batch = %d", c.max_batch);
  if (!isfinite(c.layer_norm_eps) || c.layer_norm_eps < 0.f) return fail(VX_ERR_ARG, "vx_spk_create: layer_norm_eps = %g", c.layer_norm_eps);
  if (c.flags & ~VX_SPK_KEEP_TAPS) return fail(VX_ERR_ARG, "vx_spk_create: flags = %d", c.flags);
  if (c.feat_extract_norm != 0) return fail(VX_ERR_UNSUPPORTED, "vx_spk_create: feat_extract_norm = \"layer\" (\"group\" is served)");
  if (c.do_stable_layer_norm != 0) return fail(VX_ERR_UNSUPPORTED, "vx_spk_create: do_stable_layer_norm (the post-norm encoder is served)");
  if (c.add_adapter != 0) return fail(VX_ERR_UNSUPPORTED, "vx_spk_create: add_adapter");
  if (c.activation != 0) return fail(VX_ERR_UNSUPPORTED, "vx_spk_create: activation = %d (gelu is served)", c.activation);
  const int hd = c.hidden / c.heads;
  if (hd != 16 && hd != 32 && hd != 64)
    return fail(VX_ERR_UNSUPPORTED, "vx_spk_create: head_dim = %d (16, 32 and 64 are served)", hd);
  if (c.conv_kernel[0] > SPK_C0_MAXK || c.conv_stride[0] > 32)
    return fail(VX_ERR_UNSUPPORTED, "vx_spk_create: conv layer 0: kernel %d, stride %d (up to %d and 32 are served)", c.conv_kernel[0],
                c.conv_stride[0], SPK_C0_MAXK);
  if (c.max_batch > SPK_MAX_SEG) return fail(VX_ERR_UNSUPPORTED, "vx_spk_create: max_batch = %d > %d", c.max_batch, SPK_MAX_SEG);

  std::unique_ptr<vx_spk> g(new vx_spk());
  g->cfg = c;
  g->hd = hd;
  long need = 2;
  for (int i = 0; i < c.n_tdnn; ++i) need += (long)c.tdnn_dilation[i] * (c.tdnn_kernel[i] - 1);
  for (int i = c.n_conv - 1; i >= 0; --i) need = std::min((need - 1) * c.conv_stride[i] + c.conv_kernel[i], 1L << 40);
  g->min_samples = need;
  if (c.max_samples < need)
    return fail(VX_ERR_ARG, "vx_spk_create: max_samples = %d below the shortest utterance served, %ld samples", c.max_samples, need);
  g->Tmax = (int)frames_of(c, c.max_samples, c.n_conv - 1);
  // every row buffer is indexed by rows x columns in the kernels' long arithmetic, but the segment tables are int32
  const double rows0 = (double)c.max_batch * (double)frames_of(c, c.max_samples, 0);
  if (rows0 > 2147483647.0) return fail(VX_ERR_UNSUPPORTED, "vx_spk_create: max_batch x layer-0 frames = %.0f rows exceed int32", rows0);
  make_plan(g.get());

  const int d = c.hidden, L = c.layers;
  for (int i = 0; i < c.n_conv; ++i) {
    const std::string cv = "feature_extractor.conv_layers." + std::to_string(i) + ".conv";
    add_key(g.get(), cv + ".weight", {c.conv_dim[i], i == 0 ? 1 : c.conv_dim[i - 1], c.conv_kernel[i]});
    if (c.conv_bias) add_key(g.get(), cv + ".bias", {c.conv_dim[i]});
  }
  auto norm_keys = [&](const std::string& nm, int dim) {
    add_key(g.get(), nm + ".weight", {dim});
    add_key(g.get(), nm + ".bias", {dim});
  };
  auto lin_keys = [&](const std::string& nm, int N, int K) {
    add_key(g.get(), nm + ".weight", {N, K});
    add_key(g.get(), nm + ".bias", {N});
  };
  const int Cl = c.conv_dim[c.n_conv - 1];
  norm_keys("feature_extractor.conv_layers.0.layer_norm", c.conv_dim[0]);
  norm_keys("feature_projection.layer_norm", Cl);
  lin_keys("feature_projection.projection", d, Cl);
  add_key(g.get(), "encoder.pos_conv_embed.conv.weight", {d, d / c.pos_groups, c.pos_kernel});
  add_key(g.get(), "encoder.pos_conv_embed.conv.bias", {d});
  norm_keys("encoder.layer_norm", d);
  for (int l = 0; l < L; ++l) {
    const std::string pre = "encoder.layers." + std::to_string(l) + ".";
    for (const char* nm : {"q_proj", "k_proj", "v_proj", "out_proj"}) lin_keys(pre + "attention." + nm, d, d);
    if (c.attention == VX_SPK_WAVLM) {
      lin_keys(pre + "attention.gru_rel_pos_linear", 8, hd);
      add_key(g.get(), pre + "attention.gru_rel_pos_const", {1, c.heads, 1, 1});
    }
    norm_keys(pre + "layer_norm", d);
    lin_keys(pre + "feed_forward.intermediate_dense", c.ffn, d);
    lin_keys(pre + "feed_forward.output_dense", d, c.ffn);
    norm_keys(pre + "final_layer_norm", d);
  }
  if (c.attention == VX_SPK_WAVLM) add_key(g.get(), "encoder.layers.0.attention.rel_attn_embed.weight", {c.num_buckets, c.heads});
  if (c.use_weighted_layer_sum) add_key(g.get(), "layer_weights", {L + 1});
  lin_keys("projector", c.tdnn_dim[0], d);
  int cin = c.tdnn_dim[0];
  for (int i = 0; i < c.n_tdnn; ++i) {
    lin_keys("tdnn." + std::to_string(i) + ".kernel", c.tdnn_dim[i], cin * c.tdnn_kernel[i]);
    cin = c.tdnn_dim[i];
  }
  lin_keys("feature_extractor", c.xvector, 2 * cin);
  lin_keys("classifier", c.xvector, c.xvector);
  *out = g.release();
  return VX_OK;
}

extern "C" void vx_spk_destroy(vx_spk* g) {
  if (!g) return;
  if (g->device >= 0) {
    DevGuard guard(g->device);
    (void)g->dev->stage.drain();
    g->dev.reset();
  }
  delete g;
}

extern "C" int vx_spk_set_weight(vx_spk* g, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
  return set_weight(g, "vx_spk", key, data, shape, ndim);
}

extern "C" int vx_spk_set_buckets(vx_spk* g, const int32_t* idx, int32_t n) {
  if (!g || !idx) return fail(VX_ERR_ARG, "vx_spk_set_buckets: null argument");
  if (g->finalized) return fail(VX_ERR_STATE, "vx_spk_set_buckets after vx_spk_finalize");
  if (n != 2 * g->Tmax - 1) return fail(VX_ERR_ARG, "vx_spk_set_buckets: %d indices, expected 2 x %d - 1", n, g->Tmax);
  for (int i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= g->cfg.num_buckets)
      return fail(VX_ERR_ARG, "vx_spk_set_buckets: index %d at relative position %d outside [0, %d)", idx[i], i - (g->Tmax - 1),
                  g->cfg.num_buckets);
  g->buckets.assign(idx, idx + n);
  return VX_OK;
}

extern "C" int vx_spk_finalize(vx_spk* g) {
  if (!g) return fail(VX_ERR_ARG, "vx_spk_finalize: null handle");
  if (g->finalized) return VX_OK;
  for (auto& kv : g->w)
    if (!kv.second.set) return fail(VX_ERR_WEIGHTS, "missing tensor %s", kv.first.c_str());
  const vx_spk_config& c = g->cfg;
  const bool wavlm = c.attention == VX_SPK_WAVLM;
  if (wavlm && g->buckets.empty()) return fail(VX_ERR_STATE, "vx_spk_finalize: vx_spk_set_buckets has not been called");
  const int d = c.hidden, H = c.heads, L = c.layers;
  g->packed.clear();
  const std::string c0 = "feature_extractor.conv_layers.0.";
  g->c0w = push(g->packed, g->w[c0 + "conv.weight"].data);
  if (c.conv_bias) g->c0b = push(g->packed, g->w[c0 + "conv.bias"].data);
  g->gnw = push(g->packed, g->w[c0 + "layer_norm.weight"].data);
  g->gnb = push(g->packed, g->w[c0 + "layer_norm.bias"].data);
  for (int i = 1; i < c.n_conv; ++i) {
    g->conv[i] = pack_conv(g, "feature_extractor.conv_layers." + std::to_string(i) + ".conv", c.conv_dim[i], c.conv_dim[i - 1],
                           c.conv_kernel[i], 1, c.conv_bias != 0);
    g->conv[i].stride = c.conv_stride[i];
  }
  const int Cl = c.conv_dim[c.n_conv - 1];
  g->fp_ln = pack_norm(g, "feature_projection.layer_norm");
  g->proj = pack_linear(g, "feature_projection.projection", d, Cl);
  g->pos = pack_conv(g, "encoder.pos_conv_embed.conv", d, d / c.pos_groups, c.pos_kernel, c.pos_groups, true);
  g->pos.off0 = -(c.pos_kernel / 2);  // padding k / 2; outputs 0 .. T - 1 (an even k's extra last frame is never formed)
  g->enc_ln = pack_norm(g, "encoder.layer_norm");
  g->layers.assign(L, SpkLayer());
  for (int l = 0; l < L; ++l) {
    const std::string pre = "encoder.layers." + std::to_string(l) + ".";
    SpkLayer& ly = g->layers[l];
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
    if (wavlm) {
      ly.gw = push(g->packed, g->w[pre + "attention.gru_rel_pos_linear.weight"].data);
      ly.gb = push(g->packed, g->w[pre + "attention.gru_rel_pos_linear.bias"].data);
      ly.gc = push(g->packed, g->w[pre + "attention.gru_rel_pos_const"].data);
    }
  }
  if (wavlm) {  // bias[h][r + Tmax - 1] = rel_attn_embed[bucket(r)][h]
    const HostW& e = g->w["encoder.layers.0.attention.rel_attn_embed.weight"];
    const size_t R = 2 * (size_t)g->Tmax - 1;
    std::vector<float> tab((size_t)H * R);
    for (int h = 0; h < H; ++h)
      for (size_t r = 0; r < R; ++r) tab[(size_t)h * R + r] = e.data[(size_t)g->buckets[r] * H + h];
    g->table = push(g->packed, tab);
  }
  g->lw.assign(L + 1, 0.f);
  if (c.use_weighted_layer_sum) {
    const HostW& w = g->w["layer_weights"];
    double mx = -INFINITY, den = 0.0;
    for (float v : w.data) mx = std::max(mx, (double)v);
    for (float v : w.data) den += exp((double)v - mx);
    for (int l = 0; l <= L; ++l) g->lw[l] = (float)(exp((double)w.data[l] - mx) / den);
  }
  g->projector = pack_linear(g, "projector", c.tdnn_dim[0], d);
  int cin = c.tdnn_dim[0];
  for (int i = 0; i < c.n_tdnn; ++i) {
    SpkLin t = pack_linear(g, "tdnn." + std::to_string(i) + ".kernel", c.tdnn_dim[i], cin * c.tdnn_kernel[i]);
    t.C = cin; t.taps = c.tdnn_kernel[i]; t.step = c.tdnn_dilation[i];
    g->tdnn[i] = t;
    cin = c.tdnn_dim[i];
  }
  g->fe = pack_linear(g, "feature_extractor", c.xvector, 2 * cin);
  g->cls = pack_linear(g, "classifier", c.xvector, c.xvector);
  for (auto& kv : g->w) std::vector<float>().swap(kv.second.data);  // the packed copy is the one that is kept
  g->finalized = true;
  return VX_OK;
}

extern "C" int vx_spk_embed(vx_spk* g, int32_t n, const float* const* wav, const int32_t* n_samples, int32_t flags, float* emb_out,
                            float* logits_out, void* stream) {
  if (!g || !wav || !n_samples || !emb_out) return fail(VX_ERR_ARG, "vx_spk_embed: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_spk_embed: n = %d utterances", n);
  if (flags & ~VX_SPK_NORMALIZE) return fail(VX_ERR_ARG, "vx_spk_embed: flags = %d", flags);
  if (!g->finalized) return fail(VX_ERR_STATE, "vx_spk_embed before vx_spk_finalize");
  const vx_spk_config& c = g->cfg;
  if (n > c.max_batch) return fail(VX_ERR_CAPACITY, "vx_spk_embed: n = %d utterances > max_batch %d", n, c.max_batch);
  for (int i = 0; i < n; ++i) {
    if (!wav[i]) return fail(VX_ERR_ARG, "vx_spk_embed: utterance %d: null pointer", i);
    if (n_samples[i] < g->min_samples)
      return fail(VX_ERR_ARG, "vx_spk_embed: utterance %d: %d samples, the shortest served is %ld (two pooled frames)", i, n_samples[i],
                  g->min_samples);
    if (n_samples[i] > c.max_samples)
      return fail(VX_ERR_CAPACITY, "vx_spk_embed: utterance %d: %d samples > max_samples %d", i, n_samples[i], c.max_samples);
  }
  const auto t_begin = std::chrono::steady_clock::now();
  if (g->device < 0) {
    const int rc = spk_init_device(g);
    if (rc != VX_OK) {  // a failed first use leaves the handle as it was before it
      g->dev.reset();
      g->device = -1;
      return rc;
    }
  }
  DevGuard guard(g->device);
  HIPC(guard.err);
  SpkDev& dv = *g->dev;
  hipStream_t s = (hipStream_t)stream;
  VXC(dv.stage.begin(s));
  const size_t MB = (size_t)c.max_batch;
  const float** hwav = dv.stage.host<const float*>();
  int* hns = dv.stage.host<int>(MB * sizeof(void*));
  int* hseg = dv.stage.host<int>(MB * sizeof(void*) + MB * sizeof(int));
  const int NT = n_tables(c);
  for (int t = 0; t < NT; ++t) hseg[(size_t)t * (MB + 1)] = 0;
  for (int i = 0; i < n; ++i) {
    hwav[i] = wav[i];
    hns[i] = n_samples[i];
    long T = 0;
    for (int t = 0; t < NT; ++t) {
      T = t < c.n_conv ? frames_of(c, n_samples[i], t) : tdnn_frames(c, frames_of(c, n_samples[i], c.n_conv - 1), t - c.n_conv);
      hseg[(size_t)t * (MB + 1) + i + 1] = hseg[(size_t)t * (MB + 1) + i] + (int)T;
    }
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
  VXC(run_call(x, dv.stage.dev<const float* const>(), dv.stage.dev<const int>(MB * sizeof(void*)), hseg, flags, emb_out, logits_out));
  const int rc = dv.stage.finish(s);
  g->last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return rc;
}

extern "C" int vx_spk_similarity(vx_spk* g, int32_t n, const float* a, const float* b, float* out, void* stream) {
  if (!g || !a || !b || !out) return fail(VX_ERR_ARG, "vx_spk_similarity: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_spk_similarity: n = %d pairs", n);
  spk_cosine<<<(unsigned)n, 64, 0, (hipStream_t)stream>>>(a, b, out, g->cfg.xvector);
  HIPC(hipGetLastError());
  return VX_OK;
}

extern "C" int vx_spk_read(vx_spk* g, const char* name, int32_t utt, float* dst, int64_t n_floats) {
  if (!g || !name || !dst) return fail(VX_ERR_ARG, "vx_spk_read: null argument");
  if (g->device < 0 || g->last_n == 0) return fail(VX_ERR_STATE, "vx_spk_read before any vx_spk_embed");
  const int n = g->last_n;
  if (utt < 0 || utt >= n) return fail(VX_ERR_ARG, "vx_spk_read: utterance %d of %d", utt, n);
  const vx_spk_config& c = g->cfg;
  const SpkPlan& p = g->plan;
  const int te = c.n_conv - 1;
  auto seg = [&](int t, int i) { return (long)g->last_seg[(size_t)t * (n + 1) + i]; };
  const std::string nm = name;
  const size_t rows_cap = (size_t)c.max_batch * g->Tmax;
  size_t base = 0;
  int table = te, width = c.hidden;
  auto layer_of = [&](const char* prefix, int hi, int& l) {
    const size_t k = strlen(prefix);
    if (nm.compare(0, k, prefix) != 0 || nm.size() == k) return false;
    char* end = nullptr;
    const long v = strtol(nm.c_str() + k, &end, 10);
    if (*end != 0 || v < 0 || v > hi) return false;
    l = (int)v;
    return true;
  };
  int l = 0;
  if (nm == "features") {
    base = p.conv[te & 1]; width = c.conv_dim[te];
  } else if (nm == "layer_sum") {
    base = c.use_weighted_layer_sum ? p.sum : p.hid + p.hid_stride * (size_t)((c.flags & VX_SPK_KEEP_TAPS) ? c.layers : (c.layers & 1));
  } else if (nm == "tdnn") {
    table = c.n_conv + c.n_tdnn - 1; width = c.tdnn_dim[c.n_tdnn - 1]; base = p.td[c.n_tdnn & 1];
  } else if (nm == "pooled") {
    table = -1; width = 2 * c.tdnn_dim[c.n_tdnn - 1]; base = p.pooled;
  } else if (layer_of("hidden", c.layers, l)) {
    if (!(c.flags & VX_SPK_KEEP_TAPS)) return fail(VX_ERR_STATE, "vx_spk_read: %s needs VX_SPK_KEEP_TAPS at create", name);
    base = p.hid + p.hid_stride * (size_t)l;
  } else if (layer_of("gate", c.layers - 1, l)) {
    if (c.attention != VX_SPK_WAVLM) return fail(VX_ERR_ARG, "vx_spk_read: %s: the plain mode has no gate", name);
    base = p.gate + (size_t)l * rows_cap * c.heads; width = c.heads;
  } else {
    return fail(VX_ERR_ARG, "vx_spk_read: unknown tap %s", name);
  }
  const long lo = table < 0 ? utt : seg(table, utt), rows = table < 0 ? 1 : seg(table, utt + 1) - lo;
  if (n_floats != (int64_t)rows * width)
    return fail(VX_ERR_ARG, "vx_spk_read: %s of utterance %d is %ld x %d floats, not %lld", name, utt, rows, width, (long long)n_floats);
  DevGuard guard(g->device);
  HIPC(guard.err);
  HIPC(hipStreamSynchronize(g->last_stream));
  HIPC(hipMemcpy(dst, g->dev->ws.get() + base + (size_t)lo * width, (size_t)rows * width * sizeof(float), hipMemcpyDeviceToHost));
  return VX_OK;
}

extern "C" int vx_spk_get_timings(const vx_spk* g, double* out, int32_t n) {
  if (!g || !out || n < 0 || n > 4) return fail(VX_ERR_ARG, "vx_spk_get_timings: null argument or n outside [0, 4]");
  const double v[4] = {g->last_ms, (double)(g->plan.total * sizeof(float) + g->plan.partial * sizeof(double)),
                       (double)(g->packed.size() * sizeof(float)),
                       g->last_n ? (double)g->last_seg[(size_t)(g->cfg.n_conv - 1) * (g->last_n + 1) + g->last_n] : 0.0};
  for (int i = 0; i < n; ++i) out[i] = v[i];
  return VX_OK;
}
