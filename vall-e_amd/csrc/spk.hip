// Speaker encoder (WavLM / Wav2Vec2 x-vector network) behind the C ABI (include/vallex.h, vx_spk_*).  The Wav2Vec2 backbone it shares
// with the recogniser (asr.hip) is w2v_host.hpp: the geometry and its checks, the key table, the packing, the workspace plan, the
// staging of a ragged call and the launches up to the positional convolution.  This unit keeps what is the speaker encoder's own:
// WavLM's gate and per-head bias table, the post-norm layer loop with the weighted layer sum, the TDNN and pooling head and
// vx_spk_similarity.  A translation unit and a handle of its own, like ganvoc.hip.
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
#include "w2v_host.hpp"

using namespace vx;

namespace {

struct SpkGate {  // WavLM: gru_rel_pos_linear's weight and bias, gru_rel_pos_const
  size_t w = 0, b = 0, c = 0;
};

}  // namespace

struct vx_spk : W2vHandle<W2vDev> {
  vx_spk_config cfg{};
  std::vector<int32_t> buckets;
  // offsets (floats) into the workspace, after the backbone's
  size_t p_gate = 0, p_sum = 0, p_td[2] = {0, 0}, p_pooled = 0;
  // filled by vx_spk_finalize
  size_t table = 0;
  SpkLin projector, tdnn[8], fe, cls;
  std::vector<SpkGate> gates;
  std::vector<float> lw;  // softmax(layer_weights)
};

namespace {

int n_tables(const vx_spk_config& c) { return c.n_conv + c.n_tdnn; }

long tdnn_frames(const vx_spk_config& c, long T, int upto) {
  for (int i = 0; i <= upto; ++i) T = std::max(0L, T - (long)c.tdnn_dilation[i] * (c.tdnn_kernel[i] - 1));
  return T;
}

void make_plan(vx_spk* g) {
  const vx_spk_config& c = g->cfg;
  W2vPlan& p = g->m.p;
  w2v_plan_rows(g->m, false);
  const size_t B = (size_t)c.max_batch, rows = B * (size_t)g->m.Tmax, d = (size_t)c.hidden;
  g->p_gate = p.take((size_t)c.layers * rows * c.heads);
  g->p_sum = p.take(rows * d);
  size_t widest = 0;
  for (int i = 0; i < c.n_tdnn; ++i) widest = std::max(widest, (size_t)c.tdnn_dim[i]);
  g->p_td[0] = p.take(rows * widest);
  g->p_td[1] = p.take(rows * widest);
  g->p_pooled = p.take(B * 2 * (size_t)c.tdnn_dim[c.n_tdnn - 1]);
  w2v_plan_stats(g->m);
}

int run_call(const vx_spk* g, const W2vRun& x, int flags, float* emb_out, float* logits_out) {
  const vx_spk_config& c = g->cfg;
  const W2vWeights& bw = g->m.bw;
  const W2vPlan& p = g->m.p;
  const int n = x.n, d = c.hidden, H = c.heads;
  float* ws = x.ws;
  // ---- feature encoder, projection, positional convolution
  EncRun e;
  VXC(w2v_run_features(x, (flags & VX_SPK_NORMALIZE) != 0, e));
  const long M = e.M;
  // ---- hidden state 0
  const bool wsum = c.use_weighted_layer_sum != 0;
  float* sum = wsum ? ws + g->p_sum : nullptr;
  VXC(run_ln(x, bw.enc_ln, ws + p.x0, ws + p.tmp, e.hidden(0), M, d, sum, wsum ? g->lw[0] : 0.f, 1));
  // ---- encoder layers (post-norm)
  const bool wavlm = c.attention == VX_SPK_WAVLM;
  for (int l = 0; l < c.layers; ++l) {
    const EncLayer& L = bw.layers[l];
    const float* h = e.hidden(l);
    float* gate = ws + g->p_gate + (size_t)l * (size_t)x.MB * g->m.Tmax * H;
    if (wavlm) {
      const SpkGate& G = g->gates[l];
      spk_gate<<<(unsigned)((M * H + 255) / 256), 256, 0, x.s>>>(h, x.W + G.w, x.W + G.b, x.W + G.c, gate, M, H, g->m.hd);
      HIPC(hipGetLastError());
    }
    VXC(run_attention(x, e, L, h, wavlm ? gate : nullptr, wavlm ? x.W + g->table : nullptr));
    VXC(run_ln(x, L.ln1, h, e.tmp, e.mid, M, d));
    VXC(run_lin(x, L.ff1, e.mid, d, e.ff, M, SPK_ACT_GELU));
    VXC(run_lin(x, L.ff2, e.ff, c.ffn, e.tmp, M, SPK_ACT_NONE));
    VXC(run_ln(x, L.ln2, e.mid, e.tmp, e.hidden(l + 1), M, d, sum, wsum ? g->lw[l + 1] : 0.f, 0));
  }
  // ---- head
  const int te = e.table;
  const float* top = wsum ? ws + g->p_sum : e.hidden(c.layers);
  VXC(run_lin(x, g->projector, top, d, ws + g->p_td[0], M, SPK_ACT_NONE));
  int cur = 0, cin = c.tdnn_dim[0];
  for (int i = 0; i < c.n_tdnn; ++i) {
    VXC(run_lin(x, g->tdnn[i], ws + g->p_td[cur], cin, ws + g->p_td[cur ^ 1], x.rows_of(c.n_conv + i), SPK_ACT_RELU, c.n_conv + i,
                i == 0 ? te : c.n_conv + i - 1));
    cur ^= 1;
    cin = c.tdnn_dim[i];
  }
  spk_pool<<<dim3((unsigned)((cin + 255) / 256), (unsigned)n), 256, 0, x.s>>>(ws + g->p_td[cur], ws + g->p_pooled, x.table(c.n_conv + c.n_tdnn - 1), cin);
  HIPC(hipGetLastError());
  VXC(run_lin(x, g->fe, ws + g->p_pooled, 2 * cin, emb_out, n, SPK_ACT_NONE));
  if (logits_out) VXC(run_lin(x, g->cls, emb_out, c.xvector, logits_out, n, SPK_ACT_NONE));
  return VX_OK;
}

}  // namespace

extern "C" int64_t vx_spk_frames(const vx_spk* g, int64_t n_samples) {
  return !g ? -1 : (int64_t)frames_of(g->m.q, (long)std::max<int64_t>(0, n_samples), g->cfg.n_conv - 1);
}

extern "C" int64_t vx_spk_min_samples(const vx_spk* g) { return !g ? -1 : (int64_t)g->m.min_samples; }

extern "C" int vx_spk_create(const vx_spk_config* cfg, vx_spk** out) {
  VXC(create_head("vx_spk_create", cfg, out));
  const vx_spk_config& c = *cfg;
  const char* what = "vx_spk_create";
  const W2vGeom q = w2v_geom(c, 1, (c.flags & VX_SPK_KEEP_TAPS) != 0);
  if (c.attention != VX_SPK_WAVLM && c.attention != VX_SPK_PLAIN) return fail(VX_ERR_ARG, "vx_spk_create: attention = %d", c.attention);
  VXC(w2v_validate(q, what, W2V_CHECK_SIZES));
  if (c.n_tdnn < 1 || c.n_tdnn > 8) return fail(VX_ERR_ARG, "vx_spk_create: n_tdnn = %d outside [1, 8]", c.n_tdnn);
  VXC(w2v_validate(q, what, W2V_CHECK_CONVS));
  for (int i = 0; i < c.n_tdnn; ++i)
    if (c.tdnn_dim[i] < 1 || c.tdnn_kernel[i] < 1 || c.tdnn_dilation[i] < 1)
      return fail(VX_ERR_ARG, "vx_spk_create: tdnn layer %d: dim %d, kernel %d, dilation %d", i, c.tdnn_dim[i], c.tdnn_kernel[i], c.tdnn_dilation[i]);
  if (c.pos_kernel < 1 || c.pos_groups < 1 || c.xvector < 1 || c.num_buckets < 0)
    return fail(VX_ERR_ARG, "vx_spk_create: pos_kernel %d, pos_groups %d, xvector %d, num_buckets %d", c.pos_kernel, c.pos_groups, c.xvector, c.num_buckets);
  if (c.attention == VX_SPK_WAVLM && c.num_buckets < 1) return fail(VX_ERR_ARG, "vx_spk_create: num_buckets = %d", c.num_buckets);
  VXC(w2v_validate(q, what, W2V_CHECK_RATIOS));
  if (c.flags & ~VX_SPK_KEEP_TAPS) return fail(VX_ERR_ARG, "vx_spk_create: flags = %d", c.flags);
  if (c.feat_extract_norm != 0) return fail(VX_ERR_UNSUPPORTED, "vx_spk_create: feat_extract_norm = \"layer\" (\"group\" is served)");
  if (c.do_stable_layer_norm != 0) return fail(VX_ERR_UNSUPPORTED, "vx_spk_create: do_stable_layer_norm (the post-norm encoder is served)");
  if (c.add_adapter != 0) return fail(VX_ERR_UNSUPPORTED, "vx_spk_create: add_adapter");
  if (c.activation != 0) return fail(VX_ERR_UNSUPPORTED, "vx_spk_create: activation = %d (gelu is served)", c.activation);
  VXC(w2v_validate(q, what, W2V_CHECK_SERVED));
  VXC(w2v_validate(q, what, W2V_CHECK_BATCH));

  std::unique_ptr<vx_spk> g(new vx_spk());
  g->cfg = c;
  g->m.q = q;
  long need = 2;  // two pooled frames
  for (int i = 0; i < c.n_tdnn; ++i) need += (long)c.tdnn_dilation[i] * (c.tdnn_kernel[i] - 1);
  VXC(w2v_size(g->m, what, need));
  make_plan(g.get());

  const int d = c.hidden, L = c.layers;
  w2v_add_keys(g.get(), q);
  if (c.attention == VX_SPK_WAVLM) {
    for (int l = 0; l < L; ++l) {
      lin_keys(g.get(), w2v_layer_prefix(l) + "attention.gru_rel_pos_linear", 8, g->m.hd);
      add_key(g.get(), w2v_layer_prefix(l) + "attention.gru_rel_pos_const", {1, c.heads, 1, 1});
    }
    add_key(g.get(), "encoder.layers.0.attention.rel_attn_embed.weight", {c.num_buckets, c.heads});
  }
  if (c.use_weighted_layer_sum) add_key(g.get(), "layer_weights", {L + 1});
  lin_keys(g.get(), "projector", c.tdnn_dim[0], d);
  int cin = c.tdnn_dim[0];
  for (int i = 0; i < c.n_tdnn; ++i) {
    lin_keys(g.get(), "tdnn." + std::to_string(i) + ".kernel", c.tdnn_dim[i], cin * c.tdnn_kernel[i]);
    cin = c.tdnn_dim[i];
  }
  lin_keys(g.get(), "feature_extractor", c.xvector, 2 * cin);
  lin_keys(g.get(), "classifier", c.xvector, c.xvector);
  *out = g.release();
  return VX_OK;
}

extern "C" void vx_spk_destroy(vx_spk* g) { destroy_handle(g); }

extern "C" int vx_spk_set_weight(vx_spk* g, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
  return set_weight(g, "vx_spk", key, data, shape, ndim);
}

extern "C" int vx_spk_set_buckets(vx_spk* g, const int32_t* idx, int32_t n) {
  if (!g || !idx) return fail(VX_ERR_ARG, "vx_spk_set_buckets: null argument");
  if (g->finalized) return fail(VX_ERR_STATE, "vx_spk_set_buckets after vx_spk_finalize");
  const int Tmax = g->m.Tmax;
  if (n != 2 * Tmax - 1) return fail(VX_ERR_ARG, "vx_spk_set_buckets: %d indices, expected 2 x %d - 1", n, Tmax);
  for (int i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= g->cfg.num_buckets)
      return fail(VX_ERR_ARG, "vx_spk_set_buckets: index %d at relative position %d outside [0, %d)", idx[i], i - (Tmax - 1),
                  g->cfg.num_buckets);
  g->buckets.assign(idx, idx + n);
  return VX_OK;
}

extern "C" int vx_spk_finalize(vx_spk* g) {
  if (!g) return fail(VX_ERR_ARG, "vx_spk_finalize: null handle");
  if (g->finalized) return VX_OK;
  const vx_spk_config& c = g->cfg;
  const bool wavlm = c.attention == VX_SPK_WAVLM;
  VXC(finalize_begin(g));
  if (wavlm && g->buckets.empty()) return fail(VX_ERR_STATE, "vx_spk_finalize: vx_spk_set_buckets has not been called");
  const int d = c.hidden, H = c.heads, L = c.layers;
  w2v_pack(g, g->m.q, g->m.bw);
  g->gates.assign(L, SpkGate());
  for (int l = 0; l < L; ++l) {
    w2v_pack_layer(g, g->m.q, g->m.bw, l);
    if (wavlm) {
      const std::string pre = w2v_layer_prefix(l);
      g->gates[l].w = push(g->packed, g->w[pre + "attention.gru_rel_pos_linear.weight"].data);
      g->gates[l].b = push(g->packed, g->w[pre + "attention.gru_rel_pos_linear.bias"].data);
      g->gates[l].c = push(g->packed, g->w[pre + "attention.gru_rel_pos_const"].data);
    }
  }
  if (wavlm) {  // bias[h][r + Tmax - 1] = rel_attn_embed[bucket(r)][h]
    const HostW& e = g->w["encoder.layers.0.attention.rel_attn_embed.weight"];
    const size_t R = 2 * (size_t)g->m.Tmax - 1;
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
  finalize_end(g);
  return VX_OK;
}

extern "C" int vx_spk_embed(vx_spk* g, int32_t n, const float* const* wav, const int32_t* n_samples, int32_t flags, float* emb_out,
                            float* logits_out, void* stream) {
  if (!g || !wav || !n_samples || !emb_out) return fail(VX_ERR_ARG, "vx_spk_embed: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_spk_embed: n = %d utterances", n);
  if (flags & ~VX_SPK_NORMALIZE) return fail(VX_ERR_ARG, "vx_spk_embed: flags = %d", flags);
  if (!g->finalized) return fail(VX_ERR_STATE, "vx_spk_embed before vx_spk_finalize");
  VXC(w2v_check_call(g, "vx_spk_embed", n, wav, n_samples, "two pooled frames"));
  const vx_spk_config& c = g->cfg;
  const auto t_begin = std::chrono::steady_clock::now();
  const int NT = n_tables(c);
  VXC(ensure_device(g, [NT](vx_spk* h) { return w2v_init_device(h, NT); }));
  ON_DEVICE(g->device);
  W2vRun x{};
  VXC(w2v_stage_begin(g, NT, n, wav, n_samples, (hipStream_t)stream, x));
  for (int i = 0; i < n; ++i) {
    const long Te = frames_of(g->m.q, n_samples[i], c.n_conv - 1);
    for (int t = c.n_conv; t < NT; ++t)
      x.hseg[(size_t)t * (x.MB + 1) + i + 1] = x.hseg[(size_t)t * (x.MB + 1) + i] + (int)tdnn_frames(c, Te, t - c.n_conv);
  }
  VXC(w2v_stage_commit(g, NT, x));
  VXC(run_call(g, x, flags, emb_out, logits_out));
  const int rc = g->dev->stage.finish(x.s);
  g->call.last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
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
  VXC(read_check(g, "vx_spk", "embed", name, utt, dst));
  const int n = g->call.last_n;
  const vx_spk_config& c = g->cfg;
  const W2vPlan& p = g->m.p;
  const int te = c.n_conv - 1;
  auto seg = [&](int t, int i) { return (long)g->call.last_seg[(size_t)t * (n + 1) + i]; };
  const std::string nm = name;
  const size_t rows_cap = (size_t)c.max_batch * g->m.Tmax;
  size_t base = 0;
  int table = te, width = c.hidden;
  int l = 0;
  if (nm == "features") {
    base = p.conv[te & 1]; width = c.conv_dim[te];
  } else if (nm == "layer_sum") {
    base = c.use_weighted_layer_sum ? g->p_sum : p.hid + p.hid_stride * (size_t)((c.flags & VX_SPK_KEEP_TAPS) ? c.layers : (c.layers & 1));
  } else if (nm == "tdnn") {
    table = c.n_conv + c.n_tdnn - 1; width = c.tdnn_dim[c.n_tdnn - 1]; base = g->p_td[c.n_tdnn & 1];
  } else if (nm == "pooled") {
    table = -1; width = 2 * c.tdnn_dim[c.n_tdnn - 1]; base = g->p_pooled;
  } else if (tap_index(nm, "hidden", c.layers, l)) {
    if (!(c.flags & VX_SPK_KEEP_TAPS)) return fail(VX_ERR_STATE, "vx_spk_read: %s needs VX_SPK_KEEP_TAPS at create", name);
    base = p.hid + p.hid_stride * (size_t)l;
  } else if (tap_index(nm, "gate", c.layers - 1, l)) {
    if (c.attention != VX_SPK_WAVLM) return fail(VX_ERR_ARG, "vx_spk_read: %s: the plain mode has no gate", name);
    base = g->p_gate + (size_t)l * rows_cap * c.heads; width = c.heads;
  } else {
    return fail(VX_ERR_ARG, "vx_spk_read: unknown tap %s", name);
  }
  const long lo = table < 0 ? utt : seg(table, utt), rows = table < 0 ? 1 : seg(table, utt + 1) - lo;
  return read_rows(g, "vx_spk", name, utt, base, lo, rows, width, dst, n_floats);
}

extern "C" int vx_spk_get_timings(const vx_spk* g, double* out, int32_t n) { return w2v_timings(g, "vx_spk", 0, out, n); }
