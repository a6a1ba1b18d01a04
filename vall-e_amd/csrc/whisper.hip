// Whisper recogniser (WhisperForConditionalGeneration, greedy) behind the C ABI (include/vallex.h, vx_wsp_*).  The encoder runs on the
// speaker encoder's row GEMM, plain attention and LayerNorm (spk_kernels.hpp through spk_host.hpp); its layer packing, its pre-norm layer
// loop (the recogniser's stable flavour) and the handle scaffolding are w2v_host.hpp's.  This unit keeps the log-mel front end, conv1
// and conv2, the decoder and the token loop (whisper_kernels.hpp).  A translation unit and a handle of its own, like asr.hip.
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
#include "whisper_kernels.hpp"

using namespace vx;

namespace {

constexpr int WSP_POLL = 8;  // decode steps enqueued between two reads of the finished flags

constexpr EncNames WSP_LAYER{"self_attn", "self_attn_layer_norm", "fc1", "fc2", "final_layer_norm"};

struct WspDecLayer {
  SpkLin qkv, out, cq, ckv, cout, ff1, ff2;
  SpkNorm ln1, ln2, ln3;
};

// Offsets (floats) into the workspace.
struct WspPlan {
  size_t mel = 0, c1 = 0, feat = 0, hid = 0, hid_stride = 0, mid = 0, nrm = 0, qkv = 0, att = 0, tmp = 0, ff = 0, enc = 0, ckv = 0, ckv_stride = 0,
         cache = 0, cache_stride = 0, x = 0, dn = 0, dqkv = 0, datt = 0, dq = 0, dff = 0, logits = 0, tmax = 0, tap = 0, total = 0;
};

struct WspDev : SpeechDev {
  DevBuf<unsigned char> suppress;
  DevBuf<int> state;  // cur | pos | count | finished, [max_batch] each
  int* fin_host = nullptr;  // pinned [max_batch]
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~WspDev() {
    if (fin_host) (void)hipHostFree(fin_host);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace

struct vx_wsp : SpeechHandle<WspDev> {
  vx_wsp_config cfg{};
  int P = 0, F = 0, Tt = 0, tiles = 0;
  long chunk = 0;
  WspPlan plan;
  std::vector<unsigned char> suppress;  // [vocab]
  size_t window = 0, dft = 0, dft_sin = 0, mel = 0, enc_pos = 0, tok_emb = 0, dec_pos = 0;
  SpkLin conv1, conv2, head;
  SpkNorm enc_ln, dec_ln;
  std::vector<EncLayer> enc;
  std::vector<WspDecLayer> dec;
  // the last call, for vx_wsp_read
  std::vector<int> last_prompt;  // per utterance
  double last_steps = 0.0;
};

namespace {

void make_plan(vx_wsp* g) {
  const vx_wsp_config& c = g->cfg;
  WspPlan& p = g->plan;
  const size_t B = (size_t)c.max_batch, P = (size_t)g->P, F = (size_t)g->F, d = (size_t)c.d_model, Tt = (size_t)g->Tt;
  size_t at = 0;
  auto take = [&](size_t n) { const size_t o = at; at += (n + 3) / 4 * 4; return o; };
  const bool keep = (c.flags & VX_WSP_KEEP_TAPS) != 0;
  const size_t per = g->bf16 ? 2 : 1;  // the bf16 encoder mode's rows: two elements a float
  p.mel = take(B * F * (size_t)c.n_mels);
  p.c1 = take(B * F * d);
  p.feat = take(B * P * d);
  p.hid_stride = (B * P * d + 3) / 4 * 4;
  p.hid = take(p.hid_stride * (keep ? (size_t)c.enc_layers + 1 : 2));
  p.mid = take(B * P * d);
  p.nrm = take(B * P * d / per);
  p.qkv = take(B * P * 3 * d / per);
  p.att = take(B * P * d / per);
  p.tmp = take(B * P * d);
  p.ff = take(B * P * (size_t)c.enc_ffn / per);
  p.enc = take(B * P * d);
  p.ckv_stride = (B * P * 2 * d + 3) / 4 * 4;
  p.ckv = take(p.ckv_stride * (size_t)c.dec_layers);
  p.cache_stride = (B * Tt * 2 * d + 3) / 4 * 4;
  p.cache = take(p.cache_stride * (size_t)c.dec_layers);
  p.x = take(B * d);
  p.dn = take(B * d);
  p.dqkv = take(B * 3 * d);
  p.datt = take(B * d);
  p.dq = take(B * d);
  p.dff = take(B * (size_t)c.dec_ffn);
  p.logits = take(B * (size_t)c.vocab);
  p.tmax = take(B * (size_t)g->tiles);
  p.tap = take(keep ? Tt * B * (size_t)c.vocab : 4);
  p.total = at;
}

size_t stage_bytes(const vx_wsp* g) {
  const size_t MB = (size_t)g->cfg.max_batch, Tt = (size_t)g->Tt;
  return MB * sizeof(void*) + (MB + 2 * (MB + 1) + MB * Tt + MB + MB + MB * Tt) * sizeof(int);
}

int wsp_init_device(vx_wsp* g) {
  VXC(init_device(g, g->plan.total, stage_bytes(g)));
  WspDev& d = *g->dev;
  const size_t MB = (size_t)g->cfg.max_batch;
  VXC(d.suppress.alloc(g->suppress.size() + 4));
  HIPC(hipMemcpy(d.suppress.get(), g->suppress.data(), g->suppress.size(), hipMemcpyHostToDevice));
  VXC(d.state.alloc(4 * MB));
  HIPC(hipHostMalloc((void**)&d.fin_host, MB * sizeof(int)));
  for (hipEvent_t& e : d.ev) HIPC(hipEventCreate(&e));
  return VX_OK;
}

struct CallCtx : SpkCall {
  const vx_wsp* g;
  float* ws;
};

// The token loop's GEMM on a filled argument struct: the columns per workgroup (N / 512 rounded down to a multiple of 8, at least 8,
// which holds up to N = 8191, and at most 64: the vocabulary head runs eight column passes over one staged chunk), the K chunk, the
// grid and the LDS size are chosen here and nowhere else, for the recogniser and for vx_op_wsp_gemm alike.
int launch_skinny(WspSkinnyArgs a, hipStream_t s) {
  a.cpw = std::min(64, std::max(8, a.N / 512 / 8 * 8));
  const int kc = std::min(a.K, WSP_SK_KC);
  const dim3 grid((unsigned)((a.N + a.cpw - 1) / a.cpw), (unsigned)((a.M + WSP_SK_MT - 1) / WSP_SK_MT));
  wsp_skinny_gemm<<<grid, 256, (size_t)WSP_SK_MT * kc * sizeof(float), s>>>(a);
  HIPC(hipGetLastError());
  return VX_OK;
}

// wsp_decode_attn over n utterances and H heads: the scores of up to max_keys keys and the 4 x 64 partial outputs sit in LDS.
int launch_decode_attn(const WspAttnArgs& a, int H, int n, int max_keys, hipStream_t s) {
  wsp_decode_attn<<<dim3((unsigned)H, (unsigned)n), 256, (size_t)(max_keys + 256) * sizeof(float), s>>>(a);
  HIPC(hipGetLastError());
  return VX_OK;
}

int run_skinny(const CallCtx& x, const SpkLin& l, const float* in, float* out, const float* res, int act) {
  WspSkinnyArgs a{};
  a.x = in; a.W = x.W + l.w; a.bias = l.has_bias ? x.W + l.b : nullptr; a.res = res; a.out = out;
  a.M = x.n; a.N = l.N; a.K = l.C; a.ldo = l.N; a.act = act;
  return launch_skinny(a, x.s);
}

int run_front_and_encoder(const CallCtx& x, const float* const* wav, const int* n_samples_dev, const int* hseg1, hipEvent_t after_mel) {
  const vx_wsp* g = x.g;
  const vx_wsp_config& c = g->cfg;
  const WspPlan& p = g->plan;
  const int n = x.n, d = c.d_model, P = g->P, F = g->F;
  float* ws = x.ws;
  WspMelArgs m{};
  m.wav = wav; m.n_samples = n_samples_dev; m.window = x.W + g->window; m.dft_cos = x.W + g->dft; m.dft_sin = x.W + g->dft_sin; m.mel = x.W + g->mel;
  m.out = ws + p.mel; m.tile_max = ws + p.tmax; m.frames = F; m.chunk = (int)g->chunk; m.n_mels = c.n_mels; m.tiles = g->tiles;
  wsp_logmel<<<dim3((unsigned)g->tiles, (unsigned)n), 256, 0, x.s>>>(m);
  HIPC(hipGetLastError());
  const long per = (long)F * c.n_mels;
  wsp_logmel_finish<<<dim3((unsigned)((per + 255) / 256), (unsigned)n), 256, 0, x.s>>>(ws + p.mel, ws + p.tmax, g->tiles, per);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(after_mel, x.s));
  // table 0: 2 P rows an utterance, table 1: P rows
  VXC(run_lin(x, g->conv1, ws + p.mel, c.n_mels, ws + p.c1, (long)n * F, SPK_ACT_GELU, 0, 0));
  VXC(run_lin(x, g->conv2, ws + p.c1, d, ws + p.feat, (long)n * P, SPK_ACT_GELU, 1, 0));
  const long M = (long)n * P;
  EncRun e = enc_run(ws, p, (c.flags & VX_WSP_KEEP_TAPS) != 0);
  e.M = M; e.d = d; e.H = c.enc_heads; e.hd = 64; e.ffn = c.enc_ffn; e.Tmax = P; e.table = 1; e.hseg = hseg1;
  if (g->bf16) {
    e.W16 = reinterpret_cast<const ebf_t*>(g->dev->w16.get());
    VXC(run_add_ln16(x, g->enc[0].ln1, ws + p.feat, x.W + g->enc_pos, P, e.hidden(0), e.nrm16, M, d));
    VXC(run_prenorm_layers_bf16(x, e, g->enc, g->enc_ln, e.hidden(c.enc_layers), ws + p.enc));
  } else {
    wsp_add_layernorm<<<(unsigned)((M + 3) / 4), 256, 0, x.s>>>(ws + p.feat, x.W + g->enc_pos, P, x.W + g->enc[0].ln1.w, x.W + g->enc[0].ln1.b,
                                                                 e.hidden(0), e.nrm, M, d, x.eps);
    HIPC(hipGetLastError());
    VXC(run_prenorm_layers(x, e, g->enc, g->enc_ln, e.hidden(c.enc_layers), ws + p.enc));
  }
  // every decoder layer's cross-attention keys and values, for the whole call
  for (int l = 0; l < c.dec_layers; ++l) VXC(run_lin(x, g->dec[l].ckv, ws + p.enc, d, ws + p.ckv + p.ckv_stride * (size_t)l, M, SPK_ACT_NONE));
  return VX_OK;
}

// One decode step of every utterance of the call: the same launches at every step, the state is on the device.
int run_step(const CallCtx& x, const WspState& st, const WspHeadArgs& head) {
  const vx_wsp* g = x.g;
  const vx_wsp_config& c = g->cfg;
  const WspPlan& p = g->plan;
  const int n = x.n, d = c.d_model, H = c.dec_heads;
  float* ws = x.ws;
  const float scale = 0.125f;  // 64^-1/2
  wsp_embed<<<n, 256, 0, x.s>>>(x.W + g->tok_emb, x.W + g->dec_pos, st.cur, st.pos, ws + p.x, d);
  HIPC(hipGetLastError());
  for (int l = 0; l < c.dec_layers; ++l) {
    const WspDecLayer& ly = g->dec[l];
    VXC(run_ln(x, ly.ln1, ws + p.x, nullptr, ws + p.dn, n, d));
    VXC(run_skinny(x, ly.qkv, ws + p.dn, ws + p.dqkv, nullptr, SPK_ACT_NONE));
    WspAttnArgs a{};
    float* cache = ws + p.cache + p.cache_stride * (size_t)l;
    a.q = ws + p.dqkv; a.knew = ws + p.dqkv + d; a.vnew = ws + p.dqkv + 2 * d; a.kc = cache; a.vc = cache + d; a.out = ws + p.datt;
    a.pos = st.pos; a.ldq = 3 * d; a.ld = 2 * d; a.d = d; a.keys = 0; a.rows_per_utt = g->Tt; a.scale = scale;
    VXC(launch_decode_attn(a, H, n, g->Tt, x.s));
    VXC(run_skinny(x, ly.out, ws + p.datt, ws + p.x, ws + p.x, SPK_ACT_NONE));
    VXC(run_ln(x, ly.ln2, ws + p.x, nullptr, ws + p.dn, n, d));
    VXC(run_skinny(x, ly.cq, ws + p.dn, ws + p.dq, nullptr, SPK_ACT_NONE));
    WspAttnArgs b{};
    float* ckv = ws + p.ckv + p.ckv_stride * (size_t)l;
    b.q = ws + p.dq; b.knew = nullptr; b.vnew = nullptr; b.kc = ckv; b.vc = ckv + d; b.out = ws + p.datt;
    b.pos = nullptr; b.ldq = d; b.ld = 2 * d; b.d = d; b.keys = g->P; b.rows_per_utt = g->P; b.scale = scale;
    VXC(launch_decode_attn(b, H, n, g->P, x.s));
    VXC(run_skinny(x, ly.cout, ws + p.datt, ws + p.x, ws + p.x, SPK_ACT_NONE));
    VXC(run_ln(x, ly.ln3, ws + p.x, nullptr, ws + p.dn, n, d));
    VXC(run_skinny(x, ly.ff1, ws + p.dn, ws + p.dff, nullptr, SPK_ACT_GELU));
    VXC(run_skinny(x, ly.ff2, ws + p.dff, ws + p.x, ws + p.x, SPK_ACT_NONE));
  }
  VXC(run_ln(x, g->dec_ln, ws + p.x, nullptr, ws + p.dn, n, d));
  VXC(run_skinny(x, g->head, ws + p.dn, ws + p.logits, nullptr, SPK_ACT_NONE));
  wsp_head_reduce<<<n, 256, 0, x.s>>>(head);
  HIPC(hipGetLastError());
  return VX_OK;
}

}  // namespace

extern "C" int vx_wsp_create(const vx_wsp_config* cfg, vx_wsp** out) {
  VXC(create_head("vx_wsp_create", cfg, out));
  const vx_wsp_config& c = *cfg;
  if (c.n_mels < 1 || c.d_model < 1 || c.vocab < 1)
    return fail(VX_ERR_ARG, "vx_wsp_create: num_mel_bins %d, d_model %d, vocab_size %d", c.n_mels, c.d_model, c.vocab);
  if (c.enc_layers < 1 || c.dec_layers < 1 || c.enc_layers > 256 || c.dec_layers > 256 || c.enc_heads < 1 || c.dec_heads < 1 || c.enc_ffn < 1 ||
      c.dec_ffn < 1)
    return fail(VX_ERR_ARG, "vx_wsp_create: encoder layers %d, heads %d, ffn %d; decoder layers %d, heads %d, ffn %d", c.enc_layers, c.enc_heads,
                c.enc_ffn, c.dec_layers, c.dec_heads, c.dec_ffn);
  if (c.max_source_positions < 1 || c.max_target_positions < 2)
    return fail(VX_ERR_ARG, "vx_wsp_create: max_source_positions %d, max_target_positions %d", c.max_source_positions, c.max_target_positions);
  if (c.eos_token_id < 0 || c.eos_token_id >= c.vocab) return fail(VX_ERR_ARG, "vx_wsp_create: eos_token_id %d outside [0, %d)", c.eos_token_id, c.vocab);
  if (c.max_batch < 1) return fail(VX_ERR_ARG, "vx_wsp_create: max_batch = %d", c.max_batch);
  if (c.flags & ~(VX_WSP_KEEP_TAPS | VX_WSP_ENC_BF16)) return fail(VX_ERR_ARG, "vx_wsp_create: flags = %d", c.flags);
  if (c.activation != 0) return fail(VX_ERR_UNSUPPORTED, "vx_wsp_create: activation_function = %d (gelu is served)", c.activation);
  if (c.d_model % c.enc_heads != 0 || c.d_model / c.enc_heads != 64)
    return fail(VX_ERR_UNSUPPORTED, "vx_wsp_create: encoder head_dim = %d / %d (64 is served)", c.d_model, c.enc_heads);
  if (c.d_model % c.dec_heads != 0 || c.d_model / c.dec_heads != 64)
    return fail(VX_ERR_UNSUPPORTED, "vx_wsp_create: decoder head_dim = %d / %d (64 is served)", c.d_model, c.dec_heads);
  if (c.n_mels % 16 != 0) return fail(VX_ERR_UNSUPPORTED, "vx_wsp_create: num_mel_bins = %d (multiples of 16 are served)", c.n_mels);
  if (c.enc_ffn % 16 != 0 || c.dec_ffn % 16 != 0)
    return fail(VX_ERR_UNSUPPORTED, "vx_wsp_create: ffn dims %d and %d (multiples of 16 are served)", c.enc_ffn, c.dec_ffn);
  if (c.max_source_positions > WSP_MAX_KEYS || c.max_target_positions > WSP_MAX_KEYS)
    return fail(VX_ERR_UNSUPPORTED, "vx_wsp_create: max_source_positions %d, max_target_positions %d (up to %d keys are served)",
                c.max_source_positions, c.max_target_positions, WSP_MAX_KEYS);
  if (c.max_batch > SPK_MAX_SEG) return fail(VX_ERR_UNSUPPORTED, "vx_wsp_create: max_batch = %d > %d", c.max_batch, SPK_MAX_SEG);
  if (c.flags & VX_WSP_ENC_BF16) VXC(enc_bf16_check("vx_wsp_create", c.d_model, c.enc_heads, c.enc_ffn, "encoder_attention_heads", "encoder_ffn_dim"));

  std::unique_ptr<vx_wsp> g(new vx_wsp());
  g->cfg = c;
  g->bf16 = (c.flags & VX_WSP_ENC_BF16) != 0;
  g->P = c.max_source_positions;
  g->F = 2 * g->P;
  g->Tt = c.max_target_positions;
  g->chunk = 320L * g->P;
  g->tiles = (g->F + WSP_TF - 1) / WSP_TF;
  g->suppress.assign((size_t)c.vocab, 0);
  make_plan(g.get());

  const int d = c.d_model;
  add_key(g.get(), "mel_filters", {c.n_mels, WSP_BINS});
  add_key(g.get(), "model.encoder.conv1.weight", {d, c.n_mels, 3});
  add_key(g.get(), "model.encoder.conv1.bias", {d});
  add_key(g.get(), "model.encoder.conv2.weight", {d, d, 3});
  add_key(g.get(), "model.encoder.conv2.bias", {d});
  add_key(g.get(), "model.encoder.embed_positions.weight", {g->P, d});
  for (int l = 0; l < c.enc_layers; ++l) {
    enc_layer_keys(g.get(), "model.encoder.layers." + std::to_string(l) + ".", WSP_LAYER, d, c.enc_ffn, false);
  }
  norm_keys(g.get(), "model.encoder.layer_norm", d);
  add_key(g.get(), "model.decoder.embed_tokens.weight", {c.vocab, d});
  add_key(g.get(), "model.decoder.embed_positions.weight", {g->Tt, d});
  for (int l = 0; l < c.dec_layers; ++l) {
    const std::string pre = "model.decoder.layers." + std::to_string(l) + ".";
    attn_keys(g.get(), pre + "self_attn", d, false);
    norm_keys(g.get(), pre + "self_attn_layer_norm", d);
    attn_keys(g.get(), pre + "encoder_attn", d, false);
    norm_keys(g.get(), pre + "encoder_attn_layer_norm", d);
    lin_keys(g.get(), pre + "fc1", c.dec_ffn, d);
    lin_keys(g.get(), pre + "fc2", d, c.dec_ffn);
    norm_keys(g.get(), pre + "final_layer_norm", d);
  }
  norm_keys(g.get(), "model.decoder.layer_norm", d);
  if (!c.tie_proj) add_key(g.get(), "proj_out.weight", {c.vocab, d});
  *out = g.release();
  return VX_OK;
}

extern "C" void vx_wsp_destroy(vx_wsp* g) { destroy_handle(g); }

extern "C" int vx_wsp_set_weight(vx_wsp* g, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
  return set_weight(g, "vx_wsp", key, data, shape, ndim);
}

extern "C" int vx_wsp_set_suppress(vx_wsp* g, const int32_t* ids, int32_t n_ids, const int32_t* begin_ids, int32_t n_begin) {
  if (!g || (n_ids > 0 && !ids) || (n_begin > 0 && !begin_ids) || n_ids < 0 || n_begin < 0) return fail(VX_ERR_ARG, "vx_wsp_set_suppress: bad argument");
  if (g->finalized) return fail(VX_ERR_STATE, "vx_wsp_set_suppress after vx_wsp_finalize");
  for (int i = 0; i < n_ids; ++i)
    if (ids[i] < 0 || ids[i] >= g->cfg.vocab) return fail(VX_ERR_ARG, "vx_wsp_set_suppress: suppress_tokens[%d] = %d outside [0, %d)", i, ids[i], g->cfg.vocab);
  for (int i = 0; i < n_begin; ++i)
    if (begin_ids[i] < 0 || begin_ids[i] >= g->cfg.vocab)
      return fail(VX_ERR_ARG, "vx_wsp_set_suppress: begin_suppress_tokens[%d] = %d outside [0, %d)", i, begin_ids[i], g->cfg.vocab);
  std::fill(g->suppress.begin(), g->suppress.end(), 0);
  for (int i = 0; i < n_ids; ++i) g->suppress[ids[i]] |= WSP_SUPPRESS;
  for (int i = 0; i < n_begin; ++i) g->suppress[begin_ids[i]] |= WSP_BEGIN_SUPPRESS;
  return VX_OK;
}

extern "C" int vx_wsp_finalize(vx_wsp* g) {
  if (!g) return fail(VX_ERR_ARG, "vx_wsp_finalize: null handle");
  if (g->finalized) return VX_OK;
  VXC(finalize_begin(g));
  const vx_wsp_config& c = g->cfg;
  const int d = c.d_model;
  {  // the periodic Hann window and the cos / sin table, from fp64 with the argument reduced exactly
    std::vector<float> win(WSP_NFFT), tc((size_t)WSP_DFT_ROWS * WSP_FR_K, 0.f), ts((size_t)WSP_DFT_ROWS * WSP_FR_K, 0.f);
    const double w0 = 2.0 * M_PI / WSP_NFFT;
    for (int n = 0; n < WSP_NFFT; ++n) win[n] = (float)(0.5 - 0.5 * cos(w0 * n));
    for (int j = 0; j < WSP_BINS; ++j)
      for (int k = 0; k < WSP_FR_K; ++k) {  // column k holds term n of the folded frame (whisper_kernels.hpp)
        const int n = k < WSP_FR_K / 2 ? (k < 101 ? k : -1) : (k - 3 <= 200 ? k - 3 : -1);
        if (n < 0) continue;
        const double ph = w0 * (double)((j * n) % WSP_NFFT);
        tc[(size_t)j * WSP_FR_K + k] = (float)cos(ph);
        ts[(size_t)j * WSP_FR_K + k] = (float)sin(ph);
      }
    g->window = push(g->packed, win);
    g->dft = push(g->packed, tc);
    g->dft_sin = push(g->packed, ts);
    const std::vector<float>& mf = g->w["mel_filters"].data;
    const int rows = (c.n_mels + 31) / 32 * 32;
    std::vector<float> mel((size_t)rows * WSP_MEL_K, 0.f);
    for (int m = 0; m < c.n_mels; ++m)
      for (int k = 0; k < WSP_BINS; ++k) mel[(size_t)m * WSP_MEL_K + k] = mf[(size_t)m * WSP_BINS + k];
    g->mel = push(g->packed, mel);
  }
  g->conv1 = pack_conv(g, "model.encoder.conv1", d, c.n_mels, 3, 1, true);
  g->conv1.off0 = -1;
  g->conv2 = pack_conv(g, "model.encoder.conv2", d, d, 3, 1, true);
  g->conv2.off0 = -1;
  g->conv2.stride = 2;
  g->enc_pos = push(g->packed, g->w["model.encoder.embed_positions.weight"].data);
  g->enc.clear();  // q | k | v stacked, k without a bias
  for (int l = 0; l < c.enc_layers; ++l)
    g->enc.push_back(pack_enc_layer(g, "model.encoder.layers." + std::to_string(l) + ".", WSP_LAYER, d, c.enc_ffn, false));
  g->enc_ln = pack_norm(g, "model.encoder.layer_norm");
  g->tok_emb = push(g->packed, g->w["model.decoder.embed_tokens.weight"].data);
  g->dec_pos = push(g->packed, g->w["model.decoder.embed_positions.weight"].data);
  g->dec.assign(c.dec_layers, WspDecLayer());
  for (int l = 0; l < c.dec_layers; ++l) {
    const std::string pre = "model.decoder.layers." + std::to_string(l) + ".";
    WspDecLayer& ly = g->dec[l];
    ly.qkv = pack_qkv(g, pre + "self_attn", d, false);
    ly.out = pack_linear(g, pre + "self_attn.out_proj", d, d);
    ly.ln1 = pack_norm(g, pre + "self_attn_layer_norm");
    ly.cq = pack_linear(g, pre + "encoder_attn.q_proj", d, d);
    {
      std::vector<float> wk = g->w[pre + "encoder_attn.k_proj.weight"].data, bk((size_t)d, 0.f);
      const HostW& wv = g->w[pre + "encoder_attn.v_proj.weight"];
      const HostW& bv = g->w[pre + "encoder_attn.v_proj.bias"];
      wk.insert(wk.end(), wv.data.begin(), wv.data.end());
      bk.insert(bk.end(), bv.data.begin(), bv.data.end());
      ly.ckv.w = push(g->packed, wk);
      ly.ckv.b = push(g->packed, bk);
      ly.ckv.has_bias = true; ly.ckv.C = d; ly.ckv.N = 2 * d;
    }
    ly.cout = pack_linear(g, pre + "encoder_attn.out_proj", d, d);
    ly.ln2 = pack_norm(g, pre + "encoder_attn_layer_norm");
    ly.ff1 = pack_linear(g, pre + "fc1", c.dec_ffn, d);
    ly.ff2 = pack_linear(g, pre + "fc2", d, c.dec_ffn);
    ly.ln3 = pack_norm(g, pre + "final_layer_norm");
  }
  g->dec_ln = pack_norm(g, "model.decoder.layer_norm");
  g->head = SpkLin();
  g->head.w = c.tie_proj ? g->tok_emb : push(g->packed, g->w["proj_out.weight"].data);
  g->head.has_bias = false; g->head.C = d; g->head.N = c.vocab;
  finalize_end(g);
  return VX_OK;
}

extern "C" int vx_wsp_recognize(vx_wsp* g, int32_t n, const float* const* wav, const int32_t* n_samples, const int32_t* prompt_ids,
                                const int32_t* n_prompt, int32_t prompt_stride, const int32_t* max_new_tokens, const int32_t* forced,
                                int32_t out_stride, int32_t* tokens_out, float* logprobs_out, int32_t* counts_out, int32_t* stops_out,
                                void* stream) {
  if (!g || !wav || !n_samples || !prompt_ids || !n_prompt || !max_new_tokens || !tokens_out || !logprobs_out || !counts_out || !stops_out)
    return fail(VX_ERR_ARG, "vx_wsp_recognize: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_wsp_recognize: n = %d utterances", n);
  if (!g->finalized) return fail(VX_ERR_STATE, "vx_wsp_recognize before vx_wsp_finalize");
  const vx_wsp_config& c = g->cfg;
  const int Tt = g->Tt;
  if (n > c.max_batch) return fail(VX_ERR_CAPACITY, "vx_wsp_recognize: n = %d utterances > max_batch %d", n, c.max_batch);
  if (prompt_stride < 1 || out_stride < 1 || out_stride > Tt)
    return fail(VX_ERR_ARG, "vx_wsp_recognize: prompt_stride %d, out_stride %d (1 .. max_target_positions = %d)", prompt_stride, out_stride, Tt);
  int steps = 0;
  for (int i = 0; i < n; ++i) {
    if (!wav[i]) return fail(VX_ERR_ARG, "vx_wsp_recognize: utterance %d: null pointer", i);
    if (n_samples[i] < 0) return fail(VX_ERR_ARG, "vx_wsp_recognize: utterance %d: n_samples = %d", i, n_samples[i]);
    if (n_samples[i] > g->chunk)
      return fail(VX_ERR_CAPACITY, "vx_wsp_recognize: utterance %d: n_samples = %d > the chunk of %ld samples (long-form transcription is not built)",
                  i, n_samples[i], g->chunk);
    if (n_prompt[i] < 1) return fail(VX_ERR_ARG, "vx_wsp_recognize: utterance %d: empty prompt_ids", i);
    if (n_prompt[i] > prompt_stride) return fail(VX_ERR_ARG, "vx_wsp_recognize: utterance %d: n_prompt %d > prompt_stride %d", i, n_prompt[i], prompt_stride);
    if (n_prompt[i] >= Tt)
      return fail(VX_ERR_CAPACITY, "vx_wsp_recognize: utterance %d: prompt_ids of %d tokens leave no room under max_target_positions = %d", i,
                  n_prompt[i], Tt);
    for (int k = 0; k < n_prompt[i]; ++k) {
      const int id = prompt_ids[(size_t)i * prompt_stride + k];
      if (id < 0 || id >= c.vocab) return fail(VX_ERR_ARG, "vx_wsp_recognize: utterance %d: prompt_ids[%d] = %d outside [0, %d)", i, k, id, c.vocab);
    }
    if (max_new_tokens[i] < 1 || max_new_tokens[i] > out_stride)
      return fail(VX_ERR_ARG, "vx_wsp_recognize: utterance %d: max_new_tokens = %d outside [1, out_stride = %d]", i, max_new_tokens[i], out_stride);
    const int room = Tt - n_prompt[i];
    if (forced) {
      if (max_new_tokens[i] > room)
        return fail(VX_ERR_CAPACITY, "vx_wsp_recognize: utterance %d: %d forced tokens after a prompt of %d exceed max_target_positions = %d", i,
                    max_new_tokens[i], n_prompt[i], Tt);
      for (int k = 0; k < max_new_tokens[i]; ++k) {
        const int id = forced[(size_t)i * out_stride + k];
        if (id < 0 || id >= c.vocab) return fail(VX_ERR_ARG, "vx_wsp_recognize: utterance %d: forced token %d is id %d outside [0, %d)", i, k, id, c.vocab);
      }
    }
    steps = std::max(steps, n_prompt[i] - 1 + std::min(max_new_tokens[i], room));
  }
  const auto t_begin = std::chrono::steady_clock::now();
  VXC(ensure_device(g, wsp_init_device));
  ON_DEVICE(g->device);
  WspDev& dv = *g->dev;
  hipStream_t s = (hipStream_t)stream;
  VXC(dv.stage.begin(s));
  const size_t MB = (size_t)c.max_batch;
  // wav | n_samples | table 0 | table 1 | prompt [MB][Tt] | n_prompt | max_new | forced [MB][Tt]
  size_t off = 0;
  const size_t o_wav = off; off += MB * sizeof(void*);
  const size_t o_ns = off; off += MB * sizeof(int);
  const size_t o_seg = off; off += 2 * (MB + 1) * sizeof(int);
  const size_t o_prompt = off; off += MB * Tt * sizeof(int);
  const size_t o_np = off; off += MB * sizeof(int);
  const size_t o_mn = off; off += MB * sizeof(int);
  const size_t o_forced = off;
  const float** hwav = dv.stage.host<const float*>(o_wav);
  int* hns = dv.stage.host<int>(o_ns);
  int* hseg = dv.stage.host<int>(o_seg);
  int* hprompt = dv.stage.host<int>(o_prompt);
  int* hnp = dv.stage.host<int>(o_np);
  int* hmn = dv.stage.host<int>(o_mn);
  int* hforced = dv.stage.host<int>(o_forced);
  g->last_prompt.assign((size_t)n, 0);
  hseg[0] = 0;
  hseg[MB + 1] = 0;
  for (int i = 0; i < n; ++i) {
    hwav[i] = wav[i];
    hns[i] = n_samples[i];
    hseg[i + 1] = hseg[i] + g->F;
    hseg[MB + 1 + i + 1] = hseg[MB + 1 + i] + g->P;
    for (int k = 0; k < Tt; ++k) hprompt[(size_t)i * Tt + k] = k < n_prompt[i] ? prompt_ids[(size_t)i * prompt_stride + k] : 0;
    hnp[i] = n_prompt[i];
    hmn[i] = max_new_tokens[i];
    for (int k = 0; k < out_stride; ++k) hforced[(size_t)i * out_stride + k] = (forced && k < max_new_tokens[i]) ? forced[(size_t)i * out_stride + k] : 0;
    g->last_prompt[i] = n_prompt[i];
  }
  g->call.last_n = n;
  g->call.last_stream = s;
  VXC(dv.stage.upload(dv.stage.bytes, s));
  CallCtx x{};
  x.g = g; x.eps = 1e-5f; x.W = dv.w.get(); x.ws = dv.ws.get(); x.MB = (int)MB; x.n = n; x.s = s;
  x.seg = dv.stage.dev<const int>(o_seg);
  HIPC(hipEventRecord(dv.ev[0], s));
  VXC(run_front_and_encoder(x, dv.stage.dev<const float* const>(o_wav), dv.stage.dev<const int>(o_ns), hseg + MB + 1, dv.ev[1]));
  HIPC(hipEventRecord(dv.ev[2], s));
  WspState st{dv.state.get(), dv.state.get() + MB, dv.state.get() + 2 * MB, dv.state.get() + 3 * MB};
  wsp_init_state<<<1, 64, 0, s>>>(st, dv.stage.dev<const int>(o_prompt), Tt, counts_out, stops_out, n);
  HIPC(hipGetLastError());
  WspHeadArgs head{};
  head.logits = dv.ws.get() + g->plan.logits; head.suppress = dv.suppress.get(); head.prompt = dv.stage.dev<const int>(o_prompt);
  head.n_prompt = dv.stage.dev<const int>(o_np); head.max_new = dv.stage.dev<const int>(o_mn);
  head.forced = forced ? dv.stage.dev<const int>(o_forced) : nullptr; head.st = st;
  head.tokens_out = tokens_out; head.logprob_out = logprobs_out; head.count_out = counts_out; head.stop_out = stops_out;
  head.tap = (c.flags & VX_WSP_KEEP_TAPS) ? dv.ws.get() + g->plan.tap : nullptr;
  head.V = c.vocab; head.prompt_stride = Tt; head.out_stride = out_stride; head.eos = c.eos_token_id; head.max_target = Tt; head.MB = (int)MB;
  // the token loop: WSP_POLL steps are enqueued, then the finished flags are read once
  int done_steps = 0;
  while (done_steps < steps) {
    const int upto = std::min(steps, done_steps + WSP_POLL);
    for (; done_steps < upto; ++done_steps) VXC(run_step(x, st, head));
    if (done_steps >= steps) break;
    HIPC(hipMemcpyAsync(dv.fin_host, st.finished, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    bool all = true;
    for (int i = 0; i < n; ++i) all = all && dv.fin_host[i] != 0;
    if (all) break;
  }
  HIPC(hipEventRecord(dv.ev[3], s));
  const int rc = dv.stage.finish(s);
  g->last_steps = done_steps;
  g->call.last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return rc;
}

extern "C" int vx_wsp_read(vx_wsp* g, const char* name, int32_t utt, float* dst, int64_t n_floats) {
  VXC(read_check(g, "vx_wsp", "recognize", name, utt, dst));
  const vx_wsp_config& c = g->cfg;
  const WspPlan& p = g->plan;
  const std::string nm = name;
  const bool keep = (c.flags & VX_WSP_KEEP_TAPS) != 0;
  if (nm == "logits") {  // the raw rows of the generated steps, one copy a step
    if (!keep) return fail(VX_ERR_STATE, "vx_wsp_read: logits needs VX_WSP_KEEP_TAPS at create");
    ON_DEVICE(g->device);
    HIPC(hipStreamSynchronize(g->call.last_stream));
    int count = 0;
    HIPC(hipMemcpy(&count, g->dev->state.get() + 2 * (size_t)c.max_batch + utt, sizeof(int), hipMemcpyDeviceToHost));
    if (n_floats != (int64_t)count * c.vocab)
      return fail(VX_ERR_ARG, "vx_wsp_read: logits of utterance %d is %d x %d floats, not %lld", utt, count, c.vocab, (long long)n_floats);
    for (int k = 0; k < count; ++k) {
      const size_t pos = (size_t)(g->last_prompt[utt] - 1 + k);
      HIPC(hipMemcpy(dst + (size_t)k * c.vocab, g->dev->ws.get() + p.tap + (pos * c.max_batch + utt) * c.vocab, (size_t)c.vocab * sizeof(float),
                     hipMemcpyDeviceToHost));
    }
    return VX_OK;
  }
  size_t base = 0;
  long rows = g->P;
  int width = c.d_model, l = 0;
  if (nm == "logmel") {
    base = p.mel; rows = g->F; width = c.n_mels;
  } else if (nm == "conv1") {
    base = p.c1; rows = g->F;
  } else if (nm == "features") {
    base = p.feat;
  } else if (nm == "encoder") {
    base = p.enc;
  } else if (tap_index(nm, "enc", c.enc_layers, l)) {
    if (!keep) return fail(VX_ERR_STATE, "vx_wsp_read: %s needs VX_WSP_KEEP_TAPS at create", name);
    base = p.hid + p.hid_stride * (size_t)l;
  } else {
    return fail(VX_ERR_ARG, "vx_wsp_read: unknown tap %s", name);
  }
  return read_rows(g, "vx_wsp", name, utt, base, (long)utt * rows, rows, width, dst, n_floats);
}

extern "C" int vx_wsp_get_timings(vx_wsp* g, double* out, int32_t n) {
  if (!g || !out || n < 0 || n > 7) return fail(VX_ERR_ARG, "vx_wsp_get_timings: null argument or n outside [0, 7]");
  double v[7] = {g->call.last_ms, (double)(g->plan.total * sizeof(float)),
                 (double)(g->packed.size() * sizeof(float) + g->packed16.size() * sizeof(uint16_t)), g->last_steps, 0.0, 0.0, 0.0};
  if (n > 4 && g->device >= 0 && g->call.last_n > 0) {  // the device times of the last call: waits for it
    ON_DEVICE(g->device);
    HIPC(hipEventSynchronize(g->dev->ev[3]));
    for (int i = 0; i < 3; ++i) {
      float ms = 0.f;
      HIPC(hipEventElapsedTime(&ms, g->dev->ev[i], g->dev->ev[i + 1]));
      v[4 + i] = ms;
    }
  }
  for (int i = 0; i < n; ++i) out[i] = v[i];
  return VX_OK;
}

// ---- the token loop's kernels on caller data (tests): the launchers above, no handle -----------------------------------------------
namespace {

// n ints of a device array, after what `s` holds has run.
int fetch_ints(const int* dev, size_t n, hipStream_t s, std::vector<int>& out) {
  out.resize(n);
  HIPC(hipMemcpyAsync(out.data(), dev, n * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

}  // namespace

extern "C" int vx_op_wsp_gemm(const float* x, const float* W, const float* bias, const float* res, float* out, int32_t M, int32_t N, int32_t K,
                              int32_t act, void* stream) {
  if (!x || !W || !out) return fail(VX_ERR_ARG, "vx_op_wsp_gemm: null argument");
  if (M < 1 || N < 1 || K < 1) return fail(VX_ERR_ARG, "vx_op_wsp_gemm: M %d, N %d, K %d", M, N, K);
  if (K % 4 != 0) return fail(VX_ERR_ARG, "vx_op_wsp_gemm: K = %d is no multiple of 4", K);
  if (M > SPK_MAX_SEG) return fail(VX_ERR_ARG, "vx_op_wsp_gemm: M = %d rows > %d", M, SPK_MAX_SEG);
  if (act != SPK_ACT_NONE && act != SPK_ACT_GELU) return fail(VX_ERR_ARG, "vx_op_wsp_gemm: act = %d", act);
  WspSkinnyArgs a{};
  a.x = x; a.W = W; a.bias = bias; a.res = res; a.out = out;
  a.M = M; a.N = N; a.K = K; a.ldo = N; a.act = act;
  hipStream_t s = (hipStream_t)stream;
  VXC(launch_skinny(a, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

extern "C" int vx_op_wsp_decode_attn(const float* q, const float* knew, const float* vnew, float* kcache, float* vcache, float* out, int32_t ld,
                                     int32_t ldq, int32_t d, int32_t H, int32_t n, const int32_t* pos, int32_t keys, int64_t rows_per_utt,
                                     int32_t max_keys, void* stream) {
  if (!q || !kcache || !vcache || !out) return fail(VX_ERR_ARG, "vx_op_wsp_decode_attn: null argument");
  if ((knew == nullptr) != (vnew == nullptr) || (knew == nullptr) != (pos == nullptr))
    return fail(VX_ERR_ARG, "vx_op_wsp_decode_attn: knew, vnew and pos come together (self-attention) or not at all (cross-attention)");
  if (max_keys < 1 || max_keys > WSP_MAX_KEYS) return fail(VX_ERR_ARG, "vx_op_wsp_decode_attn: max_keys = %d outside [1, %d]", max_keys, WSP_MAX_KEYS);
  if (n < 1 || n > SPK_MAX_SEG || H < 1 || d != 64 * H) return fail(VX_ERR_ARG, "vx_op_wsp_decode_attn: n %d, H %d, d %d (d = 64 H)", n, H, d);
  if (ld < d || ldq < d || ld % 4 != 0 || ldq % 4 != 0) return fail(VX_ERR_ARG, "vx_op_wsp_decode_attn: ld %d, ldq %d (multiples of 4, >= d = %d)", ld, ldq, d);
  if (rows_per_utt < 1 || rows_per_utt > WSP_MAX_KEYS) return fail(VX_ERR_ARG, "vx_op_wsp_decode_attn: rows_per_utt = %lld", (long long)rows_per_utt);
  const int room = (int)std::min<int64_t>(max_keys, rows_per_utt);
  if (!pos && (keys < 1 || keys > room)) return fail(VX_ERR_ARG, "vx_op_wsp_decode_attn: keys = %d outside [1, %d]", keys, room);
  hipStream_t s = (hipStream_t)stream;
  if (pos) {  // the kernel appends at row pos[u] and keeps pos[u] + 1 scores
    std::vector<int> hp;
    VXC(fetch_ints(pos, (size_t)n, s, hp));
    for (int u = 0; u < n; ++u)
      if (hp[u] < 0 || hp[u] >= room) return fail(VX_ERR_ARG, "vx_op_wsp_decode_attn: pos[%d] = %d outside [0, %d)", u, hp[u], room);
  }
  WspAttnArgs a{};
  a.q = q; a.knew = knew; a.vnew = vnew; a.kc = kcache; a.vc = vcache; a.out = out; a.pos = pos;
  a.ldq = ldq; a.ld = ld; a.d = d; a.keys = pos ? 0 : keys; a.rows_per_utt = rows_per_utt; a.scale = 0.125f;  // 64^-1/2
  VXC(launch_decode_attn(a, H, n, max_keys, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

extern "C" int vx_op_wsp_head(const float* logits, int32_t n, int32_t V, const uint8_t* suppress, const int32_t* prompt, int32_t prompt_stride,
                              const int32_t* n_prompt, const int32_t* max_new, const int32_t* forced, int32_t* cur, int32_t* pos, int32_t* count,
                              int32_t* finished, int32_t* tokens_out, float* logprobs_out, int32_t* counts_out, int32_t* stops_out,
                              int32_t out_stride, int32_t eos, int32_t max_target, void* stream) {
  if (!logits || !suppress || !prompt || !n_prompt || !max_new || !cur || !pos || !count || !finished || !tokens_out || !logprobs_out || !counts_out ||
      !stops_out)
    return fail(VX_ERR_ARG, "vx_op_wsp_head: null argument");
  if (n < 1 || n > SPK_MAX_SEG || V < 1 || prompt_stride < 1 || out_stride < 1)
    return fail(VX_ERR_ARG, "vx_op_wsp_head: n %d, V %d, prompt_stride %d, out_stride %d", n, V, prompt_stride, out_stride);
  if (eos < 0 || eos >= V) return fail(VX_ERR_ARG, "vx_op_wsp_head: eos = %d outside [0, %d)", eos, V);
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> hpos, hnp, hforced;  // what the kernel indexes with
  VXC(fetch_ints(pos, (size_t)n, s, hpos));
  VXC(fetch_ints(n_prompt, (size_t)n, s, hnp));
  if (forced) VXC(fetch_ints(forced, (size_t)n * out_stride, s, hforced));
  for (int u = 0; u < n; ++u) {
    if (hnp[u] < 1 || hnp[u] > prompt_stride) return fail(VX_ERR_ARG, "vx_op_wsp_head: n_prompt[%d] = %d outside [1, %d]", u, hnp[u], prompt_stride);
    const int g = hpos[u] + 1 - hnp[u];
    if (hpos[u] < 0 || g >= out_stride) return fail(VX_ERR_ARG, "vx_op_wsp_head: pos[%d] = %d: step %d outside [.., %d)", u, hpos[u], g, out_stride);
    if (forced && g >= 0 && (hforced[(size_t)u * out_stride + g] < 0 || hforced[(size_t)u * out_stride + g] >= V))
      return fail(VX_ERR_ARG, "vx_op_wsp_head: forced[%d][%d] = %d outside [0, %d)", u, g, hforced[(size_t)u * out_stride + g], V);
  }
  WspHeadArgs a{};
  a.logits = logits; a.suppress = suppress; a.prompt = prompt; a.n_prompt = n_prompt; a.max_new = max_new; a.forced = forced;
  a.st = WspState{cur, pos, count, finished};
  a.tokens_out = tokens_out; a.logprob_out = logprobs_out; a.count_out = counts_out; a.stop_out = stops_out; a.tap = nullptr;
  a.V = V; a.prompt_stride = prompt_stride; a.out_stride = out_stride; a.eos = eos; a.max_target = max_target; a.MB = n;
  wsp_head_reduce<<<n, 256, 0, s>>>(a);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

extern "C" int vx_op_wsp_embed(const float* tok_emb, const float* pos_emb, const int32_t* cur, const int32_t* pos, float* x, int32_t n, int32_t d,
                               int32_t vocab, int32_t max_pos, void* stream) {
  if (!tok_emb || !pos_emb || !cur || !pos || !x) return fail(VX_ERR_ARG, "vx_op_wsp_embed: null argument");
  if (n < 1 || n > SPK_MAX_SEG || d < 1 || vocab < 1 || max_pos < 1)
    return fail(VX_ERR_ARG, "vx_op_wsp_embed: n %d, d %d, vocab %d, max_pos %d", n, d, vocab, max_pos);
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> hc, hp;
  VXC(fetch_ints(cur, (size_t)n, s, hc));
  VXC(fetch_ints(pos, (size_t)n, s, hp));
  for (int u = 0; u < n; ++u)
    if (hc[u] < 0 || hc[u] >= vocab || hp[u] < 0 || hp[u] >= max_pos)
      return fail(VX_ERR_ARG, "vx_op_wsp_embed: utterance %d: token %d outside [0, %d) or position %d outside [0, %d)", u, hc[u], vocab, hp[u], max_pos);
  wsp_embed<<<n, 256, 0, s>>>(tok_emb, pos_emb, cur, pos, x, d);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

// ---- the bf16 encoder mode's kernels on caller data (tests): w2v_host.hpp's launchers, no handle -----------------------------------
extern "C" int vx_op_enc16_gemm(int32_t epi, const void* A_bf16, const void* W_bf16, const float* bias, const float* res, void* out, int64_t M,
                                int32_t N, int32_t K, void* stream) {
  if (M < 1) return fail(VX_ERR_ARG, "vx_op_enc16_gemm: M = %lld", (long long)M);
  hipStream_t s = (hipStream_t)stream;
  VXC(launch_ebf_gemm(epi, (const ebf_t*)A_bf16, (const ebf_t*)W_bf16, bias, res, out, (long)M, N, K, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

extern "C" int vx_op_enc16_add_ln(const float* a, const float* b, int32_t bmod, const float* w, const float* beta, float* sum, void* y_bf16,
                                  int64_t M, int32_t d, float eps, void* stream) {
  if (!a || !w || !beta || !y_bf16) return fail(VX_ERR_ARG, "vx_op_enc16_add_ln: null argument");
  if (M < 1 || d < 1 || bmod < 0 || (bmod > 0 && !b)) return fail(VX_ERR_ARG, "vx_op_enc16_add_ln: M %lld, d %d, bmod %d", (long long)M, d, bmod);
  hipStream_t s = (hipStream_t)stream;
  VXC(launch_ebf_add_ln(a, b, bmod, w, beta, sum, (ebf_t*)y_bf16, (long)M, d, eps, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}

extern "C" int vx_op_enc16_attn(const void* qkv_bf16, void* out_bf16, int32_t n, const int32_t* seg_len, int32_t heads, void* stream) {
  if (!qkv_bf16 || !out_bf16 || !seg_len) return fail(VX_ERR_ARG, "vx_op_enc16_attn: null argument");
  if (n < 1 || n > SPK_MAX_SEG || heads < 1) return fail(VX_ERR_ARG, "vx_op_enc16_attn: n %d segments (up to %d), %d heads", n, SPK_MAX_SEG, heads);
  std::vector<int> seg((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) {
    if (seg_len[i] < 0 || (long)seg[i] + seg_len[i] > 2147483647L) return fail(VX_ERR_ARG, "vx_op_enc16_attn: segment %d: %d rows", i, seg_len[i]);
    seg[i + 1] = seg[i] + seg_len[i];
  }
  hipStream_t s = (hipStream_t)stream;
  DevBuf<int> dseg;
  VXC(dseg.alloc((size_t)n + 1));
  HIPC(hipMemcpyAsync(dseg.get(), seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice, s));
  VXC(launch_ebf_attn((const ebf_t*)qkv_bf16, (ebf_t*)out_bf16, dseg.get(), seg.data(), n, heads, s));
  HIPC(hipStreamSynchronize(s));  // the tables go out of scope
  return VX_OK;
}
