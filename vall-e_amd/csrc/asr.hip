// CTC speech recogniser (Wav2Vec2ForCTC / HubertForCTC) behind the C ABI (include/vallex.h, vx_asr_*), the greedy CTC decode
// (vx_ctc_greedy), the forced alignment (vx_falign*) and the edit distance (vx_edit_distance).  The Wav2Vec2 backbone it shares with the
// speaker encoder (spk.hip) is w2v_host.hpp, in both flavours of layer 0 (group norm / asr_conv0_ln) and with the pre-norm layer loop
// Whisper's encoder runs too.  This unit keeps the post-norm loop of the group flavour, the CTC tail and the alignment.  A
// translation unit and a handle of its own, like spk.hip.
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
#include "falign_kernels.hpp"

using namespace vx;

namespace {

struct AsrDev : W2vDev {
  DevBuf<double> lp;
  DevBuf<int> ids;
  DevBuf<unsigned char> fal;  // vx_falign_asr's scratch, grow-only
  size_t fal_bytes = 0;
};

}  // namespace

struct vx_asr : W2vHandle<AsrDev> {
  vx_asr_config cfg{};
  size_t p_logits = 0;  // offset (floats) into the workspace, after the backbone's
  SpkLin head;          // filled by vx_asr_finalize
};

namespace {

int asr_init_device(vx_asr* g) {
  VXC(w2v_init_device(g, g->cfg.n_conv));
  const size_t rows = (size_t)g->cfg.max_batch * (size_t)g->m.Tmax;
  VXC(g->dev->lp.alloc(rows));
  return g->dev->ids.alloc(rows);
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

// The network up to the logits; *rows: the encoder's frames of the call.
int run_call(const vx_asr* g, const W2vRun& x, int flags, long* rows) {
  const vx_asr_config& c = g->cfg;
  const W2vWeights& bw = g->m.bw;
  const W2vPlan& p = g->m.p;
  const int d = c.hidden;
  float* ws = x.ws;
  // ---- feature encoder, projection, positional convolution
  EncRun e;
  VXC(w2v_run_features(x, (flags & VX_ASR_NORMALIZE) != 0, e));
  const long M = *rows = e.M;
  if (!c.do_stable_layer_norm) {  // post-norm: the speaker encoder's plain mode
    VXC(run_ln(x, bw.enc_ln, ws + p.x0, ws + p.tmp, e.hidden(0), M, d));
    for (int l = 0; l < c.layers; ++l) {
      const EncLayer& L = bw.layers[l];
      VXC(run_attention(x, e, L, e.hidden(l)));
      VXC(run_ln(x, L.ln1, e.hidden(l), e.tmp, e.mid, M, d));
      VXC(run_lin(x, L.ff1, e.mid, d, e.ff, M, SPK_ACT_GELU));
      VXC(run_lin(x, L.ff2, e.ff, c.ffn, e.tmp, M, SPK_ACT_NONE));
      VXC(run_ln(x, L.ln2, e.mid, e.tmp, e.hidden(l + 1), M, d));
    }
  } else {  // stable: x0 + the positional term is hidden state 0; encoder.layer_norm closes the stack
    if (g->bf16) {
      VXC(run_add_ln16(x, bw.layers[0].ln1, ws + p.x0, e.tmp, 0, e.hidden(0), e.nrm16, M, d));
      VXC(run_prenorm_layers_bf16(x, e, bw.layers, bw.enc_ln, nullptr, e.hidden(c.layers)));
    } else {
      VXC(run_add_ln(x, bw.layers[0].ln1, ws + p.x0, e.tmp, e.hidden(0), e.nrm, M, d));
      VXC(run_prenorm_layers(x, e, bw.layers, bw.enc_ln, nullptr, e.hidden(c.layers)));
    }
  }
  // ---- head
  return run_lin(x, g->head, e.hidden(c.layers), d, ws + g->p_logits, M, SPK_ACT_NONE);
}

}  // namespace

extern "C" int64_t vx_asr_frames(const vx_asr* g, int64_t n_samples) {
  return !g ? -1 : (int64_t)frames_of(g->m.q, (long)std::max<int64_t>(0, n_samples), g->cfg.n_conv - 1);
}

extern "C" int64_t vx_asr_min_samples(const vx_asr* g) { return !g ? -1 : (int64_t)g->m.min_samples; }

extern "C" int vx_asr_create(const vx_asr_config* cfg, vx_asr** out) {
  VXC(create_head("vx_asr_create", cfg, out));
  const vx_asr_config& c = *cfg;
  const char* what = "vx_asr_create";
  W2vGeom q = w2v_geom(c, c.feat_proj_layer_norm, (c.flags & VX_ASR_KEEP_TAPS) != 0);
  q.enc_bf16 = (c.flags & VX_ASR_ENC_BF16) != 0;
  VXC(w2v_validate(q, what, W2V_CHECK_SIZES));
  VXC(w2v_validate(q, what, W2V_CHECK_CONVS));
  if (c.pos_kernel < 1 || c.pos_groups < 1) return fail(VX_ERR_ARG, "vx_asr_create: pos_kernel %d, pos_groups %d", c.pos_kernel, c.pos_groups);
  if (c.vocab < 1 || c.blank < 0 || c.blank >= c.vocab) return fail(VX_ERR_ARG, "vx_asr_create: vocab %d, blank %d", c.vocab, c.blank);
  VXC(w2v_validate(q, what, W2V_CHECK_RATIOS));
  if (c.flags & ~(VX_ASR_KEEP_TAPS | VX_ASR_ENC_BF16)) return fail(VX_ERR_ARG, "vx_asr_create: flags = %d", c.flags);
  if (c.add_adapter != 0) return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: add_adapter");
  if (c.conv_pos_batch_norm != 0) return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: conv_pos_batch_norm");
  if (c.activation != 0) return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: activation = %d (gelu is served)", c.activation);
  if ((c.feat_extract_norm != 0) != (c.do_stable_layer_norm != 0))
    return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: feat_extract_norm = %d with do_stable_layer_norm = %d (group / post-norm and layer / stable are served)",
                c.feat_extract_norm, c.do_stable_layer_norm);
  if (c.feat_extract_norm != 0 && !c.conv_bias)
    return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: feat_extract_norm = \"layer\" without conv_bias");
  VXC(w2v_validate(q, what, W2V_CHECK_SERVED));
  if (c.feat_extract_norm != 0 && (c.conv_dim[0] > ASR_C0_MAXC || conv0_ln_lds_bytes(q) > (size_t)ASR_C0_LDS))
    return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: conv layer 0: dim %d x kernel %d (up to %d channels and %d bytes of tile are served)",
                c.conv_dim[0], c.conv_kernel[0], ASR_C0_MAXC, ASR_C0_LDS);
  VXC(w2v_validate(q, what, W2V_CHECK_BATCH));
  if (q.enc_bf16) {
    if (!c.do_stable_layer_norm)
      return fail(VX_ERR_UNSUPPORTED, "vx_asr_create: the bf16 encoder serves do_stable_layer_norm = 1 (the layer / stable flavour), not the group / post-norm one");
    VXC(enc_bf16_check(what, c.hidden, c.heads, c.ffn, "heads", "ffn"));
  }

  std::unique_ptr<vx_asr> g(new vx_asr());
  g->cfg = c;
  g->bf16 = q.enc_bf16 != 0;
  g->m.q = q;
  VXC(w2v_size(g->m, what, 1));  // one encoder frame
  w2v_plan_rows(g->m, true);
  g->p_logits = g->m.p.take((size_t)c.max_batch * (size_t)g->m.Tmax * (size_t)c.vocab);
  w2v_plan_stats(g->m);

  w2v_add_keys(g.get(), q);
  lin_keys(g.get(), "lm_head", c.vocab, c.hidden);
  *out = g.release();
  return VX_OK;
}

extern "C" void vx_asr_destroy(vx_asr* g) { destroy_handle(g); }

extern "C" int vx_asr_set_weight(vx_asr* g, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
  return set_weight(g, "vx_asr", key, data, shape, ndim);
}

extern "C" int vx_asr_finalize(vx_asr* g) {
  if (!g) return fail(VX_ERR_ARG, "vx_asr_finalize: null handle");
  if (g->finalized) return VX_OK;
  VXC(finalize_begin(g));
  w2v_pack(g, g->m.q, g->m.bw);
  for (int l = 0; l < g->cfg.layers; ++l) w2v_pack_layer(g, g->m.q, g->m.bw, l);
  g->head = pack_linear(g, "lm_head", g->cfg.vocab, g->cfg.hidden);
  finalize_end(g);
  return VX_OK;
}

extern "C" int vx_asr_recognize(vx_asr* g, int32_t n, const float* const* wav, const int32_t* n_samples, int32_t flags, int32_t* tokens_out,
                                int32_t* token_frames_out, int32_t* counts_out, float* mean_logprob_out, float* logits_out, void* stream) {
  if (!g || !wav || !n_samples || !tokens_out || !token_frames_out || !counts_out || !mean_logprob_out)
    return fail(VX_ERR_ARG, "vx_asr_recognize: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_asr_recognize: n = %d utterances", n);
  if (flags & ~VX_ASR_NORMALIZE) return fail(VX_ERR_ARG, "vx_asr_recognize: flags = %d", flags);
  if (!g->finalized) return fail(VX_ERR_STATE, "vx_asr_recognize before vx_asr_finalize");
  VXC(w2v_check_call(g, "vx_asr_recognize", n, wav, n_samples, "one encoder frame"));
  const vx_asr_config& c = g->cfg;
  const auto t_begin = std::chrono::steady_clock::now();
  VXC(ensure_device(g, asr_init_device));
  ON_DEVICE(g->device);
  AsrDev& dv = *g->dev;
  W2vRun x{};
  VXC(w2v_stage_begin(g, c.n_conv, n, wav, n_samples, (hipStream_t)stream, x));
  VXC(w2v_stage_commit(g, c.n_conv, x));
  long M = 0;
  VXC(run_call(g, x, flags, &M));
  const float* logits = dv.ws.get() + g->p_logits;
  VXC(launch_ctc(logits, c.vocab, c.blank, n, M, x.table(c.n_conv - 1), dv.ids.get(), dv.lp.get(), tokens_out, token_frames_out, counts_out,
                 mean_logprob_out, nullptr, x.s));
  if (logits_out) HIPC(hipMemcpyAsync(logits_out, logits, (size_t)M * c.vocab * sizeof(float), hipMemcpyDeviceToDevice, x.s));
  const int rc = dv.stage.finish(x.s);
  g->call.last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return rc;
}

extern "C" int vx_asr_read(vx_asr* g, const char* name, int32_t utt, float* dst, int64_t n_floats) {
  VXC(read_check(g, "vx_asr", "recognize", name, utt, dst));
  const int n = g->call.last_n;
  const vx_asr_config& c = g->cfg;
  const W2vPlan& p = g->m.p;
  const int te = c.n_conv - 1;
  const std::string nm = name;
  size_t base = 0;
  int table = te, width = c.hidden, l = 0;
  if (nm == "conv0") {
    table = 0; width = c.conv_dim[0]; base = p.c0;
  } else if (nm == "features") {
    base = te == 0 ? p.c0 : p.conv[te & 1]; width = c.conv_dim[te];
  } else if (nm == "logits") {
    base = g->p_logits; width = c.vocab;
  } else if (tap_index(nm, "hidden", c.layers, l)) {
    if (!(c.flags & VX_ASR_KEEP_TAPS)) return fail(VX_ERR_STATE, "vx_asr_read: %s needs VX_ASR_KEEP_TAPS at create", name);
    base = p.hid + p.hid_stride * (size_t)l;
  } else {
    return fail(VX_ERR_ARG, "vx_asr_read: unknown tap %s", name);
  }
  const int* seg = g->call.last_seg.data() + (size_t)table * (n + 1);
  return read_rows(g, "vx_asr", name, utt, base, seg[utt], (long)seg[utt + 1] - seg[utt], width, dst, n_floats);
}

extern "C" int vx_asr_get_timings(const vx_asr* g, double* out, int32_t n) {
  return w2v_timings(g, "vx_asr", g && g->dev ? g->dev->fal_bytes : 0, out, n);
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
  const int last_n = g->call.last_n;
  if (g->device < 0 || last_n == 0) return fail(VX_ERR_STATE, "vx_falign_asr before any vx_asr_recognize");
  if (n != last_n) return fail(VX_ERR_STATE, "vx_falign_asr: n = %d utterances, the last vx_asr_recognize served %d", n, last_n);
  const vx_asr_config& c = g->cfg;
  const int* seg = g->call.last_seg.data() + (size_t)(c.n_conv - 1) * (n + 1);
  std::vector<int> frames((size_t)n);
  for (int i = 0; i < n; ++i) frames[i] = seg[i + 1] - seg[i];
  FalPlan p;
  VXC(fal_plan("vx_falign_asr", c.vocab, c.blank, n, frames.data(), targets, target_len, o.max_half(), p));
  ON_DEVICE(g->device);
  AsrDev& dv = *g->dev;
  hipStream_t s = (hipStream_t)stream;
  HIPC(hipStreamWaitEvent(s, dv.stage.ev_done, 0));  // the logits of the last call, whatever stream it ran on
  if (p.bytes > dv.fal_bytes) {
    dv.fal_bytes = 0;
    VXC(dv.fal.alloc(p.bytes));
    dv.fal_bytes = p.bytes;
  }
  VXC(fal_launch(dv.ws.get() + g->p_logits, c.vocab, c.blank, n, targets, p, dv.fal.get(), o, s));
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
