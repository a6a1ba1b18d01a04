// libvallex.so — host side of the engine and the C ABI declared in include/vallex.h.
// One engine = one model replica on one GPU: weights, KV cache, activation arena, a private
// stream and the captured hipGraphs of the AR decode steps.  Every AR decode (batch-1, static
// batch, continuous-batching session) runs through one polled replay loop, replay_polled().
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <array>
#include <cstring>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "host.hpp"
#ifdef VX_STAMPS
__device__ unsigned long long g_vx_stamps[32];
__device__ unsigned long long* g_vx_kstamps = nullptr;
__device__ unsigned long long* g_fq_stamps = nullptr;
#endif
#include "ar_kernels.hpp"
#include "ar_tp.hpp"
#include "rows_kernels.hpp"
#include "mfma_kernels.hpp"
#include "batch_kernels.hpp"
#include "mx_kernels.hpp"
#include "logprob.hpp"
#include "align.hpp"
#include "meltf.hpp"

using namespace vx;

// ------------------------------------------------------------------------------ errors
// the one definition behind every unit's fail / HIPC (host.hpp)
static thread_local std::string g_err;
int vx::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

extern "C" const char* vx_last_error(void) { return g_err.c_str(); }

// ------------------------------------------------------------------------------ engine state
struct Tensor {
  void* p = nullptr;
  std::vector<int64_t> shape;
  size_t numel = 0;
  bool low = false;  // stored in the precision's matrix type (bf16 in VX_PREC_BF16)
  bool set = false;
  // VX_PREC_FP8_NAR: MXFP8 copy of the NAR stack's in_proj / linear1 / linear2 (mx_kernels.hpp): e4m3 bytes (N, K) and E8M0
  // block scales (K/32, N); the bf16 copy stays (row counts below the 256-tile path run on it)
  uint8_t *q8 = nullptr, *s8 = nullptr;
};

struct LayerW {
  const uint8_t *in_q8 = nullptr, *in_s8 = nullptr, *w1_q8 = nullptr, *w1_s8 = nullptr, *w2_q8 = nullptr, *w2_s8 = nullptr;
  const void *in_w, *out_w, *w1, *w2;
  const float *in_b, *out_b, *b1, *b2;
  const float *n1_g, *n1_b, *n2_g, *n2_b;
  // VALL-F (TransformerDecoderLayer): cross-attention over the text memory and the third norm
  const void *cin_w = nullptr, *cout_w = nullptr;
  const float *cin_b = nullptr, *cout_b = nullptr, *n3_g = nullptr, *n3_b = nullptr;
};

constexpr int POLL_CHUNK = 32;
// vx_batch_run's default stop-poll interval in steps (poll_steps <= 0): see DESIGN.md "Continuous batching" for the measurement
constexpr int BATCH_POLL_DEFAULT = 8;
enum SlotState { SLOT_VACANT = 0, SLOT_LIVE = 1, SLOT_STOPPED = 2 };  // continuous-batching session (vx_batch_open)

struct vx_engine {
  vx_config cfg{};
  bool bf16 = false;
  bool fp8nar = false;  // VX_PREC_FP8_NAR: bf16 everywhere + MXFP8 QKV / FFN GEMMs in the NAR stages at >= 4096 rows
  uint8_t *Hn8 = nullptr, *SHn = nullptr, *FF8 = nullptr, *SFF = nullptr;  // MXFP8 row operands and their scales (ld = mx_ld)
  int mx_ld = 0;
  bool vallf = false;  // VX_FLAG_VALLF: decoder layers with cross-attention over the text (valle.py:49-719)
  bool mel = false;    // the decoder side of a vx_mel handle (mel-Transformer, below): its own key table, no token head
  int npl = 2;         // norms per layer: 2 (encoder layers) / 3 (decoder layers)
  void *xkv_ar = nullptr, *xkv_nar = nullptr;  // VALL-F: per-layer K / V of the text memory, [layer][K|V][head][max_text][hd]
  int mem_len = 0;     // text rows of the current utterance's AR memory
  bool hd64 = true;  // head_dim 64 in both stacks: the MFMA row kernels and the batched decode apply
  size_t esz = 4;  // bytes per matrix / KV / GEMM-operand element
  int num_cu = 256;
  hipStream_t es = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_t[6] = {};
  hipEvent_t ev_poll[2] = {};
  std::unordered_map<std::string, Tensor> w;
  std::vector<std::string> keys;
  bool finalized = false;
  std::vector<LayerW> ar_l, nar_l;
  // sine tables
  float *pe_ar = nullptr, *pe_nar = nullptr;
  int pe_rows = 0;
  bool pe_ar_set = false, pe_nar_set = false;
  // AR buffers
  int ctx_max = 0;
  float *ar_x = nullptr, *ar_xn = nullptr, *ar_q = nullptr, *ar_part = nullptr, *ar_f = nullptr, *ar_logits = nullptr;
  void* kv = nullptr;  // [L][2][H][ctx_max][hd]
  // in-launch hand-overs of the sharded decode step (ar_granules.hpp): per-layer granule scratch, the step counter that tags the
  // granules ([0]) and the spin-timeout word ([1])
  // XCD-sharded decode step (ar_tp.hpp): two launches per layer.  Re-laid-out out-projection / linear2 weights per layer, the
  // partial-sum vectors of the two sharded GEMVs, the second residual buffer, the hidden-unit granules
  bool tp = false;
  std::vector<void*> tp_wo, tp_w2;
  long long* tp_xacc = nullptr;  // (3, d) int64 fixed-point residual accumulators in rotation (ar_tp.hpp TpAccArgs)
  float* tp_gbb = nullptr;  // (2 L + 1, 3, d): {gamma, beta, arriving bias} per norm site of the step
  fq_gran* tp_gh = nullptr;
  fq_gran *fq_gq = nullptr, *fq_gp = nullptr;
  unsigned* d_epoch = nullptr;
  ArState* d_st = nullptr;
  ArState* h_st = nullptr;  // pinned: [0] staging, [1..2] poll slots
  int *d_tokens = nullptr, *d_sampled = nullptr, *d_argmax = nullptr;
  float* d_noise = nullptr;
  size_t noise_cap = 0;
  long long* d_forced = nullptr;
  size_t forced_cap = 0;
  // row buffers
  int n_max = 0;
  float* X = nullptr;
  void *Hn = nullptr, *QKV = nullptr, *ATT = nullptr, *FF = nullptr, *VT = nullptr;
  int vt_ld = 0;
  float *yemb = nullptr, *nar_logits = nullptr, *ada = nullptr;
  long long *ids_text = nullptr, *ids_audio = nullptr, *ids_prompts = nullptr, *ids_samples = nullptr, *d_codes = nullptr;
  long long* d_fcodes = nullptr;  // teacher-forced NAR stages (vx_nar_ex): the caller's (T, Q) codes
  // scoring (vx_score / vx_score_batch), allocated at the first call: logits rows of the AR scoring pass (sc_ld floats each),
  // per-row results and int64 targets for sc_cap rows; the predict layer padded to NLL_MAXV rows for the MFMA GEMM; VALL-F:
  // the text memory of the scored utterance (xkv_ar's layout - the batch-1 decode's own memory is not touched)
  float *sc_logits = nullptr, *sc_nll = nullptr;
  int *sc_rank = nullptr, *sc_argmax = nullptr;
  long long* sc_tgt = nullptr;
  size_t sc_cap = 0;
  int sc_ld = 0, sc_rows = 0;  // sc_rows: AR rows scored by the last call (tap "score_ar_argmax")
  void *sc_head = nullptr, *xkv_score = nullptr;
  double t_score_ar = 0, t_score_nar = 0;
  // alignment (vx_align), allocated at the first call and grown on demand: the (T, Sw) map, the per-row text mass, the path with
  // its score and back-pointers, the (L, H) head weights and, when the caller's per-head buffer is host memory, its staging
  float *al_attn = nullptr, *al_mass = nullptr, *al_w = nullptr, *al_ph = nullptr;
  int* al_path = nullptr;
  double* al_score = nullptr;
  unsigned char* al_bp = nullptr;
  size_t al_cells = 0, al_rows = 0, al_ph_cells = 0;
  // ... of vx_align_batch besides: every head's own cells and row masses (align_seg_scratch), the descriptors of the tap and of
  // the path launch (2 BMAX), one path score per utterance (BMAX)
  float* al_scr = nullptr;
  AlignSeg* al_segs = nullptr;
  double* al_bscore = nullptr;
  size_t al_scr_floats = 0;
  double t_align = 0;
  // batched decode (slots)
  int bmax = 0;
  float *bx = nullptr, *bq = nullptr, *bpart = nullptr, *blogits = nullptr, *btrace = nullptr;
  vx::bf16 *bh = nullptr, *batt = nullptr, *bff = nullptr, *bkv = nullptr;
  size_t bkv_slot = 0;  // elements per slot
  bool kv8 = false;                           // VX_FLAG_KV_FP8: the slot caches are bkv8 / bkv8s, bkv stays null
  uint8_t *bkv8 = nullptr, *bkv8s = nullptr;  // e4m3 codes (bkv_slot bytes per slot), E8M0 scales (one per 16 codes)
  // VALL-F: the text memory of every slot, [slot][layer][K|V][head][max_text][64] (xkv_ar's layout per slot); bmem_slot elements
  vx::bf16* bmem = nullptr;
  size_t bmem_slot = 0;
  // VX_FLAG_VALLF_ROWS: the segmented row passes' text memories (TextMem).  xmem_rows: the batched NAR's packed per-call buffer,
  // [layer][K|V][head][cap_text][64] bf16 (grown by ensure_rows with cap_text); per-segment descriptors on the device
  bool vf_rows = false;
  vx::bf16* xmem_rows = nullptr;
  long long* d_mem_off = nullptr;
  int *d_mem_klen = nullptr, *d_mem_trow = nullptr;
  ArState* bst = nullptr;    // device, BMAX
  ArState* h_bst = nullptr;  // pinned: [0..BMAX) staging, [BMAX..3*BMAX) two poll slots
  int *btok = nullptr, *bsamp = nullptr, *bargm = nullptr;
  int btok_stride = 0;
  std::unordered_map<int, hipGraphExec_t> bgraphs;
  // segment layout of the concatenated row passes (seg_layout): start and length per segment, and for a batched prefill each
  // segment's text length (prefix mask) and slot
  int *d_seg_start = nullptr, *d_seg_len = nullptr, *d_seg_text = nullptr, *d_seg_slot = nullptr;
  // prenets (VX_FLAG_PRENET): scratch rows, conv weights re-laid out as [k][ci][co], decode-step vectors
  float *pn_a = nullptr, *pn_b = nullptr, *pn_h1 = nullptr, *pn_h2 = nullptr, *pn_text = nullptr, *d_zero = nullptr;
  float *ar_e = nullptr, *ar_h1 = nullptr, *ar_h2 = nullptr;
  float* convT[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  float* slab = nullptr;                              // split-K slabs of the N = d row GEMMs (4 x slab_rows x d fp32)
  int slab_rows = 0;
  long long *bp_text = nullptr, *bp_audio = nullptr;  // id staging of the batched prefill
  size_t cap_audio = 0, cap_text = 0;                 // rows the id / yemb / logits staging buffers hold
  int bS[BMAX] = {}, bP[BMAX] = {}, bbos[BMAX] = {}, bngen[BMAX] = {}, breason[BMAX] = {};
  bool bprefilled[BMAX] = {};
  // continuous-batching session (vx_batch_open / _admit / _run): per-slot state, the steps a live slot may still take before its
  // stop rule must have fired, and whether its bound was clamped to the KV capacity
  bool bsess = false;
  int bslot[BMAX] = {};
  long long bleft[BMAX] = {};
  bool bcap[BMAX] = {};
  double t_bdecode = 0, n_blaunch = 0;
  // VX_FLAG_LOGPROBS: the model's log-probability of every emitted token.  d_lp / blp: one fp32 per pass next to d_sampled /
  // bsamp (same indexing), written by the sampler's LP instantiation; nar_lp: [stage][generated rows of the last NAR call], written
  // by argmax_lp_rows_kernel, with that call's row offset and length per utterance.  All null without the flag.
  bool lpon = false;
  float *d_lp = nullptr, *blp = nullptr, *nar_lp = nullptr;
  int bnpass[BMAX] = {};  // passes of a stopped slot's decode (0: none finished)
  std::vector<int> nlp_off, nlp_T;
  int nlp_rows = 0;
  hipGraphExec_t gexec = nullptr;  // the batch-1 step
  int gexec_nodes = 0;             // kernel launches captured in it (vx_get_timings out[9])
  // per-utterance state
  int S = 0, P = 0, bos = 0;
  bool prefilled = false, decoded = false;
  int n_gen = 0, stop_reason = 0, n_pass = 0, last_T = 0, last_N = 0;
  double t_prefill = 0, t_decode = 0, t_nar = 0, n_launch = 0;
  // VX_TIME_GEMMS=1 (bench.py): HIP-event pairs around every QKV / out-projection / FFN GEMM of the NAR stages
  std::vector<hipEvent_t> gemm_ev;
  size_t gemm_ev_used = 0;
  double gemm_flops = 0, t_gemm = 0, gemm_flops_done = 0;
  std::vector<void*> allocs;
  char* arena = nullptr;
  size_t arena_used = 256, arena_cap = (size_t)4 << 20;  // no sub-block equals the base pointer (which `allocs` owns)
};

// Every VX_POISON fill (poison_on(), host.hpp) below goes to the engine's stream: `es` is a non-blocking stream, a null-stream
// hipMemset is not ordered with the kernels enqueued on it right afterwards (a fill landing late would wipe rows the first kernels
// had already written).
static int dalloc(vx_engine* e, void** p, size_t bytes) {
  // small blocks (the decode step's vectors, states, per-site norm parameters) share ONE 4 MB block: one translation entry
  // serves them all (each is touched by every workgroup of every launch of the step)
  static const bool arena_on = !(getenv("VX_ARENA") && atoi(getenv("VX_ARENA")) == 0);
  if (arena_on && bytes <= (64u << 10)) {
    const size_t need = (bytes ? bytes : 16) + 255 & ~(size_t)255;
    if (e->arena == nullptr) {
      HIPC(hipMalloc((void**)&e->arena, e->arena_cap));
      e->allocs.push_back(e->arena);
    }
    if (e->arena_used + need <= e->arena_cap) {
      *p = e->arena + e->arena_used;
      e->arena_used += need;
      if (poison_on()) {
        HIPC(hipMemsetAsync(*p, 0xFF, need, e->es));
        HIPC(hipStreamSynchronize(e->es));
      }
      return VX_OK;
    }
  }
  HIPC(hipMalloc(p, bytes ? bytes : 16));
  if (poison_on()) {  // debug mode: also finished before anything on another stream (weight uploads) can touch the block
    HIPC(hipMemsetAsync(*p, 0xFF, bytes ? bytes : 16, e->es));
    HIPC(hipStreamSynchronize(e->es));
  }
  e->allocs.push_back(*p);
  return VX_OK;
}
template <typename T> static int dalloc_t(vx_engine* e, T** p, size_t n) { return dalloc(e, (void**)p, n * sizeof(T)); }

constexpr int PRENET_H = 256;  // hidden width of the audio prenets (valle.py:116-122)

static bool is_matrix_key(const std::string& k) {
  auto ends = [&](const char* s) { size_t n = strlen(s); return k.size() >= n && k.compare(k.size() - n, n, s) == 0; };
  if (k.find("project_layer") != std::string::npos) return false;
  return ends("in_proj_weight") || ends("out_proj.weight") || ends("linear1.weight") || ends("linear2.weight") ||
         k.rfind("ar_predict_layer", 0) == 0 || k.rfind("nar_predict_layers", 0) == 0;
}

static bool is_mx_key(const std::string& k) {  // the NAR stack's QKV / FFN matrices (BASELINE configs[4])
  auto ends = [&](const char* s) { size_t n = strlen(s); return k.size() >= n && k.compare(k.size() - n, n, s) == 0; };
  return k.rfind("nar_decoder.layers.", 0) == 0 && (ends("in_proj_weight") || ends("linear1.weight") || ends("linear2.weight"));
}

// The reference's state_dict layout (valle.py:85-259); mirrored by valle_amd/weights.py.
// with_cross: -1 = as the engine (decoder layers in a VALL-F engine), 0 / 1 = encoder / decoder layers whatever the engine is
static void add_encoder_keys(vx_engine* e, const std::string& pre, int d, int L, bool adaptive, int with_cross = -1) {
  const bool post = e->cfg.flags & VX_FLAG_POST_NORM;  // norm=... if norm_first else None (valle.py:151, 242-246)
  const bool cross = with_cross < 0 ? (e->cfg.flags & VX_FLAG_VALLF) != 0 : with_cross != 0;  // TransformerDecoderLayer (modules/transformer.py:412-500)
  auto add = [&](const std::string& k, std::vector<int64_t> s) {
    Tensor t; t.shape = s; t.numel = 1; for (auto v : s) t.numel *= (size_t)v;
    t.low = e->bf16 && is_matrix_key(k);
    e->w[k] = t; e->keys.push_back(k);
  };
  auto norm = [&](const std::string& p) {
    if (adaptive) {
      add(p + ".project_layer.weight", {2 * d, d}); add(p + ".project_layer.bias", {2 * d});
      add(p + ".norm.weight", {d}); add(p + ".norm.bias", {d});
    } else {
      add(p + ".weight", {d}); add(p + ".bias", {d});
    }
  };
  for (int i = 0; i < L; ++i) {
    const std::string p = pre + ".layers." + std::to_string(i);
    add(p + ".self_attn.in_proj_weight", {3 * d, d}); add(p + ".self_attn.in_proj_bias", {3 * d});
    add(p + ".self_attn.out_proj.weight", {d, d}); add(p + ".self_attn.out_proj.bias", {d});
    if (cross) {
      add(p + ".multihead_attn.in_proj_weight", {3 * d, d}); add(p + ".multihead_attn.in_proj_bias", {3 * d});
      add(p + ".multihead_attn.out_proj.weight", {d, d}); add(p + ".multihead_attn.out_proj.bias", {d});
    }
    add(p + ".linear1.weight", {4 * d, d}); add(p + ".linear1.bias", {4 * d});
    add(p + ".linear2.weight", {d, 4 * d}); add(p + ".linear2.bias", {d});
    norm(p + ".norm1"); norm(p + ".norm2");
    if (cross) norm(p + ".norm3");
  }
  if (!post) norm(pre + ".norm");
}

static void mel_key_table(vx_engine* e);
static void build_key_table(vx_engine* e) {
  if (e->mel) return mel_key_table(e);
  const vx_config& c = e->cfg;
  const int d = c.d_model, dn = c.nar_d_model, Q = c.num_quantizers;
  auto add = [&](const std::string& k, std::vector<int64_t> s) {
    Tensor t; t.shape = s; t.numel = 1; for (auto v : s) t.numel *= (size_t)v;
    t.low = e->bf16 && is_matrix_key(k);
    e->w[k] = t; e->keys.push_back(k);
  };
  add("ar_text_embedding.word_embeddings.weight", {512, d});
  add("nar_text_embedding.word_embeddings.weight", {512, dn});
  add("ar_audio_embedding.word_embeddings.weight", {1025 + (c.prepend_bos ? 1 : 0), d});
  // prenets (valle.py:96-123, 181-213): Sequential indices as in the reference; BatchNorm's num_batches_tracked is an
  // integer counter the forward pass never reads and is not passed through the C ABI
  auto prenet = [&](const std::string& pre, int dd) {
    for (int conv : {1, 5, 9}) {
      const std::string cv = pre + "_text_prenet." + std::to_string(conv), bn = pre + "_text_prenet." + std::to_string(conv + 1);
      add(cv + ".weight", {dd, dd, 5}); add(cv + ".bias", {dd});
      add(bn + ".weight", {dd}); add(bn + ".bias", {dd}); add(bn + ".running_mean", {dd}); add(bn + ".running_var", {dd});
    }
    add(pre + "_text_prenet.14.weight", {dd, dd}); add(pre + "_text_prenet.14.bias", {dd});
    add(pre + "_audio_prenet.0.weight", {PRENET_H, dd}); add(pre + "_audio_prenet.0.bias", {PRENET_H});
    add(pre + "_audio_prenet.3.weight", {PRENET_H, PRENET_H}); add(pre + "_audio_prenet.3.bias", {PRENET_H});
    add(pre + "_audio_prenet.6.weight", {dd, PRENET_H}); add(pre + "_audio_prenet.6.bias", {dd});
  };
  const bool pn = c.flags & VX_FLAG_PRENET;
  if (pn) prenet("ar", d);
  add("ar_text_position.alpha", {1});
  add("ar_audio_position.alpha", {1});
  add_encoder_keys(e, "ar_decoder", d, c.num_layers, false);
  add("ar_predict_layer.weight", {1025, d});
  if (Q > 1) {
    add("nar_audio_embeddings.0.word_embeddings.weight", {1025, dn});
    for (int j = 1; j < Q; ++j) add("nar_audio_embeddings." + std::to_string(j) + ".word_embeddings.weight", {1024, dn});
    if (pn) prenet("nar", dn);
    add("nar_text_position.alpha", {1});
    add("nar_audio_position.alpha", {1});
    add_encoder_keys(e, "nar_decoder", dn, c.nar_num_layers, true);
    for (int j = 0; j < Q - 1; ++j) add("nar_predict_layers." + std::to_string(j) + ".weight", {1024, dn});
    for (int j = 0; j < Q - 1; ++j) add("nar_stage_embeddings." + std::to_string(j) + ".word_embeddings.weight", {1, dn});
  }
}

static void host_sine_table(std::vector<float>& t, int rows, int d) {
  t.assign((size_t)rows * d, 0.f);
  for (int i = 0; i < d; i += 2) {
    const float w = expf((float)i * -(logf(10000.0f) / (float)d));
    for (int p = 0; p < rows; ++p) {
      t[(size_t)p * d + i] = sinf((float)p * w);
      if (i + 1 < d) t[(size_t)p * d + i + 1] = cosf((float)p * w);
    }
  }
}

// ------------------------------------------------------------------------------ create/destroy
static int create_body(vx_engine* e);
static int tp_setup(vx_engine* e);
extern "C" void vx_destroy(vx_engine* e);
extern "C" int vx_create(const vx_config* cfg, vx_engine** out) {
  if (!cfg || !out) return fail(VX_ERR_ARG, "null argument");
  if (cfg->struct_size != (int32_t)sizeof(vx_config)) return fail(VX_ERR_ARG, "vx_config.struct_size mismatch");
  const vx_config& c = *cfg;
  if (c.d_model <= 0 || c.nhead <= 0 || c.num_layers <= 0 || c.d_model % c.nhead)
    return fail(VX_ERR_ARG, "bad d_model/nhead/num_layers");
  if (c.num_quantizers < 1 || c.num_quantizers > 8) return fail(VX_ERR_ARG, "num_quantizers must be 1..8");
  if (c.prefix_mode != 0 && c.prefix_mode != 1 && c.prefix_mode != 2 && c.prefix_mode != 4)
    return fail(VX_ERR_ARG, "prefix_mode must be 0/1/2/4");
  // ahead of the general geometry rules, so that a refused combination is reported against the flag that asked for it
  if ((c.flags & VX_FLAG_VALLF_ROWS) &&
      (!(c.flags & VX_FLAG_VALLF) || c.max_batch < 2 || c.precision != VX_PREC_BF16 || c.d_model / c.nhead != 64 ||
       (c.num_quantizers > 1 && c.nar_nhead > 0 && c.nar_d_model / c.nar_nhead != 64) ||
       (c.flags & (VX_FLAG_POST_NORM | VX_FLAG_PRENET | VX_FLAG_KV_FP8 | VX_FLAG_SIMPLE_ROWS))))
    return fail(VX_ERR_UNSUPPORTED, "VX_FLAG_VALLF_ROWS needs VX_FLAG_VALLF, max_batch >= 2, bf16 precision, head_dim 64, a pre-norm model "
                                    "without prenets, bf16 slot caches and the MFMA row kernels");
  // head_dim 64 is the built geometry (MFMA attention, batched decode); 4 / 8 / 16 / 32 run on the plain kernels, batch-1
  // only: the reference's own tests use decoder_dim 64 / nhead 16 and half of that for the NAR stack (valle_test.py:93-95)
  auto hd_ok = [](int hd) { return hd == 4 || hd == 8 || hd == 16 || hd == 32 || hd == 64; };
  if (c.num_quantizers > 1 && (c.nar_nhead <= 0 || c.nar_d_model % c.nar_nhead)) return fail(VX_ERR_ARG, "bad nar_d_model/nar_nhead");
  if (!hd_ok(c.d_model / c.nhead) || (c.num_quantizers > 1 && !hd_ok(c.nar_d_model / c.nar_nhead)))
    return fail(VX_ERR_UNSUPPORTED, "head_dim (d_model/nhead) must be 4, 8, 16, 32 or 64");
  const bool hd64 = c.d_model / c.nhead == 64 && (c.num_quantizers == 1 || c.nar_d_model / c.nar_nhead == 64);
  if (c.d_model % 8 || c.d_model > 1024 || c.nar_d_model > 1024 || (c.num_quantizers > 1 && c.nar_d_model % 8))
    return fail(VX_ERR_UNSUPPORTED, "d_model must be a multiple of 8 and <= 1024");
  if (hd64 && (c.d_model % 64 || (c.num_quantizers > 1 && c.nar_d_model % 64)))
    return fail(VX_ERR_UNSUPPORTED, "d_model must be a multiple of 64 at head_dim 64");
  if (!hd64 && c.max_batch > 1) return fail(VX_ERR_UNSUPPORTED, "batched decode needs head_dim 64");
  if (c.max_text <= 0 || c.max_audio <= 0) return fail(VX_ERR_ARG, "capacities must be positive");
  if (c.precision != VX_PREC_F32 && c.precision != VX_PREC_BF16 && c.precision != VX_PREC_FP8_NAR) return fail(VX_ERR_ARG, "bad precision");
  if (c.precision == VX_PREC_FP8_NAR && (c.num_quantizers < 2 || c.nar_d_model % 256 || c.nar_d_model / c.nar_nhead != 64 ||
                                         (c.flags & (VX_FLAG_POST_NORM | VX_FLAG_PRENET | VX_FLAG_SIMPLE_ROWS))))
    return fail(VX_ERR_UNSUPPORTED, "VX_PREC_FP8_NAR needs a pre-norm NAR stack without prenets, head_dim 64 and nar_d_model %% 256 == 0");
  if ((c.flags & (VX_FLAG_POST_NORM | VX_FLAG_PRENET)) && c.max_batch > 1)
    return fail(VX_ERR_UNSUPPORTED, "post-norm / prenet models (VALL-E or VALL-F) run on the batch-1 path only");
  if ((c.flags & VX_FLAG_VALLF) && c.precision == VX_PREC_FP8_NAR) return fail(VX_ERR_UNSUPPORTED, "VX_PREC_FP8_NAR is built for VALL-E only");
  if (c.max_batch < 0 || c.max_batch > BMAX) return fail(VX_ERR_ARG, "max_batch must be 0..%d", BMAX);
  // bgemm_kernel runs K = ns x kgroups x 128 with ns in {1, 2, 4, 8} and kgroups_for(K) in {1, 4}: the step's K = d and 4 d fit
  // those forms at exactly these four widths (384, 640, 768 and 896 would need ns = 3, 5, 6 or 7)
  if (c.max_batch > 1 && (c.precision == VX_PREC_F32 || (c.d_model != 128 && c.d_model != 256 && c.d_model != 512 && c.d_model != 1024)))
    return fail(VX_ERR_UNSUPPORTED, "batched decode needs bf16 precision and d_model in {128, 256, 512, 1024}");
  if ((c.flags & VX_FLAG_KV_FP8) && (c.max_batch < 2 || c.precision == VX_PREC_F32 || c.d_model / c.nhead != 64 ||
                                     (c.flags & (VX_FLAG_POST_NORM | VX_FLAG_PRENET | VX_FLAG_VALLF))))
    return fail(VX_ERR_UNSUPPORTED, "VX_FLAG_KV_FP8 needs max_batch >= 2, bf16 / fp8nar precision, head_dim 64 and a pre-norm VALL-E "
                                    "without prenets");

#ifdef VX_STAMPS
  if (c.flags & VX_FLAG_LOGPROBS)  // its sampler lives in logprob.hip, which the stamp ring (a device global of this unit) does not reach
    return fail(VX_ERR_UNSUPPORTED, "VX_FLAG_LOGPROBS is not available in the in-kernel stamp build: its sampler launch would go unstamped");
#endif
  ON_DEVICE(c.device);
  vx_engine* e = new vx_engine();
  e->cfg = c;
  const int rc = create_body(e);
  if (rc != VX_OK) {  // g_err holds the failing call; release whatever was allocated up to it
    const std::string keep = g_err;
    vx_destroy(e);
    g_err = keep;
    return rc;
  }
  *out = e;
  return VX_OK;
}

// Every engine batches its row passes (a batch-1 engine still runs vx_nar_batch): the segment arrays, BMAX entries each.
static int seg_alloc(vx_engine* e) {
  for (int** p : {&e->d_seg_start, &e->d_seg_len, &e->d_seg_text, &e->d_seg_slot}) VXC(dalloc_t(e, p, (size_t)BMAX));
  return VX_OK;
}

static int create_body(vx_engine* e) {
  const vx_config& c = e->cfg;
  const bool hd64 = c.d_model / c.nhead == 64 && (c.num_quantizers == 1 || c.nar_d_model / c.nar_nhead == 64);
  e->bf16 = c.precision != VX_PREC_F32;
  e->fp8nar = c.precision == VX_PREC_FP8_NAR;
  e->hd64 = hd64;
  e->vallf = c.flags & VX_FLAG_VALLF;
  e->npl = e->vallf ? 3 : 2;
  e->esz = e->bf16 ? 2 : 4;
  hipDeviceProp_t prop;
  HIPC(hipGetDeviceProperties(&prop, c.device));
  e->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  HIPC(hipStreamCreateWithFlags(&e->es, hipStreamNonBlocking));
  HIPC(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
  HIPC(hipEventCreateWithFlags(&e->ev_out, hipEventDisableTiming));
  for (auto& ev : e->ev_t) HIPC(hipEventCreate(&ev));
  for (auto& ev : e->ev_poll) HIPC(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  build_key_table(e);

  const int d = c.d_model, dn = c.num_quantizers > 1 ? c.nar_d_model : c.d_model;
  const int dmax = d > dn ? d : dn;
  e->ctx_max = c.max_text + c.max_audio;
  e->n_max = e->ctx_max;
  const int H = c.nhead, hd = d / H;
  // sine tables (embedding.py:64 starts at 4000 rows and extends on demand)
  e->pe_rows = e->ctx_max > 4000 ? e->ctx_max : 4000;
  VXC(dalloc_t(e, &e->pe_ar, (size_t)e->pe_rows * d));
  VXC(dalloc_t(e, &e->pe_nar, (size_t)e->pe_rows * dn));
  // AR
  VXC(dalloc_t(e, &e->ar_x, d));
  VXC(dalloc_t(e, &e->ar_q, d));
  VXC(dalloc_t(e, &e->ar_xn, d));  // post-norm decode: the normalised residual stream
  VXC(dalloc_t(e, &e->ar_part, (size_t)H * ATT_NSPLIT * ATT_PSTRIDE));
  VXC(dalloc_t(e, &e->ar_f, 4 * (size_t)d));
  VXC(dalloc_t(e, &e->d_epoch, 2));
  {
    const unsigned init[2] = {1u, 0u};  // tags start at 1: zero-filled granules never match
    HIPC(hipMemcpy(e->d_epoch, init, sizeof init, hipMemcpyHostToDevice));
  }
  VXC(tp_setup(e));
  const size_t nlog = (c.flags & VX_FLAG_TRACE_LOGITS) ? (size_t)c.max_audio + 2 : 1;
  VXC(dalloc_t(e, &e->ar_logits, LOGITS_CUR + nlog * AR_VOCAB));
  VXC(dalloc(e, &e->kv, (size_t)c.num_layers * 2 * H * e->ctx_max * hd * e->esz));
  VXC(dalloc_t(e, &e->d_st, 1));
  HIPC(hipHostMalloc((void**)&e->h_st, 3 * sizeof(ArState) + 16));  // + {epoch, spin-timeout word} read back per decode
  VXC(dalloc_t(e, &e->d_tokens, (size_t)c.max_audio + 2));
  VXC(dalloc_t(e, &e->d_sampled, (size_t)c.max_audio + 2));
  VXC(dalloc_t(e, &e->d_argmax, (size_t)c.max_audio + 2));
  // rows
  const size_t n = e->n_max;
  VXC(dalloc_t(e, &e->X, n * dmax));
  VXC(dalloc(e, &e->Hn, n * dmax * e->esz));
  VXC(dalloc(e, &e->QKV, n * 3 * dmax * e->esz));
  VXC(dalloc(e, &e->ATT, n * dmax * e->esz));
  // rows between the segments of a concatenated batch are never written by attention but are read by the
  // out-projection: they must hold finite values (a NaN row would reach valid rows as 0 x NaN through its V^T column)
  HIPC(hipMemsetAsync(e->ATT, 0, n * dmax * e->esz, e->es));
  e->vt_ld = ((e->n_max + 63) / 64) * 64 + 64;  // key-padded row length of V^T (16-byte aligned tiles)
  VXC(dalloc(e, &e->VT, (size_t)dmax * e->vt_ld * 2));
  HIPC(hipMemsetAsync(e->VT, 0, (size_t)dmax * e->vt_ld * 2, e->es));  // padding keys must stay finite (they meet P = 0)
  VXC(dalloc(e, &e->FF, n * 4 * dmax * e->esz));
  VXC(dalloc_t(e, &e->yemb, (size_t)c.max_audio * dn));
  VXC(dalloc_t(e, &e->nar_logits, (size_t)c.max_audio * 1024));
  VXC(dalloc_t(e, &e->ids_text, (size_t)c.max_text));
  VXC(dalloc_t(e, &e->ids_audio, (size_t)c.max_audio + 1));
  VXC(dalloc_t(e, &e->ids_prompts, (size_t)c.max_audio * 8));
  VXC(dalloc_t(e, &e->ids_samples, (size_t)c.max_audio));
  VXC(dalloc_t(e, &e->d_codes, (size_t)c.max_audio * 8));
  VXC(dalloc_t(e, &e->d_fcodes, (size_t)c.max_audio * 8));
  e->cap_audio = c.max_audio; e->cap_text = c.max_text;
  if (e->fp8nar) {
    e->mx_ld = (e->n_max + 255) / 256 * 256;
    VXC(dalloc_t(e, &e->Hn8, n * dmax));
    VXC(dalloc_t(e, &e->FF8, n * 4 * dmax));
    VXC(dalloc_t(e, &e->SHn, (size_t)(dmax / 32) * e->mx_ld));
    VXC(dalloc_t(e, &e->SFF, (size_t)(4 * dmax / 32) * e->mx_ld));
    HIPC(hipMemsetAsync(e->SHn, 0, (size_t)(dmax / 32) * e->mx_ld, e->es));  // the pad rows' scales must stay finite
    HIPC(hipMemsetAsync(e->SFF, 0, (size_t)(4 * dmax / 32) * e->mx_ld, e->es));
  }
  if (e->bf16 && !(c.flags & VX_FLAG_SIMPLE_ROWS)) {
    e->slab_rows = e->n_max < 4095 ? e->n_max : 4095;
    VXC(dalloc_t(e, &e->slab, (size_t)4 * e->slab_rows * dmax));
  }
  if (c.flags & VX_FLAG_PRENET) {
    VXC(dalloc_t(e, &e->pn_a, n * dmax));
    VXC(dalloc_t(e, &e->pn_b, n * dmax));
    VXC(dalloc_t(e, &e->pn_h1, n * PRENET_H));
    VXC(dalloc_t(e, &e->pn_h2, n * PRENET_H));
    VXC(dalloc_t(e, &e->pn_text, (size_t)c.max_text * dmax));
    VXC(dalloc_t(e, &e->d_zero, 4));
    HIPC(hipMemsetAsync(e->d_zero, 0, 16, e->es));
    VXC(dalloc_t(e, &e->ar_e, d));
    VXC(dalloc_t(e, &e->ar_h1, PRENET_H));
    VXC(dalloc_t(e, &e->ar_h2, PRENET_H));
    for (int i = 0; i < 3; ++i) {
      VXC(dalloc_t(e, &e->convT[0][i], (size_t)5 * d * d));
      if (c.num_quantizers > 1) VXC(dalloc_t(e, &e->convT[1][i], (size_t)5 * dn * dn));
    }
  }
  if (c.max_batch > 1) {
    e->bmax = c.max_batch;
    e->btok_stride = c.max_audio + 2;
    e->bkv_slot = (size_t)c.num_layers * 2 * H * e->ctx_max * hd;
    VXC(dalloc_t(e, &e->bx, (size_t)BMAX * d));
    VXC(dalloc_t(e, &e->bq, (size_t)BMAX * d));
    VXC(dalloc_t(e, &e->bpart, (size_t)4 * BMAX * d));
    VXC(dalloc_t(e, &e->blogits, (size_t)BMAX * LOGITS_CUR));
    if (c.flags & VX_FLAG_TRACE_LOGITS)  // parity tests: every pass's logits row of every slot
      VXC(dalloc_t(e, &e->btrace, (size_t)e->bmax * (c.max_audio + 2) * AR_VOCAB));
    VXC(dalloc_t(e, &e->bh, (size_t)BMAX * d));
    VXC(dalloc_t(e, &e->batt, (size_t)BMAX * d));
    VXC(dalloc_t(e, &e->bff, (size_t)BMAX * 4 * d));
    e->kv8 = c.flags & VX_FLAG_KV_FP8;
    if (e->kv8) {
      VXC(dalloc_t(e, &e->bkv8, (size_t)e->bmax * e->bkv_slot));
      VXC(dalloc_t(e, &e->bkv8s, (size_t)e->bmax * e->bkv_slot / 16));
    } else {
      VXC(dalloc_t(e, &e->bkv, (size_t)e->bmax * e->bkv_slot));
    }
    if (e->vallf) {  // 2 L max_text d bf16 per slot; rows at and past a slot's text length are never read
      e->bmem_slot = (size_t)c.num_layers * 2 * d * c.max_text;
      VXC(dalloc_t(e, &e->bmem, (size_t)e->bmax * e->bmem_slot));
    }
    VXC(dalloc_t(e, &e->bst, (size_t)BMAX));
    VXC(dalloc_t(e, &e->btok, (size_t)BMAX * e->btok_stride));
    VXC(dalloc_t(e, &e->bsamp, (size_t)BMAX * e->btok_stride));
    VXC(dalloc_t(e, &e->bargm, (size_t)BMAX * e->btok_stride));
    HIPC(hipHostMalloc((void**)&e->h_bst, 3 * BMAX * sizeof(ArState)));
    VXC(dalloc_t(e, &e->bp_text, (size_t)BMAX * c.max_text));
    VXC(dalloc_t(e, &e->bp_audio, (size_t)BMAX * (c.max_audio + 1)));
    VXC(seg_alloc(e));
    // MFMA A operands always read 32 rows: rows of unused slots must hold finite values
    HIPC(hipMemsetAsync(e->bx, 0, (size_t)BMAX * d * 4, e->es));
    HIPC(hipMemsetAsync(e->bh, 0, (size_t)BMAX * d * 2, e->es));
    HIPC(hipMemsetAsync(e->batt, 0, (size_t)BMAX * d * 2, e->es));
    HIPC(hipMemsetAsync(e->bff, 0, (size_t)BMAX * 4 * d * 2, e->es));
    HIPC(hipMemsetAsync(e->bst, 0, (size_t)BMAX * sizeof(ArState), e->es));
  }
  if (c.num_quantizers > 1)
    VXC(dalloc_t(e, &e->ada, (size_t)(c.num_quantizers - 1) * (e->npl * c.nar_num_layers + 1) * 2 * dn));
  if (e->vallf) {  // K / V of the text memory per layer, in the decode-cache layout with max_text rows per head
    VXC(dalloc(e, &e->xkv_ar, (size_t)c.num_layers * 2 * d * c.max_text * e->esz));
    if (c.num_quantizers > 1) VXC(dalloc(e, &e->xkv_nar, (size_t)c.nar_num_layers * 2 * dn * c.max_text * e->esz));
  }
  e->vf_rows = c.flags & VX_FLAG_VALLF_ROWS;
  if (e->vf_rows) {
    if (c.num_quantizers > 1) VXC(dalloc_t(e, &e->xmem_rows, (size_t)c.nar_num_layers * 2 * dn * e->cap_text));
    VXC(dalloc_t(e, &e->d_mem_off, (size_t)BMAX));
    VXC(dalloc_t(e, &e->d_mem_klen, (size_t)BMAX));
    VXC(dalloc_t(e, &e->d_mem_trow, (size_t)BMAX));
  }
  // weights
  for (auto& k : e->keys) {
    Tensor& t = e->w[k];
    VXC(dalloc(e, &t.p, t.numel * (t.low ? 2 : 4)));
    if (e->fp8nar && is_mx_key(k)) {
      VXC(dalloc_t(e, &t.q8, t.numel));
      VXC(dalloc_t(e, &t.s8, t.numel / 32));
    }
  }
  if (c.max_batch <= 1) VXC(seg_alloc(e));  // after the weights: no small block in the arena moves for lack of a batch block
  e->lpon = c.flags & VX_FLAG_LOGPROBS;
  if (e->lpon) {  // last: every other block sits where it sits without the flag
    HIPC(logprob_load());
    VXC(dalloc_t(e, &e->d_lp, (size_t)c.max_audio + 2));
    if (c.max_batch > 1) VXC(dalloc_t(e, &e->blp, (size_t)BMAX * e->btok_stride));
    if (c.num_quantizers > 1) VXC(dalloc_t(e, &e->nar_lp, (size_t)(c.num_quantizers - 1) * e->cap_audio));
  }
  HIPC(hipStreamSynchronize(e->es));  // the fills above are done before the caller's uploads (other streams) begin
  return VX_OK;
}

extern "C" void vx_destroy(vx_engine* e) {
  if (!e) return;
  DevGuard dev_guard_(e->cfg.device);
  if (e->es) (void)hipStreamSynchronize(e->es);
  for (auto& kvp : e->bgraphs) if (kvp.second) (void)hipGraphExecDestroy(kvp.second);
  if (e->h_bst) (void)hipHostFree(e->h_bst);
  if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
  for (void* p : e->allocs) (void)hipFree(p);
  if (e->d_noise) (void)hipFree(e->d_noise);
  if (e->d_forced) (void)hipFree(e->d_forced);
  if (e->h_st) (void)hipHostFree(e->h_st);
  for (auto& ev : e->ev_t) if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : e->gemm_ev) (void)hipEventDestroy(ev);
  for (auto& ev : e->ev_poll) if (ev) (void)hipEventDestroy(ev);
  if (e->ev_in) (void)hipEventDestroy(e->ev_in);
  if (e->ev_out) (void)hipEventDestroy(e->ev_out);
  if (e->es) (void)hipStreamDestroy(e->es);
  delete e;
}

// ------------------------------------------------------------------------------ weights
extern "C" int vx_set_weight(vx_engine* e, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
  if (!e || !key || !data || !shape) return fail(VX_ERR_ARG, "null argument");
  ON_DEVICE(e->cfg.device);
  auto it = e->w.find(key);
  if (it == e->w.end()) return fail(VX_ERR_WEIGHTS, "unexpected key '%s'", key);
  Tensor& t = it->second;
  bool ok = (size_t)ndim == t.shape.size();
  for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == t.shape[i];
  if (!ok) return fail(VX_ERR_WEIGHTS, "shape mismatch for '%s'", key);
  if (!t.low) {
    HIPC(hipMemcpyAsync(t.p, data, t.numel * 4, hipMemcpyDefault, e->es));
  } else {
    float* stage = nullptr;
    HIPC(hipMalloc((void**)&stage, t.numel * 4));
    HIPC(hipMemcpyAsync(stage, data, t.numel * 4, hipMemcpyDefault, e->es));
    convert_kernel<bf16><<<1024, 256, 0, e->es>>>(stage, (bf16*)t.p, t.numel);
    if (t.q8 != nullptr) {  // (N, K) -> e4m3 bytes + (K/32, N) block scales, from the fp32 values
      const int N = (int)t.shape[0], K = (int)t.shape[1];
      mx_quant_rows_kernel<<<(N + 3) / 4, 256, 0, e->es>>>(stage, t.q8, t.s8, N, K, N);
    }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(e->es));
    HIPC(hipFree(stage));
  }
  HIPC(hipStreamSynchronize(e->es));  // `data` may be freed by the caller on return
  t.set = true;
  e->finalized = false;
  return VX_OK;
}

extern "C" int vx_set_sine_table(vx_engine* e, int32_t which, const float* data, int64_t rows, int64_t dim) {
  if (!e || !data) return fail(VX_ERR_ARG, "null argument");
  ON_DEVICE(e->cfg.device);
  const int d = which == 0 ? e->cfg.d_model : e->cfg.nar_d_model;
  if (dim != d || rows < e->pe_rows) return fail(VX_ERR_ARG, "sine table must be (>= %d, %d)", e->pe_rows, d);
  const int64_t r = rows < e->pe_rows ? rows : e->pe_rows;
  HIPC(hipMemcpyAsync(which == 0 ? e->pe_ar : e->pe_nar, data, (size_t)r * d * 4, hipMemcpyDefault, e->es));
  HIPC(hipStreamSynchronize(e->es));
  (which == 0 ? e->pe_ar_set : e->pe_nar_set) = true;
  return VX_OK;
}

template <typename T> static const T* W(vx_engine* e, const std::string& k) { return (const T*)e->w.at(k).p; }

static void fill_layers(vx_engine* e, const std::string& pre, int L, bool adaptive, std::vector<LayerW>& out, int with_cross = -1) {
  const bool cross = with_cross < 0 ? e->vallf : with_cross != 0;
  out.resize(L);
  for (int i = 0; i < L; ++i) {
    const std::string p = pre + ".layers." + std::to_string(i);
    LayerW& l = out[i];
    l.in_w = W<void>(e, p + ".self_attn.in_proj_weight"); l.in_b = W<float>(e, p + ".self_attn.in_proj_bias");
    l.out_w = W<void>(e, p + ".self_attn.out_proj.weight"); l.out_b = W<float>(e, p + ".self_attn.out_proj.bias");
    l.w1 = W<void>(e, p + ".linear1.weight"); l.b1 = W<float>(e, p + ".linear1.bias");
    l.w2 = W<void>(e, p + ".linear2.weight"); l.b2 = W<float>(e, p + ".linear2.bias");
    { const Tensor &a = e->w.at(p + ".self_attn.in_proj_weight"), &b = e->w.at(p + ".linear1.weight"), &c2 = e->w.at(p + ".linear2.weight");
      l.in_q8 = a.q8; l.in_s8 = a.s8; l.w1_q8 = b.q8; l.w1_s8 = b.s8; l.w2_q8 = c2.q8; l.w2_s8 = c2.s8; }
    const std::string s = adaptive ? ".norm" : "";
    l.n1_g = W<float>(e, p + ".norm1" + s + ".weight"); l.n1_b = W<float>(e, p + ".norm1" + s + ".bias");
    l.n2_g = W<float>(e, p + ".norm2" + s + ".weight"); l.n2_b = W<float>(e, p + ".norm2" + s + ".bias");
    if (cross) {
      l.cin_w = W<void>(e, p + ".multihead_attn.in_proj_weight"); l.cin_b = W<float>(e, p + ".multihead_attn.in_proj_bias");
      l.cout_w = W<void>(e, p + ".multihead_attn.out_proj.weight"); l.cout_b = W<float>(e, p + ".multihead_attn.out_proj.bias");
      l.n3_g = W<float>(e, p + ".norm3" + s + ".weight"); l.n3_b = W<float>(e, p + ".norm3" + s + ".bias");
    }
  }
}

// AdaLN vectors: index (stage, site) -> 2*dn floats [w | b]; site = npl*layer + {0 .. npl-1} (npl = 2 norms per encoder layer,
// 3 per VALL-F decoder layer), last = final norm
static float* ada_vec(vx_engine* e, int stage, int site) {
  const int sites = e->npl * e->cfg.nar_num_layers + 1;
  return e->ada + ((size_t)stage * sites + site) * 2 * e->cfg.nar_d_model;
}

// The norm sites of a stack, n = npl * layer + k with k indexing the layer's norms in block order ({n1, n2}; VALL-F {n1, n2, n3}),
// numbered as the AdaLN sites.  Block k of layer li (0 self-attention, [1 cross-attention,] npl - 1 feed-forward) is fronted by
// front_site(li, k): pre-norm, the block's own norm; post-norm, the closing norm of the block before it (x = norm(x + block(x)),
// transformer.py:303-308), and -1 in front of layer 0 (the embedding goes in as it is).  front_site(L, 0) closes a post-norm stack.
struct NormW { const float *g, *b; };
static int front_site(const vx_engine* e, int li, int k) { return e->npl * li + k - ((e->cfg.flags & VX_FLAG_POST_NORM) ? 1 : 0); }
static NormW norm_at(const vx_engine* e, const std::vector<LayerW>& layers, int n) {
  const LayerW& l = layers[n / e->npl];
  const int k = n % e->npl;
  return k == 0 ? NormW{l.n1_g, l.n1_b} : k == 1 ? NormW{l.n2_g, l.n2_b} : NormW{l.n3_g, l.n3_b};
}

// The scoring head (vx_score on MFMA engines): ar_predict_layer padded with zero rows to NLL_MAXV.  A derived operand like the
// sharded step's re-laid-out matrices: rebuilt by every vx_finalize_weights once it exists, so a reload is scored on its own head.
static int score_head_refresh(vx_engine* e) {
  const size_t d = e->cfg.d_model;
  HIPC(hipMemsetAsync(e->sc_head, 0, (size_t)NLL_MAXV * d * 2, e->es));
  HIPC(hipMemcpyAsync(e->sc_head, e->w.at("ar_predict_layer.weight").p, (size_t)AR_VOCAB * d * 2, hipMemcpyDeviceToDevice, e->es));
  return VX_OK;
}

extern "C" int vx_finalize_weights(vx_engine* e) {
  if (!e) return fail(VX_ERR_ARG, "null engine");
  ON_DEVICE(e->cfg.device);
  for (auto& k : e->keys)
    if (!e->w[k].set) return fail(VX_ERR_WEIGHTS, "missing key '%s' (strict load)", k.c_str());
  const vx_config& c = e->cfg;
  fill_layers(e, "ar_decoder", c.num_layers, false, e->ar_l);
  if (e->tp) {  // the sharded word order of the out-projection and linear2 (ar_tp.hpp)
    for (int li = 0; li < c.num_layers; ++li) {
      const LayerW& l = e->ar_l[li];
      const unsigned g1 = (unsigned)((size_t)TP_D * TP_D * e->esz / 16 / 256), g2 = (unsigned)((size_t)TP_D * TP_FF * e->esz / 16 / 256);
      if (e->bf16) {
        tp_repack_kernel<bf16, true><<<g1, 256, 0, e->es>>>((const bf16*)l.out_w, (uint4*)e->tp_wo[li], TP_D);
        tp_repack_kernel<bf16, false><<<g2, 256, 0, e->es>>>((const bf16*)l.w2, (uint4*)e->tp_w2[li], TP_FF);
      } else {
        tp_repack_kernel<float, true><<<g1, 256, 0, e->es>>>((const float*)l.out_w, (uint4*)e->tp_wo[li], TP_D);
        tp_repack_kernel<float, false><<<g2, 256, 0, e->es>>>((const float*)l.w2, (uint4*)e->tp_w2[li], TP_FF);
      }
    }
    // {gamma, beta, bias arriving with the partials} of every norm site: 2 li = LN1 (bias = previous linear2's; none at layer 0),
    // 2 li + 1 = LN2 (bias = the out-projection's), 2 L = the final norm (bias = the last linear2's)
    auto site = [&](int idx, const float* g, const float* b, const float* bias) -> int {
      float* dst = e->tp_gbb + (size_t)idx * 3 * TP_D;
      HIPC(hipMemcpyAsync(dst, g, TP_D * 4, hipMemcpyDeviceToDevice, e->es));
      HIPC(hipMemcpyAsync(dst + TP_D, b, TP_D * 4, hipMemcpyDeviceToDevice, e->es));
      if (bias) HIPC(hipMemcpyAsync(dst + 2 * TP_D, bias, TP_D * 4, hipMemcpyDeviceToDevice, e->es));
      return VX_OK;
    };
    for (int li = 0; li < c.num_layers; ++li) {
      const LayerW& l = e->ar_l[li];
      VXC(site(2 * li, l.n1_g, l.n1_b, li ? e->ar_l[li - 1].b2 : nullptr));
      VXC(site(2 * li + 1, l.n2_g, l.n2_b, l.out_b));
    }
    VXC(site(2 * c.num_layers, W<float>(e, "ar_decoder.norm.weight"), W<float>(e, "ar_decoder.norm.bias"), e->ar_l.back().b2));
    HIPC(hipGetLastError());
  }
  std::vector<float> t;
  if (!e->pe_ar_set) {
    host_sine_table(t, e->pe_rows, c.d_model);
    HIPC(hipMemcpy(e->pe_ar, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  }
  if (c.num_quantizers > 1) {
    if (!e->pe_nar_set) {
      host_sine_table(t, e->pe_rows, c.nar_d_model);
      HIPC(hipMemcpy(e->pe_nar, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    }
    fill_layers(e, "nar_decoder", c.nar_num_layers, true, e->nar_l);
    const int dn = c.nar_d_model, Ln = c.nar_num_layers;
    for (int s = 0; s < c.num_quantizers - 1; ++s) {
      const float* emb = W<float>(e, "nar_stage_embeddings." + std::to_string(s) + ".word_embeddings.weight");
      const int npl = e->npl;
      const int nsite = npl * Ln + ((c.flags & VX_FLAG_POST_NORM) ? 0 : 1);  // post-norm: no final AdaLN
      for (int site = 0; site < nsite; ++site) {
        std::string p = site == npl * Ln ? std::string("nar_decoder.norm")
                                         : "nar_decoder.layers." + std::to_string(site / npl) + ".norm" + std::to_string(site % npl + 1);
        project_vec_kernel<<<(2 * dn + 3) / 4, 256, 0, e->es>>>(W<float>(e, p + ".project_layer.weight"),
                                                                W<float>(e, p + ".project_layer.bias"), emb,
                                                                ada_vec(e, s, site), 2 * dn, dn);
      }
    }
    HIPC(hipGetLastError());
  }
  if (c.flags & VX_FLAG_PRENET) {
    for (int which = 0; which < (c.num_quantizers > 1 ? 2 : 1); ++which) {
      const int dd = which ? c.nar_d_model : c.d_model;
      const size_t nel = (size_t)5 * dd * dd;
      for (int i = 0; i < 3; ++i)
        conv_weight_relayout_kernel<<<(unsigned)((nel + 255) / 256), 256, 0, e->es>>>(
            W<float>(e, std::string(which ? "nar" : "ar") + "_text_prenet." + std::to_string(1 + 4 * i) + ".weight"), e->convT[which][i], dd);
    }
    HIPC(hipGetLastError());
  }
  if (e->sc_head != nullptr) VXC(score_head_refresh(e));  // weights reloaded on a handle that has scored before
  HIPC(hipStreamSynchronize(e->es));
  e->finalized = true;
  return VX_OK;
}

// ------------------------------------------------------------------------------ launch helpers
template <typename WT, int KCH, int RPW, int PRO>
static void launch_gemv_inst(const GemvArgs& a, int grid, hipStream_t s) {
  // leading arguments = what the kernel loads from first (kernarg preload, ar_kernels.hpp)
  const float* xin = PRO == PRO_ATTN ? a.part : a.x;
  const unsigned nk = ((unsigned)a.N << 16) | (unsigned)a.K;  // N, K < 65536 (checked by the caller: K <= 4096, N <= 4 d)
  if (a.kid >= 0) grid += VX_KSTAMP_EXTRA;  // probe builds: one extra workgroup that only records the time (common.hpp)
  if (a.pf != nullptr) gemv_kernel<WT, KCH, RPW, PRO, 8><<<grid, 256, 0, s>>>(a.W, xin, a.gamma, a.beta, nk, a);
  else gemv_kernel<WT, KCH, RPW, PRO, 0><<<grid, 256, 0, s>>>(a.W, xin, a.gamma, a.beta, nk, a);
}

// The instance for (N, K): KCH = 16-byte chunks per lane per row, RPW = rows per wave so that one
// wave-iteration covers N over 4*grid waves, with at most 16 weight registers-quads in flight.
struct GemvPlan { int grid, kch, rpw; };
static GemvPlan gemv_plan(int N, int K, int vec, int num_cu) {
  const int need_kch = (K + 64 * vec - 1) / (64 * vec);
  // one workgroup per CU (two measured slower, profiles/r02_notes.md).  The 1025-row head streams 2 MB: 65 workgroups of 4 waves x
  // 4 rows (one pass) finish sooner than one workgroup per CU with one or two rows per wave (A/B on one box, alternating
  // processes: 230.6 vs 236.7 us per step; 129: 234)
  GemvPlan p{N == AR_VOCAB ? 65 : num_cu, 1, 1};
  while (p.kch < need_kch) p.kch <<= 1;
  if ((N + 3) / 4 < p.grid) p.grid = (N + 3) / 4;
  const int need_rpw = (N + p.grid * 4 - 1) / (p.grid * 4);
  p.rpw = need_rpw > 3 ? 4 : need_rpw;  // 3 rows per wave for N = 3 x 4 x grid (the QKV projection): every wave busy
  while (p.rpw * p.kch > 16 && p.rpw > 1) p.rpw >>= 1;
  return p;
}
// Points `a` at the weights the NEXT GEMV of the decode step streams (GemvArgs.pf): 32 KB per workgroup at most.
static void gemv_prefetch(GemvArgs& a, const void* Wn, int Nn, int Kn, bool bf, int num_cu) {
  const GemvPlan p = gemv_plan(Nn, Kn, bf ? 8 : 4, num_cu);
  const size_t slice = (size_t)4 * p.rpw * Kn * (bf ? 2 : 4), total = (size_t)Nn * Kn * (bf ? 2 : 4);
  if (Wn == nullptr || slice > 32768 || total >= (1ull << 32) || total < 16) return;
  a.pf = Wn; a.pf_slice = (unsigned)slice; a.pf_total = (unsigned)total;
}

template <typename WT, int PRO> static int launch_gemv_p(const GemvArgs& a, int num_cu, hipStream_t s) {
  constexpr int VEC = Vec16<WT>::N;
  if (a.K % VEC || a.K > 4096 || a.K % 4) return fail(VX_ERR_UNSUPPORTED, "gemv: K=%d unsupported", a.K);
  if (a.N <= 0 || a.N > 65535) return fail(VX_ERR_UNSUPPORTED, "gemv: N=%d unsupported", a.N);  // (N << 16) | K travels as one argument
  const GemvPlan pl = gemv_plan(a.N, a.K, VEC, num_cu);
  const int kch = pl.kch, rpw = pl.rpw, grid = pl.grid;
  if (kch > 16 || (PRO != PRO_COPY && (kch > 4 || a.K > 1024))) return fail(VX_ERR_UNSUPPORTED, "gemv: K=%d too large for prologue %d", a.K, PRO);
#define GV(KC, RP) if (kch == KC && rpw == RP) { launch_gemv_inst<WT, KC, RP, PRO>(a, grid, s); return VX_OK; }
  GV(1, 1) GV(1, 2) GV(1, 3) GV(1, 4) GV(2, 1) GV(2, 2) GV(2, 3) GV(2, 4) GV(4, 1) GV(4, 2) GV(4, 3) GV(4, 4)
  if constexpr (PRO == PRO_COPY) { GV(8, 1) GV(8, 2) GV(16, 1) }
#undef GV
  return fail(VX_ERR_UNSUPPORTED, "gemv: no instance for kch=%d rpw=%d", kch, rpw);
}

template <typename WT> static int launch_gemv_t(const GemvArgs& a, int num_cu, hipStream_t s) {
  if (a.pro == PRO_LN) return launch_gemv_p<WT, PRO_LN>(a, num_cu, s);
  if (a.pro == PRO_ATTN) return launch_gemv_p<WT, PRO_ATTN>(a, num_cu, s);
  return launch_gemv_p<WT, PRO_COPY>(a, num_cu, s);
}

static int launch_gemv(bool bf, const GemvArgs& a, int num_cu, hipStream_t s) {
  return bf ? launch_gemv_t<bf16>(a, num_cu, s) : launch_gemv_t<float>(a, num_cu, s);
}

// ---- the XCD-sharded decode step (ar_tp.hpp): chosen at vx_create when the geometry is BASELINE's (d = 1024, 16 heads, pre-norm,
// no prenets, VALL-E) AND all 256 workgroups of its launches are resident at once - their hand-overs spin.  VX_AR_TP=0 keeps the
// five-launch step (A/B runs, probe builds).
static int tp_setup(vx_engine* e) {
  const vx_config& c = e->cfg;
  const int d = c.d_model, H = c.nhead;
  e->tp = false;
  const char* tv = getenv("VX_AR_TP");
  if ((tv && atoi(tv) == 0) || e->vallf || d != TP_D || H != TP_H || (c.flags & (VX_FLAG_POST_NORM | VX_FLAG_PRENET))) return VX_OK;
  int n1 = 0, n2 = 0;
  if (e->bf16) {
    HIPC(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n1, (const void*)tp_attn_kernel<bf16, true>, 256, 0));
    HIPC(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n2, (const void*)tp_ffn_kernel<bf16>, 256, 0));
  } else {
    HIPC(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n1, (const void*)tp_attn_kernel<float, true>, 256, 0));
    HIPC(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n2, (const void*)tp_ffn_kernel<float>, 256, 0));
  }
  if ((long long)(n1 < n2 ? n1 : n2) * e->num_cu < TP_X * TP_WG) return VX_OK;
  const size_t L = (size_t)c.num_layers;
  VXC(dalloc_t(e, &e->tp_xacc, (size_t)3 * TP_D));
  VXC(dalloc_t(e, &e->tp_gh, L * TP_X * TP_HID));
  VXC(dalloc_t(e, &e->tp_gbb, (2 * L + 1) * 3 * TP_D));
  VXC(dalloc_t(e, &e->fq_gq, L * H * FQ_QKV));
  VXC(dalloc_t(e, &e->fq_gp, L * H * FQ_S * FQ_PART));
  HIPC(hipMemset(e->tp_gbb, 0, (2 * L + 1) * 3 * TP_D * 4));
  HIPC(hipMemset(e->tp_xacc, 0, (size_t)3 * TP_D * sizeof(long long)));
  HIPC(hipMemset(e->tp_gh, 0, L * TP_X * TP_HID * sizeof(fq_gran)));  // zero tags: never equal to a step counter (starts at 1)
  HIPC(hipMemset(e->fq_gq, 0, L * H * FQ_QKV * sizeof(fq_gran)));
  HIPC(hipMemset(e->fq_gp, 0, L * H * FQ_S * FQ_PART * sizeof(fq_gran)));
  e->tp_wo.assign(L, nullptr); e->tp_w2.assign(L, nullptr);
  for (size_t li = 0; li < L; ++li) {
    VXC(dalloc(e, &e->tp_wo[li], (size_t)TP_D * TP_D * e->esz));
    VXC(dalloc(e, &e->tp_w2[li], (size_t)TP_D * TP_FF * e->esz));
  }
  e->tp = true;
  return VX_OK;
}

template <typename T>
static int gemm_rows_t(bool mfma, const T* A, const T* Wt, const float* bias, void* C, int M, int N, int K, int epi,
                       bool out_f32, hipStream_t s, void* vt = nullptr, int vt_n0 = 0, int vt_ld = 0) {
  if constexpr (std::is_same<T, bf16>::value) {
    if (mfma) return mfma_gemm_dispatch(A, Wt, bias, C, M, N, K, epi, out_f32, s, (bf16*)vt, vt_n0, vt_ld);
  }
  gemm_simple_launch(A, Wt, bias, C, M, N, K, epi, out_f32, s);
  return VX_OK;
}

static bool use_mfma(const vx_engine* e) { return e->bf16 && e->hd64 && !(e->cfg.flags & VX_FLAG_SIMPLE_ROWS); }

static int gemm_rows(vx_engine* e, const void* A, const void* Wt, const float* bias, void* C, int M, int N, int K,
                     int epi, bool out_f32, bool emit_vt = false) {
  if (e->bf16)
    return gemm_rows_t<bf16>(use_mfma(e), (const bf16*)A, (const bf16*)Wt, bias, C, M, N, K, epi, out_f32, e->es,
                             emit_vt ? e->VT : nullptr, 2 * (N / 3), e->vt_ld);
  return gemm_rows_t<float>(false, (const float*)A, (const float*)Wt, bias, C, M, N, K, epi, out_f32, e->es);
}

// fold: the split-K slabs (and bias) of the GEMM in front of this norm, added to x first (rows_kernels.hpp)
struct Fold { const float* part = nullptr; int nsplit = 0; size_t stride = 0; const float* bias = nullptr; };
// the launch itself, on any stream (ln_rows below; vx_op_ln_fold on caller buffers)
static void ln_rows_launch(bool out_bf16, const float* x, const float* g, const float* b, const float* aw, const float* ab, void* out,
                           int rows, int d, float* xout, const Fold& f, hipStream_t s) {
  // d <= 1024 in the engine (vx_create): 4 float4 per lane
  if (out_bf16) layernorm_rows_kernel<bf16, 4><<<(rows + 3) / 4, 256, 0, s>>>(x, g, b, aw, ab, (bf16*)out, rows, d, xout, f.part, f.nsplit, f.stride, f.bias);
  else layernorm_rows_kernel<float, 4><<<(rows + 3) / 4, 256, 0, s>>>(x, g, b, aw, ab, (float*)out, rows, d, xout, f.part, f.nsplit, f.stride, f.bias);
}
static int ln_rows(vx_engine* e, const float* x, const float* g, const float* b, const float* aw, const float* ab,
                   void* out, int rows, int d, float* xout = nullptr, Fold f = Fold()) {
  ln_rows_launch(e->bf16, x, g, b, aw, ab, out, rows, d, xout, f, e->es);
  return VX_OK;
}
// fp32 linear layer on rows (prenets keep fp32 weights in every precision mode): C = [relu](A W^T + b)
static int linear_rows_f32(vx_engine* e, const float* A, const float* Wt, const float* bias, float* Cm, int M, int N, int K, bool relu) {
  return gemm_rows_t<float>(false, A, Wt, bias, Cm, M, N, K, relu ? GE_RELU : GE_BIAS, true, e->es);
}
// text prenet (valle.py:97-113): `in` (S, dd) raw embeddings -> `out` (S, dd); uses pn_a / pn_b as scratch (in/out may be them)
static int text_prenet_rows(vx_engine* e, int which, const float* in, float* out, int S, int dd) {
  const std::string pre = std::string(which ? "nar" : "ar") + "_text_prenet.";
  const float* src = in;
  float* bufs[2] = {e->pn_b, e->pn_a};
  for (int i = 0; i < 3; ++i) {
    const std::string cv = pre + std::to_string(1 + 4 * i), bn = pre + std::to_string(2 + 4 * i);
    float* dst = bufs[i & 1];
    conv5_bn_relu_kernel<<<(S + CONV_TT - 1) / CONV_TT, 256, (size_t)(CONV_TT + 4) * dd * 4, e->es>>>(
        src, e->convT[which][i], W<float>(e, cv + ".bias"), W<float>(e, bn + ".weight"), W<float>(e, bn + ".bias"),
        W<float>(e, bn + ".running_mean"), W<float>(e, bn + ".running_var"), dst, S, dd);
    src = dst;
  }
  // src == pn_b after three convolutions
  return linear_rows_f32(e, src, W<float>(e, pre + "14.weight"), W<float>(e, pre + "14.bias"), out, S, dd, dd, false);
}
// audio prenet (valle.py:115-123): `in` (rows, dd) -> `out` (rows, dd), hidden rows in pn_h1 / pn_h2
static int audio_prenet_rows(vx_engine* e, int which, const float* in, float* out, int rows, int dd) {
  const std::string pre = std::string(which ? "nar" : "ar") + "_audio_prenet.";
  VXC(linear_rows_f32(e, in, W<float>(e, pre + "0.weight"), W<float>(e, pre + "0.bias"), e->pn_h1, rows, PRENET_H, dd, true));
  VXC(linear_rows_f32(e, e->pn_h1, W<float>(e, pre + "3.weight"), W<float>(e, pre + "3.bias"), e->pn_h2, rows, PRENET_H, PRENET_H, true));
  return linear_rows_f32(e, e->pn_h2, W<float>(e, pre + "6.weight"), W<float>(e, pre + "6.bias"), out, rows, dd, PRENET_H, false);
}

// rows of the fp32 residual stream -> the GEMM operand type, no normalisation (input of a post-norm stack)
static int cast_rows(vx_engine* e, const float* x, void* out, size_t n) {
  if (e->bf16) convert_kernel<bf16><<<1024, 256, 0, e->es>>>(x, (bf16*)out, n);
  else convert_kernel<float><<<1024, 256, 0, e->es>>>(x, (float*)out, n);
  return VX_OK;
}

// How the rows of e->X are laid out: n == 0, one plain sequence; otherwise n concatenated utterances (seg_layout), segment z
// at rows [start[z], start[z] + len[z]) of the buffer (device arrays), with its own prefix mask (text, optional: text_len
// applies to all) and its own KV slot (slot, optional).
struct RowSegs {
  int n = 0, max_len = 0;
  const int *start = nullptr, *len = nullptr, *text = nullptr, *slot = nullptr;
};

static int attn_rows(vx_engine* e, const void* qkv, void* out, int M, int d, int H, int text_len, const RowSegs& segs) {
  const int hd = d / H;
  const float scale = 1.0f / sqrtf((float)hd);
  if (segs.n > 0 || use_mfma(e)) {  // segments: one launch over all of them
    const int rc = mfma_attn_dispatch((const bf16*)qkv, (const bf16*)e->VT, e->vt_ld, (bf16*)out, M, d, H, text_len, e->es,
                                      segs.start, segs.len, segs.n, segs.max_len, segs.text);
    return rc == 0 ? VX_OK : fail(VX_ERR_UNSUPPORTED, "attention: a sequence's q/k/v rows or the V^T buffer exceed 4 GB (rows %d, d %d)", M, d);
  }
  dim3 grid((M + 63) / 64, H);
#define AR(HDV)                                                                                                                   \
  if (hd == HDV) {                                                                                                                \
    if (e->bf16) attn_rows_simple_kernel<bf16, HDV><<<grid, 256, 0, e->es>>>((const bf16*)qkv, (bf16*)out, M, d, text_len, scale); \
    else attn_rows_simple_kernel<float, HDV><<<grid, 256, 0, e->es>>>((const float*)qkv, (float*)out, M, d, text_len, scale);      \
    return VX_OK;                                                                                                                 \
  }
  AR(64) AR(32) AR(16) AR(8) AR(4)
#undef AR
  return fail(VX_ERR_UNSUPPORTED, "attention: head_dim %d", hd);
}

// ---- VALL-F (valle.py:49-719): the text memory of the TransformerDecoderLayers (modules/transformer.py:409-601) ------------
// Text memory -> per-layer K / V in the decode-cache layout (nhead, max_text, hd).  `mem` = S rows of the embedded text in
// operand precision (e->Hn).  The packed cross in_proj is applied whole (the q third of the result is unused): every output
// element is its own dot product, so rows [d, 3d) equal linear(mem, w[d:], b[d:]) of torch's _in_projection_packed.
static int memory_kv(vx_engine* e, const std::vector<LayerW>& layers, void* xkv, int S, int d, int H) {
  const int hd = d / H;
  const size_t per_layer = (size_t)2 * d * e->cfg.max_text * e->esz;
  for (size_t li = 0; li < layers.size(); ++li) {
    VXC(gemm_rows(e, e->Hn, layers[li].cin_w, layers[li].cin_b, e->QKV, S, 3 * d, d, GE_BIAS, false, false));
    char* kc = (char*)xkv + li * per_layer;
    char* vc = kc + per_layer / 2;
    if (e->bf16) kv_scatter_kernel<bf16><<<S, 256, 0, e->es>>>((const bf16*)e->QKV, (bf16*)kc, (bf16*)vc, S, d, hd, e->cfg.max_text);
    else kv_scatter_kernel<float><<<S, 256, 0, e->es>>>((const float*)e->QKV, (float*)kc, (float*)vc, S, d, hd, e->cfg.max_text);
  }
  HIPC(hipGetLastError());
  return VX_OK;
}

static int cross_attn_rows(vx_engine* e, const void* q, const void* kc, const void* vc, void* out, int M, int d, int H, int Sk) {
  const int hd = d / H;
  const float scale = 1.0f / sqrtf((float)hd);
  dim3 grid((M + 63) / 64, H);
#define CA(HDV)                                                                                                                  \
  if (hd == HDV) {                                                                                                               \
    if (e->bf16) cross_attn_rows_kernel<bf16, HDV><<<grid, 256, 0, e->es>>>((const bf16*)q, d, (const bf16*)kc, (const bf16*)vc, \
                                                                            e->cfg.max_text, (bf16*)out, d, M, Sk, scale);       \
    else cross_attn_rows_kernel<float, HDV><<<grid, 256, 0, e->es>>>((const float*)q, d, (const float*)kc, (const float*)vc,     \
                                                                     e->cfg.max_text, (float*)out, d, M, Sk, scale);             \
    return VX_OK;                                                                                                                \
  }
  CA(64) CA(32) CA(16) CA(8) CA(4)
#undef CA
  return fail(VX_ERR_UNSUPPORTED, "cross-attention: head_dim %d", hd);
}

static int split_for(int K) {  // K slices of the split-K GEMMs: a multiple of the 64-wide K tile each
  for (int sp = 4; sp > 1; sp >>= 1)
    if (K % (64 * sp) == 0) return sp;
  return 1;
}

// The split-K plan of a row stack over M rows of width d.  splitk: the two N = d GEMMs of a layer (out-projection, FFN2) may
// write fp32 slabs that the next LayerNorm folds (`eligible`: what the engine and the call decide - bf16 MFMA rows, no text
// memory, no MXFP8, M within the slab buffer); sp_d / sp_ff: their K slices (1 = no slabs, residual add in the GEMM epilogue):
// the largest of 4 / 2 / 1 that keeps (128^2 tiles) x slices within one round of the chip's CUs - at 1025 rows 72 tiles x 4
// slices were 288 workgroups, i.e. two rounds, and four slabs for the next LayerNorm to fold (A/B on one box: NAR 7 stages
// 9.38 ms with 4 / 4 slices, 8.97 ms with 2 / 2; the 272-row prefill is fastest with 4 / 4: 0.91 vs 0.99 ms)
struct RowsPlan { bool splitk; int sp_d, sp_ff; };
static RowsPlan rows_plan(bool eligible, int M, int d, int num_cu) {
  auto fit = [&](int K) {
    const long long tiles = (long long)((M + 127) / 128) * (d / 128);
    for (int sp = split_for(K); sp > 1; sp >>= 1)
      if (tiles * sp <= num_cu) return sp;
    return 1;
  };
  return RowsPlan{eligible && M < 4096 && d % 128 == 0 && d >= 128, fit(d), fit(4 * d)};
}

static bool use_mfma(const vx_engine* e);
static bool time_gemms() {
  const char* v = getenv("VX_TIME_GEMMS");  // read per call: bench.py turns it on for ONE extra, untimed pass
  const bool on = v && atoi(v) != 0;
  return on;
}
// event before / after a GEMM launch on the engine stream (no-op unless VX_TIME_GEMMS=1)
static void gemm_mark(vx_engine* e, double flops) {
  if (!time_gemms()) return;
  if (e->gemm_ev_used == e->gemm_ev.size()) { hipEvent_t ev; if (hipEventCreate(&ev) != hipSuccess) return; e->gemm_ev.push_back(ev); }
  (void)hipEventRecord(e->gemm_ev[e->gemm_ev_used++], e->es);
  e->gemm_flops += flops;  // counted at the closing mark (flops > 0)
}
// after the stream has been synchronised: sum the pairs' elapsed times
static void gemm_collect(vx_engine* e) {
  e->t_gemm = 0;
  for (size_t i = 0; i + 1 < e->gemm_ev_used; i += 2) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e->gemm_ev[i], e->gemm_ev[i + 1]) == hipSuccess) e->t_gemm += ms;
  }
  e->gemm_flops_done = e->gemm_flops;
  e->gemm_ev_used = 0; e->gemm_flops = 0;
}
// VX_PREC_FP8_NAR: do this stage's QKV / FFN GEMMs run on MXFP8?  (NAR stages only, pre-norm, at or above the row threshold;
// VX_MX_MIN_ROWS lowers it: the parity tests run one utterance's 1025 rows through the MXFP8 kernels)
static bool mx_on(const vx_engine* e, int ada_stage, int M, int d) {
  const char* v = getenv("VX_MX_MIN_ROWS");
  return e->fp8nar && ada_stage >= 0 && M >= (v ? atoi(v) : 4096) && !(e->cfg.flags & VX_FLAG_POST_NORM) && use_mfma(e) && d % 256 == 0;
}

// Where run_stack also writes every layer's K / V rows: nowhere (NAR stages), a bf16 / fp32 cache in the layout of e->kv at
// `base`, the fp8 cache of slot `slot`, or each segment's rows to the slot cache its entry of RowSegs::slot names.
struct KvDst {
  enum Kind { NONE, CACHE, FP8_SLOT, SEG_SLOTS } kind = NONE;
  char* base = nullptr;  // CACHE
  int slot = 0;          // FP8_SLOT
};
// The text memory a VALL-F stack cross-attends to: layer li's K / V at kv + li * 2 d max_text elements (memory_kv's layout), `rows`
// text rows.  kv == nullptr: none (VALL-E).
// Segmented rows (VX_FLAG_VALLF_ROWS): every segment has its own memory in cross_attn_seg_kernel's addressing - layer li at kv +
// li * layer_stride elements, segment z's K there at off[z] + head * head_stride + key * 64, V at + v_offset, klen[z] keys (off /
// klen: device arrays) - and `rows` is unused.
struct TextMem {
  const void* kv = nullptr; int rows = 0;
  const long long* off = nullptr; const int* klen = nullptr;
  long long layer_stride = 0, head_stride = 0, v_offset = 0;
};
// The attention tap of run_stack (vx_align): `rows` rows of the pass from row `row` of e->X on, row i being audio position
// row0 + i, accumulate the head-weighted attention they pay to the text columns [c0, c1) of `text_len` text tokens
// (attn_text_rows_kernel, align.hpp).  w: the (L, H) weights on the device, hw: the same on the host - a layer whose weights are
// all zero is not launched unless per_head, (L, H, rows, c1 - c0), is wanted.  On a segmented AR pass (vx_align_batch) the rows,
// windows and output offsets are per segment: segs, nseg descriptors on the device (align.hpp), max_rows the largest T_z, attn /
// mass the packed outputs of `cells` cells / `rows_total` rows, scr the per-head scratch; no per_head there.
struct AttnTap {
  const float *w = nullptr, *hw = nullptr;
  int row = 0, rows = 0, row0 = 0, text_len = 0, c0 = 0, c1 = 0;
  float *attn = nullptr, *mass = nullptr, *per_head = nullptr;
  const AlignSeg* segs = nullptr;
  int nseg = 0, max_rows = 0;
  long long cells = 0, rows_total = 0;
  float* scr = nullptr;
};
static int tap_layer(vx_engine* e, const AttnTap& t, int li, int H, int hd, const void* q, long long ldq, const void* k, long long ldk,
                     long long k_head_stride, int causal, bool& first) {
  bool any = t.per_head != nullptr;
  for (int h = 0; h < H && !any; ++h) any = t.hw[li * H + h] != 0.f;
  if (!any) return VX_OK;
  float* ph = t.per_head ? t.per_head + (size_t)li * H * t.rows * (t.c1 - t.c0) : nullptr;
  if (launch_attn_text_rows(e->bf16, q, ldq, k, ldk, k_head_stride, t.rows, t.row0, H, hd, t.text_len, causal, t.c0, t.c1, t.w + li * H,
                            t.attn, t.mass, ph, first ? 1 : 0, e->es))
    return fail(VX_ERR_UNSUPPORTED, "attention tap: head_dim %d", hd);
  first = false;
  return VX_OK;
}
// The tap of one layer of a segmented pass: attn_text_seg_kernel over every segment, then the heads in head order.
static int tap_layer_segs(vx_engine* e, const AttnTap& t, int li, int H, int d, bool& first) {
  bool any = false;
  for (int h = 0; h < H && !any; ++h) any = t.hw[li * H + h] != 0.f;
  if (!any) return VX_OK;
  launch_attn_text_segs(e->QKV, (const char*)e->QKV + d * e->esz, 3 * d, t.segs, t.nseg, t.max_rows, H, t.w + li * H, t.scr, t.cells,
                        t.rows_total, t.attn, t.mass, first ? 1 : 0, e->es);
  first = false;
  return VX_OK;
}
// The text memories of n segments at once: `trows` concatenated text rows (segment z = rows [trow[z], trow[z] + S[z]), no padding)
// in operand precision in e->Hn -> one in_proj GEMM per layer over all of them (the packed cross in_proj whole, N = 3 d, as
// memory_kv) and one scatter launch into every segment's memory (`mem`, written through the same descriptors run_stack reads).
// Uploads the descriptors; the host arrays must outlive the pass.
static int memory_kv_segs(vx_engine* e, const std::vector<LayerW>& layers, const TextMem& mem, int n, const long long* off,
                          const int* S, const int* trow, int trows, int d) {
  int max_s = 0;
  for (int z = 0; z < n; ++z) max_s = std::max(max_s, S[z]);
  HIPC(hipMemcpyAsync(e->d_mem_off, off, n * sizeof(long long), hipMemcpyHostToDevice, e->es));
  HIPC(hipMemcpyAsync(e->d_mem_klen, S, n * sizeof(int), hipMemcpyHostToDevice, e->es));
  HIPC(hipMemcpyAsync(e->d_mem_trow, trow, n * sizeof(int), hipMemcpyHostToDevice, e->es));
  for (size_t li = 0; li < layers.size(); ++li) {
    VXC(gemm_rows(e, e->Hn, layers[li].cin_w, layers[li].cin_b, e->QKV, trows, 3 * d, d, GE_BIAS, false, false));
    mem_scatter_seg_kernel<<<dim3(max_s, n), 256, 0, e->es>>>((const bf16*)e->QKV, (bf16*)mem.kv + li * mem.layer_stride, e->d_mem_off,
                                                              mem.head_stride, mem.v_offset, e->d_mem_trow, e->d_mem_klen, d);
  }
  HIPC(hipGetLastError());
  return VX_OK;
}

// One stack over M rows held in e->X: encoder layers (valle.py:1035-1038 / 1125-1127) or, with a text memory, VALL-F decoder
// layers (valle.py:626-632 / 682-688, transformer.py:536-558), whose cross-attention block sits between the self-attention and
// the feed-forward block.  `ada_stage` < 0: plain LayerNorm (AR); otherwise the stage's AdaLN vectors.  `segs`: the row layout;
// `kv`: where the K/V rows also go (KvDst).
static int run_stack(vx_engine* e, const std::vector<LayerW>& layers, int M, int d, int H, int text_len, int ada_stage,
                     const RowSegs& segs, KvDst kv, TextMem mem = TextMem(), const AttnTap* tap = nullptr) {
  const bool post = e->cfg.flags & VX_FLAG_POST_NORM, cross = mem.kv != nullptr;
  if (cross && segs.n > 0 && mem.off == nullptr) return fail(VX_ERR_UNSUPPORTED, "cross-attention over segmented rows");
  if (tap && ada_stage >= 0) return fail(VX_ERR_UNSUPPORTED, "attention tap on a NAR pass");
  if (tap && segs.n > 0 && (cross || tap->segs == nullptr || !use_mfma(e)))
    return fail(VX_ERR_UNSUPPORTED, "attention tap on a segmented pass: bf16 self-attention rows of head_dim 64 with per-segment descriptors only");
  bool tap_first = true;  // the first tapped layer stores, the others add
  const int hd = d / H;
  const size_t kv_layer = (size_t)2 * H * e->ctx_max * hd * e->esz;
  const size_t mem_layer = (size_t)2 * d * e->cfg.max_text * e->esz;
  // The two N = d GEMMs of a layer (out-projection, FFN2) at M ~ 1k rows: 128^2 tiles alone are 72 workgroups, so K is
  // split over 2-4 workgroups per tile, every slice writes an fp32 slab, and the LayerNorm that follows the GEMM anyway
  // adds bias + slabs to x in a fixed order.  Larger M (batched rows) has enough tiles and adds in the GEMM epilogue.
  // Not with a text memory: the VALL-F stack is a parity path, and slabs would change its bf16 summation order.
  const RowsPlan plan = rows_plan(!cross && use_mfma(e) && M <= e->slab_rows && !mx_on(e, ada_stage, M, d), M, d, e->num_cu);
  const bool splitk = plan.splitk;
  const bool mx = mx_on(e, ada_stage, M, d);
  const bool tg = time_gemms() && ada_stage >= 0;  // NAR stages only (the cross-attention block is not timed)
  const size_t sstride = (size_t)M * d;
  const int sp_d = plan.sp_d, sp_ff = plan.sp_ff;  // K slices of the out-projection / FFN2 (rows_plan)
  Fold pend;  // split-K slabs of the GEMM that closed the previous block, folded by the next norm (or the trailing fold pass)
  // The norm in front of block k of layer li (front_site) into Hn, folding `pend`; post-norm also writes x = norm(x).  Post-norm
  // layer 0 casts x as it is.  MXFP8 (pre-norm, no slabs): the LayerNorm quantises its own row into Hn8 / SHn.
  auto norm_in = [&](int li, int k) -> int {
    const int n = front_site(e, li, k);
    if (n < 0) return cast_rows(e, e->X, e->Hn, (size_t)M * d);
    const NormW nw = norm_at(e, layers, n);
    const float* aw = ada_stage >= 0 ? ada_vec(e, ada_stage, n) : nullptr;
    const float* ab = aw ? aw + d : nullptr;
    if (mx) {
      layernorm_rows_mx_kernel<4><<<(M + 3) / 4, 256, 0, e->es>>>(e->X, nw.g, nw.b, aw, ab, e->Hn8, e->SHn, M, d, e->mx_ld);
      return VX_OK;
    }
    const Fold f = pend;
    pend = Fold();
    return ln_rows(e, e->X, nw.g, nw.b, aw, ab, e->Hn, M, d, post ? e->X : nullptr, f);
  };
  for (int li = 0; li < (int)layers.size(); ++li) {
    const LayerW& l = layers[li];
    // self-attention: pre-norm x += sa(norm(x)) (transformer.py:296-302); post-norm x = norm(x + sa(x)) (303-308)
    VXC(norm_in(li, 0));
    if (tg) gemm_mark(e, 0);
    if (mx) {  // MXFP8 QKV: the GEMM writes bf16 q/k/v (+ V^T) for the bf16 attention
      if (mx_gemm_dispatch(e->Hn8, e->SHn, e->mx_ld, l.in_q8, l.in_s8, 3 * d, l.in_b, e->QKV, nullptr, 0, M, 3 * d, d, GE_BIAS,
                           MX_OUT_BF16, e->es, (bf16*)e->VT, 2 * d, e->vt_ld))
        return fail(VX_ERR_UNSUPPORTED, "mx gemm: shape %d x %d x %d", M, 3 * d, d);
    } else {
      VXC(gemm_rows(e, e->Hn, l.in_w, l.in_b, e->QKV, M, 3 * d, d, GE_BIAS, false, use_mfma(e)));
    }
    if (tg) gemm_mark(e, 2.0 * M * 3 * d * d);
    if (tap && segs.n > 0)  // ... of every segment's tapped rows, on the matrix pipe
      VXC(tap_layer_segs(e, *tap, li, H, d, tap_first));
    else if (tap && !cross)  // VALL-E: the text columns of the self-attention of the tapped rows, from the packed q / k rows
      VXC(tap_layer(e, *tap, li, H, hd, (const char*)e->QKV + (size_t)tap->row * 3 * d * e->esz, 3 * d, (const char*)e->QKV + d * e->esz,
                    3 * d, hd, 1, tap_first));
    const size_t kvl = (size_t)2 * H * e->ctx_max * 64;  // elements per layer of a slot cache
    if (kv.kind == KvDst::SEG_SLOTS) {  // batched prefill: segment z -> slot segs.slot[z]
      if (e->kv8)
        kv8_scatter_kernel<<<dim3(segs.max_len, segs.n), 256, 0, e->es>>>((const bf16*)e->QKV, e->bkv8 + li * kvl, e->bkv8s + li * kvl / 16,
                                                                           e->bkv_slot, kvl / 2, segs.start, segs.len, segs.slot, d, e->ctx_max);
      else
        kv_scatter_seg_kernel<bf16><<<dim3(segs.max_len, segs.n), 256, 0, e->es>>>(
            (const bf16*)e->QKV, e->bkv + li * kvl, e->bkv_slot, kvl / 2, segs.start, segs.len, d, 64, e->ctx_max, segs.slot);
    } else if (kv.kind == KvDst::FP8_SLOT) {  // per-slot prefill into an fp8 slot cache
      const size_t at = (size_t)kv.slot * e->bkv_slot + li * kvl;
      kv8_scatter_kernel<<<M, 256, 0, e->es>>>((const bf16*)e->QKV, e->bkv8 + at, e->bkv8s + at / 16, 0, kvl / 2, nullptr, nullptr, nullptr,
                                               d, e->ctx_max);
    } else if (kv.kind == KvDst::CACHE) {
      char* kc = kv.base + li * kv_layer;
      char* vc = kc + kv_layer / 2;
      if (e->bf16) kv_scatter_kernel<bf16><<<M, 256, 0, e->es>>>((const bf16*)e->QKV, (bf16*)kc, (bf16*)vc, M, d, hd, e->ctx_max);
      else kv_scatter_kernel<float><<<M, 256, 0, e->es>>>((const float*)e->QKV, (float*)kc, (float*)vc, M, d, hd, e->ctx_max);
    }
    VXC(attn_rows(e, e->QKV, e->ATT, M, d, H, text_len, segs));
    // out-projection: x += out_proj(attn), folded into the norm that follows when split
    if (tg && !mx) gemm_mark(e, 0);  // (MXFP8 stages: only the fp8 GEMMs are timed; the out-projection stays bf16)
    if (splitk && sp_d > 1) {
      VXC(mfma_gemm_partial((const bf16*)e->ATT, (const bf16*)l.out_w, e->slab, M, d, d, sp_d, e->es));
      pend.part = e->slab; pend.nsplit = sp_d; pend.stride = sstride; pend.bias = l.out_b;
    } else {
      VXC(gemm_rows(e, e->ATT, l.out_w, l.out_b, e->X, M, d, d, GE_RESID, true));
    }
    if (tg && !mx) gemm_mark(e, 2.0 * M * d * d);
    if (cross) {  // cross-attention over the text: x += mha(norm(x), memory) (transformer.py:540-545, 551-557)
      VXC(norm_in(li, 1));
      VXC(gemm_rows(e, e->Hn, l.cin_w, l.cin_b, e->QKV, M, d, d, GE_BIAS, false, false));  // q = rows [0, d) of the packed in_proj
      const char* xk = (const char*)mem.kv + li * mem_layer;
      if (tap)  // VALL-F: the cross-attention of the tapped rows over this layer's memory K
        VXC(tap_layer(e, *tap, li, H, hd, (const char*)e->QKV + (size_t)tap->row * d * e->esz, d, xk, hd, (long long)e->cfg.max_text * hd, 0,
                      tap_first));
      if (segs.n > 0)  // every segment over its own memory (VX_FLAG_VALLF_ROWS)
        cross_attn_seg_launch((const bf16*)e->QKV, d, (const bf16*)mem.kv + li * mem.layer_stride, mem.off, mem.head_stride, mem.v_offset,
                              mem.klen, (bf16*)e->ATT, d, H, segs.start, segs.len, segs.n, segs.max_len, e->es);
      else VXC(cross_attn_rows(e, e->QKV, xk, xk + mem_layer / 2, e->ATT, M, d, H, mem.rows));
      VXC(gemm_rows(e, e->ATT, l.cout_w, l.cout_b, e->X, M, d, d, GE_RESID, true));
    }
    // feed-forward: x += ff(norm(x)); post-norm x = norm(x + ff(x))
    VXC(norm_in(li, e->npl - 1));
    if (tg) gemm_mark(e, 0);
    if (mx) {  // MXFP8 FFN: FFN1's epilogue quantises its ReLU output per 32-wide block, FFN2 adds into x
      if (mx_gemm_dispatch(e->Hn8, e->SHn, e->mx_ld, l.w1_q8, l.w1_s8, 4 * d, l.b1, e->FF8, e->SFF, e->mx_ld, M, 4 * d, d, GE_RELU,
                           MX_OUT_MX, e->es) ||
          mx_gemm_dispatch(e->FF8, e->SFF, e->mx_ld, l.w2_q8, l.w2_s8, d, l.b2, e->X, nullptr, 0, M, d, 4 * d, GE_RESID, MX_OUT_F32, e->es))
        return fail(VX_ERR_UNSUPPORTED, "mx gemm: FFN shapes at M=%d d=%d", M, d);
    } else {
      VXC(gemm_rows(e, e->Hn, l.w1, l.b1, e->FF, M, 4 * d, d, GE_RELU, false));
      if (splitk && sp_ff > 1) {
        VXC(mfma_gemm_partial((const bf16*)e->FF, (const bf16*)l.w2, e->slab, M, d, 4 * d, sp_ff, e->es));
        pend.part = e->slab; pend.nsplit = sp_ff; pend.stride = sstride; pend.bias = l.b2;
      } else {
        VXC(gemm_rows(e, e->FF, l.w2, l.b2, e->X, M, d, 4 * d, GE_RESID, true));
      }
    }
    if (tg) gemm_mark(e, 2.0 * 2.0 * M * 4 * d * d);
  }
  if (post) VXC(norm_in((int)layers.size(), 0));  // the last block's closing norm
  else if (pend.part != nullptr)  // the last layer's FFN2 slabs: x += b2 + slabs (no norm: the caller applies the final one)
    VXC(ln_rows(e, e->X, nullptr, nullptr, nullptr, nullptr, nullptr, M, d, nullptr, pend));
  HIPC(hipGetLastError());
  return VX_OK;
}

static int sync_in(vx_engine* e, void* stream) {
  hipStream_t cs = (hipStream_t)stream;
  if (cs == e->es) return VX_OK;
  HIPC(hipEventRecord(e->ev_in, cs));
  HIPC(hipStreamWaitEvent(e->es, e->ev_in, 0));
  return VX_OK;
}
static int sync_out(vx_engine* e, void* stream) {
  hipStream_t cs = (hipStream_t)stream;
  if (cs == e->es) return VX_OK;
  HIPC(hipEventRecord(e->ev_out, e->es));
  HIPC(hipStreamWaitEvent(cs, e->ev_out, 0));
  return VX_OK;
}

// ------------------------------------------------------------------------------ AR
// prefilled: x is a row of the prefill stack's output.  Pre-norm: the final LayerNorm is fused here (valle.py:1035-1039).
// Post-norm: there is no final norm; a prefill row is already norm2'd, the decode step's x still needs the last
// layer's norm2 (fused here instead).
static int enqueue_head(vx_engine* e, hipStream_t s, const float* x = nullptr, float* logits = nullptr,
                        const ArState* st = nullptr, bool prefilled = false, const void* pfW = nullptr, int pfN = 0, int pfK = 0) {
  const vx_config& c = e->cfg;
  const bool post = c.flags & VX_FLAG_POST_NORM;
  GemvArgs a{};
  a.W = W<void>(e, "ar_predict_layer.weight");
  a.bias = nullptr;
  a.x = x ? x : e->ar_x;
  // post-norm: the stack's closing norm (norm2 of an encoder layer, norm3 of a VALL-F decoder layer)
  const NormW fin = post ? norm_at(e, e->ar_l, front_site(e, c.num_layers, 0))
                         : NormW{W<float>(e, "ar_decoder.norm.weight"), W<float>(e, "ar_decoder.norm.bias")};
  a.gamma = fin.g; a.beta = fin.b;
  a.y = logits ? logits : e->ar_logits;
  a.N = AR_VOCAB; a.K = c.d_model;
  a.pro = (post && prefilled) ? PRO_COPY : PRO_LN; a.epi = EPI_LOGITS;
  a.st = st ? st : e->d_st;
  a.kid = (!prefilled && st == nullptr) ? 61 : -1;  // the decode step's head (probe builds)
  if (pfW) gemv_prefetch(a, pfW, pfN, pfK, e->bf16, e->num_cu);  // decode step: the next token's first GEMVs
  return launch_gemv(e->bf16, a, e->num_cu, s);
}

// The checks of one utterance to prefill (no HIP call); idx >= 0 names it in a batch.
static int check_utterance(vx_engine* e, const int64_t* text, int32_t S, const int64_t* prompt_cb0, int32_t P, int idx) {
  if (!text || (!prompt_cb0 && P > 0))
    return idx < 0 ? fail(VX_ERR_ARG, "null argument") : fail(VX_ERR_ARG, "null argument (utterance %d)", idx);
  if (S <= 0 || P < 0) return fail(VX_ERR_ARG, "S must be > 0 (valle.py:991), P >= 0");
  const vx_config& c = e->cfg;
  const int A = (c.prepend_bos ? 1 : 0) + P;
  if (S > c.max_text || A + 1 > c.max_audio) return fail(VX_ERR_CAPACITY, "S=%d / P=%d exceed capacity", S, P);
  if (A == 0) return fail(VX_ERR_ARG, "empty audio prefix needs prepend_bos");
  return VX_OK;
}
// The decode state of a prefilled utterance as of "pass 0 computed" (row = its last prefill row), without decode parameters.
static void seed_state(ArState& st, int S, int P, int bos, int row, int kv_text, bool trace) {
  memset(&st, 0, sizeof st);
  st.S = S; st.bos = bos; st.P = P; st.row = row; st.kv_text = kv_text;
  st.temperature = 1.0f; st.max_new = -1; st.trace_logits = trace ? 1 : 0;
}

// Shared by vx_ar_prefill (slot < 0: the batch-1 buffers) and vx_batch_prefill (slot >= 0).
static int prefill_impl(vx_engine* e, int slot, const int64_t* text, int32_t S, const int64_t* prompt_cb0, int32_t P,
                        void* stream) {
  if (!e) return fail(VX_ERR_ARG, "null argument");
  if (!e->finalized) return fail(VX_ERR_STATE, "weights not finalized");
  VXC(check_utterance(e, text, S, prompt_cb0, P, -1));
  const vx_config& c = e->cfg;
  const bool vf = e->vallf;  // VALL-F: the stack runs over the audio rows only, the text is cross-attention memory (valle.py:598-632)
  const int bos = c.prepend_bos ? 1 : 0, A = bos + P, M = vf ? A : S + A, d = c.d_model;
  if (slot >= e->bmax) return fail(VX_ERR_ARG, "slot %d >= max_batch %d", slot, e->bmax);
  void* xkv = slot < 0 ? e->xkv_ar : (void*)(e->bmem + (size_t)slot * e->bmem_slot);  // VALL-F: this utterance's text memory
  ON_DEVICE(c.device);
  VXC(sync_in(e, stream));
  HIPC(hipEventRecord(e->ev_t[0], e->es));
  HIPC(hipMemcpyAsync(e->ids_text, text, (size_t)S * 8, hipMemcpyDefault, e->es));
  if (bos) {
    static const long long b = NUM_AUDIO_TOKENS + 1;  // valle.py:1006-1007
    HIPC(hipMemcpyAsync(e->ids_audio, &b, 8, hipMemcpyHostToDevice, e->es));
  }
  if (P) HIPC(hipMemcpyAsync(e->ids_audio + bos, prompt_cb0, (size_t)P * 8, hipMemcpyDefault, e->es));
  if (c.flags & VX_FLAG_PRENET) {  // embedding -> prenet -> position (valle.py:995-997, 1013-1015)
    embed_accum_kernel<<<S, 256, 0, e->es>>>(e->ids_text, 1, 0, W<float>(e, "ar_text_embedding.word_embeddings.weight"), 512, d, e->pn_a, S, 1);
    VXC(text_prenet_rows(e, 0, e->pn_a, e->pn_a, S, d));
    add_pos_kernel<<<S, 256, 0, e->es>>>(e->pn_a, d, W<float>(e, "ar_text_position.alpha"), e->pe_ar, 0, e->X, S);
    if (vf) { VXC(cast_rows(e, e->X, e->Hn, (size_t)S * d)); VXC(memory_kv(e, e->ar_l, xkv, S, d, c.nhead)); }
    embed_accum_kernel<<<A, 256, 0, e->es>>>(e->ids_audio, 1, 0, W<float>(e, "ar_audio_embedding.word_embeddings.weight"), 1025 + bos, d, e->pn_a, A, 1);
    VXC(audio_prenet_rows(e, 0, e->pn_a, e->pn_b, A, d));
    add_pos_kernel<<<A, 256, 0, e->es>>>(e->pn_b, d, W<float>(e, "ar_audio_position.alpha"), e->pe_ar, 0, e->X + (size_t)(vf ? 0 : S) * d, A);
  } else {
    embed_pos_kernel<<<S, 256, 0, e->es>>>(e->ids_text, 1, 0, W<float>(e, "ar_text_embedding.word_embeddings.weight"), 512, d,
                                           W<float>(e, "ar_text_position.alpha"), e->pe_ar, 0, e->X, S);
    // VALL-F: the text rows become the per-layer memory K / V (projected once, valle.py:598-602), then the audio rows take X
    if (vf) { VXC(cast_rows(e, e->X, e->Hn, (size_t)S * d)); VXC(memory_kv(e, e->ar_l, xkv, S, d, c.nhead)); }
    embed_pos_kernel<<<A, 256, 0, e->es>>>(e->ids_audio, 1, 0, W<float>(e, "ar_audio_embedding.word_embeddings.weight"), 1025 + bos, d,
                                           W<float>(e, "ar_audio_position.alpha"), e->pe_ar, 0, e->X + (size_t)(vf ? 0 : S) * d, A);
  }
  const KvDst kv = slot < 0 ? KvDst{KvDst::CACHE, (char*)e->kv}
                 : e->kv8  ? KvDst{KvDst::FP8_SLOT, nullptr, slot}
                           : KvDst{KvDst::CACHE, (char*)(e->bkv + (size_t)slot * e->bkv_slot)};
  float* x_dst = slot < 0 ? e->ar_x : e->bx + (size_t)slot * d;
  float* lg_dst = slot < 0 ? e->ar_logits : e->blogits + (size_t)slot * LOGITS_CUR;
  ArState* st_dst = slot < 0 ? e->d_st : e->bst + slot;
  if (vf && slot < 0) e->mem_len = S;
  // VALL-F: causal over the audio rows (text_len 0), kv a CACHE destination (VX_FLAG_KV_FP8 is refused for VALL-F)
  VXC(run_stack(e, e->ar_l, M, d, c.nhead, vf ? 0 : S, -1, RowSegs(), kv, vf ? TextMem{xkv, S} : TextMem()));
  HIPC(hipMemcpyAsync(x_dst, e->X + (size_t)(M - 1) * d, (size_t)d * 4, hipMemcpyDeviceToDevice, e->es));
  ArState& st = slot < 0 ? e->h_st[0] : e->h_bst[slot];
  seed_state(st, S, P, bos, M - 1, vf ? 0 : S, slot < 0 && (c.flags & VX_FLAG_TRACE_LOGITS));
  HIPC(hipMemcpyAsync(st_dst, &st, sizeof st, hipMemcpyHostToDevice, e->es));
  VXC(enqueue_head(e, e->es, x_dst, lg_dst, st_dst, true));
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(e->ev_t[1], e->es));
  HIPC(hipStreamSynchronize(e->es));  // the staging state is reused by decode
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, e->ev_t[0], e->ev_t[1]));
  e->t_prefill = ms;
  if (slot < 0) {
    e->S = S; e->P = P; e->bos = bos;
    e->prefilled = true; e->decoded = false;
    e->n_gen = 0; e->n_pass = 1; e->stop_reason = 0;
  } else {
    e->bS[slot] = S; e->bP[slot] = P; e->bbos[slot] = bos;
    e->bprefilled[slot] = true; e->bngen[slot] = 0; e->breason[slot] = 0; e->bnpass[slot] = 0;
  }
  VXC(sync_out(e, stream));
  return VX_OK;
}

extern "C" int vx_ar_prefill(vx_engine* e, const int64_t* text, int32_t S, const int64_t* prompt_cb0, int32_t P,
                             void* stream) {
  return prefill_impl(e, -1, text, S, prompt_cb0, P, stream);
}

extern "C" int vx_batch_prefill(vx_engine* e, int32_t slot, const int64_t* text, int32_t S, const int64_t* prompt_cb0,
                                int32_t P, void* stream) {
  if (!e) return fail(VX_ERR_ARG, "null engine");
  if (slot < 0 || slot >= e->bmax) return fail(VX_ERR_ARG, "slot %d outside [0, max_batch=%d)", slot, e->bmax);
  e->bsess = false;  // the static calls end a continuous-batching session
  return prefill_impl(e, slot, text, S, prompt_cb0, P, stream);
}

// Several slots' prefills as ONE pass over the concatenated rows (each segment starts at a multiple of 64 rows):
// the GEMMs see sum(M_z) rows instead of 32 separate ~270-row problems, attention runs per segment with each
// segment's own prefix mask, K/V go straight to each slot's cache.  Same results as vx_batch_prefill per slot up
// to the GEMM kernel the dispatcher picks for the larger row count.
static int ensure_rows(vx_engine* e, size_t rows, size_t audio_rows, size_t text_rows);
template <int EPI> static int launch_bgemm(const BgemmArgs& a, hipStream_t s);

// n utterances of len[z] rows as segments of e->X, each starting at a multiple of 64 rows: start[z] (n + 1 entries, start[n] =
// all rows), row buffers and the id / embedding staging (audio_rows / text_rows) grown to fit, the layout uploaded on e->es,
// X zeroed over all rows (padding rows must stay finite: they feed V^T columns).  text / slot (optional): per-segment prefix
// lengths / slots.  min_rows: rows the buffers must hold besides (VALL-F: the concatenated text rows pass through them on their
// way to the text memory).  The host arrays must outlive the pass (the uploads are asynchronous).
static int seg_layout(vx_engine* e, int n, const int* len, const int* text, const int* slot, int d, size_t audio_rows,
                      size_t text_rows, int* start, RowSegs& segs, size_t min_rows = 0) {
  segs = RowSegs{n, 0, e->d_seg_start, e->d_seg_len, text ? e->d_seg_text : nullptr, slot ? e->d_seg_slot : nullptr};
  start[0] = 0;
  for (int z = 0; z < n; ++z) {
    start[z + 1] = start[z] + (len[z] + 63) / 64 * 64;
    if (len[z] > segs.max_len) segs.max_len = len[z];
  }
  VXC(ensure_rows(e, std::max((size_t)start[n], min_rows), audio_rows, text_rows));
  HIPC(hipMemcpyAsync(e->d_seg_start, start, n * sizeof(int), hipMemcpyHostToDevice, e->es));
  HIPC(hipMemcpyAsync(e->d_seg_len, len, n * sizeof(int), hipMemcpyHostToDevice, e->es));
  if (text) HIPC(hipMemcpyAsync(e->d_seg_text, text, n * sizeof(int), hipMemcpyHostToDevice, e->es));
  if (slot) HIPC(hipMemcpyAsync(e->d_seg_slot, slot, n * sizeof(int), hipMemcpyHostToDevice, e->es));
  HIPC(hipMemsetAsync(e->X, 0, (size_t)start[n] * d * 4, e->es));
  return VX_OK;
}

// Segment z -> slot slots[z]: only those slots' KV caches, bx / blogits / trace rows and ArState are written; bh rows are step
// scratch.
static int batch_prefill_impl(vx_engine* e, int32_t n, const int32_t* slots, const int64_t* const* text, const int32_t* S,
                              const int64_t* const* prompt_cb0, const int32_t* P, void* stream) {
  if (!e || !text || !S || !prompt_cb0 || !P) return fail(VX_ERR_ARG, "null argument");
  if (!e->finalized) return fail(VX_ERR_STATE, "weights not finalized");
  if (n < 1 || n > e->bmax) return fail(VX_ERR_ARG, "n %d outside [1, max_batch=%d]", n, e->bmax);
  if (!e->bf16 || !use_mfma(e)) return fail(VX_ERR_UNSUPPORTED, "vx_batch_prefill_all needs the bf16 MFMA row kernels");
  const vx_config& c = e->cfg;
  const int bos = c.prepend_bos ? 1 : 0, d = c.d_model;
  // VALL-F (VX_FLAG_VALLF_ROWS): the rows are the audio rows only, causal (prefix 0) as the per-slot prefill; the text goes to the
  // slots' text memories
  const bool vf = e->vallf;
  std::vector<int> start(n + 1), len(n), tlen(n), soff(n);
  std::vector<long long> moff(n);
  int srows = 0;
  for (int b = 0; b < n; ++b) {
    if (vf && S[b] > c.max_text)  // the slot's text memory holds max_text keys; nothing has been written yet
      return fail(VX_ERR_CAPACITY, "utterance %d: a text of %d tokens exceeds max_text=%d", b, S[b], c.max_text);
    VXC(check_utterance(e, text[b], S[b], prompt_cb0[b], P[b], b));
    tlen[b] = vf ? 0 : S[b];
    len[b] = tlen[b] + bos + P[b];
    soff[b] = srows; srows += S[b];
    moff[b] = (long long)slots[b] * (long long)e->bmem_slot;
  }
  ON_DEVICE(c.device);
  VXC(sync_in(e, stream));
  HIPC(hipEventRecord(e->ev_t[0], e->es));
  RowSegs segs;
  VXC(seg_layout(e, n, len.data(), tlen.data(), slots, d, e->cap_audio, e->cap_text, start.data(), segs, vf ? srows : 0));
  TextMem tmem;
  if (vf) {  // text rows (concatenated, rows [0, sum S) of X) -> every slot's memory in bmem, then X is the audio rows' again
    for (int b = 0; b < n; ++b) {
      long long* it = e->bp_text + (size_t)b * c.max_text;
      HIPC(hipMemcpyAsync(it, text[b], (size_t)S[b] * 8, hipMemcpyDefault, e->es));
      embed_pos_kernel<<<S[b], 256, 0, e->es>>>(it, 1, 0, W<float>(e, "ar_text_embedding.word_embeddings.weight"), 512, d,
                                                W<float>(e, "ar_text_position.alpha"), e->pe_ar, 0, e->X + (size_t)soff[b] * d, S[b]);
    }
    VXC(cast_rows(e, e->X, e->Hn, (size_t)srows * d));
    tmem.kv = e->bmem; tmem.off = e->d_mem_off; tmem.klen = e->d_mem_klen;
    tmem.head_stride = (long long)c.max_text * 64; tmem.v_offset = (long long)c.max_text * d; tmem.layer_stride = 2 * tmem.v_offset;
    VXC(memory_kv_segs(e, e->ar_l, tmem, n, moff.data(), S, soff.data(), srows, d));
    HIPC(hipMemsetAsync(e->X, 0, (size_t)start[n] * d * 4, e->es));
  }
  static const long long bos_id = NUM_AUDIO_TOKENS + 1;  // valle.py:1006-1007
  for (int b = 0; b < n; ++b) {
    const int A = bos + P[b];
    long long* it = e->bp_text + (size_t)b * c.max_text;
    long long* ia = e->bp_audio + (size_t)b * (c.max_audio + 1);
    if (!vf) HIPC(hipMemcpyAsync(it, text[b], (size_t)S[b] * 8, hipMemcpyDefault, e->es));
    if (bos) HIPC(hipMemcpyAsync(ia, &bos_id, 8, hipMemcpyHostToDevice, e->es));
    if (P[b]) HIPC(hipMemcpyAsync(ia + bos, prompt_cb0[b], (size_t)P[b] * 8, hipMemcpyDefault, e->es));
    float* xb = e->X + (size_t)start[b] * d;
    if (!vf) embed_pos_kernel<<<S[b], 256, 0, e->es>>>(it, 1, 0, W<float>(e, "ar_text_embedding.word_embeddings.weight"), 512, d,
                                                       W<float>(e, "ar_text_position.alpha"), e->pe_ar, 0, xb, S[b]);
    embed_pos_kernel<<<A, 256, 0, e->es>>>(ia, 1, 0, W<float>(e, "ar_audio_embedding.word_embeddings.weight"), 1025 + bos, d,
                                           W<float>(e, "ar_audio_position.alpha"), e->pe_ar, 0, xb + (size_t)tlen[b] * d, A);
  }
  VXC(run_stack(e, e->ar_l, start[n], d, c.nhead, 0, -1, segs, KvDst{KvDst::SEG_SLOTS}, tmem));
  // last row of every segment = the slot's current activation
  for (int b = 0; b < n; ++b) {
    const int sl = slots[b];
    HIPC(hipMemcpyAsync(e->bx + (size_t)sl * d, e->X + (size_t)(start[b] + len[b] - 1) * d, (size_t)d * 4, hipMemcpyDeviceToDevice, e->es));
    seed_state(e->h_bst[sl], S[b], P[b], bos, len[b] - 1, tlen[b], false);
    HIPC(hipMemcpyAsync(e->bst + sl, &e->h_bst[sl], sizeof(ArState), hipMemcpyHostToDevice, e->es));
  }
  // first logits of every slot: final LayerNorm + head, as at the end of a batched step
  ln_batch_map_kernel<<<n, 256, 0, e->es>>>(e->bx, W<float>(e, "ar_decoder.norm.weight"), W<float>(e, "ar_decoder.norm.bias"), e->bh, d,
                                            e->d_seg_slot);
  BgemmArgs hgm{};
  hgm.st = e->bst; hgm.B = n;
  hgm.A = e->bh; hgm.W = W<bf16>(e, "ar_predict_layer.weight"); hgm.N = AR_VOCAB; hgm.K = d; hgm.kgroups = 1;
  hgm.logits = e->blogits; hgm.logits_stride = LOGITS_CUR;
  hgm.trace = e->btrace; hgm.trace_rows = e->btok_stride;
  hgm.slot_map = e->d_seg_slot;
  VXC(launch_bgemm<BE_LOGITS_MAP>(hgm, e->es));
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(e->ev_t[1], e->es));
  HIPC(hipStreamSynchronize(e->es));  // the staging state is reused by decode
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, e->ev_t[0], e->ev_t[1]));
  e->t_prefill = ms;
  for (int b = 0; b < n; ++b) {
    const int sl = slots[b];
    e->bS[sl] = S[b]; e->bP[sl] = P[b]; e->bbos[sl] = bos;
    e->bprefilled[sl] = true; e->bngen[sl] = 0; e->breason[sl] = 0; e->bnpass[sl] = 0;
  }
  VXC(sync_out(e, stream));
  return VX_OK;
}

extern "C" int vx_batch_prefill_all(vx_engine* e, int32_t n, const int64_t* const* text, const int32_t* S,
                                    const int64_t* const* prompt_cb0, const int32_t* P, void* stream) {
  if (e && e->vallf && !e->vf_rows) return fail(VX_ERR_UNSUPPORTED, "vx_batch_prefill_all: VALL-F prefills slot by slot (vx_batch_prefill)");
  if (e) e->bsess = false;  // the static calls end a continuous-batching session
  int32_t slots[BMAX];  // segment z -> slot z
  for (int z = 0; z < BMAX; ++z) slots[z] = z;
  return batch_prefill_impl(e, n, slots, text, S, prompt_cb0, P, stream);
}

// The layers and the head of the XCD-sharded step (ar_tp.hpp); the sampling launch in front of them is the caller's (it writes
// the fp32 embedding into ar_x and zeroes accumulator 1).  Launch n = 2 li (attention half), 2 li + 1 (feed-forward half), 2 L
// (head) normalises accumulator n % 3, adds into (n + 1) % 3 and zeroes (n + 2) % 3; layer 0's attention half reads ar_x instead.
static int enqueue_ar_step_tp(vx_engine* e, hipStream_t s) {
  const vx_config& c = e->cfg;
  const int H = c.nhead, hd = c.d_model / H, L = c.num_layers;
  const size_t kv_layer = (size_t)2 * H * e->ctx_max * hd * e->esz;
  const int grid = TP_X * TP_WG;
  auto acc = [&](int n) { return e->tp_xacc + (size_t)(n % 3) * TP_D; };
  for (int li = 0; li < L; ++li) {
    const LayerW& l = e->ar_l[li];
    char* kc = (char*)e->kv + (size_t)li * kv_layer;
    const int n = 2 * li;
    TpAttnArgs a{};
    const float* gbb = e->tp_gbb + (size_t)(2 * li) * 3 * TP_D;
    a.qkv_bias = l.in_b; a.err = e->d_epoch + 1;
    a.gq = e->fq_gq + (size_t)li * H * FQ_QKV; a.gp = e->fq_gp + (size_t)li * H * FQ_S * FQ_PART;
    a.acc.add = acc(n + 1); a.acc.zero = acc(n + 2); a.acc.bias = l.out_b;
    a.kcache = kc; a.vcache = kc + kv_layer / 2; a.ctx_max = e->ctx_max;
    a.scale = 1.0f / sqrtf((float)hd); a.layer = li;
    if (e->bf16) {
      if (li) tp_attn_kernel<bf16, false><<<grid, 256, 0, s>>>(l.in_w, e->ar_x, acc(n), gbb, e->d_st, e->d_epoch, e->tp_wo[li], a);
      else tp_attn_kernel<bf16, true><<<grid, 256, 0, s>>>(l.in_w, e->ar_x, acc(n), gbb, e->d_st, e->d_epoch, e->tp_wo[li], a);
    } else {
      if (li) tp_attn_kernel<float, false><<<grid, 256, 0, s>>>(l.in_w, e->ar_x, acc(n), gbb, e->d_st, e->d_epoch, e->tp_wo[li], a);
      else tp_attn_kernel<float, true><<<grid, 256, 0, s>>>(l.in_w, e->ar_x, acc(n), gbb, e->d_st, e->d_epoch, e->tp_wo[li], a);
    }
    TpFfnArgs f{};
    f.b1 = l.b1; f.err = e->d_epoch + 1; f.gh = e->tp_gh + (size_t)li * TP_X * TP_HID; f.layer = li;
    f.acc.add = acc(n + 2); f.acc.zero = acc(n + 3); f.acc.bias = l.b2;
    if (e->bf16) tp_ffn_kernel<bf16><<<grid, 256, 0, s>>>(l.w1, acc(n + 1), gbb + 3 * TP_D, e->d_epoch, e->tp_w2[li], f);
    else tp_ffn_kernel<float><<<grid, 256, 0, s>>>(l.w1, acc(n + 1), gbb + 3 * TP_D, e->d_epoch, e->tp_w2[li], f);
  }
  TpHeadArgs h{};
  h.logits = e->ar_logits; h.N = AR_VOCAB;
  const int hg = (AR_VOCAB + 15) / 16;
  const float* gbh = e->tp_gbb + (size_t)(2 * L) * 3 * TP_D;
  if (e->bf16) tp_head_kernel<bf16><<<hg, 256, 0, s>>>(W<void>(e, "ar_predict_layer.weight"), acc(2 * L), gbh, e->d_st, h);
  else tp_head_kernel<float><<<hg, 256, 0, s>>>(W<void>(e, "ar_predict_layer.weight"), acc(2 * L), gbh, e->d_st, h);
  return VX_OK;
}

static SampleArgs step_sample_args(vx_engine* e) {
  const vx_config& c = e->cfg;
  SampleArgs sa{};
  sa.logits = e->ar_logits; sa.V = AR_VOCAB; sa.st = e->d_st;
  sa.tokens = e->d_tokens; sa.sampled = e->d_sampled; sa.argmaxes = e->d_argmax;
  sa.emb = W<float>(e, "ar_audio_embedding.word_embeddings.weight");
  sa.alpha = W<float>(e, "ar_audio_position.alpha");
  sa.pe = e->pe_ar; sa.x = e->ar_x; sa.d = c.d_model;
  if (c.flags & VX_FLAG_PRENET) { sa.alpha = e->d_zero; sa.x = e->ar_e; }  // raw embedding; the position is added after the prenet
  sa.kid = 0;  // stamp ids of the step (probe builds): 0 sampling, 1 + 5 l + {0 QKV, 1 attention, 2 out-proj, 3 FFN1, 4 FFN2}, 61 head
  sa.epoch = e->d_epoch;
  sa.zero_acc = e->tp ? e->tp_xacc + TP_D : nullptr;  // accumulator 1: layer 0's attention half adds into it
  return sa;
}
// y_emb = ar_audio_prenet(E[tok]); x = y_emb + alpha * pe (valle.py:1013-1015): three fp32 GEMVs, ar_e -> ar_x
static int enqueue_audio_prenet(vx_engine* e, hipStream_t s) {
  const int d = e->cfg.d_model;
  GemvArgs p0{}, p1{}, p2{};
  p0.st = p1.st = p2.st = e->d_st;
  p0.kid = p1.kid = p2.kid = -1;
  p0.W = W<void>(e, "ar_audio_prenet.0.weight"); p0.bias = W<float>(e, "ar_audio_prenet.0.bias");
  p0.x = e->ar_e; p0.y = e->ar_h1; p0.N = PRENET_H; p0.K = d; p0.pro = PRO_COPY; p0.epi = EPI_RELU;
  p1.W = W<void>(e, "ar_audio_prenet.3.weight"); p1.bias = W<float>(e, "ar_audio_prenet.3.bias");
  p1.x = e->ar_h1; p1.y = e->ar_h2; p1.N = PRENET_H; p1.K = PRENET_H; p1.pro = PRO_COPY; p1.epi = EPI_RELU;
  p2.W = W<void>(e, "ar_audio_prenet.6.weight"); p2.bias = W<float>(e, "ar_audio_prenet.6.bias");
  p2.x = e->ar_h2; p2.y = e->ar_x; p2.N = d; p2.K = PRENET_H; p2.pro = PRO_COPY; p2.epi = EPI_POS;
  p2.pe = e->pe_ar; p2.pos_alpha = W<float>(e, "ar_audio_position.alpha");
  VXC(launch_gemv(false, p0, e->num_cu, s));
  VXC(launch_gemv(false, p1, e->num_cu, s));
  return launch_gemv(false, p2, e->num_cu, s);
}

// Split-KV attention of the step's query ar_q over one cache, (nhead, ctx_max, hd) per K / V, into ar_part: keys 0 .. ArState.row
// (causal), or with fixed_ctx the first ArState.S (the text memory).  kid >= 0: stamped (probe builds: one extra workgroup).
template <typename T>
static int launch_attn_decode_t(vx_engine* e, hipStream_t s, const T* kc, const T* vc, int ctx_max, int fixed_ctx, int kid) {
  const int H = e->cfg.nhead, hd = e->cfg.d_model / H;
  const float scale = 1.0f / sqrtf((float)hd);
  const int grid = H * ATT_NSPLIT + (kid >= 0 ? VX_KSTAMP_EXTRA : 0);
  const float* q = e->ar_q;
  float* part = e->ar_part;
  switch (hd) {
    case 64: attn_decode_kernel<T, 64><<<grid, 256, 0, s>>>(q, kc, vc, part, e->d_st, ctx_max, scale, kid, fixed_ctx); break;
    case 32: attn_decode_small_kernel<T, 32><<<grid, 256, 0, s>>>(q, kc, vc, part, e->d_st, ctx_max, scale, kid, fixed_ctx); break;
    case 16: attn_decode_small_kernel<T, 16><<<grid, 256, 0, s>>>(q, kc, vc, part, e->d_st, ctx_max, scale, kid, fixed_ctx); break;
    case 8: attn_decode_small_kernel<T, 8><<<grid, 256, 0, s>>>(q, kc, vc, part, e->d_st, ctx_max, scale, kid, fixed_ctx); break;
    case 4: attn_decode_small_kernel<T, 4><<<grid, 256, 0, s>>>(q, kc, vc, part, e->d_st, ctx_max, scale, kid, fixed_ctx); break;
    default: return fail(VX_ERR_UNSUPPORTED, "decode attention: head_dim %d", hd);
  }
  return VX_OK;
}
static int launch_attn_decode(vx_engine* e, hipStream_t s, const void* kc, const void* vc, int ctx_max, int fixed_ctx, int kid) {
  if (e->bf16) return launch_attn_decode_t(e, s, (const bf16*)kc, (const bf16*)vc, ctx_max, fixed_ctx, kid);
  return launch_attn_decode_t(e, s, (const float*)kc, (const float*)vc, ctx_max, fixed_ctx, kid);
}

// One decode step: sample from the newest logits, append, run the stack on the new token, produce the next logits.  Every kernel
// reads its position from e->d_st, so the same launch sequence (captured once as a hipGraph) serves every pass.  Per layer: QKV
// GEMV, attention over the cached audio rows, out-projection; VALL-F (valle.py:613-647, transformer.py:536-560) then its
// cross-attention block: query GEMV (rows [0, d) of the packed multihead_attn in_proj), single-query attention over the layer's
// text memory, its out-projection; then FFN1, FFN2.  Every norm runs in the prologue of the GEMV that consumes it (front_site).
// Post-norm (transformer.py:303-308): ar_x holds the raw sum x + block(x) of the previous block, and the prologue that normalises
// it also leaves the normalised vector in ar_xn as the base of the next residual add.
// mel: the step of a vx_mel handle - its opening kernel stands where the sampler does, the last layer leaves its row in mel->xh
// for the next step's opening kernel and there is no token head.
struct MelStep { MelStepArgs open; };
static int enqueue_ar_step(vx_engine* e, hipStream_t s, const MelStep* mel = nullptr) {
  const vx_config& c = e->cfg;
  const int d = c.d_model, H = c.nhead, hd = d / H;
  if (mel) launch_mel_open(mel->open, s);
  else if (e->lpon) launch_sample_lp(step_sample_args(e), e->d_lp, NUM_AUDIO_TOKENS, 1, s);
  else sample_embed4_kernel<5, 17><<<1, 256, 0, s>>>(step_sample_args(e));
  if (e->tp) return enqueue_ar_step_tp(e, s);
  if (!mel && (c.flags & VX_FLAG_PRENET)) VXC(enqueue_audio_prenet(e, s));
  const size_t kv_layer = (size_t)2 * H * e->ctx_max * hd * e->esz;
  const size_t mem_layer = (size_t)2 * d * c.max_text * e->esz;
  // Stamp ids (probe builds, step_sample_args): the 64-entry ring holds 5 launches per layer and 61 for the head, so a VALL-F
  // layer's 8 launches do not fit and stay unstamped (-1: no extra workgroup).
  auto kid = [&](int li, int j) { return e->vallf ? -1 : 1 + 5 * li + j; };
  // L2 / Infinity-Cache warm-up (GemvArgs.pf): GEMV i of the step also requests the weights of GEMV i + dist, in step order
  // [QKV_0, out_0, FFN1_0, FFN2_0, QKV_1, ..., FFN2_{L-1}, head] and wrapping into the next token's step.  VALL-E only.
  static const int pf_env = getenv("VX_AR_PREFETCH") ? atoi(getenv("VX_AR_PREFETCH")) : 2;
  const int pf_dist = e->vallf ? 0 : pf_env;
  struct PfW { const void* W; int N, K; };
  std::vector<PfW> seq;
  for (int li = 0; li < c.num_layers; ++li) {
    const LayerW& l = e->ar_l[li];
    seq.push_back({l.in_w, 3 * d, d}); seq.push_back({l.out_w, d, d}); seq.push_back({l.w1, 4 * d, d}); seq.push_back({l.w2, d, 4 * d});
  }
  if (!mel) seq.push_back({W<void>(e, "ar_predict_layer.weight"), AR_VOCAB, d});
  auto warm = [&](GemvArgs& a, int idx) {
    if (pf_dist <= 0) return;
    const PfW& n = seq[(idx + pf_dist) % seq.size()];
    gemv_prefetch(a, n.W, n.N, n.K, e->bf16, e->num_cu);
  };
  // The norm in front of block k of layer li into a's prologue (none in front of post-norm layer 0).  Returns the residual base
  // of the block's closing GEMV: post-norm the normalised vector in ar_xn, else null (ar_x itself).
  auto norm_in = [&](GemvArgs& a, int li, int k) -> const float* {
    const int n = front_site(e, li, k);
    if (n < 0) { a.pro = PRO_COPY; return nullptr; }
    const NormW nw = norm_at(e, e->ar_l, n);
    a.pro = PRO_LN; a.gamma = nw.g; a.beta = nw.b;
    if (!(c.flags & VX_FLAG_POST_NORM)) return nullptr;
    a.xnorm_out = e->ar_xn;
    return e->ar_xn;
  };
  for (int li = 0; li < c.num_layers; ++li) {
    const LayerW& l = e->ar_l[li];
    char* kc = (char*)e->kv + (size_t)li * kv_layer;
    char* vc = kc + kv_layer / 2;
    // qkv = in_proj(norm(x)); k,v appended to the cache (transformer.py:297-301); x += out_proj(attn)
    GemvArgs a{};
    a.st = e->d_st; a.d = d; a.hd = hd; a.ctx_max = e->ctx_max; a.nhead = H;
    a.W = l.in_w; a.bias = l.in_b; a.x = e->ar_x;
    a.N = 3 * d; a.K = d; a.epi = EPI_QKV; a.q = e->ar_q; a.kcache = kc; a.vcache = vc;
    const float* res = norm_in(a, li, 0);
    warm(a, 4 * li);
    a.kid = kid(li, 0);
    VXC(launch_gemv(e->bf16, a, e->num_cu, s));
    VXC(launch_attn_decode(e, s, kc, vc, e->ctx_max, 0, kid(li, 1)));
    GemvArgs o{};
    o.st = e->d_st; o.hd = hd; o.nhead = H;
    o.W = l.out_w; o.bias = l.out_b; o.part = e->ar_part; o.y = e->ar_x; o.N = d; o.K = d; o.pro = PRO_ATTN; o.epi = EPI_RESID;
    o.res = res;
    warm(o, 4 * li + 1);
    o.kid = kid(li, 2);
    VXC(launch_gemv(e->bf16, o, e->num_cu, s));
    if (e->vallf) {  // q = in_proj[0:d](norm(x)); x += out_proj(attention over the text memory, ArState.S rows)
      GemvArgs q{};
      q.st = e->d_st; q.kid = -1;
      q.W = l.cin_w; q.bias = l.cin_b; q.x = e->ar_x; q.y = e->ar_q; q.N = d; q.K = d; q.epi = EPI_BIAS;
      const float* cres = norm_in(q, li, 1);
      VXC(launch_gemv(e->bf16, q, e->num_cu, s));
      const char* xk = (const char*)e->xkv_ar + (size_t)li * mem_layer;
      VXC(launch_attn_decode(e, s, xk, xk + mem_layer / 2, c.max_text, 1, -1));
      GemvArgs co{};
      co.st = e->d_st; co.hd = hd; co.nhead = H; co.kid = -1;
      co.W = l.cout_w; co.bias = l.cout_b; co.part = e->ar_part; co.y = e->ar_x; co.N = d; co.K = d; co.pro = PRO_ATTN; co.epi = EPI_RESID;
      co.res = cres;
      VXC(launch_gemv(e->bf16, co, e->num_cu, s));
    }
    // f = relu(linear1(norm(x))); x += linear2(f)
    GemvArgs f{};
    f.st = e->d_st;
    f.W = l.w1; f.bias = l.b1; f.x = e->ar_x; f.y = e->ar_f; f.N = 4 * d; f.K = d; f.epi = EPI_RELU;
    const float* fres = norm_in(f, li, e->npl - 1);
    warm(f, 4 * li + 2);
    f.kid = kid(li, 3);
    VXC(launch_gemv(e->bf16, f, e->num_cu, s));
    GemvArgs g{};
    g.st = e->d_st;
    g.W = l.w2; g.bias = l.b2; g.x = e->ar_f; g.y = e->ar_x; g.N = d; g.K = 4 * d; g.pro = PRO_COPY; g.epi = EPI_RESID;
    g.res = fres;
    if (mel && li == c.num_layers - 1) { g.y = const_cast<float*>(mel->open.xh); g.res = fres ? fres : e->ar_x; }
    warm(g, 4 * li + 3);
    g.kid = kid(li, 4);
    VXC(launch_gemv(e->bf16, g, e->num_cu, s));
  }
  if (mel) return VX_OK;
  if (pf_dist > 0) {
    const PfW& n = seq[(4 * c.num_layers + pf_dist) % seq.size()];
    return enqueue_head(e, s, nullptr, nullptr, nullptr, false, n.W, n.N, n.K);
  }
  return enqueue_head(e, s);
}

// The checks of one utterance's decode parameters (no HIP call) and its step bound: the launches after which the stop rule must
// have fired (>= 1).  16 S + 1 tokens is the WORST case (valle.py:1047); a trained model stops at EOS long before it, so a long
// text must not be refused up front: the bound is clamped to the rows the KV cache has (*cap_limited; `room` of them), and only a
// decode that really fills them while the stop rule has not fired is a capacity error.  S / P / bos are the prefill geometry;
// slot >= 0 names the batch slot in the message.
// top_p: NaN or negative is an error; 0 and >= 1 are off (stored as 0), (0, 1) filters.
static int check_top_p(float top_p) {
  if (!(top_p >= 0.f)) return fail(VX_ERR_ARG, "top_p must be >= 0 (0 or >= 1: off), got %g", (double)top_p);
  return VX_OK;
}
static float state_top_p(float top_p) { return top_p > 0.f && top_p < 1.f ? top_p : 0.f; }

static int decode_bound(vx_engine* e, int slot, const vx_decode_params& p, int S, int P, int bos, long long* steps,
                        bool* cap_limited, long long* room) {
  if (p.struct_size != (int32_t)sizeof(vx_decode_params)) return fail(VX_ERR_ARG, "vx_decode_params.struct_size mismatch");
  if (!(p.temperature > 0.f)) return fail(VX_ERR_ARG, "temperature must be > 0");
  VXC(check_top_p(p.top_p));
  long long max_tok = 16LL * S + 1 - bos;  // appended tokens (valle.py:1047: stops once bos + n_gen > 16 S)
  if (p.forced) max_tok = p.n_forced;
  else if (p.max_new_tokens >= 0 && p.max_new_tokens < max_tok) max_tok = p.max_new_tokens;
  const int cap = e->cfg.max_audio;
  *room = (long long)cap - bos - P;  // >= 1 (checked at prefill)
  *cap_limited = false;
  if (max_tok > *room) {
    if (p.forced)
      return slot < 0 ? fail(VX_ERR_CAPACITY, "need %lld audio rows, capacity %d", bos + P + max_tok, cap)
                      : fail(VX_ERR_CAPACITY, "slot %d needs %lld audio rows, capacity %d", slot, bos + P + max_tok, cap);
    max_tok = *room; *cap_limited = true;
  }
  // step j samples from logits j and appends token j+1; the step that appends the last admissible token also raises the stop
  // flag, so max_tok launches suffice (teacher forcing needs one more to close the sequence); EOS can only end it earlier.
  *steps = max_tok + (p.forced ? 1 : 0);
  if (*steps < 1) *steps = 1;
  return VX_OK;
}

// Captures enqueue(e->es) into *out on first use; with VX_FLAG_NO_GRAPH *out stays null and the step is enqueued directly.
template <typename F> static int step_graph(vx_engine* e, hipGraphExec_t* out, F enqueue, int* n_nodes = nullptr) {
  if (*out || (e->cfg.flags & VX_FLAG_NO_GRAPH)) return VX_OK;
  hipGraph_t gr = nullptr;
  HIPC(hipStreamBeginCapture(e->es, hipStreamCaptureModeThreadLocal));
  const int r = enqueue(e->es);
  hipError_t ce = hipStreamEndCapture(e->es, &gr);
  if (r == VX_OK && ce == hipSuccess && n_nodes) {
    size_t nn = 0;
    ce = hipGraphGetNodes(gr, nullptr, &nn);
    *n_nodes = (int)nn;
  }
  if (r == VX_OK && ce == hipSuccess) ce = hipGraphInstantiate(out, gr, nullptr, nullptr, 0);
  if (gr) (void)hipGraphDestroy(gr);
  VXC(r);
  HIPC(ce);
  return VX_OK;
}

// The decode loop of every AR path.  Replays the step (graph gx, or enqueue(e->es) when gx is null) in chunks of `chunk`
// launches, `bound` at most, and copies the n device states `st` into the host buffers poll[0] / poll[1] in turn behind each
// chunk.  One chunk stays in flight while the copy behind the previous one is inspected: inspect(snapshot, launches at that poll)
// returns POLL_MORE, POLL_STOP or an error code.  The poll that reaches the bound ends the loop whatever it returns; the chunk
// still in flight at the end is waited for and inspected too.  *ms spans ev_t[2] (in front of the first replay) to ev_t[3]
// (behind the last poll copy).
enum { POLL_MORE = VX_OK, POLL_STOP = -1 };
template <typename F, typename I>
static int replay_polled(vx_engine* e, hipGraphExec_t gx, F enqueue, long long bound, int chunk, const ArState* st, int n,
                         ArState* const poll[2], I inspect, long long* launched, float* ms) {
  long long at[2] = {0, 0};
  bool pending[2] = {false, false}, done = false;
  auto look = [&](int k) -> int {
    HIPC(hipEventSynchronize(e->ev_poll[k]));
    pending[k] = false;
    const int r = inspect(poll[k], at[k]);
    if (r == POLL_STOP) done = true;
    return r == POLL_STOP ? VX_OK : r;
  };
  *launched = 0;
  HIPC(hipEventRecord(e->ev_t[2], e->es));
  for (int k = 0; !done; k ^= 1) {
    const long long m = (bound - *launched) < chunk ? (bound - *launched) : chunk;
    for (long long i = 0; i < m; ++i) {
      if (gx) HIPC(hipGraphLaunch(gx, e->es));
      else VXC(enqueue(e->es));
    }
    *launched += m;
    HIPC(hipMemcpyAsync(poll[k], st, (size_t)n * sizeof(ArState), hipMemcpyDeviceToHost, e->es));
    HIPC(hipEventRecord(e->ev_poll[k], e->es));
    pending[k] = true; at[k] = *launched;
    if (pending[k ^ 1]) VXC(look(k ^ 1));
    if (!done && *launched >= bound) { VXC(look(k)); done = true; }
  }
  HIPC(hipEventRecord(e->ev_t[3], e->es));
  for (int k = 0; k < 2; ++k)
    if (pending[k]) VXC(look(k));
  HIPC(hipEventSynchronize(e->ev_t[3]));
  HIPC(hipGetLastError());
  HIPC(hipEventElapsedTime(ms, e->ev_t[2], e->ev_t[3]));
  return VX_OK;
}

extern "C" int vx_ar_decode(vx_engine* e, const vx_decode_params* p, void* stream) {
  if (!e || !p) return fail(VX_ERR_ARG, "null argument");
  if (p->struct_size != (int32_t)sizeof(vx_decode_params)) return fail(VX_ERR_ARG, "vx_decode_params.struct_size mismatch");
  if (!e->prefilled || e->decoded) return fail(VX_ERR_STATE, "vx_ar_decode needs a fresh vx_ar_prefill");
  long long bound = 0, room = 0;
  bool cap_limited = false;
  VXC(decode_bound(e, -1, *p, e->S, e->P, e->bos, &bound, &cap_limited, &room));
  const vx_config& c = e->cfg;
  ON_DEVICE(c.device);
  VXC(sync_in(e, stream));
  if (p->exp_noise) {
    if (p->noise_rows <= 0) return fail(VX_ERR_ARG, "noise_rows must be > 0");
    const size_t need = (size_t)p->noise_rows * AR_VOCAB;
    if (need > e->noise_cap) {
      if (e->d_noise) HIPC(hipFree(e->d_noise));
      HIPC(hipMalloc((void**)&e->d_noise, need * 4));
      e->noise_cap = need;
    }
    HIPC(hipMemcpyAsync(e->d_noise, p->exp_noise, need * 4, hipMemcpyDefault, e->es));
  }
  if (p->forced && p->n_forced > 0) {
    if ((size_t)p->n_forced > e->forced_cap) {
      if (e->d_forced) HIPC(hipFree(e->d_forced));
      HIPC(hipMalloc((void**)&e->d_forced, (size_t)p->n_forced * 8));
      e->forced_cap = p->n_forced;
    }
    HIPC(hipMemcpyAsync(e->d_forced, p->forced, (size_t)p->n_forced * 8, hipMemcpyDefault, e->es));
  }
  ArState& st = e->h_st[0];
  st.top_k = p->top_k; st.temperature = p->temperature; st.max_new = cap_limited ? (int)room : p->max_new_tokens;
  st.top_p = state_top_p(p->top_p);
  st.exp_noise = p->exp_noise ? e->d_noise : nullptr;
  st.noise_rows = p->noise_rows; st.seed = p->seed;
  st.forced = p->forced ? (p->n_forced > 0 ? e->d_forced : (const long long*)e->d_tokens) : nullptr;
  st.n_forced = p->forced ? p->n_forced : 0;
  HIPC(hipMemcpyAsync(e->d_st, &st, sizeof st, hipMemcpyHostToDevice, e->es));

  auto step = [e](hipStream_t s) { return enqueue_ar_step(e, s); };
  VXC(step_graph(e, &e->gexec, step, &e->gexec_nodes));
  auto stop_rule = [&](const ArState* hs, long long at) -> int {
    if (hs->done) return POLL_STOP;
    return at < bound ? POLL_MORE : fail(VX_ERR_STATE, "decode did not terminate within %lld steps", bound);
  };
  ArState* const poll[2] = {e->h_st + 1, e->h_st + 2};
  long long launched = 0;
  float ms = 0.f;
  VXC(replay_polled(e, e->gexec, step, bound, POLL_CHUNK, e->d_st, 1, poll, stop_rule, &launched, &ms));
  HIPC(hipMemcpyAsync(&e->h_st[1], e->d_st, sizeof(ArState), hipMemcpyDeviceToHost, e->es));
  unsigned* h_ep = reinterpret_cast<unsigned*>(e->h_st + 3);
  HIPC(hipMemcpyAsync(h_ep, e->d_epoch, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, e->es));
  HIPC(hipStreamSynchronize(e->es));
  HIPC(hipGetLastError());
  if (h_ep[1] != 0) {  // a bounded spin of the sharded step ran out: its workgroups were not all resident (another process on the GPU?)
    const unsigned code = h_ep[1];
    HIPC(hipMemsetAsync(e->d_epoch + 1, 0, sizeof(unsigned), e->es));
    HIPC(hipStreamSynchronize(e->es));
    return fail(VX_ERR_STATE, "decode step: hand-over %u of the sharded decode step timed out (set VX_AR_TP=0)", code);
  }
  e->t_decode = ms;
  e->n_launch = (double)launched;
  e->n_gen = e->h_st[1].n_gen;
  e->stop_reason = e->h_st[1].stop_reason;
  e->n_pass = e->h_st[1].pass + 1;
  e->decoded = true;
  VXC(sync_out(e, stream));
  if (cap_limited && e->stop_reason == VX_STOP_MAX_NEW)
    return fail(VX_ERR_CAPACITY, "capacity exceeded: the KV cache filled (max_audio = %d rows: %d prompt + %d generated) before the stop rule fired; "
                "raise max_audio", c.max_audio, e->bos + e->P, e->n_gen);
  return VX_OK;
}

// n int32 tokens at `src` (device) into the caller's int64 buffer (nothing without one)
static int read_tokens(const int* src, int n, int64_t* tokens, int32_t capacity) {
  if (!tokens) return VX_OK;
  if (capacity < n) return fail(VX_ERR_CAPACITY, "token buffer too small (%d < %d)", capacity, n);
  std::vector<int> tmp(n);
  if (n) HIPC(hipMemcpy(tmp.data(), src, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) tokens[i] = tmp[i];
  return VX_OK;
}

extern "C" int vx_ar_result(vx_engine* e, int64_t* tokens, int32_t capacity, int32_t* n_tokens, int32_t* stop_reason,
                            int32_t* n_pass) {
  if (!e) return fail(VX_ERR_ARG, "null engine");
  if (!e->decoded) return fail(VX_ERR_STATE, "no finished decode");
  ON_DEVICE(e->cfg.device);
  if (n_tokens) *n_tokens = e->n_gen;
  if (stop_reason) *stop_reason = e->stop_reason;
  if (n_pass) *n_pass = e->n_pass;
  return read_tokens(e->d_tokens, e->n_gen, tokens, capacity);
}

// n fp32 values at `src` (device) into the caller's host buffer (nothing without one)
static int read_logprobs(const float* src, int n, float* out, int32_t capacity) {
  if (!out) return VX_OK;
  if (capacity < n) return fail(VX_ERR_CAPACITY, "log-probability buffer too small (%d < %d)", capacity, n);
  if (n) HIPC(hipMemcpy(out, src, (size_t)n * 4, hipMemcpyDeviceToHost));
  return VX_OK;
}

extern "C" int vx_ar_logprobs(vx_engine* e, float* out, int32_t capacity, int32_t* n) {
  if (!e) return fail(VX_ERR_ARG, "null engine");
  if (!e->lpon) return fail(VX_ERR_UNSUPPORTED, "vx_ar_logprobs needs an engine created with VX_FLAG_LOGPROBS");
  if (!e->decoded) return fail(VX_ERR_STATE, "no finished decode");
  ON_DEVICE(e->cfg.device);
  if (n) *n = e->n_pass;
  return read_logprobs(e->d_lp, e->n_pass, out, capacity);
}

// ------------------------------------------------------------------------------ batched AR decode
template <int EPI, int NH, bool KV8> static int launch_bgemm_h(const BgemmArgs& a, int ns, int grid, hipStream_t s) {
  if (a.N > 65535 || a.K > 65535) return fail(VX_ERR_UNSUPPORTED, "bgemm: N=%d K=%d", a.N, a.K);  // (N << 16) | K travels as one argument
  const unsigned nk = ((unsigned)a.N << 16) | (unsigned)a.K;
#define BG(NSV)                                                                       \
  if (ns == NSV) {                                                                    \
    bgemm_kernel<EPI, NSV, NH, KV8><<<grid, 256, 0, s>>>(a.A, a.W, nk, a.kgroups, a); \
    return VX_OK;                                                                     \
  }
  BG(1) BG(2) BG(4) BG(8)
#undef BG
  return fail(VX_ERR_UNSUPPORTED, "bgemm: %d steps per wave", ns);
}
// KV8 (BE_QKV only): write the fp8 slot caches a.kv8 / a.kv8s
template <int EPI, bool KV8> static int launch_bgemm(const BgemmArgs& a, hipStream_t s) {
  const int ns = a.K / (a.kgroups * 128);
  const int grid = ((a.N + 15) / 16) * a.kgroups;
  if (ns * a.kgroups * 128 != a.K) return fail(VX_ERR_UNSUPPORTED, "bgemm: K=%d kgroups=%d", a.K, a.kgroups);
  // two 16-slot MFMA halves up to 32 slots, four up to 64
  return a.B <= 32 ? launch_bgemm_h<EPI, 2, KV8>(a, ns, grid, s) : launch_bgemm_h<EPI, 4, KV8>(a, ns, grid, s);
}
template <int EPI> static int launch_bgemm(const BgemmArgs& a, hipStream_t s) { return launch_bgemm<EPI, false>(a, s); }
static int kgroups_for(int K) { return (K / 128) >= 4 ? 4 : 1; }
static void launch_ln_batch(float* x, const float* part, int kgroups, const float* pbias, const float* gamma, const float* beta,
                            bf16* h, int B, int d, hipStream_t s) {
  if (part == nullptr) ln_batch_kernel<0><<<B, 256, 0, s>>>(x, nullptr, nullptr, gamma, beta, h, d);
  else if (kgroups == 4) ln_batch_kernel<4><<<B, 256, 0, s>>>(x, part, pbias, gamma, beta, h, d);
  else ln_batch_kernel<1><<<B, 256, 0, s>>>(x, part, pbias, gamma, beta, h, d);
}

// One batched step: every slot samples its next token, then the L layers run once over all B slots.  VALL-F (pre-norm,
// TransformerDecoderLayer as in enqueue_ar_step): the self-attention cache holds audio rows only (kv_text = 0), and each layer
// adds the cross-attention over the slot's text memory (bmem) between the self-attention and the feed-forward block: 11 launches
// per layer instead of 7.
static int enqueue_batch_step(vx_engine* e, int B, hipStream_t s) {
  const vx_config& c = e->cfg;
  const int d = c.d_model, H = c.nhead, hd = 64, L = c.num_layers;
  SampleArgs sa{};
  sa.logits = e->blogits; sa.V = AR_VOCAB; sa.st = e->bst;
  sa.tokens = e->btok; sa.sampled = e->bsamp; sa.argmaxes = e->bargm;
  sa.emb = W<float>(e, "ar_audio_embedding.word_embeddings.weight");
  sa.alpha = W<float>(e, "ar_audio_position.alpha");
  sa.pe = e->pe_ar; sa.x = e->bx; sa.d = d;
  sa.logits_stride = LOGITS_CUR; sa.tok_stride = e->btok_stride;
  if (e->lpon) launch_sample_lp(sa, e->blp, NUM_AUDIO_TOKENS, B, s);
  else sample_embed4_kernel<5, 17><<<B, 256, 0, s>>>(sa);
  const size_t kv_layer = (size_t)2 * H * e->ctx_max * hd;  // elements
  const float scale = 1.0f / sqrtf((float)hd);
  const int kg_d = kgroups_for(d), kg_ff = kgroups_for(4 * d);
  // no warm-up of a later GEMM's weights as in the batch-1 step: at 32 slots it measured 528-531 us per step against 524-526
  // without (profiles/r02_ab_batch_prefetch.log) - between two GEMMs of the batched step sit an attention kernel that streams
  // 87 MB of K / V and the LayerNorm, and the memory system is not idle as in the batch-1 step.
  for (int li = 0; li < L; ++li) {
    const LayerW& l = e->ar_l[li];
    // LN1 (+ the FFN2 partial sums of the previous layer)
    const bool prev = li > 0;
    launch_ln_batch(e->bx, prev ? e->bpart : nullptr, kg_ff, prev ? e->ar_l[li - 1].b2 : nullptr, l.n1_g, l.n1_b, e->bh, B, d, s);
    BgemmArgs a{};
    a.st = e->bst; a.B = B; a.d = d; a.hd = hd; a.ctx_max = e->ctx_max;
    a.A = e->bh; a.W = (const bf16*)l.in_w; a.bias = l.in_b; a.N = 3 * d; a.K = d; a.kgroups = 1;
    a.q = e->bq; a.kv_slot_stride = e->bkv_slot; a.kv_v_offset = kv_layer / 2;
    if (e->kv8) {
      a.kv8 = e->bkv8 + (size_t)li * kv_layer; a.kv8s = e->bkv8s + (size_t)li * kv_layer / 16;
      VXC((launch_bgemm<BE_QKV, true>(a, s)));
      attn_batch8_kernel<64><<<dim3(H, B), 256, 0, s>>>(e->bq, a.kv8, a.kv8s, e->bkv_slot, kv_layer / 2, e->bst, e->ctx_max, d,
                                                        scale, e->batt);
    } else {
      a.kv = e->bkv + (size_t)li * kv_layer;
      VXC(launch_bgemm<BE_QKV>(a, s));
      attn_batch_kernel<64><<<dim3(H, B), 256, 0, s>>>(e->bq, e->bkv + (size_t)li * kv_layer, e->bkv_slot, kv_layer / 2, e->bst,
                                                       e->ctx_max, d, scale, e->batt);
    }
    BgemmArgs o{};
    o.st = e->bst; o.B = B;
    o.A = e->batt; o.W = (const bf16*)l.out_w; o.N = d; o.K = d; o.kgroups = kg_d; o.part = e->bpart;
    VXC(launch_bgemm<BE_PARTIAL>(o, s));
    launch_ln_batch(e->bx, e->bpart, kg_d, l.out_b, l.n2_g, l.n2_b, e->bh, B, d, s);
    if (e->vallf) {  // q = in_proj[0:d](norm2(x)); x += out_proj(attention over the text memory); then norm3 for the FFN
      const size_t mem_layer = (size_t)2 * d * c.max_text;  // elements
      BgemmArgs cq{};
      cq.st = e->bst; cq.B = B;
      cq.A = e->bh; cq.W = (const bf16*)l.cin_w; cq.bias = l.cin_b; cq.N = d; cq.K = d; cq.kgroups = 1; cq.q = e->bq;
      VXC(launch_bgemm<BE_BIAS>(cq, s));
      attn_batch_kernel<64, true><<<dim3(H, B), 256, 0, s>>>(e->bq, e->bmem + (size_t)li * mem_layer, e->bmem_slot, mem_layer / 2, e->bst,
                                                             c.max_text, d, scale, e->batt);
      BgemmArgs co{};
      co.st = e->bst; co.B = B;
      co.A = e->batt; co.W = (const bf16*)l.cout_w; co.N = d; co.K = d; co.kgroups = kg_d; co.part = e->bpart;
      VXC(launch_bgemm<BE_PARTIAL>(co, s));
      launch_ln_batch(e->bx, e->bpart, kg_d, l.cout_b, l.n3_g, l.n3_b, e->bh, B, d, s);
    }
    BgemmArgs f{};
    f.st = e->bst; f.B = B;
    f.A = e->bh; f.W = (const bf16*)l.w1; f.bias = l.b1; f.N = 4 * d; f.K = d; f.kgroups = 1; f.f = e->bff;
    VXC(launch_bgemm<BE_RELU>(f, s));
    BgemmArgs g{};
    g.st = e->bst; g.B = B;
    g.A = e->bff; g.W = (const bf16*)l.w2; g.N = d; g.K = 4 * d; g.kgroups = kg_ff; g.part = e->bpart;
    VXC(launch_bgemm<BE_PARTIAL>(g, s));
  }
  launch_ln_batch(e->bx, e->bpart, kg_ff, e->ar_l[L - 1].b2, W<float>(e, "ar_decoder.norm.weight"),
                  W<float>(e, "ar_decoder.norm.bias"), e->bh, B, d, s);
  BgemmArgs hgm{};
  hgm.st = e->bst; hgm.B = B;
  hgm.A = e->bh; hgm.W = W<bf16>(e, "ar_predict_layer.weight"); hgm.N = AR_VOCAB; hgm.K = d; hgm.kgroups = 1;
  hgm.logits = e->blogits; hgm.logits_stride = LOGITS_CUR;
  hgm.trace = e->btrace; hgm.trace_rows = e->btok_stride;
  VXC(launch_bgemm<BE_LOGITS>(hgm, s));
  return VX_OK;
}

// Decode parameters into the slot's staging state (its prefill fields are already there).
static void batch_params_stage(vx_engine* e, int slot, const vx_decode_params& p, bool cap_limited, long long room) {
  ArState& st = e->h_bst[slot];
  st.top_k = p.top_k; st.temperature = p.temperature; st.max_new = cap_limited ? (int)room : p.max_new_tokens;
  st.top_p = state_top_p(p.top_p);
  st.exp_noise = p.exp_noise; st.noise_rows = p.noise_rows; st.seed = p.seed;
  st.forced = p.forced ? (p.n_forced > 0 ? (const long long*)p.forced : (const long long*)e->btok) : nullptr;
  st.n_forced = p.forced ? p.n_forced : 0;
}

// Replays the B-slot step until min_stopped live slots (all of them, if fewer are live) have stopped and lists those in
// stopped[0 .. *n_stopped).  Slot b < B is vacant, live or stopped by bslot[b]; a live slot may take bleft[b] more steps.  A
// stopped slot keeps the n_gen / stop_reason of the poll that first saw it done: the sampler skips a done slot, so they are final.
static int run_slots(vx_engine* e, int B, int min_stopped, int chunk, int32_t* stopped, int32_t* n_stopped) {
  *n_stopped = 0;
  long long bound = 0;  // steps until every live slot has exhausted its bound
  int live = 0;
  for (int b = 0; b < B; ++b)
    if (e->bslot[b] == SLOT_LIVE) { ++live; if (e->bleft[b] > bound) bound = e->bleft[b]; }
  if (live == 0) return VX_OK;
  auto step = [e, B](hipStream_t s) { return enqueue_batch_step(e, B, s); };
  hipGraphExec_t& gx = e->bgraphs[B];
  VXC(step_graph(e, &gx, step));
  int found = 0;
  // every live slot that has stopped is reported; a live slot past its bound that has not is an error
  auto take = [&](const ArState* hs, long long at) -> int {
    for (int b = 0; b < B; ++b) {
      if (e->bslot[b] != SLOT_LIVE) continue;
      if (hs[b].done) {
        e->bslot[b] = SLOT_STOPPED;
        e->bngen[b] = hs[b].n_gen; e->breason[b] = hs[b].stop_reason;
        e->bnpass[b] = hs[b].pass + 1;
        stopped[found++] = b;
        --live;
      } else if (at >= e->bleft[b]) {
        return fail(VX_ERR_STATE, "batched decode of slot %d did not terminate within %lld steps", b, e->bleft[b]);
      }
    }
    return found >= min_stopped || live == 0 ? POLL_STOP : POLL_MORE;
  };
  ArState* const poll[2] = {e->h_bst + BMAX, e->h_bst + 2 * BMAX};
  long long launched = 0;
  float ms = 0.f;
  VXC(replay_polled(e, gx, step, bound, chunk, e->bst, B, poll, take, &launched, &ms));
  e->t_bdecode = ms;
  e->n_blaunch = (double)launched;
  for (int b = 0; b < B; ++b)
    if (e->bslot[b] == SLOT_LIVE) e->bleft[b] -= launched;
  *n_stopped = found;
  return VX_OK;
}

extern "C" int vx_batch_decode(vx_engine* e, int32_t B, const vx_decode_params* params, void* stream) {
  if (!e || !params) return fail(VX_ERR_ARG, "null argument");
  if (B < 1 || B > e->bmax) return fail(VX_ERR_ARG, "n_slots %d outside [1, max_batch=%d]", B, e->bmax);
  for (int b = 0; b < B; ++b) {  // the parameter checks that need no slot state, before any HIP call
    if (params[b].struct_size != (int32_t)sizeof(vx_decode_params)) return fail(VX_ERR_ARG, "vx_decode_params.struct_size mismatch");
    VXC(check_top_p(params[b].top_p));
  }
  const vx_config& c = e->cfg;
  ON_DEVICE(c.device);
  e->bsess = false;  // the static calls end a continuous-batching session
  for (int b = 0; b < B; ++b) {
    const vx_decode_params& p = params[b];
    if (p.struct_size != (int32_t)sizeof(vx_decode_params)) return fail(VX_ERR_ARG, "vx_decode_params.struct_size mismatch");
    if (!e->bprefilled[b]) return fail(VX_ERR_STATE, "slot %d needs a fresh vx_batch_prefill", b);
    long long room = 0;
    VXC(decode_bound(e, b, p, e->bS[b], e->bP[b], e->bbos[b], &e->bleft[b], &e->bcap[b], &room));
    batch_params_stage(e, b, p, e->bcap[b], room);
    if (p.exp_noise && p.noise_rows <= 0) return fail(VX_ERR_ARG, "noise_rows must be > 0");
  }
  for (int b = 0; b < e->bmax; ++b) e->bslot[b] = b < B ? SLOT_LIVE : SLOT_VACANT;
  VXC(sync_in(e, stream));
  HIPC(hipMemcpyAsync(e->bst, e->h_bst, (size_t)B * sizeof(ArState), hipMemcpyHostToDevice, e->es));
  int32_t stopped[BMAX], n_stopped = 0;
  VXC(run_slots(e, B, B, POLL_CHUNK, stopped, &n_stopped));
  for (int b = 0; b < B; ++b) e->bprefilled[b] = false;
  VXC(sync_out(e, stream));
  for (int b = 0; b < B; ++b)
    if (e->bcap[b] && e->breason[b] == VX_STOP_MAX_NEW)
      return fail(VX_ERR_CAPACITY, "capacity exceeded in slot %d: the KV cache filled (max_audio = %d rows) before the stop rule fired; raise max_audio", b, c.max_audio);
  return VX_OK;
}

extern "C" int vx_batch_result(vx_engine* e, int32_t slot, int64_t* tokens, int32_t capacity, int32_t* n_tokens,
                               int32_t* stop_reason) {
  if (!e) return fail(VX_ERR_ARG, "null engine");
  if (slot < 0 || slot >= e->bmax) return fail(VX_ERR_ARG, "bad slot");
  if (e->bsess && e->bslot[slot] == SLOT_LIVE) return fail(VX_ERR_STATE, "slot %d is still decoding", slot);
  ON_DEVICE(e->cfg.device);
  const int n = e->bngen[slot];
  if (n_tokens) *n_tokens = n;
  if (stop_reason) *stop_reason = e->breason[slot];
  VXC(read_tokens(e->btok + (size_t)slot * e->btok_stride, n, tokens, capacity));
  if (e->bsess && e->bslot[slot] == SLOT_STOPPED) e->bslot[slot] = SLOT_VACANT;  // read: the slot may be admitted into again
  return VX_OK;
}

// The log-probabilities of a slot's decode.  A session's slot must be STOPPED (vx_batch_result vacates it); after vx_batch_decode
// every decoded slot answers until it is prefilled again.
extern "C" int vx_batch_logprobs(vx_engine* e, int32_t slot, float* out, int32_t capacity, int32_t* n) {
  if (!e) return fail(VX_ERR_ARG, "null engine");
  if (!e->lpon) return fail(VX_ERR_UNSUPPORTED, "vx_batch_logprobs needs an engine created with VX_FLAG_LOGPROBS");
  if (slot < 0 || slot >= e->bmax) return fail(VX_ERR_ARG, "bad slot");
  if (e->bsess && e->bslot[slot] != SLOT_STOPPED) return fail(VX_ERR_STATE, "slot %d holds no finished, unread decode", slot);
  if (e->bnpass[slot] <= 0) return fail(VX_ERR_STATE, "slot %d has no finished decode", slot);
  ON_DEVICE(e->cfg.device);
  if (n) *n = e->bnpass[slot];
  return read_logprobs(e->blp + (size_t)slot * e->btok_stride, e->bnpass[slot], out, capacity);
}

// ------------------------------------------------------------------------------ continuous batching
// A session over all max_batch slots: every slot is vacant, live (admitted, decoding) or stopped (its result not read yet).  The
// step always runs at B = max_batch (one graph, shared with vx_batch_decode); vacant and stopped slots have done = 1, so the
// sampler, the K / V append, the attention and the logits skip them and their rows of the shared GEMMs are ignored.
extern "C" int vx_batch_open(vx_engine* e, void* stream) {
  if (!e) return fail(VX_ERR_ARG, "null engine");
  if (e->bmax < 2) return fail(VX_ERR_UNSUPPORTED, "continuous batching needs an engine created with max_batch >= 2");
  if (!e->finalized) return fail(VX_ERR_STATE, "weights not finalized");
  const int d = e->cfg.d_model;
  ON_DEVICE(e->cfg.device);
  VXC(sync_in(e, stream));
  for (int b = 0; b < e->bmax; ++b) {
    seed_state(e->h_bst[b], 0, 0, 0, 0, 0, false);
    e->h_bst[b].done = 1;
  }
  HIPC(hipMemcpyAsync(e->bst, e->h_bst, (size_t)e->bmax * sizeof(ArState), hipMemcpyHostToDevice, e->es));
  // a vacant slot's rows still go through the step's GEMMs and LayerNorms: they must hold finite values
  HIPC(hipMemsetAsync(e->bx, 0, (size_t)e->bmax * d * 4, e->es));
  HIPC(hipMemsetAsync(e->blogits, 0, (size_t)e->bmax * LOGITS_CUR * 4, e->es));
  HIPC(hipStreamSynchronize(e->es));  // the staging states are rewritten by the next admission
  for (int b = 0; b < e->bmax; ++b) {
    e->bslot[b] = SLOT_VACANT; e->bleft[b] = 0; e->bcap[b] = false;
    e->bprefilled[b] = false; e->bngen[b] = 0; e->breason[b] = 0; e->bnpass[b] = 0;
  }
  e->bsess = true;
  VXC(sync_out(e, stream));
  return VX_OK;
}

extern "C" int vx_batch_admit(vx_engine* e, int32_t n, const int32_t* slots, const int64_t* const* text, const int32_t* S,
                              const int64_t* const* prompt_cb0, const int32_t* P, const vx_decode_params* params, int32_t mode,
                              void* stream) {
  if (!e || !slots || !text || !S || !prompt_cb0 || !P || !params) return fail(VX_ERR_ARG, "null argument");
  if (!e->bsess) return fail(VX_ERR_STATE, "vx_batch_admit needs an open session (vx_batch_open)");
  if (!e->finalized) return fail(VX_ERR_STATE, "weights not finalized");
  if (n < 1 || n > e->bmax) return fail(VX_ERR_ARG, "n %d outside [1, max_batch=%d]", n, e->bmax);
  if (mode != VX_ADMIT_BATCHED && mode != VX_ADMIT_PER_SLOT) return fail(VX_ERR_ARG, "unknown admission mode %d", mode);
  if (mode == VX_ADMIT_BATCHED && !use_mfma(e)) return fail(VX_ERR_UNSUPPORTED, "batched admission needs the bf16 MFMA row kernels");
  if (mode == VX_ADMIT_BATCHED && e->vallf && !e->vf_rows) return fail(VX_ERR_UNSUPPORTED, "batched admission: VALL-F admits slot by slot (VX_ADMIT_PER_SLOT)");
  const vx_config& c = e->cfg;
  const int bos = c.prepend_bos ? 1 : 0;
  // every check before anything is written: a refused admission leaves all slots as they were
  bool seen[BMAX] = {};
  for (int z = 0; z < n; ++z) {
    const int sl = slots[z];
    if (sl < 0 || sl >= e->bmax) return fail(VX_ERR_ARG, "slot %d outside [0, max_batch=%d)", sl, e->bmax);
    if (seen[sl]) return fail(VX_ERR_ARG, "slot %d admitted twice", sl);
    seen[sl] = true;
    if (e->bslot[sl] == SLOT_LIVE) return fail(VX_ERR_STATE, "slot %d is live", sl);
    if (e->bslot[sl] == SLOT_STOPPED) return fail(VX_ERR_STATE, "slot %d has stopped but its result was not read", sl);
  }
  long long steps[BMAX] = {}, room[BMAX] = {};
  bool capl[BMAX] = {};
  for (int z = 0; z < n; ++z) {
    if (mode == VX_ADMIT_BATCHED && e->vallf && S[z] > c.max_text)
      return fail(VX_ERR_CAPACITY, "utterance %d: a text of %d tokens exceeds max_text=%d", z, S[z], c.max_text);
    VXC(check_utterance(e, text[z], S[z], prompt_cb0[z], P[z], z));
    const vx_decode_params& p = params[z];
    VXC(decode_bound(e, slots[z], p, S[z], P[z], bos, &steps[z], &capl[z], &room[z]));
    if (p.exp_noise && p.noise_rows <= 0) return fail(VX_ERR_ARG, "noise_rows must be > 0");
  }
  ON_DEVICE(c.device);
  if (mode == VX_ADMIT_PER_SLOT) {  // prefill_impl touches only its slot (and synchronises the engine stream per call)
    for (int z = 0; z < n; ++z) VXC(prefill_impl(e, slots[z], text[z], S[z], prompt_cb0[z], P[z], stream));
  } else {
    VXC(batch_prefill_impl(e, n, slots, text, S, prompt_cb0, P, stream));
  }
  // arm: the prefill left each slot's state in h_bst[slot] and synchronised; add the decode parameters
  VXC(sync_in(e, stream));
  for (int z = 0; z < n; ++z) {
    const int sl = slots[z];
    batch_params_stage(e, sl, params[z], capl[z], room[z]);
    HIPC(hipMemcpyAsync(e->bst + sl, &e->h_bst[sl], sizeof(ArState), hipMemcpyHostToDevice, e->es));
    e->bslot[sl] = SLOT_LIVE; e->bleft[sl] = steps[z]; e->bcap[sl] = capl[z];
    e->bprefilled[sl] = false;
  }
  VXC(sync_out(e, stream));
  return VX_OK;
}

extern "C" int vx_batch_run(vx_engine* e, int32_t min_stopped, int32_t poll_steps, int32_t* stopped, int32_t* n_stopped,
                            void* stream) {
  if (!e) return fail(VX_ERR_ARG, "null engine");
  if (!e->bsess) return fail(VX_ERR_STATE, "vx_batch_run needs an open session (vx_batch_open)");
  if (!stopped || !n_stopped) return fail(VX_ERR_ARG, "null argument");
  *n_stopped = 0;
  ON_DEVICE(e->cfg.device);
  VXC(sync_in(e, stream));
  VXC(run_slots(e, e->bmax, min_stopped < 1 ? 1 : min_stopped, poll_steps > 0 ? poll_steps : BATCH_POLL_DEFAULT, stopped, n_stopped));
  VXC(sync_out(e, stream));
  for (int i = 0; i < *n_stopped; ++i) {
    const int b = stopped[i];
    if (e->bcap[b] && e->breason[b] == VX_STOP_MAX_NEW)
      return fail(VX_ERR_CAPACITY, "capacity exceeded in slot %d: the KV cache filled (max_audio = %d rows) before the stop rule fired; raise max_audio", b, e->cfg.max_audio);
  }
  return VX_OK;
}

// ------------------------------------------------------------------------------ NAR
// The NAR stages (valle.py:1063-1134) of n utterances, checked by the caller: text_nar[b] (S2[b] ids), prompts[b] ((P[b], Q)
// codes) and ar_tokens[b] (T[b] codes of codebook 0) -> codes_out[b] ((T[b], Q)).  segmented: the rows of all utterances are
// concatenated (seg_layout), so the GEMMs run at M ~ n x 1k rows where the MFMA kernels are efficient and attention runs per
// segment in one launch; otherwise n == 1 and its rows start at 0, unpadded.
// forced (optional, (T, Q) each): stage i's argmax is still what codes_out reports, but the embedding that feeds stage i+1 is
// taken from forced[:, i+1] - the input the reference itself gave that stage when `forced` are its codes (valle.py:1133-1134).
// Unsegmented only: prenets, VALL-F, pos_before_prenet (VALLE.continual) and stage_logits ((Q-1, T, 1024) fp32, host or
// device: every stage's logits rows, valle.py:1128).
// Scoring outputs of nar_run (vx_score): per utterance (Q-1, T_b) arrays, host or device; either may be null.  Needs `forced`:
// stage i's rows are scored against forced[:, i+1] (valle.py:886-950 at the inference prompt layout).  The caller has reserved
// e->sc_* for sum(T) rows.
struct NarScore { float* const* nll; int32_t* const* rank; };
static int nar_run(vx_engine* e, int n, bool segmented, const int64_t* const* text_nar, const int32_t* S2,
                   const int64_t* const* prompts, const int32_t* P, const int64_t* const* ar_tokens, const int32_t* T,
                   int64_t* const* codes_out, const int64_t* const* forced, void* stream, bool pos_before_prenet = false,
                   float* stage_logits = nullptr, const NarScore* score = nullptr) {
  const vx_config& c = e->cfg;
  const int Q = c.num_quantizers, dn = c.nar_d_model;
  const bool vf = e->vallf, prenet = c.flags & VX_FLAG_PRENET, post = c.flags & VX_FLAG_POST_NORM;
  // per utterance: its rows in X, tx = text rows in front of its audio rows (VALL-F, valle.py:650-708: the stack runs over the
  // audio rows, the NAR text is cross-attention memory), its offsets into the audio / generated / text id staging
  std::vector<int> start(n + 1), len(n), tx(n), aoff(n), toff(n), soff(n);
  std::vector<long long> moff(n);  // VALL-F, segmented: each segment's text memory (uploaded asynchronously: lives until the final sync)
  int arows = 0, trows = 0, srows = 0;
  for (int b = 0; b < n; ++b) {
    tx[b] = vf ? 0 : S2[b];
    len[b] = tx[b] + P[b] + T[b];
    aoff[b] = arows; toff[b] = trows; soff[b] = srows;
    arows += P[b] + T[b]; trows += T[b]; srows += S2[b];
  }
  ON_DEVICE(c.device);
  if (e->lpon && !score) { e->nlp_off.clear(); e->nlp_T.clear(); }  // nar_lp is about to be overwritten: a call that fails leaves none
  VXC(sync_in(e, stream));
  HIPC(hipEventRecord(e->ev_t[4], e->es));
  RowSegs segs;
  if (segmented) VXC(seg_layout(e, n, len.data(), nullptr, nullptr, dn, arows, srows, start.data(), segs, vf ? srows : 0));
  else start[1] = len[0];
  const int rows = start[n];
  auto emb = [&](int j) { return W<float>(e, "nar_audio_embeddings." + std::to_string(j) + ".word_embeddings.weight"); };
  for (int b = 0; b < n; ++b) {  // y = [prompt codebook 0 | AR tokens] (valle.py:1064-1066)
    long long* idp = e->ids_prompts + (size_t)aoff[b] * Q;  // (P_b, Q) rows; region sized for P+T rows per utterance
    long long* ids = e->ids_samples + toff[b];
    float* ye = e->yemb + (size_t)aoff[b] * dn;
    if (P[b]) HIPC(hipMemcpyAsync(idp, prompts[b], (size_t)P[b] * Q * 8, hipMemcpyDefault, e->es));
    HIPC(hipMemcpyAsync(ids, ar_tokens[b], (size_t)T[b] * 8, hipMemcpyDefault, e->es));
    copy_col_kernel<<<(T[b] + 255) / 256, 256, 0, e->es>>>(ids, e->d_codes + (size_t)toff[b] * Q, T[b], Q, 0);
    if (forced) HIPC(hipMemcpyAsync(e->d_fcodes + (size_t)toff[b] * Q, forced[b], (size_t)T[b] * Q * 8, hipMemcpyDefault, e->es));
    if (Q == 1) continue;
    HIPC(hipMemcpyAsync(e->ids_text + soff[b], text_nar[b], (size_t)S2[b] * 8, hipMemcpyDefault, e->es));
    if (P[b]) embed_accum_kernel<<<P[b], 256, 0, e->es>>>(idp, Q, 0, emb(0), 1025, dn, ye, P[b], 1);
    embed_accum_kernel<<<T[b], 256, 0, e->es>>>(ids, 1, 0, emb(0), 1025, dn, ye + (size_t)P[b] * dn, T[b], 1);
    if (c.prefix_mode != 0 && P[b])  // valle.py:1110-1113
      for (int j = 1; j < Q; ++j) embed_accum_kernel<<<P[b], 256, 0, e->es>>>(idp, Q, j, emb(j), 1024, dn, ye, P[b], 0);
  }
  if (Q > 1) {
    const float* a_txt = W<float>(e, "nar_text_position.alpha");
    const float* a_aud = W<float>(e, "nar_audio_position.alpha");
    if (prenet) {  // x = position(nar_text_prenet(embedding)) once (valle.py:1081-1083); kept in pn_text for every stage
      embed_accum_kernel<<<S2[0], 256, 0, e->es>>>(e->ids_text, 1, 0, W<float>(e, "nar_text_embedding.word_embeddings.weight"), 512, dn, e->pn_a, S2[0], 1);
      VXC(text_prenet_rows(e, 1, e->pn_a, e->pn_a, S2[0], dn));
      add_pos_kernel<<<S2[0], 256, 0, e->es>>>(e->pn_a, dn, a_txt, e->pe_nar, 0, e->pn_text, S2[0]);
    }
    // segmented VALL-F (VX_FLAG_VALLF_ROWS): all segments' text rows, concatenated without padding in rows [0, sum S2) of X, become
    // the packed memory xmem_rows (segment b's keys at text row soff[b] of every head) - once for all seven stages.  X is zeroed
    // again afterwards: the stages write the audio rows only and the padding rows between segments stay as seg_layout left them.
    TextMem tmem;
    if (vf && segmented) {
      for (int b = 0; b < n; ++b) {
        moff[b] = (long long)soff[b] * 64;
        embed_pos_kernel<<<S2[b], 256, 0, e->es>>>(e->ids_text + soff[b], 1, 0, W<float>(e, "nar_text_embedding.word_embeddings.weight"), 512, dn,
                                                   a_txt, e->pe_nar, 0, e->X + (size_t)soff[b] * dn, S2[b]);
      }
      VXC(cast_rows(e, e->X, e->Hn, (size_t)srows * dn));
      tmem.kv = e->xmem_rows; tmem.off = e->d_mem_off; tmem.klen = e->d_mem_klen;
      tmem.head_stride = (long long)e->cap_text * 64; tmem.v_offset = (long long)e->cap_text * dn; tmem.layer_stride = 2 * tmem.v_offset;
      VXC(memory_kv_segs(e, e->nar_l, tmem, n, moff.data(), S2, soff.data(), srows, dn));
      HIPC(hipMemsetAsync(e->X, 0, (size_t)rows * dn * 4, e->es));
    } else if (vf) {  // the text memory's K / V per layer, once for all stages (same memory and weights in every stage, valle.py:664-688)
      tmem = TextMem{e->xkv_nar, S2[0]};
      if (prenet) HIPC(hipMemcpyAsync(e->X, e->pn_text, (size_t)S2[0] * dn * 4, hipMemcpyDeviceToDevice, e->es));
      else embed_pos_kernel<<<S2[0], 256, 0, e->es>>>(e->ids_text, 1, 0, W<float>(e, "nar_text_embedding.word_embeddings.weight"), 512, dn,
                                                      a_txt, e->pe_nar, 0, e->X, S2[0]);
      VXC(cast_rows(e, e->X, e->Hn, (size_t)S2[0] * dn));
      VXC(memory_kv(e, e->nar_l, e->xkv_nar, S2[0], dn, c.nar_nhead));
    }
    for (int i = 0; i < Q - 1; ++i) {
      for (int b = 0; b < n; ++b) {
        float* xb = e->X + (size_t)start[b] * dn;
        float* xa = xb + (size_t)tx[b] * dn;  // the audio rows
        const float* ye = e->yemb + (size_t)aoff[b] * dn;
        const int A = P[b] + T[b];
        if (prenet) {
          if (!vf) HIPC(hipMemcpyAsync(xb, e->pn_text, (size_t)S2[b] * dn * 4, hipMemcpyDeviceToDevice, e->es));
          if (pos_before_prenet) {  // VALLE.continual, prefix mode 0 (valle.py:1193-1194)
            add_pos_kernel<<<A, 256, 0, e->es>>>(ye, dn, a_aud, e->pe_nar, 0, e->pn_a, A);
            VXC(audio_prenet_rows(e, 1, e->pn_a, xa, A, dn));
          } else {  // valle.py:1092-1093, 1121-1122
            VXC(audio_prenet_rows(e, 1, ye, e->pn_b, A, dn));
            add_pos_kernel<<<A, 256, 0, e->es>>>(e->pn_b, dn, a_aud, e->pe_nar, 0, xa, A);
          }
        } else {
          if (!vf) embed_pos_kernel<<<S2[b], 256, 0, e->es>>>(e->ids_text + soff[b], 1, 0, W<float>(e, "nar_text_embedding.word_embeddings.weight"),
                                                              512, dn, a_txt, e->pe_nar, 0, xb, S2[b]);
          add_pos_kernel<<<A, 256, 0, e->es>>>(ye, dn, a_aud, e->pe_nar, 0, xa, A);
        }
      }
      VXC(run_stack(e, e->nar_l, rows, dn, c.nar_nhead, -1, i, segs, KvDst(), tmem));
      // final AdaLN + predict layer on the generated rows only (valle.py:1128), compacted to [sum T][dn]
      const float* fw = post ? nullptr : ada_vec(e, i, e->npl * c.nar_num_layers);
      for (int b = 0; b < n; ++b) {
        const float* xr = e->X + (size_t)(start[b] + tx[b] + P[b]) * dn;
        void* hr = (char*)e->Hn + (size_t)toff[b] * dn * e->esz;
        if (post) VXC(cast_rows(e, xr, hr, (size_t)T[b] * dn));  // no final norm (valle.py:242-246): the rows are already norm2'd
        else VXC(ln_rows(e, xr, W<float>(e, "nar_decoder.norm.norm.weight"), W<float>(e, "nar_decoder.norm.norm.bias"), fw, fw + dn, hr,
                         T[b], dn));
      }
      VXC(gemm_rows(e, e->Hn, W<void>(e, "nar_predict_layers." + std::to_string(i) + ".weight"), nullptr, e->nar_logits,
                    trows, 1024, dn, GE_PLAIN, true));
      if (e->lpon && !score)  // VX_FLAG_LOGPROBS: the same argmax, and the log-probability of the picked code per row
        launch_argmax_lp_rows(e->nar_logits, trows, e->ids_samples, e->d_codes, Q, i + 1, e->nar_lp + (size_t)i * trows, e->es);
      else
        argmax_rows_kernel<<<(trows + 3) / 4, 256, 0, e->es>>>(e->nar_logits, 1024, trows, e->ids_samples, e->d_codes, Q, i + 1);
      if (score) {
        nll_rows_kernel<<<(trows + NLL_ROWS_PER_WG - 1) / NLL_ROWS_PER_WG, 256, 0, e->es>>>(e->nar_logits, trows, 1024, 1024, e->d_fcodes, Q, i + 1,
                                                                                   e->sc_nll, e->sc_rank, nullptr);
        for (int b = 0; b < n; ++b) {
          if (score->nll) HIPC(hipMemcpyAsync(score->nll[b] + (size_t)i * T[b], e->sc_nll + toff[b], (size_t)T[b] * 4, hipMemcpyDefault, e->es));
          if (score->rank) HIPC(hipMemcpyAsync(score->rank[b] + (size_t)i * T[b], e->sc_rank + toff[b], (size_t)T[b] * 4, hipMemcpyDefault, e->es));
        }
      }
      if (stage_logits) HIPC(hipMemcpyAsync(stage_logits + (size_t)i * trows * 1024, e->nar_logits, (size_t)trows * 1024 * 4, hipMemcpyDefault, e->es));
      if (forced && i < Q - 2)  // teacher forcing: the next stage sees the caller's codes of this stage (all segments at once)
        pick_col_kernel<<<(trows + 255) / 256, 256, 0, e->es>>>(e->d_fcodes, Q, i + 1, e->ids_samples, trows);
      if (i < Q - 2)  // valle.py:1104-1108 / 1133-1134
        for (int b = 0; b < n; ++b) {
          float* ye = e->yemb + (size_t)aoff[b] * dn;
          if (c.prefix_mode == 0 && P[b])
            embed_accum_kernel<<<P[b], 256, 0, e->es>>>(e->ids_prompts + (size_t)aoff[b] * Q, Q, i + 1, emb(i + 1), 1024, dn, ye, P[b], 0);
          embed_accum_kernel<<<T[b], 256, 0, e->es>>>(e->ids_samples + toff[b], 1, 0, emb(i + 1), 1024, dn, ye + (size_t)P[b] * dn, T[b], 0);
        }
    }
  }
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(e->ev_t[5], e->es));
  for (int b = 0; codes_out && b < n; ++b)  // (scoring passes no codes_out)
    HIPC(hipMemcpyAsync(codes_out[b], e->d_codes + (size_t)toff[b] * Q, (size_t)T[b] * Q * 8, hipMemcpyDefault, e->es));
  HIPC(hipStreamSynchronize(e->es));
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, e->ev_t[4], e->ev_t[5]));
  e->t_nar = ms;
  gemm_collect(e);
  e->last_T = trows; e->last_N = rows;
  if (e->lpon && !score) {
    e->nlp_off.assign(toff.begin(), toff.end());
    e->nlp_T.assign(T, T + n);
    e->nlp_rows = trows;
  }
  VXC(sync_out(e, stream));
  return VX_OK;
}

extern "C" int vx_nar_logprobs(vx_engine* e, int32_t utt, float* out, int64_t capacity) {
  if (!e) return fail(VX_ERR_ARG, "null engine");
  if (!e->lpon) return fail(VX_ERR_UNSUPPORTED, "vx_nar_logprobs needs an engine created with VX_FLAG_LOGPROBS");
  if (e->nlp_T.empty()) return fail(VX_ERR_STATE, "no finished NAR call");
  if (utt < 0 || utt >= (int)e->nlp_T.size()) return fail(VX_ERR_ARG, "utterance %d outside the last NAR call's [0, %d)", utt, (int)e->nlp_T.size());
  if (!out) return fail(VX_ERR_ARG, "null argument");
  const int Q = e->cfg.num_quantizers, T = e->nlp_T[utt];
  if (capacity < (int64_t)(Q - 1) * T) return fail(VX_ERR_CAPACITY, "log-probability buffer too small (%lld < %lld)", (long long)capacity, (long long)(Q - 1) * T);
  ON_DEVICE(e->cfg.device);
  for (int i = 0; i < Q - 1; ++i)
    HIPC(hipMemcpyAsync(out + (size_t)i * T, e->nar_lp + (size_t)i * e->nlp_rows + e->nlp_off[utt], (size_t)T * 4, hipMemcpyDefault, e->es));
  HIPC(hipStreamSynchronize(e->es));
  return VX_OK;
}

extern "C" int vx_nar(vx_engine* e, const int64_t* text_nar, int32_t S2, const int64_t* prompts, int32_t P,
                      const int64_t* ar_tokens, int32_t T, int64_t* codes_out, void* stream) {
  return vx_nar_ex(e, text_nar, S2, prompts, P, ar_tokens, T, codes_out, nullptr, nullptr, 0, stream);
}

extern "C" int vx_nar_ex(vx_engine* e, const int64_t* text_nar, int32_t S2, const int64_t* prompts, int32_t P,
                         const int64_t* ar_tokens, int32_t T, int64_t* codes_out, const int64_t* forced_codes,
                         float* stage_logits, int32_t continual, void* stream) {
  if (!e || !text_nar || !ar_tokens || !codes_out || (P > 0 && !prompts)) return fail(VX_ERR_ARG, "null argument");
  if (!e->finalized) return fail(VX_ERR_STATE, "weights not finalized");
  const vx_config& c = e->cfg;
  if (S2 <= 0 || T <= 0 || P < 0) return fail(VX_ERR_ARG, "bad S2/P/T");
  if (S2 > c.max_text || P + T > c.max_audio) return fail(VX_ERR_CAPACITY, "S2=%d P+T=%d exceed capacity", S2, P + T);
  return nar_run(e, 1, false, &text_nar, &S2, &prompts, &P, &ar_tokens, &T, &codes_out, forced_codes ? &forced_codes : nullptr,
                 stream, continual && c.prefix_mode == 0, stage_logits);
}

extern "C" int vx_nar_continual(vx_engine* e, const int64_t* text_nar, int32_t S2, const int64_t* prompts, int32_t P,
                                const int64_t* ar_tokens, int32_t T, int64_t* codes_out, void* stream) {
  return vx_nar_ex(e, text_nar, S2, prompts, P, ar_tokens, T, codes_out, nullptr, nullptr, 1, stream);
}

// A grown buffer replaces *p (null: a first allocation); a caller that replaces a live one has drained e->es.  `allocs` owns it.
static int regrow(vx_engine* e, void** p, size_t bytes) {
  for (auto& q : e->allocs) if (*p && q == *p) { (void)hipFree(q); q = nullptr; }
  HIPC(hipMalloc(p, bytes));
  if (poison_on()) { HIPC(hipMemsetAsync(*p, 0xFF, bytes, e->es)); HIPC(hipStreamSynchronize(e->es)); }
  e->allocs.push_back(*p);
  return VX_OK;
}

// Row buffers are sized for one utterance at vx_create; the batched NAR concatenates up to max_batch of them.
static int ensure_rows(vx_engine* e, size_t rows, size_t audio_rows, size_t text_rows) {
  const vx_config& c = e->cfg;
  const size_t dmax = c.d_model > c.nar_d_model ? c.d_model : c.nar_d_model;
  if (rows <= (size_t)e->n_max && audio_rows <= e->cap_audio && text_rows <= e->cap_text) return VX_OK;
  if (rows < (size_t)e->n_max) rows = e->n_max;
  if (audio_rows < e->cap_audio) audio_rows = e->cap_audio;
  if (text_rows < e->cap_text) text_rows = e->cap_text;
  e->cap_audio = audio_rows; e->cap_text = text_rows;
  HIPC(hipStreamSynchronize(e->es));
  e->n_max = (int)rows;
  e->vt_ld = (int)(((rows + 63) / 64) * 64 + 64);
  VXC(regrow(e, (void**)&e->X, rows * dmax * 4));
  VXC(regrow(e, &e->Hn, rows * dmax * e->esz));
  VXC(regrow(e, &e->QKV, rows * 3 * dmax * e->esz));
  VXC(regrow(e, &e->ATT, rows * dmax * e->esz));
  HIPC(hipMemsetAsync(e->ATT, 0, rows * dmax * e->esz, e->es));  // padding rows between segments are never written: keep them finite
  VXC(regrow(e, &e->FF, rows * 4 * dmax * e->esz));
  VXC(regrow(e, &e->VT, dmax * (size_t)e->vt_ld * 2));
  HIPC(hipMemsetAsync(e->VT, 0, dmax * (size_t)e->vt_ld * 2, e->es));
  HIPC(hipMemsetAsync(e->X, 0, rows * dmax * 4, e->es));
  if (e->fp8nar) {
    e->mx_ld = (int)((rows + 255) / 256 * 256);
    VXC(regrow(e, (void**)&e->Hn8, rows * dmax));
    VXC(regrow(e, (void**)&e->FF8, rows * 4 * dmax));
    VXC(regrow(e, (void**)&e->SHn, (dmax / 32) * (size_t)e->mx_ld));
    VXC(regrow(e, (void**)&e->SFF, (4 * dmax / 32) * (size_t)e->mx_ld));
    HIPC(hipMemsetAsync(e->SHn, 0, (dmax / 32) * (size_t)e->mx_ld, e->es));
    HIPC(hipMemsetAsync(e->SFF, 0, (4 * dmax / 32) * (size_t)e->mx_ld, e->es));
  }
  if (e->slab != nullptr) {  // keep the split-K path available for concatenated rows below the 256^2 threshold
    e->slab_rows = rows < 4095 ? (int)rows : 4095;
    VXC(regrow(e, (void**)&e->slab, (size_t)4 * e->slab_rows * dmax * 4));
  }
  VXC(regrow(e, (void**)&e->yemb, audio_rows * dmax * 4));
  VXC(regrow(e, (void**)&e->nar_logits, audio_rows * 1024 * 4));
  VXC(regrow(e, (void**)&e->ids_text, text_rows * 8));
  VXC(regrow(e, (void**)&e->ids_prompts, audio_rows * 8 * 8));
  VXC(regrow(e, (void**)&e->ids_samples, audio_rows * 8));
  VXC(regrow(e, (void**)&e->d_codes, audio_rows * 8 * 8));
  VXC(regrow(e, (void**)&e->d_fcodes, audio_rows * 8 * 8));
  if (e->nar_lp != nullptr) {  // VX_FLAG_LOGPROBS; the last call's values do not survive the move
    VXC(regrow(e, (void**)&e->nar_lp, (size_t)(c.num_quantizers - 1) * audio_rows * 4));
    e->nlp_off.clear(); e->nlp_T.clear();
  }
  if (e->xmem_rows != nullptr)  // VX_FLAG_VALLF_ROWS: the packed text memory of the batched NAR, cap_text rows per head
    VXC(regrow(e, (void**)&e->xmem_rows, (size_t)c.nar_num_layers * 2 * c.nar_d_model * text_rows * 2));
  return VX_OK;
}

extern "C" int vx_nar_batch(vx_engine* e, int32_t n, const int64_t* const* text_nar, const int32_t* S2,
                            const int64_t* const* prompts, const int32_t* P, const int64_t* const* ar_tokens,
                            const int32_t* T, int64_t* const* codes_out, void* stream) {
  return vx_nar_batch_ex(e, n, text_nar, S2, prompts, P, ar_tokens, T, codes_out, nullptr, stream);
}
// The NAR stages of n utterances at once, their rows concatenated (nar_run).
extern "C" int vx_nar_batch_ex(vx_engine* e, int32_t n, const int64_t* const* text_nar, const int32_t* S2,
                               const int64_t* const* prompts, const int32_t* P, const int64_t* const* ar_tokens,
                               const int32_t* T, int64_t* const* codes_out, const int64_t* const* forced_codes, void* stream) {
  if (e && e->vallf && !e->vf_rows) return fail(VX_ERR_UNSUPPORTED, "vx_nar_batch: VALL-F runs its NAR stages per utterance (vx_nar)");
  if (!e || !text_nar || !S2 || !prompts || !P || !ar_tokens || !T || !codes_out) return fail(VX_ERR_ARG, "null argument");
  if (!e->finalized) return fail(VX_ERR_STATE, "weights not finalized");
  const vx_config& c = e->cfg;
  if (n < 1 || n > BMAX) return fail(VX_ERR_ARG, "n must be 1..%d", BMAX);
  if (!e->bf16 || !use_mfma(e) || c.num_quantizers < 2) return fail(VX_ERR_UNSUPPORTED, "vx_nar_batch needs bf16 MFMA rows and num_quantizers > 1");
  if (c.flags & VX_FLAG_PRENET) return fail(VX_ERR_UNSUPPORTED, "vx_nar_batch: prenet models run on the batch-1 path only");
  for (int b = 0; b < n; ++b) {
    if (S2[b] <= 0 || T[b] <= 0 || P[b] < 0 || !text_nar[b] || !ar_tokens[b] || !codes_out[b] || (P[b] > 0 && !prompts[b]) ||
        (forced_codes && !forced_codes[b]))
      return fail(VX_ERR_ARG, "bad utterance %d", b);
    // per-utterance limits: positions index the sine table (pe_rows rows) separately for text and audio
    if (S2[b] > e->pe_rows || P[b] + T[b] > e->pe_rows)
      return fail(VX_ERR_CAPACITY, "utterance %d: S2=%d / P+T=%d exceed the %d positions of the sine table", b, S2[b], P[b] + T[b], e->pe_rows);
    if (e->vallf && S2[b] > c.max_text)  // a text memory holds max_text keys (slot memory and packed buffer alike)
      return fail(VX_ERR_CAPACITY, "utterance %d: S2=%d exceeds max_text=%d", b, S2[b], c.max_text);
  }
  return nar_run(e, n, true, text_nar, S2, prompts, P, ar_tokens, T, codes_out, forced_codes, stream);
}

// ------------------------------------------------------------------------------ scoring (vx_score / vx_score_batch)
// Teacher-forced likelihood of given codes: the AR stack over the whole sequence in one row pass (the prefill's mask, no KV
// destination) and the NAR stages through nar_run with forced codes; every scored logits row is reduced on the device by
// nll_rows_kernel.  Nothing the decode paths keep (ArState, the batch-1 cache and text memory, the slot caches) is written.

// Scratch of the scoring passes for `rows` scored rows, and the once-built operands: the AR predict layer padded with zero rows
// to NLL_MAXV (a multiple of the MFMA tile; the nll kernel reads V = 1025 of the ld = 1088 columns), VALL-F's text memory.
static int score_reserve(vx_engine* e, size_t rows) {
  const vx_config& c = e->cfg;
  const int d = c.d_model;
  if (use_mfma(e) && e->sc_head == nullptr) {
    HIPC(hipMalloc(&e->sc_head, (size_t)NLL_MAXV * d * 2));
    e->allocs.push_back(e->sc_head);
    VXC(score_head_refresh(e));
  }
  if (e->vallf && e->xkv_score == nullptr) VXC(dalloc(e, &e->xkv_score, (size_t)c.num_layers * 2 * d * c.max_text * e->esz));
  e->sc_ld = use_mfma(e) ? NLL_MAXV : AR_VOCAB;
  if (rows <= e->sc_cap) return VX_OK;
  HIPC(hipStreamSynchronize(e->es));
  e->sc_rows = 0;  // the "score_ar_argmax" tap describes the buffer that goes away here
  VXC(regrow(e, (void**)&e->sc_logits, rows * e->sc_ld * 4));
  VXC(regrow(e, (void**)&e->sc_nll, rows * 4));
  VXC(regrow(e, (void**)&e->sc_rank, rows * 4));
  VXC(regrow(e, (void**)&e->sc_argmax, rows * 4));
  VXC(regrow(e, (void**)&e->sc_tgt, rows * 8));
  e->sc_cap = rows;
  return VX_OK;
}

// true when p is ordinary host memory (or HIP cannot tell, as on a machine without a device): such codes are range-checked here
static bool host_readable(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return true; }
  return at.type == hipMemoryTypeHost || at.type == hipMemoryTypeUnregistered;
}

// The checks of one utterance to score (no HIP call before the last one, which only asks where `codes` lives); idx >= 0 names it
// in a batch.  S2 <= 0 with text_nar == NULL is legal when the NAR part is skipped.
static int check_score_utterance(vx_engine* e, const int64_t* text, int32_t S, const int64_t* text_nar, int32_t S2, const int64_t* codes,
                                 int32_t A, int32_t P, bool want_ar, bool want_nar, int idx) {
  const vx_config& c = e->cfg;
  const int Q = c.num_quantizers;
  char who[32] = "";
  if (idx >= 0) snprintf(who, sizeof who, " (utterance %d)", idx);
  if (!codes || (want_ar && !text) || (want_nar && !text_nar)) return fail(VX_ERR_ARG, "null argument%s", who);
  if (A < 1 || P < 0 || P >= A) return fail(VX_ERR_ARG, "P=%d outside [0, A=%d)%s", P, A, who);
  if ((want_ar && S <= 0) || (want_nar && S2 <= 0)) return fail(VX_ERR_ARG, "S / S2 must be > 0 (valle.py:991)%s", who);
  if (want_ar && !c.prepend_bos && P < 1)
    return fail(VX_ERR_ARG, "P=0 needs prepend_bos: without a BOS row no input row predicts the first frame%s", who);
  if ((want_ar && S > c.max_text) || (want_nar && S2 > c.max_text) || A + 1 > c.max_audio)
    return fail(VX_ERR_CAPACITY, "S=%d / S2=%d / A=%d exceed capacity (max_text %d, max_audio %d)%s", S, S2, A, c.max_text, c.max_audio, who);
  if (host_readable(codes))
    for (size_t i = 0; i < (size_t)A * Q; ++i)
      if (codes[i] < 0 || codes[i] >= NUM_AUDIO_TOKENS)
        return fail(VX_ERR_ARG, "code %lld at frame %zu, codebook %zu outside [0, %d)%s", (long long)codes[i], i / Q, i % Q, NUM_AUDIO_TOKENS, who);
  return VX_OK;
}

// The rows of the teacher-forced AR pass, shared by scoring and alignment: the layout of n utterances (segmented: concatenated
// rows as in batch_prefill_impl; else n == 1, rows from 0) and their set-up in e->X - [text | (BOS) codes[:, 0]] embedded, through
// the prenets where the model has them, positions added; VALL-F: the text rows become the memory K / V in e->xkv_score and the
// audio rows start at row 0.  The ids go to ids_text / d_fcodes ((A_b, Q) codes of utterance b at frame offset aoff[b]).
struct ScoreRows {
  std::vector<int> start, len, tlen, aoff, soff, roff;  // roff: offsets of the T_b + 1 scored rows
  RowSegs segs;
};
static int score_rows_setup(vx_engine* e, int n, bool segmented, const int64_t* const* text, const int32_t* S, const int64_t* const* codes,
                            const int32_t* A, const int32_t* P, ScoreRows& r) {
  const vx_config& c = e->cfg;
  const int Q = c.num_quantizers, d = c.d_model, bos = c.prepend_bos ? 1 : 0;
  const bool vf = e->vallf, prenet = c.flags & VX_FLAG_PRENET;
  r.start.assign(n + 1, 0); r.len.assign(n, 0); r.tlen.assign(n, 0); r.aoff.assign(n, 0); r.soff.assign(n, 0); r.roff.assign(n + 1, 0);
  std::vector<int>&start = r.start, &len = r.len, &tlen = r.tlen, &aoff = r.aoff, &soff = r.soff, &roff = r.roff;
  RowSegs& segs = r.segs;
  int arows = 0, srows = 0;
  roff[0] = 0;
  for (int b = 0; b < n; ++b) {
    tlen[b] = vf ? 0 : S[b];
    len[b] = tlen[b] + bos + A[b];
    aoff[b] = arows; soff[b] = srows;
    arows += A[b] + 1; srows += S[b];
    roff[b + 1] = roff[b] + (A[b] - P[b]) + 1;
  }
  if (segmented) VXC(seg_layout(e, n, len.data(), tlen.data(), nullptr, d, arows, srows, start.data(), segs));
  else { start[0] = 0; start[1] = len[0]; }
  VXC(score_reserve(e, roff[n]));
  static const long long bos_id = NUM_AUDIO_TOKENS + 1;  // valle.py:1006-1007
  if (bos) HIPC(hipMemcpyAsync(e->ids_audio, &bos_id, 8, hipMemcpyHostToDevice, e->es));
  const float* w_txt = W<float>(e, "ar_text_embedding.word_embeddings.weight");
  const float* w_aud = W<float>(e, "ar_audio_embedding.word_embeddings.weight");
  const float* a_txt = W<float>(e, "ar_text_position.alpha");
  const float* a_aud = W<float>(e, "ar_audio_position.alpha");
  for (int b = 0; b < n; ++b) {
    long long* it = e->ids_text + soff[b];
    long long* ic = e->d_fcodes + (size_t)aoff[b] * Q;  // the (A_b, Q) codes
    HIPC(hipMemcpyAsync(it, text[b], (size_t)S[b] * 8, hipMemcpyDefault, e->es));
    HIPC(hipMemcpyAsync(ic, codes[b], (size_t)A[b] * Q * 8, hipMemcpyDefault, e->es));
    float* xb = e->X + (size_t)start[b] * d;
    float* xa = xb + (size_t)tlen[b] * d;  // the audio rows
    if (prenet) {  // embedding -> prenet -> position (valle.py:995-997, 1013-1015); unsegmented only
      embed_accum_kernel<<<S[b], 256, 0, e->es>>>(it, 1, 0, w_txt, 512, d, e->pn_a, S[b], 1);
      VXC(text_prenet_rows(e, 0, e->pn_a, e->pn_a, S[b], d));
      add_pos_kernel<<<S[b], 256, 0, e->es>>>(e->pn_a, d, a_txt, e->pe_ar, 0, e->X, S[b]);
    } else {
      embed_pos_kernel<<<S[b], 256, 0, e->es>>>(it, 1, 0, w_txt, 512, d, a_txt, e->pe_ar, 0, e->X + (size_t)start[b] * d, S[b]);
    }
    // VALL-F: the text rows become the per-layer memory K / V (valle.py:598-602), then the audio rows take X from row 0
    if (vf) { VXC(cast_rows(e, e->X, e->Hn, (size_t)S[b] * d)); VXC(memory_kv(e, e->ar_l, e->xkv_score, S[b], d, c.nhead)); }
    if (prenet) {
      if (bos) embed_accum_kernel<<<1, 256, 0, e->es>>>(e->ids_audio, 1, 0, w_aud, 1025 + bos, d, e->pn_a, 1, 1);
      embed_accum_kernel<<<A[b], 256, 0, e->es>>>(ic, Q, 0, w_aud, 1025 + bos, d, e->pn_a + (size_t)bos * d, A[b], 1);
      VXC(audio_prenet_rows(e, 0, e->pn_a, e->pn_b, bos + A[b], d));
      add_pos_kernel<<<bos + A[b], 256, 0, e->es>>>(e->pn_b, d, a_aud, e->pe_ar, 0, xa, bos + A[b]);
    } else {
      if (bos) embed_pos_kernel<<<1, 256, 0, e->es>>>(e->ids_audio, 1, 0, w_aud, 1025 + bos, d, a_aud, e->pe_ar, 0, xa, 1);
      embed_pos_kernel<<<A[b], 256, 0, e->es>>>(ic, Q, 0, w_aud, 1025 + bos, d, a_aud, e->pe_ar, bos, xa + (size_t)bos * d, A[b]);
    }
  }
  HIPC(hipGetLastError());
  return VX_OK;
}

// The AR scoring pass of n utterances: the rows of score_rows_setup through the AR stack under the prefix mask, final norm +
// predict layer on the T + 1 rows that predict codes[P, 0] ... codes[A-1, 0], EOS (valle.py:863-877), then nll_rows_kernel.
// Outputs per utterance, T_b + 1 entries.
static int score_ar_run(vx_engine* e, int n, bool segmented, const int64_t* const* text, const int32_t* S, const int64_t* const* codes,
                        const int32_t* A, const int32_t* P, float* const* nll, int32_t* const* rank) {
  const vx_config& c = e->cfg;
  const int Q = c.num_quantizers, d = c.d_model, bos = c.prepend_bos ? 1 : 0;
  const bool vf = e->vallf, post = c.flags & VX_FLAG_POST_NORM;
  HIPC(hipEventRecord(e->ev_t[0], e->es));
  ScoreRows sr;
  VXC(score_rows_setup(e, n, segmented, text, S, codes, A, P, sr));
  const std::vector<int>&start = sr.start, &tlen = sr.tlen, &aoff = sr.aoff, &roff = sr.roff;
  const RowSegs& segs = sr.segs;
  VXC(run_stack(e, e->ar_l, start[n], d, c.nhead, segmented ? 0 : tlen[0], -1, segs, KvDst(),
                vf ? TextMem{e->xkv_score, S[0]} : TextMem()));
  // final norm (pre-norm; a post-norm stack's rows are already normalised) on the scored rows, compacted to [sum (T + 1)][d]
  for (int b = 0; b < n; ++b) {
    const int T = A[b] - P[b], first = tlen[b] + (bos ? P[b] : P[b] - 1);
    const float* xr = e->X + (size_t)(start[b] + first) * d;
    void* hr = (char*)e->Hn + (size_t)roff[b] * d * e->esz;
    if (post) VXC(cast_rows(e, xr, hr, (size_t)(T + 1) * d));
    else VXC(ln_rows(e, xr, W<float>(e, "ar_decoder.norm.weight"), W<float>(e, "ar_decoder.norm.bias"), nullptr, nullptr, hr, T + 1, d));
    score_targets_kernel<<<(T + 1 + 255) / 256, 256, 0, e->es>>>(e->d_fcodes + (size_t)aoff[b] * Q, Q, 0, P[b], T, NUM_AUDIO_TOKENS, 1,
                                                                 e->sc_tgt + roff[b]);
  }
  const int R = roff[n], ld = e->sc_ld;
  VXC(gemm_rows(e, e->Hn, e->sc_head ? e->sc_head : W<void>(e, "ar_predict_layer.weight"), nullptr, e->sc_logits, R, ld, d, GE_PLAIN, true));
  nll_rows_kernel<<<(R + NLL_ROWS_PER_WG - 1) / NLL_ROWS_PER_WG, 256, 0, e->es>>>(e->sc_logits, R, AR_VOCAB, ld, e->sc_tgt, 1, 0, e->sc_nll,
                                                                           e->sc_rank, e->sc_argmax);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(e->ev_t[1], e->es));
  for (int b = 0; b < n; ++b) {
    const size_t nb = (size_t)(roff[b + 1] - roff[b]) * 4;
    if (nll && nll[b]) HIPC(hipMemcpyAsync(nll[b], e->sc_nll + roff[b], nb, hipMemcpyDefault, e->es));
    if (rank && rank[b]) HIPC(hipMemcpyAsync(rank[b], e->sc_rank + roff[b], nb, hipMemcpyDefault, e->es));
  }
  HIPC(hipStreamSynchronize(e->es));  // the host arrays above and the staging are free again
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, e->ev_t[0], e->ev_t[1]));
  e->t_score_ar = ms;
  e->sc_rows = R;
  return VX_OK;
}

// The NAR scoring pass: nar_run on prompts = codes[:P], ar_tokens = codes[P:, 0] (as a strided view is not what nar_run takes,
// the column is staged through the device), forced = codes[P:].
static int score_nar_run(vx_engine* e, int n, bool segmented, const int64_t* const* text_nar, const int32_t* S2, const int64_t* const* codes,
                         const int32_t* A, const int32_t* P, float* const* nll, int32_t* const* rank, void* stream) {
  const int Q = e->cfg.num_quantizers;
  std::vector<const int64_t*> forced(n), tok(n);
  std::vector<int32_t> T(n);
  size_t trows = 0;
  for (int b = 0; b < n; ++b) { T[b] = A[b] - P[b]; trows += T[b]; }
  ON_DEVICE(e->cfg.device);
  VXC(score_reserve(e, trows));
  // codebook 0 of the scored frames, contiguous per utterance: gathered on the device into sc_tgt (free between the two passes)
  VXC(sync_in(e, stream));
  size_t off = 0;
  for (int b = 0; b < n; ++b) {
    forced[b] = codes[b] + (size_t)P[b] * Q;
    HIPC(hipMemcpyAsync(e->d_fcodes, forced[b], (size_t)T[b] * Q * 8, hipMemcpyDefault, e->es));
    score_targets_kernel<<<(T[b] + 255) / 256, 256, 0, e->es>>>(e->d_fcodes, Q, 0, 0, T[b], 0, 0, e->sc_tgt + off);
    tok[b] = (const int64_t*)(e->sc_tgt + off);
    off += T[b];
  }
  HIPC(hipGetLastError());
  const NarScore sc{nll, rank};
  // what nar_run records about "the last NAR call" (timings out[2] / out[7] / out[8], the sizes of the nar_logits / nar_x taps) stays
  // that of the caller's own last vx_nar: the taps' buffers are scratch, but their sizes and the timings are not scoring's to change
  const double t_nar = e->t_nar, t_gemm = e->t_gemm, flops = e->gemm_flops_done;
  const int last_T = e->last_T, last_N = e->last_N;
  const int rc = nar_run(e, n, segmented, text_nar, S2, codes, P, tok.data(), T.data(), nullptr, forced.data(), stream, false, nullptr, &sc);
  e->t_score_nar = e->t_nar;
  e->t_nar = t_nar; e->t_gemm = t_gemm; e->gemm_flops_done = flops;
  e->last_T = last_T; e->last_N = last_N;
  return rc;
}

extern "C" int vx_score(vx_engine* e, const int64_t* text, int32_t S, const int64_t* text_nar, int32_t S2, const int64_t* codes,
                        int32_t A, int32_t P, float* nll_ar, int32_t* rank_ar, float* nll_nar, int32_t* rank_nar, void* stream) {
  if (!e) return fail(VX_ERR_ARG, "null argument");
  if (!e->finalized) return fail(VX_ERR_STATE, "weights not finalized");
  const bool want_ar = nll_ar || rank_ar, want_nar = (nll_nar || rank_nar) && e->cfg.num_quantizers > 1;
  VXC(check_score_utterance(e, text, S, text_nar, S2, codes, A, P, want_ar, want_nar, -1));
  ON_DEVICE(e->cfg.device);
  if (want_ar) {
    VXC(sync_in(e, stream));
    VXC(score_ar_run(e, 1, false, &text, &S, &codes, &A, &P, &nll_ar, &rank_ar));
    VXC(sync_out(e, stream));
  }
  if (want_nar) VXC(score_nar_run(e, 1, false, &text_nar, &S2, &codes, &A, &P, nll_nar ? &nll_nar : nullptr, rank_nar ? &rank_nar : nullptr, stream));
  return VX_OK;
}

extern "C" int vx_score_batch(vx_engine* e, int32_t n, const int64_t* const* text, const int32_t* S, const int64_t* const* text_nar,
                              const int32_t* S2, const int64_t* const* codes, const int32_t* A, const int32_t* P, float* const* nll_ar,
                              int32_t* const* rank_ar, float* const* nll_nar, int32_t* const* rank_nar, void* stream) {
  if (!e) return fail(VX_ERR_ARG, "null argument");
  if (!e->finalized) return fail(VX_ERR_STATE, "weights not finalized");
  const vx_config& c = e->cfg;
  if (e->vallf) return fail(VX_ERR_UNSUPPORTED, "vx_score_batch: VALL-F scores per utterance (vx_score)");
  if (c.flags & VX_FLAG_PRENET) return fail(VX_ERR_UNSUPPORTED, "vx_score_batch: prenet models score per utterance (vx_score)");
  if (!e->bf16 || !use_mfma(e)) return fail(VX_ERR_UNSUPPORTED, "vx_score_batch needs the bf16 MFMA row kernels; use vx_score");
  const bool want_ar = nll_ar || rank_ar, want_nar = (nll_nar || rank_nar) && c.num_quantizers > 1;
  if (!codes || !A || !P || (want_ar && (!text || !S)) || (want_nar && (!text_nar || !S2))) return fail(VX_ERR_ARG, "null argument");
  if (n < 1 || n > BMAX) return fail(VX_ERR_ARG, "n must be 1..%d", BMAX);
  for (int b = 0; b < n; ++b) {
    VXC(check_score_utterance(e, want_ar ? text[b] : nullptr, want_ar ? S[b] : 0, want_nar ? text_nar[b] : nullptr, want_nar ? S2[b] : 0,
                              codes[b], A[b], P[b], want_ar, want_nar, b));
    if ((nll_ar && !nll_ar[b]) || (rank_ar && !rank_ar[b]) || (nll_nar && !nll_nar[b]) || (rank_nar && !rank_nar[b]))
      return fail(VX_ERR_ARG, "null output (utterance %d)", b);
  }
  ON_DEVICE(c.device);
  if (want_ar) {
    VXC(sync_in(e, stream));
    VXC(score_ar_run(e, n, true, text, S, codes, A, P, nll_ar, rank_ar));
    VXC(sync_out(e, stream));
  }
  if (want_nar) VXC(score_nar_run(e, n, true, text_nar, S2, codes, A, P, nll_nar, rank_nar, stream));
  return VX_OK;
}

// ------------------------------------------------------------------------------ alignment (vx_align)
// The attention the AR decoder pays to the text while it predicts each frame, from the same teacher-forced row pass as scoring
// (score_rows_setup + run_stack with an attention tap; no final norm, no predict layer), and the best monotonic path through it.
// Like scoring it writes nothing the decode paths keep.

// Scratch of vx_align / vx_align_batch for maps of `cells` cells and T rows in all, nw head weights and, when staged, ph_cells
// per-head cells; scr_floats: the per-head scratch of the batched tap (0: none).
static int align_reserve(vx_engine* e, size_t cells, size_t T, size_t nw, size_t ph_cells, size_t scr_floats = 0) {
  if (e->al_w == nullptr) { VXC(regrow(e, (void**)&e->al_w, nw * 4)); VXC(regrow(e, (void**)&e->al_score, 8)); }
  if (scr_floats && e->al_segs == nullptr) {
    VXC(regrow(e, (void**)&e->al_segs, (size_t)2 * BMAX * sizeof(AlignSeg)));
    VXC(regrow(e, (void**)&e->al_bscore, (size_t)BMAX * 8));
  }
  if (cells > e->al_cells || T > e->al_rows || ph_cells > e->al_ph_cells || scr_floats > e->al_scr_floats) HIPC(hipStreamSynchronize(e->es));
  if (cells > e->al_cells) {
    VXC(regrow(e, (void**)&e->al_attn, cells * 4));
    VXC(regrow(e, (void**)&e->al_bp, cells));
    e->al_cells = cells;
  }
  if (scr_floats > e->al_scr_floats) {
    VXC(regrow(e, (void**)&e->al_scr, scr_floats * 4));
    e->al_scr_floats = scr_floats;
  }
  if (T > e->al_rows) {
    VXC(regrow(e, (void**)&e->al_mass, T * 4));
    VXC(regrow(e, (void**)&e->al_path, T * 4));
    e->al_rows = T;
  }
  if (ph_cells > e->al_ph_cells) {
    VXC(regrow(e, (void**)&e->al_ph, ph_cells * 4));
    e->al_ph_cells = ph_cells;
  }
  return VX_OK;
}

// The (L, H) head weights of a tap as given or uniform; VX_ERR_ARG unless every entry is finite and >= 0 and one is > 0.
static int align_weights(const float* head_w, int n, std::vector<float>& hw) {
  hw.assign(n, 1.0f / (float)n);
  if (head_w == nullptr) return VX_OK;
  bool any = false;
  for (int i = 0; i < n; ++i) {
    if (!std::isfinite(head_w[i]) || head_w[i] < 0.f) return fail(VX_ERR_ARG, "head_w[%d] = %g: weights must be finite and >= 0", i, (double)head_w[i]);
    any = any || head_w[i] > 0.f;
    hw[i] = head_w[i];
  }
  if (!any) return fail(VX_ERR_ARG, "head_w is all zero: no head to align by");
  return VX_OK;
}

extern "C" int vx_align(vx_engine* e, const int64_t* text, int32_t S, const int64_t* codes, int32_t A, int32_t P, int32_t c0, int32_t c1,
                        const float* head_w, float* attn, float* mass, int32_t* path, double* path_score, float* per_head, void* stream) {
  if (!e || !attn) return fail(VX_ERR_ARG, "null argument");
  if (!e->finalized) return fail(VX_ERR_STATE, "weights not finalized");
  const vx_config& c = e->cfg;
  const int L = c.num_layers, H = c.nhead, d = c.d_model, bos = c.prepend_bos ? 1 : 0;
  if (!(0 <= c0 && c0 < c1 && c1 <= S)) return fail(VX_ERR_ARG, "text window [%d, %d) outside [0, S=%d)", c0, c1, S);
  std::vector<float> hw;
  VXC(align_weights(head_w, L * H, hw));
  VXC(check_score_utterance(e, text, S, nullptr, 0, codes, A, P, true, false, -1));
  const int T = A - P, Sw = c1 - c0, first = bos ? P : P - 1;
  if ((path || path_score) && Sw > ALIGN_MAX_SW) return fail(VX_ERR_CAPACITY, "a path over %d text tokens (at most %d)", Sw, ALIGN_MAX_SW);
  ON_DEVICE(c.device);
  VXC(sync_in(e, stream));
  HIPC(hipEventRecord(e->ev_t[0], e->es));
  ScoreRows sr;
  VXC(score_rows_setup(e, 1, false, &text, &S, &codes, &A, &P, sr));
  const size_t ph_cells = (size_t)L * H * T * Sw;
  const bool ph_staged = per_head && host_readable(per_head);
  VXC(align_reserve(e, (size_t)T * Sw, T, (size_t)L * H, ph_staged ? ph_cells : 0));
  HIPC(hipMemcpyAsync(e->al_w, hw.data(), hw.size() * 4, hipMemcpyHostToDevice, e->es));
  AttnTap tap;
  tap.w = e->al_w; tap.hw = hw.data();
  tap.row = sr.tlen[0] + first; tap.rows = T; tap.row0 = first; tap.text_len = S; tap.c0 = c0; tap.c1 = c1;
  tap.attn = e->al_attn; tap.mass = e->al_mass; tap.per_head = !per_head ? nullptr : ph_staged ? e->al_ph : per_head;
  VXC(run_stack(e, e->ar_l, sr.start[1], d, H, sr.tlen[0], -1, sr.segs, KvDst(), e->vallf ? TextMem{e->xkv_score, S} : TextMem(), &tap));
  if (path || path_score) launch_mono_path(e->al_attn, T, Sw, e->al_bp, e->al_path, e->al_score, e->es);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(e->ev_t[1], e->es));
  HIPC(hipMemcpyAsync(attn, e->al_attn, (size_t)T * Sw * 4, hipMemcpyDefault, e->es));
  if (mass) HIPC(hipMemcpyAsync(mass, e->al_mass, (size_t)T * 4, hipMemcpyDefault, e->es));
  if (path) HIPC(hipMemcpyAsync(path, e->al_path, (size_t)T * 4, hipMemcpyDefault, e->es));
  if (path_score) HIPC(hipMemcpyAsync(path_score, e->al_score, 8, hipMemcpyDefault, e->es));
  if (ph_staged) HIPC(hipMemcpyAsync(per_head, e->al_ph, ph_cells * 4, hipMemcpyDefault, e->es));
  HIPC(hipStreamSynchronize(e->es));  // the host arrays above and the staging are free again
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, e->ev_t[0], e->ev_t[1]));
  e->t_align = ms;
  return sync_out(e, stream);
}

// vx_align of n utterances in one segmented row pass (the rows of vx_score_batch): the tap runs on the matrix pipe over every
// utterance's rows at once (attn_text_seg_kernel), then one path launch over the utterances that asked for a path.
extern "C" int vx_align_batch(vx_engine* e, int32_t n, const int64_t* const* text, const int32_t* S, const int64_t* const* codes,
                              const int32_t* A, const int32_t* P, const int32_t* c0, const int32_t* c1, const float* head_w,
                              float* const* attn, float* const* mass, int32_t* const* path, double* const* path_score, void* stream) {
  if (!e) return fail(VX_ERR_ARG, "null argument");
  if (!e->finalized) return fail(VX_ERR_STATE, "weights not finalized");
  const vx_config& c = e->cfg;
  if (e->vallf) return fail(VX_ERR_UNSUPPORTED, "vx_align_batch: VALL-F aligns per utterance (vx_align)");
  if (c.flags & (VX_FLAG_PRENET | VX_FLAG_POST_NORM)) return fail(VX_ERR_UNSUPPORTED, "vx_align_batch: prenet and post-norm models align per utterance (vx_align)");
  if (!e->bf16 || !use_mfma(e)) return fail(VX_ERR_UNSUPPORTED, "vx_align_batch needs the bf16 MFMA row kernels (head_dim 64); use vx_align");
  if (!text || !S || !codes || !A || !P || !c0 || !c1 || !attn) return fail(VX_ERR_ARG, "null argument");
  if (n < 1 || n > BMAX) return fail(VX_ERR_ARG, "n must be 1..%d", BMAX);
  const int L = c.num_layers, H = c.nhead, d = c.d_model, bos = c.prepend_bos ? 1 : 0;
  std::vector<float> hw;
  VXC(align_weights(head_w, L * H, hw));
  std::vector<AlignSeg> sg(n), psg;
  std::vector<int> pidx;  // the utterances that asked for a path
  long long cells = 0, rows = 0;
  int max_rows = 0, max_sw = 0;
  for (int b = 0; b < n; ++b) {
    if (!attn[b]) return fail(VX_ERR_ARG, "null output (utterance %d)", b);
    if (!(0 <= c0[b] && c0[b] < c1[b] && c1[b] <= S[b]))
      return fail(VX_ERR_ARG, "text window [%d, %d) outside [0, S=%d) (utterance %d)", c0[b], c1[b], S[b], b);
    VXC(check_score_utterance(e, text[b], S[b], nullptr, 0, codes[b], A[b], P[b], true, false, b));
    const int T = A[b] - P[b], Sw = c1[b] - c0[b], first = bos ? P[b] : P[b] - 1;
    const bool want_path = (path && path[b]) || (path_score && path_score[b]);
    if (want_path && Sw > ALIGN_MAX_SW)
      return fail(VX_ERR_CAPACITY, "a path over %d text tokens (at most %d) (utterance %d)", Sw, ALIGN_MAX_SW, b);
    sg[b] = AlignSeg{0, S[b], S[b] + first, T, first, c0[b], c1[b], 0, cells, rows};
    if (want_path) { psg.push_back(sg[b]); pidx.push_back(b); max_sw = std::max(max_sw, Sw); }
    cells += (long long)T * Sw; rows += T;
    max_rows = std::max(max_rows, T);
  }
  ON_DEVICE(c.device);
  VXC(sync_in(e, stream));
  HIPC(hipEventRecord(e->ev_t[0], e->es));
  ScoreRows sr;
  VXC(score_rows_setup(e, n, true, text, S, codes, A, P, sr));
  for (int b = 0; b < n; ++b) sg[b].start = sr.start[b];
  for (size_t z = 0; z < psg.size(); ++z) psg[z].start = sr.start[pidx[z]];
  VXC(align_reserve(e, cells, rows, (size_t)L * H, 0, align_seg_scratch(H, cells, rows)));
  HIPC(hipMemcpyAsync(e->al_w, hw.data(), hw.size() * 4, hipMemcpyHostToDevice, e->es));
  HIPC(hipMemcpyAsync(e->al_segs, sg.data(), (size_t)n * sizeof(AlignSeg), hipMemcpyHostToDevice, e->es));
  if (!psg.empty()) HIPC(hipMemcpyAsync(e->al_segs + BMAX, psg.data(), psg.size() * sizeof(AlignSeg), hipMemcpyHostToDevice, e->es));
  AttnTap tap;
  tap.w = e->al_w; tap.hw = hw.data();
  tap.segs = e->al_segs; tap.nseg = n; tap.max_rows = max_rows; tap.cells = cells; tap.rows_total = rows; tap.scr = e->al_scr;
  tap.attn = e->al_attn; tap.mass = e->al_mass;
  VXC(run_stack(e, e->ar_l, sr.start[n], d, H, 0, -1, sr.segs, KvDst(), TextMem(), &tap));
  if (!psg.empty()) launch_mono_path_segs(e->al_attn, e->al_segs + BMAX, (int)psg.size(), max_sw, e->al_bp, e->al_path, e->al_bscore, e->es);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(e->ev_t[1], e->es));
  for (int b = 0; b < n; ++b) {
    const size_t T = sg[b].rows, Sw = sg[b].c1 - sg[b].c0;
    HIPC(hipMemcpyAsync(attn[b], e->al_attn + sg[b].cell_off, T * Sw * 4, hipMemcpyDefault, e->es));
    if (mass && mass[b]) HIPC(hipMemcpyAsync(mass[b], e->al_mass + sg[b].row_off, T * 4, hipMemcpyDefault, e->es));
    if (path && path[b]) HIPC(hipMemcpyAsync(path[b], e->al_path + sg[b].row_off, T * 4, hipMemcpyDefault, e->es));
  }
  for (size_t z = 0; z < pidx.size(); ++z)
    if (path_score && path_score[pidx[z]]) HIPC(hipMemcpyAsync(path_score[pidx[z]], e->al_bscore + z, 8, hipMemcpyDefault, e->es));
  HIPC(hipStreamSynchronize(e->es));  // the host arrays above are free again
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, e->ev_t[0], e->ev_t[1]));
  e->t_align = ms;
  return sync_out(e, stream);
}

extern "C" int vx_get_timings(vx_engine* e, double* out, int32_t n) {
  if (!e || !out) return fail(VX_ERR_ARG, "null argument");
  const double v[13] = {e->t_prefill, e->t_decode, e->t_nar, (double)e->n_pass, e->n_launch, e->t_bdecode, e->n_blaunch,
                        e->t_gemm, e->gemm_flops_done, (double)e->gexec_nodes, e->t_score_ar, e->t_score_nar, e->t_align};
  for (int i = 0; i < n && i < 13; ++i) out[i] = v[i];
  return VX_OK;
}

// Bytes of the taps whose size follows from the configuration alone (vx_buffer_bytes; vx_read_buffer's range check of the same)
static int64_t config_buffer_bytes(const vx_config& c, const std::string& n) {
  const int64_t esz = c.precision == VX_PREC_F32 ? 4 : 2;
  if (n == "ar_kv") return (int64_t)c.num_layers * 2 * c.d_model * ((int64_t)c.max_text + c.max_audio) * esz;
  if (n == "ar_mem" && (c.flags & VX_FLAG_VALLF)) return (int64_t)c.num_layers * 2 * c.d_model * (int64_t)c.max_text * esz;
  return -1;
}

extern "C" int vx_buffer_bytes(const vx_config* cfg, const char* name, int64_t* bytes) {
  if (!cfg || !name || !bytes) return fail(VX_ERR_ARG, "null argument");
  if (cfg->struct_size != (int32_t)sizeof(vx_config)) return fail(VX_ERR_ARG, "vx_config.struct_size mismatch");
  const int64_t b = config_buffer_bytes(*cfg, name);
  if (b < 0) return fail(VX_ERR_ARG, "no configuration-sized buffer '%s'", name);
  *bytes = b;
  return VX_OK;
}

extern "C" int vx_read_buffer(vx_engine* e, const char* name, void* dst, int64_t off, int64_t nbytes) {
  if (!e || !name || !dst) return fail(VX_ERR_ARG, "null argument");
  ON_DEVICE(e->cfg.device);
  HIPC(hipStreamSynchronize(e->es));
  const std::string n = name;
  const char* src = nullptr;
  int64_t size = 0;
  const bool trace = e->cfg.flags & VX_FLAG_TRACE_LOGITS;
  if (n == "ar_logits") {
    src = (const char*)(trace ? e->ar_logits + LOGITS_CUR : e->ar_logits);
    size = (int64_t)(trace ? e->n_pass : 1) * AR_VOCAB * 4;
  }
  else if (n == "ar_sampled") { src = (const char*)e->d_sampled; size = (int64_t)e->n_pass * 4; }
  else if (n == "ar_argmax") { src = (const char*)e->d_argmax; size = (int64_t)e->n_pass * 4; }
  else if (n == "nar_logits") { src = (const char*)e->nar_logits; size = (int64_t)e->last_T * 1024 * 4; }
  else if (n == "ar_x") { src = (const char*)e->ar_x; size = (int64_t)e->cfg.d_model * 4; }
  else if (n == "nar_x") { src = (const char*)e->X; size = (int64_t)e->last_N * e->cfg.nar_d_model * 4; }
  else if (n == "batch_trace" && e->btrace) { src = (const char*)e->btrace; size = (int64_t)e->bmax * e->btok_stride * AR_VOCAB * 4; }
  else if (n == "batch_logits" && e->bmax > 1) { src = (const char*)e->blogits; size = (int64_t)BMAX * LOGITS_CUR * 4; }
  else if (n == "batch_argmax" && e->bmax > 1) { src = (const char*)e->bargm; size = (int64_t)BMAX * e->btok_stride * 4; }
  else if (n == "batch_sampled" && e->bmax > 1) { src = (const char*)e->bsamp; size = (int64_t)BMAX * e->btok_stride * 4; }
  else if (n == "batch_kv" && e->bmax > 1) {
    src = e->kv8 ? (const char*)e->bkv8 : (const char*)e->bkv;
    size = (int64_t)e->bmax * e->bkv_slot * (e->kv8 ? 1 : 2);
  }
  else if (n == "ar_kv") { src = (const char*)e->kv; size = config_buffer_bytes(e->cfg, n); }
  else if (n == "ar_mem" && e->vallf) { src = (const char*)e->xkv_ar; size = config_buffer_bytes(e->cfg, n); }
  else if (n == "tp_wo" && e->tp) { src = (const char*)e->tp_wo[0]; size = (int64_t)TP_D * TP_D * e->esz; }
  else if (n == "score_ar_argmax" && e->sc_argmax) { src = (const char*)e->sc_argmax; size = (int64_t)e->sc_rows * 4; }
  else if (n == "batch_kv_scale" && e->kv8) { src = (const char*)e->bkv8s; size = (int64_t)e->bmax * e->bkv_slot / 16; }
  else return fail(VX_ERR_ARG, "unknown buffer '%s'", name);
  if (off < 0 || nbytes < 0 || off + nbytes > size) return fail(VX_ERR_ARG, "read of '%s' out of range (%lld+%lld > %lld)", name, (long long)off, (long long)nbytes, (long long)size);
  HIPC(hipStreamSynchronize(e->es));  // the copy below runs on the null stream, which the engine's non-blocking stream does not order with
  HIPC(hipMemcpy(dst, src + off, (size_t)nbytes, hipMemcpyDeviceToHost));
  return VX_OK;
}

// ------------------------------------------------------------------------------ kernel-level ops
extern "C" int vx_op_convert_bf16(const float* src, void* dst, int64_t n, void* stream) {
  convert_kernel<bf16><<<1024, 256, 0, (hipStream_t)stream>>>(src, (bf16*)dst, (size_t)n);
  HIPC(hipGetLastError());
  return VX_OK;
}

extern "C" int vx_op_layernorm(int32_t prec, const float* x, const float* gamma, const float* beta, const float* ada_w,
                               const float* ada_b, void* out, int32_t rows, int32_t d, void* stream) {
  if (d % 4 || d > 2048) return fail(VX_ERR_UNSUPPORTED, "layernorm: d=%d", d);
  hipStream_t s = (hipStream_t)stream;
  if (d <= 1024) {
    if (prec == VX_PREC_BF16) layernorm_rows_kernel<bf16, 4><<<(rows + 3) / 4, 256, 0, s>>>(x, gamma, beta, ada_w, ada_b, (bf16*)out, rows, d);
    else layernorm_rows_kernel<float, 4><<<(rows + 3) / 4, 256, 0, s>>>(x, gamma, beta, ada_w, ada_b, (float*)out, rows, d);
  } else {
    if (prec == VX_PREC_BF16) layernorm_rows_kernel<bf16, 8><<<(rows + 3) / 4, 256, 0, s>>>(x, gamma, beta, ada_w, ada_b, (bf16*)out, rows, d);
    else layernorm_rows_kernel<float, 8><<<(rows + 3) / 4, 256, 0, s>>>(x, gamma, beta, ada_w, ada_b, (float*)out, rows, d);
  }
  HIPC(hipGetLastError());
  return VX_OK;
}

extern "C" int vx_op_gemv(int32_t prec, const void* Wp, const float* bias, const float* x, float* y, int32_t N, int32_t K,
                          int32_t relu, void* stream) {
  GemvArgs a{};
  a.kid = -1;
  a.W = Wp; a.bias = bias; a.x = x; a.y = y; a.N = N; a.K = K;
  a.pro = PRO_COPY; a.epi = relu ? EPI_RELU : (bias ? EPI_BIAS : EPI_PLAIN);
  int dev = 0, cu = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev);
  VXC(launch_gemv(prec == VX_PREC_BF16, a, cu, (hipStream_t)stream));
  HIPC(hipGetLastError());
  return VX_OK;
}

extern "C" int vx_op_gemm(int32_t prec, int32_t mfma, const void* A, const void* Wp, const float* bias, float* C, int32_t M,
                          int32_t N, int32_t K, int32_t relu, void* stream) {
  if (relu && !bias) return fail(VX_ERR_ARG, "gemm: the ReLU epilogue adds a bias");
  const int epi = relu ? GE_RELU : (bias ? GE_BIAS : GE_PLAIN);
  hipStream_t s = (hipStream_t)stream;
  if (prec == VX_PREC_BF16) VXC(gemm_rows_t<bf16>(mfma != 0, (const bf16*)A, (const bf16*)Wp, bias, C, M, N, K, epi, true, s));
  else {
    if (mfma) return fail(VX_ERR_UNSUPPORTED, "MFMA GEMM is bf16 only");
    VXC(gemm_rows_t<float>(false, (const float*)A, (const float*)Wp, bias, C, M, N, K, epi, true, s));
  }
  HIPC(hipGetLastError());
  return VX_OK;
}

// The row path's own GEMM forms on caller data (bf16 output + V^T copy, fp32 residual update): what run_stack launches for QKV /
// FFN1 and for the out-projection / FFN2 at M >= 4096.
extern "C" int vx_op_gemm_rows(int32_t form, const void* A, const void* Wp, const float* bias, void* C, int32_t M, int32_t N,
                               int32_t K, int32_t relu, void* vt, int32_t vt_n0, int32_t vt_ld, void* stream) {
  if (!A || !Wp || !C || !bias || M < 1 || N < 1 || K < 1) return fail(VX_ERR_ARG, "gemm_rows: null operand or empty shape");
  if (form != 0 && form != 1) return fail(VX_ERR_ARG, "gemm_rows: form %d", form);
  if (vt && (form != 0 || vt_n0 < 0 || vt_n0 >= N || vt_n0 % 64 != 0 || vt_ld < M))
    return fail(VX_ERR_ARG, "gemm_rows: V^T copy needs form 0, 0 <= vt_n0 < N, vt_n0 %% 64 == 0 (the kernels test whole column groups), vt_ld >= M");
  hipStream_t s = (hipStream_t)stream;
  if (mfma_gemm_dispatch((const bf16*)A, (const bf16*)Wp, bias, C, M, N, K, form == 1 ? GE_RESID : (relu ? GE_RELU : GE_BIAS), form == 1, s,
                         (bf16*)vt, vt_n0, vt_ld))
    return fail(VX_ERR_UNSUPPORTED, "gemm_rows: no kernel instance");
  HIPC(hipGetLastError());
  return VX_OK;
}

// The split-K launch of the row path's N = d GEMMs on caller data (mfma_gemm_partial, as run_stack calls it): slab z (M, N) fp32 =
// A[:, z K / splits : (z + 1) K / splits] . W[:, same]^T.
extern "C" int vx_op_gemm_partial(const void* A, const void* Wp, float* slabs, int32_t M, int32_t N, int32_t K, int32_t splits,
                                  void* stream) {
  if (!A || !Wp || !slabs || M < 1) return fail(VX_ERR_ARG, "gemm_partial: null operand or M %d < 1", M);
  if (N < 128 || N % 128) return fail(VX_ERR_UNSUPPORTED, "gemm_partial: N %d (a multiple of the 128-wide tile)", N);
  if (splits != 1 && splits != 2 && splits != 4) return fail(VX_ERR_UNSUPPORTED, "gemm_partial: splits %d (1, 2 or 4)", splits);
  if (K < 64 * splits || K % (64 * splits)) return fail(VX_ERR_UNSUPPORTED, "gemm_partial: K %d (a multiple of 64 per slice, %d slices)", K, splits);
  if ((long long)((M + 127) / 128) > 65535) return fail(VX_ERR_UNSUPPORTED, "gemm_partial: M %d (more than 65535 row tiles)", M);
  VXC(mfma_gemm_partial((const bf16*)A, (const bf16*)Wp, slabs, M, N, K, splits, (hipStream_t)stream));
  HIPC(hipGetLastError());
  return VX_OK;
}

// layernorm_rows_kernel<OT, 4> with every optional argument (the launch ln_rows makes): fold of split-K slabs, xout, fold only.
extern "C" int vx_op_ln_fold(int32_t prec, float* x, const float* part, int32_t nsplit, int64_t part_stride, const float* pbias,
                             const float* gamma, const float* beta, const float* ada_w, const float* ada_b, void* out, float* xout,
                             int32_t rows, int32_t d, void* stream) {
  if (d < 4 || d % 4 || d > 1024) return fail(VX_ERR_UNSUPPORTED, "ln_fold: d %d (a multiple of 4 in [4, 1024])", d);
  if (prec != VX_PREC_BF16 && prec != VX_PREC_F32) return fail(VX_ERR_ARG, "ln_fold: prec %d", prec);
  if (!x || rows < 1) return fail(VX_ERR_ARG, "ln_fold: null x or rows %d < 1", rows);
  if (part) {
    if (nsplit < 1 || nsplit > 4) return fail(VX_ERR_ARG, "ln_fold: nsplit %d outside [1, 4]", nsplit);
    if (!pbias) return fail(VX_ERR_ARG, "ln_fold: part needs pbias");
    if (nsplit > 1 && part_stride < (int64_t)rows * d) return fail(VX_ERR_ARG, "ln_fold: part_stride %lld < rows d", (long long)part_stride);
  }
  if (!out && !part) return fail(VX_ERR_ARG, "ln_fold: the fold-only pass (out == NULL) needs part");
  if (!out && xout) return fail(VX_ERR_ARG, "ln_fold: xout needs out");
  if (out && (!gamma || !beta)) return fail(VX_ERR_ARG, "ln_fold: out needs gamma and beta");
  if ((ada_w == nullptr) != (ada_b == nullptr)) return fail(VX_ERR_ARG, "ln_fold: ada_w and ada_b come together");
  Fold f;
  if (part) { f.part = part; f.nsplit = nsplit; f.stride = (size_t)part_stride; f.bias = pbias; }
  ln_rows_launch(prec == VX_PREC_BF16, x, gamma, beta, ada_w, ada_b, out, rows, d, xout, f, (hipStream_t)stream);
  HIPC(hipGetLastError());
  return VX_OK;
}

// {splitk, sp_d, sp_ff} as run_stack chooses them (rows_plan) for a bf16, head_dim 64 stack without MXFP8 and without a text
// memory, over M rows (within the engine's capacity) of width d.  num_cu <= 0: the current device's CU count; with an explicit
// count no HIP call is made.
extern "C" int vx_op_rows_plan(int32_t M, int32_t d, int32_t num_cu, int32_t* out) {
  if (M < 1 || d < 1 || !out) return fail(VX_ERR_ARG, "rows_plan: M %d, d %d or null out", M, d);
  int cu = num_cu;
  if (cu <= 0) {
    int dev = 0;
    HIPC(hipGetDevice(&dev));
    HIPC(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev));
  }
  const RowsPlan p = rows_plan(true, M, d, cu);
  out[0] = p.splitk ? 1 : 0; out[1] = p.sp_d; out[2] = p.sp_ff;
  return VX_OK;
}

// MXFP8 GEMM of the NAR stages (mx_kernels.hpp) on caller-supplied fp32 operands: A (M, K) and W (N, K) are quantised on the
// device exactly as the engine quantises activations / weights, then multiplied by mx256_kernel.  out_mode 0: C (M, N) fp32
// [bias / ReLU]; 2: the FFN1 form - C as e4m3 bytes (M, N) in c_out and its E8M0 block scales (N/32, ld) in sc_out, ld = M
// rounded up to 256.  qa_out / sa_out (optional): the quantised A bytes (M, K) and scales (K/32, ld), so that the quantiser
// itself can be compared bit for bit with the host emulation (tests/mx_ref.py).
extern "C" int vx_op_gemm_mx(const float* A, const float* Wt, const float* bias, void* c_out, void* sc_out, int32_t M, int32_t N,
                             int32_t K, int32_t relu, int32_t out_mode, void* qa_out, void* sa_out, void* stream) {
  if (!A || !Wt || !c_out || M < 1 || N % 256 || K % 128) return fail(VX_ERR_UNSUPPORTED, "mx gemm: M=%d N=%d K=%d (N %% 256, K %% 128)", M, N, K);
  if (out_mode == 2 && !sc_out) return fail(VX_ERR_ARG, "mx gemm: out_mode 2 needs sc_out");  // arguments first, allocations after
  hipStream_t s = (hipStream_t)stream;
  const int ld = (M + 255) / 256 * 256;
  DevBuf<uint8_t> qa, sa, qw, sw;
  VXC(qa.alloc((size_t)M * K)); VXC(sa.alloc((size_t)(K / 32) * ld));
  VXC(qw.alloc((size_t)N * K)); VXC(sw.alloc((size_t)(K / 32) * N));
  HIPC(hipMemsetAsync(sa.get(), 0, (size_t)(K / 32) * ld, s));
  mx_quant_rows_kernel<<<(M + 3) / 4, 256, 0, s>>>(A, qa.get(), sa.get(), M, K, ld);
  mx_quant_rows_kernel<<<(N + 3) / 4, 256, 0, s>>>(Wt, qw.get(), sw.get(), N, K, N);
  HIPC(hipGetLastError());  // a quantiser launch failure is reported as such, not as the GEMM's
  int rc;
  if (out_mode == 2) {
    HIPC(hipMemsetAsync(sc_out, 0, (size_t)(N / 32) * ld, s));
    rc = mx_gemm_dispatch(qa.get(), sa.get(), ld, qw.get(), sw.get(), N, bias, c_out, (uint8_t*)sc_out, ld, M, N, K, GE_RELU, MX_OUT_MX, s);
  } else {
    rc = mx_gemm_dispatch(qa.get(), sa.get(), ld, qw.get(), sw.get(), N, bias, c_out, nullptr, 0, M, N, K, relu ? GE_RELU : (bias ? GE_BIAS : GE_PLAIN), MX_OUT_F32, s);
  }
  hipError_t le = hipGetLastError();
  if (rc == 0 && le == hipSuccess) {
    if (qa_out) le = hipMemcpyAsync(qa_out, qa.get(), (size_t)M * K, hipMemcpyDefault, s);
    if (le == hipSuccess && sa_out) le = hipMemcpyAsync(sa_out, sa.get(), (size_t)(K / 32) * ld, hipMemcpyDefault, s);
  }
  const hipError_t se = hipStreamSynchronize(s);  // the scratch is in use until the stream has drained, whatever happened
  if (rc) return fail(VX_ERR_UNSUPPORTED, "mx gemm: no kernel instance (rc %d)", rc);
  HIPC(le);
  HIPC(se);
  return VX_OK;
}

// (Adaptive)LayerNorm with an MXFP8 result (layernorm_rows_mx_kernel): q_out (rows, d) e4m3 bytes, s_out (d/32, ld) E8M0 bytes,
// ld = rows rounded up to 256 (pad entries zeroed).
extern "C" int vx_op_layernorm_mx(const float* x, const float* gamma, const float* beta, const float* ada_w, const float* ada_b,
                                  void* q_out, void* s_out, int32_t rows, int32_t d, void* stream) {
  if (d % 32 || d > 1024 || rows < 1) return fail(VX_ERR_UNSUPPORTED, "layernorm_mx: d=%d", d);
  hipStream_t s = (hipStream_t)stream;
  const int ld = (rows + 255) / 256 * 256;
  HIPC(hipMemsetAsync(s_out, 0, (size_t)(d / 32) * ld, s));
  layernorm_rows_mx_kernel<4><<<(rows + 3) / 4, 256, 0, s>>>(x, gamma, beta, ada_w, ada_b, (uint8_t*)q_out, (uint8_t*)s_out, rows, d, ld);
  HIPC(hipGetLastError());
  return VX_OK;
}

extern "C" int vx_op_attention(int32_t prec, int32_t mfma, const void* qkv, void* out, int32_t rows, int32_t nhead, int32_t hd,
                               int32_t text_len, void* stream) {
  if (hd != 64) return fail(VX_ERR_UNSUPPORTED, "attention: head_dim %d", hd);
  hipStream_t s = (hipStream_t)stream;
  const int d = nhead * hd;
  const float scale = 1.0f / sqrtf((float)hd);
  dim3 grid((rows + 63) / 64, nhead);
  if (prec == VX_PREC_BF16) {
    if (mfma) {
      const int vt_ld = ((rows + 63) / 64) * 64 + 64;
      bf16* vt = nullptr;
      HIPC(hipMalloc((void**)&vt, (size_t)d * vt_ld * 2));
      vt_from_qkv_kernel<<<dim3((vt_ld + 255) / 256, d), 256, 0, s>>>((const bf16*)qkv, vt, rows, d, vt_ld);
      if (mfma_attn_dispatch((const bf16*)qkv, vt, vt_ld, (bf16*)out, rows, d, nhead, text_len, s) != 0) {
        (void)hipFree(vt);
        return fail(VX_ERR_UNSUPPORTED, "attention: rows x 3 d or d x vt_ld exceed 4 GB");
      }
      HIPC(hipStreamSynchronize(s));
      HIPC(hipFree(vt));
    }
    else attn_rows_simple_kernel<bf16, 64><<<grid, 256, 0, s>>>((const bf16*)qkv, (bf16*)out, rows, d, text_len, scale);
  } else {
    if (mfma) return fail(VX_ERR_UNSUPPORTED, "MFMA attention is bf16 only");
    attn_rows_simple_kernel<float, 64><<<grid, 256, 0, s>>>((const float*)qkv, (float*)out, rows, d, text_len, scale);
  }
  HIPC(hipGetLastError());
  return VX_OK;
}

// The two alignment kernels on caller (device) buffers: see align.hpp for the operands.
extern "C" int vx_op_attn_text_rows(int32_t prec, const void* q, int64_t ldq, const void* k, int64_t ldk, int64_t k_head_stride,
                                    int32_t rows, int32_t row0, int32_t nhead, int32_t hd, int32_t text_len, int32_t causal, int32_t c0,
                                    int32_t c1, const float* head_w, float* attn, float* mass, float* per_head, int32_t first,
                                    void* stream) {
  if (!q || !k || !head_w || !attn) return fail(VX_ERR_ARG, "null argument");
  if (rows < 1 || nhead < 1 || text_len < 1 || row0 < 0) return fail(VX_ERR_ARG, "rows, nhead and text_len must be >= 1, row0 >= 0");
  if (!(0 <= c0 && c0 < c1 && c1 <= text_len)) return fail(VX_ERR_ARG, "text window [%d, %d) outside [0, %d)", c0, c1, text_len);
  if (launch_attn_text_rows(prec == VX_PREC_BF16, q, ldq, k, ldk, k_head_stride, rows, row0, nhead, hd, text_len, causal ? 1 : 0, c0, c1,
                            head_w, attn, mass, per_head, first ? 1 : 0, (hipStream_t)stream))
    return fail(VX_ERR_UNSUPPORTED, "attention tap: head_dim %d", hd);
  HIPC(hipGetLastError());
  return VX_OK;
}

extern "C" int vx_op_mono_path(const float* attn, int32_t T, int32_t Sw, int32_t* path, double* score, void* stream) {
  if (!attn || !path || !score) return fail(VX_ERR_ARG, "null argument");
  if (T < 1 || Sw < 1) return fail(VX_ERR_ARG, "T and Sw must be >= 1");
  if (Sw > ALIGN_MAX_SW) return fail(VX_ERR_CAPACITY, "a path over %d text tokens (at most %d)", Sw, ALIGN_MAX_SW);
  DevBuf<unsigned char> bp;
  VXC(bp.alloc((size_t)T * Sw));
  launch_mono_path(attn, T, Sw, bp.get(), path, score, (hipStream_t)stream);
  const hipError_t err = hipGetLastError(), err2 = hipStreamSynchronize((hipStream_t)stream);
  HIPC(err);
  HIPC(err2);
  return VX_OK;
}

// The kernels of the batched tap on caller (device) buffers.  desc: n x 9 host values per segment (start, text_len, qfirst, rows,
// row0, c0, c1, cell_off, row_off), see AlignSeg; cells / rows_total: the extents of attn / mass.  The per-head scratch is
// allocated here, filled with NaN first.
static int op_align_segs(const int64_t* desc, int32_t n, int nf, std::vector<AlignSeg>& sg) {
  sg.resize(n);
  for (int z = 0; z < n; ++z) {
    const int64_t* v = desc + (size_t)z * nf;
    sg[z] = nf == 9 ? AlignSeg{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], 0, v[7], v[8]}
                    : AlignSeg{0, 0, 0, (int)v[0], 0, 0, (int)v[1], 0, v[2], v[3]};
  }
  return VX_OK;
}

extern "C" int vx_op_attn_text_segs(const void* q, const void* k, int64_t ld, int32_t nseg, const int64_t* desc, int32_t nhead,
                                    const float* head_w, float* attn, float* mass, int64_t cells, int64_t rows_total, int32_t first,
                                    void* stream) {
  if (!q || !k || !desc || !head_w || !attn) return fail(VX_ERR_ARG, "null argument");
  if (nseg < 1 || nhead < 1 || cells < 1 || rows_total < 1) return fail(VX_ERR_ARG, "nseg, nhead, cells and rows_total must be >= 1");
  std::vector<AlignSeg> sg;
  VXC(op_align_segs(desc, nseg, 9, sg));
  int max_rows = 0;
  for (int z = 0; z < nseg; ++z) {
    const AlignSeg& g = sg[z];
    if (g.start < 0 || g.start % 64 || g.text_len < 1 || g.qfirst < 0 || g.rows < 1 || g.row0 < 0)
      return fail(VX_ERR_ARG, "segment %d: start must be a multiple of 64, text_len and rows >= 1, qfirst and row0 >= 0", z);
    if (!(0 <= g.c0 && g.c0 < g.c1 && g.c1 <= g.text_len)) return fail(VX_ERR_ARG, "segment %d: text window [%d, %d) outside [0, %d)", z, g.c0, g.c1, g.text_len);
    if (g.cell_off < 0 || g.cell_off + (long long)g.rows * (g.c1 - g.c0) > cells || g.row_off < 0 || g.row_off + g.rows > rows_total)
      return fail(VX_ERR_ARG, "segment %d: its cells or rows lie outside the outputs", z);
    max_rows = std::max(max_rows, g.rows);
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t scr_floats = align_seg_scratch(nhead, cells, rows_total);
  DevBuf<AlignSeg> d_sg;
  DevBuf<float> scr;
  VXC(d_sg.alloc(sg.size()));
  VXC(scr.alloc(scr_floats));
  VXC(d_sg.upload(sg.data(), sg.size(), s));
  HIPC(hipMemsetAsync(scr.get(), 0xFF, scr_floats * 4, s));
  launch_attn_text_segs(q, k, ld, d_sg.get(), nseg, max_rows, nhead, head_w, scr.get(), cells, rows_total, attn, mass, first ? 1 : 0, s);
  const hipError_t err = hipGetLastError(), err2 = hipStreamSynchronize(s);
  HIPC(err);
  HIPC(err2);
  return VX_OK;
}

// desc: n x 4 host values per map (T, Sw, cell_off, row_off); path: the packed rows; score: n values.
extern "C" int vx_op_mono_path_segs(const float* attn, int32_t n, const int64_t* desc, int32_t* path, double* score, void* stream) {
  if (!attn || !desc || !path || !score) return fail(VX_ERR_ARG, "null argument");
  if (n < 1) return fail(VX_ERR_ARG, "n must be >= 1");
  std::vector<AlignSeg> sg;
  VXC(op_align_segs(desc, n, 4, sg));
  int max_sw = 0;
  long long cells = 0;
  for (int z = 0; z < n; ++z) {
    if (sg[z].rows < 1 || sg[z].c1 < 1 || sg[z].cell_off < 0 || sg[z].row_off < 0) return fail(VX_ERR_ARG, "map %d: T and Sw must be >= 1, offsets >= 0", z);
    if (sg[z].c1 > ALIGN_MAX_SW) return fail(VX_ERR_CAPACITY, "a path over %d text tokens (at most %d)", sg[z].c1, ALIGN_MAX_SW);
    max_sw = std::max(max_sw, sg[z].c1);
    cells = std::max(cells, sg[z].cell_off + (long long)sg[z].rows * sg[z].c1);
  }
  hipStream_t s = (hipStream_t)stream;
  DevBuf<AlignSeg> d_sg;
  DevBuf<unsigned char> bp;
  VXC(d_sg.alloc(sg.size()));
  VXC(bp.alloc((size_t)cells));
  VXC(d_sg.upload(sg.data(), sg.size(), s));
  launch_mono_path_segs(attn, d_sg.get(), n, max_sw, bp.get(), path, score, s);
  const hipError_t err = hipGetLastError(), err2 = hipStreamSynchronize(s);
  HIPC(err);
  HIPC(err2);
  return VX_OK;
}

// Stand-alone sampling check: runs the step's sampling kernel on caller logits with a scratch
// state (no stop-rule side effects are reported; out[0] = sampled index, out[1] = argmax).
extern "C" int vx_op_nll_rows(const float* logits, int32_t rows, int32_t V, int32_t ld, const int64_t* targets, float* nll,
                              int32_t* rank, int32_t* argmax, void* stream) {
  if (!logits || !targets || !nll || !rank || !argmax) return fail(VX_ERR_ARG, "null argument");
  if (rows < 1) return fail(VX_ERR_ARG, "rows must be >= 1 (got %d)", rows);
  if (V < 1 || V > NLL_MAXV) return fail(VX_ERR_ARG, "V=%d outside [1, %d]", V, NLL_MAXV);
  if (ld < V) return fail(VX_ERR_ARG, "ld=%d < V=%d", ld, V);
  nll_rows_kernel<<<(rows + NLL_ROWS_PER_WG - 1) / NLL_ROWS_PER_WG, 256, 0, (hipStream_t)stream>>>(
      logits, rows, V, ld, (const long long*)targets, 1, 0, nll, rank, argmax);
  HIPC(hipGetLastError());
  return VX_OK;
}

// The three sampling entries below: a scratch state built from `h`, one sampler launch on the caller's logits, and the words it
// wrote read back (out[0] = sampled index, out[1] = argmax; lp_out: the log-probability SAMPLE_LP adds).
enum SampleLaunch { SAMPLE_4WAVE, SAMPLE_1WAVE, SAMPLE_LP };  // sample_embed4_kernel<5, 17> / sample_embed_kernel<32> / launch_sample_lp
static ArState op_sample_state(int32_t top_k, float temperature, float top_p, const float* exp_noise) {
  ArState h{};
  h.S = 1 << 20; h.kv_text = h.S; h.top_k = top_k; h.temperature = temperature; h.max_new = -1; h.top_p = top_p;
  h.exp_noise = exp_noise; h.noise_rows = 1; h.seed = 1;
  return h;
}
static int op_sample_run(const ArState& h, const float* logits, int32_t V, SampleLaunch which, int32_t* out, float* lp_out, hipStream_t s) {
  DevBuf<ArState> dst;
  DevBuf<int> words;
  DevBuf<float> fz;
  VXC(dst.alloc(1));
  VXC(words.alloc(16));
  VXC(fz.alloc(4096));
  HIPC(hipMemsetAsync(fz.get(), 0, 4096 * sizeof(float), s));
  VXC(dst.upload(&h, 1, s));
  SampleArgs sa{};
  sa.logits = logits; sa.V = V; sa.st = dst.get();
  sa.tokens = words.get(); sa.sampled = words.get() + 4; sa.argmaxes = words.get() + 8;
  sa.emb = fz.get(); sa.alpha = fz.get(); sa.pe = fz.get(); sa.x = fz.get() + 2048; sa.d = 0;
  if (which == SAMPLE_4WAVE) sample_embed4_kernel<5, 17><<<1, 256, 0, s>>>(sa);
  else if (which == SAMPLE_1WAVE) sample_embed_kernel<32><<<1, 64, 0, s>>>(sa);
  else launch_sample_lp(sa, reinterpret_cast<float*>(words.get() + 12), -1, 1, s);
  HIPC(hipGetLastError());
  int host[16];
  HIPC(hipMemcpyAsync(host, words.get(), sizeof host, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  out[0] = host[4];
  out[1] = host[8];
  if (lp_out) memcpy(lp_out, &host[12], sizeof(float));
  return VX_OK;
}

extern "C" int vx_op_sample(const float* logits, int32_t V, int32_t top_k, float temperature, const float* exp_noise,
                            int32_t* out, void* stream) {
  if (V < 2 || V > 2048) return fail(VX_ERR_UNSUPPORTED, "sample: V=%d", V);
  // both variants are exercised by the parity test: the 4-wave kernel of the decode step for the model's vocabulary,
  // the single-wave one for larger test vocabularies
  return op_sample_run(op_sample_state(top_k, temperature, 0.f, exp_noise), logits, V, V <= 17 * 64 ? SAMPLE_4WAVE : SAMPLE_1WAVE, out,
                       nullptr, (hipStream_t)stream);
}

// vx_op_sample with the nucleus filter: the same scratch state with top_p, on the decode step's four-wave sampler.
extern "C" int vx_op_sample_topp(const float* logits, int32_t V, int32_t top_k, float temperature, float top_p,
                                 const float* exp_noise, int32_t* out, void* stream) {
  if (!logits || !out) return fail(VX_ERR_ARG, "null argument");
  VXC(check_top_p(top_p));
  const float tp = state_top_p(top_p);
  if (tp == 0.f) return vx_op_sample(logits, V, top_k, temperature, exp_noise, out, stream);
  if (V < 2 || V > 17 * 64) return fail(VX_ERR_UNSUPPORTED, "sample_topp: V=%d (the nucleus filter is built for V <= 1088)", V);
  return op_sample_run(op_sample_state(top_k, temperature, tp, exp_noise), logits, V, SAMPLE_4WAVE, out, nullptr, (hipStream_t)stream);
}

// vx_op_sample_topp on the sampler's VX_FLAG_LOGPROBS instantiation (logprob.hip): the same scratch state, the same [sampled, argmax], and
// lp_out[0] = the log-probability of the sampled token on the raw row (lp_eos < 0: an EOS argmax does not redirect it).
extern "C" int vx_op_sample_logprob(const float* logits, int32_t V, int32_t top_k, float temperature, float top_p,
                                    const float* exp_noise, int32_t* out, float* lp_out, void* stream) {
  if (!logits || !out || !lp_out) return fail(VX_ERR_ARG, "null argument");
  VXC(check_top_p(top_p));
  if (V < 2 || V > 17 * 64) return fail(VX_ERR_UNSUPPORTED, "sample_logprob: V=%d (built for 2 <= V <= 1088)", V);
  return op_sample_run(op_sample_state(top_k, temperature, state_top_p(top_p), exp_noise), logits, V, SAMPLE_LP, out, lp_out,
                       (hipStream_t)stream);
}

// Segmented flash attention (the batched NAR / batched prefill launch of attn_rows) on caller rows: nseg segments of a bf16 qkv
// buffer of `rows` rows, described by host arrays.  seg_text == NULL: no mask; otherwise each segment's prefix mask.
extern "C" int vx_op_attention_segs(const void* qkv, void* out, int32_t rows, int32_t nhead, int32_t hd, int32_t nseg,
                                    const int32_t* seg_start, const int32_t* seg_len, const int32_t* seg_text, void* stream) {
  if (hd != 64) return fail(VX_ERR_UNSUPPORTED, "attention_segs: head_dim %d", hd);
  if (nhead < 1 || rows < 1) return fail(VX_ERR_ARG, "attention_segs: nhead %d, rows %d", nhead, rows);
  if (nseg < 1 || nseg > BMAX) return fail(VX_ERR_ARG, "attention_segs: nseg %d outside [1, %d]", nseg, BMAX);
  if (!seg_start || !seg_len) return fail(VX_ERR_ARG, "attention_segs: null segment array");
  int max_len = 0;
  for (int z = 0; z < nseg; ++z) {
    const long long st = seg_start[z], ln = seg_len[z];
    if (st < 0 || st % 64) return fail(VX_ERR_ARG, "attention_segs: segment %d starts at row %lld, not a multiple of 64", z, st);
    if (z > 0 && st < (long long)seg_start[z - 1] + seg_len[z - 1])
      return fail(VX_ERR_ARG, "attention_segs: segment %d (start %lld) overlaps or precedes segment %d", z, st, z - 1);
    if (ln < 1 || st + ln > rows) return fail(VX_ERR_ARG, "attention_segs: segment %d [%lld, %lld + %lld) outside [0, %d) or empty", z, st, st, ln, rows);
    if (seg_text && (seg_text[z] < 0 || seg_text[z] > ln))
      return fail(VX_ERR_ARG, "attention_segs: seg_text[%d] = %d outside [0, len %lld]", z, seg_text[z], ln);
    max_len = std::max(max_len, (int)ln);
  }
  hipStream_t s = (hipStream_t)stream;
  const int d = nhead * hd;
  const int vt_ld = ((rows + 63) / 64) * 64 + 64;  // as the engine (the key-group split reads one tile past the last)
  DevBuf<bf16> vt;
  DevBuf<int> segs_buf;  // start | len | text, nseg each
  VXC(vt.alloc((size_t)d * vt_ld));
  VXC(segs_buf.alloc((size_t)3 * nseg));
  int* segs = segs_buf.get();
  HIPC(hipMemcpyAsync(segs, seg_start, nseg * sizeof(int), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(segs + nseg, seg_len, nseg * sizeof(int), hipMemcpyHostToDevice, s));
  if (seg_text) HIPC(hipMemcpyAsync(segs + 2 * nseg, seg_text, nseg * sizeof(int), hipMemcpyHostToDevice, s));
  vt_from_qkv_kernel<<<dim3((vt_ld + 255) / 256, d), 256, 0, s>>>((const bf16*)qkv, vt.get(), rows, d, vt_ld);
  const int rc = mfma_attn_dispatch((const bf16*)qkv, vt.get(), vt_ld, (bf16*)out, rows, d, nhead, -1, s, segs, segs + nseg, nseg,
                                    max_len, seg_text ? segs + 2 * nseg : nullptr);
  const hipError_t le = hipGetLastError();
  const hipError_t se = hipStreamSynchronize(s);  // the scratch is in use until the stream has drained, whatever happened
  if (rc) return fail(VX_ERR_UNSUPPORTED, "attention_segs: rows x 3 d or d x vt_ld exceed 4 GB");
  HIPC(le);
  HIPC(se);
  return VX_OK;
}

// Segmented cross-attention (cross_attn_seg_kernel, the VX_FLAG_VALLF_ROWS row passes) on caller buffers: segments and per-segment
// memories described by host arrays.
extern "C" int vx_op_cross_attention_segs(const void* q, int32_t ldq, const void* mem, const int64_t* mem_off, int64_t head_stride,
                                          int64_t v_offset, const int32_t* klen, void* out, int32_t rows, int32_t nhead, int32_t nseg,
                                          const int32_t* seg_start, const int32_t* seg_len, void* stream) {
  if (nhead < 1 || rows < 1) return fail(VX_ERR_ARG, "cross_attention_segs: nhead %d, rows %d", nhead, rows);
  if (nseg < 1 || nseg > BMAX) return fail(VX_ERR_ARG, "cross_attention_segs: nseg %d outside [1, %d]", nseg, BMAX);
  if (!seg_start || !seg_len || !mem_off || !klen) return fail(VX_ERR_ARG, "cross_attention_segs: null segment array");
  if ((long long)nhead * 64 > ldq || ldq % 8) return fail(VX_ERR_ARG, "cross_attention_segs: ldq %d must be a multiple of 8 and >= 64 nhead (%d)", ldq, nhead * 64);
  if (head_stride < 64 || v_offset < 0 || head_stride % 8 || v_offset % 8)
    return fail(VX_ERR_ARG, "cross_attention_segs: head_stride %lld (>= 64) and v_offset %lld must be non-negative multiples of 8",
                (long long)head_stride, (long long)v_offset);
  int max_len = 0;
  for (int z = 0; z < nseg; ++z) {
    const long long st = seg_start[z], ln = seg_len[z];
    if (st < 0 || st % 64) return fail(VX_ERR_ARG, "cross_attention_segs: segment %d starts at row %lld, not a multiple of 64", z, st);
    if (z > 0 && st < (long long)seg_start[z - 1] + seg_len[z - 1])
      return fail(VX_ERR_ARG, "cross_attention_segs: segment %d (start %lld) overlaps or precedes segment %d", z, st, z - 1);
    if (ln < 1 || st + ln > rows) return fail(VX_ERR_ARG, "cross_attention_segs: segment %d [%lld, %lld + %lld) outside [0, %d) or empty", z, st, st, ln, rows);
    if (klen[z] < 1 || (long long)klen[z] * 64 > head_stride)
      return fail(VX_ERR_ARG, "cross_attention_segs: klen[%d] = %d outside [1, head_stride / 64 = %lld]", z, klen[z], (long long)head_stride / 64);
    if (mem_off[z] < 0 || mem_off[z] % 8) return fail(VX_ERR_ARG, "cross_attention_segs: mem_off[%d] = %lld must be a non-negative multiple of 8", z, (long long)mem_off[z]);
    max_len = std::max(max_len, (int)ln);
  }
  if (!q || !mem || !out) return fail(VX_ERR_ARG, "cross_attention_segs: null q, mem or out");
  hipStream_t s = (hipStream_t)stream;
  std::vector<long long> off(mem_off, mem_off + nseg);
  DevBuf<int> segs_buf;  // start | len | klen, nseg each
  DevBuf<long long> d_off;
  VXC(segs_buf.alloc((size_t)3 * nseg));
  VXC(d_off.alloc(nseg));
  int* segs = segs_buf.get();
  HIPC(hipMemcpyAsync(segs, seg_start, nseg * sizeof(int), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(segs + nseg, seg_len, nseg * sizeof(int), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(segs + 2 * nseg, klen, nseg * sizeof(int), hipMemcpyHostToDevice, s));
  VXC(d_off.upload(off.data(), nseg, s));
  cross_attn_seg_launch((const bf16*)q, ldq, (const bf16*)mem, d_off.get(), head_stride, v_offset, segs + 2 * nseg, (bf16*)out, nhead * 64, nhead,
                        segs, segs + nseg, nseg, max_len, s);
  const hipError_t le = hipGetLastError();
  const hipError_t se = hipStreamSynchronize(s);  // the scratch is in use until the stream has drained, whatever happened
  HIPC(le);
  HIPC(se);
  return VX_OK;
}

// The batched decode step's single-query attention (attn_batch_kernel / attn_batch8_kernel) on a caller cache of B slots, indexed
// as the engine's slot caches: slot b at b * slot_stride elements, V at v_offset, element (h * ctx_max + j) * 64 + c; fp8 scale
// bytes at that index >> 4 of kv_scale.  ctx / done: host arrays (done may be NULL: every slot live).
extern "C" int vx_op_attn_slots(int32_t kv_fp8, const float* q, const void* kv, const void* kv_scale, int64_t slot_stride,
                                int64_t v_offset, int32_t ctx_max, int32_t B, int32_t nhead, const int32_t* ctx, const int32_t* done,
                                void* out, void* stream) {
  if (B < 1 || B > BMAX) return fail(VX_ERR_ARG, "attn_slots: B %d outside [1, %d]", B, BMAX);
  if (nhead < 1 || ctx_max < 1) return fail(VX_ERR_ARG, "attn_slots: nhead %d, ctx_max %d", nhead, ctx_max);
  if (v_offset < 0 || slot_stride < 0 || v_offset % 16 || slot_stride % 16)
    return fail(VX_ERR_ARG, "attn_slots: v_offset %lld and slot_stride %lld must be non-negative multiples of 16", (long long)v_offset,
                (long long)slot_stride);
  if (!ctx) return fail(VX_ERR_ARG, "attn_slots: null ctx");
  if (kv_fp8 && !kv_scale) return fail(VX_ERR_ARG, "attn_slots: fp8 caches need kv_scale");
  std::vector<ArState> h(B);  // zero-initialised: only row and done are read
  for (int b = 0; b < B; ++b) {
    h[b].done = done ? (done[b] != 0) : 0;
    if (!h[b].done && (ctx[b] < 1 || ctx[b] > ctx_max))
      return fail(VX_ERR_ARG, "attn_slots: ctx[%d] = %d outside [1, ctx_max %d]", b, ctx[b], ctx_max);
    h[b].row = ctx[b] - 1;
  }
  hipStream_t s = (hipStream_t)stream;
  const int d = 64 * nhead;
  DevBuf<ArState> st;
  VXC(st.alloc(B));
  VXC(st.upload(h.data(), B, s));
  if (kv_fp8)
    attn_batch8_kernel<64><<<dim3(nhead, B), 256, 0, s>>>(q, (const uint8_t*)kv, (const uint8_t*)kv_scale, (size_t)slot_stride,
                                                          (size_t)v_offset, st.get(), ctx_max, d, 0.125f, (bf16*)out);
  else
    attn_batch_kernel<64><<<dim3(nhead, B), 256, 0, s>>>(q, (const bf16*)kv, (size_t)slot_stride, (size_t)v_offset, st.get(), ctx_max, d,
                                                         0.125f, (bf16*)out);
  const hipError_t le = hipGetLastError();
  const hipError_t se = hipStreamSynchronize(s);
  HIPC(le);
  HIPC(se);
  return VX_OK;
}

// The VALL-F slot step's cross-attention (attn_batch_kernel<64, MEM>) on a caller memory of B slots, bf16, indexed as the engine's
// slot memory: slot b at b * slot_stride elements, V at v_offset, element (h * max_text + j) * 64 + c.  len / done: host arrays;
// slot b attends to keys [0, len[b]) (done may be NULL: every slot live).
extern "C" int vx_op_attn_mem_slots(const float* q, const void* mem, int64_t slot_stride, int64_t v_offset, int32_t max_text, int32_t B,
                                    int32_t nhead, const int32_t* len, const int32_t* done, void* out, void* stream) {
  if (B < 1 || B > BMAX) return fail(VX_ERR_ARG, "attn_mem_slots: B %d outside [1, %d]", B, BMAX);
  if (nhead < 1 || max_text < 1) return fail(VX_ERR_ARG, "attn_mem_slots: nhead %d, max_text %d", nhead, max_text);
  if (v_offset < 0 || slot_stride < 0 || v_offset % 8 || slot_stride % 8)
    return fail(VX_ERR_ARG, "attn_mem_slots: v_offset %lld and slot_stride %lld must be non-negative multiples of 8", (long long)v_offset,
                (long long)slot_stride);
  if (!len) return fail(VX_ERR_ARG, "attn_mem_slots: null len");
  std::vector<ArState> h(B);  // zero-initialised: only S and done are read
  for (int b = 0; b < B; ++b) {
    h[b].done = done ? (done[b] != 0) : 0;
    if (!h[b].done && (len[b] < 1 || len[b] > max_text))
      return fail(VX_ERR_ARG, "attn_mem_slots: len[%d] = %d outside [1, max_text %d]", b, len[b], max_text);
    h[b].S = len[b];
  }
  hipStream_t s = (hipStream_t)stream;
  DevBuf<ArState> st;
  VXC(st.alloc(B));
  VXC(st.upload(h.data(), B, s));
  attn_batch_kernel<64, true><<<dim3(nhead, B), 256, 0, s>>>(q, (const bf16*)mem, (size_t)slot_stride, (size_t)v_offset, st.get(), max_text,
                                                             64 * nhead, 0.125f, (bf16*)out);
  const hipError_t le = hipGetLastError();
  const hipError_t se = hipStreamSynchronize(s);
  HIPC(le);
  HIPC(se);
  return VX_OK;
}

// One bgemm_kernel launch of the batched step (through launch_bgemm, so only the engine's own instances run) on caller buffers.
// done / row / pass: host arrays (nullable: zeros) of B entries, BMAX entries indexed by slot for BE_LOGITS_MAP; uploaded as ArState.
extern "C" int vx_op_bgemm(int32_t epi, int32_t kv8, const void* A, const void* W, const float* bias, int32_t N, int32_t K, int32_t B,
                           int32_t kgroups, const int32_t* done, const int32_t* row, const int32_t* pass, float* q, void* kv, void* kv8s,
                           int64_t kv_slot_stride, int64_t kv_v_offset, int32_t d, int32_t ctx_max, void* f, float* part, float* logits,
                           int32_t logits_stride, float* trace, int32_t trace_rows, const int32_t* slot_map, void* stream) {
  if (epi < BE_QKV || epi > BE_BIAS) return fail(VX_ERR_ARG, "bgemm: unknown epilogue %d", epi);
  if (kv8 && epi != BE_QKV) return fail(VX_ERR_ARG, "bgemm: kv8 needs the QKV epilogue");
  if (B < 1 || B > BMAX) return fail(VX_ERR_ARG, "bgemm: B %d outside [1, %d]", B, BMAX);
  if (N < 1 || N > 65535 || K < 1 || K > 65535) return fail(VX_ERR_ARG, "bgemm: N %d, K %d outside [1, 65535]", N, K);
  if (kgroups < 1 || (epi != BE_PARTIAL && kgroups != 1)) return fail(VX_ERR_ARG, "bgemm: kgroups %d (> 1 for BE_PARTIAL only)", kgroups);
  const int ns = K / (kgroups * 128);
  if (ns * kgroups * 128 != K || (ns != 1 && ns != 2 && ns != 4 && ns != 8))
    return fail(VX_ERR_ARG, "bgemm: K %d is not ns x kgroups %d x 128 with ns in {1, 2, 4, 8}", K, kgroups);
  if (!A || !W) return fail(VX_ERR_ARG, "bgemm: null A or W");
  if ((epi == BE_QKV || epi == BE_RELU || epi == BE_BIAS) && !bias) return fail(VX_ERR_ARG, "bgemm: epilogue %d needs bias", epi);
  const bool map = epi == BE_LOGITS_MAP;
  const int nst = map ? BMAX : B;
  if (epi == BE_QKV) {
    if (d < 64 || d % 64 || N != 3 * d) return fail(VX_ERR_ARG, "bgemm: QKV needs d %% 64 == 0 and N == 3 d (d %d, N %d)", d, N);
    if (!q || !kv || (kv8 && !kv8s)) return fail(VX_ERR_ARG, "bgemm: QKV needs q and the %s cache", kv8 ? "fp8 (codes + scales)" : "bf16");
    if (ctx_max < 1 || kv_slot_stride < 0 || kv_v_offset < 0 || (kv8 && (kv_slot_stride % 16 || kv_v_offset % 16)))
      return fail(VX_ERR_ARG, "bgemm: ctx_max %d, slot stride %lld, V offset %lld", ctx_max, (long long)kv_slot_stride,
                  (long long)kv_v_offset);
    for (int b = 0; b < B; ++b)
      if (!(done && done[b]) && (row ? row[b] : 0) >= ctx_max) return fail(VX_ERR_ARG, "bgemm: row[%d] outside [0, ctx_max %d)", b, ctx_max);
  }
  if (epi == BE_RELU && !f) return fail(VX_ERR_ARG, "bgemm: BE_RELU needs f");
  if (epi == BE_BIAS && !q) return fail(VX_ERR_ARG, "bgemm: BE_BIAS needs q");
  if (epi == BE_PARTIAL && !part) return fail(VX_ERR_ARG, "bgemm: BE_PARTIAL needs part");
  if (epi == BE_LOGITS || map) {
    if (!logits || logits_stride < N) return fail(VX_ERR_ARG, "bgemm: logits need a buffer and a stride >= N (%d)", logits_stride);
    if (trace && trace_rows < 1) return fail(VX_ERR_ARG, "bgemm: trace_rows %d", trace_rows);
  }
  if (map) {
    if (!slot_map) return fail(VX_ERR_ARG, "bgemm: BE_LOGITS_MAP needs slot_map");
    for (int z = 0; z < B; ++z)
      if (slot_map[z] < 0 || slot_map[z] >= BMAX) return fail(VX_ERR_ARG, "bgemm: slot_map[%d] = %d outside [0, %d)", z, slot_map[z], BMAX);
  }
  std::vector<ArState> h(nst);  // zero-initialised: only done, row and pass are read
  for (int b = 0; b < nst; ++b) {
    h[b].done = done ? (done[b] != 0) : 0;
    h[b].row = row ? row[b] : 0;
    h[b].pass = pass ? pass[b] : 0;
    if (h[b].row < 0 || h[b].pass < 0) return fail(VX_ERR_ARG, "bgemm: row[%d] / pass[%d] negative", b, b);
  }
  hipStream_t s = (hipStream_t)stream;
  DevBuf<ArState> st;
  DevBuf<int> d_map;
  VXC(st.alloc(nst));
  VXC(st.upload(h.data(), nst, s));
  if (map) {
    VXC(d_map.alloc(B));
    VXC(d_map.upload(slot_map, B, s));
  }
  BgemmArgs a{};
  a.A = (const bf16*)A; a.W = (const bf16*)W; a.bias = bias; a.N = N; a.K = K; a.B = B; a.kgroups = kgroups; a.st = st.get();
  a.q = q; a.kv_slot_stride = (size_t)kv_slot_stride; a.kv_v_offset = (size_t)kv_v_offset; a.d = d; a.hd = 64; a.ctx_max = ctx_max;
  a.f = (bf16*)f; a.part = part; a.logits = logits; a.logits_stride = logits_stride; a.trace = trace; a.trace_rows = trace_rows;
  a.slot_map = d_map.get();
  if (kv8) { a.kv8 = (uint8_t*)kv; a.kv8s = (uint8_t*)kv8s; } else { a.kv = (bf16*)kv; }
  int rc = VX_OK;
  switch (epi) {
    case BE_QKV: rc = kv8 ? launch_bgemm<BE_QKV, true>(a, s) : launch_bgemm<BE_QKV>(a, s); break;
    case BE_RELU: rc = launch_bgemm<BE_RELU>(a, s); break;
    case BE_PARTIAL: rc = launch_bgemm<BE_PARTIAL>(a, s); break;
    case BE_LOGITS: rc = launch_bgemm<BE_LOGITS>(a, s); break;
    case BE_LOGITS_MAP: rc = launch_bgemm<BE_LOGITS_MAP>(a, s); break;
    default: rc = launch_bgemm<BE_BIAS>(a, s); break;
  }
  const hipError_t le = hipGetLastError();
  const hipError_t se = hipStreamSynchronize(s);  // the scratch is in use until the stream has drained
  if (rc != VX_OK) return rc;
  HIPC(le);
  HIPC(se);
  return VX_OK;
}

// The batched step's LayerNorm (ln_batch_kernel<kgroups>, kgroups 0 / 1 / 4) or, with a host slot_map, batched prefill's
// ln_batch_map_kernel, on caller buffers.
extern "C" int vx_op_ln_batch(float* x, const float* part, int32_t kgroups, const float* pbias, const float* gamma, const float* beta,
                              void* h, int32_t B, int32_t d, const int32_t* slot_map, void* stream) {
  if (d < 4 || d > 1024 || d % 4) return fail(VX_ERR_ARG, "ln_batch: d %d (a multiple of 4 in [4, 1024])", d);
  if (B < 1 || B > BMAX) return fail(VX_ERR_ARG, "ln_batch: B %d outside [1, %d]", B, BMAX);
  if (kgroups != 0 && kgroups != 1 && kgroups != 4) return fail(VX_ERR_ARG, "ln_batch: kgroups %d (0, 1 or 4)", kgroups);
  if (!x || !gamma || !beta || !h) return fail(VX_ERR_ARG, "ln_batch: null x, gamma, beta or h");
  if (kgroups && (!part || !pbias)) return fail(VX_ERR_ARG, "ln_batch: kgroups %d needs part and pbias", kgroups);
  if (slot_map) {
    if (kgroups) return fail(VX_ERR_ARG, "ln_batch: the slot_map form adds no partials (kgroups %d)", kgroups);
    for (int z = 0; z < B; ++z)
      if (slot_map[z] < 0 || slot_map[z] >= BMAX) return fail(VX_ERR_ARG, "ln_batch: slot_map[%d] = %d outside [0, %d)", z, slot_map[z], BMAX);
  }
  hipStream_t s = (hipStream_t)stream;
  DevBuf<int> d_map;
  if (slot_map) {
    VXC(d_map.alloc(B));
    VXC(d_map.upload(slot_map, B, s));
    ln_batch_map_kernel<<<B, 256, 0, s>>>(x, gamma, beta, (bf16*)h, d, d_map.get());
  } else {
    launch_ln_batch(x, kgroups ? part : nullptr, kgroups, pbias, gamma, beta, (bf16*)h, B, d, s);
  }
  const hipError_t le = hipGetLastError();
  const hipError_t se = hipStreamSynchronize(s);
  HIPC(le);
  HIPC(se);
  return VX_OK;
}

// ------------------------------------------------------------------------------ mel-spectrogram Transformer (vx_mel_*)
// valle/models/transformer.py.  The handle owns a vx_engine in VALL-F form that serves as its decoder side - the KV cache, the text
// memory, the row buffers, the weights under the reference's own keys (mel_key_table) and the captured step - so the decoder
// layers are run_stack's and enqueue_ar_step's launches as they are; the encoder is run_stack over encoder layers without a mask.
// New: the step's opening kernel (meltf.hip), the fp32 head / prenet rows of the teacher-forced pass, and the stop rule.
struct vx_mel {
  vx_engine* e = nullptr;
  vx_mel_config cfg{};
  int cap = 0;  // frames
  std::vector<LayerW> enc_l;
  MelCtl* d_ctl = nullptr;
  MelCtl h_ctl{};  // staging of d_ctl: lives as long as the copy may read it
  float *xh = nullptr, *frames = nullptr, *stops = nullptr, *headW = nullptr, *headB = nullptr;
  float *fin = nullptr, *ra = nullptr, *rh1 = nullptr, *rh2 = nullptr, *rn = nullptr, *rhead = nullptr;  // row scratch
  int S = 0;
  bool encoded = false, decoded = false;
  int n_frames = 0, reason = 0, n_pass = 0;
  double t_decode = 0, n_launch = 0, t_encode = 0;
};

static void mel_key_table(vx_engine* e) {
  const int d = e->cfg.d_model, L = e->cfg.num_layers;
  auto add = [&](const std::string& k, std::vector<int64_t> s) {
    Tensor t; t.shape = s; t.numel = 1; for (auto v : s) t.numel *= (size_t)v;
    t.low = e->bf16 && is_matrix_key(k);
    e->w[k] = t; e->keys.push_back(k);
  };
  add("text_embedding.word_embeddings.weight", {512, d});
  if (e->cfg.flags & VX_FLAG_PRENET) {  // transformer.py:68-95; Sequential indices as in the reference
    for (int conv : {1, 5, 9}) {
      const std::string cv = "encoder_prenet." + std::to_string(conv), bn = "encoder_prenet." + std::to_string(conv + 1);
      add(cv + ".weight", {d, d, 5}); add(cv + ".bias", {d});
      add(bn + ".weight", {d}); add(bn + ".bias", {d}); add(bn + ".running_mean", {d}); add(bn + ".running_var", {d});
    }
    add("encoder_prenet.14.weight", {d, d}); add("encoder_prenet.14.bias", {d});
    add("decoder_prenet.0.weight", {MEL_PRENET_H, MEL_BINS}); add("decoder_prenet.0.bias", {MEL_PRENET_H});
    add("decoder_prenet.3.weight", {MEL_PRENET_H, MEL_PRENET_H}); add("decoder_prenet.3.bias", {MEL_PRENET_H});
    add("decoder_prenet.6.weight", {d, MEL_PRENET_H}); add("decoder_prenet.6.bias", {d});
  } else {
    add("decoder_prenet.weight", {d, MEL_BINS}); add("decoder_prenet.bias", {d});
  }
  add("encoder_position.alpha", {1});
  add("decoder_position.alpha", {1});
  add_encoder_keys(e, "encoder", d, L, false, 0);
  add_encoder_keys(e, "decoder", d, L, false, 1);
  add("predict_layer.weight", {MEL_BINS, d}); add("predict_layer.bias", {MEL_BINS});
  add("stop_layer.weight", {1, d}); add("stop_layer.bias", {1});
}

extern "C" void vx_mel_destroy(vx_mel* m) {
  if (!m) return;
  vx_destroy(m->e);  // every device block of the handle was allocated through the engine
  delete m;
}

extern "C" int vx_mel_create(const vx_mel_config* cfg, vx_mel** out) {
  if (!cfg || !out) return fail(VX_ERR_ARG, "null argument");
  if (cfg->struct_size != (int32_t)sizeof(vx_mel_config)) return fail(VX_ERR_ARG, "vx_mel_config.struct_size mismatch");
  const vx_mel_config& c = *cfg;
  if (c.d_model <= 0 || c.nhead <= 0 || c.num_layers <= 0 || c.d_model % c.nhead) return fail(VX_ERR_ARG, "bad d_model/nhead/num_layers");
  if (c.max_text <= 0 || c.max_frames <= 0) return fail(VX_ERR_ARG, "capacities must be positive");
  if (c.precision != VX_PREC_F32 && c.precision != VX_PREC_BF16) return fail(VX_ERR_ARG, "precision must be VX_PREC_F32 or VX_PREC_BF16");
  if (c.scaling_xformers)
    return fail(VX_ERR_UNSUPPORTED, "scaling_xformers=True (ScaledLinear / BasicNorm / DoubleSwish, transformer.py:114-172) is not built");
  const int hd = c.d_model / c.nhead;
  if (hd != 4 && hd != 8 && hd != 16 && hd != 32 && hd != 64) return fail(VX_ERR_UNSUPPORTED, "head_dim (d_model/nhead) must be 4, 8, 16, 32 or 64");
  if (c.d_model % 8 || c.d_model > 1024) return fail(VX_ERR_UNSUPPORTED, "d_model must be a multiple of 8 and <= 1024");
  if (hd == 64 && c.d_model % 64) return fail(VX_ERR_UNSUPPORTED, "d_model must be a multiple of 64 at head_dim 64");
  if ((long long)c.max_text + c.max_frames + 2 > (1 << 20)) return fail(VX_ERR_UNSUPPORTED, "max_text + max_frames above 2^20 rows");
  ON_DEVICE(c.device);
  vx_mel* m = new vx_mel();
  m->cfg = c; m->cap = c.max_frames;
  vx_engine* e = m->e = new vx_engine();
  vx_config& ec = e->cfg;
  ec.struct_size = sizeof(vx_config);
  ec.d_model = ec.nar_d_model = c.d_model; ec.nhead = ec.nar_nhead = c.nhead; ec.num_layers = ec.nar_num_layers = c.num_layers;
  ec.num_quantizers = 1; ec.precision = c.precision; ec.max_text = c.max_text; ec.max_audio = c.max_frames + 2; ec.device = c.device;
  ec.flags = VX_FLAG_VALLF | (c.norm_first ? 0 : VX_FLAG_POST_NORM) | (c.add_prenet ? VX_FLAG_PRENET : 0) |
             ((c.flags & VX_MEL_NO_GRAPH) ? VX_FLAG_NO_GRAPH : 0);
  e->mel = true;
  auto body = [&]() -> int {
    VXC(create_body(e));
    const size_t d = c.d_model, rows = (size_t)c.max_frames;
    VXC(dalloc_t(e, &m->d_ctl, 1));
    VXC(dalloc_t(e, &m->xh, d));
    VXC(dalloc_t(e, &m->frames, rows * MEL_BINS));
    VXC(dalloc_t(e, &m->stops, rows + 2));
    VXC(dalloc_t(e, &m->headW, (size_t)MEL_HEAD * d));
    VXC(dalloc_t(e, &m->headB, 128));
    VXC(dalloc_t(e, &m->fin, rows * MEL_BINS));
    VXC(dalloc_t(e, &m->ra, rows * d));
    VXC(dalloc_t(e, &m->rn, rows * d));
    VXC(dalloc_t(e, &m->rhead, rows * MEL_HEAD));
    if (c.add_prenet) {
      VXC(dalloc_t(e, &m->rh1, rows * MEL_PRENET_H));
      VXC(dalloc_t(e, &m->rh2, rows * MEL_PRENET_H));
    }
    HIPC(hipMemsetAsync(m->d_ctl, 0, sizeof(MelCtl), e->es));
    HIPC(hipStreamSynchronize(e->es));
    return VX_OK;
  };
  const int rc = body();
  if (rc != VX_OK) {
    const std::string keep = g_err;
    vx_mel_destroy(m);
    g_err = keep;
    return rc;
  }
  *out = m;
  return VX_OK;
}

extern "C" int vx_mel_set_weight(vx_mel* m, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
  if (!m) return fail(VX_ERR_ARG, "null argument");
  return vx_set_weight(m->e, key, data, shape, ndim);
}

extern "C" int vx_mel_set_sine_table(vx_mel* m, const float* data, int64_t rows, int64_t dim) {
  if (!m) return fail(VX_ERR_ARG, "null argument");
  return vx_set_sine_table(m->e, 0, data, rows, dim);
}

extern "C" int vx_mel_finalize(vx_mel* m) {
  if (!m) return fail(VX_ERR_ARG, "null argument");
  vx_engine* e = m->e;
  ON_DEVICE(e->cfg.device);
  for (auto& k : e->keys)
    if (!e->w[k].set) return fail(VX_ERR_WEIGHTS, "missing key '%s' (strict load)", k.c_str());
  const int d = e->cfg.d_model, L = e->cfg.num_layers;
  fill_layers(e, "decoder", L, false, e->ar_l, 1);
  fill_layers(e, "encoder", L, false, m->enc_l, 0);
  if (!e->pe_ar_set) {
    std::vector<float> t;
    host_sine_table(t, e->pe_rows, d);
    HIPC(hipMemcpy(e->pe_ar, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  }
  if (m->cfg.add_prenet) {
    const size_t nel = (size_t)5 * d * d;
    for (int i = 0; i < 3; ++i)
      conv_weight_relayout_kernel<<<(unsigned)((nel + 255) / 256), 256, 0, e->es>>>(
          W<float>(e, "encoder_prenet." + std::to_string(1 + 4 * i) + ".weight"), e->convT[0][i], d);
    HIPC(hipGetLastError());
  }
  // the head as one (101, d) matrix: predict_layer's rows, then stop_layer's
  HIPC(hipMemcpyAsync(m->headW, W<float>(e, "predict_layer.weight"), (size_t)MEL_BINS * d * 4, hipMemcpyDeviceToDevice, e->es));
  HIPC(hipMemcpyAsync(m->headW + (size_t)MEL_BINS * d, W<float>(e, "stop_layer.weight"), (size_t)d * 4, hipMemcpyDeviceToDevice, e->es));
  HIPC(hipMemcpyAsync(m->headB, W<float>(e, "predict_layer.bias"), MEL_BINS * 4, hipMemcpyDeviceToDevice, e->es));
  HIPC(hipMemcpyAsync(m->headB + MEL_BINS, W<float>(e, "stop_layer.bias"), 4, hipMemcpyDeviceToDevice, e->es));
  HIPC(hipStreamSynchronize(e->es));
  e->finalized = true;
  m->encoded = m->decoded = false;
  return VX_OK;
}

// The checks of vx_mel_encode, before any HIP call.
static int mel_check_text(vx_mel* m, const int64_t* text, int32_t S) {
  if (!m || !text) return fail(VX_ERR_ARG, "null argument");
  if (S <= 0) return fail(VX_ERR_ARG, "S must be > 0 (transformer.py:340)");
  if (!m->e->finalized) return fail(VX_ERR_STATE, "weights not finalized");
  if (S > m->cfg.max_text) return fail(VX_ERR_CAPACITY, "S=%d exceeds max_text=%d", S, m->cfg.max_text);
  return VX_OK;
}

// encode on the engine's stream (no synchronisation): X <- encoder(text), memory K / V of every decoder layer
static int mel_encode_rows(vx_mel* m, const int64_t* text, int S) {
  vx_engine* e = m->e;
  const int d = e->cfg.d_model, H = e->cfg.nhead;
  const bool post = e->cfg.flags & VX_FLAG_POST_NORM;
  HIPC(hipMemcpyAsync(e->ids_text, text, (size_t)S * 8, hipMemcpyDefault, e->es));
  const float* emb = W<float>(e, "text_embedding.word_embeddings.weight");
  const float* alpha = W<float>(e, "encoder_position.alpha");
  if (m->cfg.add_prenet) {  // transformer.py:69-85
    embed_accum_kernel<<<S, 256, 0, e->es>>>(e->ids_text, 1, 0, emb, 512, d, e->pn_a, S, 1);
    const float* src = e->pn_a;
    float* bufs[2] = {e->pn_b, e->pn_a};
    for (int i = 0; i < 3; ++i) {
      const std::string cv = "encoder_prenet." + std::to_string(1 + 4 * i), bn = "encoder_prenet." + std::to_string(2 + 4 * i);
      float* dst = bufs[i & 1];
      conv5_bn_relu_kernel<<<(S + CONV_TT - 1) / CONV_TT, 256, (size_t)(CONV_TT + 4) * d * 4, e->es>>>(
          src, e->convT[0][i], W<float>(e, cv + ".bias"), W<float>(e, bn + ".weight"), W<float>(e, bn + ".bias"),
          W<float>(e, bn + ".running_mean"), W<float>(e, bn + ".running_var"), dst, S, d);
      src = dst;
    }
    VXC(linear_rows_f32(e, src, W<float>(e, "encoder_prenet.14.weight"), W<float>(e, "encoder_prenet.14.bias"), e->pn_a, S, d, d, false));
    add_pos_kernel<<<S, 256, 0, e->es>>>(e->pn_a, d, alpha, e->pe_ar, 0, e->X, S);
  } else {
    embed_pos_kernel<<<S, 256, 0, e->es>>>(e->ids_text, 1, 0, emb, 512, d, alpha, e->pe_ar, 0, e->X, S);
  }
  {  // encoder layers have two norms each: the engine's norm-site arithmetic (front_site / norm_at) follows npl
    const int npl = e->npl;
    e->npl = 2;
    const int rc = run_stack(e, m->enc_l, S, d, H, -1, -1, RowSegs(), KvDst());
    e->npl = npl;
    VXC(rc);
  }
  if (post) VXC(cast_rows(e, e->X, e->Hn, (size_t)S * d));  // no final norm (transformer.py:185): X holds the last norm2's rows
  else VXC(ln_rows(e, e->X, W<float>(e, "encoder.norm.weight"), W<float>(e, "encoder.norm.bias"), nullptr, nullptr, e->Hn, S, d));
  VXC(memory_kv(e, e->ar_l, e->xkv_ar, S, d, H));
  e->mem_len = S;
  HIPC(hipGetLastError());
  return VX_OK;
}

extern "C" int vx_mel_encode(vx_mel* m, const int64_t* text, int32_t S, void* stream) {
  VXC(mel_check_text(m, text, S));
  vx_engine* e = m->e;
  ON_DEVICE(e->cfg.device);
  VXC(sync_in(e, stream));
  HIPC(hipEventRecord(e->ev_t[0], e->es));
  VXC(mel_encode_rows(m, text, S));
  HIPC(hipEventRecord(e->ev_t[1], e->es));
  HIPC(hipStreamSynchronize(e->es));  // `text` may be host memory the caller frees on return
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, e->ev_t[0], e->ev_t[1]));
  m->t_encode = ms;
  m->S = S; m->encoded = true; m->decoded = false;
  VXC(sync_out(e, stream));
  return VX_OK;
}

static MelStep mel_step(vx_mel* m) {
  vx_engine* e = m->e;
  const vx_config& c = e->cfg;
  MelStep st{};
  MelStepArgs& a = st.open;
  const NormW fin = (c.flags & VX_FLAG_POST_NORM) ? norm_at(e, e->ar_l, front_site(e, c.num_layers, 0))
                                                  : NormW{W<float>(e, "decoder.norm.weight"), W<float>(e, "decoder.norm.bias")};
  a.xh = m->xh; a.gamma = fin.g; a.beta = fin.b; a.Wh = m->headW; a.bh = m->headB;
  if (m->cfg.add_prenet) {
    a.W1 = W<float>(e, "decoder_prenet.0.weight"); a.b1 = W<float>(e, "decoder_prenet.0.bias");
    a.W2 = W<float>(e, "decoder_prenet.3.weight"); a.b2 = W<float>(e, "decoder_prenet.3.bias");
    a.W0 = W<float>(e, "decoder_prenet.6.weight"); a.b0 = W<float>(e, "decoder_prenet.6.bias");
  } else {
    a.W0 = W<float>(e, "decoder_prenet.weight"); a.b0 = W<float>(e, "decoder_prenet.bias");
  }
  a.alpha = W<float>(e, "decoder_position.alpha"); a.pe = e->pe_ar;
  a.x = e->ar_x; a.st = e->d_st; a.ctl = m->d_ctl; a.frames = m->frames; a.stops = m->stops; a.d = c.d_model;
  return st;
}

// limit: frames the decode may append; forced / n_forced: teacher forcing (frames already in m->fin)
static int mel_decode_impl(vx_mel* m, int limit, int n_forced, bool cap_limited, void* stream) {
  vx_engine* e = m->e;
  ArState& st = e->h_st[0];
  memset(&st, 0, sizeof st);
  st.S = m->S; st.row = -1; st.temperature = 1.0f; st.max_new = -1;
  HIPC(hipMemcpyAsync(e->d_st, &st, sizeof st, hipMemcpyHostToDevice, e->es));
  MelCtl& ctl = m->h_ctl;
  ctl = MelCtl{};  // the arrival counter starts from zero every decode, whatever an interrupted one left
  ctl.max_frames = limit; ctl.n_forced = n_forced; ctl.forced = n_forced > 0 ? m->fin : nullptr;
  HIPC(hipMemcpyAsync(m->d_ctl, &ctl, sizeof ctl, hipMemcpyHostToDevice, e->es));
  const MelStep ms_ = mel_step(m);
  auto step = [e, ms_](hipStream_t s) { return enqueue_ar_step(e, s, &ms_); };
  VXC(step_graph(e, &e->gexec, step, &e->gexec_nodes));
  // launch 0 forms input row 0; pass p is launch p + 1; at most limit + 1 passes (the one that stops appends nothing)
  const long long bound = (long long)(n_forced > 0 ? n_forced : limit + 1) + 1;
  auto stop_rule = [&](const ArState* hs, long long at) -> int {
    if (hs->done) return POLL_STOP;
    return at < bound ? POLL_MORE : fail(VX_ERR_STATE, "mel decode did not terminate within %lld steps", bound);
  };
  ArState* const poll[2] = {e->h_st + 1, e->h_st + 2};
  long long launched = 0;
  float ms = 0.f;
  VXC(replay_polled(e, e->gexec, step, bound, POLL_CHUNK, e->d_st, 1, poll, stop_rule, &launched, &ms));
  HIPC(hipMemcpyAsync(&e->h_st[1], e->d_st, sizeof(ArState), hipMemcpyDeviceToHost, e->es));
  HIPC(hipStreamSynchronize(e->es));
  HIPC(hipGetLastError());
  m->t_decode = ms; m->n_launch = (double)launched;
  m->n_frames = e->h_st[1].n_gen; m->reason = e->h_st[1].stop_reason; m->n_pass = e->h_st[1].pass;
  m->decoded = true;
  VXC(sync_out(e, stream));
  if (cap_limited && m->reason == VX_MEL_STOP_MAX_FRAMES)
    return fail(VX_ERR_CAPACITY, "capacity exceeded: %d frames (max_frames of the handle) were generated before the stop rule fired; raise max_frames",
                m->n_frames);
  return VX_OK;
}

extern "C" int vx_mel_decode(vx_mel* m, int32_t max_frames, void* stream) {
  if (!m) return fail(VX_ERR_ARG, "null argument");
  if (!m->encoded) return fail(VX_ERR_STATE, "vx_mel_decode needs a vx_mel_encode");
  if (max_frames > m->cap) return fail(VX_ERR_CAPACITY, "max_frames=%d exceeds the handle's capacity %d", max_frames, m->cap);
  const long long natural = 10LL * m->S;  // frames the reference's length rule admits
  int limit = max_frames;
  bool cap_limited = false;
  if (max_frames < 0) {
    cap_limited = natural > m->cap;
    limit = cap_limited ? m->cap : (int)natural;
  }
  vx_engine* e = m->e;
  ON_DEVICE(e->cfg.device);
  VXC(sync_in(e, stream));
  return mel_decode_impl(m, limit, 0, cap_limited, stream);
}

extern "C" int vx_mel_decode_forced(vx_mel* m, const float* forced, int32_t T, void* stream) {
  if (!m || !forced) return fail(VX_ERR_ARG, "null argument");
  if (!m->encoded) return fail(VX_ERR_STATE, "vx_mel_decode_forced needs a vx_mel_encode");
  if (T < 1) return fail(VX_ERR_ARG, "T must be >= 1");
  if (T > m->cap) return fail(VX_ERR_CAPACITY, "T=%d exceeds max_frames=%d", T, m->cap);
  vx_engine* e = m->e;
  ON_DEVICE(e->cfg.device);
  VXC(sync_in(e, stream));
  HIPC(hipMemcpyAsync(m->fin, forced, (size_t)T * MEL_BINS * 4, hipMemcpyDefault, e->es));
  return mel_decode_impl(m, T, T, false, stream);
}

extern "C" int vx_mel_result(vx_mel* m, float* frames, int32_t capacity, int32_t* n_frames, int32_t* stop_reason, float* stop_logits,
                             int32_t* n_pass) {
  if (!m) return fail(VX_ERR_ARG, "null argument");
  if (!m->decoded) return fail(VX_ERR_STATE, "no finished decode");
  ON_DEVICE(m->e->cfg.device);
  if (n_frames) *n_frames = m->n_frames;
  if (stop_reason) *stop_reason = m->reason;
  if (n_pass) *n_pass = m->n_pass;
  if (frames) {
    if (capacity < m->n_frames) return fail(VX_ERR_CAPACITY, "frame buffer too small (%d < %d)", capacity, m->n_frames);
    if (m->n_frames) HIPC(hipMemcpy(frames, m->frames, (size_t)m->n_frames * MEL_BINS * 4, hipMemcpyDefault));
  }
  if (stop_logits && m->n_pass) HIPC(hipMemcpy(stop_logits, m->stops, (size_t)m->n_pass * 4, hipMemcpyDefault));
  return VX_OK;
}

extern "C" int vx_mel_teacher_forced(vx_mel* m, const int64_t* text, int32_t S, const float* frames, int32_t T, float* predict,
                                     float* stop_logits, void* stream) {
  VXC(mel_check_text(m, text, S));
  if (!frames || !predict || !stop_logits) return fail(VX_ERR_ARG, "null argument");
  if (T < 1) return fail(VX_ERR_ARG, "T must be >= 1");
  if (T > m->cap) return fail(VX_ERR_CAPACITY, "T=%d exceeds max_frames=%d", T, m->cap);
  vx_engine* e = m->e;
  const int d = e->cfg.d_model, H = e->cfg.nhead;
  ON_DEVICE(e->cfg.device);
  VXC(sync_in(e, stream));
  VXC(mel_encode_rows(m, text, S));
  m->S = S; m->encoded = true; m->decoded = false;
  // inputs [0; frames[:-1]] (pad_y, transformer.py:274-279) -> decoder_prenet -> + alpha pe
  HIPC(hipMemsetAsync(m->fin, 0, MEL_BINS * 4, e->es));
  if (T > 1) HIPC(hipMemcpyAsync(m->fin + MEL_BINS, frames, (size_t)(T - 1) * MEL_BINS * 4, hipMemcpyDefault, e->es));
  if (m->cfg.add_prenet) {
    VXC(linear_rows_f32(e, m->fin, W<float>(e, "decoder_prenet.0.weight"), W<float>(e, "decoder_prenet.0.bias"), m->rh1, T, MEL_PRENET_H, MEL_BINS, true));
    VXC(linear_rows_f32(e, m->rh1, W<float>(e, "decoder_prenet.3.weight"), W<float>(e, "decoder_prenet.3.bias"), m->rh2, T, MEL_PRENET_H, MEL_PRENET_H, true));
    VXC(linear_rows_f32(e, m->rh2, W<float>(e, "decoder_prenet.6.weight"), W<float>(e, "decoder_prenet.6.bias"), m->ra, T, d, MEL_PRENET_H, false));
  } else {
    VXC(linear_rows_f32(e, m->fin, W<float>(e, "decoder_prenet.weight"), W<float>(e, "decoder_prenet.bias"), m->ra, T, d, MEL_BINS, false));
  }
  add_pos_kernel<<<T, 256, 0, e->es>>>(m->ra, d, W<float>(e, "decoder_position.alpha"), e->pe_ar, 0, e->X, T);
  // causal over the frame rows (text_len 0), no KV destination, the text as cross-attention memory
  VXC(run_stack(e, e->ar_l, T, d, H, 0, -1, RowSegs(), KvDst(), TextMem{e->xkv_ar, S}));
  const float* src = e->X;  // post-norm: the rows are the last norm3's output (transformer.py:199)
  if (!(e->cfg.flags & VX_FLAG_POST_NORM)) {
    ln_rows_launch(false, e->X, W<float>(e, "decoder.norm.weight"), W<float>(e, "decoder.norm.bias"), nullptr, nullptr, m->rn, T, d, nullptr,
                   Fold(), e->es);
    src = m->rn;
  }
  VXC(linear_rows_f32(e, src, m->headW, m->headB, m->rhead, T, MEL_HEAD, d, false));
  HIPC(hipGetLastError());
  HIPC(hipMemcpy2DAsync(predict, MEL_BINS * 4, m->rhead, MEL_HEAD * 4, MEL_BINS * 4, T, hipMemcpyDefault, e->es));
  HIPC(hipMemcpy2DAsync(stop_logits, 4, m->rhead + MEL_BINS, MEL_HEAD * 4, 4, T, hipMemcpyDefault, e->es));
  HIPC(hipStreamSynchronize(e->es));
  VXC(sync_out(e, stream));
  return VX_OK;
}

extern "C" int vx_mel_get_timings(vx_mel* m, double* out, int32_t n) {
  if (!m || !out) return fail(VX_ERR_ARG, "null argument");
  const double v[4] = {m->t_decode, m->n_launch, (double)m->e->gexec_nodes, m->t_encode};
  for (int i = 0; i < n && i < 4; ++i) out[i] = v[i];
  return VX_OK;
}

extern "C" int vx_mel_read(vx_mel* m, const char* name, void* dst, int64_t off, int64_t nbytes) {
  if (!m || !name || !dst) return fail(VX_ERR_ARG, "null argument");
  const std::string n = name;
  if (n == "ar_kv" || n == "ar_mem" || n == "ar_x") return vx_read_buffer(m->e, name, dst, off, nbytes);
  if (n != "xh") return fail(VX_ERR_ARG, "unknown buffer '%s'", name);
  vx_engine* e = m->e;
  ON_DEVICE(e->cfg.device);
  const int64_t size = (int64_t)e->cfg.d_model * 4;
  if (off < 0 || nbytes < 0 || off + nbytes > size) return fail(VX_ERR_ARG, "read of '%s' out of range (%lld+%lld > %lld)", name, (long long)off, (long long)nbytes, (long long)size);
  HIPC(hipStreamSynchronize(e->es));
  HIPC(hipMemcpy(dst, (const char*)m->xh + off, (size_t)nbytes, hipMemcpyDeviceToHost));
  return VX_OK;
}

// The step's opening kernel on caller buffers.  The state and the control words live in one device block of this call; the
// launches are ordered by the stream, nothing waits inside a kernel.
extern "C" int vx_op_mel_open(int32_t d, const float* xh, const float* gamma, const float* beta, const float* Wh, const float* bh,
                              const float* W1, const float* b1, const float* W2, const float* b2, const float* W0, const float* b0,
                              const float* alpha, const float* pe, int32_t pe_rows, float* x, float* frames, int32_t frames_cap,
                              float* stops, int32_t stops_cap, int32_t* state, int32_t max_frames, int32_t n_forced,
                              const float* forced, int32_t launches, uint32_t* arrive, void* stream) {
  if (!xh || !gamma || !beta || !Wh || !bh || !W0 || !b0 || !alpha || !pe || !x || !frames || !stops || !state)
    return fail(VX_ERR_ARG, "null argument");
  if (d <= 0 || d % 8 || d > 1024) return fail(VX_ERR_UNSUPPORTED, "d_model must be a multiple of 8 and <= 1024");
  const int given = (W1 != nullptr) + (b1 != nullptr) + (W2 != nullptr) + (b2 != nullptr);
  if (given != 0 && given != 4) return fail(VX_ERR_ARG, "mel_open: the MLP prenet needs W1, b1, W2 and b2, the linear one none of them");
  if (n_forced < 0 || (n_forced > 0 && !forced)) return fail(VX_ERR_ARG, "mel_open: n_forced=%d needs the forced frames", n_forced);
  const int row = state[0], pass = state[1], n_gen = state[2];
  if (launches < 1 || row < -1 || pass < 0 || n_gen < 0) return fail(VX_ERR_ARG, "mel_open: launches=%d row=%d pass=%d n_gen=%d", launches, row, pass, n_gen);
  // every launch may advance each of them by one: position row read row + 1, frame slot n_gen, stop slot pass
  if ((long long)row + launches >= pe_rows || (long long)n_gen + launches > frames_cap || (long long)pass + launches > stops_cap ||
      (n_forced > 0 && (long long)n_gen + launches > n_forced))
    return fail(VX_ERR_CAPACITY, "mel_open: %d launches from row=%d pass=%d n_gen=%d leave pe (%d rows), frames (%d), stops (%d) or forced (%d)",
                launches, row, pass, n_gen, pe_rows, frames_cap, stops_cap, n_forced);
  hipStream_t s = (hipStream_t)stream;
  struct Block { ArState st; MelCtl ctl; } h{};
  h.st.row = row; h.st.pass = pass; h.st.n_gen = n_gen; h.st.S = state[3]; h.st.done = state[4]; h.st.stop_reason = state[5];
  h.st.temperature = 1.0f; h.st.max_new = -1;
  h.ctl.max_frames = max_frames; h.ctl.n_forced = n_forced; h.ctl.forced = n_forced > 0 ? forced : nullptr;
  Block* dv = nullptr;
  HIPC(hipMalloc((void**)&dv, sizeof(Block)));
  auto body = [&]() -> int {
    HIPC(hipMemcpyAsync(dv, &h, sizeof h, hipMemcpyHostToDevice, s));
    MelStepArgs a{};
    a.xh = xh; a.gamma = gamma; a.beta = beta; a.Wh = Wh; a.bh = bh; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.W0 = W0; a.b0 = b0;
    a.alpha = alpha; a.pe = pe; a.x = x; a.st = &dv->st; a.ctl = &dv->ctl; a.frames = frames; a.stops = stops; a.d = d;
    for (int i = 0; i < launches; ++i) launch_mel_open(a, s);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(&h, dv, sizeof h, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return VX_OK;
  };
  const int rc = body();
  (void)hipFree(dv);
  if (rc != VX_OK) return rc;
  state[0] = h.st.row; state[1] = h.st.pass; state[2] = h.st.n_gen; state[3] = h.st.S; state[4] = h.st.done; state[5] = h.st.stop_reason;
  if (arrive) *arrive = h.ctl.arrive;
  return VX_OK;
}

#ifdef VX_PROBES
#include "probe_entry.hpp"
#endif
