/*
 * vallex.h — C ABI of the MI355X-native VALL-E inference engine (libvallex.so).
 *
 * The reference (RuntimeRacer/vall-e) is pure Python and has no FFI: its "operator interface"
 * for this path is the method valle.models.VALLE.inference (valle/models/valle.py:961-1137)
 * called from valle/bin/infer.py:197-204 and :241-248.  This header is the boundary a
 * maintainer binds instead (ctypes stub in INTEGRATION.md); every entry point cites the piece
 * of the reference it replaces.  Plain C types only: no torch / HIP types in any signature
 * (a stream is passed as void* = hipStream_t, NULL = the default stream).
 *
 * Conventions
 *   - every function returns VX_OK (0) or an error code; vx_last_error() gives the message of
 *     the last failure on the calling thread.
 *   - id / code arrays are int64 (torch.LongTensor layout, as the reference passes them) and
 *     may live in device OR host memory — the engine detects which.  The caller owns them.
 *   - one engine per device per thread; calls on one engine must not overlap.
 *   - work is ordered after everything already enqueued on `stream`, and `stream` is made to
 *     wait for the engine's work before the call returns (the engine runs on its own stream
 *     so that the AR step can be replayed as a hipGraph).
 */
#ifndef VALLEX_H
#define VALLEX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vx_engine vx_engine;

enum vx_status {
  VX_OK = 0,
  VX_ERR_ARG = 1,         /* bad argument (the reference would trip an assert, valle.py:986-991) */
  VX_ERR_HIP = 2,         /* a HIP runtime call failed */
  VX_ERR_STATE = 3,       /* call order violated (e.g. decode before prefill) */
  VX_ERR_CAPACITY = 4,    /* S / P / T exceed the capacities given at vx_create, or a decode filled the KV cache (max_audio
                             rows) before the reference's stop rule fired; the worst case 16 S + 1 alone is NOT refused */
  VX_ERR_UNSUPPORTED = 5, /* configuration outside the built scope */
  VX_ERR_WEIGHTS = 6      /* unknown key, wrong shape or missing tensor */
};

enum vx_precision {
  VX_PREC_F32 = 0, /* fp32 weights, KV cache and activations: the token-exact parity mode */
  VX_PREC_BF16 = 1, /* bf16 matrices / KV cache / GEMM operands, fp32 residual stream + accumulate */
  VX_PREC_FP8_NAR = 2 /* VX_PREC_BF16, and the NAR stages' QKV / FFN1 / FFN2 GEMMs (valle.py:1115-1134 through
                         transformer.py:296-334) on OCP e4m3 operands with E8M0 scales per 32 k (MXFP8, the matrix cores'
                         block-scaled fp8 form) wherever the stage runs at >= 4096 concatenated rows (vx_nar_batch);
                         attention, out-projection, predict layers and the whole AR path stay bf16 (BASELINE configs[4]) */
};

enum vx_stop_reason {
  VX_STOP_NONE = 0,
  VX_STOP_EOS_ARGMAX = 1, /* argmax(logits) == 1024      (valle.py:1045) */
  VX_STOP_EOS_SAMPLE = 2, /* sampled token == 1024       (valle.py:1046) */
  VX_STOP_LENGTH = 3,     /* generated > 16 * text_len   (valle.py:1047) */
  VX_STOP_MAX_NEW = 4     /* engine-level max_new_tokens (not in the reference) */
};

enum vx_flags {
  VX_FLAG_TRACE_LOGITS = 1, /* keep the (1025,) AR logits of every pass (parity tests) */
  VX_FLAG_NO_GRAPH = 2,     /* launch the AR step kernel by kernel instead of as a hipGraph */
  VX_FLAG_SIMPLE_ROWS = 4,  /* bf16 mode: use the scalar-FMA row kernels instead of MFMA (A/B checks) */
  VX_FLAG_PRENET = 16,      /* add_prenet=True (valle.py:96-123, 181-213): conv/BatchNorm text prenets and MLP audio
                               prenets in front of the position embeddings, fp32; batch-1 path only */
  VX_FLAG_POST_NORM = 8,    /* norm_first=False (valle.py:60, transformer.py:303-308): x = norm(x + block(x)), no final
                               encoder norms; batch-1 path only (max_batch must be <= 1) */
  VX_FLAG_VALLF = 32,       /* the cross-attention variant VALLF (valle.py:49-719, --model-name VALL-F): both stacks are
                               TransformerDecoderLayers (modules/transformer.py:409-601) - causal / unmasked self-attention over
                               the AUDIO rows only, cross-attention over the embedded text, three norms per layer.  Same entry
                               points (VALLF.inference, valle.py:566-710, has VALLE.inference's signature); the state_dict gains
                               layers.N.multihead_attn.* and layers.N.norm3.*.  With max_batch >= 2 (pre-norm, no prenets,
                               head_dim 64, d_model in {128, 256, 512, 1024}, bf16 precision, bf16 slot caches) the slots decode VALL-F too:
                               every slot keeps its own text memory (2 L max_text d bf16).  VALL-F slots are prefilled one by
                               one (vx_batch_prefill, VX_ADMIT_PER_SLOT) and their NAR stages run per utterance (vx_nar);
                               vx_batch_prefill_all, VX_ADMIT_BATCHED and vx_nar_batch return VX_ERR_UNSUPPORTED unless
                               VX_FLAG_VALLF_ROWS is set too */
  VX_FLAG_KV_FP8 = 64,      /* the slot caches of the batched decode (vx_batch_*) hold OCP e4m3 codes with one E8M0 scale per
                               16 channels of a K / V row instead of bf16 values: 0.53x the bytes the batched
                               step's attention reads.  Needs max_batch >= 2, VX_PREC_BF16 or VX_PREC_FP8_NAR, head_dim 64 and a
                               pre-norm VALL-E without prenets (else VX_ERR_UNSUPPORTED, before any HIP call; VALL-F included).  The batch-1 cache
                               (vx_ar_*) stays bf16 */
  VX_FLAG_VALLF_ROWS = 128, /* VALL-F row passes over concatenated utterances: vx_batch_prefill_all, VX_ADMIT_BATCHED and
                               vx_nar_batch / vx_nar_batch_ex accept the engine; the cross-attention of those passes runs per
                               segment over each utterance's own text memory (cross_attn_seg_kernel, bf16 MFMA).  Valid only
                               together with VX_FLAG_VALLF and max_batch >= 2 within the VALL-F slot limits (pre-norm, no prenets,
                               head_dim 64, d_model in {128, 256, 512, 1024}, bf16 precision, bf16 slot caches); anything else is
                               VX_ERR_UNSUPPORTED from vx_create, before any HIP call.  Cost: the engine also keeps a packed
                               text-memory buffer for the batched NAR pass, [layer][K|V][head][text rows][64] bf16 =
                               2 nar_num_layers nar_d_model bf16 per text row, max_text rows at vx_create and grown with the
                               other row buffers to the sum of the texts of the largest vx_nar_batch call.  Without the flag a
                               VALL-F engine behaves exactly as before.  vx_score_batch still refuses VALL-F */
  VX_FLAG_LOGPROBS = 256    /* generation also records the model's log-probability of every token it emits (what every serving
                               engine returns next to its tokens; best-of-N synthesis ranks candidates by it without a second
                               scoring pass).  AR: per pass i, lp[i] = z[t] - logsumexp(z) on the RAW logits row z (before
                               temperature, top-k and top-p), t = forced[i] where teacher forcing supplies a token, 1024 (EOS) when
                               pass i ended the decode with VX_STOP_EOS_ARGMAX / VX_STOP_EOS_SAMPLE, else the sampled token (tap
                               "ar_sampled"; it is the appended token whenever one is appended).  A teacher-forced decode of n tokens has
                               n + 1 passes (the pass behind the last forced token closes it and appends nothing; its value is that
                               of its sample), an EOS stop n_tokens + 1, every other stop n_tokens.  lp[:n_tokens] lines up with the
                               tokens and after an EOS stop lp[n_tokens] is the EOS term: their sum is -sum(nll_ar) of vx_score for
                               the same codes.  NAR: per stage and generated row, max(row) - logsumexp(row), the log-probability of
                               the code the stage picked.  Sums are max-subtracted, run in fp64 in a fixed order (a slot's value
                               depends neither on the batch size nor on the slot), -inf entries add 0, a -inf target gives -inf.
                               Valid with every configuration vx_create accepts.  The sampler and the NAR argmax run as separate
                               instantiations / kernels chosen on the host: without the flag the launches, the graph, the tokens and
                               the allocations are what they were.  Cost: one fp32 per pass (and per slot), (Q-1) fp32 per NAR row
                                */
};

/* Mirrors VALLE.__init__ (valle.py:727-760) / get_model (models/__init__.py:112-124). */
typedef struct vx_config {
  int32_t struct_size;     /* = sizeof(vx_config) */
  int32_t d_model;         /* --decoder-dim: multiple of 8, <= 1024 */
  int32_t nhead;           /* --nhead: d_model / nhead in {4, 8, 16, 32, 64}; 64 is the tuned geometry, the others run on plain kernels (batch-1) */
  int32_t num_layers;      /* --num-decoder-layers */
  int32_t nar_d_model;     /* int(d_model * scale_factor), valle.py:83 */
  int32_t nar_nhead;       /* int(nhead * scale_factor),   valle.py:234 */
  int32_t nar_num_layers;  /* int(L * scale_factor),       valle.py:241 */
  int32_t num_quantizers;  /* --num-quantizers (1..8) */
  int32_t prefix_mode;     /* --prefix-mode 0/1/2/4 */
  int32_t prepend_bos;     /* --prepend-bos */
  int32_t precision;       /* enum vx_precision */
  int32_t max_text;        /* capacity: phoneme ids per utterance */
  int32_t max_audio;       /* capacity: audio rows = [BOS] + prompt frames + generated frames */
  int32_t device;          /* HIP device ordinal */
  int32_t flags;           /* enum vx_flags */
  int32_t max_batch;       /* slots for batched AR decode (vx_batch_*): 0/1 = batch-1 only, <= 64; bf16 only, head_dim 64 and
                              d_model in {128, 256, 512, 1024} (else VX_ERR_UNSUPPORTED, before any HIP call) */
} vx_config;

/* Sampling / stop-rule parameters of one AR decode (VALLE.inference args top_k, temperature,
 * valle.py:967-968; topk_sampling valle.py:1287-1302).  The filters run in the reference's order: logits / temperature,
 * top-k, then the nucleus (top-p) filter of top_k_top_p_filtering (valle.py:1262-1282), then the multinomial.  top_p: 0
 * (what every zero-initialised struct holds) or any value >= 1 is off; a value in (0, 1) keeps the smallest prefix of the
 * sorted (tempered, top-k-filtered) distribution whose cumulative probability exceeds top_p, the largest token always, and
 * every token tied with the boundary token; what top-k removed stays removed.  NaN or a negative value: VX_ERR_ARG, before
 * any HIP call (vx_ar_decode, vx_batch_decode, vx_batch_admit).  Per utterance: the slots of one batch or session may mix
 * top_p values. */
typedef struct vx_decode_params {
  int32_t struct_size;
  int32_t top_k;            /* <= 0: no filtering (the reference default -100) */
  float temperature;        /* logits / temperature when != 1.0 */
  int32_t max_new_tokens;   /* < 0: reference stop rule only */
  const float* exp_noise;   /* optional (noise_rows, 1025) Exp(1) draws, row i feeds pass i:      */
  int64_t noise_rows;       /*   sample = argmax(p / q) == torch.multinomial(p, 1) on that stream  */
  uint64_t seed;            /* device counter RNG seed, used when exp_noise == NULL */
  const int64_t* forced;    /* optional teacher forcing: token appended at pass i = forced[i]     */
  int32_t n_forced;         /*   (the sample is still drawn and recorded); decode ends after them */
  float top_p;              /* nucleus filter: 0 or >= 1 = off, (0, 1) = on (fills the tail padding: sizeof stays 56) */
} vx_decode_params;

const char* vx_last_error(void);

/* VALLE(...) constructor + .to(device) (valle.py:727-760; bin/infer.py:137,147). */
int vx_create(const vx_config* cfg, vx_engine** out);
void vx_destroy(vx_engine* e);

/* model.load_state_dict(checkpoint["model"], strict=True) (bin/infer.py:139-143), one tensor
 * at a time.  `key` is the reference state_dict key, `data` fp32 (host or device), row-major. */
int vx_set_weight(vx_engine* e, const char* key, const float* data, const int64_t* shape, int32_t ndim);
/* Optional: the fp32 sine table of SinePositionalEmbedding (modules/embedding.py:75-88),
 * (rows, dim) with rows >= max(4000, max_text + max_audio).  which: 0 = AR width, 1 = NAR width.  If never set, the engine fills it with
 * host sinf/cosf (same formula; may differ from torch's table in the last ulp). */
int vx_set_sine_table(vx_engine* e, int32_t which, const float* data, int64_t rows, int64_t dim);
/* strict=True check (every key present) + model.eval(); precomputes the per-stage AdaptiveLayerNorm
 * scale/shift vectors (modules/transformer.py:93-108, constant per stage at inference). */
int vx_finalize_weights(vx_engine* e);

/* valle.py:994-1010 + the first pass of the AR loop (valle.py:1012-1039): embeds text and
 * codebook-0 prompt (+BOS), runs the AR stack under the reference mask, fills the KV cache and
 * leaves the logits of pass 0.  text: (S,), prompt_cb0: (P,). */
int vx_ar_prefill(vx_engine* e, const int64_t* text, int32_t S, const int64_t* prompt_cb0, int32_t P, void* stream);

/* The AR while-loop (valle.py:1012-1057): sample, stop test, append, next pass.  Asynchronous
 * w.r.t. the host except for periodic polls of the stop flag. */
int vx_ar_decode(vx_engine* e, const vx_decode_params* p, void* stream);

/* Blocks until the decode has finished.  tokens: host buffer of `capacity` int64 (generated
 * codebook-0 tokens, valle.py:1059).  n_pass = number of logits rows produced. */
int vx_ar_result(vx_engine* e, int64_t* tokens, int32_t capacity, int32_t* n_tokens, int32_t* stop_reason,
                 int32_t* n_pass);

/* The NAR stages (valle.py:1063-1134).  text_nar: (S2,) phoneme ids after the prefix_mode 2/4
 * trim (done by the host shim, valle.py:1068-1079); prompts: (P, Q) row-major; ar_tokens: (T,);
 * codes_out: (T, Q) int64 row-major, column 0 = ar_tokens (valle.py:1136-1137). */
int vx_nar(vx_engine* e, const int64_t* text_nar, int32_t S2, const int64_t* prompts, int32_t P,
           const int64_t* ar_tokens, int32_t T, int64_t* codes_out, void* stream);
/* vx_nar / vx_nar_continual (continual != 0) with two parity-test options.  forced_codes (optional, (T, Q) int64): stage i
 * still reports its own argmax in codes_out[:, i+1], but the embedding fed to the later stages (valle.py:1133-1134) is taken from
 * forced_codes[:, i+1] - with the reference's codes this gives every stage exactly the input the reference gave it, so bf16 / fp8
 * engines can be compared stage by stage.  stage_logits (optional, (Q-1, T, 1024) fp32, host or device): the logits rows of every
 * stage (valle.py:1128). */
int vx_nar_ex(vx_engine* e, const int64_t* text_nar, int32_t S2, const int64_t* prompts, int32_t P,
              const int64_t* ar_tokens, int32_t T, int64_t* codes_out, const int64_t* forced_codes, float* stage_logits,
              int32_t continual, void* stream);
/* VALLE.continual's NAR body (valle.py:1185-1236): same arguments as vx_nar.  Differs from vx_nar only for models with
 * prenets in prefix mode 0, where continual() applies the audio position BEFORE the audio prenet (valle.py:1193-1194). */
int vx_nar_continual(vx_engine* e, const int64_t* text_nar, int32_t S2, const int64_t* prompts, int32_t P,
           const int64_t* ar_tokens, int32_t T, int64_t* codes_out, void* stream);

/* VX_FLAG_LOGPROBS: lp of the last vx_ar_decode, n = n_pass values into the HOST buffer `out` (out NULL: only *n).  No flag:
 * VX_ERR_UNSUPPORTED; no finished decode: VX_ERR_STATE; capacity < n_pass: VX_ERR_CAPACITY.  Blocks like vx_ar_result. */
int vx_ar_logprobs(vx_engine* e, float* out, int32_t capacity, int32_t* n);
/* The same for a slot of vx_batch_decode or of a session.  In a session it must be read while the slot is STOPPED, i.e. before the
 * vx_batch_result that vacates it (else VX_ERR_STATE). */
int vx_batch_logprobs(vx_engine* e, int32_t slot, float* out, int32_t capacity, int32_t* n);
/* Utterance `utt` of the last vx_nar / vx_nar_ex / vx_nar_continual / vx_nar_batch / vx_nar_batch_ex call (kept on the device until
 * the next one): out (Q-1, T) fp32 row-major, host or device, capacity in elements.  Under forced_codes the value is still that of
 * the stage's own argmax, which is what codes_out reports.  Same error rules as above; utt outside the call: VX_ERR_ARG. */
int vx_nar_logprobs(vx_engine* e, int32_t utt, float* out, int64_t capacity);

/* ---- batched AR decode (BASELINE configs[2]): up to max_batch utterances ("slots") advance one token per
 * step and share one stream of the weights; every slot has its own padded KV cache, stop rule and sampler
 * (the reference is batch-1, valle.py:989: each slot reproduces one independent inference() call).
 * vx_batch_prefill = vx_ar_prefill into a slot; vx_batch_decode runs the shared step until every one of
 * slots [0, n_slots) has stopped (params[i] for slot i; exp_noise / forced must be DEVICE pointers that stay
 * valid during the call); vx_batch_result = vx_ar_result of a slot.  The NAR stages then run per utterance
 * with vx_nar.  VALL-F engines (VX_FLAG_VALLF): vx_batch_prefill also writes the slot's text memory; the step adds each layer's
 * cross-attention over it. */
int vx_batch_prefill(vx_engine* e, int32_t slot, const int64_t* text, int32_t S, const int64_t* prompt_cb0, int32_t P,
                     void* stream);
/* All n slots' prefills in one pass over the concatenated rows (slot z = utterance z): same contract as n calls of
 * vx_batch_prefill(z, text[z], S[z], prompt_cb0[z], P[z]); bf16 VALL-E engines, and VALL-F engines created with
 * VX_FLAG_VALLF_ROWS (the rows are then the audio rows only, every slot's text memory is written through the same slot map; other
 * VALL-F engines: VX_ERR_UNSUPPORTED).  The pointer arrays and S / P live on the host, text[z] / prompt_cb0[z] may be host or device pointers. */
int vx_batch_prefill_all(vx_engine* e, int32_t n, const int64_t* const* text, const int32_t* S,
                         const int64_t* const* prompt_cb0, const int32_t* P, void* stream);
int vx_batch_decode(vx_engine* e, int32_t n_slots, const vx_decode_params* params, void* stream);
int vx_batch_result(vx_engine* e, int32_t slot, int64_t* tokens, int32_t capacity, int32_t* n_tokens,
                    int32_t* stop_reason);

/* ---- continuous batching: a session over all max_batch slots in which finished utterances leave and new ones enter while the
 * others keep decoding (bf16 engines with max_batch >= 2).  Every slot is VACANT, LIVE (admitted, decoding) or STOPPED (finished,
 * result not read yet).  The step always runs over all max_batch slots (the graph vx_batch_decode uses at n_slots = max_batch);
 * vacant and stopped slots skip the sampling, the K / V append, the attention and the logits.
 *   vx_batch_open   ends any earlier session and makes every slot vacant (device state done, row 0; the slot's residual and
 *                   logits rows zeroed).
 *   vx_batch_admit  prefills n utterances into the given vacant slots and arms them with params[z]; the other slots' KV caches,
 *                   rows and state are not touched.  Checks as vx_batch_prefill_all / vx_batch_decode (capacity clamp included).
 *                   A slot outside [0, max_batch) or given twice: VX_ERR_ARG; a live or stopped-unread slot: VX_ERR_STATE.
 *                   mode VX_ADMIT_BATCHED prefills all n in one pass over the concatenated rows (one synchronisation);
 *                   VX_ADMIT_PER_SLOT runs vx_batch_prefill's path per slot (one synchronisation each; bitwise the static path).
 *                   VALL-F engines without VX_FLAG_VALLF_ROWS admit per slot only: VX_ADMIT_BATCHED returns VX_ERR_UNSUPPORTED.
 *                   exp_noise / forced must be DEVICE pointers that stay valid until the slot's result is read.
 *   vx_batch_run    replays the step until at least min_stopped (< 1: 1) live slots have stopped in this call, or none is left
 *                   live; polls the stop flags every poll_steps steps (<= 0: the default).  stopped (capacity
 *                   max_batch) receives the slots that stopped, n_stopped their number; vx_batch_result(slot) then returns a
 *                   slot's tokens and stop reason and makes it vacant.  VX_ERR_CAPACITY as in vx_batch_decode, naming the slot
 *                   (stopped / n_stopped are still filled); VX_ERR_STATE without an open session.
 * vx_batch_prefill, vx_batch_prefill_all and vx_batch_decode end the session. */
enum vx_admit_mode { VX_ADMIT_BATCHED = 0, VX_ADMIT_PER_SLOT = 1 };
int vx_batch_open(vx_engine* e, void* stream);
int vx_batch_admit(vx_engine* e, int32_t n, const int32_t* slots, const int64_t* const* text, const int32_t* S,
                   const int64_t* const* prompt_cb0, const int32_t* P, const vx_decode_params* params, int32_t mode, void* stream);
int vx_batch_run(vx_engine* e, int32_t min_stopped, int32_t poll_steps, int32_t* stopped, int32_t* n_stopped, void* stream);

/* The NAR stages of n (<= 32) utterances in one pass: rows are concatenated so the GEMMs run at M ~ n x 1k.
 * Arguments are arrays of n pointers / sizes with the meaning of vx_nar's.  VALL-E engines, and VALL-F engines created with
 * VX_FLAG_VALLF_ROWS (every S2 <= max_text, else VX_ERR_CAPACITY naming the utterance; other VALL-F engines: VX_ERR_UNSUPPORTED). */
int vx_nar_batch(vx_engine* e, int32_t n, const int64_t* const* text_nar, const int32_t* S2,
                 const int64_t* const* prompts, const int32_t* P, const int64_t* const* ar_tokens, const int32_t* T,
                 int64_t* const* codes_out, void* stream);

/* vx_nar_batch with per-stage teacher forcing: forced_codes[i] = (T_i, Q) int64 as in vx_nar_ex, or forced_codes == NULL. */
int vx_nar_batch_ex(vx_engine* e, int32_t n, const int64_t* const* text_nar, const int32_t* S2,
                    const int64_t* const* prompts, const int32_t* P, const int64_t* const* ar_tokens, const int32_t* T,
                    int64_t* const* codes_out, const int64_t* const* forced_codes, void* stream);

/* ---- scoring: how well does the model predict GIVEN codes.  The reference reports this as its validation numbers: VALLE.forward
 * computes F.cross_entropy(reduction="sum") and MulticlassAccuracy(top_k=10, ignore_index=1024) for the AR decoder
 * (valle.py:827-881) and for a NAR stage (valle.py:886-950).  vx_score computes the per-row terms of both, teacher-forced, on the
 * inference prompt layout: codes (A, Q) int64 row-major (host or device), frames [0, P) are the prompt, frames [P, A) are scored,
 * T = A - P.
 *   AR  (valle.py:863-877): rows [text | (BOS) codes[:, 0]] go through the AR stack ONCE under the reference mask (text rows see
 *       text, audio rows are causal; VALL-F: the text is the cross-attention memory), no KV cache is written; the T + 1 rows that
 *       predict codes[P, 0] ... codes[A-1, 0], EOS give nll_ar[j] = logsumexp(logits_j) - logits_j[target_j] and rank_ar[j] = the
 *       number of logits strictly greater than the target's (ties count for the target; top-k accuracy = rank < k).  Without
 *       prepend_bos these are input rows P-1 ... A-1, so P >= 1 is required; with it rows P ... A, and P = 0 (or P = 1 without
 *       BOS) is the reference's validation form at batch size 1: sum(nll_ar) is its summed AR loss, mean(rank_ar[target != 1024]
 *       < 10) its ArTop10Accuracy.
 *   NAR (valle.py:886-950 / 1063-1134): stage i = 0 .. Q-2 runs as in vx_nar_ex with prompts = codes[:P], codebook 0 =
 *       codes[P:, 0] and forced_codes = codes[P:]; its logits rows are scored against codes[P:, i+1] into nll_nar[i][t] /
 *       rank_nar[i][t] ((Q-1, T) row-major).  Q = 1 models skip this part.  text_nar / S2 as for vx_nar.
 * Outputs may be host or device memory; any may be NULL, and a part whose two outputs are both NULL is skipped with its inputs
 * unread (text for AR, text_nar for NAR).  Checked before any work is enqueued: null arguments, P outside [0, A), S <= 0 ->
 * VX_ERR_ARG; weights not finalised -> VX_ERR_STATE; S > max_text or A + 1 > max_audio -> VX_ERR_CAPACITY; codes in host memory
 * outside [0, 1024) -> VX_ERR_ARG (device codes are clamped by the embedding, and an out-of-range TARGET scores nll = NaN, rank =
 * -1).  Every precision mode serves it; VX_PREC_FP8_NAR runs the stages on MXFP8 under the row threshold of vx_nar.  No decode
 * state is touched: a vx_ar_decode after vx_ar_prefill + vx_score, or a session's slots, continue as if it had not run. */
int vx_score(vx_engine* e, const int64_t* text, int32_t S, const int64_t* text_nar, int32_t S2, const int64_t* codes /* (A, Q) */,
             int32_t A, int32_t P, float* nll_ar /* (T+1) */, int32_t* rank_ar /* (T+1) */, float* nll_nar /* (Q-1, T) */,
             int32_t* rank_nar /* (Q-1, T) */, void* stream);
/* vx_score of n (<= 64) utterances in one pass over the concatenated rows: the AR part as vx_batch_prefill_all's segmented stack
 * (per-segment prefix masks, no KV destination), the NAR part as vx_nar_batch_ex's.  Arguments are host arrays of n pointers /
 * sizes with vx_score's meaning; output arrays may be NULL as there.  Works on engines of any max_batch.  bf16 / fp8nar VALL-E
 * with the MFMA row kernels and without prenets; anything else: VX_ERR_UNSUPPORTED (use vx_score per utterance). */
int vx_score_batch(vx_engine* e, int32_t n, const int64_t* const* text, const int32_t* S, const int64_t* const* text_nar,
                   const int32_t* S2, const int64_t* const* codes, const int32_t* A, const int32_t* P, float* const* nll_ar,
                   int32_t* const* rank_ar, float* const* nll_nar, int32_t* const* rank_nar, void* stream);

/* ---- alignment: the attention the AR decoder pays to the text while it predicts each frame, and per-token timestamps from it.
 * The utterance is laid out as for vx_score (codes (A, Q), frames [0, P) the prompt, T = A - P) and goes through the same
 * teacher-forced row pass; row i of the outputs is the input row that predicts frame P + i (the row that predicts EOS is not
 * included).  For every tapped layer l and head h, p_lh[i, s] is the softmax probability that row puts on text token s: in VALL-E
 * the text columns of its self-attention (the softmax runs over all S text keys and the audio keys up to the row itself), in
 * VALL-F its cross-attention over the S memory keys.  This is what the reference's attention module returns with
 * need_weights=True (modules/activation.py:205-251), which its layers never ask for.
 *   attn (T, c1 - c0) fp32       sum_lh head_w[l, h] p_lh[i, c0 + j], the text window [c0, c1), 0 <= c0 < c1 <= S
 *   mass (T) fp32, nullable      sum_lh head_w[l, h] sum_{s < S} p_lh[i, s]: the weighted share of the row's attention that goes
 *                                to the text at all (1 for VALL-F)
 *   path (T) int32, nullable     the monotonic path j(0) = 0, j(T-1) = c1 - c0 - 1, steps of 0 or 1, that maximises
 *   path_score double, nullable    sum_i log(max(attn[i, j(i)], FLT_MIN)), computed in fp64, ties staying in the column;
 *                                T < c1 - c0 admits no such path: path is all -1 and path_score -inf, which is not an error
 *   per_head (L, H, T, c1 - c0) fp32, nullable   p_lh itself, every layer and head, zero-weight ones included
 * head_w: HOST array (L, H) fp32 of weights used as given, or NULL for the uniform 1 / (L H); a layer whose weights are all zero
 * is not tapped unless per_head is wanted.  Outputs may be host or device memory.  The sum over heads and layers runs in a fixed
 * order without atomics: the same call gives the same bits.  Checked before any work is enqueued: the checks of vx_score's AR part
 * (P = 0 needs prepend_bos); a window outside the text, a negative or non-finite weight, all weights zero -> VX_ERR_ARG; S >
 * max_text, A + 1 > max_audio, or a path over more than 4096 text tokens -> VX_ERR_CAPACITY.  Every engine vx_score serves; no
 * decode state is touched. */
int vx_align(vx_engine* e, const int64_t* text, int32_t S, const int64_t* codes /* (A, Q) */, int32_t A, int32_t P, int32_t c0,
             int32_t c1, const float* head_w /* (L, H) host, nullable */, float* attn /* (T, c1-c0) */, float* mass /* (T) */,
             int32_t* path /* (T) */, double* path_score, float* per_head /* (L, H, T, c1-c0) */, void* stream);

/* vx_align of n utterances in one pass over the concatenated rows (the rows of vx_score_batch).  text, S, codes, A, P, c0, c1, attn,
 * mass, path, path_score: HOST arrays of n pointers / sizes with vx_align's meaning; head_w is shared by all utterances.  mass, path
 * and path_score may be NULL, and so may any of their entries; the paths of all utterances that asked for one run side by side in
 * one launch.  There is no per_head here: finding heads stays with vx_align.  The tap runs on the matrix pipe
 * (attn_text_seg_kernel, bf16 operands, fp32 accumulation): the maps agree with vx_align's within the bf16 bound of DESIGN.md 4.7,
 * not bit for bit.  An utterance's results do not depend on the others of the call, and the same call gives the same bits.  Served:
 * the engines of vx_score_batch that are pre-norm - bf16 / fp8nar VALL-E with the MFMA row kernels (head_dim 64), no prenets - and
 * n <= 64, on engines of any max_batch; anything else: VX_ERR_UNSUPPORTED (use vx_align per utterance).  The checks are vx_align's,
 * per utterance, and name the utterance; all are made before any work is enqueued.  No decode state is touched; out[12] of
 * vx_get_timings reports the call. */
int vx_align_batch(vx_engine* e, int32_t n, const int64_t* const* text, const int32_t* S, const int64_t* const* codes, const int32_t* A,
                   const int32_t* P, const int32_t* c0, const int32_t* c1, const float* head_w /* (L, H) host, nullable */,
                   float* const* attn, float* const* mass, int32_t* const* path, double* const* path_score, void* stream);

/* Device-time of the last calls, measured with HIP events on the engine's stream:
 * out[0] prefill ms, out[1] AR decode ms, out[2] NAR ms, out[3] AR passes, out[4] graph launches, out[5] batched decode ms,
 * out[6] batched graph launches; with VX_TIME_GEMMS=1 in the environment also out[7] = ms spent in the QKV / out-projection / FFN
 * GEMM launches of the last NAR call and out[8] = their FLOPs (2 M N K each); out[9] kernel launches per pass of the batch-1 decode
 * step (nodes of its captured graph; 0 before the first vx_ar_decode and with VX_FLAG_NO_GRAPH); out[10] / out[11] ms of the AR / NAR
 * part of the last vx_score or vx_score_batch; out[12] ms of the last vx_align or vx_align_batch (row set-up, stack, taps and path). */
int vx_get_timings(vx_engine* e, double* out, int32_t n);

/* Parity-test taps: copies an internal buffer to host memory (synchronises the engine stream).
 * names: "ar_logits" (n_pass x 1025 fp32 with VX_FLAG_TRACE_LOGITS, else the last row),
 * "ar_sampled" / "ar_argmax" (int32 per pass), "nar_logits" (T x 1024 fp32 of the last stage),
 * "ar_x" (d fp32 residual stream of the last AR row), "nar_x" (N x d fp32 after the last stage),
 * "batch_logits" (64 x 1088 fp32: newest logits row of every slot), "batch_argmax" / "batch_sampled"
 * (64 x (max_audio+2) int32 per pass), "batch_trace" (max_batch x (max_audio+2) x 1025 fp32: every pass's logits row of every
 * slot, engines created with VX_FLAG_TRACE_LOGITS and max_batch > 1), "batch_kv" (the slot caches, max_batch > 1:
 * [slot][layer][K|V][head][max_text+max_audio][64] bf16, or e4m3 bytes with VX_FLAG_KV_FP8), "batch_kv_scale" (VX_FLAG_KV_FP8: the
 * E8M0 scale bytes, [slot][layer][K|V][head][max_text+max_audio][4]), "ar_kv" (the batch-1 KV cache,
 * [layer][K|V][head][max_text+max_audio][head_dim], fp32 on VX_PREC_F32 engines, else bf16), "ar_mem" (VX_FLAG_VALLF engines only:
 * the text memory the batch-1 cross-attention reads, K and V of every layer from the last prefill's text,
 * [layer][K|V][head][max_text][head_dim] in ar_kv's element type; rows at and past that text's length keep what an earlier,
 * longer text left there and are never read), "score_ar_argmax" (int32 per AR row
 * of the last vx_score / vx_score_batch, utterances concatenated: the argmax of the scored logits rows), "tp_wo" (engines that run
 * the XCD-sharded decode step only: layer 0's out-projection in the word order that step streams, d x d elements of the weight
 * type - the layout test of csrc/ar_tp.hpp tp_repack_kernel). */
int vx_read_buffer(vx_engine* e, const char* name, void* dst, int64_t offset_bytes, int64_t nbytes);

/* Bytes vx_read_buffer's tap `name` holds on an engine created with *cfg, for the taps whose size follows from the
 * configuration alone ("ar_kv"; "ar_mem" with VX_FLAG_VALLF in cfg->flags); VX_ERR_ARG for any other name.  Host only: no HIP
 * call. */
int vx_buffer_bytes(const vx_config* cfg, const char* name, int64_t* bytes);

/* Kernel-level entry points (device pointers, fp32 unless noted) used by tests/ to check each
 * HIP kernel against the oracle's corresponding torch op.  prec selects the storage type the
 * kernel is instantiated for (weights / KV: fp32 or bf16).  All run on `stream` and return
 * after enqueueing. */
int vx_op_layernorm(int32_t prec, const float* x, const float* gamma, const float* beta, const float* ada_w,
                    const float* ada_b, void* out /* fp32 or bf16 per prec */, int32_t rows, int32_t d, void* stream);
int vx_op_gemv(int32_t prec, const void* W, const float* bias, const float* x, float* y, int32_t N, int32_t K,
               int32_t relu, void* stream);
int vx_op_gemm(int32_t prec, int32_t use_mfma, const void* A, const void* W, const float* bias, float* C_f32,
               int32_t M, int32_t N, int32_t K, int32_t relu, void* stream);
/* The bf16 MFMA GEMM in the forms the engine's row path launches (mfma_gemm_dispatch; reference op: F.linear inside
 * valle/modules/transformer.py:296-334): form 0: C (M, N) bf16 = A.W^T + bias [ReLU] (QKV / FFN1), optionally with the last
 * N - vt_n0 columns (vt_n0 a multiple of 64) also written transposed to vt (N - vt_n0, vt_ld) bf16 (the V^T copy the attention
 * kernel reads; vt may be NULL); form 1: C (M, N) fp32 += A.W^T + bias (out-projection / FFN2 onto the residual stream). */
int vx_op_gemm_rows(int32_t form, const void* A_bf16, const void* W_bf16, const float* bias, void* C, int32_t M, int32_t N,
                    int32_t K, int32_t relu, void* vt_bf16, int32_t vt_n0, int32_t vt_ld, void* stream);
/* The split-K construction of the row path's N = d GEMMs (out-projection, FFN2 at M < 4096 rows), piece by piece on caller
 * data, through the launchers the engine's stack calls.
 * vx_op_gemm_partial: slab z (M, N) fp32 of slabs (splits, M, N) = A[:, z K / splits : (z + 1) K / splits] . W[:, same]^T on bf16
 * A (M, K), W (N, K); no bias.  N % 128 == 0, splits in {1, 2, 4}, K % (64 splits) == 0 (else VX_ERR_UNSUPPORTED); null operands or
 * M < 1: VX_ERR_ARG.
 * vx_op_ln_fold: the row LayerNorm with its optional arguments.  part != NULL: x[r] + (pbias + part[0][r] + ... +
 * part[nsplit-1][r]) (in that order; slab z at part + z part_stride, nsplit in 1..4) replaces the row first; it is written back
 * to x unless xout redirects the result.  out (fp32 or bf16 per prec) = [ada_w *] (LN(row) gamma + beta) [+ ada_b]; xout (fp32,
 * may alias x) receives the same values unrounded, and x itself is then left as it was.  out == NULL: fold only (needs part).
 * d a multiple of 4, <= 1024 (else VX_ERR_UNSUPPORTED); part without pbias, xout without out, out without gamma / beta: VX_ERR_ARG.
 * vx_op_rows_plan: out[3] = {split-K on, K slices of the out-projection, of FFN2} as the stack chooses them over M rows of
 * width d on a bf16, head_dim 64 engine without MXFP8 or a text memory, for num_cu compute units (<= 0: the current device's;
 * with an explicit count the call is host only).
 * All three check their arguments before any HIP call and return after enqueueing on `stream`. */
int vx_op_gemm_partial(const void* A_bf16, const void* W_bf16, float* slabs, int32_t M, int32_t N, int32_t K, int32_t splits,
                       void* stream);
int vx_op_ln_fold(int32_t prec, float* x, const float* part, int32_t nsplit, int64_t part_stride, const float* pbias,
                  const float* gamma, const float* beta, const float* ada_w, const float* ada_b, void* out, float* xout, int32_t rows,
                  int32_t d, void* stream);
int vx_op_rows_plan(int32_t M, int32_t d, int32_t num_cu, int32_t* out);
/* The MXFP8 (VX_PREC_FP8_NAR) kernels on caller data.  vx_op_gemm_mx: A (M, K) / W (N, K) fp32 device pointers are quantised
 * on the device as the engine does (e4m3 + one E8M0 scale per 32 k) and multiplied on the block-scaled matrix cores; out_mode 0:
 * c_out = C (M, N) fp32 (+bias, ReLU); out_mode 2 (FFN1's form): c_out = ReLU(C + bias) as e4m3 bytes (M, N), sc_out = its block
 * scales (N/32, ld), ld = M rounded up to 256.  qa_out / sa_out (optional): the quantised A and its scales (K/32, ld).
 * vx_op_layernorm_mx: LayerNorm / AdaLN with the quantised result, q_out (rows, d) bytes + s_out (d/32, ld) scales. */
int vx_op_gemm_mx(const float* A, const float* W, const float* bias, void* c_out, void* sc_out, int32_t M, int32_t N, int32_t K,
                  int32_t relu, int32_t out_mode, void* qa_out, void* sa_out, void* stream);
int vx_op_layernorm_mx(const float* x, const float* gamma, const float* beta, const float* ada_w, const float* ada_b, void* q_out,
                       void* s_out, int32_t rows, int32_t d, void* stream);
int vx_op_attention(int32_t prec, int32_t use_mfma, const void* qkv, void* out, int32_t rows, int32_t nhead,
                    int32_t hd, int32_t text_len_for_ar_mask /* <0: no mask */, void* stream);
/* The segmented flash attention of batched NAR / batched prefill: qkv (rows, 3 nhead hd) bf16, hd == 64; segment z is rows
 * [seg_start[z], seg_start[z] + seg_len[z]) (starts multiples of 64, increasing, not overlapping), with its own prefix mask
 * seg_text[z] in [0, seg_len[z]] (seg_text NULL: no mask).  Segment arrays on the host; out rows outside the segments are not
 * written.  A bad layout is VX_ERR_ARG before any HIP call.  Synchronises `stream`. */
int vx_op_attention_segs(const void* qkv, void* out, int32_t rows, int32_t nhead, int32_t hd, int32_t nseg, const int32_t* seg_start,
                         const int32_t* seg_len, const int32_t* seg_text /* nullable */, void* stream);
/* The segmented cross-attention of the VALL-F row passes (VX_FLAG_VALLF_ROWS): q (rows, ldq) bf16, head h at columns [64 h, 64 h +
 * 64), ldq >= 64 nhead and a multiple of 8; out (rows, 64 nhead) bf16.  Segments as in vx_op_attention_segs.  Segment z attends to all
 * klen[z] keys of its own memory and to nothing else: element (head h, key j, channel c) of K at mem + mem_off[z] + h head_stride +
 * 64 j + c, V at the same index + v_offset (bf16 elements; mem_off, head_stride and v_offset non-negative multiples of 8,
 * 1 <= klen[z] <= head_stride / 64).  Memory rows at and past klen[z] are never read.  mem_off / klen: host arrays.  out rows
 * outside the segments are not written.  A bad layout is VX_ERR_ARG before any HIP call.  Synchronises `stream`. */
int vx_op_cross_attention_segs(const void* q, int32_t ldq, const void* mem, const int64_t* mem_off, int64_t head_stride,
                               int64_t v_offset, const int32_t* klen, void* out, int32_t rows, int32_t nhead, int32_t nseg,
                               const int32_t* seg_start, const int32_t* seg_len, void* stream);
/* The batched decode step's attention over B slot caches (kv_fp8: the e4m3 codes + E8M0 scale bytes, else bf16): q (B, 64 nhead)
 * fp32, out (B, 64 nhead) bf16; slot b's K at kv + b slot_stride, V at + v_offset (elements), element (h ctx_max + j) 64 + c,
 * scales at that index >> 4 of kv_scale.  ctx / done: host arrays; slot b attends to keys [0, ctx[b]); done slots are skipped
 * (their out rows are not written).  Synchronises `stream`. */
int vx_op_attn_slots(int32_t kv_fp8, const float* q, const void* kv, const void* kv_scale, int64_t slot_stride, int64_t v_offset,
                     int32_t ctx_max, int32_t B, int32_t nhead, const int32_t* ctx, const int32_t* done /* nullable */, void* out,
                     void* stream);
/* The VALL-F slot step's cross-attention over B slots' text memory: q (B, 64 nhead) fp32, mem bf16, out (B, 64 nhead) bf16; slot b's
 * K at mem + b slot_stride, V at + v_offset (elements, multiples of 8), element (h max_text + j) 64 + c.  len / done: host arrays;
 * slot b attends to keys [0, len[b]), 1 <= len[b] <= max_text; done slots are skipped (their out rows are not written).
 * Synchronises `stream`. */
int vx_op_attn_mem_slots(const float* q, const void* mem, int64_t slot_stride, int64_t v_offset, int32_t max_text, int32_t B,
                         int32_t nhead, const int32_t* len, const int32_t* done /* nullable */, void* out, void* stream);
/* One launch of the batched step's GEMM (bgemm_kernel; C[b][n] = sum_k A[b][k] W[n][k] on bf16 A (32 rows if B <= 32, else 64;
 * rows >= B are read but unused) and W (N, K)) in its epilogue epi: 0 QKV (q (B, d) fp32 = C + bias for n < d; the K / V columns
 * go to row row[b] of live slots' caches, indexed as in vx_op_attn_slots (hd 64): bf16 kv, or with kv8 e4m3 codes in kv and E8M0
 * scale bytes in kv8s), 1 RELU (f (B, N) bf16 = ReLU(C + bias)), 2 PARTIAL (part[g][b][n] fp32, (kgroups, 64, N): the sum over
 * K group g), 3 LOGITS (logits[b * logits_stride + n] = C for live slots, and trace[(b trace_rows + pass[b]) N + n] when trace
 * != NULL and pass[b] < trace_rows), 4 LOGITS_MAP (3 with row z written to slot slot_map[z]; done / pass indexed by slot),
 * 5 BIAS (q (B, N) fp32 = C + bias).  K = ns kgroups 128 with ns in {1, 2, 4, 8}; kgroups > 1 for PARTIAL only.  done / row /
 * pass: host arrays (nullable: zeros) of B entries, 64 for LOGITS_MAP; slot_map: host.  Bad arguments: VX_ERR_ARG before any
 * HIP call.  Synchronises `stream`. */
int vx_op_bgemm(int32_t epi, int32_t kv8, const void* A_bf16, const void* W_bf16, const float* bias, int32_t N, int32_t K, int32_t B,
                int32_t kgroups, const int32_t* done, const int32_t* row, const int32_t* pass, float* q, void* kv, void* kv8s,
                int64_t kv_slot_stride, int64_t kv_v_offset, int32_t d, int32_t ctx_max, void* f_bf16, float* part, float* logits,
                int32_t logits_stride, float* trace, int32_t trace_rows, const int32_t* slot_map, void* stream);
/* The batched step's LayerNorm: kgroups 1 or 4: t = pbias + part[0][b] + ... + part[kgroups-1][b] (in that order; part
 * (kgroups, 64, d)), x[b] += t written back; kgroups 0: x only read.  Then h[b] (bf16) = LN(x[b]) gamma + beta (eps 1e-5), for
 * b < B.  slot_map (host, kgroups 0): batched prefill's form, h[z] = LN(x[slot_map[z]]).  d a multiple of 4, <= 1024.  Bad
 * arguments: VX_ERR_ARG before any HIP call.  Synchronises `stream`. */
int vx_op_ln_batch(float* x, const float* part, int32_t kgroups, const float* pbias, const float* gamma, const float* beta, void* h_bf16,
                   int32_t B, int32_t d, const int32_t* slot_map /* nullable */, void* stream);
/* The scoring reduction (nll_rows_kernel; reference op: F.cross_entropy(reduction="none") and the rank behind
 * MulticlassAccuracy(top_k), valle.py:873-881): `rows` rows of V <= 1088 fp32 logits with leading dimension ld, one int64 target
 * per row, all DEVICE pointers.  nll[r] = logsumexp(row) - row[target] (max-subtracted, summed in a fixed order: a row's result
 * does not depend on rows; -inf entries add 0; a -inf target entry gives +inf); rank[r] = entries strictly greater than the
 * target's (ties count for the target); argmax[r] = first index of the maximum (torch.argmax's rule).  A target outside [0, V):
 * nll NaN, rank -1, nothing read out of bounds.  Null pointers, rows < 1, V outside [1, 1088], ld < V: VX_ERR_ARG before any HIP
 * call. */
int vx_op_nll_rows(const float* logits, int32_t rows, int32_t V, int32_t ld, const int64_t* targets, float* nll, int32_t* rank,
                   int32_t* argmax, void* stream);
/* The attention tap of vx_align (attn_text_rows_kernel) on caller buffers, all DEVICE pointers: `rows` query rows, head h of row i
 * at q + i ldq + h hd; key j of head h at k + j ldk + h k_head_stride (elements of the type prec selects; packed (M, 3 d) rows: ldk
 * = 3 d, k_head_stride = hd; the memory layout (nhead, max_text, hd): ldk = hd, k_head_stride = max_text hd).  causal != 0: row i
 * sees keys [0, text_len + row0 + i + 1), the text keys and the audio keys up to its own (row0: audio position of row 0); causal
 * == 0: keys [0, text_len).  attn (rows, c1 - c0) += sum_h head_w[h] p_h[i, c0 + j], mass (rows, nullable) += sum_h head_w[h]
 * sum_{s < text_len} p_h[i, s] (first != 0: stored instead of added); per_head (nhead, rows, c1 - c0), nullable: p_h of every
 * head.  A zero-weight head is skipped unless per_head is given.  hd in {4, 8, 16, 32, 64}.  A row's result does not depend on
 * rows or on its place in the launch.  Bad arguments: VX_ERR_ARG before any HIP call. */
int vx_op_attn_text_rows(int32_t prec, const void* q, int64_t ldq, const void* k, int64_t ldk, int64_t k_head_stride, int32_t rows,
                         int32_t row0, int32_t nhead, int32_t hd, int32_t text_len, int32_t causal, int32_t c0, int32_t c1,
                         const float* head_w, float* attn, float* mass, float* per_head, int32_t first, void* stream);
/* The path of vx_align (mono_path_kernel) on a caller map: attn (T, Sw) fp32, path (T) int32, score (1) double, DEVICE pointers;
 * Sw <= 4096 (else VX_ERR_CAPACITY).  Synchronises `stream`. */
int vx_op_mono_path(const float* attn, int32_t T, int32_t Sw, int32_t* path, double* score, void* stream);

/* The batched tap of vx_align_batch (attn_text_seg_kernel, then the heads in head order) on caller buffers.  q / k: DEVICE bf16,
 * row i, head h at q[i * ld + h * 64 + c] (the packed (M, 3 d) rows: k = q + d, ld = 3 d).  desc: HOST, nseg x 9 values per segment:
 * start (first row, a multiple of 64), text_len, qfirst (index within the segment of the first tapped row), rows, row0 (audio index
 * of that row: tapped row i sees keys [0, text_len + row0 + i + 1) of its segment), c0, c1, cell_off, row_off (where the segment's
 * (rows, c1 - c0) cells / rows start in attn / mass).  head_w (nhead) DEVICE; attn (cells) and mass (rows_total, nullable) DEVICE
 * fp32, stored (first != 0) or added to.  Synchronises the stream. */
int vx_op_attn_text_segs(const void* q, const void* k, int64_t ld, int32_t nseg, const int64_t* desc, int32_t nhead, const float* head_w,
                         float* attn, float* mass, int64_t cells, int64_t rows_total, int32_t first, void* stream);

/* mono_path_seg_kernel: n maps in one launch, one workgroup each.  desc: HOST, n x 4 values per map: T, Sw, cell_off (of the map in
 * attn), row_off (of its path in path); score: n doubles.  attn, path, score DEVICE.  Synchronises the stream. */
int vx_op_mono_path_segs(const float* attn, int32_t n, const int64_t* desc, int32_t* path, double* score, void* stream);
int vx_op_sample(const float* logits, int32_t V, int32_t top_k, float temperature, const float* exp_noise,
                 int32_t* out_token_argmax /* [2]: sampled, argmax */, void* stream);
/* vx_op_sample with the nucleus filter after top-k (top_p as in vx_decode_params: 0 or >= 1 off, NaN / negative VX_ERR_ARG).
 * V <= 1088 runs the decode step's own sampler (the four-wave kernel every step form launches); V > 1088 with top_p on is
 * VX_ERR_UNSUPPORTED (the single-wave kernel has no nucleus stage), with top_p off it is vx_op_sample. */
int vx_op_sample_topp(const float* logits, int32_t V, int32_t top_k, float temperature, float top_p, const float* exp_noise,
                      int32_t* out_token_argmax /* [2]: sampled, argmax */, void* stream);
/* vx_op_sample_topp on the sampler instantiation of VX_FLAG_LOGPROBS: same arguments and same [sampled, argmax] result, plus
 * lp_out[0] (host) = the log-probability of the sampled token on the raw row.  V <= 1088 only (else VX_ERR_UNSUPPORTED); argument
 * checks as vx_op_sample_topp, before any HIP call. */
int vx_op_sample_logprob(const float* logits, int32_t V, int32_t top_k, float temperature, float top_p,
                         const float* exp_noise, int32_t* out_token_argmax, float* lp_out, void* stream);
int vx_op_convert_bf16(const float* src, void* dst_bf16, int64_t n, void* stream);

/* ---- EnCodec-24 kHz codec: codec tokens -> waveform (what valle/bin/infer.py:251-253 does with VALLE.inference's result
 * through valle/data/tokenizer.py:241-242) and, on a handle created with VX_CODEC_ENCODER, prompt waveform -> codec tokens
 * (tokenize_audio, valle/data/tokenizer.py:238-254).  A handle of its own: the codec has its own weights and lifetime and is
 * usable without a vx_engine.  fp32 storage and accumulation.  Geometry as transformers' EncodecConfig: the decoder is
 * conv(hidden -> 16 filters, kernel) -> LSTM + skip -> 4 x [ELU, transposed conv (k = 2 ratio, stride ratio, channels halved),
 * residual block (res_kernel, hidden width C / 2)] -> ELU -> conv(filters -> 1, last_kernel); stride-1 convolutions are causal
 * with reflect padding, weight norm is folded by the caller.  The encoder is its mirror: conv(1 -> filters,
 * kernel) -> 4 x [residual block, ELU, strided conv (k = 2 ratio, stride ratio, channels doubled; ratios in reverse order)] ->
 * LSTM + skip -> ELU -> conv(16 filters -> hidden, last_kernel) -> residual vector quantiser (nearest code per stage, first
 * index on ties).  Every convolution pads k - stride on the left and, on the right, what completes the last window (output
 * length ceil(L / stride)), both reflect. */
typedef struct vx_codec vx_codec;
enum vx_codec_flags {
  VX_CODEC_LSTM_GRAPH = 1, /* replay the LSTM's time steps as a captured linear chain instead of launching them one by one: the
                             same kernels and results; measured slower at one utterance and equal at 32 / 64,
                             so it is off by default */
  VX_CODEC_ENCODER = 2    /* the handle also encodes: vx_codec_finalize needs the encoder.* tensors as well and allocates the
                             encoder's staging; codebook_size must be a multiple of 32 and codebook_dim a multiple of 8, <= 128.
                             Without the flag nothing changes: no encoder tensor is known and vx_codec_encode is refused */
};
typedef struct vx_codec_config {
  int32_t struct_size;   /* = sizeof(vx_codec_config) */
  int32_t hidden;        /* decoder input channels (128) */
  int32_t filters;       /* num_filters (32): the LSTM runs at 16 * filters channels, which must be 64, 128, 256 or 512 */
  int32_t ratios[4];     /* up-sampling ratios in decoder order (8, 5, 4, 2) */
  int32_t kernel;        /* first convolution (7) */
  int32_t last_kernel;   /* last convolution (7) */
  int32_t res_kernel;    /* residual blocks' first convolution (3) */
  int32_t n_codebooks;   /* codebooks loaded (8 for 6 kbps; <= 32) */
  int32_t codebook_size; /* 1024 */
  int32_t codebook_dim;  /* = hidden */
  int32_t lstm_layers;   /* 1 or 2 */
  int32_t max_frames;    /* capacity: frames per utterance */
  int32_t max_batch;     /* capacity: utterances per call, <= 64 */
  int32_t device;        /* HIP device ordinal */
  int32_t flags;         /* enum vx_codec_flags */
} vx_codec_config;

/* Geometry the kernels do not serve: VX_ERR_UNSUPPORTED, before any HIP call.  Device memory is allocated by vx_codec_finalize. */
int vx_codec_create(const vx_codec_config* cfg, vx_codec** out);
void vx_codec_destroy(vx_codec* c);
/* Keys: the local EncodecModel's state_dict names with weight norm removed - decoder.layers.N.conv.weight / .bias,
 * decoder.layers.N.block.1|3.conv.*, decoder.layers.N.shortcut.conv.*, decoder.layers.1.lstm.weight_ih_l0 ... bias_hh_l1,
 * quantizer.layers.q.codebook.embed - host fp32 in torch's layouts; with VX_CODEC_ENCODER also encoder.layers.N.conv.weight /
 * .bias (N = 0, 3, 6, 9, 12, 15), encoder.layers.N.block.1|3.conv.*, encoder.layers.N.shortcut.conv.* (N = 1, 4, 7, 10) and
 * encoder.layers.13.lstm.*.  Unknown key or wrong shape: VX_ERR_WEIGHTS. */
int vx_codec_set_weight(vx_codec* c, const char* key, const float* data, const int64_t* shape, int32_t ndim);
/* Packs and uploads the weights, allocates the workspace.  A missing tensor: VX_ERR_WEIGHTS. */
int vx_codec_finalize(vx_codec* c);
/* n utterances: codes[i] HOST int64 (n_q, T[i]), wav_out[i] DEVICE fp32 of hop * T[i] samples (hop = product of the ratios,
 * 320).  Checked before any HIP call: a code outside [0, codebook_size), n_q outside [1, n_codebooks], T[i] < 1 or n < 1 ->
 * VX_ERR_ARG; T[i] > max_frames or n > max_batch -> VX_ERR_CAPACITY.  The work runs on the decoder's own stream, ordered after
 * what is already enqueued on `stream`, and `stream` waits for it before the call returns; the host waits only for the previous
 * call's staging copy.  Calls on one handle must not overlap.  A vx_codec_finalize that failed leaves a handle that answers
 * VX_ERR_STATE to finalize and decode: destroy it. */
int vx_codec_decode(vx_codec* c, int32_t n, const int64_t* const* codes, const int32_t* T, int32_t n_q, float* const* wav_out,
                    void* stream);

/* n utterances: wav[i] DEVICE fp32, n_samples[i] mono 24 kHz samples (any length >= 1, not only multiples of the hop);
 * codes_out[i] DEVICE int64 (n_q, T_i), T_i = ceil(n_samples[i] / hop).  The utterances are encoded as one ragged batch and every
 * one gets bitwise the codes it gets alone.  Checked before any HIP call, in this order (the first that applies is returned):
 * null arguments -> VX_ERR_ARG; a handle without VX_CODEC_ENCODER -> VX_ERR_STATE; n < 1 -> VX_ERR_ARG; n > max_batch ->
 * VX_ERR_CAPACITY; n_q outside [1, n_codebooks] -> VX_ERR_ARG; then per utterance in order: a null pointer or n_samples[i] < 1
 * -> VX_ERR_ARG, n_samples[i] > max_frames * hop -> VX_ERR_CAPACITY; last a handle that is not finalised -> VX_ERR_STATE.
 * Non-finite samples are not
 * checked (their codes are unspecified but in range).  Stream ordering as vx_codec_decode. */
int vx_codec_encode(vx_codec* c, int32_t n, const float* const* wav, const int32_t* n_samples, int32_t n_q, int64_t* const* codes_out,
                    void* stream);

/* Test-only (parity tests, like the vx_op_* entries below): the quantiser's input of the last vx_codec_encode on this handle
 * ([rows][hidden] fp32, the call's frames in utterance order) copied to `out` (DEVICE).  rows above that call's frame count, or
 * any rows when no encode has run since finalize or a vx_codec_decode ran after it (it reuses the buffer): VX_ERR_ARG.  Not an
 * encoder handle or not finalised: VX_ERR_STATE. */
int vx_codec_last_embeddings(vx_codec* c, float* out, int64_t rows, void* stream);

/* The codec's kernels on caller data (parity tests).  x / out: device fp32 time-major rows; w / bias: HOST fp32 in torch's
 * layouts, packed as vx_codec_finalize packs them; seg_frames: HOST nseg + 1 frame offsets (seg_frames[0] = 0) of the
 * concatenated utterances, `rate` rows per frame.  No tap and no LSTM state crosses a segment start.  Synchronous.
 * conv: w (c_out, c_in, k), causal, reflect rule, ELU on the operand when elu != 0.  convtr: w (c_in, c_out, 2 stride), the
 * stride rightmost samples trimmed, out has stride x the rows.  lstm: per layer w_ih / w_hh (4 width, width), b_ih / b_hh
 * (4 width), gate order i, f, g, o; y = lstm(x) + x. */
int vx_op_codec_conv(const float* x, const float* w, const float* bias, float* out, int32_t c_in, int32_t c_out, int32_t k,
                     int32_t elu, int32_t nseg, const int32_t* seg_frames, int32_t rate, void* stream);
int vx_op_codec_convtr(const float* x, const float* w, const float* bias, float* out, int32_t c_in, int32_t c_out, int32_t stride,
                       int32_t elu, int32_t nseg, const int32_t* seg_frames, int32_t rate, void* stream);
int vx_op_codec_lstm(const float* x, const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                     const float* const* b_hh, float* y, int32_t width, int32_t layers, int32_t nseg, const int32_t* seg_frames,
                     void* stream);

/* Encoder side.  conv_strided: x device rows of nseg utterances with HOST row offsets seg_rows_in (rate 1), w HOST (c_out, c_in,
 * k); utterance i gives ceil(len_i / stride) output rows, concatenated.  stride > 1 needs k = 2 stride; stride = 1 is the causal
 * convolution, and c_in = 1 there runs the first convolution's kernel (no ELU).  rvq_encode: emb device [rows][dim], codebooks
 * HOST [n_q][size][dim], codes_out DEVICE int32 [n_q][rows]: per stage the first index of the smallest |e|^2 - 2 r.e, then
 * r -= e.  Synchronous. */
int vx_op_codec_conv_strided(const float* x, const float* w, const float* bias, float* out, int32_t c_in, int32_t c_out, int32_t k,
                             int32_t stride, int32_t elu, int32_t nseg, const int32_t* seg_rows_in, void* stream);
int vx_op_codec_rvq_encode(const float* emb, const float* codebooks, int32_t* codes_out, int64_t rows, int32_t n_q, int32_t size,
                           int32_t dim, void* stream);

/* ---- Sample-rate conversion and mix-down in front of the encoder (what tokenize_audio does through convert_audio,
 * valle/data/tokenizer.py:245-254) and behind the decoder.  A handle of its own: no weights, no vx_codec.  The rule is the
 * Hann-windowed sinc of width 6 at roll-off 0.99: with g = gcd(orig, new), o = orig / g, n = new / g, base = 0.99 min(o, n),
 *   x[i] = mean_c in[c][i]   (fp32, channels summed in order, then divided by their count)
 *   y[j] = (base / o) sum_i x[i] sinc(pi t) cos^2(pi t / 12),  t = (i / o - j / n) base,  over |t| < 6, x = 0 outside [0, L)
 * for j < ceil(n L / o); orig == new returns x bit for bit.  The coefficients [n phases][taps] are computed in fp64 at create
 * (the scale folded in) and rounded once; a sample's products are accumulated in ascending i whatever the batch. */
typedef struct vx_resampler vx_resampler;
/* Host only, no HIP call (the table goes to the device current at the first vx_resample).  Null out, a rate <= 0 or
 * max_batch < 1 -> VX_ERR_ARG; a table above 2^24 coefficients or a rate pair whose taps do not fit the kernel's window ->
 * VX_ERR_UNSUPPORTED. */
int vx_resampler_create(int32_t orig_hz, int32_t new_hz, int32_t max_batch, vx_resampler** out);
void vx_resampler_destroy(vx_resampler* r);
/* ceil(n L / o), the samples vx_resample writes for n_samples = L; -1 for a rate <= 0 or L < 1.  Host only. */
int64_t vx_resample_length(int32_t orig_hz, int32_t new_hz, int64_t n_samples);
/* n utterances of one rate pair: in[i] DEVICE fp32 (channels[i], n_samples[i]) channel-major, out[i] DEVICE fp32 of
 * vx_resample_length(...) samples.  Every utterance is bitwise what it is alone; no tap crosses an utterance.  Checked before
 * any HIP call, in this order: null arguments or n < 1 -> VX_ERR_ARG; n > max_batch -> VX_ERR_CAPACITY; then per utterance a
 * null pointer, channels[i] < 1 or n_samples[i] < 1 -> VX_ERR_ARG, an output length beyond int32 ->
 * VX_ERR_UNSUPPORTED.  The work is enqueued on `stream`; the host waits only for the previous call's staging copy.
 * Calls on one handle must not overlap. */
int vx_resample(vx_resampler* r, int32_t n, const float* const* in, const int32_t* channels, const int32_t* n_samples,
                float* const* out, void* stream);

/* ---- log-mel filterbank (the reference's BigVGANFbank, valle/data/fbank.py:80-131) ------------------------------------------
 * A handle of its own: no weights, no vx_codec.  Per utterance, a mono fp32 waveform of L samples at 24 kHz:
 *   frames = (L + 128) / 256 (L / hop rounded half up); zeros are appended up to (frames - 1) 256 + 1024 samples (no centring,
 *   no reflection); frame f = samples [256 f, 256 f + 1024) times the periodic Hann window; one-sided DFT, bins 0..512;
 *   mag = sqrt(re^2 + im^2 + 1e-9); mel = basis (n_mels x 513) mag; out[f][m] = log(max(mel, clip)), (frames, n_mels) row-major.
 * The DFT runs as a 32 x 32 four-step factorisation on the fp32 matrix instruction with tables computed in fp64 and rounded
 * once; a filter's band is summed in ascending bin order.  A frame's bits depend on its own samples only. */
typedef struct vx_fbank vx_fbank;
typedef struct vx_fbank_config {
  int32_t struct_size;  /* sizeof(vx_fbank_config) */
  int32_t sample_rate;  /* 24000 */
  int32_t n_fft;        /* 1024 (also the window length) */
  int32_t hop;          /* 256 */
  int32_t n_mels;       /* 1 .. 128; the reference has 100 */
  float fmin, fmax;     /* band of the built-in Slaney basis, 0 <= fmin < fmax <= 12000 (the reference: 0 .. 12000) */
  float clip;           /* floor under the log, > 0 (the reference: 1e-5) */
  int32_t max_batch;    /* utterances per call */
} vx_fbank_config;
/* Host only, no HIP call (the tables go to the device current at the first extraction).  Nulls, a wrong struct_size,
 * max_batch < 1 or a clip that is not positive and finite -> VX_ERR_ARG; another geometry, n_mels or band -> VX_ERR_UNSUPPORTED.
 * The built-in basis is Slaney's: n_mels + 2 points equally spaced on the mel scale that is linear below 1 kHz (200 / 3 Hz
 * per mel) and logarithmic above (step log(6.4) / 27), triangular weights between them, each scaled by 2 / (its width in Hz);
 * fp64, rounded once. */
int vx_fbank_create(const vx_fbank_config* cfg, vx_fbank** out);
void vx_fbank_destroy(vx_fbank* fb);
/* Replaces the basis by a HOST array (n_mels x 513), dense or not; it is copied, and takes effect at the next extraction.
 * The getter copies the current one out.  Host only. */
int vx_fbank_set_mel_basis(vx_fbank* fb, const float* basis);
int vx_fbank_get_mel_basis(const vx_fbank* fb, float* basis);
/* (L + 128) / 256, the frames an utterance of n_samples = L has; 0 below 128 samples.  Host only. */
int64_t vx_fbank_frames(int64_t n_samples);
/* n utterances: wav[i] DEVICE fp32 of n_samples[i] samples, out[i] DEVICE fp32 (frames, n_mels); the pointer arrays live on
 * the host.  Every utterance is bitwise what it is alone, and two identical calls give the same bits; an utterance without
 * frames (fewer than 128 samples) writes nothing.  Checked before any HIP call, in this order: null arguments or n < 1 ->
 * VX_ERR_ARG; n > max_batch -> VX_ERR_CAPACITY; then per utterance a null pointer or n_samples[i] < 1 -> VX_ERR_ARG.  The work
 * is one launch enqueued on `stream`; the host waits only for the previous call's staging copy (and, after a new basis, for
 * the previous call).  Calls on one handle must not overlap. */
int vx_fbank_extract(vx_fbank* fb, int32_t n, const float* const* wav, const int32_t* n_samples, float* const* out, void* stream);

/* ---- dynamic time warping between two feature sequences (mel-cepstral distortion, MCD-DTW) -----------------------------------
 * A handle of its own: no weights, no vx_engine.  A pair is two fp32 DEVICE matrices A (Ta, D) and B (Tb, D), row-major,
 * 1 <= D <= 128, Ta, Tb >= 1.
 *   1. Cepstra (n_ceps >= 1; with n_ceps == 0 the rows are compared as given): every row m becomes
 *        c_k = sqrt(2 / D) sum_{n = 0 .. D-1} m_n cos(pi k (n + 1/2) / D),  k = 1 .. n_ceps <= D - 1
 *      (the orthonormal DCT-II without its 0th coefficient).  The table is computed in fp64 on the host and rounded once to fp32;
 *      a row's products (exact in fp64) are added in ascending n in fp64 and the sum is rounded once to fp32.  A row's cepstra
 *      depend on that row only.
 *   2. Local cost d(i, j) = sqrt(sum_k (a_ik - b_jk)^2), fp32: every difference is formed in fp32 first (never |a|^2 + |b|^2 -
 *      2 a.b: identical rows cost exactly 0), the squares (exact in fp64) are added in ascending k in fp64, and the root of the sum
 *      is rounded once to fp32.
 *   3. Warp, accumulated in fp64: G(0, 0) = d(0, 0); G(i, j) = d(i, j) + the minimum over the existing predecessors (i-1, j-1),
 *      (i-1, j), (i, j-1).  Ties: the diagonal predecessor is kept unless another is strictly smaller; then (i-1, j) is kept
 *      unless (i, j-1) is strictly smaller.  The path runs from (0, 0) to (Ta-1, Tb-1), is read back from the last cell and has
 *      at most Ta + Tb - 1 cells.
 *   4. Per pair: total = G(Ta-1, Tb-1) (double), path_len, and optionally the path, (path_len, 2) int32 pairs (i, j) in
 *      ascending order.  (The Python layer adds mean = total / path_len and, for n_ceps > 0, mcd_db = (10 sqrt(2) / ln 10) mean.)
 * Every cell of the warp is one fp64 min chain and one addition on exact inputs: a pair's results are the same bits on every
 * run, in any batch, and as a host restatement computes them from the same cost matrix.  Non-finite inputs give unspecified
 * values; the call still ends and writes nothing outside its outputs.
 * Workspace: 5 bytes per cell of the call (sum of Ta Tb: the fp32 cost matrix and one byte of back-pointer) and 4 n_ceps bytes
 * per frame, allocated at the first call and replaced by a larger one when a larger call arrives; never at the caps' size. */
typedef struct vx_dtw vx_dtw;
typedef struct vx_dtw_config {
  int32_t struct_size;  /* sizeof(vx_dtw_config) */
  int32_t dim;          /* D, 1 .. 128 */
  int32_t n_ceps;       /* 0 (rows as given) .. dim - 1 */
  int32_t max_frames;   /* capacity: frames per sequence, 1 .. 4096 */
  int32_t max_batch;    /* capacity: pairs per call, 1 .. 64 */
} vx_dtw_config;
/* Host only, no HIP call (the table goes to the device current at the first compare).  Nulls, a wrong struct_size or
 * max_batch < 1 -> VX_ERR_ARG; then dim outside [1, 128], n_ceps outside [0, dim - 1], max_frames outside [1, 4096] or
 * max_batch > 64 -> VX_ERR_UNSUPPORTED. */
int vx_dtw_create(const vx_dtw_config* cfg, vx_dtw** out);
void vx_dtw_destroy(vx_dtw* h);
/* n pairs in one ragged call: a[i] / b[i] DEVICE fp32 (Ta[i], dim) / (Tb[i], dim); the pointer arrays and the lengths live on
 * the host.  total (n doubles) and path_len (n int32): host or device memory.  path: nullable, and so is each entry; path[i]
 * DEVICE int32 with room for (Ta[i] + Tb[i] - 1, 2), of which the first path_len[i] pairs are written (the rest is scratch of
 * the call).  Every pair is bitwise what it is alone.  Checked before any HIP call, in this order: null arguments (path
 * excepted) or n < 1 -> VX_ERR_ARG; n > max_batch -> VX_ERR_CAPACITY; then per pair in order: a null a[i] / b[i] or a length
 * < 1 -> VX_ERR_ARG, a length > max_frames -> VX_ERR_CAPACITY (the message names the pair).  The work (cepstra, cost, warp: one
 * launch each for all pairs) is enqueued on `stream`; the host waits only for the previous call's staging copy (and, when the
 * workspace has to grow, for the previous call).  Calls on one handle must not overlap. */
int vx_dtw_compare(vx_dtw* h, int32_t n, const float* const* a, const int32_t* Ta, const float* const* b, const int32_t* Tb,
                   double* total, int32_t* path_len, int32_t* const* path, void* stream);
/* Test-only, like the vx_op_* entries above.  vx_op_dtw_cost: the cepstra (n_ceps > 0) and cost kernels on one pair; a (Ta, dim),
 * b (Tb, dim), cost (Ta, Tb) fp32, all DEVICE; frames 1 .. 4096.  vx_op_dtw_path: the warp kernel on n caller-supplied cost
 * matrices in one launch, one workgroup each.  desc: HOST, n x 4 values per matrix: Ta, Tb, cell_off (of the (Ta, Tb) matrix in
 * cost), path_off (of its path in path, in cells: int32 pairs; room for Ta + Tb - 1); cost, total (n doubles), path_len (n
 * int32) and path (nullable) DEVICE.  Bad arguments: VX_ERR_ARG (frames above 4096: VX_ERR_CAPACITY) before any HIP call.  Both
 * synchronise the stream. */
int vx_op_dtw_cost(int32_t dim, int32_t n_ceps, const float* a, int32_t Ta, const float* b, int32_t Tb, float* cost, void* stream);
int vx_op_dtw_path(const float* cost, int32_t n, const int64_t* desc, double* total, int32_t* path_len, int32_t* path, void* stream);

/* ---- fundamental frequency (YIN, de Cheveigne & Kawahara 2002) and the F0 figures along a warp path --------------------------
 * A handle of its own: no weights, no vx_engine.  The framing is the filterbank's, so row t of a track is row t of the log-mel.
 * Per utterance, a mono fp32 waveform x of L samples at 24 kHz, zeros appended past L:
 *   frames T = (L + 128) / 256 (none below 128 samples); tau_min = floor(24000 / fmax_hz), tau_max = ceil(24000 / fmin_hz), in
 *   fp64 on the fp32 fields; 12 <= tau_min < tau_max <= 512 is served.
 *   1. Half-window differences, for u = 0 .. T and tau = 0 .. tau_max:
 *        h_u(tau) = sum_{j = 0 .. 255} (x[256 u + j] - x[256 u + j + tau])^2
 *      on differences in fp32 (never energy minus correlation: at the period the two cancel, and that is where the decision is
 *      taken).  A product is fused into its sum; (u, tau) has 8 chains, chain q over j = q, q + 8, ... ascending, folded as
 *      ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).  d_t(tau) = h_t(tau) + h_{t+1}(tau), fp32: an integration window of 512 and a
 *      reach of 1024 samples, the filterbank frame's.
 *   2. Cumulative mean normalised difference: d'_t(0) = 1, d'_t(tau) = d_t(tau) tau / sum_{k = 1 .. tau} d_t(k), the running sum
 *      and the quotient in fp64, rounded once to fp32; 1 where the sum is 0 (a silent frame).
 *   3. Lag: the first tau in [tau_min, tau_max] with d'(tau) < threshold, then while tau < tau_max and d'(tau + 1) < d'(tau):
 *      tau += 1; such a frame is voiced.  Without a tau under the threshold the frame is unvoiced and tau* is the first global
 *      minimum of d' on the range.
 *   4. Refinement, in fp64 on the fp32 d': if tau* < tau_max, with a, b, c = d'(tau* - 1), d'(tau*), d'(tau* + 1) and den = a -
 *      2 b + c > 0 the offset is (a - c) / (2 den) clamped to +-0.5, else 0.  f0 = 24000 / (tau* + offset), rounded once, on
 *      voiced frames; 0 on unvoiced ones.
 *   5. Per frame: f0 (fp32, Hz), aperiodicity = d'(tau*) (fp32), lag = tau* (int32), voiced (uint8, 0 / 1).
 * A frame's bits depend on its own 1024 samples only: never on the batch, on the frame's place in the launch or on the run.
 * Non-finite samples give unspecified values; the call still ends and writes nothing outside its outputs.  There is no
 * workspace: the differences never leave the chip; a handle holds its staging block and max_batch rows of sums. */
typedef struct vx_pitch vx_pitch;
typedef struct vx_pitch_config {
  int32_t struct_size;  /* sizeof(vx_pitch_config) */
  int32_t sample_rate;  /* 24000 */
  float fmin_hz;        /* lowest f0 searched: tau_max = ceil(24000 / fmin_hz) <= 512 (46.875 Hz and up) */
  float fmax_hz;        /* highest: tau_min = floor(24000 / fmax_hz) >= 12 (up to 2000 Hz) */
  float threshold;      /* on d', positive and finite; YIN's 0.1 */
  int32_t max_frames;   /* capacity: frames per utterance, >= 1 */
  int32_t max_batch;    /* capacity: utterances (or pairs) per call, 1 .. 64 */
} vx_pitch_config;
/* Host only, no HIP call.  Nulls, a wrong struct_size, max_batch < 1, max_frames < 1 or a threshold that is not positive and
 * finite -> VX_ERR_ARG; then another sample rate, a band outside the served lags or max_batch > 64 -> VX_ERR_UNSUPPORTED. */
int vx_pitch_create(const vx_pitch_config* cfg, vx_pitch** out);
void vx_pitch_destroy(vx_pitch* h);
/* The handle's tau_min and tau_max.  Host only. */
int vx_pitch_lag_range(const vx_pitch* h, int32_t* tau_min, int32_t* tau_max);
/* n utterances in one ragged launch: wav[i] DEVICE fp32 of n_samples[i] samples; f0[i], aperiodicity[i] DEVICE fp32, lag[i]
 * DEVICE int32, voiced[i] DEVICE uint8, each of vx_fbank_frames(n_samples[i]) elements.  The pointer arrays and the lengths live
 * on the host; each of the four output arrays may be null, and so may each of its entries.  An utterance without frames (fewer
 * than 128 samples) writes nothing.  Checked before any HIP call, in this order: null h, wav or n_samples, or n < 1 ->
 * VX_ERR_ARG; n > max_batch -> VX_ERR_CAPACITY; then per utterance in order: a null wav[i] or n_samples[i] < 0 -> VX_ERR_ARG,
 * more frames than max_frames -> VX_ERR_CAPACITY (the message names the utterance).  The work is enqueued on `stream`; the host
 * waits only for the previous call's staging copy.  Calls on one handle must not overlap. */
int vx_pitch_track(vx_pitch* h, int32_t n, const float* const* wav, const int32_t* n_samples, float* const* f0,
                   float* const* aperiodicity, int32_t* const* lag, uint8_t* const* voiced, void* stream);
/* The F0 figures of n pairs of tracks along caller-supplied paths (those of vx_dtw_compare on the same framing): f0_a[i] (Ta[i])
 * and f0_b[i] (Tb[i]) DEVICE fp32 in Hz, 0 = unvoiced; path[i] DEVICE int32 (path_len[i], 2) cells (i, j), as vx_dtw_compare
 * leaves them.  The path is served on the device only: the host never reads it, so a cell outside [0, Ta) x [0, Tb) cannot be
 * refused and is clamped into the range instead.  sums: n rows of 11 doubles, host or device memory:
 *   [0] n_path  [1] n_voiced_both  [2] n_vuv_mismatch (voiced in exactly one of the two)
 *   and over the cells voiced in both, with c = 1200 log2(fa / fb), la = ln fa, lb = ln fb:
 *   [3] sum c  [4] sum c^2  [5] sum (fa - fb)^2  [6] sum la  [7] sum lb  [8] sum la^2  [9] sum lb^2  [10] sum la lb
 * all in fp64: thread t of 256 adds the cells t, t + 256, ... in ascending order, then a fixed binary tree; the same bits on
 * every run and in any batch.  (The Python layer derives rmse_cents = sqrt([4] / [1]), rmse_hz = sqrt([5] / [1]), Pearson's r of
 * la and lb, and vuv_error = [2] / [0].)  Checked before any HIP call: null arguments or n < 1 -> VX_ERR_ARG; n > max_batch ->
 * VX_ERR_CAPACITY; then per pair in order: a null pointer, Ta[i], Tb[i] or path_len[i] < 1 -> VX_ERR_ARG, Ta[i] or Tb[i] >
 * max_frames, or path_len[i] > Ta[i] + Tb[i] - 1 (the longest a warp path gets) -> VX_ERR_CAPACITY (the message names the
 * pair).  Enqueued on `stream`, as vx_pitch_track. */
int vx_pitch_compare(vx_pitch* h, int32_t n, const float* const* f0_a, const int32_t* Ta, const float* const* f0_b, const int32_t* Tb,
                     const int32_t* const* path, const int32_t* path_len, double* sums, void* stream);
/* Test-only, like the vx_op_* entries above: d' of one utterance, dprime DEVICE fp32 (frames, tau_max + 1) for the band's
 * tau_max; wav DEVICE.  Null pointers, n_samples < 0 or a band vx_pitch_create refuses -> VX_ERR_ARG before any HIP call.
 * Synchronises the stream. */
int vx_op_pitch_diff(float fmin_hz, float fmax_hz, const float* wav, int32_t n_samples, float* dprime, void* stream);

/* ---- multi-resolution STFT distance between two waveforms (Parallel WaveGAN, Yamamoto et al. 2020; BigVGAN's M-STFT column) ----
 * A handle of its own: no weights, no vx_engine.  Two mono fp32 waveforms at 24 kHz, pred (X) and target (Y), both cut to the
 * common length L = min(n_pred, n_target).  For every resolution r = (n_fft, hop, win) of the handle:
 *   frames     as torch.stft(center=True, pad_mode="reflect") makes them: T = 1 + L / hop frames, frame t centred on sample t hop;
 *              sample p < 0 is sample -p and sample p >= L is sample 2 (L - 1) - p (the edge sample is not repeated), which needs
 *              L > n_fft / 2.
 *   window     periodic Hann of `win` samples, w[j] = 0.5 - 0.5 cos(2 pi j / win), at offset (n_fft - win) / 2 (integer division)
 *              inside the n_fft frame, zero elsewhere; built in fp64 and rounded once, the product x w is fp32.
 *   magnitude  bins k = 0 .. n_fft / 2: |S|[t][k] = sqrt(max(re^2 + im^2, eps)), an fp32 number (eps = 1e-8: a floor of 1e-4).  The
 *              DFT is direct, on the fp32 matrix instruction: sample pair s = (2 s, 2 s + 1) goes to fmaf chain s mod 4, and
 *              after 8 pairs of every chain (64 samples) the four chains are added, chain 0 first, to an fp64 total and start
 *              again from zero; re^2 + im^2, the clamp and the root are fp64 on the totals, rounded once.
 *   sums       in fp64 on the fp32 magnitudes, over the T (n_fft / 2 + 1) cells:
 *                [0] sum (|Y| - |X|)^2   [1] sum |Y|^2   [2] sum |ln |Y| - ln |X||   [3] cells
 *              every thread adds its cells in a fixed order, a fixed tree adds the threads of a workgroup (16 frames x 256
 *              bins), and the workgroups of a (pair, resolution) are added in ascending order.  No atomics: the same bits on every run and in any batch.
 * (The Python layer derives sc_r = sqrt([0] / [1]), lm_r = [2] / [3] and total = mean over r of sc_r + lm_r.  sc is not symmetric
 * in (pred, target); lm is.  The clamp keeps [1] >= cells eps, so sc never divides by zero.)
 * Served: n_fft in {512, 1024, 2048}, 1 <= win <= n_fft, 1 <= hop <= n_fft, 1 .. 4 resolutions, L > max n_fft / 2 (1025 samples
 * for the default triple (1024, 120, 600), (2048, 240, 1200), (512, 50, 240)).  A shorter pair is an argument error: never a
 * silently dropped resolution.  Non-finite samples give unspecified values; the call still ends and writes nothing outside its
 * outputs.  The spectrograms never go to memory; a handle holds its tables, its staging block and three doubles per workgroup. */
typedef struct vx_stft vx_stft;
typedef struct vx_stft_config {
  int32_t struct_size;  /* sizeof(vx_stft_config) */
  int32_t sample_rate;  /* 24000 */
  int32_t n_res;        /* 1 .. 4 resolutions */
  int32_t n_fft[4];     /* each 512, 1024 or 2048 */
  int32_t hop[4];       /* 1 .. n_fft */
  int32_t win[4];       /* 1 .. n_fft */
  float eps;            /* clamp on the power, positive and finite; 1e-8 */
  int32_t max_samples;  /* capacity: samples per signal, > max n_fft / 2 */
  int32_t max_batch;    /* capacity: pairs (or signals) per call, 1 .. 64 */
} vx_stft_config;
/* Host only, no HIP call.  Nulls, a wrong struct_size, max_batch < 1, max_samples < 1 or an eps that is not positive and finite
 * -> VX_ERR_ARG; then another sample rate, n_res outside 1 .. 4, a resolution outside the served range, max_batch > 64,
 * max_samples <= max n_fft / 2 or a workspace above 2^24 tiles -> VX_ERR_UNSUPPORTED. */
int vx_stft_create(const vx_stft_config* cfg, vx_stft** out);
void vx_stft_destroy(vx_stft* h);
/* 1 + n_samples / hop of resolution `res`; 0 for a null handle, a resolution the handle does not have or n_samples < 0.  Host only. */
int vx_stft_frames(const vx_stft* h, int32_t res, int32_t n_samples);
/* n pairs in one ragged call: pred[i] (n_pred[i] samples) and target[i] (n_target[i]) DEVICE fp32; the pointer arrays and the
 * lengths live on the host.  sums: n x n_res x 4 doubles as above, host or device memory.  Samples past the common length are
 * not read.  Checked before any HIP call, in this order: null arguments or n < 1 -> VX_ERR_ARG; n > max_batch ->
 * VX_ERR_CAPACITY; then per pair in order: a null pointer or a common length <= max n_fft / 2 -> VX_ERR_ARG, a common length >
 * max_samples -> VX_ERR_CAPACITY (the message names the pair).  One launch per resolution and one for the sums, enqueued on
 * `stream`; the host waits only for the previous call's staging copy.  Calls on one handle must not overlap. */
int vx_stft_compare(vx_stft* h, int32_t n, const float* const* pred, const int32_t* n_pred, const float* const* target,
                    const int32_t* n_target, double* sums, void* stream);
/* The magnitudes of resolution `res` themselves, by the same kernel body with the store in place of the reduction: wav[i] DEVICE
 * fp32 of n_samples[i] samples, out[i] DEVICE fp32 (vx_stft_frames(h, res, n_samples[i]), n_fft / 2 + 1).  Checks as above, with
 * `res` outside the handle -> VX_ERR_ARG and n_samples[i] > n_fft / 2 of THIS resolution required.  One launch on `stream`. */
int vx_stft_magnitude(vx_stft* h, int32_t res, int32_t n, const float* const* wav, const int32_t* n_samples, float* const* out,
                      void* stream);

/* ---- the mel-spectrogram Transformer TTS model (valle/models/transformer.py, --model-name Transformer) ------------------------
 * The reference's third model: a text encoder, a decoder over log-mel frames with cross-attention to the encoded text, a 100-wide
 * regression head and a stop head.  There is no vocabulary and no sampler: the predicted frame itself is fed back through
 * decoder_prenet.  A handle of its own (own weights, KV cache and captured step); batch 1, as the reference's loop.  Its decoder
 * layer is the VALL-F one, its encoder the row stack without a mask, both through the code the token models run.
 *   encode  (transformer.py:344-347): text_embedding -> encoder_prenet (identity, or 3 x [Conv1d k=5 same, BatchNorm1d eval, ReLU]
 *           + Linear) -> x + alpha pe (scale=False) -> L encoder layers (ReLU, FFN 4 d) -> LayerNorm when norm_first; the result is
 *           projected once into every decoder layer's cross-attention K / V.
 *   decode  (transformer.py:353-385) with a KV cache, one step per frame where the reference recomputes every row on every pass
 *           (its TODO at :352).  Input row 0 is decoder_prenet(0) + alpha pe[0]; pass p runs row p through the L decoder layers,
 *           the final LayerNorm (norm_first) and predict_layer / stop_layer.  Stop rule, tested BEFORE the append (:377-383): rows
 *           > 10 S (rows = p + 1) or stop logit > 0; the stopping pass's frame is dropped, so S ids give at most 10 S frames and a
 *           stop on pass 0 gives none.  Otherwise the frame is appended and fed back at position p + 1.
 * precision VX_PREC_F32 or VX_PREC_BF16 (bf16 attention / FFN matrices, GEMM operands and KV cache; the head, the prenets and the
 * residual stream stay fp32).  scaling_xformers (ScaledLinear / BasicNorm / DoubleSwish, transformer.py:114-172) is not built. */
typedef struct vx_mel vx_mel;
enum vx_mel_stop {
  VX_MEL_STOP_NONE = 0,
  VX_MEL_STOP_LOGIT = 1,      /* stop_layer's logit > 0 (transformer.py:376) */
  VX_MEL_STOP_LENGTH = 2,     /* rows > 10 S (transformer.py:377) */
  VX_MEL_STOP_MAX_FRAMES = 3  /* engine-level max_frames (not in the reference); also how a teacher-forced decode ends */
};
enum vx_mel_flags { VX_MEL_NO_GRAPH = 1 /* launch the step kernel by kernel instead of as a hipGraph */ };
/* Mirrors Transformer.__init__ (transformer.py:47-55). */
typedef struct vx_mel_config {
  int32_t struct_size;      /* = sizeof(vx_mel_config) */
  int32_t d_model;          /* multiple of 8, <= 1024 */
  int32_t nhead;            /* d_model / nhead in {4, 8, 16, 32, 64} */
  int32_t num_layers;       /* encoder layers = decoder layers */
  int32_t norm_first;
  int32_t add_prenet;
  int32_t scaling_xformers; /* != 0: VX_ERR_UNSUPPORTED */
  int32_t precision;        /* VX_PREC_F32 or VX_PREC_BF16 */
  int32_t max_text;         /* capacity: phoneme ids per utterance */
  int32_t max_frames;       /* capacity: frames per utterance */
  int32_t device;
  int32_t flags;            /* enum vx_mel_flags */
} vx_mel_config;
/* Transformer(...) + .to(device) (transformer.py:47-207).  Checked before any HIP call: nulls, struct_size, non-positive sizes or
 * capacities, an unknown precision -> VX_ERR_ARG; scaling_xformers, a width or head_dim outside the ranges above ->
 * VX_ERR_UNSUPPORTED. */
int vx_mel_create(const vx_mel_config* cfg, vx_mel** out);
void vx_mel_destroy(vx_mel* m);
/* model.load_state_dict, one tensor at a time, under the reference's state_dict keys (transformer.py:66-203):
 * text_embedding.word_embeddings.weight, encoder_position.alpha, decoder_position.alpha, encoder.layers.N.* / decoder.layers.N.*
 * (torch.nn.TransformerEncoderLayer / TransformerDecoderLayer), encoder.norm.* / decoder.norm.* (norm_first), predict_layer.*,
 * stop_layer.*, decoder_prenet.weight / .bias or, with add_prenet, decoder_prenet.{0,3,6}.* and encoder_prenet.{1,5,9}.* (Conv1d),
 * .{2,6,10}.{weight,bias,running_mean,running_var} (BatchNorm1d; num_batches_tracked is not passed), .14.* (Linear).  data: fp32,
 * host or device.  Unknown key or wrong shape: VX_ERR_WEIGHTS. */
int vx_mel_set_weight(vx_mel* m, const char* key, const float* data, const int64_t* shape, int32_t ndim);
/* Optional: the fp32 table of SinePositionalEmbedding (modules/embedding.py:75-88), (rows, d_model) with rows >= max(4000, max_text +
 * max_frames + 2); both positions share it.  If never set the handle fills it with host sinf / cosf. */
int vx_mel_set_sine_table(vx_mel* m, const float* data, int64_t rows, int64_t dim);
/* strict=True + model.eval(): a missing tensor is VX_ERR_WEIGHTS naming it. */
int vx_mel_finalize(vx_mel* m);
/* transformer.py:342-347: the encoder over text (S,) int64, host or device, and every decoder layer's memory K / V.  Checked before
 * any HIP call: nulls -> VX_ERR_ARG; S <= 0 -> VX_ERR_ARG (:340); weights not finalised -> VX_ERR_STATE; S > max_text ->
 * VX_ERR_CAPACITY. */
int vx_mel_encode(vx_mel* m, const int64_t* text, int32_t S, void* stream);
/* transformer.py:353-385 over the text of the last vx_mel_encode.  max_frames < 0: the reference's rule only; otherwise the decode
 * also ends, with VX_MEL_STOP_MAX_FRAMES, once max_frames frames are appended and the next pass does not stop by the reference's
 * rule: its frames are bitwise the first max_frames of the unlimited run.  max_frames above the handle's capacity: VX_ERR_CAPACITY
 * before any work; with max_frames < 0 a text whose worst case 10 S exceeds the capacity is not refused, but a decode that fills the
 * capacity before the reference's rule fired returns VX_ERR_CAPACITY.  No encode since create / finalize: VX_ERR_STATE. */
int vx_mel_decode(vx_mel* m, int32_t max_frames, void* stream);
/* Parity tests: the decode with the fed-back frames taken from `forced` (T, 100) fp32, host or device, instead of the predictions
 * (which are still what vx_mel_result returns, with their stop logits): T passes, ends with VX_MEL_STOP_MAX_FRAMES, the reference's
 * stop rule is not applied.  Pass p sees exactly the rows [0; forced[:p]] of the reference's forward (transformer.py:279-300). */
int vx_mel_decode_forced(vx_mel* m, const float* forced, int32_t T, void* stream);
/* The last decode: frames (n_frames, 100) fp32 into `frames` (host or device, room for `capacity` frames; rows past n_frames are
 * not touched; NULL: counts only), the stop logit of every pass into stop_logits (host or device, nullable, room for capacity + 1
 * values), n_pass of them: n_frames + 1, or n_frames after vx_mel_decode_forced.  capacity < n_frames: VX_ERR_CAPACITY. */
int vx_mel_result(vx_mel* m, float* frames, int32_t capacity, int32_t* n_frames, int32_t* stop_reason, float* stop_logits,
                  int32_t* n_pass);
/* The quantities inside the reference's forward (transformer.py:279-300) for one utterance: text (S,), frames (T, 100) fp32; one
 * causal row pass over [0; frames[:-1]] gives predict (T, 100) and stop_logits (T,) (host or device).  Encodes the text first (the
 * handle is then as after vx_mel_encode(text, S)).  Checks as vx_mel_encode, and T < 1 -> VX_ERR_ARG, T > max_frames ->
 * VX_ERR_CAPACITY. */
int vx_mel_teacher_forced(vx_mel* m, const int64_t* text, int32_t S, const float* frames, int32_t T, float* predict,
                          float* stop_logits, void* stream);
/* out[0] ms of the last decode (device time of the replayed steps), out[1] its step launches, out[2] kernel launches per step (nodes
 * of the captured graph; 0 with VX_MEL_NO_GRAPH), out[3] ms of the last encode. */
int vx_mel_get_timings(vx_mel* m, double* out, int32_t n);
/* Parity tests: the decoder side's taps of vx_read_buffer on the handle's inner engine - "ar_kv" (the self-attention cache,
 * [layer][K|V][head][max_text + max_frames + 2][head_dim]; frame row r is cache row r), "ar_mem" (every decoder layer's cross K / V
 * of the last encode, [layer][K|V][head][max_text][head_dim]; rows at and past that text's length keep what a longer text left),
 * "ar_x" (the step's input row, d fp32) - and "xh" (d fp32: the residual row the last decoder layer left for the head). */
int vx_mel_read(vx_mel* m, const char* name, void* dst, int64_t offset_bytes, int64_t nbytes);
/* Kernel-level: `launches` launches of the decode step's opening kernel (csrc/meltf.hip, through the launcher the step uses) on
 * caller device buffers, back to back on one device-resident state, then a synchronisation.  xh / gamma / beta (d), Wh (101, d),
 * bh (101), W0 (d, K0) / b0 (d) with K0 = 256 when W1 (256, 100) / b1 / W2 (256, 256) / b2 are given and 100 when they are all
 * NULL, alpha (1), pe (pe_rows, d), forced (n_forced, 100) when n_forced > 0; outputs x (d), frames (frames_cap, 100), stops
 * (stops_cap).  state: {row, pass, n_gen, S, done, stop_reason} on the host, read before and written after the launches; *arrive
 * (nullable): the arrival counter after the last launch.  Checked before any HIP call: nulls, d % 8 or d > 1024 (as
 * vx_mel_create), a prenet given in part, row < -1, and whether `launches` launches could leave pe, frames or stops. */
int vx_op_mel_open(int32_t d, const float* xh, const float* gamma, const float* beta, const float* Wh, const float* bh,
                   const float* W1, const float* b1, const float* W2, const float* b2, const float* W0, const float* b0,
                   const float* alpha, const float* pe, int32_t pe_rows, float* x, float* frames, int32_t frames_cap, float* stops,
                   int32_t stops_cap, int32_t* state, int32_t max_frames, int32_t n_forced, const float* forced, int32_t launches,
                   uint32_t* arrive, void* stream);

/* ---- Griffin-Lim vocoder: log-mel frames to a 24 kHz waveform ------------------------------------------------------------------
 * The inverse of the filterbank above, with its framing: 24 kHz, n_fft 1024, hop 256, the periodic Hann window w.  A handle of
 * its own: no weights.  Per utterance, logmel (T, n_mels) fp32 as vx_fbank_extract writes it; B is the (n_mels x 513) mel basis
 * (by default the built-in Slaney table of vx_fbank_create, from the same routine).
 *   1. mel = exp(logmel).
 *   2. mag = max(0, mel P^T), (T, 513), with P = B^T (B B^T)^-1 (513 x n_mels): the minimum-norm least-squares inverse and a clamp
 *      at zero (the rule of torchaudio's InverseMelScale).  P is computed on the host in fp64 by Cholesky of B B^T and rounded
 *      once; every cell of mag is summed in ascending filter order.
 *   3. y = I(X) for X (T, 513) complex: frame f is the inverse real DFT of row f (bins 0..512, Hermitian extension, the
 *      imaginary parts of bins 0 and 512 ignored, scale 1 / 1024) times w; frames are overlap-added at offsets 256 f in ascending
 *      frame order; y[n] = ola[n] / max(env[n], env_floor) for n in [0, 256 T) with env[n] = sum_f w^2[n - 256 f].  The 768
 *      samples past 256 T are dropped, so the length is 256 T and vx_fbank_frames of it is T.  env_floor (default 0.1) is part of
 *      the definition: w[0] = 0 and frame 0 alone covers the first 256 samples, so the floor makes the first ~8 ms a fade-in;
 *      the interior has env = 1.5.
 *   4. S(y) is the filterbank's analysis: y followed by 768 zeros, frame f = samples [256 f, 256 f + 1024) times w, one-sided DFT.
 *   5. Griffin-Lim with momentum (torchaudio.functional.griffinlim): ang = init (unit complex; 1 + 0i without one), tprev = 0;
 *      n_iter times { reb = S(I(mag ang)); a = reb - tprev momentum / (1 + momentum); ang = a / (|a| + 1e-16); tprev = reb };
 *      y = I(mag ang).
 * fp32 throughout; both transforms are the filterbank's 32 x 32 four-step factorisation on the fp32 matrix instruction with
 * tables computed in fp64 and rounded once.  There is no random number generator: a random start is the caller's init_phase. */
typedef struct vx_vocoder vx_vocoder;
typedef struct vx_vocoder_config {
  int32_t struct_size;       /* sizeof(vx_vocoder_config) */
  int32_t sample_rate;       /* 24000 */
  int32_t n_fft;             /* 1024 (also the window length) */
  int32_t hop;               /* 256 */
  int32_t n_mels;            /* 1 .. 128 */
  float fmin, fmax;          /* band of the built-in Slaney basis, 0 <= fmin < fmax <= 12000 */
  float env_floor;           /* floor under the window envelope, > 0 (0.1) */
  int32_t max_batch;         /* utterances per call */
  int32_t max_total_frames;  /* frames per call, summed over its utterances; <= 2^21 */
} vx_vocoder_config;
/* Host only, no HIP call (the tables go to the device current at the first synthesis).  Nulls, a wrong struct_size, max_batch < 1,
 * max_total_frames < 1 or an env_floor that is not positive and finite -> VX_ERR_ARG; another geometry, n_mels, band, a
 * max_total_frames above 2^21, or a built-in basis whose B B^T has no Cholesky factor -> VX_ERR_UNSUPPORTED. */
int vx_vocoder_create(const vx_vocoder_config* cfg, vx_vocoder** out);
void vx_vocoder_destroy(vx_vocoder* v);
/* Host only.  set_mel_basis: a HOST (n_mels x 513) basis; its inverse P replaces the current one at the next synthesis.  A basis
 * whose B B^T has no Cholesky factor (a pivot below 1e-12 of its diagonal entry: empty or linearly dependent filters) ->
 * VX_ERR_UNSUPPORTED, and the handle keeps what it had.  set_inverse: the caller's own HOST (513 x n_mels) table instead, taken as
 * it is.  get_inverse copies the current (513 x n_mels) table out. */
int vx_vocoder_set_mel_basis(vx_vocoder* v, const float* basis);
int vx_vocoder_set_inverse(vx_vocoder* v, const float* inverse);
int vx_vocoder_get_inverse(const vx_vocoder* v, float* inverse);
/* 256 n_frames, the samples a synthesis of n_frames = T frames writes; 0 for a negative T.  Host only. */
int64_t vx_vocoder_samples(int64_t n_frames);
/* n utterances: logmel[i] DEVICE fp32 (n_frames[i], n_mels), wav_out[i] DEVICE fp32 of 256 n_frames[i] samples; init_phase:
 * NULL (the zero-phase start) or per utterance DEVICE fp32 (n_frames[i], 513) radians; phase_out: NULL or per utterance DEVICE
 * fp32 (n_frames[i], 513, 2), the final ang (re, im).  The pointer arrays and n_frames live on the host.  An utterance with
 * n_frames[i] = 0 writes nothing and its pointers are not looked at.  Every utterance is bitwise what it is alone, and two
 * identical calls give the same bits.  Checked before any HIP call, in this order: null arguments (init_phase and phase_out
 * excepted), n < 1, n_iter < 0, a momentum outside [0, 1) or not finite -> VX_ERR_ARG; n > max_batch -> VX_ERR_CAPACITY; then
 * per utterance in order n_frames[i] < 0 or, with frames, a null entry -> VX_ERR_ARG, and a running sum of frames above
 * max_total_frames -> VX_ERR_CAPACITY.  A call without any frame returns here.  The work (one launch for mag and the start, two
 * per iteration, two for the final y) is enqueued on `stream`; the host waits only for the previous call's staging copy (and,
 * after a new inverse or when the workspace, 14356 bytes per frame of the largest call so far, has to grow, for the previous
 * call).  Calls on one handle must not overlap. */
int vx_vocoder_synthesize(vx_vocoder* v, int32_t n, const float* const* logmel, const int32_t* n_frames,
                          const float* const* init_phase, int32_t n_iter, float momentum, float* const* wav_out,
                          float* const* phase_out, void* stream);
/* The warm start: the same call with the start given as phase_out gives it, init_ang[i] DEVICE fp32 (n_frames[i], 513, 2), taken
 * as it is (not normalised); init_ang itself must not be NULL.  With n_iter = 0 the phase_out of a synthesis reproduces its
 * waveform bit for bit. */
int vx_vocoder_synthesize_warm(vx_vocoder* v, int32_t n, const float* const* logmel, const int32_t* n_frames,
                               const float* const* init_ang, int32_t n_iter, float momentum, float* const* wav_out,
                               float* const* phase_out, void* stream);

/* ---- Neural vocoder: a HiFi-GAN / BigVGAN generator, log-mel frames to a waveform ----------------------------------------------
 * One generator family with two activation modes, a handle of its own, fp32 storage and accumulation.  Per utterance, logmel
 * (T, n_mels) fp32; below x is (C, L).  S = n_stages, u_i = rates[i], k_i = kernels[i], C_0 = initial_channels, C_{i+1} = C_i / 2,
 * R = n_resblocks with kernel sizes rk_r, D = n_dilations with dilations d_{r,m}; every convolution pads with zeros.
 *   1. x = conv_pre(logmel^T): Conv1d(n_mels -> C_0, k = 7, padding 3).  With `mean` / `scale` set (SpeechT5HifiGan's
 *      normalize_before) the input is (logmel - mean) / scale first.
 *   2. for i in 0 .. S-1:  VX_GAN_LRELU only: x = lrelu(x, lrelu_slope).  Then the transposed convolution with p = (k_i - u_i) / 2:
 *      out[co][n] = b[co] + sum over ci, t, j with n = t u_i - p + j, 0 <= j < k_i of x[ci][t] W[ci][co][j], n in [0, L u_i).
 *      Then x = (1 / R) sum_r resblock_{i,r}(x), summed in ascending r and divided by R.
 *   3. resblock_{i,r}(x): for m in 0 .. D-1 { xt = act(x); xt = conv(xt; k = rk_r, dilation d_{r,m}, padding d_{r,m} (rk_r - 1) / 2);
 *      xt = act(xt); xt = conv(xt; k = rk_r, dilation 1); x = x + xt }.  VX_GAN_LRELU: act = lrelu(., lrelu_slope).  Otherwise every
 *      act is the anti-aliased activation below with parameters of its own: activations.{2m} before the dilated convolution,
 *      activations.{2m+1} before the second.
 *   4. VX_GAN_LRELU: x = lrelu(x, 0.01) (torch's default slope, as SpeechT5HifiGan.forward and the original).  Otherwise the
 *      anti-aliased activation `activation_post`.
 *   5. y = tanh(conv_post(x)): Conv1d(C_S -> 1, k = 7, padding 3), the bias optional.  T * prod(u_i) samples.
 * The anti-aliased activation (ratio 2, 12 taps), per channel on a signal x of length L:
 *   filter f = kaiser_sinc(cutoff 0.25, half_width 0.3, K = 12): delta_f = 4 half_width, A = 2.285 (K/2 - 1) pi delta_f + 7.95,
 *      beta = 0.1102 (A - 8.7) if A > 50, 0.5842 (A - 21)^0.4 + 0.07886 (A - 21) if A >= 21, else 0; w = the symmetric Kaiser
 *      window of K points; time = -K/2 + 0.5 .. K/2 - 0.5; f = 2 cutoff w sinc(2 cutoff time), f /= sum f.  Computed in fp64 and
 *      rounded once; vx_gan_set_filter replaces it.  The same taps serve up and down.
 *   up:   xp = x replicate-padded by 5 on each side; full[m] = sum over i, j with m = 2 i + j of xp[i] f[j]; u = 2 full[15 : 15 + 2L].
 *         Equivalently u[2m] = 2 sum_{s<6} f[2s+1] x[cl(m + 2 - s)], u[2m+1] = 2 sum_{s<6} f[2s] x[cl(m + 3 - s)], cl = clamp to [0, L).
 *   act:  v = u + sin(a u)^2 / (b + 1e-9); snake: b = a = alpha, snakebeta: a = alpha, b = beta; with alpha_logscale a = exp(alpha),
 *         b = exp(beta).  a and 1 / (b + 1e-9) are formed on the host in fp64 and rounded once.
 *   down: y[t] = sum_{j<12} f[j] v[clamp(2t + j - 5, 0, 2L - 1)]: the replicate pad (5 left, 6 right) acts on the cropped 2L-long v.
 * Weight keys (fp32, host, torch layouts, weight norm already folded): conv_pre.weight (C_0, n_mels, 7), conv_pre.bias;
 * ups.{i}.weight (C_i, C_{i+1}, k_i), ups.{i}.bias; resblocks.{i R + r}.convs1.{m}.weight (C, C, rk_r) / .bias and convs2 alike;
 * resblocks.{n}.activations.{a}.alpha (C) and, for snakebeta, .beta; activation_post.alpha / .beta (C_S); conv_post.weight
 * (1, C_S, 7); optional: conv_post.bias (1), and mean with scale (n_mels). */
typedef struct vx_gan vx_gan;
enum { VX_GAN_LRELU = 0, VX_GAN_SNAKE = 1, VX_GAN_SNAKEBETA = 2 };
typedef struct vx_gan_config {
  int32_t struct_size;          /* sizeof(vx_gan_config) */
  int32_t n_mels;
  int32_t n_stages;             /* 1 .. 8 */
  int32_t rates[8];
  int32_t kernels[8];
  int32_t initial_channels;     /* C_0, a multiple of 2^n_stages */
  int32_t n_resblocks;          /* 1 .. 4 */
  int32_t resblock_kernels[4];  /* odd */
  int32_t n_dilations;          /* 1 .. 4 */
  int32_t dilations[4][4];      /* [resblock][m] */
  int32_t activation;           /* VX_GAN_* */
  int32_t alpha_logscale;       /* 0 / 1 */
  float lrelu_slope;
  int32_t max_batch;            /* utterances per call, <= 64 */
  int32_t max_total_frames;     /* frames per call, summed over its utterances; <= 2^21 */
} vx_gan_config;
/* Host only, no HIP call.  In this order: nulls, a wrong struct_size, max_batch < 1, max_total_frames < 1, n_mels < 1, n_stages /
 * n_resblocks / n_dilations outside their ranges, a rate, kernel, resblock kernel or dilation < 1, initial_channels < 1, an
 * activation outside VX_GAN_*, alpha_logscale outside 0 / 1, a lrelu_slope that is not finite -> VX_ERR_ARG; then k_i < u_i or
 * k_i - u_i odd, an even resblock kernel, initial_channels no multiple of 2^n_stages, prod(u_i) > 4096, max_batch > 64,
 * max_total_frames > 2^21 -> VX_ERR_UNSUPPORTED. */
int vx_gan_create(const vx_gan_config* cfg, vx_gan** out);
void vx_gan_destroy(vx_gan* g);
/* Host only.  data: HOST fp32 of `shape`.  Unknown key or wrong shape -> VX_ERR_WEIGHTS; after vx_gan_finalize -> VX_ERR_STATE. */
int vx_gan_set_weight(vx_gan* g, const char* key, const float* data, const int64_t* shape, int32_t ndim);
/* Host only: the 12 taps (HOST fp32) replace the built-in filter of every anti-aliased activation.  Another count -> VX_ERR_UNSUPPORTED;
 * after vx_gan_finalize -> VX_ERR_STATE. */
int vx_gan_set_filter(vx_gan* g, const float* taps, int32_t n_taps);
/* Host only: the 12 taps in use. */
int vx_gan_get_filter(const vx_gan* g, float* taps);
/* Host only: checks that every tensor is there (a missing one -> VX_ERR_WEIGHTS naming it; mean without scale too) and packs the
 * weights for the kernels.  They go to the device that is current at the first synthesis. */
int vx_gan_finalize(vx_gan* g);
/* n_frames * prod(u_i); 0 for a negative n_frames or a null handle.  Host only. */
int64_t vx_gan_samples(const vx_gan* g, int64_t n_frames);
/* n utterances: logmel[i] DEVICE fp32 (n_frames[i], n_mels), wav_out[i] DEVICE fp32 of n_frames[i] prod(u_i) samples.  The pointer
 * arrays and n_frames live on the host.  An utterance with n_frames[i] = 0 writes nothing and its pointers are not looked at.
 * Every utterance is bitwise what it is alone, and two identical calls give the same bits.  Checked before any HIP call, in this
 * order: null arguments, n < 1 -> VX_ERR_ARG; not finalized -> VX_ERR_STATE; n > max_batch -> VX_ERR_CAPACITY; then per utterance
 * in order n_frames[i] < 0 or, with frames, a null entry -> VX_ERR_ARG, and a running sum of frames above max_total_frames ->
 * VX_ERR_CAPACITY.  A call without any frame returns here.  The utterances are served in groups of whole utterances so that the
 * five row buffers (the widest stage's rows each) are reused; the work is enqueued on `stream`, and the host waits only for the
 * previous call's staging copy (and for the previous call when the workspace has to grow).  Calls on one handle must not overlap. */
int vx_gan_synthesize(vx_gan* g, int32_t n, const float* const* logmel, const int32_t* n_frames, float* const* wav_out,
                      void* stream);

/* ---- Speaker encoder: the WavLM / Wav2Vec2 x-vector network, a 16 kHz waveform to a speaker embedding ---------------------------
 * One family with two attention modes, a handle of its own, fp32 storage and accumulation (fp64 wherever a whole utterance is
 * reduced).  VX_SPK_WAVLM is the network of transformers' WavLMForXVector (gated, bucketed relative position bias), VX_SPK_PLAIN the
 * same network without the bias (Wav2Vec2ForXVector).  Per utterance, x = mono fp32 of L samples; d = hidden, H = heads,
 * hd = d / H, C_i = conv_dim[i], k_i / s_i = conv_kernel / conv_stride; no convolution of the feature encoder pads:
 * L' = (L - k) / s + 1 (integer division).  GELU is the exact one, 0.5 v (1 + erf(v / sqrt 2)).
 *   0. VX_SPK_NORMALIZE (a flag of the call): x = (x - mean) / sqrt(var + 1e-7), the biased variance of the utterance, the sums
 *      in fp64 in a fixed order.
 *   1. feature encoder: layer 0 = Conv1d(1 -> C_0, k_0, s_0), then GroupNorm with one group per channel (mean and biased
 *      variance over the utterance's own frames, fp64 sums, eps 1e-5, affine), then GELU; layers 1 .. n_conv - 1 = Conv1d(C_{i-1}
 *      -> C_i, k_i, s_i), GELU.  The result, (T, C) time-major, is the tap "features".
 *   2. projection: LayerNorm(C) (eps = layer_norm_eps, as every LayerNorm below), Linear C -> d.
 *   3. positional convolution: Conv1d(d -> d, k = pos_kernel, padding k / 2, groups = pos_groups), the last output frame dropped
 *      when k is even, GELU; h = LayerNorm(h + that).  This is hidden state 0 (tap "hidden0").
 *   4. layers l = 0 .. L-1, post-norm:  h = LN(h + Attn(h)); h = LN(h + W2 gelu(W1 h + b1) + b2) (tap "hidden<l+1>").
 *      Attn: q, k, v = Linear(h) split in H heads; scores[i][j] = (q_i . k_j) / sqrt(hd) + gate[h][i] bias[h][j - i]; softmax over
 *      j; out_proj of the weighted v.  VX_SPK_WAVLM: bias[h][r] = rel_attn_embed[bucket(r)][h] with layer 0's embedding in every
 *      layer, bucket(r) as given to vx_spk_set_buckets; the gate comes from the layer INPUT's head slice x_h (hd values), per layer:
 *      p = W_g x_h + b_g (8 values), a = sigmoid(p0 + p1 + p2 + p3), b = sigmoid(p4 + .. + p7), gate = a (b const_h - 1) + 2
 *      (tap "gate<l>", (T, H)).  VX_SPK_PLAIN: no bias term.
 *   5. head: with use_weighted_layer_sum, h = sum_l softmax(layer_weights)[l] hidden_l over the L + 1 hidden states in ascending l
 *      (tap "layer_sum"; without it the tap is the last hidden state); projector Linear d -> tdnn_dim[0]; TDNN layer i: frames
 *      t .. of the dilated window, y[t] = relu(W [x[t]; x[t + dil]; ..; x[t + (k-1) dil]] + b) with W (tdnn_dim[i], k * in) in (tap,
 *      channel) order, no padding (tap "tdnn" after the last); statistics pooling: mean and UNBIASED standard deviation over the
 *      remaining T' frames in fp64, concatenated (tap "pooled"); embedding = feature_extractor (2 tdnn_dim[-1] -> xvector);
 *      logits = classifier (xvector -> xvector) of the embedding.
 * Similarity of two embeddings: a . b / max(|a| |b|, 1e-8), fp64 sums.
 * Weight keys (fp32, host, torch layouts, transformers' names without the wavlm. / wav2vec2. prefix, weight norm folded):
 * feature_extractor.conv_layers.{i}.conv.weight (C_i, C_{i-1}, k_i) [+ .conv.bias with conv_bias],
 * feature_extractor.conv_layers.0.layer_norm.weight / .bias, feature_projection.layer_norm.*, feature_projection.projection.*,
 * encoder.pos_conv_embed.conv.weight (d, d / groups, k) / .bias, encoder.layer_norm.*, encoder.layers.{l}.attention.{q,k,v,out}_proj.*,
 * encoder.layers.{l}.layer_norm.*, .feed_forward.intermediate_dense.*, .feed_forward.output_dense.*, .final_layer_norm.*; VX_SPK_WAVLM:
 * encoder.layers.{l}.attention.gru_rel_pos_linear.weight (8, hd) / .bias, .gru_rel_pos_const (1, H, 1, 1) and
 * encoder.layers.0.attention.rel_attn_embed.weight (num_buckets, H); layer_weights (L + 1) with use_weighted_layer_sum;
 * projector.*, tdnn.{i}.kernel.weight (tdnn_dim[i], k_i in_i) / .bias, feature_extractor.weight (xvector, 2 tdnn_dim[-1]) / .bias,
 * classifier.weight (xvector, xvector) / .bias. */
typedef struct vx_spk vx_spk;
enum { VX_SPK_WAVLM = 0, VX_SPK_PLAIN = 1 };
enum { VX_SPK_KEEP_TAPS = 1 };  /* vx_spk_config.flags: every hidden state keeps a buffer of its own ("hidden<l>" can be read) */
enum { VX_SPK_NORMALIZE = 1 };  /* vx_spk_embed flags */
typedef struct vx_spk_config {
  int32_t struct_size;            /* sizeof(vx_spk_config) */
  int32_t attention;              /* VX_SPK_* */
  int32_t hidden, layers, heads, ffn;
  int32_t n_conv;                 /* 1 .. 8 */
  int32_t conv_dim[8], conv_kernel[8], conv_stride[8];
  int32_t conv_bias;              /* 0 / 1 */
  int32_t pos_kernel, pos_groups;
  int32_t num_buckets;            /* rows of rel_attn_embed */
  int32_t n_tdnn;                 /* 1 .. 8 */
  int32_t tdnn_dim[8], tdnn_kernel[8], tdnn_dilation[8];
  int32_t xvector;
  int32_t use_weighted_layer_sum; /* 0 / 1 */
  int32_t feat_extract_norm;      /* 0 = "group" (served), 1 = "layer" */
  int32_t do_stable_layer_norm;   /* 0 (served) / 1 */
  int32_t add_adapter;            /* 0 (served) / 1 */
  int32_t activation;             /* 0 = gelu (served) */
  float layer_norm_eps;
  int32_t max_batch;              /* utterances per call, <= 64 */
  int32_t max_samples;            /* samples per utterance */
  int32_t flags;                  /* VX_SPK_KEEP_TAPS */
} vx_spk_config;
/* Host only, no HIP call.  In this order: nulls, a wrong struct_size, a count or size outside its range (n_conv, n_tdnn in 1 .. 8;
 * every dimension, kernel, stride, dilation >= 1; heads dividing hidden, pos_groups dividing hidden; an attention outside VX_SPK_*;
 * max_batch < 1; eps not finite) -> VX_ERR_ARG; then feat_extract_norm = 1, do_stable_layer_norm, add_adapter, an activation
 * other than gelu, a head_dim other than 16, 32 or 64, conv_kernel[0] > 32 or conv_stride[0] > 32, max_batch > 64 ->
 * VX_ERR_UNSUPPORTED; then max_samples below vx_spk_min_samples -> VX_ERR_ARG; then max_batch x the layer-0 frames of max_samples
 * above 2^31 - 1 rows -> VX_ERR_UNSUPPORTED.  The workspace is sized from (max_batch, max_samples) and allocated on the device
 * current at the first vx_spk_embed. */
int vx_spk_create(const vx_spk_config* cfg, vx_spk** out);
void vx_spk_destroy(vx_spk* h);
/* Host only.  data: HOST fp32 of `shape`.  Unknown key or wrong shape -> VX_ERR_WEIGHTS; after vx_spk_finalize -> VX_ERR_STATE. */
int vx_spk_set_weight(vx_spk* h, const char* key, const float* data, const int64_t* shape, int32_t ndim);
/* Host only, VX_SPK_WAVLM: idx[r + Tmax - 1] = the row of rel_attn_embed for the relative position r = j - i, for every r in
 * [-(Tmax - 1), Tmax - 1], Tmax = vx_spk_frames(max_samples); n must be 2 Tmax - 1 and every index inside [0, num_buckets), else
 * VX_ERR_ARG.  The caller computes them by WavLM's rule (positive r offset by num_buckets / 2, exact below num_buckets / 4,
 * logarithmic above with the logarithm in fp32, saturated at max_bucket_distance): the library does not re-derive them. */
int vx_spk_set_buckets(vx_spk* h, const int32_t* idx, int32_t n);
/* Host only: every tensor is there (a missing one -> VX_ERR_WEIGHTS naming it; VX_SPK_WAVLM without buckets -> VX_ERR_STATE); packs
 * the weights, builds the per-head bias table (H, 2 Tmax - 1) and soft-maxes layer_weights in fp64. */
int vx_spk_finalize(vx_spk* h);
/* Frames the feature encoder leaves of n_samples (0 when too few for one); -1 for a null handle.  Host only. */
int64_t vx_spk_frames(const vx_spk* h, int64_t n_samples);
/* The shortest utterance served: the one that leaves two pooled frames (5200 at the default strides and TDNN kernels). */
int64_t vx_spk_min_samples(const vx_spk* h);
/* n utterances: wav[i] DEVICE fp32 of n_samples[i] samples at 16 kHz; emb_out DEVICE fp32 (n, xvector); logits_out NULL or DEVICE
 * fp32 (n, xvector).  The pointer array and n_samples live on the host.  Every utterance is bitwise what it is alone, and two
 * identical calls give the same bits.  Checked before any HIP call, in this order: null arguments (logits_out excepted), n < 1,
 * unknown flags -> VX_ERR_ARG; not finalized -> VX_ERR_STATE; n > max_batch -> VX_ERR_CAPACITY; then per utterance a null pointer
 * or n_samples[i] < vx_spk_min_samples (the message states both lengths) -> VX_ERR_ARG, n_samples[i] > max_samples ->
 * VX_ERR_CAPACITY.  The work is enqueued on `stream`; the host waits only for the previous call's staging copy.  Calls on one
 * handle must not overlap. */
int vx_spk_embed(vx_spk* h, int32_t n, const float* const* wav, const int32_t* n_samples, int32_t flags, float* emb_out,
                 float* logits_out, void* stream);
/* out[p] = cosine of a[p] and b[p], DEVICE fp32 (n, xvector) each, out DEVICE fp32 (n).  Nulls or n < 1 -> VX_ERR_ARG. */
int vx_spk_similarity(vx_spk* h, int32_t n, const float* a, const float* b, float* out, void* stream);
/* A read tap for the tests: waits for the last vx_spk_embed and copies utterance `utt`'s part of "features", "hidden<l>" (needs
 * VX_SPK_KEEP_TAPS), "gate<l>", "layer_sum", "tdnn" or "pooled" to dst (HOST fp32).  n_floats must be the tap's size (rows x
 * width), else VX_ERR_ARG naming it; an unknown name -> VX_ERR_ARG; no call yet, or hidden<l> without the flag -> VX_ERR_STATE. */
int vx_spk_read(vx_spk* h, const char* name, int32_t utt, float* dst, int64_t n_floats);
/* out[0] = host milliseconds the last vx_spk_embed took to enqueue, out[1] = workspace bytes, out[2] = weight bytes, out[3] =
 * encoder rows of the last call; n = how many of them are wanted (<= 4). */
int vx_spk_get_timings(const vx_spk* h, double* out, int32_t n);

/* ---- CTC speech recogniser: Wav2Vec2ForCTC / HubertForCTC, a 16 kHz waveform to token ids; the edit distance behind WER / CER ------
 * A handle of its own, fp32 storage and accumulation.  The network is the speaker encoder's (above: the same steps, the same
 * kernels, VX_SPK_PLAIN attention) up to the last hidden state, in one of two flavours, and a Linear head.  Notation as above.
 *   0. VX_ASR_NORMALIZE (a flag of the call): as VX_SPK_NORMALIZE.
 *   1. feature encoder.  group flavour (feat_extract_norm = 0): as the speaker encoder's.  layer flavour (feat_extract_norm = 1):
 *      every layer i = Conv1d(C_{i-1} -> C_i, k_i, s_i) with bias, then LayerNorm over the C_i channels of each frame (biased
 *      variance, eps 1e-5, affine), then GELU.  Taps "conv0" (T_0, C_0) after layer 0 and "features" (T, C) after the last.
 *   2. projection: LayerNorm(C) (eps = layer_norm_eps, as every LayerNorm below; skipped when feat_proj_layer_norm = 0), Linear C -> d.
 *   3. positional convolution p = gelu(Conv1d(d -> d, k = pos_kernel, padding k / 2, groups = pos_groups)), the last output frame
 *      dropped when k is even.
 *   4. encoder.  post-norm (do_stable_layer_norm = 0): h = LN_enc(h + p) (tap "hidden0"), then per layer h = LN1(h + Attn(h));
 *      h = LN2(h + FFN(h)) (tap "hidden<l+1>").  stable (do_stable_layer_norm = 1): h = h + p (tap "hidden0"), then per layer
 *      h = h + Attn(LN1(h)); h = h + FFN(LN2(h)) (tap "hidden<l+1>" for l + 1 < L), and after the last layer h = LN_enc(h) (tap
 *      "hidden<L>").  LN1 = layers.{l}.layer_norm, LN2 = layers.{l}.final_layer_norm, LN_enc = encoder.layer_norm;
 *      FFN(x) = W2 gelu(W1 x + b1) + b2; Attn as VX_SPK_PLAIN.  The residual is always the un-normed stream.
 *   5. logits = lm_head h (T, vocab), tap "logits".
 *   6. greedy CTC decode (vx_ctc_greedy on its own): per frame id[t] = argmax of the logits, the lowest index among equal maxima,
 *      and lp[t] = x[id] - log sum_c exp(x[c]) with the sum of exp(x[c] - x[id]) taken in fp64; frame t is kept when
 *      id[t] != blank and (t == 0 or id[t] != id[t - 1]): repeats are merged first, blanks removed second (A A _ A gives A A).
 *      Per utterance: the kept ids and their frame indices in frame order, their count, and the mean of lp over ALL frames.
 * Edit distance (vx_edit_distance): Levenshtein with unit costs between a reference and a hypothesis, D(i, 0) = i deletions,
 * D(0, j) = j insertions, D(i, j) = the cheapest of D(i-1, j-1) + [ref_i != hyp_j] (a match or a substitution), D(i-1, j) + 1 (a
 * deletion) and D(i, j-1) + 1 (an insertion); among equal costs the first in that order is taken, and S / D / I are the
 * counts along that choice: those of a backtrace from (R, H) with the same preference.
 * Weight keys (fp32, host, torch layouts, transformers' names without the wav2vec2. / hubert. prefix, weight norm folded): as the
 * speaker encoder's feature encoder, projection and encoder without the WavLM tensors; layer flavour: every
 * feature_extractor.conv_layers.{i}.layer_norm.* and .conv.bias; feature_projection.layer_norm.* only with feat_proj_layer_norm;
 * lm_head.weight (vocab, d) / .bias.
 * The bf16 encoder mode (VX_ASR_ENC_BF16, opt-in; VX_WSP_ENC_BF16 is the same mode of the Whisper recogniser's encoder): the
 * pre-norm layers of step 4's stable flavour run on the bf16 matrix cores; everything else - the feature encoder, the projection,
 * the positional convolution, the head, the decode, the alignment - is the fp32 mode's, launch for launch.
 *   Rounded to bf16, round-to-nearest-even: the weights of the four linears of every encoder layer (q | k | v stacked, out_proj,
 *   W1, W2), once, at *_finalize (the device keeps no fp32 copy of them); and every operand of those four GEMMs and of the two
 *   attention products: the LayerNorm outputs LN1(h) and LN2(h), q, k, v, the attention probabilities before P.V, the attention
 *   output, and gelu(W1 x + b1).
 *   Kept in fp32: all accumulation; the softmax statistics (the row maximum and the sum, which is taken over the unrounded
 *   probabilities); biases and LayerNorm parameters; the residual stream - out_proj and W2 add their bias and the residual in
 *   fp32 and store fp32; LN_enc and its output.  The taps "hidden<l>" / "enc<l>" / "encoder" keep their meaning and their type.
 * The softmax is an online one: the probabilities are rounded unnormalised, exp(s - running maximum), and the output is divided
 * by the fp32 sum at the end; a restatement that rounds the normalised probabilities differs by a rounding of the same size, which
 * the test bound covers.  Served: the stable flavour, head_dim 64, ffn a multiple of 64 (every released pre-norm width: d = 384,
 * 512, 768, 1024, 1280 with ffn = 4 d); anything else -> VX_ERR_UNSUPPORTED at create.  A ragged batch stays bitwise what each
 * utterance is alone, and a call is repeatable bit for bit: no atomics, every sum in a fixed order. */
typedef struct vx_asr vx_asr;
enum {
  VX_ASR_KEEP_TAPS = 1, /* vx_asr_config.flags: every hidden state keeps a buffer of its own ("hidden<l>" can be read) */
  VX_ASR_ENC_BF16 = 2   /* vx_asr_config.flags: the bf16 encoder mode above */
};
enum { VX_ASR_NORMALIZE = 1 };  /* vx_asr_recognize flags */
typedef struct vx_asr_config {
  int32_t struct_size;            /* sizeof(vx_asr_config) */
  int32_t hidden, layers, heads, ffn;
  int32_t n_conv;                 /* 1 .. 8 */
  int32_t conv_dim[8], conv_kernel[8], conv_stride[8];
  int32_t conv_bias;              /* 0 / 1 */
  int32_t pos_kernel, pos_groups;
  int32_t vocab, blank;           /* rows of lm_head; the CTC blank (the tokenizer's <pad>) */
  int32_t feat_extract_norm;      /* 0 = "group", 1 = "layer" */
  int32_t do_stable_layer_norm;   /* 0 / 1; served together with feat_extract_norm: 0 / 0 and 1 / 1 */
  int32_t feat_proj_layer_norm;   /* 1 (Wav2Vec2 always) / 0 (HuBERT's option) */
  int32_t add_adapter;            /* 0 (served) / 1 */
  int32_t conv_pos_batch_norm;    /* 0 (served) / 1 */
  int32_t activation;             /* 0 = gelu (served) */
  float layer_norm_eps;
  int32_t max_batch;              /* utterances per call, <= 64 */
  int32_t max_samples;            /* samples per utterance */
  int32_t flags;                  /* VX_ASR_KEEP_TAPS | VX_ASR_ENC_BF16 */
} vx_asr_config;
/* Host only, no HIP call.  In this order: nulls, a wrong struct_size, a count or size outside its range (as vx_spk_create; vocab
 * < 1, blank outside [0, vocab)) -> VX_ERR_ARG; then add_adapter, conv_pos_batch_norm, an activation other than gelu,
 * feat_extract_norm != do_stable_layer_norm (a mix the released checkpoints do not have), the layer flavour without conv_bias, a
 * head_dim other than 16, 32 or 64, conv_kernel[0] > 32 or conv_stride[0] > 32, layer flavour: conv_dim[0] > 1024 or a layer-0 tile
 * (63 stride + k + k C_0 floats) above 60 KiB, max_batch > 64 -> VX_ERR_UNSUPPORTED with the field named; then max_samples below
 * vx_asr_min_samples -> VX_ERR_ARG; then max_batch x the layer-0 frames of max_samples above 2^31 - 1 -> VX_ERR_UNSUPPORTED.
 * VX_ASR_ENC_BF16 (after the max_batch check): the group / post-norm flavour, a head_dim other than 64, an ffn that is no multiple
 * of 64 -> VX_ERR_UNSUPPORTED with the field named. */
int vx_asr_create(const vx_asr_config* cfg, vx_asr** out);
void vx_asr_destroy(vx_asr* h);
/* Host only.  data: HOST fp32 of `shape`.  Unknown key or wrong shape -> VX_ERR_WEIGHTS; after vx_asr_finalize -> VX_ERR_STATE. */
int vx_asr_set_weight(vx_asr* h, const char* key, const float* data, const int64_t* shape, int32_t ndim);
/* Host only: every tensor is there (a missing one -> VX_ERR_WEIGHTS naming it); packs the weights. */
int vx_asr_finalize(vx_asr* h);
/* Frames the feature encoder leaves of n_samples (0 when too few for one); -1 for a null handle.  Host only. */
int64_t vx_asr_frames(const vx_asr* h, int64_t n_samples);
/* The shortest utterance served: the one that leaves one encoder frame (400 samples at the default kernels and strides). */
int64_t vx_asr_min_samples(const vx_asr* h);
/* n utterances: wav[i] DEVICE fp32 of n_samples[i] samples at 16 kHz.  With T_i = vx_asr_frames(n_samples[i]) and o_i = T_0 + ..
 * + T_{i-1}: tokens_out and token_frames_out are DEVICE int32 of sum T_i entries, utterance i's kept ids and their frame indices at
 * o_i .. o_i + counts_out[i] (the rest of its T_i entries is not written); counts_out DEVICE int32 (n); mean_logprob_out DEVICE
 * fp32 (n); logits_out NULL or DEVICE fp32 (sum T_i, vocab).  The pointer array and n_samples live on the host.  Every utterance is
 * bitwise what it is alone, and two identical calls give the same bits.  Checked before any HIP call, in this order: null
 * arguments (logits_out excepted), n < 1, unknown flags -> VX_ERR_ARG; not finalized -> VX_ERR_STATE; n > max_batch ->
 * VX_ERR_CAPACITY; then per utterance a null pointer or n_samples[i] < vx_asr_min_samples (the message states both lengths) ->
 * VX_ERR_ARG, n_samples[i] > max_samples -> VX_ERR_CAPACITY.  The work is enqueued on `stream`; the host waits only for the
 * previous call's staging copy.  Calls on one handle must not overlap. */
int vx_asr_recognize(vx_asr* h, int32_t n, const float* const* wav, const int32_t* n_samples, int32_t flags, int32_t* tokens_out,
                     int32_t* token_frames_out, int32_t* counts_out, float* mean_logprob_out, float* logits_out, void* stream);
/* A read tap for the tests: waits for the last vx_asr_recognize and copies utterance `utt`'s part of "conv0", "features",
 * "hidden<l>" (needs VX_ASR_KEEP_TAPS) or "logits" to dst (HOST fp32).  n_floats must be the tap's size (rows x width), else
 * VX_ERR_ARG naming it; an unknown name -> VX_ERR_ARG; no call yet, or hidden<l> without the flag -> VX_ERR_STATE. */
int vx_asr_read(vx_asr* h, const char* name, int32_t utt, float* dst, int64_t n_floats);
/* out[0] = host milliseconds the last vx_asr_recognize took to enqueue, out[1] = workspace bytes, out[2] = weight bytes, out[3] =
 * encoder rows of the last call; n = how many of them are wanted (<= 4). */
int vx_asr_get_timings(const vx_asr* h, double* out, int32_t n);
/* Step 6 on its own, on the current device: logits DEVICE fp32 (sum frames[i], vocab), the utterances' rows concatenated; frames
 * HOST (n), each >= 0; outputs as vx_asr_recognize's (an utterance without frames: count 0, mean 0); frame_logprob_out NULL or
 * DEVICE fp32 (sum frames[i]): lp[t] rounded to fp32.  Nulls, n < 1, vocab < 1, blank outside [0, vocab), a negative frame count
 * -> VX_ERR_ARG.  Allocates its scratch and waits for `stream` before it returns (a test and tool entry, not a hot path). */
int vx_ctc_greedy(const float* logits, int32_t vocab, int32_t blank, int32_t n, const int32_t* frames, int32_t* tokens_out,
                  int32_t* token_frames_out, int32_t* counts_out, float* mean_logprob_out, float* frame_logprob_out, void* stream);
/* n pairs on the current device: ref / hyp DEVICE int32, the pairs' sequences concatenated (pair p's at the sum of the lengths
 * before it); ref_len / hyp_len HOST (n), each in [0, 2048]; out DEVICE int32 (n, 4): distance, substitutions, deletions,
 * insertions.  A zero-length side is legal.  Nulls (a sequence pointer may be null when its lengths are all 0), n < 1, a negative
 * length or one above 2048 (the message states the limit: three diagonals of 64-bit cells in LDS) -> VX_ERR_ARG.  Waits for
 * `stream` before it returns. */
int vx_edit_distance(int32_t n, const int32_t* ref, const int32_t* ref_len, const int32_t* hyp, const int32_t* hyp_len, int32_t* out,
                     void* stream);

/* ---- CTC forced alignment and text likelihood: a known text against the logits of the recogniser above ----------------------------
 * Two questions about a text that is already known: how likely it is under the audio (the forward algorithm), and where in the
 * audio each of its tokens sits (the Viterbi path through the same lattice, the rule of torchaudio's forced_align).
 * Inputs and the extended sequence.  Per utterance: logits x (T, V) fp32, a blank id b, target ids y[0..L), each in [0, V) and not
 * b.  The extended sequence z has S = 2 L + 1 states, z[2k] = b and z[2k+1] = y[k].  lse[t] = m + log sum_c exp(x[t][c] - m) with
 * m = max_c x[t][c] and the sum in fp64, as step 6 above takes it.  e[t][s] = (double)x[t][z[s]] - lse[t].  State s may be entered
 * from s and from s - 1, and from s - 2 when z[s] != b and z[s] != z[s-2].
 * Likelihood.  a[0][0] = e[0][0], a[0][1] = e[0][1], the rest -inf; a[t][s] = e[t][s] + logaddexp over the allowed predecessors at
 * t - 1, in fp64; nll = -logaddexp(a[T-1][S-1], a[T-1][S-2]), for L = 0 nll = -a[T-1][0].  An infeasible pair has nll = +inf and
 * feasible = 0, never a NaN: a pair is infeasible when T < L + #{k : y[k] == y[k-1]}, or when T = 0 with L > 0.  T = 0 with L = 0
 * gives nll = 0 (and path_logprob = 0).
 * Best path.  The same recurrence with max, on the raw logits: v[t][s] = max(...) + (double)x[t][z[s]] (lse[t] is constant over the
 * states of a frame, so it does not move the arg-max): only IEEE additions and comparisons in fp64, so that another
 * implementation of this text agrees cell for cell.  Among equal predecessors the first in the order s, s - 1, s - 2 is taken; at
 * the end S - 1 is taken before S - 2.
 * Reported.  path_logprob = v_end - sum_t lse[t]; per frame the index k of the target token it emits, or -1 for blank; per target
 * token its frames [start, end) and score = the mean of e over them, summed in fp64 in frame order and rounded to fp32.  For an
 * infeasible utterance the frame tokens and spans are -1, the scores -inf, nll = +inf and path_logprob = -inf.
 * Kernel: one workgroup per utterance, a ragged batch in one launch; a and v are double-buffered fp64 rows in LDS with one barrier
 * per frame; states outside the reachable band (s < 2 t + 2 and S - 1 - s < 2 (T - t)) are not computed; the back-pointers are 2
 * bits per cell in a workspace, and the backtrace, the spans and the scores run on the device.  No atomics: every utterance is
 * bitwise what it is alone, and two identical calls give the same bits.  Limits: L <= 1000 targets per utterance (four fp64 rows
 * of 2 L + 3 cells in 64 KiB of LDS; 20 s of audio are 999 frames, and a longer text cannot be feasible in them), any T, and
 * frames x states / 4 bytes of back-pointers summed over the call <= 2 GiB. */
/* On the current device.  logits DEVICE fp32 (sum frames[i], vocab), the utterances' rows concatenated; frames, targets (the
 * utterances' ids concatenated) and target_len HOST int32.  nll_out, path_logprob_out DEVICE fp64 (n); frame_token_out DEVICE int32
 * (sum frames[i]); tok_start_out, tok_end_out DEVICE int32 and tok_score_out DEVICE fp32 (sum target_len[i]); feasible_out DEVICE
 * int32 (n).  Any output may be null: without nll_out the sum is skipped, without all of path_logprob_out .. tok_score_out the max.
 * Checked before any HIP call: null logits / frames / target_len, no output at all, n < 1, vocab < 1, blank outside [0, vocab), a
 * negative count, null targets with a positive count, a target id equal to blank or outside [0, vocab) (the message states the
 * utterance, the position and the id) -> VX_ERR_ARG; a feasible utterance above a limit -> VX_ERR_CAPACITY naming the limit.
 * Allocates its scratch and waits for `stream` before it returns. */
int vx_falign(const float* logits, int32_t vocab, int32_t blank, int32_t n, const int32_t* frames, const int32_t* targets,
              const int32_t* target_len, double* nll_out, double* path_logprob_out, int32_t* frame_token_out, int32_t* tok_start_out,
              int32_t* tok_end_out, float* tok_score_out, int32_t* feasible_out, void* stream);
/* The same on the logits the last vx_asr_recognize on `h` left on the device (frames, vocab and blank are that call's and the
 * handle's): error rate and timestamps from one pass of the network, without a host round trip of the logits.  No previous call,
 * or n other than that call's -> VX_ERR_STATE; the other checks as above.  The scratch is the handle's and only grows;
 * vx_asr_get_timings' workspace figure includes it.  Waits for `stream` before it returns. */
int vx_falign_asr(vx_asr* h, int32_t n, const int32_t* targets, const int32_t* target_len, double* nll_out, double* path_logprob_out,
                  int32_t* frame_token_out, int32_t* tok_start_out, int32_t* tok_end_out, float* tok_score_out, int32_t* feasible_out,
                  void* stream);

/* ---- Whisper recogniser: WhisperForConditionalGeneration, a 16 kHz waveform to token ids by greedy decoding -------------------------
 * A handle of its own, fp32 storage and accumulation.  Every shape comes from the checkpoint's config.json.  P =
 * max_source_positions, Tt = max_target_positions, d = d_model, head_dim = 64; a chunk is 320 P samples (480 000 at P = 1500).
 *   1. log-mel.  The waveform is zero-padded to the chunk and framed as torch.stft(n_fft = 400, hop = 160, center = True, pad_mode =
 *      "reflect") with the periodic Hann window; power spectrum (201 bins); the last frame is dropped, 2 P frames are left; mel =
 *      mel_filters (n_mels, 201) applied to the power (the caller's table: Slaney scale and norm, 0 .. 8000 Hz, built in fp64);
 *      x = log10(max(mel, 1e-10)); x = max(x, max over the utterance of x - 8); x = (x + 4) / 4.  Tap "logmel" (2 P, n_mels).
 *   2. encoder.  gelu(Conv1d(n_mels -> d, k 3, pad 1)) (tap "conv1" (2 P, d)); gelu(Conv1d(d -> d, k 3, stride 2, pad 1)) (tap
 *      "features" (P, d)); h = that + embed_positions (tap "enc0"); per layer h = h + Attn(LN1(h)); h = h + W2 gelu(W1 LN2(h) + b1) +
 *      b2 (tap "enc<l+1>"); then LN_enc(h) (tap "encoder").  Attn: q, v and out with bias, k without, softmax(q k / 8) v per head
 *      over all P rows of the utterance: there is no attention mask, the padded part of the chunk takes part as in transformers.
 *      gelu is the exact one; every LayerNorm has eps 1e-5.
 *   3. decoder.  x = embed_tokens[id] + embed_positions[pos]; per layer x = x + SelfAttn(LN1(x)) over positions 0 .. pos (causal),
 *      x = x + CrossAttn(LN2(x)) with keys and values from the encoder output (after LN_enc), x = x + FFN(LN3(x)); then
 *      LN_dec(x); logits = proj_out.weight x, the token embedding when tie_proj = 1.
 *   4. greedy generation.  The decoder input starts with the utterance's prompt_ids.  Generated step g reads the logits of the last
 *      position: tokens of suppress_tokens are set to -inf, at g = 0 those of begin_suppress_tokens too; the token is the argmax, the
 *      lowest index among equal maxima; its log-probability is x[token] - m - log sum_c exp(x[c] - m) over that processed row, m its
 *      maximum and the sum in fp64, rounded to fp32.  The utterance stops (in this order) on eos_token_id (stop reason 1), on its
 *      max_new_tokens (2), or when the sequence, the new token included, has Tt tokens (3); the last token is reported.  A stopped
 *      utterance's later steps change none of its outputs.
 *   5. teacher forcing (forced != NULL): the same steps with forced[i][g] in place of the argmax, max_new_tokens[i] of them; eos
 *      does not stop it, and logprobs_out is every step's log-probability of the given token.
 * The host enqueues 8 decode steps at a time and reads the finished flags between them; no token is read back.  Every utterance is
 * bitwise what it is alone, and two identical calls give the same bits.
 * Weight keys (fp32, host, torch layouts, transformers' names): mel_filters (n_mels, 201); model.encoder.conv1 / conv2 .weight /
 * .bias; model.encoder.embed_positions.weight (P, d); model.encoder.layers.{l}.self_attn.{q,v,out}_proj.weight / .bias and
 * .k_proj.weight, .self_attn_layer_norm.*, .fc1.*, .fc2.*, .final_layer_norm.*; model.encoder.layer_norm.*;
 * model.decoder.embed_tokens.weight (vocab, d), model.decoder.embed_positions.weight (Tt, d), model.decoder.layers.{l}. as the
 * encoder's plus .encoder_attn.* and .encoder_attn_layer_norm.*; model.decoder.layer_norm.*; proj_out.weight (vocab, d) only with
 * tie_proj = 0.
 * VX_WSP_ENC_BF16 (opt-in): the encoder layers of step 2 in the bf16 encoder mode defined with the CTC recogniser above (LN1, LN2,
 * q, k, v, the probabilities, the attention output and gelu(W1 ..) rounded to bf16, the four matrices of every layer kept in bf16
 * only; "enc<l>" and "encoder" stay fp32).  The log-mel front end, conv1 / conv2, the cross-attention K / V projections and the
 * whole token loop are the fp32 mode's.
 * Not built: beam search, temperature fallback, timestamps, language detection, long-form transcription, a bf16 token loop. */
typedef struct vx_wsp vx_wsp;
enum {
  VX_WSP_KEEP_TAPS = 1, /* vx_wsp_config.flags: "enc<l>" and the per-step "logits" keep buffers of their own */
  VX_WSP_ENC_BF16 = 2   /* vx_wsp_config.flags: the encoder layers in the bf16 encoder mode */
};
enum { VX_WSP_STOP_EOS = 1, VX_WSP_STOP_MAX_NEW = 2, VX_WSP_STOP_MAX_TARGET = 3 };
typedef struct vx_wsp_config {
  int32_t struct_size;            /* sizeof(vx_wsp_config) */
  int32_t n_mels, d_model;        /* num_mel_bins (a multiple of 16), d_model */
  int32_t enc_layers, enc_heads, enc_ffn;
  int32_t dec_layers, dec_heads, dec_ffn;
  int32_t max_source_positions, max_target_positions;
  int32_t vocab;
  int32_t activation;             /* 0 = gelu (served) */
  int32_t tie_proj;               /* 1: proj_out.weight is model.decoder.embed_tokens.weight */
  int32_t eos_token_id;
  int32_t max_batch;              /* utterances per call, <= 64 */
  int32_t flags;                  /* VX_WSP_KEEP_TAPS | VX_WSP_ENC_BF16 */
} vx_wsp_config;
/* Host only, no HIP call.  In this order: nulls, a wrong struct_size, a count or size below 1 (max_target_positions below 2),
 * eos_token_id outside [0, vocab), unknown flags -> VX_ERR_ARG; then an activation other than gelu, a head_dim other than 64,
 * num_mel_bins or an ffn dim that is no multiple of 16, more than 4096 source or target positions, max_batch > 64 ->
 * VX_ERR_UNSUPPORTED with the field named; then, with VX_WSP_ENC_BF16, an encoder_ffn_dim that is no multiple of 64 ->
 * VX_ERR_UNSUPPORTED naming it. */
int vx_wsp_create(const vx_wsp_config* cfg, vx_wsp** out);
void vx_wsp_destroy(vx_wsp* h);
/* Host only.  data: HOST fp32 of `shape`.  Unknown key or wrong shape -> VX_ERR_WEIGHTS; after vx_wsp_finalize -> VX_ERR_STATE. */
int vx_wsp_set_weight(vx_wsp* h, const char* key, const float* data, const int64_t* shape, int32_t ndim);
/* Host only: the generation config's suppress_tokens and begin_suppress_tokens (HOST int32, either may be empty); replaces what was
 * set before.  An id outside [0, vocab) -> VX_ERR_ARG naming the list; after vx_wsp_finalize -> VX_ERR_STATE. */
int vx_wsp_set_suppress(vx_wsp* h, const int32_t* ids, int32_t n_ids, const int32_t* begin_ids, int32_t n_begin);
/* Host only: every tensor is there (a missing one -> VX_ERR_WEIGHTS naming it); packs the weights and builds the DFT table. */
int vx_wsp_finalize(vx_wsp* h);
/* n utterances: wav[i] DEVICE fp32 of n_samples[i] samples at 16 kHz (the pointer array and every int array below live on the host).
 * prompt_ids (n, prompt_stride), utterance i's first n_prompt[i] entries; max_new_tokens (n), each in [1, out_stride]; forced NULL
 * or (n, out_stride), utterance i's first max_new_tokens[i] entries.  tokens_out DEVICE int32 and logprobs_out DEVICE fp32 (n,
 * out_stride): utterance i's first counts_out[i] entries are written, the rest is left alone; counts_out and stops_out DEVICE int32
 * (n).  Checked before any HIP call, in this order: null arguments (forced excepted), n < 1 -> VX_ERR_ARG; not finalized ->
 * VX_ERR_STATE; n > max_batch -> VX_ERR_CAPACITY; strides below 1 or out_stride > Tt -> VX_ERR_ARG; then per utterance: a null
 * pointer or n_samples[i] < 0 -> VX_ERR_ARG; n_samples[i] above the chunk -> VX_ERR_CAPACITY (long-form is not built); an empty
 * prompt_ids -> VX_ERR_ARG; a prompt that leaves no room under max_target_positions -> VX_ERR_CAPACITY; an id outside [0, vocab),
 * max_new_tokens[i] outside its range -> VX_ERR_ARG; forced tokens that do not fit under max_target_positions -> VX_ERR_CAPACITY.
 * The work is enqueued on `stream`, and the host waits for it between groups of 8 decode steps.  Calls on one handle must not
 * overlap. */
int vx_wsp_recognize(vx_wsp* h, int32_t n, const float* const* wav, const int32_t* n_samples, const int32_t* prompt_ids,
                     const int32_t* n_prompt, int32_t prompt_stride, const int32_t* max_new_tokens, const int32_t* forced,
                     int32_t out_stride, int32_t* tokens_out, float* logprobs_out, int32_t* counts_out, int32_t* stops_out, void* stream);
/* A read tap for the tests: waits for the last vx_wsp_recognize and copies utterance `utt`'s "logmel", "conv1", "features",
 * "enc<l>" (0 .. enc_layers; needs VX_WSP_KEEP_TAPS), "encoder" or "logits" (needs VX_WSP_KEEP_TAPS: the raw rows (count, vocab) of
 * its generated steps) to dst (HOST fp32).  n_floats must be the tap's size, else VX_ERR_ARG naming it; an unknown name ->
 * VX_ERR_ARG; no call yet, or a tap without its flag -> VX_ERR_STATE. */
int vx_wsp_read(vx_wsp* h, const char* name, int32_t utt, float* dst, int64_t n_floats);
/* out[0] = host milliseconds the last vx_wsp_recognize took, out[1] = workspace bytes, out[2] = weight bytes, out[3] = decode steps
 * it enqueued, out[4 .. 6] = device milliseconds of its log-mel, encoder (cross keys and values included) and token loop (asking
 * for them waits for the call); n = how many are wanted (<= 7). */
int vx_wsp_get_timings(vx_wsp* h, double* out, int32_t n);
/* Test-only, like the vx_op_* entries above: the token loop's kernels on caller data, through the launchers vx_wsp_recognize uses
 * (they choose the columns per workgroup, the K chunk, the grid and the LDS size).  Every pointer is DEVICE; each call waits for
 * its work.  The argument checks come before any launch.
 * vx_op_wsp_gemm: out (M, N) = act(x (M, K) . W (N, K)^T + bias) + res; bias (N) or NULL, res (M, N) or NULL (it may be `out`),
 * act 0 none / 1 exact GELU.  K no multiple of 4, M > 64, a size below 1 -> VX_ERR_ARG.
 * vx_op_wsp_decode_attn: n utterances x H heads of 64, scale 1/8.  Utterance u's key (value) row j is kcache (vcache) + (u
 * rows_per_utt + j) ld, head h at columns 64 h; q, knew, vnew rows have ldq floats, out (n, d), d = 64 H.  Self-attention: knew,
 * vnew and pos (n) given; utterance u attends to keys 0 .. pos[u], the last of which is knew / vnew, which the kernel also stores
 * to cache row pos[u].  Cross-attention: all three NULL, `keys` keys per utterance.  max_keys sizes the LDS (scores of at most
 * that many keys): above 4096, or below a pos[u] + 1 or `keys`, or rows_per_utt below them -> VX_ERR_ARG.
 * vx_op_wsp_head: one greedy (forced: teacher-forced) step on logits (n, V), as point 4 and 5 of the definition above.  suppress
 * (V) bytes: bit 0 suppress_tokens, bit 1 begin_suppress_tokens.  prompt (n, prompt_stride), n_prompt, max_new (n), forced NULL
 * or (n, out_stride); cur, pos, count, finished (n) are the utterances' state, read and advanced: pos[u] is the position the
 * logits belong to; inside the prompt (pos[u] + 1 < n_prompt[u]) the next prompt token is fed and no output is written; a
 * finished utterance changes nothing.  tokens_out / logprobs_out (n, out_stride) get step g = pos[u] + 1 - n_prompt[u];
 * counts_out, stops_out (n).  A step outside out_stride, a forced id or eos outside [0, V) -> VX_ERR_ARG.
 * vx_op_wsp_embed: x (n, d) = tok_emb[cur[u]] + pos_emb[pos[u]]; tok_emb (vocab, d), pos_emb (max_pos, d); an index outside its
 * table -> VX_ERR_ARG. */
int vx_op_wsp_gemm(const float* x, const float* W, const float* bias, const float* res, float* out, int32_t M, int32_t N, int32_t K,
                   int32_t act, void* stream);
int vx_op_wsp_decode_attn(const float* q, const float* knew, const float* vnew, float* kcache, float* vcache, float* out, int32_t ld,
                          int32_t ldq, int32_t d, int32_t H, int32_t n, const int32_t* pos, int32_t keys, int64_t rows_per_utt,
                          int32_t max_keys, void* stream);
int vx_op_wsp_head(const float* logits, int32_t n, int32_t V, const uint8_t* suppress, const int32_t* prompt, int32_t prompt_stride,
                   const int32_t* n_prompt, const int32_t* max_new, const int32_t* forced, int32_t* cur, int32_t* pos, int32_t* count,
                   int32_t* finished, int32_t* tokens_out, float* logprobs_out, int32_t* counts_out, int32_t* stops_out,
                   int32_t out_stride, int32_t eos, int32_t max_target, void* stream);
int vx_op_wsp_embed(const float* tok_emb, const float* pos_emb, const int32_t* cur, const int32_t* pos, float* x, int32_t n, int32_t d,
                    int32_t vocab, int32_t max_pos, void* stream);
/* Test-only: the bf16 encoder mode's kernels on caller data, through the launchers the recognisers use.  Every pointer is DEVICE
 * unless said otherwise; each call waits for its work.
 * vx_op_enc16_gemm: A (M, K) and W (N, K) bf16, bias (N) fp32.  epi 0: out (M, N) bf16 = A W^T + bias; 1: bf16 = gelu(A W^T + bias),
 * the exact GELU; 2: out (M, N) fp32 = (A W^T + bias) + res, res (M, N) fp32 (it may be `out`).  N no multiple of 8, K no multiple
 * of 64, a null operand, an unknown epi -> VX_ERR_ARG.
 * vx_op_enc16_add_ln: s = a[row] + b[bmod > 0 ? row % bmod : row] (b NULL: s = a[row]) to sum (fp32, NULL: not stored; it may be
 * a); y (M, d) bf16 = LayerNorm(s) w + beta.
 * vx_op_enc16_attn: qkv (rows, 3 x 64 heads) bf16 -> out (rows, 64 heads) bf16, softmax(q k / 8) v per head over each of the n
 * segments' own rows; seg_len (n) HOST int32, the segments packed tightly in their order; n <= 64. */
int vx_op_enc16_gemm(int32_t epi, const void* A_bf16, const void* W_bf16, const float* bias, const float* res, void* out, int64_t M,
                     int32_t N, int32_t K, void* stream);
int vx_op_enc16_add_ln(const float* a, const float* b, int32_t bmod, const float* w, const float* beta, float* sum, void* y_bf16,
                       int64_t M, int32_t d, float eps, void* stream);
int vx_op_enc16_attn(const void* qkv_bf16, void* out_bf16, int32_t n, const int32_t* seg_len, int32_t heads, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VALLEX_H */
