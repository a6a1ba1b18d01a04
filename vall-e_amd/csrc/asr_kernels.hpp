// CTC speech recogniser kernels (Wav2Vec2ForCTC / HubertForCTC, 16 kHz waveform -> token ids) and the edit distance behind WER / CER.
// The definition is in include/vallex.h (vx_asr_*, vx_ctc_greedy, vx_edit_distance); the host side is asr.hip.  The row GEMM, the
// GroupNorm layer 0, the attention and the post-norm LayerNorm are spk_kernels.hpp's, used as they are; the layout (time-major rows,
// one segment table per stage, nothing crosses an utterance) is theirs too.
//
//   asr_conv0_ln        layer 0 of the "layer" feature encoder: Conv1d(1 -> C, k, stride), LayerNorm over the C channels of each
//                       frame, exact GELU, in one pass (the statistic is per frame).  A workgroup owns ASR_C0_TT frames of ONE
//                       utterance, stages their samples and the transposed weights [k][C] in LDS; a wave owns a frame at a time,
//                       a lane the channels lane, lane + 64, ..., kept in registers between the two statistics and the store.
//   asr_ln_gelu_rows    conv layers 1 .. of the "layer" flavour: the GEMM runs at SPK_ACT_NONE and this normalises its rows in
//                       place, y = gelu(LayerNorm(x)); one wave per row.
//   asr_add_layernorm   the stable (pre-norm) encoder's residual folded into the LayerNorm that follows it: s = a + b is stored as
//                       the new residual stream and y = LayerNorm(s) next to it: one pass over the rows instead of two.
//   ctc_frame_kernel    one wave per frame: the argmax (lowest index on ties) and its log-probability, x_max - logsumexp(x), the sum
//                       of exp(x - x_max) taken in fp64 (lane-strided partial sums, a fixed butterfly).
//   ctc_collapse_kernel one workgroup per utterance: frame t is kept when id[t] != blank and (t == 0 or id[t] != id[t - 1]), i.e.
//                       repeats are merged first and blanks removed second; the kept ids and their frame indices are compacted in
//                       frame order by a ballot / prefix scan, no atomics; the mean log-probability over ALL frames in fp64.
//   edit_distance_kernel  one workgroup per pair: Levenshtein distance with unit costs over anti-diagonals, three diagonals in LDS
//                       (as dtw_warp_kernel), in integers.  A cell is one 64-bit word, cost << 48 | S << 32 | D << 16 | I, so taking
//                       a step is one addition.  The predecessor is the diagonal one unless the deletion is strictly cheaper, then
//                       that unless the insertion is strictly cheaper still: S / D / I equal a backtrace with the same preference.
#pragma once
#include "spk_kernels.hpp"

namespace vx {

constexpr int ASR_C0_TT = 64;        // frames per workgroup of asr_conv0_ln
constexpr int ASR_C0_MAXC = 1024;    // channels of layer 0 served by asr_conv0_ln (16 per lane)
constexpr int ASR_C0_LDS = 60 * 1024;  // bytes: the tile's samples + the weights [k][C]
constexpr int EDIT_MAX_LEN = 2048;   // tokens per side of a pair (20 s of audio are 999 frames); 3 x 2049 x 8 bytes of LDS
constexpr int EDIT_WG = 256;
constexpr int CTC_WG = 256;

// ---- layer 0, "layer" flavour ---------------------------------------------------------------------------------------------------
struct AsrConv0Args {
  const float* const* wav;  // per utterance
  const float* nstats;      // [2 nseg] mean, rstd of the input normalisation, or null
  const float* wt;          // [k][C]: the convolution weight transposed
  const float* bias;        // [C] or null
  const float* ln_w;        // [C]
  const float* ln_b;        // [C]
  float* out;               // rows [T0 total][C]
  const int* seg;           // layer-0 output rows
  int nseg, C, k, stride;
  float eps;
};

// grid.x = the tiles of the call (ceil(len / ASR_C0_TT) per segment); 256 threads.  Dynamic LDS: ((TT - 1) stride + k) + k C floats.
static __global__ __launch_bounds__(256) void asr_conv0_ln(const AsrConv0Args a) {
  constexpr int TT = ASR_C0_TT, NI = ASR_C0_MAXC / 64;
  extern __shared__ float asr_c0_lds[];
  long lo, len, t0;
  const int s = spk_find_tile(a.seg, a.nseg, TT, blockIdx.x, lo, len, t0);
  if (s == a.nseg) return;  // uniform over the workgroup
  const int tt = len - t0 < TT ? (int)(len - t0) : TT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nsmax = (TT - 1) * a.stride + a.k;
  float* X = asr_c0_lds;
  float* Wt = asr_c0_lds + nsmax;
  const float* x = a.wav[s] + t0 * a.stride;
  const int ns = (tt - 1) * a.stride + a.k;  // inside the utterance by the definition of its frame count
  const float nm = a.nstats ? a.nstats[2 * s] : 0.f, nr = a.nstats ? a.nstats[2 * s + 1] : 1.f;
  for (int i = tid; i < ns; i += 256) X[i] = a.nstats ? (x[i] - nm) * nr : x[i];
  for (int i = tid; i < a.k * a.C; i += 256) Wt[i] = a.wt[i];
  __syncthreads();
  const float invC = 1.f / (float)a.C;
  for (int t = wave; t < tt; t += 4) {
    const float* xp = X + t * a.stride;
    float v[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int c = lane + 64 * i;
      v[i] = 0.f;
      if (c < a.C) {
        float acc = a.bias ? a.bias[c] : 0.f;
        for (int j = 0; j < a.k; ++j) acc = fmaf(xp[j], Wt[j * a.C + c], acc);
        v[i] = acc;
      }
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) sum += v[i];  // channels past C hold 0
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) sum += __shfl_xor(sum, w);
    const float mean = sum * invC;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const float dv = v[i] - mean;
      if (lane + 64 * i < a.C) q = fmaf(dv, dv, q);
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) q += __shfl_xor(q, w);
    const float rstd = 1.f / sqrtf(q * invC + a.eps);
    float* o = a.out + (lo + t0 + t) * a.C;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int c = lane + 64 * i;
      if (c < a.C) o[c] = spk_gelu((v[i] - mean) * rstd * a.ln_w[c] + a.ln_b[c]);
    }
  }
}

// ---- LayerNorm + GELU over rows, in place ---------------------------------------------------------------------------------------
// x[row] = gelu(LayerNorm(x[row])); one wave per row, the statistics as spk_layernorm takes them.  A lane rewrites only the
// elements it has read itself, after the wave's two reductions.
static __global__ __launch_bounds__(256) void asr_ln_gelu_rows(float* x, const float* __restrict__ w, const float* __restrict__ beta, long M,
                                                               int d, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  float* xp = x + row * d;
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += xp[c];
#pragma unroll
  for (int w_ = 32; w_ > 0; w_ >>= 1) s += __shfl_xor(s, w_);
  const float mean = s / d;
  float q = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float v = xp[c] - mean;
    q = fmaf(v, v, q);
  }
#pragma unroll
  for (int w_ = 32; w_ > 0; w_ >>= 1) q += __shfl_xor(q, w_);
  const float rstd = 1.f / sqrtf(q / d + eps);
  for (int c = lane; c < d; c += 64) xp[c] = spk_gelu((xp[c] - mean) * rstd * w[c] + beta[c]);
}

// ---- residual + LayerNorm -------------------------------------------------------------------------------------------------------
// s = a + b, stored to `sum` when it is not null; y = LayerNorm(s).  `sum` may be `a` (every element is read before its own lane
// rewrites it); y is neither a nor b.  One wave per row.
static __global__ __launch_bounds__(256) void asr_add_layernorm(const float* a, const float* __restrict__ b, const float* __restrict__ w,
                                                                const float* __restrict__ beta, float* sum, float* __restrict__ y, long M,
                                                                int d, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* ap = a + row * d;
  const float* bp = b + row * d;
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += ap[c] + bp[c];
#pragma unroll
  for (int w_ = 32; w_ > 0; w_ >>= 1) s += __shfl_xor(s, w_);
  const float mean = s / d;
  float q = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float v = (ap[c] + bp[c]) - mean;
    q = fmaf(v, v, q);
  }
#pragma unroll
  for (int w_ = 32; w_ > 0; w_ >>= 1) q += __shfl_xor(q, w_);
  const float rstd = 1.f / sqrtf(q / d + eps);
  for (int c = lane; c < d; c += 64) {
    const float v = ap[c] + bp[c];
    y[row * d + c] = (v - mean) * rstd * w[c] + beta[c];
    if (sum) sum[row * d + c] = v;
  }
}

// ---- greedy CTC -----------------------------------------------------------------------------------------------------------------
// Frame `row` of logits [M][vocab]: ids[row] = argmax (the lowest index among equal maxima), lp[row] = x_max - logsumexp(x) in fp64.
// One wave per frame, four frames per workgroup.
static __global__ __launch_bounds__(256) void ctc_frame_kernel(const float* __restrict__ logits, int vocab, long M, int* __restrict__ ids,
                                                               double* __restrict__ lp) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* x = logits + row * vocab;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < vocab; c += 64) {  // ascending c: a later equal value does not replace an earlier one
    const float v = x[c];
    if (v > best || bi == 0x7fffffff) { best = v; bi = c; }
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    const float ob = __shfl_xor(best, w);
    const int oi = __shfl_xor(bi, w);
    if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
  }
  double se = 0.0;
  for (int c = lane; c < vocab; c += 64) se += exp((double)x[c] - (double)best);
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) se += __shfl_xor(se, w);
  if (lane == 0) {
    ids[row] = bi;
    lp[row] = -log(se);
  }
}

// Utterance u = blockIdx.x, frames seg[u] .. seg[u + 1]: tokens / token_frames at the utterance's first row onwards, counts[u],
// mean_lp[u] (0 frames: count 0, mean 0).  frame_lp (nullable): the per-frame log-probabilities rounded to fp32.
static __global__ __launch_bounds__(CTC_WG) void ctc_collapse_kernel(const int* __restrict__ ids, const double* __restrict__ lp,
                                                                     const int* __restrict__ seg, int blank, int* __restrict__ tokens,
                                                                     int* __restrict__ token_frames, int* __restrict__ counts,
                                                                     float* __restrict__ mean_lp, float* __restrict__ frame_lp) {
  __shared__ int wtot[CTC_WG / 64];
  __shared__ double S[CTC_WG];
  const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long lo = seg[u];
  const int T = (int)((long)seg[u + 1] - lo);
  int base = 0;  // tokens kept before this chunk: the same value in every thread
  double acc = 0.0;
  for (int t0 = 0; t0 < T; t0 += CTC_WG) {
    const int t = t0 + tid;
    int id = blank;
    bool keep = false;
    if (t < T) {
      id = ids[lo + t];
      keep = id != blank && (t == 0 || id != ids[lo + t - 1]);
      const double v = lp[lo + t];
      acc += v;
      if (frame_lp) frame_lp[lo + t] = (float)v;
    }
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wave] = __popcll(m);
    __syncthreads();
    int off = base, all = 0;
#pragma unroll
    for (int w = 0; w < CTC_WG / 64; ++w) {
      if (w < wave) off += wtot[w];
      all += wtot[w];
    }
    if (keep) {
      tokens[lo + off + before] = id;
      token_frames[lo + off + before] = t;
    }
    base += all;
    __syncthreads();  // wtot is rewritten by the next chunk
  }
  S[tid] = acc;
  __syncthreads();
  for (int w = CTC_WG / 2; w > 0; w >>= 1) {
    if (tid < w) S[tid] += S[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    counts[u] = base;
    mean_lp[u] = T > 0 ? (float)(S[0] / (double)T) : 0.f;
  }
}

// ---- edit distance --------------------------------------------------------------------------------------------------------------
struct EditPair {
  int ref_off, ref_len, hyp_off, hyp_len;
};

// Pair p = blockIdx.x: out[4 p ..] = distance, substitutions, deletions, insertions turning ref into hyp.  Cell (i, j) = the first i
// reference tokens against the first j hypothesis tokens; diagonal d = i + j holds the cells indexed by i.  Dynamic LDS:
// 3 (ref_len + 1) 64-bit words, sized by the host for the longest reference of the call.
static __global__ __launch_bounds__(EDIT_WG) void edit_distance_kernel(const int* __restrict__ ref, const int* __restrict__ hyp,
                                                                       const EditPair* __restrict__ pairs, int diag_stride,
                                                                       int* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long edit_diag[];
  constexpr unsigned long long SUB = (1ull << 48) | (1ull << 32), DEL = (1ull << 48) | (1ull << 16), INS = (1ull << 48) | 1ull;
  const EditPair p = pairs[blockIdx.x];
  const int tid = threadIdx.x, R = p.ref_len, H = p.hyp_len;
  const int* r = ref + p.ref_off;
  const int* h = hyp + p.hyp_off;
  unsigned long long *cur = edit_diag, *p1 = edit_diag + diag_stride, *p2 = edit_diag + 2 * diag_stride;
  for (int d = 0; d <= R + H; ++d) {
    const int ilo = d > H ? d - H : 0, ihi = d < R ? d : R;
    for (int i = ilo + tid; i <= ihi; i += EDIT_WG) {
      const int j = d - i;
      unsigned long long best;
      if (i > 0 && j > 0) {
        best = p2[i - 1] + (r[i - 1] != h[j - 1] ? SUB : 0ull);
        const unsigned long long del = p1[i - 1] + DEL, ins = p1[i] + INS;
        if ((del >> 48) < (best >> 48)) best = del;
        if ((ins >> 48) < (best >> 48)) best = ins;
      } else if (i > 0) {
        best = p1[i - 1] + DEL;
      } else if (j > 0) {
        best = p1[i] + INS;
      } else {
        best = 0ull;
      }
      cur[i] = best;
    }
    __syncthreads();  // diagonal d is complete, and its readers of d - 2 are done: d + 1 overwrites that buffer
    unsigned long long* x = p2; p2 = p1; p1 = cur; cur = x;
  }
  if (tid == 0) {
    const unsigned long long v = p1[R];  // the last diagonal holds the one cell (R, H)
    out[4 * blockIdx.x] = (int)(v >> 48);
    out[4 * blockIdx.x + 1] = (int)((v >> 32) & 0xffff);
    out[4 * blockIdx.x + 2] = (int)((v >> 16) & 0xffff);
    out[4 * blockIdx.x + 3] = (int)(v & 0xffff);
  }
}

}  // namespace vx
