// CTC forced alignment and text likelihood on given logits (include/vallex.h, vx_falign / vx_falign_asr): the forward algorithm
// and the Viterbi path through the lattice (frames x 2 L + 1 states) of a known text, one workgroup per utterance, a ragged batch
// in one launch.  No atomics: every utterance is computed by its own workgroup in a fixed order, so it is bitwise what it is alone.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace vx {

constexpr int FAL_WG = 512;      // threads of the lattice kernel
constexpr int FAL_NS = 4;        // states per thread: s = tid + k FAL_WG
constexpr int FAL_MAX_L = 1000;  // target tokens per utterance: four fp64 rows of 2 L + 3 cells are 64096 bytes of LDS
static_assert(2 * FAL_MAX_L + 1 <= FAL_WG * FAL_NS, "every state has a thread");
static_assert(4 * (2 * FAL_MAX_L + 3) * 8 + 1024 <= 65536, "the rows fit 64 KiB of LDS next to the static arrays");

struct FalUtt {
  long long bp_off;  // words: the utterance's back-pointers, [ceil(T / 16)][S]
  int row0, T;       // its first row of the logits, its frames
  int tok0, L;       // its first target, its targets
  int feasible, pad;
};

// lse[row] = m + log sum_c exp(x[c] - m) in fp64, m = max_c x[c].  One wave per frame, four frames per workgroup.
static __global__ __launch_bounds__(256) void falign_lse_kernel(const float* __restrict__ logits, int vocab, long M, double* __restrict__ lse) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* x = logits + row * vocab;
  float best = -INFINITY;
  for (int c = lane; c < vocab; c += 64) best = fmaxf(best, x[c]);
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) best = fmaxf(best, __shfl_xor(best, w));
  double se = 0.0;
  for (int c = lane; c < vocab; c += 64) se += exp((double)x[c] - (double)best);
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) se += __shfl_xor(se, w);
  if (lane == 0) lse[row] = (double)best + log(se);
}

__device__ __forceinline__ double fal_lse3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

struct FalArgs {
  const float* logits;   // [rows][vocab]
  const double* lse;     // [rows]
  const FalUtt* utt;     // [n]
  const int* targets;    // concatenated
  unsigned* bp;          // back-pointers, 2 bits per cell: bits 2 (t & 15) of word [t >> 4][s]
  int* path;             // [rows]: the state of every frame on the best path
  double* nll;           // nullable: skips the sum
  double* path_logprob;  // the rest nullable; all null skips the max
  int* frame_token;
  int* tok_start;
  int* tok_end;
  float* tok_score;
  int* feasible;
  int vocab, blank, row_stride;  // row_stride: cells of one LDS row (2 pad cells + the call's longest S)
  int do_max;
};

// Dynamic LDS: four fp64 rows of row_stride cells: a (sum) and v (max), double-buffered; cells 0 and 1 of every row stay -inf, so
// state s sits at cell s + 2 and its predecessors s - 1, s - 2 are read without a test.
static __global__ __launch_bounds__(FAL_WG) void falign_kernel(const FalArgs A) {
  extern __shared__ __attribute__((aligned(16))) double fal_rows[];
  __shared__ double red[FAL_WG / 64];
  const FalUtt U = A.utt[blockIdx.x];
  const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int T = U.T, L = U.L, S = 2 * L + 1, V = A.vocab;
  const int* y = A.targets + U.tok0;
  const bool do_sum = A.nll != nullptr, do_max = A.do_max != 0;
  if (tid == 0 && A.feasible) A.feasible[u] = U.feasible;
  if (!U.feasible || T == 0) {  // nothing to walk: T = 0 with L = 0 is the empty path of probability 1
    const bool ok = U.feasible != 0;
    if (tid == 0) {
      if (A.nll) A.nll[u] = ok ? 0.0 : (double)INFINITY;
      if (A.path_logprob) A.path_logprob[u] = ok ? 0.0 : -(double)INFINITY;
    }
    for (int t = tid; t < T; t += FAL_WG)
      if (A.frame_token) A.frame_token[U.row0 + t] = -1;
    for (int k = tid; k < L; k += FAL_WG) {
      if (A.tok_start) A.tok_start[U.tok0 + k] = -1;
      if (A.tok_end) A.tok_end[U.tok0 + k] = -1;
      if (A.tok_score) A.tok_score[U.tok0 + k] = -INFINITY;
    }
    return;
  }
  const float* X = A.logits + (long)U.row0 * V;
  const double* lse = A.lse + U.row0;
  const int RS = A.row_stride;
  double* a0 = fal_rows;
  double* a1 = fal_rows + RS;
  double* v0 = fal_rows + 2 * RS;
  double* v1 = fal_rows + 3 * RS;
  for (int i = tid; i < 4 * RS; i += FAL_WG) fal_rows[i] = -INFINITY;

  // sum_t lse[t] in a fixed order: per thread over t = tid, tid + FAL_WG, .., a butterfly over the wave, then the waves in order
  double part = 0.0;
  for (int t = tid; t < T; t += FAL_WG) part += lse[t];
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) part += __shfl_xor(part, w);
  if (lane == 0) red[tid >> 6] = part;

  int zs[FAL_NS];
  bool skip[FAL_NS];
  float xe[FAL_NS];
  unsigned acc[FAL_NS];
#pragma unroll
  for (int k = 0; k < FAL_NS; ++k) {
    const int s = tid + k * FAL_WG;
    zs[k] = A.blank;
    skip[k] = false;
    acc[k] = 0u;
    if (s < S && (s & 1)) {
      zs[k] = y[s >> 1];
      skip[k] = s >= 3 && y[(s >> 1) - 1] != zs[k];
    }
    xe[k] = s < S ? X[zs[k]] : 0.f;
  }
  __syncthreads();
  double lse_sum = 0.0;
#pragma unroll
  for (int w = 0; w < FAL_WG / 64; ++w) lse_sum += red[w];

  double lse_t = lse[0];
  for (int t = 0; t < T; ++t) {
    // the next frame's emissions leave for the registers before this frame's cells are computed
    float nx[FAL_NS];
    double lse_n = 0.0;
    if (t + 1 < T) {
      const float* xn = X + (long)(t + 1) * V;
#pragma unroll
      for (int k = 0; k < FAL_NS; ++k) nx[k] = tid + k * FAL_WG < S ? xn[zs[k]] : 0.f;
      lse_n = lse[t + 1];
    } else {
#pragma unroll
      for (int k = 0; k < FAL_NS; ++k) nx[k] = 0.f;
    }
    const int lo = S - 2 * (T - t) > 0 ? S - 2 * (T - t) : 0;  // the reachable band, both ends inclusive
    const int hi = 2 * t + 1 < S - 1 ? 2 * t + 1 : S - 1;
    const bool flush = (t & 15) == 15 || t == T - 1;
#pragma unroll
    for (int k = 0; k < FAL_NS; ++k) {
      const int s = tid + k * FAL_WG;
      if (s < S) {
        const bool in = s >= lo && s <= hi;
        const double x = (double)xe[k];
        if (do_sum) {
          double r = -INFINITY;
          if (in) {
            if (t == 0) r = x - lse_t;
            else r = (x - lse_t) + fal_lse3(a0[s + 2], a0[s + 1], skip[k] ? a0[s] : -(double)INFINITY);
          }
          a1[s + 2] = r;
        }
        if (do_max) {
          double r = -INFINITY;
          if (in) {
            if (t == 0) {
              r = x;
            } else {
              double best = v0[s + 2];
              unsigned mv = 0u;
              const double p1 = v0[s + 1];
              if (p1 > best) { best = p1; mv = 1u; }
              if (skip[k]) {
                const double p2 = v0[s];
                if (p2 > best) { best = p2; mv = 2u; }
              }
              r = best + x;
              acc[k] |= mv << (2 * (t & 15));
            }
          }
          v1[s + 2] = r;
          if (flush) {
            A.bp[U.bp_off + (long long)(t >> 4) * S + s] = acc[k];
            acc[k] = 0u;
          }
        }
      }
    }
    __syncthreads();  // frame t is complete and its readers of frame t - 1 are done: t + 1 overwrites that row
    double* q = a0; a0 = a1; a1 = q;
    q = v0; v0 = v1; v1 = q;
#pragma unroll
    for (int k = 0; k < FAL_NS; ++k) xe[k] = nx[k];
    lse_t = lse_n;
  }
  // a0 / v0 hold frame T - 1
  if (tid == 0 && do_sum) {
    const double e1 = a0[S - 1 + 2], e2 = S >= 2 ? a0[S - 2 + 2] : -(double)INFINITY;
    A.nll[u] = -fal_lse3(e1, e2, -(double)INFINITY);
  }
  if (!do_max) return;
  __threadfence_block();
  __syncthreads();  // the back-pointer words of every thread are visible to wave 0
  if (tid < 64) {
    int cur = S - 1;
    double vend = v0[S - 1 + 2];
    if (S >= 2 && v0[S - 2 + 2] > vend) { vend = v0[S - 2 + 2]; cur = S - 2; }
    if (tid == 0 && A.path_logprob) A.path_logprob[u] = vend - lse_sum;
    // 16 frames per round: a path descends by at most 2 states a frame, so the round's words are those of states cur - 31 .. cur
    for (int tb = (T - 1) >> 4; tb >= 0; --tb) {
      const int s0 = cur;
      unsigned w = 0u;
      if (lane < 32 && s0 - lane >= 0) w = A.bp[U.bp_off + (long long)tb * S + (s0 - lane)];
      const int thi = tb * 16 + 15 < T - 1 ? tb * 16 + 15 : T - 1;
      int mine = 0;
      for (int t = thi; t >= tb * 16; --t) {
        if (lane == (t & 15)) mine = cur;
        const unsigned word = __shfl(w, s0 - cur);
        cur -= (int)((word >> (2 * (t & 15))) & 3u);  // frame 0 has no move: its bits are 0
      }
      if (lane < 16 && tb * 16 + lane < T) A.path[U.row0 + tb * 16 + lane] = mine;
    }
  }
  __threadfence_block();
  __syncthreads();  // the path is visible to every thread
  const int* path = A.path + U.row0;
  for (int t = tid; t < T; t += FAL_WG) {
    const int s = path[t];
    if (A.frame_token) A.frame_token[U.row0 + t] = (s & 1) ? s >> 1 : -1;
    if ((s & 1) && (t == 0 || path[t - 1] != s)) {  // the first frame of token k: its span and its score, in frame order
      const int k = s >> 1, id = y[k];
      double sum = 0.0;
      int e = t;
      for (; e < T && path[e] == s; ++e) sum += (double)X[(long)e * V + id] - lse[e];
      if (A.tok_start) A.tok_start[U.tok0 + k] = t;
      if (A.tok_end) A.tok_end[U.tok0 + k] = e;
      if (A.tok_score) A.tok_score[U.tok0 + k] = (float)(sum / (double)(e - t));
    }
  }
}

}  // namespace vx
