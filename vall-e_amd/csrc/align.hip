// The kernels of vx_align (the attention the AR decoder pays to the text, and the best monotonic path through it) and their
// launchers.  A translation unit of its own, like logprob.hip: no other unit sees these kernels, so the device code of every
// existing path is compiled exactly as before.  Plain VALU kernels: the pass runs once per utterance.
#include <hip/hip_runtime.h>

#include <cfloat>

#undef VX_STAMPS  // the in-kernel stamps write device globals of engine.hip's unit, out of this unit's reach
#include "align.hpp"

namespace vx {

template <int HD>
__device__ __forceinline__ float align_score(const float (&q)[HD], const float* krow, float scale) {
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < HD; c += 4) {
    const float4 kv = *reinterpret_cast<const float4*>(krow + c);
    dot = fmaf(q[c], kv.x, dot); dot = fmaf(q[c + 1], kv.y, dot);
    dot = fmaf(q[c + 2], kv.z, dot); dot = fmaf(q[c + 3], kv.w, dot);
  }
  return dot * scale;
}

// Workgroup = ALIGN_TILE_ROWS query rows, 8 threads per row, and walks the heads itself.  Thread s of a row owns the keys
// j = s (mod 8) of every 64-key LDS tile - for every head, so the cell (row, column) of the LDS accumulator belongs to one thread
// and needs no synchronisation.  Per head: pass 1 walks every key the row may see with an online max / sum per thread, merged
// over the row's 8 lanes in a fixed order; pass 2 walks the text keys again, recomputes their scores by the same instructions
// (same bits) and adds w[h] * exp(s - max) / sum.  A row's arithmetic depends on its own keys only, never on where the row sits in
// the launch.  blockIdx.y: chunks of ALIGN_COL_CHUNK columns of the window (each recomputes pass 1; one chunk up to 256 tokens).
template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_text_rows_kernel(const T* __restrict__ q_, long long ldq, const T* __restrict__ k_,
                                                             long long ldk, long long khs, int rows, int row0, int nhead,
                                                             int text_len, int causal, int c0, int c1,
                                                             const float* __restrict__ head_w, float* __restrict__ attn,
                                                             float* __restrict__ mass, float* __restrict__ per_head, int first,
                                                             float scale) {
  constexpr int TR = ALIGN_TILE_ROWS, LD = HD + 4, AL = ALIGN_COL_CHUNK + 8;  // + 8: the 8 rows of a wave on different banks
  __shared__ __attribute__((aligned(16))) float Ks[64][LD];
  __shared__ float acc[TR][AL];
  const int tid = threadIdx.x, qi = tid >> 3, s = tid & 7;
  const int q0 = blockIdx.x * TR, row = q0 + qi;
  const bool qvalid = row < rows;
  const int Sw = c1 - c0;
  const int cc0 = c0 + blockIdx.y * ALIGN_COL_CHUNK, cc1 = min(c1, cc0 + ALIGN_COL_CHUNK);
  const int limit = !qvalid ? 0 : (causal ? text_len + row0 + row + 1 : text_len);             // keys [0, limit) of this row
  const int blk_limit = causal ? text_len + row0 + min(rows, q0 + TR) : text_len;              // ... of the tile's last row
  for (int i = tid; i < TR * AL; i += 256) (&acc[0][0])[i] = 0.f;
  __syncthreads();
  constexpr int CPT = HD / 4;  // channels each of a key row's 4 loader threads copies
  const int lr = tid >> 2, lc = (tid & 3) * CPT;
  float macc = 0.f;
  for (int h = 0; h < nhead; ++h) {
    const float w = head_w[h];
    if (w == 0.f && per_head == nullptr) continue;  // uniform
    float q[HD];
#pragma unroll
    for (int c = 0; c < HD; ++c) q[c] = qvalid ? to_f32(q_[(size_t)row * ldq + h * HD + c]) : 0.f;
    const T* kh = k_ + (size_t)h * khs;
    auto load_tile = [&](int kt, int nk) {
      __syncthreads();
      const int kr = kt + lr;
#pragma unroll
      for (int j = 0; j < CPT; ++j) Ks[lr][lc + j] = (kr < nk) ? to_f32(kh[(size_t)kr * ldk + lc + j]) : 0.f;
      __syncthreads();
    };
    float m = -INFINITY, l = 0.f;
    for (int kt = 0; kt < blk_limit; kt += 64) {
      load_tile(kt, blk_limit);
#pragma unroll 4
      for (int kk = 0; kk < 8; ++kk) {
        const int kl = kk * 8 + s;
        const float sc = align_score<HD>(q, &Ks[kl][0], scale);
        if (kt + kl < limit) {
          const float mn = fmaxf(m, sc);
          l = l * expf(m - mn) + expf(sc - mn);  // exp(-inf) = 0 at the first key
          m = mn;
        }
      }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {  // the 8 threads of a row (adjacent lanes)
      const float m2 = __shfl_xor(m, off, WAVE), l2 = __shfl_xor(l, off, WAVE);
      const float mn = fmaxf(m, m2);
      const float e1 = (m == -INFINITY) ? 0.f : expf(m - mn), e2 = (m2 == -INFINITY) ? 0.f : expf(m2 - mn);
      l = __fmul_rn(l, e1) + __fmul_rn(l2, e2);  // two rounded products (no fma): both lanes of a pair get the same bits
      m = mn;
    }
    float pm = 0.f;
    for (int kt = 0; kt < text_len; kt += 64) {
      load_tile(kt, text_len);
#pragma unroll 4
      for (int kk = 0; kk < 8; ++kk) {
        const int kl = kk * 8 + s, kg = kt + kl;
        const float sc = align_score<HD>(q, &Ks[kl][0], scale);
        if (qvalid && kg < text_len) {
          const float p = expf(sc - m) / l;
          pm += p;
          if (kg >= cc0 && kg < cc1) {
            acc[qi][kg - cc0] += w * p;
            if (per_head != nullptr) per_head[((size_t)h * rows + row) * Sw + (kg - c0)] = p;
          }
        }
      }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) pm += __shfl_xor(pm, off, WAVE);
    macc += w * pm;
  }
  if (!qvalid) return;
  for (int c = cc0 + ((s - cc0) & 7); c < cc1; c += 8) {  // this thread's columns: c = s (mod 8)
    float* o = attn + (size_t)row * Sw + (c - c0);
    *o = first ? acc[qi][c - cc0] : *o + acc[qi][c - cc0];
  }
  if (mass != nullptr && blockIdx.y == 0 && s == 0) mass[row] = first ? macc : mass[row] + macc;
}

// One workgroup; lanes over the columns j, looping where Sw exceeds the workgroup; one barrier per frame (the two fp64 rows of
// the programme alternate in LDS); one byte of back-pointer per cell; thread 0 walks the path back.
__global__ __launch_bounds__(256) void mono_path_kernel(const float* __restrict__ a, int T, int Sw, unsigned char* __restrict__ bp,
                                                        int* __restrict__ path, double* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) double mono_rows[];
  const int tid = threadIdx.x;
  if (T < Sw) {  // no monotonic path visits every column
    for (int t = tid; t < T; t += 256) path[t] = -1;
    if (tid == 0) *score = -INFINITY;
    return;
  }
  double *prev = mono_rows, *cur = mono_rows + Sw;
  for (int j = tid; j < Sw; j += 256) prev[j] = j == 0 ? log((double)fmaxf(a[0], FLT_MIN)) : -INFINITY;
  __syncthreads();
  for (int t = 1; t < T; ++t) {
    for (int j = tid; j < Sw; j += 256) {
      const double stay = prev[j], adv = j > 0 ? prev[j - 1] : -INFINITY;
      const bool mv = adv > stay;  // equal predecessors: the path stays in its column
      cur[j] = (mv ? adv : stay) + log((double)fmaxf(a[(size_t)t * Sw + j], FLT_MIN));
      bp[(size_t)t * Sw + j] = mv ? 1 : 0;
    }
    __syncthreads();
    double* x = prev; prev = cur; cur = x;
  }
  if (tid == 0) {
    *score = prev[Sw - 1];
    int j = Sw - 1;
    for (int t = T - 1; t > 0; --t) {
      path[t] = j;
      j -= bp[(size_t)t * Sw + j];
    }
    path[0] = j;
  }
}

int launch_attn_text_rows(bool bf, const void* q, long long ldq, const void* k, long long ldk, long long k_head_stride, int rows,
                          int row0, int nhead, int hd, int text_len, int causal, int c0, int c1, const float* head_w, float* attn,
                          float* mass, float* per_head, int first, hipStream_t s) {
  const dim3 grid((rows + ALIGN_TILE_ROWS - 1) / ALIGN_TILE_ROWS, (c1 - c0 + ALIGN_COL_CHUNK - 1) / ALIGN_COL_CHUNK);
  const float scale = 1.0f / sqrtf((float)hd);
#define AT(HDV)                                                                                                                  \
  if (hd == HDV) {                                                                                                               \
    if (bf) attn_text_rows_kernel<bf16, HDV><<<grid, 256, 0, s>>>((const bf16*)q, ldq, (const bf16*)k, ldk, k_head_stride, rows, \
                                                                  row0, nhead, text_len, causal, c0, c1, head_w, attn, mass,    \
                                                                  per_head, first, scale);                                      \
    else attn_text_rows_kernel<float, HDV><<<grid, 256, 0, s>>>((const float*)q, ldq, (const float*)k, ldk, k_head_stride, rows, \
                                                                row0, nhead, text_len, causal, c0, c1, head_w, attn, mass,      \
                                                                per_head, first, scale);                                        \
    return 0;                                                                                                                    \
  }
  AT(64) AT(32) AT(16) AT(8) AT(4)
#undef AT
  return -1;
}

void launch_mono_path(const float* a, int T, int Sw, unsigned char* bp, int* path, double* score, hipStream_t s) {
  mono_path_kernel<<<1, 256, (size_t)2 * Sw * sizeof(double), s>>>(a, T, Sw, bp, path, score);
}

}  // namespace vx
