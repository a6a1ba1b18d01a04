// The kernels of vx_align (the attention the AR decoder pays to the text, and the best monotonic path through it) and their
// launchers.  A translation unit of its own, like logprob.hip: no other unit sees these kernels, so the device code of every
// existing path is compiled exactly as before.  vx_align's two are plain VALU kernels, one utterance per call; vx_align_batch's run
// on the matrix pipe over a concatenation of utterances.
#include <hip/hip_runtime.h>

#include <algorithm>
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

// ---- the batched tap -------------------------------------------------------------------------------------------------------
typedef __bf16 al_bf16x8 __attribute__((ext_vector_type(8)));
typedef float al_f32x16 __attribute__((ext_vector_type(16)));

// The other half of the wave: lane l <-> lane l ^ 32 (the two lanes that share a query row of a 32x32 MFMA tile).
__device__ __forceinline__ float al_xor32(float v) { return __shfl_xor(v, 32, WAVE); }

// Workgroup = (64-row tile of one segment's tapped rows, head, segment), two waves of 32 query rows: the grid is
// ceil(T / 64) x H x n workgroups, so one utterance of 753 frames and 16 heads already gives 192.  The orientation and the K
// staging of mfma_attn_kernel / cross_attn_seg_kernel without V: S^T = K . Q^T by v_mfma_f32_32x32x16_bf16, a lane holds query
// (lane & 31) and, in register v, key (v & 3) + 8 (v >> 2) + 4 (lane >> 5) of a 32-key sub-tile; 64-key K tiles double-buffered
// in LDS, rows swizzled as there; q scaled by 2^-3 in bf16 (exact).  Pass 1: running max / sum per lane over the keys [0, limit)
// of its row, tiles ascending, the two half-waves merged at the end.  Pass 2: the text tiles again - the same instructions on the
// same operands, so the same scores - and p = exp(s - max) / sum goes, un-weighted, to this head's own cells of the scratch; the
// row's text mass likewise.  attn_text_heads_kernel then adds the heads in head order: no atomics, and a row's arithmetic depends
// on its own segment only.  Key rows are clamped to the last key any row of the tile may see, masked scores are replaced by -inf
// by a select: keys past a row's limit, pad rows and V are never read.
__global__ __launch_bounds__(128) void attn_text_seg_kernel(const bf16* __restrict__ q_, const bf16* __restrict__ k_, long long ld,
                                                            const AlignSeg* __restrict__ segs, const float* __restrict__ head_w,
                                                            float* __restrict__ scr, long long cells, long long rows_total) {
  constexpr int HD = 64, NW = ALIGN_SEG_ROWS / 32, NT = NW * 64, CPT = 512 / NT;  // CPT: 16-byte chunks of a K tile per thread
  const AlignSeg sg = segs[blockIdx.z];
  const int head = blockIdx.y, t0 = blockIdx.x * ALIGN_SEG_ROWS;
  if (t0 >= sg.rows || head_w[head] == 0.f) return;  // uniform
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[2 * 8192];  // [buf][64 keys * 128 B]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int row = t0 + wave * 32 + r;
  const bool qvalid = row < sg.rows;
  const int Sw = sg.c1 - sg.c0;
  const int limit = qvalid ? sg.text_len + sg.row0 + row + 1 : 0;                      // keys [0, limit) of this row
  const int blk_limit = sg.text_len + sg.row0 + min(sg.rows, t0 + ALIGN_SEG_ROWS);    // ... of the tile's last row
  const bf16* __restrict__ const kbase = k_ + (size_t)sg.start * ld + head * HD;

  al_bf16x8 qf[4];
  {
    const bf16* qp = q_ + (size_t)(sg.start + sg.qfirst + min(row, sg.rows - 1)) * ld + head * HD + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[ks] = *reinterpret_cast<const al_bf16x8*>(qp + ks * 16);
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[ks][j] = (bf16)((float)qf[ks][j] * 0.125f);
    }
  }

  uint4 kreg[CPT];
  auto gload = [&](int kt, int nk) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int c = tid + i * NT, kr = c >> 3, ch = c & 7;
      kreg[i] = ld16(kbase + (size_t)min(kt + kr, nk - 1) * ld + ch * 8);
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int c = tid + i * NT, kr = c >> 3, ch = c & 7;
      *reinterpret_cast<uint4*>(lds_raw + buf * 8192 + kr * 128 + ((ch ^ ((kr >> 1) & 7)) << 4)) = kreg[i];
    }
  };
  // the keys [0, nk) in 64-key tiles: body(kt, the tile's scores)
  auto sweep = [&](int nk, auto&& body) {
    const int ntiles = (nk + 63) / 64;
    gload(0, nk);
    lstore(0);
    __syncthreads();
    for (int it = 0; it < ntiles; ++it) {
      const int cur = it & 1, kt = it * 64;
      if (it + 1 < ntiles) gload(kt + 64, nk);
      const unsigned char* kb = lds_raw + cur * 8192;
      const int swz = (r >> 1) & 7;
      al_f32x16 accS[2];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int v = 0; v < 16; ++v) accS[sub][v] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const al_bf16x8 kf = *reinterpret_cast<const al_bf16x8*>(kb + (sub * 32 + r) * 128 + (((ks * 2 + hh) ^ swz) << 4));
          accS[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], accS[sub], 0, 0, 0);
        }
      }
      body(kt, accS);
      if (it + 1 < ntiles) lstore(cur ^ 1);  // the other buffer: its readers passed the barrier that ended iteration it - 1
      __syncthreads();
    }
  };

  float m_run = -INFINITY, l_run = 0.f;  // l_run: this half-wave's share of the row sum
  sweep(blk_limit, [&](int kt, al_f32x16 (&accS)[2]) {
    float mloc = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int kg = kt + sub * 32 + (v & 3) + 8 * (v >> 2) + 4 * hh;
        accS[sub][v] = (kg < limit) ? accS[sub][v] : -INFINITY;
        mloc = fmaxf(mloc, accS[sub][v]);
      }
    mloc = fmaxf(mloc, al_xor32(mloc));
    const float m_new = fmaxf(m_run, mloc);
    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;  // a row past the segment sees nothing: exp(-inf - 0) = 0
    l_run *= (m_run == -INFINITY) ? 0.f : expf(m_run - m_use);
    m_run = m_new;
    float l0 = 0.f, l1 = 0.f;  // two chains, fixed order
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int v = 0; v < 16; v += 2) {
        l0 += expf(accS[sub][v] - m_use);
        l1 += expf(accS[sub][v + 1] - m_use);
      }
    l_run += l0 + l1;
  });
  const float l = l_run + al_xor32(l_run);  // commutative: both halves get the same bits

  float* cellp = scr + (size_t)head * cells + sg.cell_off + (long long)row * Sw - sg.c0;
  float pm = 0.f;
  sweep(sg.text_len, [&](int kt, al_f32x16 (&accS)[2]) {
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int kg = kt + sub * 32 + (v & 3) + 8 * (v >> 2) + 4 * hh;
        if (qvalid && kg < sg.text_len) {
          const float p = expf(accS[sub][v] - m_run) / l;
          pm += p;
          if (kg >= sg.c0 && kg < sg.c1) cellp[kg] = p;
        }
      }
  });
  pm += al_xor32(pm);
  if (qvalid && hh == 0) scr[(size_t)gridDim.y * cells + (size_t)head * rows_total + sg.row_off + row] = pm;
}

// The second pass of the batched tap: cell i of segment blockIdx.y (its T_z (c1 - c0) cells, then its T_z row masses) =
// sum_h w[h] x (head h's cell), heads ascending, zero-weight heads left out (their scratch was never written).  first: store;
// else one fp32 addition onto what is there.
__global__ __launch_bounds__(256) void attn_text_heads_kernel(const AlignSeg* __restrict__ segs, int nhead, const float* __restrict__ head_w,
                                                              const float* __restrict__ scr, long long cells, long long rows_total,
                                                              float* __restrict__ attn, float* __restrict__ mass, int first) {
  const AlignSeg sg = segs[blockIdx.y];
  const long long nc = (long long)sg.rows * (sg.c1 - sg.c0), n = nc + (mass != nullptr ? sg.rows : 0);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const bool cell = i < nc;
    const float* src = cell ? scr + sg.cell_off + i : scr + (size_t)nhead * cells + sg.row_off + (i - nc);
    const long long hs = cell ? cells : rows_total;
    float acc = 0.f;
    for (int h = 0; h < nhead; ++h) {
      const float w = head_w[h];
      if (w != 0.f) acc = fmaf(w, src[(size_t)h * hs], acc);
    }
    float* o = cell ? attn + sg.cell_off + i : mass + sg.row_off + (i - nc);
    *o = first ? acc : __fadd_rn(*o, acc);
  }
}

// mono_path_kernel, one workgroup per map: the same programme on the map blockIdx.x describes.
__global__ __launch_bounds__(256) void mono_path_seg_kernel(const float* __restrict__ a_, const AlignSeg* __restrict__ segs,
                                                            unsigned char* __restrict__ bp_, int* __restrict__ path_,
                                                            double* __restrict__ score_) {
  extern __shared__ __attribute__((aligned(16))) double mono_rows[];
  const AlignSeg sg = segs[blockIdx.x];
  const int tid = threadIdx.x, T = sg.rows, Sw = sg.c1 - sg.c0;
  const float* a = a_ + sg.cell_off;
  unsigned char* bp = bp_ + sg.cell_off;
  int* path = path_ + sg.row_off;
  double* score = score_ + blockIdx.x;
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

void launch_attn_text_segs(const void* q, const void* k, long long ld, const AlignSeg* segs, int nseg, int max_rows, int nhead,
                           const float* head_w, float* scr, long long cells, long long rows_total, float* attn, float* mass, int first,
                           hipStream_t s) {
  const dim3 grid((max_rows + ALIGN_SEG_ROWS - 1) / ALIGN_SEG_ROWS, nhead, nseg);
  attn_text_seg_kernel<<<grid, ALIGN_SEG_ROWS * 2, 0, s>>>((const bf16*)q, (const bf16*)k, ld, segs, head_w, scr, cells, rows_total);
  // one workgroup per 1024 cells of the largest segment the launch can hold, at most 256 per segment (the loop strides)
  const long long per = (cells + rows_total + 1023) / 1024;
  attn_text_heads_kernel<<<dim3((unsigned)std::min<long long>(std::max<long long>(per, 1), 256), nseg), 256, 0, s>>>(
      segs, nhead, head_w, scr, cells, rows_total, attn, mass, first);
}

void launch_mono_path_segs(const float* a, const AlignSeg* segs, int n, int max_sw, unsigned char* bp, int* path, double* score,
                           hipStream_t s) {
  mono_path_seg_kernel<<<n, 256, (size_t)2 * max_sw * sizeof(double), s>>>(a, segs, bp, path, score);
}

}  // namespace vx
