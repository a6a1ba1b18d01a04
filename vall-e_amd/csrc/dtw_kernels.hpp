// Dynamic time warping between two feature sequences (include/vallex.h, vx_dtw_*): cepstra, local cost, warp.
//
// dtw_ceps_kernel   every row m (D values) of every sequence of the call -> its n_ceps cepstra, c_k = sum_n m_n tab[n][k].  A thread
//                   owns one (row, k): the products (exact in fp64: two fp32 factors) are added in ascending n in fp64 and the sum
//                   is rounded once to fp32.  A row's cepstra depend on that row only.
// dtw_cost_kernel   grid over (pair, 64 x 64 tile of its cost matrix); 256 threads, a thread owns 4 x 4 cells (rows ty + 16 r,
//                   columns tx + 16 c).  The two row blocks go through LDS in chunks of 32 channels.  Per cell and channel the
//                   difference is formed in fp32 (identical rows: exactly 0), its square (exact in fp64) is added in ascending
//                   channel order in fp64, and sqrt of the sum is rounded once to fp32.  No atomics; a cell's bits depend on its
//                   two rows only, never on the tile, the pair's place in the launch or the batch.
// dtw_warp_kernel   one workgroup per pair, an anti-diagonal wavefront: diagonal d holds the cells (i, d - i), indexed by i; the
//                   three live diagonals (d, d - 1, d - 2) are fp64 in LDS, 3 * Ta * 8 bytes, and rotate; one barrier per
//                   diagonal.  Thread t owns the rows t, t + 256, ... and reads its cell's cost one diagonal ahead.  G(i, j) = d(i, j) + min of the existing predecessors (i-1, j-1), (i-1, j), (i, j-1); the diagonal
//                   one is kept unless another is strictly smaller, then (i-1, j) unless (i, j-1) is strictly smaller.  One byte of
//                   back-pointer per cell goes to global memory (0 diagonal, 1 from (i-1, j), 2 from (i, j-1)); thread 0 walks the
//                   path back from (Ta-1, Tb-1), filling the caller's path from its end, and the workgroup then moves it to the
//                   front.  A cell is one fp64 min chain and one addition on exact inputs: the same bits on every run and as on
//                   the host.  On the first row and column the back-trace ignores the stored byte, so whatever the costs are
//                   (NaN included) the walk stays inside the matrix and ends after at most Ta + Tb - 1 cells.
#pragma once
#include "common.hpp"

namespace vx {

constexpr int DTW_MAX_DIM = 128, DTW_MAX_FRAMES = 4096, DTW_MAX_BATCH = 64;
constexpr int DTW_TILE = 64;   // cost tile: DTW_TILE x DTW_TILE cells per workgroup
constexpr int DTW_KC = 32;     // channels per LDS chunk of the cost kernel
constexpr int DTW_WG = 256;    // threads per workgroup of every kernel here; the warp kernel walks a diagonal in chunks of DTW_WG
constexpr int DTW_NCH = DTW_MAX_FRAMES / DTW_WG;  // rows of A a thread of the warp kernel owns at most

struct DtwPair {
  const float* a;       // (Ta, D)
  const float* b;       // (Tb, D)
  int* path;            // (Ta + Tb - 1, 2), nullable
  long long cell_off;   // the pair's (Ta, Tb) cells in the cost matrix and the back-pointers
  long long ceps_off;   // the pair's (Ta + Tb, n_ceps) cepstra, A's rows first, in the cepstra buffer (floats)
  int Ta, Tb;
  int tile0;            // first cost tile of the pair in the launch
  int pad_;
};

__global__ __launch_bounds__(DTW_WG) void dtw_ceps_kernel(const DtwPair* __restrict__ pairs, const float* __restrict__ tab, int D,
                                                          int nc, float* __restrict__ ceps) {
  const DtwPair p = pairs[blockIdx.y];
  const long long items = (long long)(p.Ta + p.Tb) * nc;
  float* out = ceps + p.ceps_off;
  for (long long item = (long long)blockIdx.x * DTW_WG + threadIdx.x; item < items; item += (long long)gridDim.x * DTW_WG) {
    const int row = (int)(item / nc), k = (int)(item - (long long)row * nc);
    const float* m = row < p.Ta ? p.a + (size_t)row * D : p.b + (size_t)(row - p.Ta) * D;
    double acc = 0.0;
    for (int n = 0; n < D; ++n) acc = fma((double)m[n], (double)tab[n * nc + k], acc);
    out[item] = (float)acc;
  }
}

// K channels per row: the cepstra (K = n_ceps, rows from `ceps`) or the features as given (ceps == nullptr, K = D).
__global__ __launch_bounds__(DTW_WG) void dtw_cost_kernel(const DtwPair* __restrict__ pairs, int npairs, const float* __restrict__ ceps,
                                                          int K, float* __restrict__ cost) {
  __shared__ float As[DTW_TILE][DTW_KC + 1];
  __shared__ float Bs[DTW_TILE][DTW_KC + 1];
  const int tile = blockIdx.x, tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  int s = 0;  // the pair of the tile: the last s with tile0[s] <= tile
  for (int hi = npairs; hi - s > 1;) {
    const int mid = (s + hi) >> 1;
    if (pairs[mid].tile0 <= tile) s = mid;
    else hi = mid;
  }
  const DtwPair p = pairs[s];
  const int tj = (p.Tb + DTW_TILE - 1) / DTW_TILE, t = tile - p.tile0;
  const int i0 = (t / tj) * DTW_TILE, j0 = (t % tj) * DTW_TILE;
  const float* A = ceps ? ceps + p.ceps_off : p.a;
  const float* B = ceps ? ceps + p.ceps_off + (long long)p.Ta * K : p.b;
  double acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
  for (int k0 = 0; k0 < K; k0 += DTW_KC) {
    const int kc = min(DTW_KC, K - k0);
    __syncthreads();  // the previous chunk's reads are done
    for (int idx = tid; idx < DTW_TILE * DTW_KC; idx += DTW_WG) {
      const int r = idx >> 5, c = idx & 31;
      As[r][c] = (i0 + r < p.Ta && c < kc) ? A[(size_t)(i0 + r) * K + k0 + c] : 0.f;
      Bs[r][c] = (j0 + r < p.Tb && c < kc) ? B[(size_t)(j0 + r) * K + k0 + c] : 0.f;
    }
    __syncthreads();
    for (int c = 0; c < kc; ++c) {
      float av[4], bv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        av[r] = As[ty + 16 * r][c];
        bv[r] = Bs[tx + 16 * r][c];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double df = (double)__fsub_rn(av[r], bv[q]);
          acc[r][q] = fma(df, df, acc[r][q]);
        }
    }
  }
  float* o = cost + p.cell_off;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + ty + 16 * r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + tx + 16 * q;
      if (i < p.Ta && j < p.Tb) o[(size_t)i * p.Tb + j] = (float)sqrt(acc[r][q]);
    }
  }
}

__global__ __launch_bounds__(DTW_WG) void dtw_warp_kernel(const float* __restrict__ cost_, unsigned char* __restrict__ bp_,
                                                          const DtwPair* __restrict__ pairs, double* __restrict__ total,
                                                          int* __restrict__ path_len) {
  extern __shared__ __attribute__((aligned(16))) double dtw_diag[];
  __shared__ int s_len;
  const DtwPair p = pairs[blockIdx.x];
  const int tid = threadIdx.x, Ta = p.Ta, Tb = p.Tb, cap = Ta + Tb - 1;
  const float* cost = cost_ + p.cell_off;
  unsigned char* bp = bp_ + p.cell_off;
  double *cur = dtw_diag, *p1 = dtw_diag + Ta, *p2 = dtw_diag + 2 * Ta;  // diagonals d, d - 1, d - 2, indexed by i
  // A thread owns the rows i = tid + DTW_WG c and walks along them, one column per diagonal: consecutive addresses.  The cost of
  // its cell on diagonal d + 1 is loaded while diagonal d is computed, so the load's latency is not in the chain of a diagonal.
  float nxt[DTW_NCH];
#pragma unroll
  for (int c = 0; c < DTW_NCH; ++c) nxt[c] = 0.f;
  if (tid == 0) nxt[0] = cost[0];
  for (int d = 0; d < cap; ++d) {
#pragma unroll
    for (int c = 0; c < DTW_NCH; ++c) {
      if (DTW_WG * c >= Ta) continue;  // uniform: none of these rows exists
      const int i = tid + DTW_WG * c, j = d - i;
      const size_t idx = (size_t)i * Tb + j;  // only used where the cell exists
      const double cv = (double)nxt[c];
      if (i < Ta && j + 1 >= 0 && j + 1 < Tb) nxt[c] = cost[idx + 1];
      if (i < Ta && j >= 0 && j < Tb) {
        double best = 0.0;
        unsigned char b = 0;
        if (i > 0 && j > 0) {
          best = p2[i - 1];
          const double up = p1[i - 1], left = p1[i];
          if (up < best) { best = up; b = 1; }
          if (left < best) { best = left; b = 2; }
        } else if (i > 0) {
          best = p1[i - 1]; b = 1;
        } else if (j > 0) {
          best = p1[i]; b = 2;
        }
        cur[i] = best + cv;
        bp[idx] = b;
      }
    }
    __syncthreads();  // diagonal d is complete, and its readers of d - 2 are done: d + 1 overwrites that buffer
    double* x = p2; p2 = p1; p1 = cur; cur = x;
  }
  int* path = p.path;
  if (tid == 0) {
    int i = Ta - 1, j = Tb - 1, len = 1;
    if (path) { path[2 * (cap - 1)] = i; path[2 * (cap - 1) + 1] = j; }
    while (i > 0 || j > 0) {
      const unsigned char b = i == 0 ? 2 : (j == 0 ? 1 : bp[(size_t)i * Tb + j]);
      if (b != 2) --i;
      if (b != 1) --j;
      if (path) { path[2 * (cap - 1 - len)] = i; path[2 * (cap - 1 - len) + 1] = j; }
      ++len;
    }
    total[blockIdx.x] = p1[Ta - 1];  // the last diagonal holds the one cell (Ta - 1, Tb - 1)
    path_len[blockIdx.x] = len;
    s_len = len;
  }
  __syncthreads();
  if (!path) return;  // uniform
  const int len = s_len, off = cap - len;
  if (off == 0) return;
  // the path sits at the end of the caller's buffer: move it to the front, a chunk at a time in ascending order (a chunk's
  // destination lies below every later chunk's source)
  for (int k0 = 0; k0 < len; k0 += DTW_WG) {
    const int k = k0 + tid;
    int vi = 0, vj = 0;
    if (k < len) { vi = path[2 * (off + k)]; vj = path[2 * (off + k) + 1]; }
    __syncthreads();
    if (k < len) { path[2 * k] = vi; path[2 * k + 1] = vj; }
    __syncthreads();
  }
}

}  // namespace vx
