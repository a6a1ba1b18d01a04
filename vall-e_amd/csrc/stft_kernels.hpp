// Multi-resolution STFT distance between two waveforms, and the STFT magnitudes themselves (include/vallex.h, vx_stft_*).
//
// The DFT of a frame is DIRECT: a row GEMM over the `win` samples the window does not zero, on the fp32 matrix instruction
// (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, one rounding per product),
//   re[f][k] = sum_j x_f[j] w[j] cos(2 pi k (off + j) / n_fft),   im[f][k] = sum_j x_f[j] w[j] sin(2 pi k (off + j) / n_fft),
// x_f[j] = sample f hop - n_fft / 2 + off + j reflected into [0, L), off = (n_fft - win) / 2.  The first operand is 32 rows of
// windowed samples (row = lane & 31, the two samples of a step in the lane halves), the second 32 bins of one cos (or sin) table
// of n_fft entries in LDS, indexed (k (off + j)) mod n_fft; sin(2 pi m / n) is the cos table at m - n / 4.  The table is built
// on the host in fp64 and rounded once.  A sum over j never runs long in fp32: step s (samples 2 s and 2 s + 1) goes to chain s
// mod STFT_CHAINS, and after STFT_SEG steps of every chain the chains are added, chain 0 first, to fp64 totals and start again
// from zero.  An fp32 chain so carries the rounding of 2 STFT_SEG terms, not of win.  re^2 + im^2, the clamp and the root are
// fp64 on the totals, rounded once to the fp32 magnitude.  (Why not the filterbank's four-step factorisation: DESIGN.md section 7.)
//
// One workgroup owns a tile of consecutive frames of ONE pair at ONE resolution.  In a compare launch rows 0..15 are frames of
// pred (X) and rows 16..31 the same frames of target (Y), so both magnitudes of a cell land in one lane (accumulator registers r
// and r + 8); in a magnitude launch the 32 rows are 32 frames of one signal.  The tile's samples go to LDS once, the reflection
// about sample 0 and about sample L - 1 resolved by index while loading.  Sample i of the tile is kept at i + (i / hop) pad with
// hop + pad = 2 (mod 32), and target's copy starts at an odd offset: the 32 rows a wave half reads in one ds_read_b32 (16
// frames of both signals, hop apart) then fall on 32 different banks instead of on 2 (hop 240) or 4 (hop 120).
// The bins 0 .. n_fft / 2 - 1 are n_fft / 64 blocks of 32; a workgroup takes STFT_GROUP of them (a "unit": tile x group of
// blocks, n_fft / 512 groups per tile whatever the batch), wave w the blocks w and w + 4 of the group.  Bin n_fft / 2 rides in
// block 0: bin 0 has no imaginary part (its sin column is zero), so lane 0's sin column carries cos(pi (off + j)) instead, and
// the "imaginary" total of column 0 is the real part of bin n_fft / 2 (whose own imaginary part is zero as well).
//   compare    every lane adds its cells in fp64, blocks and registers ascending: (Y - X)^2, Y^2, |ln Y - ln X|; then a fixed
//              tree over the lanes, the four waves in order, and the unit's three sums go to the workspace.
//              stft_finish_kernel adds the units of every (pair, resolution) in ascending order.  No atomics.
//   magnitude  the store in place of the reduction.
// A cell's bits depend on its own frame's samples only: never on the batch or on the tile's place in the launch.
#pragma once
#include "common.hpp"

namespace vx {

constexpr int STFT_RATE = 24000;
constexpr int STFT_MAX_RES = 4, STFT_MAX_BATCH = 64, STFT_MAX_NFFT = 2048;
constexpr int STFT_WG = 256;
constexpr int STFT_CHAINS = 4, STFT_SEG = 8;               // fp32 chains of a sum, and the steps of a chain between two folds to fp64
constexpr int STFT_WIN_PAD = 2 * STFT_CHAINS;              // the window is zero-padded to a multiple of this
constexpr int STFT_SPAN = 5632;                            // LDS words of one signal of a compare tile (a magnitude tile: twice)
constexpr int STFT_YOFF = STFT_SPAN + 1;                   // target's copy: an odd offset (banks, above)
constexpr int STFT_ROWS_CMP = 16, STFT_ROWS_MAG = 32;      // most frames of a tile
constexpr int STFT_GROUP = 8;                              // blocks of 32 bins a workgroup takes: n_fft / 512 groups per tile

struct StftArgs {
  const float* const* x;    // [nseg] pred (compare) or the signal (magnitude)
  const float* const* y;    // [nseg] target (compare)
  float* const* out;        // [nseg] (frames, n_fft / 2 + 1) (magnitude)
  const int* tile0;         // [nseg + 1] first tile of every segment within this launch
  const int* len;           // [nseg] (common) length in samples, > n_fft / 2
  const int* frames;        // [nseg] 1 + len / hop
  const float* tab;         // [n_fft] cos(2 pi m / n_fft)
  const float* win;         // [win_pad] periodic Hann, zeros past win
  double* ws;               // [tile_base + unit][3] (compare); unit = tile * groups + group
  int nseg, n_fft, hop, win_pad, off, ft, tile_base, pad;
  float eps;
};

// The skew of a hop: hop + pad = 2 (mod 32).  A hop below 16 would more than double the tile and is left as it is.
inline int stft_pad(int hop) { return hop >= 16 ? ((2 - hop) & 31) : 0; }

// Frames per tile: as many of the rows as fit the LDS block with the skew (the device takes it from StftArgs::ft).  A frame
// always fits: 2047 + (2047 / 16) 18 < STFT_SPAN.
inline int stft_tile_frames(bool compare, int hop, int win_pad) {
  const int cap = compare ? STFT_SPAN : 2 * STFT_SPAN, rows = compare ? STFT_ROWS_CMP : STFT_ROWS_MAG;
  const int pad = stft_pad(hop), last = (win_pad - 1) + ((win_pad - 1) / hop) * pad;  // LDS word of a frame's last sample
  const int fit = 1 + (cap - last - 1) / (hop + pad);
  return fit < rows ? fit : rows;
}

template <bool COMPARE>
__global__ __launch_bounds__(STFT_WG) void stft_tile_kernel(const StftArgs a) {
  typedef float f32x16 __attribute__((ext_vector_type(16)));
  __shared__ float S[2 * STFT_SPAN + 2];
  __shared__ float T[STFT_MAX_NFFT];
  __shared__ float W[STFT_MAX_NFFT + STFT_WIN_PAD];
  __shared__ double R[STFT_WG / 64][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
  const int N = a.n_fft, mask = N - 1, bins = N / 2 + 1, hop = a.hop, pad = a.pad, steps = a.win_pad / 2;
  for (int i = tid; i < N; i += STFT_WG) T[i] = a.tab[i];
  for (int i = tid; i < a.win_pad; i += STFT_WG) W[i] = a.win[i];
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int groups = N / (64 * STFT_GROUP);  // n_fft / 2 bins in groups of 32 STFT_GROUP: 1, 2 or 4
  const int total = a.tile0[a.nseg];
  for (int unit = blockIdx.x; unit < total * groups; unit += gridDim.x) {
    const int tile = unit / groups, grp = unit - tile * groups;
    int s = 0;  // the segment of the tile: the last s with tile0[s] <= tile
    for (int hi_s = a.nseg; hi_s - s > 1;) {
      const int mid = (s + hi_s) >> 1;
      if (a.tile0[mid] <= tile) s = mid;
      else hi_s = mid;
    }
    const long L = a.len[s];
    const int f0 = (tile - a.tile0[s]) * a.ft;
    const int nft = min(a.ft, a.frames[s] - f0);  // >= 1
    const long g0 = (long)f0 * hop - N / 2 + a.off;
    const int span = (nft - 1) * hop + a.win_pad;  // with the skew <= STFT_SPAN words (compare), 2 STFT_SPAN (magnitude)
    __syncthreads();  // the previous tile's reads of S and R are done
    {
      const float* x = a.x[s];
      const float* y = COMPARE ? a.y[s] : nullptr;
      for (int i = tid; i < span; i += STFT_WG) {
        long p = g0 + i;
        if (p < 0) p = -p;
        if (p >= L) p = 2 * (L - 1) - p;
        p = min(max(p, 0L), L - 1);  // only the zero-weighted padding of the last frame can get here
        const int w = i + (i / hop) * pad;
        S[w] = x[p];
        if (COMPARE) S[STFT_YOFF + w] = y[p];
      }
    }
    __syncthreads();
    // the lane's row of the first operand
    const int row_f = COMPARE ? (c & 15) : c;
    const float* xr = S + (COMPARE ? (c >> 4) * STFT_YOFF : 0) + min(row_f, nft - 1) * (hop + pad);
    const float* wr = W + h;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int b = wave; b < STFT_GROUP; b += STFT_WG / 64) {
      const int k = 32 * (STFT_GROUP * grp + b) + c;  // the lane's bin of the second operand and of the result
      const bool dc = k == 0;                         // column 0: bin 0 in the real totals, bin n_fft / 2 in the imaginary ones
      int m = (k * (a.off + h)) & mask;
      const int dm = (2 * k) & mask;
      int ms = dc ? ((N / 2) * (a.off + h)) & mask : (m - N / 4) & mask;  // the sin column's place in the cos table
      int col = h, rem = h;  // sample j = 2 s + h of the row: its LDS word, and j mod hop (kept only where pad != 0, hop >= 16)
      double tre[16], tim[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) tre[r] = tim[r] = 0.0;
      for (int st0 = 0; st0 < steps; st0 += STFT_CHAINS * STFT_SEG) {
        const int st1 = min(steps, st0 + STFT_CHAINS * STFT_SEG);  // steps is a multiple of STFT_CHAINS
        f32x16 re[STFT_CHAINS], im[STFT_CHAINS];
#pragma unroll
        for (int q = 0; q < STFT_CHAINS; ++q) re[q] = im[q] = zero;
        for (int st = st0; st < st1; st += STFT_CHAINS) {
#pragma unroll
          for (int q = 0; q < STFT_CHAINS; ++q) {
            const float v = xr[col] * wr[2 * (st + q)];
            const float cs = T[m], sn = T[ms];
            re[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(v, cs, re[q], 0, 0, 0);
            im[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(v, sn, im[q], 0, 0, 0);
            m = (m + dm) & mask;
            ms = (ms + dm) & mask;  // dm = 0 in column 0: (n_fft / 2) 2 = 0 (mod n_fft) as well
            col += 2;
            rem += 2;
            if (rem >= hop) { rem -= hop; col += pad; }
          }
        }
#pragma unroll
        for (int q = 0; q < STFT_CHAINS; ++q)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            tre[r] += (double)re[q][r];
            tim[r] += (double)im[q][r];
          }
      }
      const double eps = (double)a.eps;
      if (COMPARE) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const int f = (r & 3) + 8 * (r >> 2) + 4 * h;  // row f is pred's frame, row f + 16 (register r + 8) target's
          if (f < nft) {
            // column 0 holds two cells: bin 0, then bin n_fft / 2
            const double px = dc ? tre[r] * tre[r] : fma(tre[r], tre[r], tim[r] * tim[r]);
            const double py = dc ? tre[r + 8] * tre[r + 8] : fma(tre[r + 8], tre[r + 8], tim[r + 8] * tim[r + 8]);
            const double X = (double)(float)sqrt(fmax(px, eps)), Y = (double)(float)sqrt(fmax(py, eps)), d = Y - X;
            s0 = fma(d, d, s0);
            s1 = fma(Y, Y, s1);
            s2 += fabs(log(Y) - log(X));
            if (dc) {
              const double X2 = (double)(float)sqrt(fmax(tim[r] * tim[r], eps)), Y2 = (double)(float)sqrt(fmax(tim[r + 8] * tim[r + 8], eps));
              const double d2 = Y2 - X2;
              s0 = fma(d2, d2, s0);
              s1 = fma(Y2, Y2, s1);
              s2 += fabs(log(Y2) - log(X2));
            }
          }
        }
      } else {
        float* o = a.out[s] + (long)f0 * bins + k;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int f = (r & 3) + 8 * (r >> 2) + 4 * h;
          if (f < nft) {
            const double p = dc ? tre[r] * tre[r] : fma(tre[r], tre[r], tim[r] * tim[r]);
            o[(long)f * bins] = (float)sqrt(fmax(p, eps));
            if (dc) o[(long)f * bins + N / 2] = (float)sqrt(fmax(tim[r] * tim[r], eps));
          }
        }
      }
    }
    if (COMPARE) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
      }
      if (lane == 0) { R[wave][0] = s0; R[wave][1] = s1; R[wave][2] = s2; }
      __syncthreads();
      if (tid < 3) a.ws[3 * ((long)a.tile_base + unit) + tid] = ((R[0][tid] + R[1][tid]) + R[2][tid]) + R[3][tid];
    }
  }
}

// Thread (pr, q): sum q of (pair, resolution) pr = pair * n_res + res, over its units [tbeg[pr], tend[pr]) of the workspace in
// ascending order.  sums[pr] = {sum (Y - X)^2, sum Y^2, sum |ln Y - ln X|, cells}.
__global__ __launch_bounds__(64) void stft_finish_kernel(const double* __restrict__ ws, const int* __restrict__ tbeg, const int* __restrict__ tend,
                                                         const double* __restrict__ cells, int npr, double* __restrict__ sums) {
  const int id = blockIdx.x * 64 + threadIdx.x, pr = id >> 2, q = id & 3;
  if (pr >= npr) return;
  if (q == 3) {
    sums[4 * (long)pr + 3] = cells[pr];
    return;
  }
  double acc = 0.0;
  for (int t = tbeg[pr]; t < tend[pr]; ++t) acc += ws[3 * (long)t + q];
  sums[4 * (long)pr + q] = acc;
}

}  // namespace vx
