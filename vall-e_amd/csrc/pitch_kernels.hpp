// Fundamental-frequency tracking (YIN, de Cheveigne & Kawahara 2002) in the filterbank's framing, and the F0 figures along a warp
// path (include/vallex.h, vx_pitch_*).
//
// pitch_track_kernel   one workgroup owns PITCH_TILE consecutive frames of ONE utterance (the tile is found by the filterbank's
//                      tile0 search; a ragged batch is one launch).  The tile's samples go to LDS once, zero past the utterance's
//                      end.
//   differences        h_u(tau) = sum_{j < 256} (x[256 u + j] - x[256 u + j + tau])^2 for the tile's halves u = f0 .. f0 + nft and
//                      tau = 0 .. tau_max, kept in LDS; frame t is d_t = h_t + h_{t+1}, so every half serves two frames.  A thread
//                      owns 4 consecutive lags of one half and walks j in chunks of 8: two 16-byte LDS reads bring x[j .. j + 7],
//                      three the window x[j + tau0 .. j + tau0 + 11], and the 5 reads feed 32 sub + fma pairs.  (u, tau) has 8
//                      fp32 chains, chain q over j = q, q + 8, ... in ascending order, folded as ((0 + 1) + (2 + 3)) + ((4 + 5) +
//                      (6 + 7)): the order is a property of (u, tau) alone, so the half two neighbouring tiles share has the same
//                      bits in both, and a frame's bits depend on its own 1024 samples only.
//   pick               after a barrier, from LDS: a wave takes a frame, lane l the lags 8 l + 1 .. 8 l + 8.  The running sum of d
//                      is fp64: a lane's 8 values in ascending order, the lanes' totals by an inclusive scan of 6 fixed steps.
//                      d'(tau) = d tau / sum evaluated in fp64 and rounded once to fp32 (1 where the sum is 0, and at tau = 0)
//                      goes to the wave's LDS row; the first lag under the threshold, the end of its descent and the first
//                      global minimum are each a per-lane scan in ascending order and a minimum over the wave.
//                      No atomics, no hand-over between workgroups, nothing read back from global memory.
// pitch_compare_kernel one workgroup per pair: thread t takes the path cells t, t + 256, ... in ascending order, every sum in
//                      fp64, then a fixed tree over the 256 partial rows.  A cell outside [0, Ta) x [0, Tb) is clamped into it.
#pragma once
#include "common.hpp"

namespace vx {

constexpr int PITCH_RATE = 24000, PITCH_HOP = 256;
constexpr int PITCH_TAU_LO = 12, PITCH_TAU_HI = 512;     // served: PITCH_TAU_LO <= tau_min < tau_max <= PITCH_TAU_HI
constexpr int PITCH_TILE = 16;                           // frames per workgroup: PITCH_TILE + 1 halves
constexpr int PITCH_WG = 256;
constexpr int PITCH_LD = 516;                            // a row of h or d': lags 0 .. 515 (129 groups of 4)
constexpr int PITCH_SPAN = (PITCH_TILE + 1) * PITCH_HOP + 528;  // samples a tile keeps: the last half's window and its read-ahead
constexpr int PITCH_MAX_BATCH = 64;
constexpr int PITCH_NSUMS = 11;                          // doubles per pair of vx_pitch_compare (include/vallex.h lists them)

struct PitchArgs {
  const float* const* wav;       // [nseg] mono fp32 at 24 kHz
  float* const* f0;              // [nseg] each (frames), entries nullable: so for every output
  float* const* ap;
  int* const* lag;
  unsigned char* const* voiced;
  float* const* dp;              // [nseg] (frames, tau_max + 1): d' itself (vx_op_pitch_diff)
  const int* tile0;              // [nseg + 1] first tile of every utterance (an utterance without frames has none)
  const int* len;                // [nseg] samples
  const int* frames;             // [nseg] (L + 128) / 256
  int nseg, tau_min, tau_max;
  float threshold;
};

struct PitchPair {
  const float* fa;   // (Ta) f0 in Hz, 0 = unvoiced
  const float* fb;   // (Tb)
  const int* path;   // (plen, 2) cells (i, j)
  int Ta, Tb, plen, pad_;
};

__device__ __forceinline__ int pitch_wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}

__global__ __launch_bounds__(PITCH_WG) void pitch_track_kernel(const PitchArgs a) {
  __shared__ __attribute__((aligned(16))) float S[PITCH_SPAN];
  __shared__ __attribute__((aligned(16))) float H[(PITCH_TILE + 1) * PITCH_LD];
  __shared__ float DP[(PITCH_WG / 64) * PITCH_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tau_min = a.tau_min, tau_max = a.tau_max;
  const int G = (tau_max + 4) >> 2;  // groups of 4 lags covering 0 .. tau_max
  const int total = a.tile0[a.nseg];
  for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {
    int s = 0;  // the utterance of the tile: the last s with tile0[s] <= tile (utterances without tiles share a start: the last wins)
    for (int hi_s = a.nseg; hi_s - s > 1;) {
      const int mid = (s + hi_s) >> 1;
      if (a.tile0[mid] <= tile) s = mid;
      else hi_s = mid;
    }
    const float* x = a.wav[s];
    const long L = a.len[s];
    const int f0 = (tile - a.tile0[s]) * PITCH_TILE;
    const int nft = min(PITCH_TILE, a.frames[s] - f0);  // >= 1
    const int nh = nft + 1;
    const long g0 = (long)f0 * PITCH_HOP;
    const int span = nh * PITCH_HOP + 528;  // <= PITCH_SPAN
    __syncthreads();  // the previous tile's reads of S, H and DP are done
    for (int i = tid; i < span; i += PITCH_WG) S[i] = g0 + i < L ? x[g0 + i] : 0.f;
    __syncthreads();

    // ---- differences ----
    for (int unit = tid; unit < nh * G; unit += PITCH_WG) {
      const int u = unit / G, g = unit - u * G;
      const float4* xa = (const float4*)(S + PITCH_HOP * u);
      const float4* xw = (const float4*)(S + PITCH_HOP * u + 4 * g);
      float acc[4][8];
#pragma unroll
      for (int l = 0; l < 4; ++l)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[l][q] = 0.f;
      for (int c = 0; c < PITCH_HOP / 8; ++c) {
        const float4 a0 = xa[2 * c], a1 = xa[2 * c + 1];
        const float4 w0 = xw[2 * c], w1 = xw[2 * c + 1], w2 = xw[2 * c + 2];
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float wv[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
          for (int l = 0; l < 4; ++l) {
            const float df = __fsub_rn(av[q], wv[q + l]);
            acc[l][q] = fmaf(df, df, acc[l][q]);
          }
      }
      float4 hv;
      float* hp = (float*)&hv;
#pragma unroll
      for (int l = 0; l < 4; ++l)
        hp[l] = __fadd_rn(__fadd_rn(__fadd_rn(acc[l][0], acc[l][1]), __fadd_rn(acc[l][2], acc[l][3])),
                          __fadd_rn(__fadd_rn(acc[l][4], acc[l][5]), __fadd_rn(acc[l][6], acc[l][7])));
      *(float4*)(H + PITCH_LD * u + 4 * g) = hv;
    }
    __syncthreads();

    // ---- pick: wave w takes the frames w, w + 4, ...; every wave runs every round (the barriers are uniform) ----
    float* dpw = DP + wave * PITCH_LD;
    for (int fl0 = 0; fl0 < nft; fl0 += PITCH_WG / 64) {
      const int fl = fl0 + wave;
      const bool live = fl < nft;
      if (live) {
        const float* ha = H + PITCH_LD * fl;
        const float* hb = ha + PITCH_LD;
        float dv[8];
        double loc[8], run = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int tau = 8 * lane + 1 + k;
          dv[k] = tau <= tau_max ? __fadd_rn(ha[tau], hb[tau]) : 0.f;
          run += (double)dv[k];
          loc[k] = run;
        }
        double inc = run;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const double o = __shfl_up(inc, off);
          if (lane >= off) inc += o;
        }
        double excl = __shfl_up(inc, 1);
        if (lane == 0) excl = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int tau = 8 * lane + 1 + k;
          const double sum = excl + loc[k];
          if (tau <= tau_max) dpw[tau] = sum > 0.0 ? (float)((double)dv[k] * (double)tau / sum) : 1.f;
        }
        if (lane == 0) dpw[0] = 1.f;
      }
      __syncthreads();
      if (live) {
        const float thr = a.threshold;
        const int NONE = 0x7fffffff;
        int first = NONE;
#pragma unroll
        for (int k = 7; k >= 0; --k) {
          const int tau = 8 * lane + 1 + k;
          if (tau >= tau_min && tau <= tau_max && dpw[tau] < thr) first = tau;
        }
        first = pitch_wave_min(first);
        int best;
        const bool is_voiced = first != NONE;
        if (is_voiced) {
          int stop = NONE;  // the first lag >= `first` at which the descent ends
#pragma unroll
          for (int k = 7; k >= 0; --k) {
            const int tau = 8 * lane + 1 + k;
            if (tau >= first && tau <= tau_max && !(tau < tau_max && dpw[tau + 1] < dpw[tau])) stop = tau;
          }
          best = pitch_wave_min(stop);
        } else {
          float mv = INFINITY;
          int mi = NONE;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int tau = 8 * lane + 1 + k;
            if (tau >= tau_min && tau <= tau_max && (mi == NONE || dpw[tau] < mv)) { mv = dpw[tau]; mi = tau; }
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(mv, off);
            const int oi = __shfl_xor(mi, off);
            if (oi != NONE && (mi == NONE || ov < mv || (ov == mv && oi < mi))) { mv = ov; mi = oi; }
          }
          best = mi;  // tau_min .. tau_max is never empty
        }
        if (lane == 0) {
          const long t = (long)f0 + fl;
          const float b = dpw[best];
          double off = 0.0;
          if (best < tau_max) {
            const double pa = (double)dpw[best - 1], pc = (double)dpw[best + 1];
            const double den = pa - 2.0 * (double)b + pc;
            if (den > 0.0) off = fmin(0.5, fmax(-0.5, (pa - pc) / (2.0 * den)));
          }
          if (a.f0[s]) a.f0[s][t] = is_voiced ? (float)((double)PITCH_RATE / ((double)best + off)) : 0.f;
          if (a.ap[s]) a.ap[s][t] = b;
          if (a.lag[s]) a.lag[s][t] = best;
          if (a.voiced[s]) a.voiced[s][t] = is_voiced ? 1 : 0;
        }
        if (a.dp[s]) {
          float* o = a.dp[s] + ((long)f0 + fl) * (tau_max + 1);
          for (int tau = lane; tau <= tau_max; tau += 64) o[tau] = dpw[tau];
        }
      }
      __syncthreads();  // the wave's row is free for its next frame
    }
  }
}

// sums[pair][PITCH_NSUMS]: n_path, n_voiced_both, n_vuv_mismatch, then over the cells voiced in both: sum c, sum c^2 (c = 1200
// log2(fa / fb)), sum (fa - fb)^2, sum la, sum lb, sum la^2, sum lb^2, sum la lb (la = ln fa, lb = ln fb).
__global__ __launch_bounds__(PITCH_WG) void pitch_compare_kernel(const PitchPair* __restrict__ pairs, double* __restrict__ sums) {
  __shared__ double R[PITCH_NSUMS][PITCH_WG];
  const PitchPair p = pairs[blockIdx.x];
  const int tid = threadIdx.x;
  double v[PITCH_NSUMS];
#pragma unroll
  for (int q = 0; q < PITCH_NSUMS; ++q) v[q] = 0.0;
  for (int k = tid; k < p.plen; k += PITCH_WG) {
    const int i = min(max(p.path[2 * (long)k], 0), p.Ta - 1), j = min(max(p.path[2 * (long)k + 1], 0), p.Tb - 1);
    const float fa = p.fa[i], fb = p.fb[j];
    const bool va = fa > 0.f, vb = fb > 0.f;
    v[0] += 1.0;
    if (va != vb) v[2] += 1.0;
    if (va && vb) {
      const double da = (double)fa, db = (double)fb;
      const double c = 1200.0 * log2(da / db), hz = da - db, la = log(da), lb = log(db);
      v[1] += 1.0;
      v[3] += c;
      v[4] = fma(c, c, v[4]);
      v[5] = fma(hz, hz, v[5]);
      v[6] += la;
      v[7] += lb;
      v[8] = fma(la, la, v[8]);
      v[9] = fma(lb, lb, v[9]);
      v[10] = fma(la, lb, v[10]);
    }
  }
#pragma unroll
  for (int q = 0; q < PITCH_NSUMS; ++q) R[q][tid] = v[q];
  __syncthreads();
  for (int w = PITCH_WG / 2; w > 0; w >>= 1) {
    if (tid < w)
#pragma unroll
      for (int q = 0; q < PITCH_NSUMS; ++q) R[q][tid] += R[q][tid + w];
    __syncthreads();
  }
  if (tid < PITCH_NSUMS) sums[(size_t)blockIdx.x * PITCH_NSUMS + tid] = R[tid][0];
}

}  // namespace vx
