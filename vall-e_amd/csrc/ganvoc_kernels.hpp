// HiFi-GAN / BigVGAN generator kernels (log-mel frames -> waveform), fp32 storage and fp32 accumulation.  The definition is in
// include/vallex.h (vx_gan_*); the host side is ganvoc.hip.
//
// Layout: time-major rows [frames * rate, C]; the utterances of a group are concatenated and every kernel receives the segment
// starts in FRAMES (seg[nseg] = total) plus the rows-per-frame rate of its operand, as the codec's kernels do.  No tap, no pad and
// no halo crosses a segment boundary.
//
//   gan_pack_rows   the callers' (T_i, n_mels) inputs -> concatenated rows, with SpeechT5HifiGan's (x - mean) / scale when given.
//   gan_gemm_rows   conv_pre, every residual convolution and every transposed convolution as a row GEMM
//                   C[row][n] = bias[n] + sum_k A(row, k) W[n][k] on v_mfma_f32_32x32x2_f32 (the tile structure of
//                   codec_gemm_rows: 32x32 accumulator per wave, BK = 16, four accumulators over interleaved k pairs summed
//                   pairwise).  A is gathered while it is staged: k = tap * C + c reads row t + off0 + tap * step of the row's own
//                   segment, zero outside it, through an optional leaky ReLU.  A dilated "same" convolution is off0 = -d (k-1)/2,
//                   step = d.  A transposed convolution (stride u, kernel k, padding p = (k-u)/2) is the same GEMM over the input
//                   rows t - q for every q with a tap 0 <= q u + r + p < k for some phase r: N = u * C_out, and output row t IS
//                   rows t u .. t u + u - 1 of the up-sampled signal (the host packs W with zeros where a phase has no tap).
//                   Epilogue: bias, residual add, and for the last convolution of a residual block the running stage sum
//                   (first block stores, later ones add, the last divides by R): one launch after the other, no atomics.
//   gan_aa_act      BigVGAN's anti-aliased periodic activation, fused: 2x polyphase up-sampling (6 taps per phase), Snake with the
//                   precise sinf, 12-tap low-pass at stride 2.  A workgroup owns GAN_AA_TT rows x GAN_AA_CC channels of ONE segment:
//                   it stages the rows plus a halo of 5 in LDS, forms every up-sampled value of its span once in LDS (the 2x signal
//                   never reaches memory) and filters it down.  Both replicate pads are index clamps: the down step clamps into the
//                   2L-long up-sampled signal of the segment, the up step clamps into the segment's L rows.
//   gan_conv_post   the last convolution (C -> 1, zero padding) with tanhf: one output sample per lane, straight into every
//                   utterance's own output.
#pragma once
#include "common.hpp"

namespace vx {

constexpr int GAN_MAX_SEG = 64;  // utterances per launch (vx_gan_config.max_batch <= 64)
constexpr int GAN_AA_TAPS = 12;
constexpr int GAN_AA_TT = 32;    // rows per workgroup of gan_aa_act
constexpr int GAN_AA_CC = 64;    // channels per workgroup

enum GanAccum { GAN_ACC_NONE = 0, GAN_ACC_FIRST = 1, GAN_ACC_ADD = 2 };

// Segment of `row` (rows = frames * rate): index, lo / len in rows.  nseg <= 64: a linear scan of scalars; empty segments are skipped.
__device__ __forceinline__ int gan_find_seg(const int* __restrict__ seg, int nseg, int rate, long row, long& lo, long& len) {
  int s = 0;
  while (s + 1 < nseg && (long)seg[s + 1] * rate <= row) ++s;
  lo = (long)seg[s] * rate;
  len = (long)seg[s + 1] * rate - lo;
  return s;
}

__device__ __forceinline__ float gan_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }
__device__ __forceinline__ long gan_clamp(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// (T_i, C) per utterance -> rows [sum T_i][C]; mean / scale [C] or null.
__global__ __launch_bounds__(256) void gan_pack_rows(const float* const* __restrict__ in, float* __restrict__ rows,
                                                     const float* __restrict__ mean, const float* __restrict__ scale, long M, int C,
                                                     const int* __restrict__ seg, int nseg) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * C) return;
  const long row = i / C;
  const int c = (int)(i - row * C);
  long lo, len;
  const int s = gan_find_seg(seg, nseg, 1, row, lo, len);
  float v = in[s][(row - lo) * C + c];
  if (mean) v = (v - mean[c]) / scale[c];
  rows[i] = v;
}

struct GanGemmArgs {
  const float* x;     // rows [*, C]
  int C, taps;        // K = taps * C, k = tap * C + c
  int off0, step;     // tap j of local row t reads local row t + off0 + j * step, zero outside [0, len)
  int lrelu;          // leaky ReLU on the gathered operand
  float slope;
  const float* W;     // [N][K] row-major
  const float* bias;  // [N] or null
  const float* res;   // [M][N] or null: added to the result (may alias out: every cell is read and written by one lane)
  float* out;         // [M][N]: written when acc == GAN_ACC_NONE
  float* sum;         // [M][N]: the stage sum, acc != GAN_ACC_NONE
  int acc;
  float div;          // != 0: the stored stage sum is divided by it (the last residual block: R)
  long M;
  int N, K;
  const int* seg;     // nseg + 1 frame offsets (device)
  int nseg, rate;     // rows per frame of the operand rows (= of the GEMM's M rows)
};

// BM = 32 * WM rows x BN = 32 * WN columns per workgroup of WM * WN waves (one 32x32 accumulator tile each), BK = 16.
// LDS tiles are [row][BK + 1] (odd stride: the per-lane operand reads A[l & 31][l >> 5] hit 32 different banks).
// VEC: C is a multiple of 16, so a K chunk lies in one tap and is loaded as float4 (rows are then 64-byte multiples).
template <int WM, int WN, bool VEC>
__global__ __launch_bounds__(WM * WN * 64) void gan_gemm_rows(const GanGemmArgs a) {
  constexpr int BM = 32 * WM, BN = 32 * WN, BK = 16, LD = BK + 1, NT = WM * WN * 64;
  constexpr int A_V = BM * BK / 4 / NT > 0 ? BM * BK / 4 / NT : 1;  // float4 per thread of the A tile
  constexpr int B_V = BN * BK / 4 / NT > 0 ? BN * BK / 4 / NT : 1;
  __shared__ float As[BM * LD];
  __shared__ float Bs[BN * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;

  // this thread's A rows: slot v covers tile row (tid + v * NT) / 4, k quad (tid + v * NT) % 4
  long seg_lo[A_V], seg_len[A_V];
#pragma unroll
  for (int v = 0; v < A_V; ++v) {
    const int idx = tid + v * NT;
    const long row = m0 + idx / 4;
    seg_lo[v] = 0;
    seg_len[v] = 0;
    if (idx < BM * BK / 4 && row < a.M) gan_find_seg(a.seg, a.nseg, a.rate, row, seg_lo[v], seg_len[v]);
  }

  float ra[A_V][4], rb[B_V][4];
  auto load = [&](int k0) {
#pragma unroll
    for (int v = 0; v < A_V; ++v) {
      const int idx = tid + v * NT;
      const long row = m0 + idx / 4;
      const int kq = (idx % 4) * 4;
      ra[v][0] = ra[v][1] = ra[v][2] = ra[v][3] = 0.f;
      if (idx >= BM * BK / 4 || row >= a.M) continue;
      if (VEC) {
        const int k = k0 + kq;
        const int tap = k / a.C, c = k - tap * a.C;
        const long src = row - seg_lo[v] + a.off0 + (long)tap * a.step;
        if (k < a.K && src >= 0 && src < seg_len[v]) {
          const float4 f = *reinterpret_cast<const float4*>(a.x + (seg_lo[v] + src) * a.C + c);
          ra[v][0] = f.x; ra[v][1] = f.y; ra[v][2] = f.z; ra[v][3] = f.w;
          if (a.lrelu) {
#pragma unroll
            for (int q = 0; q < 4; ++q) ra[v][q] = gan_lrelu(ra[v][q], a.slope);
          }
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = k0 + kq + q;
          if (k >= a.K) continue;
          const int tap = k / a.C, c = k - tap * a.C;
          const long src = row - seg_lo[v] + a.off0 + (long)tap * a.step;
          if (src >= 0 && src < seg_len[v]) {
            const float f = a.x[(seg_lo[v] + src) * a.C + c];
            ra[v][q] = a.lrelu ? gan_lrelu(f, a.slope) : f;
          }
        }
      }
    }
#pragma unroll
    for (int v = 0; v < B_V; ++v) {
      const int idx = tid + v * NT;
      const int n = n0 + idx / 4;
      const int k = k0 + (idx % 4) * 4;
      rb[v][0] = rb[v][1] = rb[v][2] = rb[v][3] = 0.f;
      if (idx >= BN * BK / 4 || n >= a.N) continue;
      const float* w = a.W + (long)n * a.K + k;
      if (VEC) {  // K is a multiple of 16 here
        const float4 f = *reinterpret_cast<const float4*>(w);
        rb[v][0] = f.x; rb[v][1] = f.y; rb[v][2] = f.z; rb[v][3] = f.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (k + q < a.K) rb[v][q] = w[q];
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int v = 0; v < A_V; ++v) {
      const int idx = tid + v * NT;
      if (idx < BM * BK / 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) As[(idx / 4) * LD + (idx % 4) * 4 + q] = ra[v][q];
      }
    }
#pragma unroll
    for (int v = 0; v < B_V; ++v) {
      const int idx = tid + v * NT;
      if (idx < BN * BK / 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) Bs[(idx / 4) * LD + (idx % 4) * 4 + q] = rb[v][q];
      }
    }
  };

  typedef float f32x16 __attribute__((ext_vector_type(16)));
  // four accumulators over interleaved k pairs, summed pairwise at the end: each is a chain of K / 4 products (the instruction
  // rounds once per product, like fmaf; one K-long chain was measured at 7.4x the host floor in the codec)
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 acc4[4] = {zero, zero, zero, zero};
  const float* ap = As + (wm * 32 + (lane & 31)) * LD + (lane >> 5);
  const float* bp = Bs + (wn * 32 + (lane & 31)) * LD + (lane >> 5);
  load(0);
  for (int k0 = 0; k0 < a.K; k0 += BK) {
    __syncthreads();  // the previous chunk's operand reads are done
    stage();
    __syncthreads();
    if (k0 + BK < a.K) load(k0 + BK);  // in flight behind this chunk's matrix instructions
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2)
      acc4[(kk >> 1) & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk], acc4[(kk >> 1) & 3], 0, 0, 0);
  }
  const f32x16 acc = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
  // D: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int n = n0 + wn * 32 + (lane & 31);
  if (n < a.N) {
    const float b = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row >= a.M) continue;
      const long i = row * a.N + n;
      float v = acc[r] + b;
      if (a.res) v = a.res[i] + v;
      if (a.acc == GAN_ACC_NONE) {
        a.out[i] = v;
      } else {
        if (a.acc == GAN_ACC_ADD) v = a.sum[i] + v;
        a.sum[i] = a.div != 0.f ? v / a.div : v;
      }
    }
  }
}

struct GanActArgs {
  const float* x;     // rows [M][C]
  float* y;           // rows [M][C]
  const float* a;     // [C] the frequency (exp(alpha) under logscale)
  const float* invb;  // [C] 1 / (b + 1e-9), b = a for snake
  long M;
  int C;
  const int* seg;
  int nseg, rate;
  float f[GAN_AA_TAPS];
};

// grid.x >= sum over the segments of ceil(len / GAN_AA_TT) (the host launches ceil(M / TT) + nseg), grid.y = ceil(C / GAN_AA_CC).
__global__ __launch_bounds__(256) void gan_aa_act(const GanActArgs p) {
  constexpr int TT = GAN_AA_TT, CC = GAN_AA_CC, XR = TT + 10, VR = 2 * TT + 11;
  __shared__ float X[XR * CC];
  __shared__ float V[VR * CC];
  __shared__ float F[GAN_AA_TAPS];
  // the tile's segment: tiles are counted per segment, so that no tile spans two
  long lo = 0, L = 0, t0 = 0;
  {
    long tile = blockIdx.x;
    int s = 0;
    for (; s < p.nseg; ++s) {
      lo = (long)p.seg[s] * p.rate;
      L = (long)p.seg[s + 1] * p.rate - lo;
      const long nt = (L + TT - 1) / TT;
      if (tile < nt) break;
      tile -= nt;
    }
    if (s == p.nseg) return;  // past the last tile (uniform over the workgroup)
    t0 = tile * TT;
  }
  const int tt = L - t0 < TT ? (int)(L - t0) : TT;
  const int tid = threadIdx.x, cl = tid & (CC - 1), r0 = tid / CC;  // 4 row groups
  const int c = blockIdx.y * CC + cl;
  const bool live = c < p.C;
  const long xlo = gan_clamp(t0 - 5, 0, L - 1), xhi = gan_clamp(t0 + tt - 1 + 5, 0, L - 1);
  const long nlo = gan_clamp(2 * t0 - 5, 0, 2 * L - 1), nhi = gan_clamp(2 * (t0 + tt - 1) + 6, 0, 2 * L - 1);
  if (tid < GAN_AA_TAPS) F[tid] = p.f[tid];
  for (long i = xlo + r0; i <= xhi; i += 256 / CC) X[(i - xlo) * CC + cl] = live ? p.x[(lo + i) * p.C + c] : 0.f;
  __syncthreads();
  const float fa = live ? p.a[c] : 0.f, fib = live ? p.invb[c] : 0.f;
  for (long n = nlo + r0; n <= nhi; n += 256 / CC) {
    const long m = n >> 1;
    // even n: taps f[1], f[3], .. against x[m + 2], x[m + 1], ..; odd n: f[0], f[2], .. against x[m + 3], x[m + 2], ..
    const int odd = (int)(n & 1);
    float u = 0.f;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      long i = m + 2 + odd - s;
      i = gan_clamp(i, 0, L - 1);   // the replicate pad of the up step
      i = gan_clamp(i, xlo, xhi);   // inside the staged rows by construction
      const float xv = X[(i - xlo) * CC + cl];
      const float fv = F[2 * s + 1 - odd];
      u = s == 0 ? xv * fv : fmaf(xv, fv, u);
    }
    u *= 2.f;
    const float sn = sinf(u * fa);
    V[(n - nlo) * CC + cl] = fmaf(sn * sn, fib, u);
  }
  __syncthreads();
  if (!live) return;
  for (int t = r0; t < tt; t += 256 / CC) {
    const long tg = t0 + t;
    float y = 0.f;
#pragma unroll
    for (int j = 0; j < GAN_AA_TAPS; ++j) {
      long n = 2 * tg + j - 5;
      n = gan_clamp(n, 0, 2 * L - 1);  // the replicate pad of the down step, on the cropped up-sampled signal
      n = gan_clamp(n, nlo, nhi);
      const float vv = V[(n - nlo) * CC + cl];
      y = j == 0 ? vv * F[0] : fmaf(vv, F[j], y);
    }
    p.y[(lo + tg) * p.C + c] = y;
  }
}

// out[s][t] = tanh(bias + sum_{j, c} act(x[t + j - (taps-1)/2][c]) w[j * C + c]), zero outside the segment; one sample per lane.
__global__ __launch_bounds__(256) void gan_conv_post(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* const* __restrict__ out, long M, int C,
                                                     int taps, int lrelu, float slope, const int* __restrict__ seg, int nseg, int rate) {
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  long lo, len;
  const int s = gan_find_seg(seg, nseg, rate, row, lo, len);
  const long t = row - lo;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;  // four chains, summed pairwise
  for (int j = 0; j < taps; ++j) {
    const long src = t + j - (taps - 1) / 2;
    if (src < 0 || src >= len) continue;
    const float* xp = x + (lo + src) * C;
    const float* wj = w + j * C;
    if ((C & 3) == 0) {
      for (int c = 0; c < C; c += 4) {
        float4 f = *reinterpret_cast<const float4*>(xp + c);
        if (lrelu) { f.x = gan_lrelu(f.x, slope); f.y = gan_lrelu(f.y, slope); f.z = gan_lrelu(f.z, slope); f.w = gan_lrelu(f.w, slope); }
        a0 = fmaf(f.x, wj[c], a0);
        a1 = fmaf(f.y, wj[c + 1], a1);
        a2 = fmaf(f.z, wj[c + 2], a2);
        a3 = fmaf(f.w, wj[c + 3], a3);
      }
    } else {
      for (int c = 0; c < C; ++c) {
        const float f = lrelu ? gan_lrelu(xp[c], slope) : xp[c];
        a0 = fmaf(f, wj[c], a0);
      }
    }
  }
  out[s][t] = tanhf(((a0 + a1) + (a2 + a3)) + (bias ? bias[0] : 0.f));
}

}  // namespace vx
