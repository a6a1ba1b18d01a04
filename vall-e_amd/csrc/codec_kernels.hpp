// EnCodec-24 kHz kernels, decoder (codes -> waveform) and encoder (waveform -> codes), fp32 storage and fp32 accumulation (the
// parity mode).
//
// Layout: time-major rows [frames * rate, C]; the rows of a ragged batch are concatenated and every kernel receives the
// segment starts (in FRAMES, seg[n] = total) plus the rows-per-frame rate of its operand, as run_stack does for the NAR rows.
// No tap and no LSTM state crosses a segment boundary.
//
//   codec_rvq_rows     x[row] = sum_q codebook_q[codes[q][row]]
//   codec_gemm_rows    every convolution but the last as a row GEMM  C[row][n] = bias[n] + sum_k A(row, k) W[n][k]  on the fp32
//                      matrix instruction (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, one rounding per product).  The operand
//                      A is gathered while it is staged: up to two parts [taps x channels], each with its own pad rule (reflect
//                      at a segment's start for the stride-1 convolutions, zero for the transposed convolution's x[t-1] tap)
//                      and an optional ELU.  A transposed convolution with k = 2 stride is this GEMM with taps {x[t-1], x[t]},
//                      N = stride * C_out: its output row t IS rows t*stride .. t*stride+stride-1 of the up-sampled signal.  The
//                      residual block's two 1x1 convolutions are one GEMM over the parts [ELU(h) ; x].
//   codec_lstm_step    one time step of the two-layer LSTM for every utterance of the batch: layer 0 at step s and layer 1 at
//                      step s - 1 (whose input half W_ih h0[s-1] is computed in the step).  One wave per hidden unit keeps the
//                      unit's four gate rows in registers and walks the utterances; finished utterances are skipped.  The decoder
//                      replays the steps as a captured linear chain of CODEC_LSTM_CHAIN launches (codec.hip).
//   codec_conv_out     the last convolution (C -> 1): one output sample per lane, bandwidth work.
//
// Encoder.  An utterance of L samples has ceil(L / 2), ceil(. / 4), ... rows per stage, so the segment starts are passed in ROWS
// per stage (rate = 1), one table per stage:
//   codec_conv_in      the first convolution (1 -> C, k = 7) over the raw samples: K = 7 is no matrix shape, one output value per lane.
//   codec_gemm_rows<.., STRIDED>  the down-sampling convolution (k = 2r, stride r) as the same row GEMM: output row t of a segment
//                      gathers input rows t r - r .. t r + r - 1 of the SAME segment of the input table (K = 2r C_in); rows before
//                      the segment mirror (reflect), rows past its end mirror too (the `extra` pad that completes the last
//                      window), a mirror image outside the segment reads the zero extension.  The residual blocks, the LSTM and
//                      the last convolution are the decoder's kernels.
//   codec_rvq_encode   the residual vector quantiser's nearest-code search, all stages in one launch (below).
//   codec_codes_out    int32 codes [n_q][rows] -> every utterance's own int64 (n_q, T_i) tensor.
//   codec_resample     windowed-sinc sample-rate conversion with the channel mean, per utterance (vx_resample; described at the kernel).
#pragma once
#include "common.hpp"

namespace vx {

constexpr int CODEC_MAX_SEG = 64;   // utterances per launch (vx_codec_config.max_batch <= 64)
constexpr int CODEC_MAX_Q = 32;     // codebooks

enum CodecPad { CODEC_PAD_REFLECT = 0, CODEC_PAD_ZERO = 1 };

__device__ __forceinline__ float codec_elu(float v) { return v > 0.f ? v : expm1f(v); }

// Segment of `row` (rows = frames * rate): lo / len in rows.  nseg <= 64: a linear scan of scalars.
__device__ __forceinline__ void codec_find_seg(const int* __restrict__ seg, int nseg, int rate, long row, long& lo, long& len) {
  int s = 0;
  while (s + 1 < nseg && (long)seg[s + 1] * rate <= row) ++s;
  lo = (long)seg[s] * rate;
  len = (long)seg[s + 1] * rate - lo;
}

// Source row of tap j (0 = oldest) of a causal k-tap window ending at local row t of a segment of `len` rows; -1 = zero.
// Reflect: index i = t + j - (k-1); i < 0 mirrors to -i; a mirror image beyond the segment's end reads the zero extension.
__device__ __forceinline__ long codec_tap_row(long t, int j, int k, long len, int pad) {
  long i = t + j - (k - 1);
  if (i >= 0) return i;
  if (pad == CODEC_PAD_ZERO) return -1;
  i = -i;
  return i < len ? i : -1;
}

// Encoder form: tap j of the k-tap window of OUTPUT row t at `stride` (left pad k - stride, reflect; right `extra` pad, reflect).
// An input not longer than the left pad is zero-extended to k - stride + 1 rows before it is mirrored (lenx below); the right
// pad is shorter than the left one (extra < stride <= k - stride), so the left pad decides the extension.
__device__ __forceinline__ long codec_tap_row_strided(long t, int j, int k, int stride, long len) {
  long i = t * stride + j - (k - stride);
  if (i < 0) {
    i = -i;
    return i < len ? i : -1;
  }
  if (i < len) return i;
  const long lenx = len > k - stride ? len : (long)(k - stride) + 1;
  if (i < lenx) return -1;
  i = 2 * (lenx - 1) - i;
  return (i >= 0 && i < len) ? i : -1;
}

struct CodecPart {
  const float* x;  // rows [*, C]
  int C, taps, pad, elu;
};

struct CodecGemmArgs {
  CodecPart part[2];
  int nparts;
  const float* W;     // [N][K] row-major, K = sum taps * C, k = tap * C + c inside a part
  const float* bias;  // [N] or null
  float* out;         // [M][N]
  long M;
  int N, K;
  const int* seg;     // nseg + 1 frame offsets (device)
  int nseg, rate;     // rows per frame of the operand rows (= of the GEMM's M rows)
  // STRIDED only (one part, pad = reflect): seg holds the OUTPUT rows' starts (rate 1), seg_in the input rows' starts
  const int* seg_in;
  int stride;
};

// BM = 32 * WM rows x BN = 32 * WN columns per workgroup of WM * WN waves (one 32x32 accumulator tile each), BK = 16.
// LDS tiles are [row][BK + 1] (odd stride: the per-lane operand reads A[l & 31][l >> 5] hit 32 different banks).
// VEC: every part's C is a multiple of 16, so a K chunk lies in one tap of one part and is loaded as float4.
template <int WM, int WN, bool VEC, bool STRIDED = false>
__global__ __launch_bounds__(WM * WN * 64) void codec_gemm_rows(const CodecGemmArgs a) {
  constexpr int BM = 32 * WM, BN = 32 * WN, BK = 16, LD = BK + 1, NT = WM * WN * 64;
  constexpr int A_V = BM * BK / 4 / NT > 0 ? BM * BK / 4 / NT : 1;   // float4 per thread of the A tile
  constexpr int B_V = BN * BK / 4 / NT > 0 ? BN * BK / 4 / NT : 1;
  __shared__ float As[BM * LD];
  __shared__ float Bs[BN * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;

  // this thread's A rows: slot v covers tile row (tid + v * NT) / 4, k quad (tid + v * NT) % 4
  // STRIDED: seg_lo / seg_len describe the INPUT segment and row_t is the output row's index inside its own segment
  long seg_lo[A_V], seg_len[A_V], row_t[A_V];
#pragma unroll
  for (int v = 0; v < A_V; ++v) {
    const int idx = tid + v * NT;
    const long row = m0 + idx / 4;
    seg_lo[v] = 0;
    seg_len[v] = 0;
    row_t[v] = 0;
    if (idx < BM * BK / 4 && row < a.M) {
      if (STRIDED) {
        int s = 0;
        while (s + 1 < a.nseg && (long)a.seg[s + 1] <= row) ++s;
        row_t[v] = row - a.seg[s];
        seg_lo[v] = a.seg_in[s];
        seg_len[v] = (long)a.seg_in[s + 1] - seg_lo[v];
      } else {
        codec_find_seg(a.seg, a.nseg, a.rate, row, seg_lo[v], seg_len[v]);
      }
    }
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
        int k = k0 + kq, p = 0;
        if (a.nparts > 1 && k >= a.part[0].taps * a.part[0].C) { k -= a.part[0].taps * a.part[0].C; p = 1; }
        const CodecPart& P = a.part[p];
        const int tap = k / P.C, c = k - tap * P.C;
        const long src = STRIDED ? codec_tap_row_strided(row_t[v], tap, P.taps, a.stride, seg_len[v])
                                 : codec_tap_row(row - seg_lo[v], tap, P.taps, seg_len[v], P.pad);
        if (k0 + kq < a.K && src >= 0) {
          const float4 f = *reinterpret_cast<const float4*>(P.x + (seg_lo[v] + src) * P.C + c);
          ra[v][0] = f.x; ra[v][1] = f.y; ra[v][2] = f.z; ra[v][3] = f.w;
          if (P.elu) {
#pragma unroll
            for (int q = 0; q < 4; ++q) ra[v][q] = codec_elu(ra[v][q]);
          }
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          int k = k0 + kq + q, p = 0;
          if (k >= a.K) continue;
          if (a.nparts > 1 && k >= a.part[0].taps * a.part[0].C) { k -= a.part[0].taps * a.part[0].C; p = 1; }
          const CodecPart& P = a.part[p];
          const int tap = k / P.C, c = k - tap * P.C;
          const long src = STRIDED ? codec_tap_row_strided(row_t[v], tap, P.taps, a.stride, seg_len[v])
                                   : codec_tap_row(row - seg_lo[v], tap, P.taps, seg_len[v], P.pad);
          if (src >= 0) {
            const float f = P.x[(seg_lo[v] + src) * P.C + c];
            ra[v][q] = P.elu ? codec_elu(f) : f;
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
  // four accumulators over interleaved k pairs, summed pairwise at the end: each is a chain of K / 4 products, which halves the
  // rounding error of one K-long chain (the instruction rounds once per product, like fmaf)
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
      if (row < a.M) a.out[row * a.N + n] = acc[r] + b;
    }
  }
}

// x[row][c] = sum_q cb[q][codes[q * rows + row]][c]; codes are the concatenated utterances, q-major per launch.
__global__ __launch_bounds__(256) void codec_rvq_rows(const int* __restrict__ codes, const float* __restrict__ cb, float* __restrict__ x,
                                                      long rows, int n_q, int size, int dim) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * dim) return;
  const long row = i / dim;
  const int c = (int)(i - row * dim);
  float s = 0.f;
  for (int q = 0; q < n_q; ++q) s += cb[((long)q * size + codes[(long)q * rows + row]) * dim + c];
  x[i] = s;
}

struct CodecLstmArgs {
  const float* gin0;   // [rows][4H] = W_ih0 x + b_ih0 + b_hh0
  const float* whh0;   // [4H][H]
  const float* w1;     // [4H][2H] = [W_ih1 | W_hh1]
  const float* b1;     // [4H] = b_ih1 + b_hh1
  const float* xin;    // [rows][H] LSTM input (skip)
  float* h0;           // [rows][H]
  float* h1;           // [rows][H]
  float* y;            // [rows][H] = h1 + xin
  float* c0;           // [nseg][H]
  float* c1;           // [nseg][H]
  const int* seg;      // nseg + 1 frame offsets
  int nseg, H, layers; // layers: 1 or 2
  const int* meta;     // null, or device {nseg, first step of this replay}: the captured chain reads both from memory, so one
                       // graph serves every batch and length
};

// Last node of the captured chain: the next replay continues n steps later.
__global__ void codec_lstm_advance(int* meta, int n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) meta[1] += n;
}

__device__ __forceinline__ float codec_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// Launch s in [0, Tmax + layers - 1): layer 0 at step s, layer 1 at step s - 1.  Grid: H / 4 workgroups per layer, 4 waves each,
// one hidden unit per wave.  KPL = H / 64 operand values per lane and gate row.
template <int KPL>
__global__ __launch_bounds__(256) void codec_lstm_step(const CodecLstmArgs a, int s) {
  const int H = KPL * 64;
  const int lane = threadIdx.x & 63;
  const int per_layer = H / 4;
  const int layer = blockIdx.x / per_layer;
  const int j = (blockIdx.x % per_layer) * 4 + (threadIdx.x >> 6);
  const int nseg = a.meta ? a.meta[0] : a.nseg;
  const int t = s + (a.meta ? a.meta[1] : 0) - layer;
  if (t < 0) return;
  {  // steps past the longest utterance (the tail of a replayed chain) leave before they load anything
    bool live = false;
    for (int b = 0; b < nseg; ++b) live = live || t < a.seg[b + 1] - a.seg[b];
    if (!live) return;
  }
  const int NK = layer ? 2 * KPL : KPL;          // values per lane of one gate row
  const int ldw = layer ? 2 * H : H;
  const float* Wm = layer ? a.w1 : a.whh0;
  float w[4][2 * KPL];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int i = 0; i < 2 * KPL; ++i) w[g][i] = i < NK ? Wm[(long)(g * H + j) * ldw + i * 64 + lane] : 0.f;
  float bias[4] = {0.f, 0.f, 0.f, 0.f};
  if (layer)
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = a.b1[g * H + j];

  for (int b = 0; b < nseg; ++b) {
    const int T = a.seg[b + 1] - a.seg[b];
    if (t >= T) continue;  // finished utterance
    const long row = (long)a.seg[b] + t;
    float v[2 * KPL];
    if (layer == 0) {
#pragma unroll
      for (int i = 0; i < KPL; ++i) v[i] = t > 0 ? a.h0[(row - 1) * H + i * 64 + lane] : 0.f;
#pragma unroll
      for (int i = KPL; i < 2 * KPL; ++i) v[i] = 0.f;
    } else {
#pragma unroll
      for (int i = 0; i < KPL; ++i) v[i] = a.h0[row * H + i * 64 + lane];
#pragma unroll
      for (int i = 0; i < KPL; ++i) v[KPL + i] = t > 0 ? a.h1[(row - 1) * H + i * 64 + lane] : 0.f;
    }
    float d[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < 2 * KPL; ++i) acc = fmaf(w[g][i], v[i], acc);
      d[g] = wave_sum(acc);
    }
    if (lane == 0) {
      float pre[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) pre[g] = d[g] + (layer ? bias[g] : a.gin0[row * 4 * H + g * H + j]);
      float* cs = (layer ? a.c1 : a.c0) + (long)b * H + j;
      const float cp = t > 0 ? *cs : 0.f;
      const float c = codec_sigmoid(pre[1]) * cp + codec_sigmoid(pre[0]) * tanhf(pre[2]);
      const float h = codec_sigmoid(pre[3]) * tanhf(c);
      *cs = c;
      if (layer == 0) {
        a.h0[row * H + j] = h;
        if (a.layers == 1) a.y[row * H + j] = h + a.xin[row * H + j];
      } else {
        a.h1[row * H + j] = h;
        a.y[row * H + j] = h + a.xin[row * H + j];
      }
    }
  }
}

// Last convolution: out[row] = bias + sum_{tap, c} ELU(x[src(row, tap)][c]) w[tap * C + c]; one output sample per lane.
__global__ __launch_bounds__(256) void codec_conv_out(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ out, long M, int C, int taps, const int* __restrict__ seg,
                                                      int nseg, int rate) {
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  long lo, len;
  codec_find_seg(seg, nseg, rate, row, lo, len);
  float acc = 0.f;
  for (int j = 0; j < taps; ++j) {
    const long src = codec_tap_row(row - lo, j, taps, len, CODEC_PAD_REFLECT);
    if (src < 0) continue;
    const float* p = x + (lo + src) * C;
    const float* wj = w + j * C;
    if ((C & 3) == 0) {
      for (int c = 0; c < C; c += 4) {
        const float4 f = *reinterpret_cast<const float4*>(p + c);
        acc = fmaf(codec_elu(f.x), wj[c], acc);
        acc = fmaf(codec_elu(f.y), wj[c + 1], acc);
        acc = fmaf(codec_elu(f.z), wj[c + 2], acc);
        acc = fmaf(codec_elu(f.w), wj[c + 3], acc);
      }
    } else {
      for (int c = 0; c < C; ++c) acc = fmaf(codec_elu(p[c]), wj[c], acc);
    }
  }
  out[row] = acc + (bias ? bias[0] : 0.f);
}

// First convolution of the encoder: out[row][o] = bias[o] + sum_j x[src(row, j)] w[o * taps + j] over the raw samples (C_in = 1);
// one output value per lane, o fastest.  seg: sample offsets of the utterances (rate 1).
__global__ __launch_bounds__(256) void codec_conv_in(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ out, long M, int Cout, int taps, const int* __restrict__ seg,
                                                     int nseg) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * Cout) return;
  const long row = i / Cout;
  const int o = (int)(i - row * Cout);
  long lo, len;
  codec_find_seg(seg, nseg, 1, row, lo, len);
  float acc = 0.f;
  for (int j = 0; j < taps; ++j) {
    const long src = codec_tap_row(row - lo, j, taps, len, CODEC_PAD_REFLECT);
    if (src >= 0) acc = fmaf(x[lo + src], w[o * taps + j], acc);
  }
  out[i] = acc + (bias ? bias[o] : 0.f);
}

// Sample-rate conversion with the mix-down folded in (in front of codec_conv_in, and behind codec_conv_out for a caller's playback
// rate).  With o = orig / gcd, n = new / gcd, output j = q n + p of an utterance reads the inputs i = q o + first[p] + k,
// k < count[p] (every i with |i - j o / n| < 6 o / base: the window is zero beyond), against coef[k][p]: tap-major, so the lanes
// of consecutive outputs read consecutive coefficients (no LDS bank conflict, coalesced from memory).  The table is built on the
// host in fp64 with the scale folded in and rounded once; it is kept in LDS when it has at most RESAMPLE_TAB entries.
// One workgroup owns tile_out <= 256 consecutive outputs of ONE utterance, one per lane: it stages their input span into LDS
// with aligned float4 loads per channel (scalar loads where a quad leaves the row), channel c added to the staged sum in order
// and the last one divided by C, so multi-channel input is never written out as mono; samples outside [0, L) are staged as
// zero, so no tap reaches another utterance.  Every lane then runs its taps in ascending i (first product, then an fmaf
// chain): the order depends neither on the grid nor on the other utterances of the call.
constexpr int RESAMPLE_SPAN = 6144;  // staged input samples per tile (the host sizes tile_out for it)
constexpr int RESAMPLE_TAB = 8192;   // coefficients held in LDS

struct ResampleArgs {
  const float* const* in;  // [nseg] (C, L) channel-major
  float* const* out;       // [nseg]
  const int* tile0;        // [nseg + 1] first tile of every utterance
  const int* len_in;       // [nseg] L
  const int* chans;        // [nseg] C
  const int* len_out;      // [nseg] ceil(n L / o)
  const float* coef;       // [T][n]
  const int* first;        // [n] offset of phase p's first tap from q o
  const int* count;        // [n] taps of phase p, 1 .. T
  int nseg, o, n, T, tile_out;
};

template <bool TAB_LDS>
__global__ __launch_bounds__(256) void codec_resample(const ResampleArgs a) {
  __shared__ float S[RESAMPLE_SPAN];
  __shared__ float Ct[TAB_LDS ? RESAMPLE_TAB : 1];
  const int tid = threadIdx.x;
  if (TAB_LDS)
    for (int i = tid; i < a.T * a.n; i += 256) Ct[i] = a.coef[i];
  const int total = a.tile0[a.nseg];
  for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {
    int s = 0;  // the utterance of the tile: the last s with tile0[s] <= tile (every utterance has a tile)
    for (int hi_s = a.nseg; hi_s - s > 1;) {
      const int mid = (s + hi_s) >> 1;
      if (a.tile0[mid] <= tile) s = mid;
      else hi_s = mid;
    }
    const float* x = a.in[s];
    const long L = a.len_in[s];
    const int C = a.chans[s], Lo = a.len_out[s];
    const int j0 = (tile - a.tile0[s]) * a.tile_out;           // < Lo
    const int j1 = (int)min((long)j0 + a.tile_out - 1, (long)Lo - 1);
    const int q0 = j0 / a.n, p0 = j0 - q0 * a.n, q1 = j1 / a.n, p1 = j1 - q1 * a.n;
    const long lo = (long)q0 * a.o + a.first[p0];              // first and one past the last input of the tile: both ends move
    const long hi = (long)q1 * a.o + a.first[p1] + a.count[p1];  // forward with j
    __syncthreads();  // the table is staged; the previous tile's reads of S are done
    for (int c = 0; c < C; ++c) {
      const float* row = x + (long)c * L;
      // quads aligned in memory: row + i4 is a multiple of 16 bytes
      const long mis = (long)((((unsigned long long)row >> 2) + (unsigned long long)lo) & 3);
      for (long i4 = lo - mis + 4L * tid; i4 < hi; i4 += 4 * 256) {
        float f[4];
        if (i4 >= 0 && i4 + 3 < L) {
          const float4 v = *reinterpret_cast<const float4*>(row + i4);
          f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) f[e] = (i4 + e >= 0 && i4 + e < L) ? row[i4 + e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long idx = i4 + e - lo;
          if (idx < 0 || idx >= hi - lo || idx >= RESAMPLE_SPAN) continue;
          const float sum = c ? S[idx] + f[e] : f[e];
          S[idx] = c == C - 1 ? sum / (float)C : sum;
        }
      }
      __syncthreads();  // the next channel's quads are aligned differently: another thread continues this sample's sum
    }
    const int j = j0 + min(tid, j1 - j0);  // no index past j1 is formed (j0 + tid could pass int32 at the longest outputs)
    if (tid <= j1 - j0) {
      const int q = j / a.n, p = j - q * a.n;
      const int cnt = a.count[p];
      const float* sp = S + ((long)q * a.o + a.first[p] - lo);
      float acc;
      if (TAB_LDS) {
        acc = sp[0] * Ct[p];
        for (int k = 1; k < cnt; ++k) acc = fmaf(sp[k], Ct[k * a.n + p], acc);
      } else {
        acc = sp[0] * a.coef[p];
        for (int k = 1; k < cnt; ++k) acc = fmaf(sp[k], a.coef[(long)k * a.n + p], acc);
      }
      a.out[s][j] = acc;
    }
  }
}

// Residual vector quantiser, encode side.  One workgroup owns CODEC_RVQ_ROWS frames and keeps their residual [32][D] in LDS over
// all n_q stages (the stages depend on each other, the frames do not).  Per stage the [32, D] x [D, S] product runs on the fp32
// matrix instruction: wave w takes the 32-code tiles w, w + 4, ...; lane half h = lane >> 5 walks k = h D / 2 .. (h + 1) D / 2 - 1
// of ITS codebook row (contiguous float4 loads from the L2-resident codebook) against the same k of the residual, two
// accumulators over alternating k.  The distance is formed as |e_j|^2 - 2 r.e_j: the |r|^2 every code of a frame shares is
// dropped, so the compared numbers are not differences of large near-equal sums (|r|^2 is the largest term as long as the
// residual is far from every code), and |e_j|^2 comes from the host in fp64, rounded once.  Arg-min is lexicographic in
// (distance, index) at every level - lane, 32-lane half, workgroup - which is the first index of the smallest distance, as
// torch.max of the negated distance gives.  Then r -= e_idx and idx goes to codes[q][row].
constexpr int CODEC_RVQ_ROWS = 32;
constexpr int CODEC_RVQ_MAX_D = 128;

__device__ __forceinline__ void codec_rvq_better(float d, int i, float& bd, int& bi) {
  if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
}

__global__ __launch_bounds__(256) void codec_rvq_encode(const float* __restrict__ emb, const float* __restrict__ cb,
                                                        const float* __restrict__ cb_sq, int* __restrict__ codes, long rows, int n_q,
                                                        int S, int D) {
  constexpr int BM = CODEC_RVQ_ROWS;
  __shared__ float Rs[BM * (CODEC_RVQ_MAX_D + 1)];
  __shared__ float best_d[4][BM];
  __shared__ int best_i[4][BM];
  __shared__ int pick[BM];
  const int LD = D + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  const long m0 = (long)blockIdx.x * BM;
  for (int i = tid; i < BM * D; i += 256) {
    const int r = i / D, c = i - r * D;
    Rs[r * LD + c] = m0 + r < rows ? emb[(m0 + r) * D + c] : 0.f;
  }
  __syncthreads();
  typedef float f32x16 __attribute__((ext_vector_type(16)));
  const int KH = D / 2;  // k values per lane half; D % 8 == 0 (checked by the host), so KH % 4 == 0
  const float* ap = Rs + col * LD + half * KH;
  for (int q = 0; q < n_q; ++q) {
    const float* E = cb + (long)q * S * D;
    const float* E2 = cb_sq + (long)q * S;
    float bd[16];
    int bi[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { bd[r] = INFINITY; bi[r] = 0x7fffffff; }
    for (int n0 = wave * 32; n0 < S; n0 += 128) {
      const int n = n0 + col;  // S % 32 == 0 (checked by the host)
      const float* ep = E + (long)n * D + half * KH;
      f32x16 acc0 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      f32x16 acc1 = acc0;
      for (int k = 0; k < KH; k += 4) {
        const float4 b = *reinterpret_cast<const float4*>(ep + k);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k], b.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k + 1], b.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k + 2], b.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k + 3], b.w, acc1, 0, 0, 0);
      }
      const float e2 = E2[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) codec_rvq_better(fmaf(-2.f, acc0[r] + acc1[r], e2), n, bd[r], bi[r]);
    }
    // D layout: column = lane & 31 (the code), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5): reduce over the 32 lanes of a half
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) {
        const float od = __shfl_xor(bd[r], off, 64);
        const int oi = __shfl_xor(bi[r], off, 64);
        codec_rvq_better(od, oi, bd[r], bi[r]);
      }
      if (col == 0) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        best_d[wave][row] = bd[r];
        best_i[wave][row] = bi[r];
      }
    }
    __syncthreads();
    if (tid < BM) {
      float d = best_d[0][tid];
      int i = best_i[0][tid];
      for (int w = 1; w < 4; ++w) codec_rvq_better(best_d[w][tid], best_i[w][tid], d, i);
      if (i < 0 || i >= S) i = 0;  // every distance NaN: any in-range index (non-finite input is not checked)
      pick[tid] = i;
      if (m0 + tid < rows) codes[(long)q * rows + m0 + tid] = i;
    }
    __syncthreads();
    for (int i = tid; i < BM * D; i += 256) {
      const int r = i / D, c = i - r * D;
      Rs[r * LD + c] -= E[(long)pick[r] * D + c];
    }
    __syncthreads();
  }
}

// codes [n_q][rows] int32 of the concatenated utterances -> out[u] (n_q, T_u) int64, seg: frame offsets.
__global__ __launch_bounds__(256) void codec_codes_out(const int* __restrict__ codes, long long* const* __restrict__ out,
                                                       const int* __restrict__ seg, int nseg, long rows, int n_q) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * n_q) return;
  const int q = (int)(i / rows);
  const long row = i - (long)q * rows;
  int s = 0;
  while (s + 1 < nseg && (long)seg[s + 1] <= row) ++s;
  const long lo = seg[s], len = (long)seg[s + 1] - lo;
  out[s][(long)q * len + (row - lo)] = codes[i];
}

}  // namespace vx
