// Speaker encoder kernels (WavLM / Wav2Vec2 x-vector network, 16 kHz waveform -> embedding), fp32 storage and fp32 accumulation,
// fp64 wherever a whole utterance is reduced.  The definition is in include/vallex.h (vx_spk_*); the host side is spk.hip.
//
// Layout: time-major rows [frames, C]; the utterances of a call are concatenated.  Every stage has a segment table of its own
// (nseg + 1 row offsets, seg[nseg] = total): the strided convolutions and the TDNN shorten every utterance by a different amount.
// No tap, no pad, no statistic and no key crosses a segment boundary, and every tile starts at its utterance's row 0, so an
// utterance's bits do not depend on its neighbours.
//
//   spk_wave_stats    optional input normalisation: per utterance sum and sum of squares in fp64 (one workgroup per utterance,
//                     lane-strided partial sums, a fixed tree), giving mean and 1 / sqrt(var + 1e-7).
//   spk_conv0_stats   layer 0 (1 -> C over k taps, stride s) is a bandwidth kernel: a workgroup owns SPK_C0_TT frames x 64 channels
//                     of ONE utterance, stages its samples in LDS and forms every output once; phase 1 keeps only fp64 sums.
//   spk_conv0_reduce  the tiles' partial sums added in ascending tile order -> mean and 1 / sqrt(var + eps) per (utterance, channel).
//   spk_conv0_apply   phase 2 recomputes the convolution (the pre-norm activations are never stored: they would be the largest
//                     tensor of the network), applies GroupNorm's affine and the exact GELU, writes rows [T0][C].
//   spk_gemm_rows     every other convolution and every Linear as a row GEMM on v_mfma_f32_32x32x2_f32 (the tile structure of
//                     gan_gemm_rows: 32x32 accumulator per wave, BK = 16, four accumulators over interleaved k pairs): operand
//                     k = tap * C + c of local output row t is input row t * stride + off0 + tap * step of the same utterance,
//                     zero outside it.  blockIdx.z is the group of a grouped convolution.  Epilogue: bias, GELU / ReLU.
//   spk_gate          WavLM's gate per (row, head) from the layer input's head slice.
//   spk_attention     softmax(q k / sqrt(hd) + gate[i] bias[h][j - i]) v with online softmax over key tiles of 32, both products on
//                     the fp32 matrix instruction; a null table is the plain mode.
//   spk_layernorm     LayerNorm(a + b) with the optional running weighted layer sum folded in (first layer stores, later add).
//   spk_pool          mean and unbiased standard deviation over an utterance's frames, fp64, frames in ascending order.
//   spk_cosine        cosine of pairs of embeddings, fp64 sums in a fixed order.
//
// Two translation units include this header (spk.hip, and asr.hip through asr_kernels.hpp), so every kernel is `static`: each unit
// carries and launches its own copy and the library has no duplicate host symbol.
#pragma once
#include "common.hpp"

namespace vx {

constexpr int SPK_MAX_SEG = 64;   // utterances per call (vx_spk_config.max_batch <= 64)
constexpr int SPK_C0_TT = 256;    // frames per workgroup of the layer-0 kernels
constexpr int SPK_C0_MAXK = 32;   // taps of layer 0 served
constexpr int SPK_ATT_WAVES = 4;  // 32 query rows per wave

enum SpkAct { SPK_ACT_NONE = 0, SPK_ACT_GELU = 1, SPK_ACT_RELU = 2 };

__device__ __forceinline__ float spk_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

// Segment of global row `row`: index; lo = its first row, len = its rows.  nseg <= 64: a linear scan.
__device__ __forceinline__ int spk_find_seg(const int* __restrict__ seg, int nseg, long row, long& lo, long& len) {
  int s = 0;
  while (s + 1 < nseg && (long)seg[s + 1] <= row) ++s;
  lo = seg[s];
  len = (long)seg[s + 1] - lo;
  return s;
}

// Tile `tile` of a launch whose tiles are counted per segment (TT rows each): the segment, or nseg when past the last tile.
__device__ __forceinline__ int spk_find_tile(const int* __restrict__ seg, int nseg, int TT, long tile, long& lo, long& len, long& t0) {
  int s = 0;
  for (; s < nseg; ++s) {
    lo = seg[s];
    len = (long)seg[s + 1] - lo;
    const long nt = (len + TT - 1) / TT;
    if (tile < nt) break;
    tile -= nt;
  }
  t0 = tile * TT;
  return s;
}

// ---- input normalisation -----------------------------------------------------------------------------------------------------
// stats[2 u] = mean, stats[2 u + 1] = 1 / sqrt(var + 1e-7), biased variance.  One workgroup of 256 per utterance.
static __global__ __launch_bounds__(256) void spk_wave_stats(const float* const* __restrict__ wav, const int* __restrict__ n_samples,
                                                      float* __restrict__ stats) {
  __shared__ double S[256], Q[256];
  const int u = blockIdx.x, tid = threadIdx.x;
  const float* x = wav[u];
  const int L = n_samples[u];
  double s = 0.0, q = 0.0;
  for (int i = tid; i < L; i += 256) {
    const double v = x[i];
    s += v;
    q += v * v;
  }
  S[tid] = s;
  Q[tid] = q;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      S[tid] += S[tid + w];
      Q[tid] += Q[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double m = S[0] / L, var = fmax(Q[0] / L - m * m, 0.0);
    stats[2 * u] = (float)m;
    stats[2 * u + 1] = (float)(1.0 / sqrt(var + 1e-7));
  }
}

// ---- layer 0 -----------------------------------------------------------------------------------------------------------------
struct SpkConv0Args {
  const float* const* wav;  // per utterance
  const float* nstats;      // [2 nseg] mean, rstd of the input normalisation, or null
  const float* w;           // [C][k]
  const float* bias;        // [C] or null
  const float* gn_w;        // [C]
  const float* gn_b;        // [C]
  double* partial;          // [tiles][C][2]
  float* cstats;            // [nseg][C][2] mean, rstd
  float* out;               // rows [T0 total][C]
  const int* seg;           // layer-0 output rows
  int nseg, C, k, stride;
  float eps;
};

// The tile's samples in LDS and this thread's channel weights; v(t) is the convolution output of local frame t0 + t.
// grid.x >= the tiles of the call (ceil(len / TT) per segment), grid.y = ceil(C / 64); 256 threads = 64 channels x 4 frame groups.
template <bool APPLY>
static __global__ __launch_bounds__(256) void spk_conv0(const SpkConv0Args a) {
  constexpr int TT = SPK_C0_TT;
  extern __shared__ float X[];  // (TT - 1) stride + k samples
  __shared__ double R[2][4][64];
  long lo, len, t0;
  const int s = spk_find_tile(a.seg, a.nseg, TT, blockIdx.x, lo, len, t0);
  if (s == a.nseg) return;  // uniform over the workgroup
  const int tt = len - t0 < TT ? (int)(len - t0) : TT;
  const int tid = threadIdx.x, cl = tid & 63, r0 = tid >> 6;
  const int c = blockIdx.y * 64 + cl;
  const bool live = c < a.C;
  const float* x = a.wav[s] + t0 * a.stride;
  const int ns = (tt - 1) * a.stride + a.k;  // inside the utterance by the definition of its frame count
  const float nm = a.nstats ? a.nstats[2 * s] : 0.f, nr = a.nstats ? a.nstats[2 * s + 1] : 1.f;
  for (int i = tid; i < ns; i += 256) X[i] = a.nstats ? (x[i] - nm) * nr : x[i];
  float w[SPK_C0_MAXK];
#pragma unroll
  for (int j = 0; j < SPK_C0_MAXK; ++j) w[j] = (live && j < a.k) ? a.w[c * a.k + j] : 0.f;
  const float b = (live && a.bias) ? a.bias[c] : 0.f;
  float mean = 0.f, rstd = 0.f, gw = 0.f, gb = 0.f;
  if (APPLY && live) {
    mean = a.cstats[((long)s * a.C + c) * 2];
    rstd = a.cstats[((long)s * a.C + c) * 2 + 1];
    gw = a.gn_w[c];
    gb = a.gn_b[c];
  }
  __syncthreads();
  double sum = 0.0, sq = 0.0;
  for (int t = r0; t < tt; t += 4) {
    const float* xp = X + t * a.stride;
    float v = b;
#pragma unroll
    for (int j = 0; j < SPK_C0_MAXK; ++j)
      if (j < a.k) v = fmaf(xp[j], w[j], v);
    if (APPLY) {
      if (live) a.out[(lo + t0 + t) * a.C + c] = spk_gelu((v - mean) * rstd * gw + gb);
    } else {
      sum += (double)v;
      sq += (double)v * (double)v;
    }
  }
  if (!APPLY) {
    R[0][r0][cl] = sum;
    R[1][r0][cl] = sq;
    __syncthreads();
    if (r0 == 0 && live) {
      double* p = a.partial + ((long)blockIdx.x * a.C + c) * 2;
      p[0] = (R[0][0][cl] + R[0][1][cl]) + (R[0][2][cl] + R[0][3][cl]);
      p[1] = (R[1][0][cl] + R[1][1][cl]) + (R[1][2][cl] + R[1][3][cl]);
    }
  }
}

// One thread per (utterance, channel): the utterance's tiles in ascending order.  grid = (ceil(C / 256), nseg).
static __global__ __launch_bounds__(256) void spk_conv0_reduce(const SpkConv0Args a) {
  const int c = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (c >= a.C) return;
  long first = 0;
  for (int i = 0; i < s; ++i) first += ((long)a.seg[i + 1] - a.seg[i] + SPK_C0_TT - 1) / SPK_C0_TT;
  const long len = (long)a.seg[s + 1] - a.seg[s], nt = (len + SPK_C0_TT - 1) / SPK_C0_TT;
  double sum = 0.0, sq = 0.0;
  for (long t = 0; t < nt; ++t) {
    const double* p = a.partial + ((first + t) * a.C + c) * 2;
    sum += p[0];
    sq += p[1];
  }
  const double m = sum / (double)len, var = fmax(sq / (double)len - m * m, 0.0);
  a.cstats[((long)s * a.C + c) * 2] = (float)m;
  a.cstats[((long)s * a.C + c) * 2 + 1] = (float)(1.0 / sqrt(var + (double)a.eps));
}

// ---- row GEMM ----------------------------------------------------------------------------------------------------------------
struct SpkGemmArgs {
  const float* x;      // input rows [*, ldx]
  int ldx, xoff, xgs;  // group g reads columns xoff + g * xgs + c
  int C, taps;         // K = taps * C, k = tap * C + c
  int stride, off0, step;  // tap j of local output row t reads local input row t * stride + off0 + j * step, zero outside [0, len_in)
  const float* W;      // [groups][N][K] row-major
  const float* bias;   // [groups][N] or null
  float* out;          // [M][ldo]: group g writes columns g * N + n
  int ldo, act;
  long M;
  int N, K;
  const int* seg_out;  // nseg + 1 output row offsets, or null: one flat segment, input row = output row
  const int* seg_in;   // nseg + 1 input row offsets
  int nseg;
};

// BM = 32 * WM rows x BN = 32 * WN columns per workgroup of WM * WN waves, BK = 16; LDS tiles [row][BK + 1].
// VEC: C, ldx, xoff and xgs are multiples of 4 and C of 16, so a K chunk lies in one tap and loads as float4.
template <int WM, int WN, bool VEC>
static __global__ __launch_bounds__(WM * WN * 64) void spk_gemm_rows(const SpkGemmArgs a) {
  constexpr int BM = 32 * WM, BN = 32 * WN, BK = 16, LD = BK + 1, NT = WM * WN * 64;
  constexpr int A_V = BM * BK / 4 / NT > 0 ? BM * BK / 4 / NT : 1;
  constexpr int B_V = BN * BK / 4 / NT > 0 ? BN * BK / 4 / NT : 1;
  __shared__ float As[BM * LD];
  __shared__ float Bs[BN * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN, g = blockIdx.z;
  const float* Wg = a.W + (long)g * a.N * a.K;
  const int xcol = a.xoff + g * a.xgs;

  // this thread's A rows: the first input row of tap 0 (relative to the input segment) and the input segment
  long in_lo[A_V], in_len[A_V], src0[A_V];
#pragma unroll
  for (int v = 0; v < A_V; ++v) {
    const int idx = tid + v * NT;
    const long row = m0 + idx / 4;
    in_lo[v] = 0; in_len[v] = 0; src0[v] = 0;
    if (idx < BM * BK / 4 && row < a.M) {
      if (a.seg_out) {
        long lo, len;
        const int s = spk_find_seg(a.seg_out, a.nseg, row, lo, len);
        in_lo[v] = a.seg_in[s];
        in_len[v] = (long)a.seg_in[s + 1] - in_lo[v];
        src0[v] = (row - lo) * a.stride + a.off0;
      } else {
        in_len[v] = a.M;
        src0[v] = row;
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
        const int k = k0 + kq;
        const int tap = k / a.C, c = k - tap * a.C;
        const long src = src0[v] + (long)tap * a.step;
        if (k < a.K && src >= 0 && src < in_len[v]) {
          const float4 f = *reinterpret_cast<const float4*>(a.x + (in_lo[v] + src) * a.ldx + xcol + c);
          ra[v][0] = f.x; ra[v][1] = f.y; ra[v][2] = f.z; ra[v][3] = f.w;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = k0 + kq + q;
          if (k >= a.K) continue;
          const int tap = k / a.C, c = k - tap * a.C;
          const long src = src0[v] + (long)tap * a.step;
          if (src >= 0 && src < in_len[v]) ra[v][q] = a.x[(in_lo[v] + src) * a.ldx + xcol + c];
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
      const float* w = Wg + (long)n * a.K + k;
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
  // four accumulators over interleaved k pairs, summed pairwise at the end: each is a chain of K / 4 products
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
    const float b = a.bias ? a.bias[(long)g * a.N + n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row >= a.M) continue;
      float v = acc[r] + b;
      if (a.act == SPK_ACT_GELU) v = spk_gelu(v);
      else if (a.act == SPK_ACT_RELU) v = fmaxf(v, 0.f);
      a.out[row * a.ldo + (long)g * a.N + n] = v;
    }
  }
}

// ---- gate --------------------------------------------------------------------------------------------------------------------
// gate[row][h] = a (b const_h - 1) + 2, a = sigmoid(sum p[0:4]), b = sigmoid(sum p[4:8]), p = Wg x[row][h hd : (h + 1) hd] + bg.
// One thread per (row, head).
static __global__ __launch_bounds__(256) void spk_gate(const float* __restrict__ x, const float* __restrict__ Wg, const float* __restrict__ bg,
                                                const float* __restrict__ cst, float* __restrict__ gate, long M, int H, int hd) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * H) return;
  const int h = (int)(i % H);
  const float* xp = x + (i / H) * ((long)H * hd) + (long)h * hd;
  float p[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;  // four chains, summed pairwise (hd is a multiple of 16)
    for (int c = 0; c < hd; c += 4) {
      s0 = fmaf(xp[c], Wg[o * hd + c], s0);
      s1 = fmaf(xp[c + 1], Wg[o * hd + c + 1], s1);
      s2 = fmaf(xp[c + 2], Wg[o * hd + c + 2], s2);
      s3 = fmaf(xp[c + 3], Wg[o * hd + c + 3], s3);
    }
    p[o] = ((s0 + s1) + (s2 + s3)) + bg[o];
  }
  const float sa = ((p[0] + p[1]) + p[2]) + p[3], sb = ((p[4] + p[5]) + p[6]) + p[7];
  const float ga = 1.f / (1.f + expf(-sa)), gb = 1.f / (1.f + expf(-sb));
  gate[i] = ga * (gb * cst[h] - 1.f) + 2.f;
}

// ---- attention ---------------------------------------------------------------------------------------------------------------
struct SpkAttnArgs {
  const float* qkv;    // rows [M][3 d]: q | k | v, head h at columns h hd
  const float* gate;   // [M][H] or null with the table
  const float* table;  // [H][2 Tmax - 1]: bias of relative position r = j - i at r + Tmax - 1; null: the plain mode
  float* out;          // rows [M][d]
  const int* seg;
  int nseg, H, d, Tmax;
  float scale;
};

// A workgroup of 4 waves owns 128 query rows of one (utterance, head); a wave owns 32 of them.  Per key tile of 32, staged in LDS
// by the whole workgroup:  S^T = K Q^T (keys on the accumulator's rows, the query on the lane), online softmax in registers
// (16 keys per lane half, the halves joined by one exchange), then O^T += V^T P^T with the score registers as the B operand as they
// lie: register r of lane half h is key (r & 3) + 8 (r >> 2) + 4 h, so the A operand of that step is V[that key][dim = lane & 31].
// grid = (query tiles counted per segment, H).
template <int HD>
static __global__ __launch_bounds__(SPK_ATT_WAVES * 64) void spk_attention(const SpkAttnArgs a) {
  constexpr int QT = 32 * SPK_ATT_WAVES, KT = 32, LDK = HD + 1, DB = (HD + 31) / 32, LDV = 32 * DB + 1;
  typedef float f32x16 __attribute__((ext_vector_type(16)));
  __shared__ float Ks[KT * LDK];
  __shared__ float Vs[KT * LDV];
  long lo, T, t0;
  const int s = spk_find_tile(a.seg, a.nseg, QT, blockIdx.x, lo, T, t0);
  if (s == a.nseg) return;  // uniform over the workgroup
  const int h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
  const long ld = 3L * a.d;
  const long qi = t0 + wave * 32 + (lane & 31);  // this lane's query (local); rows past T compute on row T - 1 and are not stored
  const long qrow = lo + (qi < T ? qi : T - 1);
  float q[HD / 2];
#pragma unroll
  for (int kk = 0; kk < HD / 2; ++kk) q[kk] = a.qkv[qrow * ld + (long)h * HD + 2 * kk + half];
  const float g = a.table ? a.gate[qrow * a.H + h] : 0.f;
  const float* tab = a.table ? a.table + (long)h * (2 * a.Tmax - 1) + (a.Tmax - 1) - (qi < T ? qi : T - 1) : nullptr;

  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 o[DB];
#pragma unroll
  for (int b = 0; b < DB; ++b) o[b] = zero;
  float m = -INFINITY, l = 0.f;

  for (long k0 = 0; k0 < T; k0 += KT) {
    __syncthreads();  // the previous tile's operand reads are done
    for (int i = tid; i < KT * HD; i += SPK_ATT_WAVES * 64) {
      const int kr = i / HD, c = i - kr * HD;
      const bool in = k0 + kr < T;
      const float* p = a.qkv + (lo + k0 + kr) * ld + (long)h * HD + c;
      Ks[kr * LDK + c] = in ? p[a.d] : 0.f;
      Vs[kr * LDV + c] = in ? p[2 * a.d] : 0.f;
    }
    if (HD < 32 * DB)
      for (int i = tid; i < KT * (32 * DB - HD); i += SPK_ATT_WAVES * 64) {
        const int kr = i / (32 * DB - HD), c = HD + i % (32 * DB - HD);
        Vs[kr * LDV + c] = 0.f;
      }
    __syncthreads();
    f32x16 sc = zero;
    const float* kp = Ks + (lane & 31) * LDK + half;
#pragma unroll
    for (int kk = 0; kk < HD / 2; ++kk) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[2 * kk], q[kk], sc, 0, 0, 0);
    float p[16], mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long j = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      float v = sc[r] * a.scale;
      if (tab && j < T) v = fmaf(g, tab[j], v);
      p[r] = j < T ? v : -INFINITY;
      mx = fmaxf(mx, p[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);  // finite: key k0 is inside the utterance
    const float alpha = expf(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      p[r] = expf(p[r] - mn);
      ps += p[r];
    }
    ps += __shfl_xor(ps, 32);
    l = fmaf(l, alpha, ps);
    m = mn;
#pragma unroll
    for (int b = 0; b < DB; ++b) {
#pragma unroll
      for (int r = 0; r < 16; ++r) o[b][r] *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = (r & 3) + 8 * (r >> 2) + 4 * half;
        o[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key * LDV + 32 * b + (lane & 31)], p[r], o[b], 0, 0, 0);
      }
    }
  }
  if (qi < T) {
    const float inv = 1.f / l;
#pragma unroll
    for (int b = 0; b < DB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int dd = 32 * b + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (dd < HD) a.out[(lo + qi) * a.d + (long)h * HD + dd] = o[b][r] * inv;
      }
  }
}

// ---- LayerNorm ---------------------------------------------------------------------------------------------------------------
// y = LayerNorm(a + b) (b may be null); with `sum`: sum = (first ? 0 : sum) + lw * y, and with lw0_src != null the layer-0 term
// is not needed here (the host runs the first fold on hidden state 0).  One wave per row; the row is read twice (mean, then the
// squared deviations); the lanes' strided partial sums are joined by a fixed butterfly.
static __global__ __launch_bounds__(256) void spk_layernorm(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ w,
                                                     const float* __restrict__ beta, float* __restrict__ y, float* __restrict__ sum,
                                                     float lw, int first, long M, int d, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* ap = a + row * d;
  const float* bp = b ? b + row * d : nullptr;
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += bp ? ap[c] + bp[c] : ap[c];
#pragma unroll
  for (int w_ = 32; w_ > 0; w_ >>= 1) s += __shfl_xor(s, w_);
  const float mean = s / d;
  float q = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float v = (bp ? ap[c] + bp[c] : ap[c]) - mean;
    q = fmaf(v, v, q);
  }
#pragma unroll
  for (int w_ = 32; w_ > 0; w_ >>= 1) q += __shfl_xor(q, w_);
  const float rstd = 1.f / sqrtf(q / d + eps);
  for (int c = lane; c < d; c += 64) {
    const float v = ((bp ? ap[c] + bp[c] : ap[c]) - mean) * rstd * w[c] + beta[c];
    y[row * d + c] = v;
    if (sum) sum[row * d + c] = first ? lw * v : fmaf(lw, v, sum[row * d + c]);
  }
}

// ---- statistics pooling ------------------------------------------------------------------------------------------------------
// pooled[u][c] = mean, pooled[u][C + c] = unbiased standard deviation over the utterance's rows, fp64, rows in ascending order.
// grid = (ceil(C / 256), nseg).
static __global__ __launch_bounds__(256) void spk_pool(const float* __restrict__ x, float* __restrict__ pooled, const int* __restrict__ seg, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y;
  if (c >= C) return;
  const long lo = seg[u], n = (long)seg[u + 1] - lo;
  double s = 0.0;
  for (long t = 0; t < n; ++t) s += (double)x[(lo + t) * C + c];
  const double mean = s / (double)n;
  double q = 0.0;
  for (long t = 0; t < n; ++t) {
    const double v = (double)x[(lo + t) * C + c] - mean;
    q += v * v;
  }
  pooled[(long)u * 2 * C + c] = (float)mean;
  pooled[(long)u * 2 * C + C + c] = (float)sqrt(q / (double)(n - 1));
}

// ---- cosine ------------------------------------------------------------------------------------------------------------------
// out[p] = a_p . b_p / max(|a_p| |b_p|, 1e-8); one wave per pair, lane-strided fp64 sums joined by a fixed butterfly.
static __global__ __launch_bounds__(64) void spk_cosine(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int dim) {
  const long p = blockIdx.x;
  const int lane = threadIdx.x;
  double ab = 0.0, aa = 0.0, bb = 0.0;
  for (int c = lane; c < dim; c += 64) {
    const double x = a[p * dim + c], y = b[p * dim + c];
    ab += x * y;
    aa += x * x;
    bb += y * y;
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    ab += __shfl_xor(ab, w);
    aa += __shfl_xor(aa, w);
    bb += __shfl_xor(bb, w);
  }
  if (lane == 0) out[p] = (float)(ab / fmax(sqrt(aa) * sqrt(bb), 1e-8));
}

}  // namespace vx
