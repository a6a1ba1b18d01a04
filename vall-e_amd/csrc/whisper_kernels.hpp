// Whisper recogniser kernels (encoder-decoder, greedy), fp32 storage and fp32 accumulation, fp64 for the logsumexp.  The definition is
// in include/vallex.h (vx_wsp_*); the host side is whisper.hip.  The encoder runs on spk_kernels.hpp's row GEMM, attention and
// LayerNorm; what is here is the part that makes it Whisper:
//
//   wsp_logmel         the log-mel front end at n_fft 400 / hop 160.  A workgroup owns WSP_TF = 32 frames of ONE utterance: it stages
//                      the windowed frames in LDS (the zero padding to the chunk and torch.stft's reflection included), multiplies
//                      them by the host-made cos / sin tables on v_mfma_f32_32x32x2_f32 (the frame is folded about its centre first,
//                      which halves the sums and their rounding error; a lane holds a bin's real and imaginary part), applies the mel
//                      table the same way, takes log10(max(., 1e-10)), stores rows [2 P][n_mels] and the tile's maximum.  A tile that lies wholly in the zero padding skips both
//                      products: they would give exactly 0, and the same log10 is taken of it.
//   wsp_logmel_finish  per utterance the maximum over its tiles in ascending order, then max(., utt_max - 8) and (. + 4) / 4 in place.
//   wsp_add_layernorm  asr_add_layernorm with the second operand's row taken modulo P: the positional table, added once.
//   wsp_embed          decoder input rows: embed_tokens[cur[u]] + embed_positions[pos[u]].
//   wsp_skinny_gemm    the token loop's GEMM (M <= 64 rows): weight streaming.  A workgroup owns WSP_SK_MT = 8 rows x `cpw` columns; the
//                      rows' activations sit in LDS a K chunk at a time, a wave owns two columns at a time and reads their weight rows
//                      as float4, a lane sums its k in ascending order and the lanes are joined by a fixed butterfly: no atomics, no
//                      split-K.  Epilogue: bias, GELU, residual add.  Also the vocabulary head.
//   wsp_decode_attn    one workgroup per (utterance, head), HD = 64, for both uses: self-attention over the cache (the step's key and
//                      value are appended by the kernel and taken from registers) and cross-attention over P encoder rows.  A thread
//                      owns the keys tid, tid + 256, ..: the K row goes straight to registers, the scores stay in LDS (at most
//                      max(P, max_target_positions) of them), so the softmax is exact rather than online; then a thread owns one
//                      output dim of a quarter of the keys (ascending), and the quarters are added in a fixed order.
//   wsp_head_reduce    one workgroup per row of logits: the two suppress lists from a byte map, the argmax (lowest index on ties),
//                      the fp64 logsumexp of the processed row, the chosen or forced token's log-probability; then the utterance's
//                      next token, position, count, finished flag and stop reason, on the device.
#pragma once
#include "spk_kernels.hpp"

namespace vx {

constexpr int WSP_NFFT = 400, WSP_HOP = 160, WSP_BINS = 201;
constexpr int WSP_TF = 32;                 // frames per workgroup of wsp_logmel
constexpr int WSP_DFT_ROWS = 224;          // 201 bins, padded to 7 tiles of 32
constexpr int WSP_FR_K = 208;              // K of the folded DFT: 2 x 104 columns (101 + 100 terms and pads)
constexpr int WSP_FR_LD = WSP_FR_K + 1;    // LDS row strides, odd: the 32 rows of an operand fall on different banks
constexpr int WSP_PW_LD = 203;
constexpr int WSP_MEL_K = 202;             // 201 bins padded to an even K
constexpr int WSP_SK_MT = 8;               // rows per workgroup of wsp_skinny_gemm
constexpr int WSP_SK_KC = 2048;            // K chunk of its LDS tile (8 x 2048 floats = 64 KiB)
constexpr int WSP_MAX_KEYS = 4096;         // scores of wsp_decode_attn in LDS

enum WspStop { WSP_STOP_NONE = 0, WSP_STOP_EOS = 1, WSP_STOP_MAX_NEW = 2, WSP_STOP_MAX_TARGET = 3 };
enum WspSuppress { WSP_SUPPRESS = 1, WSP_BEGIN_SUPPRESS = 2 };

// ---- log-mel ------------------------------------------------------------------------------------------------------------------------
struct WspMelArgs {
  const float* const* wav;  // per utterance, 16 kHz
  const int* n_samples;     // per utterance, <= chunk
  const float* window;      // [400] periodic Hann
  const float* dft_cos;     // [224][208]: row j, column k = cos(2 pi j n(k) / 400) with n(k) as the kernel folds the frame, zero pads
  const float* dft_sin;     // [224][208]: the sines
  const float* mel;         // [ceil32(n_mels)][202]: the mel table, zero padded
  float* out;               // rows [n][frames][n_mels]
  float* tile_max;          // [n][tiles]
  int frames, chunk, n_mels, tiles;  // frames = 2 P, chunk = 320 P, tiles = ceil(frames / 32)
};

// grid = (tiles, n), 256 threads.
static __global__ __launch_bounds__(256) void wsp_logmel(const WspMelArgs a) {
  typedef float f32x16 __attribute__((ext_vector_type(16)));
  __shared__ float Cf[WSP_TF * WSP_FR_LD];
  __shared__ float Sf[WSP_TF * WSP_FR_LD];
  __shared__ float Pw[WSP_TF * WSP_PW_LD];
  __shared__ float Wmax[4];
  const int u = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
  const int f0 = tile * WSP_TF;
  const int ns = a.n_samples[u];
  const float* x = a.wav[u];
  const long first = (long)f0 * WSP_HOP - WSP_NFFT / 2;  // the tile's first sample before reflection
  // every sample the tile reads is a padded zero: its first one is, and the reflection at the chunk's end lands on zeros too
  const bool zero_tile = first >= ns && (ns <= a.chunk - WSP_NFFT || (long)(f0 + WSP_TF - 1) * WSP_HOP + WSP_NFFT / 2 <= a.chunk);
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (!zero_tile) {
    auto sample = [&](long s) {  // frames past 2 P - 1 (a ragged last tile) read zeros or in-chunk samples
      if (s < 0) s = -s;
      if (s >= a.chunk) s = 2L * (a.chunk - 1) - s;
      return (s >= 0 && s < ns) ? x[s] : 0.f;
    };
    // the frame folded about its centre (the window is symmetric): c[n] = w[n] (x[n] + x[400 - n]) meets the cosines and
    // s[n] = w[n] (x[n] - x[400 - n]) the sines, n = 0 .. 200, which halves every sum; operand column k holds n = k for k < 101 and
    // n = k - 3 for 104 <= k < 205 (the two lane halves of the matrix instruction take 104 columns each), zeros elsewhere
    for (int i = tid; i < WSP_TF * WSP_FR_K; i += 256) {
      const int f = i / WSP_FR_K, k = i - f * WSP_FR_K;
      const int n = k < WSP_FR_K / 2 ? (k < 101 ? k : -1) : (k - 3 <= 200 ? k - 3 : -1);
      float c = 0.f, sn = 0.f;
      if (n >= 0) {
        const long at = first + (long)f * WSP_HOP;
        const float xa = sample(at + n);
        if (n == 0 || n == WSP_NFFT / 2) {
          c = xa * a.window[n];
        } else {
          const float xb = sample(at + WSP_NFFT - n);
          c = (xa + xb) * a.window[n];
          sn = (xa - xb) * a.window[n];
        }
      }
      Cf[f * WSP_FR_LD + k] = c;
      Sf[f * WSP_FR_LD + k] = sn;
    }
    for (int i = tid; i < WSP_TF * WSP_PW_LD; i += 256) Pw[i] = 0.f;  // the pad columns 201, 202 are operands of the mel product
    __syncthreads();
    // eight accumulators a product, summed pairwise: a chain is 13 matrix instructions long
    auto product = [&](const float* ap, const float* bp) {
      f32x16 acc[8] = {zero, zero, zero, zero, zero, zero, zero, zero};
      for (int kk = 0; kk < WSP_FR_K / 2; kk += 8) {
        const float4 b0 = *reinterpret_cast<const float4*>(bp + kk);
        const float4 b1 = *reinterpret_cast<const float4*>(bp + kk + 4);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], b0.x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk + 1], b0.y, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk + 2], b0.z, acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk + 3], b0.w, acc[3], 0, 0, 0);
        acc[4] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk + 4], b1.x, acc[4], 0, 0, 0);
        acc[5] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk + 5], b1.y, acc[5], 0, 0, 0);
        acc[6] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk + 6], b1.z, acc[6], 0, 0, 0);
        acc[7] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk + 7], b1.w, acc[7], 0, 0, 0);
      }
      return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    };
    const int aoff = (lane & 31) * WSP_FR_LD + half * (WSP_FR_K / 2);
    for (int ct = wave; ct < WSP_DFT_ROWS / 32; ct += 4) {
      const long boff = (long)(ct * 32 + (lane & 31)) * WSP_FR_K + half * (WSP_FR_K / 2);
      const f32x16 re = product(Cf + aoff, a.dft_cos + boff);
      const f32x16 im = product(Sf + aoff, a.dft_sin + boff);
      const int bin = ct * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        if (bin < WSP_BINS) Pw[row * WSP_PW_LD + bin] = re[r] * re[r] + im[r] * im[r];
      }
    }
    __syncthreads();
  }
  // mel, log10, store
  const float* pp = Pw + (lane & 31) * WSP_PW_LD + half * (WSP_MEL_K / 2);
  float mx = -INFINITY;
  for (int ct = wave; ct * 32 < a.n_mels; ct += 4) {
    f32x16 acc = zero;
    if (!zero_tile) {
      const float* mp = a.mel + (long)(ct * 32 + (lane & 31)) * WSP_MEL_K + half * (WSP_MEL_K / 2);
      f32x16 acc2[2] = {zero, zero};
      for (int kk = 0; kk + 1 < WSP_MEL_K / 2; kk += 2) {
        acc2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(pp[kk], mp[kk], acc2[0], 0, 0, 0);
        acc2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(pp[kk + 1], mp[kk + 1], acc2[1], 0, 0, 0);
      }
      acc2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(pp[WSP_MEL_K / 2 - 1], mp[WSP_MEL_K / 2 - 1], acc2[0], 0, 0, 0);  // 101 is odd
      acc = acc2[0] + acc2[1];
    }
    const int m = ct * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = f0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (m < a.n_mels && f < a.frames) {
        const float v = log10f(fmaxf(acc[r], 1e-10f));
        a.out[((long)u * a.frames + f) * a.n_mels + m] = v;
        mx = fmaxf(mx, v);
      }
    }
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) mx = fmaxf(mx, __shfl_xor(mx, w));
  if (lane == 0) Wmax[wave] = mx;
  __syncthreads();
  if (tid == 0) a.tile_max[(long)u * a.tiles + tile] = fmaxf(fmaxf(Wmax[0], Wmax[1]), fmaxf(Wmax[2], Wmax[3]));
}

// grid = (ceil(frames n_mels / 256), n): every thread takes the utterance's maximum over the tiles in ascending order.
static __global__ __launch_bounds__(256) void wsp_logmel_finish(float* __restrict__ out, const float* __restrict__ tile_max, int tiles, long per_utt) {
  const int u = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per_utt) return;
  float mx = -INFINITY;
  for (int t = 0; t < tiles; ++t) mx = fmaxf(mx, tile_max[(long)u * tiles + t]);
  float* p = out + (long)u * per_utt + i;
  *p = (fmaxf(*p, mx - 8.f) + 4.f) / 4.f;
}

// ---- residual + LayerNorm with a periodic second operand ----------------------------------------------------------------------------
// s = a[row] + b[row % bmod], stored to `sum` when it is not null (it may be `a`); y = LayerNorm(s).  One wave per row.
static __global__ __launch_bounds__(256) void wsp_add_layernorm(const float* a, const float* __restrict__ b, int bmod, const float* __restrict__ w,
                                                                const float* __restrict__ beta, float* sum, float* __restrict__ y, long M,
                                                                int d, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* ap = a + row * d;
  const float* bp = b + (row % bmod) * d;
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

// ---- the token loop -----------------------------------------------------------------------------------------------------------------
// The utterances' state on the device: nothing of it is read back per step.
struct WspState {
  int* cur;       // [n] the token the next step feeds
  int* pos;       // [n] its position in the sequence
  int* count;     // [n] tokens generated so far
  int* finished;  // [n]
};

// grid = n, 256 threads.
static __global__ __launch_bounds__(256) void wsp_embed(const float* __restrict__ tok_emb, const float* __restrict__ pos_emb, const int* __restrict__ cur,
                                                        const int* __restrict__ pos, float* __restrict__ x, int d) {
  const int u = blockIdx.x;
  const float* t = tok_emb + (long)cur[u] * d;
  const float* p = pos_emb + (long)pos[u] * d;
  for (int c = threadIdx.x; c < d; c += 256) x[(long)u * d + c] = t[c] + p[c];
}

struct WspSkinnyArgs {
  const float* x;    // [M][K]
  const float* W;    // [N][K], K a multiple of 4, rows 16-byte aligned
  const float* bias;  // [N] or null
  const float* res;  // [M][ldo] or null: added after the activation (may be `out`)
  float* out;        // [M][ldo]
  int M, N, K, ldo, act, cpw;  // cpw: columns per workgroup, a multiple of 8
};

// grid = (ceil(N / cpw), ceil(M / 8)), 256 threads.
static __global__ __launch_bounds__(256) void wsp_skinny_gemm(const WspSkinnyArgs a) {
  constexpr int MT = WSP_SK_MT, KC = WSP_SK_KC;
  extern __shared__ float wsp_sk_x[];  // [MT][min(K, KC)]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * MT, n0 = blockIdx.x * a.cpw;
  const int kc = a.K < KC ? a.K : KC;
  for (int c0 = 0; c0 < a.cpw; c0 += 8) {  // uniform over the workgroup
    const int n = n0 + c0 + 2 * wave;      // this wave's two columns
    float acc[2][MT];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[c][m] = 0.f;
    for (int k0 = 0; k0 < a.K; k0 += kc) {
      const int kn = a.K - k0 < kc ? a.K - k0 : kc;
      if (a.K > kc || c0 == 0) {  // a single chunk stays staged over the column passes
        __syncthreads();          // the previous chunk's reads are done
        for (int i = tid; i < MT * (kn / 4); i += 256) {
          const int m = i / (kn / 4), k = (i - m * (kn / 4)) * 4;
          float4 v = {0.f, 0.f, 0.f, 0.f};
          if (m0 + m < a.M) v = *reinterpret_cast<const float4*>(a.x + (long)(m0 + m) * a.K + k0 + k);
          *reinterpret_cast<float4*>(wsp_sk_x + m * kc + k) = v;
        }
        __syncthreads();
      }
      for (int k = 4 * lane; k < kn; k += 256) {
        float4 w[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          w[c] = float4{0.f, 0.f, 0.f, 0.f};
          if (n + c < a.N) w[c] = *reinterpret_cast<const float4*>(a.W + (long)(n + c) * a.K + k0 + k);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const float4 xv = *reinterpret_cast<const float4*>(wsp_sk_x + m * kc + k);
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            acc[c][m] = fmaf(xv.x, w[c].x, acc[c][m]);
            acc[c][m] = fmaf(xv.y, w[c].y, acc[c][m]);
            acc[c][m] = fmaf(xv.z, w[c].z, acc[c][m]);
            acc[c][m] = fmaf(xv.w, w[c].w, acc[c][m]);
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        float v = acc[c][m];
#pragma unroll
        for (int w_ = 32; w_ > 0; w_ >>= 1) v += __shfl_xor(v, w_);
        acc[c][m] = v;
      }
    // lane 8 c + m stores (column c, row m)
    if (lane < 2 * MT) {
      const int c = lane / MT, m = lane % MT;
      float v = 0.f;
#pragma unroll
      for (int cc = 0; cc < 2; ++cc)
#pragma unroll
        for (int mm = 0; mm < MT; ++mm)
          if (cc == c && mm == m) v = acc[cc][mm];
      if (n + c < a.N && n + c < n0 + a.cpw && m0 + m < a.M) {
        if (a.bias) v += a.bias[n + c];
        if (a.act == SPK_ACT_GELU) v = spk_gelu(v);
        const long at = (long)(m0 + m) * a.ldo + n + c;
        if (a.res) v += a.res[at];
        a.out[at] = v;
      }
    }
  }
}

struct WspAttnArgs {
  const float* q;    // [n][ldq]: head h at columns h 64
  const float* knew;  // [n][ldq] the step's key and value (self-attention), or null
  const float* vnew;
  float* kc;         // keys: utterance u's row j at kc + (u rows_per_utt + j) ld, head h at columns h 64
  float* vc;
  float* out;        // [n][d]
  const int* pos;    // self-attention: keys 0 .. pos[u] (the last one is the step's); null: `keys` of them
  int ldq, ld, d, keys;
  long rows_per_utt;
  float scale;
};

// grid = (H, n), 256 threads.
static __global__ __launch_bounds__(256) void wsp_decode_attn(const WspAttnArgs a) {
  constexpr int HD = 64;
  extern __shared__ float wsp_sc[];  // the scores, then 4 x 64 partial outputs behind them
  __shared__ float red[4];
  __shared__ float qs[HD];
  const int h = blockIdx.x, u = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.pos ? a.pos[u] + 1 : a.keys;
  float* kbase = a.kc + (long)u * a.rows_per_utt * a.ld + (long)h * HD;
  float* vbase = a.vc + (long)u * a.rows_per_utt * a.ld + (long)h * HD;
  if (a.knew && tid < HD) {  // append; the last key and value are read from the step's own rows below
    kbase[(long)(T - 1) * a.ld + tid] = a.knew[(long)u * a.ldq + h * HD + tid];
    vbase[(long)(T - 1) * a.ld + tid] = a.vnew[(long)u * a.ldq + h * HD + tid];
  }
  if (tid < HD) qs[tid] = a.q[(long)u * a.ldq + h * HD + tid];
  __syncthreads();
  float mx = -INFINITY;
  for (int j = tid; j < T; j += 256) {
    const float* kp = (a.knew && j == T - 1) ? a.knew + (long)u * a.ldq + h * HD : kbase + (long)j * a.ld;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
      const float4 kv = *reinterpret_cast<const float4*>(kp + c);
      s0 = fmaf(qs[c], kv.x, s0);
      s1 = fmaf(qs[c + 1], kv.y, s1);
      s2 = fmaf(qs[c + 2], kv.z, s2);
      s3 = fmaf(qs[c + 3], kv.w, s3);
    }
    const float s = ((s0 + s1) + (s2 + s3)) * a.scale;
    wsp_sc[j] = s;
    mx = fmaxf(mx, s);
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) mx = fmaxf(mx, __shfl_xor(mx, w));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int j = tid; j < T; j += 256) {
    const float p = expf(wsp_sc[j] - mx);
    wsp_sc[j] = p;
    sum += p;
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) sum += __shfl_xor(sum, w);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  const float inv = 1.f / ((red[0] + red[1]) + (red[2] + red[3]));
  // wave w owns the keys of quarter w in ascending order, lane = output dim: a V row is one coalesced read
  const int per = (T + 3) / 4, j0 = wave * per, j1 = (j0 + per < T) ? j0 + per : T;
  float o = 0.f;
  for (int j = j0; j < j1; ++j) {
    const float v = (a.vnew && j == T - 1) ? a.vnew[(long)u * a.ldq + h * HD + lane] : vbase[(long)j * a.ld + lane];
    o = fmaf(wsp_sc[j], v, o);
  }
  float* part = wsp_sc + T;
  part[wave * HD + lane] = o;
  __syncthreads();
  if (tid < HD) a.out[(long)u * a.d + h * HD + tid] = ((part[tid] + part[HD + tid]) + (part[2 * HD + tid] + part[3 * HD + tid])) * inv;
}

struct WspHeadArgs {
  const float* logits;           // [n][V]
  const unsigned char* suppress;  // [V] WSP_SUPPRESS | WSP_BEGIN_SUPPRESS
  const int* prompt;             // [n][prompt_stride]
  const int* n_prompt;           // [n]
  const int* max_new;            // [n]
  const int* forced;             // [n][out_stride] or null
  WspState st;
  int* tokens_out;               // [n][out_stride]
  float* logprob_out;            // [n][out_stride]
  int* count_out;                // [n]
  int* stop_out;                 // [n]
  float* tap;                    // [max_target][MB][V] or null: the raw row of every generated step, at its position
  int V, prompt_stride, out_stride, eos, max_target, MB;
};

// grid = n, 256 threads.  The utterance's step: pos[u] is the position the logits belong to.
static __global__ __launch_bounds__(256) void wsp_head_reduce(const WspHeadArgs a) {
  __shared__ float Bv[256];
  __shared__ int Bi[256];
  __shared__ double Sd[256];
  __shared__ int S0[2];
  const int u = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {  // read once: thread 0 rewrites both at the end
    S0[0] = a.st.finished[u];
    S0[1] = a.st.pos[u];
  }
  __syncthreads();
  if (S0[0]) return;  // uniform: a stopped utterance's later steps change nothing
  const int pos = S0[1], np = a.n_prompt[u];
  if (pos + 1 < np) {  // still inside the prompt: feed its next token
    if (tid == 0) {
      a.st.cur[u] = a.prompt[(long)u * a.prompt_stride + pos + 1];
      a.st.pos[u] = pos + 1;
    }
    return;
  }
  const int g = pos + 1 - np;  // the generated step
  const unsigned char mask = g == 0 ? (WSP_SUPPRESS | WSP_BEGIN_SUPPRESS) : WSP_SUPPRESS;
  const float* x = a.logits + (long)u * a.V;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = tid; c < a.V; c += 256) {  // ascending c: a later equal value does not replace an earlier one
    const float v = (a.suppress[c] & mask) ? -INFINITY : x[c];
    if (a.tap) a.tap[((long)pos * a.MB + u) * a.V + c] = x[c];
    if (v > best || bi == 0x7fffffff) {
      best = v;
      bi = c;
    }
  }
  Bv[tid] = best;
  Bi[tid] = bi;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      const float ov = Bv[tid + w];
      const int oi = Bi[tid + w];
      if (ov > Bv[tid] || (ov == Bv[tid] && oi < Bi[tid])) { Bv[tid] = ov; Bi[tid] = oi; }
    }
    __syncthreads();
  }
  const float top = Bv[0];
  const int arg = Bi[0];
  double s = 0.0;
  for (int c = tid; c < a.V; c += 256)
    if (!(a.suppress[c] & mask)) s += exp((double)x[c] - (double)top);
  Sd[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) Sd[tid] += Sd[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const int tok = a.forced ? a.forced[(long)u * a.out_stride + g] : arg;
    const double xv = (a.suppress[tok] & mask) ? -INFINITY : (double)x[tok];
    a.tokens_out[(long)u * a.out_stride + g] = tok;
    a.logprob_out[(long)u * a.out_stride + g] = (float)(xv - (double)top - log(Sd[0]));
    a.count_out[u] = g + 1;
    a.st.count[u] = g + 1;
    int stop = WSP_STOP_NONE;
    if (!a.forced && tok == a.eos) stop = WSP_STOP_EOS;
    else if (g + 1 >= a.max_new[u]) stop = WSP_STOP_MAX_NEW;
    else if (pos + 2 >= a.max_target) stop = WSP_STOP_MAX_TARGET;  // the sequence, this token included, fills the positions
    a.stop_out[u] = stop;
    if (stop != WSP_STOP_NONE) {
      a.st.finished[u] = 1;
    } else {
      a.st.cur[u] = tok;
      a.st.pos[u] = pos + 1;
    }
  }
}

// grid = 1, n threads (n <= 64): the state of a call.
static __global__ void wsp_init_state(WspState st, const int* __restrict__ prompt, int prompt_stride, int* __restrict__ count_out, int* __restrict__ stop_out, int n) {
  const int u = threadIdx.x;
  if (u >= n) return;
  st.cur[u] = prompt[(long)u * prompt_stride];
  st.pos[u] = 0;
  st.count[u] = 0;
  st.finished[u] = 0;
  count_out[u] = 0;
  stop_out[u] = WSP_STOP_NONE;
}

}  // namespace vx
