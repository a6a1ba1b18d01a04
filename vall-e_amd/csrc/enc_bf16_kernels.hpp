// The bf16 encoder mode of the recognisers (VX_WSP_ENC_BF16 / VX_ASR_ENC_BF16): the pre-norm encoder layers on the bf16 matrix
// cores.  The definition is in include/vallex.h; the host side is w2v_host.hpp (run_prenorm_layers_bf16) and the fp32 kernels of
// spk_kernels.hpp / asr_kernels.hpp / whisper_kernels.hpp are not touched: without the flag nothing of this header is launched.
//
//   ebf_gemm            C (M, N) = A (M, K) . W (N, K)^T on bf16 operands, fp32 accumulation, v_mfma_f32_32x32x16_bf16.  Three
//                       epilogues: bias -> bf16, bias + exact (erf) GELU -> bf16, bias + fp32 residual -> fp32.  A 128 x 128 tile per
//                       workgroup of four waves (2 x 2, 64 x 64 each), K in steps of 64 through one LDS stage; the next step's
//                       operands are in flight in registers while the current one is multiplied.  The sum over k has two levels
//                       (256 of k at a time into a second accumulator).  Any M (rows past M are clamped on
//                       the load and never stored), N a multiple of 8 (a tile's columns past N likewise), K a multiple of 64.  Every
//                       output element sums its k in one fixed order whatever M is: a row is bitwise what it is in any other batch.
//   ebf_add_layernorm   asr_add_layernorm / wsp_add_layernorm with the normed rows stored in bf16: s = a[row] + b[row or row % bmod]
//                       (b may be null) in fp32, stored to `sum` when that is not null; y = bf16(LayerNorm(s)), the statistics and
//                       the normalisation in fp64.  One wave per row.
//   ebf_attention       softmax(q k^T / 8) v over each segment's own rows at head_dim 64, segments of any length packed tightly.  A
//                       workgroup owns 128 query rows of one segment and one head, a wave 32 of them; keys and values go through
//                       LDS 64 at a time, the values transposed on the way in so that both products read k-contiguous fragments.
//                       S^T = K Q^T leaves a query on the lane and its keys in the registers, so the online softmax needs one
//                       exchange between the lane halves and P^T is the B operand of O^T = V^T P^T as it stands (the k order of
//                       that step is the accumulator's row order, and the V^T fragment is read in the same order).  The statistics
//                       (running maximum, sum of the unrounded probabilities) are fp32; the probabilities are rounded to bf16
//                       unnormalised, the output is divided by the sum (a true division) and rounded once.  Tiles are counted from
//                       the segment's first row: a segment is bitwise what it is alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include "spk_kernels.hpp"

namespace vx {

typedef __bf16 ebf_t;
typedef __bf16 ebf8_t __attribute__((ext_vector_type(8)));
typedef __bf16 ebf4_t __attribute__((ext_vector_type(4)));
typedef float ebf_acc_t __attribute__((ext_vector_type(16)));
typedef unsigned int ebf_u4_t __attribute__((ext_vector_type(4)));  // 16 bytes in flight (native vectors stay in registers)
typedef unsigned int ebf_u2_t __attribute__((ext_vector_type(2)));

enum EbfEpi { EBF_EPI_BF16 = 0, EBF_EPI_GELU_BF16 = 1, EBF_EPI_RESID_F32 = 2 };

constexpr int EBF_BM = 128, EBF_BN = 128, EBF_BK = 64;
constexpr int EBF_LD = EBF_BK + 8;  // elements per LDS row: 144 bytes, every 16-byte chunk stays aligned
constexpr int EBF_QT = 128;         // query rows per workgroup of ebf_attention
constexpr int EBF_KT = 64;          // keys per step

struct EbfGemmArgs {
  const ebf_t* A;     // (M, K)
  const ebf_t* W;     // (N, K)
  const float* bias;  // (N)
  const float* res;   // (M, N) fp32, EBF_EPI_RESID_F32 only; may be `out`
  void* out;          // (M, N) bf16, or fp32 with EBF_EPI_RESID_F32
  long M;
  int N, K;
};

// grid (ceil(N / 128), ceil(M / 128)), 256 threads.
template <int EPI>
static __global__ __launch_bounds__(256) void ebf_gemm(const EbfGemmArgs a) {
  constexpr int LD = EBF_LD;
  constexpr int LDT = EBF_BN + 8;  // the bf16 output tile's row stride
  static_assert(EBF_BM * LDT <= 2 * EBF_BM * LD, "the output tile reuses the operand stage");
  __shared__ __attribute__((aligned(16))) ebf_t sm[2 * EBF_BM * LD];  // A rows | W rows
  ebf_t* sA = sm;
  ebf_t* sW = sm + EBF_BM * LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const long m0 = (long)blockIdx.y * EBF_BM;
  const int n0 = blockIdx.x * EBF_BN;
  const int K = a.K, N = a.N;
  const long M = a.M;

  // two levels of summation: `acc` takes 256 of k (16 matrix steps), then moves into `tot`.  One chain over a K of 1536 rounds a
  // running sum of the full magnitude 96 times and came out at 4 x the error of a blocked host GEMM; this halves it.
  ebf_acc_t acc[2][2], tot[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = tot[i][j][v] = 0.f;

  // chunk q = tid + 256 i of an operand step: row q / 8, 16-byte chunk q % 8; rows past the end are clamped (never stored)
  const ebf_t *gA[4], *gW[4];
  int soff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = tid + 256 * i, row = q >> 3, c = q & 7;
    const long ar = m0 + row < M ? m0 + row : M - 1;
    const int wr = n0 + row < N ? n0 + row : N - 1;
    gA[i] = a.A + ar * K + c * 8;
    gW[i] = a.W + (long)wr * K + c * 8;
    soff[i] = row * LD + c * 8;
  }
  ebf_u4_t ra[4], rw[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const ebf_u4_t*>(gA[i] + k0);
      rw[i] = *reinterpret_cast<const ebf_u4_t*>(gW[i] + k0);
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += EBF_BK) {
    __syncthreads();  // the previous step's fragments have been read
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<ebf_u4_t*>(sA + soff[i]) = ra[i];
      *reinterpret_cast<ebf_u4_t*>(sW + soff[i]) = rw[i];
    }
    __syncthreads();
    if (k0 + EBF_BK < K) fetch(k0 + EBF_BK);
#pragma unroll
    for (int ks = 0; ks < EBF_BK / 16; ++ks) {
      ebf8_t fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = *reinterpret_cast<const ebf8_t*>(sA + (wm * 64 + i * 32 + r) * LD + ks * 16 + h * 8);
        fb[i] = *reinterpret_cast<const ebf8_t*>(sW + (wn * 64 + i * 32 + r) * LD + ks * 16 + h * 8);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if ((k0 / EBF_BK & 3) == 3 || k0 + EBF_BK >= K) {  // uniform: after every fourth step, and after the last
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          tot[i][j] += acc[i][j];
#pragma unroll
          for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;
        }
    }
  }

  // C/D map of the 32 x 32 product: column = lane & 31, row = (v & 3) + 8 (v >> 2) + 4 (lane >> 5)
  if constexpr (EPI == EBF_EPI_RESID_F32) {
    float* out = reinterpret_cast<float*>(a.out);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + r;
      if (n >= N) continue;
      const float bv = a.bias[n];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const long m = m0 + wm * 64 + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
          if (m < M) out[m * N + n] = (tot[i][j][v] + bv) + a.res[m * N + n];
        }
    }
  } else {
    // bf16 rows leave through LDS: the accumulator has n on the lane and scattered m in its registers; staged, a store is 16 bytes
    __syncthreads();  // every wave is done with the operand stage
    ebf_t* tile = sm;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nl = wn * 64 + j * 32 + r;
      const float bv = n0 + nl < N ? a.bias[n0 + nl] : 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int ml = wm * 64 + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
          float x = tot[i][j][v] + bv;
          if (EPI == EBF_EPI_GELU_BF16) x = spk_gelu(x);
          tile[ml * LDT + nl] = (ebf_t)x;
        }
    }
    __syncthreads();
    ebf_t* out = reinterpret_cast<ebf_t*>(a.out);
#pragma unroll
    for (int q = 0; q < 8; ++q) {  // 128 rows x 16 chunks of 8 columns; N is a multiple of 8: a chunk is inside or outside
      const int id = tid + 256 * q, row = id >> 4, c = id & 15;
      if (m0 + row < M && n0 + c * 8 < N)
        *reinterpret_cast<ebf_u4_t*>(out + (m0 + row) * N + n0 + c * 8) = *reinterpret_cast<const ebf_u4_t*>(tile + row * LDT + c * 8);
    }
  }
}

// ---- residual + LayerNorm, bf16 rows ----------------------------------------------------------------------------------------------
// s = a[row] + b[bmod > 0 ? row % bmod : row] (b null: s = a[row]), stored to `sum` when it is not null (it may be `a`);
// y = bf16(LayerNorm(s)).  The sum s is fp32, as asr_add_layernorm's; the statistics and the normalisation are taken in fp64, so that a row
// element is within one bf16 ulp of the exact LayerNorm of s even where (s - mean) rstd w and beta cancel (fp32 arithmetic leaves an
// absolute error of 1e-7 there, many ulps of a result near zero).  The kernel moves 14 bytes an element; the fp64 work hides under that.
// One wave per row.
static __global__ __launch_bounds__(256) void ebf_add_layernorm(const float* a, const float* __restrict__ b, int bmod, const float* __restrict__ w,
                                                                const float* __restrict__ beta, float* sum, ebf_t* __restrict__ y, long M,
                                                                int d, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* ap = a + row * d;
  const float* bp = b ? b + (bmod > 0 ? row % bmod : row) * d : nullptr;
  double s = 0.0;
  for (int c = lane; c < d; c += 64) s += (double)(bp ? ap[c] + bp[c] : ap[c]);
#pragma unroll
  for (int w_ = 32; w_ > 0; w_ >>= 1) s += __shfl_xor(s, w_);
  const double mean = s / d;
  double q = 0.0;
  for (int c = lane; c < d; c += 64) {
    const double v = (double)(bp ? ap[c] + bp[c] : ap[c]) - mean;
    q = fma(v, v, q);
  }
#pragma unroll
  for (int w_ = 32; w_ > 0; w_ >>= 1) q += __shfl_xor(q, w_);
  const double rstd = 1.0 / sqrt(q / d + (double)eps);
  for (int c = lane; c < d; c += 64) {
    const float v = bp ? ap[c] + bp[c] : ap[c];
    y[row * d + c] = (ebf_t)(float)(((double)v - mean) * rstd * (double)w[c] + (double)beta[c]);
    if (sum) sum[row * d + c] = v;
  }
}

// ---- attention -------------------------------------------------------------------------------------------------------------------
struct EbfAttnArgs {
  const ebf_t* qkv;  // rows (M, 3 d): q | k | v, head h at columns 64 h .. 64 h + 63 of each
  ebf_t* out;        // rows (M, d)
  const int* seg;    // [nseg + 1] row offsets
  int nseg, H, d;
};

// grid (the call's query tiles: ceil(len / 128) per segment, heads), 256 threads.
static __global__ __launch_bounds__(256) void ebf_attention(const EbfAttnArgs a) {
  constexpr int LD = EBF_LD, KT = EBF_KT;
  __shared__ __attribute__((aligned(16))) ebf_t sK[KT * LD];   // [key][channel]
  __shared__ __attribute__((aligned(16))) ebf_t sVt[64 * LD];  // [channel][key]
  long lo, T, t0;
  const int s = spk_find_tile(a.seg, a.nseg, EBF_QT, blockIdx.x, lo, T, t0);
  if (s == a.nseg) return;  // uniform over the workgroup
  const int head = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const long ld = 3L * a.d;
  const ebf_t* qb = a.qkv + lo * ld + head * 64;
  const ebf_t* kb = qb + a.d;
  const ebf_t* vb = qb + 2 * a.d;
  const bool live = t0 + wave * 32 < T;  // wave-uniform: a wave past the segment only helps with the loads
  const long qi = t0 + wave * 32 + r;
  const long qrow = qi < T ? qi : T - 1;
  ebf8_t qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const ebf8_t*>(qb + qrow * ld + ks * 16 + h * 8);

  ebf_acc_t accO[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) accO[t][v] = 0.f;
  float mrun = -INFINITY, lrun = 0.f;

  // K chunk q = tid + 256 i: key q / 8, chunk q % 8 (a key's 128 bytes are read by 8 neighbouring lanes); V chunk q: key q % 64,
  // chunk q / 64 (the transposed LDS writes of a wave fall on 64 neighbouring keys of one channel)
  ebf_u4_t rk[2], rv[2];
  auto fetch = [&](long k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = tid + 256 * i;
      const long kr = k0 + (q >> 3) < T ? k0 + (q >> 3) : T - 1;
      rk[i] = *reinterpret_cast<const ebf_u4_t*>(kb + kr * ld + (q & 7) * 8);
      const long vr = k0 + (q & 63) < T ? k0 + (q & 63) : T - 1;
      rv[i] = *reinterpret_cast<const ebf_u4_t*>(vb + vr * ld + (q >> 6) * 8);
    }
  };
  fetch(0);
  for (long k0 = 0; k0 < T; k0 += KT) {
    __syncthreads();  // the previous step's fragments have been read
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = tid + 256 * i;
      *reinterpret_cast<ebf_u4_t*>(sK + (q >> 3) * LD + (q & 7) * 8) = rk[i];
      const ebf8_t pv = __builtin_bit_cast(ebf8_t, rv[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) sVt[((q >> 6) * 8 + e) * LD + (q & 63)] = pv[e];
    }
    __syncthreads();
    if (k0 + KT < T) fetch(k0 + KT);
    if (!live) continue;

    // S^T (keys x queries): register v of sub-tile `sub` is key k0 + 32 sub + (v & 3) + 8 (v >> 2) + 4 h of the lane's query
    ebf_acc_t accS[2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
      for (int v = 0; v < 16; ++v) accS[sub][v] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const ebf8_t kf = *reinterpret_cast<const ebf8_t*>(sK + (sub * 32 + r) * LD + ks * 16 + h * 8);
        accS[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], accS[sub], 0, 0, 0);
      }
    }
    float mloc = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const long key = k0 + sub * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
        const float sc = key < T ? accS[sub][v] * 0.125f : -INFINITY;  // 64^-1/2
        accS[sub][v] = sc;
        mloc = fmaxf(mloc, sc);
      }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
    const float mnew = fmaxf(mrun, mloc);  // finite: key k0 is inside the segment
    const float alpha = __expf(mrun - mnew);
    mrun = mnew;
    float psum = 0.f;
    ebf8_t pf[2][2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float p = __expf(accS[sub][v] - mnew);
        psum += p;
        pf[sub][v >> 3][v & 7] = (ebf_t)p;
      }
    lrun = lrun * alpha + psum;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) accO[t][v] *= alpha;
    // O^T (channels x queries) += V^T P^T: element j of k-step s2 is key 32 sub + 16 s2 + 8 (j >> 2) + 4 h + (j & 3) on both sides
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const ebf_t* vp = sVt + (t * 32 + r) * LD + sub * 32 + s2 * 16 + 4 * h;
          const ebf_u2_t v0 = *reinterpret_cast<const ebf_u2_t*>(vp), v1 = *reinterpret_cast<const ebf_u2_t*>(vp + 8);
          const ebf_u4_t vv = {v0.x, v0.y, v1.x, v1.y};
          accO[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(ebf8_t, vv), pf[sub][s2], accO[t], 0, 0, 0);
        }
  }
  if (!live) return;
  const float ltot = lrun + __shfl_xor(lrun, 32);  // the two halves' keys; a + b on one side, b + a on the other
  if (qi >= T) return;
  ebf_t* op = a.out + (lo + qi) * a.d + head * 64;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {  // registers 4 g .. 4 g + 3: channels 32 t + 8 g + 4 h .. + 3
      ebf4_t o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (ebf_t)(accO[t][4 * g + j] / ltot);
      *reinterpret_cast<ebf4_t*>(op + t * 32 + 8 * g + 4 * h) = o;
    }
}

}  // namespace vx
