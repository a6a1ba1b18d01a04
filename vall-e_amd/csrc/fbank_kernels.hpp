// Log-mel filterbank (the reference's BigVGANFbank, valle/data/fbank.py:80-131) in one kernel: 24 kHz, n_fft 1024, hop 256,
// periodic Hann window, one-sided magnitude sqrt(re^2 + im^2 + 1e-9), mel basis, log with a floor.
//
// The 1024-point DFT of a frame is the four-step 32 x 32 factorisation on the fp32 matrix instruction (v_mfma_f32_32x32x2_f32:
// a k-ordered fmaf chain, one rounding per product).  With n = 32 n1 + n2 and k = k1 + 32 k2,
//   W1024^(n k) = W32^(n1 k1) * W1024^(n2 k1) * W32^(n2 k2),
//   stage 1   Y[n2][k1] = sum_n1 x[32 n1 + n2] win[32 n1 + n2] W32^(n1 k1)       2 products  (cos, sin)
//   twiddle   Z[n2][k1] = Y[n2][k1] W1024^(n2 k1)                                 in registers
//   stage 2   F[k1][k2] = sum_n2 Z[n2][k1] W32^(n2 k2)                            4 products, two chains of 64
// Stage 1 is computed transposed (rows n2, columns k1), so the lane that receives Z[.][k1] of the accumulator layout (column =
// lane & 31, rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) is the lane that supplies row k1 of stage 2's first operand: the sum
// over n2 runs in the accumulator's row order (a fixed permutation of 0..31, the same for every frame), and nothing goes through
// LDS between the stages.  Only k2 <= 16 is kept (bins 0..512; k2 = 16 only for k1 = 0).  All tables (window, cos / sin of
// 2 pi j / 1024) are built on the host in fp64 and rounded once; a lane keeps its 112 table values in registers over its frames.
//
// One workgroup owns FBANK_TILE consecutive frames of ONE utterance: their samples, contiguous, go to LDS once (zero past the
// utterance's end: the reference's right padding), wave w takes frames w, w + 4, ... and leaves their magnitudes in LDS, then
// every thread owns (frame, filter) cells: the filter's band [lo, hi] (found at set_mel_basis time; the whole row for a dense
// basis) summed in ascending bin order (an fmaf chain per aligned group of 32 bins), max with the floor, log.  No atomics, no
// hand-over between workgroups: a frame's bits depend on its own 1024 samples only, never on the batch or on its place in the
// launch.
#pragma once
#include "common.hpp"

namespace vx {

constexpr int FBANK_NFFT = 1024, FBANK_HOP = 256, FBANK_BINS = 513, FBANK_MAX_MELS = 128;
constexpr int FBANK_TILE = 16;                                               // frames per workgroup
constexpr int FBANK_SPAN = (FBANK_TILE - 1) * FBANK_HOP + FBANK_NFFT;        // samples a tile reads
constexpr int FBANK_MAG_LD = 17 * 33;                                        // magnitudes of a frame: [k2 <= 16][k1, padded to 33]
constexpr int FBANK_TAB = 3 * 1024;                                          // window | cos(2 pi j / 1024) | sin(2 pi j / 1024)

struct FbankArgs {
  const float* const* wav;  // [nseg] mono fp32
  float* const* out;        // [nseg] (frames, n_mels)
  const int* tile0;         // [nseg + 1] first tile of every utterance (an utterance without frames has none)
  const int* len;           // [nseg] samples
  const int* frames;        // [nseg] (L + 128) / 256
  const float* tab;         // [FBANK_TAB]
  const float* basis_t;     // [513][n_mels]: bin-major, so that the lanes of consecutive filters read consecutive words
  const int* band;          // lo [n_mels] | hi [n_mels]: first and last non-zero bin of a filter (lo > hi: an empty filter)
  int nseg, n_mels;
  float clip;
};

__global__ __launch_bounds__(256) void fbank_kernel(const FbankArgs a) {
  typedef float f32x16 __attribute__((ext_vector_type(16)));
  __shared__ float S[FBANK_SPAN];
  __shared__ float Mag[FBANK_TILE * FBANK_MAG_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
  const float* cs = a.tab + 1024;
  const float* sn = a.tab + 2048;
  // per lane, constant over the frames: step kk of stage 1 is n1 = 2 kk + h; register r of an accumulator is row
  // (r & 3) + 8 (r >> 2) + 4 h, which is n2 after stage 1 and k1 after stage 2
  float win[16], dc[16], ds[16], tc[16], ts[16], ec[16], es[16];
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    const int n1 = 2 * kk + h;
    win[kk] = a.tab[32 * n1 + c];
    dc[kk] = cs[32 * ((n1 * c) & 31)];
    ds[kk] = sn[32 * ((n1 * c) & 31)];
    const int n2 = (kk & 3) + 8 * (kk >> 2) + 4 * h;
    tc[kk] = cs[n2 * c];
    ts[kk] = sn[n2 * c];
    ec[kk] = cs[32 * ((n2 * c) & 31)];
    es[kk] = sn[32 * ((n2 * c) & 31)];
  }
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
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
    const int f0 = (tile - a.tile0[s]) * FBANK_TILE;
    const int nft = min(FBANK_TILE, a.frames[s] - f0);  // >= 1
    const long g0 = (long)f0 * FBANK_HOP;
    const int span = (nft - 1) * FBANK_HOP + FBANK_NFFT;
    __syncthreads();  // the previous tile's reads of S and Mag are done
    for (int i = tid; i < span; i += 256) S[i] = g0 + i < L ? x[g0 + i] : 0.f;
    __syncthreads();
    for (int fl = wave; fl < nft; fl += 4) {
      const float* xf = S + fl * FBANK_HOP + lane;  // sample 32 n1 + c = 64 kk + lane
      f32x16 yr = zero, yp = zero;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const float v = xf[64 * kk] * win[kk];
        yr = __builtin_amdgcn_mfma_f32_32x32x2f32(v, dc[kk], yr, 0, 0, 0);
        yp = __builtin_amdgcn_mfma_f32_32x32x2f32(v, ds[kk], yp, 0, 0, 0);
      }
      // Y = yr - i yp; times cos - i sin: Z = zr - i zq
      float zr[16], zq[16], nzq[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        zr[r] = fmaf(yr[r], tc[r], -(yp[r] * ts[r]));
        zq[r] = fmaf(yr[r], ts[r], yp[r] * tc[r]);
        nzq[r] = -zq[r];
      }
      // (zr - i zq)(cos - i sin) = (zr cos - zq sin) - i (zr sin + zq cos)
      f32x16 re = zero, im = zero;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(zr[r], ec[r], re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(zr[r], es[r], im, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(nzq[r], es[r], re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(zq[r], ec[r], im, 0, 0, 0);
      }
      if (c <= 16) {  // column k2 = c, row k1: bin k1 + 32 k2 <= 512
        float* mg = Mag + fl * FBANK_MAG_LD + c * 33;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k1 = (r & 3) + 8 * (r >> 2) + 4 * h;
          if (c < 16 || k1 == 0) mg[k1] = sqrtf(re[r] * re[r] + im[r] * im[r] + 1e-9f);
        }
      }
    }
    __syncthreads();
    float* o = a.out[s] + (long)f0 * a.n_mels;
    for (int item = tid; item < nft * a.n_mels; item += 256) {
      const int f = item / a.n_mels, m = item - f * a.n_mels;
      const int lo = a.band[m], hi = a.band[a.n_mels + m];
      const float* mg = Mag + f * FBANK_MAG_LD;
      // ascending bins; every aligned group of 32 bins (one k2) is an fmaf chain of its own and the groups' sums are added in
      // order: a dense basis of 513 weights then carries the rounding of a 32-chain plus a 17-chain, not of a 513-chain
      float acc = 0.f;
      for (int b0 = lo & ~31; b0 <= hi; b0 += 32) {
        const float* mrow = mg + (b0 >> 5) * 33 - b0;
        const int e = min(hi, b0 + 31);
        float part = 0.f;
        for (int b = max(lo, b0); b <= e; ++b) part = fmaf(a.basis_t[b * a.n_mels + m], mrow[b], part);
        acc += part;
      }
      // the log in fp64, rounded once: the device's logf is good to about 2 ulp (measured 1.67 ulp at the floor 1e-5, where the
      // result is -11.5 and every cell of a silent input lands), which alone is the error the fp32 host formula has in total
      o[item] = (float)log((double)fmaxf(acc, a.clip));
    }
  }
}

}  // namespace vx
