// Griffin-Lim vocoder (include/vallex.h, vx_vocoder_*): log-mel frames back to a 24 kHz waveform through the filterbank's own
// framing (n_fft 1024, hop 256, periodic Hann window).  Three kernels, fp32 throughout:
//
//   voc_mag_kernel      mag = max(0, exp(logmel) . P^T) per (frame, bin), every cell an fmaf chain in ascending filter order, and
//                       the starting phase (1 + 0i, the caller's radians, or the caller's unit complex numbers).  Once per call.
//   voc_frame_kernel    frame f of I(mag . ang): the 1024-point inverse real DFT of one row, times window / 1024.  It is the
//                       four-step 32 x 32 factorisation of fbank_kernels.hpp run backwards on v_mfma_f32_32x32x2_f32.  The row
//                       is extended to 1024 bins (X[1024 - k] = conj X[k]; the imaginary parts of bins 0 and 512 are not read),
//                       and with k = k1 + 32 k2, n = 32 n1 + n2
//                         stage A   U[k1][n2] = sum_k2 X[k1 + 32 k2] W32^(-n2 k2)              4 products (complex x complex)
//                         twiddle   V[k1][n2] = U[k1][n2] W1024^(-n2 k1)                       in registers
//                         stage B   x[32 n1 + n2] = Re sum_k1 V[k1][n2] W32^(-n1 k1)           2 products
//                       Stage A leaves column n2 = lane & 31 and rows k1 = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) in the lane that
//                       supplies exactly those (n2, k1) of stage B's first operand: nothing goes through LDS.  A lane ends with
//                       four runs of four consecutive samples and stores them as four 16-byte words.
//   voc_analysis_kernel a workgroup owns a tile of consecutive frames of ONE utterance, as the filterbank's tile does.  It GATHERS
//                       its span of y = overlap-add / max(envelope, floor) from the <= 4 frames that cover a sample, added in
//                       ascending frame order (no scatter, no atomics), zero from sample 256 T on; then either writes its 256
//                       samples per frame of y and the final phase (the last launch of a synthesis), or runs the forward
//                       four-step DFT of fbank_kernel on the span and applies a = reb - tprev c, ang = a / (|a| + 1e-16),
//                       tprev = reb per bin.
// One iteration is voc_frame_kernel + voc_analysis_kernel; a synthesis of n_iter iterations is 1 + 2 (n_iter + 1) launches.  A
// frame's bits depend on its own utterance only, never on the batch or on its place in the launch.  The tile is a run-time
// argument (VocArgs::tile: 16 frames, or 4 when the whole call has too few frames to give every CU a tile of 16): it only says
// which workgroup computes a frame, the same instructions compute it either way, so the bits do not depend on it.
#pragma once
#include "common.hpp"

namespace vx {

constexpr int VOC_NFFT = 1024, VOC_HOP = 256, VOC_BINS = 513, VOC_MAX_MELS = 128;
constexpr int VOC_TILE = 16, VOC_TILE_SMALL = 4;                       // frames per workgroup: a large call, a small call
constexpr int VOC_SPAN = (VOC_TILE - 1) * VOC_HOP + VOC_NFFT;          // samples an analysis tile holds
constexpr int VOC_Z_LD = 17 * 33;                                      // one component of a frame's spectrum: [k2 <= 16][k1, padded to 33]
constexpr int VOC_TAB = 5 * 1024;  // window | cos(2 pi j / 1024) | sin(2 pi j / 1024) | window / 1024 | window^2
enum { VOC_INIT_NONE = 0, VOC_INIT_RADIANS = 1, VOC_INIT_UNIT = 2 };

struct VocArgs {
  const float* const* logmel;  // [nseg] (T, n_mels)
  const float* const* init;    // [nseg] (T, 513) radians or (T, 513, 2) unit complex; read only when init_kind != VOC_INIT_NONE
  float* const* wav;           // [nseg] 256 T samples
  float* const* phase;         // [nseg] (T, 513, 2); written only when has_phase
  const int* tile0;            // [nseg + 1] first tile of every utterance (an utterance without frames has none)
  const int* frames;           // [nseg] T
  const int* fr0;              // [nseg] the utterance's first row in the workspace
  const float* tab;            // [VOC_TAB]
  const float* pinv_t;         // [n_mels][513]: filter-major, so that the lanes of consecutive bins read consecutive words
  float* mag;                  // workspace, one row per frame of the call: [513]
  float* ang;                  //   [513][2]
  float* tprev;                //   [513][2]
  float* fr;                   //   [1024] windowed samples of the frame
  int nseg, n_mels, init_kind, has_phase;
  int tile;                    // frames per workgroup in this call: VOC_TILE, or VOC_TILE_SMALL when the call has few frames
  float env_floor, mom;        // mom = momentum / (1 + momentum)
};

// The utterance of a tile: the last s with tile0[s] <= tile (utterances without tiles share a start: the last wins).
__device__ inline int voc_segment(const int* tile0, int nseg, int tile) {
  int s = 0;
  for (int hi_s = nseg; hi_s - s > 1;) {
    const int mid = (s + hi_s) >> 1;
    if (tile0[mid] <= tile) s = mid;
    else hi_s = mid;
  }
  return s;
}

__global__ __launch_bounds__(256) void voc_mag_kernel(const VocArgs a) {
  __shared__ float E[VOC_TILE * VOC_MAX_MELS];
  const int tid = threadIdx.x, M = a.n_mels;
  const int total = a.tile0[a.nseg];
  for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int s = voc_segment(a.tile0, a.nseg, tile);
    const int f0 = (tile - a.tile0[s]) * a.tile;
    const int nft = min(a.tile, a.frames[s] - f0);  // >= 1
    const long g0 = (long)a.fr0[s] + f0;
    const float* lm = a.logmel[s] + (long)f0 * M;
    __syncthreads();  // the previous tile's reads of E are done
    // exp in fp64, rounded once (the device's expf is good to about an ulp more than that)
    for (int i = tid; i < VOC_TILE * M; i += 256) E[(i / M) * VOC_MAX_MELS + i % M] = i < nft * M ? (float)exp((double)lm[i]) : 0.f;
    __syncthreads();
    for (int b = tid; b < VOC_BINS; b += 256) {
      float acc[VOC_TILE];
#pragma unroll
      for (int f = 0; f < VOC_TILE; ++f) acc[f] = 0.f;
      for (int m = 0; m < M; ++m) {
        const float p = a.pinv_t[m * VOC_BINS + b];
#pragma unroll
        for (int f = 0; f < VOC_TILE; ++f) acc[f] = fmaf(E[f * VOC_MAX_MELS + m], p, acc[f]);
      }
#pragma unroll
      for (int f = 0; f < VOC_TILE; ++f)
        if (f < nft) a.mag[(g0 + f) * VOC_BINS + b] = fmaxf(acc[f], 0.f);
    }
    float2* ang = (float2*)a.ang + g0 * VOC_BINS;
    for (int i = tid; i < nft * VOC_BINS; i += 256) {
      float2 v = make_float2(1.f, 0.f);
      if (a.init_kind == VOC_INIT_RADIANS) {
        double sn, cs;
        sincos((double)a.init[s][(long)f0 * VOC_BINS + i], &sn, &cs);
        v = make_float2((float)cs, (float)sn);
      } else if (a.init_kind == VOC_INIT_UNIT) {
        const float* u = a.init[s] + 2 * ((long)f0 * VOC_BINS + i);  // the caller's pointer need not be 8-byte aligned
        v = make_float2(u[0], u[1]);
      }
      ang[i] = v;
    }
  }
}

__global__ __launch_bounds__(256) void voc_frame_kernel(const VocArgs a) {
  typedef float f32x16 __attribute__((ext_vector_type(16)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
  const float* cs = a.tab + 1024;
  const float* sn = a.tab + 2048;
  const float* wn = a.tab + 3072;
  // per lane, constant over the frames: step kk of stage A is k2 = 2 kk + h; register r of an accumulator is row
  // (r & 3) + 8 (r >> 2) + 4 h, which is k1 after stage A and n2 after stage B
  float ac[16], as[16], tc[16], ts[16], ec[16], es[16], wo[16];
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    const int k2 = 2 * kk + h;
    ac[kk] = cs[32 * ((k2 * c) & 31)];
    as[kk] = sn[32 * ((k2 * c) & 31)];
    const int row = (kk & 3) + 8 * (kk >> 2) + 4 * h;
    tc[kk] = cs[row * c];
    ts[kk] = sn[row * c];
    ec[kk] = cs[32 * ((row * c) & 31)];
    es[kk] = sn[32 * ((row * c) & 31)];
    wo[kk] = wn[32 * c + row];
  }
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int total = a.tile0[a.nseg];
  for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int s = voc_segment(a.tile0, a.nseg, tile);
    const int f0 = (tile - a.tile0[s]) * a.tile;
    const int nft = min(a.tile, a.frames[s] - f0);
    const long g0 = (long)a.fr0[s] + f0;
    for (int fl = wave; fl < nft; fl += 4) {
      const float* mg = a.mag + (g0 + fl) * VOC_BINS;
      const float2* an = (const float2*)a.ang + (g0 + fl) * VOC_BINS;
      // U = ur + i ui = sum X (cos + i sin)
      f32x16 ur = zero, ui = zero;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const int k = 64 * kk + lane, kb = k <= 512 ? k : 1024 - k;  // element k1 + 32 k2 = 64 kk + lane of the extended row
        const float m = mg[kb];
        const float2 p = an[kb];
        const float xr = m * p.x;
        const float t = m * p.y;
        const float xi = (kb == 0 || kb == 512) ? 0.f : (k > 512 ? -t : t);
        ur = __builtin_amdgcn_mfma_f32_32x32x2f32(xr, ac[kk], ur, 0, 0, 0);
        ui = __builtin_amdgcn_mfma_f32_32x32x2f32(xr, as[kk], ui, 0, 0, 0);
        ur = __builtin_amdgcn_mfma_f32_32x32x2f32(-xi, as[kk], ur, 0, 0, 0);
        ui = __builtin_amdgcn_mfma_f32_32x32x2f32(xi, ac[kk], ui, 0, 0, 0);
      }
      // V = U (cos + i sin) = vr + i vi
      float vr[16], nvi[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        vr[r] = fmaf(ur[r], tc[r], -(ui[r] * ts[r]));
        nvi[r] = -fmaf(ur[r], ts[r], ui[r] * tc[r]);
      }
      // Re V (cos + i sin) = vr cos - vi sin
      f32x16 x = zero;
#pragma unroll
      for (int r = 0; r < 16; ++r) x = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[r], ec[r], x, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) x = __builtin_amdgcn_mfma_f32_32x32x2f32(nvi[r], es[r], x, 0, 0, 0);
      // column n1 = c, rows n2 = 8 q + 4 h + (0 .. 3): samples 32 c + n2, four consecutive ones per q
      float4* o = (float4*)(a.fr + (g0 + fl) * VOC_NFFT + 32 * c + 4 * h);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        o[2 * q] = make_float4(x[4 * q] * wo[4 * q], x[4 * q + 1] * wo[4 * q + 1], x[4 * q + 2] * wo[4 * q + 2], x[4 * q + 3] * wo[4 * q + 3]);
    }
  }
}

// last == 0: an iteration's second half (first != 0: tprev is taken as zero and not read).  last != 0: y and the phase go out.
__global__ __launch_bounds__(256) void voc_analysis_kernel(const VocArgs a, const int first, const int last) {
  typedef float f32x16 __attribute__((ext_vector_type(16)));
  __shared__ float S[VOC_SPAN];
  __shared__ float Z[4 * 2 * VOC_Z_LD];  // the spectra of the four frames in flight: [wave][re | im]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
  const float* cs = a.tab + 1024;
  const float* sn = a.tab + 2048;
  const float* w2 = a.tab + 4096;
  float win[16], dc[16], ds[16], tc[16], ts[16], ec[16], es[16];  // as in fbank_kernel
  if (!last) {
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
  }
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int total = a.tile0[a.nseg];
  for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int s = voc_segment(a.tile0, a.nseg, tile);
    const int T = a.frames[s];
    const int f0 = (tile - a.tile0[s]) * a.tile;
    const int nft = min(a.tile, T - f0);  // >= 1
    const long g0 = (long)a.fr0[s] + f0;
    const long n0 = (long)f0 * VOC_HOP, nend = (long)T * VOC_HOP;
    const int span = last ? nft * VOC_HOP : (nft - 1) * VOC_HOP + VOC_NFFT;
    __syncthreads();  // the previous tile's reads of S and Z are done
    for (int i = tid; i < span; i += 256) {
      const long n = n0 + i;
      float y = 0.f;
      if (n < nend) {
        const int flo = n >= 768 ? (int)((n - 768) >> 8) : 0, fhi = min((int)(n >> 8), T - 1);
        const float* src = a.fr + ((long)a.fr0[s] + flo) * VOC_NFFT + (n - (long)flo * VOC_HOP);
        const float* e = w2 + (n - (long)flo * VOC_HOP);
        float ola = 0.f, env = 0.f;
        for (int f = flo; f <= fhi; ++f, src += VOC_NFFT - VOC_HOP, e -= VOC_HOP) {
          ola += *src;
          env += *e;
        }
        y = ola / fmaxf(env, a.env_floor);
      }
      S[i] = y;
    }
    __syncthreads();
    if (last) {
      float* o = a.wav[s] + n0;
      for (int i = tid; i < span; i += 256) o[i] = S[i];
      if (a.has_phase) {
        const float* src = a.ang + g0 * (2 * VOC_BINS);
        float* dst = a.phase[s] + (long)f0 * (2 * VOC_BINS);
        for (int i = tid; i < nft * 2 * VOC_BINS; i += 256) dst[i] = src[i];
      }
      continue;
    }
    for (int fl0 = 0; fl0 < nft; fl0 += 4) {
      const int fl = fl0 + wave;
      if (fl < nft) {
        const float* xf = S + fl * VOC_HOP + lane;  // sample 32 n1 + c = 64 kk + lane
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
          float* z = Z + wave * (2 * VOC_Z_LD) + c * 33;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int k1 = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (c < 16 || k1 == 0) {
              z[k1] = re[r];
              z[VOC_Z_LD + k1] = -im[r];  // the spectrum is re - i im
            }
          }
        }
      }
      __syncthreads();
      const int nfl = min(4, nft - fl0);
      for (int i = tid; i < nfl * VOC_BINS; i += 256) {
        const int w = i / VOC_BINS, b = i - w * VOC_BINS;
        const float* z = Z + w * (2 * VOC_Z_LD) + (b >> 5) * 33 + (b & 31);
        const float rr = z[0], ri = z[VOC_Z_LD];
        const long cell = (g0 + fl0) * VOC_BINS + i;
        float2* tp = (float2*)a.tprev + cell;
        float ar = rr, ai = ri;
        if (!first) {
          const float2 t = *tp;
          ar = rr - t.x * a.mom;
          ai = ri - t.y * a.mom;
        }
        const float nrm = sqrtf(ar * ar + ai * ai) + 1e-16f;
        ((float2*)a.ang)[cell] = make_float2(ar / nrm, ai / nrm);
        *tp = make_float2(rr, ri);
      }
      __syncthreads();  // Z is free for the next four frames
    }
  }
}

}  // namespace vx
