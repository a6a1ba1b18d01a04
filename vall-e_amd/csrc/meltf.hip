// The launch that opens every decode step of the mel-spectrogram Transformer (valle/models/transformer.py:356-383 with a KV
// cache): where the token models sample from 1025 logits and embed the token, this model has no vocabulary - the head is 101 dot
// products (predict_layer's 100 mel bins and stop_layer's logit), the stop rule is a threshold, and the frame itself goes back in
// through decoder_prenet.  One kernel does all of it:
//   * every workgroup redundantly normalises the last residual row and forms the 101 dot products - the same loads, the same
//     fixed reduction order, hence the same bits everywhere: redundant work in place of a launch boundary;
//   * every workgroup decides the stop rule from its own copy and writes ITS slice of the next input row,
//     decoder_prenet(frame) + alpha pe[position]; the two 256-wide layers of the MLP prenet are computed redundantly as well;
//   * exactly one workgroup stores the frame and the stop logit, advances the position and raises the stop flag.
// The position word is read by every workgroup and advanced by one of them in the same launch.  No workgroup may see the advanced
// value, and none may spin: thread 0 of every workgroup reads the state, then adds one to an arrival counter (agent scope); the
// workgroup whose add returns grid - 1 knows that every other workgroup has read, does the book-keeping and resets the counter.
// Nothing a workgroup writes is read by another in the same launch (the next input row goes to `x`, the head reads `xh`), so the
// counter carries no payload and needs no fence.  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include "../../include/vallex.h"
#include "meltf.hpp"

namespace vx {

// Latency: the step streams ~400 MB (bf16) of layer weights between two of these launches, so every load here misses the L2 and a
// dependent round trip costs 1.5 - 2 us.  The kernel is therefore built around few round trips, not few bytes: the state, the
// residual row, this workgroup's prenet rows (16 rows per wave, held in registers from the start) and the first head batch are
// requested at entry, before anything is waited for; the 26 head rows of a wave come in 4 batches of 7 x 4 loads of 16 bytes;
// the arrival add is issued early and its result is looked at only in front of the book-keeping.
constexpr int MEL_HB = 7;      // head rows per batch and wave
constexpr int MEL_HROWS = 26;  // head rows per wave: 4 x 26 >= 101
constexpr int MEL_PR = 16;     // prenet rows per wave: 4 x 16 x MEL_GRID >= 1024

// y + alpha p with the product rounded on its own, as torch's two operations.  __fadd_rn(y, __fmul_rn(alpha, p)) does not say
// that: the two intrinsics are a plain `*` and `+`, which the compiler contracts into one fused multiply-add (one rounding).
__device__ __forceinline__ float add_scaled_2r(float y, float alpha, float p) {
#pragma clang fp contract(off)
  const float m = alpha * p;
  return y + m;
}

__global__ __launch_bounds__(256) void mel_open_kernel(const MelStepArgs a) {
  __shared__ __attribute__((aligned(16))) float sx[1024];            // the normalised row
  __shared__ __attribute__((aligned(16))) float sf[128];             // predict [0, 100), stop logit [100]
  __shared__ __attribute__((aligned(16))) float sin_[MEL_PRENET_H];  // the prenet's input: the fed-back frame, later its 2nd hidden layer
  __shared__ __attribute__((aligned(16))) float sh[MEL_PRENET_H];
  __shared__ float sbh[128], sb0[64], spe[64];  // head bias; prenet bias and position row of this workgroup's slice
  __shared__ float red[4];
  __shared__ int ss[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = a.d;
  const int K0 = a.W1 != nullptr ? MEL_PRENET_H : MEL_BINS;

  // ---- (A) every load that depends on nothing, issued before anything is waited for ----
  int s_row = 0, s_done = 0, s_pass = 0, s_ngen = 0, s_S = 0, s_max = 0, s_forced = 0;
  if (tid == 0) {
    const ArState* st = a.st;
    s_row = st->row; s_done = st->done; s_pass = st->pass; s_ngen = st->n_gen; s_S = st->S;
    s_max = a.ctl->max_frames; s_forced = a.ctl->n_forced;
  }
  const int k0 = tid * 4;
  const int kc = min(k0, d - 4);
  const float4 xv_ = *reinterpret_cast<const float4*>(a.xh + kc);
  const float4 gv_ = *reinterpret_cast<const float4*>(a.gamma + kc);
  const float4 bv_ = *reinterpret_cast<const float4*>(a.beta + kc);
  // this workgroup's slice of the d prenet rows (the last slices are ragged or empty); wave w owns MEL_PR consecutive rows
  const int per = (d + MEL_GRID - 1) / MEL_GRID;  // <= 64
  const int lo = min((int)blockIdx.x * per, d), hi = min(lo + per, d);
  // biases of the rows this workgroup finishes: requested now, parked in LDS later - a load at the point of use would be one
  // more round trip per batch
  const int pr = min(lo + (tid & 63), d - 1);
  const float bh_r = a.bh[min(tid, MEL_HEAD - 1)], b0_r = a.b0[pr], al = a.alpha[0];
  float4 w0[MEL_PR];
#pragma unroll
  for (int j = 0; j < MEL_PR; ++j)
    w0[j] = *reinterpret_cast<const float4*>(a.W0 + (size_t)min(lo + wave * MEL_PR + j, d - 1) * K0 + min(lane * 4, K0 - 4));
  float4 w[MEL_HB][4];
  auto head_issue = [&](int b) {
#pragma unroll
    for (int j = 0; j < MEL_HB; ++j) {
      const int r = min(wave * MEL_HROWS + min(b * MEL_HB + j, MEL_HROWS - 1), MEL_HEAD - 1);
#pragma unroll
      for (int c = 0; c < 4; ++c) w[j][c] = *reinterpret_cast<const float4*>(a.Wh + (size_t)r * d + min(c * 256 + lane * 4, d - 4));
    }
  };
  head_issue(0);
  __builtin_amdgcn_sched_barrier(0);  // keep the loads above where they are: the scheduler would sink them to their first use

  unsigned ticket = 0;
  if (tid == 0) {
    ss[0] = s_row; ss[1] = s_done; ss[2] = s_pass; ss[3] = s_ngen; ss[4] = s_S; ss[5] = s_max; ss[6] = s_forced;
    // the state is in registers (it was just stored to LDS): the add cannot overtake the reads.  A finished decode keeps
    // replaying the step: nobody counts, nobody writes (done is only ever set behind every workgroup's read).
    if (!s_done) ticket = __hip_atomic_fetch_add(&a.ctl->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const int row = ss[0], pass = ss[2], n_gen = ss[3], S = ss[4], max_frames = ss[5], n_forced = ss[6];
  if (ss[1]) return;  // uniform over the grid
  const float pe_r = a.pe[(size_t)(row + 1) * d + pr];  // the one load that needs the position: in flight across the head
  if (tid < MEL_HEAD) sbh[tid] = bh_r;

  int reason = VX_MEL_STOP_NONE;
  bool append = false, go = true;
  float stop = 0.f;
  if (row >= 0) {
    // ---- final LayerNorm of the row (two-pass, as F.layer_norm), all 256 threads, 4 channels each (d <= 1024) ----
    const bool kin = k0 < d;
    const float4 xv = kin ? xv_ : make_float4(0.f, 0.f, 0.f, 0.f);
    const float mean = block_sum<4>(xv.x + xv.y + xv.z + xv.w, red) / (float)d;
    const float4 dv = make_float4(xv.x - mean, xv.y - mean, xv.z - mean, xv.w - mean);
    const float sq = kin ? dv.x * dv.x + dv.y * dv.y + dv.z * dv.z + dv.w * dv.w : 0.f;
    const float rstd = 1.0f / sqrtf(block_sum<4>(sq, red) / (float)d + LN_EPS);
    *reinterpret_cast<float4*>(sx + k0) = kin ? make_float4(dv.x * rstd * gv_.x + bv_.x, dv.y * rstd * gv_.y + bv_.y,
                                                            dv.z * rstd * gv_.z + bv_.z, dv.w * rstd * gv_.w + bv_.w)
                                              : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    // ---- 101 dot products of length d: wave w owns rows [26 w, 26 w + 26), 7 at a time ----
    float4 xr[4];
    bool kok[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      kok[c] = c * 256 + lane * 4 < d;
      xr[c] = *reinterpret_cast<const float4*>(sx + c * 256 + lane * 4);  // zeros past d
    }
#pragma unroll 1
    for (int b = 0; b * MEL_HB < MEL_HROWS; ++b) {
      if (b) head_issue(b);
#pragma unroll
      for (int j = 0; j < MEL_HB; ++j) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (kok[c]) {
            s = fmaf(w[j][c].x, xr[c].x, s); s = fmaf(w[j][c].y, xr[c].y, s);
            s = fmaf(w[j][c].z, xr[c].z, s); s = fmaf(w[j][c].w, xr[c].w, s);
          }
        }
        s = wave_sum_dpp(s);
        const int i = b * MEL_HB + j, r = wave * MEL_HROWS + i;
        if (lane == 0 && i < MEL_HROWS && r < MEL_HEAD) sf[r] = s + sbh[r];
      }
    }
    __syncthreads();
    stop = sf[MEL_BINS];
    // ---- the stop rule, tested before the append (transformer.py:376-383): the stopping pass's frame is dropped ----
    if (n_forced > 0) {
      append = true;
      if (n_gen + 1 >= n_forced) reason = VX_MEL_STOP_MAX_FRAMES;
    } else if (row + 1 > 10 * S) reason = VX_MEL_STOP_LENGTH;
    else if (stop > 0.f) reason = VX_MEL_STOP_LOGIT;
    else if (n_gen >= max_frames) reason = VX_MEL_STOP_MAX_FRAMES;
    else append = true;
    go = append && reason == VX_MEL_STOP_NONE;
  }

  if (go) {
    // ---- the next input row: decoder_prenet(frame) + alpha pe[row + 1]; the frame at position 0 is all zero ----
    if (tid < MEL_PRENET_H) {
      float v = 0.f;
      if (tid < MEL_BINS && row >= 0) v = n_forced > 0 ? a.ctl->forced[(size_t)n_gen * MEL_BINS + tid] : sf[tid];
      sin_[tid] = v;
    }
    if (tid < 64) { sb0[tid] = b0_r; spe[tid] = pe_r; }
    __syncthreads();
    if (a.W1 != nullptr) {  // Linear(100, 256) + ReLU, Linear(256, 256) + ReLU: one output per thread, redundantly
      {
        const float* wr = a.W1 + (size_t)tid * MEL_BINS;
        float s = 0.f;
#pragma unroll 5
        for (int k = 0; k < MEL_BINS; k += 4) {
          const float4 wv = *reinterpret_cast<const float4*>(wr + k);
          const float4 iv = *reinterpret_cast<const float4*>(sin_ + k);
          s = fmaf(wv.x, iv.x, s); s = fmaf(wv.y, iv.y, s); s = fmaf(wv.z, iv.z, s); s = fmaf(wv.w, iv.w, s);
        }
        sh[tid] = fmaxf(s + a.b1[tid], 0.f);
      }
      __syncthreads();
      {
        const float* wr = a.W2 + (size_t)tid * MEL_PRENET_H;
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < MEL_PRENET_H; k += 4) {
          const float4 wv = *reinterpret_cast<const float4*>(wr + k);
          const float4 iv = *reinterpret_cast<const float4*>(sh + k);
          s = fmaf(wv.x, iv.x, s); s = fmaf(wv.y, iv.y, s); s = fmaf(wv.z, iv.z, s); s = fmaf(wv.w, iv.w, s);
        }
        sin_[tid] = fmaxf(s + a.b2[tid], 0.f);  // sin_ was last read in front of the barrier above
      }
      __syncthreads();
    }
    // a wave per row, K0 <= 256: one 16-byte load per lane and row, in registers since entry
    const bool lk = lane * 4 < K0;
    const float4 iv = lk ? *reinterpret_cast<const float4*>(sin_ + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < MEL_PR; ++j) {
      float s = 0.f;
      if (lk) { s = fmaf(w0[j].x, iv.x, s); s = fmaf(w0[j].y, iv.y, s); s = fmaf(w0[j].z, iv.z, s); s = fmaf(w0[j].w, iv.w, s); }
      s = wave_sum_dpp(s);
      const int r = lo + wave * MEL_PR + j;
      if (lane == 0 && r < hi) a.x[r] = add_scaled_2r(s + sb0[wave * MEL_PR + j], al, spe[wave * MEL_PR + j]);
    }
  }

  // ---- book-keeping: the workgroup that arrived last, i.e. behind every other workgroup's read of the state ----
  if (tid == 0) ss[7] = ticket == gridDim.x - 1 ? 1 : 0;
  __syncthreads();
  if (ss[7]) {
    if (row >= 0 && append && tid < MEL_BINS) a.frames[(size_t)n_gen * MEL_BINS + tid] = sf[tid];
    if (tid == 0) {
      ArState* st = a.st;
      if (row >= 0) {
        a.stops[pass] = stop;
        st->pass = pass + 1;
        if (append) st->n_gen = n_gen + 1;
        if (reason != VX_MEL_STOP_NONE) { st->done = 1; st->stop_reason = reason; }
      }
      if (go) st->row = row + 1;
      __hip_atomic_store(&a.ctl->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

void launch_mel_open(const MelStepArgs& a, hipStream_t s) { mel_open_kernel<<<MEL_GRID, 256, 0, s>>>(a); }

}  // namespace vx
