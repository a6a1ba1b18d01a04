// The kernels of VX_FLAG_LOGPROBS (generation records the model's log-probability of every token it emits) and their launchers.
// A translation unit of its own on purpose: the engine's other device code is compiled without these instantiations in sight, so
// an engine without the flag runs bit for bit the kernels it ran before (with the sampler's LP instantiation in the same unit the
// compiler scheduled the plain one differently).  The engine picks the launcher on the host; nothing here is reached without the
// flag except through vx_op_sample_logprob.
#include <hip/hip_runtime.h>

#undef VX_STAMPS  // the in-kernel stamps write device globals of engine.hip's unit, out of this unit's reach: vx_create refuses the flag in a stamp build
#include "logprob.hpp"

namespace vx {

// sample_embed4_kernel (ar_kernels.hpp) on engines created with VX_FLAG_LOGPROBS, chosen on the host: the sampler body's LP
// instantiation, which also stores lp[slot * tok_stride + pass] next to `sampled`.  lp_eos: the token an EOS stop is scored at
// (1024 in the decode steps; < 0: always the sampled token, vx_op_sample_logprob).  Loads, bookkeeping and their order are a copy of that
// kernel's, line for line (its comments apply; change both together): moving them into a function both kernels call, by reference or
// by value, changed the instructions the compiler emits for the plain kernel.
template <int NVT, int NV0>
__global__ __launch_bounds__(256) void sample_embed4_lp_kernel(const SampleArgs a, float* lp, int lp_eos) {
  const int slot = blockIdx.x;
  ArState* st = a.st + slot;
  const int tid = threadIdx.x;
  const int V = a.V;
  const ArState s = *st;
  const unsigned epoch_old = a.epoch != nullptr ? *a.epoch : 0u;
  __builtin_amdgcn_sched_barrier(0);
  const float* lg = a.logits + (size_t)slot * a.logits_stride;
  float v[NVT], w0[NV0];
#pragma unroll
  for (int j = 0; j < NVT; ++j) v[j] = lg[min(j * 256 + tid, V - 1)];
  if (tid < 64) {  // wave 0
#pragma unroll
    for (int j = 0; j < NV0; ++j) w0[j] = lg[min(j * 64 + tid, V - 1)];
  }
  auto book = [&]() {
    if (a.epoch != nullptr && tid == 0) {
      const unsigned n = epoch_old + 1u;
      *a.epoch = n ? n : 1u;
    }
    if (a.zero_acc != nullptr) {
      *reinterpret_cast<uint4*>(a.zero_acc + 4 * tid) = make_uint4(0u, 0u, 0u, 0u);
      *reinterpret_cast<uint4*>(a.zero_acc + 4 * tid + 2) = make_uint4(0u, 0u, 0u, 0u);
    }
  };
  if (s.done) { book(); return; }  // uniform
  sample4_body<NVT, NV0, true>(a, st, s, v, w0, slot, book, lp, lp_eos);
}

// argmax_rows_kernel of engines created with VX_FLAG_LOGPROBS (chosen on the host): the same samples / codes, and conf[r] = the
// log-probability of the picked code, max(row) - logsumexp(row) = -log(sum(exp(row - max))).  N = 1024 logits per row, one wave
// per row, the row read once into registers; the argmax by the same first-index rule, the sum as in nll_rows_kernel: fp64,
// lane-local in ascending column order, then the butterfly over the 64 lanes, so a row's value depends neither on `rows` nor on
// where the row sits in the launch.  -inf entries add 0.
__global__ __launch_bounds__(256) void argmax_lp_rows_kernel(const float* __restrict__ logits, int rows,
                                                             long long* __restrict__ samples, long long* __restrict__ codes,
                                                             int Q, int col, float* __restrict__ conf) {
  constexpr int N = 1024, NV = N / 64;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;  // wave-uniform
  const float* row = logits + (size_t)r * N;
  float v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = row[i * 64 + lane];
  ValIdx best{-INFINITY, 0x7fffffff};
#pragma unroll
  for (int i = 0; i < NV; ++i) best = better(best, ValIdx{v[i], i * 64 + lane});
  best = wave_argmax(best);
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < NV; ++i) s += (double)expf(v[i] - best.v);  // exp(-inf) = 0
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, WAVE);
  if (lane == 0) {
    samples[r] = best.i;
    codes[(size_t)r * Q + col] = best.i;
    conf[r] = (float)(-log(s));
  }
}

// Loads this unit's code object now: the first use of the sampler would otherwise fall into the stream capture of the step graph,
// where the runtime must not allocate.
hipError_t logprob_load() {
  hipFuncAttributes fa;
  return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(sample_embed4_lp_kernel<5, 17>));
}

void launch_sample_lp(const SampleArgs& a, float* lp, int lp_eos, int slots, hipStream_t s) {
  sample_embed4_lp_kernel<5, 17><<<slots, 256, 0, s>>>(a, lp, lp_eos);
}

void launch_argmax_lp_rows(const float* logits, int rows, long long* samples, long long* codes, int Q, int col, float* conf,
                           hipStream_t s) {
  argmax_lp_rows_kernel<<<(rows + 3) / 4, 256, 0, s>>>(logits, rows, samples, codes, Q, col, conf);
}

}  // namespace vx
