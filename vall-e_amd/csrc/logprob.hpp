// Launchers of the VX_FLAG_LOGPROBS kernels (logprob.hip, a translation unit of its own: see there).
#pragma once
#include "ar_kernels.hpp"

namespace vx {

// Resolves the unit's kernels on the current device (vx_create with the flag: not inside a stream capture later).
__attribute__((visibility("hidden"))) hipError_t logprob_load();
// The decode step's sampler (sample_embed4_kernel<5, 17>, one workgroup per slot) in its LP instantiation: also stores
// lp[slot * a.tok_stride + pass].  lp_eos: the token an EOS stop is scored at, < 0: always the sampled token.
__attribute__((visibility("hidden"))) void launch_sample_lp(const SampleArgs& a, float* lp, int lp_eos, int slots, hipStream_t s);
// argmax_rows_kernel over `rows` rows of 1024 logits, and conf[r] = max(row) - logsumexp(row).
__attribute__((visibility("hidden"))) void launch_argmax_lp_rows(const float* logits, int rows, long long* samples, long long* codes,
                                                                 int Q, int col, float* conf, hipStream_t s);

}  // namespace vx
