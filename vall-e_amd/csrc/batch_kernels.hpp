// Batched AR decode: up to 32 utterances ("slots") advance one token per step and share ONE stream of
// the 304 MB of weights (BASELINE configs[2]: padded per-slot KV cache, hipGraph-captured step).
// Per layer: ln_batch -> bgemm(QKV) -> attn_batch -> bgemm(out, partial) -> ln_batch(+partials) ->
// bgemm(FFN1) -> bgemm(FFN2, partial); the partial sums of the N = d GEMMs are reduced, in a fixed
// order, by the LayerNorm kernel that follows them anyway.  VALL-F layers insert their cross-attention after the second
// ln_batch: bgemm(query, BE_BIAS) -> attn_batch<MEM> over the slot's text memory -> bgemm(out, partial) -> ln_batch(+partials).
#pragma once
#include "common.hpp"
#include "ar_kernels.hpp"
#include "mfma_kernels.hpp"
#include "mx_kernels.hpp"

namespace vx {

constexpr int BMAX = 64;  // slots per engine (up to four 16-row MFMA halves)
typedef __bf16 bf16x8b_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// BE_LOGITS_MAP: BE_LOGITS for the rows of a batched prefill - A row z belongs to slot slot_map[z]
// BE_BIAS: q = A W^T + bias as fp32 rows (N columns), every row < B (the VALL-F cross-attention query)
enum BgemmEpi { BE_QKV = 0, BE_RELU = 1, BE_PARTIAL = 2, BE_LOGITS = 3, BE_LOGITS_MAP = 4, BE_BIAS = 5 };

struct BgemmArgs {
  const bf16* A;      // (32, K) activations, rows >= B hold finite stale values
  const bf16* W;      // (N, K)
  const float* bias;  // (N,) [BE_QKV, BE_RELU, BE_BIAS]
  int N, K, B;
  int kgroups;        // K split over workgroups (BE_PARTIAL); 1 otherwise
  const ArState* st;  // (32,) per-slot state
  // outputs
  float* q;           // BE_QKV: (32, d); BE_BIAS: (32, N)
  bf16* kv;           // BE_QKV: this layer's cache base of slot 0; slot stride kv_slot_stride elements
  size_t kv_slot_stride, kv_v_offset;  // elements
  int d, hd, ctx_max;
  bf16* f;            // BE_RELU: (32, N)
  float* part;        // BE_PARTIAL: (kgroups, 32, N)
  float* logits;      // BE_LOGITS: (32, logits_stride)
  int logits_stride;
  float* trace;       // BE_LOGITS, optional (VX_FLAG_TRACE_LOGITS): (slots, trace_rows, N) - row `pass` of every live slot
  int trace_rows;
  const int* slot_map;  // BE_LOGITS_MAP: (B,) slot of every A row
  // BE_QKV with fp8 slot caches (VX_FLAG_KV_FP8): this layer's code / scale bases of slot 0, indexed as `kv` (kv8s by index >> 4)
  uint8_t* kv8;
  uint8_t* kv8s;
};

// ---- fp8 slot caches (VX_FLAG_KV_FP8) ----------------------------------------------------------------------------------------
// Every K / V row of a head (64 channels) is four blocks of 16 consecutive channels; a block is 16 OCP e4m3 codes plus one E8M0
// scale byte (value = code x 2^(byte - 127)).  Codes sit at the bf16 cache's element index (one byte each), the block's scale at
// that index >> 4.  The source values are the bf16 values the bf16 cache would hold.  Mirrored by tests/kv8_ref.py.
// Scale: the smallest byte with amax <= 448 x 2^(byte - 127) - the MX rule (mx_block_scale) plus one where that rule would clip
// the block's largest element - so no value is clamped; the multiply by 2^(127 - byte) is exact and lands in [-448, 448].
__device__ __forceinline__ uint32_t kv8_block_scale(float amax, float& inv) {
  const uint32_t E = (__float_as_uint(amax) >> 23) & 0xffu;
  uint32_t byte = max(E, 8u) - 8u;
  if (amax * __uint_as_float((254u - byte) << 23) > 448.f) ++byte;
  inv = __uint_as_float((254u - byte) << 23);  // 2^(127 - byte)
  return byte;
}
// 2^(byte - 127) as an fp32 factor (byte 0: the subnormal 2^-127)
__device__ __forceinline__ float kv8_scale(uint32_t byte) { return __uint_as_float(byte ? byte << 23 : 0x00400000u); }
// one code, RNE (the argument is already scaled into [-448, 448])
__device__ __forceinline__ uint32_t kv8_code(float v) { return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.f, 0, false) & 0xffu; }
__device__ __forceinline__ void kv8_unpack(const uint4& r, float (&o)[16]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[k], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[k], true);
    o[4 * k] = lo[0]; o[4 * k + 1] = lo[1]; o[4 * k + 2] = hi[0]; o[4 * k + 3] = hi[1];
  }
}

// C[b][n] = sum_k A[b][k] W[n][k] on v_mfma_f32_16x16x32_bf16: one workgroup = one 16-row n tile (x one K
// group), its 4 waves take 4 K slices of NS steps and are summed through LDS in wave order.  Lane
// (c = l&15, g = l>>4) holds act[b = c (+16)][8g..8g+8) and W[n0 + c][8g..8g+8) of each 32-wide step; the
// accumulator has n on the lane and b = 4g + v in its 4 registers.
// The operands of the kernel's FIRST loads (A, W, sizes) are explicit leading arguments: with the build's
// `-amdgpu-kernarg-preload-count` they arrive in SGPRs at wave launch (hipcc does not preload by-value structs), so the weight
// and activation loads do not wait for a kernarg fetch.  nk = (N << 16) | K.
// KV8 (BE_QKV): K / V rows go to the fp8 slot caches (a.kv8 / a.kv8s) instead of the bf16 ones.
template <int EPI, int NS, int NH, bool KV8 = false>  // NH 16-row halves of slots: 2 (B <= 32) or 4 (B <= 64)
__global__ __launch_bounds__(256) void bgemm_kernel(const bf16* __restrict__ A_, const bf16* __restrict__ W_, unsigned nk, int kgroups,
                                                    const BgemmArgs a) {
  __shared__ float red[4][4 * NH][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int ntile = blockIdx.x / kgroups, kg = blockIdx.x - ntile * kgroups;
  const int n0 = ntile * 16;
  const int K = (int)(nk & 0xffffu), Nn = (int)(nk >> 16);
  const int kbeg = kg * (K / kgroups) + wave * NS * 32;
  const bf16* wp = W_ + (size_t)min(n0 + c, Nn - 1) * K + kbeg + 8 * g;
  const bf16* ap = A_ + (size_t)c * K + kbeg + 8 * g;
  // epilogue operands first (clamped, unconditional): fetched after the K loop they are one more exposed memory round trip
  float bias_v = 0.f;
  if (EPI == BE_QKV || EPI == BE_RELU || EPI == BE_BIAS) bias_v = a.bias[min(n0 + c, a.N - 1)];
  int st_done[NH], st_row[NH];  // st_row: KV row (BE_QKV) / pass index of the logits row being produced (BE_LOGITS trace)
#pragma unroll
  for (int u = 0; u < NH; ++u) {
    st_done[u] = 0; st_row[u] = 0;
    if (EPI == BE_QKV || EPI == BE_LOGITS || EPI == BE_LOGITS_MAP) {
      const int i = wave * NH + u, r = min(16 * (i >> 2) + 4 * g + (i & 3), a.B - 1);
      const int b = EPI == BE_LOGITS_MAP ? a.slot_map[r] : r;
      st_done[u] = a.st[b].done;
      st_row[u] = EPI == BE_QKV ? a.st[b].row : a.st[b].pass;
    }
  }
  bf16x8b_t wf[NS], af[NH][NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) wf[s] = *reinterpret_cast<const bf16x8b_t*>(wp + s * 32);
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int h = 0; h < NH; ++h) af[h][s] = *reinterpret_cast<const bf16x8b_t*>(ap + (size_t)16 * h * K + s * 32);
  f32x4_t acc[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) acc[h] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int h = 0; h < NH; ++h) acc[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[h][s], wf[s], acc[h], 0, 0, 0);
#pragma unroll
  for (int h = 0; h < NH; ++h)
#pragma unroll
    for (int v = 0; v < 4; ++v) red[wave][4 * h + v][lane] = acc[h][v];
  __syncthreads();
  // wave w finishes values {NH w, .., NH w + NH-1} of the 4 NH per lane: value i -> batch row b = 16*(i>>2) + 4g + (i&3)
  const int n = n0 + c;
#pragma unroll
  for (int u = 0; u < NH; ++u) {
    const int i = wave * NH + u;
    const float x = ((red[0][i][lane] + red[1][i][lane]) + red[2][i][lane]) + red[3][i][lane];
    const int b = 16 * (i >> 2) + 4 * g + (i & 3);
    // fp8 slot caches: the 16 lanes of this DPP row hold channels n0 .. n0 + 15 of slot b, i.e. one cache block.  Its scale is
    // reduced here, ahead of the branches below, whose conditions are uniform per row, so every lane of the row takes part.
    float k8v = 0.f;
    uint32_t k8s = 0;
    if constexpr (EPI == BE_QKV && KV8) {
      k8v = (float)(bf16)(x + bias_v);  // the value the bf16 cache would hold
      float am = group8_max_dpp(fabsf(k8v));
      am = fmaxf(am, dpp_f<0x140>(am, am));  // row_mirror: the other 8 lanes of the row
      float inv;
      k8s = kv8_block_scale(am, inv);
      k8v *= inv;
    }
    if (b >= a.B || n >= a.N) continue;
    if (EPI == BE_PARTIAL) {
      a.part[((size_t)kg * BMAX + b) * a.N + n] = x;
    } else if (EPI == BE_RELU) {
      a.f[(size_t)b * a.N + n] = (bf16)fmaxf(x + bias_v, 0.f);
    } else if (EPI == BE_BIAS) {
      a.q[(size_t)b * a.N + n] = x + bias_v;
    } else if (EPI == BE_LOGITS || EPI == BE_LOGITS_MAP) {
      const int sb = EPI == BE_LOGITS_MAP ? a.slot_map[b] : b;
      if (!st_done[u]) {
        a.logits[(size_t)sb * a.logits_stride + n] = x;
        if (a.trace != nullptr && st_row[u] < a.trace_rows) a.trace[((size_t)sb * a.trace_rows + st_row[u]) * a.N + n] = x;
      }
    } else {  // BE_QKV
      const float v = x + bias_v;
      const int sec = n / a.d, ii = n - sec * a.d;
      if (sec == 0) {
        a.q[(size_t)b * a.d + ii] = v;
      } else if (!st_done[u]) {
        const int h = ii / a.hd, cc = ii - h * a.hd;
        if constexpr (KV8) {
          const size_t at = (size_t)b * a.kv_slot_stride + (sec == 2 ? a.kv_v_offset : 0) + ((size_t)h * a.ctx_max + st_row[u]) * a.hd + cc;
          a.kv8[at] = (uint8_t)kv8_code(k8v);
          if (c == 0) a.kv8s[at >> 4] = (uint8_t)k8s;
        } else {
          bf16* base = a.kv + (size_t)b * a.kv_slot_stride + (sec == 2 ? a.kv_v_offset : 0);
          base[((size_t)h * a.ctx_max + st_row[u]) * a.hd + cc] = (bf16)v;
        }
      }
    }
  }
}

// x[b] += bias + sum_g part[g][b] (KG > 0; written back), then h[b] = bf16(LN(x[b]) * gamma + beta).
// One workgroup per slot, thread t owns columns [4t, 4t+4): every load of the kernel (x, bias, the KG partials,
// gamma, beta) is issued up front, so the kernel is one memory round trip plus two workgroup reductions.
// The body reads x row b and writes h row hb (b == hb on the step; ln_batch_map_kernel packs mapped slots into rows 0..n-1).
template <int KG>
__device__ __forceinline__ void ln_batch_body(float* __restrict__ x, const float* __restrict__ part, const float* __restrict__ pbias,
                                              const float* __restrict__ gamma, const float* __restrict__ beta, bf16* __restrict__ h,
                                              int d, int b, int hb) {
  __shared__ float red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool live = tid * 4 < d;
  const int k = live ? tid * 4 : 0;  // idle threads (d < 1024) load column 0 and contribute zeros
  float* xr = x + (size_t)b * d;
  float4 v = *reinterpret_cast<const float4*>(xr + k);
  const float4 gm = *reinterpret_cast<const float4*>(gamma + k);
  const float4 bt = *reinterpret_cast<const float4*>(beta + k);
  if (KG > 0) {
    float4 t = *reinterpret_cast<const float4*>(pbias + k);
    float4 p[KG > 0 ? KG : 1];
#pragma unroll
    for (int gi = 0; gi < KG; ++gi) p[gi] = *reinterpret_cast<const float4*>(part + ((size_t)gi * BMAX + b) * d + k);
#pragma unroll
    for (int gi = 0; gi < KG; ++gi) { t.x += p[gi].x; t.y += p[gi].y; t.z += p[gi].z; t.w += p[gi].w; }
    v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    if (live) *reinterpret_cast<float4*>(xr + k) = v;
  }
  if (!live) v = make_float4(0.f, 0.f, 0.f, 0.f);
  const float s = wave_sum_dpp((v.x + v.y) + (v.z + v.w));
  if (lane == 0) red[0][wave] = s;
  __syncthreads();
  const float mean = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)d;
  const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
  const float ss = wave_sum_dpp(live ? (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3) : 0.f);
  if (lane == 0) red[1][wave] = ss;
  __syncthreads();
  const float rstd = 1.0f / sqrtf(((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)d + LN_EPS);
  if (live) {
    union { bf16 e[4]; uint2 u; } pk;
    pk.e[0] = (bf16)(d0 * rstd * gm.x + bt.x);
    pk.e[1] = (bf16)(d1 * rstd * gm.y + bt.y);
    pk.e[2] = (bf16)(d2 * rstd * gm.z + bt.z);
    pk.e[3] = (bf16)(d3 * rstd * gm.w + bt.w);
    *reinterpret_cast<uint2*>(h + (size_t)hb * d + k) = pk.u;
  }
}
template <int KG>
__global__ __launch_bounds__(256) void ln_batch_kernel(float* __restrict__ x, const float* __restrict__ part,
                                                       const float* __restrict__ pbias, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, bf16* __restrict__ h, int d) {
  ln_batch_body<KG>(x, part, pbias, gamma, beta, h, d, blockIdx.x, blockIdx.x);
}
// Batched prefill: workgroup z normalises slot slot_map[z]'s row of x into row z of h (the A operand of
// the BE_LOGITS_MAP head).  x is only read.
__global__ __launch_bounds__(256) void ln_batch_map_kernel(float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, bf16* __restrict__ h, int d,
                                                           const int* __restrict__ slot_map) {
  ln_batch_body<0>(x, nullptr, nullptr, gamma, beta, h, d, slot_map[blockIdx.x], blockIdx.x);
}

// Single-query attention of every (slot, head): grid = (nhead, B), one workgroup walks all cached keys of its
// head (running max / sum across passes) and writes the normalised output as the bf16 A operand of the
// out-projection.  Same inner structure as attn_decode_kernel.
// MEM (VALL-F cross-attention): the keys are the slot's text memory, st[slot].S of them (kv / kv_slot_stride / ctx_max describe
// the memory buffer) instead of the st[slot].row + 1 cached self-attention keys.
template <int HD, bool MEM = false>
__global__ __launch_bounds__(256) void attn_batch_kernel(const float* __restrict__ q, const bf16* __restrict__ kv,
                                                         size_t kv_slot_stride, size_t kv_v_offset,
                                                         const ArState* __restrict__ st, int ctx_max, int d, float scale,
                                                         bf16* __restrict__ out) {
  constexpr int VEC = 8, LPK = HD / VEC, KPW = 64 / LPK, KPB = 4 * KPW, UNR = 4;
  __shared__ float sm_red[4];
  __shared__ __attribute__((aligned(16))) float sm_o[4 * KPW][HD + 1];
  __shared__ float sm_l[4 * KPW];
  const int h = blockIdx.x, slot = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane % LPK, grp = lane / LPK;
  const int done = st[slot].done;
  const int ctx = MEM ? st[slot].S : st[slot].row + 1;
  float qv[VEC];
#pragma unroll
  for (int i = 0; i < VEC; i += 4) {
    const float4 t = *reinterpret_cast<const float4*>(q + (size_t)slot * d + h * HD + sub * VEC + i);
    qv[i] = t.x; qv[i + 1] = t.y; qv[i + 2] = t.z; qv[i + 3] = t.w;
  }
  __builtin_amdgcn_sched_barrier(0);  // the q loads go out with the state's, not behind the branch on it
  // finished and vacant slots: nothing reads their output (their logits and KV rows are no longer written), so they skip the walk
  // over their cache and keep the finite row the last step wrote (zeros for a slot never filled).  Uniform per workgroup.
  if (done) return;
  const bf16* kb = kv + (size_t)slot * kv_slot_stride + (size_t)h * ctx_max * HD + sub * VEC;
  const bf16* vb = kb + kv_v_offset;
  float M = -INFINITY, L = 0.f, acc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
  constexpr int STEP = UNR * KPB;
  // Two register sets: the loads of pass p+1 are in flight while pass p is scored.  They are issued
  // unconditionally on clamped rows (the pass after the last re-reads the last key and is never scored), so the
  // loop body has no branch around a load and the waits stay counted.
  uint4 kr0[UNR], vr0[UNR], kr1[UNR], vr1[UNR];
  auto issue = [&](uint4 (&kr)[UNR], uint4 (&vr)[UNR], int base) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = min(base + u * KPB + wave * KPW + grp, ctx - 1);
      kr[u] = ld16(kb + (size_t)j * HD);
      vr[u] = ld16(vb + (size_t)j * HD);
    }
    __builtin_amdgcn_sched_barrier(0);  // keep the loads here, ahead of the scoring of the other set
  };
  auto score = [&](const uint4 (&kr)[UNR], const uint4 (&vr)[UNR], int base) {
    float sc[UNR], mloc = -INFINITY;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = base + u * KPB + wave * KPW + grp;
      float kf[VEC];
      unpack<bf16>(kr[u], kf);
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) dot = fmaf(kf[i], qv[i], dot);
      dot = group8_sum_dpp(dot);
      sc[u] = (j < ctx) ? dot * scale : -INFINITY;
      mloc = fmaxf(mloc, sc[u]);
    }
    // running maximum per WAVE (merged across the four waves once, at the end): a workgroup-wide maximum per pass cost two
    // barriers per 128 keys, and with them the waves' loads and arithmetic stopped overlapping each other's
    const float Mn = fmaxf(M, wave_max_dpp(mloc));
    const float corr = (M == -INFINITY) ? 0.f : expf(M - Mn);
    L *= corr;
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] *= corr;
    M = Mn;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      float vf[VEC];
      unpack<bf16>(vr[u], vf);
      const float p = (sc[u] == -INFINITY) ? 0.f : expf(sc[u] - M);
      L += p;
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = fmaf(p, vf[i], acc[i]);
    }
  };
  issue(kr0, vr0, 0);
  for (int base = 0;;) {
    issue(kr1, vr1, base + STEP);
    score(kr0, vr0, base);
    base += STEP;
    if (base >= ctx) break;
    issue(kr0, vr0, base + STEP);
    score(kr1, vr1, base);
    base += STEP;
    if (base >= ctx) break;
  }
  const int gi = wave * KPW + grp;
#pragma unroll
  for (int i = 0; i < VEC; ++i) sm_o[gi][sub * VEC + i] = acc[i];
  if (sub == 0) sm_l[gi] = L;
  if (lane == 0) sm_red[wave] = M;
  __syncthreads();
  if (tid < HD) {
    // every wave scored at least one live key (ctx >= 1 and the first pass covers key 0 in wave 0; a wave whose keys were all past
    // ctx has M = -inf, L = 0, acc = 0 and weight 0)
    const float Ma = fmaxf(fmaxf(sm_red[0], sm_red[1]), fmaxf(sm_red[2], sm_red[3]));
    float o = 0.f, l = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float wgt = (sm_red[w] == -INFINITY) ? 0.f : expf(sm_red[w] - Ma);
      float ow = 0.f, lw = 0.f;
#pragma unroll
      for (int gidx = 0; gidx < KPW; ++gidx) { ow += sm_o[w * KPW + gidx][tid]; lw += sm_l[w * KPW + gidx]; }
      o = fmaf(wgt, ow, o);
      l = fmaf(wgt, lw, l);
    }
    out[(size_t)slot * d + h * HD + tid] = (bf16)(o / l);
  }
}

// Prefill rows -> fp8 slot caches (the fp8 forms of kv_scatter_kernel / kv_scatter_seg_kernel): one thread per 16-channel block of
// a K or V row.  codes / scales: this layer's bases of slot 0 (or of the prefilled slot), indexed as in BgemmArgs.kv8 / kv8s.
// seg_start == nullptr: row j of the buffer -> position j of the slot at codes (grid.x = rows); otherwise row j of segment z ->
// position j of slot seg_slot[z] (grid = (max segment length, segments)).
__global__ __launch_bounds__(256) void kv8_scatter_kernel(const bf16* __restrict__ qkv, uint8_t* __restrict__ codes,
                                                          uint8_t* __restrict__ scales, size_t slot_stride, size_t v_offset,
                                                          const int* __restrict__ seg_start, const int* __restrict__ seg_len,
                                                          const int* __restrict__ seg_slot, int d, int ctx_max) {
  constexpr int HD = 64;
  const int j = blockIdx.x, z = blockIdx.y;
  size_t r = j, base = 0;
  if (seg_start != nullptr) {
    if (j >= seg_len[z]) return;
    r = (size_t)seg_start[z] + j;
    base = (size_t)seg_slot[z] * slot_stride;
  }
  const int nb = d / 16;  // blocks per K (or V) row
  for (int t = threadIdx.x; t < 2 * nb; t += blockDim.x) {
    const int sec = t >= nb, i = 16 * (t - sec * nb);
    const int h = i / HD, cc = i - h * HD;
    const bf16* src = qkv + r * 3 * d + (size_t)(1 + sec) * d + i;
    float f[2][8];
    unpack<bf16>(ld16(src), f[0]);
    unpack<bf16>(ld16(src + 8), f[1]);
    float am = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) am = fmaxf(am, fmaxf(fabsf(f[0][k]), fabsf(f[1][k])));
    float inv;
    const uint32_t sb = kv8_block_scale(am, inv);
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float* p = f[k >> 1] + 4 * (k & 1);
      int pk = __builtin_amdgcn_cvt_pk_fp8_f32(p[0] * inv, p[1] * inv, 0, false);
      pk = __builtin_amdgcn_cvt_pk_fp8_f32(p[2] * inv, p[3] * inv, pk, true);
      w[k] = (uint32_t)pk;
    }
    const size_t at = base + (sec ? v_offset : 0) + ((size_t)h * ctx_max + j) * HD + cc;
    *reinterpret_cast<uint4*>(codes + at) = make_uint4(w[0], w[1], w[2], w[3]);
    scales[at >> 4] = (uint8_t)sb;
  }
}

// attn_batch_kernel on the fp8 slot caches: one 16-byte load carries a key's 16-channel block, so 4 lanes hold a key and a wave
// scores 16 keys per pass.  The block scales (one byte per key and lane) multiply the lane's partial dot before the 4-lane sum
// (K) and the lane's softmax weight (V): both are exact power-of-two factors.
template <int HD>
__global__ __launch_bounds__(256) void attn_batch8_kernel(const float* __restrict__ q, const uint8_t* __restrict__ kv,
                                                          const uint8_t* __restrict__ kvs, size_t kv_slot_stride, size_t kv_v_offset,
                                                          const ArState* __restrict__ st, int ctx_max, int d, float scale,
                                                          bf16* __restrict__ out) {
  constexpr int VEC = 16, LPK = HD / VEC, KPW = 64 / LPK, KPB = 4 * KPW, UNR = 4;
  __shared__ float sm_red[4];
  __shared__ __attribute__((aligned(16))) float sm_o[4 * KPW][HD + 1];
  __shared__ float sm_l[4 * KPW];
  const int h = blockIdx.x, slot = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane % LPK, grp = lane / LPK;
  const int done = st[slot].done;
  const int ctx = st[slot].row + 1;
  float qv[VEC];
#pragma unroll
  for (int i = 0; i < VEC; i += 4) {
    const float4 t = *reinterpret_cast<const float4*>(q + (size_t)slot * d + h * HD + sub * VEC + i);
    qv[i] = t.x; qv[i + 1] = t.y; qv[i + 2] = t.z; qv[i + 3] = t.w;
  }
  __builtin_amdgcn_sched_barrier(0);
  if (done) return;  // finished and vacant slots, as attn_batch_kernel
  const size_t ko = (size_t)slot * kv_slot_stride + (size_t)h * ctx_max * HD;
  const uint8_t* kb = kv + ko + sub * VEC;
  const uint8_t* vb = kb + kv_v_offset;
  const uint8_t* ksb = kvs + (ko >> 4) + sub;
  const uint8_t* vsb = ksb + (kv_v_offset >> 4);
  float M = -INFINITY, L = 0.f, acc[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
  constexpr int STEP = UNR * KPB;
  // two register sets, clamped unconditional loads: as attn_batch_kernel
  uint4 kr0[UNR], vr0[UNR], kr1[UNR], vr1[UNR];
  uint32_t ks0[UNR], vs0[UNR], ks1[UNR], vs1[UNR];
  auto issue = [&](uint4 (&kr)[UNR], uint4 (&vr)[UNR], uint32_t (&ks)[UNR], uint32_t (&vs)[UNR], int base) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = min(base + u * KPB + wave * KPW + grp, ctx - 1);
      kr[u] = *reinterpret_cast<const uint4*>(kb + (size_t)j * HD);
      vr[u] = *reinterpret_cast<const uint4*>(vb + (size_t)j * HD);
      ks[u] = ksb[(size_t)j * (HD / 16)];
      vs[u] = vsb[(size_t)j * (HD / 16)];
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto score = [&](const uint4 (&kr)[UNR], const uint4 (&vr)[UNR], const uint32_t (&ks)[UNR], const uint32_t (&vs)[UNR], int base) {
    float sc[UNR], mloc = -INFINITY;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = base + u * KPB + wave * KPW + grp;
      float kf[VEC];
      kv8_unpack(kr[u], kf);
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) dot = fmaf(kf[i], qv[i], dot);
      dot = group4_sum_dpp(dot * kv8_scale(ks[u]));
      sc[u] = (j < ctx) ? dot * scale : -INFINITY;
      mloc = fmaxf(mloc, sc[u]);
    }
    const float Mn = fmaxf(M, wave_max_dpp(mloc));
    const float corr = (M == -INFINITY) ? 0.f : expf(M - Mn);
    L *= corr;
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] *= corr;
    M = Mn;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      float vf[VEC];
      kv8_unpack(vr[u], vf);
      const float p = (sc[u] == -INFINITY) ? 0.f : expf(sc[u] - M);
      L += p;
      const float pv = p * kv8_scale(vs[u]);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = fmaf(pv, vf[i], acc[i]);
    }
  };
  issue(kr0, vr0, ks0, vs0, 0);
  for (int base = 0;;) {
    issue(kr1, vr1, ks1, vs1, base + STEP);
    score(kr0, vr0, ks0, vs0, base);
    base += STEP;
    if (base >= ctx) break;
    issue(kr0, vr0, ks0, vs0, base + STEP);
    score(kr1, vr1, ks1, vs1, base);
    base += STEP;
    if (base >= ctx) break;
  }
  const int gi = wave * KPW + grp;
#pragma unroll
  for (int i = 0; i < VEC; ++i) sm_o[gi][sub * VEC + i] = acc[i];
  if (sub == 0) sm_l[gi] = L;
  if (lane == 0) sm_red[wave] = M;
  __syncthreads();
  if (tid < HD) {
    const float Ma = fmaxf(fmaxf(sm_red[0], sm_red[1]), fmaxf(sm_red[2], sm_red[3]));
    float o = 0.f, l = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float wgt = (sm_red[w] == -INFINITY) ? 0.f : expf(sm_red[w] - Ma);
      float ow = 0.f, lw = 0.f;
#pragma unroll
      for (int gidx = 0; gidx < KPW; ++gidx) { ow += sm_o[w * KPW + gidx][tid]; lw += sm_l[w * KPW + gidx]; }
      o = fmaf(wgt, ow, o);
      l = fmaf(wgt, lw, l);
    }
    out[(size_t)slot * d + h * HD + tid] = (bf16)(o / l);
  }
}

}  // namespace vx
