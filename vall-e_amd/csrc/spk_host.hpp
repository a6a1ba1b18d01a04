// The leaf pieces of the host side of the units built on spk_kernels.hpp (spk.hip, asr.hip, whisper.hip): the packing of one tensor
// of the handle's weight table (weights_host.hpp) for the row GEMM and the launches of the shared kernels.  What is built from them -
// the encoder layer, the Wav2Vec2 backbone, the handle scaffolding - is w2v_host.hpp, which the units include.  A handle type G has
// `std::map<std::string, HostW> w`, `std::vector<float> packed` and `bool finalized` (w2v_host.hpp's SpeechHandle).  Everything here
// has internal linkage: each unit launches its own copy of the kernels (they are `static` in spk_kernels.hpp).
#pragma once
#include <math.h>

#include "weights_host.hpp"
#include "spk_kernels.hpp"

namespace vx {
namespace {

// One row GEMM: the packed weight [groups][N][K] and bias as offsets into the device block, and the gather rule.
struct SpkLin {
  size_t w = 0, b = 0;
  bool has_bias = false;
  int C = 0, taps = 1, stride = 1, off0 = 0, step = 1, N = 0, groups = 1;
};
struct SpkNorm {
  size_t w = 0, b = 0;
};

template <class G>
SpkNorm pack_norm(G* g, const std::string& name) {
  SpkNorm n;
  n.w = push(g->packed, g->w[name + ".weight"].data);
  n.b = push(g->packed, g->w[name + ".bias"].data);
  return n;
}

// Linear (N, K): the torch layout is the GEMM's.
template <class G>
SpkLin pack_linear(G* g, const std::string& name, int N, int K) {
  SpkLin l;
  l.w = push(g->packed, g->w[name + ".weight"].data);
  l.b = push(g->packed, g->w[name + ".bias"].data);
  l.has_bias = true;
  l.C = K; l.N = N;
  return l;
}

// Conv1d (O, Cg, k) in `groups` groups: W[g][n][j * Cg + c] = w[g * (O / groups) + n][c][j].
template <class G>
SpkLin pack_conv(G* g, const std::string& name, int O, int Cg, int k, int groups, bool bias) {
  SpkLin l;
  l.w = push(g->packed, conv_rows(g->w[name + ".weight"].data.data(), O, Cg, k));
  l.has_bias = bias;
  if (bias) l.b = push(g->packed, g->w[name + ".bias"].data);
  l.C = Cg; l.taps = k; l.N = O / groups; l.groups = groups;
  return l;
}

int launch_gemm(const SpkGemmArgs& a, int groups, hipStream_t s) {
  if (a.M <= 0) return VX_OK;
  // float4 gathers: every operand address a multiple of 16 bytes (the caller's emb_out is the classifier's operand)
  const bool vec = a.C % 16 == 0 && a.ldx % 4 == 0 && a.xoff % 4 == 0 && a.xgs % 4 == 0 && (uintptr_t)a.x % 16 == 0;
  if (a.N <= 32) {
    dim3 g((unsigned)((a.M + 127) / 128), (unsigned)((a.N + 31) / 32), (unsigned)groups);
    if (vec) spk_gemm_rows<4, 1, true><<<g, 256, 0, s>>>(a);
    else spk_gemm_rows<4, 1, false><<<g, 256, 0, s>>>(a);
  } else {
    dim3 g((unsigned)((a.M + 63) / 64), (unsigned)((a.N + 63) / 64), (unsigned)groups);
    if (vec) spk_gemm_rows<2, 2, true><<<g, 256, 0, s>>>(a);
    else spk_gemm_rows<2, 2, false><<<g, 256, 0, s>>>(a);
  }
  HIPC(hipGetLastError());
  return VX_OK;
}

// One call's view of a handle's device state: the packed weights, the segment tables [n_tables][MB + 1] and the stream.
struct SpkCall {
  const float* W;
  const int* seg;
  int MB, n;
  hipStream_t s;
  float eps;  // layer_norm_eps
  const int* table(int i) const { return seg + (size_t)i * (MB + 1); }
};

// out rows (table t_out, M of them) = act(l(x rows of table t_in)); seg tables null: flat.
int run_lin(const SpkCall& x, const SpkLin& l, const float* in, int ldx, float* out, long M, int act, int t_out = -1, int t_in = -1) {
  SpkGemmArgs a{};
  a.x = in; a.ldx = ldx; a.xoff = 0; a.xgs = l.groups > 1 ? l.C : 0;
  a.C = l.C; a.taps = l.taps; a.stride = l.stride; a.off0 = l.off0; a.step = l.step;
  a.W = x.W + l.w; a.bias = l.has_bias ? x.W + l.b : nullptr;
  a.out = out; a.ldo = l.N * l.groups; a.act = act;
  a.M = M; a.N = l.N; a.K = l.taps * l.C;
  a.seg_out = t_out >= 0 ? x.table(t_out) : nullptr;
  a.seg_in = t_in >= 0 ? x.table(t_in) : nullptr;
  a.nseg = x.n;
  return launch_gemm(a, l.groups, x.s);
}

int run_ln(const SpkCall& x, const SpkNorm& nm, const float* a, const float* b, float* y, long M, int d, float* sum = nullptr,
           float lw = 0.f, int first = 0) {
  spk_layernorm<<<(unsigned)((M + 3) / 4), 256, 0, x.s>>>(a, b, x.W + nm.w, x.W + nm.b, y, sum, lw, first, M, d, x.eps);
  HIPC(hipGetLastError());
  return VX_OK;
}

template <int HD>
int launch_attn(const SpkAttnArgs& a, unsigned tiles, hipStream_t s) {
  spk_attention<HD><<<dim3(tiles, (unsigned)a.H), SPK_ATT_WAVES * 64, 0, s>>>(a);
  HIPC(hipGetLastError());
  return VX_OK;
}

// Attention over the rows of `seg` (hseg: its host copy), qkv rows [M][3 d] -> out rows [M][d].
int run_attn(const SpkCall& x, const int* seg, const int* hseg, const float* qkv, const float* gate, const float* table, float* out, int H,
             int d, int hd, int Tmax) {
  long qtiles = 0;
  for (int i = 0; i < x.n; ++i) qtiles += ((long)hseg[i + 1] - hseg[i] + 32 * SPK_ATT_WAVES - 1) / (32 * SPK_ATT_WAVES);
  SpkAttnArgs a{};
  a.qkv = qkv; a.gate = gate; a.table = table; a.out = out;
  a.seg = seg; a.nseg = x.n; a.H = H; a.d = d; a.Tmax = Tmax; a.scale = (float)(1.0 / sqrt((double)hd));
  if (hd == 16) return launch_attn<16>(a, (unsigned)qtiles, x.s);
  if (hd == 32) return launch_attn<32>(a, (unsigned)qtiles, x.s);
  return launch_attn<64>(a, (unsigned)qtiles, x.s);
}

}  // namespace
}  // namespace vx
