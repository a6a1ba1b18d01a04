// The weight table of a handle that takes its tensors one by one (vx_*_set_weight) and packs them at vx_*_finalize: codec.hip,
// ganvoc.hip and, through spk_host.hpp, spk.hip, asr.hip and whisper.hip.  Host code only.  A handle type G has
// `std::map<std::string, HostW> w`, `bool finalized` and, where it packs, `std::vector<float> packed`.  A new weighted handle starts
// here:  add_key at create;  set_weight as its *_set_weight;  missing_tensor, then push / conv_rows into the packed block at finalize.
#pragma once
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "host.hpp"

namespace vx {
namespace {

struct HostW {
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool set = false, optional = false;
};

template <class G>
void add_key(G* g, const std::string& key, std::vector<int64_t> shape, bool optional = false) {
  HostW t;
  t.shape = std::move(shape);
  t.optional = optional;
  g->w[key] = std::move(t);
}

// The body of vx_*_set_weight (`what` names the handle in the messages: "vx_spk").
template <class G>
int set_weight(G* g, const char* what, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
  if (!g || !key || !data || !shape) return fail(VX_ERR_ARG, "%s_set_weight: null argument", what);
  if (g->finalized) return fail(VX_ERR_STATE, "%s_set_weight after %s_finalize", what, what);
  auto it = g->w.find(key);
  if (it == g->w.end()) return fail(VX_ERR_WEIGHTS, "unknown key %s", key);
  HostW& t = it->second;
  bool same = ndim == (int32_t)t.shape.size();
  size_t n = 1;
  for (size_t i = 0; same && i < t.shape.size(); ++i) {
    same = shape[i] == t.shape[i];
    n *= (size_t)t.shape[i];
  }
  if (!same) {
    std::string want, got;
    for (int64_t v : t.shape) want += (want.empty() ? "" : ", ") + std::to_string(v);
    for (int i = 0; i < ndim && i < 8; ++i) got += (got.empty() ? "" : ", ") + std::to_string(shape[i]);
    return fail(VX_ERR_WEIGHTS, "%s: shape (%s), expected (%s)", key, got.c_str(), want.c_str());
  }
  t.data.assign(data, data + n);
  t.set = true;
  return VX_OK;
}

// The opening of vx_*_finalize: refuses with the first required key that is unset.
template <class G>
int missing_tensor(const G* g) {
  for (auto& kv : g->w)
    if (!kv.second.set && !kv.second.optional) return fail(VX_ERR_WEIGHTS, "missing tensor %s", kv.first.c_str());
  return VX_OK;
}

// Appends v to the packed block at the next multiple of `align_floats` (4: a 16-byte boundary); returns where it starts.
size_t push(std::vector<float>& p, const std::vector<float>& v, size_t align_floats = 4) {
  p.resize((p.size() + align_floats - 1) / align_floats * align_floats, 0.f);
  const size_t at = p.size();
  p.insert(p.end(), v.begin(), v.end());
  return at;
}

// Conv1d (O, C, k) -> the rows of the row GEMMs: out[o][j * C + c] = w[o][c][j], tap j = 0 the oldest sample.
std::vector<float> conv_rows(const float* w, int O, int C, int k) {
  std::vector<float> p((size_t)O * C * k);
  for (int o = 0; o < O; ++o)
    for (int c = 0; c < C; ++c)
      for (int j = 0; j < k; ++j) p[((size_t)o * k + j) * C + c] = w[((size_t)o * C + c) * k + j];
  return p;
}

}  // namespace
}  // namespace vx
