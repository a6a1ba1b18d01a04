// Log-mel filterbank behind the C ABI (include/vallex.h, vx_fbank_*): the host tables, the staging of a ragged call (CallStage,
// host.hpp) and the one launch of fbank_kernels.hpp.  A translation unit and a handle of its own, like logprob.hip and align.hip: no other unit sees
// this kernel, so the device code of every existing path is compiled exactly as before.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#undef VX_STAMPS  // the in-kernel stamps write device globals of engine.hip's unit, out of this unit's reach
#include "host.hpp"
#include "mel_basis.hpp"
#include "fbank_kernels.hpp"

using namespace vx;

namespace {
// Device side of a handle: made on the device that is current at the first vx_fbank_extract, dropped as a whole.
struct FbankDev {
  DevBuf<float> tab, basis_t;
  DevBuf<int> band;
  CallStage stage;  // per call: a RaggedTable of wav | out pointers, tile0, len | frames
};
}  // namespace

struct vx_fbank : LazyDev<FbankDev> {
  int n_mels = 0, max_batch = 0;
  float clip = 0.f;
  std::vector<float> basis;  // [n_mels][513]
  std::vector<float> tab;    // window | cos | sin
  bool basis_dirty = true;   // the device copy is older than `basis`
};

namespace {

enum { COL_WAV, COL_OUT, N_PTR_COLS };  // the staged block's pointer columns
enum { COL_LEN, COL_FRAMES, N_INT_COLS };  // and its int columns

RaggedTable call_table(const vx_fbank* fb) { return RaggedTable(fb->max_batch, N_PTR_COLS, N_INT_COLS); }

// First use: the tables go to the current device.
int fbank_init_device(vx_fbank* fb) {
  VXC(open_device(fb));
  FbankDev& d = *fb->dev;
  VXC(d.tab.alloc(FBANK_TAB));
  VXC(d.basis_t.alloc((size_t)fb->n_mels * FBANK_BINS));
  VXC(d.band.alloc(2 * (size_t)fb->n_mels));
  VXC(d.stage.init(call_table(fb).bytes()));
  HIPC(hipMemcpy(d.tab.get(), fb->tab.data(), FBANK_TAB * sizeof(float), hipMemcpyHostToDevice));
  fb->basis_dirty = true;
  return VX_OK;
}

// The basis bin-major and every filter's band.  Blocking copies: the previous call's kernel has been waited for.
int fbank_upload_basis(vx_fbank* fb) {
  const int M = fb->n_mels;
  std::vector<float> t((size_t)FBANK_BINS * M);
  std::vector<int> band(2 * (size_t)M);
  for (int m = 0; m < M; ++m) {
    int lo = FBANK_BINS, hi = -1;
    for (int b = 0; b < FBANK_BINS; ++b) {
      const float v = fb->basis[(size_t)m * FBANK_BINS + b];
      t[(size_t)b * M + m] = v;
      if (v != 0.f) { lo = std::min(lo, b); hi = b; }  // a NaN weight is non-zero: it reaches the sum
    }
    band[m] = hi < 0 ? 0 : lo;
    band[M + m] = hi;
  }
  HIPC(hipMemcpy(fb->dev->basis_t.get(), t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(fb->dev->band.get(), band.data(), band.size() * sizeof(int), hipMemcpyHostToDevice));
  fb->basis_dirty = false;
  return VX_OK;
}

}  // namespace

extern "C" int64_t vx_fbank_frames(int64_t n_samples) {
  return n_samples < 0 ? 0 : (n_samples + FBANK_HOP / 2) / FBANK_HOP;
}

extern "C" int vx_fbank_create(const vx_fbank_config* cfg, vx_fbank** out) {
  VXC(create_head("vx_fbank_create", cfg, out));
  if (cfg->max_batch < 1) return fail(VX_ERR_ARG, "vx_fbank_create: max_batch = %d", cfg->max_batch);
  if (!(cfg->clip > 0.f) || !isfinite(cfg->clip)) return fail(VX_ERR_ARG, "vx_fbank_create: clip = %g (the floor under the log is positive)", cfg->clip);
  if (cfg->sample_rate != 24000 || cfg->n_fft != FBANK_NFFT || cfg->hop != FBANK_HOP)
    return fail(VX_ERR_UNSUPPORTED, "vx_fbank_create: %d Hz, n_fft %d, hop %d: 24000 / %d / %d is served", cfg->sample_rate, cfg->n_fft,
                 cfg->hop, FBANK_NFFT, FBANK_HOP);
  if (cfg->n_mels < 1 || cfg->n_mels > FBANK_MAX_MELS)
    return fail(VX_ERR_UNSUPPORTED, "vx_fbank_create: n_mels = %d outside [1, %d]", cfg->n_mels, FBANK_MAX_MELS);
  if (!(cfg->fmin >= 0.f) || !(cfg->fmin < cfg->fmax) || !(cfg->fmax <= 12000.f))
    return fail(VX_ERR_UNSUPPORTED, "vx_fbank_create: band %g .. %g Hz: 0 <= fmin < fmax <= 12000 is served", cfg->fmin, cfg->fmax);
  vx_fbank* fb = new vx_fbank();
  fb->n_mels = cfg->n_mels; fb->max_batch = cfg->max_batch; fb->clip = cfg->clip;
  fb->basis = slaney_basis(cfg->sample_rate, cfg->n_mels, FBANK_BINS, cfg->fmin, cfg->fmax);
  fb->tab = hann_cos_sin_1024();
  *out = fb;
  return VX_OK;
}

extern "C" void vx_fbank_destroy(vx_fbank* fb) { destroy_handle(fb); }

extern "C" int vx_fbank_set_mel_basis(vx_fbank* fb, const float* basis) {
  if (!fb || !basis) return fail(VX_ERR_ARG, "vx_fbank_set_mel_basis: null argument");
  fb->basis.assign(basis, basis + (size_t)fb->n_mels * FBANK_BINS);
  fb->basis_dirty = true;
  return VX_OK;
}

extern "C" int vx_fbank_get_mel_basis(const vx_fbank* fb, float* basis) {
  if (!fb || !basis) return fail(VX_ERR_ARG, "vx_fbank_get_mel_basis: null argument");
  memcpy(basis, fb->basis.data(), fb->basis.size() * sizeof(float));
  return VX_OK;
}

extern "C" int vx_fbank_extract(vx_fbank* fb, int32_t n, const float* const* wav, const int32_t* n_samples, float* const* out,
                                void* stream) {
  if (!fb || !wav || !n_samples || !out) return fail(VX_ERR_ARG, "vx_fbank_extract: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_fbank_extract: n = %d utterances", n);
  if (n > fb->max_batch) return fail(VX_ERR_CAPACITY, "vx_fbank_extract: n = %d utterances > max_batch %d", n, fb->max_batch);
  std::vector<int> tile0(n + 1, 0), frames(n);
  for (int i = 0; i < n; ++i) {
    if (!wav[i] || !out[i]) return fail(VX_ERR_ARG, "vx_fbank_extract: utterance %d: null pointer", i);
    if (n_samples[i] < 1) return fail(VX_ERR_ARG, "vx_fbank_extract: utterance %d: %d samples", i, n_samples[i]);
    frames[i] = (int)vx_fbank_frames(n_samples[i]);
    const long tiles = tile0[i] + ((long)frames[i] + FBANK_TILE - 1) / FBANK_TILE;
    if (tiles > 0x7fffffffL) return fail(VX_ERR_UNSUPPORTED, "vx_fbank_extract: utterance %d: the call's tiles exceed int32", i);
    tile0[i + 1] = (int)tiles;
  }
  if (tile0[n] == 0) return VX_OK;  // no utterance has a frame: nothing to write
  VXC(ensure_device(fb, fbank_init_device));
  ON_DEVICE(fb->device);
  FbankDev& d = *fb->dev;
  hipStream_t s = (hipStream_t)stream;
  if (fb->basis_dirty) {
    VXC(d.stage.drain());  // nothing reads the device copy of the basis any more
    VXC(fbank_upload_basis(fb));
  }
  VXC(d.stage.begin(s));
  const RaggedTable t = call_table(fb);
  memcpy(t.host_ptrs<const float*>(d.stage, COL_WAV), wav, n * sizeof(float*));
  memcpy(t.host_ptrs<float*>(d.stage, COL_OUT), out, n * sizeof(float*));
  memcpy(t.host_tile0(d.stage), tile0.data(), (n + 1) * sizeof(int));
  memcpy(t.host_ints(d.stage, COL_LEN), n_samples, n * sizeof(int));
  memcpy(t.host_ints(d.stage, COL_FRAMES), frames.data(), n * sizeof(int));
  VXC(d.stage.upload(t.bytes(), s));
  FbankArgs a{};
  a.wav = t.dev_ptrs<const float* const>(d.stage, COL_WAV);
  a.out = t.dev_ptrs<float* const>(d.stage, COL_OUT);
  a.tile0 = t.dev_tile0(d.stage); a.len = t.dev_ints(d.stage, COL_LEN); a.frames = t.dev_ints(d.stage, COL_FRAMES);
  a.tab = d.tab.get(); a.basis_t = d.basis_t.get(); a.band = d.band.get();
  a.nseg = n; a.n_mels = fb->n_mels; a.clip = fb->clip;
  const unsigned grid = (unsigned)std::min(tile0[n], 4096);
  fbank_kernel<<<grid, 256, 0, s>>>(a);
  HIPC(hipGetLastError());
  return d.stage.finish(s);
}
