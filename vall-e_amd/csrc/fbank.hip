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
  // per call: wav pointers [max_batch] | out pointers [max_batch] | tile0 [max_batch + 1] | len | frames [max_batch each]
  CallStage stage;
};
}  // namespace

struct vx_fbank {
  int n_mels = 0, max_batch = 0;
  float clip = 0.f;
  std::vector<float> basis;  // [n_mels][513]
  std::vector<float> tab;    // window | cos | sin
  bool basis_dirty = true;   // the device copy is older than `basis`
  int device = -1;  // >= 0: `dev` is complete
  std::unique_ptr<FbankDev> dev;
};

namespace {

// First use: the tables go to the current device.
int fbank_init_device(vx_fbank* fb) {
  int dev = 0;
  HIPC(hipGetDevice(&dev));
  fb->device = dev;
  fb->dev.reset(new FbankDev());
  FbankDev& d = *fb->dev;
  const size_t MB = (size_t)fb->max_batch;
  VXC(d.tab.alloc(FBANK_TAB));
  VXC(d.basis_t.alloc((size_t)fb->n_mels * FBANK_BINS));
  VXC(d.band.alloc(2 * (size_t)fb->n_mels));
  VXC(d.stage.init(2 * MB * sizeof(void*) + (3 * MB + 1) * sizeof(int)));
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
  if (!cfg || !out) return fail(VX_ERR_ARG, "vx_fbank_create: null argument");
  if (cfg->struct_size != (int32_t)sizeof(vx_fbank_config))
    return fail(VX_ERR_ARG, "vx_fbank_create: struct_size %d, expected %zu", cfg->struct_size, sizeof(vx_fbank_config));
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
  fb->tab.resize(FBANK_TAB);
  const double pi = 3.14159265358979323846;
  for (int j = 0; j < 1024; ++j) {
    const double t = 2.0 * pi * (double)j / 1024.0;
    fb->tab[j] = (float)(0.5 - 0.5 * cos(t));  // periodic Hann
    fb->tab[1024 + j] = (float)cos(t);
    fb->tab[2048 + j] = (float)sin(t);
  }
  // the multiples of a quarter turn exactly (cos(pi / 2) in fp64 is 6e-17, not 0)
  fb->tab[1024 + 256] = 0.f; fb->tab[1024 + 768] = 0.f; fb->tab[2048 + 512] = 0.f;
  *out = fb;
  return VX_OK;
}

extern "C" void vx_fbank_destroy(vx_fbank* fb) {
  if (!fb) return;
  if (fb->device >= 0) {
    DevGuard g(fb->device);
    (void)fb->dev->stage.drain();
    fb->dev.reset();
  }
  delete fb;
}

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
  if (fb->device < 0) {
    const int rc = fbank_init_device(fb);
    if (rc != VX_OK) {  // a failed first use leaves the handle as it was before it
      fb->dev.reset();
      fb->device = -1;
      return rc;
    }
  }
  DevGuard g(fb->device);
  HIPC(g.err);
  FbankDev& d = *fb->dev;
  hipStream_t s = (hipStream_t)stream;
  if (fb->basis_dirty) {
    VXC(d.stage.drain());  // nothing reads the device copy of the basis any more
    VXC(fbank_upload_basis(fb));
  }
  VXC(d.stage.begin(s));
  const size_t MB = (size_t)fb->max_batch;
  const float** hin = d.stage.host<const float*>();
  float** hout = d.stage.host<float*>(MB * sizeof(void*));
  int* hint = d.stage.host<int>(2 * MB * sizeof(void*));
  for (int i = 0; i < n; ++i) {
    hin[i] = wav[i];
    hout[i] = out[i];
    hint[MB + 1 + i] = n_samples[i];
    hint[2 * MB + 1 + i] = frames[i];
  }
  memcpy(hint, tile0.data(), (n + 1) * sizeof(int));
  VXC(d.stage.upload(d.stage.bytes, s));
  FbankArgs a{};
  a.wav = d.stage.dev<const float* const>();
  a.out = d.stage.dev<float* const>(MB * sizeof(void*));
  const int* dint = d.stage.dev<const int>(2 * MB * sizeof(void*));
  a.tile0 = dint; a.len = dint + MB + 1; a.frames = dint + 2 * MB + 1;
  a.tab = d.tab.get(); a.basis_t = d.basis_t.get(); a.band = d.band.get();
  a.nseg = n; a.n_mels = fb->n_mels; a.clip = fb->clip;
  const unsigned grid = (unsigned)std::min(tile0[n], 4096);
  fbank_kernel<<<grid, 256, 0, s>>>(a);
  HIPC(hipGetLastError());
  return d.stage.finish(s);
}
