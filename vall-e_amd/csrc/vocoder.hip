// Griffin-Lim vocoder behind the C ABI (include/vallex.h, vx_vocoder_*): the host tables (window, twiddles, the least-squares
// inverse of the mel basis), the staging of a ragged call (CallStage, host.hpp), the workspace and the launches of
// vocoder_kernels.hpp.  A translation unit and a handle of its own, like fbank.hip: no other unit sees these kernels, so the
// device code of every existing path is compiled exactly as before.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#undef VX_STAMPS  // the in-kernel stamps write device globals of engine.hip's unit, out of this unit's reach
#include "host.hpp"
#include "mel_basis.hpp"
#include "vocoder_kernels.hpp"

using namespace vx;

namespace {
// Device side of a handle: made on the device that is current at the first vx_vocoder_synthesize, dropped as a whole.
struct VocDev {
  DevBuf<float> tab, pinv_t;
  // one block, grown when a larger call arrives: mag [cap][513] | ang [cap][513][2] | tprev [cap][513][2] | frames [cap][1024]
  DevBuf<float> ws;
  long cap = 0;
  CallStage stage;  // per call: a RaggedTable of logmel | init | wav | phase pointers, tile0, frames | fr0
};
constexpr long VOC_WS_ROW = VOC_BINS * 5 + VOC_NFFT;  // floats per frame of the workspace

enum { COL_LOGMEL, COL_INIT, COL_WAV, COL_PHASE, N_PTR_COLS };  // the staged block's pointer columns
enum { COL_FRAMES, COL_FR0, N_INT_COLS };                       // and its int columns
}  // namespace

struct vx_vocoder : LazyDev<VocDev> {
  int n_mels = 0, max_batch = 0;
  long max_total_frames = 0;
  float env_floor = 0.f;
  std::vector<float> pinv;  // [513][n_mels]
  std::vector<float> tab;
  bool pinv_dirty = true;   // the device copy is older than `pinv`
};

namespace {

RaggedTable call_table(const vx_vocoder* v) { return RaggedTable(v->max_batch, N_PTR_COLS, N_INT_COLS); }

// P = B^T (B B^T)^-1 for B (M x 513), in fp64 by Cholesky of B B^T, rounded once: (513 x M).  False when B B^T has no factor
// (a pivot that is not positive, or below 1e-12 of its diagonal entry: the rows of B are linearly dependent to working accuracy).
bool mel_inverse(const std::vector<double>& B, int M, std::vector<float>& P) {
  std::vector<double> L((size_t)M * M, 0.0);
  for (int i = 0; i < M; ++i)
    for (int j = 0; j <= i; ++j) {
      double g = 0.0;
      for (int b = 0; b < VOC_BINS; ++b) g += B[(size_t)i * VOC_BINS + b] * B[(size_t)j * VOC_BINS + b];
      L[(size_t)i * M + j] = g;
    }
  for (int j = 0; j < M; ++j) {
    const double gjj = L[(size_t)j * M + j];
    double d = gjj;
    for (int k = 0; k < j; ++k) d -= L[(size_t)j * M + k] * L[(size_t)j * M + k];
    if (!isfinite(d) || !(d > 1e-12 * gjj)) return false;
    const double ljj = sqrt(d);
    L[(size_t)j * M + j] = ljj;
    for (int i = j + 1; i < M; ++i) {
      double v = L[(size_t)i * M + j];
      for (int k = 0; k < j; ++k) v -= L[(size_t)i * M + k] * L[(size_t)j * M + k];
      L[(size_t)i * M + j] = v / ljj;
    }
  }
  P.assign((size_t)VOC_BINS * M, 0.f);
  std::vector<double> x(M);
  for (int b = 0; b < VOC_BINS; ++b) {  // (L L^T) x = column b of B
    for (int i = 0; i < M; ++i) {
      double v = B[(size_t)i * VOC_BINS + b];
      for (int k = 0; k < i; ++k) v -= L[(size_t)i * M + k] * x[k];
      x[i] = v / L[(size_t)i * M + i];
    }
    for (int i = M - 1; i >= 0; --i) {
      double v = x[i];
      for (int k = i + 1; k < M; ++k) v -= L[(size_t)k * M + i] * x[k];
      x[i] = v / L[(size_t)i * M + i];
    }
    for (int i = 0; i < M; ++i) {
      if (!isfinite(x[i])) return false;
      P[(size_t)b * M + i] = (float)x[i];
    }
  }
  return true;
}

// First use: the tables go to the current device.
int voc_init_device(vx_vocoder* v) {
  VXC(open_device(v));
  VocDev& d = *v->dev;
  VXC(d.tab.alloc(VOC_TAB));
  VXC(d.pinv_t.alloc((size_t)v->n_mels * VOC_BINS));
  VXC(d.stage.init(call_table(v).bytes()));
  HIPC(hipMemcpy(d.tab.get(), v->tab.data(), VOC_TAB * sizeof(float), hipMemcpyHostToDevice));
  v->pinv_dirty = true;
  return VX_OK;
}

// The inverse filter-major.  A blocking copy: the previous call's kernels have been waited for.
int voc_upload_inverse(vx_vocoder* v) {
  const int M = v->n_mels;
  std::vector<float> t((size_t)M * VOC_BINS);
  for (int b = 0; b < VOC_BINS; ++b)
    for (int m = 0; m < M; ++m) t[(size_t)m * VOC_BINS + b] = v->pinv[(size_t)b * M + m];
  HIPC(hipMemcpy(v->dev->pinv_t.get(), t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
  v->pinv_dirty = false;
  return VX_OK;
}

int voc_synthesize(vx_vocoder* v, const char* who, int32_t n, const float* const* logmel, const int32_t* n_frames,
                   const float* const* init, int init_kind, int32_t n_iter, float momentum, float* const* wav_out,
                   float* const* phase_out, void* stream) {
  if (!v || !logmel || !n_frames || !wav_out) return fail(VX_ERR_ARG, "%s: null argument", who);
  if (n < 1) return fail(VX_ERR_ARG, "%s: n = %d utterances", who, n);
  if (n_iter < 0) return fail(VX_ERR_ARG, "%s: n_iter = %d", who, n_iter);
  if (!isfinite(momentum) || !(momentum >= 0.f) || !(momentum < 1.f))
    return fail(VX_ERR_ARG, "%s: momentum = %g outside [0, 1)", who, momentum);
  if (n > v->max_batch) return fail(VX_ERR_CAPACITY, "%s: n = %d utterances > max_batch %d", who, n, v->max_batch);
  std::vector<int> tile0(n + 1, 0), fr0(n, 0);
  long total = 0;
  for (int i = 0; i < n; ++i) {
    const int T = n_frames[i];
    if (T < 0) return fail(VX_ERR_ARG, "%s: utterance %d: %d frames", who, i, T);
    if (T > 0 && (!logmel[i] || !wav_out[i] || (init && !init[i]) || (phase_out && !phase_out[i])))
      return fail(VX_ERR_ARG, "%s: utterance %d: null pointer", who, i);
    fr0[i] = (int)total;
    total += T;
    if (total > v->max_total_frames)
      return fail(VX_ERR_CAPACITY, "%s: %ld frames up to utterance %d > max_total_frames %ld", who, total, i, v->max_total_frames);
  }
  if (total == 0) return VX_OK;  // no utterance has a frame: nothing to write
  VXC(ensure_device(v, voc_init_device));
  ON_DEVICE(v->device);
  VocDev& d = *v->dev;
  hipStream_t s = (hipStream_t)stream;
  if (v->pinv_dirty) {
    VXC(d.stage.drain());  // nothing reads the device copy of the inverse any more
    VXC(voc_upload_inverse(v));
  }
  if (total > d.cap) {
    VXC(d.stage.drain());  // nothing uses the old workspace any more
    const long cap = std::min((total + 1023) / 1024 * 1024, (v->max_total_frames + 3) / 4 * 4);  // a multiple of 4: 16-byte rows
    d.cap = 0;
    VXC(d.ws.alloc((size_t)cap * VOC_WS_ROW));
    d.cap = cap;
  }
  // few frames: tiles of 4, so that a single utterance still spreads over the CUs (the bits do not depend on the tile)
  const int tile = (total + VOC_TILE - 1) / VOC_TILE >= 2L * vx_cu_count() ? VOC_TILE : VOC_TILE_SMALL;
  for (int i = 0; i < n; ++i) tile0[i + 1] = tile0[i] + (n_frames[i] + tile - 1) / tile;
  VXC(d.stage.begin(s));
  const RaggedTable t = call_table(v);
  auto put = [&](int k, const float* const* src) {  // an optional column the caller left out: null pointers
    const float** hp = t.host_ptrs<const float*>(d.stage, k);
    for (int i = 0; i < n; ++i) hp[i] = src ? src[i] : nullptr;
  };
  put(COL_LOGMEL, logmel); put(COL_INIT, init); put(COL_WAV, wav_out); put(COL_PHASE, phase_out);
  memcpy(t.host_tile0(d.stage), tile0.data(), (n + 1) * sizeof(int));
  memcpy(t.host_ints(d.stage, COL_FRAMES), n_frames, n * sizeof(int));
  memcpy(t.host_ints(d.stage, COL_FR0), fr0.data(), n * sizeof(int));
  VXC(d.stage.upload(t.bytes(), s));
  VocArgs a{};
  a.logmel = t.dev_ptrs<const float* const>(d.stage, COL_LOGMEL);
  a.init = t.dev_ptrs<const float* const>(d.stage, COL_INIT);
  a.wav = t.dev_ptrs<float* const>(d.stage, COL_WAV);
  a.phase = t.dev_ptrs<float* const>(d.stage, COL_PHASE);
  a.tile0 = t.dev_tile0(d.stage); a.frames = t.dev_ints(d.stage, COL_FRAMES); a.fr0 = t.dev_ints(d.stage, COL_FR0);
  a.tab = d.tab.get(); a.pinv_t = d.pinv_t.get();
  a.mag = d.ws.get();
  a.ang = a.mag + d.cap * VOC_BINS;
  a.tprev = a.ang + d.cap * 2 * VOC_BINS;
  a.fr = a.tprev + d.cap * 2 * VOC_BINS;
  a.nseg = n; a.n_mels = v->n_mels; a.tile = tile;
  a.init_kind = init ? init_kind : VOC_INIT_NONE;
  a.has_phase = phase_out ? 1 : 0;
  a.env_floor = v->env_floor;
  a.mom = (float)((double)momentum / (1.0 + (double)momentum));
  const unsigned grid = (unsigned)std::min(tile0[n], 4096);
  voc_mag_kernel<<<grid, 256, 0, s>>>(a);
  for (int it = 0; it <= n_iter; ++it) {
    voc_frame_kernel<<<grid, 256, 0, s>>>(a);
    voc_analysis_kernel<<<grid, 256, 0, s>>>(a, it == 0, it == n_iter);
  }
  HIPC(hipGetLastError());
  return d.stage.finish(s);
}

}  // namespace

extern "C" int64_t vx_vocoder_samples(int64_t n_frames) { return n_frames < 0 ? 0 : n_frames * VOC_HOP; }

extern "C" int vx_vocoder_create(const vx_vocoder_config* cfg, vx_vocoder** out) {
  VXC(create_head("vx_vocoder_create", cfg, out));
  if (cfg->max_batch < 1) return fail(VX_ERR_ARG, "vx_vocoder_create: max_batch = %d", cfg->max_batch);
  if (cfg->max_total_frames < 1) return fail(VX_ERR_ARG, "vx_vocoder_create: max_total_frames = %d", cfg->max_total_frames);
  if (!(cfg->env_floor > 0.f) || !isfinite(cfg->env_floor))
    return fail(VX_ERR_ARG, "vx_vocoder_create: env_floor = %g (the floor under the window envelope is positive)", cfg->env_floor);
  if (cfg->sample_rate != 24000 || cfg->n_fft != VOC_NFFT || cfg->hop != VOC_HOP)
    return fail(VX_ERR_UNSUPPORTED, "vx_vocoder_create: %d Hz, n_fft %d, hop %d: 24000 / %d / %d is served", cfg->sample_rate,
                cfg->n_fft, cfg->hop, VOC_NFFT, VOC_HOP);
  if (cfg->n_mels < 1 || cfg->n_mels > VOC_MAX_MELS)
    return fail(VX_ERR_UNSUPPORTED, "vx_vocoder_create: n_mels = %d outside [1, %d]", cfg->n_mels, VOC_MAX_MELS);
  if (!(cfg->fmin >= 0.f) || !(cfg->fmin < cfg->fmax) || !(cfg->fmax <= 12000.f))
    return fail(VX_ERR_UNSUPPORTED, "vx_vocoder_create: band %g .. %g Hz: 0 <= fmin < fmax <= 12000 is served", cfg->fmin, cfg->fmax);
  // 2^31 / (2 x 513) rows keep every cell index of a row pointer's offset arithmetic far inside int64 and fr0 inside int32
  if (cfg->max_total_frames > (1 << 21))
    return fail(VX_ERR_UNSUPPORTED, "vx_vocoder_create: max_total_frames = %d > %d", cfg->max_total_frames, 1 << 21);
  std::unique_ptr<vx_vocoder> v(new vx_vocoder());
  v->n_mels = cfg->n_mels; v->max_batch = cfg->max_batch; v->max_total_frames = cfg->max_total_frames;
  v->env_floor = cfg->env_floor;
  if (!mel_inverse(slaney_basis_f64(cfg->sample_rate, cfg->n_mels, VOC_BINS, cfg->fmin, cfg->fmax), cfg->n_mels, v->pinv))
    return fail(VX_ERR_UNSUPPORTED, "vx_vocoder_create: the built-in basis of %d filters in %g .. %g Hz has linearly dependent "
                "filters (B B^T has no Cholesky factor)", cfg->n_mels, cfg->fmin, cfg->fmax);
  v->tab = hann_cos_sin_1024();
  v->tab.resize(VOC_TAB);
  const double pi = 3.14159265358979323846;
  for (int j = 0; j < 1024; ++j) {  // the synthesis window and the envelope's term, from the window in fp64
    const double w = 0.5 - 0.5 * cos(2.0 * pi * (double)j / 1024.0);
    v->tab[3072 + j] = (float)(w / 1024.0);
    v->tab[4096 + j] = (float)(w * w);
  }
  *out = v.release();
  return VX_OK;
}

extern "C" void vx_vocoder_destroy(vx_vocoder* v) { destroy_handle(v); }

extern "C" int vx_vocoder_set_mel_basis(vx_vocoder* v, const float* basis) {
  if (!v || !basis) return fail(VX_ERR_ARG, "vx_vocoder_set_mel_basis: null argument");
  std::vector<double> B(basis, basis + (size_t)v->n_mels * VOC_BINS);
  std::vector<float> P;
  if (!mel_inverse(B, v->n_mels, P))
    return fail(VX_ERR_UNSUPPORTED, "vx_vocoder_set_mel_basis: B B^T has no Cholesky factor (linearly dependent or non-finite "
                "filters): pass the inverse of your choice to vx_vocoder_set_inverse");
  v->pinv.swap(P);
  v->pinv_dirty = true;
  return VX_OK;
}

extern "C" int vx_vocoder_set_inverse(vx_vocoder* v, const float* inverse) {
  if (!v || !inverse) return fail(VX_ERR_ARG, "vx_vocoder_set_inverse: null argument");
  v->pinv.assign(inverse, inverse + (size_t)VOC_BINS * v->n_mels);
  v->pinv_dirty = true;
  return VX_OK;
}

extern "C" int vx_vocoder_get_inverse(const vx_vocoder* v, float* inverse) {
  if (!v || !inverse) return fail(VX_ERR_ARG, "vx_vocoder_get_inverse: null argument");
  memcpy(inverse, v->pinv.data(), v->pinv.size() * sizeof(float));
  return VX_OK;
}

extern "C" int vx_vocoder_synthesize(vx_vocoder* v, int32_t n, const float* const* logmel, const int32_t* n_frames,
                                     const float* const* init_phase, int32_t n_iter, float momentum, float* const* wav_out,
                                     float* const* phase_out, void* stream) {
  return voc_synthesize(v, "vx_vocoder_synthesize", n, logmel, n_frames, init_phase, VOC_INIT_RADIANS, n_iter, momentum, wav_out,
                        phase_out, stream);
}

extern "C" int vx_vocoder_synthesize_warm(vx_vocoder* v, int32_t n, const float* const* logmel, const int32_t* n_frames,
                                          const float* const* init_ang, int32_t n_iter, float momentum, float* const* wav_out,
                                          float* const* phase_out, void* stream) {
  if (!init_ang) return fail(VX_ERR_ARG, "vx_vocoder_synthesize_warm: null argument");
  return voc_synthesize(v, "vx_vocoder_synthesize_warm", n, logmel, n_frames, init_ang, VOC_INIT_UNIT, n_iter, momentum, wav_out,
                        phase_out, stream);
}
