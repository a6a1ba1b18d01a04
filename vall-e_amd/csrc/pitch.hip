// Pitch tracking behind the C ABI (include/vallex.h, vx_pitch_*): the argument checks, the staging of a ragged call (CallStage,
// host.hpp) and the launches of pitch_kernels.hpp.  A translation unit and a handle of its own, like fbank.hip and dtw.hip: no
// other unit sees these kernels, so the device code of every existing path is compiled exactly as before.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#undef VX_STAMPS  // the in-kernel stamps write device globals of engine.hip's unit, out of this unit's reach
#include "host.hpp"
#include "pitch_kernels.hpp"

using namespace vx;

namespace {
// Device side of a handle: made on the device that is current at the first call, dropped as a whole.
struct PitchDev {
  // per call, vx_pitch_track: track_table();  vx_pitch_compare: PitchPair [max_batch].  One block, sized to the larger.
  CallStage stage;
  DevBuf<double> sums;  // [max_batch][PITCH_NSUMS]
};

enum { COL_WAV, COL_F0, COL_AP, COL_LAG, COL_VOICED, COL_DP, N_PTR_COLS };  // the track table's pointer columns
enum { COL_LEN, COL_FRAMES, N_INT_COLS };                                   // and its int columns

RaggedTable track_table(int max_batch) { return RaggedTable(max_batch, N_PTR_COLS, N_INT_COLS); }
}  // namespace

struct vx_pitch : LazyDev<PitchDev> {
  int tau_min = 0, tau_max = 0, max_frames = 0, max_batch = 0;
  float threshold = 0.f;
};

namespace {

int pitch_init_device(vx_pitch* h) {
  VXC(open_device(h));
  VXC(h->dev->stage.init(std::max(track_table(h->max_batch).bytes(), (size_t)h->max_batch * sizeof(PitchPair))));
  return h->dev->sums.alloc((size_t)h->max_batch * PITCH_NSUMS);
}

// tau_min = floor(24000 / fmax), tau_max = ceil(24000 / fmin), in fp64 on the fp32 arguments.
bool lag_range(float fmin, float fmax, int* tau_min, int* tau_max) {
  if (!(fmin > 0.f) || !(fmax > 0.f) || !isfinite(fmin) || !isfinite(fmax)) return false;
  const double lo = floor((double)PITCH_RATE / (double)fmax), hi = ceil((double)PITCH_RATE / (double)fmin);
  if (!(lo >= PITCH_TAU_LO) || !(hi <= PITCH_TAU_HI) || !(lo < hi)) return false;
  *tau_min = (int)lo;
  *tau_max = (int)hi;
  return true;
}

struct TrackCall {
  int32_t n;
  const float* const* wav;
  const int32_t* len;
  float* const* f0;
  float* const* ap;
  int32_t* const* lag;
  uint8_t* const* voiced;
  float* const* dp;
};

// The checks of a track call (before any HIP call) and its tiles; `who` names the entry point in the messages.
int track_check(const char* who, int max_batch, int max_frames, const TrackCall& c, std::vector<int>& tile0, std::vector<int>& frames) {
  if (!c.wav || !c.len) return fail(VX_ERR_ARG, "%s: null argument", who);
  if (c.n < 1) return fail(VX_ERR_ARG, "%s: n = %d utterances", who, c.n);
  if (c.n > max_batch) return fail(VX_ERR_CAPACITY, "%s: n = %d utterances > max_batch %d", who, c.n, max_batch);
  tile0.assign(c.n + 1, 0);
  frames.assign(c.n, 0);
  for (int i = 0; i < c.n; ++i) {
    if (!c.wav[i]) return fail(VX_ERR_ARG, "%s: utterance %d: null pointer", who, i);
    if (c.len[i] < 0) return fail(VX_ERR_ARG, "%s: utterance %d: %d samples", who, i, c.len[i]);
    const long long fr = ((long long)c.len[i] + PITCH_HOP / 2) / PITCH_HOP;
    if (fr > max_frames) return fail(VX_ERR_CAPACITY, "%s: utterance %d: %lld frames > max_frames %d", who, i, fr, max_frames);
    frames[i] = (int)fr;
    const long long tiles = tile0[i] + (fr + PITCH_TILE - 1) / PITCH_TILE;
    if (tiles > 0x7fffffffLL) return fail(VX_ERR_UNSUPPORTED, "%s: utterance %d: the call's tiles exceed int32", who, i);
    tile0[i + 1] = (int)tiles;
  }
  return VX_OK;
}

// Stages the call on `st` and launches; the caller has run track_check and begun the stage.
int track_launch(CallStage& st, int max_batch, int tau_min, int tau_max, float threshold, const TrackCall& c, const std::vector<int>& tile0,
                 const std::vector<int>& frames, hipStream_t s) {
  const RaggedTable t = track_table(max_batch);
  auto put = [&](int k, auto src) {  // an output the caller does not want: null pointers
    const void** hp = t.host_ptrs<const void*>(st, k);
    for (int i = 0; i < c.n; ++i) hp[i] = src ? src[i] : nullptr;
  };
  put(COL_WAV, c.wav); put(COL_F0, c.f0); put(COL_AP, c.ap); put(COL_LAG, c.lag); put(COL_VOICED, c.voiced); put(COL_DP, c.dp);
  memcpy(t.host_tile0(st), tile0.data(), (c.n + 1) * sizeof(int));
  memcpy(t.host_ints(st, COL_LEN), c.len, c.n * sizeof(int));
  memcpy(t.host_ints(st, COL_FRAMES), frames.data(), c.n * sizeof(int));
  VXC(st.upload(t.bytes(), s));
  PitchArgs a{};
  a.wav = t.dev_ptrs<const float* const>(st, COL_WAV);
  a.f0 = t.dev_ptrs<float* const>(st, COL_F0);
  a.ap = t.dev_ptrs<float* const>(st, COL_AP);
  a.lag = t.dev_ptrs<int* const>(st, COL_LAG);
  a.voiced = t.dev_ptrs<unsigned char* const>(st, COL_VOICED);
  a.dp = t.dev_ptrs<float* const>(st, COL_DP);
  a.tile0 = t.dev_tile0(st); a.len = t.dev_ints(st, COL_LEN); a.frames = t.dev_ints(st, COL_FRAMES);
  a.nseg = c.n; a.tau_min = tau_min; a.tau_max = tau_max; a.threshold = threshold;
  const unsigned grid = (unsigned)std::min(tile0[c.n], 1 << 16);
  pitch_track_kernel<<<grid, PITCH_WG, 0, s>>>(a);
  HIPC(hipGetLastError());
  return VX_OK;
}

}  // namespace

extern "C" int vx_pitch_create(const vx_pitch_config* cfg, vx_pitch** out) {
  VXC(create_head("vx_pitch_create", cfg, out));
  if (cfg->max_batch < 1) return fail(VX_ERR_ARG, "vx_pitch_create: max_batch = %d", cfg->max_batch);
  if (cfg->max_frames < 1) return fail(VX_ERR_ARG, "vx_pitch_create: max_frames = %d", cfg->max_frames);
  if (!(cfg->threshold > 0.f) || !isfinite(cfg->threshold))
    return fail(VX_ERR_ARG, "vx_pitch_create: threshold = %g (positive and finite)", cfg->threshold);
  if (cfg->sample_rate != PITCH_RATE) return fail(VX_ERR_UNSUPPORTED, "vx_pitch_create: %d Hz: %d is served", cfg->sample_rate, PITCH_RATE);
  int tau_min = 0, tau_max = 0;
  if (!lag_range(cfg->fmin_hz, cfg->fmax_hz, &tau_min, &tau_max))
    return fail(VX_ERR_UNSUPPORTED,
                "vx_pitch_create: %g .. %g Hz: lags floor(%d / fmax) = tau_min >= %d, ceil(%d / fmin) = tau_max <= %d, tau_min < tau_max are served",
                cfg->fmin_hz, cfg->fmax_hz, PITCH_RATE, PITCH_TAU_LO, PITCH_RATE, PITCH_TAU_HI);
  if (cfg->max_batch > PITCH_MAX_BATCH) return fail(VX_ERR_UNSUPPORTED, "vx_pitch_create: max_batch = %d > %d", cfg->max_batch, PITCH_MAX_BATCH);
  vx_pitch* h = new vx_pitch();
  h->tau_min = tau_min; h->tau_max = tau_max; h->threshold = cfg->threshold;
  h->max_frames = cfg->max_frames; h->max_batch = cfg->max_batch;
  *out = h;
  return VX_OK;
}

extern "C" void vx_pitch_destroy(vx_pitch* h) { destroy_handle(h); }

extern "C" int vx_pitch_lag_range(const vx_pitch* h, int32_t* tau_min, int32_t* tau_max) {
  if (!h || !tau_min || !tau_max) return fail(VX_ERR_ARG, "vx_pitch_lag_range: null argument");
  *tau_min = h->tau_min;
  *tau_max = h->tau_max;
  return VX_OK;
}

extern "C" int vx_pitch_track(vx_pitch* h, int32_t n, const float* const* wav, const int32_t* n_samples, float* const* f0,
                              float* const* aperiodicity, int32_t* const* lag, uint8_t* const* voiced, void* stream) {
  if (!h) return fail(VX_ERR_ARG, "vx_pitch_track: null argument");
  const TrackCall c{n, wav, n_samples, f0, aperiodicity, lag, voiced, nullptr};
  std::vector<int> tile0, frames;
  VXC(track_check("vx_pitch_track", h->max_batch, h->max_frames, c, tile0, frames));
  if (tile0[n] == 0) return VX_OK;  // no utterance has a frame: nothing to write
  VXC(ensure_device(h, pitch_init_device));
  ON_DEVICE(h->device);
  PitchDev& d = *h->dev;
  hipStream_t s = (hipStream_t)stream;
  VXC(d.stage.begin(s));
  VXC(track_launch(d.stage, h->max_batch, h->tau_min, h->tau_max, h->threshold, c, tile0, frames, s));
  return d.stage.finish(s);
}

extern "C" int vx_pitch_compare(vx_pitch* h, int32_t n, const float* const* f0_a, const int32_t* Ta, const float* const* f0_b,
                                const int32_t* Tb, const int32_t* const* path, const int32_t* path_len, double* sums, void* stream) {
  if (!h || !f0_a || !Ta || !f0_b || !Tb || !path || !path_len || !sums) return fail(VX_ERR_ARG, "vx_pitch_compare: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_pitch_compare: n = %d pairs", n);
  if (n > h->max_batch) return fail(VX_ERR_CAPACITY, "vx_pitch_compare: n = %d pairs > max_batch %d", n, h->max_batch);
  std::vector<PitchPair> ps(n);
  for (int i = 0; i < n; ++i) {
    if (!f0_a[i] || !f0_b[i] || !path[i]) return fail(VX_ERR_ARG, "vx_pitch_compare: pair %d: null pointer", i);
    if (Ta[i] < 1 || Tb[i] < 1 || path_len[i] < 1)
      return fail(VX_ERR_ARG, "vx_pitch_compare: pair %d: %d x %d frames, %d path cells", i, Ta[i], Tb[i], path_len[i]);
    if (Ta[i] > h->max_frames || Tb[i] > h->max_frames)
      return fail(VX_ERR_CAPACITY, "vx_pitch_compare: pair %d: %d x %d frames > max_frames %d", i, Ta[i], Tb[i], h->max_frames);
    if ((long long)path_len[i] > (long long)Ta[i] + Tb[i] - 1)
      return fail(VX_ERR_CAPACITY, "vx_pitch_compare: pair %d: %d path cells > Ta + Tb - 1 = %lld", i, path_len[i], (long long)Ta[i] + Tb[i] - 1);
    PitchPair& p = ps[i];
    p.fa = f0_a[i]; p.fb = f0_b[i]; p.path = path[i];
    p.Ta = Ta[i]; p.Tb = Tb[i]; p.plen = path_len[i]; p.pad_ = 0;
  }
  VXC(ensure_device(h, pitch_init_device));
  ON_DEVICE(h->device);
  PitchDev& d = *h->dev;
  hipStream_t s = (hipStream_t)stream;
  VXC(d.stage.begin(s));
  memcpy(d.stage.host<PitchPair>(), ps.data(), (size_t)n * sizeof(PitchPair));
  VXC(d.stage.upload((size_t)n * sizeof(PitchPair), s));
  pitch_compare_kernel<<<n, PITCH_WG, 0, s>>>(d.stage.dev<const PitchPair>(), d.sums.get());
  HIPC(hipGetLastError());
  const hipError_t e = hipMemcpyAsync(sums, d.sums.get(), (size_t)n * PITCH_NSUMS * sizeof(double), hipMemcpyDefault, s);
  VXC(d.stage.finish(s));
  HIPC(e);
  return VX_OK;
}

// d' of one utterance on caller data, with a stage of its own; synchronous.
extern "C" int vx_op_pitch_diff(float fmin_hz, float fmax_hz, const float* wav, int32_t n_samples, float* dprime, void* stream) {
  if (!wav || !dprime) return fail(VX_ERR_ARG, "vx_op_pitch_diff: null argument");
  int tau_min = 0, tau_max = 0;
  if (!lag_range(fmin_hz, fmax_hz, &tau_min, &tau_max)) return fail(VX_ERR_ARG, "vx_op_pitch_diff: %g .. %g Hz is not served", fmin_hz, fmax_hz);
  const float* wavs[1] = {wav};
  float* dps[1] = {dprime};
  const TrackCall c{1, wavs, &n_samples, nullptr, nullptr, nullptr, nullptr, dps};
  std::vector<int> tile0, frames;
  VXC(track_check("vx_op_pitch_diff", 1, 0x7fffffff, c, tile0, frames));
  if (tile0[1] == 0) return VX_OK;
  hipStream_t s = (hipStream_t)stream;
  CallStage st;
  VXC(st.init(track_table(1).bytes()));
  VXC(track_launch(st, 1, tau_min, tau_max, 1.f, c, tile0, frames, s));
  HIPC(hipStreamSynchronize(s));
  return VX_OK;
}
