// The multi-resolution STFT distance behind the C ABI (include/vallex.h, vx_stft_*): the argument checks, the host-built tables,
// the staging of a ragged call (CallStage, host.hpp) and the launches of stft_kernels.hpp.  A translation unit and a handle of
// its own, like fbank.hip, dtw.hip and pitch.hip: no other unit sees these kernels, so the device code of every existing path is
// compiled exactly as before.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#undef VX_STAMPS  // the in-kernel stamps write device globals of engine.hip's unit, out of this unit's reach
#include "host.hpp"
#include "stft_kernels.hpp"

using namespace vx;

namespace {
struct Res {
  int n_fft = 0, hop = 0, win = 0, win_pad = 0, off = 0;
};

// Device side of a handle: made on the device that is current at the first call, dropped as a whole.
struct StftDev {
  // per call: x [MB] | y or out [MB] pointers, then ints: len [MB] | per resolution tile0 [MB + 1], frames [MB] | tbeg, tend
  // [MB * R] | doubles: cells [MB * R]
  CallStage stage;
  DevBuf<float> tab[STFT_MAX_RES], win[STFT_MAX_RES];
  DevBuf<double> ws;    // [workgroups of a full call][3]
  DevBuf<double> sums;  // [max_batch][n_res][4]
};
}  // namespace

struct vx_stft : LazyDev<StftDev> {
  int n_res = 0, max_samples = 0, max_batch = 0, max_nfft = 0;
  Res res[STFT_MAX_RES];
  float eps = 0.f;
};

namespace {

long long frames_of(const Res& r, long long L) { return 1 + L / r.hop; }

int groups_of(const Res& r) { return r.n_fft / (64 * STFT_GROUP); }  // workgroups per tile

long long tiles_of(const Res& r, long long frames, bool compare) {
  const int ft = stft_tile_frames(compare, r.hop, r.win_pad);
  return (frames + ft - 1) / ft;
}

// Byte offsets of the staging block.  Not a RaggedTable: tile0 | frames repeat per resolution, and tbeg, tend and the fp64 cells
// follow them.
struct Layout {
  size_t ptr_y, ints, res0, res_stride, tbeg, tend, cells, bytes;
  Layout(int max_batch, int n_res) {
    const size_t MB = (size_t)max_batch, R = (size_t)n_res;
    ptr_y = MB * sizeof(void*);
    ints = 2 * MB * sizeof(void*);
    res0 = ints + MB * sizeof(int);
    res_stride = (2 * MB + 1) * sizeof(int);
    tbeg = res0 + R * res_stride;
    tend = tbeg + MB * R * sizeof(int);
    cells = (tend + MB * R * sizeof(int) + 7) & ~(size_t)7;
    bytes = cells + MB * R * sizeof(double);
  }
};

int stft_init_device(vx_stft* h) {
  VXC(open_device(h));
  StftDev& d = *h->dev;
  VXC(d.stage.init(Layout(h->max_batch, h->n_res).bytes));
  long long tiles = 0;
  for (int r = 0; r < h->n_res; ++r) {
    const Res& g = h->res[r];
    tiles += (long long)h->max_batch * tiles_of(g, frames_of(g, h->max_samples), true) * groups_of(g);
    // tables in fp64, rounded once
    std::vector<float> tab(g.n_fft), win(g.win_pad, 0.f);
    for (int m = 0; m < g.n_fft; ++m) tab[m] = (float)cos(2.0 * M_PI * (double)m / (double)g.n_fft);
    for (int j = 0; j < g.win; ++j) win[j] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)j / (double)g.win));
    VXC(d.tab[r].alloc(tab.size()));
    VXC(d.win[r].alloc(win.size()));
    HIPC(hipMemcpy(d.tab[r].get(), tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d.win[r].get(), win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  VXC(d.ws.alloc((size_t)tiles * 3));
  VXC(d.sums.alloc((size_t)h->max_batch * h->n_res * 4));
  return VX_OK;
}

StftArgs args_of(const vx_stft* h, int r, int n, bool compare, const Layout& lay) {
  const StftDev& d = *h->dev;
  const Res& g = h->res[r];
  const size_t MB = (size_t)h->max_batch;
  StftArgs a{};
  a.x = d.stage.dev<const float* const>();
  a.y = d.stage.dev<const float* const>(lay.ptr_y);
  a.out = d.stage.dev<float* const>(lay.ptr_y);
  a.len = d.stage.dev<const int>(lay.ints);
  a.tile0 = d.stage.dev<const int>(lay.res0 + (size_t)r * lay.res_stride);
  a.frames = a.tile0 + MB + 1;
  a.tab = d.tab[r].get();
  a.win = d.win[r].get();
  a.ws = d.ws.get();
  a.nseg = n; a.n_fft = g.n_fft; a.hop = g.hop; a.win_pad = g.win_pad; a.off = g.off;
  a.ft = stft_tile_frames(compare, g.hop, g.win_pad);
  a.pad = stft_pad(g.hop);
  a.tile_base = 0;
  a.eps = h->eps;
  return a;
}

}  // namespace

extern "C" int vx_stft_create(const vx_stft_config* cfg, vx_stft** out) {
  VXC(create_head("vx_stft_create", cfg, out));
  if (cfg->max_batch < 1) return fail(VX_ERR_ARG, "vx_stft_create: max_batch = %d", cfg->max_batch);
  if (cfg->max_samples < 1) return fail(VX_ERR_ARG, "vx_stft_create: max_samples = %d", cfg->max_samples);
  if (!(cfg->eps > 0.f) || !isfinite(cfg->eps)) return fail(VX_ERR_ARG, "vx_stft_create: eps = %g (positive and finite)", cfg->eps);
  if (cfg->sample_rate != STFT_RATE) return fail(VX_ERR_UNSUPPORTED, "vx_stft_create: %d Hz: %d is served", cfg->sample_rate, STFT_RATE);
  if (cfg->n_res < 1 || cfg->n_res > STFT_MAX_RES)
    return fail(VX_ERR_UNSUPPORTED, "vx_stft_create: %d resolutions: 1 .. %d are served", cfg->n_res, STFT_MAX_RES);
  int max_nfft = 0;
  for (int r = 0; r < cfg->n_res; ++r) {
    const int N = cfg->n_fft[r], hop = cfg->hop[r], win = cfg->win[r];
    if ((N != 512 && N != 1024 && N != 2048) || win < 1 || win > N || hop < 1 || hop > N)
      return fail(VX_ERR_UNSUPPORTED,
                  "vx_stft_create: resolution %d: n_fft %d, hop %d, win %d: n_fft in {512, 1024, 2048}, 1 <= win <= n_fft, 1 <= hop <= n_fft are served",
                  r, N, hop, win);
    max_nfft = std::max(max_nfft, N);
  }
  if (cfg->max_batch > STFT_MAX_BATCH) return fail(VX_ERR_UNSUPPORTED, "vx_stft_create: max_batch = %d > %d", cfg->max_batch, STFT_MAX_BATCH);
  if (cfg->max_samples <= max_nfft / 2)
    return fail(VX_ERR_UNSUPPORTED, "vx_stft_create: max_samples = %d: a pair needs more than %d samples", cfg->max_samples, max_nfft / 2);
  long long tiles = 0;
  for (int r = 0; r < cfg->n_res; ++r) {
    Res g;
    g.n_fft = cfg->n_fft[r]; g.hop = cfg->hop[r]; g.win = cfg->win[r];
    g.win_pad = (g.win + STFT_WIN_PAD - 1) / STFT_WIN_PAD * STFT_WIN_PAD;
    tiles += (long long)cfg->max_batch * tiles_of(g, frames_of(g, cfg->max_samples), true) * groups_of(g);
  }
  if (tiles > (1LL << 24)) return fail(VX_ERR_UNSUPPORTED, "vx_stft_create: max_batch x max_samples: %lld workgroups > 2^24", tiles);
  vx_stft* h = new vx_stft();
  h->n_res = cfg->n_res; h->max_samples = cfg->max_samples; h->max_batch = cfg->max_batch; h->max_nfft = max_nfft; h->eps = cfg->eps;
  for (int r = 0; r < cfg->n_res; ++r) {
    Res& g = h->res[r];
    g.n_fft = cfg->n_fft[r]; g.hop = cfg->hop[r]; g.win = cfg->win[r];
    g.win_pad = (g.win + STFT_WIN_PAD - 1) / STFT_WIN_PAD * STFT_WIN_PAD;
    g.off = (g.n_fft - g.win) / 2;
  }
  *out = h;
  return VX_OK;
}

extern "C" void vx_stft_destroy(vx_stft* h) { destroy_handle(h); }

extern "C" int vx_stft_frames(const vx_stft* h, int32_t res, int32_t n_samples) {
  if (!h || res < 0 || res >= h->n_res || n_samples < 0) return 0;
  return (int)frames_of(h->res[res], n_samples);
}

extern "C" int vx_stft_compare(vx_stft* h, int32_t n, const float* const* pred, const int32_t* n_pred, const float* const* target,
                               const int32_t* n_target, double* sums, void* stream) {
  if (!h || !pred || !n_pred || !target || !n_target || !sums) return fail(VX_ERR_ARG, "vx_stft_compare: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_stft_compare: n = %d pairs", n);
  if (n > h->max_batch) return fail(VX_ERR_CAPACITY, "vx_stft_compare: n = %d pairs > max_batch %d", n, h->max_batch);
  std::vector<int> len(n);
  for (int i = 0; i < n; ++i) {
    if (!pred[i] || !target[i]) return fail(VX_ERR_ARG, "vx_stft_compare: pair %d: null pointer", i);
    const int L = std::min(n_pred[i], n_target[i]);
    if (L <= h->max_nfft / 2)
      return fail(VX_ERR_ARG, "vx_stft_compare: pair %d: common length %d: more than %d samples are needed (reflect padding of n_fft %d)", i, L,
                  h->max_nfft / 2, h->max_nfft);
    if (L > h->max_samples) return fail(VX_ERR_CAPACITY, "vx_stft_compare: pair %d: common length %d > max_samples %d", i, L, h->max_samples);
    len[i] = L;
  }
  VXC(ensure_device(h, stft_init_device));
  ON_DEVICE(h->device);
  StftDev& d = *h->dev;
  hipStream_t s = (hipStream_t)stream;
  const Layout lay(h->max_batch, h->n_res);
  const size_t MB = (size_t)h->max_batch;
  VXC(d.stage.begin(s));
  const void** hx = d.stage.host<const void*>();
  const void** hy = d.stage.host<const void*>(lay.ptr_y);
  int* hlen = d.stage.host<int>(lay.ints);
  int* tbeg = d.stage.host<int>(lay.tbeg);
  int* tend = d.stage.host<int>(lay.tend);
  double* cells = d.stage.host<double>(lay.cells);
  for (int i = 0; i < n; ++i) { hx[i] = pred[i]; hy[i] = target[i]; hlen[i] = len[i]; }
  int base[STFT_MAX_RES], count[STFT_MAX_RES], run = 0;
  for (int r = 0; r < h->n_res; ++r) {
    const Res& gr = h->res[r];
    int* tile0 = d.stage.host<int>(lay.res0 + (size_t)r * lay.res_stride);
    int* frames = tile0 + MB + 1;
    base[r] = run;
    tile0[0] = 0;
    for (int i = 0; i < n; ++i) {
      const long long fr = frames_of(gr, len[i]);
      frames[i] = (int)fr;
      tile0[i + 1] = tile0[i] + (int)tiles_of(gr, fr, true);
      tbeg[i * h->n_res + r] = run + tile0[i] * groups_of(gr);
      tend[i * h->n_res + r] = run + tile0[i + 1] * groups_of(gr);
      cells[i * h->n_res + r] = (double)fr * (double)(gr.n_fft / 2 + 1);
    }
    count[r] = tile0[n] * groups_of(gr);
    run += count[r];
  }
  VXC(d.stage.upload(lay.bytes, s));
  for (int r = 0; r < h->n_res; ++r) {  // one launch per resolution, then one for the sums
    StftArgs a = args_of(h, r, n, true, lay);
    a.tile_base = base[r];
    stft_tile_kernel<true><<<(unsigned)std::min(count[r], 1 << 16), STFT_WG, 0, s>>>(a);
    HIPC(hipGetLastError());
  }
  const int npr = n * h->n_res;
  stft_finish_kernel<<<(npr * 4 + 63) / 64, 64, 0, s>>>(d.ws.get(), d.stage.dev<const int>(lay.tbeg), d.stage.dev<const int>(lay.tend),
                                                       d.stage.dev<const double>(lay.cells), npr, d.sums.get());
  HIPC(hipGetLastError());
  const hipError_t e = hipMemcpyAsync(sums, d.sums.get(), (size_t)npr * 4 * sizeof(double), hipMemcpyDefault, s);
  VXC(d.stage.finish(s));
  HIPC(e);
  return VX_OK;
}

extern "C" int vx_stft_magnitude(vx_stft* h, int32_t res, int32_t n, const float* const* wav, const int32_t* n_samples, float* const* out,
                                 void* stream) {
  if (!h || !wav || !n_samples || !out) return fail(VX_ERR_ARG, "vx_stft_magnitude: null argument");
  if (res < 0 || res >= h->n_res) return fail(VX_ERR_ARG, "vx_stft_magnitude: resolution %d of %d", res, h->n_res);
  if (n < 1) return fail(VX_ERR_ARG, "vx_stft_magnitude: n = %d signals", n);
  if (n > h->max_batch) return fail(VX_ERR_CAPACITY, "vx_stft_magnitude: n = %d signals > max_batch %d", n, h->max_batch);
  const Res& gr = h->res[res];
  for (int i = 0; i < n; ++i) {
    if (!wav[i] || !out[i]) return fail(VX_ERR_ARG, "vx_stft_magnitude: signal %d: null pointer", i);
    if (n_samples[i] <= gr.n_fft / 2)
      return fail(VX_ERR_ARG, "vx_stft_magnitude: signal %d: %d samples: more than %d are needed (reflect padding of n_fft %d)", i, n_samples[i],
                  gr.n_fft / 2, gr.n_fft);
    if (n_samples[i] > h->max_samples)
      return fail(VX_ERR_CAPACITY, "vx_stft_magnitude: signal %d: %d samples > max_samples %d", i, n_samples[i], h->max_samples);
  }
  VXC(ensure_device(h, stft_init_device));
  ON_DEVICE(h->device);
  StftDev& d = *h->dev;
  hipStream_t s = (hipStream_t)stream;
  const Layout lay(h->max_batch, h->n_res);
  const size_t MB = (size_t)h->max_batch;
  VXC(d.stage.begin(s));
  const void** hx = d.stage.host<const void*>();
  void** ho = d.stage.host<void*>(lay.ptr_y);
  int* hlen = d.stage.host<int>(lay.ints);
  int* tile0 = d.stage.host<int>(lay.res0 + (size_t)res * lay.res_stride);
  int* frames = tile0 + MB + 1;
  tile0[0] = 0;
  for (int i = 0; i < n; ++i) {
    hx[i] = wav[i]; ho[i] = out[i]; hlen[i] = n_samples[i];
    const long long fr = frames_of(gr, n_samples[i]);
    frames[i] = (int)fr;
    tile0[i + 1] = tile0[i] + (int)tiles_of(gr, fr, false);
  }
  VXC(d.stage.upload(lay.bytes, s));
  const StftArgs a = args_of(h, res, n, false, lay);
  stft_tile_kernel<false><<<(unsigned)std::min(tile0[n] * groups_of(gr), 1 << 16), STFT_WG, 0, s>>>(a);
  HIPC(hipGetLastError());
  return d.stage.finish(s);
}
