// Dynamic time warping behind the C ABI (include/vallex.h, vx_dtw_*): the host table of the cepstra, the staging of a ragged call
// (CallStage, host.hpp), the workspace that grows with the calls, and the launches of dtw_kernels.hpp.  A translation unit and a
// handle of its own, like fbank.hip: no other unit sees these kernels, so the device code of every existing path is compiled
// exactly as before.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#undef VX_STAMPS  // the in-kernel stamps write device globals of engine.hip's unit, out of this unit's reach
#include "host.hpp"
#include "dtw_kernels.hpp"

using namespace vx;

namespace {
// Device side of a handle: made on the device that is current at the first vx_dtw_compare, dropped as a whole.
struct DtwDev {
  DevBuf<float> tab;
  CallStage stage;       // per call: DtwPair [max_batch]
  DevBuf<double> total;  // [max_batch]
  DevBuf<int> len;       // [max_batch]
  // workspace, sized to the largest call so far: 4 (cost) + 1 (back-pointer) bytes per cell, 4 n_ceps bytes per frame
  DevBuf<float> cost, ceps;
  DevBuf<unsigned char> bp;
  long long cap_cells = 0, cap_rows = 0;
};
}  // namespace

struct vx_dtw : LazyDev<DtwDev> {
  int dim = 0, n_ceps = 0, max_frames = 0, max_batch = 0;
  std::vector<float> tab;  // [dim][n_ceps]: sqrt(2 / dim) cos(pi k (n + 1/2) / dim), k = 1 .. n_ceps
};

namespace {

// The orthonormal DCT-II without its 0th row, n-major: fp64, rounded once.
std::vector<float> dct_table(int dim, int n_ceps) {
  std::vector<float> t((size_t)dim * n_ceps);
  const double pi = 3.14159265358979323846, scale = sqrt(2.0 / (double)dim);
  for (int n = 0; n < dim; ++n)
    for (int k = 1; k <= n_ceps; ++k) t[(size_t)n * n_ceps + (k - 1)] = (float)(scale * cos(pi * (double)k * ((double)n + 0.5) / (double)dim));
  return t;
}

// First use: the table goes to the current device.
int dtw_init_device(vx_dtw* h) {
  VXC(open_device(h));
  DtwDev& d = *h->dev;
  const size_t MB = (size_t)h->max_batch;
  VXC(d.stage.init(MB * sizeof(DtwPair)));
  VXC(d.total.alloc(MB));
  VXC(d.len.alloc(MB));
  if (h->n_ceps > 0) {
    VXC(d.tab.alloc(h->tab.size()));
    HIPC(hipMemcpy(d.tab.get(), h->tab.data(), h->tab.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  return VX_OK;
}

// The workspace follows the largest call: a larger one waits for the previous call and replaces the buffers.
int dtw_grow(vx_dtw* h, long long cells, long long rows) {
  DtwDev& d = *h->dev;
  if (cells <= d.cap_cells && rows <= d.cap_rows) return VX_OK;
  VXC(d.stage.drain());
  if (cells > d.cap_cells) {
    d.cap_cells = 0;
    d.cost.reset();
    d.bp.reset();
    VXC(d.cost.alloc((size_t)cells));
    VXC(d.bp.alloc((size_t)cells));
    d.cap_cells = cells;
  }
  if (rows > d.cap_rows && h->n_ceps > 0) {
    d.cap_rows = 0;
    VXC(d.ceps.alloc((size_t)rows * h->n_ceps));
    d.cap_rows = rows;
  }
  return VX_OK;
}

// Cepstra (n_ceps > 0) and the cost matrices of the n staged pairs.
void launch_dtw_cost(const DtwPair* d_pairs, int n, int tiles, long long max_rows, const float* d_tab, int dim, int n_ceps, float* d_ceps,
                     float* d_cost, hipStream_t s) {
  if (n_ceps > 0) {
    const long long blocks = (max_rows * n_ceps + DTW_WG - 1) / DTW_WG;
    dtw_ceps_kernel<<<dim3((unsigned)std::min<long long>(std::max<long long>(blocks, 1), 1024), n), DTW_WG, 0, s>>>(d_pairs, d_tab, dim,
                                                                                                                  n_ceps, d_ceps);
    dtw_cost_kernel<<<tiles, DTW_WG, 0, s>>>(d_pairs, n, d_ceps, n_ceps, d_cost);
  } else {
    dtw_cost_kernel<<<tiles, DTW_WG, 0, s>>>(d_pairs, n, nullptr, dim, d_cost);
  }
}

// One workgroup per pair; the three diagonals of the longest A of the launch in LDS.
hipError_t launch_dtw_warp(const float* d_cost, unsigned char* d_bp, const DtwPair* d_pairs, int n, int max_ta, double* d_total, int* d_len,
                           hipStream_t s) {
  const size_t lds = (size_t)3 * max_ta * sizeof(double);
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute((const void*)dtw_warp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * DTW_MAX_FRAMES * 8);
    if (e != hipSuccess) return e;
  }
  dtw_warp_kernel<<<n, DTW_WG, lds, s>>>(d_cost, d_bp, d_pairs, d_total, d_len);
  return hipGetLastError();
}

}  // namespace

extern "C" int vx_dtw_create(const vx_dtw_config* cfg, vx_dtw** out) {
  VXC(create_head("vx_dtw_create", cfg, out));
  if (cfg->max_batch < 1) return fail(VX_ERR_ARG, "vx_dtw_create: max_batch = %d", cfg->max_batch);
  if (cfg->dim < 1 || cfg->dim > DTW_MAX_DIM) return fail(VX_ERR_UNSUPPORTED, "vx_dtw_create: dim = %d outside [1, %d]", cfg->dim, DTW_MAX_DIM);
  if (cfg->n_ceps < 0 || cfg->n_ceps > cfg->dim - 1)
    return fail(VX_ERR_UNSUPPORTED, "vx_dtw_create: n_ceps = %d outside [0, dim - 1 = %d]", cfg->n_ceps, cfg->dim - 1);
  if (cfg->max_frames < 1 || cfg->max_frames > DTW_MAX_FRAMES)
    return fail(VX_ERR_UNSUPPORTED, "vx_dtw_create: max_frames = %d outside [1, %d]", cfg->max_frames, DTW_MAX_FRAMES);
  if (cfg->max_batch > DTW_MAX_BATCH) return fail(VX_ERR_UNSUPPORTED, "vx_dtw_create: max_batch = %d > %d", cfg->max_batch, DTW_MAX_BATCH);
  vx_dtw* h = new vx_dtw();
  h->dim = cfg->dim; h->n_ceps = cfg->n_ceps; h->max_frames = cfg->max_frames; h->max_batch = cfg->max_batch;
  h->tab = dct_table(cfg->dim, cfg->n_ceps);
  *out = h;
  return VX_OK;
}

extern "C" void vx_dtw_destroy(vx_dtw* h) { destroy_handle(h); }

extern "C" int vx_dtw_compare(vx_dtw* h, int32_t n, const float* const* a, const int32_t* Ta, const float* const* b, const int32_t* Tb,
                              double* total, int32_t* path_len, int32_t* const* path, void* stream) {
  if (!h || !a || !Ta || !b || !Tb || !total || !path_len) return fail(VX_ERR_ARG, "vx_dtw_compare: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_dtw_compare: n = %d pairs", n);
  if (n > h->max_batch) return fail(VX_ERR_CAPACITY, "vx_dtw_compare: n = %d pairs > max_batch %d", n, h->max_batch);
  std::vector<DtwPair> ps(n);
  long long cells = 0, rows = 0, max_rows = 0;
  int tiles = 0, max_ta = 0;
  for (int i = 0; i < n; ++i) {
    if (!a[i] || !b[i]) return fail(VX_ERR_ARG, "vx_dtw_compare: pair %d: null pointer", i);
    if (Ta[i] < 1 || Tb[i] < 1) return fail(VX_ERR_ARG, "vx_dtw_compare: pair %d: %d x %d frames", i, Ta[i], Tb[i]);
    if (Ta[i] > h->max_frames || Tb[i] > h->max_frames)
      return fail(VX_ERR_CAPACITY, "vx_dtw_compare: pair %d: %d x %d frames > max_frames %d", i, Ta[i], Tb[i], h->max_frames);
    DtwPair& p = ps[i];
    p.a = a[i]; p.b = b[i]; p.path = path ? path[i] : nullptr;
    p.cell_off = cells; p.ceps_off = rows * h->n_ceps;
    p.Ta = Ta[i]; p.Tb = Tb[i]; p.tile0 = tiles; p.pad_ = 0;
    cells += (long long)Ta[i] * Tb[i];
    rows += (long long)Ta[i] + Tb[i];
    max_rows = std::max(max_rows, (long long)Ta[i] + Tb[i]);
    tiles += ((Ta[i] + DTW_TILE - 1) / DTW_TILE) * ((Tb[i] + DTW_TILE - 1) / DTW_TILE);  // <= 64 pairs x 64 x 64 tiles
    max_ta = std::max(max_ta, Ta[i]);
  }
  VXC(ensure_device(h, dtw_init_device));
  ON_DEVICE(h->device);
  DtwDev& d = *h->dev;
  hipStream_t s = (hipStream_t)stream;
  VXC(dtw_grow(h, cells, rows));
  VXC(d.stage.begin(s));
  memcpy(d.stage.host<DtwPair>(), ps.data(), (size_t)n * sizeof(DtwPair));
  VXC(d.stage.upload((size_t)n * sizeof(DtwPair), s));
  const DtwPair* dp = d.stage.dev<const DtwPair>();
  launch_dtw_cost(dp, n, tiles, max_rows, d.tab.get(), h->dim, h->n_ceps, d.ceps.get(), d.cost.get(), s);
  HIPC(hipGetLastError());
  HIPC(launch_dtw_warp(d.cost.get(), d.bp.get(), dp, n, max_ta, d.total.get(), d.len.get(), s));
  hipError_t e1 = hipMemcpyAsync(total, d.total.get(), (size_t)n * sizeof(double), hipMemcpyDefault, s);
  hipError_t e2 = hipMemcpyAsync(path_len, d.len.get(), (size_t)n * sizeof(int), hipMemcpyDefault, s);
  VXC(d.stage.finish(s));
  HIPC(e1);
  HIPC(e2);
  return VX_OK;
}

// The cepstra and cost kernels of one pair on caller data; synchronous.
extern "C" int vx_op_dtw_cost(int32_t dim, int32_t n_ceps, const float* a, int32_t Ta, const float* b, int32_t Tb, float* cost,
                              void* stream) {
  if (!a || !b || !cost) return fail(VX_ERR_ARG, "vx_op_dtw_cost: null argument");
  if (dim < 1 || dim > DTW_MAX_DIM || n_ceps < 0 || n_ceps > dim - 1)
    return fail(VX_ERR_ARG, "vx_op_dtw_cost: dim = %d, n_ceps = %d (dim in [1, %d], n_ceps in [0, dim - 1])", dim, n_ceps, DTW_MAX_DIM);
  if (Ta < 1 || Tb < 1 || Ta > DTW_MAX_FRAMES || Tb > DTW_MAX_FRAMES)
    return fail(VX_ERR_ARG, "vx_op_dtw_cost: %d x %d frames (1 .. %d each)", Ta, Tb, DTW_MAX_FRAMES);
  DtwPair p{};
  p.a = a; p.b = b; p.Ta = Ta; p.Tb = Tb;
  const int tiles = ((Ta + DTW_TILE - 1) / DTW_TILE) * ((Tb + DTW_TILE - 1) / DTW_TILE);
  const std::vector<float> tab = dct_table(dim, n_ceps);
  hipStream_t s = (hipStream_t)stream;
  DevBuf<DtwPair> d_p;
  DevBuf<float> d_tab, d_ceps;
  VXC(d_p.alloc(1));
  if (n_ceps > 0) {
    VXC(d_tab.alloc(tab.size()));
    VXC(d_ceps.alloc((size_t)(Ta + Tb) * n_ceps));
  }
  VXC(d_p.upload(&p, 1, s));
  if (n_ceps > 0) VXC(d_tab.upload(tab.data(), tab.size(), s));
  launch_dtw_cost(d_p.get(), 1, tiles, (long long)Ta + Tb, d_tab.get(), dim, n_ceps, d_ceps.get(), cost, s);
  const hipError_t err = hipGetLastError();
  const hipError_t err2 = hipStreamSynchronize(s);  // also: `p` and `tab` outlive their copies
  HIPC(err);
  HIPC(err2);
  return VX_OK;
}

// desc: n x 4 host values per matrix (Ta, Tb, cell_off, path_off); synchronous.
extern "C" int vx_op_dtw_path(const float* cost, int32_t n, const int64_t* desc, double* total, int32_t* path_len, int32_t* path,
                              void* stream) {
  if (!cost || !desc || !total || !path_len) return fail(VX_ERR_ARG, "vx_op_dtw_path: null argument");
  if (n < 1) return fail(VX_ERR_ARG, "vx_op_dtw_path: n = %d matrices", n);
  std::vector<DtwPair> ps(n);
  long long cells = 0;
  int max_ta = 0;
  for (int z = 0; z < n; ++z) {
    const int64_t* d = desc + 4 * (size_t)z;
    if (d[0] < 1 || d[1] < 1 || d[2] < 0 || d[3] < 0) return fail(VX_ERR_ARG, "vx_op_dtw_path: matrix %d: Ta and Tb must be >= 1, offsets >= 0", z);
    if (d[0] > DTW_MAX_FRAMES || d[1] > DTW_MAX_FRAMES)
      return fail(VX_ERR_CAPACITY, "vx_op_dtw_path: matrix %d: %lld x %lld frames (at most %d each)", z, (long long)d[0], (long long)d[1], DTW_MAX_FRAMES);
    DtwPair& p = ps[z];
    p = DtwPair{};
    p.Ta = (int)d[0]; p.Tb = (int)d[1]; p.cell_off = d[2];
    p.path = path ? path + 2 * d[3] : nullptr;
    cells = std::max(cells, (long long)d[2] + (long long)d[0] * d[1]);
    max_ta = std::max(max_ta, p.Ta);
  }
  hipStream_t s = (hipStream_t)stream;
  DevBuf<DtwPair> d_p;
  DevBuf<unsigned char> bp;
  VXC(d_p.alloc(ps.size()));
  VXC(bp.alloc((size_t)cells));
  VXC(d_p.upload(ps.data(), ps.size(), s));
  const hipError_t err = launch_dtw_warp(cost, bp.get(), d_p.get(), n, max_ta, total, path_len, s);
  const hipError_t err2 = hipStreamSynchronize(s);
  HIPC(err);
  HIPC(err2);
  return VX_OK;
}
