// api.hip -- extern "C" entry points of libgslm.so (declared in include/gslm.h).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "gslm_kernels.hpp"

namespace gslm {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

thread_local DebugSync g_debug;

int launch_failed(hipError_t e, const char* file, int line) {
  const char* base = std::strrchr(file, '/');
  set_error(std::string(g_debug.on ? "kernel failed (debug mode: stream synchronised after the launch at " : "kernel launch (") +
            (base ? base + 1 : file) + ":" + std::to_string(line) + "): " + hipGetErrorString(e));
  return GSLM_ERR_HIP;
}

namespace {

struct Carver {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off = align_up(off + count * sizeof(T));
    return p;
  }
};

}  // namespace

size_t geom_layout(int64_t P, void* base, GeomBufs* o) {
  Carver c{(char*)base};
  GeomBufs g;
  g.rec = c.take<float4>((size_t)P * RECS);
  g.depth_key = c.take<uint32_t>(P);
  g.tiles = c.take<uint32_t>(P);
  g.rect = c.take<uint2>(P);
  g.vals_init = c.take<uint32_t>(P);
  g.sorted_idx = g.vals_init;
  g.keys_alt = c.take<uint32_t>(P);
  g.vals_alt = c.take<uint32_t>(P);
  g.offsets = c.take<uint32_t>(P);
  g.goff = c.take<uint32_t>(P);
  g.hist = c.take<uint32_t>(sort_hist_bytes(P) / 4);
  g.scan_tmp = c.take<uint32_t>(scan_tmp_bytes(P) / 4);
  g.counters = c.take<uint32_t>(16);
  g.clampw = c.take<uint32_t>(P);
  if (o) *o = g;
  return c.off;
}

size_t bin_layout(int64_t N, int ntiles, void* base, BinBufs* o) {
  Carver c{(char*)base};
  BinBufs b;
  b.keys0 = c.take<uint32_t>(N);
  b.keys1 = c.take<uint32_t>(N);
  b.vals0 = c.take<uint32_t>(N);
  b.vals1 = c.take<uint32_t>(N);
  b.hist = c.take<uint32_t>(sort_hist_bytes(N) / 4);
  b.ranges = c.take<uint2>(ntiles);
  b.tile_order = c.take<uint32_t>(ntiles);
  b.tile_neff = c.take<uint32_t>((size_t)4 * ntiles);
  b.end_bit = 1;
  while ((1ll << b.end_bit) < (long long)ntiles) ++b.end_bit;
  b.passes = (b.end_bit + 7) / 8;
  b.point_list = (b.passes & 1) ? b.vals1 : b.vals0;
  b.keys_sorted = (b.passes & 1) ? b.keys1 : b.keys0;
  b.slots = (b.passes & 1) ? b.keys0 : b.keys1;
  if (o) *o = b;
  return c.off;
}

size_t img_layout(int H, int W, void* base, ImgBufs* o) {
  Carver c{(char*)base};
  ImgBufs b;
  b.final_T = c.take<float>((size_t)H * W);
  b.n_contrib = c.take<uint32_t>((size_t)H * W);
  if (o) *o = b;
  return c.off;
}

size_t scratch_layout(int64_t P, int64_t N, void* base, ScratchBufs* o) {
  Carver c{(char*)base};
  ScratchBufs b;
  b.trec = c.take<float4>((size_t)P * REC_F4);
  b.contrib = c.take<float4>((size_t)N * REC_F4);
  b.hscan = c.take<uint32_t>((size_t)N + 1);
  b.scan_tmp = c.take<uint32_t>(scan_tmp_bytes(N) / 4);
  if (o) *o = b;
  return c.off;
}

static int make_view(const gslm_view* in, int M, ViewK* v) {
  if (!in) { set_error("view is NULL"); return GSLM_ERR_INVALID; }
  if (in->image_height <= 0 || in->image_width <= 0) { set_error("image size must be positive"); return GSLM_ERR_INVALID; }
  if (in->image_height > 65535 * 16 || in->image_width > 65535 * 16) { set_error("image too large"); return GSLM_ERR_INVALID; }
  if (in->sh_degree < 0 || in->sh_degree > 3) { set_error("sh_degree must be in [0,3]"); return GSLM_ERR_INVALID; }
  if (!(in->tanfovx > 0.0) || !(in->tanfovy > 0.0)) { set_error("tanfov must be positive"); return GSLM_ERR_INVALID; }
  v->H = in->image_height;
  v->W = in->image_width;
  v->gx = (v->W + TILE_X - 1) / TILE_X;
  v->gy = (v->H + TILE_Y - 1) / TILE_Y;
  v->focal_x = (float)((double)v->W / (2.0 * in->tanfovx));
  v->focal_y = (float)((double)v->H / (2.0 * in->tanfovy));
  v->limx = (float)(1.3 * in->tanfovx);
  v->limy = (float)(1.3 * in->tanfovy);
  std::memcpy(v->view, in->viewmatrix, sizeof(v->view));
  std::memcpy(v->proj, in->projmatrix, sizeof(v->proj));
  for (int k = 0; k < 3; ++k) { v->campos[k] = in->campos[k]; v->bg[k] = in->bg[k]; }
  v->scale_mod = (float)in->scale_modifier;
  v->D = in->sh_degree;
  v->M = M;
  v->antialiasing = in->antialiasing ? 1 : 0;
  v->exhaustive = in->debug ? 1 : 0;
  return GSLM_OK;
}

static int make_gauss(const gslm_gaussians* in, const ViewK* v, GaussK* g, bool tangent) {
  if (!in) { set_error("gaussians is NULL"); return GSLM_ERR_INVALID; }
  if (in->P < 0 || in->P > MAX_P) { set_error("P out of range [0, 2^28 - 1]"); return GSLM_ERR_INVALID; }
  g->P = in->P;
  g->raw = in->raw ? 1 : 0;
  g->M = in->max_coeffs;
  g->means3D = in->means3D;
  g->opac = in->opacities;
  g->scales = in->scales;
  g->rot = in->rotations;
  g->cov3D = in->cov3D_precomp;
  g->dc = in->sh_dc;
  g->dc_stride = in->sh_dc_stride;
  g->rest = in->sh_rest;
  g->rest_stride = in->sh_rest_stride;
  g->colors = in->colors_precomp;
  if (tangent || in->P == 0) return GSLM_OK;
  if (!g->means3D || !g->opac) { set_error("means3D and opacities are required"); return GSLM_ERR_INVALID; }
  if (!g->cov3D && !(g->scales && g->rot)) { set_error("need scales+rotations or cov3D_precomp"); return GSLM_ERR_INVALID; }
  if (!g->colors) {
    if (!g->dc) { set_error("need shs or colors_precomp"); return GSLM_ERR_INVALID; }
    if ((v->D + 1) * (v->D + 1) > g->M) { set_error("sh_degree exceeds stored coefficients"); return GSLM_ERR_INVALID; }
    if (g->M > 1 && !g->rest) { set_error("sh_rest is NULL"); return GSLM_ERR_INVALID; }
  }
  return GSLM_OK;
}

// the preprocess kernels' outputs inside a geometry workspace; pos: the view's depth positions, or NULL (index space)
static PreOutBufs pre_out_bufs(const GeomBufs& gb, const uint32_t* pos) {
  return PreOutBufs{gb.rec, gb.depth_key, gb.tiles, gb.rect, gb.clampw, pos};
}

// order_mode (gslm_preprocess_ordered): 0 sort, 1 sort and copy the order out to depth_order, 2 take the order from
// depth_order instead of sorting
int do_preprocess(const ViewK& v, const GaussK& g, const GeomBufs& gb, int32_t* radii, hipStream_t s,
                  uint32_t* depth_order, int order_mode) {
  int st = launch_preprocess(v, g, pre_out_bufs(gb, nullptr), radii, s);
  if (st) return st;
  const int64_t P = g.P;
  if (P == 0) {
    GSLM_HIP_CHECK(hipMemsetAsync(gb.counters, 0, 4, s));
    return GSLM_OK;
  }
  const uint32_t* tiles_sorted = nullptr;  // the tile counts in depth order, when the sort gathered them
  if (order_mode == 2) {
    GSLM_HIP_CHECK(hipMemcpyAsync(gb.sorted_idx, depth_order, (size_t)P * 4, hipMemcpyDeviceToDevice, s));
  } else {
    // depth sort of (key, index) pairs: the first scatter generates the indices (no iota pass), the last writes
    // tiles[index] where the sorted keys would go.  key_range: the passes sort the bytes of key - min and those past
    // the frame's span run as copies (the 32-bit order exactly; sort.hip KeyRange): 3 working passes at the bench
    // scene's depths, -7 us per forward (profiles/r06/ab_depth_key_range/; routing the working passes through a third
    // buffer pair instead of copying measured the same).  (Round 6 also measured 3 passes of 11-bit digits against 4 of
    // 8 bits: 90.9 against 90.8 us per 1M keys -- the 2048-digit scatter and scan cost what the fourth pass did --
    // profiles/r06/ab_depth_sort_d11_neutral/.)
    bool alt = false;
    st = radix_sort_pairs(gb.depth_key, gb.vals_init, gb.keys_alt, gb.vals_alt, P, 32, gb.hist, &alt, s, true, gb.tiles,
                          nullptr, nullptr, nullptr, true);
    if (st) return st;
    if (alt) GSLM_HIP_CHECK(hipMemcpyAsync(gb.sorted_idx, gb.vals_alt, (size_t)P * 4, hipMemcpyDeviceToDevice, s));
    tiles_sorted = alt ? gb.keys_alt : gb.depth_key;
    if (order_mode == 1)
      GSLM_HIP_CHECK(hipMemcpyAsync(depth_order, gb.sorted_idx, (size_t)P * 4, hipMemcpyDeviceToDevice, s));
  }
  // tile-count scans in index order (gradient-row offsets goff) and in depth order (duplicate offsets)
  return exclusive_scan_u32_dual(gb.tiles, gb.sorted_idx, gb.goff, gb.offsets, P, gb.scan_tmp, gb.counters + 1,
                                 gb.counters, s, tiles_sorted);
}

// the line search's shared binning: the n parameter sets' geometries, and the union list's per-set masks
// the depth-space render records of gslm_preprocess_views(depth_pos): [P][RECS] float4 at the start of a workspace
size_t depth_records_bytes(int64_t P) { return align_up((size_t)(P > 0 ? P : 0) * RECS * sizeof(float4)); }

// the n per-set depth-space workspaces (each set_bytes long): only their render records are read
int union_sets(const void* const* geoms, int32_t n, int64_t P, size_t set_bytes, UnionSets* u) {
  if (n < 1 || n > MAX_UNION_SETS) {
    set_error("union: 1 <= n <= 8 parameter sets");
    return GSLM_ERR_INVALID;
  }
  if (!geoms) { set_error("union: NULL geoms"); return GSLM_ERR_INVALID; }
  if (set_bytes < depth_records_bytes(P)) { set_error("union: a set's workspace is below gslm_depth_records_bytes(P)"); return GSLM_ERR_CAPACITY; }
  *u = UnionSets{};
  u->n = n;
  for (int a = 0; a < n; ++a) {
    if (!geoms[a] && P) { set_error("union: NULL geometry"); return GSLM_ERR_INVALID; }
    u->rec[a] = reinterpret_cast<const float4*>(geoms[a]);  // geom_layout's first region (rec at offset 0)
    u->tiles[a] = nullptr;
    u->rect[a] = nullptr;
  }
  return GSLM_OK;
}

size_t union_masks_layout(int64_t N, int ntiles, void* binning, UnionMasks* o) {
  BinBufs bb;
  const size_t off = bin_layout(N, ntiles, nullptr, &bb);
  Carver c{(char*)binning};
  c.off = off;
  UnionMasks m;
  m.m0 = c.take<uint32_t>(N);
  m.m1 = c.take<uint32_t>(N);
  m.hist = c.take<uint32_t>(sort_hist_bytes(N, true) / 4);
  m.nsets = c.take<uint32_t>(4);
  m.sorted = (bb.passes & 1) ? m.m1 : m.m0;
  if (o) *o = m;
  return c.off;
}

}  // namespace gslm

using namespace gslm;

extern "C" {

const char* gslm_last_error(void) { return g_last_error.c_str(); }
int gslm_abi_version(void) { return GSLM_ABI_VERSION; }

size_t gslm_geom_bytes(int64_t P) { return geom_layout(P, nullptr, nullptr); }
size_t gslm_image_bytes(int32_t H, int32_t W) { return img_layout(H, W, nullptr, nullptr); }
size_t gslm_binning_bytes(int64_t N, int32_t H, int32_t W) {
  const int ntiles = ((W + TILE_X - 1) / TILE_X) * ((H + TILE_Y - 1) / TILE_Y);
  return bin_layout(N, ntiles, nullptr, nullptr);
}
size_t gslm_scratch_bytes(int64_t P, int64_t N) { return scratch_layout(P, N, nullptr, nullptr); }

// gslm_preprocess and its ordered form: one body, order_mode 0 for the plain one
static int preprocess(const gslm_view* view, const gslm_gaussians* gi, void* geom, size_t geom_bytes, int32_t* out_radii,
                      uint32_t* depth_order, int32_t order_mode, void* stream) {
  ViewK v;
  GaussK g;
  int st = make_view(view, gi ? gi->max_coeffs : 0, &v);
  if (st) return st;
  if ((st = make_gauss(gi, &v, &g, false))) return st;
  if (geom_bytes < gslm_geom_bytes(g.P) || (!geom && g.P)) { set_error("geometry workspace too small"); return GSLM_ERR_CAPACITY; }
  GeomBufs gb;
  geom_layout(g.P, geom, &gb);
  return do_preprocess(v, g, gb, out_radii, (hipStream_t)stream, depth_order, order_mode);
}

int gslm_preprocess(const gslm_view* view, const gslm_gaussians* gi, void* geom, size_t geom_bytes, int32_t* out_radii,
                    void* stream) {
  DebugScope dbg_scope(view != nullptr && view->debug != 0, stream);
  return preprocess(view, gi, geom, geom_bytes, out_radii, nullptr, 0, stream);
}

int gslm_preprocess_ordered(const gslm_view* view, const gslm_gaussians* gi, void* geom, size_t geom_bytes,
                            int32_t* out_radii, uint32_t* depth_order, int32_t order_mode, void* stream) {
  if (order_mode < 0 || order_mode > 2) { set_error("preprocess_ordered: order_mode must be 0, 1 or 2"); return GSLM_ERR_INVALID; }
  if (order_mode && gi && gi->P > 0 && !depth_order) { set_error("preprocess_ordered: NULL depth_order"); return GSLM_ERR_INVALID; }
  return preprocess(view, gi, geom, geom_bytes, out_radii, depth_order, order_mode, stream);
}

int gslm_preprocess_views(const gslm_view* views, int32_t nviews, const gslm_gaussians* gi, void* const* geoms,
                          size_t geom_bytes, const uint32_t* const* depth_pos, void* stream) {
  if (!views || !gi || !geoms || nviews < 1 || nviews > MAX_PRE_VIEWS) {
    set_error("preprocess_views: NULL argument or nviews outside 1..8");
    return GSLM_ERR_INVALID;
  }
  PreViewsK pv;
  GaussK g;
  int st;
  for (int b = 0; b < nviews; ++b) {
    if ((st = make_view(&views[b], gi->max_coeffs, &pv.v[b]))) return st;
    if ((st = make_gauss(gi, &pv.v[b], &g, false))) return st;  // each view's SH degree against the stored coefficients
    const size_t need = depth_pos ? depth_records_bytes(g.P) : gslm_geom_bytes(g.P);
    if (geom_bytes < need || (!geoms[b] && g.P)) { set_error("geometry workspace too small"); return GSLM_ERR_CAPACITY; }
    GeomBufs gb;
    geom_layout(g.P, geoms[b], &gb);  // depth space writes the records (offset 0) only
    const uint32_t* pos = depth_pos ? depth_pos[b] : nullptr;
    if (depth_pos && !pos && g.P) { set_error("preprocess_views: NULL depth positions"); return GSLM_ERR_INVALID; }
    pv.out[b] = pre_out_bufs(gb, pos);
  }
  pv.n = nviews;
  return launch_preprocess_views(pv, g, (hipStream_t)stream);
}

int gslm_depth_positions(const uint32_t* depth_order, int64_t P, uint32_t* depth_pos, void* stream) {
  if (P < 0 || P > MAX_P || (P && (!depth_order || !depth_pos))) {
    set_error("depth_positions: NULL order / positions or P out of range");
    return GSLM_ERR_INVALID;
  }
  return launch_depth_positions(P, depth_order, depth_pos, (hipStream_t)stream);
}

int gslm_num_rendered(const void* geom, int64_t P, int64_t* out, void* stream) {
  GeomBufs gb;
  geom_layout(P, const_cast<void*>(geom), &gb);
  // a pinned word per host thread: the read-back is one DMA + stream sync instead of a staged pageable copy
  thread_local uint32_t* pinned = nullptr;
  if (!pinned) GSLM_HIP_CHECK(hipHostMalloc((void**)&pinned, sizeof(uint32_t), hipHostMallocDefault));
  GSLM_HIP_CHECK(hipMemcpyAsync(pinned, gb.counters, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  GSLM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  *out = (int64_t)*pinned;
  return GSLM_OK;
}

}  // extern "C"

namespace gslm {
constexpr int READ_COUNTS_MAX = 32;
struct CountPtrs {
  const uint32_t* p[READ_COUNTS_MAX];
};
// the pair counts of up to 32 geometries into pinned host memory in ONE launch (thread k: count k), where one
// 4-byte device-to-host copy per geometry is a blit launch each, in series on the stream
__global__ void k_read_counts(CountPtrs c, int n, uint32_t* __restrict__ out) {
  const int k = threadIdx.x;
  if (k < n) out[k] = *c.p[k];
}

// gslm_robust as the entry points take it (gslm_kernels.hpp)
int robust_arg(const gslm_robust* robust, const char* what, bool* on, gslm_robust* out) {
  *on = false;
  if (!robust || robust->kind == GSLM_ROBUST_NONE) return GSLM_OK;
  if (robust->kind != GSLM_ROBUST_HUBER && robust->kind != GSLM_ROBUST_CAUCHY) {
    set_error(std::string(what) + ": unknown robust kind (GSLM_ROBUST_NONE / HUBER / CAUCHY)");
    return GSLM_ERR_INVALID;
  }
  if (!(std::isfinite(robust->delta) && robust->delta > 0.0f)) {
    set_error(std::string(what) + ": robust delta must be finite and > 0");
    return GSLM_ERR_INVALID;
  }
  *on = true;
  *out = *robust;
  return GSLM_OK;
}
}  // namespace gslm

extern "C" {

int gslm_num_rendered_many(const void* const* geoms, const int64_t* Ps, int32_t n, int64_t* out, void* stream) {
  if (n < 0 || (n > 0 && (!geoms || !Ps || !out))) { set_error("num_rendered_many: NULL argument"); return GSLM_ERR_INVALID; }
  if (n == 0) return GSLM_OK;
  // one pinned array per host thread, grown on demand: one gather launch per 32 geometries writing into it, then
  // ONE stream sync
  thread_local uint32_t* pinned = nullptr;
  thread_local uint32_t* pinned_dev = nullptr;
  thread_local int32_t cap = 0;
  if (cap < n) {
    if (pinned) GSLM_HIP_CHECK(hipHostFree(pinned));
    pinned = pinned_dev = nullptr;
    cap = 0;
    GSLM_HIP_CHECK(hipHostMalloc((void**)&pinned, sizeof(uint32_t) * (size_t)n, hipHostMallocDefault));
    GSLM_HIP_CHECK(hipHostGetDevicePointer((void**)&pinned_dev, pinned, 0));
    cap = n;
  }
  for (int32_t k0 = 0; k0 < n; k0 += READ_COUNTS_MAX) {
    CountPtrs c{};
    const int m = n - k0 < READ_COUNTS_MAX ? n - k0 : READ_COUNTS_MAX;
    for (int k = 0; k < m; ++k) {
      GeomBufs gb;
      geom_layout(Ps[k0 + k], const_cast<void*>(geoms[k0 + k]), &gb);
      c.p[k] = gb.counters;
    }
    hipLaunchKernelGGL(k_read_counts, dim3(1), dim3(64), 0, (hipStream_t)stream, c, m, pinned_dev + k0);
    GSLM_LAUNCH_CHECK();
  }
  GSLM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  for (int32_t k = 0; k < n; ++k) out[k] = (int64_t)pinned[k];
  return GSLM_OK;
}

int gslm_rasterize(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes,
                   int64_t N, void* image, size_t image_bytes, float* out_color, float* out_invdepth,
                   void* stream) {
  DebugScope dbg_scope(view != nullptr && view->debug != 0, stream);
  ViewK v;
  int st = make_view(view, 1, &v);
  if (st) return st;
  if (binning_bytes < gslm_binning_bytes(N, v.H, v.W)) { set_error("binning workspace too small"); return GSLM_ERR_CAPACITY; }
  if (image_bytes < gslm_image_bytes(v.H, v.W)) { set_error("image workspace too small"); return GSLM_ERR_CAPACITY; }
  if (!out_color) { set_error("out_color is NULL"); return GSLM_ERR_INVALID; }
  GeomBufs gb;
  BinBufs bb;
  ImgBufs ib;
  geom_layout(P, geom, &gb);
  bin_layout(N, v.gx * v.gy, binning, &bb);
  img_layout(v.H, v.W, image, &ib);
  hipStream_t s = (hipStream_t)stream;
  if ((st = launch_binning(v, P, gb, bb, N, s))) return st;
  return launch_render_fwd(v, gb, bb, ib, out_color, out_invdepth, s);
}

size_t gslm_loss_scratch_bytes(int32_t H, int32_t W) {
  const int64_t ntiles = (int64_t)((W + TILE_X - 1) / TILE_X) * ((H + TILE_Y - 1) / TILE_Y);
  return (size_t)(ntiles > 0 ? ntiles : 1) * sizeof(double);
}

// gslm_rasterize_loss and its exposure and robust forms: one body, `exposure` / `robust` NULL for the plain one
static int rasterize_loss(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes, int64_t N,
                          const float* gt, const float* alpha_mask, const float* exposure, bool want_exposure,
                          void* scratch, size_t scratch_bytes, double* loss_dev, int32_t accumulate, void* stream,
                          const gslm_robust* robust = nullptr, const DepthLossK* depth = nullptr) {
  bool rob = false;
  gslm_robust rb{};
  int st = robust_arg(robust, "rasterize_loss_robust", &rob, &rb);
  if (st) return st;
  ViewK v;
  st = make_view(view, 1, &v);
  if (st) return st;
  if (want_exposure && !exposure) { set_error("rasterize_loss_exposure: NULL exposure"); return GSLM_ERR_INVALID; }
  if (depth && !depth->gt) { set_error("rasterize_loss_depth: NULL invdepth_gt"); return GSLM_ERR_INVALID; }
  if (binning_bytes < gslm_binning_bytes(N, v.H, v.W)) { set_error("binning workspace too small"); return GSLM_ERR_CAPACITY; }
  if (scratch_bytes < gslm_loss_scratch_bytes(v.H, v.W)) { set_error("loss scratch too small"); return GSLM_ERR_CAPACITY; }
  if (!gt || !loss_dev || !scratch) { set_error("rasterize_loss: NULL gt / loss / scratch"); return GSLM_ERR_INVALID; }
  GeomBufs gb;
  BinBufs bb;
  geom_layout(P, geom, &gb);
  bin_layout(N, v.gx * v.gy, binning, &bb);
  hipStream_t s = (hipStream_t)stream;
  if ((st = launch_binning(v, P, gb, bb, N, s))) return st;
  return launch_render_loss(v, gb, bb, gt, alpha_mask, (double*)scratch, loss_dev, accumulate ? 1 : 0, s, nullptr, 0,
                            nullptr, exposure, rob ? &rb : nullptr, depth);
}

// depth_weight checked (finite, >= 0) into the loss blends' block
static int depth_loss_arg(const char* who, const float* invdepth_gt, const float* depth_mask, double depth_weight,
                          DepthLossK* out) {
  if (!(depth_weight >= 0.0) || !std::isfinite(depth_weight)) {
    set_error(std::string(who) + ": depth_weight must be finite and >= 0");
    return GSLM_ERR_INVALID;
  }
  *out = DepthLossK{invdepth_gt, depth_mask, 0.5 * depth_weight};
  return GSLM_OK;
}

int gslm_rasterize_loss_depth(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes,
                              int64_t N, const float* gt, const float* alpha_mask, const float* invdepth_gt,
                              const float* depth_mask, double depth_weight, void* scratch, size_t scratch_bytes,
                              double* loss_dev, int32_t accumulate, void* stream) {
  DepthLossK dl;
  if (int st = depth_loss_arg("rasterize_loss_depth", invdepth_gt, depth_mask, depth_weight, &dl)) return st;
  return rasterize_loss(view, P, geom, binning, binning_bytes, N, gt, alpha_mask, nullptr, false, scratch,
                        scratch_bytes, loss_dev, accumulate, stream, nullptr, &dl);
}

int gslm_rasterize_loss_robust(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes,
                               int64_t N, const float* gt, const float* alpha_mask, const gslm_robust* robust,
                               void* scratch, size_t scratch_bytes, double* loss_dev, int32_t accumulate,
                               void* stream) {
  return rasterize_loss(view, P, geom, binning, binning_bytes, N, gt, alpha_mask, nullptr, false, scratch,
                        scratch_bytes, loss_dev, accumulate, stream, robust);
}

int gslm_rasterize_loss(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes, int64_t N,
                        const float* gt, const float* alpha_mask, void* scratch, size_t scratch_bytes, double* loss_dev,
                        int32_t accumulate, void* stream) {
  return rasterize_loss(view, P, geom, binning, binning_bytes, N, gt, alpha_mask, nullptr, false, scratch,
                        scratch_bytes, loss_dev, accumulate, stream);
}

int gslm_rasterize_loss_exposure(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes,
                                 int64_t N, const float* gt, const float* alpha_mask, const float* exposure,
                                 void* scratch, size_t scratch_bytes, double* loss_dev, int32_t accumulate,
                                 void* stream) {
  return rasterize_loss(view, P, geom, binning, binning_bytes, N, gt, alpha_mask, exposure, true, scratch,
                        scratch_bytes, loss_dev, accumulate, stream);
}

// ---- device-count forms: the pair count stays on the device (no read-back between preprocess and binning) ----
int64_t gslm_binning_capacity(size_t binning_bytes, int32_t H, int32_t W) {
  if (H <= 0 || W <= 0 || binning_bytes < gslm_binning_bytes(0, H, W)) return 0;
  // gslm_binning_bytes is non-decreasing in N: the largest N that fits, by bisection
  int64_t lo = 0, hi = (int64_t)1 << 40;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (gslm_binning_bytes(mid, H, W) <= binning_bytes) lo = mid;
    else hi = mid;
  }
  return lo > (int64_t)0xFFFFFFFFu ? (int64_t)0xFFFFFFFFu : lo;
}

int gslm_rasterize_dev(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes, void* image,
                       size_t image_bytes, float* out_color, float* out_invdepth, uint32_t* n_out, void* stream) {
  DebugScope dbg_scope(view != nullptr && view->debug != 0, stream);
  ViewK v;
  int st = make_view(view, 1, &v);
  if (st) return st;
  if (image_bytes < gslm_image_bytes(v.H, v.W)) { set_error("image workspace too small"); return GSLM_ERR_CAPACITY; }
  if (!out_color) { set_error("out_color is NULL"); return GSLM_ERR_INVALID; }
  const int64_t cap = gslm_binning_capacity(binning_bytes, v.H, v.W);
  if (binning_bytes < gslm_binning_bytes(0, v.H, v.W)) { set_error("binning workspace too small"); return GSLM_ERR_CAPACITY; }
  GeomBufs gb;
  BinBufs bb;
  ImgBufs ib;
  geom_layout(P, geom, &gb);
  bin_layout(cap, v.gx * v.gy, binning, &bb);
  img_layout(v.H, v.W, image, &ib);
  hipStream_t s = (hipStream_t)stream;
  if ((st = launch_binning(v, P, gb, bb, cap, s, true, n_out))) return st;
  return launch_render_fwd(v, gb, bb, ib, out_color, out_invdepth, s);
}

int gslm_rasterize_loss_dev(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes,
                            const float* gt, const float* alpha_mask, void* scratch, size_t scratch_bytes, double* loss_dev,
                            int32_t accumulate, uint32_t* n_out, void* stream) {
  ViewK v;
  int st = make_view(view, 1, &v);
  if (st) return st;
  if (binning_bytes < gslm_binning_bytes(0, v.H, v.W)) { set_error("binning workspace too small"); return GSLM_ERR_CAPACITY; }
  if (scratch_bytes < gslm_loss_scratch_bytes(v.H, v.W)) { set_error("loss scratch too small"); return GSLM_ERR_CAPACITY; }
  if (!gt || !loss_dev || !scratch) { set_error("rasterize_loss: NULL gt / loss / scratch"); return GSLM_ERR_INVALID; }
  const int64_t cap = gslm_binning_capacity(binning_bytes, v.H, v.W);
  GeomBufs gb;
  BinBufs bb;
  geom_layout(P, geom, &gb);
  bin_layout(cap, v.gx * v.gy, binning, &bb);
  hipStream_t s = (hipStream_t)stream;
  if ((st = launch_binning(v, P, gb, bb, cap, s, true, n_out))) return st;
  return launch_render_loss(v, gb, bb, gt, alpha_mask, (double*)scratch, loss_dev, accumulate ? 1 : 0, s);
}

// ---- the line search's shared binning (ABI 8; forward.hip k_union_rect / k_duplicate_union) ----
size_t gslm_union_binning_bytes(int64_t N, int32_t H, int32_t W) {
  const int ntiles = ((W + TILE_X - 1) / TILE_X) * ((H + TILE_Y - 1) / TILE_Y);
  return union_masks_layout(N, ntiles, nullptr, nullptr);
}

size_t gslm_depth_records_bytes(int64_t P) { return depth_records_bytes(P); }

int gslm_union_geometry(const gslm_view* view, int64_t P, const void* const* geoms, int32_t n, size_t set_bytes,
                        void* union_geom, size_t union_geom_bytes, void* stream) {
  ViewK v;
  int st = make_view(view, 1, &v);
  if (st) return st;
  if (P < 0 || P > MAX_P) { set_error("P out of range [0, 2^28 - 1]"); return GSLM_ERR_INVALID; }
  if (union_geom_bytes < gslm_geom_bytes(P) || (!union_geom && P)) { set_error("union geometry workspace too small"); return GSLM_ERR_CAPACITY; }
  UnionSets u;
  if ((st = union_sets(geoms, n, P, set_bytes, &u))) return st;
  GeomBufs ug;
  geom_layout(P, union_geom, &ug);
  hipStream_t s = (hipStream_t)stream;
  if (P == 0) {
    GSLM_HIP_CHECK(hipMemsetAsync(ug.counters, 0, 4, s));
    return GSLM_OK;
  }
  if ((st = launch_union_rect(P, u, ug, s))) return st;
  // the union tile counts, already in depth order: k_duplicate_union's offsets, and the pair count in counters[0]
  return exclusive_scan_u32(ug.tiles, nullptr, ug.offsets, P, ug.scan_tmp, ug.counters, s);
}

int gslm_union_binning(const gslm_view* view, int64_t P, const void* union_geom, void* binning, size_t binning_bytes,
                       int64_t N, const void* const* geoms, int32_t n, size_t set_bytes, void* stream) {
  ViewK v;
  int st = make_view(view, 1, &v);
  if (st) return st;
  if (P < 0 || P > MAX_P || N < 0 || N > 0xFFFFFFFFll) { set_error("union_binning: P or N out of range"); return GSLM_ERR_INVALID; }
  if (binning_bytes < gslm_union_binning_bytes(N, v.H, v.W) || !binning) { set_error("union binning workspace too small"); return GSLM_ERR_CAPACITY; }
  if (P && !union_geom) { set_error("union_binning: NULL union geometry"); return GSLM_ERR_INVALID; }
  UnionSets u;
  if ((st = union_sets(geoms, n, P, set_bytes, &u))) return st;
  GeomBufs ug;
  BinBufs bb;
  UnionMasks um;
  geom_layout(P, const_cast<void*>(union_geom), &ug);
  bin_layout(N, v.gx * v.gy, binning, &bb);
  union_masks_layout(N, v.gx * v.gy, binning, &um);
  // the set count the masks are built for (gslm_rasterize_loss_slot renders a NaN loss for a slot past it)
  GSLM_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(um.nsets), (int)n, 1, (hipStream_t)stream));
  return launch_union_binning(v, P, ug, bb, um, N, u, (hipStream_t)stream);
}

static int rasterize_loss_slot(const gslm_view* view, int64_t P, const void* geom, size_t set_bytes,
                               const void* binning, size_t binning_bytes, int64_t N, int32_t slot, int32_t n_sets,
                               const float* gt, const float* alpha_mask, const float* exposure, bool want_exposure,
                               void* scratch, size_t scratch_bytes, double* loss_dev, int32_t accumulate,
                               void* stream, const gslm_robust* robust = nullptr, const DepthLossK* depth = nullptr) {
  bool rob = false;
  gslm_robust rb{};
  int st = robust_arg(robust, "rasterize_loss_slot_robust", &rob, &rb);
  if (st) return st;
  ViewK v;
  st = make_view(view, 1, &v);
  if (st) return st;
  if (depth && !depth->gt) { set_error("rasterize_loss_slot_depth: NULL invdepth_gt"); return GSLM_ERR_INVALID; }
  if (want_exposure && !exposure) { set_error("rasterize_loss_slot_exposure: NULL exposure"); return GSLM_ERR_INVALID; }
  if (n_sets < 1 || n_sets > MAX_UNION_SETS || slot < 0 || slot >= n_sets) {
    set_error("rasterize_loss_slot: need 0 <= slot < n_sets <= 8");
    return GSLM_ERR_INVALID;
  }
  if (set_bytes < depth_records_bytes(P)) { set_error("rasterize_loss_slot: set workspace below gslm_depth_records_bytes(P)"); return GSLM_ERR_CAPACITY; }
  if (N < 0 || N > 0xFFFFFFFFll) { set_error("rasterize_loss_slot: N out of range"); return GSLM_ERR_INVALID; }
  if (binning_bytes < gslm_union_binning_bytes(N, v.H, v.W) || !binning) { set_error("union binning workspace too small"); return GSLM_ERR_CAPACITY; }
  if (scratch_bytes < gslm_loss_scratch_bytes(v.H, v.W)) { set_error("loss scratch too small"); return GSLM_ERR_CAPACITY; }
  if (!gt || !loss_dev || !scratch) { set_error("rasterize_loss_slot: NULL gt / loss / scratch"); return GSLM_ERR_INVALID; }
  if (P && !geom) { set_error("rasterize_loss_slot: NULL geometry"); return GSLM_ERR_INVALID; }
  GeomBufs gb;
  BinBufs bb;
  UnionMasks um;
  geom_layout(P, const_cast<void*>(geom), &gb);
  bin_layout(N, v.gx * v.gy, const_cast<void*>(binning), &bb);
  union_masks_layout(N, v.gx * v.gy, const_cast<void*>(binning), &um);
  return launch_render_loss(v, gb, bb, gt, alpha_mask, (double*)scratch, loss_dev, accumulate ? 1 : 0,
                            (hipStream_t)stream, N > 0 ? um.sorted : nullptr, 4 * slot, um.nsets, exposure,
                            rob ? &rb : nullptr, depth);
}

int gslm_rasterize_loss_slot_depth(const gslm_view* view, int64_t P, const void* geom, size_t set_bytes,
                                   const void* binning, size_t binning_bytes, int64_t N, int32_t slot, int32_t n_sets,
                                   const float* gt, const float* alpha_mask, const float* invdepth_gt,
                                   const float* depth_mask, double depth_weight, void* scratch, size_t scratch_bytes,
                                   double* loss_dev, int32_t accumulate, void* stream) {
  DepthLossK dl;
  if (int st = depth_loss_arg("rasterize_loss_slot_depth", invdepth_gt, depth_mask, depth_weight, &dl)) return st;
  return rasterize_loss_slot(view, P, geom, set_bytes, binning, binning_bytes, N, slot, n_sets, gt, alpha_mask, nullptr,
                             false, scratch, scratch_bytes, loss_dev, accumulate, stream, nullptr, &dl);
}

int gslm_rasterize_loss_slot_robust(const gslm_view* view, int64_t P, const void* geom, size_t set_bytes,
                                    const void* binning, size_t binning_bytes, int64_t N, int32_t slot,
                                    int32_t n_sets, const float* gt, const float* alpha_mask,
                                    const gslm_robust* robust, void* scratch, size_t scratch_bytes, double* loss_dev,
                                    int32_t accumulate, void* stream) {
  return rasterize_loss_slot(view, P, geom, set_bytes, binning, binning_bytes, N, slot, n_sets, gt, alpha_mask, nullptr,
                             false, scratch, scratch_bytes, loss_dev, accumulate, stream, robust);
}

int gslm_rasterize_loss_slot(const gslm_view* view, int64_t P, const void* geom, size_t set_bytes, const void* binning,
                             size_t binning_bytes, int64_t N, int32_t slot, int32_t n_sets, const float* gt,
                             const float* alpha_mask, void* scratch, size_t scratch_bytes, double* loss_dev,
                             int32_t accumulate, void* stream) {
  return rasterize_loss_slot(view, P, geom, set_bytes, binning, binning_bytes, N, slot, n_sets, gt, alpha_mask, nullptr,
                             false, scratch, scratch_bytes, loss_dev, accumulate, stream);
}

int gslm_rasterize_loss_slot_exposure(const gslm_view* view, int64_t P, const void* geom, size_t set_bytes,
                                      const void* binning, size_t binning_bytes, int64_t N, int32_t slot,
                                      int32_t n_sets, const float* gt, const float* alpha_mask, const float* exposure,
                                      void* scratch, size_t scratch_bytes, double* loss_dev, int32_t accumulate,
                                      void* stream) {
  return rasterize_loss_slot(view, P, geom, set_bytes, binning, binning_bytes, N, slot, n_sets, gt, alpha_mask,
                             exposure, true, scratch, scratch_bytes, loss_dev, accumulate, stream);
}

size_t gslm_loss_sets_scratch_bytes(int32_t n, int32_t H, int32_t W) {
  return (size_t)(n > 0 ? n : 1) * gslm_loss_scratch_bytes(H, W);
}

static int rasterize_loss_sets(const gslm_view* view, int64_t P, const void* const* geoms, int32_t n,
                               int32_t first_set, size_t set_bytes, const void* binning, size_t binning_bytes,
                               int64_t N, const float* gt, const float* alpha_mask, const float* const* exposure,
                               bool want_exposure, void* scratch, size_t scratch_bytes, double* const* loss_dev,
                               int32_t accumulate, void* stream, const gslm_robust* robust = nullptr) {
  bool rob = false;
  gslm_robust rb{};
  int st = robust_arg(robust, "rasterize_loss_sets_robust", &rob, &rb);
  if (st) return st;
  ViewK v;
  st = make_view(view, 1, &v);
  if (st) return st;
  if (n < 1 || first_set < 0 || first_set + n > MAX_UNION_SETS) {
    set_error("rasterize_loss_sets: 1 <= n parameter sets, slots first_set .. first_set + n - 1 within [0, 8)");
    return GSLM_ERR_INVALID;
  }
  if (N < 0 || N > 0xFFFFFFFFll) { set_error("rasterize_loss_sets: N out of range"); return GSLM_ERR_INVALID; }
  if (binning_bytes < gslm_union_binning_bytes(N, v.H, v.W) || !binning) { set_error("union binning workspace too small"); return GSLM_ERR_CAPACITY; }
  if (scratch_bytes < gslm_loss_sets_scratch_bytes(n, v.H, v.W)) { set_error("loss scratch too small"); return GSLM_ERR_CAPACITY; }
  if (!gt || !loss_dev || !scratch || !geoms) { set_error("rasterize_loss_sets: NULL gt / loss / scratch / geoms"); return GSLM_ERR_INVALID; }
  if (set_bytes < depth_records_bytes(P)) { set_error("rasterize_loss_sets: set workspace below gslm_depth_records_bytes(P)"); return GSLM_ERR_CAPACITY; }
  if (want_exposure && !exposure) { set_error("rasterize_loss_sets_exposure: NULL exposure array"); return GSLM_ERR_INVALID; }
  SetRecsK sr{};
  LossPtrsK lp{};
  ExpPtrsK xp{};
  for (int a = 0; a < n; ++a) {
    if ((P && !geoms[a]) || !loss_dev[a]) { set_error("rasterize_loss_sets: NULL geometry / loss"); return GSLM_ERR_INVALID; }
    if (want_exposure) {
      if (!exposure[a]) { set_error("rasterize_loss_sets_exposure: NULL exposure entry"); return GSLM_ERR_INVALID; }
      xp.x[a] = exposure[a];
    }
    GeomBufs gb;
    geom_layout(P, const_cast<void*>(geoms[a]), &gb);
    sr.rec[a] = gb.rec;
    lp.loss[a] = loss_dev[a];
  }
  BinBufs bb;
  UnionMasks um;
  bin_layout(N, v.gx * v.gy, const_cast<void*>(binning), &bb);
  union_masks_layout(N, v.gx * v.gy, const_cast<void*>(binning), &um);
  // um.nsets: slots at or past the set count gslm_union_binning recorded render a NaN loss (as the slot form)
  return launch_render_loss_sets(v, sr, n, bb, um.sorted, gt, alpha_mask, (double*)scratch, lp, accumulate ? 1 : 0,
                                 (hipStream_t)stream, first_set, um.nsets, want_exposure ? &xp : nullptr,
                                 rob ? &rb : nullptr);
}

int gslm_rasterize_loss_sets_robust(const gslm_view* view, int64_t P, const void* const* geoms, int32_t n,
                                    int32_t first_set, size_t set_bytes, const void* binning, size_t binning_bytes,
                                    int64_t N, const float* gt, const float* alpha_mask, const gslm_robust* robust,
                                    void* scratch, size_t scratch_bytes, double* const* loss_dev, int32_t accumulate,
                                    void* stream) {
  return rasterize_loss_sets(view, P, geoms, n, first_set, set_bytes, binning, binning_bytes, N, gt, alpha_mask, nullptr,
                             false, scratch, scratch_bytes, loss_dev, accumulate, stream, robust);
}

int gslm_rasterize_loss_sets(const gslm_view* view, int64_t P, const void* const* geoms, int32_t n, int32_t first_set,
                             size_t set_bytes, const void* binning, size_t binning_bytes, int64_t N, const float* gt,
                             const float* alpha_mask, void* scratch, size_t scratch_bytes, double* const* loss_dev,
                             int32_t accumulate, void* stream) {
  return rasterize_loss_sets(view, P, geoms, n, first_set, set_bytes, binning, binning_bytes, N, gt, alpha_mask, nullptr,
                             false, scratch, scratch_bytes, loss_dev, accumulate, stream);
}

int gslm_rasterize_loss_sets_exposure(const gslm_view* view, int64_t P, const void* const* geoms, int32_t n,
                                      int32_t first_set, size_t set_bytes, const void* binning, size_t binning_bytes,
                                      int64_t N, const float* gt, const float* alpha_mask,
                                      const float* const* exposure, void* scratch, size_t scratch_bytes,
                                      double* const* loss_dev, int32_t accumulate, void* stream) {
  return rasterize_loss_sets(view, P, geoms, n, first_set, set_bytes, binning, binning_bytes, N, gt, alpha_mask,
                             exposure, true, scratch, scratch_bytes, loss_dev, accumulate, stream);
}

int gslm_num_rendered_copy(const void* geom, int64_t P, uint32_t* dst, void* stream) {
  if (!dst || (P > 0 && !geom)) { set_error("num_rendered_copy: NULL geom / dst"); return GSLM_ERR_INVALID; }
  if (P == 0) {
    GSLM_HIP_CHECK(hipMemsetAsync(dst, 0, 4, (hipStream_t)stream));
    return GSLM_OK;
  }
  GeomBufs gb;
  geom_layout(P, const_cast<void*>(geom), &gb);
  GSLM_HIP_CHECK(hipMemcpyAsync(dst, gb.counters, 4, hipMemcpyDefault, (hipStream_t)stream));
  return GSLM_OK;
}

int gslm_forward(const gslm_view* view, const gslm_gaussians* gi, void* geom, size_t geom_bytes, void* binning,
                 size_t binning_bytes, void* image, size_t image_bytes, float* out_color, float* out_invdepth,
                 int32_t* out_radii, int64_t* out_num_rendered, void* stream) {
  DebugScope dbg_scope(view != nullptr && view->debug != 0, stream);
  int st = gslm_preprocess(view, gi, geom, geom_bytes, out_radii, stream);
  if (st) return st;
  int64_t N = 0;
  if ((st = gslm_num_rendered(geom, gi->P, &N, stream))) return st;
  if (out_num_rendered) *out_num_rendered = N;
  if (binning_bytes < gslm_binning_bytes(N, view->image_height, view->image_width)) {
    set_error("binning workspace too small for num_rendered");
    return GSLM_ERR_CAPACITY;
  }
  return gslm_rasterize(view, gi->P, geom, binning, binning_bytes, N, image, image_bytes, out_color, out_invdepth,
                        stream);
}


static GradK make_gradk(const gslm_grads* o) {
  GradK k;
  k.means2D = o->means2D;
  k.means3D = o->means3D;
  k.opac = o->opacities;
  k.scales = o->scales;
  k.rot = o->rotations;
  k.cov3D = o->cov3D;
  k.dc = o->sh_dc;
  k.dc_stride = o->sh_dc_stride;
  k.rest = o->sh_rest;
  k.rest_stride = o->sh_rest_stride;
  k.colors = o->colors;
  k.accumulate = o->accumulate;
  return k;
}

static GaussK tangent_from_grads(const gslm_grads* t, const GaussK& g, bool mask_xyz) {
  GaussK k;
  k.P = g.P;
  k.raw = g.raw;
  k.M = g.M;
  k.means3D = mask_xyz ? nullptr : t->means3D;
  k.opac = t->opacities;
  k.scales = t->scales;
  k.rot = t->rotations;
  k.cov3D = t->cov3D;
  k.dc = t->sh_dc;
  k.dc_stride = t->sh_dc_stride;
  k.rest = t->sh_rest;
  k.rest_stride = t->sh_rest_stride;
  k.colors = t->colors;
  return k;
}

struct Bound {
  ViewK v;
  GaussK g;
  GeomBufs gb;
  BinBufs bb;
  ImgBufs ib;
  ScratchBufs sb;
};

static int bind_all(const gslm_view* view, const gslm_gaussians* gi, const void* geom, const void* binning,
                    int64_t N, const void* image, void* scratch, size_t scratch_bytes, Bound* b) {
  int st = make_view(view, gi ? gi->max_coeffs : 0, &b->v);
  if (st) return st;
  if ((st = make_gauss(gi, &b->v, &b->g, false))) return st;
  if (scratch_bytes < gslm_scratch_bytes(b->g.P, N)) {
    set_error("scratch workspace too small");
    return GSLM_ERR_CAPACITY;
  }
  geom_layout(b->g.P, const_cast<void*>(geom), &b->gb);
  bin_layout(N, b->v.gx * b->v.gy, const_cast<void*>(binning), &b->bb);
  img_layout(b->v.H, b->v.W, const_cast<void*>(image), &b->ib);
  scratch_layout(b->g.P, N, scratch, &b->sb);
  return GSLM_OK;
}

int gslm_backward(const gslm_view* view, const gslm_gaussians* gi, const void* geom, const void* binning, int64_t N,
                  const void* image, const float* dL_dcolor, const float* dL_dinvdepth, void* scratch,
                  size_t scratch_bytes, const gslm_grads* out, void* stream) {
  DebugScope dbg_scope(view != nullptr && view->debug != 0, stream);
  Bound b;
  int st = bind_all(view, gi, geom, binning, N, image, scratch, scratch_bytes, &b);
  if (st) return st;
  if (!out || !dL_dcolor) { set_error("backward: NULL dL_dcolor or outputs"); return GSLM_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  if ((st = launch_render_bwd(b.v, b.gb, b.bb, b.ib, N, dL_dcolor, dL_dinvdepth, b.sb, s))) return st;
  return launch_preprocess_bwd(b.v, b.g, b.gb, b.bb, b.sb, make_gradk(out), true, s);
}

int gslm_jvp(const gslm_view* view, const gslm_gaussians* gi, const gslm_gaussians* tangent,
             const float* means2D_tangent, const void* geom, const void* binning, int64_t N, const void* image,
             void* scratch, size_t scratch_bytes, float* out_color_t, float* out_invdepth_t, void* stream) {
  DebugScope dbg_scope(view != nullptr && view->debug != 0, stream);
  Bound b;
  int st = bind_all(view, gi, geom, binning, N, image, scratch, scratch_bytes, &b);
  if (st) return st;
  if (!out_color_t) { set_error("jvp: NULL out_color_t"); return GSLM_ERR_INVALID; }
  GaussK t;
  if ((st = make_gauss(tangent, &b.v, &t, true))) return st;
  t.P = b.g.P;
  t.raw = b.g.raw;
  t.M = b.g.M;
  return launch_jvp(b.v, b.g, t, means2D_tangent, b.gb, b.bb, b.ib, b.sb, out_color_t, out_invdepth_t,
                    (hipStream_t)stream);
}

// The fused CG direction update of gslm_matvec_opts (xpby_s .. xpby_x_offset) as a kernel argument; R is
// the SH-rest width of v and s (3(M-1), or 3 projected).
static int build_xpby(const gslm_matvec_opts* opts, const gslm_grads* vin, int R, bool mask_xyz, XpbyK* out) {
  const gslm_grads* sv = opts->xpby_s;
  if (!opts->beta_num || !opts->beta_den) {
    set_error("matvec: xpby needs the TANGENT stage and beta_num / beta_den");
    return GSLM_ERR_INVALID;
  }
  if (vin->sh_dc_stride != 3 || sv->sh_dc_stride != 3 || (R > 0 && (vin->sh_rest_stride != R || sv->sh_rest_stride != R))) {
    set_error("matvec: xpby needs contiguous SH groups (dc stride 3, rest stride 3(M-1), or 3 projected)");
    return GSLM_ERR_INVALID;
  }
  XpbyK xp{};
  float* pp[6] = {vin->means3D, vin->sh_dc, vin->sh_rest, vin->scales, vin->rotations, vin->opacities};
  const float* ss[6] = {sv->means3D, sv->sh_dc, sv->sh_rest, sv->scales, sv->rotations, sv->opacities};
  const int ww[6] = {3, 3, R, 3, 4, 1};
  for (int k = 0; k < 6; ++k) {
    if ((pp[k] == nullptr) != (ss[k] == nullptr) || (ww[k] == 0 && pp[k])) {
      set_error("matvec: xpby groups of v and s must match");
      return GSLM_ERR_INVALID;
    }
    // with mask_xyz the xyz group is left untouched: it is zero in every LM iterate (s and p alike)
    xp.p[k] = (ww[k] && !(k == 0 && mask_xyz)) ? pp[k] : nullptr;
    xp.s[k] = ss[k];
    xp.w[k] = ww[k];
  }
  xp.num = opts->beta_num;
  xp.den = opts->beta_den;
  xp.tail_p = opts->xpby_tail_n > 0 ? opts->xpby_tail_v : nullptr;
  xp.tail_s = opts->xpby_tail_s;
  xp.tail_n = opts->xpby_tail_n;
  if (xp.tail_p && !xp.tail_s) { set_error("matvec: xpby tail without s"); return GSLM_ERR_INVALID; }
  xp.anum = opts->alpha_num;
  xp.aden = opts->alpha_den;
  xp.xoff = opts->xpby_x_offset / (int64_t)sizeof(float);
  if (xp.anum && (!xp.aden || opts->xpby_x_offset % (int64_t)sizeof(float) != 0)) {
    set_error("matvec: deferred x update needs alpha_den and a float-aligned xpby_x_offset");
    return GSLM_ERR_INVALID;
  }
  *out = xp;
  return GSLM_OK;
}

static const uint32_t* active_params_bind(const void* block, int64_t na, GaussK* g);

// ---- the decoded product call: every refusal of the product entry points happens while a Plan is built, before the
// first launch; running a Plan can fail on a HIP error only ----
// A call as bits: the entry point (E_*), and what its options and arguments ask for (F_*).
enum : uint32_t {
  E_MATVEC_EX = 1u << 0, E_MATVEC_ACTIVE = 1u << 1, E_GATHER_SCREEN = 1u << 2, E_GATHER_VIEWS = 1u << 3,
  E_TANGENT_VIEWS = 1u << 4, E_MATVEC = E_MATVEC_EX | E_MATVEC_ACTIVE, E_GATHER = E_GATHER_SCREEN | E_GATHER_VIEWS,
  F_LEAN = 1u << 5, F_EXPOSURE = 1u << 6, F_DAMP_VEC = 1u << 7, F_PROJECTED = 1u << 8, F_SEED = 1u << 9,
  F_JV_OUT = 1u << 10, F_TREC_IN = 1u << 11, F_REST_BASIS = 1u << 12, F_DAMP7 = 1u << 13, F_XPBY = 1u << 14,
  F_TANGENT = 1u << 15, F_RENDER = 1u << 16, F_GATHER = 1u << 17, F_SCREEN = 1u << 18, F_OVERWRITE = 1u << 19,
  F_UNMASKED = 1u << 20,    // mask_xyz = 0
  F_TAIL_DIRTY = 1u << 21,  // no GSLM_MV_TAIL_CLEAN
  F_DEPTH = 1u << 22,       // GSLM_MV_DEPTH
  F_XYZ = 1u << 23,         // GSLM_MV_XYZ
  F_LIST = 1u << 24,        // the union-list form of an entry point (gslm_gather_views_active, gslm_tangent_views_active)
};
// Which go together, once: a call in `mode` with any of `excludes` is refused (GSLM_ERR_INVALID).
static const struct { uint32_t mode, excludes; const char* msg; } kExcludes[] = {
    {E_GATHER, F_DAMP_VEC, "gather: GSLM_MV_DAMP_VEC is an option of gslm_matvec_view_ex / gslm_matvec_view_active"},
    {E_MATVEC_EX, F_LEAN, "matvec: GSLM_MV_LEAN is an option of gslm_matvec_view_active"},
    {E_MATVEC, F_REST_BASIS, "matvec: rest_basis is an option of gslm_tangent_views / gslm_gather_screen"},
    {E_MATVEC_ACTIVE, F_UNMASKED | F_TAIL_DIRTY | F_SCREEN | F_TREC_IN,
     "matvec_view_active: needs mask_xyz and GSLM_MV_TAIL_CLEAN (the list comes from that row map); no SCREEN stage, "
     "no trec_in"},
    {F_DAMP_VEC, F_DAMP7 | F_LEAN | F_EXPOSURE | F_UNMASKED | F_SEED | F_JV_OUT | F_SCREEN | F_TREC_IN | F_REST_BASIS,
     "matvec: GSLM_MV_DAMP_VEC needs mask_xyz and excludes damp7, pixel_seed, jv_out, the SCREEN stage, trec_in, "
     "rest_basis, GSLM_MV_LEAN and GSLM_MV_EXPOSURE"},
    {F_EXPOSURE, F_LEAN | F_UNMASKED | F_SEED | F_JV_OUT | F_SCREEN | F_TREC_IN | F_REST_BASIS,
     "matvec: GSLM_MV_EXPOSURE needs mask_xyz and excludes pixel_seed, jv_out, the SCREEN stage, trec_in, rest_basis "
     "and GSLM_MV_LEAN"},
    {F_PROJECTED, F_SCREEN, "matvec: GSLM_MV_SH_REST_PROJECTED is a single-view mode (no SCREEN stage)"},
    {F_TREC_IN, F_TANGENT, "matvec: trec_in replaces the TANGENT stage"},
    {F_SEED, F_UNMASKED | F_XPBY | F_TANGENT | F_SCREEN,
     "matvec: pixel_seed (J^T seed) needs mask_xyz and excludes TANGENT / SCREEN / xpby"},
    {F_JV_OUT, F_SEED | F_GATHER | F_SCREEN, "matvec: jv_out excludes pixel_seed, GATHER and SCREEN"},
    {F_DEPTH, F_UNMASKED | F_EXPOSURE | F_DAMP_VEC | F_JV_OUT | F_SCREEN | E_GATHER | E_TANGENT_VIEWS,
     "GSLM_MV_DEPTH is an option of gslm_matvec_view_ex / gslm_matvec_view_active on the LM rows (mask_xyz); it "
     "excludes GSLM_MV_EXPOSURE, GSLM_MV_DAMP_VEC, jv_out and the SCREEN stage"},
    {F_XYZ, E_MATVEC | E_GATHER_SCREEN | E_TANGENT_VIEWS | F_LIST | F_DAMP_VEC | F_DEPTH | F_EXPOSURE,
     "GSLM_MV_XYZ is an option of gslm_gather_views (the matvec entry points have mask_xyz; the list forms, "
     "gslm_gather_screen and gslm_tangent_views run without it); it excludes GSLM_MV_DAMP_VEC, GSLM_MV_DEPTH and "
     "GSLM_MV_EXPOSURE"},
};
static bool excluded(uint32_t f, uint32_t mode) {
  for (const auto& r : kExcludes)
    if (r.mode == mode && (f & mode) && (f & r.excludes)) {
      set_error(r.msg);
      return true;
    }
  return false;
}

struct Plan {
  uint32_t f;                  // E_* | F_*
  int64_t rows;                // rows of every group of vin and y
  const double* stop;          // cg_ctl -> ViewK::stop
  const double* damp7;
  DampVecK dvec;               // F_DAMP_VEC
  double *dot_out, *part;      // <v, y> and the gather's partials of it (dot_defer: the partials alone)
  XpbyK xp;                    // F_XPBY, with the lean beta partials
  GaussK t;                    // the tangent: vin's groups
  GaussK gp;                   // the parameters the kernels read: g, or the list-order block (then with clamp_list)
  const uint32_t* clamp_list;
  const int32_t* ids;          // the active list (na < 0: none)
  const uint32_t* hrow;
  int64_t na;
  const gslm_matvec_opts* o;   // trec_in, pixel_seed, jv_out and screen_out are read from the options as they are
  const gslm_exposure_opts* expo;
  RestK rc;
  bool gather;                 // GATHER runs (no jv_out, no SCREEN); flat is built when it has rows
  FlatK flat;
};

// The base options of `entry`; `accepts`: the F_* bits that entry point decodes (the others it has always ignored).
static void plan_base(uint32_t entry, uint32_t accepts, const gslm_matvec_opts* o, bool mask_xyz, int M, Plan* pl) {
  *pl = Plan{};
  const int32_t st = (o && o->stages) ? o->stages : GSLM_STAGE_ALL, fl = o ? o->flags : 0;
  uint32_t f = (st & GSLM_STAGE_TANGENT ? F_TANGENT : 0) | (st & GSLM_STAGE_RENDER ? F_RENDER : 0) |
               (st & GSLM_STAGE_GATHER ? F_GATHER : 0) | (st & GSLM_STAGE_SCREEN ? F_SCREEN : 0) |
               (st & GSLM_STAGE_OVERWRITE ? F_OVERWRITE : 0) | (fl & GSLM_MV_LEAN ? F_LEAN : 0) |
               (fl & GSLM_MV_EXPOSURE ? F_EXPOSURE : 0) | (fl & GSLM_MV_DAMP_VEC ? F_DAMP_VEC : 0) |
               (fl & GSLM_MV_DEPTH ? F_DEPTH : 0) | (fl & GSLM_MV_XYZ ? F_XYZ : 0) |
               ((fl & GSLM_MV_SH_REST_PROJECTED) && M > 1 ? F_PROJECTED : 0) | (fl & GSLM_MV_TAIL_CLEAN ? 0 : F_TAIL_DIRTY) |
               (mask_xyz ? 0 : F_UNMASKED);
  if (o) f |= (o->pixel_seed ? F_SEED : 0) | (o->jv_out ? F_JV_OUT : 0) | (o->trec_in ? F_TREC_IN : 0) |
              (o->rest_basis ? F_REST_BASIS : 0) | (o->damp7 ? F_DAMP7 : 0) | (o->xpby_s ? F_XPBY : 0);
  pl->f = entry | (f & (accepts | F_TANGENT | F_RENDER | F_GATHER | F_OVERWRITE | F_UNMASKED | F_TAIL_DIRTY));
  pl->o = o;
  pl->stop = o ? o->cg_ctl : nullptr;
  pl->damp7 = (pl->f & F_DAMP7) ? o->damp7 : nullptr;
  pl->na = -1;
}

// dot_vy and its scratch over `rows` rows (defer: GSLM_MV_LEAN's dot_defer, the partials without the finished dot)
static int plan_dot(const char* who, int64_t rows, bool defer, Plan* pl) {
  pl->dot_out = pl->o ? pl->o->dot_vy : nullptr;
  if (!pl->dot_out && !defer) return GSLM_OK;
  if (!pl->o->dot_scratch || pl->o->dot_scratch_bytes < gslm_dot_scratch_bytes(rows)) {
    set_error(std::string(who) + ": dot scratch too small");
    return GSLM_ERR_CAPACITY;
  }
  pl->part = (double*)pl->o->dot_scratch;
  return GSLM_OK;
}

// FlatK over a flat param-space output y and input v (GradK views of the 7-group vectors).
static int make_flatk(const GaussK& g, const GradK& y, const GradK& vin, const double* damp7, bool overwrite,
                      double* dot_part, FlatK* out, bool rest_proj = false, int rest_V = 0) {
  const int64_t R = rest_V ? 3 * rest_V : rest_proj ? 3 : 3 * (g.M - 1);
  if (g.cov3D || g.colors || !g.raw || (g.M > 1 && y.rest_stride != R) || y.dc_stride != 3) {
    set_error("LM gather expects raw leaves with SH colours and a flat param-space output");
    return GSLM_ERR_INVALID;
  }
  if (rest_proj && g.M > 1 && vin.rest && vin.rest_stride != 3) {
    set_error("LM gather: a projected SH-rest group has 3 floats per Gaussian in v and y");
    return GSLM_ERR_INVALID;
  }
  if (rest_V && g.M > 1 && vin.rest && vin.rest_stride != R) {
    set_error("LM gather: SH-rest coordinates need 3 rest_views floats per Gaussian in v and y");
    return GSLM_ERR_INVALID;
  }
  FlatK o;
  o.y[0] = y.means3D; o.y[1] = y.dc; o.y[2] = y.rest; o.y[3] = y.scales; o.y[4] = y.rot; o.y[5] = y.opac;
  o.v[0] = vin.means3D; o.v[1] = vin.dc; o.v[2] = vin.rest; o.v[3] = vin.scales; o.v[4] = vin.rot; o.v[5] = vin.opac;
  // damp7 = xyz, dc, rest, scaling, rotation, opacity, exposure (GaussianModelDampMatrix order)
  for (int k = 0; k < 6; ++k) o.damp[k] = damp7 ? (float)damp7[k] : 0.f;
  o.use_damp = damp7 ? 1 : 0;
  o.overwrite = overwrite ? 1 : 0;
  o.rest_proj = (rest_proj && g.M > 1) ? 1 : 0;
  o.rest_V = g.M > 1 ? rest_V : 0;
  o.dot_part = dot_part;
  if (o.use_damp || dot_part)
    for (int k = 0; k < 6; ++k)
      if (!o.v[k] && !(k == 2 && g.M == 1)) {
        set_error("damping needs every group of v");
        return GSLM_ERR_INVALID;
      }
  *out = o;
  return GSLM_OK;
}

// The GATHER stage's FlatK from the plan's damp7, OVERWRITE, partials, projection and SH-rest coordinates.
static int plan_flat(const GaussK& g, const gslm_grads* y, const gslm_grads* vin, Plan* pl) {
  if ((pl->f & F_XYZ) && (!y->means3D || !vin->means3D)) {
    set_error("gather_views: GSLM_MV_XYZ needs the xyz groups of v and y");
    return GSLM_ERR_INVALID;
  }
  return make_flatk(g, make_gradk(y), make_gradk(vin), pl->damp7, (pl->f & F_OVERWRITE) != 0, pl->part, &pl->flat,
                    (pl->f & F_PROJECTED) != 0, pl->rc.R ? pl->rc.V : 0);
}

// The plan of gslm_matvec_view_ex (na < 0) and gslm_matvec_view_active (na >= 0: the groups of vin, y and the fused
// direction update hold the na Gaussians ids[0 .. na) only).  Every set_error of the two calls is here; it calls no
// HIP function and writes nothing but *pl.
static int plan_matvec(uint32_t entry, const gslm_matvec_opts* opts, const Bound& b, const gslm_grads* vin,
                       const gslm_grads* y, const float* pixel_weight, bool mask_xyz, const int32_t* ids, int64_t na,
                       const uint32_t* hrow, Plan* pl) {
  if (!vin || !y || !pixel_weight) { set_error("matvec: NULL argument"); return GSLM_ERR_INVALID; }
  plan_base(entry, ~0u, opts, mask_xyz, b.g.M, pl);
  const uint32_t f = pl->f;
  int st;
  // (one extension struct lies behind the base: a flag's exclusions are checked before its extension is read)
  if (excluded(f, F_XYZ) || excluded(f, F_DEPTH) || excluded(f, F_DAMP_VEC) || excluded(f, E_MATVEC_EX) ||
      excluded(f, F_EXPOSURE))
    return GSLM_ERR_INVALID;
  // GSLM_MV_EXPOSURE: opts is the base of a gslm_matvec_opts_exposure; RENDER runs the product under the camera's
  // trained exposure and sums the 12 exposure rows
  if (f & F_EXPOSURE) {
    const gslm_exposure_opts* expo = &reinterpret_cast<const gslm_matvec_opts_exposure*>(opts)->exposure;
    if (!expo->exposure || !expo->v_rows || !expo->y_rows || !expo->color || !expo->u_image || !expo->scratch) {
      set_error("matvec: GSLM_MV_EXPOSURE with a NULL member of gslm_exposure_opts");
      return GSLM_ERR_INVALID;
    }
    if (expo->scratch_bytes < gslm_exposure_scratch_bytes(b.v.H, b.v.W)) {
      set_error("matvec: GSLM_MV_EXPOSURE scratch below gslm_exposure_scratch_bytes");
      return GSLM_ERR_CAPACITY;
    }
    pl->expo = expo;
  }
  // GSLM_MV_DAMP_VEC: opts is the base of a gslm_matvec_opts_damp; GATHER adds d (.) v with d read per element
  if (f & F_DAMP_VEC) {
    const gslm_grads* d = reinterpret_cast<const gslm_matvec_opts_damp*>(opts)->damp_vec;
    if (!d || !d->means3D || !d->sh_dc || (b.g.M > 1 && !d->sh_rest) || !d->scales || !d->rotations || !d->opacities) {
      set_error("matvec: GSLM_MV_DAMP_VEC with a NULL damp_vec or a NULL group of it");
      return GSLM_ERR_INVALID;
    }
    if (d->sh_dc_stride != y->sh_dc_stride || (b.g.M > 1 && d->sh_rest_stride != y->sh_rest_stride)) {
      set_error("matvec: GSLM_MV_DAMP_VEC: damp_vec has the groups and strides of v and y");
      return GSLM_ERR_INVALID;
    }
    pl->dvec = DampVecK{{d->means3D, d->sh_dc, d->sh_rest, d->scales, d->rotations, d->opacities}};
  }
  const bool active = na >= 0;
  pl->rows = active ? na : b.g.P;
  if (active && (na > b.g.P || (na > 0 && (!ids || !hrow)))) {
    set_error("matvec_view_active: 0 <= n_active <= P, a non-NULL list and its row offsets");
    return GSLM_ERR_INVALID;
  }
  if (excluded(f, E_MATVEC_ACTIVE)) return GSLM_ERR_INVALID;
  pl->ids = ids;
  pl->hrow = hrow;
  pl->na = na;
  // GSLM_MV_LEAN: opts is the base of a gslm_matvec_opts_lean; <v, y> may stay as the gather's partials (dot_defer)
  const gslm_cg_lean* lean = (f & F_LEAN) ? &reinterpret_cast<const gslm_matvec_opts_lean*>(opts)->lean : nullptr;
  const bool dot_defer = lean && lean->dot_defer;
  if (dot_defer && opts->dot_vy) {
    set_error("matvec_view_active (GSLM_MV_LEAN): dot_defer leaves <v, y> as partials in dot_scratch (dot_vy must be NULL)");
    return GSLM_ERR_INVALID;
  }
  if ((st = plan_dot("matvec", pl->rows, dot_defer, pl))) return st;
  if (!b.g.raw) { set_error("matvec: gaussians must be the raw GaussianModel leaves (raw = 1)"); return GSLM_ERR_INVALID; }
  if (excluded(f, E_MATVEC)) return GSLM_ERR_INVALID;
  pl->t = tangent_from_grads(vin, b.g, mask_xyz);
  if (f & F_PROJECTED) {
    if (vin->sh_rest && vin->sh_rest_stride != 3) {
      set_error("matvec: a projected SH-rest group has 3 floats per Gaussian (sh_rest_stride 3)");
      return GSLM_ERR_INVALID;
    }
    if (excluded(f, F_PROJECTED)) return GSLM_ERR_INVALID;
    pl->t.rest_proj = 1;
  }
  if (f & F_XPBY) {
    if (!(f & F_TANGENT)) {
      set_error("matvec: xpby needs the TANGENT stage and beta_num / beta_den");
      return GSLM_ERR_INVALID;
    }
    if ((st = build_xpby(opts, vin, (f & F_PROJECTED) ? 3 : 3 * (b.g.M - 1), mask_xyz, &pl->xp))) return st;
    if (lean && lean->beta_partials) {
      if (lean->beta_np < 0 || lean->beta_partials == opts->dot_scratch) {
        set_error("matvec_view_active (GSLM_MV_LEAN): beta's partials need a count and a buffer other than dot_scratch");
        return GSLM_ERR_INVALID;
      }
      pl->xp.num_part = (const double*)lean->beta_partials;
      pl->xp.num_np = lean->beta_np;
      pl->xp.num_store = lean->beta_store;
    }
  } else if (lean && lean->beta_partials) {
    set_error("matvec_view_active (GSLM_MV_LEAN): beta's partials without the fused direction update (xpby_s)");
    return GSLM_ERR_INVALID;
  }
  // the list-order parameter block (gslm_active_params): the ACTIVE kernels read row j of it, not row ids[j] of g
  // (GSLM_MV_LEAN is the active entry point's, so there is a list)
  pl->gp = b.g;
  if (lean && lean->params) pl->clamp_list = active_params_bind(lean->params, na, &pl->gp);
  if (excluded(f, F_TREC_IN) || excluded(f, F_SEED) || excluded(f, F_JV_OUT)) return GSLM_ERR_INVALID;
  if ((f & F_SCREEN) && (!mask_xyz || !opts->screen_out)) {
    set_error("matvec: GSLM_STAGE_SCREEN needs mask_xyz and opts->screen_out");
    return GSLM_ERR_INVALID;
  }
  pl->gather = (f & F_GATHER) && !(f & (F_JV_OUT | F_SCREEN));
  if (!pl->gather || pl->rows == 0) return GSLM_OK;
  if ((st = plan_flat(pl->gp, y, vin, pl))) return st;
  if (f & F_DAMP_VEC) {  // d's groups are checked above; make_flatk asks for v's with damp7 or a dot only
    for (int k = 0; k < 6; ++k)
      if (!pl->flat.v[k] && !(k == 2 && b.g.M == 1)) {
        set_error("matvec: GSLM_MV_DAMP_VEC needs every group of v");
        return GSLM_ERR_INVALID;
      }
    pl->flat.use_damp = 1;
  }
  return GSLM_OK;
}

// Runs a plan of plan_matvec: up to four stages, no refusal left.
static int run_matvec(Bound& b, const Plan& pl, const float* pixel_weight, int64_t N, void* stream) {
  const uint32_t f = pl.f;
  const bool mask = !(f & F_UNMASKED), tail_clean = !(f & F_TAIL_DIRTY);
  hipStream_t s = (hipStream_t)stream;
  int st;
  b.v.stop = pl.stop;
  if (f & F_TREC_IN) b.sb.trec = reinterpret_cast<float4*>(const_cast<float*>(pl.o->trec_in));
  if ((f & F_TANGENT) && (st = launch_tangent_pre(b.v, pl.gp, pl.t, nullptr, b.gb, b.sb, (f & F_XPBY) ? &pl.xp : nullptr,
                                                  s, mask, pl.ids, pl.na, pl.clamp_list)))
    return st;
  if (f & F_JV_OUT) {
    if (!(f & F_RENDER)) return GSLM_OK;
    if (N > 0) return launch_render_jv(b.v, pl.t, b.gb, b.bb, b.ib, b.sb, mask, pl.o->jv_out, s);
    GSLM_HIP_CHECK(hipMemsetAsync(pl.o->jv_out, 0, (size_t)3 * b.v.H * b.v.W * sizeof(float), s));
    return GSLM_OK;
  }
  const bool render = (f & F_RENDER) != 0;
  if (render && (f & F_SEED)) {
    if ((st = launch_render_vjp_lm(b.v, b.gb, b.bb, b.ib, N, pl.o->pixel_seed, b.sb, tail_clean, s,
                                   (f & F_DEPTH) != 0)))
      return st;
  } else if (render && (f & F_EXPOSURE)) {
    const gslm_exposure_opts* expo = pl.expo;
    const ExposureK ex{expo->exposure, expo->v_rows, expo->color, expo->u_image};
    if (N > 0)
      st = launch_matvec_render_exposure(b.v, pl.t, b.gb, b.bb, b.ib, b.sb, N, pixel_weight, ex, tail_clean, s);
    else  // an empty list: no tile pass, J v = 0, and the exposure columns alone remain
      st = launch_exposure_u_empty(b.v.H, b.v.W, ex.color, pixel_weight, ex.V, b.v.stop, ex.u, s);
    if (st) return st;
    if ((st = launch_exposure_rows(b.v.H, b.v.W, ex.color, ex.u, ex.V, (float)expo->damp, expo->overwrite != 0,
                                   b.v.stop, (double*)expo->scratch, expo->y_rows, s)))
      return st;
  } else if (render && N > 0 &&
             (st = launch_matvec_render(b.v, pl.t, b.gb, b.bb, b.ib, b.sb, N, pixel_weight, mask, tail_clean, s,
                                        (f & F_DEPTH) != 0))) {
    return st;
  }
  if (f & F_SCREEN) return launch_rowsum_screen(b.g, b.gb, b.sb, pl.o->screen_out, s);
  if (!pl.gather) return GSLM_OK;
  if ((st = launch_gather_lm(b.v, pl.gp, b.gb, b.sb, pl.flat, mask, s, pl.ids, pl.na, pl.hrow, pl.clamp_list,
                             (f & F_DAMP_VEC) ? &pl.dvec : nullptr)))
    return st;
  if (pl.dot_out) return gslm_dot_finalize(pl.part, (int32_t)((pl.rows + 255) / 256), pl.dot_out, stream);
  return GSLM_OK;
}

// bind_all, build the plan, run the plan
static int matvec_view(uint32_t entry, const gslm_view* view, const gslm_gaussians* gi, const gslm_grads* vin,
                       const float* pixel_weight, int32_t mask_xyz, const void* geom, const void* binning,
                       int64_t N, const void* image, void* scratch, size_t scratch_bytes, const gslm_grads* y,
                       const gslm_matvec_opts* opts, const int32_t* ids, int64_t na, const uint32_t* hrow,
                       void* stream) {
  DebugScope dbg_scope(view != nullptr && view->debug != 0, stream);
  Bound b;
  Plan pl;
  int st = bind_all(view, gi, geom, binning, N, image, scratch, scratch_bytes, &b);
  if (st) return st;
  if ((st = plan_matvec(entry, opts, b, vin, y, pixel_weight, mask_xyz != 0, ids, na, hrow, &pl))) return st;
  return run_matvec(b, pl, pixel_weight, N, stream);
}

int gslm_matvec_view_ex(const gslm_view* view, const gslm_gaussians* gi, const gslm_grads* vin,
                        const float* pixel_weight, int32_t mask_xyz, const void* geom, const void* binning,
                        int64_t N, const void* image, void* scratch, size_t scratch_bytes, const gslm_grads* y,
                        const gslm_matvec_opts* opts, void* stream) {
  return matvec_view(E_MATVEC_EX, view, gi, vin, pixel_weight, mask_xyz, geom, binning, N, image, scratch, scratch_bytes,
                     y, opts, nullptr, -1, nullptr, stream);
}

int gslm_matvec_view_active(const gslm_view* view, const gslm_gaussians* gi, const gslm_grads* vin,
                            const float* pixel_weight, int32_t mask_xyz, const void* geom, const void* binning,
                            int64_t N, const void* image, void* scratch, size_t scratch_bytes, const gslm_grads* y,
                            const gslm_matvec_opts* opts, const int32_t* active_ids, const uint32_t* active_rows,
                            int64_t n_active, void* stream) {
  if (n_active < 0) { set_error("matvec_view_active: negative n_active"); return GSLM_ERR_INVALID; }
  return matvec_view(E_MATVEC_ACTIVE, view, gi, vin, pixel_weight, mask_xyz, geom, binning, N, image, scratch,
                     scratch_bytes, y, opts, active_ids, n_active, active_rows, stream);
}

// diag(2 J^T diag(w) J [+ D]) of the matrix gslm_matvec_view_ex applies (solver_functions.py:83-132), one view
int gslm_lm_diag_view(const gslm_view* view, const gslm_gaussians* gi, const float* pixel_weight, int32_t mask_xyz,
                      const void* geom, const void* binning, int64_t N, const void* image, void* scratch,
                      size_t scratch_bytes, const gslm_grads* diag, const double* damp7, int32_t flags, void* stream) {
  // every check before any launch: an error return leaves the destination untouched
  if (!mask_xyz) {
    set_error("lm_diag_view: the diagonal is the LM rows' (mask_xyz = 1: no colour x geometry cross terms)");
    return GSLM_ERR_INVALID;
  }
  if (!pixel_weight || !diag) {
    set_error("lm_diag_view: NULL pixel_weight or destination");
    return GSLM_ERR_INVALID;
  }
  if (flags & ~(GSLM_DIAG_TAIL_CLEAN | GSLM_DIAG_ACCUMULATE | GSLM_DIAG_SH_REST_PROJECTED)) {
    set_error("lm_diag_view: unknown flag bits");
    return GSLM_ERR_INVALID;
  }
  if (!view || !gi || !geom || !image || !scratch || N < 0 || (N > 0 && !binning)) {
    set_error("lm_diag_view: NULL view, gaussians or workspace, or a negative pair count");
    return GSLM_ERR_INVALID;
  }
  Bound b;
  int st = bind_all(view, gi, geom, binning, N, image, scratch, scratch_bytes, &b);
  if (st) return st;
  if (!b.g.raw || b.g.cov3D || b.g.colors) {
    set_error("lm_diag_view: gaussians must be the raw GaussianModel leaves with SH colours");
    return GSLM_ERR_INVALID;
  }
  const bool proj = (flags & GSLM_DIAG_SH_REST_PROJECTED) && b.g.M > 1;
  const int64_t R = proj ? 3 : 3 * (b.g.M - 1);
  if ((diag->sh_dc && diag->sh_dc_stride != 3) || (diag->sh_rest && b.g.M > 1 && diag->sh_rest_stride != R)) {
    set_error("lm_diag_view: the destination is a flat param-space vector (dc stride 3, rest stride 3(M-1), or 3 "
              "projected)");
    return GSLM_ERR_INVALID;
  }
  DebugScope dbg_scope(view->debug != 0, stream);
  return launch_lm_diag(b.v, b.g, b.gb, b.bb, b.ib, b.sb, N, pixel_weight, make_gradk(diag), damp7,
                        !(flags & GSLM_DIAG_ACCUMULATE), proj, (flags & GSLM_DIAG_TAIL_CLEAN) != 0,
                        (hipStream_t)stream);
}

// The list-order parameter block: [xyz 3 | raw scale 3 | raw rotation 4 | raw opacity 1] floats and the clamp
// word, each an array over the na listed Gaussians -- everything chain_jvp / chain_vjp load per Gaussian on the LM
// rows (xyz frozen: the primal SH coefficients are not read).
static size_t active_params_layout(int64_t na, void* base, float** xyz, float** sc, float** rot, float** op,
                                   uint32_t** cw) {
  Carver c{(char*)base};
  const int64_t n = na > 0 ? na : 1;
  float* a = c.take<float>(3 * n);
  float* b = c.take<float>(3 * n);
  float* r = c.take<float>(4 * n);
  float* o = c.take<float>(n);
  uint32_t* w = c.take<uint32_t>(n);
  if (xyz) { *xyz = a; *sc = b; *rot = r; *op = o; *cw = w; }
  return c.off;
}

static const uint32_t* active_params_bind(const void* block, int64_t na, GaussK* g) {
  float *xyz, *sc, *rot, *op;
  uint32_t* cw;
  active_params_layout(na, const_cast<void*>(block), &xyz, &sc, &rot, &op, &cw);
  g->means3D = xyz;
  g->scales = sc;
  g->rot = rot;
  g->opac = op;
  return cw;
}

size_t gslm_active_params_bytes(int64_t n_active) {
  return active_params_layout(n_active, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int gslm_active_params(const gslm_gaussians* gi, const void* geom, int64_t P, const int32_t* active_ids,
                       int64_t n_active, void* block, size_t block_bytes, int32_t* pos_dev, void* stream) {
  if (!gi || !geom || P < 0 || n_active < 0 || n_active > P || !block || !pos_dev || (n_active > 0 && !active_ids)) {
    set_error("active_params: NULL argument or 0 <= n_active <= P violated");
    return GSLM_ERR_INVALID;
  }
  if (block_bytes < gslm_active_params_bytes(n_active)) {
    set_error("active_params: block smaller than gslm_active_params_bytes(n_active)");
    return GSLM_ERR_CAPACITY;
  }
  if (gi->P != P || !gi->raw || gi->cov3D_precomp || gi->colors_precomp ||
      (P > 0 && (!gi->means3D || !gi->scales || !gi->rotations || !gi->opacities))) {
    set_error("active_params: the raw GaussianModel leaves of the P Gaussians the list was built for");
    return GSLM_ERR_INVALID;
  }
  GeomBufs gb;
  geom_layout(P, const_cast<void*>(geom), &gb);
  float *xyz, *sc, *rot, *op;
  uint32_t* cw;
  active_params_layout(n_active, block, &xyz, &sc, &rot, &op, &cw);
  return launch_active_params(gi->means3D, gi->scales, gi->rotations, gi->opacities, gb.clampw, active_ids, n_active,
                              P, xyz, sc, rot, op, cw, pos_dev, (hipStream_t)stream);
}

int gslm_cg_start_active(const float* g_full, const int32_t* active_ids, int64_t n_active, int64_t P,
                         const int32_t* widths, int32_t ngroups, int64_t tail_n, int64_t lo, float* s, float* p,
                         float* q, float* x, void* partials, void* stream) {
  return launch_cg_start_active(g_full, active_ids, n_active, P, widths, ngroups, tail_n, lo, s, p, q, x,
                                (double*)partials, (hipStream_t)stream);
}

int gslm_cg_end_active(const float* x, const float* p, const double* num_dev, const double* den_dev, int64_t lo,
                       const int32_t* pos_dev, int64_t n_active, int64_t P, const int32_t* widths, int32_t ngroups,
                       int64_t tail_n, float* out_full, const void* fin_partials, int32_t fin_np, double* fin_dev,
                       void* stream) {
  return launch_cg_end_active(x, p, num_dev, den_dev, lo, pos_dev, n_active, P, widths, ngroups, tail_n, out_full,
                              (const double*)fin_partials, fin_np, fin_dev, (hipStream_t)stream);
}

// the active list's workspace: the flags / their scan [P], the scan's block sums, its total
static size_t active_work_layout(int64_t P, void* base, uint32_t** flags, uint32_t** tmp, uint32_t** total) {
  Carver c{(char*)base};
  uint32_t* f = c.take<uint32_t>(P > 0 ? P : 1);
  uint32_t* t = c.take<uint32_t>(scan_tmp_bytes(P > 0 ? P : 1) / 4);
  uint32_t* n = c.take<uint32_t>(4);
  if (flags) { *flags = f; *tmp = t; *total = n; }
  return c.off;
}

size_t gslm_active_list_bytes(int64_t P) { return active_work_layout(P, nullptr, nullptr, nullptr, nullptr); }

int gslm_active_list(const void* geom, int64_t P, int64_t N, const void* scratch, size_t scratch_bytes, void* work,
                     size_t work_bytes, int32_t* ids_dev, uint32_t* rows_dev, int64_t* count_dev, void* stream) {
  if (P < 0 || N < 0 || !geom || !scratch || !work || !count_dev || !rows_dev || (P > 0 && !ids_dev)) {
    set_error("active_list: NULL workspace / output or negative size");
    return GSLM_ERR_INVALID;
  }
  if (scratch_bytes < gslm_scratch_bytes(P, N) || work_bytes < gslm_active_list_bytes(P)) {
    set_error("active_list: scratch or work workspace too small");
    return GSLM_ERR_CAPACITY;
  }
  GeomBufs gb;
  ScratchBufs sb;
  geom_layout(P, const_cast<void*>(geom), &gb);
  scratch_layout(P, N, const_cast<void*>(scratch), &sb);
  uint32_t *flags, *tmp, *total;
  active_work_layout(P, work, &flags, &tmp, &total);
  return launch_active_list(P, N, gb, sb, flags, tmp, total, ids_dev, rows_dev, count_dev, (hipStream_t)stream);
}

size_t gslm_active_union_bytes(int64_t P) { return active_work_layout(P, nullptr, nullptr, nullptr, nullptr); }

int gslm_active_union(const gslm_view_ws* ws, int32_t nviews, int64_t P, void* work, size_t work_bytes, int32_t* ids_dev,
                      uint32_t* hrow_dev, uint32_t* aflags_dev, int64_t* count_dev, void* stream) {
  if (!ws || nviews < 1 || P < 0 || P > MAX_P || !work || !count_dev || !hrow_dev || (P > 0 && (!ids_dev || !aflags_dev))) {
    set_error("active_union: NULL argument, nviews below 1 or P out of range");
    return GSLM_ERR_INVALID;
  }
  for (int b = 0; b < nviews; ++b)
    if (ws[b].num_rendered < 0 || (ws[b].num_rendered > 0 && P > 0 && (!ws[b].geom || !ws[b].scratch))) {
      set_error("active_union: negative num_rendered or a NULL workspace of a view that rendered");
      return GSLM_ERR_INVALID;
    }
  if (work_bytes < gslm_active_union_bytes(P)) {
    set_error("active_union: work area below gslm_active_union_bytes(P)");
    return GSLM_ERR_CAPACITY;
  }
  for (int b = 0; b < nviews; ++b)
    if (ws[b].num_rendered > 0 && ws[b].scratch_bytes < gslm_scratch_bytes(P, ws[b].num_rendered)) {
      set_error("active_union: scratch workspace too small");
      return GSLM_ERR_CAPACITY;
    }
  std::vector<GeomBufs> gbs(nviews);
  std::vector<ScratchBufs> sbs(nviews);
  std::vector<int64_t> nr(nviews);
  for (int b = 0; b < nviews; ++b) {
    nr[b] = ws[b].num_rendered;
    if (nr[b] == 0) continue;  // nothing rendered: no row map exists, the workspaces are not read
    geom_layout(P, const_cast<void*>(ws[b].geom), &gbs[b]);
    scratch_layout(P, nr[b], const_cast<void*>(ws[b].scratch), &sbs[b]);
  }
  uint32_t *flags, *tmp, *total;
  active_work_layout(P, work, &flags, &tmp, &total);
  return launch_active_union(gbs.data(), sbs.data(), nr.data(), nviews, P, flags, tmp, total, ids_dev, hrow_dev,
                             aflags_dev, count_dev, (hipStream_t)stream);
}

int gslm_inspect_rowmap(const void* geom, int64_t P, int64_t N, const void* scratch, size_t scratch_bytes,
                        uint32_t* goff, uint32_t* hscan, void* stream) {
  if (P < 0 || N < 0 || !geom || !scratch) { set_error("inspect_rowmap: NULL workspace or negative size"); return GSLM_ERR_INVALID; }
  if (scratch_bytes < gslm_scratch_bytes(P, N)) { set_error("inspect_rowmap: scratch workspace too small"); return GSLM_ERR_CAPACITY; }
  GeomBufs gb;
  ScratchBufs sb;
  geom_layout(P, const_cast<void*>(geom), &gb);
  scratch_layout(P, N, const_cast<void*>(scratch), &sb);
  hipStream_t s = (hipStream_t)stream;
  if (goff && P > 0) GSLM_HIP_CHECK(hipMemcpyAsync(goff, gb.goff, (size_t)P * 4, hipMemcpyDeviceToDevice, s));
  if (hscan) GSLM_HIP_CHECK(hipMemcpyAsync(hscan, sb.hscan, (size_t)(N + 1) * 4, hipMemcpyDeviceToDevice, s));
  return GSLM_OK;
}

int gslm_inspect_list(const void* binning, size_t binning_bytes, int64_t N, int32_t H, int32_t W, uint32_t* words,
                      uint32_t* slots, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || !binning) { set_error("inspect_list: NULL binning, negative count or empty image"); return GSLM_ERR_INVALID; }
  if (binning_bytes < gslm_binning_bytes(N, H, W)) { set_error("inspect_list: binning workspace too small"); return GSLM_ERR_CAPACITY; }
  BinBufs bb;
  bin_layout(N, ((W + TILE_X - 1) / TILE_X) * ((H + TILE_Y - 1) / TILE_Y), const_cast<void*>(binning), &bb);
  hipStream_t s = (hipStream_t)stream;
  if (words && N > 0) GSLM_HIP_CHECK(hipMemcpyAsync(words, bb.point_list, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
  if (slots && N > 0) GSLM_HIP_CHECK(hipMemcpyAsync(slots, bb.slots, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
  return GSLM_OK;
}

int gslm_active_pack(const float* src, float* dst, const int32_t* active_ids, int64_t n_active, int64_t P,
                     const int32_t* widths, int32_t ngroups, int64_t tail_n, void* stream) {
  return launch_active_pack(true, src, dst, active_ids, n_active, P, widths, ngroups, tail_n, (hipStream_t)stream);
}

int gslm_active_unpack(const float* src, float* dst, const int32_t* active_ids, int64_t n_active, int64_t P,
                       const int32_t* widths, int32_t ngroups, int64_t tail_n, void* stream) {
  return launch_active_pack(false, src, dst, active_ids, n_active, P, widths, ngroups, tail_n, (hipStream_t)stream);
}

int gslm_sh_rest_project(const gslm_view* view, const gslm_gaussians* gi, int32_t mode, const float* in,
                         int64_t in_stride, float* out, int64_t out_stride, void* stream) {
  ViewK v;
  GaussK g;
  int st;
  if (!view || !gi) { set_error("sh_rest_project: NULL view / gaussians"); return GSLM_ERR_INVALID; }
  if ((st = make_view(view, gi->max_coeffs, &v))) return st;
  if ((st = make_gauss(gi, &v, &g, false))) return st;
  if (mode != 0 && mode != 1) { set_error("sh_rest_project: mode must be 0 (expand) or 1 (project)"); return GSLM_ERR_INVALID; }
  if (g.P > 0 && g.M > 1 && (!in || !out || !g.means3D)) { set_error("sh_rest_project: NULL buffer"); return GSLM_ERR_INVALID; }
  const int64_t full = 3 * (int64_t)(g.M - 1);
  if ((mode == 0 && (in_stride < 3 || out_stride < full)) || (mode == 1 && (in_stride < full || out_stride < 3))) {
    set_error("sh_rest_project: strides too small for [P,3] / [P,M-1,3] rows");
    return GSLM_ERR_INVALID;
  }
  return launch_sh_rest_project(v, g, mode, in, in_stride, out, out_stride, (hipStream_t)stream);
}

// the views of one SH-rest coordinate system: 1..GSLM_MAX_REST_VIEWS, one SH degree
static int rest_views(const char* who, const gslm_view* views, int32_t nviews, const gslm_gaussians* gi, ViewK* vk,
                      GaussK* g) {
  if (!views || !gi || nviews < 1 || nviews > GSLM_MAX_REST_VIEWS) {
    set_error(std::string(who) + ": NULL views / gaussians or nviews outside 1..GSLM_MAX_REST_VIEWS");
    return GSLM_ERR_INVALID;
  }
  int st;
  for (int b = 0; b < nviews; ++b) {
    if ((st = make_view(&views[b], gi->max_coeffs, &vk[b]))) return st;
    if (vk[b].D != vk[0].D) {
      set_error(std::string(who) + ": the views must share one SH degree");
      return GSLM_ERR_INVALID;
    }
  }
  if ((st = make_gauss(gi, &vk[0], g, false))) return st;
  if (g->P > 0 && !g->means3D) {
    set_error(std::string(who) + ": NULL means3D");
    return GSLM_ERR_INVALID;
  }
  return GSLM_OK;
}

int gslm_rest_basis(const gslm_view* views, int32_t nviews, const gslm_gaussians* gi, float* R_out, void* stream) {
  ViewK vk[GSLM_MAX_REST_VIEWS];
  GaussK g;
  int st;
  if ((st = rest_views("rest_basis", views, nviews, gi, vk, &g))) return st;
  if (g.P > 0 && !R_out) { set_error("rest_basis: NULL R_out"); return GSLM_ERR_INVALID; }
  return launch_rest_basis(vk, nviews, g, R_out, (hipStream_t)stream);
}

int gslm_rest_coords(const gslm_view* views, int32_t nviews, const gslm_gaussians* gi, const float* R, int32_t mode,
                     const float* in, int64_t in_stride, float* out, int64_t out_stride, void* stream) {
  ViewK vk[GSLM_MAX_REST_VIEWS];
  GaussK g;
  int st;
  if ((st = rest_views("rest_coords", views, nviews, gi, vk, &g))) return st;
  if (mode != 0 && mode != 1) { set_error("rest_coords: mode must be 0 (expand) or 1 (project)"); return GSLM_ERR_INVALID; }
  if (g.M < 2) return GSLM_OK;
  if (g.P > 0 && (!R || !in || !out)) { set_error("rest_coords: NULL buffer"); return GSLM_ERR_INVALID; }
  const int64_t full = 3 * (int64_t)(g.M - 1), coords = 3 * (int64_t)nviews;
  if ((mode == 0 && (in_stride < coords || out_stride < full)) || (mode == 1 && (in_stride < full || out_stride < coords))) {
    set_error("rest_coords: strides too small for [P,V,3] / [P,M-1,3] rows");
    return GSLM_ERR_INVALID;
  }
  return launch_rest_coords(vk, nviews, g, R, mode, in, in_stride, out, out_stride, (hipStream_t)stream);
}

// opts->rest_basis of gslm_tangent_views / gslm_gather_screen: the coordinate system and this call's columns
static int rest_opts(const char* who, int32_t nviews, Plan* pl) {
  const gslm_matvec_opts* opts = pl->o;
  if (!(pl->f & F_REST_BASIS)) return GSLM_OK;
  if (opts->rest_views < 1 || opts->rest_views > GSLM_MAX_REST_VIEWS || opts->view_base < 0 ||
      opts->view_base + nviews > opts->rest_views) {
    set_error(std::string(who) + ": rest_views outside 1..GSLM_MAX_REST_VIEWS or views past its last column");
    return GSLM_ERR_INVALID;
  }
  pl->rc.R = opts->rest_basis;
  pl->rc.V = opts->rest_views;
  pl->rc.view_base = opts->view_base;
  return GSLM_OK;
}

// The views of a multi-view product call, each with the solve's stop flag (a stopped solve's kernels return at once),
// and the Gaussians, which must be the raw leaves (sh_only: with SH colours and no cov3D)
static int bind_views(const char* who, const gslm_view* views, int32_t nviews, const gslm_gaussians* gi,
                      const Plan& pl, bool sh_only, ViewK* vk, GaussK* g) {
  int st;
  for (int b = 0; b < nviews; ++b) {
    if ((st = make_view(&views[b], gi->max_coeffs, &vk[b]))) return st;
    vk[b].stop = pl.stop;
  }
  if ((st = make_gauss(gi, &vk[0], g, false))) return st;
  if (!g->raw || (sh_only && (g->cov3D || g->colors))) {
    set_error(std::string(who) + ": gaussians must be the raw GaussianModel leaves (raw = 1)");
    return GSLM_ERR_INVALID;
  }
  return GSLM_OK;
}

int gslm_gather_screen(const gslm_view* views, int32_t nviews, const gslm_gaussians* gi, const float* screen,
                       const gslm_grads* vin, const gslm_grads* y, const gslm_matvec_opts* opts, void* stream) {
  if (!views || nviews < 1 || nviews > 16 || !gi || !screen || !vin || !y) {
    set_error("gather_screen: NULL argument or nviews outside 1..16");
    return GSLM_ERR_INVALID;
  }
  Plan pl;
  plan_base(E_GATHER_SCREEN, F_DAMP_VEC | F_DAMP7 | F_REST_BASIS | F_DEPTH | F_XYZ, opts, true, 0, &pl);
  if (excluded(pl.f, F_XYZ) || excluded(pl.f, E_GATHER) || excluded(pl.f, F_DEPTH)) return GSLM_ERR_INVALID;
  ViewK vk[16];
  GaussK g;
  int st;
  if ((st = bind_views("gather_screen", views, nviews, gi, pl, false, vk, &g))) return st;
  if ((st = plan_dot("gather_screen", g.P, false, &pl))) return st;
  const int64_t sstride = (opts && opts->screen_stride) ? opts->screen_stride : g.P;
  if (sstride < g.P) { set_error("gather_screen: screen_stride below P"); return GSLM_ERR_INVALID; }
  if ((st = rest_opts("gather_screen", nviews, &pl))) return st;
  if (g.P > 0 && (st = plan_flat(g, y, vin, &pl))) return st;
  if ((st = launch_gather_screen(vk, nviews, g, screen, sstride, pl.flat, (hipStream_t)stream, pl.rc))) return st;
  if (pl.dot_out) return gslm_dot_finalize(pl.part, (int32_t)((g.P + 255) / 256), pl.dot_out, stream);
  return GSLM_OK;
}

// gslm_gather_views (na < 0) and gslm_gather_views_active (na >= 0: the groups of vin and y hold the na Gaussians
// ids[0 .. na) of the batch's union list only)
static int gather_views(const gslm_view* views, const gslm_view_ws* ws, int32_t nviews, const gslm_gaussians* gi,
                        const gslm_grads* vin, const gslm_grads* y, const gslm_matvec_opts* opts, const int32_t* ids,
                        int64_t na, const uint32_t* hrow, int64_t hstride, const uint32_t* aflags, int64_t fstride,
                        void* stream) {
  const bool active = na >= 0;
  if (!views || !ws || nviews < 1 || nviews > MAX_SCREEN_VIEWS || !gi || !vin || !y) {
    set_error("gather_views: NULL argument or nviews outside 1..16");
    return GSLM_ERR_INVALID;
  }
  Plan pl;
  // (GSLM_MV_EXPOSURE is decoded for GSLM_MV_XYZ's refusal alone: without that flag it is ignored as ever)
  plan_base(E_GATHER_VIEWS | (active ? F_LIST : 0), F_DAMP_VEC | F_DAMP7 | F_REST_BASIS | F_DEPTH | F_XYZ | F_EXPOSURE,
            opts, true, 0, &pl);
  if (excluded(pl.f, F_XYZ) || excluded(pl.f, E_GATHER) || excluded(pl.f, F_DEPTH)) return GSLM_ERR_INVALID;
  if (active && (na > gi->P || !hrow || hstride < na + 1 || fstride < na || (na > 0 && (!ids || !aflags)))) {
    set_error("gather_views_active: n_active above P, a NULL list or a stride that does not hold it");
    return GSLM_ERR_INVALID;
  }
  ViewK vk[MAX_SCREEN_VIEWS];
  GeomBufs gbs[MAX_SCREEN_VIEWS];
  ScratchBufs sbs[MAX_SCREEN_VIEWS];
  int64_t nr[MAX_SCREEN_VIEWS];
  GaussK g;
  int st;
  if ((st = bind_views("gather_views", views, nviews, gi, pl, false, vk, &g))) return st;
  for (int b = 0; b < nviews; ++b) {
    nr[b] = ws[b].num_rendered;
    if (nr[b] < 0 || (nr[b] > 0 && g.P > 0 && (!ws[b].geom || !ws[b].scratch))) {
      set_error("gather_views: negative num_rendered or a NULL workspace of a view that rendered");
      return GSLM_ERR_INVALID;
    }
    if (nr[b] == 0) continue;  // nothing rendered: no row map exists, the workspaces are not read
    if (ws[b].scratch_bytes < gslm_scratch_bytes(g.P, nr[b])) {
      set_error("gather_views: scratch workspace too small");
      return GSLM_ERR_CAPACITY;
    }
    geom_layout(g.P, const_cast<void*>(ws[b].geom), &gbs[b]);
    scratch_layout(g.P, nr[b], const_cast<void*>(ws[b].scratch), &sbs[b]);
  }
  pl.rows = active ? na : g.P;
  if ((st = plan_dot("gather_views", pl.rows, false, &pl))) return st;
  if ((st = rest_opts("gather_views", nviews, &pl))) return st;
  if (pl.rows > 0 && (st = plan_flat(g, y, vin, &pl))) return st;
  pl.flat.dot_part = pl.part;  // (an empty call still finishes its dot: the sum of no partials)
  return launch_gather_views(vk, gbs, sbs, nr, nviews, g, pl.flat, pl.dot_out, (hipStream_t)stream, pl.rc, ids,
                             active ? na : -1, hrow, hstride, aflags, fstride, (pl.f & F_XYZ) != 0);
}

int gslm_gather_views(const gslm_view* views, const gslm_view_ws* ws, int32_t nviews, const gslm_gaussians* gi,
                      const gslm_grads* vin, const gslm_grads* y, const gslm_matvec_opts* opts, void* stream) {
  return gather_views(views, ws, nviews, gi, vin, y, opts, nullptr, -1, nullptr, 0, nullptr, 0, stream);
}

int gslm_gather_views_active(const gslm_view* views, const gslm_view_ws* ws, int32_t nviews, const gslm_gaussians* gi,
                             const gslm_grads* vin, const gslm_grads* y, const int32_t* active_ids, int64_t n_active,
                             const uint32_t* hrow, int64_t hrow_stride, const uint32_t* aflags, int64_t flags_stride,
                             const gslm_matvec_opts* opts, void* stream) {
  if (n_active < 0) { set_error("gather_views_active: negative n_active"); return GSLM_ERR_INVALID; }
  return gather_views(views, ws, nviews, gi, vin, y, opts, active_ids, n_active, hrow, hrow_stride, aflags,
                      flags_stride, stream);
}

int gslm_view_flags(const void* geom, int64_t P, uint32_t* out, void* stream) {
  if (P < 0 || (P > 0 && (!geom || !out))) { set_error("view_flags: NULL geom / out"); return GSLM_ERR_INVALID; }
  GeomBufs gb;
  geom_layout(P, const_cast<void*>(geom), &gb);
  return launch_view_flags(P, gb, out, (hipStream_t)stream);
}

// gslm_tangent_views (na < 0) and gslm_tangent_views_active (na >= 0: the groups of vin and of the fused direction
// update, and the rows of vflags, hold the na Gaussians ids[0 .. na) of the batch's union list only)
static int tangent_views(const gslm_view* views, int32_t nviews, const gslm_gaussians* gi, const gslm_grads* vin,
                         int32_t mask_xyz, const uint32_t* vflags, int64_t flags_stride, float* trec_out,
                         int64_t trec_stride, const gslm_matvec_opts* opts, const int32_t* ids, int64_t na,
                         void* stream) {
  const bool active = na >= 0;
  if (!views || nviews < 1 || nviews > MAX_SCREEN_VIEWS || !gi || !vin) {
    set_error("tangent_views: NULL argument or nviews outside 1..16");
    return GSLM_ERR_INVALID;
  }
  if (active && (!mask_xyz || na > gi->P || (na > 0 && !ids))) {
    set_error("tangent_views_active: the LM rows (mask_xyz) and a list of at most P Gaussians");
    return GSLM_ERR_INVALID;
  }
  Plan pl;
  plan_base(E_TANGENT_VIEWS | (active ? F_LIST : 0), F_XPBY | F_REST_BASIS | F_DEPTH | F_XYZ, opts, mask_xyz != 0, 0, &pl);
  if (excluded(pl.f, F_XYZ) || excluded(pl.f, F_DEPTH)) return GSLM_ERR_INVALID;
  ViewK vk[MAX_SCREEN_VIEWS];
  GaussK g;
  int st;
  if ((st = bind_views("tangent_views", views, nviews, gi, pl, true, vk, &g))) return st;
  if (g.P > 0 && (!vflags || !trec_out || flags_stride < (active ? na : g.P) || trec_stride < g.P)) {
    set_error("tangent_views: NULL vflags / trec_out or a stride below P");
    return GSLM_ERR_INVALID;
  }
  GaussK t = tangent_from_grads(vin, g, mask_xyz != 0);
  if ((st = rest_opts("tangent_views", nviews, &pl))) return st;
  const RestK& rc = pl.rc;
  const int R = rc.R ? 3 * rc.V : 3 * (g.M - 1);
  if (t.rest && t.rest_stride != R) {
    set_error(rc.R ? "tangent_views: SH-rest coordinates need stride 3 rest_views"
                   : "tangent_views: the SH-rest tangent needs stride 3(M-1)");
    return GSLM_ERR_INVALID;
  }
  if (rc.R && g.M > 1) {
    t.rest_R = rc.R;
    t.rest_V = rc.V;
  }
  const bool fused = (pl.f & F_XPBY) != 0;
  if (fused && (st = build_xpby(opts, vin, R, mask_xyz != 0, &pl.xp))) return st;
  return launch_tangent_views(vk, nviews, g, t, vflags, flags_stride, trec_out, trec_stride, fused ? &pl.xp : nullptr,
                              (hipStream_t)stream, mask_xyz != 0, rc.view_base, ids, active ? na : -1);
}

int gslm_tangent_views(const gslm_view* views, int32_t nviews, const gslm_gaussians* gi, const gslm_grads* vin,
                       int32_t mask_xyz, const uint32_t* vflags, int64_t flags_stride, float* trec_out,
                       int64_t trec_stride, const gslm_matvec_opts* opts, void* stream) {
  return tangent_views(views, nviews, gi, vin, mask_xyz, vflags, flags_stride, trec_out, trec_stride, opts, nullptr, -1,
                       stream);
}

int gslm_tangent_views_active(const gslm_view* views, int32_t nviews, const gslm_gaussians* gi, const gslm_grads* vin,
                              int32_t mask_xyz, const int32_t* active_ids, int64_t n_active, const uint32_t* aflags,
                              int64_t flags_stride, float* trec_out, int64_t trec_stride, const gslm_matvec_opts* opts,
                              void* stream) {
  if (n_active < 0) { set_error("tangent_views_active: negative n_active"); return GSLM_ERR_INVALID; }
  return tangent_views(views, nviews, gi, vin, mask_xyz, aflags, flags_stride, trec_out, trec_stride, opts, active_ids,
                       n_active, stream);
}

int gslm_matvec_view(const gslm_view* view, const gslm_gaussians* gi, const gslm_grads* vin,
                     const float* pixel_weight, int32_t mask_xyz, const void* geom, const void* binning, int64_t N,
                     const void* image, void* scratch, size_t scratch_bytes, const gslm_grads* y, void* stream) {
  return gslm_matvec_view_ex(view, gi, vin, pixel_weight, mask_xyz, geom, binning, N, image, scratch, scratch_bytes,
                             y, nullptr, stream);
}

int gslm_inspect(const void* geom, int64_t P, const void* binning, int64_t N, int32_t H, int32_t W,
                 const void* image, uint32_t* point_list, uint32_t* ranges, uint32_t* tiles_touched, float* final_T,
                 uint32_t* n_contrib, float* records, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  GeomBufs gb;
  BinBufs bb;
  ImgBufs ib;
  const int ntiles = ((W + TILE_X - 1) / TILE_X) * ((H + TILE_Y - 1) / TILE_Y);
  geom_layout(P, const_cast<void*>(geom), &gb);
  bin_layout(N, ntiles, const_cast<void*>(binning), &bb);
  img_layout(H, W, const_cast<void*>(image), &ib);
  const auto D2D = hipMemcpyDeviceToDevice;
  if (point_list && N) {
    const int st = launch_point_ids(bb.point_list, N, point_list, s);
    if (st) return st;
  }
  if (ranges && binning) GSLM_HIP_CHECK(hipMemcpyAsync(ranges, bb.ranges, (size_t)ntiles * 8, D2D, s));
  if (tiles_touched && P) GSLM_HIP_CHECK(hipMemcpyAsync(tiles_touched, gb.tiles, (size_t)P * 4, D2D, s));
  if (final_T && image) GSLM_HIP_CHECK(hipMemcpyAsync(final_T, ib.final_T, (size_t)H * W * 4, D2D, s));
  if (n_contrib && image) GSLM_HIP_CHECK(hipMemcpyAsync(n_contrib, ib.n_contrib, (size_t)H * W * 4, D2D, s));
  if (records && P)  // 12 floats per Gaussian out of the 64-B record stride
    GSLM_HIP_CHECK(hipMemcpy2DAsync(records, 48, gb.rec, RECS * sizeof(float4), 48, (size_t)P, D2D, s));
  return GSLM_OK;
}

}  // extern "C"
