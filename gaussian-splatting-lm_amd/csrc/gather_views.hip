// gather_views.hip -- the per-Gaussian side of the single-process multi-view LM product (gslm_gather_views,
// gslm.lm.BatchedLMProblem): one pass over the Gaussians sums every view's head rows and applies every view's
// chain, where the per-view loop runs one k_gather_lm per view (each re-reading and re-writing the whole y) and
// the exchange's form runs one k_rowsum_screen per view into a [P][8] table that k_gather_screen reads back.
//   y = [y +] [D v +] sum_b C_b^T (sum of Gaussian i's head rows in view b),   <v, y> partials
// Same row sums (block_sum_rows<2> over the same 256-Gaussian partition), same chain and the same accumulation
// order as k_rowsum_screen x V + k_gather_screen, so the results are those kernels' bit for bit.
// XYZ (GSLM_MV_XYZ): the views' head rows are the 48-byte ones of an unmasked RENDER stage (block_sum_rows<3>), the
// chain includes the means (with the SH colour's view-direction term) and y's xyz group is written with the others.
#include <type_traits>
#include "gslm_gather.hpp"

namespace gslm {

// Every view's geometry workspace has the layout of the same P (geom_layout), so goff and clampw lie at one
// offset from tiles in all of them; a view's hscan lies hoff float4 past its rows (scratch_layout).  rows NULL:
// the view rendered nothing (no row map exists), it is skipped.
struct ViewWsK {
  const uint32_t* tiles[MAX_SCREEN_VIEWS];
  const float4* rows[MAX_SCREEN_VIEWS];
  uint32_t hoff[MAX_SCREEN_VIEWS];
  int32_t goff_off, clamp_off;  // in words, from tiles
};
// ACTIVE's workspace argument instead: the views' rows (NULL as above) and the union list of the batch
// (gslm_active_union).  v and y hold the na listed Gaussians, entry j's head rows in view b are
// [hrow[b hstride + j], hrow[b hstride + j + 1]) and aflags[b fstride + j] is that view's gslm_view_flags word of
// Gaussian ids[j].
struct ActiveWsK {
  const float4* rows[MAX_SCREEN_VIEWS];
  const int32_t* ids;
  const uint32_t* hrow;
  const uint32_t* aflags;
  int64_t na, hstride, fstride;
};
static_assert(sizeof(ActiveWsK) <= sizeof(ViewWsK), "k_gather_views<., ACTIVE>: no more kernel arguments than the full one");
static_assert(sizeof(ViewsK) + sizeof(ViewWsK) + sizeof(GaussK) + sizeof(FlatK) + sizeof(RestK) <= 4096,
              "k_gather_views: kernel arguments past 4 KB");

template <bool ACTIVE, typename WS>
__device__ __forceinline__ int64_t nrows_of(const WS& ws, const GaussK& g) {
  if constexpr (ACTIVE) return ws.na;
  else return g.P;
}

// ACTIVE (gslm_gather_views_active): thread j handles Gaussian ids[j] of the scene (parameters, the factor R) and row
// j of v, y, hrow and aflags.  A block's 256 consecutive listed Gaussians still own one contiguous range of head rows
// in every view -- the Gaussians between two listed ones own none in any view -- so the row sums and their order are
// the full kernel's (k_gather_lm<..., ACTIVE> for one view); the view's tiles, goff, hscan and clampw are not read.
template <bool COORDS, bool ACTIVE = false, bool XYZ = false>
__global__ __launch_bounds__(256) void k_gather_views(ViewsK vs, std::conditional_t<ACTIVE, ActiveWsK, ViewWsK> ws,
                                                       GaussK g, FlatK o, RestK rc) {
  static_assert(!(ACTIVE && XYZ), "k_gather_views: the union list's rows are the masked ones");
  constexpr int ROWF4 = XYZ ? 3 : 2;  // float4 per head row
  extern __shared__ __attribute__((aligned(16))) float s_rest[];  // the views' row chunks, then the epilogue's stage
  __shared__ double s_dot[4];
  if (cg_stopped(vs.v[0])) return;  // a stopped solve (gslm_matvec_opts.cg_ctl): block-uniform, before any barrier
  if constexpr (XYZ) {
    // raw leaves with SH colours (make_flatk has refused anything else): as compile-time facts they drop the
    // chain's other branches, which with the means' terms would not fit the scalar registers
    g.cov3D = nullptr;
    g.colors = nullptr;
  }
  const int64_t nrows = nrows_of<ACTIVE>(ws, g);  // rows of v and y
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x;
  const int64_t j = i0 + threadIdx.x;
  const int64_t nvalid = min((int64_t)blockDim.x, nrows - i0);
  const int64_t il = i0 + nvalid - 1;  // the block's last Gaussian
  const bool valid = j < nrows;
  int64_t i = j;
  if constexpr (ACTIVE) i = valid ? (int64_t)ws.ids[j] : 0;
  ChainOut acc;
  acc.dop = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) { acc.dscale[k] = 0.f; acc.dmean[k] = 0.f; }
#pragma unroll
  for (int k = 0; k < 4; ++k) acc.drot[k] = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) acc.dsh[k][0] = acc.dsh[k][1] = acc.dsh[k][2] = 0.f;
#pragma unroll 1
  for (int b = 0; b < vs.n; ++b) {
    const float4* __restrict__ rows = ws.rows[b];
    if (!rows) continue;  // an empty view: a kernel argument, so the whole block skips it (no barrier is missed)
    float G2[NV];
    uint32_t clamp;
    if constexpr (ACTIVE) {
      // the list's own row offsets and flag words, read coalesced; every thread runs the row sums (they hold
      // barriers), also past na and for a listed Gaussian this view does not move (an empty range)
      const uint32_t* __restrict__ hrow = ws.hrow + (int64_t)b * ws.hstride;
      const uint32_t f = valid ? ws.aflags[(int64_t)b * ws.fstride + j] : 0u;
      const uint32_t R0 = hrow[i0], R1 = hrow[i0 + nvalid];
      const uint32_t h0 = valid ? hrow[j] : R1, h1 = valid ? hrow[j + 1] : R1;
      block_sum_rows<2>(rows, R0, R1, h0, h1 - h0, reinterpret_cast<float4*>(s_rest), G2);
      if (!(f >> 31)) continue;
      clamp = f & 7u;
    } else {
      const uint32_t* __restrict__ tiles = ws.tiles[b];
      const uint32_t* __restrict__ goff = tiles + ws.goff_off;
      const uint32_t* __restrict__ hscan = reinterpret_cast<const uint32_t*>(rows + ws.hoff[b]);
      // the block's contiguous head-row range of this view and this Gaussian's part of it (k_rowsum_screen); every
      // thread runs the row sums -- they hold barriers -- also past P and for a Gaussian the view does not see
      const uint32_t n = i < g.P ? tiles[i] : 0u;
      const uint32_t R0 = hscan[goff[i0]], R1 = hscan[goff[il] + tiles[il]];
      const uint32_t h0 = i < g.P ? hscan[goff[i]] : R1, h1 = i < g.P ? hscan[goff[i] + n] : R1;
      block_sum_rows<ROWF4>(rows, R0, R1, h0, h1 - h0, reinterpret_cast<float4*>(s_rest), G2);
      if (!n) continue;
      clamp = (tiles + ws.clamp_off)[i] & 7u;
    }
    ChainOut co;
    chain_vjp<true>(vs.v[b], g, i, true, clamp, G2, /*want_means=*/XYZ, co);
    acc.dop += co.dop;
    if constexpr (XYZ) {
#pragma unroll
      for (int k = 0; k < 3; ++k) acc.dmean[k] += co.dmean[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) acc.dscale[k] += co.dscale[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc.drot[k] += co.drot[k];
    if constexpr (COORDS) {
      // SH-rest coordinates (k_gather_screen<true>): view b is column view_base + b of R
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc.dsh[0][ch] += co.dsh[0][ch];
      const int col = rc.view_base + b;
      const float* Rc = rc.R + i * rest_basis_floats(rc.V) + rest_basis_floats(col);
#pragma unroll
      for (int q = 0; q < MAX_REST_VIEWS; ++q)
        if (q <= col) {
          const float r = Rc[q];
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) acc.dsh[1 + q][ch] += r * co.dres[ch];
        }
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        acc.dsh[k][0] += co.dsh[k][0];
        acc.dsh[k][1] += co.dsh[k][1];
        acc.dsh[k][2] += co.dsh[k][2];
      }
    }
  }
  if constexpr (ACTIVE) g.P = ws.na;  // the epilogue writes rows j < na of y (it reads P and M of g only)
  lm_epilogue<XYZ>(g.M, g, acc, o, s_rest, s_dot);
}

// <v, y> from the blocks' partials: k_dot_final's sum (cg.hip), except that a stopped solve -- whose gather wrote no
// partials -- leaves the dot as it is
__global__ __launch_bounds__(256) void k_dot_final_views(const double* __restrict__ part, int np,
                                                         double* __restrict__ out, const double* __restrict__ ctl) {
  __shared__ double s[4];
  if (ctl != nullptr && *ctl != 0.0) return;
  double x = strided_sum_in_order(part, np);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  if (lane == 0) s[w] = x;
  __syncthreads();
  if (tid == 0) *out = ((s[0] + s[1]) + s[2]) + s[3];
}

int launch_gather_views(const ViewK* views, const GeomBufs* gbs, const ScratchBufs* sbs, const int64_t* nr,
                        int nviews, const GaussK& g, const FlatK& o, double* dot_out, hipStream_t s, const RestK& rc,
                        const int32_t* ids, int64_t na, const uint32_t* hrow, int64_t hstride, const uint32_t* aflags,
                        int64_t fstride, bool xyz) {
  double* const dot_part = o.dot_part;
  const bool active = na >= 0;
  const int64_t nrows = active ? na : g.P;  // rows of v and y
  if (nrows == 0) {
    if (dot_out) {  // an empty sum
      hipLaunchKernelGGL(k_dot_final_views, dim3(1), dim3(256), 0, s, dot_part, 0, dot_out, views[0].stop);
      GSLM_LAUNCH_CHECK();
    }
    return GSLM_OK;
  }
  // guards of this launcher's own contract: gather_views (api.hip) has checked both, so neither is reachable from
  // the C ABI
  if (nviews < 1 || nviews > MAX_SCREEN_VIEWS) {
    set_error("gather_views: 1..16 views per call");
    return GSLM_ERR_INVALID;
  }
  if (active && (!ids || !hrow || !aflags || hstride < na + 1 || fstride < na)) {
    set_error("internal: the active-list gather needs the union list and strides that hold it");
    return GSLM_ERR_INVALID;
  }
  if (active && xyz) {
    set_error("internal: the active-list gather runs on the LM rows (no GSLM_MV_XYZ)");
    return GSLM_ERR_INVALID;
  }
  ViewsK vs;
  ViewWsK ws{};
  vs.n = nviews;
  for (int b = 0; b < nviews; ++b) {
    vs.v[b] = views[b];
    if (nr[b] <= 0) continue;  // rows stays NULL: skipped
    // (the geometry layout depends on P only: any view's offsets are every view's)
    ws.goff_off = (int32_t)(gbs[b].goff - gbs[b].tiles);
    ws.clamp_off = (int32_t)(gbs[b].clampw - gbs[b].tiles);
    const size_t hbytes = (size_t)(reinterpret_cast<const char*>(sbs[b].hscan) -
                                   reinterpret_cast<const char*>(sbs[b].contrib));
    if (hbytes % sizeof(float4) != 0 || hbytes / sizeof(float4) > 0xFFFFFFFFull) {
      set_error("gather_views: num_rendered too large for the row map offset");
      return GSLM_ERR_INVALID;
    }
    ws.tiles[b] = gbs[b].tiles;
    ws.rows[b] = sbs[b].contrib;
    ws.hoff[b] = (uint32_t)(hbytes / sizeof(float4));
  }
  ActiveWsK aw{};
  for (int b = 0; b < nviews; ++b) aw.rows[b] = ws.rows[b];
  aw.ids = ids;
  aw.hrow = hrow;
  aw.aflags = aflags;
  aw.na = na;
  aw.hstride = hstride;
  aw.fstride = fstride;
  const unsigned nb = (unsigned)((nrows + 255) / 256);
  const size_t chunk_lds = (size_t)GATHER_CHUNK * (xyz ? 3 : 2) * sizeof(float4);
  const size_t stage = (o.rest_V ? (size_t)256 * 3 * o.rest_V : sh_stage_floats<false>(g.M)) * sizeof(float);
  const size_t lds = (stage > chunk_lds ? stage : chunk_lds) + 16;
  if (o.rest_V && xyz)
    hipLaunchKernelGGL((k_gather_views<true, false, true>), dim3(nb), dim3(256), lds, s, vs, ws, g, o, rc);
  else if (xyz)
    hipLaunchKernelGGL((k_gather_views<false, false, true>), dim3(nb), dim3(256), lds, s, vs, ws, g, o, rc);
  else if (o.rest_V && active)
    hipLaunchKernelGGL((k_gather_views<true, true>), dim3(nb), dim3(256), lds, s, vs, aw, g, o, rc);
  else if (o.rest_V)
    hipLaunchKernelGGL(k_gather_views<true>, dim3(nb), dim3(256), lds, s, vs, ws, g, o, rc);
  else if (active)
    hipLaunchKernelGGL((k_gather_views<false, true>), dim3(nb), dim3(256), lds, s, vs, aw, g, o, rc);
  else
    hipLaunchKernelGGL(k_gather_views<false>, dim3(nb), dim3(256), lds, s, vs, ws, g, o, rc);
  GSLM_LAUNCH_CHECK();
  if (dot_out) {
    hipLaunchKernelGGL(k_dot_final_views, dim3(1), dim3(256), 0, s, dot_part, (int)nb, dot_out, views[0].stop);
    GSLM_LAUNCH_CHECK();
  }
  return GSLM_OK;
}

}  // namespace gslm
