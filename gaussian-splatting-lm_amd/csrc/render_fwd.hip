// render_fwd.hip -- the rasterizer forward's per-tile blend (upstream renderCUDA semantics, SURVEY App. A
// step 11): one 16x16 tile per 256-thread block, wave w on the tile's 8x8 quadrant w (tile_pixel), each wave
// visiting only the list entries whose alpha region reaches its quadrant (the point list's quadrant masks),
// front to back until T < 1e-4.
//
// Compiled apart from the per-Gaussian kernels with -fno-slp-vectorize (Makefile), like the other tile
// passes: the loop body is scalar f32 math and one branch, the per-lane stop kept as a lane mask (the wave
// leaves when every lane has stopped), no software pipelining of the next records (measured: no gain).
#include "gslm_tile.hpp"

namespace gslm {

// One independent wave per 8x8 quadrant: 64 list positions per round, each lane fetches one, the entries whose
// mask holds the quadrant stage their record in the wave's own LDS slots (lane-indexed), and the wave walks the
// round's hit bits in list order.  No block barrier: a wave leaves as soon as all of its pixels have stopped,
// however far the tile's other quadrants still go (a block-cooperative version with 256-entry LDS batches
// measured 1.5% slower on the full forward).  The visit and the loss are gslm_tile.hpp's front-to-back parts.
// MODE (the epilogue): FWD_FULL colour + inverse depth + final_T / n_contrib (gslm_rasterize, the drop-in forward);
// FWD_NO_INV the same without the inverse depth (the LM paths); FWD_LOSS no image, the per-tile sum of the
// pixels' loss_term -> part[tile] (gslm_rasterize_loss, the LM line search's validation loss).
enum { FWD_FULL = 0, FWD_NO_INV = 1, FWD_LOSS = 2 };

// The switches of FWD_LOSS; none changes the blend loop, which is the same loop with the same registers.
// SLOT: the line search's union list (gslm_rasterize_loss_slot) -- an entry is visited by its set's bits of amask
// (k_slot_masks: the set's own quadrant mask, 0 outside the set's rect) instead of the point list's.
// EXPO: loss_term<true> through the camera's exposure map X (12 device floats, wave-uniform, read after the loop).
// ROBUST (never with EXPO): loss_term's robust form with the block rb.
// DEPTH (the plain loss only; gslm_rasterize_loss_depth and its slot form): the loop also accumulates the inverse depth
// Dp exactly as FWD_FULL does, and after the three colour terms, in their order, the pixel adds the depth block's term
// (gslm_lm_residual_depth's r, in its order): r = m_d (Dp - Dgt), dl.half_weight ((double) r (double) r) -- half the
// weight, since the final pass doubles every tile sum (the [r; r] aliasing, which the depth block does not have; the
// halving and the doubling are exact).
template <int MODE, bool SLOT = false, bool EXPO = false, bool ROBUST = false, bool DEPTH = false>
__global__ __launch_bounds__(256) void k_render_fwd_wave(ViewK v, const uint2* __restrict__ ranges,
                                                          const uint32_t* __restrict__ tile_order,
                                                          const uint32_t* __restrict__ point_list,
                                                          const float4* __restrict__ rec, float* __restrict__ out_color,
                                                          float* __restrict__ out_invdepth, float* __restrict__ final_T,
                                                          uint32_t* __restrict__ n_contrib, const float* __restrict__ gt,
                                                          const float* __restrict__ mask, double* __restrict__ part,
                                                          const uint32_t* __restrict__ amask, int shift,
                                                          const float* __restrict__ X, gslm_robust rb,
                                                          DepthLossK dl) {
  static_assert(!EXPO || MODE == FWD_LOSS, "the exposure map belongs to the loss epilogue");
  static_assert(!DEPTH || (MODE == FWD_LOSS && !EXPO && !ROBUST), "the depth term belongs to the plain loss epilogue");
  static_assert(!ROBUST || (MODE == FWD_LOSS && !EXPO), "the robust loss belongs to the plain loss epilogue");
  __shared__ float4 s_rec[4][3 * 64];
  const TilePix p = tile_pix(v, tile_order);
  const int tid = threadIdx.x, q = tid >> 6, lane = tid & 63;
  const float pxf = (float)p.px, pyf = (float)p.py;
  const uint2 range = ranges[p.tile];
  const int n = (int)(range.y - range.x);
  const uint32_t* pl = point_list + range.x;
  float4* s = s_rec[q];

  FwdPix st = fwd_pix(p.inside);
  uint32_t last = 0;
  float Dp = 0.f;
  uint64_t live = __builtin_amdgcn_ballot_w64(p.inside);  // lanes not yet stopped (inside the image), wave-uniform
  for (int base = 0; base < n; base += 64) {
    if (live == 0ull) break;  // every pixel of this quadrant has stopped
    const int k = base + lane;
    bool hit = false;
    if (k < n) {
      const uint32_t e = pl[k];
      if (((SLOT ? amask[range.x + k] >> shift : pl_mask(e)) >> q) & 1u) {
        hit = true;
        stage_hit(s, lane, load_rec(rec, pl_id(e)));
      }
    }
    uint64_t hb = __ballot(hit);
    wave_lds_sync();
    while (hb) {
      const int j = (int)__builtin_ctzll(hb);
      hb = clear_bit(hb, j);
      const HitRec h = load_hit<true>(s, j);
      float wt;
      const bool stop = fwd_visit(h, pxf, pyf, st, wt);
      if (MODE == FWD_FULL || DEPTH) Dp = __builtin_fmaf(h.c.y, wt, Dp);
      if (MODE != FWD_LOSS) last = wt > 0.0f ? (uint32_t)(base + j + 1) : last;  // blended: 1-based list position
      // the stop compare's lane mask (no VGPR round trip) leaves `live`; the round ends when no lane is
      live_update(live, hb, __builtin_amdgcn_ballot_w64(stop));
    }
    wave_lds_sync();
  }
  const float T = st.final_T();
  const int64_t pid = p.pid;
  const int64_t HW = (int64_t)v.H * v.W;
  float R[3];
  st.composite(T, v.bg, R);
  if constexpr (MODE == FWD_LOSS) {
    __shared__ double s_sum[4];
    double acc = 0.0;
    if (p.inside) {
      const float m = mask ? mask[pid] : 1.0f;
      const float gtc[3] = {gt[pid], gt[HW + pid], gt[2 * HW + pid]};
      float x[12];
      if constexpr (EXPO) {
#pragma unroll
        for (int k = 0; k < 12; ++k) x[k] = X[k];  // wave-uniform
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) acc += loss_term<EXPO, ROBUST>(R, x, c, m, gtc[c], rb);
      if constexpr (DEPTH) {
        const float md = dl.mask ? dl.mask[pid] : 1.0f;
        const float r = md * (Dp - dl.gt[pid]);
        acc += dl.half_weight * ((double)r * (double)r);
      }
    }
    const double sum = block_sum4(acc, s_sum);
    if (tid == 0) part[p.tile] = sum;
  } else if (p.inside) {
    final_T[pid] = T;
    n_contrib[pid] = last;
    out_color[pid] = R[0];
    out_color[HW + pid] = R[1];
    out_color[2 * HW + pid] = R[2];
    if (MODE == FWD_FULL) out_invdepth[pid] = Dp;
  }
}

// The line search's union list blended for all NS parameter sets in ONE pass (gslm_rasterize_loss_sets): per wave the
// list is walked once -- each round's 64 entries and their mask words loaded once -- and set a's round is
// k_render_fwd_wave<FWD_LOSS, true>'s round for slot a: its hits (bit 4a + q) staged from set a's records, the same
// fwd_visit on set a's own pixel state, the same per-set stop.  Set a + 1's records are loaded while set a's
// hits are visited, so a round waits on two dependent loads (entries, set 0's records) instead of two per set.
// Every set's visits and their order are the single-set kernel's: the same losses, bitwise.
// EXPO: set a's loss_term<true> through its own exposure map xp.x[a], read after the list walk and indexed by the
// unrolled set number only.  ROBUST (never with EXPO): one block rb for all sets.
template <int NS, bool EXPO = false, bool ROBUST = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NS <= 6 ? 8 : 1))) void k_render_loss_sets(ViewK v, const uint2* __restrict__ ranges,
                                                           const uint32_t* __restrict__ tile_order,
                                                           const uint32_t* __restrict__ point_list,
                                                           const uint32_t* __restrict__ amask, SetRecsK sr,
                                                           const float* __restrict__ gt, const float* __restrict__ mask,
                                                           double* __restrict__ part, int shift, ExpPtrsK xp,
                                                           gslm_robust rb) {
  __shared__ float4 s_rec[4][3 * 64];
  const TilePix p = tile_pix(v, tile_order);
  const int tid = threadIdx.x, q = tid >> 6, lane = tid & 63;
  const float pxf = (float)p.px, pyf = (float)p.py;
  const uint2 range = ranges[p.tile];
  const int n = (int)(range.y - range.x);
  const uint32_t* pl = point_list + range.x;
  const uint32_t* am = amask + range.x;
  float4* s = s_rec[q];
  FwdPix st[NS];
  uint64_t live[NS];  // per set: lanes not yet stopped
  const uint64_t in0 = __builtin_amdgcn_ballot_w64(p.inside);
#pragma unroll
  for (int a = 0; a < NS; ++a) {
    st[a] = fwd_pix(p.inside);
    live[a] = in0;
  }
  for (int base = 0; base < n; base += 64) {
    bool all = true;
#pragma unroll
    for (int a = 0; a < NS; ++a) all = all && live[a] == 0ull;
    if (all) break;  // every pixel of this quadrant has stopped in every set
    const int k = base + lane;
    uint32_t g = 0u, m = 0u;
    if (k < n) {
      g = pl_id(pl[k]);
      m = am[k] >> shift;  // sets first_set.. of the union binning (gslm_rasterize_loss_sets' first_set)
    }
    // set 0's records of this lane's entry (if it is a hit of a set still blending).  Three float4 across the set loop,
    // not a HitRec filled by load_rec: that form costs k_render_loss_sets<3, false, true> two VGPRs (56 for 54)
    bool hit = live[0] != 0ull && ((m >> q) & 1u);
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
    if (hit) {
      const float4* r = sr.rec[0] + RECS * (size_t)g;
      r0 = r[0];
      r1 = r[1];
      r2 = r[2];
    }
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      if (hit) stage_hit(s, lane, {r0, r1, r2});
      uint64_t hb = __ballot(hit);
      wave_lds_sync();
      if (a + 1 < NS) {  // the next set's records while this set's hits are visited
        hit = live[a + 1] != 0ull && ((m >> (4 * (a + 1) + q)) & 1u);
        if (hit) {
          const float4* r = sr.rec[a + 1] + RECS * (size_t)g;
          r0 = r[0];
          r1 = r[1];
          r2 = r[2];
        }
      }
      FwdPix pa = st[a];
      uint64_t lv = live[a];
      while (hb) {
        const int j = (int)__builtin_ctzll(hb);
        hb = clear_bit(hb, j);
        const HitRec h = load_hit<false>(s, j);
        float wt;
        const bool stop = fwd_visit(h, pxf, pyf, pa, wt);
        live_update(lv, hb, __builtin_amdgcn_ballot_w64(stop));
      }
      st[a] = pa;
      live[a] = lv;
      wave_lds_sync();  // this set's hits read before the next set's are staged
    }
  }
  const int64_t HW = (int64_t)v.H * v.W;
  __shared__ double s_sum[NS][4];
  float gtc[3] = {0.f, 0.f, 0.f};
  float mv = 1.0f;
  if (p.inside) {
    // from the loop's live pixel centre, not TilePix's kept index: no 64-bit value held in registers across the loop
    const int64_t pid = (int64_t)(int)pyf * v.W + (int)pxf;
    mv = mask ? mask[pid] : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) gtc[c] = gt[c * HW + pid];
  }
#pragma unroll
  for (int a = 0; a < NS; ++a) {
    double acc = 0.0;
    if (p.inside) {
      float R[3], x[12];
      st[a].composite(st[a].final_T(), v.bg, R);
      if constexpr (EXPO) {
        const float* __restrict__ X = xp.x[a];
#pragma unroll
        for (int k = 0; k < 12; ++k) x[k] = X[k];  // wave-uniform
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) acc += loss_term<EXPO, ROBUST>(R, x, c, mv, gtc[c], rb);
    }
    wave_sum_store(acc, s_sum[a]);  // all sets' sums behind one barrier
  }
  __syncthreads();
  if (tid < NS) part[(int64_t)tid * (v.gx * v.gy) + p.tile] = sum4(s_sum[tid]);
}

// per set a (block a): the sum of its per-tile partials in tile order (deterministic), times 2 (the [r; r] aliasing),
// into *loss[a]; one block and one pointer for the single-set losses (launch_render_loss).
// nsets (or NULL): the union binning's recorded set count -- slot first_set + a at or past it (masks that were never
// built) gets a NaN loss
__global__ __launch_bounds__(256) void k_tile_loss_final_sets(const double* __restrict__ part, int np, int accumulate,
                                                               LossPtrsK lp, const uint32_t* __restrict__ nsets,
                                                               int first_set) {
  __shared__ double s[4];
  const int a = blockIdx.x;
  const double sum = block_sum4(strided_sum_in_order(part + (int64_t)a * np, np), s);
  if (threadIdx.x == 0) {
    double l = 2.0 * sum;
    if (nsets && (uint32_t)(first_set + a) >= *nsets) l = __longlong_as_double(0x7ff8000000000000ll);  // quiet NaN
    double* out = lp.loss[a];
    *out = accumulate ? *out + l : l;
  }
}

int launch_render_loss_sets(const ViewK& v, const SetRecsK& sr, int nsets, const BinBufs& bb, const uint32_t* amask,
                            const float* gt, const float* mask, double* part, const LossPtrsK& lp, int accumulate,
                            hipStream_t s, int first_set, const uint32_t* nsets_dev, const ExpPtrsK* xp,
                            const gslm_robust* robust) {
  const int ntiles = v.gx * v.gy;
  if (ntiles == 0) {
    if (!accumulate)
      for (int a = 0; a < nsets; ++a) GSLM_HIP_CHECK(hipMemsetAsync(lp.loss[a], 0, sizeof(double), s));
    return GSLM_OK;
  }
  const ExpPtrsK x = xp ? *xp : ExpPtrsK{};
  const gslm_robust rb = robust ? *robust : gslm_robust{};
  if (xp && robust) {
    set_error("rasterize_loss_sets: no exposure x robust form");
    return GSLM_ERR_INVALID;
  }
  const auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(ntiles), dim3(TILE_PIX), 0, s, v, bb.ranges, bb.tile_order, bb.point_list, amask,
                       sr, gt, mask, part, 4 * first_set, x, rb);
  };
  switch (nsets) {
#define GSLM_LOSS_SETS(NS)                                        \
  case NS:                                                        \
    if (xp) launch(k_render_loss_sets<NS, true>);                 \
    else if (robust) launch(k_render_loss_sets<NS, false, true>); \
    else launch(k_render_loss_sets<NS>);                          \
    break;
    GSLM_LOSS_SETS(1) GSLM_LOSS_SETS(2) GSLM_LOSS_SETS(3) GSLM_LOSS_SETS(4)
    GSLM_LOSS_SETS(5) GSLM_LOSS_SETS(6) GSLM_LOSS_SETS(7) GSLM_LOSS_SETS(8)
#undef GSLM_LOSS_SETS
    default:
      set_error("rasterize_loss_sets: 1..8 parameter sets");
      return GSLM_ERR_INVALID;
  }
  hipLaunchKernelGGL(k_tile_loss_final_sets, dim3(nsets), dim3(256), 0, s, (const double*)part, ntiles, accumulate, lp,
                     amask ? nsets_dev : nullptr, first_set);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

// What k_render_fwd_wave takes besides the view, the binning and the records: a launcher names the members its mode
// reads, the others stay NULL.
struct FwdArgs {
  float* out_color = nullptr;
  float* out_invdepth = nullptr;
  float* final_T = nullptr;
  uint32_t* n_contrib = nullptr;
  const float* gt = nullptr;
  const float* mask = nullptr;
  double* part = nullptr;
  const uint32_t* amask = nullptr;
  int shift = 0;
  const float* X = nullptr;
  gslm_robust rb{};
  DepthLossK dl{};
};
template <int MODE, bool SLOT = false, bool EXPO = false, bool ROBUST = false, bool DEPTH = false>
static void launch_fwd(const ViewK& v, const GeomBufs& gb, const BinBufs& bb, const FwdArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((k_render_fwd_wave<MODE, SLOT, EXPO, ROBUST, DEPTH>), dim3(v.gx * v.gy), dim3(TILE_PIX), 0, s, v,
                     bb.ranges, bb.tile_order, bb.point_list, gb.rec, a.out_color, a.out_invdepth, a.final_T,
                     a.n_contrib, a.gt, a.mask, a.part, a.amask, a.shift, a.X, a.rb, a.dl);
}

int launch_render_fwd(const ViewK& v, const GeomBufs& gb, const BinBufs& bb, const ImgBufs& ib, float* out_color,
                      float* out_invdepth, hipStream_t s) {
  if (v.gx * v.gy == 0) return GSLM_OK;
  FwdArgs a;
  a.out_color = out_color;
  a.out_invdepth = out_invdepth;
  a.final_T = ib.final_T;
  a.n_contrib = ib.n_contrib;
  if (out_invdepth) launch_fwd<FWD_FULL>(v, gb, bb, a, s);
  else launch_fwd<FWD_NO_INV>(v, gb, bb, a, s);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

int launch_render_loss(const ViewK& v, const GeomBufs& gb, const BinBufs& bb, const float* gt, const float* mask,
                       double* part, double* loss, int accumulate, hipStream_t s, const uint32_t* amask, int shift,
                       const uint32_t* nsets, const float* exposure, const gslm_robust* robust,
                       const DepthLossK* depth) {
  const int ntiles = v.gx * v.gy;
  if (ntiles == 0) {
    if (!accumulate) GSLM_HIP_CHECK(hipMemsetAsync(loss, 0, sizeof(double), s));
    return GSLM_OK;
  }
  if ((exposure && robust) || (depth && (exposure || robust))) {
    set_error("rasterize_loss: no exposure x robust, depth x exposure or depth x robust form");
    return GSLM_ERR_INVALID;
  }
  FwdArgs a;
  a.gt = gt;
  a.mask = mask;
  a.part = part;
  a.amask = amask;
  a.shift = shift;
  a.X = exposure;
  if (robust) a.rb = *robust;
  if (depth) a.dl = *depth;
  if (depth && amask) launch_fwd<FWD_LOSS, true, false, false, true>(v, gb, bb, a, s);
  else if (depth) launch_fwd<FWD_LOSS, false, false, false, true>(v, gb, bb, a, s);
  else if (robust && amask) launch_fwd<FWD_LOSS, true, false, true>(v, gb, bb, a, s);
  else if (robust) launch_fwd<FWD_LOSS, false, false, true>(v, gb, bb, a, s);
  else if (exposure && amask) launch_fwd<FWD_LOSS, true, true>(v, gb, bb, a, s);
  else if (exposure) launch_fwd<FWD_LOSS, false, true>(v, gb, bb, a, s);
  else if (amask) launch_fwd<FWD_LOSS, true>(v, gb, bb, a, s);
  else launch_fwd<FWD_LOSS>(v, gb, bb, a, s);
  // the one-set case of the sets' final pass: slot shift / 4 of the union binning
  LossPtrsK lp{};
  lp.loss[0] = loss;
  hipLaunchKernelGGL(k_tile_loss_final_sets, dim3(1), dim3(256), 0, s, (const double*)part, ntiles, accumulate, lp,
                     amask ? nsets : nullptr, shift / 4);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

}  // namespace gslm
