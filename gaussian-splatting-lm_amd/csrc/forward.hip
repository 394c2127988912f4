// forward.hip -- rasterizer forward for gfx950.
//
//   k_preprocess, k_preprocess_dma, k_preprocess_views
//                  one thread per Gaussian: cull, project, cov3D, EWA cov2D, conic, radius, rect, SH->RGB; writes a
//                  48-B render record (64-B stride, the rect again in its fourth slot) + depth key + tile count + rect
//                  + clamp word.  Three kernels (SH rows read from global memory / staged by LDS-DMA / several views
//                  per pass) written from the shared parts above them: write_record, write_index_outputs,
//                  pin_pre_in, stage_sh_dma_begin / stage_sh_dma_finish.
//   (depth sort of P keys + scan of tile counts in depth order: sort.hip)
//   k_duplicate    emits (tile id, Gaussian id) pairs in depth order: the later *stable* sort on
//                  the tile id alone then yields upstream's (tile, depth, index) order with
//                  2 radix passes over N_dup instead of 6 (SURVEY §7 "Sort"); the sorted values
//                  ARE the point list.
//   k_ranges       per-tile [start, end) from key changes (identifyTileRanges).
//   k_tile_order, k_tile_order_xcd   the tile passes' launch order (longest list first; XCD-banded for the LM product).
//   k_point_ids    the Gaussian ids of a point list (its quadrant masks stripped).
//   k_tile_neff, k_tile_cost, k_quad_live, k_row_flags, k_row_final   the LM row map and the LM product's tile cost.
//   k_active_flags, k_active_scatter, k_union_flags, k_union_scatter   the active Gaussians of one view / of a batch.
//   k_depth_positions, k_union_rect, k_duplicate_union   the line search's union binning in depth space.
//   launchers: launch_preprocess(_views), launch_binning, launch_ranges, launch_tile_order, launch_lm_rowmap,
//   launch_active_list / _union, launch_depth_positions, launch_union_rect / _binning, launch_point_ids.
//   (k_render_fwd, the per-tile blend: render_fwd.hip)
#include "gslm_internal.hpp"
#include "gslm_kernels.hpp"
#include "gslm_tile.hpp"

namespace gslm {

// ------------------------------------------------------------------ the preprocess kernels' shared parts
// The arithmetic is gslm_kernels.hpp's (load_pre_in, preprocess_core, preprocess_color); the parts below are what the
// three kernels do around it.  Each is block-uniform only where it says so.

// The rect as k_duplicate and row_slot read it: min | max, x in the low and y in the high 16 bits.
__device__ __forceinline__ uint2 pack_rect(const PreOut& o) {
  return make_uint2((uint32_t)o.rmin_x | ((uint32_t)o.rmin_y << 16), (uint32_t)o.rmax_x | ((uint32_t)o.rmax_y << 16));
}

// The 64-B render record of one visible Gaussian at `rec` (index space: rec + RECS * i; depth space: rec + RECS *
// pos[i]): three float4 of (x, y, conic | opacity, rgb | 1/depth, clamp word, tq) and the rect again in the fourth slot
// -- k_duplicate's random per-Gaussian read is then one 64-B record (one cache line) instead of the record and a rect
// line.  The only place that knows the record's layout on the writing side.
__device__ __forceinline__ void write_record(float4* __restrict__ rec, const PreOut& o) {
  const uint2 rc = pack_rect(o);
  rec[0] = make_float4(o.x, o.y, o.conic[0], o.conic[1]);
  rec[1] = make_float4(o.conic[2], o.opac, o.rgb[0], o.rgb[1]);
  rec[2] = make_float4(o.rgb[2], 1.0f / o.depth, __uint_as_float(o.clamped), o.tq);
  rec[3] = make_float4(__uint_as_float(rc.x), __uint_as_float(rc.y), 0.f, 0.f);
}
// A culled Gaussian's record in depth space: the zero rect slot alone (an empty rect; the union binning reads no other
// slot of it).  Index space writes nothing for a culled Gaussian: its tile count is 0 and nothing reads its record.
__device__ __forceinline__ void write_culled_record(float4* __restrict__ rec) {
  rec[3] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// Every index-space output of Gaussian i, once: tile count, depth key, radius (where asked for) and, when visible, the
// record, the rect and the clamp word (both read only where tiles[i] != 0).  o.depth must be set whether visible or not
// (preprocess_core sets it before any cull), o's other fields only when visible.
// The depth key: the depth's bits for every Gaussian in front of the near plane, culled by its footprint or not, and
// 0xFFFFFFFF otherwise.  The depth order then depends on means3D and the view alone, so one view's order is reusable
// while xyz is unchanged (the LM step freezes xyz: gslm_preprocess_ordered).  The point list is the same either way
// (Gaussians culled later emit no tile).
__device__ __forceinline__ void write_index_outputs(const PreOutBufs& ob, int* __restrict__ radii_out, int64_t i,
                                                    bool vis, const PreOut& o) {
  ob.depth_key[i] = o.depth > 0.2f ? __float_as_uint(o.depth) : 0xFFFFFFFFu;
  if (!vis) {
    ob.tiles[i] = 0u;
    if (radii_out) radii_out[i] = 0;
    return;
  }
  write_record(ob.rec + RECS * i, o);
  ob.tiles[i] = (uint32_t)((o.rmax_x - o.rmin_x) * (o.rmax_y - o.rmin_y));
  ob.rect[i] = pack_rect(o);
  ob.clampw[i] = o.clamped;
  if (radii_out) radii_out[i] = o.radius;
}

// Keeps the loads of `in` (and the wait for them) ahead of whatever follows: hipcc waits vmcnt(0) at the first use of
// an ordinary load issued while an LDS-DMA is outstanding, so inputs still in flight behind the DMA would make the
// geometry wait for the rows.  Emits no instruction.
__device__ __forceinline__ void pin_pre_in(const PreIn& in) {
  asm volatile("" : : "v"(in.x), "v"(in.y), "v"(in.z), "v"(in.c[0]), "v"(in.c[1]), "v"(in.c[2]), "v"(in.c[3]),
               "v"(in.c[4]), "v"(in.c[5]), "v"(in.qw), "v"(in.op));
}

__device__ __forceinline__ void glds16(const float4* src, float4* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// The block's SH-rest rows staged in LDS by LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave-instruction, no VGPR
// round trip), in two halves with the geometry between them.  The order is the contract:
//   1. every thread has loaded and pinned its Gaussian's inputs (load_pre_in, pin_pre_in);
//   2. stage_sh_dma_begin issues the DMA;
//   3. the geometry (preprocess_core, no colour) runs while the rows land;
//   4. stage_sh_dma_finish: the barrier, the tail, g.rest pointed at the copy;
//   5. the colour (preprocess_color) reads the rows from LDS.
// Both are block-uniform: every thread of a 256-thread block calls them, live or not, before any early return.
// The span: [nv][g.rest_stride] floats from `lead` floats before the block's first rest row (stage_lead: 16-B
// aligned there, and i0 * rest_stride * 4 B is a multiple of 16 as i0 % 256 == 0), copied to s_rows[0 ..) --
// 256 * rest_stride floats of dynamic LDS.
struct ShSpan {
  const float* rows;  // the span in global memory
  int64_t total, n4;  // its floats, its whole float4s
};

// Issues the span's whole float4s: 64-float4 chunks, chunk c by wave c % 4.  A lane past the last float4 re-reads the
// last one: the clamp to n4 - 1 keeps every source address inside the span.  (Its LDS slot lies behind the span's
// whole float4s and inside the 256 rows, as ceil(n4 / 64) <= rest_stride; finish's tail overwrites the floats of it
// that are read.)  n4 == 0 (a last block of one short row) issues nothing: the loop is left before the clamp could
// form index -1.
__device__ __forceinline__ ShSpan stage_sh_dma_begin(const GaussK& g, int lead, float* s_rows) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x;
  const int64_t nv = min((int64_t)blockDim.x, g.P - i0);
  ShSpan sp;
  sp.total = nv * g.rest_stride;
  sp.n4 = sp.total / 4;
  sp.rows = g.rest - lead + i0 * g.rest_stride;
  const float4* src4 = reinterpret_cast<const float4*>(sp.rows);
  float4* dst4 = reinterpret_cast<float4*>(s_rows);
  for (int64_t c = w; c * 64 < sp.n4; c += 4) {
    const int64_t e = min(c * 64 + lane, sp.n4 - 1);
    glds16(src4 + e, dst4 + c * 64);
  }
  return sp;
}

// The DMA has landed after the barrier (its vmcnt(0)); a span that is not a whole number of float4 (the last block
// only) gets its last 1-3 floats by plain loads and a second barrier.  Then g reads the block's rows from LDS.
__device__ __forceinline__ void stage_sh_dma_finish(GaussK& g, int lead, float* s_rows, const ShSpan& sp) {
  __syncthreads();
  if (sp.n4 * 4 < sp.total) {
    for (int64_t e = sp.n4 * 4 + threadIdx.x; e < sp.total; e += blockDim.x) s_rows[e] = sp.rows[e];
    __syncthreads();
  }
  g.rest = s_rows + lead;
  g.rest_base = (int64_t)blockIdx.x * blockDim.x;
}

// ------------------------------------------------------------------ the preprocess kernels
// The SH rows read from global memory: the kernel of the layouts stage_lead refuses (colours given, degree 0, an
// unaligned or padded rest).
template <bool RAW>
__global__ __launch_bounds__(256) void k_preprocess(ViewK v, GaussK g, PreOutBufs ob, int* __restrict__ radii_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.P) return;
  PreOut o;
  const bool vis = preprocess_one<RAW>(v, g, i, o);
  write_index_outputs(ob, radii_out, i, vis, o);
}

// k_preprocess with the block's SH-rest rows staged by LDS-DMA and the staging overlapped with the geometry
// (stage_sh_dma_begin's contract).  Per-thread reads of the rows at a 180-B stride made every load instruction touch
// 64 cache lines (the unstaged kernel ran at ~2.2 TB/s on the contiguous leaf).  Same arithmetic in the same order:
// bitwise the same records.
template <bool RAW>
__global__ __launch_bounds__(256) void k_preprocess_dma(ViewK v, GaussK g, PreOutBufs ob, int* __restrict__ radii_out,
                                                         int lead) {
  extern __shared__ __attribute__((aligned(16))) float s_sh[];  // [256 * rest_stride]
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < g.P;
  PreIn in{};
  if (live) load_pre_in<RAW>(g, i, in);
  pin_pre_in(in);
  const ShSpan sp = stage_sh_dma_begin(g, lead, s_sh);
  PreOut o;
  const bool vis = live && preprocess_core<RAW, false>(v, g, i, in, o);
  stage_sh_dma_finish(g, lead, s_sh, sp);
  if (!live) return;
  if (vis) preprocess_color(v, g, i, in, o);
  write_index_outputs(ob, radii_out, i, vis, o);
}

// k_preprocess_dma for up to MAX_PRE_VIEWS views in one pass over the Gaussians (gslm_preprocess_views: the line
// search's parameter sets over a batch of validation views).  A view's inputs cost 236 B per Gaussian at SH 3 against
// 84 B of its outputs; the block loads its Gaussians' inputs and stages their SH rows once, then writes every view's
// outputs from them.  Per view the same functions in the same order as k_preprocess_dma: bitwise the same geometry.
// STAGE: the rows are staged (views_pass_ok: lead 0); otherwise (SH degree 0, colours or cov3D given, an odd layout)
// every view reads its inputs from global memory -- the same outputs, depth space included.
// A view with depth positions (the line search's union lists) gets the render record alone, at the Gaussian's depth
// position: one 64-B record per Gaussian, read in depth order by the union binning.
template <bool RAW, bool STAGE>
__global__ __launch_bounds__(256) void k_preprocess_views(PreViewsK pv, GaussK g) {
  extern __shared__ __attribute__((aligned(16))) float s_sh[];  // [256 * rest_stride] (STAGE)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < g.P;
  PreIn in{};
  if (live) load_pre_in<RAW>(g, i, in);
  pin_pre_in(in);
  ShSpan sp{};
  if constexpr (STAGE) sp = stage_sh_dma_begin(g, 0, s_sh);
  // view 0's geometry while the rows land (as k_preprocess_dma)
  PreOut o0;
  const bool vis0 = live && preprocess_core<RAW, false>(pv.v[0], g, i, in, o0);
  if constexpr (STAGE) stage_sh_dma_finish(g, 0, s_sh, sp);
  if (!live) return;
#pragma unroll 1
  for (int b = 0; b < pv.n; ++b) {
    const ViewK& v = pv.v[b];
    const PreOutBufs& ob = pv.out[b];
    PreOut o;
    bool vis;
    if (b == 0) {
      o = o0;
      vis = vis0;
    } else {
      vis = preprocess_core<RAW, false>(v, g, i, in, o);
    }
    float4* const drec = ob.pos ? ob.rec + RECS * (size_t)ob.pos[i] : nullptr;  // depth space
    // (the culled exit stands before the colour: `if (vis)` around the colour and one writer call behind it compiled
    // to 2-5 more VGPRs in every instantiation)
    if (!vis) {
      if (drec) write_culled_record(drec);
      else write_index_outputs(ob, nullptr, i, false, o);
      continue;
    }
    preprocess_color(v, g, i, in, o);
    if (drec) write_record(drec, o);
    else write_index_outputs(ob, nullptr, i, true, o);
  }
}

// whether k_preprocess_views can stage the SH rows: raw GaussianModel leaves with the SH rest as its contiguous 16-B
// aligned leaf (otherwise the unstaged instantiation runs, depth positions included)
static bool views_pass_ok(const GaussK& g) { return g.raw && !g.cov3D && stage_lead(g) == 0; }

int launch_preprocess_views(const PreViewsK& pv, const GaussK& g, hipStream_t s) {
  if (g.P == 0 || pv.n == 0) return GSLM_OK;
  const dim3 grid((unsigned)((g.P + 255) / 256));
  if (views_pass_ok(g)) {
    const size_t lds = (size_t)256 * g.rest_stride * sizeof(float);
    hipLaunchKernelGGL((k_preprocess_views<true, true>), grid, dim3(256), lds, s, pv, g);
  } else if (g.raw) {  // every layout and both output spaces (depth positions included): no per-view fallback
    hipLaunchKernelGGL((k_preprocess_views<true, false>), grid, dim3(256), 0, s, pv, g);
  } else {
    hipLaunchKernelGGL((k_preprocess_views<false, false>), grid, dim3(256), 0, s, pv, g);
  }
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

// One block per 256 consecutive Gaussians of the depth order: their (tile, id) pairs are one contiguous
// output range, written by the whole block in element order (coalesced, and a large Gaussian's tiles are
// spread over the block instead of one thread's loop).  Element e belongs to the last Gaussian whose
// local offset is <= e (binary search in LDS); inside a Gaussian the rect is walked row-major.
// n_dev (or NULL): N is the list capacity and *n_dev the pair count (the depth-order scan's total, not read back
// by the host: gslm_rasterize_dev); pairs past the capacity are not written (the host sees the count and renders
// that view again with a larger list)
// zero_ranges (ntiles of them): the tile ranges the binning's k_ranges fills afterwards, zeroed here by a grid-stride
// store (every range left [0, 0) stays an empty tile) -- one memset launch less per binning
__device__ __forceinline__ void zero_tile_ranges(uint2* __restrict__ ranges, int ntiles) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < ntiles; t += (int64_t)gridDim.x * blockDim.x)
    ranges[t] = make_uint2(0u, 0u);
}

__global__ __launch_bounds__(256) void k_duplicate(int64_t P, int gx, const uint32_t* __restrict__ sorted_idx,
                                                    const uint32_t* __restrict__ offsets, uint32_t N,
                                                    const uint32_t* __restrict__ n_dev,
                                                    const uint2* __restrict__ rect, const float4* __restrict__ rec,
                                                    uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                    uint2* __restrict__ zero_ranges, int ntiles) {
  __shared__ QuadCull s_q[256];
  __shared__ uint32_t s_off[257];
  __shared__ uint32_t s_g[256];
  __shared__ uint32_t s_rc[256][3];  // x0, y0, width
  zero_tile_ranges(zero_ranges, ntiles);
  const int tid = threadIdx.x;
  const int64_t s0 = (int64_t)blockIdx.x * 256, s = s0 + tid;
  const int64_t slast = min(s0 + 255, P - 1);
  const uint32_t base = offsets[s0];
  const uint32_t Ntot = n_dev ? *n_dev : N;
  uint32_t n = 0;
  if (s < P) {
    const uint32_t g = sorted_idx[s];
    // the tile count from the depth-order scan (coalesced) instead of tiles[g] (a random line per Gaussian);
    // culled Gaussians (n = 0) then touch nothing else
    const uint32_t o = offsets[s];
    n = (s + 1 < P ? offsets[s + 1] : Ntot) - o;
    s_off[tid] = o - base;
    if (n) {
      const float4 r3 = rec[RECS * (int64_t)g + 3];  // the rect (k_preprocess' copy in the record's padding)
      const uint2 rc = make_uint2(__float_as_uint(r3.x), __float_as_uint(r3.y));
      const int x0 = rc.x & 0xFFFF, y0 = rc.x >> 16, x1 = rc.y & 0xFFFF;
      s_rc[tid][0] = (uint32_t)x0;
      s_rc[tid][1] = (uint32_t)y0;
      s_rc[tid][2] = (uint32_t)(x1 - x0);
      s_g[tid] = g;
      const float4 r0 = rec[RECS * (int64_t)g + 0];
      s_q[tid] = quad_cull_prep(r0.x, r0.y, r0.z, r0.w, rec[RECS * (int64_t)g + 1].x, rec[RECS * (int64_t)g + 2].w);
    }
  } else {
    s_off[tid] = 0xFFFFFFFFu;  // past the block's last Gaussian: never an owner
  }
  if (s == slast) s_off[256] = offsets[s] - base + n;
  __syncthreads();
  // the block's pairs [base, base + total), clipped to the capacity (a no-op when N is the count)
  const uint32_t total = base < N ? min(s_off[256], N - base) : 0u;
  for (uint32_t e = tid; e < total; e += 256) {
    // last t with s_off[t] <= e (s_off[0] = 0; non-decreasing, 0xFFFFFFFF past the block's last Gaussian): 8 fixed
    // steps, no divergent loop (its per-lane exit made every step a few scalar exec-mask instructions)
    int lo = 0;
#pragma unroll
    for (int step = 128; step > 0; step >>= 1) lo = s_off[lo + step] <= e ? lo + step : lo;
    const uint32_t li = e - s_off[lo];
    const uint32_t w = s_rc[lo][2];
    const uint32_t dy = li / w;
    const int tx = (int)(s_rc[lo][0] + (li - dy * w)), ty = (int)(s_rc[lo][1] + dy);
    keys[base + e] = (uint32_t)(ty * gx + tx);
    vals[base + e] = s_g[lo] | (quad_mask(s_q[lo], tx, ty) << ID_BITS);
  }
}

// Launch order of the tile passes: tiles by descending list length (a longest-first schedule, so the
// costliest tiles do not start last and set the kernel's tail).  One block; buckets of the length
// (exact below 768 entries, 32-wide above), order inside a bucket arbitrary.  Only scheduling
// changes: every tile's results are independent of when it runs.
// cost (or NULL): a per-tile cost key instead of the list length (k_tile_cost: the LM product's modelled wave-visits).
__global__ __launch_bounds__(1024) void k_tile_order(int ntiles, const uint2* __restrict__ ranges,
                                                      uint32_t* __restrict__ order, const uint32_t* __restrict__ cost) {
  __shared__ uint32_t s_cnt[1024];
  const int tid = threadIdx.x;
  s_cnt[tid] = 0u;
  __syncthreads();
  auto bucket = [&](int t) {
    const uint32_t n = cost ? cost[t] : ranges[t].y - ranges[t].x;
    return 1023u - (n < 768u ? n : min(1023u, 768u + ((n - 768u) >> 5)));  // heaviest first
  };
  for (int t = tid; t < ntiles; t += 1024) atomicAdd(&s_cnt[bucket(t)], 1u);
  __syncthreads();
  // exclusive scan of the 1024 bucket counts: each wave's 64 by shuffles, then the 16 wave totals (two barriers;
  // a block-wide Hillis-Steele scan took 20)
  __shared__ uint32_t s_wsum[16];
  const int lane = tid & 63, w = tid >> 6;
  const uint32_t v = s_cnt[tid];
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) s_wsum[w] = inc;
  __syncthreads();
  uint32_t wbase = 0u;
  for (int k = 0; k < w; ++k) wbase += s_wsum[k];
  s_cnt[tid] = wbase + inc - v;  // exclusive
  __syncthreads();
  for (int t = tid; t < ntiles; t += 1024) order[atomicAdd(&s_cnt[bucket(t)], 1u)] = (uint32_t)t;
}

// XCD-aware form of the launch order (the LM product's).  Blocks are dealt round-robin over the 8
// XCDs, so blocks b and b + 8 share one XCD's L2 (MI355X_MICROARCH.md §Workgroup dispatch: observed, a speed choice,
// never correctness).  The tiles are cut, in row-major order, into XG contiguous bands of equal total weight (the
// cost key, or the list length, + 1), band g longest-first as k_tile_order orders the whole frame, and band g's k-th
// tile launched as block 8 k + g while every band still has tiles (the bands' leftover, cheapest tiles close the
// order).  Each XCD then gathers the records of about an eighth of the frame's Gaussians instead of all of them.
constexpr int XG = 8;
__global__ __launch_bounds__(1024) void k_tile_order_xcd(int ntiles, const uint2* __restrict__ ranges,
                                                          uint32_t* __restrict__ order,
                                                          const uint32_t* __restrict__ cost) {
  __shared__ uint32_t s_cnt[XG][1024];
  __shared__ unsigned long long s_w64[16];
  __shared__ uint32_t s_w32[16];
  __shared__ uint32_t s_n[XG];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  auto len = [&](int t) { return cost ? cost[t] : ranges[t].y - ranges[t].x; };
  auto bucket = [&](uint32_t n) { return 1023u - (n < 768u ? n : min(1023u, 768u + ((n - 768u) >> 5))); };
  // 1. each thread a contiguous run of tiles: its weight, the block-wide exclusive prefix of the runs' weights
  const int seg = (ntiles + 1023) / 1024, t0 = min(ntiles, tid * seg), t1 = min(ntiles, t0 + seg);
  unsigned long long mine = 0ull;
  for (int t = t0; t < t1; ++t) mine += (unsigned long long)len(t) + 1ull;
  unsigned long long inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) s_w64[w] = inc;
#pragma unroll
  for (int g = 0; g < XG; ++g) s_cnt[g][tid] = 0u;
  __syncthreads();
  unsigned long long before = 0ull, total = 0ull;
  for (int k = 0; k < 16; ++k) {
    if (k < w) before += s_w64[k];
    total += s_w64[k];
  }
  before += inc - mine;
  // band of a tile: where the middle of its weight falls in the frame's total
  auto band = [&](unsigned long long pre, uint32_t wt) {
    return (int)min((unsigned long long)(XG - 1), ((2ull * pre + wt) * XG) / (2ull * total));
  };
  // 2. histogram of (band, length bucket)
  {
    unsigned long long pre = before;
    for (int t = t0; t < t1; ++t) {
      const uint32_t n = len(t);
      atomicAdd(&s_cnt[band(pre, n + 1u)][bucket(n)], 1u);
      pre += n + 1u;
    }
  }
  __syncthreads();
  // 3. per band, the exclusive scan of its 1024 bucket counts (the existing k_tile_order scan, once per band)
  for (int g = 0; g < XG; ++g) {
    const uint32_t v = s_cnt[g][tid];
    uint32_t inc32 = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(inc32, o, 64);
      if (lane >= o) inc32 += y;
    }
    if (lane == 63) s_w32[w] = inc32;
    __syncthreads();
    uint32_t wbase = 0u, tot = 0u;
    for (int k = 0; k < 16; ++k) {
      if (k < w) wbase += s_w32[k];
      tot += s_w32[k];
    }
    s_cnt[g][tid] = wbase + inc32 - v;
    if (tid == 0) s_n[g] = tot;
    __syncthreads();
  }
  // 4. each tile's rank in its band -> its block
  uint32_t m = s_n[0];
#pragma unroll
  for (int g = 1; g < XG; ++g) m = min(m, s_n[g]);
  unsigned long long pre = before;
  for (int t = t0; t < t1; ++t) {
    const uint32_t n = len(t);
    const int g = band(pre, n + 1u);
    pre += n + 1u;
    const uint32_t r = atomicAdd(&s_cnt[g][bucket(n)], 1u);
    uint32_t b;
    if (r < m) {
      b = r * XG + (uint32_t)g;
    } else {
      b = m * XG + (r - m);
      for (int h = 0; h < g; ++h) b += s_n[h] - m;
    }
    order[b] = (uint32_t)t;
  }
}

// the launch order of a tile pass: by the LM product's modelled cost (cost != NULL) k_tile_order_xcd, unless
// GSLM_TILE_ORDER=flat (A/B); by list length (the forward, the loss blends) the frame-wide k_tile_order -- banded by
// length the blends ran 11-15% slower (profiles/r05/ab/tile_order_xcd_lm_kept/): a list's length does not price a
// blend that stops at T < 1e-4, so equal-length bands are unequal work for their XCDs, while the modelled cost does
static bool tile_order_xcd() {
  static const bool on = [] {
    const char* e = getenv("GSLM_TILE_ORDER");
    return !(e && std::string(e) == "flat");
  }();
  return on;
}
// one launcher for both forms (the tile passes' through launch_tile_order, gslm_selftest_tile_order's by its argument)
int launch_tile_order_form(int form, int ntiles, const uint2* ranges, uint32_t* order, const uint32_t* cost,
                           hipStream_t s) {
  if (form == TILE_ORDER_XCD)
    hipLaunchKernelGGL(k_tile_order_xcd, dim3(1), dim3(1024), 0, s, ntiles, ranges, order, cost);
  else
    hipLaunchKernelGGL(k_tile_order, dim3(1), dim3(1024), 0, s, ntiles, ranges, order, cost);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}
int launch_tile_order(int ntiles, const uint2* ranges, uint32_t* order, const uint32_t* cost, hipStream_t s) {
  return launch_tile_order_form(cost && tile_order_xcd() ? TILE_ORDER_XCD : TILE_ORDER_FLAT, ntiles, ranges, order, cost,
                                s);
}

// Gaussian ids of the sorted list (mask bits stripped), for gslm_inspect.
__global__ __launch_bounds__(256) void k_point_ids(int64_t N, const uint32_t* __restrict__ pl, uint32_t* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < N) out[k] = pl_id(pl[k]);
}

// n_dev (or NULL): as k_duplicate (N the capacity, *n_dev the count); n_out (or NULL) receives the count.
// RANGES_KEYS consecutive keys per thread from one 16-B load (the list's key buffers are 256-B aligned), the keys just
// before and after the group from memory (the neighbouring threads' loads: cache hits): a quarter of the threads of a
// key per thread, each with one vector load instead of three scalar ones.
constexpr int RANGES_KEYS = 4;
__global__ __launch_bounds__(256) void k_ranges(int64_t N, const uint32_t* __restrict__ keys,
                                                 uint2* __restrict__ ranges, const uint32_t* __restrict__ n_dev,
                                                 uint32_t* __restrict__ n_out) {
  const int64_t k0 = RANGES_KEYS * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  if (n_dev) {
    const uint32_t c = *n_dev;
    if (n_out && k0 == 0) *n_out = c;
    N = min(N, (int64_t)c);
  }
  if (k0 >= N) return;
  constexpr uint32_t NONE = 0xFFFFFFFFu;  // never a tile id: a list edge
  uint32_t t[RANGES_KEYS];
  if (k0 + RANGES_KEYS <= N) {
    const uint4 v = *reinterpret_cast<const uint4*>(keys + k0);
    t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < RANGES_KEYS; ++j) t[j] = k0 + j < N ? keys[k0 + j] : NONE;
  }
  const uint32_t before = k0 > 0 ? keys[k0 - 1] : NONE;
  const uint32_t after = k0 + RANGES_KEYS < N ? keys[k0 + RANGES_KEYS] : NONE;
#pragma unroll
  for (int j = 0; j < RANGES_KEYS; ++j) {
    if (t[j] == NONE) break;  // past the list's end
    const uint32_t p = j ? t[j - 1] : before, q = j + 1 < RANGES_KEYS ? t[j + 1] : after;
    if (p != t[j]) ranges[t[j]].x = (uint32_t)(k0 + j);
    if (q != t[j]) ranges[t[j]].y = (uint32_t)(k0 + j + 1);
  }
}
// k_ranges over N sorted keys (the binnings', and gslm_selftest_ranges'): the ranges zeroed beforehand, N > 0
int launch_ranges(int64_t N, const uint32_t* keys_sorted, uint2* ranges, const uint32_t* n_dev, uint32_t* n_out,
                  hipStream_t s) {
  if (N <= 0) return GSLM_OK;
  const unsigned nbN = (unsigned)((N + 256 * RANGES_KEYS - 1) / (256 * RANGES_KEYS));
  hipLaunchKernelGGL(k_ranges, dim3(nbN), dim3(256), 0, s, N, keys_sorted, ranges, n_dev, n_out);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

// ---- the LM row map (ScratchBufs::hscan), once per geometry ----
// Computed by the first LM product on a geometry (GSLM_MV_TAIL_CLEAN protocol), not by the forward: the
// goff / rect gathers are random over 12 B per Gaussian and the drop-in backward does not need the map.
// largest n_contrib over each tile quadrant's pixels (wave q's 8x8 block, tile_pixel): list positions at or past it
// are blended by no pixel of that quadrant
__global__ __launch_bounds__(256) void k_tile_neff(ViewK v, const uint32_t* __restrict__ n_contrib,
                                                    uint32_t* __restrict__ neff) {
  const int tile = blockIdx.x, tile_x = tile % v.gx, tile_y = tile / v.gx;
  int px, py;
  tile_pixel(tile_x, tile_y, threadIdx.x, px, py);
  int wm = (px < v.W && py < v.H) ? (int)n_contrib[(int64_t)py * v.W + px] : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) wm = max(wm, __shfl_xor(wm, o));
  if ((threadIdx.x & 63) == 0) neff[4 * tile + (threadIdx.x >> 6)] = (uint32_t)wm;
}

// The LM product's cost of a tile, in wave-visits (k_render_matvec's schedule model): the J v pass runs one
// independent wave per quadrant, so its busiest wave -- the largest count over quadrants q of the list positions
// below the quadrant's bound neff[q] whose mask holds q -- sets its time; the VJP pass runs 128-entry batches from
// max_q neff down with a block barrier around each, so every batch costs its busiest wave's count.  Cost = the two
// summed.  Tiles ordered by it (k_tile_order) schedule the product's blocks longest-first by what they actually do:
// the list length, the forward's key, ranks them by entries no LM pass visits (tools/exp/tile_sched.py: modelled
// idle tail 11.8% of the launch by length, 5.3% by this cost).  One block per tile; threads 0..127 take batch b,
// 128..255 batch b + 1 (two waves per batch).
__global__ __launch_bounds__(256) void k_tile_cost(const uint2* __restrict__ ranges,
                                                    const uint32_t* __restrict__ point_list,
                                                    const uint32_t* __restrict__ neff, uint32_t* __restrict__ cost) {
  __shared__ uint32_t s_c[4][4];  // [wave][quadrant] counts of the current pair of batches
  const int tile = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
  const uint2 r = ranges[tile];
  const uint32_t len = r.y - r.x;
  uint32_t wm[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) wm[q] = min(neff[4 * tile + q], len);
  const int n_eff = (int)max(max(wm[0], wm[1]), max(wm[2], wm[3]));
  uint32_t tot[4] = {0u, 0u, 0u, 0u}, vjp = 0u;
  for (int base = 0; base < n_eff; base += 256) {
    // batch b = base / 128 + (tid >> 7): list position n_eff - 1 - (base + tid)
    const int pos = n_eff - 1 - (base + tid);
    uint32_t m = 0u;
    if (pos >= 0) {
      const uint32_t e = point_list[r.x + pos];
      m = pl_mask(e) & (((uint32_t)pos < wm[0] ? 1u : 0u) | ((uint32_t)pos < wm[1] ? 2u : 0u) |
                        ((uint32_t)pos < wm[2] ? 4u : 0u) | ((uint32_t)pos < wm[3] ? 8u : 0u));
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t c = (uint32_t)__popcll(__ballot((m >> q) & 1u));
      if ((tid & 63) == 0) s_c[w][q] = c;
    }
    __syncthreads();
    uint32_t b0 = 0u, b1 = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t c0 = s_c[0][q] + s_c[1][q], c1 = s_c[2][q] + s_c[3][q];
      tot[q] += c0 + c1;
      b0 = max(b0, c0);
      b1 = max(b1, c1);
    }
    vjp += b0 + b1;
    __syncthreads();
  }
  if (tid == 0) cost[tile] = max(max(tot[0], tot[1]), max(tot[2], tot[3])) + vjp;
}

// GSLM_LIVE_MASKS=0 (A/B): the row map on the binning's own quadrant masks, without k_quad_live.  Read at every row
// map, once per geometry (gslm.lm.live_masks validates the value).
static bool live_masks_on() {
  const char* e = getenv("GSLM_LIVE_MASKS");
  return !(e && std::string(e) == "0");
}

// Refines the list's quadrant masks to the visits some pixel blends.  The binning's mask bit q of an entry says its
// alpha region can reach quadrant q (quad_mask: conservative); whether any pixel of the quadrant blends it -- inside
// the image, list position below its n_contrib, !(power > 0), alpha >= 1/255 -- depends on the geometry only, which
// is fixed from one forward to the next: rhs(), every CG iteration, every restart.  A visit that no lane blends
// runs no body in the J v pass and stores a zero partial in the VJP pass, so with its bit cleared both skip it and
// compute the same bits; an entry left with an empty mask is no head (k_row_flags) and owns no row.
// One block per tile, one independent wave per quadrant, in the shape of jvp_wave_packed: 64 list positions per
// round, only the wave's hits below its bound neff[q], the primal half of the record (position, conic, opacity) in
// the wave's own LDS slots, power and alpha exactly as jvp_wave_packed and vjp_tile compute them (gpower, gexp,
// fminf(0.99f, o G), uncontracted).  The lane that fetched a hit no lane blends clears bit q of that entry:
// an integer atomic AND, each of the tile's four waves owning one bit of the word.  Nothing else in the entry
// changes, and positions at or past neff[q] are left alone (every consumer masks them by the same bound).
// Idempotent: a cleared bit is no hit and a live visit stays live, so a row map rebuilt on one binning
// (launch_lm_rowmap once per product kind) refines nothing further.
__global__ __launch_bounds__(256) void k_quad_live(ViewK v, const uint2* __restrict__ ranges,
                                                    const uint32_t* __restrict__ tile_order,
                                                    const uint32_t* __restrict__ neff,
                                                    const float4* __restrict__ rec,
                                                    const uint32_t* __restrict__ n_contrib, uint32_t* point_list) {
  __shared__ float4 s_a[4][64];  // [wave][lane]: x, y, conic a, conic b
  __shared__ float2 s_b[4][64];  //               conic c, opacity
  const TilePix p = tile_pix(v, tile_order);
  const int tid = threadIdx.x, q = tid >> 6, lane = tid & 63;
  const uint32_t my_last = p.inside ? n_contrib[p.pid] : 0u;
  const uint2 range = ranges[p.tile];
  const int wm = __builtin_amdgcn_readfirstlane((int)min(neff[4 * p.tile + q], range.y - range.x));
  const float pxf = (float)p.px, pyf = (float)p.py;
  uint32_t* pl = point_list + range.x;
  float4* sa = s_a[q];
  float2* sb = s_b[q];
  for (int base = 0; base < wm; base += 64) {
    const int k = base + lane;
    bool hit = false;
    if (k < wm) {
      // the other waves clear their own bits of this word meanwhile: bit q and the id are this wave's to read
      const uint32_t e = __hip_atomic_load(pl + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((pl_mask(e) >> q) & 1u) {
        hit = true;
        const uint32_t g = pl_id(e);
        const float4 r0 = rec[RECS * (size_t)g + 0], r1 = rec[RECS * (size_t)g + 1];
        sa[lane] = r0;
        sb[lane] = make_float2(r1.x, r1.y);
      }
    }
    uint64_t hb = __ballot(hit);
    const int rel = (int)my_last - base;  // pos = base + j < my_last as j < rel
    uint64_t live = 0ull;                 // the round's hits some lane blends
    wave_lds_sync();
    while (hb) {
      const int j = (int)__builtin_ctzll(hb);
      hb = clear_bit(hb, j);
      const float4 a = sa[j];
      const float2 b = sb[j];
      const float dx = a.x - pxf, dy = a.y - pyf;
      const float power = gpower(a.z, a.w, b.x, dx, dy);
      const float G = gexp(power);
      const float alpha = fminf(0.99f, b.y * G);
      const bool c_last = j < rel, c_pow = !(power > 0.0f), c_alpha = alpha >= 1.0f / 255.0f;
      if (__builtin_amdgcn_ballot_w64(c_last && c_pow && c_alpha)) live |= 1ull << j;
    }
    if (hit && !((live >> lane) & 1ull)) atomicAnd(pl + k, ~(1u << (ID_BITS + q)));
    wave_lds_sync();
  }
}

// The quadrants whose pixels still blend at list position pos (vjp_tile's per-wave bounds) and the entry's
// effective mask: its quadrant mask restricted to them.  A head entry is one with a non-empty effective mask.
__device__ __forceinline__ uint32_t eff_mask(uint32_t e, uint32_t pos, const uint32_t* wm4) {
  const uint32_t wb = (pos < wm4[0] ? 1u : 0u) | (pos < wm4[1] ? 2u : 0u) | (pos < wm4[2] ? 4u : 0u) |
                      (pos < wm4[3] ? 8u : 0u);
  return pl_mask(e) & wb;
}

// head flag of every sorted entry at its goff-order slot, and the goff slot itself in slots[k]
__global__ __launch_bounds__(256) void k_row_flags(int64_t N, int gx, const uint32_t* __restrict__ keys,
                                                    const uint32_t* __restrict__ point_list,
                                                    const uint2* __restrict__ ranges, const uint32_t* __restrict__ neff,
                                                    const uint32_t* __restrict__ goff, const uint2* __restrict__ rect,
                                                    uint32_t* __restrict__ slots, uint32_t* __restrict__ flags) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  const uint32_t t = keys[k];
  const uint32_t e = point_list[k];
  const uint32_t g = pl_id(e);
  const uint32_t o = row_slot(goff[g], rect[g], (int)(t % (uint32_t)gx), (int)(t / (uint32_t)gx));
  slots[k] = o;
  flags[o] = eff_mask(e, (uint32_t)k - ranges[t].x, neff + 4 * (size_t)t) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_row_final(int64_t N, const uint32_t* __restrict__ hscan,
                                                    uint32_t* __restrict__ slots) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < N) slots[k] = hscan[slots[k]];  // non-heads get the next head's slot; they are never written
}

int launch_lm_rowmap(const ViewK& v, const GeomBufs& gb, const BinBufs& bb, const ImgBufs& ib, const ScratchBufs& sb,
                     int64_t N, hipStream_t s) {
  const int ntiles = v.gx * v.gy;
  if (N <= 0 || ntiles == 0) {
    GSLM_HIP_CHECK(hipMemsetAsync(sb.hscan, 0, sizeof(uint32_t), s));
    return GSLM_OK;
  }
  const unsigned nb = (unsigned)((N + 255) / 256);
  hipLaunchKernelGGL(k_tile_neff, dim3(ntiles), dim3(TILE_PIX), 0, s, v, ib.n_contrib, bb.tile_neff);
  // the masks refined before the costs and the head flags read them; in the launch order the binning (or an earlier
  // row map on it) left
  if (live_masks_on())
    hipLaunchKernelGGL(k_quad_live, dim3(ntiles), dim3(TILE_PIX), 0, s, v, bb.ranges, bb.tile_order, bb.tile_neff,
                       gb.rec, ib.n_contrib, bb.point_list);
  if (N + 1 >= ntiles) {
    // the LM tile passes' launch order by their modelled cost (hscan holds the costs until k_row_flags rewrites it;
    // only the schedule changes, every tile's results are independent of when it runs)
    hipLaunchKernelGGL(k_tile_cost, dim3(ntiles), dim3(256), 0, s, bb.ranges, bb.point_list, bb.tile_neff, sb.hscan);
    if (int st = launch_tile_order(ntiles, bb.ranges, bb.tile_order, sb.hscan, s)) return st;
  }
  hipLaunchKernelGGL(k_row_flags, dim3(nb), dim3(256), 0, s, N, v.gx, bb.keys_sorted, bb.point_list, bb.ranges,
                     bb.tile_neff, gb.goff, gb.rect, bb.slots, sb.hscan);
  GSLM_LAUNCH_CHECK();
  // in place (exclusive_scan_u32 picks k_scan_apply_inplace: no __restrict__ aliasing of in and out)
  const int st = exclusive_scan_u32(sb.hscan, nullptr, sb.hscan, N, sb.scan_tmp, sb.hscan + N, s);
  if (st) return st;
  hipLaunchKernelGGL(k_row_final, dim3(nb), dim3(256), 0, s, N, sb.hscan, bb.slots);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

// ---- the active list (gslm_active_list), once per geometry ----
// Gaussian i is active when it owns at least one head row of the LM row map: hscan[goff + tiles] > hscan[goff].
__device__ __forceinline__ uint32_t owns_head_row(int64_t i, const uint32_t* __restrict__ tiles,
                                                  const uint32_t* __restrict__ goff,
                                                  const uint32_t* __restrict__ hscan) {
  const uint32_t n = tiles[i];
  if (n == 0) return 0u;
  const uint32_t o = goff[i];
  return hscan[o + n] > hscan[o] ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_active_flags(int64_t P, const uint32_t* __restrict__ tiles,
                                                       const uint32_t* __restrict__ goff,
                                                       const uint32_t* __restrict__ hscan, uint32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < P) flags[i] = owns_head_row(i, tiles, goff, hscan);
}

// pos = the exclusive scan of the flags: ids[pos[i]] = i for the active i (ascending), *count = their number, and
// hrow[pos[i]] = the first head row of i, hrow[*count] = the number of head rows: the rows of list entry j are
// [hrow[j], hrow[j + 1]) -- the Gaussians between two listed ones own none -- so the list's gather reads its row
// offsets coalesced, without the goff -> hscan chain by id
__global__ __launch_bounds__(256) void k_active_scatter(int64_t P, int64_t N, const uint32_t* __restrict__ tiles,
                                                         const uint32_t* __restrict__ goff,
                                                         const uint32_t* __restrict__ hscan,
                                                         const uint32_t* __restrict__ pos,
                                                         const uint32_t* __restrict__ total, int32_t* __restrict__ ids,
                                                         uint32_t* __restrict__ hrow, int64_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    *count = (int64_t)*total;
    hrow[*total] = hscan[N];
  }
  if (i < P && owns_head_row(i, tiles, goff, hscan)) {
    ids[pos[i]] = (int32_t)i;
    hrow[pos[i]] = hscan[goff[i]];
  }
}

int launch_active_list(int64_t P, int64_t N, const GeomBufs& gb, const ScratchBufs& sb, uint32_t* flags,
                       uint32_t* scan_tmp, uint32_t* total, int32_t* ids, uint32_t* hrow, int64_t* count,
                       hipStream_t s) {
  if (P <= 0) {
    GSLM_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int64_t), s));
    GSLM_HIP_CHECK(hipMemsetAsync(hrow, 0, sizeof(uint32_t), s));
    return GSLM_OK;
  }
  const unsigned nb = (unsigned)((P + 255) / 256);
  hipLaunchKernelGGL(k_active_flags, dim3(nb), dim3(256), 0, s, P, gb.tiles, gb.goff, sb.hscan, flags);
  GSLM_LAUNCH_CHECK();
  // in place, as the row map's own scan
  const int st = exclusive_scan_u32(flags, nullptr, flags, P, scan_tmp, total, s);
  if (st) return st;
  hipLaunchKernelGGL(k_active_scatter, dim3(nb), dim3(256), 0, s, P, N, gb.tiles, gb.goff, sb.hscan, flags, total, ids,
                     hrow, count);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

// ---- the union list of a view batch (gslm_active_union), once per geometry ----
// Up to MAX_SCREEN_VIEWS views' row maps per launch; tiles NULL: the view rendered nothing (no row map exists).
// Every view's geometry has the layout of the same P, so goff and clampw lie at one offset from tiles in all of them.
struct UnionWsK {
  const uint32_t* tiles[MAX_SCREEN_VIEWS];
  const uint32_t* hscan[MAX_SCREEN_VIEWS];
  int64_t N[MAX_SCREEN_VIEWS];
  int32_t goff_off, clamp_off;  // in words, from tiles
  int n;
};

// flags[i] = [flags[i] |] (Gaussian i owns a head row in one of these views)
__global__ __launch_bounds__(256) void k_union_flags(int64_t P, UnionWsK ws, int first, uint32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  uint32_t f = first ? 0u : flags[i];
  for (int b = 0; b < ws.n && !f; ++b)
    if (ws.tiles[b]) f = owns_head_row(i, ws.tiles[b], ws.tiles[b] + ws.goff_off, ws.hscan[b]);
  flags[i] = f;
}

// pos = the exclusive scan of the union flags, so Gaussian i is listed when pos steps at i (pos[P] being *total):
// ids[pos[i]] = i, and for view b = view_base + k of this launch hrow[b][pos[i]] = hscan_b[goff_b[i]] -- the first
// head row of i in view b, or of the next Gaussian that has one: the Gaussians between two listed ones own no row in
// any view, so entry j's rows in view b are [hrow[b][j], hrow[b][j + 1]), empty when view b does not move it --
// hrow[b][*total] = view b's head rows, and aflags[b][pos[i]] = k_view_flags' word of i in view b.  A view without
// a row map gets zeros.  The launch with view_base 0 also writes ids and *count.
__global__ __launch_bounds__(256) void k_union_scatter(int64_t P, UnionWsK ws, int view_base,
                                                        const uint32_t* __restrict__ pos,
                                                        const uint32_t* __restrict__ total, int32_t* __restrict__ ids,
                                                        uint32_t* __restrict__ hrow, uint32_t* __restrict__ aflags,
                                                        int64_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t na = *total;
  if (i == 0) {
    if (view_base == 0) *count = (int64_t)na;
    for (int b = 0; b < ws.n; ++b)
      hrow[(int64_t)(view_base + b) * (P + 1) + na] = ws.tiles[b] ? ws.hscan[b][ws.N[b]] : 0u;
  }
  if (i >= P) return;
  const uint32_t j = pos[i];
  if ((i + 1 < P ? pos[i + 1] : na) == j) return;  // not listed
  if (view_base == 0) ids[j] = (int32_t)i;
  for (int b = 0; b < ws.n; ++b) {
    const uint32_t* __restrict__ tiles = ws.tiles[b];
    uint32_t h = 0u, f = 0u;
    if (tiles) {
      h = ws.hscan[b][(tiles + ws.goff_off)[i]];
      f = tiles[i] ? (0x80000000u | ((tiles + ws.clamp_off)[i] & 7u)) : 0u;
    }
    hrow[(int64_t)(view_base + b) * (P + 1) + j] = h;
    aflags[(int64_t)(view_base + b) * P + j] = f;
  }
}

int launch_active_union(const GeomBufs* gbs, const ScratchBufs* sbs, const int64_t* nr, int nviews, int64_t P,
                        uint32_t* flags, uint32_t* scan_tmp, uint32_t* total, int32_t* ids, uint32_t* hrow,
                        uint32_t* aflags, int64_t* count, hipStream_t s) {
  if (P <= 0) {
    GSLM_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int64_t), s));
    GSLM_HIP_CHECK(hipMemsetAsync(hrow, 0, (size_t)nviews * sizeof(uint32_t), s));  // [V][P + 1] with P = 0
    return GSLM_OK;
  }
  const unsigned nb = (unsigned)((P + 255) / 256);
  auto chunk = [&](int b0) {
    UnionWsK ws{};
    ws.n = nviews - b0 < MAX_SCREEN_VIEWS ? nviews - b0 : MAX_SCREEN_VIEWS;
    for (int k = 0; k < ws.n; ++k) {
      const int b = b0 + k;
      if (nr[b] <= 0) continue;  // tiles stays NULL
      ws.goff_off = (int32_t)(gbs[b].goff - gbs[b].tiles);
      ws.clamp_off = (int32_t)(gbs[b].clampw - gbs[b].tiles);
      ws.tiles[k] = gbs[b].tiles;
      ws.hscan[k] = sbs[b].hscan;
      ws.N[k] = nr[b];
    }
    return ws;
  };
  for (int b0 = 0; b0 < nviews; b0 += MAX_SCREEN_VIEWS) {
    hipLaunchKernelGGL(k_union_flags, dim3(nb), dim3(256), 0, s, P, chunk(b0), b0 == 0 ? 1 : 0, flags);
    GSLM_LAUNCH_CHECK();
  }
  // in place, as the row map's own scan
  const int st = exclusive_scan_u32(flags, nullptr, flags, P, scan_tmp, total, s);
  if (st) return st;
  for (int b0 = 0; b0 < nviews; b0 += MAX_SCREEN_VIEWS) {
    hipLaunchKernelGGL(k_union_scatter, dim3(nb), dim3(256), 0, s, P, chunk(b0), b0, flags, total, ids, hrow, aflags,
                       count);
    GSLM_LAUNCH_CHECK();
  }
  return GSLM_OK;
}

// ---- the line search's shared binning (gslm_union_*) ----
// The seven line-search points of train_jvp.py:262-280 differ only in the groups the LM step moves (xyz is masked,
// :221-227), so one view's Gaussians keep their screen centre and depth order at every point and only their
// footprints change.  Each point's exact point list -- the (tile, Gaussian) pairs of its rects in (tile, depth,
// index) order -- is then the subsequence of ONE list binned over the union of the points' rects: the entries whose
// tile lies in that point's rect.  k_duplicate_union gives every entry 4 bits per point: that point's quadrant mask
// (quad_mask of its own record, the bits its exact k_duplicate would write) where the tile is in its rect, 0
// elsewhere; the tile sort carries them with the pairs.  A blend that visits by those bits visits the exact list's
// entries, in its order, with the same records: the same image and loss, bitwise (gslm_rasterize_loss_slot).

// The union list is built in DEPTH SPACE: the sets' records sit at their Gaussians' depth positions s (gslm_preprocess_
// views with depth positions), so every pass below reads them coalesced in s and the point list's values are depth
// positions.  The blend indexes the set's records by them (the same records, the same (tile, depth, index) order).

// k_depth_positions: pos[order[s]] = s (the depth order's inverse)
__global__ __launch_bounds__(256) void k_depth_positions(int64_t P, const uint32_t* __restrict__ order,
                                                          uint32_t* __restrict__ pos) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < P) pos[order[s]] = (uint32_t)s;
}

// per depth position: the union of the sets' rects (a culled set's rect slot is zero), as the union geometry's tile
// count and rect
__global__ __launch_bounds__(256) void k_union_rect(int64_t P, UnionSets u, uint32_t* __restrict__ utiles,
                                                     uint2* __restrict__ urect) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  uint32_t x0 = 0xFFFFu, y0 = 0xFFFFu, x1 = 0u, y1 = 0u;
  for (int a = 0; a < u.n; ++a) {
    const float4 r3 = u.rec[a][RECS * i + 3];
    const uint32_t lo = __float_as_uint(r3.x), hi = __float_as_uint(r3.y);
    if (hi == 0u) continue;  // culled in set a
    x0 = min(x0, lo & 0xFFFFu);
    y0 = min(y0, lo >> 16);
    x1 = max(x1, hi & 0xFFFFu);
    y1 = max(y1, hi >> 16);
  }
  const bool any = x1 > x0 && y1 > y0;
  utiles[i] = any ? (x1 - x0) * (y1 - y0) : 0u;
  urect[i] = any ? make_uint2(x0 | (y0 << 16), x1 | (y1 << 16)) : make_uint2(0u, 0u);
}

// k_duplicate over the union rects in depth space (the same emission as k_duplicate: one block per DUPU_G depth
// positions, elements in order, a Gaussian's rect row-major), the value the depth position with quadrant bits 0xF,
// and amask[e] = bits 4a..4a+3 the quadrant mask of set a.  Each (Gaussian, set) quadrant test is prepared once
// (quad_cull_prep on the set's record, read coalesced in depth space) into LDS -- [ia b det ta] [ydom yr sqm mode]
// and the set's rect -- and every element evaluates quad_mask on it: the bits k_duplicate writes for that set's own
// list.  (Preparing per element was 6 square roots and 4 divisions per set and entry: 252 us per 1080p view at 1M,
// 5x the plain k_duplicate.)  The centre is the same in every set that keeps the Gaussian (the points share xyz and
// the view), so its copy in s_gxy is written by each such set with the same bits.  Quarter-size blocks keep the
// staging at NS * 2.5 KB of LDS (dynamic: NS * 2 * DUPU_G float4); DUPU_SPLIT threads share a Gaussian's sets.
#ifndef GSLM_DUPU_G
#define GSLM_DUPU_G 64  // 64: 15 KB of staging at six sets, 8 blocks per CU (union binning 0.290 -> 0.272 ms against 128)
#endif
constexpr int DUPU_G = GSLM_DUPU_G;
constexpr int DUPU_SPLIT = 256 / DUPU_G;  // threads per Gaussian in the staging
template <int NS>
__global__ __launch_bounds__(256) void k_duplicate_union(int64_t P, int gx, const uint32_t* __restrict__ offsets,
                                                          uint32_t N, const uint2* __restrict__ urect, UnionSets u,
                                                          uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                          uint32_t* __restrict__ amask, uint2* __restrict__ zero_ranges,
                                                          int ntiles) {
  extern __shared__ float4 s_set[];  // [NS][2][DUPU_G]
  zero_tile_ranges(zero_ranges, ntiles);
  __shared__ uint2 s_srect[NS][DUPU_G];
  __shared__ float2 s_gxy[DUPU_G];
  __shared__ uint32_t s_off[DUPU_G + 1];
  __shared__ uint32_t s_rc[DUPU_G][3];  // x0, y0, width of the union rect
  const int tid = threadIdx.x, gi = tid & (DUPU_G - 1), half = tid / DUPU_G;
  const int64_t s0 = (int64_t)blockIdx.x * DUPU_G, s = s0 + gi;
  const int64_t slast = min(s0 + DUPU_G - 1, P - 1);
  const uint32_t base = offsets[s0];
  uint32_t n = 0;
  if (s < P) {
    const uint32_t o = offsets[s];
    n = (s + 1 < P ? offsets[s + 1] : N) - o;
    if (half == 0) {
      s_off[gi] = o - base;
      if (n) {
        const uint2 rc = urect[s];
        const int x0 = rc.x & 0xFFFF, y0 = rc.x >> 16, x1 = rc.y & 0xFFFF;
        s_rc[gi][0] = (uint32_t)x0;
        s_rc[gi][1] = (uint32_t)y0;
        s_rc[gi][2] = (uint32_t)(x1 - x0);
      }
    }
    if (n) {
#pragma unroll
      for (int k = 0; k < (NS + DUPU_SPLIT - 1) / DUPU_SPLIT; ++k) {
        const int a = DUPU_SPLIT * k + half;
        if (a >= NS) break;
        const float4* r = u.rec[a] + RECS * (size_t)s;
        const float4 r0 = r[0], r3 = r[3];
        const float r1x = r[1].x, r2w = r[2].w;
        const uint2 rc = make_uint2(__float_as_uint(r3.x), __float_as_uint(r3.y));
        s_srect[a][gi] = rc;  // zero when set a culls the Gaussian (its other record fields are stale: unused)
        if (rc.y != 0u) {
          const QuadCull q = quad_cull_prep(r0.x, r0.y, r0.z, r0.w, r1x, r2w);
          s_set[(2 * a) * DUPU_G + gi] = make_float4(q.ia, q.b, q.det, q.ta);
          s_set[(2 * a + 1) * DUPU_G + gi] = make_float4(q.ydom, q.yr, q.sqm, __int_as_float(q.mode));
          s_gxy[gi] = make_float2(r0.x, r0.y);
        }
      }
    }
  } else if (half == 0) {
    s_off[gi] = 0xFFFFFFFFu;  // past the block's last Gaussian: never an owner
  }
  if (s == slast && half == 0) s_off[DUPU_G] = offsets[s] - base + n;
  __syncthreads();
  const uint32_t total = base < N ? min(s_off[DUPU_G], N - base) : 0u;
  for (uint32_t e = tid; e < total; e += 256) {
    int lo = 0;
#pragma unroll
    for (int step = DUPU_G / 2; step > 0; step >>= 1) lo = s_off[lo + step] <= e ? lo + step : lo;
    const uint32_t li = e - s_off[lo];
    const uint32_t w = s_rc[lo][2];
    const uint32_t dy = li / w;
    const int tx = (int)(s_rc[lo][0] + (li - dy * w)), ty = (int)(s_rc[lo][1] + dy);
    const float2 gxy = s_gxy[lo];
    uint32_t m = 0u;
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      const uint2 rc = s_srect[a][lo];
      if (tx < (int)(rc.x & 0xFFFFu) || ty < (int)(rc.x >> 16) || tx >= (int)(rc.y & 0xFFFFu) || ty >= (int)(rc.y >> 16))
        continue;  // outside set a's rect (an empty rect when set a culls the Gaussian)
      const float4 qa = s_set[(2 * a) * DUPU_G + lo], qb = s_set[(2 * a + 1) * DUPU_G + lo];
      QuadCull q;
      q.gx = gxy.x;
      q.gy = gxy.y;
      q.ia = qa.x;
      q.b = qa.y;
      q.det = qa.z;
      q.ta = qa.w;
      q.ydom = qb.x;
      q.yr = qb.y;
      q.sqm = qb.z;
      q.mode = __float_as_int(qb.w);
      m |= quad_mask(q, tx, ty) << (4 * a);
    }
    keys[base + e] = (uint32_t)(ty * gx + tx);
    vals[base + e] = (uint32_t)(s0 + lo) | (0xFu << ID_BITS);
    amask[base + e] = m;
  }
}

int launch_depth_positions(int64_t P, const uint32_t* order, uint32_t* pos, hipStream_t s) {
  if (P <= 0) return GSLM_OK;
  hipLaunchKernelGGL(k_depth_positions, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, order, pos);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

int launch_union_rect(int64_t P, const UnionSets& u, const GeomBufs& ug, hipStream_t s) {
  if (P <= 0) return GSLM_OK;
  hipLaunchKernelGGL(k_union_rect, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, u, ug.tiles, ug.rect);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

int launch_union_binning(const ViewK& v, int64_t P, const GeomBufs& ug, const BinBufs& bb, const UnionMasks& um,
                         int64_t N, const UnionSets& u, hipStream_t s) {
  const int ntiles = v.gx * v.gy;
  if (P == 0 || N == 0) GSLM_HIP_CHECK(hipMemsetAsync(bb.ranges, 0, (size_t)ntiles * sizeof(uint2), s));
  if (P > 0 && N > 0) {  // (k_duplicate_union also zeroes the tile ranges)
    const size_t lds = (size_t)u.n * 2 * DUPU_G * sizeof(float4);
    const dim3 grid((unsigned)((P + DUPU_G - 1) / DUPU_G));
    switch (u.n) {
#define GSLM_DUP_UNION(NS)                                                                                         \
  case NS:                                                                                                         \
    hipLaunchKernelGGL(k_duplicate_union<NS>, grid, dim3(256), lds, s, P, v.gx, ug.offsets, (uint32_t)N, ug.rect, u, \
                       bb.keys0, bb.vals0, um.m0, bb.ranges, ntiles);                                                \
    break;
      GSLM_DUP_UNION(1) GSLM_DUP_UNION(2) GSLM_DUP_UNION(3) GSLM_DUP_UNION(4)
      GSLM_DUP_UNION(5) GSLM_DUP_UNION(6) GSLM_DUP_UNION(7) GSLM_DUP_UNION(8)
#undef GSLM_DUP_UNION
      default:
        set_error("union binning: 1..8 parameter sets");
        return GSLM_ERR_INVALID;
    }
    GSLM_LAUNCH_CHECK();
    bool alt = false;
    int st = radix_sort_pairs(bb.keys0, bb.vals0, bb.keys1, bb.vals1, N, bb.end_bit, um.hist, &alt, s, false, nullptr,
                              nullptr, um.m0, um.m1);
    if (st != GSLM_OK) return st;
    if ((alt ? bb.vals1 : bb.vals0) != bb.point_list || (alt ? um.m1 : um.m0) != um.sorted) {
      set_error("internal: radix pass count disagrees with the union binning layout");
      return GSLM_ERR_INVALID;
    }
    if ((st = launch_ranges(N, bb.keys_sorted, bb.ranges, nullptr, nullptr, s))) return st;
  }
  if (int st = launch_tile_order(ntiles, bb.ranges, bb.tile_order, nullptr, s)) return st;
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

// ------------------------------------------------------------------ launchers

// The SH rows staged through LDS wherever stage_lead allows: the contiguous [P, M-1, 3] rest leaf (raw GaussianModel
// tensors, or the dc / rest pair of render(separate_sh=True)), or the rest inside upstream's [P, M, 3] features tensor
// (render()'s get_features: each rest row 3 floats past its dc at one 3M stride) -- whole rows staged from the dc slot.
template <bool RAW>
static void launch_preprocess_raw(const ViewK& v, const GaussK& g, const PreOutBufs& ob, int* radii_out, hipStream_t s) {
  const dim3 grid((unsigned)((g.P + 255) / 256));
  const int lead = stage_lead(g);
  if (lead >= 0)
    hipLaunchKernelGGL((k_preprocess_dma<RAW>), grid, dim3(256), (size_t)256 * g.rest_stride * sizeof(float), s, v, g, ob,
                       radii_out, lead);
  else
    hipLaunchKernelGGL((k_preprocess<RAW>), grid, dim3(256), 0, s, v, g, ob, radii_out);
}

int launch_preprocess(const ViewK& v, const GaussK& g, const PreOutBufs& ob, int* radii_out, hipStream_t s) {
  if (g.P == 0) return GSLM_OK;
  if (g.raw) launch_preprocess_raw<true>(v, g, ob, radii_out, s);
  else launch_preprocess_raw<false>(v, g, ob, radii_out, s);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

int launch_binning(const ViewK& v, int64_t P, const GeomBufs& gb, const BinBufs& bb, int64_t N, hipStream_t s,
                   bool device_count, uint32_t* n_out) {
  const int ntiles = v.gx * v.gy;
  // device_count: N is the list capacity, the pair count stays on the device (gb.counters[0])
  const uint32_t* n_dev = device_count ? gb.counters : nullptr;
  if (P > 0)  // (k_duplicate also zeroes the tile ranges)
    hipLaunchKernelGGL(k_duplicate, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, v.gx, gb.sorted_idx,
                       gb.offsets, (uint32_t)N, n_dev, gb.rect, gb.rec, bb.keys0, bb.vals0, bb.ranges, ntiles);
  else
    GSLM_HIP_CHECK(hipMemsetAsync(bb.ranges, 0, (size_t)ntiles * sizeof(uint2), s));
  GSLM_LAUNCH_CHECK();
  if (N == 0) {  // every range stays [0, 0); the tile passes still read a launch order
    if (n_out) {
      if (P > 0) GSLM_HIP_CHECK(hipMemcpyAsync(n_out, gb.counters, 4, hipMemcpyDeviceToDevice, s));
      else GSLM_HIP_CHECK(hipMemsetAsync(n_out, 0, 4, s));
    }
    if (int st = launch_tile_order(ntiles, bb.ranges, bb.tile_order, nullptr, s)) return st;
    GSLM_LAUNCH_CHECK();
    return GSLM_OK;
  }
  bool alt = false;
  int st = radix_sort_pairs(bb.keys0, bb.vals0, bb.keys1, bb.vals1, N, bb.end_bit, bb.hist, &alt, s, false, nullptr,
                            n_dev);
  if (st != GSLM_OK) return st;
  if ((alt ? bb.vals1 : bb.vals0) != bb.point_list) {
    set_error("internal: radix pass count disagrees with the binning layout");
    return GSLM_ERR_INVALID;
  }
  if ((st = launch_ranges(N, bb.keys_sorted, bb.ranges, n_dev, n_out, s))) return st;
  if (int st = launch_tile_order(ntiles, bb.ranges, bb.tile_order, nullptr, s)) return st;
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

int launch_point_ids(const uint32_t* point_list, int64_t N, uint32_t* out, hipStream_t s) {
  if (N <= 0) return GSLM_OK;
  hipLaunchKernelGGL(k_point_ids, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, N, point_list, out);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

}  // namespace gslm
