// tangent.hip -- per-Gaussian side of the forward-mode tangent.
//
//   k_preprocess_jvp   one thread per visible Gaussian: tangent render record (48 B) from the
//                      input tangents (chain_jvp, exact transpose of chain_vjp); optionally first
//                      the deferred CG direction update p = s + beta p of its block (block_xpby).
// Compiled apart from the tile passes: these per-Gaussian kernels keep clang's SLP vectoriser,
// which the tile passes turn off (Makefile).
#include "gslm_tile.hpp"
#include "gslm_chain.hpp"

namespace gslm {

// p = s + beta p over this block's 256 Gaussians' slices of every group, and the flat tail by block 0.
// Same arithmetic as k_xpby_dev (bitwise).  The narrow groups (xyz, dc, scaling, rotation, opacity, and the
// SH rest when projected: <= 4 floats per Gaussian, so <= 4 elements per thread each) are loaded in one pass --
// every s / p / x load of the block in flight before the first store -- instead of one latency per group; a
// full-layout SH rest (3(M-1) floats per Gaussian) streams in its own loop.
__device__ __forceinline__ void block_xpby(const XpbyK& xp, int64_t P, float* s_rest) {
  // beta's numerator may still be the update kernel's block partials (XpbyK::num_part; load_scalar)
  __shared__ double s_fin[DOT_THREADS / 64 + 1];
  const float b = (float)(load_scalar(ScalarK{xp.num, xp.num_part, xp.num_np, xp.num_store}, s_fin) / (*xp.den));
  const bool with_x = xp.anum != nullptr;
  const float a = with_x ? (float)((*xp.anum) / (*xp.aden)) : 0.f;  // gslm_cg_update's alpha, bitwise
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x;
  const int64_t nv = min((int64_t)blockDim.x, P - i0);
  const int tid = threadIdx.x;
  constexpr int MAXW[6] = {3, 3, 3, 3, 4, 1};  // per-Gaussian widths the one-pass path covers
  const bool rest_narrow = xp.w[2] <= 3;
  float sv[17], pv[17], xv[17];
  int n = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int j = 0; j < MAXW[k]; ++j, ++n) {
      const int64_t e = (int64_t)j * blockDim.x + tid;
      const bool on = xp.p[k] && (k != 2 || rest_narrow) && e < nv * xp.w[k];
      const int64_t gi = i0 * xp.w[k] + e;
      sv[n] = on ? xp.s[k][gi] : 0.f;
      pv[n] = on ? xp.p[k][gi] : 0.f;
      xv[n] = (on && with_x) ? xp.p[k][xp.xoff + gi] : 0.f;
    }
  }
  n = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int j = 0; j < MAXW[k]; ++j, ++n) {
      const int64_t e = (int64_t)j * blockDim.x + tid;
      const bool on = xp.p[k] && (k != 2 || rest_narrow) && e < nv * xp.w[k];
      if (on) {
        const int64_t gi = i0 * xp.w[k] + e;
        if (with_x) xp.p[k][xp.xoff + gi] = xv[n] + a * pv[n];
        const float r = sv[n] + b * pv[n];
        xp.p[k][gi] = r;
        if (k == 2) s_rest[e] = r;  // the SH-rest slice stays in LDS for the tangent below
      }
    }
  }
  if (xp.p[2] && !rest_narrow) {
    float* p = xp.p[2] + i0 * xp.w[2];
    const float* s = xp.s[2] + i0 * xp.w[2];
    const int64_t len = nv * xp.w[2];
    constexpr int U = 8;
    for (int64_t e0 = 0; e0 < len; e0 += (int64_t)U * blockDim.x) {
      float su[U], pu[U], xu[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t e = e0 + (int64_t)u * blockDim.x + tid;
        su[u] = e < len ? s[e] : 0.f;
        pu[u] = e < len ? p[e] : 0.f;
        xu[u] = (e < len && with_x) ? p[xp.xoff + e] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t e = e0 + (int64_t)u * blockDim.x + tid;
        if (e < len) {
          if (with_x) p[xp.xoff + e] = xu[u] + a * pu[u];
          const float r = su[u] + b * pu[u];
          p[e] = r;
          s_rest[e] = r;
        }
      }
    }
  }
  if (blockIdx.x == 0 && xp.tail_p)
    for (int64_t e = threadIdx.x; e < xp.tail_n; e += blockDim.x) {
      const float pvt = xp.tail_p[e];
      if (with_x) xp.tail_p[xp.xoff + e] = xp.tail_p[xp.xoff + e] + a * pvt;
      xp.tail_p[e] = xp.tail_s[e] + b * pvt;
    }
}

// Tangent render record of Gaussian i: 12 floats [dx dy da db | dc dop dr dg | db dinv 0 0] (3 float4), or for
// the LM rows (xyz frozen, no inverse-depth term; `compact`) 8 floats [da db dc dop | dr dg db 0] (2 float4).
__device__ __forceinline__ void store_trec(float4* __restrict__ out, int64_t i, const float T2[10], bool compact) {
  if (compact) {
    out[2 * i + 0] = make_float4(T2[2], T2[3], T2[4], T2[5]);
    out[2 * i + 1] = make_float4(T2[6], T2[7], T2[8], 0.f);
  } else {
    out[3 * i + 0] = make_float4(T2[0], T2[1], T2[2], T2[3]);
    out[3 * i + 1] = make_float4(T2[4], T2[5], T2[6], T2[7]);
    out[3 * i + 2] = make_float4(T2[8], T2[9], 0.f, 0.f);
  }
}

// ACTIVE (gslm_matvec_view_active): thread j handles Gaussian ids[j] of the scene (parameters, clamp word, tile
// count, tangent record) and row j of the tangent's groups and of the fused direction update, which hold the na
// listed Gaussians only.  Same arithmetic per Gaussian as the full-layout kernel.  With clamp_list the parameters
// and the clamp word are read from row j of the list-order copy (gslm_active_params) instead of row ids[j].
template <bool RAW, bool XPBY, bool ACTIVE = false>
__global__ __launch_bounds__(256) void k_preprocess_jvp(ViewK v, GaussK g, GaussK t, const float* __restrict__ m2t,
                                                         const uint32_t* __restrict__ clampw,
                                                         const uint32_t* __restrict__ tiles,
                                                         float4* __restrict__ trec, XpbyK xp, int compact,
                                                         int lead, const int32_t* __restrict__ ids, int64_t na,
                                                         const uint32_t* __restrict__ clamp_list) {
  extern __shared__ __attribute__((aligned(16))) float s_rest[];  // XPBY: [256 * 3(M-1)]; lead >= 0: [256 * rest_stride]
  if (cg_stopped(v)) return;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = ACTIVE ? na : g.P;  // rows of the tangent's groups
  if (!XPBY && !ACTIVE && lead >= 0) {
    // the drop-in JVP: the block's primal SH rows through LDS (per-thread reads at a 3M-float stride touch a line
    // per lane per load; stage_lead)
    stage_sh_rows(g, lead, s_rest);
  }
  if (XPBY) {
    // the direction this kernel reads is the updated one: each thread reads back only its own
    // Gaussian's elements, all written by this block before the barrier; its SH-rest tangent (the
    // bulk of them, 3(M-1) floats at a 180-B stride) from the LDS copy instead of memory
    block_xpby(xp, n, s_rest);
    __syncthreads();
    if (t.rest) {
      t.rest = s_rest;
      t.rest_base = (int64_t)blockIdx.x * blockDim.x;
    }
  }
  if (j >= n) return;
  const int64_t i = ACTIVE ? (int64_t)ids[j] : j;
  if (!ACTIVE && tiles[i] == 0) return;  // never gathered by the render passes (a listed Gaussian always is)
  float T2[10];
  // clamp_list (gslm_active_params): g's parameter arrays and the clamp words are the list's own, row j
  const bool listed = ACTIVE && clamp_list != nullptr;
  chain_jvp<RAW>(v, g, t, m2t, listed ? j : i, j, listed ? clamp_list[j] : clampw[i], T2);
  store_trec(trec, i, T2, compact != 0);
}

// ------------------------------------------------------------------ launcher
int launch_tangent_pre(const ViewK& v, const GaussK& g, const GaussK& t, const float* m2t, const GeomBufs& gb,
                       const ScratchBufs& sb, const XpbyK* xp, hipStream_t s, bool compact, const int32_t* ids,
                       int64_t na, const uint32_t* clamp_list) {
  const bool active = na >= 0;
  const int64_t n = active ? na : g.P;
  // no rows with a fused direction update: one block still applies the flat tail's update (block_xpby)
  if (n == 0 && !(xp && xp->tail_p)) return GSLM_OK;
  const unsigned nb = (unsigned)((n + 255) / 256) + (n == 0 ? 1u : 0u);
  XpbyK none{};
  const XpbyK& x = xp ? *xp : none;
  // (this and the xp check below guard the launcher's own contract: the C entry points' plan -- api.hip plan_matvec,
  // build_xpby -- has checked both, so neither is reachable from the C ABI)
  if (active && (!g.raw || m2t || (na > 0 && !ids))) {
    set_error("internal: the active-list tangent runs on raw leaves without a means2D tangent");
    return GSLM_ERR_INVALID;
  }
  if (xp) {
    if (t.rest && (t.rest != xp->p[2] || t.rest_stride != xp->w[2])) {
      set_error("internal: fused xpby expects the tangent's SH-rest group to be p's");
      return GSLM_ERR_INVALID;
    }
    const size_t lds = (size_t)256 * xp->w[2] * sizeof(float);
    if (active)
      hipLaunchKernelGGL((k_preprocess_jvp<true, true, true>), dim3(nb), dim3(256), lds, s, v, g, t, m2t, gb.clampw,
                         gb.tiles, sb.trec, x, compact ? 1 : 0, -1, ids, na, clamp_list);
    else if (g.raw)
      hipLaunchKernelGGL((k_preprocess_jvp<true, true>), dim3(nb), dim3(256), lds, s, v, g, t, m2t, gb.clampw, gb.tiles,
                         sb.trec, x, compact ? 1 : 0, -1, nullptr, -1, nullptr);
    else
      hipLaunchKernelGGL((k_preprocess_jvp<false, true>), dim3(nb), dim3(256), lds, s, v, g, t, m2t, gb.clampw, gb.tiles,
                         sb.trec, x, compact ? 1 : 0, -1, nullptr, -1, nullptr);
  } else if (active) {
    hipLaunchKernelGGL((k_preprocess_jvp<true, false, true>), dim3(nb), dim3(256), 0, s, v, g, t, m2t, gb.clampw,
                       gb.tiles, sb.trec, x, compact ? 1 : 0, -1, ids, na, clamp_list);
  } else {
    const int lead = g.P > 0 ? stage_lead(g) : -1;
    const size_t lds = lead >= 0 ? (size_t)256 * g.rest_stride * sizeof(float) : 0;
    if (g.raw)
      hipLaunchKernelGGL((k_preprocess_jvp<true, false>), dim3(nb), dim3(256), lds, s, v, g, t, m2t, gb.clampw, gb.tiles,
                         sb.trec, x, compact ? 1 : 0, lead, nullptr, -1, nullptr);
    else
      hipLaunchKernelGGL((k_preprocess_jvp<false, false>), dim3(nb), dim3(256), lds, s, v, g, t, m2t, gb.clampw, gb.tiles,
                         sb.trec, x, compact ? 1 : 0, lead, nullptr, -1, nullptr);
  }
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

// Gaussian-sharded exchange: the tangent render records of a Gaussian range for several views (the
// TANGENT stage of k_preprocess_jvp, looped over views), after the optional fused direction update.
// The block's SH-rest tangent slice is staged in LDS once and read by every view's chain.
// ACTIVE (gslm_tangent_views_active): thread j handles Gaussian ids[j] of the scene (parameters, the factor R, the
// tangent record) and row j of the tangent's groups, of the fused direction update and of the views' flag words
// (vflags is then the union list's aflags: [view][row]), which hold the na listed Gaussians only.  Same arithmetic
// per Gaussian as the full-layout kernel; the records land in row ids[j] of the views' [P][8] tables.
template <bool XPBY, bool ACTIVE = false>
__global__ __launch_bounds__(256) void k_tangent_views(ViewsK vs, GaussK g, GaussK t, const uint32_t* __restrict__ vflags,
                                                        int64_t fstride, float4* __restrict__ out, int64_t ostride,
                                                        XpbyK xp, int compact, int view_base,
                                                        const int32_t* __restrict__ ids, int64_t na) {
  extern __shared__ __attribute__((aligned(16))) float s_rest[];  // [256 * 3(M-1)]
  if (cg_stopped(vs.v[0])) return;  // a stopped solve (gslm_matvec_opts.cg_ctl): block-uniform, before any barrier
  const int64_t n = ACTIVE ? na : g.P;  // rows of the tangent's groups
  const int64_t j0 = (int64_t)blockIdx.x * blockDim.x;
  const int64_t j = j0 + threadIdx.x;
  if (XPBY) {
    block_xpby(xp, n, s_rest);
  } else if (t.rest) {
    const int64_t len = min((int64_t)blockDim.x, n - j0) * t.rest_stride;
    const float* src = t.rest + j0 * t.rest_stride;
    for (int64_t e = threadIdx.x; e < len; e += blockDim.x) s_rest[e] = src[e];
  }
  __syncthreads();
  if (t.rest) {
    t.rest = s_rest;
    t.rest_base = j0;
  }
  if (j >= n) return;
  const int64_t i = ACTIVE ? (int64_t)ids[j] : j;
#pragma unroll 1
  for (int b = 0; b < vs.n; ++b) {
    const uint32_t f = vflags[(int64_t)b * fstride + j];
    if (!(f >> 31)) continue;
    t.rest_col = view_base + b;  // SH-rest coordinates: this view's column of R
    float T2[10];
    chain_jvp<true>(vs.v[b], g, t, nullptr, i, j, f & 7u, T2);
    store_trec(out, (int64_t)b * ostride + i, T2, compact != 0);
  }
}

int launch_tangent_views(const ViewK* views, int nviews, const GaussK& g, const GaussK& t, const uint32_t* vflags,
                         int64_t fstride, float* out, int64_t ostride, const XpbyK* xp, hipStream_t s, bool compact,
                         int view_base, const int32_t* ids, int64_t na) {
  if (nviews < 1 || nviews > MAX_SCREEN_VIEWS) {
    set_error("tangent_views: 1..16 views per call");
    return GSLM_ERR_INVALID;
  }
  const bool active = na >= 0;
  const int64_t n = active ? na : g.P;
  if (n == 0 && !(xp && xp->tail_p)) return GSLM_OK;  // an empty shard with a tail: one block updates it
  // (the two internal checks guard the launcher's own contract: tangent_views and build_xpby in api.hip have checked
  // both, so neither is reachable from the C ABI)
  if (xp && t.rest && (t.rest != xp->p[2] || t.rest_stride != xp->w[2])) {
    set_error("internal: fused xpby expects the tangent's SH-rest group to be p's");
    return GSLM_ERR_INVALID;
  }
  if (active && na > 0 && !ids) {
    set_error("internal: the active-list tangent needs the list");
    return GSLM_ERR_INVALID;
  }
  ViewsK vs;
  for (int b = 0; b < nviews; ++b) vs.v[b] = views[b];
  vs.n = nviews;
  const unsigned nb = (unsigned)((n + 255) / 256) + (n == 0 ? 1u : 0u);
  const size_t lds = t.rest ? (size_t)256 * t.rest_stride * sizeof(float) : 0;
  XpbyK none{};
  float4* o = reinterpret_cast<float4*>(out);
  if (active && xp)
    hipLaunchKernelGGL((k_tangent_views<true, true>), dim3(nb), dim3(256), lds, s, vs, g, t, vflags, fstride, o, ostride,
                       *xp, compact ? 1 : 0, view_base, ids, na);
  else if (active)
    hipLaunchKernelGGL((k_tangent_views<false, true>), dim3(nb), dim3(256), lds, s, vs, g, t, vflags, fstride, o, ostride,
                       none, compact ? 1 : 0, view_base, ids, na);
  else if (xp)
    hipLaunchKernelGGL(k_tangent_views<true>, dim3(nb), dim3(256), lds, s, vs, g, t, vflags, fstride, o, ostride, *xp,
                       compact ? 1 : 0, view_base, nullptr, -1);
  else
    hipLaunchKernelGGL(k_tangent_views<false>, dim3(nb), dim3(256), lds, s, vs, g, t, vflags, fstride, o, ostride, none,
                       compact ? 1 : 0, view_base, nullptr, -1);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

}  // namespace gslm
