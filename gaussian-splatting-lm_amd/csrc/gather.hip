// gather.hip -- per-Gaussian side of the VJP: row sums and the chain rule to the parameters.
//
//   k_preprocess_bwd   one block per 256 consecutive Gaussians: sums their contiguous rows and
//                      chains the screen-space gradient to means3D / scales / rotations / SH /
//                      opacity (or to cov3D_precomp / colors_precomp), fusing the activation
//                      derivatives when the inputs are raw GaussianModel leaves (drop-in backward).
//   k_gather_lm        the LM specialisation (raw leaves, SH colours): writes the flat param-space
//                      vector directly, overwrite or accumulate, with the damping term D v fused in,
//                      SH-rest stores staged through LDS so every store instruction is a contiguous
//                      256-B wave segment.
// Compiled apart from the tile passes: these keep clang's SLP vectoriser (Makefile).
#include "gslm_tile.hpp"
#include "gslm_chain.hpp"
#include "gslm_gather.hpp"

namespace gslm {

template <int ROWF4>
__device__ __forceinline__ void sum_rows(const float4* __restrict__ rows, uint32_t off, uint32_t n, float G2[NV]) {
#pragma unroll
  for (int q = 0; q < NV; ++q) G2[q] = 0.f;
  for (uint32_t t = 0; t < n; ++t) {
    float r[NV];
    load_row<ROWF4>(rows, (size_t)off + t, r);
#pragma unroll
    for (int q = 0; q < NV; ++q) G2[q] += r[q];
  }
}

// Drop-in backward, one block per 256 consecutive Gaussians: block-cooperative row sums (their rows
// are one contiguous range), the chain rule per thread, and the SH gradient -- 3M floats per Gaussian,
// the bulk of the output -- staged through LDS and stored as contiguous wave segments (per-thread
// stores at a 3M-float stride would touch a cache line per lane per store).
template <bool RAW>
__global__ __launch_bounds__(256) void k_preprocess_bwd(ViewK v, GaussK g, const uint32_t* __restrict__ clampw,
                                                         const uint32_t* __restrict__ tiles,
                                                         const uint32_t* __restrict__ goff,
                                                         const float4* __restrict__ rows, GradK out, int want_means) {
  extern __shared__ __attribute__((aligned(16))) float s_buf[];  // row chunks, then the factored SH stage
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x;
  const int64_t i = i0 + tid;
  const int64_t nvalid = min((int64_t)blockDim.x, g.P - i0);
  const uint32_t n = i < g.P ? tiles[i] : 0u;
  float G2[NV];
  {
    const int64_t il = i0 + nvalid - 1;
    const uint32_t R0 = goff[i0], R1 = goff[il] + tiles[il];
    block_sum_rows<3>(rows, R0, R1, i < g.P ? goff[i] : R1, n, reinterpret_cast<float4*>(s_buf), G2);
  }
  const int nc = (v.D + 1) * (v.D + 1);
  const bool sh_out = !g.colors && (out.dc || out.rest);
  // the SH colour's view-direction term of the means gradient needs <dres, sh_k> for every coefficient: per thread at a
  // 3M-float stride each of those 3(nc - 1) loads touches a line per lane, so it is formed block-cooperatively below
  // from coalesced reads of the block's SH rows (DEFER_DIR; block-uniform)
  const bool dir_term = want_means && out.means3D && !g.colors && v.D > 0;
  ChainOut co;
  if (i < g.P) {
    chain_vjp<RAW, true>(v, g, i, n != 0, n ? clampw[i] : 0u, G2, want_means != 0, co);
    write_grads(g, out, i, co, v.M, nc, want_means != 0 && !dir_term, /*skip_sh=*/true);
  }
  if (!sh_out && !dir_term) return;  // block-uniform
  // factored staging (gslm_gather.hpp): dsh[k][ch] = shB[k] dres[ch]
  float* s_d = s_buf + 256 * SHB_STRIDE;
  float* s_w = s_d + 256 * 4;  // [256][SHB_STRIDE]: <dres, sh_k> of the block's Gaussians
  if (i < g.P) {
#pragma unroll
    for (int k = 0; k < 16; ++k) s_buf[tid * SHB_STRIDE + k] = co.shB[k];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s_d[tid * 4 + ch] = co.dres[ch];
  }
  __syncthreads();
  if (dir_term) {
    // element e = (Gaussian ii, coefficient k): 64 lanes read 4 Gaussians' consecutive 48-float rows
    for (int e = tid; e < (int)nvalid * 16; e += blockDim.x) {
      const int ii = e >> 4, k = e & 15;
      float w = 0.f;
      if (k >= 1 && k < nc) {
        const int64_t gi = i0 + ii;
        const float s0 = g.sh(gi, k, 0), s1 = g.sh(gi, k, 1), s2 = g.sh(gi, k, 2);
        w = s_d[ii * 4 + 0] * s0 + s_d[ii * 4 + 1] * s1 + s_d[ii * 4 + 2] * s2;  // chain_vjp's w, bitwise
      }
      s_w[ii * SHB_STRIDE + k] = w;
    }
    __syncthreads();
    if (i < g.P && n != 0) {
      float dm[3] = {co.dmean[0], co.dmean[1], co.dmean[2]};
      add_dir_term(v.D, co.dir, co.dirlen, s_w + tid * SHB_STRIDE, dm);
#pragma unroll
      for (int k = 0; k < 3; ++k) put(&out.means3D[3 * i + k], dm[k], out.accumulate);
    } else if (i < g.P) {
#pragma unroll
      for (int k = 0; k < 3; ++k) put(&out.means3D[3 * i + k], co.dmean[k], out.accumulate);
    }
  }
  if (!sh_out) return;
  const int acc = out.accumulate;
  const int R = 3 * v.M;
  const float invR = 1.0f / (float)R;
  for (int e = tid; e < (int)nvalid * R; e += blockDim.x) {
    const int ii = (int)(((float)e + 0.5f) * invR);  // exact: e < 256 R (see lm_epilogue)
    const int r = e - ii * R, k = r / 3, ch = r - 3 * k;
    const float val = k < nc ? s_buf[ii * SHB_STRIDE + k] * s_d[ii * 4 + ch] : 0.f;
    const int64_t gi = i0 + ii;
    if (k == 0) {
      if (out.dc) put(&out.dc[gi * out.dc_stride + ch], val, acc);
    } else if (out.rest) {
      put(&out.rest[gi * out.rest_stride + 3 * (k - 1) + ch], val, acc);
    }
  }
}

// PROJ: the projected SH-rest layout (FlatK::rest_proj) as a compile-time fact, which drops the full layout's
// SH-rest epilogue from the code: at 5 waves per SIMD (96 VGPRs) over the 4 the unconstrained register count
// allows it runs 76 -> 71 us at 1M (the kernel is latency-bound: row sums, then the parameters, then the
// vector groups).  The full-layout variant keeps the compiler's register count: forced to 96 VGPRs its SH-rest
// epilogue spills and takes 0.18 -> 0.31 ms.
// ACTIVE (gslm_matvec_view_active): thread j handles Gaussian ids[j] of the scene (parameters, clamp word, tile
// count) and row j of v and y, which hold the na listed Gaussians only.  The head rows of a block's 256 consecutive
// listed Gaussians are still one contiguous range -- the Gaussians between them own none -- so the row sums and
// their order are those of the full-layout kernel; their offsets come from the list's own hrow, read coalesced.
// DVEC (GSLM_MV_DAMP_VEC): D v with d read per element from dk (lm_epilogue); the other instantiations take an empty
// struct there and keep their code.
template <bool WANT_MEANS, int ROWF4, bool PROJ, bool ACTIVE = false, bool DVEC = false>
__global__ __launch_bounds__(256, PROJ ? 5 : 1) void k_gather_lm(ViewK v, GaussK g, const uint32_t* __restrict__ clampw,
                                                    const uint32_t* __restrict__ tiles,
                                                    const uint32_t* __restrict__ goff,
                                                    const uint32_t* __restrict__ hscan,
                                                    const float4* __restrict__ rows, FlatK o,
                                                    const int32_t* __restrict__ ids, int64_t na,
                                                    const uint32_t* __restrict__ hrow,
                                                    const uint32_t* __restrict__ clamp_list,
                                                    std::conditional_t<DVEC, DampVecK, NoDampVec> dk) {
  o.rest_proj = PROJ ? 1 : 0;  // the launcher picked the variant from it
  if (cg_stopped(v)) return;
  extern __shared__ __attribute__((aligned(16))) float s_rest[];  // row chunks, then the factored SH stage
  __shared__ double s_dot[4];
  const int tid = threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.x * blockDim.x;
  const int64_t j = j0 + tid;
  const int64_t nrows = ACTIVE ? na : g.P;  // rows of v and y
  const int64_t nvalid = min((int64_t)blockDim.x, nrows - j0);
  const bool valid = j < nrows;
  const int64_t i = ACTIVE ? (valid ? (int64_t)ids[j] : 0) : j;
  // (a listed Gaussian owns a head row, so it touches a tile: its tile count is not read)
  const uint32_t n = ACTIVE ? (valid ? 1u : 0u) : (valid ? tiles[i] : 0u);
  float G2[NV];
  if (ACTIVE) {
    // the list's own row offsets (k_active_scatter): entry j's head rows are [hrow[j], hrow[j + 1])
    const uint32_t R0 = hrow[j0], R1 = hrow[j0 + nvalid];
    const uint32_t h0 = valid ? hrow[j] : R1, h1 = valid ? hrow[j + 1] : R1;
    block_sum_rows<ROWF4>(rows, R0, R1, h0, h1 - h0, reinterpret_cast<float4*>(s_rest), G2);
  } else {
    // this Gaussian's head rows (the LM row map): [hscan[goff], hscan[goff + tiles])
    const int64_t il = j0 + nvalid - 1;
    const uint32_t R0 = hscan[goff[j0]], R1 = hscan[goff[il] + tiles[il]];
    const uint32_t h0 = valid ? hscan[goff[i]] : R1, h1 = valid ? hscan[goff[i] + n] : R1;
    block_sum_rows<ROWF4>(rows, R0, R1, h0, h1 - h0, reinterpret_cast<float4*>(s_rest), G2);
  }
  ChainOut co;
  // clamp_list (gslm_active_params): g's parameter arrays and the clamp words are the list's own, row j
  const bool listed = ACTIVE && clamp_list != nullptr;
  if (valid) chain_vjp<true>(v, g, listed ? j : i, n != 0, n ? (listed ? clamp_list[j] : clampw[i]) : 0u, G2, WANT_MEANS, co);
  if (ACTIVE) g.P = na;  // the epilogue writes rows j < na of y (it reads P and M of g only)
  if constexpr (DVEC) lm_epilogue<WANT_MEANS, true, true>((v.D + 1) * (v.D + 1), g, co, o, s_rest, s_dot, &dk);
  else lm_epilogue<WANT_MEANS, true>((v.D + 1) * (v.D + 1), g, co, o, s_rest, s_dot);
}

// The SH-rest group of one view's Krylov space (GSLM_MV_SH_REST_PROJECTED): with one view every
// Gaussian's SH-rest column of J is B_rest(dir) (x) (d rgb), so J^T J + D (D a scalar on the group) maps
// span{B_rest(dir) (x) e_c} into itself, and every CG iterate started from J^T b stays there: 3
// coordinates per Gaussian along the unit direction Bh = B_rest / |B_rest| replace 3(M-1) floats.
//   mode 0 (expand):  out[i, k-1, c] = Bh_k in[i, c]         (k < nc; 0 for inactive coefficients)
//   mode 1 (project): out[i, c] = sum_k Bh_k in[i, k-1, c]
__global__ __launch_bounds__(256) void k_sh_rest_project(ViewK v, GaussK g, int mode, const float* __restrict__ in,
                                                         int64_t in_stride, float* __restrict__ out,
                                                         int64_t out_stride) {
  // the block's [256, M-1, 3] rows go through LDS so the full-layout side is read / written coalesced
  extern __shared__ __attribute__((aligned(16))) float s_rows[];
  const int R = 3 * (g.M - 1);
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x;
  const int64_t nv = min((int64_t)blockDim.x, g.P - i0);
  const int64_t i = i0 + threadIdx.x;
  if (mode == 1) {  // gather the rows to project
    for (int64_t e = threadIdx.x; e < nv * R; e += blockDim.x) {
      const int64_t ii = e / R, r = e - ii * R;
      s_rows[e] = in[(i0 + ii) * in_stride + r];
    }
    __syncthreads();
  }
  if (i < g.P) {
    const float x = g.means3D[3 * i + 0], y = g.means3D[3 * i + 1], z = g.means3D[3 * i + 2];
    const float dx = x - v.campos[0], dy = y - v.campos[1], dz = z - v.campos[2];
    const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
    float B[16];
    sh_basis(v.D, dx / len, dy / len, dz / len, B);
    const int nc = (v.D + 1) * (v.D + 1);
    const float nb = sh_rest_norm(B, nc);
    const float inv = nb > 0.f ? 1.f / nb : 0.f;
    float* row = s_rows + (int64_t)threadIdx.x * R;
    if (mode == 0) {
      for (int k = 1; k < g.M; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) row[3 * (k - 1) + c] = k < nc ? (B[k] * inv) * in[i * in_stride + c] : 0.f;
    } else {
      float acc[3] = {0.f, 0.f, 0.f};
      for (int k = 1; k < g.M && k < nc; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += (B[k] * inv) * row[3 * (k - 1) + c];
#pragma unroll
      for (int c = 0; c < 3; ++c) out[i * out_stride + c] = acc[c];
    }
  }
  if (mode == 0) {  // scatter the expanded rows
    __syncthreads();
    for (int64_t e = threadIdx.x; e < nv * R; e += blockDim.x) {
      const int64_t ii = e / R, r = e - ii * R;
      out[(i0 + ii) * out_stride + r] = s_rows[e];
    }
  }
}

// ---------------------------------------------------------------- launchers
int launch_sh_rest_project(const ViewK& v, const GaussK& g, int mode, const float* in, int64_t in_stride, float* out,
                           int64_t out_stride, hipStream_t s) {
  if (g.P == 0 || g.M < 2) return GSLM_OK;
  const size_t lds = (size_t)256 * 3 * (g.M - 1) * sizeof(float);
  hipLaunchKernelGGL(k_sh_rest_project, dim3((unsigned)((g.P + 255) / 256)), dim3(256), lds, s, v, g, mode, in,
                     in_stride, out, out_stride);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

int launch_preprocess_bwd(const ViewK& v, const GaussK& g, const GeomBufs& gb, const BinBufs& bb,
                          const ScratchBufs& sb, const GradK& out, bool want_means, hipStream_t s) {
  (void)bb;
  if (g.P == 0) return GSLM_OK;
  const unsigned nb = (unsigned)((g.P + 255) / 256);
  // the factored SH stage and the block's <dres, sh_k> (256 x SHB_STRIDE floats)
  const size_t sh_lds = (sh_stage_floats<true>(g.M) + (size_t)256 * SHB_STRIDE) * sizeof(float);
  const size_t chunk_lds = (size_t)GATHER_CHUNK * 3 * sizeof(float4);
  // (staging the primal SH rows here as k_preprocess_jvp does measured 221 -> 229 us at 1M: the 48 KB of LDS cost
  // more occupancy than the strided reads; profiles/r04/ab/dropin_staging -- only the 15 dot products with dres
  // are needed, formed from coalesced reads instead)
  const size_t lds = sh_lds > chunk_lds ? sh_lds : chunk_lds;
  if (g.raw)
    hipLaunchKernelGGL(k_preprocess_bwd<true>, dim3(nb), dim3(256), lds, s, v, g, gb.clampw, gb.tiles, gb.goff,
                       sb.contrib, out, want_means ? 1 : 0);
  else
    hipLaunchKernelGGL(k_preprocess_bwd<false>, dim3(nb), dim3(256), lds, s, v, g, gb.clampw, gb.tiles, gb.goff,
                       sb.contrib, out, want_means ? 1 : 0);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

int launch_gather_lm(const ViewK& v, const GaussK& g, const GeomBufs& gb, const ScratchBufs& sb, const FlatK& o,
                     bool mask_xyz, hipStream_t s, const int32_t* ids, int64_t na, const uint32_t* hrow,
                     const uint32_t* clamp_list, const DampVecK* dk) {
  const bool active = na >= 0;
  const int64_t nrows = active ? na : g.P;
  if (nrows == 0) return GSLM_OK;
  // guards of this launcher's own contract: the C entry points' plan (api.hip plan_matvec) has checked all of it,
  // so neither is reachable from the C ABI
  if (active && (!mask_xyz || !ids || !hrow)) {
    set_error("internal: the active-list gather runs on the LM rows (mask_xyz)");
    return GSLM_ERR_INVALID;
  }
  if (dk && (!mask_xyz || !o.use_damp)) {
    set_error("internal: the damping vector runs on the LM rows");
    return GSLM_ERR_INVALID;
  }
  const unsigned nb = (unsigned)((nrows + 255) / 256);
  const size_t rest_lds = sh_stage_floats<true>(g.M) * sizeof(float);
  const size_t chunk_lds = (size_t)GATHER_CHUNK * (mask_xyz ? 2 : 3) * sizeof(float4);
  const size_t lds = (rest_lds > chunk_lds ? rest_lds : chunk_lds) + 16;
  // the ten instantiations: the full rows (WANT_MEANS) by PROJ, the LM rows by PROJ x ACTIVE x DVEC
  auto launch = [&](auto means, auto proj, auto act, auto dvec) {
    constexpr bool MEANS = decltype(means)::value, DVEC = decltype(dvec)::value;
    std::conditional_t<DVEC, DampVecK, NoDampVec> d{};
    if constexpr (DVEC) d = *dk;
    hipLaunchKernelGGL((k_gather_lm<MEANS, MEANS ? 3 : 2, decltype(proj)::value, decltype(act)::value, DVEC>), dim3(nb),
                       dim3(256), lds, s, v, g, gb.clampw, gb.tiles, gb.goff, sb.hscan, sb.contrib, o, ids, na, hrow,
                       clamp_list, d);
  };
  with_bool(o.rest_proj != 0, [&](auto proj) {
    if (!mask_xyz) return launch(std::true_type{}, proj, std::false_type{}, std::false_type{});
    with_bool(active, [&](auto act) { with_bool(dk != nullptr, [&](auto dvec) { launch(std::false_type{}, proj, act, dvec); }); });
  });
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

// ---- flat vectors between the P layout and an active list's (gslm_active_pack / gslm_active_unpack) ----
struct PackK {
  int w[8];        // floats per row of each group
  int64_t poff[8]; // first float of each group in the P layout
  int64_t aoff[8]; // ... in the list's layout
  int n;
  int wsum;
};
// element e = (list row j, float c of the row's wsum floats over all groups), TO_ACTIVE: dst[list] = src[P layout]
template <bool TO_ACTIVE>
__global__ __launch_bounds__(256) void k_active_pack(PackK k, const int32_t* __restrict__ ids, int64_t na,
                                                      const float* __restrict__ src, float* __restrict__ dst) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= na * k.wsum) return;
  const int64_t j = e / k.wsum;
  int c = (int)(e - j * k.wsum), grp = 0;
  while (grp < k.n - 1 && c >= k.w[grp]) c -= k.w[grp++];
  const int64_t full = k.poff[grp] + (int64_t)ids[j] * k.w[grp] + c;
  const int64_t act = k.aoff[grp] + j * k.w[grp] + c;
  if (TO_ACTIVE) dst[act] = src[full];
  else dst[full] = src[act];
}

int launch_active_pack(bool to_active, const float* src, float* dst, const int32_t* ids, int64_t na, int64_t P,
                       const int32_t* widths, int ngroups, int64_t tail_n, hipStream_t s) {
  if (ngroups < 1 || ngroups > 8 || !widths || na < 0 || na > P || tail_n < 0 || !src || !dst || (na > 0 && !ids)) {
    set_error("active pack: 1..8 groups, 0 <= n_active <= P, non-NULL buffers");
    return GSLM_ERR_INVALID;
  }
  PackK k{};
  int64_t po = 0, ao = 0;
  for (int q = 0; q < ngroups; ++q) {
    if (widths[q] < 0) { set_error("active pack: negative group width"); return GSLM_ERR_INVALID; }
    k.w[q] = widths[q];
    k.poff[q] = po;
    k.aoff[q] = ao;
    po += P * widths[q];
    ao += na * widths[q];
    k.wsum += widths[q];
  }
  k.n = ngroups;
  const int64_t src_n = to_active ? po : ao, dst_n = to_active ? ao : po;
  if (!to_active) GSLM_HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)dst_n * sizeof(float), s));  // +0.0f off the list
  if (tail_n > 0)
    GSLM_HIP_CHECK(hipMemcpyAsync(dst + dst_n, src + src_n, (size_t)tail_n * sizeof(float), hipMemcpyDeviceToDevice, s));
  const int64_t total = na * k.wsum;
  if (total == 0) return GSLM_OK;
  const unsigned nb = (unsigned)((total + 255) / 256);
  if (to_active) hipLaunchKernelGGL(k_active_pack<true>, dim3(nb), dim3(256), 0, s, k, ids, na, src, dst);
  else hipLaunchKernelGGL(k_active_pack<false>, dim3(nb), dim3(256), 0, s, k, ids, na, src, dst);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

// ---- the list-order parameter block (gslm_active_params) ----
__global__ __launch_bounds__(256) void k_active_params(const float* __restrict__ means3D, const float* __restrict__ scales,
                                                        const float* __restrict__ rot, const float* __restrict__ opac,
                                                        const uint32_t* __restrict__ clampw,
                                                        const int32_t* __restrict__ ids, int64_t na,
                                                        float* __restrict__ xyz_l, float* __restrict__ scales_l,
                                                        float* __restrict__ rot_l, float* __restrict__ opac_l,
                                                        uint32_t* __restrict__ clamp_l, int32_t* __restrict__ pos) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= na) return;
  const int64_t i = ids[j];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    xyz_l[3 * j + k] = means3D[3 * i + k];
    scales_l[3 * j + k] = scales[3 * i + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) rot_l[4 * j + k] = rot[4 * i + k];
  opac_l[j] = opac[i];
  clamp_l[j] = clampw[i];
  pos[i] = (int32_t)j;
}

int launch_active_params(const float* means3D, const float* scales, const float* rot, const float* opac,
                         const uint32_t* clampw, const int32_t* ids, int64_t na, int64_t P, float* xyz_l,
                         float* scales_l, float* rot_l, float* opac_l, uint32_t* clamp_l, int32_t* pos, hipStream_t s) {
  if (P > 0) GSLM_HIP_CHECK(hipMemsetAsync(pos, 0xFF, (size_t)P * sizeof(int32_t), s));  // -1: not listed
  if (na == 0) return GSLM_OK;
  hipLaunchKernelGGL(k_active_params, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, s, means3D, scales, rot, opac,
                     clampw, ids, na, xyz_l, scales_l, rot_l, opac_l, clamp_l, pos);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

// ---- the lean CG loop's first and last launch (gslm_cg_start_active / gslm_cg_end_active) ----
static int make_packk(const char* who, const int32_t* widths, int ngroups, int64_t na, int64_t P, PackK* k, int64_t* po,
                      int64_t* ao) {
  if (ngroups < 1 || ngroups > 8 || !widths || na < 0 || na > P) {
    set_error(std::string(who) + ": 1..8 groups, 0 <= n_active <= P");
    return GSLM_ERR_INVALID;
  }
  *k = PackK{};
  *po = *ao = 0;
  for (int q = 0; q < ngroups; ++q) {
    if (widths[q] < 0) { set_error(std::string(who) + ": negative group width"); return GSLM_ERR_INVALID; }
    k->w[q] = widths[q];
    k->poff[q] = *po;
    k->aoff[q] = *ao;
    *po += P * widths[q];
    *ao += na * widths[q];
    k->wsum += widths[q];
  }
  k->n = ngroups;
  return GSLM_OK;
}

// r / w and r % w of a non-negative r: 32-bit when r fits (every layout the solver meets), 64-bit otherwise
__device__ __forceinline__ void divmod_w(int64_t r, int w, int64_t& d, int& c) {
  if (r < ((int64_t)1 << 32)) {
    // (the solver's widths as constants: a multiply or a shift instead of the division loop)
    const uint32_t d32 = w == 3 ? (uint32_t)r / 3u : w == 4 ? (uint32_t)r / 4u : w == 1 ? (uint32_t)r
                                                                                         : (uint32_t)r / (uint32_t)w;
    d = d32;
    c = (int)((uint32_t)r - d32 * (uint32_t)w);
  } else {
    d = r / w;
    c = (int)(r - d * w);
  }
}

// The solve's start in one pass over the list layout: s = p = (the listed rows of the full-layout g), q = x = 0 on
// [lo, n), and the partials of gamma_0 = <s, s> over [lo, n) with k_dot_partial's element-to-thread mapping
// (DOT_BLOCKS blocks of DOT_THREADS, element lo + b DOT_THREADS + t + m stride in order of m), so the finished sum
// is bitwise gslm_dot's.  The head [0, lo) (the masked xyz group) is zeroed in all four.
__global__ __launch_bounds__(DOT_THREADS) void k_cg_start_active(PackK k, const int32_t* __restrict__ ids, int64_t lo,
                                                                  int64_t ao, int64_t po, int64_t tail_n,
                                                                  const float* __restrict__ gf, float* __restrict__ s,
                                                                  float* __restrict__ p, float* __restrict__ q,
                                                                  float* __restrict__ x, double* __restrict__ part) {
  __shared__ double sm[DOT_THREADS / 64];
  const int64_t n = ao + tail_n;
  const int64_t stride = (int64_t)gridDim.x * DOT_THREADS;
  const int64_t t0 = (int64_t)blockIdx.x * DOT_THREADS + threadIdx.x;
  for (int64_t m = t0; m < lo; m += stride) s[m] = p[m] = q[m] = x[m] = 0.f;
  double acc = 0.0;
  constexpr int U = 4;  // elements of a thread in flight (two dependent loads each); summed in their order
  for (int64_t m0 = lo + t0; m0 < n; m0 += U * stride) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t m = m0 + u * stride;
      v[u] = 0.f;
      if (m >= n) continue;
      if (m >= ao) {
        v[u] = gf[po + (m - ao)];
      } else {
        int grp = 0;
        while (grp < k.n - 1 && m >= k.aoff[grp + 1]) ++grp;
        int64_t j;
        int c;
        divmod_w(m - k.aoff[grp], k.w[grp], j, c);
        v[u] = gf[k.poff[grp] + (int64_t)ids[j] * k.w[grp] + c];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t m = m0 + u * stride;
      if (m >= n) continue;
      s[m] = v[u];
      p[m] = v[u];
      q[m] = 0.f;
      x[m] = 0.f;
      acc += (double)v[u] * (double)v[u];
    }
  }
  const double t = block_sum_d(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

int launch_cg_start_active(const float* g_full, const int32_t* ids, int64_t na, int64_t P, const int32_t* widths,
                           int ngroups, int64_t tail_n, int64_t lo, float* s_, float* p, float* q, float* x,
                           double* part, hipStream_t s) {
  PackK k;
  int64_t po, ao;
  int st = make_packk("cg_start_active", widths, ngroups, na, P, &k, &po, &ao);
  if (st) return st;
  if (!g_full || !s_ || !p || !q || !x || !part || (na > 0 && !ids) || tail_n < 0 || lo < 0 || lo > ao + tail_n) {
    set_error("cg_start_active: NULL buffer, negative tail or lo outside [0, n]");
    return GSLM_ERR_INVALID;
  }
  hipLaunchKernelGGL(k_cg_start_active, dim3(DOT_BLOCKS), dim3(DOT_THREADS), 0, s, k, ids, lo, ao, po, tail_n, g_full, s_,
                     p, q, x, part);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

// The solve's end in one pass over the full-layout output: thread (group blockIdx.y, Gaussian i) writes the row's
// floats -- x + a p of list row pos[i] (a = num / den, k_axpy_dev's arithmetic, applied on [lo, n) as the solve's
// last deferred update is), or +0.0f when i is not listed; the blocks of the row past the groups copy the tail.
// Block (0, 0) also finishes the last gamma' into its slot (nobody else will read those partials).
__global__ __launch_bounds__(DOT_THREADS) void k_cg_end_active(PackK k, const int32_t* __restrict__ pos, int64_t P,
                                                                int64_t lo, int64_t ao, int64_t po, int64_t tail_n,
                                                                const float* __restrict__ x, const float* __restrict__ p,
                                                                const double* __restrict__ num,
                                                                const double* __restrict__ den, float* __restrict__ out,
                                                                ScalarK fin) {
  __shared__ double sm[DOT_THREADS / 64 + 1];
  if (blockIdx.x == 0 && blockIdx.y == 0 && fin.part) load_scalar(fin, sm);  // (block-uniform)
  float af = 0.f;
  if (num) {
    const double a = den ? (*num) / (*den) : (*num);
    af = (float)(a * (double)1.0f);
  }
  const int grp = blockIdx.y;
  if (grp == k.n) {
    const int64_t stride = (int64_t)gridDim.x * DOT_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * DOT_THREADS + threadIdx.x; e < tail_n; e += stride) {
      const int64_t m = ao + e;
      float v = x[m];
      if (num && m >= lo) v = v + af * p[m];
      out[po + e] = v;
    }
    return;
  }
  const int64_t i = (int64_t)blockIdx.x * DOT_THREADS + threadIdx.x;
  if (i >= P) return;
  const int w = k.w[grp];
  const int32_t j = pos[i];
  float* o = out + k.poff[grp] + i * w;
  if (j < 0) {
    for (int c = 0; c < w; ++c) o[c] = 0.f;
    return;
  }
  const int64_t m0 = k.aoff[grp] + (int64_t)j * w;
  for (int c0 = 0; c0 < w; c0 += 4) {
    float xv[4], pv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool on = c0 + c < w;
      xv[c] = on ? x[m0 + c0 + c] : 0.f;
      pv[c] = (on && num && m0 + c0 + c >= lo) ? p[m0 + c0 + c] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c0 + c < w) o[c0 + c] = (num && m0 + c0 + c >= lo) ? xv[c] + af * pv[c] : xv[c];
  }
}

int launch_cg_end_active(const float* x, const float* p, const double* num, const double* den, int64_t lo,
                         const int32_t* pos, int64_t na, int64_t P, const int32_t* widths, int ngroups,
                         int64_t tail_n, float* out, const double* fin_part, int fin_np, double* fin_dev,
                         hipStream_t s) {
  PackK k;
  int64_t po, ao;
  int st = make_packk("cg_end_active", widths, ngroups, na, P, &k, &po, &ao);
  if (st) return st;
  if (!x || !out || (num && !p) || (P > 0 && !pos) || tail_n < 0 || lo < 0 || (fin_part && (fin_np < 0 || !fin_dev))) {
    set_error("cg_end_active: NULL buffer, negative tail or lo, or partials without a slot for their sum");
    return GSLM_ERR_INVALID;
  }
  int64_t nb = (P + DOT_THREADS - 1) / DOT_THREADS;
  nb = nb < 1 ? 1 : nb;
  hipLaunchKernelGGL(k_cg_end_active, dim3((unsigned)nb, (unsigned)(k.n + 1)), dim3(DOT_THREADS), 0, s, k, pos, P, lo, ao,
                     po, tail_n, x, p, num, den, out, ScalarK{nullptr, fin_part, fin_np, fin_dev});
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

}  // namespace gslm
