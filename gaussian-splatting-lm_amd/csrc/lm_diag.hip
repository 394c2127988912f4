// lm_diag.hip -- diag(J^T W J + D) of the LM normal equations on the LM rows (xyz frozen), and the vector kernels
// of Jacobi-preconditioned CG.
//
//   k_render_diag    per tile, back to front over the list with the parts of vjp_tile's pass (gslm_tile.hpp:
//                    wave_bounds, stage_entry into 128-entry batches, primal_test, combine_waves) around a visit of
//                    its own: per head entry twelve image sums over the pixels that blend it -- nine monomials
//                    sum w G^2 dx^i dy^j of the geometry block and three colour sums -- one 48-byte row per entry
//                    through the LM row map.
//   k_gather_diag    per Gaussian: the sum of its head rows, the 4x4 block S in (conic a, b, c, effective opacity),
//                    diag_j = c_j^T S c_j with c_j = chain_jvp of parameter j's unit tangent, and B_k^2 S_col[c]
//                    for the SH groups; written into the flat layout (full or single-view projected), overwrite
//                    or accumulate, with D added on request.
//   k_pcg_update     x += a p, s -= a q, z = s (.) minv and the block partials of <s, z>.
// With mask_xyz the view direction is fixed, so a parameter moves either the colour or (a, b, c, o), never both:
// no colour x geometry cross terms.  d alpha / d(a, b, c, o) = G (-o dx^2 / 2, -o dx dy, -o dy^2 / 2, 1), the
// derivative k_render_matvec applies (the 0.99 clamp ignored, as upstream and vjp_tile ignore it): this is the
// diagonal of that operator.  No float atomics: bitwise reproducible.
#include "gslm_tile.hpp"
#include "gslm_chain.hpp"
#include "gslm_gather.hpp"

namespace gslm {

constexpr int DIAG_BATCH = 128;
constexpr int ND = 12;  // floats per row: [m00 m20 m11 m02 | m40 m31 m22 m13 | m04 col_r col_g col_b]

// 128-entry batches: 24.2 KB of per-wave partials + 5 KB of records -> 5 blocks per CU
__global__ __launch_bounds__(256) void k_render_diag(ViewK v, const uint2* __restrict__ ranges,
                                                     const uint32_t* __restrict__ tile_order,
                                                     const uint32_t* __restrict__ point_list,
                                                     const float4* __restrict__ rec,
                                                     const uint32_t* __restrict__ slots,
                                                     const float* __restrict__ final_T,
                                                     const uint32_t* __restrict__ n_contrib,
                                                     const float* __restrict__ weight, float4* __restrict__ rows) {
  constexpr int B = DIAG_BATCH;
  constexpr int STR = acc_stride<B>();
  __shared__ uint64_t s_bits[16];
  __shared__ int s_misc[4];
  __shared__ float s_acc[4 * ND * STR];  // [wave][value][batch element]
  __shared__ float2 s_rp[5 * B];         // the batch's five record planes (stage_entry)
  const TilePix p = tile_pix(v, tile_order);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t pid = p.pid;
  const int64_t HW = (int64_t)v.H * v.W;
  const uint2 range = ranges[p.tile];
  const float pxf = (float)p.px, pyf = (float)p.py;
  uint32_t last = 0;
  float T = 0.f, W0 = 0.f, W1 = 0.f, W2 = 0.f;
  if (p.inside) {
    last = n_contrib[pid];
    T = final_T[pid];
    // 2 w: the [r; r] pair, as in u = 2 w (.) J v
    W0 = 2.f * weight[pid];
    W1 = 2.f * weight[HW + pid];
    W2 = 2.f * weight[2 * HW + pid];
  }
  // the background term of d colour_c / d alpha is tb_c / (1 - alpha), tb_c = -T_final bg_c
  const float tb0 = -T * v.bg[0], tb1 = -T * v.bg[1], tb2 = -T * v.bg[2];
  // the colour accumulated behind the current entry, per channel (VjpPix::accd carries only its dot with the seed)
  float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
  const WaveBounds wb = wave_bounds(last, range, s_misc);
  const int n_eff = wb.n_eff;
  const int rounds = (n_eff + B - 1) / B;
  for (int r = 0; r < rounds; ++r) {
    const int base = n_eff - 1 - r * B;  // list position of batch element 0
    const int cnt = min(B, base + 1);
    __syncthreads();
    uint32_t my_slot = 0, my_mask = 0u;
    if (tid < cnt) {
      uint32_t g;
      my_mask = stage_entry<B>(point_list, range.x, base - tid, rec, wb, s_rp, tid, g);
      if (my_mask) my_slot = slots[range.x + base - tid];  // a head entry: it owns a row of the LM row map
    }
    publish_quad_masks(my_mask, s_bits);
    __syncthreads();
#pragma unroll 1
    for (int wd = 0; wd < (B + 63) / 64; ++wd) {
      uint64_t hits = wave_bits(s_bits, w, wd);
      while (hits) {
        const int hb = (int)__builtin_ctzll(hits);
        hits = clear_bit(hits, hb);
        const int j = 64 * wd + hb;
        const VisitRec e = load_visit<B>(s_rp, j);
        const Primal pt = primal_test(e, pxf, pyf, (uint32_t)(base - j), last);  // base - j: 0-based list position
        const float dx = pt.dx, dy = pt.dy;
        float r1v = 0.f, r2v = 0.f;
        if (pt.any) {
          // an invalid lane runs the body with alpha = G = 0: its values are 0, T and the accumulation are unchanged
#pragma clang fp contract(fast)
          const float a_e = pt.valid ? pt.alpha : 0.f;
          const float G_e = pt.valid ? pt.G : 0.f;
          const float inv1ma = rcp_f(1.f - a_e);
          T = T * inv1ma;  // the transmittance in front of this entry
          const float aT = a_e * T;
          const float aT2 = aT * aT;
          // g_c = d colour_c / d alpha = (col_c - acc_c) T - T_final bg_c / (1 - alpha): vjp_tile's dL_dalpha for
          // the seed e_c; this entry joins the accumulation behind the next one after it is used
          const float d0 = e.rg.x - acc0, d1 = e.rg.y - acc1, d2 = e.bd.x - acc2;
          // (sums of two products name the product that is rounded: which one contraction would fuse is the
          // compiler's choice, and it changes with the code around it)
          const float g0 = fmaf(tb0, inv1ma, d0 * T), g1 = fmaf(tb1, inv1ma, d1 * T), g2 = fmaf(tb2, inv1ma, d2 * T);
          acc0 = acc0 + a_e * d0;
          acc1 = acc1 + a_e * d1;
          acc2 = acc2 + a_e * d2;
          // (W0 g0^2 + W1 g1^2) + W2 g2^2
          const float om = fmaf(W2 * g2, g2, fmaf(W1 * g1, g1, W0 * g0 * g0));
          const float h = om * (G_e * G_e);
          const float dx2 = dx * dx, dxy = dx * dy, dy2 = dy * dy;
          const float hx2 = h * dx2, hxy = h * dxy, hy2 = h * dy2;
          float pv[8], qv[8];
          pv[0] = h;
          pv[1] = hx2;
          pv[2] = hxy;
          pv[3] = hy2;
          pv[4] = hx2 * dx2;
          pv[5] = hx2 * dxy;
          pv[6] = hx2 * dy2;  // the (2,2) monomial: shared by the a.c and the b.b term
          pv[7] = hxy * dy2;
          qv[0] = hy2 * dy2;
          qv[1] = W0 * aT2;
          qv[2] = W1 * aT2;
          qv[3] = W2 * aT2;
          // slots 4..7 of the second reduction are never stored and never mix into a stored one
#pragma unroll
          for (int k = 4; k < 8; ++k) qv[k] = qv[k - 4];
          r1v = wave_reduce8_t(pv, lane);
          r2v = wave_reduce8_t(qv, lane);
        }
        const int k = lane >> 3;
        if ((lane & 7) == 0) {
          s_acc[(w * ND + k) * STR + j] = r1v;
          if (k < 4) s_acc[(w * ND + 8 + k) * STR + j] = r2v;
        }
      }
    }
    __syncthreads();
    // rows only for the entries some wave visited
    if (tid < cnt && my_mask) {
      float t[ND];
#pragma unroll
      for (int q = 0; q < ND; ++q) t[q] = combine_waves<ND, STR>(s_acc, q, tid, my_mask);
      rows[3 * (size_t)my_slot + 0] = make_float4(t[0], t[1], t[2], t[3]);
      rows[3 * (size_t)my_slot + 1] = make_float4(t[4], t[5], t[6], t[7]);
      rows[3 * (size_t)my_slot + 2] = make_float4(t[8], t[9], t[10], t[11]);
    }
  }
}

struct DiagK {
  float* y[6];    // xyz, dc, rest, scaling, rotation, opacity groups of the destination (NULL: not written)
  float damp[6];
  int add_damp;   // D is added (once: the caller asks for it in one view of a sum over views)
  int overwrite;
  int has_rows;   // the view rendered something: the row map and the rows exist
};

__device__ __forceinline__ void put_diag(float* y, int64_t e, float val, float d, const DiagK& o) {
  const float x = o.add_damp ? val + d : val;
  y[e] = o.overwrite ? x : y[e] + x;
}

// c^T S c for the symmetric 4x4 block S in (conic a, b, c, effective opacity) of a Gaussian with effective opacity
// op, from the nine monomial sums m = [m00 m20 m11 m02 m40 m31 m22 m13 m04]:
//   d alpha / d(a, b, c, o) = G (-op dx^2 / 2, -op dx dy, -op dy^2 / 2, 1)
__device__ __forceinline__ float quad_s(const float m[ND], float op, const float t[10]) {
  const float ca = -0.5f * op * t[2], cb = -op * t[3], cc = -0.5f * op * t[4], co = t[5];
  // sum w G^2 (ca dx^2 + cb dx dy + cc dy^2 + co)^2, expanded in the monomials
  return ca * ca * m[4] + 2.f * ca * cb * m[5] + (2.f * ca * cc + cb * cb) * m[6] + 2.f * cb * cc * m[7] +
         cc * cc * m[8] + 2.f * co * (ca * m[1] + cb * m[2] + cc * m[3]) + co * co * m[0];
}

// PROJ: the single-view projected SH-rest layout (3 floats per Gaussian along B_rest / |B_rest|).
template <bool PROJ>
__global__ __launch_bounds__(256) void k_gather_diag(ViewK v, GaussK g, const uint32_t* __restrict__ clampw,
                                                     const uint32_t* __restrict__ tiles,
                                                     const uint32_t* __restrict__ goff,
                                                     const uint32_t* __restrict__ hscan,
                                                     const float4* __restrict__ rows, DiagK o) {
  __shared__ float4 s_buf[GATHER_CHUNK * 3];  // row chunks, then the factored SH stage (256 x (17 + 4) floats)
  static_assert(sizeof(float4) * GATHER_CHUNK * 3 >= sizeof(float) * 256 * (SHB_STRIDE + 4), "SH stage fits");
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x;
  const int64_t i = i0 + tid;
  const int64_t nvalid = min((int64_t)blockDim.x, g.P - i0);
  const bool valid = i < g.P;
  float m[ND];
#pragma unroll
  for (int q = 0; q < ND; ++q) m[q] = 0.f;
  bool seen = false;
  if (o.has_rows) {  // (block-uniform)
    // this Gaussian's head rows (the LM row map): [hscan[goff], hscan[goff + tiles])
    const int64_t il = i0 + nvalid - 1;
    const uint32_t n = valid ? tiles[i] : 0u;
    const uint32_t R0 = hscan[goff[i0]], R1 = hscan[goff[il] + tiles[il]];
    const uint32_t h0 = valid ? hscan[goff[i]] : R1, h1 = valid ? hscan[goff[i] + n] : R1;
    block_sum_rows<3, ND>(rows, R0, R1, h0, h1 - h0, s_buf, m);
    seen = h1 > h0;
  }
  const int nc = (v.D + 1) * (v.D + 1);
  float dsc[3] = {0.f, 0.f, 0.f}, drot[4] = {0.f, 0.f, 0.f, 0.f}, dop = 0.f;
  float B2[16], scol[3] = {0.f, 0.f, 0.f}, nb2 = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) B2[k] = 0.f;
  if (valid && seen) {  // an unseen Gaussian gets D alone: nothing is read for it
    const uint32_t cw = clampw[i];
    // c_j = chain_jvp of the unit tangent of parameter j (3 scalings, 4 rotations, the opacity): the antialiasing
    // factor's share of do, scale_modifier and the raw-mode activations are the chain's own
    float ts[3], tr[4], to[1];
    GaussK t{};
    t.P = g.P;
    t.raw = g.raw;
    t.M = g.M;
    t.scales = ts;
    t.rot = tr;
    t.opac = to;
    t.dc_stride = 3;
    t.rest_stride = 3;
    float op_eff = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
      for (int k = 0; k < 3; ++k) ts[k] = (j == k) ? 1.f : 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) tr[k] = (j == 3 + k) ? 1.f : 0.f;
      to[0] = (j == 7) ? 1.f : 0.f;
      float T2[10];
      chain_jvp<true>(v, g, t, nullptr, i, 0, cw, T2);
      if (j == 0) {
        // the effective opacity of the render record (activated opacity x antialiasing factor)
        Geo e;
        compute_geo<true>(v, g, i, cw, e);
        op_eff = e.op * e.h;
      }
      const float val = quad_s(m, op_eff, T2);
      if (j < 3) dsc[j] = val;
      else if (j < 7) drot[j - 3] = val;
      else dop = val;
    }
    // DC and SH rest: B_k(dir)^2 S_col[c] on the channels the SH clamp leaves free
    const float x = g.means3D[3 * i + 0], y = g.means3D[3 * i + 1], z = g.means3D[3 * i + 2];
    float ddx = x - v.campos[0], ddy = y - v.campos[1], ddz = z - v.campos[2];
    const float len = sqrtf((ddx * ddx + ddy * ddy) + ddz * ddz);
    float Bv[16];
    sh_basis(v.D, ddx / len, ddy / len, ddz / len, Bv);
#pragma unroll
    for (int k = 0; k < 16; ++k) B2[k] = k < nc ? Bv[k] * Bv[k] : 0.f;
    const float nb = sh_rest_norm(Bv, nc);
    nb2 = nb * nb;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) scol[ch] = ((cw >> ch) & 1u) ? 0.f : m[9 + ch];
  }
  if (valid) {
    if (o.y[0]) {  // xyz is frozen: D alone
#pragma unroll
      for (int k = 0; k < 3; ++k) put_diag(o.y[0], 3 * i + k, 0.f, o.damp[0], o);
    }
    if (o.y[1])
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) put_diag(o.y[1], 3 * i + ch, B2[0] * scol[ch], o.damp[1], o);
    if (o.y[3])
#pragma unroll
      for (int k = 0; k < 3; ++k) put_diag(o.y[3], 3 * i + k, dsc[k], o.damp[3], o);
    if (o.y[4])
#pragma unroll
      for (int k = 0; k < 4; ++k) put_diag(o.y[4], 4 * i + k, drot[k], o.damp[4], o);
    if (o.y[5]) put_diag(o.y[5], i, dop, o.damp[5], o);
    if (PROJ && o.y[2] && g.M > 1)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) put_diag(o.y[2], 3 * i + ch, nb2 * scol[ch], o.damp[2], o);
  }
  if (PROJ || !o.y[2] || g.M < 2) return;  // (block-uniform)
  // the full layout's SH-rest group, factored through LDS as lm_epilogue's: stores in contiguous wave segments
  float* s_B = reinterpret_cast<float*>(s_buf);
  float* s_d = s_B + 256 * SHB_STRIDE;
  if (valid) {
#pragma unroll
    for (int k = 0; k < 16; ++k) s_B[tid * SHB_STRIDE + k] = B2[k];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s_d[tid * 4 + ch] = scol[ch];
  }
  __syncthreads();
  const int R = 3 * (g.M - 1);
  const int64_t base = i0 * R, total = nvalid * R;
  const float invR = 1.0f / (float)R;
  for (int64_t e = tid; e < total; e += blockDim.x) {
    // e -> (Gaussian ii, coefficient k >= 1, channel ch); the float quotient is exact: e < 256 R (lm_epilogue)
    const int ii = (int)(((float)e + 0.5f) * invR);
    const int r = (int)e - ii * R;
    const int k = 1 + r / 3, ch = r - 3 * (k - 1);
    const float val = k < nc ? s_B[ii * SHB_STRIDE + k] * s_d[ii * 4 + ch] : 0.f;
    put_diag(o.y[2], base + e, val, o.damp[2], o);
  }
}

int launch_lm_diag(const ViewK& v, const GaussK& g, const GeomBufs& gb, const BinBufs& bb, const ImgBufs& ib,
                   const ScratchBufs& sb, int64_t N, const float* weight, const GradK& y, const double* damp7,
                   bool overwrite, bool rest_proj, bool tail_clean, hipStream_t s) {
  const int ntiles = v.gx * v.gy;
  const bool has_rows = N > 0 && ntiles > 0;
  if (has_rows) {
    // the LM row map (and the refined quadrant masks): the current one, or built here as a product would
    if (!tail_clean) {
      const int st = launch_lm_rowmap(v, gb, bb, ib, sb, N, s);
      if (st) return st;
    }
    hipLaunchKernelGGL(k_render_diag, dim3(ntiles), dim3(TILE_PIX), 0, s, v, bb.ranges, bb.tile_order, bb.point_list,
                       gb.rec, bb.slots, ib.final_T, ib.n_contrib, weight, sb.contrib);
    GSLM_LAUNCH_CHECK();
  }
  if (g.P == 0) return GSLM_OK;
  DiagK o;
  o.y[0] = y.means3D; o.y[1] = y.dc; o.y[2] = y.rest; o.y[3] = y.scales; o.y[4] = y.rot; o.y[5] = y.opac;
  for (int k = 0; k < 6; ++k) o.damp[k] = damp7 ? (float)damp7[k] : 0.f;
  o.add_damp = damp7 ? 1 : 0;
  o.overwrite = overwrite ? 1 : 0;
  o.has_rows = has_rows ? 1 : 0;
  const unsigned nb = (unsigned)((g.P + 255) / 256);
  if (rest_proj && g.M > 1)
    hipLaunchKernelGGL(k_gather_diag<true>, dim3(nb), dim3(256), 0, s, v, g, gb.clampw, gb.tiles, gb.goff, sb.hscan,
                       sb.contrib, o);
  else
    hipLaunchKernelGGL(k_gather_diag<false>, dim3(nb), dim3(256), 0, s, v, g, gb.clampw, gb.tiles, gb.goff, sb.hscan,
                       sb.contrib, o);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

// One preconditioned CG step on flat vectors, a = gam / del (device scalars):
//   x += a p (x != NULL) ;  s -= a q ;  z = s (.) minv ;  part[block] = sum s_new z_new
// k_cg_update's element-to-thread mapping and summation order: with minv = 1 the partials are bitwise its own.
__global__ __launch_bounds__(DOT_THREADS) void k_pcg_update(int64_t n, const double* __restrict__ gam,
                                                            const double* __restrict__ del,
                                                            const float* __restrict__ p, const float* __restrict__ q,
                                                            float* __restrict__ x, float* __restrict__ s,
                                                            const float* __restrict__ minv, float* __restrict__ z,
                                                            double* __restrict__ part) {
  __shared__ double sm[DOT_THREADS / 64 + 1];
  const float a = (float)(*gam / *del);
  double acc = 0.0;
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * DOT_THREADS;
  const float4* p4 = reinterpret_cast<const float4*>(p);
  const float4* q4 = reinterpret_cast<const float4*>(q);
  const float4* m4 = reinterpret_cast<const float4*>(minv);
  float4* x4 = reinterpret_cast<float4*>(x);
  float4* s4 = reinterpret_cast<float4*>(s);
  float4* z4 = reinterpret_cast<float4*>(z);
  const bool do_x = x != nullptr;
  for (int64_t i = (int64_t)blockIdx.x * DOT_THREADS + threadIdx.x; i < n4; i += stride) {
    const float4 qv = q4[i], mv = m4[i];
    float4 sv = s4[i];
    if (do_x) {
      const float4 pv = p4[i];
      float4 xv = x4[i];
      xv.x += a * pv.x; xv.y += a * pv.y; xv.z += a * pv.z; xv.w += a * pv.w;
      x4[i] = xv;
    }
    sv.x -= a * qv.x; sv.y -= a * qv.y; sv.z -= a * qv.z; sv.w -= a * qv.w;
    s4[i] = sv;
    const float4 zv = make_float4(sv.x * mv.x, sv.y * mv.y, sv.z * mv.z, sv.w * mv.w);
    z4[i] = zv;
    acc += (double)sv.x * zv.x + (double)sv.y * zv.y + (double)sv.z * zv.z + (double)sv.w * zv.w;
  }
  for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * DOT_THREADS + threadIdx.x; i < n; i += stride) {
    if (do_x) x[i] = x[i] + a * p[i];
    const float sv = s[i] - a * q[i];
    s[i] = sv;
    const float zv = sv * minv[i];
    z[i] = zv;
    acc += (double)sv * zv;
  }
  const double t = block_sum_d(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void k_precond_invert(int64_t n, const float* __restrict__ m,
                                                        float* __restrict__ minv) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float d = m[i];
    minv[i] = d > 0.f ? 1.f / d : 0.f;  // (a NaN entry: 0)
  }
}

}  // namespace gslm

using namespace gslm;

extern "C" {

int gslm_pcg_update(int64_t n, const double* gam_dev, const double* del_dev, const float* p, const float* q, float* x,
                    float* s, const float* minv, float* z, void* scratch, double* gam_new_dev, void* stream) {
  if (n < 0 || !gam_dev || !del_dev || !q || !s || !minv || !z || !scratch || !gam_new_dev || (x && !p)) {
    set_error("gslm_pcg_update: n < 0, a NULL scalar, vector or scratch, or x without p");
    return GSLM_ERR_INVALID;
  }
  if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(x) |
       reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(minv) | reinterpret_cast<uintptr_t>(z)) & 15) {
    set_error("gslm_pcg_update: vectors must be 16-byte aligned");
    return GSLM_ERR_INVALID;
  }
  hipLaunchKernelGGL(k_pcg_update, dim3(DOT_BLOCKS), dim3(DOT_THREADS), 0, (hipStream_t)stream, n, gam_dev, del_dev, p,
                     q, x, s, minv, z, (double*)scratch);
  GSLM_LAUNCH_CHECK();
  return gslm_dot_finalize(scratch, DOT_BLOCKS, gam_new_dev, stream);
}

int gslm_precond_invert(int64_t n, const float* m, float* minv, void* stream) {
  if (n < 0 || (n > 0 && (!m || !minv))) {
    set_error("gslm_precond_invert: n < 0 or a NULL vector");
    return GSLM_ERR_INVALID;
  }
  if (n == 0) return GSLM_OK;
  int64_t nb = (n + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(k_precond_invert, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, n, m, minv);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

}  // extern "C"
