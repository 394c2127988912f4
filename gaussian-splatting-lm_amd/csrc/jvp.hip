// jvp.hip -- tile passes of the forward-mode tangent and of the fused LM normal-equations product
// (the per-Gaussian tangent records come from tangent.hip).
//
//   k_render_jvp       per tile, front-to-back over the *primal's* sorted list (no re-sort), the
//                      skip/stop decisions frozen at the primal (bounded by n_contrib):
//                        dC += drgb a T + rgb (da T + a dT),  dT <- dT (1 - a) - T da.
//   k_render_matvec    the fused pair: JVP pass -> u = 2 w (.) J v in registers -> VJP pass ->
//                      one reduced row per (tile, Gaussian); the per-pixel J v never touches HBM.
//                      With the compact LM records the JVP pass runs one independent wave per quadrant
//                      (jvp_wave_packed, no block barrier; k_render_jv_wave is the J v-only form); with
//                      screen-position tangents the block-cooperative jvp_tile.
//   k_render_matvec_exposure   k_render_matvec<false> with the exposure map between its passes; the two share
//                      one LDS plan (MatvecLds) and one set of per-pixel loads (MatvecPix).
// Every kernel here starts with gslm_tile.hpp's tile_pix; jvp_tile takes its per-wave bounds from wave_bounds.
#include "gslm_tile.hpp"
#include "gslm_chain.hpp"

namespace gslm {

constexpr int MATVEC_BATCH = 128;

struct JvpPix {
  float T, dT, dC[3], dD;
};

// Front-to-back tangent pass over the tile, BATCH list entries staged in LDS per round.
// Block-uniform; blockDim = 256.  Wave w visits only the batch elements whose alpha region reaches its
// 8x8 quadrant (publish_quad_masks) and that lie before the last position any of its pixels blends (the
// primal's n_contrib; wave_bounds, as vjp_tile); a lane blends entry `pos` only while
// pos < its own n_contrib -- the stop decision frozen at the primal, without a per-iteration done flag.
// Records: the primal's three float4 (the third as a float2) and the 12-float tangent record of the drop-in
// JVP, [dx dy da db | dc dop dr dg | db dinv].  (The LM product's compact records go through jvp_wave_packed.)
template <bool WITH_XY, bool WITH_INV, int BATCH>
__device__ __forceinline__ void jvp_tile(JvpPix& o, bool inside, float pxf, float pyf, uint32_t last, uint2 range,
                                         const uint32_t* __restrict__ point_list, const float4* __restrict__ rec,
                                         const float4* __restrict__ trec,
                                         float4* s_r0, float4* s_r1, float2* s_r2, float4* s_t0, float4* s_t1,
                                         float2* s_t2, uint64_t* s_bits, int* s_cnt) {
  static_assert(WITH_XY || WITH_INV, "the LM product's compact records are jvp_wave_packed's");
  const int tid = threadIdx.x, w = tid >> 6;
  o.T = 1.f;
  o.dT = 0.f;
  o.dC[0] = o.dC[1] = o.dC[2] = 0.f;
  o.dD = 0.f;
  const uint32_t my_last = inside ? last : 0u;
  const WaveBounds wb = wave_bounds(my_last, range, s_cnt);
  const int n_eff = wb.n_eff;
  const int rounds = (n_eff + BATCH - 1) / BATCH;
  for (int r = 0; r < rounds; ++r) {
    __syncthreads();  // the previous batch has been consumed
    const int k = r * BATCH + tid;
    uint32_t m = 0u;
    if (tid < BATCH && k < n_eff) {
      const uint32_t e = point_list[range.x + k];
      const int64_t g = pl_id(e);
      // quadrants it can touch, and only the waves that still blend at this list position
      m = pl_mask(e) & wb.blending(k);
      s_r0[tid] = rec[RECS * g + 0];
      s_r1[tid] = rec[RECS * g + 1];
      const float4 r2 = rec[RECS * g + 2];
      const float4 t0 = trec[3 * g + 0], t1 = trec[3 * g + 1], t2 = trec[3 * g + 2];
      s_r2[tid] = make_float2(r2.x, r2.y);
      s_t0[tid] = t0;
      s_t1[tid] = t1;
      s_t2[tid] = make_float2(t2.x, t2.y);
    }
    publish_quad_masks(m, s_bits);
    __syncthreads();
    // this wave's hits in list order (latency is hidden by occupancy -- 8 waves per SIMD -- rather than
    // by register prefetch, which costs issue slots and occupancy)
    HitIter it(s_bits, w);
    for (int j = it.next(); j >= 0; j = it.next()) {
      const float4 a = s_r0[j], b = s_r1[j], t0 = s_t0[j], t1 = s_t1[j];
      const float2 cc = s_r2[j], t2 = s_t2[j];
      // all of the entry's primal and tangent record in one LDS round trip (the empty asm pins the
      // loads here; otherwise the tangent half is fetched inside the branch, a second exposed latency)
      asm volatile("" : : "v"(t0.z), "v"(t0.w), "v"(t1.x), "v"(t1.y), "v"(t1.z), "v"(t1.w), "v"(t2.x), "v"(b.z),
                   "v"(b.w), "v"(cc.x));
      const uint32_t pos = (uint32_t)(r * BATCH + j);
      const float dx = a.x - pxf, dy = a.y - pyf;
      const float power = gpower(a.z, a.w, b.x, dx, dy);
      const float G = gexp(power);
      const float alpha = fminf(0.99f, b.y * G);
      if (pos < my_last && !(power > 0.0f) && alpha >= 1.0f / 255.0f) {
        // the tangent arithmetic decides nothing (stop is frozen at the primal): FMA-contracted
#pragma clang fp contract(fast)
        float dpower = -0.5f * (t0.z * dx * dx + t1.x * dy * dy) - t0.w * dx * dy;
        if (WITH_XY) {
          const float ddx = t0.x, ddy = t0.y;
          dpower += -(a.z * dx * ddx + b.x * dy * ddy) - a.w * (ddx * dy + dx * ddy);
        }
        const float dalpha = G * (t1.y + b.y * dpower);
        const float wt = alpha * o.T;
        const float dw = dalpha * o.T + alpha * o.dT;
        o.dC[0] += t1.z * wt + b.z * dw;
        o.dC[1] += t1.w * wt + b.w * dw;
        o.dC[2] += t2.x * wt + cc.x * dw;
        if (WITH_INV) o.dD += t2.y * wt + cc.y * dw;
        o.dT = o.dT * (1.f - alpha) - o.T * dalpha;
        o.T = o.T * (1.f - alpha);
      }
    }
  }
}

// Front-to-back tangent pass of ONE wave over its 8x8 quadrant q, independent of the tile's other waves (no
// block barrier): 64 list positions per round, each lane fetches one; the entries whose quadrant mask holds q
// stage the compact LM record in the wave's own LDS slots (lane-indexed), and the wave walks the round's hit
// bits in list order.  The record: the primal's nine floats and the LM rows' compact tangent record (store_trec:
// [da db dc dop | dr dg db 0]) as 4 float4 at one LDS stride -- [x y a b], [c o r g], [blue da' db' dc'],
// [dop dr dg db] -- which the hit loop reads with one address register; the tangent conic carries its power
// factors (da' = -da / 2, db' = -db, dc' = -dc / 2).  A lane blends position pos only while pos < its own n_contrib
// (my_last): the skip and stop decisions are the primal's.
// DEPTH (k_render_matvec_depth): the record's 1/z is staged as a fifth, float plane sd (64 floats, the wave's own) and
// the visit adds dD += 1/z dw.  With xyz frozen 1/z has no tangent: the inverse depth moves through alpha only.
template <bool DEPTH = false>
__device__ __forceinline__ void jvp_wave_packed(JvpPix& o, float pxf, float pyf, uint32_t my_last, int wm, int q,
                                                const uint32_t* __restrict__ pl, const float4* __restrict__ rec,
                                                const float4* __restrict__ trec, float4* s, float* sd = nullptr) {
  const int lane = threadIdx.x & 63;
  o.T = 1.f;
  o.dT = 0.f;
  o.dC[0] = o.dC[1] = o.dC[2] = 0.f;
  o.dD = 0.f;
  for (int base = 0; base < wm; base += 64) {
    const int k = base + lane;
    bool hit = false;
    if (k < wm) {
      const uint32_t e = pl[k];
      if ((pl_mask(e) >> q) & 1u) {
        hit = true;
        const uint32_t g = pl_id(e);
        const float4 r0 = rec[RECS * (size_t)g + 0], r1 = rec[RECS * (size_t)g + 1], r2 = rec[RECS * (size_t)g + 2];
        const float4 c0 = trec[2 * (size_t)g + 0], c1 = trec[2 * (size_t)g + 1];
        s[lane] = r0;
        s[64 + lane] = r1;
        s[128 + lane] = make_float4(r2.x, -0.5f * c0.x, -c0.y, -0.5f * c0.z);  // blue, da', db', dc'
        s[192 + lane] = make_float4(c0.w, c1.x, c1.y, c1.z);                    // dopacity, dr, dg, db
        if constexpr (DEPTH) sd[lane] = r2.y;                                   // 1/z
      }
    }
    uint64_t hb = __ballot(hit);
    // pos = base + j < my_last as j < my_last - base: the lane's bound once per round, the hit's index compared as
    // the SGPR it is (no scalar add per visit)
    const int rel = (int)my_last - base;
    wave_lds_sync();
    while (hb) {
      const int j = (int)__builtin_ctzll(hb);
      hb = clear_bit(hb, j);
      const float4 a = s[j], b = s[64 + j], C = s[128 + j], D = s[192 + j];
      asm volatile("" : : "v"(b.z), "v"(b.w), "v"(C.x), "v"(C.y), "v"(C.z), "v"(C.w), "v"(D.x), "v"(D.y), "v"(D.z),
                   "v"(D.w));
      float invz = 0.f;
      if constexpr (DEPTH) {
        invz = sd[j];
        asm volatile("" : : "v"(invz));  // with the record's other loads
      }
      const float dx = a.x - pxf, dy = a.y - pyf;
      const float power = gpower(a.z, a.w, b.x, dx, dy);
      const float G = gexp(power);
      const float alpha = fminf(0.99f, b.y * G);
      if (j < rel && !(power > 0.0f) && alpha >= 1.0f / 255.0f) {
#pragma clang fp contract(fast)
        const float dpower = fmaf(dx, fmaf(C.y, dx, C.z * dy), C.w * dy * dy);  // 5 VALU, not 6
        const float dalpha = G * (D.x + b.y * dpower);
        const float wt = alpha * o.T;
        const float dw = dalpha * o.T + alpha * o.dT;
        // two FMAs into the accumulator per channel (not mul + fma + add)
        o.dC[0] = fmaf(b.z, dw, fmaf(D.y, wt, o.dC[0]));
        o.dC[1] = fmaf(b.w, dw, fmaf(D.z, wt, o.dC[1]));
        o.dC[2] = fmaf(C.x, dw, fmaf(D.w, wt, o.dC[2]));
        if constexpr (DEPTH) o.dD = fmaf(invz, dw, o.dD);
        o.dT = o.dT * (1.f - alpha) - o.T * dalpha;
        o.T = o.T * (1.f - alpha);
      }
    }
    wave_lds_sync();
  }
}

// jvp_wave_packed for the thread's wave on its own quadrant of tile p: the wave's bound (the largest n_contrib of its
// pixels, `last` being 0 outside the image; clamped by the range length as wave_bounds' n_eff is) and its 256 float4
// of the 4 x 256 at s_rec.  DEPTH: and its 64 floats of the 1/z plane behind them (s_rec + 1024: 4 x 64 floats).
template <bool DEPTH = false>
__device__ __forceinline__ void jvp_wave_quadrant(JvpPix& o, const TilePix& p, uint32_t last, uint2 range,
                                                  const uint32_t* __restrict__ point_list,
                                                  const float4* __restrict__ rec, const float4* __restrict__ trec,
                                                  float4* s_rec) {
  const int q = threadIdx.x >> 6;
  const int wm = __builtin_amdgcn_readfirstlane(min(wave_max_u((int)last), (int)(range.y - range.x)));
  if constexpr (DEPTH)
    jvp_wave_packed<true>(o, (float)p.px, (float)p.py, last, wm, q, point_list + range.x, rec, trec, s_rec + 256 * q,
                          reinterpret_cast<float*>(s_rec + 4 * 256) + 64 * q);
  else
    jvp_wave_packed(o, (float)p.px, (float)p.py, last, wm, q, point_list + range.x, rec, trec, s_rec + 256 * q);
}

// J v only, compact LM records, one independent wave per quadrant (jvp_wave_packed).
__global__ __launch_bounds__(256) void k_render_jv_wave(ViewK v, const uint2* __restrict__ ranges,
                                                         const uint32_t* __restrict__ tile_order,
                                                         const uint32_t* __restrict__ point_list,
                                                         const float4* __restrict__ rec, const float4* __restrict__ trec,
                                                         const uint32_t* __restrict__ n_contrib,
                                                         float* __restrict__ out_color_t) {
  __shared__ float4 s_rec[4 * 256];
  const TilePix p = tile_pix(v, tile_order);
  const int64_t pid = p.pid;
  const uint32_t last = p.inside ? n_contrib[pid] : 0u;
  JvpPix o;
  jvp_wave_quadrant(o, p, last, ranges[p.tile], point_list, rec, trec, s_rec);
  if (p.inside) {
    const int64_t HW = (int64_t)v.H * v.W;
    out_color_t[pid] = o.dC[0] + o.dT * v.bg[0];
    out_color_t[HW + pid] = o.dC[1] + o.dT * v.bg[1];
    out_color_t[2 * HW + pid] = o.dC[2] + o.dT * v.bg[2];
  }
}

template <bool WITH_XY>
__global__ __launch_bounds__(256) void k_render_jvp(ViewK v, const uint2* __restrict__ ranges,
                                                     const uint32_t* __restrict__ tile_order,
                                                     const uint32_t* __restrict__ point_list,
                                                     const float4* __restrict__ rec, const float4* __restrict__ trec,
                                                     const uint32_t* __restrict__ n_contrib,
                                                     float* __restrict__ out_color_t, float* __restrict__ out_inv_t) {
  constexpr int B = TILE_PIX;
  __shared__ float4 s_r0[B], s_r1[B], s_t0[B], s_t1[B];
  __shared__ float2 s_r2[B], s_t2[B];
  __shared__ uint64_t s_bits[16];
  __shared__ int s_cnt[4];
  const TilePix p = tile_pix(v, tile_order);
  const int64_t pid = p.pid;
  const uint32_t last = p.inside ? n_contrib[pid] : 0u;
  JvpPix o;
  jvp_tile<WITH_XY, true, B>(o, p.inside, (float)p.px, (float)p.py, last, ranges[p.tile], point_list, rec, trec, s_r0,
                             s_r1, s_r2, s_t0, s_t1, s_t2, s_bits, s_cnt);
  if (p.inside) {
    const int64_t HW = (int64_t)v.H * v.W;
    out_color_t[pid] = o.dC[0] + o.dT * v.bg[0];
    out_color_t[HW + pid] = o.dC[1] + o.dT * v.bg[1];
    out_color_t[2 * HW + pid] = o.dC[2] + o.dT * v.bg[2];
    if (out_inv_t) out_inv_t[pid] = o.dD;
  }
}

// The LDS plan of k_render_matvec<WITH_XY> (k_render_matvec_exposure uses <false>'s), in float4 of one region s.
// The JVP pass's records and the VJP pass's staged records and per-wave partials (+ its n_eff scratch) are never
// live together (vjp_tile starts with a block barrier).  Without screen-position tangents the JVP pass runs one
// independent wave per quadrant (jvp_wave_quadrant: 4 x 256 float4 of wave-private records from s); with them the
// block-cooperative jvp_tile, its primal records where vjp_tile's planes will be and its tangent records below.
template <bool WITH_XY>
struct MatvecLds {
  static constexpr int B = MATVEC_BATCH;
  // vjp_tile's partials, rounded up to 512 B: its record planes then start on a ds_read2st64 stride (no address add
  // per visit)
  static constexpr int kAcc = (vjp_acc_floats<WITH_XY, false, B>() + 3) / 4 + 31 & ~31;
  static constexpr int kVjp = kAcc + B + B + B / 2;  // + vjp_tile's 5 float2 planes (jvp_tile's r0, r1, r2)
  static constexpr int kJvp = WITH_XY ? 0 : 4 * 256;
  static constexpr int kFloat4 = kVjp > kJvp ? kVjp : kJvp;
  static_assert(!WITH_XY || kAcc >= 2 * B + B / 2, "jvp_tile's tangent records must fit below r0");
  static __device__ __forceinline__ float* acc(float4* s) { return reinterpret_cast<float*>(s); }
  static __device__ __forceinline__ int* misc(float4* s) { return reinterpret_cast<int*>(s); }  // before acc is written
  static __device__ __forceinline__ float2* planes(float4* s) { return reinterpret_cast<float2*>(s + kAcc); }
  static __device__ __forceinline__ float4* r0(float4* s) { return s + kAcc; }
  static __device__ __forceinline__ float4* r1(float4* s) { return s + kAcc + B; }
  static __device__ __forceinline__ float2* r2(float4* s) { return reinterpret_cast<float2*>(s + kAcc + 2 * B); }
  static __device__ __forceinline__ float4* t0(float4* s) { return s; }
  static __device__ __forceinline__ float4* t1(float4* s) { return s + B; }
  static __device__ __forceinline__ float2* t2(float4* s) { return reinterpret_cast<float2*>(s + 2 * B); }
};

// A pixel's inputs to the fused product: the primal's n_contrib and final T and the three channel weights (zeros
// outside the image).
struct MatvecPix {
  uint32_t last;
  float Tf, w0, w1, w2;
};
__device__ __forceinline__ MatvecPix load_matvec_pix(const ViewK& v, const TilePix& p,
                                                     const float* __restrict__ final_T,
                                                     const uint32_t* __restrict__ n_contrib,
                                                     const float* __restrict__ weight) {
  MatvecPix m{0u, 0.f, 0.f, 0.f, 0.f};
  if (p.inside) {
    const int64_t HW = (int64_t)v.H * v.W;
    m.last = n_contrib[p.pid];
    m.Tf = final_T[p.pid];
    m.w0 = weight[p.pid];
    m.w1 = weight[HW + p.pid];
    m.w2 = weight[2 * HW + p.pid];
  }
  return m;
}

// Fused (J^T W J) v for one view: JVP pass, per-pixel weight, VJP pass.
template <bool WITH_XY>
__global__ __launch_bounds__(256, WITH_XY ? 6 : 8) void k_render_matvec(ViewK v, const uint2* __restrict__ ranges,
                                                        const uint32_t* __restrict__ tile_order,
                                                        const uint32_t* __restrict__ point_list,
                                                        const float4* __restrict__ rec, const float4* __restrict__ trec,
                                                        const uint32_t* __restrict__ slots,
                                                        const uint2* __restrict__ rect,
                                                        const uint32_t* __restrict__ goff,
                                                        const float* __restrict__ final_T,
                                                        const uint32_t* __restrict__ n_contrib,
                                                        const float* __restrict__ weight, float4* __restrict__ contrib) {
  // 128-entry batches.  The LM instantiation (WITH_XY = false): 20.1 KB of LDS and 47 VGPRs -> 8 blocks per CU, 8
  // waves per SIMD (hipcc -Rpass-analysis=kernel-resource-usage; profiles/r04/resource_usage.txt); the drop-in
  // one (screen-position tangents): 23.8 KB, 64 VGPRs -> 6 blocks per CU
  using Lds = MatvecLds<WITH_XY>;
  constexpr int B = Lds::B;
  __shared__ uint64_t s_bits[16];
  __shared__ int s_cnt[4];
  __shared__ float4 s_lds[Lds::kFloat4];
  if (cg_stopped(v)) return;
  const TilePix p = tile_pix(v, tile_order);
  const uint2 range = ranges[p.tile];
  const MatvecPix m = load_matvec_pix(v, p, final_T, n_contrib, weight);
  JvpPix o;
  if constexpr (WITH_XY)
    jvp_tile<WITH_XY, false, B>(o, p.inside, (float)p.px, (float)p.py, m.last, range, point_list, rec, trec,
                                Lds::r0(s_lds), Lds::r1(s_lds), Lds::r2(s_lds), Lds::t0(s_lds), Lds::t1(s_lds),
                                Lds::t2(s_lds), s_bits, s_cnt);
  else
    jvp_wave_quadrant(o, p, m.last, range, point_list, rec, trec, s_lds);
  // u = 2 * w (.) (J v)   -- factor 2: the [r; r] residual aliasing of batch_training_loss.py:17
  const float u0 = 2.f * m.w0 * (o.dC[0] + o.dT * v.bg[0]);
  const float u1 = 2.f * m.w1 * (o.dC[1] + o.dT * v.bg[1]);
  const float u2 = 2.f * m.w2 * (o.dC[2] + o.dT * v.bg[2]);
  VjpPix st;
  vjp_init(st, v, p.inside, m.Tf, m.last, u0, u1, u2, 0.f);
  vjp_tile<WITH_XY, false, WITH_XY ? 3 : 2, B>(st, (float)p.px, (float)p.py, p.tile_x, p.tile_y, range, point_list, rec,
                                               slots, rect, goff, Lds::planes(s_lds), s_bits, Lds::acc(s_lds),
                                               Lds::misc(s_lds), contrib);
}

// k_render_matvec<false> under a trained per-camera exposure (GSLM_MV_EXPOSURE): between the two passes the
// 3x4 affine map of gaussian_renderer/__init__.py:113-119 and its transpose.  With dR = J v (the tangent pass's
// colour, background term included), R the forward's raw render, X the camera's exposure and V the direction's
// exposure rows:
//   dC_j = ((dR_0 X[0][j] + dR_1 X[1][j]) + dR_2 X[2][j]) + (((R_0 V[0][j] + R_1 V[1][j]) + R_2 V[2][j]) + V[j][3])
//   u_j  = 2 w_j dC_j                     -> ex.u (the exposure rows sum R_i u_j and u_j in a streaming pass of their
//                                            own: this kernel is VALU- and occupancy-bound, a 12-sum block reduction
//                                            does not belong in it)
//   ub_i = (X[i][0] u_0 + X[i][1] u_1) + X[i][2] u_2      the back-to-front pass's seed
// X and V are wave-uniform loads.  With X = [I | 0] and V = 0 every product is by 1 or 0: the rows are those of
// k_render_matvec<false>.
__global__ __launch_bounds__(256, 8) void k_render_matvec_exposure(
    ViewK v, const uint2* __restrict__ ranges, const uint32_t* __restrict__ tile_order,
    const uint32_t* __restrict__ point_list, const float4* __restrict__ rec, const float4* __restrict__ trec,
    const uint32_t* __restrict__ slots, const uint2* __restrict__ rect, const uint32_t* __restrict__ goff,
    const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib, const float* __restrict__ weight,
    float4* __restrict__ contrib, ExposureK ex) {
  using Lds = MatvecLds<false>;
  __shared__ uint64_t s_bits[16];
  __shared__ float4 s_lds[Lds::kFloat4];
  if (cg_stopped(v)) return;
  const TilePix p = tile_pix(v, tile_order);
  const int64_t pid = p.pid;
  const int64_t HW = (int64_t)v.H * v.W;
  const uint2 range = ranges[p.tile];
  const MatvecPix m = load_matvec_pix(v, p, final_T, n_contrib, weight);
  JvpPix o;
  jvp_wave_quadrant(o, p, m.last, range, point_list, rec, trec, s_lds);
  // the forward's colour: loaded after the tangent pass (three registers it need not carry)
  float R0 = 0.f, R1 = 0.f, R2 = 0.f;
  if (p.inside) {
    R0 = ex.color[pid];
    R1 = ex.color[HW + pid];
    R2 = ex.color[2 * HW + pid];
  }
  const float* __restrict__ X = ex.X;
  const float* __restrict__ V = ex.V;
  const float dR0 = o.dC[0] + o.dT * v.bg[0];
  const float dR1 = o.dC[1] + o.dT * v.bg[1];
  const float dR2 = o.dC[2] + o.dT * v.bg[2];
  const float dC0 = ((dR0 * X[0] + dR1 * X[4]) + dR2 * X[8]) + (((R0 * V[0] + R1 * V[4]) + R2 * V[8]) + V[3]);
  const float dC1 = ((dR0 * X[1] + dR1 * X[5]) + dR2 * X[9]) + (((R0 * V[1] + R1 * V[5]) + R2 * V[9]) + V[7]);
  const float dC2 = ((dR0 * X[2] + dR1 * X[6]) + dR2 * X[10]) + (((R0 * V[2] + R1 * V[6]) + R2 * V[10]) + V[11]);
  // u = 2 * w (.) dC   -- factor 2: the [r; r] residual aliasing of batch_training_loss.py:17
  const float u0 = 2.f * m.w0 * dC0;
  const float u1 = 2.f * m.w1 * dC1;
  const float u2 = 2.f * m.w2 * dC2;
  if (p.inside) {
    ex.u[pid] = u0;
    ex.u[HW + pid] = u1;
    ex.u[2 * HW + pid] = u2;
  }
  const float ub0 = (X[0] * u0 + X[1] * u1) + X[2] * u2;
  const float ub1 = (X[4] * u0 + X[5] * u1) + X[6] * u2;
  const float ub2 = (X[8] * u0 + X[9] * u1) + X[10] * u2;
  VjpPix st;
  vjp_init(st, v, p.inside, m.Tf, m.last, ub0, ub1, ub2, 0.f);
  vjp_tile<false, false, 2, Lds::B>(st, (float)p.px, (float)p.py, p.tile_x, p.tile_y, range, point_list, rec, slots,
                                    rect, goff, Lds::planes(s_lds), s_bits, Lds::acc(s_lds), Lds::misc(s_lds), contrib);
}

// k_render_matvec<false> with an inverse-depth residual (GSLM_MV_DEPTH): weight is [4, H, W], its fourth plane
// w3 = lambda_d m_d^2.  The J v pass carries dD = sum 1/z dw (jvp_wave_packed<true>; the inverse depth has no background
// term), u3 = w3 dD -- the depth block enters the loss once: no factor 2 -- seeds the back-to-front pass's dinv, and
// vjp_tile's "seed only" form folds <1/z, u3> into dL/dalpha.  The LM rows, the row map and the LDS (the 1/z plane
// lies in the 224 float4 between the J v pass's records and kVjp) are k_render_matvec<false>'s; with w3 = 0 so are
// the rows' bits (cd + 1/z 0 = cd).
__global__ __launch_bounds__(256, 8) void k_render_matvec_depth(
    ViewK v, const uint2* __restrict__ ranges, const uint32_t* __restrict__ tile_order,
    const uint32_t* __restrict__ point_list, const float4* __restrict__ rec, const float4* __restrict__ trec,
    const uint32_t* __restrict__ slots, const uint2* __restrict__ rect, const uint32_t* __restrict__ goff,
    const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib, const float* __restrict__ weight,
    float4* __restrict__ contrib) {
  using Lds = MatvecLds<false>;
  static_assert(Lds::kFloat4 >= 4 * 256 + 64, "the 1/z plane fits behind the J v pass's records");
  __shared__ uint64_t s_bits[16];
  __shared__ float4 s_lds[Lds::kFloat4];
  if (cg_stopped(v)) return;
  const TilePix p = tile_pix(v, tile_order);
  const uint2 range = ranges[p.tile];
  const MatvecPix m = load_matvec_pix(v, p, final_T, n_contrib, weight);
  const float w3 = p.inside ? weight[3 * ((int64_t)v.H * v.W) + p.pid] : 0.f;
  JvpPix o;
  jvp_wave_quadrant<true>(o, p, m.last, range, point_list, rec, trec, s_lds);
  const float u0 = 2.f * m.w0 * (o.dC[0] + o.dT * v.bg[0]);
  const float u1 = 2.f * m.w1 * (o.dC[1] + o.dT * v.bg[1]);
  const float u2 = 2.f * m.w2 * (o.dC[2] + o.dT * v.bg[2]);
  const float u3 = w3 * o.dD;
  VjpPix st;
  vjp_init(st, v, p.inside, m.Tf, m.last, u0, u1, u2, u3);
  vjp_tile<false, false, 2, Lds::B, true>(st, (float)p.px, (float)p.py, p.tile_x, p.tile_y, range, point_list, rec,
                                          slots, rect, goff, Lds::planes(s_lds), s_bits, Lds::acc(s_lds),
                                          Lds::misc(s_lds), contrib);
}

// ------------------------------------------------------------------ launchers
int launch_jvp(const ViewK& v, const GaussK& g, const GaussK& t, const float* m2t, const GeomBufs& gb,
               const BinBufs& bb, const ImgBufs& ib, const ScratchBufs& sb, float* out_color_t, float* out_inv_t,
               hipStream_t s) {
  int st = launch_tangent_pre(v, g, t, m2t, gb, sb, nullptr, s, false);  // the drop-in JVP: 12-float records
  if (st) return st;
  const int ntiles = v.gx * v.gy;
  const bool xy = t.means3D != nullptr || m2t != nullptr;
  if (xy)
    hipLaunchKernelGGL(k_render_jvp<true>, dim3(ntiles), dim3(TILE_PIX), 0, s, v, bb.ranges, bb.tile_order, bb.point_list, gb.rec,
                       sb.trec, ib.n_contrib, out_color_t, out_inv_t);
  else
    hipLaunchKernelGGL(k_render_jvp<false>, dim3(ntiles), dim3(TILE_PIX), 0, s, v, bb.ranges, bb.tile_order, bb.point_list, gb.rec,
                       sb.trec, ib.n_contrib, out_color_t, out_inv_t);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

int launch_render_jv(const ViewK& v, const GaussK& t, const GeomBufs& gb, const BinBufs& bb, const ImgBufs& ib,
                     const ScratchBufs& sb, bool mask_xyz, float* jv_out, hipStream_t s) {
  const int ntiles = v.gx * v.gy;
  if (mask_xyz)  // the TANGENT stage of the LM rows wrote compact records
    hipLaunchKernelGGL(k_render_jv_wave, dim3(ntiles), dim3(TILE_PIX), 0, s, v, bb.ranges, bb.tile_order,
                       bb.point_list, gb.rec, sb.trec, ib.n_contrib, jv_out);
  else
    hipLaunchKernelGGL(k_render_jvp<true>, dim3(ntiles), dim3(TILE_PIX), 0, s, v, bb.ranges, bb.tile_order,
                       bb.point_list, gb.rec, sb.trec, ib.n_contrib, jv_out, (float*)nullptr);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

int launch_matvec_render(const ViewK& v, const GaussK& t, const GeomBufs& gb, const BinBufs& bb, const ImgBufs& ib,
                         const ScratchBufs& sb, int64_t N, const float* weight, bool mask_xyz, bool tail_clean,
                         hipStream_t s, bool depth) {
  const int ntiles = v.gx * v.gy;
  // the LM row map (head entries only; ScratchBufs::hscan): computed by the first product on a geometry
  if (!tail_clean) {
    const int st = launch_lm_rowmap(v, gb, bb, ib, sb, N, s);
    if (st) return st;
  }
  if (depth && mask_xyz)
    hipLaunchKernelGGL(k_render_matvec_depth, dim3(ntiles), dim3(TILE_PIX), 0, s, v, bb.ranges, bb.tile_order,
                       bb.point_list, gb.rec, sb.trec, bb.slots, gb.rect, gb.goff, ib.final_T, ib.n_contrib, weight,
                       sb.contrib);
  else if (mask_xyz)
    hipLaunchKernelGGL(k_render_matvec<false>, dim3(ntiles), dim3(TILE_PIX), 0, s, v, bb.ranges, bb.tile_order, bb.point_list,
                       gb.rec, sb.trec, bb.slots, gb.rect, gb.goff, ib.final_T, ib.n_contrib, weight,
                       sb.contrib);
  else
    hipLaunchKernelGGL(k_render_matvec<true>, dim3(ntiles), dim3(TILE_PIX), 0, s, v, bb.ranges, bb.tile_order, bb.point_list,
                       gb.rec, sb.trec, bb.slots, gb.rect, gb.goff, ib.final_T, ib.n_contrib, weight,
                       sb.contrib);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

int launch_matvec_render_exposure(const ViewK& v, const GaussK& t, const GeomBufs& gb, const BinBufs& bb,
                                  const ImgBufs& ib, const ScratchBufs& sb, int64_t N, const float* weight,
                                  const ExposureK& ex, bool tail_clean, hipStream_t s) {
  const int ntiles = v.gx * v.gy;
  if (!tail_clean) {
    const int st = launch_lm_rowmap(v, gb, bb, ib, sb, N, s);
    if (st) return st;
  }
  hipLaunchKernelGGL(k_render_matvec_exposure, dim3(ntiles), dim3(TILE_PIX), 0, s, v, bb.ranges, bb.tile_order,
                     bb.point_list, gb.rec, sb.trec, bb.slots, gb.rect, gb.goff, ib.final_T, ib.n_contrib, weight,
                     sb.contrib, ex);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

}  // namespace gslm
