// residual.hip -- the LM residual epilogue of one view in one pass.
//
// Reference (disable_ssim=True, train_jvp.py:212): batch_render clamps the render to [0, 1]
// (gaussian_renderer/batch_render.py:118), compute_batch_loss_block multiplies by the alpha mask and
// subtracts the ground truth (solver/batch_training_loss.py:10-17, 56-67), the "ssim" slot aliases
// the L1 slot, and loss_scalar = ||r||^2 + ||r||^2 (solver/loss_image_state.py:16-19).  The
// reference pads every view to the batch's max H x W; padded pixels carry r = 0 and contribute
// nothing, so each view is processed at its own size here.
//
// Per pixel p and channel c, R = color, m = alpha mask (1 when absent), g = ground truth:
//   r      = m clamp(R, 0, 1) - g                      residual
//   w      = m m 1[0 <= R <= 1]                       weight of J^T J (d r / d R squared)
//   seed   = -2 m 1[0 <= R <= 1] r                    dL/dR of J^T b, b = -[r; r]  (the rhs backward input)
//   loss  += 2 sum r^2                                 (double, block partials + one final pass)
// The float expressions follow the torch ones in gslm/lm.py's reference restatement operation by
// operation, so r, w and seed are bit-identical to it.
#include <algorithm>
#include <cmath>

#include "gslm_kernels.hpp"

namespace gslm {

constexpr int RES_THREADS = 256;

// ROBUST (gslm_lm_residual_robust; rb a checked HUBER / CAUCHY block, robust_weight / robust_rho of gslm_kernels.hpp):
//   w = ((m m) inside) rho',   seed = (((-2 m) inside) r) rho',   loss += 2 sum rho     -- r itself is stored unscaled.
// The plain instantiation reads no rb and is the kernel it was.
template <bool ROBUST>
__global__ __launch_bounds__(RES_THREADS) void k_lm_residual(int64_t HW, const float* __restrict__ color,
                                                             const float* __restrict__ gt,
                                                             const float* __restrict__ mask,
                                                             float* __restrict__ residual, float* __restrict__ weight,
                                                             float* __restrict__ seed, double* __restrict__ part,
                                                             gslm_robust rb) {
  __shared__ double s[RES_THREADS / 64];
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * RES_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * RES_THREADS + threadIdx.x; p < HW; p += stride) {
    const float m = mask ? mask[p] : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t k = c * HW + p;
      const float R = color[k];
      const float inside = (R >= 0.0f && R <= 1.0f) ? 1.0f : 0.0f;
      const float r = m * clamp01(R) - gt[k];
      if (residual) residual[k] = r;
      if constexpr (ROBUST) {
        const float dr = robust_weight(rb, r);
        if (weight) weight[k] = ((m * m) * inside) * dr;
        if (seed) seed[k] = (((-2.0f * m) * inside) * r) * dr;
        acc += robust_rho(rb, r);
      } else {
        if (weight) weight[k] = (m * m) * inside;
        if (seed) seed[k] = ((-2.0f * m) * inside) * r;
        acc += (double)r * (double)r;
      }
    }
  }
  const double sum = block_sum4(acc, s);
  if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

__global__ __launch_bounds__(RES_THREADS) void k_lm_loss_final(const double* __restrict__ part, int np, int accumulate,
                                                               double* __restrict__ loss) {
  __shared__ double s[RES_THREADS / 64];
  const double sum = block_sum4(strided_sum_in_order(part, np), s);
  if (threadIdx.x == 0) {
    const double l = 2.0 * sum;  // [r; r] aliasing
    *loss = accumulate ? *loss + l : l;
  }
}

// ---- the inverse-depth block (gslm_lm_residual_depth; the reference's Ll1depth_per_pixel slot, as a least-squares
// block that enters the loss once) ----
// Per pixel p, D = the rendered inverse depth (no background term, no clamp), g = its target, m = the depth mask
// (1 when absent), lam = (float)depth_weight:
//   r     = m * (D - g)                 one subtraction, one product
//   w     = lam * (m * m)               weight of J_D^T W_d J_D
//   seed  = -w * r                      (-w) * r: the negation is exact; dL/dD of J^T b
//   loss += (double)depth_weight * ((double)r * (double)r)      per pixel; block partials, then k_lm_depth_loss_final
// in this order, uncontracted.  With a mask of zeros and ones -w r = -lam m^2 (D - g), the right-hand side's term.
__global__ __launch_bounds__(RES_THREADS) void k_lm_residual_depth(int64_t HW, const float* __restrict__ invdepth,
                                                                   const float* __restrict__ gt,
                                                                   const float* __restrict__ mask, float lam,
                                                                   double lam_d, float* __restrict__ residual,
                                                                   float* __restrict__ weight, float* __restrict__ seed,
                                                                   double* __restrict__ part) {
  __shared__ double s[RES_THREADS / 64];
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * RES_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * RES_THREADS + threadIdx.x; p < HW; p += stride) {
    const float m = mask ? mask[p] : 1.0f;
    const float r = m * (invdepth[p] - gt[p]);
    const float w = lam * (m * m);
    if (residual) residual[p] = r;
    if (weight) weight[p] = w;
    if (seed) seed[p] = (-w) * r;
    acc += lam_d * ((double)r * (double)r);
  }
  const double sum = block_sum4(acc, s);
  if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// k_lm_loss_final without the [r; r] factor: the depth block enters the loss once
__global__ __launch_bounds__(RES_THREADS) void k_lm_depth_loss_final(const double* __restrict__ part, int np,
                                                                     int accumulate, double* __restrict__ loss) {
  __shared__ double s[RES_THREADS / 64];
  const double sum = block_sum4(strided_sum_in_order(part, np), s);
  if (threadIdx.x == 0) *loss = accumulate ? *loss + sum : sum;
}

// ---- the same epilogue under a trained per-camera exposure (gaussian_renderer/__init__.py:113-119) ----
// X = the camera's 3x4 exposure, row-major [i][k].  Per pixel, R the raw render:
//   C_j    = ((R_0 X[0][j] + R_1 X[1][j]) + R_2 X[2][j]) + X[j][3]       exposed colour
//   r_j    = m clamp(C_j, 0, 1) - g_j,   w_j = m m 1[0 <= C_j <= 1],   sC_j = -2 m 1[0 <= C_j <= 1] r_j
//   seed_i = (X[i][0] sC_0 + X[i][1] sC_1) + X[i][2] sC_2                dL/dR of J^T b (the pixel_seed pass's input)
//   G[i][j] += R_i sC_j,  G[j][3] += sC_j                                the exposure rows of J^T b
// (products and sums in this order, uncontracted: r, w and seed are bit-identical to the torch restatement, and with
// X = [I | 0] to k_lm_residual's.)  The 12 row sums and the loss: double block partials, one final pass in fixed order.
constexpr int EXP_PART = 1024;  // partials per sum: part[k * EXP_PART + block]

// rows[4 i + j] += R_i u_j, rows[4 j + 3] += u_j
__device__ __forceinline__ void exposure_rows_add(double* rows, float R0, float R1, float R2, float u0, float u1,
                                                  float u2) {
  const double R[3] = {(double)R0, (double)R1, (double)R2}, u[3] = {(double)u0, (double)u1, (double)u2};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) rows[4 * i + j] += R[i] * u[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) rows[4 * j + 3] += u[j];
}

// the block's sum of each acc[k] -> part[k * EXP_PART + blockIdx.x]  (s: N * RES_THREADS / 64 doubles of LDS)
template <int N>
__device__ __forceinline__ void block_sums_store(double* acc, double* s, double* __restrict__ part) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // wave_sum_store's tree, written out: called here it costs k_lm_residual_exposure four VGPRs (80 for 76)
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double a = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
    if (lane == 0) s[4 * k + w] = a;
  }
  __syncthreads();
  if (tid < N) part[tid * EXP_PART + blockIdx.x] = sum4(s + 4 * tid);
}

__global__ __launch_bounds__(RES_THREADS) void k_lm_residual_exposure(
    int64_t HW, const float* __restrict__ color, const float* __restrict__ gt, const float* __restrict__ mask,
    const float* __restrict__ X, float* __restrict__ residual, float* __restrict__ weight, float* __restrict__ seed,
    int want_rows, double* __restrict__ part) {
  __shared__ double s[13 * RES_THREADS / 64];
  double acc[13];
#pragma unroll
  for (int k = 0; k < 13; ++k) acc[k] = 0.0;
  float x[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) x[k] = X[k];  // wave-uniform
  const int64_t stride = (int64_t)gridDim.x * RES_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * RES_THREADS + threadIdx.x; p < HW; p += stride) {
    const float m = mask ? mask[p] : 1.0f;
    const float R0 = color[p], R1 = color[HW + p], R2 = color[2 * HW + p];
    float sC[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int64_t k = j * HW + p;
      const float C = ((R0 * x[j] + R1 * x[4 + j]) + R2 * x[8 + j]) + x[4 * j + 3];
      const float inside = (C >= 0.0f && C <= 1.0f) ? 1.0f : 0.0f;
      const float r = m * clamp01(C) - gt[k];
      if (residual) residual[k] = r;
      if (weight) weight[k] = (m * m) * inside;
      sC[j] = ((-2.0f * m) * inside) * r;
      acc[12] += (double)r * (double)r;
    }
    if (seed) {
#pragma unroll
      for (int i = 0; i < 3; ++i) seed[i * HW + p] = (x[4 * i] * sC[0] + x[4 * i + 1] * sC[1]) + x[4 * i + 2] * sC[2];
    }
    if (want_rows) exposure_rows_add(acc, R0, R1, R2, sC[0], sC[1], sC[2]);
  }
  block_sums_store<13>(acc, s, part);
}

// u -> the exposure rows of one view's product: the 12 sums of R_i u_j and u_j over the image
__global__ __launch_bounds__(RES_THREADS) void k_exposure_rows(int64_t HW, const float* __restrict__ color,
                                                               const float* __restrict__ u, const double* stop,
                                                               double* __restrict__ part) {
  __shared__ double s[12 * RES_THREADS / 64];
  if (stop != nullptr && *stop != 0.0) return;
  double acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * RES_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * RES_THREADS + threadIdx.x; p < HW; p += stride)
    exposure_rows_add(acc, color[p], color[HW + p], color[2 * HW + p], u[p], u[HW + p], u[2 * HW + p]);
  block_sums_store<12>(acc, s, part);
}

// out[k] = [out[k] unless overwrite] + damp v[k] + (float) sum of part[k][0 .. np), k = blockIdx.x < 12 (v may be NULL)
__global__ __launch_bounds__(RES_THREADS) void k_exposure_rows_final(const double* __restrict__ part, int np,
                                                                     const float* __restrict__ v, float damp,
                                                                     int overwrite, const double* stop,
                                                                     float* __restrict__ out) {
  __shared__ double s[RES_THREADS / 64];
  if (stop != nullptr && *stop != 0.0) return;
  const int k = blockIdx.x;
  const float sum = (float)block_sum4(strided_sum_in_order(part + (size_t)k * EXP_PART, np), s);
  if (threadIdx.x == 0) {
    float base = overwrite ? 0.0f : out[k];
    if (v) base += damp * v[k];
    out[k] = base + sum;
  }
}

// the tile pass's exposure step for a view with an empty list (no tile kernel runs): J v = 0, so
// u_j = 2 w_j (((R_0 V[0][j] + R_1 V[1][j]) + R_2 V[2][j]) + V[j][3])
__global__ __launch_bounds__(RES_THREADS) void k_exposure_u_empty(int64_t HW, const float* __restrict__ color,
                                                                  const float* __restrict__ weight,
                                                                  const float* __restrict__ V, const double* stop,
                                                                  float* __restrict__ u) {
  if (stop != nullptr && *stop != 0.0) return;
  const int64_t p = (int64_t)blockIdx.x * RES_THREADS + threadIdx.x;
  if (p >= HW) return;
  const float R0 = color[p], R1 = color[HW + p], R2 = color[2 * HW + p];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float dC = 0.0f + (((R0 * V[j] + R1 * V[4 + j]) + R2 * V[8 + j]) + V[4 * j + 3]);
    u[j * HW + p] = 2.f * weight[j * HW + p] * dC;
  }
}

static int exposure_grid(int64_t HW) {
  return (int)std::min<int64_t>(EXP_PART, std::max<int64_t>(1, (HW + RES_THREADS - 1) / RES_THREADS));
}

int launch_exposure_u_empty(int H, int W, const float* color, const float* weight, const float* V, const double* stop,
                            float* u, hipStream_t s) {
  const int64_t HW = (int64_t)H * W;
  if (HW == 0) return GSLM_OK;
  hipLaunchKernelGGL(k_exposure_u_empty, dim3((unsigned)((HW + RES_THREADS - 1) / RES_THREADS)), dim3(RES_THREADS), 0,
                     s, HW, color, weight, V, stop, u);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

int launch_exposure_rows(int H, int W, const float* color, const float* u, const float* v_rows, float damp,
                         bool overwrite, const double* stop, double* part, float* y_rows, hipStream_t s) {
  const int64_t HW = (int64_t)H * W;
  const int nb = exposure_grid(HW);
  hipLaunchKernelGGL(k_exposure_rows, dim3(nb), dim3(RES_THREADS), 0, s, HW, color, u, stop, part);
  GSLM_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_exposure_rows_final, dim3(12), dim3(RES_THREADS), 0, s, part, nb, v_rows, damp,
                     overwrite ? 1 : 0, stop, y_rows);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

}  // namespace gslm

using namespace gslm;

extern "C" {

size_t gslm_residual_scratch_bytes(int32_t H, int32_t W) {
  (void)H;
  (void)W;
  return (size_t)1024 * sizeof(double);
}

// gslm_lm_residual and its robust form: one body, `robust` NULL for the plain one
static int lm_residual(int32_t H, int32_t W, const float* color, const float* gt, const float* alpha_mask,
                       const gslm_robust* robust, float* residual, float* weight, float* seed, void* scratch,
                       size_t scratch_bytes, double* loss_dev, int32_t accumulate, void* stream) {
  bool on = false;
  gslm_robust rb{};
  if (int st = robust_arg(robust, "lm_residual_robust", &on, &rb)) return st;
  if (H < 0 || W < 0) { set_error("lm_residual: negative image size"); return GSLM_ERR_INVALID; }
  const int64_t HW = (int64_t)H * W;
  if (HW > 0 && (!color || !gt)) { set_error("lm_residual: NULL color / gt"); return GSLM_ERR_INVALID; }
  if (!loss_dev || !scratch) { set_error("lm_residual: NULL loss or scratch"); return GSLM_ERR_INVALID; }
  if (scratch_bytes < gslm_residual_scratch_bytes(H, W)) { set_error("lm_residual: scratch too small"); return GSLM_ERR_CAPACITY; }
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (HW + RES_THREADS - 1) / RES_THREADS));
  double* part = (double*)scratch;
  if (on)
    hipLaunchKernelGGL(k_lm_residual<true>, dim3(nb), dim3(RES_THREADS), 0, s, HW, color, gt, alpha_mask, residual,
                       weight, seed, part, rb);
  else
    hipLaunchKernelGGL(k_lm_residual<false>, dim3(nb), dim3(RES_THREADS), 0, s, HW, color, gt, alpha_mask, residual,
                       weight, seed, part, rb);
  GSLM_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_lm_loss_final, dim3(1), dim3(RES_THREADS), 0, s, part, nb, accumulate ? 1 : 0, loss_dev);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}

int gslm_lm_residual(int32_t H, int32_t W, const float* color, const float* gt, const float* alpha_mask,
                     float* residual, float* weight, float* seed, void* scratch, size_t scratch_bytes,
                     double* loss_dev, int32_t accumulate, void* stream) {
  return lm_residual(H, W, color, gt, alpha_mask, nullptr, residual, weight, seed, scratch, scratch_bytes, loss_dev,
                     accumulate, stream);
}

int gslm_lm_residual_robust(int32_t H, int32_t W, const float* color, const float* gt, const float* alpha_mask,
                            const gslm_robust* robust, float* residual, float* weight, float* seed, void* scratch,
                            size_t scratch_bytes, double* loss_dev, int32_t accumulate, void* stream) {
  return lm_residual(H, W, color, gt, alpha_mask, robust, residual, weight, seed, scratch, scratch_bytes, loss_dev,
                     accumulate, stream);
}

int gslm_lm_residual_depth(int32_t H, int32_t W, const float* invdepth, const float* invdepth_gt,
                           const float* depth_mask, double depth_weight, float* residual, float* weight, float* seed,
                           void* scratch, size_t scratch_bytes, double* loss_dev, int32_t accumulate, void* stream) {
  if (H < 0 || W < 0) { set_error("lm_residual_depth: negative image size"); return GSLM_ERR_INVALID; }
  const int64_t HW = (int64_t)H * W;
  if (HW > 0 && (!invdepth || !invdepth_gt)) { set_error("lm_residual_depth: NULL invdepth / invdepth_gt"); return GSLM_ERR_INVALID; }
  if (!(depth_weight >= 0.0) || !std::isfinite(depth_weight)) {
    set_error("lm_residual_depth: depth_weight must be finite and >= 0");
    return GSLM_ERR_INVALID;
  }
  if (!loss_dev || !scratch) { set_error("lm_residual_depth: NULL loss or scratch"); return GSLM_ERR_INVALID; }
  if (scratch_bytes < gslm_residual_scratch_bytes(H, W)) { set_error("lm_residual_depth: scratch too small"); return GSLM_ERR_CAPACITY; }
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (HW + RES_THREADS - 1) / RES_THREADS));
  double* part = (double*)scratch;
  hipLaunchKernelGGL(k_lm_residual_depth, dim3(nb), dim3(RES_THREADS), 0, s, HW, invdepth, invdepth_gt, depth_mask,
                     (float)depth_weight, depth_weight, residual, weight, seed, part);
  GSLM_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_lm_depth_loss_final, dim3(1), dim3(RES_THREADS), 0, s, part, nb, accumulate ? 1 : 0, loss_dev);
  GSLM_LAUNCH_CHECK();
  return GSLM_OK;
}


size_t gslm_exposure_scratch_bytes(int32_t H, int32_t W) {
  (void)H;
  (void)W;
  return (size_t)13 * EXP_PART * sizeof(double);
}

int gslm_lm_residual_exposure(int32_t H, int32_t W, const float* color, const float* gt, const float* alpha_mask,
                              const float* exposure, float* residual, float* weight, float* seed, float* rhs_rows,
                              void* scratch, size_t scratch_bytes, double* loss_dev, int32_t accumulate,
                              void* stream) {
  if (H < 0 || W < 0) { set_error("lm_residual_exposure: negative image size"); return GSLM_ERR_INVALID; }
  const int64_t HW = (int64_t)H * W;
  if (HW > 0 && (!color || !gt)) { set_error("lm_residual_exposure: NULL color / gt"); return GSLM_ERR_INVALID; }
  if (!exposure) { set_error("lm_residual_exposure: NULL exposure (12 device floats)"); return GSLM_ERR_INVALID; }
  if (!loss_dev || !scratch) { set_error("lm_residual_exposure: NULL loss or scratch"); return GSLM_ERR_INVALID; }
  if (scratch_bytes < gslm_exposure_scratch_bytes(H, W)) {
    set_error("lm_residual_exposure: scratch too small");
    return GSLM_ERR_CAPACITY;
  }
  hipStream_t s = (hipStream_t)stream;
  const int nb = exposure_grid(HW);
  double* part = (double*)scratch;
  hipLaunchKernelGGL(k_lm_residual_exposure, dim3(nb), dim3(RES_THREADS), 0, s, HW, color, gt, alpha_mask, exposure,
                     residual, weight, seed, rhs_rows ? 1 : 0, part);
  GSLM_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_lm_loss_final, dim3(1), dim3(RES_THREADS), 0, s, part + (size_t)12 * EXP_PART, nb,
                     accumulate ? 1 : 0, loss_dev);
  GSLM_LAUNCH_CHECK();
  if (rhs_rows) {
    hipLaunchKernelGGL(k_exposure_rows_final, dim3(12), dim3(RES_THREADS), 0, s, part, nb, (const float*)nullptr, 0.0f,
                       0, (const double*)nullptr, rhs_rows);
    GSLM_LAUNCH_CHECK();
  }
  return GSLM_OK;
}

}  // extern "C"
