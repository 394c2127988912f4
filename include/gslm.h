/*
 * gslm.h -- C ABI of the MI355X-native Gaussian-splat rasterizer + LM normal-equations matvec.
 *
 * Drop-in boundary.  The reference binds its rasterizer through pybind11
 * (`diff_gaussian_rasterization._C`, absent submodule) from the Python call sites below; every
 * entry point here replaces one of those calls:
 *
 *   gslm_preprocess + gslm_rasterize (= gslm_forward)
 *        <- GaussianRasterizer.forward, called at gaussian_renderer/__init__.py:102-110,
 *           gaussian_renderer/batch_render.py:100-108, gaussian_renderer/reference_render.py:102
 *   gslm_backward   <- autograd backward of the rasterizer, driven by loss_image_state.py:93-97
 *                      from solver/solver_functions.py:119 (matvec_T)
 *   gslm_jvp        <- forward-mode tangent of the rasterizer (fork), driven by fwAD at
 *                      solver/solver_functions.py:86-92 (matvec)
 *   gslm_matvec_view<- fused (J^T W J) v of one view: solver_functions.py:83-132 matvec followed
 *                      by matvec_T with the disable_ssim residual of batch_training_loss.py:10-17
 *   gslm_cg_*       <- GaussianModelState dot / saxpy (solver/gaussian_model_state.py:197-273)
 *                      used by cgls_damped (solver/conjugate_gradient.py:51-127), device resident
 *
 * Conventions: raw device pointers, sizes, a settings POD and a hipStream_t (passed as void*).
 * Every function returns GSLM_OK (0) or a negative status; gslm_last_error() describes the last
 * failure.  No internal threads, no allocation (the caller allocates workspaces sized by the
 * *_bytes queries), stream ordered, not re-entrant on one workspace.  Only gslm_num_rendered(_many) and
 * gslm_forward (which calls it) synchronise the stream (the upstream forward does the same to
 * size its binning buffers); the *_dev rasterize forms do not.
 */
#ifndef GSLM_H
#define GSLM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSLM_OK 0
#define GSLM_ERR_INVALID (-1)
#define GSLM_ERR_HIP (-2)
#define GSLM_ERR_CAPACITY (-3) /* a workspace is too small; the required size is reported */

#define GSLM_ABI_VERSION 9

/* GaussianRasterizationSettings (gaussian_renderer/__init__.py:36-50) as a POD. */
typedef struct gslm_view {
  int32_t image_height;
  int32_t image_width;
  double tanfovx;
  double tanfovy;
  double scale_modifier;
  float viewmatrix[16]; /* world_view_transform, row-major torch storage (= column-major for the kernel) */
  float projmatrix[16]; /* full_proj_transform */
  float campos[3];
  float bg[3];
  int32_t sh_degree;    /* active SH degree D */
  int32_t prefiltered;
  int32_t antialiasing;
  int32_t debug;        /* nonzero (the settings' `debug`, arguments/__init__.py:70): upstream's debug mode --
                           gslm_preprocess / _rasterize(_dev) / _forward / _backward / _jvp / _matvec_view_ex
                           synchronise their stream after every kernel and fail at the launch that faulted
                           (gslm_last_error names its source line) -- and the exhaustive tile traversal: every
                           wave visits every list entry, as upstream does (the quadrant cull is off; results are
                           bit-identical either way) */
} gslm_view;

/* Per-Gaussian inputs.  With raw = 0 they are the activated tensors the rasterizer receives
 * (means3D, opacities = sigmoid, scales = exp, rotations = normalize, shs = cat(dc, rest));
 * with raw = 1 they are the GaussianModel leaves (_xyz, _opacity, _scaling, _rotation,
 * _features_dc, _features_rest, scene/gaussian_model.py:53-69) and the activations of
 * gaussian_model.py:192-220 are fused into the kernels.  SH coefficient k of Gaussian i,
 * channel c is sh_dc[i*sh_dc_stride + c] for k = 0 and sh_rest[i*sh_rest_stride + 3*(k-1) + c]
 * otherwise.  For tangents (gslm_jvp) the same struct carries the tangent tensors; a NULL pointer
 * means a zero tangent. */
typedef struct gslm_gaussians {
  int64_t P;
  int32_t max_coeffs; /* K: coefficients stored per Gaussian (dc + rest) */
  int32_t raw;
  const float* means3D;       /* [P,3] */
  const float* opacities;     /* [P]   */
  const float* scales;        /* [P,3] or NULL when cov3D_precomp is given */
  const float* rotations;     /* [P,4] (w,x,y,z) */
  const float* cov3D_precomp; /* [P,6] or NULL */
  const float* sh_dc;         /* or NULL when colors_precomp is given */
  int64_t sh_dc_stride;
  const float* sh_rest;
  int64_t sh_rest_stride;
  const float* colors_precomp; /* [P,3] or NULL */
} gslm_gaussians;

/* Gradients / param-space vectors, one pointer per GaussianModelState group
 * (solver/gaussian_model_state.py:52-62).  NULL = not requested.  Strides as in gslm_gaussians. */
typedef struct gslm_grads {
  float* means2D;   /* [P,3] NDC-space screen gradient (means2D.grad, gaussian_model.py:561-563) */
  float* means3D;   /* [P,3] */
  float* opacities; /* [P]   */
  float* scales;    /* [P,3] */
  float* rotations; /* [P,4] */
  float* cov3D;     /* [P,6] (only when cov3D_precomp was the input) */
  float* sh_dc;
  int64_t sh_dc_stride;
  float* sh_rest;
  int64_t sh_rest_stride;
  float* colors;    /* [P,3] (only when colors_precomp was the input) */
  int32_t accumulate; /* 1: add into the outputs, 0: overwrite */
} gslm_grads;

/* ---- workspace sizing (two-call protocol: query, allocate with the caller's allocator, call) ---- */
size_t gslm_geom_bytes(int64_t P);
size_t gslm_image_bytes(int32_t H, int32_t W);
size_t gslm_binning_bytes(int64_t num_rendered, int32_t H, int32_t W);
size_t gslm_scratch_bytes(int64_t P, int64_t num_rendered); /* backward / jvp / matvec scratch */

/* ---- forward (rasterizer_impl forward: preprocess -> scan -> duplicateWithKeys -> sort -> ranges -> render) ---- */
/* Per-Gaussian preprocess, depth sort and tile-count scan.  Writes radii (int32 [P]) if non-NULL. */
int gslm_preprocess(const gslm_view* view, const gslm_gaussians* g, void* geom, size_t geom_bytes,
                    int32_t* out_radii, void* stream);
/* gslm_preprocess with a reusable depth order.  The depth order (the stable sort of every Gaussian in front of the
 * near plane by view-space depth, index order on ties; Gaussians culled later by their footprint emit no tile, so
 * the point list is the same whatever their place) depends on means3D and the view alone.
 *   order_mode 0: as gslm_preprocess;  1: also copy the order to depth_order[P];
 *   2: take the order from depth_order[P] -- written by a mode-1 call on the same view with the same means3D --
 *      instead of sorting (the LM line search renders each validation view at 7 step sizes with xyz frozen,
 *      train_jvp.py:221-227,262-279: the same point list, bitwise, without the four depth-sort passes). */
int gslm_preprocess_ordered(const gslm_view* view, const gslm_gaussians* g, void* geom, size_t geom_bytes,
                            int32_t* out_radii, uint32_t* depth_order, int32_t order_mode, void* stream);
/* The per-Gaussian stage of gslm_preprocess for nviews <= 8 views in one pass over the Gaussians (ABI 8): each view's
 * render records, depth keys, tile counts and rects into geoms[b] (each >= gslm_geom_bytes(P)), bitwise as
 * gslm_preprocess writes them, with no depth sort and no tile-count scan.  A Gaussian's 236 B of inputs (SH 3) are
 * read once for the views.  depth_pos (or NULL): per view the Gaussians' depth positions (gslm_depth_positions of the
 * view's depth order); then only the render records are written, each at its Gaussian's depth position, the rect
 * slot zero when culled -- the DEPTH SPACE the line search's union binning reads (below) -- and each geoms[b] needs
 * only gslm_depth_records_bytes(P) (64 B per Gaussian; ABI 9).  Every layout and SH degree (ABI 9: degree 0 too). */
size_t gslm_depth_records_bytes(int64_t P);
int gslm_preprocess_views(const gslm_view* views, int32_t nviews, const gslm_gaussians* g, void* const* geoms,
                          size_t geom_bytes, const uint32_t* const* depth_pos, void* stream);
/* depth_pos[depth_order[s]] = s for s < P (the inverse of a gslm_preprocess_ordered depth order). */
int gslm_depth_positions(const uint32_t* depth_order, int64_t P, uint32_t* depth_pos, void* stream);
/* Synchronous read of the number of (tile, Gaussian) pairs produced by gslm_preprocess. */
int gslm_num_rendered(const void* geom, int64_t P, int64_t* out_num_rendered, void* stream);
/* The same for n preprocessed geometries (geoms[k] over Ps[k] Gaussians) with ONE stream synchronisation:
 * a batch of views (the line search's validation renders, gslm.lm.LossEvaluator) preprocesses every view first,
 * then sizes every view's binning from one read-back instead of one round trip per view. */
int gslm_num_rendered_many(const void* const* geoms, const int64_t* Ps, int32_t n, int64_t* out_num_rendered,
                           void* stream);
/* Binning + tile sort + ranges + per-tile blend.  out_color [3,H,W], out_invdepth [1,H,W] (nullable). */
int gslm_rasterize(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes,
                   int64_t num_rendered, void* image, size_t image_bytes, float* out_color,
                   float* out_invdepth, void* stream);
/* The LM line search's validation loss of one view with no image written (gslm.lm.LossEvaluator; train_jvp.py:258,
 * 268,279 val_loss_func().loss_scalar with disable_ssim=True): gslm_rasterize's binning and blend, the blend's
 * epilogue computing r = m clamp(color, 0, 1) - gt per pixel and channel (gslm_lm_residual's arithmetic; gt [3,H,W],
 * alpha_mask [H,W] or NULL) and summing r^2 in double per tile, then *loss_dev = [*loss_dev if accumulate] +
 * 2 sum over tiles in tile order (deterministic).  No colour, inverse depth, final_T or n_contrib is written.
 * scratch >= gslm_loss_scratch_bytes(H, W). */
size_t gslm_loss_scratch_bytes(int32_t H, int32_t W);
int gslm_rasterize_loss(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes,
                        int64_t num_rendered, const float* gt, const float* alpha_mask, void* scratch,
                        size_t scratch_bytes, double* loss_dev, int32_t accumulate, void* stream);
/* Device-count forms (ABI 7): no host read-back of the pair count between gslm_preprocess and the binning.  The
 * binning workspace is used as a list of gslm_binning_capacity(binning_bytes, H, W) pairs; the count stays in the
 * geometry workspace and the kernels read it there.  n_out (device or host-pinned uint32, nullable) receives the count
 * in stream order: when it exceeds the capacity the pairs past it were dropped and the image / loss is invalid -- render
 * the view again with gslm_rasterize and a buffer of gslm_binning_bytes(count).  The binning written here serves this
 * render only (gslm_backward / gslm_jvp / gslm_matvec_* take the layout of the exact count: use gslm_rasterize for
 * those).  Same pairs, order, image and loss as gslm_rasterize / gslm_rasterize_loss whenever the count fits. */
int64_t gslm_binning_capacity(size_t binning_bytes, int32_t H, int32_t W);
int gslm_rasterize_dev(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes,
                       void* image, size_t image_bytes, float* out_color, float* out_invdepth, uint32_t* n_out,
                       void* stream);
int gslm_rasterize_loss_dev(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes,
                            const float* gt, const float* alpha_mask, void* scratch, size_t scratch_bytes,
                            double* loss_dev, int32_t accumulate, uint32_t* n_out, void* stream);
/* Stream-ordered 4-byte copy of gslm_preprocess' pair count to dst (device or host-pinned); no synchronisation. */
int gslm_num_rendered_copy(const void* geom, int64_t P, uint32_t* dst, void* stream);

/* ---- The line search's shared binning (ABI 8; ABI 9: the per-set workspaces' size set_bytes, each
 * >= gslm_depth_records_bytes(P), and n_sets for gslm_rasterize_loss_slot, checked against slot and against the set
 * count gslm_union_binning recorded in the binning workspace -- a slot past it renders a NaN loss instead of a
 * plausible background-only one) ----
 * train_jvp.py:262-277 renders every validation view at six points theta + alpha s (alpha = 2, 1, .., 1/16) of one step
 * s whose xyz group is masked (:221-227).  A view's Gaussians then keep their screen centre and depth order at every
 * point, and each point's exact point list is the subsequence of one list binned over the union of the points' rects:
 * the entries whose tile lies in that point's rect, in the same (tile, depth, index) order.  So a view is binned once
 * for the six points instead of once per point (gslm.lm.LossEvaluator.evaluate_points):
 *   1. each point's render records in depth space, in its own geometry workspace (geoms[a]: gslm_preprocess_views
 *      with the view's depth positions; the depth order from one gslm_preprocess_ordered, order_mode 1);
 *   2. gslm_union_geometry: the union of the n <= 8 points' rects per depth position into union_geom, the tile counts
 *      scanned -- gslm_num_rendered(union_geom) is the union list's length N;
 *   3. gslm_union_binning (workspace >= gslm_union_binning_bytes(N, H, W)): duplicate + tile sort + ranges of the union
 *      list, each entry carrying 4 bits per point through the sort (slot a: the point's quadrant mask of the entry --
 *      the bits its own binning would give it -- and 0 when its tile is outside the point's rect or the Gaussian is
 *      culled there);
 *   4. gslm_rasterize_loss_slot(geom = geoms[a], slot = a): gslm_rasterize_loss's blend + loss over the entries of
 *      slot a -- the same visits in the same order with the same records as the exact render: the same loss, bitwise.
 * The union list's values are depth positions (every pass reads the points' records coalesced in depth order). */
size_t gslm_union_binning_bytes(int64_t num_rendered, int32_t H, int32_t W);
int gslm_union_geometry(const gslm_view* view, int64_t P, const void* const* geoms, int32_t n, size_t set_bytes,
                        void* union_geom, size_t union_geom_bytes, void* stream);
int gslm_union_binning(const gslm_view* view, int64_t P, const void* union_geom, void* binning, size_t binning_bytes,
                       int64_t num_rendered, const void* const* geoms, int32_t n, size_t set_bytes, void* stream);
int gslm_rasterize_loss_slot(const gslm_view* view, int64_t P, const void* geom, size_t set_bytes, const void* binning,
                             size_t binning_bytes, int64_t num_rendered, int32_t slot, int32_t n_sets, const float* gt,
                             const float* alpha_mask, void* scratch, size_t scratch_bytes, double* loss_dev,
                             int32_t accumulate, void* stream);
/* Step 4 for n sets in one pass over the union list (the list walked once; set a + 1's records loaded while set a's
 * hits are visited): geoms[a] / loss_dev[a] are slot first_set + a's (ABI 9: a group of the binning's sets);
 * *loss_dev[a] = [*loss_dev[a] if accumulate] + that set's loss, bitwise gslm_rasterize_loss_slot(geoms[a],
 * first_set + a).  scratch >= gslm_loss_sets_scratch_bytes(n, H, W). */
size_t gslm_loss_sets_scratch_bytes(int32_t n, int32_t H, int32_t W);
int gslm_rasterize_loss_sets(const gslm_view* view, int64_t P, const void* const* geoms, int32_t n, int32_t first_set,
                             size_t set_bytes, const void* binning, size_t binning_bytes, int64_t num_rendered,
                             const float* gt, const float* alpha_mask, void* scratch, size_t scratch_bytes,
                             double* const* loss_dev, int32_t accumulate, void* stream);
/* The three loss blends under a trained per-camera exposure (still ABI 9, additive): the plain form's arguments,
 * checks, scratch sizes and per-tile sums, with the pixel's final colour R = C + T bg mapped through the camera's
 * exposure X before the clamp -- gslm_lm_residual_exposure's arithmetic in its order, so the per-pixel residuals are
 * that function's floats on gslm_rasterize's image:
 *   C'_j = ((R_0 X[j] + R_1 X[4 + j]) + R_2 X[8 + j]) + X[4 j + 3],   r_j = m clamp(C'_j, 0, 1) - gt_j.
 * exposure: 12 device floats (the model's [3, 4] row of the view's camera), read by the kernel in stream order -- no
 * host read; X = [I | 0] gives the plain form's loss bitwise.  gslm_rasterize_loss_sets_exposure takes a host array of
 * n device pointers, entry a belonging to slot first_set + a (each set its own X).  A NULL exposure, or a NULL entry
 * of the array, returns GSLM_ERR_INVALID before any launch.  The device-count form has no exposure variant. */
int gslm_rasterize_loss_exposure(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes,
                                 int64_t num_rendered, const float* gt, const float* alpha_mask, const float* exposure,
                                 void* scratch, size_t scratch_bytes, double* loss_dev, int32_t accumulate,
                                 void* stream);
int gslm_rasterize_loss_slot_exposure(const gslm_view* view, int64_t P, const void* geom, size_t set_bytes,
                                      const void* binning, size_t binning_bytes, int64_t num_rendered, int32_t slot,
                                      int32_t n_sets, const float* gt, const float* alpha_mask, const float* exposure,
                                      void* scratch, size_t scratch_bytes, double* loss_dev, int32_t accumulate,
                                      void* stream);
int gslm_rasterize_loss_sets_exposure(const gslm_view* view, int64_t P, const void* const* geoms, int32_t n,
                                      int32_t first_set, size_t set_bytes, const void* binning, size_t binning_bytes,
                                      int64_t num_rendered, const float* gt, const float* alpha_mask,
                                      const float* const* exposure, void* scratch, size_t scratch_bytes,
                                      double* const* loss_dev, int32_t accumulate, void* stream);
/* The three loss blends under a robust loss (still ABI 9, additive; rho and its arithmetic: at
 * gslm_lm_residual_robust below):
 * the plain form's arguments, checks, scratch sizes, visits and per-pixel residuals r, with the per-tile sum taking
 * rho(r^2) -- gslm_lm_residual_robust's double expression on the same float r and the same float test -- in place
 * of r^2.  `robust` is read on the host and passed by value; one block serves all sets of a call.  robust NULL or kind
 * GSLM_ROBUST_NONE launches the plain form's kernel (the same bits); an unknown kind, or a delta that is not finite
 * and > 0, returns GSLM_ERR_INVALID before any launch.  There is no device-count form and no exposure x robust form. */
enum { GSLM_ROBUST_NONE = 0, GSLM_ROBUST_HUBER = 1, GSLM_ROBUST_CAUCHY = 2 };
typedef struct {
  int32_t kind;  /* GSLM_ROBUST_* */
  float delta;   /* the scale: finite and > 0 (ignored with GSLM_ROBUST_NONE) */
} gslm_robust;
int gslm_rasterize_loss_robust(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes,
                               int64_t num_rendered, const float* gt, const float* alpha_mask,
                               const gslm_robust* robust, void* scratch, size_t scratch_bytes,
                               double* loss_dev, int32_t accumulate, void* stream);
int gslm_rasterize_loss_slot_robust(const gslm_view* view, int64_t P, const void* geom, size_t set_bytes,
                                    const void* binning, size_t binning_bytes, int64_t num_rendered, int32_t slot,
                                    int32_t n_sets, const float* gt, const float* alpha_mask,
                                    const gslm_robust* robust, void* scratch, size_t scratch_bytes,
                                    double* loss_dev, int32_t accumulate, void* stream);
int gslm_rasterize_loss_sets_robust(const gslm_view* view, int64_t P, const void* const* geoms, int32_t n,
                                    int32_t first_set, size_t set_bytes, const void* binning, size_t binning_bytes,
                                    int64_t num_rendered, const float* gt, const float* alpha_mask,
                                    const gslm_robust* robust, void* scratch, size_t scratch_bytes,
                                    double* const* loss_dev, int32_t accumulate, void* stream);
/* Convenience: gslm_preprocess + gslm_num_rendered + gslm_rasterize.  If binning_bytes is too
 * small returns GSLM_ERR_CAPACITY with *out_num_rendered set (geometry is valid: call
 * gslm_rasterize with a larger buffer). */
int gslm_forward(const gslm_view* view, const gslm_gaussians* g, void* geom, size_t geom_bytes,
                 void* binning, size_t binning_bytes, void* image, size_t image_bytes,
                 float* out_color, float* out_invdepth, int32_t* out_radii,
                 int64_t* out_num_rendered, void* stream);

/* ---- backward (VJP) of gslm_forward.  dL_dinvdepth may be NULL. ---- */
int gslm_backward(const gslm_view* view, const gslm_gaussians* g, const void* geom, const void* binning,
                  int64_t num_rendered, const void* image, const float* dL_dcolor,
                  const float* dL_dinvdepth, void* scratch, size_t scratch_bytes,
                  const gslm_grads* out, void* stream);

/* ---- forward-mode tangent (JVP) of gslm_forward; reuses the forward's sorted lists.
 * means2D_tangent [P,3] may be NULL. ---- */
int gslm_jvp(const gslm_view* view, const gslm_gaussians* g, const gslm_gaussians* tangent,
             const float* means2D_tangent, const void* geom, const void* binning, int64_t num_rendered,
             const void* image, void* scratch, size_t scratch_bytes, float* out_color_t,
             float* out_invdepth_t, void* stream);

/* ---- fused LM normal-equations product of one view:
 *   y += 2 * J^T ( w (.) (J v) )     (J: d clamp-free render / d raw params, g->raw must be 1)
 * w [3,H,W] is the per-pixel weight m^2 * 1[0 <= R <= 1] of the disable_ssim residual
 * (batch_training_loss.py:10-17; the factor 2 is the [r; r] aliasing).  This J has no exposure
 * column; GSLM_MV_EXPOSURE (below) is the product with the cameras' trained exposures.
 * mask_xyz = 1 freezes the xyz group (train_jvp.py:221-227): v.xyz is ignored, y.xyz untouched. ---- */
int gslm_matvec_view(const gslm_view* view, const gslm_gaussians* g, const gslm_grads* v,
                     const float* pixel_weight, int32_t mask_xyz, const void* geom, const void* binning,
                     int64_t num_rendered, const void* image, void* scratch, size_t scratch_bytes,
                     const gslm_grads* y, void* stream);

/* The three stages of gslm_matvec_view, separately launchable (profiling, overlap):
 * TANGENT: per-Gaussian tangent records from v; RENDER: fused JVP->VJP tile pass writing one row per
 * (tile, Gaussian); GATHER: per-Gaussian gather-sum + chain rule, y += ... */
#define GSLM_STAGE_TANGENT 1
#define GSLM_STAGE_RENDER 2
#define GSLM_STAGE_GATHER 4
#define GSLM_STAGE_ALL 7
#define GSLM_STAGE_OVERWRITE 8 /* GATHER writes y instead of accumulating into it */
#define GSLM_STAGE_SCREEN 16   /* view-sharded exchange: write this view's per-Gaussian screen-space sums to
                                  opts->screen_out (see gslm_gather_screen) instead of gathering into y */
/* opts->flags: GSLM_MV_TAIL_CLEAN -- the caller guarantees that the LM row map an earlier RENDER stage built
 * for this same geometry / binning is intact (no forward or drop-in backward, no other use of the scratch's map
 * or of the binning buffer since).  The row map gives gradient rows only to HEAD list entries (positions below
 * the largest n_contrib of their tile: every later entry's row would be zero), packed per Gaussian; it holds
 * each sorted entry's row slot (in the binning buffer's free sort ping-pong half) and the per-Gaussian row
 * offsets (in the scratch).  It depends on the geometry only, so an LM step's CG loop builds it once; without
 * the flag RENDER rebuilds it.
 * Building the row map WRITES the binning workspace (the `const void* binning` of the gslm_matvec_view* forms: their
 * RENDER stage without the flag, the fused product, the J^T b / pixel_seed pass and the exposure form alike;
 * gslm_backward and gslm_jvp build no row map and leave the binning as it is): besides the row slots it
 * clears, in the sorted list's words, the quadrant-mask bits of the (entry, quadrant) visits that no pixel blends
 * (inside the image, list position below the pixel's n_contrib, !(power > 0), alpha >= 1/255).  The tile passes skip
 * those visits and compute the same bits; refining a refined list changes nothing; the next forward rebuilds the
 * list.  The environment variable GSLM_LIVE_MASKS=0 leaves the binning's masks as they are (A/B runs).  The library
 * reads it at every row map and takes any other value as on; gslm.lm.live_masks() refuses values other than 0 and 1
 * for the Python host. */
#define GSLM_MV_TAIL_CLEAN 1
/* opts->flags: GSLM_MV_SH_REST_PROJECTED -- single-view Krylov space of the SH-rest group.  With one view,
 * Gaussian i's SH-rest columns of J are B_rest(dir_i) (x) d rgb, so J^T W J + D (D a scalar on the group)
 * maps span{B_rest(dir_i) (x) e_c} to itself and every CG iterate started from J^T b lies in it.  With this
 * flag the SH-rest group of v, y and xpby_s holds 3 floats per Gaussian (sh_rest_stride 3): the coordinates
 * along Bh = B_rest / |B_rest| (the same operator on the 3(M-1) -> 3 coordinates of that span; convert with
 * gslm_sh_rest_project).  Not for the SCREEN stage (multi-view). */
#define GSLM_MV_SH_REST_PROJECTED 2
/* The options of the product entry points: gslm_matvec_view_ex, gslm_matvec_view_active, gslm_gather_screen,
 * gslm_gather_views (_active) and gslm_tangent_views (_active).
 * Error contract, for all of them: every GSLM_ERR_INVALID or GSLM_ERR_CAPACITY return precedes the call's first
 * launch and leaves every caller buffer untouched -- y, v (the fused direction update's p) and x, jv_out, screen_out,
 * the dot and its scratch, the exposure rows, and the scratch workspace.  Only GSLM_ERR_HIP can follow a launch. */
typedef struct gslm_matvec_opts {
  int32_t stages;         /* GSLM_STAGE_* bits; 0 means GSLM_STAGE_ALL (accumulate) */
  int32_t flags;          /* GSLM_MV_* bits */
  const double* damp7;    /* host array (GaussianModelDampMatrix order: xyz, dc, rest, scaling, rotation,
                             opacity, exposure) or NULL; when set GATHER also adds D v (exposure untouched: the
                             tail is the caller's, or gslm_exposure_opts.damp's with GSLM_MV_EXPOSURE) */
  double* dot_vy;         /* device double or NULL: receives <v, y> over the gathered groups after GATHER */
  void* dot_scratch;      /* device scratch for dot_vy, >= gslm_dot_scratch_bytes(P) bytes */
  size_t dot_scratch_bytes;
  /* Fused CG direction update (the p = s + beta p of conjugate_gradient.py:121-123, deferred into the
   * next product): when xpby_s is set, before the TANGENT stage every group of v becomes
   * s + beta v, beta = *beta_num / *beta_den (device doubles), and so does the flat tail
   * xpby_tail_v[0..xpby_tail_n) (the exposure group) from xpby_tail_s.  v's groups must be
   * contiguous per Gaussian (sh_dc_stride 3, sh_rest_stride 3(M-1)) and writable.  Same arithmetic
   * as gslm_xpby_dev.  With mask_xyz the xyz group is not touched (zero in every LM iterate). */
  const gslm_grads* xpby_s;
  const double* beta_num;
  const double* beta_den;
  float* xpby_tail_v;
  const float* xpby_tail_s;
  int64_t xpby_tail_n;
  float* screen_out;      /* GSLM_STAGE_SCREEN output, P x 8 floats */
  /* J^T seed instead of J^T W J v: when set, RENDER runs only the back-to-front pass with dL/dcolor =
   * pixel_seed ([3,H,W], e.g. gslm_lm_residual's seed) into the LM rows, and GATHER sums them as usual
   * (v is then only read for D v / dot_vy).  Needs mask_xyz; excludes TANGENT, SCREEN and xpby.  This
   * is the J^T b of an LM step (train_jvp.py:243, solver_functions.py:101-132) on the fused path. */
  const float* pixel_seed;
  /* J v only: when set, RENDER runs the front-to-back tangent pass alone and writes the colour tangent
   * J v ([3,H,W], before the clamp / mask) to jv_out; no rows are written, so GATHER must not be in the
   * same call.  The SSIM residual's product uses it: J v -> gslm_ssim_normal -> pixel_seed. */
  float* jv_out;
  /* Deferred x update of the previous CG step (conjugate_gradient.py:95 x += alpha p), fused with xpby:
   * when alpha_num is set, every element of v (groups and tail) first adds (alpha_num / alpha_den) v into
   * x, where x lives xpby_x_offset bytes from v (x and v two flat vectors of the same layout).  Same
   * arithmetic as gslm_cg_update's x update, so the iterates are bitwise those of the undeferred loop. */
  const double* alpha_num;
  const double* alpha_den;
  int64_t xpby_x_offset;
  /* Gaussian-sharded exchange (gslm_tangent_views below): when set, RENDER reads this view's tangent render
   * records (gslm_tangent_views' output once exchanged: [>= P][8] floats with mask_xyz, [>= P][12] without)
   * instead of the TANGENT stage's (TANGENT must be off). */
  const float* trec_in;
  /* gslm_gather_screen only: Gaussians between consecutive views' blocks of screen (0 means P). */
  int64_t screen_stride;
  /* Device CG control block of gslm_cg_monitor, or NULL: when cg_ctl[0] != 0 (the solve's stopping tests have
   * fired) the TANGENT, RENDER and GATHER kernels of this call return without work (and without writing y,
   * the dot or the direction update), so a host can enqueue a whole CGLS schedule without reading the tests
   * back each iteration.  gslm_matvec_view_ex, gslm_tangent_views and gslm_gather_screen (the Gaussian-sharded
   * exchange's stages) all honour it. */
  const double* cg_ctl;
  /* gslm_tangent_views / gslm_gather_screen only (ABI 6): SH-rest coordinates of the Gaussian-sharded exchange.
   * When rest_basis is set, the SH-rest group of v, y (and of the fused direction update's s) holds 3 rest_views
   * floats per Gaussian -- the coordinates of the SH-rest vector in an orthonormal basis of span{B_rest(dir_b)}
   * over the job's rest_views views b -- and rest_basis is gslm_rest_basis' per-Gaussian factor R of those
   * views; view k of this call is column view_base + k of R.  See gslm_rest_basis. */
  const float* rest_basis;
  int32_t rest_views;
  int32_t view_base;
} gslm_matvec_opts;
int gslm_matvec_view_ex(const gslm_view* view, const gslm_gaussians* g, const gslm_grads* v,
                        const float* pixel_weight, int32_t mask_xyz, const void* geom, const void* binning,
                        int64_t num_rendered, const void* image, void* scratch, size_t scratch_bytes,
                        const gslm_grads* y, const gslm_matvec_opts* opts, void* stream);

/* SH-rest coordinates of GSLM_MV_SH_REST_PROJECTED for this view (gaussians: the raw leaves; means3D and
 * max_coeffs are used).  mode 0 (expand): out[i*out_stride + 3(k-1) + c] = Bh_k(dir_i) in[i*in_stride + c];
 * mode 1 (project): out[i*out_stride + c] = sum_k Bh_k(dir_i) in[i*in_stride + 3(k-1) + c]; Bh = B_rest/|B_rest|
 * over the view's active degree (inactive coefficients expand to 0). */
int gslm_sh_rest_project(const gslm_view* view, const gslm_gaussians* g, int32_t mode, const float* in,
                         int64_t in_stride, float* out, int64_t out_stride, void* stream);

/* ---- The single-view product on the Gaussians the view can move (additive entry points, still ABI 9: no
 * existing struct or signature changes) ----
 * A Gaussian that owns no head row in the LM row map (GSLM_MV_TAIL_CLEAN above) is visited by no wave of the
 * RENDER stage: its column of this view's J is exactly zero, so J^T W J + D acts on it as D alone, and a CG
 * solve from x0 = 0 whose right-hand side is zero there keeps s, p, q and x exactly zero on it.  The ACTIVE
 * Gaussians are the others; the per-Gaussian stages can run on vectors that hold the active Gaussians only.
 *
 * gslm_active_list: ids_dev[0 .. *count_dev) = the ascending ids i with at least one head row, from the row map a
 * RENDER stage built for this geometry and binning (valid exactly while GSLM_MV_TAIL_CLEAN may be passed; the
 * list depends on the geometry only), and rows_dev[0 .. *count_dev] = their row offsets: list entry j's head rows
 * are [rows_dev[j], rows_dev[j + 1]) (the Gaussians between two listed ones own none).  ids_dev holds P entries,
 * rows_dev P + 1; work is a device workspace of gslm_active_list_bytes(P) bytes.  Stream ordered, no
 * synchronisation: read *count_dev back after it. */
size_t gslm_active_list_bytes(int64_t P);
int gslm_active_list(const void* geom, int64_t P, int64_t num_rendered, const void* scratch, size_t scratch_bytes,
                     void* work, size_t work_bytes, int32_t* ids_dev, uint32_t* rows_dev, int64_t* count_dev,
                     void* stream);
/* gslm_matvec_view_ex on an active list (active_ids, active_rows: gslm_active_list's two outputs; mask_xyz only;
 * not the SCREEN stage, trec_in or rest_basis): every group of v, y and xpby_s (and x at xpby_x_offset) is
 * [n_active x width] -- row j belongs to Gaussian active_ids[j] -- while g, geom, binning and scratch stay the
 * scene's.  TANGENT and GATHER run one thread per list entry; RENDER
 * is the same launch.  Per-element arithmetic is that of gslm_matvec_view_ex: with v zero off the list, y here is
 * bitwise the rows active_ids of the full product's y (dot_vy sums the same products in another grouping).
 * dot_scratch >= gslm_dot_scratch_bytes(n_active).  Requires GSLM_MV_TAIL_CLEAN (the list comes from that map). */
int gslm_matvec_view_active(const gslm_view* view, const gslm_gaussians* g, const gslm_grads* v,
                            const float* pixel_weight, int32_t mask_xyz, const void* geom, const void* binning,
                            int64_t num_rendered, const void* image, void* scratch, size_t scratch_bytes,
                            const gslm_grads* y, const gslm_matvec_opts* opts, const int32_t* active_ids,
                            const uint32_t* active_rows, int64_t n_active, void* stream);
/* Flat param-space vectors between the P layout and the n_active layout: ngroups consecutive groups of
 * [rows x widths[k]] floats followed by a flat tail of tail_n floats (copied).  pack: dst row j of every group =
 * src row active_ids[j].  unpack: the reverse, every other row of dst written +0.0f.  ngroups <= 8. */
int gslm_active_pack(const float* src, float* dst, const int32_t* active_ids, int64_t n_active, int64_t P,
                     const int32_t* widths, int32_t ngroups, int64_t tail_n, void* stream);
int gslm_active_unpack(const float* src, float* dst, const int32_t* active_ids, int64_t n_active, int64_t P,
                       const int32_t* widths, int32_t ngroups, int64_t tail_n, void* stream);

/* ---- The lean single-view CG loop (additive entry points, still ABI 9) ----
 * The benchmark-mode solve on an active list with less work around the tile pass and bitwise the same iterates:
 *  - a dot's block partials are summed by the kernel that needs the scalar (the additions of gslm_dot_finalize in
 *    its order), so the loop launches no finalisation; one consumer also stores the sum to the scalar's slot;
 *  - the per-Gaussian kernels read the chains' parameters from a copy in list order (gslm_active_params);
 *  - one launch starts a solve (gslm_cg_start_active) and one ends it (gslm_cg_end_active). */
typedef struct gslm_cg_lean {
  const void* beta_partials; /* beta_num of the fused direction update (gslm_matvec_opts.xpby_s) as the beta_np
                                partials gslm_cg_update_lean left, or NULL: *beta_num is finished.  Not dot_scratch. */
  int32_t beta_np;
  int32_t dot_defer;         /* nonzero: GATHER leaves <v, y> as (n_active + 255) / 256 partials in
                                opts->dot_scratch and launches no finalisation (opts->dot_vy must be NULL) */
  double* beta_store;        /* or NULL: receives the sum of beta_partials */
  const void* params;        /* or NULL: gslm_active_params' block for active_ids */
} gslm_cg_lean;
/* gslm_matvec_view_active takes them as an extension of its options: with GSLM_MV_LEAN in opts->flags, opts points
 * to the base member of a gslm_matvec_opts_lean. */
#define GSLM_MV_LEAN 4
typedef struct gslm_matvec_opts_lean {
  gslm_matvec_opts base;
  gslm_cg_lean lean;
} gslm_matvec_opts_lean;
/* The parameters the LM chains load per Gaussian (xyz, raw scale, raw rotation, raw opacity, the clamp word of
 * geom) copied in list order into block (>= gslm_active_params_bytes(n_active)), and pos_dev [P]: pos[active_ids[j]]
 * = j, -1 for a Gaussian off the list.  The block is a snapshot: rebuild it when the list or a parameter changes. */
size_t gslm_active_params_bytes(int64_t n_active);
int gslm_active_params(const gslm_gaussians* g, const void* geom, int64_t P, const int32_t* active_ids,
                       int64_t n_active, void* block, size_t block_bytes, int32_t* pos_dev, void* stream);
/* Start of a solve on the list layout (groups as gslm_active_pack): s = p = the listed rows of the full-layout
 * g_full, q = x = 0 (the head [0, lo) zero in all four), and partials (1024 doubles) of <s, s> over [lo, n) whose
 * gslm_dot_finalize sum is bitwise gslm_dot's. */
int gslm_cg_start_active(const float* g_full, const int32_t* active_ids, int64_t n_active, int64_t P,
                         const int32_t* widths, int32_t ngroups, int64_t tail_n, int64_t lo, float* s, float* p,
                         float* q, float* x, void* partials, void* stream);
/* gslm_cg_update with x == NULL whose delta arrives as del_np partials (summed by every block, stored to del_dev
 * by one), and gamma as the finished *gam_dev or -- gam_partials non-NULL, after gslm_cg_start_active -- as gam_np
 * partials whose sum one block stores to *gam_dev; the partials of <s, s> stay in partials_out (1024 doubles, a
 * buffer of its own). */
int gslm_cg_update_lean(int64_t n, double* gam_dev, const void* gam_partials, int32_t gam_np,
                        const void* del_partials, int32_t del_np, double* del_dev, const float* p, const float* q,
                        float* s, void* partials_out, void* stream);
/* End of a solve: out_full (full layout) = the list-layout x [+ (num / den) p on [lo, n), num_dev non-NULL] at the
 * listed rows and the tail, +0.0f elsewhere -- gslm_axpy_dev then gslm_active_unpack in one pass over out_full;
 * pos_dev from gslm_active_params.  fin_partials (or NULL): fin_np partials whose sum is stored to *fin_dev. */
int gslm_cg_end_active(const float* x, const float* p, const double* num_dev, const double* den_dev, int64_t lo,
                       const int32_t* pos_dev, int64_t n_active, int64_t P, const int32_t* widths, int32_t ngroups,
                       int64_t tail_n, float* out_full, const void* fin_partials, int32_t fin_np, double* fin_dev,
                       void* stream);

/* ---- The single-view product under a trained per-camera exposure (additive entry points, still ABI 9; DESIGN.md
 * 4.5d; gslm.lm.LMProblem(train_exposure=True)) ----
 * render() maps the raw render R through the camera's 3x4 exposure X before the clamp
 * (gaussian_renderer/__init__.py:113-119): C_j = sum_i R_i X[i][j] + X[j][3].  With it the residual is
 * r_j = m clamp(C_j, 0, 1) - gt_j, and J gains the 12 columns dC/dX of every camera of the batch.  For a direction
 * (v, V), V the 3x4 exposure rows of v (row-major [i][k], as X):
 *   dC_j = sum_i (J v)_i X[i][j] + sum_i R_i V[i][j] + V[j][3],      u_j = 2 w_j dC_j,  w = m^2 1[0 <= C <= 1]
 *   Gaussian rows  y += J^T ub,  ub_i = sum_j X[i][j] u_j
 *   exposure rows  Y[i][j] += sum_pix R_i u_j  (j < 3),   Y[j][3] += sum_pix u_j.
 * GSLM_MV_EXPOSURE in opts->flags: opts points to the base member of a gslm_matvec_opts_exposure and the RENDER stage
 * runs this product: the tile pass forms dC, u and ub between its two halves and leaves u in u_image; a streaming
 * pass sums the 12 exposure rows (double block partials, one final pass in fixed order: deterministic) into
 *   y_rows[k] = [y_rows[k] unless overwrite] + damp v_rows[k] + sum_k.
 * pixel_weight is gslm_lm_residual_exposure's weight.  Accepted by gslm_matvec_view_ex and gslm_matvec_view_active
 * (the exposure rows are part of the flat tail, which gslm_active_pack copies).  dot_vy covers the Gaussian groups
 * only: the caller adds the tail's <V, Y>.  GSLM_ERR_INVALID (nothing launched): with pixel_seed, jv_out,
 * GSLM_STAGE_SCREEN, trec_in, rest_basis, GSLM_MV_LEAN or mask_xyz = 0, or a NULL member; GSLM_ERR_CAPACITY: scratch
 * below gslm_exposure_scratch_bytes.  With cg_ctl[0] != 0 neither y nor y_rows nor u_image is written. */
#define GSLM_MV_EXPOSURE 8
typedef struct gslm_exposure_opts {
  const float* exposure;  /* X: 12 device floats, the camera's row of GaussianModel._exposure */
  const float* v_rows;    /* V: 12 device floats, the camera's exposure rows of v (read after the TANGENT stage's
                             fused direction update, which covers the tail) */
  float* y_rows;          /* Y: 12 device floats, the camera's exposure rows of y */
  const float* color;     /* [3,H,W]: the forward's out_color (the raw render R) */
  float* u_image;         /* [3,H,W] scratch: receives u */
  void* scratch;          /* >= gslm_exposure_scratch_bytes(H, W) */
  size_t scratch_bytes;
  double damp;            /* y_rows += damp v_rows (pass it with one view per camera and product) */
  int32_t overwrite;      /* nonzero: y_rows is written, not accumulated into */
  int32_t _pad;
} gslm_exposure_opts;
typedef struct gslm_matvec_opts_exposure {
  gslm_matvec_opts base;
  gslm_exposure_opts exposure;
} gslm_matvec_opts_exposure;
size_t gslm_exposure_scratch_bytes(int32_t H, int32_t W);
/* gslm_lm_residual on the exposed colour C (above), exposure = X (12 device floats):
 *   residual = m clamp(C, 0, 1) - gt,   weight = m^2 1[0 <= C <= 1]                     (NULL: not written)
 *   seed_i   = sum_j X[i][j] sC_j,  sC_j = -2 m 1[0 <= C_j <= 1] residual_j              (NULL: not written)
 *              -- dL/dR of J^T b: feed it to pixel_seed as gslm_lm_residual's
 *   rhs_rows[4 i + j] += sum_pix R_i sC_j,  rhs_rows[4 j + 3] += sum_pix sC_j            (NULL: not computed)
 *              -- the exposure rows of J^T b, accumulated into 12 device floats (views sharing a camera add up)
 * and *loss_dev = [*loss_dev if accumulate] + 2 sum residual^2.  C, seed: products and sums left to right,
 * uncontracted; with X = [I | 0] residual, weight and seed are bitwise gslm_lm_residual's.  Deterministic (double
 * block partials, one final pass in fixed order).  scratch >= gslm_exposure_scratch_bytes(H, W). */
int gslm_lm_residual_exposure(int32_t H, int32_t W, const float* color, const float* gt, const float* alpha_mask,
                              const float* exposure, float* residual, float* weight, float* seed, float* rhs_rows,
                              void* scratch, size_t scratch_bytes, double* loss_dev, int32_t accumulate,
                              void* stream);

/* ---- view-sharded exchange (multi-GPU LM product), SURVEY 8(e) ----
 * Instead of all-reducing the param-space partial J^T W J v (F = 59 floats per Gaussian at SH 3),
 * every rank all-gathers per-view screen-space sums (8 floats per Gaussian per view) and applies the
 * per-view chains itself.  GSLM_STAGE_SCREEN of gslm_matvec_view_ex writes, for Gaussian i of the
 * view, screen[8 i .. 8 i + 7] = (dL/dconic a, b, c, dL/dopacity_eff, dL/dr, dL/dg, dL/db, flags),
 * flags = bit 31 visible | bits 0-2 SH clamp mask (as float bits); xyz must be masked.
 * gslm_gather_screen(views[0..nviews), screen[nviews][P][8]) then writes
 *   y = sum_b J_b^T screen_b [+ D v]   (views summed in index order: identical on every rank),
 * with opts->stages' OVERWRITE bit, damp7 and dot_vy as in gslm_matvec_view_ex.  nviews <= 16 per
 * call (accumulate further calls).  Replaces the reduction of solver_functions.py:110-121. */
int gslm_gather_screen(const gslm_view* views, int32_t nviews, const gslm_gaussians* g, const float* screen,
                       const gslm_grads* v, const gslm_grads* y, const gslm_matvec_opts* opts, void* stream);

/* ---- single-process multi-view product (additive entry point, still ABI 9; gslm.lm.BatchedLMProblem) ----
 * gslm_gather_screen with the views' row sums fused in: instead of one SCREEN stage per view into a [P][8] table,
 * gslm_gather_views reads every view's head rows where the last RENDER stage of that view left them (the fused
 * product, the pixel_seed pass or the trec_in form), addressed through that view's LM row map -- so ws[b] must be
 * the geometry and scratch of a view for which GSLM_MV_TAIL_CLEAN may be passed -- and writes
 *   y = [y +] [D v +] sum_b C_b^T (sum of the head rows of Gaussian i in view b)   (views summed in index order)
 * in one pass over the Gaussians: V row sums, V chains, one read and one write of y.  Without GSLM_MV_XYZ it is the
 * xyz-masked form: no view adds to y.xyz (with OVERWRITE it is written as the D v term alone, as gslm_gather_screen
 * does).  GSLM_MV_XYZ in opts->flags (this entry point only): the xyz rows are part of the product.  Every
 * ws[b].scratch must then hold 48-byte head rows, that is the rows an unmasked RENDER stage of that view (mask_xyz = 0,
 * with or without trec_in) wrote on its current row map -- the kernel cannot check this; the scratch holds
 * room for num_rendered 48-byte rows either way, so a mismatched call reads in bounds and computes nonsense.  The chain then
 * includes the means (with the SH colour's view-direction term, which reads the primal SH coefficients), y.xyz is
 * written like the other groups, the xyz groups of v and y must not be NULL, and <v, y> includes them.
 * GSLM_ERR_INVALID with GSLM_MV_XYZ on any other entry point (gslm_matvec_view_ex / gslm_matvec_view_active have their
 * mask_xyz argument; gslm_gather_screen, gslm_gather_views_active and gslm_tangent_views[_active] have no such form),
 * or together with GSLM_MV_DAMP_VEC, GSLM_MV_DEPTH or GSLM_MV_EXPOSURE.  opts as gslm_gather_screen: the OVERWRITE bit of stages,
 * damp7, dot_vy / dot_scratch, cg_ctl (a stopped solve leaves y and *dot_vy as they are) and rest_basis / rest_views / view_base (y's SH-rest group then holds the
 * gslm_rest_basis coordinates).  A view with num_rendered == 0 contributes nothing and its workspaces are not
 * read (no row map exists for it).  nviews 1..16 per call (accumulate further calls).  GSLM_ERR_INVALID: NULL
 * arguments, nviews outside 1..16, non-raw Gaussians, group strides that do not match the layout, rest_basis with
 * rest_views outside 1..GSLM_MAX_REST_VIEWS; GSLM_ERR_CAPACITY: a scratch below gslm_scratch_bytes(P,
 * num_rendered) or a dot scratch below gslm_dot_scratch_bytes(P).  Nothing is launched on an error. */
typedef struct gslm_view_ws {
  const void* geom;        /* the view's geometry workspace */
  const void* scratch;     /* the view's matvec scratch: its LM row map and head rows */
  size_t scratch_bytes;
  int64_t num_rendered;
} gslm_view_ws;
#define GSLM_MV_XYZ (1 << 6) /* 64: the next bit after GSLM_MV_DEPTH */
int gslm_gather_views(const gslm_view* views, const gslm_view_ws* ws, int32_t nviews, const gslm_gaussians* g,
                      const gslm_grads* v, const gslm_grads* y, const gslm_matvec_opts* opts, void* stream);

/* ---- Gaussian-sharded exchange (multi-GPU LM product; gslm.parallel.GaussianShardedOperator, exchange
 * "gaussian", the default of gslm.parallel.ShardedLMProblem when every rank renders the same number of views) ----
 * Rank r owns Gaussians [r S, (r + 1) S) of every CG vector and the vector algebra on them.  Per product:
 *   gslm_tangent_views   this shard's tangent render records for EVERY view b (chain_jvp, the TANGENT stage
 *                        of gslm_matvec_view_ex for a Gaussian range) -> all-to-all -> each rank holds its
 *                        own view's [P][8] table (mask_xyz; [P][12] without) for opts->trec_in;
 *   RENDER | SCREEN      with opts->trec_in -> [P][8] screen sums -> all-to-all -> each rank holds
 *                        screen[b][S][8] of its shard for every view;
 *   gslm_gather_screen   over the shard (g = the shard's slice of the leaves, opts->screen_stride = S).
 * A rank receives (32 + 32) (n - 1) / n bytes per Gaussian per view it renders instead of the screen
 * all-gather's 32 (n - 1), and runs 1/n of the chains and vector algebra.
 * gslm_view_flags: out[i] = 0 if Gaussian i touches no tile of the preprocessed view, else
 * 0x80000000 | its 3 SH-clamp bits (the flags word of the SCREEN rows); exchanged once per geometry. */
int gslm_view_flags(const void* geom, int64_t P, uint32_t* out, void* stream);
/* trec_out[(b trec_stride + i) * R ..] = tangent render record of shard Gaussian i in view b where
 * vflags[b flags_stride + i] is visible (other records untouched), R = 8 floats with mask_xyz (the LM rows:
 * [da db dc dop | dr dg db 0], the conic / opacity / colour tangents) or 12 without
 * ([dx dy da db | dc dop dr dg | db dinv 0 0]), b < nviews (<= 16).  g / v: the shard's
 * leaves and direction (P = shard size, SH-rest stride 3(M-1)); opts (or NULL): only the fused direction
 * update (xpby_s, beta_*, alpha_*, xpby_x_offset, xpby_tail_*) of gslm_matvec_view_ex, applied once before
 * the views' tangents.  The flat tail (xpby_tail_*) is updated once per call, so it must be this rank's
 * private copy and be passed to one call per product (several calls of one product: only the first gets
 * opts); an empty shard (P = 0) with a tail still applies the tail's update.
 * The trec_in table a RENDER stage reads must hold the records of every Gaussian the vflags of that same
 * geometry (gslm_view_flags of this view's current preprocess) mark visible: the kernel cannot check it. */
int gslm_tangent_views(const gslm_view* views, int32_t nviews, const gslm_gaussians* g, const gslm_grads* v,
                       int32_t mask_xyz, const uint32_t* vflags, int64_t flags_stride, float* trec_out,
                       int64_t trec_stride, const gslm_matvec_opts* opts, void* stream);

/* ---- The multi-view product on the Gaussians the batch can move (additive entry points, still ABI 9: no existing
 * struct or signature changes; gslm.lm.BatchedLMProblem(union_active=True)) ----
 * The argument of gslm_active_list holds for the union U of the views' lists: off U every view's column of J is
 * exactly zero, so sum_b J_b^T W_b J_b + D acts there as D alone, J^T b is zero there, and a CG solve from x0 = 0
 * keeps s, p, q and x exactly zero off U.  The SH-rest coordinates of gslm_rest_basis are per Gaussian, so the
 * restriction composes with them unchanged.  The two per-Gaussian passes then run on vectors that hold U only.
 *
 * gslm_active_union replaces nviews calls of gslm_active_list and the union of their outputs.  ws[b] as for
 * gslm_gather_views: the geometry and scratch of a view for which GSLM_MV_TAIL_CLEAN may be passed; nviews >= 1
 * (the list is over the whole batch, not per 16 views).  Outputs, all device memory:
 *   ids_dev [P]             ids_dev[0 .. *count_dev) = the ascending ids that own a head row in at least one view
 *                           with num_rendered > 0;
 *   hrow_dev [nviews][P+1]  hrow[b (P+1) + j] = view b's first head row of list entry j, hrow[b (P+1) + *count_dev]
 *                           = view b's number of head rows: entry j's head rows in view b are [hrow[b][j],
 *                           hrow[b][j+1]), an empty range when view b does not move it (the Gaussians between two
 *                           listed ones own no row in any view);
 *   aflags_dev [nviews][P]  aflags[b P + j] = gslm_view_flags' word of Gaussian ids[j] in view b;
 *   count_dev               the list's length, to be read back after the call (stream ordered, no synchronisation).
 * A view with num_rendered == 0 gets zeros in hrow and aflags and its workspaces are not read.  work is a device
 * workspace of gslm_active_union_bytes(P) bytes.  GSLM_ERR_INVALID: NULL arguments, nviews < 1, P out of range, a
 * negative num_rendered or a NULL workspace of a view that rendered; GSLM_ERR_CAPACITY: a scratch below
 * gslm_scratch_bytes(P, num_rendered) or a work area below gslm_active_union_bytes(P).  Nothing is launched on an
 * error. */
size_t gslm_active_union_bytes(int64_t P);
int gslm_active_union(const gslm_view_ws* ws, int32_t nviews, int64_t P, void* work, size_t work_bytes,
                      int32_t* ids_dev, uint32_t* hrow_dev, uint32_t* aflags_dev, int64_t* count_dev, void* stream);
/* gslm_tangent_views on the union list (mask_xyz only): every group of v and of the fused direction update
 * (xpby_s, x at xpby_x_offset) is [n_active x width] -- row j belongs to Gaussian active_ids[j] -- while g stays the
 * scene's.  aflags: rows b of gslm_active_union's aflags for the nviews views of this call (flags_stride >=
 * n_active; P as gslm_active_union wrote them).  The record of list entry j in view b goes to row active_ids[j] of
 * view b's table (trec_stride >= P), so the RENDER stages that read it (opts->trec_in) are unchanged; the records of
 * Gaussians off the list are not written and never read (the tile pass reads a record only below a quadrant's
 * bound, which is the head rule).  opts->rest_basis stays the scene's [P] factors, read by id.  Per-Gaussian
 * arithmetic is gslm_tangent_views'.  GSLM_ERR_INVALID: as gslm_tangent_views, and mask_xyz == 0, n_active outside
 * 0..P, a NULL list with n_active > 0, flags_stride < n_active.  Nothing is launched on an error. */
int gslm_tangent_views_active(const gslm_view* views, int32_t nviews, const gslm_gaussians* g, const gslm_grads* v,
                              int32_t mask_xyz, const int32_t* active_ids, int64_t n_active, const uint32_t* aflags,
                              int64_t flags_stride, float* trec_out, int64_t trec_stride,
                              const gslm_matvec_opts* opts, void* stream);
/* gslm_gather_views on the union list: every group of v and y is [n_active x width]; hrow / aflags: rows b of
 * gslm_active_union's outputs for the nviews views of this call (hrow_stride >= n_active + 1, flags_stride >=
 * n_active).  The row ranges come from hrow, visibility and the SH clamp bits from aflags; the views' tiles, goff,
 * hscan and clamp words are not read.  Per-element arithmetic, the order of each Gaussian's row sum and the order
 * of the views are gslm_gather_views': with v zero off the list, y here is bitwise the rows active_ids of the full
 * product's y; dot_vy sums the same products as (n_active + 255) / 256 partials (dot_scratch >=
 * gslm_dot_scratch_bytes(n_active)).  opts as gslm_gather_views.  A view with num_rendered == 0 contributes
 * nothing and its workspaces are not read.  GSLM_ERR_INVALID / GSLM_ERR_CAPACITY: as gslm_gather_views, and
 * GSLM_ERR_INVALID for n_active outside 0..P, a NULL list, or a stride that does not hold it.  Nothing is launched
 * on an error. */
int gslm_gather_views_active(const gslm_view* views, const gslm_view_ws* ws, int32_t nviews, const gslm_gaussians* g,
                             const gslm_grads* v, const gslm_grads* y, const int32_t* active_ids, int64_t n_active,
                             const uint32_t* hrow, int64_t hrow_stride, const uint32_t* aflags, int64_t flags_stride,
                             const gslm_matvec_opts* opts, void* stream);

/* ---- SH-rest coordinates of the Gaussian-sharded exchange (ABI 6) ----
 * The SH-rest column of J for view b is B_rest(dir_b) (x) (d rgb), B_rest the view's SH basis over
 * coefficients 1..nc-1.  So with V views every CGLS iterate started from J^T b keeps each Gaussian's SH-rest
 * group in span{B_rest(dir_b) : b < V} (x) R^3, which (J^T J + D) maps into itself (D is a scalar on the group):
 * 3 V coordinates per Gaussian in an orthonormal basis Q of that span replace 3(M-1) floats (V = 1 is
 * GSLM_MV_SH_REST_PROJECTED).  With B = Q R (Gram-Schmidt in view order; R upper triangular, the Cholesky
 * factor of the Gram matrix B^T B, computed in double), view b's colour tangent is sum_{j<=b} R[j][b] c_j and
 * its gradient adds R[j][b] dL/drgb_b to coordinate j: the per-Gaussian kernels need R only.  A view whose
 * direction adds less than 1e-6 of its norm to the span of the earlier ones (R[b][b]^2 <= 1e-12 G[b][b]) gets
 * row b of R zeroed: its coordinate stays 0.
 *   gslm_rest_basis   R_out[i * V(V+1)/2 + b(b+1)/2 + j] = R[j][b] (j <= b), float, for the V = nviews views
 *                     (1..GSLM_MAX_REST_VIEWS) and the Gaussians of g (means3D and max_coeffs used; the SH
 *                     degree of views[0]).
 *   gslm_rest_coords  mode 0 (expand): out[i*out_stride + 3(k-1) + c] = (Q c_i)[k][c] (0 for k >= nc);
 *                     mode 1 (project): out[i*out_stride + 3j + c] = (Q^T t_i)[j][c], t_i = in[i*in_stride ..]
 *                     in the [M-1][3] layout (the orthogonal projection onto the span). */
#define GSLM_MAX_REST_VIEWS 8
int gslm_rest_basis(const gslm_view* views, int32_t nviews, const gslm_gaussians* g, float* R_out, void* stream);
int gslm_rest_coords(const gslm_view* views, int32_t nviews, const gslm_gaussians* g, const float* R, int32_t mode,
                     const float* in, int64_t in_stride, float* out, int64_t out_stride, void* stream);

/* ---- device-resident CG vector algebra on flat fp32 vectors (param-space, n floats) ----
 * damp_groups: per-element damping is d[group(i)] with group boundaries bounds[0..ngroups]. */
size_t gslm_dot_scratch_bytes(int64_t n);
/* out (double, device) = sum_i a_i b_i d_i  (d = NULL means 1).  Deterministic. */
int gslm_dot(const float* a, const float* b, const int64_t* group_bounds, const double* group_damp,
             int32_t ngroups, int64_t n, void* scratch, double* out_dev, void* stream);
/* y = alpha * x + y, alpha read from device memory as num/den (den==NULL -> 1), times sign. */
int gslm_axpy_dev(int64_t n, const double* num_dev, const double* den_dev, float sign, const float* x,
                  float* y, void* stream);
/* p = s + beta p, beta = num/den from device memory */
int gslm_xpby_dev(int64_t n, const float* s, const double* num_dev, const double* den_dev, float* p,
                  void* stream);
/* One CG step, a = gam / del read from device memory:  x += a p;  s -= a q;
 * *gam_new_dev = <s, s> (scratch >= gslm_dot_scratch_bytes(n)).  Vectors 16-byte aligned.
 * x == NULL: only s -= a q and <s, s> (the x update deferred into the next product's xpby, see
 * gslm_matvec_opts.alpha_num; p is then not read). */
int gslm_cg_update(int64_t n, const double* gam_dev, const double* del_dev, const float* p, const float* q,
                   float* x, float* s, void* scratch, double* gam_new_dev, void* stream);
/* gslm_cg_update plus the residual monitor of conjugate_gradient.py:103-104 in the same pass:
 * *xg_dev = <x_new, g>, *xs_dev = <x_new, s_new> (g = J^T b).  scratch >= 3 * 1024 doubles.
 * cg_ctl (or NULL): gslm_cg_monitor's control block; with cg_ctl[0] != 0, *del_dev < 1e-20 (the early
 * termination of conjugate_gradient.py:88-91) or a non-finite *del_dev, x and s are left untouched. */
int gslm_cg_update_monitor(int64_t n, const double* gam_dev, const double* del_dev, const float* p, const float* q,
                           float* x, float* s, const float* g, void* scratch, size_t scratch_bytes,
                           double* gam_new_dev, double* xg_dev, double* xs_dev, const double* cg_ctl, void* stream);
/* The stopping tests of cgls_damped (conjugate_gradient.py:88-117) on the device, one launch per inner iteration
 * after gslm_cg_update_monitor (and after any cross-rank sums of its scalars).  cg_ctl = doubles
 * [stop, iters, last_res, n_hist, history[max_hist]], initialised by the caller to [0, 0, +inf, 0, ...]:
 *   *del < 1e-20 -> stop = 1;  res = (*b2 - *xg) - *xs is appended to history;  res > last_res -> stop = 2;
 *   *gam_new < max(tol sqrt(*gam), atol) -> stop = 3;  otherwise iters += 1.
 * Any of *gam, *gam_new, *del, *xg, *xs not finite -> stop = 4 (GSLM_CG_STOP_NONFINITE; the reference's NaN
 * asserts, solver/solver_functions.py:125-130) -- the caller must not use the iterate.  *gam and *del are checked
 * before everything else; *gam_new, *xg, *xs after the *del < 1e-20 test (gslm_cg_update_monitor leaves them
 * undefined on such a delta).
 * Once stop != 0 every later gslm_cg_monitor / gslm_cg_update_monitor / product with opts->cg_ctl is a no-op. */
#define GSLM_CG_STOP_NONFINITE 4
int gslm_cg_monitor(const double* gam_dev, const double* gam_new_dev, const double* del_dev, const double* xg_dev,
                    const double* xs_dev, const double* b2_dev, double tol, double atol, double* cg_ctl,
                    int32_t max_hist, void* stream);
/* *out_dev = sum of np per-block partials (second pass of the fused dots) */
int gslm_dot_finalize(const void* partials, int32_t np, double* out_dev, void* stream);
/* y += d[group] * x (the damping term D x) */
int gslm_damp_add(int64_t n, const float* x, const int64_t* group_bounds, const double* group_damp,
                  int32_t ngroups, float* y, void* stream);

/* ---- Marquardt-scaled damping D = lambda diag(J^T W J) (additive entry points, still ABI 9) ----
 * gslm_marquardt_scale: d[i] = (float)lambda[group(i)] * max(diag[i], floor) on a flat vector of n floats -- the
 * damping vector of a diagonal (gslm_lm_diag_view without damp7).  Groups as gslm_dot / gslm_damp_add: bounds[0 ..
 * ngroups], ngroups <= 8, host arrays (an element outside every group gets 0; ngroups = 0: lambda = 1); groups of
 * zero width and n = 0 are legal.  The max is the select diag < floor ? floor : diag, so a NaN diagonal gives a NaN
 * d (which the solve's non-finite checks then meet).  d may be diag.  GSLM_ERR_INVALID, nothing launched: n < 0,
 * a floor that is negative, NaN or beyond float, more than 8 groups, a NULL group array with ngroups > 0, or a NULL
 * vector with n > 0. */
int gslm_marquardt_scale(int64_t n, const float* diag, const int64_t* group_bounds, const double* group_lambda,
                         int32_t ngroups, double floor, float* d, void* stream);
/* GSLM_MV_DAMP_VEC in opts->flags: opts points to the base member of a gslm_matvec_opts_damp, and GATHER forms
 *   y = [y_old +] J^T(...) + d (.) v
 * with d read per element from damp_vec: a flat param-space vector with the groups and strides of v and y (the
 * projected SH-rest group included; on an active list, the listed rows).  Per element the arithmetic is damp7's --
 * val + d v, a multiply and an add -- so a d that is constant per group gives damp7's y and dot_vy bitwise; dot_vy
 * includes the term.  The xyz group (mask_xyz) is written d (.) v, as damp7's.  Accepted by gslm_matvec_view_ex and
 * gslm_matvec_view_active; gslm_gather_views, gslm_gather_views_active and gslm_gather_screen refuse the flag.
 * GSLM_ERR_INVALID before anything is launched (outputs untouched): with a non-NULL damp7; a NULL damp_vec or a
 * NULL group of it (sh_rest excepted when max_coeffs = 1) or SH strides other than y's; pixel_seed, jv_out,
 * GSLM_STAGE_SCREEN, trec_in or rest_basis; GSLM_MV_LEAN or GSLM_MV_EXPOSURE; mask_xyz = 0. */
#define GSLM_MV_DAMP_VEC 16
typedef struct gslm_matvec_opts_damp {
  gslm_matvec_opts base;
  const gslm_grads* damp_vec;
} gslm_matvec_opts_damp;

/* ---- diag(J^T W J + D) and Jacobi-preconditioned CG (additive entry points, still ABI 9) ----
 * gslm_lm_diag_view: the diagonal of the matrix gslm_matvec_view_ex applies for one view with mask_xyz (the
 * reference's matvec / matvec_T pair, solver/solver_functions.py:83-132, on the [r; r] residual):
 *   diag = 2 J^T diag(pixel_weight) J [+ D],
 * written into the groups of `diag` (a flat param-space vector as gslm_matvec_view_ex's y: sh_dc_stride 3,
 * sh_rest_stride 3(M-1), or 3 with GSLM_DIAG_SH_REST_PROJECTED -- coordinate c of the projected group gets
 * |B_rest|^2 S_col[c]; a NULL group is not written).  The derivative of alpha is the product's own (d alpha / d o = G,
 * d alpha / d power = o G, the 0.99 clamp ignored), so this is the diagonal of that operator exactly.  With the view
 * direction frozen no parameter moves both the colour and the conic / opacity: a tile pass sums twelve values per
 * head entry of the LM row map (9 geometry monomials, 3 colour sums; 48 bytes, the scratch's gradient rows hold
 * them) and a per-Gaussian pass applies the chains.  The xyz group gets D alone, and so does a Gaussian without a
 * head row.  damp7 (host, GaussianModelDampMatrix order) or NULL: D is added per group (pass it for one view of a
 * sum over views).  flags: GSLM_DIAG_TAIL_CLEAN -- the LM row map of this geometry is current (as GSLM_MV_TAIL_CLEAN;
 * without it the call builds the map, after which the flag may be passed to the products too);
 * GSLM_DIAG_ACCUMULATE -- add into diag instead of overwriting it.  The scratch's gradient rows are overwritten
 * (every product rewrites its own).  No float atomics: bitwise reproducible.
 * GSLM_ERR_INVALID, before anything is launched, for mask_xyz = 0, a NULL pixel_weight or diag, unknown flags,
 * non-raw gaussians or a destination with other strides; GSLM_ERR_CAPACITY for a scratch below
 * gslm_scratch_bytes(P, num_rendered) (which covers 48 bytes per head row).  On an error the outputs are untouched. */
#define GSLM_DIAG_TAIL_CLEAN 1
#define GSLM_DIAG_ACCUMULATE 2
#define GSLM_DIAG_SH_REST_PROJECTED 4
int gslm_lm_diag_view(const gslm_view* view, const gslm_gaussians* g, const float* pixel_weight, int32_t mask_xyz,
                      const void* geom, const void* binning, int64_t num_rendered, const void* image, void* scratch,
                      size_t scratch_bytes, const gslm_grads* diag, const double* damp7, int32_t flags,
                      void* stream);
/* One preconditioned CG step, a = gam / del read from device memory:  x += a p (x == NULL: skipped, p not read);
 * s -= a q;  z = s (.) minv;  *gam_new_dev = <s, z> (scratch >= gslm_dot_scratch_bytes(n)).  Vectors 16-byte
 * aligned.  gslm_cg_update's element order and double partial sums: with minv = 1 the results are bitwise its own.
 * The direction update p = z + beta p is gslm_xpby_dev. */
int gslm_pcg_update(int64_t n, const double* gam_dev, const double* del_dev, const float* p, const float* q,
                    float* x, float* s, const float* minv, float* z, void* scratch, double* gam_new_dev,
                    void* stream);
/* minv[j] = 1 / m[j], or 0 where m[j] <= 0 (or NaN): the Jacobi preconditioner of a diagonal m. */
int gslm_precond_invert(int64_t n, const float* m, float* minv, void* stream);

/* ---- RCCL collectives over xGMI, communicator handle passed in (SURVEY 8(b) "gslm_allreduce*", 8(e)) ----
 * The reference has no multi-GPU code (its LinearSolverFunctions renders a view batch serially on one GPU,
 * solver/solver_functions.py:88-93,110-121); these replace the all-reduce of J^T r / J^T J v and of the CG scalars
 * that SURVEY 8(e) adds, and carry the Gaussian-sharded exchange's all-to-alls, for a host that does not go through
 * torch.distributed (gslm.parallel uses them with GSLM_COMM=native; its default is torch.distributed's "nccl"
 * backend, the same RCCL).  One rank calls gslm_comm_unique_id and the host broadcasts the gslm_comm_id_bytes()
 * bytes; every rank then calls gslm_comm_init with its HIP device current (blocks until all ranks joined).  The
 * collectives are enqueued on `stream` (RCCL stream semantics: ordered after the kernels enqueued on it before, and
 * before those after) and never synchronise the host.  librccl is loaded on the first call (GSLM_ERR_HIP if absent). */
int32_t gslm_comm_id_bytes(void);
int gslm_comm_unique_id(void* id_out);
int gslm_comm_init(const void* id, int32_t nranks, int32_t rank, void** comm_out);
int gslm_comm_destroy(void* comm);
/* in-place sums over the ranks: param-space partial products (f32), CG scalars / losses (f64) */
int gslm_allreduce_sum_f32(void* comm, float* buf, int64_t n, void* stream);
int gslm_allreduce_sum_f64(void* comm, double* buf, int64_t n, void* stream);
/* recv[r * bytes_per_rank ...] = rank r's send[rank * bytes_per_rank ...] (the Gaussian-sharded exchange's records
 * and screen sums, gslm_tangent_views / GSLM_STAGE_SCREEN) */
int gslm_alltoall(void* comm, const void* send, void* recv, int64_t bytes_per_rank, void* stream);
/* recv[r * bytes_per_rank ...] = rank r's send[0 .. bytes_per_rank) (the screen exchange's per-view sums,
 * gslm_gather_screen) */
int gslm_allgather(void* comm, const void* send, void* recv, int64_t bytes_per_rank, void* stream);

/* ---- LM residual epilogue of one view (replaces the render clamp
 * gaussian_renderer/batch_render.py:118 + compute_batch_loss_block, solver/batch_training_loss.py:10-17,
 * 56-67, disable_ssim=True, and loss_scalar, solver/loss_image_state.py:16-19) ----
 * color / gt / residual / weight / seed are [3,H,W]; alpha_mask [H,W] or NULL (= 1).  Writes
 *   residual = m clamp(color, 0, 1) - gt          (NULL: not written)
 *   weight   = m^2 1[0 <= color <= 1]             (the per-pixel weight of gslm_matvec_view_ex; NULL: not
 *                                                  written -- with residual and seed NULL too, the loss alone:
 *                                                  the line search's validation loss)
 *   seed     = -2 m 1[0 <= color <= 1] residual   (NULL: not written; gslm_backward's dL/dcolor for J^T b)
 * and *loss_dev (device double) = [*loss_dev if accumulate] + 2 sum residual^2 ([r; r] aliasing).
 * Deterministic (fixed two-pass reduction); scratch >= gslm_residual_scratch_bytes(H, W). */
size_t gslm_residual_scratch_bytes(int32_t H, int32_t W);
int gslm_lm_residual(int32_t H, int32_t W, const float* color, const float* gt, const float* alpha_mask,
                     float* residual, float* weight, float* seed, void* scratch, size_t scratch_bytes,
                     double* loss_dev, int32_t accumulate, void* stream);

/* ---- Robust losses of the LM step (still ABI 9, additive): iteratively reweighted least squares in the first-order
 * Triggs form.  The loss is 2 sum rho(r^2) over the residual elements r of gslm_lm_residual, and with
 * rho' = rho'(r^2) taken at the linearisation point the weight and the seed are gslm_lm_residual's times rho' -- so
 * J^T b is exactly -1/2 grad loss and every product downstream is 2 J^T (W rho') J + D without knowing about it.
 *   HUBER   rho(s) = s                          rho' = 1                 where |r| <= delta
 *                    2 delta |r| - delta^2            delta / |r|        elsewhere
 *   CAUCHY  rho(s) = delta^2 log1p(s / delta^2) rho' = 1 / (1 + t t),    t = r / delta
 * Arithmetic: one float test per element, fabsf(r) <= delta, serves rho and rho'; rho' in float with correctly rounded
 * divisions and uncontracted products; rho in double from (double)r and (double)delta.  A NaN r gives a NaN weight,
 * seed and loss.  gslm_robust {kind, delta}: declared with the loss blends above. */
/* gslm_lm_residual under a robust loss: the same arguments, optional outputs, scratch size and two-pass double
 * reduction, with
 *   residual = r                                        (unscaled: the residual the caller inspects)
 *   weight   = ((m m) 1[0 <= color <= 1]) rho'
 *   seed     = (((-2 m) 1[0 <= color <= 1]) r) rho'
 *   *loss_dev = [*loss_dev if accumulate] + 2 sum rho.
 * robust NULL or kind GSLM_ROBUST_NONE is gslm_lm_residual itself (the same kernel: the same bits).  An unknown kind,
 * or a delta that is not finite and > 0, returns GSLM_ERR_INVALID before any launch, the outputs untouched. */
int gslm_lm_residual_robust(int32_t H, int32_t W, const float* color, const float* gt, const float* alpha_mask,
                            const gslm_robust* robust, float* residual, float* weight, float* seed, void* scratch,
                            size_t scratch_bytes, double* loss_dev, int32_t accumulate, void* stream);

/* ---- The inverse-depth residual of the LM step (still ABI 9, additive) ----
 * The reference's solver state reserves a third residual block, Ll1depth_per_pixel (solver/loss_image_state.py), for
 * the cameras' invdepthmap / depth_mask; here it is a least-squares block that enters the loss once:
 *   loss = 2 sum ||m clamp01(R) - gt||^2 + lambda_d sum (m_d (D - Dgt))^2,
 *   A v  = sum_b (2 J_c^T W_c J_c + J_D^T W_d J_D) v + D v,   W_d = lambda_d m_d^2,
 *   J^T b = (the colour part) - sum_b J_D^T (lambda_d m_d^2 (D - Dgt)),
 * D the rendered inverse depth (gslm_rasterize's out_invdepth: no background term, no clamp).  On the LM rows
 * (xyz frozen) a Gaussian's 1/z is a constant, so J_D has columns through alpha only -- scaling, rotation, opacity --
 * and the LM row format, the row map, the active list and the SH-rest projection are unchanged.
 *
 * gslm_lm_residual_depth: the block's epilogue for one view.  invdepth / invdepth_gt / residual / weight / seed are
 * [H,W] planes; depth_mask [H,W] or NULL (= 1).  Per pixel, in float, in this order and uncontracted:
 *   r        = m * (invdepth - invdepth_gt)
 *   weight   = (float)depth_weight * (m * m)       (plane 3 of a GSLM_MV_DEPTH pixel_weight)
 *   seed     = (-weight) * r                       (plane 3 of a GSLM_MV_DEPTH pixel_seed; for a mask of zeros and
 *                                                   ones this is -lambda_d m_d^2 (D - Dgt), the term of J^T b above)
 * and *loss_dev = [*loss_dev if accumulate] + sum over pixels of depth_weight * ((double)r * (double)r): per thread in
 * pixel order p, p + stride, ..., then gslm_lm_residual's block sums and final pass, without its factor 2.
 * residual, weight and seed are optional (NULL: not written; all three NULL: the loss alone).  A NaN invdepth gives a
 * NaN r, seed and loss.  scratch >= gslm_residual_scratch_bytes(H, W).  GSLM_ERR_INVALID, before any launch and with
 * the outputs untouched: negative sizes, a NULL invdepth / invdepth_gt with H W > 0, a NULL loss_dev or scratch, a
 * depth_weight that is negative or not finite; GSLM_ERR_CAPACITY for a scratch that is too small. */
int gslm_lm_residual_depth(int32_t H, int32_t W, const float* invdepth, const float* invdepth_gt,
                           const float* depth_mask, double depth_weight, float* residual, float* weight, float* seed,
                           void* scratch, size_t scratch_bytes, double* loss_dev, int32_t accumulate, void* stream);
/* GSLM_MV_DEPTH in opts->flags (no extension struct: it composes with GSLM_MV_LEAN and GSLM_MV_SH_REST_PROJECTED):
 * pixel_weight is [4,H,W] and opts->pixel_seed, when given, is [4,H,W]; the fourth plane is the depth block's weight
 * or seed (gslm_lm_residual_depth's).  It selects the RENDER stage's kernel only: the tile pass carries
 * dD = sum 1/z d(alpha T) beside the colour tangent, u_3 = w_3 dD seeds the back-to-front pass, and dL/dalpha gains
 * <1/z, u_3>; with a fourth plane of zeros y, dot_vy and J^T b are bitwise those of the call without the flag.
 * Accepted by gslm_matvec_view_ex and gslm_matvec_view_active.  GSLM_ERR_INVALID before anything is launched (outputs
 * untouched): mask_xyz = 0, GSLM_MV_EXPOSURE, GSLM_MV_DAMP_VEC, jv_out, GSLM_STAGE_SCREEN; and from gslm_tangent_views,
 * gslm_gather_views and gslm_gather_screen (and their _active forms). */
#define GSLM_MV_DEPTH 32
/* The line search's loss with the depth block: gslm_rasterize_loss and gslm_rasterize_loss_slot (the same arguments,
 * workspaces, scratch and error returns) with the inverse depth accumulated in the blend exactly as gslm_rasterize
 * does and, per pixel after its three colour terms, the term depth_weight / 2 * ((double) r (double) r) of
 * r = m_d (D - invdepth_gt) (gslm_lm_residual_depth's float arithmetic), which the final pass doubles with the tile
 * sums: *loss_dev = [*loss_dev if accumulate] + 2 sum ||m clamp01(R) - gt||^2 + depth_weight sum r^2, the loss of
 * gslm_rasterize + gslm_lm_residual + gslm_lm_residual_depth up to the grouping of the double sum.  invdepth_gt [H,W];
 * depth_mask [H,W] or NULL (= 1).  The slot form blends set `slot` of a union binning by that set's own masks and
 * records (which carry 1/z), as gslm_rasterize_loss_slot does.  GSLM_ERR_INVALID before any launch, the loss
 * untouched: a NULL invdepth_gt, a depth_weight that is negative or not finite, and everything the plain forms
 * refuse.  There is no all-sets, device-count, exposure or robust form. */
int gslm_rasterize_loss_depth(const gslm_view* view, int64_t P, void* geom, void* binning, size_t binning_bytes,
                              int64_t num_rendered, const float* gt, const float* alpha_mask, const float* invdepth_gt,
                              const float* depth_mask, double depth_weight, void* scratch, size_t scratch_bytes,
                              double* loss_dev, int32_t accumulate, void* stream);
int gslm_rasterize_loss_slot_depth(const gslm_view* view, int64_t P, const void* geom, size_t set_bytes,
                                   const void* binning, size_t binning_bytes, int64_t num_rendered, int32_t slot,
                                   int32_t n_sets, const float* gt, const float* alpha_mask, const float* invdepth_gt,
                                   const float* depth_mask, double depth_weight, void* scratch, size_t scratch_bytes,
                                   double* loss_dev, int32_t accumulate, void* stream);

/* ---- SSIM residual of the LM step (solver/batch_training_loss.py:18-30 with
 * disable_ssim=False, FUSED_SSIM_AVAILABLE=False, on utils/loss_utils.py:91-122 ssim_per_pixel) ----
 * Per view: r1 = a sqrt(|x - gt| + 1e-6), r2 = b sqrt(|1 - SSIM(x, gt)| + 1e-6) with x = m clamp(color, 0, 1),
 * a = sqrt((1 - lambda) / 3HW), b = sqrt(lambda / 3HW) (batch_training_loss.py:69-77); residual vector
 * [r1; r2], loss = ||r1||^2 + ||r2||^2.  `state` (gslm_ssim_state_bytes) keeps the linearisation at x.
 * gslm_ssim_residual: *loss_dev = [*loss_dev if accumulate] + loss; r1 / r2 / seed optional; seed =
 *   dL/dcolor of J^T b = -M (d1 r1 + S^T c2 r2) (feed it to gslm_matvec_view_ex's pixel_seed).
 * gslm_ssim_normal: u = M (d1^2 + S^T c2^2 S) M jv, the image-space factor of J^T J: with jv = J v
 *   (gslm_matvec_opts.jv_out), pixel_seed = u gives J^T J v.  Overwrites the state's scratch plane, so
 *   call gslm_ssim_residual with seed != NULL before the first gslm_ssim_normal of a geometry. */
size_t gslm_ssim_state_bytes(int32_t H, int32_t W);
int gslm_ssim_residual(int32_t H, int32_t W, const float* color, const float* gt, const float* alpha_mask,
                       float lambda_dssim, void* state, size_t state_bytes, float* r1, float* r2, float* seed,
                       double* loss_dev, int32_t accumulate, void* stream);
int gslm_ssim_normal(int32_t H, int32_t W, const float* gt, void* state, const float* jv, float* u, void* stream);

/* ---- the first-order loss's SSIM term (train.py:121-125 ssim(image, gt) = utils/loss_utils.py:59-89 with
 * size_average; upstream's optional fused_ssim plays this role) ----
 * img, gt [C,H,W] f32.  gslm_ssim_mean: *ssim_out (device f32) = mean of the SSIM map (11-tap Gaussian
 * window, sigma 1.5, zero padding), and `state` keeps the map's linearisation for the backward.
 * gslm_ssim_mean_backward: grad_img = *grad_out * d mean(SSIM) / d img (grad_out: device f32 scalar). */
size_t gslm_ssim_mean_state_bytes(int32_t C, int32_t H, int32_t W);
int gslm_ssim_mean(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, void* state,
                   size_t state_bytes, float* ssim_out, void* stream);
int gslm_ssim_mean_backward(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, const void* state,
                            const float* grad_out, float* grad_img, void* stream);

/* ---- distCUDA2 (simple-knn, called at scene/gaussian_model.py:249 to initialise scales) ----
 * out[i] = mean of the squared distances from point i to its 3 nearest other points (exact; FLT_MAX
 * for missing neighbours when n < 4).  xyz [n,3] f32.  Synchronises once (bounding box -> grid size).
 * scratch >= gslm_knn_scratch_bytes(n). */
size_t gslm_knn_scratch_bytes(int64_t n);
int gslm_knn3_mean_dist(int64_t n, const float* xyz, float* out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- first-order training step ----
 * One parameter group of GaussianModel.training_setup (scene/gaussian_model.py:273-280: xyz, f_dc, f_rest,
 * opacity, scaling, rotation; the exposure optimizer of :291 is one more group).  grad == NULL skips the
 * group (torch.optim skips parameters whose .grad is None). */
#define GSLM_ADAM_MAX_GROUPS 8
typedef struct gslm_adam_group {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;                   /* floats in the group */
  int32_t floats_per_gaussian; /* sparse: n == floats_per_gaussian * num_gaussians */
  int32_t _pad;
  double lr;                   /* param_group["lr"] */
  int64_t step;                /* dense: state["step"] after its increment (bias correction 1 - beta^step) */
} gslm_adam_group;
/* sparse == 0: torch.optim.Adam(params, lr, eps) step (train.py:184-186) -- its foreach arithmetic in f32:
 *   m += (1-b1)(g-m); v = v b2 + (1-b2) g g; p += (-lr/(1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps).
 * sparse != 0: SparseGaussianAdam.step(visible, num_gaussians) (train.py:180-183; gaussian_model.py:29,286,
 *   upstream 3dgs_accel rasterizer, absent): elements of Gaussians with visible[g] == 0 untouched, others
 *   m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p += -lr m / (sqrt(v) + eps)  (no bias correction).
 * One launch for all groups. */
int gslm_adam_step(const gslm_adam_group* groups, int32_t ngroups, double beta1, double beta2, double eps,
                   const uint8_t* visible, int64_t num_gaussians, int32_t sparse, void* stream);
/* train.py:166-167 (gaussian_model.py:561-563) fused, for the Gaussians with radii > 0 (render()'s
 * visibility_filter): max_radii2D = max(max_radii2D, radii) (skipped when max_radii2D is NULL),
 * xyz_gradient_accum += ||means2D_grad[i, 0:2]||, denom += 1.  means2D_grad rows are grad_stride floats. */
int gslm_densify_stats(int64_t P, const float* means2D_grad, int64_t grad_stride, const int32_t* radii,
                       float* max_radii2D, float* xyz_gradient_accum, float* denom, void* stream);

/* ---- diagnostics: device-to-device copies of internal buffers (any output may be NULL) ----
 * point_list [N] u32 (Gaussian id per sorted slot), ranges [ntiles*2] u32, tiles_touched [P] u32,
 * final_T [H*W] f32, n_contrib [H*W] u32, render records [P*12] f32. */
int gslm_inspect(const void* geom, int64_t P, const void* binning, int64_t num_rendered, int32_t H, int32_t W,
                 const void* image, uint32_t* point_list, uint32_t* ranges, uint32_t* tiles_touched,
                 float* final_T, uint32_t* n_contrib, float* records, void* stream);

/* The LM row map of the last RENDER stage on this geometry (valid while GSLM_MV_TAIL_CLEAN may be passed), copied
 * device to device: goff [P] u32 (first goff-order slot of each Gaussian's tiles_touched entries) and hscan
 * [num_rendered + 1] u32 (head entries among the slots before each) -- Gaussian i's head rows are
 * [hscan[goff[i]], hscan[goff[i] + tiles_touched[i]]).  Either output may be NULL.  Additive, still ABI 9. */
int gslm_inspect_rowmap(const void* geom, int64_t P, int64_t num_rendered, const void* scratch, size_t scratch_bytes,
                        uint32_t* goff, uint32_t* hscan, void* stream);

/* The sorted list's raw words of a binning, copied device to device: words [num_rendered] u32 (Gaussian id in the low
 * 28 bits, quadrant mask in the top 4 -- the binning's masks, or those the LM row map refined to the visits some
 * pixel blends, GSLM_LIVE_MASKS) and slots [num_rendered] u32 (the row map's head-row slot of each sorted entry;
 * valid as gslm_inspect_rowmap's outputs are).  Either output may be NULL.  Additive, still ABI 9. */
int gslm_inspect_list(const void* binning, size_t binning_bytes, int64_t num_rendered, int32_t H, int32_t W,
                      uint32_t* words, uint32_t* slots, void* stream);

/* Device self-test of the wave primitives (one 64-lane wave).  in: [64][8] floats, out: [64].
 * which = 0: transposed 8-value reduction (lane l returns the sum of value (l >> 3) & 7);
 * which = 1: DPP sum of in[l*8] (lane 63 returns the total). */
int gslm_selftest(int32_t which, const float* in, float* out, void* stream);
/* Device self-test of the library's exclusive u32 scan (the tile-count and LM row-map scans): out[i] = sum_{j<i} in[j],
 * *total = the sum (both device).  force_top != 0 takes the long-scan form (a scan of the block sums in a launch of
 * its own, used above 4096 blocks of 2048) at any n.  tmp: >= 8 ceil(n / 2048) + 64 bytes of device scratch, rounded
 * up to a multiple of 256. */
int gslm_selftest_scan(const uint32_t* in, uint32_t* out, int64_t n, int32_t force_top, void* tmp, size_t tmp_bytes,
                       uint32_t* total, void* stream);
/* The same for the dual scan (the binning's two offset sequences in one pass): out_a[i] = sum_{j<i} in[j] and
 * out_b[i] = sum_{j<i} b[j], with b = in_b, or in gathered through idx (a permutation of [0, n)) when in_b is NULL;
 * exactly one of idx and in_b is given.  *total_a, *total_b = the two sums.  tmp as gslm_selftest_scan (it holds
 * both sequences' block sums). */
int gslm_selftest_scan_dual(const uint32_t* in, const uint32_t* idx, const uint32_t* in_b, uint32_t* out_a,
                            uint32_t* out_b, int64_t n, int32_t force_top, void* tmp, size_t tmp_bytes,
                            uint32_t* total_a, uint32_t* total_b, void* stream);
/* Device self-tests of the three binning primitives behind every image (additive, still ABI 9): thin wrappers of the
 * library's own launchers, all buffers device memory unless noted.
 *
 * gslm_selftest_sort: the stable LSD radix sort of (u32 key, u32 value) pairs on key bits [0, end_bit), 1 <= end_bit <=
 * 32 (the tile sort, the depth sort, the union binning's payload sort, the k-NN cell sort): ceil(end_bit / 8) passes
 * of ceil(end_bit / passes) bits, the last one the rest (13 bits: 7 + 6, not 8 + 5), keys equal on those bits keep their input order, and the bits at or above
 * end_bit travel with their key unchanged.  k0 / v0 hold the input, k1 / v1 are their ping-pong partners, n words each;
 * *result_in_alt (host) = 1 when the sorted pairs are in k1 / v1 (an odd pass count), 0 when in k0 / v0.
 *   iota_values != 0: the values are the indices 0..n-1 and v0 is not read (it may be NULL).
 *   last_gather (or NULL): a table the last pass reads -- the output key slot i holds last_gather[value i] in place of
 *     the sorted key.
 *   n_dev (or NULL, device u32): n is a capacity and the first min(n, *n_dev) pairs are sorted; nothing past that
 *     count is written.
 *   p0 / p1 (both or neither): a payload word per pair, moved with it; the result is in p1 exactly when *result_in_alt.
 *   key_range != 0 (end_bit 32, no payload, no n_dev; refused otherwise): the depth sort's form, which sorts
 *     key - min over the keys other than 0xFFFFFFFF in as many byte passes as that span needs and copies in the rest --
 *     the same output as the plain 32-bit sort.
 *   hist: gslm_selftest_sort_hist_bytes(n, payload != 0) bytes of scratch, 8-byte aligned.  On return its words
 *     [256 nb, 256 nb + 256), nb = (bytes - 1040) / 1032, hold the last pass's count of keys per digit.
 * GSLM_ERR_INVALID for n < 0, end_bit outside 1..32, a NULL buffer, one payload buffer without the other or a refused
 * key_range combination; GSLM_ERR_CAPACITY for a short hist; nothing is launched then, or when n == 0. */
size_t gslm_selftest_sort_hist_bytes(int64_t n, int32_t payload);
int gslm_selftest_sort(uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, uint32_t* p0, uint32_t* p1, int64_t n,
                       int32_t end_bit, int32_t iota_values, int32_t key_range, const uint32_t* last_gather,
                       const uint32_t* n_dev, void* hist, size_t hist_bytes, int32_t* result_in_alt, void* stream);
/* gslm_selftest_ranges: the per-tile [start, end) of a sorted list of n tile ids, each below ntiles (keys: 16-byte
 * aligned): ranges [ntiles][2] is zeroed, then tile t's pair set to its run of keys; an absent tile stays (0, 0).
 * n_dev (or NULL): n is a capacity and the list the first min(n, *n_dev) keys (the rest are not read); n_out (or
 * NULL, only with n_dev; not written when n == 0) then receives *n_dev itself, uncapped. */
int gslm_selftest_ranges(const uint32_t* keys, int64_t n, int32_t ntiles, const uint32_t* n_dev, uint32_t* n_out,
                         uint32_t* ranges, void* stream);
/* gslm_selftest_tile_order: the tile passes' launch order, order [ntiles] a permutation of the tiles, by each tile's
 * cost[t], or with cost == NULL its list length ranges[t][1] - ranges[t][0].  form 0: heaviest first over the whole
 * frame, in buckets of the cost (exact below 768, 32 wide above, one bucket from 8928 on; arbitrary inside a bucket).
 * form 1: the tiles cut in row-major order into 8 bands of about equal weight (cost + 1), each band heaviest first,
 * and the bands interleaved -- entry 8 k + g is band g's k-th tile while every band still has one, the bands'
 * leftovers follow band by band.  The form is the argument's, whatever GSLM_TILE_ORDER says. */
int gslm_selftest_tile_order(const uint32_t* ranges, const uint32_t* cost, int32_t ntiles, int32_t form,
                             uint32_t* order, void* stream);

const char* gslm_last_error(void);
int gslm_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GSLM_H */
