/* qsp_hip.h -- C-ABI of the MI355X-native joint object-optimisation hot path of QSP-SLAM.
 *
 * One shared library (libqsp_hip.so) exports every symbol declared here: plain pointers and sizes, int status
 * returns, no exceptions across the boundary, no torch / Eigen / OpenCV types.  Each entry point names the reference
 * interface it replaces (paths relative to the reference root, GetOverMassif/QSP-SLAM).
 *
 * Threading: a handle (decoder, batch, BA problem) may be used by one host thread at a time; distinct handles are
 * independent.  The reference calls both paths from the LocalMapping thread under the GIL (include/System.h:61-75).
 *
 * Path A  (DeepSDF object refinement)  replaces reconstruct/optimizer.py + reconstruct/loss.py + loss_utils.py
 * Path B  (joint bundle adjustment)    replaces src/Optimizer.cc, src/Optimizer_util.cc, include/ObjectPoseGraph.h
 *                                      on top of Thirdparty/g2o (BlockSolver_6_3 + LM + LinearSolverEigen)
 */
#ifndef QSP_HIP_H
#define QSP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------
 * status codes
 * ------------------------------------------------------------------------------------------------------------ */
enum {
    QSP_OK = 0,
    QSP_ERR_INVALID = 1,      /* bad argument (null pointer, negative size, inconsistent counts)            */
    QSP_ERR_UNSUPPORTED = 2,  /* decoder architecture outside the supported family (see qsp_decoder_create) */
    QSP_ERR_DEVICE = 3,       /* a HIP call failed; qsp_last_error() holds the text                          */
    QSP_ERR_NO_DEVICE = 4     /* no gfx950 device visible -- there is no CPU fallback                        */
};

const char* qsp_last_error(void);   /* thread-local text of the last failure */
int qsp_version(void);              /* ABI version, currently 1 */
int qsp_device_count(void);

/* ===============================================================================================================
 * Path A -- DeepSDF decoder and object refinement
 * ============================================================================================================ */

/* Decoder description.  Replaces deep_sdf/workspace.py:202-224 (config_decoder) + deep_sdf/deep_sdf_decoder.py:9-110.
 * weight[l] is (out_dim[l], in_dim[l]) row-major.  If weight_g != NULL and weight_g[l] != NULL, weight[l] is the
 * weight-norm direction v and the effective matrix is g * v / ||v||_row (old-style torch weight_norm, dim 0), folded
 * once at creation instead of on every call as the reference does.
 * Supported family: n_layers = 9, hidden width 512, code_len = 64, latent_in_layer = 4 (the DSP-SLAM "8 x 512"
 * decoder: 67->512, 512->512 x2, 512->445, 512->512 x4, 512->1, ReLU, final tanh).  Anything else: QSP_ERR_UNSUPPORTED. */
typedef struct {
    int32_t n_layers;
    int32_t code_len;
    int32_t latent_in_layer;
    const int32_t* in_dim;
    const int32_t* out_dim;
    const float* const* weight;
    const float* const* weight_g;   /* may be NULL */
    const float* const* bias;
} qsp_decoder_desc;

typedef struct qsp_decoder qsp_decoder;

/* Threads.  A decoder owns one HIP stream, one resident refinement batch and a few fields that a call rewrites for its own duration
 * (the f32 override of a range fallback, the screening margin of a self-check repeat).  Every entry point that launches on a
 * decoder -- qsp_decode_sdf*, qsp_sdf_value_grad, qsp_refine_batch_set_state / _run / _get, qsp_reconstruct_objects,
 * qsp_estimate_pose, qsp_refine_detections, qsp_mesh_extract / _from_volume and their batch forms, qsp_decoder_set_option -- takes the decoder's lock:
 * host threads may share a decoder and get correct results, one call at a time.  Threads that should overlap on the GPU use a
 * decoder each.  A call on a decoder GROUP (qsp_decoder_group_create below) -- the *_group entry points and the batch calls on a
 * group's batch -- takes the lock of every member, always in the same order (by address), so it cannot deadlock against
 * single-decoder calls or other group calls on other threads; it runs on its first member's stream. */
int qsp_decoder_create(const qsp_decoder_desc* desc, int device, qsp_decoder** out);
/* Batches and mesh extractors created from a decoder use it until they are destroyed: destroy them first.  (Destroying one of
 * them after its decoder only frees its own memory and is harmless; any other call on it is undefined.)  With decoder groups:
 * destroy the group's batches, then the group, then its decoders. */
void qsp_decoder_destroy(qsp_decoder* dec);

/* Decoder options.  QSP_DEC_OPT_FORWARD_PRECISION selects the arithmetic of the FORWARD-ONLY decoder passes (qsp_decode_sdf,
 * the voxel-grid decode of qsp_mesh_extract, the ray-sample forward pass of the refinement, reconstruct/loss.py:78):
 *   0 (default)  exact float32 multiply-adds on the f32 matrix pipe (v_mfma_f32_32x32x2_f32);
 *   1            every f32 weight and activation as the exact sum of three bf16 values, six bf16 products per multiply-add on
 *                the bf16 matrix pipe with f32 accumulation (v_mfma_f32_32x32x16_bf16): float32-equivalent accuracy (2.2e-7
 *                relative on the SDF value against float64; plain f32: 1.8e-7) at up to 2.67 x the f32 pipe's rate.  Results
 *                differ from mode 0 in the last bits, as two float32 implementations with different summation orders do;
 *   2            every f32 weight and activation as two fp16 values, x = hi + 2^-11 lo' (22 significand bits), three fp16
 *                products per multiply-add on the fp16 matrix pipe with f32 accumulation (v_mfma_f32_32x32x16_f16): the same
 *                float32-equivalent accuracy (1.8e-7) at up to 5.3 x the f32 pipe's rate.  fp16's range is the precondition:
 *                qsp_decoder_set_option returns QSP_ERR_UNSUPPORTED for a decoder with a weight beyond +-65 000, and a call
 *                during which an activation or a back-propagated gradient exceeded 65 504 in magnitude FAILS with
 *                QSP_ERR_UNSUPPORTED instead of returning numbers (its outputs are then undefined; modes 0 and 1 have no such
 *                limit).  A DeepSDF decoder's activations are O(10).
 * QSP_DEC_OPT_JACOBIAN_PRECISION selects the same (0, 1, 2) for the forward+backward pass that builds the Jacobian rows and the
 * normal equations (qsp_sdf_value_grad and the fused kernel of the refinement, reconstruct/loss_utils.py:82-103): that pass has
 * no discrete decision besides the ReLU masks, so modes 1 and 2 move H, b by float32 rounding noise only.
 * QSP_DEC_OPT_TILE_POINTS (64, the default, or 32): points per workgroup tile of the Jacobian / normal-equation kernel of the
 * refinement batches created AFTER the call (the forward pass over the ray samples keeps 64).  A single object of a few
 * thousand surface points fills only tens of the 256 CUs with 64-point tiles; 32-point tiles spread it over twice as many work
 * items at ~0.67 of the time each -- the latency option for the reference's one-object-per-call pattern
 * (reconstruct/optimizer.py:96-281 called from src/LocalMapping_util.cc:705-760).  Exists on the split-fp16 pipe only (both
 * precisions = 2; qsp_refine_batch_create returns QSP_ERR_UNSUPPORTED otherwise).  The partition of the normal-equation
 * partial sums follows the tile size, so results are bit-reproducible per tile size, not across the two.
 * QSP_DEC_OPT_RENDER_SCREENING (value = margin in units of 1e-6 SDF, 0 = off, the default): the ray-sample forward pass of the
 * refinement (reconstruct/loss.py:78) in two passes.  The render term clamps -- a sample with |sdf| >= cut_off contributes an
 * occupancy of exactly 0 or 1 (reconstruct/loss_utils.py:40-48) -- so away from the surface only the SIGN of the value is used.
 * Pass 1 evaluates every sample with one fp16 term per operand (a third of the matrix-pipe work, 128-point tiles); pass 2
 * re-evaluates the samples with |s1| < cut_off + margin on the split-fp16 pipe and overwrites them.  With margin >= the
 * largest |s1 - s3| the result (K, n_valid, H, b, every later iterate) equals the unscreened split-fp16 result BIT FOR BIT;
 * 20 000 (0.02) is > 8 x the largest difference measured over the fixtures and the randomised sweep (profiles/r03_*).  Needs
 * QSP_DEC_OPT_FORWARD_PRECISION = 2 (QSP_ERR_UNSUPPORTED otherwise); margins above 5 x the usual cut_off (50 000) are refused:
 * at that point the second pass covers most samples and the option has no purpose.  The premise is checked on every run: the
 * second pass has both values of each band sample in hand and keeps the largest |s1 - s3|; a run in which it exceeds HALF the
 * margin is repeated from its starting state in one pass (qsp_decoder_get_counter(QSP_DEC_CNT_SCREEN_FALLBACKS) counts them,
 * qsp_refine_profile.screen_max_diff / .screen_fallbacks report the last run), so a decoder whose screening values are worse
 * than the fixtures' costs time, not bits.
 * QSP_DEC_OPT_SCREEN_AUDIT (N, default 100; 0 = off, 1 = every sample): the band check alone looks only where the screening pass
 * put a sample INSIDE the band.  The second pass therefore also re-evaluates a fixed pseudo-random one in N of the samples the
 * screening pass put OUTSIDE (a hash of hypothesis, sample and iteration), folds their |s1 - s3| into screen_max_diff, and counts
 * each one whose split-fp16 value lies inside the cut-off or has the other sign -- a clamp the one-pass result would not have
 * made -- as a hard failure (qsp_refine_profile.screen_audit_failures): the run is repeated in one pass like above.  An audited
 * sample's overwritten value is only ever read through the clamp, so the audit changes no bit of a passing run.
 * QSP_DEC_OPT_DEPTH_STAGING (1, the default: batches of more than 64 rounds of 128-sample tiles over the chip / 2: always / 0: never):
 * a screened run evaluates the ray samples in two depth stages -- indices [0, D/2)
 * of every ray, then [D/2, D) of the rays that have no OPAQUE sample (sdf <= -cut_off: occupancy exactly 1) yet.  Behind an
 * opaque sample the transmittance of reconstruct/loss.py:101 is exactly 0, so those samples' values reach no output (every term
 * they enter is multiplied by that zero; d e / d o of an in-band one is 0 and dropped by the 1e-2 rule, :103-128): they are not
 * evaluated.  ~20 % of the samples on the synthetic scenes; every output bit-identical to 0 (tests/test_gpu_screening.py).  Only
 * a decoder that returns NaN behind a surface would tell the two apart.
 * QSP_DEC_OPT_SCREENING_MIN_SAMPLES (-1, the default, or a count): a run is screened only when its batch holds more ray samples
 * (rays x depth samples, summed over the hypotheses) than this; -1 = more than two rounds of 64-point tiles over the chip.  A
 * batch that fits one round -- one object per call -- is one tile deep either way and faster in one pass.  The result is the
 * same bits whichever way a run goes.  0 = always screen (tests).
 * QSP_DEC_OPT_NARROW_TILE (1 / 0): decoders much smaller than the 8 x 512 shape they are embedded in (e.g. 4 x 256 / code 32: less
 * than half of its multiply-adds) run the NARROW form of the split-fp16 tile by default -- identity slots, all-zero k-slabs and
 * all-zero column blocks are skipped, exactly; 0 evaluates the embedded form at the full shape's cost (measurements, tests);
 * QSP_DEC_CNT_NARROW_TILE says which is in use.  Other pipes (f32, split bf16) always run the embedded form.
 * QSP_DEC_OPT_USE_TANH (0 / 1): NetworkSpecs.use_tanh of deep_sdf/deep_sdf_decoder.py:66-68,92-94 -- a tanh on the output
 * layer in front of the final tanh.
 * QSP_DEC_OPT_RANGE_FALLBACK (1, the default / 0): when a split-fp16 kernel meets an activation or gradient outside fp16's
 * range, 1 re-runs THAT call on the exact-f32 pipe inside the library and returns its result (counted by
 * qsp_decoder_get_counter(QSP_DEC_CNT_RANGE_FALLBACKS)); 0 fails the call with QSP_ERR_UNSUPPORTED as round 2 did. */
enum { QSP_DEC_OPT_FORWARD_PRECISION = 1, QSP_DEC_OPT_JACOBIAN_PRECISION = 2, QSP_DEC_OPT_TILE_POINTS = 3,
       QSP_DEC_OPT_RENDER_SCREENING = 4, QSP_DEC_OPT_USE_TANH = 5, QSP_DEC_OPT_RANGE_FALLBACK = 6,
       QSP_DEC_OPT_SCREENING_MIN_SAMPLES = 7, QSP_DEC_OPT_NARROW_TILE = 8, QSP_DEC_OPT_SCREEN_AUDIT = 9,
       QSP_DEC_OPT_DEPTH_STAGING = 10 };
enum { QSP_DEC_CNT_RANGE_FALLBACKS = 1, QSP_DEC_CNT_ARENA_REUSED = 2, QSP_DEC_CNT_ARENA_CREATED = 3, QSP_DEC_CNT_NARROW_TILE = 4,
       QSP_DEC_CNT_SCREEN_FALLBACKS = 5 };
/* lifetime counters of a decoder: calls that were re-run on the f32 pipe because a value left fp16's range; calls of
 * qsp_reconstruct_objects that refilled the decoder's resident batch / that had to (re)allocate it */
int64_t qsp_decoder_get_counter(qsp_decoder* dec, int32_t counter);
int qsp_decoder_set_option(qsp_decoder* dec, int32_t option, int32_t value);

/* decode_sdf, reconstruct/loss_utils.py:51-79.  Host pointers: code (code_len), xyz (n,3) row-major, sdf_out (n). */
int qsp_decode_sdf(qsp_decoder* dec, const float* code, const float* xyz, int64_t n, float* sdf_out);

/* Diagnostic: the values the FIRST pass of QSP_DEC_OPT_RENDER_SCREENING computes (one fp16 term per operand).  They are not
 * SDF values of the decoder's precision and nothing in the library returns them as such; tests and tools/screen_margin.py use
 * this entry to measure |s1 - s3|, the quantity the screening margin has to cover.  Host pointers. */
int qsp_decode_sdf_screen(qsp_decoder* dec, const float* code, const float* xyz, int64_t n, float* s1_out);

/* get_batch_sdf_jacobian, reconstruct/loss_utils.py:82-103 (out_dim = 1): y (n) and d y / d [code | xyz] (n, code_len+3),
 * without the weight gradients the reference's autograd also accumulates and never uses.  Host pointers. */
int qsp_sdf_value_grad(qsp_decoder* dec, const float* code, const float* xyz, int64_t n, float* y, float* grad);

/* The `optimizer` block of the detector-config JSON (configs/config_*.json:21-41) read by
 * reconstruct/optimizer.py:27-44. */
typedef struct {
    float k1, k2, k3, k4;      /* render, sdf, code-prior, rotation-prior weights                    */
    float b1, b2;              /* Huber thresholds: render, sdf                                       */
    float lr;                  /* learning_rate                                                       */
    float s_damp;              /* scale_damping                                                       */
    float cut_off;             /* cut_off_threshold (SDF -> occupancy)                                */
    int32_t n_iter;            /* joint_optim.num_iterations                                          */
    int32_t n_depth;           /* num_depth_samples (<= 64)                                           */
    int32_t code_len;          /* 64                                                                  */
} qsp_joint_cfg;

/* A resident batch of refinement hypotheses.  An *object* owns the observations of one detection (surface points,
 * rays, depths: the arguments src/LocalMapping_util.cc:585-672 assembles); a *hypothesis* is one call of
 * Optimizer.reconstruct_object (reconstruct/optimizer.py:96-281) on an object from its own initial pose/code -- the
 * reference makes flip_sample_num (=4) such calls per object, serially (LocalMapping_util.cc:705-760).  All
 * hypotheses of a batch advance together, one fused launch sequence per Gauss-Newton iteration, with no host
 * synchronisation inside the iteration loop. */
typedef struct qsp_refine_batch qsp_refine_batch;

/* pts[o]: (n_pts[o],3) row-major camera-frame points; rays[o]: (n_rays[o],3); depth[o]: (n_fg[o]) observed depth of
 * the first n_fg[o] rays (the rest are background rays).  hyp_obj[h] = object index of hypothesis h.  Host pointers;
 * everything is copied to the device here and stays resident. */
int qsp_refine_batch_create(qsp_decoder* dec, const qsp_joint_cfg* cfg, int32_t n_obj,
                            const float* const* pts, const int32_t* n_pts,
                            const float* const* rays, const int32_t* n_rays,
                            const float* const* depth, const int32_t* n_fg,
                            int32_t n_hyp, const int32_t* hyp_obj, qsp_refine_batch** out);
void qsp_refine_batch_destroy(qsp_refine_batch* b);

/* (re)initialise every hypothesis: t_cam_obj (n_hyp,4,4) row-major Sim3 object->camera, code (n_hyp,code_len) or NULL
 * for the zero code (reconstruct/optimizer.py:111-119).  Clears is_good/loss. */
int qsp_refine_batch_set_state(qsp_refine_batch* b, const float* t_cam_obj, const float* code);

/* Run n_iter Gauss-Newton iterations (n_iter <= 0: cfg.n_iter) and wait for completion. */
int qsp_refine_batch_run(qsp_refine_batch* b, int32_t n_iter);

/* Results per hypothesis: t_cam_obj_out (n_hyp,4,4), code_out (n_hyp,code_len), loss_out (n_hyp), is_good_out (n_hyp).
 * is_good = 0 reproduces the reference's early exits (fewer than 10 ray samples in the unit ball, NaN loss):
 * the pose/code outputs of such a hypothesis are unspecified, loss is that of the last completed iteration. */
int qsp_refine_batch_get(qsp_refine_batch* b, float* t_cam_obj_out, float* code_out, float* loss_out,
                         uint8_t* is_good_out);

/* Introspection of the LAST iteration run, for parity tests: H (n_hyp,71,71), rhs (n_hyp,71), dx (n_hyp,71),
 * n_valid (n_hyp) ray samples inside the unit ball, n_render (n_hyp) render rows K, loss terms (n_hyp,2) =
 * (sdf, render).  Any pointer may be NULL. */
int qsp_refine_batch_trace(qsp_refine_batch* b, float* H, float* rhs, float* dx, int32_t* n_valid,
                           int32_t* n_render, float* loss_terms);
/* ... and the rotation prior's own terms of that iteration (reconstruct/loss.py:155-178): rot4 (n_hyp,4) = J_rot (the three
 * rotation entries 3..5 of J_sim3) and res_rot -- lets a parity test separate the decoder part of rhs from the k4-weighted one. */
int qsp_refine_batch_trace_rot(qsp_refine_batch* b, float* rot4);

/* Parity-test tap.  enable != 0 (with NULL outputs) before a run makes the fused kernel also store every augmented Jacobian
 * row it feeds to the normal equations: [d e/d xi (7) | d e/d code (64) | robust residual] = 72 floats per row.  After
 * the run, a second call with outputs copies hypothesis `hyp`: rows_sdf (n_pts,72), rows_render (n_render,72) of the LAST
 * iteration.  Reference quantities: jac_toc / jac_code / robust residual of reconstruct/loss.py:22-43,143-150 and
 * loss_utils.py:250-265.  enable == 0 frees the tap buffer. */
int qsp_refine_batch_rows(qsp_refine_batch* b, int enable, int32_t hyp, float* rows_sdf, float* rows_render);

/* Timing of the last qsp_refine_batch_run, measured with HIP events on the library's own stream. */
typedef struct {
    float ms_total;          /* first launch -> last kernel complete                                  */
    float ms_mlp_jtj;        /* sum over launches of the fused MLP fwd+bwd+JtJ kernel                */
    float ms_mlp_fwd;        /* sum over launches of the forward-only MLP kernel (ray samples)       */
    float ms_other;          /* ray sampling, render scan, reduce+solve                              */
    int32_t n_launch_jtj, n_launch_fwd;
    int64_t pts_jtj;         /* points through fwd+bwd (sdf points + render rows), all iterations     */
    int64_t pts_fwd;         /* points through forward only (valid ray samples), all iterations       */
    int64_t tiles_jtj, tiles_fwd;   /* 64-point tiles actually executed (incl. padding rows)          */
    int64_t pts_band;        /* screened forward pass: samples re-evaluated by the second pass (0 when off) */
    int32_t range_fallbacks; /* 1 if this run was repeated on the f32 pipe (QSP_DEC_OPT_RANGE_FALLBACK)     */
    int32_t screen_fallbacks;/* 1 if this run was repeated in one pass (screening self-check, QSP_DEC_OPT_RENDER_SCREENING) */
    float screen_max_diff;   /* largest |s1 - s3| the second pass saw on a band or audited sample (0 when not screened)      */
    int32_t screen_audit_failures; /* audited OUT-of-band samples whose split-fp16 value was inside the cut-off or of the other
                                * sign: > 0 = the screened attempt was wrong somewhere and the run was repeated in one pass    */
    int64_t pts_audit;       /* out-of-band samples the second pass re-evaluated as the audit (QSP_DEC_OPT_SCREEN_AUDIT)      */
} qsp_refine_profile;
int qsp_refine_batch_profile(qsp_refine_batch* b, int enable, qsp_refine_profile* out);

/* One-shot entry point with the reference's per-call semantics, batched over hypotheses: fill + set_state + run + get on a
 * batch that stays resident with the decoder (sized by the high-water mark of the calls so far: no device allocation per call
 * once it has settled; released by qsp_decoder_destroy).  Optimizer.reconstruct_object, reconstruct/optimizer.py:96-281, as
 * src/LocalMapping_util.cc:705-760 calls it -- one object (x its yaw flips) per call.  Results do not depend on what the
 * resident batch held before. */
int qsp_reconstruct_objects(qsp_decoder* dec, const qsp_joint_cfg* cfg, int32_t n_obj,
                            const float* const* pts, const int32_t* n_pts,
                            const float* const* rays, const int32_t* n_rays,
                            const float* const* depth, const int32_t* n_fg,
                            int32_t n_hyp, const int32_t* hyp_obj, const float* t_cam_obj, const float* code,
                            float* t_cam_obj_out, float* code_out, float* loss_out, uint8_t* is_good_out);

/* Optimizer.estimate_pose_cam_obj, reconstruct/optimizer.py:47-93, batched: per item an SE3 t_co (4,4), a scale, surface
 * points and a code; n_iter SDF-only Gauss-Newton iterations on the 6 pose dimensions (1e-2 damping, raw residual,
 * inlier filter |res| <= 0.05 after iteration index 4).  t_co_out (n,4,4) SE3.  Host pointers.
 * An item that has no point to iterate on -- n_pts[i] = 0 (pts[i] is then not read), or every point removed by the inlier filter --
 * is no error: like the reference, which divides by the point count, the call returns QSP_OK with all 16 entries of that item's
 * matrix NaN; the other items of the call are not affected (a call whose items all have n_pts[i] = 0 launches nothing).  n <= 0, a null argument, a negative n_pts[i] or a null pts[i] with
 * n_pts[i] > 0: QSP_ERR_INVALID, t_co_out untouched. */
int qsp_estimate_pose(qsp_decoder* dec, int32_t n, const float* t_co_se3, const float* scale,
                      const float* const* pts, const int32_t* n_pts, const float* code, int32_t n_iter,
                      float* t_co_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Mesh extraction: MeshExtractor.extract_mesh_from_code, reconstruct/optimizer.py:284-304
 * = decode_sdf over the voxel grid of create_voxel_grid (reconstruct/utils.py:98-117) + marching cubes at level 0
 * (convert_sdf_voxels_to_mesh, reconstruct/utils.py:120-141, skimage.measure.marching_cubes_lewiner there).
 * Both stages run on the device; only vertices and faces come back.
 *   voxel_points (dim^3, 3): the grid in the reference's order, point index = i0*dim^2 + i1*dim + i2 (host pointer, copied).
 *   Marching cubes = Lewiner's (Lewiner et al., JGT 2003) as scikit-image 0.18's marching_cubes_lewiner runs it -- the call of
 *   reconstruct/utils.py:131 --, reproduced on the device with its case tables (csrc/mesh_lewiner.hpp): one vertex per
 *   sign-changing grid edge (+ the extra vertex of some ambiguous configurations), numbered by first use in a z-outermost sweep
 *   of the cells; faces in that sweep's order, corners reversed (gradient_direction='descent').  Same vertices, same faces, same
 *   ORDER as scikit-image on the same volume (tests/golden/mc_lewiner_*.npz hold its output).
 *   vertices: qsp_mesh_fetch gives (V,3) float32 = float32(index coordinate) * float32(2/(dim-1)) - 1; qsp_mesh_fetch_f64 gives
 *   the reference's own float64 values, float32(index coordinate) * (2.0/(dim-1)) + (-1.0), bit for bit.
 *   qsp_mesh_extractor_set_method(m, 1) selects the triangulation of rounds 2-3 instead (face-consistent segments from a
 *   generated 256-case table, vertices ordered by owning grid point then axis: the same vertex set, other diagonals).
 *
 * Batches: the reference extracts a mesh after every successful refinement (src/LocalMapping_util.cc:832); after a batched
 * refinement that is many codes at once.  qsp_mesh_extract_batch / qsp_mesh_from_volumes take n codes / volumes and give n
 * meshes, each the mesh the single call gives (decoded volume bit for bit on every precision -- one exception below --; vertex numbers from 0 and
 * face indices local to each mesh; scikit-image's values and order), with one launch per stage and one synchronisation for all
 * of them instead of per mesh.  Method 0 only: with method 1 selected both return QSP_ERR_UNSUPPORTED.  n == 0 is QSP_OK and
 * touches nothing (a batch result that is resident stays); null pointers and n < 0 are QSP_ERR_INVALID.  An item whose volume
 * has no surface has counts 0 and does not fail the call.  A split-fp16 decode that leaves fp16's range is repeated on the f32
 * pipe and counted (per pass, see below), or fails with QSP_ERR_UNSUPPORTED when QSP_DEC_OPT_RANGE_FALLBACK is 0, as
 * qsp_mesh_extract does.  The one case in which an item is NOT the single call's mesh follows from that: the range flag is
 * one per decoder, so when some items of a split-fp16 pass leave the range ALL volumes of that pass are decoded on the f32
 * pipe, also those whose single call would have stayed on the split-fp16 pipe (f32 bits instead of split-fp16 bits: inside the
 * decoder tolerance, not bit-identical).  Both calls take the decoder's lock.
 *   Passes: a batch is processed in passes of at most 64 volumes (the default; qsp_mesh_extractor_set_batch_limit sets
 *   1 .. 64).  A pass needs 20 bytes of scratch per grid point (rounded up to 2048 points per volume) and volume: 42 MB for 64
 *   volumes of 32^3, 336 MB at 64^3, 2.7 GB at 128^3 -- lower the limit where that is too much.  The n decoded volumes (4 bytes
 *   per point) and the meshes stay on the device until the next batch call; all buffers grow to the high-water mark and are
 *   freed with the extractor.  No result depends on the limit.
 *   State: single and batch calls run the same launch chain on the same scratch, which holds nothing after a call returns;
 *   the results (volumes, meshes, counts) are kept twice.  qsp_mesh_fetch / qsp_mesh_fetch_f64 give the mesh of the last
 *   successful qsp_mesh_extract / qsp_mesh_from_volume, qsp_mesh_fetch_batch the result of the last successful batch call, in
 *   whatever order single and batch calls were mixed.  A call that fails leaves no result of its kind: after a failed single
 *   call qsp_mesh_fetch / _fetch_f64 return QSP_ERR_INVALID until the next successful one (as qsp_mesh_fetch_batch does after a
 *   failed batch call) -- the volume the failed call overwrote cannot be fetched under the counts of the call before.
 *   Over a decoder group: after a refinement over a decoder group (below) the codes of one key frame belong to several classes,
 *   and the reference meshes each with the extractor of its class (src/LocalMapping_util.cc:818-835).  An extractor created
 *   with qsp_mesh_extractor_create_group (declared with the decoder groups) shares one grid between the members;
 *   qsp_mesh_extract_batch_group takes n codes and n class indices (position in the group) and gives n meshes from the same
 *   passes: one grid-decode launch in which every volume is decoded with the parameters of its class, then the stages above.
 *   Each item is bit for bit the mesh and the volume qsp_mesh_extract gives for that code on an extractor of that class's
 *   decoder, on every precision.  The exception above widens with the group: a pass is repeated whole on the f32 pipe when the
 *   range flag of ANY member is up after it (every member's tiles raise that member's flag), so items of every class in that
 *   pass carry f32 bits.  The repeat is counted the way a group refinement call counts its own: once per repeated pass, in
 *   QSP_DEC_CNT_RANGE_FALLBACKS of member 0, whichever member left the range; with QSP_DEC_OPT_RANGE_FALLBACK = 0 the call fails
 *   with QSP_ERR_UNSUPPORTED and leaves no batch result.  qsp_mesh_fetch_batch, qsp_mesh_from_volume(s), qsp_mesh_fetch(_f64),
 *   set_batch_limit, set_method and destroy work on such an extractor as on any other; the calls that take codes without classes
 *   (qsp_mesh_extract, qsp_mesh_extract_batch) return QSP_ERR_INVALID on it, as qsp_mesh_extract_batch_group does on an
 *   extractor over one decoder. */
typedef struct qsp_mesh_extractor qsp_mesh_extractor;
int qsp_mesh_extractor_create(qsp_decoder* dec, int32_t voxels_dim, const float* voxel_points, qsp_mesh_extractor** out);
void qsp_mesh_extractor_destroy(qsp_mesh_extractor* m);
/* decode the volume for `code` (64 floats) and run marching cubes; results stay on the device, counts are returned */
int qsp_mesh_extract(qsp_mesh_extractor* m, const float* code, int64_t* n_verts, int64_t* n_faces);
/* marching cubes on a caller-supplied (dim,dim,dim) volume (convert_sdf_voxels_to_mesh alone) */
int qsp_mesh_from_volume(qsp_mesh_extractor* m, const float* sdf_volume, int64_t* n_verts, int64_t* n_faces);
/* copy the last result out: verts (n_verts,3), faces (n_faces,3), optionally the (dim^3) volume; any pointer may be NULL */
int qsp_mesh_fetch(qsp_mesh_extractor* m, float* verts, int32_t* faces, float* sdf_volume);
/* the last result's vertices as float64 (n_verts,3), as convert_sdf_voxels_to_mesh returns them */
int qsp_mesh_fetch_f64(qsp_mesh_extractor* m, double* verts);
/* 0 (default): Lewiner's marching cubes, what the reference calls; 1: the face-consistent table of rounds 2-3 */
int qsp_mesh_extractor_set_method(qsp_mesh_extractor* m, int32_t method);
/* B codes (n x code_len floats) -> B meshes; counts per item; results stay on the device */
int qsp_mesh_extract_batch(qsp_mesh_extractor* m, int32_t n, const float* codes, int64_t* n_verts, int64_t* n_faces);
/* marching cubes alone on n caller-supplied (dim,dim,dim) volumes */
int qsp_mesh_from_volumes(qsp_mesh_extractor* m, int32_t n, const float* sdf_volumes, int64_t* n_verts, int64_t* n_faces);
/* last batch result, concatenated in item order; any pointer may be NULL.  verts: float32 as qsp_mesh_fetch gives them;
 * verts_f64: the reference's float64 values as qsp_mesh_fetch_f64 gives them; faces: indices local to each item's mesh;
 * sdf_volumes: (n, dim^3) */
int qsp_mesh_fetch_batch(qsp_mesh_extractor* m, float* verts, double* verts_f64, int32_t* faces, float* sdf_volumes);
/* volumes per pass of the batch calls: 1 .. 64 (default 64) */
int qsp_mesh_extractor_set_batch_limit(qsp_mesh_extractor* m, int32_t max_volumes_per_pass);
/* method 1's generated case table: ntri[256], tri[256][24] cube-edge ids (edge = 4*axis + u + 2v), -1 padded */
int qsp_mc_tables(int8_t* ntri, int8_t* tri);

/* ===============================================================================================================
 * Path B -- joint bundle adjustment (camera poses, map points, object poses)
 * ============================================================================================================ */

/* The g2o graph that Optimizer::{Local,}JointBundleAdjustment (src/Optimizer_util.cc:44-307,309-771) and
 * Optimizer::{Local,}BundleAdjustment (src/Optimizer.cc:54-242,458-783) build with heap-allocated vertices and edges,
 * flattened into arrays.  Poses are SE3Quat values laid out (tx ty tz qx qy qz qw) -- T_cw for key-frames
 * (VertexSE3Expmap, estimate = Converter::toSE3Quat(pKF->GetPose())), T_ow for objects (pMO->SE3Tow).
 * kf_id / pt_id / obj_id are the g2o VERTEX ids the reference assigns (mnId, mnId + maxKFid + 1,
 * mnId + maxKFid + maxMPid + 2): they define the order of the unknowns (hessian indices), which this library
 * reproduces exactly.  Edge arrays keep the caller's order; per-edge outputs come back in that order.
 * All arrays are copied at creation. */
typedef struct {
    int32_t n_kf, n_pt, n_obj, n_mono, n_stereo, n_objedge;
    const double* kf_pose;        /* [n_kf][7]                                                             */
    const uint8_t* kf_fixed;      /* [n_kf]  vSE3->setFixed(...)                                           */
    const int64_t* kf_id;         /* [n_kf]                                                                */
    const double* kf_K;           /* [n_kf][5]  fx fy cx cy bf (pKF->fx ... pKF->mbf)                      */
    const double* pt_xyz;         /* [n_pt][3]  VertexSBAPointXYZ, marginalised                            */
    const int64_t* pt_id;
    const double* obj_pose;       /* [n_obj][7]                                                            */
    const int64_t* obj_id;
    const int32_t* mono_pt;       /* EdgeSE3ProjectXYZ: vertex 0 = point, vertex 1 = key-frame             */
    const int32_t* mono_kf;
    const double* mono_obs;       /* [n_mono][2]  kpUn.pt                                                  */
    const double* mono_info;      /* [n_mono]     invSigma2 (information = invSigma2 * I)                  */
    const int32_t* stereo_pt;     /* EdgeStereoSE3ProjectXYZ                                               */
    const int32_t* stereo_kf;
    const double* stereo_obs;     /* [n_stereo][3]  u v u_right                                            */
    const double* stereo_info;
    const int32_t* objedge_kf;    /* EdgeSE3LieAlgebra (include/ObjectPoseGraph.h:57-89): vertex 0 = key-frame */
    const int32_t* objedge_obj;   /*                                                      vertex 1 = object   */
    const double* objedge_meas;   /* [n_objedge][7]  Z = det->SE3Tco                                        */
    double objedge_info;          /* information = objedge_info * I6 (1e3 in the reference)                 */
} qsp_ba_scene;

/* Per-iteration record of one optimize() call (G2OBatchStatistics-like, block_solver.hpp:441-453): the caller provides the
 * arrays with capacity `cap`. */
typedef struct {
    int32_t cap, n;
    double* chi2;            /* robust chi2 after the iteration                                             */
    double* lambda;          /* LM damping after the iteration                                              */
    int32_t* trials;         /* LM trials spent in the iteration (<= 10)                                    */
    int32_t* accepted;       /* 1 if the last trial was accepted                                            */
    int32_t result;          /* 0 ran all iterations, 1 terminated by the LM stop rules, 2 stop flag         */
    int32_t iterations;      /* iterations done                                                              */
    int32_t n_pose_blocks;   /* free key-frames + objects (reduced system = 6 x this)                        */
    int32_t n_landmarks;     /* active points                                                                */
} qsp_ba_trace;

typedef struct {
    float ms_total;          /* whole optimize() call on the GPU stream                                      */
    float ms_linearize;      /* sum over linearisations of the three J^T W J kernels (k_lin_*)               */
    float ms_schur, ms_solve, ms_update;
    int32_t n_linearize, n_trials;
    int64_t bytes_linearize; /* ALGORITHMIC bytes of one linearisation: 176 B/mono edge, 184 B/stereo edge,
                                392 B/free pose or object, 120 B/point, 352 B/object edge */
    int32_t cholesky_chain;  /* 1: the dense factorisation runs as one launch -- a resident chain workgroup and tile workgroups
                                beside it (QSP_BA_OPT_CHOLESKY_CHAIN), 0: one launch per block step                  */
    int32_t chain_timeouts;  /* solves of this problem in which a flag wait of that launch expired: the trial was repeated on
                                the one-launch-per-step form, which the problem keeps from there on (0 in a healthy run)  */
    int32_t boundary_device; /* qsp_ba_local_joint calls of this problem whose stage boundary (outlier classification, re-index,
                                the second stage's first system) ran on the device behind the first stage's last trial ...  */
    int32_t boundary_host;   /* ... and those that took the host path: the last trial was rejected, a key-frame or object
                                vertex lost its last active edge (the reduced system changes shape), or several ranks       */
    int32_t schur_form;      /* how the last Levenberg-Marquardt trial of the last solve built the reduced camera system: 0 key-frame
                                pair lists (no atomics), 1 per landmark (FP64 atomics), 2 block rows (LDS atomics), -1 none was
                                built (no trial ran, or no free key-frame).  Filled with profiling on or off                 */
} qsp_ba_stats;

typedef struct qsp_ba_problem qsp_ba_problem;

int qsp_ba_create(const qsp_ba_scene* scene, int device, qsp_ba_problem** out);
void qsp_ba_destroy(qsp_ba_problem* p);
/* qsp_ba_destroy keeps what is expensive to make for the next problem on the same device: the problem's streams (a hardware queue
 * costs milliseconds to bring up), up to 16 device chunks / 512 MB and its pinned staging buffers.  A caller that builds a problem
 * per bundle adjustment -- Optimizer::LocalJointBundleAdjustment, src/Optimizer_util.cc:309-771, as LocalMapping calls it --
 * pays 1.3 ms instead of 7 ms per create + destroy.  The one-shot batch calls (Sim3 optimisation and RANSAC, SearchBySim3,
 * SearchByBoW, the essential graph, the ellipsoid fits and the object gate) take their one device block from the same cache and
 * give it back when they return.  qsp_ba_release_caches() gives everything back (any thread, no problem of the process may be
 * inside a call). */
void qsp_ba_release_caches(void);

/* g2o edge levels: 1 = excluded from optimisation (e->setLevel(1), src/Optimizer_util.cc:621-654).  NULL = all active.
 * A problem is long-lived and may be driven in any order of calls.  What it holds for the caller:
 *   levels     what the last qsp_ba_set_levels or qsp_ba_local_joint left (the latter: all active, then the outlier set of its
 *              stage boundary; nothing when it returned at once on a raised stop flag);
 *   estimates  what the last solve or qsp_ba_set_state left.
 * qsp_ba_set_shard*, qsp_ba_set_deterministic and qsp_ba_set_option change how the NEXT solve is computed; they never change
 * levels or estimates, whenever they are called -- also between a qsp_ba_set_levels / qsp_ba_local_joint and the solve that
 * follows. */
int qsp_ba_set_levels(qsp_ba_problem* p, const uint8_t* mono, const uint8_t* stereo, const uint8_t* objedge);

/* optimizer.initializeOptimization(0); optimizer.optimize(n_iter) -- Levenberg-Marquardt with Schur complement over the
 * points (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-164, block_solver.hpp:354-486).
 * delta_* are the Huber deltas of RobustKernelHuber (<= 0: no kernel).  stop_flag mirrors setForceStopFlag(pbStopFlag):
 * polled before every iteration and LM trial; may be NULL.  trace may be NULL. */
int qsp_ba_optimize(qsp_ba_problem* p, int32_t n_iter, double delta_mono, double delta_stereo, double delta_obj,
                    const volatile uint8_t* stop_flag, qsp_ba_trace* trace);

/* The two-stage schedule of Optimizer::LocalJointBundleAdjustment (src/Optimizer_util.cc:598-661): optimize(5) with Huber
 * sqrt(5.991)/sqrt(7.815)/sqrt(1e3); edges with chi2 > 5.991 / 7.815 / 1e3 or non-positive depth go to level 1; kernels
 * dropped; optimize(10).  Returns early (state of stage 1 kept) when *stop_flag is set, as the reference does. */
int qsp_ba_local_joint(qsp_ba_problem* p, const volatile uint8_t* stop_flag, qsp_ba_trace* stage1, qsp_ba_trace* stage2);

int qsp_ba_set_state(qsp_ba_problem* p, const double* kf_pose, const double* pt_xyz, const double* obj_pose);
int qsp_ba_get_state(qsp_ba_problem* p, double* kf_pose, double* pt_xyz, double* obj_pose);

/* Per-edge chi2 = e^T Omega e of the LAST error evaluation (what e->chi2() returns in the reference's outlier checks,
 * which may belong to a rejected LM trial -- reproduced), and isDepthPositive() from the current estimates. */
int qsp_ba_get_edges(qsp_ba_problem* p, double* mono_chi2, double* stereo_chi2, double* objedge_chi2,
                     uint8_t* mono_depth_positive, uint8_t* stereo_depth_positive);

/* hessianIndex of every vertex as g2o's buildIndexMapping assigns it for the last optimize() call (-1: fixed or
 * inactive): free key-frames and objects in ascending vertex id, then points in ascending vertex id. */
int qsp_ba_get_index(qsp_ba_problem* p, int32_t* kf_hidx, int32_t* obj_hidx, int32_t* pt_hidx);

int qsp_ba_profile(qsp_ba_problem* p, int enable, qsp_ba_stats* out);

/* Multi-GPU: shard ONE scene's landmarks over `world` ranks (one process per GPU, every rank created from the same scene).
 * Rank r linearises and marginalises the landmarks with pt_id % world == r; the camera-object edges (a few thousand at
 * most) are linearised by every rank and counted by rank 0; the shared camera block is combined with ONE sum all-reduce of
 * the reduced system (dimp^2 + dimp doubles, dimp = 6 x free key-frames rounded up to 64) per Levenberg-Marquardt trial,
 * plus three tiny ones (pose blocks after linearisation, chi2 and rho scalars); every rank then solves the reduced system
 * redundantly and updates its own landmarks.  `fn` must sum
 * `count` doubles at `device_buf` in place over all ranks and be complete (or ordered on `hip_stream`) when it returns;
 * with torch.distributed this is all_reduce on RCCL ("nccl" backend) over xGMI -- see qsp_slam_amd/parallel.py.
 * The reference has no counterpart (single process).
 * May be called at any time between solves, again with another (rank, world), or with world == 1 to switch sharding off.  The
 * sharding is not part of the caller's levels (see qsp_ba_set_levels): the levels and estimates the problem holds stay as they
 * are, "belongs to another rank" never shows in qsp_ba_get_index (a landmark is inactive only if the CALLER's levels leave it no
 * edge), and nothing of one (rank, world) survives the change to another. */
typedef int (*qsp_allreduce_fn)(void* ctx, double* device_buf, int64_t count, void* hip_stream);
int qsp_ba_set_shard(qsp_ba_problem* p, int32_t rank, int32_t world, qsp_allreduce_fn fn, void* ctx);

/* The same sharding with the collectives issued by the library itself: ncclAllReduce(ncclDouble, ncclSum) on the
 * problem's own HIP stream, in place on the device buffers -- no host synchronisation per collective, the stream orders
 * each reduction between the kernels that write and read its buffer.  `nccl_comm` is an ncclComm_t of `world` ranks (one per
 * GPU) that the caller owns: one made by qsp_comm_create below, or the embedding application's own.  Per LM iteration: one
 * reduction of the pose blocks + b_p + chi2 (36 n_pose + dim + 1 doubles) and, in the first iteration, a 1-double MAX for
 * lambda's initial value; per LM trial: the reduced system (dimp^2 + dimp doubles) and two scalars (chi2, rho
 * denominator); per optimize() call: the landmarks (3 n_pt doubles).  Sums are re-associated across ranks, so a sharded
 * solve follows the unsharded one to ~1e-9 relative, not bit for bit.  world == 1 (comm ignored) switches sharding off. */
int qsp_ba_set_shard_rccl(qsp_ba_problem* p, int32_t rank, int32_t world, void* nccl_comm);

/* ---------------------------------------------------------------------------------------------------------------
 * RCCL communicator owned by the library (one process per GPU; xGMI inside a node).  librccl.so.1 is resolved at run time
 * -- the copy already mapped into the process (PyTorch ships one) or the ROCm installation's -- so the library has no
 * link-time dependency on it and single-GPU users never load it.
 *   qsp_comm_unique_id: ncclGetUniqueId on ONE rank; the 128 bytes travel to the other ranks by any side channel
 *                       (torch.distributed broadcast, a file, MPI).
 *   qsp_comm_create:    ncclCommInitRank on `device`; collective over all ranks.
 *   qsp_comm_adopt:     wrap an ncclComm_t the application already has (not destroyed by qsp_comm_destroy).
 *   qsp_comm_allreduce_f64 / qsp_comm_allgather_f32: in-place SUM of `count` doubles / gather of `count_per_rank` floats
 *                       per rank into recv (world x count_per_rank) on `hip_stream` (NULL: the null stream); asynchronous. */
#define QSP_COMM_ID_BYTES 128
typedef struct qsp_comm qsp_comm;
int qsp_comm_unique_id(uint8_t* id_out /* [QSP_COMM_ID_BYTES] */);
int qsp_comm_create(const uint8_t* id /* [QSP_COMM_ID_BYTES] */, int32_t rank, int32_t world, int device, qsp_comm** out);
int qsp_comm_adopt(void* nccl_comm, int32_t rank, int32_t world, int device, qsp_comm** out);
void qsp_comm_destroy(qsp_comm* c);
void* qsp_comm_nccl(qsp_comm* c);     /* the ncclComm_t, for qsp_ba_set_shard_rccl */
/* librccl is resolved at run time: QSP_RCCL_LIB=<path> if set (an explicit library wins; a path that does not load is an error),
 * else the copy already mapped into the process, else librccl.so.1.  Test hook for the shared-memory stand-in of tests/stub_rccl
 * (which lets a one-GPU box execute the RCCL-on-stream path with two ranks): collectives that ran with world > 1 on this
 * communicator, out3 = [sum all-reduces, max all-reduces, all-gathers]; QSP_ERR_UNSUPPORTED with a real RCCL. */
int qsp_comm_stub_counts(qsp_comm* c, int64_t* out3);
int32_t qsp_comm_rank(qsp_comm* c);
int32_t qsp_comm_world(qsp_comm* c);
int qsp_comm_allreduce_f64(qsp_comm* c, double* device_buf, int64_t count, void* hip_stream);
int qsp_comm_allgather_f32(qsp_comm* c, const float* send, float* recv, int64_t count_per_rank, void* hip_stream);

/* Reproducible mode: the Schur complement is accumulated without atomics, every sum in a fixed order (per pair of
 * key-frames over their common landmarks in landmark order, pair lists built on the host from sum_l k_l (k_l+1)/2 entries,
 * 144 B per edge of extra device storage), so repeated runs give the same bits.  It is the DEFAULT whenever the lists stay
 * below 4 M entries (C2, C4, C5 of BASELINE.json all do; as fast as the atomic kernels there); larger graphs fall back to
 * FP64 atomics (run-to-run spread of the final chi2 3e-15 .. 8e-9 relative).  on = 1 forces it
 * (QSP_ERR_UNSUPPORTED when the graph is too large), on = 0 selects the atomic kernels. */
int qsp_ba_set_deterministic(qsp_ba_problem* p, int on);

/* Solver options.  QSP_BA_OPT_OBJECT_ELIMINATION (default 1): the object vertices -- connected to key-frames only, so their part
 * of the reduced system is block diagonal -- are eliminated in closed form in front of the dense factorisation, which then
 * covers the free key-frames only (what the fill-reducing ordering of the reference's sparse LDLT achieves,
 * Thirdparty/g2o/g2o/solvers/linear_solver_eigen.h:147-201).  0 keeps objects inside the dense system (same solution to
 * rounding; A/B tests).  Takes effect at the next optimize() call.
 * QSP_BA_OPT_CHOLESKY_CHAIN (default 1 where the reduced system has more than one block row): the blocked Cholesky of the reduced
 * system (linear_solver_eigen.h:94-124) as ONE launch on the problem's stream: the first workgroup to start carries the serial
 * chain -- update of the next diagonal block, its factorisation, the forward substitution -- and never leaves its compute unit, the
 * others take the remaining tiles by ticket and keep each in registers through all its steps; they meet through flags in device
 * memory.  A tile waits only for the chain and for tiles with smaller tickets, which running workgroups hold, so the launch makes
 * progress however few of its workgroups are resident.  Waits are bounded all the same: if one expires (compute units withheld
 * for ~1-2 s) the trial is repeated on the one-launch-per-step form -- same operations, same order, same bits -- and the problem
 * stays on it (qsp_ba_stats.chain_timeouts counts; a line on stderr).  QSP_BA_CHOL=steps in the environment selects that form
 * outright.  Value 2 is for tests: the chain is launched WITHOUT its tile workgroups, so its first wait must expire (about a
 * second); the call must neither hang nor fail, and must give the step form's bits. */
enum { QSP_BA_OPT_OBJECT_ELIMINATION = 1, QSP_BA_OPT_CHOLESKY_CHAIN = 2 };
int qsp_ba_set_option(qsp_ba_problem* p, int32_t option, int32_t value);

/* ---------------------------------------------------------------------------------------------------------------
 * Pose-only optimisation: Optimizer::PoseOptimization(Frame*), src/Optimizer.cc:244-456 --
 * one free SE3 vertex, one unary edge per matched map point (EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose),
 * 4 rounds of optimize(10) with inlier / outlier re-classification (chi2 5.991 / 7.815), robust kernel off from round 3.
 * The whole procedure is one kernel launch.  Host pointers.
 *   K (5) fx fy cx cy bf; pose (7) tx ty tz qx qy qz qw of T_cw = Converter::toSE3Quat(pFrame->mTcw);
 *   X (n,3) world points; obs (n,3) u v u_right (third entry ignored where stereo[i] == 0); info (n) invSigma2;
 *   outlier (n) out = pFrame->mvbOutlier of the matched points; *n_inliers = nInitialCorrespondences - nBad (0 and the
 *   pose unchanged when n < 3, :368-369). */
typedef struct qsp_pose_optimizer qsp_pose_optimizer;
typedef struct {
    int32_t iters[4];          /* LM iterations run in each round                       */
    double trace[4][10][3];    /* chi2, lambda, trials after each (round, iteration)    */
} qsp_pose_trace;
int qsp_pose_optimizer_create(int device, int32_t max_points, qsp_pose_optimizer** out);
void qsp_pose_optimizer_destroy(qsp_pose_optimizer* h);
int qsp_pose_optimize(qsp_pose_optimizer* h, int32_t n, const double* K, const double* pose_in, const double* X,
                      const double* obs, const double* info, const uint8_t* stereo, double* pose_out, uint8_t* outlier,
                      int32_t* n_inliers, qsp_pose_trace* trace);

/* ---------------------------------------------------------------------------------------------------------------
 * Caller-side marshalling on the device: what LocalMapping::ProcessDetectedObjects does
 * around Optimizer.reconstruct_object for every detection of a key frame, src/LocalMapping_util.cc:585-760 --
 *   surface_points_cam = Rcw * x3Dw + tcw over the object's map points                               (:610-628)
 *   depth_obs = z of the same transform over the detection's feature points, ray = invK * (u, v, 1)  (:634-669)
 *   rays = [fg_rays ; background_rays]                                                               (:671-672)
 *   hypothesis k: t_cam_obj = SE3Tcw * Sim3Two with the rotation block of Sim3Two right-multiplied by
 *   AngleAxisf(k * flip_sample_angle, e_y); k = 0 only when the object already has a good orientation (:706-733)
 *   keep the first result, replace it when it is not good or when the new one is good with a smaller loss (:748-752)
 * -- for ALL detections in one call: world-frame inputs go up once, three small kernels assemble the resident batch and
 * the initial states, the Gauss-Newton iterations run as in qsp_refine_batch_run, one kernel applies the selection rule, and
 * only the kept pose / code / loss per detection come back.  The filters on MapPoint flags (isBad, isOutlier, object_id:
 * :612-617,640-647) are pointer chasing over the map and stay with the caller: the arrays hold the points that passed.
 * Host pointers; ragged arrays are concatenated, *_off has n_det + 1 entries.
 * Every count may be 0.  A detection without feature points (fg_off[d + 1] == fg_off[d]) is refined on its background rays alone
 * and owns no entry of depth_obs; one without map points (pts_off[d + 1] == pts_off[d]) is accepted and comes back as
 * reconstruct_object gives it for an empty point set: every hypothesis not good with loss 0 (optimizer.py:168-169), so
 * kept_flip = n_flip - 1 and is_good = 0.
 * Refusals are QSP_ERR_INVALID: n_det <= 0, a null T_cw / K / T_wo / offset array, offsets that do not start at 0 or decrease,
 * an n_flip outside 1 .. 64, an observation array that is null while its offsets count rows, a cfg->code_len that is not the
 * decoder's (and, for the group entry, a null det_class or a class outside the group).  The code refuses before any launch: no
 * output is written. */
typedef struct {
    int32_t n_det;
    const float* T_cw;         /* (n_det,4,4) row-major SE3 pose of the detection's key frame (KeyFrame::GetPose)        */
    const float* K;            /* (n_det,4) fx fy cx cy (Tracking::GetCameraIntrinsics)                                  */
    const float* T_wo;         /* (n_det,4,4) MapObject::Sim3Two                                                         */
    const float* code;         /* (n_det,code_len) MapObject::vShapeCode, or NULL for zero codes                         */
    const int32_t* n_flip;     /* (n_det) 1 if MapObject::findGoodOrientation else flip_sample_num; NULL = all 1         */
    double flip_angle;         /* flip_sample_angle = 2 pi / flip_sample_num (src/LocalMapping.cc:76)                    */
    const int32_t* pts_off;    /* map points on the object, world frame                                                  */
    const float* pts_world;    /* (pts_off[n_det],3)                                                                     */
    const int32_t* fg_off;     /* feature points of the detection that lie on the object                                 */
    const float* fg_px;        /* (fg_off[n_det],2) undistorted key-point pixel (mvKeysUn[idx].pt)                       */
    const float* fg_world;     /* (fg_off[n_det],3) world position of the matched map point                              */
    const int32_t* bg_off;     /* background rays of the detection (ObjectDetection::background_rays)                    */
    const float* bg_rays;      /* (bg_off[n_det],3)                                                                      */
} qsp_detections;

typedef struct {               /* any pointer may be NULL */
    float* t_cam_obj;          /* (n_det,4,4) Sim3Tco of the kept result (unspecified where is_good == 0)                */
    float* code;               /* (n_det,code_len)                                                                       */
    float* loss;               /* (n_det) loss of the kept result                                                        */
    uint8_t* is_good;          /* (n_det) 0: the reference's t_cam_obj would be None                                     */
    int32_t* kept_flip;        /* (n_det) index k of the kept hypothesis                                                 */
    float* losses;             /* (sum n_flip) loss of every hypothesis, detection-major (the "# Losses" line, :755-759) */
    /* parity taps: the assembled inputs as reconstruct_object would have received them */
    float* pts_cam;            /* (pts_off[n_det],3)                                                                     */
    float* rays;               /* (fg_off[n_det] + bg_off[n_det], 3), per detection foreground then background           */
    float* depth_obs;          /* (fg_off[n_det])                                                                        */
    float* t_cam_obj_init;     /* (sum n_flip,4,4)                                                                       */
} qsp_detection_results;

int qsp_refine_detections(qsp_decoder* dec, const qsp_joint_cfg* cfg, const qsp_detections* det,
                          qsp_detection_results* out);

/* ---------------------------------------------------------------------------------------------------------------
 * Decoder groups: the objects of several classes in ONE batch.  QSP-SLAM builds one optimizer per class id, all with the same
 * code length and optimiser parameters (src/LocalMapping.cc:33-69, the assumption stated at :47), and LocalMapping_util.cc
 * picks the one of each detection's class.  A group is an ordered set of existing decoders, one per class; the group entry
 * points take a class index in [0, n) per object / detection and advance the objects of all classes together, in the same
 * launches per iteration as one decoder's batch: each work item of a decoder kernel reads the parameters of its object's
 * class.  Every hypothesis's numbers are those of the same object in a batch of its own class's decoder alone (same slot
 * count, i.e. same largest point set), bit for bit.
 *   1..16 members, on one device.  Members may differ in weights, shape (any the single decoder accepts) and use_tanh; they
 *   must agree on code_len, both precisions, tile points, narrow tile, render screening (margin, audit, minimum samples, depth
 *   staging) and range fallback: QSP_ERR_UNSUPPORTED names the first option that differs.  Checked again at every group call
 *   (options may change after creation).  A class index outside [0, n): QSP_ERR_INVALID.
 *   Range fallback: when a split-fp16 pass of ANY member leaves fp16's range, the whole call is repeated on the f32 pipe for
 *   every member (qsp_refine_profile.range_fallbacks, QSP_DEC_CNT_RANGE_FALLBACKS of member 0).
 *   Threads and lifetime: see qsp_decoder_create. */
enum { QSP_GROUP_MAX = 16 };
typedef struct qsp_decoder_group qsp_decoder_group;
int qsp_decoder_group_create(qsp_decoder* const* decs, int32_t n, qsp_decoder_group** out);
void qsp_decoder_group_destroy(qsp_decoder_group* g);
/* qsp_refine_batch_create over a group: obj_class[o] = member of object o.  The batch is an ordinary qsp_refine_batch: set_state,
 * run, get, trace, trace_rot, rows and profile work on it unchanged. */
int qsp_refine_batch_create_group(qsp_decoder_group* g, const qsp_joint_cfg* cfg, int32_t n_obj,
                                  const float* const* pts, const int32_t* n_pts,
                                  const float* const* rays, const int32_t* n_rays,
                                  const float* const* depth, const int32_t* n_fg, const int32_t* obj_class,
                                  int32_t n_hyp, const int32_t* hyp_obj, qsp_refine_batch** out);
/* qsp_reconstruct_objects over a group, on a resident batch owned by the group (results do not depend on what it held before) */
int qsp_reconstruct_objects_group(qsp_decoder_group* g, const qsp_joint_cfg* cfg, int32_t n_obj,
                                  const float* const* pts, const int32_t* n_pts,
                                  const float* const* rays, const int32_t* n_rays,
                                  const float* const* depth, const int32_t* n_fg, const int32_t* obj_class,
                                  int32_t n_hyp, const int32_t* hyp_obj, const float* t_cam_obj, const float* code,
                                  float* t_cam_obj_out, float* code_out, float* loss_out, uint8_t* is_good_out);
/* qsp_estimate_pose over a group: obj_class[i] = member of item i */
int qsp_estimate_pose_group(qsp_decoder_group* g, int32_t n, const float* t_co_se3, const float* scale,
                            const float* const* pts, const int32_t* n_pts, const float* code, const int32_t* obj_class,
                            int32_t n_iter, float* t_co_out);
/* qsp_refine_detections over a group: det_class[d] = member of detection d */
int qsp_refine_detections_group(qsp_decoder_group* g, const qsp_joint_cfg* cfg, const qsp_detections* det,
                                const int32_t* det_class, qsp_detection_results* out);
/* Mesh extraction over a group (see "Mesh extraction", Batches): the meshes of the codes of all classes in one call.
 *   The group's options are checked (and its parameter copy refreshed) at every qsp_mesh_extract_batch_group, which holds the
 *   locks of all members; a class index outside [0, members) is QSP_ERR_INVALID, null pointers and n < 0 too; n == 0 is QSP_OK
 *   and touches nothing; method 1 is QSP_ERR_UNSUPPORTED as for qsp_mesh_extract_batch.
 *   Lifetime: destroy the extractor before the group, and the group before its decoders. */
/* an extractor over a decoder group: the grid is shared, every code names its class (position in the group) */
int qsp_mesh_extractor_create_group(qsp_decoder_group* g, int32_t voxels_dim, const float* voxel_points, qsp_mesh_extractor** out);
/* n codes (n x code_len) + n class indices -> n meshes; everything else as qsp_mesh_extract_batch */
int qsp_mesh_extract_batch_group(qsp_mesh_extractor* m, int32_t n, const float* codes, const int32_t* cls,
                                 int64_t* n_verts, int64_t* n_faces);

/* ---------------------------------------------------------------------------------------------------------------
 * Single-ellipsoid fits, batched: EllipsoidExtractor::OptimizeEllipsoidUsingPlanes,
 * src/pca/EllipsoidExtractorLocalOptimization.cpp:16-85 -- per ellipsoid one VertexEllipsoidXYZABC (translation and half-axes
 * free, rotation fixed) and one unary EdgeEllipsoidPlane per plane (error = distance from the plane to the nearest tangent
 * point, src/pca/EllipsoidExtractorEdges.cpp:35-175; information 1; g2o's numeric Jacobian, delta 1e-9), dense
 * Levenberg-Marquardt, optimize(n_iter) (reference: 10).  One wave per ellipsoid, all ellipsoids in one launch.
 *   ellipsoid_in/out (n,10): translation (3), quaternion x y z w (4), half-axes (3) = g2o::ellipsoid::toVector()
 *   planes (plane_off[n],4): A B C D of the planes of ellipsoid i at [plane_off[i], plane_off[i+1]); no planes: unchanged
 *   normal_direction != 0: the residual of EdgeSE3EllipsoidPlane with setNormalDirection(true) and an identity camera
 *   (GetDistanceWithDirection + its NaN -> 0 rule, EllipsoidExtractorEdges.cpp:151-226) instead of EdgeEllipsoidPlane's
 *   chi2_out (n), iters_out (n), trace (n,n_iter,3) chi2 / lambda / trials per iteration: optional.  Host pointers. */
int qsp_ellipsoid_fit_planes(int device, int32_t n, const double* ellipsoid_in, const int32_t* plane_off,
                             const double* planes, int32_t n_iter, int32_t normal_direction, double* ellipsoid_out,
                             double* chi2_out, int32_t* iters_out, double* trace);

/* The OTHER single-ellipsoid problem of the reference: priorInfer::infer, src/core/PriorInfer.cpp:331-427 -- one
 * VertexEllipsoidXYZABCYaw (7 unknowns: translation in the ellipsoid's frame, half-axes, yaw; include/core/BasicEllipsoidEdges.h:46,
 * src/core/Ellipsoid.cpp:78-106), a fixed identity camera, and per ellipsoid
 *   planes_normal [off_normal[i], off_normal[i+1]): EdgeSE3EllipsoidPlaneWithNormal (2-D: nearest tangent distance, smallest angle
 *       between the plane normal and an ellipsoid axis; information diag(1, 1 / sigma^2) w^2; Huber delta 1),
 *       src/pca/EllipsoidExtractorEdges.h:52, .cpp:297-375;
 *   planes [off_plane[i], off_plane[i+1]): EdgeSE3EllipsoidPlane with setNormalDirection(true) (1-D; information w^2; Huber);
 *   pri (n,2), weight (n): EdgePri, error = (mid / min, max / min of the |half-axes|) - pri, information weight^2, no kernel;
 *   ground_plane_weight (n) or NULL: w of the FIRST plane of each of the two lists (bUseGroundPlaneWeight), otherwise w = 1;
 * g2o's numeric Jacobians (delta 1e-9), dense Levenberg-Marquardt, optimize(n_iter) (reference: 10).  One wave per ellipsoid.
 * Outputs as qsp_ellipsoid_fit_planes (the quaternion changes here).  Host pointers. */
int qsp_ellipsoid_fit_prior(int device, int32_t n, const double* ellipsoid_in, const int32_t* off_normal, const double* planes_normal,
                            const int32_t* off_plane, const double* planes, const double* pri, const double* weight,
                            const double* ground_plane_weight, double angle_sigma_deg, int32_t n_iter, double* ellipsoid_out,
                            double* chi2_out, int32_t* iters_out, double* trace);

/* ---------------------------------------------------------------------------------------------------------------
 * Sim3 refinement of loop candidates, batched: Optimizer::OptimizeSim3, src/Optimizer.cc:1050-1245, for every candidate key
 * frame of LoopClosing::ComputeSim3 in ONE launch (one wave per candidate) -- per candidate one free Sim3 S12 (7 unknowns, or 6
 * with fix_scale), per match the edge pair
 *     e12 = obs1 - cam1(project(S12 * P2c)),   e21 = obs2 - cam2(project(S12^-1 * P1c)),   chi2 = invSigma2 |e|^2,
 * Huber with delta = (double)sqrtf(th2) on both, g2o's numeric Jacobians (central differences through the vertex's oplus, delta
 * 1e-9; with fix_scale the scale column is exactly 0), dense Levenberg-Marquardt: optimize(5); a pair leaves when either chi2
 * exceeds th2; fewer than 10 pairs left: 0 inliers and S12 as it came (the flags are still reported); otherwise
 * optimize(nBad > 0 ? 10 : 5) on the remaining pairs and the final count.
 *   match_off (n_cand + 1): candidate c owns the matches [match_off[c], match_off[c+1]); starts at 0, never decreases
 *   K1, K2 (n_cand,4) fx fy cx cy of the two key frames; sim3_in / sim3_out (n_cand,8) tx ty tz qx qy qz qw s
 *   P1c, P2c (n_match,3): the matched points in their OWN camera frames (R1w X1 + t1w, R2w X2 + t2w, as doubles);
 *   obs1, obs2 (n_match,2) undistorted key points; info1, info2 (n_match) invSigma2 of their octaves
 *   inlier (n_match) out: 1 = the pair survived every check made; n_inliers (n_cand) out; trace (n_cand) out or NULL.
 * A candidate's result has the same bits alone, in any batch and at any position.  Host pointers.  n_cand == 0 is QSP_OK and
 * touches nothing; a candidate without matches returns 0 inliers and its input.  Null pointers, n_cand < 0, offsets that do not
 * start at 0 or decrease: QSP_ERR_INVALID.  No output is written unless the call returns QSP_OK. */
typedef struct {
    int32_t iters[2];          /* LM iterations run in each of the two optimize calls         */
    double trace[2][10][3];    /* chi2, lambda, trials after each (optimize call, iteration)   */
} qsp_sim3_trace;
int qsp_sim3_optimize_batch(int device, int32_t n_cand, const int32_t* match_off, const double* K1, const double* K2,
                            const double* sim3_in, const double* P1c, const double* P2c, const double* obs1, const double* obs2,
                            const double* info1, const double* info2, double th2, int32_t fix_scale, double* sim3_out,
                            uint8_t* inlier, int32_t* n_inliers, qsp_sim3_trace* trace);

/* ---------------------------------------------------------------------------------------------------------------
 * Sim3 RANSAC of loop candidates, batched: Sim3Solver (src/Sim3Solver.cc) for every candidate key frame of
 * LoopClosing::ComputeSim3 in ONE call -- one wave per (candidate, hypothesis), then one wave per candidate.  Per hypothesis
 * ComputeSim3 (:226-337: Horn's closed form on three pairs; FP64 from the float32 inputs, the eigenvector of N by cyclic Jacobi,
 * T12 / T21 rounded to float32 once) and CheckInliers (:340-364: a match is an inlier when |p1 - cam1(T12 X2c)|^2 < maxErr1 and
 * |cam2(T21 X1c) - p2|^2 < maxErr2, strict, in float32 as the reference evaluates it; p = cam(Xc) and maxErr = 9.210 sigma2 are
 * derived on the device as the constructor does, :81-109).  The result of candidate c is its FIRST hypothesis with more than
 * min_inliers inliers, which is what iterate() returns however its calls are sliced.
 *   match_off (n_cand + 1): candidate c owns the matches [match_off[c], match_off[c+1]); starts at 0, never decreases
 *   trip_off (n_cand + 1), triples (trip_off[n_cand],3): the caller's random triples, match indices local to the candidate, three
 *       different ones each; n_its (n_cand): how many of them candidate c evaluates (mRansacMaxIts), at most 1024
 *   K1, K2 (n_cand,4) fx fy cx cy; X1c, X2c (n_match,3) the matched points in their own camera frames; sigma2_1, sigma2_2
 *       (n_match) mvLevelSigma2[octave] of the two key points
 *   first_it (n_cand) out: the 1-based iteration of the first success, 0 = none; R12 (n_cand,9) row-major, t12 (n_cand,3), s12
 *       (n_cand): mR12i, mt12i, ms12i of that hypothesis (zeros when none; s12 = 1 exactly under fix_scale); inlier (n_match):
 *       its flags (zeros when none); n_inliers (n_cand): its count
 *   hyp_inliers (trip_off[n_cand]) out or NULL: the count of every hypothesis evaluated (0 beyond n_its): the tests' tap.
 * What the reference leaves in mBest* after a run that never succeeds is not reproduced.  A triple whose points coincide gives
 * NaN and counts 0; so does every comparison against a point with z == 0.  A candidate's result has the same bits alone, in any
 * batch and at any position.  Host pointers.  n_cand == 0 is QSP_OK and touches nothing; a candidate without matches or with
 * n_its == 0 returns first_it 0.  Null pointers, n_cand < 0, offsets that do not start at 0 or decrease, n_its[c] < 0 or above
 * trip_off[c+1] - trip_off[c] or above 1024, a triple index outside the candidate, a triple with two equal indices:
 * QSP_ERR_INVALID.  No output is written unless the call returns QSP_OK. */
int qsp_sim3_ransac_batch(int device, int32_t n_cand, const int32_t* match_off, const int32_t* n_its, const int32_t* trip_off,
                          const int32_t* triples, const float* K1, const float* K2, const float* X1c, const float* X2c,
                          const float* sigma2_1, const float* sigma2_2, int32_t min_inliers, int32_t fix_scale, int32_t* first_it,
                          float* R12, float* t12, float* s12, uint8_t* inlier, int32_t* n_inliers, int32_t* hyp_inliers);

/* ---------------------------------------------------------------------------------------------------------------
 * Essential-graph optimisation: Optimizer::OptimizeEssentialGraph, src/Optimizer.cc:785-1048, from initializeOptimization() to
 * the corrected map points.  n_kf VertexSim3Expmap in hessian order (ascending key-frame id), n_edge EdgeSim3 in insertion
 * order with error log(meas * S[v0] * S[v1]^-1), identity information, no robust kernel, g2o's numeric Jacobians (central
 * differences through the vertex's oplus, delta 1e-9), g2o's Levenberg-Marquardt over a dense FP64 Cholesky of the
 * 7 n_free (fix_scale: 6 n_free, the scale rows carry nothing) unknowns, optimize(n_iter) (reference: 20), then
 * pt_out[p] = S_out[r]^-1.map(S_in[r].map(pt_in[p])), r = pt_ref[p].
 *   sim3_in / sim3_out (n_kf,8) tx ty tz qx qy qz qw s; fixed (n_kf) 1 = the vertex does not move (reference: the loop key frame)
 *   edge_v0, edge_v1 (n_edge) vertex indices (setVertex(0,.), setVertex(1,.)); meas (n_edge,8); duplicate edges all count
 *   lambda_init > 0: LM's first lambda (reference: 1e-16); <= 0: g2o's 1e-5 max |H_jj|, which is what computeLambdaInit() does
 *   when no user value is set (optimization_algorithm_levenberg.cpp:166-180) -- the same function, not an extension
 *   n_pt, pt_in / pt_out (n_pt,3), pt_ref (n_pt) vertex indices; n_pt == 0 with NULL point arrays is valid
 *   trace out or NULL: iterations run and, for the first 32, chi2, lambda, trials and whether the last trial was accepted.
 * No floating-point atomics: two calls on the same input return the same bits.  Host pointers.  n_kf == 0 is QSP_OK and touches
 * nothing; n_edge == 0 or no free vertex returns the input.  Null pointers, negative counts, indices out of range, edge_v0 ==
 * edge_v1, n_iter < 0: QSP_ERR_INVALID.  More than 10208 unknowns (or 2^30 edges, or a graph the host cannot stage): QSP_ERR_UNSUPPORTED before anything is enqueued.  No output
 * is written unless the call returns QSP_OK. */
typedef struct {
    int32_t iters;             /* LM iterations run                                                           */
    int32_t reserved;
    double trace[32][4];       /* chi2, lambda, trials, last trial accepted (0/1) after each iteration         */
} qsp_essential_trace;
int qsp_essential_graph_optimize(int device, int32_t n_kf, const double* sim3_in, const uint8_t* fixed, int32_t n_edge,
                                 const int32_t* edge_v0, const int32_t* edge_v1, const double* meas, int32_t fix_scale,
                                 int32_t n_iter, double lambda_init, int32_t n_pt, const double* pt_in, const int32_t* pt_ref,
                                 double* sim3_out, double* pt_out, qsp_essential_trace* trace);

/* A read-only window on one linearisation and one trial of qsp_essential_graph_optimize, for tests; nothing in the drop-in calls
 * it.  Same graph arguments (no points) and one lambda > 0.  It runs once what the optimise loop runs per iteration (errors,
 * numeric Jacobians, assembly, reductions) and per trial (damping, factorisation, back-substitution, update, errors at the trial
 * states, reductions) -- the same kernels, grids and buffers, through the same host code -- and copies the buffers down:
 *   E (n_edge,7), chi (n_edge)   the errors and their squared norms at sim3_in
 *   J (n_edge,2,7,7)             [edge][side][direction][error row]; the side of a fixed vertex, which the device never writes,
 *                                is reported as zeros
 *   H (dim,dim), b (dim)         dim = (fix_scale ? 6 : 7) * number of free vertices, row-major without the padding of the
 *                                factorisation's 64-wide blocks
 *   x (dim)                      the solution of (H + lambda I) x = b
 *   sim3_trial (n_kf,8)          exp(x) * sim3_in; fixed vertices are copies
 *   info (7)                     after the linearisation: chi2, max |H_jj|; after the trial: chi2 at sim3_trial, computeScale(),
 *                                the factorisation's failure flag (0 = it succeeded), as the device wrote them; then dim and nb
 *                                (the number of 64-wide blocks)
 * Refusals as for qsp_essential_graph_optimize; also QSP_ERR_INVALID for a null output, a lambda that is not positive and
 * finite, n_edge == 0 and no free vertex (nothing to show).  No output is written unless the call returns QSP_OK. */
int qsp_essential_graph_stages(int device, int32_t n_kf, const double* sim3_in, const uint8_t* fixed, int32_t n_edge,
                               const int32_t* edge_v0, const int32_t* edge_v1, const double* meas, int32_t fix_scale, double lambda,
                               double* E, double* chi, double* J, double* H, double* b, double* x, double* sim3_trial, double* info);

/* ---------------------------------------------------------------------------------------------------------------
 * The map-point gate of LocalMapping::ProcessDetectedObjects (src/LocalMapping_util.cc:490-494, 508-511), batched: per
 * object either MapObject::RemoveOutliersSimple + ComputeCuboidPCA (src/MapObject.cc:275-313, 361-475; mode QSP_GATE_PCA)
 * or MapObject::RemoveOutliersModel (src/MapObject.cc:316-358; mode QSP_GATE_MODEL).  One workgroup per object, all objects
 * of the call in one launch.  pts_world holds the world positions of each object's non-bad map points in
 * GetMapPointsOnObject() order (the isBad / null filter stays with the caller, as for qsp_detections).
 *   QSP_GATE_PCA:   erased[i] = |x_i - mean of all points| > 1 (the points RemoveOutliersSimple erases); no point at all, or
 *     none left: status QSP_GATE_BAD (the reference calls SetBadFlag), every other output of the object 0.  Over the N
 *     survivors: mean m and scatter sum (x-m)(x-m)^T, its eigenvectors v0 v1 v2 by ascending eigenvalue, R = [v1 | v0 | -v2],
 *     column 0 negated if det R < 0, columns 0 and 1 negated if R[1][1] > 0.  SIGN CONVENTION: v2 enters with its
 *     largest-magnitude component positive (the first such component on a tie); Eigen's own choice is an accident of its
 *     iteration, and the other choice flips columns 0 and 2 of R together, which the yaw-flip hypotheses of the refinement
 *     absorb.  X_o = R^-1 x; per axis the int(0.05 N)-th and int(0.95 N)-th order statistics (exactly the values std::sort
 *     puts there, ties included; float32 keys taken about R^-1 m, which leaves the order and the differences as they are):
 *     whl = x(hi) - x(lo), centre in the box = (x(hi) + x(lo)) / 2, centre_w = R centre; outlier[i] = on any axis
 *     |X_o - centre| > 1.2 dim / 2, survivors only; T_wo_pca = [0.40 l R, centre_w; 0 0 0 1], the pose ComputeCuboidPCA(true)
 *     would set -- the caller applies it or not.
 *   QSP_GATE_MODEL: 10 vertices or fewer: status QSP_GATE_SKIPPED, no flag, whl 0.  Otherwise min / max per column of the
 *     object's vertices, M = T_wo[:3,:3], whl = (max - min) cbrt(det M), x_o = M^-1 (x - T_wo[:3,3]) (what
 *     invScale * Rwo.inverse() * x - invScale * Rwo.inverse() * two evaluates), outlier[i] = x_o outside
 *     [1.2 xmin, 1.2 xmax] x [1.5 ymin, 1.5 ymax] x [1.2 zmin, 1.2 zmax] -- factors on the COORDINATES, as in the
 *     reference.  erased is 0; R, centre_w and T_wo_pca are 0.
 * Every sum is a double sum in a fixed order over the point index (no floating-point atomics), the eigenvectors are cyclic
 * Jacobi in double, the inverses cofactors in double, and every output is rounded to float32 once: an object's outputs have
 * the same bits alone, in any batch, at any position and next to objects of the other mode.  Up to QSP_GATE_LDS_POINTS
 * points an object is staged on chip; beyond, every pass reads it again from memory (same results).  Host pointers.
 * n_obj == 0 is QSP_OK and touches nothing.  Null in / out / mode / pts_off (or pts_world with points present), n_obj < 0,
 * offsets that do not start at 0 or decrease, a mode outside {0, 1}, a MODEL object while T_wo, vert_off or verts is NULL:
 * QSP_ERR_INVALID.  More than 2^20 points in one object: QSP_ERR_UNSUPPORTED, decided on the offsets before any point is
 * read.  No output is written unless the call returns QSP_OK.  Non-finite coordinates are the caller's problem: the flags
 * and boxes of an object that holds one are unspecified. */
enum { QSP_GATE_PCA = 0, QSP_GATE_MODEL = 1 };
enum { QSP_GATE_OK = 0, QSP_GATE_BAD = 1, QSP_GATE_SKIPPED = 2 };
enum { QSP_GATE_LDS_POINTS = 4096, QSP_GATE_MAX_POINTS = 1 << 20 };
typedef struct {
    int32_t n_obj;
    const int32_t* mode;      /* (n_obj) */
    const int32_t* pts_off;   /* (n_obj+1) */
    const float* pts_world;   /* (pts_off[n_obj],3) */
    const float* T_wo;        /* (n_obj,4,4) Sim3Two, row-major; read in MODEL mode only; may be NULL if no object is MODEL */
    const int32_t* vert_off;  /* (n_obj+1); may be NULL if no object is MODEL */
    const float* verts;       /* (vert_off[n_obj],3) */
} qsp_object_gate_in;
typedef struct {              /* any pointer may be NULL */
    uint8_t* erased;          /* (pts_off[n_obj]) */
    uint8_t* outlier;         /* (pts_off[n_obj]) */
    float* whl;               /* (n_obj,3) */
    float* R;                 /* (n_obj,3,3) PCA */
    float* centre_w;          /* (n_obj,3) PCA */
    float* T_wo_pca;          /* (n_obj,4,4) PCA */
    int32_t* status;          /* (n_obj) */
} qsp_object_gate_out;
int qsp_object_gates(int device, const qsp_object_gate_in* in, qsp_object_gate_out* out);

/* ---------------------------------------------------------------------------------------------------------------
 * ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1102-1326) for every loop candidate of a key frame in ONE call: the step of
 * LoopClosing::ComputeSim3 between qsp_sim3_ransac_batch and qsp_sim3_optimize_batch.  Key frame 1 (the current one) is given
 * once, key frame 2 per candidate.  One wave per (candidate, direction, source slot), then one thread per slot of key frame 1
 * for the agreement: two launches.
 * Per direction (1 -> 2 with sR21 = (1.0 / s12) R12^T -- a double factor, rounded to float32 once -- and t21 = -sR21 t12;
 * 2 -> 1 with sR12 = s12 R12 and t12) and per source slot with has_point && !pre, in the reference's float32 arithmetic (matrix
 * rows summed in double and rounded once, t added in float32; 1.0 / z and the norm in double, rounded once; u = fx * x + cx as a
 * separate multiply and add):
 *   skip when z < 0, when (u, v) is outside [min_x, max_x) x [min_y, max_y) of the TARGET frame, when dist3D < dist_min_inv or
 *   dist3D > dist_max_inv;  level = clamp(ceil(logf(dist_max / dist3D) / log_scale), 0, n_levels - 1) and radius = th *
 *   scale_factors[level] with the TARGET frame's log_scale, n_levels and scale_factors (MapPoint::PredictScale);
 *   a target key point is eligible when its own cell (round((x - min_x) * grid_w_inv), round((y - min_y) * grid_h_inv)) lies in
 *   the grid (Frame::PosInGrid: others were never filed) and in the range KeyFrame::GetFeaturesInArea visits, |kx - u| < radius
 *   && |ky - v| < radius (strict) and level - 1 <= octave <= level;  the best is the eligible key point of minimum Hamming
 *   distance to mp_desc over the 256 bits, ties to the first in the reference's traversal order (cell x, cell y, index);  it is
 *   kept when the distance is <= 100 (TH_HIGH).
 * pre2 only keeps a slot from being a SOURCE of pass 2 -> 1; as a target it is matched like any other (as in the reference).
 * match12[c][i1] = best1[i1] when best1[i1] >= 0 && best2[best1[i1]] == i1, else -1 (slots with pre1 set: -1, the caller keeps
 * what it had); n_found[c] counts them.  K is key frame 1's, used for BOTH directions, as the reference does.
 * A candidate's outputs have the same bits alone, in any batch and at any position.  Host pointers.  n_cand == 0 is QSP_OK and
 * touches nothing.  Null pointers (arrays of a frame with n == 0 may be NULL; the tap is four arrays or four NULLs), n_cand < 0,
 * n < 0 or n > 2^26, off2 that does not start at 0, decreases or does not step by kf2[c].n, a key point's octave outside
 * [0, n_levels), n_levels outside [1, 16], a grid outside 1..64 x 1..64: QSP_ERR_INVALID.  More than 2^31 - 1 slots in one
 * call: QSP_ERR_UNSUPPORTED.  No output is written unless the call returns QSP_OK. */
typedef struct {
    int32_t n;                    /* key points = map-point slots (KeyFrame::N), at most 2^26 */
    const float* kp;              /* (n,2) mvKeysUn[i].pt */
    const int32_t* octave;        /* (n) mvKeysUn[i].octave */
    const uint8_t* desc;          /* (n,32) rows of mDescriptors */
    float min_x, max_x, min_y, max_y;     /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    int32_t grid_cols, grid_rows;         /* mnGridCols, mnGridRows: at most 64 x 64 */
    float grid_w_inv, grid_h_inv;         /* mfGridElementWidthInv, mfGridElementHeightInv */
    int32_t n_levels;                     /* mnScaleLevels, at most 16 */
    float log_scale;                      /* mfLogScaleFactor */
    const float* scale_factors;   /* (n_levels) mvScaleFactors */
    float Rcw[9], tcw[3];                 /* GetRotation() row-major, GetTranslation() */
    /* the map point of each slot (GetMapPointMatches()[i]) */
    const uint8_t* has_point;     /* (n) 1 = pMP && !pMP->isBad(); the rest of a slot without one is not read */
    const float* Xw;              /* (n,3) GetWorldPos() */
    const float* dist_min_inv;    /* (n) GetMinDistanceInvariance() */
    const float* dist_max_inv;    /* (n) GetMaxDistanceInvariance() */
    const float* dist_max;        /* (n) mfMaxDistance, what PredictScale divides */
    const uint8_t* mp_desc;       /* (n,32) GetDescriptor() */
} qsp_orb_frame;
typedef struct {
    int32_t n_cand;
    const qsp_orb_frame* kf1;     /* one: shared by all candidates */
    const qsp_orb_frame* kf2;     /* (n_cand) */
    const int32_t* off2;          /* (n_cand+1): candidate c owns [off2[c], off2[c+1]) of pre2 / best2 / dist2; steps by kf2[c].n */
    const float* K;               /* (n_cand,4) fx fy cx cy of key frame 1 */
    const float* s12;             /* (n_cand) */
    const float* R12;             /* (n_cand,9) row-major */
    const float* t12;             /* (n_cand,3) */
    const float* th;              /* (n_cand) the reference passes 7.5 */
    const uint8_t* pre1;          /* (n_cand,kf1->n) vbAlreadyMatched1 */
    const uint8_t* pre2;          /* (off2[n_cand]) vbAlreadyMatched2 */
} qsp_search_sim3_in;
typedef struct {
    int32_t* match12;             /* (n_cand,kf1->n) index in key frame 2 of each newly agreed match, else -1 */
    int32_t* n_found;             /* (n_cand) */
    /* the tests' tap, all four or all NULL: vnMatch1 / vnMatch2 before the agreement step and their Hamming distances (-1 where no
     * key point was eligible; a distance above 100 is reported with best -1) */
    int32_t* best1;               /* (n_cand,kf1->n) */
    int32_t* dist1;               /* (n_cand,kf1->n) */
    int32_t* best2;               /* (off2[n_cand]) */
    int32_t* dist2;               /* (off2[n_cand]) */
} qsp_search_sim3_out;
int qsp_search_by_sim3_batch(int device, const qsp_search_sim3_in* in, qsp_search_sim3_out* out);

/* ---------------------------------------------------------------------------------------------------------------
 * ORBmatcher::SearchByBoW for every candidate in ONE call: the loop that opens LoopClosing::ComputeSim3 (key-frame overload,
 * src/ORBmatcher.cc:522-655; shared_is_source = 1: the shared frame is key frame 1, the SOURCE of every candidate) and the loop
 * of Tracking::Relocalization (frame overload, :159-288; shared_is_source = 0: every candidate key frame is the source and the
 * shared frame the TARGET; the reference's th is <= 50 there: th_inclusive = 1).  One wave per (candidate, node of the source
 * frame), then one workgroup per candidate for the orientation check: two launches.
 * A frame gives its descriptors, key-point angles, which slots are eligible (key-frame side: pMP && !pMP->isBad(); the frame of
 * the frame overload: all, eligible = NULL) and its DBoW2::FeatureVector in CSR form: node ids strictly ascending, and per node
 * the feature indices IN THE ORDER THE REFERENCE'S VECTOR HOLDS THEM (the greedy depends on it).  A feature index may appear
 * once per frame: nodes are then independent of each other, which is what lets the device take them in parallel.
 * Per node id both frames hold, the sources are walked in list order; a source that is eligible is compared with every target of
 * the node that is eligible and not yet taken by an earlier source: bestDist1 with the first-in-list target under the strict
 * `dist < bestDist1`, bestDist2 the second smallest distance (both start at 256; two equal minima give bestDist2 == bestDist1).
 * It is matched when bestDist1 < th (<= th with th_inclusive), (float)bestDist1 < nn_ratio * (float)bestDist2 in float32 and a
 * target was found at all; the target is then taken.  With check_orientation: rot = angle_src - angle_tgt, + 360.0f when below
 * 0, bin = round(rot * (1.0f / 30)) half away from zero (so only bins 0..12 ever fill and the reference's `bin == 30` wrap never
 * fires: kept); ComputeThreeMaxima (:1601-1642) as written; matches in no kept bin are set back to -1.  An angle pair whose bin
 * would leave [0, 30] (the reference asserts) is counted in no bin and culled.
 * Outputs are indexed by SOURCE slot: shared_is_source = 1: (n_cand, shared->n); 0: flat over the candidates' slots, candidate c
 * at [sum of cand[0..c).n, + cand[c].n).  A candidate's outputs have the same bits alone, in any batch and at any position.
 * Host pointers.  n_cand == 0 is QSP_OK and touches nothing.  QSP_ERR_INVALID: null required pointers (arrays of a frame with
 * n == 0 or no nodes may be NULL, node_off never), negative sizes, node_off that does not start at 0, decreases or exceeds n, node
 * ids not strictly ascending, a feature index outside its frame or listed twice in it, nn_ratio not finite, th outside [0, 256].
 * More than 2^31 - 1 slots (or n_cand * shared->n, or nodes) in one call: QSP_ERR_UNSUPPORTED.  No output is written unless the
 * call returns QSP_OK. */
typedef struct {
    int32_t n;                    /* key points (KeyFrame::N / Frame::N) */
    const uint8_t* desc;          /* (n,32) rows of mDescriptors */
    const float* angle;           /* (n) mvKeysUn[i].angle (key frame) / mvKeys[i].angle (frame) */
    const uint8_t* eligible;      /* (n) 1 = the slot takes part; NULL = every slot does */
    int32_t n_nodes;              /* mFeatVec.size() */
    const int32_t* node_id;       /* (n_nodes) strictly ascending */
    const int32_t* node_off;      /* (n_nodes+1) starts at 0 */
    const int32_t* feat;          /* (node_off[n_nodes]) feature indices of each node, in the reference's order */
} qsp_bow_frame;
typedef struct {
    int32_t n_cand;
    int32_t shared_is_source;     /* 1: loop closing (key-frame overload); 0: relocalisation (frame overload) */
    const qsp_bow_frame* shared;  /* one: shared by all candidates */
    const qsp_bow_frame* cand;    /* (n_cand) */
    int32_t th;                   /* TH_LOW: 50 */
    int32_t th_inclusive;         /* 0: bestDist1 < th (key-frame overload); 1: <= th (frame overload) */
    float nn_ratio;               /* mfNNratio */
    int32_t check_orientation;    /* mbCheckOrientation */
} qsp_search_bow_in;
typedef struct {
    int32_t* match;               /* per source slot: the target's index, else -1 */
    int32_t* n_matches;           /* (n_cand) */
    /* the tests' taps, each may be NULL */
    int32_t* match_raw;           /* like match: before the rotation cull */
    int32_t* dist;                /* like match: bestDist1 of each source accepted before the cull, else -1 */
    int32_t* hist;                /* (n_cand,30) the rotation histogram (zeros without check_orientation) */
    int32_t* ind;                 /* (n_cand,3) ind1 ind2 ind3 of ComputeThreeMaxima (-1 -1 -1 without check_orientation) */
} qsp_search_bow_out;
int qsp_search_by_bow_batch(int device, const qsp_search_bow_in* in, qsp_search_bow_out* out);

/* ---------------------------------------------------------------------------------------------------------------
 * ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-823, CheckDistEpipolarLine :140-157) for every covisible neighbour of
 * LocalMapping::CreateNewMapPoints in ONE call.  Key frame 1 (the current one, the SOURCE) is given once, key frame 2 (the
 * target) per neighbour.  One wave per (neighbour, position in key frame 1's feature list), then one workgroup per neighbour for
 * the orientation check: two launches.
 * A frame is a qsp_bow_frame -- descriptors, mvKeysUn[i].angle, the FeatureVector in CSR form with the reference's list order, and
 * eligible[i] = (GetMapPoint(i) == NULL): the reference tests for null only here, not isBad() (NULL = every slot) -- and beside it
 * mvKeysUn[i].pt, the stereo flag mvuRight[i] >= 0 and, read of the targets only, mvLevelSigma2 and mvScaleFactors gathered
 * through the key point's octave.  Per neighbour: F12 (the caller's ComputeF12) and the epipole of key frame 1 in its image.
 * Per node id both frames hold, for every source of the node that is eligible (and stereo, with only_stereo): bestDist = th,
 * bestIdx2 = -1; the node's targets are walked in list order; a target that is not eligible (or not stereo, with only_stereo) is
 * skipped; dist = Hamming distance over the 256 bits; skipped when dist > th || dist > bestDist (INCLUSIVE: th itself is
 * accepted, and an EQUAL distance later in the list replaces the earlier best); when neither side is stereo, skipped when
 * (ex - x2)^2 + (ey - y2)^2 < 100.0f * scale2 in float32; then a = x1 F00 + y1 F10 + F20 (b, c alike), num = a x2 + b y2 + c,
 * den = a a + b b, all float32 and left to right; den == 0 refuses; dsqr = num * num / den; accepted when
 * (double)dsqr < 3.84 * (double)sigma2.  A target that fails a geometric test changes nothing, so the result is the passing target
 * of smallest distance, the LAST in list order among equals.  The reference never sets its vbMatched2: two sources may take the
 * same target (kept); mfNNratio is not read.  With check_orientation the tail is qsp_search_by_bow_batch's.
 * Non-finite F12, epipole or key-point values are not refused: the IEEE compares decide as in the reference (a NaN never matches
 * and never skips).  A neighbour's outputs have the same bits alone, in any batch and at any position.
 * Host pointers.  n_cand == 0 is QSP_OK and touches nothing.  QSP_ERR_INVALID: null required pointers (arrays of a frame with
 * n == 0 or no nodes may be NULL, node_off never; sigma2 and scale of kf1 are not read), negative sizes, what qsp_search_by_bow_batch
 * refuses of a feature vector, th outside [0, 256].  More than 2^31 - 1 slots (or n_cand * kf1->bow.n, or nodes, or n_cand * the
 * length of kf1's feature list) in one call: QSP_ERR_UNSUPPORTED.  No output is written unless the call returns QSP_OK. */
typedef struct {
    qsp_bow_frame bow;            /* desc, angle, eligible = no map point in the slot, the FeatureVector */
    const float* xy;              /* (n,2) mvKeysUn[i].pt */
    const uint8_t* stereo;        /* (n) mvuRight[i] >= 0 */
    const float* sigma2;          /* (n) mvLevelSigma2[mvKeysUn[i].octave]; targets only */
    const float* scale;           /* (n) mvScaleFactors[mvKeysUn[i].octave]; targets only */
} qsp_tri_frame;
typedef struct {
    int32_t n_cand;
    const qsp_tri_frame* kf1;     /* one: the source of every neighbour */
    const qsp_tri_frame* kf2;     /* (n_cand) */
    const float* F12;             /* (n_cand,9) row-major */
    const float* exy;             /* (n_cand,2) the epipole ex ey (:664-670) */
    int32_t th;                   /* TH_LOW: 50 */
    int32_t only_stereo;          /* bOnlyStereo */
    int32_t check_orientation;    /* mbCheckOrientation */
} qsp_search_tri_in;
typedef struct {
    int32_t* match;               /* (n_cand,kf1->bow.n) the target's index, else -1 */
    int32_t* n_matches;           /* (n_cand) */
    /* the tests' taps, each may be NULL: as in qsp_search_bow_out */
    int32_t* match_raw;           /* (n_cand,kf1->bow.n) before the rotation cull */
    int32_t* dist;                /* (n_cand,kf1->bow.n) bestDist of each source matched before the cull, else -1 */
    int32_t* hist;                /* (n_cand,30) */
    int32_t* ind;                 /* (n_cand,3) */
} qsp_search_tri_out;
int qsp_search_for_triangulation_batch(int device, const qsp_search_tri_in* in, qsp_search_tri_out* out);

/* ---------------------------------------------------------------------------------------------------------------
 * The MATCH PHASE of ORBmatcher::Fuse for every target key frame in ONE call: the pose overload (src/ORBmatcher.cc:825-975) that
 * LocalMapping::SearchInNeighbors runs per neighbour and once back into the current key frame, and the Sim3 overload (:977-1100)
 * that LoopClosing::SearchAndFuse runs per corrected key frame.  Everything up to (bestIdx, bestDist) reads only the point and
 * the target frame; the map enters afterwards, in the action (GetMapPoint(bestIdx), Replace, AddObservation / AddMapPoint,
 * vpReplacePoint[iMP] = ...), which the caller replays on the host in the reference's order (OrbMatcherHip::FuseBatch).  One wave
 * per (target, listed point): one launch.
 * A target is a qsp_orb_frame, of which kp, octave, desc, the bounds and grid, n_levels, log_scale, scale_factors, Rcw and tcw are
 * read (the map-point fields are not and may be NULL), and beside it K (fx fy cx cy mbf), the camera centre Ow, th, mvuRight,
 * mvInvLevelSigma2 and check_reprojection: 1 = the pose overload with its chi-square test (:914-938), 0 = the Sim3 overload, which
 * has none (for it Rcw = sRcw / scw, tcw = t / scw and Ow = -Rcw^T tcw are the caller's, :986-990).  The map points are ONE pool
 * shared by all targets; target k searches the pool indices list_idx[list_off[k] .. list_off[k+1]), in that order: the points the
 * reference would not skip at :846-850 / :1005.  Outputs are per listed pair, in list order.
 * Per pair, in the reference's float32 arithmetic (matrix rows summed in double and rounded once, t added in float32; 1 / z
 * rounded to float32 once; u = fx * x + cx as a separate multiply and add; ur = u - mbf * invz; PO = Xw - Ow in float32, cv::norm(PO)
 * summed and square-rooted in double and rounded once, PO.dot(Pn) summed in double):
 *   skip when z < 0, when (u, v) is outside [min_x, max_x) x [min_y, max_y), when dist3D < dist_min_inv or dist3D > dist_max_inv,
 *   when PO.dot(Pn) < 0.5 * dist3D (in double);  level = clamp(ceil(logf(dist_max / dist3D) / log_scale), 0, n_levels - 1) and
 *   radius = th * scale_factors[level];  a key point is eligible when its own cell (round((x - min_x) * grid_w_inv),
 *   round((y - min_y) * grid_h_inv)) lies in the grid and in the range KeyFrame::GetFeaturesInArea visits, |kx - u| < radius &&
 *   |ky - v| < radius (strict), level - 1 <= octave <= level and, with check_reprojection, e2 * inv_level_sigma2[octave] (a
 *   float32 product; e2 = ex*ex + ey*ey (+ er*er) in float32, left to right) is not > 7.8 in double when u_right >= 0 (zero
 *   included), else not > 5.99;  the best is the eligible key point of minimum Hamming distance over the 256 bits, ties to the
 *   first in the reference's traversal order (cell x, cell y, index);  it is kept when the distance is <= 50 (TH_LOW).
 * The overloads' initial bestDist (256 and INT_MAX) cannot differ under that threshold.
 * reason names the first gate that ended the pair: 0 matched, 1 z < 0, 2 outside the image, 3 distance limits, 4 viewing angle,
 * 5 no cell range or no key point in the area (vIndices empty), 6 none of the area's key points eligible, 7 best above TH_LOW
 * (best_idx -1, best_dist the distance); level is the predicted level, -1 where a gate before it ended the pair.
 * A pair's outputs have the same bits alone, in any batch and at any list position.  Host pointers.  n_target == 0 or an empty
 * list is QSP_OK and touches nothing; a target with an empty list or without key points is legal.  Null pointers where data is
 * required (arrays of a target with n == 0 may be NULL; the tap is two arrays or two NULLs), negative counts, n > 2^26, list_off
 * that does not start at 0 or decreases, list_idx outside [0, n_point), a key point's octave outside [0, n_levels), n_levels
 * outside [1, 16], a grid outside 1..64 x 1..64, u_right_off that does not start at 0 or step by target[k].n: QSP_ERR_INVALID.
 * More than 2^31 - 1 pairs (or key-point slots) in one call: QSP_ERR_UNSUPPORTED.  No output is written unless the call returns
 * QSP_OK. */
typedef struct {
    int32_t n_target;
    const qsp_orb_frame* target;          /* (n_target) */
    const float* K;                       /* (n_target,5) fx fy cx cy mbf */
    const float* Ow;                      /* (n_target,3) GetCameraCenter() / -Rcw^T tcw */
    const float* th;                      /* (n_target) the reference passes 3.0 (SearchInNeighbors) and 4 (SearchAndFuse) */
    const int32_t* u_right_off;           /* (n_target+1): target k owns [u_right_off[k], u_right_off[k+1]) of u_right; steps by target[k].n */
    const float* u_right;                 /* (u_right_off[n_target]) mvuRight */
    const float* inv_level_sigma2;        /* (n_target,16) mvInvLevelSigma2, the first n_levels read */
    const uint8_t* check_reprojection;    /* (n_target) 1 = pose overload, 0 = Sim3 overload */
    int32_t n_point;                      /* the pool */
    const float* Xw;                      /* (n_point,3) GetWorldPos() */
    const float* normal;                  /* (n_point,3) GetNormal() */
    const float* dist_min_inv;            /* (n_point) GetMinDistanceInvariance() */
    const float* dist_max_inv;            /* (n_point) GetMaxDistanceInvariance() */
    const float* dist_max;                /* (n_point) mfMaxDistance, what PredictScale divides */
    const uint8_t* desc;                  /* (n_point,32) GetDescriptor() */
    const int64_t* list_off;              /* (n_target+1) starts at 0 */
    const int32_t* list_idx;              /* (list_off[n_target]) pool indices */
} qsp_fuse_in;
typedef struct {
    int32_t* best_idx;                    /* (list_off[n_target]) the target's key point, else -1 */
    int32_t* best_dist;                   /* (list_off[n_target]) its Hamming distance; -1 where no key point was eligible */
    /* the tests' tap, both or both NULL */
    int32_t* reason;                      /* (list_off[n_target]) */
    int32_t* level;                       /* (list_off[n_target]) */
} qsp_fuse_out;
int qsp_fuse_batch(int device, const qsp_fuse_in* in, qsp_fuse_out* out);

/* ---------------------------------------------------------------------------------------------------------------
 * The numeric part of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:467-607, KeyFrame::UnprojectStereo src/KeyFrame.cc:
 * 616-632) for every covisible neighbour in ONE call: qsp_triangulate_batch on a match grid the caller holds, and
 * qsp_create_new_map_points_batch, which runs qsp_search_for_triangulation_batch's two launches and then the two of the
 * triangulation in one staging block (one upload, one download; the match grid stays on the device in between).
 * match is qsp_search_tri_out.match: (n_cand, kf1->n) int32, per slot of key frame 1 the neighbour's index idx2 or -1.  A frame
 * is a qsp_triangulate_frame: GetRotation, GetTranslation, GetCameraCenter, fx fy cx cy invfx invfy mb mbf and per slot
 * mvKeysUn[i].pt, mvKeys[i].pt (the DISTORTED point: what UnprojectStereo reads), mvuRight, mvDepth and mvLevelSigma2 /
 * mvScaleFactors gathered through mvKeysUn[i].octave.  ratio_factor is 1.5f * mfScaleFactor of key frame 1.
 * Per slot (k, idx1) with idx2 >= 0, one lane, in the reference's arithmetic -- float32 one IEEE operation at a time; a CV_32F
 * matrix product row (Rwc * xn, Rwc * x3Dc) summed in double and rounded once, the camera centre then added in float32 (the
 * project's convention for cv::Mat products; whether OpenCV folds UnprojectStereo's product and sum into one rounding is not
 * verified: INTEGRATION.md lists it under the deviations); Mat::dot
 * and cv::norm in double, so z = (float)(Rcw.row(2).dot(x3D) + (double)tcw[2]) (x, y alike) and cosParallaxRays =
 * (float)(dot / (norm1 * norm2)); invz = (float)(1.0 / z); u = fx * x * invz + cx left to right; a float32 quotient correctly
 * rounded; compares against 5.991 * sigma2, 7.8 * sigma2 and 0.9998 in double; cos(2 * atan2(mb / 2, depth)) with each function
 * evaluated in double and rounded to float32 (within one ulp of a float libm):
 *   stereo1 = mvuRight1 >= 0, stereo2 alike; cosParallaxStereo1 is formed when stereo1, cosParallaxStereo2 only when !stereo1 &&
 *   stereo2 (the reference's `else if`), either is cosParallaxRays + 1 otherwise;
 *   path 1 (SVD) when cosRays < min(stereo cosines) && cosRays > 0 && (stereo1 || stereo2 || cosRays < 0.9998): A (4x4) is formed
 *   in float32 (xn[0] * Tcw.row(2) - Tcw.row(0), ...: one multiply and one subtract per entry); the right singular vector v of its
 *   smallest singular value is computed in FP64 by a one-sided Jacobi iteration (at most 30 sweeps, ended by a sweep without a
 *   rotation); refused when (float)v[3] == 0, else x3D[i] = (float)(v[i] / v[3]).  OpenCV's float32 SVD is NOT restated bit for
 *   bit: the FP64 null vector of the same float32 A lies inside the reference's own rounding noise;
 *   path 2 when stereo1 && cos1 < cos2: x3D = KeyFrame 1's UnprojectStereo(idx1); path 3 when stereo2 && cos2 < cos1: key frame
 *   2's; mvDepth <= 0 there refuses the pair (reason 10: the reference would go on with an empty Mat); else path 0, reason 2;
 *   then z1 <= 0, z2 <= 0, the reprojection error in key frame 1 (mono: ex*ex + ey*ey > 5.991 * sigma2; stereo: + er*er > 7.8 *
 *   sigma2 with u_r = u - mbf * invz) and in key frame 2, where u_r subtracts KEY FRAME 1's mbf (:582, kept), dist1 == 0 ||
 *   dist2 == 0, and ratioDist * ratio_factor < ratioOctave || ratioDist > ratioOctave * ratio_factor.
 * accept[k][idx1] = the pair passes every gate.  first[k][idx1] = it passes and no neighbour k' < k has an accepted pair at idx1:
 * the points the reference creates (an earlier neighbour's point fills the slot, which then no longer matches).  x3D is the
 * point wherever one was formed, zeros elsewhere; n_new[k] counts first[k].  reason: 0 accepted, 1 no match, 2 low parallax and no
 * usable stereo, 3 w == 0, 4 z1 <= 0, 5 z2 <= 0, 6 reprojection in key frame 1, 7 in key frame 2, 8 a zero distance, 9 scale
 * ratio, 10 UnprojectStereo on mvDepth <= 0.  path: 0 none, 1 SVD, 2 / 3 UnprojectStereo of key frame 1 / 2.  cos_rays for every
 * matched slot; z (z1, z2), err2 (both sums) and ratio_dist hold each value once the pair reached it, else 0.
 * Non-finite values are not refused: the IEEE compares decide.  A slot's outputs have the same bits alone, in any batch and at
 * any position; `first` and n_new are defined over the batch.  Host pointers.  n_cand == 0 is QSP_OK and touches nothing.
 * QSP_ERR_INVALID: null required pointers (arrays of a frame with n == 0 may be NULL; every tap may be NULL), negative sizes, a
 * match index outside [-1, kf2[k].n); for the chained call also what qsp_search_for_triangulation_batch refuses and a frame whose
 * key-point count differs between the two inputs.  More than 2^31 - 1 slots (n_cand * kf1->n, or key points) in one call:
 * QSP_ERR_UNSUPPORTED.  No output is written unless the call returns QSP_OK. */
typedef struct {
    int32_t n;                    /* key points */
    float Rcw[9], tcw[3], Ow[3];  /* GetRotation (row-major), GetTranslation, GetCameraCenter */
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
    const float* xy_un;           /* (n,2) mvKeysUn[i].pt */
    const float* xy;              /* (n,2) mvKeys[i].pt */
    const float* u_right;         /* (n) mvuRight */
    const float* depth;           /* (n) mvDepth */
    const float* sigma2;          /* (n) mvLevelSigma2[mvKeysUn[i].octave] */
    const float* scale;           /* (n) mvScaleFactors[mvKeysUn[i].octave] */
} qsp_triangulate_frame;
typedef struct {
    int32_t n_cand;
    const qsp_triangulate_frame* kf1;     /* one */
    const qsp_triangulate_frame* kf2;     /* (n_cand) */
    float ratio_factor;                   /* 1.5f * kf1's mfScaleFactor */
} qsp_triangulate_geom;
typedef struct {
    uint8_t* accept;              /* (n_cand,kf1->n) */
    uint8_t* first;               /* (n_cand,kf1->n) */
    float* x3D;                   /* (n_cand,kf1->n,3) */
    int32_t* n_new;               /* (n_cand) */
    /* the tests' taps, each may be NULL */
    int32_t* reason;              /* (n_cand,kf1->n) */
    int32_t* path;                /* (n_cand,kf1->n) */
    float* cos_rays;              /* (n_cand,kf1->n) */
    float* z;                     /* (n_cand,kf1->n,2) */
    float* err2;                  /* (n_cand,kf1->n,2) */
    float* ratio_dist;            /* (n_cand,kf1->n) */
} qsp_triangulate_out;
int qsp_triangulate_batch(int device, const qsp_triangulate_geom* geom, const int32_t* match, qsp_triangulate_out* out);
int qsp_create_new_map_points_batch(int device, const qsp_search_tri_in* in, const qsp_triangulate_geom* geom, qsp_search_tri_out* search_out,
                                    qsp_triangulate_out* out);

/* ---------------------------------------------------------------------------------------------------------------
 * The tracking thread's projection searches, with the result of the reference's SERIAL loop:
 *   mode 0, LOCAL: Frame::isInFrustum (src/Frame.cc:306-362) and ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&,
 *                  th) (src/ORBmatcher.cc:45-129), what Tracking::SearchLocalPoints runs;
 *   mode 1, LAST:  ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th, bMono) (:1328-1470), what
 *                  Tracking::TrackWithMotionModel runs.
 * Sources are numbered in the reference's loop order.  Source i sees key-point slot idx as taken when slot_blocked[idx] (the slot
 * held a point with Observations() > 0 before the call) or when an earlier source j < i with src_blocks[j] chose idx -- nothing
 * else crosses between sources, so the loop is the unique fixed point of choice[i] = match(i; blocked = initial U {choice[j] : j <
 * i, src_blocks[j]}).  It is iterated in parallel rounds (round 1 with the initial blocks only; round r with claim[idx] = the
 * smallest blocking j that chose idx in round r - 1, an integer minimum) until a round repeats the choices of the one before:
 * after round r the sources 0 .. r - 1 hold their serial values, so at most n_src + 1 rounds are needed; n_rounds reports them.
 * The current frame is a qsp_orb_frame of which kp, octave, desc, the bounds and grid, n_levels, log_scale, scale_factors, Rcw and
 * tcw are read (the map-point fields are not and may be NULL).
 * Arithmetic, the reference's float32 one operation at a time: matrix rows summed in double and rounded once, t added in float32;
 * PO = Xw - Ow in float32, cv::norm(PO) and PO.dot(Pn) in double; compares against double literals in double.
 * LOCAL, per source with src_valid (the caller folds isBad() and "already matched in this frame" into it):
 *   Pc = Rcw Xw + tcw; refuse PcZ < 0; invz = 1.0f / PcZ, u = fx * PcX * invz + cx (left to right), v likewise; refuse u < min_x ||
 *   u > max_x, v likewise (closed at both ends); dist = (float)norm(PO), refuse dist < dist_min_inv || dist > dist_max_inv; viewCos =
 *   (float)(PO.dot(Pn) / dist), refuse viewCos < view_cos_limit; level = clamp(ceil(logf(dist_max / dist) / log_scale), 0, n_levels -
 *   1); proj_xr = u - mbf * invz.  These six are outputs (in_view = 0 and the rest 0 for a refused or invalid source).
 *   r = viewCos > 0.998 ? 2.5f : 4.0f, times th only when th != 1.0; radius = r * scale_factors[level]; the area is
 *   Frame::GetFeaturesInArea(u, v, radius, level - 1, level): a key point is in it when its own cell (round((x - min_x) *
 *   grid_w_inv), round((y - min_y) * grid_h_inv)) lies in the grid and in the visited range, level - 1 <= octave <= level and |kx -
 *   u| < radius && |ky - v| < radius (strict).  Of the area, blocked slots are skipped, and slots with u_right > 0 and |proj_xr -
 *   u_right| > radius.  Best and second best are the two smallest (Hamming distance, traversal position (cell x, cell y, index))
 *   of what remains, below 256.  The source is kept when dist <= 100 and not (level_best == level2 && (float)dist > nn_ratio *
 *   (float)dist2).
 * LAST, per source with src_valid (a point, and not mvbOutlier):
 *   x3Dc = Rcw Xw + tcw; invzc = (float)(1.0 / z), refuse invzc < 0; u = fx * xc * invzc + cx; the same closed image test; radius =
 *   th * scale_factors[src_octave]; with tlc = last_Rcw * (-Rcw^T tcw) + last_tcw: forward (tlc.z > mb && !mono) takes octave >=
 *   src_octave, backward (-tlc.z > mb && !mono) octave <= src_octave, otherwise src_octave - 1 <= octave <= src_octave + 1; blocked
 *   slots are skipped, and slots with u_right > 0 and |(u - mbf * invzc) - u_right| > radius.  Best only, kept when <= 100.  With
 *   check_orientation: rot = src_angle - kp_angle[best], + 360 when negative, bin = round(rot * (1.0f / 30)), 30 becomes 0; the
 *   30-bin histogram, ComputeThreeMaxima and the nulling of :1447-1467 follow.
 * Where the reference would run into undefined behaviour or an assert the library does not follow it: a source whose u or v is
 * NaN (it passes every reference compare and reaches (int)floor(NaN); z == +0 with xc == 0 is one way there), whose dist, viewCos
 * or predicted level is NaN (dist == 0 among them), or whose radius is NaN ends with reason 6 and matches nothing; an infinite u
 * or v is outside the image like any other; a Hamming distance of 256 never beats the reference's initial 256; a bin outside [0,
 * 30) (a NaN or out-of-range angle) is reported as -1 and counted in no bin, so the match stays.
 * reason: 0 matched, 1 !src_valid, 2 behind the camera, 3 outside the image, 4 distance limits, 5 viewing angle, 6 not finite, 7 no
 * cell range or no key point in the area, 8 every key point of the area skipped, 9 best above 100, 10 refused by the ratio test.
 * The action phase is index work on the host: the sources in order write slot_src[choice[i]] = i (the last writer stays) and are
 * counted; with the orientation check every source of a bin outside the three maxima sets ITS slot to -2 -- also where a later
 * source had over-written it, as the reference does -- and is subtracted.
 * No floating-point atomics: a call's outputs have the same bits on every run.  Host pointers.  n_src == 0 is QSP_OK and touches
 * nothing.  QSP_ERR_INVALID: null required pointers (arrays of a frame with n == 0 may be NULL; the arrays of the other mode and
 * the taps may be NULL), negative counts, n > 2^26 or n_src > 2^26, n_levels outside [1, 16], a grid outside 1..64 x 1..64, a key point's octave or
 * (LAST) a valid source's src_octave outside [0, n_levels), an unknown mode.  QSP_ERR_DEVICE with "internal error" in the
 * text: the rounds did not settle within n_src + 1 (impossible by the argument above: a bug).  No output is written unless the call
 * returns QSP_OK. */
typedef struct {
    int32_t mode;                         /* 0 LOCAL, 1 LAST */
    const qsp_orb_frame* frame;           /* the current frame */
    float K[5];                           /* fx fy cx cy mbf */
    float Ow[3];                          /* mOw (LOCAL) */
    float mb;                             /* (LAST) */
    const float* u_right;                 /* (n) mvuRight */
    const uint8_t* slot_blocked;          /* (n) 1 = mvpMapPoints[idx] && mvpMapPoints[idx]->Observations() > 0 at entry */
    const float* kp_angle;                /* (n) mvKeysUn[idx].angle; LAST with check_orientation */
    float th, nn_ratio, view_cos_limit;   /* nn_ratio and view_cos_limit: LOCAL */
    int32_t check_orientation, mono;      /* LAST */
    float last_Rcw[9], last_tcw[3];       /* LAST: the last frame's pose */
    int32_t n_src;
    const uint8_t* src_valid;             /* (n_src) */
    const uint8_t* src_blocks;            /* (n_src) 1 = the source's point has Observations() > 0 */
    const float* Xw;                      /* (n_src,3) GetWorldPos() */
    const uint8_t* desc;                  /* (n_src,32) GetDescriptor() */
    const float* normal;                  /* (n_src,3) GetNormal(); LOCAL */
    const float* dist_min_inv;            /* (n_src) LOCAL */
    const float* dist_max_inv;            /* (n_src) LOCAL */
    const float* dist_max;                /* (n_src) mfMaxDistance; LOCAL */
    const int32_t* src_octave;            /* (n_src) LastFrame.mvKeys[i].octave; LAST */
    const float* src_angle;               /* (n_src) LastFrame.mvKeysUn[i].angle; LAST with check_orientation */
} qsp_search_proj_in;
typedef struct {
    int32_t* choice;                      /* (n_src) the slot the source's point was written to, else -1 */
    int32_t* dist;                        /* (n_src) the best distance, -1 where nothing was compared */
    int32_t* slot_src;                    /* (n) the source whose point the slot holds at the end, -1 untouched, -2 nulled */
    /* LOCAL: Frame::isInFrustum */
    uint8_t* in_view;                     /* (n_src) mbTrackInView */
    float *proj_x, *proj_y, *proj_xr;     /* (n_src) mTrackProjX, mTrackProjY, mTrackProjXR */
    int32_t* level;                       /* (n_src) mnTrackScaleLevel */
    float* view_cos;                      /* (n_src) mTrackViewCos */
    /* the tests' taps, each may be NULL */
    int32_t* reason;                      /* (n_src) */
    int32_t *dist2, *level_best, *level2; /* (n_src) LOCAL: -1 where there is none */
    int32_t* bin;                         /* (n_src) LAST with check_orientation: the histogram bin of a matched source, else -1 */
    int32_t n_matches;                    /* as the reference counts: over-written writes included, histogram removals subtracted */
    int32_t hist[30], ind[3];             /* LAST with check_orientation; else 0 and -1 */
    int32_t n_rounds;
} qsp_search_proj_out;
int qsp_search_by_projection(int device, const qsp_search_proj_in* in, qsp_search_proj_out* out);

/* ---------------------------------------------------------------------------------------------------------------
 * The two projection searches against a list of map points that fill slots of ONE frame, with the result of the reference's
 * SERIAL loop:
 *   mode 0, RELOC: ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th,
 *                  ORBdist) (src/ORBmatcher.cc:1472-1599), what Tracking::Relocalization runs between two PoseOptimization calls;
 *   mode 1, SIM3:  ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints,
 *                  vector<MapPoint*>& vpMatched, th) (:290-403), what LoopClosing::ComputeSim3 runs on the accepted candidate.
 * Sources are numbered in the reference's loop order (RELOC: the slots of pKF->GetMapPointMatches(); SIM3: vpPoints, the same
 * point listed twice being two sources).  Source i sees slot idx as taken when slot_blocked[idx] (the slot was non-null at entry,
 * whatever its point's observations) or when ANY earlier source chose idx: both loops test the slot for non-null and every
 * matched source writes its point there.  So this is the fixed point of qsp_search_by_projection with every source blocking,
 * iterated in the same rounds; and since a later source never chooses a slot an earlier one holds, all choices >= 0 are distinct:
 * no slot is over-written, and n_matches is their number less the histogram removals.
 * `frame` is the frame searched: kp, octave, desc, the bounds and grid, n_levels, log_scale, scale_factors, Rcw and tcw are read
 * (the map-point fields are not and may be NULL).  RELOC: the current frame.  SIM3: pKF, with Rcw = sRcw / scw and tcw = Scw.t /
 * scw, scw = sqrt(row0 . row0), and Ow = -Rcw^T tcw, decomposed by the caller with the reference's cv::Mat operations.
 * Arithmetic, the reference's float32 one operation at a time: matrix rows summed in double and rounded once, t added in float32;
 * PO = Xw - Ow in float32, cv::norm(PO) and PO.dot(Pn) in double; compares against double literals in double; the level is
 * clamp(ceil(logf(dist_max / dist) / log_scale), 0, n_levels - 1) (MapPoint::PredictScale) as in LOCAL.
 * RELOC, per source with src_valid (the caller folds null, isBad() and membership of sAlreadyFound into it):
 *   x3Dc = Rcw Xw + tcw; invzc = (float)(1.0 / z) and NO test of its sign: a point behind the camera that projects inside the image
 *   is searched and can match; u = fx * xc * invzc + cx (left to right), v likewise; refuse u < min_x || u > max_x, v likewise
 *   (closed at both ends); dist3D = (float)norm(Xw - Ow), refuse dist3D < dist_min_inv || dist3D > dist_max_inv; no viewing-angle
 *   test; radius = th * scale_factors[level]; the area is Frame::GetFeaturesInArea(u, v, radius, level - 1, level + 1): a key point
 *   is in it when its own cell (round((x - min_x) * grid_w_inv), round((y - min_y) * grid_h_inv)) lies in the grid and in the
 *   visited range, level - 1 <= octave <= level + 1 and |kx - u| < radius && |ky - v| < radius (strict).  Taken slots are skipped.
 *   The best is the smallest (Hamming distance, cell x, cell y, index) below 256, kept when dist <= orb_dist.  With
 *   check_orientation: rot = src_angle - kp_angle[best], + 360 when negative, bin = round(rot * (1.0f / 30)), 30 becomes 0; the
 *   30-bin histogram, ComputeThreeMaxima and the nulling of :1577-1596 follow (slot_src = -2, n_matches reduced).
 * SIM3, per source with src_valid (!isBad() and not in spAlreadyFound, the non-null entries of vpMatched at entry):
 *   p3Dc = Rcw Xw + tcw; refuse z < 0.0 (-0.0 passes); invz = 1 / z in float32, x = p3Dc.x * invz, u = fx * x + cx -- another order
 *   of operations than RELOC's --, v likewise; KeyFrame::IsInImage is half-open: refuse unless u >= min_x && u < max_x && v >= min_y
 *   && v < max_y (a NaN u or v fails it and is refused here, as in the reference); dist = (float)norm(Xw - Ow), the same limits;
 *   refuse PO.dot(Pn) < 0.5 * dist, compared in double; radius = th * scale_factors[level]; the area is
 *   KeyFrame::GetFeaturesInArea(u, v, radius), which has no level filter; of the area, taken slots are skipped, then key points
 *   with octave < level - 1 || octave > level (these were in the area: when nothing else remains the reason is 8, not 7).  The best
 *   is the smallest key, kept when dist <= 50 (TH_LOW); orb_dist must say 50.  No orientation check.
 * No right-image test and no ratio test in either.  th is a float; SIM3's caller passes its int converted, as the reference's
 * th * mvScaleFactors[level] converts it.
 * Where the reference would run into undefined behaviour the library follows LOCAL / LAST: a RELOC source whose u or v is NaN (z ==
 * +0 with xc == 0), a source whose dist or predicted level is NaN, or whose radius is NaN, ends with reason 6 and matches nothing; an
 * infinite u or v is outside the image like any other; a Hamming distance of 256 never beats the initial 256; a bin outside [0, 30)
 * is reported as -1 and counted in no bin, so the match stays.
 * reason: as qsp_search_by_projection's (2 only in SIM3, 5 only in SIM3, 10 never).  level, proj_x, proj_y: the predicted level and
 * (u, v) of a source that passed every gate (reasons 0, 7, 8, 9), else 0.  slot_src: the source whose point the slot holds at the
 * end, -1 untouched (slots taken at entry among them), -2 nulled by the histogram (RELOC only).
 * No floating-point atomics: a call's outputs have the same bits on every run.  Host pointers.  n_src == 0 is QSP_OK and touches
 * nothing.  QSP_ERR_INVALID: null required pointers (arrays of a frame with n == 0 may be NULL; normal is required in SIM3,
 * kp_angle and src_angle in RELOC with check_orientation; the taps may be NULL), negative counts, n > 2^26 or n_src > 2^26, n_levels
 * outside [1, 16], a grid outside 1..64 x 1..64, a key point's octave outside [0, n_levels), an unknown mode, SIM3 with orb_dist !=
 * 50 or check_orientation != 0.  QSP_ERR_DEVICE with "internal error" in the text: the rounds did not settle within n_src + 1, or a
 * taken slot was chosen (both impossible by the argument above: a bug).  No output is written unless the call returns QSP_OK. */
typedef struct {
    int32_t mode;                         /* 0 RELOC, 1 SIM3 */
    const qsp_orb_frame* frame;           /* RELOC: the current frame; SIM3: pKF with the decomposed Scw as its pose */
    float K[4];                           /* fx fy cx cy */
    float Ow[3];                          /* -Rcw^T tcw */
    const uint8_t* slot_blocked;          /* (n) 1 = the slot is non-null at entry */
    const float* kp_angle;                /* (n) mvKeysUn[idx].angle; RELOC with check_orientation */
    float th;
    int32_t orb_dist;                     /* RELOC: ORBdist; SIM3: 50 */
    int32_t check_orientation;            /* RELOC */
    int32_t n_src;
    const uint8_t* src_valid;             /* (n_src) */
    const float* Xw;                      /* (n_src,3) GetWorldPos() */
    const uint8_t* desc;                  /* (n_src,32) GetDescriptor() */
    const float* dist_min_inv;            /* (n_src) GetMinDistanceInvariance() */
    const float* dist_max_inv;            /* (n_src) GetMaxDistanceInvariance() */
    const float* dist_max;                /* (n_src) mfMaxDistance, what PredictScale divides */
    const float* normal;                  /* (n_src,3) GetNormal(); SIM3 */
    const float* src_angle;               /* (n_src) pKF->mvKeysUn[i].angle; RELOC with check_orientation */
} qsp_search_proj_kf_in;
typedef struct {
    int32_t* choice;                      /* (n_src) the slot the source's point was written to, else -1 */
    int32_t* dist;                        /* (n_src) the best distance, -1 where nothing was compared */
    int32_t* slot_src;                    /* (n) the source whose point the slot holds at the end, -1 untouched, -2 nulled */
    /* the tests' taps, each may be NULL */
    int32_t* reason;                      /* (n_src) */
    int32_t* level;                       /* (n_src) the predicted level */
    float *proj_x, *proj_y;               /* (n_src) */
    int32_t* bin;                         /* (n_src) RELOC with check_orientation: the histogram bin of a matched source, else -1 */
    int32_t n_matches;                    /* matched sources less the histogram removals */
    int32_t hist[30], ind[3];             /* RELOC with check_orientation; else 0 and -1 */
    int32_t n_rounds;
} qsp_search_proj_kf_out;
int qsp_search_by_projection_kf(int device, const qsp_search_proj_kf_in* in, qsp_search_proj_kf_out* out);

/* ---------------------------------------------------------------------------------------------------------------
 * Place recognition: KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:76-197,
 * :199-309) and the minimum-score loop of LoopClosing::DetectLoop (src/LoopClosing.cc:131-148) against a key-frame database that
 * is RESIDENT on the device.  L1Scoring::score is Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68.
 *
 * A qsp_place_db holds, per key frame it knows (a SLOT): the DBoW2::BowVector (word ids int32 strictly ascending, values double,
 * in one growing arena), whether the key frame is LISTED (= in the reference's inverted file) with its list sequence number (the
 * order of the add() calls), and the reference's per-key-frame query state: loop stamp / word count / score (mnLoopQuery,
 * mnLoopWords, mLoopScore) and the same three for relocalisation.  The scores persist from query to query as the members do.
 *
 *   put(kf_id, n, word, value, listed)  makes a key frame known; listed = 1 also appends it to the inverted order (add()).  n == 0
 *                                       is legal.  An id that was erased may be put again: it is a new key frame.
 *   list(kf_id)                         KeyFrameDatabase::add for a known, unlisted key frame.
 *   erase(kf_id)                        KeyFrameDatabase::erase: forgets the key frame; unknown id: QSP_OK, nothing happens.  The slot
 *                                       stays as a hole until clear() (no compaction); size() reports the holes.
 *   clear()                             forgets everything; the handle then behaves like a fresh one.
 *   query / accumulate                  below.  put, list, erase and clear end the life of the last query of either mode:
 *                                       accumulate after them is QSP_ERR_INVALID.
 *
 * qsp_place_db_query -- the map-sized part (:81-139 / :203-253), every rule as the reference has it:
 *   - SHARING.  A listed key frame shares with the query when the two word lists intersect; its common-word count is the size
 *     of the intersection.  LOOP: a key frame named in `excluded` (pKF->GetConnectedKeyFrames(); unknown ids are ignored) is
 *     neither pushed nor stamped (:93-101).  RELOC ignores `excluded`.
 *   - ORDER of lKFsSharingWords.  The reference finds key frames walking the query's words ascending and each word's list in
 *     add() order: that is ascending (first common word, list sequence number), and that key is what the device sorts by.
 *   - minCommonWords = (int)((float)maxCommonWords * 0.8f), a float32 product, truncated.  Scored: common words > minCommonWords.
 *   - SCORE.  Sum in double, in ascending word order over the common words, of fabs(vi - wi) - fabs(vi) - fabs(wi) (vi the
 *     query's value, wi the key frame's), then -sum / 2.0, then converted to float.  The float is what is stored and compared.
 *   - LOOP keeps a scored key frame in lScoreAndMatch when si >= minScore; RELOC keeps every scored one.
 *   - LOOP's minScore is in->min_score, or, with n_ref > 0, DetectLoop's: 1.0f, then (float)score(query, ref) for each ref in
 *     order, keeping the smaller (`score < minScore`).  Every ref must be known (listed or not); the shim leaves bad ones out.
 *   Outputs: n_sharing, max_common, min_common, min_score_used (RELOC: 0), n_match and lScoreAndMatch as (match_id, match_score)
 *   in the reference's order; the taps give id, common-word count and first common word per sharing key frame in order.  Every
 *   output array needs room for `listed` entries (qsp_place_db_size); the first n_match / n_sharing are written.
 *
 * qsp_place_db_accumulate -- the covisibility pass (:144-196 / :258-308) over the lScoreAndMatch the last query of that mode
 * returned, on the device against the resident per-slot state.  The caller gives GetBestCovisibilityKeyFrames(10) of each entry
 * in CSR form (nbr_off (n+1), nbr_id), in the reference's order; a neighbour id that is unknown or erased is "not of this query".
 *   - LOOP: a neighbour counts when this query stamped it and its common words are > minCommonWords; bestAccScore starts at
 *     minScore.  RELOC: a neighbour counts when this query stamped it, EVEN IF IT WAS NOT SCORED in this query -- its score is
 *     then the one left by the last query that scored it (:273-281); bestAccScore starts at 0.
 *   - accScore += score in float32 in neighbour order; the best key frame changes on a strict `>`; minScoreToRetain =
 *     0.75f * bestAccScore; an entry is retained when its accumulated score is strictly greater; the candidates are the retained
 *     entries' best key frames, first occurrence kept.
 *   Outputs: n_cand and cand_id (room for n), taps acc_score (n) and best_id (n).
 *
 * DEVIATIONS, all three on purpose:
 *   1. The reference never initialises mRelocScore; here it starts at 0.0f (so does the loop score).
 *   2. The reference stamps with the querying frame's mnId, so two queries with the same id would double-count the words; here
 *      every call is a new query.
 *   3. mnRelocQuery / mnLoopQuery start at 0 in the reference, so a query by frame id 0 never finds a key frame it has not
 *      stamped before; not reproduced.
 *
 * Host pointers.  No output is written unless the call returns QSP_OK, and a refused put / list leaves the database as it was.
 * A query that is refused (QSP_ERR_INVALID / _UNSUPPORTED) leaves the resident state as it was too.  A query that fails LATER, with
 * QSP_ERR_DEVICE or out of host memory after its kernels were launched, writes no output either, but the stamps, word counts and
 * scores of its mode on the device may already be those of the failed query (a later RELOC query can then read such a score as the
 * stale one); the last query of that mode is dead, so accumulate is refused until the next successful query.
 * SIZE.  No count is capped, but the order and the accumulate kernel are ONE workgroup each, taking entries 1024 at a time, and the
 * ranking is quadratic in the number of sharing key frames: that part is serial on one compute unit (about 3 ms at 5000 sharing
 * key frames, profiles/place_db.txt).
 * QSP_ERR_INVALID: null required pointers (arrays of n == 0 entries may be NULL), negative sizes, an unknown mode, words that are
 * negative or not strictly ascending, values that are not finite, a kf_id put twice, listing an unknown or already listed id, an
 * unknown ref_id, a min_score that is NaN, nbr_off that does not start at 0 or decreases, and accumulate called with ids that are
 * not the last query's lScoreAndMatch of that mode.  More than 2^31 - 1 words or slots: QSP_ERR_UNSUPPORTED.
 * words_hint / slots_hint of create: the initial capacities (0: 1 Mi words, 1024 slots); both grow by doubling. */
typedef struct qsp_place_db qsp_place_db;
enum { QSP_PLACE_LOOP = 0, QSP_PLACE_RELOC = 1 };
typedef struct {
    int32_t mode;                 /* QSP_PLACE_LOOP / QSP_PLACE_RELOC */
    int32_t n;                    /* the query's mBowVec.size() */
    const int32_t* word;          /* (n) strictly ascending */
    const double* value;          /* (n) */
    int32_t n_excluded;           /* LOOP */
    const int64_t* excluded;      /* (n_excluded) ids of the connected key frames */
    float min_score;              /* LOOP with n_ref == 0 */
    int32_t n_ref;                /* LOOP: > 0 computes DetectLoop's minimum score from these */
    const int64_t* ref_id;        /* (n_ref) */
} qsp_place_query_in;
typedef struct {
    int32_t n_sharing, max_common, min_common, n_match;
    float min_score_used;
    int64_t* match_id;            /* (listed) lScoreAndMatch: the key frames ... */
    float* match_score;           /* (listed) ... and their scores */
    /* the tests' taps, each may be NULL: lKFsSharingWords in order */
    int64_t* sharing_id;          /* (listed) */
    int32_t* sharing_common;      /* (listed) */
    int32_t* sharing_first;       /* (listed) the first common word */
} qsp_place_query_out;
typedef struct {
    int32_t n_cand;
    int64_t* cand_id;             /* (n) */
    /* the tests' taps, each may be NULL */
    float* acc_score;             /* (n) */
    int64_t* best_id;             /* (n) */
} qsp_place_acc_out;
int qsp_place_db_create(int device, int64_t words_hint, int32_t slots_hint, qsp_place_db** db);
void qsp_place_db_destroy(qsp_place_db* db);
int qsp_place_db_put(qsp_place_db* db, int64_t kf_id, int32_t n, const int32_t* word, const double* value, int32_t listed);
int qsp_place_db_list(qsp_place_db* db, int64_t kf_id);
int qsp_place_db_erase(qsp_place_db* db, int64_t kf_id);
int qsp_place_db_clear(qsp_place_db* db);
/* each may be NULL; device_bytes: what the handle holds on the device */
int qsp_place_db_size(qsp_place_db* db, int32_t* known, int32_t* listed, int32_t* dead_slots, int64_t* device_bytes);
int qsp_place_db_query(qsp_place_db* db, const qsp_place_query_in* in, qsp_place_query_out* out);
int qsp_place_db_accumulate(qsp_place_db* db, int32_t mode, int32_t n, const int64_t* id, const int32_t* nbr_off, const int64_t* nbr_id,
                            qsp_place_acc_out* out);

#ifdef __cplusplus
}
#endif
#endif /* QSP_HIP_H */
