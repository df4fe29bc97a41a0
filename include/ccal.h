/*
 * ccal.h -- C ABI of the MI355X-native reprojection residual + Jacobian engine
 * and Gauss-Newton / Levenberg-Marquardt normal-equation builder.
 *
 * This is the drop-in boundary for the hot path of
 * powei-lin/camera-intrinsic-calibration-rs (paths below are relative to the
 * reference tree).  A Rust caller binds these symbols with `extern "C"`
 * (INTEGRATION.md shows the stub); everything is plain pointers + sizes, no
 * C++ types, no exceptions, no torch types.  All floating point is f64 except
 * the detected-corner inputs, which are f32 exactly as the reference holds
 * them (src/detected_points.rs:6-9, widened at src/optimization/factors.rs:141-143).
 *
 * What each entry point replaces:
 *   ccal_problem_create      the `problem.add_residual_block(2, [...], ReprojectionFactor|
 *                            OtherCamReprojectionFactor, HuberLoss(1.0))` loops
 *                            src/util.rs:401-414 and src/util.rs:595-631
 *   ccal_set_bounds          tiny_solver::Problem::set_variable_bounds   src/util.rs:36-47
 *   ccal_fix_param           tiny_solver::Problem::fix_variable          src/util.rs:61,461,666
 *   ccal_apply_reference_bounds / ccal_disable_distortions
 *                            set_problem_parameter_bound / _disabled     src/util.rs:29-71
 *   ccal_eval                Factor::residual_func evaluated with dual numbers for every
 *                            block (src/optimization/factors.rs:152-173, 204-228)
 *   ccal_build_normal        tiny-solver's J^T J / J^T r assembly (call sites src/util.rs:455,670),
 *                            with the per-frame pose blocks eliminated exactly (Schur)
 *   ccal_solve / _dev        GaussNewtonOptimizer::optimize(&problem, &initial_values, None)
 *                            src/util.rs:443-463 and 668-670 (+ an LM mode)
 *   ccal_init_poses          the unproject + sqpnp pose initialisation inside calib_camera  src/util.rs:418-436
 *   ccal_reprojection_errors / ccal_validation
 *                            validation()                                 src/util.rs:721-795
 *   ccal_rdh_batch / ccal_radial_distortion_homography
 *                            radial_distortion_homography                 src/optimization/homography.rs:218-271
 *   ccal_homography_to_focal homography_to_focal                          src/optimization/homography.rs:274-325
 *   ccal_pnp_batch           sqpnp_solve_glam (any 3-D point set), batched  src/util.rs:431
 *   ccal_init_poses_division init_pose                                    src/optimization/linear.rs:5-21
 *   ccal_refine_poses_batch  ReprojectionFactor + HuberLoss over the pose alone, intrinsics fixed, batched
 *   ccal_refine_rig_poses_batch
 *                            OtherCamReprojectionFactor + HuberLoss over T_0_b alone, intrinsics and extrinsics fixed, batched
 *   ccal_refine_corners_batch / _dev
 *                            the sub-pixel step at the end of image_to_option_feature_frame  src/data_loader.rs:36-70 (not the detector)
 *   ccal_detect_corners_batch / _dev
 *                            checkerboard-corner candidates of whole images (this project's integer saddle rule; the reference's
 *                            tag detector is in the absent aprilgrid crate)
 *   ccal_decode_tags_batch / _dev
 *                            which tag a candidate quad holds, its turn and its bit errors, against a caller-supplied family
 *                            (this project's rule; what tag_detector.detect decides inside the absent aprilgrid crate)
 *   ccal_propose_quads_batch / _dev
 *                            candidate tag outlines of an AprilGrid from refined saddle points: what feeds ccal_decode_tags_* from
 *                            images alone (this project's rule)
 *
 * Parameter layout.
 *   intr   [n_cams][CCAL_PMAX]  FULL model parameters [fx,fy,cx,cy,dist...] per camera, like
 *                               GenericModel::params().  With xy_same_focal the solver variable is
 *                               f = intr[c][0] and fy is ignored on input / set to f on output
 *                               (src/util.rs:391-395, 467-470).
 *   poses  [n_slots][6]         rvec(3), tvec(3) of T_cam0_board per frame slot
 *                               ("rvec{i}","tvec{i}" / "rvec_0_b_{f}","tvec_0_b_{f}").
 *   extr   [n_cams][6]          rvec, tvec of T_cam_i_cam0 ("rvec_{c}_0","tvec_{c}_0"); row 0 unused.
 * Solver-visible intrinsic index space ("eff" indices): full index with fy removed when
 * xy_same_focal (the `shift` of src/util.rs:35).  Bounds / fixed flags use eff indices, exactly
 * like the reference's set_variable_bounds / fix_variable calls.
 *
 * Jacobian column order of one block (ccal_eval): [theta_c (P_eff) | rvec_0_b | tvec_0_b] for
 * camera 0 blocks and [theta_c | rvec_0_b | tvec_0_b | rvec_c_0 | tvec_c_0] for camera c>0
 * (src/util.rs:411, 621-627).
 * Reduced ("camera") system column order (ccal_build_normal): for c = 0..n_cams-1:
 * theta_c (P_eff(c)), then for c>0 rvec_c_0, tvec_c_0.  K = sum P_eff + 6 (n_cams-1).
 *
 * Environment.  The behaviour contract of this ABI does not depend on the environment.  libccal_hip.so reads exactly TWO
 * variables: CCAL_RCCL_LIB (the RCCL library to dlopen when none is loaded in the process yet) and CCAL_MULTI_TRANSPORT
 * (inproc | rccl: the transport ccal_multi_create picks when the caller leaves the choice to it).  Neither changes a result.
 * The A/B developer switches and the test hooks live in a second library that only the parity tests load
 * (libccal_hip_legacy.so); a binding sets nothing.
 */
#ifndef CCAL_H
#define CCAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCAL_PMAX 10          /* row stride of intr / bounds arrays (max model has 9 params) */
#define CCAL_MAX_CAMS 8
#define CCAL_KMAX 128         /* the reduced camera system has fewer columns than this: eight cameras of any model fit (8 x 9 + 7 x 6 = 114) */

typedef enum {
    CCAL_OK = 0,
    CCAL_ERR_INVALID_ARG = 1,
    CCAL_ERR_HIP = 2,
    CCAL_ERR_NONFINITE = 3,       /* NaN/Inf cost: tiny-solver returns None (src/util.rs:455-457) */
    CCAL_ERR_NOT_PD = 4,          /* Cholesky of the normal equations failed: None */
    CCAL_ERR_NO_CONVERGENCE = 5,  /* informational: max_iterations reached (reference still returns Some) */
    CCAL_ERR_UNSUPPORTED = 6,
    CCAL_ERR_NO_MEMORY = 7,       /* host allocation failed inside the library (never thrown across the ABI) */
    CCAL_NO_RESULT = 8            /* the reference's `None` of an estimator that found nothing (homography_to_focal, an RANSAC
                                     without one admissible hypothesis): not a failure of the call, the caller tries again */
} ccal_status;

typedef enum {                    /* camera-intrinsic-model GenericModel variants on the hot path */
    CCAL_MODEL_UCM = 0,           /* [fx,fy,cx,cy,alpha]              tests/optimization_test.rs:41 */
    CCAL_MODEL_EUCM = 1,          /* [fx,fy,cx,cy,alpha,beta]         data/eucm.json              */
    CCAL_MODEL_KB4 = 2,           /* [fx,fy,cx,cy,k1,k2,k3,k4]                                     */
    CCAL_MODEL_OPENCV5 = 3,       /* [fx,fy,cx,cy,k1,k2,p1,p2,k3]                                  */
    CCAL_MODEL_EUCMT = 4          /* [fx,fy,cx,cy,alpha,beta,t1,t2]: PARAMETER CONTAINER ONLY - the target of the closed-form
                                     UCM -> EUCMT conversion (src/util.rs:236-243); its projection exists only in the absent
                                     crate, so problems with it are refused with CCAL_ERR_UNSUPPORTED */
} ccal_model;

/* What this build assumes about the crate camera-intrinsic-model 0.8 (Cargo.toml:25; its source is not part of the
 * reference tree) and can be changed at run time, per context, without rebuilding a kernel.  Defaults:
 * camera_intrinsic_calibration_rs_amd/csrc/ccal_models.hpp. */
typedef struct {
    double kb4_small_radius;       /* KB4 project_one: sqrt(x^2+y^2) <= this -> pinhole limit.  Default 1e-8 */
    double dist_lo[4][5];          /* [ccal_model][i]: lower / upper bound of distortion parameter i in the order of the     */
    double dist_hi[4][5];          /* model rows of ccal_model above (OPENCV5: k1, k2, p1, p2, k3 whatever ocv5_order says), */
                                   /* i.e. what distortion_params_bound() returns (applied at src/util.rs:40-48)             */
    double unproject_small_radius; /* unprojection (pose initialisation, convert_model's rays): image-plane radius below which
                                      the ray is the optical axis.  Default 1e-8 */
    int32_t ocv5_order[5];         /* WHERE k1, k2, p1, p2, k3 sit among the five distortion parameters of an OPENCV5 params()
                                      vector: parameter 4 + ocv5_order[i] is k1 (i = 0), k2, p1, p2, k3 (i = 4).  Default
                                      {0, 1, 2, 3, 4} = OpenCV's own order.  Every array of this ABI that follows the parameter
                                      order (intrinsics in / out, eff indices of bounds and fixed parameters, Jacobian and
                                      normal-equation columns, "the last k distortion parameters") follows THIS order */
    int32_t reserved_;
} ccal_model_conventions;

typedef struct ccal_ctx ccal_ctx;          /* one GPU + one HIP stream; single caller */
typedef struct ccal_problem ccal_problem;  /* inputs resident in HBM + workspaces */

/* Problem description = the reference's calib-frame inputs flattened.
 * An "observation frame" is one (camera, frame slot) pair with its detected corners stored
 * contiguously: corners [obs_offsets[i], obs_offsets[i+1]) of the SoA arrays.  Single camera:
 * n_obs == n_slots, obs_cam[i] == 0, obs_slot[i] == i. */
typedef struct {
    int32_t n_cams;
    const int32_t* model;          /* [n_cams] ccal_model */
    const double* width;           /* [n_cams] image width  (bounds, src/util.rs:38) */
    const double* height;          /* [n_cams] image height (bounds, src/util.rs:39) */
    int32_t xy_same_focal;         /* ReprojectionFactor::xy_same_focal */
    int32_t n_slots;               /* board-pose slots (frames) */
    int32_t n_obs;                 /* observation frames */
    const int32_t* obs_cam;        /* [n_obs] */
    const int32_t* obs_slot;       /* [n_obs] */
    const int64_t* obs_offsets;    /* [n_obs+1] */
    const float* p3d_x;            /* [n_corners] board point (FeaturePoint::p3d), f32 */
    const float* p3d_y;
    const float* p3d_z;
    const float* p2d_u;            /* [n_corners] detected pixel (FeaturePoint::p2d), f32 */
    const float* p2d_v;
    double huber_delta;            /* HuberLoss::new(1.0) in the reference; <= 0 disables the loss */
} ccal_problem_desc;

typedef enum { CCAL_METHOD_GN = 0, CCAL_METHOD_LM = 1 } ccal_method;

typedef struct {
    int32_t method;                /* CCAL_METHOD_GN is the reference's optimizer (parity mode) */
    int32_t max_iterations;        /* tiny-solver default 100 */
    double min_abs_error_decrease; /* 1e-5 */
    double min_rel_error_decrease; /* 1e-5 */
    double min_error;              /* 1e-10 */
    double lm_initial_radius;      /* 1e4   (LM only; Ceres-style trust region, lambda = 1/radius) */
    double lm_min_diagonal;        /* 1e-6 */
    double lm_max_diagonal;        /* 1e32 */
    int32_t verbose;
    int32_t timeout_s;             /* host-side watchdog of the device-resident loop, seconds without a step completing.
                                      0 = default: 30 s on a single GPU, 600 s in a sharded solve (a communicator or an
                                      all-reduce callback is set): a step that waits for a peer - still uploading, still
                                      setting up RCCL channels - is waited for, a peer that died does not hang the
                                      survivors for ever.  Give every rank the same value: a rank that gives up
                                      (CCAL_ERR_HIP, "timed out") leaves the shared sequence of collectives while its peers
                                      are inside ncclAllReduce - see "Errors" below: exit or abort the communicator, never
                                      re-exec a process that has touched the GPU */
    int32_t error_metric;          /* what the stop rules above call "error" - a guess about the absent crate made switchable
                                      (tiny-solver 0.18, Optimizer::compute_error: squared_norm_l2() or norm_l2() of the
                                      loss-corrected residuals; call sites src/util.rs:443,455).  CCAL_ERROR_SQUARED_NORM (0,
                                      the default): sum rho'(s) s, what ccal_report::initial_cost / final_cost hold.
                                      CCAL_ERROR_NORM (1): its square root - min_error and the absolute / relative decreases are
                                      then compared on sqrt(cost); the reports still hold the squared norm */
    int32_t reserved_;             /* 0 */
} ccal_solver_opts;
typedef enum { CCAL_ERROR_SQUARED_NORM = 0, CCAL_ERROR_NORM = 1 } ccal_error_metric;

typedef struct {
    int32_t status;                /* ccal_status of the solve */
    int32_t iterations;            /* linear solves performed */
    int32_t lm_accepted;
    int32_t lm_rejected;
    double initial_cost;           /* sum over blocks of rho'(s) * s at the start (tiny-solver's "error") */
    double final_cost;
    double solve_ms;               /* wall time of the iteration loop */
    int32_t lm_spec_hits;          /* LM: accepted steps whose speculative elimination was the next system (one group) */
    int32_t lm_spec_misses;        /*     ... and those that needed a re-elimination group                              */
} ccal_report;

/* Frame-sharded multi-GPU solves (one process per GPU, every rank holds a contiguous range of frame slots and the
 * same camera parameters): ONE in-place sum of a small device buffer ([reduced system | cost | model decrease | failed
 * blocks], 100..400 doubles) over all ranks per optimizer step, Gauss-Newton and Levenberg-Marquardt alike.
 *   ccal_set_rccl_comm   the library calls ncclAllReduce(buf, buf, n, ncclDouble, ncclSum, comm, stream) itself,
 *                        stream-ordered, and keeps enqueueing steps ahead of the host.  The production path.
 *   ccal_set_allreduce   a callback does the sum (ordered on `hip_stream`) - for transports other than RCCL
 *                        (the tests use gloo); the loop then waits for every step before it enqueues the next.
 * Neither set = single GPU.
 * Errors: every rank issues the same sequence of collectives by construction (one per step, decisions taken from
 * all-reduced sums).  If a sharded ccal_solve nevertheless returns an error other than the solver's own verdicts
 * (NONFINITE / NOT_PD / NO_CONVERGENCE, which all ranks reach together), collectives of this rank may still be queued
 * with no partner: treat the communicator as INVALID - abort it (ncclCommAbort) or exit the process; do not reuse it and
 * do not wait for the stream. */
typedef int (*ccal_allreduce_fn)(void* user, double* device_buf, size_t count, void* hip_stream);
#define CCAL_RCCL_UNIQUE_ID_BYTES 128

/* ---- context ----------------------------------------------------------------------------
 * A problem holds its context: ccal_ctx_destroy with problems still alive is deferred to the last ccal_problem_destroy
 * (any destruction order is safe); a caller-provided stream must stay alive while work is enqueued on it. */
int ccal_ctx_create(int device_id, void* hip_stream /* hipStream_t or NULL = own stream */, ccal_ctx** out);
void ccal_ctx_destroy(ccal_ctx* ctx);
const char* ccal_last_error(const ccal_ctx* ctx);
const char* ccal_version(void);
int ccal_model_num_params(int model);            /* 5 / 6 / 8 / 9 (/ 8 for the EUCMT container), -1 if unknown */
/* Conventions of a context: read them, change a field, set them (in == NULL restores the defaults).  They apply to
 * everything the context evaluates afterwards (kernels receive the threshold as an argument) and to later
 * ccal_apply_reference_bounds / ccal_convert_model calls. */
int ccal_get_model_conventions(const ccal_ctx* ctx, ccal_model_conventions* out);
int ccal_set_model_conventions(ccal_ctx* ctx, const ccal_model_conventions* in);

/* Host memory the caller hands to ccal_solve* / ccal_upload_params / ccal_download_params can be PINNED once (page-locked and
 * mapped for the GPU): the library then moves it without its intermediate staging copy - the kernels read the starting poses where
 * the caller keeps them, the result is written there by one DMA (10 000 frames: ~85 us of a 240-us ccal_solve are the two staging
 * copies of 480 KB of poses; src/util.rs:384-390 hands such a map over per call).  ccal_pin_buffer registers [host_ptr, host_ptr +
 * bytes) (hipHostRegister; memory the caller allocated pinned itself - hipHostMalloc - is recognised without it); the range must
 * stay allocated until ccal_unpin_buffer or ccal_ctx_destroy.  Pinning never changes a result (same kernels, same bits). */
int ccal_pin_buffer(ccal_ctx* ctx, void* host_ptr, size_t bytes);
int ccal_unpin_buffer(ccal_ctx* ctx, void* host_ptr);

/* ---- problem ---------------------------------------------------------------------------- */
/* One problem holds at most 2^30 - 1 corners (CCAL_ERR_INVALID_ARG beyond: shard the frames, ccal_multi_problem_create). */
int ccal_problem_create(ccal_ctx* ctx, const ccal_problem_desc* desc, ccal_problem** out);
void ccal_problem_destroy(ccal_problem* p);
int ccal_set_defaults(ccal_solver_opts* opts);   /* tiny-solver OptimizerOptions::default() */
int ccal_set_bounds(ccal_problem* p, int cam, int eff_idx, double lo, double hi);
int ccal_clear_bounds(ccal_problem* p, int cam, int eff_idx);
int ccal_fix_param(ccal_problem* p, int cam, int eff_idx);
int ccal_unfix_param(ccal_problem* p, int cam, int eff_idx);
int ccal_apply_reference_bounds(ccal_problem* p);                 /* src/util.rs:29-49 for every camera */
int ccal_disable_distortions(ccal_problem* p, int n_disabled, double* intr_io /* zeroed in place */);
int ccal_set_allreduce(ccal_problem* p, ccal_allreduce_fn fn, void* user);
int ccal_set_rccl_comm(ccal_problem* p, void* nccl_comm /* ncclComm_t created by the host or by ccal_rccl_comm_create; NULL = none */);
/* Communicator bootstrap for hosts that do not link RCCL themselves: rank 0 draws an id, hands its 128 bytes to every
 * rank by any means (file, socket, MPI, the launcher's store), every rank creates its communicator on its context's GPU.
 * RCCL is resolved at run time (the instance already loaded into the process, else librccl.so.1). */
int ccal_rccl_available(void);                                    /* 1 if an RCCL library could be resolved */
int ccal_rccl_version(void);                                      /* ncclGetVersion, 0 if unavailable */
int ccal_rccl_unique_id(void* id_out /* CCAL_RCCL_UNIQUE_ID_BYTES */);
int ccal_rccl_comm_create(ccal_ctx* ctx, int world, int rank, const void* id /* 128 bytes */, void** comm_out);
int ccal_rccl_comm_destroy(void* comm);
int ccal_rccl_comm_count(void* comm);                             /* ncclCommCount: ranks of the communicator, -1 on error */

int64_t ccal_num_corners(const ccal_problem* p);
int ccal_reduced_dim(const ccal_problem* p);                      /* K */
int ccal_block_dim(const ccal_problem* p, int cam);               /* D of that camera's blocks */
int ccal_eff_num_params(const ccal_problem* p, int cam);          /* P_eff */
int64_t ccal_jacobian_len(const ccal_problem* p);                 /* doubles in J_out of ccal_eval */

/* ---- mode E: residual + Jacobian of every block ------------------------------------------
 * r_out [n_corners][2]; J_out: per observation frame, [n_i][2][D_cam] row-major blocks, frames
 * concatenated (offset of frame i = sum_{j<i} n_j * 2 * D_cam(j)).  apply_loss != 0 applies the
 * Huber corrector (r and J scaled by sqrt(rho')) the way tiny-solver does before assembly.
 * *_dev variants take device pointers and only enqueue work on the context stream. */
int ccal_eval(ccal_problem* p, const double* intr, const double* poses, const double* extr,
              int apply_loss, double* r_out, double* J_out);
int ccal_upload_params(ccal_problem* p, const double* intr, const double* poses, const double* extr);
int ccal_download_params(ccal_problem* p, double* intr, double* poses, double* extr);
int ccal_eval_dev(ccal_problem* p, int apply_loss, double* r_out_dev, double* J_out_dev);
int ccal_sync(ccal_ctx* ctx);

/* ---- mode N: fused normal equations + exact per-frame Schur complement -------------------
 * S [K][K] (row-major, symmetric, full), b [K] = reduced J^T r (so S dx = -b), cost = sum rho' s.
 * lambda > 0 adds Marquardt damping lambda * clamp(diag) to every block before elimination. */
int ccal_build_normal(ccal_problem* p, const double* intr, const double* poses, const double* extr,
                      double lambda, double* S, double* b, double* cost);
int ccal_build_normal_dev(ccal_problem* p, double lambda);   /* uses uploaded params; result stays on device */

/* ---- the optimizer loop --------------------------------------------------------------------
 * ccal_solve: host pointers in and out (poses staged through pinned memory both ways - unless the caller's arrays are pinned
 * themselves, ccal_pin_buffer: then they are read and written in place).
 * ccal_solve_dev: the starting point is what ccal_upload_params (or a previous solve) left on the device, the result
 * stays there (ccal_download_params fetches it); the call itself moves ~1 KB to the device and polls a status word. */
int ccal_solve(ccal_problem* p, const ccal_solver_opts* opts,
               double* intr_io, double* poses_io, double* extr_io, ccal_report* report);
int ccal_solve_dev(ccal_problem* p, const ccal_solver_opts* opts, ccal_report* report);
/* n INDEPENDENT problems solved side by side in ONE call (the per-camera calib_camera calls of a rig, the retries of
 * src/bin/camera_calibration.rs:205-246, many sessions of a service): a session-sized problem (a few hundred frames) leaves
 * the GPU almost idle - one latency-bound launch per optimizer step.  Session-sized single-camera problems of one
 * GPU, model and focal mode advance in LOCKSTEP: ONE launch per step serves all of them (the problems' workgroups side by side), so
 * a batch of eight costs the host what one solve costs.  Everything else (rigs, large problems) is driven per context by a
 * host thread of its own (create such problems on contexts of their own - ccal_ctx_create with stream NULL - to make them overlap;
 * those that share a context are solved one after the other).  A problem's launches are sized for its share of the GPU (the batch's
 * problems on that device): fewer, longer wavefronts than a lone ccal_solve takes - results equal to n ccal_solve calls up to the
 * order of summation (<= 1e-11 relative; the lane mapping, hence the order, depends on how many problems of the batch share the
 * GPU: the same problem in another batch may differ in the last bits); verdict and iteration count can differ from a lone
 * ccal_solve only where a stop threshold is met to within that rounding.  A problem that needs bit-reproducible results
 * whatever runs beside it is solved with ccal_solve.  intr_io == NULL: device-resident like ccal_solve_dev (poses_io / extr_io ignored);
 * else intr_io[i] / poses_io[i] / extr_io[i] as in ccal_solve.  Every problem's verdict goes to reports[i].status; the return
 * value is CCAL_OK unless a call failed for another reason (then the first such code).  Sharded problems are refused. */
int ccal_solve_batch(ccal_problem** problems, int n, const ccal_solver_opts* opts,
                     double** intr_io, double** poses_io, double** extr_io, ccal_report* reports);

/* ---- one process, several GPUs ------------------------------------------------------------------
 * The reference is ONE process: calib_camera is one blocking call of the tool's main (src/util.rs:384-390,
 * src/bin/camera_calibration.rs:70).  These entry points keep it that way on a multi-GPU node: the library shards the
 * frame slots, drives every GPU from a host thread of its own and owns the transport of the step's one all-reduce.
 *
 * ccal_solve_sharded: n shards of ONE problem - problems created by the caller on n DIFFERENT contexts (one per GPU;
 *   contexts on the same GPU work too), each holding a contiguous range of the frame slots with every camera's
 *   observations of those slots, the same cameras, bounds and fixed parameters.  intr_io / extr_io: the shared camera
 *   block (in: starting point, out: result - bit-identical on every shard, checked); poses_io[i]: shard i's poses
 *   [n_slots_i][6].  Transport: whatever is set on ALL shards (ccal_set_rccl_comm / ccal_set_allreduce); none set = the
 *   library's in-process transport for the duration of the call (HIP events order the shards' streams, a kernel adds the
 *   shards' buffers in shard order; needs the shards on one GPU or peer access between their GPUs).  The report is the
 *   solve's (every shard reaches the same verdict and iteration count; solve_ms = the slowest shard).
 * ccal_multi_*: the same with the sharding done by the library.  ccal_multi_create makes one context per listed device
 *   and the transport between them - RCCL (ncclCommInitAll, one communicator per device) when the devices are all
 *   different and RCCL can be resolved, the in-process transport otherwise (a device listed twice: two shards on one GPU).
 *   ccal_multi_problem_create takes the SAME description as ccal_problem_create and cuts it into contiguous slot ranges
 *   balanced by corner count; poses / poses_obs / n_used keep the caller's slot and observation-frame order.
 * Threading: like a ccal_ctx, a ccal_multi (and its problems) is single-caller; the host threads that drive the devices inside a
 * call are the library's own.
 * Errors: as for sharded solves above.  A shard that fails raises a flag its peers see at their next look at the status word: they
 * stop waiting at once (not at the timeout).  After an error other than the solver's verdicts a ccal_multi with the in-process
 * transport recovers by itself; with RCCL its communicators are aborted and every later ccal_multi_solve on it fails
 * (CCAL_ERR_HIP): destroy it and create a new one. */
#define CCAL_MULTI_MAX_DEVICES 16
typedef enum { CCAL_TRANSPORT_NONE = 0 /* one device */, CCAL_TRANSPORT_RCCL = 1, CCAL_TRANSPORT_INPROC = 2 } ccal_transport;
typedef struct ccal_multi ccal_multi;                  /* a set of contexts (one per listed device) + their transport */
typedef struct ccal_multi_problem ccal_multi_problem;  /* one problem, frame slots sharded over the contexts of a ccal_multi */

int ccal_solve_sharded(ccal_problem** shards, int n, const ccal_solver_opts* opts,
                       double* intr_io, double** poses_io, double* extr_io, ccal_report* report);

int ccal_multi_create(const int* device_ids, int n_dev, ccal_multi** out);
/* the same with the transport named: -1 = automatic (ccal_multi_create), CCAL_TRANSPORT_RCCL = communicators even for ONE listed
 * device, CCAL_TRANSPORT_INPROC = the in-process transport even where RCCL is there.  A transport asked for by name is not
 * replaced by another one when it cannot be set up (CCAL_ERR_UNSUPPORTED, reason in ccal_create_last_error). */
int ccal_multi_create_transport(const int* device_ids, int n_dev, int transport, ccal_multi** out);
int ccal_multi_rccl_ranks(const ccal_multi* m);        /* ranks RCCL counts in the set's communicators (ncclCommCount); 0: not RCCL */
/* why the last ccal_ctx_create / ccal_multi_create* ON THIS THREAD failed (no handle exists to ask); "" after a success */
const char* ccal_create_last_error(void);
/* Host-only (no GPU touched): where ccal_multi_problem_create cuts a description into n_shards contiguous frame-slot ranges
 * balanced by corner count - first_out[i] .. first_out[i + 1] are shard i's slots (first_out has n_shards + 1 entries).  A host
 * that runs one process per GPU cuts its problem with the same function (bench.py --frames-total does). */
int ccal_partition_slots(const ccal_problem_desc* desc, int n_shards, int32_t* first_out);
void ccal_multi_destroy(ccal_multi* m);                /* deferred to the last ccal_multi_problem_destroy if problems are alive */
int ccal_multi_num_devices(const ccal_multi* m);
int ccal_multi_transport(const ccal_multi* m);         /* ccal_transport */
ccal_ctx* ccal_multi_ctx(ccal_multi* m, int i);        /* context of device i (ccal_last_error, conventions) */
const char* ccal_multi_last_error(const ccal_multi* m);
int ccal_multi_set_model_conventions(ccal_multi* m, const ccal_model_conventions* in);   /* on every context */
int ccal_multi_sync(ccal_multi* m);

int ccal_multi_problem_create(ccal_multi* m, const ccal_problem_desc* desc, ccal_multi_problem** out);
void ccal_multi_problem_destroy(ccal_multi_problem* mp);
int ccal_multi_problem_num_shards(const ccal_multi_problem* mp);
ccal_problem* ccal_multi_problem_shard(ccal_multi_problem* mp, int i);   /* borrowed: sizes, mode E buffers; do not destroy */
int ccal_multi_problem_slot_range(const ccal_multi_problem* mp, int i, int32_t* first_slot, int32_t* n_slots);
int ccal_multi_set_bounds(ccal_multi_problem* mp, int cam, int eff_idx, double lo, double hi);
int ccal_multi_clear_bounds(ccal_multi_problem* mp, int cam, int eff_idx);
int ccal_multi_fix_param(ccal_multi_problem* mp, int cam, int eff_idx);
int ccal_multi_unfix_param(ccal_multi_problem* mp, int cam, int eff_idx);
int ccal_multi_apply_reference_bounds(ccal_multi_problem* mp);
int ccal_multi_disable_distortions(ccal_multi_problem* mp, int n_disabled, double* intr_io);
int ccal_multi_init_poses(ccal_multi_problem* mp, const double* intr, int min_points, double* poses_obs, int32_t* n_used);
int ccal_multi_upload_params(ccal_multi_problem* mp, const double* intr, const double* poses /* [n_slots][6], all slots */, const double* extr);
int ccal_multi_eval_dev(ccal_multi_problem* mp, int apply_loss, double* const* r_dev, double* const* J_dev);   /* per shard device buffers; no collective */
/* validation() (src/util.rs:721-795) over the shards: the same statistics, bit for bit, as ccal_validation on one GPU */
int ccal_multi_validation(ccal_multi_problem* mp, int cam, const double* intr, const double* poses, const double* extr,
                          double* avg_99_percent, double* median);
int ccal_multi_reprojection_errors(ccal_multi_problem* mp, const double* intr, const double* poses, const double* extr,
                                   double* err_out /* [n_corners], the description's corner order */,
                                   const int64_t* obs_offsets /* the description's obs_offsets [n_obs + 1] */);
int ccal_multi_solve(ccal_multi_problem* mp, const ccal_solver_opts* opts,
                     double* intr_io, double* poses_io /* [n_slots][6], all slots */, double* extr_io, ccal_report* report);

/* ---- per-frame pose initialisation (src/util.rs:418-436) ---------------------------------
 * What calib_camera does before it builds the problem: unproject the detections with the current model,
 * keep the valid ones, divide by z, planar PnP (the reference calls sqpnp_simple; here a plane-induced
 * homography -- same basin, the joint solve refines it).  poses_obs [n_obs][6] = T_cam_board of every
 * observation frame; n_used [n_obs] = corners that entered the estimate, 0 = no pose (the reference skips
 * frames with fewer than 10 valid unprojections: pass min_points = 10).
 * A frame gets NO pose - six zeros, n_used 0 - when
 *   - fewer than min_points corners unproject (outside the model's domain, or not in front of the camera),
 *   - its valid corners do not span the board plane (one row, one column, a diagonal, one corner repeated: rotation about the
 *     line is free): a Cholesky pivot s of the 8 x 8 normal matrix M is at or below 2^-36 (1.46e-11) x its own diagonal entry M_jj.
 *     Well-posed frames sit above 1e-6 (two adjacent rows: 2.6e-3), rank-deficient ones at rounding, below 1e-13,
 *   - the homography's first two columns are not two directions (a norm at or below 1e-12) or the result is not finite.
 * Of the homography's two signs the pose is the one with the corners in front of the camera (their summed depth is positive, the
 * rule of ccal_pnp_batch), wherever the board's origin lies.
 *
 * The homography serves frames whose corners all have z == 0 (z = -0 counts).  A frame with any z != 0 - a board whose coordinates
 * are not at z = 0, boards hinged at an angle, any 3-D target - takes a general PnP instead (ccal_pnp_batch below: the same
 * estimator, the same rules for "no pose"); one call may mix both kinds of frame, for any camera of a rig.  The same holds for
 * ccal_init_poses_division and ccal_multi_init_poses. */
int ccal_init_poses(ccal_problem* p, const double* intr, int min_points, double* poses_obs, int32_t* n_used);

/* ---- general PnP, batched (sqpnp_simple::sqpnp_solve_glam: src/util.rs:431, src/optimization/linear.rs:19, examples/test_pnp.rs:61)
 * n_prob independent problems in one launch, one wavefront each.  Problem i holds the points [offsets[i], offsets[i + 1]) of
 * xyz [.][3] (any 3-D point set, planar ones included) and xn [.][2], their NORMALISED image points (x / z, y / z of the unprojected
 * detections); offsets[0] == 0; points with a coordinate that is not finite are left out.  The estimator minimises the cost SQPnP is
 * built on: with Q_i = [1 0 -x_i; 0 1 -y_i],
 *     E(R, t) = sum_i | Q_i (R X_i + t) |^2
 * is quadratic in t, so t*(R) = P vec(R) and E(R) = vec(R)^T Omega vec(R) with a 9 x 9 Omega from per-point sums (the X_i centred on
 * their centroid).  E(R) is minimised over SO(3) from 64 fixed, well-spread starting rotations, 24 damped Gauss-Newton steps and 2
 * undamped ones each;
 * the result is the candidate of lowest E among those with the points in front of the camera, sum_i (R X_i + t)_z > 0 (the mirror
 * twin of a coplanar target has the same E and negative depth: it loses), ties to the lowest start index.  The outputs are a pure
 * function of a problem's points: they do not depend on what else is in the batch.
 * poses_out [n_prob][6] = rvec (from the quaternion with qw >= 0), tvec = t*(R); n_used_out [n_prob] = points that entered, 0 = no
 * pose; cost_out [n_prob] (or NULL) = E at the result.  A problem gets NO pose - six zeros, n_used 0, cost 0 - when
 *   - fewer than max(min_points, 4) points are valid,
 *   - sum_i Q_i^T Q_i is singular (n sum(x^2 + y^2) - (sum x)^2 - (sum y)^2 <= 1e-12 n sum(x^2 + y^2): one image point),
 *   - the points are collinear: the second eigenvalue of the centred scatter sum (X_i - c)(X_i - c)^T is <= 1e-6 x the largest,
 *   - no candidate is in front of the camera: none of the 64 has sum_i (R X_i + t)_z > 0, or the points lie BEHIND the camera -
 *     the lowest E among the candidates at negative depth is below 0.5 x the lowest in front - 5e-5 trace(Omega).  (Points behind
 *     the camera put the global minimum of E at negative depth and leave only poor local minima in front.  trace(Omega) / 3 is the
 *     mean of E over all rotations; the term keeps the rule away from frames whose pose in front fits to noise or rounding level,
 *     where a coplanar target's mirror twin may come out lower by chance.)  Or
 *   - the result is not finite.
 * The call returns CCAL_OK in all these cases.  n_prob == 0 is allowed (nothing is read or written).  offsets[0] != 0, decreasing
 * offsets, more than 2^24 points in a problem or a NULL required pointer: CCAL_ERR_INVALID_ARG, nothing is launched. */
int ccal_pnp_batch(ccal_ctx* ctx, int n_prob, const int64_t* offsets /* [n_prob + 1] */, const double* xyz /* [.][3] */,
                   const double* xn /* [.][2] */, int min_points, double* poses_out /* [n_prob][6] */, int32_t* n_used_out,
                   double* cost_out /* [n_prob] or NULL */);

/* ---- pose refinement under fixed intrinsics, batched (the ReprojectionFactor of src/optimization/factors.rs:152-173 with its
 * HuberLoss, over rvec | tvec only; what examples/test_pnp.rs needs after its PnP, and what an error on held-out frames needs)
 * n_prob independent frames in one launch, one wavefront each.  Frame i holds the points [offsets[i], offsets[i + 1]) of xyz [.][3]
 * (board points) and uv [.][2] (their detections, pixels); offsets[0] == 0; points with a coordinate that is not finite are left
 * out.  params: the camera's params() vector in the context's conventions (ocv5_order, KB4 small radius); it stays fixed.  For
 * every frame the call minimises, from the pose given in poses_io, the Huber objective
 *     F(rvec, tvec) = sum_i rho(s_i),   s_i = | project(params, R(rvec) X_i + tvec) - uv_i |^2,
 *     rho(s) = s for s <= delta^2, else 2 delta sqrt(s) - delta^2;  rho'(s) = 1, else delta / sqrt(s);  huber_delta <= 0: rho(s) = s,
 * with the Huber corrector of the joint solve: residual and Jacobian rows scaled by sqrt(rho'(s)), so that g below is half the
 * gradient of F.  The cost REPORTED (cost0_out, cost_out) is the library's cost (ccal_report), sum_i rho'(s_i) s_i.  While no corner
 * is beyond delta the two are the same function.  With outliers they are not (delta sqrt(s) per outlier against 2 delta sqrt(s) -
 * delta^2) and their minima differ: steps and stop rules are judged on F, the function the step descends - judged on the reported
 * cost, the iteration would end between the two minima, at a stationary point of neither.  That is the one place where the rule
 * below departs from ccal_solve's LM mode, which judges on the reported cost.  The optimizer is always Levenberg-Marquardt
 * (opts->method is ignored; opts == NULL: the values of ccal_set_defaults), the rule of ccal_solve's LM mode with one state PER
 * FRAME:
 *     radius = lm_initial_radius, dec = 2;  H = J^T J, g = J^T r (corrected rows) at the accepted pose
 *     step:   (H + lambda D) d = -g,  lambda = 1 / radius,  D_ii = clamp(H_ii, lm_min_diagonal, lm_max_diagonal);
 *             model decrease mc = d^T (lambda D d - g);  trial = pose + d;  rho = (F - F_trial) / mc;  iterations += 1
 *     - mc >= 0 and the model decrease (in the error metric) < min_abs_error_decrease or < min_rel_error_decrease x error:
 *       converged - the trial is taken if its F is lower - CCAL_OK
 *     - else mc > 0 and rho > 0: the trial is accepted, radius = min(1e16, radius / max(1/3, 1 - (2 rho - 1)^3)), dec = 2; CCAL_OK
 *       when error < min_error, |error decrease| < min_abs_error_decrease or |error decrease| / last error < min_rel_error_decrease
 *     - else (also: the system is not positive definite, the trial cost is not finite): rejected, radius /= dec, dec *= 2;
 *       radius < 1e-32: CCAL_ERR_NO_CONVERGENCE
 *     - iterations >= max_iterations: CCAL_ERR_NO_CONVERGENCE (the pose is the best accepted one)
 * "error" is F, or its square root with error_metric = CCAL_ERROR_NORM.  A frame stops by its own rule: it neither waits
 * for nor is held up by the other frames of the batch.
 * A corner whose projection is undefined at a pose (not finite: a point at depth 0 for OPENCV5, on the singular cone of UCM / EUCM)
 * has no rule of its own, as in ccal_eval / ccal_solve: its residual makes F and the cost NaN.  At the starting pose that ends the frame
 * with CCAL_ERR_NONFINITE (pose untouched, cost0 = cost = that value); at a trial pose the step is rejected like any other step to
 * a cost that is not finite.
 * Per frame: status_out is CCAL_OK, CCAL_ERR_NO_CONVERGENCE, CCAL_ERR_NONFINITE, CCAL_NO_RESULT (fewer than max(min_points, 3)
 * valid points or a starting pose that is not finite: pose untouched, iterations 0, n_used 0, both costs 0, every err_out row of
 * the frame NaN); CCAL_ERR_NOT_PD belongs to the set of values a caller should expect but the LM rule above turns a failed
 * factorisation into a rejected step.  iters_out = steps tried, n_used_out = valid points, cost0_out / cost_out = the reported
 * cost at the start / at the result; any of these four may be NULL.  err_out [n_points] (or NULL) = | project - uv | in pixels at the result,
 * NaN in the rows of left-out points.  The call returns CCAL_OK in all these cases; n_prob == 0 is allowed (nothing is read or
 * written).  A frame's outputs are a pure function of that frame's inputs: they do not depend on its place in the batch or on the
 * other frames, and are bit-identical from run to run (lane-private sums in f64, one xor-shuffle butterfly, no atomics).
 * The EUCMT container: CCAL_ERR_UNSUPPORTED.  An unknown model, offsets[0] != 0, decreasing offsets, more than 2^24 points in a
 * frame or a NULL required pointer (params, offsets, poses_io, status_out; xyz / uv when there are points): CCAL_ERR_INVALID_ARG.
 * Nothing is launched or written in either case. */
int ccal_refine_poses_batch(ccal_ctx* ctx, int model, const double* params, double huber_delta,
                            int n_prob, const int64_t* offsets /* [n_prob + 1] */,
                            const double* xyz /* [.][3] */, const double* uv /* [.][2] pixels */,
                            int min_points, const ccal_solver_opts* opts /* NULL: defaults */,
                            double* poses_io /* [n_prob][6] in: start, out: result */,
                            int32_t* status_out, int32_t* iters_out, int32_t* n_used_out,
                            double* cost0_out, double* cost_out,      /* [n_prob] each, any may be NULL except status */
                            double* err_out /* [n_points] pixel error at the result, or NULL */);

/* ---- board poses of a rig under fixed intrinsics AND extrinsics, batched (the OtherCamReprojectionFactor of
 * src/optimization/factors.rs:179-228 with its HuberLoss, over rvec_0_b | tvec_0_b only: what a rig's error on held-out frames
 * needs, and examples/test_pnp.rs for a rig) - ccal_refine_poses_batch with the sum taken over every camera that saw the board.
 * n_slots independent frame slots in one launch, one wavefront each.  Slot s owns the segments [seg_offsets[s], seg_offsets[s + 1]);
 * segment j is one camera's observation of the slot: camera seg_cam[j] (0 .. n_cams - 1; a camera may appear more than once) and
 * the points [pt_offsets[j], pt_offsets[j + 1]) of xyz [.][3] (board points) and uv [.][2] (their detections, pixels);
 * seg_offsets[0] == 0, pt_offsets[0] == 0.  model [n_cams], params [n_cams][CCAL_PMAX] (each row a params() vector in the
 * context's conventions: ocv5_order, KB4 small radius) and extr [n_cams][6] (rvec | tvec of T_c_0) stay fixed.  EVERY row of extr
 * is used as given; zeros make that camera the rig frame, as the reference fixes camera 0.  For every slot the call minimises,
 * from the pose T_0_b given in poses_io,
 *     F(rvec, tvec) = sum over the slot's segments j, points i of  rho(s_i),
 *     s_i = | project(params_c, R(rvec_c_0) (R(rvec) X_i + tvec) + tvec_c_0) - uv_i |^2,   c = seg_cam[j],
 * and everything else is, word for word, the rule stated at ccal_refine_poses_batch with "frame" read as "slot" and every sum
 * taken over all the slot's segments: rho and the corrector, the reported cost sum rho'(s_i) s_i against the judged F, the
 * Levenberg-Marquardt rule with one state per slot, points with a coordinate that is not finite left out (NaN in their err_out
 * row), a projection undefined at the start: CCAL_ERR_NONFINITE, the per-slot statuses and outputs, which of them may be NULL,
 * the pure-function and bit-reproducibility statement (the order of summation is that of the slot's own segments).
 * CCAL_NO_RESULT: fewer than max(min_points, 3) valid points OVER ALL CAMERAS of the slot (a slot seen by two cameras with two
 * corners each has a pose at min_points = 4) or a starting pose that is not finite: pose untouched, iterations 0, n_used 0, both
 * costs 0, every err_out row of the slot NaN.  n_slots == 0, a slot without segments and a segment without points are valid.
 * n_cams outside 1 .. CCAL_MAX_CAMS, an unknown model, seg_cam out of range, offsets that do not start at 0 or decrease, more than
 * 2^24 points in a slot or a NULL required pointer (model, params, extr; with n_slots > 0 seg_offsets, poses_io, status_out; seg_cam
 * / pt_offsets when there are segments; xyz / uv when there are points): CCAL_ERR_INVALID_ARG.  An EUCMT camera:
 * CCAL_ERR_UNSUPPORTED.  Nothing is launched or written in either case. */
int ccal_refine_rig_poses_batch(ccal_ctx* ctx, int n_cams, const int32_t* model /* [n_cams] */,
                                const double* params /* [n_cams][CCAL_PMAX] */,
                                const double* extr /* [n_cams][6] rvec|tvec of T_c_0 */,
                                double huber_delta, int n_slots, const int64_t* seg_offsets /* [n_slots + 1] */,
                                const int32_t* seg_cam /* [n_seg] */, const int64_t* pt_offsets /* [n_seg + 1] */,
                                const double* xyz /* [.][3] */, const double* uv /* [.][2] pixels */,
                                int min_points, const ccal_solver_opts* opts /* NULL: defaults */,
                                double* poses_io /* [n_slots][6] T_0_b in: start, out: result */,
                                int32_t* status_out, int32_t* iters_out, int32_t* n_used_out,
                                double* cost0_out, double* cost_out,      /* [n_slots] each, any may be NULL except status */
                                double* err_out /* [n_points] pixel error at the result, or NULL */);

/* ---- initialisation from detections alone (try_init_camera, src/util.rs:107-159) --------------
 * radial_distortion_homography (src/optimization/homography.rs:218-271): RANSAC over a six-point minimal solver for a
 * homography H with one-parameter division distortion lambda between two views of the board, n_hyp (reference: 1 000) random
 * samples scored on ALL pairs (mean distance of evaluate_homography_lambda, :169-216), for n_prob independent problems in one
 * launch.  Problem i holds the pairs [pair_offsets[i], pair_offsets[i + 1]) of `pairs` [.][4] = (x, y, x', y'), NORMALISED
 * (p - (w/2, h/2)) / max(w/2, h/2) (:223-238); pair_offsets[0] == 0; fewer than 6 pairs in any problem: CCAL_ERR_INVALID_ARG,
 * nothing is launched.  Hypothesis h of problem i samples 6 distinct pairs by a partial Fisher-Yates shuffle driven by the
 * counter-based splitmix64 stream (seeds[i] + h * 0xD1B54A32D192ED03; outputs 1..6; draw k: j = k + z_k mod (n - k)) - the
 * reference shuffles with an unseeded generator.  All arithmetic is f64 (the reference: f32).  The winner is the lowest score,
 * ties to the lowest hypothesis index: the outputs are a pure function of (pairs, seed, n_hyp), and hypothesis h does not
 * depend on n_hyp or on what else is in the batch.
 * Per problem: lambda_out [n_prob], H_out [n_prob][9] row-major (scale as the solver leaves it), score_out [n_prob],
 * best_idx_out [n_prob] (winning hypothesis), n_valid_out [n_prob] (hypotheses with an admissible root and a finite score).
 * A problem without one: n_valid 0, best_idx -1, lambda 0, H 0, score +inf (the call still returns CCAL_OK).
 * Optional per-hypothesis outputs (NULL: not wanted): hyp_sample [n_prob][n_hyp][6], hyp_lambda [n_prob][n_hyp],
 * hyp_H [n_prob][n_hyp][9], hyp_score [n_prob][n_hyp] (+inf, lambda 0, H 0 where the solver returned none). */
int ccal_rdh_batch(ccal_ctx* ctx, int n_prob, const int64_t* pair_offsets, const double* pairs, const uint64_t* seeds, int n_hyp,
                   double* lambda_out, double* H_out, double* score_out, int32_t* best_idx_out, int32_t* n_valid_out,
                   int32_t* hyp_sample, double* hyp_lambda, double* hyp_H, double* hyp_score);
/* one problem; CCAL_NO_RESULT when no hypothesis was valid (outputs as above) */
int ccal_radial_distortion_homography(ccal_ctx* ctx, const double* pairs, int n_pairs, uint64_t seed, int n_hyp,
                                      double* lambda_out, double* H_out, double* score_out, int32_t* best_idx_out, int32_t* n_valid_out);
/* homography_to_focal (src/optimization/homography.rs:274-325): focal length in units of the normalisation from H (row-major),
 * CCAL_NO_RESULT (and *f = 0) where the reference returns None.  Host code, no context. */
int ccal_homography_to_focal(const double* H, double* f);
/* init_pose (src/optimization/linear.rs:5-21) for every observation frame of the problem: bearings
 * ((p2d - c) / half) / (1 + lambda r^2) with c = (w/2, h/2), half = max(w/2, h/2) of the frame's camera, then the planar PnP of
 * ccal_init_poses (the same kernel body; corners with 1 + lambda r^2 <= 0 are left out).  Outputs as ccal_init_poses. */
int ccal_init_poses_division(ccal_problem* p, double lambda, int min_points, double* poses_obs, int32_t* n_used);

/* ---- init_camera_extrinsic (src/util.rs:511-561) ------------------------------------------
 * T_i_0 of camera i from the board poses camera 0 and camera i estimated for the same n_common frames:
 * one SE3Factor (src/optimization/factors.rs:234-272) per frame, HuberLoss(0.5), Gauss-Newton from
 * T_i_b[0] * T_0_b[0]^-1 (or from t_i_0_io when use_initial != 0).  A 6-unknown problem: host code of the
 * library, needs no context.  poses_* are [n_common][6] rvec,tvec. */
int ccal_init_camera_extrinsic(const double* poses_cam0, const double* poses_cami, int n_common,
                               double* t_i_0_io, int use_initial, ccal_report* report);
/* the same with the optimizer's stop rules given (max_iterations, min_error, min_abs / min_rel_error_decrease, error_metric);
 * opts == NULL: the defaults, i.e. the call above */
int ccal_init_camera_extrinsic_opts(const double* poses_cam0, const double* poses_cami, int n_common,
                                    double* t_i_0_io, int use_initial, const ccal_solver_opts* opts, ccal_report* report);
/* One SE3Factor block (src/optimization/factors.rs:248-271): r[6] = the rvec,tvec of T_i_b^-1 * (T_i_0 * T_0_b) and its
 * 6 x 6 Jacobian (row-major) with respect to x = rvec,tvec of T_i_0 - what tiny-solver's dual numbers evaluate to. */
int ccal_se3_factor(const double* pose_0_b, const double* pose_i_b, const double* x, double* r_out, double* J_out);

/* ---- convert_model (src/util.rs:224-282) -----------------------------------------------------
 * Fit the target model to the source model over the reference's pixel grid: ModelConvertFactor
 * (src/optimization/factors.rs:10-76) = ONE residual block source.project(ray) - target.project(ray) over the
 * rays the source model unprojects from rows/cols edge = max(w,h)/100 .. in steps of max(w,h)/30, 10000 where a
 * projection is undefined, HuberLoss(1.0) on the whole block; Gauss-Newton on all target intrinsics with the
 * reference's parameter bounds, the last `disabled_distortions` parameters fixed at 0; UCM -> EUCM is the closed
 * form beta = 1 (util.rs:229-235), UCM -> EUCMT the closed form beta = 1, t1 = t2 = 0 (util.rs:236-243).  tgt_params_io: in = the target's current parameters (its first four are
 * replaced by the source's fx, fy, cx, cy: util.rs:256-258), out = the fitted parameters.  opts NULL = the
 * reference's Gauss-Newton defaults.  Rays and the per-iteration Gram run on the device; the <= 9 x 9 solve
 * on the host. */
int ccal_convert_model(ccal_ctx* ctx, int src_model, const double* src_params, int tgt_model,
                       double* tgt_params_io, double width, double height, int disabled_distortions,
                       const ccal_solver_opts* opts, ccal_report* report);

/* ---- applying a calibration: points, undistortion maps, remap ------------------------------------
 * The tail of the reference's examples (examples/convert_model.rs:27-29, examples/test_pnp.rs:51,78-80): model.unproject,
 * estimate_new_camera_matrix_for_undistort, init_undistort_map, remap.  `params` is a params() vector of `model` in the
 * context's conventions (ocv5_order; the KB4 / unprojection small radii apply).  The EUCMT container: CCAL_ERR_UNSUPPORTED.
 *
 * ccal_project_points    GenericModel::project: xyz [n][3] -> uv_out [n][2], valid_out [n] (1 where project is defined: in front
 *                        of the UCM / EUCM cone, a non-zero KB4 point, z > 1e-9 for OPENCV5); invalid rows are NaN, NaN.
 * ccal_unproject_points  GenericModel::unproject: uv [n][2] -> rays_out [n][3] (a unit ray; (mx, my, 1) below KB4's small
 *                        radius), valid_out [n]; invalid rows are NaN.  n == 0 is allowed in both.
 *                        THE CONTRACT of every unprojection of this library (this call, the new camera matrix, the renderer,
 *                        ccal_convert_model's rays, pose initialisation): valid means the ray re-projects onto the pixel under
 *                        the acceptance rule, None otherwise.  The rule: the iterative inverses (KB4's Newton, OPENCV5's fixed
 *                        point) accept their last iterate only if its residual is below 1e-9 in normalised image units; the
 *                        closed form (UCM, EUCM) only inside its domain and where its denominator and the ray's norm are
 *                        positive finite numbers (alpha = 1 on the domain's edge is None).  A pixel that has a ray which the
 *                        published iteration does not find from its start is None as well.
 * ccal_estimate_new_camera_matrix
 *                        the pinhole K_out [9] (row-major [[f,0,cx],[0,f,cy],[0,0,1]]) whose new_w x new_h image (0, 0: width x
 *                        height) holds the rays of the four edge midpoints (cx,0), (W-1,cy), (cx,H-1), (0,cy) of the model:
 *                        with x/z, y/z of their unprojections, min_x = |min x/z|, max_x = max x/z (y alike),
 *                        cx' = new_w min_x / (min_x + max_x), f = balance max(new_w / (min_x + max_x), new_h / (min_y + max_y))
 *                        + (1 - balance) min(the same two).  balance outside [0, 1]: CCAL_ERR_INVALID_ARG.  A midpoint that
 *                        cannot be unprojected or has z <= 0: CCAL_NO_RESULT.
 * ccal_undistort_map_*   a device-resident pair of f32 maps [new_h][new_w]: for output pixel (x, y) the source pixel
 *                        project(R^T ((x - cx) / fx, (y - cy) / fy, 1)) of K = [[fx,0,cx],[0,fy,cy],[0,0,1]] (row-major; R
 *                        row-major, NULL = identity), NaN, NaN where project is undefined.  _from_host: any caller-made maps.
 *                        A map holds its context like a problem does.  At most 2^31 - 1 pixels.
 * ccal_remap / _dev      bilinear resampling of n_img interleaved images [n_img][src_h][src_w][channels] of one size through
 *                        the map into [n_img][new_h][new_w][channels]; (dtype, channels) = (CCAL_PIX_U8, 1), (CCAL_PIX_U8, 3)
 *                        or (CCAL_PIX_U16, 1).  A map entry (mx, my) is valid iff both are finite, 0 <= mx <= src_w - 1 and
 *                        0 <= my <= src_h - 1 (-0.0 counts as 0); an invalid entry writes 0 in every channel.  Valid, in f32:
 *                        x0 = floor(mx), ax = mx - x0, x1 = min(x0 + 1, src_w - 1), y alike,
 *                        val = (1 - ay) ((1 - ax) p00 + ax p01) + ay ((1 - ax) p10 + ax p11), output floorf(val + 0.5f)
 *                        clamped to the type's range.  ccal_remap: host pointers, returns when dst is written.
 *                        ccal_remap_dev: device pointers, only enqueues on the context's stream (ccal_sync waits). */
typedef struct ccal_undistort_map ccal_undistort_map;
typedef enum { CCAL_PIX_U8 = 0, CCAL_PIX_U16 = 1 } ccal_pixel_type;
int ccal_project_points(ccal_ctx* ctx, int model, const double* params, int64_t n, const double* xyz, double* uv_out, uint8_t* valid_out);
int ccal_unproject_points(ccal_ctx* ctx, int model, const double* params, int64_t n, const double* uv, double* rays_out, uint8_t* valid_out);
int ccal_estimate_new_camera_matrix(ccal_ctx* ctx, int model, const double* params, int width, int height, double balance,
                                    int new_w, int new_h, double* K_out /* [9] */);
int ccal_undistort_map_create(ccal_ctx* ctx, int model, const double* params, const double* K /* [9] */, const double* R /* [9] or NULL */,
                              int new_w, int new_h, ccal_undistort_map** out);
int ccal_undistort_map_from_host(ccal_ctx* ctx, const float* xmap, const float* ymap, int w, int h, ccal_undistort_map** out);
int ccal_undistort_map_download(ccal_undistort_map* map, float* xmap_out, float* ymap_out);
void ccal_undistort_map_destroy(ccal_undistort_map* map);
int ccal_remap(ccal_undistort_map* map, int dtype, int channels, int src_w, int src_h, int n_img, const void* src, void* dst);
int ccal_remap_dev(ccal_undistort_map* map, int dtype, int channels, int src_w, int src_h, int n_img, const void* src_dev, void* dst_dev);

/* ---- from pixels to detections: sub-pixel refinement of coarse corners ------------------------------
 * The last step of every target detector (what load_feature_data's image_to_option_feature_frame ends with, src/data_loader.rs:36-70;
 * the detector itself lives in the absent aprilgrid crate and is NOT here): each coarse corner is moved onto the grey-level saddle
 * by the gradient-orthogonality fit below.  The rule is this project's; tests/corner_ref.py is its f64 yardstick.
 *
 * Images: n_img single-channel images of one size, [n_img][height][width] of CCAL_PIX_U8 or CCAL_PIX_U16; a pixel's centre is at
 * integer coordinates, as in ccal_remap.  Image k owns the corners [offsets[k], offsets[k + 1]) of xy_io [.][2] = (x, y).
 * I(x, y) is ccal_remap's bilinear sample, in f64 (no f32 anywhere): x0 = floor(x), ax = x - x0, x1 = min(x0 + 1, width - 1), y alike,
 *     top = p00 + ax (p01 - p00), bot = p10 + ax (p11 - p10), I = top + ay (bot - top)
 * - the same interpolant written in differences, so that a constant neighbourhood samples to EXACTLY its value and two equal rows
 * to exactly equal values whatever the fractions are: a flat patch has all sums 0 and an axis-parallel edge b = 0 and a or d = 0, not
 * rounding noise that the relative degenerate test below would have to judge.
 * For a corner with start c0, h = half_win and c = c0, repeat:
 *   inside      c.x >= h + 1, c.x <= width - 2 - h, c.y >= h + 1, c.y <= height - 2 - h (the patch lies in the image; the four
 *               comparisons are exact, their right sides are integers) and both finite; else the corner ends CCAL_NO_RESULT, position c0.
 *   patch       P(i, j) = I(c.x + i, c.y + j), i, j in [-h-1, h+1]; gx(i, j) = P(i+1, j) - P(i-1, j), gy(i, j) = P(i, j+1) - P(i, j-1)
 *               for i, j in [-h, h] (no factor 1/2: it cancels).
 *   weights     w(i, j) = w1(i) w1(j), w1(i) = exp(-(i / h)^2).
 *   sums        over the window: a = sum w gx^2, b = sum w gx gy, d = sum w gy^2, u = sum w (gx^2 i + gx gy j),
 *               v = sum w (gx gy i + gy^2 j); det = a d - b^2.
 *   degenerate  !(det > 1e-12 (a + d)^2) - a flat patch, a single edge, sums that are not finite: CCAL_ERR_NOT_PD, position c0.
 *   update      delta = ((d u - b v) / det, (a v - b u) / det); c += delta; iterations += 1; e = sqrt(delta.x^2 + delta.y^2).
 *   stop        e <= eps: CCAL_OK.  Else iterations >= max_iterations: CCAL_ERR_NO_CONVERGENCE, the position is the last iterate.
 * After a stop by either rule, the drift test: |c.x - c0.x| > h or |c.y - c0.y| > h (the window slid off the corner it was
 * given): CCAL_NO_RESULT, position c0.
 * Per corner: xy_io (the position), status_out, iters_out (updates made; NULL: not wanted), lambda_min_out (NULL: not wanted) = the
 * smaller eigenvalue ((a + d) - sqrt((a - d)^2 + 4 b^2)) / 2 of [[a, b], [b, d]] divided by (sum_i w1(i))^2, at the LAST EVALUATED
 * iterate - NaN when none was evaluated (the start was not inside).  It is a corner-strength figure a caller can threshold; it
 * scales with the square of the image contrast.
 * A corner's outputs are a pure function of its image, its start and (half_win, max_iterations, eps): they do not depend on its
 * place in the batch or on what else is in it, and they are bit-identical from run to run (a fixed lane-to-pixel mapping,
 * lane-private sums, one xor butterfly, no atomics).
 * ccal_refine_corners_batch: host pointers.  ccal_refine_corners_dev: `images_dev` is a device pointer (the output of
 * ccal_remap_dev on this context's stream, or a block whose writes are complete); corners and outputs stay host arrays.  Both
 * return when the outputs are written.
 * CCAL_ERR_INVALID_ARG, nothing launched or written: half_win outside 1 .. 15, max_iterations < 1, eps < 0 or not finite, a dtype
 * other than the two, width, height <= 0 or n_img < 0, more than 2^31 - 1 pixels in an image or corners in the call, offsets that
 * do not start at 0 or decrease, a NULL required pointer (with n_img > 0: images, offsets, status_out; xy_io when there are
 * corners).  n_img == 0 and an image without corners are valid. */
int ccal_refine_corners_batch(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images,
                              const int64_t* offsets /* [n_img + 1] */, double* xy_io /* [.][2] in: start, out: result */,
                              int half_win, int max_iterations, double eps,
                              int32_t* status_out, int32_t* iters_out /* or NULL */, double* lambda_min_out /* or NULL */);
int ccal_refine_corners_dev(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images_dev,
                            const int64_t* offsets /* [n_img + 1] */, double* xy_io /* [.][2] */,
                            int half_win, int max_iterations, double eps,
                            int32_t* status_out, int32_t* iters_out /* or NULL */, double* lambda_min_out /* or NULL */);

/* ---- from pixels to detections: checkerboard-corner candidates of whole images (saddle detector) ------------------------------
 * The step in front of the refinement above: every image of a batch searched for grey-level saddles (the inner corners of a
 * checkerboard), in INTEGER arithmetic throughout - the outputs are decisions, and tests/detect_ref.py, the numpy int64
 * yardstick, is met bit for bit.  The rule is this project's (the determinant-of-Hessian saddle response the checkerboard
 * detectors of OpenCV and Kalibr also start from); tags are not decoded here.
 *
 * Images: as above - n_img single-channel images of one size, [n_img][height][width] of CCAL_PIX_U8 or CCAL_PIX_U16, a pixel's
 * centre at integer coordinates, I(x, y) the pixel value.  Parameters: step s in 1 .. 4, nms_radius r in 1 .. 15,
 * min_response >= 1, rel_q10 in 0 .. 1024, cap >= 1.
 *   smooth      S(x, y) = sum over i, j in -2 .. 2 of b(i) b(j) I(x + i, y + j), b = [1, 4, 6, 4, 1]: an integer, no division;
 *               S <= 256 * 65535 < 2^24.
 *   Hessian     hxx = S(x+s, y) - 2 S(x, y) + S(x-s, y), hyy = S(x, y+s) - 2 S(x, y) + S(x, y-s),
 *               hxy = S(x+s, y+s) - S(x+s, y-s) - S(x-s, y+s) + S(x-s, y-s): int32, |hxx|, |hyy|, |hxy| <= 2 * 2^24 = 2^25.
 *   response    R = hxy^2 - 16 hxx hyy in int64: -16 s^4 det H of a quadratic, positive at a saddle, and the same for the
 *               saddles xy and (x^2 - y^2) / 2 (a rotation by 45 degrees).  |R| <= 2^50 + 16 * 2^50 < 2^55: it cannot overflow.
 *   domain      the pixels with s + 2 <= x <= width - 1 - (s + 2) and s + 2 <= y <= height - 1 - (s + 2) - every pixel R reads
 *               lies in the image.  An image too small to have one is valid and yields nothing.
 *   local max   p in the domain with R(p) >= min_response such that for every domain pixel q != p with |q.x - p.x| <= r and
 *               |q.y - p.y| <= r: R(p) > R(q) if q precedes p in row-major order (q.y < p.y, or q.y == p.y and q.x < p.x),
 *               R(p) >= R(q) otherwise.  Pixels outside the domain do not compete.  (Of equal neighbours the first in row-major
 *               order wins, so two local maxima are never within r of each other in both coordinates.)
 *   threshold   Rmax = the largest R over the image's domain.  With Rmax > 0: T = max(min_response, (Rmax >> 10) * rel_q10); a
 *               candidate is a local maximum with R >= T.  With Rmax <= 0 there is no local maximum and no candidate.
 * Outputs per image k, the candidates in row-major order of (y, x): count_out[k] = their number - it may exceed cap, then the
 * first cap in that order are stored -, xy_out [n_img][cap][2] = (x, y), hess_out [n_img][cap][3] = (hxx, hyy, hxy),
 * response_out [n_img][cap] = R (NULL: not wanted).  Rows past min(count, cap) are not written.
 * min_response scales with the square of the image contrast (R is quadratic in the grey levels), like lambda_min above; no
 * useful value has been measured.  1 screens flat neighbourhoods and axis-parallel edges (R = 0 exactly there); an oblique
 * straight edge leaves a positive residue of the differences, which rel_q10 has to cut.
 * An image's outputs are a pure function of that image and (step, nms_radius, min_response, rel_q10, cap): they do not depend
 * on its place in the batch, on what else is in it or on how the library cuts the batch into chunks, and they are bit-identical
 * from run to run (integers only, Rmax by an integer max, a candidate's place fixed by its position: no arrival order anywhere).
 * ccal_detect_corners_batch: host pointers.  ccal_detect_corners_dev: `images_dev` is a device pointer (the output of
 * ccal_remap_dev on this context's stream, or a block whose writes are complete); the outputs stay host arrays.  Both return
 * when the outputs are written.
 * CCAL_ERR_INVALID_ARG, nothing launched or written: step outside 1 .. 4, nms_radius outside 1 .. 15, min_response < 1, rel_q10
 * outside 0 .. 1024, cap < 1, a dtype other than the two, width, height <= 0 or n_img < 0, more than 2^31 - 1 pixels in an image,
 * a NULL required pointer (with n_img > 0: images, count_out, xy_out, hess_out).  n_img == 0 is valid. */
int ccal_detect_corners_batch(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images,
                              int step, int nms_radius, int64_t min_response, int rel_q10, int cap,
                              int32_t* count_out /* [n_img] */, int32_t* xy_out /* [n_img][cap][2] */,
                              int32_t* hess_out /* [n_img][cap][3] */, int64_t* response_out /* [n_img][cap] or NULL */);
int ccal_detect_corners_dev(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images_dev,
                            int step, int nms_radius, int64_t min_response, int rel_q10, int cap,
                            int32_t* count_out /* [n_img] */, int32_t* xy_out /* [n_img][cap][2] */,
                            int32_t* hess_out /* [n_img][cap][3] */, int64_t* response_out /* [n_img][cap] or NULL */);

/* ---- from pixels to detections: decoding tags in candidate quads (batched quad sampling and code match) -----------------------
 * What the reference's front end does before it names corners (image_to_option_feature_frame, src/data_loader.rs:36-70: corner
 * id = tag_id * 4 + i, looked up in Board::init_aprilgrid, src/board.rs:46-95): given an image and a candidate quad, decide which
 * tag of a family this is, how it is turned and by how many bits it misses.  Quads are NOT proposed here (ccal_propose_quads_* below
 * does that for AprilGrids).  The rule is this
 * project's; the reference's decoder lives in the absent aprilgrid crate, so parity with it is NOT pinned.  A family is data - a
 * bit count and a list of codes - and the caller supplies it (from the library that printed the board); none is built in.
 * tests/tag_ref.py is the rule's numpy f64 yardstick; the library evaluates the rule without fused multiply-adds, each product
 * and sum rounded on its own.
 *
 * Images: as for ccal_refine_corners_* - [n_img][height][width] of CCAL_PIX_U8 / CCAL_PIX_U16, a pixel's centre at integer
 * coordinates, I(x, y) that section's bilinear f64 sample written in differences.  Image k owns the quads
 * [offsets[k], offsets[k + 1]) of quads [.][4][2] = (x, y); a quad's corners q0 .. q3 go around the tag's OUTER border edge in
 * order.  Family: d in 3 .. 8 data cells per side, n_codes >= 1 codes, each < 2^(d d).  Parameters: border in 1 .. 2 (black cells
 * around the data), samples S in 1 .. 4, min_contrast >= 0 and finite, max_border_errors >= 0, max_hamming in 0 .. d d.
 * n = d + 2 border (at most 12) cells per side.
 *   1 map        the unit square onto the quad, (0,0) -> q0, (1,0) -> q1, (1,1) -> q2, (0,1) -> q3, q_i = (x_i, y_i):
 *                S_ = q0 - q1 + q2 - q3, D1 = q1 - q2, D2 = q3 - q2, den = D1.x D2.y - D2.x D1.y,
 *                g = (S_.x D2.y - D2.x S_.y) / den, h = (D1.x S_.y - S_.x D1.y) / den,
 *                a = x1 - x0 + g x1, b = x3 - x0 + h x3, c = x0, d_ = y1 - y0 + g y1, e = y3 - y0 + h y3, f = y0,
 *                w = g u + h v + 1, x = (a u + b v + c) / w, y = (d_ u + e v + f) / w.
 *   2 cells      cell (row j, col i), i, j in 0 .. n - 1, has S S sample points at u = (i + (2p + 1) / (2S)) / n,
 *                v = (j + (2q + 1) / (2S)) / n; its value is the mean of I over them (summed q outer, p inner, divided by S S).
 *   3 inside     every sample point has w finite and > 0, 0 <= x <= width - 1 and 0 <= y <= height - 1 (false for NaN); else
 *                CCAL_TAG_OUTSIDE.  This also catches den == 0, corners that are not finite and crossed quads.
 *   4 threshold  lo, hi = the smallest and largest cell value over all n n cells.  !(hi - lo >= min_contrast):
 *                CCAL_TAG_LOW_CONTRAST.  t = lo + (hi - lo) / 2; a cell is white (1) iff its value > t;
 *                margin = min over the cells of |value - t|.
 *   5 border     the white cells among the n n - d d border cells; more than max_border_errors: CCAL_TAG_BORDER.
 *   6 code       data cell (r, c) = cell (border + r, border + c): code = sum bit(r, c) << (d d - 1 - (r d + c)) - row-major from
 *                q0's corner, the first cell in the highest bit.
 *   7 turns      T(B)(r, c) = B(d - 1 - c, r) is one quarter turn clockwise; code_k is the code of T^k(B), k = 0 .. 3.
 *   8 match      over all (m, k) the smallest key (popcount(code_k ^ codes[m]), m, k) in lexicographic order.  Its distance
 *                above max_hamming: CCAL_TAG_NO_CODE.  Else CCAL_TAG_OK with id = m, rot = k, hamming.
 *   9 corners    canonical corner i is the outer corner of the printed tag at the code image's top-left, top-right,
 *                bottom-right, bottom-left for i = 0 .. 3: corners_out[i] = q[(i + 3 rot) mod 4].
 * Outputs per quad: reason_out; id_out, rot_out, hamming_out (-1 unless CCAL_TAG_OK); corners_out [.][4][2] (NaN unless
 * CCAL_TAG_OK; NULL: not wanted); code_out = code_0 (written for every reason past CCAL_TAG_LOW_CONTRAST, 0 otherwise; NULL: not
 * wanted); margin_out (NaN for CCAL_TAG_OUTSIDE; NULL: not wanted).
 * A quad's outputs are a pure function of its image, its corners, the family and the parameters: they do not depend on its place
 * in the batch, on what else is in it or on how the library cuts the batch into chunks, and they are bit-identical from run to
 * run (a fixed lane-to-cell mapping, lo / hi / margin by exact min / max, the match by the minimum of an integer key, no atomics).
 * ccal_decode_tags_batch: host pointers.  ccal_decode_tags_dev: `images_dev` is a device pointer (the output of ccal_remap_dev
 * on this context's stream, or a block whose writes are complete); everything else stays a host array.  Both return when the
 * outputs are written.
 * CCAL_ERR_INVALID_ARG, nothing launched or written: a parameter outside the ranges above, a code >= 2^(d d) (d d < 64 only), a
 * dtype other than the two, width, height <= 0 or n_img < 0, more than 2^31 - 1 pixels in an image or quads in the call, offsets
 * that do not start at 0 or decrease, a NULL required pointer (with n_img > 0: images, offsets, codes, reason_out, id_out,
 * rot_out, hamming_out; quads when there are quads).  n_img == 0 and an image without quads are valid. */
typedef enum {
    CCAL_TAG_OK = 0,
    CCAL_TAG_OUTSIDE = 1,
    CCAL_TAG_LOW_CONTRAST = 2,
    CCAL_TAG_BORDER = 3,
    CCAL_TAG_NO_CODE = 4
} ccal_tag_reason;
int ccal_decode_tags_batch(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images,
                           const int64_t* offsets /* [n_img + 1] */, const double* quads /* [.][4][2] */, int d, int border,
                           const uint64_t* codes /* [n_codes] */, int n_codes, int samples, double min_contrast,
                           int max_border_errors, int max_hamming,
                           int32_t* reason_out, int32_t* id_out, int32_t* rot_out, int32_t* hamming_out,
                           double* corners_out /* [.][4][2] or NULL */, uint64_t* code_out /* or NULL */, double* margin_out /* or NULL */);
int ccal_decode_tags_dev(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images_dev,
                         const int64_t* offsets /* [n_img + 1] */, const double* quads /* [.][4][2] */, int d, int border,
                         const uint64_t* codes /* [n_codes] */, int n_codes, int samples, double min_contrast,
                         int max_border_errors, int max_hamming,
                         int32_t* reason_out, int32_t* id_out, int32_t* rot_out, int32_t* hamming_out,
                         double* corners_out /* [.][4][2] or NULL */, uint64_t* code_out /* or NULL */, double* margin_out /* or NULL */);

/* ---- from pixels to detections: proposing AprilGrid tag quads from corner candidates ------------------------------------------
 * The step between the refinement and the decoder above: the refined saddle points of an image grouped into candidate tag
 * outlines, which go straight into ccal_decode_tags_*.  It rests on the geometry of an AprilGrid (tags with black gap squares at
 * their corners): a tag's four outer corners are saddles - the black border cell meets the black gap square diagonally -, and
 * along each outer edge the inside is the black border ring and the outside the white gap strip, for the whole length of the
 * edge.  Plain AprilTags without gap squares are not served.  The rule is this project's (what the absent aprilgrid crate does in
 * its place is not pinned); tests/quad_ref.py is its numpy f64 yardstick, and the library evaluates it without fused
 * multiply-adds, each product and sum rounded on its own, so the yardstick is met exactly.
 *
 * Images: as in the three sections above - [n_img][height][width] of CCAL_PIX_U8 / CCAL_PIX_U16, a pixel's centre at integer
 * coordinates, I(x, y) the bilinear f64 sample written in differences of ccal_refine_corners_*.  Image k owns the points
 * [offsets[k], offsets[k + 1]) of xy [.][2] = (x, y), f64: the refined candidates, in any order; indices below are local to the image.
 * Parameters: min_side >= 1 (px; 20 is a useful default), max_side >= min_side (120; half the larger image side in the Python
 * layers), max_side_ratio >= 1 (2), 0 < offset <= 0.25 (1 / (2 (d + 2 border)) - half a cell - for a family of d x d bits; 1/16
 * for a 36-bit family with one border cell), samples K in 1 .. 16 (8), min_contrast >= 0 and finite, in grey levels of the dtype
 * (40 for 8-bit images), cap >= 1.  At offset = 1/8 the inner samples of such a family sit on the boundary between the border
 * ring and the data cells, and the rendered fixture of the tests loses tags: keep the samples in the middle of the ring.
 *   1 edge       the directed pair A -> B, A != B: e = B - A, L2 = e.x e.x + e.y e.y; min_side^2 <= L2 <= max_side^2, else no edge.
 *                n = (-offset * e.y, offset * e.x): the inward offset vector - with y pointing down it points to the right of the
 *                walk from A to B; no square root.  For k = 0 .. K - 1: t = (k + 1) / (K + 1), p = (A.x + t e.x, A.y + t e.y),
 *                in_k = I(p + n), out_k = I(p - n).  All 2 K sample points satisfy 0 <= x <= width - 1 and 0 <= y <= height - 1
 *                (false for NaN), else no edge.  dark = max in_k, bright = min out_k: an edge iff bright - dark >= min_contrast.
 *   2 lists      out(A) = the B with an edge A -> B in increasing index order, cut to the first CCAL_QUAD_MAX_OUT_EDGES.  If any
 *                list of an image is cut, bit 0 of that image's flags_out is set: proposals may then be missing.
 *   3 quads      (A, B, C, D) with B in out(A), C in out(B), D in out(C), A in out(D); all four distinct; A the smallest index
 *                (each outline appears once); strictly convex and clockwise in image coordinates: with e1 = B - A, e2 = C - B,
 *                e3 = D - C, e4 = A - D the cross products u.x v.y - u.y v.x of (e1, e2), (e2, e3), (e3, e4), (e4, e1) are all
 *                > 0; and the largest squared side <= max_side_ratio^2 times the smallest.
 * Outputs per image k, the quads in lexicographic order of (A, B, C, D): count_out[k] = their number - it may exceed cap, then the
 * first cap in that order are stored -, idx_out [n_img][cap][4] = the corner indices, quads_out [n_img][cap][4][2] = the corners'
 * coordinates, bit-equal to the input points (NULL: not wanted), flags_out[k].  Rows past min(count, cap) are not written.
 * A proposed quad starts at whichever of its corners has the smallest index; ccal_decode_tags_* names the turn.
 * An image's outputs are a pure function of that image, its points and the parameters: they do not depend on its place in the
 * batch, on what else is in it, on how the library cuts the batch into chunks or on the run (no atomics; a point's out-edges and
 * an image's quads are compacted by ballot and prefix in index order).
 * ccal_propose_quads_batch: host pointers.  ccal_propose_quads_dev: `images_dev` is a device pointer (the output of ccal_remap_dev
 * on this context's stream, or a block whose writes are complete); everything else stays a host array.  Both return when the
 * outputs are written.
 * CCAL_ERR_INVALID_ARG, nothing launched or written: a parameter outside the ranges above, a dtype other than the two, width,
 * height <= 0 or n_img < 0, more than 2^31 - 1 pixels in an image, offsets that do not start at 0 or decrease, more than 32768
 * points in one image (the pair search is quadratic) or 2^31 - 1 in the call, a NULL required pointer (with n_img > 0: images,
 * offsets, count_out, flags_out, idx_out; xy when there are points).  n_img == 0 and an image without points are valid. */
#define CCAL_QUAD_MAX_OUT_EDGES 8
int ccal_propose_quads_batch(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images,
                             const int64_t* offsets /* [n_img + 1] */, const double* xy /* [.][2] */,
                             double min_side, double max_side, double max_side_ratio, double offset, int samples, double min_contrast,
                             int cap, int32_t* count_out /* [n_img] */, int32_t* flags_out /* [n_img] */,
                             int32_t* idx_out /* [n_img][cap][4] */, double* quads_out /* [n_img][cap][4][2] or NULL */);
int ccal_propose_quads_dev(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images_dev,
                           const int64_t* offsets /* [n_img + 1] */, const double* xy /* [.][2] */,
                           double min_side, double max_side, double max_side_ratio, double offset, int samples, double min_contrast,
                           int cap, int32_t* count_out /* [n_img] */, int32_t* flags_out /* [n_img] */,
                           int32_t* idx_out /* [n_img][cap][4] */, double* quads_out /* [n_img][cap][4][2] or NULL */);

/* ---- from pixels to detections: AprilGrid tags from images in one call ------------------------------------------------------------
 * What the reference does per image in one function (image_to_option_feature_frame, src/data_loader.rs:36-70), up to the tags: the
 * four sections above chained on the device - the image block is uploaded once per chunk (not at all by the _dev form) and no
 * per-point or per-quad array comes back before the tags.  Looking the corners up on a board (id * 4 + i, MIN_CORNERS) stays with
 * the caller.  The rule composes the four rules above by reference and adds only the links; tests/tagchain_ref.py is its numpy
 * yardstick, and the four calls above with the links done on the host give the same bits.
 *
 * Images: as above - [n_img][height][width] of CCAL_PIX_U8 / CCAL_PIX_U16.  Family: d, codes, n_codes as for ccal_decode_tags_*.
 * Options: every field of ccal_detect_tags_opts is named after the stage parameter it feeds and has that parameter's range; there
 * are no defaults (the Python layer's: step 1, nms_radius 5, min_response 1, rel_q10 102, cand_cap 4096; half_win 4,
 * max_iterations 30, eps 1e-3; merge_radius 1; min_side 20, max_side half the larger image side, max_side_ratio 2, offset
 * 1 / (2 (d + 2 border)), edge_samples 8, edge_min_contrast 40, quad_cap 1024; border 1, cell_samples 3, tag_min_contrast 40,
 * max_border_errors 0, max_hamming 2).  Per image:
 *   1 candidates  ccal_detect_corners_* with (step, nms_radius, min_response, rel_q10): the stored candidates are the first
 *                 min(count, cand_cap) in row-major order.
 *   2 starts      the integer (x, y) of each stored candidate as f64.
 *   3 refine      ccal_refine_corners_* with (half_win, max_iterations, eps) on those starts; only corners with status CCAL_OK go on,
 *                 in candidate order.
 *   4 round       each coordinate through f32 (round to nearest even) and back to f64: the f32 a FeaturePoint holds.
 *   5 merge       the points in that order; a point is dropped if |dx| <= merge_radius and |dy| <= merge_radius against a point
 *                 KEPT before it (a dropped point screens nothing).  The difference of two f32 values is exact in f64: no rounding
 *                 enters the test.
 *   6 propose     ccal_propose_quads_* with (min_side, max_side, max_side_ratio, offset, edge_samples, edge_min_contrast) on the kept
 *                 points: the stored quads are the first min(count, quad_cap) in its lexicographic order.
 *   7 decode      ccal_decode_tags_* with (border, cell_samples, tag_min_contrast, max_border_errors, max_hamming) on every stored quad.
 *   8 select      among the image's CCAL_TAG_OK quads each id keeps the quad with the smallest (hamming, -margin); on an exact tie
 *                 the quad earlier in the proposer's order.  The tags are listed in ascending id.
 * Outputs per image k: count_out[k] = the number of distinct ids - it may exceed tag_cap, then the first tag_cap are stored -,
 * id_out, rot_out, hamming_out [n_img][tag_cap], corners_out [n_img][tag_cap][4][2] in the decoder's canonical order, margin_out
 * [n_img][tag_cap] (NULL: not wanted), flags_out[k] (bit 0: the proposer's cut-list bit; bit 1: more candidates than cand_cap;
 * bit 2: more quads than quad_cap; bit 3: more tags than tag_cap), stats_out [n_img][4] (NULL: not wanted) = candidates found,
 * points after the merge, quads found, CCAL_TAG_OK quads before the selection.  Rows past min(count, tag_cap) are not written.
 * An image's outputs are a pure function of that image, the family and the options: they do not depend on its place in the batch,
 * on what else is in it, on how the library cuts the batch into chunks or on the run.  The links use no atomics; every order is an
 * index order (the merge walks the candidates one by one, the selection compares every pair, the scans are prefix sums).
 * ccal_detect_tags_batch: host pointers.  ccal_detect_tags_dev: `images_dev` is a device pointer (the output of ccal_remap_dev on
 * this context's stream, or a block whose writes are complete); everything else stays a host array.  Both return when the outputs
 * are written.
 * CCAL_ERR_INVALID_ARG, nothing launched or written: opts NULL, a field outside its stage's range, merge_radius negative or not
 * finite, cand_cap outside 1 .. 32768 (the proposer's point limit), quad_cap or tag_cap < 1, a code >= 2^(d d) (d d < 64 only), a
 * dtype other than the two, width, height <= 0 or n_img < 0, more than 2^31 - 1 pixels in an image, a NULL required pointer (with
 * n_img > 0: images, codes, count_out, id_out, rot_out, hamming_out, corners_out, flags_out).  n_img == 0 is valid. */
typedef struct {
    /* detector */
    int32_t step, nms_radius;
    int64_t min_response;
    int32_t rel_q10, cand_cap;
    /* refinement */
    int32_t half_win, max_iterations;
    double eps;
    /* merge */
    double merge_radius;
    /* proposer */
    double min_side, max_side, max_side_ratio, offset, edge_min_contrast;
    int32_t edge_samples, quad_cap;
    /* decoder */
    int32_t border, cell_samples;
    double tag_min_contrast;
    int32_t max_border_errors, max_hamming;
    /* output */
    int32_t tag_cap, reserved_;
} ccal_detect_tags_opts;
int ccal_detect_tags_batch(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images,
                           int d, const uint64_t* codes /* [n_codes] */, int n_codes, const ccal_detect_tags_opts* opts,
                           int32_t* count_out /* [n_img] */, int32_t* id_out, int32_t* rot_out, int32_t* hamming_out /* [n_img][tag_cap] */,
                           double* corners_out /* [n_img][tag_cap][4][2] */, double* margin_out /* [n_img][tag_cap] or NULL */,
                           int32_t* flags_out /* [n_img] */, int32_t* stats_out /* [n_img][4] or NULL */);
int ccal_detect_tags_dev(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images_dev,
                         int d, const uint64_t* codes /* [n_codes] */, int n_codes, const ccal_detect_tags_opts* opts,
                         int32_t* count_out /* [n_img] */, int32_t* id_out, int32_t* rot_out, int32_t* hamming_out /* [n_img][tag_cap] */,
                         double* corners_out /* [n_img][tag_cap][4][2] */, double* margin_out /* [n_img][tag_cap] or NULL */,
                         int32_t* flags_out /* [n_img] */, int32_t* stats_out /* [n_img][4] or NULL */);

/* ---- from pixels to detections: a complete checkerboard from corner candidates ----------------------------------------------------
 * The corner candidates of an image - refined positions and the detector's Hessians - ordered into a plain checkerboard of
 * cols x rows inner corners, all images of a batch at once; and the chain from images to boards in one device-resident call.
 * tests/board_ref.py is the numpy f64 yardstick of the rule below; the board unit is compiled without fused multiply-adds, and its
 * outputs equal the yardstick's to the bit.  Every operation is an IEEE f64 + - * / or sqrt, rounded on its own, in the order
 * written; |v| of a 2-vector is sqrt(vx vx + vy vy).
 *
 * Limits: cols, rows in CCAL_BOARD_MIN_SIDE .. CCAL_BOARD_MAX_SIDE (2 .. 20); at most CCAL_BOARD_MAX_ROWS (4096) input rows per
 * image; at most CCAL_BOARD_MAX_KEPT (512) rows kept after the screen - an image over that limit gets flag bit 1
 * (CCAL_BOARD_FLAG_KEPT_LIMIT) and no board, never a partial result.  Positions must be small enough that the squares of their
 * differences do not overflow.
 *
 * Per image, rows i = 0 .. m - 1 of (x, y) and (hxx, hyy, hxy) - hxy is four times the mixed derivative, as the detector stores it:
 *   1 screen   R = hxy hxy - (16 hxx) hyy.  A row is usable when x, y and R are finite and R > 0.  Fewer than cols * rows
 *              usable rows: no board, 0 rows kept.  Rank the usable rows by (R descending, i ascending); t = 0.5 R of the row of rank
 *              cols rows - 1; the usable rows with R >= t are kept.
 *   2 order    the n kept rows sorted by (y, x, i) ascending: the slots 0 .. n - 1 everything below speaks of.
 *   3 edges    per slot b = hxy / 4, mu = 0.5 (hxx + hyy), dl = 0.5 (hxx - hyy), r = sqrt(dl dl + b b), l1 = mu + r, l0 = mu - r;
 *              v = (dl + r, b) when dl >= 0, else (b, r - dl); v = v / |v| ((1, 0) when |v| is not > 0); w = (-vy, vx);
 *              A = sqrt(max(l1, 0)), B = sqrt(max(-l0, 0)); d1 = B v + A w, d2 = B v + (-A) w, each divided by max(|d|, 1e-300):
 *              the two zero-curvature directions of [[hxx, b], [b, hyy]].  The four directions of a slot are d1, d2, -d1, -d2.
 *   4 links    for slots a != b: e = P[b] - P[a], dist = |e|, u = e / dist; cos(a, k, b) = d_k(a).x ux + d_k(a).y uy for k = 0, 1
 *              and its negative for k = 2, 3.  b is seen from a along k when dist > 0, cos(a, k, b) > 0.9, some cos(b, k', a) > 0.9
 *              (u turns its sign exactly) and the polarities are opposite: (hxx_a hxx_b + hyy_a hyy_b) + (2 b_a) b_b < 0.
 *              link[a][k] = the nearest such b, the lower slot on equal distances, or none.
 *   5 attempts seeds in (R descending, slot ascending) order - the seed rank -, for each the edge pairs (kb, kc) = (0, 1), (0, 3),
 *              (2, 1), (2, 3) in that order; an attempt exists when link[s][kb] and link[s][kc] exist and differ.
 *   6 grow     the lattice starts as s at cell (0, 0), link[s][kb] at (1, 0), link[s][kc] at (0, 1).  A sweep visits, in ascending
 *              (i, j), the empty cells with |i|, |j| <= cols + rows that had a filled 4-neighbour when the sweep began; a cell
 *              filled earlier in the sweep is seen by the predictions of the later ones.  The prediction of cell (i, j): for the
 *              steps (di, dj) = (1, 0), (0, 1), (-1, 0), (0, -1), with p1 = (i - di, j - dj) and p2 = (i - 2 di, j - 2 dj) both
 *              filled: 2 P[p1] - P[p2] with span |P[p1] - P[p2]|; then for (di, dj) = (1, 1), (1, -1), (-1, 1), (-1, -1), with
 *              p1 = (i - di, j), p2 = (i, j - dj), p3 = (i - di, j - dj) all filled: (P[p1] + P[p2]) - P[p3] with span the smaller
 *              of |P[p1] - P[p3]|, |P[p2] - P[p3]|.  The stencils that apply are summed in that order, coordinate by coordinate,
 *              the sum divided by their number; the span is the smallest.  No stencil: the cell stays empty.  The cell takes the
 *              slot q not in the lattice with d = |P[q] - prediction| <= 0.3 span whose polarity is opposite to that of every
 *              filled 4-neighbour of the cell, the smallest d, the lower slot on equal d.  Sweeps repeat until one fills nothing.
 *   7 settle   up to three rounds over the filled cells in ascending (i, j): the cell is emptied and its slot freed, step 6's
 *              choice is made for it (its own slot when there is none); a round that changes nothing is the last.
 *   8 window   over the box of the filled cells: the cols x rows and rows x cols windows in which every cell is filled.  The
 *              attempt finds a board when there is exactly one.  The FIRST attempt in (seed rank, pair) order that does is the
 *              winner; every attempt is run and counted whatever the others do.
 *   9 label    G[j][i] = the window, h x w.  With o = P[G[0][0]], ec = P[G[0][1]] - o, er = P[G[1][0]] - o: when
 *              ec.x er.y - ec.y er.x < 0 the window is mirrored in i.  Of the turns A[r][c] = G[r][c], G[c][w-1-r],
 *              G[h-1-r][w-1-c], G[h-1-c][r] those of shape rows x cols are admissible; the one whose A[0][0] is smallest in
 *              (y, x) wins, the earlier on a tie.  Corner id = r cols + c is A[r][c]; its board point is (c, r) squares.
 * The method is that of the Python layer's assemble_checkerboard, which states the reasons; a partial board gives none.
 *
 * ccal_assemble_checkerboards_batch: all arrays are host pointers.  offsets [n_img + 1] (offsets[0] == 0, no decrease); xy
 * [offsets[n_img]][2]; hess [offsets[n_img]][3].  Per image k: found_out[k] = 0 / 1; xy_out [n_img][cols rows][2] = the positions
 * in id order, copies of the input; idx_out [n_img][cols rows] (NULL: not wanted) = the image's row index of each; flags_out[k]
 * (bit 1 only); stats_out [n_img][4] (NULL: not wanted) = rows kept, attempts that found a board, the winner's seed rank and pair
 * (-1, -1 without a winner).  The xy_out and idx_out rows of an image without a board are not written.
 *
 * ccal_detect_checkerboards_batch / _dev: images in, boards out, nothing coming back between the stages.  Images as above.  Every
 * field of ccal_detect_checkerboards_opts is the stage parameter of that name and has its range, cand_cap in 1 .. 4096; there are no
 * defaults (the Python layer's: step 1, nms_radius 5, min_response 1, rel_q10 102, cand_cap 4096; half_win 5, max_iterations 30,
 * eps 1e-3).  Per image:
 *   1 candidates  ccal_detect_corners_* with (step, nms_radius, min_response, rel_q10): the first min(count, cand_cap) in row-major order.
 *   2 starts      the integer (x, y) of each stored candidate as f64.
 *   3 refine      ccal_refine_corners_* with (half_win, max_iterations, eps) on those starts.
 *   4 rows        the corners with status CCAL_OK in candidate order, each with its candidate's Hessian as f64.
 *   5 assemble    the rule above with (cols, rows).
 * Outputs per image k: found_out[k]; xy_out [n_img][cols rows][2] in f64 as refined, before any rounding to f32, not written
 * without a board; flags_out[k]: bit 0 (CCAL_BOARD_FLAG_CAND_CAP) more candidates than cand_cap, bit 1 the kept limit; stats_out
 * [n_img][4] (NULL: not wanted) as above.
 * All three are pure functions of an image's rows (of the image and the options): the outputs do not depend on the image's place
 * in the batch, on what else is in it, on how the library cuts the batch into chunks or on the run.  No atomics; every order is an
 * index order.  The _dev form takes a device pointer to the images (the output of ccal_remap_dev on this context's stream, or a
 * block whose writes are complete); everything else stays a host array.  All return when the outputs are written.
 * CCAL_ERR_INVALID_ARG, nothing launched or written: cols or rows outside 2 .. 20, n_img < 0, offsets that decrease or do not start
 * at 0, more than 4096 rows in an image, opts NULL, a field outside its stage's range, cand_cap outside 1 .. 4096, a dtype other
 * than the two, width, height <= 0, more than 2^31 - 1 pixels in an image, a NULL required pointer (with n_img > 0: offsets, xy and
 * hess when there is a row, images, found_out, xy_out, flags_out).  n_img == 0 is valid. */
#define CCAL_BOARD_MIN_SIDE 2
#define CCAL_BOARD_MAX_SIDE 20
#define CCAL_BOARD_MAX_ROWS 4096
#define CCAL_BOARD_MAX_KEPT 512
#define CCAL_BOARD_FLAG_CAND_CAP 1
#define CCAL_BOARD_FLAG_KEPT_LIMIT 2
int ccal_assemble_checkerboards_batch(ccal_ctx* ctx, int n_img, const int64_t* offsets /* [n_img + 1] */, const double* xy,
                                      const double* hess, int cols, int rows, int32_t* found_out /* [n_img] */,
                                      double* xy_out /* [n_img][cols*rows][2] */, int32_t* idx_out /* [n_img][cols*rows] or NULL */,
                                      int32_t* flags_out /* [n_img] */, int32_t* stats_out /* [n_img][4] or NULL */);
typedef struct {
    /* detector */
    int32_t step, nms_radius;
    int64_t min_response;
    int32_t rel_q10, cand_cap;
    /* refinement */
    int32_t half_win, max_iterations;
    double eps;
    /* assembly */
    int32_t cols, rows;
    int64_t reserved_;
} ccal_detect_checkerboards_opts;
int ccal_detect_checkerboards_batch(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images,
                                    const ccal_detect_checkerboards_opts* opts, int32_t* found_out /* [n_img] */,
                                    double* xy_out /* [n_img][cols*rows][2] */, int32_t* flags_out /* [n_img] */,
                                    int32_t* stats_out /* [n_img][4] or NULL */);
int ccal_detect_checkerboards_dev(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images_dev,
                                  const ccal_detect_checkerboards_opts* opts, int32_t* found_out /* [n_img] */,
                                  double* xy_out /* [n_img][cols*rows][2] */, int32_t* flags_out /* [n_img] */,
                                  int32_t* stats_out /* [n_img][4] or NULL */);

/* ---- rendering calibration targets through the camera models ----------------------------------------------------------------------
 * Grey images of a checkerboard or an AprilGrid as a camera of one of the four models sees it at given poses: what a synthetic
 * session, a check of a planned board, lens and distance, or a timing tool needs in front of the image stages above.
 * tests/render_ref.py is the numpy f64 yardstick of the rule below; the render unit is compiled without fused multiply-adds, so
 * that steps 3 to 5 round as numpy rounds them.  Every operation is an IEEE f64 + - * / floor or rint, rounded on its own, in the
 * order written.
 *
 * Inputs.  model, params: UCM, EUCM, KB4 or OPENCV5 with its parameters in the context's conventions (OPENCV5's coefficients are
 * permuted to the canonical order at the boundary, as by ccal_project_points; the two small-radius thresholds are the context's).
 * dtype, width, height, n_img: the images [n_img][height][width] of CCAL_PIX_U8 / CCAL_PIX_U16.  poses [n_img][6]: rvec then tvec,
 * board -> camera.  The host turns each into R = I + sin(a) K + (1 - cos(a)) K K (a = |rvec|, K = [rvec / a]x; R = I when
 * a < 1e-12) and tb = R^T t, tb_j = R[0][j] t[0] + R[1][j] t[1] + R[2][j] t[2], in f64.  target: ccal_render_target, one struct for
 * both kinds.  opts: ccal_render_opts - supersample s in 1 .. 8; black, white, background in 8-bit grey levels (finite); margin >= 0
 * in metres, +inf allowed: the white sheet extends that far beyond the pattern.  ccal_render_set_defaults: s = 4, black 40, white
 * 215, background 0, margin = one square (checkerboard) or one tag pitch tag_size (1 + tag_spacing) (AprilGrid).
 *
 * Per sub-pixel ray (a, b), a, b = 0 .. s - 1, of pixel (px, py); its class is B (black), W (white) or G (background):
 *   1 pixel     u = px + ((a + 0.5) / s - 0.5), v = py + ((b + 0.5) / s - 0.5).
 *   2 ray       GenericModel::unproject of (u, v) as ccal_unproject_points states it; no ray: G.
 *   3 plane     d_j = R[0][j] ray.x + R[1][j] ray.y + R[2][j] ray.z (d = R^T ray); k = tb.z / d.z; k not finite or not > 0: G.
 *   4 point     X = k d.x - tb.x, Y = k d.y - tb.y: the point of the plane z = 0 of the board.
 *   5 pattern   below; a point outside the sheet: G.
 * Checkerboard (cols, rows inner corners, square): sheet -square - margin <= X <= cols square + margin, the same for Y with rows.
 *   i = floor(X / square) + 1, j = floor(Y / square) + 1; the point is on the pattern when 0 <= i <= cols and 0 <= j <= rows, and
 *   then B when i + j is even; everything else on the sheet is W.  Inner corner (c, r) lies at (c square, r square, 0) - the
 *   labelling of ccal_detect_checkerboards_*.
 * AprilGrid (tag_size, tag_spacing, tag_rows, tag_cols, first_id, family_bits = d d, codes, border): x to the right, rows towards
 *   negative y.  pitch = tag_size (1 + tag_spacing), Yd = -Y, sheet -tag_spacing tag_size - margin <= X <= tag_cols pitch + margin,
 *   the same for Yd with tag_rows.  c = floor(X / pitch), r = floor(Yd / pitch), u = (X - c pitch) / tag_size,
 *   v = (Yd - r pitch) / tag_size.  Inside a tag - 0 <= c < tag_cols, 0 <= r < tag_rows, u < 1, v < 1 - with n = d + 2 border:
 *   cell (cv, cu) = (floor(v n), floor(u n)) clamped to 0 .. n - 1; a cell of the border ring is B; data cell (cv - border,
 *   cu - border) = (y, x) is W when bit d d - 1 - (y d + x) of code first_id + r tag_cols + c is set, else B - the bit order of
 *   ccal_decode_tags_*.  A gap square - u >= 1, v >= 1, -1 <= c < tag_cols, -1 <= r < tag_rows - is B.  Everything else on the
 *   sheet is W.  Tag (r, c)'s outer corners are (x, y), (x + s, y), (x + s, y - s), (x, y - s) with x = c pitch, y = -r pitch,
 *   s = tag_size: the order of the decoder's corners_out.
 * Pixel: lum = ((n_B black + n_W white) + n_G background) / (s s); the pixel is rint(lum) for u8 and rint(lum 257) for u16 (round
 * half to even), clamped to the type.  The plane is two-sided: a pose that shows the back shows the mirror image.  These are ideal
 * images; lens blur, vignetting, exposure and sensor noise are the photometric stage's, stated in the next section
 * (ccal_render_photo_targets_* renders and degrades in one call).
 * An image is a pure function of the model, the target, the options and its pose: image k of a call equals the same pose rendered
 * alone, whatever the batch and however the library cuts it into chunks, and runs repeat to the bit.  No atomics.
 *
 * ccal_render_targets_batch: images_out is a host array.  ccal_render_targets_dev: images_out_dev is a device pointer; the render
 * runs on the context's stream and the block is never touched by the host, so it goes straight into ccal_detect_checkerboards_dev,
 * ccal_detect_tags_dev or ccal_remap_dev.  Both return when the images are written.
 * CCAL_ERR_UNSUPPORTED: the EUCMT container.  CCAL_ERR_INVALID_ARG with a message that names the argument, nothing launched or
 * written: an unknown model, dtype or target kind; width, height <= 0 or n_img < 0; more than 2^31 - 1 pixels in an image;
 * supersample outside 1 .. 8; black, white or background not finite; margin negative or NaN; square, tag_size or tag_spacing not
 * finite and positive; cols, rows, tag_rows or tag_cols < 1; more than 4096 tags; family_bits not a square in 1 .. 64; border < 1;
 * first_id < 0; n_codes < first_id + tag_rows tag_cols; params, target or opts NULL; with n_img > 0: poses, the output pointer or
 * (AprilGrid) codes NULL.  n_img == 0 is valid. */
typedef enum { CCAL_TARGET_CHECKERBOARD = 0, CCAL_TARGET_APRILGRID = 1 } ccal_target_kind;
typedef struct {
    int32_t kind;                          /* ccal_target_kind */
    /* checkerboard */
    int32_t cols, rows, reserved_;         /* inner corners */
    double square;                         /* metres */
    /* AprilGrid */
    double tag_size, tag_spacing;          /* metres; the gap between tags as a fraction of tag_size */
    int32_t tag_rows, tag_cols, first_id, family_bits, n_codes, border;
    const uint64_t* codes;                 /* [n_codes]: the family's table, as for ccal_decode_tags_* */
} ccal_render_target;
typedef struct {
    int32_t supersample, reserved_;
    double black, white, background;       /* 8-bit grey levels */
    double margin;                         /* metres */
} ccal_render_opts;
int ccal_render_set_defaults(const ccal_render_target* target, ccal_render_opts* opts);
int ccal_render_targets_batch(ccal_ctx* ctx, int model, const double* params, int dtype, int width, int height, int n_img,
                              const double* poses /* [n_img][6] */, const ccal_render_target* target, const ccal_render_opts* opts,
                              void* images_out /* [n_img][height][width] */);
int ccal_render_targets_dev(ccal_ctx* ctx, int model, const double* params, int dtype, int width, int height, int n_img,
                            const double* poses /* [n_img][6] */, const ccal_render_target* target, const ccal_render_opts* opts,
                            void* images_out_dev /* [n_img][height][width] */);

/* ---- the photometric stage: lens blur, vignetting, exposure and sensor noise ------------------------------------------------------
 * From ideal irradiance to pixels: what stands between the renderer above and the frames a camera delivers, so that a robustness
 * question of the image stages (what half_win, nms_radius, rel_threshold, min_contrast or offset tolerate at a given defocus and
 * noise level) is answered without the images leaving the device.  tests/photo_ref.py is the numpy yardstick of the rule below and
 * the device is held to it to the bit: the unit is compiled without fused multiply-adds; all arithmetic is IEEE f64 + - * /, floor,
 * rint, min, max, every operation rounded on its own, in the order written; the integer parts are u64 modulo 2^64.
 *
 * Options: ccal_photo_opts.  blur_sigma in 0 .. 16/3 px (a Gaussian PSF; 0: none); vignette v >= 0 (the gain at the corners is
 * 1 / (1 + v)^2; 0: none); gain finite, >= 0 (exposure; 1: none); noise_read >= 0 in 8-bit grey levels; noise_shot >= 0, variance
 * per grey level; seed; first_index >= 0: the noise stream of image k of a call is seed + first_index + k.
 * ccal_photo_set_defaults switches everything off: 0, 0, 1, 0, 0, 0, 0.
 *
 * Tables, made on the host (ccal_photo_tables returns exactly what the kernel uses; host only, no context):
 *   radius  r = min(16, ceil(3 blur_sigma)).
 *   taps    w_0 = 1, w_k = exp(-k k / (2 sigma sigma)) (0 where 2 sigma sigma underflows), norm = w_0 + 2 (w_1 + ... + w_r) with the
 *           inner sum in ascending k, t_k = w_k / norm, k = 0 .. r; for r = 0, t_0 = 1.  taps_out[17]: the entries above r are 0.
 *   sigma   T[g] = sqrt(noise_read noise_read + noise_shot g), g = 0 .. 255.
 *
 * Per output pixel (x, y) of image k of W x H pixels.  I is the ideal image on the 16-bit scale: a u16 source as it is, 257 p for a
 * u8 source.
 *   a  H(x, y) = the sum over j = -r .. r, ascending, of t_|j| I(clamp(x + j, 0, W - 1), y): acc = 0.0, then acc = acc + t I.
 *   b  B(x, y) = the same sum over H(x, clamp(y + j, 0, H - 1)).  For r = 0, B = I.
 *   c  V = ((B / 257) gain) g with g = 1 / ((1 + v rho2) (1 + v rho2)), rho2 = (dx dx + dy dy) / (cx cx + cy cy), cx = (W - 1) / 2,
 *      cy = (H - 1) / 2, dx = x - cx, dy = y - cy; for a 1 x 1 image rho2 = 0.
 *   d  Vc = min(max(V, 0), 255), i = min(floor(Vc), 254), sig = T[i] + (T[i + 1] - T[i]) (Vc - i).
 *   e  z = (S - 393210) / 65536, S = the integer sum of the twelve 16-bit fields of w_0, w_1, w_2; w_j = mix(key + 4 (y W + x) + j),
 *      key = mix(seed + first_index + k); mix(a) is splitmix64's finaliser: a ^= a >> 30, a *= 0xBF58476D1CE4E5B9, a ^= a >> 27,
 *      a *= 0x94D049BB133111EB, a ^= a >> 31.  z is an Irwin-Hall draw of unit variance with its tails cut at +-6.
 *   f  Y = V + sig z.
 *   g  u8: rint(min(max(Y, 0), 255)); u16: rint(min(max(Y 257, 0), 65535)).
 * Consequences: with every effect off and u16 output the result is the source (of ccal_render_photo_targets_*: the images of
 * ccal_render_targets_* at CCAL_PIX_U16) bit for bit; image k of a call equals image 0 of a call with first_index + k, in any batch,
 * under any chunking, from run to run.  No atomics.
 *
 * ccal_photo_apply_dev: src_dev [n_img][height][width] of src_dtype to dst_dev of dst_dtype, both device pointers, CCAL_PIX_U8 /
 * CCAL_PIX_U16 each.  It only enqueues on the context's stream, like ccal_remap_dev, and stages nothing: the tables travel in the
 * kernel's arguments.  The two blocks must not overlap.
 * ccal_render_photo_targets / _dev: the arguments of ccal_render_targets_batch / _dev and the photo options.  The ideal images are
 * rendered at CCAL_PIX_U16 chunk by chunk into the call's own block and go through the stage into images_out (a host array) /
 * images_out_dev; an image's noise index is its index in the call.  Both return when the images are written.
 * CCAL_ERR_INVALID_ARG with a message that names the argument, nothing launched or written: photo NULL; blur_sigma outside
 * 0 .. 16/3 or NaN; vignette, noise_read, noise_shot or gain negative or not finite; first_index < 0; a dtype other than the two,
 * width, height <= 0, n_img < 0, more than 2^31 - 1 pixels in an image; with n_img > 0 a NULL block or blocks that overlap; and
 * what ccal_render_targets_* refuses.  n_img == 0 is valid. */
#define CCAL_PHOTO_MAX_RADIUS 16
typedef struct {
    double blur_sigma;                     /* px, 0 .. 16/3: Gaussian PSF; 0 = none */
    double vignette;                       /* v >= 0: corner gain 1 / (1 + v)^2; 0 = none */
    double gain;                           /* exposure, finite, >= 0; 1 = none */
    double noise_read;                     /* grey levels (8-bit scale), >= 0 */
    double noise_shot;                     /* variance per grey level, >= 0 */
    uint64_t seed;
    int64_t first_index;                   /* the noise stream of image k is seed + first_index + k */
} ccal_photo_opts;
int ccal_photo_set_defaults(ccal_photo_opts* photo);
int ccal_photo_tables(const ccal_photo_opts* photo, int32_t* radius_out, double* taps_out /* [17] */, double* sigma_out /* [256] */);
int ccal_photo_apply_dev(ccal_ctx* ctx, int src_dtype, int dst_dtype, int width, int height, int n_img, const void* src_dev,
                         void* dst_dev, const ccal_photo_opts* photo);
int ccal_render_photo_targets(ccal_ctx* ctx, int model, const double* params, int dtype, int width, int height, int n_img,
                              const double* poses /* [n_img][6] */, const ccal_render_target* target, const ccal_render_opts* opts,
                              const ccal_photo_opts* photo, void* images_out /* [n_img][height][width] */);
int ccal_render_photo_targets_dev(ccal_ctx* ctx, int model, const double* params, int dtype, int width, int height, int n_img,
                                  const double* poses /* [n_img][6] */, const ccal_render_target* target,
                                  const ccal_render_opts* opts, const ccal_photo_opts* photo,
                                  void* images_out_dev /* [n_img][height][width] */);

/* ---- local contrast normalisation: frames ahead of the detectors ----------------------------------------------------------------
 * The saddle detector keeps candidates above rel_threshold times the strongest response of the whole image, and the proposer's and
 * the decoder's min_contrast are absolute grey levels: a frame whose contrast falls towards the edge (vignetting) or that is
 * under-exposed loses corners and tags where a fisheye lens has its information.  This stage maps every pixel to its distance from
 * the mean of the (2 r + 1)^2 window around it in units of the window's standard deviation, device block to device block; the result
 * feeds the _dev calls above as any frame does.  It is for frames that need it, not a default: on a clean frame it costs accuracy
 * (README, EXPERIMENTS.md).  tests/normalize_ref.py is the numpy yardstick of the rule below and the device is held to it to the
 * bit: the sums, the variance term and its square root are exact integers (u64 / i64 suffice: the largest intermediate is
 * 4225^2 65535^2 < 2^63), the last two steps are IEEE f64, every operation rounded on its own (the unit is compiled without fused
 * multiply-adds).
 *
 * Options: ccal_normalize_opts.  radius r in 1 .. 32: the window is (2 r + 1)^2 pixels, N its pixel count; min_sigma in 0 .. 255, in
 * 8-bit grey levels: the noise floor, so that flat regions are not blown up; amp finite, >= 0: output grey levels (8-bit scale) per
 * local standard deviation.  ccal_normalize_set_defaults: 16, 0, 4.0, 64.0 - a window half black, half white maps to 64 and 192.
 *
 * Per output pixel (x, y) of image k of W x H pixels.  I is the source on the 16-bit scale: a u16 source as it is, 257 p for a u8
 * source.
 *   a  S1 = the sum of I(clamp(x + i, 0, W - 1), clamp(y + j, 0, H - 1)) over i, j = -r .. r; S2 = the same sum of I I.
 *   b  v = N S2 - S1 S1; s0 = the largest integer with s0 s0 <= v; F = max(1, rint(257 min_sigma)); s = max(s0, N F).
 *   c  d = N I(x, y) - S1.
 *   d  q = (double)d / (double)s; Y = 128.0 + amp q.
 *   e  u8: rint(min(max(Y, 0), 255)); u16: rint(min(max(Y 257, 0), 65535)).
 * Consequences: a constant image gives 128 (u8) or 32896 (u16) everywhere; a u16 source equal to 257 times a u8 source gives the
 * same output; image k does not depend on its batch; results are equal from run to run.  No atomics.  Because the sums are
 * integers, the order of summation is free - the kernel keeps running sums down a column - and that latitude is deliberate.
 *
 * ccal_normalize_dev: src_dev [n_img][height][width] of src_dtype to dst_dev of dst_dtype, both device pointers, CCAL_PIX_U8 /
 * CCAL_PIX_U16 each.  It only enqueues on the context's stream, like ccal_photo_apply_dev, allocates and stages nothing.  The two
 * blocks must not overlap.  There is no host-pointer form.
 * CCAL_ERR_INVALID_ARG with a message that names the argument, nothing launched or written: norm NULL; radius outside 1 .. 32;
 * min_sigma outside 0 .. 255 or NaN; amp negative or not finite; a dtype other than the two, width, height <= 0, n_img < 0, more
 * than 2^31 - 1 pixels in an image; with n_img > 0 a NULL block or blocks that overlap.  n_img == 0 is valid.
 * ccal_normalize_set_defaults is host only and needs no context. */
#define CCAL_NORMALIZE_MAX_RADIUS 32
typedef struct {
    int32_t radius;                        /* r in 1 .. 32: a window of (2 r + 1)^2 pixels */
    int32_t reserved_;
    double min_sigma;                      /* grey levels (8-bit scale), 0 .. 255: the floor of the local standard deviation */
    double amp;                            /* output grey levels (8-bit scale) per local standard deviation; finite, >= 0 */
} ccal_normalize_opts;
int ccal_normalize_set_defaults(ccal_normalize_opts* norm);
int ccal_normalize_dev(ccal_ctx* ctx, int src_dtype, int dst_dtype, int width, int height, int n_img, const void* src_dev,
                       void* dst_dev, const ccal_normalize_opts* norm);

/* ---- grey frames from colour and raw Bayer frames, with binning ------------------------------------------------------------------
 * Every image stage above takes single-channel frames.  The reference hands its detector whatever the session's .png / .jpg
 * decodes to (src/data_loader.rs:36-44), for most cameras colour; machine-vision cameras deliver the raw Bayer mosaic.  This stage
 * turns any of the layouts below into a grey block, device block to device block, optionally binned 2 x or 4 x for sensors far
 * larger than the detector's working scale (README).  The rule is exact integer arithmetic with ONE rounding; tests/grey_ref.py is
 * its numpy yardstick and the device is held to it to the bit.
 *
 * Source block.  Interleaved layouts (RGB, BGR, RGBA, BGRA): [n_img][height][width][c] of src_dtype, c = 3 or 4; alpha is ignored.
 * GREY and the Bayer layouts: [n_img][height][width].  A u16 block is 2-byte aligned, as its type requires; nothing more is asked
 * of either block's address.  A Bayer layout names the 2 x 2 cell at the image's origin in row-major order, (x, y) = (column, row) -
 * other libraries name the same mosaics differently:
 *
 *     layout                    (0,0)  (1,0)  (0,1)  (1,1)
 *     CCAL_LAYOUT_BAYER_RGGB      R      G      G      B
 *     CCAL_LAYOUT_BAYER_BGGR      B      G      G      R
 *     CCAL_LAYOUT_BAYER_GRBG      G      R      B      G
 *     CCAL_LAYOUT_BAYER_GBRG      G      B      R      G
 *
 * Destination block.  [n_img][height / bin][width / bin] of dst_dtype, integer division: the rows and columns of an incomplete
 * last block are dropped.  Output pixel X has its centre at source coordinate bin X + (bin - 1) / 2 (likewise Y): a corner found at
 * x in the grey frame lies at bin x + (bin - 1) / 2 on the sensor.
 *
 * Options: ccal_grey_opts.  bin 1, 2 or 4; the weights w_r, w_g, w_b >= 0 with w_r + w_g + w_b == 65536.
 * ccal_grey_set_defaults: 1; 19595, 38470, 7471 (0.299 / 0.587 / 0.114).
 *
 * Per source pixel (x, y).  I is the sample on the 16-bit scale: a u16 sample as it is, 257 p for a u8 sample.
 *   a  the triple (R4, G4, B4), four times the channel values, so that every term is an integer.
 *        GREY         all three are 4 I.
 *        interleaved  4 times the channel.
 *        Bayer, at an R or B site of colour c: c4 = 4 I(x, y); G4 = the sum of the four edge neighbours; the opposite colour = the
 *                     sum of the four diagonal neighbours.
 *        Bayer, at a G site: G4 = 4 I; the colour of the horizontal neighbours is 2 (I(x - 1, y) + I(x + 1, y)), the colour of the
 *                     vertical neighbours 2 (I(x, y - 1) + I(x, y + 1)).
 *        Bayer border a neighbour coordinate i outside 0 .. n - 1 is reflected about the edge pixel: i < 0 gives -i, i >= n gives
 *                     2 (n - 1) - i.  This keeps the mosaic's parity; hence width and height are at least 2 for a Bayer layout.
 *   b  N = w_r R4 + w_g G4 + w_b B4 (< 2^34).
 * Per output pixel: S = the sum of N over its bin x bin block (< 2^38); s = 18 + 2 log2(bin);
 *   u16: (S + 2^(s-1)) >> s;   u8: floor((S + 257 2^(s-1)) / (257 2^s)).  One rounding, half up, for either type.
 * Consequences: GREY at bin 1 with equal types is a copy; u8 -> u16 is 257 p; u16 -> u8 is (v + 128) / 257; a u16 source equal to
 * 257 times a u8 source gives the same output for every layout, bin and destination type (so a u8 source is computed in 32 bits); a
 * Bayer frame whose sites are all v gives v; full-scale input gives exactly 255 / 65535 at every bin; BGR(A) equals RGB(A) with the
 * channels swapped; RGBA equals RGB for any alpha; image k does not depend on its batch; results are equal from run to run.  No
 * atomics, no floating point.
 *
 * ccal_grey_dev: it only enqueues on the context's stream, like ccal_normalize_dev, allocates and stages nothing.  The two blocks
 * must not overlap.  There is no host-pointer and no in-place form.
 * CCAL_ERR_INVALID_ARG with a message that starts "ccal_grey_dev: " and names the argument, nothing launched or written: opts NULL; a
 * layout outside the enum; bin not 1, 2 or 4; a negative weight or a sum other than 65536; a dtype other than the two; width,
 * height <= 0 or n_img < 0; more than 2^31 - 1 pixels in a source image; width < bin or height < bin; a Bayer layout with a side
 * below 2; with n_img > 0 a NULL block or blocks that share a byte (their byte counts follow from the layout, the types and the bin;
 * blocks that touch are fine).  n_img == 0 is valid and looks at no pointer.
 * ccal_grey_set_defaults is host only and needs no context. */
typedef enum {
    CCAL_LAYOUT_GREY = 0, CCAL_LAYOUT_RGB, CCAL_LAYOUT_BGR, CCAL_LAYOUT_RGBA, CCAL_LAYOUT_BGRA,
    CCAL_LAYOUT_BAYER_RGGB, CCAL_LAYOUT_BAYER_BGGR, CCAL_LAYOUT_BAYER_GRBG, CCAL_LAYOUT_BAYER_GBRG
} ccal_pixel_layout;
typedef struct {
    int32_t bin;                           /* 1, 2 or 4: the output is [height / bin][width / bin] */
    int32_t w_r, w_g, w_b;                 /* >= 0, w_r + w_g + w_b == 65536 */
} ccal_grey_opts;
int ccal_grey_set_defaults(ccal_grey_opts* opts);
int ccal_grey_dev(ccal_ctx* ctx, int layout, int src_dtype, int dst_dtype, int width, int height, int n_img, const void* src_dev,
                  void* dst_dev, const ccal_grey_opts* opts);

/* ---- reference validation() statistics (src/util.rs:721-795) ---------------------------- */
int ccal_reprojection_errors(ccal_problem* p, const double* intr, const double* poses, const double* extr,
                             double* err_out /* [n_corners] Euclidean px error */);
int ccal_validation(ccal_problem* p, int cam, const double* intr, const double* poses, const double* extr,
                    double* avg_99_percent, double* median);

/* ---- calibration uncertainty at a solved point: covariances and leverage ---------------------
 * How well every parameter and every board pose is determined, and which detections carry the estimate - the first-order
 * (Gauss-Newton) covariance of the least-squares problem ccal_solve minimises.  The rule:
 *   The unknowns, in order: x = [camera block (K columns, in the order of ccal_build_normal) | pose of slot 0 (rvec, tvec) |
 *   pose of slot 1 | ...].  J and r are the loss-corrected Jacobian and residuals of all cameras at the given point - exactly
 *   what ccal_eval(..., apply_loss = 1, ...) returns - and H = J^T J.
 *   - Columns of parameters fixed with ccal_fix_param / ccal_disable_distortions are removed before anything is inverted; their
 *     rows and columns of every output are 0.
 *   - Bounds are IGNORED: a parameter resting on a bound is treated as free (its variance is that of the unbounded problem).
 *   - A slot without a single corner has no pose: it is not an unknown.
 *   With n_free = K_free + 6 n_posed, N the number of corners and dof = 2 N - n_free (dof <= 0: CCAL_ERR_INVALID_ARG):
 *   cost         = sum r^2 over the loss-corrected residuals (the quantity ccal_report::final_cost holds)
 *   sigma2       = cost / dof
 *   cov_cam      [K][K] = sigma2 (H^-1)[camera, camera] = sigma2 S^-1, S the reduced system of mode N at lambda = 0
 *   cov_poses    [n_slots][6][6] = sigma2 (V_s^-1 + Y_s^T S^-1 Y_s), Y_s = W_s V_s^-1; V_s the slot's 6 x 6 block of H, W_s its
 *                K x 6 coupling block summed over every camera that saw the slot.  The covariance is in the parameters the solver
 *                steps in (additive axis-angle and translation).  An empty slot: 36 NaN and slot_status 1 (else 0)
 *   leverage     [n_corners] = trace(J_k H^-1 J_k^T), J_k the corner's two rows, with (H^-1)[camera, pose s] = -S^-1 Y_s: NOT
 *                scaled by sigma2, in [0, 2]; the sum over all corners equals n_free (report->leverage_sum: check it)
 * A Cholesky pivot of any V_s or of S at or below 2^-36 x its own diagonal entry: CCAL_ERR_NOT_PD for the whole call (the rule of
 * ccal_init_poses); report->bad_slot names the first offending slot, -1 for S.  Nothing is written to the arrays then.
 * intr == NULL: the point is what ccal_upload_params or a device-resident solve left on the device (poses / extr are ignored);
 * the results are the same bits as with host pointers to the same values.  cov_poses, leverage, slot_status may be NULL.
 * Results are bit-identical from run to run (fixed summation orders, no atomics) and do not depend on what ran before.
 * A sharded problem (communicator, callback or in-process peer set): CCAL_ERR_UNSUPPORTED.  p, cov_cam or report NULL, poses NULL
 * with slots or extr NULL with several cameras (when intr is given): CCAL_ERR_INVALID_ARG, the argument named in ccal_last_error. */
typedef struct {
    int32_t status;                /* ccal_status of the call */
    int32_t bad_slot;              /* CCAL_ERR_NOT_PD: the first slot whose V_s failed, -1: S; else -1 */
    int64_t dof;                   /* 2 N - n_free */
    int32_t n_free;                /* K_free + 6 n_posed */
    int32_t n_posed;               /* slots with at least one corner */
    double cost, sigma2, leverage_sum;
    int32_t reserved_[4];          /* 0 */
} ccal_cov_report;
int ccal_covariance(ccal_problem* p, const double* intr, const double* poses, const double* extr,   /* intr == NULL: the point on the device */
                    double* cov_cam /* [K][K] */, double* cov_poses /* [n_slots][36] or NULL */,
                    double* leverage /* [n_corners], the description's corner order, or NULL */,
                    int32_t* slot_status /* [n_slots] or NULL */, ccal_cov_report* report);

#ifdef __cplusplus
}
#endif
#endif /* CCAL_H */
