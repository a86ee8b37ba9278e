/*
 * sslam.h — C-ABI of the MI355X-native semantic_slam hot path (libsslam_hip.so).
 *
 * Plain pointers and sizes only; no torch / g2o / PCL / ROS types.  Every entry point names the
 * reference interface it replaces (paths relative to the reference repository root).
 * The C++ shims that give these the reference's own method names live in
 *   include/ps_graph_slam_amd/graph_slam.hpp              (ps_graph_slam::GraphSLAM)
 *   include/ps_graph_slam_amd/information_matrix_calculator.hpp (ps_graph_slam::InformationMatrixCalculator)
 *   include/planar_segmentation_amd/point_cloud_segmentation.hpp (point_cloud_segmentation)
 * and INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - return value: >= 0 success (ids / counts where stated), < 0 error (sslam_last_error()).
 *   - poses: 7 doubles  t(x,y,z) q(x,y,z,w)   (same order as g2o's VERTEX_SE3:QUAT row)
 *   - information matrices: dense row-major d x d doubles (d = 6 or 3)
 *   - handles are not re-entrant; different handles may be used from different threads.
 *   - all compute runs on the GPU; there is NO CPU fallback: without a HIP device
 *     sslam_graph_optimize()/sslam_seg_segment() fail with SSLAM_ERR_NO_DEVICE.
 */
#ifndef SSLAM_H
#define SSLAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSLAM_OK 0
#define SSLAM_ERR_INVALID (-1)
#define SSLAM_ERR_NO_DEVICE (-2)
#define SSLAM_ERR_HIP (-3)
#define SSLAM_ERR_NUMERIC (-4)      /* non-finite chi2 / factorisation breakdown */
#define SSLAM_ERR_TOO_FEW_EDGES (-5) /* reference: graph_slam.cpp:184-186 returns false */
#define SSLAM_ERR_UNSUPPORTED (-6)
#define SSLAM_ERR_IO (-7)

const char* sslam_last_error(void);
/* number of visible HIP devices (0 on a CPU-only box; never fails) */
int sslam_device_count(void);
/* Page-locked host memory (hipHostMalloc / hipHostFree) for callers that do not link HIP themselves: clouds handed to
 * sslam_seg_submit_batch from such a buffer are copied asynchronously.  NULL (and sslam_last_error) without a device. */
void* sslam_pinned_alloc(size_t bytes);
void sslam_pinned_free(void* p);

/* ============================================================================================
 * Backend: ps_graph_slam::GraphSLAM  (reference include/ps_graph_slam/graph_slam.hpp:37-144)
 * ==========================================================================================*/
typedef struct sslam_graph sslam_graph;

typedef struct sslam_opt_stats {
  int iterations;        /* LM iterations performed (g2o SparseOptimizer::optimize return value) */
  int trials;            /* linear solves (accepted + rejected LM trials) */
  int status;            /* 0 = iteration cap reached, 1 = LM terminated (10 failed trials or rho == 0),
                            <0 = SSLAM_ERR_* */
  int host_plan_us;      /* sslam_graph_optimize: microseconds of host work before the first launch of this call that a structure change
                            cost -- batch tables + symbolic factorisation (0 when the structure of the last call was reused); 0 in batches */
  double chi2_before;    /* graph->chi2() before (graph_slam.cpp:202) */
  double chi2_after;     /* graph->chi2() after  (graph_slam.cpp:211) */
  double lambda;         /* final LM damping */
  double seconds;        /* wall time of the call (graph_slam.cpp:204-215 "time:") */
  int64_t solver_iterations; /* PCG iterations summed over trials (0 for the direct solver) */
} sslam_opt_stats;

/* GraphSLAM::GraphSLAM (graph_slam.cpp:40-97): LM over block-sparse normal equations, sensor
 * offset parameter id 0 = identity.  device = HIP device ordinal. */
sslam_graph* sslam_graph_create(int device);
/* GraphSLAM::~GraphSLAM (graph_slam.cpp:102) */
void sslam_graph_destroy(sslam_graph* g);

/* add_se3_node (graph_slam.cpp:104-115).  The reference fixes the first vertex of the graph;
 * pass fixed = -1 to get exactly that rule, 0/1 to force.  Returns the vertex id (= number of
 * vertices before the call, graph_slam.cpp:106). */
int sslam_graph_add_vertex_se3(sslam_graph* g, const double t_q[7], int fixed);
/* add_point_xyz_node (graph_slam.cpp:127-134) */
int sslam_graph_add_vertex_point(sslam_graph* g, const double p[3]);
/* add_plane_node (commented out in the reference, graph_slam.cpp:117-125; g2o::VertexPlane) */
int sslam_graph_add_vertex_plane(sslam_graph* g, const double n_d[4]);

/* add_se3_edge (graph_slam.cpp:136-148): g2o::EdgeSE3 between SE3 vertices i and j. Returns edge id. */
int sslam_graph_add_edge_se3(sslam_graph* g, int i, int j, const double z_tq[7], const double info[36]);
/* add_se3_point_xyz_edge (graph_slam.cpp:150-166): g2o::EdgeSE3PointXYZ, offset parameter 0.
 * The reference passes an uninitialised robust-kernel pointer (quirk B1): no kernel is applied unless the option
 * "robust_kernel_dcs" asks for the one it names (g2o::RobustKernelDCS). */
int sslam_graph_add_edge_se3_point(sslam_graph* g, int i, int l, const double z[3], const double info[9]);
/* add_se3_plane_edge (commented out, graph_slam.hpp:73-75) -> g2o::EdgeSE3Plane
 * (reference include/g2o/edge_se3_plane.hpp:8-48; numeric Jacobian: g2o's central differences, delta 1e-9 -- evaluated on the device once per
 * edge and linearisation by k_plane_jacobians, a thread per evaluation (round 6); the plane rotation is formed from the normal's components
 * instead of through its two angles: the same matrix to an ulp). */
int sslam_graph_add_edge_se3_plane(sslam_graph* g, int i, int l, const double z[4], const double info[9]);

/* add_point_xyz_point_xyz_edge (graph_slam.cpp:168-180): g2o::EdgePointXYZ between two VertexPointXYZ, e = (p2 - p1) - z.  Declared and
 * defined by the reference, never called there.  With such edges the landmark block of H is no longer block diagonal: solver 2
 * (Schur complement on the landmarks) refuses the graph, the Cholesky solvers and solver 0 take it as it is. */
int sslam_graph_add_edge_point_point(sslam_graph* g, int l1, int l2, const double z[3], const double info[9]);

/* add_se3_prior_xyz_edge (commented out in the reference, graph_slam.hpp:115-126, the declaration :125-126; g2o registration EDGE_SE3_PRIORXYZ, graph_slam.cpp:32):
 * hdl_graph_slam's EdgeSE3PriorXYZ, a unary edge on the SE3 vertex v with e = t(v) - z and a 3 x 3 information matrix -- an absolute
 * position (GNSS, a motion-capture fix, a surveyed marker).  Analytic Jacobian [R | 0] (g2o differentiates it numerically; DESIGN.md
 * section 2).  Not touched by "robust_kernel_dcs" (that option stays on the landmark edges); a kernel of its own -- a GNSS fix under multipath --
 * comes from sslam_graph_set_edge_robust_kernel.  Returns the edge id (same counter as the binary
 * edges); a prior counts as an edge for the < 10 edges rule and gives its vertex a hessian index. */
int sslam_graph_add_edge_se3_prior_xyz(sslam_graph* g, int v, const double z[3], const double info[9]);
/* add_se3_prior_xy_edge (commented out, graph_slam.hpp:115-123, the declaration :122-123; EDGE_SE3_PRIORXY, graph_slam.cpp:31): EdgeSE3PriorXY, e = t(v).xy - z,
 * 2 x 2 information matrix; otherwise as sslam_graph_add_edge_se3_prior_xyz. */
int sslam_graph_add_edge_se3_prior_xy(sslam_graph* g, int v, const double z[2], const double info[4]);

int sslam_graph_num_vertices(const sslam_graph* g);
int sslam_graph_num_edges(const sslam_graph* g);

/* vertex->estimate() / setEstimate(); out has 7 (SE3), 3 (point) or 4 (plane) doubles */
int sslam_graph_get_vertex(const sslam_graph* g, int id, double* out);
int sslam_graph_set_vertex(sslam_graph* g, int id, const double* in);
/* vertex->hessianIndex() after initializeOptimization (used at semantic_graph_slam.cpp:188-190):
 * scalar offset in g2o's ordering (non-fixed vertices with edges, by id), or -1. */
int sslam_graph_hessian_index(sslam_graph* g, int id);

/* Options (doubles): "solver" 1 = sparse block Cholesky (default; what "lm_var" + csparse selects in the reference),
 * 0 = block-Jacobi PCG on the full system, 2 = Schur complement on the landmark block + PCG on the reduced pose system (matrix-free;
 * BASELINE.json north_star).  SOLVER 2 IS S-SCALE ONLY: its preconditioner is block-Jacobi, and on a long pose chain with the reference's
 * odometry information (1 / 0.00001 on the rotation block against 2.5 on a landmark, config/bucket_detector.yaml:22-27) the reduced
 * system needs ~1,050 CG iterations per damping trial at 5000 poses (157 ms, against 1.5 ms for the direct solver) -- it converges to the
 * same optimum (tests: S config, and since round 6 three LM iterations of the L config against the oracle) but is not a solver for the
 * L configuration; use 1.  Round 6 measured what the missing preconditioner would buy (tools/pcg_preconditioner_experiment.py, the L graph's
 * reduced system at g2o's first lambda, relative residual 1e-10): block-Jacobi 801 CG iterations, the EXACT block-tridiagonal factor of
 * the odometry chain 111, wider bands (2-16 blocks) 111-112 -- what is left is the coupling of poses on different laps through shared
 * landmarks.  A tridiagonal solve is two sequential sweeps over 5000 blocks per CG iteration: ~110 x 1.5 ms per trial on one wave per
 * graph, slower than the 157 ms it would replace, and still above the 100 iterations asked for -> not built; decision closed.  (3, the window-plan Cholesky of round 3 -- register-resident sliding
 * fronts, VALU and FP64-MFMA updates; correct, leaner in traffic, 2-2.7x slower -- was removed from the library in round 5; DESIGN.md
 * section 5 keeps its measurements.)  "pcg_tol" relative residual; "pcg_max_iters";
 * "robust_kernel_dcs" = phi > 0: g2o::RobustKernelDCS(delta = phi) on every landmark edge (EdgeSE3PointXYZ / EdgeSE3Plane), as
 * graph_slam.cpp:155,161 intends (opt-in, phi = 1 is g2o's default delta); 0 = no kernel (default);
 * "fused_small_graph" 1 (default) / 0: a batch of fewer than eight graphs whose elimination tree is narrower than the chip runs the
 * factorisation, both triangular solves and the begin / end halves of a damping trial in ONE dependency-driven launch (k_chol_flow; the
 * reference's per-tick call pattern, semantic_graph_slam.cpp:58-102); 0: the stand-alone kernels -- same results, bitwise.  (The
 * one-workgroup-per-graph kernel k_lm_trial_small of round 4 -- measured slower, DESIGN.md section 5 -- left the library in round 5.)
 * "speculative_trials" 0 / 1 (default since round 5) / 2: a single small graph runs the damping trials of an LM iteration side by side -- g2o's retry
 * lambdas are known when the iteration starts -- in the lanes of ONE launch (k_chol_spec_round) that also replays the accept / reject
 * sequence over their results: bitwise the sequential result, trial counts included.  1: the lanes join once a trial of the iteration
 * has been rejected, and only while every lane gets a workgroup per piece of the tree (about 200 keyframes); 2: every round with all ten
 * lanes.  Mode 1 measured 5.5 vs 6.0 ms per tick at 110 keyframes and 7.4 vs 7.6 at 436 (re-measured
 * in round 5) and is never slower with the lanes-fit rule: the default.  SSLAM_LM_SPEC=0/1/2 in the environment overrides the option for
 * every graph of the process. */
int sslam_graph_set_option(sslam_graph* g, const char* key, double value);

/* Per-edge robust kernels (hdl_graph_slam's GraphSLAM::add_robust_kernel(edge, type, size); what graph_slam.cpp:155,161 of the reference means to
 * do, quirk B1).  g2o semantics (BaseEdge::robustInformation): with e2 = e^T Omega e and d = delta, H += J^T (rho1 Omega) J,
 * b -= J^T (rho1 Omega) e, and the edge's chi2 term is rho0.  g2o's second-order term (rho[2]) is commented out upstream and stays out.
 *
 *   id  name         rho0                                        rho1
 *   0   none         e2                                          1
 *   1   Huber        e2 if e2 <= d^2, else 2 d sqrt(e2) - d^2    1, else d / sqrt(e2)
 *   2   PseudoHuber  2 d^2 (sqrt(1 + e2/d^2) - 1)                1 / sqrt(1 + e2/d^2)
 *   3   Cauchy       d^2 log(1 + e2/d^2)                         1 / (1 + e2/d^2)
 *   4   Welsch       d^2 (1 - exp(-e2/d^2))                      exp(-e2/d^2)
 *   5   Fair         2 d^2 (a - log1p(a)), a = sqrt(e2)/d        1 / (1 + a)
 *   6   Saturated    e2 if e2 <= d^2, else d^2                   1, else 0
 *   7   DCS          e2 s, s = min(1, (2d/(d+e2))^2)             s
 *
 * These are the g2o kernels whose formulas are the same in every g2o release.  GemanMcClure and Tukey changed between releases and are left
 * out on purpose.  Any edge id of the shared counter, any edge class.  kind outside 0..7, delta <= 0 or non-finite with kind != 0, or an
 * unknown edge id: SSLAM_ERR_INVALID, graph untouched.  kind = 0 removes the kernel.
 * Precedence: an edge with a kernel of its own uses it; a landmark edge without one still follows "robust_kernel_dcs"; every other edge
 * without one is plain least squares.
 * A kernel is a VALUE of the edge, not structure: setting one keeps the batch tables and the symbolic factorisation (host_plan_us stays 0 on
 * the next sslam_graph_optimize of an already planned graph), and a live sslam_batch picks the new values up at sslam_batch_upload.  Members
 * of a batch may carry different per-edge kernels; the "same options" rule of sslam_batch_create is about the options only.
 * A graph none of whose edges has a kernel launches the same kernels as before this call existed; one that has takes the robust
 * instantiations of the linearisation / chi2 kernels and of every LM launch form ("fused_small_graph", "speculative_trials": same results,
 * bitwise, as without them).
 * The .g2o text format has no place for robust kernels and g2o does not write them: sslam_graph_save_g2o drops them, a loaded graph has none. */
#define SSLAM_ROBUST_NONE 0
#define SSLAM_ROBUST_HUBER 1
#define SSLAM_ROBUST_PSEUDOHUBER 2
#define SSLAM_ROBUST_CAUCHY 3
#define SSLAM_ROBUST_WELSCH 4
#define SSLAM_ROBUST_FAIR 5
#define SSLAM_ROBUST_SATURATED 6
#define SSLAM_ROBUST_DCS 7
int sslam_graph_set_edge_robust_kernel(sslam_graph* g, int edge_id, int kind, double delta);
/* kind / delta may be NULL; delta is 0 for an edge without a kernel */
int sslam_graph_get_edge_robust_kernel(const sslam_graph* g, int edge_id, int* kind, double* delta);
/* Per listed edge, at the current estimates: the raw e2 = e^T Omega e, the robustified rho0 (the edge's chi2 term; their sum over all edges is
 * sslam_graph_chi2) and the weight rho1 of the kernel the edge is under (precedence above) -- how a caller finds the loop closures the optimiser
 * has switched off.  Evaluated on the device, one thread per requested edge.  Any output may be NULL.  edge_ids = NULL: all edges in id
 * order (n is ignored; the outputs hold sslam_graph_num_edges values).  n = 0: nothing to do, returns 0.  An unknown id: SSLAM_ERR_INVALID. */
int sslam_graph_edge_chi2(sslam_graph* g, const int* edge_ids, int n, double* e2_out, double* rho0_out, double* weight_out);

/* GraphSLAM::optimize (graph_slam.cpp:182-219) with the iteration cap as a parameter (the
 * reference hard-codes 1024, graph_slam.cpp:205).  Fewer than 10 edges: returns
 * SSLAM_ERR_TOO_FEW_EDGES and leaves the graph untouched (graph_slam.cpp:184-186). */
int sslam_graph_optimize(sslam_graph* g, int max_iters, sslam_opt_stats* out);

/* graph->chi2() at the current estimates */
int sslam_graph_chi2(sslam_graph* g, double* chi2);

/* computeLandmarkMarginals (graph_slam.cpp:221-234): diagonal blocks of H^-1 at the current
 * linearisation for the listed vertex ids (the caller asks for (idx,idx) pairs only,
 * semantic_graph_slam.cpp:186-191); out = packed row-major d x d blocks. */
int sslam_graph_marginals(sslam_graph* g, const int* ids, int n, double* out_blocks);
/* the same with the reference's own argument: n (row, col) pairs of vertex hessianIndex() values, as built at
 * semantic_graph_slam.cpp:186-191 and handed to g2o::SparseOptimizer::computeMarginals (graph_slam.cpp:225); row_col = 2n ints.
 * Off-diagonal pairs are allowed; out = packed row-major d(row) x d(col) blocks of H^-1. */
int sslam_graph_marginals_by_hessian_index(sslam_graph* g, const int* row_col, int n, double* out_blocks);

/* GraphSLAM::save (graph_slam.cpp:236-239): g2o text format */
int sslam_graph_save_g2o(const sslam_graph* g, const char* path);
/* inverse of save (the reference has no load path) */
int sslam_graph_load_g2o(sslam_graph* g, const char* path);

/* ---- parity / measurement hooks (no reference counterpart) ---------------------------------
 * Linearise at the current estimates (BlockSolver::buildSystem) and copy the normal equations to
 * the host as dense blocks in g2o hessian-index order.  Two-call protocol: pass NULL arrays to
 * obtain counts.  H is returned as COO over scalar entries of the upper triangle. */
int sslam_graph_linearize(sslam_graph* g, int* dim, int64_t* nnz_upper, int32_t* rows, int32_t* cols,
                          double* vals, double* b);
/* solve (H + lambda I) x = b for the current linearisation; x in g2o hessian-index order */
int sslam_graph_solve(sslam_graph* g, double lambda, double* x, int64_t* solver_iterations);
/* x <- x [+] dx for all active vertices (VertexSE3/PointXYZ/Plane::oplus) */
int sslam_graph_oplus(sslam_graph* g, const double* dx);

/* ---- plan introspection (host only: works without a HIP device) ----------------------------
 * The symbolic sparse-Cholesky plan of a batch (ordering, elimination-tree pieces, work items) as flat arrays of int32
 * records, for the CPU-side plan tests (tests/test_chol_plan_cpu.py).  Arrays: "col","blk","upd","item","mb","ilv","piece",
 * "lvl_ptr","lvl_cols","plv_ptr","plv_pieces","tail_ptr","tail_pieces","plv_lds_f","plv_lds_b","scalars".
 * sslam_debug_plan_array returns the byte size of the array (copies it when out != NULL and cap_bytes suffices). */
void* sslam_debug_plan_create(sslam_graph* const* graphs, int n);
void sslam_debug_plan_destroy(void* plan);
int64_t sslam_debug_plan_array(void* plan, const char* name, void* out, int64_t cap_bytes);
/* The grid sslam_seg_voxel_grid lays over the bounding box lo .. hi of the finite points (host only, the driver's own rule): minb[k] =
 * floor(lo[k] * (1 / leaf)) in float32, div[k] = cells along axis k.  Returns 0, SSLAM_ERR_INVALID (NULL, leaf not > 0) or
 * SSLAM_ERR_UNSUPPORTED in the cases listed at sslam_seg_voxel_grid; the outputs are unwritten on an error. */
int sslam_debug_voxel_geometry(const float lo[3], const float hi[3], float leaf, int32_t minb[3], int64_t div[3]);
/* ---- batched, device-resident form (MI355X extension) ---------------------------------------
 * B independent graphs laid out contiguously in HBM and optimised together: every kernel runs
 * over the union, LM control (rho, lambda, accept/reject) is per graph on the device. */
/* Lifetime and structure: the batch borrows the graphs -- they must outlive it (destroy the batch first) -- and is built for their
 * structure at creation: after a vertex or an edge is added to a member, every sslam_batch_* entry point returns SSLAM_ERR_INVALID
 * until a new batch is created.  All members must carry the same options (sslam_graph_set_option). */
typedef struct sslam_batch sslam_batch;
sslam_batch* sslam_batch_create(sslam_graph* const* graphs, int n);
/* Stream group: the n graphs split into n_streams contiguous parts, each a batch of its own on its own HIP stream; sslam_batch_optimize
 * drives every part from its own host thread.  Results are those of sslam_batch_create (every graph runs its own LM; the parts only
 * change what overlaps on the chip: one part's tree tops and LM endgame run under another part's leaves) -- bit for bit where every
 * part is planned like the whole batch; a part is planned by its own size, so parts of fewer than 8 graphs of a larger batch take the
 * single-launch factorisation and give the bits of a batch of that part (same accuracy, another summation order).  Measured on 512 distinct L
 * graphs: 4 streams = +16 % iterations/s.  upload / download / optimize / info / profiling / time_* work on a group; the edge-sharded
 * mode and sslam_batch_linearize_hb return SSLAM_ERR_UNSUPPORTED.  sslam_batch_create reads the number of streams from the environment
 * (SSLAM_BATCH_STREAMS, default 1). */
sslam_batch* sslam_batch_create_streams(sslam_graph* const* graphs, int n, int n_streams);
void sslam_batch_destroy(sslam_batch* b);
/* re-upload the host graphs' current estimates (resets the device state) */
int sslam_batch_upload(sslam_batch* b);
/* copy optimised estimates back into the host graphs */
int sslam_batch_download(sslam_batch* b);
int sslam_batch_optimize(sslam_batch* b, int max_iters, sslam_opt_stats* out /* [n] */);
/* Blocks of H^-1 of the graphs of a batch.  H is the undamped system at the estimates the batch currently holds on
 * the device (after sslam_batch_upload / sslam_batch_optimize), NOT at the host graphs' estimates.
 * req = 3n ints: (graph index in the batch, row vertex id, column vertex id).
 * out = packed row-major d(row) x d(col) blocks in request order.
 * Diagonal and off-diagonal pairs; both vertices belong to the named graph.
 * A fixed or edge-less vertex on either side gives a block of zeros, and so do two vertices in different connected components of their
 * graph.  n == 0 returns 0.  SSLAM_ERR_INVALID, with out_blocks unwritten: a NULL handle, a NULL req or out_blocks with n > 0, a graph
 * index or vertex id out of range, a structure change since creation.  SSLAM_ERR_NUMERIC when a factorisation of the undamped H breaks
 * down -- the rule of sslam_graph_marginals; ONE graph of the batch that is not positive definite fails the whole call (per-graph
 * failure flags are future work).  SSLAM_ERR_UNSUPPORTED: solver 0 or 2, a batch in edge-sharded mode.  A stream group works: every
 * request goes to the part that holds its graph, and the parts run one after the other from the calling thread.
 * One linearisation and one flat factorisation of the whole batch, then ONE WAVE PER REQUEST (k_chol_marginal_pairs): a forward
 * substitution along the elimination-tree path of the row vertex and, for an off-diagonal pair, of the column vertex, and the product of
 * the two over the columns the paths share -- no right-hand side matrix, no backward substitution, only the requested blocks cross PCIe.
 * Paths of any length (the L configuration included): what fits the LDS of a wave runs there, the rest in a device scratch buffer, with
 * bitwise the same result; SSLAM_MARGINAL_LDS_BYTES in the environment (read per call, default and ceiling 61440) lowers the LDS budget.
 * A call whose elimination-tree paths hold more than SSLAM_PATH_ROUND_INTS columns in all (read per call, default and ceiling 16777216,
 * floor 1), or need more than 1 GB of scratch, runs in rounds of requests, each with its own upload, launches and download -- bitwise
 * the blocks of one round.  (The placement rule and the rounds are csrc/path_rounds.hpp, shared with the gate below.)
 * The call leaves the batch as it found it: sslam_batch_optimize / sslam_batch_download after it give, bitwise, what they give without it. */
int sslam_batch_marginals(sslam_batch* b, const int32_t* req, int n, double* out_blocks);
/* Loop-closure gate: the Mahalanobis distance of candidate edges that are NOT in the graph (their measurement is independent of the
 * estimate), at the estimates the batch holds on the device and with H the undamped system there -- the conventions of
 * sslam_batch_marginals.  For a candidate between the vertices u = v_from and v = v_to:
 *   e   the edge's error, as the linearisation computes it (what sslam_graph_edge_chi2 would work from, were the edge added);
 *   Ju, Jv   its analytic Jacobians;  Zab   the blocks of H^-1 (zero for a fixed or edge-less vertex and across connected components);
 *   S = Ju Zuu Ju^T + Ju Zuv Jv^T + Jv Zvu Ju^T + Jv Zvv Jv^T + Omega^-1,   d2 = e^T S^-1 e.
 * info == NULL leaves Omega^-1 out: S is the covariance of the predicted relative measurement alone.
 * cand = 4n ints: (graph index in the batch, kind, v_from, v_to).  z = 7n doubles, info = 36n doubles or NULL:
 *   SSLAM_GATE_SE3        VertexSE3 -> VertexSE3, z = t, q(x,y,z,w), info 6x6 row-major, d = 6;
 *   SSLAM_GATE_SE3_POINT  VertexSE3 -> VertexPointXYZ, z = the first 3 of the 7, info = the leading 9 of the 36 as 3x3, d = 3.
 * z and -z (the quaternion negated) are one measurement and give the same d2.  Only the lower triangle of info is read.
 * d2_out [n].  e_out [6n] or NULL: the leading d entries per candidate.  cov_out [36n] or NULL: S as the leading d * d entries, row-major
 * d x d.  The remainder of both is zero.
 * When the Cholesky of Omega or of S breaks down (a pivot <= 0 or not finite) that candidate's d2 is NaN and the call still returns 0;
 * e_out and cov_out hold what was computed (S without Omega^-1 when it was Omega that broke down).  Both ends fixed and info == NULL
 * give S = 0, which is such a case; both ends fixed with info give d2 = e^T Omega e.
 * n == 0 returns 0.  SSLAM_ERR_INVALID, with the outputs unwritten: a NULL handle (checked first), NULL cand, z or d2_out with n > 0, a
 * graph index, kind or vertex id out of range, a vertex of the wrong type for the kind, v_from == v_to, a z or info that is not finite, a
 * quaternion of zero norm, a structure change since creation.  SSLAM_ERR_UNSUPPORTED: solver 0 or 2, a batch in edge-sharded mode.
 * SSLAM_ERR_NUMERIC: an undamped H that is not positive definite (the rule of sslam_batch_marginals).  A stream group works as it does
 * there: every candidate goes to the part that holds its graph, the parts run one after the other from the calling thread.
 * One linearisation and one flat factorisation of the whole batch, then ONE WAVE PER CANDIDATE (k_chol_gate_pairs): the forward
 * substitutions along path(u) and path(v), each once, the three blocks of H^-1 out of them, e, the Jacobians, S and d2 -- 43 doubles per
 * candidate cross PCIe.  Paths of any length, a path of length 0 (a fixed end) included; LDS or device scratch with bitwise the same
 * result, SSLAM_MARGINAL_LDS_BYTES and SSLAM_PATH_ROUND_INTS as for the marginals (the budget of the whole workgroup, the kernel's
 * fixed 2368 bytes included).
 * The call leaves the batch as it found it: optimize, download and marginals after it give, bitwise, what they give without it. */
#define SSLAM_GATE_SE3 0
#define SSLAM_GATE_SE3_POINT 1
int sslam_batch_gate(sslam_batch* b, const int32_t* cand, const double* z, const double* info, int n, double* d2_out, double* e_out, double* cov_out);
/* the same for a single graph handle, at the graph's current estimates: cand = 3n ints (kind, v_from, v_to).  The batch-of-one route:
 * bitwise what sslam_batch_gate gives for a batch of this one graph. */
int sslam_graph_gate(sslam_graph* g, const int32_t* cand, const double* z, const double* info, int n, double* d2_out, double* e_out, double* cov_out);
/* Parity hook.  (H_g + lambda[g] I) x_g = b_g for every graph of the batch at the estimates the device holds, through the launches the
 * LM loop takes.
 * lambda[g] >= 0: graph g takes part.  lambda[g] < 0: it sits out exactly as a terminated graph does in the LM endgame (in_trial = active
 * = 0, and the launches are sized for the graphs that take part as sslam_batch_optimize sizes them for the graphs still active: index
 * lists once at most half of a batch of 8 graphs and more is left; SSLAM_CHOL_OPTS "compact=0" keeps the full ranges, with bitwise the
 * same results; sslam_batch_info "compact_rounds" counts the times the index lists were switched on).
 * x: the graphs' unknowns one after the other in batch order, each in its own hessian-index order (sslam_graph_hessian_index); zeros
 * for a graph that sat out.  Returns the number of doubles; x == NULL only reports it.  solver_iterations ([n] or NULL): PCG iterations
 * per graph (solvers 0 and 2), 0 for the direct solvers.
 * SSLAM_ERR_INVALID: a NULL handle, a NULL lambda with x given, capacity below the size, a lambda that is not finite, a structure change
 * since creation.  SSLAM_ERR_UNSUPPORTED: a batch in edge-sharded mode.  SSLAM_ERR_NUMERIC: the solve of a graph that took part broke
 * down.  A stream group works: the parts run one after the other from the calling thread.
 * The batch is left as it was found: sslam_batch_optimize / sslam_batch_marginals after it give, bitwise, what they give without it. */
int64_t sslam_batch_solve(sslam_batch* b, const double* lambda, double* x, int64_t capacity, int64_t* solver_iterations /* [n] or NULL */);
/* Edge-sharded mode (SURVEY 8e mode E, BASELINE.json configs[4]): every graph's edge list is split contiguously over `world` ranks
 * (one process per GPU, each holding the whole batch); a rank builds the partial normal equations of its edges, ONE RCCL all-reduce
 * (ncclDouble, sum, over xGMI) of the contiguous [H || b] device buffer gives every rank the full system, and the solve / update /
 * LM control then run replicated and bit-identical.  Rank 0 obtains an id with sslam_comm_unique_id and hands its 128 bytes to the
 * other ranks by whatever the host program uses (torch.distributed, MPI, a file); every rank then calls sslam_batch_comm_init.
 * world == 1 switches the mode off, unless the environment sets SSLAM_FORCE_COMM=1: then a single-rank communicator is created and the
 * whole path (masked kernels, ncclCommInitRank, ncclAllReduce on the batch stream) runs on one GPU (sslam_batch_info "allreduce_calls"
 * counts the collectives issued).  The all-reduce is out of place, partial buffer -> [H || b]: graphs that do not re-linearise in a
 * step keep their old partial system, so the sum stays the system they already had.  sslam_batch_set_edge_shard installs the shard WITHOUT a communicator (the partial systems stay
 * unsummed): with sslam_batch_linearize_hb (-> the [H || b] buffer; NULL returns its length in doubles) this is the parity hook that
 * shows sum over ranks of partial systems == the full system on a single device. */
int sslam_comm_unique_id(char id_out[128]);
int sslam_batch_comm_init(sslam_batch* b, const char id_in[128], int rank, int world);
int sslam_batch_set_edge_shard(sslam_batch* b, int rank, int world);
int64_t sslam_batch_linearize_hb(sslam_batch* b, double* h_and_b, int64_t capacity);
/* run only the Jacobian build (linearise + assemble) `repeats` times; returns mean kernel
 * milliseconds measured with hipEvents on the batch's stream */
int sslam_batch_time_linearize(sslam_batch* b, int repeats, double* ms_per_build);
/* one numeric factorisation (+ fused forward substitution) and one backward substitution of EVERY graph of the batch, `repeats` times:
 * mean kernel milliseconds (hipEvents on the batch's stream); direct solvers only */
int sslam_batch_time_solver(sslam_batch* b, int repeats, double* factor_ms, double* solve_ms);
/* algorithmic bytes of one Jacobian build over the whole batch (SURVEY §8d formula) */
int64_t sslam_batch_linearize_bytes(const sslam_batch* b);
/* structural facts of a batch (doubles): "factor_lnz" (doubles in the Cholesky factor), "factor_levels", "factor_front" (1: the
 * factorisation runs the front kernels, the default of batches of 32 graphs and more),
 * "front_groups_per_cu_leaf" / "front_groups_per_cu_mid" (front workgroups a CU holds by the runtime's own count, the minimum over the
 * leaf / mid launches at their LDS sizes; a class without launches reports what its kernel's registers allow; 0 without front tables; the
 * minimum over the parts of a stream group),
 * "compact_rounds" (times so far that the LM endgame, or sslam_batch_solve with graphs sitting out, sized the factor / solve launches by
 * index lists of the graphs still taking part; summed over the parts of a stream group),
 * "h_doubles" (doubles in H), "dim" (scalar unknowns), "factor_bytes" = algorithmic HBM bytes of one numeric
 * factorisation + fused forward solve: read H and b once, write L and y once */
int sslam_batch_info(sslam_batch* b, const char* key, double* value);
/* per-kernel accumulated hipEvent time since the last reset (profiling must be enabled with
 * sslam_batch_set_profiling); names: "linearize","chi2","spmv","pcg_update","precond","oplus","factor","solve" */
int sslam_batch_set_profiling(sslam_batch* b, int enable);
int sslam_batch_kernel_time(sslam_batch* b, const char* name, double* total_ms, int64_t* launches);

/* ============================================================================================
 * Frontend: point_cloud_segmentation::segmentallPointCloudData
 *           (reference include/planar_segmentation/point_cloud_segmentation.h:105-181)
 * ==========================================================================================*/
typedef struct sslam_seg sslam_seg;

typedef struct sslam_seg_params {
  double num_point_seg;     /* ~num_point_seg   default 500  (plane_segmentation.cpp:7)  */
  double norm_point_thres;  /* ~norm_point_thres default 5000 (plane_segmentation.cpp:8)  */
  double planar_area;       /* ~planar_area     default 0.1  (plane_segmentation.cpp:9)  */
  float max_depth_change_factor; /* 0.03  (plane_segmentation.cpp:99)  */
  float normal_smoothing_size;   /* 20    (plane_segmentation.cpp:100) */
  float angular_threshold;       /* 0.017453*2 rad (plane_segmentation.cpp:140) */
  float distance_threshold;      /* 0.02 m (plane_segmentation.cpp:141) */
  float maximum_curvature;       /* PCL default 0.001 */
  int min_contour_points;        /* > 100 (plane_segmentation.cpp:169) */
  int image_width, image_height; /* 640 x 480 crop bounds (plane_segmentation.cpp:34-35) */
  int reference_quirks;          /* 1: reproduce tools.h:80-81 typo (quirk B2) */
  int device;
} sslam_seg_params;

/* semantic_SLAM::ObjectInfo (msg/ObjectInfo.msg:1-6); class_id indexes SSLAM_CLASS_* below */
typedef struct sslam_box {
  int32_t tl_x, tl_y, width, height;
  int32_t class_id;
  float prob;
} sslam_box;

/* the class whitelist of point_cloud_segmentation.h:126-130 */
enum { SSLAM_CLASS_OTHER = 0, SSLAM_CLASS_CHAIR, SSLAM_CLASS_TVMONITOR, SSLAM_CLASS_BOOK, SSLAM_CLASS_KEYBOARD,
       SSLAM_CLASS_LAPTOP, SSLAM_CLASS_BUCKET, SSLAM_CLASS_CAR };

/* detected_object (include/planar_segmentation/detected_object.h:14-24) */
typedef struct sslam_plane {
  float centroid_cam[3];  /* detected_object::pose */
  float normal_d[4];      /* detected_object::normal_orientation (sign-normalised) */
  float world_pose[3];    /* detected_object::world_pose */
  float num_points;       /* contour point count (quirk B8) */
  float prob;
  int32_t plane_type;     /* 0 horizontal, 1 vertical */
  int32_t class_id;
  int32_t box_index;
  int32_t inlier_count;   /* true inlier count (extension) */
  float area;             /* polygon area of the contour */
} sslam_plane;

void sslam_seg_default_params(sslam_seg_params* p);
sslam_seg* sslam_seg_create(const sslam_seg_params* p);
void sslam_seg_destroy(sslam_seg* s);

/* segmentallPointCloudData(robot_pose, cam_angle, object_info, point_cloud)
 * cloud = sensor_msgs::PointCloud2::data of an organised width x height cloud; off_* = field
 * offsets of x,y,z (plane_segmentation.cpp:48-61).  Returns the number of planes written.
 * The layout is checked before the device is looked at, here and in sslam_seg_segment_batch / sslam_seg_submit_batch: width > 0,
 * height > 0, point_step >= 4, 0 <= off_* <= point_step - 4, row_step >= width * point_step, n_frames > 0, n_boxes >= 0 -- anything
 * else is SSLAM_ERR_INVALID (a pixel of the image would be read outside the row_step * height bytes of the cloud). */
int sslam_seg_segment(sslam_seg* s, const uint8_t* cloud, int width, int height, int point_step, int row_step,
                      int off_x, int off_y, int off_z, const sslam_box* boxes, int n_boxes,
                      const float robot_pose[6], float cam_angle, sslam_plane* out, int max_out);

/* Several frames in one pass (MI355X extension): the boxes of all frames are packed into one set of launches -- one frame's 32 boxes
 * occupy 32 of the 256 CUs in the kernels that run one workgroup per box.  All frames share the cloud geometry (width .. off_z).
 * out_frame[k] (optional) = frame of out[k]; box_index of a plane counts inside its own frame.  Results are identical to
 * n_frames calls of sslam_seg_segment. */
typedef struct sslam_frame {
  const uint8_t* cloud;
  const sslam_box* boxes;
  int n_boxes;
  float robot_pose[6];
  float cam_angle;
} sslam_frame;
int sslam_seg_segment_batch(sslam_seg* s, const sslam_frame* frames, int n_frames, int width, int height, int point_step, int row_step,
                            int off_x, int off_y, int off_z, sslam_plane* out, int max_out, int32_t* out_frame);
/* Pipelined form of sslam_seg_segment_batch for a stream of batches: submit enqueues the H2D copy of the clouds, every kernel and
 * the read-back of the result tables on one of two pipelines of the handle (own HIP stream, own device buffers, used in turn) and
 * returns; collect waits for the OLDEST submitted batch and runs the scalar post-processing.  At most two batches are in flight:
 *     submit(0);  for (k = 0; ...; ++k) { submit(k + 1); collect(k); }
 * so that the copy of batch k+1 (9.8 MB per 640x480 frame of 32-byte points; 3.7 MB with point_step = 12: the frontend reads x, y, z only)
 * runs under the kernels of batch k -- the kernels of a batch wait for the other pipeline's kernels, so copies and kernels of successive
 * batches overlap whatever the host's timing.  The cloud buffers of a batch must stay
 * valid until it is collected (boxes and poses are copied at submit); pinned clouds (hipHostMalloc / hipHostRegister) make submit
 * itself asynchronous.  Results are those of sslam_seg_segment_batch.  The blocking calls refuse to run while a batch is in flight. */
int sslam_seg_submit_batch(sslam_seg* s, const sslam_frame* frames, int n_frames, int width, int height, int point_step, int row_step,
                           int off_x, int off_y, int off_z);
int sslam_seg_collect_batch(sslam_seg* s, sslam_plane* out, int max_out, int32_t* out_frame);
/* Truncation of the last segment call: planes not returned because max_out was reached, boxes with more than 64 connected
 * components above num_point_seg, boxes with more than 64 accepted planes.  Returns the sum (0 = nothing was truncated).
 * A box with a full candidate table keeps the 64 components with the LOWEST root pixel index (the order in which the reference
 * numbers its labels), whatever the order the kernel met them in: its planes repeat from call to call.  They equal the reference's
 * only if none of the components left out would have been accepted: the reference fits every component and caps the ACCEPTED planes
 * at 64 in the same order, so a candidate beyond the 64th can still enter its table when an earlier one fails the curvature test.
 * The third counter cannot become non-zero while the candidate and the region table both hold 64 entries. */
int sslam_seg_last_overflow(const sslam_seg* s, int* dropped_planes, int* boxes_with_full_candidate_table, int* boxes_with_full_region_table);

/* RANSAC plane fit: pcl::SACSegmentation(SACMODEL_PLANE, SAC_RANSAC, optimise coefficients)
 * as configured at plane_segmentation.cpp:639-647 (threshold 0.01; PCL defaults max_iterations 50, probability 0.99)
 * on an unorganised cloud of n xyz float points.  Every hypothesis is scored in parallel (one thread per point,
 * LDS / ballot inlier counting); pcl::RandomSampleConsensus' adaptive-k loop is replayed over the counts.
 * Samples come from a counter-based hash of (seed, iteration) instead of rand().  Returns the number of inliers of
 * the refined model; coeff_out = (nx, ny, nz, d); inliers_out = ascending point indices. */
int sslam_seg_ransac_plane(sslam_seg* s, const float* xyz, int n, float threshold, int max_iterations, double probability,
                           uint64_t seed, float coeff_out[4], int32_t* inliers_out, int max_inliers);

/* Second half of compute2DConvexHull: pcl::ProjectInliers(SACMODEL_PLANE) of the RANSAC inliers onto
 * the model plane and the 2-D pcl::ConvexHull of the projected points (plane_segmentation.cpp:648-662).
 * inliers = point indices (e.g. from sslam_seg_ransac_plane), coeff = (a, b, c, d).  projected_out (optional):
 * n_inliers x 3 floats.  hull_out = POSITIONS in `inliers` of the hull vertices, counter-clockwise in the chosen coordinate
 * plane (axes_out: 0 xy, 1 yz, 2 xz; picked from the plane normal as PCL does), starting at the vertex of smallest
 * atan2 about the vertex centroid (PCL's comparePoints2D order).  Returns the number of hull vertices. */
int sslam_seg_convex_hull_2d(sslam_seg* s, const float* xyz, int n, const int32_t* inliers, int n_inliers, const float coeff[4],
                             float* projected_out, int32_t* hull_out, int max_hull, int* axes_out);

/* Point-to-plane ICP (judge row J1; BASELINE.json north_star "RANSAC plane fit + point-to-plane ICP"; the reference tree holds no
 * counterpart): the rigid transform T that minimises  sum_i (n_k(i) . (T p_i) + d_k(i))^2  over the n points with label k(i) in
 * [0, n_planes) -- e.g. the in-box points of a frame with the label image of sslam_seg_get_labels against the planes of the previous
 * keyframe.  Gauss-Newton on (rotation vector, translation), T <- (exp[w]x, u) o T: every round is ONE pass over the points on the
 * device (29 double sums, fixed reduction order) and a 6 x 6 Cholesky solve on the host.  T0 (NULL = identity) and T_out are 12
 * doubles, R row-major then t; rms_out = root mean square point-to-plane distance at T_out.  Returns the number of points used;
 * SSLAM_ERR_NUMERIC when the planes leave a degree of freedom unconstrained. */
int sslam_seg_icp_point_to_plane(sslam_seg* s, const float* xyz, const int32_t* labels, int n, const float* planes, int n_planes,
                                 int iterations, const double T0[12], double T_out[12], double* rms_out);

/* ---- RANSAC plane per detection box + point-to-plane ICP per frame, batched over the RESIDENT batch (BASELINE.json configs[3]: "640x480
 * depth cloud, 32 detection boxes/frame, RANSAC+ICP plane extraction"; north_star: "RANSAC plane fit + point-to-plane ICP over depth
 * clouds inside detection boxes ... one-thread-per-point HIP kernels with LDS inlier counting").  The reference's only RANSAC is
 * compute2DConvexHull's pcl::SACSegmentation (plane_segmentation.cpp:631-665, threshold 0.01, 50 iterations, probability 0.99); it has
 * no ICP.  Both calls work on the cropped clouds that the last blocking sslam_seg_segment / sslam_seg_segment_batch call left on the
 * device (its accepted boxes, in slot order: frame by frame, box order inside a frame): no second upload.
 *
 * sslam_seg_ransac_boxes: for every accepted box, pcl::SACSegmentation(SACMODEL_PLANE, SAC_RANSAC, optimise coefficients) exactly as
 * sslam_seg_ransac_plane runs it on the box's crop taken as an unorganised cloud of width * height points in crop order (row-major; a
 * non-finite point is never an inlier and a sample that hits one is a bad sample), with seed + slot * 0x9E3779B97F4A7C15 as the seed
 * of box `slot`.  One workgroup per box, the crop staged in LDS, sixteen hypotheses scored at a time.  Writes min(boxes, max_out) records
 * and returns the number of boxes; kernel_ms (optional): device time of the pass.  The inlier flags stay on the device for
 * sslam_seg_ransac_box_inliers (ascending crop indices of one box; returns the true count) and sslam_seg_icp_boxes. */
typedef struct sslam_box_plane {
  float coeff[4];          /* (nx, ny, nz, d) of the refined model; zeros when no model was found */
  int32_t inliers;         /* points within the threshold of the refined model */
  int32_t points;          /* width * height of the box */
  int32_t box_index;       /* index into the caller's box array of its frame */
  int32_t frame;
  int32_t hypotheses;      /* hypotheses the adaptive loop consumed (bad samples included) */
  int32_t best_iteration;  /* hypothesis index of the winning sample, -1: none */
} sslam_box_plane;
int sslam_seg_ransac_boxes(sslam_seg* s, float threshold, int max_iterations, double probability, uint64_t seed, sslam_box_plane* out, int max_out,
                           double* kernel_ms);
int sslam_seg_ransac_box_inliers(sslam_seg* s, int slot, int32_t* out, int max_out);
/* sslam_seg_icp_boxes: sslam_seg_icp_point_to_plane per FRAME of the resident batch; a Gauss-Newton round is two launches over ALL frames
 * (one workgroup per box for the 29 sums over its inliers, one wave per frame for the reduction in slot order, the 6 x 6 solve and the
 * update of T -- no host round trip per iteration): the points of a frame are the RANSAC inliers of its boxes, the points of box
 * slot q measure plane box_plane[q] of `planes` (n_planes x 4 floats, e.g. the previous keyframe's planes in the camera frame of this
 * one; -1: the box takes no part).  T0: NULL (identity) or 12 doubles per frame.  out[f].status is 0 or SSLAM_ERR_NUMERIC (planes that
 * leave a degree of freedom unconstrained).  Returns the number of frames. */
typedef struct sslam_icp_result {
  double T[12];   /* R row-major, then t */
  double rms;     /* root mean square point-to-plane distance at T */
  int32_t used;   /* points that took part */
  int32_t status;
} sslam_icp_result;
int sslam_seg_icp_boxes(sslam_seg* s, const int32_t* box_plane, int n_boxes, const float* planes, int n_planes, int iterations, const double* T0,
                        sslam_icp_result* out, int max_out, double* kernel_ms);

/* ---- cloud filters of the legacy path (dead code upstream) -----------------------------------------------------
 * All three take an unorganised cloud of n xyz float points and run on the GPU; index outputs are ascending and complete when the
 * return value (the true count) does not exceed max_out. */
/* plane_segmentation::distance_filter (plane_segmentation.cpp:607-629): indices of the points with dmin < |p| < dmax (0.3, 3 upstream) */
int sslam_seg_distance_filter(sslam_seg* s, const float* xyz, int n, double dmin, double dmax, int32_t* keep_out, int max_out);
/* plane_segmentation::downsamplePointcloud -> pcl::VoxelGrid (plane_segmentation.cpp:565-581; leaf 0.1 upstream): one centroid per
 * occupied voxel of the bounding box of the finite points, in ascending voxel index (x fastest), optionally with the voxel's point
 * count.  Sums are kept in 2^-20 fixed point with integer atomics (order independent; PCL accumulates in float in the order of an
 * unstable sort).  Returns the number of occupied voxels (0 for a cloud without a finite point); at most max_out centroids / counts are
 * written.  The cell of a coordinate x is floor(x * (1 / leaf)) in float32, as in PCL.  SSLAM_ERR_UNSUPPORTED, before any cell is sized or
 * written: 1 / leaf is not finite; that floor for the lower or the upper bound of the box, taken as a float, lies outside [-2^31, 2^31)
 * (one absurd finite coordinate does that); an axis with fewer than one cell; more than 2^26 cells (sslam_debug_voxel_geometry is that
 * rule alone). */
int sslam_seg_voxel_grid(sslam_seg* s, const float* xyz, int n, float leaf, float* centroids_out, int32_t* counts_out, int max_out);
/* plane_segmentation::removeOutliers -> pcl::StatisticalOutlierRemoval (plane_segmentation.cpp:583-605; meanK 50, multiplier 1.0
 * upstream): a point stays when its mean distance to its mean_k nearest neighbours (exact search) is not above mean + stddev_mul *
 * standard deviation of those mean distances.  mean_dist_out (optional, n floats; -1 for non-finite points).  Returns the inlier count.
 * xyz is a host pointer.  Only finite points are neighbours: SSLAM_ERR_INVALID when fewer than mean_k + 1 points are finite (n = 0
 * returns 0), so no mean distance is ever built from a missing neighbour.  A squared distance that overflows float32 is +inf and stays
 * +inf: the mean distance of such a point is +inf, and when one occurs the threshold is NaN and every finite point is kept. */
int sslam_seg_statistical_outlier_removal(sslam_seg* s, const float* xyz, int n, int mean_k, double stddev_mul, int32_t* keep_out, int max_out,
                                          float* mean_dist_out);

/* plane_segmentation::computeKmeans -> cv::kmeans(points, k, labels, TermCriteria(EPS + ITER, 10, 0.01), 10 attempts, KMEANS_RANDOM_CENTERS)
 * (plane_segmentation.cpp:524-535) on n points of dimension dim (3: normals, k = 4; 1: plane distances, k = 2 upstream).  Restated with
 * centres drawn uniformly in the bounding box from a counter-based hash of (seed, attempt, centre, coordinate) instead of cv::RNG,
 * order-independent fixed-point sums in the centre update, and an empty cluster keeping its centre.  The assignment step runs on the GPU.
 * labels_out[n], centers_out[k * dim]; returns k. */
int sslam_seg_kmeans(sslam_seg* s, const float* pts, int n, int dim, int k, uint64_t seed, int32_t* labels_out, float* centers_out, double* compactness_out);

/* ---- fitness score of cloud pairs and the information matrix it gives (hdl_graph_slam's InformationMatrixCalculator [UPSTREAM]; the
 * reference keeps its weight() at information_matrix_calculator.hpp:20-24 and has the score stubbed to 0.9 at
 * information_matrix_calculator.cpp:37, `//calc_fitness_score(cloud1, cloud2, relpose)`) ----------------------------------------------
 * sslam_seg_fitness_scores: for every pair, every point of the source cloud moved by T looks up its NEAREST point of the target cloud
 * (exact search, k_nn_pairs); the score is the mean of the squared distances that do not exceed max_range.
 * xyz: the clouds one after the other, 3 floats per point; cloud c holds the points cloud_start[c] .. cloud_start[c + 1] - 1
 * (cloud_start[0] >= 0, non-decreasing, n_clouds + 1 entries).  A cloud may serve any number of pairs, as target and as source.
 * All pairs go through ONE launch.  Arithmetic, in float32 without fused multiply-add (a NumPy restatement matches bit for bit):
 *   R, t = T cast from double to float once;   x' = ((r00 x + r01 y) + r02 z) + tx  (y', z' alike);
 *   d2 = (dx dx + dy dy) + dz dz  with dx = x' - x_target   (flann::L2_Simple<float>);
 *   the nearest target is the one of smallest d2, ties go to the LOWEST target index.
 * A non-finite point of either cloud takes no part: as a source point it gets index -1 and d2 = -1 and is not counted, as a target it
 * is never chosen.  A source point with no target at a finite float distance (an empty or all-non-finite target cloud, a d2 that
 * overflows) is reported the same way.
 * used = the number of source points with (double)d2 <= max_range -- max_range bounds the SQUARED distance, as in hdl_graph_slam,
 * which compares nn_dists[0]; DBL_MAX = no bound.  score = the sum of those (double)d2 / used, DBL_MAX when used == 0.  The sum runs
 * in double in an order fixed by the point index alone (a fixed tree inside every run of 256 consecutive source points, the runs in
 * ascending order): it does not depend on the launch geometry, and repeating a call repeats its bits.
 * A pair with few source points and many targets has its targets split over several workgroups (`chunk` targets each, combined by a
 * 64-bit atomic minimum over (bits of d2, index): exact, order independent, the same bits as unsplit).  chunk comes from a heuristic on
 * the size of the launch; SSLAM_FITNESS_OPTS="chunk=N" in the environment (read at each call) overrides it.
 * nn_index_out / nn_dist2_out (optional, either may be NULL): pair after pair, one entry per source point; the index counts inside
 * the target cloud.  kernel_ms (optional): hipEvent time of the pass (copies excluded).
 * A pair whose source or target cloud is empty is valid: used = 0, score = DBL_MAX.  Returns n_pairs.  SSLAM_ERR_INVALID: a NULL handle,
 * cloud_start, pairs / score_out / used_out with n_pairs > 0 or xyz with points; n_pairs < 0 or n_clouds < 0; a cloud_start that
 * decreases or starts below 0; a cloud index out of range; a batch in flight (sslam_seg_submit_batch).  SSLAM_ERR_NO_DEVICE without a GPU. */
typedef struct sslam_fitness_pair {
  int32_t target, source;   /* cloud indices */
  double T[12];             /* R row-major, then t: source -> target frame */
  double max_range;         /* bound on the SQUARED distance; DBL_MAX = none */
} sslam_fitness_pair;
int sslam_seg_fitness_scores(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, const sslam_fitness_pair* pairs, int n_pairs,
                             double* score_out, int32_t* used_out, int32_t* nn_index_out, float* nn_dist2_out, double* kernel_ms);
/* InformationMatrixCalculator::calc_information_matrix, the branch without ~use_const_inf_matrix (information_matrix_calculator.cpp:39-50):
 *   weight(a, max_x, min_y, max_y, x) = min_y + (max_y - min_y) * (1 - exp(-a x)) / (1 - exp(-a max_x))     (hpp:20-24; no clamp: a score
 *   above fitness_score_thresh gives more than max_y, DBL_MAX a finite matrix);
 *   w_x = (float) weight(var_gain_a, fitness_score_thresh, min_stddev_x^2, max_stddev_x^2, fitness), w_q alike with the _q pair;
 *   info = diag(1 / w_x, 1 / w_x, 1 / w_x, 1 / w_q, 1 / w_q, 1 / w_q), row-major 6 x 6.
 * Host only: needs no device.  sslam_inf_default_params: 20, 0.1, 5.0, 0.05, 0.2, 0.5 -- hdl_graph_slam's defaults [UPSTREAM, unverified
 * here]: quoted from memory, hdl_graph_slam is not part of the reference tree, whose members of these names are never initialised. */
typedef struct sslam_inf_params {
  double var_gain_a, min_stddev_x, max_stddev_x, min_stddev_q, max_stddev_q, fitness_score_thresh;
} sslam_inf_params;
void sslam_inf_default_params(sslam_inf_params* p);
int sslam_information_from_fitness(const sslam_inf_params* p, double fitness, double info[36]);

/* ---- scan matching: nearest-neighbour ICP of cloud pairs (what hdl_graph_slam's LoopDetector::matching does with
 * pcl::IterativeClosestPoint [UPSTREAM]; the reference has no scan matcher) ------------------------------------------------------------
 * sslam_seg_register_pairs: for every pair, the rigid transform T (source -> target frame) that the point-to-point ICP loop reaches from
 * the initial guess T0, and the fitness score at it.  Clouds are laid out as for sslam_seg_fitness_scores; a cloud may serve several
 * pairs.  All pairs share one set of launches per iteration, and the whole loop runs on the device: the host only reads, every 8
 * iterations at most, how many pairs are still unfinished.  One iteration of a pair, from its current T (12 doubles):
 *   1. correspondences: exactly the fitness pass at T (R, t cast to float once, the float32 arithmetic and the lowest-index tie rule
 *      stated above).  Source point i is ACCEPTED when it found a neighbour and (double)d2 <= max_corr2.
 *   2. fewer than 3 accepted: status = SSLAM_ERR_NUMERIC, the pair is finished and T is left as it stood before this pass.
 *   3. in double, over the accepted points: n, sum p, sum q, sum p q^T with p the ORIGINAL source point and q its target, widened from
 *      float.  The order of summation is fixed by the point index alone (the tree of the fitness score inside every run of 256
 *      consecutive source points, the runs in ascending order; no floating-point atomics): it depends neither on the target split nor
 *      on the other pairs of the call, and repeating a call repeats its bits.
 *   4. T_new = the rigid transform minimising sum |R p + t - q|^2 over those correspondences, solved for the ABSOLUTE transform (no
 *      composition of increments, so no composition error accumulates): Horn's closed form, the unit quaternion of R being the dominant
 *      eigenvector of a symmetric 4 x 4 matrix of the cross-covariance, found by cyclic Jacobi sweeps; t = mean q - R mean p.  This is
 *      the minimiser pcl::TransformationEstimationSVD computes.  R is a proper rotation (det = +1) for coplanar correspondences too.
 *      COLLINEAR correspondences leave the rotation about their line undetermined: any of the minimisers may be returned.
 *      The sums are not centred, so the update loses |mean|^2 / spread^2 in relative accuracy (spread^2: the smallest variance of the
 *      cloud): about 1e-11 in t for clouds a few metres wide and 30 m from the origin of their coordinates, about 1e-6 at 1000 m.
 *   5. iterations += 1 and T = T_new; if no entry of T moved by more than epsilon (max |T_new - T| <= epsilon over the 12 entries) the
 *      pair is finished with converged = 1.  epsilon = 0 asks for T to repeat bit for bit, which happens once the correspondences
 *      repeat (equal correspondences give equal sums).
 * A finished pair is frozen: its T never changes again while the others iterate on, at most max_iterations times.  Then one more
 * fitness pass at the final T fills score, used and the optional nn_index_out / nn_dist2_out (layout as in sslam_seg_fitness_scores):
 * bitwise what sslam_seg_fitness_scores returns for out.T with max_range = max_corr2, so sslam_information_from_fitness(out.score) is
 * the information matrix of the loop edge.  max_iterations = 0 is valid: T = T0 and the call is the fitness pass at T0.
 * kernel_ms (optional): hipEvent time from the first reset to the end of the final pass (the reads of the counter in between included).
 * Empty clouds are valid (status SSLAM_ERR_NUMERIC when max_iterations > 0; used = 0, score = DBL_MAX).  Returns n_pairs.
 * SSLAM_ERR_INVALID: the cases of sslam_seg_fitness_scores (with out in the place of score_out / used_out), max_iterations < 0, a
 * negative or NaN epsilon.  SSLAM_ERR_NO_DEVICE without a GPU.  SSLAM_FITNESS_OPTS="chunk=N" acts as in the fitness pass. */
typedef struct sslam_reg_pair {
  int32_t target, source;      /* cloud indices, as in sslam_fitness_pair */
  double  T0[12];              /* initial guess, R row-major then t: source -> target frame */
  double  max_corr2;           /* bound on the SQUARED correspondence distance; DBL_MAX = none */
} sslam_reg_pair;
typedef struct sslam_reg_result {
  double  T[12];               /* the estimate the loop ended at */
  double  score;               /* fitness score AT T, as sslam_seg_fitness_scores with max_range = max_corr2 */
  int32_t used;                /* source points behind `score` */
  int32_t iterations;          /* updates of T that were carried out */
  int32_t converged;           /* 1: the last update moved no entry of T by more than epsilon */
  int32_t status;              /* 0, or SSLAM_ERR_NUMERIC: fewer than 3 accepted correspondences in some pass; T as it stood before that pass */
} sslam_reg_result;
int sslam_seg_register_pairs(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, const sslam_reg_pair* pairs, int n_pairs,
                             int max_iterations, double epsilon, sslam_reg_result* out, int32_t* nn_index_out, float* nn_dist2_out, double* kernel_ms);

/* ---- generalized ICP: plane-to-plane scan matching (hdl_graph_slam's registration_method GICP / FAST_GICP: pcl::GeneralizedIterativeClosestPoint,
 * fast_gicp::FastGICP [UPSTREAM, quoted from memory]; the reference has no scan matcher) ------------------------------------------------
 * sslam_seg_cloud_covariances: for every point, the covariance of its k nearest neighbours inside its OWN cloud, regularised to a plane
 * (k_knn_cov).  Clouds are laid out as for sslam_seg_fitness_scores.  cov_out: 6 doubles per point of xyz (xx xy xz yy yz zz; a point
 * before cloud_start[0] gets zeros).  knn_index_out (optional): k int32 per point, indices inside the point's cloud, -1 padded.
 *   Neighbours.  d2 = (dx dx + dy dy) + dz dz in float32 without fused multiply-add, dx = x_query - x_candidate.  The candidates are
 *     the finite points of the query's cloud, the query itself included.  The set is the k smallest by (d2, index), lexicographic: ties
 *     go to the lowest index.  It does not depend on the launch geometry, and a NumPy float32 restatement gives the same indices bit
 *     for bit.  knn_index_out lists them in that (d2, index) order.  A cloud with m < k finite points uses all m.
 *   Covariance, in double: mean = the sum of the neighbours in that order / m;  C = sum (q - mean)(q - mean)^T / m.
 *   Regularisation (fast_gicp's RegularizationMethod::PLANE): C = U diag(l0 <= l1 <= l2) U^T is replaced by U diag(plane_epsilon, 1, 1) U^T,
 *     which is I - (1 - plane_epsilon) n n^T with n the unit eigenvector of l0, and is computed that way: cyclic Jacobi sweeps on the
 *     symmetric 3 x 3 matrix in double.  Where l0 = l1 (collinear or isotropic neighbourhoods) n is not determined: any minimiser may be
 *     returned.
 *   m < 3: the identity.  A non-finite point gets six zeros (and k times -1); it can never be a correspondence, so they are never read.
 * k: 3 .. 32 (callers default to 20); plane_epsilon: finite, in (0, 1] (1e-3).  kernel_ms (optional): hipEvent time of the kernel.
 * Returns the number of points.  SSLAM_ERR_INVALID, before any device call: the cases of sslam_seg_fitness_scores (cov_out in the place
 * of the outputs), k or plane_epsilon outside their range.  SSLAM_ERR_NO_DEVICE without a GPU.
 *
 * sslam_seg_register_pairs_gicp: sslam_seg_register_pairs with the generalized-ICP update.  cov: 6 doubles per point of xyz as
 * sslam_seg_cloud_covariances writes them, or NULL: they are computed inside the call, once per cloud that some pair names, with
 * params (NULL: sslam_gicp_default_params: k 20, plane_epsilon 1e-3; with cov given, params is only checked).  The launch structure,
 * the freezing of finished pairs, the convergence rule, the final fitness pass and the errors are those of sslam_seg_register_pairs.
 * One iteration of a pair from its T = (R, t):
 *   1. correspondences: exactly step 1 of sslam_seg_register_pairs (the indices are bitwise those of the fitness pass at T).
 *   2. per accepted pair (source i, target j), in double:  x = R p + t,  r = q - x,  M = (C_j + R C_i R^T)^-1 by cofactors (with
 *      regularised covariances its eigenvalues lie in [1 / 2, 1 / (2 plane_epsilon)]),  J = [ [x]x | -I ]  for the left perturbation
 *      T <- exp(delta) T, delta = (w, v).  29 sums: the upper triangle of J^T M J, J^T M r, r^T M r and the count, in the fixed order
 *      of step 3 of sslam_seg_register_pairs.
 *   3. H delta = -b by Cholesky.  Fewer than 3 accepted, a pivot that is not positive or a sum or result that is not finite:
 *      status = SSLAM_ERR_NUMERIC, the pair is finished and T is left as it stood before this pass.
 *   4. R_new = exp([w]x) R, passed through its unit quaternion (largest-pivot branch) and back, so that R stays a proper rotation to
 *      1e-12 after any number of iterations;  t_new = exp([w]x) t + v.
 *   5. iterations += 1; converged when max |T_new - T| <= epsilon over the 12 entries.  Unlike the closed form of the point-to-point
 *      update, a Gauss-Newton step keeps moving T in its last bits: epsilon = 0 runs a pair to max_iterations.
 * DEVIATION: M is held fixed within an iteration and rebuilt at the next, and the step is plain Gauss-Newton.  fast_gicp wraps the same
 * step in Levenberg-Marquardt and PCL's GICP minimises with BFGS; neither was needed on the scenes this project tests.
 * score is the EUCLIDEAN fitness score at out.T, bitwise what sslam_seg_fitness_scores returns (hdl's getFitnessScore for every method),
 * so fitness_score_thresh and sslam_information_from_fitness apply unchanged.  max_iterations = 0: T = T0, the fitness pass at T0, and
 * the covariances are neither read nor computed.  kernel_ms does not include a covariance pass made inside the call.
 * SSLAM_ERR_INVALID also for params with k or plane_epsilon out of range. */
typedef struct sslam_gicp_params {
  int32_t k;                   /* 20    neighbours per covariance, 3 .. 32 */
  double  plane_epsilon;       /* 1e-3  the eigenvalue along the normal, in (0, 1] */
} sslam_gicp_params;
void sslam_gicp_default_params(sslam_gicp_params* p);
int sslam_seg_cloud_covariances(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, int k, double plane_epsilon, double* cov_out,
                                int32_t* knn_index_out, double* kernel_ms);
int sslam_seg_register_pairs_gicp(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds, const sslam_reg_pair* pairs, int n_pairs,
                                  const double* cov, const sslam_gicp_params* params, int max_iterations, double epsilon, sslam_reg_result* out,
                                  int32_t* nn_index_out, float* nn_dist2_out, double* kernel_ms);

/* ---- map cloud: every cloud at its pose, reduced to one cloud over a SPARSE voxel grid (hdl_graph_slam's
 * MapCloudGenerator::generate(keyframes, resolution) [UPSTREAM, quoted from memory]: transform, concatenate, octree-downsample; the
 * reference planned the call -- mapping::generateMap / opitmizeMap at semantic_graph_slam.cpp:36-40, 72-73, 85-86, commented out) ------
 * sslam_seg_map_cloud: clouds laid out as for sslam_seg_fitness_scores (cloud_start: n_clouds + 1 entries, non-decreasing, first >= 0);
 * T: 12 doubles per cloud, R row-major, then t, taking the cloud into the map frame.  sslam_seg_voxel_grid cannot serve here: it sizes a
 * dense grid over the bounding box and refuses more than 2^26 cells, and nearly all of a map's box is empty.
 * Transform, in float32 without fused multiply-add (a NumPy restatement matches bit for bit; the arithmetic of the fitness pass):
 *   R, t = T cast from double to float once;   x' = ((r00 x + r01 y) + r02 z) + tx  (y', z' alike).
 * A point takes no part when one of its three coordinates, or one of its three transformed coordinates, is not finite.
 * Cell: i = (int)floorf(x' * inv) per axis with inv = 1.0f / resolution, the rule of sslam_seg_voxel_grid.  Cells are GLOBAL: they do not
 * depend on the bounding box, so two calls over different sets of clouds put the same point into the same cell.
 * Sparse grid, two levels: a brick is 8 x 8 x 8 cells, brick index b = i >> 3 (arithmetic shift: floor division), local index l = i & 7.
 *   0. min / max pass over the transformed points.  The cell bounds of that box must pass the 32-bit test of sslam_seg_voxel_grid, and the
 *      dense grid of BRICKS over it may hold at most 2^26 bricks (the same rule, applied to cell >> 3): otherwise SSLAM_ERR_UNSUPPORTED,
 *      before anything is sized or written.
 *   1. the occupied bricks are flagged; an ordered compaction gives their ascending list and a brick -> slot table.  More than 2^20
 *      occupied bricks (2^29 cells, about 15 GB of tables): SSLAM_ERR_UNSUPPORTED, the number in the message.
 *   2. per voxel slot * 512 + local: the point count (int32) and the sums of x', y', z' in 2^-20 fixed point, llrint((double)x' * 1048576.0),
 *      by 64-bit integer atomics as in sslam_seg_voxel_grid.  Integer sums are exact and independent of arrival order: the result does
 *      not depend on the launch geometry, and repeating a call repeats its bits.  A sum is an int64: |x'| times the voxel's count must
 *      stay below 2^43, which a map's metres do by many orders of magnitude; beyond it the centroid is undefined.  (The direct form:
 *      one 32-bit and three 64-bit atomics per point, no merge of equal cells inside a wave.  Never float atomics.)
 *   3. the voxels with count >= max(min_points, 1) are compacted; one record each:
 *      xyz_out: the CENTROID (float)(((double)sum / 1048576.0) / (double)count); cells_out: the global cell ix, iy, iz; counts_out: count.
 * DEVIATION: hdl's octree returns the voxel CENTRES (getOccupiedVoxelCenters); the centre of record k is (cells_out[3 k + a] + 0.5) *
 * resolution, for a caller that wants it.
 * Output order: ascending occupied brick in the dense brick grid, x fastest -- (bz, by, bx) -- and inside a brick ascending local index,
 * x fastest -- (lz, ly, lx).  It is the order of the two ordered compactions: no sort, and fixed by the points alone, not by the order
 * of the clouds or of the points in them.
 * A workgroup never spans two clouds (R, t are uniform in the wave); each pass recomputes the transform instead of storing it.
 * cells_out, counts_out, stats are optional.  Returns the number of voxels that pass min_points -- the true count; at most max_out
 * records are written -- and 0 for no clouds or no usable point.
 * stats: kernel_ms sums the hipEvent times of the four passes (the copies between them excluded; the 4-byte read of a compaction's total
 * inside pass 3 included); sslam_seg_last_map_timing gives the four of the last call: min / max, bricks, accumulate, voxels + records.
 * SSLAM_ERR_INVALID: a NULL handle; cloud_start or T NULL with clouds; xyz NULL with points; xyz_out NULL with max_out > 0; a negative
 * n_clouds, max_out or min_points; a cloud_start that decreases or starts below 0; a resolution that is not finite and positive, or
 * whose 1 / resolution is not finite in float; a non-finite entry of T; a batch in flight (sslam_seg_submit_batch).
 * SSLAM_ERR_UNSUPPORTED also for more than 2^22 clouds.  SSLAM_ERR_NO_DEVICE without a GPU. */
typedef struct sslam_map_stats {
  int32_t n_clouds, n_points;      /* given; n_points counts every row, finite or not */
  int32_t n_used;                  /* points that landed in a voxel */
  int32_t n_bricks, n_voxels;      /* occupied bricks; occupied voxels BEFORE min_points */
  int64_t upload_bytes;            /* host -> device bytes this call moved: points, poses and cloud_start */
  double  kernel_ms;               /* hipEvent time of the passes, copies excluded */
} sslam_map_stats;
int sslam_seg_map_cloud(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds,
                        const double* T /* 12 per cloud: R row-major, then t; cloud -> map frame */,
                        float resolution, int min_points,
                        float* xyz_out, int32_t* cells_out, int32_t* counts_out, int max_out,
                        sslam_map_stats* stats);
int sslam_seg_last_map_timing(const sslam_seg* s, double ms[4]);

/* ---- occupancy map: every cloud at its pose, every point a ray from the sensor, free / occupied / unknown per cell of the SPARSE grid of
 * sslam_seg_map_cloud.  The reference's demo output: its README launch runs octomap_server (resolution 0.05, sensor_model/max_range 10,
 * pointcloud_min_z -1, pointcloud_max_z 5) on the clouds and poses the SLAM node publishes; sslam_occ_default_params holds those values and
 * OctoMap's sensor model [UPSTREAM, quoted from memory]: hit 0.7, miss 0.4, clamp 0.1192 .. 0.971, occupancy threshold 0.5, each
 * probability turned into log-odds log(p / (1 - p)) on the host in double and cast to float.  The kernels only see the float log-odds.
 * cloud_start, T, the cast of T to float, the transform x' = ((r00 x + r01 y) + r02 z) + tx without fused multiply-add and the rule for
 * non-finite rows are those of sslam_seg_map_cloud.  The ray origin of a cloud is T applied to sensor_origin in the same arithmetic; a cloud
 * whose ray origin is not finite takes no part.  A ray whose end point has z' outside [z_min, z_max] takes no part (n_clipped_z).
 * The traversal is exact, in integers.  inv = 1.0f / resolution.
 *   position of a coordinate p: u = p * inv (float), c = (int)floorf(u) -- the cell rule of the map cloud --, f = u - floorf(u),
 *     q = min((int)(f * 1024.0f), 1023) (f rounds to 1 for a tiny negative u), Q = (int64)c * 1024 + q: an integer in 1/1024 cell.
 *     Qo of the ray origin, Qe of the end point.  |u| must stay below 2^19 cells on every axis for every ray that takes part:
 *     otherwise SSLAM_ERR_UNSUPPORTED (it keeps |D|^2 below 2^63).
 *   range: D = Qe - Qo, len2 = |D|^2 in int64, R = (int64)floor((double)max_range * (double)inv * 1024.0), 1 <= R <= 2^20.  When
 *     len2 > R^2 the ray is TRUNCATED: L = the smallest integer with L^2 >= len2 (a double square root corrected by integer checks),
 *     D_a = (D_a * R) / L in C integer division, Qe = Qo + D.  Cell = Q >> 10, q = Q & 1023.
 *   steps: n_a = |ce_a - co_a| per axis; the ray makes exactly n_x + n_y + n_z steps of one cell along one axis.  Per axis the numerator
 *     of the parameter of the next face: 1024 - qo_a when D_a > 0, qo_a when D_a < 0, + 1024 per step on that axis.  The next step is on
 *     the axis, among those with steps left, with the smallest num_a / |D_a|, compared by cross-multiplication in int64; an exact tie goes
 *     to the lowest axis.  (Only axes with steps left: the walk arrives at the end cell also when a ray going down ends on a face.)
 *   counts: the start cell and every cell stepped into except the last get one miss; the last cell one hit, or one miss when the ray was
 *     truncated (also when it has no step at all).  An untruncated ray of zero steps is one hit on its cell.
 *   log-odds of a cell: t = (float)hits * l_hit + (float)misses * l_miss, both products and the sum rounded to float (no contraction),
 *     then fminf(fmaxf(t, l_min), l_max).  A cell is occupied when that is >= l_occ.
 * DEVIATIONS from OctoMap [UPSTREAM, quoted from memory]: (1) per-ray integration as in insertPointCloudRays, not the per-scan
 * de-duplication of insertPointCloud (a cell once per scan, a hit overriding a miss); (2) the clamp is applied once, to the sum, not after
 * every update: the result is independent of the order of clouds and points and of the launch geometry, and equals OctoMap's whenever
 * no intermediate value reaches a clamp; (3) the product is a flat list of cells at one resolution, not an octree.
 * Passes (integer atomics only; the launch geometry, the 8 x 8 x 8 bricks and both limits -- 2^26 bricks in the box, 2^20 touched bricks,
 * SSLAM_ERR_UNSUPPORTED before anything is written -- are the map cloud's): 0. the box of the start and end cells and the ray counters;
 * 1. every ray is walked and the bricks it enters are flagged, then compacted; 2. every ray is walked again: one int32 atomic add per cell
 * into misses[slot * 512 + local] or hits[...] (8 bytes per cell of a touched brick); 3. the known cells (hits + misses > 0) that pass
 * `emit` are compacted and written.  Output order: that of the map cloud, bricks ascending with x fastest, then the local index.
 * cells_out (3 per record), hits_out, misses_out, logodds_out, stats: each optional.  Returns the number of records that pass `emit` -- the
 * true count; at most max_out are written -- and 0 for no clouds or no ray.
 * SSLAM_ERR_INVALID: a NULL handle or params; cloud_start or T NULL with clouds; xyz NULL with points; negative n_clouds or max_out; a
 * cloud_start that decreases or starts below 0; a non-finite entry of T or sensor_origin; resolution or max_range not finite and positive
 * (or 1 / resolution not finite); R outside 1 .. 2^20; l_hit not > 0, l_miss not < 0; l_min > l_max, z_min > z_max, or a NaN among them or
 * in l_occ; emit outside 0 .. 2; a batch in flight.  SSLAM_ERR_UNSUPPORTED also for more than 2^22 clouds.  SSLAM_ERR_NO_DEVICE without a GPU. */
typedef struct sslam_occ_params {
  float resolution;          /* cell edge, m */
  float max_range;           /* m; rays longer than this are cut there and end in a miss */
  float z_min, z_max;        /* a ray whose transformed end point has z' outside [z_min, z_max] takes no part */
  float sensor_origin[3];    /* in the cloud frame; the ray origin is T applied to it */
  float l_hit, l_miss;       /* log-odds added per hit (> 0) and per miss (< 0) */
  float l_min, l_max;        /* clamp of the sum (the scans entries: of every update) */
  float l_occ;               /* a cell is occupied when its log-odds >= l_occ */
  int32_t emit;              /* 0 every known cell, 1 occupied only, 2 free only */
} sslam_occ_params;
typedef struct sslam_occ_stats {
  int32_t n_clouds, n_points;      /* given; n_points counts every row, finite or not */
  int32_t n_rays;                  /* rays that took part, the truncated ones included */
  int32_t n_truncated, n_clipped_z;
  int32_t n_bricks, n_cells;       /* touched bricks; known cells BEFORE emit */
  int32_t reserved;
  int64_t n_steps;                 /* cells visited, the start and end cells included: the sum of all hits and misses, the atomics of pass 2
                                      (the scans entries: the (scan, cell) updates, again the sum of all hits and misses) */
  int64_t upload_bytes;            /* host -> device bytes this call moved */
  double  kernel_ms;               /* hipEvent time of the four passes, copies excluded */
} sslam_occ_stats;
void sslam_occ_default_params(sslam_occ_params* p);
int sslam_seg_occupancy_map(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds,
                            const double* T /* 12 per cloud: R row-major, then t; cloud -> map frame */, const sslam_occ_params* p,
                            int32_t* cells_out, int32_t* hits_out, int32_t* misses_out, float* logodds_out, int max_out,
                            sslam_occ_stats* stats);
/* hipEvent milliseconds of the four passes of the last call: box, bricks, accumulate, cells + records */
int sslam_seg_last_occupancy_timing(const sslam_seg* s, double ms[4]);

/* ---- occupancy map by scans: OctoMap's insertPointCloud, what octomap_server's insertScan runs [UPSTREAM, quoted from memory]: per scan a set
 * of free cells and a set of occupied cells, a free cell dropped when the same scan also saw it occupied, every remaining cell updated ONCE
 * and clamped after that update.  The arguments, params and stats are those of sslam_seg_occupancy_map.
 * Unchanged from sslam_seg_occupancy_map: the rays, the z clip, the cut at max_range, the integer walk, both limits, the argument errors,
 * the output order (bricks ascending with x fastest, then the local index), count-only calls, `emit` and max_out.
 * New:
 *   scans: a scan is one cloud, that is one entry of cloud_start.  Scans are applied in the order given.  A cloud that takes no part (empty,
 *     ray origin not finite, every row clipped or not finite) is a scan without updates.  One cloud split in two is two scans, so the
 *     split changes the result, unlike in the ray entry.
 *   sets per scan: H = the last cells of its rays that were not truncated; M = every other cell its walks visit, the last cell of a
 *     truncated ray included, minus H: a hit overrides a miss.
 *   update per scan, for each cell of H or M, from lo = 0.0f the first time the cell is touched:
 *     lo = fminf(fmaxf(lo + l, l_min), l_max), l = l_hit for H and l_miss for M, the sum rounded to float (no contraction).  A cell gets at
 *     most one update per scan, so there is no order inside a scan.
 *   outputs: hits_out = the number of scans with the cell in H; misses_out = the number of scans with the cell in M; logodds_out = lo after
 *     the last scan.  The known cells, hits + misses > 0, are the cells the ray entry reports for the same input.  `emit` tests the
 *     sequential lo against l_occ.
 *   stats: n_rays, n_truncated, n_clipped_z, n_bricks and n_cells as in the ray entry; n_steps = the sum of hits_out and misses_out at
 *     emit 0, the number of (scan, cell) updates; reserved 0; kernel_ms and sslam_seg_last_occupancy_timing cover the call as before, slot
 *     2 being mark plus fold.
 *   independence: of the order and the multiplicity of the points inside a cloud, of the launch geometry and of the chunk width below.  The
 *     result depends on the order of the clouds, as OctoMap's does.  A repeated call repeats its bits.
 * DEVIATIONS (1) and (2) of sslam_seg_occupancy_map are gone for these entries; (3) stays: a flat list of cells, not an octree.
 * Passes (integer atomics only): 0 and 1 are the ray entry's.  2, per chunk of 64 consecutive clouds: mark -- every ray of the chunk is
 * walked and bit (cloud - first cloud of the chunk) is set in the cell's 64-bit hit or miss mask by an atomic OR, issued only when a plain
 * load shows the bit still clear (OR is idempotent, so neither a lost race nor the order matters) -- then fold: one thread per cell of the
 * bricks the chunk entered applies the set bits in ascending order to the cell's hits, misses and lo and clears the masks.  All launches go
 * on the handle's stream with no host round trip between chunks.  28 bytes per cell of a touched brick: hits, misses, lo, two masks (15 GB
 * at the limit of 2^20 touched bricks).  3. the known cells that pass `emit` are compacted and written. */
int sslam_seg_occupancy_map_scans(sslam_seg* s, const float* xyz, const int32_t* cloud_start, int n_clouds,
                                  const double* T /* 12 per cloud: R row-major, then t; cloud -> map frame */, const sslam_occ_params* p,
                                  int32_t* cells_out, int32_t* hits_out, int32_t* misses_out, float* logodds_out, int max_out,
                                  sslam_occ_stats* stats);
/* hipEvent milliseconds of mark and of fold, each summed over the chunks of the last scans call (their sum is slot 2 of the timing above) */
int sslam_seg_last_occupancy_scan_timing(const sslam_seg* s, double ms[2]);
/* counts[0]: the cells the mark launches of the last scans call visited (the ray entry's n_steps for the same input); counts[1]: the
 * atomic ORs they issued, the rest having found their bit set by the plain load.  counts[1] varies from run to run; the result does not. */
int sslam_seg_last_occupancy_scan_counts(const sslam_seg* s, int64_t counts[2]);

/* parity hooks: per-box products of the last sslam_seg_segment call.
 * normals: w*h*4 floats (nx,ny,nz,curvature), labels: w*h int32 (-1 = no plane; otherwise the
 * region index in output order of pcl::OrganizedMultiPlaneSegmentation::segmentAndRefine). */
int sslam_seg_get_normals(sslam_seg* s, int box, float* out);
int sslam_seg_get_labels(sslam_seg* s, int box, int32_t* out);
/* GPU kernel time (hipEvents on the handle's stream, H2D/D2H excluded) and wall time of the last call */
int sslam_seg_last_timing(const sslam_seg* s, double* kernel_ms, double* total_ms);
/* semantic_tools::transformNormalsToWorld (include/tools.h:18-102): 4x4 row-major float */
int sslam_seg_transform(const sslam_seg* s, const float robot_pose[6], float cam_angle, float out16[16]);


/* ============================================================================================
 * Orchestrator tick without ROS: semantic_graph_slam (reference include/ps_graph_slam/semantic_graph_slam.h,
 * src/ps_graph_slam/semantic_graph_slam.cpp) + KeyframeUpdater (keyframe_updater.hpp:41-65) + data_association
 * (data_association.h:70-389) + InformationMatrixCalculator (information_matrix_calculator.cpp:28-35).  SURVEY §8 rows f3, f2.
 * The ROS node becomes a thin shell: its callbacks call the set_* / vio entry points, its 30 Hz loop calls sslam_slam_run.
 * ==========================================================================================*/
typedef struct sslam_slam sslam_slam;

typedef struct sslam_slam_params {
  double keyframe_delta_trans, keyframe_delta_angle, keyframe_delta_time; /* 0.5, 0.5, 1 (keyframe_updater.hpp:24-29) */
  int max_keyframes_per_update;          /* 10 (semantic_graph_slam.cpp:18) */
  int update_keyframes_using_detections; /* ~update_key_using_det, false (semantic_graph_slam.cpp:22-23) */
  double camera_angle_deg;               /* ~camera_angle, degrees (semantic_graph_slam.cpp:24,29) */
  int add_first_lan;                     /* ~add_first_lan (semantic_graph_slam.cpp:25,54-55,289-329) */
  double first_lan[3];                   /* 1.8, 0, 0.3 */
  int use_const_inf_matrix;              /* information_matrix_calculator.cpp:9,29 */
  double const_stddev_x, const_stddev_q; /* 0 -> 0.0667 (information_matrix_calculator.cpp:11-17) */
  double maha_dist_thres, eq_dist_thres; /* 0.5, 1.21 (data_association.h:49-50) */
  double land_noise_low, land_noise_high;/* 0.5, 0.9  (data_association.h:51-52) */
  int use_maha_dist, use_eq_dist, use_rtab_map_odom; /* true, false, false (data_association.h:53-55) */
  int max_iterations;                    /* 1024 (graph_slam.cpp:205) */
  int reference_quirks;                  /* bit 0: keep distance_min across the detections of a frame (quirk B5, data_association.h:101);
                                            default 0 = reset per detection */
  int device;
} sslam_slam_params;

/* data_association's landmark (include/ps_graph_slam/landmark.h:17-33) */
typedef struct sslam_landmark {
  int32_t id;            /* index in the landmark list */
  int32_t vertex;        /* graph vertex id of landmark::node (-1 before it is added) */
  int32_t class_id;      /* landmark::type */
  int32_t plane_type;    /* landmark::plane_type: 0 horizontal, 1 vertical */
  int32_t is_new;
  float pose[3];         /* world position the landmark was created / last observed at */
  float local_pose[3];   /* observation in the robot frame (the edge measurement) */
  float covariance[9];   /* 3x3, row-major: marginal of the last optimisation (getAndSetLandmarkCov) */
  float normal[4];       /* normal_orientation in the world frame */
  float distance;        /* association distance of the observation that produced this record (extension) */
} sslam_landmark;

typedef struct sslam_tick_stats {
  int keyframes_added;     /* <= max_keyframes_per_update */
  int landmarks_added, landmarks_matched, landmark_edges_added;
  int optimized;           /* GraphSLAM::optimize() returned true */
  int marginals_ok;        /* computeLandmarkMarginals returned true */
  sslam_opt_stats opt;
  double seconds_frontend, seconds_association, seconds_optimize, seconds_marginals;
} sslam_tick_stats;

void sslam_slam_default_params(sslam_slam_params* p);
/* semantic_graph_slam::init (semantic_graph_slam.cpp:11-56).  seg: the frontend handle used for keyframes that carry a cloud and
 * boxes (NULL when every keyframe brings pre-segmented objects); it is borrowed, not owned. */
sslam_slam* sslam_slam_create(const sslam_slam_params* p, sslam_seg* seg);
void sslam_slam_destroy(sslam_slam* s);
/* Information of the odometry edges from the fitness score of the two keyframes' clouds (what `use_const_inf_matrix = false` means
 * upstream; sslam_slam_create still refuses that flag, whose branch reads uninitialised members in the reference, and this setter is
 * the defined-behaviour route to the same capability).  p = NULL: back to the constant matrix.  voxel_leaf: 0 -> 0.1; max_range (a
 * bound on the SQUARED distance, as in sslam_seg_fitness_scores): <= 0 -> DBL_MAX.
 * With the model set, a tick collects its consecutive keyframe pairs (prev, kf) first.  Where both carry a cloud (a keyframe takes the
 * cloud of sslam_slam_set_point_cloud with its detection boxes, as before, and under this model also a cloud that arrived since the last
 * keyframe without boxes), the finite points of either cloud are voxel-grid downsampled (sslam_seg_voxel_grid, voxel_leaf) and the
 * score of rel = prev.odom^-1 * kf.odom is computed with prev's cloud as the target, kf's as the source and T = rel: all pairs of the
 * tick in ONE sslam_seg_fitness_scores pass on the frontend handle given to sslam_slam_create (SSLAM_ERR_INVALID from sslam_slam_run
 * when that handle is NULL and a pair needs it).  Each such edge gets sslam_information_from_fitness of its score; a pair where either
 * keyframe has no cloud gets the constant matrix.  The downsampled cloud of the last keyframe of a tick is kept as the target of the
 * first pair of the next tick.  Without the model a tick does what it did before this call existed, edge for edge.
 * Returns 0; SSLAM_ERR_INVALID for a NULL handle, a negative or non-finite voxel_leaf, a non-finite max_range. */
int sslam_slam_set_fitness_information(sslam_slam* s, const sslam_inf_params* p, float voxel_leaf, double max_range);
/* the odometry edges the last sslam_slam_run added, in order: the fitness score and the number of points it averages over; -1 and -1
 * for an edge that took the constant matrix.  Returns the number of edges (copies min(n, max); either output may be NULL); 0 when
 * the model was not set during that run. */
int sslam_slam_last_fitness(const sslam_slam* s, double* score, int32_t* used, int max);

/* ---- loop closing inside the tick (hdl_graph_slam's LoopDetector::detect [UPSTREAM]: find_candidates, matching, an EdgeSE3 with a robust
 * kernel; the reference has no loop detector).  Off until sslam_slam_set_loop_closure is called with parameters; a handle on which it
 * never was, or was last called with NULL, runs its ticks bit for bit as before this call existed and keeps no cloud for it. ---------------
 * sslam_loop_default_params: 5.0, 8.0, 5.0, DBL_MAX, 0.5, 64, 0.01, 0, 0.1, 0, Huber 1.0, sslam_inf_default_params -- hdl_graph_slam's defaults
 * [UPSTREAM, unverified here]: quoted from memory, hdl_graph_slam is not part of the reference tree. */
typedef struct sslam_loop_params {
  double  distance_thresh;                 /* 5.0   candidate: xy distance of the two estimates */
  double  accum_distance_thresh;           /* 8.0   candidate: travelled distance between the two keyframes */
  double  distance_from_last_edge_thresh;  /* 5.0   travelled distance since the keyframe of the last accepted loop */
  double  fitness_score_max_range;         /* DBL_MAX   bound on the SQUARED correspondence distance (max_corr2 of the scan matcher) */
  double  fitness_score_thresh;            /* 0.5   a best score above it: no loop */
  int32_t max_iterations;                  /* 64    of sslam_seg_register_pairs */
  double  epsilon;                         /* 0.01  of sslam_seg_register_pairs */
  int32_t max_candidates;                  /* 0 = all that pass; M in 1 .. 64 = the M nearest */
  float   voxel_leaf;                      /* 0.1   downsampling of a keyframe's cloud (0 -> 0.1) */
  double  gate_chi2;                       /* 0 = no gate; else a loop is accepted only with d2 < gate_chi2 (12.59: 6 degrees of freedom, 95 %) */
  int32_t robust_kernel;                   /* SSLAM_ROBUST_* of the loop edge: SSLAM_ROBUST_HUBER; SSLAM_ROBUST_NONE = none */
  double  robust_delta;                    /* 1.0 */
  sslam_inf_params inf;                    /* information of the loop edge from its score */
} sslam_loop_params;
void sslam_loop_default_params(sslam_loop_params* p);
#define SSLAM_LOOP_ADDED 0      /* the loop edge was added */
#define SSLAM_LOOP_SCORE 1      /* the best score is above fitness_score_thresh */
#define SSLAM_LOOP_GATE 2       /* d2 >= gate_chi2, or d2 is NaN */
#define SSLAM_LOOP_NO_MATCH 3   /* no pair ended with status 0 and used > 0 */
/* one record per new keyframe that reached the selection (step 5 below) with at least one candidate */
typedef struct sslam_loop {
  int32_t new_vertex, cand_vertex;         /* graph vertex ids of the target (the new keyframe) and the source (the best candidate; -1: NO_MATCH) */
  int32_t n_candidates;
  int32_t outcome;                         /* SSLAM_LOOP_* */
  int32_t edge_id;                         /* -1 unless ADDED */
  int32_t used, iterations, converged;     /* of the best pair, as sslam_reg_result has them; 0 with NO_MATCH */
  double  T[12];                           /* of the best pair: R row-major, then t, candidate -> new keyframe (zero with NO_MATCH) */
  double  score;                           /* of the best pair (DBL_MAX with NO_MATCH) */
  double  d2;                              /* of the gate; NaN when the gate is off or was not reached */
} sslam_loop;
/* p = NULL: off, and the downsampled clouds kept so far are dropped.  Otherwise the following ticks do, after the association loop and
 * before the optimisation (where hdl calls detect):
 *   0. sslam_slam_vio keeps the latest cloud on every keyframe that has a fresh one (as under sslam_slam_set_fitness_information).  The
 *      finite points of each new keyframe's cloud are voxel-grid downsampled once (sslam_seg_voxel_grid, voxel_leaf); the result stays on
 *      the keyframe for the rest of the run, the raw cloud is dropped as before.  A keyframe without a cloud (or without a finite point)
 *      is neither a candidate nor matched.  Clouds are taken to be in the frame of the keyframe's pose, as the fitness model does.
 *   1. the estimates of all keyframes are read from the graph; new ones sit at the estimate their vertex was added with.
 *   2. new keyframes with accum_distance - last_edge_accum < distance_from_last_edge_thresh are dropped, at the value last_edge_accum
 *      has when the tick starts (0 before the first loop; it only grows, so these would be skipped in any order).
 *   3. candidates: ONE k_loop_candidates launch (sslam_slam_loop_candidates below) over the processed keyframes, never over the same
 *      tick's new ones.
 *   4. ONE sslam_seg_register_pairs call for every (new, candidate) pair of the tick: target = the new keyframe's cloud, source = the
 *      candidate's, max_corr2 = fitness_score_max_range, T0 = estimate_new^-1 * estimate_cand -- both estimates with their quaternion
 *      normalised, q = conj(q_new) q_cand normalised again, R0 = the matrix of q, t0 = -(Rn t_new) + Rn t_cand with Rn the matrix of
 *      conj(q_new).  hdl zeroes the z of its guess for ground vehicles; this does not (DEVIATION: the reference flies).
 *   5. the new keyframes in order, the rule of step 2 applied again with the running last_edge_accum, which makes the result that of
 *      hdl's sequential loop.  The best pair of a keyframe is the one of lowest score among those with status == 0 and used > 0, equal
 *      scores going to the lowest keyframe index.  `converged` is reported, not demanded: PCL counts a loop that ran out of iterations
 *      as converged [UPSTREAM, unverified].  A best score above fitness_score_thresh: SCORE.
 *   6. info = sslam_information_from_fitness(&inf, score); z = (t, quaternion of R by the branch with the largest pivot, as INTEGRATION.md
 *      section 2 spells out).  With gate_chi2 > 0, ONE sslam_graph_gate call for the best pairs of the tick that passed the score test,
 *      before any loop edge is added; d2 >= gate_chi2 or NaN: GATE.
 *   7. sslam_graph_add_edge_se3(new vertex, candidate vertex, z, info), the robust kernel unless it is SSLAM_ROBUST_NONE,
 *      last_edge_accum = the new keyframe's accum_distance: ADDED.
 * An error of any step ends sslam_slam_run the way its other errors do (the keyframes stay in the graph, nothing is optimised).
 * Returns 0.  SSLAM_ERR_INVALID: a NULL handle; with p: a threshold (the three distances, both fitness values, gate_chi2, voxel_leaf) that
 * is negative or not finite, max_candidates outside 0 .. 64, a negative max_iterations, a negative or NaN epsilon, a robust_kernel that is
 * not a SSLAM_ROBUST_* kind or a robust_delta that sslam_graph_set_edge_robust_kernel would refuse for it, no frontend handle given to
 * sslam_slam_create.  Host only: needs no device. */
int sslam_slam_set_loop_closure(sslam_slam* s, const sslam_loop_params* p);
/* the records of the last sslam_slam_run, in the order of the new keyframes; returns their number (copies min(n, max); out may be NULL) */
int sslam_slam_last_loops(const sslam_slam* s, sslam_loop* out, int max);
/* wall seconds inside the last sslam_slam_run: [0] the candidate launch with its copies, [1] sslam_seg_register_pairs, [2] sslam_graph_gate,
 * [3] the whole loop stage, the downsampling of the new clouds included.  All zero with loop closure off. */
int sslam_slam_last_loop_timing(const sslam_slam* s, double seconds[4]);
/* The scan matcher of step 4 (hdl_graph_slam's registration_method).  SSLAM_REG_ICP, the default: sslam_seg_register_pairs.
 * SSLAM_REG_GICP: step 0 also computes the covariances of every new keyframe's downsampled cloud (sslam_seg_cloud_covariances with p; NULL:
 * sslam_gicp_default_params), ONCE per keyframe, and keeps them with the cloud; step 4 calls sslam_seg_register_pairs_gicp with them.  A
 * keyframe downsampled before GICP was chosen gets its covariances the first time it is packed for a match.  Selection, score test, gate
 * and edge are untouched, and [1] of sslam_slam_last_loop_timing is the matcher, whichever it is.  A separate call so that
 * sslam_loop_params keeps its layout; a handle on which it was never made, or made with SSLAM_REG_ICP, runs its ticks bit for bit as
 * before.  Changing the method or its parameters drops the kept covariances.  Returns 0; SSLAM_ERR_INVALID: a NULL handle, another
 * method, k outside 3 .. 32, a plane_epsilon that is not finite or not in (0, 1].  Host only: needs no device. */
#define SSLAM_REG_ICP 0
#define SSLAM_REG_GICP 1
int sslam_slam_set_loop_registration(sslam_slam* s, int method, const sslam_gicp_params* p);
/* *clouds = the keyframe clouds that went through sslam_seg_cloud_covariances since the handle was created.  Returns 0. */
int sslam_slam_loop_covariance_passes(const sslam_slam* s, int64_t* clouds);
/* LoopDetector::find_candidates for all new keyframes of a tick in one launch (k_loop_candidates), on its own.  keys: x, y, accum_distance
 * per old keyframe; news: the same per new keyframe.  Old keyframe k passes for new keyframe n when
 *   accum_n - accum_k >= accum_distance_thresh,   d2 <= distance_thresh * distance_thresh with d2 = dx dx + dy dy,
 * and all six values, the difference and d2 are finite.  d2 is formed in double without fused multiply-add (a NumPy float64 restatement
 * matches bit for bit), the squared threshold once on the host.  DEVIATION in form: hdl compares the norm with the threshold; comparing
 * the squares is the same test except in the last bit at the boundary.
 * max_candidates == 0: count_out[n] = the number that pass, row n of cand_out = the first `cap` of them in ascending index.
 * max_candidates == M: row n = the M smallest under the order (d2, index) -- equal d2 goes to the lowest index -- written in that order,
 * the first `cap` of them; count_out[n] = min(M, the number that pass).  Entries of cand_out that are not filled hold -1.
 * One wave per new keyframe, its lanes striding over the old ones; ballot-and-prefix compaction, or M rounds of a per-lane scan for the
 * smallest key above the last one chosen and a wave reduction: no atomics, no dependence on the launch geometry.  The tables travel
 * through the handle's pinned scratch on the handle's stream.  Only the two distance thresholds and max_candidates of p are read.
 * Returns n_new.  SSLAM_ERR_INVALID: a NULL handle or p, negative n_keys, n_new or cap, a NULL keys / news / count_out with entries, a NULL
 * cand_out with n_new * cap > 0, a threshold that is negative or not finite, max_candidates outside 0 .. 64.  SSLAM_ERR_NO_DEVICE without a GPU. */
int sslam_slam_loop_candidates(sslam_slam* s, const double* keys, int n_keys, const double* news, int n_new, const sslam_loop_params* p,
                               int32_t* cand_out, int32_t* count_out, int cap);
/* ---- the map of a run: keyframe clouds kept on the device, put at their current estimates by sslam_seg_map_cloud's kernels (where the
 * reference has its commented-out mapping thread, semantic_graph_slam.cpp:72-73, 85-86).  Off until sslam_slam_set_map_clouds is called
 * with on != 0; a handle on which it never was, or was last called with on = 0, runs its ticks bit for bit as before this call existed
 * and keeps nothing.  Turning it off drops what was kept. -----------------------------------------------------------------------------
 * With it on: sslam_slam_vio keeps the latest cloud on every keyframe that has a fresh one (as under sslam_slam_set_fitness_information).
 * In the tick, before the raw cloud is dropped, the finite points of each new keyframe's cloud are voxel-grid downsampled once
 * (sslam_seg_voxel_grid, keyframe_leaf; 0 -> 0.1) and the result is appended ONCE to a device buffer of the handle.  The leaf is
 * independent of loop closure's voxel_leaf (with both on and equal leaves the one downsampled cloud serves both).  A keyframe without a
 * cloud, or without a finite point, holds no map cloud.  Clouds are taken to be in the frame of the keyframe's pose, as the fitness
 * model and the loop stage take them.  Neither switch position changes an estimate: the map clouds feed nothing back into the graph.
 * The kept clouds live on the orchestrator's device (sslam_slam_params.device) and are read there by the frontend handle's kernels, so
 * both handles must name the SAME device: on != 0 with sslam_seg_params.device != sslam_slam_params.device is refused here, on the host.
 * Returns 0; SSLAM_ERR_INVALID for a NULL handle, a negative or non-finite keyframe_leaf, on != 0 without a frontend handle;
 * SSLAM_ERR_UNSUPPORTED for on != 0 with the two handles on different devices. */
int sslam_slam_set_map_clouds(sslam_slam* s, int on, float keyframe_leaf /* 0 -> 0.1 */);
/* the number of map clouds kept so far and, in *n_points (optional), their points: a bound on the voxels sslam_slam_map_cloud can return.
 * Host only. */
int sslam_slam_map_clouds_kept(const sslam_slam* s, int32_t* n_points);
/* sslam_seg_map_cloud (resolution, min_points, the outputs, the order and the limits as stated there) over the processed keyframes that
 * hold a map cloud, in keyframe order.  Pose of a cloud: its keyframe's current graph estimate with the quaternion normalised, R the
 * matrix of that quaternion (the function of step 4 of the loop stage), t the translation.  Only the poses travel per call: after the
 * first call stats->upload_bytes is 48 bytes per cloud (12 floats) when no keyframe arrived in between, else that plus 12 bytes per
 * point of the clouds appended since the last call (a new cloud's boundary is written by a device fill, not a copy).
 * vertex_out / poses_out (optional, at most max_clouds clouds are written): the vertex id and the 12 doubles, before their cast to
 * float, of every cloud used -- what the map was built from; the same call through sslam_seg_map_cloud with the same clouds repeats it.
 * Returns the voxel count; 0 with map clouds off or none kept.  Errors: those of sslam_seg_map_cloud; SSLAM_ERR_INVALID also for a
 * negative max_clouds or an estimate that is not finite; SSLAM_ERR_UNSUPPORTED when clouds are kept and the two handles name different
 * devices (sslam_slam_set_map_clouds refuses that already; checked again because the kernels would read another device's memory). */
int sslam_slam_map_cloud(sslam_slam* s, float resolution, int min_points,
                         float* xyz_out, int32_t* cells_out, int32_t* counts_out, int max_out,
                         int32_t* vertex_out, double* poses_out, int max_clouds, sslam_map_stats* stats);
/* sslam_seg_occupancy_map (params, the outputs, the order and the limits as stated there) over the same kept clouds at the same poses as
 * sslam_slam_map_cloud -- where the reference's launch file runs octomap_server.  Only the poses travel: stats->upload_bytes is 48 bytes per
 * keyframe plus the bytes of the clouds appended since the last map or occupancy call.  Returns the record count; 0 with map clouds off or
 * none kept.  Errors: those of sslam_seg_occupancy_map and of sslam_slam_map_cloud. */
int sslam_slam_occupancy_map(sslam_slam* s, const sslam_occ_params* p, int32_t* cells_out, int32_t* hits_out, int32_t* misses_out,
                             float* logodds_out, int max_out, sslam_occ_stats* stats);
/* sslam_seg_occupancy_map_scans over the same kept clouds, at the same poses and through the same pose upload: every keyframe's cloud is one
 * scan, applied in keyframe order.  upload_bytes, the return value and the errors as for sslam_slam_occupancy_map. */
int sslam_slam_occupancy_map_scans(sslam_slam* s, const sslam_occ_params* p, int32_t* cells_out, int32_t* hits_out, int32_t* misses_out,
                                   float* logodds_out, int max_out, sslam_occ_stats* stats);
/* setPointCloudData (semantic_graph_slam.cpp:341-345): the cloud is copied */
int sslam_slam_set_point_cloud(sslam_slam* s, const uint8_t* cloud, int width, int height, int point_step, int row_step,
                               int off_x, int off_y, int off_z);
/* setDetectedObjectInfo (semantic_graph_slam.cpp:353-357) */
int sslam_slam_set_detected_objects(sslam_slam* s, const sslam_box* boxes, int n_boxes);
/* extension: objects segmented elsewhere (e.g. by one sslam_seg_segment_batch call over a recorded sequence) for the next keyframe;
 * they replace the frontend call of semantic_data_ass (semantic_graph_slam.cpp:217-219) and count as an available detection */
int sslam_slam_set_segmented_objects(sslam_slam* s, const sslam_plane* objects, int n);
/* VIOCallback (semantic_graph_slam.cpp:234-287): keyframe gate, dead-reckoned robot pose, queue.  Returns 1 when the odometry sample
 * became a keyframe, 0 when the gate rejected it. */
int sslam_slam_vio(sslam_slam* s, int32_t stamp_sec, int32_t stamp_nsec, const double odom_tq[7]);
/* run (semantic_graph_slam.cpp:58-102): returns 1 when keyframes were processed, 0 when the queue was empty.  On an error after the
 * queue was touched, the keyframes that reached the graph stay in it (once: sslam_slam_keyframes lists them), their objects are lost,
 * nothing is optimised in that call, and the next call associates against the landmark table uploaded again. */
int sslam_slam_run(sslam_slam* s, sslam_tick_stats* stats);
/* getRobotPose / getMap2OdomTrans / getVIOPose (semantic_graph_slam.cpp:375-381,333-339) */
int sslam_slam_robot_pose(const sslam_slam* s, double tq[7]);
int sslam_slam_map2odom(const sslam_slam* s, double tq[7]);
/* getMappedLandmarks (semantic_graph_slam.cpp:366-368): returns the number of landmarks (copies min(n, max)) */
int sslam_slam_landmarks(const sslam_slam* s, sslam_landmark* out, int max);
/* getKeyframes (semantic_graph_slam.cpp:370-373): graph vertex ids and current estimates (7 doubles each) of the processed keyframes */
int sslam_slam_keyframes(const sslam_slam* s, int32_t* vertex_ids, double* estimates_tq, int max);
/* the underlying GraphSLAM (saveGraph, semantic_graph_slam.cpp:391-394; borrowed) */
sslam_graph* sslam_slam_graph(sslam_slam* s);
/* data_association::find_matches (data_association.h:75-95) on its own: associates n segmented objects seen from robot_pose
 * (x,y,z,roll,pitch,yaw) against the mapped landmarks ON THE DEVICE and appends the new ones to the landmark list (without adding
 * graph vertices: parity hook for the association kernel).  out = n records.
 * A sslam_slam_run after the hook still optimises, but finds no marginal for the vertex-less landmarks: marginals_ok == 0, every
 * covariance keeps its value, no error is returned. */
int sslam_slam_find_matches(sslam_slam* s, const sslam_plane* objects, int n, const float robot_pose[6], sslam_landmark* out);

/* ---- scan-matching odometry (hdl_graph_slam's prefiltering_nodelet and scan_matching_odometry_nodelet [UPSTREAM, quoted from memory]):
 * the pose the orchestrator's sslam_slam_vio takes, computed from the clouds alone ----------------------------------------------------
 * pcl::RadiusOutlierRemoval (hdl's outlier_removal_method RADIUS; radius 0.8, 2 neighbours there).  The project's own rule, PCL's boundary
 * sense being [UPSTREAM, quoted from memory]: a finite point is kept when at least min_neighbors OTHER finite points lie within radius,
 * that is d2 <= r2 with d2 = (dx dx + dy dy) + dz dz in float32 without fused multiply-add, dx = x_query - x_candidate (the arithmetic of
 * the nearest-neighbour kernels), and r2 = (float)(radius * radius).  Duplicates of a point count as its neighbours.  A non-finite point
 * is never kept and never a neighbour.  keep_out: the ascending indices of the kept points, at most max_out of them; the return value is
 * the true count.  count_out (optional, n entries): the neighbours of every point, -1 for a non-finite one.  n = 0 returns 0.
 * SSLAM_ERR_INVALID: a NULL handle or xyz, n < 0, keep_out NULL with max_out > 0, a radius that is not finite and positive, a negative
 * min_neighbors.  SSLAM_ERR_NO_DEVICE without a GPU. */
int sslam_seg_radius_outlier_removal(sslam_seg* s, const float* xyz, int n, double radius, int min_neighbors, int32_t* keep_out, int max_out,
                                     int32_t* count_out);

/* The prefilter chain in hdl's order -- distance filter, downsample, outlier removal -- on ONE upload of xyz: the intermediate clouds stay on
 * the device (every stage's kept points go through the ordered compaction there), xyz_out comes back once.  The host reads back only what
 * sizes a launch: a count per stage, the bounding box of the voxel grid, the three moments (sum, sum of squares, number) of the
 * statistical stage.  The result is bit for bit the composition of sslam_seg_distance_filter + gather, sslam_seg_voxel_grid on the result,
 * and sslam_seg_statistical_outlier_removal or sslam_seg_radius_outlier_removal + gather.
 * A stage that is off passes its input on.  Non-finite points are dropped by the first stage that runs; where none has run when the chain
 * ends (all off, or the statistical stage skipped), the chain ends in a compaction of the finite points.  The statistical stage is
 * SKIPPED when fewer than mean_k + 1 finite points reach it (the stand-alone call refuses those), so a sparse frame is no error.
 * counts (optional): the points after each of the three stages.  An empty result is valid.  At most max_out points are written to
 * xyz_out; the return value is the true count.  kernel_ms (optional): hipEvent time from the first kernel to the last.
 * SSLAM_ERR_INVALID, before any device call: a NULL handle or params, xyz NULL with n > 0, n < 0, max_out < 0, xyz_out NULL with max_out > 0,
 * distance_near / distance_far NaN (with the distance filter on), leaf not positive and finite (VOXELGRID), mean_k outside 1 .. 63
 * or stddev_mul NaN (STATISTICAL), radius not finite and positive or min_neighbors < 0 (RADIUS), downsample or outlier not one of the
 * values below, a batch in flight.  SSLAM_ERR_UNSUPPORTED from the voxel geometry is passed on.  SSLAM_ERR_NO_DEVICE without a GPU. */
#define SSLAM_DOWNSAMPLE_NONE 0
#define SSLAM_DOWNSAMPLE_VOXELGRID 1
#define SSLAM_OUTLIER_NONE 0
#define SSLAM_OUTLIER_STATISTICAL 1
#define SSLAM_OUTLIER_RADIUS 2
typedef struct sslam_prefilter_params {
  int32_t use_distance_filter;      /* 1 */
  double  distance_near, distance_far;   /* 1.0, 100.0: kept when near < |p| < far, the rule of sslam_seg_distance_filter */
  int32_t downsample;               /* SSLAM_DOWNSAMPLE_VOXELGRID */
  float   leaf;                     /* 0.1 */
  int32_t outlier;                  /* SSLAM_OUTLIER_STATISTICAL */
  int32_t mean_k;                   /* 20 */
  double  stddev_mul;               /* 1.0 */
  double  radius;                   /* 0.8 */
  int32_t min_neighbors;            /* 2 */
} sslam_prefilter_params;
void sslam_prefilter_default_params(sslam_prefilter_params* p);
int sslam_seg_prefilter(sslam_seg* s, const float* xyz, int n, const sslam_prefilter_params* p, float* xyz_out, int max_out, int32_t counts[3],
                        double* kernel_ms);

/* The odometry handle: every frame is matched against the current KEYFRAME cloud, starting from the last relative transform; a new
 * keyframe is taken when the relative motion or the time since the last one passes a threshold (hdl's matching()).  On the host:
 * keyframe_pose and prev_trans (keyframe -> last accepted frame; 12 doubles each, R row-major then t) and the keyframe's stamp.  On the
 * device: the keyframe's filtered cloud and, under GICP, its covariances; the frame goes up once as raw points and only its 12 doubles
 * come back.  One push:
 *   1. the prefilter chain above on the frame; under GICP the covariances of the filtered frame, once (sslam_seg_cloud_covariances' kernel).
 *   2. no keyframe yet: an empty filtered frame returns SSLAM_ERR_NUMERIC and the handle stays without one; otherwise the frame becomes
 *      the keyframe, keyframe_pose = prev_trans = I, pose = I, new_keyframe = 1, accepted = 1, matched = 0.
 *   3. match: target = keyframe, source = frame, T0 = prev_trans, max_corr2 = max_correspondence_distance squared -- one pair of
 *      sslam_seg_register_pairs(_gicp) exactly (kernels, chunks of 8 iterations, the final fitness pass); under GICP the keyframe's
 *      covariances are those computed when it was a frame.  T: keyframe -> frame.
 *   4. status != 0 (fewer than 3 correspondences, a failed step) is "not converged" in hdl's sense; a match that merely reached
 *      max_iterations counts as converged, as PCL's criterion does (a deviation from a strict reading of hasConverged).  Not converged:
 *      pose = keyframe_pose * prev_trans, accepted = 0, nothing else changes.
 *   5. with transform_thresholding: delta = inverse(prev_trans) * T; |t(delta)| > max_acceptable_trans or angle(delta) >
 *      max_acceptable_angle: the frame is handled as in 4.
 *   6. otherwise pose = keyframe_pose * T, prev_trans = T, accepted = 1; delta_trans = |t(T)|, delta_angle = angle(T), delta_time =
 *      (sec - keyframe sec) + 1e-9 * (nsec - keyframe nsec) in double.
 *   7. any of the three STRICTLY above its keyframe_delta_* threshold: the frame's device cloud and covariances become the keyframe's
 *      (the two slots of the device arena swap roles; nothing crosses the host), keyframe_pose = pose, the stamp is kept, prev_trans = I,
 *      new_keyframe = 1.
 * angle(T) is upstream's acos(Quaternionf(R).w()), HALF the rotation angle -- an upstream quirk kept so that hdl's threshold values mean
 * what they mean there; here acos(min(1, |w|)) with w from the unit quaternion of R by the largest-pivot branch.
 * Products are plain double on the host, no fused multiply-add: C = A * B has R_C[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j]
 * and t_C[i] = ((A[i][0] t_B[0] + A[i][1] t_B[1]) + A[i][2] t_B[2]) + t_A[i]; inverse(A) has R = transpose(R_A) and
 * t[i] = -((A[0][i] t_A[0] + A[1][i] t_A[1]) + A[2][i] t_A[2]); |t| = sqrt((t0 t0 + t1 t1) + t2 t2).
 * Several odometry handles may share one frontend handle; they share no state.  A failed push leaves the handle as it was.
 * SSLAM_ERR_INVALID: NULL arguments (stats may be NULL), n < 0, parameters out of range (the checks of the prefilter and of the
 * generalized-ICP parameters; max_iterations < 0; epsilon, the correspondence distance or one of the five thresholds not finite and
 * >= 0; a method other than the two), a frontend batch in flight.  create checks the handle and the parameters and returns NULL on a
 * bad one, with the reason in sslam_last_error.
 * SSLAM_ERR_NO_DEVICE without a GPU: create succeeds and push fails. */
typedef struct sslam_odom sslam_odom;
typedef struct sslam_odom_params {
  sslam_prefilter_params prefilter;
  int32_t method;                   /* SSLAM_REG_GICP (hdl's default is FAST_GICP) | SSLAM_REG_ICP */
  sslam_gicp_params gicp;           /* 20, 1e-3 */
  int32_t max_iterations;           /* 64 */
  double  epsilon;                  /* 0.01: the rule of sslam_seg_register_pairs, the largest change of an entry of T */
  double  max_correspondence_distance;   /* 2.5; squared before use */
  double  keyframe_delta_trans, keyframe_delta_angle, keyframe_delta_time;   /* 0.25 m, 0.15 (see angle), 1.0 s */
  int32_t transform_thresholding;   /* 0 */
  double  max_acceptable_trans, max_acceptable_angle;   /* 1.0, 1.0 */
} sslam_odom_params;
typedef struct sslam_odom_stats {
  int32_t n_raw, n_filtered;        /* points of the frame before and after the prefilter */
  int32_t matched;                  /* 1 when the frame was matched against a keyframe (0 for the frame that became the first one) */
  int32_t iterations, converged, status, used;   /* as sslam_reg_result has them; 0 without a match */
  int32_t accepted, new_keyframe, keyframes;     /* keyframes: taken so far, this call included */
  int64_t covariance_passes;        /* covariance launches of the handle so far: one per pushed frame under GICP, none per keyframe */
  double  fitness;                  /* the Euclidean fitness score at the final T; 0 without a match */
  double  T[12];                    /* keyframe -> frame, what the pose was built from: the match's T when accepted, else prev_trans */
  double  delta_trans, delta_angle, delta_time;  /* of an accepted frame; 0 otherwise */
  double  prefilter_ms, covariance_ms, registration_ms;   /* hipEvent times */
  double  total_ms;                 /* the whole call, wall clock */
} sslam_odom_stats;
void        sslam_odom_default_params(sslam_odom_params* p);
sslam_odom* sslam_odom_create(sslam_seg* seg, const sslam_odom_params* p);   /* p NULL: the defaults; seg is borrowed and must outlive the handle */
void        sslam_odom_destroy(sslam_odom* o);
int         sslam_odom_reset(sslam_odom* o);                                 /* forgets the keyframe and the counters; returns 0 */
int         sslam_odom_push(sslam_odom* o, const float* xyz, int n, int32_t stamp_sec, int32_t stamp_nsec, double pose_out[12], sslam_odom_stats* stats);
/* the current keyframe's filtered cloud (at most max_out points; returns the true count, 0 without a keyframe) and its pose (optional) */
int         sslam_odom_keyframe(const sslam_odom* o, float* xyz_out, int max_out, double pose_out[12]);

#ifdef __cplusplus
}
#endif
#endif /* SSLAM_H */
