/* include/viorb_essential_graph.h — the essential-graph optimisation of loop closing in the C ABI. Included by viorb.h (after the global
 * bundle adjustments, whose info layout and viorb_debug_gba_last_trials it shares); include viorb.h, not this file. The ctypes mirror is
 * viorb_amd/capi.py: SIGNATURES_ESSENTIAL_GRAPH. */
#ifndef VIORB_ESSENTIAL_GRAPH_H
#define VIORB_ESSENTIAL_GRAPH_H
#ifndef VIORB_H
#error "include viorb.h"
#endif

/* Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:4313-4587, BlockSolver_7_3; called by LoopClosing::CorrectLoop,
 * src/LoopClosing.cc:593): a pose graph over every key frame of the map as a Sim3 (VertexSim3Expmap, 7), one EdgeSim3 per edge of the
 * essential graph (error = log(C * S_i * S_j^-1), information = identity, no robust kernel, numeric Jacobians), ONE
 * optimize(cfg->iterations) of g2o's Levenberg with setUserLambdaInit(1e-16), then the write-back of key-frame poses and map points.
 * The choice of edges and CorrectLoop's propagation stay with the caller (the covisibility update and LoopConnections are
 * viorb_update_connections, viorb_covisibility.h); this is the solve.
 * A Sim3 is 8 doubles r(x y z w) t s, as viorb_sim3_opt_inputs::S12.
 *   Scw [nk][8]        vScw, the vertex estimate: the CorrectedSim3 entry where there is one, else (Rcw, tcw, 1)
 *   Smeas [nk][8]      the NonCorrectedSim3 entry where there is one, else the same row as Scw
 *   fixed [nk]         the reference fixes pLoopKF; at least one fixed vertex is required (with lambda = 1e-16 nothing else holds the gauge)
 *   edge_idx [ne][2]   (vertex 0 = i, vertex 1 = j); its measurement is Sji = Sjw * Swi
 *   edge_corrected[ne] 1: a LoopConnections edge (:4385-4413), both operands of Sji from Scw; 0: a spanning-tree, loop or covisibility
 *                      edge (:4416-4516), both from Smeas. Two edges may join the same pair; an edge between two fixed vertices adds
 *                      to chi2 only.
 *   points [np][3]     float world positions; point_ref [np]: the index of mnCorrectedReference or of the reference key frame, -1: the
 *                      point is skipped and copied
 * Outputs: Scw_out [nk][8] (fixed rows copied; a free vertex without an edge keeps its estimate), Tcw_out [nk][12] = R row-major then
 * t / s, points_out [np][3] = correctedSwr.map(Srw.map(P)) with Srw the INPUT Scw of the point's reference, rounded to float once,
 * info = chi2 before, chi2 after, iterations, trials, final lambda, failed factorisations. viorb_debug_gba_last_trials reports this
 * solve too. There is no stop flag: the reference's call has none.
 * VIORB_ERR_INVALID_ARG: an edge index out of range or i == j, a pose that is not finite or has a scale <= 0, a point_ref outside
 * -1..nk-1, no fixed vertex. VIORB_ERR_CAPACITY: more than 3510 free key frames (a system of order 24570), or a workspace that is too
 * small; never a truncated solve. FP64 on the calling thread's current HIP device; the host form is re-entrant. */
typedef struct viorb_eg_config { int32_t iterations; int32_t fix_scale; } viorb_eg_config;
size_t viorb_essential_graph_workspace_bytes(int nk, int ne, int np);
int viorb_optimize_essential_graph(const viorb_eg_config* cfg, const double* Scw, const double* Smeas, const uint8_t* fixed, int nk,
                                   const int32_t* edge_idx, const uint8_t* edge_corrected, int ne, const float* points,
                                   const int32_t* point_ref, int np, double* Scw_out, double* Tcw_out, float* points_out, double info[6]);
/* The same with the arrays in device memory (Scw_out is the working state and must not alias Scw); cfg and info are host pointers.
 * workspace: viorb_essential_graph_workspace_bytes(nk, ne, np) bytes of device memory; its contents on entry are ignored. The argument
 * checks run in a kernel. */
int viorb_optimize_essential_graph_device(const viorb_eg_config* cfg, const double* Scw, const double* Smeas, const uint8_t* fixed, int nk,
                                          const int32_t* edge_idx, const uint8_t* edge_corrected, int ne, const float* points,
                                          const int32_t* point_ref, int np, double* Scw_out, double* Tcw_out, float* points_out,
                                          double info[6], void* workspace, size_t workspace_bytes, void* stream);
/* Test hooks (no device), essential_graph_core.h compiled for the host: g2o's Sim3::log of S8 (omega, upsilon, sigma); one EdgeSim3
 * with measurement C8 between the estimates Si8 (vertex 0) and Sj8 (vertex 1): e7 and the numeric Jacobians Ji49 / Jj49 [7][7] (row =
 * error row), all zero for a fixed side. */
int viorb_debug_sim3_log(const double* S8, double* out7);
int viorb_debug_essential_graph_edge(const double* Si8, const double* Sj8, const double* C8, int fix_scale, int fixed_i, int fixed_j,
                                     double* e7, double* Ji49, double* Jj49);

#endif /* VIORB_ESSENTIAL_GRAPH_H */
