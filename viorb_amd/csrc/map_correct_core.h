// viorb_amd/csrc/map_correct_core.h — the propagation of LoopClosing::CorrectLoop over the current key frame's covisibles, shared by the HIP
// kernels of map_correction.hip and by the host (viorb_debug_correct_loop_host; tests/cpp/map_correct_core_host_test.cpp drives this
// header alone, under the address and undefined-behaviour sanitizers, against the literal loop).
//
// What is restated (reference file:line):
//   LoopClosing::CorrectLoop          src/LoopClosing.cc:460-542 (CorrectedSim3 / NonCorrectedSim3 :473-495, the ordered point pass
//                                     :498-527, the key-frame poses :530-538; UpdateConnections :541 is covisibility.hip)
//   KeyFrame::SetPose                 src/KeyFrame.cc:361-375 (Rwc, Ow, Twc)
//   MapPoint::UpdateNormalAndDepth    src/MapPoint.cc:337-378
//   Converter::toCvMat(g2o::Sim3)     src/Converter.cc:93-99
// Float / double placement is the audit table of DESIGN.md §2 ("Map correction"). The only ordered part is who corrects a point: the
// member key frame with the lowest key that holds it, which is an integer minimum (snap_min) over the members' keypoints. Everything
// after that is per key frame or per point. The float sum of a normal runs in ascending key of the observers whatever order the
// snapshot lists them in: every term is stored at its key position among the observers first and the sum walks the positions.
// The second half of the file (ag_*) is the map update after a global bundle adjustment, src/LoopClosing.cc:712-803 =
// src/LocalMapping.cc:824-916, with KeyFrame::UpdatePoseFromNS (src/KeyFrame.cc:102-119) and Converter::toCvMatInverse.
#pragma once
#include <stdint.h>
#include <string.h>
#include "sim3_core.h"              // sim3d, sim3_mul / sim3_inv / sim3_map; vio_core.h: mat2q, qmat; mapping_core.h: map_norm3d
#include "map_snapshot_core.h"      // the snapshot's layout, its observation word, the validator's checks, the memory shim

namespace viorb {

enum { MC_OK = 0, MC_INVALID = -1 };
enum { MC_NO_CLAIM = 0x7fffffff, MC_MEMBER = 0x10000, MC_RANK = 0xffff };     // claim[p] of a point no member corrects; key[k] = rank | member bit

// The snapshot (viorb_correct_loop_map with the scale table), the working state (the workspace; host: plain arrays) and the result
struct ClMap {
    int batch, n_kf, n_kp, n_pt, n_obs, n_conn;
    const int32_t* kf_start; const int32_t* kf_by_key; const int32_t* kp_start; const int32_t* kp_point;
    const int32_t* pt_start; const uint8_t* pt_bad; const int32_t* obs_start; const uint32_t* obs;
    const float* pose12; const float* pts_f; const int32_t* pt_ref; const int32_t* pt_corrected_by;
    const int32_t* cur_kf; const int32_t* cur_id; const double* Scw8; const int32_t* conn_start; const int32_t* conn_kf;
    float sf[16]; int nlevels;           // mvScaleFactors; the levels from nlevels on repeat the last
};
struct ClWork {
    int32_t* key;                        // [n_kf]: a slot's key position (the permutation check's marks), MC_MEMBER added for a member
    int32_t* memb;                       // [n_kf]: -1, or the member's ordinal in the list, the current key frame last (the distinct check's marks)
    int32_t* claim;                      // [n_pt]: the lowest key position of a member that corrects the point, or MC_NO_CLAIM
    float* Ow_in;                        // [n_kf][3]: the camera centre of the input pose
    double* Swi;                         // [n_kf][8]: the inverse of CorrectedSim3 (members)
    int32_t* terms;                      // [n_obs][3]: the unit vectors of a point's normal as float bits, in key order of the observers
    int32_t* info;                       // [batch]: accepted
};
struct ClOut {
    int32_t* status; int32_t* n_member; int32_t* member_kf; float* Scw_f12; double* Scw_out; double* Smeas_out; float* pose12_out; float* Ow_out;
    float* pts_f_out; int32_t* pt_corrected_by_out; int32_t* pt_corrected_ref_out; uint8_t* pt_touched;
};

#if defined(__HIP_DEVICE_COMPILE__)
VIORB_HD int32_t mc_f2i(float v) { return __float_as_int(v); }
VIORB_HD float mc_i2f(int32_t v) { return __int_as_float(v); }
#else
VIORB_HD int32_t mc_f2i(float v) { int32_t o; memcpy(&o, &v, 4); return o; }
VIORB_HD float mc_i2f(int32_t v) { float o; memcpy(&o, &v, 4); return o; }
#endif

// ---- arithmetic ----------------------------------------------------------------------------------------------------------------------------
// KeyFrame::SetPose (:365-368): Rwc = Rcw^T, Ow = -Rwc * tcw. The negation is applied to the entries before the products (a sign change
// is exact, so where it stands does not matter), the products are summed left to right in float (oracle/README.md row 13).
VIORB_HD void mc_camera_centre(const float* T, float* Ow) {
#pragma unroll
    for (int r = 0; r < 3; r++) Ow[r] = ((-T[r]) * T[9] + (-T[3 + r]) * T[10]) + (-T[6 + r]) * T[11];
}
// Sim3(toMatrix3d(R), toVector3d(t), 1.0) of a float pose (:484, :492): widened to double, Eigen's Quaterniond(Matrix3d), not normalised
VIORB_HD sim3d mc_sim3_of_pose(const float* R, const float* t) {
    sim3d o;
    o.r = mat2q(mkm(R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8]));
    o.t = mk3((double)t[0], (double)t[1], (double)t[2]); o.s = 1.0;
    return o;
}
// Tic = Tiw * Twc (:481), 4 x 4 float: every entry is four products summed left to right in float, the zeros of Twc's last row and its
// one included. Ti: the pose of key frame i; Tc, Owc: the pose and the centre of the current key frame, Rwc[k][c] = Tc[3 * c + k].
VIORB_HD void mc_Tic(const float* Ti, const float* Tc, const float* Owc, float* Ric, float* tic) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) Ric[3 * r + c] = ((Ti[3 * r] * Tc[3 * c] + Ti[3 * r + 1] * Tc[3 * c + 1]) + Ti[3 * r + 2] * Tc[3 * c + 2]) + Ti[9 + r] * 0.0f;
        tic[r] = ((Ti[3 * r] * Owc[0] + Ti[3 * r + 1] * Owc[1]) + Ti[3 * r + 2] * Owc[2]) + Ti[9 + r] * 1.0f;
    }
}
// toCvSE3(qmat(r), t * (1. / s)) rounded to float (:530-536)
VIORB_HD void mc_pose_of_sim3(const sim3d& S, float* T12) {
    double R[9];
    stm(R, qmat(S.r));
    const d3 t = S.t * (1. / S.s);
#pragma unroll
    for (int i = 0; i < 9; i++) T12[i] = (float)R[i];
    T12[9] = (float)t.x; T12[10] = (float)t.y; T12[11] = (float)t.z;
}
// Converter::toCvMat(Sim3): the top three rows of [s * R | t] rounded to float, as the Sim3 matchers read a similarity
VIORB_HD void mc_f12_of_sim3(const sim3d& S, float* T12) {
    double R[9];
    stm(R, scl(qmat(S.r), S.s));
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) T12[4 * r + c] = (float)R[3 * r + c];
    T12[3] = (float)S.t.x; T12[7] = (float)S.t.y; T12[11] = (float)S.t.z;
}
VIORB_HD bool mc_finite12(const float* v) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; i++) ok &= (v[i] - v[i] == 0.0f);
    return ok;
}
VIORB_HD bool mc_sim3_ok(const double* S8) {
    bool ok = S8[7] > 0.0;
#pragma unroll
    for (int k = 0; k < 8; k++) ok &= (S8[k] - S8[k] == 0.0);
    return ok;
}

// ---- the stream validator: the steps of map_snapshot_core.h on this snapshot's arrays ----------------------------------------------------
// Step 1: kp_start is nested under kf_start, obs_start under pt_start; conn_start is a batch-level array.
VIORB_HD bool cl_validate_ranges(const ClMap& M, int b, int tid, int nt) {
    bool ok = true;
    for (int i = tid; i <= b; i += nt) {
        if (!(snap_span(M.kf_start, i, i + 1, M.n_kf) && snap_span(M.pt_start, i, i + 1, M.n_pt) && snap_span(M.conn_start, i, i + 1, M.n_conn))) { ok = false; continue; }
        ok = ok && snap_span(M.kp_start, M.kf_start[i], M.kf_start[i + 1], M.n_kp) && snap_span(M.obs_start, M.pt_start[i], M.pt_start[i + 1], M.n_obs);
    }
    return ok;
}
// Step 2: the nested offsets, the stream's scalars, every key frame's pose and its entry of kf_by_key, the covisible list.
VIORB_HD bool cl_validate_offsets(const ClMap& M, const SnapStream& S, int b, int tid, int nt) {
    bool ok = S.nk <= SNAP_MAX_KF && M.cur_kf[b] >= 0 && M.cur_kf[b] < S.nk && mc_sim3_ok(M.Scw8 + 8 * (size_t)b);
    ok &= snap_offsets_run(M.kp_start, S.k0, S.nk, M.n_kp, tid, nt);
    ok &= snap_offsets_run(M.obs_start, S.p0, S.np, M.n_obs, tid, nt);
    for (int k = tid; k < S.nk; k += nt) {
        const int key = M.kf_by_key[S.k0 + k];
        ok &= key >= 0 && key < S.nk && mc_finite12(M.pose12 + 12 * (size_t)(S.k0 + k));
    }
    ok &= snap_entries_within(M.conn_kf, M.conn_start[b], M.conn_start[b + 1], 0, S.nk, tid, nt);
    return ok;
}
// Step 3: every slot of the observations.
VIORB_HD bool cl_validate_entries(const ClMap& M, const SnapStream& S, int tid, int nt) {
    return snap_obs_slots_below(M.obs, M.obs_start[S.p0], M.obs_start[S.p0 + S.np], S.nk, tid, nt);
}
// Step 4 is snap_distinct_fill / snap_distinct_check of kf_by_key on key[], which leaves key = the inverse permutation, and the same on
// memb[] for the members: the list and, with the ordinal behind it, the current key frame, so that a list that names a slot twice or names
// the current key frame loses a mark. cl_members_clear, a barrier, cl_members_fill, a barrier, cl_members_check.
VIORB_HD void cl_members_clear(const ClMap& M, const SnapStream& S, const ClWork& W, int tid, int nt) {
    for (int k = tid; k < S.nk; k += nt) W.memb[S.k0 + k] = -1;
    for (int p = tid; p < S.np; p += nt) W.claim[S.p0 + p] = MC_NO_CLAIM;
}
// member j of the stream in list order: conn_kf, then the current key frame
VIORB_HD int cl_member(const ClMap& M, int b, int j) { const int c0 = M.conn_start[b], n = M.conn_start[b + 1] - c0; return j < n ? M.conn_kf[c0 + j] : M.cur_kf[b]; }
VIORB_HD void cl_members_fill(const ClMap& M, const SnapStream& S, const ClWork& W, int b, int tid, int nt) {
    for (int j = tid, n = M.conn_start[b + 1] - M.conn_start[b] + 1; j < n; j += nt) W.memb[S.k0 + cl_member(M, b, j)] = j;
}
VIORB_HD bool cl_members_check(const ClMap& M, const SnapStream& S, const ClWork& W, int b, int tid, int nt) {
    bool ok = true;
    for (int j = tid, n = M.conn_start[b + 1] - M.conn_start[b] + 1; j < n; j += nt) ok &= W.memb[S.k0 + cl_member(M, b, j)] == j;
    return ok;
}
// Step 5, the members' keypoints, the only ones read: a point index within the stream; a good, observed point has its reference key frame
// among its observers. The same walk makes the claims (:498-515): a point that is not bad and not yet corrected by this loop goes to the
// member with the lowest key that holds it. A stream refused here has written claims: they are working state and nobody reads them.
VIORB_HD bool cl_validate_and_claim(const ClMap& M, const SnapStream& S, const ClWork& W, int b, int tid, int nt) {
    bool ok = true;
    const int cur_id = M.cur_id[b];
    for (int j = 0, n = M.conn_start[b + 1] - M.conn_start[b] + 1; j < n; j++) {
        const int k = cl_member(M, b, j), g = S.k0 + k, rank = W.key[g];
        for (int i = M.kp_start[g] + tid, e = M.kp_start[g + 1]; i < e; i += nt) {
            const int p = M.kp_point[i];
            if (p < -1 || p >= S.np) { ok = false; continue; }
            if (p < 0 || M.pt_bad[S.p0 + p]) continue;                                          // :510-513
            const int gp = S.p0 + p, o0 = M.obs_start[gp], o1 = M.obs_start[gp + 1], ref = M.pt_ref[gp];
            bool found = o0 == o1;
            for (int o = o0; o < o1; o++) found |= snap_obs_slot(M.obs[o]) == ref;
            ok &= found;
            if (M.pt_corrected_by[gp] != cur_id) snap_min(&W.claim[gp], rank);                  // :514
        }
    }
    return ok;
}

// ---- key frames (:473-495, :530-538): the share of key frame k of an accepted stream ------------------------------------------------------
VIORB_HD void cl_key_frame(const ClMap& M, const SnapStream& S, const ClWork& W, const ClOut& R, int b, int k) {
    const int g = S.k0 + k, cur = M.cur_kf[b], j = W.memb[g], rank = W.key[g];
    float T[12], Ow[3];
#pragma unroll
    for (int i = 0; i < 12; i++) T[i] = M.pose12[12 * (size_t)g + i];
    mc_camera_centre(T, Ow);
    const sim3d Siw = mc_sim3_of_pose(T, T + 9);                                                // :490-494
    sim3_st(R.Smeas_out + 8 * (size_t)g, Siw);
#pragma unroll
    for (int i = 0; i < 3; i++) W.Ow_in[3 * (size_t)g + i] = Ow[i];
    if (j < 0) {                                                                                // not a member: as the essential graph reads it
        sim3_st(R.Scw_out + 8 * (size_t)g, Siw);
#pragma unroll
        for (int i = 0; i < 12; i++) R.pose12_out[12 * (size_t)g + i] = T[i];
#pragma unroll
        for (int i = 0; i < 3; i++) R.Ow_out[3 * (size_t)g + i] = Ow[i];
        return;
    }
    sim3d C = sim3_ld(M.Scw8 + 8 * (size_t)b);                                                  // :465
    if (k != cur) {                                                                             // :481-487
        float Tc[12], Owc[3], Ric[9], tic[3];
#pragma unroll
        for (int i = 0; i < 12; i++) Tc[i] = M.pose12[12 * (size_t)(S.k0 + cur) + i];
        mc_camera_centre(Tc, Owc);
        mc_Tic(T, Tc, Owc, Ric, tic);
        C = sim3_mul(mc_sim3_of_pose(Ric, tic), C);
    }
    sim3_st(R.Scw_out + 8 * (size_t)g, C);
    sim3_st(W.Swi + 8 * (size_t)g, sim3_inv(C));                                                // :502
    float Tn[12], Own[3], F[12];
    mc_pose_of_sim3(C, Tn);
    mc_camera_centre(Tn, Own);
    mc_f12_of_sim3(C, F);
    // its position among the members in ascending key: the order of CorrectedSim3
    int at = 0;
    const int m0 = M.conn_start[b] + b, n = M.conn_start[b + 1] - M.conn_start[b] + 1;
    for (int i = 0; i < n; i++) at += (W.key[S.k0 + cl_member(M, b, i)] & MC_RANK) < (rank & MC_RANK) ? 1 : 0;
    R.member_kf[m0 + at] = k;
#pragma unroll
    for (int i = 0; i < 12; i++) { R.pose12_out[12 * (size_t)g + i] = Tn[i]; R.Scw_f12[12 * (size_t)(m0 + at) + i] = F[i]; }
#pragma unroll
    for (int i = 0; i < 3; i++) R.Ow_out[3 * (size_t)g + i] = Own[i];
}
// after every key frame's share has read key[]: the member bit
VIORB_HD void cl_mark_members(const ClMap& M, const SnapStream& S, const ClWork& W, int b, int tid, int nt) {
    for (int j = tid, n = M.conn_start[b + 1] - M.conn_start[b] + 1; j < n; j += nt) W.key[S.k0 + cl_member(M, b, j)] |= MC_MEMBER;
}

// ---- points (:507-526) -----------------------------------------------------------------------------------------------------------------------
// Point p of an accepted stream, one lane: moved by its claimer or copied. Returns the claim; Pn = the new position of a moved point.
VIORB_HD int cl_point_move(const ClMap& M, const SnapStream& S, const ClWork& W, const ClOut& R, int b, int p, float* Pn) {
    const size_t g = (size_t)(S.p0 + p);
    const int c = W.claim[g];
    const float* in = M.pts_f + 8 * g; float* out = R.pts_f_out + 8 * g;
    if (c == MC_NO_CLAIM) {
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = in[i];
        R.pt_corrected_by_out[g] = M.pt_corrected_by[g]; R.pt_corrected_ref_out[g] = -1; R.pt_touched[g] = 0;
        return c;
    }
    const int m = M.kf_by_key[S.k0 + c];
    const sim3d Siw = sim3_ld(R.Smeas_out + 8 * (size_t)(S.k0 + m)), Swi = sim3_ld(W.Swi + 8 * (size_t)(S.k0 + m));
    const d3 q = sim3_map(Swi, sim3_map(Siw, mk3((double)in[0], (double)in[1], (double)in[2])));        // :518-520
    Pn[0] = (float)q.x; Pn[1] = (float)q.y; Pn[2] = (float)q.z;
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = Pn[i];
    R.pt_corrected_by_out[g] = M.cur_id[b]; R.pt_corrected_ref_out[g] = m; R.pt_touched[g] = 1;
    return c;
}
// The camera centre of observer s when the point's claimer, at key position c, runs UpdateNormalAndDepth: the corrected one when s is a
// member strictly below c (its SetPose, :538, has run), else the input one. Selected by value.
VIORB_HD const float* cl_centre(const ClWork& W, const ClOut& R, const SnapStream& S, const int32_t* key, int s, int c) {
    const int k = key[s];
    const bool corrected = (k & MC_MEMBER) && (k & MC_RANK) < c;
    return (corrected ? R.Ow_out : W.Ow_in) + 3 * (size_t)(S.k0 + s);
}
// UpdateNormalAndDepth (MapPoint.cc:337-378) of moved point p at Pn, claimed at key position c, by `nl` lanes in step (the device: one
// wavefront; the host: lane 0 of 1). key: the stream's key[] (device: in LDS while the stream's key frames fit).
VIORB_HD void cl_point_normal(const ClMap& M, const SnapStream& S, const ClWork& W, const ClOut& R, const int32_t* key, int p, int c, const float* Pn, int lane, int nl) {
    const size_t g = (size_t)(S.p0 + p);
    const int o0 = M.obs_start[g], n = M.obs_start[g + 1] - o0;
    float* out = R.pts_f_out + 8 * g;
    if (n == 0) {                                                                               // :352: the normal and the range stay
        for (int i = 3 + lane; i < 8; i += nl) out[i] = M.pts_f[8 * g + i];
        return;
    }
    for (int i = lane; i < n; i += nl) {
        const int s = snap_obs_slot(M.obs[o0 + i]), rs = key[s] & MC_RANK;
        int pos = 0;                                                                            // the observers before it in mObservations
        for (int j = 0; j < n; j++) { const int rj = key[snap_obs_slot(M.obs[o0 + j])] & MC_RANK; pos += (rj < rs || (rj == rs && j < i)) ? 1 : 0; }
        const float* Ow = cl_centre(W, R, S, key, s, c);
        const float d0 = Pn[0] - Ow[0], d1 = Pn[1] - Ow[1], d2 = Pn[2] - Ow[2];                 // :361
        const double nrm = map_norm3d(d0, d1, d2);
        int32_t* t = W.terms + 3 * (size_t)(o0 + pos);
        snap_st_wg(&t[0], mc_f2i((float)((double)d0 / nrm))); snap_st_wg(&t[1], mc_f2i((float)((double)d1 / nrm))); snap_st_wg(&t[2], mc_f2i((float)((double)d2 / nrm)));
    }
    snap_fence_wg();
    for (int x = lane; x < 3; x += nl) {                                                        // :362 in mObservations' order, :376
        float acc = 0.0f;
        for (int j = 0; j < n; j++) acc = acc + mc_i2f(snap_ld_wg(&W.terms[3 * (size_t)(o0 + j) + x]));
        out[3 + x] = (float)((double)acc / (double)n);
    }
    if (lane == 0) {                                                                            // :366-375
        const int ref = M.pt_ref[g];
        int oct = 0, seen = 0;
        for (int j = 0; j < n; j++) { const uint32_t w = M.obs[o0 + j]; const int hit = snap_obs_slot(w) == ref && !seen; oct = hit ? snap_obs_octave(w) : oct; seen |= hit; }
        const float* Ow = cl_centre(W, R, S, key, ref, c);
        const float dist = (float)map_norm3d(Pn[0] - Ow[0], Pn[1] - Ow[1], Pn[2] - Ow[2]);
        const float maxd = dist * M.sf[oct > 15 ? 15 : oct];
        out[7] = maxd; out[6] = maxd / M.sf[M.nlevels - 1];
    }
}

VIORB_HD void cl_write_status(const ClOut& R, int b, bool ok, int n_member) { R.status[b] = ok ? MC_OK : MC_INVALID; if (ok) R.n_member[b] = n_member; }

// The phases of the device form on one host thread, stream by stream. W holds arrays of the sizes ClWork names.
inline void cl_run_host(const ClMap& M, const ClWork& W, const ClOut& R) {
    for (int b = 0; b < M.batch; b++) {
        bool ok = cl_validate_ranges(M, b, 0, 1);
        SnapStream S = {0, 0, 0, 0};
        if (ok) { S = snap_stream(M.kf_start, M.pt_start, b); ok = cl_validate_offsets(M, S, b, 0, 1); }
        ok = ok && cl_validate_entries(M, S, 0, 1);
        if (ok) { snap_distinct_fill(M.kf_by_key + S.k0, S.nk, W.key + S.k0, 0, 1); ok = snap_distinct_check(M.kf_by_key + S.k0, S.nk, W.key + S.k0, 0, 1); }
        if (ok) { cl_members_clear(M, S, W, 0, 1); cl_members_fill(M, S, W, b, 0, 1); ok = cl_members_check(M, S, W, b, 0, 1); }
        ok = ok && cl_validate_and_claim(M, S, W, b, 0, 1);
        W.info[b] = ok;
        cl_write_status(R, b, ok, ok ? M.conn_start[b + 1] - M.conn_start[b] + 1 : 0);
        if (!ok) continue;
        for (int k = 0; k < S.nk; k++) cl_key_frame(M, S, W, R, b, k);
        cl_mark_members(M, S, W, b, 0, 1);
        for (int p = 0; p < S.np; p++) {
            float Pn[3] = {0.0f, 0.0f, 0.0f};
            const int c = cl_point_move(M, S, W, R, b, p, Pn);
            if (c != MC_NO_CLAIM) cl_point_normal(M, S, W, R, W.key + S.k0, p, c, Pn, 0, 1);
        }
    }
}

// ==== the map update after a global bundle adjustment (src/LoopClosing.cc:712-803 = src/LocalMapping.cc:824-916) ============================
// A breadth-first walk of the spanning tree from mvpKeyFrameOrigins carries mTcwGBA / mNavStateGBA to the key frames the adjustment did not
// contain; every reached key frame takes its GBA NavState and the pose UpdatePoseFromNS derives from it; every good point moves to mPosGBA
// or through its reference key frame. The walk's order decides nothing: a key frame outside the adjustment depends on its parent only,
// so a lane per key frame walks up to its anchor (the nearest ancestor inside the adjustment, or the root) and multiplies back down.
enum { AG_BAD = 0, AG_POS_GBA = 1, AG_BY_REF = 2, AG_UNTOUCHED = 3, AG_REF_UNREACHED = 4 };       // pt_code (VIORB_AGBA_PT_*)

struct AgMap {
    int batch, n_kf, n_child, n_origin, n_pt;
    const int32_t* kf_start; const int32_t* child_start; const int32_t* child_kf; const int32_t* origin_start; const int32_t* origin_kf;
    const uint8_t* kf_in_gba; const float* pose12; const float* TcwGBA12; const double* ns22; const double* nsGBA22;
    const int32_t* pt_start; const uint8_t* pt_bad; const uint8_t* pt_in_gba; const float* Pw; const float* PosGBA; const int32_t* pt_ref;
    float Tbc[12];
};
struct AgWork {
    int32_t* parent;                     // [n_kf]: the slot whose child list names the key frame, or -1
    int32_t* count;                      // [n_kf]: how many child lists name it
    int32_t* mark;                       // [n_kf]: -1, or the ordinal of the origin (the distinct check's marks)
    int32_t* info;                       // [batch]: accepted
};
struct AgOut {
    int32_t* status; float* pose12_out; double* ns22_out; float* TcwBef_out; double* nsBef_out; float* TcwGBA_out; double* nsGBA_out;
    uint8_t* kf_in_gba_out; uint8_t* kf_reached; float* Pw_out; uint8_t* pt_code;
};

// C = A * B of two poses as 4 x 4 float matrices (cv::Mat operator*, the small-matrix gemm): four products per entry summed left to
// right in float, the 0 0 0 1 of B's last row included
VIORB_HD void mc_mul44(const float* A, const float* B, float* C) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) C[3 * r + c] = ((A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c]) + A[9 + r] * 0.0f;
        C[9 + r] = ((A[3 * r] * B[9] + A[3 * r + 1] * B[10]) + A[3 * r + 2] * B[11]) + A[9 + r] * 1.0f;
    }
}
VIORB_HD bool mc_finite_d(const double* v, int n) { bool ok = true; for (int i = 0; i < n; i++) ok &= (v[i] - v[i] == 0.0); return ok; }
VIORB_HD bool mc_finite3(const float* v) { return (v[0] - v[0] == 0.0f) && (v[1] - v[1] == 0.0f) && (v[2] - v[2] == 0.0f); }

// KeyFrame::UpdatePoseFromNS (src/KeyFrame.cc:102-119) of a NavState row: the stored quaternion as it is (Get_RotMatrix), the float
// arithmetic of pose_from_navstate_f32
VIORB_HD void ag_pose_of_ns(const double* ns, const float* Tbc, float* pose12) {
    pvr s; s.P = ld3(ns); s.V = ld3(ns + 3); s.q = mkq(ns[6], ns[7], ns[8], ns[9]);
    double cam16[16];
#pragma unroll
    for (int i = 0; i < 4; i++) cam16[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) cam16[4 + i] = (double)Tbc[i];
#pragma unroll
    for (int i = 0; i < 3; i++) cam16[13 + i] = (double)Tbc[9 + i];
    pose_from_navstate_f32(s, cam16, pose12);
}
// mNavStateGBA of a child outside the adjustment (:739-748): its NavState with P, R, V replaced from TwbGBA = toCvMatInverse(Tbc * TcwGBA)
VIORB_HD void ag_ns_of_pose(const double* ns_child, const float* Tbc, const float* TcwGBA, double* out22) {
    float Tbw[12], Pwb[3];
    mc_mul44(Tbc, TcwGBA, Tbw);
    mc_camera_centre(Tbw, Pwb);                                                                 // twc = -Rwc * tcw of toCvMatInverse
    const m33 Rwb = mkm(Tbw[0], Tbw[3], Tbw[6], Tbw[1], Tbw[4], Tbw[7], Tbw[2], Tbw[5], Tbw[8]);   // Rbw^T, widened
    const m33 Rw1 = qmat(mkq(ns_child[6], ns_child[7], ns_child[8], ns_child[9]));
    const d3 V2 = mulv(mul(Rwb, tr(Rw1)), ld3(ns_child + 3));                                   // RwbGBA * Rw1.transpose() * Vw1
    const quat q = qnorm(mat2q(Rwb));                                                           // Set_Rot: Sophus::SO3(Matrix3d)
#pragma unroll
    for (int i = 0; i < 22; i++) out22[i] = ns_child[i];
    out22[0] = (double)Pwb[0]; out22[1] = (double)Pwb[1]; out22[2] = (double)Pwb[2];
    out22[3] = V2.x; out22[4] = V2.y; out22[5] = V2.z;
    out22[6] = q.x; out22[7] = q.y; out22[8] = q.z; out22[9] = q.w;
}

// ---- the stream validator ----------------------------------------------------------------------------------------------------------------------
VIORB_HD bool ag_validate_ranges(const AgMap& M, int b, int tid, int nt) {
    bool ok = true;
    for (int i = tid; i <= b; i += nt) {
        if (!(snap_span(M.kf_start, i, i + 1, M.n_kf) && snap_span(M.pt_start, i, i + 1, M.n_pt) && snap_span(M.origin_start, i, i + 1, M.n_origin))) { ok = false; continue; }
        ok = ok && snap_span(M.child_start, M.kf_start[i], M.kf_start[i + 1], M.n_child);
    }
    return ok;
}
// the nested offsets, the slots of the child lists and of the origins, finite poses and NavStates (the GBA ones where the walk reads them
// as given: inside the adjustment), finite points, the reference key frame of every point that may be moved through it
VIORB_HD bool ag_validate_entries(const AgMap& M, const SnapStream& S, int b, int tid, int nt) {
    bool ok = S.nk <= SNAP_MAX_KF;
    ok &= snap_offsets_run(M.child_start, S.k0, S.nk, M.n_child, tid, nt);
    for (int k = tid; k < S.nk; k += nt) {
        const size_t g = (size_t)(S.k0 + k);
        ok &= mc_finite12(M.pose12 + 12 * g) && mc_finite_d(M.ns22 + 22 * g, 22);
        if (M.kf_in_gba[g]) ok &= mc_finite12(M.TcwGBA12 + 12 * g) && mc_finite_d(M.nsGBA22 + 22 * g, 22);
    }
    for (int p = tid; p < S.np; p += nt) {
        const size_t g = (size_t)(S.p0 + p);
        if (M.pt_bad[g]) continue;
        if (M.pt_in_gba[g]) { ok &= mc_finite3(M.PosGBA + 3 * g); continue; }
        ok &= mc_finite3(M.Pw + 3 * g) && M.pt_ref[g] >= 0 && M.pt_ref[g] < S.nk;
    }
    return ok;
}
VIORB_HD bool ag_validate_slots(const AgMap& M, const SnapStream& S, int b, int tid, int nt) {
    bool ok = snap_entries_within(M.child_kf, M.child_start[S.k0], M.child_start[S.k0 + S.nk], 0, S.nk, tid, nt);
    ok &= snap_entries_within(M.origin_kf, M.origin_start[b], M.origin_start[b + 1], 0, S.nk, tid, nt);
    return ok;
}
VIORB_HD void ag_tree_clear(const SnapStream& S, const AgWork& W, int tid, int nt) {
    for (int k = tid; k < S.nk; k += nt) { W.parent[S.k0 + k] = -1; W.count[S.k0 + k] = 0; W.mark[S.k0 + k] = -1; }
}
VIORB_HD void ag_tree_fill(const AgMap& M, const SnapStream& S, const AgWork& W, int b, int tid, int nt) {
    for (int k = tid; k < S.nk; k += nt)
        for (int i = M.child_start[S.k0 + k], e = M.child_start[S.k0 + k + 1]; i < e; i++) { const int c = S.k0 + M.child_kf[i]; snap_fetch_add(&W.count[c], 1); W.parent[c] = k; }
    for (int j = tid, o0 = M.origin_start[b], n = M.origin_start[b + 1] - o0; j < n; j += nt) W.mark[S.k0 + M.origin_kf[o0 + j]] = j;
}
// nobody is a child twice; an origin is listed once and is nobody's child; walking up from any key frame ends (no cycle)
VIORB_HD bool ag_tree_check(const AgMap& M, const SnapStream& S, const AgWork& W, int b, int tid, int nt) {
    bool ok = true;
    for (int j = tid, o0 = M.origin_start[b], n = M.origin_start[b + 1] - o0; j < n; j += nt) { const int o = S.k0 + M.origin_kf[o0 + j]; ok &= W.mark[o] == j && snap_ld_agent(&W.count[o]) == 0; }
    for (int k = tid; k < S.nk; k += nt) {
        ok &= snap_ld_agent(&W.count[S.k0 + k]) <= 1;
        int a = k, steps = 0;
        while (W.parent[S.k0 + a] >= 0 && steps <= S.nk) { a = W.parent[S.k0 + a]; steps++; }
        ok &= steps <= S.nk;
    }
    return ok;
}

// ---- key frame k of an accepted stream (:717-757) ------------------------------------------------------------------------------------------------
VIORB_HD void ag_key_frame(const AgMap& M, const SnapStream& S, const AgWork& W, const AgOut& R, int k) {
    const size_t g = (size_t)(S.k0 + k);
    const int32_t* parent = W.parent + S.k0;
    int root = k, run = 0;                                   // run: the steps up to the anchor
    bool anchored = M.kf_in_gba[g] != 0;
    while (parent[root] >= 0) { root = parent[root]; if (!anchored) { run++; anchored = M.kf_in_gba[S.k0 + root] != 0; } }
    const bool reached = W.mark[S.k0 + root] >= 0;
    const bool derived = reached && !M.kf_in_gba[g] && parent[k] >= 0;  // a child outside the adjustment: :732
    float T[12]; double ns[22];
#pragma unroll
    for (int i = 0; i < 12; i++) T[i] = M.TcwGBA12[12 * g + i];
#pragma unroll
    for (int i = 0; i < 22; i++) ns[i] = M.nsGBA22[22 * g + i];
    if (derived) {
        int a = k;
        for (int i = 0; i < run; i++) a = parent[a];
#pragma unroll
        for (int i = 0; i < 12; i++) T[i] = M.TcwGBA12[12 * (size_t)(S.k0 + a) + i];
        for (int d = run - 1; d >= 0; d--) {                            // down the run: the child at distance d from k, its parent at d + 1
            int c = k;
            for (int i = 0; i < d; i++) c = parent[c];
            const float* Tc = M.pose12 + 12 * (size_t)(S.k0 + c); const float* Tp = M.pose12 + 12 * (size_t)(S.k0 + parent[c]);
            float Owp[3], Rcp[9], tcp[3], Tcp[12], Tn[12];
            mc_camera_centre(Tp, Owp);
            mc_Tic(Tc, Tp, Owp, Rcp, tcp);                              // Tchildc = pChild->GetPose() * Twc (:734)
#pragma unroll
            for (int i = 0; i < 9; i++) Tcp[i] = Rcp[i];
            Tcp[9] = tcp[0]; Tcp[10] = tcp[1]; Tcp[11] = tcp[2];
            mc_mul44(Tcp, T, Tn);                                       // :735
#pragma unroll
            for (int i = 0; i < 12; i++) T[i] = Tn[i];
        }
        ag_ns_of_pose(M.ns22 + 22 * g, M.Tbc, T, ns);
    }
    R.kf_reached[g] = reached ? 1 : 0;
    R.kf_in_gba_out[g] = (M.kf_in_gba[g] || derived) ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 12; i++) { R.TcwBef_out[12 * g + i] = M.pose12[12 * g + i]; R.TcwGBA_out[12 * g + i] = T[i]; }
#pragma unroll
    for (int i = 0; i < 22; i++) { R.nsBef_out[22 * g + i] = M.ns22[22 * g + i]; R.nsGBA_out[22 * g + i] = ns[i]; R.ns22_out[22 * g + i] = reached ? ns[i] : M.ns22[22 * g + i]; }
    float Tnew[12];
    ag_pose_of_ns(ns, M.Tbc, Tnew);
#pragma unroll
    for (int i = 0; i < 12; i++) R.pose12_out[12 * g + i] = reached ? Tnew[i] : M.pose12[12 * g + i];
}
// ---- point p (:771-802) ------------------------------------------------------------------------------------------------------------------------
VIORB_HD void ag_point(const AgMap& M, const SnapStream& S, const AgOut& R, int p) {
    const size_t g = (size_t)(S.p0 + p);
    float P[3] = {M.Pw[3 * g], M.Pw[3 * g + 1], M.Pw[3 * g + 2]};
    int code = AG_BAD;
    if (!M.pt_bad[g]) {
        if (M.pt_in_gba[g]) { code = AG_POS_GBA; P[0] = M.PosGBA[3 * g]; P[1] = M.PosGBA[3 * g + 1]; P[2] = M.PosGBA[3 * g + 2]; }
        else {
            const size_t r = (size_t)(S.k0 + M.pt_ref[g]);
            code = !R.kf_in_gba_out[r] ? AG_UNTOUCHED : !R.kf_reached[r] ? AG_REF_UNREACHED : AG_BY_REF;
            if (code == AG_BY_REF) {
                const float* Tb = R.TcwBef_out + 12 * r; const float* Tn = R.pose12_out + 12 * r;
                float Xc[3], Ow[3];
#pragma unroll
                for (int i = 0; i < 3; i++) Xc[i] = (float)((double)((Tb[3 * i] * P[0] + Tb[3 * i + 1] * P[1]) + Tb[3 * i + 2] * P[2]) + (double)Tb[9 + i]);      // :794
                mc_camera_centre(Tn, Ow);                               // GetPoseInverse: Rwc = Rcw^T, twc = Ow
#pragma unroll
                for (int i = 0; i < 3; i++) P[i] = (float)((double)((Tn[i] * Xc[0] + Tn[3 + i] * Xc[1]) + Tn[6 + i] * Xc[2]) + (double)Ow[i]);                   // :801
            }
        }
    }
    R.Pw_out[3 * g] = P[0]; R.Pw_out[3 * g + 1] = P[1]; R.Pw_out[3 * g + 2] = P[2];
    R.pt_code[g] = (uint8_t)code;
}

inline void ag_run_host(const AgMap& M, const AgWork& W, const AgOut& R) {
    for (int b = 0; b < M.batch; b++) {
        bool ok = ag_validate_ranges(M, b, 0, 1);
        SnapStream S = {0, 0, 0, 0};
        if (ok) { S = snap_stream(M.kf_start, M.pt_start, b); ok = ag_validate_entries(M, S, b, 0, 1); }
        ok = ok && ag_validate_slots(M, S, b, 0, 1);
        if (ok) { ag_tree_clear(S, W, 0, 1); ag_tree_fill(M, S, W, b, 0, 1); ok = ag_tree_check(M, S, W, b, 0, 1); }
        W.info[b] = ok; R.status[b] = ok ? MC_OK : MC_INVALID;
        if (!ok) continue;
        for (int k = 0; k < S.nk; k++) ag_key_frame(M, S, W, R, k);
        for (int p = 0; p < S.np; p++) ag_point(M, S, R, p);
    }
}

} // namespace viorb
