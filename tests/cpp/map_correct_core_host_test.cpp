// tests/cpp/map_correct_core_host_test.cpp — viorb_amd/csrc/map_correct_core.h alone, compiled for the host under the address and
// undefined-behaviour sanitizers (tests/test_map_correction_host_sanitized.py): random small streams through cl_run_host (validate, claim,
// key frames, points) against the literal loop of LoopClosing::CorrectLoop written below on std::map and std::vector, bit for bit; then
// every kind of broken snapshot, each of which the validator must refuse without reading through it and without writing anything but the
// status. The arrays are exactly as long as the snapshot says, so a read or write past an end is an error of the sanitizer.
// The literal loop below is independent of the header in its order and selection logic only: the quaternion and Sim3 arithmetic
// (mat2q, qmat, sim3_mul, sim3_inv, sim3_map) is the header's own. It is no second oracle for the arithmetic: that is the numpy checker
// tests/map_correction_ref.py, which shares no code with the library. The second half does the same for the map update after a global
// bundle adjustment: ag_run_host against the literal breadth-first walk from the origins (order, flags and the matrix products written
// out here; the NavState conversions are the header's own).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <map>
#include <vector>
#include <string>
#include <algorithm>
#include "map_correct_core.h"

using namespace viorb;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 11); }
static int rint_(int n) { return n > 0 ? (int)(rnd() % (uint32_t)n) : 0; }
static double runi() { return (rnd() & 0xffffff) / (double)0x1000000; }

struct Scene {
    std::vector<int32_t> kf_start, kf_by_key, kp_start, kp_point, pt_start, obs_start, pt_ref, pt_by, cur_kf, cur_id, conn_start, conn_kf;
    std::vector<uint8_t> pt_bad; std::vector<uint32_t> obs; std::vector<float> pose12, pts_f; std::vector<double> Scw8;
};
struct Result {
    std::vector<int32_t> status, n_member, member_kf, by, cref; std::vector<float> f12, pose, Ow, pts; std::vector<double> Scw, Smeas; std::vector<uint8_t> touched;
    bool operator==(const Result& o) const {
        auto same = [](const auto& a, const auto& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0); };
        return same(status, o.status) && same(n_member, o.n_member) && same(member_kf, o.member_kf) && same(by, o.by) && same(cref, o.cref) && same(f12, o.f12) &&
               same(pose, o.pose) && same(Ow, o.Ow) && same(pts, o.pts) && same(Scw, o.Scw) && same(Smeas, o.Smeas) && same(touched, o.touched);
    }
};
static const int FILL = 77;
static Result blank(const Scene& s) {
    const size_t nb = s.cur_kf.size(), nk = s.kf_by_key.size(), np = s.pt_bad.size(), nm = s.conn_kf.size() + nb;
    Result r;
    r.status.assign(nb, FILL); r.n_member.assign(nb, FILL); r.member_kf.assign(nm, FILL); r.by.assign(np, FILL); r.cref.assign(np, FILL); r.f12.assign(nm * 12, FILL);
    r.pose.assign(nk * 12, FILL); r.Ow.assign(nk * 3, FILL); r.pts.assign(np * 8, FILL); r.Scw.assign(nk * 8, FILL); r.Smeas.assign(nk * 8, FILL); r.touched.assign(np, FILL);
    return r;
}
static float g_sf[16];
static const int NLEVELS = 8;

static Result run_core(const Scene& s) {
    Result r = blank(s);
    ClMap M;
    M.batch = (int)s.cur_kf.size(); M.n_kf = (int)s.kf_by_key.size(); M.n_kp = (int)s.kp_point.size(); M.n_pt = (int)s.pt_bad.size(); M.n_obs = (int)s.obs.size(); M.n_conn = (int)s.conn_kf.size();
    M.kf_start = s.kf_start.data(); M.kf_by_key = s.kf_by_key.data(); M.kp_start = s.kp_start.data(); M.kp_point = s.kp_point.data(); M.pt_start = s.pt_start.data();
    M.pt_bad = s.pt_bad.data(); M.obs_start = s.obs_start.data(); M.obs = s.obs.data(); M.pose12 = s.pose12.data(); M.pts_f = s.pts_f.data(); M.pt_ref = s.pt_ref.data();
    M.pt_corrected_by = s.pt_by.data(); M.cur_kf = s.cur_kf.data(); M.cur_id = s.cur_id.data(); M.Scw8 = s.Scw8.data(); M.conn_start = s.conn_start.data(); M.conn_kf = s.conn_kf.data();
    for (int i = 0; i < 16; i++) M.sf[i] = g_sf[i < NLEVELS ? i : NLEVELS - 1];
    M.nlevels = NLEVELS;
    std::vector<int32_t> key(M.n_kf, -5), memb(M.n_kf, -5), claim(M.n_pt, -5), terms((size_t)M.n_obs * 3, -5), info(M.batch, -5);       // dirty on entry
    std::vector<float> Ow((size_t)M.n_kf * 3, -5.f); std::vector<double> Swi((size_t)M.n_kf * 8, -5.);
    ClWork W; W.key = key.data(); W.memb = memb.data(); W.claim = claim.data(); W.Ow_in = Ow.data(); W.Swi = Swi.data(); W.terms = terms.data(); W.info = info.data();
    ClOut R; R.status = r.status.data(); R.n_member = r.n_member.data(); R.member_kf = r.member_kf.data(); R.Scw_f12 = r.f12.data(); R.Scw_out = r.Scw.data(); R.Smeas_out = r.Smeas.data();
    R.pose12_out = r.pose.data(); R.Ow_out = r.Ow.data(); R.pts_f_out = r.pts.data(); R.pt_corrected_by_out = r.by.data(); R.pt_corrected_ref_out = r.cref.data(); R.pt_touched = r.touched.data();
    cl_run_host(M, W, R);
    return r;
}

// ---- the literal loop (src/LoopClosing.cc:460-542) on a good snapshot -------------------------------------------------------------------------
static std::map<std::string, long> g_seen;
static void centre(const float* T, float* Ow) { for (int r = 0; r < 3; r++) Ow[r] = ((-T[r]) * T[9] + (-T[3 + r]) * T[10]) + (-T[6 + r]) * T[11]; }
static sim3d of_pose(const float* R, const float* t) {
    sim3d o; o.r = mat2q(mkm(R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8])); o.t = mk3(t[0], t[1], t[2]); o.s = 1.0; return o;
}
static void literal_stream(const Scene& s, int b, Result& r) {
    const int k0 = s.kf_start[b], nk = s.kf_start[b + 1] - k0, p0 = s.pt_start[b], np = s.pt_start[b + 1] - p0, cur = s.cur_kf[b], cur_id = s.cur_id[b];
    std::vector<int> rank(nk);
    for (int j = 0; j < nk; j++) rank[s.kf_by_key[k0 + j]] = j;
    std::vector<float> Tcw(s.pose12.begin() + 12 * (size_t)k0, s.pose12.begin() + 12 * (size_t)(k0 + nk)), Ow(3 * (size_t)nk), P(s.pts_f.begin() + 8 * (size_t)p0, s.pts_f.begin() + 8 * (size_t)(p0 + np));
    for (int k = 0; k < nk; k++) centre(&Tcw[12 * k], &Ow[3 * k]);
    std::vector<int> connected(s.conn_kf.begin() + s.conn_start[b], s.conn_kf.begin() + s.conn_start[b + 1]);
    connected.push_back(cur);
    std::map<int, sim3d> Corrected, NonCorrected;                           // keyed by key position: the iteration order of std::map<KeyFrame*, ...>
    const sim3d Scw = sim3_ld(&s.Scw8[8 * (size_t)b]);
    Corrected[rank[cur]] = Scw;
    float Twc[16];                                                      // GetPoseInverse
    for (int r_ = 0; r_ < 3; r_++) { for (int c = 0; c < 3; c++) Twc[4 * r_ + c] = Tcw[12 * cur + 3 * c + r_]; Twc[4 * r_ + 3] = Ow[3 * cur + r_]; }
    Twc[12] = Twc[13] = Twc[14] = 0.f; Twc[15] = 1.f;
    for (int i : connected) {
        float Tiw[16];
        for (int r_ = 0; r_ < 3; r_++) { for (int c = 0; c < 3; c++) Tiw[4 * r_ + c] = Tcw[12 * i + 3 * r_ + c]; Tiw[4 * r_ + 3] = Tcw[12 * i + 9 + r_]; }
        Tiw[12] = Tiw[13] = Tiw[14] = 0.f; Tiw[15] = 1.f;
        if (i != cur) {
            float Tic[16];
            for (int r_ = 0; r_ < 4; r_++) for (int c = 0; c < 4; c++) Tic[4 * r_ + c] = ((Tiw[4 * r_] * Twc[c] + Tiw[4 * r_ + 1] * Twc[4 + c]) + Tiw[4 * r_ + 2] * Twc[8 + c]) + Tiw[4 * r_ + 3] * Twc[12 + c];
            const float Ric[9] = {Tic[0], Tic[1], Tic[2], Tic[4], Tic[5], Tic[6], Tic[8], Tic[9], Tic[10]}, tic[3] = {Tic[3], Tic[7], Tic[11]};
            Corrected[rank[i]] = sim3_mul(of_pose(Ric, tic), Scw);
        }
        NonCorrected[rank[i]] = of_pose(&Tcw[12 * i], &Tcw[12 * i + 9]);
    }
    std::vector<int> by(s.pt_by.begin() + p0, s.pt_by.begin() + p0 + np), cref(np, -1), touched(np, 0);
    std::vector<float> pose_out = Tcw;
    int at = 0;
    const int m0 = s.conn_start[b] + b;
    for (auto& kv : Corrected) {
        const int i = s.kf_by_key[k0 + kv.first];
        const sim3d Siw_c = kv.second, Swi_c = sim3_inv(Siw_c), Siw = NonCorrected[kv.first];
        for (int x = s.kp_start[k0 + i]; x < s.kp_start[k0 + i + 1]; x++) {
            const int p = s.kp_point[x];
            if (p < 0) { g_seen["null-keypoint"]++; continue; }
            if (s.pt_bad[p0 + p]) { g_seen["bad-point"]++; continue; }
            for (int y = s.kp_start[k0 + i]; y < x; y++) if (s.kp_point[y] == p) { g_seen["twice-in-member"]++; break; }
            if (by[p] == cur_id) { if (touched[p] && cref[p] != i) g_seen["two-members"]++; else if (!touched[p]) g_seen["already-corrected"]++; continue; }
            const d3 q = sim3_map(Swi_c, sim3_map(Siw, mk3(P[8 * p], P[8 * p + 1], P[8 * p + 2])));
            P[8 * p] = (float)q.x; P[8 * p + 1] = (float)q.y; P[8 * p + 2] = (float)q.z;
            by[p] = cur_id; cref[p] = i; touched[p] = 1;
            // UpdateNormalAndDepth on the state as it stands
            std::multimap<int, uint32_t> observations;
            for (int o = s.obs_start[p0 + p]; o < s.obs_start[p0 + p + 1]; o++) observations.insert({rank[s.obs[o] & 0xffff], s.obs[o]});
            if (observations.empty()) { g_seen["no-observations"]++; continue; }
            float normal[3] = {0.f, 0.f, 0.f};
            int n = 0;
            for (auto& ow : observations) {
                const int k = (int)(ow.second & 0xffff);
                const float d[3] = {P[8 * p] - Ow[3 * k], P[8 * p + 1] - Ow[3 * k + 1], P[8 * p + 2] - Ow[3 * k + 2]};
                const double nrm = std::sqrt(((double)d[0] * d[0] + (double)d[1] * d[1]) + (double)d[2] * d[2]);
                for (int c = 0; c < 3; c++) normal[c] = normal[c] + (float)((double)d[c] / nrm);
                n++;
                const bool member = Corrected.count(ow.first) != 0;
                g_seen[!member ? "observer-not-member" : ow.first < kv.first ? "observer-below" : ow.first == kv.first ? "observer-equal" : "observer-above"]++;
            }
            const int ref = s.pt_ref[p0 + p];
            g_seen[Corrected.count(rank[ref]) && rank[ref] < kv.first ? "ref-below" : "ref-not-below"]++;
            const float d[3] = {P[8 * p] - Ow[3 * ref], P[8 * p + 1] - Ow[3 * ref + 1], P[8 * p + 2] - Ow[3 * ref + 2]};
            const float dist = (float)std::sqrt(((double)d[0] * d[0] + (double)d[1] * d[1]) + (double)d[2] * d[2]);
            int level = 0;
            for (int o = s.obs_start[p0 + p + 1] - 1; o >= s.obs_start[p0 + p]; o--) if ((int)(s.obs[o] & 0xffff) == ref) level = (int)((s.obs[o] >> 16) & 0xff);
            P[8 * p + 7] = dist * g_sf[level]; P[8 * p + 6] = P[8 * p + 7] / g_sf[NLEVELS - 1];
            for (int c = 0; c < 3; c++) P[8 * p + 3 + c] = (float)((double)normal[c] / (double)n);
        }
        double R9[9];
        stm(R9, qmat(Siw_c.r));
        const d3 t = Siw_c.t * (1. / Siw_c.s);
        for (int c = 0; c < 9; c++) pose_out[12 * i + c] = (float)R9[c];
        pose_out[12 * i + 9] = (float)t.x; pose_out[12 * i + 10] = (float)t.y; pose_out[12 * i + 11] = (float)t.z;
        centre(&pose_out[12 * i], &Ow[3 * i]);                           // SetPose
        r.member_kf[m0 + at] = i;
        stm(R9, scl(qmat(Siw_c.r), Siw_c.s));
        for (int r_ = 0; r_ < 3; r_++) for (int c = 0; c < 3; c++) r.f12[12 * (size_t)(m0 + at) + 4 * r_ + c] = (float)R9[3 * r_ + c];
        r.f12[12 * (size_t)(m0 + at) + 3] = (float)Siw_c.t.x; r.f12[12 * (size_t)(m0 + at) + 7] = (float)Siw_c.t.y; r.f12[12 * (size_t)(m0 + at) + 11] = (float)Siw_c.t.z;
        at++;
        if (Siw_c.s != 1.0) g_seen["scale-not-1"]++;
    }
    r.status[b] = MC_OK; r.n_member[b] = at;
    for (int k = 0; k < nk; k++) {
        const sim3d Sm = of_pose(&Tcw[12 * k], &Tcw[12 * k + 9]);
        sim3_st(&r.Smeas[8 * (size_t)(k0 + k)], Sm);
        sim3_st(&r.Scw[8 * (size_t)(k0 + k)], Corrected.count(rank[k]) ? Corrected[rank[k]] : Sm);
        for (int c = 0; c < 12; c++) r.pose[12 * (size_t)(k0 + k) + c] = pose_out[12 * k + c];
        for (int c = 0; c < 3; c++) r.Ow[3 * (size_t)(k0 + k) + c] = Ow[3 * k + c];
    }
    for (int p = 0; p < np; p++) {
        for (int c = 0; c < 8; c++) r.pts[8 * (size_t)(p0 + p) + c] = P[8 * p + c];
        r.by[p0 + p] = by[p]; r.cref[p0 + p] = cref[p]; r.touched[p0 + p] = (uint8_t)touched[p];
    }
    if (connected.size() == 1) g_seen["empty-list"]++;
    if (np == 0) g_seen["no-points"]++;
}

// ---- random streams ---------------------------------------------------------------------------------------------------------------------------
static void add_stream(Scene& s) {
    const int nk = 1 + rint_(9), np = rint_(14), k0 = (int)s.kf_by_key.size(), p0 = (int)s.pt_bad.size(), cur = rint_(nk);
    std::vector<int> perm(nk);
    for (int k = 0; k < nk; k++) perm[k] = k;
    for (int k = nk - 1; k > 0; k--) std::swap(perm[k], perm[rint_(k + 1)]);
    for (int k = 0; k < nk; k++) s.kf_by_key.push_back(perm[k]);
    for (int k = nk - 1; k > 0; k--) std::swap(perm[k], perm[rint_(k + 1)]);
    int n_conn = rint_(nk);
    for (int k = 0; k < nk && n_conn > 0; k++) if (perm[k] != cur) { s.conn_kf.push_back(perm[k]); n_conn--; }
    s.conn_start.push_back((int)s.conn_kf.size());
    s.cur_kf.push_back(cur); s.cur_id.push_back(7);
    for (int p = 0; p < np; p++) {
        const int n = rint_(10) == 0 ? 0 : rint_(std::min(nk, 5) + 1);
        std::vector<int> ks(nk);
        for (int k = 0; k < nk; k++) ks[k] = k;
        for (int k = nk - 1; k > 0; k--) std::swap(ks[k], ks[rint_(k + 1)]);
        for (int i = 0; i < n; i++) s.obs.push_back((uint32_t)ks[i] | ((uint32_t)rint_(8) << 16) | ((uint32_t)rint_(2) << 24));
        s.obs_start.push_back((int)s.obs.size());
        s.pt_ref.push_back(n ? ks[rint_(n)] : -1); s.pt_bad.push_back(rint_(10) == 0); s.pt_by.push_back(rint_(10) == 0 ? 7 : rint_(5));
        for (int c = 0; c < 8; c++) s.pts_f.push_back((float)(runi() * 8 - 4));
    }
    for (int k = 0; k < nk; k++) {
        const int m = np ? rint_(9) : rint_(3);
        for (int i = 0; i < m; i++) s.kp_point.push_back(np && rint_(6) ? rint_(np) : -1);
        s.kp_start.push_back((int)s.kp_point.size());
        // a rotation about a random axis by a small angle or close to a half turn: the four branches of the quaternion conversion
        double w[3] = {runi() - 0.5, runi() - 0.5, runi() - 0.5};
        const int kind = rint_(6);
        if (kind >= 1 && kind <= 3) w[kind - 1] += 3.14159265358979;
        const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), a = std::sin(th) / th, c2 = (1 - std::cos(th)) / (th * th);
        const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
        for (int r_ = 0; r_ < 3; r_++) for (int c = 0; c < 3; c++) {
            double kk = 0;
            for (int j = 0; j < 3; j++) kk += K[3 * r_ + j] * K[3 * j + c];
            s.pose12.push_back((float)((r_ == c) + a * K[3 * r_ + c] + c2 * kk));
        }
        for (int c = 0; c < 3; c++) s.pose12.push_back((float)(runi() * 6 - 3));
    }
    double q[4] = {runi() - 0.5, runi() - 0.5, runi() - 0.5, runi() + 0.1};
    const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int c = 0; c < 4; c++) s.Scw8.push_back(q[c] / qn);
    for (int c = 0; c < 3; c++) s.Scw8.push_back(runi() * 4 - 2);
    s.Scw8.push_back(rint_(3) ? 0.5 + runi() * 1.5 : 1.0);
    s.kf_start.push_back(k0 + nk); s.pt_start.push_back(p0 + np);
}
static Scene make_batch(int streams) {
    Scene s;
    s.kf_start.push_back(0); s.pt_start.push_back(0); s.conn_start.push_back(0); s.kp_start.push_back(0); s.obs_start.push_back(0);
    for (int b = 0; b < streams; b++) add_stream(s);
    return s;
}
static void count_branches(const Scene& s) {
    for (size_t k = 0; k < s.kf_by_key.size(); k++) {
        const float* R = &s.pose12[12 * k];
        const double t = (double)R[0] + R[4] + R[8];
        g_seen[t > 0 ? "mat2q-trace" : (R[0] >= R[4] && R[0] >= R[8]) ? "mat2q-x" : (R[4] > R[0] && R[4] >= R[8]) ? "mat2q-y" : "mat2q-z"]++;
    }
}

// ---- the map update after a global bundle adjustment: ag_run_host against the literal breadth-first walk ------------------------------------
struct GbaScene {
    std::vector<int32_t> kf_start, child_start, child_kf, origin_start, origin_kf, pt_start, pt_ref;
    std::vector<uint8_t> in_gba, pt_bad, pt_in; std::vector<float> pose, gba, Pw, PosGBA; std::vector<double> ns, nsg;
};
struct GbaResult {
    std::vector<int32_t> status; std::vector<float> pose, bef, gba, Pw; std::vector<double> ns, nsbef, nsg; std::vector<uint8_t> flag, reached, code;
    bool operator==(const GbaResult& o) const {
        auto same = [](const auto& a, const auto& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0); };
        return same(status, o.status) && same(pose, o.pose) && same(bef, o.bef) && same(gba, o.gba) && same(Pw, o.Pw) && same(ns, o.ns) && same(nsbef, o.nsbef) && same(nsg, o.nsg) &&
               same(flag, o.flag) && same(reached, o.reached) && same(code, o.code);
    }
};
static const float g_Tbc[12] = {0.0148655f, -0.999881f, 0.0041403f, 0.999557f, 0.0149672f, 0.0257155f, -0.0257744f, 0.0037562f, 0.999661f, -0.0216401f, -0.064677f, 0.0098107f};
static GbaResult gba_blank(const GbaScene& s) {
    const size_t nb = s.kf_start.size() - 1, nk = s.in_gba.size(), np = s.pt_bad.size();
    GbaResult r;
    r.status.assign(nb, FILL); r.pose.assign(nk * 12, FILL); r.bef.assign(nk * 12, FILL); r.gba.assign(nk * 12, FILL); r.Pw.assign(np * 3, FILL); r.ns.assign(nk * 22, FILL);
    r.nsbef.assign(nk * 22, FILL); r.nsg.assign(nk * 22, FILL); r.flag.assign(nk, FILL); r.reached.assign(nk, FILL); r.code.assign(np, FILL);
    return r;
}
static GbaResult gba_core(const GbaScene& s) {
    GbaResult r = gba_blank(s);
    AgMap M;
    M.batch = (int)s.kf_start.size() - 1; M.n_kf = (int)s.in_gba.size(); M.n_child = (int)s.child_kf.size(); M.n_origin = (int)s.origin_kf.size(); M.n_pt = (int)s.pt_bad.size();
    M.kf_start = s.kf_start.data(); M.child_start = s.child_start.data(); M.child_kf = s.child_kf.data(); M.origin_start = s.origin_start.data(); M.origin_kf = s.origin_kf.data();
    M.kf_in_gba = s.in_gba.data(); M.pose12 = s.pose.data(); M.TcwGBA12 = s.gba.data(); M.ns22 = s.ns.data(); M.nsGBA22 = s.nsg.data(); M.pt_start = s.pt_start.data();
    M.pt_bad = s.pt_bad.data(); M.pt_in_gba = s.pt_in.data(); M.Pw = s.Pw.data(); M.PosGBA = s.PosGBA.data(); M.pt_ref = s.pt_ref.data();
    for (int i = 0; i < 12; i++) M.Tbc[i] = g_Tbc[i];
    std::vector<int32_t> parent(M.n_kf, -5), count(M.n_kf, -5), mark(M.n_kf, -5), info(M.batch, -5);                                   // dirty on entry
    AgWork W; W.parent = parent.data(); W.count = count.data(); W.mark = mark.data(); W.info = info.data();
    AgOut R; R.status = r.status.data(); R.pose12_out = r.pose.data(); R.ns22_out = r.ns.data(); R.TcwBef_out = r.bef.data(); R.nsBef_out = r.nsbef.data(); R.TcwGBA_out = r.gba.data();
    R.nsGBA_out = r.nsg.data(); R.kf_in_gba_out = r.flag.data(); R.kf_reached = r.reached.data(); R.Pw_out = r.Pw.data(); R.pt_code = r.code.data();
    ag_run_host(M, W, R);
    return r;
}
static void mul44(const float* A, const float* B, float* C) {          // 4 x 4 with the last rows written out
    float a[16], b[16];
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) { a[4 * r + c] = A[3 * r + c]; b[4 * r + c] = B[3 * r + c]; } a[4 * r + 3] = A[9 + r]; b[4 * r + 3] = B[9 + r]; }
    for (int c = 0; c < 4; c++) { a[12 + c] = b[12 + c] = c == 3 ? 1.f : 0.f; }
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) {
        const float v = ((a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c]) + a[4 * r + 2] * b[8 + c]) + a[4 * r + 3] * b[12 + c];
        if (c < 3) C[3 * r + c] = v; else C[9 + r] = v;
    }
}
static void inverse_pose(const float* T, float* I) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) I[3 * r + c] = T[3 * c + r]; centre(T, I + 9); }
// the literal walk (src/LoopClosing.cc:713-803) of one stream; the NavState arithmetic (ag_ns_of_pose, ag_pose_of_ns) is the header's own
static void gba_literal(const GbaScene& s, int b, GbaResult& r) {
    const int k0 = s.kf_start[b], nk = s.kf_start[b + 1] - k0, p0 = s.pt_start[b], np = s.pt_start[b + 1] - p0;
    std::vector<float> Tcw(s.pose.begin() + 12 * (size_t)k0, s.pose.begin() + 12 * (size_t)(k0 + nk)), G(s.gba.begin() + 12 * (size_t)k0, s.gba.begin() + 12 * (size_t)(k0 + nk)), Bef = Tcw;
    std::vector<double> ns(s.ns.begin() + 22 * (size_t)k0, s.ns.begin() + 22 * (size_t)(k0 + nk)), nsg(s.nsg.begin() + 22 * (size_t)k0, s.nsg.begin() + 22 * (size_t)(k0 + nk)), nsbef = ns;
    std::vector<int> flag(nk), reached(nk, 0), depth(nk, 0);
    for (int k = 0; k < nk; k++) flag[k] = s.in_gba[k0 + k];
    std::vector<int> queue(s.origin_kf.begin() + s.origin_start[b], s.origin_kf.begin() + s.origin_start[b + 1]);
    if (queue.size() >= 2) g_seen["two-origins"]++;
    for (size_t head = 0; head < queue.size(); head++) {
        const int k = queue[head];
        float Twc[12];
        inverse_pose(&Tcw[12 * k], Twc);
        if (!flag[k]) g_seen["root-outside"]++;
        int outside = 0;
        for (int i = s.child_start[k0 + k]; i < s.child_start[k0 + k + 1]; i++) {
            const int c = s.child_kf[i];
            if (!flag[c]) {
                float Tcc[12];
                mul44(&Tcw[12 * c], Twc, Tcc);
                mul44(Tcc, &G[12 * k], &G[12 * c]);
                flag[c] = 1; depth[c] = depth[k] + 1; outside++;
                if (depth[c] == 3) g_seen["chain-of-three-outside"]++;
                ag_ns_of_pose(&ns[22 * c], g_Tbc, &G[12 * c], &nsg[22 * c]);
            }
            queue.push_back(c);
        }
        if (outside >= 2) g_seen["siblings"]++;
        for (int i = 0; i < 22; i++) ns[22 * k + i] = nsg[22 * k + i];
        ag_pose_of_ns(&ns[22 * k], g_Tbc, &Tcw[12 * k]);
        reached[k] = 1;
    }
    for (int k = 0; k < nk; k++) {
        const size_t g = (size_t)(k0 + k);
        if (!reached[k]) g_seen["unreached-kf"]++;
        for (int i = 0; i < 12; i++) { r.pose[12 * g + i] = Tcw[12 * k + i]; r.bef[12 * g + i] = Bef[12 * k + i]; r.gba[12 * g + i] = G[12 * k + i]; }
        for (int i = 0; i < 22; i++) { r.ns[22 * g + i] = ns[22 * k + i]; r.nsbef[22 * g + i] = nsbef[22 * k + i]; r.nsg[22 * g + i] = nsg[22 * k + i]; }
        r.flag[g] = (uint8_t)flag[k]; r.reached[g] = (uint8_t)reached[k];
    }
    for (int p = 0; p < np; p++) {
        const size_t g = (size_t)(p0 + p);
        float P[3] = {s.Pw[3 * g], s.Pw[3 * g + 1], s.Pw[3 * g + 2]};
        int code = AG_BAD;
        if (!s.pt_bad[g]) {
            if (s.pt_in[g]) { code = AG_POS_GBA; for (int i = 0; i < 3; i++) P[i] = s.PosGBA[3 * g + i]; }
            else {
                const int ref = s.pt_ref[g];
                if (!flag[ref]) code = AG_UNTOUCHED;
                else if (!reached[ref]) code = AG_REF_UNREACHED;
                else {
                    code = AG_BY_REF;
                    const float* Tb = &Bef[12 * ref];
                    float Xc[3], Twc[12];
                    for (int i = 0; i < 3; i++) Xc[i] = (float)((double)((Tb[3 * i] * P[0] + Tb[3 * i + 1] * P[1]) + Tb[3 * i + 2] * P[2]) + (double)Tb[9 + i]);
                    inverse_pose(&Tcw[12 * ref], Twc);
                    for (int i = 0; i < 3; i++) P[i] = (float)((double)((Twc[3 * i] * Xc[0] + Twc[3 * i + 1] * Xc[1]) + Twc[3 * i + 2] * Xc[2]) + (double)Twc[9 + i]);
                }
            }
        }
        g_seen[std::string("code-") + (char)('0' + code)]++;
        for (int i = 0; i < 3; i++) r.Pw[3 * g + i] = P[i];
        r.code[g] = (uint8_t)code;
    }
    r.status[b] = MC_OK;
}
static void gba_add_stream(GbaScene& s) {
    const int nk = 1 + rint_(12), np = rint_(16), k0 = (int)s.in_gba.size();
    std::vector<int> order(nk), roots;
    for (int k = 0; k < nk; k++) order[k] = k;
    for (int k = nk - 1; k > 0; k--) std::swap(order[k], order[rint_(k + 1)]);
    std::vector<std::vector<int> > children(nk);
    for (int j = 0; j < nk; j++) {
        if (j == 0 || rint_(7) == 0) roots.push_back(order[j]);
        else children[order[std::max(0, j - 1 - rint_(3))]].push_back(order[j]);
    }
    for (int k = 0; k < nk; k++) { for (int c : children[k]) s.child_kf.push_back(c); s.child_start.push_back((int)s.child_kf.size()); }
    int n_or = 0;
    for (int rt : roots) if (rint_(3) || (n_or == 0 && rt == roots.back())) { s.origin_kf.push_back(rt); n_or++; }
    s.origin_start.push_back((int)s.origin_kf.size());
    for (int k = 0; k < nk; k++) {
        s.in_gba.push_back(rint_(5) < 3);
        for (int which = 0; which < 2; which++) {
            std::vector<float>& T = which ? s.gba : s.pose;
            double w[3] = {runi() - 0.5, runi() - 0.5, runi() - 0.5};
            const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), a = std::sin(th) / th, c2 = (1 - std::cos(th)) / (th * th);
            const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
            for (int r_ = 0; r_ < 3; r_++) for (int c = 0; c < 3; c++) { double kk = 0; for (int j = 0; j < 3; j++) kk += K[3 * r_ + j] * K[3 * j + c]; T.push_back((float)((r_ == c) + a * K[3 * r_ + c] + c2 * kk)); }
            for (int c = 0; c < 3; c++) T.push_back((float)(runi() * 6 - 3));
            std::vector<double>& N = which ? s.nsg : s.ns;
            double q[4] = {runi() - 0.5, runi() - 0.5, runi() - 0.5, runi() - 0.5};
            const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            for (int c = 0; c < 6; c++) N.push_back(runi() * 4 - 2);
            for (int c = 0; c < 4; c++) N.push_back(q[c] / qn);
            for (int c = 0; c < 12; c++) N.push_back(runi() * 0.02 - 0.01);
        }
    }
    for (int p = 0; p < np; p++) {
        s.pt_bad.push_back(rint_(7) == 0); s.pt_in.push_back(rint_(5) < 2); s.pt_ref.push_back(rint_(nk));
        for (int c = 0; c < 3; c++) { s.Pw.push_back((float)(runi() * 8 - 4)); s.PosGBA.push_back((float)(runi() * 8 - 4)); }
    }
    s.kf_start.push_back(k0 + nk); s.pt_start.push_back((int)s.pt_bad.size());
}
static bool gba_rounds(uint64_t& checksum, long& maps, long& refused) {
    for (int round = 0; round < 600; round++) {
        GbaScene s;
        s.kf_start.push_back(0); s.pt_start.push_back(0); s.origin_start.push_back(0); s.child_start.push_back(0);
        const int nb = 1 + rint_(4);
        for (int b = 0; b < nb; b++) gba_add_stream(s);
        GbaResult want = gba_blank(s);
        for (int b = 0; b < nb; b++) gba_literal(s, b, want);
        const GbaResult got = gba_core(s);
        if (!(got == want)) { printf("map round %d: the core differs from the literal walk\n", round); return false; }
        for (float v : got.Pw) { uint32_t u; memcpy(&u, &v, 4); checksum = checksum * 1099511628211ull + u; }
        maps += nb;
        GbaScene bad = s;
        const int b = rint_(nb), k0 = s.kf_start[b], nk = s.kf_start[b + 1] - k0, p0 = s.pt_start[b], np = s.pt_start[b + 1] - p0, c0 = s.child_start[k0], nc = s.child_start[k0 + nk] - c0,
                  o0 = s.origin_start[b], no = s.origin_start[b + 1] - o0;
        switch (round % 8) {
            case 0: if (!nc) continue; bad.child_kf[c0 + rint_(nc)] = rint_(2) ? nk + rint_(1 << 20) : -1 - rint_(1 << 20); break;
            case 1: if (nc < 2) continue; bad.child_kf[c0] = bad.child_kf[c0 + 1]; break;                                       // a child twice
            case 2: { int k = -1; for (int x = 0; x < nk && k < 0; x++) if (s.child_start[k0 + x + 1] > s.child_start[k0 + x]) k = x; if (k < 0) continue; bad.child_kf[s.child_start[k0 + k]] = k; break; }   // its own child
            case 3: bad.origin_kf[o0 + rint_(no)] = rint_(2) ? nk + rint_(1 << 20) : -1 - rint_(1 << 20); break;
            case 4: if (!nc) continue; bad.origin_kf[o0] = s.child_kf[c0]; break;                                              // an origin that is a child
            case 5: bad.pose[12 * (size_t)(k0 + rint_(nk)) + rint_(12)] = NAN; break;
            case 6: bad.ns[22 * (size_t)(k0 + rint_(nk)) + rint_(22)] = INFINITY; break;
            default: { int p = -1; for (int x = 0; x < np && p < 0; x++) if (!s.pt_bad[p0 + x] && !s.pt_in[p0 + x]) p = p0 + x; if (p < 0) continue; bad.pt_ref[p] = rint_(2) ? nk + rint_(1 << 28) : -1 - rint_(1 << 28); }
        }
        GbaResult want_bad = gba_blank(s);
        for (int x = 0; x < nb; x++) if (x != b) gba_literal(s, x, want_bad);
        want_bad.status[b] = MC_INVALID;
        if (!(gba_core(bad) == want_bad)) { printf("map round %d (kind %d): a broken map was not refused alone\n", round, round % 8); return false; }
        refused++;
    }
    return true;
}

int main() {
    g_sf[0] = 1.0f;
    for (int i = 1; i < 16; i++) g_sf[i] = g_sf[i - 1] * 1.2f;
    long streams = 0, refused = 0;
    uint64_t checksum = 0;
    for (int round = 0; round < 800; round++) {
        const Scene s = make_batch(1 + rint_(4));
        const int nb = (int)s.cur_kf.size();
        count_branches(s);
        // a point's reference key frame is always among its observers and every index is in range: a good snapshot
        Result want = blank(s);
        for (int b = 0; b < nb; b++) literal_stream(s, b, want);
        const Result got = run_core(s);
        if (!(got == want)) { printf("round %d: the core differs from the literal loop\n", round); return 1; }
        for (float v : got.pts) { uint32_t u; memcpy(&u, &v, 4); checksum = checksum * 1099511628211ull + u; }
        streams += nb;
        // one broken stream in the batch: it alone is refused and writes nothing but its status
        Scene bad = s;
        const int b = rint_(nb), k0 = s.kf_start[b], nk = s.kf_start[b + 1] - k0, p0 = s.pt_start[b], np = s.pt_start[b + 1] - p0, c0 = s.conn_start[b], nc = s.conn_start[b + 1] - c0;
        switch (round % 12) {
            case 0: bad.kf_by_key[k0 + rint_(nk)] = nk + rint_(1 << 20); break;
            case 1: bad.kf_by_key[k0 + rint_(nk)] = -1 - rint_(1 << 20); break;
            case 2: if (nk < 2) continue; bad.kf_by_key[k0] = bad.kf_by_key[k0 + 1]; break;
            case 3: bad.cur_kf[b] = rint_(2) ? nk + rint_(1 << 20) : -1 - rint_(1 << 20); break;
            case 4: if (!nc) continue; bad.conn_kf[c0 + rint_(nc)] = rint_(2) ? nk + rint_(1 << 20) : -1 - rint_(1 << 20); break;
            case 5: if (!nc) continue; bad.conn_kf[c0 + rint_(nc)] = s.cur_kf[b]; break;
            case 6: if (nc < 2) continue; bad.conn_kf[c0] = bad.conn_kf[c0 + 1]; break;
            case 7: bad.pose12[12 * (size_t)(k0 + rint_(nk)) + rint_(12)] = rint_(2) ? INFINITY : NAN; break;
            case 8: bad.Scw8[8 * (size_t)b + 7] = rint_(2) ? 0.0 : -1.0; break;
            case 9: { if (!np) continue; const int p = p0 + rint_(np); if (s.obs_start[p] == s.obs_start[p + 1]) continue; bad.obs[s.obs_start[p]] = (uint32_t)(nk + rint_(60000 - nk)) | (5u << 16); break; }
            case 10: {                                                  // a member's keypoint far outside the points
                int i = -1;
                for (int j = 0; j <= nc && i < 0; j++) { const int k = j < nc ? s.conn_kf[c0 + j] : s.cur_kf[b]; if (s.kp_start[k0 + k + 1] > s.kp_start[k0 + k]) i = s.kp_start[k0 + k]; }
                if (i < 0) continue;
                bad.kp_point[i] = rint_(2) ? np + rint_(1 << 28) : -2 - rint_(1 << 28);
                break;
            }
            default: {                                                  // the reference key frame of a corrected, observed point: out of range or not an observer
                int p = -1;
                for (int x = 0; x < np && p < 0; x++) if (want.touched[p0 + x] && s.obs_start[p0 + x + 1] > s.obs_start[p0 + x]) p = p0 + x;
                if (p < 0) continue;
                int other = -1;
                for (int k = 0; k < nk && other < 0; k++) { bool obs = false; for (int o = s.obs_start[p]; o < s.obs_start[p + 1]; o++) obs |= (int)(s.obs[o] & 0xffff) == k; if (!obs) other = k; }
                bad.pt_ref[p] = (other >= 0 && rint_(2)) ? other : (rint_(2) ? nk + rint_(1 << 28) : -1 - rint_(1 << 28));
            }
        }
        Result want_bad = blank(s);
        for (int x = 0; x < nb; x++) if (x != b) literal_stream(s, x, want_bad);
        want_bad.status[b] = MC_INVALID;
        if (!(run_core(bad) == want_bad)) { printf("round %d (kind %d): a broken stream was not refused alone\n", round, round % 12); return 1; }
        refused++;
    }
    long maps = 0, maps_refused = 0;
    if (!gba_rounds(checksum, maps, maps_refused)) return 1;
    printf("checksum %016llx\nstreams %ld refused %ld maps %ld maps-refused %ld", (unsigned long long)checksum, streams, refused, maps, maps_refused);
    for (auto& kv : g_seen) printf(" %s %ld", kv.first.c_str(), kv.second);
    printf("\n");
    return 0;
}
