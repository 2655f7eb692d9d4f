// tests/cpp/map_fusion_core_host_test.cpp — the host build of viorb_amd/csrc/map_fusion_core.h as a stand-alone program. No GPU, no library:
// only the header.
//   map_fusion_core_host_test FILE [FILE ...]   the program that tests/test_map_fusion_host_sanitized.py compiles with
//                                               -fsanitize=address,undefined and runs as a child process. Every FILE is a packed snapshot
//                                               that viorb_amd/snapshot.py's write_snapshot leaves: the 10 totals as int32, then the
//                                               arrays of viorb_fuse_map in their order, each exactly as long as its total says, so that
//                                               the address sanitizer sees any read or write past an end. fuse_run_host runs on it with
//                                               a workspace and result arrays of exactly the totals, filled with 77 beforehand. One line
//                                               per file: a checksum over every result array in the order of viorb_fuse_result (status
//                                               last), which the Python side compares with the checker's, and the status of every stream.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "map_fusion_core.h"

using namespace viorb;

static void fail(const char* what) { std::printf("FAILED: %s\n", what); std::exit(2); }

struct Reader {
    FILE* f;
    template <class T> std::vector<T> take(size_t n) {
        std::vector<T> v(n);
        if (n && std::fread(v.data(), sizeof(T), n, f) != n) fail("short file");
        return v;
    }
};

static unsigned long long h = 0;
static void mix(unsigned long long v) { h = h * 1000003ull + (v & 0xffffffffull); }
template <class T> static void mix_all(const std::vector<T>& v) { for (const T& x : v) mix((unsigned long long)(long long)x); }

static void run_file(const char* path) {
    Reader in = {std::fopen(path, "rb")};
    if (!in.f) fail("cannot open the snapshot");
    const std::vector<int32_t> hd = in.take<int32_t>(10);
    const size_t nb = hd[0], nk = hd[1], ni = hd[2], np = hd[3], no = hd[4], nc = hd[5], nl = hd[6], nf = hd[7], nj = hd[8], nq = hd[9];
    const auto kf_start = in.take<int32_t>(nb + 1), kf_by_key = in.take<int32_t>(nk);
    const auto kf_bad = in.take<uint8_t>(nk);
    const auto kp_start = in.take<int32_t>(nk + 1), kp_point = in.take<int32_t>(ni);
    const auto kp_octave = in.take<uint8_t>(ni), kp_stereo = in.take<uint8_t>(ni);
    const auto pt_start = in.take<int32_t>(nb + 1);
    const auto pt_bad = in.take<uint8_t>(np);
    const auto pt_nobs = in.take<int32_t>(np), pt_found = in.take<int32_t>(np), pt_visible = in.take<int32_t>(np), obs_start = in.take<int32_t>(np + 1);
    const auto obs = in.take<uint32_t>(no);
    const auto obs_feat = in.take<int32_t>(no), call_start = in.take<int32_t>(nb + 1), call_kf = in.take<int32_t>(nc);
    const auto call_kind = in.take<uint8_t>(nc);
    const auto call_list = in.take<int32_t>(nc), call_n = in.take<int32_t>(nc), call_feat = in.take<int32_t>(nc), call_op = in.take<int32_t>(nc + 1);
    const auto list_point = in.take<int32_t>(nl), op_feat = in.take<int32_t>(nf), obs_out_start = in.take<int32_t>(nb + 1);
    if (std::fgetc(in.f) != EOF) fail("the file is longer than its totals say");
    std::fclose(in.f);

    FuseMap M;
    M.batch = (int)nb; M.n_kf = (int)nk; M.n_kp = (int)ni; M.n_pt = (int)np; M.n_obs = (int)no; M.n_call = (int)nc; M.n_list = (int)nl; M.n_feat = (int)nf;
    M.n_op = (int)nj; M.n_obs_out = (int)nq;
    M.kf_start = kf_start.data(); M.kf_by_key = kf_by_key.data(); M.kf_bad = kf_bad.data(); M.kp_start = kp_start.data(); M.kp_point = kp_point.data();
    M.kp_octave = kp_octave.data(); M.kp_stereo = kp_stereo.data(); M.pt_start = pt_start.data(); M.pt_bad = pt_bad.data(); M.pt_nobs = pt_nobs.data();
    M.pt_found = pt_found.data(); M.pt_visible = pt_visible.data(); M.obs_start = obs_start.data(); M.obs = obs.data(); M.obs_feat = obs_feat.data();
    M.call_start = call_start.data(); M.call_kf = call_kf.data(); M.call_kind = call_kind.data(); M.call_list = call_list.data(); M.call_n = call_n.data();
    M.call_feat = call_feat.data(); M.call_op = call_op.data(); M.list_point = list_point.data(); M.op_feat = op_feat.data(); M.obs_out_start = obs_out_start.data();

    std::vector<int32_t> rank(nk, -5), bad(np, -5), replaced(np, -5), dirty(np, -5), stamp(np, -5), head(np, -5), tail(np, -5), cnt(np, -5), dcnt(np, -5), next(np + nj, -5),
        rep(nj, -5), pfeat(no + nj, -5), info(nb, -5), tot(nb, -5), dtot(nb, -5);
    std::vector<uint32_t> found(np, 5u), visible(np, 5u), pool(no + nj, 5u);
    FuseWork W;
    W.rank = rank.data(); W.bad = bad.data(); W.replaced = replaced.data(); W.dirty = dirty.data(); W.stamp = stamp.data(); W.found = found.data(); W.visible = visible.data();
    W.head = head.data(); W.tail = tail.data(); W.cnt = cnt.data(); W.dcnt = dcnt.data(); W.next = next.data(); W.rep = rep.data(); W.pool = pool.data(); W.pfeat = pfeat.data();
    W.info = info.data(); W.tot = tot.data(); W.dtot = dtot.data();

    std::vector<int32_t> status(nb, 77), o_kp(ni, 77), o_nobs(np, 77), o_start(np + 1, 77), o_feat(nq, 77), o_need(nb, 77), o_found(np, 77), o_visible(np, 77), o_replaced(np, 77),
        d_start(np + 1, 77), d_kf(nq, 77), d_feat(nq, 77), o_reason(nj, 77), o_other(nj, 77), o_nfused(nc, 77);
    std::vector<uint8_t> o_bad(np, 77), o_dirty(np, 77), o_touched(no, 77);
    std::vector<uint32_t> o_obs(nq, 77u);
    FuseOut R;
    R.status = status.data(); R.kp_point_out = o_kp.data(); R.pt_bad_out = o_bad.data(); R.pt_nobs_out = o_nobs.data(); R.obs_start_out = o_start.data(); R.obs_out = o_obs.data();
    R.obs_feat_out = o_feat.data(); R.need = o_need.data(); R.pt_found_out = o_found.data(); R.pt_visible_out = o_visible.data(); R.pt_replaced_out = o_replaced.data();
    R.pt_dirty = o_dirty.data(); R.obs_touched = o_touched.data(); R.dirty_obs_start = d_start.data(); R.dirty_obs_kf = d_kf.data(); R.dirty_obs_feat = d_feat.data();
    R.op_reason = o_reason.data(); R.op_other = o_other.data(); R.call_nfused = o_nfused.data();

    fuse_run_host(M, W, R);

    h = 0;
    mix_all(o_kp); mix_all(o_bad); mix_all(o_nobs); mix_all(o_start); mix_all(o_obs); mix_all(o_feat); mix_all(o_need); mix_all(o_found); mix_all(o_visible);
    mix_all(o_replaced); mix_all(o_dirty); mix_all(o_touched); mix_all(d_start); mix_all(d_kf); mix_all(d_feat); mix_all(o_reason); mix_all(o_other); mix_all(o_nfused);
    mix_all(status);
    std::printf("checksum %016llx status", h);
    for (int32_t s : status) std::printf(" %d", s);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) fail("usage: map_fusion_core_host_test FILE [FILE ...]");
    for (int i = 1; i < argc; i++) run_file(argv[i]);
    return 0;
}
