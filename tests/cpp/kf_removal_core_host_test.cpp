// tests/cpp/kf_removal_core_host_test.cpp — the host build of viorb_amd/csrc/kf_removal_core.h as a stand-alone program. No GPU, no library:
// only the header.
//   kf_removal_core_host_test FILE [FILE ...]   the program that tests/test_kf_removal_host_sanitized.py compiles with
//                                               -fsanitize=address,undefined and runs as a child process. Every FILE is a packed snapshot
//                                               that viorb_amd/snapshot.py's write_snapshot leaves: 8 totals and ccap as int32, then the
//                                               arrays of viorb_kfr_map in their order, each exactly as long as its total says, so that
//                                               the address sanitizer sees any read or write past an end. kfr_run_host runs on it with
//                                               a workspace and result arrays of exactly the totals, filled with 77 beforehand. One line
//                                               per file: a checksum over every result array in the order of viorb_kfr_result (status
//                                               last), which the Python side compares with the checker's, and the status of every stream.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "kf_removal_core.h"

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
    const std::vector<int32_t> hd = in.take<int32_t>(9);
    const size_t nb = hd[0], nk = hd[1], ni = hd[2], np = hd[3], no = hd[4], nc = hd[5], nr = hd[6], nop = hd[7], cc = hd[8];
    const auto kf_start = in.take<int32_t>(nb + 1), kf_by_key = in.take<int32_t>(nk);
    const auto kf_flags = in.take<uint8_t>(nk);
    const auto kf_parent = in.take<int32_t>(nk), kf_prev = in.take<int32_t>(nk), kf_next = in.take<int32_t>(nk);
    const auto kf_pose12 = in.take<float>(12 * nk);
    const auto kp_start = in.take<int32_t>(nk + 1), kp_point = in.take<int32_t>(ni), pt_start = in.take<int32_t>(nb + 1);
    const auto pt_bad = in.take<uint8_t>(np);
    const auto pt_nobs = in.take<int32_t>(np), pt_ref = in.take<int32_t>(np), obs_start = in.take<int32_t>(np + 1);
    const auto obs = in.take<uint32_t>(no);
    const auto conn_start = in.take<int32_t>(nk + 1), conn_kf = in.take<int32_t>(nc), conn_w = in.take<int32_t>(nc);
    const auto ord_start = in.take<int32_t>(nk + 1), ord_kf = in.take<int32_t>(nr), ord_w = in.take<int32_t>(nr);
    const auto op_start = in.take<int32_t>(nb + 1), op_kf = in.take<int32_t>(nop);
    const auto op_kind = in.take<uint8_t>(nop);
    if (std::fgetc(in.f) != EOF) fail("the file is longer than its totals say");
    std::fclose(in.f);

    KfrMap M;
    CovMap& C = M.C;
    C.batch = (int)nb; C.n_kf = (int)nk; C.n_kp = (int)ni; C.n_pt = (int)np; C.n_obs = (int)no; C.n_conn = (int)nc; C.n_ord = (int)nr; C.n_target = (int)nop;
    C.kf_start = kf_start.data(); C.kf_by_key = kf_by_key.data(); C.kf_flags = kf_flags.data(); C.kf_parent = kf_parent.data(); C.kp_start = kp_start.data();
    C.kp_point = kp_point.data(); C.pt_start = pt_start.data(); C.pt_bad = pt_bad.data(); C.obs_start = obs_start.data(); C.obs = obs.data();
    C.conn_start = conn_start.data(); C.conn_kf = conn_kf.data(); C.conn_w = conn_w.data(); C.ord_start = ord_start.data(); C.ord_kf = ord_kf.data(); C.ord_w = ord_w.data();
    C.target_start = op_start.data(); C.target_kf = op_kf.data(); C.ccap = (int)cc; C.erase_targets = 0;
    M.kf_prev = kf_prev.data(); M.kf_next = kf_next.data(); M.kf_pose12 = kf_pose12.data(); M.pt_nobs = pt_nobs.data(); M.pt_ref = pt_ref.data(); M.op_kind = op_kind.data();

    std::vector<int32_t> rank(nk, -5), flags(nk, -5), parent(nk, -5), prev(nk, -5), next(nk, -5), mark(nk, -5), child(nk, -5), pt(np, -5), ref(np, -5), info(nb, -5);
    KfrWork W;
    W.C = CovWork();
    W.C.rank = rank.data(); W.C.flags = flags.data(); W.C.info = info.data();
    W.parent = parent.data(); W.prev = prev.data(); W.next = next.data(); W.mark = mark.data(); W.child = child.data(); W.pt = pt.data(); W.ref = ref.data();

    std::vector<int32_t> ck(nk * cc, 77), cw(ck), ok(ck), ow(ck), cn(nk, 77), on(cn), status(nb, 77), o_parent(cn), o_prev(cn), o_next(cn), o_nobs(np, 77), o_ref(o_nobs),
        o_kp(ni, 77), o_reason(nop, 77), o_children(o_reason), o_fallback(o_reason), o_rebuilt(o_reason), o_points_bad(o_reason);
    std::vector<uint8_t> o_flags(nk, 77), o_repreint(o_flags), o_touched(o_flags), o_bad(np, 77), o_alive(no, 77);
    std::vector<float> o_Tcp(12 * nk, 77.0f);
    KfrOut R;
    R.C = CovOut();
    R.C.conn_kf_out = ck.data(); R.C.conn_w_out = cw.data(); R.C.conn_n_out = cn.data(); R.C.ord_kf_out = ok.data(); R.C.ord_w_out = ow.data(); R.C.ord_n_out = on.data();
    R.C.status = status.data(); R.C.kf_touched = o_touched.data();
    R.kf_parent_out = o_parent.data(); R.kf_flags_out = o_flags.data(); R.kf_prev_out = o_prev.data(); R.kf_next_out = o_next.data(); R.kf_repreint = o_repreint.data();
    R.kf_Tcp_out = o_Tcp.data(); R.pt_nobs_out = o_nobs.data(); R.pt_bad_out = o_bad.data(); R.obs_alive = o_alive.data(); R.pt_ref_out = o_ref.data(); R.kp_point_out = o_kp.data();
    R.op_reason = o_reason.data(); R.op_children = o_children.data(); R.op_fallback = o_fallback.data(); R.op_rebuilt = o_rebuilt.data(); R.op_points_bad = o_points_bad.data();

    kfr_run_host(M, W, R);

    h = 0;
    mix_all(ck); mix_all(cw); mix_all(cn); mix_all(ok); mix_all(ow); mix_all(on);
    mix_all(o_parent); mix_all(o_flags); mix_all(o_prev); mix_all(o_next); mix_all(o_repreint);
    for (float v : o_Tcp) { uint32_t bits; std::memcpy(&bits, &v, 4); mix(bits); }
    mix_all(o_touched); mix_all(o_nobs); mix_all(o_bad); mix_all(o_alive); mix_all(o_ref); mix_all(o_kp);
    mix_all(o_reason); mix_all(o_children); mix_all(o_fallback); mix_all(o_rebuilt); mix_all(o_points_bad); mix_all(status);
    std::printf("checksum %016llx status", h);
    for (int32_t s : status) std::printf(" %d", s);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) fail("usage: kf_removal_core_host_test FILE [FILE ...]");
    for (int i = 1; i < argc; i++) run_file(argv[i]);
    return 0;
}
