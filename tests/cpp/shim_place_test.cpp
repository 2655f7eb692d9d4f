// tests/cpp/shim_place_test.cpp — compile / link / run test of viorb_shim::KeyFrameDatabase (viorb_amd/shim/KeyFrameDatabase_shim.h)
// against stand-ins that carry the reference's member names (place_standin.h).
//   shim_place_test                      no device needed: without a device add, both Detect functions and loop_min_score throw with the
//                                        library's error text; erase of an absent key frame and clear do not
//   shim_place_test problem.bin out.bin  reads a problem written by tests/test_gpu_place_shim.py, runs loop_min_score, one loop query and one
//                                        relocalisation query and writes what they returned
#include <cstdio>
#include <stdexcept>
#include <vector>
#include "place_standin.h"
#include "KeyFrameDatabase_shim.h"

using namespace standin;
typedef viorb_shim::KeyFrameDatabase<KeyFrame, Frame> Database;

template <class Fn> static bool throws(Fn f) {
    try { f(); } catch (const std::runtime_error& e) { printf("  threw: %s\n", e.what()); return true; }
    return false;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::vector<KeyFrame> kf(3);
        for (int k = 0; k < 3; k++) { kf[k].mnId = k; kf[k].mBowVec[5] = 0.5; kf[k].mBowVec[7 + k] = 0.5; }
        kf[2].connected.insert(&kf[1]);
        Frame F; F.mBowVec = kf[0].mBowVec;
        Database db(100);
        db.erase(&kf[0]); db.clear();                                // neither needs a device
        if (viorb_device_count() >= 1) {
            db.add(&kf[0]); db.add(&kf[1]);
            const std::vector<KeyFrame*> r = db.DetectRelocalizationCandidates(&F), l = db.DetectLoopCandidates(&kf[2], 0.01f);
            const float ms = db.loop_min_score(&kf[2], std::vector<KeyFrame*>(1, &kf[1]));
            if (r.size() != 1 || r[0] != &kf[0] || l.size() != 1 || l[0] != &kf[0] || ms != 0.5f) { printf("FAIL: tiny database\n"); return 1; }
            printf("OK device\n");
            return 0;
        }
        printf("OK no device\n");
        const bool all = throws([&] { db.add(&kf[0]); }) && throws([&] { db.DetectLoopCandidates(&kf[2], 0.1f); }) &&
                         throws([&] { db.DetectRelocalizationCandidates(&F); }) && throws([&] { db.loop_min_score(&kf[2], std::vector<KeyFrame*>(1, &kf[1])); });
        if (!all || db.slot(&kf[0]) != -1) { printf("FAIL: no device, but a template did not throw or kept the key frame\n"); return 1; }
        return 0;
    }
    FILE* f = fopen(argv[1], "rb"); if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<double> in(bytes / sizeof(double)); if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2; fclose(f);
    // n_words N n_erased n_conn | erased | connected | covis10 [(N-1)*10] | per key frame: count, words, vals     (key frame N-1 asks)
    const double* q = in.data();
    const int n_words = (int)q[0], N = (int)q[1], n_erased = (int)q[2], n_conn = (int)q[3], S = N - 1;
    q += 4;
    const double *erased = q, *conn = q + n_erased, *cov = conn + n_conn;
    q = cov + (size_t)S * 10;
    std::vector<KeyFrame> kf(N);
    for (int k = 0; k < N; k++) {
        const int c = (int)*q++;
        for (int i = 0; i < c; i++) kf[k].mBowVec[(unsigned)q[i]] = q[c + i];
        q += 2 * c;
        kf[k].mnId = 1000 + k;
    }
    for (int s = 0; s < S; s++)
        for (int k = 0; k < 10; k++) if (cov[(size_t)s * 10 + k] >= 0) kf[s].covisible.push_back(&kf[(int)cov[(size_t)s * 10 + k]]);
    std::vector<KeyFrame*> vpConnected;
    for (int i = 0; i < n_conn; i++) { kf[S].connected.insert(&kf[(int)conn[i]]); vpConnected.push_back(&kf[(int)conn[i]]); }
    KeyFrame never_added; kf[S].connected.insert(&never_added);      // connected, but not in the database
    Frame F; F.mBowVec = kf[S].mBowVec;
    std::vector<double> out;
    try {
        Database db(n_words, 8, 1024);
        for (int s = 0; s < S; s++) db.add(&kf[s]);
        for (int i = 0; i < n_erased; i++) db.erase(&kf[(int)erased[i]]);
        const float ms = db.loop_min_score(&kf[S], vpConnected);
        const std::vector<KeyFrame*> l = db.DetectLoopCandidates(&kf[S], ms), r = db.DetectRelocalizationCandidates(&F);
        out.push_back(ms); out.push_back((double)l.size());
        for (size_t i = 0; i < l.size(); i++) out.push_back((double)l[i]->mnId);
        out.push_back((double)r.size());
        for (size_t i = 0; i < r.size(); i++) out.push_back((double)r[i]->mnId);
    } catch (const std::runtime_error& e) { printf("FAIL: %s\n", e.what()); return 1; }
    f = fopen(argv[2], "wb"); if (!f) return 2;
    fwrite(out.data(), sizeof(double), out.size(), f); fclose(f);
    printf("OK loop %d reloc %d\n", (int)out[1], (int)out[2 + (int)out[1]]);
    return 0;
}
