// tests/cpp/shim_two_view_test.cpp — compile / link / run test of viorb_shim::Initializer (viorb_amd/shim/Initializer_shim.h) with the
// stand-ins of two_view_standin.h. Usage: shim_two_view_test problem.bin out.bin. The problem file (written by
// tests/test_gpu_two_view_shim.py) holds n1, n2, the seed, K4, the key points of both frames and vMatches12. The program runs
// Initializer::Initialize the way Tracking::MonocularInitialization does and writes what it returned. Exit code 0: it ran (whatever it
// returned), 3: the library reported an error (printed), 2: usage.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "two_view_standin.h"
#include "Initializer_shim.h"

typedef viorb_shim::Initializer<standin::Frame> Initializer;

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: shim_two_view_test problem.bin out.bin\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int hdr[3]; float K4[4];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(K4, 4, 4, f) != 4) return 2;
    const int n1 = hdr[0], n2 = hdr[1];
    std::vector<float> xy1(2 * n1 + 1), xy2(2 * n2 + 1); std::vector<int> m(n1 + 1);
    if ((int)std::fread(&xy1[0], 4, 2 * n1, f) != 2 * n1 || (int)std::fread(&xy2[0], 4, 2 * n2, f) != 2 * n2 || (int)std::fread(&m[0], 4, n1, f) != n1) return 2;
    std::fclose(f);
    standin::Frame F1, F2;
    F1.mK.create(3, 3, CV_32F); F1.mK.at<float>(0, 0) = K4[0]; F1.mK.at<float>(1, 1) = K4[1]; F1.mK.at<float>(0, 2) = K4[2]; F1.mK.at<float>(1, 2) = K4[3]; F1.mK.at<float>(2, 2) = 1.f;
    F2.mK = F1.mK;
    for (int i = 0; i < n1; i++) F1.mvKeysUn.push_back(cv::KeyPoint(xy1[2 * i], xy1[2 * i + 1]));
    for (int i = 0; i < n2; i++) F2.mvKeysUn.push_back(cv::KeyPoint(xy2[2 * i], xy2[2 * i + 1]));
    m.resize(n1);
    Initializer init(F1, 1.0, 200);
    init.mSeed = (unsigned)hdr[2];
    cv::Mat R21, t21; std::vector<cv::Point3f> vP3D; std::vector<bool> vbTriangulated;
    bool ok = false;
    try {
        ok = init.Initialize(F2, m, R21, t21, vP3D, vbTriangulated);
    } catch (const std::runtime_error& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int head[3] = {ok ? 1 : 0, init.mLastStatus, init.mLastReason};
    std::fwrite(head, 4, 3, o);
    if (ok) {
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { const float v = R21.at<float>(r, c); std::fwrite(&v, 4, 1, o); }
        for (int r = 0; r < 3; r++) { const float v = t21.at<float>(r); std::fwrite(&v, 4, 1, o); }
        for (int i = 0; i < n1; i++) { const float p[3] = {vP3D[i].x, vP3D[i].y, vP3D[i].z}; std::fwrite(p, 4, 3, o); }
        for (int i = 0; i < n1; i++) { const unsigned char b = vbTriangulated[i]; std::fwrite(&b, 1, 1, o); }
    }
    std::fclose(o);
    std::printf("Initialize returned %d (status %d, reason %d)\n", (int)ok, init.mLastStatus, init.mLastReason);
    return 0;
}
