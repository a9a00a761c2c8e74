// ransac_caller.cpp -- stand-alone caller of Sim3SolverHip::FindBatch over the stand-in map types of this directory and the stub of
// qsp_sim3_ransac_batch (tests/test_shim_sim3_ransac.py builds and runs it; never loaded into Python).  The scene is procedural so
// that the test can restate it: key frame 1 with 30 slots, five candidate key frames.
#include <cstdio>
#include <cstring>
#include <cmath>
#include <memory>
#include <vector>

#include "mock_ransac.h"
#include "qsp_optimizer_shim.h"

using namespace ORB_SLAM2;

static const int N_SLOTS = 30, N_KEYS = 40;

static void make_kf(RansacKeyFrame& kf, int k) {
    kf.mnId = k;
    kf.mK = cv::Mat(3, 3, CV_32F);
    kf.mK.at<float>(0, 0) = 500.f + k; kf.mK.at<float>(1, 1) = 510.f + k;
    kf.mK.at<float>(0, 2) = 320.f + 0.5f * k; kf.mK.at<float>(1, 2) = 240.f + 0.25f * k; kf.mK.at<float>(2, 2) = 1.f;
    kf.Tcw = cv::Mat(4, 4, CV_32F);
    const double a = 0.1 * k;
    kf.Tcw.at<float>(0, 0) = (float)std::cos(a); kf.Tcw.at<float>(0, 1) = (float)-std::sin(a);
    kf.Tcw.at<float>(1, 0) = (float)std::sin(a); kf.Tcw.at<float>(1, 1) = (float)std::cos(a);
    kf.Tcw.at<float>(2, 2) = 1.f; kf.Tcw.at<float>(3, 3) = 1.f;
    for (int r = 0; r < 3; ++r) kf.Tcw.at<float>(r, 3) = 0.1f * (r + 1) * k;
    for (int j = 0; j < N_KEYS; ++j) kf.mvKeysUn.push_back(cv::KeyPoint{{7.f * j, 5.f * j}, j % 4});
    float s = 1.f;
    for (int o = 0; o < 4; ++o) { kf.mvLevelSigma2.push_back(s * s); s *= 1.2f; }
}
static std::vector<std::unique_ptr<MapPoint>> g_points;       // owns every map point of the scene
static MapPoint* make_mp(int id, float x, float y, float z) {
    g_points.emplace_back(new MapPoint());
    MapPoint* p = g_points.back().get();
    p->mnId = id;
    p->pos = cv::Mat(3, 1, CV_32F);
    p->pos.at<float>(0) = x; p->pos.at<float>(1) = y; p->pos.at<float>(2) = z;
    return p;
}

struct Scene {
    RansacKeyFrame kf1, kf[5];
    std::vector<std::vector<MapPoint*>> m;    // vpMatched12 of the five candidates
    Scene() : m(5) {
        make_kf(kf1, 1);
        for (int c = 0; c < 5; ++c) make_kf(kf[c], 2 + c);
        for (int i = 0; i < N_SLOTS; ++i) {
            MapPoint* p = make_mp(i, 0.1f * i - 0.5f, 0.05f * i, 2.f + 0.3f * i);
            if (i != 4) p->obs[&kf1] = (size_t)((i * 2) % N_KEYS);                // slot 4: not in key frame 1, index -1
            if (i == 5) p->bad = true;                                            // bad pMP1
            kf1.mps.push_back(i == 3 ? nullptr : p);                              // null pMP1
        }
        for (int c = 0; c < 5; ++c)
            for (int i = 0; i < N_SLOTS; ++i) {
                MapPoint* p = make_mp(100 * (c + 1) + i, 0.1f * i - 0.4f, 0.05f * i + 0.1f * c, 2.5f + 0.3f * i);
                if (i != 9) p->obs[&kf[c]] = (size_t)((i * 3 + c) % N_KEYS);      // slot 9: not in the candidate, index -1
                if (i == 7) p->bad = true;                                        // bad pMP2
                const bool none = i == 2 || (c == 2 && i >= 15) || (c == 4 && i >= 26);   // candidate 2 keeps 9, candidate 4 exactly 20
                m[c].push_back(none ? nullptr : p);
            }
    }
};

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    Scene sc;
    std::vector<RansacKeyFrame*> kfs;
    for (int c = 0; c < 5; ++c) kfs.push_back(&sc.kf[c]);
    int k = 0, lo_bad = 0;
    std::vector<int> his;
    auto draw = [&](int lo, int hi) { lo_bad += lo != 0; his.push_back(hi); return lo + (17 * k++ + 3) % (hi - lo + 1); };
    Sim3SolverHip::Result out;
    if (!std::strcmp(mode, "prefilled")) {             // what a failed call must leave alone
        out.cand.resize(1);
        out.cand[0].first_it = 77;
        out.order.assign(1, 5);
    }
    const int st = Sim3SolverHip::FindBatch(&sc.kf1, kfs, sc.m, !std::strcmp(mode, "fix"), draw, out);
    // with a caller's minInliers below 3 a candidate of fewer than three matches still has no triple to draw: 0 iterations
    std::printf("small %d %d %d %d\n", Sim3SolverHip::Iterations(2, 0.99, 1, 300), Sim3SolverHip::Iterations(0, 0.99, 0, 300),
                Sim3SolverHip::Iterations(3, 0.99, 3, 300), Sim3SolverHip::Iterations(4, 0.99, 2, 300));
    std::printf("status %d\nlo_bad %d\nhis", st, lo_bad);
    for (int h : his) std::printf(" %d", h);
    std::printf("\norder");
    for (int c : out.order) std::printf(" %d", c);
    std::printf("\n");
    for (size_t c = 0; c < out.cand.size(); ++c) {
        const Sim3SolverHip::Candidate& C = out.cand[c];
        std::printf("cand %zu %d %d %d %d %.9g |", c, C.N, C.nIterations, C.first_it, C.nInliers, C.s);
        for (float v : C.R) std::printf(" %.9g", v);
        std::printf(" |");
        for (float v : C.t) std::printf(" %.9g", v);
        std::printf(" |");
        for (bool b : C.vbInliers) std::printf(" %d", b ? 1 : 0);
        std::printf("\n");
    }
    return 0;
}
