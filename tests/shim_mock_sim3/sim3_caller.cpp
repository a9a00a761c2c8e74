// sim3_caller.cpp -- stand-alone caller of the drop-in Optimizer::OptimizeSim3 and of OptimizerHip::OptimizeSim3(Batch) over the
// stand-in map types of this directory and the C-ABI stubs (tests/test_shim_sim3.py builds and runs it; never loaded into Python).
// The scene is procedural so that the test can restate it: key frame 1 with 20 slots, two candidate key frames.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "Optimizer.h"
#include "qsp_optimizer_shim.h"

using namespace ORB_SLAM2;
extern "C" long qsp_optimizer_failure_count(void);
extern "C" long qsp_optimizer_fallback_count(void);

static void make_kf(KeyFrame& kf, int k, int n_keys) {
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
    for (int j = 0; j < n_keys; ++j) kf.mvKeysUn.push_back(cv::KeyPoint{{100.f * k + 7.f * j + 0.25f, 50.f + 5.f * j + 0.5f * k}, j % 4});
    for (int o = 0; o < 4; ++o) kf.mvInvLevelSigma2.push_back(1.f / (float)(1 << o));
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
    KeyFrame kf1, kf2, kf3;
    std::vector<MapPoint*> m2, m3;            // vpMatches1 of the two candidates
    Scene() {
        const int N = 20;
        make_kf(kf1, 1, N); make_kf(kf2, 2, 25); make_kf(kf3, 3, 25);
        for (int i = 0; i < N; ++i) {
            MapPoint* p = make_mp(i, 0.1f * i - 0.5f, 0.05f * i, 2.f + 0.3f * i);
            if (i == 5) p->bad = true;                                            // bad pMP1
            kf1.mps.push_back(i == 3 ? nullptr : p);                              // null pMP1
        }
        for (int c = 0; c < 2; ++c) {
            KeyFrame* kf = c ? &kf3 : &kf2;
            std::vector<MapPoint*>& m = c ? m3 : m2;
            for (int i = 0; i < N; ++i) {
                MapPoint* p = make_mp(100 * (c + 1) + i, 0.1f * i - 0.4f, 0.05f * i + 0.1f * c, 2.5f + 0.3f * i);
                if (i != 9) p->obs[kf] = (size_t)((i * 3 + c) % 25);              // slot 9: not in the key frame, index -1
                if (i == 7) p->bad = true;                                        // bad pMP2
                m.push_back((i == 2 || (c == 1 && i >= 10)) ? nullptr : p);       // null match; candidate 2 keeps 5 pairs only
            }
        }
    }
};

static void show(const char* tag, int n, const std::vector<MapPoint*>& m, const g2o::Sim3& S) {
    std::printf("%s %d |", tag, n);
    for (MapPoint* p : m) std::printf(" %d", p ? 1 : 0);
    std::printf(" | %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", S.translation()[0], S.translation()[1], S.translation()[2],
                S.rotation().x(), S.rotation().y(), S.rotation().z(), S.rotation().w(), S.scale());
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    Scene sc;
    g2o::Sim3 S2(Eigen::Quaterniond(0.9, 0.1, -0.2, 0.3), Eigen::Vector3d(1, 2, 3), 1.25);
    g2o::Sim3 S3(Eigen::Quaterniond(0.8, -0.3, 0.2, 0.1), Eigen::Vector3d(-1, 0.5, 4), 0.75);
    if (!std::strcmp(mode, "single")) {                // OptimizerHip::OptimizeSim3 on the full and on the early-return path
        int st = -1;
        int n = OptimizerHip::OptimizeSim3(&sc.kf1, &sc.kf2, sc.m2, S2, 10.f, true, &st);
        std::printf("status %d\n", st);
        show("full", n, sc.m2, S2);
        n = OptimizerHip::OptimizeSim3(&sc.kf1, &sc.kf3, sc.m3, S3, 10.f, false, &st);
        std::printf("status %d\n", st);
        show("early", n, sc.m3, S3);
    } else if (!std::strcmp(mode, "batch")) {
        std::vector<KeyFrame*> kfs{&sc.kf2, &sc.kf3};
        std::vector<std::vector<MapPoint*>> m{sc.m2, sc.m3};
        std::vector<g2o::Sim3> S{S2, S3};
        std::vector<int> n;
        const int st = OptimizerHip::OptimizeSim3Batch(&sc.kf1, kfs, m, S, 10.f, false, n);
        std::printf("status %d\n", st);
        if (st == QSP_OK) { show("full", n[0], m[0], S[0]); show("early", n[1], m[1], S[1]); }
    } else {                                           // the drop-in member, as LoopClosing::ComputeSim3 calls it
        const int n = Optimizer::OptimizeSim3(&sc.kf1, &sc.kf2, sc.m2, S2, 10, true);
        show("dropin", n, sc.m2, S2);
        std::printf("failures %ld fallbacks %ld\n", qsp_optimizer_failure_count(), qsp_optimizer_fallback_count());
    }
    return 0;
}
