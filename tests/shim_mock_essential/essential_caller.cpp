// essential_caller.cpp -- stand-alone caller of the drop-in Optimizer::OptimizeEssentialGraph and of
// OptimizerHip::OptimizeEssentialGraph over the stand-in map types of this directory and the C-ABI stubs
// (tests/test_shim_essential.py builds and runs it; never loaded into Python).  The scene is procedural so that the test can
// restate it: key frames 0..7 in a shuffled map order, 6 bad, loop key frame 1, current key frame 7.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "Optimizer.h"
#include "qsp_optimizer_shim.h"

using namespace ORB_SLAM2;
extern "C" long qsp_optimizer_failure_count(void);
extern "C" long qsp_optimizer_fallback_count(void);

static void make_kf(KeyFrame& kf, int k) {
    kf.mnId = k;
    kf.Tcw = cv::Mat(4, 4, CV_32F);
    const double a = 0.1 * k;
    kf.Tcw.at<float>(0, 0) = (float)std::cos(a); kf.Tcw.at<float>(0, 1) = (float)-std::sin(a);
    kf.Tcw.at<float>(1, 0) = (float)std::sin(a); kf.Tcw.at<float>(1, 1) = (float)std::cos(a);
    kf.Tcw.at<float>(2, 2) = 1.f; kf.Tcw.at<float>(3, 3) = 1.f;
    for (int r = 0; r < 3; ++r) kf.Tcw.at<float>(r, 3) = 0.1f * (r + 1) * k;
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    KeyFrame kf[8];
    for (int k = 0; k < 8; ++k) make_kf(kf[k], k);
    kf[6].bad = true;
    const int parent[8] = {-1, 4, 1, 2, 3, 4, 5, 5};
    for (int k = 1; k < 8; ++k) kf[k].parent = &kf[parent[k]];
    kf[4].loop_edges.insert(&kf[2]);
    kf[2].loop_edges.insert(&kf[4]);
    auto W = [&](int k, std::vector<std::pair<int, int>> w) { for (auto& e : w) kf[k].weights.push_back({e.first < 0 ? nullptr : &kf[e.first], e.second}); };
    W(3, {{1, 150}, {5, 130}, {2, 120}, {-1, 115}, {0, 110}, {4, 90}});
    W(4, {{3, 180}, {2, 170}, {1, 160}, {0, 140}, {6, 130}});
    W(5, {{3, 200}, {4, 150}, {2, 105}, {1, 30}, {0, 99}});
    W(7, {{2, 150}, {3, 120}, {5, 110}, {0, 50}, {1, 20}});
    Map map;
    for (int k : {3, 0, 5, 1, 7, 2, 6, 4}) map.kfs.push_back(&kf[k]);
    MapPoint mp[5];
    const int ref[5] = {3, 2, 0, 6, 1};
    for (int i = 0; i < 5; ++i) {
        mp[i].mnId = i;
        mp[i].pos = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) mp[i].pos.at<float>(r) = 0.25f * i + 0.5f * r;
        mp[i].ref = &kf[ref[i]];
        map.mps.push_back(&mp[i]);
    }
    mp[1].bad = true;
    mp[2].mnCorrectedByKF = 7; mp[2].mnCorrectedReference = 5;
    KeyFrameAndPose nonc, corr;
    corr[&kf[7]] = g2o::Sim3(Eigen::Quaterniond(0.9, 0.1, -0.2, 0.3), Eigen::Vector3d(1, 2, 3), 1.25);
    corr[&kf[5]] = g2o::Sim3(Eigen::Quaterniond(0.8, -0.3, 0.2, 0.1), Eigen::Vector3d(-1, 0.5, 4), 0.75);
    nonc[&kf[7]] = g2o::Sim3(Eigen::Quaterniond(0.7, 0.2, 0.1, -0.3), Eigen::Vector3d(0.5, -2, 1), 1.0);
    nonc[&kf[5]] = g2o::Sim3(Eigen::Quaterniond(0.6, 0.3, -0.1, 0.2), Eigen::Vector3d(2, 1, -1), 1.0);
    std::map<KeyFrame*, std::set<KeyFrame*>> conn;
    conn[&kf[7]] = {&kf[1], &kf[0], &kf[2]};
    conn[&kf[5]] = {&kf[1], &kf[3]};
    if (!std::strcmp(mode, "member")) {
        const int st = OptimizerHip::OptimizeEssentialGraph(&map, &kf[1], &kf[7], nonc, corr, conn, true);
        std::printf("status %d\n", st);
    } else {
        Optimizer::OptimizeEssentialGraph(&map, &kf[1], &kf[7], nonc, corr, conn, false);
    }
    for (int k = 0; k < 8; ++k) {
        std::printf("kf %d %d |", k, kf[k].n_set_pose);
        for (int i = 0; i < 16; ++i) std::printf(" %.9g", kf[k].Tcw.at<float>(i / 4, i % 4));
        std::printf("\n");
    }
    for (int i = 0; i < 5; ++i)
        std::printf("mp %d %d | %.9g %.9g %.9g\n", i, mp[i].n_updates, mp[i].pos.at<float>(0), mp[i].pos.at<float>(1), mp[i].pos.at<float>(2));
    std::printf("failures %ld fallbacks %ld\n", qsp_optimizer_failure_count(), qsp_optimizer_fallback_count());
    return 0;
}
