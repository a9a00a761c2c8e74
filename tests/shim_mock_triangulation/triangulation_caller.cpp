// triangulation_caller.cpp -- stand-alone caller of OrbMatcherHip::SearchForTriangulationBatch over the stand-in map types of this
// directory and the stub of qsp_search_for_triangulation_batch (tests/test_shim_search_triangulation.py builds and runs it; never
// loaded into Python).  The scene is procedural so that the test can restate it: key frames k = 1 (10 slots, the source) and
// k = 2, 3, 4 (6, 0 and 8 slots, the neighbours).  Mode "tri": three neighbours, bOnlyStereo = false, checkOri = false; "stereo":
// bOnlyStereo = true, checkOri = true; "empty": no neighbours.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mock_triangulation.h"
#include "qsp_optimizer_shim.h"

using namespace ORB_SLAM2;

static std::vector<std::unique_ptr<SearchMapPoint>> g_points;       // owns every map point of the scene

static void make_kf(TriKeyFrame& kf, int k, int n) {
    kf.mnId = k;
    kf.mDescriptors.rows = n;
    kf.fx = 500.f + k; kf.fy = 510.f + k; kf.cx = 320.f + 0.5f * k; kf.cy = 240.f - 0.25f * k;
    for (int l = 0; l < 4; ++l) {
        kf.mvScaleFactors.push_back(1.f + 0.25f * l + 0.01f * k);
        kf.mvLevelSigma2.push_back(2.f + l + 0.5f * k);
    }
    for (int j = 0; j < n; ++j) {
        kf.mvKeysUn.push_back(AngleKeyPoint{{1.5f * j + k, 2.25f * j - k}, (j + k) % 4, 10.f * j + k + 0.5f});
        kf.mvuRight.push_back(j % 3 == 0 ? 5.f : -1.f);
        for (int b = 0; b < 32; ++b) kf.mDescriptors.d.push_back((unsigned char)(j * 7 + b * 3 + k));
        g_points.emplace_back(new SearchMapPoint());
        SearchMapPoint* p = g_points.back().get();
        p->mnId = 100 * k + j;
        if (j == 2) p->bad = true;                                      // a BAD point still fills its slot: not eligible
        kf.slots.push_back(j == 2 || j == 4 ? p : nullptr);             // every other slot is null: eligible
    }
    for (int j = n - 1; j >= 0; --j) kf.mFeatVec[3 * (j % 4) + k].push_back(j);      // lists in DESCENDING index order
    kf.Tcw = cv::Mat(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) kf.Tcw.at<float>(r, c) = (r == c ? 0.9f : 0.1f * (r - c)) + 0.01f * k;
        kf.Tcw.at<float>(r, 3) = 0.3f * r - 0.2f * k + 1.7f;
    }
    kf.Tcw.at<float>(3, 3) = 1.f;
    kf.Ow = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) kf.Ow.at<float>(r) = 0.37f * (r + 1) - 0.11f * k;
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "tri";
    const int N[4] = {10, 6, 0, 8};
    TriKeyFrame kf[4];
    for (int k = 0; k < 4; ++k) make_kf(kf[k], k + 1, N[k]);
    std::vector<std::vector<std::pair<size_t, size_t>>> pairs(1, std::vector<std::pair<size_t, size_t>>(1, std::make_pair((size_t)900, (size_t)901)));
    std::vector<int> counts = {-4};                                     // sentinels: untouched on failure
    std::vector<TriKeyFrame*> cands;
    std::vector<cv::Mat> vF12;
    if (std::strcmp(mode, "empty")) {
        cands = {&kf[1], &kf[2], &kf[3]};
        for (int c = 0; c < 3; ++c) {
            cv::Mat F(3, 3, CV_32F);
            for (int r = 0; r < 3; ++r)
                for (int q = 0; q < 3; ++q) F.at<float>(r, q) = 10.f * c + 3 * r + q + 0.5f;
            vF12.push_back(F);
        }
    }
    const bool stereo = !std::strcmp(mode, "stereo");
    const int st = OrbMatcherHip::SearchForTriangulationBatch(&kf[0], cands, vF12, stereo, stereo, pairs, counts);
    std::printf("status %d\ncounts", st);
    for (int c : counts) std::printf(" %d", c);
    std::printf("\n");
    for (const auto& v : pairs) {
        std::printf("pairs");
        for (const auto& p : v) std::printf(" %zu %zu", p.first, p.second);
        std::printf("\n");
    }
    return 0;
}
