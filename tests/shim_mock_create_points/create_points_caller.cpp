// create_points_caller.cpp -- stand-alone caller of OrbMatcherHip::CreateNewMapPointsBatch and TriangulateBatch over the stand-in
// map types of this directory and the stub of the two library calls (tests/test_shim_triangulate.py builds and runs it; never loaded
// into Python).  The scene is procedural so that the test can restate it: key frames k = 1 (10 slots, the source) and k = 2, 3, 4
// (6, 0 and 8 slots, the neighbours), every value a function of (k, slot) and no two arrays alike.  Mode "create": the chained call
// (bOnlyStereo = false, no orientation check); "flags": both flags set; "tri": TriangulateBatch on hand-made match lists; "empty":
// no neighbours.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mock_create_points.h"
#include "qsp_optimizer_shim.h"

using namespace ORB_SLAM2;

static std::vector<std::unique_ptr<SearchMapPoint>> g_points;       // owns every map point of the scene

static void make_kf(CreateKeyFrame& kf, int k, int n) {
    kf.mnId = k;
    kf.mDescriptors.rows = n;
    kf.fx = 500.f + k; kf.fy = 510.f + k; kf.cx = 320.f + 0.5f * k; kf.cy = 240.f - 0.25f * k;
    kf.invfx = 0.002f + 0.0001f * k; kf.invfy = 0.003f - 0.0001f * k;              // (not 1 / fx: the shim must READ them)
    kf.mb = 0.08f + 0.01f * k; kf.mbf = 40.f + k; kf.mfScaleFactor = 1.2f + 0.05f * k;
    for (int l = 0; l < 4; ++l) {
        kf.mvScaleFactors.push_back(1.f + 0.25f * l + 0.01f * k);
        kf.mvLevelSigma2.push_back(2.f + l + 0.5f * k);
    }
    for (int j = 0; j < n; ++j) {
        kf.mvKeysUn.push_back(AngleKeyPoint{{1.5f * j + k, 2.25f * j - k}, (j + k) % 4, 10.f * j + k + 0.5f});
        kf.mvKeys.push_back(cv::KeyPoint{{1.5f * j + k + 0.75f, 2.25f * j - k - 0.375f}, (j + k + 1) % 4});   // another point AND another octave
        kf.mvuRight.push_back(j % 3 == 0 ? 5.f + j : -1.f);
        kf.mvDepth.push_back(j % 3 == 0 ? 3.f + 0.5f * j + k : -1.f);
        for (int b = 0; b < 32; ++b) kf.mDescriptors.d.push_back((unsigned char)(j * 7 + b * 3 + k));
        g_points.emplace_back(new SearchMapPoint());
        SearchMapPoint* p = g_points.back().get();
        p->mnId = 100 * k + j;
        kf.slots.push_back(j == 4 ? p : nullptr);                       // slot 4 is filled: not eligible
    }
    for (int j = 0; j < n; ++j) kf.mFeatVec[3 * (j % 4) + k].push_back(j);
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
    const char* mode = argc > 1 ? argv[1] : "create";
    const int N[4] = {10, 6, 0, 8};
    CreateKeyFrame kf[4];
    for (int k = 0; k < 4; ++k) make_kf(kf[k], k + 1, N[k]);
    std::vector<OrbMatcherHip::NewPoint> vNew(1);                       // sentinels: untouched on failure
    vNew[0].k = 77; vNew[0].idx1 = 78; vNew[0].idx2 = 79;
    std::vector<int> counts = {-4};
    std::vector<CreateKeyFrame*> cands;
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
    int st;
    if (!std::strcmp(mode, "tri")) {
        std::vector<std::vector<std::pair<size_t, size_t>>> lists(3);
        lists[0] = {{1, 5}, {3, 0}, {8, 2}};
        lists[2] = {{0, 7}, {2, 1}, {9, 3}};
        st = OrbMatcherHip::TriangulateBatch(&kf[0], cands, lists, vNew);
    } else {
        const bool flags = !std::strcmp(mode, "flags");
        st = OrbMatcherHip::CreateNewMapPointsBatch(&kf[0], cands, vF12, flags, flags, vNew, counts);
    }
    std::printf("status %d\ncounts", st);
    for (int c : counts) std::printf(" %d", c);
    std::printf("\n");
    for (const auto& p : vNew) {
        std::printf("new %zu %zu %zu %d %d", p.k, p.idx1, p.idx2, p.x3D.rows, p.x3D.cols);
        for (int r = 0; r < p.x3D.rows * p.x3D.cols; ++r) std::printf(" %.9g", p.x3D.at<float>(r));
        std::printf("\n");
    }
    return 0;
}
