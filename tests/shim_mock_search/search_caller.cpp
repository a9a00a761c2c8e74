// search_caller.cpp -- stand-alone caller of OrbMatcherHip::SearchBySim3Batch over the stand-in map types of this directory and the
// stub of qsp_search_by_sim3_batch (tests/test_shim_search_sim3.py builds and runs it; never loaded into Python).  The scene is
// procedural so that the test can restate it: key frame 1 with 12 slots, three candidate key frames of 8, 0 and 10 slots.  Mode
// "mixed": every candidate key frame has a pyramid (levels, scale) and a grid (columns, rows) of its own, none of them key frame 1's.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mock_search.h"
#include "qsp_optimizer_shim.h"

using namespace ORB_SLAM2;

static const int N1 = 12, N2[3] = {8, 0, 10};

static const int MIX_LEVELS[3] = {5, 16, 1}, MIX_COLS[3] = {5, 64, 1}, MIX_ROWS[3] = {7, 64, 1};
static const float MIX_SCALE[3] = {1.5f, 1.1f, 1.3f}, MIX_LOG[3] = {0.4055f, 0.0953f, 0.2624f};

static void make_kf(SearchKeyFrame& kf, int k, int n, bool mixed = false) {
    const int levels = mixed ? MIX_LEVELS[k - 2] : 4, cols = mixed ? MIX_COLS[k - 2] : 64, rows = mixed ? MIX_ROWS[k - 2] : 48;
    const float scale = mixed ? MIX_SCALE[k - 2] : 1.2f;
    kf.mnId = k;
    kf.fx = 500.f + k; kf.fy = 510.f + k; kf.cx = 320.f + 0.5f * k; kf.cy = 240.f + 0.25f * k;
    kf.Tcw = cv::Mat(4, 4, CV_32F);
    const double a = 0.1 * k;
    kf.Tcw.at<float>(0, 0) = (float)std::cos(a); kf.Tcw.at<float>(0, 1) = (float)-std::sin(a);
    kf.Tcw.at<float>(1, 0) = (float)std::sin(a); kf.Tcw.at<float>(1, 1) = (float)std::cos(a);
    kf.Tcw.at<float>(2, 2) = 1.f; kf.Tcw.at<float>(3, 3) = 1.f;
    for (int r = 0; r < 3; ++r) kf.Tcw.at<float>(r, 3) = 0.1f * (r + 1) * k;
    kf.mDescriptors.rows = n;
    for (int j = 0; j < n; ++j) {
        kf.mvKeysUn.push_back(cv::KeyPoint{{7.f * j + k, 5.f * j + 2.f * k}, j % levels});
        for (int b = 0; b < 32; ++b) kf.mDescriptors.d.push_back((unsigned char)(j * 7 + b * 3 + k));
    }
    kf.mnMinX = -k; kf.mnMaxX = 640 + k; kf.mnMinY = -2 * k; kf.mnMaxY = 480 + k;
    kf.mnGridCols = cols; kf.mnGridRows = rows;
    kf.mfGridElementWidthInv = (float)cols / (float)(kf.mnMaxX - kf.mnMinX);
    kf.mfGridElementHeightInv = (float)rows / (float)(kf.mnMaxY - kf.mnMinY);
    kf.mnScaleLevels = levels;
    kf.mfLogScaleFactor = mixed ? MIX_LOG[k - 2] : 0.1823f;
    float s = 1.f;
    for (int o = 0; o < levels; ++o) { kf.mvScaleFactors.push_back(s); s *= scale; }
}
static std::vector<std::unique_ptr<SearchMapPoint>> g_points;       // owns every map point of the scene
static SearchMapPoint* make_mp(int id, int i, float dy) {
    g_points.emplace_back(new SearchMapPoint());
    SearchMapPoint* p = g_points.back().get();
    p->mnId = id;
    p->pos = cv::Mat(3, 1, CV_32F);
    p->pos.at<float>(0) = 0.1f * i - 0.5f; p->pos.at<float>(1) = 0.05f * i + dy; p->pos.at<float>(2) = 2.f + 0.3f * i;
    p->mfMaxDistance = 3.f + 0.25f * i + 0.01f * id;
    p->mfMinDistance = p->mfMaxDistance / 2.f;
    p->desc.rows = 1;
    for (int b = 0; b < 32; ++b) p->desc.d.push_back((unsigned char)(id * 5 + b));
    return p;
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    SearchKeyFrame kf1, kf2[3];
    make_kf(kf1, 1, N1);
    for (int i = 0; i < N1; ++i) {
        SearchMapPoint* p = make_mp(i, i, 0.f);
        p->obs[&kf1] = (size_t)i;
        if (i == 5) p->bad = true;                                      // a bad point: has_point 0
        kf1.slots.push_back(i == 3 ? nullptr : p);                      // a null slot
    }
    std::vector<SearchKeyFrame*> kfs;
    for (int c = 0; c < 3; ++c) {
        make_kf(kf2[c], 2 + c, N2[c], !std::strcmp(mode, "mixed"));
        for (int j = 0; j < N2[c]; ++j) {
            SearchMapPoint* p = make_mp(100 * (c + 1) + j, j, 0.1f * c);
            p->obs[&kf2[c]] = (size_t)j;
            if (j == 2) p->bad = true;
            kf2[c].slots.push_back(j == 1 ? nullptr : p);
        }
        kfs.push_back(&kf2[c]);
    }
    SearchMapPoint* foreign = make_mp(900, 1, 0.f);                      // a map point no candidate key frame observes
    std::vector<std::vector<SearchMapPoint*>> m(3, std::vector<SearchMapPoint*>(N1, nullptr));
    m[0][4] = kf2[0].slots[6];                                          // an earlier match: pre1[4] and pre2[6]
    m[0][7] = foreign;                                                  // ... one without an index in key frame 2: pre1[7] only
    m[1][2] = foreign;
    m[2][0] = kf2[2].slots[9];
    std::vector<float> s12 = {1.1f, 0.9f, 1.25f};
    std::vector<cv::Mat> R12, t12;
    for (int c = 0; c < 3; ++c) {
        cv::Mat R(3, 3, CV_32F), t(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) {
            for (int q = 0; q < 3; ++q) R.at<float>(r, q) = 10.f * c + 3.f * r + q;      // row-major: R(r, q) at 3 r + q
            t.at<float>(r) = 0.5f * c + r;
        }
        R12.push_back(R); t12.push_back(t);
    }
    std::vector<int> found = {-4, -4, -4};
    if (!std::strcmp(mode, "short")) s12.pop_back();                    // an argument of the wrong length
    const int st = OrbMatcherHip::SearchBySim3Batch(&kf1, kfs, m, s12, R12, t12, 7.5f, found);
    std::printf("status %d\nfound", st);
    for (int f : found) std::printf(" %d", f);
    std::printf("\n");
    for (int c = 0; c < 3; ++c) {
        std::printf("matches");
        for (SearchMapPoint* p : m[c]) std::printf(" %ld", p ? (long)p->mnId : -1L);
        std::printf("\n");
    }
    return 0;
}
