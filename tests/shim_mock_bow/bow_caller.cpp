// bow_caller.cpp -- stand-alone caller of both OrbMatcherHip::SearchByBoWBatch overloads over the stand-in map types of this
// directory and the stub of qsp_search_by_bow_batch (tests/test_shim_search_bow.py builds and runs it; never loaded into Python).
// The scene is procedural so that the test can restate it: key frames k = 1 (10 slots) and k = 2, 3, 4 (6, 0 and 8 slots), a frame
// of 7 key points.  Mode "kf": the loop-closing overload; "frame": the relocalisation overload; "kf_empty" / "frame_empty": no
// candidates.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mock_bow.h"
#include "qsp_optimizer_shim.h"

using namespace ORB_SLAM2;

static std::vector<std::unique_ptr<SearchMapPoint>> g_points;       // owns every map point of the scene

static void make_kf(BowKeyFrame& kf, int k, int n) {
    kf.mnId = k;
    kf.mDescriptors.rows = n;
    for (int j = 0; j < n; ++j) {
        kf.mvKeysUn.push_back(AngleKeyPoint{{1.f * j, 2.f * j}, j % 4, 10.f * j + k + 0.5f});
        for (int b = 0; b < 32; ++b) kf.mDescriptors.d.push_back((unsigned char)(j * 7 + b * 3 + k));
        g_points.emplace_back(new SearchMapPoint());
        SearchMapPoint* p = g_points.back().get();
        p->mnId = 100 * k + j;
        if (j == 2) p->bad = true;                                      // a bad point: not eligible
        kf.slots.push_back(j == 1 ? nullptr : p);                       // a null slot: not eligible
    }
    for (int j = n - 1; j >= 0; --j) kf.mFeatVec[3 * (j % 4) + k].push_back(j);      // lists in DESCENDING index order
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "kf";
    const int N[4] = {10, 6, 0, 8};
    BowKeyFrame kf[4];
    for (int k = 0; k < 4; ++k) make_kf(kf[k], k + 1, N[k]);
    BowFrame F;
    F.N = 7;
    F.mDescriptors.rows = 7;
    for (int j = 0; j < 7; ++j) {
        F.mvKeys.push_back(AngleKeyPoint{{3.f * j, 1.f * j}, 0, 3.f * j + 0.25f});
        for (int b = 0; b < 32; ++b) F.mDescriptors.d.push_back((unsigned char)(j * 5 + b));
        F.mFeatVec[2 * (j % 3)].push_back(j);
    }
    SearchMapPoint foreign;
    foreign.mnId = 900;
    std::vector<std::vector<SearchMapPoint*>> m(1, std::vector<SearchMapPoint*>(1, &foreign));      // sentinels: untouched on failure
    std::vector<int> counts = {-4};
    std::vector<BowKeyFrame*> cands;
    if (!std::strstr(mode, "empty")) cands = {&kf[1], &kf[2], &kf[3]};
    int st;
    if (!std::strncmp(mode, "kf", 2)) st = OrbMatcherHip::SearchByBoWBatch(&kf[0], cands, 0.75f, true, m, counts);
    else st = OrbMatcherHip::SearchByBoWBatch(cands, F, 0.9f, false, m, counts);
    std::printf("status %d\ncounts", st);
    for (int c : counts) std::printf(" %d", c);
    std::printf("\n");
    for (const auto& v : m) {
        std::printf("matches");
        for (SearchMapPoint* p : v) std::printf(" %ld", p ? (long)p->mnId : -1L);
        std::printf("\n");
    }
    return 0;
}
