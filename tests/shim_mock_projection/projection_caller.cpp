// projection_caller.cpp -- stand-alone caller of OrbMatcherHip::SearchLocalPoints and OrbMatcherHip::SearchByProjection over the
// stand-in types of this directory and the stub of qsp_search_by_projection (tests/test_shim_search_projection.py builds and runs
// it; never loaded into Python).  Everything a frame and a point hold is procedural (make_frame, make_point), so that the test can
// restate it.  Usage: projection_caller local|last.
// The current frame is frame 1 with 7 key points; its slot 2 holds an observed point (id 100) and its slot 4 a point without
// observations (id 101).  local: the local map points are ids 0..5 with 1 null, 2 bad and 3 already seen in this frame.  last: the
// last frame is frame 2 with 6 key points holding ids 0..5 with 1 null, slot 2 an outlier and 4 bad (the reference does not ask).
// Prints the status, n_matches, every point's tracking members and the current frame's slots as point ids.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mock_projection.h"
#include "qsp_optimizer_shim.h"

using namespace ORB_SLAM2;

static void make_frame(ProjFrame& F, int k, int n) {
    F.N = n;
    F.mnId = 10 + k;
    F.fx = 500.f + k; F.fy = 510.f + k; F.cx = 320.f + 0.5f * k; F.cy = 240.f - 0.25f * k; F.mbf = 40.f + k; F.mb = 0.1f + 0.01f * k;
    F.mnMinX = -1.5f - k; F.mnMaxX = 640.5f + k; F.mnMinY = -2.25f; F.mnMaxY = 481.75f;
    F.mfGridElementWidthInv = 64.f / (F.mnMaxX - F.mnMinX);
    F.mfGridElementHeightInv = 48.f / (F.mnMaxY - F.mnMinY);
    F.mnScaleLevels = 4;
    F.mfLogScaleFactor = 0.2f + 0.01f * k;
    for (int l = 0; l < 4; ++l) F.mvScaleFactors.push_back(1.f + 0.25f * l + 0.01f * k);
    F.mDescriptors.rows = n;
    for (int j = 0; j < n; ++j) {
        F.mvKeysUn.push_back(ProjKeyPoint{{1.5f * j + k, 2.25f * j - k}, (j + k) % 4, 10.f * j + k});
        F.mvKeys.push_back(ProjKeyPoint{{1.5f * j + k + 0.5f, 2.25f * j - k - 0.5f}, (j + k + 1) % 4, 10.f * j + k + 3.f});
        F.mvuRight.push_back(j % 3 == 0 ? 5.f + j : -1.f);
        for (int b = 0; b < 32; ++b) F.mDescriptors.d.push_back((unsigned char)(j * 7 + b * 3 + k));
    }
    F.mvpMapPoints.assign(n, nullptr);
    F.mvbOutlier.assign(n, false);
    F.mTcw = cv::Mat(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) F.mTcw.at<float>(r, c) = (r == c ? 0.9f : 0.1f * (r - c)) + 0.01f * k;
        F.mTcw.at<float>(r, 3) = 0.3f * r - 0.2f * k + 1.7f;
    }
    F.mTcw.at<float>(3, 3) = 1.f;
    F.Ow = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) F.Ow.at<float>(r) = 0.37f * (r + 1) - 0.11f * k;
}

static void make_point(ProjMapPoint& p, int i) {
    p.mnId = i;
    p.pos = cv::Mat(3, 1, CV_32F);
    p.nrm = cv::Mat(3, 1, CV_32F);
    const float X[3] = {0.1f * i + 1.f, 0.2f * i - 1.f, 0.05f * i + 3.f}, N[3] = {0.01f * i, 0.02f * i, 1.f - 0.001f * i};
    for (int r = 0; r < 3; ++r) { p.pos.at<float>(r) = X[r]; p.nrm.at<float>(r) = N[r]; }
    p.mfMaxDistance = 10.f + i;
    p.mfMinDistance = 1.f + 0.1f * i;
    p.desc.rows = 1;
    for (int b = 0; b < 32; ++b) p.desc.d.push_back((unsigned char)(i * 5 + b));
    p.n_obs = i % 3;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const bool local = std::strcmp(argv[1], "local") == 0;
    std::vector<std::unique_ptr<ProjMapPoint>> pts;
    for (int i = 0; i < 6; ++i) { pts.emplace_back(new ProjMapPoint); make_point(*pts.back(), i); }
    ProjMapPoint held, temporal;
    make_point(held, 100); held.n_obs = 2;
    make_point(temporal, 101); temporal.n_obs = 0;
    ProjFrame cur, last;
    make_frame(cur, 1, 7);
    cur.mvpMapPoints[2] = &held;
    cur.mvpMapPoints[4] = &temporal;
    int n_matches = -5, rc;
    if (local) {
        std::vector<ProjMapPoint*> v;
        for (auto& p : pts) v.push_back(p.get());
        v[1] = nullptr;
        pts[2]->bad = true;
        pts[3]->mnLastFrameSeen = cur.mnId;
        rc = OrbMatcherHip::SearchLocalPoints(cur, v, 3.f, 0.8f, &n_matches);
    } else {
        make_frame(last, 2, 6);
        for (int i = 0; i < 6; ++i) last.mvpMapPoints[i] = pts[i].get();
        last.mvpMapPoints[1] = nullptr;
        last.mvbOutlier[2] = true;
        pts[4]->bad = true;
        rc = OrbMatcherHip::SearchByProjection(cur, last, 7.f, false, true, &n_matches);
    }
    std::printf("status %d\nn_matches %d\n", rc, n_matches);
    for (auto& p : pts)
        std::printf("point %lu %d %.9g %.9g %.9g %d %.9g %d\n", p->mnId, p->mbTrackInView ? 1 : 0, p->mTrackProjX, p->mTrackProjY, p->mTrackProjXR,
                    p->mnTrackScaleLevel, p->mTrackViewCos, p->visible);
    std::printf("slots");
    for (ProjMapPoint* p : cur.mvpMapPoints) std::printf(" %ld", p ? (long)p->mnId : -1L);
    std::printf("\n");
    return 0;
}
