// projection_kf_caller.cpp -- stand-alone caller of the relocalisation and Sim3 overloads of OrbMatcherHip::SearchByProjection over
// the stand-in types of this directory and the stub of qsp_search_by_projection_kf (tests/test_shim_search_projection_kf.py builds
// and runs it; never loaded into Python).  Everything a frame, a key frame and a point hold is procedural, so that the test can
// restate it.  Usage: projection_kf_caller reloc|sim3.
// reloc: the current frame is frame 1 with 7 key points; its slot 2 holds an observed point (id 100) and its slot 4 a point with
// ZERO observations (id 101).  The key frame is key frame 2 with 6 slots holding ids 0..5 with 1 null, 2 bad and 3 in sAlreadyFound.
// sim3: the key frame is key frame 1 with 7 key points, Scw = 2 [R | t] of a procedural pose; vpMatched holds id 3 in slot 2 and id
// 101 (zero observations) in slot 4; vpPoints are ids 0..5 with 1 null, 2 bad, 3 already found.
// Prints the status, n_matches and the slots (of the current frame / of vpMatched) as point ids.
#include <cstdio>
#include <cstring>
#include <memory>
#include <set>
#include <vector>

#include "mock_projection_kf.h"
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
}

static void make_key_frame(ProjKeyFrame& F, int k, int n) {
    F.mnId = 20 + k;
    F.fx = 400.f + k; F.fy = 410.f + k; F.cx = 300.f + 0.5f * k; F.cy = 200.f - 0.25f * k; F.mbf = 30.f + k;
    F.mnMinX = -3 - k; F.mnMaxX = 650 + k; F.mnMinY = -4; F.mnMaxY = 490;
    F.mnGridCols = 60 + k; F.mnGridRows = 40 + k;
    F.mfGridElementWidthInv = (float)F.mnGridCols / (float)(F.mnMaxX - F.mnMinX);
    F.mfGridElementHeightInv = (float)F.mnGridRows / (float)(F.mnMaxY - F.mnMinY);
    F.mnScaleLevels = 5;
    F.mfLogScaleFactor = 0.3f + 0.01f * k;
    for (int l = 0; l < 5; ++l) F.mvScaleFactors.push_back(1.f + 0.5f * l + 0.01f * k);
    F.mDescriptors.rows = n;
    for (int j = 0; j < n; ++j) {
        F.mvKeysUn.push_back(ProjKeyPoint{{2.5f * j + k, 3.25f * j - k}, (j + k) % 5, 7.f * j + k});
        for (int b = 0; b < 32; ++b) F.mDescriptors.d.push_back((unsigned char)(j * 11 + b * 5 + k));
    }
    F.pts.assign(n, nullptr);
    F.Tcw = cv::Mat(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) F.Tcw.at<float>(r, c) = (r == c ? 0.8f : 0.2f * (r - c)) + 0.01f * k;
        F.Tcw.at<float>(r, 3) = 0.4f * r - 0.1f * k + 1.1f;
    }
    F.Tcw.at<float>(3, 3) = 1.f;
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
    const bool reloc = std::strcmp(argv[1], "reloc") == 0;
    std::vector<std::unique_ptr<ProjMapPoint>> pts;
    for (int i = 0; i < 6; ++i) { pts.emplace_back(new ProjMapPoint); make_point(*pts.back(), i); }
    ProjMapPoint held, temporal;
    make_point(held, 100); held.n_obs = 2;
    make_point(temporal, 101); temporal.n_obs = 0;
    pts[2]->bad = true;
    int n_matches = -5, rc;
    std::vector<ProjMapPoint*> slots;
    if (reloc) {
        ProjFrame cur;
        make_frame(cur, 1, 7);
        cur.mvpMapPoints[2] = &held;
        cur.mvpMapPoints[4] = &temporal;
        ProjKeyFrame kf;
        make_key_frame(kf, 2, 6);
        for (int i = 0; i < 6; ++i) kf.pts[i] = pts[i].get();
        kf.pts[1] = nullptr;
        std::set<ProjMapPoint*> found;
        found.insert(pts[3].get());
        rc = OrbMatcherHip::SearchByProjection(cur, &kf, found, 10.f, 100, true, &n_matches);
        slots = cur.mvpMapPoints;
    } else {
        ProjKeyFrame kf;
        make_key_frame(kf, 1, 7);
        cv::Mat Scw(4, 4, CV_32F);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) Scw.at<float>(r, c) = 2.f * ((r == c ? 0.6f : 0.3f * (c - r)) + 0.05f * r);
            Scw.at<float>(r, 3) = 2.f * (0.7f * r - 0.4f);
        }
        Scw.at<float>(3, 3) = 1.f;
        std::vector<ProjMapPoint*> v, matched(7, nullptr);
        for (auto& p : pts) v.push_back(p.get());
        v[1] = nullptr;
        matched[2] = pts[3].get();
        matched[4] = &temporal;
        rc = OrbMatcherHip::SearchByProjection(&kf, Scw, v, matched, 10, &n_matches);
        slots = matched;
    }
    std::printf("status %d\nn_matches %d\n", rc, n_matches);
    std::printf("slots");
    for (ProjMapPoint* p : slots) std::printf(" %ld", p ? (long)p->mnId : -1L);
    std::printf("\n");
    return 0;
}
