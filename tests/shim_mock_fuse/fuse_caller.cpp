// fuse_caller.cpp -- stand-alone caller of both OrbMatcherHip::FuseBatch overloads over the stand-in map types of this directory and
// the stub of qsp_fuse_batch (tests/test_shim_fuse.py builds and runs it; never loaded into Python).  The MAP of a scene comes from
// the file named on the command line; what a key frame and a point hold beside that is procedural (make_kf, make_point), so that
// the test can restate it.  Scene file, one record per line:
//   mode pose|sim3 / th <float> / callback 0|1 / kf <slots> / pt <bad> (or `pt null`) / obs <point> <kf> <slot> / targets <kf> ...
// Prints the status, vnFused, n_stale, the replacements, the calls of after_target and the map as it is afterwards.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "mock_fuse.h"
#include "qsp_optimizer_shim.h"

using namespace ORB_SLAM2;

static void make_kf(FuseKeyFrame& kf, int k, int n) {
    kf.mnId = k;
    kf.mDescriptors.rows = n;
    kf.fx = 500.f + k; kf.fy = 510.f + k; kf.cx = 320.f + 0.5f * k; kf.cy = 240.f - 0.25f * k; kf.mbf = 40.f + k;
    kf.mnScaleLevels = 4;
    kf.mfLogScaleFactor = 0.2f + 0.01f * k;
    for (int l = 0; l < 4; ++l) {
        kf.mvScaleFactors.push_back(1.f + 0.25f * l + 0.01f * k);
        kf.mvInvLevelSigma2.push_back(1.f / (2.f + l + 0.5f * k));
    }
    kf.mnMinX = -k; kf.mnMaxX = 640 + k; kf.mnMinY = 0; kf.mnMaxY = 480;
    kf.mnGridCols = 64; kf.mnGridRows = 48;
    kf.mfGridElementWidthInv = 64.f / (float)(kf.mnMaxX - kf.mnMinX);
    kf.mfGridElementHeightInv = 48.f / 480.f;
    for (int j = 0; j < n; ++j) {
        kf.mvKeysUn.push_back(cv::KeyPoint{{1.5f * j + k, 2.25f * j - k}, (j + k) % 4});
        kf.mvuRight.push_back(j % 3 == 0 ? 5.f + j : -1.f);
        for (int b = 0; b < 32; ++b) kf.mDescriptors.d.push_back((unsigned char)(j * 7 + b * 3 + k));
    }
    kf.mvp.assign(n, nullptr);
    kf.Tcw = cv::Mat(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) kf.Tcw.at<float>(r, c) = (r == c ? 0.9f : 0.1f * (r - c)) + 0.01f * k;
        kf.Tcw.at<float>(r, 3) = 0.3f * r - 0.2f * k + 1.7f;
    }
    kf.Tcw.at<float>(3, 3) = 1.f;
    kf.Ow = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) kf.Ow.at<float>(r) = 0.37f * (r + 1) - 0.11f * k;
}

static void make_point(FuseMapPoint& p, int i, bool bad) {
    p.mnId = i;
    p.bad = bad;
    p.pos = cv::Mat(3, 1, CV_32F);
    p.nrm = cv::Mat(3, 1, CV_32F);
    const float X[3] = {0.1f * i + 1.f, 0.2f * i - 1.f, 0.05f * i + 3.f}, N[3] = {0.01f * i, 0.02f * i, 1.f - 0.001f * i};
    for (int r = 0; r < 3; ++r) { p.pos.at<float>(r) = X[r]; p.nrm.at<float>(r) = N[r]; }
    p.mfMaxDistance = 10.f + i;
    p.mfMinDistance = 1.f + 0.1f * i;
    p.desc.rows = 1;
    for (int b = 0; b < 32; ++b) p.desc.d.push_back((unsigned char)(i * 5 + b));
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string line, mode = "pose";
    float th = 3.f;
    bool callback = false;
    std::vector<std::unique_ptr<FuseKeyFrame>> kfs;
    std::vector<std::unique_ptr<FuseMapPoint>> owned;
    std::vector<FuseMapPoint*> points;
    std::vector<FuseKeyFrame*> targets;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string what;
        s >> what;
        if (what == "mode") s >> mode;
        else if (what == "th") s >> th;
        else if (what == "callback") s >> callback;
        else if (what == "kf") {
            int n; s >> n;
            kfs.emplace_back(new FuseKeyFrame());
            make_kf(*kfs.back(), (int)kfs.size() - 1, n);
        } else if (what == "pt") {
            std::string v; s >> v;
            if (v == "null") { points.push_back(nullptr); continue; }
            owned.emplace_back(new FuseMapPoint());
            make_point(*owned.back(), (int)points.size(), v == "1");
            points.push_back(owned.back().get());
        } else if (what == "obs") {
            int p, k, slot; s >> p >> k >> slot;
            points[p]->obs[kfs[k].get()] = slot;
            kfs[k]->mvp[slot] = points[p];
        } else if (what == "targets") {
            int k;
            while (s >> k) targets.push_back(kfs[k].get());
        }
    }
    std::vector<int> fused = {-4};                                      // sentinels: untouched on failure
    int n_stale = -5, st;
    std::vector<std::vector<FuseMapPoint*>> replace(1, std::vector<FuseMapPoint*>(1, nullptr));
    std::vector<size_t> called;
    if (mode == "pose") {
        st = OrbMatcherHip::FuseBatch(targets, points, th, fused, &n_stale);
    } else {
        std::vector<cv::Mat> vScw;
        for (FuseKeyFrame* kf : targets) {
            const float s = 1.5f + 0.25f * kf->mnId;
            cv::Mat S(4, 4, CV_32F);
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) S.at<float>(r, c) = s * kf->Tcw.at<float>(r, c);
            S.at<float>(3, 3) = 1.f;
            vScw.push_back(S);
        }
        // the caller's block between two targets: the key frame's point is replaced BY the loop point
        auto after = [&](size_t k) {
            called.push_back(k);
            if (!callback) return;
            for (size_t i = 0; i < points.size(); ++i)
                if (replace[k][i]) replace[k][i]->Replace(points[i]);
        };
        st = OrbMatcherHip::FuseBatch(targets, vScw, points, th, replace, fused, std::function<void(size_t)>(after), &n_stale);
    }
    std::printf("status %d\nfused", st);
    for (int f : fused) std::printf(" %d", f);
    std::printf("\nstale %d\ncalled", n_stale);
    for (size_t k : called) std::printf(" %zu", k);
    std::printf("\n");
    for (const auto& v : replace) {
        std::printf("replace");
        for (FuseMapPoint* p : v) std::printf(" %ld", p ? (long)p->mnId : -1L);
        std::printf("\n");
    }
    for (const auto& kf : kfs) {
        std::printf("slots");
        for (FuseMapPoint* p : kf->mvp) std::printf(" %ld", p ? (long)p->mnId : -1L);
        std::printf("\n");
    }
    for (FuseMapPoint* p : points) {
        if (!p) { std::printf("point null\n"); continue; }
        std::printf("point %d", p->bad ? 1 : 0);
        for (size_t k = 0; k < kfs.size(); ++k) {
            auto f = p->obs.find(kfs[k].get());
            if (f != p->obs.end()) std::printf(" %zu:%zu", k, f->second);
        }
        std::printf("\n");
    }
    return 0;
}
