// mock_projection.h -- stand-ins for what OrbMatcherHip::SearchLocalPoints and OrbMatcherHip::SearchByProjection read and write of a
// Frame and of a MapPoint (include/Frame.h, MapPoint.h of the reference), on top of the stand-in map types of
// tests/shim_mock_fuse/mock_fuse.h, which the rest of include/qsp_optimizer_shim.h needs.  Both members are templates on the frame
// and the point type, so a frame of its own is enough: unlike the Frame of the shared stand-ins it has mvKeys beside mvKeysUn, key
// points with an angle, descriptors, the grid and pyramid members, mb, the camera centre and an id.  Observations() is a number the
// test sets (0: a temporal point, which does not block).  TEST STAND-INS, as there.
#pragma once
#include "../shim_mock_fuse/mock_fuse.h"

#define FRAME_GRID_ROWS 48
#define FRAME_GRID_COLS 64

namespace ORB_SLAM2 {
struct ProjKeyPoint { cv::Point2f pt; int octave; float angle; };

class ProjMapPoint : public FuseMapPoint {
public:
    bool mbTrackInView = false;
    float mTrackProjX = -1.f, mTrackProjY = -1.f, mTrackProjXR = -1.f, mTrackViewCos = -1.f;
    int mnTrackScaleLevel = -1;
    long unsigned int mnLastFrameSeen = 0;
    int n_obs = 0, visible = 0;
    int Observations() { return n_obs; }
    void IncreaseVisible(int n = 1) { visible += n; }
};

class ProjFrame {
public:
    int N = 0;
    long unsigned int mnId = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0, mb = 0;
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0, mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    int mnScaleLevels = 0;
    float mfLogScaleFactor = 0;
    std::vector<float> mvScaleFactors;
    cv::Mat mTcw, Ow;
    std::vector<ProjKeyPoint> mvKeys, mvKeysUn;
    DescMat mDescriptors;
    std::vector<float> mvuRight;
    std::vector<ProjMapPoint*> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    cv::Mat GetCameraCenter() { return Ow.clone(); }
};
}  // namespace ORB_SLAM2
