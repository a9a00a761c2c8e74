// mock_create_points.h -- the stand-in map types of tests/shim_mock_triangulation/mock_triangulation.h plus what
// LocalMapping::CreateNewMapPoints and KeyFrame::UnprojectStereo read that they lack: invfx, invfy, mb, mfScaleFactor, the DISTORTED
// key points mvKeys and mvDepth (include/KeyFrame.h of the reference).  OrbMatcherHip::CreateNewMapPointsBatch is a template on the
// key-frame type, so a derived stand-in is enough.  TEST STAND-INS, as there.
#pragma once
#include "../shim_mock_triangulation/mock_triangulation.h"

namespace ORB_SLAM2 {
class CreateKeyFrame : public TriKeyFrame {
public:
    float invfx = 0.f, invfy = 0.f, mb = 0.f, mfScaleFactor = 0.f;
    std::vector<cv::KeyPoint> mvKeys;
    std::vector<float> mvDepth;
};
}  // namespace ORB_SLAM2
