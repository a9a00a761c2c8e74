// mock_projection_kf.h -- stand-ins for what the relocalisation and Sim3 overloads of OrbMatcherHip::SearchByProjection read of a
// KeyFrame (include/KeyFrame.h of the reference), on top of the stand-in frame and point of tests/shim_mock_projection/: a key frame
// whose undistorted key points have an angle and whose slots hold the frame's point type.  TEST STAND-INS, as there.
#pragma once
#include "../shim_mock_projection/mock_projection.h"

namespace ORB_SLAM2 {
class ProjKeyFrame : public FuseKeyFrame {
public:
    std::vector<ProjKeyPoint> mvKeysUn;            // hides the base's, which has no angle
    std::vector<ProjMapPoint*> pts;
    std::vector<ProjMapPoint*> GetMapPointMatches() { return pts; }
};
}  // namespace ORB_SLAM2
