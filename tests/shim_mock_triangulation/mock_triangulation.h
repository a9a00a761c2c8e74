// mock_triangulation.h -- the stand-in map types of tests/shim_mock_bow/mock_bow.h plus what ORBmatcher::SearchForTriangulation
// reads that they lack: the key frame's mvLevelSigma2 and GetCameraCenter() (include/KeyFrame.h of the reference).
// OrbMatcherHip::SearchForTriangulationBatch is a template on the key-frame type, so a derived stand-in is enough.
// TEST STAND-INS, as there.
#pragma once
#include "../shim_mock_bow/mock_bow.h"

namespace ORB_SLAM2 {
class TriKeyFrame : public BowKeyFrame {
public:
    std::vector<float> mvLevelSigma2;
    cv::Mat Ow;
    cv::Mat GetCameraCenter() { return Ow.clone(); }
};
}  // namespace ORB_SLAM2
