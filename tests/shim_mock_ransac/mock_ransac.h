// mock_ransac.h -- the stand-in map types of tests/shim_mock_sim3/mock_orbslam.h plus the one member Sim3Solver's constructor
// reads that they lack: KeyFrame::mvLevelSigma2 (src/Sim3Solver.cc:84-85).  Sim3SolverHip::FindBatch is a template on the key
// frame type, so a derived stand-in is enough.  TEST STAND-INS, as there.
#pragma once
#include "../shim_mock_sim3/mock_orbslam.h"

namespace ORB_SLAM2 {
class RansacKeyFrame : public KeyFrame {
public:
    std::vector<float> mvLevelSigma2;
};
}  // namespace ORB_SLAM2
