// mock_place.h -- the stand-in map types of tests/shim_mock_sim3/mock_orbslam.h plus what KeyFrameDatabase reads that they lack:
// the DBoW2::BowVector (a std::map<unsigned, double>) of a key frame and of a frame, GetConnectedKeyFrames() and
// GetBestCovisibilityKeyFrames(N) (include/KeyFrame.h, Frame.h of the reference).  KeyFrameDatabaseHip is a template on the
// key-frame type, so a derived stand-in is enough.  TEST STAND-INS, as there.
#pragma once
#include <map>
#include <set>
#include <vector>

#include "../shim_mock_sim3/mock_orbslam.h"

namespace ORB_SLAM2 {
typedef std::map<unsigned int, double> BowVector;

class PlaceKeyFrame : public KeyFrame {
public:
    BowVector mBowVec;
    std::vector<PlaceKeyFrame*> ordered;                  // mvpOrderedConnectedKeyFrames
    int n_best_calls = 0;
    std::set<PlaceKeyFrame*> GetConnectedKeyFrames() { return std::set<PlaceKeyFrame*>(ordered.begin(), ordered.end()); }
    std::vector<PlaceKeyFrame*> GetVectorCovisibleKeyFrames() { return ordered; }      // (hides the base's)
    std::vector<PlaceKeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
        ++n_best_calls;
        return (int)ordered.size() < N ? ordered : std::vector<PlaceKeyFrame*>(ordered.begin(), ordered.begin() + N);
    }
};

class PlaceFrame {
public:
    long unsigned int mnId = 0;
    BowVector mBowVec;
};
}  // namespace ORB_SLAM2
