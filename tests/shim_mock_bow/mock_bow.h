// mock_bow.h -- the stand-in map types of tests/shim_mock_search/mock_search.h plus what ORBmatcher::SearchByBoW reads that they
// lack: the key point's angle, the DBoW2::FeatureVector (a std::map<unsigned, std::vector<unsigned>>) of a key frame and of a
// frame, and the frame's descriptors and key points (include/Frame.h, KeyFrame.h of the reference).
// OrbMatcherHip::SearchByBoWBatch is a template on the frame types, so derived stand-ins are enough.  TEST STAND-INS, as there.
#pragma once
#include <map>
#include <vector>

#include "../shim_mock_search/mock_search.h"

namespace ORB_SLAM2 {
struct AngleKeyPoint { cv::Point2f pt; int octave; float angle; };        // cv::KeyPoint with the member SearchByBoW reads
typedef std::map<unsigned int, std::vector<unsigned int>> FeatureVector;

class BowKeyFrame : public SearchKeyFrame {
public:
    FeatureVector mFeatVec;
    std::vector<AngleKeyPoint> mvKeysUn;                                  // (hides the angle-less stand-in of the base)
};

class BowFrame {
public:
    int N = 0;
    FeatureVector mFeatVec;
    DescMat mDescriptors;
    std::vector<AngleKeyPoint> mvKeys;
};
}  // namespace ORB_SLAM2
