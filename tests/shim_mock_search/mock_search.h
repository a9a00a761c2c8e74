// mock_search.h -- the stand-in map types of tests/shim_mock_sim3/mock_orbslam.h plus what ORBmatcher::SearchBySim3 reads that they
// lack: the key frame's descriptors, image bounds, grid and scale members (include/KeyFrame.h of the reference) and the map
// point's descriptor and distance getters (include/MapPoint.h).  OrbMatcherHip::SearchBySim3Batch is a template on both types, so
// derived stand-ins are enough.  TEST STAND-INS, as there.
#pragma once
#include <cstdint>

#include "../shim_mock_sim3/mock_orbslam.h"

namespace ORB_SLAM2 {
struct DescMat {                                   // a CV_8U cv::Mat: rows of 32 bytes
    int rows = 0;
    std::vector<unsigned char> d;
    DescMat row(int i) const { DescMat r; r.rows = 1; r.d.assign(d.begin() + 32 * i, d.begin() + 32 * (i + 1)); return r; }
    template <typename T> const T& at(int r, int c) const { return d[32 * r + c]; }
};

class SearchMapPoint : public MapPoint {
public:
    float mfMaxDistance = 0.f, mfMinDistance = 0.f;
    DescMat desc;
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    DescMat GetDescriptor() { return desc; }
};

class SearchKeyFrame : public KeyFrame {
public:
    DescMat mDescriptors;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0, mnGridCols = 0, mnGridRows = 0, mnScaleLevels = 0;
    float mfGridElementWidthInv = 0.f, mfGridElementHeightInv = 0.f, mfLogScaleFactor = 0.f;
    std::vector<float> mvScaleFactors;
    std::vector<SearchMapPoint*> slots;
    std::vector<SearchMapPoint*> GetMapPointMatches() { return slots; }
};
}  // namespace ORB_SLAM2
