// mock_fuse.h -- the stand-in map types of tests/shim_mock_search/mock_search.h plus what ORBmatcher::Fuse reads and writes that
// they lack (include/KeyFrame.h, MapPoint.h of the reference): the map point's normal, IsInKeyFrame, Observations, AddObservation
// and Replace; the key frame's camera centre, GetMapPoint, AddMapPoint and GetMapPoints.  OrbMatcherHip::FuseBatch is a template on
// both types, so derived stand-ins are enough.  Replace is written from what it means for a map: the survivor takes over every
// slot the dying point holds, unless it is observed in that key frame already (the slot is emptied then); the dying point is bad
// afterwards and observes nothing (tests/fuse_oracle.py, MapModel, says the same in Python).  TEST STAND-INS, as there.
#pragma once
#include <set>

#include "../shim_mock_search/mock_search.h"

namespace ORB_SLAM2 {
class FuseKeyFrame;

class FuseMapPoint : public SearchMapPoint {
public:
    cv::Mat nrm;
    cv::Mat GetNormal() { return nrm.clone(); }
    bool IsInKeyFrame(KeyFrame* k) { return obs.count(k) != 0; }
    int Observations() { return (int)obs.size(); }
    void AddObservation(KeyFrame* k, size_t idx) { obs[k] = idx; }
    inline void Replace(FuseMapPoint* survivor);
};

class FuseKeyFrame : public SearchKeyFrame {
public:
    std::vector<FuseMapPoint*> mvp;
    cv::Mat Ow;
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    FuseMapPoint* GetMapPoint(size_t idx) { return mvp[idx]; }
    void AddMapPoint(FuseMapPoint* p, size_t idx) { mvp[idx] = p; }
    std::set<FuseMapPoint*> GetMapPoints() {
        std::set<FuseMapPoint*> s;
        for (FuseMapPoint* p : mvp)
            if (p && !p->isBad()) s.insert(p);
        return s;
    }
};

inline void FuseMapPoint::Replace(FuseMapPoint* survivor) {
    if (survivor == this) return;
    const std::map<KeyFrame*, size_t> mine = obs;
    obs.clear();
    bad = true;
    for (const auto& e : mine) {
        FuseKeyFrame* k = static_cast<FuseKeyFrame*>(e.first);
        if (survivor->IsInKeyFrame(k)) k->mvp[e.second] = nullptr;
        else { k->mvp[e.second] = survivor; survivor->AddObservation(k, e.second); }
    }
}
}  // namespace ORB_SLAM2
