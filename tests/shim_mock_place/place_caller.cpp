// place_caller.cpp -- stand-alone caller of KeyFrameDatabaseHip over the stand-in map types of this directory and the stub of the
// qsp_place_db calls (tests/test_shim_place_db.py builds and runs it; never loaded into Python).  The scene is procedural so that
// the test can restate it: key frames k = 0..5 with mnId 10 + k, words {k, k + 3, 2k + 7} inserted in DESCENDING order (the map
// sorts them), values (w + 1) / 64; key frame k's ordered covisibles are k + 1 ... k + 13 modulo 6 without k itself: 11 entries
// (with repeats), one more than GetBestCovisibilityKeyFrames(10) returns; key frame 2 is bad.
// Added in the order 3, 0, 2, 4, 1; key frame 2 is erased again, key frame 5 is never added.
// Modes: "loop" (given minimum score), "loop_ref" (DetectLoop's minimum), "reloc", "empty" (an empty database), "lifecycle".
#include <cstdio>
#include <cstring>
#include <vector>

#include "mock_place.h"
#include "qsp_optimizer_shim.h"

using namespace ORB_SLAM2;

static void print(const char* what, const std::vector<PlaceKeyFrame*>& v) {
    std::printf("%s", what);
    for (PlaceKeyFrame* p : v) std::printf(" %ld", (long)p->mnId);
    std::printf("\n");
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "loop";
    PlaceKeyFrame kf[6];
    for (int k = 0; k < 6; ++k) {
        kf[k].mnId = 10 + k;
        const int w[3] = {2 * k + 7, k + 3, k};
        for (int j = 0; j < 3; ++j) kf[k].mBowVec[(unsigned)w[j]] = (w[j] + 1) / 64.0;
        for (int d = 1; d <= 13; ++d)
            if ((k + d) % 6 != k) kf[k].ordered.push_back(&kf[(k + d) % 6]);
    }
    kf[2].bad = true;
    PlaceFrame F;
    F.mnId = 0;
    F.mBowVec[9] = 0.25; F.mBowVec[1] = 0.5; F.mBowVec[4] = 0.25;
    {
        KeyFrameDatabaseHip<PlaceKeyFrame> db;
        if (std::strcmp(mode, "empty") != 0) {
            int st = 0;
            for (int k : {3, 0, 2, 4, 1}) st |= db.add(&kf[k]);
            st |= db.erase(&kf[2]);
            st |= db.erase(&kf[5]);                                       // never added: nothing happens
            std::printf("status %d\n", st);
        }
        if (!std::strcmp(mode, "loop")) {
            kf[5].ordered.resize(2);                                      // connected to 10 and 11 only
            print("candidates", db.DetectLoopCandidates(&kf[5], 0.125f));
        } else if (!std::strcmp(mode, "loop_ref")) {
            kf[0].ordered = {&kf[2], &kf[5], &kf[1]};                     // a bad one, one the database does not know yet, a listed one
            print("candidates", db.DetectLoopCandidates(&kf[0]));
            print("again", db.DetectLoopCandidates(&kf[0]));              // key frame 15 is known by now: no second put
        } else if (!std::strcmp(mode, "reloc") || !std::strcmp(mode, "empty")) {
            print("candidates", db.DetectRelocalizationCandidates(&F));
        } else if (!std::strcmp(mode, "lifecycle")) {
            std::printf("status %d\n", db.add(&kf[5]));
            std::printf("status %d\n", db.clear());
            std::printf("status %d\n", db.add(&kf[1]));
            std::printf("status %d\n", db.add(&kf[1]));                   // a repeated add: no call, no failure
            print("candidates", db.DetectRelocalizationCandidates(&F));
        }
        std::printf("best_calls");
        for (int k = 0; k < 6; ++k) std::printf(" %d", kf[k].n_best_calls);
        std::printf("\nfailures %ld\n", qsp_shim::failure_count());
    }
    return 0;
}
