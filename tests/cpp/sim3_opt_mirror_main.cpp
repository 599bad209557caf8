// Instantiates slam-dynamic_amd/host/Optimizer.h's ORB_SLAM2::Optimizer::OptimizeSim3 with minimal key-frame and map-point types, so
// that the mirror's compile and link against the library are checked (tests/test_sim3_opt_mirror.py).  Run on a machine with a GPU it
// optimises one clean synthetic pair and prints the return value.
#include <cstdio>
#include <memory>
#include <vector>
#include "Optimizer.h"

struct KF;
struct MP {
    float X[3];
    int idx2;
    bool bad = false;
    bool isBad() const { return bad; }
    int GetIndexInKeyFrame(const KF*) const { return idx2; }
    const float* GetWorldPos() const { return X; }
};
struct Pose { float m[16]; };
struct KF {
    std::vector<std::shared_ptr<MP>> pts;
    std::vector<sd_keypoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2 = std::vector<float>(8, 1.0f);
    float fx = 500, fy = 500, cx = 320, cy = 240;
    Pose T = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    std::vector<std::shared_ptr<MP>> GetMapPointMatches() const { return pts; }
    Pose GetPose() const { return T; }
};

int main()
{
    KF k1, k2;
    std::vector<std::shared_ptr<MP>> matches;
    for (int i = 0; i < 40; i++) {                               // both cameras at the origin, S12 = identity: every point seen where it is
        auto p = std::make_shared<MP>();
        p->X[0] = (float)((i % 8) - 4); p->X[1] = (float)((i / 8) - 2); p->X[2] = 8.0f + (float)(i % 5);
        p->idx2 = i;
        sd_keypoint kp = {};
        kp.x = k1.fx * p->X[0] / p->X[2] + k1.cx; kp.y = k1.fy * p->X[1] / p->X[2] + k1.cy; kp.octave = i % 8;
        k1.pts.push_back(p); k1.mvKeysUn.push_back(kp); k2.pts.push_back(p); k2.mvKeysUn.push_back(kp);
        matches.push_back(p);
    }
    matches[3].reset();
    ORB_SLAM2::Sim3 S;
    S.t[0] = 0.05;
    const int n = ORB_SLAM2::Optimizer::OptimizeSim3(&k1, &k2, matches, S, 10.0f, false);
    printf("OptimizeSim3 = %d, t = %.6f %.6f %.6f, s = %.6f\n", n, S.t[0], S.t[1], S.t[2], S.s);
    return n == 39 ? 0 : 1;
}
