// Exercises slam-dynamic_amd/host/Optimizer.h (ORB_SLAM2::Optimizer::PoseOptimization mirror) on the GPU:
//   pose_mirror_main <in.bin> <out.bin>
// in.bin : int32 N, float cam[5] (fx fy cx cy mbf), float Tcw[16], then N records {int32 has_point; float xw[3]; float u, v, ur, inv_sigma2}
// out.bin: int32 return value, float Tcw[16], uint8 mvbOutlier[N]
#include <cstdio>
#include <cstdint>
#include <vector>
#include "Frame.h"
#include "Optimizer.h"

struct MapPointT {
    float X[3];
    const float* GetWorldPos() const { return X; }
};

struct FrameT {
    int N = 0;
    std::vector<const MapPointT*> mvpMapPoints;
    std::vector<sd_keypoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<bool> mvbOutlier;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    sdfe::Pose mTcw;
    void SetPose(const sdfe::Pose& T) { mTcw = T; }
};

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t n = 0;
    float cam[5];
    FrameT F;
    if (fread(&n, 4, 1, f) != 1 || fread(cam, 4, 5, f) != 5 || fread(F.mTcw.m, 4, 16, f) != 16) return 4;
    std::vector<MapPointT> points(n);
    F.N = n; F.mvpMapPoints.assign(n, nullptr); F.mvKeysUn.resize(n); F.mvuRight.resize(n); F.mvbOutlier.assign(n, true);
    F.fx = cam[0]; F.fy = cam[1]; F.cx = cam[2]; F.cy = cam[3]; F.mbf = cam[4];
    for (int i = 0; i < n; i++) {
        int32_t has = 0;
        float r[7];
        if (fread(&has, 4, 1, f) != 1 || fread(r, 4, 7, f) != 7) return 5;
        points[i].X[0] = r[0]; points[i].X[1] = r[1]; points[i].X[2] = r[2];
        if (has) F.mvpMapPoints[i] = &points[i];
        F.mvKeysUn[i] = sd_keypoint();
        F.mvKeysUn[i].x = r[3]; F.mvKeysUn[i].y = r[4]; F.mvKeysUn[i].octave = i % 8;
        F.mvuRight[i] = r[5];
        F.mvbOutlier[i] = !has;                  // untouched for keypoints without a map point
        if ((int)F.mvInvLevelSigma2.size() <= i % 8) F.mvInvLevelSigma2.resize(i % 8 + 1);
        F.mvInvLevelSigma2[i % 8] = r[6];
    }
    fclose(f);
    const int ret = ORB_SLAM2::Optimizer::PoseOptimization(&F);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 6;
    fwrite(&ret, 4, 1, o);
    fwrite(F.mTcw.m, 4, 16, o);
    for (int i = 0; i < n; i++) { const uint8_t b = F.mvbOutlier[i] ? 1 : 0; fwrite(&b, 1, 1, o); }
    fclose(o);
    return 0;
}
