// Header-only mirror of ORB_SLAM2::Optimizer::PoseOptimization (include/Optimizer.h, src/Optimizer.cc:239-451) over the C ABI
// (sd_pose_optimize_host, include/sd_frontend.h): same signature, same return value, same effect on the frame.  Templated on the frame
// type like host/Frame.h; FrameT provides the Frame members the reference reads and writes:
//   N, mvpMapPoints[i] (pointer-like, NULL = no match; ->GetWorldPos() returns a 3-vector indexable with [k]), mvKeysUn[i] (sd_keypoint
//   layout: x, y, octave), mvuRight[i], mvInvLevelSigma2[octave], fx, fy, cx, cy, mbf, mTcw (a 4x4 row-major f32 pose with member m[16],
//   as sdfe::Pose), mvbOutlier[i], SetPose(const decltype(mTcw)&).
// No OpenCV.  The solve runs on the current HIP device; errors throw std::runtime_error (the reference has no failure path).
#pragma once
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "sd_frontend.h"

namespace ORB_SLAM2 {

class Optimizer {
public:
    template <class FrameT>
    static int PoseOptimization(FrameT* pFrame)
    {
        // one edge per matched keypoint, in keypoint order (the edges' insertion order, Optimizer.cc:279-356)
        const int N = pFrame->N;
        std::vector<sd_pose_edge> edges;
        edges.reserve(N);
        for (int i = 0; i < N; i++) {
            const auto& pMP = pFrame->mvpMapPoints[i];
            if (!pMP) continue;
            const auto Xw = pMP->GetWorldPos();
            const sd_keypoint& kpUn = pFrame->mvKeysUn[i];
            sd_pose_edge e;
            e.xw[0] = (float)Xw[0]; e.xw[1] = (float)Xw[1]; e.xw[2] = (float)Xw[2];
            e.u = kpUn.x; e.v = kpUn.y; e.ur = pFrame->mvuRight[i];
            e.inv_sigma2 = pFrame->mvInvLevelSigma2[kpUn.octave];
            e.kp_index = i;
            edges.push_back(e);
        }
        const int32_t off[2] = {0, (int32_t)edges.size()};
        sd_camera cam;
        std::memset(&cam, 0, sizeof(cam));
        cam.fx = pFrame->fx; cam.fy = pFrame->fy; cam.cx = pFrame->cx; cam.cy = pFrame->cy; cam.mbf = pFrame->mbf;
        float Tcw[16];
        std::memcpy(Tcw, pFrame->mTcw.m, sizeof(Tcw));
        std::vector<uint8_t> outlier(edges.size() + 1, 0);
        int32_t nGood = 0;
        const int rc = sd_pose_optimize_host(1, off, edges.data(), &cam, Tcw, outlier.data(), &nGood);
        if (rc != SD_OK) throw std::runtime_error(std::string("Optimizer::PoseOptimization: ") + sd_last_error());
        for (size_t k = 0; k < edges.size(); k++) pFrame->mvbOutlier[edges[k].kp_index] = outlier[k] != 0;
        if (edges.size() < 3) return 0;                          // nInitialCorrespondences < 3: the pose is left as it was
        auto pose = pFrame->mTcw;
        std::memcpy(pose.m, Tcw, sizeof(Tcw));
        pFrame->SetPose(pose);
        return nGood;
    }
};

}  // namespace ORB_SLAM2
