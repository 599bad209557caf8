// Header-only mirror of ORB_SLAM2::Optimizer::PoseOptimization (include/Optimizer.h, src/Optimizer.cc:239-451) over the C ABI
// (sd_pose_optimize_host, include/sd_frontend.h): same signature, same return value, same effect on the frame.  Templated on the frame
// type like host/Frame.h; FrameT provides the Frame members the reference reads and writes:
//   N, mvpMapPoints[i] (pointer-like, NULL = no match; ->GetWorldPos() returns a 3-vector indexable with [k]), mvKeysUn[i] (sd_keypoint
//   layout: x, y, octave), mvuRight[i], mvInvLevelSigma2[octave], fx, fy, cx, cy, mbf, mTcw (a 4x4 row-major f32 pose with member m[16],
//   as sdfe::Pose), mvbOutlier[i], SetPose(const decltype(mTcw)&).
// Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241) likewise, over sd_sim3_optimize_host.  KeyFrameT provides GetMapPointMatches()
// (a vector of pointer-like map points), mvKeysUn[i], mvInvLevelSigma2[octave], fx, fy, cx, cy and GetPose() (a row-major 4x4 f32 pose
// with member m[16]); a map point provides isBad(), GetIndexInKeyFrame(pKF) and GetWorldPos().  g2oS12 is an ORB_SLAM2::Sim3 below
// (g2o::Sim3's members: r as x y z w, t, s).  The prior crosses the ABI as the f32 R12 / t12 / s12 that LoopClosing.cc:323 builds it from.
// No OpenCV.  The solve runs on the current HIP device; errors throw std::runtime_error (the reference has no failure path).
#pragma once
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "sd_frontend.h"

namespace ORB_SLAM2 {

struct Sim3 { double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1; };       // g2o::Sim3: rotation (x y z w), translation, scale

class Optimizer {
public:
    template <class KeyFrameT, class MapPointPtr>
    static int OptimizeSim3(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointPtr>& vpMatches1, Sim3& g2oS12, const float th2,
                            const bool bFixScale)
    {
        // one correspondence per i that passes the `continue`s of :1101-1136, in i order
        const int N = (int)vpMatches1.size();
        const auto vpMapPoints1 = pKF1->GetMapPointMatches();
        std::vector<sd_sim3_opt_corr> corr;
        corr.reserve(N);
        for (int i = 0; i < N; i++) {
            if (!vpMatches1[i]) continue;
            const auto& pMP1 = vpMapPoints1[i];
            const auto& pMP2 = vpMatches1[i];
            const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (!pMP1 || pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
            const auto X1 = pMP1->GetWorldPos();
            const auto X2 = pMP2->GetWorldPos();
            const sd_keypoint& kpUn1 = pKF1->mvKeysUn[i];
            const sd_keypoint& kpUn2 = pKF2->mvKeysUn[i2];
            sd_sim3_opt_corr c;
            for (int k = 0; k < 3; k++) { c.xw1[k] = (float)X1[k]; c.xw2[k] = (float)X2[k]; }
            c.obs1[0] = kpUn1.x; c.obs1[1] = kpUn1.y; c.obs2[0] = kpUn2.x; c.obs2[1] = kpUn2.y;
            c.inv_sigma2_1 = pKF1->mvInvLevelSigma2[kpUn1.octave]; c.inv_sigma2_2 = pKF2->mvInvLevelSigma2[kpUn2.octave];
            c.tag = i;
            corr.push_back(c);
        }
        sd_sim3_opt_problem P;
        std::memset(&P, 0, sizeof(P));
        std::memcpy(P.Tcw1, pKF1->GetPose().m, sizeof(P.Tcw1));
        std::memcpy(P.Tcw2, pKF2->GetPose().m, sizeof(P.Tcw2));
        P.fx1 = pKF1->fx; P.fy1 = pKF1->fy; P.cx1 = pKF1->cx; P.cy1 = pKF1->cy;
        P.fx2 = pKF2->fx; P.fy2 = pKF2->fy; P.cx2 = pKF2->cx; P.cy2 = pKF2->cy;
        {
            const double x = g2oS12.q[0], y = g2oS12.q[1], z = g2oS12.q[2], w = g2oS12.q[3];
            const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                                 2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
            for (int k = 0; k < 9; k++) P.R12[k] = (float)R[k];
            for (int k = 0; k < 3; k++) P.t12[k] = (float)g2oS12.t[k];
            P.s12 = (float)g2oS12.s;
        }
        P.th2 = th2; P.fix_scale = bFixScale ? 1 : 0;
        const int32_t off[2] = {0, (int32_t)corr.size()};
        std::vector<uint8_t> state(corr.size() + 1, 0);
        sd_sim3_opt_result res;
        const int rc = sd_sim3_optimize_host(1, off, corr.data(), &P, &res, state.data());
        if (rc != SD_OK) throw std::runtime_error(std::string("Optimizer::OptimizeSim3: ") + sd_last_error());
        for (size_t k = 0; k < corr.size(); k++)
            if (state[k]) vpMatches1[corr[k].tag] = MapPointPtr();   // both checks set the match to NULL, also on the `return 0` path
        if (res.written) {                                           // g2oS12 = vSim3_recov->estimate()
            for (int k = 0; k < 4; k++) g2oS12.q[k] = res.q[k];
            for (int k = 0; k < 3; k++) g2oS12.t[k] = res.t[k];
            g2oS12.s = res.s;
        }
        return res.ret;
    }

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
