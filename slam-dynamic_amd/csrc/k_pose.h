// Optimizer::PoseOptimization (src/Optimizer.cc:239-451) with the vendored g2o's Levenberg-Marquardt for
// many independent frames in one launch: one 256-thread workgroup per problem runs all 4 rounds x optimize(10) on the device.
// Per-edge work is strided over the workgroup; the sums the algorithm needs (the 21 + 6 distinct entries of H and b with the
// active robust chi2 per iteration, the chi2 alone per LM trial, nBad per round) are reduced by wave64 xor-butterflies and a
// fixed-order sum of the four wave partials in LDS, so every lane holds the same bits and a problem's result does not depend on
// which problems share the launch.  Everything that follows a reduction (the 6x6 pivoted LDL^T, SE3 exp / compose /
// renormalise, the LM bookkeeping) is computed uniformly by every lane.  f64 throughout; inputs f32 as the reference's.
// The arithmetic shared with k_ba.h and k_sim3_opt.h (quaternion, edge error, Huber, LDL^T, reductions) is sd_g2o_math.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sd_frontend.h"
#include "sd_plan.h"
#include "sd_g2o_math.h"

#define SD_POSE_THREADS 256

struct SdPoseArgs {
    const sd_pose_edge* edges;
    const int* first;         // problem q: edges [first[q], last[q])
    const int* last;
    const sd_camera* cam;     // [p]: camera of workgroup p
    float* Tcw;               // [q][16] row-major, in / out
    uint8_t* outlier;         // [edge] mvbOutlier
    int* nGood;               // [q] the return value
    const int* map;           // nullable: problem of workgroup p = map[p]
};

namespace sdpose {

typedef sd_se3 T;

__device__ __forceinline__ T compose(const T& a, const T& b)       // SE3Quat::operator*
{
    T r;
    double p0, p1, p2;
    sd_quat_rot(a.r, b.t0, b.t1, b.t2, p0, p1, p2);
    r.t0 = a.t0 + p0; r.t1 = a.t1 + p1; r.t2 = a.t2 + p2;
    r.r = sd_quat_mul(a.r, b.r);
    sd_quat_renorm(r.r);
    return r;
}

__device__ __forceinline__ T expmap(const double (&u)[6])           // SE3Quat::exp
{
    const double w0 = u[0], w1 = u[1], w2 = u[2];
    const double th = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    // Omega = skew(w); Omega^2 = w w^T - |w|^2 I, formed as the 3x3 product the reference takes
    const double O[3][3] = {{0, -w2, w1}, {w2, 0, -w0}, {-w1, w0, 0}};
    double O2[3][3], R[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    if (th < 0.00001) {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) { R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j]; V[i][j] = R[i][j]; }
    } else {
        const double s = sin(th), c = cos(th);
        const double a = s / th, b = (1 - c) / (th * th), g = (th - s) / pow(th, 3);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                R[i][j] = ((i == j ? 1.0 : 0.0) + a * O[i][j]) + b * O2[i][j];
                V[i][j] = ((i == j ? 1.0 : 0.0) + b * O[i][j]) + g * O2[i][j];
            }
    }
    T r;
    r.r = sd_quat_of(R);
    r.t0 = V[0][0] * u[3] + V[0][1] * u[4] + V[0][2] * u[5];
    r.t1 = V[1][0] * u[3] + V[1][1] * u[4] + V[1][2] * u[5];
    r.t2 = V[2][0] * u[3] + V[2][1] * u[4] + V[2][2] * u[5];
    sd_quat_renorm(r.r);
    return r;
}

}  // namespace sdpose

__global__ void __launch_bounds__(SD_POSE_THREADS) k_pose_optimize(SdPoseArgs A)
{
    using namespace sdpose;
    __shared__ double red[4 * 28];
    const int q = A.map ? A.map[blockIdx.x] : blockIdx.x;
    const int e0 = A.first[q], e1 = A.last[q], nE = e1 - e0;
    const int tid = threadIdx.x;
    const sd_pose_edge* __restrict__ E = A.edges;
    uint8_t* __restrict__ out = A.outlier;
    for (int i = e0 + tid; i < e1; i += SD_POSE_THREADS) out[i] = 0;     // mvbOutlier[i] = false for every edge
    if (nE < 3) {                                                        // nInitialCorrespondences < 3: return 0, pose untouched
        if (tid == 0) A.nGood[q] = 0;
        return;
    }
    __syncthreads();
    const sd_camera C0 = A.cam[blockIdx.x];
    const sd_se3_cam c = {(double)C0.fx, (double)C0.fy, (double)C0.cx, (double)C0.cy, (double)C0.mbf};
    float* Tq = A.Tcw + (size_t)q * 16;
    const T pose0 = sd_se3_of(Tq);                                       // Converter::toSE3Quat(pFrame->mTcw)
    const double dM = (double)(float)sqrt(5.991), dS = (double)(float)sqrt(7.815);
    bool robust = true;
    int nBad = 0, nBadPrev = 0;
    T est = pose0;
    for (int round = 0; round < 4; round++) {
        est = pose0;                                                     // every round restarts from the input pose
        T errPose = est;                                                 // pose of the last computeActiveErrors (the edges' cached _error)
        if (nE - nBadPrev > 0) {                                         // else: no active vertex, optimize() returns -1
            double lambda = 0.0, xs[6] = {0, 0, 0, 0, 0, 0};
            int ni = 2, nStop = 0;
            for (int it = 0; it < 10; it++) {
                // solve(it): computeActiveErrors + activeRobustChi2 + buildSystem at est
                double v[28];
#pragma unroll
                for (int k = 0; k < 28; k++) v[k] = 0.0;
                for (int i = e0 + tid; i < e1; i += SD_POSE_THREADS) {
                    if (out[i]) continue;                                // level 1
                    const sd_pose_edge ed = E[i];
                    double rr[3], p[3];
                    const int D = sd_se3_error(est, c, ed.xw[0], ed.xw[1], ed.xw[2], ed.u, ed.v, ed.ur, rr, p);
                    const double w = (double)ed.inv_sigma2, c2 = sd_se3_chi2(rr, D, w);
                    double rho0 = c2, rho1 = 1.0;
                    if (robust) sd_huber(c2, D == 2 ? dM : dS, rho0, rho1);
                    v[27] += rho0;
                    // linearizeOplus (types_six_dof_expmap.cpp:266-364)
                    const double x = p[0], y = p[1], iz = 1.0 / p[2], iz2 = iz * iz;
                    double J[3][6];
                    J[0][0] = x * y * iz2 * c.fx; J[0][1] = -(1 + (x * x * iz2)) * c.fx; J[0][2] = y * iz * c.fx;
                    J[0][3] = -iz * c.fx; J[0][4] = 0; J[0][5] = x * iz2 * c.fx;
                    J[1][0] = (1 + y * y * iz2) * c.fy; J[1][1] = -x * y * iz2 * c.fy; J[1][2] = -x * iz * c.fy;
                    J[1][3] = 0; J[1][4] = -iz * c.fy; J[1][5] = y * iz2 * c.fy;
                    J[2][0] = J[0][0] - c.bf * y * iz2; J[2][1] = J[0][1] + c.bf * x * iz2; J[2][2] = J[0][2];
                    J[2][3] = J[0][3]; J[2][4] = 0; J[2][5] = J[0][5] - c.bf * iz2;
                    const double wo = robust ? rho1 * w : w;             // robustInformation: rho[1] * information
#pragma unroll
                    for (int i2 = 0; i2 < 6; i2++)
#pragma unroll
                        for (int j = 0; j <= i2; j++) {
                            double h = (J[0][i2] * wo) * J[0][j] + (J[1][i2] * wo) * J[1][j];
                            if (D == 3) h = h + (J[2][i2] * wo) * J[2][j];
                            v[i2 * (i2 + 1) / 2 + j] += h;
                        }
#pragma unroll
                    for (int i2 = 0; i2 < 6; i2++) {
                        double g = robust ? ((rho1 * J[0][i2]) * w) * rr[0] + ((rho1 * J[1][i2]) * w) * rr[1]
                                          : (J[0][i2] * w) * rr[0] + (J[1][i2] * w) * rr[1];
                        if (D == 3) g = g + (robust ? ((rho1 * J[2][i2]) * w) * rr[2] : (J[2][i2] * w) * rr[2]);
                        v[21 + i2] += g;
                    }
                }
                sd_block_sum<28>(v, red);
                errPose = est;
                double H[21], b[6];
#pragma unroll
                for (int k = 0; k < 21; k++) H[k] = v[k];
#pragma unroll
                for (int k = 0; k < 6; k++) b[k] = -v[21 + k];            // b -= J^T W e
                double currentChi = v[27];
                const double iniChi = currentChi;
                if (it == 0) {                                           // computeLambdaInit: tau * max |diag H|
                    double md = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; j++) md = fmax(fabs(H[j * (j + 1) / 2 + j]), md);
                    lambda = 1e-5 * md; ni = 2; nStop = 0;
                }
                double rho = 0.0;
                int qmax = 0;
                do {
                    const T backup = est;
                    const bool ok2 = sd_ldlt_solve<6>(H, b, lambda, xs);
                    est = compose(expmap(xs), est);                      // VertexSE3Expmap::oplusImpl
                    double tc[1] = {0.0};
                    for (int i = e0 + tid; i < e1; i += SD_POSE_THREADS) {
                        if (out[i]) continue;
                        const sd_pose_edge ed = E[i];
                        double rr[3], p[3];
                        const int D = sd_se3_error(est, c, ed.xw[0], ed.xw[1], ed.xw[2], ed.u, ed.v, ed.ur, rr, p);
                        double rho0 = sd_se3_chi2(rr, D, (double)ed.inv_sigma2), rho1;
                        if (robust) sd_huber(rho0, D == 2 ? dM : dS, rho0, rho1);
                        tc[0] += rho0;
                    }
                    sd_block_sum<1>(tc, red);
                    errPose = est;
                    const double tempChi = ok2 ? tc[0] : 1.7976931348623157e308;
                    rho = currentChi - tempChi;
                    double scale = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; j++) scale += xs[j] * (lambda * xs[j] + b[j]);
                    scale += 1e-3;
                    rho /= scale;
                    if (rho > 0 && __builtin_isfinite(tempChi)) {
                        double alpha = 1. - pow((2 * rho - 1), 3);
                        alpha = fmin(alpha, 2. / 3.);
                        lambda *= fmax(1. / 3., alpha);
                        ni = 2;
                        currentChi = tempChi;
                    } else {
                        lambda *= ni;
                        ni *= 2;
                        est = backup;                                    // pop(): the edges keep the rejected trial's errors
                    }
                    qmax++;
                } while (rho < 0 && qmax < 10);
                if (qmax == 10 || rho == 0) break;
                if ((iniChi - currentChi) * 1e3 < iniChi) nStop++; else nStop = 0;
                if (nStop >= 3) break;
            }
        }
        // classification: outliers of the previous round get computeError() at est, the others keep their cached error
        __syncthreads();
        double nb[1] = {0.0};
        for (int i = e0 + tid; i < e1; i += SD_POSE_THREADS) {
            const sd_pose_edge ed = E[i];
            double rr[3], p[3];
            const int D = sd_se3_error(out[i] ? est : errPose, c, ed.xw[0], ed.xw[1], ed.xw[2], ed.u, ed.v, ed.ur, rr, p);
            const float c2 = (float)sd_se3_chi2(rr, D, (double)ed.inv_sigma2);
            const bool bad = c2 > (D == 2 ? 5.991f : 7.815f);
            out[i] = bad ? 1 : 0;
            nb[0] += bad ? 1.0 : 0.0;
        }
        sd_block_sum<1>(nb, red);
        nBad = (int)nb[0];
        nBadPrev = nBad;
        if (round == 2) robust = false;
        if (nE < 10) break;
    }
    __syncthreads();
    if (tid < 16) {                                                      // Converter::toCvMat(SE3Quat): R from the quaternion, t, f32
        double R[3][3];
        sd_quat_matrix(est.r, R);
        const double M[16] = {R[0][0], R[0][1], R[0][2], est.t0, R[1][0], R[1][1], R[1][2], est.t1, R[2][0], R[2][1], R[2][2], est.t2, 0, 0, 0, 1};
        double m = 0.0;
#pragma unroll
        for (int k = 0; k < 16; k++) if (tid == k) m = M[k];               // a select per entry: no indexed register array
        Tq[tid] = (float)m;
    }
    if (tid == 0) A.nGood[q] = nE - nBad;
}

// The edges of PoseOptimization(&mCurrentFrame) after SearchByProjection(mCurrentFrame, mLastFrame): one workgroup per projection
// pair, keypoints of the Current slot in index order, an edge for every i with match[i] >= 0 (mvpMapPoints[i] != NULL), compacted by
// a ballot prefix so the edge order is the keypoint order.  Pair `pair` owns edges [pair * cap, pair * cap + n).  Also copies the
// prior pose into the pair's pose slot.  Tracker gating: a pair whose `active` entry is 0, or whose matcher returned fewer than
// minMatches, gets no edges (ran = 0).
struct SdPoseEdgeArgs {
    const sd_keypoint* kp;            // mvKeysUn of the batch
    const float* uRight;
    const int* count;
    const float* xw;                  // map-point table [slot][cap][3]
    const int* match;                 // [pair][cap]
    const int2* pairIdx;              // (Current slot, Last slot) of every pair
    const float* TcwPair;             // [pair][16]: the pose the pair was matched with
    const float* Tin;                 // nullable [k][16]: the caller's prior of launch entry k
    const int* map;                   // [k] pair of launch entry k
    const int* active; int activeBase;
    const int* nmatch; int minMatches;
    sd_pose_edge* edges; int* first; int* last; float* Tout; int* ran;
    float invSigma2[SD_MAX_LEVELS]; int nLevels;
    int cap;
};

__global__ void __launch_bounds__(256) k_pose_edges(SdPoseEdgeArgs A)
{
    __shared__ int wsum[4];
    const int k = blockIdx.x, pair = A.map[k], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = A.cap;
    const int2 cl = A.pairIdx[pair];
    if (tid < 16) A.Tout[(size_t)pair * 16 + tid] = A.Tin ? A.Tin[(size_t)k * 16 + tid] : A.TcwPair[(size_t)pair * 16 + tid];
    const bool run = !(A.active && !A.active[pair - A.activeBase]) && !(A.minMatches > 0 && A.nmatch[pair] < A.minMatches);
    const size_t e0 = (size_t)pair * cap;
    if (!run) {
        if (tid == 0) { A.first[pair] = (int)e0; A.last[pair] = (int)e0; A.ran[pair] = 0; }
        return;
    }
    const int N = A.count[cl.x];
    const int* __restrict__ m = A.match + (size_t)pair * cap;
    const size_t cur = (size_t)cl.x * cap, lst = (size_t)cl.y * cap;
    int base = 0;
    for (int c = 0; c < N; c += 256) {
        const int i = c + tid;
        const int mi = i < N ? m[i] : -1;
        const bool pred = mi >= 0;
        const unsigned long long bal = __ballot(pred);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) { if (w < wave) off += wsum[w]; tot += wsum[w]; }
        if (pred) {
            const sd_keypoint kp = A.kp[cur + i];
            float w = 0.f;
#pragma unroll
            for (int l = 0; l < SD_MAX_LEVELS; l++) if (kp.octave == l) w = A.invSigma2[l];
            sd_pose_edge e;
            e.xw[0] = A.xw[(lst + mi) * 3 + 0]; e.xw[1] = A.xw[(lst + mi) * 3 + 1]; e.xw[2] = A.xw[(lst + mi) * 3 + 2];
            e.u = kp.x; e.v = kp.y; e.ur = A.uRight[cur + i]; e.inv_sigma2 = w; e.kp_index = i;
            A.edges[e0 + off + pre] = e;
        }
        __syncthreads();
        base += tot;
    }
    if (tid == 0) { A.first[pair] = (int)e0; A.last[pair] = (int)e0 + base; A.ran[pair] = 1; }
}
