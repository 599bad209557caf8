// Optimizer::PoseOptimization (src/Optimizer.cc:239-451) with the vendored g2o's Levenberg-Marquardt for
// many independent frames in one launch: one 256-thread workgroup per problem runs all 4 rounds x optimize(10) on the device.
// Per-edge work is strided over the workgroup; the sums the algorithm needs (the 21 + 6 distinct entries of H and b with the
// active robust chi2 per iteration, the chi2 alone per LM trial, nBad per round) are reduced by wave64 xor-butterflies and a
// fixed-order sum of the four wave partials in LDS, so every lane holds the same bits and a problem's result does not depend on
// which problems share the launch.  Everything that follows a reduction (the 6x6 pivoted LDL^T, SE3 exp / compose /
// renormalise, the LM bookkeeping) is computed uniformly by every lane.  f64 throughout; inputs f32 as the reference's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sd_frontend.h"
#include "sd_plan.h"

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

struct Q { double x, y, z, w; };
struct T { Q r; double t0, t1, t2; };

__device__ __forceinline__ void renorm(Q& q)        // SE3Quat::normalizeRotation: w >= 0, then Quaterniond::normalize
{
    if (q.w < 0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
    const double n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    if (n2 > 0) { const double n = sqrt(n2); q.x = q.x / n; q.y = q.y / n; q.z = q.z / n; q.w = q.w / n; }
}

__device__ __forceinline__ Q quat_of(double m00, double m01, double m02, double m10, double m11, double m12, double m20, double m21,
                                     double m22)            // Quaterniond(const Matrix3d&)
{
    Q q;
    const double tr = m00 + m11 + m22;
    int i = 0;                                          // largest diagonal entry, first one on ties
    if (m11 > m00) i = 1;
    if (m22 > (i == 1 ? m11 : m00)) i = 2;
    if (tr > 0) {
        double t = sqrt(tr + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (m21 - m12) * t; q.y = (m02 - m20) * t; q.z = (m10 - m01) * t;
    } else if (i == 2) {
        // i = 2 (j = 0, k = 1)
        double t = sqrt(m22 - m00 - m11 + 1.0);
        q.z = 0.5 * t;
        t = 0.5 / t;
        q.w = (m10 - m01) * t; q.x = (m02 + m20) * t; q.y = (m12 + m21) * t;
    } else if (i == 1) {
        // i = 1 (j = 2, k = 0)
        double t = sqrt(m11 - m22 - m00 + 1.0);
        q.y = 0.5 * t;
        t = 0.5 / t;
        q.w = (m02 - m20) * t; q.z = (m21 + m12) * t; q.x = (m01 + m10) * t;
    } else {
        // i = 0 (j = 1, k = 2)
        double t = sqrt(m00 - m11 - m22 + 1.0);
        q.x = 0.5 * t;
        t = 0.5 / t;
        q.w = (m21 - m12) * t; q.y = (m10 + m01) * t; q.z = (m20 + m02) * t;
    }
    return q;
}

__device__ __forceinline__ void rot(const Q& q, double v0, double v1, double v2, double& o0, double& o1, double& o2)
{
    double u0 = q.y * v2 - q.z * v1, u1 = q.z * v0 - q.x * v2, u2 = q.x * v1 - q.y * v0;
    u0 = u0 + u0; u1 = u1 + u1; u2 = u2 + u2;
    const double c0 = q.y * u2 - q.z * u1, c1 = q.z * u0 - q.x * u2, c2 = q.x * u1 - q.y * u0;
    o0 = v0 + q.w * u0 + c0; o1 = v1 + q.w * u1 + c1; o2 = v2 + q.w * u2 + c2;
}

__device__ __forceinline__ T compose(const T& a, const T& b)       // SE3Quat::operator*
{
    T r;
    double p0, p1, p2;
    rot(a.r, b.t0, b.t1, b.t2, p0, p1, p2);
    r.t0 = a.t0 + p0; r.t1 = a.t1 + p1; r.t2 = a.t2 + p2;
    r.r.w = a.r.w * b.r.w - a.r.x * b.r.x - a.r.y * b.r.y - a.r.z * b.r.z;
    r.r.x = a.r.w * b.r.x + a.r.x * b.r.w + a.r.y * b.r.z - a.r.z * b.r.y;
    r.r.y = a.r.w * b.r.y + a.r.y * b.r.w + a.r.z * b.r.x - a.r.x * b.r.z;
    r.r.z = a.r.w * b.r.z + a.r.z * b.r.w + a.r.x * b.r.y - a.r.y * b.r.x;
    renorm(r.r);
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
    r.r = quat_of(R[0][0], R[0][1], R[0][2], R[1][0], R[1][1], R[1][2], R[2][0], R[2][1], R[2][2]);
    r.t0 = V[0][0] * u[3] + V[0][1] * u[4] + V[0][2] * u[5];
    r.t1 = V[1][0] * u[3] + V[1][1] * u[4] + V[1][2] * u[5];
    r.t2 = V[2][0] * u[3] + V[2][1] * u[4] + V[2][2] * u[5];
    renorm(r.r);
    return r;
}

struct Cam { double fx, fy, cx, cy, bf; };

// computeError of either edge type at pose s; D = 2 (mono, ur < 0) or 3 (stereo: invz rounded to f32, types_six_dof_expmap.cpp:299-306)
__device__ __forceinline__ int err(const sd_pose_edge& E, const Cam& c, const T& s, double& e0, double& e1, double& e2, double& p0,
                                   double& p1, double& p2)
{
    rot(s.r, (double)E.xw[0], (double)E.xw[1], (double)E.xw[2], p0, p1, p2);
    p0 = p0 + s.t0; p1 = p1 + s.t1; p2 = p2 + s.t2;
    if (E.ur < 0) {
        e0 = (double)E.u - ((p0 / p2) * c.fx + c.cx);
        e1 = (double)E.v - ((p1 / p2) * c.fy + c.cy);
        e2 = 0.0;
        return 2;
    }
    const double iz = (double)(float)(1.0 / p2);
    const double r0 = p0 * iz * c.fx + c.cx;
    e0 = (double)E.u - r0;
    e1 = (double)E.v - (p1 * iz * c.fy + c.cy);
    e2 = (double)E.ur - (r0 - c.bf * iz);
    return 3;
}

__device__ __forceinline__ double chi2(double e0, double e1, double e2, int D, double w)
{
    double s = e0 * (w * e0) + e1 * (w * e1);
    if (D == 3) s = s + e2 * (w * e2);
    return s;
}

// wave64 xor-butterfly (every lane of the wave ends with the same bits), then the four wave partials in a fixed order
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* red)
{
#pragma unroll
    for (int k = 0; k < K; k++) {
        double x = v[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
        v[k] = x;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                                    // earlier readers of `red` are done
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[wave * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = (red[k] + red[K + k]) + (red[2 * K + k] + red[3 * K + k]);
}

// (H + lambda I) x = b by Eigen::LDLT's pivoted LDL^T (lower storage); returns isPositive().  x keeps its value when not positive.
// H holds the lower triangle row by row: H[i(i+1)/2 + j], j <= i.  Every index is a compile-time constant after unrolling.
__device__ __forceinline__ bool solve6(const double (&H)[21], const double (&b)[6], double lambda, double (&x)[6])
{
    double A[6][6];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) A[i][j] = j <= i ? H[i * (i + 1) / 2 + j] : 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) A[i][i] += lambda;
    int tr[6];
    int sign = 0;                                       // 0 zero, 1 positive semi-definite, 2 negative semi-definite, 3 indefinite
#pragma unroll
    for (int k = 0; k < 6; k++) {
        int p = k;
        double big = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; i++) if (fabs(A[i][i]) > big) { big = fabs(A[i][i]); p = i; }
        tr[k] = p;
#pragma unroll
        for (int q = k + 1; q < 6; q++) {
            if (p == q) {
                double t;
#pragma unroll
                for (int j = 0; j < k; j++) { t = A[k][j]; A[k][j] = A[q][j]; A[q][j] = t; }
                t = A[k][k]; A[k][k] = A[q][q]; A[q][q] = t;
#pragma unroll
                for (int i = k + 1; i < q; i++) { t = A[i][k]; A[i][k] = A[q][i]; A[q][i] = t; }
#pragma unroll
                for (int i = q + 1; i < 6; i++) { t = A[i][k]; A[i][k] = A[i][q]; A[i][q] = t; }
            }
        }
        if (k > 0) {
            double tmp[6];
#pragma unroll
            for (int j = 0; j < k; j++) tmp[j] = A[j][j] * A[k][j];
            double s = A[k][0] * tmp[0];
#pragma unroll
            for (int j = 1; j < k; j++) s = s + A[k][j] * tmp[j];
            A[k][k] -= s;
#pragma unroll
            for (int i = k + 1; i < 6; i++) {
                double r = A[i][0] * tmp[0];
#pragma unroll
                for (int j = 1; j < k; j++) r = r + A[i][j] * tmp[j];
                A[i][k] -= r;
            }
        }
        const double akk = A[k][k];
        if (fabs(akk) > 0) {
#pragma unroll
            for (int i = k + 1; i < 6; i++) A[i][k] /= akk;
        }
        if (sign == 1) { if (akk < 0) sign = 3; }
        else if (sign == 2) { if (akk > 0) sign = 3; }
        else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
    }
    if (!(sign == 1 || sign == 0)) return false;
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) y[i] = b[i];
#pragma unroll
    for (int k = 0; k < 6; k++)
#pragma unroll
        for (int q = k + 1; q < 6; q++)
            if (tr[k] == q) { const double t = y[k]; y[k] = y[q]; y[q] = t; }
#pragma unroll
    for (int i = 1; i < 6; i++) {
        double s = A[i][0] * y[0];
#pragma unroll
        for (int j = 1; j < i; j++) s = s + A[i][j] * y[j];
        y[i] -= s;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) y[i] = fabs(A[i][i]) > 2.2250738585072014e-308 ? y[i] / A[i][i] : 0.0;
#pragma unroll
    for (int i = 4; i >= 0; i--) {
        double s = A[i + 1][i] * y[i + 1];
#pragma unroll
        for (int j = i + 2; j < 6; j++) s = s + A[j][i] * y[j];
        y[i] -= s;
    }
#pragma unroll
    for (int k = 5; k >= 0; k--)
#pragma unroll
        for (int q = k + 1; q < 6; q++)
            if (tr[k] == q) { const double t = y[k]; y[k] = y[q]; y[q] = t; }
#pragma unroll
    for (int i = 0; i < 6; i++) x[i] = y[i];
    return true;
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
    const Cam c = {(double)C0.fx, (double)C0.fy, (double)C0.cx, (double)C0.cy, (double)C0.mbf};
    float* Tq = A.Tcw + (size_t)q * 16;
    T pose0;                                                             // Converter::toSE3Quat(pFrame->mTcw)
    pose0.r = quat_of(Tq[0], Tq[1], Tq[2], Tq[4], Tq[5], Tq[6], Tq[8], Tq[9], Tq[10]);
    pose0.t0 = Tq[3]; pose0.t1 = Tq[7]; pose0.t2 = Tq[11];
    renorm(pose0.r);
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
                    double r0, r1, r2, p0, p1, p2;
                    const int D = err(ed, c, est, r0, r1, r2, p0, p1, p2);
                    const double w = (double)ed.inv_sigma2, c2 = chi2(r0, r1, r2, D, w);
                    double rho0 = c2, rho1 = 1.0;
                    if (robust) {
                        const double delta = D == 2 ? dM : dS, dsqr = delta * delta;
                        if (!(c2 <= dsqr)) { const double sq = sqrt(c2); rho0 = 2 * sq * delta - dsqr; rho1 = delta / sq; }
                    }
                    v[27] += rho0;
                    // linearizeOplus (types_six_dof_expmap.cpp:266-364)
                    const double x = p0, y = p1, iz = 1.0 / p2, iz2 = iz * iz;
                    double J[3][6];
                    J[0][0] = x * y * iz2 * c.fx; J[0][1] = -(1 + (x * x * iz2)) * c.fx; J[0][2] = y * iz * c.fx;
                    J[0][3] = -iz * c.fx; J[0][4] = 0; J[0][5] = x * iz2 * c.fx;
                    J[1][0] = (1 + y * y * iz2) * c.fy; J[1][1] = -x * y * iz2 * c.fy; J[1][2] = -x * iz * c.fy;
                    J[1][3] = 0; J[1][4] = -iz * c.fy; J[1][5] = y * iz2 * c.fy;
                    J[2][0] = J[0][0] - c.bf * y * iz2; J[2][1] = J[0][1] + c.bf * x * iz2; J[2][2] = J[0][2];
                    J[2][3] = J[0][3]; J[2][4] = 0; J[2][5] = J[0][5] - c.bf * iz2;
                    const double rr[3] = {r0, r1, r2};
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
                block_sum<28>(v, red);
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
                    const bool ok2 = solve6(H, b, lambda, xs);
                    est = compose(expmap(xs), est);                      // VertexSE3Expmap::oplusImpl
                    double tc[1] = {0.0};
                    for (int i = e0 + tid; i < e1; i += SD_POSE_THREADS) {
                        if (out[i]) continue;
                        const sd_pose_edge ed = E[i];
                        double r0, r1, r2, p0, p1, p2;
                        const int D = err(ed, c, est, r0, r1, r2, p0, p1, p2);
                        const double c2 = chi2(r0, r1, r2, D, (double)ed.inv_sigma2);
                        double rho0 = c2;
                        if (robust) {
                            const double delta = D == 2 ? dM : dS, dsqr = delta * delta;
                            if (!(c2 <= dsqr)) rho0 = 2 * sqrt(c2) * delta - dsqr;
                        }
                        tc[0] += rho0;
                    }
                    block_sum<1>(tc, red);
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
            double r0, r1, r2, p0, p1, p2;
            const int D = err(ed, c, out[i] ? est : errPose, r0, r1, r2, p0, p1, p2);
            const float c2 = (float)chi2(r0, r1, r2, D, (double)ed.inv_sigma2);
            const bool bad = c2 > (D == 2 ? 5.991f : 7.815f);
            out[i] = bad ? 1 : 0;
            nb[0] += bad ? 1.0 : 0.0;
        }
        block_sum<1>(nb, red);
        nBad = (int)nb[0];
        nBadPrev = nBad;
        if (round == 2) robust = false;
        if (nE < 10) break;
    }
    __syncthreads();
    if (tid < 16) {                                                      // Converter::toCvMat(SE3Quat): R from the quaternion, t, f32
        const Q& r = est.r;
        const double tx = 2 * r.x, ty = 2 * r.y, tz = 2 * r.z;
        const double twx = tx * r.w, twy = ty * r.w, twz = tz * r.w, txx = tx * r.x, txy = ty * r.x, txz = tz * r.x;
        const double tyy = ty * r.y, tyz = tz * r.y, tzz = tz * r.z;
        double m;
        switch (tid) {
            case 0: m = 1 - (tyy + tzz); break;  case 1: m = txy - twz; break;      case 2: m = txz + twy; break;  case 3: m = est.t0; break;
            case 4: m = txy + twz; break;        case 5: m = 1 - (txx + tzz); break; case 6: m = tyz - twx; break;  case 7: m = est.t1; break;
            case 8: m = txz - twy; break;        case 9: m = tyz + twx; break;      case 10: m = 1 - (txx + tyy); break; case 11: m = est.t2; break;
            case 15: m = 1.0; break;
            default: m = 0.0; break;
        }
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
