// The arithmetic of the vendored g2o / Eigen that the three Levenberg-Marquardt kernels restate -- k_pose_optimize (k_pose.h),
// k_local_ba (k_ba.h), k_sim3_optimize (k_sim3_opt.h with sd_sim3_math.h) -- and k_sim3_refine.h, held ONCE: Quaterniond from and to a
// 3 x 3 matrix and times a vector, SE3Quat::normalizeRotation, the SE3 projection edges' computeError and chi2, RobustKernelHuber
// and the dense pivoted LDL^T of LinearSolverDense.
// Every copy has to agree with Eigen / g2o to the bit (and the Sim3 edges are differentiated numerically with delta = 1e-9: a one-ulp
// difference in an error is a 1e-5 difference in J), so the first part is plain f64 + - * / sqrt under SD_HD, compiled without
// contraction on either side (all correctly rounded on x86 and gfx950): tests/cpp/sim3_opt_oracle.cpp reaches it through
// sd_sim3_math.h on the host.  The second part (wave and workgroup reductions) is device-only.
// NOT here, because the reference's arithmetic differs between the solvers: the Jacobians and gradient terms of the SE3 edges (the
// unary edge multiplies by 1 / z, the binary one divides by z), Sim3's chi2 with the 0.0 * e terms of its 2 x 2 product, the cube of
// the good-step scale (the device library's pow for SE3, t * t * t for Sim3) and the trigonometry.
// NOT here either: the damping bookkeeping of OptimizationAlgorithmLevenberg (lambda, ni, nStop; accept / reject; the stop rules), which
// each kernel keeps inline.  As one value type with init / trial / stop it computed the same bits, but it moved the register
// assignment of all of k_sim3_optimize (352 spilled VGPRs) and the Sim3 refine chain measured slower than its own spread (DESIGN Q24c).
#pragma once
#if !defined(__HIPCC__)
#include <cmath>
using std::sqrt;
#endif
#include "sd_trig.h"

struct sd_quat { double x, y, z, w; };                          // Eigen coefficient order
struct sd_se3 { sd_quat r; double t0, t1, t2; };                // g2o::SE3Quat

SD_HD sd_quat sd_quat_of(const double (&m)[3][3])                // Eigen::Quaterniond(const Matrix3d&)
{
    sd_quat q;
    const double tr = m[0][0] + m[1][1] + m[2][2];
    int i = 0;                                                   // largest diagonal entry, first one on ties
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > (i == 1 ? m[1][1] : m[0][0])) i = 2;
    if (tr > 0) {
        double t = sqrt(tr + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (m[2][1] - m[1][2]) * t; q.y = (m[0][2] - m[2][0]) * t; q.z = (m[1][0] - m[0][1]) * t;
    } else if (i == 2) {
        // i = 2 (j = 0, k = 1)
        double t = sqrt(m[2][2] - m[0][0] - m[1][1] + 1.0);
        q.z = 0.5 * t;
        t = 0.5 / t;
        q.w = (m[1][0] - m[0][1]) * t; q.x = (m[0][2] + m[2][0]) * t; q.y = (m[1][2] + m[2][1]) * t;
    } else if (i == 1) {
        // i = 1 (j = 2, k = 0)
        double t = sqrt(m[1][1] - m[2][2] - m[0][0] + 1.0);
        q.y = 0.5 * t;
        t = 0.5 / t;
        q.w = (m[0][2] - m[2][0]) * t; q.z = (m[2][1] + m[1][2]) * t; q.x = (m[0][1] + m[1][0]) * t;
    } else {
        // i = 0 (j = 1, k = 2)
        double t = sqrt(m[0][0] - m[1][1] - m[2][2] + 1.0);
        q.x = 0.5 * t;
        t = 0.5 / t;
        q.w = (m[2][1] - m[1][2]) * t; q.y = (m[1][0] + m[0][1]) * t; q.z = (m[2][0] + m[0][2]) * t;
    }
    return q;
}

SD_HD void sd_quat_matrix(const sd_quat& q, double (&R)[3][3])   // Quaterniond::toRotationMatrix()
{
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w, txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
}

SD_HD void sd_quat_rot(const sd_quat& q, double v0, double v1, double v2, double& o0, double& o1, double& o2)
{                                                                // Quaterniond * Vector3d
    double u0 = q.y * v2 - q.z * v1, u1 = q.z * v0 - q.x * v2, u2 = q.x * v1 - q.y * v0;
    u0 = u0 + u0; u1 = u1 + u1; u2 = u2 + u2;
    const double c0 = q.y * u2 - q.z * u1, c1 = q.z * u0 - q.x * u2, c2 = q.x * u1 - q.y * u0;
    o0 = v0 + q.w * u0 + c0; o1 = v1 + q.w * u1 + c1; o2 = v2 + q.w * u2 + c2;
}

SD_HD sd_quat sd_quat_mul(const sd_quat& a, const sd_quat& b)    // Quaterniond * Quaterniond
{
    sd_quat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}

SD_HD void sd_quat_renorm(sd_quat& q)                           // SE3Quat::normalizeRotation: w >= 0, then Quaterniond::normalize
{
    if (q.w < 0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
    const double n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    if (n2 > 0) { const double n = sqrt(n2); q.x = q.x / n; q.y = q.y / n; q.z = q.z / n; q.w = q.w / n; }
}

SD_HD sd_se3 sd_se3_of(const float* T)                           // Converter::toSE3Quat of a row-major 4 x 4 f32 pose
{
    double R[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[i][j] = (double)T[4 * i + j];
    sd_se3 s;
    s.r = sd_quat_of(R);
    s.t0 = T[3]; s.t1 = T[7]; s.t2 = T[11];
    sd_quat_renorm(s.r);
    return s;
}

struct sd_se3_cam { double fx, fy, cx, cy, bf; };

// computeError of the pose-only and the two-vertex projection edges alike: the point X in the camera of pose s (p) and obs - projection
// (e); returns D = 2 (mono, ur < 0) or 3 (stereo: invz rounded to f32, types_six_dof_expmap.cpp:188-195 and :299-306)
SD_HD int sd_se3_error(const sd_se3& s, const sd_se3_cam& c, double X0, double X1, double X2, float u, float v, float ur, double (&e)[3],
                       double (&p)[3])
{
    sd_quat_rot(s.r, X0, X1, X2, p[0], p[1], p[2]);
    p[0] = p[0] + s.t0; p[1] = p[1] + s.t1; p[2] = p[2] + s.t2;
    if (ur < 0) {
        e[0] = (double)u - ((p[0] / p[2]) * c.fx + c.cx);
        e[1] = (double)v - ((p[1] / p[2]) * c.fy + c.cy);
        e[2] = 0.0;
        return 2;
    }
    const double iz = (double)(float)(1.0 / p[2]);
    const double r0 = p[0] * iz * c.fx + c.cx;
    e[0] = (double)u - r0;
    e[1] = (double)v - (p[1] * iz * c.fy + c.cy);
    e[2] = (double)ur - (r0 - c.bf * iz);
    return 3;
}

SD_HD double sd_se3_chi2(const double (&e)[3], int D, double w)  // error . (w I) error, without the 0.0 * e terms sd_s3_chi2 carries
{
    double s = e[0] * (w * e[0]) + e[1] * (w * e[1]);
    if (D == 3) s = s + e[2] * (w * e[2]);
    return s;
}

// RobustKernelHuber::robustify: rho[0], rho[1].  A NaN e takes the second branch, as !(e <= dsqr) does.
SD_HD void sd_huber(double e, double delta, double& rho0, double& rho1)
{
    const double dsqr = delta * delta;
    if (e <= dsqr) { rho0 = e; rho1 = 1.; }
    else { const double sq = sqrt(e); rho0 = 2 * sq * delta - dsqr; rho1 = delta / sq; }
}

// (H + lambda I) x = b by Eigen::LDLT's pivoted LDL^T (lower storage) for N unknowns; returns isPositive().  x keeps its value when not
// positive.  H holds the lower triangle row by row: H[i(i+1)/2 + j], j <= i (so the first N rows of a larger one serve as well).
template <int N>
SD_HD bool sd_ldlt_solve(const double* H, const double* b, double lambda, double (&x)[N])
{
    double A[N][N];
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) A[i][j] = j <= i ? H[i * (i + 1) / 2 + j] : 0.0;
#pragma unroll
    for (int i = 0; i < N; i++) A[i][i] += lambda;
    int tr[N];
    int sign = 0;                                                // 0 zero, 1 positive semi-definite, 2 negative semi-definite, 3 indefinite
#pragma unroll
    for (int k = 0; k < N; k++) {
        int p = k;
        double big = A[k][k] < 0 ? -A[k][k] : A[k][k];
#pragma unroll
        for (int i = k + 1; i < N; i++) { const double a = A[i][i] < 0 ? -A[i][i] : A[i][i]; if (a > big) { big = a; p = i; } }
        tr[k] = p;
#pragma unroll
        for (int q = k + 1; q < N; q++) {                        // every index a compile-time constant after unrolling
            if (p == q) {
                double t;
#pragma unroll
                for (int j = 0; j < k; j++) { t = A[k][j]; A[k][j] = A[q][j]; A[q][j] = t; }
                t = A[k][k]; A[k][k] = A[q][q]; A[q][q] = t;
#pragma unroll
                for (int i = k + 1; i < q; i++) { t = A[i][k]; A[i][k] = A[q][i]; A[q][i] = t; }
#pragma unroll
                for (int i = q + 1; i < N; i++) { t = A[i][k]; A[i][k] = A[i][q]; A[i][q] = t; }
            }
        }
        if (k > 0) {
            double tmp[N];
#pragma unroll
            for (int j = 0; j < k; j++) tmp[j] = A[j][j] * A[k][j];
            double s = A[k][0] * tmp[0];
#pragma unroll
            for (int j = 1; j < k; j++) s = s + A[k][j] * tmp[j];
            A[k][k] -= s;
#pragma unroll
            for (int i = k + 1; i < N; i++) {
                double r = A[i][0] * tmp[0];
#pragma unroll
                for (int j = 1; j < k; j++) r = r + A[i][j] * tmp[j];
                A[i][k] -= r;
            }
        }
        const double akk = A[k][k];
        if ((akk < 0 ? -akk : akk) > 0) {
#pragma unroll
            for (int i = k + 1; i < N; i++) A[i][k] /= akk;
        }
        if (sign == 1) { if (akk < 0) sign = 3; }
        else if (sign == 2) { if (akk > 0) sign = 3; }
        else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
    }
    if (!(sign == 1 || sign == 0)) return false;
    double y[N];
#pragma unroll
    for (int i = 0; i < N; i++) y[i] = b[i];
#pragma unroll
    for (int k = 0; k < N; k++)
#pragma unroll
        for (int q = k + 1; q < N; q++)
            if (tr[k] == q) { const double t = y[k]; y[k] = y[q]; y[q] = t; }
#pragma unroll
    for (int i = 1; i < N; i++) {
        double s = A[i][0] * y[0];
#pragma unroll
        for (int j = 1; j < i; j++) s = s + A[i][j] * y[j];
        y[i] -= s;
    }
#pragma unroll
    for (int i = 0; i < N; i++) { const double a = A[i][i] < 0 ? -A[i][i] : A[i][i]; y[i] = a > 2.2250738585072014e-308 ? y[i] / A[i][i] : 0.0; }
#pragma unroll
    for (int i = N - 2; i >= 0; i--) {
        double s = A[i + 1][i] * y[i + 1];
#pragma unroll
        for (int j = i + 2; j < N; j++) s = s + A[j][i] * y[j];
        y[i] -= s;
    }
#pragma unroll
    for (int k = N - 1; k >= 0; k--)
#pragma unroll
        for (int q = k + 1; q < N; q++)
            if (tr[k] == q) { const double t = y[k]; y[k] = y[q]; y[q] = t; }
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = y[i];
    return true;
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------- device only: reductions that leave every lane with the same bits
template <int K>
__device__ __forceinline__ void sd_wave_sum(double (&v)[K])      // wave64 xor-butterfly
{
#pragma unroll
    for (int k = 0; k < K; k++) {
        double x = v[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
        v[k] = x;
    }
}

// a 256-thread workgroup: the wave sums, then the four wave partials in a fixed order through red[4 * K] in LDS
template <int K>
__device__ __forceinline__ void sd_block_sum(double (&v)[K], double* red)
{
    sd_wave_sum<K>(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                                             // earlier readers of `red` are done
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[wave * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = (red[k] + red[K + k]) + (red[2 * K + k] + red[3 * K + k]);
}

__device__ __forceinline__ double sd_block_max(double x, double* red)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = x;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}
#endif
