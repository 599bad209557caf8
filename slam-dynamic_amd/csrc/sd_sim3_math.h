// The arithmetic of Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241) that both the kernel (k_sim3_opt.h) and the CPU oracle
// (tests/cpp/sim3_opt_oracle.cpp) must evaluate to the same bits: g2o's Sim3 (types/sim3.h), VertexSim3Expmap::oplusImpl, the two
// projection edges' computeError (types_seven_dof_expmap.h:130-171) and the robustified quadratic form of one edge
// (base_binary_edge.hpp:54-120).  What Sim3 shares with the SE3 solvers (the quaternion, Huber, the dense pivoted LDL^T of
// LinearSolverDense) is sd_g2o_math.h.
// The edges have no analytic Jacobian, so g2o differentiates them numerically with delta = 1e-9: a one-ulp difference in an error is
// a 1e-5 difference in J.  Hence ONE header, plain f64 + - * / sqrt and explicit fma only (all correctly rounded on x86 and gfx950),
// compiled without contraction on either side, and private sin / cos / exp built from those operations (DESIGN Q45).
#pragma once
#include "sd_g2o_math.h"

// g2o::Sim3: r, t, s.  The rotation is the shared sd_quat; qx .. qw name the same four doubles (two layout-compatible structs in
// a union, read through either), which is how the oracle spells them.
struct sd_s3 { union { sd_quat r; struct { double qx, qy, qz, qw; }; }; double t0, t1, t2, s; };

// the shared functions under the names the oracle calls them by
SD_HD void sd_s3_quat_of(const double (&m)[3][3], sd_s3& o) { o.r = sd_quat_of(m); }
SD_HD void sd_s3_huber(double e, double delta, double& rho0, double& rho1) { sd_huber(e, delta, rho0, rho1); }
template <int N>
SD_HD bool sd_s3_solve(const double* H, const double* b, double lambda, double (&x)[N]) { return sd_ldlt_solve<N>(H, b, lambda, x); }

// sin and cos of x >= 0 (an update's rotation angle): the quadrant reduction and fdlibm kernels of sd_cos_sin_f32, kept in f64.
// Within 1 ulp of glibc on [1e-5, 8] (tests/cpp/sim3_math_check.cpp); beyond 1e9, or not finite: NaN.
SD_HD void sd_s3_sincos(double x, double& sn_, double& cs_)
{
    if (!(x > -1e9 && x < 1e9)) { sn_ = cs_ = (x - x) / (x - x); return; }
    const double kd = __builtin_rint(x * 0.63661977236758134308);
    const int n = (int)((long long)kd & 3);
    double r = __builtin_fma(-kd, 1.5707963267948966, x);
    r = __builtin_fma(-kd, 6.123233995736766e-17, r);
    const double z = r * r;
    const double ps = __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08),
                                    2.75573137070700676789e-06), -1.98412698298579493134e-04), 8.33333333332248946124e-03), -1.66666666666666324348e-01);
    const double sn = __builtin_fma(z * r, ps, r);
    const double pc = __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09),
                                    -2.75573143513906633035e-07), 2.48015872894767294178e-05), -1.38888888888741095749e-03), 4.16666666666666019037e-02);
    const double cs = 1.0 - __builtin_fma(0.5, z, -(z * z) * pc);
    const double c = (n & 1) ? sn : cs, s = (n & 1) ? cs : sn;
    cs_ = (n == 1 || n == 2) ? -c : c;
    sn_ = (n >= 2) ? -s : s;
}

SD_HD double sd_s3_pow2(int k)                                  // 2^k, |k| <= 1023, by exact doublings or halvings
{
    double f = 1.0, b = k < 0 ? 0.5 : 2.0;
    if (k < 0) k = -k;
    for (int i = 0; i < 10; i++) { if (k & 1) f = f * b; b = b * b; k >>= 1; }
    return f;
}

// exp(x) after fdlibm's e_exp.c: x = k ln2 + r, exp(r) = 1 + 2r / (R(r^2) - r), scaled by 2^k in two steps.
SD_HD double sd_s3_exp(double x)
{
    if (!(x == x)) return x;
    if (x > 709.78) return 1.7976931348623157e308 * 2.0;
    if (x < -708.0) return 0.0;                                  // no subnormal results: a scale of 1e-308 is no estimate
    const double kd = __builtin_rint(x * 1.44269504088896338700e+00);
    const double hi = __builtin_fma(-kd, 6.93147180369123816490e-01, x);
    const double lo = kd * 1.90821492927058770002e-10;
    const double r = hi - lo;
    const double t = r * r;
    const double c = r - t * __builtin_fma(t, __builtin_fma(t, __builtin_fma(t, __builtin_fma(t, 4.13813679705723846039e-08, -1.65339022054652515390e-06),
                                           6.61375632143793436117e-05), -2.77777777770155933842e-03), 1.66666666666666019037e-01);
    double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    const int k = (int)kd, k1 = k / 2;                           // |k| <= 1024: 2^k as two factors, so that neither overflows before y scales it
    return (y * sd_s3_pow2(k1)) * sd_s3_pow2(k - k1);
}

SD_HD void sd_s3_map(const sd_s3& S, double x, double y, double z, double& o0, double& o1, double& o2)      // s * (r * xyz) + t
{
    double r0, r1, r2;
    sd_quat_rot(S.r, x, y, z, r0, r1, r2);
    o0 = S.s * r0 + S.t0; o1 = S.s * r1 + S.t1; o2 = S.s * r2 + S.t2;
}

SD_HD sd_s3 sd_s3_mul(const sd_s3& a, const sd_s3& b)           // Sim3::operator* (no renormalisation)
{
    sd_s3 r;
    r.r = sd_quat_mul(a.r, b.r);
    double p0, p1, p2;
    sd_quat_rot(a.r, b.t0, b.t1, b.t2, p0, p1, p2);
    r.t0 = a.s * p0 + a.t0; r.t1 = a.s * p1 + a.t1; r.t2 = a.s * p2 + a.t2;
    r.s = a.s * b.s;
    return r;
}

SD_HD sd_s3 sd_s3_inverse(const sd_s3& a)                       // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
{
    sd_s3 r;
    r.r.x = -a.r.x; r.r.y = -a.r.y; r.r.z = -a.r.z; r.r.w = a.r.w;
    const double m = -1. / a.s;
    sd_quat_rot(r.r, m * a.t0, m * a.t1, m * a.t2, r.t0, r.t1, r.t2);
    r.s = 1. / a.s;
    return r;
}

// Sim3(const Vector7d& update) (sim3.h:70-142).  branch: 0 sigma and theta small, 1 theta large, 2 sigma large, 3 both large.
SD_HD sd_s3 sd_s3_exp_update(const double (&u)[7], int& branch)
{
    const double w0 = u[0], w1 = u[1], w2 = u[2], sigma = u[6];
    const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double O[3][3] = {{0, -w2, w1}, {w2, 0, -w0}, {-w1, w0, 0}};
    double O2[3][3], R[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    sd_s3 S;
    S.s = sd_s3_exp(sigma);
    const double eps = 0.00001;
    double A, B, C;
    const bool smallSigma = (sigma < 0 ? -sigma : sigma) < eps, smallTheta = theta < eps;
    branch = (smallSigma ? 0 : 2) + (smallTheta ? 0 : 1);
    double sn = 0.0, cs = 1.0;
    if (!smallTheta) sd_s3_sincos(theta, sn, cs);
    if (smallTheta) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
    } else {
        const double a = sn / theta, b = (1 - cs) / (theta * theta);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + a * O[i][j]) + b * O2[i][j];
    }
    if (smallSigma) {
        C = 1;
        if (smallTheta) { A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta2 = theta * theta;
            A = (1 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        const double sigma2 = sigma * sigma;
        if (smallTheta) {
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double a = S.s * sn, b = S.s * cs, theta2 = theta * theta;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    S.r = sd_quat_of(R);
    double W[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) W[i][j] = (A * O[i][j] + B * O2[i][j]) + C * (i == j ? 1.0 : 0.0);
    S.t0 = W[0][0] * u[3] + W[0][1] * u[4] + W[0][2] * u[5];
    S.t1 = W[1][0] * u[3] + W[1][1] * u[4] + W[1][2] * u[5];
    S.t2 = W[2][0] * u[3] + W[2][1] * u[4] + W[2][2] * u[5];
    return S;
}

// VertexSim3Expmap::oplusImpl: the update's scale entry is zeroed IN PLACE when the scale is fixed (the caller's vector is the
// solver's x, which computeScale reads afterwards), then estimate = Sim3(update) * estimate.
SD_HD sd_s3 sd_s3_oplus(const sd_s3& est, double (&u)[7], bool fixScale, int& branch)
{
    if (fixScale) u[6] = 0;
    return sd_s3_mul(sd_s3_exp_update(u, branch), est);
}

// Camera coordinates of a map point: the f32 statement of Sim3Solver (R * X + t as the cv::Mat product evaluates it, DESIGN Q39)
SD_HD void sd_s3_to_camera(const float* T, float x, float y, float z, float& ox, float& oy, float& oz)
{
    float s;
    s = T[0] * x + T[1] * y; s = s + T[2] * z; ox = s + T[3];
    s = T[4] * x + T[5] * y; s = s + T[6] * z; oy = s + T[7];
    s = T[8] * x + T[9] * y; s = s + T[10] * z; oz = s + T[11];
}

struct sd_s3_cam { double fx, fy, cx, cy; };

// computeError of either edge: obs - cam_map(project(S.map(X))); S is the estimate for EdgeSim3ProjectXYZ and its inverse for
// EdgeInverseSim3ProjectXYZ.  No depth test: z = 0 gives Inf / NaN, a point behind the camera projects like any other.
SD_HD void sd_s3_error(const sd_s3& S, const sd_s3_cam& c, double X, double Y, double Z, double u, double v, double& e0, double& e1)
{
    double p0, p1, p2;
    sd_s3_map(S, X, Y, Z, p0, p1, p2);
    e0 = u - ((p0 / p2) * c.fx + c.cx);
    e1 = v - ((p1 / p2) * c.fy + c.cy);
}

// chi2() = error . (information * error) with information = w I, multiplied out as the 2x2 product is
SD_HD double sd_s3_chi2(double e0, double e1, double w)
{
    return e0 * (w * e0 + 0.0 * e1) + e1 * (0.0 * e0 + w * e1);
}

// One edge's share of the 7x7 system (constructQuadraticForm's robust branch, the Sim3 vertex being the only free one):
// v[0..27] += lower triangle of J^T (rho1 w I) J row by row, v[28..34] += J^T (rho1 * -(w I) e), v[35] += rho0.
SD_HD void sd_s3_accumulate(double e0, double e1, const double (&J)[2][7], double w, double delta, double (&v)[36])
{
    double rho0, rho1;
    sd_huber(sd_s3_chi2(e0, e1, w), delta, rho0, rho1);
    const double wo = rho1 * w;
    double r0 = -(w * e0 + 0.0 * e1), r1 = -(0.0 * e0 + w * e1);
    r0 = r0 * rho1; r1 = r1 * rho1;
    for (int i = 0; i < 7; i++) {
        const double a0 = J[0][i] * wo + J[1][i] * 0.0, a1 = J[0][i] * 0.0 + J[1][i] * wo;
        for (int j = 0; j <= i; j++) v[i * (i + 1) / 2 + j] += a0 * J[0][j] + a1 * J[1][j];
        v[28 + i] += J[0][i] * r0 + J[1][i] * r1;
    }
    v[35] += rho0;
}

// The factor the damping is multiplied by after an accepted step (optimization_algorithm_levenberg.cpp:135-139); pow(., 3) as the
// product t * t * t, which lies within one ulp of any library's
SD_HD double sd_s3_good_step_scale(double rho)
{
    const double t = 2 * rho - 1;
    double alpha = 1. - t * t * t;
    alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
    return 1. / 3. > alpha ? 1. / 3. : alpha;                    // (std::max)(_goodStepLowerScale, alpha)
}

SD_HD bool sd_s3_solve7(const double* H, const double* b, double lambda, double (&x)[7]) { return sd_ldlt_solve<7>(H, b, lambda, x); }
