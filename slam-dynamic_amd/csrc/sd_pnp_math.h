// PnPsolver's arithmetic (src/PnPsolver.cc, cited as PnP:line) as plain C++: + - * /, f64 sqrt, nothing else from libm.  ONE statement,
// included by the kernels (k_pnp.h) and by the CPU oracle (tests/cpp/pnp_oracle.cpp); both sides compile it with -ffp-contract=off, and
// gfx950's f64 division and sqrt are correctly rounded (k_sim3.h relies on the same), so both give the same bytes.  DESIGN.md Q46.
//
// The EPnP pipeline is written once over a context `C` that says how a sum over the correspondences is taken and who runs the scalar
// sections in between:
//   int  C::n()                                   number of correspondences of this solve
//   void C::point(i, pw[3], uv[2])                correspondence i, widened to f64 (add_correspondence, PnP:363-373)
//   bool C::leader() / void C::sync()             the scalar sections run under leader(); sync() orders them against the sums
//   void C::sum<K>(count, f, out)                 out[k] = sum over i < count of v[k], f(i, v) giving item i's K terms; collective, and
//                                                 `out` is visible to the leader once it returns
// SeqCtx (below) is the reference's order: one accumulator per term, items ascending.  TreeCtx is the order the refine kernel uses:
// SD_PNP_LEAVES leaves, leaf j takes items j, j + LEAVES, ... ascending, then inside every group of 64 leaves leaf[j] += leaf[j + s]
// for s = 32, 16, 8, 4, 2, 1, then (g0 + g1) + (g2 + g3).
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define SD_PNP_HD __host__ __device__ __forceinline__
#else
#define SD_PNP_HD inline
#endif

#define SD_PNP_LEAVES 256
#define SD_PNP_SVD_SWEEPS 30

namespace sdpnp {

constexpr double kEps = 2.220446049250313e-16;     // DBL_EPSILON

SD_PNP_HD double dabs(double x) { return x < 0 ? -x : x; }

SD_PNP_HD unsigned long long splitmix64(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The four indices iteration `it` (1-based) draws (PnP:188-201).  Draw d is splitmix64(splitmix64(seed) + 4 it + d) modulo the CURRENT
// size N - d; the swap-with-back removal is followed on a sparse copy of vAvailableIndices: only the (at most three) overwritten
// positions are kept, the latest write first.  N >= 4.
SD_PNP_HD void sample4(unsigned long long seed, int it, int N, int idx[4])
{
    const unsigned long long base = splitmix64(seed) + ((unsigned long long)it << 2);
    int pos[3], val[3];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int d = 0; d < 4; d++) {
        const int size = N - d;
        const int r = (int)(splitmix64(base + (unsigned long long)d) % (unsigned long long)size);
        int vr = r, vb = size - 1;
        bool fr = false, fb = false;
        for (int k = d - 1; k >= 0; k--) {
            if (!fr && pos[k] == r) { vr = val[k]; fr = true; }
            if (!fb && pos[k] == size - 1) { vb = val[k]; fb = true; }
        }
        idx[d] = vr;
        if (d < 3) { pos[d] = r; val[d] = vb; }
    }
}

// CheckInliers for one correspondence (PnP:314-329) as typed: mRi / mti / fu .. vc are double, the point is float; Xc, Yc, invZc are
// narrowed to float, ue / ve stay double, distX / distY / error2 are float.  Zc == 0 and NaN need no branch: the comparison is false.
SD_PNP_HD bool check_inlier(const double* R, const double* t, float X, float Y, float Z, float u, float v, double fu, double fv, double uc,
                            double vc, float maxError)
{
    const float Xc = (float)(R[0] * (double)X + R[1] * (double)Y + R[2] * (double)Z + t[0]);
    const float Yc = (float)(R[3] * (double)X + R[4] * (double)Y + R[5] * (double)Z + t[1]);
    const float invZc = (float)(1 / (R[6] * (double)X + R[7] * (double)Y + R[8] * (double)Z + t[2]));
    const double ue = uc + fu * (double)Xc * (double)invZc;
    const double ve = vc + fv * (double)Yc * (double)invZc;
    const float distX = (float)((double)u - ue);
    const float distY = (float)((double)v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < maxError;
}

// ---- the ONE singular value routine behind every cvSVD / cvInvert(CV_SVD) / cvSolve(CV_SVD)  [OpenCV-recall: frozen here] ----
// One-sided Jacobi (Hestenes) on the columns of W (m x n row-major, m >= n, n <= 12), V (n x n) accumulated from the identity.
//   order     pairs (p, q), p < q, p ascending then q ascending; at most SD_PNP_SVD_SWEEPS sweeps; a sweep that rotates nothing ends it
//   rotate    iff |g| > DBL_EPSILON sqrt(a b), with a = |w_p|^2, b = |w_q|^2, g = w_p . w_q summed over rows ascending
//   angle     P = 2 g, B = a - b, G = sqrt(P P + B B); B < 0: s = sqrt((G - B) / 2 / G), c = P / (G s 2); else c = sqrt((G + B) / (G 2)),
//             s = P / (G c 2); (w_p, w_q) <- (c w_p + s w_q, -s w_p + c w_q), the same on V's columns
//   values    w_j = sqrt(sum of squares of column j), rows ascending; perm lists the columns by descending w, the first of equal values
//             first (a NaN never moves forward).  Columns are not moved: singular triple r is (W[:, perm[r]] / w, w, V[:, perm[r]]).
//   signs     none is imposed: U and V carry whatever the rotations from V = I leave.
//   U         column j of U is W[:, j] / w_j, and zero when w_j == 0.  For the two SYMMETRIC matrices whose U^T the reference asks for
//             (PW0^T PW0 and M^T M) row r of "U^T" is V[:, perm[r]]: equal to the left vector wherever w > 0 and still orthonormal in the
//             null space, which is exactly what EPnP reads.
template <class WV, class VV>
SD_PNP_HD void svd(const int m, const int n, WV W, VV V, double* w, int* perm)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SD_PNP_SVD_SWEEPS; sweep++) {
        bool changed = false;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                double a = 0, b = 0, g = 0;
                for (int k = 0; k < m; k++) {
                    const double wp = W[k * n + p], wq = W[k * n + q];
                    a += wp * wp; b += wq * wq; g += wp * wq;
                }
                if (!(dabs(g) > kEps * sqrt(a * b))) continue;
                changed = true;
                const double P = g * 2, B = a - b, G = sqrt(P * P + B * B);
                double c, s;
                if (B < 0) { s = sqrt((G - B) * 0.5 / G); c = P / (G * s * 2); }
                else { c = sqrt((G + B) / (G * 2)); s = P / (G * c * 2); }
                for (int k = 0; k < m; k++) {
                    const double wp = W[k * n + p], wq = W[k * n + q];
                    W[k * n + p] = c * wp + s * wq; W[k * n + q] = c * wq - s * wp;
                }
                for (int k = 0; k < n; k++) {
                    const double vp = V[k * n + p], vq = V[k * n + q];
                    V[k * n + p] = c * vp + s * vq; V[k * n + q] = c * vq - s * vp;
                }
            }
        if (!changed) break;
    }
    for (int j = 0; j < n; j++) {
        double s = 0;
        for (int k = 0; k < m; k++) { const double x = W[k * n + j]; s += x * x; }
        w[j] = sqrt(s);
        perm[j] = j;
    }
    for (int j = 1; j < n; j++) {                                     // stable insertion: strictly larger moves forward
        const int pj = perm[j];
        int k = j;
        while (k > 0 && w[pj] > w[perm[k - 1]]) { perm[k] = perm[k - 1]; k--; }
        perm[k] = pj;
    }
}

// x = V diag(1 / w) U^T b over the singular values ABOVE the threshold 2 DBL_EPSILON (w_0 + .. + w_{n-1}), taken in perm order; the
// back-substitution of cvSolve / cvInvert  [OpenCV-recall]
template <class WV, class VV>
SD_PNP_HD void svd_backsub(const int m, const int n, WV W, VV V, const double* w, const int* perm, const double* b, double* x)
{
    double thr = 0;
    for (int j = 0; j < n; j++) thr += w[perm[j]];
    thr *= 2 * kEps;
    for (int i = 0; i < n; i++) x[i] = 0;
    for (int r = 0; r < n; r++) {
        const int j = perm[r];
        if (!(w[j] > thr)) continue;
        double d = 0;
        for (int k = 0; k < m; k++) d += W[k * n + j] * b[k];
        d = d / w[j] / w[j];
        for (int i = 0; i < n; i++) x[i] += V[i * n + j] * d;
    }
}

// cvSolve(A, b, x, CV_SVD) for the 6 x 4 / 6 x 3 / 6 x 5 systems of find_betas_approx_*
SD_PNP_HD void svd_solve(const int m, const int n, const double* A, const double* b, double* x)
{
    double W[30], V[25], w[5];
    int perm[5];
    for (int i = 0; i < m * n; i++) W[i] = A[i];
    svd(m, n, W, V, w, perm);
    svd_backsub(m, n, W, V, w, perm, b, x);
}

// qr_solve (PnP:860-950) on the 6 x 4 system of a Gauss-Newton step.  The reference leaves its `eta == 0` exit unset; here X keeps its
// previous value (zero before the first step).
SD_PNP_HD void qr_solve(double* pA, double* pb, double* pX)
{
    const int nr = 6, nc = 4;
    double A1[4], A2[4];
    for (int k = 0; k < nc; k++) {
        const int kk = k * nc + k;
        double eta = dabs(pA[kk]);
        for (int i = k + 1; i < nr; i++) {
            const double elt = dabs(pA[kk + (i - k - 1) * nc]);           // as typed: the pointer trails i by one row
            if (eta < elt) eta = elt;
        }
        if (eta == 0) return;
        double sum = 0;
        const double inv_eta = 1. / eta;
        for (int i = k; i < nr; i++) { pA[i * nc + k] *= inv_eta; sum += pA[i * nc + k] * pA[i * nc + k]; }
        double sigma = sqrt(sum);
        if (pA[kk] < 0) sigma = -sigma;
        pA[kk] += sigma;
        A1[k] = sigma * pA[kk];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double s2 = 0;
            for (int i = k; i < nr; i++) s2 += pA[i * nc + k] * pA[i * nc + j];
            const double tau = s2 / A1[k];
            for (int i = k; i < nr; i++) pA[i * nc + j] -= tau * pA[i * nc + k];
        }
    }
    for (int j = 0; j < nc; j++) {                                    // b <- Qt b
        double tau = 0;
        for (int i = j; i < nr; i++) tau += pA[i * nc + j] * pb[i];
        tau /= A1[j];
        for (int i = j; i < nr; i++) pb[i] -= tau * pA[i * nc + j];
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];                             // X = R-1 b
    for (int i = nc - 2; i >= 0; i--) {
        double sum = 0;
        for (int j = i + 1; j < nc; j++) sum += pA[i * nc + j] * pX[j];
        pX[i] = (pb[i] - sum) / A2[i];
    }
}

struct Camera { double fu, fv, uc, vc; };

// Everything compute_pose keeps between its sums.  One per solve: per lane in the hypothesis kernel, in LDS in the refine kernel.
struct State {
    double cws[4][3], ci[9], L[60], rho[6], ccs[4][3], pc0[3], pw0[3];
    double Rs[3][9], ts[3][3], rep[3];
    double acc[12];          // a sum's result
    double w12[12];
    double R[9], t[3];       // the chosen pose
    int perm12[12];
    int winner;              // 1, 2 or 3: the beta approximation whose pose was chosen
    int flags;               // branches taken, for the oracle's counters (SD_PNP_F_*)
};
#define SD_PNP_F_B4_NEG 1        // find_betas_approx_1: b4[0] < 0
#define SD_PNP_F_B4_ZERO 2       // b4[0] == 0
#define SD_PNP_F_B3_1_NEG 4      // find_betas_approx_2: b3[1] < 0
#define SD_PNP_F_SIGN 8          // solve_for_sign flipped (any of the three)
#define SD_PNP_F_DET 16          // det < 0 (any of the three)

SD_PNP_HD double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SD_PNP_HD double dist2(const double* p1, const double* p2)
{
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

// alphas of one point (PnP:423-433), recomputed wherever the reference reads its table
SD_PNP_HD void alphas_of(const State& S, const double* pi, double* a)
{
    for (int j = 0; j < 3; j++)
        a[1 + j] = S.ci[3 * j] * (pi[0] - S.cws[0][0]) + S.ci[3 * j + 1] * (pi[1] - S.cws[0][1]) + S.ci[3 * j + 2] * (pi[2] - S.cws[0][2]);
    a[0] = 1.0 - a[1] - a[2] - a[3];
}

// pcs of one point (PnP:466-475) from the current ccs
SD_PNP_HD void pc_of(const State& S, const double* a, double* pc)
{
    for (int j = 0; j < 3; j++) pc[j] = a[0] * S.ccs[0][j] + a[1] * S.ccs[1][j] + a[2] * S.ccs[2][j] + a[3] * S.ccs[3][j];
}

// find_betas_approx_1 / _2 / _3 (PnP:667-758)
SD_PNP_HD void find_betas(int which, State& S, double* betas)
{
    double l[30], b[5];
    if (which == 1) {
        for (int i = 0; i < 6; i++) { l[4 * i] = S.L[10 * i]; l[4 * i + 1] = S.L[10 * i + 1]; l[4 * i + 2] = S.L[10 * i + 3]; l[4 * i + 3] = S.L[10 * i + 6]; }
        svd_solve(6, 4, l, S.rho, b);
        if (b[0] < 0) {
            S.flags |= SD_PNP_F_B4_NEG;
            betas[0] = sqrt(-b[0]); betas[1] = -b[1] / betas[0]; betas[2] = -b[2] / betas[0]; betas[3] = -b[3] / betas[0];
        } else {
            if (b[0] == 0) S.flags |= SD_PNP_F_B4_ZERO;
            betas[0] = sqrt(b[0]); betas[1] = b[1] / betas[0]; betas[2] = b[2] / betas[0]; betas[3] = b[3] / betas[0];
        }
        return;
    }
    const int nc = which == 2 ? 3 : 5;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < nc; j++) l[nc * i + j] = S.L[10 * i + j];
    svd_solve(6, nc, l, S.rho, b);
    if (b[0] < 0) { betas[0] = sqrt(-b[0]); betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0; }
    else { betas[0] = sqrt(b[0]); betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0; }
    if (b[1] < 0) { betas[0] = -betas[0]; if (which == 2) S.flags |= SD_PNP_F_B3_1_NEG; }
    betas[2] = which == 2 ? 0.0 : b[3] / betas[0];
    betas[3] = 0.0;
}

// gauss_newton (PnP:812-858): five steps
SD_PNP_HD void gauss_newton(const State& S, double* betas)
{
    double x[4] = {0, 0, 0, 0};
    for (int k = 0; k < 5; k++) {
        double A[24], b[6];
        for (int i = 0; i < 6; i++) {
            const double* rowL = S.L + i * 10;
            double* rowA = A + i * 4;
            rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            b[i] = S.rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] +
                               rowL[3] * betas[0] * betas[2] + rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                               rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] + rowL[8] * betas[2] * betas[3] +
                               rowL[9] * betas[3] * betas[3]);
        }
        qr_solve(A, b, x);
        for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
}

// compute_pose (PnP:477-525).  W / V: 144 doubles each, indexable with [] (the 12 x 12 M^T M and its V).  The pose lands in S.R / S.t
// (valid for every participant after the call when S is shared) and the mean reprojection error is returned by the leader's S.rep.
template <class C, class WV, class VV>
SD_PNP_HD void compute_pose(C& c, State& S, WV W, VV V, const Camera cam)
{
    const int n = c.n();
    // choose_control_points (PnP:375-409)
    c.template sum<3>(n, [&](int i, double* v) { double uv[2]; c.point(i, v, uv); }, S.acc);
    if (c.leader()) {
        S.flags = 0;
        for (int j = 0; j < 3; j++) S.cws[0][j] = S.acc[j] / n;
    }
    c.sync();
    // cvMulTransposed(PW0, PW0tPW0, 1)  [OpenCV-recall]: A^T A, the upper triangle summed over rows ascending, then mirrored
    c.template sum<6>(n, [&](int i, double* v) {
        double pw[3], uv[2];
        c.point(i, pw, uv);
        const double d0 = pw[0] - S.cws[0][0], d1 = pw[1] - S.cws[0][1], d2 = pw[2] - S.cws[0][2];
        v[0] = d0 * d0; v[1] = d0 * d1; v[2] = d0 * d2; v[3] = d1 * d1; v[4] = d1 * d2; v[5] = d2 * d2;
    }, S.acc);
    if (c.leader()) {
        double A3[9] = {S.acc[0], S.acc[1], S.acc[2], S.acc[1], S.acc[3], S.acc[4], S.acc[2], S.acc[4], S.acc[5]};
        double V3[9], w3[3];
        int p3[3];
        svd(3, 3, A3, V3, w3, p3);                                    // cvSVD(PW0tPW0, DC, UCt, 0, MODIFY_A | U_T)
        for (int i = 1; i < 4; i++) {
            const double k = sqrt(w3[p3[i - 1]] / n);
            for (int j = 0; j < 3; j++) S.cws[i][j] = S.cws[0][j] + k * V3[3 * j + p3[i - 1]];
        }
        // compute_barycentric_coordinates (PnP:411-421): cvInvert(CC, CC_inv, CV_SVD)
        double cc[9], e[3], x[3];
        for (int i = 0; i < 3; i++)
            for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = S.cws[j][i] - S.cws[0][i];
        svd(3, 3, cc, V3, w3, p3);
        for (int k = 0; k < 3; k++) {
            e[0] = k == 0 ? 1.0 : 0.0; e[1] = k == 1 ? 1.0 : 0.0; e[2] = k == 2 ? 1.0 : 0.0;
            svd_backsub(3, 3, cc, V3, w3, p3, e, x);
            S.ci[k] = x[0]; S.ci[3 + k] = x[1]; S.ci[6 + k] = x[2];
        }
        // compute_rho (PnP:802-810)
        S.rho[0] = dist2(S.cws[0], S.cws[1]); S.rho[1] = dist2(S.cws[0], S.cws[2]); S.rho[2] = dist2(S.cws[0], S.cws[3]);
        S.rho[3] = dist2(S.cws[1], S.cws[2]); S.rho[4] = dist2(S.cws[1], S.cws[3]); S.rho[5] = dist2(S.cws[2], S.cws[3]);
    }
    c.sync();
    // fill_M (PnP:436-451) and cvMulTransposed(M, MtM, 1): entry (a, b), b >= a, summed over M's 2 n rows ascending; one row of the
    // upper triangle per sum
    for (int a = 0; a < 12; a++) {
        c.template sum<12>(2 * n, [&](int r, double* v) {
            double pw[3], uv[2], al[4], mrow[12];
            c.point(r >> 1, pw, uv);
            alphas_of(S, pw, al);
            for (int i = 0; i < 4; i++) {
                if ((r & 1) == 0) { mrow[3 * i] = al[i] * cam.fu; mrow[3 * i + 1] = 0.0; mrow[3 * i + 2] = al[i] * (cam.uc - uv[0]); }
                else { mrow[3 * i] = 0.0; mrow[3 * i + 1] = al[i] * cam.fv; mrow[3 * i + 2] = al[i] * (cam.vc - uv[1]); }
            }
            for (int b = 0; b < 12; b++) v[b] = b >= a ? mrow[a] * mrow[b] : 0.0;
        }, S.acc);
        if (c.leader())
            for (int b = a; b < 12; b++) { W[a * 12 + b] = S.acc[b]; W[b * 12 + a] = S.acc[b]; }
        c.sync();
    }
    for (int which = 1; which <= 3; which++) {
        if (c.leader()) {
            if (which == 1) {
                svd(12, 12, W, V, S.w12, S.perm12);                   // cvSVD(MtM, D, Ut, 0, MODIFY_A | U_T): row r of Ut = V[:, perm12[r]]
                // compute_L_6x10 (PnP:760-800)
                double dv[4][6][3];
                for (int i = 0; i < 4; i++) {
                    const int col = S.perm12[11 - i];
                    int a = 0, b = 1;
                    for (int j = 0; j < 6; j++) {
                        dv[i][j][0] = V[(3 * a) * 12 + col] - V[(3 * b) * 12 + col];
                        dv[i][j][1] = V[(3 * a + 1) * 12 + col] - V[(3 * b + 1) * 12 + col];
                        dv[i][j][2] = V[(3 * a + 2) * 12 + col] - V[(3 * b + 2) * 12 + col];
                        b++;
                        if (b > 3) { a++; b = a + 1; }
                    }
                }
                for (int i = 0; i < 6; i++) {
                    double* row = S.L + 10 * i;
                    row[0] = dot3(dv[0][i], dv[0][i]);
                    row[1] = 2.0 * dot3(dv[0][i], dv[1][i]);
                    row[2] = dot3(dv[1][i], dv[1][i]);
                    row[3] = 2.0 * dot3(dv[0][i], dv[2][i]);
                    row[4] = 2.0 * dot3(dv[1][i], dv[2][i]);
                    row[5] = dot3(dv[2][i], dv[2][i]);
                    row[6] = 2.0 * dot3(dv[0][i], dv[3][i]);
                    row[7] = 2.0 * dot3(dv[1][i], dv[3][i]);
                    row[8] = 2.0 * dot3(dv[2][i], dv[3][i]);
                    row[9] = dot3(dv[3][i], dv[3][i]);
                }
            }
            double betas[4];
            find_betas(which, S, betas);
            gauss_newton(S, betas);
            // compute_ccs (PnP:453-464)
            for (int i = 0; i < 4; i++) S.ccs[i][0] = S.ccs[i][1] = S.ccs[i][2] = 0.0;
            for (int i = 0; i < 4; i++) {
                const int col = S.perm12[11 - i];
                for (int j = 0; j < 4; j++)
                    for (int k = 0; k < 3; k++) S.ccs[j][k] += betas[i] * V[(3 * j + k) * 12 + col];
            }
            // solve_for_sign (PnP:636-649): pcs[2] of the FIRST point only; negating ccs negates every pc exactly
            double pw[3], uv[2], al[4], pc[3];
            c.point(0, pw, uv);
            alphas_of(S, pw, al);
            pc_of(S, al, pc);
            if (pc[2] < 0.0) {
                S.flags |= SD_PNP_F_SIGN;
                for (int i = 0; i < 4; i++)
                    for (int j = 0; j < 3; j++) S.ccs[i][j] = -S.ccs[i][j];
            }
        }
        c.sync();
        // estimate_R_and_t (PnP:569-627)
        c.template sum<6>(n, [&](int i, double* v) {
            double pw[3], uv[2], al[4];
            c.point(i, pw, uv);
            alphas_of(S, pw, al);
            pc_of(S, al, v);
            v[3] = pw[0]; v[4] = pw[1]; v[5] = pw[2];
        }, S.acc);
        if (c.leader())
            for (int j = 0; j < 3; j++) { S.pc0[j] = S.acc[j] / n; S.pw0[j] = S.acc[3 + j] / n; }
        c.sync();
        c.template sum<9>(n, [&](int i, double* v) {
            double pw[3], uv[2], al[4], pc[3];
            c.point(i, pw, uv);
            alphas_of(S, pw, al);
            pc_of(S, al, pc);
            for (int j = 0; j < 3; j++) {
                v[3 * j] = (pc[j] - S.pc0[j]) * (pw[0] - S.pw0[0]);
                v[3 * j + 1] = (pc[j] - S.pc0[j]) * (pw[1] - S.pw0[1]);
                v[3 * j + 2] = (pc[j] - S.pc0[j]) * (pw[2] - S.pw0[2]);
            }
        }, S.acc);
        if (c.leader()) {
            double abt[9], V3[9], w3[3], U[9];
            int p3[3];
            for (int k = 0; k < 9; k++) abt[k] = S.acc[k];
            svd(3, 3, abt, V3, w3, p3);                               // cvSVD(ABt, D, U, V, MODIFY_A): U, V untransposed, columns in perm order
            for (int r = 0; r < 3; r++)
                for (int k = 0; k < 3; k++) {
                    const int j = p3[k];
                    U[3 * r + k] = w3[j] == 0 ? 0.0 : abt[3 * r + j] / w3[j];
                }
            double* R = S.Rs[which - 1];
            double* t = S.ts[which - 1];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++)
                    R[3 * i + j] = U[3 * i] * V3[3 * j + p3[0]] + U[3 * i + 1] * V3[3 * j + p3[1]] + U[3 * i + 2] * V3[3 * j + p3[2]];
            const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] -
                               R[0] * R[5] * R[7];
            if (det < 0) { S.flags |= SD_PNP_F_DET; R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
            t[0] = S.pc0[0] - dot3(R, S.pw0);
            t[1] = S.pc0[1] - dot3(R + 3, S.pw0);
            t[2] = S.pc0[2] - dot3(R + 6, S.pw0);
        }
        c.sync();
        // reprojection_error (PnP:550-567)
        c.template sum<1>(n, [&](int i, double* v) {
            double pw[3], uv[2];
            c.point(i, pw, uv);
            const double* R = S.Rs[which - 1];
            const double* t = S.ts[which - 1];
            const double Xc = dot3(R, pw) + t[0];
            const double Yc = dot3(R + 3, pw) + t[1];
            const double inv_Zc = 1.0 / (dot3(R + 6, pw) + t[2]);
            const double ue = cam.uc + cam.fu * Xc * inv_Zc;
            const double ve = cam.vc + cam.fv * Yc * inv_Zc;
            v[0] = sqrt((uv[0] - ue) * (uv[0] - ue) + (uv[1] - ve) * (uv[1] - ve));
        }, S.acc);
        if (c.leader()) S.rep[which - 1] = S.acc[0] / n;
        c.sync();
    }
    if (c.leader()) {
        int N = 1;
        if (S.rep[1] < S.rep[0]) N = 2;
        if (S.rep[2] < S.rep[N - 1]) N = 3;
        S.winner = N;
        for (int k = 0; k < 9; k++) S.R[k] = S.Rs[N - 1][k];
        for (int k = 0; k < 3; k++) S.t[k] = S.ts[N - 1][k];
    }
    c.sync();
}

// ---- the two orders of a sum that need no GPU ----
// Set: what a solve runs over -- `n` rows of pts (x y z u v maxError, 6 floats each), through `index` when it is not null.
struct PointSet {
    const float* pts; const int* index; int count;
    SD_PNP_HD void get(int i, double* pw, double* uv) const
    {
        const float* p = pts + 6 * (size_t)(index ? index[i] : i);
        pw[0] = p[0]; pw[1] = p[1]; pw[2] = p[2]; uv[0] = p[3]; uv[1] = p[4];
    }
};

struct SeqCtx {
    PointSet set;
    SD_PNP_HD int n() const { return set.count; }
    SD_PNP_HD void point(int i, double* pw, double* uv) const { set.get(i, pw, uv); }
    SD_PNP_HD bool leader() const { return true; }
    SD_PNP_HD void sync() const {}
    template <int K, class F>
    SD_PNP_HD void sum(int count, F f, double* out) const
    {
        double acc[K], v[K];
        for (int k = 0; k < K; k++) acc[k] = 0;
        for (int i = 0; i < count; i++) {
            f(i, v);
            for (int k = 0; k < K; k++) acc[k] += v[k];
        }
        for (int k = 0; k < K; k++) out[k] = acc[k];
    }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// the refine kernel's order, restated sequentially (the kernel itself is k_pnp.h's BlockCtx)
struct TreeCtx {
    PointSet set;
    int n() const { return set.count; }
    void point(int i, double* pw, double* uv) const { set.get(i, pw, uv); }
    bool leader() const { return true; }
    void sync() const {}
    template <int K, class F>
    void sum(int count, F f, double* out) const
    {
        static thread_local double leaf[SD_PNP_LEAVES][12];
        double v[K];
        for (int j = 0; j < SD_PNP_LEAVES; j++) {
            for (int k = 0; k < K; k++) leaf[j][k] = 0;
            for (int i = j; i < count; i += SD_PNP_LEAVES) {
                f(i, v);
                for (int k = 0; k < K; k++) leaf[j][k] += v[k];
            }
        }
        for (int g = 0; g < SD_PNP_LEAVES; g += 64)
            for (int s = 32; s >= 1; s >>= 1)
                for (int j = 0; j < s; j++)
                    for (int k = 0; k < K; k++) leaf[g + j][k] += leaf[g + j + s][k];
        for (int k = 0; k < K; k++) out[k] = (leaf[0][k] + leaf[64][k]) + (leaf[128][k] + leaf[192][k]);
    }
};
#endif

}  // namespace sdpnp
