// Independent CPU oracle of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778) from initializeOptimization() on, and of the
// pieces of the vendored g2o it runs: OptimizationAlgorithmLevenberg::solve, SparseOptimizer::optimize / initializeOptimization(level),
// BaseBinaryEdge::constructQuadraticForm, RobustKernelHuber, the two two-vertex projection edges (types_six_dof_expmap.cpp:103-157,
// 188-310), BlockSolver_6_3::buildSystem / setLambda / solve (the Schur complement, block_solver.hpp:354-500), SE3Quat and
// Converter::toSE3Quat / toCvMat; then MapPoint::UpdateNormalAndDepth for the optimised points (DESIGN Q32-Q38).
// A literal, sequential f64 restatement: sums over edges run in insertion order, the Schur loop runs over landmarks in index order and
// over a landmark's pose blocks in pose order.  The reduced system is factorised by an unpivoted LDL^T in natural order that fails on a
// pivot equal to zero (what Eigen::SimplicialLDLT reports; its fill-reducing ordering changes rounding only and is not modelled).
// Shares no code with the device kernel (slam-dynamic_amd/csrc/k_ba.h).  Test infrastructure only: g++ -O2 -ffp-contract=off.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct KF { float Tcw[16]; float fx, fy, cx, cy, mbf; uint8_t fixed; uint8_t pad[3]; };          // sd_ba_keyframe
struct Edge { int32_t kf, point; float u, v, ur, inv_sigma2; int32_t tag, reserved; };             // sd_ba_edge
struct Stats { int32_t iterations[2], trials[2], rejected[2]; int32_t n_level1, n_erased; double chi2[2]; };   // sd_ba_stats
static_assert(sizeof(KF) == 88 && sizeof(Edge) == 32 && sizeof(Stats) == 48, "records");

enum { B_MONO, B_STEREO, B_FIXED_LOCAL, B_EDGE_TO_FIXED, B_SINGLE_MONO, B_LEVEL1_CHI2, B_LEVEL1_DEPTH, B_POINT_INACTIVE, B_KF_INACTIVE,
       B_REJECTED, B_STOP_NBAD, B_STOP_TERMINATE, B_NOOP, B_HUBER, B_POSE_POSE, B_FACTOR_FAIL, B_ERASE_CHI2, B_ERASE_DEPTH, B_ROUND2_EMPTY,
       B_FIXED_PLUS_ONE_LOCAL, B_NO_POSE, B_DUPLICATE,
       // info slots of the crafted cases (tests/ba_crafted.py): the last LM trial of round 1 / 2 was rejected; level-1 edges whose point
       // stays active in round 2; stereo edges linearised in round 1 with 5.991 < chi2 <= 7.815; Quaterniond(Matrix3d) branches taken
       B_LAST_REJECTED_R1, B_LAST_REJECTED_R2, B_LEVEL1_POINT_ACTIVE, B_STEREO_BETWEEN, B_QUAT_TR, B_QUAT_I0, B_QUAT_I1, B_QUAT_I2, B_COUNT };
int64_t g_branch[B_COUNT];
// The deliberately wrong twins (`flags` of sd_ba_oracle; 0 = the oracle).  Each makes one mistake a restatement of Optimizer.cc:453-778
// could make; tests/test_ba_crafted.py shows that each differs from the oracle on the crafted case named for it.
enum { T_F32_COMPARE = 1,       // classification as PoseOptimization does it: (float)chi2 > (float)bound
       T_NO_DEPTH_TEST = 2,     // drops !isDepthPositive()
       T_FRESH_CHI2 = 4,        // recomputes every edge's error at the current estimates before each classification
       T_LEVEL1_ACTIVE = 8,     // round 2 runs over all edges
       T_LAMBDA_CARRIED = 16,   // round 2 starts from round 1's lambda, nu and stop counter
       T_DELTA_SWAPPED = 32 };  // stereo edges get the mono Huber delta
int g_flags = 0;
std::vector<double> g_round1_points;                      // the point estimates of the last call when round 1 ended (test hook)

struct Quat { double x, y, z, w; };
struct SE3 { Quat r; double t[3]; };

void normalize_rotation(Quat& q)
{
    if (q.w < 0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
    const double n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    if (n2 > 0) { const double n = std::sqrt(n2); q.x /= n; q.y /= n; q.z /= n; q.w /= n; }
}
Quat q_from_matrix(const double m[3][3])
{
    Quat q;
    double c[3];
    const double tr = m[0][0] + m[1][1] + m[2][2];
    if (tr > 0) {
        g_branch[B_QUAT_TR]++;
        double t = std::sqrt(tr + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (m[2][1] - m[1][2]) * t; q.y = (m[0][2] - m[2][0]) * t; q.z = (m[1][0] - m[0][1]) * t;
        return q;
    }
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > m[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    g_branch[B_QUAT_I0 + i]++;
    double t = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
    c[i] = 0.5 * t;
    t = 0.5 / t;
    q.w = (m[k][j] - m[j][k]) * t;
    c[j] = (m[j][i] + m[i][j]) * t;
    c[k] = (m[k][i] + m[i][k]) * t;
    q.x = c[0]; q.y = c[1]; q.z = c[2];
    return q;
}
Quat q_mul(const Quat& a, const Quat& b)
{
    Quat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}
void q_rotate(const Quat& q, const double v[3], double out[3])
{
    double uv[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    const double c[3] = {q.y * uv[2] - q.z * uv[1], q.z * uv[0] - q.x * uv[2], q.x * uv[1] - q.y * uv[0]};
    for (int i = 0; i < 3; i++) out[i] = v[i] + q.w * uv[i] + c[i];
}
void q_to_matrix(const Quat& q, double R[3][3])
{
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz;       R[0][2] = txz + twy;
    R[1][0] = txy + twz;       R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy;       R[2][1] = tyz + twx;       R[2][2] = 1 - (txx + tyy);
}
SE3 se3_from_rt(const double R[3][3], const double t[3])
{
    SE3 s;
    s.r = q_from_matrix(R);
    s.t[0] = t[0]; s.t[1] = t[1]; s.t[2] = t[2];
    normalize_rotation(s.r);
    return s;
}
SE3 se3_mul(const SE3& a, const SE3& b)
{
    SE3 r = a;
    double rb[3];
    q_rotate(a.r, b.t, rb);
    for (int i = 0; i < 3; i++) r.t[i] += rb[i];
    r.r = q_mul(a.r, b.r);
    normalize_rotation(r.r);
    return r;
}
SE3 se3_exp(const double u[6])
{
    const double w[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]};
    const double theta = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double Om[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
    double Om2[3][3], R[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Om2[i][j] = Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j];
    if (theta < 0.00001) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = V[i][j] = ((i == j ? 1.0 : 0.0) + Om[i][j]) + Om2[i][j];
    } else {
        const double a = std::sin(theta) / theta, b = (1 - std::cos(theta)) / (theta * theta), c = (theta - std::sin(theta)) / std::pow(theta, 3);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                R[i][j] = ((i == j ? 1.0 : 0.0) + a * Om[i][j]) + b * Om2[i][j];
                V[i][j] = ((i == j ? 1.0 : 0.0) + b * Om[i][j]) + c * Om2[i][j];
            }
    }
    double t[3];
    for (int i = 0; i < 3; i++) t[i] = V[i][0] * up[0] + V[i][1] * up[1] + V[i][2] * up[2];
    return se3_from_rt(R, t);
}
SE3 to_se3quat(const float* T)
{
    double R[3][3], t[3];
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R[i][j] = T[i * 4 + j]; t[i] = T[i * 4 + 3]; }
    return se3_from_rt(R, t);
}
void to_cvmat(const SE3& s, float* T)
{
    double R[3][3];
    q_to_matrix(s.r, R);
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T[i * 4 + j] = (float)R[i][j]; T[i * 4 + 3] = (float)s.t[i]; }
    T[12] = T[13] = T[14] = 0.f; T[15] = 1.f;
}

struct Graph {
    int nKF, nLocal, nPt, nE;
    const KF* kf; const Edge* E;
    std::vector<SE3> pose; std::vector<double> X;          // estimates
    std::vector<uint8_t> level;                            // per edge
    std::vector<double> chi2c;                             // the edges' cached chi2 (error of the last computeActiveErrors that saw them)
    bool robust;
    double lambda; int ni, nBad;                           // LM state at the end of the last optimize() (read by T_LAMBDA_CARRIED only)
    // per round
    std::vector<int> poseIdx, ptIdx;                       // index in Hpp / Hll, -1 when fixed or inactive
    int nPose, nLm;
};

void transform(const Graph& G, const Edge& e, double p[3])
{
    q_rotate(G.pose[e.kf].r, &G.X[3 * e.point], p);
    for (int i = 0; i < 3; i++) p[i] = p[i] + G.pose[e.kf].t[i];
}
int edge_error(const Graph& G, const Edge& e, double r[3], double p[3])
{
    const KF& k = G.kf[e.kf];
    const double fx = k.fx, fy = k.fy, cx = k.cx, cy = k.cy, bf = k.mbf;
    transform(G, e, p);
    if (e.ur < 0) {
        r[0] = (double)e.u - ((p[0] / p[2]) * fx + cx);
        r[1] = (double)e.v - ((p[1] / p[2]) * fy + cy);
        r[2] = 0;
        return 2;
    }
    const double invz = (double)(float)(1.0 / p[2]);       // const float invz = 1.0f/trans_xyz[2]
    const double r0 = p[0] * invz * fx + cx;
    r[0] = (double)e.u - r0;
    r[1] = (double)e.v - (p[1] * invz * fy + cy);
    r[2] = (double)e.ur - (r0 - bf * invz);
    return 3;
}
double chi2_of(const double r[3], int D, double w)
{
    double s = r[0] * (w * r[0]) + r[1] * (w * r[1]);
    if (D == 3) s = s + r[2] * (w * r[2]);
    return s;
}
// linearizeOplus: A = d e / d point (D x 3), B = d e / d pose (D x 6)
void edge_jacobians(const Graph& G, const Edge& e, int D, double A[3][3], double B[3][6])
{
    const KF& k = G.kf[e.kf];
    const double fx = k.fx, fy = k.fy, bf = k.mbf;
    double p[3], R[3][3];
    transform(G, e, p);
    q_to_matrix(G.pose[e.kf].r, R);
    const double x = p[0], y = p[1], z = p[2], z_2 = z * z;
    if (D == 2) {
        const double s = -1. / z;
        const double M[2][3] = {{s * fx, s * 0.0, s * (-x / z * fx)}, {s * 0.0, s * fy, s * (-y / z * fy)}};
        for (int r = 0; r < 2; r++)
            for (int c = 0; c < 3; c++) A[r][c] = (M[r][0] * R[0][c] + M[r][1] * R[1][c]) + M[r][2] * R[2][c];
        for (int c = 0; c < 3; c++) A[2][c] = 0;
    } else {
        for (int c = 0; c < 3; c++) {
            A[0][c] = -fx * R[0][c] / z + fx * x * R[2][c] / z_2;
            A[1][c] = -fy * R[1][c] / z + fy * y * R[2][c] / z_2;
            A[2][c] = A[0][c] - bf * R[2][c] / z_2;
        }
    }
    B[0][0] = x * y / z_2 * fx; B[0][1] = -(1 + (x * x / z_2)) * fx; B[0][2] = y / z * fx;
    B[0][3] = -1. / z * fx;     B[0][4] = 0;                         B[0][5] = x / z_2 * fx;
    B[1][0] = (1 + y * y / z_2) * fy; B[1][1] = -x * y / z_2 * fy; B[1][2] = -x / z * fy;
    B[1][3] = 0;                      B[1][4] = -1. / z * fy;      B[1][5] = y / z_2 * fy;
    if (D == 3) {
        B[2][0] = B[0][0] - bf * y / z_2; B[2][1] = B[0][1] + bf * x / z_2; B[2][2] = B[0][2];
        B[2][3] = B[0][3];                B[2][4] = 0;                      B[2][5] = B[0][5] - bf / z_2;
    } else {
        for (int c = 0; c < 6; c++) B[2][c] = 0;
    }
}

const double kDeltaMono = (double)(float)std::sqrt(5.991), kDeltaStereo = (double)(float)std::sqrt(7.815);
double delta_of(int D) { return D == 2 || (g_flags & T_DELTA_SWAPPED) ? kDeltaMono : kDeltaStereo; }

// computeActiveErrors + activeRobustChi2
double active_chi(Graph& G)
{
    double chi = 0;
    for (int i = 0; i < G.nE; i++) {
        if (G.level[i]) continue;
        double r[3], p[3];
        const int D = edge_error(G, G.E[i], r, p);
        const double c2 = chi2_of(r, D, (double)G.E[i].inv_sigma2);
        G.chi2c[i] = c2;
        if (G.robust) {
            const double d = delta_of(D), dsqr = d * d;
            chi += c2 <= dsqr ? c2 : 2 * std::sqrt(c2) * d - dsqr;
        } else chi += c2;
    }
    return chi;
}

struct PLBlock { int pose; double W[6][3]; };
struct System {
    std::vector<double> Hpp, bp, Hll, bl;                   // nPose x 36, nPose x 6, nLm x 9, nLm x 3
    std::vector<std::vector<PLBlock>> Hpl;                  // per landmark, sorted by pose
};

void build_system(Graph& G, System& Y)
{
    Y.Hpp.assign((size_t)G.nPose * 36, 0.0); Y.bp.assign((size_t)G.nPose * 6, 0.0);
    Y.Hll.assign((size_t)G.nLm * 9, 0.0); Y.bl.assign((size_t)G.nLm * 3, 0.0);
    Y.Hpl.assign(G.nLm, {});
    for (int n = 0; n < G.nE; n++) {
        if (G.level[n]) continue;
        const Edge& e = G.E[n];
        double r[3], p[3], A[3][3], B[3][6];
        const int D = edge_error(G, e, r, p);
        edge_jacobians(G, e, D, A, B);
        const double w = (double)e.inv_sigma2;
        double rho1 = 1.0;
        if (G.robust) {
            const double c2 = chi2_of(r, D, w), d = delta_of(D), dsqr = d * d;
            if (D == 3 && c2 > 5.991 && c2 <= 7.815) g_branch[B_STEREO_BETWEEN]++;
            if (!(c2 <= dsqr)) { rho1 = d / std::sqrt(c2); g_branch[B_HUBER]++; }
        }
        const double wo = G.robust ? rho1 * w : w;
        double orr[3];                                     // omega_r = -omega * error (* rho[1])
        for (int k = 0; k < D; k++) { orr[k] = -(w * r[k]); if (G.robust) orr[k] *= rho1; }
        const int li = G.ptIdx[e.point], pi = G.poseIdx[e.kf];
        {                                                  // the point is never fixed
            double* H = &Y.Hll[(size_t)li * 9]; double* b = &Y.bl[(size_t)li * 3];
            for (int i = 0; i < 3; i++) {
                double g = A[0][i] * orr[0];
                for (int k = 1; k < D; k++) g = g + A[k][i] * orr[k];
                b[i] += g;
                for (int j = 0; j < 3; j++) {
                    double h = (A[0][i] * wo) * A[0][j];
                    for (int k = 1; k < D; k++) h = h + (A[k][i] * wo) * A[k][j];
                    H[i * 3 + j] += h;
                }
            }
        }
        if (pi >= 0) {
            double* H = &Y.Hpp[(size_t)pi * 36]; double* b = &Y.bp[(size_t)pi * 6];
            for (int i = 0; i < 6; i++) {
                double g = B[0][i] * orr[0];
                for (int k = 1; k < D; k++) g = g + B[k][i] * orr[k];
                b[i] += g;
                for (int j = 0; j < 6; j++) {
                    double h = (B[0][i] * wo) * B[0][j];
                    for (int k = 1; k < D; k++) h = h + (B[k][i] * wo) * B[k][j];
                    H[i * 6 + j] += h;
                }
            }
            std::vector<PLBlock>& col = Y.Hpl[li];
            PLBlock* blk = nullptr;
            for (PLBlock& q : col) if (q.pose == pi) { blk = &q; g_branch[B_DUPLICATE]++; }
            if (!blk) { col.push_back(PLBlock{pi, {}}); blk = &col.back(); }
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < 3; j++) {
                    double h = G.robust ? (B[0][i] * wo) * A[0][j] : B[0][i] * (A[0][j] * w);
                    for (int k = 1; k < D; k++) h = h + (G.robust ? (B[k][i] * wo) * A[k][j] : B[k][i] * (A[k][j] * w));
                    blk->W[i][j] += h;
                }
        }
    }
    for (auto& col : Y.Hpl) std::sort(col.begin(), col.end(), [](const PLBlock& a, const PLBlock& b) { return a.pose < b.pose; });
}

void inverse3(const double m[9], double inv[9])            // Eigen's 3x3 inverse: cofactors over the determinant
{
    double cof[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            cof[i][j] = m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
        }
    const double det = (cof[0][0] * m[0] + cof[1][0] * m[3]) + cof[2][0] * m[6];
    const double invdet = 1.0 / det;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) inv[j * 3 + i] = cof[i][j] * invdet;
}

// BlockSolver::solve with lambda on both diagonals; x = [poses | landmarks]; returns false when the factorisation fails
bool solve_system(const Graph& G, const System& Y, double lambda, std::vector<double>& x)
{
    const int n = 6 * G.nPose;
    std::vector<double> S((size_t)n * n, 0.0), coef(n, 0.0), Dinv((size_t)G.nLm * 9);
    for (int p = 0; p < G.nPose; p++)
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) S[(size_t)(6 * p + i) * n + 6 * p + j] = Y.Hpp[(size_t)p * 36 + i * 6 + j] + (i == j ? lambda : 0.0);
    for (int l = 0; l < G.nLm; l++) {
        double D[9];
        for (int k = 0; k < 9; k++) D[k] = Y.Hll[(size_t)l * 9 + k];
        D[0] += lambda; D[4] += lambda; D[8] += lambda;
        double* Di = &Dinv[(size_t)l * 9];
        inverse3(D, Di);
        double db[3];
        for (int i = 0; i < 3; i++) db[i] = (Di[i * 3] * Y.bl[l * 3] + Di[i * 3 + 1] * Y.bl[l * 3 + 1]) + Di[i * 3 + 2] * Y.bl[l * 3 + 2];
        const std::vector<PLBlock>& col = Y.Hpl[l];
        for (size_t a = 0; a < col.size(); a++) {
            const int i1 = col[a].pose;
            double BD[6][3];
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < 3; j++) BD[i][j] = (col[a].W[i][0] * Di[j] + col[a].W[i][1] * Di[3 + j]) + col[a].W[i][2] * Di[6 + j];
            for (int i = 0; i < 6; i++) coef[6 * i1 + i] += (col[a].W[i][0] * db[0] + col[a].W[i][1] * db[1]) + col[a].W[i][2] * db[2];
            for (size_t b = a; b < col.size(); b++) {
                const int i2 = col[b].pose;
                if (i2 != i1) g_branch[B_POSE_POSE]++;
                for (int i = 0; i < 6; i++)
                    for (int j = 0; j < 6; j++)
                        S[(size_t)(6 * i1 + i) * n + 6 * i2 + j] -= (BD[i][0] * col[b].W[j][0] + BD[i][1] * col[b].W[j][1]) + BD[i][2] * col[b].W[j][2];
            }
        }
    }
    std::vector<double> bs(n);
    for (int i = 0; i < n; i++) bs[i] = Y.bp[i] - coef[i];
    // LDL^T of the upper triangle of S (L = U^T), natural order
    std::vector<double> L((size_t)n * n, 0.0), d(n);
    for (int j = 0; j < n; j++) {
        double s = S[(size_t)j * n + j];
        for (int k = 0; k < j; k++) s -= (L[(size_t)j * n + k] * L[(size_t)j * n + k]) * d[k];
        d[j] = s;
        if (s == 0.0) { g_branch[B_FACTOR_FAIL]++; return false; }
        for (int i = j + 1; i < n; i++) {
            double t = S[(size_t)j * n + i];
            for (int k = 0; k < j; k++) t -= (L[(size_t)i * n + k] * L[(size_t)j * n + k]) * d[k];
            L[(size_t)i * n + j] = t / s;
        }
    }
    for (int i = 0; i < n; i++) { double s = bs[i]; for (int k = 0; k < i; k++) s -= L[(size_t)i * n + k] * x[k]; x[i] = s; }
    for (int i = 0; i < n; i++) x[i] = x[i] / d[i];
    for (int i = n - 1; i >= 0; i--) { double s = x[i]; for (int k = i + 1; k < n; k++) s -= L[(size_t)k * n + i] * x[k]; x[i] = s; }
    // landmarks: xl = Dinv (bl - Hpl^T xp)
    for (int l = 0; l < G.nLm; l++) {
        double cl[3] = {Y.bl[l * 3], Y.bl[l * 3 + 1], Y.bl[l * 3 + 2]};
        for (const PLBlock& q : Y.Hpl[l])
            for (int j = 0; j < 3; j++)
                for (int i = 0; i < 6; i++) cl[j] += q.W[i][j] * -x[6 * q.pose + i];
        const double* Di = &Dinv[(size_t)l * 9];
        for (int i = 0; i < 3; i++) x[n + 3 * l + i] = (Di[i * 3] * cl[0] + Di[i * 3 + 1] * cl[1]) + Di[i * 3 + 2] * cl[2];
    }
    return true;
}

struct Margins { double chi2, depth, rho, stop; };
void margin_min(double& m, double v) { if (v < m) m = v; }

// initializeOptimization(level 0) + optimize(maxIt)
void optimize(Graph& G, int maxIt, int round, Stats& st, Margins& mg)
{
    // active vertices: those with a level-0 edge; the index mapping holds the non-fixed ones, poses then landmarks, in table order
    std::vector<int> kfEdges(G.nKF, 0), ptEdges(G.nPt, 0);
    int nActive = 0;
    for (int i = 0; i < G.nE; i++) if (!G.level[i]) { kfEdges[G.E[i].kf]++; ptEdges[G.E[i].point]++; nActive++; }
    G.poseIdx.assign(G.nKF, -1); G.ptIdx.assign(G.nPt, -1);
    G.nPose = G.nLm = 0;
    for (int k = 0; k < G.nKF; k++) {
        const bool fixed = k >= G.nLocal || G.kf[k].fixed;
        if (kfEdges[k] && !fixed) G.poseIdx[k] = G.nPose++;
        if (round == 1 && k < G.nLocal && !fixed && !kfEdges[k]) g_branch[B_KF_INACTIVE]++;
    }
    for (int p = 0; p < G.nPt; p++) {
        if (ptEdges[p]) G.ptIdx[p] = G.nLm++;
        else if (round == 1) g_branch[B_POINT_INACTIVE]++;
    }
    st.iterations[round] = st.trials[round] = st.rejected[round] = 0;
    st.chi2[round] = 0;
    if (nActive == 0) { if (round == 1) g_branch[B_ROUND2_EMPTY]++; return; }     // "0 vertices to optimize"
    if (G.nPose == 0) g_branch[B_NO_POSE]++;
    const int n6 = 6 * G.nPose, nx = n6 + 3 * G.nLm;
    std::vector<double> x(nx, 0.0), xs(nx);
    System Y;
    const bool carried = (g_flags & T_LAMBDA_CARRIED) && round == 1;
    double lambda = carried ? G.lambda : 0;
    int ni = carried ? G.ni : 2, nBad = carried ? G.nBad : 0;
    double currentChi = 0;
    bool lastRejected = false;
    for (int it = 0; it < maxIt; it++) {
        st.iterations[round]++;
        currentChi = active_chi(G);
        const double iniChi = currentChi;
        build_system(G, Y);
        if (it == 0 && !carried) {
            double md = 0;
            for (int p = 0; p < G.nPose; p++) for (int j = 0; j < 6; j++) md = std::max(std::fabs(Y.Hpp[(size_t)p * 36 + j * 7]), md);
            for (int l = 0; l < G.nLm; l++) for (int j = 0; j < 3; j++) md = std::max(std::fabs(Y.Hll[(size_t)l * 9 + j * 4]), md);
            lambda = 1e-5 * md; ni = 2; nBad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const std::vector<SE3> poseBackup = G.pose;
            const std::vector<double> XBackup = G.X;
            xs = x;
            const bool ok2 = solve_system(G, Y, lambda, xs);
            if (ok2) x = xs;
            for (int k = 0; k < G.nKF; k++) if (G.poseIdx[k] >= 0) G.pose[k] = se3_mul(se3_exp(&x[6 * G.poseIdx[k]]), G.pose[k]);
            for (int p = 0; p < G.nPt; p++) if (G.ptIdx[p] >= 0) for (int j = 0; j < 3; j++) G.X[3 * p + j] += x[n6 + 3 * G.ptIdx[p] + j];
            double tempChi = active_chi(G);
            if (!ok2) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            double scale = 0;
            for (int j = 0; j < nx; j++) scale += x[j] * (lambda * x[j] + (j < n6 ? Y.bp[j] : Y.bl[j - n6]));
            scale += 1e-3;
            rho /= scale;
            margin_min(mg.rho, std::fabs(rho));
            st.trials[round]++;
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = std::min(alpha, 2. / 3.);
                lambda *= std::max(1. / 3., alpha);
                ni = 2;
                currentChi = tempChi;
                lastRejected = false;
            } else {
                lambda *= ni;
                ni *= 2;
                G.pose = poseBackup; G.X = XBackup;
                st.rejected[round]++;
                g_branch[B_REJECTED]++;
                lastRejected = true;
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        if (qmax == 10 || rho == 0) { g_branch[B_STOP_TERMINATE]++; break; }
        margin_min(mg.stop, std::fabs((iniChi - currentChi) * 1e3 - iniChi) / std::max(iniChi, DBL_MIN));
        if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
        if (nBad >= 3) { g_branch[B_STOP_NBAD]++; break; }
    }
    st.chi2[round] = currentChi;
    G.lambda = lambda; G.ni = ni; G.nBad = nBad;
    if (lastRejected) g_branch[B_LAST_REJECTED_R1 + round]++;
}

// T_FRESH_CHI2: the error of every edge at the current estimates, whatever its level
void refresh_chi2(Graph& G)
{
    for (int i = 0; i < G.nE; i++) {
        double r[3], p[3];
        const int D = edge_error(G, G.E[i], r, p);
        G.chi2c[i] = chi2_of(r, D, (double)G.E[i].inv_sigma2);
    }
}

// chi2() > bound || !isDepthPositive(): chi2 from the edge's cached error, the depth from the current estimates
bool classify(const Graph& G, int i, Margins& mg, int chiBranch, int depthBranch)
{
    const Edge& e = G.E[i];
    double p[3];
    transform(G, e, p);
    const double bound = e.ur < 0 ? 5.991 : 7.815;
    margin_min(mg.chi2, std::fabs(G.chi2c[i] - bound) / bound);
    margin_min(mg.depth, std::fabs(p[2]) / std::max(std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]), DBL_MIN));
    const bool c = (g_flags & T_F32_COMPARE) ? (float)G.chi2c[i] > (float)bound : G.chi2c[i] > bound;
    const bool dneg = (g_flags & T_NO_DEPTH_TEST) ? false : !(p[2] > 0.0);
    if (c) g_branch[chiBranch]++;
    if (dneg) g_branch[depthBranch]++;
    return c || dneg;
}

}  // namespace

// the f64 point estimates of the last sd_ba_oracle call at the end of round 1 (process-wide, like the branch counters); returns how many
extern "C" int sd_ba_oracle_round1_points(double* out, int cap)
{
    const int n = (int)std::min<size_t>(g_round1_points.size(), (size_t)cap);
    for (int i = 0; i < n; i++) out[i] = g_round1_points[i];
    return n;
}
extern "C" int sd_ba_oracle_branch_count() { return B_COUNT; }
extern "C" int64_t* sd_ba_oracle_branches() { return g_branch; }
extern "C" void sd_ba_oracle_reset_branches() { std::memset(g_branch, 0, sizeof g_branch); }

// One problem.  kfs [n_kf] (the first n_local are the local keyframes), xw [n_pt][3], edges [n_e] in insertion order, ref_kf [n_pt]
// (-1 = skip).  Out: Tcw [n_local][16], xw_out [n_pt][3], normal [n_pt][3], dist [n_pt], level1 / erase [n_e], stats, margins [4] =
// the smallest relative distance of a decision from its threshold (chi2 bound, depth over range, |rho|, stop rule).
// flags: 0 = the oracle, else a sum of the T_* twins.  cached (may be null) [2][n_e]: every edge's cached chi2 as the first and the
// second classification read it.  Returns 0, or -1 for an index out of range.
extern "C" int sd_ba_oracle(int n_kf, int n_local, const void* kfs, int n_pt, const float* xw, int n_e, const void* edges,
                            const int32_t* ref_kf, float* Tcw, float* xw_out, float* normal, float* dist, uint8_t* level1, uint8_t* erase,
                            void* stats, double* margins, int flags, double* cached)
{
    Graph G;
    g_flags = flags;
    G.lambda = 0; G.ni = 2; G.nBad = 0;
    G.nKF = n_kf; G.nLocal = n_local; G.nPt = n_pt; G.nE = n_e;
    G.kf = (const KF*)kfs; G.E = (const Edge*)edges;
    for (int i = 0; i < n_e; i++) if (G.E[i].kf < 0 || G.E[i].kf >= n_kf || G.E[i].point < 0 || G.E[i].point >= n_pt) return -1;
    for (int p = 0; p < n_pt; p++) if (ref_kf[p] < -1 || ref_kf[p] >= n_kf) return -1;
    Stats& st = *(Stats*)stats;
    std::memset(&st, 0, sizeof st);
    Margins mg = {DBL_MAX, DBL_MAX, DBL_MAX, DBL_MAX};
    G.pose.resize(n_kf); G.X.resize((size_t)n_pt * 3);
    for (int k = 0; k < n_kf; k++) G.pose[k] = to_se3quat(G.kf[k].Tcw);
    for (int i = 0; i < n_pt * 3; i++) G.X[i] = xw[i];
    G.level.assign(n_e, 0); G.chi2c.assign(n_e, 0.0);
    G.robust = true;
    // branch bookkeeping on the structure
    {
        std::vector<int> nEdge(n_pt, 0), nMono(n_pt, 0), nFixed(n_pt, 0), nFree(n_pt, 0);
        for (int i = 0; i < n_e; i++) {
            const Edge& e = G.E[i];
            const bool fixed = e.kf >= n_local || G.kf[e.kf].fixed;
            g_branch[e.ur < 0 ? B_MONO : B_STEREO]++;
            if (fixed) g_branch[B_EDGE_TO_FIXED]++;
            if (e.kf < n_local && G.kf[e.kf].fixed) g_branch[B_FIXED_LOCAL]++;
            nEdge[e.point]++; nMono[e.point] += e.ur < 0; nFixed[e.point] += fixed; nFree[e.point] += !fixed;
        }
        for (int p = 0; p < n_pt; p++) {
            if (nEdge[p] == 1 && nMono[p] == 1) g_branch[B_SINGLE_MONO]++;
            if (nFixed[p] >= 1 && nFree[p] == 1) g_branch[B_FIXED_PLUS_ONE_LOCAL]++;
        }
    }
    const bool noop = n_e == 0;
    if (noop) g_branch[B_NOOP]++;
    if (!noop) {
        optimize(G, 5, 0, st, mg);
        if (flags & T_FRESH_CHI2) refresh_chi2(G);
        if (cached) for (int i = 0; i < n_e; i++) cached[i] = G.chi2c[i];
        for (int i = 0; i < n_e; i++) {
            level1[i] = 0;
            if (classify(G, i, mg, B_LEVEL1_CHI2, B_LEVEL1_DEPTH)) { level1[i] = 1; st.n_level1++; }
            if (!(flags & T_LEVEL1_ACTIVE)) G.level[i] = level1[i];
        }
        {
            std::vector<int> left(n_pt, 0);
            for (int i = 0; i < n_e; i++) if (!G.level[i]) left[G.E[i].point]++;
            for (int i = 0; i < n_e; i++) if (G.level[i] && left[G.E[i].point]) g_branch[B_LEVEL1_POINT_ACTIVE]++;
        }
        g_round1_points = G.X;
        G.robust = false;
        optimize(G, 10, 1, st, mg);
        if (flags & T_FRESH_CHI2) refresh_chi2(G);
        if (cached) for (int i = 0; i < n_e; i++) cached[n_e + i] = G.chi2c[i];
        for (int i = 0; i < n_e; i++) { erase[i] = classify(G, i, mg, B_ERASE_CHI2, B_ERASE_DEPTH); st.n_erased += erase[i]; }
    }
    // outputs
    if (noop) {
        for (int k = 0; k < n_local; k++) std::memcpy(Tcw + 16 * k, G.kf[k].Tcw, 64);
        std::memcpy(xw_out, xw, (size_t)n_pt * 12);
    } else {
        for (int k = 0; k < n_local; k++) to_cvmat(G.pose[k], Tcw + 16 * k);
        for (int i = 0; i < n_pt * 3; i++) xw_out[i] = (float)G.X[i];
    }
    // UpdateNormalAndDepth from the f32 outputs
    std::vector<double> Ow((size_t)n_kf * 3);
    for (int k = 0; k < n_kf; k++) {
        const float* T = k < n_local ? Tcw + 16 * k : G.kf[k].Tcw;
        for (int j = 0; j < 3; j++) Ow[3 * k + j] = -(((double)T[j] * (double)T[3] + (double)T[4 + j] * (double)T[7]) + (double)T[8 + j] * (double)T[11]);
    }
    std::vector<double> acc((size_t)n_pt * 3, 0.0); std::vector<int> cnt(n_pt, 0);
    for (int i = 0; i < n_e; i++) {
        if (erase[i]) continue;
        const Edge& e = G.E[i];
        double dlt[3];
        for (int j = 0; j < 3; j++) dlt[j] = (double)xw_out[3 * e.point + j] - Ow[3 * e.kf + j];
        const double nrm = std::sqrt((dlt[0] * dlt[0] + dlt[1] * dlt[1]) + dlt[2] * dlt[2]);
        for (int j = 0; j < 3; j++) acc[3 * e.point + j] += dlt[j] / nrm;
        cnt[e.point]++;
    }
    for (int p = 0; p < n_pt; p++) {
        for (int j = 0; j < 3; j++) normal[3 * p + j] = cnt[p] ? (float)(acc[3 * p + j] / cnt[p]) : 0.f;
        if (ref_kf[p] < 0) dist[p] = -1.f;
        else {
            double dlt[3];
            for (int j = 0; j < 3; j++) dlt[j] = (double)xw_out[3 * p + j] - Ow[3 * ref_kf[p] + j];
            dist[p] = (float)std::sqrt((dlt[0] * dlt[0] + dlt[1] * dlt[1]) + dlt[2] * dlt[2]);
        }
    }
    margins[0] = mg.chi2; margins[1] = mg.depth; margins[2] = mg.rho; margins[3] = mg.stop;
    return 0;
}
