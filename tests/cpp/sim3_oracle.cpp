// Sequential CPU restatement of Sim3Solver (src/Sim3Solver.cc) as DESIGN.md Q39 freezes it: one problem at a time, one iteration
// after the other, literal vectors and loops, returning at the first hypothesis with more than mRansacMinInliers inliers exactly as
// iterate() does.  Written from the reference and Q39, not from the kernels.  Built by tests/sim3_cases.py with
// g++ -O2 -ffp-contract=off (and once more with -ffp-contract=fast to count the decisions that contraction would change).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include <algorithm>

extern "C" {

struct Corr { float xw1[3], xw2[3]; float sigma2_1, sigma2_2; int32_t tag; };
struct Problem { float Tcw1[16], Tcw2[16]; float K1[4], K2[4]; int32_t fix_scale, reserved; uint64_t seed; };
struct Result { int32_t found, no_more, iteration, n_inliers, max_its, reserved; float T12[16], R12[9], t12[3], s12; };

}

namespace {

uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

uint64_t draw(uint64_t seed, int iteration, int d) { return splitmix64(splitmix64(seed) + ((uint64_t)iteration << 2) + (uint64_t)d); }

// :163-177 on a literal vector
void sample_literal(uint64_t seed, int iteration, int N, int out[3])
{
    std::vector<size_t> vAvailableIndices;
    for (int i = 0; i < N; i++) vAvailableIndices.push_back(i);
    for (short i = 0; i < 3; ++i) {
        int randi = (int)(draw(seed, iteration, i) % (uint64_t)vAvailableIndices.size());
        out[i] = (int)vAvailableIndices[randi];
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
    }
}

struct Vec3 { float v[3]; };

Vec3 transform(const float* T, const Vec3& X)      // R X + t of a row-major 4x4: (a0 b0 + a1 b1) + a2 b2, then + t, f32
{
    Vec3 r;
    for (int i = 0; i < 3; i++) {
        float s = T[4 * i] * X.v[0] + T[4 * i + 1] * X.v[1];
        s = s + T[4 * i + 2] * X.v[2];
        r.v[i] = s + T[4 * i + 3];
    }
    return r;
}

void project(const Vec3& P, const float* K, float uv[2])        // FromCameraToImage / Project; K = fx fy cx cy
{
    const float invz = 1 / P.v[2];
    const float x = P.v[0] * invz;
    const float y = P.v[1] * invz;
    uv[0] = K[0] * x + K[2];
    uv[1] = K[1] * y + K[3];
}

float max_error(float sigma2)                                    // std::vector<size_t>::push_back(9.210*sigma2), read back as float
{
    const double d = 9.210 * (double)sigma2;
    if (!(d >= 1.0)) return 0.f;
    if (d >= 9.0e18) return 9.0e18f;
    size_t n = (size_t)d;
    return (float)n;
}

struct Hyp { float T12[16], T21[16], R[9], t[3], s; };

void jacobi_rotate(double A[4][4], double V[4][4], int p, int q)
{
    if (A[p][q] == 0.0) return;
    double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
    double t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    double c = 1.0 / std::sqrt(t * t + 1.0);
    double s = t * c;
    for (int k = 0; k < 4; k++) { double x = A[k][p], y = A[k][q]; A[k][p] = c * x - s * y; A[k][q] = s * x + c * y; }
    for (int k = 0; k < 4; k++) { double x = A[p][k], y = A[q][k]; A[p][k] = c * x - s * y; A[q][k] = s * x + c * y; }
    for (int k = 0; k < 4; k++) { double x = V[k][p], y = V[k][q]; V[k][p] = c * x - s * y; V[k][q] = s * x + c * y; }
}

// ComputeSim3 (:226-337).  P1, P2: 3x3, column k = sampled point k
void compute_sim3(const float P1[3][3], const float P2[3][3], bool fixScale, Hyp& H)
{
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
    for (int r = 0; r < 3; r++) {
        O1[r] = ((P1[r][0] + P1[r][1]) + P1[r][2]) / 3.0f;
        O2[r] = ((P2[r][0] + P2[r][1]) + P2[r][2]) / 3.0f;
    }
    for (int i = 0; i < 3; i++)
        for (int r = 0; r < 3; r++) { Pr1[r][i] = P1[r][i] - O1[r]; Pr2[r][i] = P2[r][i] - O2[r]; }
    float M[3][3];                                               // Pr2 * Pr1.t()
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float s = Pr2[i][0] * Pr1[j][0] + Pr2[i][1] * Pr1[j][1];
            M[i][j] = s + Pr2[i][2] * Pr1[j][2];
        }
    double N11, N12, N13, N14, N22, N23, N24, N33, N34, N44;
    N11 = M[0][0] + M[1][1] + M[2][2];
    N12 = M[1][2] - M[2][1];
    N13 = M[2][0] - M[0][2];
    N14 = M[0][1] - M[1][0];
    N22 = M[0][0] - M[1][1] - M[2][2];
    N23 = M[0][1] + M[1][0];
    N24 = M[2][0] + M[0][2];
    N33 = -M[0][0] + M[1][1] - M[2][2];
    N34 = M[1][2] + M[2][1];
    N44 = -M[0][0] - M[1][1] + M[2][2];
    double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 10; sweep++)
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) jacobi_rotate(A, V, p, q);
    int top = 0;
    for (int k = 1; k < 4; k++) if (A[k][k] > A[top][top]) top = k;
    double q[4];
    for (int k = 0; k < 4; k++) q[k] = V[k][top];
    double norm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    double w = q[0] / norm, x = q[1] / norm, y = q[2] / norm, z = q[3] / norm;
    float R[3][3];
    R[0][0] = (float)(1.0 - 2.0 * (y * y + z * z)); R[0][1] = (float)(2.0 * (x * y - w * z)); R[0][2] = (float)(2.0 * (x * z + w * y));
    R[1][0] = (float)(2.0 * (x * y + w * z)); R[1][1] = (float)(1.0 - 2.0 * (x * x + z * z)); R[1][2] = (float)(2.0 * (y * z - w * x));
    R[2][0] = (float)(2.0 * (x * z - w * y)); R[2][1] = (float)(2.0 * (y * z + w * x)); R[2][2] = (float)(1.0 - 2.0 * (x * x + y * y));
    float P3[3][3];                                              // R * Pr2
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float s = R[i][0] * Pr2[0][j] + R[i][1] * Pr2[1][j];
            P3[i][j] = s + R[i][2] * Pr2[2][j];
        }
    float s12;
    if (!fixScale) {
        double nom = 0;
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) nom += (double)Pr1[i][j] * (double)P3[i][j];
        float aux[3][3];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) aux[i][j] = P3[i][j] * P3[i][j];
        double den = 0;
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) den += aux[i][j];
        s12 = (float)(nom / den);
    } else
        s12 = 1.0f;
    float sR[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) sR[i][j] = s12 * R[i][j];
    float t12[3];
    for (int i = 0; i < 3; i++) {
        float s = sR[i][0] * O2[0] + sR[i][1] * O2[1];
        s = s + sR[i][2] * O2[2];
        t12[i] = O1[i] - s;
    }
    float sRinv[3][3];
    const double inv = 1.0 / s12;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) sRinv[i][j] = (float)(inv * R[j][i]);
    float tinv[3];
    for (int i = 0; i < 3; i++) {
        float s = (-sRinv[i][0]) * t12[0] + (-sRinv[i][1]) * t12[1];
        tinv[i] = s + (-sRinv[i][2]) * t12[2];
    }
    std::memset(&H, 0, sizeof H);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) { H.T12[4 * i + j] = sR[i][j]; H.T21[4 * i + j] = sRinv[i][j]; H.R[3 * i + j] = R[i][j]; }
        H.T12[4 * i + 3] = t12[i]; H.T21[4 * i + 3] = tinv[i]; H.t[i] = t12[i];
    }
    H.T12[15] = 1.f; H.T21[15] = 1.f; H.s = s12;
}

struct Solver {
    int N = 0;
    std::vector<Vec3> mvX3Dc1, mvX3Dc2;
    std::vector<float> mvP1im1, mvP2im2;           // 2 per point
    std::vector<float> mvnMaxError1, mvnMaxError2;
    const Problem* P = nullptr;

    Solver(const Problem* p, const Corr* c, int n) : P(p)
    {
        for (int i = 0; i < n; i++) {
            Vec3 a, b;
            std::memcpy(a.v, c[i].xw1, 12); std::memcpy(b.v, c[i].xw2, 12);
            mvnMaxError1.push_back(max_error(c[i].sigma2_1));
            mvnMaxError2.push_back(max_error(c[i].sigma2_2));
            mvX3Dc1.push_back(transform(p->Tcw1, a));
            mvX3Dc2.push_back(transform(p->Tcw2, b));
        }
        N = n;
        for (int i = 0; i < N; i++) {
            float uv[2];
            project(mvX3Dc1[i], p->K1, uv); mvP1im1.push_back(uv[0]); mvP1im1.push_back(uv[1]);
            project(mvX3Dc2[i], p->K2, uv); mvP2im2.push_back(uv[0]); mvP2im2.push_back(uv[1]);
        }
    }

    // CheckInliers (:340-364); err (nullable): 2 per point
    int check(const Hyp& H, std::vector<bool>& in, float* err) const
    {
        int n = 0;
        for (int i = 0; i < N; i++) {
            float a[2], b[2];
            project(transform(H.T12, mvX3Dc2[i]), P->K1, a);       // vP2im1
            project(transform(H.T21, mvX3Dc1[i]), P->K2, b);       // vP1im2
            const float d1x = mvP1im1[2 * i] - a[0], d1y = mvP1im1[2 * i + 1] - a[1];
            const float d2x = b[0] - mvP2im2[2 * i], d2y = b[1] - mvP2im2[2 * i + 1];
            const float err1 = (float)((double)d1x * d1x + (double)d1y * d1y);
            const float err2 = (float)((double)d2x * d2x + (double)d2y * d2y);
            if (err) { err[2 * i] = err1; err[2 * i + 1] = err2; }
            if (err1 < mvnMaxError1[i] && err2 < mvnMaxError2[i]) { in[i] = true; n++; }
            else in[i] = false;
        }
        return n;
    }
};

int ransac_max_its(double probability, int minInliers, int maxIterations, int N)      // SetRansacParameters (:114-138)
{
    float epsilon = (float)minInliers / N;
    int nIterations;
    if (minInliers == N)
        nIterations = 1;
    else {
        double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
        if (!(v < (double)maxIterations)) nIterations = maxIterations;      // also NaN
        else if (v <= 1.0) nIterations = 1;
        else nIterations = (int)v;
    }
    return std::max(1, std::min(nIterations, maxIterations));
}

}  // namespace

extern "C" {

// find() of one problem.  info[0]: 0 = N < minInliers (or < 3): no hypothesis, 1 = found, 2 = iterations exhausted;
// info[1] = hypotheses evaluated; info[2] = times a later hypothesis replaced the best with an EQUAL count (the >= of :183);
// info[3] = hypotheses with a non-finite scale or translation.
int sd_sim3_oracle_find(const Problem* p, const Corr* c, int n, double probability, int minInliers, int maxIterations, Result* out,
                        uint8_t* inliers, int64_t* info)
{
    std::memset(out, 0, sizeof *out);
    for (int i = 0; i < n; i++) inliers[i] = 0;
    for (int k = 0; k < 4; k++) info[k] = 0;
    Solver S(p, c, n);
    const int mRansacMaxIts = ransac_max_its(probability, minInliers, maxIterations, n);
    out->max_its = mRansacMaxIts;
    if (S.N < minInliers || S.N < 3) { out->no_more = 1; return 0; }
    int mnIterations = 0, mnBestInliers = 0, bestIteration = 0;
    Hyp best;
    std::memset(&best, 0, sizeof best);
    std::vector<bool> mvbInliersi(S.N);
    while (mnIterations < mRansacMaxIts) {
        mnIterations++;
        int idx[3];
        sample_literal(p->seed, mnIterations, S.N, idx);
        float P1[3][3], P2[3][3];
        for (int i = 0; i < 3; i++)
            for (int r = 0; r < 3; r++) { P1[r][i] = S.mvX3Dc1[idx[i]].v[r]; P2[r][i] = S.mvX3Dc2[idx[i]].v[r]; }
        Hyp H;
        compute_sim3(P1, P2, p->fix_scale != 0, H);
        info[1]++;
        if (!std::isfinite(H.s) || !std::isfinite(H.t[0]) || !std::isfinite(H.t[1]) || !std::isfinite(H.t[2])) info[3]++;
        const int mnInliersi = S.check(H, mvbInliersi, nullptr);
        if (mnInliersi >= mnBestInliers) {
            if (mnIterations > 1 && mnInliersi == mnBestInliers) info[2]++;
            mnBestInliers = mnInliersi;
            best = H;
            bestIteration = mnIterations;
            if (mnInliersi > minInliers) {
                for (int i = 0; i < S.N; i++) if (mvbInliersi[i]) inliers[i] = 1;
                out->found = 1;
                break;
            }
        }
    }
    if (!out->found) out->no_more = 1;
    out->iteration = bestIteration; out->n_inliers = mnBestInliers;
    std::memcpy(out->T12, best.T12, 64); std::memcpy(out->R12, best.R, 36); std::memcpy(out->t12, best.t, 12); out->s12 = best.s;
    info[0] = out->found ? 1 : 2;
    return 0;
}

// find() of problems [first, last) of packed tables, one after the other (a host thread of tools/bench_sim3.py takes one such chunk,
// so that the timed region is this loop and nothing else).  corr_offset [n + 1]; results [n]; inliers [correspondences]; info [n][4].
int sd_sim3_oracle_find_range(int first, int last, const int32_t* corr_offset, const Corr* corr, const Problem* problems, double probability,
                              int minInliers, int maxIterations, Result* results, uint8_t* inliers, int64_t* info)
{
    for (int p = first; p < last; p++)
        sd_sim3_oracle_find(problems + p, corr + corr_offset[p], corr_offset[p + 1] - corr_offset[p], probability, minInliers, maxIterations,
                            results + p, inliers + corr_offset[p], info + 4 * p);
    return 0;
}

// the three indices of one iteration, on the literal vector
void sd_sim3_oracle_sample(uint64_t seed, int iteration, int N, int* out) { sample_literal(seed, iteration, N, out); }
// the same with the three draws given (for the exhaustive comparison with the closed form): r[k] < N - k
void sd_sim3_oracle_remove(const int* r, int N, int* out)
{
    std::vector<size_t> v;
    for (int i = 0; i < N; i++) v.push_back(i);
    for (int i = 0; i < 3; i++) { out[i] = (int)v[r[i]]; v[r[i]] = v.back(); v.pop_back(); }
}

// ComputeSim3 of three given camera-frame pairs (x1 [3][3], x2 [3][3]: point-major) -> T12 [16], T21 [16], R [9], t [3], s
void sd_sim3_oracle_horn(const float* x1, const float* x2, int fixScale, float* out)
{
    float P1[3][3], P2[3][3];
    for (int i = 0; i < 3; i++) for (int r = 0; r < 3; r++) { P1[r][i] = x1[3 * i + r]; P2[r][i] = x2[3 * i + r]; }
    Hyp H;
    compute_sim3(P1, P2, fixScale != 0, H);
    std::memcpy(out, &H, sizeof H);
}

// CheckInliers of a given T12 / T21: err [n][2], inlier [n]; returns the count
int sd_sim3_oracle_check(const Problem* p, const Corr* c, int n, const float* T12, const float* T21, float* err, uint8_t* inlier)
{
    Solver S(p, c, n);
    Hyp H;
    std::memset(&H, 0, sizeof H);
    std::memcpy(H.T12, T12, 64); std::memcpy(H.T21, T21, 64);
    std::vector<bool> in(n);
    const int k = S.check(H, in, err);
    for (int i = 0; i < n; i++) inlier[i] = in[i] ? 1 : 0;
    return k;
}

int sd_sim3_oracle_max_its(double probability, int minInliers, int maxIterations, int N) { return ransac_max_its(probability, minInliers, maxIterations, N); }

}

// ---------------------------------------------------------------- ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1259-1483)
// Literal: a key frame with its own mGrid of index vectors, GetFeaturesInArea returning a vector, the three loops as written.
extern "C" {
struct KeyPoint { float x, y, size, angle, response; int32_t octave, class_id; };
struct MapPointRec { float xw[3], normal[3], mfMinDistance, mfMaxDistance; uint32_t flags; };
struct CamRec { float fx, fy, cx, cy, mbf, mb, mnMinX, mnMaxX, mnMinY, mnMaxY; };
}

namespace {

enum { B_NULL_OR_BAD, B_ALREADY, B_Z_NEG, B_U_BELOW_MIN, B_U_AT_MAX, B_V_BELOW_MIN, B_V_AT_MAX, B_NOT_FINITE, B_DIST_BELOW, B_DIST_ABOVE,
       B_EMPTY, B_NO_OCTAVE, B_TOO_FAR, B_MATCH };
enum { C_OCTAVE_BELOW, C_OCTAVE_ABOVE, C_OCTAVE_LM1, C_OCTAVE_L, C_TIE, C_WINDOW_MAX, C_AGREE_FAIL, C_AGREE_OK, C_COLS_MAX, C_COUNT };

struct KeyFrameO {
    int N;
    const KeyPoint* mvKeysUn;
    const uint8_t* mDescriptors;
    CamRec cam;
    float mfGridElementWidthInv, mfGridElementHeightInv;
    std::vector<size_t> mGrid[64][48];

    KeyFrameO(int n, const KeyPoint* kp, const uint8_t* d, const CamRec& c) : N(n), mvKeysUn(kp), mDescriptors(d), cam(c)
    {
        mfGridElementWidthInv = 64.0f / (cam.mnMaxX - cam.mnMinX);
        mfGridElementHeightInv = 48.0f / (cam.mnMaxY - cam.mnMinY);
        for (int i = 0; i < N; i++) {                                 // Frame::AssignFeaturesToGrid / PosInGrid
            int posX = (int)std::round((kp[i].x - cam.mnMinX) * mfGridElementWidthInv);
            int posY = (int)std::round((kp[i].y - cam.mnMinY) * mfGridElementHeightInv);
            if (posX < 0 || posX >= 64 || posY < 0 || posY >= 48) continue;
            mGrid[posX][posY].push_back(i);
        }
    }

    std::vector<size_t> GetFeaturesInArea(float x, float y, float r, int* cols) const
    {
        std::vector<size_t> vIndices;
        const int nMinCellX = std::max(0, (int)std::floor((x - cam.mnMinX - r) * mfGridElementWidthInv));
        if (nMinCellX >= 64) return vIndices;
        const int nMaxCellX = std::min(63, (int)std::ceil((x - cam.mnMinX + r) * mfGridElementWidthInv));
        if (nMaxCellX < 0) return vIndices;
        const int nMinCellY = std::max(0, (int)std::floor((y - cam.mnMinY - r) * mfGridElementHeightInv));
        if (nMinCellY >= 48) return vIndices;
        const int nMaxCellY = std::min(47, (int)std::ceil((y - cam.mnMinY + r) * mfGridElementHeightInv));
        if (nMaxCellY < 0) return vIndices;
        *cols = nMaxCellX - nMinCellX + 1;
        for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
            for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
                const std::vector<size_t>& vCell = mGrid[ix][iy];
                for (size_t j = 0; j < vCell.size(); j++) {
                    const KeyPoint& kpUn = mvKeysUn[vCell[j]];
                    const float distx = kpUn.x - x, disty = kpUn.y - y;
                    if (std::fabs(distx) < r && std::fabs(disty) < r) vIndices.push_back(vCell[j]);
                }
            }
        return vIndices;
    }
    bool IsInImage(float x, float y) const { return x >= cam.mnMinX && x < cam.mnMaxX && y >= cam.mnMinY && y < cam.mnMaxY; }
};

int DescriptorDistance(const uint8_t* a, const uint8_t* b)
{
    int dist = 0;
    for (int i = 0; i < 32; i++) { unsigned v = a[i] ^ b[i]; while (v) { dist += v & 1; v >>= 1; } }
    return dist;
}

float logf_cr(float x) { return (float)std::log((double)x); }        // std::log(float), taken correctly rounded

int PredictScale(const MapPointRec& mp, float currentDist, float scaleFactor, int nScaleLevels)      // MapPoint.cc:385-399
{
    float ratio = mp.mfMaxDistance / currentDist;
    int nScale = (int)std::ceil(logf_cr(ratio) / logf_cr(scaleFactor));
    if (nScale < 0) nScale = 0;
    else if (nScale >= nScaleLevels) nScale = nScaleLevels - 1;
    return nScale;
}

// one of the two search loops (:1305-1382 / :1385-1462): points of `src` through Tsrc and then T (= [sR21 | t21] or [sR12 | t12]) into dst
void search_direction(int Nsrc, const int* srcPoint, const std::vector<bool>& vbAlreadyMatched, const float* Tsrc, const float* T,
                      const KeyFrameO& dst, const MapPointRec* points, const uint8_t* pdesc, int nPoints, int nlevels, const float* scale,
                      float th, std::vector<int>& vnMatch, int* branch, int64_t* counters)
{
    const CamRec& cam = dst.cam;
    for (int i1 = 0; i1 < Nsrc; i1++) {
        const int m = srcPoint[i1];
        if (m < 0 || m >= nPoints) { branch[i1] = B_NULL_OR_BAD; continue; }
        if (vbAlreadyMatched[i1]) { branch[i1] = B_ALREADY; continue; }
        const MapPointRec& mp = points[m];
        Vec3 p3Dw; std::memcpy(p3Dw.v, mp.xw, 12);
        Vec3 p3Dc1 = transform(Tsrc, p3Dw);
        Vec3 p3Dc2 = transform(T, p3Dc1);
        if (p3Dc2.v[2] < 0.0) { branch[i1] = B_Z_NEG; continue; }
        const float invz = 1.0 / p3Dc2.v[2];
        const float x = p3Dc2.v[0] * invz;
        const float y = p3Dc2.v[1] * invz;
        const float u = cam.fx * x + cam.cx;
        const float v = cam.fy * y + cam.cy;
        if (!dst.IsInImage(u, v)) {
            branch[i1] = u < cam.mnMinX ? B_U_BELOW_MIN : u >= cam.mnMaxX ? B_U_AT_MAX : v < cam.mnMinY ? B_V_BELOW_MIN : v >= cam.mnMaxY ? B_V_AT_MAX : B_NOT_FINITE;
            continue;
        }
        const float maxDistance = 1.2f * mp.mfMaxDistance;
        const float minDistance = 0.8f * mp.mfMinDistance;
        const float dist3D = (float)std::sqrt((double)p3Dc2.v[0] * p3Dc2.v[0] + (double)p3Dc2.v[1] * p3Dc2.v[1] + (double)p3Dc2.v[2] * p3Dc2.v[2]);
        if (dist3D < minDistance) { branch[i1] = B_DIST_BELOW; continue; }
        if (dist3D > maxDistance) { branch[i1] = B_DIST_ABOVE; continue; }
        const int nPredictedLevel = PredictScale(mp, dist3D, scale[1], nlevels);
        const float radius = th * scale[nPredictedLevel];
        int cols = 0;
        const std::vector<size_t> vIndices = dst.GetFeaturesInArea(u, v, radius, &cols);
        if (vIndices.empty()) { branch[i1] = B_EMPTY; continue; }
        counters[C_WINDOW_MAX] = std::max<int64_t>(counters[C_WINDOW_MAX], (int64_t)vIndices.size());
        counters[C_COLS_MAX] = std::max<int64_t>(counters[C_COLS_MAX], cols);
        const uint8_t* dMP = pdesc + (size_t)m * 32;
        int bestDist = 0x7FFFFFFF;
        int bestIdx = -1;
        for (std::vector<size_t>::const_iterator vit = vIndices.begin(); vit != vIndices.end(); vit++) {
            const size_t idx = *vit;
            const KeyPoint& kp = dst.mvKeysUn[idx];
            if (kp.octave < nPredictedLevel - 1) { counters[C_OCTAVE_BELOW]++; continue; }
            if (kp.octave > nPredictedLevel) { counters[C_OCTAVE_ABOVE]++; continue; }
            counters[kp.octave == nPredictedLevel ? C_OCTAVE_L : C_OCTAVE_LM1]++;
            const int dist = DescriptorDistance(dMP, dst.mDescriptors + idx * 32);
            if (dist == bestDist) counters[C_TIE]++;
            if (dist < bestDist) { bestDist = dist; bestIdx = (int)idx; }
        }
        if (bestDist <= 100) { vnMatch[i1] = bestIdx; branch[i1] = B_MATCH; }
        else branch[i1] = bestIdx < 0 ? B_NO_OCTAVE : B_TOO_FAR;
    }
}

}  // namespace

extern "C" {

int sd_sim3_oracle_counter_count() { return C_COUNT; }

// One SearchBySim3 call.  kf*_point: GetMapPointMatches() as indices into `points` (-1: NULL or bad); matched12 [N1] as in the header.
// Out: vnMatch1 [N1], vnMatch2 [N2], match12 [N1] (idx2 where the function sets vpMatches12[i1]), branch1 [N1], branch2 [N2],
// counters [C_COUNT] (accumulated).  Returns nFound.
int sd_sim3_oracle_search(int N1, const KeyPoint* kp1, const uint8_t* desc1, const float* Tcw1, const int* kf1_point, int N2,
                          const KeyPoint* kp2, const uint8_t* desc2, const float* Tcw2, const int* kf2_point, const int* matched12,
                          const MapPointRec* points, const uint8_t* pdesc, int nPoints, const CamRec* cam, int nlevels, const float* scale,
                          float s12, const float* R12, const float* t12, float th, int* vnMatch1o, int* vnMatch2o, int* match12,
                          int* branch1, int* branch2, int64_t* counters)
{
    KeyFrameO pKF1(N1, kp1, desc1, *cam), pKF2(N2, kp2, desc2, *cam);
    // sR12 = s12 * R12; sR21 = (1.0 / s12) * R12.t(); t21 = -sR21 * t12, as 4x4 [sR | t]
    float T12[16], T21[16];
    std::memset(T12, 0, sizeof T12); std::memset(T21, 0, sizeof T21);
    const double inv = 1.0 / s12;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { T12[4 * i + j] = s12 * R12[3 * i + j]; T21[4 * i + j] = (float)(inv * R12[3 * j + i]); }
    for (int i = 0; i < 3; i++) {
        T12[4 * i + 3] = t12[i];
        float s = (-T21[4 * i]) * t12[0] + (-T21[4 * i + 1]) * t12[1];
        T21[4 * i + 3] = s + (-T21[4 * i + 2]) * t12[2];
    }
    T12[15] = 1.f; T21[15] = 1.f;
    std::vector<bool> vbAlreadyMatched1(N1, false), vbAlreadyMatched2(N2, false);
    for (int i = 0; i < N1; i++) {
        if (matched12[i] != -1) {
            vbAlreadyMatched1[i] = true;
            int idx2 = matched12[i];
            if (idx2 >= 0 && idx2 < N2) vbAlreadyMatched2[idx2] = true;
        }
    }
    std::vector<int> vnMatch1(N1, -1), vnMatch2(N2, -1);
    search_direction(N1, kf1_point, vbAlreadyMatched1, Tcw1, T21, pKF2, points, pdesc, nPoints, nlevels, scale, th, vnMatch1, branch1, counters);
    search_direction(N2, kf2_point, vbAlreadyMatched2, Tcw2, T12, pKF1, points, pdesc, nPoints, nlevels, scale, th, vnMatch2, branch2, counters);
    int nFound = 0;
    for (int i1 = 0; i1 < N1; i1++) {
        match12[i1] = -1;
        int idx2 = vnMatch1[i1];
        if (idx2 >= 0) {
            int idx1 = vnMatch2[idx2];
            if (idx1 == i1) { match12[i1] = idx2; nFound++; counters[C_AGREE_OK]++; }
            else counters[C_AGREE_FAIL]++;
        }
    }
    for (int i = 0; i < N1; i++) vnMatch1o[i] = vnMatch1[i];
    for (int i = 0; i < N2; i++) vnMatch2o[i] = vnMatch2[i];
    return nFound;
}

}
