// CPU oracle of sd_batch_search_for_triangulation / sd_batch_create_new_map_points: a sequential restatement of
//   LocalMapping::CreateNewMapPoints              src/LocalMapping.cc:208-453
//   LocalMapping::ComputeF12                      src/LocalMapping.cc:537-554
//   ORBmatcher::SearchForTriangulation            src/ORBmatcher.cc:814-980
//   ORBmatcher::CheckDistEpipolarLine             src/ORBmatcher.cc:140-157
//   KeyFrame::SetPose / UnprojectStereo           src/KeyFrame.cc:70-84, 615-631
// statement by statement: the running bestDist loop, the f1it / f2it walk with lower_bound, the neighbour loop that really sets the
// current keyframe's map points.  It does NOT use the device's reformulation (independent pairs + first surviving neighbour): that the
// two agree is what the tests establish.  Numerics as frozen in DESIGN.md Q25-Q30; compile with -ffp-contract=off.
// Besides the results it counts which branch was taken (sd_tri_oracle_branches) and can trace every triangulated match.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

namespace {

struct KeyPoint { float x, y, size, angle, response; int32_t octave, class_id; };      // cv::KeyPoint's layout (28 bytes)

// ---- a CV_32F cv::Mat, as far as this function uses one (Q14b: a product accumulates in double, k ascending, one narrowing)
struct Mat {
    int rows = 0, cols = 0;
    std::vector<float> d;
    Mat() {}
    Mat(int r, int c) : rows(r), cols(c), d((size_t)r * c, 0.f) {}
    float& at(int i, int j = 0) { return d[(size_t)i * cols + j]; }
    float at(int i, int j = 0) const { return d[(size_t)i * cols + j]; }
    bool empty() const { return d.empty(); }
    Mat t() const { Mat o(cols, rows); for (int i = 0; i < rows; i++) for (int j = 0; j < cols; j++) o.at(j, i) = at(i, j); return o; }
    Mat row(int i) const { Mat o(1, cols); for (int j = 0; j < cols; j++) o.at(0, j) = at(i, j); return o; }
    Mat block(int r0, int r1, int c0, int c1) const { Mat o(r1 - r0, c1 - c0); for (int i = r0; i < r1; i++) for (int j = c0; j < c1; j++) o.at(i - r0, j - c0) = at(i, j); return o; }
};
Mat neg(const Mat& a) { Mat o = a; for (float& v : o.d) v = -v; return o; }
Mat gemm(const Mat& a, const Mat& b, const Mat* c = nullptr)       // a * b [+ c]
{
    Mat o(a.rows, b.cols);
    for (int i = 0; i < a.rows; i++)
        for (int j = 0; j < b.cols; j++) {
            double s = 0.0;
            for (int k = 0; k < a.cols; k++) s += (double)a.at(i, k) * (double)b.at(k, j);
            if (c) s += (double)c->at(i, j);
            o.at(i, j) = (float)s;
        }
    return o;
}
Mat sub(const Mat& a, const Mat& b) { Mat o = a; for (size_t i = 0; i < o.d.size(); i++) o.d[i] = a.d[i] - b.d[i]; return o; }
double dot(const Mat& a, const Mat& b) { double s = 0.0; for (size_t i = 0; i < a.d.size(); i++) s += (double)a.d[i] * (double)b.d[i]; return s; }   // Q11
double norm(const Mat& a) { double s = 0.0; for (float v : a.d) s += (double)v * (double)v; return std::sqrt(s); }                                  // Q11

enum Branch {
    B_SHARED_NODE, B_SKIP_MP1, B_SKIP_ONLYSTEREO1, B_SKIP_MP2, B_SKIP_ONLYSTEREO2, B_DIST_REJECT, B_DIST51, B_EPIPOLE_EXCLUDED, B_EPIPOLE_NEAR_BUT_STEREO,
    B_DEN_ZERO, B_EPI_FAIL, B_EPI_PASS, B_TIE_LATER_WINS, B_BETTER_FAILED_WORSE_PASSED, B_BEST50, B_TWO_IDX1_ONE_IDX2, B_HIST_CULLED, B_BIG_NODE,
    B_NEIGH_SKIP_STEREO, B_NEIGH_SKIP_MONO, B_NEIGH_RUN, B_COUNT
};
thread_local int64_t g_branch[B_COUNT];        // per thread: the benchmark runs the oracle on 16 of them

struct KeyFrame {
    int N = 0;
    const KeyPoint* mvKeysUn = nullptr; const KeyPoint* mvKeys = nullptr;
    const uint8_t* desc = nullptr; const float* mvuRight = nullptr; const float* mvDepth = nullptr;
    std::map<unsigned, std::vector<unsigned>> mFeatVec;          // DBoW2::FeatureVector
    std::vector<uint8_t> mvpMapPoints;                            // != NULL
    Mat Tcw, Ow, Twc;
    float fx, fy, cx, cy, invfx, invfy, mbf, mb;
    const float* mvScaleFactors; const float* mvLevelSigma2; float mfScaleFactor;
    void SetPose(const Mat& Tcw_)
    {
        Tcw = Tcw_;
        Mat Rcw = Tcw.block(0, 3, 0, 3), tcw = Tcw.block(0, 3, 3, 4);
        Mat Rwc = Rcw.t();
        Ow = gemm(neg(Rwc), tcw);
        Twc = Mat(4, 4);
        for (int i = 0; i < 4; i++) Twc.at(i, i) = 1.f;
        for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) Twc.at(i, j) = Rwc.at(i, j); Twc.at(i, 3) = Ow.at(i); }
    }
    Mat GetRotation() const { return Tcw.block(0, 3, 0, 3); }
    Mat GetTranslation() const { return Tcw.block(0, 3, 3, 4); }
    Mat GetCameraCenter() const { return Ow; }
    bool GetMapPoint(size_t i) const { return mvpMapPoints[i] != 0; }
    void AddMapPoint(size_t i) { mvpMapPoints[i] = 1; }
    Mat UnprojectStereo(int i) const
    {
        const float z = mvDepth[i];
        if (z > 0) {
            const float u = mvKeys[i].x, v = mvKeys[i].y;
            const float x = (u - cx) * z * invfx, y = (v - cy) * z * invfy;
            Mat x3Dc(3, 1); x3Dc.at(0) = x; x3Dc.at(1) = y; x3Dc.at(2) = z;
            Mat R = Twc.block(0, 3, 0, 3), t = Twc.block(0, 3, 3, 4);
            return gemm(R, x3Dc, &t);
        }
        return Mat();
    }
};

const int TH_LOW = 50, HISTO_LENGTH = 30;

int DescriptorDistance(const uint8_t* a, const uint8_t* b)
{
    int dist = 0;
    for (int i = 0; i < 32; i++) dist += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return dist;
}

bool CheckDistEpipolarLine(const KeyPoint& kp1, const KeyPoint& kp2, const Mat& F12, const KeyFrame* pKF2)
{
    const float a = kp1.x * F12.at(0, 0) + kp1.y * F12.at(1, 0) + F12.at(2, 0);
    const float b = kp1.x * F12.at(0, 1) + kp1.y * F12.at(1, 1) + F12.at(2, 1);
    const float c = kp1.x * F12.at(0, 2) + kp1.y * F12.at(1, 2) + F12.at(2, 2);
    const float num = a * kp2.x + b * kp2.y + c;
    const float den = a * a + b * b;
    if (den == 0) { g_branch[B_DEN_ZERO]++; return false; }
    const float dsqr = num * num / den;
    return dsqr < 3.84 * pKF2->mvLevelSigma2[kp2.octave];
}

void ComputeThreeMaxima(std::vector<int>* histo, const int L, int& ind1, int& ind2, int& ind3)      // ORBmatcher.cc:1758-1799
{
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < L; i++) {
        const int s = (int)histo[i].size();
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}

int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, const Mat& F12, std::vector<std::pair<size_t, size_t>>& vMatchedPairs,
                           const bool bOnlyStereo, const bool mbCheckOrientation, std::vector<int>* matches12 = nullptr)
{
    const auto& vFeatVec1 = pKF1->mFeatVec;
    const auto& vFeatVec2 = pKF2->mFeatVec;
    Mat Cw = pKF1->GetCameraCenter();
    Mat R2w = pKF2->GetRotation();
    Mat t2w = pKF2->GetTranslation();
    Mat C2 = gemm(R2w, Cw, &t2w);
    const float invz = 1.0f / C2.at(2);
    const float ex = pKF2->fx * C2.at(0) * invz + pKF2->cx;
    const float ey = pKF2->fy * C2.at(1) * invz + pKF2->cy;

    int nmatches = 0;
    std::vector<bool> vbMatched2(pKF2->N, false);
    std::vector<int> vMatches12(pKF1->N, -1);
    std::vector<int> rotHist[HISTO_LENGTH];
    const float factor = 1.0f / HISTO_LENGTH;

    auto f1it = vFeatVec1.begin(), f2it = vFeatVec2.begin();
    auto f1end = vFeatVec1.end(), f2end = vFeatVec2.end();
    while (f1it != f1end && f2it != f2end) {
        if (f1it->first == f2it->first) {
            g_branch[B_SHARED_NODE]++;
            if (f2it->second.size() > 128) g_branch[B_BIG_NODE]++;
            for (size_t i1 = 0, iend1 = f1it->second.size(); i1 < iend1; i1++) {
                const size_t idx1 = f1it->second[i1];
                if (pKF1->GetMapPoint(idx1)) { g_branch[B_SKIP_MP1]++; continue; }
                const bool bStereo1 = pKF1->mvuRight[idx1] >= 0;
                if (bOnlyStereo)
                    if (!bStereo1) { g_branch[B_SKIP_ONLYSTEREO1]++; continue; }
                const KeyPoint& kp1 = pKF1->mvKeysUn[idx1];
                const uint8_t* d1 = pKF1->desc + idx1 * 32;
                int bestDist = TH_LOW;
                int bestIdx2 = -1;
                int minFailed = 1 << 30;                       // instrumentation only
                for (size_t i2 = 0, iend2 = f2it->second.size(); i2 < iend2; i2++) {
                    size_t idx2 = f2it->second[i2];
                    const bool pMP2 = pKF2->GetMapPoint(idx2);
                    if (vbMatched2[idx2] || pMP2) { g_branch[B_SKIP_MP2]++; continue; }
                    const bool bStereo2 = pKF2->mvuRight[idx2] >= 0;
                    if (bOnlyStereo)
                        if (!bStereo2) { g_branch[B_SKIP_ONLYSTEREO2]++; continue; }
                    const uint8_t* d2 = pKF2->desc + idx2 * 32;
                    const int dist = DescriptorDistance(d1, d2);
                    if (dist == TH_LOW + 1) g_branch[B_DIST51]++;
                    if (dist > TH_LOW || dist > bestDist) { g_branch[B_DIST_REJECT]++; continue; }
                    const KeyPoint& kp2 = pKF2->mvKeysUn[idx2];
                    {
                        const float distex = ex - kp2.x, distey = ey - kp2.y;
                        const bool near = distex * distex + distey * distey < 100 * pKF2->mvScaleFactors[kp2.octave];
                        if (near && (bStereo1 || bStereo2)) g_branch[B_EPIPOLE_NEAR_BUT_STEREO]++;
                    }
                    if (!bStereo1 && !bStereo2) {
                        const float distex = ex - kp2.x;
                        const float distey = ey - kp2.y;
                        if (distex * distex + distey * distey < 100 * pKF2->mvScaleFactors[kp2.octave]) { g_branch[B_EPIPOLE_EXCLUDED]++; continue; }
                    }
                    if (CheckDistEpipolarLine(kp1, kp2, F12, pKF2)) {
                        g_branch[B_EPI_PASS]++;
                        if (bestIdx2 >= 0 && dist == bestDist) g_branch[B_TIE_LATER_WINS]++;
                        bestIdx2 = (int)idx2;
                        bestDist = dist;
                    } else {
                        g_branch[B_EPI_FAIL]++;
                        minFailed = std::min(minFailed, dist);
                    }
                }
                if (bestIdx2 >= 0) {
                    if (minFailed < bestDist) g_branch[B_BETTER_FAILED_WORSE_PASSED]++;
                    if (bestDist == TH_LOW) g_branch[B_BEST50]++;
                    const KeyPoint& kp2 = pKF2->mvKeysUn[bestIdx2];
                    vMatches12[idx1] = bestIdx2;
                    nmatches++;
                    if (mbCheckOrientation) {
                        float rot = kp1.angle - kp2.angle;
                        if (rot < 0.0) rot += 360.0f;
                        int bin = (int)std::round(rot * factor);
                        if (bin == HISTO_LENGTH) bin = 0;
                        rotHist[bin].push_back((int)idx1);
                    }
                }
            }
            f1it++;
            f2it++;
        } else if (f1it->first < f2it->first) {
            f1it = vFeatVec1.lower_bound(f2it->first);
        } else {
            f2it = vFeatVec2.lower_bound(f1it->first);
        }
    }
    if (mbCheckOrientation) {
        int ind1 = -1, ind2 = -1, ind3 = -1;
        ComputeThreeMaxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3);
        for (int i = 0; i < HISTO_LENGTH; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (size_t j = 0, jend = rotHist[i].size(); j < jend; j++) {
                vMatches12[rotHist[i][j]] = -1;
                nmatches--;
                g_branch[B_HIST_CULLED]++;
            }
        }
    }
    vMatchedPairs.clear();
    vMatchedPairs.reserve(nmatches);
    std::vector<int> taken(pKF2->N, 0);
    for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
        if (vMatches12[i] < 0) continue;
        if (taken[vMatches12[i]]++) g_branch[B_TWO_IDX1_ONE_IDX2]++;
        vMatchedPairs.push_back(std::make_pair(i, (size_t)vMatches12[i]));
    }
    if (matches12) *matches12 = vMatches12;
    return nmatches;
}

Mat SkewSymmetricMatrix(const Mat& v)
{
    Mat o(3, 3);
    o.at(0, 1) = -v.at(2); o.at(0, 2) = v.at(1);
    o.at(1, 0) = v.at(2); o.at(1, 2) = -v.at(0);
    o.at(2, 0) = -v.at(1); o.at(2, 1) = v.at(0);
    return o;
}

// the inverse of K in closed form (Q26): computed in double, narrowed
Mat Kinv(const KeyFrame* k)
{
    Mat o(3, 3);
    o.at(0, 0) = (float)(1.0 / (double)k->fx); o.at(0, 2) = (float)(-(double)k->cx / (double)k->fx);
    o.at(1, 1) = (float)(1.0 / (double)k->fy); o.at(1, 2) = (float)(-(double)k->cy / (double)k->fy);
    o.at(2, 2) = 1.f;
    return o;
}

Mat ComputeF12(KeyFrame* pKF1, KeyFrame* pKF2)
{
    Mat R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation();
    Mat R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
    Mat R12 = gemm(R1w, R2w.t());
    Mat t12 = gemm(gemm(neg(R1w), R2w.t()), t2w, &t1w);
    Mat t12x = SkewSymmetricMatrix(t12);
    return gemm(gemm(gemm(Kinv(pKF1).t(), t12x), R12), Kinv(pKF2));
}

// ---- the frozen null vector (Q29): one-sided Jacobi on A promoted to f64, pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), SWEEPS sweeps
int g_sweeps = 8;                                  // changed only by the single-threaded convergence test
void NullVector4(const Mat& A, float x[4], double v64[4])
{
    double a[4][4], v[4][4];
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { a[r][c] = (double)A.at(r, c); v[r][c] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < g_sweeps; sweep++)
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int r = 0; r < 4; r++) { alpha += a[r][p] * a[r][p]; beta += a[r][q] * a[r][q]; gamma += a[r][p] * a[r][q]; }
                if (gamma != 0.0) {
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
                    for (int r = 0; r < 4; r++) {
                        const double ap = a[r][p], aq = a[r][q], vp = v[r][p], vq = v[r][q];
                        a[r][p] = cs * ap - sn * aq; a[r][q] = sn * ap + cs * aq;
                        v[r][p] = cs * vp - sn * vq; v[r][q] = sn * vp + cs * vq;
                    }
                }
            }
    int best = 0; double nbest = 0.0;
    for (int c = 0; c < 4; c++) {
        double n = 0.0;
        for (int r = 0; r < 4; r++) n += a[r][c] * a[r][c];
        if (c == 0 || n < nbest) { nbest = n; best = c; }
    }
    const double b0 = v[0][best], b1 = v[1][best], b2 = v[2][best], b3 = v[3][best];
    const double nv = std::sqrt(((b0 * b0 + b1 * b1) + b2 * b2) + b3 * b3);
    const double o[4] = {b0 / nv, b1 / nv, b2 / nv, b3 / nv};
    for (int i = 0; i < 4; i++) { x[i] = (float)o[i]; if (v64) v64[i] = o[i]; }
}

// cos(2 * atan2(mb / 2, depth)) frozen as (d^2 - h^2) / (d^2 + h^2) in double (Q28)
float CosStereo(float mb, float depth)
{
    const double h = (double)mb / 2.0, d = (double)depth;
    return (float)((d * d - h * h) / (d * d + h * h));
}

enum Path { P_NONE, P_SVD, P_UNPROJ1, P_UNPROJ2 };
enum Outcome { O_CREATED, O_LOW_PARALLAX, O_W0, O_Z1, O_Z2, O_REPROJ1_MONO, O_REPROJ1_STEREO, O_REPROJ2_MONO, O_REPROJ2_STEREO, O_DIST0, O_SCALE_LOW, O_SCALE_HIGH, O_NO_DEPTH };
struct Trace { int32_t neighbour, idx1, idx2, path, outcome, stereo1, stereo2, pad; float cosRays; float A[16]; float x3D[3]; };   // 112 bytes
struct NewPoint { int32_t neighbour, idx1, idx2; float xw[3]; };

int CreateNewMapPoints(KeyFrame* mpCurrentKeyFrame, std::vector<KeyFrame*>& vpNeighKFs, bool mbMonocular, const float* medianDepth,
                       NewPoint* out, Trace* trace, int traceCap, int* nTrace)
{
    Mat Rcw1 = mpCurrentKeyFrame->GetRotation();
    Mat Rwc1 = Rcw1.t();
    Mat tcw1 = mpCurrentKeyFrame->GetTranslation();
    Mat Tcw1 = mpCurrentKeyFrame->Tcw.block(0, 3, 0, 4);
    Mat Ow1 = mpCurrentKeyFrame->GetCameraCenter();
    const float& fx1 = mpCurrentKeyFrame->fx; const float& fy1 = mpCurrentKeyFrame->fy;
    const float& cx1 = mpCurrentKeyFrame->cx; const float& cy1 = mpCurrentKeyFrame->cy;
    const float& invfx1 = mpCurrentKeyFrame->invfx; const float& invfy1 = mpCurrentKeyFrame->invfy;
    const float ratioFactor = 1.5f * mpCurrentKeyFrame->mfScaleFactor;
    int nnew = 0, nt = 0;
    for (size_t i = 0; i < vpNeighKFs.size(); i++) {
        KeyFrame* pKF2 = vpNeighKFs[i];
        Mat Ow2 = pKF2->GetCameraCenter();
        Mat vBaseline = sub(Ow2, Ow1);
        const float baseline = (float)norm(vBaseline);
        if (!mbMonocular) {
            if (baseline < pKF2->mb) { g_branch[B_NEIGH_SKIP_STEREO]++; continue; }
        } else {
            const float medianDepthKF2 = medianDepth[i];
            const float ratioBaselineDepth = baseline / medianDepthKF2;
            if (ratioBaselineDepth < 0.01) { g_branch[B_NEIGH_SKIP_MONO]++; continue; }
        }
        g_branch[B_NEIGH_RUN]++;
        Mat F12 = ComputeF12(mpCurrentKeyFrame, pKF2);
        std::vector<std::pair<size_t, size_t>> vMatchedIndices;
        SearchForTriangulation(mpCurrentKeyFrame, pKF2, F12, vMatchedIndices, false, false);
        Mat Rcw2 = pKF2->GetRotation();
        Mat Rwc2 = Rcw2.t();
        Mat tcw2 = pKF2->GetTranslation();
        Mat Tcw2 = pKF2->Tcw.block(0, 3, 0, 4);
        const float& fx2 = pKF2->fx; const float& fy2 = pKF2->fy; const float& cx2 = pKF2->cx; const float& cy2 = pKF2->cy;
        const float& invfx2 = pKF2->invfx; const float& invfy2 = pKF2->invfy;
        const int nmatches = (int)vMatchedIndices.size();
        for (int ikp = 0; ikp < nmatches; ikp++) {
            const int idx1 = (int)vMatchedIndices[ikp].first;
            const int idx2 = (int)vMatchedIndices[ikp].second;
            Trace T; memset(&T, 0, sizeof(T));
            T.neighbour = (int)i; T.idx1 = idx1; T.idx2 = idx2;
            auto done = [&](int outcome) { T.outcome = outcome; if (trace && nt < traceCap) trace[nt] = T; nt++; };
            const KeyPoint& kp1 = mpCurrentKeyFrame->mvKeysUn[idx1];
            const float kp1_ur = mpCurrentKeyFrame->mvuRight[idx1];
            bool bStereo1 = kp1_ur >= 0;
            const KeyPoint& kp2 = pKF2->mvKeysUn[idx2];
            const float kp2_ur = pKF2->mvuRight[idx2];
            bool bStereo2 = kp2_ur >= 0;
            T.stereo1 = bStereo1; T.stereo2 = bStereo2;
            Mat xn1(3, 1); xn1.at(0) = (kp1.x - cx1) * invfx1; xn1.at(1) = (kp1.y - cy1) * invfy1; xn1.at(2) = 1.0f;
            Mat xn2(3, 1); xn2.at(0) = (kp2.x - cx2) * invfx2; xn2.at(1) = (kp2.y - cy2) * invfy2; xn2.at(2) = 1.0f;
            Mat ray1 = gemm(Rwc1, xn1);
            Mat ray2 = gemm(Rwc2, xn2);
            const float cosParallaxRays = (float)(dot(ray1, ray2) / (norm(ray1) * norm(ray2)));
            T.cosRays = cosParallaxRays;
            float cosParallaxStereo = cosParallaxRays + 1;
            float cosParallaxStereo1 = cosParallaxStereo;
            float cosParallaxStereo2 = cosParallaxStereo;
            if (bStereo1)
                cosParallaxStereo1 = CosStereo(mpCurrentKeyFrame->mb, mpCurrentKeyFrame->mvDepth[idx1]);
            else if (bStereo2)
                cosParallaxStereo2 = CosStereo(pKF2->mb, pKF2->mvDepth[idx2]);
            cosParallaxStereo = std::min(cosParallaxStereo1, cosParallaxStereo2);
            Mat x3D;
            if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || cosParallaxRays < 0.9998)) {
                T.path = P_SVD;
                Mat A(4, 4);
                for (int c = 0; c < 4; c++) {
                    A.at(0, c) = xn1.at(0) * Tcw1.at(2, c) - Tcw1.at(0, c);
                    A.at(1, c) = xn1.at(1) * Tcw1.at(2, c) - Tcw1.at(1, c);
                    A.at(2, c) = xn2.at(0) * Tcw2.at(2, c) - Tcw2.at(0, c);
                    A.at(3, c) = xn2.at(1) * Tcw2.at(2, c) - Tcw2.at(1, c);
                }
                memcpy(T.A, A.d.data(), 64);
                float v[4];
                NullVector4(A, v, nullptr);
                if (v[3] == 0) { done(O_W0); continue; }
                x3D = Mat(3, 1);
                for (int k = 0; k < 3; k++) x3D.at(k) = v[k] / v[3];
            } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
                T.path = P_UNPROJ1;
                x3D = mpCurrentKeyFrame->UnprojectStereo(idx1);
                if (x3D.empty()) { done(O_NO_DEPTH); continue; }       // uRight >= 0 with depth <= 0: no point (the reference would go on with an empty Mat)
            } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
                T.path = P_UNPROJ2;
                x3D = pKF2->UnprojectStereo(idx2);
                if (x3D.empty()) { done(O_NO_DEPTH); continue; }
            } else { done(O_LOW_PARALLAX); continue; }
            for (int k = 0; k < 3; k++) T.x3D[k] = x3D.at(k);
            Mat x3Dt = x3D.t();
            float z1 = (float)(dot(Rcw1.row(2), x3Dt) + tcw1.at(2));
            if (z1 <= 0) { done(O_Z1); continue; }
            float z2 = (float)(dot(Rcw2.row(2), x3Dt) + tcw2.at(2));
            if (z2 <= 0) { done(O_Z2); continue; }
            const float& sigmaSquare1 = mpCurrentKeyFrame->mvLevelSigma2[kp1.octave];
            const float x1 = (float)(dot(Rcw1.row(0), x3Dt) + tcw1.at(0));
            const float y1 = (float)(dot(Rcw1.row(1), x3Dt) + tcw1.at(1));
            const float invz1 = (float)(1.0 / z1);
            if (!bStereo1) {
                float u1 = fx1 * x1 * invz1 + cx1;
                float v1 = fy1 * y1 * invz1 + cy1;
                float errX1 = u1 - kp1.x;
                float errY1 = v1 - kp1.y;
                if ((errX1 * errX1 + errY1 * errY1) > 5.991 * sigmaSquare1) { done(O_REPROJ1_MONO); continue; }
            } else {
                float u1 = fx1 * x1 * invz1 + cx1;
                float u1_r = u1 - mpCurrentKeyFrame->mbf * invz1;
                float v1 = fy1 * y1 * invz1 + cy1;
                float errX1 = u1 - kp1.x;
                float errY1 = v1 - kp1.y;
                float errX1_r = u1_r - kp1_ur;
                if ((errX1 * errX1 + errY1 * errY1 + errX1_r * errX1_r) > 7.8 * sigmaSquare1) { done(O_REPROJ1_STEREO); continue; }
            }
            const float sigmaSquare2 = pKF2->mvLevelSigma2[kp2.octave];
            const float x2 = (float)(dot(Rcw2.row(0), x3Dt) + tcw2.at(0));
            const float y2 = (float)(dot(Rcw2.row(1), x3Dt) + tcw2.at(1));
            const float invz2 = (float)(1.0 / z2);
            if (!bStereo2) {
                float u2 = fx2 * x2 * invz2 + cx2;
                float v2 = fy2 * y2 * invz2 + cy2;
                float errX2 = u2 - kp2.x;
                float errY2 = v2 - kp2.y;
                if ((errX2 * errX2 + errY2 * errY2) > 5.991 * sigmaSquare2) { done(O_REPROJ2_MONO); continue; }
            } else {
                float u2 = fx2 * x2 * invz2 + cx2;
                float u2_r = u2 - mpCurrentKeyFrame->mbf * invz2;
                float v2 = fy2 * y2 * invz2 + cy2;
                float errX2 = u2 - kp2.x;
                float errY2 = v2 - kp2.y;
                float errX2_r = u2_r - kp2_ur;
                if ((errX2 * errX2 + errY2 * errY2 + errX2_r * errX2_r) > 7.8 * sigmaSquare2) { done(O_REPROJ2_STEREO); continue; }
            }
            Mat normal1 = sub(x3D, Ow1);
            float dist1 = (float)norm(normal1);
            Mat normal2 = sub(x3D, Ow2);
            float dist2 = (float)norm(normal2);
            if (dist1 == 0 || dist2 == 0) { done(O_DIST0); continue; }
            const float ratioDist = dist2 / dist1;
            const float ratioOctave = mpCurrentKeyFrame->mvScaleFactors[kp1.octave] / pKF2->mvScaleFactors[kp2.octave];
            if (ratioDist * ratioFactor < ratioOctave) { done(O_SCALE_LOW); continue; }
            if (ratioDist > ratioOctave * ratioFactor) { done(O_SCALE_HIGH); continue; }
            // Triangulation is successful
            mpCurrentKeyFrame->AddMapPoint(idx1);
            pKF2->AddMapPoint(idx2);
            NewPoint& np = out[nnew];
            np.neighbour = (int)i; np.idx1 = idx1; np.idx2 = idx2;
            for (int k = 0; k < 3; k++) np.xw[k] = x3D.at(k);
            done(O_CREATED);
            nnew++;
        }
    }
    if (nTrace) *nTrace = nt;
    return nnew;
}

}  // namespace

extern "C" {

struct sd_tri_kf {              // one keyframe as the tests hand it over
    int32_t N, nfv;
    const KeyPoint* keysUn; const KeyPoint* keys; const uint8_t* desc; const float* uRight; const float* depth;
    const uint32_t* fvNode; const uint32_t* fvFeat;       // the flattened FeatureVector
    const uint8_t* hasMp;                                   // nullable
    const float* Tcw;                                       // 16, row-major
};
struct sd_tri_cam { float fx, fy, cx, cy, mbf, mb, scaleFactor; int32_t nlevels; const float* scale; const float* sigma2; };

static void fill(KeyFrame& K, const sd_tri_kf& k, const sd_tri_cam& c)
{
    K.N = k.N; K.mvKeysUn = k.keysUn; K.mvKeys = k.keys; K.desc = k.desc; K.mvuRight = k.uRight; K.mvDepth = k.depth;
    for (int i = 0; i < k.nfv; i++) K.mFeatVec[k.fvNode[i]].push_back(k.fvFeat[i]);
    K.mvpMapPoints.assign(k.N, 0);
    if (k.hasMp) for (int i = 0; i < k.N; i++) K.mvpMapPoints[i] = k.hasMp[i];
    K.fx = c.fx; K.fy = c.fy; K.cx = c.cx; K.cy = c.cy; K.invfx = 1.0f / c.fx; K.invfy = 1.0f / c.fy; K.mbf = c.mbf; K.mb = c.mb;
    K.mvScaleFactors = c.scale; K.mvLevelSigma2 = c.sigma2; K.mfScaleFactor = c.scaleFactor;
    Mat T(4, 4); memcpy(T.d.data(), k.Tcw, 64);
    K.SetPose(T);
}

int64_t* sd_tri_oracle_branches(void) { return g_branch; }
int sd_tri_oracle_branch_count(void) { return B_COUNT; }
void sd_tri_oracle_reset_branches(void) { memset(g_branch, 0, sizeof(g_branch)); }
void sd_tri_oracle_set_sweeps(int n) { g_sweeps = n; }

// match12 [N1], pairs [N1][2]; returns nmatches; F12out (nullable) [9]
int sd_tri_oracle_search(const sd_tri_kf* k1, const sd_tri_kf* k2, const sd_tri_cam* cam, int onlyStereo, int checkOrientation,
                         int32_t* match12, int32_t* pairs, int32_t* npairs, float* F12out)
{
    KeyFrame A, B;
    fill(A, *k1, *cam); fill(B, *k2, *cam);
    KeyFrame* pA = &A; KeyFrame* pB = &B;
    Mat F12 = ComputeF12(pA, pB);
    if (F12out) memcpy(F12out, F12.d.data(), 36);
    std::vector<std::pair<size_t, size_t>> vp;
    std::vector<int> m12;
    const int n = SearchForTriangulation(pA, pB, F12, vp, onlyStereo != 0, checkOrientation != 0, &m12);
    for (int i = 0; i < A.N; i++) match12[i] = m12[i];
    for (size_t i = 0; i < vp.size(); i++) { pairs[2 * i] = (int)vp[i].first; pairs[2 * i + 1] = (int)vp[i].second; }
    *npairs = (int)vp.size();
    return n;
}

// out [N1]; trace (nullable) [traceCap]; returns nnew
int sd_tri_oracle_create(const sd_tri_kf* k1, int nNeigh, const sd_tri_kf* k2s, const float* medianDepth, const sd_tri_cam* cam,
                         NewPoint* out, Trace* trace, int traceCap, int32_t* nTrace)
{
    KeyFrame A;
    fill(A, *k1, *cam);
    std::vector<KeyFrame> Ks(nNeigh);
    std::vector<KeyFrame*> ptr;
    for (int i = 0; i < nNeigh; i++) { fill(Ks[i], k2s[i], *cam); ptr.push_back(&Ks[i]); }
    return CreateNewMapPoints(&A, ptr, medianDepth != nullptr, medianDepth, out, trace, traceCap, nTrace);
}

void sd_tri_oracle_null4(const float* A16, float* x4, double* v4)
{
    Mat A(4, 4); memcpy(A.d.data(), A16, 64);
    NullVector4(A, x4, v4);
}

}
