// CPU oracle of sd_batch_search_by_projection_reloc: a sequential restatement of
//   ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
//                                                                                  src/ORBmatcher.cc:1629-1756
//   Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel)                          src/Frame.cc:735-788
//   Frame::AssignFeaturesToGrid, MapPoint::PredictScale(dist, Frame*), ORBmatcher::ComputeThreeMaxima
// over plain arrays, statement by statement: the loop writes mvpMapPoints while it goes on, the histogram culls after it.  It does NOT use
// the device's reformulation (a key list per keyframe feature replayed in chunks): that they agree is what the tests establish.  Numerics
// as frozen in DESIGN.md Q31 (cv::Mat products left to right in f32, cv::norm through f64) and Q44; compile with -ffp-contract=off.
// Besides the results it counts which branch was taken (sd_reloc_oracle_branches), and sd_reloc_oracle_set_twin selects one deliberately
// wrong rule, so that the tests can show their crafted cases tell the right rule from its neighbour.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <set>
#include <vector>

// tests/cpp/pose_oracle.cpp, compiled into the same library: Optimizer::PoseOptimization over an edge list
extern "C" int sd_pose_oracle(int mode, int n_edges, const void* edges, const float* cam5, float* Tcw, uint8_t* outlier, int32_t* stats, double* aux);

namespace {

struct KeyPoint { float x, y, size, angle, response; int32_t octave, class_id; };      // cv::KeyPoint's layout (28 bytes)
struct Camera { float fx, fy, cx, cy, mbf, mb, mnMinX, mnMaxX, mnMinY, mnMaxY; };       // sd_camera
struct PointRec { float xw[3], normal[3], minDistance, maxDistance; uint32_t flags; };  // sd_map_point: mfMinDistance / mfMaxDistance raw
enum Twin { TWIN_NONE, TWIN_TIE_TO_LATER_VISIT, TWIN_LT_ORBDIST, TWIN_Z_POSITIVE, TWIN_CULLED_FREED_EARLY, TWIN_EXCLUSIVE_MAX_BOUND,
            TWIN_LEVEL_GATE_OF_SIM3, TWIN_DISCARD_AFTER_SECOND_OPTIMISATION, TWIN_GE_30 };
// the exits of include/sd_frontend.h
enum { X_NULL = 1, X_BAD, X_FOUND, X_OUT_U, X_OUT_V, X_DIST_MIN, X_DIST_MAX, X_WINDOW_EMPTY, X_NO_FREE, X_ABOVE_DIST, X_MATCHED, X_CULLED };

const int HISTO_LENGTH = 30;
const int GRID_COLS = 64, GRID_ROWS = 48;

enum Branch {
    B_NULL, B_BAD, B_FOUND, B_OUT_U, B_OUT_V, B_DIST_MIN, B_DIST_MAX, B_WINDOW_EMPTY, B_NO_FREE, B_ABOVE_DIST, B_MATCHED, B_CULLED,
    B_Z_NEGATIVE_SEARCHED, B_NAN_PROJECTION, B_U_EQ_MINX, B_U_EQ_MAXX, B_V_EQ_MINY, B_V_EQ_MAXY, B_DIST_EQ_MIN, B_DIST_EQ_MAX,
    B_LEVEL_0, B_LEVEL_TOP, B_OCTAVE_BELOW, B_OCTAVE_ABOVE, B_OCTAVE_LM1, B_OCTAVE_L, B_OCTAVE_LP1,
    B_CLIP_LEFT, B_CLIP_RIGHT, B_CLIP_TOP, B_CLIP_BOTTOM, B_ON_RADIUS, B_HELD_ON_ENTRY, B_TAKEN_BY_EARLIER, B_LOSER_SECOND_CHOICE,
    B_TIE_FIRST_WINS, B_DIST_EQ_ORB, B_DIST_ORB_PLUS_1, B_DIST_256, B_BIN_WRAP, B_CULLED_HAD_BLOCKED, B_WINDOW_OVER_64, B_NO_FEATURES,
    B_COUNT
};
thread_local int64_t g_branch[B_COUNT];        // per thread: the benchmark runs the oracle on several of them
thread_local int g_twin = TWIN_NONE;

// std::log(float) taken correctly rounded
float logf_cr(float x) { return (float)std::log((double)x); }

int DescriptorDistance(const uint8_t* a, const uint8_t* b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

struct Frame {
    int N = 0;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<uint8_t> mDescriptors;
    std::vector<float> mvuRight, mvInvLevelSigma2;               // the cascade only (sd_reloc_oracle_frame_set_stereo)
    Camera cam;
    int nlevels = 0;
    std::vector<float> mvScaleFactors;
    float mfLogScaleFactor = 0.f, mfGridElementWidthInv = 0.f, mfGridElementHeightInv = 0.f;
    std::vector<size_t> mGrid[GRID_COLS][GRID_ROWS];

    void AssignFeaturesToGrid()
    {
        mfGridElementWidthInv = (float)GRID_COLS / (cam.mnMaxX - cam.mnMinX);
        mfGridElementHeightInv = (float)GRID_ROWS / (cam.mnMaxY - cam.mnMinY);
        for (int i = 0; i < N; i++) {
            const KeyPoint& kp = mvKeysUn[i];
            const int posX = (int)roundf((kp.x - cam.mnMinX) * mfGridElementWidthInv);
            const int posY = (int)roundf((kp.y - cam.mnMinY) * mfGridElementHeightInv);
            if (posX < 0 || posX >= GRID_COLS || posY < 0 || posY >= GRID_ROWS) continue;
            mGrid[posX][posY].push_back(i);
        }
    }
    std::vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r, const int minLevel, const int maxLevel) const
    {
        std::vector<size_t> vIndices;
        if (x != x || y != y) { g_branch[B_NAN_PROJECTION]++; return vIndices; }       // (int)floor(NaN): the cell tests fail on every target seen
        const int rawMinX = (int)floorf((x - cam.mnMinX - r) * mfGridElementWidthInv);
        const int nMinCellX = std::max(0, rawMinX);
        if (nMinCellX >= GRID_COLS) return vIndices;
        const int rawMaxX = (int)ceilf((x - cam.mnMinX + r) * mfGridElementWidthInv);
        const int nMaxCellX = std::min(GRID_COLS - 1, rawMaxX);
        if (nMaxCellX < 0) return vIndices;
        const int rawMinY = (int)floorf((y - cam.mnMinY - r) * mfGridElementHeightInv);
        const int nMinCellY = std::max(0, rawMinY);
        if (nMinCellY >= GRID_ROWS) return vIndices;
        const int rawMaxY = (int)ceilf((y - cam.mnMinY + r) * mfGridElementHeightInv);
        const int nMaxCellY = std::min(GRID_ROWS - 1, rawMaxY);
        if (nMaxCellY < 0) return vIndices;
        if (rawMinX < 0) g_branch[B_CLIP_LEFT]++;
        if (rawMaxX > GRID_COLS - 1) g_branch[B_CLIP_RIGHT]++;
        if (rawMinY < 0) g_branch[B_CLIP_TOP]++;
        if (rawMaxY > GRID_ROWS - 1) g_branch[B_CLIP_BOTTOM]++;
        const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
        if (minLevel == -1) g_branch[B_LEVEL_0]++;
        if (maxLevel == nlevels) g_branch[B_LEVEL_TOP]++;
        for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
            for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
                const std::vector<size_t>& vCell = mGrid[ix][iy];
                if (vCell.empty()) continue;
                for (size_t j = 0, jend = vCell.size(); j < jend; j++) {
                    const KeyPoint& kpUn = mvKeysUn[vCell[j]];
                    if (bCheckLevels) {
                        if (kpUn.octave < minLevel) { g_branch[B_OCTAVE_BELOW]++; continue; }
                        if (maxLevel >= 0)
                            if (kpUn.octave > (g_twin == TWIN_LEVEL_GATE_OF_SIM3 ? maxLevel - 1 : maxLevel)) { g_branch[B_OCTAVE_ABOVE]++; continue; }
                    }
                    const float distx = kpUn.x - x;
                    const float disty = kpUn.y - y;
                    if (fabsf(distx) == r || fabsf(disty) == r) g_branch[B_ON_RADIUS]++;
                    if (fabsf(distx) < r && fabsf(disty) < r) {
                        vIndices.push_back(vCell[j]);
                        g_branch[kpUn.octave == minLevel ? B_OCTAVE_LM1 : (kpUn.octave == maxLevel ? B_OCTAVE_LP1 : B_OCTAVE_L)]++;
                    }
                }
            }
        return vIndices;
    }
};

int PredictScale(float mfMaxDistance, float currentDist, const Frame* pF)
{
    const float ratio = mfMaxDistance / currentDist;
    int nScale = (int)ceilf(logf_cr(ratio) / pF->mfLogScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= pF->nlevels) nScale = pF->nlevels - 1;
    return nScale;
}

void ComputeThreeMaxima(const std::vector<int>* histo, const int L, int& ind1, int& ind2, int& ind3)
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

// skipBlock (the TWIN_CULLED_FREED_EARLY rerun): keyframe features whose match never enters mvpMapPoints
int Search(const Frame& CurrentFrame, const Frame* pKF, const float* mTcw, const int32_t* kfPoint, const uint8_t* found, const PointRec* points,
           const uint8_t* descs, int32_t* mvpMapPoints, int32_t* fromKf, int32_t* exits, int32_t* best, const float th, const int ORBdist,
           const std::vector<char>* skipBlock)
{
    int nmatches = 0;
    const float* T = mTcw;                                        // Rcw = T[4r + c], tcw = T[4r + 3]
    float Ow[3];
    for (int i = 0; i < 3; i++) {
        float s = (-T[0 + i]) * T[3] + (-T[4 + i]) * T[7];
        Ow[i] = s + (-T[8 + i]) * T[11];
    }
    const Camera& cam = CurrentFrame.cam;
    std::vector<int> rotHist[HISTO_LENGTH];
    const float factor = 1.0f / HISTO_LENGTH;
    std::vector<char> blockedSomeone(CurrentFrame.N, 0);
    for (int i = 0; i < CurrentFrame.N; i++) fromKf[i] = -1;
    if (CurrentFrame.N == 0) g_branch[B_NO_FEATURES]++;

    for (int i = 0, iend = pKF->N; i < iend; i++) {
        best[2 * i] = -1; best[2 * i + 1] = 256;
        const int pMP = kfPoint[i];
        if (pMP < 0) { exits[i] = X_NULL; g_branch[B_NULL]++; continue; }
        const PointRec& mp = points[pMP];
        if (!(mp.flags & 1u)) { exits[i] = X_BAD; g_branch[B_BAD]++; continue; }
        if (found && found[i]) { exits[i] = X_FOUND; g_branch[B_FOUND]++; continue; }
        // Project
        float x3Dc[3];
        for (int r = 0; r < 3; r++) {
            float s = T[4 * r] * mp.xw[0] + T[4 * r + 1] * mp.xw[1];
            s = s + T[4 * r + 2] * mp.xw[2];
            x3Dc[r] = s + T[4 * r + 3];
        }
        const float xc = x3Dc[0];
        const float yc = x3Dc[1];
        const float invzc = 1.0 / x3Dc[2];
        const float u = cam.fx * xc * invzc + cam.cx;
        const float v = cam.fy * yc * invzc + cam.cy;
        if (g_twin == TWIN_Z_POSITIVE && !(x3Dc[2] > 0.0f)) { exits[i] = X_OUT_U; continue; }
        if (g_twin == TWIN_EXCLUSIVE_MAX_BOUND ? (u < cam.mnMinX || u >= cam.mnMaxX) : (u < cam.mnMinX || u > cam.mnMaxX)) { exits[i] = X_OUT_U; g_branch[B_OUT_U]++; continue; }
        if (g_twin == TWIN_EXCLUSIVE_MAX_BOUND ? (v < cam.mnMinY || v >= cam.mnMaxY) : (v < cam.mnMinY || v > cam.mnMaxY)) { exits[i] = X_OUT_V; g_branch[B_OUT_V]++; continue; }
        // Compute predicted scale level
        const float PO[3] = {mp.xw[0] - Ow[0], mp.xw[1] - Ow[1], mp.xw[2] - Ow[2]};
        double n2 = (double)PO[0] * (double)PO[0]; n2 += (double)PO[1] * (double)PO[1]; n2 += (double)PO[2] * (double)PO[2];
        float dist3D = (float)std::sqrt(n2);                     // cv::norm accumulates in double (Q11)
        const float maxDistance = 1.2f * mp.maxDistance;         // GetMaxDistanceInvariance()
        const float minDistance = 0.8f * mp.minDistance;         // GetMinDistanceInvariance()
        if (dist3D < minDistance) { exits[i] = X_DIST_MIN; g_branch[B_DIST_MIN]++; continue; }
        if (dist3D > maxDistance) { exits[i] = X_DIST_MAX; g_branch[B_DIST_MAX]++; continue; }
        if (u == cam.mnMinX) g_branch[B_U_EQ_MINX]++;
        if (u == cam.mnMaxX) g_branch[B_U_EQ_MAXX]++;
        if (v == cam.mnMinY) g_branch[B_V_EQ_MINY]++;
        if (v == cam.mnMaxY) g_branch[B_V_EQ_MAXY]++;
        if (dist3D == minDistance) g_branch[B_DIST_EQ_MIN]++;
        if (dist3D == maxDistance) g_branch[B_DIST_EQ_MAX]++;
        if (x3Dc[2] < 0.0f) g_branch[B_Z_NEGATIVE_SEARCHED]++;
        int nPredictedLevel = PredictScale(mp.maxDistance, dist3D, &CurrentFrame);
        // Search in a window
        const float radius = th * CurrentFrame.mvScaleFactors[nPredictedLevel];
        const std::vector<size_t> vIndices2 = CurrentFrame.GetFeaturesInArea(u, v, radius, nPredictedLevel - 1, nPredictedLevel + 1);
        if (vIndices2.empty()) { exits[i] = X_WINDOW_EMPTY; g_branch[B_WINDOW_EMPTY]++; continue; }
        if (vIndices2.size() > 64) g_branch[B_WINDOW_OVER_64]++;
        const uint8_t* dMP = descs + (size_t)pMP * 32;
        int bestDist = 256;
        int bestIdx2 = -1;
        int lostDist = 256;                                       // the nearest member an earlier feature of this call took
        std::vector<size_t> lostTo;
        for (std::vector<size_t>::const_iterator vit = vIndices2.begin(); vit != vIndices2.end(); vit++) {
            const size_t i2 = *vit;
            if (mvpMapPoints[i2] != -1) {
                if (fromKf[i2] < 0) g_branch[B_HELD_ON_ENTRY]++;
                else { g_branch[B_TAKEN_BY_EARLIER]++; lostDist = std::min(lostDist, DescriptorDistance(dMP, &CurrentFrame.mDescriptors[i2 * 32])); lostTo.push_back(i2); }
                continue;
            }
            const int dist = DescriptorDistance(dMP, &CurrentFrame.mDescriptors[i2 * 32]);
            if (dist == 256) g_branch[B_DIST_256]++;
            if (g_twin == TWIN_TIE_TO_LATER_VISIT ? (dist <= bestDist && dist < 256) : dist < bestDist) {
                bestDist = dist;
                bestIdx2 = (int)i2;
            } else if (dist == bestDist && bestIdx2 >= 0) g_branch[B_TIE_FIRST_WINS]++;
        }
        if (lostDist <= ORBdist && lostDist <= bestDist) {       // an earlier feature changed what this one finds
            for (size_t q = 0; q < lostTo.size(); q++) blockedSomeone[lostTo[q]] = 1;
            if (bestDist <= ORBdist) g_branch[B_LOSER_SECOND_CHOICE]++;
        }
        if (bestDist == ORBdist) g_branch[B_DIST_EQ_ORB]++;
        if (bestDist == ORBdist + 1) g_branch[B_DIST_ORB_PLUS_1]++;
        best[2 * i] = bestIdx2; best[2 * i + 1] = bestDist;
        if (g_twin == TWIN_LT_ORBDIST ? bestDist < ORBdist : bestDist <= ORBdist) {
            exits[i] = X_MATCHED;
            if (!(skipBlock && (*skipBlock)[i])) {
                mvpMapPoints[bestIdx2] = pMP;
                fromKf[bestIdx2] = i;
                nmatches++;
                float rot = pKF->mvKeysUn[i].angle - CurrentFrame.mvKeysUn[bestIdx2].angle;
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)roundf(rot * factor);
                if (bin == HISTO_LENGTH) { bin = 0; g_branch[B_BIN_WRAP]++; }
                if (bin < 0 || bin > HISTO_LENGTH) bin = 0;          // angles outside [0, 360): the reference asserts; the library files them in bin 0
                rotHist[bin].push_back(bestIdx2);
            } else exits[i] = X_CULLED;
        } else exits[i] = bestIdx2 < 0 ? X_NO_FREE : X_ABOVE_DIST;
    }

    int ind1 = -1, ind2 = -1, ind3 = -1;
    ComputeThreeMaxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3);
    for (int i = 0; i < HISTO_LENGTH; i++) {
        if (i != ind1 && i != ind2 && i != ind3) {
            for (size_t j = 0, jend = rotHist[i].size(); j < jend; j++) {
                const int i2 = rotHist[i][j];
                exits[fromKf[i2]] = X_CULLED;
                if (blockedSomeone[i2]) g_branch[B_CULLED_HAD_BLOCKED]++;
                mvpMapPoints[i2] = -1;
                fromKf[i2] = -1;
                nmatches--;
            }
        }
    }
    for (int i = 0; i < pKF->N; i++) {
        if (exits[i] == X_MATCHED) g_branch[B_MATCHED]++;
        else if (exits[i] == X_CULLED) g_branch[B_CULLED]++;
        else if (exits[i] == X_NO_FREE) g_branch[B_NO_FREE]++;
        else if (exits[i] == X_ABOVE_DIST) g_branch[B_ABOVE_DIST]++;
    }
    return nmatches;
}

struct PoseEdge { float xw[3]; float u, v, ur; float inv_sigma2; int32_t kp_index; };   // sd_pose_edge
struct RelocResult { int32_t stage_reached, matched, n_good[3], n_additional[2]; float Tcw_stage[3][16]; float Tcw[16]; };   // sd_reloc_result

// Optimizer::PoseOptimization(&mCurrentFrame) (src/Optimizer.cc:239-451): an edge for every key point that holds a point, in key point
// order; mvbOutlier is written for those key points only
int PoseOptimization(const Frame& F, float* mTcw, const int32_t* mvpMapPoints, uint8_t* mvbOutlier, const PointRec* points)
{
    std::vector<PoseEdge> edges;
    for (int i = 0; i < F.N; i++) {
        if (mvpMapPoints[i] < 0) continue;
        const PointRec& mp = points[mvpMapPoints[i]];
        const KeyPoint& kpUn = F.mvKeysUn[i];
        edges.push_back({{mp.xw[0], mp.xw[1], mp.xw[2]}, kpUn.x, kpUn.y, F.mvuRight[i], F.mvInvLevelSigma2[kpUn.octave], i});
    }
    std::vector<uint8_t> out(edges.size() + 1, 0);
    const float cam5[5] = {F.cam.fx, F.cam.fy, F.cam.cx, F.cam.cy, F.cam.mbf};
    const int nGood = sd_pose_oracle(0, (int)edges.size(), edges.data(), cam5, mTcw, out.data(), nullptr, nullptr);
    for (size_t e = 0; e < edges.size(); e++) mvbOutlier[edges[e].kp_index] = out[e];
    return nGood;
}

}  // namespace

extern "C" {

void sd_reloc_oracle_frame_set_stereo(void* k_, const float* uRight, const float* invSigma2)
{
    Frame* k = (Frame*)k_;
    k->mvuRight.assign(uRight, uRight + k->N); k->mvInvLevelSigma2.assign(invSigma2, invSigma2 + k->nlevels);
}

// Tracking::Relocalization from `if(!Tcw.empty())` to `if(nGood>=50)` (src/Tracking.cc:2292-2358) for one candidate.  framePoint[N2] in:
// mvpMapPoints after lines 2300-2309 (the BoW match where vbInliers, else -1); out: the final mvpMapPoints.  outlier[N2] out: mvbOutlier
// (false on entry, as Frame's constructor leaves it).  perturb (nullable, [3][16]) is added to the pose after each optimisation: the
// tests use it to show that a case's decisions do not hang on the last bits of a pose.
void sd_reloc_oracle_refine(const void* frame_, const void* kf_, const float* Tcw, const int32_t* kfPoint, const PointRec* points,
                            const uint8_t* descs, int32_t* framePoint, uint8_t* outlier, RelocResult* R, const float* perturb)
{
    const Frame& F = *(const Frame*)frame_;
    const Frame* pKF = (const Frame*)kf_;
    float mTcw[16];
    memcpy(mTcw, Tcw, sizeof(mTcw));
    memset(R, 0, sizeof(*R));
    for (int k = 0; k < 3; k++) R->n_good[k] = -1;
    R->n_additional[0] = R->n_additional[1] = -1;
    for (int i = 0; i < F.N; i++) outlier[i] = 0;
    std::vector<int32_t> fromKf(F.N + 1), exits(pKF->N + 1), best(2 * pKF->N + 2);
    std::vector<uint8_t> found(pKF->N + 1);
    auto sFoundOf = [&]() {
        std::set<int32_t> sFound;
        for (int j = 0; j < F.N; j++) if (framePoint[j] >= 0) sFound.insert(framePoint[j]);
        for (int i = 0; i < pKF->N; i++) found[i] = kfPoint[i] >= 0 && sFound.count(kfPoint[i]);
    };
    auto optimise = [&](int k) {
        const int n = PoseOptimization(F, mTcw, framePoint, outlier, points);
        if (perturb) for (int q = 0; q < 12; q++) mTcw[q] += perturb[16 * k + q];
        R->n_good[k] = n;
        for (int s = k; s < 3; s++) memcpy(R->Tcw_stage[s], mTcw, sizeof(mTcw));
        return n;
    };
    auto discard = [&]() { for (int io = 0; io < F.N; io++) if (outlier[io]) framePoint[io] = -1; };
    for (int s = 0; s < 3; s++) memcpy(R->Tcw_stage[s], mTcw, sizeof(mTcw));
    sFoundOf();                                                   // sFound: the inliers of lines 2300-2309
    R->stage_reached = 1;
    int nGood = optimise(0);
    if (nGood >= 10) {
        discard();
        if (nGood < 50) {
            R->stage_reached = 2;
            int nadditional = Search(F, pKF, mTcw, kfPoint, found.data(), points, descs, framePoint, fromKf.data(), exits.data(), best.data(), 10, 100, nullptr);
            R->n_additional[0] = nadditional;
            if (nadditional + nGood >= 50) {
                R->stage_reached = 3;
                nGood = optimise(1);
                if (g_twin == TWIN_DISCARD_AFTER_SECOND_OPTIMISATION) discard();
                if ((g_twin == TWIN_GE_30 ? nGood >= 30 : nGood > 30) && nGood < 50) {
                    R->stage_reached = 4;
                    sFoundOf();
                    nadditional = Search(F, pKF, mTcw, kfPoint, found.data(), points, descs, framePoint, fromKf.data(), exits.data(), best.data(), 3, 64, nullptr);
                    R->n_additional[1] = nadditional;
                    if (nGood + nadditional >= 50) {
                        R->stage_reached = 5;
                        nGood = optimise(2);
                        discard();
                    }
                }
            }
        }
    }
    R->matched = nGood >= 50;
    memcpy(R->Tcw, mTcw, sizeof(mTcw));
}

int sd_reloc_oracle_branch_count() { return B_COUNT; }
int64_t* sd_reloc_oracle_branches() { return g_branch; }
void sd_reloc_oracle_reset_branches() { memset(g_branch, 0, sizeof(g_branch)); }
void sd_reloc_oracle_set_twin(int t) { g_twin = t; }

void* sd_reloc_oracle_frame_new(int N, const KeyPoint* keysUn, const uint8_t* desc, const Camera* cam, int nlevels, const float* scale)
{
    Frame* k = new Frame();
    k->N = N;
    k->mvKeysUn.assign(keysUn, keysUn + N); k->mDescriptors.assign(desc, desc + (size_t)N * 32);
    k->cam = *cam; k->nlevels = nlevels;
    k->mvScaleFactors.assign(scale, scale + nlevels);
    k->mfLogScaleFactor = logf_cr(nlevels > 1 ? scale[1] : 1.0f);
    k->AssignFeaturesToGrid();
    return k;
}
void sd_reloc_oracle_frame_free(void* k) { delete (Frame*)k; }

// SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) with CurrentFrame.mTcw = Tcw.  kfPoint[N1]: index into points or -1;
// found[N1] (nullable): the feature's point is in sAlreadyFound; framePoint[N2]: mvpMapPoints, in and out (-1 NULL).
// fromKf[N2], exits[N1], best[N1][2] as the device reports them.  -> nmatches
int sd_reloc_oracle_search(const void* frame_, const void* kf_, const float* Tcw, const int32_t* kfPoint, const uint8_t* found,
                           const PointRec* points, const uint8_t* descs, int32_t* framePoint, int32_t* fromKf, int32_t* exits, int32_t* best,
                           float th, int ORBdist)
{
    const Frame& F = *(const Frame*)frame_;
    const Frame* pKF = (const Frame*)kf_;
    if (g_twin != TWIN_CULLED_FREED_EARLY) return Search(F, pKF, Tcw, kfPoint, found, points, descs, framePoint, fromKf, exits, best, th, ORBdist, nullptr);
    // the wrong twin: what the histogram removes never blocked anyone.  A first run finds what is removed, a second leaves it out.
    std::vector<int32_t> fp(framePoint, framePoint + F.N);
    g_twin = TWIN_NONE;
    Search(F, pKF, Tcw, kfPoint, found, points, descs, fp.data(), fromKf, exits, best, th, ORBdist, nullptr);
    std::vector<char> skip(pKF->N, 0);
    for (int i = 0; i < pKF->N; i++) skip[i] = exits[i] == X_CULLED;
    const int nm = Search(F, pKF, Tcw, kfPoint, found, points, descs, framePoint, fromKf, exits, best, th, ORBdist, &skip);
    g_twin = TWIN_CULLED_FREED_EARLY;
    return nm;
}

}  // extern "C"
