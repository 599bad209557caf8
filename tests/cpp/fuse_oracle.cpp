// CPU oracle of sd_batch_fuse / sd_distinctive_descriptors_device: a sequential restatement of
//   ORBmatcher::Fuse(pKF, vpMapPoints, th)          src/ORBmatcher.cc:982-1132
//   KeyFrame::GetFeaturesInArea / IsInImage          src/KeyFrame.cc:569-613
//   Frame::AssignFeaturesToGrid / PosInGrid          src/Frame.cc:463-478, 790-800 (the keyframe copies the frame's grid)
//   MapPoint::PredictScale                           src/MapPoint.cc:399-414
//   MapPoint::ComputeDistinctiveDescriptors          src/MapPoint.cc:242-307
//   MapPoint::AddObservation / Replace               src/MapPoint.cc:98-109, 177-215
// statement by statement: the running bestDist loop over the vector GetFeaturesInArea returns, the tail that changes what a feature
// holds while the loop goes on.  It does NOT use the device's reformulation (independent entries + first taker per feature): that the
// two agree is what the tests establish.  Numerics as frozen in DESIGN.md Q31; compile with -ffp-contract=off.
// Three layers: (a) the search of one entry and the sequential job over an occupancy table, (b) ComputeDistinctiveDescriptors,
// (c) a small map model (points with observation maps, keyframes with mvpMapPoints) that runs the literal Fuse including its tail.
// Besides the results it counts which branch was taken (sd_fuse_oracle_branches).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

namespace {

struct KeyPoint { float x, y, size, angle, response; int32_t octave, class_id; };      // cv::KeyPoint's layout (28 bytes)
struct Camera { float fx, fy, cx, cy, mbf, mb, mnMinX, mnMaxX, mnMinY, mnMaxY; };       // sd_camera
struct PointRec { float xw[3], normal[3], minDistance, maxDistance; uint32_t flags; };  // sd_map_point: mfMinDistance / mfMaxDistance raw
struct Hit { int32_t cand, idx, dist, action, other; };                                  // sd_fuse_hit
enum { ACT_ADD = 1, ACT_MEET_KF = 2, ACT_MEET_BAD = 3, ACT_MEET_CANDIDATE = 4 };

const int TH_LOW = 50;
const int GRID_COLS = 64, GRID_ROWS = 48;

enum Branch {
    B_ENTRY_SKIP, B_SEARCHED, B_Z_NEGATIVE, B_Z_ZERO, B_OUT_OF_IMAGE, B_U_EQ_MAXX, B_U_EQ_MINX, B_DIST_BELOW_MIN, B_DIST_ABOVE_MAX, B_VIEW_ANGLE,
    B_WINDOW_EMPTY, B_CLIP_LEFT, B_CLIP_RIGHT, B_CLIP_TOP, B_CLIP_BOTTOM, B_OCTAVE_BELOW, B_OCTAVE_ABOVE, B_OCTAVE_LM1, B_OCTAVE_L,
    B_STEREO_FAIL, B_STEREO_PASS, B_MONO_FAIL, B_MONO_PASS, B_URIGHT_ZERO_STEREO, B_TIE_EARLIER_WINS, B_TIE_HIGHER_INDEX_EARLIER,
    B_CLOSER_OUT_OF_RANGE, B_DIST50, B_DIST51, B_MEET_KF, B_MEET_BAD, B_ADD, B_MEET_CANDIDATE, B_NO_FEATURES, B_EMPTY_JOB, B_WINDOW_OVER_64,
    B_COUNT
};
thread_local int64_t g_branch[B_COUNT];        // per thread: the benchmark runs the oracle on 16 of them

// std::log(float) taken correctly rounded
float logf_cr(float x) { return (float)std::log((double)x); }

int DescriptorDistance(const uint8_t* a, const uint8_t* b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

struct KeyFrame {
    int N = 0;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<uint8_t> mDescriptors;
    std::vector<float> mvuRight;
    float Tcw[16];
    float Ow[3];
    Camera cam;
    int nlevels = 0;
    std::vector<float> mvScaleFactors, mvInvLevelSigma2;
    float mfLogScaleFactor = 0.f, mfGridElementWidthInv = 0.f, mfGridElementHeightInv = 0.f;
    std::vector<size_t> mGrid[GRID_COLS][GRID_ROWS];

    void SetPose(const float* T)
    {
        memcpy(Tcw, T, 64);
        // Ow = -Rcw.t() * tcw: f32, left to right (Q31)
        for (int i = 0; i < 3; i++) {
            float s = (-T[0 + i]) * T[3] + (-T[4 + i]) * T[7];
            Ow[i] = s + (-T[8 + i]) * T[11];
        }
    }
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
    bool IsInImage(float x, float y) const { return x >= cam.mnMinX && x < cam.mnMaxX && y >= cam.mnMinY && y < cam.mnMaxY; }
    std::vector<size_t> GetFeaturesInArea(float x, float y, float r) const
    {
        std::vector<size_t> vIndices;
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
        for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
            for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
                const std::vector<size_t>& vCell = mGrid[ix][iy];
                for (size_t j = 0, jend = vCell.size(); j < jend; j++) {
                    const KeyPoint& kpUn = mvKeysUn[vCell[j]];
                    const float distx = kpUn.x - x;
                    const float disty = kpUn.y - y;
                    if (fabsf(distx) < r && fabsf(disty) < r) vIndices.push_back(vCell[j]);
                }
            }
        return vIndices;
    }
};

// MapPoint::PredictScale(currentDist, pKF)
int PredictScale(float mfMaxDistance, float currentDist, const KeyFrame* pKF)
{
    const float ratio = mfMaxDistance / currentDist;
    int nScale = (int)ceilf(logf_cr(ratio) / pKF->mfLogScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= pKF->nlevels) nScale = pKF->nlevels - 1;
    return nScale;
}

// ORBmatcher.cc:1009-1106 for one map point that passed the `continue`s at :1003-1007
void SearchOne(const KeyFrame* pKF, const PointRec& mp, const uint8_t* dMP, float th, int& bestIdx, int& bestDist)
{
    bestDist = 256; bestIdx = -1;
    g_branch[B_SEARCHED]++;
    if (pKF->N == 0) g_branch[B_NO_FEATURES]++;
    const float* T = pKF->Tcw;
    const float fx = pKF->cam.fx, fy = pKF->cam.fy, cx = pKF->cam.cx, cy = pKF->cam.cy, bf = pKF->cam.mbf;
    // p3Dc = Rcw * p3Dw + tcw: f32, left to right (Q31)
    float p3Dc[3];
    for (int i = 0; i < 3; i++) {
        float s = T[4 * i] * mp.xw[0] + T[4 * i + 1] * mp.xw[1];
        s = s + T[4 * i + 2] * mp.xw[2];
        p3Dc[i] = s + T[4 * i + 3];
    }
    if (p3Dc[2] < 0.0f) { g_branch[B_Z_NEGATIVE]++; return; }
    const float invz = 1 / p3Dc[2];
    const float x = p3Dc[0] * invz;
    const float y = p3Dc[1] * invz;
    const float u = fx * x + cx;
    const float v = fy * y + cy;
    if (!pKF->IsInImage(u, v)) {
        if (p3Dc[2] == 0.0f) g_branch[B_Z_ZERO]++;
        else if (u == pKF->cam.mnMaxX) g_branch[B_U_EQ_MAXX]++;
        else g_branch[B_OUT_OF_IMAGE]++;
        return;
    }
    if (u == pKF->cam.mnMinX) g_branch[B_U_EQ_MINX]++;
    const float ur = u - bf * invz;
    const float maxDistance = 1.2f * mp.maxDistance;             // GetMaxDistanceInvariance()
    const float minDistance = 0.8f * mp.minDistance;             // GetMinDistanceInvariance()
    const float PO[3] = {mp.xw[0] - pKF->Ow[0], mp.xw[1] - pKF->Ow[1], mp.xw[2] - pKF->Ow[2]};
    double n2 = (double)PO[0] * (double)PO[0]; n2 += (double)PO[1] * (double)PO[1]; n2 += (double)PO[2] * (double)PO[2];
    const float dist3D = (float)std::sqrt(n2);                   // cv::norm accumulates in double (Q11)
    if (dist3D < minDistance) { g_branch[B_DIST_BELOW_MIN]++; return; }
    if (dist3D > maxDistance) { g_branch[B_DIST_ABOVE_MAX]++; return; }
    double dot = (double)PO[0] * (double)mp.normal[0]; dot += (double)PO[1] * (double)mp.normal[1]; dot += (double)PO[2] * (double)mp.normal[2];
    if (dot < 0.5 * dist3D) { g_branch[B_VIEW_ANGLE]++; return; }
    const int nPredictedLevel = PredictScale(mp.maxDistance, dist3D, pKF);
    const float radius = th * pKF->mvScaleFactors[nPredictedLevel];
    const std::vector<size_t> vIndices = pKF->GetFeaturesInArea(u, v, radius);
    if (vIndices.empty()) { g_branch[B_WINDOW_EMPTY]++; return; }
    if (vIndices.size() > 64) g_branch[B_WINDOW_OVER_64]++;
    int closestOutOfRange = 256;
    for (std::vector<size_t>::const_iterator vit = vIndices.begin(), vend = vIndices.end(); vit != vend; vit++) {
        const size_t idx = *vit;
        const KeyPoint& kp = pKF->mvKeysUn[idx];
        const int kpLevel = kp.octave;
        if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) {
            g_branch[kpLevel < nPredictedLevel - 1 ? B_OCTAVE_BELOW : B_OCTAVE_ABOVE]++;
            closestOutOfRange = std::min(closestOutOfRange, DescriptorDistance(dMP, &pKF->mDescriptors[idx * 32]));
            continue;
        }
        g_branch[kpLevel == nPredictedLevel ? B_OCTAVE_L : B_OCTAVE_LM1]++;
        if (pKF->mvuRight[idx] >= 0) {
            if (pKF->mvuRight[idx] == 0) g_branch[B_URIGHT_ZERO_STEREO]++;
            const float kpx = kp.x, kpy = kp.y, kpr = pKF->mvuRight[idx];
            const float ex = u - kpx;
            const float ey = v - kpy;
            const float er = ur - kpr;
            const float e2 = ex * ex + ey * ey + er * er;
            if (e2 * pKF->mvInvLevelSigma2[kpLevel] > 7.8) { g_branch[B_STEREO_FAIL]++; continue; }
            g_branch[B_STEREO_PASS]++;
        } else {
            const float kpx = kp.x, kpy = kp.y;
            const float ex = u - kpx;
            const float ey = v - kpy;
            const float e2 = ex * ex + ey * ey;
            if (e2 * pKF->mvInvLevelSigma2[kpLevel] > 5.99) { g_branch[B_MONO_FAIL]++; continue; }
            g_branch[B_MONO_PASS]++;
        }
        const int dist = DescriptorDistance(dMP, &pKF->mDescriptors[idx * 32]);
        if (dist < bestDist) {
            bestDist = dist;
            bestIdx = (int)idx;
        } else if (dist == bestDist && bestIdx >= 0) {
            g_branch[B_TIE_EARLIER_WINS]++;
            if ((int)idx < bestIdx) g_branch[B_TIE_HIGHER_INDEX_EARLIER]++;
        }
    }
    if (bestIdx >= 0 && closestOutOfRange < bestDist) g_branch[B_CLOSER_OUT_OF_RANGE]++;
    if (bestDist == TH_LOW) g_branch[B_DIST50]++;
    if (bestDist == TH_LOW + 1) g_branch[B_DIST51]++;
}

// MapPoint::ComputeDistinctiveDescriptors from vDescriptors on: BestIdx, or -1 when vDescriptors is empty
int Distinctive(int N, const uint8_t* vDescriptors)
{
    if (N <= 0) return -1;
    std::vector<float> Distances((size_t)N * N);
    for (int i = 0; i < N; i++) {
        Distances[(size_t)i * N + i] = 0;
        for (int j = i + 1; j < N; j++) {
            const int distij = DescriptorDistance(vDescriptors + (size_t)i * 32, vDescriptors + (size_t)j * 32);
            Distances[(size_t)i * N + j] = distij;
            Distances[(size_t)j * N + i] = distij;
        }
    }
    int BestMedian = INT_MAX;
    int BestIdx = 0;
    for (int i = 0; i < N; i++) {
        std::vector<int> vDists(Distances.begin() + (size_t)i * N, Distances.begin() + (size_t)(i + 1) * N);
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[(size_t)(0.5 * (N - 1))];
        if (median < BestMedian) { BestMedian = median; BestIdx = i; }
    }
    return BestIdx;
}

// ---------------------------------------------------------------- (c) the map model
struct Model;
struct MapPoint {
    int mnId = 0;
    PointRec rec;
    uint8_t mDescriptor[32];
    bool mbBad = false;
    std::map<int, size_t> mObservations;          // keyframe id -> feature (std::map<KeyFrame*, size_t> in the caller's order)
    int nObs = 0, mnVisible = 1, mnFound = 1, mpReplaced = -1;
    bool inMap = true;
};
struct ModelKF { KeyFrame* kf = nullptr; std::vector<int> mvpMapPoints; bool bad = false; };
struct Model {
    std::vector<ModelKF> kfs;
    std::vector<MapPoint> pts;
    ~Model() { for (ModelKF& k : kfs) delete k.kf; }
    bool IsInKeyFrame(int p, int kf) const { return pts[p].mObservations.count(kf) != 0; }
    void AddObservation(int p, int kf, size_t idx)
    {
        MapPoint& P = pts[p];
        if (P.mObservations.count(kf)) return;
        P.mObservations[kf] = idx;
        if (kfs[kf].kf->mvuRight[idx] >= 0) P.nObs += 2; else P.nObs++;
    }
    void ComputeDistinctiveDescriptors(int p)
    {
        MapPoint& P = pts[p];
        if (P.mbBad) return;
        if (P.mObservations.empty()) return;
        std::vector<uint8_t> vDescriptors;
        for (std::map<int, size_t>::iterator mit = P.mObservations.begin(); mit != P.mObservations.end(); mit++)
            if (!kfs[mit->first].bad) {
                const uint8_t* row = &kfs[mit->first].kf->mDescriptors[mit->second * 32];
                vDescriptors.insert(vDescriptors.end(), row, row + 32);
            }
        if (vDescriptors.empty()) return;
        const int BestIdx = Distinctive((int)(vDescriptors.size() / 32), vDescriptors.data());
        memcpy(P.mDescriptor, &vDescriptors[(size_t)BestIdx * 32], 32);
    }
    void Replace(int self, int pMP)
    {
        if (pts[pMP].mnId == pts[self].mnId) return;
        std::map<int, size_t> obs = pts[self].mObservations;
        pts[self].mObservations.clear();
        pts[self].mbBad = true;
        const int nvisible = pts[self].mnVisible, nfound = pts[self].mnFound;
        pts[self].mpReplaced = pMP;
        for (std::map<int, size_t>::iterator mit = obs.begin(); mit != obs.end(); mit++) {
            const int pKF = mit->first;
            if (!IsInKeyFrame(pMP, pKF)) {
                kfs[pKF].mvpMapPoints[mit->second] = pMP;       // ReplaceMapPointMatch
                AddObservation(pMP, pKF, mit->second);
            } else {
                kfs[pKF].mvpMapPoints[mit->second] = -1;        // EraseMapPointMatch
            }
        }
        pts[pMP].mnFound += nfound;
        pts[pMP].mnVisible += nvisible;
        ComputeDistinctiveDescriptors(pMP);
        pts[self].inMap = false;                                 // mpMap->EraseMapPoint(this)
    }
    // ORBmatcher.cc:1108-1128
    bool Tail(int pKF, int pMP, int bestIdx, int bestDist)
    {
        if (bestDist <= TH_LOW) {
            const int pMPinKF = kfs[pKF].mvpMapPoints[bestIdx];
            if (pMPinKF >= 0) {
                if (!pts[pMPinKF].mbBad) {
                    if (pts[pMPinKF].nObs > pts[pMP].nObs) Replace(pMP, pMPinKF);
                    else Replace(pMPinKF, pMP);
                }
            } else {
                AddObservation(pMP, pKF, bestIdx);
                kfs[pKF].mvpMapPoints[bestIdx] = pMP;            // AddMapPoint
            }
            return true;
        }
        return false;
    }
    bool Skipped(int pKF, int pMP) const { return pMP < 0 || pts[pMP].mbBad || IsInKeyFrame(pMP, pKF); }
    int Fuse(int pKF, int nMPs, const int* vpMapPoints, float th)
    {
        int nFused = 0;
        for (int i = 0; i < nMPs; i++) {
            const int pMP = vpMapPoints[i];
            if (Skipped(pKF, pMP)) { g_branch[B_ENTRY_SKIP]++; continue; }
            int bestIdx, bestDist;
            SearchOne(kfs[pKF].kf, pts[pMP].rec, pts[pMP].mDescriptor, th, bestIdx, bestDist);
            if (Tail(pKF, pMP, bestIdx, bestDist)) nFused++;
        }
        return nFused;
    }
};

template <typename T> void put(std::vector<uint8_t>& o, const T& v) { const uint8_t* p = (const uint8_t*)&v; o.insert(o.end(), p, p + sizeof(T)); }

}  // namespace

extern "C" {

int sd_fuse_oracle_branch_count() { return B_COUNT; }
int64_t* sd_fuse_oracle_branches() { return g_branch; }
void sd_fuse_oracle_reset_branches() { memset(g_branch, 0, sizeof(g_branch)); }

// ---- (a)
void* sd_fuse_oracle_kf_new(int N, const KeyPoint* keysUn, const uint8_t* desc, const float* uRight, const float* Tcw, const Camera* cam,
                            int nlevels, const float* scale, const float* invSigma2)
{
    KeyFrame* k = new KeyFrame();
    k->N = N;
    k->mvKeysUn.assign(keysUn, keysUn + N); k->mDescriptors.assign(desc, desc + (size_t)N * 32); k->mvuRight.assign(uRight, uRight + N);
    k->cam = *cam; k->nlevels = nlevels;
    k->mvScaleFactors.assign(scale, scale + nlevels); k->mvInvLevelSigma2.assign(invSigma2, invSigma2 + nlevels);
    k->mfLogScaleFactor = logf_cr(nlevels > 1 ? scale[1] : 1.0f);
    k->SetPose(Tcw);
    k->AssignFeaturesToGrid();
    return k;
}
void sd_fuse_oracle_kf_free(void* k) { delete (KeyFrame*)k; }

void sd_fuse_oracle_search(const void* kf, const PointRec* mp, const uint8_t* desc, float th, int32_t* best /*[2]*/)
{
    int bi, bd;
    SearchOne((const KeyFrame*)kf, *mp, desc, th, bi, bd);
    best[0] = bi; best[1] = bd;
}

// The reference's loop over one job; state (nullable, [N]: 0 empty, 1 a point that is not bad, 2 a bad point) is what the keyframe's
// features hold when the function starts, and AddMapPoint changes it as the loop goes.  -> nFused
int sd_fuse_oracle_job(const void* kf_, int n, const int32_t* cand, const PointRec* points, const uint8_t* descs, const uint8_t* state, float th,
                       int32_t* best /*[n][2]*/, Hit* hits, int32_t* nhits)
{
    const KeyFrame* pKF = (const KeyFrame*)kf_;
    std::vector<int> holds(pKF->N, -1);            // -1 empty, -2 a point of the keyframe, -3 a bad one, >= 0 the entry AddMapPoint put there
    if (state) for (int i = 0; i < pKF->N; i++) holds[i] = state[i] == 0 ? -1 : (state[i] == 1 ? -2 : -3);
    if (n == 0) g_branch[B_EMPTY_JOB]++;
    int nFused = 0, nh = 0;
    for (int i = 0; i < n; i++) {
        best[2 * i] = -1; best[2 * i + 1] = 256;
        if (cand[i] < 0) { g_branch[B_ENTRY_SKIP]++; continue; }
        int bestIdx, bestDist;
        SearchOne(pKF, points[cand[i]], descs + (size_t)cand[i] * 32, th, bestIdx, bestDist);
        best[2 * i] = bestIdx; best[2 * i + 1] = bestDist;
        if (bestDist <= TH_LOW) {
            Hit h = {i, bestIdx, bestDist, 0, -1};
            const int in = holds[bestIdx];
            if (in != -1) {
                if (in == -2) { h.action = ACT_MEET_KF; g_branch[B_MEET_KF]++; }
                else if (in == -3) { h.action = ACT_MEET_BAD; g_branch[B_MEET_BAD]++; }
                else { h.action = ACT_MEET_CANDIDATE; h.other = in; g_branch[B_MEET_CANDIDATE]++; }
            } else {
                h.action = ACT_ADD; g_branch[B_ADD]++;
                holds[bestIdx] = i;
            }
            hits[nh++] = h;
            nFused++;
        }
    }
    *nhits = nh;
    return nFused;
}

// ---- (b)
int sd_fuse_oracle_distinctive(int N, const uint8_t* descs, uint8_t* out /*nullable [32]*/)
{
    const int b = Distinctive(N, descs);
    if (b >= 0 && out) memcpy(out, descs + (size_t)b * 32, 32);
    return b;
}

// ---- (c)
void* sd_fuse_model_new() { return new Model(); }
void sd_fuse_model_free(void* m) { delete (Model*)m; }
int sd_fuse_model_add_kf(void* m_, void* kf)          // takes the keyframe of sd_fuse_oracle_kf_new over
{
    Model* m = (Model*)m_;
    ModelKF k; k.kf = (KeyFrame*)kf; k.mvpMapPoints.assign(k.kf->N, -1);
    m->kfs.push_back(k);
    return (int)m->kfs.size() - 1;
}
int sd_fuse_model_add_point(void* m_, const PointRec* rec, const uint8_t* desc, int bad)
{
    Model* m = (Model*)m_;
    MapPoint p; p.mnId = (int)m->pts.size(); p.rec = *rec; memcpy(p.mDescriptor, desc, 32); p.mbBad = bad != 0;
    m->pts.push_back(p);
    return p.mnId;
}
void sd_fuse_model_observe(void* m_, int p, int kf, int idx)           // AddObservation + AddMapPoint
{
    Model* m = (Model*)m_;
    m->AddObservation(p, kf, idx);
    m->kfs[kf].mvpMapPoints[idx] = p;
}
void sd_fuse_model_set_feature(void* m_, int kf, int idx, int p) { ((Model*)m_)->kfs[kf].mvpMapPoints[idx] = p; }     // mvpMapPoints alone
int sd_fuse_model_fuse(void* m_, int kf, int n, const int32_t* cand, float th) { return ((Model*)m_)->Fuse(kf, n, cand, th); }
// what a caller uploads for one job: entries (-1 where the reference `continue`s) and the feature states of the keyframe
void sd_fuse_model_snapshot(const void* m_, int kf, int n, const int32_t* cand, int32_t* entries, uint8_t* state)
{
    const Model* m = (const Model*)m_;
    for (int i = 0; i < n; i++) entries[i] = m->Skipped(kf, cand[i]) ? -1 : cand[i];
    const ModelKF& K = m->kfs[kf];
    for (int i = 0; i < K.kf->N; i++) state[i] = K.mvpMapPoints[i] < 0 ? 0 : (m->pts[K.mvpMapPoints[i]].mbBad ? 2 : 1);
}
// the search of every entry against the map as it stands (the snapshot), no tail
void sd_fuse_model_search(const void* m_, int kf, int n, const int32_t* cand, float th, int32_t* best)
{
    const Model* m = (const Model*)m_;
    for (int i = 0; i < n; i++) {
        best[2 * i] = -1; best[2 * i + 1] = 256;
        if (m->Skipped(kf, cand[i])) continue;
        int bi, bd;
        SearchOne(m->kfs[kf].kf, m->pts[cand[i]].rec, m->pts[cand[i]].mDescriptor, th, bi, bd);
        best[2 * i] = bi; best[2 * i + 1] = bd;
    }
}
// the tail in entry order over proposals found elsewhere -> nFused
int sd_fuse_model_tail(void* m_, int kf, int n, const int32_t* cand, const int32_t* best)
{
    Model* m = (Model*)m_;
    int nFused = 0;
    for (int i = 0; i < n; i++)
        if (cand[i] >= 0 && best[2 * i] >= 0 && m->Tail(kf, cand[i], best[2 * i], best[2 * i + 1])) nFused++;
    return nFused;
}
int sd_fuse_model_point_count(const void* m_) { return (int)((const Model*)m_)->pts.size(); }
void sd_fuse_model_points(const void* m_, PointRec* rec, uint8_t* desc, uint8_t* bad, int32_t* nobs)
{
    const Model* m = (const Model*)m_;
    for (size_t i = 0; i < m->pts.size(); i++) {
        rec[i] = m->pts[i].rec; memcpy(desc + i * 32, m->pts[i].mDescriptor, 32); bad[i] = m->pts[i].mbBad; nobs[i] = m->pts[i].nObs;
    }
}
// everything the model holds, in one canonical byte string
int sd_fuse_model_dump(const void* m_, uint8_t* out, int cap)
{
    const Model* m = (const Model*)m_;
    std::vector<uint8_t> o;
    for (const ModelKF& k : m->kfs) { put(o, (int32_t)k.mvpMapPoints.size()); for (int p : k.mvpMapPoints) put(o, (int32_t)p); }
    for (const MapPoint& p : m->pts) {
        put(o, (int32_t)p.mnId); put(o, (int32_t)p.mbBad); put(o, (int32_t)p.inMap); put(o, (int32_t)p.nObs); put(o, (int32_t)p.mnVisible);
        put(o, (int32_t)p.mnFound); put(o, (int32_t)p.mpReplaced);
        o.insert(o.end(), p.mDescriptor, p.mDescriptor + 32);
        put(o, (int32_t)p.mObservations.size());
        for (std::map<int, size_t>::const_iterator it = p.mObservations.begin(); it != p.mObservations.end(); it++) { put(o, (int32_t)it->first); put(o, (int32_t)it->second); }
    }
    if ((int)o.size() <= cap && out) memcpy(out, o.data(), o.size());
    return (int)o.size();
}

}
