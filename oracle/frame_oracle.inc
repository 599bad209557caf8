// TEST INFRASTRUCTURE — part of the CPU oracle (included by sd_oracle.cpp inside extern "C").
// Frame grid, UnprojectStereo and the Frame<->Frame projection matcher.
//
// Small cv::Mat products (3x3 * 3x1 + 3x1, CV_32F) are restated as plain f32 expressions
// evaluated left to right without contraction: t = (a0*b0 + a1*b1) + a2*b2; d = t + c
// [OpenCV-recall: cv::gemm small-matrix path; DESIGN.md "Oracle spec" Q5].

struct OrcCamera {   // Frame.h:160-210 statics
    float fx, fy, cx, cy, mbf, mb;
    float mnMinX, mnMaxX, mnMinY, mnMaxY;
};

static inline void mat3_mul_add(const float* R /*row-major 3x3, row stride rs*/, int rs, const float* x, const float* t,
                                float* out)
{
    for (int i = 0; i < 3; i++) {
        float s = R[i * rs + 0] * x[0] + R[i * rs + 1] * x[1];
        s = s + R[i * rs + 2] * x[2];
        out[i] = s + t[i];
    }
}

// Frame::PosInGrid (Frame.cc:790-800)
static inline bool PosInGrid(const KeyPoint& kp, const OrcCamera& c, int& posX, int& posY)
{
    const float wInv = static_cast<float>(FRAME_GRID_COLS) / static_cast<float>(c.mnMaxX - c.mnMinX);   // Frame.cc:276-277
    const float hInv = static_cast<float>(FRAME_GRID_ROWS) / static_cast<float>(c.mnMaxY - c.mnMinY);
    posX = (int)roundf((kp.x - c.mnMinX) * wInv);
    posY = (int)roundf((kp.y - c.mnMinY) * hInv);
    if (posX < 0 || posX >= FRAME_GRID_COLS || posY < 0 || posY >= FRAME_GRID_ROWS) return false;
    return true;
}

struct OrcGrid { std::vector<size_t> cell[FRAME_GRID_COLS][FRAME_GRID_ROWS]; };

// Frame::AssignFeaturesToGrid (Frame.cc:463-478)
static void AssignFeaturesToGrid(const KeyPoint* kpsUn, int N, const OrcCamera& c, OrcGrid& g)
{
    for (int i = 0; i < N; i++) {
        int x, y;
        if (PosInGrid(kpsUn[i], c, x, y)) g.cell[x][y].push_back(i);
    }
}

// Frame::GetFeaturesInArea (Frame.cc:735-788)
static std::vector<size_t> GetFeaturesInArea(const OrcGrid& g, const KeyPoint* kpsUn, const OrcCamera& c, float x, float y,
                                             float r, int minLevel, int maxLevel)
{
    std::vector<size_t> vIndices;
    const float wInv = static_cast<float>(FRAME_GRID_COLS) / static_cast<float>(c.mnMaxX - c.mnMinX);
    const float hInv = static_cast<float>(FRAME_GRID_ROWS) / static_cast<float>(c.mnMaxY - c.mnMinY);
    const int nMinCellX = std::max(0, (int)floorf((x - c.mnMinX - r) * wInv));
    if (nMinCellX >= FRAME_GRID_COLS) return vIndices;
    const int nMaxCellX = std::min((int)FRAME_GRID_COLS - 1, (int)ceilf((x - c.mnMinX + r) * wInv));
    if (nMaxCellX < 0) return vIndices;
    const int nMinCellY = std::max(0, (int)floorf((y - c.mnMinY - r) * hInv));
    if (nMinCellY >= FRAME_GRID_ROWS) return vIndices;
    const int nMaxCellY = std::min((int)FRAME_GRID_ROWS - 1, (int)ceilf((y - c.mnMinY + r) * hInv));
    if (nMaxCellY < 0) return vIndices;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
        for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
            const std::vector<size_t>& vCell = g.cell[ix][iy];
            for (size_t j = 0; j < vCell.size(); j++) {
                const KeyPoint& kpUn = kpsUn[vCell[j]];
                if (bCheckLevels) {
                    if (kpUn.octave < minLevel) continue;
                    if (maxLevel >= 0)
                        if (kpUn.octave > maxLevel) continue;
                }
                const float distx = kpUn.x - x, disty = kpUn.y - y;
                if (fabsf(distx) < r && fabsf(disty) < r) vIndices.push_back(vCell[j]);
            }
        }
    return vIndices;
}

// Grid cell of every keypoint (posX*48+posY, or -1 when outside), for tests of the device grid.
void orc_grid_cells(const void* kps_, int N, const float* cam10, int* cellOut)
{
    const KeyPoint* kps = (const KeyPoint*)kps_;
    OrcCamera c; memcpy(&c, cam10, sizeof(c));
    for (int i = 0; i < N; i++) {
        int x, y;
        cellOut[i] = PosInGrid(kps[i], c, x, y) ? x * FRAME_GRID_ROWS + y : -1;
    }
}

// Frame::UnprojectStereo (Frame.cc:1074-1088) for all keypoints; Twc = [mRwc | mOw] row-major 4x4.
// Points without depth get valid=0 and xw = 0.
void orc_unproject(const void* kps_, const float* depth, int N, const float* cam10, const float* Twc, float* xw,
                   uint8_t* valid)
{
    const KeyPoint* kps = (const KeyPoint*)kps_;
    OrcCamera c; memcpy(&c, cam10, sizeof(c));
    const float invfx = 1.0f / c.fx, invfy = 1.0f / c.fy;   // Frame.cc:283-284
    const float Ow[3] = {Twc[3], Twc[7], Twc[11]};
    for (int i = 0; i < N; i++) {
        const float z = depth[i];
        valid[i] = 0; xw[3 * i] = xw[3 * i + 1] = xw[3 * i + 2] = 0.f;
        if (z > 0) {
            const float u = kps[i].x, v = kps[i].y;
            const float x = (u - c.cx) * z * invfx;
            const float y = (v - c.cy) * z * invfy;
            const float p[3] = {x, y, z};
            mat3_mul_add(Twc, 4, p, Ow, &xw[3 * i]);
            valid[i] = 1;
        }
    }
}

// ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1758-1799) on bin sizes
static void ComputeThreeMaxima(const int* histoSize, const int L, int& ind1, int& ind2, int& ind3)
{
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < L; i++) {
        const int s = histoSize[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}

// ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th, bMono [, points_last, points_current])
// (ORBmatcher.cc:1485-1627 and the pair-emitting overload :407-559).
//   flags[i] bit0: LastFrame.mvpMapPoints[i] != NULL && !mvbOutlier[i];  bit1: pMP->Observations() > 0
//   xw[i]: pMP->GetWorldPos();  dMP: pMP->GetDescriptor() (32 B per point)
//   occupied[i2] (optional): CurrentFrame.mvpMapPoints[i2] already holds a point with Observations() > 0
//   match[i2]: index i of the Last-frame point now in CurrentFrame.mvpMapPoints[i2], or -1
//   pairs: (i, i2) for every accepted match, in order of i (points_last / points_current, :505-506)
//   outcome[i] (optional, the _ex entry): where Last-frame point i left the function, in the order of the reference's exits
enum { FF_NO_POINT, FF_BEHIND, FF_U_OUT, FF_V_OUT, FF_WINDOW_EMPTY, FF_NO_CANDIDATE, FF_DIST_HIGH, FF_MATCHED, FF_MATCHED_THEN_CULLED };
static int search_by_projection_impl(const void* kpC_, const uint8_t* descC, const float* uRightC, int Nc, const void* kpL_,
                                     const uint8_t* dMP, int Nl, const float* xw, const uint8_t* flags, const float* Tcw,
                                     const float* Tlw, const float* cam10, const float* scaleFactors, float th, int bMono,
                                     int checkOrientation, const uint8_t* occupied, int* match, int* pairs, int* npairs, int* outcome)
{
    const KeyPoint* kpC = (const KeyPoint*)kpC_; const KeyPoint* kpL = (const KeyPoint*)kpL_;
    OrcCamera c; memcpy(&c, cam10, sizeof(c));
    OrcGrid grid;
    AssignFeaturesToGrid(kpC, Nc, c, grid);
    int nmatches = 0;
    std::vector<int> rotHist[HISTO_LENGTH];
    std::vector<int> rotHistPoint[HISTO_LENGTH];      // the Last-frame point behind every rotHist entry (for outcome[] only)
    const float factor = 1.0f / HISTO_LENGTH;
    // twc = -Rcw.t()*tcw ; tlc = Rlw*twc + tlw
    float twc[3], tlc[3];
    const float tcw[3] = {Tcw[3], Tcw[7], Tcw[11]}, tlw[3] = {Tlw[3], Tlw[7], Tlw[11]};
    for (int i = 0; i < 3; i++) {
        float s = (-Tcw[0 * 4 + i]) * tcw[0] + (-Tcw[1 * 4 + i]) * tcw[1];
        s = s + (-Tcw[2 * 4 + i]) * tcw[2];
        twc[i] = s;
    }
    mat3_mul_add(Tlw, 4, twc, tlw, tlc);
    const bool bForward = tlc[2] > c.mb && !bMono;
    const bool bBackward = -tlc[2] > c.mb && !bMono;
    std::vector<uint8_t> taken(Nc, 0);      // mvpMapPoints[i2] && Observations() > 0
    for (int i = 0; i < Nc; i++) { match[i] = -1; if (occupied) taken[i] = occupied[i]; }
    int np = 0;
#define FF_EXIT(code) { if (outcome) outcome[i] = (code); continue; }
    for (int i = 0; i < Nl; i++) {
        if (!(flags[i] & 1)) FF_EXIT(FF_NO_POINT)
        float x3Dc[3];
        mat3_mul_add(Tcw, 4, &xw[3 * i], tcw, x3Dc);
        const float xc = x3Dc[0], yc = x3Dc[1];
        const float invzc = 1.0f / x3Dc[2];
        if (invzc < 0) FF_EXIT(FF_BEHIND)
        float u = c.fx * xc * invzc + c.cx;
        float v = c.fy * yc * invzc + c.cy;
        if (u < c.mnMinX || u > c.mnMaxX) FF_EXIT(FF_U_OUT)
        if (v < c.mnMinY || v > c.mnMaxY) FF_EXIT(FF_V_OUT)
        int nLastOctave = kpL[i].octave;
        float radius = th * scaleFactors[nLastOctave];
        std::vector<size_t> vIndices2;
        if (bForward) vIndices2 = GetFeaturesInArea(grid, kpC, c, u, v, radius, nLastOctave, -1);
        else if (bBackward) vIndices2 = GetFeaturesInArea(grid, kpC, c, u, v, radius, 0, nLastOctave);
        else vIndices2 = GetFeaturesInArea(grid, kpC, c, u, v, radius, nLastOctave - 1, nLastOctave + 1);
        if (vIndices2.empty()) FF_EXIT(FF_WINDOW_EMPTY)
        const uint8_t* d1 = dMP + (size_t)i * 32;
        int bestDist = 256, bestIdx2 = -1;
        for (size_t k = 0; k < vIndices2.size(); k++) {
            const size_t i2 = vIndices2[k];
            if (taken[i2]) continue;
            if (uRightC[i2] > 0) {
                const float ur = u - c.mbf * invzc;
                const float er = fabsf(ur - uRightC[i2]);
                if (er > radius) continue;
            }
            const int dist = DescriptorDistance(d1, descC + i2 * 32);
            if (dist < bestDist) { bestDist = dist; bestIdx2 = (int)i2; }
        }
        if (bestDist <= TH_HIGH) {
            match[bestIdx2] = i;
            if (flags[i] & 2) taken[bestIdx2] = 1;
            nmatches++;
            if (pairs) { pairs[2 * np] = i; pairs[2 * np + 1] = bestIdx2; }
            np++;
            if (checkOrientation) {
                float rot = kpL[i].angle - kpC[bestIdx2].angle;
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)roundf(rot * factor);
                if (bin == HISTO_LENGTH) bin = 0;
                rotHist[bin].push_back(bestIdx2);
                rotHistPoint[bin].push_back(i);
            }
            if (outcome) outcome[i] = FF_MATCHED;
        } else if (outcome) outcome[i] = bestIdx2 < 0 ? FF_NO_CANDIDATE : FF_DIST_HIGH;
    }
#undef FF_EXIT
    if (checkOrientation) {
        int ind1 = -1, ind2 = -1, ind3 = -1;
        int sizes[HISTO_LENGTH];
        for (int i = 0; i < HISTO_LENGTH; i++) sizes[i] = (int)rotHist[i].size();
        ComputeThreeMaxima(sizes, HISTO_LENGTH, ind1, ind2, ind3);
        for (int i = 0; i < HISTO_LENGTH; i++)
            if (i != ind1 && i != ind2 && i != ind3)
                for (size_t j = 0; j < rotHist[i].size(); j++) {
                    match[rotHist[i][j]] = -1; nmatches--;
                    if (outcome) outcome[rotHistPoint[i][j]] = FF_MATCHED_THEN_CULLED;
                }
    }
    if (npairs) *npairs = np;
    return nmatches;
}

int orc_search_by_projection(const void* kpC_, const uint8_t* descC, const float* uRightC, int Nc, const void* kpL_,
                             const uint8_t* dMP, int Nl, const float* xw, const uint8_t* flags, const float* Tcw,
                             const float* Tlw, const float* cam10, const float* scaleFactors, float th, int bMono,
                             int checkOrientation, const uint8_t* occupied, int* match, int* pairs, int* npairs)
{
    return search_by_projection_impl(kpC_, descC, uRightC, Nc, kpL_, dMP, Nl, xw, flags, Tcw, Tlw, cam10, scaleFactors, th, bMono,
                                     checkOrientation, occupied, match, pairs, npairs, 0);
}

int orc_search_by_projection_ex(const void* kpC_, const uint8_t* descC, const float* uRightC, int Nc, const void* kpL_,
                                const uint8_t* dMP, int Nl, const float* xw, const uint8_t* flags, const float* Tcw,
                                const float* Tlw, const float* cam10, const float* scaleFactors, float th, int bMono,
                                int checkOrientation, const uint8_t* occupied, int* match, int* pairs, int* npairs, int* outcome)
{
    return search_by_projection_impl(kpC_, descC, uRightC, Nc, kpL_, dMP, Nl, xw, flags, Tcw, Tlw, cam10, scaleFactors, th, bMono,
                                     checkOrientation, occupied, match, pairs, npairs, outcome);
}

// ---------------------------------------------------------------------------------------------------------
// Local-map search: Frame::isInFrustum (Frame.cc:677-733) for every local map point, then
// ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (ORBmatcher.cc:45-129), as
// Tracking::SearchLocalPoints runs them (Tracking.cc:2014-2064).
//   OpenCV leaves [OpenCV-recall, DESIGN.md Q11]: cv::norm(3x1 f32) = sqrt in double of a double sum of squares;
//   Mat::dot(3x1 f32) accumulates in double; std::log(float) is taken correctly rounded (double log, rounded to f32).
// ---------------------------------------------------------------------------------------------------------
struct OrcMapPoint {       // 36 B
    float xw[3];           // pMP->GetWorldPos()
    float normal[3];       // pMP->GetNormal()
    float minDistance;     // mfMinDistance (GetMinDistanceInvariance() = 0.8f * this, MapPoint.cc:373-377)
    float maxDistance;     // mfMaxDistance (GetMaxDistanceInvariance() = 1.2f * this, MapPoint.cc:379-383)
    uint32_t flags;        // bit0: !isBad() && mnLastFrameSeen != frame id (SearchLocalPoints :2041-2044); bit1: Observations() > 0
};
struct OrcTrack { float projX, projY, projXR, viewCos; int32_t level; int32_t inView; };   // mTrackProj*, mTrackViewCos, mnTrackScaleLevel, mbTrackInView

static inline float logf_cr(float x) { return (float)log((double)x); }

// MapPoint::PredictScale(const float&, Frame*) (MapPoint.cc:402-417)
static inline int PredictScale(float maxDistance, float currentDist, float logScaleFactor, int nScaleLevels)
{
    const float ratio = maxDistance / currentDist;
    int nScale = (int)ceilf(logf_cr(ratio) / logScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= nScaleLevels) nScale = nScaleLevels - 1;
    return nScale;
}

// why: the exit taken (LM_*), LM_MATCHED standing for "in view" until the search decides
enum { LM_FLAG_OFF, LM_BEHIND, LM_U_OUT, LM_V_OUT, LM_DIST_BELOW_MIN, LM_DIST_ABOVE_MAX, LM_VIEW_ANGLE, LM_WINDOW_EMPTY, LM_NO_CANDIDATE,
       LM_DIST_HIGH, LM_RATIO, LM_MATCHED };
static bool isInFrustum(const OrcMapPoint& mp, const float* Tcw, const float* Ow, const OrcCamera& c, float logScaleFactor,
                        int nScaleLevels, float viewingCosLimit, OrcTrack& t, int& why)
{
    t.inView = 0;
    const float tcw[3] = {Tcw[3], Tcw[7], Tcw[11]};
    float Pc[3];
    mat3_mul_add(Tcw, 4, mp.xw, tcw, Pc);
    const float PcX = Pc[0], PcY = Pc[1], PcZ = Pc[2];
    if (PcZ < 0.0f) { why = LM_BEHIND; return false; }
    const float invz = 1.0f / PcZ;
    const float u = c.fx * PcX * invz + c.cx;
    const float v = c.fy * PcY * invz + c.cy;
    if (u < c.mnMinX || u > c.mnMaxX) { why = LM_U_OUT; return false; }
    if (v < c.mnMinY || v > c.mnMaxY) { why = LM_V_OUT; return false; }
    const float maxDistance = 1.2f * mp.maxDistance;
    const float minDistance = 0.8f * mp.minDistance;
    const float PO[3] = {mp.xw[0] - Ow[0], mp.xw[1] - Ow[1], mp.xw[2] - Ow[2]};
    double s2 = 0;
    for (int i = 0; i < 3; i++) s2 += (double)PO[i] * (double)PO[i];
    const float dist = (float)sqrt(s2);
    if (dist < minDistance || dist > maxDistance) { why = dist < minDistance ? LM_DIST_BELOW_MIN : LM_DIST_ABOVE_MAX; return false; }
    double dot = 0;
    for (int i = 0; i < 3; i++) dot += (double)PO[i] * (double)mp.normal[i];
    const float viewCos = (float)(dot / (double)dist);
    if (viewCos < viewingCosLimit) { why = LM_VIEW_ANGLE; return false; }
    why = LM_MATCHED;
    const int nPredictedLevel = PredictScale(mp.maxDistance, dist, logScaleFactor, nScaleLevels);
    t.inView = 1;
    t.projX = u;
    t.projXR = u - c.mbf * invz;
    t.projY = v;
    t.level = nPredictedLevel;
    t.viewCos = viewCos;
    return true;
}

// Returns nmatches.  occupied[i] (optional): F.mvpMapPoints[i] holds a point with Observations() > 0 before the call.
// mpMatch[m] = keypoint index given to map point m (or -1); kpMatch[i] = map point finally stored in F.mvpMapPoints[i] by
// this call (or -1); track[m] = the isInFrustum outputs.
// outcome[m] (optional, the _ex entry): LM_*; best[4 * m ..] (optional): bestDist, bestDist2, bestLevel, bestLevel2 as they stood at
// the ratio test (256 / -1 where the search was not reached or found nothing).
static int search_local_map_impl(const void* kpF_, const uint8_t* descF, const float* uRightF, int N, const void* mps_,
                                 const uint8_t* mpDesc, int M, const float* Tcw, const float* cam10, const float* scaleFactors,
                                 int nScaleLevels, float th, float nnratio, float viewingCosLimit, const uint8_t* occupied,
                                 void* track_, int* mpMatch, int* kpMatch, int* outcome, int* best)
{
    const KeyPoint* kpF = (const KeyPoint*)kpF_;
    const OrcMapPoint* mps = (const OrcMapPoint*)mps_;
    OrcTrack* track = (OrcTrack*)track_;
    OrcCamera c; memcpy(&c, cam10, sizeof(c));
    OrcGrid grid;
    AssignFeaturesToGrid(kpF, N, c, grid);
    const float logScaleFactor = logf_cr(scaleFactors[1]);      // Frame.cc:80 mfLogScaleFactor = log(mfScaleFactor)
    // Frame::UpdatePoseMatrices (Frame.cc:667-674): mOw = -mRcw.t()*mtcw
    float Ow[3];
    for (int i = 0; i < 3; i++) {
        float s = (-Tcw[0 * 4 + i]) * Tcw[3] + (-Tcw[1 * 4 + i]) * Tcw[7];
        s = s + (-Tcw[2 * 4 + i]) * Tcw[11];
        Ow[i] = s;
    }
    std::vector<uint8_t> taken(N, 0);
    for (int i = 0; i < N; i++) { kpMatch[i] = -1; if (occupied) taken[i] = occupied[i]; }
    for (int m = 0; m < M; m++) {
        mpMatch[m] = -1;
        memset(&track[m], 0, sizeof(OrcTrack));
        int why = LM_FLAG_OFF;
        if (mps[m].flags & 1) isInFrustum(mps[m], Tcw, Ow, c, logScaleFactor, nScaleLevels, viewingCosLimit, track[m], why);
        if (outcome) outcome[m] = why;
        if (best) { best[4 * m] = 256; best[4 * m + 1] = 256; best[4 * m + 2] = -1; best[4 * m + 3] = -1; }
    }
    int nmatches = 0;
    const bool bFactor = th != 1.0;
    for (int iMP = 0; iMP < M; iMP++) {
        const OrcTrack& t = track[iMP];
        if (!t.inView) continue;
        const int nPredictedLevel = t.level;
        float r = t.viewCos > 0.998 ? 2.5f : 4.0f;             // RadiusByViewingCos (:131-137)
        if (bFactor) r *= th;
        const std::vector<size_t> vIndices =
            GetFeaturesInArea(grid, kpF, c, t.projX, t.projY, r * scaleFactors[nPredictedLevel], nPredictedLevel - 1, nPredictedLevel);
        if (vIndices.empty()) { if (outcome) outcome[iMP] = LM_WINDOW_EMPTY; continue; }
        const uint8_t* MPdescriptor = mpDesc + (size_t)iMP * 32;
        int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
        for (size_t k = 0; k < vIndices.size(); k++) {
            const size_t idx = vIndices[k];
            if (taken[idx]) continue;
            if (uRightF[idx] > 0) {
                const float er = fabsf(t.projXR - uRightF[idx]);
                if (er > r * scaleFactors[nPredictedLevel]) continue;
            }
            const int dist = DescriptorDistance(MPdescriptor, descF + idx * 32);
            if (dist < bestDist) {
                bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = kpF[idx].octave; bestIdx = (int)idx;
            } else if (dist < bestDist2) {
                bestLevel2 = kpF[idx].octave; bestDist2 = dist;
            }
        }
        if (best) { best[4 * iMP] = bestDist; best[4 * iMP + 1] = bestDist2; best[4 * iMP + 2] = bestLevel; best[4 * iMP + 3] = bestLevel2; }
        if (outcome) outcome[iMP] = bestIdx < 0 ? LM_NO_CANDIDATE : LM_DIST_HIGH;
        if (bestDist <= TH_HIGH) {
            if (bestLevel == bestLevel2 && bestDist > nnratio * bestDist2) { if (outcome) outcome[iMP] = LM_RATIO; continue; }
            kpMatch[bestIdx] = iMP;
            if (mps[iMP].flags & 2) taken[bestIdx] = 1;
            mpMatch[iMP] = bestIdx;
            nmatches++;
            if (outcome) outcome[iMP] = LM_MATCHED;
        }
    }
    return nmatches;
}

int orc_search_local_map(const void* kpF_, const uint8_t* descF, const float* uRightF, int N, const void* mps_,
                         const uint8_t* mpDesc, int M, const float* Tcw, const float* cam10, const float* scaleFactors,
                         int nScaleLevels, float th, float nnratio, float viewingCosLimit, const uint8_t* occupied,
                         void* track_, int* mpMatch, int* kpMatch)
{
    return search_local_map_impl(kpF_, descF, uRightF, N, mps_, mpDesc, M, Tcw, cam10, scaleFactors, nScaleLevels, th, nnratio,
                                 viewingCosLimit, occupied, track_, mpMatch, kpMatch, 0, 0);
}

int orc_search_local_map_ex(const void* kpF_, const uint8_t* descF, const float* uRightF, int N, const void* mps_,
                            const uint8_t* mpDesc, int M, const float* Tcw, const float* cam10, const float* scaleFactors,
                            int nScaleLevels, float th, float nnratio, float viewingCosLimit, const uint8_t* occupied,
                            void* track_, int* mpMatch, int* kpMatch, int* outcome, int* best)
{
    return search_local_map_impl(kpF_, descF, uRightF, N, mps_, mpDesc, M, Tcw, cam10, scaleFactors, nScaleLevels, th, nnratio,
                                 viewingCosLimit, occupied, track_, mpMatch, kpMatch, outcome, best);
}

// ---------------------------------------------------------------------------------------------------------
// Frame::UndistortKeyPoints / ComputeImageBounds (Frame.cc:812-872) for a camera WITH distortion:
// cv::undistortPoints(src, dst, mK, mDistCoef, cv::Mat(), mK) [OpenCV-recall, 3.4.x, modules/imgproc/src/undistort.cpp
// cvUndistortPointsInternal]: all arithmetic in double; x = (u - cx)/fx, y = (v - cy)/fy; five fixed-point iterations of
//   r2 = x*x + y*y;  icdist = (1 + ((k6*r2 + k5)*r2 + k4)*r2) / (1 + ((k3*r2 + k2)*r2 + k1)*r2)   [k4..k6 = 0 here]
//   dX = 2*p1*x*y + p2*(r2 + 2*x*x);  dY = p1*(r2 + 2*y*y) + 2*p2*x*y;  x = (x0 - dX)*icdist;  y = (y0 - dY)*icdist
// then u' = x*fx + cx, v' = y*fy + cy (P = mK), stored as f32.  dist = (k1, k2, p1, p2, k3) as Tracking.cc:76-90 fills it.
// ---------------------------------------------------------------------------------------------------------
void orc_undistort_points(const float* pts, int N, const float* K4 /*fx fy cx cy*/, const float* dist5, float* out)
{
    const double fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    const double k1 = dist5[0], k2 = dist5[1], p1 = dist5[2], p2 = dist5[3], k3 = dist5[4];
    const double ifx = 1. / fx, ify = 1. / fy;
    for (int i = 0; i < N; i++) {
        double x = pts[2 * i], y = pts[2 * i + 1];
        x = (x - cx) * ifx; y = (y - cy) * ify;
        const double x0 = x, y0 = y;
        for (int j = 0; j < 5; j++) {
            const double r2 = x * x + y * y;
            const double icdist = (1 + ((0. * r2 + 0.) * r2 + 0.) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2);
            const double deltaX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
            const double deltaY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
            x = (x0 - deltaX) * icdist;
            y = (y0 - deltaY) * icdist;
        }
        out[2 * i] = (float)(x * fx + cx);
        out[2 * i + 1] = (float)(y * fy + cy);
    }
}

// Frame::ComputeImageBounds (Frame.cc:844-872): mnMinX, mnMaxX, mnMinY, mnMaxY
void orc_image_bounds(int cols, int rows, const float* K4, const float* dist5, float* bounds4)
{
    if (dist5[0] != 0.0f) {
        const float corners[8] = {0.f, 0.f, (float)cols, 0.f, 0.f, (float)rows, (float)cols, (float)rows};
        float u[8];
        orc_undistort_points(corners, 4, K4, dist5, u);
        bounds4[0] = std::min(u[0], u[4]); bounds4[1] = std::max(u[2], u[6]);
        bounds4[2] = std::min(u[1], u[3]); bounds4[3] = std::max(u[5], u[7]);
    } else {
        bounds4[0] = 0.0f; bounds4[1] = (float)cols; bounds4[2] = 0.0f; bounds4[3] = (float)rows;
    }
}
