// The matchers of LoopClosing::ComputeSim3 / SearchAndFuse as batched kernels (gfx950, wave64):
//   k_search_by_bow_kf   ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12)                         src/ORBmatcher.cc:679-812
//   k_loop_search<0>     the per-candidate search of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, ..)  src/ORBmatcher.cc:1134-1236
//   k_loop_search<1>     the per-candidate window of SearchByProjection(pKF, Scw, vpPoints, ..)    src/ORBmatcher.cc:290-392
//   k_loop_assign        its sequential greedy `vpMatched[bestIdx] = pMP`                          src/ORBmatcher.cc:372-398
// Both Scw functions receive [Rcw | tcw] already decomposed (sd_scw.h) and are k_fuse_search without its chi-square and
// uRight tests: the view of the point, PredictScale, the GetFeaturesInArea window and its walk are the shared ones of k_area.h.  The
// tail of the Sim3 Fuse is k_fuse_resolve (k_fuse.h), unchanged.
// SearchByProjection is a greedy: a feature taken by an earlier candidate is invisible to the later ones.  k_loop_search<1> keeps, per
// candidate, the SD_PROJ_K smallest (distance, visiting order) keys over the features that were free on entry: what the reference finds
// at the candidate's turn is the first key whose feature is still free.  k_loop_assign replays the candidates in order, 64 at a time:
// every lane picks against the committed state, the lanes before the first one whose pick an earlier lane of the round takes are final
// and commit, the others pick again.  The first undecided lane never conflicts, so a round commits at least one candidate, and what is
// committed is exactly what the sequential loop gives.  A candidate whose SD_PROJ_K keys are all taken while its window held more sets
// SD_ERR_LOOP_LIST: the answer is refused (sd_batch_sync), never guessed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_area.h"
#include "k_match.h"
#include "k_fuse.h"

#define SD_ERR_LOOP_LIST 128     // bit of the workspace's capacity flag (sd_batch_sync)
#define SD_LOOP_ERR_POINT 1      // a candidate or a d_matched value outside its table

// ORBmatcher.cc:1165-1206 / :320-360 for one point: the projection and every `continue` before GetFeaturesInArea.
struct SdLoopView { bool ok; float u, v, radius; int level; };
__device__ __forceinline__ SdLoopView sd_loop_view(const SdMapPoint& mp, const float* __restrict__ T, const SdCamera& cam,
                                                   const float* s_scale, int nlevels, float th)
{
    SdLoopView w; w.ok = true; w.level = 0; w.radius = 0.f;
    float xc, yc, zc;
    sd_mat3_mul_add(T, mp.xw[0], mp.xw[1], mp.xw[2], xc, yc, zc);
    if (zc < 0.0f) w.ok = false;
    const float invz = 1.0f / zc;
    const float x = xc * invz, y = yc * invz;
    w.u = cam.fx * x + cam.cx;
    w.v = cam.fy * y + cam.cy;
    if (!(w.u >= cam.mnMinX && w.u < cam.mnMaxX && w.v >= cam.mnMinY && w.v < cam.mnMaxY)) w.ok = false;      // KeyFrame::IsInImage
    float ox, oy, oz;
    sd_cam_centre(T, ox, oy, oz);
    const SdPointView pv = sd_view_of_point(mp, ox, oy, oz);
    if (pv.dist3D < 0.8f * mp.minDistance || pv.dist3D > 1.2f * mp.maxDistance) w.ok = false;
    if (pv.dot < 0.5 * (double)pv.dist3D) w.ok = false;
    if (w.ok) {
        w.level = sd_predict_scale(mp.maxDistance, pv.dist3D, s_scale[1], nlevels);
        w.radius = th * s_scale[w.level];
    }
    return w;
}

// One wave per entry, grid.y = job.
// MODE 0 (Fuse): best[e] = (bestIdx, bestDist) with bestDist starting at INT_MAX: a lone member at distance 256 is (idx, 256);
//                (-1, 256) when the point was rejected or no feature passed the level gate.
// MODE 1 (SearchByProjection): matched = the job's incoming vpMatched row ([cap]: -1 free, >= 0 a point, -2 a point outside the table).
//                A candidate that occurs in the row is in spAlreadyFound and skipped; a feature with matched != -1 is no target;
//                list[e][k] = (distance << 16 | feature) of the k-th smallest (distance, visiting order) key with distance < 256,
//                listN[e] = how many keys the window held.
template <int MODE>
__global__ void __launch_bounds__(256) k_loop_search(
    const sd_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc, const float* __restrict__ uRight,
    const unsigned short* __restrict__ sortedIdx, const unsigned short* __restrict__ cellStart, const int* __restrict__ count,
    const SdMapPoint* __restrict__ mps, const uint8_t* __restrict__ mpDesc, int nPoints, const int* __restrict__ frameOf,
    const int* __restrict__ candOff, const int* __restrict__ candPoint, const float* __restrict__ Tcw,
    const int* __restrict__ matched /*MODE 1: [n_jobs][cap]*/, int2* __restrict__ best /*MODE 0*/, unsigned* __restrict__ list /*MODE 1*/,
    int* __restrict__ listN /*MODE 1*/, int* __restrict__ errFlag, SdLevelTables L, SdCamera cam, float th, int cap)
{
    __shared__ float s_scale[SD_MAX_LEVELS];
    __shared__ unsigned long long s_row[4][SD_PROJ_K];
    if (threadIdx.x < SD_MAX_LEVELS) s_scale[threadIdx.x] = L.scale[threadIdx.x];
    __syncthreads();
    const int job = blockIdx.y;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e0 = candOff[job], M = candOff[job + 1] - e0;
    const int el = blockIdx.x * 4 + wv;
    if (el >= M) return;
    const int e = e0 + el;
    const int m = candPoint[e];
    const float* T = Tcw + (size_t)job * 16;
    bool ok = m >= 0 && m < nPoints;
    if ((m < -1 || m >= nPoints) && lane == 0) atomicOr(errFlag, SD_LOOP_ERR_POINT);
    const int img = frameOf[job];
    const int* mrow = MODE == 1 ? matched + (size_t)job * cap : nullptr;
    if (MODE == 1) {                                             // spAlreadyFound.count(pMP); every wave checks the whole row's range
        const int N = count[img];
        bool found = false, outside = false;
        for (int i = lane; i < N; i += 64) { const int held = mrow[i]; found |= held == m; outside |= held < -2 || held >= nPoints; }
        if (outside) atomicOr(errFlag, SD_LOOP_ERR_POINT);
        if (ok && __any(found)) ok = false;
    }
    unsigned bestKey = 0xFFFFFFFFu;          // MODE 0: (distance << 16 | walk position)
    int bestIdx = -1;
    SdBest64 top;                            // MODE 1
    if (ok) {
        const SdMapPoint mp = mps[m];
        const SdLoopView w = sd_loop_view(mp, T, cam, s_scale, L.nlevels, th);
        if (w.ok) {
            const SdAreaWindow W = sd_area_window(cam, w.u, w.v, w.radius);
            if (!W.empty) {
                const uint4* dl = (const uint4*)(mpDesc + (size_t)m * 32);
                const uint4 l0 = dl[0], l1 = dl[1];
                const SdImageArrays C = sd_image_arrays(kp, nullptr, uRight, desc, sortedIdx, cellStart, img, cap);
                const SdAreaWalk<64> walk(C, W, true, lane);
                for (int base = 0; base < walk.total; base += 64) {      // a window of more than 64 features takes several passes
                    const int tt = base + lane;
                    const int i2 = walk.member(tt);
                    bool hit = false;
                    int dist = 256;
                    if (i2 >= 0) {
                        const sd_keypoint k = C.kp[i2];
                        const float distx = k.x - w.u, disty = k.y - w.v;
                        if (fabsf(distx) < w.radius && fabsf(disty) < w.radius && k.octave >= w.level - 1 && k.octave <= w.level) {
                            bool isFree = true;
                            if (MODE == 1) {
                                const int held = mrow[i2];
                                isFree = held == -1 || held < -2 || held >= nPoints;      // outside the table: read as -1 (flagged by the row scan)
                            }
                            if (isFree) {
                                const uint4* dr = (const uint4*)(C.desc + (size_t)i2 * 32);
                                dist = sd_hamming256(l0, l1, dr[0], dr[1]);
                                hit = true;
                            }
                        }
                    }
                    if (MODE == 0) {
                        const unsigned key = ((unsigned)dist << 16) | (unsigned)tt;
                        if (hit && key < bestKey) { bestKey = key; bestIdx = i2; }
                    } else {
                        hit = hit && dist < 256;
                        top.push(s_row[wv], lane, hit, ((unsigned long long)(unsigned)dist << 32) | ((unsigned long long)(unsigned)tt << 16) | (unsigned)(i2 & 0xFFFF));
                    }
                }
            }
        }
    }
    if (MODE == 0) {
        const unsigned w = sd_wave_min_u32(bestKey);
        int2 out = make_int2(-1, 256);
        if (w != 0xFFFFFFFFu) {
            const unsigned long long who = __ballot(bestKey == w);           // keys are unique: the walk position is in the low bits
            out.x = __shfl(bestIdx, __ffsll((long long)who) - 1, 64);
            out.y = (int)(w >> 16);
        }
        if (lane == 0) best[e] = out;
    } else {
        const unsigned long long key = top.finish(s_row[wv], lane);
        if (key != ~0ull) list[(size_t)e * SD_PROJ_K + lane] = ((unsigned)(key >> 32) << 16) | (unsigned)(key & 0xFFFFu);
        if (lane == 0) listN[e] = top.n;
    }
}

// One wave per job: the candidates in order, 64 per chunk (see the head of this file).  taken = one bit per feature in dynamic LDS
// ((cap + 31) / 32 words).  assigned[job][idx] = position of the candidate that took the feature (-1 elsewhere, all cap entries
// written), best[e] = (bestIdx, bestDist) as found at the candidate's turn, nmatch[job] = the return value.
__global__ void __launch_bounds__(64) k_loop_assign(const int* __restrict__ candOff, const unsigned* __restrict__ list,
                                                    const int* __restrict__ listN, int cap, int* __restrict__ assigned,
                                                    int2* __restrict__ best, int* __restrict__ nmatch, int* __restrict__ capFlag)
{
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned* taken = (unsigned*)smem;
    const int job = blockIdx.x, lane = threadIdx.x;
    const int e0 = candOff[job], M = candOff[job + 1] - e0;
    int* arow = assigned + (size_t)job * cap;
    for (int i = lane; i < (cap + 31) / 32; i += 64) taken[i] = 0u;
    for (int i = lane; i < cap; i += 64) arow[i] = -1;
    __syncthreads();
    int nm = 0;
    for (int base = 0; base < M; base += 64) {
        const int p = base + lane;
        const size_t e = (size_t)e0 + p;
        bool done = p >= M;
        const int total = done ? 0 : listN[e];
        const int n = total < SD_PROJ_K ? total : SD_PROJ_K;
        const unsigned* mine = list + e * SD_PROJ_K;
        int cursor = 0;
        while (__any(!done)) {
            int pickIdx = -1, pickDist = 256;
            if (!done) {
                while (cursor < n) {
                    const unsigned k = mine[cursor];
                    const int idx = (int)(k & 0xFFFFu);
                    if (!((taken[idx >> 5] >> (idx & 31)) & 1u)) { pickIdx = idx; pickDist = (int)(k >> 16); break; }
                    cursor++;
                }
            }
            const bool take = !done && pickIdx >= 0 && pickDist <= SD_TH_LOW;
            bool conflict = false;
            unsigned long long tm = __ballot(take);
            while (tm) {                                               // wave-uniform: the lanes that would take a feature this round
                const int j = __ffsll((long long)tm) - 1;
                tm &= tm - 1;
                const int ij = __builtin_amdgcn_readlane(pickIdx, j);
                if (!done && j < lane && ij == pickIdx) conflict = true;
            }
            const unsigned long long cm = __ballot(conflict);
            const int firstC = cm ? __ffsll((long long)cm) - 1 : 64;
            if (!done && lane < firstC) {
                if (take) { atomicOr(&taken[pickIdx >> 5], 1u << (pickIdx & 31)); arow[pickIdx] = p; nm++; }
                if (pickIdx < 0 && total > SD_PROJ_K) atomicOr(capFlag, SD_ERR_LOOP_LIST);     // every kept key taken, the window held more
                best[e] = make_int2(pickIdx, pickDist);
                done = true;
            }
            __syncthreads();                                           // one wave: orders the LDS bits before the next round's reads
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) nm += __shfl_xor(nm, d, 64);
    if (lane == 0) nmatch[job] = nm;
}

// ---------------------------------------------------------------- ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12)
// The shared body of k_match.h: one workgroup per pair, a wave per FeatureVector node both keyframes share, KF1's features of the node
// in order, best and second best over the not-yet-taken valid KF2 features; the register path up to SD_BOW_REGF KF2 features, the
// memory path beyond.  What differs from k_search_by_bow: the result is indexed by the KF1 feature (match12[idx1] = idx2), KF2 has a
// validity mask too, the acceptance is bestDist1 < TH_LOW (strict), and the histogram holds idx1.
__global__ void __launch_bounds__(64 * SD_BOW_WAVES) k_search_by_bow_kf(
    const sd_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc, const int* __restrict__ count,
    const unsigned* __restrict__ fvFeat, const int* __restrict__ fvRunStart, const unsigned* __restrict__ fvRunNode,
    const int* __restrict__ meta, const uint8_t* __restrict__ valid1 /*nullable [pair][cap]*/, const uint8_t* __restrict__ valid2,
    const int2* __restrict__ pairIdx, int cap, float nnratio, int checkOrientation, int* __restrict__ matchOut, int* __restrict__ nmatchOut)
{
    sd_search_by_bow<true, true>(kp, desc, count, fvFeat, fvRunStart, fvRunNode, meta, valid1, valid2, pairIdx, cap, nnratio,
                                 checkOrientation, matchOut, nmatchOut);
}
