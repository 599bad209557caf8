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
#include "k_bow.h"
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
        unsigned w = bestKey;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { const unsigned o = (unsigned)__shfl_xor((int)w, d, 64); w = o < w ? o : w; }
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
// The structure of k_search_by_bow (k_bow.h): one workgroup per pair, a wave per FeatureVector node both keyframes share, KF1's
// features of the node in order, best and second best over the not-yet-taken valid KF2 features; the register path up to SD_BOW_REGF
// KF2 features, the memory path beyond.  What differs: the result is indexed by the KF1 feature (match12[idx1] = idx2), KF2 has a
// validity mask too, the acceptance is bestDist1 < TH_LOW (strict), and the histogram holds idx1.
__global__ void __launch_bounds__(64 * SD_BOW_WAVES) k_search_by_bow_kf(
    const sd_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc, const int* __restrict__ count,
    const unsigned* __restrict__ fvFeat, const int* __restrict__ fvRunStart, const unsigned* __restrict__ fvRunNode,
    const int* __restrict__ meta, const uint8_t* __restrict__ valid1 /*nullable [pair][cap]*/, const uint8_t* __restrict__ valid2,
    const int2* __restrict__ pairIdx, int cap, float nnratio, int checkOrientation, int* __restrict__ matchOut, int* __restrict__ nmatchOut)
{
    extern __shared__ __align__(16) unsigned char smem[];
    int* s_match = (int*)smem;                               // [cap] match12
    uint8_t* s_bin = (uint8_t*)(s_match + cap);              // [cap] by idx1
    uint8_t* s_taken = s_bin + cap;                          // [cap] vbMatched2 (the memory path)
    __shared__ int s_hist[SD_HISTO];
    __shared__ int s_ind[3];
    __shared__ int s_nm;
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int img1 = pairIdx[pair].x, img2 = pairIdx[pair].y;
    const int N1 = count[img1], N2 = count[img2];
    for (int i = tid; i < N1; i += 64 * SD_BOW_WAVES) s_match[i] = -1;
    for (int i = tid; i < N2; i += 64 * SD_BOW_WAVES) s_taken[i] = 0;
    if (tid < SD_HISTO) s_hist[tid] = 0;
    if (tid == 0) s_nm = 0;
    __syncthreads();
    const int runs1 = meta[img1 * 4 + 1], runs2 = meta[img2 * 4 + 1];
    const int* rs1 = fvRunStart + (size_t)img1 * (cap + 1);
    const int* rs2 = fvRunStart + (size_t)img2 * (cap + 1);
    const unsigned* rn1 = fvRunNode + (size_t)img1 * cap;
    const unsigned* rn2 = fvRunNode + (size_t)img2 * cap;
    const unsigned* ff1 = fvFeat + (size_t)img1 * cap;
    const unsigned* ff2 = fvFeat + (size_t)img2 * cap;
    const uint8_t* d1 = desc + (size_t)img1 * cap * 32;
    const uint8_t* d2 = desc + (size_t)img2 * cap * 32;
    const sd_keypoint* k1p = kp + (size_t)img1 * cap;
    const sd_keypoint* k2p = kp + (size_t)img2 * cap;
    const uint8_t* v1 = valid1 ? valid1 + (size_t)pair * cap : nullptr;
    const uint8_t* v2 = valid2 ? valid2 + (size_t)pair * cap : nullptr;
    const float factor = 1.0f / SD_HISTO;
    int nm = 0;
    for (int rk = wv; rk < runs1; rk += SD_BOW_WAVES) {
        const unsigned node = rn1[rk];
        int lo = 0, hi = runs2;                               // lower_bound of node in KF2's runs
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (rn2[mid] < node) lo = mid + 1; else hi = mid; }
        if (lo >= runs2 || rn2[lo] != node) continue;
        const int a0 = rs1[rk], a1 = rs1[rk + 1], c0 = rs2[lo], c1 = rs2[lo + 1];
        if (c1 - c0 <= SD_BOW_REGF) {
            // ---- the register path: lane l owns KF2 positions l and l + 64 of the node and their taken flags
            unsigned i2l[2]; uint4 f0[2], f1[2]; bool freeF[2];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const int c = c0 + lane + 64 * q;
                freeF[q] = c < c1;
                i2l[q] = freeF[q] ? ff2[c] : 0u;
                if (freeF[q] && v2 && !v2[i2l[q]]) freeF[q] = false;
                const uint4* pf = (const uint4*)(d2 + (size_t)i2l[q] * 32);
                f0[q] = pf[0]; f1[q] = pf[1];
            }
            for (int kb = a0; kb < a1; kb += 64) {
                const int a = kb + lane;
                const unsigned i1l = a < a1 ? ff1[a] : 0u;
                const int ok1 = a < a1 && (!v1 || v1[i1l]);
                const uint4* pk = (const uint4*)(d1 + (size_t)i1l * 32);
                const uint4 kl0 = pk[0], kl1 = pk[1];
                const float ang1 = k1p[i1l].angle;
                const int nstep = a1 - kb < 64 ? a1 - kb : 64;
                for (int t = 0; t < nstep; t++) {
                    if (!__builtin_amdgcn_readlane(ok1, t)) continue;
                    uint4 k0, k1;
                    k0.x = (unsigned)__builtin_amdgcn_readlane((int)kl0.x, t); k0.y = (unsigned)__builtin_amdgcn_readlane((int)kl0.y, t);
                    k0.z = (unsigned)__builtin_amdgcn_readlane((int)kl0.z, t); k0.w = (unsigned)__builtin_amdgcn_readlane((int)kl0.w, t);
                    k1.x = (unsigned)__builtin_amdgcn_readlane((int)kl1.x, t); k1.y = (unsigned)__builtin_amdgcn_readlane((int)kl1.y, t);
                    k1.z = (unsigned)__builtin_amdgcn_readlane((int)kl1.z, t); k1.w = (unsigned)__builtin_amdgcn_readlane((int)kl1.w, t);
                    unsigned key[2];
#pragma unroll
                    for (int q = 0; q < 2; q++)
                        key[q] = freeF[q] ? (((unsigned)sd_hamming256(k0, k1, f0[q], f1[q]) << 16) | (unsigned)(lane + 64 * q)) : 0xFFFFFFFFu;
                    unsigned b1 = key[0] < key[1] ? key[0] : key[1];
                    unsigned b2 = key[0] < key[1] ? key[1] : key[0];
#pragma unroll
                    for (int d = 32; d > 0; d >>= 1) {
                        const unsigned o1 = (unsigned)__shfl_xor((int)b1, d, 64), o2 = (unsigned)__shfl_xor((int)b2, d, 64);
                        const unsigned hi1 = b1 > o1 ? b1 : o1, lo2 = b2 < o2 ? b2 : o2;
                        b1 = b1 < o1 ? b1 : o1;
                        b2 = hi1 < lo2 ? hi1 : lo2;
                    }
                    if (b1 == 0xFFFFFFFFu) continue;
                    const int bestDist1 = (int)(b1 >> 16), bestDist2 = b2 == 0xFFFFFFFFu ? 256 : (int)(b2 >> 16);
                    if (bestDist1 < SD_TH_LOW && (float)bestDist1 < nnratio * (float)bestDist2) {
                        const int pos = (int)(b1 & 0xFFFFu);
                        const unsigned i1t = (unsigned)__builtin_amdgcn_readlane((int)i1l, t);
                        const float a1t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ang1), t));
                        if ((pos & 63) == lane) {
                            const int q = pos >> 6;
                            const unsigned i2 = q ? i2l[1] : i2l[0];
                            if (q) freeF[1] = false; else freeF[0] = false;
                            s_match[i1t] = (int)i2;
                            int bin = 0;
                            if (checkOrientation) {
                                float rot = a1t - k2p[i2].angle;
                                if (rot < 0.0f) rot += 360.0f;
                                bin = (int)roundf(rot * factor);
                                if (bin == SD_HISTO) bin = 0;
                                atomicAdd(&s_hist[bin], 1);
                            }
                            s_bin[i1t] = (uint8_t)bin;
                        }
                        nm++;
                    }
                }
            }
        } else {
            // ---- the memory path: lanes over KF2's features of the node, the taken flags in LDS
            for (int a = a0; a < a1; a++) {
                const unsigned i1 = ff1[a];
                if (v1 && !v1[i1]) continue;
                const uint4* pk = (const uint4*)(d1 + (size_t)i1 * 32);
                const uint4 k0 = pk[0], k1 = pk[1];
                unsigned b1 = 0xFFFFFFFFu, b2 = 0xFFFFFFFFu;     // smallest and second smallest (distance << 16 | position in the node)
                for (int c = c0 + lane; c < c1; c += 64) {
                    const unsigned i2 = ff2[c];
                    if (s_taken[i2] || (v2 && !v2[i2])) continue;
                    const uint4* pf = (const uint4*)(d2 + (size_t)i2 * 32);
                    const unsigned key = ((unsigned)sd_hamming256(k0, k1, pf[0], pf[1]) << 16) | (unsigned)(c - c0);
                    if (key < b1) { b2 = b1; b1 = key; } else if (key < b2) b2 = key;
                }
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) {
                    const unsigned o1 = (unsigned)__shfl_xor((int)b1, d, 64), o2 = (unsigned)__shfl_xor((int)b2, d, 64);
                    const unsigned hi1 = b1 > o1 ? b1 : o1, lo2 = b2 < o2 ? b2 : o2;
                    b1 = b1 < o1 ? b1 : o1;
                    b2 = hi1 < lo2 ? hi1 : lo2;
                }
                if (b1 == 0xFFFFFFFFu) continue;                  // no free valid KF2 feature in this node
                const int bestDist1 = (int)(b1 >> 16), bestDist2 = b2 == 0xFFFFFFFFu ? 256 : (int)(b2 >> 16);
                if (bestDist1 < SD_TH_LOW && (float)bestDist1 < nnratio * (float)bestDist2) {
                    const unsigned i2 = ff2[c0 + (int)(b1 & 0xFFFFu)];
                    if (lane == 0) {
                        s_match[i1] = (int)i2;
                        s_taken[i2] = 1;
                        int bin = 0;
                        if (checkOrientation) {
                            float rot = k1p[i1].angle - k2p[i2].angle;
                            if (rot < 0.0f) rot += 360.0f;
                            bin = (int)roundf(rot * factor);
                            if (bin == SD_HISTO) bin = 0;
                            atomicAdd(&s_hist[bin], 1);
                        }
                        s_bin[i1] = (uint8_t)bin;
                    }
                    nm++;
                    __builtin_amdgcn_wave_barrier();
                }
                __threadfence_block();                            // s_taken written by lane 0 is read by every lane next round
            }
        }
    }
    if (lane == 0) atomicAdd(&s_nm, nm);
    __syncthreads();
    if (checkOrientation) {
        if (tid == 0) {
            int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;     // ComputeThreeMaxima (ORBmatcher.cc:1758-1799)
            for (int b = 0; b < SD_HISTO; b++) {
                const int s = s_hist[b];
                if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = b; }
                else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = b; }
                else if (s > max3) { max3 = s; ind3 = b; }
            }
            if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
            else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
            s_ind[0] = ind1; s_ind[1] = ind2; s_ind[2] = ind3;
        }
        __syncthreads();
        const int i1 = s_ind[0], i2 = s_ind[1], i3 = s_ind[2];
        int culled = 0;
        for (int i = tid; i < N1; i += 64 * SD_BOW_WAVES)
            if (s_match[i] >= 0) { const int b = s_bin[i]; if (b != i1 && b != i2 && b != i3) { s_match[i] = -1; culled++; } }
        if (culled) atomicSub(&s_nm, culled);
        __syncthreads();
    }
    for (int i = tid; i < cap; i += 64 * SD_BOW_WAVES) matchOut[(size_t)pair * cap + i] = i < N1 ? s_match[i] : -1;
    if (tid == 0) nmatchOut[pair] = s_nm;
}
