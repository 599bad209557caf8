// The relocalisation matcher as batched kernels (gfx950, wave64):
//   k_reloc_search   the per-feature window of ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)
//                                                                                                   src/ORBmatcher.cc:1629-1711
//   k_reloc_assign   its sequential greedy `CurrentFrame.mvpMapPoints[bestIdx2] = pMP`, the rotation histogram and its culling
//                                                                                                   src/ORBmatcher.cc:1712-1755
// A job is (frame slot, keyframe slot, Tcw, th, ORBdist).  The keyframe's features are visited in order; each projects its map point
// into the frame and takes the nearest free frame feature of its window, and a feature taken by an earlier one is invisible to the
// later ones.  The scheme is the one of k_loop.h: k_reloc_search keeps, per keyframe feature, the SD_PROJ_K smallest (distance,
// visiting order) keys over the frame features that were free on entry, k_reloc_assign replays the features in order, 64 per round,
// and commits the lanes before the first conflict.  A feature whose SD_PROJ_K keys are all taken while its window held more sets
// SD_ERR_LOOP_LIST: the answer is refused (sd_batch_sync), never guessed.
// What differs from the Sim3 projection (k_loop.h), each a statement of the reference:
//   no `z > 0` test; invzc is a double division rounded to float; u = (fx * xc) * invzc + cx;
//   both image bounds and both distance bounds are inclusive; there is no viewing-angle test;
//   the window keeps octaves level - 1 .. level + 1 (Frame::GetFeaturesInArea with minLevel / maxLevel);
//   the acceptance is bestDist <= ORBdist, per job;
//   matches outside the three largest rotation bins become NULL after the loop, so they blocked later features during it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_area.h"
#include "k_match.h"
#include "k_loop.h"

#define SD_RELOC_ERR_POINT 1     // a d_kf_point or d_frame_point value outside [-1, n_points)
#define SD_RELOC_PENDING 255     // between the two kernels: the window held a member, the greedy decides

// The projection of ORBmatcher.cc:1654-1683 for one point: every `continue` before GetFeaturesInArea -> exit code, 0 = go on.
struct SdRelocView { int exit; float u, v, radius; int level; };
__device__ __forceinline__ SdRelocView sd_reloc_view(const SdMapPoint& mp, const float* __restrict__ T, const SdCamera& cam,
                                                     const float* s_scale, int nlevels, float th)
{
    SdRelocView w; w.exit = 0; w.level = 0; w.radius = 0.f;
    float xc, yc, zc;
    sd_mat3_mul_add(T, mp.xw[0], mp.xw[1], mp.xw[2], xc, yc, zc);
    const float invzc = (float)(1.0 / (double)zc);
    w.u = cam.fx * xc * invzc + cam.cx;
    w.v = cam.fy * yc * invzc + cam.cy;
    if (w.u < cam.mnMinX || w.u > cam.mnMaxX) { w.exit = SD_RELOC_OUT_U; return w; }
    if (w.v < cam.mnMinY || w.v > cam.mnMaxY) { w.exit = SD_RELOC_OUT_V; return w; }
    float ox, oy, oz;
    sd_cam_centre(T, ox, oy, oz);
    const SdPointView pv = sd_view_of_point(mp, ox, oy, oz);
    if (pv.dist3D < 0.8f * mp.minDistance) { w.exit = SD_RELOC_DIST_MIN; return w; }
    if (pv.dist3D > 1.2f * mp.maxDistance) { w.exit = SD_RELOC_DIST_MAX; return w; }
    // a NaN projection passes both image tests; GetFeaturesInArea then returns nothing
    if (w.u != w.u || w.v != w.v) { w.exit = SD_RELOC_WINDOW_EMPTY; return w; }
    w.level = sd_predict_scale(mp.maxDistance, pv.dist3D, s_scale[1], nlevels);
    w.radius = th * s_scale[w.level];
    return w;
}

// Which steps of the cascade (sd_batch_relocalize_refine, Tracking.cc:2311-2347) a job takes, as a function of what the earlier steps
// left in memory: nGood [3][nJobs] of the three optimisations, nAdd [2][nJobs] of the two searches.  Every kernel of the cascade asks
// for its own step, so no job needs the host between steps.  nGood == NULL: not a cascade, everything runs.
struct SdRelocPlan { const int* nGood; const int* nAdd; int nJobs; };
enum { SD_RELOC_STEP_ALWAYS = 0, SD_RELOC_STEP_SEARCH1, SD_RELOC_STEP_OPT2, SD_RELOC_STEP_SEARCH2, SD_RELOC_STEP_OPT3 };
__device__ __forceinline__ bool sd_reloc_runs(const SdRelocPlan& P, int job, int step)
{
    if (step == SD_RELOC_STEP_ALWAYS || !P.nGood) return true;
    const int ng1 = P.nGood[job];
    const bool s1 = ng1 >= 10 && ng1 < 50;                       // :2313 `continue`, :2321
    if (step == SD_RELOC_STEP_SEARCH1) return s1;
    const bool o2 = s1 && P.nAdd[job] + ng1 >= 50;               // :2325
    if (step == SD_RELOC_STEP_OPT2) return o2;
    const int ng2 = o2 ? P.nGood[P.nJobs + job] : 0;
    const bool s2 = o2 && ng2 > 30 && ng2 < 50;                  // :2331
    if (step == SD_RELOC_STEP_SEARCH2) return s2;
    return s2 && ng2 + P.nAdd[P.nJobs + job] >= 50;              // :2340
}

// One wave per keyframe feature, grid.y = job; rows are [job][cap].  found (nullable): per keyframe feature; mark (nullable,
// [job][nPoints]): per point id, the form the cascade derives sAlreadyFound in.  A job whose step does not run leaves at once.
// exitCode[e] = the `continue` the feature took, or SD_RELOC_PENDING; list[e][k] = (distance << 16 | frame feature) of the k-th smallest
// (distance, visiting order) key with distance < 256 over the members free on entry, listN[e] = how many such keys the window held.
__global__ void __launch_bounds__(256) k_reloc_search(
    const sd_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc, const float* __restrict__ uRight,
    const unsigned short* __restrict__ sortedIdx, const unsigned short* __restrict__ cellStart, const int* __restrict__ count,
    const SdMapPoint* __restrict__ mps, const uint8_t* __restrict__ mpDesc, int nPoints, const int2* __restrict__ slots,
    const float* __restrict__ Tcw, const float* __restrict__ thOf, const int* __restrict__ kfPoint, const int* __restrict__ framePoint,
    const uint8_t* __restrict__ found /*nullable*/, const uint8_t* __restrict__ mark /*nullable*/, unsigned* __restrict__ list,
    int* __restrict__ listN, int* __restrict__ exitCode, int* __restrict__ errFlag, SdLevelTables L, SdCamera cam, int cap, SdRelocPlan plan, int step)
{
    __shared__ float s_scale[SD_MAX_LEVELS];
    __shared__ unsigned long long s_row[4][SD_PROJ_K];
    if (threadIdx.x < SD_MAX_LEVELS) s_scale[threadIdx.x] = L.scale[threadIdx.x];
    __syncthreads();
    const int job = blockIdx.y;
    if (!sd_reloc_runs(plan, job, step)) return;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int fimg = slots[job].x, kimg = slots[job].y;
    const int N1 = min(count[kimg], cap), N2 = min(count[fimg], cap);
    const int* krow = kfPoint + (size_t)job * cap;
    const int* frow = framePoint + (size_t)job * cap;
    if (blockIdx.x == 0) {                                       // the first workgroup of a job checks the range of both rows
        bool outside = false;
        for (int i = threadIdx.x; i < N1; i += 256) { const int m = krow[i]; outside |= m < -1 || m >= nPoints; }
        for (int i = threadIdx.x; i < N2; i += 256) { const int m = frow[i]; outside |= m < -1 || m >= nPoints; }
        if (outside) atomicOr(errFlag, SD_RELOC_ERR_POINT);
    }
    const int el = blockIdx.x * 4 + wv;
    if (el >= N1) return;
    const size_t e = (size_t)job * cap + el;
    int m = krow[el];
    if (m < -1 || m >= nPoints) m = -1;                          // outside the table: read as -1
    int ex = 0;
    if (m < 0) ex = SD_RELOC_NULL;
    else if (!(mps[m].flags & 1u)) ex = SD_RELOC_BAD;
    else if ((found && found[e]) || (mark && mark[(size_t)job * nPoints + m])) ex = SD_RELOC_FOUND;
    else ex = -1;
    SdBest64 top;
    if (ex < 0) {
        const SdMapPoint mp = mps[m];
        const SdRelocView w = sd_reloc_view(mp, Tcw + (size_t)job * 16, cam, s_scale, L.nlevels, thOf[job]);
        ex = w.exit;
        if (ex == 0) {
            ex = SD_RELOC_WINDOW_EMPTY;
            const SdAreaWindow W = sd_area_window(cam, w.u, w.v, w.radius);
            if (!W.empty) {
                const uint4* dl = (const uint4*)(mpDesc + (size_t)m * 32);
                const uint4 l0 = dl[0], l1 = dl[1];
                const SdImageArrays C = sd_image_arrays(kp, nullptr, uRight, desc, sortedIdx, cellStart, fimg, cap);
                const SdAreaWalk<64> walk(C, W, true, lane);
                bool member = false;
                for (int base = 0; base < walk.total; base += 64) {      // a window of more than 64 features takes several passes
                    const int tt = base + lane;
                    const int i2 = walk.member(tt);
                    bool hit = false;
                    int dist = 256;
                    if (i2 >= 0) {
                        const sd_keypoint k = C.kp[i2];
                        const float distx = k.x - w.u, disty = k.y - w.v;
                        if (k.octave >= w.level - 1 && k.octave <= w.level + 1 && fabsf(distx) < w.radius && fabsf(disty) < w.radius) {
                            member = true;
                            const int held = frow[i2];
                            if (held == -1 || held < -1 || held >= nPoints) {      // outside the table: read as -1 (flagged by the row scan)
                                const uint4* dr = (const uint4*)(C.desc + (size_t)i2 * 32);
                                dist = sd_hamming256(l0, l1, dr[0], dr[1]);
                                hit = dist < 256;
                            }
                        }
                    }
                    top.push(s_row[wv], lane, hit, ((unsigned long long)(unsigned)dist << 32) | ((unsigned long long)(unsigned)tt << 16) | (unsigned)(i2 & 0xFFFF));
                }
                if (__any(member)) ex = SD_RELOC_PENDING;
            }
        }
    }
    if (ex == SD_RELOC_PENDING) {
        const unsigned long long key = top.finish(s_row[wv], lane);
        if (key != ~0ull) list[e * SD_PROJ_K + lane] = ((unsigned)(key >> 32) << 16) | (unsigned)(key & 0xFFFFu);
        if (lane == 0) listN[e] = top.n;
    }
    if (lane == 0) exitCode[e] = ex;
}

// One wave per job: the keyframe's features in order, 64 per chunk (see the head of k_loop.h).  taken = one bit per frame feature in
// dynamic LDS ((cap + 31) / 32 words).  Lane l owns the features p = l (mod 64) in the replay and in the culling pass, so what a
// lane reads back from memory it wrote itself.
// Outputs, rows [job][cap], every entry written: framePointOut = mvpMapPoints after the call, fromKf = the keyframe feature that
// supplied a new entry (-1 elsewhere), exitCode / best = per keyframe feature the exit and (bestIdx2, bestDist) at its turn;
// nmatch[job] = the return value.
__global__ void __launch_bounds__(64) k_reloc_assign(
    const sd_keypoint* __restrict__ kp, const int* __restrict__ count, const int2* __restrict__ slots, const int* __restrict__ orbOf,
    const unsigned* __restrict__ list, const int* __restrict__ listN, const int* __restrict__ kfPoint, const int* __restrict__ framePoint,
    int nPoints, int cap, int* exitCode, int* framePointOut, int* fromKf, int2* best, int* __restrict__ nmatch, int* __restrict__ capFlag,
    SdRelocPlan plan, int step)
{
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned* taken = (unsigned*)smem;
    __shared__ int s_hist[SD_HISTO];
    __shared__ SdRotKeep s_keep;
    const int job = blockIdx.x, lane = threadIdx.x;
    const int fimg = slots[job].x, kimg = slots[job].y;
    const int N1 = min(count[kimg], cap), N2 = min(count[fimg], cap);
    const int orb = orbOf[job];
    const size_t r0 = (size_t)job * cap;
    const int* krow = kfPoint + r0;
    const int* fin = framePoint + r0;
    int* frow = framePointOut + r0;
    int* arow = fromKf + r0;
    const sd_keypoint* kkp = kp + (size_t)kimg * cap;
    const sd_keypoint* fkp = kp + (size_t)fimg * cap;
    for (int i = lane; i < (cap + 31) / 32; i += 64) taken[i] = 0u;
    if (lane < SD_HISTO) s_hist[lane] = 0;
    for (int i = lane; i < cap; i += 64) {
        int held = i < N2 ? fin[i] : -1;
        if (held < -1 || held >= nPoints) held = -1;
        frow[i] = held; arow[i] = -1;
    }
    if (!sd_reloc_runs(plan, job, step)) {                       // the step does not run: mvpMapPoints passes through
        for (int p = lane; p < cap; p += 64) { exitCode[r0 + p] = 0; best[r0 + p] = make_int2(-1, 256); }
        if (lane == 0) nmatch[job] = 0;
        return;
    }
    __syncthreads();
    int nm = 0;
    for (int base = 0; base < N1; base += 64) {
        const int p = base + lane;
        const size_t e = r0 + p;
        bool done = p >= N1;
        if (!done && exitCode[e] != SD_RELOC_PENDING) { best[e] = make_int2(-1, 256); done = true; }
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
            const bool take = !done && pickIdx >= 0 && pickDist <= orb;
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
                if (take) {
                    atomicOr(&taken[pickIdx >> 5], 1u << (pickIdx & 31));
                    int m = krow[p];
                    frow[pickIdx] = m; arow[pickIdx] = p; nm++;
                    atomicAdd(&s_hist[sd_rot_bin(kkp[p].angle, fkp[pickIdx].angle)], 1);
                }
                if (pickIdx < 0 && total > SD_PROJ_K) atomicOr(capFlag, SD_ERR_LOOP_LIST);     // every kept key taken, the window held more
                exitCode[e] = take ? SD_RELOC_MATCHED : (pickIdx < 0 ? SD_RELOC_NO_FREE : SD_RELOC_ABOVE_DIST);
                best[e] = make_int2(pickIdx, pickDist);
                done = true;
            }
            __syncthreads();                                           // one wave: orders the LDS bits before the next round's reads
        }
    }
    __syncthreads();
    if (lane == 0) s_keep = sd_three_maxima(s_hist);
    __syncthreads();
    const SdRotKeep keep = s_keep;
    for (int p = lane; p < cap; p += 64) {
        const size_t e = r0 + p;
        if (p >= N1) { exitCode[e] = SD_RELOC_NULL; best[e] = make_int2(-1, 256); continue; }
        if (exitCode[e] != SD_RELOC_MATCHED) continue;
        const int idx = best[e].x;
        if (!keep.keeps(sd_rot_bin(kkp[p].angle, fkp[idx].angle))) { frow[idx] = -1; arow[idx] = -1; exitCode[e] = SD_RELOC_CULLED; nm--; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) nm += __shfl_xor(nm, d, 64);
    if (lane == 0) nmatch[job] = nm;
}

// ---------------------------------------------------------------- the cascade of Tracking::Relocalization (Tracking.cc:2292-2358)
// Rows are [job][cap]; one 256-thread workgroup per job in every kernel below.

// Entry: P0 = the job's mvpMapPoints (values outside the table read as -1, rows beyond the frame's count -1), mvbOutlier = false,
// sFound as marks over point ids (the caller cleared `mark`), and the range check of both index rows.
__global__ void __launch_bounds__(256) k_reloc_begin(const int* __restrict__ count, const int2* __restrict__ slots, const int* __restrict__ kfPoint,
                                                     const int* __restrict__ framePoint, int nPoints, int cap, int* __restrict__ P0,
                                                     uint8_t* __restrict__ outlier, uint8_t* __restrict__ mark, int* __restrict__ errFlag)
{
    const int job = blockIdx.x;
    const int N2 = min(count[slots[job].x], cap), N1 = min(count[slots[job].y], cap);
    const size_t r0 = (size_t)job * cap;
    bool outside = false;
    for (int i = threadIdx.x; i < cap; i += 256) {
        int m = i < N2 ? framePoint[r0 + i] : -1;
        if (m < -1 || m >= nPoints) { outside = true; m = -1; }
        P0[r0 + i] = m; outlier[r0 + i] = 0;
        if (m >= 0) mark[(size_t)job * nPoints + m] = 1;
        if (i < N1) { const int k = kfPoint[r0 + i]; outside |= k < -1 || k >= nPoints; }
    }
    if (outside) atomicOr(errFlag, SD_RELOC_ERR_POINT);
}

// sFound rebuilt from every non-NULL entry (Tracking.cc:2333-2336); the caller cleared `mark`
__global__ void __launch_bounds__(256) k_reloc_mark(const int* __restrict__ P, int nPoints, int cap, uint8_t* __restrict__ mark, SdRelocPlan plan, int step)
{
    const int job = blockIdx.x;
    if (!sd_reloc_runs(plan, job, step)) return;
    for (int i = threadIdx.x; i < cap; i += 256) { const int m = P[(size_t)job * cap + i]; if (m >= 0) mark[(size_t)job * nPoints + m] = 1; }
}

// The edges of PoseOptimization(&mCurrentFrame) from the job's assignment: key points of the frame slot in index order, an edge for every
// i with P[i] >= 0, compacted by a ballot prefix as k_pose_edges does.  Job `job` owns edges [job * cap, job * cap + n); a job whose step
// does not run gets an empty range, which k_pose_optimize answers with 0 and an untouched pose.  The pose of the step starts as the
// pose of the step before.
struct SdRelocEdgeArgs {
    const sd_keypoint* kp; const float* uRight; const int* count; const int2* slots; const SdMapPoint* mps; const int* P;
    const float* Tprev; float* Tcur; sd_pose_edge* edges; int* first; int* last;
    float invSigma2[SD_MAX_LEVELS]; int cap;
};
__global__ void __launch_bounds__(256) k_reloc_edges(SdRelocEdgeArgs A, SdRelocPlan plan, int step)
{
    __shared__ int wsum[4];
    const int job = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = A.cap;
    if (tid < 16) A.Tcur[(size_t)job * 16 + tid] = A.Tprev[(size_t)job * 16 + tid];
    const size_t e0 = (size_t)job * cap;
    if (!sd_reloc_runs(plan, job, step)) {
        if (tid == 0) { A.first[job] = (int)e0; A.last[job] = (int)e0; }
        return;
    }
    const int fimg = A.slots[job].x;
    const int N = min(A.count[fimg], cap);
    const int* __restrict__ m = A.P + e0;
    const size_t cur = (size_t)fimg * cap;
    int base = 0;
    for (int c = 0; c < N; c += 256) {
        const int i = c + tid;
        const int mi = i < N ? m[i] : -1;
        const bool pred = mi >= 0;
        const unsigned long long bal = __ballot(pred);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) { if (w < wave) off += wsum[w]; tot += wsum[w]; }
        if (pred) {
            const sd_keypoint kp = A.kp[cur + i];
            float w = 0.f;
#pragma unroll
            for (int l = 0; l < SD_MAX_LEVELS; l++) if (kp.octave == l) w = A.invSigma2[l];
            const SdMapPoint mp = A.mps[mi];
            sd_pose_edge e;
            e.xw[0] = mp.xw[0]; e.xw[1] = mp.xw[1]; e.xw[2] = mp.xw[2];
            e.u = kp.x; e.v = kp.y; e.ur = A.uRight[cur + i]; e.inv_sigma2 = w; e.kp_index = i;
            A.edges[e0 + off + pre] = e;
        }
        __syncthreads();
        base += tot;
    }
    if (tid == 0) { A.first[job] = (int)e0; A.last[job] = (int)e0 + base; }
}

// After an optimisation: mvbOutlier of the key points that had an edge, and (Pout != NULL) the assignment that follows it: a copy of
// Pin, with the outliers set to NULL when `discard` applies -- after the first optimisation only if nGood >= 10 (the `continue` of
// :2313 comes first), after the third always, after the second never (Pout == NULL).
__global__ void __launch_bounds__(256) k_reloc_after(const sd_pose_edge* __restrict__ edges, const int* __restrict__ first, const int* __restrict__ last,
                                                     const uint8_t* __restrict__ edgeOut, const int* __restrict__ nGoodStep, const int* __restrict__ Pin,
                                                     int* __restrict__ Pout, uint8_t* __restrict__ outlier, int cap, int minGood, SdRelocPlan plan, int step)
{
    const int job = blockIdx.x;
    const size_t r0 = (size_t)job * cap;
    if (Pout) for (int i = threadIdx.x; i < cap; i += 256) Pout[r0 + i] = Pin[r0 + i];
    if (!sd_reloc_runs(plan, job, step)) return;
    __syncthreads();
    const bool discard = Pout && nGoodStep[job] >= minGood;
    for (int e = first[job] + threadIdx.x; e < last[job]; e += 256) {
        const int i = edges[e].kp_index;
        const uint8_t o = edgeOut[e];
        outlier[r0 + i] = o;
        if (discard && o) Pout[r0 + i] = -1;
    }
}

// sd_reloc_result of every job from what the steps left
__global__ void __launch_bounds__(256) k_reloc_finish(const float* __restrict__ T /*[4][nJobs][16]*/, sd_reloc_result* __restrict__ res, SdRelocPlan plan)
{
    const int job = blockIdx.x * 256 + threadIdx.x;
    if (job >= plan.nJobs) return;
    const bool s1 = sd_reloc_runs(plan, job, SD_RELOC_STEP_SEARCH1), o2 = sd_reloc_runs(plan, job, SD_RELOC_STEP_OPT2);
    const bool s2 = sd_reloc_runs(plan, job, SD_RELOC_STEP_SEARCH2), o3 = sd_reloc_runs(plan, job, SD_RELOC_STEP_OPT3);
    sd_reloc_result r;
    r.stage_reached = 1 + (s1 ? 1 : 0) + (o2 ? 1 : 0) + (s2 ? 1 : 0) + (o3 ? 1 : 0);
    r.n_good[0] = plan.nGood[job];
    r.n_good[1] = o2 ? plan.nGood[plan.nJobs + job] : -1;
    r.n_good[2] = o3 ? plan.nGood[2 * plan.nJobs + job] : -1;
    r.n_additional[0] = s1 ? plan.nAdd[job] : -1;
    r.n_additional[1] = s2 ? plan.nAdd[plan.nJobs + job] : -1;
    const int nGood = o3 ? r.n_good[2] : (o2 ? r.n_good[1] : r.n_good[0]);
    r.matched = nGood >= 50 ? 1 : 0;                             // :2354
    for (int k = 0; k < 3; k++)
        for (int q = 0; q < 16; q++) r.Tcw_stage[k][q] = T[((size_t)(k + 1) * plan.nJobs + job) * 16 + q];
    for (int q = 0; q < 16; q++) r.Tcw[q] = r.Tcw_stage[2][q];
    res[job] = r;
}
