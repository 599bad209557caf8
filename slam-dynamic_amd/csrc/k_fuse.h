// LocalMapping::SearchInNeighbors as batched kernels (gfx950, wave64):
//   k_fuse_search    the per-candidate search of ORBmatcher::Fuse(pKF, vpMapPoints, th)     src/ORBmatcher.cc:982-1106
//   k_fuse_resolve   what the tail (:1108-1128) will meet at bestIdx, hits compacted         src/ORBmatcher.cc:1108-1128
//   k_distinctive    MapPoint::ComputeDistinctiveDescriptors                                 src/MapPoint.cc:242-307
// The search of one candidate reads nothing another candidate writes (GetFeaturesInArea, the key points and the descriptors of pKF do
// not change inside Fuse), so an entry is one wave.  The tail mutates the pointer graph and stays with the caller; k_fuse_resolve only
// says, per hit, what the feature held when the call started and who among the job's entries reached an empty feature first.
// The point's view, PredictScale, the GetFeaturesInArea window and its walk are the shared ones of k_area.h; k_fuse_search keeps Fuse's
// own gates, its chi-square test and the wave minimum.  Numerics: DESIGN.md Q31.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_area.h"
#include "k_match.h"
#include "k_bow.h"

struct SdFuseHit { int cand, idx, dist, action, other; };       // sd_fuse_hit

#define SD_FUSE_ERR_POINT 1      // an entry named a point outside [0, n_points)

// One wave per entry, grid.y = job.  best[e] = (bestIdx, bestDist), (-1, 256) when the point was rejected or no feature passed.
__global__ void __launch_bounds__(256) k_fuse_search(
    const sd_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc, const float* __restrict__ uRight,
    const unsigned short* __restrict__ sortedIdx, const unsigned short* __restrict__ cellStart, const SdMapPoint* __restrict__ mps,
    const uint8_t* __restrict__ mpDesc, int nPoints, const int* __restrict__ frameOf /*[n_jobs] image slot*/,
    const int* __restrict__ candOff /*[n_jobs+1]*/, const int* __restrict__ candPoint, const float* __restrict__ Tcw,
    int2* __restrict__ best, int* __restrict__ errFlag, SdLevelTables L, SdCamera cam, float th, int cap)
{
    __shared__ float s_scale[SD_MAX_LEVELS], s_invSigma2[SD_MAX_LEVELS];
    if (threadIdx.x < SD_MAX_LEVELS) { s_scale[threadIdx.x] = L.scale[threadIdx.x]; s_invSigma2[threadIdx.x] = L.invSigma2[threadIdx.x]; }
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
    if ((m < -1 || m >= nPoints) && lane == 0) atomicOr(errFlag, SD_FUSE_ERR_POINT);
    unsigned bestKey = 0xFFFFFFFFu;          // (distance << 16 | walk position): the minimum distance, the earlier visit on a tie
    int bestIdx = -1;
    if (ok) {
        const SdMapPoint mp = mps[m];
        float xc, yc, zc;
        sd_mat3_mul_add(T, mp.xw[0], mp.xw[1], mp.xw[2], xc, yc, zc);
        if (zc < 0.0f) ok = false;
        const float invz = 1.0f / zc;
        const float x = xc * invz, y = yc * invz;
        const float u = cam.fx * x + cam.cx;
        const float v = cam.fy * y + cam.cy;
        if (!(u >= cam.mnMinX && u < cam.mnMaxX && v >= cam.mnMinY && v < cam.mnMaxY)) ok = false;      // KeyFrame::IsInImage
        const float ur = u - cam.mbf * invz;
        float ox, oy, oz;
        sd_cam_centre(T, ox, oy, oz);
        const SdPointView w = sd_view_of_point(mp, ox, oy, oz);
        if (w.dist3D < 0.8f * mp.minDistance || w.dist3D > 1.2f * mp.maxDistance) ok = false;
        if (w.dot < 0.5 * (double)w.dist3D) ok = false;
        if (ok) {
            const int level = sd_predict_scale(mp.maxDistance, w.dist3D, s_scale[1], L.nlevels);
            const float radius = th * s_scale[level];
            const SdAreaWindow W = sd_area_window(cam, u, v, radius);
            if (!W.empty) {
                const uint4* dl = (const uint4*)(mpDesc + (size_t)m * 32);
                const uint4 l0 = dl[0], l1 = dl[1];
                const SdImageArrays C = sd_image_arrays(kp, nullptr, uRight, desc, sortedIdx, cellStart, frameOf[job], cap);
                const SdAreaWalk<64> walk(C, W, true, lane);
                for (int base = 0; base < walk.total; base += 64) {      // a window of more than 64 features takes several passes
                    const int tt = base + lane;
                    const int i2 = walk.member(tt);
                    if (i2 >= 0) {
                        const sd_keypoint k = C.kp[i2];
                        const float distx = k.x - u, disty = k.y - v;
                        if (fabsf(distx) < radius && fabsf(disty) < radius && k.octave >= level - 1 && k.octave <= level) {
                            const float kr = C.uRight[i2];
                            const float ex = u - k.x, ey = v - k.y;
                            const float inv = s_invSigma2[k.octave];
                            bool pass;
                            if (kr >= 0) {
                                const float er = ur - kr;
                                float e2 = ex * ex + ey * ey; e2 = e2 + er * er;
                                pass = !((double)(e2 * inv) > 7.8);
                            } else {
                                const float e2 = ex * ex + ey * ey;
                                pass = !((double)(e2 * inv) > 5.99);
                            }
                            if (pass) {
                                const uint4* dr = (const uint4*)(C.desc + (size_t)i2 * 32);
                                const int dist = sd_hamming256(l0, l1, dr[0], dr[1]);
                                const unsigned key = ((unsigned)dist << 16) | (unsigned)tt;
                                if (dist < 256 && key < bestKey) { bestKey = key; bestIdx = i2; }
                            }
                        }
                    }
                }
            }
        }
    }
    const unsigned w = sd_wave_min_u32(bestKey);
    int2 out = make_int2(-1, 256);
    if (w != 0xFFFFFFFFu) {
        const unsigned long long who = __ballot(bestKey == w);           // keys are unique: the walk position is in the low bits
        out.x = __shfl(bestIdx, __ffsll((long long)who) - 1, 64);
        out.y = (int)(w >> 16);
    }
    if (lane == 0) best[e] = out;
}

// One workgroup per job, entries in order.  first[] ([cap] ints: dynamic LDS when firstGlobal is NULL, else row `job` of firstGlobal)
// holds, per empty feature, the smallest position among the job's hits on it.
__global__ void __launch_bounds__(256) k_fuse_resolve(const int* __restrict__ count, const int* __restrict__ frameOf,
                                                      const int* __restrict__ candOff, const int2* __restrict__ best,
                                                      const uint8_t* __restrict__ kfState /*nullable [n_jobs][cap]*/, int cap,
                                                      int* __restrict__ firstGlobal, SdFuseHit* __restrict__ hits, int* __restrict__ nfused)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int s_scan[257];
    const int job = blockIdx.x, tid = threadIdx.x;
    int* first = firstGlobal ? firstGlobal + (size_t)job * cap : (int*)smem;
    const int e0 = candOff[job], M = candOff[job + 1] - e0;
    const int N = count[frameOf[job]];
    const uint8_t* st = kfState ? kfState + (size_t)job * cap : nullptr;
    for (int i = tid; i < N; i += 256) first[i] = 0x7FFFFFFF;
    __syncthreads();
    for (int p = tid; p < M; p += 256) {
        const int2 b = best[e0 + p];
        if (b.y <= SD_TH_LOW && b.x >= 0 && b.x < N && (st ? st[b.x] : 0) == 0) atomicMin(&first[b.x], p);
    }
    __syncthreads();
    int total = 0;
    for (int base = 0; base < M; base += 256) {
        const int p = base + tid;
        int2 b = make_int2(-1, 256);
        if (p < M) b = best[e0 + p];
        const bool hit = b.y <= SD_TH_LOW && b.x >= 0 && b.x < N;
        s_scan[tid] = hit ? 1 : 0;
        __syncthreads();
        sd_scan256(s_scan, tid);
        __syncthreads();
        if (hit) {
            const int state = st ? st[b.x] : 0;
            SdFuseHit h; h.cand = p; h.idx = b.x; h.dist = b.y; h.other = -1;
            if (state == 1) h.action = SD_FUSE_MEET_KF;
            else if (state != 0) h.action = SD_FUSE_MEET_BAD;
            else if (first[b.x] == p) h.action = SD_FUSE_ADD;
            else { h.action = SD_FUSE_MEET_CANDIDATE; h.other = first[b.x]; }
            hits[(size_t)e0 + total + s_scan[tid]] = h;
        }
        total += s_scan[256];
        __syncthreads();
    }
    if (tid == 0) nfused[job] = total;
}

// ---------------------------------------------------------------- MapPoint::ComputeDistinctiveDescriptors
// One wave per point.  The median of row i is the smallest v with #{j : d(i, j) <= v} > (int)(0.5 * (N - 1)): nine bisection steps over
// [0, 256], no sorted row is kept.  N <= 64: lane = row.  Larger N: the wave walks the rows, its lanes run over the columns.
__device__ __forceinline__ int sd_dist_desc(const uint8_t* __restrict__ a, const uint4 b0, const uint4 b1)
{
    const uint4* p = (const uint4*)a;
    return sd_hamming256(p[0], p[1], b0, b1);
}

__global__ void __launch_bounds__(256) k_distinctive(int nPoints, const int* __restrict__ obsOff, const uint8_t* __restrict__ obsDesc,
                                                     int* __restrict__ bestObs, uint8_t* __restrict__ descOut /*nullable*/)
{
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + wv;
    if (p >= nPoints) return;
    const int o0 = obsOff[p], N = obsOff[p + 1] - o0;
    if (N <= 0) { if (lane == 0) bestObs[p] = -1; return; }
    const uint8_t* D = obsDesc + (size_t)o0 * 32;
    const int k = (N - 1) >> 1;                        // (int)(0.5 * (N - 1))
    int bestRow = 0;
    if (N <= 64) {
        unsigned key = 0xFFFFFFFFu;
        if (lane < N) {
            const uint4* mine = (const uint4*)(D + (size_t)lane * 32);
            const uint4 a0 = mine[0], a1 = mine[1];
            int lo = 0, hi = 256;                       // the answer lies in [lo, hi]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                int c = 0;
                for (int j = 0; j < N; j++) c += sd_dist_desc(D + (size_t)j * 32, a0, a1) <= mid ? 1 : 0;
                if (c > k) hi = mid; else lo = mid + 1;
            }
            key = ((unsigned)lo << 16) | (unsigned)lane;
        }
        key = sd_wave_min_u32(key);
        bestRow = (int)(key & 0xFFFFu);                 // the first row with the strictly smallest median
    } else {
        int bestMedian = 0x7FFFFFFF;
        for (int i = 0; i < N; i++) {                   // wave-uniform
            const uint4* row = (const uint4*)(D + (size_t)i * 32);
            const uint4 a0 = row[0], a1 = row[1];
            int lo = 0, hi = 256;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                int c = 0;
                for (int j = lane; j < N; j += 64) c += sd_dist_desc(D + (size_t)j * 32, a0, a1) <= mid ? 1 : 0;
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
                if (c > k) hi = mid; else lo = mid + 1;
            }
            if (lo < bestMedian) { bestMedian = lo; bestRow = i; }
        }
    }
    if (lane == 0) bestObs[p] = bestRow;
    if (descOut && lane < 32) descOut[(size_t)p * 32 + lane] = D[(size_t)bestRow * 32 + lane];
}
