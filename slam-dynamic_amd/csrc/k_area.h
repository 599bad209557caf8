// What the projection matchers share (gfx950, wave64): a 3-D point seen from a pose, the window GetFeaturesInArea(u, v, r) opens
// over the sorted 64x48 grid, the walk over the window's members in the reference's visiting order, and the running best-64 of
// the keys a walk yields.  k_proj_candidates, k_local_candidates (k_frame.h) and k_fuse_search (k_fuse.h) are built from these; a
// new window matcher starts here.  Device inline helpers and PODs only: no kernel, no state.
// Everything here decides output bytes -- the visiting order, the one-ulp cell bounds, the f64 sums -- so the operation order of
// every helper is part of its contract (the library is built with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sd_plan.h"
#include "../../include/sd_frontend.h"

#define SD_GRID_COLS 64   // FRAME_GRID_COLS, Frame.h:40
#define SD_GRID_ROWS 48   // FRAME_GRID_ROWS, Frame.h:39
#define SD_GRID_CELLS (SD_GRID_COLS * SD_GRID_ROWS)
#define SD_PROJ_K 64      // candidates kept per projected point (one per lane)

struct SdCamera { float fx, fy, cx, cy, mbf, mb, mnMinX, mnMaxX, mnMinY, mnMaxY; };
struct SdMapPoint { float xw[3]; float normal[3]; float minDistance, maxDistance; unsigned flags; };     // sd_map_point

// mvScaleFactors / mvLevelSigma2 / mvInvLevelSigma2 for the kernels that take them by value; 1.f beyond nlevels (level_tables(), sd_api.hip)
struct SdLevelTables { float scale[SD_MAX_LEVELS], sigma2[SD_MAX_LEVELS], invSigma2[SD_MAX_LEVELS]; int nlevels; };

__device__ __forceinline__ int sd_hamming256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1)
{
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

__device__ __forceinline__ void sd_mat3_mul_add(const float* __restrict__ T /*row-major 4x4*/, float x, float y, float z,
                                                float& ox, float& oy, float& oz)
{
    // t = (a0*b0 + a1*b1) + a2*b2 ; d = t + c   (f32, left to right, no contraction)
    float s;
    s = T[0] * x + T[1] * y; s = s + T[2] * z; ox = s + T[3];
    s = T[4] * x + T[5] * y; s = s + T[6] * z; oy = s + T[7];
    s = T[8] * x + T[9] * y; s = s + T[10] * z; oz = s + T[11];
}

// Ow = -Rcw.t() * tcw of the row-major 4x4 pose T (Frame.cc:669-674, KeyFrame.cc:51-66; twc at ORBmatcher.cc:1498)
__device__ __forceinline__ void sd_cam_centre(const float* __restrict__ T, float& ox, float& oy, float& oz)
{
    float s;
    s = (-T[0]) * T[3] + (-T[4]) * T[7]; ox = s + (-T[8]) * T[11];
    s = (-T[1]) * T[3] + (-T[5]) * T[7]; oy = s + (-T[9]) * T[11];
    s = (-T[2]) * T[3] + (-T[6]) * T[7]; oz = s + (-T[10]) * T[11];
}

// PO = P - Ow, dist3D = cv::norm(PO) and PO.dot(Pn) through f64 sums (Frame.cc:707-716, ORBmatcher.cc:1031-1041).  What a caller
// compares the two with is its own reference statement: isInFrustum divides, Fuse multiplies.
struct SdPointView { float px, py, pz, dist3D; double dot; };
__device__ __forceinline__ SdPointView sd_view_of_point(const SdMapPoint& mp, float ox, float oy, float oz)
{
    SdPointView w;
    w.px = mp.xw[0] - ox; w.py = mp.xw[1] - oy; w.pz = mp.xw[2] - oz;
    double s2 = (double)w.px * (double)w.px; s2 += (double)w.py * (double)w.py; s2 += (double)w.pz * (double)w.pz;
    w.dist3D = (float)sqrt(s2);
    w.dot = (double)w.px * (double)mp.normal[0]; w.dot += (double)w.py * (double)mp.normal[1]; w.dot += (double)w.pz * (double)mp.normal[2];
    return w;
}

// std::log(float), taken correctly rounded (the oracle's logf_cr)
__device__ __forceinline__ float sd_logf_cr(float x) { return (float)log((double)x); }

// MapPoint::PredictScale (MapPoint.cc:385-414), scale1 = mvScaleFactors[1]
__device__ __forceinline__ int sd_predict_scale(float maxDistance, float dist, float scale1, int nlevels)
{
    const float ratio = maxDistance / dist;
    const float logScaleFactor = sd_logf_cr(scale1);
    int nScale = (int)ceilf(sd_logf_cr(ratio) / logScaleFactor);
    if (nScale < 0) nScale = 0; else if (nScale >= nlevels) nScale = nlevels - 1;
    return nScale;
}

// mfGridElementWidthInv / mfGridElementHeightInv (Frame.cc:110-111): the grid (k_grid_cells) and its readers take them from here
__device__ __forceinline__ void sd_grid_inv(const SdCamera& cam, float& wInv, float& hInv)
{
    wInv = (float)SD_GRID_COLS / (cam.mnMaxX - cam.mnMinX);
    hInv = (float)SD_GRID_ROWS / (cam.mnMaxY - cam.mnMinY);
}

// The cell bounds of Frame::GetFeaturesInArea (Frame.cc:735-754) / KeyFrame::GetFeaturesInArea (KeyFrame.cc:569-588);
// empty = one of the reference's early returns.
struct SdAreaWindow { int minX, maxX, minY, maxY; bool empty; };
__device__ __forceinline__ SdAreaWindow sd_area_window(const SdCamera& cam, float u, float v, float radius)
{
    float wInv, hInv;
    sd_grid_inv(cam, wInv, hInv);
    SdAreaWindow w;
    w.minX = max(0, (int)floorf((u - cam.mnMinX - radius) * wInv));
    w.maxX = min(SD_GRID_COLS - 1, (int)ceilf((u - cam.mnMinX + radius) * wInv));
    w.minY = max(0, (int)floorf((v - cam.mnMinY - radius) * hInv));
    w.maxY = min(SD_GRID_ROWS - 1, (int)ceilf((v - cam.mnMinY + radius) * hInv));
    w.empty = w.minX >= SD_GRID_COLS || w.maxX < 0 || w.minY >= SD_GRID_ROWS || w.maxY < 0;
    return w;
}

// The arrays of one image slot that a window search reads (cellOf may be NULL for a caller that never reads it).
struct SdImageArrays { const sd_keypoint* kp; const short* cellOf; const float* uRight; const uint8_t* desc; const unsigned short *sorted, *cellStart; };
__device__ __forceinline__ SdImageArrays sd_image_arrays(const sd_keypoint* kp, const short* cellOf, const float* uRight, const uint8_t* desc,
                                                         const unsigned short* sortedIdx, const unsigned short* cellStart, int img, int cap)
{
    const size_t o = (size_t)img * cap;
    return {kp + o, cellOf ? cellOf + o : nullptr, uRight + o, desc + o * 32, sortedIdx + o, cellStart + (size_t)img * (SD_GRID_CELLS + 8)};
}

// A group of GW lanes (16 or 64, gl = lane in the group) on one window.  GetFeaturesInArea visits cells ix-major / iy-minor
// (Frame.cc:758-785, KeyFrame.cc:590-605) and the cells (ix, minY..maxY) are one contiguous run of the sorted list: group lane
// j < nCols fetches the run of column minX + j, a group prefix sum turns the runs into one flat range [0, total) in visiting
// order, and member(t) maps a flat position back to a key point, so a kernel tests GW members per step:
//     for (int base = 0; __any(base < walk.total); base += GW) { const int i2 = walk.member(base + gl); if (i2 >= 0) ... }
// Every lane of the wave must construct the walk and call member() together (cross-lane shuffles); a group without a window
// passes live = false.  tooWide = the window spans more than GW columns: nothing is walked, the caller redoes it with GW = 64.
template <int GW>
struct SdAreaWalk {
    const unsigned short* sorted;
    int nCols, colsU, runS, excl, total;
    bool tooWide;
    __device__ __forceinline__ SdAreaWalk(const SdImageArrays& A, const SdAreaWindow& w, bool live, int gl) : sorted(A.sorted)
    {
        nCols = live ? w.maxX - w.minX + 1 : 0;
        tooWide = nCols > GW;
        if (tooWide) nCols = 0;
        int runN = 0; runS = 0;
        if (gl < nCols) {
            const int ix = w.minX + gl;
            runS = A.cellStart[ix * SD_GRID_ROWS + w.minY];
            runN = A.cellStart[ix * SD_GRID_ROWS + w.maxY + 1] - runS;
        }
        int incl = runN;
#pragma unroll
        for (int o = 1; o < GW; o <<= 1) { const int t = __shfl_up(incl, o, GW); if (gl >= o) incl += t; }
        total = __shfl(incl, GW - 1, GW);
        excl = incl - runN;
        colsU = nCols;                                             // the wave-uniform bound of member()'s column search
#pragma unroll
        for (int o = GW; o < 64; o <<= 1) colsU = max(colsU, __shfl_xor(colsU, o, 64));
        colsU = __builtin_amdgcn_readfirstlane(colsU);
    }
    // key-point index of flat position t, -1 beyond the window's last member
    __device__ __forceinline__ int member(int t) const
    {
        int col = 0;                                               // owner column: the last group lane whose exclusive prefix is <= t
        for (int j = 1; j < colsU; j++) { const int ej = __shfl(excl, j, GW); if (j < nCols && ej <= t) col = j; }
        const int cS = __shfl(runS, col, GW), cE = __shfl(excl, col, GW);
        return t < total ? (int)sorted[cS + (t - cE)] : -1;
    }
};

// wave-wide ascending bitonic sort of one 64-bit key per lane
// (n wave-uniform: keys occupy lanes 0 .. n-1, the others hold the maximum, so a network over the first 2^ceil(log2 n) lanes suffices;
// with lane = the lane in a group of 16 and n <= 16 every group of the wave sorts its own keys)
__device__ __forceinline__ unsigned long long sd_wave_sort64(unsigned long long key, int lane, int n = 64)
{
    int m = 2;
    while (m < n) m <<= 1;
    for (int k = 2; k <= m && n > 1; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, j, 64);
            const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), j, 64);
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            const bool takeMin = (((lane & k) == 0) == ((lane & j) == 0));
            key = takeMin ? (key < other ? key : other) : (key > other ? key : other);
        }
    return key;
}
// merge two ascending 64-key sequences held one per lane, keep the 64 smallest (ascending)
__device__ __forceinline__ unsigned long long sd_wave_merge_low64(unsigned long long a, unsigned long long b, int lane)
{
    const unsigned lo = (unsigned)__shfl((int)(unsigned)b, 63 - lane, 64);
    const unsigned hi = (unsigned)__shfl((int)(unsigned)(b >> 32), 63 - lane, 64);
    const unsigned long long br = ((unsigned long long)hi << 32) | lo;
    unsigned long long key = a < br ? a : br;                 // bitonic: the 64 smallest of both
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) {
        const unsigned l2 = (unsigned)__shfl_xor((int)(unsigned)key, j, 64);
        const unsigned h2 = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), j, 64);
        const unsigned long long other = ((unsigned long long)h2 << 32) | l2;
        key = ((lane & j) == 0) ? (key < other ? key : other) : (key > other ? key : other);
    }
    return key;
}

// The 64 smallest keys of a whole-wave walk: a window may hold more than 64 hits, and a truncated list must be the true head of the
// full one.  Hits wait compacted in an LDS row of 64 keys owned by the wave; when the next step's hits would not fit, and at the
// end, the row is sorted and merged into `best` (lane k = the k-th smallest key so far).  n counts every hit pushed.
// The row is written by some lanes and read back by others of the SAME wave, with no workgroup barrier.  The LDS executes one wave's
// DS instructions in issue order, so the hardware needs nothing; but the compiler reasons per lane, sees no dependence between
// lanes, and must keep every lane's write before the read and every next write after it: __builtin_amdgcn_wave_barrier() is that
// ordering point and emits no instruction.  The lgkmcnt(0) wait is not required by the in-order argument; it is kept because it
// costs a few cycles once per 64 hits on a rare path.
struct SdBest64 {
    unsigned long long best = ~0ull;
    int nbuf = 0, n = 0;
    __device__ __forceinline__ void drain(unsigned long long* __restrict__ row, int lane)
    {
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);                    // lgkmcnt(0): this wave's LDS writes are done
        unsigned long long kb = lane < nbuf ? row[lane] : ~0ull;
        kb = sd_wave_sort64(kb, lane, nbuf);
        best = sd_wave_merge_low64(best, kb, lane);
        nbuf = 0;
        __builtin_amdgcn_wave_barrier();
    }
    // all 64 lanes call it once per step; `hit` lanes contribute `key`
    __device__ __forceinline__ void push(unsigned long long* __restrict__ row, int lane, bool hit, unsigned long long key)
    {
        const unsigned long long m = __ballot(hit);
        const int h = __popcll(m);
        if (nbuf + h > SD_PROJ_K) drain(row, lane);
        if (hit) row[nbuf + __popcll(m & ((1ull << lane) - 1ull))] = key;
        nbuf += h; n += h;
    }
    // -> best: lane k holds the k-th smallest key of all pushed (~0ull beyond min(n, 64))
    __device__ __forceinline__ unsigned long long finish(unsigned long long* __restrict__ row, int lane) { drain(row, lane); return best; }
};
