// Small kernels of the frame-level boundary (sd_tracker, sd_tracker.inc): everything here is per-lane bookkeeping that must
// not cost a host round trip -- the heavy work is in k_extract.h / k_fast.h / k_frame.h / k_motion.h / k_cull.h.
//   k_copy_frames     every mover of frame slots: Frame's copy constructor (src/Frame.cc:39-63) for a list of (src, dst) slots, the pool
//                     and initialisation-extractor copies between workspaces, prefetched frames <-> fixed-stride records
//   k_lane_gate       `if(!mCurrentFrame.objects.empty() && ...)` (src/Tracking.cc:622) evaluated on the device
//   k_reset_boxes     the constructors without boxes: objects.clear(), N_d = 0
//   k_fill_mono       `mvuRight = vector<float>(N,-1); mvDepth = vector<float>(N,-1);` (src/Frame.cc:432-434)
//   k_lane_summary    what the host needs of a frame after a step, packed for ONE device-to-host copy
#pragma once
#include "k_cull.h"
#include "k_motion.h"

// One segment per per-slot array of a frame (frame_arrays in sd_api.hip): slot k of a side lies at base + k * stride.  A record side is the
// same thing with base = records + the segment's offset and stride = the record stride.  Passed by value: 24 * (8 + 8 + 4 + 4 + 4) + 4 bytes,
// 680 with padding.
#define SD_COPY_SEGS 24
struct SdCopyTable {
    const char* src[SD_COPY_SEGS]; char* dst[SD_COPY_SEGS];
    unsigned srcStride[SD_COPY_SEGS], dstStride[SD_COPY_SEGS], bytes[SD_COPY_SEGS];
    int n;
};

// grid (blocks, segments, copies): copy z moves slot sd.x of the source side to slot sd.y of the destination side, (sd.x, sd.y) = pairs[z]
// or, without a list, (srcFirst + z * srcStep, dstFirst + z * dstStep).  A slot copied onto itself is skipped.
__global__ void __launch_bounds__(256) k_copy_frames(SdCopyTable T, const int2* __restrict__ pairs, int srcFirst, int srcStep, int dstFirst, int dstStep)
{
    const int seg = blockIdx.y, z = blockIdx.z;
    const int2 sd = pairs ? pairs[z] : make_int2(srcFirst + z * srcStep, dstFirst + z * dstStep);
    const unsigned n = T.bytes[seg];
    const char* s = T.src[seg] + (size_t)sd.x * T.srcStride[seg];
    char* d = T.dst[seg] + (size_t)sd.y * T.dstStride[seg];
    if (s == d) return;
    const bool a16 = ((((size_t)s) | ((size_t)d)) & 15) == 0;
    const unsigned quads = a16 ? n >> 4 : 0;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < quads; i += gridDim.x * 256) ((uint4*)d)[i] = ((const uint4*)s)[i];
    for (unsigned i = (quads << 4) + blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) d[i] = s[i];
}

__global__ void k_lane_gate(const SdFrameBoxes* __restrict__ fb, const int* __restrict__ want, int* __restrict__ active, int n, int slotStep)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s < n) active[s] = (want[s] && fb[s * slotStep].nb > 0) ? 1 : 0;
}

__global__ void k_reset_boxes(SdFrameBoxes* __restrict__ fb, const int* __restrict__ count, const int* __restrict__ slots, int n)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int slot = slots[i];
    SdFrameBoxes& F = fb[slot];
    F.nb = 0; F.nAll = count[slot]; F.nOri = count[slot]; F.nDyn = 0; F.boxStart[0] = 0;
}

__global__ void __launch_bounds__(256) k_fill_mono(const int* __restrict__ count, float* __restrict__ uRight, float* __restrict__ depth, int cap)
{
    const int img = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count[img]) return;
    uRight[(size_t)img * cap + i] = -1.f; depth[(size_t)img * cap + i] = -1.f;
}

struct SdLaneSummary {
    int N, nb, nAll, nOri, nDyn;
    int flag, nH, nF, sepRet, nTrackMatches, nTrackPairs, nLastMatches;
    int box_idx[SD_MAXB], box_status[SD_MAXB], keptOrig[SD_MAXB];
    double boxes[SD_MAXB][4];
};
// TrackWithMotionModel's tail (sd_tracker_set_pose_optimization), written by k_pose_lane_summary.  The tracker keeps these behind its
// lane summaries in the same buffer, so the step's one results copy simply grows by them when the tail ran.
struct SdPoseSummary {
    float Tcw[16];
    int ran, nMatches, nInitial, nGood, nMap, ok;
};

__global__ void __launch_bounds__(64) k_lane_summary(const SdFrameBoxes* __restrict__ fb, const int* __restrict__ count,
                                                     const SdMotionResult* __restrict__ moRes, const int* __restrict__ sepRet,
                                                     const int* __restrict__ nmatch, const int* __restrict__ npairs, int nLanes, int slotStep,
                                                     int haveLast, SdLaneSummary* __restrict__ out)
{
    const int s = blockIdx.x, tid = threadIdx.x;
    const int slot = s * slotStep;
    const SdFrameBoxes& F = fb[slot];
    SdLaneSummary& O = out[s];
    if (tid < SD_MAXB) {
        const bool in = tid < F.nb;
        O.box_idx[tid] = in ? F.box_idx[tid] : 0; O.box_status[tid] = in ? F.box_status[tid] : 0; O.keptOrig[tid] = in ? F.keptOrig[tid] : 0;
        for (int k = 0; k < 4; k++) O.boxes[tid][k] = in ? F.boxes[tid][k] : 0.0;
    }
    if (tid == 0) {
        O.N = count[slot]; O.nb = F.nb; O.nAll = F.nAll; O.nOri = F.nOri; O.nDyn = F.nDyn;
        O.flag = moRes ? moRes[s].flag : 0; O.nH = moRes ? moRes[s].nH : 0; O.nF = moRes ? moRes[s].nF : 0;
        O.sepRet = sepRet[s]; O.nTrackMatches = nmatch[s]; O.nTrackPairs = npairs[s];
        O.nLastMatches = haveLast ? nmatch[nLanes + s] : -1;
    }
}

// TrackWithMotionModel after PoseOptimization (src/Tracking.cc:1762-1789) for lane s = pair nLanes + s: nmatchesMap counts the
// non-outlier matches whose mLastFrame point has Observations() > 0 (flag bit1 of the Last slot's map-point table).
__global__ void __launch_bounds__(256) k_pose_lane_summary(const sd_pose_edge* __restrict__ edges, const int* __restrict__ first,
                                                           const int* __restrict__ last, const float* __restrict__ Tcw,
                                                           const uint8_t* __restrict__ outlier, const int* __restrict__ good,
                                                           const int* __restrict__ ran, const int* __restrict__ match,
                                                           const uint8_t* __restrict__ flags, const int2* __restrict__ pairIdx,
                                                           const int* __restrict__ nmatch, const int* __restrict__ active, int nLanes,
                                                           int cap, SdPoseSummary* __restrict__ out)
{
    __shared__ int nMap;
    const int s = blockIdx.x, pair = nLanes + s, tid = threadIdx.x;
    if (tid == 0) nMap = 0;
    __syncthreads();
    const int e0 = first[pair], e1 = last[pair];
    const size_t lst = (size_t)pairIdx[pair].y * cap;
    int c = 0;
    for (int i = e0 + tid; i < e1; i += 256)
        if (!outlier[i]) c += (flags[lst + match[(size_t)pair * cap + edges[i].kp_index]] & 2) ? 1 : 0;
    if (c) atomicAdd(&nMap, c);
    __syncthreads();
    SdPoseSummary& O = out[s];
    if (tid < 16) O.Tcw[tid] = Tcw[(size_t)pair * 16 + tid];
    if (tid == 0) {
        const int r = ran[pair], n = e1 - e0;
        O.ran = r; O.nMatches = active[s] ? nmatch[pair] : -1; O.nInitial = n; O.nGood = n < 3 ? 0 : good[pair];
        O.nMap = nMap; O.ok = r && nMap >= 10;
    }
}
