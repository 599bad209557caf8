// What the descriptor matchers share (gfx950, wave64), each rule written once: ORBmatcher's thresholds, the rotation bin and
// ComputeThreeMaxima, the wave-wide minimum and top two of packed keys, the pairing of two FeatureVectors node by node, and the body
// of SearchByBoW.  k_proj_resolve (k_frame.h), k_search_by_bow (k_bow.h), k_search_by_bow_kf (k_loop.h), k_tri_match
// (k_triangulate.h) and k_reloc_assign (k_reloc.h) are built from these; a new descriptor matcher starts here.
// Everything here decides output bytes, so the comparisons and the operation order of every helper are part of its contract.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_area.h"

#define SD_TH_HIGH 100    // ORBmatcher.cc:37
#define SD_TH_LOW 50      // ORBmatcher.cc:38
#define SD_HISTO 30       // HISTO_LENGTH, ORBmatcher.cc:39

// ---------------------------------------------------------------- the rotation check
// rot = a1 - a2 -> rotation bin (ORBmatcher.cc:1719-1724, the same statement in every matcher).  Key-point angles lie in [0, 360), which
// gives a bin in 0..12; for anything else the reference asserts, and the bin is filed in bin 0 (the relocalisation section).
__device__ __forceinline__ int sd_rot_bin(float a1, float a2)
{
    float rot = a1 - a2;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / SD_HISTO));
    if (bin == SD_HISTO) bin = 0;
    return (unsigned)bin < (unsigned)SD_HISTO ? bin : 0;
}

// ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1758-1799) over the SD_HISTO bin sizes: the bins a match must lie in to survive.
struct SdRotKeep {
    int ind1, ind2, ind3;
    __device__ __forceinline__ bool keeps(int bin) const { return bin == ind1 || bin == ind2 || bin == ind3; }
};
__device__ __forceinline__ SdRotKeep sd_three_maxima(const int* hist)
{
    int max1 = 0, max2 = 0, max3 = 0;
    SdRotKeep k; k.ind1 = -1; k.ind2 = -1; k.ind3 = -1;
    for (int b = 0; b < SD_HISTO; b++) {
        const int s = hist[b];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; k.ind3 = k.ind2; k.ind2 = k.ind1; k.ind1 = b; }
        else if (s > max2) { max3 = max2; max2 = s; k.ind3 = k.ind2; k.ind2 = b; }
        else if (s > max3) { max3 = s; k.ind3 = b; }
    }
    if (max2 < 0.1f * (float)max1) { k.ind2 = -1; k.ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { k.ind3 = -1; }
    return k;
}

// ---------------------------------------------------------------- wave-wide reductions of packed keys
// A key is (distance << 16 | position): the minimum is the nearest, the earlier position on a tie; 0xFFFFFFFF = no candidate.
__device__ __forceinline__ unsigned sd_wave_min_u32(unsigned k)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const unsigned o = (unsigned)__shfl_xor((int)k, d, 64); k = o < k ? o : k; }
    return k;
}

// One butterfly for the smallest and the second smallest key of the wave.  In: every lane's own smallest (b1) and second smallest
// (b2); out: the wave's, in every lane.  Keys are unique (the position is in the low bits) apart from 0xFFFFFFFF.
__device__ __forceinline__ void sd_wave_top2_u32(unsigned& b1, unsigned& b2)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned o1 = (unsigned)__shfl_xor((int)b1, d, 64), o2 = (unsigned)__shfl_xor((int)b2, d, 64);
        const unsigned hi1 = b1 > o1 ? b1 : o1, lo2 = b2 < o2 ? b2 : o2;
        b1 = b1 < o1 ? b1 : o1;
        b2 = hi1 < lo2 ? hi1 : lo2;
    }
}

// ---------------------------------------------------------------- two FeatureVectors, node by node
// One image's FeatureVector as k_bow_finalize leaves it: `runs` vocabulary nodes ascending, run r = positions
// [runStart[r], runStart[r + 1]) of `feat` (feature indices ascending inside a run), and the image's descriptors and key points.
struct SdFvView {
    int runs;
    const int* runStart; const unsigned* runNode; const unsigned* feat;
    const uint8_t* desc; const sd_keypoint* kp;
};
__device__ __forceinline__ SdFvView sd_fv_view(const sd_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc,
                                               const unsigned* __restrict__ fvFeat, const int* __restrict__ fvRunStart,
                                               const unsigned* __restrict__ fvRunNode, const int* __restrict__ meta, int img, int cap)
{
    SdFvView V;
    V.runs = meta[img * 4 + 1];
    V.runStart = fvRunStart + (size_t)img * (cap + 1);
    V.runNode = fvRunNode + (size_t)img * cap;
    V.feat = fvFeat + (size_t)img * cap;
    V.desc = desc + (size_t)img * cap * 32;
    V.kp = kp + (size_t)img * cap;
    return V;
}

#define SD_BOW_REGF 128          // side-2 features of a node that a wave holds in registers (two per lane); larger nodes stream from memory
// Run r1 of side 1 and the run of the same node on side 2 (lower_bound in its runs): positions [a0, a1) of A.feat, [c0, c1) of B.feat.
struct SdNodePair { bool found; int a0, a1, c0, c1; };
__device__ __forceinline__ SdNodePair sd_fv_pair(const SdFvView& A, int r1, const SdFvView& B)
{
    SdNodePair n; n.found = false; n.a0 = n.a1 = n.c0 = n.c1 = 0;
    const unsigned node = A.runNode[r1];
    int lo = 0, hi = B.runs;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (B.runNode[mid] < node) lo = mid + 1; else hi = mid; }
    if (lo >= B.runs || B.runNode[lo] != node) return n;
    n.found = true;
    n.a0 = A.runStart[r1]; n.a1 = A.runStart[r1 + 1]; n.c0 = B.runStart[lo]; n.c1 = B.runStart[lo + 1];
    return n;
}

// ---------------------------------------------------------------- ORBmatcher::SearchByBoW
// One workgroup per pair of images; a wave takes a vocabulary node both FeatureVectors share.  A side-2 feature belongs to exactly one
// node, so waves never contend for one; inside a node the side-1 features are walked in order (the order that decides which side-2
// features are already taken, ORBmatcher.cc:206-207).  Best / second best over the not-yet-taken side-2 features = first and second
// entry of the (distance, position) order (see k_local_resolve).
// The two callers differ in four statements of the reference:
//   BY_IDX1   the result is match[idx1] = idx2 (KeyFrame-KeyFrame, :679-812), not match[idx2] = idx1 (KeyFrame-Frame, :159-288).  The
//             memory path then keeps its taken flags in `taken`; otherwise match[idx2] >= 0 is the flag;
//   STRICT    the acceptance is bestDist1 < TH_LOW, not <=;
//   valid2    side 2 has a validity mask too (NULL: none).
#define SD_BOW_WAVES 16
struct SdBowLds { int* match; uint8_t* bin; uint8_t* taken; int* hist; };      // [cap] by result index, [cap] by idx2 (BY_IDX1), [SD_HISTO]

template <bool STRICT>
__device__ __forceinline__ bool sd_bow_accepts(unsigned b1, unsigned b2, float nnratio)
{
    const int bestDist1 = (int)(b1 >> 16), bestDist2 = b2 == 0xFFFFFFFFu ? 256 : (int)(b2 >> 16);
    return (STRICT ? bestDist1 < SD_TH_LOW : bestDist1 <= SD_TH_LOW) && (float)bestDist1 < nnratio * (float)bestDist2;
}

// by one lane: the match, its rotation bin and the histogram
template <bool BY_IDX1>
__device__ __forceinline__ void sd_bow_commit(const SdBowLds& S, unsigned i1, unsigned i2, float ang1, float ang2, int checkOrientation)
{
    const unsigned r = BY_IDX1 ? i1 : i2;
    S.match[r] = (int)(BY_IDX1 ? i2 : i1);
    int bin = 0;
    if (checkOrientation) { bin = sd_rot_bin(ang1, ang2); atomicAdd(&S.hist[bin], 1); }
    S.bin[r] = (uint8_t)bin;
}

// A node with up to SD_BOW_REGF side-2 features (the usual case: ~20 x 20 features at level L - 4): the wave keeps the node's side-2
// descriptors in registers (lane l owns positions l and l + 64, and with them their taken flags), gathers the side-1 descriptors 64 at
// a time and broadcasts one per step by readlane: no memory access inside the serial loop.  Returns the matches made.
template <bool BY_IDX1, bool STRICT>
__device__ __forceinline__ int sd_bow_node_regs(const SdFvView& A, const SdFvView& B, const SdNodePair& n, const uint8_t* v1, const uint8_t* v2,
                                                const SdBowLds& S, float nnratio, int checkOrientation, int lane)
{
    int nm = 0;
    unsigned i2l[2]; uint4 f0[2], f1[2]; bool freeF[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int c = n.c0 + lane + 64 * q;
        freeF[q] = c < n.c1;
        i2l[q] = freeF[q] ? B.feat[c] : 0u;
        if (freeF[q] && v2 && !v2[i2l[q]]) freeF[q] = false;
        const uint4* pf = (const uint4*)(B.desc + (size_t)i2l[q] * 32);
        f0[q] = pf[0]; f1[q] = pf[1];
    }
    for (int kb = n.a0; kb < n.a1; kb += 64) {
        const int a = kb + lane;
        const unsigned i1l = a < n.a1 ? A.feat[a] : 0u;
        const int ok1 = a < n.a1 && (!v1 || v1[i1l]);
        const uint4* pk = (const uint4*)(A.desc + (size_t)i1l * 32);
        const uint4 kl0 = pk[0], kl1 = pk[1];
        const float ang1 = A.kp[i1l].angle;
        const int nstep = n.a1 - kb < 64 ? n.a1 - kb : 64;
        for (int t = 0; t < nstep; t++) {
            if (!__builtin_amdgcn_readlane(ok1, t)) continue;
            uint4 k0, k1;                                  // t is wave-uniform: v_readlane, no LDS crossbar
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
            sd_wave_top2_u32(b1, b2);
            if (b1 == 0xFFFFFFFFu) continue;
            if (sd_bow_accepts<STRICT>(b1, b2, nnratio)) {
                const int pos = (int)(b1 & 0xFFFFu);
                const unsigned i1t = (unsigned)__builtin_amdgcn_readlane((int)i1l, t);
                const float a1t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ang1), t));
                if ((pos & 63) == lane) {                  // the owning lane commits
                    const int q = pos >> 6;
                    const unsigned i2 = q ? i2l[1] : i2l[0];
                    if (q) freeF[1] = false; else freeF[0] = false;
                    sd_bow_commit<BY_IDX1>(S, i1t, i2, a1t, B.kp[i2].angle, checkOrientation);
                }
                nm++;
            }
        }
    }
    return nm;
}

// A node with more side-2 features than the registers hold: lanes over side 2's features of the node, from memory, a running top two
// per lane; the taken flags in LDS.
template <bool BY_IDX1, bool STRICT>
__device__ __forceinline__ int sd_bow_node_mem(const SdFvView& A, const SdFvView& B, const SdNodePair& n, const uint8_t* v1, const uint8_t* v2,
                                               const SdBowLds& S, float nnratio, int checkOrientation, int lane)
{
    int nm = 0;
    for (int a = n.a0; a < n.a1; a++) {
        const unsigned i1 = A.feat[a];
        if (v1 && !v1[i1]) continue;
        const uint4* pk = (const uint4*)(A.desc + (size_t)i1 * 32);
        const uint4 k0 = pk[0], k1 = pk[1];
        unsigned b1 = 0xFFFFFFFFu, b2 = 0xFFFFFFFFu;     // smallest and second smallest (distance << 16 | position in the node)
        for (int c = n.c0 + lane; c < n.c1; c += 64) {
            const unsigned i2 = B.feat[c];
            if ((BY_IDX1 ? S.taken[i2] != 0 : S.match[i2] >= 0) || (v2 && !v2[i2])) continue;
            const uint4* pf = (const uint4*)(B.desc + (size_t)i2 * 32);
            const unsigned key = ((unsigned)sd_hamming256(k0, k1, pf[0], pf[1]) << 16) | (unsigned)(c - n.c0);
            if (key < b1) { b2 = b1; b1 = key; } else if (key < b2) b2 = key;
        }
        sd_wave_top2_u32(b1, b2);
        if (b1 == 0xFFFFFFFFu) continue;                  // no free valid side-2 feature in this node
        if (sd_bow_accepts<STRICT>(b1, b2, nnratio)) {
            const unsigned i2 = B.feat[n.c0 + (int)(b1 & 0xFFFFu)];
            if (lane == 0) {
                if (BY_IDX1) S.taken[i2] = 1;
                sd_bow_commit<BY_IDX1>(S, i1, i2, A.kp[i1].angle, B.kp[i2].angle, checkOrientation);
            }
            nm++;
            __builtin_amdgcn_wave_barrier();
        }
        __threadfence_block();                            // the flag written by lane 0 is read by every lane next round
    }
    return nm;
}

// The body of k_search_by_bow and k_search_by_bow_kf.  Dynamic LDS: match [cap] int, bin [cap], and for BY_IDX1 taken [cap].
// matchOut[pair][i] for every i < (BY_IDX1 ? cap : N2); nmatchOut[pair] = the return value.
template <bool BY_IDX1, bool STRICT>
__device__ __forceinline__ void sd_search_by_bow(
    const sd_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc, const int* __restrict__ count,
    const unsigned* __restrict__ fvFeat, const int* __restrict__ fvRunStart, const unsigned* __restrict__ fvRunNode,
    const int* __restrict__ meta, const uint8_t* __restrict__ valid1 /*nullable [pair][cap]*/, const uint8_t* __restrict__ valid2,
    const int2* __restrict__ pairIdx, int cap, float nnratio, int checkOrientation, int* __restrict__ matchOut, int* __restrict__ nmatchOut)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int s_hist[SD_HISTO];
    __shared__ SdRotKeep s_keep;
    __shared__ int s_nm;
    SdBowLds S;
    S.match = (int*)smem; S.bin = (uint8_t*)(S.match + cap); S.taken = S.bin + cap; S.hist = s_hist;
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int img1 = pairIdx[pair].x, img2 = pairIdx[pair].y;
    const int N2 = count[img2];
    const int NR = BY_IDX1 ? count[img1] : N2;               // the result's index range
    for (int i = tid; i < NR; i += 64 * SD_BOW_WAVES) S.match[i] = -1;
    if (BY_IDX1) for (int i = tid; i < N2; i += 64 * SD_BOW_WAVES) S.taken[i] = 0;
    if (tid < SD_HISTO) s_hist[tid] = 0;
    if (tid == 0) s_nm = 0;
    __syncthreads();
    const SdFvView A = sd_fv_view(kp, desc, fvFeat, fvRunStart, fvRunNode, meta, img1, cap);
    const SdFvView B = sd_fv_view(kp, desc, fvFeat, fvRunStart, fvRunNode, meta, img2, cap);
    const uint8_t* v1 = valid1 ? valid1 + (size_t)pair * cap : nullptr;
    const uint8_t* v2 = valid2 ? valid2 + (size_t)pair * cap : nullptr;
    int nm = 0;
    for (int r1 = wv; r1 < A.runs; r1 += SD_BOW_WAVES) {
        const SdNodePair n = sd_fv_pair(A, r1, B);
        if (!n.found) continue;
        if (n.c1 - n.c0 <= SD_BOW_REGF) nm += sd_bow_node_regs<BY_IDX1, STRICT>(A, B, n, v1, v2, S, nnratio, checkOrientation, lane);
        else nm += sd_bow_node_mem<BY_IDX1, STRICT>(A, B, n, v1, v2, S, nnratio, checkOrientation, lane);
    }
    if (lane == 0) atomicAdd(&s_nm, nm);
    __syncthreads();
    if (checkOrientation) {
        if (tid == 0) s_keep = sd_three_maxima(s_hist);
        __syncthreads();
        const SdRotKeep keep = s_keep;
        int culled = 0;
        for (int i = tid; i < NR; i += 64 * SD_BOW_WAVES)
            if (S.match[i] >= 0 && !keep.keeps(S.bin[i])) { S.match[i] = -1; culled++; }
        if (culled) atomicSub(&s_nm, culled);
        __syncthreads();
    }
    const int nOut = BY_IDX1 ? cap : NR;
    for (int i = tid; i < nOut; i += 64 * SD_BOW_WAVES) matchOut[(size_t)pair * cap + i] = i < NR ? S.match[i] : -1;
    if (tid == 0) nmatchOut[pair] = s_nm;
}
