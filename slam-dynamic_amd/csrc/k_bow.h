// Bag-of-words kernels: the DBoW2 vocabulary tree of the reference (vendored, Thirdparty/DBoW2) and
// ORBmatcher::SearchByBoW.
//   k_bow_transform     TemplatedVocabulary::transform(feature, word, weight, nid, levelsup)   TemplatedVocabulary.h:1218-1259
//   k_bow_finalize      ... transform(features, BowVector, FeatureVector, levelsup)           TemplatedVocabulary.h:1127-1203
//                       BowVector::addWeight / addIfNotExist / normalize                      BowVector.cpp:35-85
//                       FeatureVector::addFeature                                             FeatureVector.cpp:30-46
//   k_search_by_bow     ORBmatcher::SearchByBoW(KeyFrame*, Frame&, matches)                   src/ORBmatcher.cc:159-288
// The vocabulary is ONE packed buffer (the object bench.py broadcasts over RCCL at start-up):
//   SdVocabHeader | desc[n][32] u8 | weight[n] f64 | parent[n] i32 | childStart[n+1] i32 | childIdx[n-1] i32 | wordId[n] i32
// Node ids are the reference's (line number of the text file, root = 0); children keep file order, which decides ties.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_sort.h"
#include "k_match.h"

struct SdVocabHeader {
    uint32_t magic, version, k, L, scoring, weighting, nNodes, nWords;
    uint64_t offDesc, offWeight, offParent, offChildStart, offChildIdx, offWordId, totalBytes;
    uint64_t pad[5];
};                                     // 128 bytes
#define SD_VOCAB_MAGIC 0x42564453u     // "SDVB"

struct SdVocabDev {                    // device pointers into the packed buffer
    const uint8_t* desc; const double* weight; const int* childStart; const int* childIdx; const int* wordId;
    int L, scoring, weighting, nNodes;
};

// 16 lanes per feature: lane j scores child j (k <= 20 children: at most two rounds), a 16-lane butterfly keeps the
// first minimum in child order (the reference's strict `d < best_d`).
__global__ void __launch_bounds__(256) k_bow_transform(const uint8_t* __restrict__ desc, const int* __restrict__ count,
                                                       const int* __restrict__ imgOf, SdVocabDev V, int levelsup, int cap,
                                                       unsigned* __restrict__ wordOut, double* __restrict__ weightOut,
                                                       unsigned* __restrict__ nidOut)
{
    const int img = imgOf[blockIdx.y];
    const int sub = threadIdx.x & 15;
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int N = count[img];
    const bool act = i < N;                       // whole 16-lane groups go inactive together
    const size_t o = (size_t)img * cap + (act ? i : 0);
    const uint4* df = (const uint4*)(desc + o * 32);
    const uint4 f0 = df[0], f1 = df[1];
    const int nid_level = V.L - levelsup;
    unsigned node = 0, nid = 0;
    bool nidSet = nid_level <= 0;
    int level = 0;
    while (true) {
        const int cs = V.childStart[node], ce = V.childStart[node + 1];
        if (cs == ce) break;                      // leaf
        level++;
        unsigned best = 0xFFFFFFFFu;
        for (int c0 = cs; c0 < ce; c0 += 16) {
            const int idx = c0 + sub;
            unsigned key = 0xFFFFFFFFu;
            if (idx < ce) {
                const unsigned child = (unsigned)V.childIdx[idx];
                const uint4* dn = (const uint4*)(V.desc + (size_t)child * 32);
                key = ((unsigned)sd_hamming256(f0, f1, dn[0], dn[1]) << 16) | (unsigned)(idx - cs);
            }
            best = key < best ? key : best;
        }
#pragma unroll
        for (int d = 8; d > 0; d >>= 1) { const unsigned o2 = (unsigned)__shfl_xor((int)best, d, 16); best = o2 < best ? o2 : best; }
        node = (unsigned)V.childIdx[cs + (int)(best & 0xFFFFu)];
        if (level == nid_level) { nid = node; nidSet = true; }
    }
    if (!nidSet) nid = node;                      // spec Q12: the reference leaves *nid unwritten here
    if (act && sub == 0) { wordOut[o] = (unsigned)V.wordId[node]; weightOut[o] = V.weight[node]; nidOut[o] = nid; }
}

// One workgroup per image.  FeatureVector = the features with weight > 0 sorted by (node id, feature index), + its runs;
// BowVector = the distinct words ascending; a word seen c times holds ((w + w) + ...) summed c times in feature order (all
// terms are the word's own weight) for TF / TF-IDF, w for IDF / BINARY; then the reference's normalisation, summed in
// ascending word order by one lane (double additions do not commute bit-for-bit).
// exclusive scan of s[0..256) in place, total in s[256]; called by all 256 threads between two barriers of the caller
__device__ __forceinline__ void sd_scan256(int* s, int tid)
{
    if (tid < 64) {
        const int a = s[4 * tid], b = s[4 * tid + 1], c = s[4 * tid + 2], d = s[4 * tid + 3];
        const int sum = a + b + c + d;
        int incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (tid >= o) incl += t; }
        const int ex = incl - sum;
        s[4 * tid] = ex; s[4 * tid + 1] = ex + a; s[4 * tid + 2] = ex + a + b; s[4 * tid + 3] = ex + a + b + c;
        if (tid == 63) s[256] = incl;
    }
}

__global__ void __launch_bounds__(256) k_bow_finalize(const int* __restrict__ count, const int* __restrict__ imgOf,
                                                      const unsigned* __restrict__ word, const double* __restrict__ weight,
                                                      const unsigned* __restrict__ nid, int cap, int sortCap, int scoring, int weighting,
                                                      unsigned* __restrict__ fvNode, unsigned* __restrict__ fvFeat,
                                                      int* __restrict__ fvRunStart, unsigned* __restrict__ fvRunNode,
                                                      unsigned* __restrict__ bowWord, double* __restrict__ bowVal,
                                                      int* __restrict__ meta /*[img][4]: nf, nRuns, nb, -*/)
{
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* keys = (unsigned long long*)smem;       // [sortCap]
    int* s_scan = (int*)(keys + sortCap);                        // [256 + 1]
    __shared__ double s_norm;
    const int img = imgOf[blockIdx.x], tid = threadIdx.x;
    const int N = count[img];
    int sortN = 256;                                             // this image's sort size: the power of two above its keypoint count
    while (sortN < N) sortN <<= 1;
    const size_t base = (size_t)img * cap;
    // ---------------- FeatureVector
    for (int t = tid; t < sortN; t += 256) {
        unsigned long long key = ~0ull;
        if (t < N && weight[base + t] > 0) key = ((unsigned long long)nid[base + t] << 32) | (unsigned)t;
        keys[t] = key;
    }
    __syncthreads();
    sd_block_sort64(keys, sortN, tid, 256);
    // nf = number of real keys; runs = distinct node ids.  Chunked scan: thread t owns items [t*per, (t+1)*per)
    const int per = sortN / 256 > 0 ? sortN / 256 : 1;
    {
        int nfLocal = 0, runsLocal = 0;
        for (int q = 0; q < per; q++) {
            const int t = tid * per + q;
            if (t < sortN && keys[t] != ~0ull) {
                nfLocal++;
                if (t == 0 || (keys[t] >> 32) != (keys[t - 1] >> 32)) runsLocal++;
            }
        }
        s_scan[tid] = runsLocal;
        __syncthreads();
        sd_scan256(s_scan, tid);
        __syncthreads();
        int r = s_scan[tid];
        for (int q = 0; q < per; q++) {
            const int t = tid * per + q;
            if (t < sortN && keys[t] != ~0ull) {
                fvNode[base + t] = (unsigned)(keys[t] >> 32); fvFeat[base + t] = (unsigned)(keys[t] & 0xFFFFFFFFu);
                if (t == 0 || (keys[t] >> 32) != (keys[t - 1] >> 32)) { fvRunStart[(size_t)img * (cap + 1) + r] = t; fvRunNode[base + r] = (unsigned)(keys[t] >> 32); r++; }
            }
        }
        const int nRuns = s_scan[256];
        __syncthreads();
        s_scan[tid] = nfLocal;
        __syncthreads();
        if (tid == 0) {
            int nf = 0; for (int k = 0; k < 256; k++) nf += s_scan[k];
            meta[img * 4 + 0] = nf; meta[img * 4 + 1] = nRuns;
            fvRunStart[(size_t)img * (cap + 1) + nRuns] = nf;
        }
        __syncthreads();
    }
    // ---------------- BowVector
    for (int t = tid; t < sortN; t += 256) {
        unsigned long long key = ~0ull;
        if (t < N && weight[base + t] > 0) key = ((unsigned long long)word[base + t] << 32) | (unsigned)t;
        keys[t] = key;
    }
    __syncthreads();
    sd_block_sort64(keys, sortN, tid, 256);
    {
        int local = 0;
        for (int q = 0; q < per; q++) {
            const int t = tid * per + q;
            if (t < sortN && keys[t] != ~0ull && (t == 0 || (keys[t] >> 32) != (keys[t - 1] >> 32))) local++;
        }
        s_scan[tid] = local;
        __syncthreads();
        sd_scan256(s_scan, tid);
        __syncthreads();
        int r = s_scan[tid];
        const int nb = s_scan[256];
        for (int q = 0; q < per; q++) {
            const int t = tid * per + q;
            if (t < sortN && keys[t] != ~0ull && (t == 0 || (keys[t] >> 32) != (keys[t - 1] >> 32))) {
                const unsigned w = (unsigned)(keys[t] >> 32);
                int c = 1;
                while (t + c < sortN && (unsigned)(keys[t + c] >> 32) == w) c++;
                const double wv = weight[base + (unsigned)(keys[t] & 0xFFFFFFFFu)];
                double v = wv;
                if (weighting == 0 || weighting == 1) for (int a = 1; a < c; a++) v += wv;       // addWeight, once per feature
                bowWord[base + r] = w; bowVal[base + r] = v;
                r++;
            }
        }
        __threadfence_block();
        __syncthreads();
        double* vals = (double*)keys;                          // the sorted keys are dead: stage the values for the serial sum
        for (int t = tid; t < nb; t += 256) vals[t] = bowVal[base + t];
        __syncthreads();
        const bool must = scoring != 5;
        if ((weighting == 0 || weighting == 1) && nb > 0 && !must) {
            const double nd = (double)nb;
            for (int t = tid; t < nb; t += 256) vals[t] /= nd;
        }
        __syncthreads();
        if (must) {
            if (tid < 64) {
                // The sum must run in word order (f64 rounding).  Wave 0 fetches 64 values per step (one per lane) and adds them
                // in lane order through v_readlane: ~16 cycles per element instead of an LDS round trip per element.
                double norm = 0.0;
                for (int t0 = 0; t0 < nb; t0 += 64) {
                    const double v = t0 + tid < nb ? vals[t0 + tid] : 0.0;      // +0.0 / 0*0 leave the sum unchanged
                    const double e = scoring != 1 ? fabs(v) : v * v;
                    const unsigned long long bits = __builtin_bit_cast(unsigned long long, e);
                    const int lo = (int)(unsigned)bits, hi = (int)(unsigned)(bits >> 32);
#pragma unroll
                    for (int l = 0; l < 64; l++) {
                        const unsigned long long b = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, l) << 32) | (unsigned)__builtin_amdgcn_readlane(lo, l);
                        norm += __builtin_bit_cast(double, b);
                    }
                }
                if (scoring == 1) norm = sqrt(norm);
                if (tid == 0) s_norm = norm;
            }
            __syncthreads();
            const double norm = s_norm;
            if (norm > 0.0) for (int t = tid; t < nb; t += 256) vals[t] /= norm;
        }
        for (int t = tid; t < nb; t += 256) bowVal[base + t] = vals[t];
        if (tid == 0) meta[img * 4 + 2] = nb;
    }
}

// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, matches): side 1 = the keyframe, side 2 = the frame; matchOut[pair][frame feature] =
// keyframe feature, the acceptance is bestDist1 <= TH_LOW, the frame has no validity mask.  The body is the shared one of k_match.h.
__global__ void __launch_bounds__(64 * SD_BOW_WAVES) k_search_by_bow(
    const sd_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc, const int* __restrict__ count,
    const unsigned* __restrict__ fvFeat, const int* __restrict__ fvRunStart, const unsigned* __restrict__ fvRunNode,
    const int* __restrict__ meta, const uint8_t* __restrict__ kfValid /*nullable [pair][cap]*/, const int2* __restrict__ pairIdx,
    int cap, float nnratio, int checkOrientation, int* __restrict__ matchOut, int* __restrict__ nmatchOut)
{
    sd_search_by_bow<false, false>(kp, desc, count, fvFeat, fvRunStart, fvRunNode, meta, kfValid, nullptr, pairIdx, cap, nnratio,
                                   checkOrientation, matchOut, nmatchOut);
}
