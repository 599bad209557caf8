// KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:76-309) and the L1 score of
// DBoW2 (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) over a device-resident table of BowVectors.  There is no inverted file: every
// live entry is matched against every query of the call.  Five kernels per call:
//   k_kfdb_excl        (loop form) the excluded set as a [query][kf] byte table
//   k_kfdb_match<0>    common-word count, smallest shared word and si of every (query, live entry): one wave per entry
//   k_kfdb_threshold   per query maxCommonWords, minCommonWords and the length of lKFsSharingWords
//   k_kfdb_tail        per query the list order, lScoreAndMatch, the covisibility accumulation, the retention and the first-occurrence rule
//   k_kfdb_reloc_store (reloc form) mRelocScore of every entry some query of the call scored
// k_kfdb_match<1> is sd_kfdb_score: the same wave function over a caller's list of entries.
// Nothing here multiplies and adds, so nothing can contract; the f64 sum of a score is added by one in-order loop per wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SD_KFDB_NEIGH 10
#define SD_KFDB_EPB 4                  // entries per workgroup of k_kfdb_match: one per wave (a lone query is bound by latency, not by traffic)
#define SD_KFDB_UNROLL 4               // binary searches a lane keeps in flight
#define SD_KFDB_TT 1024                // threads of k_kfdb_tail: one workgroup per query, so its width is the query's latency
#define SD_KFDB_TAIL_LDS (SD_KFDB_SORT_LDS * 12 + SD_KFDB_TT * 8 + (SD_KFDB_TT / 64 + 4) * 4)      // keys, kf ids, the reduction's values and positions, wave sums, two counters
#define SD_KFDB_SORT_LDS 4096          // sharing lists up to this length are ordered in LDS, longer ones in the database's own scratch rows

struct SdKfdbEntry {                   // 64 bytes; the host writes the first 14 words, the device `count` (batch adds) and `reloc`
    int off; unsigned seq; int live; int nNeigh; int neigh[SD_KFDB_NEIGH];
    int count; float reloc;
};
struct SdKfdbQ { long long start; int n; int slot; float minScore; int auxOff; int auxN; int pad; };      // n < 0: the count is meta[slot][2]
struct SdKfdbInfo { int nShare, maxC, minC, nscores, nAcc, nCand; float bestAcc, minRetain; };             // == sd_kfdb_query_info
struct SdKfdbMember { int kf, common, scored; float si; };                                                  // == sd_kfdb_member
struct SdKfdbAcc { float acc; int best; };                                                                  // == sd_kfdb_acc

struct SdKfdbArgs {
    SdKfdbEntry* entry; const unsigned* poolW; const double* poolV;
    const SdKfdbQ* q; const unsigned* qWord; const double* qVal; const int* meta; const int* aux;
    int K, stride, nQ, maxQW, sortStride, reloc;
    int* cnt; unsigned* firstW; float* si; unsigned char* excl; int* mark;
    unsigned long long* sortKey; int* sortKf;
    SdKfdbInfo* info; SdKfdbMember* member; SdKfdbAcc* acc; int* cand;
    float* score;
};

__device__ __forceinline__ int kfdb_query_words(const SdKfdbArgs& A, const SdKfdbQ& Q)
{
    const int n = Q.n >= 0 ? Q.n : A.meta[Q.slot * 4 + 2];
    return n < 0 ? 0 : (n > A.maxQW ? A.maxQW : n);
}

// One entry against the query whose ascending words lie in LDS: the lanes stride over the entry's words, four binary searches each in
// flight; the terms of the common words are added to S in ascending word order by a loop over the ballot, so every lane holds the same S.
__device__ __forceinline__ double kfdb_wave_entry(const unsigned* qw, int nq, int top, const double* qv, const unsigned* ew, const double* ev, int ne,
                                                  int lane, int& count, unsigned& first)
{
    double S = 0.0;
    count = 0; first = 0xFFFFFFFFu;
    if (nq <= 0) return S;
    unsigned next[SD_KFDB_UNROLL];
#pragma unroll
    for (int u = 0; u < SD_KFDB_UNROLL; u++) next[u] = u * 64 + lane < ne ? ew[u * 64 + lane] : 0u;
    for (int base = 0; base < ne; base += 64 * SD_KFDB_UNROLL) {
        unsigned w[SD_KFDB_UNROLL]; int pos[SD_KFDB_UNROLL]; double t[SD_KFDB_UNROLL]; bool hit[SD_KFDB_UNROLL];
#pragma unroll
        for (int u = 0; u < SD_KFDB_UNROLL; u++) {                   // the next step's words travel while this step searches
            const int i = base + (SD_KFDB_UNROLL + u) * 64 + lane;
            w[u] = next[u];
            next[u] = i < ne ? ew[i] : 0u;
            pos[u] = 0;
        }
        // lower bound: pos = number of query words < w.  Every read is unconditional (the index is clamped, nq > 0 here) so that the four
        // LDS reads of a step are in flight together instead of one per branch.
        for (int step = top; step > 0; step >>= 1) {
            unsigned x[SD_KFDB_UNROLL];
#pragma unroll
            for (int u = 0; u < SD_KFDB_UNROLL; u++) x[u] = qw[min(pos[u] + step, nq) - 1];
#pragma unroll
            for (int u = 0; u < SD_KFDB_UNROLL; u++) {
                const int p = pos[u] + step;
                pos[u] = (p <= nq && x[u] < w[u]) ? p : pos[u];
            }
        }
        unsigned at[SD_KFDB_UNROLL];
#pragma unroll
        for (int u = 0; u < SD_KFDB_UNROLL; u++) at[u] = qw[min(pos[u], nq - 1)];
#pragma unroll
        for (int u = 0; u < SD_KFDB_UNROLL; u++) {
            const int i = base + u * 64 + lane;
            hit[u] = i < ne && pos[u] < nq && at[u] == w[u];
            t[u] = 0.0;
            if (hit[u]) {
                const double vi = qv[pos[u]], wi = ev[i];
                t[u] = (fabs(vi - wi) - fabs(vi)) - fabs(wi);
            }
        }
#pragma unroll
        for (int u = 0; u < SD_KFDB_UNROLL; u++) {
            unsigned long long m = __ballot(hit[u]);
            if (m) {
                if (count == 0) first = (unsigned)__shfl((int)w[u], __ffsll((long long)m) - 1);
                count += __popcll(m);
                while (m) {
                    const int l = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    S += __shfl(t[u], l);
                }
            }
        }
    }
    return S;
}

// MODE 0: grid (tiles of SD_KFDB_EPB entry ids, queries) -> cnt / firstW / si of every id below K (cnt 0: not live, excluded or nothing shared).
// MODE 1: grid (tiles of the longest list, queries) -> score[auxOff + j] of list item j, -1 where the listed id is not live.
template <int MODE>
__global__ __launch_bounds__(256) void k_kfdb_match(SdKfdbArgs A)
{
    extern __shared__ unsigned kfdb_qw[];
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SdKfdbQ Q = A.q[q];
    const int first = blockIdx.x * SD_KFDB_EPB;
    if (MODE == 1 && first >= Q.auxN) return;
    const int nq = kfdb_query_words(A, Q);
    const unsigned* gw = A.qWord + Q.start;
    const double* qv = A.qVal + Q.start;
    for (int i = tid; i < nq; i += 256) kfdb_qw[i] = gw[i];
    __syncthreads();
    int top = 0;
    if (nq > 0) { top = 1; while (top * 2 <= nq) top *= 2; }
    for (int k = 0; k < SD_KFDB_EPB / 4; k++) {
        const int item = first + k * 4 + wave;
        int e = item;
        if (MODE == 1) {
            if (item >= Q.auxN) continue;
            e = A.aux[Q.auxOff + item];
        } else if (item >= A.K) continue;
        const bool inRange = e >= 0 && e < A.K;
        const size_t row = (size_t)q * A.stride + (inRange ? e : 0);
        bool ok = false;
        int off = 0, ne = 0;
        if (inRange) {
            const SdKfdbEntry* E = A.entry + e;
            ok = E->live != 0;
            off = E->off; ne = E->count;
            if (MODE == 0 && ok && A.excl && A.excl[row]) ok = false;
        }
        int count = 0; unsigned fw = 0xFFFFFFFFu; double S = 0.0;
        if (ok) S = kfdb_wave_entry(kfdb_qw, nq, top, qv, A.poolW + off, A.poolV + off, ne, lane, count, fw);
        if (lane == 0) {
            const float si = (float)(-S / 2.0);
            if (MODE == 1) A.score[Q.auxOff + item] = ok ? si : -1.0f;
            else { A.cnt[row] = count; A.firstW[row] = fw; A.si[row] = si; }
        }
    }
}

// spConnectedKeyFrames of every query as bytes; ids at or above K cannot be live
__global__ __launch_bounds__(256) void k_kfdb_excl(SdKfdbArgs A)
{
    const int q = blockIdx.x, tid = threadIdx.x;
    unsigned char* row = A.excl + (size_t)q * A.stride;
    for (int e = tid; e < A.K; e += 256) row[e] = 0;
    __syncthreads();
    const SdKfdbQ Q = A.q[q];
    for (int j = tid; j < Q.auxN; j += 256) {
        const int id = A.aux[Q.auxOff + j];
        if (id >= 0 && id < A.K) row[id] = 1;
    }
}

// maxCommonWords, minCommonWords = (int)(maxCommonWords * 0.8f) and lKFsSharingWords.size()  (KeyFrameDatabase.cc:112-120, 227-235)
__global__ __launch_bounds__(256) void k_kfdb_threshold(SdKfdbArgs A)
{
    __shared__ int s_max, s_n;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) { s_max = 0; s_n = 0; }
    __syncthreads();
    const int* cnt = A.cnt + (size_t)q * A.stride;
    int mx = 0, n = 0;
    for (int e = tid; e < A.K; e += 256) {
        const int c = cnt[e];
        if (c > 0) { n++; mx = c > mx ? c : mx; }
    }
    if (n) { atomicMax(&s_max, mx); atomicAdd(&s_n, n); }
    __syncthreads();
    if (tid == 0) {
        SdKfdbInfo I;
        I.nShare = s_n; I.maxC = s_max; I.minC = (int)((float)s_max * 0.8f);
        I.nscores = 0; I.nAcc = 0; I.nCand = 0; I.bestAcc = 0.f; I.minRetain = 0.f;
        A.info[q] = I;
    }
}

// ascending bitonic sort of n (power of two) keys with a payload by one workgroup, in LDS or in device memory
template <typename KP, typename VP>
__device__ __forceinline__ void kfdb_sort_pairs(KP keys, VP vals, int n, int tid, int nthreads)
{
    // as sd_block_sort64: a thread owns compare-exchange pairs, four per step with all their reads in flight together
    const int half = n >> 1;
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p0 = tid; p0 < half; p0 += 4 * nthreads) {
                unsigned long long a[4], b[4];
                int va[4], vb[4], tt[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int p = p0 + u * nthreads;
                    tt[u] = -1;
                    if (p < half) {
                        const int t = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                        tt[u] = t; a[u] = keys[t]; b[u] = keys[t | j]; va[u] = vals[t]; vb[u] = vals[t | j];
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int t = tt[u];
                    if (t >= 0 && (a[u] > b[u]) == ((t & k) == 0)) {
                        keys[t] = b[u]; keys[t | j] = a[u];
                        vals[t] = vb[u]; vals[t | j] = va[u];
                    }
                }
            }
            __syncthreads();
        }
}

// exclusive position of every set flag among the workgroup's SD_KFDB_TT threads, in thread order; total = their number
__device__ __forceinline__ int kfdb_block_scan(bool flag, int tid, int* s_w, int& total)
{
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned long long m = __ballot(flag);
    const int ex = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    int off = 0;
    for (int k = 0; k < wave; k++) off += s_w[k];
    total = 0;
    for (int k = 0; k < SD_KFDB_TT / 64; k++) total += s_w[k];
    __syncthreads();
    return off + ex;
}

// the score a neighbour contributes in the reloc form: this query's if it scored the entry, else that of the latest
// earlier query of the call that did, else the stored mRelocScore
__device__ __forceinline__ float kfdb_reloc_score(const SdKfdbArgs& A, int q, int nb, int c, int minC)
{
    if (c > minC) return A.si[(size_t)q * A.stride + nb];
    for (int p = q - 1; p >= 0; p--)
        if (A.cnt[(size_t)p * A.stride + nb] > A.info[p].minC) return A.si[(size_t)p * A.stride + nb];
    return A.entry[nb].reloc;
}

// KeyFrameDatabase.cc:122-196 / 237-308 for one query per workgroup
__global__ __launch_bounds__(SD_KFDB_TT) void k_kfdb_tail(SdKfdbArgs A)
{
    // all of the workgroup's LDS is dynamic (SD_KFDB_TAIL_LDS bytes), carved at multiples of 16: a static variable in front of it would
    // shift the base of the 64-bit keys
    extern __shared__ __attribute__((aligned(16))) unsigned long long kfdb_keys[];        // SD_KFDB_SORT_LDS keys, then as many kf ids
    float* s_val = (float*)(kfdb_keys + SD_KFDB_SORT_LDS) + SD_KFDB_SORT_LDS;
    int* s_idx = (int*)(s_val + SD_KFDB_TT);
    int* s_w = s_idx + SD_KFDB_TT;
    int& s_n = s_w[SD_KFDB_TT / 64];
    int& s_nsc = s_w[SD_KFDB_TT / 64 + 1];
    const int q = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)q * A.stride;
    const int* cnt = A.cnt + row;
    const float* si = A.si + row;
    int* mark = A.mark + row;
    int* L = A.sortKf + (size_t)q * A.sortStride;
    SdKfdbInfo I = A.info[q];
    const int n = I.nShare, minC = I.minC;
    const float minScore = A.reloc ? 0.f : A.q[q].minScore;

    // lKFsSharingWords in the order of (smallest shared word, sequence number)
    int P = 1;
    while (P < n) P <<= 1;
    const bool inLds = P <= SD_KFDB_SORT_LDS;
    unsigned long long* gk = A.sortKey + (size_t)q * A.sortStride;
    int* lkf = (int*)(kfdb_keys + SD_KFDB_SORT_LDS);
    if (tid == 0) { s_n = 0; s_nsc = 0; }
    if (inLds) { for (int i = n + tid; i < P; i += SD_KFDB_TT) { kfdb_keys[i] = ~0ull; lkf[i] = -1; } }
    else { for (int i = n + tid; i < P; i += SD_KFDB_TT) { gk[i] = ~0ull; L[i] = -1; } }
    __syncthreads();
    for (int e = tid; e < A.K; e += SD_KFDB_TT) {
        mark[e] = 0x7FFFFFFF;
        if (cnt[e] > 0) {
            const int p = atomicAdd(&s_n, 1);
            const unsigned long long key = ((unsigned long long)A.firstW[row + e] << 32) | A.entry[e].seq;
            if (p < n) {
                if (inLds) { kfdb_keys[p] = key; lkf[p] = e; }
                else { gk[p] = key; L[p] = e; }
            }
        }
    }
    __syncthreads();
    if (n > 1) {
        if (inLds) kfdb_sort_pairs(kfdb_keys, lkf, P, tid, SD_KFDB_TT);
        else kfdb_sort_pairs(gk, L, P, tid, SD_KFDB_TT);
    }
    if (inLds) for (int i = tid; i < n; i += SD_KFDB_TT) L[i] = lkf[i];
    __syncthreads();

    // the members, lScoreAndMatch and the accumulation over GetBestCovisibilityKeyFrames(10)
    SdKfdbMember* member = A.member + row;
    SdKfdbAcc* acc = A.acc + row;
    int nAcc = 0;
    for (int base = 0; base < n; base += SD_KFDB_TT) {
        const int i = base + tid;
        bool kept = false;
        int e = -1;
        float s = 0.f;
        if (i < n) {
            e = L[i];
            const int c = cnt[e];
            const bool scored = c > minC;
            s = scored ? si[e] : 0.f;
            SdKfdbMember M; M.kf = e; M.common = c; M.scored = scored ? 1 : 0; M.si = s;
            member[i] = M;
            if (scored) atomicAdd(&s_nsc, 1);
            kept = scored && (A.reloc || s >= minScore);
        }
        int total;
        const int pos = nAcc + kfdb_block_scan(kept, tid, s_w, total);
        nAcc += total;
        if (kept) {
            float best = s, accScore = s;
            int bestKf = e;
            const SdKfdbEntry* E = A.entry + e;
            const int nn = E->nNeigh < SD_KFDB_NEIGH ? E->nNeigh : SD_KFDB_NEIGH;
            for (int j = 0; j < nn; j++) {
                const int nb = E->neigh[j];
                if (nb < 0 || nb >= A.K || !A.entry[nb].live) continue;
                const int c2 = cnt[nb];
                if (c2 <= 0) continue;                                   // not in lKFsSharingWords (or excluded)
                float s2;
                if (A.reloc) s2 = kfdb_reloc_score(A, q, nb, c2, minC);
                else { if (!(c2 > minC)) continue; s2 = si[nb]; }
                accScore += s2;
                if (s2 > best) { bestKf = nb; best = s2; }
            }
            SdKfdbAcc R; R.acc = accScore; R.best = bestKf;
            acc[pos] = R;
        }
    }
    __syncthreads();

    // bestAccScore: the sequential `if (acc > best) best = acc` keeps, among equal maxima, the earliest (the start value comes first)
    float bv = minScore;
    int bi = tid == 0 ? -1 : 0x7FFFFFFF;                                 // 0x7FFFFFFF: nothing seen yet
    for (int i = tid; i < nAcc; i += SD_KFDB_TT) {
        const float v = acc[i].acc;
        if (bi == 0x7FFFFFFF || v > bv) { bv = v; bi = i; }
    }
    s_val[tid] = bv; s_idx[tid] = bi;
    __syncthreads();
    for (int h = SD_KFDB_TT / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const float v = s_val[tid + h]; const int ix = s_idx[tid + h];
            const float mv = s_val[tid]; const int mi = s_idx[tid];
            if (ix != 0x7FFFFFFF && (mi == 0x7FFFFFFF || v > mv || (v == mv && ix < mi))) { s_val[tid] = v; s_idx[tid] = ix; }
        }
        __syncthreads();
    }
    const float bestAcc = s_val[0];
    const float minRetain = 0.75f * bestAcc;

    // retention and the first occurrence of every pBestKF
    for (int i = tid; i < nAcc; i += SD_KFDB_TT)
        if (acc[i].acc > minRetain) atomicMin(&mark[acc[i].best], i);
    __syncthreads();
    int* cand = A.cand + row;
    int nCand = 0;
    for (int base = 0; base < nAcc; base += SD_KFDB_TT) {
        const int i = base + tid;
        bool out = false;
        int kf = -1;
        if (i < nAcc) { kf = acc[i].best; out = acc[i].acc > minRetain && mark[kf] == i; }
        int total;
        const int pos = nCand + kfdb_block_scan(out, tid, s_w, total);
        nCand += total;
        if (out) cand[pos] = kf;
    }
    if (tid == 0) {
        I.nscores = s_nsc; I.nAcc = nAcc; I.nCand = nCand; I.bestAcc = bestAcc; I.minRetain = minRetain;
        A.info[q] = I;
    }
}

// mRelocScore after the call: the score of the last query that scored the entry
__global__ __launch_bounds__(256) void k_kfdb_reloc_store(SdKfdbArgs A)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= A.K || !A.entry[e].live) return;
    for (int p = A.nQ - 1; p >= 0; p--)
        if (A.cnt[(size_t)p * A.stride + e] > A.info[p].minC) { A.entry[e].reloc = A.si[(size_t)p * A.stride + e]; return; }
}

// KeyFrameDatabase::add from a slot of sd_batch_compute_bow: the slot's BowVector into the pool, its length and mRelocScore = 0 into the entry
__global__ __launch_bounds__(256) void k_kfdb_add_batch(const unsigned* word, const double* value, const int* meta, int cap, SdKfdbEntry* E,
                                                        unsigned* poolW, double* poolV)
{
    int n = meta[2];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int off = E->off;
    if (i < n) { poolW[off + i] = word[i]; poolV[off + i] = value[i]; }
    if (i == 0) { E->count = n; E->reloc = 0.f; }
}
