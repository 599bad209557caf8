// The covisibility graph on the device: KeyFrame::UpdateConnections / AddConnection / UpdateBestCovisibles /
// EraseConnection (src/KeyFrame.cc:123-208, 289-379, 553-567) over a device mirror of the map's tables.  The observation relation is not
// stored: the observers of point p are the pool slots with mp[slot] == p, found through a CSR by point that is rebuilt when the tables changed.
//   k_covis_set_matches / _set_matches_dev / _set_bad / _set_parent / _add_batch / _clear_kf   the mutations
//   k_covis_csr_check      after matches came from device arrays: no keyframe may name a point twice
//   k_covis_csr_count / _scan_blocks / _scan_sums / _scan_add / _fill               the inverse index (integer atomics only)
//   k_covis_counter<LDS>   KFcounter of every listed keyframe: one workgroup per keyframe, the counter in LDS or in the job's global row
//   k_covis_apply          one listed keyframe's effects: a workgroup per keyframe id, launched once per job in list order
//   k_covis_erase          EraseConnection on the row of an erased keyframe
//   k_covis_to_kfdb        the first ten of an ordered list into a KeyFrameDatabase entry
//   k_covis_culling        LocalMapping::KeyFrameCulling: one workgroup walks the candidates, because the loop is sequential
//   k_covis_local_map<LDS> Tracking::UpdateLocalKeyFrames + UpdateLocalPoints: one workgroup per frame
// The only floating point is the culling's f32 depth comparison and its one f64 product (no add: nothing contracts).  Integer atomics only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_sort.h"
#include "k_kfdb.h"

#define SD_COVIS_TH 15                 // UpdateConnections: th
#define SD_COVIS_LDS_KF 4096           // KFcounter lives in LDS up to this many keyframe ids (16 KB of the 160 KB: ten workgroups a CU), in a global row above
#define SD_COVIS_MAX_KF 8192           // the rows are dense (12 bytes a pair of ids); the sort of a whole row is 8 bytes a keyframe of LDS
#define SD_COVIS_SORT_LDS(n2) ((size_t)(n2) * 8 + 8)
#define SD_COVIS_SCAN 1024

struct SdCovisKf { int off, n, live, prot; int parent, first, nOrd, pad; };       // the host writes the first 16 bytes, the device the rest
struct SdCovisJob { int kf, nmax, kfmax, any; };                                   // nmax 0: the counter was empty

struct SdCovisArgs {
    SdCovisKf* kf; int* mp; int* owner; unsigned char* oct; unsigned char* st; float* depth; unsigned char* bad;
    int* start; int* cur; int* obs; int* bsum;
    int* row; int* ordId; int* ordW;           // [maxKf][maxKf]
    int* cnt; SdCovisJob* job; const int* list;  // [maxJobs][maxKf], [maxJobs], the listed ids
    int K, stride, P, poolUsed, n2;
};

// ---- mutations
// the three below: one thread per listed item; the host lists every (keyframe, feature), point or keyframe once, with its final value
__global__ void k_covis_set_matches(SdCovisArgs A, const int* kf, const int* idx, const int* mpId, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SdCovisKf E = A.kf[kf[i]];
    if (idx[i] < E.n) A.mp[E.off + idx[i]] = mpId[i];                 // a batch slot's count is the device's: the host checked against its capacity
}

// The same from device arrays.  The host has not seen these items: an entry that names no live keyframe, no feature of it or no possible
// point is left out and raises err[0].
__global__ void k_covis_set_matches_dev(SdCovisArgs A, const int* kf, const int* idx, const int* mpId, int n, int maxPoints, int* err)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = kf[i], f = idx[i], p = mpId[i];
    bool ok = k >= 0 && k < A.K && p >= -1 && p < maxPoints && f >= 0;
    if (ok) {
        const SdCovisKf E = A.kf[k];
        ok = E.live && f < E.n;
        if (ok) A.mp[E.off + f] = p;
    }
    if (!ok) atomicOr(err, 1);
}

// After the index was filled: err[1] when two entries of one point's list belong to one keyframe (two features of a keyframe name the point).
__global__ void k_covis_csr_check(SdCovisArgs A, int* err)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= A.P) return;
    const int b = A.start[p], e = A.start[p + 1];
    for (int o1 = b; o1 < e; o1++) {
        const int k1 = A.owner[A.obs[o1]];
        for (int o2 = o1 + 1; o2 < e; o2++)
            if (A.owner[A.obs[o2]] == k1) { atomicOr(err + 1, 1); return; }
    }
}

__global__ void k_covis_set_bad(unsigned char* bad, const int* id, const int* val, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) bad[id[i]] = val[i] ? 1 : 0;
}

__global__ void k_covis_set_parent(SdCovisArgs A, const int* kf, const int* parent, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) A.kf[kf[i]].parent = parent[i];
}

__global__ void k_covis_add_batch(SdCovisArgs A, int kf, const sd_keypoint* kp, const float* uright, const float* depth, const int* count, int cap)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int n = *count; n = n < 0 ? 0 : (n > cap ? cap : n);
    SdCovisKf* E = A.kf + kf;
    if (i == 0) { E->n = n; E->parent = -1; E->first = 1; E->nOrd = 0; }
    if (i >= cap) return;
    const int s = E->off + i;
    A.mp[s] = -1; A.owner[s] = i < n ? kf : -1;
    A.oct[s] = i < n ? (unsigned char)kp[i].octave : 0; A.st[s] = (i < n && uright[i] >= 0.0f) ? 1 : 0; A.depth[s] = i < n ? depth[i] : 0.0f;
}

__global__ void k_covis_clear_kf(SdCovisArgs A, int kf)
{
    // the matches of an erased keyframe, its row and its ordered list
    const SdCovisKf E = A.kf[kf];
    const int t = blockIdx.x * blockDim.x + threadIdx.x, T = gridDim.x * blockDim.x;
    for (int i = t; i < E.n; i += T) { A.mp[E.off + i] = -1; A.owner[E.off + i] = -1; }
    for (int i = t; i < A.stride; i += T) A.row[(size_t)kf * A.stride + i] = 0;
    if (t == 0) { A.kf[kf].nOrd = 0; A.kf[kf].live = 0; }
}

// ---- the inverse index
__global__ void k_covis_csr_count(SdCovisArgs A)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= A.poolUsed) return;
    const int p = A.mp[s];
    if (p >= 0 && p < A.P) atomicAdd(A.cur + p, 1);
}

// exclusive scan of 1024 ints by one workgroup of 1024 threads; returns the total in every thread
__device__ __forceinline__ int covis_block_scan(int v, int* sh, int tid, int& excl)
{
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < SD_COVIS_SCAN; d <<= 1) {
        const int a = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += a;
        __syncthreads();
    }
    excl = sh[tid] - v;
    const int total = sh[SD_COVIS_SCAN - 1];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(SD_COVIS_SCAN) void k_covis_scan_blocks(SdCovisArgs A)
{
    __shared__ int sh[SD_COVIS_SCAN];
    const int i = blockIdx.x * SD_COVIS_SCAN + threadIdx.x;
    int e;
    const int total = covis_block_scan(i < A.P ? A.cur[i] : 0, sh, threadIdx.x, e);
    if (i < A.P) A.start[i] = e;
    if (threadIdx.x == 0) A.bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(SD_COVIS_SCAN) void k_covis_scan_sums(SdCovisArgs A, int nBlocks)
{
    __shared__ int sh[SD_COVIS_SCAN];
    int carry = 0;
    for (int base = 0; base < nBlocks; base += SD_COVIS_SCAN) {
        const int i = base + threadIdx.x;
        int e;
        const int total = covis_block_scan(i < nBlocks ? A.bsum[i] : 0, sh, threadIdx.x, e);
        if (i < nBlocks) A.bsum[i] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) A.start[A.P] = carry;
}

__global__ __launch_bounds__(SD_COVIS_SCAN) void k_covis_scan_add(SdCovisArgs A)
{
    const int i = blockIdx.x * SD_COVIS_SCAN + threadIdx.x;
    if (i >= A.P) return;
    const int s = A.start[i] + A.bsum[blockIdx.x];
    A.start[i] = s; A.cur[i] = s;
}

__global__ void k_covis_csr_fill(SdCovisArgs A)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= A.poolUsed) return;
    const int p = A.mp[s];
    if (p >= 0 && p < A.P) A.obs[atomicAdd(A.cur + p, 1)] = s;         // the order inside a point's list is unspecified; nothing reads it as an order
}

// ---- UpdateConnections
// KFcounter of job blockIdx.x into cnt[job][0..K): over the keyframe's non-null, non-bad points every observer but itself.
template <bool LDS>
__global__ __launch_bounds__(256) void k_covis_counter(SdCovisArgs A)
{
    extern __shared__ int covis_c[];
    __shared__ unsigned long long best;
    __shared__ int any;
    const int job = blockIdx.x, tid = threadIdx.x, self = A.list[job];
    int* g = A.cnt + (size_t)job * A.stride;
    int* c = LDS ? covis_c : g;
    for (int i = tid; i < A.K; i += 256) c[i] = 0;
    if (tid == 0) { best = 0ull; any = 0; }
    __syncthreads();
    const SdCovisKf E = A.kf[self];
    for (int i = tid; i < E.n; i += 256) {
        const int p = A.mp[E.off + i];
        if (p < 0 || p >= A.P || A.bad[p]) continue;
        for (int o = A.start[p], oe = A.start[p + 1]; o < oe; o++) {
            const int k2 = A.owner[A.obs[o]];
            if (k2 != self && k2 >= 0 && k2 < A.K) atomicAdd(c + k2, 1);
        }
    }
    __syncthreads();
    // nmax and pKFmax: the largest count, the lowest id among equals (picked on > in ascending id)
    unsigned long long mine = 0ull; int some = 0;
    for (int i = tid; i < A.K; i += 256) {
        const int w = LDS ? c[i] : __hip_atomic_load(c + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the global row was counted by atomics
        if (LDS) g[i] = w;
        if (w > 0) {
            const unsigned long long key = ((unsigned long long)(unsigned)w << 32) | (unsigned)(0x7FFFFFFF - i);
            mine = key > mine ? key : mine;
            some |= w >= SD_COVIS_TH;
        }
    }
    if (mine) atomicMax(&best, mine);
    if (some) atomicOr(&any, 1);
    __syncthreads();
    if (tid == 0) {
        SdCovisJob J;
        J.kf = self; J.nmax = (int)(best >> 32); J.kfmax = best ? 0x7FFFFFFF - (int)(best & 0xFFFFFFFFu) : -1; J.any = any;
        A.job[job] = J;
    }
}

// A row (with entry `ovId` read as `ovW` when ovId >= 0) ordered by descending (weight, id) into the keyframe's list.  minW: entries below it
// are left out; only: >= 0 keeps that id alone.
__device__ __forceinline__ void covis_order(const SdCovisArgs& A, const int* row, int ovId, int ovW, int minW, int only, int target, unsigned long long* keys, int* nsh)
{
    const int tid = threadIdx.x;
    if (tid == 0) *nsh = 0;
    __syncthreads();
    int m = 0;
    for (int i = tid; i < A.n2; i += 256) {
        int w = i < A.K ? (i == ovId ? ovW : row[i]) : 0;
        if (w < minW || (only >= 0 && i != only)) w = 0;
        keys[i] = w > 0 ? (((unsigned long long)(unsigned)w << 32) | (unsigned)i) : 0ull;
        m += w > 0;
    }
    if (m) atomicAdd(nsh, m);
    __syncthreads();
    sd_block_sort64(keys, A.n2, tid, 256);
    const int n = *nsh;
    int* oi = A.ordId + (size_t)target * A.stride; int* ow = A.ordW + (size_t)target * A.stride;
    for (int j = tid; j < n; j += 256) {
        const unsigned long long k = keys[A.n2 - 1 - j];
        oi[j] = (int)(k & 0xFFFFFFFFu); ow[j] = (int)(k >> 32);
    }
    if (tid == 0) A.kf[target].nOrd = n;
    __syncthreads();
}

// The effects of job `job`: workgroup X = the listed keyframe itself (its row becomes KFcounter, its list the kept pairs, its parent the
// front on a first connection) or a kept keyframe (AddConnection: nothing when it holds that weight already, else its entry is written and
// its list rebuilt from its whole row).  Launched once per job, so the jobs of a call take effect in list order.
__global__ __launch_bounds__(256) void k_covis_apply(SdCovisArgs A, int job)
{
    extern __shared__ unsigned long long covis_keys[];       // n2 keys, then the list length
    int* const nsh = (int*)(covis_keys + A.n2);
    const SdCovisJob J = A.job[job];
    const int X = blockIdx.x, tid = threadIdx.x;
    if (J.nmax == 0) return;                                           // empty counter: nothing changes
    const int* c = A.cnt + (size_t)job * A.stride;
    if (X == J.kf) {
        int* row = A.row + (size_t)X * A.stride;
        for (int i = tid; i < A.K; i += 256) row[i] = c[i];
        covis_order(A, c, -1, 0, J.any ? SD_COVIS_TH : 1, J.any ? -1 : J.kfmax, X, covis_keys, nsh);
        if (tid == 0) {
            SdCovisKf* E = A.kf + X;
            if (E->first && !E->prot) { E->parent = A.ordId[(size_t)X * A.stride]; E->first = 0; }
        }
        return;
    }
    const int w = c[X];
    if (!(J.any ? w >= SD_COVIS_TH : X == J.kfmax)) return;
    int* row = A.row + (size_t)X * A.stride;
    if (row[J.kf] == w) return;
    covis_order(A, row, J.kf, w, 1, -1, X, covis_keys, nsh);
    if (tid == 0) row[J.kf] = w;
}

// EraseConnection(kf) on every keyframe of kf's row: workgroup X drops its entry and re-sorts from its whole row.  k_covis_clear_kf follows.
__global__ __launch_bounds__(256) void k_covis_erase(SdCovisArgs A, int kf)
{
    extern __shared__ unsigned long long covis_keys[];
    int* const nsh = (int*)(covis_keys + A.n2);
    const int X = blockIdx.x;
    if (X == kf || A.row[(size_t)kf * A.stride + X] == 0) return;
    int* row = A.row + (size_t)X * A.stride;
    if (row[kf] == 0) return;                                          // mConnectedKeyFrameWeights.count(pKF) == 0: no update
    covis_order(A, row, kf, 0, 1, -1, X, covis_keys, nsh);
    if (threadIdx.x == 0) row[kf] = 0;
}

// GetBestCovisibilityKeyFrames(10) of the listed keyframes into the neighbour fields of their KeyFrameDatabase entries
__global__ void k_covis_to_kfdb(SdCovisArgs A, SdKfdbEntry* entry, int n)
{
    const int j = blockIdx.x, t = threadIdx.x;
    if (j >= n || t >= SD_KFDB_NEIGH) return;
    const int kf = A.list[j];
    const int m = min(A.kf[kf].nOrd, SD_KFDB_NEIGH);
    entry[kf].neigh[t] = t < m ? A.ordId[(size_t)kf * A.stride + t] : 0;
    if (t == 0) entry[kf].nNeigh = m;
}

// ---- LocalMapping::KeyFrameCulling (src/LocalMapping.cc:633-697)
struct SdCovisCull { int flag, nMPs, nRedundant; };                    // == sd_covis_cull_result

// One workgroup walks the candidate list, because the reference's loop is sequential: a flagged candidate whose not_erase is 0 is removed for
// every later one.  Nothing is written to the graph: `removed` lives in LDS, and what a removal does to a point is recomputed from its
// observer list -- the removed observers do not count, and a point that lost one and is left with a weighted count <= 2 is bad
// (MapPoint::EraseObservation -> SetBadFlag).  The count only falls, so "is <= 2 now and lost one" is "went bad at some removal".
__global__ __launch_bounds__(1024) void k_covis_culling(SdCovisArgs A, const int* notErase, int n, int monocular, float thDepth, SdCovisCull* out)
{
    __shared__ unsigned char removed[SD_COVIS_MAX_KF];
    __shared__ int nMPs, nRed;
    const int tid = threadIdx.x;
    for (int i = tid; i < A.K; i += 1024) removed[i] = 0;
    __syncthreads();
    for (int c = 0; c < n; c++) {
        const int kf = A.list[c];
        const SdCovisKf E = A.kf[kf];
        if (tid == 0) { nMPs = 0; nRed = 0; }
        __syncthreads();
        if (!E.prot) {
            int myMPs = 0, myRed = 0;
            for (int i = tid; i < E.n; i += 1024) {
                const int s = E.off + i, p = A.mp[s];
                if (p < 0 || p >= A.P || A.bad[p]) continue;
                if (!monocular) { const float d = A.depth[s]; if (d > thDepth || d < 0.0f) continue; }
                const int lvl = A.oct[s];
                int obsW = 0, lost = 0, fine = 0;
                for (int o = A.start[p], oe = A.start[p + 1]; o < oe; o++) {
                    const int s2 = A.obs[o], k2 = A.owner[s2];
                    if (k2 < 0 || k2 >= A.K) continue;
                    if (removed[k2]) { lost = 1; continue; }
                    obsW += A.st[s2] ? 2 : 1;
                    if (k2 != kf && (int)A.oct[s2] <= lvl + 1) fine++;
                }
                if (lost && obsW <= 2) continue;                      // bad since a removal of this call
                myMPs++;
                if (obsW > 3 && fine >= 3) myRed++;
            }
            if (myMPs) atomicAdd(&nMPs, myMPs);
            if (myRed) atomicAdd(&nRed, myRed);
        }
        __syncthreads();
        const int flag = !E.prot && (double)nRed > 0.9 * (double)nMPs;
        if (tid == 0) {
            SdCovisCull R; R.flag = flag; R.nMPs = nMPs; R.nRedundant = nRed;
            out[c] = R;
            if (flag && !notErase[c]) removed[kf] = 1;
        }
        __syncthreads();
    }
}

// ---- Tracking::UpdateLocalKeyFrames + UpdateLocalPoints (src/Tracking.cc:2076-2210)
struct SdCovisLocal { int nKf, nFirst, refKf, nPoints, overflow, nBadEntries; };       // == sd_covis_local_info
struct SdCovisQ { int off, n; };

__device__ __forceinline__ int covis_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One workgroup per query.  c[id] > 0 while voting = the votes; afterwards c[id] != 0 = "mnTrackReferenceForFrame == this frame".
template <bool LDS>
__global__ __launch_bounds__(1024) void k_covis_local_map(SdCovisArgs A, const SdCovisQ* qs, const int* frameMp, unsigned char* entryBad, int* lkf, int* lpt,
                                                           unsigned* seen, int seenWords, int maxLocal, SdCovisLocal* info)
{
    extern __shared__ int covis_c[];
    __shared__ int sh[SD_COVIS_SCAN];
    __shared__ unsigned long long best;
    __shared__ int nList, nBad, child, stop, nPts, ovf;
    const int q = blockIdx.x, tid = threadIdx.x;
    const SdCovisQ Q = qs[q];
    int* c = LDS ? covis_c : A.cnt + (size_t)q * A.stride;
    int* L = lkf + (size_t)q * A.stride;
    int* out = lpt + (size_t)q * maxLocal;
    unsigned* bits = seen + (size_t)q * seenWords;
    for (int i = tid; i < A.K; i += 1024) c[i] = 0;
    if (tid == 0) { best = 0ull; nList = 0; nBad = 0; stop = 0; nPts = 0; ovf = 0; }
    __syncthreads();
    // the votes of the frame's non-bad points; its entries that name a bad point are reported (the reference nulls them)
    int myBad = 0;
    for (int e = tid; e < Q.n; e += 1024) {
        const int p = frameMp[Q.off + e];
        int isBad = 0;
        if (p >= 0 && p < A.P) {
            if (A.bad[p]) isBad = 1;
            else
                for (int o = A.start[p], oe = A.start[p + 1]; o < oe; o++) {
                    const int k2 = A.owner[A.obs[o]];
                    if (k2 >= 0 && k2 < A.K) atomicAdd(c + k2, 1);
                }
        }
        if (entryBad) entryBad[Q.off + e] = (unsigned char)isBad;
        myBad += isBad;
    }
    if (myBad) atomicAdd(&nBad, myBad);
    __syncthreads();
    // the voted keyframes in ascending id (an observer is live by construction); pKFmax on > in ascending id
    for (int base = 0; base < A.K; base += SD_COVIS_SCAN) {
        const int i = base + tid;
        const int w = i < A.K ? covis_ld(c + i) : 0;
        int e;
        const int total = covis_block_scan(w > 0, sh, tid, e);
        if (w > 0) {
            L[nList + e] = i;
            const unsigned long long key = ((unsigned long long)(unsigned)w << 32) | (unsigned)(0x7FFFFFFF - i);
            atomicMax(&best, key);
        }
        __syncthreads();
        if (tid == 0) nList += total;
        __syncthreads();
    }
    const int nFirst = nList;
    // the neighbours of the first segment's members: the reference's loop, statement by statement
    for (int m = 0; m < nFirst; m++) {
        if (tid == 0) {
            child = 0x7FFFFFFF;
            if (nList > 80) stop = 1;
        }
        __syncthreads();
        if (stop) break;
        const int kf = L[m];
        if (tid == 0) {
            const int nb = min(A.kf[kf].nOrd, SD_KFDB_NEIGH);
            for (int j = 0; j < nb; j++) {
                const int x = A.ordId[(size_t)kf * A.stride + j];
                if (A.kf[x].live && covis_ld(c + x) == 0) { L[nList++] = x; c[x] = 1; break; }
            }
        }
        __syncthreads();
        for (int i = tid; i < A.K; i += 1024)                          // GetChilds() is a set<KeyFrame*>: ascending id
            if (i != kf && A.kf[i].live && A.kf[i].parent == kf && covis_ld(c + i) == 0) atomicMin(&child, i);
        __syncthreads();
        if (tid == 0) {
            if (child != 0x7FFFFFFF) { L[nList++] = child; c[child] = 1; }
            const int par = A.kf[kf].parent;
            if (par >= 0 && par < A.K && covis_ld(c + par) == 0) { L[nList++] = par; c[par] = 1; stop = 1; }      // this break leaves the whole loop
        }
        __syncthreads();
        if (stop) break;
    }
    __syncthreads();
    const int nKf = nList;
    // the local points: first occurrence over (local keyframes in list order, feature index).  A keyframe never names a point twice, so the
    // features of one keyframe are independent of each other.
    for (int m = 0; m < nKf; m++) {
        const SdCovisKf E = A.kf[L[m]];
        for (int base = 0; base < E.n; base += SD_COVIS_SCAN) {
            const int i = base + tid;
            int p = -1;
            if (i < E.n && E.live) {
                p = A.mp[E.off + i];
                if (p >= 0 && (p >= A.P || A.bad[p] || ((__hip_atomic_load(bits + (p >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (p & 31)) & 1u))) p = -1;
            }
            int e;
            const int total = covis_block_scan(p >= 0, sh, tid, e);
            if (p >= 0) {
                atomicOr(bits + (p >> 5), 1u << (p & 31));
                if (nPts + e < maxLocal) out[nPts + e] = p;
            }
            __syncthreads();
            if (tid == 0) { if (nPts + total > maxLocal) ovf = 1; nPts += total; }
            __syncthreads();
        }
    }
    if (tid == 0) {
        SdCovisLocal I;
        I.nKf = nKf; I.nFirst = nFirst; I.refKf = best ? 0x7FFFFFFF - (int)(best & 0xFFFFFFFFu) : -1; I.nPoints = nPts; I.overflow = ovf; I.nBadEntries = nBad;
        info[q] = I;
    }
}
