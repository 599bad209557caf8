// PnPsolver (src/PnPsolver.cc) for many independent relocalisation candidates in one launch sequence: the 4-point EPnP RANSAC with
// Refine that Tracking::Relocalization (src/Tracking.cc:2256-2309) polls five iterations at a time.  The inlier count of EVERY iteration
// 1 .. end is evaluated in parallel (the sampler is counter-based, so no solver state is carried), then one workgroup per problem replays
// the sequential part of iterate() as a pure function of those counts.
//   k_pnp_prepare       per correspondence: x y z u v and mvMaxError = sigma2 * th2 (f32)
//   k_pnp_hypotheses    one lane per (problem, iteration): sample -> 4-point EPnP (sd_pnp_math.h, sums in the reference's order) -> mRi, mti
//                       in f64.  The 12 x 12 M^T M and its V live in LDS, element k of lane l at [k * 64 + l] (conflict-free).
//   k_pnp_count         correspondences staged once per chunk in LDS; one wave counts one hypothesis with ballot / popcount
//   k_pnp_refine        one workgroup per problem: walks the prefix maxima of the counts in order, runs Refine() -- the n-point EPnP with
//                       fixed-order tree sums, CheckInliers, count > min_inliers -- once per distinct best, writes the record and the mask
//   k_pnp_gather / k_pnp_handover   the relocalisation chain (sd_batch_relocalize_pnp): the problem from the BoW row, and the row and pose
//                       for the cascade of k_reloc.h (at the end of this file)
// All arithmetic is sd_pnp_math.h's, shared with the CPU oracle (tests/cpp/pnp_oracle.cpp).  No atomic; every output word has one writer;
// a problem's bytes do not depend on what shares its launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sd_pnp_math.h"
#include "k_area.h"

#define SD_PNP_CHUNK 1024            // correspondences staged in LDS at a time (6 floats each, 24 KB)
#define SD_PNP_HYP_PER_BLOCK 32      // hypotheses one workgroup of k_pnp_count counts over its staged correspondences
#define SD_PNP_MAX_N 4096            // == SD_PNP_MAX_CORRESPONDENCES
#define SD_PNP_MAX_ITS 4096          // == SD_PNP_MAX_ITERATIONS
#define SD_PNP_HYP_LDS (2 * 144 * 64 * 8)      // k_pnp_hypotheses: W and V of 64 lanes

// what the kernels read per problem: the caller's record plus where its rows live
struct SdPnpProb {
    sd_pnp_problem P;
    int c0, n;                // correspondences [c0, c0 + n)
    int end;                  // iterations 1 .. end are evaluated: max(maxIts, start + n_iterations), or 0 when N < mRansacMinInliers
    int h0;                   // first row of the problem's hypotheses / counts in the workspace
    int minInliers;           // mRansacMinInliers after SetRansacParameters
    int maxIts;               // mRansacMaxIts after SetRansacParameters
    float th2;
    int pad;
};
struct SdPnpPt { float x, y, z, u, v, e; };        // 24 bytes: mvP3Dw, mvP2D, mvMaxError (sdpnp::PointSet's row)
struct SdPnpHyp { double R[9], t[3]; };            // 96 bytes: mRi, mti

struct SdPnpArgs {
    const SdPnpProb* prob;
    const sd_pnp_corr* corr;
    SdPnpPt* pts;             // [correspondence]
    SdPnpHyp* hyp;            // [h0 + iteration - 1]
    int* count;               // [h0 + iteration - 1] mnInliersi
    sd_pnp_result* result;    // [problem]
    uint8_t* inlier;          // [correspondence]
};

namespace sdpnp {

// 144 doubles of one lane, interleaved with the other 63 lanes' in LDS
struct LaneView {
    double* p;
    __device__ __forceinline__ double& operator[](int i) const { return p[i * 64]; }
};

// The refine kernel's order of a sum (sd_pnp_math.h: TreeCtx restates it for the CPU): 256 leaves = threads, items strided by 256,
// shuffle tree inside each wave, then (w0 + w1) + (w2 + w3).
struct BlockCtx {
    PointSet set;
    double (*red)[12];        // [4][12] in LDS
    int tid;
    __device__ __forceinline__ int n() const { return set.count; }
    __device__ __forceinline__ void point(int i, double* pw, double* uv) const { set.get(i, pw, uv); }
    __device__ __forceinline__ bool leader() const { return tid == 0; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    template <int K, class F>
    __device__ __forceinline__ void sum(int count, F f, double* out) const
    {
        double acc[K], v[K];
#pragma unroll
        for (int k = 0; k < K; k++) acc[k] = 0;
        for (int i = tid; i < count; i += SD_PNP_LEAVES) {
            f(i, v);
#pragma unroll
            for (int k = 0; k < K; k++) acc[k] += v[k];
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
            for (int k = 0; k < K; k++) acc[k] += __shfl_down(acc[k], s, 64);
        if ((tid & 63) == 0)
#pragma unroll
            for (int k = 0; k < K; k++) red[tid >> 6][k] = acc[k];
        __syncthreads();
        if (tid == 0)
#pragma unroll
            for (int k = 0; k < K; k++) out[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        __syncthreads();
    }
};

}  // namespace sdpnp

// grid (blocks over the largest problem, problems)
__global__ void __launch_bounds__(256) k_pnp_prepare(SdPnpArgs A)
{
    const SdPnpProb& Q = A.prob[blockIdx.y];
    const int n = Q.n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const sd_pnp_corr c = A.corr[(size_t)Q.c0 + i];
        SdPnpPt p;
        p.x = c.xw[0]; p.y = c.xw[1]; p.z = c.xw[2]; p.u = c.uv[0]; p.v = c.uv[1];
        p.e = c.sigma2 * Q.th2;                                       // mvMaxError (PnP:154-156)
        A.pts[(size_t)Q.c0 + i] = p;
    }
}

// grid (ceil(largest end / 64), problems), 64 threads, SD_PNP_HYP_LDS bytes of dynamic LDS: lane = one iteration
__global__ void __launch_bounds__(64) k_pnp_hypotheses(SdPnpArgs A)
{
    extern __shared__ __align__(16) double pnp_wv[];
    const SdPnpProb& Q = A.prob[blockIdx.y];
    const int it = blockIdx.x * 64 + threadIdx.x + 1;                 // mnIterations after the increment (PnP:185)
    if (it > Q.end) return;
    int idx[4];
    sdpnp::sample4(Q.P.seed, it, Q.n, idx);
    sdpnp::SeqCtx ctx;
    ctx.set.pts = (const float*)(A.pts + (size_t)Q.c0); ctx.set.index = idx; ctx.set.count = 4;
    const sdpnp::LaneView W = {pnp_wv + threadIdx.x}, V = {pnp_wv + 144 * 64 + threadIdx.x};
    const sdpnp::Camera cam = {(double)Q.P.fx, (double)Q.P.fy, (double)Q.P.cx, (double)Q.P.cy};
    sdpnp::State S;
    sdpnp::compute_pose(ctx, S, W, V, cam);
    SdPnpHyp H;
#pragma unroll
    for (int k = 0; k < 9; k++) H.R[k] = S.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) H.t[k] = S.t[k];
    A.hyp[(size_t)Q.h0 + it - 1] = H;
}

// grid (ceil(largest end / SD_PNP_HYP_PER_BLOCK), problems), 256 threads.  The workgroup stages the problem's correspondences chunk by
// chunk (component-major, rows one float apart from a bank multiple) and each of its four waves counts SD_PNP_HYP_PER_BLOCK / 4
// hypotheses over every chunk: lane = correspondence, ballot + popcount, wave-uniform running count.
__global__ void __launch_bounds__(256) k_pnp_count(SdPnpArgs A)
{
    constexpr int STRIDE = SD_PNP_CHUNK + 1, PER_WAVE = SD_PNP_HYP_PER_BLOCK / 4;
    __shared__ float sm[6 * STRIDE];
    const SdPnpProb& Q = A.prob[blockIdx.y];
    const int first = blockIdx.x * SD_PNP_HYP_PER_BLOCK;             // 0-based hypothesis rows of this workgroup
    if (first >= Q.end) return;                                       // uniform over the workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double fu = Q.P.fx, fv = Q.P.fy, uc = Q.P.cx, vc = Q.P.cy;
    int cnt[PER_WAVE];
#pragma unroll
    for (int k = 0; k < PER_WAVE; k++) cnt[k] = 0;
    const int n = Q.n;
    for (int c0 = 0; c0 < n; c0 += SD_PNP_CHUNK) {
        const int m = min(SD_PNP_CHUNK, n - c0);
        const float* __restrict__ src = (const float*)(A.pts + (size_t)Q.c0 + c0);
        __syncthreads();                                              // the previous chunk's readers are done
        for (int e = tid; e < m * 6; e += 256) sm[(e % 6) * STRIDE + e / 6] = src[e];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER_WAVE; k++) {
            const int h = first + wave * PER_WAVE + k;
            if (h < Q.end) {                                          // uniform over the wave
                const SdPnpHyp* __restrict__ H = A.hyp + (size_t)Q.h0 + h;
                for (int i = lane; i < ((m + 63) & ~63); i += 64) {
                    bool in = false;
                    if (i < m)
                        in = sdpnp::check_inlier(H->R, H->t, sm[i], sm[STRIDE + i], sm[2 * STRIDE + i], sm[3 * STRIDE + i], sm[4 * STRIDE + i],
                                                 fu, fv, uc, vc, sm[5 * STRIDE + i]);
                    cnt[k] += __popcll(__ballot(in));
                }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < PER_WAVE; k++) {
            const int h = first + wave * PER_WAVE + k;
            if (h < Q.end) A.count[(size_t)Q.h0 + h] = cnt[k];
        }
    }
}

// One workgroup (256 threads) per problem: iterate()'s sequential part (PnP:209-257) over the counts c[1 .. end].
//   thread 0 scans the counts in order, keeping mnBestInliers / its iteration b (strict >, PnP:212), and stops at the next iteration
//   it > start with c[it] >= min_inliers whose b has not already failed Refine in this call;
//   the workgroup then rebuilds the mask of hypothesis b (ordered compaction), runs Refine (PnP:260-305) and either returns or goes on.
__global__ void __launch_bounds__(256) k_pnp_refine(SdPnpArgs A)
{
    __shared__ sdpnp::State S;
    __shared__ double s_W[144], s_V[144], s_red[4][12];
    __shared__ int s_cnt[SD_PNP_MAX_ITS], s_list[SD_PNP_MAX_N];
    __shared__ uint8_t s_mask[SD_PNP_MAX_N];
    __shared__ int s_w[4], s_it, s_b, s_best;
    const SdPnpProb& Q = A.prob[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = Q.n, end = Q.end, minI = Q.minInliers, start = Q.P.start_iteration;
    const double fu = Q.P.fx, fv = Q.P.fy, uc = Q.P.cx, vc = Q.P.cy;
    const SdPnpPt* __restrict__ pts = A.pts + (size_t)Q.c0;
    sd_pnp_result* R = A.result + blockIdx.x;
    for (int i = tid; i < end; i += 256) s_cnt[i] = A.count[(size_t)Q.h0 + i];
    __syncthreads();
    int pos = 1, best = 0, bIt = 0, lastFail = 0, nRefines = 0;       // thread 0's walk; nRefines is uniform
    for (;;) {
        if (tid == 0) {
            int stop = 0;
            for (int it = pos; it <= end; it++) {
                const int c = s_cnt[it - 1];
                if (c >= minI) {
                    if (c > best) { best = c; bIt = it; }
                    if (it > start && bIt != lastFail) { stop = it; break; }
                }
            }
            s_it = stop; s_b = bIt; s_best = best;
        }
        __syncthreads();
        const int it = s_it, b = s_b;
        if (it == 0) break;
        // mvbBestInliers: the mask of hypothesis b, and vIndices (PnP:262-271) in ascending order
        const SdPnpHyp* __restrict__ H = A.hyp + (size_t)Q.h0 + b - 1;
        int running = 0;
        for (int base = 0; base < N; base += 256) {
            const int i = base + tid;
            bool in = false;
            if (i < N) { const SdPnpPt p = pts[i]; in = sdpnp::check_inlier(H->R, H->t, p.x, p.y, p.z, p.u, p.v, fu, fv, uc, vc, p.e); }
            const unsigned long long bal = __ballot(in);
            if (lane == 0) s_w[wave] = __popcll(bal);
            __syncthreads();
            int off = running;
            for (int w = 0; w < wave; w++) off += s_w[w];
            if (in) s_list[off + __popcll(bal & ((1ull << lane) - 1ull))] = i;
            running += (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
            __syncthreads();
        }
        sdpnp::BlockCtx ctx;
        ctx.set.pts = (const float*)pts; ctx.set.index = s_list; ctx.set.count = running; ctx.red = s_red; ctx.tid = tid;
        const sdpnp::Camera cam = {fu, fv, uc, vc};
        sdpnp::compute_pose(ctx, S, s_W, s_V, cam);
        nRefines++;
        // CheckInliers on the refined pose (PnP:287-290)
        int cnt = 0;
        for (int base = 0; base < N; base += 256) {
            const int i = base + tid;
            bool in = false;
            if (i < N) {
                const SdPnpPt p = pts[i];
                in = sdpnp::check_inlier(S.R, S.t, p.x, p.y, p.z, p.u, p.v, fu, fv, uc, vc, p.e);
                s_mask[i] = in ? 1 : 0;
            }
            cnt += __popcll(__ballot(in));
        }
        if (lane == 0) s_w[wave] = cnt;
        __syncthreads();
        const int refined = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        if (refined > minI) {                                         // PnP:292, strict
            for (int i = tid; i < N; i += 256) A.inlier[(size_t)Q.c0 + i] = s_mask[i];
            if (tid < 16) {
                const int r = tid >> 2, c = tid & 3;
                R->Tcw[tid] = r == 3 ? (c == 3 ? 1.f : 0.f) : (c == 3 ? (float)S.t[r] : (float)S.R[3 * r + c]);
            }
            if (tid == 0) {
                R->kind = 1; R->no_more = 0; R->iteration = it; R->n_inliers = refined; R->best_iteration = b; R->best_inliers = s_best;
                R->n_refines = nRefines; R->min_inliers = minI; R->max_its = Q.maxIts; R->reserved = 0;
            }
            return;
        }
        __syncthreads();                                              // s_w, s_it are rewritten by the next round
        if (tid == 0) { lastFail = b; pos = it + 1; }
    }
    // PnP:241-257: nothing refined.  mnIterations >= mRansacMaxIts holds by construction of `end`
    const int b = s_b, bestCount = s_best;
    const bool have = b > 0;                                          // mnBestInliers >= mRansacMinInliers
    const SdPnpHyp* __restrict__ H = A.hyp + (size_t)Q.h0 + (have ? b - 1 : 0);
    for (int i = tid; i < N; i += 256) {
        bool in = false;
        if (have) { const SdPnpPt p = pts[i]; in = sdpnp::check_inlier(H->R, H->t, p.x, p.y, p.z, p.u, p.v, fu, fv, uc, vc, p.e); }
        A.inlier[(size_t)Q.c0 + i] = in ? 1 : 0;
    }
    if (tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        float v = 0.f;
        if (have) v = r == 3 ? (c == 3 ? 1.f : 0.f) : (c == 3 ? (float)H->t[r] : (float)H->R[3 * r + c]);
        R->Tcw[tid] = v;
    }
    if (tid == 0) {
        R->kind = have ? 2 : 0; R->no_more = 1; R->iteration = end; R->n_inliers = have ? bestCount : 0;
        R->best_iteration = b; R->best_inliers = bestCount; R->n_refines = nRefines; R->min_inliers = minI; R->max_its = Q.maxIts;
        R->reserved = 0;
    }
}

// the debug copy of the counts and hypotheses (either may be null): grid (blocks over the largest end, problems); row p gets iterations 1 .. end
__global__ void __launch_bounds__(256) k_pnp_copy_counts(SdPnpArgs A, int* __restrict__ out, double* __restrict__ poses, int stride)
{
    const SdPnpProb& Q = A.prob[blockIdx.y];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < Q.end; i += gridDim.x * 256) {
        const size_t o = (size_t)blockIdx.y * stride + i;
        if (out) out[o] = A.count[(size_t)Q.h0 + i];
        if (poses) {
            const SdPnpHyp H = A.hyp[(size_t)Q.h0 + i];
            for (int k = 0; k < 9; k++) poses[o * 12 + k] = H.R[k];
            for (int k = 0; k < 3; k++) poses[o * 12 + 9 + k] = H.t[k];
        }
    }
}

// ---------------------------------------------------------------- the relocalisation chain (sd_batch_relocalize_pnp, sd_pnp.inc)
// Rows are [job][cap]: job j owns correspondences and hypotheses at fixed strides, so nothing about a job depends on its neighbours.
struct SdPnpChainArgs {
    const sd_keypoint* kp;          // mvKeysUn, [slot][cap]
    const int* count;               // key points per slot
    const int2* slots;              // (frame slot, keyframe slot) per job
    const int* match;               // [job][cap] vvpMapPointMatches: point index or -1 per frame key point
    const SdMapPoint* mps; int nPoints, cap;
    const sd_pnp_problem* in;       // [job] the caller's record
    const int2* table;              // [cap + 1] (mRansacMinInliers, mRansacMaxIts) of SetRansacParameters for every N, made on the host
    sd_pnp_corr* corr;              // [job][cap]
    SdPnpProb* prob;                // [job]
    float th2; int endCap;          // hypotheses per job in the workspace
    int* row; float* T;             // the hand-over: [job][cap] mvpMapPoints, [job][16] Tcw
    const sd_pnp_result* result; const uint8_t* inlier;
};

// The constructor's gather (PnP:79-101) for one job per workgroup: frame key points in index order, kept when the match names a point of
// the table whose good flag is set (bit 0, as the reloc matcher reads it); ordered ballot compaction.  Then the job's problem row: N is
// known here, its SetRansacParameters values are read from the host-made table.
__global__ void __launch_bounds__(256) k_pnp_gather(SdPnpChainArgs A, SdLevelTables L)
{
    __shared__ int s_w[4];
    const int job = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = A.slots[job].x;
    const int N2 = min(A.count[slot], A.cap);
    const size_t r0 = (size_t)job * A.cap;
    const sd_keypoint* __restrict__ kp = A.kp + (size_t)slot * A.cap;
    int running = 0;
    for (int base = 0; base < N2; base += 256) {
        const int i = base + tid;
        int m = -1;
        if (i < N2) m = A.match[r0 + i];
        const bool keep = m >= 0 && m < A.nPoints && (A.mps[m].flags & 1u);
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int off = running;
        for (int w = 0; w < wave; w++) off += s_w[w];
        if (keep) {
            const sd_keypoint k = kp[i];
            const SdMapPoint mp = A.mps[m];
            sd_pnp_corr c;
            c.xw[0] = mp.xw[0]; c.xw[1] = mp.xw[1]; c.xw[2] = mp.xw[2]; c.uv[0] = k.x; c.uv[1] = k.y;
            c.sigma2 = L.sigma2[min(max(k.octave, 0), SD_MAX_LEVELS - 1)]; c.tag = i;
            A.corr[r0 + off + __popcll(bal & ((1ull << lane) - 1ull))] = c;
        }
        running += (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        __syncthreads();
    }
    if (tid == 0) {
        SdPnpProb q;
        q.P = A.in[job]; q.c0 = (int)r0; q.n = running; q.h0 = job * A.endCap; q.th2 = A.th2; q.pad = 0;
        const int2 t = A.table[running];
        q.minInliers = t.x; q.maxIts = t.y;
        q.end = running < t.x ? 0 : min(max(t.y, q.P.start_iteration + q.P.n_iterations), A.endCap);
        A.prob[job] = q;
    }
}

// Tracking.cc:2300-2309 for one job per workgroup: mvpMapPoints[i] = the match where vbInliers[i], else NULL; and the pose for the cascade.
// A job of kind 0 has no inlier: its row is all -1, so the cascade builds no edge for it and every later step is off.  A match outside
// [-1, nPoints) is passed through, so that the cascade's own range check reports it.
__global__ void __launch_bounds__(256) k_pnp_handover(SdPnpChainArgs A)
{
    const int job = blockIdx.x, tid = threadIdx.x;
    const size_t r0 = (size_t)job * A.cap;
    const int N2 = min(A.count[A.slots[job].x], A.cap);
    for (int i = tid; i < A.cap; i += 256) {
        const int m = i < N2 ? A.match[r0 + i] : -1;
        A.row[r0 + i] = (m < -1 || m >= A.nPoints) ? m : -1;
    }
    __syncthreads();
    const int n = A.prob[job].n;
    for (int e = tid; e < n; e += 256)
        if (A.inlier[r0 + e]) { const int i = A.corr[r0 + e].tag; A.row[r0 + i] = A.match[r0 + i]; }
    if (tid < 16) A.T[job * 16 + tid] = A.result[job].Tcw[tid];
}
