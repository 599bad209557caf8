// LoopClosing::ComputeSim3 after the RANSAC (src/LoopClosing.cc:312-340) for many (keyframe, candidate) jobs without a host round
// trip: the kernels around the existing k_sim3_mark / k_sim3_search / k_sim3_agree (k_sim3.h) and k_sim3_optimize (k_sim3_opt.h).
//   k_refine_begin    per job: vpMapPointMatches[i1] = vbInliers ? the BoW match : NULL (:314-319) as a matched12 row, and the pair
//                     record of SearchBySim3 from the RANSAC's R12 / t12 / s12 (the statement sd_batch_search_by_sim3 makes on the host)
//   k_refine_build    per job: the pairs SearchBySim3 added are merged (ORBmatcher.cc:1476), then one correspondence per i1 that passes
//                     Optimizer.cc:1101-1136, compacted in i1 order by a ballot prefix, and the optimiser's problem record
//   k_refine_finish   per job: the final vpMapPointMatches per KF1 feature, matched = ret >= 20, Scw = gScm * gSmw in f64 (:330-334)
// A job whose RANSAC found nothing does not run: its pair is skipped by the search, it gets no correspondence, the optimiser answers 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_sim3.h"
#include "k_sim3_opt.h"

struct SdRefineJob { float T1[16], T2[16]; int slot1, slot2, c0, nc; };      // poses, slots, the job's rows [c0, c0 + nc) of the RANSAC's correspondences

struct SdRefineArgs {
    const SdRefineJob* jobs;
    const sd_sim3_result* ransac;          // [job]
    const sd_sim3_corr* rcorr;             // the RANSAC's correspondences (tag = i1) and its inlier bytes
    const uint8_t* inlier;
    const int* bow12;                      // [job][cap] the BoW matches: idx2, -2 (not in KF2) or -1 (NULL)
    const int* kfPoint[2];                 // [job][cap] GetMapPointMatches() as point indices, -1 = NULL or bad
    const SdMapPoint* mps; int nPoints;
    const sd_keypoint* kp; const int* count;
    SdSim3Pair* pairs;                     // out: SearchBySim3's pair table
    int* merged12;                         // [job][cap] out of begin: SearchBySim3's vpMatches12
    const int* add12;                      // [job][cap] what SearchBySim3 added
    sd_sim3_opt_corr* ocorr; SdSim3OptProb* oprob; const sd_sim3_opt_result* ores; const uint8_t* ostate;
    int* final12;                          // [job][cap]
    sd_sim3_refine_result* out;
    float invSigma2[SD_MAX_LEVELS];
    float fx, fy, cx, cy, th2;
    int fixScale, cap;
};

__global__ void __launch_bounds__(256) k_refine_begin(SdRefineArgs A)
{
    const int job = blockIdx.x, tid = threadIdx.x;
    const SdRefineJob& J = A.jobs[job];
    const sd_sim3_result& R = A.ransac[job];
    const bool run = R.found != 0;
    const size_t row = (size_t)job * A.cap;
    for (int i = tid; i < A.cap; i += 256) A.merged12[row + i] = -1;
    __syncthreads();
    if (run)
        for (int e = tid; e < J.nc; e += 256) {                          // tags are distinct: one writer per entry
            const int i1 = A.rcorr[(size_t)J.c0 + e].tag;
            if (A.inlier[(size_t)J.c0 + e] && i1 >= 0 && i1 < A.cap) A.merged12[row + i1] = A.bow12[row + i1];
        }
    if (tid == 0) {                                                      // ORBmatcher.cc:1276-1278 as DESIGN Q39 freezes it
        SdSim3Pair P;
        const float sc = R.s12;
        const double inv = 1.0 / (double)sc;
        float sR21[3][3];
        for (int i = 0; i < 16; i++) { P.T1[i] = J.T1[i]; P.T2[i] = J.T2[i]; }
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) { P.T12[4 * i + j] = sc * R.R12[3 * i + j]; sR21[i][j] = (float)(inv * (double)R.R12[3 * j + i]); P.T21[4 * i + j] = sR21[i][j]; }
            P.T12[4 * i + 3] = R.t12[i];
        }
        for (int i = 0; i < 3; i++) { float a = (-sR21[i][0]) * R.t12[0] + (-sR21[i][1]) * R.t12[1]; P.T21[4 * i + 3] = a + (-sR21[i][2]) * R.t12[2]; }
        for (int j = 0; j < 3; j++) { P.T12[12 + j] = 0.f; P.T21[12 + j] = 0.f; }
        P.T12[15] = 1.f; P.T21[15] = 1.f;
        P.slot1 = J.slot1; P.slot2 = J.slot2; P.pad[0] = run ? 0 : 1; P.pad[1] = 0;
        A.pairs[job] = P;
    }
}

// vpMapPointMatches[i1] after SearchBySim3's additions, in matched12's encoding
__device__ __forceinline__ int sd_refine_match(const SdRefineArgs& A, size_t row, int i1)
{
    const int add = A.add12[row + i1];
    return add >= 0 ? add : A.merged12[row + i1];
}

__global__ void __launch_bounds__(256) k_refine_build(SdRefineArgs A)
{
    __shared__ int wsum[4];
    const int job = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SdRefineJob& J = A.jobs[job];
    const sd_sim3_result& R = A.ransac[job];
    const bool run = R.found != 0;
    const size_t row = (size_t)job * A.cap;
    const int N1 = A.count[J.slot1], N2 = A.count[J.slot2];
    const size_t kp1 = (size_t)J.slot1 * A.cap, kp2 = (size_t)J.slot2 * A.cap;
    int base = 0;
    if (run)
        for (int c = 0; c < N1; c += 256) {
            const int i1 = c + tid;
            int i2 = -1, p1 = -1, p2 = -1;
            if (i1 < N1) {
                i2 = sd_refine_match(A, row, i1);                        // -1: vpMatches1[i] NULL; -2 or beyond N2: i2 < 0 (:1114)
                p1 = A.kfPoint[0][row + i1];
                if (i2 >= 0 && i2 < N2) p2 = A.kfPoint[1][row + i2];
            }
            const bool pred = p1 >= 0 && p1 < A.nPoints && p2 >= 0 && p2 < A.nPoints;
            const unsigned long long bal = __ballot(pred);
            const int pre = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) wsum[wave] = __popcll(bal);
            __syncthreads();
            int off = base, tot = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) { if (w < wave) off += wsum[w]; tot += wsum[w]; }
            if (pred) {
                const sd_keypoint k1 = A.kp[kp1 + i1], k2 = A.kp[kp2 + i2];
                float w1 = 0.f, w2 = 0.f;
#pragma unroll
                for (int l = 0; l < SD_MAX_LEVELS; l++) { if (k1.octave == l) w1 = A.invSigma2[l]; if (k2.octave == l) w2 = A.invSigma2[l]; }
                sd_sim3_opt_corr o;
                const SdMapPoint a = A.mps[p1], b = A.mps[p2];
                o.xw1[0] = a.xw[0]; o.xw1[1] = a.xw[1]; o.xw1[2] = a.xw[2]; o.xw2[0] = b.xw[0]; o.xw2[1] = b.xw[1]; o.xw2[2] = b.xw[2];
                o.obs1[0] = k1.x; o.obs1[1] = k1.y; o.obs2[0] = k2.x; o.obs2[1] = k2.y;
                o.inv_sigma2_1 = w1; o.inv_sigma2_2 = w2; o.tag = i1;
                A.ocorr[row + off + pre] = o;
            }
            __syncthreads();
            base += tot;
        }
    if (tid == 0) {
        SdSim3OptProb Q;
        for (int i = 0; i < 16; i++) { Q.P.Tcw1[i] = J.T1[i]; Q.P.Tcw2[i] = J.T2[i]; }
        Q.P.fx1 = A.fx; Q.P.fy1 = A.fy; Q.P.cx1 = A.cx; Q.P.cy1 = A.cy; Q.P.fx2 = A.fx; Q.P.fy2 = A.fy; Q.P.cx2 = A.cx; Q.P.cy2 = A.cy;
        for (int i = 0; i < 9; i++) Q.P.R12[i] = R.R12[i];
        for (int i = 0; i < 3; i++) Q.P.t12[i] = R.t12[i];
        Q.P.s12 = R.s12; Q.P.th2 = A.th2; Q.P.fix_scale = A.fixScale;
        Q.c0 = (int)row; Q.n = base;
        A.oprob[job] = Q;
    }
}

__global__ void __launch_bounds__(256) k_refine_finish(SdRefineArgs A)
{
    const int job = blockIdx.x, tid = threadIdx.x;
    const SdRefineJob& J = A.jobs[job];
    const bool run = A.ransac[job].found != 0;
    const size_t row = (size_t)job * A.cap;
    const int N1 = A.count[J.slot1];
    const sd_sim3_opt_result O = A.ores[job];
    for (int i = tid; i < A.cap; i += 256) A.final12[row + i] = (run && i < N1) ? sd_refine_match(A, row, i) : -1;
    __syncthreads();
    for (int k = tid; k < O.n_correspondences; k += 256)                 // both checks set vpMatches1[idx] = NULL, also on the `return 0` path
        if (A.ostate[row + k]) A.final12[row + A.ocorr[row + k].tag] = -1;
    if (tid == 0) {
        sd_sim3_refine_result r;
        r.ran = run ? 1 : 0; r.matched = (run && O.ret >= 20) ? 1 : 0; r.n_built = O.n_correspondences; r.reserved = 0;
        // g2o::Sim3 gSmw(Converter::toMatrix3d(pKF->GetRotation()), Converter::toVector3d(pKF->GetTranslation()), 1.0); mg2oScw = gScm * gSmw
        sd_s3 gScm, gSmw;
        gScm.r.x = O.q[0]; gScm.r.y = O.q[1]; gScm.r.z = O.q[2]; gScm.r.w = O.q[3]; gScm.t0 = O.t[0]; gScm.t1 = O.t[1]; gScm.t2 = O.t[2]; gScm.s = O.s;
        double Rm[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Rm[i][j] = (double)J.T2[4 * i + j];
        gSmw.r = sd_quat_of(Rm);
        gSmw.t0 = (double)J.T2[3]; gSmw.t1 = (double)J.T2[7]; gSmw.t2 = (double)J.T2[11]; gSmw.s = 1.0;
        const sd_s3 S = sd_s3_mul(gScm, gSmw);
        r.Scw_q[0] = S.r.x; r.Scw_q[1] = S.r.y; r.Scw_q[2] = S.r.z; r.Scw_q[3] = S.r.w; r.Scw_t[0] = S.t0; r.Scw_t[1] = S.t1; r.Scw_t[2] = S.t2; r.Scw_s = S.s;
        double Rq[3][3];
        sd_quat_matrix(S.r, Rq);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) r.Scw[i * 4 + j] = (float)(S.s * Rq[i][j]);            // Converter::toCvMat(g2o::Sim3)
        r.Scw[3] = (float)S.t0; r.Scw[7] = (float)S.t1; r.Scw[11] = (float)S.t2;
        r.Scw[12] = 0.f; r.Scw[13] = 0.f; r.Scw[14] = 0.f; r.Scw[15] = 1.f;
        r.opt = O;
        A.out[job] = r;
    }
}
