// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778) from initializeOptimization() on, with the vendored g2o's Levenberg-Marquardt
// over BlockSolver_6_3 (Schur complement on the landmarks), and MapPoint::UpdateNormalAndDepth for the optimised points; DESIGN Q32-Q38.
// One 256-thread workgroup per problem runs both rounds (optimize(5) with Huber, classification, optimize(10) without) and every LM trial
// on the device; no host synchronisation, no grid barrier, no floating-point atomic.  f64 throughout; inputs f32 as the reference's.
//
// Per linearisation every active edge writes one 54-double record (its terms of Hpp, bp, Hll, bl and its 6x3 block of Hpl) to the
// workspace; the per-vertex blocks are GATHERED from the records over index lists built once per call (edges of a keyframe, edges of a
// point, both in insertion order): a wave per pose block (lanes stride the list, wave64 xor-butterfly), a lane per point (sequential).
// Per LM trial: Hll + lambda inverted per point, the reduced camera system S = Hpp + lambda - sum Hpl Hll^-1 Hpl^T assembled a block row
// per wave in LDS (the edges of the row's keyframe in list order, then the edges of each edge's point), stored to the workspace, factorised
// by a right-looking blocked LDL^T (SD_BA_NB-wide panels: diagonal tile and panel in LDS, trailing update from LDS), solved blocked
// through the same tile, and the points back-substituted a lane each.  Every sum has a fixed order, and every decision is taken on values
// that all lanes hold with the same bits, so a problem's result is bit-identical run to run and does not depend on the launch it shares.
//
// Caps (SD_BA_MAX_* below; checked by the host entry points before anything is launched; nothing is ever truncated).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sd_frontend.h"
#include "k_pose.h"

#define SD_BA_THREADS 256
#define SD_BA_NB 48                 // panel width of the blocked LDL^T (8 pose blocks)
#define SD_BA_MAX_LOCAL 64          // local keyframes per problem (S is at most 384 x 384)
#define SD_BA_MAX_FIXED 128         // fixed cameras per problem
#define SD_BA_MAX_POINTS 8192
#define SD_BA_MAX_EDGES 65536
#define SD_BA_REC 54                // doubles per edge record: Hpp 21 (lower), bp 6, Hll 6 (lower), bl 3, Hpl 18 (6 x 3 row-major)
#define SD_BA_PHASES 6               // index lists, linearisation (records + gathers), Schur assembly, factorisation, solves, update + chi2
#define SD_BA_TP (SD_BA_NB + 1)     // LDS pitch of the tile and the panel: consecutive rows fall on different banks

struct SdBaProblem { int kf0, nKF, nLocal, pt0, nPt, e0, nE, pad; unsigned long long wsD, wsI; };   // workspace offsets in doubles / ints

static inline size_t sd_ba_ws_doubles(size_t nKF, size_t nL, size_t nPt, size_t nE)
{
    return 17 * nKF + 24 * nPt + 54 * nL + 36 * nL * nL + (SD_BA_REC + 1) * nE;
}
static inline size_t sd_ba_ws_ints(size_t nKF, size_t nL, size_t nPt, size_t nE) { return (3 * nKF + 1) + nL + (3 * nPt + 1) + 3 * nE + 8; }
// dynamic LDS in bytes for a launch whose largest problem has nL local keyframes
static inline size_t sd_ba_lds_bytes(size_t nL)
{
    const size_t n6 = 6 * nL, panel = n6 > SD_BA_NB ? (n6 - SD_BA_NB) * SD_BA_TP : 0, rows = 4 * 6 * n6;
    return 8 * (4 * 28 + 6 * SD_BA_MAX_LOCAL + 2 * SD_BA_NB + SD_BA_NB * SD_BA_TP + (panel > rows ? panel : rows) + 8);
}

struct SdBaArgs {
    const SdBaProblem* prob;
    const sd_ba_keyframe* kfs; const float* xw; const sd_ba_edge* edges; const int* refKf;
    float* Tcw; float* xwOut; float* normal; float* dist; uint8_t* level1; uint8_t* erase; sd_ba_stats* stats;
    double* wsD; int* wsI;
    long long* prof;          // nullable: [problem][SD_BA_PHASES] wall-clock ticks per phase (profiling)
};

// profiling: thread 0 adds the ticks since the last mark to phase ph (after a barrier, so the phase is complete)
#define SD_BA_MARK(ph) do { if (A.prof) { __syncthreads(); if (tid == 0) { const long long t_ = wall_clock64(); A.prof[(size_t)blockIdx.x * SD_BA_PHASES + (ph)] += t_ - profT; profT = t_; } } } while (0)

namespace sdba {
using sdpose::T;
typedef sd_se3_cam Cam;

__device__ __forceinline__ T load_pose(const double* p) { T s; s.r.x = p[0]; s.r.y = p[1]; s.r.z = p[2]; s.r.w = p[3]; s.t0 = p[4]; s.t1 = p[5]; s.t2 = p[6]; return s; }
__device__ __forceinline__ void store_pose(double* p, const T& s) { p[0] = s.r.x; p[1] = s.r.y; p[2] = s.r.z; p[3] = s.r.w; p[4] = s.t0; p[5] = s.t1; p[6] = s.t2; }

// computeError of either two-vertex edge at the stored pose and point
__device__ __forceinline__ int err(const sd_ba_edge& E, const Cam& c, const double* pose, const double* X, double (&r)[3], double (&p)[3])
{
    return sd_se3_error(load_pose(pose), c, X[0], X[1], X[2], E.u, E.v, E.ur, r, p);
}
__device__ __forceinline__ Cam cam_of(const sd_ba_keyframe& k) { return {(double)k.fx, (double)k.fy, (double)k.cx, (double)k.cy, (double)k.mbf}; }

// Eigen's 3x3 inverse (cofactors over the determinant) of the symmetric m = [m00 m10 m11 m20 m21 m22]; the result is symmetric too
__device__ __forceinline__ void inverse3(const double (&m)[6], double (&o)[6])
{
    const double m00 = m[0], m10 = m[1], m11 = m[2], m20 = m[3], m21 = m[4], m22 = m[5];
    const double c00 = m11 * m22 - m21 * m21, c10 = m21 * m20 - m10 * m22, c20 = m10 * m21 - m11 * m20;
    const double c11 = m22 * m00 - m20 * m20, c21 = m20 * m10 - m21 * m00, c22 = m00 * m11 - m10 * m10;
    const double det = (c00 * m00 + c10 * m10) + c20 * m20, id = 1.0 / det;
    o[0] = c00 * id; o[1] = c10 * id; o[2] = c11 * id; o[3] = c20 * id; o[4] = c21 * id; o[5] = c22 * id;
}
// orders this wave's LDS accesses across its lanes (a block row of S is written and read back by different lanes of one wave)
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// linearizeOplus + constructQuadraticForm of one edge: its record (SD_BA_REC doubles, layout above).  Kept out of line: inlined, its
// ~60 live doubles push the whole kernel into scratch.
__device__ __noinline__ void edge_record(bool robust, int D, const Cam& c, double wgt, double rho1, const double (&r)[3], const double (&p)[3],
                                         const double* pose, double* o)
{
    double R[3][3];
    sd_quat_matrix(load_pose(pose).r, R);
    const double x = p[0], y = p[1], z = p[2], z_2 = z * z;
    double Ja[3][3], Jb[3][6];
    if (D == 2) {
        const double s = -1. / z;
        const double M[2][3] = {{s * c.fx, s * 0.0, s * (-x / z * c.fx)}, {s * 0.0, s * c.fy, s * (-y / z * c.fy)}};
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) Ja[a][b] = (M[a][0] * R[0][b] + M[a][1] * R[1][b]) + M[a][2] * R[2][b];
#pragma unroll
        for (int b = 0; b < 3; b++) Ja[2][b] = 0.0;
    } else {
#pragma unroll
        for (int b = 0; b < 3; b++) {
            Ja[0][b] = -c.fx * R[0][b] / z + c.fx * x * R[2][b] / z_2;
            Ja[1][b] = -c.fy * R[1][b] / z + c.fy * y * R[2][b] / z_2;
            Ja[2][b] = Ja[0][b] - c.bf * R[2][b] / z_2;
        }
    }
    Jb[0][0] = x * y / z_2 * c.fx; Jb[0][1] = -(1 + (x * x / z_2)) * c.fx; Jb[0][2] = y / z * c.fx;
    Jb[0][3] = -1. / z * c.fx; Jb[0][4] = 0; Jb[0][5] = x / z_2 * c.fx;
    Jb[1][0] = (1 + y * y / z_2) * c.fy; Jb[1][1] = -x * y / z_2 * c.fy; Jb[1][2] = -x / z * c.fy;
    Jb[1][3] = 0; Jb[1][4] = -1. / z * c.fy; Jb[1][5] = y / z_2 * c.fy;
    if (D == 3) {
        Jb[2][0] = Jb[0][0] - c.bf * y / z_2; Jb[2][1] = Jb[0][1] + c.bf * x / z_2; Jb[2][2] = Jb[0][2];
        Jb[2][3] = Jb[0][3]; Jb[2][4] = 0; Jb[2][5] = Jb[0][5] - c.bf / z_2;
    } else {
#pragma unroll
        for (int b = 0; b < 6; b++) Jb[2][b] = 0.0;
    }
    const double wo = robust ? rho1 * wgt : wgt;
    double orr[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { orr[k] = -(wgt * r[k]); if (robust) orr[k] *= rho1; }
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b <= a; b++) {
            double h = (Jb[0][a] * wo) * Jb[0][b] + (Jb[1][a] * wo) * Jb[1][b];
            if (D == 3) h = h + (Jb[2][a] * wo) * Jb[2][b];
            o[a * (a + 1) / 2 + b] = h;
        }
#pragma unroll
    for (int a = 0; a < 6; a++) {
        double g = Jb[0][a] * orr[0] + Jb[1][a] * orr[1];
        if (D == 3) g = g + Jb[2][a] * orr[2];
        o[21 + a] = g;
    }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b <= a; b++) {
            double h = (Ja[0][a] * wo) * Ja[0][b] + (Ja[1][a] * wo) * Ja[1][b];
            if (D == 3) h = h + (Ja[2][a] * wo) * Ja[2][b];
            o[27 + a * (a + 1) / 2 + b] = h;
        }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double g = Ja[0][a] * orr[0] + Ja[1][a] * orr[1];
        if (D == 3) g = g + Ja[2][a] * orr[2];
        o[33 + a] = g;
    }
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            double h = robust ? (Jb[0][a] * wo) * Ja[0][b] + (Jb[1][a] * wo) * Ja[1][b] : Jb[0][a] * (Ja[0][b] * wgt) + Jb[1][a] * (Ja[1][b] * wgt);
            if (D == 3) h = h + (robust ? (Jb[2][a] * wo) * Ja[2][b] : Jb[2][a] * (Ja[2][b] * wgt));
            o[36 + a * 3 + b] = h;
        }
}

// One row below the diagonal tile: x (L D)^T = a against the tile in LDS; the row of L goes back to the workspace and into the panel.
__device__ __noinline__ void panel_row(double* srow, int nb, const double* Tl, const double* Dv, double* prow)
{
    double x[SD_BA_NB];
#pragma unroll
    for (int c = 0; c < SD_BA_NB; c++) x[c] = c < nb ? srow[c] : 0.0;
#pragma unroll
    for (int j = 0; j < SD_BA_NB; j++) {
        double t = x[j];
#pragma unroll
        for (int c = 0; c < j; c++) t -= (x[c] * Tl[j * SD_BA_TP + c]) * Dv[c];
        x[j] = t / Dv[j];
    }
#pragma unroll
    for (int c = 0; c < SD_BA_NB; c++) { prow[c] = x[c]; if (c < nb) srow[c] = x[c]; }
}

}  // namespace sdba

__global__ void __launch_bounds__(SD_BA_THREADS) k_local_ba(SdBaArgs A)
{
    using namespace sdba;
    extern __shared__ __align__(16) double ba_lds[];
    __shared__ int sh_i[8];
    __shared__ int sh_key[2 * SD_BA_THREADS];
    long long profT = A.prof ? wall_clock64() : 0;
    const SdBaProblem P = A.prob[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nKF = P.nKF, nL = P.nLocal, nPt = P.nPt, nE = P.nE;
    const sd_ba_keyframe* __restrict__ KF = A.kfs + P.kf0;
    const sd_ba_edge* __restrict__ E = A.edges + P.e0;
    const int* __restrict__ refKf = A.refKf + P.pt0;
    // ---- LDS
    double* red = ba_lds;                                 // 4 x 28
    double* yv = red + 4 * 28;                            // 6 x SD_BA_MAX_LOCAL: right-hand side / solution of the reduced system
    double* Lcol = yv + 6 * SD_BA_MAX_LOCAL;              // SD_BA_NB
    double* Dv = Lcol + SD_BA_NB;                         // SD_BA_NB
    double* Tl = Dv + SD_BA_NB;                           // SD_BA_NB x SD_BA_TP
    double* big = Tl + SD_BA_NB * SD_BA_TP;               // the panel, or four block rows of S
    // ---- workspace
    double* w = A.wsD + P.wsD;
    double* est = w; w += 7 * nKF;
    double* bak = w; w += 7 * nKF;
    double* Ow = w; w += 3 * nKF;
    double* X = w; w += 3 * nPt;
    double* Xbak = w; w += 3 * nPt;
    double* Hll = w; w += 6 * nPt;
    double* bl = w; w += 3 * nPt;
    double* Dinv = w; w += 6 * nPt;
    double* xl = w; w += 3 * nPt;
    double* Hpp = w; w += 36 * nL;
    double* bp = w; w += 6 * nL;
    double* xp = w; w += 6 * nL;
    double* dg = w; w += 6 * nL;
    double* S = w; w += 36 * (size_t)nL * nL;
    double* rec = w; w += (size_t)SD_BA_REC * nE;
    double* chi2c = w;
    int* wi = A.wsI + P.wsI;
    int* kfStart = wi; wi += nKF + 1;
    int* poseIdx = wi; wi += nKF;
    int* kfAct = wi; wi += nKF;
    int* poseKf = wi; wi += nL;
    int* ptStart = wi; wi += nPt + 1;
    int* ptCur = wi; wi += nPt;
    int* ptAct = wi; wi += nPt;
    int* kfList = wi; wi += nE;
    int* ptList = wi; wi += nE;
    int* level = wi;
    sd_ba_stats* st = A.stats + blockIdx.x;

    // ---- validation: an index out of range makes the problem a no-op with iterations = -1 (the host entry point never lets one through)
    int bad = 0;
    for (int i = tid; i < nE; i += SD_BA_THREADS) { const sd_ba_edge e = E[i]; if (e.kf < 0 || e.kf >= nKF || e.point < 0 || e.point >= nPt) bad = 1; }
    for (int p = tid; p < nPt; p += SD_BA_THREADS) { const int r = refKf[p]; if (r < -1 || r >= nKF) bad = 1; }
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid == 0) { sd_ba_stats z = {}; z.iterations[0] = z.iterations[1] = -1; *st = z; }
        return;
    }
    // ---- estimates: Converter::toSE3Quat(GetPose()), toVector3d(GetWorldPos())
    for (int k = tid; k < nKF; k += SD_BA_THREADS) {
        const float* Tq = KF[k].Tcw;
        // sd_se3_of(Tq), spelled out: through the call the kernel comes out 8 bytes shorter here, which moves every loop of the trial
        // off the addresses it is measured at (profiles/lm_shared_math.txt)
        const double R0[3][3] ={{Tq[0], Tq[1], Tq[2]}, {Tq[4], Tq[5], Tq[6]}, {Tq[8], Tq[9], Tq[10]}};
        T s;
        s.r = sd_quat_of(R0);
        s.t0 = Tq[3]; s.t1 = Tq[7]; s.t2 = Tq[11];
        sd_quat_renorm(s.r);
        store_pose(est + 7 * k, s);
        kfStart[k] = 0;
    }
    for (int i = tid; i < 3 * nPt; i += SD_BA_THREADS) X[i] = (double)A.xw[(size_t)P.pt0 * 3 + i];
    for (int p = tid; p < nPt; p += SD_BA_THREADS) ptCur[p] = 0;
    for (int i = tid; i < nE; i += SD_BA_THREADS) level[i] = 0;
    __syncthreads();
    // ---- index lists, insertion order: counts through integer atomics, a prefix sum, then a stable fill 256 edges at a time -- an edge's
    // slot is its list's fill so far plus the number of earlier edges of the chunk with the same key, so no list is ever sorted.
    for (int k = tid; k < nKF; k += SD_BA_THREADS) kfAct[k] = 0;
    __syncthreads();
    for (int i = tid; i < nE; i += SD_BA_THREADS) { atomicAdd(&ptCur[E[i].point], 1); atomicAdd(&kfAct[E[i].kf], 1); }
    __syncthreads();
    if (tid == 0) { int s = 0; for (int k = 0; k < nKF; k++) { kfStart[k] = s; s += kfAct[k]; } kfStart[nKF] = s; }
    if (tid == 64) { int s = 0; for (int p = 0; p < nPt; p++) { ptStart[p] = s; s += ptCur[p]; } ptStart[nPt] = s; }
    __syncthreads();
    for (int p = tid; p < nPt; p += SD_BA_THREADS) ptCur[p] = 0;
    for (int k = tid; k < nKF; k += SD_BA_THREADS) kfAct[k] = 0;
    __syncthreads();
    for (int c0 = 0; c0 < nE; c0 += SD_BA_THREADS) {
        const int i = c0 + tid, n = min(SD_BA_THREADS, nE - c0);
        const int kp = i < nE ? E[i].point : -1, kk = i < nE ? E[i].kf : -1;
        sh_key[tid] = kp; sh_key[SD_BA_THREADS + tid] = kk;
        __syncthreads();
        int rp = 0, tp = 0, rk = 0, tk = 0;
        for (int j = 0; j < n; j++) {
            const bool sp = sh_key[j] == kp, sk = sh_key[SD_BA_THREADS + j] == kk;
            tp += sp; tk += sk;
            if (j < tid) { rp += sp; rk += sk; }
        }
        if (i < nE) { ptList[ptStart[kp] + ptCur[kp] + rp] = i; kfList[kfStart[kk] + kfAct[kk] + rk] = i; }
        __syncthreads();
        if (i < nE) { if (rp == tp - 1) ptCur[kp] += tp; if (rk == tk - 1) kfAct[kk] += tk; }     // the chunk's last edge of a key
        __syncthreads();
    }
    SD_BA_MARK(0);

    const double dM = (double)(float)sqrt(5.991), dS = (double)(float)sqrt(7.815);
    int iters[2] = {0, 0}, trials[2] = {0, 0}, rejected[2] = {0, 0}, nLevel1 = 0, nErased = 0;
    double chiOut[2] = {0.0, 0.0};

    for (int round = 0; round < 2 && nE > 0; round++) {
        const bool robust = round == 0;
        const int maxIt = round == 0 ? 5 : 10;
        // ---- initializeOptimization(0): active vertices have a level-0 edge; the index mapping takes the non-fixed ones in table order
        for (int k = tid; k < nKF; k += SD_BA_THREADS) kfAct[k] = 0;
        for (int p = tid; p < nPt; p += SD_BA_THREADS) ptAct[p] = 0;
        __syncthreads();
        double na[1] = {0.0};
        for (int i = tid; i < nE; i += SD_BA_THREADS) if (!level[i]) { kfAct[E[i].kf] = 1; ptAct[E[i].point] = 1; na[0] += 1.0; }
        sd_block_sum<1>(na, red);
        if (tid == 0) {
            int n = 0;
            for (int k = 0; k < nKF; k++) { const bool fixed = k >= nL || KF[k].fixed; if (kfAct[k] && !fixed) { poseIdx[k] = n; poseKf[n] = k; n++; } else poseIdx[k] = -1; }
            sh_i[0] = n;
        }
        __syncthreads();
        const int nPose = sh_i[0], n6 = 6 * nPose;
        if (na[0] == 0.0) continue;                                          // optimize() returns -1: "0 vertices to optimize"
        for (int i = tid; i < 6 * nL; i += SD_BA_THREADS) xp[i] = 0.0;
        for (int i = tid; i < 3 * nPt; i += SD_BA_THREADS) xl[i] = 0.0;
        double lambda = 0.0, currentChi = 0.0;
        int ni = 2, nStop = 0;
        for (int it = 0; it < maxIt; it++) {
            iters[round]++;
            __syncthreads();
            // ---- computeActiveErrors + activeRobustChi2 + linearizeOplus + constructQuadraticForm: one record per active edge
            double cs[1] = {0.0};
            for (int i = tid; i < nE; i += SD_BA_THREADS) {
                if (level[i]) continue;
                const sd_ba_edge ed = E[i];
                const Cam c = cam_of(KF[ed.kf]);
                double r[3], p[3];
                const int D = err(ed, c, est + 7 * ed.kf, X + 3 * ed.point, r, p);
                const double wgt = (double)ed.inv_sigma2, c2 = sd_se3_chi2(r, D, wgt);
                chi2c[i] = c2;
                double rho0 = c2, rho1 = 1.0;
                if (robust) sd_huber(c2, D == 2 ? dM : dS, rho0, rho1);
                cs[0] += rho0;
                edge_record(robust, D, c, wgt, rho1, r, p, est + 7 * ed.kf, rec + (size_t)SD_BA_REC * i);
            }
            sd_block_sum<1>(cs, red);                                          // (its barriers also publish the records)
            currentChi = cs[0];
            const double iniChi = currentChi;
            // ---- gather: pose blocks a wave each, point blocks a lane each
            for (int pi = wave; pi < nPose; pi += 4) {
                const int k = poseKf[pi], a0 = kfStart[k], a1 = kfStart[k + 1];
                double v[27];
#pragma unroll
                for (int j = 0; j < 27; j++) v[j] = 0.0;
                for (int a = a0 + lane; a < a1; a += 64) {
                    const int e = kfList[a];
                    if (level[e]) continue;
                    const double* o = rec + (size_t)SD_BA_REC * e;
#pragma unroll
                    for (int j = 0; j < 27; j++) v[j] += o[j];
                }
                sd_wave_sum<27>(v);
                if (lane < 36) {
                    const int a = lane / 6, b = lane % 6, idx = a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a;
                    double x = 0.0;
#pragma unroll
                    for (int j = 0; j < 21; j++) if (j == idx) x = v[j];
                    Hpp[36 * pi + lane] = x;
                } else if (lane < 42) {
                    double x = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; j++) if (j == lane - 36) x = v[21 + j];
                    bp[6 * pi + lane - 36] = x;
                }
            }
            for (int p = tid; p < nPt; p += SD_BA_THREADS) {
                if (!ptAct[p]) continue;
                double v[9];
#pragma unroll
                for (int j = 0; j < 9; j++) v[j] = 0.0;
                for (int a = ptStart[p]; a < ptStart[p + 1]; a++) {
                    const int e = ptList[a];
                    if (level[e]) continue;
                    const double* o = rec + (size_t)SD_BA_REC * e + 27;
#pragma unroll
                    for (int j = 0; j < 9; j++) v[j] += o[j];
                }
#pragma unroll
                for (int j = 0; j < 6; j++) Hll[6 * p + j] = v[j];
#pragma unroll
                for (int j = 0; j < 3; j++) bl[3 * p + j] = v[6 + j];
            }
            __syncthreads();
            SD_BA_MARK(1);
            if (it == 0) {                                                   // computeLambdaInit: tau * max |diag H| over the index mapping
                double md = 0.0;
                for (int i = tid; i < n6; i += SD_BA_THREADS) md = fmax(fabs(Hpp[36 * (i / 6) + 7 * (i % 6)]), md);
                for (int p = tid; p < nPt; p += SD_BA_THREADS)
                    if (ptAct[p]) md = fmax(fmax(fabs(Hll[6 * p]), fabs(Hll[6 * p + 2])), fmax(fabs(Hll[6 * p + 5]), md));
                md = sd_block_max(md, red);
                lambda = 1e-5 * md; ni = 2; nStop = 0;
            }
            double rho = 0.0;
            int qmax = 0;
            do {
                __syncthreads();
                // ---- push(): backup of the estimates
                for (int i = tid; i < 7 * nKF; i += SD_BA_THREADS) bak[i] = est[i];
                for (int i = tid; i < 3 * nPt; i += SD_BA_THREADS) Xbak[i] = X[i];
                // ---- setLambda + the landmark inverses
                for (int p = tid; p < nPt; p += SD_BA_THREADS) {
                    if (!ptAct[p]) continue;
                    double m[6], o[6];
#pragma unroll
                    for (int j = 0; j < 6; j++) m[j] = Hll[6 * p + j];
                    m[0] += lambda; m[2] += lambda; m[5] += lambda;
                    inverse3(m, o);
#pragma unroll
                    for (int j = 0; j < 6; j++) Dinv[6 * p + j] = o[j];
                }
                __syncthreads();
                // ---- S (upper block triangle) and b_schur, a block row per wave in LDS
                double* row = big + (size_t)wave * 6 * n6;
                for (int pi = wave; pi < nPose; pi += 4) {
                    wave_lds_sync();
                    for (int i = lane; i < 6 * n6; i += 64) row[i] = 0.0;
                    wave_lds_sync();
                    const int a = lane / 6, b = lane % 6;
                    if (lane < 36) row[a * n6 + 6 * pi + b] = Hpp[36 * pi + lane] + (a == b ? lambda : 0.0);
                    double coef = 0.0;
                    const int k = poseKf[pi], a0 = kfStart[k], a1 = kfStart[k + 1];
                    for (int ia = a0; ia < a1; ia++) {
                        const int e1 = kfList[ia];
                        if (level[e1]) continue;
                        const int p = E[e1].point;
                        const double* W1 = rec + (size_t)SD_BA_REC * e1 + 36;
                        const double* Di = Dinv + 6 * p;
                        if (lane < 36) {
                            // row a of Y = W1 Dinv
                            const double w0 = W1[a * 3], w1 = W1[a * 3 + 1], w2 = W1[a * 3 + 2];
                            const double y0 = (w0 * Di[0] + w1 * Di[1]) + w2 * Di[3], y1 = (w0 * Di[1] + w1 * Di[2]) + w2 * Di[4],
                                         y2 = (w0 * Di[3] + w1 * Di[4]) + w2 * Di[5];
                            for (int ib = ptStart[p]; ib < ptStart[p + 1]; ib++) {
                                const int e2 = ptList[ib];
                                if (level[e2]) continue;
                                const int pj = poseIdx[E[e2].kf];
                                if (pj < pi) continue;                       // fixed (-1) or below the diagonal
                                const double* W2 = rec + (size_t)SD_BA_REC * e2 + 36 + 3 * b;
                                row[a * n6 + 6 * pj + b] -= (y0 * W2[0] + y1 * W2[1]) + y2 * W2[2];
                            }
                        } else if (lane < 42) {
                            const int i = lane - 36;
                            const double b0 = bl[3 * p], b1 = bl[3 * p + 1], b2 = bl[3 * p + 2];
                            const double d0 = (Di[0] * b0 + Di[1] * b1) + Di[3] * b2, d1 = (Di[1] * b0 + Di[2] * b1) + Di[4] * b2,
                                         d2 = (Di[3] * b0 + Di[4] * b1) + Di[5] * b2;
                            coef += (W1[i * 3] * d0 + W1[i * 3 + 1] * d1) + W1[i * 3 + 2] * d2;
                        }
                    }
                    if (lane >= 36 && lane < 42) yv[6 * pi + lane - 36] = bp[6 * pi + lane - 36] - coef;
                    wave_lds_sync();
                    for (int i = lane; i < 6 * n6; i += 64) S[(size_t)(6 * pi + i / n6) * n6 + i % n6] = row[i];
                }
                __syncthreads();
                // ---- mirror: the factorisation reads the lower triangle
                for (int i = tid; i < n6 * n6; i += SD_BA_THREADS) { const int r = i / n6, c = i % n6; if (c < r) S[i] = S[(size_t)c * n6 + r]; }
                __syncthreads();
                SD_BA_MARK(2);
                // ---- blocked LDL^T, natural order; a pivot equal to zero fails the trial
                bool ok2 = true;
                for (int k0 = 0; k0 < n6 && ok2; k0 += SD_BA_NB) {
                    const int nb = min(SD_BA_NB, n6 - k0), m = n6 - k0 - nb;
                    for (int i = tid; i < SD_BA_NB * SD_BA_NB; i += SD_BA_THREADS) {
                        const int r = i / SD_BA_NB, c = i % SD_BA_NB;
                        Tl[r * SD_BA_TP + c] = (r < nb && c < nb) ? (c <= r ? S[(size_t)(k0 + r) * n6 + k0 + c] : 0.0) : (r == c ? 1.0 : 0.0);
                    }
                    __syncthreads();
                    for (int j = 0; j < SD_BA_NB; j++) {
                        const double d = Tl[j * SD_BA_TP + j];
                        if (d == 0.0) { ok2 = false; break; }                // uniform: every lane reads the same word
                        if (tid > j && tid < SD_BA_NB) Lcol[tid] = Tl[tid * SD_BA_TP + j] / d;
                        if (tid == j) Dv[j] = d;
                        __syncthreads();
                        const int rem = SD_BA_NB - 1 - j;                    // rows j+1 .. NB-1; pairs (r, c), j < c <= r
                        for (int i = tid; i < rem * rem; i += SD_BA_THREADS) {
                            const int r = j + 1 + i / rem, c = j + 1 + i % rem;
                            if (c <= r) Tl[r * SD_BA_TP + c] -= (Lcol[r] * Lcol[c]) * d;
                        }
                        __syncthreads();
                        if (tid > j && tid < SD_BA_NB) Tl[tid * SD_BA_TP + j] = Lcol[tid];
                        __syncthreads();
                    }
                    if (!ok2) break;
                    for (int i = tid; i < nb * nb; i += SD_BA_THREADS) {
                        const int r = i / nb, c = i % nb;
                        if (c < r) S[(size_t)(k0 + r) * n6 + k0 + c] = Tl[r * SD_BA_TP + c];
                    }
                    if (tid < nb) dg[k0 + tid] = Dv[tid];
                    // panel: row r of the rows below solves x (L D)^T = a against the tile
                    for (int r = tid; r < m; r += SD_BA_THREADS) {
                        panel_row(S + (size_t)(k0 + nb + r) * n6 + k0, nb, Tl, Dv, big + r * SD_BA_TP);
                    }
                    __syncthreads();
                    for (int i = tid; i < m * m; i += SD_BA_THREADS) {
                        const int r = i / m, c = i % m;
                        if (c > r) continue;
                        double s = 0.0;
#pragma unroll 8
                        for (int j = 0; j < SD_BA_NB; j++) s += (big[r * SD_BA_TP + j] * big[c * SD_BA_TP + j]) * Dv[j];
                        S[(size_t)(k0 + nb + r) * n6 + k0 + nb + c] -= s;
                    }
                    __syncthreads();
                }
                SD_BA_MARK(3);
                if (ok2) {
                    // ---- L y = b (blocked: the tile in LDS, the rows below from the workspace), D, L^T x = y
                    for (int k0 = 0; k0 < n6; k0 += SD_BA_NB) {
                        const int nb = min(SD_BA_NB, n6 - k0);
                        for (int i = tid; i < nb * nb; i += SD_BA_THREADS) { const int r = i / nb, c = i % nb; if (c < r) Tl[r * SD_BA_TP + c] = S[(size_t)(k0 + r) * n6 + k0 + c]; }
                        __syncthreads();
                        for (int j = 0; j < nb; j++) {
                            if (tid > j && tid < nb) yv[k0 + tid] -= Tl[tid * SD_BA_TP + j] * yv[k0 + j];
                            __syncthreads();
                        }
                        for (int r = k0 + nb + tid; r < n6; r += SD_BA_THREADS) {
                            double s = 0.0;
                            for (int c = 0; c < nb; c++) s += S[(size_t)r * n6 + k0 + c] * yv[k0 + c];
                            yv[r] -= s;
                        }
                        __syncthreads();
                    }
                    for (int i = tid; i < n6; i += SD_BA_THREADS) yv[i] = yv[i] / dg[i];
                    __syncthreads();
                    for (int k0 = ((n6 - 1) / SD_BA_NB) * SD_BA_NB; k0 >= 0; k0 -= SD_BA_NB) {
                        const int nb = min(SD_BA_NB, n6 - k0);
                        if (tid < nb) {
                            double s = 0.0;
                            for (int r = k0 + nb; r < n6; r++) s += S[(size_t)r * n6 + k0 + tid] * yv[r];
                            yv[k0 + tid] -= s;
                        }
                        for (int i = tid; i < nb * nb; i += SD_BA_THREADS) { const int r = i / nb, c = i % nb; if (c < r) Tl[r * SD_BA_TP + c] = S[(size_t)(k0 + r) * n6 + k0 + c]; }
                        __syncthreads();
                        for (int j = nb - 1; j > 0; j--) {
                            if (tid < j) yv[k0 + tid] -= Tl[j * SD_BA_TP + tid] * yv[k0 + j];
                            __syncthreads();
                        }
                    }
                    for (int i = tid; i < n6; i += SD_BA_THREADS) xp[i] = yv[i];
                    // ---- landmarks: xl = Dinv (bl - Hpl^T xp)
                    for (int p = tid; p < nPt; p += SD_BA_THREADS) {
                        if (!ptAct[p]) continue;
                        double c0 = bl[3 * p], c1 = bl[3 * p + 1], c2 = bl[3 * p + 2];
                        for (int a = ptStart[p]; a < ptStart[p + 1]; a++) {
                            const int e = ptList[a];
                            if (level[e]) continue;
                            const int pj = poseIdx[E[e].kf];
                            if (pj < 0) continue;
                            const double* W = rec + (size_t)SD_BA_REC * e + 36;
#pragma unroll
                            for (int i = 0; i < 6; i++) { const double nx = -yv[6 * pj + i]; c0 += W[i * 3] * nx; c1 += W[i * 3 + 1] * nx; c2 += W[i * 3 + 2] * nx; }
                        }
                        const double* Di = Dinv + 6 * p;
                        xl[3 * p] = (Di[0] * c0 + Di[1] * c1) + Di[3] * c2;
                        xl[3 * p + 1] = (Di[1] * c0 + Di[2] * c1) + Di[4] * c2;
                        xl[3 * p + 2] = (Di[3] * c0 + Di[4] * c1) + Di[5] * c2;
                    }
                }
                __syncthreads();
                SD_BA_MARK(4);
                // ---- update(x): oplus on every vertex of the index mapping (a failed solve leaves x as it was)
                for (int pi = tid; pi < nPose; pi += SD_BA_THREADS) {
                    const int k = poseKf[pi];
                    const double u[6] = {xp[6 * pi], xp[6 * pi + 1], xp[6 * pi + 2], xp[6 * pi + 3], xp[6 * pi + 4], xp[6 * pi + 5]};
                    store_pose(est + 7 * k, sdpose::compose(sdpose::expmap(u), load_pose(est + 7 * k)));
                }
                for (int p = tid; p < nPt; p += SD_BA_THREADS)
                    if (ptAct[p]) { X[3 * p] += xl[3 * p]; X[3 * p + 1] += xl[3 * p + 1]; X[3 * p + 2] += xl[3 * p + 2]; }
                __syncthreads();
                // ---- computeActiveErrors + activeRobustChi2, computeScale
                double tc[2] = {0.0, 0.0};
                for (int i = tid; i < nE; i += SD_BA_THREADS) {
                    if (level[i]) continue;
                    const sd_ba_edge ed = E[i];
                    double r[3], p[3];
                    const int D = err(ed, cam_of(KF[ed.kf]), est + 7 * ed.kf, X + 3 * ed.point, r, p);
                    const double c2 = sd_se3_chi2(r, D, (double)ed.inv_sigma2);
                    chi2c[i] = c2;
                    double rho0 = c2, rho1;
                    if (robust) sd_huber(c2, D == 2 ? dM : dS, rho0, rho1);
                    tc[0] += rho0;
                }
                for (int i = tid; i < n6; i += SD_BA_THREADS) tc[1] += xp[i] * (lambda * xp[i] + bp[i]);
                for (int p = tid; p < nPt; p += SD_BA_THREADS)
                    if (ptAct[p]) {
#pragma unroll
                        for (int j = 0; j < 3; j++) tc[1] += xl[3 * p + j] * (lambda * xl[3 * p + j] + bl[3 * p + j]);
                    }
                sd_block_sum<2>(tc, red);
                SD_BA_MARK(5);
                const double tempChi = ok2 ? tc[0] : 1.7976931348623157e308;
                rho = currentChi - tempChi;
                rho /= tc[1] + 1e-3;
                trials[round]++;
                if (rho > 0 && __builtin_isfinite(tempChi)) {
                    double alpha = 1. - pow((2 * rho - 1), 3);
                    alpha = fmin(alpha, 2. / 3.);
                    lambda *= fmax(1. / 3., alpha);
                    ni = 2;
                    currentChi = tempChi;
                } else {
                    lambda *= ni;
                    ni *= 2;
                    rejected[round]++;
                    for (int i = tid; i < 7 * nKF; i += SD_BA_THREADS) est[i] = bak[i];     // pop(): the edges keep the rejected trial's errors
                    for (int i = tid; i < 3 * nPt; i += SD_BA_THREADS) X[i] = Xbak[i];
                }
                qmax++;
            } while (rho < 0 && qmax < 10);
            if (qmax == 10 || rho == 0) break;
            if ((iniChi - currentChi) * 1e3 < iniChi) nStop++; else nStop = 0;
            if (nStop >= 3) break;
        }
        chiOut[round] = currentChi;
        __syncthreads();
        // ---- chi2() > bound || !isDepthPositive(): chi2 from the cached error, the depth from the estimates
        if (round == 0) {
            double nb1[1] = {0.0};
            for (int i = tid; i < nE; i += SD_BA_THREADS) {
                const sd_ba_edge ed = E[i];
                const T s = load_pose(est + 7 * ed.kf);
                double p0, p1, p2;
                sd_quat_rot(s.r, X[3 * ed.point], X[3 * ed.point + 1], X[3 * ed.point + 2], p0, p1, p2);
                p2 = p2 + s.t2;
                const bool out = chi2c[i] > (ed.ur < 0 ? 5.991 : 7.815) || !(p2 > 0.0);
                level[i] = out ? 1 : 0;
                A.level1[(size_t)P.e0 + i] = out ? 1 : 0;
                nb1[0] += out ? 1.0 : 0.0;
            }
            sd_block_sum<1>(nb1, red);
            nLevel1 = (int)nb1[0];
        }
    }
    // ---- vToErase membership
    __syncthreads();
    if (nE > 0) {
        double ne[1] = {0.0};
        for (int i = tid; i < nE; i += SD_BA_THREADS) {
            const sd_ba_edge ed = E[i];
            const T s = load_pose(est + 7 * ed.kf);
            double p0, p1, p2;
            sd_quat_rot(s.r, X[3 * ed.point], X[3 * ed.point + 1], X[3 * ed.point + 2], p0, p1, p2);
            p2 = p2 + s.t2;
            const bool out = chi2c[i] > (ed.ur < 0 ? 5.991 : 7.815) || !(p2 > 0.0);
            A.erase[(size_t)P.e0 + i] = out ? 1 : 0;
            level[i] = out ? 1 : 0;                                          // reused below: 1 = erased
            ne[0] += out ? 1.0 : 0.0;
        }
        sd_block_sum<1>(ne, red);
        nErased = (int)ne[0];
    }
    // ---- outputs: Converter::toCvMat(SE3Quat) of the local keyframes, the points in f32; a no-op problem hands its input back
    for (int k = tid; k < nL; k += SD_BA_THREADS) {
        float* To = A.Tcw + (size_t)(P.kf0 + k) * 16;
        if (nE == 0) {
#pragma unroll
            for (int j = 0; j < 16; j++) To[j] = KF[k].Tcw[j];
        } else {
            const T s = load_pose(est + 7 * k);
            double R[3][3];
            sd_quat_matrix(s.r, R);
            To[0] = (float)R[0][0]; To[1] = (float)R[0][1]; To[2] = (float)R[0][2]; To[3] = (float)s.t0;
            To[4] = (float)R[1][0]; To[5] = (float)R[1][1]; To[6] = (float)R[1][2]; To[7] = (float)s.t1;
            To[8] = (float)R[2][0]; To[9] = (float)R[2][1]; To[10] = (float)R[2][2]; To[11] = (float)s.t2;
            To[12] = 0.f; To[13] = 0.f; To[14] = 0.f; To[15] = 1.f;
        }
    }
    for (int i = tid; i < 3 * nPt; i += SD_BA_THREADS) A.xwOut[(size_t)P.pt0 * 3 + i] = nE == 0 ? A.xw[(size_t)P.pt0 * 3 + i] : (float)X[i];
    __syncthreads();
    // ---- UpdateNormalAndDepth from the f32 outputs: Ow = -R^T t per keyframe, then a lane per point over its kept edges in order
    for (int k = tid; k < nKF; k += SD_BA_THREADS) {
        const float* Tq = k < nL ? A.Tcw + (size_t)(P.kf0 + k) * 16 : KF[k].Tcw;
#pragma unroll
        for (int j = 0; j < 3; j++) Ow[3 * k + j] = -(((double)Tq[j] * (double)Tq[3] + (double)Tq[4 + j] * (double)Tq[7]) + (double)Tq[8 + j] * (double)Tq[11]);
    }
    __syncthreads();
    for (int p = tid; p < nPt; p += SD_BA_THREADS) {
        const float* xo = A.xwOut + (size_t)(P.pt0 + p) * 3;
        const double x0 = xo[0], x1 = xo[1], x2 = xo[2];
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        int n = 0;
        for (int a = ptStart[p]; a < ptStart[p + 1]; a++) {
            const int e = ptList[a];
            if (level[e]) continue;
            const int k = E[e].kf;
            const double d0 = x0 - Ow[3 * k], d1 = x1 - Ow[3 * k + 1], d2 = x2 - Ow[3 * k + 2];
            const double nrm = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            a0 += d0 / nrm; a1 += d1 / nrm; a2 += d2 / nrm;
            n++;
        }
        float* no = A.normal + (size_t)(P.pt0 + p) * 3;
        no[0] = n ? (float)(a0 / n) : 0.f; no[1] = n ? (float)(a1 / n) : 0.f; no[2] = n ? (float)(a2 / n) : 0.f;
        const int rk = refKf[p];
        float dd = -1.f;
        if (rk >= 0) {
            const double d0 = x0 - Ow[3 * rk], d1 = x1 - Ow[3 * rk + 1], d2 = x2 - Ow[3 * rk + 2];
            dd = (float)sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        }
        A.dist[P.pt0 + p] = dd;
    }
    if (tid == 0) {
        sd_ba_stats z;
        z.iterations[0] = iters[0]; z.iterations[1] = iters[1]; z.trials[0] = trials[0]; z.trials[1] = trials[1];
        z.rejected[0] = rejected[0]; z.rejected[1] = rejected[1]; z.n_level1 = nLevel1; z.n_erased = nErased;
        z.chi2[0] = chiOut[0]; z.chi2[1] = chiOut[1];
        *st = z;
    }
}
