// LocalMapping::CreateNewMapPoints as three batched kernels (gfx950, wave64):
//   k_tri_match         ORBmatcher::SearchForTriangulation + CheckDistEpipolarLine     src/ORBmatcher.cc:814-980, 140-157
//   k_tri_triangulate   the per-match body of CreateNewMapPoints                       src/LocalMapping.cc:285-432
//   k_tri_resolve       mpCurrentKeyFrame->AddMapPoint(pMP, idx1) across neighbours    src/LocalMapping.cc:238-452
// A feature idx1 of KF1 is matched independently of every other (vbMatched2 is never set, ORBmatcher.cc:834/882), so a
// (keyframe, neighbour) pair is one workgroup; the only coupling between neighbours -- an idx1 triangulated with neighbour k is
// skipped by the later ones -- is applied afterwards: k_tri_resolve keeps the first surviving neighbour per idx1.
// Numerics: DESIGN.md Q25-Q30.  Everything derived from the two poses alone (F12, the epipole, Ow, the baseline rule) is formed
// on the host (sd_api.hip, tri_pair_setup).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_frame.h"
#include "k_match.h"
#include "k_bow.h"

#define SD_TRI_WAVES 16
#define SD_TRI_THREADS (64 * SD_TRI_WAVES)
#define SD_TRI_SWEEPS 8          // Jacobi sweeps of the 4x4 null vector (Q29)

struct SdTriPair {
    int img1, img2;              // batch slots of KF1 (the current keyframe) and KF2
    int row1, row2;              // rows of the has-map-point tables
    int skip;                    // the neighbour fails the baseline rule: no matches
    float ex, ey;                // epipole of KF1's centre in KF2
    float F12[9];
    float T1[12], T2[12];        // [Rcw | tcw], three rows of four
    float Ow1[3], Ow2[3];
};

// The candidate test of one (idx1, idx2): everything after `dist > TH_LOW` at ORBmatcher.cc:895-912.  nearEp = the epipole
// exclusion of idx2 (it does not depend on idx1), th = 3.84 * sigma2 of idx2's level (double).
__device__ __forceinline__ unsigned sd_tri_key(int dist, int pos, bool ok2, bool mono1, bool mono2, bool nearEp, float a, float b,
                                               float c, float den, float x2, float y2, double th)
{
    if (!ok2 || dist > SD_TH_LOW) return 0xFFFFFFFFu;
    if (mono1 && mono2 && nearEp) return 0xFFFFFFFFu;
    if (den == 0.0f) return 0xFFFFFFFFu;
    const float num = a * x2 + b * y2 + c;
    const float dsqr = num * num / den;
    if (!((double)dsqr < th)) return 0xFFFFFFFFu;
    return ((unsigned)dist << 16) | (unsigned)(0xFFFF - pos);           // minimum distance, the LAST position on a tie
}

// One workgroup per pair, one wave per vocabulary node both FeatureVectors share (the node pairing of k_match.h); the wave walks KF1's
// features of the node one after the other, its lanes run over KF2's features of the node: in registers up to SD_BOW_REGF of them, from
// memory beyond.
__global__ void __launch_bounds__(SD_TRI_THREADS) k_tri_match(
    const sd_keypoint* __restrict__ kpUn, const uint8_t* __restrict__ desc, const float* __restrict__ uRight, const int* __restrict__ count,
    const unsigned* __restrict__ fvFeat, const int* __restrict__ fvRunStart, const unsigned* __restrict__ fvRunNode,
    const int* __restrict__ meta, const uint8_t* __restrict__ hasMp1 /*nullable [row][cap]*/, const uint8_t* __restrict__ hasMp2,
    const SdTriPair* __restrict__ pairsIn, SdLevelTables L, int cap, int onlyStereo, int checkOrientation,
    int* __restrict__ matchOut, int* __restrict__ pairsOut, int* __restrict__ npairsOut, int* __restrict__ nmatchOut /*nullable*/)
{
    extern __shared__ __align__(16) unsigned char smem[];
    int* s_match = (int*)smem;                               // [cap]
    int* s_cnt = s_match + cap;                              // [SD_TRI_THREADS]
    uint8_t* s_bin = (uint8_t*)(s_cnt + SD_TRI_THREADS);     // [cap]
    __shared__ int s_hist[SD_HISTO];
    __shared__ SdRotKeep s_keep;
    __shared__ int s_total;
    __shared__ float s_scale[SD_MAX_LEVELS], s_sigma2[SD_MAX_LEVELS];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const SdTriPair* P = pairsIn + pair;
    const int img1 = P->img1, img2 = P->img2;
    const int N1 = count[img1];
    for (int i = tid; i < N1; i += SD_TRI_THREADS) s_match[i] = -1;
    if (tid < SD_HISTO) s_hist[tid] = 0;
    if (tid < SD_MAX_LEVELS) { s_scale[tid] = L.scale[tid]; s_sigma2[tid] = L.sigma2[tid]; }
    __syncthreads();
    const SdFvView V1 = sd_fv_view(kpUn, desc, fvFeat, fvRunStart, fvRunNode, meta, img1, cap);
    const SdFvView V2 = sd_fv_view(kpUn, desc, fvFeat, fvRunStart, fvRunNode, meta, img2, cap);
    const int runs1 = P->skip ? 0 : V1.runs;
    const float* ur1 = uRight + (size_t)img1 * cap;
    const float* ur2 = uRight + (size_t)img2 * cap;
    const uint8_t* h1 = hasMp1 ? hasMp1 + (size_t)P->row1 * cap : nullptr;
    const uint8_t* h2 = hasMp2 ? hasMp2 + (size_t)P->row2 * cap : nullptr;
    const float ex = P->ex, ey = P->ey;
    const float F00 = P->F12[0], F01 = P->F12[1], F02 = P->F12[2], F10 = P->F12[3], F11 = P->F12[4], F12_ = P->F12[5],
                F20 = P->F12[6], F21 = P->F12[7], F22 = P->F12[8];
    for (int r1 = wv; r1 < runs1; r1 += SD_TRI_WAVES) {
        const SdNodePair n = sd_fv_pair(V1, r1, V2);
        if (!n.found) continue;
        const int a0 = n.a0, a1 = n.a1, c0 = n.c0, c1 = n.c1;
        const bool inRegs = c1 - c0 <= SD_BOW_REGF;
        // register path: lane l owns positions l and l + 64 of the node's KF2 list for the whole node
        bool ok2[2] = {false, false}, mono2[2] = {false, false}, nearEp[2] = {false, false};
        uint4 g0[2], g1[2]; float x2[2], y2[2]; double th[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            g0[q] = make_uint4(0, 0, 0, 0); g1[q] = g0[q]; x2[q] = 0.f; y2[q] = 0.f; th[q] = 0.0;
            const int c = c0 + lane + 64 * q;
            if (inRegs && c < c1) {
                const unsigned i2 = V2.feat[c];
                const sd_keypoint kp = V2.kp[i2];
                const bool st2 = ur2[i2] >= 0;
                ok2[q] = !(h2 && h2[i2]) && (!onlyStereo || st2);
                mono2[q] = !st2;
                const float dx = ex - kp.x, dy = ey - kp.y;
                nearEp[q] = dx * dx + dy * dy < 100 * s_scale[kp.octave];
                th[q] = 3.84 * (double)s_sigma2[kp.octave];
                x2[q] = kp.x; y2[q] = kp.y;
                const uint4* pf = (const uint4*)(V2.desc + (size_t)i2 * 32);
                g0[q] = pf[0]; g1[q] = pf[1];
            }
        }
        for (int a = a0; a < a1; a++) {                       // wave-uniform
            const unsigned i1 = V1.feat[a];
            if (h1 && h1[i1]) continue;
            const bool st1 = ur1[i1] >= 0;
            if (onlyStereo && !st1) continue;
            const sd_keypoint kp1 = V1.kp[i1];
            const uint4* pk = (const uint4*)(V1.desc + (size_t)i1 * 32);
            const uint4 e0 = pk[0], e1 = pk[1];
            const float la = kp1.x * F00 + kp1.y * F10 + F20;             // the epipolar line of kp1 in KF2
            const float lb = kp1.x * F01 + kp1.y * F11 + F21;
            const float lc = kp1.x * F02 + kp1.y * F12_ + F22;
            const float den = la * la + lb * lb;
            unsigned best = 0xFFFFFFFFu;
            if (inRegs) {
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const unsigned key = sd_tri_key(sd_hamming256(e0, e1, g0[q], g1[q]), lane + 64 * q, ok2[q], !st1, mono2[q], nearEp[q],
                                                    la, lb, lc, den, x2[q], y2[q], th[q]);
                    best = key < best ? key : best;
                }
            } else {
                for (int c = c0 + lane; c < c1; c += 64) {
                    const unsigned i2 = V2.feat[c];
                    const sd_keypoint kp = V2.kp[i2];
                    const bool st2 = ur2[i2] >= 0;
                    const float dx = ex - kp.x, dy = ey - kp.y;
                    const uint4* pf = (const uint4*)(V2.desc + (size_t)i2 * 32);
                    const unsigned key = sd_tri_key(sd_hamming256(e0, e1, pf[0], pf[1]), c - c0, !(h2 && h2[i2]) && (!onlyStereo || st2), !st1,
                                                    !st2, dx * dx + dy * dy < 100 * s_scale[kp.octave], la, lb, lc, den, kp.x, kp.y,
                                                    3.84 * (double)s_sigma2[kp.octave]);
                    best = key < best ? key : best;
                }
            }
            best = sd_wave_min_u32(best);
            if (best == 0xFFFFFFFFu) continue;
            if (lane == 0) {
                const unsigned i2 = V2.feat[c0 + (0xFFFF - (int)(best & 0xFFFFu))];
                s_match[i1] = (int)i2;
                int bin = 0;
                if (checkOrientation) { bin = sd_rot_bin(kp1.angle, V2.kp[i2].angle); atomicAdd(&s_hist[bin], 1); }
                s_bin[i1] = (uint8_t)bin;
            }
        }
    }
    __syncthreads();
    if (checkOrientation) {
        if (tid == 0) s_keep = sd_three_maxima(s_hist);
        __syncthreads();
        const SdRotKeep keep = s_keep;
        for (int i = tid; i < N1; i += SD_TRI_THREADS)
            if (s_match[i] >= 0 && !keep.keeps(s_bin[i])) s_match[i] = -1;
        __syncthreads();
    }
    // vMatchedPairs: (idx1, idx2) in ascending idx1.  Thread t owns idx1 in [t * per, (t + 1) * per)
    const int per = (N1 + SD_TRI_THREADS - 1) / SD_TRI_THREADS;
    int mine = 0;
    for (int q = 0; q < per; q++) { const int i = tid * per + q; if (i < N1 && s_match[i] >= 0) mine++; }
    s_cnt[tid] = mine;
    __syncthreads();
    if (tid < 64) {                                           // exclusive scan of the 1024 counts: 16 per lane
        int sum = 0;
        for (int q = 0; q < SD_TRI_WAVES; q++) sum += s_cnt[tid * SD_TRI_WAVES + q];
        int incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (tid >= o) incl += t; }
        int run = incl - sum;
        for (int q = 0; q < SD_TRI_WAVES; q++) { const int v = s_cnt[tid * SD_TRI_WAVES + q]; s_cnt[tid * SD_TRI_WAVES + q] = run; run += v; }
        if (tid == 63) s_total = incl;
    }
    __syncthreads();
    int r = s_cnt[tid];
    for (int q = 0; q < per; q++) {
        const int i = tid * per + q;
        if (i < N1 && s_match[i] >= 0) { int* o = pairsOut + ((size_t)pair * cap + r) * 2; o[0] = i; o[1] = s_match[i]; r++; }
    }
    for (int i = tid; i < cap; i += SD_TRI_THREADS) matchOut[(size_t)pair * cap + i] = i < N1 ? s_match[i] : -1;
    if (tid == 0) { npairsOut[pair] = s_total; if (nmatchOut) nmatchOut[pair] = s_total; }
}

// ---------------------------------------------------------------- triangulation of one match
// a 3-vector product the way a CV_32F gemm forms it (Q14b): double accumulation, k ascending, one narrowing
__device__ __forceinline__ float sd_tri_dot3(float a0, float a1, float a2, float b0, float b1, float b2)
{
    double s = (double)a0 * (double)b0; s += (double)a1 * (double)b1; s += (double)a2 * (double)b2;
    return (float)s;
}
__device__ __forceinline__ float sd_tri_dot3_add(float a0, float a1, float a2, float b0, float b1, float b2, float c)
{
    double s = (double)a0 * (double)b0; s += (double)a1 * (double)b1; s += (double)a2 * (double)b2; s += (double)c;
    return (float)s;
}
__device__ __forceinline__ double sd_tri_sumsq3(float a0, float a1, float a2)
{
    double s = (double)a0 * (double)a0; s += (double)a1 * (double)a1; s += (double)a2 * (double)a2;
    return s;
}

// Right singular vector of the smallest singular value of the 4x4 A (Q29): one-sided Jacobi in f64, pairs (0,1) (0,2) (0,3) (1,2)
// (1,3) (2,3), SD_TRI_SWEEPS sweeps, the column of the smallest norm (the first on a tie), normalised, narrowed.  Every array index
// is a compile-time constant after unrolling: registers, no scratch.
__device__ __forceinline__ void sd_tri_null4(const float (&A)[4][4], float (&x)[4])
{
    double a[4][4], v[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) { a[r][c] = (double)A[r][c]; v[r][c] = r == c ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < SD_TRI_SWEEPS; sweep++) {
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int r = 0; r < 4; r++) { alpha += a[r][p] * a[r][p]; beta += a[r][q] * a[r][q]; gamma += a[r][p] * a[r][q]; }
                if (gamma != 0.0) {
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const double ap = a[r][p], aq = a[r][q], vp = v[r][p], vq = v[r][q];
                        a[r][p] = cs * ap - sn * aq; a[r][q] = sn * ap + cs * aq;
                        v[r][p] = cs * vp - sn * vq; v[r][q] = sn * vp + cs * vq;
                    }
                }
            }
    }
    double nb = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        double n = 0.0;
#pragma unroll
        for (int r = 0; r < 4; r++) n += a[r][c] * a[r][c];
        if (c == 0 || n < nb) { nb = n; b0 = v[0][c]; b1 = v[1][c]; b2 = v[2][c]; b3 = v[3][c]; }
    }
    const double nv = sqrt(((b0 * b0 + b1 * b1) + b2 * b2) + b3 * b3);
    x[0] = (float)(b0 / nv); x[1] = (float)(b1 / nv); x[2] = (float)(b2 / nv); x[3] = (float)(b3 / nv);
}

// cos(2 * atan2(mb / 2, depth)) as (d^2 - h^2) / (d^2 + h^2), h = mb / 2, in double (Q28)
__device__ __forceinline__ float sd_tri_cos_stereo(float mb, float depth)
{
    const double h = (double)mb / 2.0, d = (double)depth;
    return (float)((d * d - h * h) / (d * d + h * h));
}

// KeyFrame::UnprojectStereo (KeyFrame.cc:615-631): mvKeys, not mvKeysUn
__device__ __forceinline__ void sd_tri_unproject(const float* T /*[Rcw|tcw]*/, const float* Ow, float u, float v, float z, SdCamera cam,
                                                 float invfx, float invfy, float (&X)[3])
{
    const float x = (u - cam.cx) * z * invfx, y = (v - cam.cy) * z * invfy;
    X[0] = sd_tri_dot3_add(T[0], T[4], T[8], x, y, z, Ow[0]);          // Rwc = Rcw^T
    X[1] = sd_tri_dot3_add(T[1], T[5], T[9], x, y, z, Ow[1]);
    X[2] = sd_tri_dot3_add(T[2], T[6], T[10], x, y, z, Ow[2]);
}

// reprojection test of one camera (LocalMapping.cc:363-414): false = rejected
__device__ __forceinline__ bool sd_tri_reproj(const float* T, const float (&X)[3], float z, bool stereo, float kx, float ky, float kur,
                                              float sigma2, SdCamera cam)
{
    const float xc = sd_tri_dot3_add(T[0], T[1], T[2], X[0], X[1], X[2], T[3]);
    const float yc = sd_tri_dot3_add(T[4], T[5], T[6], X[0], X[1], X[2], T[7]);
    const float invz = (float)(1.0 / (double)z);
    const float u = cam.fx * xc * invz + cam.cx;
    const float v = cam.fy * yc * invz + cam.cy;
    const float eX = u - kx, eY = v - ky;
    if (!stereo) return !((double)(eX * eX + eY * eY) > 5.991 * (double)sigma2);
    const float u_r = u - cam.mbf * invz;
    const float eR = u_r - kur;
    return !((double)(eX * eX + eY * eY + eR * eR) > 7.8 * (double)sigma2);
}

// One lane per match: entry j of the pair's vMatchedPairs.  ok[pair][idx1] (zeroed by the caller) = the triangulation survived every
// test, xw = the new point.
__global__ void __launch_bounds__(256) k_tri_triangulate(
    const sd_keypoint* __restrict__ kpUn, const sd_keypoint* __restrict__ kpRaw, const float* __restrict__ uRight, const float* __restrict__ depth,
    const SdTriPair* __restrict__ pairsIn, const int* __restrict__ pairList, const int* __restrict__ npairs, SdLevelTables L, SdCamera cam,
    float ratioFactor, int cap, uint8_t* __restrict__ okOut, float* __restrict__ xwOut)
{
    __shared__ float s_scale[SD_MAX_LEVELS], s_sigma2[SD_MAX_LEVELS];
    if (threadIdx.x < SD_MAX_LEVELS) { s_scale[threadIdx.x] = L.scale[threadIdx.x]; s_sigma2[threadIdx.x] = L.sigma2[threadIdx.x]; }
    __syncthreads();
    const int pair = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const SdTriPair* P = pairsIn + pair;
    if (j >= npairs[pair]) return;
    const int i1 = pairList[((size_t)pair * cap + j) * 2], i2 = pairList[((size_t)pair * cap + j) * 2 + 1];
    const size_t o = (size_t)pair * cap + i1;
    const size_t o1 = (size_t)P->img1 * cap + i1, o2 = (size_t)P->img2 * cap + i2;
    const sd_keypoint kp1 = kpUn[o1], kp2 = kpUn[o2];
    const float ur1 = uRight[o1], ur2 = uRight[o2];
    const bool st1 = ur1 >= 0, st2 = ur2 >= 0;
    const float* T1 = P->T1; const float* T2 = P->T2;
    const float invfx = 1.0f / cam.fx, invfy = 1.0f / cam.fy;
    const float xn1x = (kp1.x - cam.cx) * invfx, xn1y = (kp1.y - cam.cy) * invfy;
    const float xn2x = (kp2.x - cam.cx) * invfx, xn2y = (kp2.y - cam.cy) * invfy;
    const float r1x = sd_tri_dot3(T1[0], T1[4], T1[8], xn1x, xn1y, 1.0f), r1y = sd_tri_dot3(T1[1], T1[5], T1[9], xn1x, xn1y, 1.0f),
                r1z = sd_tri_dot3(T1[2], T1[6], T1[10], xn1x, xn1y, 1.0f);
    const float r2x = sd_tri_dot3(T2[0], T2[4], T2[8], xn2x, xn2y, 1.0f), r2y = sd_tri_dot3(T2[1], T2[5], T2[9], xn2x, xn2y, 1.0f),
                r2z = sd_tri_dot3(T2[2], T2[6], T2[10], xn2x, xn2y, 1.0f);
    double dot = (double)r1x * (double)r2x; dot += (double)r1y * (double)r2y; dot += (double)r1z * (double)r2z;
    const double n1 = sqrt(sd_tri_sumsq3(r1x, r1y, r1z)), n2 = sqrt(sd_tri_sumsq3(r2x, r2y, r2z));
    const float cosRays = (float)(dot / (n1 * n2));
    float cosSt1 = cosRays + 1, cosSt2 = cosRays + 1;
    if (st1) cosSt1 = sd_tri_cos_stereo(cam.mb, depth[o1]);
    else if (st2) cosSt2 = sd_tri_cos_stereo(cam.mb, depth[o2]);          // `else if`: LocalMapping.cc:314
    const float cosSt = cosSt2 < cosSt1 ? cosSt2 : cosSt1;
    float X[3];
    if (cosRays < cosSt && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) {
        float A[4][4], x4[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            A[0][c] = xn1x * T1[8 + c] - T1[c]; A[1][c] = xn1y * T1[8 + c] - T1[4 + c];
            A[2][c] = xn2x * T2[8 + c] - T2[c]; A[3][c] = xn2y * T2[8 + c] - T2[4 + c];
        }
        sd_tri_null4(A, x4);
        if (x4[3] == 0) return;
        X[0] = x4[0] / x4[3]; X[1] = x4[1] / x4[3]; X[2] = x4[2] / x4[3];
    } else if (st1 && cosSt1 < cosSt2) {
        if (!(depth[o1] > 0)) return;                                     // UnprojectStereo returns no point (KeyFrame.cc:618)
        const sd_keypoint r = kpRaw[o1];
        sd_tri_unproject(T1, P->Ow1, r.x, r.y, depth[o1], cam, invfx, invfy, X);
    } else if (st2 && cosSt2 < cosSt1) {
        if (!(depth[o2] > 0)) return;
        const sd_keypoint r = kpRaw[o2];
        sd_tri_unproject(T2, P->Ow2, r.x, r.y, depth[o2], cam, invfx, invfy, X);
    } else return;
    const float z1 = sd_tri_dot3_add(T1[8], T1[9], T1[10], X[0], X[1], X[2], T1[11]);
    if (z1 <= 0) return;
    const float z2 = sd_tri_dot3_add(T2[8], T2[9], T2[10], X[0], X[1], X[2], T2[11]);
    if (z2 <= 0) return;
    if (!sd_tri_reproj(T1, X, z1, st1, kp1.x, kp1.y, ur1, s_sigma2[kp1.octave], cam)) return;
    if (!sd_tri_reproj(T2, X, z2, st2, kp2.x, kp2.y, ur2, s_sigma2[kp2.octave], cam)) return;
    const float dist1 = (float)sqrt(sd_tri_sumsq3(X[0] - P->Ow1[0], X[1] - P->Ow1[1], X[2] - P->Ow1[2]));
    const float dist2 = (float)sqrt(sd_tri_sumsq3(X[0] - P->Ow2[0], X[1] - P->Ow2[1], X[2] - P->Ow2[2]));
    if (dist1 == 0 || dist2 == 0) return;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = s_scale[kp1.octave] / s_scale[kp2.octave];
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return;
    xwOut[3 * o] = X[0]; xwOut[3 * o + 1] = X[1]; xwOut[3 * o + 2] = X[2];
    okOut[o] = 1;
}

// One workgroup per keyframe: its neighbours in list order, idx1 ascending inside a neighbour; an idx1 goes to the first neighbour
// whose triangulation survived.  Thread t owns idx1 in [t * per, (t + 1) * per), so a scan of the per-thread counts gives the
// creation order.
__global__ void __launch_bounds__(256) k_tri_resolve(const int* __restrict__ count, const SdTriPair* __restrict__ pairsIn,
                                                     const int* __restrict__ neighOffset, const int* __restrict__ match,
                                                     const uint8_t* __restrict__ ok, const float* __restrict__ xw, int cap,
                                                     sd_new_map_point* __restrict__ out, int* __restrict__ nnew)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint8_t* s_taken = smem;                                  // [cap]
    __shared__ int s_scan[257];
    const int kf = blockIdx.x, tid = threadIdx.x;
    const int p0 = neighOffset[kf], p1 = neighOffset[kf + 1];
    int total = 0;
    if (p1 > p0) {
        const int N1 = count[pairsIn[p0].img1];
        const int per = (N1 + 255) / 256;
        for (int i = tid; i < N1; i += 256) s_taken[i] = 0;
        __syncthreads();
        for (int p = p0; p < p1; p++) {
            const size_t base = (size_t)p * cap;
            int mine = 0;
            for (int q = 0; q < per; q++) { const int i = tid * per + q; if (i < N1 && ok[base + i] && !s_taken[i]) mine++; }
            s_scan[tid] = mine;
            __syncthreads();
            sd_scan256(s_scan, tid);
            __syncthreads();
            int r = total + s_scan[tid];
            for (int q = 0; q < per; q++) {
                const int i = tid * per + q;
                if (i < N1 && ok[base + i] && !s_taken[i]) {
                    sd_new_map_point m;
                    m.neighbour = p - p0; m.idx1 = i; m.idx2 = match[base + i];
                    m.xw[0] = xw[3 * (base + i)]; m.xw[1] = xw[3 * (base + i) + 1]; m.xw[2] = xw[3 * (base + i) + 2];
                    out[(size_t)kf * cap + r] = m;
                    s_taken[i] = 1;
                    r++;
                }
            }
            total += s_scan[256];
            __syncthreads();
        }
    }
    if (tid == 0) nnew[kf] = total;
}
