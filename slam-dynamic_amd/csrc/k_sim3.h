// Sim3Solver (src/Sim3Solver.cc) for many independent loop candidates in one launch sequence: the 3-point Horn RANSAC that
// LoopClosing::ComputeSim3 (src/LoopClosing.cc:232-400) polls five iterations at a time.  All iterations of a problem are evaluated
// in parallel and the answer is selected by ITERATION INDEX, so it is what find() == iterate(mRansacMaxIts) returns and does not
// depend on which hypothesis finishes first.
//   k_sim3_prepare      per correspondence: camera-frame points Rcw X + tcw, their images, the two truncated error bounds
//   k_sim3_hypotheses   one lane per (problem, iteration): sample -> Horn's closed form (4x4 Jacobi in registers) -> T12, T21
//   k_sim3_count        correspondences staged once per workgroup in LDS; one wave counts one hypothesis with ballot / popcount
//   k_sim3_select       one wave per problem: integer minima / maxima over packed (count, iteration) keys -> sd_sim3_result
//   k_sim3_inliers      re-evaluates the winning hypothesis to write the inlier bytes
// From the sample to the inlier test only + - * / and f64 sqrt are used, in a fixed order (the library is built with
// -ffp-contract=off), so the CPU oracle's independent restatement (tests/cpp/sim3_oracle.cpp) gives the same bytes.  No
// floating-point atomic, no atomic at all: every output word has one writer, and a problem's result is bit-identical whatever
// shares its launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_area.h"
#include "k_match.h"
#include "k_motion.h"

#define SD_SIM3_CHUNK 512            // correspondences staged in LDS at a time (12 floats each, 24 KB)
#define SD_SIM3_HYP_PER_BLOCK 32     // hypotheses one workgroup of k_sim3_count counts over its staged correspondences
#define SD_SIM3_SWEEPS 10            // cyclic Jacobi sweeps of the 4x4 N (fixed; 6 rotations each)
#define SD_SIM3_MAX_N 4096           // == SD_SIM3_MAX_CORRESPONDENCES: a count fits the upper half of a selection key
#define SD_SIM3_MAX_ITS 4096         // == SD_SIM3_MAX_ITERATIONS: an iteration index fits the lower half

// what the kernels read per problem: the caller's record plus where its rows live
struct SdSim3Prob {
    sd_sim3_problem P;
    int c0, n;                // correspondences [c0, c0 + n)
    int maxIts;               // hypotheses to run: ransacMaxIts, or 0 when N < mRansacMinInliers (or N < 3)
    int h0;                   // first row of the problem's hypotheses / counts in the workspace
    int minInliers;
    int ransacMaxIts;         // mRansacMaxIts after SetRansacParameters
    int pad[2];
};
struct SdSim3Pt { float x1[3], x2[3], u1, v1, u2, v2, e1, e2; };      // 48 bytes: mvX3Dc1, mvX3Dc2, mvP1im1, mvP2im2, mvnMaxError1/2
struct SdSim3Hyp { float T12[16], T21[16], R[9], t[3], s, pad[3]; };     // 192 bytes: mT12i, mT21i, mR12i, mt12i, ms12i

struct SdSim3Args {
    const SdSim3Prob* prob;
    const sd_sim3_corr* corr;
    SdSim3Pt* pts;            // [correspondence]
    SdSim3Hyp* hyp;           // [h0 + iteration - 1]
    int* count;               // [h0 + iteration - 1] mnInliersi
    sd_sim3_result* result;   // [problem]
    uint8_t* inlier;          // [correspondence]
};

namespace sdsim3 {

// mvnMaxError is a std::vector<size_t> (include/Sim3Solver.h:78-79): 9.210 * sigma2 truncated, then compared as float
__device__ __forceinline__ float max_error(float sigma2)
{
    const double d = 9.210 * (double)sigma2;
    if (!(d >= 1.0)) return 0.f;                                      // below one, negative or NaN: nothing passes `err < 0`
    if (d >= 9.0e18) return 9.0e18f;
    return (float)(unsigned long long)d;
}

// FromCameraToImage / Project (:382-423)
__device__ __forceinline__ void to_image(float X, float Y, float Z, float fx, float fy, float cx, float cy, float& u, float& v)
{
    const float invz = 1 / Z;
    const float x = X * invz, y = Y * invz;
    u = fx * x + cx; v = fy * y + cy;
}

// one entry of mvAllIndices after `skip` (the first draw) was replaced by the back of the N-vector
__device__ __forceinline__ int after_first(int j, int r0, int N) { return j == r0 ? N - 1 : j; }

// The three indices iteration `it` (1-based) draws (:163-177): draw d is sd_splitmix64 of (seed, it, d) reduced modulo the CURRENT
// size of vAvailableIndices, mapped through the swap-with-back removal in closed form.
__device__ __forceinline__ void sample(unsigned long long seed, int it, int N, int& i0, int& i1, int& i2)
{
    const unsigned long long base = sd_splitmix64(seed) + ((unsigned long long)it << 2);
    const int r0 = (int)(sd_splitmix64(base + 0ull) % (unsigned long long)N);
    const int r1 = (int)(sd_splitmix64(base + 1ull) % (unsigned long long)(N - 1));
    const int r2 = (int)(sd_splitmix64(base + 2ull) % (unsigned long long)(N - 2));
    i0 = r0;
    i1 = after_first(r1, r0, N);
    i2 = r2 == r1 ? after_first(N - 2, r0, N) : after_first(r2, r0, N);
}

// one Jacobi rotation of the symmetric 4x4 A in the (P, Q) plane, accumulated into V (columns = eigenvectors)
template <int P, int Q>
__device__ __forceinline__ void rotate(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[P][Q];
    if (apq != 0.0) {
        const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
        const double at = theta < 0.0 ? -theta : theta;
        double t = 1.0 / (at + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 4; k++) {                                 // A <- A J
            const double akp = A[k][P], akq = A[k][Q];
            A[k][P] = c * akp - s * akq; A[k][Q] = s * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {                                 // A <- J^T A
            const double apk = A[P][k], aqk = A[Q][k];
            A[P][k] = c * apk - s * aqk; A[Q][k] = s * apk + c * aqk;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double vkp = V[k][P], vkq = V[k][Q];
            V[k][P] = c * vkp - s * vkq; V[k][Q] = s * vkp + c * vkq;
        }
    }
}

// Sim3Solver::ComputeSim3 (:226-337) on the three sampled pairs; a[k] / b[k] = column k of P1 / P2
__device__ __forceinline__ void horn(const float (&a)[3][3], const float (&b)[3][3], bool fixScale, SdSim3Hyp& H)
{
    // Step 1: centroids and relative coordinates, f32
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];                         // Pr[row][column]
#pragma unroll
    for (int r = 0; r < 3; r++) {
        O1[r] = ((a[0][r] + a[1][r]) + a[2][r]) / 3.0f;
        O2[r] = ((b[0][r] + b[1][r]) + b[2][r]) / 3.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) { Pr1[r][k] = a[k][r] - O1[r]; Pr2[r][k] = b[k][r] - O2[r]; }
    }
    // Step 2: M = Pr2 * Pr1^T, f32
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { float s = Pr2[i][0] * Pr1[j][0] + Pr2[i][1] * Pr1[j][1]; M[i][j] = s + Pr2[i][2] * Pr1[j][2]; }
    // Step 3: N, its ten entries formed in f32 as the reference's float expressions are
    const float N11 = (M[0][0] + M[1][1]) + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
    const float N22 = (M[0][0] - M[1][1]) - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
    const float N33 = (-M[0][0] + M[1][1]) - M[2][2], N34 = M[1][2] + M[2][1], N44 = (-M[0][0] - M[1][1]) + M[2][2];
    double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    // Step 4: eigenvector of the largest eigenvalue, fixed-sweep cyclic Jacobi in f64
#pragma nounroll
    for (int sweep = 0; sweep < SD_SIM3_SWEEPS; sweep++) {
        rotate<0, 1>(A, V); rotate<0, 2>(A, V); rotate<0, 3>(A, V); rotate<1, 2>(A, V); rotate<1, 3>(A, V); rotate<2, 3>(A, V);
    }
    double best = A[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (A[k][k] > best) { best = A[k][k]; q0 = V[0][k]; q1 = V[1][k]; q2 = V[2][k]; q3 = V[3][k]; }
    const double qn = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    const double w = q0 / qn, x = q1 / qn, y = q2 / qn, z = q3 / qn;
    // the rotation straight from the unit quaternion (q and -q give the same matrix)
    float R[3][3];
    R[0][0] = (float)(1.0 - 2.0 * (y * y + z * z)); R[0][1] = (float)(2.0 * (x * y - w * z)); R[0][2] = (float)(2.0 * (x * z + w * y));
    R[1][0] = (float)(2.0 * (x * y + w * z)); R[1][1] = (float)(1.0 - 2.0 * (x * x + z * z)); R[1][2] = (float)(2.0 * (y * z - w * x));
    R[2][0] = (float)(2.0 * (x * z - w * y)); R[2][1] = (float)(2.0 * (y * z + w * x)); R[2][2] = (float)(1.0 - 2.0 * (x * x + y * y));
    // Step 5: P3 = R * Pr2, f32.  Step 6: scale, f64 sums in row-major order
    float s12 = 1.0f;
    if (!fixScale) {
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                float p3 = R[i][0] * Pr2[0][j] + R[i][1] * Pr2[1][j]; p3 = p3 + R[i][2] * Pr2[2][j];
                nom += (double)Pr1[i][j] * (double)p3;
                den += (double)(p3 * p3);
            }
        s12 = (float)(nom / den);
    }
    // Steps 7, 8: t12 = O1 - sR * O2; T12 = [sR | t12]; T21 = [(1/s) R^T | -(1/s) R^T t12]
    float sR[3][3], t[3], sRi[3][3], ti[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) sR[i][j] = s12 * R[i][j];
#pragma unroll
    for (int i = 0; i < 3; i++) { float s = sR[i][0] * O2[0] + sR[i][1] * O2[1]; s = s + sR[i][2] * O2[2]; t[i] = O1[i] - s; }
    const double inv = 1.0 / (double)s12;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) sRi[i][j] = (float)(inv * (double)R[j][i]);
#pragma unroll
    for (int i = 0; i < 3; i++) { float s = (-sRi[i][0]) * t[0] + (-sRi[i][1]) * t[1]; ti[i] = s + (-sRi[i][2]) * t[2]; }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) { H.T12[4 * i + j] = sR[i][j]; H.T21[4 * i + j] = sRi[i][j]; H.R[3 * i + j] = R[i][j]; }
        H.T12[4 * i + 3] = t[i]; H.T21[4 * i + 3] = ti[i]; H.t[i] = t[i];
        H.T12[12 + i] = 0.f; H.T21[12 + i] = 0.f;
    }
    H.T12[15] = 1.f; H.T21[15] = 1.f; H.s = s12; H.pad[0] = H.pad[1] = H.pad[2] = 0.f;
}

struct Cams { float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2; };

// CheckInliers (:340-364) for one correspondence; z == 0 and NaN simply fail both comparisons
__device__ __forceinline__ bool is_inlier(const float* __restrict__ T12, const float* __restrict__ T21, const Cams& c, float x1, float y1,
                                          float z1, float x2, float y2, float z2, float u1, float v1, float u2, float v2, float e1, float e2)
{
    float X, Y, Z, pu, pv;
    sd_mat3_mul_add(T12, x2, y2, z2, X, Y, Z);                        // vP2im1
    to_image(X, Y, Z, c.fx1, c.fy1, c.cx1, c.cy1, pu, pv);
    const float dx1 = u1 - pu, dy1 = v1 - pv;
    sd_mat3_mul_add(T21, x1, y1, z1, X, Y, Z);                        // vP1im2
    to_image(X, Y, Z, c.fx2, c.fy2, c.cx2, c.cy2, pu, pv);
    const float dx2 = pu - u2, dy2 = pv - v2;
    const float err1 = (float)((double)dx1 * (double)dx1 + (double)dy1 * (double)dy1);   // Mat::dot sums in f64
    const float err2 = (float)((double)dx2 * (double)dx2 + (double)dy2 * (double)dy2);
    return err1 < e1 && err2 < e2;
}

}  // namespace sdsim3

// grid (blocks over the largest problem, problems)
__global__ void __launch_bounds__(256) k_sim3_prepare(SdSim3Args A)
{
    const SdSim3Prob& Q = A.prob[blockIdx.y];
    const int n = Q.n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const sd_sim3_corr c = A.corr[(size_t)Q.c0 + i];
        SdSim3Pt p;
        sd_mat3_mul_add(Q.P.Tcw1, c.xw1[0], c.xw1[1], c.xw1[2], p.x1[0], p.x1[1], p.x1[2]);
        sd_mat3_mul_add(Q.P.Tcw2, c.xw2[0], c.xw2[1], c.xw2[2], p.x2[0], p.x2[1], p.x2[2]);
        sdsim3::to_image(p.x1[0], p.x1[1], p.x1[2], Q.P.fx1, Q.P.fy1, Q.P.cx1, Q.P.cy1, p.u1, p.v1);
        sdsim3::to_image(p.x2[0], p.x2[1], p.x2[2], Q.P.fx2, Q.P.fy2, Q.P.cx2, Q.P.cy2, p.u2, p.v2);
        p.e1 = sdsim3::max_error(c.sigma2_1); p.e2 = sdsim3::max_error(c.sigma2_2);
        A.pts[(size_t)Q.c0 + i] = p;
    }
}

// grid (ceil(largest maxIts / 64), problems), 64 threads: lane = one iteration
__global__ void __launch_bounds__(64) k_sim3_hypotheses(SdSim3Args A)
{
    const SdSim3Prob& Q = A.prob[blockIdx.y];
    const int it = blockIdx.x * 64 + threadIdx.x + 1;                 // mnIterations after the increment (:161)
    if (it > Q.maxIts) return;
    int idx[3];
    sdsim3::sample(Q.P.seed, it, Q.n, idx[0], idx[1], idx[2]);
    float a[3][3], b[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const SdSim3Pt& p = A.pts[(size_t)Q.c0 + idx[k]];
#pragma unroll
        for (int r = 0; r < 3; r++) { a[k][r] = p.x1[r]; b[k][r] = p.x2[r]; }
    }
    SdSim3Hyp H;
    sdsim3::horn(a, b, Q.P.fix_scale != 0, H);
    A.hyp[(size_t)Q.h0 + it - 1] = H;
}

// grid (ceil(largest maxIts / SD_SIM3_HYP_PER_BLOCK), problems), 256 threads.  The workgroup stages the problem's correspondences
// chunk by chunk (component-major, rows one float apart from a bank multiple) and each of its four waves counts
// SD_SIM3_HYP_PER_BLOCK / 4 hypotheses over every chunk: lane = correspondence, ballot + popcount, wave-uniform running count.
__global__ void __launch_bounds__(256) k_sim3_count(SdSim3Args A)
{
    constexpr int STRIDE = SD_SIM3_CHUNK + 1, PER_WAVE = SD_SIM3_HYP_PER_BLOCK / 4;
    __shared__ float sm[12 * STRIDE];
    const SdSim3Prob& Q = A.prob[blockIdx.y];
    const int first = blockIdx.x * SD_SIM3_HYP_PER_BLOCK;            // 0-based hypothesis rows of this workgroup
    if (first >= Q.maxIts) return;                                    // uniform over the workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const sdsim3::Cams cam = {Q.P.fx1, Q.P.fy1, Q.P.cx1, Q.P.cy1, Q.P.fx2, Q.P.fy2, Q.P.cx2, Q.P.cy2};
    int cnt[PER_WAVE];
#pragma unroll
    for (int k = 0; k < PER_WAVE; k++) cnt[k] = 0;
    const int n = Q.n;
    for (int c0 = 0; c0 < n; c0 += SD_SIM3_CHUNK) {
        const int m = min(SD_SIM3_CHUNK, n - c0);
        const float* __restrict__ src = (const float*)(A.pts + (size_t)Q.c0 + c0);
        __syncthreads();                                              // the previous chunk's readers are done
        for (int e = tid; e < m * 12; e += 256) sm[(e % 12) * STRIDE + e / 12] = src[e];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER_WAVE; k++) {
            const int h = first + wave * PER_WAVE + k;
            if (h < Q.maxIts) {                                       // uniform over the wave
                const SdSim3Hyp* __restrict__ H = A.hyp + (size_t)Q.h0 + h;
                for (int i = lane; i < ((m + 63) & ~63); i += 64) {
                    bool in = false;
                    if (i < m)
                        in = sdsim3::is_inlier(H->T12, H->T21, cam, sm[i], sm[STRIDE + i], sm[2 * STRIDE + i], sm[3 * STRIDE + i],
                                               sm[4 * STRIDE + i], sm[5 * STRIDE + i], sm[6 * STRIDE + i], sm[7 * STRIDE + i],
                                               sm[8 * STRIDE + i], sm[9 * STRIDE + i], sm[10 * STRIDE + i], sm[11 * STRIDE + i]);
                    cnt[k] += __popcll(__ballot(in));
                }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < PER_WAVE; k++) {
            const int h = first + wave * PER_WAVE + k;
            if (h < Q.maxIts) A.count[(size_t)Q.h0 + h] = cnt[k];
        }
    }
}

// one wave per problem.  found: the LOWEST iteration whose count is > mRansacMinInliers (:192; every earlier best is <= it, so the
// `>= mnBestInliers` guard of :183 holds there).  Otherwise mnBestInliers / mBestT12: the largest count and, among equal counts, the
// LATEST iteration (`>=`), i.e. the maximum of (count << 16 | iteration).
__global__ void __launch_bounds__(64) k_sim3_select(SdSim3Args A)
{
    const SdSim3Prob& Q = A.prob[blockIdx.x];
    const int lane = threadIdx.x;
    unsigned firstOk = 0xFFFFFFFFu, bestKey = 0u;
    for (int it = lane + 1; it <= Q.maxIts; it += 64) {
        const int c = A.count[(size_t)Q.h0 + it - 1];
        if (c > Q.minInliers) firstOk = min(firstOk, (unsigned)it);
        bestKey = max(bestKey, ((unsigned)c << 16) | (unsigned)it);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        firstOk = min(firstOk, (unsigned)__shfl_xor((int)firstOk, o, 64));
        bestKey = max(bestKey, (unsigned)__shfl_xor((int)bestKey, o, 64));
    }
    const bool found = firstOk != 0xFFFFFFFFu;
    const int it = found ? (int)firstOk : (int)(bestKey & 0xFFFFu);   // 0: the problem ran no hypothesis
    sd_sim3_result* R = A.result + blockIdx.x;
    const SdSim3Hyp* H = A.hyp + (size_t)Q.h0 + (it > 0 ? it - 1 : 0);
    if (lane < 16) R->T12[lane] = it > 0 ? H->T12[lane] : 0.f;
    if (lane < 9) R->R12[lane] = it > 0 ? H->R[lane] : 0.f;
    if (lane < 3) R->t12[lane] = it > 0 ? H->t[lane] : 0.f;
    if (lane == 0) {
        R->found = found ? 1 : 0; R->no_more = found ? 0 : 1; R->iteration = it;
        R->n_inliers = it > 0 ? A.count[(size_t)Q.h0 + it - 1] : 0;
        R->max_its = Q.ransacMaxIts; R->reserved = 0;
        R->s12 = it > 0 ? H->s : 0.f;
    }
}

// grid (blocks over the largest problem, problems): vbInliers of find() -- the winning hypothesis' mask, all zero when nothing was found
__global__ void __launch_bounds__(256) k_sim3_inliers(SdSim3Args A)
{
    const SdSim3Prob& Q = A.prob[blockIdx.y];
    const sd_sim3_result* R = A.result + blockIdx.y;
    const bool found = R->found != 0;
    const SdSim3Hyp* __restrict__ H = A.hyp + (size_t)Q.h0 + (found ? R->iteration - 1 : 0);
    const sdsim3::Cams cam = {Q.P.fx1, Q.P.fy1, Q.P.cx1, Q.P.cy1, Q.P.fx2, Q.P.fy2, Q.P.cx2, Q.P.cy2};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < Q.n; i += gridDim.x * 256) {
        bool in = false;
        if (found) {
            const SdSim3Pt p = A.pts[(size_t)Q.c0 + i];
            in = sdsim3::is_inlier(H->T12, H->T21, cam, p.x1[0], p.x1[1], p.x1[2], p.x2[0], p.x2[1], p.x2[2], p.u1, p.v1, p.u2, p.v2, p.e1, p.e2);
        }
        A.inlier[(size_t)Q.c0 + i] = in ? 1 : 0;
    }
}

// ---------------------------------------------------------------- ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1259-1483)
// Per pair (KF1 slot, KF2 slot) and direction: what the kernels read.  T1 / T2 = the key frames' poses; T21 = [sR21 | t21] and
// T12 = [sR12 | t12] are formed on the host as Q39 freezes them.
// pad[0] != 0: the pair is skipped by all three kernels (a job of the refine chain that does not run); the host path writes 0.
struct SdSim3Pair { float T1[16], T2[16], T21[16], T12[16]; int slot1, slot2, pad[2]; };      // 272 bytes

struct SdSim3SearchArgs {
    const sd_keypoint* kp; const uint8_t* desc; const float* uRight; const unsigned short *sortedIdx, *cellStart; const int* count;
    const SdSim3Pair* pairs;
    const SdMapPoint* mps; const uint8_t* mpDesc; int nPoints;
    const int* kfPoint[2];     // [pair][cap]: vpMapPoints1 / vpMapPoints2 as indices into mps, -1 = NULL or isBad()
    const int* matched12;      // [pair][cap]
    uint8_t* already2;         // [pair][cap] vbAlreadyMatched2
    int* vnMatch[2];           // [pair][cap] vnMatch1 / vnMatch2
    int* match12;              // [pair][cap]
    int* nFound;               // [pair]
    int* errFlag;
    int cap;
};

#define SD_SIM3_TH_HIGH 100     // ORBmatcher::TH_HIGH

// vbAlreadyMatched2 (:1289-1299): grid (blocks over cap, pairs).  already2 was cleared by the caller.  Every writer stores the same 1.
__global__ void __launch_bounds__(256) k_sim3_mark(SdSim3SearchArgs A)
{
    const int pair = blockIdx.y;
    const SdSim3Pair& P = A.pairs[pair];
    if (P.pad[0]) return;
    const int N1 = A.count[P.slot1], N2 = A.count[P.slot2];
    const size_t row = (size_t)pair * A.cap;
    for (int i1 = blockIdx.x * 256 + threadIdx.x; i1 < N1; i1 += gridDim.x * 256) {
        const int idx2 = A.matched12[row + i1];
        if (idx2 >= 0 && idx2 < N2) A.already2[row + idx2] = 1;
    }
}

// One wave per (pair, direction, feature): grid (ceil(cap / 4), 2 * pairs), direction = blockIdx.y & 1 (0: KF1's points into KF2).
// Built from k_area.h; the gates are SearchBySim3's own (:1305-1382): no viewing angle, no chi-square, octave in [level - 1, level],
// `dist < bestDist` (the earlier visit wins a tie), bestDist <= TH_HIGH.  Both directions use the one camera, as the reference does.
__global__ void __launch_bounds__(256) k_sim3_search(SdSim3SearchArgs A, SdLevelTables L, SdCamera cam, float th)
{
    __shared__ float s_scale[SD_MAX_LEVELS];
    if (threadIdx.x < SD_MAX_LEVELS) s_scale[threadIdx.x] = L.scale[threadIdx.x];
    __syncthreads();
    const int pair = blockIdx.y >> 1, dir = blockIdx.y & 1;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const SdSim3Pair& P = A.pairs[pair];
    if (P.pad[0]) return;
    const int src = dir == 0 ? P.slot1 : P.slot2, dst = dir == 0 ? P.slot2 : P.slot1;
    const int N = A.count[src];
    const int i = blockIdx.x * 4 + wv;
    if (i >= N) return;
    const size_t row = (size_t)pair * A.cap;
    const int m = A.kfPoint[dir][row + i];
    bool ok = m >= 0 && m < A.nPoints;
    if ((m < -1 || m >= A.nPoints) && lane == 0) atomicOr(A.errFlag, 1);
    if (dir == 0) { if (A.matched12[row + i] != -1) ok = false; }          // vbAlreadyMatched1
    else if (A.already2[row + i]) ok = false;
    unsigned bestKey = 0xFFFFFFFFu;
    int bestIdx = -1;
    if (ok) {
        const SdMapPoint mp = A.mps[m];
        float xa, ya, za, xc, yc, zc;
        sd_mat3_mul_add(dir == 0 ? P.T1 : P.T2, mp.xw[0], mp.xw[1], mp.xw[2], xa, ya, za);     // p3Dc1 = R1w p3Dw + t1w
        sd_mat3_mul_add(dir == 0 ? P.T21 : P.T12, xa, ya, za, xc, yc, zc);                     // p3Dc2 = sR21 p3Dc1 + t21
        if (zc < 0.0f) ok = false;
        const float invz = 1.0f / zc;
        const float x = xc * invz, y = yc * invz;
        const float u = cam.fx * x + cam.cx;
        const float v = cam.fy * y + cam.cy;
        if (!(u >= cam.mnMinX && u < cam.mnMaxX && v >= cam.mnMinY && v < cam.mnMaxY)) ok = false;      // KeyFrame::IsInImage
        double s2 = (double)xc * (double)xc; s2 += (double)yc * (double)yc; s2 += (double)zc * (double)zc;
        const float dist3D = (float)sqrt(s2);                                                  // cv::norm of the camera-frame point
        if (dist3D < 0.8f * mp.minDistance || dist3D > 1.2f * mp.maxDistance) ok = false;
        if (ok) {
            const int level = sd_predict_scale(mp.maxDistance, dist3D, s_scale[1], L.nlevels);
            const float radius = th * s_scale[level];
            const SdAreaWindow W = sd_area_window(cam, u, v, radius);
            if (!W.empty) {
                const uint4* dl = (const uint4*)(A.mpDesc + (size_t)m * 32);
                const uint4 l0 = dl[0], l1 = dl[1];
                const SdImageArrays C = sd_image_arrays(A.kp, nullptr, A.uRight, A.desc, A.sortedIdx, A.cellStart, dst, A.cap);
                const SdAreaWalk<64> walk(C, W, true, lane);
                for (int base = 0; base < walk.total; base += 64) {
                    const int tt = base + lane;
                    const int i2 = walk.member(tt);
                    if (i2 >= 0) {
                        const sd_keypoint k = C.kp[i2];
                        const float distx = k.x - u, disty = k.y - v;
                        if (fabsf(distx) < radius && fabsf(disty) < radius && k.octave >= level - 1 && k.octave <= level) {
                            const uint4* dr = (const uint4*)(C.desc + (size_t)i2 * 32);
                            const int dist = sd_hamming256(l0, l1, dr[0], dr[1]);
                            const unsigned key = ((unsigned)dist << 16) | (unsigned)tt;
                            if (key < bestKey) { bestKey = key; bestIdx = i2; }
                        }
                    }
                }
            }
        }
    }
    const unsigned w = sd_wave_min_u32(bestKey);
    int out = -1;
    if (w != 0xFFFFFFFFu && (int)(w >> 16) <= SD_SIM3_TH_HIGH) {
        const unsigned long long who = __ballot(bestKey == w);           // keys are unique: the walk position is in the low bits
        out = __shfl(bestIdx, __ffsll((long long)who) - 1, 64);
    }
    if (lane == 0) A.vnMatch[dir][row + i] = out;
}

// The agreement loop (:1464-1480): one workgroup per pair.  match12[i1] = idx2 where vnMatch2[vnMatch1[i1]] == i1, else -1.
__global__ void __launch_bounds__(256) k_sim3_agree(SdSim3SearchArgs A)
{
    __shared__ int s_n[4];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const SdSim3Pair& P = A.pairs[pair];
    if (P.pad[0]) { if (tid == 0) A.nFound[pair] = 0; return; }
    const int N1 = A.count[P.slot1], N2 = A.count[P.slot2];
    const size_t row = (size_t)pair * A.cap;
    int n = 0;
    for (int base = 0; base < N1; base += 256) {
        const int i1 = base + tid;
        bool agree = false;
        int idx2 = -1;
        if (i1 < N1) {
            idx2 = A.vnMatch[0][row + i1];
            if (idx2 >= 0 && idx2 < N2) agree = A.vnMatch[1][row + idx2] == i1;
            A.match12[row + i1] = agree ? idx2 : -1;
        }
        n += __popcll(__ballot(agree));
    }
    if ((tid & 63) == 0) s_n[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) A.nFound[pair] = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
}
