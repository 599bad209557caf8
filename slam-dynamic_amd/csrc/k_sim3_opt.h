// Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241) with the vendored g2o's Levenberg-Marquardt and NUMERIC Jacobians for many
// independent (keyframe, loop candidate) pairs in one launch: ONE WAVE per problem (a 64-thread workgroup) runs optimize(5), the
// classification, optimize(5 or 10) and the final count.  A problem is a single 7x7 block over 20 - 300 correspondences, so a wave
// holds 1 - 5 of them per lane; with one wave there is no barrier between the ~60 reductions of a problem and no LDS round trip in
// them (k_pose_optimize spends most of its time in exactly those for problems of this size), and 512 problems still fill the chip.
// Lane l owns correspondences l, l + 64, ... and adds their terms in that order; the 36 sums (28 of H, 7 of b, chi2) then go through
// a wave64 xor-butterfly, so every lane holds the same bits and the order depends on nothing outside the problem.  Everything after
// a reduction (the 7x7 pivoted LDL^T, Sim3(update), the LM bookkeeping) is computed uniformly by every lane.
// Numeric differentiation (base_binary_edge.hpp:147-200): the 14 probe estimates oplus(+-1e-9 e_d) do not depend on the edge, so
// lanes 0..13 form one each (and its inverse) per linearisation and publish it in LDS; every edge is then evaluated 15 times.
// The arithmetic is sd_sim3_math.h, shared with the CPU oracle.  f64 throughout; no atomic; every output word has one writer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sd_frontend.h"
#include "sd_sim3_math.h"

struct SdSim3OptProb { sd_sim3_opt_problem P; int c0, n; };      // the caller's record plus its correspondences [c0, c0 + n)

struct SdSim3OptArgs {
    const SdSim3OptProb* prob;
    const sd_sim3_opt_corr* corr;
    sd_sim3_opt_result* result;
    uint8_t* state;
};

namespace sds3o {

__device__ __forceinline__ int wave_count(bool pred) { return __popcll(__ballot(pred)); }

struct Pt { double X1, Y1, Z1, X2, Y2, Z2, u1, v1, u2, v2, w1, w2; };

__device__ __forceinline__ Pt load(const sd_sim3_opt_corr& c, const sd_sim3_opt_problem& P)
{
    float a, b, d;
    Pt p;
    sd_s3_to_camera(P.Tcw1, c.xw1[0], c.xw1[1], c.xw1[2], a, b, d);
    p.X1 = a; p.Y1 = b; p.Z1 = d;
    sd_s3_to_camera(P.Tcw2, c.xw2[0], c.xw2[1], c.xw2[2], a, b, d);
    p.X2 = a; p.Y2 = b; p.Z2 = d;
    p.u1 = c.obs1[0]; p.v1 = c.obs1[1]; p.u2 = c.obs2[0]; p.v2 = c.obs2[1];
    p.w1 = c.inv_sigma2_1; p.w2 = c.inv_sigma2_2;
    return p;
}

// the robust chi2 of both edges of every live correspondence at S (computeActiveErrors + activeRobustChi2)
__device__ __forceinline__ double robust_chi2(const sd_sim3_opt_corr* corr, const uint8_t* st, const SdSim3OptProb& Q, const sd_s3& S,
                                              const sd_s3_cam& c1, const sd_s3_cam& c2, double delta)
{
    const sd_s3 Si = sd_s3_inverse(S);
    double tc[1] = {0.0};
    for (int i = threadIdx.x; i < Q.n; i += 64) {
        if (st[i]) continue;
        const Pt p = load(corr[i], Q.P);
        double e0, e1, r0, r1;
        sd_s3_error(S, c1, p.X2, p.Y2, p.Z2, p.u1, p.v1, e0, e1);
        sd_huber(sd_s3_chi2(e0, e1, p.w1), delta, r0, r1);
        tc[0] += r0;
        sd_s3_error(Si, c2, p.X1, p.Y1, p.Z1, p.u2, p.v2, e0, e1);
        sd_huber(sd_s3_chi2(e0, e1, p.w2), delta, r0, r1);
        tc[0] += r0;
    }
    sd_wave_sum<1>(tc);
    return tc[0];
}

}  // namespace sds3o

__global__ void __launch_bounds__(64) k_sim3_optimize(SdSim3OptArgs A)
{
    using namespace sds3o;
    __shared__ sd_s3 probe[14][2];                                       // oplus(+-delta e_d) and its inverse
    const SdSim3OptProb& Q = A.prob[blockIdx.x];
    const sd_sim3_opt_problem& P = Q.P;
    const int lane = threadIdx.x, n = Q.n;
    uint8_t* st = A.state + (size_t)Q.c0;                                // entry i is only ever touched by lane i % 64
    const sd_sim3_opt_corr* corr = A.corr + (size_t)Q.c0;
    for (int i = lane; i < n; i += 64) st[i] = 0;
    const sd_s3_cam c1 = {(double)P.fx1, (double)P.fy1, (double)P.cx1, (double)P.cy1};
    const sd_s3_cam c2 = {(double)P.fx2, (double)P.fy2, (double)P.cx2, (double)P.cy2};
    const double th2 = (double)P.th2, delta = (double)(float)sqrt(th2);    // const float deltaHuber = sqrt(th2)
    const bool fix = P.fix_scale != 0;
    sd_s3 prior;                                                         // g2o::Sim3(Matrix3d R, Vector3d t, double s)
    {
        double R[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) R[i][j] = (double)P.R12[i * 3 + j];
        prior.r = sd_quat_of(R);
        prior.t0 = (double)P.t12[0]; prior.t1 = (double)P.t12[1]; prior.t2 = (double)P.t12[2];
        prior.s = (double)P.s12;
    }
    sd_s3 est = prior, errEst = prior;                                   // errEst: the estimate of the last computeActiveErrors
    double xs[7] = {0, 0, 0, 0, 0, 0, 0};                                // the solver's x: zeroed once, kept between the rounds
    int nBad = 0, ret = 0, written = 0, more = 5;
    int its[2] = {0, 0}, trials[2] = {0, 0}, stop[2] = {0, 0};
    for (int round = 0; round < 2; round++) {
        const int maxIt = round == 0 ? 5 : more;
        if (n - nBad > 0) {                                              // else: no active vertex, optimize() returns -1
            double lambda = 0.0;
            int ni = 2, nStop = 0;
            for (int it = 0; it < maxIt; it++) {
                // computeActiveErrors + activeRobustChi2 + buildSystem (linearizeOplus numerically) at est
                __syncthreads();                                         // the previous linearisation's readers are done
                if (lane < 14) {
                    double u[7];
#pragma unroll
                    for (int d = 0; d < 7; d++) u[d] = d == (lane >> 1) ? ((lane & 1) ? -1e-9 : 1e-9) : 0.0;
                    int br;
                    const sd_s3 pe = sd_s3_oplus(est, u, fix, br);
                    probe[lane][0] = pe; probe[lane][1] = sd_s3_inverse(pe);
                }
                __syncthreads();
                const sd_s3 inv = sd_s3_inverse(est);
                const double scalar = 1.0 / (2 * 1e-9);
                double v[36];
#pragma unroll
                for (int k = 0; k < 36; k++) v[k] = 0.0;
                for (int i = lane; i < n; i += 64) {
                    if (st[i]) continue;
                    const Pt p = load(corr[i], P);
                    double a0, a1, b0, b1, J12[2][7], J21[2][7];
#pragma unroll
                    for (int d = 0; d < 7; d++) {
                        double m0, m1;
                        sd_s3_error(probe[2 * d][0], c1, p.X2, p.Y2, p.Z2, p.u1, p.v1, a0, a1);
                        sd_s3_error(probe[2 * d + 1][0], c1, p.X2, p.Y2, p.Z2, p.u1, p.v1, m0, m1);
                        J12[0][d] = scalar * (a0 - m0); J12[1][d] = scalar * (a1 - m1);
                        sd_s3_error(probe[2 * d][1], c2, p.X1, p.Y1, p.Z1, p.u2, p.v2, b0, b1);
                        sd_s3_error(probe[2 * d + 1][1], c2, p.X1, p.Y1, p.Z1, p.u2, p.v2, m0, m1);
                        J21[0][d] = scalar * (b0 - m0); J21[1][d] = scalar * (b1 - m1);
                    }
                    sd_s3_error(est, c1, p.X2, p.Y2, p.Z2, p.u1, p.v1, a0, a1);
                    sd_s3_accumulate(a0, a1, J12, p.w1, delta, v);
                    sd_s3_error(inv, c2, p.X1, p.Y1, p.Z1, p.u2, p.v2, b0, b1);
                    sd_s3_accumulate(b0, b1, J21, p.w2, delta, v);
                }
                sd_wave_sum<36>(v);
                errEst = est;
                double currentChi = v[35];
                const double iniChi = currentChi;
                if (it == 0) {                                           // computeLambdaInit: tau * max |diag H|
                    double md = 0.0;
#pragma unroll
                    for (int j = 0; j < 7; j++) md = fmax(fabs(v[j * (j + 1) / 2 + j]), md);
                    lambda = 1e-5 * md; ni = 2; nStop = 0;
                }
                double rho = 0.0;
                int qmax = 0;
                do {
                    const sd_s3 backup = est;
                    const bool ok2 = sd_s3_solve7(v, v + 28, lambda, xs);
                    int br;
                    est = sd_s3_oplus(est, xs, fix, br);
                    const double tc = robust_chi2(corr, st, Q, est, c1, c2, delta);
                    errEst = est;
                    const double tempChi = ok2 ? tc : 1.7976931348623157e308;
                    rho = currentChi - tempChi;
                    double scale = 0.0;
#pragma unroll
                    for (int j = 0; j < 7; j++) scale += xs[j] * (lambda * xs[j] + v[28 + j]);
                    scale += 1e-3;
                    rho /= scale;
                    if (rho > 0 && __builtin_isfinite(tempChi)) {
                        lambda *= sd_s3_good_step_scale(rho);
                        ni = 2;
                        currentChi = tempChi;
                    } else {
                        lambda *= ni;
                        ni *= 2;
                        est = backup;                                    // pop(): the edges keep the rejected trial's errors
                    }
                    qmax++;
                } while (rho < 0 && qmax < 10);
                its[round] = it + 1; trials[round] += qmax;
                if (qmax == 10) { stop[round] = 1; break; }
                if (rho == 0) { stop[round] = 2; break; }
                if ((iniChi - currentChi) * 1e3 < iniChi) nStop++; else nStop = 0;
                if (nStop >= 3) { stop[round] = 3; break; }
            }
        }
        // chi2() of both edges reads the error cached by the last computeActiveErrors: at errEst, which a rejected last trial leaves
        // different from est
        const sd_s3 errInv = sd_s3_inverse(errEst);
        int nFlag = 0, nIn = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            bool live = false, bad = false;
            if (i < n && !st[i]) {
                live = true;
                const Pt p = load(corr[i], P);
                double e0, e1;
                sd_s3_error(errEst, c1, p.X2, p.Y2, p.Z2, p.u1, p.v1, e0, e1);
                const double x12 = sd_s3_chi2(e0, e1, p.w1);
                sd_s3_error(errInv, c2, p.X1, p.Y1, p.Z1, p.u2, p.v2, e0, e1);
                const double x21 = sd_s3_chi2(e0, e1, p.w2);
                bad = x12 > th2 || x21 > th2;
                if (bad) st[i] = round == 0 ? 1 : 2;
            }
            nFlag += wave_count(bad); nIn += wave_count(live && !bad);
        }
        if (round == 0) {
            nBad = nFlag;
            more = nBad > 0 ? 10 : 5;
            if (n - nBad < 10) break;                                    // return 0: g2oS12 is NOT written back
        } else {
            ret = nIn; written = 1;
        }
    }
    if (lane == 0) {
        const sd_s3 o = written ? est : prior;
        sd_sim3_opt_result r;
        r.ret = ret; r.n_correspondences = n; r.n_bad = nBad; r.more_iterations = more;
        r.iterations[0] = its[0]; r.iterations[1] = its[1]; r.trials[0] = trials[0]; r.trials[1] = trials[1];
        r.stop[0] = stop[0]; r.stop[1] = stop[1]; r.written = written; r.reserved = 0;
        r.q[0] = o.r.x; r.q[1] = o.r.y; r.q[2] = o.r.z; r.q[3] = o.r.w; r.t[0] = o.t0; r.t[1] = o.t1; r.t[2] = o.t2; r.s = o.s;
        // Converter::toCvSE3(s * R, t) with R = Quaterniond::toRotationMatrix()
        double R[3][3];
        sd_quat_matrix(o.r, R);
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) r.T12[i * 4 + j] = (float)(o.s * R[i][j]);
        }
        r.T12[3] = (float)o.t0; r.T12[7] = (float)o.t1; r.T12[11] = (float)o.t2;
        r.T12[12] = 0.f; r.T12[13] = 0.f; r.T12[14] = 0.f; r.T12[15] = 1.f;
        A.result[blockIdx.x] = r;
    }
}
