// CPU oracle of Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241): a sequential restatement of the graph the function builds and
// of the pieces of the vendored g2o it runs -- literal vectors of edges, SparseOptimizer::optimize / initializeOptimization,
// OptimizationAlgorithmLevenberg::solve one trial after the other, BaseBinaryEdge's numeric linearizeOplus with push / oplus /
// computeError / pop per probe, the edges' cached _error that chi2() reads.  The arithmetic of one error, one Sim3(update) and one
// edge's quadratic form is slam-dynamic_amd/csrc/sd_sim3_math.h, the header the kernel includes (a last-bit difference in an error
// is a 1e-5 difference in the numeric Jacobian; DESIGN Q45).  Sums run edge by edge in the order the edges were added (or the
// reverse, OPT_REVERSE); OPT_WAVE restates the kernel's fixed summation order instead (64 lane partials, then the xor-butterfly), which
// makes the two comparable bit for bit -- the only way to compare the LM decisions of a converged problem, which are rounding noise.
// Build: g++ -std=c++17 -O2 -ffp-contract=off -I slam-dynamic_amd/csrc -I include; a second build with -ffp-contract=fast and FMA
// measures the spread.  `flags` also selects deliberately WRONG twins, each of which must differ on a crafted case.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "sd_frontend.h"
#include "sd_sim3_math.h"

namespace {

enum {
    TWIN_ANALYTIC = 1,        // analytic Jacobians instead of the numeric ones
    TWIN_RECOMPUTE = 2,       // computeError() re-run at the estimate before chi2()
    TWIN_WRITE_ON_ZERO = 4,   // g2oS12 written back on the `return 0` path
    TWIN_KEEP_LAMBDA = 8,     // lambda, _ni, _nBad not restarted by the second optimize()
    TWIN_SINGLE_CHI2 = 16,    // e12->chi2() > th2 alone
    VARIANT_DROP_SCALE = 32,  // fixed scale: the seventh column dropped (a 6 x 6 system) instead of zeroed -- NOT wrong: the same bits
    OPT_REVERSE = 64,         // the edges visited last to first (spread)
    OPT_WAVE = 128,           // sums in the kernel's fixed order: correspondence i adds to partial i % 64, then an xor-butterfly
};

// info: what a run reached
enum { I_BRANCH0 = 0 /* ..3: Sim3(update) branches of the solver's updates */, I_SOLVE_FAILED = 4, I_REJECTED = 5, I_LAST_REJECTED_R1 = 6,
       I_LAST_REJECTED_R2 = 7, I_STALE_DECIDES_R1 = 8, I_STALE_DECIDES_R2 = 9, I_NONFINITE = 10, I_HUBER = 11, I_COUNT = 16 };
// margins: the smallest relative distance of a decision from its threshold
enum { M_CHI2 = 0, M_RHO = 1, M_STOP = 2, M_STALE = 3 /* a MAXIMUM: the largest |cached chi2 - fresh chi2| / th2 of a check */, M_COUNT = 4 };

struct Edge {                 // one EdgeSim3ProjectXYZ (inverse = false) or EdgeInverseSim3ProjectXYZ
    bool inverse;
    double X, Y, Z;           // the fixed VertexSBAPointXYZ it hangs on
    double u, v, w;           // measurement, information = w I
    int corr;
    double e0, e1;            // _error as the last computeError left it
    double J[2][7];
};

struct Graph {
    sd_s3 est;                // VertexSim3Expmap::_estimate
    sd_s3_cam c1, c2;
    bool fix, wave = false;
    double delta;
    std::vector<Edge> edges;  // active edges, in the order of addition
    std::vector<int> order;   // the order sums visit them in
};

void compute_error(const Graph& G, Edge& e, const sd_s3& S)
{
    if (e.inverse) sd_s3_error(sd_s3_inverse(S), G.c2, e.X, e.Y, e.Z, e.u, e.v, e.e0, e.e1);
    else sd_s3_error(S, G.c1, e.X, e.Y, e.Z, e.u, e.v, e.e0, e.e1);
}

void analytic_jacobian(const Graph& G, const Edge& e, const sd_s3& S, double (&J)[2][7])
{
    double R[3][3];
    {
        const double x = S.qx, y = S.qy, z = S.qz, w = S.qw;
        R[0][0] = 1 - 2 * (y * y + z * z); R[0][1] = 2 * (x * y - z * w); R[0][2] = 2 * (x * z + y * w);
        R[1][0] = 2 * (x * y + z * w); R[1][1] = 1 - 2 * (x * x + z * z); R[1][2] = 2 * (y * z - x * w);
        R[2][0] = 2 * (x * z - y * w); R[2][1] = 2 * (y * z + x * w); R[2][2] = 1 - 2 * (x * x + y * y);
    }
    double p[3], dp[3][7];
    if (!e.inverse) {                       // p = S X; d(exp(u) S X) = -[p]x dw + dv + p dsigma
        sd_s3_map(S, e.X, e.Y, e.Z, p[0], p[1], p[2]);
        const double sk[3][3] = {{0, p[2], -p[1]}, {-p[2], 0, p[0]}, {p[1], -p[0], 0}};
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) { dp[i][j] = sk[i][j]; dp[i][3 + j] = i == j ? 1.0 : 0.0; }
            dp[i][6] = p[i];
        }
    } else {                                // p = S^-1 exp(-u) X: dp = (1 / s) R^T ([X]x dw - dv - X dsigma)
        const sd_s3 Si = sd_s3_inverse(S);
        sd_s3_map(Si, e.X, e.Y, e.Z, p[0], p[1], p[2]);
        const double X[3] = {e.X, e.Y, e.Z};
        const double sk[3][3] = {{0, -X[2], X[1]}, {X[2], 0, -X[0]}, {-X[1], X[0], 0}};      // [X]x
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) {
                dp[i][j] = (R[0][i] * sk[0][j] + R[1][i] * sk[1][j] + R[2][i] * sk[2][j]) / S.s;
                dp[i][3 + j] = -R[j][i] / S.s;
            }
            dp[i][6] = -(R[0][i] * X[0] + R[1][i] * X[1] + R[2][i] * X[2]) / S.s;
        }
    }
    const sd_s3_cam& c = e.inverse ? G.c2 : G.c1;
    const double iz = 1.0 / p[2];
    for (int d = 0; d < 7; d++) {
        J[0][d] = -c.fx * (dp[0][d] * iz - p[0] * iz * iz * dp[2][d]);
        J[1][d] = -c.fy * (dp[1][d] * iz - p[1] * iz * iz * dp[2][d]);
    }
    if (G.fix) { J[0][6] = 0; J[1][6] = 0; }
}

// BaseBinaryEdge::linearizeOplus for the free Sim3 vertex (base_binary_edge.hpp:176-200)
void numeric_jacobian(Graph& G, Edge& e)
{
    const double delta = 1e-9;
    const double scalar = 1.0 / (2 * delta);
    const double b0 = e.e0, b1 = e.e1;      // errorBeforeNumeric
    double add[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int d = 0; d < 7; d++) {
        int br;
        const sd_s3 backup = G.est;         // push
        add[d] = delta;
        G.est = sd_s3_oplus(G.est, add, G.fix, br);
        compute_error(G, e, G.est);
        double k0 = e.e0, k1 = e.e1;        // errorBak
        G.est = backup;                     // pop
        add[d] = -delta;
        G.est = sd_s3_oplus(G.est, add, G.fix, br);
        compute_error(G, e, G.est);
        k0 -= e.e0; k1 -= e.e1;
        G.est = backup;
        add[d] = 0.0;
        e.J[0][d] = scalar * k0; e.J[1][d] = scalar * k1;
    }
    e.e0 = b0; e.e1 = b1;
}

void margin_min(double& m, double v) { if (v == v && v < m) m = v; }

// the wave64 xor-butterfly over 64 lane partials of K sums each: every lane ends with the same bits, lane 0's are returned in part[0]
template <int K>
void butterfly(double (*part)[K])
{
    for (int o = 32; o >= 1; o >>= 1) {
        double next[64][K];
        for (int l = 0; l < 64; l++) for (int k = 0; k < K; k++) next[l][k] = part[l][k] + part[l ^ o][k];
        memcpy(part, next, sizeof(next));
    }
}

double active_robust_chi2(const Graph& G)
{
    if (G.wave) {
        double part[64][1];
        for (int l = 0; l < 64; l++) part[l][0] = 0.0;
        for (const Edge& e : G.edges) {
            double r0, r1;
            sd_s3_huber(sd_s3_chi2(e.e0, e.e1, e.w), G.delta, r0, r1);
            part[e.corr & 63][0] += r0;
        }
        butterfly<1>(part);
        return part[0][0];
    }
    double s = 0.0;
    for (int k : G.order) {
        const Edge& e = G.edges[k];
        double r0, r1;
        sd_s3_huber(sd_s3_chi2(e.e0, e.e1, e.w), G.delta, r0, r1);
        s += r0;
    }
    return s;
}

struct Lm { double lambda = 0; int ni = 2, nBad = 0; };

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg::solve; returns the iterations run
int optimize(Graph& G, int iterations, int flags, Lm& lm, bool restart, double (&x)[7], int& trials, int& stop, bool& lastRejected,
             int64_t* info, double* mg)
{
    trials = 0; stop = SD_SIM3_OPT_STOP_OK; lastRejected = false;
    if (G.edges.empty()) return 0;          // no active vertex: optimize() returns -1 before anything runs
    int done = 0;
    for (int it = 0; it < iterations; it++) {
        for (int k : G.order) compute_error(G, G.edges[k], G.est);          // computeActiveErrors
        double currentChi = active_robust_chi2(G);
        double v[36], part[64][36];
        for (int k = 0; k < 36; k++) v[k] = 0.0;
        for (int l = 0; l < 64; l++) for (int k = 0; k < 36; k++) part[l][k] = 0.0;
        for (int k : G.order) {             // buildSystem: linearizeOplus, constructQuadraticForm
            Edge& e = G.edges[k];
            if (flags & TWIN_ANALYTIC) analytic_jacobian(G, e, G.est, e.J);
            else numeric_jacobian(G, e);
            sd_s3_accumulate(e.e0, e.e1, e.J, e.w, G.delta, G.wave ? part[e.corr & 63] : v);
            if (!(sd_s3_chi2(e.e0, e.e1, e.w) <= G.delta * G.delta)) info[I_HUBER]++;
            if (!std::isfinite(e.e0) || !std::isfinite(e.e1)) info[I_NONFINITE]++;
        }
        if (G.wave) {
            butterfly<36>(part);
            for (int k = 0; k < 36; k++) v[k] = part[0][k];
            currentChi = v[35];             // the kernel takes chi2 from the same pass
        }
        const double iniChi = currentChi;
        if (it == 0 && restart) {           // computeLambdaInit
            double md = 0.0;
            for (int j = 0; j < 7; j++) md = std::max(std::fabs(v[j * (j + 1) / 2 + j]), md);
            lm.lambda = 1e-5 * md; lm.ni = 2; lm.nBad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const sd_s3 backup = G.est;     // push
            bool ok2;
            if ((flags & VARIANT_DROP_SCALE) && G.fix) {
                double x6[6] = {x[0], x[1], x[2], x[3], x[4], x[5]};
                ok2 = sd_s3_solve<6>(v, v + 28, lm.lambda, x6);             // the first 21 entries are the 6 x 6 lower triangle
                for (int j = 0; j < 6; j++) x[j] = x6[j];
                x[6] = 0;
            } else ok2 = sd_s3_solve7(v, v + 28, lm.lambda, x);
            if (!ok2) info[I_SOLVE_FAILED]++;
            int br = 0;
            G.est = sd_s3_oplus(G.est, x, G.fix, br);
            info[I_BRANCH0 + br]++;
            for (int k : G.order) compute_error(G, G.edges[k], G.est);
            double tempChi = active_robust_chi2(G);
            if (!ok2) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            if (ok2) margin_min(mg[M_RHO], std::fabs(rho) / std::max(std::max(std::fabs(currentChi), std::fabs(tempChi)), DBL_MIN));
            double scale = 0.;
            for (int j = 0; j < 7; j++) scale += x[j] * (lm.lambda * x[j] + v[28 + j]);
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && std::isfinite(tempChi)) {
                lm.lambda *= sd_s3_good_step_scale(rho);
                lm.ni = 2;
                currentChi = tempChi;
                lastRejected = false;
            } else {
                lm.lambda *= lm.ni;
                lm.ni *= 2;
                G.est = backup;             // pop: the edges keep the rejected trial's _error
                lastRejected = true;
                info[I_REJECTED]++;
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        trials += qmax; done = it + 1;
        if (qmax == 10) { stop = SD_SIM3_OPT_STOP_TRIALS; break; }
        if (rho == 0) { stop = SD_SIM3_OPT_STOP_RHO_ZERO; break; }
        margin_min(mg[M_STOP], std::fabs((iniChi - currentChi) * 1e3 - iniChi) / std::max(iniChi, DBL_MIN));
        if ((iniChi - currentChi) * 1e3 < iniChi) lm.nBad++; else lm.nBad = 0;
        if (lm.nBad >= 3) { stop = SD_SIM3_OPT_STOP_NO_GAIN; break; }
    }
    return done;
}

// the check after an optimize(): which correspondences have e12->chi2() > th2 || e21->chi2() > th2
void classify(Graph& G, const std::vector<int>& pair12, const std::vector<int>& pair21, double th2, int flags, std::vector<char>& bad,
              int64_t& staleDecides, double* mg)
{
    bad.assign(pair12.size(), 0);
    for (size_t i = 0; i < pair12.size(); i++) {
        if (pair12[i] < 0) continue;
        Edge a = G.edges[pair12[i]], b = G.edges[pair21[i]];
        Edge fa = a, fb = b;
        compute_error(G, fa, G.est); compute_error(G, fb, G.est);          // what a fresh computeError would give
        const bool fresh = sd_s3_chi2(fa.e0, fa.e1, fa.w) > th2 || sd_s3_chi2(fb.e0, fb.e1, fb.w) > th2;
        if (flags & TWIN_RECOMPUTE) { a = fa; b = fb; }
        const double x12 = sd_s3_chi2(a.e0, a.e1, a.w), x21 = sd_s3_chi2(b.e0, b.e1, b.w);
        margin_min(mg[M_CHI2], std::fabs(x12 - th2) / th2);
        if (!(flags & TWIN_SINGLE_CHI2)) margin_min(mg[M_CHI2], std::fabs(x21 - th2) / th2);
        const double f12 = sd_s3_chi2(fa.e0, fa.e1, fa.w), f21 = sd_s3_chi2(fb.e0, fb.e1, fb.w);
        const double far = std::max(std::fabs(x12 - f12), std::fabs(x21 - f21)) / th2;
        if (far == far && far > mg[M_STALE]) mg[M_STALE] = far;
        const bool cached = (flags & TWIN_SINGLE_CHI2) ? x12 > th2 : (x12 > th2 || x21 > th2);
        bad[i] = cached;
        if (cached != fresh) staleDecides++;
    }
}

void run(const sd_sim3_opt_problem& P, const sd_sim3_opt_corr* corr, int n, int flags, sd_sim3_opt_result& res, uint8_t* state, int64_t* info,
         double* mg)
{
    for (int k = 0; k < I_COUNT; k++) info[k] = 0;
    for (int k = 0; k < M_COUNT; k++) mg[k] = DBL_MAX;
    mg[M_STALE] = 0.0;
    Graph G;
    G.c1 = {(double)P.fx1, (double)P.fy1, (double)P.cx1, (double)P.cy1};
    G.c2 = {(double)P.fx2, (double)P.fy2, (double)P.cx2, (double)P.cy2};
    G.fix = P.fix_scale != 0;
    const double th2 = (double)P.th2;
    G.delta = (double)(float)std::sqrt(th2);
    sd_s3 prior;
    {
        double R[3][3];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i][j] = (double)P.R12[i * 3 + j];
        sd_s3_quat_of(R, prior);
        prior.t0 = P.t12[0]; prior.t1 = P.t12[1]; prior.t2 = P.t12[2]; prior.s = P.s12;
    }
    G.est = prior;
    G.wave = (flags & OPT_WAVE) != 0;
    std::vector<int> pair12(n), pair21(n);
    for (int i = 0; i < n; i++) {
        float a, b, c;
        Edge e12, e21;
        sd_s3_to_camera(P.Tcw2, corr[i].xw2[0], corr[i].xw2[1], corr[i].xw2[2], a, b, c);
        e12.inverse = false; e12.X = a; e12.Y = b; e12.Z = c; e12.u = corr[i].obs1[0]; e12.v = corr[i].obs1[1]; e12.w = corr[i].inv_sigma2_1;
        sd_s3_to_camera(P.Tcw1, corr[i].xw1[0], corr[i].xw1[1], corr[i].xw1[2], a, b, c);
        e21.inverse = true; e21.X = a; e21.Y = b; e21.Z = c; e21.u = corr[i].obs2[0]; e21.v = corr[i].obs2[1]; e21.w = corr[i].inv_sigma2_2;
        e12.corr = e21.corr = i; e12.e0 = e12.e1 = e21.e0 = e21.e1 = 0;
        pair12[i] = (int)G.edges.size(); G.edges.push_back(e12);
        pair21[i] = (int)G.edges.size(); G.edges.push_back(e21);
        state[i] = 0;
    }
    auto set_order = [&]() {
        G.order.clear();
        for (size_t k = 0; k < G.edges.size(); k++) G.order.push_back((int)k);
        if (flags & OPT_REVERSE) std::reverse(G.order.begin(), G.order.end());
    };
    set_order();
    memset(&res, 0, sizeof(res));
    res.n_correspondences = n;
    Lm lm;
    double x[7] = {0, 0, 0, 0, 0, 0, 0};
    bool lastRejected = false;
    std::vector<char> bad;
    // optimizer.initializeOptimization(); optimizer.optimize(5);
    res.iterations[0] = optimize(G, 5, flags, lm, true, x, res.trials[0], res.stop[0], lastRejected, info, mg);
    info[I_LAST_REJECTED_R1] = lastRejected;
    classify(G, pair12, pair21, th2, flags, bad, info[I_STALE_DECIDES_R1], mg);
    int nBad = 0;
    {
        std::vector<Edge> kept;
        for (int i = 0; i < n; i++) {
            if (bad[i]) { state[i] = 1; nBad++; pair12[i] = pair21[i] = -1; continue; }      // removeEdge
            const Edge a = G.edges[pair12[i]], b = G.edges[pair21[i]];
            pair12[i] = (int)kept.size(); kept.push_back(a);
            pair21[i] = (int)kept.size(); kept.push_back(b);
        }
        G.edges.swap(kept);
        set_order();
    }
    res.n_bad = nBad;
    res.more_iterations = nBad > 0 ? 10 : 5;
    sd_s3 out = prior;
    if (n - nBad < 10) {
        res.ret = 0;
        if (flags & TWIN_WRITE_ON_ZERO) { out = G.est; res.written = 1; }
    } else {
        res.iterations[1] = optimize(G, res.more_iterations, flags, lm, !(flags & TWIN_KEEP_LAMBDA), x, res.trials[1], res.stop[1], lastRejected,
                                     info, mg);
        info[I_LAST_REJECTED_R2] = lastRejected;
        classify(G, pair12, pair21, th2, flags, bad, info[I_STALE_DECIDES_R2], mg);
        int nIn = 0;
        for (int i = 0; i < n; i++) {
            if (pair12[i] < 0) continue;
            if (bad[i]) state[i] = 2; else nIn++;
        }
        res.ret = nIn; res.written = 1; out = G.est;
    }
    res.q[0] = out.qx; res.q[1] = out.qy; res.q[2] = out.qz; res.q[3] = out.qw;
    res.t[0] = out.t0; res.t[1] = out.t1; res.t[2] = out.t2; res.s = out.s;
    const double tx = 2 * out.qx, ty = 2 * out.qy, tz = 2 * out.qz;
    const double twx = tx * out.qw, twy = ty * out.qw, twz = tz * out.qw, txx = tx * out.qx, txy = ty * out.qx, txz = tz * out.qx;
    const double tyy = ty * out.qy, tyz = tz * out.qy, tzz = tz * out.qz;
    const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) res.T12[i * 4 + j] = (float)(out.s * R[i * 3 + j]);
    res.T12[3] = (float)out.t0; res.T12[7] = (float)out.t1; res.T12[11] = (float)out.t2; res.T12[15] = 1.f;
}

}  // namespace

extern "C" {

// info [16] int64, margins [4] double (see the enums above)
void sd_sim3_opt_oracle(const sd_sim3_opt_problem* P, const sd_sim3_opt_corr* corr, int n, int flags, sd_sim3_opt_result* res, uint8_t* state,
                        int64_t* info, double* margins)
{
    run(*P, corr, n, flags, *res, state, info, margins);
}

// problems [p0, p1) of packed tables; one call per host thread
void sd_sim3_opt_oracle_range(int p0, int p1, const int32_t* off, const sd_sim3_opt_corr* corr, const sd_sim3_opt_problem* problems, int flags,
                              sd_sim3_opt_result* res, uint8_t* state, int64_t* info, double* margins)
{
    for (int p = p0; p < p1; p++)
        run(problems[p], corr + off[p], off[p + 1] - off[p], flags, res[p], state + off[p], info + (size_t)p * I_COUNT, margins + (size_t)p * M_COUNT);
}

// Both Jacobians and the errors of one correspondence's two edges at the estimate est = (qx qy qz qw t0 t1 t2 s):
// Jnum / Jana [4][7] (rows: e12.x, e12.y, e21.x, e21.y), err [4]
void sd_sim3_opt_oracle_jacobians(const sd_sim3_opt_problem* P, const sd_sim3_opt_corr* c, const double* est, double* Jnum, double* Jana, double* err)
{
    Graph G;
    G.c1 = {(double)P->fx1, (double)P->fy1, (double)P->cx1, (double)P->cy1};
    G.c2 = {(double)P->fx2, (double)P->fy2, (double)P->cx2, (double)P->cy2};
    G.fix = P->fix_scale != 0; G.delta = 1;
    G.est = {est[0], est[1], est[2], est[3], est[4], est[5], est[6], est[7]};
    for (int k = 0; k < 2; k++) {
        float a, b, d;
        Edge e;
        e.inverse = k == 1; e.corr = 0;
        if (k == 0) { sd_s3_to_camera(P->Tcw2, c->xw2[0], c->xw2[1], c->xw2[2], a, b, d); e.u = c->obs1[0]; e.v = c->obs1[1]; e.w = c->inv_sigma2_1; }
        else { sd_s3_to_camera(P->Tcw1, c->xw1[0], c->xw1[1], c->xw1[2], a, b, d); e.u = c->obs2[0]; e.v = c->obs2[1]; e.w = c->inv_sigma2_2; }
        e.X = a; e.Y = b; e.Z = d;
        compute_error(G, e, G.est);
        err[2 * k] = e.e0; err[2 * k + 1] = e.e1;
        numeric_jacobian(G, e);
        for (int r = 0; r < 2; r++) for (int d2 = 0; d2 < 7; d2++) Jnum[(2 * k + r) * 7 + d2] = e.J[r][d2];
        double J[2][7];
        analytic_jacobian(G, e, G.est, J);
        for (int r = 0; r < 2; r++) for (int d2 = 0; d2 < 7; d2++) Jana[(2 * k + r) * 7 + d2] = J[r][d2];
    }
}

// Sim3(update) * est, for the branch tests: out = (qx qy qz qw t0 t1 t2 s); returns the branch
int sd_sim3_opt_oracle_oplus(const double* est, const double* update, int fix_scale, double* out)
{
    double u[7];
    for (int i = 0; i < 7; i++) u[i] = update[i];
    int br = 0;
    const sd_s3 S = {est[0], est[1], est[2], est[3], est[4], est[5], est[6], est[7]};
    const sd_s3 r = sd_s3_oplus(S, u, fix_scale != 0, br);
    out[0] = r.qx; out[1] = r.qy; out[2] = r.qz; out[3] = r.qw; out[4] = r.t0; out[5] = r.t1; out[6] = r.t2; out[7] = r.s;
    return br;
}

// activeRobustChi2 over the correspondences with live[i] != 0 at est, summed edge by edge in order
double sd_sim3_opt_oracle_objective(const sd_sim3_opt_problem* P, const sd_sim3_opt_corr* corr, int n, const uint8_t* live, const double* est)
{
    Graph G;
    G.c1 = {(double)P->fx1, (double)P->fy1, (double)P->cx1, (double)P->cy1};
    G.c2 = {(double)P->fx2, (double)P->fy2, (double)P->cx2, (double)P->cy2};
    G.delta = (double)(float)std::sqrt((double)P->th2);
    G.est = {est[0], est[1], est[2], est[3], est[4], est[5], est[6], est[7]};
    double s = 0.0;
    for (int i = 0; i < n; i++) {
        if (!live[i]) continue;
        for (int k = 0; k < 2; k++) {
            float a, b, d;
            Edge e;
            e.inverse = k == 1;
            if (k == 0) { sd_s3_to_camera(P->Tcw2, corr[i].xw2[0], corr[i].xw2[1], corr[i].xw2[2], a, b, d); e.u = corr[i].obs1[0]; e.v = corr[i].obs1[1]; e.w = corr[i].inv_sigma2_1; }
            else { sd_s3_to_camera(P->Tcw1, corr[i].xw1[0], corr[i].xw1[1], corr[i].xw1[2], a, b, d); e.u = corr[i].obs2[0]; e.v = corr[i].obs2[1]; e.w = corr[i].inv_sigma2_2; }
            e.X = a; e.Y = b; e.Z = d;
            compute_error(G, e, G.est);
            double r0, r1;
            sd_s3_huber(sd_s3_chi2(e.e0, e.e1, e.w), G.delta, r0, r1);
            s += r0;
        }
    }
    return s;
}

// the pieces of sd_sim3_math.h the kernel and the oracle share beyond the errors, exposed so that numpy can check them
int sd_sim3_opt_oracle_solve7(const double* H28, const double* b7, double lambda, double* x7)
{
    double x[7];
    for (int i = 0; i < 7; i++) x[i] = x7[i];
    const bool ok = sd_s3_solve7(H28, b7, lambda, x);
    for (int i = 0; i < 7; i++) x7[i] = x[i];
    return ok ? 1 : 0;
}

void sd_sim3_opt_oracle_accumulate(double e0, double e1, const double* J14, double w, double delta, double* v36)
{
    double J[2][7], v[36];
    for (int r = 0; r < 2; r++) for (int d = 0; d < 7; d++) J[r][d] = J14[r * 7 + d];
    for (int k = 0; k < 36; k++) v[k] = v36[k];
    sd_s3_accumulate(e0, e1, J, w, delta, v);
    for (int k = 0; k < 36; k++) v36[k] = v[k];
}

double sd_sim3_opt_oracle_good_step_scale(double rho) { return sd_s3_good_step_scale(rho); }

}  // extern "C"
