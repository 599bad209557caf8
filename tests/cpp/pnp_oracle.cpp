// TEST INFRASTRUCTURE: a literal, sequential restatement of PnPsolver (src/PnPsolver.cc, cited as PnP:line) for tests/pnp_cases.py --
// vectors, one iteration after the other, mnBestInliers / mvbBestInliers as members, returning at the first success.  Only the EPnP
// arithmetic is shared with the kernels (slam-dynamic_amd/csrc/sd_pnp_math.h); the control flow here is the reference's
// own loop, not the kernels' closed rule.  `order` picks how Refine sums over its inliers: 0 = the reference's sequential order, 1 =
// the refine kernel's tree order.  `twin` switches ONE deliberate mistake on, so that the tests can show each crafted case tells the
// right statement from its neighbour.  Built with -ffp-contract=off, and a second time with -ffp-contract=fast to measure the spread.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../slam-dynamic_amd/csrc/sd_pnp_math.h"

namespace {

struct Corr { float xw[3], uv[2], sigma2; int32_t tag; };
struct Problem { float fx, fy, cx, cy; uint64_t seed; int32_t start_iteration, n_iterations; };
struct Result {
    int32_t kind, no_more, iteration, n_inliers, best_iteration, best_inliers, n_refines, min_inliers, max_its, reserved;
    float Tcw[16];
};
static_assert(sizeof(Corr) == 28 && sizeof(Problem) == 32 && sizeof(Result) == 104, "records");

enum Twin { TWIN_NONE = 0, TWIN_REFINE_GE = 1, TWIN_BEST_GE = 2, TWIN_REFINE_CURRENT = 3, TWIN_LOOP_AND = 4, TWIN_ERR_LE = 5, TWIN_POW4 = 6 };

// info[] slots
enum { I_KIND, I_ITERATIONS, I_REFINE_CALLS, I_BEST_UPDATES, I_TIES, I_HYP_FLAGS, I_WIN1, I_WIN2, I_WIN3, I_REFINE_FLAGS, I_REFINE_WINNER,
       I_REFINE_FAILS, I_DISTINCT_REFINES, I_BELOW_MIN, I_COUNT };

unsigned long long splitmix64(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

struct Solver {
    std::vector<float> pts;                       // x y z u v maxError per correspondence (mvP3Dw, mvP2D, mvMaxError)
    int N = 0;
    sdpnp::Camera cam;
    uint64_t seed = 0;
    int order = 0, twin = 0;
    double mRi[9], mti[3];
    std::vector<uint8_t> mvbInliersi, mvbBestInliers, mvbRefinedInliers;
    int mnInliersi = 0, mnIterations = 0, mnBestInliers = 0, mnRefinedInliers = 0, mnBestIteration = 0;
    int mRansacMinInliers = 0, mRansacMaxIts = 0;
    float mBestTcw[16], mRefinedTcw[16];
    int64_t info[I_COUNT];
    int lastRefined = 0;
    double W[144], V[144];
    sdpnp::State S;

    Solver(const Problem& P, const Corr* c, int n, int order_, int twin_) : N(n), seed(P.seed), order(order_), twin(twin_)
    {
        cam = {(double)P.fx, (double)P.fy, (double)P.cx, (double)P.cy};
        pts.resize(6 * (size_t)n + 6);
        for (int i = 0; i < n; i++) { float* p = &pts[6 * i]; p[0] = c[i].xw[0]; p[1] = c[i].xw[1]; p[2] = c[i].xw[2]; p[3] = c[i].uv[0]; p[4] = c[i].uv[1]; p[5] = 0; }
        std::memset(info, 0, sizeof info);
        std::memset(mBestTcw, 0, sizeof mBestTcw);
        std::memset(mRefinedTcw, 0, sizeof mRefinedTcw);
    }

    // PnP:121-157
    void SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2, const Corr* c)
    {
        mRansacMinInliers = minInliers;
        mRansacMaxIts = maxIterations;
        float mRansacEpsilon = epsilon;
        mvbInliersi.assign(N, 0);
        int nMinInliers = N * mRansacEpsilon;
        if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
        if (nMinInliers < minSet) nMinInliers = minSet;
        mRansacMinInliers = nMinInliers;
        if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
        int nIterations;
        if (mRansacMinInliers == N) nIterations = 1;
        else {
            const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)mRansacEpsilon, twin == TWIN_POW4 ? 4.0 : 3.0)));
            nIterations = !(v < (double)maxIterations) ? maxIterations : (v <= 1.0 ? 1 : (int)v);      // the clamp of Q39
        }
        mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
        for (int i = 0; i < N; i++) pts[6 * i + 5] = c[i].sigma2 * th2;
    }

    void pose(const int* index, int n, bool refine)
    {
        sdpnp::PointSet set = {pts.data(), index, n};
        if (order == 1 && refine) { sdpnp::TreeCtx ctx = {set}; sdpnp::compute_pose(ctx, S, W, V, cam); }
        else { sdpnp::SeqCtx ctx = {set}; sdpnp::compute_pose(ctx, S, W, V, cam); }
        for (int k = 0; k < 9; k++) mRi[k] = S.R[k];
        for (int k = 0; k < 3; k++) mti[k] = S.t[k];
    }

    // PnP:308-339
    void CheckInliers()
    {
        mnInliersi = 0;
        for (int i = 0; i < N; i++) {
            const float* p = &pts[6 * i];
            bool in = sdpnp::check_inlier(mRi, mti, p[0], p[1], p[2], p[3], p[4], cam.fu, cam.fv, cam.uc, cam.vc, p[5]);
            if (twin == TWIN_ERR_LE && !in) {                         // error2 <= max: restated here, the shared test is strict
                const float Xc = (float)(mRi[0] * (double)p[0] + mRi[1] * (double)p[1] + mRi[2] * (double)p[2] + mti[0]);
                const float Yc = (float)(mRi[3] * (double)p[0] + mRi[4] * (double)p[1] + mRi[5] * (double)p[2] + mti[1]);
                const float invZc = (float)(1 / (mRi[6] * (double)p[0] + mRi[7] * (double)p[1] + mRi[8] * (double)p[2] + mti[2]));
                const double ue = cam.uc + cam.fu * (double)Xc * (double)invZc, ve = cam.vc + cam.fv * (double)Yc * (double)invZc;
                const float distX = (float)((double)p[3] - ue), distY = (float)((double)p[4] - ve);
                const float error2 = distX * distX + distY * distY;
                in = error2 <= p[5];
            }
            mvbInliersi[i] = in;
            if (in) mnInliersi++;
        }
    }

    int sample[4];
    // PnP:188-201 on a literal vector
    void draw()
    {
        std::vector<size_t> vAvailableIndices(N);
        for (int i = 0; i < N; i++) vAvailableIndices[i] = i;
        const unsigned long long base = splitmix64(seed) + 4ull * (unsigned long long)mnIterations;
        for (short i = 0; i < 4; ++i) {
            const int randi = (int)(splitmix64(base + (unsigned long long)i) % (unsigned long long)vAvailableIndices.size());
            sample[i] = (int)vAvailableIndices[randi];
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }

    void narrow(float* T)
    {
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T[4 * r + c] = (float)mRi[3 * r + c]; T[4 * r + 3] = (float)mti[r]; }
        T[12] = T[13] = T[14] = 0.f; T[15] = 1.f;
    }

    // PnP:260-305
    bool Refine()
    {
        const std::vector<uint8_t>& mask = twin == TWIN_REFINE_CURRENT ? mvbInliersi : mvbBestInliers;
        std::vector<int> vIndices;
        for (size_t i = 0; i < mask.size(); i++)
            if (mask[i]) vIndices.push_back((int)i);
        info[I_REFINE_CALLS]++;
        if (mnBestIteration != lastRefined) { info[I_DISTINCT_REFINES]++; lastRefined = mnBestIteration; }
        pose(vIndices.data(), (int)vIndices.size(), true);
        info[I_REFINE_FLAGS] |= S.flags; info[I_REFINE_WINNER] = S.winner;
        CheckInliers();
        mnRefinedInliers = mnInliersi;
        mvbRefinedInliers = mvbInliersi;
        if (twin == TWIN_REFINE_GE ? mnInliersi >= mRansacMinInliers : mnInliersi > mRansacMinInliers) { narrow(mRefinedTcw); return true; }
        info[I_REFINE_FAILS]++;
        return false;
    }

    // one pass of the loop body up to the best update (PnP:184-224); returns mnInliersi >= mRansacMinInliers
    bool hypothesis()
    {
        mnIterations++;
        draw();
        pose(sample, 4, false);
        info[I_HYP_FLAGS] |= S.flags; info[I_WIN1 + S.winner - 1]++;
        CheckInliers();
        if (mnInliersi == mRansacMinInliers - 1) info[I_BELOW_MIN]++;
        if (mnInliersi >= mRansacMinInliers) {
            if (mnInliersi == mnBestInliers) info[I_TIES]++;
            if (twin == TWIN_BEST_GE ? mnInliersi >= mnBestInliers : mnInliersi > mnBestInliers) {
                mvbBestInliers = mvbInliersi;
                mnBestInliers = mnInliersi;
                mnBestIteration = mnIterations;
                narrow(mBestTcw);
                info[I_BEST_UPDATES]++;
            }
            return true;
        }
        return false;
    }

    // PnP:165-258.  A call with start > 0 first replays iterations 1 .. start without Refine: that is the state the earlier calls left
    // (each of them either failed every Refine or returned, and the members keep the best of all iterations so far).
    void iterate(int start, int nIterations, Result& R, uint8_t* vbInliers)
    {
        std::memset(&R, 0, sizeof R);
        R.min_inliers = mRansacMinInliers; R.max_its = mRansacMaxIts;
        for (int i = 0; i < N; i++) vbInliers[i] = 0;
        if (N < mRansacMinInliers) { R.no_more = 1; info[I_KIND] = 0; return; }
        while (mnIterations < start) hypothesis();
        lastRefined = 0;
        for (int k = 0; k < I_COUNT; k++) if (k != I_HYP_FLAGS && k != I_WIN1 && k != I_WIN2 && k != I_WIN3) info[k] = 0;
        int nCurrentIterations = 0;
        while (twin == TWIN_LOOP_AND ? (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations)
                                     : (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations)) {
            nCurrentIterations++;
            if (hypothesis() && Refine()) {
                R.kind = 1; R.iteration = mnIterations; R.n_inliers = mnRefinedInliers;
                for (int i = 0; i < N; i++) vbInliers[i] = mvbRefinedInliers[i];
                std::memcpy(R.Tcw, mRefinedTcw, sizeof R.Tcw);
                finish(R);
                return;
            }
        }
        R.iteration = mnIterations;
        if (mnIterations >= mRansacMaxIts) {
            R.no_more = 1;
            if (mnBestInliers >= mRansacMinInliers) {
                R.kind = 2; R.n_inliers = mnBestInliers;
                for (int i = 0; i < N; i++) vbInliers[i] = mvbBestInliers[i];
                std::memcpy(R.Tcw, mBestTcw, sizeof R.Tcw);
            }
        }
        finish(R);
    }

    void finish(Result& R)
    {
        R.best_iteration = mnBestIteration; R.best_inliers = mnBestInliers; R.n_refines = (int)info[I_DISTINCT_REFINES];
        info[I_KIND] = R.kind; info[I_ITERATIONS] = mnIterations;
    }
};

void run(const Problem& P, const Corr* c, int n, double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2,
         int order, int twin, Result* res, uint8_t* inl, int64_t* info)
{
    Solver s(P, c, n, order, twin);
    s.SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, th2, c);
    s.iterate(P.start_iteration, P.n_iterations, *res, inl);
    if (info) std::memcpy(info, s.info, sizeof s.info);
}

}  // namespace

extern "C" {

int sd_pnp_oracle_info_count() { return I_COUNT; }

void sd_pnp_oracle_iterate(const Problem* P, const Corr* c, int n, double probability, int minInliers, int maxIterations, int minSet,
                           float epsilon, float th2, int order, int twin, Result* res, uint8_t* inl, int64_t* info)
{
    run(*P, c, n, probability, minInliers, maxIterations, minSet, epsilon, th2, order, twin, res, inl, info);
}

// problems [p0, p1) of packed tables, for the host-thread timings
void sd_pnp_oracle_iterate_range(int p0, int p1, const int32_t* off, const Corr* c, const Problem* P, double probability, int minInliers,
                                 int maxIterations, int minSet, float epsilon, float th2, int order, Result* res, uint8_t* inl, int64_t* info)
{
    for (int p = p0; p < p1; p++)
        run(P[p], c + off[p], off[p + 1] - off[p], probability, minInliers, maxIterations, minSet, epsilon, th2, order, 0, res + p, inl + off[p],
            info ? info + (size_t)p * I_COUNT : nullptr);
}

// the inlier count, pose (mRi row-major, mti: 12 doubles) and mask of EVERY iteration 1 .. n_its, each evaluated as the loop would
void sd_pnp_oracle_hypotheses(const Problem* P, const Corr* c, int n, float th2, int n_its, int32_t* counts, double* poses, uint8_t* masks)
{
    Solver s(*P, c, n, 0, 0);
    s.mvbInliersi.assign(n, 0);
    for (int i = 0; i < n; i++) s.pts[6 * i + 5] = c[i].sigma2 * th2;
    for (int it = 1; it <= n_its; it++) {
        s.mnIterations = it - 1;
        s.mnIterations++;
        s.draw();
        s.pose(s.sample, 4, false);
        s.CheckInliers();
        counts[it - 1] = s.mnInliersi;
        if (poses) { for (int k = 0; k < 9; k++) poses[12 * (it - 1) + k] = s.mRi[k]; for (int k = 0; k < 3; k++) poses[12 * (it - 1) + 9 + k] = s.mti[k]; }
        if (masks) for (int i = 0; i < n; i++) masks[(size_t)(it - 1) * n + i] = s.mvbInliersi[i];
    }
}

void sd_pnp_oracle_sample(uint64_t seed, int it, int N, int32_t* out)
{
    Problem P = {};
    P.seed = seed;
    Solver s(P, nullptr, 0, 0, 0);
    s.N = N; s.mnIterations = it;
    s.draw();
    for (int k = 0; k < 4; k++) out[k] = s.sample[k];
}

void sd_pnp_oracle_sample_closed(uint64_t seed, int it, int N, int32_t* out)
{
    int idx[4];
    sdpnp::sample4(seed, it, N, idx);
    for (int k = 0; k < 4; k++) out[k] = idx[k];
}

// compute_pose on n given points (6 floats each: x y z u v unused); out = mRi, mti (12 doubles); extra = winner, flags, rep[3], w12[12]
void sd_pnp_oracle_pose(const float* pts, int n, const double* cam4, int order, double* out, double* extra)
{
    static thread_local double W[144], V[144];
    sdpnp::State S;
    const sdpnp::Camera cam = {cam4[0], cam4[1], cam4[2], cam4[3]};
    sdpnp::PointSet set = {pts, nullptr, n};
    if (order == 1) { sdpnp::TreeCtx ctx = {set}; sdpnp::compute_pose(ctx, S, W, V, cam); }
    else { sdpnp::SeqCtx ctx = {set}; sdpnp::compute_pose(ctx, S, W, V, cam); }
    for (int k = 0; k < 9; k++) out[k] = S.R[k];
    for (int k = 0; k < 3; k++) out[9 + k] = S.t[k];
    if (extra) {
        extra[0] = S.winner; extra[1] = S.flags;
        for (int k = 0; k < 3; k++) extra[2 + k] = S.rep[k];
        for (int k = 0; k < 12; k++) extra[5 + k] = S.w12[S.perm12[k]];
    }
}

// CheckInliers of a pose (12 doubles) over n rows (x y z u v maxError); returns the count
int sd_pnp_oracle_check(const double* pose, const float* pts, int n, const double* cam4, uint8_t* mask)
{
    int cnt = 0;
    for (int i = 0; i < n; i++) {
        const float* p = pts + 6 * i;
        const bool in = sdpnp::check_inlier(pose, pose + 9, p[0], p[1], p[2], p[3], p[4], cam4[0], cam4[1], cam4[2], cam4[3], p[5]);
        if (mask) mask[i] = in;
        cnt += in;
    }
    return cnt;
}

// Refine (PnP:260-305) on a given mask over rows (x y z u v maxError): pose out (12 doubles), refined mask; returns the refined count
int sd_pnp_oracle_refine(const float* pts, int n, const uint8_t* mask, const double* cam4, int order, double* out, uint8_t* refined)
{
    std::vector<int> idx;
    for (int i = 0; i < n; i++) if (mask[i]) idx.push_back(i);
    static thread_local double W[144], V[144];
    sdpnp::State S;
    const sdpnp::Camera cam = {cam4[0], cam4[1], cam4[2], cam4[3]};
    sdpnp::PointSet set = {pts, idx.data(), (int)idx.size()};
    if (order == 1) { sdpnp::TreeCtx ctx = {set}; sdpnp::compute_pose(ctx, S, W, V, cam); }
    else { sdpnp::SeqCtx ctx = {set}; sdpnp::compute_pose(ctx, S, W, V, cam); }
    for (int k = 0; k < 9; k++) out[k] = S.R[k];
    for (int k = 0; k < 3; k++) out[9 + k] = S.t[k];
    return sd_pnp_oracle_check(out, pts, n, cam4, refined);
}

// SetRansacParameters: out = mRansacMinInliers, mRansacMaxIts
void sd_pnp_oracle_params(double probability, int minInliers, int maxIterations, int minSet, float epsilon, int N, int twin, int32_t* out)
{
    Problem P = {};
    std::vector<Corr> c(N > 0 ? N : 1);
    std::memset(c.data(), 0, c.size() * sizeof(Corr));
    Solver s(P, c.data(), N, 0, twin);
    s.SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, 1.f, c.data());
    out[0] = s.mRansacMinInliers; out[1] = s.mRansacMaxIts;
}

// the one SVD routine on an m x n matrix (row-major): w sorted descending, U (m x n) and V (n x n) with columns in that order
void sd_pnp_oracle_svd(const double* A, int m, int n, double* w, double* U, double* V)
{
    double Wm[144], Vm[144], wm[12];
    int perm[12];
    for (int i = 0; i < m * n; i++) Wm[i] = A[i];
    sdpnp::svd(m, n, Wm, Vm, wm, perm);
    for (int r = 0; r < n; r++) {
        const int j = perm[r];
        w[r] = wm[j];
        for (int k = 0; k < m; k++) U[k * n + r] = wm[j] == 0 ? 0.0 : Wm[k * n + j] / wm[j];
        for (int k = 0; k < n; k++) V[k * n + r] = Vm[k * n + j];
    }
}

}  // extern "C"
