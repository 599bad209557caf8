// ORB_SLAM2::PnPsolver (include/PnPsolver.h, src/PnPsolver.cc) over the device solver: a header-only mirror whose iterate() / find() are
// ONE sd_pnp_ransac_host call each.  The constructor takes plain arrays instead of a Frame: for every kept match, in
// key-point order, the world point, the undistorted key point, mvLevelSigma2[octave] and the key-point index (what PnPsolver.cc:79-101
// gathers), plus fx fy cx cy, the size of vpMapPointMatches and a sampler seed (the reference's DUtils::Random stream cannot be
// specified; the device sampler is counter-based).  mnIterations is kept across calls, so a second iterate(5) continues where the first
// stopped, exactly as the reference's members do.
// No OpenCV: a pose is 16 floats, row-major, `empty` when the reference returns cv::Mat().  Errors throw std::runtime_error.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "sd_frontend.h"

namespace ORB_SLAM2 {

struct PnPPose {
    bool isEmpty = true;
    float m[16] = {};
    bool empty() const { return isEmpty; }
    float at(int r, int c) const { return m[4 * r + c]; }
};

class PnPsolver {
public:
    PnPsolver(const std::vector<float>& p3Dw, const std::vector<float>& p2D, const std::vector<float>& sigma2, const std::vector<int>& keyPointIndices,
              size_t nMatches, float fx, float fy, float cx, float cy, uint64_t seed)
        : mnIterations(0), mnMatches(nMatches)
    {
        const size_t N = keyPointIndices.size();
        if (p3Dw.size() != 3 * N || p2D.size() != 2 * N || sigma2.size() != N) throw std::runtime_error("PnPsolver: array sizes differ");
        for (size_t i = 0; i < N; i++)                           // vbInliers is indexed by them (:233)
            if (keyPointIndices[i] < 0 || (size_t)keyPointIndices[i] >= nMatches) throw std::runtime_error("PnPsolver: a key-point index lies outside the matches");
        mCorr.resize(N);
        for (size_t i = 0; i < N; i++) {
            sd_pnp_corr& c = mCorr[i];
            c.xw[0] = p3Dw[3 * i]; c.xw[1] = p3Dw[3 * i + 1]; c.xw[2] = p3Dw[3 * i + 2];
            c.uv[0] = p2D[2 * i]; c.uv[1] = p2D[2 * i + 1];
            c.sigma2 = sigma2[i]; c.tag = keyPointIndices[i];
        }
        mProblem.fx = fx; mProblem.fy = fy; mProblem.cx = cx; mProblem.cy = cy; mProblem.seed = seed;
        mProblem.start_iteration = 0; mProblem.n_iterations = 1;
        SetRansacParameters();
    }

    // PnPsolver.cc:121-157: the arguments are kept and evaluated by the library on every call (the effective mRansacMinInliers /
    // mRansacMaxIts come back in mLast)
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f,
                             float th2 = 5.991f)
    {
        mProbability = probability; mMinInliers = minInliers; mMaxIterations = maxIterations; mMinSet = minSet; mEpsilon = epsilon; mTh2 = th2;
    }

    // PnPsolver.cc:159-163
    PnPPose find(std::vector<bool>& vbInliers, int& nInliers)
    {
        bool bFlag;
        // iterate(mRansacMaxIts): below mRansacMaxIts the loop runs up to it whatever nIterations <= it is (:182); at or beyond it,
        // mRansacMaxIts more iterations run.  The effective mRansacMaxIts is known from the last record (SetRansacParameters in between
        // is not followed); the count is clipped to the library's cap on start + n_iterations instead of being refused.
        int n = 1;
        if (mnIterations > 0) n = mnIterations < mLast.max_its ? mLast.max_its - mnIterations : mLast.max_its;
        if (n > SD_PNP_MAX_ITERATIONS - mnIterations) n = SD_PNP_MAX_ITERATIONS - mnIterations;
        return iterate(n > 1 ? n : 1, bFlag, vbInliers, nInliers);
    }

    // PnPsolver.cc:165-258
    PnPPose iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        const int32_t off[2] = {0, (int32_t)mCorr.size()};
        std::vector<uint8_t> inl(mCorr.size() + 1);
        mProblem.start_iteration = mnIterations; mProblem.n_iterations = nIterations;
        const int rc = sd_pnp_ransac_host(1, off, mCorr.data(), &mProblem, mProbability, mMinInliers, mMaxIterations, mMinSet, mEpsilon, mTh2,
                                          &mLast, inl.data(), nullptr, nullptr, 0);
        if (rc != SD_OK) throw std::runtime_error(std::string("PnPsolver::iterate: ") + sd_last_error());
        mnIterations = mLast.iteration;
        bNoMore = mLast.no_more != 0;
        vbInliers.clear();
        nInliers = 0;
        PnPPose T;
        if (mLast.kind == 0) return T;
        nInliers = mLast.n_inliers;
        vbInliers.assign(mnMatches, false);
        for (size_t i = 0; i < mCorr.size(); i++)
            if (inl[i]) vbInliers[mCorr[i].tag] = true;
        T.isEmpty = false;
        for (int k = 0; k < 16; k++) T.m[k] = mLast.Tcw[k];
        return T;
    }

    int mnIterations;                 // as the reference's member: iterations run so far
    sd_pnp_result mLast = {};         // the record of the last call (best_iteration, n_refines, min_inliers, max_its, ...)

private:
    std::vector<sd_pnp_corr> mCorr;
    sd_pnp_problem mProblem = {};
    size_t mnMatches;
    double mProbability = 0.99;
    int mMinInliers = 8, mMaxIterations = 300, mMinSet = 4;
    float mEpsilon = 0.4f, mTh2 = 5.991f;
};

}  // namespace ORB_SLAM2
