// PnPsolver on the device (include/sd_frontend.h, kernels in k_pnp.h, arithmetic in sd_pnp_math.h, DESIGN.md Q46).  Included by
// sd_api.hip inside its extern "C" block.  Stateless like sd_sim3_ransac_*: the problem table goes through an SdTableRing, the scratch
// arrays sit behind an SdWorkspace, which sd_pnp_ransac_device shares with the PnP stage of sd_batch_relocalize_pnp.
static_assert(sizeof(sd_pnp_corr) == 28 && sizeof(sd_pnp_problem) == 32 && sizeof(sd_pnp_result) == 104, "pnp records");
static_assert(sizeof(SdPnpPt) == 24 && sizeof(SdPnpHyp) == 96 && sizeof(SdPnpProb) == 64, "pnp workspace records");
static_assert(SD_PNP_MAX_N == SD_PNP_MAX_CORRESPONDENCES && SD_PNP_MAX_ITS == SD_PNP_MAX_ITERATIONS, "pnp caps");
static_assert(SD_PNP_MAX_PROBLEMS <= 65535, "a problem is a grid row");
namespace {
struct PnpState {
    SdTableRing<SdPnpProb> prob;
    SdWorkspace ws; SdDevBuf<SdPnpPt> pts; SdDevBuf<SdPnpHyp> hyp; SdDevBuf<int> count; size_t capPts = 0, capHyp = 0;
    // the workspace entered on `s` with room for needPts points and needHyp hypotheses
    int enter(hipStream_t s, size_t needPts, size_t needHyp)
    {
        SD_TRY(ws.enter(s, capPts < needPts || capHyp < needHyp));
        SD_TRY(SdWorkspace::grow(capPts, needPts, {{&pts, sizeof(SdPnpPt)}}));
        return SdWorkspace::grow(capHyp, needHyp, {{&hyp, sizeof(SdPnpHyp)}, {&count, sizeof(int)}});
    }
};
SdDeviceTable<PnpState> g_pnp;
}

// PnPsolver::SetRansacParameters (PnPsolver.cc:121-157) as written: `int nMinInliers = N*epsilon` through float, the epsilon raise,
// pow(epsilon, 3) although the minimal set is 4, mRansacMinInliers == N -> 1.  The double is clamped before the conversion to int as
// sim3_max_its does (Q39), so that no value of it is undefined.
static void pnp_ransac_parameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, int N, int& minOut, int& itsOut)
{
    int nMinInliers = (int)((float)N * epsilon);
    if (nMinInliers < minInliers) nMinInliers = minInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    float eps = epsilon;
    if (eps < (float)nMinInliers / N) eps = (float)nMinInliers / N;
    int nIterations;
    if (nMinInliers == N) nIterations = 1;
    else {
        const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)eps, 3.0)));
        nIterations = !(v < (double)maxIterations) ? maxIterations : (v <= 1.0 ? 1 : (int)v);
    }
    minOut = nMinInliers;
    itsOut = std::max(1, std::min(nIterations, maxIterations));
}

// the host-side checks both entry points share; fills the problem table
static int pnp_plan(int n, const int32_t* off, const sd_pnp_problem* problems, double probability, int minInliers, int maxIterations, int minSet,
                    float epsilon, float th2, std::vector<SdPnpProb>& tab, size_t& nHyp, int& maxN, int& maxEnd)
{
    if (!off || !problems) return set_err(SD_ERR_INVALID, "bad pnp_ransac arguments");
    if (minSet != 4) return set_err(SD_ERR_INVALID, "pnp_ransac min_set must be 4");
    if (!(probability > 0.0 && probability < 1.0)) return set_err(SD_ERR_INVALID, "pnp_ransac probability must lie in (0, 1)");
    if (minInliers < 0) return set_err(SD_ERR_INVALID, "pnp_ransac min_inliers must not be negative");
    if (maxIterations < 1 || maxIterations > SD_PNP_MAX_ITS) return set_err(SD_ERR_INVALID, "pnp_ransac max_iterations outside [1, 4096]");
    if (!(epsilon > 0.f && epsilon <= 1.f)) return set_err(SD_ERR_INVALID, "pnp_ransac epsilon must lie in (0, 1]");
    if (!(th2 > 0.f)) return set_err(SD_ERR_INVALID, "pnp_ransac th2 must be positive");
    if (n > SD_PNP_MAX_PROBLEMS) return set_err(SD_ERR_INVALID, "pnp_ransac: more than 65535 problems in one call");
    SD_TRY(check_offsets("pnp_ransac", off, n, nullptr));
    tab.resize(n);
    nHyp = 0; maxN = 0; maxEnd = 0;
    for (int p = 0; p < n; p++) {
        const int N = off[p + 1] - off[p];
        if (N > SD_PNP_MAX_N) return set_err(SD_ERR_INVALID, "pnp_ransac problem " + std::to_string(p) + " holds more than 4096 correspondences");
        const sd_pnp_problem& P = problems[p];
        if (P.start_iteration < 0 || P.n_iterations < 1 || (long long)P.start_iteration + P.n_iterations > SD_PNP_MAX_ITS)
            return set_err(SD_ERR_INVALID, "pnp_ransac problem " + std::to_string(p) + ": start_iteration + n_iterations outside [1, 4096]");
        SdPnpProb& q = tab[p];
        q.P = P; q.c0 = off[p]; q.n = N; q.th2 = th2; q.pad = 0;
        pnp_ransac_parameters(probability, minInliers, maxIterations, minSet, epsilon, N, q.minInliers, q.maxIts);
        q.end = N < q.minInliers ? 0 : std::max(q.maxIts, P.start_iteration + P.n_iterations);
        q.h0 = (int)nHyp;
        nHyp += (size_t)q.end;
        maxN = std::max(maxN, q.n); maxEnd = std::max(maxEnd, q.end);
    }
    if (nHyp > (size_t)0x7FFFFFFF) return set_err(SD_ERR_INVALID, "pnp_ransac: more than 2^31 hypotheses in one call");
    return SD_OK;
}

int sd_pnp_ransac_device(int n_problems, const int32_t* corr_offset, const sd_pnp_corr* d_corr, const sd_pnp_problem* problems,
                         double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2,
                         sd_pnp_result* d_results, uint8_t* d_inliers, int32_t* d_counts, double* d_poses, int counts_stride, void* stream_)
{
    if (n_problems < 0) return set_err(SD_ERR_INVALID, "bad pnp_ransac arguments");
    if (n_problems == 0) return SD_OK;
    std::vector<SdPnpProb> tab;
    size_t nHyp = 0;
    int maxN = 0, maxEnd = 0;
    int rc = pnp_plan(n_problems, corr_offset, problems, probability, min_inliers, max_iterations, min_set, epsilon, th2, tab, nHyp, maxN, maxEnd);
    if (rc != SD_OK) return rc;
    const size_t nC = (size_t)corr_offset[n_problems];
    if (!d_results || (nC && (!d_corr || !d_inliers))) return set_err(SD_ERR_INVALID, "bad pnp_ransac arguments");
    if ((d_counts || d_poses) && counts_stride < maxEnd) return set_err(SD_ERR_INVALID, "pnp_ransac counts_stride is smaller than a problem's iteration count");
    hipStream_t s = (hipStream_t)stream_;
    HIPCHK(sd_raise_lds_limit((const void*)k_pnp_hypotheses, SD_PNP_HYP_LDS));
    decltype(g_pnp)::Locked B;
    SD_TRY(g_pnp.lock("pnp_ransac", B));
    SdPnpArgs A;
    SD_TRY(B->prob.stage(tab.data(), (size_t)n_problems, s, A.prob));
    SD_TRY(B->enter(s, std::max<size_t>(nC, 1), std::max<size_t>(nHyp, 1)));
    A.corr = d_corr; A.pts = B->pts; A.hyp = B->hyp; A.count = B->count; A.result = d_results; A.inlier = d_inliers;
    if (maxN > 0) {
        hipLaunchKernelGGL(k_pnp_prepare, dim3(std::max(1, (maxN + 255) / 256), n_problems), dim3(256), 0, s, A);
        LAUNCH_CHECK("k_pnp_prepare");
    }
    if (maxEnd > 0) {
        hipLaunchKernelGGL(k_pnp_hypotheses, dim3((maxEnd + 63) / 64, n_problems), dim3(64), SD_PNP_HYP_LDS, s, A);
        LAUNCH_CHECK("k_pnp_hypotheses");
        hipLaunchKernelGGL(k_pnp_count, dim3((maxEnd + SD_PNP_HYP_PER_BLOCK - 1) / SD_PNP_HYP_PER_BLOCK, n_problems), dim3(256), 0, s, A);
        LAUNCH_CHECK("k_pnp_count");
        if (d_counts || d_poses) {
            hipLaunchKernelGGL(k_pnp_copy_counts, dim3((maxEnd + 255) / 256, n_problems), dim3(256), 0, s, A, d_counts, d_poses, counts_stride);
            LAUNCH_CHECK("k_pnp_copy_counts");
        }
    }
    hipLaunchKernelGGL(k_pnp_refine, dim3(n_problems), dim3(256), 0, s, A);
    LAUNCH_CHECK("k_pnp_refine");
    SD_TRY(B->ws.leave(s));
    return B->prob.publish(s);
}

int sd_pnp_ransac_host(int n_problems, const int32_t* corr_offset, const sd_pnp_corr* corr, const sd_pnp_problem* problems,
                       double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2,
                       sd_pnp_result* results, uint8_t* inliers, int32_t* counts, double* poses, int counts_stride)
{
    if (n_problems < 0) return set_err(SD_ERR_INVALID, "bad pnp_ransac arguments");
    if (n_problems == 0) return SD_OK;
    std::vector<SdPnpProb> tab;
    size_t nHyp = 0;
    int maxN = 0, maxEnd = 0;
    int rc = pnp_plan(n_problems, corr_offset, problems, probability, min_inliers, max_iterations, min_set, epsilon, th2, tab, nHyp, maxN, maxEnd);
    if (rc != SD_OK) return rc;
    const size_t nC = (size_t)corr_offset[n_problems];
    if (!results || (nC && (!corr || !inliers))) return set_err(SD_ERR_INVALID, "bad pnp_ransac arguments");
    if ((counts || poses) && (counts_stride < maxEnd || counts_stride < 1)) return set_err(SD_ERR_INVALID, "pnp_ransac counts_stride is smaller than a problem's iteration count");
    rc = require_device();
    if (rc != SD_OK) return rc;
    SdDevBuf<sd_pnp_corr> d_c; SdDevBuf<sd_pnp_result> d_r; SdDevBuf<uint8_t> d_i; SdDevBuf<int32_t> d_n; SdDevBuf<double> d_p;
    const size_t nCounts = counts ? (size_t)n_problems * counts_stride : 0, nPoses = poses ? (size_t)n_problems * counts_stride * 12 : 0;
    HIPCHK(d_c.alloc(std::max<size_t>(nC, 1) * sizeof(sd_pnp_corr))); HIPCHK(d_r.alloc((size_t)n_problems * sizeof(sd_pnp_result)));
    HIPCHK(d_i.alloc(std::max<size_t>(nC, 1)));
    if (nCounts) { HIPCHK(d_n.alloc(nCounts * 4)); HIPCHK(hipMemset(d_n, 0, nCounts * 4)); }
    if (nPoses) { HIPCHK(d_p.alloc(nPoses * 8)); HIPCHK(hipMemset(d_p, 0, nPoses * 8)); }
    if (nC) HIPCHK(hipMemcpy(d_c, corr, nC * sizeof(sd_pnp_corr), hipMemcpyHostToDevice));
    rc = sd_pnp_ransac_device(n_problems, corr_offset, d_c, problems, probability, min_inliers, max_iterations, min_set, epsilon, th2, d_r, d_i,
                              nCounts ? (int32_t*)d_n : nullptr, nPoses ? (double*)d_p : nullptr, counts_stride, nullptr);
    if (rc != SD_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(results, d_r, (size_t)n_problems * sizeof(sd_pnp_result), hipMemcpyDeviceToHost));
    if (nC) HIPCHK(hipMemcpy(inliers, d_i, nC, hipMemcpyDeviceToHost));
    if (nCounts) HIPCHK(hipMemcpy(counts, d_n, nCounts * 4, hipMemcpyDeviceToHost));
    if (nPoses) HIPCHK(hipMemcpy(poses, d_p, nPoses * 8, hipMemcpyDeviceToHost));
    return SD_OK;
}

// ---------------------------------------------------------------- Tracking::Relocalization 2256-2358 as one launch sequence
// gather (k_pnp_gather) -> the PnP stage against the caps -> the hand-over (k_pnp_handover) -> the cascade of sd_reloc.inc from the device pose
int sd_batch_relocalize_pnp(sd_batch* b, int n_jobs, const int32_t* frame_index, const int32_t* kf_index, const sd_pnp_problem* problems,
                            double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2,
                            const int32_t* d_bow_match, const int32_t* d_kf_point, const sd_map_point* d_points, const uint8_t* d_point_desc,
                            int n_points, const sd_camera* cam, sd_reloc_result** d_results, void* stream_)
{
    if (d_results) *d_results = nullptr;
    if (!b || n_jobs < 0 || n_jobs > SD_RELOC_MAX_JOBS || n_points < 0 || !cam_ok(cam) ||
        (n_jobs > 0 && (!frame_index || !kf_index || !problems || !d_bow_match || !d_kf_point)))
        return set_err(SD_ERR_INVALID, "bad relocalize_pnp arguments");
    if (min_set != 4) return set_err(SD_ERR_INVALID, "relocalize_pnp min_set must be 4");
    if (!(probability > 0.0 && probability < 1.0)) return set_err(SD_ERR_INVALID, "relocalize_pnp probability must lie in (0, 1)");
    if (min_inliers < 0) return set_err(SD_ERR_INVALID, "relocalize_pnp min_inliers must not be negative");
    if (max_iterations < 1 || max_iterations > SD_PNP_MAX_ITS) return set_err(SD_ERR_INVALID, "relocalize_pnp max_iterations outside [1, 4096]");
    if (!(epsilon > 0.f && epsilon <= 1.f)) return set_err(SD_ERR_INVALID, "relocalize_pnp epsilon must lie in (0, 1]");
    if (!(th2 > 0.f)) return set_err(SD_ERR_INVALID, "relocalize_pnp th2 must be positive");
    b->relocRefine.jobs = 0; b->relocPnp.jobs = 0;
    if (n_jobs == 0) return SD_OK;
    int endCap = max_iterations;
    for (int j = 0; j < n_jobs; j++) {
        const sd_pnp_problem& P = problems[j];
        if (P.start_iteration < 0 || P.n_iterations < 1 || (long long)P.start_iteration + P.n_iterations > SD_PNP_MAX_ITS)
            return set_err(SD_ERR_INVALID, "relocalize_pnp job " + std::to_string(j) + ": start_iteration + n_iterations outside [1, 4096]");
        endCap = std::max(endCap, P.start_iteration + P.n_iterations);
    }
    int rc = check_slots(b, "relocalize_pnp", frame_index, kf_index, n_jobs, SD_SLOT_RANGE);
    if (rc == SD_OK) rc = check_slots(b, "relocalize_pnp", frame_index, kf_index, n_jobs, SD_SLOT_RESULTS | SD_SLOT_GRID);
    if (rc != SD_OK) return rc;
    if (n_points > 0 && (!d_points || !d_point_desc)) return set_err(SD_ERR_INVALID, "relocalize_pnp: n_points but no map points given");
    const int cap = b->plan.kpCap;
    if (cap > SD_PNP_MAX_N) return set_err(SD_ERR_UNSUPPORTED, "relocalize_pnp: more than 4096 keypoints per image");      // a problem's cap; never a truncation
    const size_t J = (size_t)n_jobs, nHyp = J * (size_t)endCap, nPts = J * (size_t)cap;
    if (nHyp > (size_t)0x7FFFFFFF) return set_err(SD_ERR_INVALID, "relocalize_pnp: more than 2^31 hypotheses in one call");
    HIPCHK(sd_raise_lds_limit((const void*)k_pnp_hypotheses, SD_PNP_HYP_LDS));
    hipStream_t s = pick_stream(b, stream_);
    rc = b->reloc.grow(b, s, n_jobs);                              // the slot table is the matcher's, as in the cascade
    if (rc == SD_OK) rc = b->relocPnp.grow(b, s, n_jobs);
    if (rc != SD_OK) return rc;
    b->reloc.jobs = 0;
    sd_batch::RelocPnp& R = b->relocPnp;
    R.table.resize((size_t)cap + 1);
    for (int N = 0; N <= cap; N++) pnp_ransac_parameters(probability, min_inliers, max_iterations, min_set, epsilon, N, R.table[N].x, R.table[N].y);
    b->reloc.slots.resize(n_jobs);
    for (int j = 0; j < n_jobs; j++) b->reloc.slots[j] = make_int2(frame_index[j], kf_index[j]);
    HIPCHK(hipMemcpyAsync(b->reloc.d_slots, b->reloc.slots.data(), J * sizeof(int2), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(R.d_table, R.table.data(), ((size_t)cap + 1) * sizeof(int2), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(R.d_in, problems, J * sizeof(sd_pnp_problem), hipMemcpyHostToDevice, s));
    {
        decltype(g_pnp)::Locked B;
        SD_TRY(g_pnp.lock("relocalize_pnp", B));
        SD_TRY(B->enter(s, nPts, nHyp));
        SdPnpChainArgs G;
        G.kp = KPUN(b); G.count = b->d_count; G.slots = b->reloc.d_slots; G.match = d_bow_match; G.mps = (const SdMapPoint*)d_points; G.nPoints = n_points;
        G.cap = cap; G.in = R.d_in; G.table = R.d_table; G.corr = R.d_corr; G.prob = R.d_prob; G.th2 = th2; G.endCap = endCap; G.row = R.d_row; G.T = R.d_T;
        G.result = R.d_res; G.inlier = R.d_inl;
        SdPnpArgs A;
        A.prob = R.d_prob; A.corr = R.d_corr; A.pts = B->pts; A.hyp = B->hyp; A.count = B->count; A.result = R.d_res; A.inlier = R.d_inl;
        hipLaunchKernelGGL(k_pnp_gather, dim3(n_jobs), dim3(256), 0, s, G, level_tables(b));
        LAUNCH_CHECK("k_pnp_gather");
        hipLaunchKernelGGL(k_pnp_prepare, dim3((cap + 255) / 256, n_jobs), dim3(256), 0, s, A);
        LAUNCH_CHECK("k_pnp_prepare");
        hipLaunchKernelGGL(k_pnp_hypotheses, dim3((endCap + 63) / 64, n_jobs), dim3(64), SD_PNP_HYP_LDS, s, A);
        LAUNCH_CHECK("k_pnp_hypotheses");
        hipLaunchKernelGGL(k_pnp_count, dim3((endCap + SD_PNP_HYP_PER_BLOCK - 1) / SD_PNP_HYP_PER_BLOCK, n_jobs), dim3(256), 0, s, A);
        LAUNCH_CHECK("k_pnp_count");
        hipLaunchKernelGGL(k_pnp_refine, dim3(n_jobs), dim3(256), 0, s, A);
        LAUNCH_CHECK("k_pnp_refine");
        hipLaunchKernelGGL(k_pnp_handover, dim3(n_jobs), dim3(256), 0, s, G);
        LAUNCH_CHECK("k_pnp_handover");
        SD_TRY(B->ws.leave(s));
    }
    rc = reloc_refine_run(b, n_jobs, frame_index, kf_index, nullptr, R.d_T, d_kf_point, R.d_row, d_points, d_point_desc, n_points, cam, d_results, s);
    if (rc != SD_OK) return rc;
    R.jobs = n_jobs;
    return SD_OK;
}

int sd_batch_download_reloc_pnp(sd_batch* b, int job, sd_pnp_result* pnp, int32_t* n_corr, sd_pnp_corr* corr, uint8_t* inliers, int32_t* row,
                                sd_reloc_result* result, int32_t* frame_point, uint8_t* outlier, int cap)
{
    if (!b || job < 0 || job >= b->relocPnp.jobs) return set_err(SD_ERR_INVALID, "download_reloc_pnp: no such job in the last sd_batch_relocalize_pnp");
    int rc = sd_batch_download_reloc(b, job, result, frame_point, outlier, cap);          // synchronises and reports a point outside its table
    if (rc != SD_OK) return rc;
    const size_t n = (size_t)b->plan.kpCap;
    if ((corr || inliers || row) && cap < b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "the reloc rows need kp_capacity entries");
    sd_batch::RelocPnp& R = b->relocPnp;
    if (pnp) HIPCHK(hipMemcpy(pnp, R.d_res + job, sizeof(sd_pnp_result), hipMemcpyDeviceToHost));
    if (n_corr) {
        SdPnpProb q;
        HIPCHK(hipMemcpy(&q, R.d_prob + job, sizeof q, hipMemcpyDeviceToHost));
        *n_corr = q.n;
    }
    if (corr) HIPCHK(hipMemcpy(corr, R.d_corr + (size_t)job * n, n * sizeof(sd_pnp_corr), hipMemcpyDeviceToHost));
    if (inliers) HIPCHK(hipMemcpy(inliers, R.d_inl + (size_t)job * n, n, hipMemcpyDeviceToHost));
    if (row) HIPCHK(hipMemcpy(row, R.d_row + (size_t)job * n, n * 4, hipMemcpyDeviceToHost));
    return SD_OK;
}
