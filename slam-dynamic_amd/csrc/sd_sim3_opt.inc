// Optimizer::OptimizeSim3 on the device (include/sd_frontend.h, kernel in k_sim3_opt.h, DESIGN.md Q45).  Included by sd_api.hip inside
// its extern "C" block.  Stateless like sd_sim3_ransac_*: the problem table goes through an SdTableRing; the kernel needs no workspace.
static_assert(sizeof(sd_sim3_opt_corr) == 52 && sizeof(sd_sim3_opt_problem) == 220 && sizeof(sd_sim3_opt_result) == 176, "sim3_opt records");
static_assert(sizeof(SdSim3OptProb) == 228, "sim3_opt problem row");
namespace {
SdDeviceTable<SdTableRing<SdSim3OptProb>> g_sim3Opt;
}

// the host-side checks both entry points share; fills the problem table
static int sim3_opt_plan(int n, const int32_t* off, const sd_sim3_opt_problem* problems, std::vector<SdSim3OptProb>& tab)
{
    if (!off || !problems) return set_err(SD_ERR_INVALID, "bad sim3_optimize arguments");
    if (n > SD_SIM3_MAX_PROBLEMS) return set_err(SD_ERR_INVALID, "sim3_optimize: more than 65535 problems in one call");
    SD_TRY(check_offsets("sim3_optimize", off, n, nullptr));
    tab.resize(n);
    for (int p = 0; p < n; p++) {
        const int N = off[p + 1] - off[p];
        if (N > SD_SIM3_MAX_CORRESPONDENCES)
            return set_err(SD_ERR_INVALID, "sim3_optimize problem " + std::to_string(p) + " holds more than 4096 correspondences");
        const sd_sim3_opt_problem& P = problems[p];
        if (!(P.th2 > 0) || !std::isfinite(P.th2)) return set_err(SD_ERR_INVALID, "sim3_optimize problem " + std::to_string(p) + ": th2 must be positive");
        bool finite = std::isfinite(P.s12);
        for (int k = 0; k < 9; k++) finite = finite && std::isfinite(P.R12[k]);
        for (int k = 0; k < 3; k++) finite = finite && std::isfinite(P.t12[k]);
        if (!finite) return set_err(SD_ERR_INVALID, "sim3_optimize problem " + std::to_string(p) + ": the prior is not finite");
        tab[p].P = P; tab[p].c0 = off[p]; tab[p].n = N;
    }
    return SD_OK;
}

int sd_sim3_optimize_device(int n_problems, const int32_t* corr_offset, const sd_sim3_opt_corr* d_corr,
                            const sd_sim3_opt_problem* problems, sd_sim3_opt_result* d_results, uint8_t* d_state, void* stream_)
{
    if (n_problems < 0) return set_err(SD_ERR_INVALID, "bad sim3_optimize arguments");
    if (n_problems == 0) return SD_OK;
    std::vector<SdSim3OptProb> tab;
    int rc = sim3_opt_plan(n_problems, corr_offset, problems, tab);
    if (rc != SD_OK) return rc;
    const size_t nC = (size_t)corr_offset[n_problems];
    if (!d_results || (nC && (!d_corr || !d_state))) return set_err(SD_ERR_INVALID, "bad sim3_optimize arguments");
    hipStream_t s = (hipStream_t)stream_;
    decltype(g_sim3Opt)::Locked ring;
    SD_TRY(g_sim3Opt.lock("sim3_optimize", ring));
    SdSim3OptArgs A;
    SD_TRY(ring->stage(tab.data(), (size_t)n_problems, s, A.prob));
    A.corr = d_corr; A.result = d_results; A.state = d_state;
    hipLaunchKernelGGL(k_sim3_optimize, dim3(n_problems), dim3(64), 0, s, A);
    LAUNCH_CHECK("k_sim3_optimize");
    return ring->publish(s);
}

int sd_sim3_optimize_host(int n_problems, const int32_t* corr_offset, const sd_sim3_opt_corr* corr, const sd_sim3_opt_problem* problems,
                          sd_sim3_opt_result* results, uint8_t* state)
{
    if (n_problems < 0) return set_err(SD_ERR_INVALID, "bad sim3_optimize arguments");
    if (n_problems == 0) return SD_OK;
    std::vector<SdSim3OptProb> tab;
    int rc = sim3_opt_plan(n_problems, corr_offset, problems, tab);
    if (rc != SD_OK) return rc;
    const size_t nC = (size_t)corr_offset[n_problems];
    if (!results || (nC && (!corr || !state))) return set_err(SD_ERR_INVALID, "bad sim3_optimize arguments");
    rc = require_device();
    if (rc != SD_OK) return rc;
    SdDevBuf<sd_sim3_opt_corr> d_c; SdDevBuf<sd_sim3_opt_result> d_r; SdDevBuf<uint8_t> d_s;
    HIPCHK(d_c.alloc(std::max<size_t>(nC, 1) * sizeof(sd_sim3_opt_corr))); HIPCHK(d_r.alloc((size_t)n_problems * sizeof(sd_sim3_opt_result)));
    HIPCHK(d_s.alloc(std::max<size_t>(nC, 1)));
    if (nC) HIPCHK(hipMemcpy(d_c, corr, nC * sizeof(sd_sim3_opt_corr), hipMemcpyHostToDevice));
    rc = sd_sim3_optimize_device(n_problems, corr_offset, d_c, problems, d_r, d_s, nullptr);
    if (rc != SD_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(results, d_r, (size_t)n_problems * sizeof(sd_sim3_opt_result), hipMemcpyDeviceToHost));
    if (nC) HIPCHK(hipMemcpy(state, d_s, nC, hipMemcpyDeviceToHost));
    return SD_OK;
}
