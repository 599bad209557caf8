// LoopClosing::ComputeSim3's refine chain (include/sd_frontend.h, kernels in k_sim3_refine.h, DESIGN.md Q45).  Included by sd_api.hip
// inside its extern "C" block.  Six launches and four memsets per call, whatever the number of jobs; no host synchronisation except
// when the library-owned tables grow.
static_assert(sizeof(sd_sim3_refine_result) == 320 && sizeof(SdRefineJob) == 144, "sim3 refine records");

static int ensure_refine(sd_batch* b, int n_jobs, hipStream_t s)
{
    if (n_jobs <= b->rfJobCap) return SD_OK;
    HIPCHK(hipStreamSynchronize(s));
    const size_t want = (size_t)std::max(n_jobs, 2 * b->rfJobCap), rows = want * b->plan.kpCap;
    b->rfJobCap = 0; b->rfJobs = 0;
    b->d_rfJobs.reset(); b->d_rfMerged.reset(); b->d_rfFinal.reset(); b->d_rfCorr.reset(); b->d_rfProb.reset(); b->d_rfOpt.reset();
    b->d_rfState.reset(); b->d_rfOut.reset();
    HIPCHK(b->d_rfJobs.alloc(want * sizeof(SdRefineJob))); HIPCHK(b->d_rfMerged.alloc(rows * 4)); HIPCHK(b->d_rfFinal.alloc(rows * 4));
    HIPCHK(b->d_rfCorr.alloc(rows * sizeof(sd_sim3_opt_corr))); HIPCHK(b->d_rfProb.alloc(want * sizeof(SdSim3OptProb)));
    HIPCHK(b->d_rfOpt.alloc(want * sizeof(sd_sim3_opt_result))); HIPCHK(b->d_rfState.alloc(rows)); HIPCHK(b->d_rfOut.alloc(want * sizeof(sd_sim3_refine_result)));
    b->rfJobCap = (int)want;
    return SD_OK;
}

int sd_batch_compute_sim3_refine(sd_batch* b, int n_jobs, const int32_t* kf1_index, const int32_t* kf2_index, const float* Tcw1_host,
                                 const float* Tcw2_host, const sd_sim3_result* d_ransac, const int32_t* corr_offset, const sd_sim3_corr* d_corr,
                                 const uint8_t* d_inliers, const int32_t* d_bow12, const sd_camera* cam, float th, float th2, int fix_scale,
                                 const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points, const int32_t* d_kf1_point,
                                 const int32_t* d_kf2_point, void* stream_)
{
    if (!b || n_jobs < 0 || n_jobs > 32767 || n_points < 0 || !cam_ok(cam) || !(th > 0) || !(th2 > 0) || !std::isfinite(th2) ||
        (n_jobs > 0 && (!kf1_index || !kf2_index || !Tcw1_host || !Tcw2_host || !d_ransac || !corr_offset || !d_bow12 || !d_kf1_point || !d_kf2_point)))
        return set_err(SD_ERR_INVALID, "bad compute_sim3_refine arguments");
    b->rfJobs = 0; b->s3Pairs = 0;
    if (n_jobs == 0) return SD_OK;
    if (n_points > 0 && (!d_points || !d_point_desc)) return set_err(SD_ERR_INVALID, "compute_sim3_refine: n_points but no point table");
    if (corr_offset[0] != 0) return set_err(SD_ERR_INVALID, "compute_sim3_refine: corr_offset must start at 0 and ascend");
    for (int j = 0; j < n_jobs; j++) {
        if (corr_offset[j + 1] < corr_offset[j]) return set_err(SD_ERR_INVALID, "compute_sim3_refine: corr_offset must start at 0 and ascend");
        if (kf1_index[j] < 0 || kf1_index[j] >= b->maxImages || kf2_index[j] < 0 || kf2_index[j] >= b->maxImages)
            return set_err(SD_ERR_INVALID, "compute_sim3_refine: slot out of range");
    }
    if (corr_offset[n_jobs] > 0 && (!d_corr || !d_inliers)) return set_err(SD_ERR_INVALID, "compute_sim3_refine: correspondences but no tables");
    for (int j = 0; j < n_jobs; j++) {
        if (!slot_ok(b, kf1_index[j]) || !slot_ok(b, kf2_index[j])) return set_err(SD_ERR_STATE, "compute_sim3_refine: slot holds no results");
        if (!b->gridValid[kf1_index[j]] || !b->gridValid[kf2_index[j]])
            return set_err(SD_ERR_STATE, "compute_sim3_refine: sd_batch_assign_grid has not run on both slots");
    }
    const int cap = b->plan.kpCap;
    if (cap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    const hipStream_t prev = b->lastStream;
    hipStream_t s = stream_ ? (hipStream_t)stream_ : prev;
    b->lastStream = s;
    int rc = ensure_sim3(b, n_jobs, s, prev);
    if (rc != SD_OK) return rc;
    rc = ensure_refine(b, n_jobs, s);
    if (rc != SD_OK) return rc;
    HIPCHK(hipMemsetAsync(b->d_s3Err, 0, 4, s));
    b->rfHost.resize(n_jobs);
    for (int j = 0; j < n_jobs; j++) {
        SdRefineJob& J = b->rfHost[j];
        memcpy(J.T1, Tcw1_host + (size_t)j * 16, 64); memcpy(J.T2, Tcw2_host + (size_t)j * 16, 64);
        J.slot1 = kf1_index[j]; J.slot2 = kf2_index[j]; J.c0 = corr_offset[j]; J.nc = corr_offset[j + 1] - corr_offset[j];
    }
    HIPCHK(hipMemcpyAsync(b->d_rfJobs, b->rfHost.data(), (size_t)n_jobs * sizeof(SdRefineJob), hipMemcpyHostToDevice, s));
    SdRefineArgs A;
    A.jobs = b->d_rfJobs; A.ransac = d_ransac; A.rcorr = d_corr; A.inlier = d_inliers; A.bow12 = d_bow12;
    A.kfPoint[0] = d_kf1_point; A.kfPoint[1] = d_kf2_point; A.mps = (const SdMapPoint*)d_points; A.nPoints = n_points;
    A.kp = KPUN(b); A.count = b->d_count; A.pairs = b->d_s3Pairs; A.merged12 = b->d_rfMerged; A.add12 = b->d_s3Match12;
    A.ocorr = b->d_rfCorr; A.oprob = b->d_rfProb; A.ores = b->d_rfOpt; A.ostate = b->d_rfState; A.final12 = b->d_rfFinal; A.out = b->d_rfOut;
    for (int l = 0; l < SD_MAX_LEVELS; l++) A.invSigma2[l] = l < b->ex->prm.nlevels ? b->ex->prm.invSigma2[l] : 0.f;
    A.fx = cam->fx; A.fy = cam->fy; A.cx = cam->cx; A.cy = cam->cy; A.th2 = th2; A.fixScale = fix_scale ? 1 : 0; A.cap = cap;
    hipLaunchKernelGGL(k_refine_begin, dim3(n_jobs), dim3(256), 0, s, A);
    LAUNCH_CHECK("k_refine_begin");
    rc = sim3_search_launch(b, n_jobs, cam, th, d_points, d_point_desc, n_points, d_kf1_point, d_kf2_point, b->d_rfMerged, s);
    if (rc != SD_OK) return rc;
    hipLaunchKernelGGL(k_refine_build, dim3(n_jobs), dim3(256), 0, s, A);
    LAUNCH_CHECK("k_refine_build");
    SdSim3OptArgs O;
    O.prob = b->d_rfProb; O.corr = b->d_rfCorr; O.result = b->d_rfOpt; O.state = b->d_rfState;
    hipLaunchKernelGGL(k_sim3_optimize, dim3(n_jobs), dim3(64), 0, s, O);
    LAUNCH_CHECK("k_sim3_optimize");
    hipLaunchKernelGGL(k_refine_finish, dim3(n_jobs), dim3(256), 0, s, A);
    LAUNCH_CHECK("k_refine_finish");
    b->rfJobs = n_jobs; b->s3Pairs = n_jobs;
    return SD_OK;
}

static int refine_ready(sd_batch* b, int job)
{
    if (job < 0 || job >= b->rfJobs) return set_err(SD_ERR_INVALID, "download_sim3_refine: no such job in the last sd_batch_compute_sim3_refine");
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int err = 0;
    HIPCHK(hipMemcpy(&err, b->d_s3Err, 4, hipMemcpyDeviceToHost));
    if (err) return set_err(SD_ERR_INVALID, "compute_sim3_refine: a feature names a point outside [-1, n_points)");
    return SD_OK;
}

int sd_batch_download_sim3_refine(sd_batch* b, int job, sd_sim3_refine_result* result, int32_t* final12, int cap)
{
    if (!b) return set_err(SD_ERR_INVALID, "bad download_sim3_refine arguments");
    int rc = refine_ready(b, job);
    if (rc != SD_OK) return rc;
    if (final12 && cap < b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "sim3 refine buffers need kp_capacity entries");
    if (result) HIPCHK(hipMemcpy(result, b->d_rfOut + job, sizeof(sd_sim3_refine_result), hipMemcpyDeviceToHost));
    if (final12) HIPCHK(hipMemcpy(final12, b->d_rfFinal + (size_t)job * b->plan.kpCap, (size_t)b->plan.kpCap * 4, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_batch_download_sim3_refine_stages(sd_batch* b, int job, int32_t* merged12, sd_sim3_opt_corr* corr, uint8_t* state, int cap, int* n_built)
{
    if (!b || !n_built) return set_err(SD_ERR_INVALID, "bad download_sim3_refine_stages arguments");
    int rc = refine_ready(b, job);
    if (rc != SD_OK) return rc;
    if (cap < b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "sim3 refine buffers need kp_capacity entries");
    const size_t row = (size_t)job * b->plan.kpCap, n = (size_t)b->plan.kpCap;
    SdSim3OptProb Q;
    HIPCHK(hipMemcpy(&Q, b->d_rfProb + job, sizeof(Q), hipMemcpyDeviceToHost));
    *n_built = Q.n;
    if (merged12) HIPCHK(hipMemcpy(merged12, b->d_rfMerged + row, n * 4, hipMemcpyDeviceToHost));
    if (corr && Q.n > 0) HIPCHK(hipMemcpy(corr, b->d_rfCorr + row, (size_t)Q.n * sizeof(sd_sim3_opt_corr), hipMemcpyDeviceToHost));
    if (state && Q.n > 0) HIPCHK(hipMemcpy(state, b->d_rfState + row, (size_t)Q.n, hipMemcpyDeviceToHost));
    return SD_OK;
}
