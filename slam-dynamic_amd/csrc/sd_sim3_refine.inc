// LoopClosing::ComputeSim3's refine chain (include/sd_frontend.h, kernels in k_sim3_refine.h, DESIGN.md Q45).  Included by sd_api.hip
// inside its extern "C" block.  Six launches and four memsets per call, whatever the number of jobs; no host synchronisation except
// when the library-owned tables grow.
static_assert(sizeof(sd_sim3_refine_result) == 320 && sizeof(SdRefineJob) == 144, "sim3 refine records");

int sd_batch_compute_sim3_refine(sd_batch* b, int n_jobs, const int32_t* kf1_index, const int32_t* kf2_index, const float* Tcw1_host,
                                 const float* Tcw2_host, const sd_sim3_result* d_ransac, const int32_t* corr_offset, const sd_sim3_corr* d_corr,
                                 const uint8_t* d_inliers, const int32_t* d_bow12, const sd_camera* cam, float th, float th2, int fix_scale,
                                 const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points, const int32_t* d_kf1_point,
                                 const int32_t* d_kf2_point, void* stream_)
{
    if (!b || n_jobs < 0 || n_jobs > 32767 || n_points < 0 || !cam_ok(cam) || !(th > 0) || !(th2 > 0) || !std::isfinite(th2) ||
        (n_jobs > 0 && (!kf1_index || !kf2_index || !Tcw1_host || !Tcw2_host || !d_ransac || !corr_offset || !d_bow12 || !d_kf1_point || !d_kf2_point)))
        return set_err(SD_ERR_INVALID, "bad compute_sim3_refine arguments");
    b->sim3Refine.jobs = 0; b->sim3.pairs = 0;
    if (n_jobs == 0) return SD_OK;
    if (n_points > 0 && (!d_points || !d_point_desc)) return set_err(SD_ERR_INVALID, "compute_sim3_refine: n_points but no point table");
    int rc = check_offsets("compute_sim3_refine", corr_offset, n_jobs, nullptr);
    if (rc == SD_OK) rc = check_slots(b, "compute_sim3_refine", kf1_index, kf2_index, n_jobs, SD_SLOT_RANGE);
    if (rc != SD_OK) return rc;
    if (corr_offset[n_jobs] > 0 && (!d_corr || !d_inliers)) return set_err(SD_ERR_INVALID, "compute_sim3_refine: correspondences but no tables");
    rc = check_slots(b, "compute_sim3_refine", kf1_index, kf2_index, n_jobs, SD_SLOT_RESULTS | SD_SLOT_GRID);
    if (rc != SD_OK) return rc;
    const int cap = b->plan.kpCap;
    if (cap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    hipStream_t s = pick_stream(b, stream_);
    rc = b->sim3.grow(b, s, n_jobs);
    if (rc == SD_OK) rc = b->sim3Refine.grow(b, s, n_jobs);
    if (rc != SD_OK) return rc;
    HIPCHK(hipMemsetAsync(b->sim3.d_err, 0, 4, s));
    b->sim3Refine.host.resize(n_jobs);
    for (int j = 0; j < n_jobs; j++) {
        SdRefineJob& J = b->sim3Refine.host[j];
        memcpy(J.T1, Tcw1_host + (size_t)j * 16, 64); memcpy(J.T2, Tcw2_host + (size_t)j * 16, 64);
        J.slot1 = kf1_index[j]; J.slot2 = kf2_index[j]; J.c0 = corr_offset[j]; J.nc = corr_offset[j + 1] - corr_offset[j];
    }
    HIPCHK(hipMemcpyAsync(b->sim3Refine.d_jobs, b->sim3Refine.host.data(), (size_t)n_jobs * sizeof(SdRefineJob), hipMemcpyHostToDevice, s));
    SdRefineArgs A;
    A.jobs = b->sim3Refine.d_jobs; A.ransac = d_ransac; A.rcorr = d_corr; A.inlier = d_inliers; A.bow12 = d_bow12;
    A.kfPoint[0] = d_kf1_point; A.kfPoint[1] = d_kf2_point; A.mps = (const SdMapPoint*)d_points; A.nPoints = n_points;
    A.kp = KPUN(b); A.count = b->d_count; A.pairs = b->sim3.d_pairs; A.merged12 = b->sim3Refine.d_merged; A.add12 = b->sim3.d_match12;
    A.ocorr = b->sim3Refine.d_corr; A.oprob = b->sim3Refine.d_prob; A.ores = b->sim3Refine.d_opt; A.ostate = b->sim3Refine.d_state; A.final12 = b->sim3Refine.d_final; A.out = b->sim3Refine.d_out;
    for (int l = 0; l < SD_MAX_LEVELS; l++) A.invSigma2[l] = l < b->ex->prm.nlevels ? b->ex->prm.invSigma2[l] : 0.f;
    A.fx = cam->fx; A.fy = cam->fy; A.cx = cam->cx; A.cy = cam->cy; A.th2 = th2; A.fixScale = fix_scale ? 1 : 0; A.cap = cap;
    hipLaunchKernelGGL(k_refine_begin, dim3(n_jobs), dim3(256), 0, s, A);
    LAUNCH_CHECK("k_refine_begin");
    rc = sim3_search_launch(b, n_jobs, cam, th, d_points, d_point_desc, n_points, d_kf1_point, d_kf2_point, b->sim3Refine.d_merged, s);
    if (rc != SD_OK) return rc;
    hipLaunchKernelGGL(k_refine_build, dim3(n_jobs), dim3(256), 0, s, A);
    LAUNCH_CHECK("k_refine_build");
    SdSim3OptArgs O;
    O.prob = b->sim3Refine.d_prob; O.corr = b->sim3Refine.d_corr; O.result = b->sim3Refine.d_opt; O.state = b->sim3Refine.d_state;
    hipLaunchKernelGGL(k_sim3_optimize, dim3(n_jobs), dim3(64), 0, s, O);
    LAUNCH_CHECK("k_sim3_optimize");
    hipLaunchKernelGGL(k_refine_finish, dim3(n_jobs), dim3(256), 0, s, A);
    LAUNCH_CHECK("k_refine_finish");
    b->sim3Refine.jobs = n_jobs; b->sim3.pairs = n_jobs;
    return SD_OK;
}

static int refine_ready(sd_batch* b, int job)
{
    if (job < 0 || job >= b->sim3Refine.jobs) return set_err(SD_ERR_INVALID, "download_sim3_refine: no such job in the last sd_batch_compute_sim3_refine");
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int err = 0;
    HIPCHK(hipMemcpy(&err, b->sim3.d_err, 4, hipMemcpyDeviceToHost));
    if (err) return set_err(SD_ERR_INVALID, "compute_sim3_refine: a feature names a point outside [-1, n_points)");
    return SD_OK;
}

int sd_batch_download_sim3_refine(sd_batch* b, int job, sd_sim3_refine_result* result, int32_t* final12, int cap)
{
    if (!b) return set_err(SD_ERR_INVALID, "bad download_sim3_refine arguments");
    int rc = refine_ready(b, job);
    if (rc != SD_OK) return rc;
    if (final12 && cap < b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "sim3 refine buffers need kp_capacity entries");
    if (result) HIPCHK(hipMemcpy(result, b->sim3Refine.d_out + job, sizeof(sd_sim3_refine_result), hipMemcpyDeviceToHost));
    if (final12) HIPCHK(hipMemcpy(final12, b->sim3Refine.d_final + (size_t)job * b->plan.kpCap, (size_t)b->plan.kpCap * 4, hipMemcpyDeviceToHost));
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
    HIPCHK(hipMemcpy(&Q, b->sim3Refine.d_prob + job, sizeof(Q), hipMemcpyDeviceToHost));
    *n_built = Q.n;
    if (merged12) HIPCHK(hipMemcpy(merged12, b->sim3Refine.d_merged + row, n * 4, hipMemcpyDeviceToHost));
    if (corr && Q.n > 0) HIPCHK(hipMemcpy(corr, b->sim3Refine.d_corr + row, (size_t)Q.n * sizeof(sd_sim3_opt_corr), hipMemcpyDeviceToHost));
    if (state && Q.n > 0) HIPCHK(hipMemcpy(state, b->sim3Refine.d_state + row, (size_t)Q.n, hipMemcpyDeviceToHost));
    return SD_OK;
}
