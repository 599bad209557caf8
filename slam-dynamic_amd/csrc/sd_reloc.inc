// Tracking::Relocalization's matcher (include/sd_frontend.h, kernels in k_reloc.h, DESIGN.md Q44).  Included by sd_api.hip inside its
// extern "C" block.  Reference: src/ORBmatcher.cc:1629-1756.

int sd_batch_search_by_projection_reloc(sd_batch* b, int n_jobs, const int32_t* frame_index, const int32_t* kf_index, const float* Tcw_host,
                                        const float* th, const int32_t* orb_dist, const int32_t* d_kf_point, const int32_t* d_frame_point,
                                        const uint8_t* d_found, const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points,
                                        const sd_camera* cam, int32_t** d_frame_point_out, int32_t** d_from_kf, int32_t** d_nmatches,
                                        void* stream_)
{
    if (d_frame_point_out) *d_frame_point_out = nullptr;
    if (d_from_kf) *d_from_kf = nullptr;
    if (d_nmatches) *d_nmatches = nullptr;
    if (!b || n_jobs < 0 || n_jobs > SD_RELOC_MAX_JOBS || n_points < 0 || !cam_ok(cam) ||
        (n_jobs > 0 && (!frame_index || !kf_index || !Tcw_host || !th || !orb_dist || !d_kf_point || !d_frame_point)))
        return set_err(SD_ERR_INVALID, "bad search_by_projection_reloc arguments");
    b->reloc.jobs = 0;
    if (n_jobs == 0) return SD_OK;
    int rc = check_slots(b, "search_by_projection_reloc", frame_index, kf_index, n_jobs, SD_SLOT_RANGE);
    if (rc != SD_OK) return rc;
    for (int j = 0; j < n_jobs; j++) {
        if (!(th[j] > 0)) return set_err(SD_ERR_INVALID, "search_by_projection_reloc: th must be positive");
        if (orb_dist[j] < 0 || orb_dist[j] > 255) return set_err(SD_ERR_INVALID, "search_by_projection_reloc: ORBdist outside [0, 255]");
    }
    rc = check_slots(b, "search_by_projection_reloc", frame_index, kf_index, n_jobs, SD_SLOT_RESULTS | SD_SLOT_GRID);
    if (rc != SD_OK) return rc;
    // a job whose keyframe carries points needs the table; without one every d_kf_point value is outside it and reads as -1
    if (n_points > 0 && (!d_points || !d_point_desc)) return set_err(SD_ERR_INVALID, "search_by_projection_reloc: n_points but no map points given");
    const int cap = b->plan.kpCap;
    if (cap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    hipStream_t s = pick_stream(b, stream_);
    rc = b->reloc.grow(b, s, n_jobs);
    if (rc != SD_OK) return rc;
    b->reloc.slots.resize(n_jobs);
    for (int j = 0; j < n_jobs; j++) b->reloc.slots[j] = make_int2(frame_index[j], kf_index[j]);
    HIPCHK(hipMemsetAsync(b->reloc.d_err, 0, 4, s));              // the flag belongs to this call: every job's download reports it
    HIPCHK(hipMemcpyAsync(b->reloc.d_slots, b->reloc.slots.data(), (size_t)n_jobs * sizeof(int2), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->reloc.d_T, Tcw_host, (size_t)n_jobs * 64, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->reloc.d_th, th, (size_t)n_jobs * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->reloc.d_orb, orb_dist, (size_t)n_jobs * 4, hipMemcpyHostToDevice, s));
    {
        ProfScope ps(b, s, K_RELOC_S);
        hipLaunchKernelGGL(k_reloc_search, dim3((cap + 3) / 4, n_jobs), dim3(256), 0, s, KPUN(b), b->d_desc, b->d_uright, b->d_sortedIdx, b->d_cellStart,
                           b->d_count, (const SdMapPoint*)d_points, d_point_desc, n_points, b->reloc.d_slots.get(), b->reloc.d_T.get(), b->reloc.d_th.get(),
                           d_kf_point, d_frame_point, d_found, (const uint8_t*)nullptr, b->reloc.d_list.get(), b->reloc.d_listN.get(), b->reloc.d_exit.get(),
                           b->reloc.d_err.get(), level_tables(b), to_cam(cam), cap, SdRelocPlan{nullptr, nullptr, n_jobs}, (int)SD_RELOC_STEP_ALWAYS);
        LAUNCH_CHECK("k_reloc_search");
    }
    {
        ProfScope ps(b, s, K_RELOC_A);
        hipLaunchKernelGGL(k_reloc_assign, dim3(n_jobs), dim3(64), (size_t)((cap + 31) / 32) * 4 + 16, s, KPUN(b), b->d_count, b->reloc.d_slots.get(),
                           b->reloc.d_orb.get(), b->reloc.d_list.get(), b->reloc.d_listN.get(), d_kf_point, d_frame_point, n_points, cap,
                           b->reloc.d_exit.get(), b->reloc.d_frame.get(), b->reloc.d_from.get(), b->reloc.d_best.get(), b->reloc.d_nm.get(), b->d_err.get(),
                           SdRelocPlan{nullptr, nullptr, n_jobs}, (int)SD_RELOC_STEP_ALWAYS);
        LAUNCH_CHECK("k_reloc_assign");
    }
    b->reloc.jobs = n_jobs;
    if (d_frame_point_out) *d_frame_point_out = b->reloc.d_frame;
    if (d_from_kf) *d_from_kf = b->reloc.d_from;
    if (d_nmatches) *d_nmatches = b->reloc.d_nm;
    return SD_OK;
}

int sd_batch_download_reloc_matches(sd_batch* b, int job, int32_t* frame_point, int32_t* from_kf, int32_t* exits, int32_t* best, int cap,
                                    int* nmatches)
{
    if (!b || !nmatches) return set_err(SD_ERR_INVALID, "bad download_reloc_matches arguments");
    if (job < 0 || job >= b->reloc.jobs) return set_err(SD_ERR_INVALID, "download_reloc_matches: no such job in the last sd_batch_search_by_projection_reloc");
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int err = 0;
    HIPCHK(hipMemcpy(&err, b->reloc.d_err, 4, hipMemcpyDeviceToHost));
    if (err) return set_err(SD_ERR_INVALID, "search_by_projection_reloc: a d_kf_point or d_frame_point entry names a point outside its table");
    HIPCHK(hipMemcpy(nmatches, b->reloc.d_nm + job, 4, hipMemcpyDeviceToHost));
    const size_t n = (size_t)b->plan.kpCap, r0 = (size_t)job * n;
    if ((frame_point || from_kf || exits || best) && cap < b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "the reloc rows need kp_capacity entries");
    if (frame_point) HIPCHK(hipMemcpy(frame_point, b->reloc.d_frame + r0, n * 4, hipMemcpyDeviceToHost));
    if (from_kf) HIPCHK(hipMemcpy(from_kf, b->reloc.d_from + r0, n * 4, hipMemcpyDeviceToHost));
    if (exits) HIPCHK(hipMemcpy(exits, b->reloc.d_exit + r0, n * 4, hipMemcpyDeviceToHost));
    if (best) HIPCHK(hipMemcpy(best, b->reloc.d_best + r0, n * sizeof(int2), hipMemcpyDeviceToHost));
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// The cascade after PnP of Tracking::Relocalization (src/Tracking.cc:2292-2358), every step predicated per job on the device
// ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(sd_reloc_result) == 284, "sd_reloc_result is 7 ints and 4 poses");

// The body of the cascade on stream s for checked arguments.  The poses come from the host (Tcw_host) or, when that is null, from device
// memory (d_Tcw, [n_jobs][16], read on s): sd_batch_relocalize_pnp's hand-over.
static int reloc_refine_run(sd_batch* b, int n_jobs, const int32_t* frame_index, const int32_t* kf_index, const float* Tcw_host, const float* d_Tcw,
                            const int32_t* d_kf_point, const int32_t* d_frame_point, const sd_map_point* d_points, const uint8_t* d_point_desc,
                            int n_points, const sd_camera* cam, sd_reloc_result** d_results, hipStream_t s);

int sd_batch_relocalize_refine(sd_batch* b, int n_jobs, const int32_t* frame_index, const int32_t* kf_index, const float* Tcw_host,
                               const int32_t* d_kf_point, const int32_t* d_frame_point, const sd_map_point* d_points, const uint8_t* d_point_desc,
                               int n_points, const sd_camera* cam, sd_reloc_result** d_results, void* stream_)
{
    if (d_results) *d_results = nullptr;
    if (!b || n_jobs < 0 || n_jobs > SD_RELOC_MAX_JOBS || n_points < 0 || !cam_ok(cam) ||
        (n_jobs > 0 && (!frame_index || !kf_index || !Tcw_host || !d_kf_point || !d_frame_point)))
        return set_err(SD_ERR_INVALID, "bad relocalize_refine arguments");
    b->relocRefine.jobs = 0;
    if (n_jobs == 0) return SD_OK;
    int rc = check_slots(b, "relocalize_refine", frame_index, kf_index, n_jobs, SD_SLOT_RANGE);
    if (rc == SD_OK) rc = check_slots(b, "relocalize_refine", frame_index, kf_index, n_jobs, SD_SLOT_RESULTS | SD_SLOT_GRID);
    if (rc != SD_OK) return rc;
    if (n_points > 0 && (!d_points || !d_point_desc)) return set_err(SD_ERR_INVALID, "relocalize_refine: n_points but no map points given");
    const int cap = b->plan.kpCap;
    if (cap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    return reloc_refine_run(b, n_jobs, frame_index, kf_index, Tcw_host, nullptr, d_kf_point, d_frame_point, d_points, d_point_desc, n_points, cam, d_results,
                            pick_stream(b, stream_));
}

static int reloc_refine_run(sd_batch* b, int n_jobs, const int32_t* frame_index, const int32_t* kf_index, const float* Tcw_host, const float* d_Tcw,
                            const int32_t* d_kf_point, const int32_t* d_frame_point, const sd_map_point* d_points, const uint8_t* d_point_desc,
                            int n_points, const sd_camera* cam, sd_reloc_result** d_results, hipStream_t s)
{
    int rc = SD_OK;
    const int cap = b->plan.kpCap;
    const size_t markBytes = std::max<size_t>((size_t)n_jobs * (size_t)n_points, 16);
    rc = b->reloc.grow(b, s, n_jobs);                             // the slot table and the kept keys are the matcher's
    if (rc == SD_OK) rc = b->relocRefine.grow(b, s, n_jobs, markBytes);
    if (rc != SD_OK) return rc;
    b->reloc.jobs = 0;                                             // the matcher's tables are reused: its last results are gone
    const size_t J = (size_t)n_jobs, rows = J * cap;
    b->reloc.slots.resize(n_jobs); b->relocRefine.th.resize(2 * J); b->relocRefine.orb.resize(2 * J); b->relocRefine.cam.assign(J, *cam);
    for (int j = 0; j < n_jobs; j++) {
        b->reloc.slots[j] = make_int2(frame_index[j], kf_index[j]);
        b->relocRefine.th[j] = 10.f; b->relocRefine.orb[j] = 100; b->relocRefine.th[J + j] = 3.f; b->relocRefine.orb[J + j] = 64;       // Tracking.cc:2323, :2337
    }
    int* P[5]; for (int k = 0; k < 5; k++) P[k] = b->relocRefine.d_P + k * rows;
    float* T[4]; for (int k = 0; k < 4; k++) T[k] = b->relocRefine.d_T + k * J * 16;
    const SdRelocPlan plan{b->relocRefine.d_good.get(), b->relocRefine.d_nm.get(), n_jobs};
    const SdMapPoint* mps = (const SdMapPoint*)d_points;
    HIPCHK(hipMemsetAsync(b->reloc.d_err, 0, 4, s));
    HIPCHK(hipMemcpyAsync(b->reloc.d_slots, b->reloc.slots.data(), J * sizeof(int2), hipMemcpyHostToDevice, s));
    if (Tcw_host) HIPCHK(hipMemcpyAsync(T[0], Tcw_host, J * 64, hipMemcpyHostToDevice, s));
    else HIPCHK(hipMemcpyAsync(T[0], d_Tcw, J * 64, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(b->relocRefine.d_th, b->relocRefine.th.data(), 2 * J * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->relocRefine.d_orb, b->relocRefine.orb.data(), 2 * J * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->relocRefine.d_cam, b->relocRefine.cam.data(), J * sizeof(sd_camera), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(b->relocRefine.d_mark, 0, markBytes, s));
    {
        ProfScope ps(b, s, K_RELOC_X);
        hipLaunchKernelGGL(k_reloc_begin, dim3(n_jobs), dim3(256), 0, s, b->d_count, b->reloc.d_slots.get(), d_kf_point, d_frame_point, n_points, cap, P[0],
                           b->relocRefine.d_outlier.get(), b->relocRefine.d_mark.get(), b->reloc.d_err.get());
        LAUNCH_CHECK("k_reloc_begin");
    }
    SdRelocEdgeArgs E;
    E.kp = KPUN(b); E.uRight = b->d_uright; E.count = b->d_count; E.slots = b->reloc.d_slots; E.mps = mps; E.cap = cap;
    const SdLevelTables LT = level_tables(b);
    for (int l = 0; l < SD_MAX_LEVELS; l++) E.invSigma2[l] = LT.invSigma2[l];
    // optimisation k: edges from Pin, pose T[k] -> T[k + 1]; then mvbOutlier and (Pout) the assignment that follows
    auto optimise = [&](int k, int step, const int* Pin, int* Pout, int minGood) -> int {
        E.P = Pin; E.Tprev = T[k]; E.Tcur = T[k + 1]; E.edges = b->relocRefine.d_edges + k * rows; E.first = b->relocRefine.d_first + k * J; E.last = b->relocRefine.d_last + k * J;
        {
            ProfScope ps(b, s, K_RELOC_E);
            hipLaunchKernelGGL(k_reloc_edges, dim3(n_jobs), dim3(256), 0, s, E, plan, step);
            LAUNCH_CHECK("k_reloc_edges");
        }
        SdPoseArgs A;
        A.edges = E.edges; A.first = E.first; A.last = E.last; A.cam = b->relocRefine.d_cam; A.Tcw = T[k + 1]; A.outlier = b->relocRefine.d_edgeOut + k * rows;
        A.nGood = b->relocRefine.d_good + k * J; A.map = nullptr;
        {
            ProfScope ps(b, s, K_RELOC_O);
            hipLaunchKernelGGL(k_pose_optimize, dim3(n_jobs), dim3(SD_POSE_THREADS), 0, s, A);
            LAUNCH_CHECK("k_pose_optimize");
        }
        {
            ProfScope ps(b, s, K_RELOC_X);
            hipLaunchKernelGGL(k_reloc_after, dim3(n_jobs), dim3(256), 0, s, (const sd_pose_edge*)E.edges, (const int*)E.first, (const int*)E.last,
                               (const uint8_t*)A.outlier, (const int*)A.nGood, Pin, Pout, b->relocRefine.d_outlier.get(), cap, minGood, plan, step);
            LAUNCH_CHECK("k_reloc_after");
        }
        return SD_OK;
    };
    // search w: SearchByProjection(CurrentFrame, pKF, sFound, th, ORBdist) from Pin under pose Tk -> Pout
    auto search = [&](int w, int step, const float* Tk, const int* Pin, int* Pout) -> int {
        {
            ProfScope ps(b, s, K_RELOC_S);
            hipLaunchKernelGGL(k_reloc_search, dim3((cap + 3) / 4, n_jobs), dim3(256), 0, s, KPUN(b), b->d_desc, b->d_uright, b->d_sortedIdx, b->d_cellStart,
                               b->d_count, mps, d_point_desc, n_points, b->reloc.d_slots.get(), Tk, (const float*)(b->relocRefine.d_th + w * J), d_kf_point, Pin,
                               (const uint8_t*)nullptr, (const uint8_t*)b->relocRefine.d_mark.get(), b->reloc.d_list.get(), b->reloc.d_listN.get(),
                               b->relocRefine.d_exit + w * rows, b->reloc.d_err.get(), LT, to_cam(cam), cap, plan, step);
            LAUNCH_CHECK("k_reloc_search");
        }
        {
            ProfScope ps(b, s, K_RELOC_A);
            hipLaunchKernelGGL(k_reloc_assign, dim3(n_jobs), dim3(64), (size_t)((cap + 31) / 32) * 4 + 16, s, KPUN(b), b->d_count, b->reloc.d_slots.get(),
                               (const int*)(b->relocRefine.d_orb + w * J), b->reloc.d_list.get(), b->reloc.d_listN.get(), d_kf_point, Pin, n_points, cap,
                               b->relocRefine.d_exit + w * rows, Pout, b->relocRefine.d_from + w * rows, b->relocRefine.d_best + w * rows, b->relocRefine.d_nm + w * J, b->d_err.get(), plan, step);
            LAUNCH_CHECK("k_reloc_assign");
        }
        return SD_OK;
    };
    if ((rc = optimise(0, SD_RELOC_STEP_ALWAYS, P[0], P[1], 10)) != SD_OK) return rc;                 // :2311-2318
    if ((rc = search(0, SD_RELOC_STEP_SEARCH1, T[1], P[1], P[2])) != SD_OK) return rc;                // :2323
    if ((rc = optimise(1, SD_RELOC_STEP_OPT2, P[2], nullptr, 0)) != SD_OK) return rc;                 // :2327, no discard
    HIPCHK(hipMemsetAsync(b->relocRefine.d_mark, 0, markBytes, s));
    {
        ProfScope ps(b, s, K_RELOC_X);
        hipLaunchKernelGGL(k_reloc_mark, dim3(n_jobs), dim3(256), 0, s, (const int*)P[2], n_points, cap, b->relocRefine.d_mark.get(), plan, (int)SD_RELOC_STEP_SEARCH2);   // :2333-2336
        LAUNCH_CHECK("k_reloc_mark");
    }
    if ((rc = search(1, SD_RELOC_STEP_SEARCH2, T[2], P[2], P[3])) != SD_OK) return rc;                // :2337
    if ((rc = optimise(2, SD_RELOC_STEP_OPT3, P[3], P[4], INT_MIN)) != SD_OK) return rc;              // :2342-2346
    {
        ProfScope ps(b, s, K_RELOC_X);
        hipLaunchKernelGGL(k_reloc_finish, dim3((n_jobs + 255) / 256), dim3(256), 0, s, (const float*)b->relocRefine.d_T.get(), b->relocRefine.d_res.get(), plan);
        LAUNCH_CHECK("k_reloc_finish");
    }
    b->relocRefine.jobs = n_jobs;
    if (d_results) *d_results = b->relocRefine.d_res;
    return SD_OK;
}

static int refine_ready(sd_batch* b, int job, const char* who)
{
    if (!b) return set_err(SD_ERR_INVALID, std::string(who) + ": null batch");
    if (job < 0 || job >= b->relocRefine.jobs) return set_err(SD_ERR_INVALID, std::string(who) + ": no such job in the last sd_batch_relocalize_refine");
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int err = 0;
    HIPCHK(hipMemcpy(&err, b->reloc.d_err, 4, hipMemcpyDeviceToHost));
    if (err) return set_err(SD_ERR_INVALID, "relocalize_refine: a d_kf_point or d_frame_point entry names a point outside its table");
    return SD_OK;
}

int sd_batch_download_reloc(sd_batch* b, int job, sd_reloc_result* result, int32_t* frame_point, uint8_t* outlier, int cap)
{
    int rc = refine_ready(b, job, "download_reloc");
    if (rc != SD_OK) return rc;
    const size_t n = (size_t)b->plan.kpCap, rows = (size_t)b->relocRefine.jobs * n;
    if ((frame_point || outlier) && cap < b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "the reloc rows need kp_capacity entries");
    if (result) HIPCHK(hipMemcpy(result, b->relocRefine.d_res + job, sizeof(sd_reloc_result), hipMemcpyDeviceToHost));
    if (frame_point) HIPCHK(hipMemcpy(frame_point, b->relocRefine.d_P + 4 * rows + (size_t)job * n, n * 4, hipMemcpyDeviceToHost));
    if (outlier) HIPCHK(hipMemcpy(outlier, b->relocRefine.d_outlier + (size_t)job * n, n, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_batch_download_reloc_optimisation(sd_batch* b, int job, int stage, sd_pose_edge* edges, uint8_t* edge_outlier, int cap_edges, int* n_edges,
                                         float* Tcw_in)
{
    if (stage < 0 || stage > 2 || !n_edges) return set_err(SD_ERR_INVALID, "bad download_reloc_optimisation arguments");
    int rc = refine_ready(b, job, "download_reloc_optimisation");
    if (rc != SD_OK) return rc;
    const size_t J = (size_t)b->relocRefine.jobs, rows = J * b->plan.kpCap;
    int fl[2];
    HIPCHK(hipMemcpy(&fl[0], b->relocRefine.d_first + stage * J + job, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&fl[1], b->relocRefine.d_last + stage * J + job, 4, hipMemcpyDeviceToHost));
    const int n = fl[1] - fl[0];
    *n_edges = n;
    if ((edges || edge_outlier) && n > cap_edges) return set_err(SD_ERR_CAPACITY, "reloc edge buffers too small");
    if (edges && n > 0) HIPCHK(hipMemcpy(edges, b->relocRefine.d_edges + stage * rows + fl[0], (size_t)n * sizeof(sd_pose_edge), hipMemcpyDeviceToHost));
    if (edge_outlier && n > 0) HIPCHK(hipMemcpy(edge_outlier, b->relocRefine.d_edgeOut + stage * rows + fl[0], (size_t)n, hipMemcpyDeviceToHost));
    if (Tcw_in) HIPCHK(hipMemcpy(Tcw_in, b->relocRefine.d_T + (stage * J + job) * 16, 64, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_batch_download_reloc_search(sd_batch* b, int job, int which, int32_t* frame_point_in, int32_t* frame_point_out, int32_t* from_kf,
                                   int32_t* exits, int32_t* best, int cap, int* nmatches)
{
    if (which < 0 || which > 1) return set_err(SD_ERR_INVALID, "bad download_reloc_search arguments");
    int rc = refine_ready(b, job, "download_reloc_search");
    if (rc != SD_OK) return rc;
    const size_t n = (size_t)b->plan.kpCap, J = (size_t)b->relocRefine.jobs, rows = J * n, r0 = (size_t)job * n;
    if ((frame_point_in || frame_point_out || from_kf || exits || best) && cap < b->plan.kpCap)
        return set_err(SD_ERR_CAPACITY, "the reloc rows need kp_capacity entries");
    if (nmatches) HIPCHK(hipMemcpy(nmatches, b->relocRefine.d_nm + which * J + job, 4, hipMemcpyDeviceToHost));
    if (frame_point_in) HIPCHK(hipMemcpy(frame_point_in, b->relocRefine.d_P + (which + 1) * rows + r0, n * 4, hipMemcpyDeviceToHost));
    if (frame_point_out) HIPCHK(hipMemcpy(frame_point_out, b->relocRefine.d_P + (which + 2) * rows + r0, n * 4, hipMemcpyDeviceToHost));
    if (from_kf) HIPCHK(hipMemcpy(from_kf, b->relocRefine.d_from + which * rows + r0, n * 4, hipMemcpyDeviceToHost));
    if (exits) HIPCHK(hipMemcpy(exits, b->relocRefine.d_exit + which * rows + r0, n * 4, hipMemcpyDeviceToHost));
    if (best) HIPCHK(hipMemcpy(best, b->relocRefine.d_best + which * rows + r0, n * sizeof(int2), hipMemcpyDeviceToHost));
    return SD_OK;
}
