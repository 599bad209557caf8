// Tracking::Relocalization's matcher (include/sd_frontend.h, kernels in k_reloc.h, DESIGN.md Q44).  Included by sd_api.hip inside its
// extern "C" block.  Reference: src/ORBmatcher.cc:1629-1756.

// Job tables, kept keys and result rows of sd_batch_search_by_projection_reloc: they grow with the largest call seen (old ones freed
// first), as ensure_loop does
static int ensure_reloc(sd_batch* b, int n_jobs, hipStream_t s)
{
    const size_t cap = b->plan.kpCap;
    if (!b->d_relocErr) { HIPCHK(b->d_relocErr.alloc(4)); HIPCHK(hipMemset(b->d_relocErr, 0, 4)); }
    if (n_jobs <= b->relocJobCap) return SD_OK;
    HIPCHK(hipStreamSynchronize(s));
    const size_t want = (size_t)std::min(std::max(n_jobs, 2 * b->relocJobCap), SD_RELOC_MAX_JOBS), rows = want * cap;
    b->relocJobCap = 0; b->relocJobs = 0;
    b->d_relocSlots.reset(); b->d_relocT.reset(); b->d_relocTh.reset(); b->d_relocOrb.reset(); b->d_relocNm.reset(); b->d_relocList.reset();
    b->d_relocListN.reset(); b->d_relocExit.reset(); b->d_relocBest.reset(); b->d_relocFrame.reset(); b->d_relocFrom.reset();
    HIPCHK(b->d_relocSlots.alloc(want * sizeof(int2))); HIPCHK(b->d_relocT.alloc(want * 64)); HIPCHK(b->d_relocTh.alloc(want * 4));
    HIPCHK(b->d_relocOrb.alloc(want * 4)); HIPCHK(b->d_relocNm.alloc(want * 4)); HIPCHK(b->d_relocList.alloc(rows * SD_PROJ_K * 4));
    HIPCHK(b->d_relocListN.alloc(rows * 4)); HIPCHK(b->d_relocExit.alloc(rows * 4)); HIPCHK(b->d_relocBest.alloc(rows * sizeof(int2)));
    HIPCHK(b->d_relocFrame.alloc(rows * 4)); HIPCHK(b->d_relocFrom.alloc(rows * 4));
    b->relocJobCap = (int)want;
    return SD_OK;
}

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
    b->relocJobs = 0;
    if (n_jobs == 0) return SD_OK;
    for (int j = 0; j < n_jobs; j++) {
        if (frame_index[j] < 0 || frame_index[j] >= b->maxImages || kf_index[j] < 0 || kf_index[j] >= b->maxImages)
            return set_err(SD_ERR_INVALID, "search_by_projection_reloc: slot out of range");
        if (!(th[j] > 0)) return set_err(SD_ERR_INVALID, "search_by_projection_reloc: th must be positive");
        if (orb_dist[j] < 0 || orb_dist[j] > 255) return set_err(SD_ERR_INVALID, "search_by_projection_reloc: ORBdist outside [0, 255]");
    }
    for (int j = 0; j < n_jobs; j++) {
        if (!slot_ok(b, frame_index[j]) || !slot_ok(b, kf_index[j])) return set_err(SD_ERR_STATE, "search_by_projection_reloc: slot holds no results");
        if (!b->gridValid[frame_index[j]] || !b->gridValid[kf_index[j]])
            return set_err(SD_ERR_STATE, "search_by_projection_reloc: sd_batch_assign_grid has not run on this slot");
    }
    // a job whose keyframe carries points needs the table; without one every d_kf_point value is outside it and reads as -1
    if (n_points > 0 && (!d_points || !d_point_desc)) return set_err(SD_ERR_INVALID, "search_by_projection_reloc: n_points but no map points given");
    const int cap = b->plan.kpCap;
    if (cap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    hipStream_t s = stream_ ? (hipStream_t)stream_ : b->lastStream;
    b->lastStream = s;
    int rc = ensure_reloc(b, n_jobs, s);
    if (rc != SD_OK) return rc;
    b->relocSlots.resize(n_jobs);
    for (int j = 0; j < n_jobs; j++) b->relocSlots[j] = make_int2(frame_index[j], kf_index[j]);
    HIPCHK(hipMemsetAsync(b->d_relocErr, 0, 4, s));              // the flag belongs to this call: every job's download reports it
    HIPCHK(hipMemcpyAsync(b->d_relocSlots, b->relocSlots.data(), (size_t)n_jobs * sizeof(int2), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->d_relocT, Tcw_host, (size_t)n_jobs * 64, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->d_relocTh, th, (size_t)n_jobs * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->d_relocOrb, orb_dist, (size_t)n_jobs * 4, hipMemcpyHostToDevice, s));
    {
        ProfScope ps(b, s, K_RELOC_S);
        hipLaunchKernelGGL(k_reloc_search, dim3((cap + 3) / 4, n_jobs), dim3(256), 0, s, KPUN(b), b->d_desc, b->d_uright, b->d_sortedIdx, b->d_cellStart,
                           b->d_count, (const SdMapPoint*)d_points, d_point_desc, n_points, b->d_relocSlots.get(), b->d_relocT.get(), b->d_relocTh.get(),
                           d_kf_point, d_frame_point, d_found, (const uint8_t*)nullptr, b->d_relocList.get(), b->d_relocListN.get(), b->d_relocExit.get(),
                           b->d_relocErr.get(), level_tables(b), to_cam(cam), cap, SdRelocPlan{nullptr, nullptr, n_jobs}, (int)SD_RELOC_STEP_ALWAYS);
        LAUNCH_CHECK("k_reloc_search");
    }
    {
        ProfScope ps(b, s, K_RELOC_A);
        hipLaunchKernelGGL(k_reloc_assign, dim3(n_jobs), dim3(64), (size_t)((cap + 31) / 32) * 4 + 16, s, KPUN(b), b->d_count, b->d_relocSlots.get(),
                           b->d_relocOrb.get(), b->d_relocList.get(), b->d_relocListN.get(), d_kf_point, d_frame_point, n_points, cap,
                           b->d_relocExit.get(), b->d_relocFrame.get(), b->d_relocFrom.get(), b->d_relocBest.get(), b->d_relocNm.get(), b->d_err.get(),
                           SdRelocPlan{nullptr, nullptr, n_jobs}, (int)SD_RELOC_STEP_ALWAYS);
        LAUNCH_CHECK("k_reloc_assign");
    }
    b->relocJobs = n_jobs;
    if (d_frame_point_out) *d_frame_point_out = b->d_relocFrame;
    if (d_from_kf) *d_from_kf = b->d_relocFrom;
    if (d_nmatches) *d_nmatches = b->d_relocNm;
    return SD_OK;
}

int sd_batch_download_reloc_matches(sd_batch* b, int job, int32_t* frame_point, int32_t* from_kf, int32_t* exits, int32_t* best, int cap,
                                    int* nmatches)
{
    if (!b || !nmatches) return set_err(SD_ERR_INVALID, "bad download_reloc_matches arguments");
    if (job < 0 || job >= b->relocJobs) return set_err(SD_ERR_INVALID, "download_reloc_matches: no such job in the last sd_batch_search_by_projection_reloc");
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int err = 0;
    HIPCHK(hipMemcpy(&err, b->d_relocErr, 4, hipMemcpyDeviceToHost));
    if (err) return set_err(SD_ERR_INVALID, "search_by_projection_reloc: a d_kf_point or d_frame_point entry names a point outside its table");
    HIPCHK(hipMemcpy(nmatches, b->d_relocNm + job, 4, hipMemcpyDeviceToHost));
    const size_t n = (size_t)b->plan.kpCap, r0 = (size_t)job * n;
    if ((frame_point || from_kf || exits || best) && cap < b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "the reloc rows need kp_capacity entries");
    if (frame_point) HIPCHK(hipMemcpy(frame_point, b->d_relocFrame + r0, n * 4, hipMemcpyDeviceToHost));
    if (from_kf) HIPCHK(hipMemcpy(from_kf, b->d_relocFrom + r0, n * 4, hipMemcpyDeviceToHost));
    if (exits) HIPCHK(hipMemcpy(exits, b->d_relocExit + r0, n * 4, hipMemcpyDeviceToHost));
    if (best) HIPCHK(hipMemcpy(best, b->d_relocBest + r0, n * sizeof(int2), hipMemcpyDeviceToHost));
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// The cascade after PnP of Tracking::Relocalization (src/Tracking.cc:2292-2358), every step predicated per job on the device
// ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(sd_reloc_result) == 284, "sd_reloc_result is 7 ints and 4 poses");

// Tables of sd_batch_relocalize_refine: they grow with the largest call seen (jobs; jobs x points for the sFound marks)
static int ensure_refine(sd_batch* b, int n_jobs, size_t markBytes, hipStream_t s)
{
    const size_t cap = b->plan.kpCap;
    if (n_jobs > b->rrJobCap || markBytes > b->rrMarkCap) HIPCHK(hipStreamSynchronize(s));
    if (markBytes > b->rrMarkCap) {
        b->rrMarkCap = 0; b->d_rrMark.reset();
        HIPCHK(b->d_rrMark.alloc(markBytes));
        b->rrMarkCap = markBytes;
    }
    if (n_jobs <= b->rrJobCap) return SD_OK;
    const size_t want = (size_t)std::min(std::max(n_jobs, 2 * b->rrJobCap), SD_RELOC_MAX_JOBS), rows = want * cap;
    b->rrJobCap = 0; b->rrJobs = 0;
    b->d_rrP.reset(); b->d_rrFrom.reset(); b->d_rrExit.reset(); b->d_rrBest.reset(); b->d_rrNm.reset(); b->d_rrGood.reset(); b->d_rrFirst.reset();
    b->d_rrLast.reset(); b->d_rrEdges.reset(); b->d_rrEdgeOut.reset(); b->d_rrOutlier.reset(); b->d_rrT.reset(); b->d_rrTh.reset(); b->d_rrOrb.reset();
    b->d_rrCam.reset(); b->d_rrRes.reset();
    HIPCHK(b->d_rrP.alloc(5 * rows * 4)); HIPCHK(b->d_rrFrom.alloc(2 * rows * 4)); HIPCHK(b->d_rrExit.alloc(2 * rows * 4));
    HIPCHK(b->d_rrBest.alloc(2 * rows * sizeof(int2))); HIPCHK(b->d_rrNm.alloc(2 * want * 4)); HIPCHK(b->d_rrGood.alloc(3 * want * 4));
    HIPCHK(b->d_rrFirst.alloc(3 * want * 4)); HIPCHK(b->d_rrLast.alloc(3 * want * 4)); HIPCHK(b->d_rrEdges.alloc(3 * rows * sizeof(sd_pose_edge)));
    HIPCHK(b->d_rrEdgeOut.alloc(3 * rows)); HIPCHK(b->d_rrOutlier.alloc(rows)); HIPCHK(b->d_rrT.alloc(4 * want * 64)); HIPCHK(b->d_rrTh.alloc(2 * want * 4));
    HIPCHK(b->d_rrOrb.alloc(2 * want * 4)); HIPCHK(b->d_rrCam.alloc(want * sizeof(sd_camera))); HIPCHK(b->d_rrRes.alloc(want * sizeof(sd_reloc_result)));
    b->rrJobCap = (int)want;
    return SD_OK;
}

int sd_batch_relocalize_refine(sd_batch* b, int n_jobs, const int32_t* frame_index, const int32_t* kf_index, const float* Tcw_host,
                               const int32_t* d_kf_point, const int32_t* d_frame_point, const sd_map_point* d_points, const uint8_t* d_point_desc,
                               int n_points, const sd_camera* cam, sd_reloc_result** d_results, void* stream_)
{
    if (d_results) *d_results = nullptr;
    if (!b || n_jobs < 0 || n_jobs > SD_RELOC_MAX_JOBS || n_points < 0 || !cam_ok(cam) ||
        (n_jobs > 0 && (!frame_index || !kf_index || !Tcw_host || !d_kf_point || !d_frame_point)))
        return set_err(SD_ERR_INVALID, "bad relocalize_refine arguments");
    b->rrJobs = 0;
    if (n_jobs == 0) return SD_OK;
    for (int j = 0; j < n_jobs; j++)
        if (frame_index[j] < 0 || frame_index[j] >= b->maxImages || kf_index[j] < 0 || kf_index[j] >= b->maxImages)
            return set_err(SD_ERR_INVALID, "relocalize_refine: slot out of range");
    for (int j = 0; j < n_jobs; j++) {
        if (!slot_ok(b, frame_index[j]) || !slot_ok(b, kf_index[j])) return set_err(SD_ERR_STATE, "relocalize_refine: slot holds no results");
        if (!b->gridValid[frame_index[j]] || !b->gridValid[kf_index[j]])
            return set_err(SD_ERR_STATE, "relocalize_refine: sd_batch_assign_grid has not run on this slot");
    }
    if (n_points > 0 && (!d_points || !d_point_desc)) return set_err(SD_ERR_INVALID, "relocalize_refine: n_points but no map points given");
    const int cap = b->plan.kpCap;
    if (cap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    hipStream_t s = stream_ ? (hipStream_t)stream_ : b->lastStream;
    b->lastStream = s;
    const size_t markBytes = std::max<size_t>((size_t)n_jobs * (size_t)n_points, 16);
    int rc = ensure_reloc(b, n_jobs, s);                          // the slot table and the kept keys are the matcher's
    if (rc != SD_OK) return rc;
    rc = ensure_refine(b, n_jobs, markBytes, s);
    if (rc != SD_OK) return rc;
    b->relocJobs = 0;                                             // the matcher's tables are reused: its last results are gone
    const size_t J = (size_t)n_jobs, rows = J * cap;
    b->relocSlots.resize(n_jobs); b->rrTh.resize(2 * J); b->rrOrb.resize(2 * J); b->rrCam.assign(J, *cam);
    for (int j = 0; j < n_jobs; j++) {
        b->relocSlots[j] = make_int2(frame_index[j], kf_index[j]);
        b->rrTh[j] = 10.f; b->rrOrb[j] = 100; b->rrTh[J + j] = 3.f; b->rrOrb[J + j] = 64;       // Tracking.cc:2323, :2337
    }
    int* P[5]; for (int k = 0; k < 5; k++) P[k] = b->d_rrP + k * rows;
    float* T[4]; for (int k = 0; k < 4; k++) T[k] = b->d_rrT + k * J * 16;
    const SdRelocPlan plan{b->d_rrGood.get(), b->d_rrNm.get(), n_jobs};
    const SdMapPoint* mps = (const SdMapPoint*)d_points;
    HIPCHK(hipMemsetAsync(b->d_relocErr, 0, 4, s));
    HIPCHK(hipMemcpyAsync(b->d_relocSlots, b->relocSlots.data(), J * sizeof(int2), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(T[0], Tcw_host, J * 64, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->d_rrTh, b->rrTh.data(), 2 * J * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->d_rrOrb, b->rrOrb.data(), 2 * J * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->d_rrCam, b->rrCam.data(), J * sizeof(sd_camera), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(b->d_rrMark, 0, markBytes, s));
    {
        ProfScope ps(b, s, K_RELOC_X);
        hipLaunchKernelGGL(k_reloc_begin, dim3(n_jobs), dim3(256), 0, s, b->d_count, b->d_relocSlots.get(), d_kf_point, d_frame_point, n_points, cap, P[0],
                           b->d_rrOutlier.get(), b->d_rrMark.get(), b->d_relocErr.get());
        LAUNCH_CHECK("k_reloc_begin");
    }
    SdRelocEdgeArgs E;
    E.kp = KPUN(b); E.uRight = b->d_uright; E.count = b->d_count; E.slots = b->d_relocSlots; E.mps = mps; E.cap = cap;
    const SdLevelTables LT = level_tables(b);
    for (int l = 0; l < SD_MAX_LEVELS; l++) E.invSigma2[l] = LT.invSigma2[l];
    // optimisation k: edges from Pin, pose T[k] -> T[k + 1]; then mvbOutlier and (Pout) the assignment that follows
    auto optimise = [&](int k, int step, const int* Pin, int* Pout, int minGood) -> int {
        E.P = Pin; E.Tprev = T[k]; E.Tcur = T[k + 1]; E.edges = b->d_rrEdges + k * rows; E.first = b->d_rrFirst + k * J; E.last = b->d_rrLast + k * J;
        {
            ProfScope ps(b, s, K_RELOC_E);
            hipLaunchKernelGGL(k_reloc_edges, dim3(n_jobs), dim3(256), 0, s, E, plan, step);
            LAUNCH_CHECK("k_reloc_edges");
        }
        SdPoseArgs A;
        A.edges = E.edges; A.first = E.first; A.last = E.last; A.cam = b->d_rrCam; A.Tcw = T[k + 1]; A.outlier = b->d_rrEdgeOut + k * rows;
        A.nGood = b->d_rrGood + k * J; A.map = nullptr;
        {
            ProfScope ps(b, s, K_RELOC_O);
            hipLaunchKernelGGL(k_pose_optimize, dim3(n_jobs), dim3(SD_POSE_THREADS), 0, s, A);
            LAUNCH_CHECK("k_pose_optimize");
        }
        {
            ProfScope ps(b, s, K_RELOC_X);
            hipLaunchKernelGGL(k_reloc_after, dim3(n_jobs), dim3(256), 0, s, (const sd_pose_edge*)E.edges, (const int*)E.first, (const int*)E.last,
                               (const uint8_t*)A.outlier, (const int*)A.nGood, Pin, Pout, b->d_rrOutlier.get(), cap, minGood, plan, step);
            LAUNCH_CHECK("k_reloc_after");
        }
        return SD_OK;
    };
    // search w: SearchByProjection(CurrentFrame, pKF, sFound, th, ORBdist) from Pin under pose Tk -> Pout
    auto search = [&](int w, int step, const float* Tk, const int* Pin, int* Pout) -> int {
        {
            ProfScope ps(b, s, K_RELOC_S);
            hipLaunchKernelGGL(k_reloc_search, dim3((cap + 3) / 4, n_jobs), dim3(256), 0, s, KPUN(b), b->d_desc, b->d_uright, b->d_sortedIdx, b->d_cellStart,
                               b->d_count, mps, d_point_desc, n_points, b->d_relocSlots.get(), Tk, (const float*)(b->d_rrTh + w * J), d_kf_point, Pin,
                               (const uint8_t*)nullptr, (const uint8_t*)b->d_rrMark.get(), b->d_relocList.get(), b->d_relocListN.get(),
                               b->d_rrExit + w * rows, b->d_relocErr.get(), LT, to_cam(cam), cap, plan, step);
            LAUNCH_CHECK("k_reloc_search");
        }
        {
            ProfScope ps(b, s, K_RELOC_A);
            hipLaunchKernelGGL(k_reloc_assign, dim3(n_jobs), dim3(64), (size_t)((cap + 31) / 32) * 4 + 16, s, KPUN(b), b->d_count, b->d_relocSlots.get(),
                               (const int*)(b->d_rrOrb + w * J), b->d_relocList.get(), b->d_relocListN.get(), d_kf_point, Pin, n_points, cap,
                               b->d_rrExit + w * rows, Pout, b->d_rrFrom + w * rows, b->d_rrBest + w * rows, b->d_rrNm + w * J, b->d_err.get(), plan, step);
            LAUNCH_CHECK("k_reloc_assign");
        }
        return SD_OK;
    };
    if ((rc = optimise(0, SD_RELOC_STEP_ALWAYS, P[0], P[1], 10)) != SD_OK) return rc;                 // :2311-2318
    if ((rc = search(0, SD_RELOC_STEP_SEARCH1, T[1], P[1], P[2])) != SD_OK) return rc;                // :2323
    if ((rc = optimise(1, SD_RELOC_STEP_OPT2, P[2], nullptr, 0)) != SD_OK) return rc;                 // :2327, no discard
    HIPCHK(hipMemsetAsync(b->d_rrMark, 0, markBytes, s));
    {
        ProfScope ps(b, s, K_RELOC_X);
        hipLaunchKernelGGL(k_reloc_mark, dim3(n_jobs), dim3(256), 0, s, (const int*)P[2], n_points, cap, b->d_rrMark.get(), plan, (int)SD_RELOC_STEP_SEARCH2);   // :2333-2336
        LAUNCH_CHECK("k_reloc_mark");
    }
    if ((rc = search(1, SD_RELOC_STEP_SEARCH2, T[2], P[2], P[3])) != SD_OK) return rc;                // :2337
    if ((rc = optimise(2, SD_RELOC_STEP_OPT3, P[3], P[4], INT_MIN)) != SD_OK) return rc;              // :2342-2346
    {
        ProfScope ps(b, s, K_RELOC_X);
        hipLaunchKernelGGL(k_reloc_finish, dim3((n_jobs + 255) / 256), dim3(256), 0, s, (const float*)b->d_rrT.get(), b->d_rrRes.get(), plan);
        LAUNCH_CHECK("k_reloc_finish");
    }
    b->rrJobs = n_jobs;
    if (d_results) *d_results = b->d_rrRes;
    return SD_OK;
}

static int refine_ready(sd_batch* b, int job, const char* who)
{
    if (!b) return set_err(SD_ERR_INVALID, std::string(who) + ": null batch");
    if (job < 0 || job >= b->rrJobs) return set_err(SD_ERR_INVALID, std::string(who) + ": no such job in the last sd_batch_relocalize_refine");
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int err = 0;
    HIPCHK(hipMemcpy(&err, b->d_relocErr, 4, hipMemcpyDeviceToHost));
    if (err) return set_err(SD_ERR_INVALID, "relocalize_refine: a d_kf_point or d_frame_point entry names a point outside its table");
    return SD_OK;
}

int sd_batch_download_reloc(sd_batch* b, int job, sd_reloc_result* result, int32_t* frame_point, uint8_t* outlier, int cap)
{
    int rc = refine_ready(b, job, "download_reloc");
    if (rc != SD_OK) return rc;
    const size_t n = (size_t)b->plan.kpCap, rows = (size_t)b->rrJobs * n;
    if ((frame_point || outlier) && cap < b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "the reloc rows need kp_capacity entries");
    if (result) HIPCHK(hipMemcpy(result, b->d_rrRes + job, sizeof(sd_reloc_result), hipMemcpyDeviceToHost));
    if (frame_point) HIPCHK(hipMemcpy(frame_point, b->d_rrP + 4 * rows + (size_t)job * n, n * 4, hipMemcpyDeviceToHost));
    if (outlier) HIPCHK(hipMemcpy(outlier, b->d_rrOutlier + (size_t)job * n, n, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_batch_download_reloc_optimisation(sd_batch* b, int job, int stage, sd_pose_edge* edges, uint8_t* edge_outlier, int cap_edges, int* n_edges,
                                         float* Tcw_in)
{
    if (stage < 0 || stage > 2 || !n_edges) return set_err(SD_ERR_INVALID, "bad download_reloc_optimisation arguments");
    int rc = refine_ready(b, job, "download_reloc_optimisation");
    if (rc != SD_OK) return rc;
    const size_t J = (size_t)b->rrJobs, rows = J * b->plan.kpCap;
    int fl[2];
    HIPCHK(hipMemcpy(&fl[0], b->d_rrFirst + stage * J + job, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&fl[1], b->d_rrLast + stage * J + job, 4, hipMemcpyDeviceToHost));
    const int n = fl[1] - fl[0];
    *n_edges = n;
    if ((edges || edge_outlier) && n > cap_edges) return set_err(SD_ERR_CAPACITY, "reloc edge buffers too small");
    if (edges && n > 0) HIPCHK(hipMemcpy(edges, b->d_rrEdges + stage * rows + fl[0], (size_t)n * sizeof(sd_pose_edge), hipMemcpyDeviceToHost));
    if (edge_outlier && n > 0) HIPCHK(hipMemcpy(edge_outlier, b->d_rrEdgeOut + stage * rows + fl[0], (size_t)n, hipMemcpyDeviceToHost));
    if (Tcw_in) HIPCHK(hipMemcpy(Tcw_in, b->d_rrT + (stage * J + job) * 16, 64, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_batch_download_reloc_search(sd_batch* b, int job, int which, int32_t* frame_point_in, int32_t* frame_point_out, int32_t* from_kf,
                                   int32_t* exits, int32_t* best, int cap, int* nmatches)
{
    if (which < 0 || which > 1) return set_err(SD_ERR_INVALID, "bad download_reloc_search arguments");
    int rc = refine_ready(b, job, "download_reloc_search");
    if (rc != SD_OK) return rc;
    const size_t n = (size_t)b->plan.kpCap, J = (size_t)b->rrJobs, rows = J * n, r0 = (size_t)job * n;
    if ((frame_point_in || frame_point_out || from_kf || exits || best) && cap < b->plan.kpCap)
        return set_err(SD_ERR_CAPACITY, "the reloc rows need kp_capacity entries");
    if (nmatches) HIPCHK(hipMemcpy(nmatches, b->d_rrNm + which * J + job, 4, hipMemcpyDeviceToHost));
    if (frame_point_in) HIPCHK(hipMemcpy(frame_point_in, b->d_rrP + (which + 1) * rows + r0, n * 4, hipMemcpyDeviceToHost));
    if (frame_point_out) HIPCHK(hipMemcpy(frame_point_out, b->d_rrP + (which + 2) * rows + r0, n * 4, hipMemcpyDeviceToHost));
    if (from_kf) HIPCHK(hipMemcpy(from_kf, b->d_rrFrom + which * rows + r0, n * 4, hipMemcpyDeviceToHost));
    if (exits) HIPCHK(hipMemcpy(exits, b->d_rrExit + which * rows + r0, n * 4, hipMemcpyDeviceToHost));
    if (best) HIPCHK(hipMemcpy(best, b->d_rrBest + which * rows + r0, n * sizeof(int2), hipMemcpyDeviceToHost));
    return SD_OK;
}
