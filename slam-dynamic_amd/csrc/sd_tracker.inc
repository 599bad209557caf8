// sd_tracker: the Frame-level boundary (include/sd_frontend.h).  Host orchestration of one frame per lane:
//   Tracking::GrabImage* -> Frame::Frame (x5) -> Track_new's dynamic block -> [match vs mLastFrame] -> q_frame / mLastFrame.
// Included by sd_api.hip inside its extern "C" block.  Reference: src/Tracking.cc:170-343, 586-666, 952-1086;
// src/Frame.cc:66-461.  ONE host synchronisation per call in the common case: everything that decides what runs next
// (objects.empty(), nmatches < 20, TrackHomo's flag, Separate's return value) is evaluated on the device (k_lane_gate, the
// `active` / `redoBelow` arguments of the matcher and model-fit kernels); the host replays the queue bookkeeping from the
// per-lane summary afterwards.  Only a lane whose TrackHomo failed AND whose queue holds a second frame more than 0.2 s
// old (cameras above 10 fps) costs another round.

struct sd_tracker {
    sd_tracker_params p;
    std::unique_ptr<sd_batch> b;
    int S = 0, ipl = 1, nCur = 0, R = 0, ring0 = 0;
    struct QE { double t; int slot; int hasBoxes; int frameId; };
    struct Lane {
        std::vector<QE> q;                 // Tracking::q_frame, front = oldest
        std::vector<int> freeSlots;        // ring slots not referenced by q
        int frameNo = 0;
        int lastSlot = -1;                 // mLastFrame (== the newest queue entry)
        int nLast = 0;                     // mLastFrame.objects / box_idx / omit / box_velocity
        double lastObjects[SD_MAXB][4]; int lastIdx[SD_MAXB]; uint8_t lastOmit[SD_MAXB]; double lastVel[SD_MAXB][2];
    };
    std::vector<Lane> lanes;
    SdDevBuf<int> d_want, d_active, d_activeLast, d_slotList;
    SdDevBuf<SdLaneSummary> d_sum;
    SdLaneSummary* h_sum = nullptr;        // pinned
    SdDevBuf<uint8_t> d_hostImg; SdDevBuf<uint16_t> d_hostDepth;      // staging of sd_tracker_track_host
    // host staging (must outlive the asynchronous uploads of a call)
    std::vector<double> hBoxes; std::vector<int32_t> hNb, hIdx, hSlots, hCur, hRef, hLast, hWant, hActiveLast, hResetSlots;
    std::vector<uint8_t> hOmit; std::vector<double> hVel;
    std::vector<float> hI, hTcw, hTrw, hTlw, hTwc;
    std::vector<std::vector<float>> poseOfSlot;   // Tcw of the frame kept in a ring slot
    // monocular: mpIniORBextractor (Tracking.cc:127-128) and its workspace; the lanes' results are moved into `b` (same row stride)
    std::unique_ptr<sd_extractor> exIni; std::unique_ptr<sd_batch> bIni;
    // time-batched mode (sd_tracker_prefetch): the history-free part of up to 2 x lookahead frames per lane lives in `bp`
    std::unique_ptr<sd_batch> bp[2];                                                   // one workspace per outstanding block
    // Invariant the pool slots rely on: sd_tracker_track ends with a synchronisation (tracker_summary), so when a block's workspace is
    // refilled -- only a later prefetch / import can do that -- every pool copy-out that read it has completed.  Prefetch and import therefore
    // need no ordering against the copy-out; `ready` orders the other direction (fill before copy-out / export).
    struct Block { int n = 0, next = 0; hipEvent_t ready = nullptr; };                 // frames of the block, `next` consumed so far
    Block blocks[2]; int blockHead = 0, blockCount = 0;
    // caller-owned SLAM state (sd_tracker_set_state); empty = the automatic rule of the sharded batch mode
    std::vector<int32_t> state;
    // opt-in TrackWithMotionModel tail (sd_tracker_set_pose_optimization) and its per-lane results of the last call
    bool poseOpt = false, poseRanStep = false;
    std::vector<sd_pose_result> poseRes;
    bool notInitialised(int l) const { return state.empty() ? lanes[l].frameNo == 0 : !(state[l] & 1); }         // mState == NOT_INITIALIZED on entry to Track_new
    bool useIniExtractor(int l) const { return bIni && (state.empty() ? lanes[l].frameNo < 2 : !(state[l] & 1)); } // GrabImageMonocular, Tracking.cc:335-338
    bool canTrackHomo(int l) const { return state.empty() ? lanes[l].frameNo >= 2 : (state[l] & 2) != 0; }       // mState==OK && !mVelocity.empty(), Tracking.cc:971
    ~sd_tracker()
    {
        if (b) (void)hipDeviceSynchronize();
        if (h_sum) (void)hipHostFree(h_sum);
        for (auto& bl : blocks) if (bl.ready) (void)hipEventDestroy(bl.ready);
    }
};

static void tracker_reset_lanes(sd_tracker* t)
{
    t->lanes.assign(t->S, sd_tracker::Lane());
    for (int s = 0; s < t->S; s++)
        for (int k = t->R - 1; k >= 0; k--) t->lanes[s].freeSlots.push_back(t->ring0 + s * t->R + k);
}

int sd_tracker_create(sd_tracker** out, sd_extractor* ex, const sd_tracker_params* p)
{
    if (!out) return SD_ERR_INVALID;
    *out = nullptr;
    if (!ex || !p || p->n_lanes < 1 || p->width < 1 || p->height < 1 || (p->channels != 1 && p->channels != 3 && p->channels != 4) ||
        p->sensor < SD_SENSOR_MONOCULAR || p->sensor > SD_SENSOR_RGBD || !cam_ok(&p->cam) || !(p->fps > 0) || p->ini_features < 0 || p->lookahead < 0 ||
        (p->depth_type != SD_DEPTH_U16 && p->depth_type != SD_DEPTH_F32))
        return set_err(SD_ERR_INVALID, "bad tracker parameters");
    if (p->sensor != SD_SENSOR_MONOCULAR && !(p->cam.mbf > 0)) return set_err(SD_ERR_INVALID, "Camera.bf must be positive");
    std::unique_ptr<sd_tracker> t(new sd_tracker());
    t->p = *p;
    t->S = p->n_lanes;
    t->ipl = p->sensor == SD_SENSOR_STEREO ? 2 : 1;
    t->nCur = t->S * t->ipl;
    t->R = (int)ceil(0.3 * (double)p->fps) + 1;           // q_frame never holds more than ceil(0.3 * fps) frames; + 1: the incoming one
    t->ring0 = t->nCur;
    int minCap = 0;
    if (p->sensor == SD_SENSOR_MONOCULAR && p->ini_features > 0 && p->ini_features != ex->prm.nfeatures) {
        // mpIniORBextractor = new ORBextractor(2*nFeatures, fScaleFactor, nLevels, fIniThFAST, fMinThFAST) (Tracking.cc:127-128)
        t->exIni.reset(new sd_extractor(*ex));
        sd_params_init(t->exIni->prm, p->ini_features, (float)ex->prm.scaleFactor, ex->prm.nlevels, ex->prm.iniTh, ex->prm.minTh);
        memcpy(t->exIni->prm.blurTaps, ex->prm.blurTaps, sizeof(ex->prm.blurTaps));
        SdPlan a, c;
        if (!sd_plan_build(a, ex->prm, p->width, p->height) || !sd_plan_build(c, t->exIni->prm, p->width, p->height))
            return set_err(SD_ERR_UNSUPPORTED, a.error.empty() ? c.error : a.error);
        minCap = a.kpCap > c.kpCap ? a.kpCap : c.kpCap;
    }
    int rc = batch_create_impl(t->b, ex, p->width, p->height, t->nCur + t->S * t->R, minCap);
    if (rc == SD_OK && t->exIni) rc = batch_create_impl(t->bIni, t->exIni.get(), p->width, p->height, t->S, minCap);
    for (int k = 0; k < 2 && rc == SD_OK && p->lookahead > 0; k++) rc = batch_create_impl(t->bp[k], ex, p->width, p->height, p->lookahead * t->nCur, minCap);
    if (rc != SD_OK) return rc;
    sd_batch* b = t->b.get();
    {
        const float K4[4] = {p->cam.fx, p->cam.fy, p->cam.cx, p->cam.cy};
        rc = sd_batch_set_distortion(b, K4, p->dist);              // Camera.k1 != 0 (TUM1 / TUM2 / EuRoC): mvKeysUn becomes a second array
        for (auto& q : t->bp) if (rc == SD_OK && q) rc = sd_batch_set_distortion(q.get(), K4, p->dist);
        if (rc == SD_OK) rc = ensure_motion(b);           // the model-fit buffers now, not inside the first step
        if (rc != SD_OK) return rc;
    }
    HIPCHK(t->d_want.alloc((size_t)t->S * 4));
    HIPCHK(t->d_active.alloc((size_t)t->S * 4));
    HIPCHK(t->d_activeLast.alloc((size_t)t->S * 4));
    HIPCHK(t->d_slotList.alloc((size_t)t->S * 4));
    const size_t sumBytes = (size_t)t->S * (sizeof(SdLaneSummary) + sizeof(SdPoseSummary));   // lane summaries, then the pose tail's
    HIPCHK(t->d_sum.alloc(sumBytes));
    HIPCHK(hipHostMalloc((void**)&t->h_sum, sumBytes, hipHostMallocDefault));
    for (auto& bl : t->blocks) if (t->bp[0]) HIPCHK(hipEventCreateWithFlags(&bl.ready, hipEventDisableTiming));
    t->poseOfSlot.assign(b->maxImages, std::vector<float>());
    t->hI.assign((size_t)t->S * 16, 0.f);
    for (int s = 0; s < t->S; s++) for (int k = 0; k < 4; k++) t->hI[(size_t)s * 16 + 5 * k] = 1.f;
    tracker_reset_lanes(t.get());
    *out = t.release();
    return SD_OK;
}

int sd_tracker_destroy(sd_tracker* t) { delete t; return SD_OK; }

int sd_tracker_reset(sd_tracker* t)
{
    if (!t) return SD_ERR_INVALID;
    HIPCHK(hipDeviceSynchronize());
    tracker_reset_lanes(t);
    t->blockHead = 0; t->blockCount = 0;
    return SD_OK;
}

// What follows extraction in the history-free half of F frames (left slots f * ipl of `b`): UndistortKeyPoints (the identity and free when
// Camera.k1 == 0), then the stereo / RGB-D association or the monocular fill
static int tracker_associate(sd_tracker* t, sd_batch* b, int F, const void* d_depth, size_t depth_stride_elems, size_t depth_pitch_elems, hipStream_t s)
{
    const sd_camera* cam = &t->p.cam;
    std::vector<int32_t> slots(F);
    for (int f = 0; f < F; f++) slots[f] = f * t->ipl;
    int rc = sd_batch_undistort(b, F, slots.data(), s);
    if (rc != SD_OK) return rc;
    if (t->p.sensor == SD_SENSOR_STEREO) return sd_batch_stereo_match(b, F, cam->mbf, cam->fx, s);
    if (t->p.sensor == SD_SENSOR_RGBD) {
        const float factor = fabsf(t->p.depth_map_factor) < 1e-5f ? 1.0f : 1.0f / t->p.depth_map_factor;       // Tracking.cc:141-146
        // `if((fabs(mDepthMapFactor-1.0f)>1e-5) || imDepth.type()!=CV_32F) imDepth.convertTo(imDepth,CV_32F,mDepthMapFactor)` (Tracking.cc:271-272)
        if (t->p.depth_type == SD_DEPTH_F32)
            return sd_batch_rgbd_from_f32_scaled(b, (const float*)d_depth, depth_stride_elems, depth_pitch_elems, F, fabsf(factor - 1.0f) > 1e-5f ? factor : 1.0f, cam->mbf, s);
        return sd_batch_rgbd_from_u16(b, (const uint16_t*)d_depth, depth_stride_elems, depth_pitch_elems, F, factor, cam->mbf, s);
    }
    hipLaunchKernelGGL(k_fill_mono, dim3((b->plan.kpCap + 255) / 256, F), dim3(256), 0, s, b->d_count, b->d_uright, b->d_depth, b->plan.kpCap);
    LAUNCH_CHECK("k_fill_mono");
    return SD_OK;
}

// The history-free half of a frame for `n` frames per lane in one batch (images in frame-major order: frame k, lane s, eye e): GrabImage*'s
// conversion, ORB extraction, then tracker_associate.  Slot of (k, s, e) in `b` = (k * S + s) * ipl + e.
static int tracker_front_half(sd_tracker* t, sd_batch* b, int n, const uint8_t* d_images, size_t stride, size_t image_pitch, const void* d_depth,
                              size_t depth_stride_elems, size_t depth_pitch_elems, hipStream_t s)
{
    const int F = n * t->S;
    int rc = sd_batch_extract_pixels_device(b, d_images, stride, image_pitch, t->p.channels, t->p.rgb_order, F * t->ipl, s);
    if (rc != SD_OK) return rc;
    return tracker_associate(t, b, F, d_depth, depth_stride_elems, depth_pitch_elems, s);
}

int sd_tracker_prefetch(sd_tracker* t, const uint8_t* d_images, size_t stride, size_t image_pitch, const void* d_depth,
                        size_t depth_stride_elems, size_t depth_pitch_elems, int n_frames, void* stream_)
{
    if (!t || !d_images || n_frames < 1) return set_err(SD_ERR_INVALID, "bad prefetch arguments");
    if (!t->bp[0] || n_frames > t->p.lookahead) return set_err(SD_ERR_STATE, "prefetch needs params.lookahead >= n_frames");
    if (t->bIni) return set_err(SD_ERR_UNSUPPORTED, "prefetch with a monocular initialisation extractor");
    if (t->p.sensor == SD_SENSOR_RGBD && !d_depth) return set_err(SD_ERR_INVALID, "RGB-D tracking needs a depth image");
    if (t->blockCount == 2) return set_err(SD_ERR_STATE, "two prefetched blocks are outstanding: consume one with sd_tracker_track first");
    const int slot = (t->blockHead + t->blockCount) & 1;
    sd_tracker::Block& B = t->blocks[slot];
    B.n = n_frames; B.next = 0;
    sd_batch* bp = t->bp[slot].get();
    hipStream_t s = stream_ ? (hipStream_t)stream_ : bp->stream;
    int rc = tracker_front_half(t, bp, n_frames, d_images, stride, image_pitch, d_depth, depth_stride_elems, depth_pitch_elems, s);
    if (rc != SD_OK) return rc;
    HIPCHK(hipEventRecord(B.ready, s));
    t->blockCount++;
    return SD_OK;
}

// The record of one prefetched (frame, lane): the FRONT arrays of its left pool slot back to back, each padded to 16 bytes
static size_t record_pad(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

size_t sd_tracker_prefetched_record_bytes(const sd_tracker* t)
{
    if (!t || !t->bp[0]) return 0;
    SdSlotArray A[SD_COPY_SEGS];
    size_t bytes = 0;
    for (int i = 0, n = frame_arrays(t->bp[0].get(), SD_FRAME_FRONT, A); i < n; i++) bytes += record_pad(A[i].bytes);
    return bytes;
}

static bool record_stride_ok(const sd_tracker* t, size_t stride) { return t->bp[0] && stride >= sd_tracker_prefetched_record_bytes(t) && (stride & 15) == 0; }

// pool slots of `bp` -> records `stride` bytes apart (toRecord), or the records -> the pool slots
static SdCopyTable record_table(const sd_batch* bp, char* records, size_t stride, bool toRecord)
{
    SdCopyTable T = frame_copy_table(bp, bp, SD_FRAME_FRONT);
    size_t off = 0;
    for (int i = 0; i < T.n; i++) {
        if (toRecord) { T.dst[i] = records + off; T.dstStride[i] = (unsigned)stride; }
        else { T.src[i] = records + off; T.srcStride[i] = (unsigned)stride; }
        off += record_pad(T.bytes[i]);
    }
    return T;
}

int sd_tracker_export_prefetched(sd_tracker* t, int first_frame, int n_frames, void* d_records, size_t record_stride, void* stream_)
{
    if (!t || !d_records || first_frame < 0 || n_frames < 1 || ((size_t)d_records & 15)) return set_err(SD_ERR_INVALID, "bad export_prefetched arguments");
    if (!t->bp[0] || t->blockCount == 0) return set_err(SD_ERR_STATE, "export_prefetched: no prefetched block is outstanding");
    const int slot = (t->blockHead + t->blockCount - 1) & 1;               // the newest block
    sd_tracker::Block& B = t->blocks[slot];
    if (first_frame + n_frames > B.n) return set_err(SD_ERR_INVALID, "export_prefetched: frames beyond the block");
    if (!record_stride_ok(t, record_stride)) return set_err(SD_ERR_INVALID, "export_prefetched: record stride below the record size or not a multiple of 16");
    sd_batch* bp = t->bp[slot].get();
    hipStream_t s = stream_ ? (hipStream_t)stream_ : bp->stream;
    HIPCHK(hipStreamWaitEvent(s, B.ready, 0));
    return launch_copy_frames(record_table(bp, (char*)d_records, record_stride, true), 4, n_frames * t->S, nullptr, first_frame * t->nCur, t->ipl, 0, 1, s);
}

int sd_tracker_import_prefetched(sd_tracker* t, const void* d_records, size_t record_stride, int n_frames, void* stream_)
{
    if (!t || !d_records || n_frames < 1 || ((size_t)d_records & 15)) return set_err(SD_ERR_INVALID, "bad import_prefetched arguments");
    if (!t->bp[0] || n_frames > t->p.lookahead) return set_err(SD_ERR_STATE, "import_prefetched needs params.lookahead >= n_frames");
    if (t->bIni) return set_err(SD_ERR_UNSUPPORTED, "prefetched frames with a monocular initialisation extractor");
    if (t->blockCount == 2) return set_err(SD_ERR_STATE, "two prefetched blocks are outstanding: consume one with sd_tracker_track first");
    if (!record_stride_ok(t, record_stride)) return set_err(SD_ERR_INVALID, "import_prefetched: record stride below the record size or not a multiple of 16");
    const int slot = (t->blockHead + t->blockCount) & 1;
    sd_tracker::Block& B = t->blocks[slot];
    sd_batch* bp = t->bp[slot].get();
    hipStream_t s = stream_ ? (hipStream_t)stream_ : bp->stream;
    int rc = launch_copy_frames(record_table(bp, (char*)const_cast<void*>(d_records), record_stride, false), 4, n_frames * t->S, nullptr, 0, 1, 0, t->ipl, s);
    if (rc != SD_OK) return rc;
    B.n = n_frames; B.next = 0;
    HIPCHK(hipEventRecord(B.ready, s));
    t->blockCount++;
    return SD_OK;
}

int sd_tracker_discard_prefetched(sd_tracker* t)
{
    if (!t) return SD_ERR_INVALID;
    if (t->blockCount == 0) return set_err(SD_ERR_STATE, "discard_prefetched: no prefetched block is outstanding");
    t->blockCount--;                                                        // the newest block; the oldest keeps its place at blockHead
    return SD_OK;
}

int sd_tracker_set_state(sd_tracker* t, const int32_t* state)
{
    if (!t) return SD_ERR_INVALID;
    if (!state) t->state.clear(); else t->state.assign(state, state + t->S);
    return SD_OK;
}

// The back end's MapPoints of the frame just tracked: they replace the map-point table of the lane's mLastFrame / newest q_frame
// entry (one ring slot), which later frames project (Tracking.cc:998-1010, 1714-1741).
int sd_tracker_set_mappoints(sd_tracker* t, const float* xw, const uint8_t* flags, const int32_t* n)
{
    if (!t || !xw || !flags || !n) return set_err(SD_ERR_INVALID, "bad set_mappoints arguments");
    sd_batch* b = t->b.get();
    const size_t cap = b->plan.kpCap;
    hipStream_t s = b->lastStream;
    for (int l = 0; l < t->S; l++) {
        if (n[l] < 0) continue;
        const int slot = t->lanes[l].lastSlot;
        if (slot < 0) return set_err(SD_ERR_STATE, "set_mappoints before the lane's first frame");
        if ((size_t)n[l] > cap) return set_err(SD_ERR_CAPACITY, "more map points than key-point slots");
        HIPCHK(hipMemsetAsync(b->d_flags + (size_t)slot * cap, 0, cap, s));
        if (n[l] > 0) {
            HIPCHK(hipMemcpyAsync(b->d_xw + (size_t)slot * cap * 3, xw + (size_t)l * cap * 3, (size_t)n[l] * 12, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(b->d_flags + (size_t)slot * cap, flags + (size_t)l * cap, (size_t)n[l], hipMemcpyHostToDevice, s));
        }
    }
    HIPCHK(hipStreamSynchronize(s));          // the caller's buffers are free again
    return SD_OK;
}

int sd_tracker_batch(sd_tracker* t, sd_batch** b)
{
    if (!t || !b) return SD_ERR_INVALID;
    *b = t->b.get();
    return SD_OK;
}

// The head of Track_new's loop (Tracking.cc:623-631) WITHOUT side effects: index into the lane's queue of the frame
// TrackHomo would run against if the current frame has boxes, starting the scan at queue position `from`; -1 = none.
static int tracker_peek_candidate(const sd_tracker::Lane& L, double t, int from)
{
    for (size_t k = from; k < L.q.size(); k++) {
        if (!(t - L.q[k].t > 0.2f)) return -1;
        if (L.q[k].hasBoxes) return (int)k;        // box-less fronts are popped and skipped
    }
    return -1;
}

#define TRK(call) do { int rc_ = (call); if (rc_ != SD_OK) return rc_; } while (0)

// One round of TrackHomo + Separate + UpdateFrame for the lanes whose hWant entry is set (pair index = lane).
static int tracker_dynamic_round(sd_tracker* t, const float* Tcw, hipStream_t s)
{
    sd_batch* b = t->b.get();
    const int S = t->S;
    const sd_camera* cam = &t->p.cam;
    const float th = t->p.sensor == SD_SENSOR_STEREO ? 7.0f : 15.0f;           // Tracking.cc:990-994
    const int bMono = t->p.sensor == SD_SENSOR_MONOCULAR;
    HIPCHK(hipMemcpyAsync(t->d_want, t->hWant.data(), (size_t)S * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_lane_gate, dim3((S + 63) / 64), dim3(64), 0, s, b->d_fb, t->d_want, t->d_active, S, t->ipl);
    LAUNCH_CHECK("k_lane_gate");
    TRK(search_by_projection_impl(b, 0, S, t->hCur.data(), t->hRef.data(), Tcw, t->hTrw.data(), cam, th, bMono, 1, nullptr, nullptr, s, t->d_active, 0, 1));
    TRK(search_by_projection_impl(b, 0, S, t->hCur.data(), t->hRef.data(), Tcw, t->hTrw.data(), cam, 2 * th, bMono, 1, nullptr, nullptr, s, t->d_active, 20, 0));
    TRK(estimate_motion_impl(b, S, s, t->d_active, 20));
    TRK(separate_impl(b, S, t->hCur.data(), t->hRef.data(), nullptr, nullptr, nullptr, nullptr, nullptr, s, t->hLast.data(), t->d_active));
    TRK(sd_batch_update_frame(b, 1, s));
    if (b->hasDist) {                                              // UpdateFrame appended key points: their mvKeysUn entries
        std::vector<int32_t> cur(S);
        for (int l = 0; l < S; l++) cur[l] = l * t->ipl;
        TRK(sd_batch_undistort(b, S, cur.data(), s));
    }
    return SD_OK;
}

// TrackWithMotionModel's matcher against mLastFrame (pairs [S, 2S)); with pose mode also its tail: the 2*th retry below 20 matches
// (the redoBelow path TrackHomo uses), then PoseOptimization of the lanes with >= 20 matches (Tracking.cc:1741-1759)
static int tracker_last_matcher(sd_tracker* t, const int32_t* cur, const int32_t* last, const float* Tcw, hipStream_t s)
{
    sd_batch* b = t->b.get();
    const int S = t->S, bMono = t->p.sensor == SD_SENSOR_MONOCULAR;
    const float th = t->p.sensor == SD_SENSOR_STEREO ? 7.0f : 15.0f;           // Tracking.cc:1727-1731
    TRK(search_by_projection_impl(b, S, S, cur, last, Tcw, t->hTlw.data(), &t->p.cam, th, bMono, 1, nullptr, nullptr, s, t->d_activeLast, 0, 1));
    if (!t->poseOpt) return SD_OK;
    TRK(search_by_projection_impl(b, S, S, cur, last, Tcw, t->hTlw.data(), &t->p.cam, 2 * th, bMono, 1, nullptr, nullptr, s, t->d_activeLast, 20, 0));
    std::vector<int32_t> pairs(S);
    for (int l = 0; l < S; l++) pairs[l] = S + l;
    TRK(batch_pose_impl(b, S, pairs.data(), nullptr, s, t->d_activeLast, S, 20));
    t->poseRanStep = true;
    return SD_OK;
}

static int tracker_summary(sd_tracker* t, int haveLast, hipStream_t s)
{
    sd_batch* b = t->b.get();
    b->lastStream = s;
    hipLaunchKernelGGL(k_lane_summary, dim3(t->S), dim3(64), 0, s, b->d_fb, b->d_count, b->d_moRes, b->d_sepRet, b->d_nmatch, b->d_npairs, t->S, t->ipl,
                       haveLast, t->d_sum);
    LAUNCH_CHECK("k_lane_summary");
    if (t->poseRanStep) {
        hipLaunchKernelGGL(k_pose_lane_summary, dim3(t->S), dim3(256), 0, s, b->d_poseEdges, b->d_poseFirst, b->d_poseLast, b->d_poseT, b->d_poseOut,
                           b->d_poseGood, b->d_poseRan, b->d_match, b->d_flags, b->d_pairIdx, b->d_nmatch, t->d_activeLast, t->S, b->plan.kpCap,
                           (SdPoseSummary*)(t->d_sum + t->S));
        LAUNCH_CHECK("k_pose_lane_summary");
    }
    const size_t bytes = (size_t)t->S * (sizeof(SdLaneSummary) + (t->poseRanStep ? sizeof(SdPoseSummary) : 0));
    HIPCHK(hipMemcpyAsync(t->h_sum, t->d_sum, bytes, hipMemcpyDeviceToHost, s));
    return sd_batch_sync(b);
}

int sd_tracker_track(sd_tracker* t, const uint8_t* d_images, size_t stride, size_t image_pitch, const void* d_depth,
                     size_t depth_stride_elems, size_t depth_pitch_elems, const double* boxes, const int32_t* n_boxes,
                     const double* timestamps, const float* Tcw_in, const float* Twc_in, sd_lane_result* results, void* stream_)
{
    if (!t || !timestamps) return set_err(SD_ERR_INVALID, "bad track arguments");
    const bool fromPool = d_images == nullptr;                 // the history-free half was run ahead by sd_tracker_prefetch
    if (fromPool && t->blockCount == 0) return set_err(SD_ERR_INVALID, "no image and no prefetched frame");
    if (!fromPool && t->blockCount > 0) return set_err(SD_ERR_STATE, "prefetched frames are outstanding: consume them (d_images == NULL) first");
    if (!fromPool && t->p.sensor == SD_SENSOR_RGBD && !d_depth) return set_err(SD_ERR_INVALID, "RGB-D tracking needs a depth image");
    if ((Tcw_in == nullptr) != (Twc_in == nullptr)) return set_err(SD_ERR_INVALID, "give both Tcw and Twc or neither");
    sd_batch* b = t->b.get();
    const int S = t->S, ipl = t->ipl;
    hipStream_t s = stream_ ? (hipStream_t)stream_ : b->stream;
    const sd_camera* cam = &t->p.cam;
    const float* Tcw = Tcw_in ? Tcw_in : t->hI.data();
    const float* Twc = Twc_in ? Twc_in : t->hI.data();
    const bool withBoxes = t->p.sensor != SD_SENSOR_MONOCULAR && boxes && n_boxes;     // the monocular ctor takes no boxes (Frame.cc:406)

    // ---- Frame::boxTrack on the host (f64, a handful of boxes).  It reads host state only (mLastFrame's boxes), so it runs FIRST: every
    // argument error it can raise (more than SD_MAX_BOXES boxes, the re-injected boxes overflowing the table) and an exhausted ring leave the
    // tracker -- and in the time-batched mode the pool of prefetched frames -- exactly as they were, and the call can be repeated
    for (int l = 0; l < S; l++)
        if (t->lanes[l].freeSlots.empty()) return set_err(SD_ERR_STATE, "tracker ring exhausted");
    t->hBoxes.assign((size_t)S * SD_MAXB * 4, 0.0); t->hNb.assign(S, 0); t->hIdx.assign((size_t)S * SD_MAXB, 0);
    t->hOmit.assign((size_t)S * SD_MAXB, 0); t->hVel.assign((size_t)S * SD_MAXB * 2, 0.0);
    t->hSlots.clear(); t->hResetSlots.clear();
    std::vector<int> sepLane;
    for (int l = 0; l < S; l++) {
        sd_tracker::Lane& L = t->lanes[l];
        const bool has = withBoxes && n_boxes[l] >= 0;
        if (!has) { t->hResetSlots.push_back(l * ipl); continue; }
        if (n_boxes[l] > SD_MAXB) return set_err(SD_ERR_CAPACITY, "more than SD_MAX_BOXES boxes in a frame");
        double* bx = &t->hBoxes[(size_t)l * SD_MAXB * 4];
        memcpy(bx, boxes + (size_t)l * SD_MAXB * 4, (size_t)n_boxes[l] * 32);
        int nOut = 0;
        TRK(sd_box_track(bx, n_boxes[l], SD_MAXB, &L.lastObjects[0][0], L.nLast, L.lastIdx, L.lastOmit, &L.lastVel[0][0], t->p.width, t->p.height,
                         &t->hIdx[(size_t)l * SD_MAXB], &t->hOmit[(size_t)l * SD_MAXB], &t->hVel[(size_t)l * SD_MAXB * 2], &nOut));
        t->hNb[l] = nOut;
        if (nOut == 0) { t->hResetSlots.push_back(l * ipl); continue; }
        sepLane.push_back(l);
        t->hSlots.push_back(l * ipl);
    }

    // ---- GrabImage* + ORB extraction of both eyes
    if (fromPool) {
        // frame `next` of the oldest outstanding block: its left slots (key points, descriptors, mvKeysUn, mvuRight / mvDepth, level counts)
        // move to the lanes' current slots in one launch; nothing downstream reads the right eye's slot or the pyramid again
        sd_tracker::Block& B = t->blocks[t->blockHead];
        sd_batch* bp = t->bp[t->blockHead].get();
        HIPCHK(hipStreamWaitEvent(s, B.ready, 0));
        TRK(launch_copy_frames(frame_copy_table(bp, b, SD_FRAME_FRONT), 8, S, nullptr, B.next * t->nCur, ipl, 0, ipl, s));
        b->nExtracted = t->nCur; b->nStereo = t->p.sensor == SD_SENSOR_STEREO ? S : 0; b->lastStream = s;
        for (int l = 0; l < S; l++) { b->slotValid[l * ipl] = 1; b->gridValid[l * ipl] = 0; }
        if (++B.next == B.n) { t->blockHead ^= 1; t->blockCount--; }
    } else {
        int nIni = 0;
        for (int l = 0; l < S; l++) nIni += t->useIniExtractor(l) ? 1 : 0;
        if (nIni < S) TRK(sd_batch_extract_pixels_device(b, d_images, stride, image_pitch, t->p.channels, t->p.rgb_order, t->nCur, s));
        if (nIni > 0) {                                            // monocular lanes that are not initialised: mpIniORBextractor (Tracking.cc:335-338)
            sd_batch* bi = t->bIni.get();
            TRK(sd_batch_extract_pixels_device(bi, d_images, stride, image_pitch, t->p.channels, t->p.rgb_order, S, s));
            const SdCopyTable T = frame_copy_table(bi, b, SD_FRAME_EXTRACT);
            for (int l0 = 0; l0 < S;) {                            // runs of consecutive lanes: one launch each
                if (!t->useIniExtractor(l0)) { l0++; continue; }
                int l1 = l0;
                while (l1 < S && t->useIniExtractor(l1)) l1++;
                TRK(launch_copy_frames(T, 8, l1 - l0, nullptr, l0, 1, l0, 1, s));
                l0 = l1;
            }
            b->nExtracted = S; b->nStereo = 0; b->lastStream = s;
            for (int l = 0; l < S; l++) { b->slotValid[l] = 1; b->gridValid[l] = 0; }
        }
    }
    // ---- UndistortKeyPoints, then the stereo / RGB-D association (done ahead by sd_tracker_prefetch for a pool frame)
    if (!fromPool) TRK(tracker_associate(t, b, S, d_depth, depth_stride_elems, depth_pitch_elems, s));
    std::vector<int32_t> curSlots(S);
    for (int l = 0; l < S; l++) curSlots[l] = l * ipl;
    // ---- firstSeparate + split on the device (boxTrack ran on the host above)
    if (!t->hResetSlots.empty()) {
        const int n = (int)t->hResetSlots.size();
        HIPCHK(hipMemcpyAsync(t->d_slotList, t->hResetSlots.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_reset_boxes, dim3((n + 63) / 64), dim3(64), 0, s, b->d_fb, b->d_count, t->d_slotList, n);
        LAUNCH_CHECK("k_reset_boxes");
    }
    if (!sepLane.empty()) {
        const int n = (int)sepLane.size();
        std::vector<double> pb((size_t)n * SD_MAXB * 4); std::vector<int32_t> pn(n), pi((size_t)n * SD_MAXB);
        for (int k = 0; k < n; k++) {
            const int l = sepLane[k];
            memcpy(&pb[(size_t)k * SD_MAXB * 4], &t->hBoxes[(size_t)l * SD_MAXB * 4], SD_MAXB * 32);
            memcpy(&pi[(size_t)k * SD_MAXB], &t->hIdx[(size_t)l * SD_MAXB], SD_MAXB * 4);
            pn[k] = t->hNb[l];
        }
        TRK(sd_batch_first_separate(b, n, t->hSlots.data(), pb.data(), pn.data(), pi.data(), s));
    }
    if (!sepLane.empty()) TRK(sd_batch_undistort(b, S, curSlots.data(), s));      // firstSeparate permuted mvKeys: mvKeysUn / mvdynKeysUn follow
    TRK(assign_grid_impl(b, S, ipl, cam, s));

    // ---- per-pair result state of this step
    HIPCHK(hipMemsetAsync(b->d_moRes, 0, (size_t)S * sizeof(SdMotionResult), s));
    HIPCHK(hipMemsetAsync(b->d_sepRet, 0, (size_t)S * 4, s));
    HIPCHK(hipMemsetAsync(b->d_dynStart, 0, (size_t)S * (SD_MAXB + 1) * 4, s));
    HIPCHK(hipMemsetAsync(b->d_nmatch, 0, (size_t)2 * S * 4, s));
    HIPCHK(hipMemsetAsync(b->d_npairs, 0, (size_t)2 * S * 4, s));
    b->dlPairs = 2 * S; b->nMotion = S; b->nSepPairs = S; b->nPairs = S;

    // ---- Track_new's dynamic block, first round: every lane whose queue offers a reference frame (gated on the device by
    // `!mCurrentFrame.objects.empty()`); mState == OK && !mVelocity.empty() from the lane's third frame on
    t->hCur.assign(S, 0); t->hRef.assign(S, 0); t->hLast.assign(S, 0); t->hWant.assign(S, 0);
    t->hTrw.assign((size_t)S * 16, 0.f);
    std::vector<int> candPos(S, -1);
    bool anyWant = false;
    for (int l = 0; l < S; l++) {
        sd_tracker::Lane& L = t->lanes[l];
        t->hCur[l] = t->hRef[l] = t->hLast[l] = l * ipl;          // valid slots for skipped pairs
        memcpy(&t->hTrw[(size_t)l * 16], &t->hI[0], 64);
        if (t->notInitialised(l) || t->hNb[l] == 0) continue;
        const int k = tracker_peek_candidate(L, timestamps[l], 0);
        candPos[l] = k;
        if (k < 0 || !t->canTrackHomo(l)) continue;               // TrackHomo returns 0 without a velocity model
        t->hWant[l] = 1; anyWant = true;
        t->hRef[l] = L.q[k].slot; t->hLast[l] = L.lastSlot;
        const std::vector<float>& P = t->poseOfSlot[L.q[k].slot];
        if (P.size() == 16) memcpy(&t->hTrw[(size_t)l * 16], P.data(), 64);
    }
    if (anyWant) TRK(tracker_dynamic_round(t, Tcw, s));

    // ---- the frame's map points (sharded batch mode: its own stereo points), UpdateFeaturesToGrid
    // (monocular: mvDepth is -1 everywhere, so the same kernel leaves "no point" flags and zeroed coordinates)
    TRK(sd_batch_unproject(b, 0, ipl, S, cam, Twc, s));
    if (anyWant) TRK(assign_grid_impl(b, S, ipl, cam, s));

    // ---- TrackWithMotionModel's matcher against mLastFrame (pairs [S, 2S))
    bool anyLast = false;
    t->poseRanStep = false;
    if (t->p.track_last) {
        t->hActiveLast.assign(S, 0);
        std::vector<int32_t> cur(S), last(S);
        t->hTlw.assign((size_t)S * 16, 0.f);
        for (int l = 0; l < S; l++) {
            sd_tracker::Lane& L = t->lanes[l];
            cur[l] = last[l] = l * ipl;
            memcpy(&t->hTlw[(size_t)l * 16], &t->hI[0], 64);
            if (L.lastSlot < 0) continue;
            t->hActiveLast[l] = 1; anyLast = true; last[l] = L.lastSlot;
            const std::vector<float>& P = t->poseOfSlot[L.lastSlot];
            if (P.size() == 16) memcpy(&t->hTlw[(size_t)l * 16], P.data(), 64);
        }
        if (anyLast) {
            HIPCHK(hipMemcpyAsync(t->d_activeLast, t->hActiveLast.data(), (size_t)S * 4, hipMemcpyHostToDevice, s));
            TRK(tracker_last_matcher(t, cur.data(), last.data(), Tcw, s));
        }
    }

    // ---- mLastFrame = Frame(mCurrentFrame); q_frame.push(mCurrentFrame): a free ring slot of the lane takes the copy
    std::vector<int32_t> src(S), dst(S);
    for (int l = 0; l < S; l++) {
        sd_tracker::Lane& L = t->lanes[l];
        if (L.freeSlots.empty()) return set_err(SD_ERR_STATE, "tracker ring exhausted");
        src[l] = l * ipl; dst[l] = L.freeSlots.back();
    }
    TRK(sd_batch_copy_frames(b, S, src.data(), dst.data(), s));
    TRK(tracker_summary(t, anyLast ? 1 : 0, s));                  // the one synchronisation of the step

    // ---- host replay of Track_new's queue logic with the flags the device produced; rare extra rounds
    std::vector<int> refSlotOut(S, -1), refIdOut(S, -1);
    for (int round = 0;; round++) {
        bool again = false;
        t->hWant.assign(S, 0);
        for (int l = 0; l < S; l++) {
            sd_tracker::Lane& L = t->lanes[l];
            const SdLaneSummary& U = t->h_sum[l];
            if (candPos[l] == -2) continue;                        // lane finished in an earlier round
            if (t->notInitialised(l) || U.nb == 0 || L.q.empty()) { candPos[l] = -2; continue; }      // Tracking.cc:599-622
            // destructive replay of the loop head: drop box-less fronts, stop at the first frame not older than 0.2 s
            int ref = -1;
            while (!L.q.empty() && timestamps[l] - L.q.front().t > 0.2f) {
                if (!L.q.front().hasBoxes) { L.freeSlots.push_back(L.q.front().slot); L.q.erase(L.q.begin()); continue; }
                ref = 0;
                break;
            }
            if (ref < 0) { candPos[l] = -2; continue; }
            const bool ran = round == 0 ? (t->canTrackHomo(l) && candPos[l] >= 0) : true;
            refSlotOut[l] = L.q.front().slot; refIdOut[l] = L.q.front().frameId;
            const int flag = ran ? U.flag : 0;
            if (flag != 0) { candPos[l] = -2; continue; }          // Separate / UpdateFrame ran on the device, `break`
            if (L.q.size() == 1) { candPos[l] = -2; continue; }    // Tracking.cc:657-658
            L.freeSlots.push_back(L.q.front().slot); L.q.erase(L.q.begin());
            // the loop continues with the next front: another round only if it is a candidate too
            const int k = tracker_peek_candidate(L, timestamps[l], 0);
            if (k < 0) {                                           // replay the remaining pops of box-less fronts, then done
                while (!L.q.empty() && timestamps[l] - L.q.front().t > 0.2f && !L.q.front().hasBoxes) { L.freeSlots.push_back(L.q.front().slot); L.q.erase(L.q.begin()); }
                candPos[l] = -2; continue;
            }
            if (!t->canTrackHomo(l)) { candPos[l] = k; again = true; continue; }      // TrackHomo keeps returning 0: replay only
            while (k > 0 && !L.q.front().hasBoxes) { L.freeSlots.push_back(L.q.front().slot); L.q.erase(L.q.begin()); }
            t->hWant[l] = 1; again = true; candPos[l] = 0;
            t->hRef[l] = L.q.front().slot; t->hLast[l] = L.lastSlot;
            const std::vector<float>& P = t->poseOfSlot[L.q.front().slot];
            memcpy(&t->hTrw[(size_t)l * 16], P.size() == 16 ? P.data() : &t->hI[0], 64);
        }
        if (!again) break;
        bool launch = false;
        for (int l = 0; l < S; l++) launch |= t->hWant[l] != 0;
        if (launch) {
            // the lanes of this round: their current frames still sit in the current slots (N == N_s: UpdateFrame did not run)
            TRK(tracker_dynamic_round(t, Tcw, s));
            TRK(sd_batch_unproject(b, 0, ipl, S, cam, Twc, s));
            TRK(assign_grid_impl(b, S, ipl, cam, s));
            if (anyLast) {
                std::vector<int32_t> cur(S), last(S);
                for (int l = 0; l < S; l++) { cur[l] = l * ipl; last[l] = t->hActiveLast[l] ? t->lanes[l].lastSlot : l * ipl; }
                TRK(tracker_last_matcher(t, cur.data(), last.data(), Tcw, s));
            }
            TRK(sd_batch_copy_frames(b, S, src.data(), dst.data(), s));
            TRK(tracker_summary(t, anyLast ? 1 : 0, s));
        }
    }

    // ---- end of Track_new: `if(q_frame.size() >= mMaxFrames * 0.3) q_frame.pop(); q_frame.push(mCurrentFrame)`; mLastFrame
    for (int l = 0; l < S; l++) {
        sd_tracker::Lane& L = t->lanes[l];
        const SdLaneSummary& U = t->h_sum[l];
        if (t->notInitialised(l)) { for (auto& e : L.q) L.freeSlots.push_back(e.slot); L.q.clear(); }   // NOT_INITIALIZED: the queue is emptied (Tracking.cc:600-605)
        if ((double)L.q.size() >= (double)t->p.fps * 0.3 && !L.q.empty()) { L.freeSlots.push_back(L.q.front().slot); L.q.erase(L.q.begin()); }
        // take dst[l] out of the free list (a pop above may have pushed other slots on top of it)
        for (size_t k = 0; k < L.freeSlots.size(); k++) if (L.freeSlots[k] == dst[l]) { L.freeSlots.erase(L.freeSlots.begin() + k); break; }
        L.q.push_back({timestamps[l], dst[l], U.nb > 0 ? 1 : 0, L.frameNo});
        L.lastSlot = dst[l];
        t->poseOfSlot[dst[l]].assign(Tcw + (size_t)l * 16, Tcw + (size_t)l * 16 + 16);
        // mLastFrame's box members for the next boxTrack: the boxes that survived the empty-box erase
        L.nLast = U.nb;
        for (int j = 0; j < U.nb; j++) {
            const int o = U.keptOrig[j];
            for (int k = 0; k < 4; k++) L.lastObjects[j][k] = U.boxes[j][k];
            L.lastIdx[j] = U.box_idx[j];
            L.lastOmit[j] = t->hOmit[(size_t)l * SD_MAXB + o];
            L.lastVel[j][0] = t->hVel[((size_t)l * SD_MAXB + o) * 2]; L.lastVel[j][1] = t->hVel[((size_t)l * SD_MAXB + o) * 2 + 1];
        }
        if (t->poseOpt) {                                          // TrackWithMotionModel's tail (defaults when no matcher ran)
            sd_pose_result& P = t->poseRes[l];
            memset(&P, 0, sizeof(P));
            P.n_matches = -1;
            memcpy(P.Tcw, Tcw + (size_t)l * 16, 64);
            if (t->poseRanStep) {
                const SdPoseSummary& Q = ((const SdPoseSummary*)(t->h_sum + S))[l];
                memcpy(P.Tcw, Q.Tcw, 64);
                P.ran = Q.ran; P.n_matches = Q.nMatches; P.n_initial = Q.nInitial; P.n_good = Q.nGood; P.n_matches_map = Q.nMap; P.ok = Q.ok;
            }
        }
        if (results) {
            sd_lane_result& Rr = results[l];
            memset(&Rr, 0, sizeof(Rr));
            Rr.frame_id = L.frameNo; Rr.cur_slot = l * ipl; Rr.last_slot = dst[l];
            Rr.ref_slot = refSlotOut[l]; Rr.ref_frame_id = refIdOut[l];
            Rr.track_flag = U.flag; Rr.separate_ret = U.sepRet; Rr.n_track_matches = U.nTrackMatches; Rr.n_track_pairs = U.nTrackPairs;
            Rr.n_h = U.nH; Rr.n_f = U.nF; Rr.n_last_matches = U.nLastMatches;
            Rr.N = U.N; Rr.N_s = U.nOri; Rr.N_d = U.nDyn; Rr.n_boxes = U.nb;
            for (int j = 0; j < U.nb; j++) {
                Rr.box_idx[j] = U.box_idx[j]; Rr.box_status[j] = U.box_status[j]; Rr.omit[j] = L.lastOmit[j];
                for (int k = 0; k < 4; k++) Rr.objects[j][k] = U.boxes[j][k];
                Rr.box_velocity[j][0] = L.lastVel[j][0]; Rr.box_velocity[j][1] = L.lastVel[j][1];
            }
        }
        L.frameNo++;
    }
    return SD_OK;
}

int sd_tracker_set_pose_optimization(sd_tracker* t, int enable)
{
    if (!t) return set_err(SD_ERR_INVALID, "null tracker");
    if (enable && !t->p.track_last) return set_err(SD_ERR_STATE, "pose optimisation needs track_last");
    if (enable) {                                              // the pose buffers now, not inside the first step
        int rc = ensure_pose(t->b.get());
        if (rc != SD_OK) return rc;
    }
    t->poseOpt = enable != 0;
    t->poseRes.assign(t->poseOpt ? t->S : 0, sd_pose_result());
    return SD_OK;
}

int sd_tracker_pose_results(sd_tracker* t, sd_pose_result* results)
{
    if (!t || !results) return set_err(SD_ERR_INVALID, "bad pose_results arguments");
    if (!t->poseOpt) return set_err(SD_ERR_STATE, "pose optimisation is off");
    memcpy(results, t->poseRes.data(), (size_t)t->S * sizeof(sd_pose_result));
    return SD_OK;
}

int sd_tracker_track_host(sd_tracker* t, const uint8_t* const* images, size_t stride, const void* const* depth,
                          size_t depth_stride_elems, const double* boxes, const int32_t* n_boxes, const double* timestamps,
                          const float* Tcw, const float* Twc, sd_lane_result* results)
{
    if (!t || !images || !timestamps) return set_err(SD_ERR_INVALID, "bad track_host arguments");
    const int W = t->p.width, H = t->p.height, ch = t->p.channels;
    const size_t row = (size_t)W * ch, img = row * H;
    if (stride < row) return set_err(SD_ERR_INVALID, "stride smaller than a row");
    hipStream_t s = t->b->stream;
    if (!t->d_hostImg) HIPCHK(t->d_hostImg.alloc(img * t->nCur));
    for (int i = 0; i < t->nCur; i++) {
        if (!images[i]) return set_err(SD_ERR_INVALID, "null image");
        HIPCHK(hipMemcpy2DAsync(t->d_hostImg + img * i, row, images[i], stride, row, H, hipMemcpyHostToDevice, s));
    }
    if (t->p.sensor == SD_SENSOR_RGBD) {
        if (!depth || depth_stride_elems < (size_t)W) return set_err(SD_ERR_INVALID, "RGB-D tracking needs depth images");
        const size_t eb = t->p.depth_type == SD_DEPTH_F32 ? 4 : 2;
        if (!t->d_hostDepth) HIPCHK(t->d_hostDepth.alloc((size_t)W * H * eb * t->S));
        for (int l = 0; l < t->S; l++) {
            if (!depth[l]) return set_err(SD_ERR_INVALID, "null depth image");
            HIPCHK(hipMemcpy2DAsync((char*)t->d_hostDepth.get() + (size_t)W * H * eb * l, (size_t)W * eb, depth[l], depth_stride_elems * eb, (size_t)W * eb, H, hipMemcpyHostToDevice, s));
        }
    }
    return sd_tracker_track(t, t->d_hostImg, row, img, t->d_hostDepth, (size_t)W, (size_t)W * H, boxes, n_boxes, timestamps, Tcw, Twc, results, s);
}
#undef TRK
