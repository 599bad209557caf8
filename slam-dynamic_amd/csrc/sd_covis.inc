// sd_covis: the device mirror of the map's covisibility graph (include/sd_frontend.h, kernels in k_covis.h, DESIGN.md Q43).  Included by
// sd_api.hip inside its extern "C" block, after sd_kfdb.inc.  Reference: src/KeyFrame.cc:123-208, 289-379, 553-567.  The host keeps what it
// decides and what it must check before a launch: offsets, live and protected flags, and the match table of every keyframe (two features of
// one keyframe must not name one point).  Rows, ordered lists, parents and the first-connection flags are the device's.

static_assert(sizeof(sd_covis_cull_result) == sizeof(SdCovisCull) && sizeof(sd_covis_local_info) == sizeof(SdCovisLocal), "covis records");
static_assert(SD_COVIS_MAX_KF == SD_COVIS_MAX_KEYFRAMES && sizeof(sd_covis_keyframe_info) == 36, "covis header");
#define SD_COVIS_STAGE 65536                   // items of one upload of a mutation list; longer lists go in several

struct sd_covis {
    int maxKf = 0, maxFeat = 0, maxPoints = 0, maxJobs = 0, maxLocal = 0, seenWords = 0;
    int lastCull = -1, lastLocal = -1;         // candidates / queries of the last culling / local-map call
    std::vector<SdCovisKf> h;                  // off, n (a batch slot's capacity), live, prot
    std::vector<int> hMp;                      // [maxFeat] the match tables as the host calls left them
    int poolUsed = 0, kfHigh = 0, mpHigh = 0;  // 1 + the largest keyframe / point id named since the last clear
    bool dirty = true;                         // the tables changed since the inverse index was built
    bool mirror = true;                        // hMp is what the device holds: false once matches came from device arrays
    SdDevBuf<int> d_err;                       // [0] a device-array item was out of range, [1] a keyframe names a point twice
    hipStream_t lastStream = nullptr;
    hipEvent_t order = nullptr;
    SdDevBuf<SdCovisKf> d_kf; SdDevBuf<int> d_mp, d_owner, d_obs, d_start, d_cur, d_bsum, d_row, d_ordId, d_ordW, d_cnt, d_list, d_stage;
    SdDevBuf<unsigned char> d_oct, d_st, d_bad; SdDevBuf<float> d_depth; SdDevBuf<SdCovisJob> d_job;
    SdDevBuf<SdCovisCull> d_cull; SdDevBuf<SdCovisQ> d_q; SdDevBuf<int> d_lkf, d_lpt; SdDevBuf<unsigned> d_seen; SdDevBuf<SdCovisLocal> d_linfo;
    std::vector<int> hStage; std::vector<SdCovisQ> hQ;
    ~sd_covis() { if (order) (void)hipEventDestroy(order); }
};

static SdCovisArgs covis_args(sd_covis* cv)
{
    SdCovisArgs A;
    A.kf = cv->d_kf; A.mp = cv->d_mp; A.owner = cv->d_owner; A.oct = cv->d_oct; A.st = cv->d_st; A.depth = cv->d_depth; A.bad = cv->d_bad;
    A.start = cv->d_start; A.cur = cv->d_cur; A.obs = cv->d_obs; A.bsum = cv->d_bsum; A.row = cv->d_row; A.ordId = cv->d_ordId; A.ordW = cv->d_ordW;
    A.cnt = cv->d_cnt; A.job = cv->d_job; A.list = cv->d_list;
    A.K = cv->kfHigh; A.stride = cv->maxKf; A.P = cv->mpHigh; A.poolUsed = cv->poolUsed;
    A.n2 = 2;
    while (A.n2 < cv->kfHigh) A.n2 <<= 1;
    return A;
}

int sd_covis_create(sd_covis** out, int max_keyframes, int max_features, int max_points, int max_jobs, int max_local_points)
{
    if (!out) return set_err(SD_ERR_INVALID, "null argument");
    *out = nullptr;
    if (max_keyframes < 1 || max_keyframes > SD_COVIS_MAX_KEYFRAMES || max_features < 1 || max_points < 1 || max_jobs < 1 || max_jobs > 65535 || max_local_points < 1 ||
        (size_t)max_jobs * (size_t)max_local_points > ((size_t)1 << 30))
        return set_err(SD_ERR_INVALID, "covis_create: sizes outside [1, ..], more than 8192 keyframes, more than 65535 jobs or more than 2^30 (job, local point) cells");
    int rc = require_device();
    if (rc != SD_OK) return rc;
    std::unique_ptr<sd_covis> cv(new sd_covis());
    cv->maxKf = max_keyframes; cv->maxFeat = max_features; cv->maxPoints = max_points; cv->maxJobs = max_jobs; cv->maxLocal = max_local_points; cv->seenWords = max_points / 32 + 1;
    const size_t K = (size_t)max_keyframes, F = (size_t)max_features, P = (size_t)max_points;
    HIPCHK(cv->d_kf.alloc(K * sizeof(SdCovisKf)));
    HIPCHK(cv->d_mp.alloc(F * 4)); HIPCHK(cv->d_owner.alloc(F * 4)); HIPCHK(cv->d_obs.alloc(F * 4)); HIPCHK(cv->d_oct.alloc(F)); HIPCHK(cv->d_st.alloc(F)); HIPCHK(cv->d_depth.alloc(F * 4));
    HIPCHK(cv->d_bad.alloc(P)); HIPCHK(cv->d_start.alloc((P + 1) * 4)); HIPCHK(cv->d_cur.alloc(P * 4)); HIPCHK(cv->d_bsum.alloc((P / SD_COVIS_SCAN + 2) * 4));
    HIPCHK(cv->d_row.alloc(K * K * 4)); HIPCHK(cv->d_ordId.alloc(K * K * 4)); HIPCHK(cv->d_ordW.alloc(K * K * 4));
    HIPCHK(cv->d_cnt.alloc((size_t)max_jobs * K * 4)); HIPCHK(cv->d_job.alloc((size_t)max_jobs * sizeof(SdCovisJob))); HIPCHK(cv->d_list.alloc((size_t)max_jobs * 4));
    HIPCHK(cv->d_cull.alloc((size_t)max_jobs * sizeof(SdCovisCull))); HIPCHK(cv->d_q.alloc((size_t)max_jobs * sizeof(SdCovisQ))); HIPCHK(cv->d_lkf.alloc((size_t)max_jobs * K * 4));
    HIPCHK(cv->d_lpt.alloc((size_t)max_jobs * max_local_points * 4)); HIPCHK(cv->d_seen.alloc((size_t)max_jobs * cv->seenWords * 4)); HIPCHK(cv->d_linfo.alloc((size_t)max_jobs * sizeof(SdCovisLocal)));
    HIPCHK(cv->d_err.alloc(8)); HIPCHK(hipMemset(cv->d_err, 0, 8));
    HIPCHK(cv->d_stage.alloc((size_t)SD_COVIS_STAGE * 3 * 4));
    HIPCHK(hipMemset(cv->d_kf, 0, K * sizeof(SdCovisKf))); HIPCHK(hipMemset(cv->d_row, 0, K * K * 4)); HIPCHK(hipMemset(cv->d_bad, 0, P));
    HIPCHK(hipEventCreateWithFlags(&cv->order, hipEventDisableTiming));
    cv->h.assign(K, SdCovisKf()); cv->hMp.assign(F, -1);
    *out = cv.release();
    return SD_OK;
}

int sd_covis_destroy(sd_covis* cv)
{
    if (cv) (void)hipStreamSynchronize(cv->lastStream);
    delete cv;
    return SD_OK;
}

static int covis_stream(sd_covis* cv, void* stream_, hipStream_t fallback, hipStream_t& s)
{
    s = stream_ ? (hipStream_t)stream_ : fallback;
    if (s != cv->lastStream) {
        HIPCHK(hipEventRecord(cv->order, cv->lastStream));
        HIPCHK(hipStreamWaitEvent(s, cv->order, 0));
        cv->lastStream = s;
    }
    return SD_OK;
}

int sd_covis_clear(sd_covis* cv)
{
    if (!cv) return SD_ERR_INVALID;
    hipStream_t s = cv->lastStream;
    if (cv->kfHigh > 0) {
        HIPCHK(hipMemsetAsync(cv->d_kf, 0, (size_t)cv->kfHigh * sizeof(SdCovisKf), s));
        HIPCHK(hipMemsetAsync(cv->d_row, 0, (size_t)cv->kfHigh * cv->maxKf * 4, s));
    }
    if (cv->mpHigh > 0) HIPCHK(hipMemsetAsync(cv->d_bad, 0, (size_t)cv->mpHigh, s));
    std::fill(cv->h.begin(), cv->h.begin() + cv->kfHigh, SdCovisKf());
    std::fill(cv->hMp.begin(), cv->hMp.begin() + cv->poolUsed, -1);
    if (!cv->mirror) HIPCHK(hipMemsetAsync(cv->d_err, 0, 8, s));
    cv->poolUsed = 0; cv->kfHigh = 0; cv->mpHigh = 0; cv->dirty = true; cv->mirror = true; cv->lastCull = cv->lastLocal = -1;
    return SD_OK;
}

// the checks and the host half of an add: `reserve` pool features for keyframe kf_id
static int covis_new_kf(sd_covis* cv, int kf_id, int reserve, int prot, const char* who)
{
    if (kf_id < 0 || kf_id >= cv->maxKf) return set_err(SD_ERR_INVALID, std::string(who) + ": kf_id outside [0, max_keyframes)");
    SdCovisKf& E = cv->h[kf_id];
    if (E.live) return set_err(SD_ERR_STATE, std::string(who) + ": keyframe " + std::to_string(kf_id) + " is already in the graph");
    if ((long long)cv->poolUsed + reserve > cv->maxFeat) return set_err(SD_ERR_CAPACITY, std::string(who) + ": the feature pool is full (erased keyframes are reclaimed by clear only)");
    E = SdCovisKf();
    E.off = cv->poolUsed; E.n = reserve; E.live = 1; E.prot = prot ? 1 : 0; E.parent = -1; E.first = 1;
    cv->poolUsed += reserve;
    cv->kfHigh = std::max(cv->kfHigh, kf_id + 1);
    cv->dirty = true;
    return SD_OK;
}

int sd_covis_add_from_batch(sd_covis* cv, sd_batch* b, int n, const int32_t* image_index, const int32_t* kf_id, const uint8_t* is_protected, void* stream_)
{
    if (!cv || !b || n < 0 || (n > 0 && (!image_index || !kf_id))) return set_err(SD_ERR_INVALID, "bad covis_add_from_batch arguments");
    const int cap = b->plan.kpCap;
    for (int i = 0; i < n; i++) {
        if (image_index[i] < 0 || image_index[i] >= b->maxImages || kf_id[i] < 0 || kf_id[i] >= cv->maxKf)
            return set_err(SD_ERR_INVALID, "covis_add_from_batch: slot or kf_id out of range");
        if (!b->slotValid[image_index[i]]) return set_err(SD_ERR_STATE, "covis_add_from_batch: the slot holds no frame");
        if (cv->h[kf_id[i]].live) return set_err(SD_ERR_STATE, "covis_add_from_batch: keyframe " + std::to_string(kf_id[i]) + " is already in the graph");
        for (int j = 0; j < i; j++) if (kf_id[j] == kf_id[i]) return set_err(SD_ERR_STATE, "covis_add_from_batch: a kf_id is listed twice");
    }
    if ((long long)cv->poolUsed + (long long)n * cap > cv->maxFeat) return set_err(SD_ERR_CAPACITY, "covis_add_from_batch: the feature pool is full (erased keyframes are reclaimed by clear only)");
    hipStream_t s;
    int rc = covis_stream(cv, stream_, b->lastStream, s);
    if (rc != SD_OK) return rc;
    for (int i = 0; i < n; i++) {
        rc = covis_new_kf(cv, kf_id[i], cap, is_protected ? is_protected[i] : 0, "covis_add_from_batch");
        if (rc != SD_OK) return rc;
        HIPCHK(hipMemcpyAsync(cv->d_kf + kf_id[i], &cv->h[kf_id[i]], sizeof(SdCovisKf), hipMemcpyHostToDevice, s));
        const size_t off = (size_t)image_index[i] * cap;
        hipLaunchKernelGGL(k_covis_add_batch, dim3((cap + 255) / 256), dim3(256), 0, s, covis_args(cv), kf_id[i], b->d_kp + off, b->d_uright + off, b->d_depth + off,
                           b->d_count + image_index[i], cap);
        LAUNCH_CHECK("k_covis_add_batch");
    }
    return SD_OK;
}

int sd_covis_add_host(sd_covis* cv, int kf_id, int n_features, const uint8_t* octave, const float* uright, const float* depth, int is_protected)
{
    if (!cv || n_features < 0 || (n_features > 0 && (!octave || !uright || !depth))) return set_err(SD_ERR_INVALID, "bad covis_add_host arguments");
    int rc = covis_new_kf(cv, kf_id, n_features, is_protected, "covis_add_host");
    if (rc != SD_OK) return rc;
    const SdCovisKf& E = cv->h[kf_id];
    hipStream_t s = cv->lastStream;
    if (n_features) {
        std::vector<int> own((size_t)n_features, kf_id), none((size_t)n_features, -1);
        std::vector<unsigned char> st((size_t)n_features);
        for (int i = 0; i < n_features; i++) st[i] = uright[i] >= 0.0f ? 1 : 0;
        HIPCHK(hipMemcpyAsync(cv->d_owner + E.off, own.data(), (size_t)n_features * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(cv->d_mp + E.off, none.data(), (size_t)n_features * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(cv->d_st + E.off, st.data(), (size_t)n_features, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(cv->d_oct + E.off, octave, (size_t)n_features, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(cv->d_depth + E.off, depth, (size_t)n_features * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                       // the staging vectors above end with this call
    }
    HIPCHK(hipMemcpyAsync(cv->d_kf + kf_id, &E, sizeof(SdCovisKf), hipMemcpyHostToDevice, s));
    return SD_OK;
}

// uploads `cols` columns of n ints (hStage: column c at [c * n, (c + 1) * n)) in pieces of SD_COVIS_STAGE and runs `launch(d0, d1, d2, m)` on each
extern "C++" {
template <typename F>
static int covis_staged(sd_covis* cv, int n, int cols, F launch)
{
    hipStream_t s = cv->lastStream;
    for (int base = 0; base < n; base += SD_COVIS_STAGE) {
        const int m = std::min(n - base, SD_COVIS_STAGE);
        for (int c = 0; c < cols; c++)
            HIPCHK(hipMemcpyAsync(cv->d_stage + (size_t)c * SD_COVIS_STAGE, cv->hStage.data() + (size_t)c * n + base, (size_t)m * 4, hipMemcpyHostToDevice, s));
        launch(cv->d_stage.get(), cv->d_stage + SD_COVIS_STAGE, cv->d_stage + 2 * SD_COVIS_STAGE, m, s);
        LAUNCH_CHECK("covis mutation");
    }
    return SD_OK;
}
}

int sd_covis_set_matches(sd_covis* cv, int n, const int32_t* kf_id, const int32_t* idx, const int32_t* mp_id)
{
    if (!cv || n < 0 || (n > 0 && (!kf_id || !idx || !mp_id))) return set_err(SD_ERR_INVALID, "bad covis_set_matches arguments");
    for (int i = 0; i < n; i++) {
        if (kf_id[i] < 0 || kf_id[i] >= cv->maxKf || mp_id[i] < -1 || mp_id[i] >= cv->maxPoints)
            return set_err(SD_ERR_INVALID, "covis_set_matches: kf_id outside [0, max_keyframes) or mp_id outside [-1, max_points)");
        const SdCovisKf& E = cv->h[kf_id[i]];
        if (!E.live) return set_err(SD_ERR_STATE, "covis_set_matches: keyframe " + std::to_string(kf_id[i]) + " is not in the graph");
        if (idx[i] < 0 || idx[i] >= E.n) return set_err(SD_ERR_INVALID, "covis_set_matches: feature index outside the keyframe");
    }
    // the list in order on the host's tables; then no keyframe it touched may name a point twice
    std::vector<std::pair<int, int>> undo;                       // (slot, value before the call), first touch only
    std::vector<int> slotKf;
    std::map<int, int> seen;
    for (int i = 0; i < n; i++) {
        const int slot = cv->h[kf_id[i]].off + idx[i];
        if (seen.emplace(slot, (int)undo.size()).second) { undo.push_back({slot, cv->hMp[slot]}); slotKf.push_back(kf_id[i]); }
        cv->hMp[slot] = mp_id[i];
    }
    std::vector<int> touched(slotKf);
    std::sort(touched.begin(), touched.end());
    touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
    for (int k : touched) {
        if (!cv->mirror) break;                                  // the device checks instead (k_covis_csr_check)
        const SdCovisKf& E = cv->h[k];
        std::vector<int> pts;
        for (int i = 0; i < E.n; i++) if (cv->hMp[E.off + i] >= 0) pts.push_back(cv->hMp[E.off + i]);
        std::sort(pts.begin(), pts.end());
        if (std::adjacent_find(pts.begin(), pts.end()) != pts.end()) {
            for (auto& u : undo) cv->hMp[u.first] = u.second;
            return set_err(SD_ERR_INVALID, "covis_set_matches: two features of keyframe " + std::to_string(k) + " would name one map point");
        }
    }
    const int m = (int)undo.size();
    cv->hStage.resize((size_t)m * 3);
    for (int i = 0; i < m; i++) {
        const int slot = undo[i].first, v = cv->hMp[slot];
        cv->hStage[i] = slotKf[i]; cv->hStage[(size_t)m + i] = slot - cv->h[slotKf[i]].off; cv->hStage[(size_t)2 * m + i] = v;
        cv->mpHigh = std::max(cv->mpHigh, v + 1);
    }
    cv->dirty = true;
    const SdCovisArgs A = covis_args(cv);
    return covis_staged(cv, m, 3, [&](int* a, int* b, int* c, int cnt, hipStream_t s) {
        hipLaunchKernelGGL(k_covis_set_matches, dim3((cnt + 255) / 256), dim3(256), 0, s, A, a, b, c, cnt);
    });
}

int sd_covis_set_matches_device(sd_covis* cv, int n, const int32_t* d_kf_id, const int32_t* d_idx, const int32_t* d_mp_id, void* stream_)
{
    if (!cv || n < 0 || (n > 0 && (!d_kf_id || !d_idx || !d_mp_id))) return set_err(SD_ERR_INVALID, "bad covis_set_matches_device arguments");
    hipStream_t s;
    int rc = covis_stream(cv, stream_, cv->lastStream, s);
    if (rc != SD_OK || n == 0) return rc;
    // the host no longer knows the tables: every point id may be in use, and the duplicate check moves to the device
    cv->mirror = false; cv->mpHigh = cv->maxPoints; cv->dirty = true;
    hipLaunchKernelGGL(k_covis_set_matches_dev, dim3((n + 255) / 256), dim3(256), 0, s, covis_args(cv), d_kf_id, d_idx, d_mp_id, n, cv->maxPoints, cv->d_err.get());
    LAUNCH_CHECK("k_covis_set_matches_dev");
    return SD_OK;
}

// what the device found in device-array matches, for a download that has synchronised
static int covis_device_errors(sd_covis* cv, const char* who)
{
    if (cv->mirror) return SD_OK;
    int e[2] = {0, 0};
    HIPCHK(hipMemcpy(e, cv->d_err, 8, hipMemcpyDeviceToHost));
    if (e[0]) {
        HIPCHK(hipMemset(cv->d_err, 0, 4));                      // reported once; the entries were left out
        return set_err(SD_ERR_INVALID, std::string(who) + ": a covis_set_matches_device item named no live keyframe, no feature of it or no possible point (it was ignored)");
    }
    if (e[1]) return set_err(SD_ERR_INVALID, std::string(who) + ": two features of one keyframe name one map point");
    return SD_OK;
}

// a list of (id, value) pairs with the last value of every id, into hStage's two columns
static int covis_last_wins(sd_covis* cv, int n, const int32_t* id, const int* val)
{
    std::map<int, int> last;
    for (int i = 0; i < n; i++) last[id[i]] = val[i];
    const int m = (int)last.size();
    cv->hStage.resize((size_t)m * 2);
    int i = 0;
    for (auto& kv : last) { cv->hStage[i] = kv.first; cv->hStage[(size_t)m + i] = kv.second; i++; }
    return m;
}

int sd_covis_set_point_bad(sd_covis* cv, int n, const int32_t* mp_id, const uint8_t* bad)
{
    if (!cv || n < 0 || (n > 0 && (!mp_id || !bad))) return set_err(SD_ERR_INVALID, "bad covis_set_point_bad arguments");
    std::vector<int> v((size_t)n);
    for (int i = 0; i < n; i++) {
        if (mp_id[i] < 0 || mp_id[i] >= cv->maxPoints) return set_err(SD_ERR_INVALID, "covis_set_point_bad: mp_id outside [0, max_points)");
        v[i] = bad[i];
    }
    const int m = covis_last_wins(cv, n, mp_id, v.data());
    for (int i = 0; i < m; i++)
        if (cv->hStage[i] >= cv->mpHigh) { cv->mpHigh = cv->hStage[i] + 1; cv->dirty = true; }      // the index by point covers [0, mpHigh)
    unsigned char* d_bad = cv->d_bad;
    return covis_staged(cv, m, 2, [&](int* a, int* b, int*, int cnt, hipStream_t s) {
        hipLaunchKernelGGL(k_covis_set_bad, dim3((cnt + 255) / 256), dim3(256), 0, s, d_bad, a, b, cnt);
    });
}

int sd_covis_set_parent(sd_covis* cv, int n, const int32_t* kf_id, const int32_t* parent_id)
{
    if (!cv || n < 0 || (n > 0 && (!kf_id || !parent_id))) return set_err(SD_ERR_INVALID, "bad covis_set_parent arguments");
    for (int i = 0; i < n; i++) {
        if (kf_id[i] < 0 || kf_id[i] >= cv->maxKf || parent_id[i] < -1 || parent_id[i] >= cv->maxKf)
            return set_err(SD_ERR_INVALID, "covis_set_parent: kf_id outside [0, max_keyframes) or parent outside [-1, max_keyframes)");
        if (!cv->h[kf_id[i]].live) return set_err(SD_ERR_STATE, "covis_set_parent: keyframe " + std::to_string(kf_id[i]) + " is not in the graph");
        if (parent_id[i] >= cv->kfHigh) return set_err(SD_ERR_STATE, "covis_set_parent: parent " + std::to_string(parent_id[i]) + " was never added");
    }
    const int m = covis_last_wins(cv, n, kf_id, parent_id);
    const SdCovisArgs A = covis_args(cv);
    return covis_staged(cv, m, 2, [&](int* a, int* b, int*, int cnt, hipStream_t s) {
        hipLaunchKernelGGL(k_covis_set_parent, dim3((cnt + 255) / 256), dim3(256), 0, s, A, a, b, cnt);
    });
}

int sd_covis_erase_keyframe(sd_covis* cv, int n, const int32_t* kf_id)
{
    if (!cv || n < 0 || (n > 0 && !kf_id)) return set_err(SD_ERR_INVALID, "bad covis_erase_keyframe arguments");
    for (int i = 0; i < n; i++)
        if (kf_id[i] < 0 || kf_id[i] >= cv->maxKf) return set_err(SD_ERR_INVALID, "covis_erase_keyframe: kf_id outside [0, max_keyframes)");
    hipStream_t s = cv->lastStream;
    for (int i = 0; i < n; i++) {
        SdCovisKf& E = cv->h[kf_id[i]];
        if (!E.live || E.prot) continue;                       // KeyFrame::SetBadFlag returns at once for mnId == 0
        const SdCovisArgs A = covis_args(cv);
        HIPCHK(sd_raise_lds_limit((const void*)k_covis_erase, (int)SD_COVIS_SORT_LDS(A.n2)));
        hipLaunchKernelGGL(k_covis_erase, dim3(A.K), dim3(256), SD_COVIS_SORT_LDS(A.n2), s, A, kf_id[i]);
        LAUNCH_CHECK("k_covis_erase");
        hipLaunchKernelGGL(k_covis_clear_kf, dim3(8), dim3(256), 0, s, A, kf_id[i]);
        LAUNCH_CHECK("k_covis_clear_kf");
        std::fill(cv->hMp.begin() + E.off, cv->hMp.begin() + E.off + E.n, -1);
        E.live = 0;
        cv->dirty = true;
    }
    return SD_OK;
}

// the CSR by map point, when a table changed since it was built
static int covis_index(sd_covis* cv, hipStream_t s)
{
    if (!cv->dirty) return SD_OK;
    const SdCovisArgs A = covis_args(cv);
    if (A.P > 0) {
        const int nb = (A.P + SD_COVIS_SCAN - 1) / SD_COVIS_SCAN;
        HIPCHK(hipMemsetAsync(cv->d_cur, 0, (size_t)A.P * 4, s));
        if (A.poolUsed > 0) { hipLaunchKernelGGL(k_covis_csr_count, dim3((A.poolUsed + 255) / 256), dim3(256), 0, s, A); LAUNCH_CHECK("k_covis_csr_count"); }
        hipLaunchKernelGGL(k_covis_scan_blocks, dim3(nb), dim3(SD_COVIS_SCAN), 0, s, A); LAUNCH_CHECK("k_covis_scan_blocks");
        hipLaunchKernelGGL(k_covis_scan_sums, dim3(1), dim3(SD_COVIS_SCAN), 0, s, A, nb); LAUNCH_CHECK("k_covis_scan_sums");
        hipLaunchKernelGGL(k_covis_scan_add, dim3(nb), dim3(SD_COVIS_SCAN), 0, s, A); LAUNCH_CHECK("k_covis_scan_add");
        if (A.poolUsed > 0) { hipLaunchKernelGGL(k_covis_csr_fill, dim3((A.poolUsed + 255) / 256), dim3(256), 0, s, A); LAUNCH_CHECK("k_covis_csr_fill"); }
        if (!cv->mirror) {
            HIPCHK(hipMemsetAsync(cv->d_err + 1, 0, 4, s));
            hipLaunchKernelGGL(k_covis_csr_check, dim3((A.P + 255) / 256), dim3(256), 0, s, A, cv->d_err.get()); LAUNCH_CHECK("k_covis_csr_check");
        }
    }
    cv->dirty = false;
    return SD_OK;
}

static int covis_check_list(sd_covis* cv, const char* who, int n, const int32_t* kf_id)
{
    if (!cv || n < 0 || (n > 0 && !kf_id)) return set_err(SD_ERR_INVALID, std::string(who) + ": null argument");
    if (n > cv->maxJobs) return set_err(SD_ERR_CAPACITY, std::string(who) + ": more keyframes than max_jobs");
    for (int i = 0; i < n; i++) {
        if (kf_id[i] < 0 || kf_id[i] >= cv->maxKf) return set_err(SD_ERR_INVALID, std::string(who) + ": kf_id outside [0, max_keyframes)");
        if (!cv->h[kf_id[i]].live) return set_err(SD_ERR_STATE, std::string(who) + ": keyframe " + std::to_string(kf_id[i]) + " is not in the graph");
    }
    return SD_OK;
}

int sd_covis_update_connections(sd_covis* cv, int n, const int32_t* kf_id, void* stream_)
{
    int rc = covis_check_list(cv, "covis_update_connections", n, kf_id);
    if (rc != SD_OK) return rc;
    hipStream_t s;
    rc = covis_stream(cv, stream_, cv->lastStream, s);
    if (rc != SD_OK || n == 0) return rc;
    rc = covis_index(cv, s);
    if (rc != SD_OK) return rc;
    cv->hStage.assign(kf_id, kf_id + n);
    HIPCHK(hipMemcpyAsync(cv->d_list, cv->hStage.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    const SdCovisArgs A = covis_args(cv);
    if (A.K <= SD_COVIS_LDS_KF) hipLaunchKernelGGL(k_covis_counter<true>, dim3(n), dim3(256), (size_t)A.K * 4, s, A);
    else hipLaunchKernelGGL(k_covis_counter<false>, dim3(n), dim3(256), 0, s, A);
    LAUNCH_CHECK("k_covis_counter");
    HIPCHK(sd_raise_lds_limit((const void*)k_covis_apply, (int)SD_COVIS_SORT_LDS(A.n2)));
    for (int j = 0; j < n; j++) {                              // the calls of one launch behave as if run in list order
        hipLaunchKernelGGL(k_covis_apply, dim3(A.K), dim3(256), SD_COVIS_SORT_LDS(A.n2), s, A, j);
        LAUNCH_CHECK("k_covis_apply");
    }
    return SD_OK;
}

int sd_covis_download_connections(sd_covis* cv, int kf_id, int best_n, int min_weight, int32_t* ordered_id, int32_t* ordered_weight, int cap_ordered,
                                  sd_covis_keyframe_info* info, int32_t* row_id, int32_t* row_weight, int cap_row)
{
    if (!cv || kf_id < 0 || kf_id >= cv->maxKf || !info) return set_err(SD_ERR_INVALID, "bad covis_download_connections arguments");
    HIPCHK(hipStreamSynchronize(cv->lastStream));
    int rc = covis_device_errors(cv, "covis_download_connections");
    if (rc != SD_OK) return rc;
    SdCovisKf E;
    HIPCHK(hipMemcpy(&E, cv->d_kf + kf_id, sizeof(E), hipMemcpyDeviceToHost));
    std::vector<int> oi((size_t)std::max(E.nOrd, 1)), ow((size_t)std::max(E.nOrd, 1)), row((size_t)std::max(cv->kfHigh, 1), 0);
    if (E.nOrd > 0) {
        HIPCHK(hipMemcpy(oi.data(), cv->d_ordId + (size_t)kf_id * cv->maxKf, (size_t)E.nOrd * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ow.data(), cv->d_ordW + (size_t)kf_id * cv->maxKf, (size_t)E.nOrd * 4, hipMemcpyDeviceToHost));
    }
    if (cv->kfHigh > 0) HIPCHK(hipMemcpy(row.data(), cv->d_row + (size_t)kf_id * cv->maxKf, (size_t)cv->kfHigh * 4, hipMemcpyDeviceToHost));
    int nRow = 0;
    for (int i = 0; i < cv->kfHigh; i++) nRow += row[i] != 0;
    info->live = E.live; info->n_features = E.n; info->is_protected = E.prot; info->parent = E.live ? E.parent : -1; info->first_connection = E.first;
    info->n_ordered = E.nOrd; info->n_row = nRow;
    info->n_best = std::min(E.nOrd, std::max(best_n, 0));      // GetBestCovisibilityKeyFrames(best_n)
    int nw = 0;                                                // GetCovisiblesByWeight(min_weight): the prefix up to upper_bound(.., w, a > b), and empty when that is the end
    while (nw < E.nOrd && !(min_weight > ow[nw])) nw++;
    info->n_by_weight = nw == E.nOrd ? 0 : nw;
    if ((ordered_id || ordered_weight) && E.nOrd > cap_ordered) return set_err(SD_ERR_CAPACITY, "covis_download_connections: ordered buffer too small");
    if ((row_id || row_weight) && nRow > cap_row) return set_err(SD_ERR_CAPACITY, "covis_download_connections: row buffer too small");
    for (int i = 0; i < E.nOrd; i++) { if (ordered_id) ordered_id[i] = oi[i]; if (ordered_weight) ordered_weight[i] = ow[i]; }
    for (int i = 0, j = 0; i < cv->kfHigh; i++)
        if (row[i] != 0) { if (row_id) row_id[j] = i; if (row_weight) row_weight[j] = row[i]; j++; }
    return SD_OK;
}

int sd_covis_keyframe_culling(sd_covis* cv, int n, const int32_t* cand_kf_id, const uint8_t* not_erase, int monocular, float th_depth, void* stream_)
{
    int rc = covis_check_list(cv, "covis_keyframe_culling", n, cand_kf_id);
    if (rc != SD_OK) return rc;
    std::vector<int> ids(cand_kf_id, cand_kf_id + n);
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return set_err(SD_ERR_INVALID, "covis_keyframe_culling: a candidate is listed twice");
    hipStream_t s;
    rc = covis_stream(cv, stream_, cv->lastStream, s);
    if (rc != SD_OK) return rc;
    cv->lastCull = n;
    if (n == 0) return SD_OK;
    rc = covis_index(cv, s);
    if (rc != SD_OK) return rc;
    cv->hStage.resize((size_t)2 * n);
    for (int i = 0; i < n; i++) { cv->hStage[i] = cand_kf_id[i]; cv->hStage[(size_t)n + i] = not_erase ? not_erase[i] != 0 : 0; }
    HIPCHK(hipMemcpyAsync(cv->d_list, cv->hStage.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(cv->d_stage, cv->hStage.data() + n, (size_t)n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_covis_culling, dim3(1), dim3(1024), 0, s, covis_args(cv), cv->d_stage.get(), n, monocular ? 1 : 0, th_depth, cv->d_cull.get());
    LAUNCH_CHECK("k_covis_culling");
    return SD_OK;
}

int sd_covis_download_culling(sd_covis* cv, sd_covis_cull_result* out, int cap, int* n)
{
    if (!cv) return SD_ERR_INVALID;
    if (cv->lastCull < 0) return set_err(SD_ERR_STATE, "covis_download_culling: no culling call has run");
    if (n) *n = cv->lastCull;
    if (!out) return SD_OK;
    if (cv->lastCull > cap) return set_err(SD_ERR_CAPACITY, "covis_download_culling: buffer too small");
    HIPCHK(hipStreamSynchronize(cv->lastStream));
    int rc = covis_device_errors(cv, "covis_download_culling");
    if (rc != SD_OK) return rc;
    if (cv->lastCull) HIPCHK(hipMemcpy(out, cv->d_cull, (size_t)cv->lastCull * sizeof(SdCovisCull), hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_covis_local_map(sd_covis* cv, int n_queries, const int32_t* point_offset, const int32_t* d_mp_id, uint8_t* d_entry_bad, void* stream_)
{
    if (!cv || n_queries < 0 || (n_queries > 0 && !point_offset)) return set_err(SD_ERR_INVALID, "covis_local_map: null argument");
    if (n_queries > cv->maxJobs) return set_err(SD_ERR_CAPACITY, "covis_local_map: more queries than max_jobs");
    cv->hQ.assign((size_t)n_queries, SdCovisQ());
    for (int q = 0; q < n_queries; q++) {
        const long long n = (long long)point_offset[q + 1] - point_offset[q];
        if (point_offset[q] < 0 || n < 0) return set_err(SD_ERR_INVALID, "covis_local_map: offsets must not be negative or decrease");
        cv->hQ[q].off = point_offset[q]; cv->hQ[q].n = (int)n;
    }
    if (n_queries > 0 && point_offset[n_queries] > 0 && !d_mp_id) return set_err(SD_ERR_INVALID, "covis_local_map: null point ids");
    hipStream_t s;
    int rc = covis_stream(cv, stream_, cv->lastStream, s);
    if (rc != SD_OK) return rc;
    cv->lastLocal = n_queries;
    if (n_queries == 0) return SD_OK;
    rc = covis_index(cv, s);
    if (rc != SD_OK) return rc;
    HIPCHK(hipMemcpyAsync(cv->d_q, cv->hQ.data(), (size_t)n_queries * sizeof(SdCovisQ), hipMemcpyHostToDevice, s));
    const SdCovisArgs A = covis_args(cv);
    const int seenWords = A.P / 32 + 1;                          // a row of seen bits per query, over the point ids in use
    HIPCHK(hipMemsetAsync(cv->d_seen, 0, (size_t)n_queries * seenWords * 4, s));
    if (A.K <= SD_COVIS_LDS_KF)
        hipLaunchKernelGGL(k_covis_local_map<true>, dim3(n_queries), dim3(1024), (size_t)std::max(A.K, 1) * 4, s, A, cv->d_q.get(), d_mp_id, d_entry_bad, cv->d_lkf.get(), cv->d_lpt.get(),
                           cv->d_seen.get(), seenWords, cv->maxLocal, cv->d_linfo.get());
    else
        hipLaunchKernelGGL(k_covis_local_map<false>, dim3(n_queries), dim3(1024), 0, s, A, cv->d_q.get(), d_mp_id, d_entry_bad, cv->d_lkf.get(), cv->d_lpt.get(),
                           cv->d_seen.get(), seenWords, cv->maxLocal, cv->d_linfo.get());
    LAUNCH_CHECK("k_covis_local_map");
    return SD_OK;
}

int sd_covis_local_map_host(sd_covis* cv, int n_queries, const int32_t* point_offset, const int32_t* mp_id, uint8_t* entry_bad)
{
    if (!cv || n_queries < 0 || (n_queries > 0 && !point_offset)) return set_err(SD_ERR_INVALID, "covis_local_map_host: null argument");
    const long long total = n_queries > 0 ? point_offset[n_queries] : 0;
    if (total < 0 || (total > 0 && !mp_id)) return set_err(SD_ERR_INVALID, "covis_local_map_host: null point ids");
    SdDevBuf<int> d_id; SdDevBuf<unsigned char> d_bad;
    HIPCHK(d_id.alloc(std::max<size_t>((size_t)total, 1) * 4)); HIPCHK(d_bad.alloc(std::max<size_t>((size_t)total, 1)));
    if (total) HIPCHK(hipMemcpy(d_id, mp_id, (size_t)total * 4, hipMemcpyHostToDevice));
    int rc = sd_covis_local_map(cv, n_queries, point_offset, d_id, d_bad, nullptr);
    hipError_t e = hipStreamSynchronize(cv->lastStream);                 // before the staging is freed, whatever the call returned
    if (rc != SD_OK) return rc;
    HIPCHK(e);
    if (total && entry_bad) HIPCHK(hipMemcpy(entry_bad, d_bad, (size_t)total, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_covis_download_local_map(sd_covis* cv, int query, sd_covis_local_info* info, int32_t* local_kf, int cap_kf, int32_t* local_point, int cap_points)
{
    if (!cv) return SD_ERR_INVALID;
    if (cv->lastLocal < 0) return set_err(SD_ERR_STATE, "covis_download_local_map: no local-map call has run");
    if (query < 0 || query >= cv->lastLocal) return set_err(SD_ERR_INVALID, "covis_download_local_map: query outside the last call");
    HIPCHK(hipStreamSynchronize(cv->lastStream));
    int rc = covis_device_errors(cv, "covis_download_local_map");
    if (rc != SD_OK) return rc;
    SdCovisLocal I;
    HIPCHK(hipMemcpy(&I, cv->d_linfo + query, sizeof(I), hipMemcpyDeviceToHost));
    if (info) memcpy(info, &I, sizeof(I));
    if (I.overflow) return set_err(SD_ERR_CAPACITY, "covis_download_local_map: the query has " + std::to_string(I.nPoints) + " local points, more than max_local_points");
    if ((local_kf && I.nKf > cap_kf) || (local_point && I.nPoints > cap_points)) return set_err(SD_ERR_CAPACITY, "covis_download_local_map: buffer too small");
    if (local_kf && I.nKf) HIPCHK(hipMemcpy(local_kf, cv->d_lkf + (size_t)query * cv->maxKf, (size_t)I.nKf * 4, hipMemcpyDeviceToHost));
    if (local_point && I.nPoints) HIPCHK(hipMemcpy(local_point, cv->d_lpt + (size_t)query * cv->maxLocal, (size_t)I.nPoints * 4, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_kfdb_set_covisible_from_covis(sd_kfdb* db, sd_covis* cv, int n, const int32_t* kf_id, void* stream_)
{
    if (!db) return set_err(SD_ERR_INVALID, "kfdb_set_covisible_from_covis: null database");
    int rc = covis_check_list(cv, "kfdb_set_covisible_from_covis", n, kf_id);
    if (rc != SD_OK) return rc;
    if (cv->kfHigh > db->maxKf) return set_err(SD_ERR_INVALID, "kfdb_set_covisible_from_covis: the graph holds keyframe ids beyond the database's max_keyframes (a neighbour could not be named)");
    for (int i = 0; i < n; i++) {
        if (kf_id[i] >= db->maxKf) return set_err(SD_ERR_INVALID, "kfdb_set_covisible_from_covis: kf_id outside the database's [0, max_keyframes)");
        if (!db->h[kf_id[i]].live) return set_err(SD_ERR_STATE, "kfdb_set_covisible_from_covis: keyframe " + std::to_string(kf_id[i]) + " is not in the database");
    }
    hipStream_t s, s2;
    rc = covis_stream(cv, stream_, cv->lastStream, s);
    if (rc != SD_OK) return rc;
    rc = kfdb_stream(db, s, s, s2);
    if (rc != SD_OK || n == 0) return rc;
    cv->hStage.assign(kf_id, kf_id + n);
    HIPCHK(hipMemcpyAsync(cv->d_list, cv->hStage.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_covis_to_kfdb, dim3(n), dim3(64), 0, s, covis_args(cv), db->d_entry.get(), n);
    LAUNCH_CHECK("k_covis_to_kfdb");
    return SD_OK;
}
