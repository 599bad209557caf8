// sd_kfdb: the device-resident KeyFrameDatabase (include/sd_frontend.h, kernels in k_kfdb.h, DESIGN.md Q42).  Included by sd_api.hip inside
// its extern "C" block.  Reference: src/KeyFrameDatabase.cc:33-309.  The host keeps a mirror of what it decides (offset, sequence number,
// live flag, neighbours); the device alone knows the length of an entry added from a batch slot and every mRelocScore.

static_assert(sizeof(SdKfdbEntry) == 64 && offsetof(SdKfdbEntry, count) == 56, "kfdb entry: the host owns the first 56 bytes");
static_assert(sizeof(sd_kfdb_query_info) == sizeof(SdKfdbInfo) && sizeof(sd_kfdb_member) == sizeof(SdKfdbMember) && sizeof(sd_kfdb_acc) == sizeof(SdKfdbAcc),
              "kfdb records");
static_assert(SD_KFDB_NEIGH == SD_KFDB_MAX_NEIGHBOURS, "kfdb neighbours");
#define SD_KFDB_HOST_BYTES 56

struct sd_kfdb {
    int maxKf = 0, maxPool = 0, maxQ = 0, maxQW = 0, sortStride = 1;
    std::vector<SdKfdbEntry> h;                // the host's part of the entry table (count = words reserved in the pool)
    int poolUsed = 0, idHigh = 0;              // idHigh: 1 + the largest id added since the last clear
    unsigned nextSeq = 0;
    int lastN = -1;                            // queries of the last detect call
    hipStream_t lastStream = nullptr;
    hipEvent_t order = nullptr;                // carries the call order over a change of stream
    SdDevBuf<SdKfdbEntry> d_entry; SdDevBuf<unsigned> d_poolW; SdDevBuf<double> d_poolV;
    // per-call work tables, [maxQ][maxKf] unless noted
    SdDevBuf<SdKfdbQ> d_q;                     // [maxQ]
    SdDevBuf<int> d_aux;                       // excluded ids / listed ids
    SdDevBuf<int> d_cnt, d_mark, d_sortKf, d_cand; SdDevBuf<unsigned> d_firstW; SdDevBuf<float> d_si; SdDevBuf<unsigned char> d_excl;
    SdDevBuf<unsigned long long> d_sortKey;    // [maxQ][sortStride]
    SdDevBuf<SdKfdbInfo> d_info; SdDevBuf<SdKfdbMember> d_member; SdDevBuf<SdKfdbAcc> d_acc;
    std::vector<SdKfdbQ> hQ; std::vector<int> hAux;        // host staging of the uploads
    size_t auxCap = 0;
    ~sd_kfdb() { if (order) (void)hipEventDestroy(order); }
};

int sd_kfdb_create(sd_kfdb** out, int max_keyframes, int max_pool_words, int max_queries, int max_query_words)
{
    if (!out) return set_err(SD_ERR_INVALID, "null argument");
    *out = nullptr;
    if (max_keyframes < 1 || max_pool_words < 1 || max_queries < 1 || max_queries > 65535 || max_query_words < 1 ||
        max_query_words > SD_KFDB_MAX_QUERY_WORDS || (size_t)max_keyframes * (size_t)max_queries > ((size_t)1 << 28))
        return set_err(SD_ERR_INVALID, "kfdb_create: sizes outside [1, ..], more than 65535 queries, more than 16384 query words or more than 2^28 (query, keyframe) cells");
    int rc = require_device();
    if (rc != SD_OK) return rc;
    std::unique_ptr<sd_kfdb> db(new sd_kfdb());
    db->maxKf = max_keyframes; db->maxPool = max_pool_words; db->maxQ = max_queries; db->maxQW = max_query_words;
    while (db->sortStride < max_keyframes) db->sortStride <<= 1;
    const size_t K = (size_t)max_keyframes, Q = (size_t)max_queries, cells = K * Q, sortCells = Q * (size_t)db->sortStride;
    db->auxCap = cells;
    HIPCHK(db->d_entry.alloc(K * sizeof(SdKfdbEntry))); HIPCHK(db->d_poolW.alloc((size_t)max_pool_words * 4)); HIPCHK(db->d_poolV.alloc((size_t)max_pool_words * 8));
    HIPCHK(db->d_q.alloc(Q * sizeof(SdKfdbQ))); HIPCHK(db->d_aux.alloc(db->auxCap * 4));
    HIPCHK(db->d_cnt.alloc(cells * 4)); HIPCHK(db->d_mark.alloc(cells * 4)); HIPCHK(db->d_cand.alloc(cells * 4)); HIPCHK(db->d_firstW.alloc(cells * 4));
    HIPCHK(db->d_si.alloc(cells * 4)); HIPCHK(db->d_excl.alloc(cells)); HIPCHK(db->d_sortKf.alloc(sortCells * 4)); HIPCHK(db->d_sortKey.alloc(sortCells * 8));
    HIPCHK(db->d_info.alloc(Q * sizeof(SdKfdbInfo))); HIPCHK(db->d_member.alloc(cells * sizeof(SdKfdbMember))); HIPCHK(db->d_acc.alloc(cells * sizeof(SdKfdbAcc)));
    HIPCHK(hipMemset(db->d_entry, 0, K * sizeof(SdKfdbEntry)));
    HIPCHK(hipEventCreateWithFlags(&db->order, hipEventDisableTiming));
    db->h.assign(K, SdKfdbEntry());
    *out = db.release();
    return SD_OK;
}

int sd_kfdb_destroy(sd_kfdb* db)
{
    if (db) (void)hipStreamSynchronize(db->lastStream);
    delete db;
    return SD_OK;
}

// the stream of this call; a call on another stream than the previous one waits on the device for it
static int kfdb_stream(sd_kfdb* db, void* stream_, hipStream_t fallback, hipStream_t& s)
{
    s = stream_ ? (hipStream_t)stream_ : fallback;
    if (s != db->lastStream) {
        HIPCHK(hipEventRecord(db->order, db->lastStream));
        HIPCHK(hipStreamWaitEvent(s, db->order, 0));
        db->lastStream = s;
    }
    return SD_OK;
}

int sd_kfdb_clear(sd_kfdb* db)
{
    if (!db) return SD_ERR_INVALID;
    if (db->idHigh > 0) HIPCHK(hipMemsetAsync(db->d_entry, 0, (size_t)db->idHigh * sizeof(SdKfdbEntry), db->lastStream));
    std::fill(db->h.begin(), db->h.begin() + db->idHigh, SdKfdbEntry());
    db->poolUsed = 0; db->idHigh = 0; db->nextSeq = 0;
    return SD_OK;
}

// the checks and the host half of KeyFrameDatabase::add: `reserve` pool words for a new entry of id kf_id
static int kfdb_new_entry(sd_kfdb* db, int kf_id, int reserve, const char* who)
{
    if (kf_id < 0 || kf_id >= db->maxKf) return set_err(SD_ERR_INVALID, std::string(who) + ": kf_id outside [0, max_keyframes)");
    SdKfdbEntry& E = db->h[kf_id];
    if (E.live) return set_err(SD_ERR_STATE, std::string(who) + ": keyframe " + std::to_string(kf_id) + " is already in the database");
    if ((long long)db->poolUsed + reserve > db->maxPool) return set_err(SD_ERR_CAPACITY, std::string(who) + ": the word pool is full (erased entries are reclaimed by clear only)");
    E = SdKfdbEntry();
    E.off = db->poolUsed; E.seq = db->nextSeq++; E.live = 1; E.count = reserve;
    db->poolUsed += reserve;
    db->idHigh = std::max(db->idHigh, kf_id + 1);
    return SD_OK;
}

int sd_kfdb_add_from_batch(sd_kfdb* db, sd_batch* b, int n, const int32_t* image_index, const int32_t* kf_id, void* stream_)
{
    if (!db || !b || n < 0 || (n > 0 && (!image_index || !kf_id))) return set_err(SD_ERR_INVALID, "bad kfdb_add_from_batch arguments");
    const int cap = b->plan.kpCap;
    for (int i = 0; i < n; i++) {
        if (image_index[i] < 0 || image_index[i] >= b->maxImages || kf_id[i] < 0 || kf_id[i] >= db->maxKf)
            return set_err(SD_ERR_INVALID, "kfdb_add_from_batch: slot or kf_id out of range");
        if (!b->d_bowWordF || !b->bowValid[image_index[i]]) return set_err(SD_ERR_STATE, "kfdb_add_from_batch: no bag of words computed for this slot");
        if (db->h[kf_id[i]].live) return set_err(SD_ERR_STATE, "kfdb_add_from_batch: keyframe " + std::to_string(kf_id[i]) + " is already in the database");
        for (int j = 0; j < i; j++) if (kf_id[j] == kf_id[i]) return set_err(SD_ERR_STATE, "kfdb_add_from_batch: a kf_id is listed twice");
    }
    // the length of a slot's BowVector is known to the device only: an entry reserves the slot's capacity
    if ((long long)db->poolUsed + (long long)n * cap > db->maxPool) return set_err(SD_ERR_CAPACITY, "kfdb_add_from_batch: the word pool is full (erased entries are reclaimed by clear only)");
    hipStream_t s;
    int rc = kfdb_stream(db, stream_, b->lastStream, s);
    if (rc != SD_OK) return rc;
    for (int i = 0; i < n; i++) {
        rc = kfdb_new_entry(db, kf_id[i], cap, "kfdb_add_from_batch");
        if (rc != SD_OK) return rc;
        SdKfdbEntry* dE = db->d_entry + kf_id[i];
        HIPCHK(hipMemcpyAsync(dE, &db->h[kf_id[i]], SD_KFDB_HOST_BYTES, hipMemcpyHostToDevice, s));
        const size_t off = (size_t)image_index[i] * cap;
        hipLaunchKernelGGL(k_kfdb_add_batch, dim3((cap + 255) / 256), dim3(256), 0, s, b->d_bowWord + off, b->d_bowVal + off, b->d_bowMeta + image_index[i] * 4, cap,
                           dE, db->d_poolW.get(), db->d_poolV.get());
        LAUNCH_CHECK("k_kfdb_add_batch");
    }
    return SD_OK;
}

int sd_kfdb_add_host(sd_kfdb* db, int kf_id, const uint32_t* bow_word, const double* bow_value, int n_words)
{
    if (!db || n_words < 0 || (n_words > 0 && (!bow_word || !bow_value))) return set_err(SD_ERR_INVALID, "bad kfdb_add_host arguments");
    for (int i = 1; i < n_words; i++)
        if (bow_word[i] <= bow_word[i - 1]) return set_err(SD_ERR_INVALID, "kfdb_add_host: word ids must be strictly ascending");
    int rc = kfdb_new_entry(db, kf_id, n_words, "kfdb_add_host");
    if (rc != SD_OK) return rc;
    const SdKfdbEntry& E = db->h[kf_id];
    hipStream_t s = db->lastStream;
    if (n_words) {
        HIPCHK(hipMemcpyAsync(db->d_poolW + E.off, bow_word, (size_t)n_words * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(db->d_poolV + E.off, bow_value, (size_t)n_words * 8, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(db->d_entry + kf_id, &E, sizeof(SdKfdbEntry), hipMemcpyHostToDevice, s));      // count = n_words, reloc = +0
    return SD_OK;
}

int sd_kfdb_erase(sd_kfdb* db, int n, const int32_t* kf_id)
{
    if (!db || n < 0 || (n > 0 && !kf_id)) return set_err(SD_ERR_INVALID, "bad kfdb_erase arguments");
    for (int i = 0; i < n; i++)
        if (kf_id[i] < 0 || kf_id[i] >= db->maxKf) return set_err(SD_ERR_INVALID, "kfdb_erase: kf_id outside [0, max_keyframes)");
    for (int i = 0; i < n; i++) {
        SdKfdbEntry& E = db->h[kf_id[i]];
        if (!E.live) continue;                               // erase of a keyframe that is not in the lists does nothing (KeyFrameDatabase.cc:58-65)
        E.live = 0;
        // off, seq, live only: the neighbour fields of the device entry may have been written by sd_kfdb_set_covisible_from_covis, which the mirror does not see
        HIPCHK(hipMemcpyAsync(db->d_entry + kf_id[i], &E, offsetof(SdKfdbEntry, nNeigh), hipMemcpyHostToDevice, db->lastStream));
    }
    return SD_OK;
}

int sd_kfdb_set_covisible(sd_kfdb* db, int n, const int32_t* kf_id, const int32_t* neigh, const int32_t* count)
{
    if (!db || n < 0 || (n > 0 && (!kf_id || !neigh || !count))) return set_err(SD_ERR_INVALID, "bad kfdb_set_covisible arguments");
    for (int i = 0; i < n; i++) {
        if (kf_id[i] < 0 || kf_id[i] >= db->maxKf) return set_err(SD_ERR_INVALID, "kfdb_set_covisible: kf_id outside [0, max_keyframes)");
        if (!db->h[kf_id[i]].live) return set_err(SD_ERR_STATE, "kfdb_set_covisible: keyframe " + std::to_string(kf_id[i]) + " is not in the database");
        if (count[i] < 0 || count[i] > SD_KFDB_NEIGH) return set_err(SD_ERR_INVALID, "kfdb_set_covisible: more than 10 neighbours");
        for (int j = 0; j < count[i]; j++)
            if (neigh[i * SD_KFDB_NEIGH + j] < 0 || neigh[i * SD_KFDB_NEIGH + j] >= db->maxKf) return set_err(SD_ERR_INVALID, "kfdb_set_covisible: neighbour id outside [0, max_keyframes)");
    }
    for (int i = 0; i < n; i++) {
        SdKfdbEntry& E = db->h[kf_id[i]];
        E.nNeigh = count[i];
        for (int j = 0; j < SD_KFDB_NEIGH; j++) E.neigh[j] = j < count[i] ? neigh[i * SD_KFDB_NEIGH + j] : 0;
        HIPCHK(hipMemcpyAsync(db->d_entry + kf_id[i], &E, SD_KFDB_HOST_BYTES, hipMemcpyHostToDevice, db->lastStream));
    }
    return SD_OK;
}

int sd_kfdb_download_entry(sd_kfdb* db, int kf_id, uint32_t* word, double* value, int cap_words, int* n_words, uint32_t* seq, int* live,
                           float* reloc_score, int32_t* neigh, int* n_neigh)
{
    if (!db || kf_id < 0 || kf_id >= db->maxKf) return set_err(SD_ERR_INVALID, "bad kfdb_download_entry arguments");
    HIPCHK(hipStreamSynchronize(db->lastStream));
    SdKfdbEntry E;
    HIPCHK(hipMemcpy(&E, db->d_entry + kf_id, sizeof(E), hipMemcpyDeviceToHost));
    if (n_words) *n_words = E.count;
    if (seq) *seq = E.seq;
    if (live) *live = E.live;
    if (reloc_score) *reloc_score = E.reloc;
    if (n_neigh) *n_neigh = E.nNeigh;
    if (neigh) for (int j = 0; j < SD_KFDB_NEIGH; j++) neigh[j] = j < E.nNeigh ? E.neigh[j] : -1;
    if ((word || value) && E.count > cap_words) return set_err(SD_ERR_CAPACITY, "kfdb_download_entry: buffer too small");
    if (E.count > 0) {
        if (word) HIPCHK(hipMemcpy(word, db->d_poolW + E.off, (size_t)E.count * 4, hipMemcpyDeviceToHost));
        if (value) HIPCHK(hipMemcpy(value, db->d_poolV + E.off, (size_t)E.count * 8, hipMemcpyDeviceToHost));
    }
    return SD_OK;
}

// ---- the queries
// The query table of a call from host offsets (slots == NULL) or batch slots; returns the LDS words k_kfdb_match needs.
static int kfdb_plan_queries(sd_kfdb* db, const char* who, int n_queries, const int32_t* query_offset, const sd_batch* b, const int32_t* slots, int& ldsWords)
{
    if (n_queries < 0 || n_queries > db->maxQ) return set_err(n_queries < 0 ? SD_ERR_INVALID : SD_ERR_CAPACITY, std::string(who) + ": n_queries outside [0, max_queries]");
    db->hQ.assign((size_t)n_queries, SdKfdbQ());
    ldsWords = 1;
    if (slots) {
        const int cap = b->plan.kpCap;
        if (cap > db->maxQW) return set_err(SD_ERR_CAPACITY, std::string(who) + ": the batch's key-point capacity exceeds max_query_words");
        for (int q = 0; q < n_queries; q++) {
            if (slots[q] < 0 || slots[q] >= b->maxImages) return set_err(SD_ERR_INVALID, std::string(who) + ": slot out of range");
            if (!b->d_bowWordF || !b->bowValid[slots[q]]) return set_err(SD_ERR_STATE, std::string(who) + ": no bag of words computed for this slot");
            db->hQ[q].start = (long long)slots[q] * cap; db->hQ[q].n = -1; db->hQ[q].slot = slots[q];
        }
        ldsWords = cap;
        return SD_OK;
    }
    if (n_queries > 0 && !query_offset) return set_err(SD_ERR_INVALID, std::string(who) + ": null query offsets");
    for (int q = 0; q < n_queries; q++) {
        const long long n = (long long)query_offset[q + 1] - query_offset[q];
        if (query_offset[q] < 0 || n < 0) return set_err(SD_ERR_INVALID, std::string(who) + ": query offsets must not be negative or decrease");
        if (n > db->maxQW) return set_err(SD_ERR_CAPACITY, std::string(who) + ": query " + std::to_string(q) + " holds more than max_query_words words");
        db->hQ[q].start = query_offset[q]; db->hQ[q].n = (int)n; db->hQ[q].slot = 0;
        ldsWords = std::max(ldsWords, (int)n);
    }
    return SD_OK;
}

// a CSR of kf ids (excluded sets, score lists) into the staging of the query table; every id must name a possible keyframe
static int kfdb_plan_aux(sd_kfdb* db, const char* who, int n_queries, const int32_t* off, const int32_t* ids, int& longest)
{
    db->hAux.clear();
    longest = 0;
    if (!off) return SD_OK;
    if (n_queries > 0 && off[0] != 0) return set_err(SD_ERR_INVALID, std::string(who) + ": id offsets must start at 0");
    for (int q = 0; q < n_queries; q++) {
        const long long n = (long long)off[q + 1] - off[q];
        if (n < 0) return set_err(SD_ERR_INVALID, std::string(who) + ": id offsets must not decrease");
        db->hQ[q].auxOff = off[q]; db->hQ[q].auxN = (int)n;
        longest = std::max(longest, (int)n);
    }
    const size_t total = n_queries > 0 ? (size_t)off[n_queries] : 0;
    if (total > db->auxCap) return set_err(SD_ERR_CAPACITY, std::string(who) + ": more listed ids than max_queries * max_keyframes");
    if (total && !ids) return set_err(SD_ERR_INVALID, std::string(who) + ": null id list");
    for (size_t i = 0; i < total; i++)
        if (ids[i] < 0 || ids[i] >= db->maxKf) return set_err(SD_ERR_INVALID, std::string(who) + ": listed kf_id outside [0, max_keyframes)");
    db->hAux.assign(ids, ids + total);
    return SD_OK;
}

static SdKfdbArgs kfdb_args(sd_kfdb* db, int nQ, const unsigned* qWord, const double* qVal, const int* meta)
{
    SdKfdbArgs A;
    A.entry = db->d_entry; A.poolW = db->d_poolW; A.poolV = db->d_poolV; A.q = db->d_q; A.qWord = qWord; A.qVal = qVal; A.meta = meta; A.aux = db->d_aux;
    A.K = db->idHigh; A.stride = db->maxKf; A.nQ = nQ; A.maxQW = db->maxQW; A.sortStride = db->sortStride; A.reloc = 0;
    A.cnt = db->d_cnt; A.firstW = db->d_firstW; A.si = db->d_si; A.excl = nullptr; A.mark = db->d_mark; A.sortKey = db->d_sortKey; A.sortKf = db->d_sortKf;
    A.info = db->d_info; A.member = db->d_member; A.acc = db->d_acc; A.cand = db->d_cand; A.score = nullptr;
    return A;
}

static int kfdb_upload_plan(sd_kfdb* db, int nQ, hipStream_t s)
{
    HIPCHK(hipMemcpyAsync(db->d_q, db->hQ.data(), (size_t)nQ * sizeof(SdKfdbQ), hipMemcpyHostToDevice, s));
    if (!db->hAux.empty()) HIPCHK(hipMemcpyAsync(db->d_aux, db->hAux.data(), db->hAux.size() * 4, hipMemcpyHostToDevice, s));
    return SD_OK;
}

// both forms, from a device CSR (b == NULL) or from batch slots
static int kfdb_detect(sd_kfdb* db, const char* who, bool reloc, int n_queries, const int32_t* query_offset, const uint32_t* d_word, const double* d_value,
                       sd_batch* b, const int32_t* slots, const float* min_score, const int32_t* excl_offset, const int32_t* excl_id, void* stream_)
{
    if (!db || (b && !slots)) return set_err(SD_ERR_INVALID, std::string(who) + ": null argument");
    int ldsWords = 1, longest = 0;
    int rc = kfdb_plan_queries(db, who, n_queries, query_offset, b, slots, ldsWords);
    if (rc != SD_OK) return rc;
    if (!b && n_queries > 0 && query_offset[n_queries] > 0 && (!d_word || !d_value)) return set_err(SD_ERR_INVALID, std::string(who) + ": null query arrays");
    if (!reloc) {
        if (n_queries > 0 && !min_score) return set_err(SD_ERR_INVALID, std::string(who) + ": null min_score");
        rc = kfdb_plan_aux(db, who, n_queries, excl_offset, excl_id, longest);
        if (rc != SD_OK) return rc;
        for (int q = 0; q < n_queries; q++) db->hQ[q].minScore = min_score[q];
    } else db->hAux.clear();
    hipStream_t s;
    rc = kfdb_stream(db, stream_, b ? b->lastStream : db->lastStream, s);
    if (rc != SD_OK) return rc;
    db->lastN = n_queries;
    if (n_queries == 0) return SD_OK;
    rc = kfdb_upload_plan(db, n_queries, s);
    if (rc != SD_OK) return rc;
    SdKfdbArgs A = b ? kfdb_args(db, n_queries, b->d_bowWord, b->d_bowVal, b->d_bowMeta) : kfdb_args(db, n_queries, d_word, d_value, nullptr);
    A.reloc = reloc ? 1 : 0;
    if (!reloc && excl_offset) {
        A.excl = db->d_excl;
        hipLaunchKernelGGL(k_kfdb_excl, dim3(n_queries), dim3(256), 0, s, A);
        LAUNCH_CHECK("k_kfdb_excl");
    }
    if (A.K > 0) {
        hipLaunchKernelGGL(k_kfdb_match<0>, dim3((A.K + SD_KFDB_EPB - 1) / SD_KFDB_EPB, n_queries), dim3(256), (size_t)ldsWords * 4, s, A);
        LAUNCH_CHECK("k_kfdb_match");
    }
    hipLaunchKernelGGL(k_kfdb_threshold, dim3(n_queries), dim3(256), 0, s, A);
    LAUNCH_CHECK("k_kfdb_threshold");
    hipLaunchKernelGGL(k_kfdb_tail, dim3(n_queries), dim3(SD_KFDB_TT), (size_t)SD_KFDB_TAIL_LDS, s, A);
    LAUNCH_CHECK("k_kfdb_tail");
    if (reloc && A.K > 0) {
        hipLaunchKernelGGL(k_kfdb_reloc_store, dim3((A.K + 255) / 256), dim3(256), 0, s, A);
        LAUNCH_CHECK("k_kfdb_reloc_store");
    }
    return SD_OK;
}

int sd_kfdb_detect_loop(sd_kfdb* db, int n_queries, const int32_t* query_offset, const uint32_t* d_query_word, const double* d_query_value,
                        const float* min_score, const int32_t* excl_offset, const int32_t* excl_id, void* stream)
{
    return kfdb_detect(db, "kfdb_detect_loop", false, n_queries, query_offset, d_query_word, d_query_value, nullptr, nullptr, min_score, excl_offset, excl_id, stream);
}

int sd_kfdb_detect_loop_batch(sd_kfdb* db, sd_batch* b, int n_queries, const int32_t* image_index, const float* min_score, const int32_t* excl_offset,
                              const int32_t* excl_id, void* stream)
{
    if (!b) return set_err(SD_ERR_INVALID, "kfdb_detect_loop_batch: null batch");
    return kfdb_detect(db, "kfdb_detect_loop_batch", false, n_queries, nullptr, nullptr, nullptr, b, image_index, min_score, excl_offset, excl_id, stream);
}

int sd_kfdb_detect_reloc(sd_kfdb* db, int n_queries, const int32_t* query_offset, const uint32_t* d_query_word, const double* d_query_value, void* stream)
{
    return kfdb_detect(db, "kfdb_detect_reloc", true, n_queries, query_offset, d_query_word, d_query_value, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int sd_kfdb_detect_reloc_batch(sd_kfdb* db, sd_batch* b, int n_queries, const int32_t* image_index, void* stream)
{
    if (!b) return set_err(SD_ERR_INVALID, "kfdb_detect_reloc_batch: null batch");
    return kfdb_detect(db, "kfdb_detect_reloc_batch", true, n_queries, nullptr, nullptr, nullptr, b, image_index, nullptr, nullptr, nullptr, stream);
}

// the host forms: upload the query CSR, run, synchronise
static int kfdb_detect_host(sd_kfdb* db, const char* who, bool reloc, int n_queries, const int32_t* query_offset, const uint32_t* word, const double* value,
                            const float* min_score, const int32_t* excl_offset, const int32_t* excl_id)
{
    if (!db || n_queries < 0 || (n_queries > 0 && !query_offset)) return set_err(SD_ERR_INVALID, std::string(who) + ": null argument");
    const long long total = n_queries > 0 ? query_offset[n_queries] : 0;
    if (total < 0 || (total > 0 && (!word || !value))) return set_err(SD_ERR_INVALID, std::string(who) + ": null query arrays");
    SdDevBuf<unsigned> d_w; SdDevBuf<double> d_v;
    HIPCHK(d_w.alloc(std::max<size_t>((size_t)total, 1) * 4)); HIPCHK(d_v.alloc(std::max<size_t>((size_t)total, 1) * 8));
    if (total) { HIPCHK(hipMemcpy(d_w, word, (size_t)total * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_v, value, (size_t)total * 8, hipMemcpyHostToDevice)); }
    int rc = kfdb_detect(db, who, reloc, n_queries, query_offset, d_w, d_v, nullptr, nullptr, min_score, excl_offset, excl_id, nullptr);
    hipError_t e = hipStreamSynchronize(db->lastStream);                 // before the staging is freed, whatever the call returned
    if (rc != SD_OK) return rc;
    HIPCHK(e);
    return SD_OK;
}

int sd_kfdb_detect_loop_host(sd_kfdb* db, int n_queries, const int32_t* query_offset, const uint32_t* query_word, const double* query_value,
                             const float* min_score, const int32_t* excl_offset, const int32_t* excl_id)
{
    return kfdb_detect_host(db, "kfdb_detect_loop_host", false, n_queries, query_offset, query_word, query_value, min_score, excl_offset, excl_id);
}

int sd_kfdb_detect_reloc_host(sd_kfdb* db, int n_queries, const int32_t* query_offset, const uint32_t* query_word, const double* query_value)
{
    return kfdb_detect_host(db, "kfdb_detect_reloc_host", true, n_queries, query_offset, query_word, query_value, nullptr, nullptr, nullptr);
}

int sd_kfdb_download_candidates(sd_kfdb* db, int query, int32_t* cand, int cap_cand, sd_kfdb_query_info* info, sd_kfdb_member* sharing, int cap_sharing,
                                sd_kfdb_acc* acc, int cap_acc)
{
    if (!db) return SD_ERR_INVALID;
    if (db->lastN < 0) return set_err(SD_ERR_STATE, "kfdb_download_candidates: no query has run");
    if (query < 0 || query >= db->lastN) return set_err(SD_ERR_INVALID, "kfdb_download_candidates: query outside the last call");
    HIPCHK(hipStreamSynchronize(db->lastStream));
    SdKfdbInfo I;
    HIPCHK(hipMemcpy(&I, db->d_info + query, sizeof(I), hipMemcpyDeviceToHost));
    if (info) memcpy(info, &I, sizeof(I));
    if ((cand && I.nCand > cap_cand) || (sharing && I.nShare > cap_sharing) || (acc && I.nAcc > cap_acc))
        return set_err(SD_ERR_CAPACITY, "kfdb_download_candidates: buffer too small");
    const size_t row = (size_t)query * db->maxKf;
    if (cand && I.nCand) HIPCHK(hipMemcpy(cand, db->d_cand + row, (size_t)I.nCand * 4, hipMemcpyDeviceToHost));
    if (sharing && I.nShare) HIPCHK(hipMemcpy(sharing, db->d_member + row, (size_t)I.nShare * sizeof(SdKfdbMember), hipMemcpyDeviceToHost));
    if (acc && I.nAcc) HIPCHK(hipMemcpy(acc, db->d_acc + row, (size_t)I.nAcc * sizeof(SdKfdbAcc), hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_kfdb_score(sd_kfdb* db, int n_queries, const int32_t* query_offset, const uint32_t* d_query_word, const double* d_query_value,
                  const int32_t* list_offset, const int32_t* list_id, float* d_score, void* stream_)
{
    if (!db || (n_queries > 0 && !list_offset)) return set_err(SD_ERR_INVALID, "kfdb_score: null argument");
    int ldsWords = 1, longest = 0;
    int rc = kfdb_plan_queries(db, "kfdb_score", n_queries, query_offset, nullptr, nullptr, ldsWords);
    if (rc != SD_OK) return rc;
    if (n_queries > 0 && query_offset[n_queries] > 0 && (!d_query_word || !d_query_value)) return set_err(SD_ERR_INVALID, "kfdb_score: null query arrays");
    rc = kfdb_plan_aux(db, "kfdb_score", n_queries, list_offset, list_id, longest);
    if (rc != SD_OK) return rc;
    if (longest > 0 && !d_score) return set_err(SD_ERR_INVALID, "kfdb_score: null score array");
    hipStream_t s;
    rc = kfdb_stream(db, stream_, db->lastStream, s);
    if (rc != SD_OK) return rc;
    if (n_queries == 0 || longest == 0) return SD_OK;
    rc = kfdb_upload_plan(db, n_queries, s);
    if (rc != SD_OK) return rc;
    SdKfdbArgs A = kfdb_args(db, n_queries, d_query_word, d_query_value, nullptr);
    A.score = d_score;
    hipLaunchKernelGGL(k_kfdb_match<1>, dim3((longest + SD_KFDB_EPB - 1) / SD_KFDB_EPB, n_queries), dim3(256), (size_t)ldsWords * 4, s, A);
    LAUNCH_CHECK("k_kfdb_match");
    return SD_OK;
}
