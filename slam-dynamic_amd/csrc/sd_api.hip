// C-ABI implementation of include/sd_frontend.h: host orchestration of the HIP kernels.
// There is no CPU fallback anywhere in this file: without a usable HIP device every compute
// entry point returns SD_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstddef>
#include <cmath>
#include <climits>
#include <string>
#include <vector>
#include <map>
#include <memory>
#include <mutex>
#include "k_extract.h"
#include "k_frame.h"
#include "k_fast.h"
#include "k_motion.h"
#include "k_cull.h"
#include "k_tracker.h"
#include "k_cloud.h"
#include "k_pose.h"
#include "k_triangulate.h"
#include "k_fuse.h"
#include "k_ba.h"
#include "k_sim3.h"
#include "k_sim3_opt.h"
#include "k_sim3_refine.h"
#include "k_pnp.h"
#include "k_loop.h"
#include "k_reloc.h"
#include "k_kfdb.h"
#include "k_covis.h"
#include "sd_scw.h"
#include "sd_common.h"
#include "sd_vocab.h"

static thread_local std::string g_err;
int sd_set_err(int code, const std::string& msg) { g_err = msg; return code; }

hipError_t sd_raise_lds_limit(const void* kernel, int bytes)
{
    if (bytes <= 64 * 1024) return hipSuccess;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, int> limits;      // (device, kernel) -> the highest limit set so far
    std::lock_guard<std::mutex> lk(mu);
    int& limit = limits[{dev, kernel}];
    if (bytes > limit && (e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)) == hipSuccess) limit = bytes;
    return e;
}

struct sd_extractor {
    SdParams prm;
};

enum KernelId { K_PYR0, K_PYR, K_FAST, K_QTREE, K_ORIENT, K_BLUR, K_DESC, K_STEREO, K_STEREO_F, K_RGBD, K_GRID, K_UNPROJ, K_PROJ_A, K_PROJ_B, K_BOXSEP, K_SEPARATE, K_UPDATE, K_LOCAL_A, K_LOCAL_B, K_BOW_T, K_BOW_F, K_BOW_S, K_MOTION_P, K_MOTION_H, K_MOTION_S, K_TRI_M, K_TRI_T, K_TRI_R, K_FUSE_S, K_FUSE_R, K_SIM3_M, K_SIM3_S, K_SIM3_A, K_LOOP_BOW, K_LOOP_F, K_LOOP_P, K_LOOP_A, K_RELOC_S, K_RELOC_A, K_RELOC_E, K_RELOC_O, K_RELOC_X, K_COUNT };
static const char* kKernelNames[K_COUNT] = {"k_pyr_level0", "k_pyr_level", "k_fast_cells", "k_quadtree", "k_orient",
                                            "k_blur", "k_describe", "k_stereo_match", "k_stereo_filter", "k_rgbd",
                                            "k_grid_cells", "k_unproject", "k_proj_candidates", "k_proj_resolve",
                                            "k_box_separate", "k_separate", "k_update_frame", "k_local_candidates", "k_local_resolve", "k_bow_transform", "k_bow_finalize", "k_search_by_bow", "k_motion_prepare", "k_motion_hyp", "k_motion_select", "k_tri_match", "k_tri_triangulate", "k_tri_resolve", "k_fuse_search", "k_fuse_resolve", "k_sim3_mark", "k_sim3_search", "k_sim3_agree", "k_search_by_bow_kf", "k_loop_search<0>", "k_loop_search<1>", "k_loop_assign", "k_reloc_search", "k_reloc_assign", "k_reloc_edges", "k_pose_optimize (reloc)", "k_reloc_begin/after/mark/finish"};

#define SD_PT_TW 256
#define SD_PT_TH 16
struct SdPyrTiles { int tilesX = 0, tilesY = 0, srcRowBytes = 0, srcRowsMax = 0, extOff = 0; size_t lds = 0; bool use = false; };

// ---- THE growth rule of the library-owned tables that follow the largest call seen (the nested groups of sd_batch below).  A group is a
// list of arrays that share one size: `unit` bytes per unit of that size plus `fixed` bytes each.  need <= cap: nothing happens.  Otherwise
// the stream the workspace used before this call (`prev`) and the stream of this call are synchronised, since either may still read the old
// arrays; the cap and the job count of the group's last call (`jobs`, where downloads read the group) go to 0; every array is freed, and only
// then allocated at max(need, 2 * cap) clipped to `limit` (the bound the caller enforces on `need`; `need` itself for a size the workspace
// fixes).  A failed allocation leaves the group empty under cap 0: a non-zero cap never stands over a freed array.
struct SdGrowArray { SdDevMem* buf; size_t unit, fixed = 0; };

static int sd_grow(hipStream_t prev, hipStream_t s, size_t& cap, int* jobs, size_t need, size_t limit, std::initializer_list<SdGrowArray> arrays)
{
    if (need <= cap) return SD_OK;
    if (prev != s) HIPCHK(hipStreamSynchronize(prev));
    HIPCHK(hipStreamSynchronize(s));
    const size_t want = std::min(std::max(need, 2 * cap), limit);
    cap = 0;
    if (jobs) *jobs = 0;
    for (const SdGrowArray& a : arrays) a.buf->reset();
    hipError_t e = hipSuccess;
    for (const SdGrowArray& a : arrays) if (e == hipSuccess) e = a.buf->alloc(want * a.unit + a.fixed);
    if (e != hipSuccess) for (const SdGrowArray& a : arrays) a.buf->reset();
    HIPCHK(e);
    cap = want;
    return SD_OK;
}
#define SD_MAX_ENTRIES ((size_t)INT_MAX)      // entry tables are addressed through int32 offsets

// ---- THE process-wide state of the stateless solver entry points (sd_pose_optimize_*, sd_local_ba_*, sd_sim3_ransac_*,
// sd_sim3_optimize_*, sd_pnp_ransac_* and the PnP stage of sd_batch_relocalize_pnp): per solver one SdDeviceTable of a state made of an
// SdTableRing and, where the kernels need scratch memory, an SdWorkspace.  These tables follow the largest call EXACTLY (no doubling as in
// sd_grow: the footprint of a process is the largest call's) and wait on events, not on streams: successive calls may use any streams.
#define SD_SOLVER_RING 8
#define SD_SOLVER_MAX_DEVICES 64

// One State per device behind one mutex per solver.  The array is never destroyed: no device call after the runtime has shut down at exit.
template <typename State>
struct SdDeviceTable {
    State* const states = new State[SD_SOLVER_MAX_DEVICES];
    std::mutex mu;
    struct Locked { std::unique_lock<std::mutex> lk; State* st = nullptr; int device = 0; State* operator->() const { return st; } };
    // the state of the current device, the table locked for as long as `out` lives
    int lock(const char* who, Locked& out)
    {
        HIPCHK(hipGetDevice(&out.device));
        if (out.device < 0 || out.device >= SD_SOLVER_MAX_DEVICES)
            return set_err(SD_ERR_UNSUPPORTED, std::string(who) + ": device index beyond the solver tables");
        out.lk = std::unique_lock<std::mutex>(mu);
        out.st = states + out.device;
        return SD_OK;
    }
};

// The host rows of a call (cameras, problem records) reach its kernels through a ring of SD_SOLVER_RING library-owned device tables, so
// that the host waits only when the call SD_SOLVER_RING calls earlier on the same device has not finished yet.  stage(): the slot `next`
// waits for the event of the call that last used it (created on first use), is regrown to exactly n rows when it is smaller (cap 0 while
// it is freed) and receives the rows on `s`.  publish(), after the call's last launch: records the event on `s` and only then advances,
// so a call that fails in between leaves `next` where it was and the next call stages the same slot again.
template <typename T>
struct SdTableRing {
    SdDevBuf<T> d[SD_SOLVER_RING]; size_t cap[SD_SOLVER_RING] = {}; hipEvent_t done[SD_SOLVER_RING] = {}; int next = 0;
    int stage(const T* rows, size_t n, hipStream_t s, const T*& table)
    {
        const int k = next;
        if (done[k]) HIPCHK(hipEventSynchronize(done[k]));     // the launch that last used this table has read it
        else HIPCHK(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
        if (cap[k] < n) { cap[k] = 0; HIPCHK(d[k].alloc(n * sizeof(T))); cap[k] = n; }
        HIPCHK(hipMemcpyAsync(d[k], rows, n * sizeof(T), hipMemcpyHostToDevice, s));
        table = d[k];
        return SD_OK;
    }
    int publish(hipStream_t s)
    {
        HIPCHK(hipEventRecord(done[next], s));
        next = (next + 1) % SD_SOLVER_RING;
        return SD_OK;
    }
};

// The grow-only scratch arrays the calls of one solver on one device share, behind ONE event recorded after the last launch that used
// them.  enter(): a call that has to grow an array waits for that launch on the host (the arrays are about to be freed), any other call
// makes its stream wait.  grow(): a group of arrays that share a cap goes to exactly `need` units, the cap 0 while they are freed: a
// non-zero cap never stands over a freed array.  leave(): records.  wait(): the host waits for the last call (sd_local_ba_profile).
struct SdWorkspace {
    hipEvent_t done = nullptr;
    int enter(hipStream_t s, bool grows)
    {
        if (!done) HIPCHK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        else if (grows) HIPCHK(hipEventSynchronize(done));
        else HIPCHK(hipStreamWaitEvent(s, done, 0));
        return SD_OK;
    }
    static int grow(size_t& cap, size_t need, std::initializer_list<SdGrowArray> arrays)
    {
        if (cap >= need) return SD_OK;
        cap = 0;
        for (const SdGrowArray& a : arrays) HIPCHK(a.buf->alloc(need * a.unit));
        cap = need;
        return SD_OK;
    }
    int leave(hipStream_t s) { HIPCHK(hipEventRecord(done, s)); return SD_OK; }
    int wait() { HIPCHK(hipEventSynchronize(done)); return SD_OK; }
};
#define SD_TRY(call) do { int rc_ = (call); if (rc_ != SD_OK) return rc_; } while (0)

struct sd_batch {
    std::vector<SdPyrTiles> pyrTiles;      // per level: tile grid of k_pyr_level_tiles
    SdDevBuf<int> d_pyrExt;
    SdDevBuf<int> d_blurTiles; int nBlurTiles = 0;      // k_blur_wide: tile list of one image
    sd_extractor* ex = nullptr;
    SdPlan plan;
    SdDevPlan hplan;
    int maxImages = 0;
    int nExtracted = 0;       // images processed by the last extract
    std::vector<uint8_t> slotValid;   // slot holds frame results (extracted or carried over)
    std::vector<uint8_t> gridValid;   // sd_batch_assign_grid has run on what the slot holds now (sd_batch_fuse asks)
    SdDevBuf<int2> d_pairIdx;
    int nStereo = 0;
    hipStream_t stream = nullptr;
    hipStream_t lastStream = nullptr;
    hipStream_t prevStream = nullptr;     // lastStream before the pick_stream of this call: growth waits for both
    // device buffers
    SdDevBuf<SdDevPlan> d_plan;
    SdDevBuf<SdCell> d_cells;
    SdDevBuf<SdFastCell> d_fcells; int fastListCap = 0, fastMaxCap = 0;   // k_fast_cells_staged: per-cell descriptors, list sizes
    SdDevBuf<int16_t> d_tabs;
    SdDevBuf<uint8_t> d_pyr;
    SdDevBuf<uint8_t> d_blur;
    SdDevBuf<uint32_t> d_cellList;
    SdDevBuf<int> d_cellCount;
    SdDevBuf<uint32_t> d_cand;
    SdDevBuf<uint16_t> d_nodeOf;
    SdDevBuf<int> d_lvlCount;
    SdDevBuf<int> d_candCount;
    SdDevBuf<uint32_t> d_lvlKp;
    SdDevBuf<float2> d_rot;
    SdDevBuf<sd_keypoint> d_kp;
    SdDevBuf<sd_keypoint> d_kpUn; SdDevBuf<sd_keypoint> d_kpDUn; SdDistortion dist; bool hasDist = false; SdDevBuf<int> d_unSlots;   // mvKeysUn / mvdynKeysUn (sd_batch_set_distortion)
    SdDevBuf<uint8_t> d_desc;
    SdDevBuf<int> d_count;
    SdDevBuf<int> d_err;
    bool cullOk = true;              // the per-key-point LDS tables of k_box_separate / k_separate fit this workspace's capacity
    SdDevBuf<float> d_uright;
    SdDevBuf<float> d_depth;
    SdDevBuf<int> d_sad;
    SdDevBuf<unsigned short> d_rowIdx;   // right keypoints bucketed by row (stereo)
    SdDevBuf<int> d_rowStart;
    SdDevBuf<short> d_cellOf;      // grid cell of every keypoint
    SdDevBuf<unsigned short> d_sortedIdx;   // keypoint indices sorted by (cell, index)
    SdDevBuf<unsigned short> d_cellStart;   // [maxImages][3072 + 8]
    int gridSortN = 0;
    SdDevBuf<float> d_xw;          // map-point world positions [maxImages][cap][3]
    SdDevBuf<uint8_t> d_flags;     // bit0: has map point (not outlier); bit1: Observations() > 0
    SdDevBuf<unsigned short> d_pcand;
    SdDevBuf<uint8_t> d_pncand;
    // bag of words (per image): per-feature word / weight / node, FeatureVector (sorted) + runs, BowVector
    SdDevBuf<unsigned> d_bowWordF; SdDevBuf<double> d_bowWF; SdDevBuf<unsigned> d_bowNidF; SdDevBuf<unsigned> d_fvNode; SdDevBuf<unsigned> d_fvFeat;
    SdDevBuf<int> d_fvRunStart; SdDevBuf<unsigned> d_fvRunNode; SdDevBuf<unsigned> d_bowWord; SdDevBuf<double> d_bowVal; SdDevBuf<int> d_bowMeta;
    SdDevBuf<int> d_bowImg; std::vector<uint8_t> bowValid;
    SdDevBuf<float> d_moPts; SdDevBuf<SdMotionNorm> d_moNorm; SdDevBuf<int> d_moCounts; SdDevBuf<double> d_moModels; SdDevBuf<uint8_t> d_moMaskH; SdDevBuf<uint8_t> d_moMaskF;
    SdDevBuf<SdMotionResult> d_moRes; int nMotion = 0;      // TrackHomo model fit
    // sd_batch_search_local_map: frame / offset table (allocated once), and the candidates per local map point, grown with the largest local map seen
    struct LocalMap {
        SdDevBuf<int> d_idx; SdDevBuf<unsigned> d_cand; SdDevBuf<uint8_t> d_n, d_ovf; size_t cap = 0;
        int grow(const sd_batch* b, hipStream_t s, size_t total)
        {
            return sd_grow(b->prevStream, s, cap, nullptr, total, SD_MAX_ENTRIES, {{&d_cand, SD_PROJ_K * 4}, {&d_n, 1}, {&d_ovf, 1}});
        }
    } localMap;
    SdDevBuf<int> d_match;
    SdDevBuf<int> d_pairs;
    SdDevBuf<int> d_npairs;
    SdDevBuf<int> d_nmatch;
    SdDevBuf<float> d_pose;        // staging for host poses: [2][maxImages][16]
    // PoseOptimization per projection pair (sd_batch_pose_optimize), allocated on first use: edges [maxImages][cap], edge ranges,
    // pose in / out, mvbOutlier per edge, return value, camera, whether it ran; pairCam = the camera each pair was matched with
    SdDevBuf<sd_pose_edge> d_poseEdges; SdDevBuf<int> d_poseFirst; SdDevBuf<int> d_poseLast; SdDevBuf<float> d_poseT;
    SdDevBuf<uint8_t> d_poseOut; SdDevBuf<int> d_poseGood; SdDevBuf<sd_camera> d_poseCam; SdDevBuf<int> d_poseMap; SdDevBuf<int> d_poseRan;
    SdDevBuf<float> d_poseTin;
    // SearchForTriangulation / CreateNewMapPoints (k_triangulate.h), grown on demand: the pair records (host staging that must outlive the
    // async upload), and for CreateNewMapPoints the (keyframe x neighbour) match tables with the per-match triangulation results, and the
    // compacted new points per keyframe, which sd_batch_download_new_map_points reads for the `kfs` keyframes of the last call
    struct Tri {
        SdDevBuf<SdTriPair> d_pairs; std::vector<SdTriPair> hostPairs; size_t pairCap = 0;
        SdDevBuf<int> d_match, d_pairList, d_np; SdDevBuf<uint8_t> d_ok; SdDevBuf<float> d_xw; size_t tableCap = 0;
        SdDevBuf<int> d_off, d_nnew; SdDevBuf<sd_new_map_point> d_new; size_t kfCap = 0; int kfs = 0;
        int growPairs(const sd_batch* b, hipStream_t s, size_t n) { return sd_grow(b->prevStream, s, pairCap, nullptr, n, SD_MAX_ENTRIES, {{&d_pairs, sizeof(SdTriPair)}}); }
        int growTables(const sd_batch* b, hipStream_t s, size_t nKf, size_t nP)
        {
            const size_t cap = b->plan.kpCap;
            int rc = sd_grow(b->prevStream, s, kfCap, &kfs, nKf, SD_MAX_ENTRIES, {{&d_off, 4, 4}, {&d_nnew, 4}, {&d_new, cap * sizeof(sd_new_map_point)}});
            if (rc != SD_OK) return rc;
            return sd_grow(b->prevStream, s, tableCap, nullptr, nP, SD_MAX_ENTRIES, {{&d_match, cap * 4}, {&d_pairList, cap * 8}, {&d_np, 4}, {&d_ok, cap}, {&d_xw, cap * 12}});
        }
    } tri;
    // ORBmatcher::Fuse (k_fuse.h), grown with the largest call seen: job tables (slot, offsets, poses), per-entry results, and the
    // first-taker table of k_fuse_resolve where [cap] ints do not fit the LDS (one row per job of THIS call: its size is fixed by the call).
    // d_err is cleared by the download that reports it; `off` holds the offsets of the last call for the downloads
    struct Fuse {
        SdDevBuf<int> d_jobs, d_n, d_first, d_err; SdDevBuf<float> d_T; SdDevBuf<int2> d_best; SdDevBuf<SdFuseHit> d_hits;
        size_t jobCap = 0, entryCap = 0, firstCap = 0; int jobs = 0; std::vector<int32_t> off;
        int grow(const sd_batch* b, hipStream_t s, size_t nJobs, size_t total, bool firstInMemory)
        {
            if (!d_err) { HIPCHK(d_err.alloc(4)); HIPCHK(hipMemset(d_err, 0, 4)); }
            int rc = sd_grow(b->prevStream, s, jobCap, &jobs, nJobs, 65535, {{&d_jobs, 8, 4}, {&d_T, 64}, {&d_n, 4}});
            if (rc == SD_OK) rc = sd_grow(b->prevStream, s, entryCap, &jobs, total, SD_MAX_ENTRIES, {{&d_best, sizeof(int2)}, {&d_hits, sizeof(SdFuseHit)}});
            if (rc == SD_OK && firstInMemory) rc = sd_grow(b->prevStream, s, firstCap, &jobs, nJobs, nJobs, {{&d_first, (size_t)b->plan.kpCap * 4}});
            return rc;
        }
    } fuse;
    // sd_batch_search_by_sim3: pair table (staged on the host) and per-pair rows [pairs][cap], grown with the largest call seen;
    // sd_batch_compute_sim3_refine runs its search over the same tables.  d_err belongs to one call
    struct Sim3 {
        SdDevBuf<SdSim3Pair> d_pairs; SdDevBuf<int> d_match1, d_match2, d_match12, d_found, d_err; SdDevBuf<uint8_t> d_already;
        size_t cap = 0; int pairs = 0; std::vector<SdSim3Pair> host;
        int grow(const sd_batch* b, hipStream_t s, size_t nPairs)
        {
            const size_t row = b->plan.kpCap;
            if (!d_err) HIPCHK(d_err.alloc(4));
            return sd_grow(b->prevStream, s, cap, &pairs, nPairs, 32767,
                           {{&d_pairs, sizeof(SdSim3Pair)}, {&d_match1, row * 4}, {&d_match2, row * 4}, {&d_match12, row * 4}, {&d_found, 4}, {&d_already, row}});
        }
    } sim3;
    // sd_batch_compute_sim3_refine (k_sim3_refine.h): job table (staged on the host), merged matches, built correspondences, optimiser
    // tables, final matches
    struct Sim3Refine {
        SdDevBuf<SdRefineJob> d_jobs; SdDevBuf<int> d_merged, d_final; SdDevBuf<sd_sim3_opt_corr> d_corr; SdDevBuf<SdSim3OptProb> d_prob;
        SdDevBuf<sd_sim3_opt_result> d_opt; SdDevBuf<uint8_t> d_state; SdDevBuf<sd_sim3_refine_result> d_out;
        size_t cap = 0; int jobs = 0; std::vector<SdRefineJob> host;
        int grow(const sd_batch* b, hipStream_t s, size_t nJobs)
        {
            const size_t row = b->plan.kpCap;
            return sd_grow(b->prevStream, s, cap, &jobs, nJobs, 32767,
                           {{&d_jobs, sizeof(SdRefineJob)}, {&d_merged, row * 4}, {&d_final, row * 4}, {&d_corr, row * sizeof(sd_sim3_opt_corr)},
                            {&d_prob, sizeof(SdSim3OptProb)}, {&d_opt, sizeof(sd_sim3_opt_result)}, {&d_state, row}, {&d_out, sizeof(sd_sim3_refine_result)}});
        }
    } sim3Refine;
    // the Scw matchers of loop closing (k_loop.h), grown with the largest call seen.  T: the decomposed poses (host staging that outlives
    // the upload), SHARED by sd_batch_fuse_sim3 and sd_batch_search_by_projection_sim3.  The rest is the projection's: the offsets of the
    // last call, its job tables, the kept keys per candidate, the per-entry results and the per-job rows [jobs][cap].  d_err belongs to one call
    struct Loop {
        std::vector<float> T; std::vector<int32_t> off;
        SdDevBuf<int> d_jobs, d_nm, d_assigned, d_err, d_listN; SdDevBuf<float> d_T; SdDevBuf<unsigned> d_list; SdDevBuf<int2> d_best;
        size_t jobCap = 0, entryCap = 0; int jobs = 0;
        int grow(const sd_batch* b, hipStream_t s, size_t nJobs, size_t total)
        {
            if (!d_err) { HIPCHK(d_err.alloc(4)); HIPCHK(hipMemset(d_err, 0, 4)); }
            int rc = sd_grow(b->prevStream, s, jobCap, &jobs, nJobs, 65535, {{&d_jobs, 8, 4}, {&d_T, 64}, {&d_nm, 4}, {&d_assigned, (size_t)b->plan.kpCap * 4}});
            if (rc != SD_OK) return rc;
            return sd_grow(b->prevStream, s, entryCap, &jobs, total, SD_MAX_ENTRIES, {{&d_list, SD_PROJ_K * 4}, {&d_listN, 4}, {&d_best, sizeof(int2)}});
        }
    } loop;
    // sd_batch_search_by_projection_reloc (k_reloc.h), grown with the largest call seen: job tables (slots, poses, th, ORBdist; the slot
    // pairs staged on the host), the kept keys per keyframe feature and the result rows [jobs][cap].  sd_batch_relocalize_refine reuses
    // the slot table and the kept keys.  d_err belongs to one call
    struct Reloc {
        std::vector<int2> slots; size_t cap = 0; int jobs = 0;
        SdDevBuf<int2> d_slots, d_best; SdDevBuf<float> d_T, d_th; SdDevBuf<int> d_orb, d_nm, d_listN, d_exit, d_frame, d_from, d_err; SdDevBuf<unsigned> d_list;
        int grow(const sd_batch* b, hipStream_t s, size_t nJobs)
        {
            const size_t row = b->plan.kpCap;
            if (!d_err) { HIPCHK(d_err.alloc(4)); HIPCHK(hipMemset(d_err, 0, 4)); }
            return sd_grow(b->prevStream, s, cap, &jobs, nJobs, SD_RELOC_MAX_JOBS,
                           {{&d_slots, sizeof(int2)}, {&d_T, 64}, {&d_th, 4}, {&d_orb, 4}, {&d_nm, 4}, {&d_list, row * SD_PROJ_K * 4}, {&d_listN, row * 4},
                            {&d_exit, row * 4}, {&d_best, row * sizeof(int2)}, {&d_frame, row * 4}, {&d_from, row * 4}});
        }
    } reloc;
    // sd_batch_relocalize_refine: the assignment after each step P [5][jobs][cap], the two searches' rows [2][jobs][cap], the three
    // optimisations' edges [3][jobs][cap] with their ranges, flags and return values, the poses [4][jobs][16], mvbOutlier [jobs][cap],
    // the sFound marks [jobs][n_points] (as many bytes as THIS call needs), the per-job th / ORBdist / camera of the steps (staged on the
    // host), the results
    struct RelocRefine {
        SdDevBuf<int> d_P, d_from, d_exit, d_nm, d_good, d_first, d_last, d_orb; SdDevBuf<int2> d_best; SdDevBuf<sd_pose_edge> d_edges;
        SdDevBuf<uint8_t> d_edgeOut, d_outlier, d_mark; SdDevBuf<float> d_T, d_th; SdDevBuf<sd_camera> d_cam; SdDevBuf<sd_reloc_result> d_res;
        std::vector<float> th; std::vector<int> orb; std::vector<sd_camera> cam; size_t cap = 0, markCap = 0; int jobs = 0;
        int grow(const sd_batch* b, hipStream_t s, size_t nJobs, size_t markBytes)
        {
            const size_t row = b->plan.kpCap;
            int rc = sd_grow(b->prevStream, s, markCap, &jobs, markBytes, markBytes, {{&d_mark, 1}});
            if (rc != SD_OK) return rc;
            return sd_grow(b->prevStream, s, cap, &jobs, nJobs, SD_RELOC_MAX_JOBS,
                           {{&d_P, 5 * row * 4}, {&d_from, 2 * row * 4}, {&d_exit, 2 * row * 4}, {&d_best, 2 * row * sizeof(int2)}, {&d_nm, 2 * 4}, {&d_good, 3 * 4},
                            {&d_first, 3 * 4}, {&d_last, 3 * 4}, {&d_edges, 3 * row * sizeof(sd_pose_edge)}, {&d_edgeOut, 3 * row}, {&d_outlier, row}, {&d_T, 4 * 64},
                            {&d_th, 2 * 4}, {&d_orb, 2 * 4}, {&d_cam, sizeof(sd_camera)}, {&d_res, sizeof(sd_reloc_result)}});
        }
    } relocRefine;
    // sd_batch_relocalize_pnp: per job the gathered problem [jobs][cap], its mask, record, problem row and caller's record, the row and pose
    // handed to the cascade, and the SetRansacParameters table per N [cap + 1]
    struct RelocPnp {
        SdDevBuf<sd_pnp_corr> d_corr; SdDevBuf<uint8_t> d_inl; SdDevBuf<sd_pnp_result> d_res; SdDevBuf<SdPnpProb> d_prob; SdDevBuf<sd_pnp_problem> d_in;
        SdDevBuf<int> d_row; SdDevBuf<float> d_T; SdDevBuf<int2> d_table; std::vector<int2> table; size_t cap = 0, tableCap = 0; int jobs = 0;
        int grow(const sd_batch* b, hipStream_t s, size_t nJobs)
        {
            const size_t row = b->plan.kpCap;
            int rc = sd_grow(b->prevStream, s, tableCap, &jobs, row + 1, row + 1, {{&d_table, sizeof(int2)}});
            if (rc != SD_OK) return rc;
            return sd_grow(b->prevStream, s, cap, &jobs, nJobs, SD_RELOC_MAX_JOBS,
                           {{&d_corr, row * sizeof(sd_pnp_corr)}, {&d_inl, row}, {&d_res, sizeof(sd_pnp_result)}, {&d_prob, sizeof(SdPnpProb)},
                            {&d_in, sizeof(sd_pnp_problem)}, {&d_row, row * 4}, {&d_T, 64}});
        }
    } relocPnp;
    std::vector<sd_camera> pairCam, hPoseCam; std::vector<int32_t> hPoseMap;
    int nPairs = 0;
    int dlPairs = 0;          // pairs sd_batch_download_matches may read (the tracker also keeps pairs at [n_lanes, 2 * n_lanes))
    // dynamic-object cull
    SdDevBuf<SdFrameBoxes> d_fb;
    SdDevBuf<SdFrameBoxes> d_fbStage;     // one upload per sd_batch_first_separate call
    SdDevBuf<int> d_boxItems;
    SdDevBuf<sd_keypoint> d_kpT; SdDevBuf<uint8_t> d_descT; SdDevBuf<float> d_urT; SdDevBuf<float> d_depT;
    SdDevBuf<sd_keypoint> d_kpD; SdDevBuf<uint8_t> d_descD; SdDevBuf<float> d_urD; SdDevBuf<float> d_depD;
    SdDevBuf<int> d_slots;
    SdDevBuf<float> d_HorF; SdDevBuf<int> d_sepFlag; SdDevBuf<int> d_lastIdx; SdDevBuf<int> d_lastStatus; SdDevBuf<int> d_nLast;
    SdDevBuf<int> d_dynStart; SdDevBuf<int> d_dynStatus; SdDevBuf<int> d_sepMatches; SdDevBuf<int> d_sepRet;
    SdDevBuf<int2> d_sepPairs;
    SdDevBuf<int2> d_copyPairs;
    // sd_batch_backproject_dense: 64-bit words of point marks (as many as the workspace's geometry needs), row counts, poses, slots
    struct Cloud {
        SdDevBuf<unsigned long long> d_bits; SdDevBuf<int> d_rows, d_slots; SdDevBuf<double> d_T; size_t cap = 0;
        int grow(const sd_batch* b, hipStream_t s, size_t need, int rows3)
        {
            const size_t nI = b->maxImages;
            return sd_grow(b->prevStream, s, cap, nullptr, need, need, {{&d_bits, 8}, {&d_rows, 0, nI * rows3 * 2 * 4}, {&d_T, 0, nI * 16 * 8}, {&d_slots, 0, nI * 4}});
        }
    } cloud;
    int itemsCap = 0;
    int nSepPairs = 0;
    const int* sepActive = nullptr;          // active mask of the last separate (tracker mode), applied by update_frame too
    std::vector<SdFrameBoxes> hostBoxes;     // staging that must outlive the async uploads
    std::vector<int2> hostPairs, hostCopyPairs;
    SdDevBuf<uint8_t> d_stage;    // staging for host-image uploads
    size_t stageBytes = 0;
    int qtMN = 0, qtSortP = 0;
    size_t qtLds = 0;
    // profiling
    bool profiling = false;
    struct Rec { hipEvent_t a, b; int kid; };
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    double totalMs[K_COUNT] = {0};
    int64_t launches[K_COUNT] = {0};
    ~sd_batch()
    {
        for (auto& r : pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        for (auto e : pool) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// mvKeysUn of the batch: the key points themselves unless a distortion was set (Frame.cc:814-818)
#define KPUN(b) ((b)->hasDist ? (b)->d_kpUn : (b)->d_kp)
#define KPDUN(b) ((b)->hasDist ? (b)->d_kpDUn : (b)->d_kpD)

// ---- What a frame is: the per-slot arrays of a workspace, slot k of each at base + k * bytes, in ONE fixed order.  Every mover of frames
// (sd_batch_copy_frame[s], the tracker's pool / initialisation-extractor copies, the prefetched records) takes its segments from here, so a
// new per-slot array is added in this list and nowhere else.  The subsets are prefixes of each other:
//   EXTRACT  what ORB extraction writes
//   FRONT    the history-free half (+ undistortion, stereo / RGB-D association); padded to 16 bytes per segment, in this order, it is the
//            layout of a prefetched record (sd_tracker_prefetched_record_bytes)
//   ALL      Frame's copy constructor (Frame.cc:39-63)
enum SdFrameSubset { SD_FRAME_EXTRACT, SD_FRAME_FRONT, SD_FRAME_ALL };
struct SdSlotArray { const void* base; size_t bytes; SdFrameSubset subset; bool distOnly; };

static int frame_arrays(const sd_batch* b, SdFrameSubset subset, SdSlotArray out[SD_COPY_SEGS])
{
    const size_t cap = b->plan.kpCap, kp = cap * sizeof(sd_keypoint);
    const SdSlotArray all[] = {
        {b->d_count, 4, SD_FRAME_EXTRACT, false}, {b->d_lvlCount, (size_t)b->plan.nlevels * 4, SD_FRAME_EXTRACT, false},
        {b->d_kp, kp, SD_FRAME_EXTRACT, false}, {b->d_desc, cap * 32, SD_FRAME_EXTRACT, false},
        {b->d_uright, cap * 4, SD_FRAME_FRONT, false}, {b->d_depth, cap * 4, SD_FRAME_FRONT, false}, {b->d_sad, cap * 4, SD_FRAME_FRONT, false},
        {b->d_kpUn, kp, SD_FRAME_FRONT, true},
        {b->d_cellOf, cap * 2, SD_FRAME_ALL, false}, {b->d_xw, cap * 12, SD_FRAME_ALL, false}, {b->d_flags, cap, SD_FRAME_ALL, false},
        {b->d_sortedIdx, cap * 2, SD_FRAME_ALL, false}, {b->d_cellStart, (SD_GRID_CELLS + 8) * 2, SD_FRAME_ALL, false},
        {b->d_kpD, kp, SD_FRAME_ALL, false}, {b->d_descD, cap * 32, SD_FRAME_ALL, false}, {b->d_urD, cap * 4, SD_FRAME_ALL, false},
        {b->d_depD, cap * 4, SD_FRAME_ALL, false}, {b->d_kpDUn, kp, SD_FRAME_ALL, true},
        {b->d_fb, sizeof(SdFrameBoxes), SD_FRAME_ALL, false}, {b->d_boxItems, (size_t)b->itemsCap * 4, SD_FRAME_ALL, false},
    };
    static_assert(sizeof(all) / sizeof(all[0]) <= SD_COPY_SEGS, "SdCopyTable must hold every per-slot array of a frame");
    int n = 0;
    for (const SdSlotArray& a : all)
        if (a.subset <= subset && (!a.distOnly || b->hasDist)) out[n++] = a;
    return n;
}

// `subset` of src's slots -> dst's slots: two workspaces of the same plan, or one and the same
static SdCopyTable frame_copy_table(const sd_batch* src, const sd_batch* dst, SdFrameSubset subset)
{
    SdSlotArray A[SD_COPY_SEGS], B[SD_COPY_SEGS];
    SdCopyTable T;
    T.n = frame_arrays(src, subset, A);
    frame_arrays(dst, subset, B);
    for (int i = 0; i < T.n; i++) {
        T.src[i] = (const char*)A[i].base; T.dst[i] = (char*)const_cast<void*>(B[i].base);
        T.srcStride[i] = T.dstStride[i] = T.bytes[i] = (unsigned)A[i].bytes;
    }
    return T;
}

// copy z of n: slot pairs[z].x -> pairs[z].y, or without a list slot srcFirst + z * srcStep -> dstFirst + z * dstStep
static int launch_copy_frames(const SdCopyTable& T, int blocks, int n, const int2* pairs, int srcFirst, int srcStep, int dstFirst, int dstStep, hipStream_t s)
{
    hipLaunchKernelGGL(k_copy_frames, dim3(blocks, T.n, n), dim3(256), 0, s, T, pairs, srcFirst, srcStep, dstFirst, dstStep);
    LAUNCH_CHECK("k_copy_frames");
    return SD_OK;
}

extern "C" {

int sd_version(void) { return 100; }

const char* sd_status_string(int s)
{
    switch (s) {
    case SD_OK: return "ok";
    case SD_ERR_INVALID: return "invalid argument";
    case SD_ERR_NO_DEVICE: return "no HIP device";
    case SD_ERR_HIP: return "HIP error";
    case SD_ERR_CAPACITY: return "buffer too small";
    case SD_ERR_UNSUPPORTED: return "unsupported geometry";
    case SD_ERR_STATE: return "call sequence error";
    default: return "unknown";
    }
}

const char* sd_last_error(void) { return g_err.c_str(); }

int sd_device_count(int* n)
{
    if (!n) return SD_ERR_INVALID;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c <= 0) { *n = 0; return set_err(SD_ERR_NO_DEVICE, "hipGetDeviceCount: no device"); }
    *n = c;
    return SD_OK;
}

int sd_extractor_create(sd_extractor** out, int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
{
    if (!out) return SD_ERR_INVALID;
    *out = nullptr;
    if (nfeatures < 1 || nlevels < 1 || nlevels > SD_MAX_LEVELS || !(scaleFactor > 1.0f) || iniThFAST < 1 ||
        iniThFAST > 255 || minThFAST < 1 || minThFAST > 255)
        return set_err(SD_ERR_INVALID, "extractor parameters out of range");
    sd_extractor* ex = new sd_extractor();
    sd_params_init(ex->prm, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST);
    *out = ex;
    return SD_OK;
}

int sd_extractor_destroy(sd_extractor* ex) { delete ex; return SD_OK; }

int sd_extractor_set_blur_taps(sd_extractor* ex, const uint16_t taps[7])
{
    if (!ex || !taps) return SD_ERR_INVALID;
    unsigned sum = 0;
    for (int i = 0; i < 7; i++) sum += taps[i];
    if (sum > 257) return set_err(SD_ERR_INVALID, "blur taps must sum to <= 257 (8.8 fixed point)");
    for (int i = 0; i < 7; i++) if (taps[i] > 255) return set_err(SD_ERR_INVALID, "each blur tap must be <= 255");
    memcpy(ex->prm.blurTaps, taps, 14);
    return SD_OK;
}

int sd_extractor_levels(const sd_extractor* ex, int* nlevels, float* scale_factor)
{
    if (!ex) return SD_ERR_INVALID;
    if (nlevels) *nlevels = ex->prm.nlevels;
    if (scale_factor) *scale_factor = (float)ex->prm.scaleFactor;
    return SD_OK;
}

int sd_extractor_tables(const sd_extractor* ex, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                        int32_t* quota, int32_t* umax)
{
    if (!ex) return SD_ERR_INVALID;
    const SdParams& p = ex->prm;
    for (int i = 0; i < p.nlevels; i++) {
        if (scale) scale[i] = p.scale[i];
        if (inv_scale) inv_scale[i] = p.inv[i];
        if (sigma2) sigma2[i] = p.sigma2[i];
        if (inv_sigma2) inv_sigma2[i] = p.invSigma2[i];
        if (quota) quota[i] = p.quota[i];
    }
    if (umax) for (int i = 0; i < 16; i++) umax[i] = p.umax[i];
    return SD_OK;
}

int sd_extractor_level_size(const sd_extractor* ex, int width, int height, int level, int* lw, int* lh)
{
    if (!ex || level < 0 || level >= ex->prm.nlevels || width < 1 || height < 1) return SD_ERR_INVALID;
    if (lw) *lw = sd_cvRoundf((float)width * ex->prm.inv[level]);
    if (lh) *lh = sd_cvRoundf((float)height * ex->prm.inv[level]);
    return SD_OK;
}

// minKpCap: row stride of the per-image result arrays at least this (a tracker whose lanes switch between two extractors)
static int batch_create_impl(std::unique_ptr<sd_batch>& out, sd_extractor* ex, int width, int height, int max_images, int minKpCap)
{
    if (!ex || width < 1 || height < 1 || max_images < 1) return set_err(SD_ERR_INVALID, "bad batch arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_err(SD_ERR_NO_DEVICE, "no HIP device: the front end has no CPU fallback");
    std::unique_ptr<sd_batch> b(new sd_batch());
    b->ex = ex;
    b->maxImages = max_images;
    if (!sd_plan_build(b->plan, ex->prm, width, height, minKpCap)) return set_err(SD_ERR_UNSUPPORTED, b->plan.error);
    const SdPlan& P = b->plan;
    SdDevPlan& D = b->hplan;
    memset(&D, 0, sizeof(D));
    for (int l = 0; l < P.nlevels; l++) D.lv[l] = P.lv[l];
    D.nlevels = P.nlevels; D.iniTh = ex->prm.iniTh; D.minTh = ex->prm.minTh;
    D.cellTotal = (int)P.cells.size(); D.cellListCap = P.cellListCap;
    D.kpCapLevels = P.kpCapLevels; D.kpCap = P.kpCap;
    D.pyrImageBytes = P.pyrImageBytes; D.blurImageBytes = P.blurImageBytes;
    for (int i = 0; i < 16; i++) D.umax[i] = ex->prm.umax[i];
    for (int i = 0; i < 7; i++) D.taps[i] = ex->prm.blurTaps[i];
    // quadtree LDS sizing: list capacity L (quota + 3, the initial nodes, or the cell count of a level)
    int MN = 0;
    for (int l = 0; l < P.nlevels; l++) {
        MN = std::max(MN, P.lv[l].kpCap + 8);
        MN = std::max(MN, P.lv[l].nCells + 16);
    }
    MN = (MN + 7) & ~7;
    int sortP = 1;
    while (sortP < MN) sortP <<= 1;
    size_t lds = (size_t)sortP * 8 + (size_t)MN * (8 + 8 + 4 * 4 + 16 * 2 + 2 * 3) + 64;
    if (lds > 160 * 1024 - 256 || MN > 30000)
        return set_err(SD_ERR_UNSUPPORTED, "per-level feature quota too large for the LDS quadtree (nfeatures too high)");
    b->qtMN = MN; b->qtSortP = sortP; b->qtLds = lds;

    const size_t nI = (size_t)max_images;
    HIPCHK(b->d_plan.alloc(sizeof(SdDevPlan)));
    HIPCHK(b->d_cells.alloc(sizeof(SdCell) * P.cells.size()));
    HIPCHK(b->d_fcells.alloc(sizeof(SdFastCell) * P.cells.size()));
    HIPCHK(b->d_tabs.alloc(sizeof(int16_t) * P.tabs.size()));
    HIPCHK(b->d_pyr.alloc(nI * P.pyrImageBytes + 4096));
    HIPCHK(b->d_blur.alloc(nI * P.blurImageBytes + 4096));
    HIPCHK(b->d_cellList.alloc(nI * P.cellListCap * 4 + 64));
    HIPCHK(b->d_cellCount.alloc(nI * P.cells.size() * 4));
    HIPCHK(b->d_cand.alloc(nI * P.cellListCap * 4 + 64));
    HIPCHK(b->d_nodeOf.alloc(nI * P.cellListCap * 2 + 64));
    HIPCHK(b->d_lvlCount.alloc(nI * P.nlevels * 4 + SD_MAX_LEVELS * 4));      // + padding: sd_level_counts loads SD_MAX_LEVELS entries
    HIPCHK(b->d_candCount.alloc(nI * P.nlevels * 4));
    HIPCHK(b->d_lvlKp.alloc(nI * P.kpCapLevels * 4));
    HIPCHK(b->d_rot.alloc(nI * P.kpCapLevels * sizeof(float2)));
    HIPCHK(b->d_kp.alloc(nI * P.kpCap * sizeof(sd_keypoint)));
    HIPCHK(b->d_desc.alloc(nI * P.kpCap * 32));
    HIPCHK(b->d_count.alloc(nI * 4));
    HIPCHK(b->d_err.alloc(4));
    HIPCHK(b->d_uright.alloc(nI * P.kpCap * 4));
    HIPCHK(b->d_depth.alloc(nI * P.kpCap * 4));
    HIPCHK(b->d_sad.alloc(nI * P.kpCap * 4));
    HIPCHK(b->d_rowIdx.alloc(nI * P.kpCap * 2));
    HIPCHK(b->d_rowStart.alloc(nI * (size_t)(P.lv[0].H + 8) * 4));
    HIPCHK(b->d_cellOf.alloc(nI * P.kpCap * 2));
    HIPCHK(b->d_sortedIdx.alloc(nI * P.kpCap * 2));
    HIPCHK(b->d_cellStart.alloc(nI * (SD_GRID_CELLS + 8) * 2));
    { int sn = 1; while (sn < P.kpCap) sn <<= 1; b->gridSortN = sn; }
    HIPCHK(b->d_xw.alloc(nI * P.kpCap * 12));
    HIPCHK(b->d_flags.alloc(nI * P.kpCap));
    HIPCHK(b->d_pcand.alloc(nI * P.kpCap * SD_PROJ_K * 2));
    HIPCHK(b->d_pncand.alloc(nI * P.kpCap));
    HIPCHK(b->d_match.alloc(nI * P.kpCap * 4));
    HIPCHK(b->d_pairs.alloc(nI * P.kpCap * 8));
    HIPCHK(b->d_npairs.alloc(nI * 4));
    HIPCHK(b->d_nmatch.alloc(nI * 4));
    HIPCHK(b->d_pose.alloc(nI * 2 * 16 * 4));
    b->itemsCap = 2 * P.kpCap;
    HIPCHK(b->d_fb.alloc(nI * sizeof(SdFrameBoxes)));
    HIPCHK(b->d_fbStage.alloc(nI * sizeof(SdFrameBoxes)));
    HIPCHK(b->d_boxItems.alloc(nI * b->itemsCap * 4));
    HIPCHK(b->d_kpT.alloc(nI * P.kpCap * sizeof(sd_keypoint)));
    HIPCHK(b->d_descT.alloc(nI * P.kpCap * 32));
    HIPCHK(b->d_urT.alloc(nI * P.kpCap * 4));
    HIPCHK(b->d_depT.alloc(nI * P.kpCap * 4));
    HIPCHK(b->d_kpD.alloc(nI * P.kpCap * sizeof(sd_keypoint)));
    HIPCHK(b->d_descD.alloc(nI * P.kpCap * 32));
    HIPCHK(b->d_urD.alloc(nI * P.kpCap * 4));
    HIPCHK(b->d_depD.alloc(nI * P.kpCap * 4));
    HIPCHK(b->d_slots.alloc(nI * 4));
    HIPCHK(b->d_HorF.alloc(nI * 9 * 4));
    HIPCHK(b->d_sepFlag.alloc(nI * 4));
    HIPCHK(b->d_lastIdx.alloc(nI * SD_MAXB * 4));
    HIPCHK(b->d_lastStatus.alloc(nI * SD_MAXB * 4));
    HIPCHK(b->d_nLast.alloc(nI * 4));
    HIPCHK(b->d_dynStart.alloc(nI * (SD_MAXB + 1) * 4));
    HIPCHK(b->d_dynStatus.alloc(nI * b->itemsCap * 4));
    HIPCHK(b->d_sepMatches.alloc(nI * b->itemsCap * 8));
    HIPCHK(b->d_sepRet.alloc(nI * 4));
    HIPCHK(b->d_sepPairs.alloc(nI * sizeof(int2)));
    HIPCHK(b->d_copyPairs.alloc(nI * sizeof(int2)));
    HIPCHK(b->d_pairIdx.alloc(nI * sizeof(int2)));
    b->slotValid.assign(nI, 0);
    b->gridValid.assign(nI, 0);
    HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    HIPCHK(hipMemcpy(b->d_plan, &D, sizeof(D), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->d_cells, P.cells.data(), sizeof(SdCell) * P.cells.size(), hipMemcpyHostToDevice));
    {
        std::vector<SdFastCell> fc(P.cells.size());
        for (size_t i = 0; i < P.cells.size(); i++) {
            const SdCell& c = P.cells[i];
            const SdLevel& g = P.lv[c.level];
            fc[i].srcOff = (uint32_t)(g.pyrOffset + (SD_EDGE + c.y0) * g.stride + SD_XOFF + c.x0 - 1);
            fc[i].stride = g.stride;
            fc[i].ww = (short)(c.x1 - c.x0); fc[i].wh = (short)(c.y1 - c.y0);
            fc[i].jw = c.jw; fc[i].ih = c.ih; fc[i].listOffset = c.listOffset; fc[i].cap = c.cap;
            b->fastListCap = std::max(b->fastListCap, (c.x1 - c.x0 - 6) * (c.y1 - c.y0 - 6));      // largest scanned area of a cell
            b->fastMaxCap = std::max(b->fastMaxCap, c.cap);
        }
        b->fastListCap = (b->fastListCap + 7) & ~7;
        HIPCHK(hipMemcpy(b->d_fcells, fc.data(), sizeof(SdFastCell) * fc.size(), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(b->d_tabs, P.tabs.data(), sizeof(int16_t) * P.tabs.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(b->d_err, 0, 4));
    HIPCHK(hipMemset(b->d_fb, 0, nI * sizeof(SdFrameBoxes)));
    // the dynamic-object kernels keep per-key-point tables in LDS, sized by this workspace's capacity
    const int needSep = (int)sd_separate_lds(P.kpCap), needBox = (int)sd_box_separate_lds(P.kpCap);
    // The kernels' static LDS (k_box_separate: 3 KB of per-box tables) counts against the same 160 KB: without it a capacity of
    // 8,034 to 8,188 slots passed this test and the workspace could not be created at all -- raising the limit failed with
    // "invalid argument" (tests/test_gpu_motion.py, the 8120-feature workspace).
    hipFuncAttributes faSep, faBox;
    HIPCHK(hipFuncGetAttributes(&faSep, (const void*)k_separate));
    HIPCHK(hipFuncGetAttributes(&faBox, (const void*)k_box_separate));
    b->cullOk = needSep + faSep.sharedSizeBytes <= 160 * 1024 && needBox + faBox.sharedSizeBytes <= 160 * 1024;       // otherwise sd_batch_first_separate / sd_batch_separate refuse (extraction and matching are not affected)
    if (b->cullOk) {
        HIPCHK(sd_raise_lds_limit((const void*)k_separate, needSep));
        HIPCHK(sd_raise_lds_limit((const void*)k_box_separate, needBox));
    }
    HIPCHK(hipMemset(b->d_count, 0, nI * 4));
    HIPCHK(hipMemset(b->d_lvlCount, 0, nI * P.nlevels * 4));
    HIPCHK(sd_raise_lds_limit((const void*)k_quadtree, (int)lds));
    b->lastStream = b->stream;
    out = std::move(b);
    return SD_OK;
}

int sd_batch_create(sd_batch** out, sd_extractor* ex, int width, int height, int max_images)
{
    if (!out) return SD_ERR_INVALID;
    std::unique_ptr<sd_batch> b;
    int rc = batch_create_impl(b, ex, width, height, max_images, 0);
    *out = b.release();
    return rc;
}

int sd_batch_destroy(sd_batch* b)
{
    if (b) { (void)hipDeviceSynchronize(); delete b; }
    return SD_OK;
}

int sd_batch_kp_capacity(const sd_batch* b, int* cap)
{
    if (!b || !cap) return SD_ERR_INVALID;
    *cap = b->plan.kpCap;
    return SD_OK;
}

// ---- profiling helpers: hipEvents on the stream the kernel is launched on
static hipEvent_t get_event(sd_batch* b)
{
    if (!b->pool.empty()) { hipEvent_t e = b->pool.back(); b->pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
struct ProfScope {
    sd_batch* b; hipStream_t s; int kid; hipEvent_t a, e;
    ProfScope(sd_batch* b_, hipStream_t s_, int kid_) : b(b_), s(s_), kid(kid_)
    {
        if (b->profiling) { a = get_event(b); e = get_event(b); (void)hipEventRecord(a, s); }
    }
    ~ProfScope()
    {
        if (b->profiling) { (void)hipEventRecord(e, s); b->pending.push_back({a, e, kid}); }
    }
};
static void drain_profile(sd_batch* b)
{
    for (auto& r : b->pending) {
        float ms = 0;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            b->totalMs[r.kid] += ms;
            b->launches[r.kid]++;
        }
        b->pool.push_back(r.a); b->pool.push_back(r.b);
    }
    b->pending.clear();
}

static bool slot_ok(const sd_batch* b, int image) { return image >= 0 && image < b->maxImages && b->slotValid[image]; }

// What a call asks of the slots its job table names: in range (else SD_ERR_INVALID), holding results, sd_batch_assign_grid run,
// sd_batch_compute_bow run (else SD_ERR_STATE).  GRID and BOW are asked together with RESULTS.
enum { SD_SLOT_RANGE = 1, SD_SLOT_RESULTS = 2, SD_SLOT_GRID = 4, SD_SLOT_BOW = 8 };

// One pass over the n jobs of a table, slot a[i] (and a2[i], where a job names two): the refusal of the first job that fails a test of
// `need`, a job's tests in the order above.  A call that refuses every slot out of range before any state makes two calls, RANGE first.
static int check_slots(const sd_batch* b, const char* who, const int32_t* a, const int32_t* a2, int n, int need)
{
    auto fails = [&](int i, auto ok) { return !ok(a[i]) || (a2 && !ok(a2[i])); };
    for (int i = 0; i < n; i++) {
        if ((need & SD_SLOT_RANGE) && fails(i, [&](int k) { return k >= 0 && k < b->maxImages; })) return set_err(SD_ERR_INVALID, std::string(who) + ": slot out of range");
        if ((need & SD_SLOT_RESULTS) && fails(i, [&](int k) { return slot_ok(b, k); })) return set_err(SD_ERR_STATE, std::string(who) + ": slot holds no results");
        if ((need & SD_SLOT_GRID) && fails(i, [&](int k) { return b->gridValid[k] != 0; }))
            return set_err(SD_ERR_STATE, std::string(who) + ": sd_batch_assign_grid has not run on this slot");
        if ((need & SD_SLOT_BOW) && fails(i, [&](int k) { return b->d_bowWordF && b->bowValid[k]; }))
            return set_err(SD_ERR_STATE, std::string(who) + ": sd_batch_compute_bow has not run on this slot");
    }
    return SD_OK;
}

// off[0, n]: the ranges of n jobs in one table; maxLen (optional) receives the longest
static int check_offsets(const char* who, const int32_t* off, int n, int* maxLen)
{
    bool ok = off[0] == 0;
    int longest = 0;
    for (int j = 0; j < n && ok; j++) { ok = off[j + 1] >= off[j]; if (ok) longest = std::max(longest, off[j + 1] - off[j]); }
    if (!ok) return set_err(SD_ERR_INVALID, std::string(who) + ": offsets must start at 0 and ascend");
    if (maxLen) *maxLen = longest;
    return SD_OK;
}

// The stream of this call: the caller's, or the one the workspace used last
static hipStream_t pick_stream(sd_batch* b, void* stream_)
{
    b->prevStream = b->lastStream;
    return b->lastStream = stream_ ? (hipStream_t)stream_ : b->lastStream;
}

static int extract_impl(sd_batch* b, const uint8_t* d_gray, size_t stride, size_t image_pitch, int n_images, void* stream_, int colorMode);

int sd_batch_extract_device(sd_batch* b, const uint8_t* d_gray, size_t stride, size_t image_pitch, int n_images,
                            void* stream_)
{
    return extract_impl(b, d_gray, stride, image_pitch, n_images, stream_, 0);
}

int sd_batch_extract_color_device(sd_batch* b, const uint8_t* d_src, size_t stride, size_t image_pitch, int rgb_order, int n_images,
                                  void* stream_)
{
    return extract_impl(b, d_src, stride, image_pitch, n_images, stream_, rgb_order ? 2 : 1);
}

int sd_batch_extract_pixels_device(sd_batch* b, const uint8_t* d_src, size_t stride, size_t image_pitch, int channels, int rgb_order,
                                   int n_images, void* stream_)
{
    if (channels != 1 && channels != 3 && channels != 4) return set_err(SD_ERR_INVALID, "images must have 1, 3 or 4 channels (Tracking.cc:175-200)");
    return extract_impl(b, d_src, stride, image_pitch, n_images, stream_, channels == 1 ? 0 : (channels == 3 ? 1 : 3) + (rgb_order ? 1 : 0));
}

// Once per workspace: the LDS extents of k_pyr_level_tiles per level (or the per-thread kernel as a fallback) and the tiles' source origins
static int ensure_pyr_tiles(sd_batch* b)
{
    if (!b->pyrTiles.empty()) return SD_OK;
    const SdPlan& P = b->plan;
    const int nl = P.nlevels;
    std::vector<SdPyrTiles> tiles(nl);
    auto refl = [](int p, int len) { if (p < 0) p = -p; if (p >= len) p = 2 * (len - 1) - p; return p; };
    std::vector<int> ext;             // per level: source column origin of every tile column, (row origin, rows) of every tile row
    for (int l = 1; l < nl; l++) {
        const SdLevel& g = P.lv[l];
        const int16_t* ct = &P.tabs[4 * (size_t)g.tabOffset];
        const int16_t* rt = ct + 4 * (size_t)g.W;
        const int PW = g.W + 2 * SD_EDGE, HPl = g.H + 2 * SD_EDGE, sH = P.lv[l - 1].H;
        SdPyrTiles t;
        t.tilesX = (PW + SD_PT_XSHIFT + SD_PT_TW - 1) / SD_PT_TW; t.tilesY = (HPl + SD_PT_TH - 1) / SD_PT_TH;
        t.extOff = (int)ext.size();
        int spanX = 0, spanY = 0;
        for (int tx = 0; tx < t.tilesX; tx++) {
            int lo = 1 << 30, hi = -1;
            for (int k = 0; k < SD_PT_TW; k++) {
                const int sx = ct[4 * refl(std::min(std::max(tx * SD_PT_TW - SD_PT_XSHIFT + k, 0), PW - 1) - SD_EDGE, g.W)];
                lo = std::min(lo, sx); hi = std::max(hi, sx);
            }
            spanX = std::max(spanX, hi - lo + 2);
            ext.push_back(lo);
        }
        for (int ty = 0; ty < t.tilesY; ty++) {
            int lo = 1 << 30, hi = -1;
            for (int k = 0; k < SD_PT_TH; k++) {
                const int sy = rt[4 * refl(std::min(ty * SD_PT_TH + k, HPl - 1) - SD_EDGE, g.H)];
                lo = std::min(lo, std::min(std::max(sy, 0), sH - 1)); hi = std::max(hi, std::min(std::max(sy + 1, 0), sH - 1));
            }
            spanY = std::max(spanY, hi - lo + 1);
            ext.push_back(lo); ext.push_back(hi - lo + 1);
        }
        t.srcRowBytes = (spanX + 16 + 15) & ~15; t.srcRowsMax = spanY;
        t.lds = (size_t)t.srcRowsMax * t.srcRowBytes + (size_t)t.srcRowsMax * SD_PT_TW * 2;
        t.use = t.lds <= 48 * 1024 && g.W >= 40 && g.H >= 40;
        tiles[l] = t;
    }
    SdDevBuf<int> d_ext;
    if (!ext.empty()) {
        HIPCHK(d_ext.alloc(ext.size() * 4));
        HIPCHK(hipMemcpy(d_ext, ext.data(), ext.size() * 4, hipMemcpyHostToDevice));
    }
    b->d_pyrExt = std::move(d_ext);
    b->pyrTiles = std::move(tiles);
    return SD_OK;
}

// Once per workspace: the non-empty 128 x SD_BLUR_TR tiles of one image, level by level (k_blur_wide)
static int ensure_blur_tiles(sd_batch* b)
{
    if (b->d_blurTiles) return SD_OK;
    const SdPlan& P = b->plan;
    std::vector<int> t;
    for (int l = 0; l < P.nlevels; l++)
        for (int ty = 0; ty * SD_BLUR_TR < P.lv[l].H; ty++)
            for (int tx = 0; tx * 128 < P.lv[l].W; tx++) t.push_back(l | (tx << 8) | (ty << 16));
    SdDevBuf<int> d_tiles;
    HIPCHK(d_tiles.alloc(t.size() * 4));
    HIPCHK(hipMemcpy(d_tiles, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    b->d_blurTiles = std::move(d_tiles);
    b->nBlurTiles = (int)t.size();
    return SD_OK;
}

// colorMode 0: 8-bit gray input; 1 / 2: 3-channel BGR / RGB, 3 / 4: 4-channel BGRA / RGBA input converted on the way into level 0
static int extract_impl(sd_batch* b, const uint8_t* d_gray, size_t stride, size_t image_pitch, int n_images, void* stream_, int colorMode)
{
    if (!b || n_images < 0 || n_images > b->maxImages) return set_err(SD_ERR_INVALID, "bad extract arguments");
    hipStream_t s = stream_ ? (hipStream_t)stream_ : b->stream;
    b->lastStream = s;
    b->nExtracted = 0;
    b->nStereo = 0;
    if (n_images == 0) return SD_OK;
    if (!d_gray) return set_err(SD_ERR_INVALID, "null image pointer");
    const SdPlan& P = b->plan;
    const int bpp = colorMode == 0 ? 1 : (colorMode <= 2 ? 3 : 4), rgbOrder = (colorMode == 2 || colorMode == 4) ? 1 : 0;
    if (stride < (size_t)P.W * bpp) return set_err(SD_ERR_INVALID, "stride smaller than width");
    const int nl = P.nlevels;
    int rc = ensure_pyr_tiles(b);                 // the per-workspace tile tables, built by the first extract
    if (rc == SD_OK) rc = ensure_blur_tiles(b);
    if (rc != SD_OK) return rc;
    {
        ProfScope ps(b, s, K_PYR0);
        const SdLevel& g = P.lv[0];
        {
            // interior 16-byte groups flattened over (row, group) so that every wave is full + a small kernel for the groups on the frame
            const int gpr = g.W / 16;                                                    // groups fully inside the interior
            const int lastGroup = (g.W + SD_EDGE - 1) / 16;                              // group of the last frame column
            const int tail = lastGroup - gpr + 1, rows = g.H + 2 * SD_EDGE;
            const dim3 gi((unsigned)((size_t)rows * gpr + 255) / 256, n_images), gf((unsigned)(rows * (2 + tail) + 255) / 256, n_images);
            if (gpr > 0) {
                const uint32_t gprInv = 0xFFFFFFFFu / (uint32_t)gpr + 1u;
                if (bpp == 4) hipLaunchKernelGGL(k_pyr_level0_rgba, gi, dim3(256), 0, s, d_gray, stride, image_pitch, rgbOrder, b->d_pyr, b->d_plan, gpr, gprInv);
                else if (bpp == 3) hipLaunchKernelGGL(k_pyr_level0_rgb, gi, dim3(256), 0, s, d_gray, stride, image_pitch, rgbOrder, b->d_pyr, b->d_plan, gpr, gprInv);
                else hipLaunchKernelGGL(k_pyr_level0_gray, gi, dim3(256), 0, s, d_gray, stride, image_pitch, b->d_pyr, b->d_plan, gpr, gprInv);
            }
            if (colorMode) hipLaunchKernelGGL(k_pyr_level0_rgb_frame, gf, dim3(256), 0, s, d_gray, stride, image_pitch, rgbOrder, b->d_pyr, b->d_plan, gpr, tail, bpp);
            else hipLaunchKernelGGL(k_pyr_level0_gray_frame, gf, dim3(256), 0, s, d_gray, stride, image_pitch, b->d_pyr, b->d_plan, gpr, tail);
        }
    }
    LAUNCH_CHECK("k_pyr_level0");
    for (int l = 1; l < nl; l++) {
        ProfScope ps(b, s, K_PYR);
        const SdLevel& g = P.lv[l];
        const SdPyrTiles& t = b->pyrTiles[l];
        if (t.use) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pyr_level_tiles<SD_PT_TW, SD_PT_TH>), dim3(t.tilesX, t.tilesY, n_images), dim3(256), t.lds, s, b->d_pyr,
                               (const short4*)b->d_tabs.get(), b->d_plan, l, t.srcRowBytes, t.srcRowsMax, b->d_pyrExt + t.extOff);
        } else {                         // resize ratios too large for the LDS tile: one thread per 4 pixels x 4 rows
            dim3 blk(64, 4), grd(((g.W + 39 + 3) / 4 + 63) / 64, (g.H + 2 * SD_EDGE + 4 * SD_PYR_ROWS - 1) / (4 * SD_PYR_ROWS), n_images);
            hipLaunchKernelGGL(k_pyr_level, grd, blk, 0, s, b->d_pyr, (const short4*)b->d_tabs.get(), b->d_plan, l);
        }
    }
    LAUNCH_CHECK("k_pyr_level");
    {
        // (Running the blur on a side stream was measured twice: forked after the pyramid (beside FAST) no gain; forked after
        // FAST so that it runs beside the quadtree both kernels stretch (0.45 + 0.35 ms -> 0.73 ms together): +0.8 % frames/s,
        // not worth a second stream and overlapped per-kernel timings — everything stays on one stream.)
        ProfScope ps(b, s, K_BLUR);
        dim3 grd((unsigned)b->nBlurTiles * (unsigned)((n_images + 7) / 8 * 8));
        unsigned tapSum = 0;
        for (int i = 0; i < 7; i++) tapSum += b->hplan.taps[i];
        if (tapSum <= 256) hipLaunchKernelGGL(k_blur_wide<false>, grd, dim3(256), 0, s, b->d_pyr, b->d_blur, b->d_plan, b->d_blurTiles, b->nBlurTiles, n_images);
        else hipLaunchKernelGGL(k_blur_wide<true>, grd, dim3(256), 0, s, b->d_pyr, b->d_blur, b->d_plan, b->d_blurTiles, b->nBlurTiles, n_images);
    }
    LAUNCH_CHECK("k_blur");
    {
        ProfScope ps(b, s, K_FAST);
        dim3 grd((unsigned)P.cells.size(), n_images);
        if (P.maxWin <= SD_FS_MAXWIN)
        {
            const int listCap = b->fastListCap;
            const size_t lds = (size_t)listCap * 4 + ((size_t)b->fastMaxCap + 4) * 4;
            // 128-thread workgroups: measured best (64: 0.66 ms, 128: 0.49 ms, 256: 0.65 ms per 128-image launch)
            // grid = (8 x cells, image groups): workgroup -> (cell, XCD, image group) -- see the kernel
            SdFastArgs fa;
            fa.pyrImageBytes = P.pyrImageBytes; fa.cellTotal = (int)P.cells.size(); fa.nImages = n_images; fa.listCap = listCap;
            fa.minTh = b->hplan.minTh; fa.iniTh = b->hplan.iniTh; fa.cellListCap = P.cellListCap;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fast_cells_staged<128>), dim3((unsigned)P.cells.size() * 8u, (unsigned)((n_images + 7) / 8)), dim3(128),
                               lds, s, b->d_pyr, b->d_fcells, b->d_cellList, b->d_cellCount, fa);
        }
        else
            hipLaunchKernelGGL(k_fast_cells, grd, dim3(256), 0, s, b->d_pyr, b->d_cells, b->d_cellList, b->d_cellCount, b->d_plan);
    }
    LAUNCH_CHECK("k_fast_cells");
    {
        ProfScope ps(b, s, K_QTREE);
        dim3 grd(n_images, nl);
        hipLaunchKernelGGL(k_quadtree, grd, dim3(256), b->qtLds, s, b->d_cellList, b->d_cellCount, b->d_cells, b->d_cand,
                           b->d_nodeOf, b->d_lvlCount, b->d_candCount, b->d_lvlKp, b->d_err, b->d_plan, b->qtMN, b->qtSortP);
    }
    LAUNCH_CHECK("k_quadtree");
    {
        ProfScope ps(b, s, K_ORIENT);
        const int gpi = (P.kpCapLevels + 7) / 8, n8 = (n_images + 7) / 8 * 8;
        hipLaunchKernelGGL(k_orient, dim3((unsigned)gpi * n8), dim3(256), 0, s, b->d_pyr, b->d_lvlKp, b->d_lvlCount, b->d_kp, b->d_rot, b->d_count,
                           b->d_plan, n_images, gpi);
    }
    LAUNCH_CHECK("k_orient");
    {
        ProfScope ps(b, s, K_DESC);
        const int gpi = (P.kpCapLevels + 4 * SD_DP_KPW - 1) / (4 * SD_DP_KPW), n8 = (n_images + 7) / 8 * 8;
        hipLaunchKernelGGL(k_describe, dim3((unsigned)gpi * n8), dim3(256), 0, s, b->d_blur, b->d_lvlKp, b->d_lvlCount, b->d_rot, b->d_desc, b->d_plan,
                           n_images, gpi);
    }
    LAUNCH_CHECK("k_describe");
    b->nExtracted = n_images;
    for (int i = 0; i < n_images; i++) { b->slotValid[i] = 1; b->gridValid[i] = 0; }
    return SD_OK;
}

int sd_batch_sync(sd_batch* b)
{
    if (!b) return SD_ERR_INVALID;
    HIPCHK(hipStreamSynchronize(b->lastStream));
    drain_profile(b);
    int err = 0;
    HIPCHK(hipMemcpy(&err, b->d_err, 4, hipMemcpyDeviceToHost));
    if (err) {
        (void)hipMemset(b->d_err, 0, 4);
        return set_err(SD_ERR_UNSUPPORTED, "device capacity exceeded: 1|2 quadtree nodes, 4 projection candidates, 8|16|32 box tables, 64 local-map candidates, 128 Sim3 projection keys (flag " + std::to_string(err) + ")");
    }
    return SD_OK;
}

int sd_batch_extract_host(sd_batch* b, const uint8_t* gray, size_t stride, size_t image_pitch, int n_images)
{
    if (!b || n_images < 0 || n_images > b->maxImages) return set_err(SD_ERR_INVALID, "bad extract arguments");
    if (!gray || n_images == 0) { b->nExtracted = 0; return SD_OK; }   // empty image: silent return
    const SdPlan& P = b->plan;
    const size_t tight = (size_t)P.W * P.H;
    const size_t need = tight * n_images;
    if (b->stageBytes < need) {
        b->stageBytes = 0;
        HIPCHK(b->d_stage.alloc(need));
        b->stageBytes = need;
    }
    for (int i = 0; i < n_images; i++)
        HIPCHK(hipMemcpy2DAsync(b->d_stage + tight * i, P.W, gray + image_pitch * i, stride, P.W, P.H,
                                hipMemcpyHostToDevice, b->stream));
    int rc = sd_batch_extract_device(b, b->d_stage, P.W, tight, n_images, b->stream);
    if (rc != SD_OK) return rc;
    return sd_batch_sync(b);
}

int sd_batch_results_device(sd_batch* b, sd_keypoint** d_kp, uint8_t** d_desc, int32_t** d_count, int* cap)
{
    if (!b) return SD_ERR_INVALID;
    if (d_kp) *d_kp = b->d_kp;
    if (d_desc) *d_desc = b->d_desc;
    if (d_count) *d_count = b->d_count;
    if (cap) *cap = b->plan.kpCap;
    return SD_OK;
}

int sd_batch_counts(sd_batch* b, int32_t* counts, int n_images)
{
    if (!b || !counts || n_images < 0 || n_images > b->maxImages) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    for (int i = 0; i < n_images; i++) counts[i] = 0;
    int n = std::min(n_images, b->nExtracted);
    if (n > 0) HIPCHK(hipMemcpy(counts, b->d_count, (size_t)n * 4, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_batch_download(sd_batch* b, int image, sd_keypoint* kp, uint8_t* desc, int cap, int* n, int32_t* per_level)
{
    if (!b || !n || image < 0 || image >= b->maxImages) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    *n = 0;
    if (per_level) for (int l = 0; l < b->plan.nlevels; l++) per_level[l] = 0;
    if (!slot_ok(b, image)) return SD_OK;
    int cnt = 0;
    HIPCHK(hipMemcpy(&cnt, b->d_count + image, 4, hipMemcpyDeviceToHost));
    if (cnt > cap) { *n = cnt; return set_err(SD_ERR_CAPACITY, "keypoint buffer too small"); }
    if (cnt > 0) {
        if (kp) HIPCHK(hipMemcpy(kp, b->d_kp + (size_t)image * b->plan.kpCap, (size_t)cnt * sizeof(sd_keypoint), hipMemcpyDeviceToHost));
        if (desc) HIPCHK(hipMemcpy(desc, b->d_desc + (size_t)image * b->plan.kpCap * 32, (size_t)cnt * 32, hipMemcpyDeviceToHost));
    }
    if (per_level)
        HIPCHK(hipMemcpy(per_level, b->d_lvlCount + (size_t)image * b->plan.nlevels, (size_t)b->plan.nlevels * 4, hipMemcpyDeviceToHost));
    *n = cnt;
    return SD_OK;
}

int sd_batch_pyramid_level(sd_batch* b, int image, int level, const uint8_t** d_interior, int* w, int* h, size_t* stride)
{
    if (!b || image < 0 || image >= b->maxImages || level < 0 || level >= b->plan.nlevels) return SD_ERR_INVALID;
    const SdLevel& g = b->plan.lv[level];
    if (d_interior) *d_interior = b->d_pyr + (size_t)image * b->plan.pyrImageBytes + g.pyrOffset + (size_t)SD_EDGE * g.stride + SD_XOFF;
    if (w) *w = g.W;
    if (h) *h = g.H;
    if (stride) *stride = (size_t)g.stride;
    return SD_OK;
}

int sd_batch_download_pyramid(sd_batch* b, int image, int level, uint8_t* padded_out)
{
    if (!b || !padded_out || image < 0 || image >= b->maxImages || level < 0 || level >= b->plan.nlevels) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    const SdLevel& g = b->plan.lv[level];
    const uint8_t* src = b->d_pyr + (size_t)image * b->plan.pyrImageBytes + g.pyrOffset + (SD_XOFF - SD_EDGE);
    HIPCHK(hipMemcpy2D(padded_out, g.W + 2 * SD_EDGE, src, g.stride, g.W + 2 * SD_EDGE, g.H + 2 * SD_EDGE, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_batch_download_blurred(sd_batch* b, int image, int level, uint8_t* out)
{
    if (!b || !out || image < 0 || image >= b->maxImages || level < 0 || level >= b->plan.nlevels) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    const SdLevel& g = b->plan.lv[level];
    const uint8_t* src = b->d_blur + (size_t)image * b->plan.blurImageBytes + g.blurOffset;
    HIPCHK(hipMemcpy2D(out, g.W, src, g.blurStride, g.W, g.H, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_batch_candidate_counts(sd_batch* b, int image, int32_t* per_level)
{
    if (!b || !per_level || image < 0 || image >= b->maxImages) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    HIPCHK(hipMemcpy(per_level, b->d_candCount + (size_t)image * b->plan.nlevels, (size_t)b->plan.nlevels * 4, hipMemcpyDeviceToHost));
    return SD_OK;
}

// ---------------------------------------------------------------- stereo / RGB-D
int sd_batch_stereo_match(sd_batch* b, int n_frames, float mbf, float fx, void* stream_)
{
    if (!b || n_frames < 0) return SD_ERR_INVALID;
    if (2 * n_frames > b->nExtracted) return set_err(SD_ERR_STATE, "stereo_match needs 2*n_frames extracted images (L,R interleaved)");
    if (!(fx > 0) || !(mbf > 0)) return set_err(SD_ERR_INVALID, "mbf and fx must be positive");
    if (b->plan.kpCap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    hipStream_t s = pick_stream(b, stream_);
    if (n_frames == 0) return SD_OK;
    const int H0 = b->plan.lv[0].H;
    // a right keypoint's band is floor(y - r) .. ceil(y + r), r = 2*scale[octave]: +2 covers floor/ceil and (int)y
    const int bandR = (int)ceilf(2.0f * b->plan.lv[b->plan.nlevels - 1].scale) + 2;
    {
        ProfScope ps(b, s, K_STEREO);
        const size_t lds = (size_t)(2 * H0 + 16) * 4;
        hipLaunchKernelGGL(k_row_sort, dim3(n_frames, 2), dim3(256), lds, s, b->d_kp, b->d_count, b->d_rowIdx, b->d_rowStart,
                           b->plan.kpCap, H0);
    }
    LAUNCH_CHECK("k_row_sort");
    {
        ProfScope ps(b, s, K_STEREO);
        if (SD_SR_ROWS + 2 * bandR + 2 > SD_SR_RS) return set_err(SD_ERR_UNSUPPORTED, "stereo row band larger than the staged row table (too many pyramid levels)");
        const int chunks = (H0 + SD_SR_ROWS - 1) / SD_SR_ROWS;      // SD_SR_ROWS image rows of one frame per workgroup, XCD-aware 1-D order
        hipLaunchKernelGGL(k_stereo_match, dim3((unsigned)chunks * (unsigned)((n_frames + 7) / 8 * 8)), dim3(256), 0, s, b->d_kp, b->d_desc, b->d_count, b->d_pyr, b->d_uright,
                           b->d_depth, b->d_sad, b->d_rowIdx, b->d_rowStart, bandR, b->d_plan, mbf, fx, n_frames, chunks);
    }
    LAUNCH_CHECK("k_stereo_match");
    {
        ProfScope ps(b, s, K_STEREO_F);
        hipLaunchKernelGGL(k_stereo_filter, dim3(n_frames), dim3(256), 0, s, b->d_count, b->d_uright, b->d_depth, b->d_sad, b->d_plan);
    }
    LAUNCH_CHECK("k_stereo_filter");
    b->nStereo = n_frames;
    return SD_OK;
}

int sd_batch_stereo_device(sd_batch* b, float** d_uright, float** d_depth, int* cap)
{
    if (!b) return SD_ERR_INVALID;
    if (d_uright) *d_uright = b->d_uright;
    if (d_depth) *d_depth = b->d_depth;
    if (cap) *cap = b->plan.kpCap;
    return SD_OK;
}

int sd_batch_download_stereo(sd_batch* b, int frame, float* uright, float* depth, int32_t* sad_dist, int cap)
{
    if (!b || frame < 0 || frame >= b->nStereo) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int cnt = 0;
    HIPCHK(hipMemcpy(&cnt, b->d_count + 2 * frame, 4, hipMemcpyDeviceToHost));
    if (cnt > cap) return set_err(SD_ERR_CAPACITY, "stereo buffer too small");
    const size_t off = (size_t)(2 * frame) * b->plan.kpCap;
    if (cnt > 0) {
        if (uright) HIPCHK(hipMemcpy(uright, b->d_uright + off, (size_t)cnt * 4, hipMemcpyDeviceToHost));
        if (depth) HIPCHK(hipMemcpy(depth, b->d_depth + off, (size_t)cnt * 4, hipMemcpyDeviceToHost));
        if (sad_dist) HIPCHK(hipMemcpy(sad_dist, b->d_sad + off, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    }
    return SD_OK;
}

int sd_batch_rgbd_from_u16(sd_batch* b, const uint16_t* d_depth, size_t stride_elems, size_t image_pitch_elems,
                           int n_images, float depth_factor, float mbf, void* stream_)
{
    if (!b || !d_depth || n_images < 0) return SD_ERR_INVALID;
    if (n_images > b->nExtracted) return set_err(SD_ERR_STATE, "rgbd lookup needs extracted images");
    hipStream_t s = pick_stream(b, stream_);
    if (n_images == 0) return SD_OK;
    {
        ProfScope ps(b, s, K_RGBD);
        dim3 grd((b->plan.kpCap + 255) / 256, n_images);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rgbd<uint16_t>), grd, dim3(256), 0, s, b->d_kp, KPUN(b), b->d_count, d_depth, stride_elems,
                           image_pitch_elems, depth_factor, mbf, b->d_uright, b->d_depth, b->d_plan);
    }
    LAUNCH_CHECK("k_rgbd");
    return SD_OK;
}

int sd_batch_rgbd_from_f32(sd_batch* b, const float* d_depth, size_t stride_elems, size_t image_pitch_elems, int n_images,
                           float mbf, void* stream_)
{
    return sd_batch_rgbd_from_f32_scaled(b, d_depth, stride_elems, image_pitch_elems, n_images, 1.0f, mbf, stream_);
}

int sd_batch_rgbd_from_f32_scaled(sd_batch* b, const float* d_depth, size_t stride_elems, size_t image_pitch_elems, int n_images,
                                  float depth_factor, float mbf, void* stream_)
{
    if (!b || !d_depth || n_images < 0) return SD_ERR_INVALID;
    if (n_images > b->nExtracted) return set_err(SD_ERR_STATE, "rgbd lookup needs extracted images");
    hipStream_t s = pick_stream(b, stream_);
    if (n_images == 0) return SD_OK;
    {
        ProfScope ps(b, s, K_RGBD);
        dim3 grd((b->plan.kpCap + 255) / 256, n_images);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rgbd<float>), grd, dim3(256), 0, s, b->d_kp, KPUN(b), b->d_count, d_depth, stride_elems,
                           image_pitch_elems, depth_factor, mbf, b->d_uright, b->d_depth, b->d_plan);
    }
    LAUNCH_CHECK("k_rgbd");
    return SD_OK;
}

int sd_batch_download_rgbd(sd_batch* b, int image, float* uright, float* depth, int cap)
{
    if (!b || !slot_ok(b, image)) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int cnt = 0;
    HIPCHK(hipMemcpy(&cnt, b->d_count + image, 4, hipMemcpyDeviceToHost));
    if (cnt > cap) return set_err(SD_ERR_CAPACITY, "rgbd buffer too small");
    const size_t off = (size_t)image * b->plan.kpCap;
    if (cnt > 0) {
        if (uright) HIPCHK(hipMemcpy(uright, b->d_uright + off, (size_t)cnt * 4, hipMemcpyDeviceToHost));
        if (depth) HIPCHK(hipMemcpy(depth, b->d_depth + off, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    }
    return SD_OK;
}

// ---------------------------------------------------------------- preprocessing / Hamming
int sd_cvt_gray_device(const uint8_t* d_src, int width, int height, size_t src_stride, size_t src_pitch, int channels,
                       int rgb_order, uint8_t* d_dst, size_t dst_stride, size_t dst_pitch, int n_images, void* stream)
{
    if (!d_src || !d_dst || width < 1 || height < 1 || n_images < 0 || (channels != 3 && channels != 4)) return SD_ERR_INVALID;
    if (n_images == 0) return SD_OK;
    dim3 blk(64, 4), grd(((width + 3) / 4 + 63) / 64, (height + 3) / 4, n_images);
    if (channels == 3)
        hipLaunchKernelGGL(k_cvt_gray3_wide, dim3(((width + 15) / 16 + 63) / 64, (height + 3) / 4, n_images), blk, 0, (hipStream_t)stream, d_src, width, height, src_stride, src_pitch,
                           rgb_order, d_dst, dst_stride, dst_pitch);
    else
        hipLaunchKernelGGL(k_cvt_gray, grd, blk, 0, (hipStream_t)stream, d_src, width, height, src_stride, src_pitch, channels,
                           rgb_order, d_dst, dst_stride, dst_pitch);
    LAUNCH_CHECK("k_cvt_gray");
    return SD_OK;
}

int sd_depth_to_f32_device(const uint16_t* d_src, int width, int height, size_t src_stride_elems, float factor, float* d_dst,
                           int n_images, size_t src_pitch_elems, void* stream)
{
    if (!d_src || !d_dst || width < 1 || height < 1 || n_images < 0) return SD_ERR_INVALID;
    if (n_images == 0) return SD_OK;
    dim3 blk(64, 4), grd((width + 63) / 64, (height + 3) / 4, n_images);
    hipLaunchKernelGGL(k_depth_to_f32, grd, blk, 0, (hipStream_t)stream, d_src, width, height, src_stride_elems, src_pitch_elems,
                       factor, d_dst);
    LAUNCH_CHECK("k_depth_to_f32");
    return SD_OK;
}

int sd_descriptor_distance(const uint8_t a[32], const uint8_t b[32])
{
    int d = 0;
    for (int i = 0; i < 4; i++) {
        uint64_t x, y;
        memcpy(&x, a + 8 * i, 8); memcpy(&y, b + 8 * i, 8);
        d += __builtin_popcountll(x ^ y);
    }
    return d;
}

int sd_hamming_matrix_device(const uint8_t* d_a, int na, const uint8_t* d_b, int nb, uint16_t* d_out, void* stream)
{
    if (!d_a || !d_b || !d_out || na < 0 || nb < 0) return SD_ERR_INVALID;
    if (na == 0 || nb == 0) return SD_OK;
    dim3 blk(64, 4), grd((nb + 63) / 64, (na + 3) / 4);
    hipLaunchKernelGGL(k_hamming_matrix, grd, blk, 0, (hipStream_t)stream, d_a, na, d_b, nb, d_out);
    LAUNCH_CHECK("k_hamming_matrix");
    return SD_OK;
}


// ---------------------------------------------------------------- grid / unproject / projection matcher
static int cam_ok(const sd_camera* c)
{
    return c && c->fx > 0 && c->fy > 0 && c->mnMaxX > c->mnMinX && c->mnMaxY > c->mnMinY;
}
static SdCamera to_cam(const sd_camera* c)
{
    SdCamera k = {c->fx, c->fy, c->cx, c->cy, c->mbf, c->mb, c->mnMinX, c->mnMaxX, c->mnMinY, c->mnMaxY};
    return k;
}

static int assign_grid_impl(sd_batch* b, int n_images, int image_step, const sd_camera* cam, void* stream_);
int sd_batch_assign_grid(sd_batch* b, int n_images, const sd_camera* cam, void* stream_) { return assign_grid_impl(b, n_images, 1, cam, stream_); }

// slots 0, image_step, 2 * image_step, ... (n_images of them): the tracker grids the left images only
static int assign_grid_impl(sd_batch* b, int n_images, int image_step, const sd_camera* cam, void* stream_)
{
    if (!b || n_images < 0 || image_step < 1 || !cam_ok(cam)) return set_err(SD_ERR_INVALID, "bad grid arguments");
    if ((n_images - 1) * image_step + 1 > b->nExtracted) return set_err(SD_ERR_STATE, "grid needs extracted images");
    hipStream_t s = pick_stream(b, stream_);
    if (n_images == 0) return SD_OK;
    {
        ProfScope ps(b, s, K_GRID);
        dim3 grd((b->plan.kpCap + 255) / 256, n_images);
        hipLaunchKernelGGL(k_grid_cells, grd, dim3(256), 0, s, KPUN(b), b->d_count, b->d_cellOf, to_cam(cam), b->plan.kpCap, image_step);
    }
    LAUNCH_CHECK("k_grid_cells");
    const size_t gridLds = (size_t)(SD_GRID_CELLS + 8) * 4 + (size_t)SD_GRID_CELLS * 4 + (size_t)b->plan.kpCap * 2 + 16;
    if (gridLds > 64 * 1024) return set_err(SD_ERR_UNSUPPORTED, "too many keypoints per image for the grid sort");
    {
        ProfScope ps(b, s, K_GRID);
        hipLaunchKernelGGL(k_grid_sort, dim3(n_images), dim3(256), gridLds, s, b->d_cellOf, b->d_count, b->d_sortedIdx,
                           b->d_cellStart, b->plan.kpCap, image_step);
    }
    LAUNCH_CHECK("k_grid_sort");
    for (int i = 0; i < n_images; i++) b->gridValid[i * image_step] = 1;
    return SD_OK;
}

int sd_batch_download_grid(sd_batch* b, int image, int16_t* cell, int cap)
{
    if (!b || !cell || !slot_ok(b, image)) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int cnt = 0;
    HIPCHK(hipMemcpy(&cnt, b->d_count + image, 4, hipMemcpyDeviceToHost));
    if (cnt > cap) return set_err(SD_ERR_CAPACITY, "grid buffer too small");
    if (cnt > 0) HIPCHK(hipMemcpy(cell, b->d_cellOf + (size_t)image * b->plan.kpCap, (size_t)cnt * 2, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_batch_download_grid_index(sd_batch* b, int image, uint16_t* sorted_idx, int cap, uint16_t* cell_start, int* n_in_grid)
{
    if (!b || !sorted_idx || !cell_start || !n_in_grid || !slot_ok(b, image)) return SD_ERR_INVALID;
    int rc = check_slots(b, "download_grid_index", &image, nullptr, 1, SD_SLOT_GRID);
    if (rc != SD_OK) return rc;
    rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    HIPCHK(hipMemcpy(cell_start, b->d_cellStart + (size_t)image * (SD_GRID_CELLS + 8), (size_t)(SD_GRID_CELLS + 1) * 2, hipMemcpyDeviceToHost));
    const int total = cell_start[SD_GRID_CELLS];
    *n_in_grid = total;
    if (total > cap || total > b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "grid index buffer too small");
    if (total > 0) HIPCHK(hipMemcpy(sorted_idx, b->d_sortedIdx + (size_t)image * b->plan.kpCap, (size_t)total * 2, hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_batch_unproject(sd_batch* b, int first_image, int image_step, int n_frames, const sd_camera* cam, const float* Twc_host,
                       void* stream_)
{
    if (!b || n_frames < 0 || first_image != 0 || image_step < 1 || !cam_ok(cam) || !Twc_host)
        return set_err(SD_ERR_INVALID, "bad unproject arguments");
    if (n_frames > 0 && !slot_ok(b, (n_frames - 1) * image_step)) return set_err(SD_ERR_STATE, "unproject needs extracted images");
    hipStream_t s = pick_stream(b, stream_);
    if (n_frames == 0) return SD_OK;
    HIPCHK(hipMemcpyAsync(b->d_pose, Twc_host, (size_t)n_frames * 64, hipMemcpyHostToDevice, s));
    {
        ProfScope ps(b, s, K_UNPROJ);
        dim3 grd((b->plan.kpCap + 255) / 256, n_frames);
        hipLaunchKernelGGL(k_unproject, grd, dim3(256), 0, s, KPUN(b), b->d_count, b->d_depth, b->d_pose, b->d_xw, b->d_flags,
                           to_cam(cam), b->plan.kpCap, image_step);
    }
    LAUNCH_CHECK("k_unproject");
    return SD_OK;
}

int sd_batch_mappoints_device(sd_batch* b, float** d_xw, uint8_t** d_flags, int* cap)
{
    if (!b) return SD_ERR_INVALID;
    if (d_xw) *d_xw = b->d_xw;
    if (d_flags) *d_flags = b->d_flags;
    if (cap) *cap = b->plan.kpCap;
    return SD_OK;
}

int sd_batch_set_mappoints(sd_batch* b, int image, const float* xw, const uint8_t* flags, int n)
{
    if (!b || image < 0 || image >= b->maxImages || n < 0 || n > b->plan.kpCap || !xw || !flags) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    if (n > 0) {
        HIPCHK(hipMemcpy(b->d_xw + (size_t)image * b->plan.kpCap * 3, xw, (size_t)n * 12, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b->d_flags + (size_t)image * b->plan.kpCap, flags, (size_t)n, hipMemcpyHostToDevice));
    }
    return SD_OK;
}

int sd_batch_download_mappoints(sd_batch* b, int image, float* xw, uint8_t* flags, int cap)
{
    if (!b || !slot_ok(b, image)) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int cnt = 0;
    HIPCHK(hipMemcpy(&cnt, b->d_count + image, 4, hipMemcpyDeviceToHost));
    if (cnt > cap) return set_err(SD_ERR_CAPACITY, "map point buffer too small");
    if (cnt > 0) {
        if (xw) HIPCHK(hipMemcpy(xw, b->d_xw + (size_t)image * b->plan.kpCap * 3, (size_t)cnt * 12, hipMemcpyDeviceToHost));
        if (flags) HIPCHK(hipMemcpy(flags, b->d_flags + (size_t)image * b->plan.kpCap, (size_t)cnt, hipMemcpyDeviceToHost));
    }
    return SD_OK;
}

// pairBase: first pair index of the per-pair arrays this call uses (the tracker keeps TrackHomo's pairs at [0, S) and
// TrackWithMotionModel's at [S, 2S)); d_active / redoBelow: see SdProjArgs; upload: 0 = index and pose arrays of a preceding
// call are reused (the 2*th retry).
static int search_by_projection_impl(sd_batch* b, int pairBase, int n_pairs, const int32_t* cur_index, const int32_t* last_index,
                                     const float* Tcw_host, const float* Tlw_host, const sd_camera* cam, float th, int bMono,
                                     int checkOrientation, const uint8_t* d_occupied, const uint8_t* d_mp_desc, void* stream_,
                                     const int* d_active, int redoBelow, int upload);

int sd_batch_search_by_projection(sd_batch* b, int n_pairs, const int32_t* cur_index, const int32_t* last_index,
                                  const float* Tcw_host, const float* Tlw_host, const sd_camera* cam, float th, int bMono,
                                  int checkOrientation, const uint8_t* d_occupied, const uint8_t* d_mp_desc, void* stream_)
{
    return search_by_projection_impl(b, 0, n_pairs, cur_index, last_index, Tcw_host, Tlw_host, cam, th, bMono, checkOrientation,
                                     d_occupied, d_mp_desc, stream_, nullptr, 0, 1);
}

static int search_by_projection_impl(sd_batch* b, int pairBase, int n_pairs, const int32_t* cur_index, const int32_t* last_index,
                                     const float* Tcw_host, const float* Tlw_host, const sd_camera* cam, float th, int bMono,
                                     int checkOrientation, const uint8_t* d_occupied, const uint8_t* d_mp_desc, void* stream_,
                                     const int* d_active, int redoBelow, int upload)
{
    if (!b || n_pairs < 0 || pairBase < 0 || pairBase + n_pairs > b->maxImages || !cam_ok(cam) || !Tcw_host || !Tlw_host || !(th > 0) ||
        (n_pairs > 0 && (!cur_index || !last_index)))
        return set_err(SD_ERR_INVALID, "bad search_by_projection arguments");
    std::vector<int2> idx(n_pairs);
    int rc = check_slots(b, "search_by_projection", cur_index, last_index, n_pairs, SD_SLOT_RESULTS);
    if (rc != SD_OK) return rc;
    for (int p = 0; p < n_pairs; p++) idx[p] = make_int2(cur_index[p], last_index[p]);
    if (b->plan.kpCap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    hipStream_t s = pick_stream(b, stream_);
    if (pairBase == 0) b->nPairs = 0;
    if (n_pairs == 0) return SD_OK;
    float* dTc = b->d_pose + (size_t)pairBase * 16;
    float* dTl = b->d_pose + ((size_t)b->maxImages + pairBase) * 16;
    int2* dIdx = b->d_pairIdx + pairBase;
    if (upload) {
        HIPCHK(hipMemcpyAsync(dTc, Tcw_host, (size_t)n_pairs * 64, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dTl, Tlw_host, (size_t)n_pairs * 64, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dIdx, idx.data(), (size_t)n_pairs * sizeof(int2), hipMemcpyHostToDevice, s));
    }
    const int cap = b->plan.kpCap;
    const size_t pOff = (size_t)pairBase * cap;
    {
        ProfScope ps(b, s, K_PROJ_A);
        dim3 grd((cap + 15) / 16, n_pairs);                 // 16 points per workgroup: four per wave, 16 lanes each
        SdProjArgs pa;
        pa.kp = KPUN(b); pa.desc = b->d_desc; pa.uRight = b->d_uright; pa.count = b->d_count; pa.cellOf = b->d_cellOf;
        pa.sortedIdx = b->d_sortedIdx; pa.cellStart = b->d_cellStart; pa.xw = b->d_xw; pa.flags = b->d_flags;
        pa.dmp = d_mp_desc ? d_mp_desc : b->d_desc; pa.Tcw = dTc; pa.Tlw = dTl; pa.cand = b->d_pcand + pOff * SD_PROJ_K; pa.ncand = b->d_pncand + pOff;
        pa.errFlag = b->d_err; pa.P = b->d_plan; pa.cam = to_cam(cam); pa.th = th; pa.bMono = bMono; pa.pairIdx = dIdx;
        pa.active = d_active; pa.redoNmatch = b->d_nmatch + pairBase; pa.redoBelow = redoBelow;
        hipLaunchKernelGGL(k_proj_candidates, grd, dim3(256), 0, s, pa);
    }
    LAUNCH_CHECK("k_proj_candidates");
    {
        ProfScope ps(b, s, K_PROJ_B);
        const size_t capA = (size_t)((cap + 15) & ~15);
        size_t lds = capA * (4 + 4 + 4 + 2 + 1 + 1 + 1) + 16;
        if (lds > 160 * 1024 - 256) return set_err(SD_ERR_UNSUPPORTED, "too many keypoints per image for the projection matcher's LDS tables");
        HIPCHK(sd_raise_lds_limit((const void*)k_proj_resolve, (int)lds));
        hipLaunchKernelGGL(k_proj_resolve, dim3(n_pairs), dim3(64), lds, s, KPUN(b), b->d_count, b->d_flags, b->d_pcand + pOff * SD_PROJ_K, b->d_pncand + pOff,
                           d_occupied, b->d_match + pOff, b->d_pairs + pOff * 2, b->d_npairs + pairBase, b->d_nmatch + pairBase, b->d_plan, checkOrientation,
                           dIdx, d_active, redoBelow, b->d_err);
    }
    LAUNCH_CHECK("k_proj_resolve");
    if (pairBase == 0) b->nPairs = n_pairs;
    b->dlPairs = std::max(pairBase + n_pairs, pairBase ? b->dlPairs : 0);
    if (b->pairCam.size() != (size_t)b->maxImages) b->pairCam.assign(b->maxImages, sd_camera());
    for (int p = 0; p < n_pairs; p++) b->pairCam[pairBase + p] = *cam;
    return SD_OK;
}

// Tracking::SearchLocalPoints (Tracking.cc:2014-2064): Frame::isInFrustum for every local map point, then
// ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (ORBmatcher.cc:45-129).
int sd_batch_search_local_map(sd_batch* b, int n_frames, const int32_t* frame_index, const int32_t* point_offset,
                              const sd_map_point* d_points, const uint8_t* d_point_desc, const float* Tcw_host,
                              const sd_camera* cam, float th, float nnratio, float viewing_cos_limit,
                              const uint8_t* d_occupied, sd_track_info* d_track, int32_t* d_point_match,
                              int32_t* d_kp_match, int32_t* d_nmatches, void* stream_)
{
    if (!b || n_frames < 0 || n_frames > b->maxImages || !cam_ok(cam) || !(th > 0) ||
        (n_frames > 0 && (!frame_index || !point_offset || !Tcw_host || !d_track || !d_point_match || !d_kp_match || !d_nmatches)))
        return set_err(SD_ERR_INVALID, "bad search_local_map arguments");
    if (n_frames == 0) return SD_OK;
    int maxM = 0, rc = SD_OK;
    // frame by frame, the slot and then the ranges up to this frame: a call wrong in both ways gets the code of its first wrong frame
    for (int f = 0; f < n_frames && rc == SD_OK; f++) {
        rc = check_slots(b, "search_local_map", frame_index + f, nullptr, 1, SD_SLOT_RESULTS);
        if (rc == SD_OK) rc = check_offsets("search_local_map", point_offset, f + 1, &maxM);
    }
    if (rc != SD_OK) return rc;
    const int total = point_offset[n_frames];
    if (total > 0 && (!d_points || !d_point_desc)) return set_err(SD_ERR_INVALID, "search_local_map: no map points given");
    if (b->plan.kpCap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    hipStream_t s = pick_stream(b, stream_);
    if (!b->localMap.d_idx) HIPCHK(b->localMap.d_idx.alloc((size_t)(2 * b->maxImages + 2) * sizeof(int)));
    rc = b->localMap.grow(b, s, total);
    if (rc != SD_OK) return rc;
    int* dFrameOf = b->localMap.d_idx;
    int* dOff = b->localMap.d_idx + b->maxImages;
    HIPCHK(hipMemcpyAsync(dFrameOf, frame_index, (size_t)n_frames * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dOff, point_offset, (size_t)(n_frames + 1) * 4, hipMemcpyHostToDevice, s));
    float* dT = b->d_pose;
    HIPCHK(hipMemcpyAsync(dT, Tcw_host, (size_t)n_frames * 64, hipMemcpyHostToDevice, s));
    const int cap = b->plan.kpCap;
    if (maxM > 0) {
        ProfScope ps(b, s, K_LOCAL_A);
        hipLaunchKernelGGL(k_local_candidates, dim3((maxM + 3) / 4, n_frames), dim3(256), 0, s, KPUN(b), b->d_desc, b->d_uright, b->d_count,
                           b->d_cellOf, b->d_sortedIdx, b->d_cellStart, (const SdMapPoint*)d_points, d_point_desc, dFrameOf, dOff, dT,
                           (SdTrack*)d_track, b->localMap.d_cand, b->localMap.d_n, b->localMap.d_ovf, b->d_plan, to_cam(cam), th, viewing_cos_limit);
        LAUNCH_CHECK("k_local_candidates");
    }
    {
        ProfScope ps(b, s, K_LOCAL_B);
        const size_t lds = (size_t)cap * 4 + cap + 16;
        hipLaunchKernelGGL(k_local_resolve, dim3(n_frames), dim3(64), lds, s, KPUN(b), b->d_count, (const SdMapPoint*)d_points, dFrameOf, dOff,
                           b->localMap.d_cand, b->localMap.d_n, b->localMap.d_ovf, d_occupied, d_point_match, d_kp_match, d_nmatches, b->d_err, b->d_plan, nnratio);
        LAUNCH_CHECK("k_local_resolve");
    }
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Vocabulary (Thirdparty/DBoW2 TemplatedVocabulary) and the bag-of-words matcher
// ---------------------------------------------------------------------------------------------------------
static int require_device()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return set_err(SD_ERR_NO_DEVICE, "no HIP device: the vocabulary lives in HBM, there is no CPU fallback");
    return SD_OK;
}

static int vocab_from_lines(sd_vocab** out, const SdVocabLines& lines)
{
    std::vector<uint8_t> blob;
    if (!vocab_pack(lines, blob)) return set_err(SD_ERR_INVALID, "vocabulary: a node names a parent that does not precede it");
    sd_vocab* v = new sd_vocab();
    memcpy(&v->h, blob.data(), sizeof(SdVocabHeader));
    if (v->owned.alloc(blob.size()) != hipSuccess) { delete v; return set_err(SD_ERR_HIP, "hipMalloc(vocabulary)"); }
    v->d_blob = v->owned;
    if (hipMemcpy(v->d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) { delete v; return set_err(SD_ERR_HIP, "hipMemcpy(vocabulary)"); }
    vocab_bind(v);
    *out = v;
    return SD_OK;
}

int sd_vocab_load_text(sd_vocab** out, const char* path)
{
    if (!out || !path) return set_err(SD_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc = require_device();
    if (rc != SD_OK) return rc;
    SdVocabLines lines;
    std::string err;
    if (!vocab_parse_text(path, lines, err)) return set_err(SD_ERR_INVALID, err);
    return vocab_from_lines(out, lines);
}

int sd_vocab_from_nodes(sd_vocab** out, int k, int L, int scoring, int weighting, int n_lines, const int32_t* parent,
                        const uint8_t* is_leaf, const uint8_t* desc, const double* weight)
{
    if (!out || n_lines < 0 || (n_lines > 0 && (!parent || !is_leaf || !desc || !weight))) return set_err(SD_ERR_INVALID, "null argument");
    *out = nullptr;
    if (k < 0 || k > 20 || L < 1 || L > 10 || scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3)
        return set_err(SD_ERR_INVALID, "Vocabulary loading failure: This is not a correct text file!");
    int rc = require_device();
    if (rc != SD_OK) return rc;
    SdVocabLines lines;
    lines.k = k; lines.L = L; lines.scoring = scoring; lines.weighting = weighting;
    lines.parent.assign(parent, parent + n_lines); lines.isLeaf.assign(is_leaf, is_leaf + n_lines);
    lines.desc.assign(desc, desc + (size_t)n_lines * 32); lines.weight.assign(weight, weight + n_lines);
    return vocab_from_lines(out, lines);
}

int sd_vocab_from_packed_device(sd_vocab** out, void* d_blob, size_t bytes)
{
    if (!out || !d_blob || bytes < sizeof(SdVocabHeader)) return set_err(SD_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc = require_device();
    if (rc != SD_OK) return rc;
    SdVocabHeader h;
    HIPCHK(hipMemcpy(&h, d_blob, sizeof(h), hipMemcpyDeviceToHost));
    SdVocabHeader chk = h;
    if (h.magic != SD_VOCAB_MAGIC || h.version != 1 || vocab_layout(chk) != h.totalBytes || h.totalBytes > bytes ||
        chk.offWordId != h.offWordId || chk.offDesc != h.offDesc)
        return set_err(SD_ERR_INVALID, "not a packed vocabulary");
    sd_vocab* v = new sd_vocab();
    v->h = h; v->d_blob = d_blob;
    vocab_bind(v);
    *out = v;
    return SD_OK;
}

void sd_vocab_destroy(sd_vocab* v) { delete v; }

int sd_vocab_info(const sd_vocab* v, int* k, int* L, int* scoring, int* weighting, int* n_nodes, int* n_words)
{
    if (!v) return SD_ERR_INVALID;
    if (k) *k = (int)v->h.k; if (L) *L = (int)v->h.L; if (scoring) *scoring = (int)v->h.scoring; if (weighting) *weighting = (int)v->h.weighting;
    if (n_nodes) *n_nodes = (int)v->h.nNodes; if (n_words) *n_words = (int)v->h.nWords;
    return SD_OK;
}

int sd_vocab_packed_device(sd_vocab* v, void** d_blob, size_t* bytes)
{
    if (!v) return SD_ERR_INVALID;
    if (d_blob) *d_blob = v->d_blob;
    if (bytes) *bytes = (size_t)v->h.totalBytes;
    return SD_OK;
}

size_t sd_vocab_packed_bytes(int n_nodes)
{
    SdVocabHeader h = {};
    h.nNodes = (uint32_t)(n_nodes < 0 ? 0 : n_nodes);
    return vocab_layout(h);
}

int sd_vocab_download_nodes(const sd_vocab* v, int32_t* parent, int32_t* n_children, int32_t* word_id, uint8_t* desc, double* weight)
{
    if (!v) return SD_ERR_INVALID;
    const int n = (int)v->h.nNodes;
    const uint8_t* p = (const uint8_t*)v->d_blob;
    if (parent) HIPCHK(hipMemcpy(parent, p + v->h.offParent, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (word_id) HIPCHK(hipMemcpy(word_id, p + v->h.offWordId, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (desc) HIPCHK(hipMemcpy(desc, p + v->h.offDesc, (size_t)n * 32, hipMemcpyDeviceToHost));
    if (weight) HIPCHK(hipMemcpy(weight, p + v->h.offWeight, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (n_children) {
        std::vector<int> cs(n + 1);
        HIPCHK(hipMemcpy(cs.data(), p + v->h.offChildStart, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) n_children[i] = cs[i + 1] - cs[i];
    }
    return SD_OK;
}

static int ensure_bow(sd_batch* b)
{
    if (b->d_bowWordF) return SD_OK;
    const size_t nI = b->maxImages, cap = b->plan.kpCap;
    SdDevBuf<unsigned> wordF, nidF, fvNode, fvFeat, fvRunNode, word; SdDevBuf<double> wF, val; SdDevBuf<int> fvRunStart, meta, img;
    HIPCHK(wordF.alloc(nI * cap * 4)); HIPCHK(wF.alloc(nI * cap * 8)); HIPCHK(nidF.alloc(nI * cap * 4)); HIPCHK(fvNode.alloc(nI * cap * 4));
    HIPCHK(fvFeat.alloc(nI * cap * 4)); HIPCHK(fvRunStart.alloc(nI * (cap + 1) * 4)); HIPCHK(fvRunNode.alloc(nI * cap * 4)); HIPCHK(word.alloc(nI * cap * 4));
    HIPCHK(val.alloc(nI * cap * 8)); HIPCHK(meta.alloc(nI * 4 * 4)); HIPCHK(img.alloc(nI * 4));
    HIPCHK(hipMemset(meta, 0, nI * 16));
    b->d_bowWF = std::move(wF); b->d_bowNidF = std::move(nidF); b->d_fvNode = std::move(fvNode); b->d_fvFeat = std::move(fvFeat); b->d_fvRunStart = std::move(fvRunStart);
    b->d_fvRunNode = std::move(fvRunNode); b->d_bowWord = std::move(word); b->d_bowVal = std::move(val); b->d_bowMeta = std::move(meta); b->d_bowImg = std::move(img);
    b->bowValid.assign(nI, 0);
    b->d_bowWordF = std::move(wordF);           // last: it marks the group as present
    return SD_OK;
}

// Frame::ComputeBoW (src/Frame.cc:803-810) for the listed image slots.
int sd_batch_compute_bow(sd_batch* b, const sd_vocab* v, int n_images, const int32_t* image_index, int levelsup, void* stream_)
{
    if (!b || !v || n_images < 0 || n_images > b->maxImages || (n_images > 0 && !image_index) || levelsup < 0)
        return set_err(SD_ERR_INVALID, "bad compute_bow arguments");
    if (v->h.nNodes <= 1) return set_err(SD_ERR_INVALID, "compute_bow: empty vocabulary");
    int rc = check_slots(b, "compute_bow", image_index, nullptr, n_images, SD_SLOT_RESULTS);
    if (rc != SD_OK) return rc;
    const int cap = b->plan.kpCap;
    int sortN = 256;                     // LDS capacity of k_bow_finalize's sort: its per-image sort size starts at 256 too
    while (sortN < cap) sortN <<= 1;
    if (sortN > 8192) return set_err(SD_ERR_UNSUPPORTED, "compute_bow: more than 8192 keypoints per image");
    rc = ensure_bow(b);
    if (rc != SD_OK) return rc;
    hipStream_t s = pick_stream(b, stream_);
    if (n_images == 0) return SD_OK;
    HIPCHK(hipMemcpyAsync(b->d_bowImg, image_index, (size_t)n_images * 4, hipMemcpyHostToDevice, s));
    {
        ProfScope ps(b, s, K_BOW_T);
        hipLaunchKernelGGL(k_bow_transform, dim3((cap + 15) / 16, n_images), dim3(256), 0, s, b->d_desc, b->d_count, b->d_bowImg, v->dev, levelsup, cap,
                           b->d_bowWordF, b->d_bowWF, b->d_bowNidF);
        LAUNCH_CHECK("k_bow_transform");
    }
    {
        ProfScope ps(b, s, K_BOW_F);
        const size_t lds = (size_t)sortN * 8 + 257 * 4 + 16;
        hipLaunchKernelGGL(k_bow_finalize, dim3(n_images), dim3(256), lds, s, b->d_count, b->d_bowImg, b->d_bowWordF, b->d_bowWF, b->d_bowNidF, cap, sortN,
                           (int)v->h.scoring, (int)v->h.weighting, b->d_fvNode, b->d_fvFeat, b->d_fvRunStart, b->d_fvRunNode, b->d_bowWord,
                           b->d_bowVal, b->d_bowMeta);
        LAUNCH_CHECK("k_bow_finalize");
    }
    for (int i = 0; i < n_images; i++) b->bowValid[image_index[i]] = 1;
    return SD_OK;
}

int sd_batch_bow_device(sd_batch* b, uint32_t** d_bow_word, double** d_bow_value, uint32_t** d_fv_node, uint32_t** d_fv_feature,
                        int32_t** d_meta, int* cap)
{
    if (!b) return SD_ERR_INVALID;
    int rc = ensure_bow(b);
    if (rc != SD_OK) return rc;
    if (d_bow_word) *d_bow_word = b->d_bowWord; if (d_bow_value) *d_bow_value = b->d_bowVal;
    if (d_fv_node) *d_fv_node = b->d_fvNode; if (d_fv_feature) *d_fv_feature = b->d_fvFeat;
    if (d_meta) *d_meta = b->d_bowMeta; if (cap) *cap = b->plan.kpCap;
    return SD_OK;
}

int sd_batch_download_bow(sd_batch* b, int image, uint32_t* bow_word, double* bow_value, int* n_words, uint32_t* fv_node,
                          uint32_t* fv_feature, int* n_features, uint32_t* feature_word, double* feature_weight, uint32_t* feature_node, int cap)
{
    if (!b || image < 0 || image >= b->maxImages) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    if (!b->d_bowWordF || !b->bowValid[image]) return set_err(SD_ERR_STATE, "download_bow: no bag of words computed for this slot");
    int meta[4];
    HIPCHK(hipMemcpy(meta, b->d_bowMeta + image * 4, 16, hipMemcpyDeviceToHost));
    int cnt = 0;
    HIPCHK(hipMemcpy(&cnt, b->d_count + image, 4, hipMemcpyDeviceToHost));
    if (cnt > cap) return set_err(SD_ERR_CAPACITY, "bow buffer too small");
    const size_t off = (size_t)image * b->plan.kpCap;
    if (n_words) *n_words = meta[2];
    if (n_features) *n_features = meta[0];
    if (meta[2] > 0) {
        if (bow_word) HIPCHK(hipMemcpy(bow_word, b->d_bowWord + off, (size_t)meta[2] * 4, hipMemcpyDeviceToHost));
        if (bow_value) HIPCHK(hipMemcpy(bow_value, b->d_bowVal + off, (size_t)meta[2] * 8, hipMemcpyDeviceToHost));
    }
    if (meta[0] > 0) {
        if (fv_node) HIPCHK(hipMemcpy(fv_node, b->d_fvNode + off, (size_t)meta[0] * 4, hipMemcpyDeviceToHost));
        if (fv_feature) HIPCHK(hipMemcpy(fv_feature, b->d_fvFeat + off, (size_t)meta[0] * 4, hipMemcpyDeviceToHost));
    }
    if (cnt > 0) {
        if (feature_word) HIPCHK(hipMemcpy(feature_word, b->d_bowWordF + off, (size_t)cnt * 4, hipMemcpyDeviceToHost));
        if (feature_weight) HIPCHK(hipMemcpy(feature_weight, b->d_bowWF + off, (size_t)cnt * 8, hipMemcpyDeviceToHost));
        if (feature_node) HIPCHK(hipMemcpy(feature_node, b->d_bowNidF + off, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    }
    return SD_OK;
}

// ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (src/ORBmatcher.cc:159-288)
int sd_batch_search_by_bow(sd_batch* b, int n_pairs, const int32_t* kf_index, const int32_t* frame_index, const uint8_t* d_kf_valid,
                           float nnratio, int checkOrientation, void* stream_)
{
    if (!b || n_pairs < 0 || n_pairs > b->maxImages || (n_pairs > 0 && (!kf_index || !frame_index)))
        return set_err(SD_ERR_INVALID, "bad search_by_bow arguments");
    std::vector<int2> idx(n_pairs);
    int rc = check_slots(b, "search_by_bow", kf_index, frame_index, n_pairs, SD_SLOT_RESULTS | SD_SLOT_BOW);
    if (rc != SD_OK) return rc;
    for (int p = 0; p < n_pairs; p++) idx[p] = make_int2(kf_index[p], frame_index[p]);
    hipStream_t s = pick_stream(b, stream_);
    b->nPairs = 0; b->dlPairs = 0;
    if (n_pairs == 0) return SD_OK;
    HIPCHK(hipMemcpyAsync(b->d_pairIdx, idx.data(), (size_t)n_pairs * sizeof(int2), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(b->d_npairs, 0, (size_t)n_pairs * 4, s));
    const int cap = b->plan.kpCap;
    {
        ProfScope ps(b, s, K_BOW_S);
        const size_t lds = (size_t)cap * 4 + cap + 16;
        hipLaunchKernelGGL(k_search_by_bow, dim3(n_pairs), dim3(64 * SD_BOW_WAVES), lds, s, b->d_kp, b->d_desc, b->d_count, b->d_fvFeat, b->d_fvRunStart, b->d_fvRunNode,
                           b->d_bowMeta, d_kf_valid, b->d_pairIdx, cap, nnratio, checkOrientation, b->d_match, b->d_nmatch);
        LAUNCH_CHECK("k_search_by_bow");
    }
    b->nPairs = n_pairs; b->dlPairs = n_pairs;
    return SD_OK;
}

// ---------------------------------------------------------------- SearchForTriangulation / CreateNewMapPoints (k_triangulate.h)
// Everything the reference derives from the two poses alone, as cv::Mat forms it (every small product accumulates in
// double, k ascending, and narrows once).
namespace {
inline float tri_acc3(const float* a, int sa, const float* b, int sb, bool neg = false, const float* add = nullptr)
{
    double s = 0.0;
    for (int k = 0; k < 3; k++) s += (double)(neg ? -a[k * sa] : a[k * sa]) * (double)b[k * sb];
    if (add) s += (double)*add;
    return (float)s;
}
inline void tri_mul33(const float* A, const float* B, float* C)      // C = A * B, row-major 3x3
{
    float out[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) out[i * 3 + j] = tri_acc3(A + i * 3, 1, B + j, 3);
    memcpy(C, out, sizeof(out));
}
// KeyFrame::SetPose: Ow = -Rwc * tcw (KeyFrame.cc:70-84)
inline void tri_center(const float* T /*4x4*/, float* Ow)
{
    const float t[3] = {T[3], T[7], T[11]};
    for (int i = 0; i < 3; i++) Ow[i] = tri_acc3(T + i, 4, t, 1, true);       // row i of Rwc = column i of Rcw
}
// false = the neighbour is skipped by the baseline rule (LocalMapping.cc:245-262)
inline void tri_pair_setup(const float* Tcw1, const float* Tcw2, const sd_camera& cam, const float* medianDepth, bool baselineRule, SdTriPair& P)
{
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) { P.T1[r * 4 + c] = Tcw1[r * 4 + c]; P.T2[r * 4 + c] = Tcw2[r * 4 + c]; }
    tri_center(Tcw1, P.Ow1); tri_center(Tcw2, P.Ow2);
    P.skip = 0;
    if (baselineRule) {
        const float bx = P.Ow2[0] - P.Ow1[0], by = P.Ow2[1] - P.Ow1[1], bz = P.Ow2[2] - P.Ow1[2];
        double ss = (double)bx * (double)bx; ss += (double)by * (double)by; ss += (double)bz * (double)bz;
        const float baseline = (float)std::sqrt(ss);
        if (!medianDepth) { if (baseline < cam.mb) P.skip = 1; }
        else { const float ratio = baseline / *medianDepth; if ((double)ratio < 0.01) P.skip = 1; }
    }
    float R1[9], R2[9], R2t[9], t1[3], t2[3];
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) { R1[r * 3 + c] = Tcw1[r * 4 + c]; R2[r * 3 + c] = Tcw2[r * 4 + c]; R2t[c * 3 + r] = Tcw2[r * 4 + c]; } t1[r] = Tcw1[r * 4 + 3]; t2[r] = Tcw2[r * 4 + 3]; }
    // ComputeF12 (LocalMapping.cc:537-554)
    float R12[9], t12[3];
    tri_mul33(R1, R2t, R12);
    for (int i = 0; i < 3; i++) t12[i] = tri_acc3(R12 + i * 3, 1, t2, 1, true, &t1[i]);
    const float t12x[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};
    const float ifx = (float)(1.0 / (double)cam.fx), ify = (float)(1.0 / (double)cam.fy);
    const float icx = (float)(-(double)cam.cx / (double)cam.fx), icy = (float)(-(double)cam.cy / (double)cam.fy);
    const float Kinv[9] = {ifx, 0.f, icx, 0.f, ify, icy, 0.f, 0.f, 1.f};
    const float KinvT[9] = {ifx, 0.f, 0.f, 0.f, ify, 0.f, icx, icy, 1.f};
    float M[9];
    tri_mul33(KinvT, t12x, M); tri_mul33(M, R12, M); tri_mul33(M, Kinv, P.F12);
    // the epipole of KF1's centre in KF2 (ORBmatcher.cc:820-827)
    float C2[3];
    for (int i = 0; i < 3; i++) C2[i] = tri_acc3(R2 + i * 3, 1, P.Ow1, 1, false, &t2[i]);
    const float invz = 1.0f / C2[2];
    P.ex = cam.fx * C2[0] * invz + cam.cx;
    P.ey = cam.fy * C2[1] * invz + cam.cy;
}
// the per-level tables of the kernels that take them by value (k_tri_match, k_tri_triangulate, k_fuse_search): 1.f beyond nlevels
SdLevelTables level_tables(const sd_batch* b)
{
    const SdParams& prm = b->ex->prm;
    SdLevelTables L;
    for (int l = 0; l < SD_MAX_LEVELS; l++) { const bool in = l < prm.nlevels; L.scale[l] = in ? prm.scale[l] : 1.f; L.sigma2[l] = in ? prm.sigma2[l] : 1.f; L.invSigma2[l] = in ? prm.invSigma2[l] : 1.f; }
    L.nlevels = prm.nlevels;
    return L;
}
int tri_launch_match(sd_batch* b, int n, const uint8_t* h1, const uint8_t* h2, int onlyStereo, int checkOrientation, int* match, int* pairs,
                     int* np, int* nm, hipStream_t s)
{
    const int cap = b->plan.kpCap;
    const size_t lds = (size_t)cap * 4 + SD_TRI_THREADS * 4 + cap + 16;
    if (lds > 64 * 1024) HIPCHK(sd_raise_lds_limit((const void*)k_tri_match, (int)lds));
    ProfScope ps(b, s, K_TRI_M);
    hipLaunchKernelGGL(k_tri_match, dim3(n), dim3(SD_TRI_THREADS), lds, s, KPUN(b), b->d_desc, b->d_uright, b->d_count, b->d_fvFeat, b->d_fvRunStart,
                       b->d_fvRunNode, b->d_bowMeta, h1, h2, b->tri.d_pairs, level_tables(b), cap, onlyStereo, checkOrientation, match, pairs, np, nm);
    LAUNCH_CHECK("k_tri_match");
    return SD_OK;
}
}

// ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (src/ORBmatcher.cc:814-980)
int sd_batch_search_for_triangulation(sd_batch* b, int n_pairs, const int32_t* kf1_index, const int32_t* kf2_index, const float* Tcw1_host,
                                      const float* Tcw2_host, const sd_camera* cam, const uint8_t* d_has_mp1, const uint8_t* d_has_mp2,
                                      int only_stereo, int check_orientation, void* stream_)
{
    if (!b || n_pairs <= 0 || n_pairs > b->maxImages || !cam_ok(cam) || !kf1_index || !kf2_index || !Tcw1_host || !Tcw2_host)
        return set_err(SD_ERR_INVALID, "bad search_for_triangulation arguments");
    int rc = check_slots(b, "search_for_triangulation", kf1_index, kf2_index, n_pairs, SD_SLOT_RANGE | SD_SLOT_RESULTS | SD_SLOT_BOW);
    if (rc != SD_OK) return rc;
    if (b->plan.kpCap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    hipStream_t s = pick_stream(b, stream_);
    b->nPairs = 0; b->dlPairs = 0;
    std::vector<SdTriPair>& P = b->tri.hostPairs;
    P.resize(n_pairs);
    for (int p = 0; p < n_pairs; p++) {
        P[p].img1 = kf1_index[p]; P[p].img2 = kf2_index[p]; P[p].row1 = p; P[p].row2 = p;
        tri_pair_setup(Tcw1_host + 16 * (size_t)p, Tcw2_host + 16 * (size_t)p, *cam, nullptr, false, P[p]);
    }
    rc = b->tri.growPairs(b, s, n_pairs);
    if (rc != SD_OK) return rc;
    HIPCHK(hipMemcpyAsync(b->tri.d_pairs, P.data(), (size_t)n_pairs * sizeof(SdTriPair), hipMemcpyHostToDevice, s));
    rc = tri_launch_match(b, n_pairs, d_has_mp1, d_has_mp2, only_stereo != 0, check_orientation != 0, b->d_match, b->d_pairs, b->d_npairs, b->d_nmatch, s);
    if (rc != SD_OK) return rc;
    b->nPairs = n_pairs; b->dlPairs = n_pairs;
    return SD_OK;
}

// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:208-453) for n_kf keyframes and their neighbour lists
int sd_batch_create_new_map_points(sd_batch* b, int n_kf, const int32_t* kf_index, const float* kf_Tcw_host, const uint8_t* d_kf_has_mp,
                                   const int32_t* neigh_offset, const int32_t* neigh_index, const float* neigh_Tcw_host,
                                   const float* neigh_median_depth, const uint8_t* d_neigh_has_mp, const sd_camera* cam,
                                   sd_new_map_point** d_new, int32_t** d_nnew, void* stream_)
{
    if (!b || n_kf <= 0 || !cam_ok(cam) || !kf_index || !kf_Tcw_host || !neigh_offset)
        return set_err(SD_ERR_INVALID, "bad create_new_map_points arguments");
    int rc = check_offsets("create_new_map_points", neigh_offset, n_kf, nullptr);
    if (rc != SD_OK) return rc;
    const int nP = neigh_offset[n_kf];
    if (nP > 0 && (!neigh_index || !neigh_Tcw_host)) return set_err(SD_ERR_INVALID, "bad create_new_map_points arguments");
    rc = check_slots(b, "create_new_map_points", kf_index, nullptr, n_kf, SD_SLOT_RANGE | SD_SLOT_RESULTS | SD_SLOT_BOW);
    if (rc == SD_OK) rc = check_slots(b, "create_new_map_points", neigh_index, nullptr, nP, SD_SLOT_RANGE | SD_SLOT_RESULTS | SD_SLOT_BOW);
    if (rc != SD_OK) return rc;
    if (b->plan.kpCap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    hipStream_t s = pick_stream(b, stream_);
    b->tri.kfs = 0;
    if (d_new) *d_new = nullptr;
    if (d_nnew) *d_nnew = nullptr;
    const size_t cap = b->plan.kpCap;
    rc = b->tri.growTables(b, s, n_kf, nP);
    if (rc != SD_OK) return rc;
    HIPCHK(hipMemcpyAsync(b->tri.d_off, neigh_offset, ((size_t)n_kf + 1) * 4, hipMemcpyHostToDevice, s));
    if (nP > 0) {
        std::vector<SdTriPair>& P = b->tri.hostPairs;
        P.resize(nP);
        for (int k = 0; k < n_kf; k++)
            for (int p = neigh_offset[k]; p < neigh_offset[k + 1]; p++) {
                P[p].img1 = kf_index[k]; P[p].img2 = neigh_index[p]; P[p].row1 = k; P[p].row2 = p;
                tri_pair_setup(kf_Tcw_host + 16 * (size_t)k, neigh_Tcw_host + 16 * (size_t)p, *cam, neigh_median_depth ? neigh_median_depth + p : nullptr, true, P[p]);
            }
        rc = b->tri.growPairs(b, s, nP);
        if (rc != SD_OK) return rc;
        HIPCHK(hipMemcpyAsync(b->tri.d_pairs, P.data(), (size_t)nP * sizeof(SdTriPair), hipMemcpyHostToDevice, s));
        rc = tri_launch_match(b, nP, d_kf_has_mp, d_neigh_has_mp, 0, 0, b->tri.d_match, b->tri.d_pairList, b->tri.d_np, nullptr, s);   // ORBmatcher(0.6, false), bOnlyStereo = false
        if (rc != SD_OK) return rc;
        SdCamera c; memcpy(&c, cam, sizeof(c));
        const float ratioFactor = 1.5f * (float)b->ex->prm.scaleFactor;
        HIPCHK(hipMemsetAsync(b->tri.d_ok, 0, (size_t)nP * cap, s));
        ProfScope ps(b, s, K_TRI_T);
        hipLaunchKernelGGL(k_tri_triangulate, dim3((unsigned)((cap + 255) / 256), nP), dim3(256), 0, s, KPUN(b), b->d_kp, b->d_uright, b->d_depth,
                           b->tri.d_pairs, b->tri.d_pairList, b->tri.d_np, level_tables(b), c, ratioFactor, (int)cap, b->tri.d_ok, b->tri.d_xw);
        LAUNCH_CHECK("k_tri_triangulate");
    }
    {
        const size_t lds = cap + 16;
        ProfScope ps(b, s, K_TRI_R);
        hipLaunchKernelGGL(k_tri_resolve, dim3(n_kf), dim3(256), lds, s, b->d_count, b->tri.d_pairs, b->tri.d_off, b->tri.d_match, b->tri.d_ok, b->tri.d_xw, (int)cap,
                           b->tri.d_new.get(), b->tri.d_nnew);
        LAUNCH_CHECK("k_tri_resolve");
    }
    b->tri.kfs = n_kf;
    if (d_new) *d_new = b->tri.d_new;
    if (d_nnew) *d_nnew = b->tri.d_nnew;
    return SD_OK;
}

int sd_batch_download_new_map_points(sd_batch* b, int kf, sd_new_map_point* out, int cap, int* nnew)
{
    if (!b || !nnew) return set_err(SD_ERR_INVALID, "bad download_new_map_points arguments");
    if (kf < 0 || kf >= b->tri.kfs) return set_err(SD_ERR_INVALID, "download_new_map_points: no such keyframe in the last sd_batch_create_new_map_points");
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int n = 0;
    HIPCHK(hipMemcpy(&n, b->tri.d_nnew + kf, 4, hipMemcpyDeviceToHost));
    *nnew = n;
    if (n > cap) return set_err(SD_ERR_CAPACITY, "new map point buffer too small");
    if (out && n > 0) HIPCHK(hipMemcpy(out, b->tri.d_new + (size_t)kf * b->plan.kpCap, (size_t)n * sizeof(sd_new_map_point), hipMemcpyDeviceToHost));
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// LocalMapping::SearchInNeighbors: ORBmatcher::Fuse(pKF, vpMapPoints, th) and MapPoint::ComputeDistinctiveDescriptors (k_fuse.h)
// ---------------------------------------------------------------------------------------------------------
// sim3 = the job's pose is a similarity Scw (ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)): decomposed here (sd_scw.h), searched
// by k_loop_search<0>; the tail is the same k_fuse_resolve
static int fuse_impl(sd_batch* b, int n_jobs, const int32_t* kf_index, const float* Tcw_host, const int32_t* cand_offset,
                     const int32_t* d_cand_point, const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points,
                     const uint8_t* d_kf_state, const sd_camera* cam, float th, int32_t** d_best, sd_fuse_hit** d_hits,
                     int32_t** d_nfused, void* stream_, bool sim3)
{
    static_assert(sizeof(SdFuseHit) == sizeof(sd_fuse_hit) && sizeof(sd_fuse_hit) == 20, "sd_fuse_hit is 20 bytes");
    if (d_best) *d_best = nullptr;
    if (d_hits) *d_hits = nullptr;
    if (d_nfused) *d_nfused = nullptr;
    if (!b || n_jobs < 0 || n_jobs > 65535 || n_points < 0 || !cam_ok(cam) || !(th > 0) || (n_jobs > 0 && (!kf_index || !Tcw_host || !cand_offset)))
        return set_err(SD_ERR_INVALID, "bad fuse arguments");
    b->fuse.jobs = 0;
    if (n_jobs == 0) return SD_OK;
    int maxM = 0;
    int rc = check_offsets("fuse", cand_offset, n_jobs, &maxM);
    if (rc == SD_OK) rc = check_slots(b, "fuse", kf_index, nullptr, n_jobs, SD_SLOT_RANGE);
    if (rc == SD_OK) rc = check_slots(b, "fuse", kf_index, nullptr, n_jobs, SD_SLOT_RESULTS | SD_SLOT_GRID);
    if (rc != SD_OK) return rc;
    const int total = cand_offset[n_jobs];
    if (total > 0 && (!d_cand_point || !d_points || !d_point_desc || n_points == 0)) return set_err(SD_ERR_INVALID, "fuse: entries but no map points given");
    const int cap = b->plan.kpCap;
    if (cap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    hipStream_t s = pick_stream(b, stream_);
    // the first-taker table of k_fuse_resolve: [cap] ints in LDS while that fits beside the scan, else one row per job in memory
    const size_t lds = (size_t)cap * 4 + 16;
    const bool firstInMemory = lds > SD_LDS_MAX_BYTES - 2048;
    rc = b->fuse.grow(b, s, n_jobs, total, firstInMemory);
    if (rc != SD_OK) return rc;
    int* dFrameOf = b->fuse.d_jobs;
    int* dOff = b->fuse.d_jobs + n_jobs;
    b->fuse.off.assign(cand_offset, cand_offset + n_jobs + 1);
    HIPCHK(hipMemcpyAsync(dFrameOf, kf_index, (size_t)n_jobs * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dOff, cand_offset, ((size_t)n_jobs + 1) * 4, hipMemcpyHostToDevice, s));
    if (sim3) {
        b->loop.T.resize((size_t)n_jobs * 16);
        for (int j = 0; j < n_jobs; j++) sd_scw_decompose(Tcw_host + (size_t)j * 16, b->loop.T.data() + (size_t)j * 16);
        Tcw_host = b->loop.T.data();
    }
    HIPCHK(hipMemcpyAsync(b->fuse.d_T, Tcw_host, (size_t)n_jobs * 64, hipMemcpyHostToDevice, s));
    if (maxM > 0 && sim3) {
        ProfScope ps(b, s, K_LOOP_F);
        hipLaunchKernelGGL(k_loop_search<0>, dim3((maxM + 3) / 4, n_jobs), dim3(256), 0, s, KPUN(b), b->d_desc, b->d_uright, b->d_sortedIdx, b->d_cellStart,
                           b->d_count, (const SdMapPoint*)d_points, d_point_desc, n_points, dFrameOf, dOff, d_cand_point, b->fuse.d_T, (const int*)nullptr,
                           b->fuse.d_best.get(), (unsigned*)nullptr, (int*)nullptr, b->fuse.d_err.get(), level_tables(b), to_cam(cam), th, cap);
        LAUNCH_CHECK("k_loop_search<0>");
    } else if (maxM > 0) {
        ProfScope ps(b, s, K_FUSE_S);
        hipLaunchKernelGGL(k_fuse_search, dim3((maxM + 3) / 4, n_jobs), dim3(256), 0, s, KPUN(b), b->d_desc, b->d_uright, b->d_sortedIdx, b->d_cellStart,
                           (const SdMapPoint*)d_points, d_point_desc, n_points, dFrameOf, dOff, d_cand_point, b->fuse.d_T, b->fuse.d_best.get(),
                           b->fuse.d_err.get(), level_tables(b), to_cam(cam), th, cap);
        LAUNCH_CHECK("k_fuse_search");
    }
    {
        if (!firstInMemory && lds > 64 * 1024) HIPCHK(sd_raise_lds_limit((const void*)k_fuse_resolve, (int)lds));
        ProfScope ps(b, s, K_FUSE_R);
        hipLaunchKernelGGL(k_fuse_resolve, dim3(n_jobs), dim3(256), firstInMemory ? 0 : lds, s, b->d_count, dFrameOf, dOff, b->fuse.d_best.get(), d_kf_state, cap,
                           firstInMemory ? b->fuse.d_first.get() : nullptr, b->fuse.d_hits.get(), b->fuse.d_n.get());
        LAUNCH_CHECK("k_fuse_resolve");
    }
    b->fuse.jobs = n_jobs;
    if (d_best) *d_best = (int32_t*)b->fuse.d_best.get();
    if (d_hits) *d_hits = (sd_fuse_hit*)b->fuse.d_hits.get();
    if (d_nfused) *d_nfused = b->fuse.d_n;
    return SD_OK;
}

int sd_batch_fuse(sd_batch* b, int n_jobs, const int32_t* kf_index, const float* Tcw_host, const int32_t* cand_offset,
                  const int32_t* d_cand_point, const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points,
                  const uint8_t* d_kf_state, const sd_camera* cam, float th, int32_t** d_best, sd_fuse_hit** d_hits,
                  int32_t** d_nfused, void* stream_)
{
    return fuse_impl(b, n_jobs, kf_index, Tcw_host, cand_offset, d_cand_point, d_points, d_point_desc, n_points, d_kf_state, cam, th, d_best, d_hits,
                     d_nfused, stream_, false);
}

// ---------------------------------------------------------------------------------------------------------
// LoopClosing::ComputeSim3 / SearchAndFuse: the matchers that take a similarity or two keyframes (k_loop.h)
// ---------------------------------------------------------------------------------------------------------
// ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1134-1257)
int sd_batch_fuse_sim3(sd_batch* b, int n_jobs, const int32_t* kf_index, const float* Scw_host, const int32_t* cand_offset,
                       const int32_t* d_cand_point, const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points,
                       const uint8_t* d_kf_state, const sd_camera* cam, float th, int32_t** d_best, sd_fuse_hit** d_hits,
                       int32_t** d_nfused, void* stream_)
{
    return fuse_impl(b, n_jobs, kf_index, Scw_host, cand_offset, d_cand_point, d_points, d_point_desc, n_points, d_kf_state, cam, th, d_best, d_hits,
                     d_nfused, stream_, true);
}

// ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (src/ORBmatcher.cc:679-812)
int sd_batch_search_by_bow_kf(sd_batch* b, int n_pairs, const int32_t* kf1_index, const int32_t* kf2_index, const uint8_t* d_valid1,
                              const uint8_t* d_valid2, float nnratio, int check_orientation, void* stream_)
{
    if (!b || n_pairs < 0 || n_pairs > b->maxImages || (n_pairs > 0 && (!kf1_index || !kf2_index)))
        return set_err(SD_ERR_INVALID, "bad search_by_bow_kf arguments");
    std::vector<int2> idx(n_pairs);
    int rc = check_slots(b, "search_by_bow_kf", kf1_index, kf2_index, n_pairs, SD_SLOT_RANGE);
    if (rc == SD_OK) rc = check_slots(b, "search_by_bow_kf", kf1_index, kf2_index, n_pairs, SD_SLOT_RESULTS | SD_SLOT_BOW);
    if (rc != SD_OK) return rc;
    for (int p = 0; p < n_pairs; p++) idx[p] = make_int2(kf1_index[p], kf2_index[p]);
    const int cap = b->plan.kpCap;
    const size_t lds = (size_t)cap * 4 + 2 * (size_t)cap + 16;
    if (lds > SD_LDS_MAX_BYTES - 1024) return set_err(SD_ERR_UNSUPPORTED, "search_by_bow_kf: the key-point capacity exceeds the LDS tables");
    hipStream_t s = pick_stream(b, stream_);
    b->nPairs = 0; b->dlPairs = 0;
    if (n_pairs == 0) return SD_OK;
    HIPCHK(hipMemcpyAsync(b->d_pairIdx, idx.data(), (size_t)n_pairs * sizeof(int2), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(b->d_npairs, 0, (size_t)n_pairs * 4, s));
    {
        if (lds > 64 * 1024) HIPCHK(sd_raise_lds_limit((const void*)k_search_by_bow_kf, (int)lds));
        ProfScope ps(b, s, K_LOOP_BOW);
        hipLaunchKernelGGL(k_search_by_bow_kf, dim3(n_pairs), dim3(64 * SD_BOW_WAVES), lds, s, KPUN(b), b->d_desc, b->d_count, b->d_fvFeat, b->d_fvRunStart,
                           b->d_fvRunNode, b->d_bowMeta, d_valid1, d_valid2, b->d_pairIdx, cap, nnratio, check_orientation, b->d_match, b->d_nmatch);
        LAUNCH_CHECK("k_search_by_bow_kf");
    }
    b->nPairs = n_pairs; b->dlPairs = n_pairs;
    return SD_OK;
}

// ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th)
// (src/ORBmatcher.cc:290-403)
int sd_batch_search_by_projection_sim3(sd_batch* b, int n_jobs, const int32_t* kf_index, const float* Scw_host, const int32_t* cand_offset,
                                       const int32_t* d_cand_point, const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points,
                                       const int32_t* d_matched, const sd_camera* cam, int th, int32_t** d_assigned, int32_t** d_best,
                                       int32_t** d_nmatches, void* stream_)
{
    if (d_assigned) *d_assigned = nullptr;
    if (d_best) *d_best = nullptr;
    if (d_nmatches) *d_nmatches = nullptr;
    if (!b || n_jobs < 0 || n_jobs > 65535 || n_points < 0 || !cam_ok(cam) || th <= 0 || (n_jobs > 0 && (!kf_index || !Scw_host || !cand_offset || !d_matched)))
        return set_err(SD_ERR_INVALID, "bad search_by_projection_sim3 arguments");
    b->loop.jobs = 0;
    if (n_jobs == 0) return SD_OK;
    int maxM = 0;
    int rc = check_offsets("search_by_projection_sim3", cand_offset, n_jobs, &maxM);
    if (rc == SD_OK) rc = check_slots(b, "search_by_projection_sim3", kf_index, nullptr, n_jobs, SD_SLOT_RANGE);
    if (rc == SD_OK) rc = check_slots(b, "search_by_projection_sim3", kf_index, nullptr, n_jobs, SD_SLOT_RESULTS | SD_SLOT_GRID);
    if (rc != SD_OK) return rc;
    const int total = cand_offset[n_jobs];
    if (total > 0 && (!d_cand_point || !d_points || !d_point_desc || n_points == 0))
        return set_err(SD_ERR_INVALID, "search_by_projection_sim3: entries but no map points given");
    const int cap = b->plan.kpCap;
    if (cap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    hipStream_t s = pick_stream(b, stream_);
    rc = b->loop.grow(b, s, n_jobs, total);
    if (rc != SD_OK) return rc;
    int* dFrameOf = b->loop.d_jobs;
    int* dOff = b->loop.d_jobs + n_jobs;
    b->loop.off.assign(cand_offset, cand_offset + n_jobs + 1);
    b->loop.T.resize((size_t)n_jobs * 16);
    for (int j = 0; j < n_jobs; j++) sd_scw_decompose(Scw_host + (size_t)j * 16, b->loop.T.data() + (size_t)j * 16);
    HIPCHK(hipMemsetAsync(b->loop.d_err, 0, 4, s));               // the flag belongs to this call: every job's download reports it
    HIPCHK(hipMemcpyAsync(dFrameOf, kf_index, (size_t)n_jobs * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dOff, cand_offset, ((size_t)n_jobs + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->loop.d_T, b->loop.T.data(), (size_t)n_jobs * 64, hipMemcpyHostToDevice, s));
    if (maxM > 0) {
        ProfScope ps(b, s, K_LOOP_P);
        hipLaunchKernelGGL(k_loop_search<1>, dim3((maxM + 3) / 4, n_jobs), dim3(256), 0, s, KPUN(b), b->d_desc, b->d_uright, b->d_sortedIdx, b->d_cellStart,
                           b->d_count, (const SdMapPoint*)d_points, d_point_desc, n_points, dFrameOf, dOff, d_cand_point, b->loop.d_T, d_matched,
                           (int2*)nullptr, b->loop.d_list.get(), b->loop.d_listN.get(), b->loop.d_err.get(), level_tables(b), to_cam(cam), (float)th, cap);
        LAUNCH_CHECK("k_loop_search<1>");
    }
    {
        ProfScope ps(b, s, K_LOOP_A);
        hipLaunchKernelGGL(k_loop_assign, dim3(n_jobs), dim3(64), (size_t)((cap + 31) / 32) * 4 + 16, s, dOff, b->loop.d_list.get(), b->loop.d_listN.get(), cap,
                           b->loop.d_assigned.get(), b->loop.d_best.get(), b->loop.d_nm.get(), b->d_err.get());
        LAUNCH_CHECK("k_loop_assign");
    }
    b->loop.jobs = n_jobs;
    if (d_assigned) *d_assigned = b->loop.d_assigned;
    if (d_best) *d_best = (int32_t*)b->loop.d_best.get();
    if (d_nmatches) *d_nmatches = b->loop.d_nm;
    return SD_OK;
}

int sd_batch_download_projection_sim3(sd_batch* b, int job, int32_t* assigned, int cap, int32_t* best, int cap_entries, int* n_entries, int* nmatches)
{
    if (!b || !n_entries || !nmatches || cap_entries < 0) return set_err(SD_ERR_INVALID, "bad download_projection_sim3 arguments");
    if (job < 0 || job >= b->loop.jobs) return set_err(SD_ERR_INVALID, "download_projection_sim3: no such job in the last sd_batch_search_by_projection_sim3");
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int err = 0;
    HIPCHK(hipMemcpy(&err, b->loop.d_err, 4, hipMemcpyDeviceToHost));
    if (err) return set_err(SD_ERR_INVALID, "search_by_projection_sim3: a candidate or a matched entry names a point outside its table");
    const int e0 = b->loop.off[job], n = b->loop.off[job + 1] - e0;
    *n_entries = n;
    HIPCHK(hipMemcpy(nmatches, b->loop.d_nm + job, 4, hipMemcpyDeviceToHost));
    if (best && n > cap_entries) return set_err(SD_ERR_CAPACITY, "projection_sim3 result buffers too small");
    if (assigned && cap < b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "the assigned row needs kp_capacity entries");
    if (assigned) HIPCHK(hipMemcpy(assigned, b->loop.d_assigned + (size_t)job * b->plan.kpCap, (size_t)b->plan.kpCap * 4, hipMemcpyDeviceToHost));
    if (best && n > 0) HIPCHK(hipMemcpy(best, b->loop.d_best + e0, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_batch_download_fuse(sd_batch* b, int job, int32_t* best, sd_fuse_hit* hits, int cap_entries, int* n_entries, int* nfused)
{
    if (!b || !n_entries || !nfused || cap_entries < 0) return set_err(SD_ERR_INVALID, "bad download_fuse arguments");
    if (job < 0 || job >= b->fuse.jobs) return set_err(SD_ERR_INVALID, "download_fuse: no such job in the last sd_batch_fuse");
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int err = 0;
    HIPCHK(hipMemcpy(&err, b->fuse.d_err, 4, hipMemcpyDeviceToHost));
    if (err) {
        HIPCHK(hipMemset(b->fuse.d_err, 0, 4));
        return set_err(SD_ERR_INVALID, "fuse: an entry names a point outside [-1, n_points)");
    }
    const int e0 = b->fuse.off[job], n = b->fuse.off[job + 1] - e0;
    *n_entries = n;
    int nf = 0;
    HIPCHK(hipMemcpy(&nf, b->fuse.d_n + job, 4, hipMemcpyDeviceToHost));
    *nfused = nf;
    if (n > cap_entries) return set_err(SD_ERR_CAPACITY, "fuse result buffers too small");
    if (best && n > 0) HIPCHK(hipMemcpy(best, b->fuse.d_best + e0, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost));
    if (hits && nf > 0) HIPCHK(hipMemcpy(hits, b->fuse.d_hits + e0, (size_t)nf * sizeof(SdFuseHit), hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_distinctive_descriptors_device(int n_points, const int32_t* d_obs_offset, const uint8_t* d_obs_desc, int32_t* d_best_obs,
                                      uint8_t* d_desc_out, void* stream_)
{
    if (n_points < 0 || (n_points > 0 && (!d_obs_offset || !d_obs_desc || !d_best_obs))) return set_err(SD_ERR_INVALID, "bad distinctive_descriptors arguments");
    if (n_points == 0) return SD_OK;
    hipLaunchKernelGGL(k_distinctive, dim3((n_points + 3) / 4), dim3(256), 0, (hipStream_t)stream_, n_points, d_obs_offset, d_obs_desc, d_best_obs, d_desc_out);
    LAUNCH_CHECK("k_distinctive");
    return SD_OK;
}

// The model-fit buffers of sd_batch_estimate_motion (a tracker allocates them at creation)
static int ensure_motion(sd_batch* b)
{
    if (b->d_moPts) return SD_OK;
    const size_t nI = b->maxImages, cap = b->plan.kpCap;
    SdDevBuf<float> pts; SdDevBuf<SdMotionNorm> norm; SdDevBuf<int> counts; SdDevBuf<double> models; SdDevBuf<uint8_t> maskH, maskF; SdDevBuf<SdMotionResult> res;
    HIPCHK(pts.alloc(nI * cap * 16)); HIPCHK(norm.alloc(nI * sizeof(SdMotionNorm))); HIPCHK(counts.alloc(nI * SD_MOTION_K * 4));
    HIPCHK(models.alloc(nI * SD_MOTION_K * 72)); HIPCHK(maskH.alloc(nI * cap)); HIPCHK(maskF.alloc(nI * cap)); HIPCHK(res.alloc(nI * sizeof(SdMotionResult)));
    b->d_moNorm = std::move(norm); b->d_moCounts = std::move(counts); b->d_moModels = std::move(models); b->d_moMaskH = std::move(maskH);
    b->d_moMaskF = std::move(maskF); b->d_moRes = std::move(res);
    b->d_moPts = std::move(pts);                // last: it marks the group as present
    return SD_OK;
}

// The model fit of Tracking::TrackHomo (src/Tracking.cc:1026-1075) for every pair of the preceding
// sd_batch_search_by_projection: points_last / points_current -> H, F, inlier masks, the choice 1 (H) / 2 (F) / 0.
static int estimate_motion_impl(sd_batch* b, int n_pairs, void* stream_, const int* d_active, int minMatches);
int sd_batch_estimate_motion(sd_batch* b, void* stream_) { return estimate_motion_impl(b, b ? b->nPairs : 0, stream_, nullptr, 0); }

// d_active: see SdProjArgs; minMatches > 0: a pair whose matcher returned fewer matches gets flag 0 (TrackHomo's `nmatches<20`)
static int estimate_motion_impl(sd_batch* b, int n_pairs, void* stream_, const int* d_active, int minMatches)
{
    if (!b) return set_err(SD_ERR_INVALID, "null batch");
    b->nMotion = 0;
    if (n_pairs <= 0) return set_err(SD_ERR_STATE, "estimate_motion: no preceding sd_batch_search_by_projection");
    hipStream_t s = pick_stream(b, stream_);
    const size_t cap = b->plan.kpCap;
    int rc = ensure_motion(b);
    if (rc != SD_OK) return rc;
    {
        ProfScope ps(b, s, K_MOTION_P);
        hipLaunchKernelGGL(k_motion_prepare, dim3(n_pairs), dim3(256), cap * 16, s, KPUN(b), b->d_pairs, b->d_npairs, b->d_pairIdx, (int)cap, b->d_moPts, b->d_moNorm,
                           d_active, minMatches > 0 ? (const int*)b->d_nmatch : (const int*)nullptr, minMatches);
        LAUNCH_CHECK("k_motion_prepare");
    }
    {
        ProfScope ps(b, s, K_MOTION_H);
        for (int stage = 0; stage < 2; stage++) {
            const int nh = stage ? SD_MOTION_N1 : SD_MOTION_N0;
            hipLaunchKernelGGL(k_motion_models, dim3(nh / 64, n_pairs), dim3(64), 0, s, b->d_moPts, b->d_moNorm, (int)cap, b->d_moCounts, b->d_moModels, d_active, stage);
            LAUNCH_CHECK("k_motion_models");
            hipLaunchKernelGGL(k_motion_count, dim3(nh / SD_MOTION_HB, n_pairs), dim3(256), 0, s, b->d_moPts, b->d_moNorm, (int)cap, b->d_moCounts, b->d_moModels, d_active, stage);
            LAUNCH_CHECK("k_motion_count");
        }
    }
    {
        ProfScope ps(b, s, K_MOTION_S);
        hipLaunchKernelGGL(k_motion_select, dim3(n_pairs), dim3(256), 0, s, b->d_moPts, b->d_moNorm, b->d_moCounts, (int)cap, b->d_moMaskH, b->d_moMaskF, b->d_moRes, d_active);
        LAUNCH_CHECK("k_motion_select");
    }
    b->nMotion = n_pairs;
    return SD_OK;
}

int sd_batch_download_motion(sd_batch* b, int pair, double* H, double* F, uint8_t* mask_h, uint8_t* mask_f, int cap, int* n_points,
                             int* n_h, int* n_f, float* HorF, int* flag)
{
    if (!b || pair < 0 || pair >= b->nMotion) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    SdMotionResult r;
    HIPCHK(hipMemcpy(&r, b->d_moRes + pair, sizeof(r), hipMemcpyDeviceToHost));
    int np = 0;
    HIPCHK(hipMemcpy(&np, b->d_npairs + pair, 4, hipMemcpyDeviceToHost));
    if (np > cap && (mask_h || mask_f)) return set_err(SD_ERR_CAPACITY, "mask buffer too small");
    if (H) memcpy(H, r.H, sizeof(r.H)); if (F) memcpy(F, r.F, sizeof(r.F)); if (HorF) memcpy(HorF, r.HorF, sizeof(r.HorF));
    if (n_h) *n_h = r.nH; if (n_f) *n_f = r.nF; if (flag) *flag = r.flag; if (n_points) *n_points = np;
    if (np > 0) {
        if (mask_h) HIPCHK(hipMemcpy(mask_h, b->d_moMaskH + (size_t)pair * b->plan.kpCap, np, hipMemcpyDeviceToHost));
        if (mask_f) HIPCHK(hipMemcpy(mask_f, b->d_moMaskF + (size_t)pair * b->plan.kpCap, np, hipMemcpyDeviceToHost));
    }
    return SD_OK;
}

// Frame::UndistortKeyPoints / ComputeImageBounds (src/Frame.cc:812-872) for cameras with distortion.
static SdDistortion to_distortion(const float* K4, const float* dist5)
{
    SdDistortion D;
    D.fx = K4[0]; D.fy = K4[1]; D.cx = K4[2]; D.cy = K4[3];
    D.k1 = dist5[0]; D.k2 = dist5[1]; D.p1 = dist5[2]; D.p2 = dist5[3]; D.k3 = dist5[4];
    return D;
}

int sd_undistort_points_device(const float* d_pts, int n, const float* K4, const float* dist5, float* d_out, void* stream)
{
    if (n < 0 || !K4 || !dist5 || (n > 0 && (!d_pts || !d_out))) return set_err(SD_ERR_INVALID, "bad undistort arguments");
    if (n == 0) return SD_OK;
    hipLaunchKernelGGL(k_undistort_points, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_pts, n, to_distortion(K4, dist5), d_out);
    LAUNCH_CHECK("k_undistort_points");
    return SD_OK;
}

int sd_batch_undistort_keypoints(sd_batch* b, int n_images, const float* K4, const float* dist5, sd_keypoint* d_keys_un, void* stream_)
{
    if (!b || n_images < 0 || n_images > b->nExtracted || !K4 || !dist5 || !d_keys_un) return set_err(SD_ERR_INVALID, "bad undistort_keypoints arguments");
    if (n_images == 0) return SD_OK;
    hipStream_t s = pick_stream(b, stream_);
    const int cap = b->plan.kpCap;
    hipLaunchKernelGGL(k_undistort_keypoints, dim3((cap + 255) / 256, n_images), dim3(256), 0, s, b->d_kp, b->d_count, cap, to_distortion(K4, dist5),
                       dist5[0] == 0.0f ? 1 : 0, d_keys_un);                      // mDistCoef.at<float>(0) == 0.0 -> mvKeysUn = mvKeys
    LAUNCH_CHECK("k_undistort_keypoints");
    return SD_OK;
}

// mvKeysUn as a second key-point array of the batch: with a distortion set, grid, projection / local-map matchers, the RGB-D
// right coordinate, UnprojectStereo, the motion fit's point pairs and classifyH / classifyF read the undistorted key points, exactly
// where the reference reads mvKeysUn; box membership, the depth lookup and the stereo matcher keep reading mvKeys.
int sd_batch_set_distortion(sd_batch* b, const float* K4, const float* dist5)
{
    if (!b || !K4 || !dist5) return SD_ERR_INVALID;
    if (dist5[0] == 0.0f) { b->hasDist = false; return SD_OK; }       // mDistCoef.at<float>(0) == 0.0 -> mvKeysUn = mvKeys (Frame.cc:814-818)
    if (!b->d_kpUn) {
        const size_t nI = b->maxImages, cap = b->plan.kpCap;
        SdDevBuf<sd_keypoint> kpUn, kpDUn; SdDevBuf<int> slots;
        HIPCHK(kpUn.alloc(nI * cap * sizeof(sd_keypoint))); HIPCHK(kpDUn.alloc(nI * cap * sizeof(sd_keypoint))); HIPCHK(slots.alloc(nI * 4));
        b->d_kpDUn = std::move(kpDUn); b->d_unSlots = std::move(slots); b->d_kpUn = std::move(kpUn);      // d_kpUn last: it marks the group as present
    }
    b->dist = to_distortion(K4, dist5);
    b->hasDist = true;
    return SD_OK;
}

int sd_batch_undistort(sd_batch* b, int n_slots, const int32_t* slots, void* stream_)
{
    if (!b || n_slots < 0 || n_slots > b->maxImages || (n_slots > 0 && !slots)) return set_err(SD_ERR_INVALID, "bad undistort arguments");
    hipStream_t s = pick_stream(b, stream_);
    if (!b->hasDist || n_slots == 0) return SD_OK;
    for (int i = 0; i < n_slots; i++) if (slots[i] < 0 || slots[i] >= b->maxImages) return set_err(SD_ERR_INVALID, "bad undistort slot");
    HIPCHK(hipMemcpyAsync(b->d_unSlots, slots, (size_t)n_slots * 4, hipMemcpyHostToDevice, s));
    const int cap = b->plan.kpCap;
    hipLaunchKernelGGL(k_undistort_slots, dim3((cap + 255) / 256, n_slots, 2), dim3(256), 0, s, b->d_kp, b->d_kpD, b->d_count, &b->d_fb[0].nDyn,
                       (int)(sizeof(SdFrameBoxes) / 4), b->d_unSlots, cap, b->dist, b->d_kpUn, b->d_kpDUn);
    LAUNCH_CHECK("k_undistort_slots");
    return SD_OK;
}

int sd_batch_download_keys_un(sd_batch* b, int image, sd_keypoint* kp, int cap, int* n)
{
    if (!b || !n || !slot_ok(b, image)) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int cnt = 0;
    HIPCHK(hipMemcpy(&cnt, b->d_count + image, 4, hipMemcpyDeviceToHost));
    *n = cnt;
    if (cnt > cap) return set_err(SD_ERR_CAPACITY, "keypoint buffer too small");
    if (cnt > 0 && kp) HIPCHK(hipMemcpy(kp, KPUN(b) + (size_t)image * b->plan.kpCap, (size_t)cnt * sizeof(sd_keypoint), hipMemcpyDeviceToHost));
    return SD_OK;
}

int sd_batch_download_dynamic_keys_un(sd_batch* b, int slot, sd_keypoint* kp, int cap, int* n)
{
    if (!b || !n || !slot_ok(b, slot)) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    SdFrameBoxes h;
    HIPCHK(hipMemcpy(&h, b->d_fb + slot, sizeof(h), hipMemcpyDeviceToHost));
    *n = h.nDyn;
    if (h.nDyn > cap) return set_err(SD_ERR_CAPACITY, "dynamic keypoint buffer too small");
    if (h.nDyn > 0 && kp) HIPCHK(hipMemcpy(kp, KPDUN(b) + (size_t)slot * b->plan.kpCap, (size_t)h.nDyn * sizeof(sd_keypoint), hipMemcpyDeviceToHost));
    return SD_OK;
}

// Four corner points, once per camera: host arithmetic (double, the same expression order as the kernel).
int sd_image_bounds(int cols, int rows, const float* K4, const float* dist5, float* bounds4)
{
    if (!K4 || !dist5 || !bounds4 || cols < 1 || rows < 1) return SD_ERR_INVALID;
    if (dist5[0] != 0.0f) {
        const double fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3], k1 = dist5[0], k2 = dist5[1], p1 = dist5[2], p2 = dist5[3], k3 = dist5[4];
        const float corners[8] = {0.f, 0.f, (float)cols, 0.f, 0.f, (float)rows, (float)cols, (float)rows};
        float u[8];
        const double ifx = 1. / fx, ify = 1. / fy;
        for (int i = 0; i < 4; i++) {
            double x = corners[2 * i], y = corners[2 * i + 1];
            x = (x - cx) * ifx; y = (y - cy) * ify;
            const double x0 = x, y0 = y;
            for (int j = 0; j < 5; j++) {
                const double r2 = x * x + y * y;
                const double icdist = (1 + ((0. * r2 + 0.) * r2 + 0.) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2);
                const double deltaX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
                const double deltaY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
                x = (x0 - deltaX) * icdist;
                y = (y0 - deltaY) * icdist;
            }
            u[2 * i] = (float)(x * fx + cx); u[2 * i + 1] = (float)(y * fy + cy);
        }
        bounds4[0] = std::min(u[0], u[4]); bounds4[1] = std::max(u[2], u[6]);
        bounds4[2] = std::min(u[1], u[3]); bounds4[3] = std::max(u[5], u[7]);
    } else {
        bounds4[0] = 0.0f; bounds4[1] = (float)cols; bounds4[2] = 0.0f; bounds4[3] = (float)rows;
    }
    return SD_OK;
}

// Frame copy (mLastFrame = Frame(mCurrentFrame), Tracking.cc; Frame.cc:39-63): every per-slot array (frame_arrays) of n (src, dst) slot
// pairs in one launch; the pairs come from `d_pairs` or, for one pair, as (src0, dst0)
static int copy_frames_impl(sd_batch* b, int n, const int2* d_pairs, int src0, int dst0, const int32_t* src, const int32_t* dst, hipStream_t s)
{
    int rc = launch_copy_frames(frame_copy_table(b, b, SD_FRAME_ALL), 8, n, d_pairs, src0, 0, dst0, 0, s);
    if (rc != SD_OK) return rc;
    for (int i = 0; i < n; i++) {
        b->slotValid[dst[i]] = 1;
        b->gridValid[dst[i]] = b->gridValid[src[i]];             // the grid arrays travel with the frame
        if (!b->bowValid.empty()) b->bowValid[dst[i]] = 0;      // mBowVec / mFeatVec are recomputed on demand (ComputeBoW's `if(mBowVec.empty())`)
    }
    return SD_OK;
}

int sd_batch_copy_frame(sd_batch* b, int src, int dst, void* stream_)
{
    if (!b || !slot_ok(b, src) || dst < 0 || dst >= b->maxImages || src == dst) return set_err(SD_ERR_INVALID, "bad copy_frame slots");
    hipStream_t s = pick_stream(b, stream_);
    return copy_frames_impl(b, 1, nullptr, src, dst, &src, &dst, s);
}

int sd_batch_copy_frames(sd_batch* b, int n, const int32_t* src, const int32_t* dst, void* stream_)
{
    if (!b || n < 0 || n > b->maxImages || (n > 0 && (!src || !dst))) return set_err(SD_ERR_INVALID, "bad copy_frames arguments");
    hipStream_t s = pick_stream(b, stream_);
    if (n == 0) return SD_OK;
    std::vector<int2>& pr = b->hostCopyPairs;
    pr.resize(n);
    for (int i = 0; i < n; i++) {
        if (!slot_ok(b, src[i]) || dst[i] < 0 || dst[i] >= b->maxImages) return set_err(SD_ERR_INVALID, "bad copy_frames slots");
        pr[i] = make_int2(src[i], dst[i]);
    }
    HIPCHK(hipMemcpyAsync(b->d_copyPairs, pr.data(), (size_t)n * sizeof(int2), hipMemcpyHostToDevice, s));
    return copy_frames_impl(b, n, b->d_copyPairs, 0, 0, src, dst, s);
}

int sd_batch_matches_device(sd_batch* b, int32_t** d_match, int32_t** d_pairs, int32_t** d_npairs, int32_t** d_nmatches, int* cap)
{
    if (!b) return SD_ERR_INVALID;
    if (d_match) *d_match = b->d_match;
    if (d_pairs) *d_pairs = b->d_pairs;
    if (d_npairs) *d_npairs = b->d_npairs;
    if (d_nmatches) *d_nmatches = b->d_nmatch;
    if (cap) *cap = b->plan.kpCap;
    return SD_OK;
}

int sd_batch_download_matches(sd_batch* b, int pair, int32_t* match, int32_t* pairs, int cap, int* npairs, int* nmatches)
{
    if (!b || pair < 0 || pair >= b->dlPairs) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    if (cap < b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "match buffers need kp_capacity entries");
    int np = 0, nm = 0;
    HIPCHK(hipMemcpy(&np, b->d_npairs + pair, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&nm, b->d_nmatch + pair, 4, hipMemcpyDeviceToHost));
    if (match) HIPCHK(hipMemcpy(match, b->d_match + (size_t)pair * b->plan.kpCap, (size_t)b->plan.kpCap * 4, hipMemcpyDeviceToHost));
    if (pairs && np > 0) HIPCHK(hipMemcpy(pairs, b->d_pairs + (size_t)pair * b->plan.kpCap * 2, (size_t)np * 8, hipMemcpyDeviceToHost));
    if (npairs) *npairs = np;
    if (nmatches) *nmatches = nm;
    return SD_OK;
}


// ---------------------------------------------------------------- Optimizer::PoseOptimization (k_pose.h)
// Plain form: the caller's edges.  The cameras travel through an SdTableRing.
namespace {
SdDeviceTable<SdTableRing<sd_camera>> g_poseCams;
}

static int pose_launch(const SdPoseArgs& A, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_pose_optimize, dim3(n), dim3(SD_POSE_THREADS), 0, s, A);
    LAUNCH_CHECK("k_pose_optimize");
    return SD_OK;
}

int sd_pose_optimize_device(int n_problems, const int32_t* d_edge_offset, const sd_pose_edge* d_edges, const sd_camera* cams,
                            float* d_Tcw, uint8_t* d_outlier, int32_t* d_n_good, void* stream_)
{
    if (n_problems < 0 || (n_problems > 0 && (!d_edge_offset || !d_edges || !cams || !d_Tcw || !d_outlier || !d_n_good)))
        return set_err(SD_ERR_INVALID, "bad pose_optimize arguments");
    if (n_problems == 0) return SD_OK;
    hipStream_t s = (hipStream_t)stream_;
    decltype(g_poseCams)::Locked C;
    SD_TRY(g_poseCams.lock("pose_optimize", C));
    SdPoseArgs A;
    SD_TRY(C->stage(cams, (size_t)n_problems, s, A.cam));
    A.edges = d_edges; A.first = d_edge_offset; A.last = d_edge_offset + 1; A.Tcw = d_Tcw; A.outlier = d_outlier;
    A.nGood = d_n_good; A.map = nullptr;
    SD_TRY(pose_launch(A, n_problems, s));
    return C->publish(s);
}

int sd_pose_optimize_host(int n_problems, const int32_t* edge_offset, const sd_pose_edge* edges, const sd_camera* cams,
                          float* Tcw, uint8_t* outlier, int32_t* n_good)
{
    if (n_problems < 0 || (n_problems > 0 && (!edge_offset || !cams || !Tcw || !n_good))) return set_err(SD_ERR_INVALID, "bad pose_optimize arguments");
    if (n_problems == 0) return SD_OK;
    int rc = check_offsets("pose_optimize", edge_offset, n_problems, nullptr);
    if (rc != SD_OK) return rc;
    const size_t nE = (size_t)edge_offset[n_problems];
    if (nE > 0 && (!edges || !outlier)) return set_err(SD_ERR_INVALID, "bad pose_optimize arguments");
    rc = require_device();
    if (rc != SD_OK) return rc;
    SdDevBuf<int32_t> d_off, d_g; SdDevBuf<sd_pose_edge> d_e; SdDevBuf<float> d_T; SdDevBuf<uint8_t> d_o;
    HIPCHK(d_off.alloc((size_t)(n_problems + 1) * 4)); HIPCHK(d_e.alloc(std::max<size_t>(nE, 1) * sizeof(sd_pose_edge)));
    HIPCHK(d_T.alloc((size_t)n_problems * 64)); HIPCHK(d_o.alloc(std::max<size_t>(nE, 1))); HIPCHK(d_g.alloc((size_t)n_problems * 4));
    HIPCHK(hipMemcpy(d_off, edge_offset, (size_t)(n_problems + 1) * 4, hipMemcpyHostToDevice));
    if (nE) HIPCHK(hipMemcpy(d_e, edges, nE * sizeof(sd_pose_edge), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_T, Tcw, (size_t)n_problems * 64, hipMemcpyHostToDevice));
    rc = sd_pose_optimize_device(n_problems, d_off, d_e, cams, d_T, d_o, d_g, nullptr);
    if (rc != SD_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(Tcw, d_T, (size_t)n_problems * 64, hipMemcpyDeviceToHost));
    if (nE) HIPCHK(hipMemcpy(outlier, d_o, nE, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n_good, d_g, (size_t)n_problems * 4, hipMemcpyDeviceToHost));
    return SD_OK;
}

// ---------------------------------------------------------------- Optimizer::LocalBundleAdjustment (k_ba.h)
static_assert(sizeof(sd_ba_keyframe) == 88 && sizeof(sd_ba_edge) == 32 && sizeof(sd_ba_stats) == 48, "local BA records");
static_assert(SD_BA_MAX_LOCAL == SD_BA_MAX_LOCAL_KEYFRAMES && SD_BA_MAX_FIXED == SD_BA_MAX_FIXED_KEYFRAMES &&
              SD_BA_MAX_POINTS == SD_BA_MAX_POINTS_PER_PROBLEM && SD_BA_MAX_EDGES == SD_BA_MAX_EDGES_PER_PROBLEM, "local BA caps");
namespace {
struct BaState {
    SdTableRing<SdBaProblem> prob;
    SdWorkspace ws; SdDevBuf<double> wsD; SdDevBuf<int> wsI; size_t capD = 0, capI = 0;
    SdDevBuf<long long> prof; size_t capProf = 0; int profProblems = 0;      // the last profiled call
};
SdDeviceTable<BaState> g_ba;
bool g_baProfiling = false;       // under g_ba.mu
}
static_assert(SD_BA_PHASES == SD_BA_PROFILE_PHASES, "local BA phases");

// the host-side checks both entry points share; fills the problem table and the workspace sizes
static int ba_plan(int n, const int32_t* kfOff, const int32_t* nLocal, const int32_t* ptOff, const int32_t* eOff, std::vector<SdBaProblem>& tab,
                   size_t& needD, size_t& needI, int& maxLocal)
{
    if (!kfOff || !nLocal || !ptOff || !eOff) return set_err(SD_ERR_INVALID, "bad local_ba arguments");
    for (const int32_t* off : {kfOff, ptOff, eOff}) SD_TRY(check_offsets("local_ba", off, n, nullptr));
    tab.resize(n);
    needD = needI = 0; maxLocal = 0;
    for (int p = 0; p < n; p++) {
        const int nk = kfOff[p + 1] - kfOff[p], np = ptOff[p + 1] - ptOff[p], ne = eOff[p + 1] - eOff[p];
        if (nLocal[p] < 0 || nLocal[p] > nk) return set_err(SD_ERR_INVALID, "n_local outside the problem's keyframes");
        if (nLocal[p] > SD_BA_MAX_LOCAL || nk - nLocal[p] > SD_BA_MAX_FIXED || np > SD_BA_MAX_POINTS || ne > SD_BA_MAX_EDGES)
            return set_err(SD_ERR_INVALID, "local_ba problem " + std::to_string(p) + " is over the caps (64 local / 128 fixed keyframes, 8192 points, 65536 edges)");
        SdBaProblem& q = tab[p];
        q.kf0 = kfOff[p]; q.nKF = nk; q.nLocal = nLocal[p]; q.pt0 = ptOff[p]; q.nPt = np; q.e0 = eOff[p]; q.nE = ne; q.pad = 0;
        q.wsD = needD; q.wsI = needI;
        needD += (sd_ba_ws_doubles(nk, nLocal[p], np, ne) + 1) & ~(size_t)1;
        needI += (sd_ba_ws_ints(nk, nLocal[p], np, ne) + 3) & ~(size_t)3;
        maxLocal = std::max(maxLocal, nLocal[p]);
    }
    if (sd_ba_lds_bytes(maxLocal) > SD_LDS_MAX_BYTES) return set_err(SD_ERR_INVALID, "local_ba reduced system beyond the LDS of a workgroup");
    return SD_OK;
}

int sd_local_ba_device(int n_problems, const int32_t* kf_offset, const int32_t* n_local, const int32_t* point_offset,
                       const int32_t* edge_offset, const sd_ba_keyframe* d_kfs, const float* d_xw, const sd_ba_edge* d_edges,
                       const int32_t* d_ref_kf, float* d_Tcw, float* d_xw_out, float* d_normal, float* d_dist, uint8_t* d_level1,
                       uint8_t* d_erase, sd_ba_stats* d_stats, void* stream_)
{
    if (n_problems < 0) return set_err(SD_ERR_INVALID, "bad local_ba arguments");
    if (n_problems == 0) return SD_OK;
    std::vector<SdBaProblem> tab;
    size_t needD = 0, needI = 0;
    int maxLocal = 0;
    int rc = ba_plan(n_problems, kf_offset, n_local, point_offset, edge_offset, tab, needD, needI, maxLocal);
    if (rc != SD_OK) return rc;
    const bool anyKf = kf_offset[n_problems] > 0, anyPt = point_offset[n_problems] > 0, anyE = edge_offset[n_problems] > 0;
    if (!d_stats || (anyKf && (!d_kfs || !d_Tcw)) || (anyPt && (!d_xw || !d_ref_kf || !d_xw_out || !d_normal || !d_dist)) ||
        (anyE && (!d_edges || !d_level1 || !d_erase)))
        return set_err(SD_ERR_INVALID, "bad local_ba arguments");
    hipStream_t s = (hipStream_t)stream_;
    decltype(g_ba)::Locked B;
    SD_TRY(g_ba.lock("local_ba", B));
    SdBaArgs A;
    SD_TRY(B->prob.stage(tab.data(), (size_t)n_problems, s, A.prob));
    const size_t needProf = g_baProfiling ? (size_t)n_problems * SD_BA_PHASES : 0;      // (the wait of enter() also covers the previous call's use of `prof`)
    SD_TRY(B->ws.enter(s, B->capD < needD || B->capI < needI || B->capProf < needProf));
    SD_TRY(SdWorkspace::grow(B->capD, needD, {{&B->wsD, sizeof(double)}}));
    SD_TRY(SdWorkspace::grow(B->capI, needI, {{&B->wsI, sizeof(int)}}));
    SD_TRY(SdWorkspace::grow(B->capProf, needProf, {{&B->prof, sizeof(long long)}}));
    const int lds = (int)sd_ba_lds_bytes(maxLocal);
    HIPCHK(sd_raise_lds_limit((const void*)k_local_ba, lds));
    A.kfs = d_kfs; A.xw = d_xw; A.edges = d_edges; A.refKf = d_ref_kf; A.Tcw = d_Tcw; A.xwOut = d_xw_out; A.normal = d_normal;
    A.dist = d_dist; A.level1 = d_level1; A.erase = d_erase; A.stats = d_stats; A.wsD = B->wsD; A.wsI = B->wsI; A.prof = nullptr;
    if (needProf) {
        HIPCHK(hipMemsetAsync(B->prof, 0, needProf * sizeof(long long), s));
        A.prof = B->prof; B->profProblems = n_problems;
    }
    hipLaunchKernelGGL(k_local_ba, dim3(n_problems), dim3(SD_BA_THREADS), lds, s, A);
    LAUNCH_CHECK("k_local_ba");
    SD_TRY(B->ws.leave(s));
    return B->prob.publish(s);
}

int sd_local_ba_set_profiling(int on)
{
    std::lock_guard<std::mutex> lk(g_ba.mu);
    g_baProfiling = on != 0;
    return SD_OK;
}

int sd_local_ba_profile(int n_problems, double* ms)
{
    if (!ms) return set_err(SD_ERR_INVALID, "bad local_ba_profile arguments");
    decltype(g_ba)::Locked B;
    SD_TRY(g_ba.lock("local_ba_profile", B));
    if (B->profProblems == 0) return set_err(SD_ERR_STATE, "no profiled sd_local_ba_device call on this device");      // else ws has its event
    if (n_problems != B->profProblems) return set_err(SD_ERR_INVALID, "n_problems is not that of the last profiled call");
    SD_TRY(B->ws.wait());
    std::vector<long long> t((size_t)n_problems * SD_BA_PHASES);
    HIPCHK(hipMemcpy(t.data(), B->prof, t.size() * sizeof(long long), hipMemcpyDeviceToHost));
    int khz = 0;
    HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, B.device));
    if (khz <= 0) return set_err(SD_ERR_UNSUPPORTED, "the device reports no wall-clock rate");
    for (size_t i = 0; i < t.size(); i++) ms[i] = (double)t[i] / (double)khz;
    return SD_OK;
}

int sd_local_ba_host(int n_problems, const int32_t* kf_offset, const int32_t* n_local, const int32_t* point_offset,
                     const int32_t* edge_offset, const sd_ba_keyframe* kfs, const float* xw, const sd_ba_edge* edges,
                     const int32_t* ref_kf, float* Tcw, float* xw_out, float* normal, float* dist, uint8_t* level1, uint8_t* erase,
                     sd_ba_stats* stats)
{
    if (n_problems < 0) return set_err(SD_ERR_INVALID, "bad local_ba arguments");
    if (n_problems == 0) return SD_OK;
    std::vector<SdBaProblem> tab;
    size_t needD = 0, needI = 0;
    int maxLocal = 0;
    int rc = ba_plan(n_problems, kf_offset, n_local, point_offset, edge_offset, tab, needD, needI, maxLocal);
    if (rc != SD_OK) return rc;
    const size_t nK = (size_t)kf_offset[n_problems], nP = (size_t)point_offset[n_problems], nE = (size_t)edge_offset[n_problems];
    if (!stats || (nK && (!kfs || !Tcw)) || (nP && (!xw || !ref_kf || !xw_out || !normal || !dist)) || (nE && (!edges || !level1 || !erase)))
        return set_err(SD_ERR_INVALID, "bad local_ba arguments");
    for (int p = 0; p < n_problems; p++) {
        const SdBaProblem& q = tab[p];
        for (int i = 0; i < q.nE; i++) {
            const sd_ba_edge& e = edges[(size_t)q.e0 + i];
            if (e.kf < 0 || e.kf >= q.nKF || e.point < 0 || e.point >= q.nPt)
                return set_err(SD_ERR_INVALID, "local_ba problem " + std::to_string(p) + ": edge " + std::to_string(i) + " indexes outside its tables");
        }
        for (int i = 0; i < q.nPt; i++)
            if (ref_kf[(size_t)q.pt0 + i] < -1 || ref_kf[(size_t)q.pt0 + i] >= q.nKF)
                return set_err(SD_ERR_INVALID, "local_ba problem " + std::to_string(p) + ": ref_kf outside its keyframes");
    }
    rc = require_device();
    if (rc != SD_OK) return rc;
    SdDevBuf<sd_ba_keyframe> d_k; SdDevBuf<float> d_x, d_T, d_xo, d_n, d_d; SdDevBuf<sd_ba_edge> d_e; SdDevBuf<int32_t> d_r; SdDevBuf<uint8_t> d_l, d_er;
    SdDevBuf<sd_ba_stats> d_s;
    const size_t mK = std::max<size_t>(nK, 1), mP = std::max<size_t>(nP, 1), mE = std::max<size_t>(nE, 1);
    HIPCHK(d_k.alloc(mK * sizeof(sd_ba_keyframe))); HIPCHK(d_T.alloc(mK * 64)); HIPCHK(d_x.alloc(mP * 12)); HIPCHK(d_xo.alloc(mP * 12));
    HIPCHK(d_n.alloc(mP * 12)); HIPCHK(d_d.alloc(mP * 4)); HIPCHK(d_r.alloc(mP * 4)); HIPCHK(d_e.alloc(mE * sizeof(sd_ba_edge)));
    HIPCHK(d_l.alloc(mE)); HIPCHK(d_er.alloc(mE)); HIPCHK(d_s.alloc((size_t)n_problems * sizeof(sd_ba_stats)));
    if (nK) HIPCHK(hipMemcpy(d_k, kfs, nK * sizeof(sd_ba_keyframe), hipMemcpyHostToDevice));
    if (nP) { HIPCHK(hipMemcpy(d_x, xw, nP * 12, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_r, ref_kf, nP * 4, hipMemcpyHostToDevice)); }
    if (nE) HIPCHK(hipMemcpy(d_e, edges, nE * sizeof(sd_ba_edge), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_T, 0, mK * 64)); HIPCHK(hipMemset(d_l, 0, mE)); HIPCHK(hipMemset(d_er, 0, mE));
    rc = sd_local_ba_device(n_problems, kf_offset, n_local, point_offset, edge_offset, d_k, d_x, d_e, d_r, d_T, d_xo, d_n, d_d, d_l, d_er, d_s, nullptr);
    if (rc != SD_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    if (nK) HIPCHK(hipMemcpy(Tcw, d_T, nK * 64, hipMemcpyDeviceToHost));
    if (nP) {
        HIPCHK(hipMemcpy(xw_out, d_xo, nP * 12, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(normal, d_n, nP * 12, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dist, d_d, nP * 4, hipMemcpyDeviceToHost));
    }
    if (nE) { HIPCHK(hipMemcpy(level1, d_l, nE, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(erase, d_er, nE, hipMemcpyDeviceToHost)); }
    HIPCHK(hipMemcpy(stats, d_s, (size_t)n_problems * sizeof(sd_ba_stats), hipMemcpyDeviceToHost));
    return SD_OK;
}

// ---------------------------------------------------------------- Sim3Solver RANSAC (k_sim3.h)
static_assert(sizeof(sd_sim3_corr) == 36 && sizeof(sd_sim3_problem) == 176 && sizeof(sd_sim3_result) == 140, "sim3 records");
static_assert(sizeof(SdSim3Pt) == 48 && sizeof(SdSim3Hyp) == 192 && sizeof(SdSim3Prob) == 208, "sim3 workspace records");
static_assert(SD_SIM3_MAX_N == SD_SIM3_MAX_CORRESPONDENCES && SD_SIM3_MAX_ITS == SD_SIM3_MAX_ITERATIONS, "sim3 caps");
static_assert(SD_SIM3_MAX_N < (1 << 15) && SD_SIM3_MAX_ITS < (1 << 16), "a (count, iteration) key is 32 bits");
static_assert(SD_SIM3_MAX_PROBLEMS <= 65535, "a problem is a grid row");
namespace {
struct Sim3State {
    SdTableRing<SdSim3Prob> prob;
    SdWorkspace ws; SdDevBuf<SdSim3Pt> pts; SdDevBuf<SdSim3Hyp> hyp; SdDevBuf<int> count; size_t capPts = 0, capHyp = 0;
};
SdDeviceTable<Sim3State> g_sim3;
}

// Sim3Solver::SetRansacParameters (Sim3Solver.cc:114-138) as written; the double is clamped before the conversion to int so that no
// value of it is undefined (N < minInliers makes it NaN, a tiny epsilon makes it -inf)
static int sim3_max_its(double probability, int minInliers, int maxIterations, int N)
{
    const float epsilon = (float)minInliers / N;
    int nIterations;
    if (minInliers == N) nIterations = 1;
    else {
        const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
        nIterations = !(v < (double)maxIterations) ? maxIterations : (v <= 1.0 ? 1 : (int)v);
    }
    return std::max(1, std::min(nIterations, maxIterations));
}

// the host-side checks both entry points share; fills the problem table
static int sim3_plan(int n, const int32_t* off, const sd_sim3_problem* problems, double probability, int minInliers, int maxIterations,
                     std::vector<SdSim3Prob>& tab, size_t& nHyp, int& maxN, int& maxIts)
{
    if (!off || !problems) return set_err(SD_ERR_INVALID, "bad sim3_ransac arguments");
    if (!(probability > 0.0 && probability < 1.0)) return set_err(SD_ERR_INVALID, "sim3_ransac probability must lie in (0, 1)");
    if (minInliers < 0) return set_err(SD_ERR_INVALID, "sim3_ransac min_inliers must not be negative");
    if (maxIterations < 1 || maxIterations > SD_SIM3_MAX_ITS) return set_err(SD_ERR_INVALID, "sim3_ransac max_iterations outside [1, 4096]");
    if (n > SD_SIM3_MAX_PROBLEMS) return set_err(SD_ERR_INVALID, "sim3_ransac: more than 65535 problems in one call");
    SD_TRY(check_offsets("sim3_ransac", off, n, nullptr));
    tab.resize(n);
    nHyp = 0; maxN = 0; maxIts = 0;
    for (int p = 0; p < n; p++) {
        const int N = off[p + 1] - off[p];
        if (N > SD_SIM3_MAX_N) return set_err(SD_ERR_INVALID, "sim3_ransac problem " + std::to_string(p) + " holds more than 4096 correspondences");
        SdSim3Prob& q = tab[p];
        q.P = problems[p]; q.c0 = off[p]; q.n = N; q.minInliers = minInliers; q.pad[0] = q.pad[1] = 0;
        q.ransacMaxIts = sim3_max_its(probability, minInliers, maxIterations, N);
        q.maxIts = (N < minInliers || N < 3) ? 0 : q.ransacMaxIts;
        q.h0 = (int)nHyp;
        nHyp += (size_t)q.maxIts;
        maxN = std::max(maxN, q.n); maxIts = std::max(maxIts, q.maxIts);
    }
    if (nHyp > (size_t)0x7FFFFFFF) return set_err(SD_ERR_INVALID, "sim3_ransac: more than 2^31 hypotheses in one call");
    return SD_OK;
}

int sd_sim3_ransac_device(int n_problems, const int32_t* corr_offset, const sd_sim3_corr* d_corr, const sd_sim3_problem* problems,
                          double probability, int min_inliers, int max_iterations, sd_sim3_result* d_results, uint8_t* d_inliers,
                          int32_t* max_its_out, void* stream_)
{
    if (n_problems < 0) return set_err(SD_ERR_INVALID, "bad sim3_ransac arguments");
    if (n_problems == 0) return SD_OK;
    std::vector<SdSim3Prob> tab;
    size_t nHyp = 0;
    int maxN = 0, maxIts = 0;
    int rc = sim3_plan(n_problems, corr_offset, problems, probability, min_inliers, max_iterations, tab, nHyp, maxN, maxIts);
    if (rc != SD_OK) return rc;
    const size_t nC = (size_t)corr_offset[n_problems];
    if (!d_results || (nC && (!d_corr || !d_inliers))) return set_err(SD_ERR_INVALID, "bad sim3_ransac arguments");
    if (max_its_out)
        for (int p = 0; p < n_problems; p++)
            max_its_out[p] = tab[p].ransacMaxIts;
    hipStream_t s = (hipStream_t)stream_;
    decltype(g_sim3)::Locked B;
    SD_TRY(g_sim3.lock("sim3_ransac", B));
    SdSim3Args A;
    SD_TRY(B->prob.stage(tab.data(), (size_t)n_problems, s, A.prob));
    const size_t needPts = std::max<size_t>(nC, 1), needHyp = std::max<size_t>(nHyp, 1);
    SD_TRY(B->ws.enter(s, B->capPts < needPts || B->capHyp < needHyp));
    SD_TRY(SdWorkspace::grow(B->capPts, needPts, {{&B->pts, sizeof(SdSim3Pt)}}));
    SD_TRY(SdWorkspace::grow(B->capHyp, needHyp, {{&B->hyp, sizeof(SdSim3Hyp)}, {&B->count, sizeof(int)}}));
    A.corr = d_corr; A.pts = B->pts; A.hyp = B->hyp; A.count = B->count; A.result = d_results; A.inlier = d_inliers;
    const int rowBlocks = std::max(1, (maxN + 255) / 256);
    if (maxN > 0) {
        hipLaunchKernelGGL(k_sim3_prepare, dim3(rowBlocks, n_problems), dim3(256), 0, s, A);
        LAUNCH_CHECK("k_sim3_prepare");
    }
    if (maxIts > 0) {
        hipLaunchKernelGGL(k_sim3_hypotheses, dim3((maxIts + 63) / 64, n_problems), dim3(64), 0, s, A);
        LAUNCH_CHECK("k_sim3_hypotheses");
        hipLaunchKernelGGL(k_sim3_count, dim3((maxIts + SD_SIM3_HYP_PER_BLOCK - 1) / SD_SIM3_HYP_PER_BLOCK, n_problems), dim3(256), 0, s, A);
        LAUNCH_CHECK("k_sim3_count");
    }
    hipLaunchKernelGGL(k_sim3_select, dim3(n_problems), dim3(64), 0, s, A);
    LAUNCH_CHECK("k_sim3_select");
    if (maxN > 0) {
        hipLaunchKernelGGL(k_sim3_inliers, dim3(rowBlocks, n_problems), dim3(256), 0, s, A);
        LAUNCH_CHECK("k_sim3_inliers");
    }
    SD_TRY(B->ws.leave(s));
    return B->prob.publish(s);
}

int sd_sim3_ransac_host(int n_problems, const int32_t* corr_offset, const sd_sim3_corr* corr, const sd_sim3_problem* problems,
                        double probability, int min_inliers, int max_iterations, sd_sim3_result* results, uint8_t* inliers)
{
    if (n_problems < 0) return set_err(SD_ERR_INVALID, "bad sim3_ransac arguments");
    if (n_problems == 0) return SD_OK;
    std::vector<SdSim3Prob> tab;
    size_t nHyp = 0;
    int maxN = 0, maxIts = 0;
    int rc = sim3_plan(n_problems, corr_offset, problems, probability, min_inliers, max_iterations, tab, nHyp, maxN, maxIts);
    if (rc != SD_OK) return rc;
    const size_t nC = (size_t)corr_offset[n_problems];
    if (!results || (nC && (!corr || !inliers))) return set_err(SD_ERR_INVALID, "bad sim3_ransac arguments");
    rc = require_device();
    if (rc != SD_OK) return rc;
    SdDevBuf<sd_sim3_corr> d_c; SdDevBuf<sd_sim3_result> d_r; SdDevBuf<uint8_t> d_i;
    HIPCHK(d_c.alloc(std::max<size_t>(nC, 1) * sizeof(sd_sim3_corr))); HIPCHK(d_r.alloc((size_t)n_problems * sizeof(sd_sim3_result)));
    HIPCHK(d_i.alloc(std::max<size_t>(nC, 1)));
    if (nC) HIPCHK(hipMemcpy(d_c, corr, nC * sizeof(sd_sim3_corr), hipMemcpyHostToDevice));
    rc = sd_sim3_ransac_device(n_problems, corr_offset, d_c, problems, probability, min_inliers, max_iterations, d_r, d_i, nullptr, nullptr);
    if (rc != SD_OK) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(results, d_r, (size_t)n_problems * sizeof(sd_sim3_result), hipMemcpyDeviceToHost));
    if (nC) HIPCHK(hipMemcpy(inliers, d_i, nC, hipMemcpyDeviceToHost));
    return SD_OK;
}

// ---------------------------------------------------------------- ORBmatcher::SearchBySim3 (k_sim3.h)
static int sim3_search_launch(sd_batch* b, int n_pairs, const sd_camera* cam, float th, const sd_map_point* d_points, const uint8_t* d_point_desc,
                              int n_points, const int32_t* d_kf1_point, const int32_t* d_kf2_point, const int32_t* d_matched12, hipStream_t s);

int sd_batch_search_by_sim3(sd_batch* b, int n_pairs, const int32_t* kf1_index, const int32_t* kf2_index, const float* Tcw1_host,
                            const float* Tcw2_host, const float* s12, const float* R12, const float* t12, const sd_camera* cam, float th,
                            const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points, const int32_t* d_kf1_point,
                            const int32_t* d_kf2_point, const int32_t* d_matched12, void* stream_)
{
    static_assert(sizeof(SdSim3Pair) == 272, "sim3 pair record");
    if (!b || n_pairs < 0 || n_pairs > 32767 || n_points < 0 || !cam_ok(cam) || !(th > 0) ||
        (n_pairs > 0 && (!kf1_index || !kf2_index || !Tcw1_host || !Tcw2_host || !s12 || !R12 || !t12 || !d_kf1_point || !d_kf2_point || !d_matched12)))
        return set_err(SD_ERR_INVALID, "bad search_by_sim3 arguments");
    b->sim3.pairs = 0;
    if (n_pairs == 0) return SD_OK;
    if (n_points > 0 && (!d_points || !d_point_desc)) return set_err(SD_ERR_INVALID, "search_by_sim3: n_points but no point table");
    int rc = check_slots(b, "search_by_sim3", kf1_index, kf2_index, n_pairs, SD_SLOT_RANGE);
    if (rc == SD_OK) rc = check_slots(b, "search_by_sim3", kf1_index, kf2_index, n_pairs, SD_SLOT_RESULTS | SD_SLOT_GRID);
    if (rc != SD_OK) return rc;
    const int cap = b->plan.kpCap;
    if (cap > 65535) return set_err(SD_ERR_UNSUPPORTED, "more than 65535 keypoints per image");
    hipStream_t s = pick_stream(b, stream_);
    rc = b->sim3.grow(b, s, n_pairs);
    if (rc != SD_OK) return rc;
    HIPCHK(hipMemsetAsync(b->sim3.d_err, 0, 4, s));               // the flag belongs to this call: every pair's download reports it
    // the transformation between the cameras (ORBmatcher.cc:1276-1278), as DESIGN Q39 freezes it
    b->sim3.host.resize(n_pairs);
    for (int p = 0; p < n_pairs; p++) {
        SdSim3Pair& P = b->sim3.host[p];
        memcpy(P.T1, Tcw1_host + (size_t)p * 16, 64); memcpy(P.T2, Tcw2_host + (size_t)p * 16, 64);
        const float sc = s12[p];
        const float* R = R12 + (size_t)p * 9;
        const float* t = t12 + (size_t)p * 3;
        const double inv = 1.0 / (double)sc;
        float sR21[3][3];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) { P.T12[4 * i + j] = sc * R[3 * i + j]; sR21[i][j] = (float)(inv * (double)R[3 * j + i]); P.T21[4 * i + j] = sR21[i][j]; }
            P.T12[4 * i + 3] = t[i];
        }
        for (int i = 0; i < 3; i++) { float a = (-sR21[i][0]) * t[0] + (-sR21[i][1]) * t[1]; P.T21[4 * i + 3] = a + (-sR21[i][2]) * t[2]; }
        for (int j = 0; j < 3; j++) { P.T12[12 + j] = 0.f; P.T21[12 + j] = 0.f; }
        P.T12[15] = 1.f; P.T21[15] = 1.f;
        P.slot1 = kf1_index[p]; P.slot2 = kf2_index[p]; P.pad[0] = P.pad[1] = 0;
    }
    HIPCHK(hipMemcpyAsync(b->sim3.d_pairs, b->sim3.host.data(), (size_t)n_pairs * sizeof(SdSim3Pair), hipMemcpyHostToDevice, s));
    rc = sim3_search_launch(b, n_pairs, cam, th, d_points, d_point_desc, n_points, d_kf1_point, d_kf2_point, d_matched12, s);
    if (rc != SD_OK) return rc;
    b->sim3.pairs = n_pairs;
    return SD_OK;
}

// the three kernels of SearchBySim3 over the pair table b->sim3.d_pairs (filled by the caller, on the host or on the device)
static int sim3_search_launch(sd_batch* b, int n_pairs, const sd_camera* cam, float th, const sd_map_point* d_points, const uint8_t* d_point_desc,
                              int n_points, const int32_t* d_kf1_point, const int32_t* d_kf2_point, const int32_t* d_matched12, hipStream_t s)
{
    const int cap = b->plan.kpCap;
    const size_t rows = (size_t)n_pairs * cap;
    HIPCHK(hipMemsetAsync(b->sim3.d_already, 0, rows, s));
    HIPCHK(hipMemsetAsync(b->sim3.d_match1, 0xFF, rows * 4, s)); HIPCHK(hipMemsetAsync(b->sim3.d_match2, 0xFF, rows * 4, s));
    HIPCHK(hipMemsetAsync(b->sim3.d_match12, 0xFF, rows * 4, s));
    SdSim3SearchArgs A;
    A.kp = KPUN(b); A.desc = b->d_desc; A.uRight = b->d_uright; A.sortedIdx = b->d_sortedIdx; A.cellStart = b->d_cellStart; A.count = b->d_count;
    A.pairs = b->sim3.d_pairs; A.mps = (const SdMapPoint*)d_points; A.mpDesc = d_point_desc; A.nPoints = n_points;
    A.kfPoint[0] = d_kf1_point; A.kfPoint[1] = d_kf2_point; A.matched12 = d_matched12; A.already2 = b->sim3.d_already;
    A.vnMatch[0] = b->sim3.d_match1; A.vnMatch[1] = b->sim3.d_match2; A.match12 = b->sim3.d_match12; A.nFound = b->sim3.d_found; A.errFlag = b->sim3.d_err; A.cap = cap;
    {
        ProfScope ps(b, s, K_SIM3_M);
        hipLaunchKernelGGL(k_sim3_mark, dim3((cap + 255) / 256, n_pairs), dim3(256), 0, s, A);
        LAUNCH_CHECK("k_sim3_mark");
    }
    {
        ProfScope ps(b, s, K_SIM3_S);
        hipLaunchKernelGGL(k_sim3_search, dim3((cap + 3) / 4, 2 * n_pairs), dim3(256), 0, s, A, level_tables(b), to_cam(cam), th);
        LAUNCH_CHECK("k_sim3_search");
    }
    {
        ProfScope ps(b, s, K_SIM3_A);
        hipLaunchKernelGGL(k_sim3_agree, dim3(n_pairs), dim3(256), 0, s, A);
        LAUNCH_CHECK("k_sim3_agree");
    }
    return SD_OK;
}

int sd_batch_download_sim3_matches(sd_batch* b, int pair, int32_t* match12, int32_t* vnMatch1, int32_t* vnMatch2, int cap, int* n_found)
{
    if (!b || !n_found) return set_err(SD_ERR_INVALID, "bad download_sim3_matches arguments");
    if (pair < 0 || pair >= b->sim3.pairs) return set_err(SD_ERR_INVALID, "download_sim3_matches: no such pair in the last sd_batch_search_by_sim3");
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int err = 0;
    HIPCHK(hipMemcpy(&err, b->sim3.d_err, 4, hipMemcpyDeviceToHost));
    if (err) return set_err(SD_ERR_INVALID, "search_by_sim3: a feature names a point outside [-1, n_points)");
    if (cap < b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "sim3 match buffers need kp_capacity entries");
    const size_t row = (size_t)pair * b->plan.kpCap, bytes = (size_t)b->plan.kpCap * 4;
    if (match12) HIPCHK(hipMemcpy(match12, b->sim3.d_match12 + row, bytes, hipMemcpyDeviceToHost));
    if (vnMatch1) HIPCHK(hipMemcpy(vnMatch1, b->sim3.d_match1 + row, bytes, hipMemcpyDeviceToHost));
    if (vnMatch2) HIPCHK(hipMemcpy(vnMatch2, b->sim3.d_match2 + row, bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n_found, b->sim3.d_found + pair, 4, hipMemcpyDeviceToHost));
    return SD_OK;
}

static int ensure_pose(sd_batch* b)
{
    if (b->d_poseEdges) return SD_OK;
    const size_t nI = b->maxImages, cap = b->plan.kpCap;
    SdDevBuf<sd_pose_edge> edges; SdDevBuf<int> first, last, good, map, ran; SdDevBuf<float> T, Tin; SdDevBuf<uint8_t> out; SdDevBuf<sd_camera> cam;
    HIPCHK(edges.alloc(nI * cap * sizeof(sd_pose_edge))); HIPCHK(first.alloc(nI * 4)); HIPCHK(last.alloc(nI * 4)); HIPCHK(T.alloc(nI * 64));
    HIPCHK(out.alloc(nI * cap)); HIPCHK(good.alloc(nI * 4)); HIPCHK(cam.alloc(nI * sizeof(sd_camera))); HIPCHK(map.alloc(nI * 4));
    HIPCHK(ran.alloc(nI * 4)); HIPCHK(Tin.alloc(nI * 64));
    HIPCHK(hipMemset(first, 0, nI * 4)); HIPCHK(hipMemset(last, 0, nI * 4)); HIPCHK(hipMemset(good, 0, nI * 4)); HIPCHK(hipMemset(ran, 0, nI * 4));
    b->d_poseFirst = std::move(first); b->d_poseLast = std::move(last); b->d_poseT = std::move(T); b->d_poseOut = std::move(out); b->d_poseGood = std::move(good);
    b->d_poseCam = std::move(cam); b->d_poseMap = std::move(map); b->d_poseRan = std::move(ran); b->d_poseTin = std::move(Tin);
    b->d_poseEdges = std::move(edges);          // last: it marks the group as present
    return SD_OK;
}

// d_active / activeBase / minMatches: the tracker's gating (SdPoseEdgeArgs); the plain entry passes none
static int batch_pose_impl(sd_batch* b, int n_pairs, const int32_t* pair_index, const float* Tcw_host, hipStream_t s, const int* d_active,
                           int activeBase, int minMatches)
{
    if (!b || n_pairs < 0 || (n_pairs > 0 && !pair_index)) return set_err(SD_ERR_INVALID, "bad batch pose_optimize arguments");
    if (n_pairs == 0) return SD_OK;
    if (b->pairCam.size() != (size_t)b->maxImages) return set_err(SD_ERR_STATE, "pose_optimize before search_by_projection");
    std::vector<uint8_t> seen(b->maxImages, 0);
    for (int k = 0; k < n_pairs; k++) {
        if (pair_index[k] < 0 || pair_index[k] >= b->dlPairs) return set_err(SD_ERR_STATE, "pose_optimize: pair holds no projection matches");
        if (seen[pair_index[k]]++) return set_err(SD_ERR_INVALID, "pose_optimize: a pair is listed twice");
    }
    int rc = ensure_pose(b);
    if (rc != SD_OK) return rc;
    b->lastStream = s;
    b->hPoseMap.assign(pair_index, pair_index + n_pairs);
    b->hPoseCam.resize(n_pairs);
    for (int k = 0; k < n_pairs; k++) b->hPoseCam[k] = b->pairCam[pair_index[k]];
    HIPCHK(hipMemcpyAsync(b->d_poseMap, b->hPoseMap.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->d_poseCam, b->hPoseCam.data(), (size_t)n_pairs * sizeof(sd_camera), hipMemcpyHostToDevice, s));
    if (Tcw_host) HIPCHK(hipMemcpyAsync(b->d_poseTin, Tcw_host, (size_t)n_pairs * 64, hipMemcpyHostToDevice, s));
    SdPoseEdgeArgs E;
    E.kp = KPUN(b); E.uRight = b->d_uright; E.count = b->d_count; E.xw = b->d_xw; E.match = b->d_match; E.pairIdx = b->d_pairIdx;
    E.TcwPair = b->d_pose; E.Tin = Tcw_host ? b->d_poseTin : nullptr; E.map = b->d_poseMap; E.active = d_active; E.activeBase = activeBase; E.nmatch = b->d_nmatch;
    E.minMatches = minMatches; E.edges = b->d_poseEdges; E.first = b->d_poseFirst; E.last = b->d_poseLast; E.Tout = b->d_poseT; E.ran = b->d_poseRan;
    for (int l = 0; l < SD_MAX_LEVELS; l++) E.invSigma2[l] = l < b->ex->prm.nlevels ? b->ex->prm.invSigma2[l] : 0.f;
    E.nLevels = b->ex->prm.nlevels; E.cap = b->plan.kpCap;
    hipLaunchKernelGGL(k_pose_edges, dim3(n_pairs), dim3(256), 0, s, E);
    LAUNCH_CHECK("k_pose_edges");
    SdPoseArgs A;
    A.edges = b->d_poseEdges; A.first = b->d_poseFirst; A.last = b->d_poseLast; A.cam = b->d_poseCam; A.Tcw = b->d_poseT;
    A.outlier = b->d_poseOut; A.nGood = b->d_poseGood; A.map = b->d_poseMap;
    return pose_launch(A, n_pairs, s);
}

int sd_batch_pose_optimize(sd_batch* b, int n_pairs, const int32_t* pair_index, const float* Tcw_host, void* stream_)
{
    if (!b) return set_err(SD_ERR_INVALID, "null batch");
    hipStream_t s = stream_ ? (hipStream_t)stream_ : b->lastStream;
    return batch_pose_impl(b, n_pairs, pair_index, Tcw_host, s, nullptr, 0, 0);
}

int sd_batch_download_pose(sd_batch* b, int pair, float* Tcw, uint8_t* outlier, int cap, int* n_initial, int* n_good)
{
    if (!b || pair < 0 || pair >= b->maxImages) return set_err(SD_ERR_INVALID, "bad download_pose arguments");
    if (!b->d_poseEdges) return set_err(SD_ERR_STATE, "no pose_optimize ran on this batch");
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    if (outlier && cap < b->plan.kpCap) return set_err(SD_ERR_CAPACITY, "outlier buffer needs kp_capacity entries");
    int f = 0, l = 0, g = 0;
    HIPCHK(hipMemcpy(&f, b->d_poseFirst + pair, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&l, b->d_poseLast + pair, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&g, b->d_poseGood + pair, 4, hipMemcpyDeviceToHost));
    if (Tcw) HIPCHK(hipMemcpy(Tcw, b->d_poseT + (size_t)pair * 16, 64, hipMemcpyDeviceToHost));
    const int n = l - f;
    if (outlier) {
        memset(outlier, 0, (size_t)b->plan.kpCap);
        if (n > 0) {
            std::vector<sd_pose_edge> e(n);
            std::vector<uint8_t> o(n);
            HIPCHK(hipMemcpy(e.data(), b->d_poseEdges + f, (size_t)n * sizeof(sd_pose_edge), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(o.data(), b->d_poseOut + f, (size_t)n, hipMemcpyDeviceToHost));
            for (int i = 0; i < n; i++) outlier[e[i].kp_index] = o[i];
        }
    }
    if (n_initial) *n_initial = n;
    if (n_good) *n_good = n < 3 ? 0 : g;
    return SD_OK;
}


// ---------------------------------------------------------------- dynamic-object cull
static SdCullPtrs cull_ptrs(sd_batch* b)
{
    SdCullPtrs A;
    A.kp = b->d_kp; A.desc = b->d_desc; A.uright = b->d_uright; A.depth = b->d_depth; A.count = b->d_count;
    A.kpT = b->d_kpT; A.descT = b->d_descT; A.urT = b->d_urT; A.depT = b->d_depT;
    A.kpD = b->d_kpD; A.descD = b->d_descD; A.urD = b->d_urD; A.depD = b->d_depD; A.kpDUn = KPDUN(b);
    A.fb = b->d_fb; A.boxItems = b->d_boxItems; A.cap = b->plan.kpCap; A.itemsCap = b->itemsCap; A.errFlag = b->d_err;
    return A;
}

namespace {
struct HRect { double x, y, w, h; bool empty() const { return w <= 0 || h <= 0; } double area() const { return w * h; } };
inline HRect hrect_and(HRect a, const HRect& b)
{
    const double x1 = a.x > b.x ? a.x : b.x, y1 = a.y > b.y ? a.y : b.y;
    const double x2 = a.x + a.w < b.x + b.w ? a.x + a.w : b.x + b.w, y2 = a.y + a.h < b.y + b.h ? a.y + a.h : b.y + b.h;
    HRect r = {x1, y1, x2 - x1, y2 - y1};
    if (r.w <= 0 || r.h <= 0) r = HRect{0, 0, 0, 0};
    return r;
}
inline HRect hrect_or(HRect a, const HRect& b)
{
    if (a.empty()) return b;
    if (b.empty()) return a;
    const double x1 = a.x < b.x ? a.x : b.x, y1 = a.y < b.y ? a.y : b.y;
    const double x2 = a.x + a.w > b.x + b.w ? a.x + a.w : b.x + b.w, y2 = a.y + a.h > b.y + b.h ? a.y + a.h : b.y + b.h;
    return HRect{x1, y1, x2 - x1, y2 - y1};
}
}  // namespace

// Frame::boxTrack (src/Frame.cc:481-552) — host code: a handful of boxes per frame, f64 arithmetic.
int sd_box_track(double* boxes, int n_box, int cap, const double* last_objects, int n_last, const int32_t* last_box_idx,
                 const uint8_t* last_omit, const double* last_velocity, int img_cols, int img_rows, int32_t* box_idx,
                 uint8_t* omit, double* velocity, int* n_out)
{
    if (!boxes || n_box < 0 || cap < n_box || n_last < 0 || !box_idx || !omit || !velocity || !n_out ||
        (n_last > 0 && (!last_objects || !last_box_idx || !last_omit || !last_velocity)))
        return set_err(SD_ERR_INVALID, "bad box_track arguments");
    std::vector<HRect> bx(n_box);
    for (int i = 0; i < n_box; i++) bx[i] = HRect{boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3]};
    std::vector<int> idx(n_box, -1);
    std::vector<uint8_t> om(n_box, 0);
    std::vector<double> vel(2 * (size_t)n_box, 0.0);
    if (n_last > 0) {
        std::vector<HRect> lo(n_last);
        for (int i = 0; i < n_last; i++) lo[i] = HRect{last_objects[4 * i], last_objects[4 * i + 1], last_objects[4 * i + 2], last_objects[4 * i + 3]};
        for (int i = 0; i < n_last; i++) {           // greedy 1 - IoU association, later previous boxes may overwrite
            double minCost = 1;
            int best = -1;
            for (int j = 0; j < n_box; j++) {
                const double cost = 1 - hrect_and(lo[i], bx[j]).area() / hrect_or(lo[i], bx[j]).area();
                if (cost < minCost) { minCost = cost; best = j; }
            }
            if (best != -1 && !last_omit[i]) {
                idx[best] = last_box_idx[i];
                vel[2 * best] = bx[best].x + bx[best].w / 2 - lo[i].x - lo[i].w / 2;
                vel[2 * best + 1] = bx[best].y + bx[best].h / 2 - lo[i].y - lo[i].h / 2;
            }
        }
        for (int i = 0; i < n_last; i++) {           // re-inject an unmatched previous box once
            if (last_omit[i]) continue;
            bool found = false;
            for (size_t k = 0; k < idx.size(); k++) found |= idx[k] == last_box_idx[i];
            if (found) continue;
            const float cx = (float)(lo[i].x + lo[i].w / 2 + last_velocity[2 * i]);
            const float cy = (float)(lo[i].y + lo[i].h / 2 + last_velocity[2 * i + 1]);
            if (0.f <= cx && cx < (float)img_cols && 0.f <= cy && cy < (float)img_rows) {
                bx.push_back(HRect{lo[i].x + last_velocity[2 * i], lo[i].y + last_velocity[2 * i + 1], lo[i].w, lo[i].h});
                idx.push_back(last_box_idx[i]);
                om.push_back(1);
                vel.push_back(last_velocity[2 * i]); vel.push_back(last_velocity[2 * i + 1]);
            }
        }
        for (int i = 0; i < n_box; i++) {            // new ids for unmatched current boxes
            if (idx[i] != -1) continue;
            int mx = idx[0];
            for (size_t k = 1; k < idx.size(); k++) mx = idx[k] > mx ? idx[k] : mx;
            idx[i] = mx + 1;
        }
    } else {
        for (int i = 0; i < n_box; i++) idx[i] = i;
    }
    const int n = (int)bx.size();
    if (n > cap) return set_err(SD_ERR_CAPACITY, "box buffer too small for the re-injected boxes");
    for (int i = 0; i < n; i++) {
        boxes[4 * i] = bx[i].x; boxes[4 * i + 1] = bx[i].y; boxes[4 * i + 2] = bx[i].w; boxes[4 * i + 3] = bx[i].h;
        box_idx[i] = idx[i]; omit[i] = om[i]; velocity[2 * i] = vel[2 * i]; velocity[2 * i + 1] = vel[2 * i + 1];
    }
    *n_out = n;
    return SD_OK;
}

int sd_batch_first_separate(sd_batch* b, int n_frames, const int32_t* slots, const double* boxes, const int32_t* n_boxes,
                            const int32_t* box_idx, void* stream_)
{
    if (!b || n_frames < 0 || n_frames > b->maxImages || (n_frames > 0 && (!slots || !boxes || !n_boxes || !box_idx)))
        return set_err(SD_ERR_INVALID, "bad first_separate arguments");
    if (!b->cullOk) return set_err(SD_ERR_UNSUPPORTED, "more key points per image than the dynamic-object kernels' LDS tables hold (about 6,800)");
    hipStream_t s = pick_stream(b, stream_);
    if (n_frames == 0) return SD_OK;
    std::vector<SdFrameBoxes>& h = b->hostBoxes;
    h.resize(n_frames);
    for (int f = 0; f < n_frames; f++) {
        int rc = check_slots(b, "first_separate", slots + f, nullptr, 1, SD_SLOT_RESULTS);
        if (rc != SD_OK) return rc;
        if (n_boxes[f] < 0 || n_boxes[f] > SD_MAXB) return set_err(SD_ERR_CAPACITY, "more than SD_MAX_BOXES boxes in a frame");
        memset(&h[f], 0, sizeof(SdFrameBoxes));
        h[f].nb = n_boxes[f];
        for (int j = 0; j < n_boxes[f]; j++) {
            for (int k = 0; k < 4; k++) h[f].boxes[j][k] = boxes[((size_t)f * SD_MAXB + j) * 4 + k];
            h[f].box_idx[j] = box_idx[(size_t)f * SD_MAXB + j];
            h[f].box_status[j] = -1;
        }
    }
    HIPCHK(hipMemcpyAsync(b->d_fbStage, h.data(), (size_t)n_frames * sizeof(SdFrameBoxes), hipMemcpyHostToDevice, s));      // one copy; the workgroups scatter
    HIPCHK(hipMemcpyAsync(b->d_slots, slots, (size_t)n_frames * 4, hipMemcpyHostToDevice, s));
    {
        ProfScope ps(b, s, K_BOXSEP);
        hipLaunchKernelGGL(k_box_separate, dim3(n_frames), dim3(256), sd_box_separate_lds(b->plan.kpCap), s, cull_ptrs(b), b->d_slots, b->d_fbStage);
    }
    LAUNCH_CHECK("k_box_separate");
    return SD_OK;
}

int sd_batch_download_boxes(sd_batch* b, int slot, int* nb, double* boxes, int32_t* box_idx, int32_t* box_status, int32_t* kept_orig,
                            int32_t* box_start, int32_t* box_items, int items_cap, int* n_all, int* n_static)
{
    if (!b || !slot_ok(b, slot)) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    SdFrameBoxes h;
    HIPCHK(hipMemcpy(&h, b->d_fb + slot, sizeof(h), hipMemcpyDeviceToHost));
    if (nb) *nb = h.nb;
    if (n_all) *n_all = h.nAll;
    if (n_static) *n_static = h.nOri;
    for (int j = 0; j < h.nb; j++) {
        if (boxes) for (int k = 0; k < 4; k++) boxes[4 * j + k] = h.boxes[j][k];
        if (box_idx) box_idx[j] = h.box_idx[j];
        if (box_status) box_status[j] = h.box_status[j];
        if (kept_orig) kept_orig[j] = h.keptOrig[j];
    }
    if (box_start) for (int j = 0; j <= h.nb; j++) box_start[j] = h.boxStart[j];
    if (box_items) {
        const int n = h.boxStart[h.nb];
        if (n > items_cap) return set_err(SD_ERR_CAPACITY, "box item buffer too small");
        if (n > 0) HIPCHK(hipMemcpy(box_items, b->d_boxItems + (size_t)slot * b->itemsCap, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    return SD_OK;
}

static_assert(sizeof(sd_frame_boxes) == sizeof(SdFrameBoxes) && offsetof(sd_frame_boxes, box_status) == offsetof(SdFrameBoxes, box_status) &&
              offsetof(sd_frame_boxes, box_start) == offsetof(SdFrameBoxes, boxStart), "sd_frame_boxes is the public face of SdFrameBoxes");
int sd_batch_boxes_device(sd_batch* b, sd_frame_boxes** d_frame_boxes)
{
    if (!b || !d_frame_boxes) return SD_ERR_INVALID;
    *d_frame_boxes = (sd_frame_boxes*)b->d_fb.get();
    return SD_OK;
}

int sd_batch_download_dynamic(sd_batch* b, int slot, sd_keypoint* kp, uint8_t* desc, float* uright, float* depth, int cap, int* n)
{
    if (!b || !slot_ok(b, slot) || !n) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    SdFrameBoxes h;
    HIPCHK(hipMemcpy(&h, b->d_fb + slot, sizeof(h), hipMemcpyDeviceToHost));
    *n = h.nDyn;
    if (h.nDyn > cap) return set_err(SD_ERR_CAPACITY, "dynamic keypoint buffer too small");
    const size_t off = (size_t)slot * b->plan.kpCap;
    if (h.nDyn > 0) {
        if (kp) HIPCHK(hipMemcpy(kp, b->d_kpD + off, (size_t)h.nDyn * sizeof(sd_keypoint), hipMemcpyDeviceToHost));
        if (desc) HIPCHK(hipMemcpy(desc, b->d_descD + off * 32, (size_t)h.nDyn * 32, hipMemcpyDeviceToHost));
        if (uright) HIPCHK(hipMemcpy(uright, b->d_urD + off, (size_t)h.nDyn * 4, hipMemcpyDeviceToHost));
        if (depth) HIPCHK(hipMemcpy(depth, b->d_depD + off, (size_t)h.nDyn * 4, hipMemcpyDeviceToHost));
    }
    return SD_OK;
}

static int separate_impl(sd_batch* b, int n_pairs, const int32_t* cur_index, const int32_t* ref_index, const float* HorF,
                         const int32_t* flag, const int32_t* last_box_idx, const int32_t* last_box_status, const int32_t* n_last,
                         void* stream_, const int32_t* last_slot, const int* d_active);
int sd_batch_separate(sd_batch* b, int n_pairs, const int32_t* cur_index, const int32_t* ref_index, const float* HorF,
                      const int32_t* flag, const int32_t* last_box_idx, const int32_t* last_box_status, const int32_t* n_last,
                      void* stream_)
{
    return separate_impl(b, n_pairs, cur_index, ref_index, HorF, flag, last_box_idx, last_box_status, n_last, stream_, nullptr, nullptr);
}

// last_slot (host, nullable): slot of mLastFrame per pair, replaces last_box_idx / last_box_status / n_last; d_active: see SdSepArgs
static int separate_impl(sd_batch* b, int n_pairs, const int32_t* cur_index, const int32_t* ref_index, const float* HorF,
                         const int32_t* flag, const int32_t* last_box_idx, const int32_t* last_box_status, const int32_t* n_last,
                         void* stream_, const int32_t* last_slot, const int* d_active)
{
    if (!b || n_pairs < 0 || n_pairs > b->maxImages ||
        (n_pairs > 0 && (!cur_index || !ref_index || (!HorF) != (!flag) || (!last_slot && (!last_box_idx || !last_box_status || !n_last)))))
        return set_err(SD_ERR_INVALID, "bad separate arguments");
    if (!b->cullOk) return set_err(SD_ERR_UNSUPPORTED, "more key points per image than the dynamic-object kernels' LDS tables hold (about 6,800)");
    const bool fromMotion = n_pairs > 0 && !HorF;          // HorF == flag == NULL: pair p uses the model fit of pair p
    if (fromMotion && b->nMotion < n_pairs) return set_err(SD_ERR_STATE, "separate: no sd_batch_estimate_motion results for these pairs");
    hipStream_t s = pick_stream(b, stream_);
    b->nSepPairs = 0;
    if (n_pairs == 0) return SD_OK;
    std::vector<int2>& idx = b->hostPairs;
    idx.resize(n_pairs);
    for (int p = 0; p < n_pairs; p++) {
        int rc = check_slots(b, "separate", cur_index + p, ref_index + p, 1, SD_SLOT_RESULTS);
        if (rc != SD_OK) return rc;
        if (!fromMotion && flag[p] != 1 && flag[p] != 2) return set_err(SD_ERR_INVALID, "separate: flag must be 1 (H) or 2 (F)");
        if (last_slot ? !slot_ok(b, last_slot[p]) : (n_last[p] < 0 || n_last[p] > SD_MAXB)) return set_err(SD_ERR_INVALID, "separate: bad n_last / last slot");
        idx[p] = make_int2(cur_index[p], ref_index[p]);
    }
    HIPCHK(hipMemcpyAsync(b->d_sepPairs, idx.data(), (size_t)n_pairs * sizeof(int2), hipMemcpyHostToDevice, s));
    if (fromMotion) {
        hipLaunchKernelGGL(k_motion_to_sep, dim3((n_pairs + 63) / 64), dim3(64), 0, s, b->d_moRes, b->d_HorF, b->d_sepFlag, n_pairs, d_active);
        LAUNCH_CHECK("k_motion_to_sep");
    } else {
        HIPCHK(hipMemcpyAsync(b->d_HorF, HorF, (size_t)n_pairs * 36, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(b->d_sepFlag, flag, (size_t)n_pairs * 4, hipMemcpyHostToDevice, s));
    }
    if (last_slot) {
        HIPCHK(hipMemcpyAsync(b->d_nLast, last_slot, (size_t)n_pairs * 4, hipMemcpyHostToDevice, s));      // d_nLast doubles as the slot list
    } else {
        HIPCHK(hipMemcpyAsync(b->d_lastIdx, last_box_idx, (size_t)n_pairs * SD_MAXB * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(b->d_lastStatus, last_box_status, (size_t)n_pairs * SD_MAXB * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(b->d_nLast, n_last, (size_t)n_pairs * 4, hipMemcpyHostToDevice, s));
    }
    SdSepArgs G;
    G.pairIdx = b->d_sepPairs; G.HorF = b->d_HorF; G.flag = b->d_sepFlag; G.lastIdx = b->d_lastIdx; G.lastStatus = b->d_lastStatus;
    G.nLast = b->d_nLast; G.dynStart = b->d_dynStart; G.dynStatus = b->d_dynStatus; G.matches = b->d_sepMatches; G.ret = b->d_sepRet;
    G.lastSlot = last_slot ? b->d_nLast : nullptr; G.active = d_active;
    b->sepActive = d_active;
    {
        ProfScope ps(b, s, K_SEPARATE);
        hipLaunchKernelGGL(k_separate, dim3(n_pairs), dim3(256), sd_separate_lds(b->plan.kpCap), s, cull_ptrs(b), G);
    }
    LAUNCH_CHECK("k_separate");
    b->nSepPairs = n_pairs;
    return SD_OK;
}

int sd_batch_download_separate(sd_batch* b, int pair, int32_t* ret, int32_t* dyn_start, int32_t* dyn_status, int32_t* matches, int cap)
{
    if (!b || pair < 0 || pair >= b->nSepPairs) return SD_ERR_INVALID;
    int rc = sd_batch_sync(b);
    if (rc != SD_OK) return rc;
    int ds[SD_MAXB + 1];
    HIPCHK(hipMemcpy(ds, b->d_dynStart + (size_t)pair * (SD_MAXB + 1), sizeof(ds), hipMemcpyDeviceToHost));
    if (dyn_start) memcpy(dyn_start, ds, sizeof(ds));
    const int n = ds[SD_MAXB];
    if (n > cap) return set_err(SD_ERR_CAPACITY, "dynStatus buffer too small");
    if (ret) HIPCHK(hipMemcpy(ret, b->d_sepRet + pair, 4, hipMemcpyDeviceToHost));
    if (n > 0) {
        if (dyn_status) HIPCHK(hipMemcpy(dyn_status, b->d_dynStatus + (size_t)pair * b->itemsCap, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (matches) HIPCHK(hipMemcpy(matches, b->d_sepMatches + (size_t)pair * b->itemsCap * 2, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    return SD_OK;
}

int sd_batch_update_frame(sd_batch* b, int only_if_static, void* stream_)
{
    if (!b) return SD_ERR_INVALID;
    if (b->nSepPairs <= 0) return set_err(SD_ERR_STATE, "update_frame needs a preceding separate");
    hipStream_t s = pick_stream(b, stream_);
    SdSepArgs G;
    G.pairIdx = b->d_sepPairs; G.HorF = b->d_HorF; G.flag = b->d_sepFlag; G.lastIdx = b->d_lastIdx; G.lastStatus = b->d_lastStatus;
    G.nLast = b->d_nLast; G.dynStart = b->d_dynStart; G.dynStatus = b->d_dynStatus; G.matches = b->d_sepMatches; G.ret = b->d_sepRet;
    G.lastSlot = nullptr; G.active = b->sepActive;
    {
        ProfScope ps(b, s, K_UPDATE);
        const size_t lds = (size_t)b->itemsCap * 4 + (size_t)b->plan.kpCap + 64;
        hipLaunchKernelGGL(k_update_frame, dim3(b->nSepPairs), dim3(256), lds, s, cull_ptrs(b), G,
                           only_if_static ? (const int*)b->d_sepRet : (const int*)nullptr);
    }
    LAUNCH_CHECK("k_update_frame");
    return SD_OK;
}


// ---------------------------------------------------------------- reference-frame queue (Tracking.cc:620-666, 952-959)
struct sd_refqueue {
    struct E { double t; int slot; int hasBoxes; };
    std::vector<E> q;      // front = oldest
};

int sd_refqueue_create(sd_refqueue** out) { if (!out) return SD_ERR_INVALID; *out = new sd_refqueue(); return SD_OK; }
int sd_refqueue_destroy(sd_refqueue* q) { delete q; return SD_OK; }
int sd_refqueue_clear(sd_refqueue* q) { if (!q) return SD_ERR_INVALID; q->q.clear(); return SD_OK; }   // :602-605
int sd_refqueue_size(const sd_refqueue* q, int* n) { if (!q || !n) return SD_ERR_INVALID; *n = (int)q->q.size(); return SD_OK; }

// The `while(mCurrentFrame.mTimeStamp - q_frame.front().mTimeStamp > 0.2f)` head of the loop (:623-631): drops
// box-less fronts, then yields the oldest frame more than 0.2 s older than the current one, or -1.
int sd_refqueue_candidate(sd_refqueue* q, double cur_timestamp, int cur_has_boxes, int* slot)
{
    if (!q || !slot) return SD_ERR_INVALID;
    *slot = -1;
    if (!cur_has_boxes) return SD_OK;                              // `!mCurrentFrame.objects.empty()` (:622)
    while (!q->q.empty() && cur_timestamp - q->q.front().t > 0.2f) {
        if (!q->q.front().hasBoxes) { q->q.erase(q->q.begin()); continue; }   // reference: no emptiness re-check (UB)
        *slot = q->q.front().slot;
        return SD_OK;
    }
    return SD_OK;
}

// TrackHomo failed on the candidate (:655-661): pop it unless it is the last element; *again = loop continues.
int sd_refqueue_reject(sd_refqueue* q, int* again)
{
    if (!q || !again) return SD_ERR_INVALID;
    *again = 0;
    if (q->q.size() <= 1) return SD_OK;
    q->q.erase(q->q.begin());
    *again = 1;
    return SD_OK;
}

// After tracking (mState == OK): `if(q_frame.size() >= mMaxFrames * 0.3) q_frame.pop(); q_frame.push(cur)` (:952-959).
// *evicted_slot = slot of the popped frame (its batch slot can be reused) or -1.
int sd_refqueue_push(sd_refqueue* q, double timestamp, int slot, int has_boxes, int max_frames, int* evicted_slot)
{
    if (!q) return SD_ERR_INVALID;
    if (evicted_slot) *evicted_slot = -1;
    if ((double)q->q.size() >= max_frames * 0.3 && !q->q.empty()) {
        if (evicted_slot) *evicted_slot = q->q.front().slot;
        q->q.erase(q->q.begin());
    }
    q->q.push_back({timestamp, slot, has_boxes});
    return SD_OK;
}


// ---------------------------------------------------------------- profiling
int sd_batch_set_profiling(sd_batch* b, int enabled)
{
    if (!b) return SD_ERR_INVALID;
    b->profiling = enabled != 0;
    return SD_OK;
}
int sd_batch_kernel_count(const sd_batch* b, int* n)
{
    if (!b || !n) return SD_ERR_INVALID;
    *n = K_COUNT;
    return SD_OK;
}
int sd_batch_kernel_times(sd_batch* b, int index, const char** name, double* total_ms, int64_t* launches)
{
    if (!b || index < 0 || index >= K_COUNT) return SD_ERR_INVALID;
    drain_profile(b);
    if (name) *name = kKernelNames[index];
    if (total_ms) *total_ms = b->totalMs[index];
    if (launches) *launches = b->launches[index];
    return SD_OK;
}
int sd_batch_reset_kernel_times(sd_batch* b)
{
    if (!b) return SD_ERR_INVALID;
    drain_profile(b);
    for (int i = 0; i < K_COUNT; i++) { b->totalMs[i] = 0; b->launches[i] = 0; }
    return SD_OK;
}

// PointCloudMapping::generatePointCloud (src/pointcloudmapping.cc:59-103) for frame slots of the batch
int sd_batch_backproject_dense(sd_batch* b, int n_frames, const int32_t* slots, const uint8_t* d_color, size_t color_stride,
                               size_t color_pitch, const uint16_t* d_depth, size_t depth_stride_elems, size_t depth_pitch_elems,
                               float depth_factor, const uint8_t* d_mask, size_t mask_stride, size_t mask_pitch, const sd_camera* cam,
                               const double* Twc_host, sd_cloud_point* d_points, int cap_points, int32_t* d_counts, void* stream_)
{
    if (!b || n_frames < 0 || n_frames > b->maxImages || !cam_ok(cam) || (n_frames > 0 && (!slots || !d_color || !d_depth || !Twc_host || !d_points || !d_counts)))
        return set_err(SD_ERR_INVALID, "bad backproject_dense arguments");
    const int W = b->plan.W, H = b->plan.H;
    const int cols3 = (W + 2) / 3, rows3 = (H + 2) / 3, words = (cols3 + 63) / 64;
    if (cap_points < cols3 * rows3) return set_err(SD_ERR_CAPACITY, "cap_points must be at least ceil(W/3) * ceil(H/3)");
    if (words > 64) return set_err(SD_ERR_UNSUPPORTED, "image wider than 12288 pixels");
    if (color_stride < (size_t)3 * W || depth_stride_elems < (size_t)W || (d_mask && mask_stride < (size_t)W)) return set_err(SD_ERR_INVALID, "stride smaller than width");
    hipStream_t s = pick_stream(b, stream_);
    if (n_frames == 0) return SD_OK;
    int rc = check_slots(b, "backproject_dense", slots, nullptr, n_frames, SD_SLOT_RESULTS);
    if (rc == SD_OK) rc = b->cloud.grow(b, s, (size_t)b->maxImages * rows3 * words, rows3);
    if (rc != SD_OK) return rc;
    HIPCHK(hipMemcpyAsync(b->cloud.d_T, Twc_host, (size_t)n_frames * 128, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b->cloud.d_slots, slots, (size_t)n_frames * 4, hipMemcpyHostToDevice, s));
    SdCloudArgs A;
    A.fb = b->d_fb; A.slots = b->cloud.d_slots; A.color = d_color; A.colorStride = color_stride; A.colorPitch = color_pitch;
    A.depth = d_depth; A.depthStride = depth_stride_elems; A.depthPitch = depth_pitch_elems; A.depthFactor = depth_factor;
    A.mask = d_mask; A.maskStride = mask_stride; A.maskPitch = mask_pitch; A.fx = cam->fx; A.fy = cam->fy; A.cx = cam->cx; A.cy = cam->cy;
    A.Twc = b->cloud.d_T; A.W = W; A.H = H; A.cols3 = cols3; A.rows3 = rows3; A.words = words; A.bits = b->cloud.d_bits; A.rowCount = b->cloud.d_rows;
    A.points = (sd_cloud_point_dev*)d_points; A.capPoints = cap_points; A.counts = d_counts;
    hipLaunchKernelGGL(k_cloud_mark, dim3(rows3, n_frames), dim3(256), 0, s, A);
    LAUNCH_CHECK("k_cloud_mark");
    hipLaunchKernelGGL(k_cloud_emit, dim3(rows3, n_frames), dim3(256), 0, s, A);
    LAUNCH_CHECK("k_cloud_emit");
    return SD_OK;
}

#include "sd_tracker.inc"
#include "sd_kfdb.inc"
#include "sd_covis.inc"
#include "sd_reloc.inc"
#include "sd_sim3_opt.inc"
#include "sd_sim3_refine.inc"
#include "sd_pnp.inc"

} // extern "C"
