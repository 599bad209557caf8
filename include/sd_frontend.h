/* sd_frontend.h — C ABI of the MI355X-native per-frame front end (libsd_frontend.so).
 *
 * Drop-in boundary for the hot path of li-guihai/slam-dynamic (an ORB-SLAM2 fork):
 * ORBextractor, the Frame-side stereo/RGB-D association, the 256-bit Hamming matchers
 * and the dynamic-point cull.  The reference has no FFI layer — its boundary is the C++
 * class API in namespace ORB_SLAM2 — so every entry point below names the reference
 * interface it replaces (file:line relative to the reference tree).  Plain pointers and
 * sizes only; no OpenCV, torch or STL types.  All functions return an int status
 * (SD_OK == 0, < 0 on error) and never throw or abort.  The reference-side bindings a
 * maintainer would add are shown in INTEGRATION.md and in
 * slam-dynamic_amd/host/ORBextractor.h (a header-only mirror of the class API).
 *
 * Device model: one process per GPU.  Pointers named d_* are device (HBM) pointers;
 * `stream` is a hipStream_t passed as void* (NULL = the library's own stream).
 */
#ifndef SD_FRONTEND_H
#define SD_FRONTEND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_OK 0
#define SD_ERR_INVALID (-1)     /* bad argument                                             */
#define SD_ERR_NO_DEVICE (-2)   /* no HIP device / HIP runtime unusable (never a CPU fallback) */
#define SD_ERR_HIP (-3)         /* a HIP call failed; see sd_last_error()                   */
#define SD_ERR_CAPACITY (-4)    /* caller buffer too small                                  */
#define SD_ERR_UNSUPPORTED (-5) /* geometry outside what the kernels were sized for         */
#define SD_ERR_STATE (-6)       /* call sequence error (e.g. stereo before extract)         */

/* Same 28-byte layout as cv::KeyPoint {Point2f pt; float size, angle, response; int octave, class_id;}
 * so an adapter can memcpy into std::vector<cv::KeyPoint> (ORBextractor.h:59-61). */
typedef struct sd_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} sd_keypoint;

typedef struct sd_extractor sd_extractor; /* ORB_SLAM2::ORBextractor state (parameters, tables)      */
typedef struct sd_batch sd_batch;         /* device workspace for up to max_images images of one size */

int sd_version(void);
const char* sd_status_string(int status);
const char* sd_last_error(void); /* thread-local text of the last SD_ERR_HIP / SD_ERR_UNSUPPORTED */
int sd_device_count(int* n);     /* hipGetDeviceCount; SD_ERR_NO_DEVICE when none */

/* ---- ORBextractor (include/ORBextractor.h:45-114, src/ORBextractor.cc:410-470) ---- */

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)  ORBextractor.h:51 */
int sd_extractor_create(sd_extractor** out, int nfeatures, float scaleFactor, int nlevels, int iniThFAST,
                        int minThFAST);
int sd_extractor_destroy(sd_extractor* ex);
/* The 7 fixed-point (8.8) taps of GaussianBlur(7x7, sigma 2) (ORBextractor.cc:1086) are a spec
 * parameter (OpenCV-version dependent); default {18,34,48,56,48,34,18}. */
int sd_extractor_set_blur_taps(sd_extractor* ex, const uint16_t taps[7]);
/* GetLevels / GetScaleFactor / GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares  (ORBextractor.h:63-83) + mnFeaturesPerLevel, umax (ORBextractor.h:102-104).
 * Any pointer may be NULL.  scale..inv_sigma2, quota: nlevels entries; umax: 16 entries. */
int sd_extractor_levels(const sd_extractor* ex, int* nlevels, float* scale_factor);
int sd_extractor_tables(const sd_extractor* ex, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                        int32_t* quota, int32_t* umax);
/* Size of mvImagePyramid[level] for a WxH input (ORBextractor.cc:1111-1112). */
int sd_extractor_level_size(const sd_extractor* ex, int width, int height, int level, int* lw, int* lh);

/* ---- batched ORBextractor::operator() (src/ORBextractor.cc:1043-1105) ----
 * One sd_batch owns, in HBM, the 8-level padded pyramid (the public member mvImagePyramid,
 * ORBextractor.h:85), the blurred planes, FAST candidates and the results of up to max_images
 * images of width x height.  Like the reference object it is not re-entrant: one batch per
 * concurrent caller (the reference uses one extractor per eye, Frame.cc:87-90). */
int sd_batch_create(sd_batch** out, sd_extractor* ex, int width, int height, int max_images);
int sd_batch_destroy(sd_batch* b);
int sd_batch_kp_capacity(const sd_batch* b, int* cap); /* max keypoints one image can return */

/* operator()(image, mask [ignored], keypoints, descriptors) for n_images gray images already in
 * HBM: image i starts at d_gray + i*image_pitch, rows `stride` bytes apart.  Asynchronous on
 * `stream`; results stay on the device. */
int sd_batch_extract_device(sd_batch* b, const uint8_t* d_gray, size_t stride, size_t image_pitch, int n_images,
                            void* stream);
/* The same for 3-channel 8-bit input (BGR, or RGB when rgb_order != 0: Camera.RGB): Tracking::GrabImageRGBD / GrabImageStereo's
 * cvtColor (src/Tracking.cc:179-198,259-268) fused into the extractor's level-0 copy (src/ORBextractor.cc:1127-1128), so the
 * gray image is never stored; it is the interior of pyramid level 0 (sd_batch_pyramid_level).  Results are identical to
 * sd_cvt_gray_device followed by sd_batch_extract_device.  `stride` in bytes (>= 3 * width). */
int sd_batch_extract_color_device(sd_batch* b, const uint8_t* d_src, size_t stride, size_t image_pitch, int rgb_order, int n_images,
                                  void* stream);
/* The same for any input Tracking::GrabImage* accepts (src/Tracking.cc:175-200, 187-200: `if(mImGray.channels()==3) ... else
 * if(mImGray.channels()==4)` with CV_RGB2GRAY / CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY): channels = 1 (gray, copied), 3, or 4 (the
 * alpha byte is ignored, same weights).  `stride` in bytes (>= channels * width). */
int sd_batch_extract_pixels_device(sd_batch* b, const uint8_t* d_src, size_t stride, size_t image_pitch, int channels, int rgb_order,
                                   int n_images, void* stream);
/* Same, from host memory (upload + extract + stream sync).  Empty image (NULL / 0 size) => 0 keypoints,
 * as ORBextractor.cc:1046-1047. */
int sd_batch_extract_host(sd_batch* b, const uint8_t* gray, size_t stride, size_t image_pitch, int n_images);

/* Results.  Device views: kp [max_images][cap], desc [max_images][cap][32], count [max_images]. */
int sd_batch_results_device(sd_batch* b, sd_keypoint** d_kp, uint8_t** d_desc, int32_t** d_count, int* cap);
int sd_batch_counts(sd_batch* b, int32_t* counts, int n_images);           /* syncs the stream */
int sd_batch_download(sd_batch* b, int image, sd_keypoint* kp, uint8_t* desc, int cap, int* n,
                      int32_t* per_level /* nlevels or NULL */);
/* mvImagePyramid[level] of image `image`: device pointer to the interior (x=0,y=0) pixel; the 19-px
 * BORDER_REFLECT_101 frame lies at negative offsets (ORBextractor.cc:1107-1130). */
int sd_batch_pyramid_level(sd_batch* b, int image, int level, const uint8_t** d_interior, int* w, int* h,
                           size_t* stride);
/* Copy the padded plane ((h+38) x (w+38), tightly packed) / the blurred interior plane (h x w) to host. */
int sd_batch_download_pyramid(sd_batch* b, int image, int level, uint8_t* padded_out);
int sd_batch_download_blurred(sd_batch* b, int image, int level, uint8_t* out);
/* Number of FAST candidates per level before the quadtree (vToDistributeKeys.size(), ORBextractor.cc:829) */
int sd_batch_candidate_counts(sd_batch* b, int image, int32_t* per_level);

/* ---- Frame::ComputeStereoMatches (src/Frame.cc:874-1048) ----
 * The batch must hold n_frames stereo pairs extracted as images 2f (left) and 2f+1 (right).
 * mbf = Camera.bf, fx = Camera.fx (mb = mbf/fx, Frame.cc:228).  Outputs per left keypoint, stored at the
 * LEFT image's slot (image index 2f) of the [max_images][cap] arrays. */
int sd_batch_stereo_match(sd_batch* b, int n_frames, float mbf, float fx, void* stream);
int sd_batch_stereo_device(sd_batch* b, float** d_uright, float** d_depth, int* cap); /* [max_images][cap] */
int sd_batch_download_stereo(sd_batch* b, int frame, float* uright, float* depth, int32_t* sad_dist, int cap);

/* ---- Frame::ComputeStereoFromRGBD (src/Frame.cc:1051-1072) + depth scaling (Tracking.cc:271-272) ----
 * d_depth: 16-bit depth images (rows `stride_elems` elements apart); depth_factor = 1/DepthMapFactor.
 * Fuses imDepth.convertTo(CV_32F, factor) with the per-keypoint lookup (undistortion is the identity
 * when k1 == 0, Frame.cc:814-818).  One image per frame. */
int sd_batch_rgbd_from_u16(sd_batch* b, const uint16_t* d_depth, size_t stride_elems, size_t image_pitch_elems,
                           int n_images, float depth_factor, float mbf, void* stream);
int sd_batch_rgbd_from_f32(sd_batch* b, const float* d_depth, size_t stride_elems, size_t image_pitch_elems,
                           int n_images, float mbf, void* stream);
/* CV_32F depth that still has to be scaled: `if((fabs(mDepthMapFactor-1.0f)>1e-5) || imDepth.type()!=CV_32F) imDepth.convertTo(imDepth,
 * CV_32F, mDepthMapFactor)` (Tracking.cc:271-272) for a CV_32F input and a factor other than 1: d = depth * depth_factor in f32. */
int sd_batch_rgbd_from_f32_scaled(sd_batch* b, const float* d_depth, size_t stride_elems, size_t image_pitch_elems, int n_images,
                                  float depth_factor, float mbf, void* stream);
int sd_batch_download_rgbd(sd_batch* b, int image, float* uright, float* depth, int cap);


/* ---- Frame statics (include/Frame.h:160-210): intrinsics, stereo baseline, undistorted image bounds ---- */
typedef struct sd_camera {
    float fx, fy, cx, cy, mbf, mb;               /* mb = mbf/fx (Frame.cc:228) */
    float mnMinX, mnMaxX, mnMinY, mnMaxY;        /* Frame::ComputeImageBounds (Frame.cc:844-872) */
} sd_camera;

/* Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cc:463-478,790-800): the 64x48 grid cell of every
 * keypoint (posX*48 + posY, or -1 outside).  The device form of mGrid: per-cell lists are implied by
 * (cell, keypoint index) order, which is the visiting order of GetFeaturesInArea (Frame.cc:735-788). */
int sd_batch_assign_grid(sd_batch* b, int n_images, const sd_camera* cam, void* stream);
int sd_batch_download_grid(sd_batch* b, int image, int16_t* cell, int cap);
/* The sorted form of the grid that the window matchers walk: sorted_idx[0 .. *n_in_grid) = the indices of the in-grid keypoints
 * ordered by (cell, index); cell_start[c] = the number of in-grid keypoints in cells below c, c = 0 .. 3072 (3073 entries,
 * cell_start[3072] == *n_in_grid).  Read-only.  SD_ERR_STATE if sd_batch_assign_grid has not run on what the slot holds,
 * SD_ERR_CAPACITY (with *n_in_grid set) if cap < *n_in_grid. */
int sd_batch_download_grid_index(sd_batch* b, int image, uint16_t* sorted_idx, int cap, uint16_t* cell_start, int* n_in_grid);

/* Frame::UnprojectStereo (src/Frame.cc:1074-1088) for every keypoint of frames first_image + k*image_step,
 * k < n_frames, using the depth of the preceding stereo / RGB-D step.  Twc_host: n_frames row-major 4x4
 * [mRwc | mOw].  Fills the batch's map-point table: world position + flags (bit0 valid, bit1 = the map
 * point has Observations() > 0, never set here).  first_image must be 0. */
int sd_batch_unproject(sd_batch* b, int first_image, int image_step, int n_frames, const sd_camera* cam,
                       const float* Twc_host, void* stream);
/* The map-point table ([max_images][cap][3] f32, [max_images][cap] u8): a caller that owns real MapPoints
 * (Tracking) writes LastFrame.mvpMapPoints[i]->GetWorldPos() / flags here instead of calling unproject. */
int sd_batch_mappoints_device(sd_batch* b, float** d_xw, uint8_t** d_flags, int* cap);
int sd_batch_set_mappoints(sd_batch* b, int image, const float* xw, const uint8_t* flags, int n);
int sd_batch_download_mappoints(sd_batch* b, int image, float* xw, uint8_t* flags, int cap);

/* ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th, bMono[, points_last, points_current])
 * (src/ORBmatcher.cc:1485-1627 and the pair-emitting overload :407-559, called from Tracking::TrackHomo,
 * Tracking.cc:998-1010, and TrackWithMotionModel).  Pair p matches Current = slot cur_index[p] against
 * Last = slot last_index[p] of the same batch (host index arrays; sd_batch_assign_grid must have run on the
 * Current slots).  Tcw_host / Tlw_host: n_pairs row-major 4x4 poses (CurrentFrame.mTcw, LastFrame.mTcw).
 * d_occupied (nullable, [n_pairs][cap] u8): CurrentFrame.mvpMapPoints[i2] already holds a point with
 * Observations() > 0.  d_mp_desc (nullable, [max_images][cap][32]): pMP->GetDescriptor() of the Last frame's
 * points; NULL = the Last frame's own descriptors.
 * Results: match[i2] = index of the Last-frame point assigned to Current keypoint i2 or -1 (the new
 * CurrentFrame.mvpMapPoints); pairs = (i, i2) in order of i == points_last / points_current BEFORE the
 * rotation-histogram cull (ORBmatcher.cc:505-506); nmatches = the function's return value. */
int sd_batch_search_by_projection(sd_batch* b, int n_pairs, const int32_t* cur_index, const int32_t* last_index,
                                  const float* Tcw_host, const float* Tlw_host, const sd_camera* cam, float th, int bMono,
                                  int checkOrientation, const uint8_t* d_occupied, const uint8_t* d_mp_desc, void* stream);
/* Tracking::SearchLocalPoints (src/Tracking.cc:2014-2064) = Frame::isInFrustum(pMP, viewing_cos_limit)
 * (src/Frame.cc:677-733) for every local map point, then ORBmatcher::SearchByProjection(Frame& F, const
 * vector<MapPoint*>& vpMapPoints, th) with mfNNratio = nnratio (src/ORBmatcher.cc:45-129; the caller passes th = 1,
 * 3 for RGB-D, 5 after a relocalisation, Tracking.cc:2055-2063).  Frame f < n_frames is batch slot frame_index[f]
 * (sd_batch_assign_grid must have run on it) with local map points [point_offset[f], point_offset[f+1]) of the flat
 * device arrays d_points / d_point_desc (pMP->GetDescriptor(), 32 B each), pose Tcw_host[f] (row-major 4x4 mTcw).
 * d_occupied (nullable, [n_frames][cap] u8): F.mvpMapPoints[i] already holds a point with Observations() > 0.
 * Outputs (device): d_track[m] = mbTrackInView / mTrackProjX / mTrackProjY / mTrackProjXR / mnTrackScaleLevel /
 * mTrackViewCos; d_point_match[m] = keypoint index given to point m or -1; d_kp_match[f][i] (row stride =
 * sd_batch cap) = index, relative to point_offset[f], of the point this call leaves in F.mvpMapPoints[i], or -1;
 * d_nmatches[f] = the function's return value. */
typedef struct sd_map_point {
    float xw[3];          /* GetWorldPos() */
    float normal[3];      /* GetNormal() */
    float min_distance;   /* mfMinDistance (GetMinDistanceInvariance() / 0.8f) */
    float max_distance;   /* mfMaxDistance (GetMaxDistanceInvariance() / 1.2f) */
    uint32_t flags;       /* bit0: !isBad() && mnLastFrameSeen != F.mnId; bit1: Observations() > 0 */
} sd_map_point;           /* 36 bytes */
typedef struct sd_track_info { float proj_x, proj_y, proj_xr, view_cos; int32_t level; int32_t in_view; } sd_track_info;   /* 24 bytes */
int sd_batch_search_local_map(sd_batch* b, int n_frames, const int32_t* frame_index, const int32_t* point_offset,
                              const sd_map_point* d_points, const uint8_t* d_point_desc, const float* Tcw_host,
                              const sd_camera* cam, float th, float nnratio, float viewing_cos_limit,
                              const uint8_t* d_occupied, sd_track_info* d_track, int32_t* d_point_match,
                              int32_t* d_kp_match, int32_t* d_nmatches, void* stream);
/* ---- Optimizer::PoseOptimization (src/Optimizer.cc:239-451; the vendored g2o's Levenberg-Marquardt) ----
 * Pose-only bundle adjustment of many independent frames in one launch, as TrackReferenceKeyFrame, TrackWithMotionModel,
 * TrackLocalMap and Relocalization call it (src/Tracking.cc:1636,1759,1801,2311).  One edge per frame keypoint i with
 * mvpMapPoints[i] != NULL, in keypoint order (the edges' insertion order, which orders g2o's sums): xw = pMP->GetWorldPos(),
 * (u, v) = mvKeysUn[i].pt, ur = mvuRight[i] (< 0: monocular edge, else stereo), inv_sigma2 = mvInvLevelSigma2[mvKeysUn[i].octave],
 * kp_index = i (carried, not read by the solver). */
typedef struct sd_pose_edge {
    float xw[3];
    float u, v, ur;
    float inv_sigma2;
    int32_t kp_index;
} sd_pose_edge;                                   /* 32 bytes */
/* Problem p owns edges [d_edge_offset[p], d_edge_offset[p+1]) of d_edges; cams [n_problems] (host): fx, fy, cx, cy, mbf of the
 * frame; d_Tcw [n_problems][16] row-major f32: pFrame->mTcw in, the optimised pose out (untouched when the problem has fewer than
 * 3 edges); d_outlier [edges] u8 = mvbOutlier of each edge; d_n_good [n_problems] = the function's return value
 * (nInitialCorrespondences - nBad).  Asynchronous on `stream`, except that the cameras go through a ring of 8 library-owned device
 * tables per device: a call waits on the host until the launch that used its table 8 calls earlier on the same device has finished. */
int sd_pose_optimize_device(int n_problems, const int32_t* d_edge_offset, const sd_pose_edge* d_edges, const sd_camera* cams,
                            float* d_Tcw, uint8_t* d_outlier, int32_t* d_n_good, void* stream);
/* The same from host arrays (edge_offset [n_problems + 1], edges, Tcw in / out, outlier, n_good): uploads, runs, synchronises. */
int sd_pose_optimize_host(int n_problems, const int32_t* edge_offset, const sd_pose_edge* edges, const sd_camera* cams,
                          float* Tcw, uint8_t* outlier, int32_t* n_good);
/* ---- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:453-778) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:330-371) ----
 * Many independent local bundle adjustments in one launch, from the point where the reference calls initializeOptimization():
 * optimize(5) with Huber kernels, classification (chi2 > 5.991 | 7.815 or non-positive depth -> level 1), optimize(10) over the
 * level-0 edges without kernels, the same test once more (the erase flag), then normal and distance of the optimised points.
 * pbStopFlag is not modelled: the caller tests it before the call (DESIGN Q32-Q38).  A problem is three tables:
 *   keyframes: lLocalKeyFrames first (n_local of them), then lFixedCameras.  Tcw = GetPose() row-major; fx .. mbf as the edges take
 *              them from pKFi; fixed = (mnId == 0) for a local keyframe, ignored (always fixed) for a fixed camera.  Table order is
 *              the order of the pose blocks in the reduced camera system.
 *   points:    xw = GetWorldPos() in lLocalMapPoints order; every point is marginalised.
 *   edges:     in insertion order (which orders the sums).  kf / point index the problem's own tables; ur < 0 = monocular edge;
 *              inv_sigma2 = mvInvLevelSigma2[octave]; tag is carried, not read. */
typedef struct sd_ba_keyframe {
    float Tcw[16];
    float fx, fy, cx, cy, mbf;
    uint8_t fixed;
    uint8_t reserved[3];
} sd_ba_keyframe;                                 /* 88 bytes */
typedef struct sd_ba_edge {
    int32_t kf, point;
    float u, v, ur;
    float inv_sigma2;
    int32_t tag;
    int32_t reserved;
} sd_ba_edge;                                     /* 32 bytes */
/* Per problem; index 0 = optimize(5), 1 = optimize(10).  iterations: LM iterations run; trials: linear solves tried; rejected: trials
 * undone; chi2: the active chi2 the round ended with; n_level1 / n_erased: edges the two classifications flagged.
 * iterations = {-1, -1} marks a problem whose device tables held an index out of range (device entry point only): nothing else of
 * that problem is written. */
typedef struct sd_ba_stats {
    int32_t iterations[2], trials[2], rejected[2];
    int32_t n_level1, n_erased;
    double chi2[2];
} sd_ba_stats;                                    /* 48 bytes */
#define SD_BA_MAX_LOCAL_KEYFRAMES 64
#define SD_BA_MAX_FIXED_KEYFRAMES 128
#define SD_BA_MAX_POINTS_PER_PROBLEM 8192
#define SD_BA_MAX_EDGES_PER_PROBLEM 65536
/* Problem p owns keyframes [kf_offset[p], kf_offset[p+1]) (the first n_local[p] local), points [point_offset[p], ..) and edges
 * [edge_offset[p], ..); the four tables are HOST arrays (n_problems + 1, n_problems, n_problems + 1, n_problems + 1 entries), every
 * d_ array is device memory.  d_ref_kf [points]: keyframe index of the point's reference keyframe for the distance, -1 = skip.
 * Out: d_Tcw [keyframes][16]: Converter::toCvMat of the optimised pose in the rows of LOCAL keyframes (rows of fixed cameras are not
 * written); d_xw_out [points][3]; d_normal [points][3] = mean over the point's edges that were not erased of the unit vector from
 * the keyframe's centre (zero when none is left); d_dist [points] = |xw - Ow(ref_kf)| or -1; d_level1 / d_erase [edges] u8; d_stats
 * [n_problems].  A problem without edges is a no-op: poses and points come back as given.  Anything over the caps above, offsets
 * that decrease or n_local beyond the problem's keyframes: SD_ERR_INVALID before anything is launched.
 * Stateless with respect to sd_batch.  Asynchronous on `stream`: no host synchronisation, except that the problem table goes through
 * a ring of 8 library-owned device tables per device (as the cameras of sd_pose_optimize_device) and that the library-owned workspace
 * is shared by the calls on one device -- a call waits on the device for the previous one, and on the host only when the workspace
 * has to grow. */
int sd_local_ba_device(int n_problems, const int32_t* kf_offset, const int32_t* n_local, const int32_t* point_offset,
                       const int32_t* edge_offset, const sd_ba_keyframe* d_kfs, const float* d_xw, const sd_ba_edge* d_edges,
                       const int32_t* d_ref_kf, float* d_Tcw, float* d_xw_out, float* d_normal, float* d_dist, uint8_t* d_level1,
                       uint8_t* d_erase, sd_ba_stats* d_stats, void* stream);
/* The same from host arrays: checks every edge's and ref_kf's index (out of range: SD_ERR_INVALID, nothing launched), uploads, runs,
 * synchronises. */
int sd_local_ba_host(int n_problems, const int32_t* kf_offset, const int32_t* n_local, const int32_t* point_offset,
                     const int32_t* edge_offset, const sd_ba_keyframe* kfs, const float* xw, const sd_ba_edge* edges,
                     const int32_t* ref_kf, float* Tcw, float* xw_out, float* normal, float* dist, uint8_t* level1, uint8_t* erase,
                     sd_ba_stats* stats);
/* Profiling (a developer switch, off by default, process-wide): with it on, every sd_local_ba_device call also records, per problem, the
 * device wall-clock time its workgroup spent in each phase, summed over both rounds and all LM trials: 0 index lists, 1 linearisation
 * (edge records and the gathers of Hpp / Hll), 2 Schur assembly (landmark inverses, S, b_schur), 3 factorisation, 4 the triangular
 * solves and the landmark back-substitution, 5 update and chi2.  The marks add one barrier each, so a profiled call is slightly slower.
 * sd_local_ba_profile waits for the last profiled call on the current device and returns its figures in milliseconds
 * (ms [n_problems][SD_BA_PROFILE_PHASES]); SD_ERR_STATE when there is none, SD_ERR_INVALID when n_problems is not that call's. */
#define SD_BA_PROFILE_PHASES 6
int sd_local_ba_set_profiling(int on);
int sd_local_ba_profile(int n_problems, double* ms);
/* ---- Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc), as LoopClosing::ComputeSim3 drives it (src/LoopClosing.cc:232-400) ----
 * Up to SD_SIM3_MAX_PROBLEMS independent Sim3Solver problems in one launch sequence: the 3-point Horn RANSAC of one (keyframe, loop candidate)
 * pair each.  A problem is what the constructor gathers (Sim3Solver.cc:36-112): one record per kept correspondence, in i1 order --
 * xw1 / xw2 = GetWorldPos() of pMP1 / pMP2, sigma2_1 / sigma2_2 = mvLevelSigma2[octave] of the two key points, tag = i1 (carried,
 * never read) -- plus Tcw1 / Tcw2 = GetPose() row-major, the two cameras (mK1, mK2), bFixScale and a 64-bit seed.  The sampler is
 * counter-based (DUtils::Random's rand() stream cannot be specified): draw d of iteration it is sd_splitmix64 of (seed, it, d)
 * reduced modulo the current size of vAvailableIndices and mapped through the swap-with-back removal of :163-177 (DESIGN Q39). */
typedef struct sd_sim3_corr {
    float xw1[3], xw2[3];
    float sigma2_1, sigma2_2;
    int32_t tag;
} sd_sim3_corr;                                   /* 36 bytes */
typedef struct sd_sim3_problem {
    float Tcw1[16], Tcw2[16];
    float fx1, fy1, cx1, cy1;                     /* pKF1->mK */
    float fx2, fy2, cx2, cy2;                     /* pKF2->mK */
    int32_t fix_scale;                            /* mbFixScale */
    int32_t reserved;
    uint64_t seed;
} sd_sim3_problem;                                /* 176 bytes */
/* What find() == iterate(mRansacMaxIts) leaves (Sim3Solver.cc:140-213).  found = 1: the hypothesis of the LOWEST iteration whose
 * inlier count is > min_inliers (:183-199); iteration is its 1-based index (mnIterations at the return), n_inliers its count, no_more
 * = 0.  found = 0: no_more = 1 and iteration / n_inliers / T12 .. s12 are mnBestInliers / mBestT12 ..: the largest count and, among
 * equal counts, the LATEST iteration (:183 compares with >=).  A problem with fewer correspondences than min_inliers (:146-150), or
 * fewer than the 3 a sample needs, runs no hypothesis: found = 0, no_more = 1, iteration = 0, everything else zero.
 * max_its = mRansacMaxIts after SetRansacParameters (:114-138).  T12 = [s12 R12 | t12] row-major 4x4. */
typedef struct sd_sim3_result {
    int32_t found, no_more, iteration, n_inliers, max_its, reserved;
    float T12[16], R12[9], t12[3], s12;
} sd_sim3_result;                                 /* 140 bytes */
#define SD_SIM3_MAX_CORRESPONDENCES 4096          /* per problem */
#define SD_SIM3_MAX_ITERATIONS 4096               /* max_iterations */
#define SD_SIM3_MAX_PROBLEMS 65535                /* per call */
/* Problem p owns correspondences [corr_offset[p], corr_offset[p+1]) of d_corr; corr_offset [n_problems + 1] and problems
 * [n_problems] are HOST arrays, d_ arrays device memory.  probability / min_inliers / max_iterations: SetRansacParameters' arguments
 * (the reference passes 0.99, 20, 300); its formula is evaluated on the host as written and the effective count comes back in
 * max_its_out [n_problems] (host, nullable) and in every result.  Out: d_results [n_problems]; d_inliers [correspondences] u8, indexed
 * like d_corr: entry e is vbInliers[d_corr[e].tag] of find() (the winning hypothesis' mask; all zero when found = 0).
 * More than SD_SIM3_MAX_PROBLEMS problems, more than SD_SIM3_MAX_CORRESPONDENCES in a problem, max_iterations outside
 * [1, SD_SIM3_MAX_ITERATIONS], min_inliers < 0, probability outside (0, 1), offsets that do not start at 0 or decrease: SD_ERR_INVALID before anything is launched, never a
 * truncation.  Stateless with respect to sd_batch.  Asynchronous on `stream` with no host synchronisation, except that the problem
 * table goes through a ring of 8 library-owned device tables per device and the library-owned workspace (grown with the largest call
 * seen) is shared by the calls on one device, as for sd_local_ba_device. */
int sd_sim3_ransac_device(int n_problems, const int32_t* corr_offset, const sd_sim3_corr* d_corr, const sd_sim3_problem* problems,
                          double probability, int min_inliers, int max_iterations, sd_sim3_result* d_results, uint8_t* d_inliers,
                          int32_t* max_its_out, void* stream);
/* The same from host arrays: uploads, runs, synchronises. */
int sd_sim3_ransac_host(int n_problems, const int32_t* corr_offset, const sd_sim3_corr* corr, const sd_sim3_problem* problems,
                        double probability, int min_inliers, int max_iterations, sd_sim3_result* results, uint8_t* inliers);
/* ---- PnPsolver (include/PnPsolver.h, src/PnPsolver.cc), as Tracking::Relocalization drives it (src/Tracking.cc:2256-2309) ----
 * Up to SD_PNP_MAX_PROBLEMS independent PnPsolver problems in one launch sequence: the 4-point EPnP RANSAC with Refine of one (lost frame,
 * candidate key frame) pair each (DESIGN Q46).  A problem is what the constructor gathers (PnPsolver.cc:67-110): one record per kept
 * correspondence, in key-point order -- xw = mvP3Dw, uv = mvP2D (mvKeysUn[i].pt), sigma2 = mvLevelSigma2[octave], tag = i (carried,
 * never read) -- plus fx fy cx cy, a 64-bit seed, start_iteration = mnIterations on entry (0 for a first call) and n_iterations = the
 * argument of iterate (the reference passes 5).  The sampler is Q39's: draw d of iteration it is sd_splitmix64(sd_splitmix64(seed) +
 * 4 it + d) modulo the current size of vAvailableIndices, mapped through the swap-with-back removal of :188-201. */
typedef struct sd_pnp_corr {
    float xw[3];
    float uv[2];
    float sigma2;
    int32_t tag;
} sd_pnp_corr;                                    /* 28 bytes */
typedef struct sd_pnp_problem {
    float fx, fy, cx, cy;                         /* F.fx .. F.cy (:104-107) */
    uint64_t seed;
    int32_t start_iteration, n_iterations;
} sd_pnp_problem;                                 /* 32 bytes */
/* What iterate(n_iterations) leaves (PnPsolver.cc:165-258).  The loop condition `mnIterations < mRansacMaxIts || nCurrentIterations <
 * nIterations` makes a call run iterations start + 1 .. end, end = max(max_its, start_iteration + n_iterations): a first call is find().
 *   kind 1  Refine() succeeded (:226-236): Tcw = mRefinedTcw, n_inliers = mnRefinedInliers, the mask is mvbRefinedInliers, iteration =
 *           mnIterations at the return (the lowest it in (start, end] with count >= min_inliers whose best passes Refine), no_more = 0
 *   kind 2  nothing refined but a best exists (:241-255): Tcw = mBestTcw, n_inliers = mnBestInliers, the best mask, no_more = 1
 *   kind 0  empty pose (N < min_inliers, :173-177, or no hypothesis reached min_inliers): no_more = 1, Tcw and the mask zero
 * best_iteration / best_inliers: the iteration that set mnBestInliers (the EARLIEST of equal counts, :212 is strict; 0 = none) and its
 * count; n_refines: Refine() evaluations of this call (one per distinct best).  min_inliers / max_its: mRansacMinInliers / mRansacMaxIts
 * after SetRansacParameters (:121-157).  Tcw row-major 4x4, R and t narrowed to f32 once. */
typedef struct sd_pnp_result {
    int32_t kind, no_more, iteration, n_inliers, best_iteration, best_inliers, n_refines, min_inliers, max_its, reserved;
    float Tcw[16];
} sd_pnp_result;                                  /* 104 bytes */
#define SD_PNP_MAX_CORRESPONDENCES 4096           /* per problem */
#define SD_PNP_MAX_ITERATIONS 4096                /* max_iterations, and start_iteration + n_iterations */
#define SD_PNP_MAX_PROBLEMS 65535                 /* per call */
/* Problem p owns correspondences [corr_offset[p], corr_offset[p+1]) of d_corr; corr_offset [n_problems + 1] and problems [n_problems]
 * are HOST arrays, d_ arrays device memory.  probability .. th2: SetRansacParameters' six arguments (the reference passes 0.99, 10, 300,
 * 4, 0.5, 5.991), evaluated on the host as written (:121-157).  Out: d_results [n_problems]; d_inliers [correspondences] u8, indexed like
 * d_corr: entry e is vbInliers[d_corr[e].tag] of the returned kind.  d_counts (nullable, device, [n_problems * counts_stride] int32):
 * a debug copy of the inlier counts, row p holding mnInliersi of iterations 1 .. end in [0, end) (end = 0 for a problem that runs none);
 * counts_stride must then be >= every end.  d_poses (nullable, device, [n_problems * counts_stride * 12] f64): the hypotheses themselves,
 * mRi row-major then mti, laid out like d_counts.
 * min_set != 4, more than SD_PNP_MAX_PROBLEMS problems, more than SD_PNP_MAX_CORRESPONDENCES in a problem, max_iterations or
 * start_iteration + n_iterations outside [1, SD_PNP_MAX_ITERATIONS], start_iteration < 0, n_iterations < 1, min_inliers < 0, probability
 * outside (0, 1), epsilon outside (0, 1], th2 <= 0, offsets that do not start at 0 or decrease: SD_ERR_INVALID before anything is
 * launched, never a truncation.  Stateless with respect to sd_batch.  Asynchronous on `stream` with no host synchronisation, except that
 * the problem table goes through a ring of 8 library-owned device tables per device and the library-owned workspace (grown with the
 * largest call seen) is shared by the calls on one device, as for sd_sim3_ransac_device. */
int sd_pnp_ransac_device(int n_problems, const int32_t* corr_offset, const sd_pnp_corr* d_corr, const sd_pnp_problem* problems,
                         double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2,
                         sd_pnp_result* d_results, uint8_t* d_inliers, int32_t* d_counts, double* d_poses, int counts_stride, void* stream);
/* The same from host arrays: uploads, runs, synchronises.  counts / poses (nullable, host) as d_counts / d_poses. */
int sd_pnp_ransac_host(int n_problems, const int32_t* corr_offset, const sd_pnp_corr* corr, const sd_pnp_problem* problems,
                       double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2,
                       sd_pnp_result* results, uint8_t* inliers, int32_t* counts, double* poses, int counts_stride);
/* ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241), as LoopClosing::ComputeSim3 calls it after SearchBySim3 (:326) ----
 * Up to SD_SIM3_MAX_PROBLEMS independent problems in one launch: one free Sim3 vertex, two projection edges per correspondence
 * (x1 = S12 X2 and x2 = S12^-1 X1), Huber with delta = (float)sqrt(th2), g2o's Levenberg-Marquardt with NUMERIC Jacobians (delta =
 * 1e-9), optimize(5), the chi2 classification, optimize(5 or 10) and the final count, all in one kernel (DESIGN Q45).
 * A correspondence is one that passed the `continue`s of :1101-1136 (the caller applies them, as for sd_sim3_ransac_*), in i order:
 * xw1 / xw2 = GetWorldPos() of pMP1 / pMP2, obs1 / obs2 = mvKeysUn[i].pt / mvKeysUn[i2].pt, inv_sigma2_1 / _2 =
 * mvInvLevelSigma2[octave] of the two key points, tag = i (carried, never read).  Camera coordinates are R * xw + t of Tcw1 / Tcw2 in
 * f32, the statement sd_sim3_ransac_* uses.  R12 (row-major 3x3) / t12 / s12: the prior g2oS12 = Sim3(R, t, s). */
typedef struct sd_sim3_opt_corr {
    float xw1[3], xw2[3];
    float obs1[2], obs2[2];
    float inv_sigma2_1, inv_sigma2_2;
    int32_t tag;
} sd_sim3_opt_corr;                               /* 52 bytes */
typedef struct sd_sim3_opt_problem {
    float Tcw1[16], Tcw2[16];
    float fx1, fy1, cx1, cy1;                     /* pKF1->mK */
    float fx2, fy2, cx2, cy2;                     /* pKF2->mK */
    float R12[9], t12[3], s12;
    float th2;
    int32_t fix_scale;                            /* bFixScale */
} sd_sim3_opt_problem;                            /* 220 bytes */
/* ret = the return value (nIn, or 0 from `if (nCorrespondences - nBad < 10) return 0`); n_bad = nBad of the first check;
 * more_iterations = nMoreIterations; per optimize() call r: iterations[r] = LM iterations run, trials[r] = solves (the sum of
 * qmax), stop[r] = SD_SIM3_OPT_STOP_*.  written = 1 when g2oS12 was assigned (:1238): q (x y z w) / t / s are then the estimate, else
 * the prior as Sim3(R12, t12, s12) holds it -- the `return 0` path leaves g2oS12 alone but keeps the matches it set to NULL.
 * T12 = [s R | t] row-major 4x4 in f32 (Converter::toCvSE3(s * R, t)). */
#define SD_SIM3_OPT_STOP_OK 0                     /* every iteration returned OK */
#define SD_SIM3_OPT_STOP_TRIALS 1                 /* Terminate: ten trials after a failure */
#define SD_SIM3_OPT_STOP_RHO_ZERO 2               /* Terminate: rho == 0 */
#define SD_SIM3_OPT_STOP_NO_GAIN 3                /* Terminate: _nBad >= 3 */
typedef struct sd_sim3_opt_result {
    int32_t ret, n_correspondences, n_bad, more_iterations;
    int32_t iterations[2], trials[2], stop[2], written, reserved;
    double q[4], t[3], s;
    float T12[16];
} sd_sim3_opt_result;                             /* 176 bytes */
/* Problem p owns correspondences [corr_offset[p], corr_offset[p+1]) of d_corr; corr_offset [n_problems + 1] and problems
 * [n_problems] are HOST arrays, d_ arrays device memory.  Out: d_results [n_problems]; d_state [correspondences] u8, indexed like
 * d_corr: 0 = inlier at the end, 1 = removed by the first check (vpMatches1[i] = NULL, edges removed), 2 = set to NULL by the
 * last check.  More than SD_SIM3_MAX_PROBLEMS problems, more than SD_SIM3_MAX_CORRESPONDENCES in a problem, th2 not > 0, a
 * non-finite R12 / t12 / s12, offsets that do not start at 0 or decrease: SD_ERR_INVALID before anything is launched, never a
 * truncation.  Stateless with respect to sd_batch; asynchronous on `stream` with no host synchronisation, the problem table going
 * through a ring of 8 library-owned device tables per device as for sd_sim3_ransac_device.  A problem's bytes do not depend on what
 * shares its launch or on its position in it. */
int sd_sim3_optimize_device(int n_problems, const int32_t* corr_offset, const sd_sim3_opt_corr* d_corr,
                            const sd_sim3_opt_problem* problems, sd_sim3_opt_result* d_results, uint8_t* d_state, void* stream);
/* The same from host arrays: uploads, runs, synchronises. */
int sd_sim3_optimize_host(int n_problems, const int32_t* corr_offset, const sd_sim3_opt_corr* corr, const sd_sim3_opt_problem* problems,
                          sd_sim3_opt_result* results, uint8_t* state);
/* ---- LoopClosing::ComputeSim3 after the RANSAC (src/LoopClosing.cc:312-340) as ONE launch sequence for n_jobs (keyframe, candidate)
 * jobs of a batch, without a host round trip (DESIGN Q45): per job, from the RANSAC's answer d_ransac[job] (device, as
 * sd_sim3_ransac_device leaves it; a job with found == 0 does not run),
 *   1. vpMapPointMatches[i1] = vbInliers ? the BoW match : NULL -- from d_bow12 [n_jobs][cap] (the KF-KF SearchByBoW result in
 *      d_matched12's encoding: idx2 = GetIndexInKeyFrame(pKF2), -2 when the point is not in KF2, -1 NULL) and the RANSAC's d_corr (tag =
 *      i1) / d_inliers, rows [corr_offset[job], corr_offset[job + 1]) (corr_offset is a HOST array),
 *   2. SearchBySim3 at `th` (the reference passes 7.5) with R12 / t12 / s12 of d_ransac[job]; the pairs it adds are merged
 *      (vpMatches12[i1] = vpMapPoints2[idx2]),
 *   3. the correspondences of OptimizeSim3, built in i1 order: GetMapPointMatches()[i1] and the match's point both non-NULL and not
 *      bad, i2 = the match's index in KF2 inside [0, N2) (-2 is skipped, Optimizer.cc:1114), mvKeysUn, octave -> mvInvLevelSigma2, xw,
 *   4. OptimizeSim3 with th2 (the reference passes 10) and fix_scale, both cameras = `cam` as in sd_batch_search_by_sim3,
 *   5. matched = ret >= 20,  6. Scw = gScm * gSmw in f64, gSmw = Sim3(Quaterniond(R2w), t2w, 1), and its f32 4x4 [s R | t].
 * Every other argument follows sd_batch_search_by_sim3 (slots with sd_batch_assign_grid done, Tcw1 / Tcw2 host [n_jobs][16], the point
 * table, d_kf1_point / d_kf2_point [n_jobs][cap]), including its answer-or-refuse rule: a point index outside [-1, n_points) turns every
 * download of the call into SD_ERR_INVALID.  The `break` over candidates and the round-robin bookkeeping stay with the caller. */
typedef struct sd_sim3_refine_result {
    int32_t ran, matched, n_built, reserved;      /* ran: d_ransac[job].found; n_built: correspondences handed to the optimiser */
    double Scw_q[4], Scw_t[3], Scw_s;             /* mg2oScw (rotation x y z w); meaningful when matched */
    float Scw[16];                                /* mScw = Converter::toCvMat(mg2oScw) */
    sd_sim3_opt_result opt;                       /* step 4: ret, n_bad, ..., gScm */
} sd_sim3_refine_result;                          /* 320 bytes */
int sd_batch_compute_sim3_refine(sd_batch* b, int n_jobs, const int32_t* kf1_index, const int32_t* kf2_index, const float* Tcw1_host,
                                 const float* Tcw2_host, const sd_sim3_result* d_ransac, const int32_t* corr_offset, const sd_sim3_corr* d_corr,
                                 const uint8_t* d_inliers, const int32_t* d_bow12, const sd_camera* cam, float th, float th2, int fix_scale,
                                 const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points, const int32_t* d_kf1_point,
                                 const int32_t* d_kf2_point, void* stream);
/* Job `job` of the last call (synchronises).  result (nullable); final12 [cap] (nullable): the final vpMapPointMatches per KF1 feature in
 * d_matched12's encoding (idx2, -2, or -1 for NULL: never matched, or set to NULL by either check of the optimiser). */
int sd_batch_download_sim3_refine(sd_batch* b, int job, sd_sim3_refine_result* result, int32_t* final12, int cap);
/* One stage at a time, so that a test can feed each stage's input to a reference: merged12 [cap] = step 1's row (SearchBySim3's
 * vpMatches12); the search's own output through sd_batch_download_sim3_matches(job); corr [cap] / state [cap] (nullable) = step 3's
 * correspondences and the optimiser's state bytes, *n_built of them. */
int sd_batch_download_sim3_refine_stages(sd_batch* b, int job, int32_t* merged12, sd_sim3_opt_corr* corr, uint8_t* state, int cap, int* n_built);
/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:1259-1483; LoopClosing.cc:362 passes th =
 * 7.5) for n_pairs independent (KF1 slot, KF2 slot) pairs of one batch; sd_batch_assign_grid must have run on both slots of every
 * pair (SD_ERR_STATE otherwise).  Host, per pair: kf1_index / kf2_index (slots), Tcw1 / Tcw2 (GetPose(), row-major 4x4), s12, R12
 * (row-major 3x3), t12.  `cam` serves both directions, as the reference takes fx .. cy from pKF1 for both (:1262-1265).
 * Device: the point table d_points / d_point_desc (GetDescriptor(), 32 B each) of n_points entries as for sd_batch_fuse (xw and
 * min_distance / max_distance are read: GetMinDistanceInvariance() = 0.8f * min_distance, GetMaxDistanceInvariance() = 1.2f *
 * max_distance); d_kf1_point / d_kf2_point [n_pairs][cap]: GetMapPointMatches() of the two key frames as indices into the point
 * table, -1 for NULL or isBad(); d_matched12 [n_pairs][cap]: -1 where vpMatches12[i1] is NULL, else GetIndexInKeyFrame(pKF2) of that
 * point -- -2 when the point is not in KF2; a value outside [0, N2) marks vbAlreadyMatched1 only (:1289-1299).
 * Results stay in library-owned device memory (sd_batch_download_sim3_matches): match12[i1] = idx2 for the pairs the function ADDS
 * to vpMatches12 (-1 elsewhere: vpMatches12[i1] = vpMapPoints2[idx2] is the caller's to perform), vnMatch1 / vnMatch2 as they stand
 * before the agreement loop (:1464-1480), n_found = the return value.  A point index outside [-1, n_points) cannot be seen by the
 * host: the kernel treats it as -1 and the download of EVERY pair of that call returns SD_ERR_INVALID (the next call starts clean). */
int sd_batch_search_by_sim3(sd_batch* b, int n_pairs, const int32_t* kf1_index, const int32_t* kf2_index, const float* Tcw1_host,
                            const float* Tcw2_host, const float* s12, const float* R12, const float* t12, const sd_camera* cam, float th,
                            const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points, const int32_t* d_kf1_point,
                            const int32_t* d_kf2_point, const int32_t* d_matched12, void* stream);
/* match12 / vnMatch1 / vnMatch2: `cap` >= kp_capacity entries each (nullable); entries beyond N1 / N2 are -1. */
int sd_batch_download_sim3_matches(sd_batch* b, int pair, int32_t* match12, int32_t* vnMatch1, int32_t* vnMatch2, int cap, int* n_found);
/* PoseOptimization of mCurrentFrame after ORBmatcher::SearchByProjection(mCurrentFrame, mLastFrame, ...) for projection pairs
 * pair_index[k] (host, k < n_pairs) of the last sd_batch_search_by_projection: the edges are built on the device from the pair's
 * Current slot (mvKeysUn, mvuRight, octave -> the extractor's mvInvLevelSigma2), its match array (mvpMapPoints) and the Last
 * slot's map-point table (xw[match[i]]), with the camera the pair was matched with.  Tcw_host (nullable, [n_pairs][16]): the prior;
 * NULL = the Tcw the pair was matched with.  Results stay per pair: sd_batch_download_pose. */
int sd_batch_pose_optimize(sd_batch* b, int n_pairs, const int32_t* pair_index, const float* Tcw_host, void* stream);
/* Tcw[16] = the optimised mTcw (the prior when fewer than 3 edges), outlier [cap] = mvbOutlier per CURRENT keypoint (0 where no
 * edge), n_initial = nInitialCorrespondences, n_good = the return value. */
int sd_batch_download_pose(sd_batch* b, int pair, float* Tcw, uint8_t* outlier, int cap, int* n_initial, int* n_good);
/* ---- vocabulary + bag of words (Thirdparty/DBoW2, src/Frame.cc:803-810, src/ORBmatcher.cc:159-288) ----
 * sd_vocab = ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>): one packed buffer in HBM
 * (header | desc[n][32] | weight[n] f64 | parent[n] | childStart[n+1] | childIdx[n-1] | wordId[n]; node ids and the
 * order of children are the text file's).  The buffer is what a multi-GPU job broadcasts once at start-up:
 * rank 0 loads, every rank allocates sd_vocab_packed_bytes(n_nodes), RCCL-broadcasts into it and adopts it with
 * sd_vocab_from_packed_device (the buffer stays owned by the caller). */
typedef struct sd_vocab sd_vocab;
/* TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1338-1424; System.cc:70-78 loads ORBvoc.txt with it).
 * Errors: unreadable file or a header outside k<=20, 1<=L<=10, scoring<=5, weighting<=3 -> SD_ERR_INVALID with the
 * reference's message. */
int sd_vocab_load_text(sd_vocab** out, const char* path);
/* The same from parsed node lines (line i = node i+1): parent id, isLeaf, 32 descriptor bytes, weight. */
int sd_vocab_from_nodes(sd_vocab** out, int k, int L, int scoring, int weighting, int n_lines, const int32_t* parent,
                        const uint8_t* is_leaf, const uint8_t* desc, const double* weight);
int sd_vocab_from_packed_device(sd_vocab** out, void* d_blob, size_t bytes);
void sd_vocab_destroy(sd_vocab* v);
int sd_vocab_info(const sd_vocab* v, int* k, int* L, int* scoring, int* weighting, int* n_nodes, int* n_words);
int sd_vocab_packed_device(sd_vocab* v, void** d_blob, size_t* bytes);
size_t sd_vocab_packed_bytes(int n_nodes);
int sd_vocab_download_nodes(const sd_vocab* v, int32_t* parent, int32_t* n_children, int32_t* word_id, uint8_t* desc, double* weight);

/* Frame::ComputeBoW (src/Frame.cc:803-810): mpORBvocabulary->transform(descriptors, mBowVec, mFeatVec, levelsup = 4)
 * for the listed image slots.  Per slot: the BowVector (distinct word ids ascending + f64 values, normalised as the
 * vocabulary's scoring asks), the FeatureVector flattened in map order (node id at level L - levelsup, feature index),
 * and per feature the word / weight / node of TemplatedVocabulary::transform(feature, ...).
 * meta[image][4] = {listed features, distinct nodes, distinct words, 0}. */
int sd_batch_compute_bow(sd_batch* b, const sd_vocab* v, int n_images, const int32_t* image_index, int levelsup, void* stream);
int sd_batch_bow_device(sd_batch* b, uint32_t** d_bow_word, double** d_bow_value, uint32_t** d_fv_node, uint32_t** d_fv_feature,
                        int32_t** d_meta, int* cap);
int sd_batch_download_bow(sd_batch* b, int image, uint32_t* bow_word, double* bow_value, int* n_words, uint32_t* fv_node,
                          uint32_t* fv_feature, int* n_features, uint32_t* feature_word, double* feature_weight,
                          uint32_t* feature_node, int cap);
/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (src/ORBmatcher.cc:159-288;
 * callers Tracking::TrackReferenceKeyFrame and Relocalization): pair p matches keyframe slot kf_index[p] against frame
 * slot frame_index[p] (sd_batch_compute_bow must have run on both).  d_kf_valid (nullable, [n_pairs][cap] u8):
 * pKF->GetMapPointMatches()[i] != NULL && !isBad().  Results through sd_batch_download_matches: match[iF] = index of the
 * keyframe feature whose map point lands in vpMapPointMatches[iF] (or -1), nmatches = the return value; no pairs. */
int sd_batch_search_by_bow(sd_batch* b, int n_pairs, const int32_t* kf_index, const int32_t* frame_index,
                           const uint8_t* d_kf_valid, float nnratio, int checkOrientation, void* stream);

/* ---- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:208-453) ----
 * ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (src/ORBmatcher.cc:814-980, with
 * CheckDistEpipolarLine :140-157) for n_pairs independent pairs of batch slots: KF1 = slot kf1_index[p], KF2 = slot kf2_index[p]
 * (sd_batch_compute_bow must have run on both: SD_ERR_STATE otherwise).  Tcw1_host / Tcw2_host: n_pairs row-major 4x4 poses; F12
 * (LocalMapping::ComputeF12, :537-554) and the epipole are formed from them and `cam` on the host.  d_has_mp1 / d_has_mp2
 * (nullable, [n_pairs][cap] u8): pKF->GetMapPoint(i) != NULL.  check_orientation = the matcher's mbCheckOrientation
 * (CreateNewMapPoints builds ORBmatcher(0.6, false)).  As in the reference two features of KF1 may take the same feature of KF2
 * (vbMatched2 is never set).  Results through sd_batch_download_matches: match[idx1] = idx2 or -1, pairs = vMatchedPairs
 * ((idx1, idx2), ascending idx1), nmatches = the return value. */
int sd_batch_search_for_triangulation(sd_batch* b, int n_pairs, const int32_t* kf1_index, const int32_t* kf2_index,
                                      const float* Tcw1_host, const float* Tcw2_host, const sd_camera* cam,
                                      const uint8_t* d_has_mp1, const uint8_t* d_has_mp2, int only_stereo, int check_orientation,
                                      void* stream);
/* A point CreateNewMapPoints creates: `neighbour` = position in the keyframe's neighbour list, idx1 / idx2 = the observations
 * (pMP->AddObservation(mpCurrentKeyFrame, idx1), AddObservation(pKF2, idx2)), xw = the MapPoint's world position. */
typedef struct sd_new_map_point {
    int32_t neighbour, idx1, idx2;
    float xw[3];
} sd_new_map_point;       /* 24 bytes */
/* The loop body of CreateNewMapPoints for n_kf keyframes in one launch sequence.  Keyframe k = slot kf_index[k] with pose
 * kf_Tcw_host[k] and d_kf_has_mp (nullable, [n_kf][cap] u8: GetMapPoint(i) != NULL when the function starts); it owns neighbours
 * [neigh_offset[k], neigh_offset[k+1]) in GetBestCovisibilityKeyFrames order: slot neigh_index[j], pose neigh_Tcw_host[j],
 * d_neigh_has_mp (nullable, [neighbours][cap] u8).  neigh_median_depth NULL = the stereo / RGB-D rule `baseline < mb -> skip`;
 * otherwise the monocular rule `baseline / neigh_median_depth[j] < 0.01 -> skip` (pKF2->ComputeSceneMedianDepth(2), the caller's).
 * A feature triangulated with one neighbour is skipped by the later ones (AddMapPoint, :440).  Keyframes of one call do not see each
 * other's new points.  The early return on CheckNewKeyFrames() is the caller's: it passes the neighbours it wants.
 * The poses are used as given (any 4x4): a match whose triangulation has x3D[3] == 0 is skipped, as in the reference.  A stereo point
 * (uRight >= 0) whose depth is <= 0 is skipped where the reference would unproject it.
 * Output (library-owned device memory, valid until the next call): d_new [n_kf][cap] records in creation order (neighbour ascending,
 * then idx1 ascending), d_nnew [n_kf] = nnew. */
int sd_batch_create_new_map_points(sd_batch* b, int n_kf, const int32_t* kf_index, const float* kf_Tcw_host,
                                   const uint8_t* d_kf_has_mp, const int32_t* neigh_offset, const int32_t* neigh_index,
                                   const float* neigh_Tcw_host, const float* neigh_median_depth, const uint8_t* d_neigh_has_mp,
                                   const sd_camera* cam, sd_new_map_point** d_new, int32_t** d_nnew, void* stream);
int sd_batch_download_new_map_points(sd_batch* b, int kf, sd_new_map_point* out, int cap, int* nnew);

/* ---- LocalMapping::SearchInNeighbors (src/LocalMapping.cc:455-535) ----
 * The per-candidate search of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:982-1106) for n_jobs calls at once; the tail
 * (:1108-1128: Replace / AddObservation / AddMapPoint) stays with the caller that owns the map, who walks the sd_fuse_hit records.
 * Job j = Fuse(slot kf_index[j], entries [cand_offset[j], cand_offset[j+1]) of d_cand_point, th) with pose Tcw_host[j] (row-major 4x4);
 * sd_batch_assign_grid must have run on the slot since it was last extracted (SD_ERR_STATE otherwise).  An entry is an index into
 * d_points / d_point_desc (n_points records; sd_map_point as for sd_batch_search_local_map, `flags` ignored) or -1 where the reference
 * `continue`s at :1003-1007 (NULL, isBad(), IsInKeyFrame(pKF)).  Many jobs may name the same point; the entries of ONE job must be
 * distinct points (not checked).  d_kf_state (nullable = every feature empty, [n_jobs][cap] u8): 0 = GetMapPoint(idx) == NULL, 1 = the
 * feature holds a point that is not bad, 2 = it holds a bad point.  n_jobs is not bounded by max_images (at most 65535 per call).
 * Every job sees the map as given: a Replace the caller's tail performs for job j is not seen by job j+1 of the same call.
 * Outputs (library-owned device memory, valid until the next call): d_best[e] = (bestIdx, bestDist) per entry, (-1, 256) when the point
 * was rejected or no feature passed; d_hits at cand_offset[j] = the entries of job j with bestDist <= TH_LOW in entry order: cand =
 * position in the job's list, idx = bestIdx, dist = bestDist, action = what the tail meets at idx: SD_FUSE_MEET_KF (state 1),
 * SD_FUSE_MEET_BAD (state 2: counted, nothing done), SD_FUSE_ADD (state 0, the job's first hit on idx) or SD_FUSE_MEET_CANDIDATE (state
 * 0, a later hit; other = `cand` of the entry that got SD_FUSE_ADD, -1 for every other action); d_nfused[j] = the return value.
 * Errors: SD_ERR_INVALID for negative or descending offsets, cand_offset[0] != 0, th <= 0, a slot out of range, NULL tables with
 * n_jobs > 0.  The entries live in device memory, so one outside [-1, n_points) is found by the kernel: it is searched as -1, nothing
 * is read out of range, and the next sd_batch_download_fuse returns SD_ERR_INVALID. */
typedef struct sd_fuse_hit { int32_t cand, idx, dist, action, other; } sd_fuse_hit;   /* 20 bytes */
enum { SD_FUSE_ADD = 1, SD_FUSE_MEET_KF = 2, SD_FUSE_MEET_BAD = 3, SD_FUSE_MEET_CANDIDATE = 4 };
int sd_batch_fuse(sd_batch* b, int n_jobs, const int32_t* kf_index, const float* Tcw_host, const int32_t* cand_offset,
                  const int32_t* d_cand_point, const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points,
                  const uint8_t* d_kf_state, const sd_camera* cam, float th, int32_t** d_best, sd_fuse_hit** d_hits,
                  int32_t** d_nfused, void* stream);
/* best [n][2] (nullable), hits (nullable) with room for cap_entries records, n_entries = the job's entry count, nfused = its return
 * value.  SD_ERR_CAPACITY when the job has more than cap_entries entries. */
int sd_batch_download_fuse(sd_batch* b, int job, int32_t* best, sd_fuse_hit* hits, int cap_entries, int* n_entries, int* nfused);

/* ---- LoopClosing::ComputeSim3 (src/LoopClosing.cc:240-400) and SearchAndFuse (:586-620): the matchers ----
 * Both Scw functions decompose the similarity on the host per job, as DESIGN.md Q41 freezes it: scw = (float)sqrt(f64 sum of the squares
 * of row 0), inv = (float)(1.0 / (double)scw), Rcw = sRcw * inv and tcw = t * inv element-wise in f32; Ow follows as for any pose.
 *
 * ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1134-1257).  Job tables, entries, d_kf_state, outputs and
 * the sd_batch_download_fuse records are those of sd_batch_fuse (Scw_host: n_jobs row-major 4x4 similarities); an entry is -1 for isBad()
 * or a member of pKF->GetMapPoints().  The search has no chi-square and no uRight test, and bestDist starts at INT_MAX: a lone member at
 * distance 256 is reported as (idx, 256) and is not a hit.  Action codes: SD_FUSE_MEET_KF = vpReplacePoint[cand] = the feature's point;
 * SD_FUSE_MEET_BAD = counted only; SD_FUSE_ADD = AddObservation + AddMapPoint; SD_FUSE_MEET_CANDIDATE = the feature now holds the
 * earlier candidate `other`, which is what vpReplacePoint[cand] becomes. */
int sd_batch_fuse_sim3(sd_batch* b, int n_jobs, const int32_t* kf_index, const float* Scw_host, const int32_t* cand_offset,
                       const int32_t* d_cand_point, const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points,
                       const uint8_t* d_kf_state, const sd_camera* cam, float th, int32_t** d_best, sd_fuse_hit** d_hits,
                       int32_t** d_nfused, void* stream);
/* ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (src/ORBmatcher.cc:679-812) for n_pairs (at most max_images) independent pairs of
 * slots; sd_batch_compute_bow must have run on both (SD_ERR_STATE otherwise).  d_valid1 / d_valid2 (nullable, [n_pairs][cap] u8): the
 * feature's map point is non-NULL and not bad.  Results through sd_batch_download_matches: match[idx1] = idx2 or -1 (the assignment
 * vpMatches12[idx1] = vpMapPoints2[idx2] stays the caller's), nmatches = the return value, no pairs.  Unlike the keyframe-frame
 * function the acceptance is bestDist1 < TH_LOW. */
int sd_batch_search_by_bow_kf(sd_batch* b, int n_pairs, const int32_t* kf1_index, const int32_t* kf2_index, const uint8_t* d_valid1,
                              const uint8_t* d_valid2, float nnratio, int check_orientation, void* stream);
/* ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:290-403) for n_jobs calls at once.  Job j = slot
 * kf_index[j] (sd_batch_assign_grid must have run on it), Scw_host[j], entries [cand_offset[j], cand_offset[j+1]) of d_cand_point (indices
 * into d_points / d_point_desc as for sd_batch_fuse, -1 where isBad()) and row j of d_matched ([n_jobs][cap] i32, the incoming vpMatched:
 * -1 NULL, a point index, or -2 for a point outside the table).  A candidate that occurs in its job's row is in spAlreadyFound and is
 * skipped; a feature whose row value is not -1 is never a target.  The function is a sequential greedy (a feature taken by an earlier
 * candidate is invisible to the later ones) and the result is what the sequential loop gives.
 * Outputs (library-owned device memory, valid until the next call): d_assigned [n_jobs][cap] = position in the job's list of the
 * candidate that took the feature, -1 elsewhere (features matched on entry stay -1); d_best[e] = (bestIdx, bestDist) as found at the
 * entry's turn, (-1, 256) when it was rejected or nothing passed; d_nmatches[j] = the return value.
 * Per candidate the 64 smallest (distance, visiting order) keys of its window are kept.  A candidate that finds all 64 taken while its
 * window held more is not answered: the next sd_batch_sync (and with it every download) returns SD_ERR_UNSUPPORTED with flag 128.
 * An entry outside [-1, n_points) or a d_matched value outside [-2, n_points) on any feature of a job's slot (a job with at least one
 * entry scans its whole row) is read as -1 and turns the downloads of the call into SD_ERR_INVALID.  Other errors as for sd_batch_fuse
 * (th <= 0 is SD_ERR_INVALID).  No host synchronisation inside the call, except when a call has more jobs or entries than any before it:
 * the library-owned tables then grow, and the stream is synchronised once before the old ones are freed (as in sd_batch_fuse). */
int sd_batch_search_by_projection_sim3(sd_batch* b, int n_jobs, const int32_t* kf_index, const float* Scw_host, const int32_t* cand_offset,
                                       const int32_t* d_cand_point, const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points,
                                       const int32_t* d_matched, const sd_camera* cam, int th, int32_t** d_assigned, int32_t** d_best,
                                       int32_t** d_nmatches, void* stream);
/* assigned (nullable) with room for cap >= kp_capacity entries, best [n][2] (nullable) with room for cap_entries pairs; SD_ERR_CAPACITY
 * when a buffer that was given is too small.  n_entries = the job's entry count, nmatches = its return value. */
int sd_batch_download_projection_sim3(sd_batch* b, int job, int32_t* assigned, int cap, int32_t* best, int cap_entries, int* n_entries,
                                      int* nmatches);
/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
 * (src/ORBmatcher.cc:1629-1756), the matcher of Tracking::Relocalization (src/Tracking.cc:2323, :2343), for n_jobs calls at once, with
 * mbCheckOrientation set as Relocalization sets it.  Job j = frame slot frame_index[j], keyframe slot kf_index[j] (sd_batch_assign_grid
 * must have run on both, SD_ERR_STATE otherwise; jobs may share slots), CurrentFrame.mTcw = Tcw_host[j] (row-major 4x4), th[j] and
 * orb_dist[j].  Per-job device rows, each [n_jobs][cap] with cap = kp_capacity:
 *   d_kf_point     pKF->GetMapPointMatches() as indices into d_points / d_point_desc (sd_map_point records and 32-byte descriptors as for
 *                  sd_batch_fuse), -1 for NULL; isBad() is flag bit 0 cleared;
 *   d_frame_point  CurrentFrame.mvpMapPoints on entry as point indices, -1 for NULL (each job has its own, also on a shared frame slot);
 *   d_found        (nullable, u8) per KEYFRAME feature: its point is in sAlreadyFound.  The set is expressed over point ids by the caller:
 *                  every keyframe feature that carries an id of the set is flagged.  Two features carrying one id are two visits of the
 *                  loop, as in the reference; each follows its own flag.
 * Reproduced as the reference states them: no `z > 0` test (a point behind the camera that projects inside the image is searched),
 * invzc = 1.0 / z in double rounded to float, u < mnMinX || u > mnMaxX (both ends inside, likewise v), both distance bounds inside,
 * Frame::GetFeaturesInArea(u, v, th * mvScaleFactors[level], level - 1, level + 1), the sequential greedy (a frame feature that holds a
 * point, from the entry row or from an earlier keyframe feature of this call, is no target), dist < bestDist, bestDist <= ORBdist, and
 * the rotation histogram whose losers become NULL after the loop.
 * Outputs (library-owned device memory, valid until the next call), rows [n_jobs][cap]: d_frame_point_out = mvpMapPoints after the call,
 * d_from_kf = the keyframe feature that supplied a new entry, -1 elsewhere; d_nmatches[j] = the return value.  Per keyframe feature the
 * exit it took (SD_RELOC_*) and (bestIdx2, bestDist) at its turn come with sd_batch_download_reloc_matches.
 * Caps: n_jobs <= SD_RELOC_MAX_JOBS, features per slot = the batch's kp_capacity (<= 65535); 0 < th, 0 <= ORBdist <= 255 (a larger one
 * would index with bestIdx2 == -1 in the reference): SD_ERR_INVALID before anything is launched.
 * Per keyframe feature the 64 smallest (distance, visiting order) keys of its window are kept.  A feature that finds all 64 taken while
 * its window held more is not answered: the next sd_batch_sync (and with it every download) returns SD_ERR_UNSUPPORTED with flag 128.
 * A d_kf_point / d_frame_point value outside [-1, n_points) is read as -1 and turns the downloads of the call into SD_ERR_INVALID.
 * No host synchronisation inside the call, except when a call has more jobs than any before it: the library-owned tables then grow,
 * and the stream is synchronised once before the old ones are freed (as in sd_batch_fuse). */
#define SD_RELOC_MAX_JOBS 4096
#define SD_RELOC_NULL 1          /* the keyframe feature has no point (or lies beyond the keyframe's count) */
#define SD_RELOC_BAD 2           /* isBad() */
#define SD_RELOC_FOUND 3         /* in sAlreadyFound */
#define SD_RELOC_OUT_U 4         /* u < mnMinX || u > mnMaxX */
#define SD_RELOC_OUT_V 5
#define SD_RELOC_DIST_MIN 6      /* dist3D < 0.8f * min_distance */
#define SD_RELOC_DIST_MAX 7      /* dist3D > 1.2f * max_distance */
#define SD_RELOC_WINDOW_EMPTY 8  /* vIndices2.empty() */
#define SD_RELOC_NO_FREE 9       /* every member held a point (or lay at distance 256): bestIdx2 == -1 */
#define SD_RELOC_ABOVE_DIST 10   /* bestDist > ORBdist */
#define SD_RELOC_MATCHED 11
#define SD_RELOC_CULLED 12       /* matched, then removed by the rotation histogram */
int sd_batch_search_by_projection_reloc(sd_batch* b, int n_jobs, const int32_t* frame_index, const int32_t* kf_index, const float* Tcw_host,
                                        const float* th, const int32_t* orb_dist, const int32_t* d_kf_point, const int32_t* d_frame_point,
                                        const uint8_t* d_found, const sd_map_point* d_points, const uint8_t* d_point_desc, int n_points,
                                        const sd_camera* cam, int32_t** d_frame_point_out, int32_t** d_from_kf, int32_t** d_nmatches,
                                        void* stream);
/* Job `job` of the last sd_batch_search_by_projection_reloc.  frame_point, from_kf, exits (each [cap]) and best ([cap][2]) are nullable
 * and need room for cap >= kp_capacity entries (SD_ERR_CAPACITY otherwise); nmatches = the return value. */
int sd_batch_download_reloc_matches(sd_batch* b, int job, int32_t* frame_point, int32_t* from_kf, int32_t* exits, int32_t* best, int cap,
                                    int* nmatches);
/* The cascade of Tracking::Relocalization after PnP, from `if(!Tcw.empty())` to `if(nGood>=50)` (src/Tracking.cc:2292-2358), for n_jobs
 * (frame, candidate keyframe) pairs as one launch sequence without a host synchronisation between its steps.  Job j is what the reference
 * holds at line 2292: frame slot frame_index[j], keyframe slot kf_index[j] (sd_batch_assign_grid on both), Tcw_host[j] = the pose of
 * PnPsolver::iterate, row j of d_frame_point = mvpMapPoints after lines 2300-2309 (the BoW match where vbInliers, else -1) and row j of
 * d_kf_point = vpCandidateKFs[i]->GetMapPointMatches(), both [n_jobs][cap] indices into d_points as for sd_batch_search_by_projection_reloc.
 * sFound is derived on the device, over point ids: the non-NULL entries of d_frame_point, and at line 2333 every non-NULL entry of the
 * assignment, outliers of the second optimisation included.  Steps, each predicated per job on the device:
 *   1  PoseOptimization (k_pose_optimize on edges built from the assignment in key point order: mvKeysUn, mvuRight, mvInvLevelSigma2 of
 *      the octave, the point's position); nGood < 10 is the `continue`; else outliers become NULL
 *   2  nGood < 50: SearchByProjection(.., sFound, 10, 100)
 *   3  nadditional + nGood >= 50: PoseOptimization; NO outlier is set to NULL after this one (the reference does not)
 *   4  30 < nGood < 50: sFound rebuilt, SearchByProjection(.., sFound, 3, 64)
 *   5  nGood + nadditional >= 50: PoseOptimization, outliers become NULL
 * matched = nGood >= 50 of the last optimisation that ran.  The caller applies the reference's `break`: the first job of a frame, in
 * candidate order, with matched set is the answer; jobs are independent because lines 2300-2309 rewrite every entry of mvpMapPoints for
 * each candidate.  PnPsolver, mnLastRelocFrameId and that `break` stay on the host.
 * stage_reached = the number of the last step that ran; n_good / n_additional are -1 for a step that did not run; Tcw_stage[k] = the pose
 * after optimisation k (the pose before it where it did not run), Tcw = Tcw_stage[2].
 * Caps, refusals and the answer-or-refuse rule of the searches are those of sd_batch_search_by_projection_reloc; the call reuses that
 * function's library-owned tables, so its last results are gone.  No host synchronisation inside the call except when the tables grow. */
typedef struct sd_reloc_result {
    int32_t stage_reached, matched;
    int32_t n_good[3], n_additional[2];
    float Tcw_stage[3][16];
    float Tcw[16];
} sd_reloc_result;
int sd_batch_relocalize_refine(sd_batch* b, int n_jobs, const int32_t* frame_index, const int32_t* kf_index, const float* Tcw_host,
                               const int32_t* d_kf_point, const int32_t* d_frame_point, const sd_map_point* d_points, const uint8_t* d_point_desc,
                               int n_points, const sd_camera* cam, sd_reloc_result** d_results, void* stream);
/* Job `job` of the last sd_batch_relocalize_refine: the result record, and per frame key point the final mvpMapPoints (point index or -1)
 * and mvbOutlier (written only where a key point had an edge, as the reference does: a key point whose outlier was set to NULL keeps its
 * flag).  Each pointer is nullable; the rows need cap >= kp_capacity entries. */
int sd_batch_download_reloc(sd_batch* b, int job, sd_reloc_result* result, int32_t* frame_point, uint8_t* outlier, int cap);
/* ---- Tracking::Relocalization, lines 2256-2358, for any number of (frame slot, keyframe slot) jobs as ONE launch sequence with no host round
 * trip (DESIGN Q46): the PnPsolver constructor's gather, iterate(n_iterations), lines 2300-2309 and the cascade of sd_batch_relocalize_refine.
 * d_bow_match [n_jobs][cap] i32 (device): row j = vvpMapPointMatches of the job per FRAME key point, a point index or -1 (what
 * sd_batch_search_by_bow leaves).  The gather keeps, in key-point order, every match whose point has its good flag set (bit 0 of
 * sd_map_point.flags, the flag the reloc matcher reads; PnPsolver.cc:83-85): xw from d_points, uv = mvKeysUn[i].pt and sigma2 =
 * mvLevelSigma2[octave] from the frame slot, tag = i.  problems [n_jobs] (host): fx fy cx cy, seed, start_iteration, n_iterations per job;
 * probability .. th2 as for sd_pnp_ransac_device.  N is a device value here, so SetRansacParameters is evaluated on the host for EVERY N in
 * [0, cap] (as written, :121-157) into a table the device reads, and the stage is launched against the caps.  The PnP record of a job is what
 * sd_pnp_ransac_device gives for the gathered problem.  Then mvpMapPoints[i] = the match where vbInliers[i], else -1 (:2300-2309), and the
 * cascade runs from the DEVICE pose; a job of kind 0 has an all -1 row, so no step of the cascade does anything for it (nGood = 0).  Its
 * results are those sd_batch_relocalize_refine gives when fed that pose and row.  kp_capacity above SD_PNP_MAX_CORRESPONDENCES:
 * SD_ERR_UNSUPPORTED; otherwise the refusals of the two calls it joins.  Still with the caller: the `nmatches < 15` discard (:2260-2264; a job
 * with fewer matches is simply not submitted), vbDiscarded (from no_more), the `break` over candidates and mnLastRelocFrameId. */
int sd_batch_relocalize_pnp(sd_batch* b, int n_jobs, const int32_t* frame_index, const int32_t* kf_index, const sd_pnp_problem* problems,
                            double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2,
                            const int32_t* d_bow_match, const int32_t* d_kf_point, const sd_map_point* d_points, const uint8_t* d_point_desc,
                            int n_points, const sd_camera* cam, sd_reloc_result** d_results, void* stream);
/* Job `job` of the last sd_batch_relocalize_pnp (every pointer nullable): the PnP record; the gathered problem (n_corr rows of corr, their
 * inlier bytes); the row handed to the cascade; and what sd_batch_download_reloc reports.  corr / inliers / row / frame_point / outlier hold
 * kp_capacity entries (cap >= that). */
int sd_batch_download_reloc_pnp(sd_batch* b, int job, sd_pnp_result* pnp, int32_t* n_corr, sd_pnp_corr* corr, uint8_t* inliers, int32_t* row,
                                sd_reloc_result* result, int32_t* frame_point, uint8_t* outlier, int cap);
/* What optimisation `stage` (0 .. 2) of the job saw and decided: its edges in order, mvbOutlier per edge, the pose it started from.
 * n_edges = 0 for a stage that did not run. */
int sd_batch_download_reloc_optimisation(sd_batch* b, int job, int stage, sd_pose_edge* edges, uint8_t* edge_outlier, int cap_edges,
                                         int* n_edges, float* Tcw_in);
/* Search `which` (0: th 10 / ORBdist 100, 1: th 3 / ORBdist 64) of the job: mvpMapPoints before and after it and the rows of
 * sd_batch_download_reloc_matches.  A search that did not run passes mvpMapPoints through, with exits 0 and nmatches 0.  Its pose is
 * Tcw_stage[which] of the result, its sFound the non-NULL entries of d_frame_point (0) or of frame_point_in (1). */
int sd_batch_download_reloc_search(sd_batch* b, int job, int which, int32_t* frame_point_in, int32_t* frame_point_out, int32_t* from_kf,
                                   int32_t* exits, int32_t* best, int cap, int* nmatches);
/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) for n_points points in one launch (the "Update points" loop of
 * SearchInNeighbors, Replace, CreateNewMapPoints).  Point p owns observations [d_obs_offset[p], d_obs_offset[p+1]) of d_obs_desc (32 B
 * each, 16-byte aligned) in the order the reference fills vDescriptors: the caller's std::map order, bad keyframes left out.
 * d_best_obs[p] = BestIdx relative to the point's first observation (the first row whose median distance, sorted[(int)(0.5*(N-1))] of
 * the full matrix row with its zero diagonal, is strictly smallest) or -1 when it has none; d_desc_out (nullable, [n_points][32])
 * receives the chosen descriptor and is untouched for -1.  Every pointer is device memory; asynchronous on `stream`. */
int sd_distinctive_descriptors_device(int n_points, const int32_t* d_obs_offset, const uint8_t* d_obs_desc, int32_t* d_best_obs,
                                      uint8_t* d_desc_out, void* stream);

/* The model fit of Tracking::TrackHomo (src/Tracking.cc:1026-1075) for every pair of the preceding
 * sd_batch_search_by_projection, from its points_last / points_current: replaces cv::findHomography(points_last,
 * points_current, RANSAC, 3, inliers_H), cv::findFundamentalMat(..., RANSAC, 3, 0.99, inliers_F), the inlier counts
 * and the choice `n_H > n_F ? (H, return 1) : (F, return 2)` when either count exceeds 10 (else 0).  The estimator is
 * this library's own specification (OpenCV's cannot be matched bit for bit without OpenCV); HorF / flag
 * are what sd_batch_separate takes.  Masks are indexed like the pair list of sd_batch_download_matches. */
int sd_batch_estimate_motion(sd_batch* b, void* stream);
int sd_batch_download_motion(sd_batch* b, int pair, double* H, double* F, uint8_t* mask_h, uint8_t* mask_f, int cap,
                             int* n_points, int* n_h, int* n_f, float* HorF, int* flag);

/* Frame::UndistortKeyPoints (src/Frame.cc:812-842) and Frame::ComputeImageBounds (:844-872) for cameras whose
 * Camera.k1 is not zero (TUM1 / TUM2 / EuRoC settings): cv::undistortPoints(pts, mK, mDistCoef, Mat(), mK).  K4 = fx, fy,
 * cx, cy; dist5 = k1, k2, p1, p2, k3 (Tracking.cc:76-90).  sd_batch_undistort_keypoints writes the mvKeysUn records of the
 * first n_images slots to d_keys_un ([n_images][cap] sd_keypoint; a plain copy when k1 == 0, as the reference does).
 * sd_image_bounds gives mnMinX, mnMaxX, mnMinY, mnMaxY for sd_camera. */
int sd_undistort_points_device(const float* d_pts, int n, const float* K4, const float* dist5, float* d_out, void* stream);
/* mvKeysUn as a second key-point array of the batch (cameras with Camera.k1 != 0: TUM1 / TUM2 / EuRoC settings).  After
 * sd_batch_set_distortion every consumer that reads mvKeysUn in the reference does so here: the grid (PosInGrid / GetFeaturesInArea),
 * both SearchByProjection overloads, ComputeStereoFromRGBD's `kpU.pt.x - mbf/d` (Frame.cc:1069), UnprojectStereo, the point pairs of
 * TrackHomo and classifyH / classifyF (mvdynKeysUn); box membership, the depth lookup and the stereo matcher keep reading mvKeys.
 * sd_batch_undistort (re)computes the arrays of the listed slots -- call it after an extraction, after sd_batch_first_separate
 * (it permutes mvKeys) and after sd_batch_update_frame (it appends); sd_tracker_* does.  dist5[0] == 0 switches it off again. */
int sd_batch_set_distortion(sd_batch* b, const float* K4, const float* dist5);
int sd_batch_undistort(sd_batch* b, int n_slots, const int32_t* slots, void* stream);
int sd_batch_download_keys_un(sd_batch* b, int image, sd_keypoint* kp, int cap, int* n);
int sd_batch_download_dynamic_keys_un(sd_batch* b, int slot, sd_keypoint* kp, int cap, int* n); /* mvdynKeysUn, indexed like sd_batch_download_dynamic */
int sd_batch_undistort_keypoints(sd_batch* b, int n_images, const float* K4, const float* dist5, sd_keypoint* d_keys_un, void* stream);
int sd_image_bounds(int cols, int rows, const float* K4, const float* dist5, float* bounds4);

/* Frame copy constructor (src/Frame.cc:39-63), as in `mLastFrame = Frame(mCurrentFrame)`: copies the frame
 * results of slot src (keypoints, descriptors, mvuRight/mvDepth, grid cells, map-point table) to slot dst. */
int sd_batch_copy_frame(sd_batch* b, int src, int dst, void* stream);
int sd_batch_matches_device(sd_batch* b, int32_t** d_match, int32_t** d_pairs, int32_t** d_npairs, int32_t** d_nmatches,
                            int* cap);
int sd_batch_download_matches(sd_batch* b, int pair, int32_t* match, int32_t* pairs, int cap, int* npairs, int* nmatches);

/* ---- dynamic-object handling (src/Frame.cc:481-641, src/Tracking.cc:1093-1367) ---- */
/* Capacity of every per-frame box table of this ABI (the reference's vector<cv::Rect2d> is unbounded, include/Frame.h:55-68): a frame
 * may bring up to SD_MAX_BOXES detector boxes, and objects (the boxes after Frame::boxTrack's re-injection of unmatched last-frame boxes)
 * must fit the same table -- SD_ERR_CAPACITY says so explicitly when it does not; nothing is ever truncated. */
#define SD_MAX_BOXES 64
/* Frame::boxTrack(boxes, last_frame) (src/Frame.cc:481-552), host code (f64, a handful of boxes).  boxes: [cap][4]
 * (x, y, width, height) in/out — unmatched last-frame boxes are re-injected once, so *n_out may exceed n_box.
 * Outputs box_idx / omit / velocity ([cap], [cap], [cap][2]) are the frame's members of the same names. */
int sd_box_track(double* boxes, int n_box, int cap, const double* last_objects, int n_last, const int32_t* last_box_idx,
                 const uint8_t* last_omit, const double* last_velocity, int img_cols, int img_rows, int32_t* box_idx,
                 uint8_t* omit, double* velocity, int* n_out);
/* Frame::firstSeparate + the ctor split (src/Frame.cc:555-604, 336-367) for n_frames frame slots: keypoints
 * inside any box become dynamic (class_id = pre-split index), arrays are reordered static-first, N becomes
 * N_s, empty boxes are erased exactly as the reference does it (quirk included), per-box keypoint lists
 * (mvdynKeys/mdynDescriptors/mvudynRight/mvdynDepth) are index lists into the frame's arrays.
 * boxes: [n_frames][SD_MAX_BOXES][4], box_idx: [n_frames][SD_MAX_BOXES] (boxTrack outputs).  Run after the
 * stereo / RGB-D step (the lookup is per keypoint, so the order relative to the reorder is immaterial).
 * BOUND (this library's, the reference has none -- Frame.cc:555-604 works on std::vectors): the dynamic-object kernels keep a frame's key-point masks
 * in LDS (20 bytes per key-point slot): on a workspace whose extractor yields more than about 6,800 key points per image this call and
 * sd_batch_separate return SD_ERR_UNSUPPORTED (extraction and matching are not affected).  Rounds 1-3 stopped at 2,048; since round 4 the tables are sized by the workspace and a box's descriptors pass
 * through LDS in chunks of 2,048 (tests/test_gpu_cull.py: 5,000 features, one box holding 4,600 of them).  Nothing is ever truncated silently. */
int sd_batch_first_separate(sd_batch* b, int n_frames, const int32_t* slots, const double* boxes, const int32_t* n_boxes,
                            const int32_t* box_idx, void* stream);
/* Frame::objects / box_idx / box_status and the per-box lists of a slot.  kept_orig[j] = index (before the
 * erase) of surviving box j — apply the same selection to omit / box_velocity on the host.  box_start has nb+1
 * entries; box_items index the frame's DYNAMIC keypoint arrays (sd_batch_download_dynamic): the keypoints that
 * fell inside boxes, in original order — mvdynKeys[b][k] == dynamic[box_items[box_start[b] + k]]. */
int sd_batch_download_boxes(sd_batch* b, int slot, int* nb, double* boxes, int32_t* box_idx, int32_t* box_status,
                            int32_t* kept_orig, int32_t* box_start, int32_t* box_items, int items_cap, int* n_all,
                            int* n_static);
/* The per-slot record behind sd_batch_download_boxes as it lies in HBM ([max_images] of them): what a multi-GPU job gathers
 * beside the keypoint arrays (objects, box_idx, box_status, N_s = n_static, N_d = n_dynamic). */
typedef struct sd_frame_boxes {
    int32_t nb, n_all, n_static, n_dynamic;
    double boxes[SD_MAX_BOXES][4];
    int32_t box_idx[SD_MAX_BOXES], box_status[SD_MAX_BOXES], kept_orig[SD_MAX_BOXES];
    int32_t box_start[SD_MAX_BOXES + 1];
    int32_t pad_;
} sd_frame_boxes;
int sd_batch_boxes_device(sd_batch* b, sd_frame_boxes** d_frame_boxes);
/* The dynamic keypoints of a slot (class_id = index before the split), their descriptors, mvuRight and mvDepth. */
int sd_batch_download_dynamic(sd_batch* b, int slot, sd_keypoint* kp, uint8_t* desc, float* uright, float* depth, int cap, int* n);
/* Tracking::Separate(HorF, flag, dynStatus) (src/Tracking.cc:1093-1239) for n_pairs (current, reference) slots:
 * per box with the same id in both frames cv::BFMatcher(NORM_HAMMING, crossCheck).match, the <3 / <20 % skip,
 * classifyH (flag 1, :1241-1309) or classifyF (flag 2, :1311-1367) with H/F row-major 3x3 f32, the static /
 * dynamic box decision and box_status update against mLastFrame's (last_box_idx / last_box_status, [n_pairs][SD_MAX_BOXES]).
 * HorF == flag == NULL: pair p takes both from pair p of the preceding sd_batch_estimate_motion without leaving the
 * device; a pair whose TrackHomo flag is 0 is skipped as Tracking::Track_new does (ret 0, nothing classified). */
int sd_batch_separate(sd_batch* b, int n_pairs, const int32_t* cur_index, const int32_t* ref_index, const float* HorF,
                      const int32_t* flag, const int32_t* last_box_idx, const int32_t* last_box_status,
                      const int32_t* n_last, void* stream);
/* ret = Separate's return value; dyn_start[SD_MAX_BOXES + 1] / dyn_status = dynStatus as CSR over the current frame's boxes
 * (entries: index into the box list or -1); matches = (queryIdx, trainIdx) per entry. */
int sd_batch_download_separate(sd_batch* b, int pair, int32_t* ret, int32_t* dyn_start, int32_t* dyn_status, int32_t* matches,
                               int cap);
/* Frame::UpdateFrame(dynStatus) (src/Frame.cc:607-641) on the current frames of the last sd_batch_separate:
 * re-admitted keypoints are appended behind the static ones (class_id de-duplicated, push_back order), N grows.
 * only_if_static != 0 applies it only where Separate returned 1 (Tracking.cc:651-653).  Re-run
 * sd_batch_assign_grid afterwards (UpdateFeaturesToGrid). */
int sd_batch_update_frame(sd_batch* b, int only_if_static, void* stream);

/* Reference-frame queue of the dynamic block of Tracking::Track_new (src/Tracking.cc:620-666, 952-959; q_frame,
 * Tracking.h:109): host logic.  candidate(): oldest queued frame more than 0.2 s older than the current one
 * that has boxes (box-less fronts are dropped), or -1; reject(): TrackHomo failed on it, pop unless last;
 * push(): after a tracked frame, keep at most 0.3*fps frames (max_frames = Camera.fps). */
typedef struct sd_refqueue sd_refqueue;
int sd_refqueue_create(sd_refqueue** out);
int sd_refqueue_destroy(sd_refqueue* q);
int sd_refqueue_clear(sd_refqueue* q);
int sd_refqueue_size(const sd_refqueue* q, int* n);
int sd_refqueue_candidate(sd_refqueue* q, double cur_timestamp, int cur_has_boxes, int* slot);
int sd_refqueue_reject(sd_refqueue* q, int* again);
int sd_refqueue_push(sd_refqueue* q, double timestamp, int slot, int has_boxes, int max_frames, int* evicted_slot);

/* ---- Frame-level boundary: Tracking::GrabImage* -> Frame::Frame -> the dynamic block of Tracking::Track_new ----
 * sd_tracker is the per-frame front end of ORB_SLAM2::Tracking for n_lanes independent camera streams ("lanes": one
 * System each in the reference) that advance together, one frame per lane per call.  One call =
 *   System::TrackStereo / TrackRGBD / TrackMonocular (include/System.h:66-79, src/System.cc:119-375)
 *   -> Tracking::GrabImageStereo / GrabImageRGBD / GrabImageMonocular (src/Tracking.cc:170-343): cvtColor, depth scaling
 *   -> Frame::Frame, all five constructors (src/Frame.cc:66-126, 129-237, 240-294, 297-403, 406-461): extract (both eyes),
 *      boxTrack, firstSeparate + split, stereo / RGB-D association, grid
 *   -> Track_new's dynamic block (src/Tracking.cc:620-666): reference frame from q_frame, TrackHomo (:968-1086, th / 2*th
 *      retry, H / F fit), Separate (:1093-1239), UpdateFrame (Frame.cc:607-641)
 *   -> [track_last] TrackWithMotionModel's SearchByProjection(mCurrentFrame, mLastFrame, th) (src/Tracking.cc:1714-1741)
 *   -> q_frame.push / mLastFrame = Frame(mCurrentFrame) (src/Tracking.cc:952-959).
 * What is NOT behind this boundary is the SLAM state: the pose prediction mVelocity * mLastFrame.mTcw is an input (Tcw,
 * identity when NULL), a frame's map points are its own stereo points (Frame::UnprojectStereo), and `mState == OK &&
 * !mVelocity.empty()` is taken to hold from a lane's third frame on.  Stereo + boxes follows DESIGN.md Q9.
 * Results stay in the tracker's sd_batch (sd_tracker_batch): lane s's mCurrentFrame is slot cur_slot (valid until the next
 * call), TrackHomo's pair index is s, the last-frame matcher's pair index is n_lanes + s (sd_batch_download_matches /
 * _motion / _separate); every sd_batch_download_* call works on these slots. */
#define SD_SENSOR_MONOCULAR 0 /* System::eSensor, include/System.h:60-64 */
#define SD_SENSOR_STEREO 1
#define SD_SENSOR_RGBD 2
typedef struct sd_tracker sd_tracker;
typedef struct sd_tracker_params {
    int32_t sensor;         /* SD_SENSOR_* */
    int32_t width, height;
    int32_t channels;       /* input images: 1 = 8-bit gray, 3 = 8-bit BGR / RGB, 4 = BGRA / RGBA (cvtColor fused into the level-0 copy;
                             * Tracking.cc:175-200) */
    int32_t rgb_order;      /* Camera.RGB (Tracking.cc:107-112) */
    int32_t n_lanes;        /* independent camera streams */
    int32_t track_last;     /* != 0: also match against mLastFrame */
    int32_t depth_type;     /* RGB-D: element type of the depth image, SD_DEPTH_U16 (CV_16U) or SD_DEPTH_F32 (CV_32F: passed through when
                             * DepthMapFactor is 1, scaled in f32 otherwise -- Tracking.cc:271-272) */
    sd_camera cam;          /* Camera.fx .. Camera.bf and the image bounds */
    float dist[5];          /* Camera.k1, k2, p1, p2, k3 (k1 == 0: mvKeysUn == mvKeys, as Frame.cc:814-818) */
    float fps;              /* Camera.fps = mMaxFrames (Tracking.cc:93-98) */
    float depth_map_factor; /* DepthMapFactor (Tracking.cc:141-146); RGB-D only */
    float th_depth;         /* ThDepth (kept for the caller; not used on this path) */
    int32_t ini_features;   /* monocular: nFeatures of mpIniORBextractor (Tracking.cc:127-128: 2 * nFeatures), used while a lane is not
                             * initialised (Tracking.cc:335-338); 0 = one extractor for every frame */
    int32_t lookahead;      /* > 0: frames per lane sd_tracker_prefetch may extract ahead in one call (two such blocks can be outstanding) */
} sd_tracker_params;
#define SD_DEPTH_U16 0
#define SD_DEPTH_F32 1
typedef struct sd_lane_result {
    int32_t frame_id;       /* mnId within the lane (0, 1, ...) */
    int32_t cur_slot;       /* sd_batch slot of mCurrentFrame */
    int32_t last_slot;      /* slot of the copy kept as mLastFrame and as q_frame's newest entry */
    int32_t ref_slot, ref_frame_id; /* the reference frame TrackHomo ran against last (-1: the dynamic block did not run) */
    int32_t track_flag;     /* TrackHomo's return value: 0 failed / not run, 1 H, 2 F */
    int32_t separate_ret;   /* Separate's return value (0 when it did not run) */
    int32_t n_track_matches, n_track_pairs, n_h, n_f; /* nmatches, points_last.size(), n_H, n_F of TrackHomo */
    int32_t n_last_matches; /* SearchByProjection(mCurrentFrame, mLastFrame) or -1 */
    int32_t N, N_s, N_d;    /* keypoints after UpdateFrame; static / dynamic after the ctor's split */
    int32_t n_boxes;        /* objects.size() after the empty-box erase */
    int32_t box_idx[SD_MAX_BOXES], box_status[SD_MAX_BOXES];
    uint8_t omit[SD_MAX_BOXES];
    uint8_t pad_[4];
    double objects[SD_MAX_BOXES][4], box_velocity[SD_MAX_BOXES][2];
} sd_lane_result;
int sd_tracker_create(sd_tracker** out, sd_extractor* ex, const sd_tracker_params* params);
int sd_tracker_destroy(sd_tracker* t);
int sd_tracker_reset(sd_tracker* t);              /* Tracking::Reset (src/Tracking.cc:2369-2409): every lane starts over */
int sd_tracker_batch(sd_tracker* t, sd_batch** b); /* the workspace that holds the frames (owned by the tracker) */
/* One frame of every lane.  d_images: image k (0 = left / the only one, 1 = right) of lane s starts at
 * d_images + (s * images_per_lane + k) * image_pitch, rows `stride` bytes apart, `channels` bytes per pixel.
 * d_depth (RGB-D): depth image (CV_16U, or CV_32F when params.depth_type says so) of lane s at d_depth + s * depth_pitch_elems elements.  boxes [n_lanes][SD_MAX_BOXES][4]
 * (x, y, w, h) / n_boxes [n_lanes]: the detector's boxes of this frame; n_boxes[s] < 0 (or boxes == NULL) selects the
 * constructor without boxes for that lane.  timestamps [n_lanes].  Tcw / Twc (nullable, [n_lanes][16] row-major): pose
 * of the frame and its inverse.  results [n_lanes] (nullable).  The call returns after the results are on the host. */
int sd_tracker_track(sd_tracker* t, const uint8_t* d_images, size_t stride, size_t image_pitch, const void* d_depth,
                     size_t depth_stride_elems, size_t depth_pitch_elems, const double* boxes, const int32_t* n_boxes,
                     const double* timestamps, const float* Tcw, const float* Twc, sd_lane_result* results, void* stream);
/* The same from host images (a per-frame caller such as System::TrackStereo): images[s * images_per_lane + k] points to image k
 * of lane s in host memory (rows `stride` bytes apart), depth[s] to lane s's CV_16U depth image (RGB-D).  Uploads, then
 * sd_tracker_track. */
int sd_tracker_track_host(sd_tracker* t, const uint8_t* const* images, size_t stride, const void* const* depth,
                          size_t depth_stride_elems, const double* boxes, const int32_t* n_boxes, const double* timestamps,
                          const float* Tcw, const float* Twc, sd_lane_result* results);
/* Time-batched mode (BASELINE configs[4]: whole sequences, few lanes per GPU).  A frame's work splits into a history-free part --
 * GrabImage*'s cvtColor, ORB extraction of both eyes, UndistortKeyPoints, ComputeStereoMatches / ComputeStereoFromRGBD: more than 95 % of
 * the front end's time -- and the recurrence along the stream (boxTrack -> firstSeparate -> TrackHomo vs the queued frame -> Separate ->
 * UpdateFrame -> match vs mLastFrame), whose box ids (`max + 1`, Frame.cc:545-550) depend on the stream's whole history, so a stream
 * cannot be cut into independently processed chunks.  sd_tracker_prefetch runs the history-free part for the NEXT n_frames frames of every
 * lane in one batch (image e of frame k of lane s at d_images + ((k * n_lanes + s) * images_per_lane + e) * image_pitch, depth image of
 * frame k of lane s at d_depth + (k * n_lanes + s) * depth_pitch_elems), asynchronously on `stream`; the following n_frames calls of
 * sd_tracker_track with d_images == NULL consume them in order and run only the recurrence.  Results are identical to n_frames plain
 * calls.  Needs params.lookahead >= n_frames; two blocks may be outstanding (extract block b + 1 while block b is tracked). */
int sd_tracker_prefetch(sd_tracker* t, const uint8_t* d_images, size_t stride, size_t image_pitch, const void* d_depth,
                        size_t depth_stride_elems, size_t depth_pitch_elems, int n_frames, void* stream);
/* Frames -- not streams -- sharded over GPUs (BASELINE configs[4] on N > 1 ranks: "independent frames shard across the 8 GPUs").  Everything
 * a frame computes before Frame::boxTrack (src/Frame.cc:129-161: GrabImage*'s cvtColor, ORB extraction of both eyes, UndistortKeyPoints,
 * ComputeStereoMatches / ComputeStereoFromRGBD) depends on the frame's images alone; the recurrence (Frame.cc:162 onward, Tracking.cc:620-666,
 * 952-959) stays with the GPU that owns the stream.  So ANY GPU may run sd_tracker_prefetch on any frames (a "worker" tracker whose lanes are
 * simply batch entries), export the results as fixed-stride records, move them (RCCL all-to-all, the caller's business) and the owner imports
 * them as a prefetched block that sd_tracker_track(d_images == NULL) consumes exactly like a block it had extracted itself.
 *   record = N, per-level counts, mvKeys, mDescriptors, mvuRight, mvDepth, stereo SADs [, mvKeysUn when Camera.k1 != 0], each padded to 16 bytes:
 *            sd_tracker_prefetched_record_bytes(t) bytes (0 for a tracker without lookahead), the same for every tracker built with the same
 *            extractor parameters, image size and distortion setting -- the pyramid is not part of it (nothing after the association reads it).
 *   export : frames [first_frame, first_frame + n_frames) of the NEWEST outstanding prefetched block -> d_records[(k * n_lanes + s)] in
 *            frame-major order, on `stream` (waits for the block's extraction).  The caller orders a later prefetch into the same block behind it
 *            (same stream or an event).
 *   import : n_frames * n_lanes records in frame-major order become the next outstanding block (params.lookahead >= n_frames; two blocks may be
 *            outstanding); d_records may be reused once `stream` has passed this call.
 *   discard: a worker drops its newest block after exporting it (it will never track it).
 *   record_stride >= the record size, a multiple of 16 (d_records 16-byte aligned): the caller may keep its own bytes behind a record -- the
 *            detector's boxes of the frame travel there in bench.py. */
size_t sd_tracker_prefetched_record_bytes(const sd_tracker* t);
int sd_tracker_export_prefetched(sd_tracker* t, int first_frame, int n_frames, void* d_records, size_t record_stride, void* stream);
int sd_tracker_import_prefetched(sd_tracker* t, const void* d_records, size_t record_stride, int n_frames, void* stream);
int sd_tracker_discard_prefetched(sd_tracker* t);
/* The SLAM state a caller with a live back end owns, handed over the boundary (all optional; without them the tracker runs in its
 * sharded batch mode):
 *  - the pose prior is the Tcw / Twc argument of sd_tracker_track: `mCurrentFrame.SetPose(mVelocity*mLastFrame.mTcw)` (Tracking.cc:982)
 *    and the mRwc / mOw of Frame::UpdatePoseMatrices (Frame.cc:663-675);
 *  - sd_tracker_set_mappoints: the MapPoints of the frame just tracked, as the back end left them (mCurrentFrame.mvpMapPoints after
 *    TrackWithMotionModel / TrackLocalMap): xw [n_lanes][cap][3] = mvpMapPoints[i]->GetWorldPos(), flags [n_lanes][cap] (bit0: the point
 *    exists and is not an outlier, bit1: Observations() > 0), n [n_lanes] = entries given for the lane (its N), < 0 = leave the lane's
 *    own stereo points.  Call it after sd_tracker_track: it replaces the map-point table of the lane's mLastFrame, which is also the
 *    newest q_frame entry (they are copies of the same frame, Tracking.cc:952-959), i.e. what TrackHomo's and TrackWithMotionModel's
 *    SearchByProjection project in later frames (Tracking.cc:998-1010, ORBmatcher.cc:1485-1627).  The tracker never rewrites it;
 *  - sd_tracker_set_state: [n_lanes] bit0 = the lane is initialised (mState != NOT_INITIALIZED / NO_IMAGES_YET: the monocular lane uses
 *    mpORBextractorLeft instead of mpIniORBextractor, Tracking.cc:335-338), bit1 = `mState==OK && !mVelocity.empty()` (TrackHomo may
 *    run, Tracking.cc:971).  NULL returns to the automatic rule (frame 0, 1 of a lane: neither; later: both). */
int sd_tracker_set_mappoints(sd_tracker* t, const float* xw, const uint8_t* flags, const int32_t* n);
int sd_tracker_set_state(sd_tracker* t, const int32_t* state);
/* Opt-in TrackWithMotionModel tail (src/Tracking.cc:1728-1789), with track_last: after the last-frame matcher the search is repeated
 * with 2*th for the lanes below 20 matches, a lane still below 20 stops there (ran = 0), the others run PoseOptimization with the Tcw
 * argument of sd_tracker_track as the prior, count nmatchesMap (non-outlier matches whose mLastFrame point has flag bit1, i.e.
 * Observations() > 0: 0 in the sharded batch mode, where a frame's own stereo points have no observations) and set
 * ok = nmatchesMap >= 10.  All of it is enqueued before the step's one synchronisation.  enable = 0 (the default): nothing changes.
 * The matches stay at pair n_lanes + s; the pose problem of lane s is pair n_lanes + s of sd_batch_download_pose. */
typedef struct sd_pose_result {
    float Tcw[16];          /* the optimised mCurrentFrame.mTcw (the prior when ran == 0) */
    int32_t ran;            /* PoseOptimization ran (nmatches >= 20 after the 2*th retry) */
    int32_t n_matches;      /* nmatches after the retry (the same as sd_lane_result.n_last_matches) */
    int32_t n_initial, n_good;      /* nInitialCorrespondences, PoseOptimization's return value */
    int32_t n_matches_map;  /* nmatchesMap */
    int32_t ok;             /* TrackWithMotionModel's return value: nmatchesMap >= 10 */
} sd_pose_result;
int sd_tracker_set_pose_optimization(sd_tracker* t, int enable);
int sd_tracker_pose_results(sd_tracker* t, sd_pose_result* results);   /* [n_lanes], of the last sd_tracker_track */
/* Batch copy of frame slots (Frame's copy constructor, src/Frame.cc:39-63) in one launch: slot src[i] -> dst[i]. */
int sd_batch_copy_frames(sd_batch* b, int n, const int32_t* src, const int32_t* dst, void* stream);

/* ---- dense RGB-D back-projection with the dynamic mask ----
 * PointCloudMapping::generatePointCloud(kf, color, depth, mask, dyn_obj) (src/pointcloudmapping.cc:59-103) for n_frames frame
 * slots: every third row / column; a pixel is skipped when it lies inside a dynamic box AND mask != 0, or when its depth is
 * outside [0.01, 5]; dyn_obj = the slot's objects whose box_status is 0 or 2 (Tracking::CreateNewKeyFrame, src/Tracking.cc:
 * 1999-2007).  d_color: 8-bit 3-channel image as handed to TrackRGBD (bytes 0, 1, 2 of a pixel become b, g, r); d_depth: CV_16U
 * with depth_factor = 1 / DepthMapFactor (the imDepth of Tracking.cc:271-272); d_mask: the 8-bit mask image (0 = background;
 * the reference converts it to CV_32F and tests != 0), may be NULL (nothing is masked).  Twc_host: [n_frames][16] row-major f64,
 * the T.inverse().matrix() of the key frame pose.  Output: d_points [n_frames][cap_points] in the reference's push_back order
 * (pcl::PointXYZRGBA payload), d_counts [n_frames][2] = {cloud size, masked_num}.  cap_points >= ceil(W/3) * ceil(H/3). */
typedef struct sd_cloud_point { float x, y, z; uint8_t b, g, r, a; } sd_cloud_point;
int sd_batch_backproject_dense(sd_batch* b, int n_frames, const int32_t* slots, const uint8_t* d_color, size_t color_stride,
                               size_t color_pitch, const uint16_t* d_depth, size_t depth_stride_elems, size_t depth_pitch_elems,
                               float depth_factor, const uint8_t* d_mask, size_t mask_stride, size_t mask_pitch, const sd_camera* cam,
                               const double* Twc_host, sd_cloud_point* d_points, int cap_points, int32_t* d_counts, void* stream);

/* ---- detector: yolov3Segment (include/yolo.h:22-48, src/yolo.cc, src/yolo/yolov3.cfg) ----
 * cv::dnn's Darknet importer + Net::forward + the reference's post-processing, on MFMA (f16 operands, f32
 * accumulation).  The network is given as a layer list (the five layer types of yolov3.cfg); weights are the
 * payload of a Darknet .weights file (floats after the header; per convolutional layer: biases, [scales, rolling
 * mean, rolling variance], weights [filters][c][size][size]), i.e. what readNetFromDarknet (yolo.cc:27) consumes. */
#define SD_YOLO_CONV 0
#define SD_YOLO_SHORTCUT 1
#define SD_YOLO_ROUTE 2
#define SD_YOLO_UPSAMPLE 3
#define SD_YOLO_YOLO 4
typedef struct sd_yolo_layer {
    int32_t type;
    int32_t filters, size, stride, batch_normalize, leaky; /* [convolutional]; leaky 0 = linear; pad = size/2 */
    int32_t from[2], nfrom;                                /* [shortcut] from / [route] layers (negative = relative) */
    int32_t mask[3];                                       /* [yolo] anchor indices */
} sd_yolo_layer;
typedef struct sd_yolo sd_yolo;
/* The 107 layers and 9 anchors of src/yolo/yolov3.cfg. */
int sd_yolo_v3_layers(sd_yolo_layer* layers, int cap, int* n, float anchors[18]);
/* yolov3Segment::yolov3Segment (yolo.cc:15-31); net_w x net_h = inpWidth x inpHeight (yolo.h:26-27). */
int sd_yolo_create(sd_yolo** out, const sd_yolo_layer* layers, int n_layers, const float anchors[18], int classes, int net_w,
                   int net_h, int max_batch);
/* The same with the arithmetic chosen: SD_YOLO_F16 = f16 operands, f32 accumulation on v_mfma_f32_32x32x16_f16 (default, the
 * throughput mode); SD_YOLO_F32 = f32 operands and accumulation on v_mfma_f32_32x32x2_f32, i.e. the reference's own arithmetic
 * (cv::dnn computes in f32, src/yolo.cc:29), at 1/16 of the MFMA rate.  In F32 mode sd_yolo_download_layer returns floats.
 * SD_YOLO_F32W = SD_YOLO_F32 with the 3 x 3 stride-1 layers of >= 64 input channels and >= 128 filters computed as Winograd
 * F(2 x 2, 3 x 3) in f32 (2.25 x fewer multiplies on those layers; sums of inputs and of weights are multiplied, so the last bits
 * differ from the direct f32 convolution -- held to the same layer tolerance and box-set test as SD_YOLO_F32). */
#define SD_YOLO_F16 0
#define SD_YOLO_F32 1
#define SD_YOLO_F32W 2
/* SD_YOLO_F32X3 = SD_YOLO_F32 with the >= 64-filter layers computed on three bf16 limbs per f32 operand (x = hi + mid + lo exactly;
 * a product = its six limb products of weight >= 2^-16, each exact in f32, accumulated in f32 by v_mfma_f32_32x32x16_bf16): what is
 * dropped is <= 2^-23 of a product, the size of an f32 multiply's own rounding.  Held to the same layer tolerance and box-set test. */
#define SD_YOLO_F32X3 3
int sd_yolo_create_prec(sd_yolo** out, const sd_yolo_layer* layers, int n_layers, const float anchors[18], int classes, int net_w,
                        int net_h, int max_batch, int precision);
int sd_yolo_precision(const sd_yolo* y, int* precision);
int sd_yolo_destroy(sd_yolo* y);
int sd_yolo_weight_count(const sd_yolo* y, size_t* n_floats);
int sd_yolo_load_darknet_weights(sd_yolo* y, const float* payload, size_t n_floats);
int sd_yolo_layer_shape(const sd_yolo* y, int layer, int* h, int* w, int* c);
int sd_yolo_flops(const sd_yolo* y, double* flops_per_image);
/* The MFMA FLOPs the chosen mode actually executes per image (== sd_yolo_flops except in SD_YOLO_F32W). */
int sd_yolo_mfma_flops(const sd_yolo* y, double* flops_per_image);
/* bf16 MFMA FLOPs per image executed by the limb kernels of SD_YOLO_F32X3 (0 in the other modes; sd_yolo_mfma_flops then counts
 * only the layers that stay on the f32 MFMA). */
int sd_yolo_mfma_flops_bf16(const sd_yolo* y, double* flops_per_image);
/* How many convolutions the mode computes as Winograd F(2 x 2, 3 x 3) (0 except in SD_YOLO_F32W). */
int sd_yolo_winograd_layers(const sd_yolo* y, int* n_layers);
/* blobFromImage + net.forward + the confidence filter (yolo.cc:63-68,163-183) for n 8-bit 3-channel images in HBM
 * (channel order as cv::imread delivers it, i.e. BGR; swapRB is applied as in the reference). */
int sd_yolo_forward_device(sd_yolo* y, const uint8_t* d_bgr, int width, int height, size_t stride, size_t image_pitch, int n,
                           float conf_threshold, void* stream);
/* Test access: layer output (f16, NHWC, dense) of one image; region-layer rows [total_rows][5 + classes] of image 0
 * (only after a forward with n == 1). */
int sd_yolo_download_layer(sd_yolo* y, int layer, int image, uint16_t* f16_nhwc_out); /* float* in SD_YOLO_F32 mode */
/* Test access: the same with the channels the layer STORES beyond its own -- *stored_channels = its channel count rounded up to 32 (256 for a
 * 255-channel head; the padding must stay zero), [H][W][*stored_channels]; `out` may be null to ask for the count alone. */
int sd_yolo_download_layer_stored(sd_yolo* y, int layer, int image, uint16_t* out, int* stored_channels);
int sd_yolo_download_region(sd_yolo* y, float* rows, int* total_rows);
/* Host-image forms for a per-frame caller (`yolo->Segmentation_(imLeft)`, stereo_kitti.cc:107): upload + forward of one
 * 8-bit BGR image, and yolov3Segment::Segmentation's mask in host memory (image 0 of the last forward). */
int sd_yolo_forward_host(sd_yolo* y, const uint8_t* bgr, int width, int height, size_t stride, float conf_threshold);
int sd_yolo_mask_host(sd_yolo* y, int frame_cols, int frame_rows, float conf_threshold, float nms_threshold, uint8_t* mask,
                      size_t stride, int* no_target);
/* yolov3Segment::Segmentation_ result for one image (yolo.cc:151-206): NMSBoxes(conf, nms), class filter
 * {person, car, bicycle, bus, truck}, box width -20 % / height +60 % about the centre.  boxes: [cap][4] x,y,w,h. */
/* yolov3Segment::Segmentation (yolo.cc:34-58, postprocess :80-137): d_mask (frame_rows x frame_cols u8 in HBM) = 1 except
 * inside the 31x31-ellipse dilation of the kept boxes' central halves; all ones and *no_target = 1 when none is kept. */
int sd_yolo_mask_device(sd_yolo* y, int image, int frame_cols, int frame_rows, float conf_threshold, float nms_threshold,
                        uint8_t* d_mask, size_t stride, int* no_target, void* stream);
int sd_yolo_boxes(sd_yolo* y, int image, int frame_cols, int frame_rows, float conf_threshold, float nms_threshold, double* boxes,
                  int32_t* class_ids, float* confidences, int cap, int* n);
/* The same post-processing for the first n_images of the last forward pass on the device (sort by score, greedy NMS,
 * class filter, rectCenterScale): boxes [n_images][SD_MAX_BOXES][4] f64 (x, y, w, h), class ids / confidences
 * [n_images][SD_MAX_BOXES], n_boxes[n_images].  _device writes device buffers and does not synchronise; _batch also
 * downloads (one synchronisation for the whole batch).  More than 4096 rows above the threshold or more than
 * SD_MAX_BOXES kept boxes in an image -> SD_ERR_CAPACITY (use the per-image host form). */
/* Overlap mode (f32-class modes; off by default).  A pass is blobFromImage -> 75 convolutions -> three region decodes -> (caller) NMS + download; on ONE
 * stream the small kernels at both ends (about 1.5 % of a 256-image pass) serialise with the next pass's convolutions.  With overlap on,
 * sd_yolo_forward_device(stream) issues the convolutions on `stream`, blobFromImage on an internal stream ahead of them and the decodes on another
 * behind their heads (events order them; consecutive passes are protected against each other the same way), and sd_yolo_boxes_device / _batch wait for
 * the decodes on THEIR stream argument -- give them a stream of their own and enqueue the next pass before consuming this one's boxes
 * (bench.py: two passes ahead).  `stream` of sd_yolo_forward_device is then NOT a completion point for the decoded rows; the host forms
 * (sd_yolo_boxes, sd_yolo_mask_*) synchronise the device as before.  Results are the same bits either way (tests/test_gpu_yolo.py). */
int sd_yolo_set_overlap(sd_yolo* y, int on);
int sd_yolo_boxes_device(sd_yolo* y, int n_images, int frame_cols, int frame_rows, float conf_threshold, float nms_threshold,
                         double* d_boxes, int32_t* d_class_ids, float* d_confidences, int32_t* d_n_boxes, void* stream);
int sd_yolo_boxes_batch(sd_yolo* y, int n_images, int frame_cols, int frame_rows, float conf_threshold, float nms_threshold,
                        double* boxes, int32_t* class_ids, float* confidences, int32_t* n_boxes, void* stream);

/* ---- Tracking::GrabImage* preprocessing (src/Tracking.cc:170-343) ---- */
/* cvtColor(RGB|BGR|RGBA|BGRA -> GRAY); rgb_order = Camera.RGB.  channels 3 or 4. */
int sd_cvt_gray_device(const uint8_t* d_src, int width, int height, size_t src_stride, size_t src_pitch, int channels,
                       int rgb_order, uint8_t* d_dst, size_t dst_stride, size_t dst_pitch, int n_images, void* stream);
/* imDepth.convertTo(CV_32F, factor) for CV_16U input. */
int sd_depth_to_f32_device(const uint16_t* d_src, int width, int height, size_t src_stride_elems, float factor,
                           float* d_dst, int n_images, size_t src_pitch_elems, void* stream);

/* ---- ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1804-1820) ---- */
int sd_descriptor_distance(const uint8_t a[32], const uint8_t b[32]); /* host, returns 0..256 */
/* All-pairs Hamming distances of two descriptor sets in HBM: out[i*nb + j] (u16). */
int sd_hamming_matrix_device(const uint8_t* d_a, int na, const uint8_t* d_b, int nb, uint16_t* d_out, void* stream);

/* ---- KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:33-309) ----
 * The database both candidate searches read, resident on the device: LoopClosing::DetectLoop (src/LoopClosing.cc:95-230) takes its
 * candidates from DetectLoopCandidates, Tracking::Relocalization (src/Tracking.cc:2219) from DetectRelocalizationCandidates, and the
 * matchers above take those candidates as input.  A keyframe is named by a caller-chosen kf_id in [0, max_keyframes).  The device holds
 * an entry per id (pool offset, word count, insertion sequence number, live flag, mRelocScore, up to SD_KFDB_MAX_NEIGHBOURS neighbour
 * ids), a pool of BowVectors (u32 word ids ascending, f64 values, laid out as sd_batch_bow_device lays them out) and the work tables of
 * a call, all allocated by sd_kfdb_create: no call allocates.  There is no inverted file: a query is matched against every live entry
 * (DESIGN.md Q42), and the order of the reference's lists is reproduced from the sequence numbers.
 * Capacities: max_pool_words words in the pool, max_queries queries per call of at most max_query_words (<= SD_KFDB_MAX_QUERY_WORDS)
 * words each.  Anything beyond them is SD_ERR_CAPACITY (or SD_ERR_INVALID for an id or a size that can never be valid) before anything
 * is launched, never a truncation.  The pool words of an erased entry are NOT reclaimed before sd_kfdb_clear; an entry added from a batch
 * slot reserves the batch's key-point capacity, because the length of its BowVector is known to the device only.
 * Ordering: the calls of one database take effect on the device in the order they are made, whichever streams they name (a change of
 * stream is bridged with an event); the host-side calls (add_host, erase, set_covisible, clear) are enqueued on the stream of the
 * previous call and do not wait for it.  Like sd_batch, a database is not re-entrant. */
typedef struct sd_kfdb sd_kfdb;
#define SD_KFDB_MAX_NEIGHBOURS 10
#define SD_KFDB_MAX_QUERY_WORDS 16384
int sd_kfdb_create(sd_kfdb** out, int max_keyframes, int max_pool_words, int max_queries, int max_query_words);
int sd_kfdb_destroy(sd_kfdb* db);
int sd_kfdb_clear(sd_kfdb* db);                         /* KeyFrameDatabase::clear; sequence numbers and the pool start again */
/* KeyFrameDatabase::add(pKF) for n slots of a batch on which sd_batch_compute_bow has run (SD_ERR_STATE otherwise): slot image_index[i]
 * becomes entry kf_id[i].  A device-to-device copy with no host synchronisation; stream NULL = the batch's.  Adding an id that is live
 * is SD_ERR_STATE.  Every add takes the next sequence number; an id added again after an erase is a new entry (new sequence number,
 * mRelocScore +0, no neighbours). */
int sd_kfdb_add_from_batch(sd_kfdb* db, sd_batch* b, int n, const int32_t* image_index, const int32_t* kf_id, void* stream);
/* The same from host arrays: word ids strictly ascending (SD_ERR_INVALID otherwise), values taken as given (not normalised). */
int sd_kfdb_add_host(sd_kfdb* db, int kf_id, const uint32_t* bow_word, const double* bow_value, int n_words);
/* KeyFrameDatabase::erase(pKF) for n ids; an id that is not live is skipped, as the reference finds nothing to erase. */
int sd_kfdb_erase(sd_kfdb* db, int n, const int32_t* kf_id);
/* pKF->GetBestCovisibilityKeyFrames(10) of n live entries as the caller's graph has it now: neigh [n][10] ids in the reference's order,
 * count [n] <= 10.  Call it wherever KeyFrame::UpdateBestCovisibles runs.  A neighbour that is not live when a query runs is skipped
 * by that query (the reference's graph holds no erased keyframe). */
int sd_kfdb_set_covisible(sd_kfdb* db, int n, const int32_t* kf_id, const int32_t* neigh, const int32_t* count);
/* One entry back (synchronises): words / values (cap_words entries each, nullable), n_words, sequence number, live flag, mRelocScore,
 * neigh [10] (-1 beyond n_neigh).  An id that was never added reads as all zero. */
int sd_kfdb_download_entry(sd_kfdb* db, int kf_id, uint32_t* bow_word, double* bow_value, int cap_words, int* n_words, uint32_t* seq, int* live,
                           float* reloc_score, int32_t* neigh, int* n_neigh);

/* KeyFrameDatabase::DetectLoopCandidates(pKF, minScore) (:76-197) and DetectRelocalizationCandidates(F) (:199-309) for n_queries
 * queries in one launch sequence.  Query q is the BowVector at [query_offset[q], query_offset[q+1]) of d_query_word / d_query_value
 * (query_offset is a HOST array of n_queries + 1 entries, the two d_ arrays device memory; word ids ascending).  The loop form takes per
 * query min_score[q] (host) and pKF->GetConnectedKeyFrames() as a host CSR of kf ids (excl_offset [n_queries + 1] starting at 0, excl_id;
 * excl_offset NULL = nothing excluded; an id that is not live is ignored, one outside [0, max_keyframes) is SD_ERR_INVALID).
 * What the functions compute, with the reference's types: the entries sharing a word with the query (and not excluded), in the order of
 * (smallest shared word id, sequence number), which is the order of lKFsSharingWords; minCommonWords = (int)(maxCommonWords * 0.8f); an
 * entry is scored iff its count is > minCommonWords, with si = (float)(-S / 2.0), S the f64 sum, from +0.0 and in ascending word order, of
 * (fabs(vi - wi) - fabs(vi)) - fabs(wi) over the common words (vi the query's value); the loop form keeps si >= min_score, counts a
 * neighbour iff it is in the list with a count > minCommonWords, and starts bestAccScore at min_score; the reloc form keeps every scored
 * entry, counts a neighbour iff it is in the list and starts at 0; a better neighbour replaces pBestKF on > only; minScoreToRetain = 0.75f *
 * bestAccScore, retention on > only; a repeated pBestKF is returned once, at its first position.
 * mRelocScore: the reloc form reads the member of neighbours it did not score in this query.  It is +0 when an entry is
 * added, every reloc query writes it for each entry it scores, and the queries of one call behave as if run one after the other in index
 * order.  The loop form neither reads nor writes it; apart from this member a query's answer does not depend on what shares its call.
 * Values must be finite.  Both calls enqueue on `stream` (NULL = the stream of the database's previous call) and return without a host
 * synchronisation; the results stay in the database until its next query call. */
int sd_kfdb_detect_loop(sd_kfdb* db, int n_queries, const int32_t* query_offset, const uint32_t* d_query_word, const double* d_query_value,
                        const float* min_score, const int32_t* excl_offset, const int32_t* excl_id, void* stream);
int sd_kfdb_detect_reloc(sd_kfdb* db, int n_queries, const int32_t* query_offset, const uint32_t* d_query_word, const double* d_query_value,
                         void* stream);
/* The same with query q = the BowVector of batch slot image_index[q] (sd_batch_compute_bow must have run on it: SD_ERR_STATE otherwise;
 * the batch's key-point capacity must not exceed max_query_words: SD_ERR_CAPACITY).  stream NULL = the batch's. */
int sd_kfdb_detect_loop_batch(sd_kfdb* db, sd_batch* b, int n_queries, const int32_t* image_index, const float* min_score,
                              const int32_t* excl_offset, const int32_t* excl_id, void* stream);
int sd_kfdb_detect_reloc_batch(sd_kfdb* db, sd_batch* b, int n_queries, const int32_t* image_index, void* stream);
/* The same from a host CSR: uploads, runs, synchronises. */
int sd_kfdb_detect_loop_host(sd_kfdb* db, int n_queries, const int32_t* query_offset, const uint32_t* query_word, const double* query_value,
                             const float* min_score, const int32_t* excl_offset, const int32_t* excl_id);
int sd_kfdb_detect_reloc_host(sd_kfdb* db, int n_queries, const int32_t* query_offset, const uint32_t* query_word, const double* query_value);
/* What a query leaves.  n_sharing = lKFsSharingWords.size(); nscores as the reference counts it; n_acc = lAccScoreAndMatch.size();
 * best_acc_score / min_score_to_retain are the start value and 0.75f times it when nothing was kept. */
typedef struct sd_kfdb_query_info {
    int32_t n_sharing, max_common_words, min_common_words, nscores, n_acc, n_candidates;
    float best_acc_score, min_score_to_retain;
} sd_kfdb_query_info;                             /* 32 bytes */
typedef struct sd_kfdb_member { int32_t kf_id, common_words, scored; float si; } sd_kfdb_member;    /* 16 bytes; si = +0 when not scored */
typedef struct sd_kfdb_acc { float acc_score; int32_t best_kf; } sd_kfdb_acc;                       /* 8 bytes */
/* Synchronises once and returns query `query` of the last detect call: cand = the candidate kf ids in the reference's order
 * (info->n_candidates of them), sharing = lKFsSharingWords in list order, acc = lAccScoreAndMatch in list order.  Every pointer is
 * nullable; SD_ERR_CAPACITY when a buffer that was given is too small (info is filled first, so a caller can size and repeat). */
int sd_kfdb_download_candidates(sd_kfdb* db, int query, int32_t* cand, int cap_cand, sd_kfdb_query_info* info, sd_kfdb_member* sharing,
                                int cap_sharing, sd_kfdb_acc* acc, int cap_acc);
/* (float)mpVoc->score(query, entry) for listed entries -- the scores from which LoopClosing::DetectLoop (:125-139) takes its minScore.
 * Queries as for sd_kfdb_detect_loop; query q lists kf ids [list_offset[q], list_offset[q+1]) of list_id (host arrays, list_offset[0] =
 * 0) and d_score (device, one f32 per listed id, in list order) receives the scores.  A listed id that is not live gets -1 (no L1 score
 * of finite vectors is below -0): the caller scores those few itself.  Asynchronous on `stream`. */
int sd_kfdb_score(sd_kfdb* db, int n_queries, const int32_t* query_offset, const uint32_t* d_query_word, const double* d_query_value,
                  const int32_t* list_offset, const int32_t* list_id, float* d_score, void* stream);

/* ---- the covisibility graph on the device (KeyFrame::UpdateConnections, AddConnection, UpdateBestCovisibles, EraseConnection:
 * src/KeyFrame.cc:123-208, 289-379, 553-567) ----
 * sd_covis mirrors the part of the map the covisibility bookkeeping reads.  Per keyframe: a live flag, its features (mvpMapPoints as point
 * ids, -1 = none; mvKeysUn[i].octave; mvuRight[i] >= 0; mvDepth[i]), its parent, mbFirstConnection, a protected flag (mnId == 0, given at
 * add time because kf_id is the caller's), its row mConnectedKeyFrameWeights and its ordered list mvpOrderedConnectedKeyFrames /
 * mvOrderedWeights.  Per map point: a bad flag.  The caller chooses kf_id in [0, max_keyframes) -- the ids it uses in sd_kfdb, so that the
 * two compose -- and mp_id in [0, max_points).
 * The observation relation is DERIVED from the keyframe tables and not stored: the observations of point p are exactly the (kf, i) of live
 * keyframes with mvpMapPoints[i] == p.  A state in which the two sides of that reference disagree (inside MapPoint::Replace or SetBadFlag)
 * cannot be represented: the caller uploads after its tail has finished.  An index by map point is rebuilt on the device when a table
 * changed since the last query; the order inside one point's list is unspecified and no result depends on it.
 * Where the reference orders by KeyFrame* (map<KeyFrame*, ..> iteration, the second key of sort(vPairs)), pointer order is kf_id order:
 * the ordered list is by descending (weight, kf_id), pKFmax is the lowest id among equal maxima.
 * Everything is allocated by sd_covis_create: no call allocates device memory (except sd_covis_local_map_host, for its staging).  The rows are dense, 12 bytes per pair of keyframe ids, hence
 * max_keyframes <= SD_COVIS_MAX_KEYFRAMES.  max_features bounds the features of all keyframes added since the last clear (an erased
 * keyframe's are NOT reclaimed before sd_covis_clear; a keyframe added from a batch slot takes the slot's capacity), max_jobs the
 * keyframes or frames listed in one query, max_local_points the local points of one frame.  Anything beyond a capacity is SD_ERR_CAPACITY, an id or size that can never be valid SD_ERR_INVALID,
 * before anything is launched; nothing is ever truncated.  Calls take effect in the order made; a change of stream is bridged with an
 * event; the object is not re-entrant.  Only the download_* and *_host calls (and sd_covis_add_host, which ends with its uploads done)
 * synchronises with the host. */
#define SD_COVIS_MAX_KEYFRAMES 8192
typedef struct sd_covis sd_covis;
int sd_covis_create(sd_covis** out, int max_keyframes, int max_features, int max_points, int max_jobs, int max_local_points);
int sd_covis_destroy(sd_covis* cv);
int sd_covis_clear(sd_covis* cv);
/* n slots of a batch become keyframes, device to device: octave, uRight >= 0 and depth of slot image_index[i] (what the last stereo or
 * RGB-D call left there) are copied; all matches start at -1, there are no connections, no parent, mbFirstConnection is set.
 * is_protected (nullable = none) marks mnId == 0.  A live kf_id, or one listed twice: SD_ERR_STATE.  stream NULL = the batch's. */
int sd_covis_add_from_batch(sd_covis* cv, sd_batch* b, int n, const int32_t* image_index, const int32_t* kf_id, const uint8_t* is_protected,
                            void* stream);
/* The same from host arrays of n_features entries each. */
int sd_covis_add_host(sd_covis* cv, int kf_id, int n_features, const uint8_t* octave, const float* uright, const float* depth,
                      int is_protected);
/* mvpMapPoints[idx[i]] of keyframe kf_id[i] = mp_id[i], -1 erases; applied in list order.  Stands for AddMapPoint + AddObservation,
 * EraseMapPointMatch + EraseObservation and the net effect of Replace.  A keyframe that is not live: SD_ERR_STATE.  If after the call two
 * features of one keyframe would name the same point: SD_ERR_INVALID and nothing changes.  For a keyframe added from a batch slot idx is
 * checked against the slot's capacity; an idx at or beyond the slot's key-point count is ignored on the device. */
int sd_covis_set_matches(sd_covis* cv, int n, const int32_t* kf_id, const int32_t* idx, const int32_t* mp_id);
/* The same from device arrays of n items (what a device matcher wrote), asynchronous on `stream` (NULL = the object's last), with no host
 * copy.  The caller guarantees what the host-array path checks: every item names a live keyframe, a feature of it and a point id in
 * [-1, max_points), no (keyframe, feature) is listed twice (the order of the items is unspecified), and afterwards no keyframe names a
 * point twice.  The device checks instead of trusting: an item out of range is left out, and two features of one keyframe naming one
 * point are found when the index by map point is next rebuilt; either makes the next sd_covis_download_* return SD_ERR_INVALID (an
 * out-of-range item is reported once; a doubly named point until the tables are corrected).  From the first such call until
 * sd_covis_clear the host no longer knows the match tables: sd_covis_set_matches still checks its ids, but the doubly-named-point refusal
 * is the device's too, and the index covers all of [0, max_points). */
int sd_covis_set_matches_device(sd_covis* cv, int n, const int32_t* d_kf_id, const int32_t* d_idx, const int32_t* d_mp_id, void* stream);
int sd_covis_set_point_bad(sd_covis* cv, int n, const int32_t* mp_id, const uint8_t* bad);         /* MapPoint::isBad() */
/* mpParent (-1 = none): what the caller's spanning-tree repair (KeyFrame::SetBadFlag, :479-537, ChangeParent) decided. */
int sd_covis_set_parent(sd_covis* cv, int n, const int32_t* kf_id, const int32_t* parent_id);
/* The graph part of KeyFrame::SetBadFlag, in list order: EraseConnection(this) on every keyframe of its row (each such keyframe's ordered
 * list is rebuilt from its whole row, as UpdateBestCovisibles does), its matches, row and list cleared, no longer live.  A protected or
 * not-live id is skipped. */
int sd_covis_erase_keyframe(sd_covis* cv, int n, const int32_t* kf_id);
/* KeyFrame::UpdateConnections for n <= max_jobs live keyframes (SD_ERR_STATE otherwise); they behave as if run in list order.  KFcounter:
 * over the keyframe's non-null, non-bad points every observer but itself.  Empty counter: nothing changes.  Keyframes with count >= 15
 * are kept, or if none the single maximum (picked on > in ascending id).  Each kept keyframe X gets AddConnection(this, w): no effect when
 * X holds this keyframe with that weight, else X's entry is written and X's list rebuilt from X's whole row.  This keyframe's row becomes
 * KFcounter (every non-zero count), its list the kept pairs; on a first connection of an unprotected keyframe parent = front of the list.
 * Asynchronous on `stream` (NULL = the object's last). */
int sd_covis_update_connections(sd_covis* cv, int n, const int32_t* kf_id, void* stream);
typedef struct sd_covis_keyframe_info {
    int32_t live, n_features, is_protected, parent, first_connection;
    int32_t n_ordered, n_row;
    int32_t n_best;          /* GetBestCovisibilityKeyFrames(best_n) is the first n_best of the ordered list */
    int32_t n_by_weight;     /* GetCovisiblesByWeight(min_weight) is the first n_by_weight: the prefix up to upper_bound(weights, w, a > b), and, as in
                                the reference, EMPTY when every weight is >= w */
} sd_covis_keyframe_info;   /* 36 bytes */
/* Synchronises.  ordered_id / ordered_weight: GetVectorCovisibleKeyFrames() and mvOrderedWeights; row_id / row_weight:
 * mConnectedKeyFrameWeights in ascending id (GetConnectedKeyFrames, GetWeight).  Arrays nullable; info is filled first, SD_ERR_CAPACITY
 * when a given buffer is too small. */
int sd_covis_download_connections(sd_covis* cv, int kf_id, int best_n, int min_weight, int32_t* ordered_id, int32_t* ordered_weight,
                                  int cap_ordered, sd_covis_keyframe_info* info, int32_t* row_id, int32_t* row_weight, int cap_row);
/* LocalMapping::KeyFrameCulling (src/LocalMapping.cc:633-697) over cand_kf_id = GetVectorCovisibleKeyFrames() of the current keyframe (n <=
 * max_jobs live keyframes, none twice), in list order.  A protected candidate is skipped.  A feature is skipped when its point is null or
 * bad, or, unless `monocular`, when depth > th_depth || depth < 0 (f32; a NaN depth counts).  Every other feature increments nMPs; with
 * Observations() (2 per stereo observer, 1 otherwise) > 3 and at least 3 other observers of octave <= this octave + 1 it is redundant.
 * flag = (double)nRedundant > 0.9 * (double)nMPs.  The loop is sequential, as the reference's: a flagged candidate whose not_erase (nullable
 * = all 0) is 0 counts as removed for every later candidate -- its observations count nowhere, and a point that lost an observer this
 * way and is left with a weighted count <= 2 is bad (MapPoint::EraseObservation -> SetBadFlag).  A flagged candidate with not_erase 1
 * changes nothing (mbToBeErased).  The call changes no state: the caller commits what it deletes with sd_covis_erase_keyframe and
 * sd_covis_set_point_bad.  Asynchronous on `stream`. */
int sd_covis_keyframe_culling(sd_covis* cv, int n, const int32_t* cand_kf_id, const uint8_t* not_erase, int monocular, float th_depth,
                              void* stream);
typedef struct sd_covis_cull_result { int32_t flag, n_mps, n_redundant; } sd_covis_cull_result;      /* 12 bytes */
/* The last culling call's record per candidate (synchronises); out nullable to ask for *n alone. */
int sd_covis_download_culling(sd_covis* cv, sd_covis_cull_result* out, int cap, int* n);
/* Tracking::UpdateLocalKeyFrames then UpdateLocalPoints (src/Tracking.cc:2076-2210) for n_queries <= max_jobs frames.  Query q is the
 * frame's mvpMapPoints as point ids (-1 = null): entries [point_offset[q], point_offset[q+1]) of the device array d_mp_id (point_offset is a
 * host array).  Votes come from the non-bad points; the list starts with the voted keyframes in ascending id, reference_kf = pKFmax
 * (picked on >).  Then the reference's loop over those members, literally: stop when the list holds more than 80; per member append the
 * first not yet included live one of its ten best covisibles, then the first such child (ascending id), then the parent if not included
 * -- and the parent's break ends the WHOLE loop, as in the source (:2192-2200).  Local points: first occurrence over (local keyframes in
 * list order, feature index), null and bad points excluded.  d_entry_bad (nullable, device, one byte per entry of d_mp_id) receives 1
 * where the frame named a bad point (the reference nulls those).  An empty vote counter gives reference_kf -1 and empty lists: the
 * reference returns early and keeps what it had.  Asynchronous on `stream`. */
int sd_covis_local_map(sd_covis* cv, int n_queries, const int32_t* point_offset, const int32_t* d_mp_id, uint8_t* d_entry_bad, void* stream);
/* The same from host arrays: uploads, runs, synchronises, downloads entry_bad (nullable).  The one call that allocates device memory: a
 * staging buffer for the ids and flags, freed before it returns. */
int sd_covis_local_map_host(sd_covis* cv, int n_queries, const int32_t* point_offset, const int32_t* mp_id, uint8_t* entry_bad);
typedef struct sd_covis_local_info {
    int32_t n_keyframes, n_voted, reference_kf, n_points;
    int32_t overflow;        /* more local points than max_local_points: n_points is the true count, the download is SD_ERR_CAPACITY */
    int32_t n_bad_entries;
} sd_covis_local_info;      /* 24 bytes */
/* One query of the last local-map call (synchronises): info first, then the lists (nullable).  SD_ERR_CAPACITY when the query overflowed
 * max_local_points -- never a short list -- or a given buffer is too small. */
int sd_covis_download_local_map(sd_covis* cv, int query, sd_covis_local_info* info, int32_t* local_kf, int cap_kf, int32_t* local_point,
                                int cap_points);
/* sd_kfdb_set_covisible for n keyframes live in both objects (SD_ERR_STATE otherwise), device to device: the first ten of each ordered
 * list.  The graph must hold no keyframe id at or beyond the database's max_keyframes (SD_ERR_INVALID: a neighbour could not be named).
 * Last writer wins between this call and sd_kfdb_set_covisible.  Ordered after the earlier calls of both objects on `stream` (NULL = the
 * graph's last). */
int sd_kfdb_set_covisible_from_covis(sd_kfdb* db, sd_covis* cv, int n, const int32_t* kf_id, void* stream);

/* ---- profiling support for bench.py ----
 * When enabled, every kernel of the batch pipeline is bracketed by hipEvents on the stream it is
 * launched on; sd_batch_kernel_times returns the accumulated milliseconds and launch counts. */
int sd_batch_set_profiling(sd_batch* b, int enabled);
int sd_batch_kernel_count(const sd_batch* b, int* n);
int sd_batch_kernel_times(sd_batch* b, int index, const char** name, double* total_ms, int64_t* launches);
int sd_batch_reset_kernel_times(sd_batch* b);
int sd_batch_sync(sd_batch* b);

#ifdef __cplusplus
}
#endif
#endif /* SD_FRONTEND_H */
