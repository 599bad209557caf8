"""ctypes binding of libsd_frontend.so (the C ABI in include/sd_frontend.h).

This is plumbing for tests and bench.py: the product is the shared library.  Class and
method names follow the reference's C++ API (ORB_SLAM2::ORBextractor, Frame, ORBmatcher) so
that the parity tests read like calls into the reference.  There is NO CPU fallback: if the
library is missing, or no HIP device is present, calls raise.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SD_FRONTEND_LIB") or os.path.join(_HERE, "lib", "libsd_frontend.so")     # the override is for kernel experiments only

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])

SD_OK = 0
SD_ERR_INVALID, SD_ERR_NO_DEVICE, SD_ERR_HIP, SD_ERR_CAPACITY, SD_ERR_UNSUPPORTED, SD_ERR_STATE = -1, -2, -3, -4, -5, -6
# sd_batch_search_by_projection_reloc: the jobs one call takes, and the exit of a keyframe feature (download_reloc_matches)
SD_RELOC_MAX_JOBS = 4096
(SD_RELOC_NULL, SD_RELOC_BAD, SD_RELOC_FOUND, SD_RELOC_OUT_U, SD_RELOC_OUT_V, SD_RELOC_DIST_MIN, SD_RELOC_DIST_MAX, SD_RELOC_WINDOW_EMPTY,
 SD_RELOC_NO_FREE, SD_RELOC_ABOVE_DIST, SD_RELOC_MATCHED, SD_RELOC_CULLED) = range(1, 13)
RELOC_RESULT_DTYPE = np.dtype([("stage_reached", "<i4"), ("matched", "<i4"), ("n_good", "<i4", (3,)), ("n_additional", "<i4", (2,)),
                               ("Tcw_stage", "<f4", (3, 4, 4)), ("Tcw", "<f4", (4, 4))])      # sd_reloc_result


class SdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("sd_frontend error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Load the HIP extension; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`"
                              % LIB_PATH)
        try:
            # torch bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's): import it first so the
            # process holds ONE HIP runtime shared by torch (device memory, RCCL) and this library.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.sd_status_string.restype = C.c_char_p
        L.sd_last_error.restype = C.c_char_p
        vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
        L.sd_extractor_create.argtypes = [C.POINTER(vp), i, f, i, i, i]
        L.sd_extractor_destroy.argtypes = [vp]
        L.sd_extractor_set_blur_taps.argtypes = [vp, vp]
        L.sd_extractor_levels.argtypes = [vp, C.POINTER(i), C.POINTER(f)]
        L.sd_extractor_tables.argtypes = [vp] * 7
        L.sd_extractor_level_size.argtypes = [vp, i, i, i, C.POINTER(i), C.POINTER(i)]
        L.sd_batch_create.argtypes = [C.POINTER(vp), vp, i, i, i]
        L.sd_batch_destroy.argtypes = [vp]
        L.sd_batch_kp_capacity.argtypes = [vp, C.POINTER(i)]
        L.sd_batch_extract_device.argtypes = [vp, vp, sz, sz, i, vp]
        L.sd_batch_extract_color_device.argtypes = [vp, vp, sz, sz, i, i, vp]
        L.sd_batch_extract_pixels_device.argtypes = [vp, vp, sz, sz, i, i, i, vp]
        L.sd_batch_rgbd_from_f32_scaled.argtypes = [vp, vp, sz, sz, i, f, f, vp]
        L.sd_tracker_set_mappoints.argtypes = [vp, vp, vp, vp]
        L.sd_tracker_set_state.argtypes = [vp, vp]
        L.sd_tracker_prefetch.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, vp]
        L.sd_tracker_prefetched_record_bytes.argtypes = [vp]
        L.sd_tracker_prefetched_record_bytes.restype = sz
        L.sd_tracker_export_prefetched.argtypes = [vp, i, i, vp, sz, vp]
        L.sd_tracker_import_prefetched.argtypes = [vp, vp, sz, i, vp]
        L.sd_tracker_discard_prefetched.argtypes = [vp]
        L.sd_batch_extract_host.argtypes = [vp, vp, sz, sz, i]
        L.sd_batch_results_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i)]
        L.sd_batch_counts.argtypes = [vp, vp, i]
        L.sd_batch_download.argtypes = [vp, i, vp, vp, i, C.POINTER(i), vp]
        L.sd_batch_pyramid_level.argtypes = [vp, i, i, C.POINTER(vp), C.POINTER(i), C.POINTER(i), C.POINTER(sz)]
        L.sd_batch_download_pyramid.argtypes = [vp, i, i, vp]
        L.sd_batch_download_blurred.argtypes = [vp, i, i, vp]
        L.sd_batch_candidate_counts.argtypes = [vp, i, vp]
        L.sd_batch_stereo_match.argtypes = [vp, i, f, f, vp]
        L.sd_batch_stereo_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i)]
        L.sd_batch_download_stereo.argtypes = [vp, i, vp, vp, vp, i]
        L.sd_batch_rgbd_from_u16.argtypes = [vp, vp, sz, sz, i, f, f, vp]
        L.sd_batch_rgbd_from_f32.argtypes = [vp, vp, sz, sz, i, f, vp]
        L.sd_batch_download_rgbd.argtypes = [vp, i, vp, vp, i]
        L.sd_batch_assign_grid.argtypes = [vp, i, vp, vp]
        L.sd_batch_download_grid.argtypes = [vp, i, vp, i]
        L.sd_batch_download_grid_index.argtypes = [vp, i, vp, i, vp, C.POINTER(i)]
        L.sd_batch_unproject.argtypes = [vp, i, i, i, vp, vp, vp]
        L.sd_batch_mappoints_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i)]
        L.sd_batch_set_mappoints.argtypes = [vp, i, vp, vp, i]
        L.sd_batch_download_mappoints.argtypes = [vp, i, vp, vp, i]
        L.sd_batch_search_by_projection.argtypes = [vp, i, vp, vp, vp, vp, vp, f, i, i, vp, vp, vp]
        L.sd_batch_copy_frame.argtypes = [vp, i, i, vp]
        L.sd_batch_matches_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i)]
        L.sd_batch_download_matches.argtypes = [vp, i, vp, vp, i, C.POINTER(i), C.POINTER(i)]
        L.sd_box_track.argtypes = [vp, i, i, vp, i, vp, vp, vp, i, i, vp, vp, vp, C.POINTER(i)]
        L.sd_batch_first_separate.argtypes = [vp, i, vp, vp, vp, vp, vp]
        L.sd_batch_download_boxes.argtypes = [vp, i, C.POINTER(i), vp, vp, vp, vp, vp, vp, i, C.POINTER(i), C.POINTER(i)]
        L.sd_batch_download_dynamic.argtypes = [vp, i, vp, vp, vp, vp, i, C.POINTER(i)]
        L.sd_batch_separate.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, vp]
        L.sd_batch_download_separate.argtypes = [vp, i, C.POINTER(i), vp, vp, vp, i]
        L.sd_batch_update_frame.argtypes = [vp, i, vp]
        L.sd_refqueue_create.argtypes = [C.POINTER(vp)]
        L.sd_refqueue_destroy.argtypes = [vp]
        L.sd_refqueue_clear.argtypes = [vp]
        L.sd_refqueue_size.argtypes = [vp, C.POINTER(i)]
        L.sd_refqueue_candidate.argtypes = [vp, C.c_double, i, C.POINTER(i)]
        L.sd_refqueue_reject.argtypes = [vp, C.POINTER(i)]
        L.sd_refqueue_push.argtypes = [vp, C.c_double, i, i, i, C.POINTER(i)]
        L.sd_cvt_gray_device.argtypes = [vp, i, i, sz, sz, i, i, vp, sz, sz, i, vp]
        L.sd_depth_to_f32_device.argtypes = [vp, i, i, sz, f, vp, i, sz, vp]
        L.sd_descriptor_distance.argtypes = [vp, vp]
        L.sd_hamming_matrix_device.argtypes = [vp, i, vp, i, vp, vp]
        L.sd_batch_set_profiling.argtypes = [vp, i]
        L.sd_batch_kernel_count.argtypes = [vp, C.POINTER(i)]
        L.sd_batch_kernel_times.argtypes = [vp, i, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.sd_batch_reset_kernel_times.argtypes = [vp]
        L.sd_batch_sync.argtypes = [vp]
        L.sd_device_count.argtypes = [C.POINTER(i)]
        L.sd_tracker_create.argtypes = [C.POINTER(vp), vp, vp]
        L.sd_tracker_destroy.argtypes = [vp]
        L.sd_tracker_reset.argtypes = [vp]
        L.sd_tracker_batch.argtypes = [vp, C.POINTER(vp)]
        L.sd_tracker_track.argtypes = [vp, vp, sz, sz, vp, sz, sz, vp, vp, vp, vp, vp, vp, vp]
        L.sd_batch_copy_frames.argtypes = [vp, i, vp, vp, vp]
        L.sd_batch_boxes_device.argtypes = [vp, C.POINTER(vp)]
        L.sd_batch_set_distortion.argtypes = [vp, vp, vp]
        L.sd_batch_undistort.argtypes = [vp, i, vp, vp]
        L.sd_batch_download_keys_un.argtypes = [vp, i, vp, i, C.POINTER(i)]
        L.sd_batch_download_dynamic_keys_un.argtypes = [vp, i, vp, i, C.POINTER(i)]
        L.sd_image_bounds.argtypes = [i, i, vp, vp, vp]
        L.sd_batch_backproject_dense.argtypes = [vp, i, vp, vp, sz, sz, vp, sz, sz, f, vp, sz, sz, vp, vp, vp, i, vp, vp]
        L.sd_pose_optimize_device.argtypes = [i, vp, vp, vp, vp, vp, vp, vp]
        L.sd_pose_optimize_host.argtypes = [i, vp, vp, vp, vp, vp, vp]
        L.sd_local_ba_device.argtypes = [i] + [vp] * 16
        L.sd_local_ba_host.argtypes = [i] + [vp] * 15
        L.sd_local_ba_set_profiling.argtypes = [i]
        L.sd_local_ba_profile.argtypes = [i, vp]
        L.sd_sim3_ransac_device.argtypes = [i, vp, vp, vp, C.c_double, i, i, vp, vp, vp, vp]
        L.sd_sim3_ransac_host.argtypes = [i, vp, vp, vp, C.c_double, i, i, vp, vp]
        L.sd_pnp_ransac_device.argtypes = [i, vp, vp, vp, C.c_double, i, i, i, C.c_float, C.c_float, vp, vp, vp, vp, i, vp]
        L.sd_pnp_ransac_host.argtypes = [i, vp, vp, vp, C.c_double, i, i, i, C.c_float, C.c_float, vp, vp, vp, vp, i]
        L.sd_sim3_optimize_device.argtypes = [i, vp, vp, vp, vp, vp, vp]
        L.sd_batch_compute_sim3_refine.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, i, vp, vp, i, vp, vp, vp]
        L.sd_batch_download_sim3_refine.argtypes = [vp, i, vp, vp, i]
        L.sd_batch_download_sim3_refine_stages.argtypes = [vp, i, vp, vp, vp, i, vp]
        L.sd_sim3_optimize_host.argtypes = [i, vp, vp, vp, vp, vp]
        L.sd_batch_pose_optimize.argtypes = [vp, i, vp, vp, vp]
        L.sd_batch_download_pose.argtypes = [vp, i, vp, vp, i, C.POINTER(i), C.POINTER(i)]
        L.sd_tracker_set_pose_optimization.argtypes = [vp, i]
        L.sd_tracker_pose_results.argtypes = [vp, vp]
        L.sd_batch_search_for_triangulation.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, i, i, vp]
        L.sd_batch_create_new_map_points.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), vp]
        L.sd_batch_download_new_map_points.argtypes = [vp, i, vp, i, C.POINTER(i)]
        L.sd_batch_fuse.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, i, vp, vp, f, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]
        L.sd_batch_download_fuse.argtypes = [vp, i, vp, vp, i, C.POINTER(i), C.POINTER(i)]
        L.sd_batch_fuse_sim3.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, i, vp, vp, f, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]
        L.sd_batch_search_by_bow_kf.argtypes = [vp, i, vp, vp, vp, vp, f, i, vp]
        L.sd_batch_search_by_projection_sim3.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, i, vp, vp, i, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]
        L.sd_batch_download_projection_sim3.argtypes = [vp, i, vp, i, vp, i, C.POINTER(i), C.POINTER(i)]
        L.sd_batch_search_by_projection_reloc.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]
        L.sd_batch_download_reloc_matches.argtypes = [vp, i, vp, vp, vp, vp, i, C.POINTER(i)]
        L.sd_batch_relocalize_refine.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, i, vp, C.POINTER(vp), vp]
        L.sd_batch_download_reloc.argtypes = [vp, i, vp, vp, vp, i]
        L.sd_batch_relocalize_pnp.argtypes = [vp, i, vp, vp, vp, C.c_double, i, i, i, C.c_float, C.c_float, vp, vp, vp, vp, i, vp, C.POINTER(vp), vp]
        L.sd_batch_download_reloc_pnp.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, vp, i]
        L.sd_batch_download_reloc_optimisation.argtypes = [vp, i, i, vp, vp, i, C.POINTER(i), vp]
        L.sd_batch_download_reloc_search.argtypes = [vp, i, i, vp, vp, vp, vp, vp, i, C.POINTER(i)]
        L.sd_batch_search_by_sim3.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, vp, f, vp, vp, i, vp, vp, vp, vp]
        L.sd_batch_download_sim3_matches.argtypes = [vp, i, vp, vp, vp, i, C.POINTER(i)]
        L.sd_distinctive_descriptors_device.argtypes = [i, vp, vp, vp, vp, vp]
        L.sd_kfdb_create.argtypes = [C.POINTER(vp), i, i, i, i]
        L.sd_kfdb_destroy.argtypes = [vp]
        L.sd_kfdb_clear.argtypes = [vp]
        L.sd_kfdb_add_from_batch.argtypes = [vp, vp, i, vp, vp, vp]
        L.sd_kfdb_add_host.argtypes = [vp, i, vp, vp, i]
        L.sd_kfdb_erase.argtypes = [vp, i, vp]
        L.sd_kfdb_set_covisible.argtypes = [vp, i, vp, vp, vp]
        L.sd_kfdb_download_entry.argtypes = [vp, i, vp, vp, i, C.POINTER(i), C.POINTER(C.c_uint32), C.POINTER(i), C.POINTER(f), vp, C.POINTER(i)]
        L.sd_kfdb_detect_loop.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp]
        L.sd_kfdb_detect_reloc.argtypes = [vp, i, vp, vp, vp, vp]
        L.sd_kfdb_detect_loop_batch.argtypes = [vp, vp, i, vp, vp, vp, vp, vp]
        L.sd_kfdb_detect_reloc_batch.argtypes = [vp, vp, i, vp, vp]
        L.sd_kfdb_detect_loop_host.argtypes = [vp, i, vp, vp, vp, vp, vp, vp]
        L.sd_kfdb_detect_reloc_host.argtypes = [vp, i, vp, vp, vp]
        L.sd_kfdb_download_candidates.argtypes = [vp, i, vp, i, vp, vp, i, vp, i]
        L.sd_kfdb_score.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp]
        L.sd_covis_create.argtypes = [C.POINTER(vp), i, i, i, i, i]
        L.sd_covis_destroy.argtypes = [vp]
        L.sd_covis_clear.argtypes = [vp]
        L.sd_covis_add_from_batch.argtypes = [vp, vp, i, vp, vp, vp, vp]
        L.sd_covis_add_host.argtypes = [vp, i, i, vp, vp, vp, i]
        L.sd_covis_set_matches.argtypes = [vp, i, vp, vp, vp]
        L.sd_covis_set_matches_device.argtypes = [vp, i, vp, vp, vp, vp]
        L.sd_covis_set_point_bad.argtypes = [vp, i, vp, vp]
        L.sd_covis_set_parent.argtypes = [vp, i, vp, vp]
        L.sd_covis_erase_keyframe.argtypes = [vp, i, vp]
        L.sd_covis_update_connections.argtypes = [vp, i, vp, vp]
        L.sd_covis_download_connections.argtypes = [vp, i, i, i, vp, vp, i, vp, vp, vp, i]
        L.sd_covis_keyframe_culling.argtypes = [vp, i, vp, vp, i, f, vp]
        L.sd_covis_download_culling.argtypes = [vp, vp, i, C.POINTER(i)]
        L.sd_covis_local_map.argtypes = [vp, i, vp, vp, vp, vp]
        L.sd_covis_local_map_host.argtypes = [vp, i, vp, vp, vp]
        L.sd_covis_download_local_map.argtypes = [vp, i, vp, vp, i, vp, i]
        L.sd_kfdb_set_covisible_from_covis.argtypes = [vp, vp, i, vp, vp]
        _lib = L
    return _lib


def check(rc):
    if rc != SD_OK:
        L = lib()
        raise SdError(rc, (L.sd_status_string(rc) or b"").decode() + ": " + (L.sd_last_error() or b"").decode())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class ORBextractor:
    """ORB_SLAM2::ORBextractor (include/ORBextractor.h:45-114): parameters and derived tables."""

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST):
        L = lib()
        self.h = C.c_void_p()
        check(L.sd_extractor_create(C.byref(self.h), nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST))
        self.nfeatures, self.nlevels = nfeatures, nlevels
        self.mvScaleFactor = np.zeros(nlevels, np.float32); self.mvInvScaleFactor = np.zeros(nlevels, np.float32)
        self.mvLevelSigma2 = np.zeros(nlevels, np.float32); self.mvInvLevelSigma2 = np.zeros(nlevels, np.float32)
        self.mnFeaturesPerLevel = np.zeros(nlevels, np.int32); self.umax = np.zeros(16, np.int32)
        check(L.sd_extractor_tables(self.h, _p(self.mvScaleFactor), _p(self.mvInvScaleFactor), _p(self.mvLevelSigma2),
                                    _p(self.mvInvLevelSigma2), _p(self.mnFeaturesPerLevel), _p(self.umax)))

    def __del__(self):
        try:
            lib().sd_extractor_destroy(self.h)
        except Exception:
            pass

    def GetLevels(self):
        n = C.c_int(); s = C.c_float()
        check(lib().sd_extractor_levels(self.h, C.byref(n), C.byref(s)))
        return n.value

    def GetScaleFactor(self):
        n = C.c_int(); s = C.c_float()
        check(lib().sd_extractor_levels(self.h, C.byref(n), C.byref(s)))
        return s.value

    def set_blur_taps(self, taps):
        t = np.asarray(taps, np.uint16)
        check(lib().sd_extractor_set_blur_taps(self.h, _p(t)))

    def level_size(self, width, height, level):
        w = C.c_int(); h = C.c_int()
        check(lib().sd_extractor_level_size(self.h, width, height, level, C.byref(w), C.byref(h)))
        return w.value, h.value


class Batch:
    """Device workspace: batched ORBextractor::operator() + the Frame-side association steps."""

    def __init__(self, extractor, width, height, max_images, handle=None):
        self.ex = extractor
        self.W, self.H, self.max_images = width, height, max_images
        self.owned = handle is None
        self.h = C.c_void_p()
        if handle is None:
            check(lib().sd_batch_create(C.byref(self.h), extractor.h, width, height, max_images))
        else:                                  # a view of the workspace owned by a Tracker
            self.h = C.c_void_p(handle)
        c = C.c_int()
        check(lib().sd_batch_kp_capacity(self.h, C.byref(c)))
        self.cap = c.value

    def close(self):
        if self.h and self.owned:
            lib().sd_batch_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- extraction
    def extract_host(self, images):
        """images: (n, H, W) u8 array (or list of (H, W) arrays)."""
        arr = np.ascontiguousarray(np.stack(images) if isinstance(images, (list, tuple)) else images, np.uint8)
        if arr.ndim == 2:
            arr = arr[None]
        n, h, w = arr.shape
        assert (h, w) == (self.H, self.W)
        check(lib().sd_batch_extract_host(self.h, _p(arr), w, w * h, n))
        return n

    def extract_device(self, d_ptr, stride, pitch, n, stream=None):
        check(lib().sd_batch_extract_device(self.h, C.c_void_p(d_ptr), stride, pitch, n, C.c_void_p(stream or 0)))

    def extract_color_device(self, d_ptr, stride, pitch, n, rgb_order=True, stream=None):
        """cvtColor + operator() for 3-channel images in HBM (GrabImageRGBD's conversion fused into pyramid level 0)."""
        check(lib().sd_batch_extract_color_device(self.h, C.c_void_p(d_ptr), stride, pitch, int(bool(rgb_order)), n,
                                                  C.c_void_p(stream or 0)))

    def extract_pixels_device(self, d_ptr, stride, pitch, n, channels, rgb_order=True, stream=None):
        """Any input GrabImage* accepts: 1 (gray), 3 or 4 channels (Tracking.cc:175-200)."""
        check(lib().sd_batch_extract_pixels_device(self.h, C.c_void_p(d_ptr), stride, pitch, channels, int(bool(rgb_order)), n,
                                                   C.c_void_p(stream or 0)))

    def sync(self):
        check(lib().sd_batch_sync(self.h))

    def counts(self, n):
        out = np.zeros(n, np.int32)
        check(lib().sd_batch_counts(self.h, _p(out), n))
        return out

    def download(self, image):
        kp = np.zeros(self.cap, KP_DTYPE); desc = np.zeros((self.cap, 32), np.uint8)
        per_level = np.zeros(self.ex.nlevels, np.int32)
        n = C.c_int()
        check(lib().sd_batch_download(self.h, image, _p(kp), _p(desc), self.cap, C.byref(n), _p(per_level)))
        return kp[:n.value].copy(), desc[:n.value].copy(), per_level

    def download_keys_un(self, image):
        """mvKeysUn of a slot (== mvKeys unless sd_batch_set_distortion was called with Camera.k1 != 0)."""
        kp = np.zeros(self.cap, KP_DTYPE)
        n = C.c_int()
        check(lib().sd_batch_download_keys_un(self.h, image, _p(kp), self.cap, C.byref(n)))
        return kp[:n.value].copy()

    def download_dynamic_keys_un(self, slot):
        """mvdynKeysUn of a slot, indexed like download_dynamic (== its key points unless a distortion is set)."""
        kp = np.zeros(self.cap, KP_DTYPE)
        n = C.c_int()
        check(lib().sd_batch_download_dynamic_keys_un(self.h, slot, _p(kp), self.cap, C.byref(n)))
        return kp[:n.value].copy()

    def set_distortion(self, K4, dist5):
        k = np.ascontiguousarray(K4, np.float32); d = np.ascontiguousarray(dist5, np.float32)
        check(lib().sd_batch_set_distortion(self.h, _p(k), _p(d)))

    def undistort(self, slots, stream=None):
        sl = np.ascontiguousarray(slots, np.int32)
        check(lib().sd_batch_undistort(self.h, len(sl), _p(sl), C.c_void_p(stream or 0)))

    def pyramid(self, image, level):
        w, h = self.ex.level_size(self.W, self.H, level)
        out = np.zeros((h + 38, w + 38), np.uint8)
        check(lib().sd_batch_download_pyramid(self.h, image, level, _p(out)))
        return out

    def blurred(self, image, level):
        w, h = self.ex.level_size(self.W, self.H, level)
        out = np.zeros((h, w), np.uint8)
        check(lib().sd_batch_download_blurred(self.h, image, level, _p(out)))
        return out

    def candidate_counts(self, image):
        out = np.zeros(self.ex.nlevels, np.int32)
        check(lib().sd_batch_candidate_counts(self.h, image, _p(out)))
        return out

    def results_device(self):
        kp, desc, cnt = C.c_void_p(), C.c_void_p(), C.c_void_p()
        cap = C.c_int()
        check(lib().sd_batch_results_device(self.h, C.byref(kp), C.byref(desc), C.byref(cnt), C.byref(cap)))
        return kp.value, desc.value, cnt.value, cap.value

    def matches_device(self):
        """Device pointers of the projection matcher's per-pair arrays: (d_match, d_pairs, d_npairs, d_nmatches, cap)."""
        m, pr, npr, nm = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        cap = C.c_int()
        check(lib().sd_batch_matches_device(self.h, C.byref(m), C.byref(pr), C.byref(npr), C.byref(nm), C.byref(cap)))
        return m.value, pr.value, npr.value, nm.value, cap.value

    # -- Frame::ComputeStereoMatches
    def stereo_match(self, n_frames, mbf, fx, stream=None):
        check(lib().sd_batch_stereo_match(self.h, n_frames, mbf, fx, C.c_void_p(stream or 0)))

    def download_stereo(self, frame):
        ur = np.zeros(self.cap, np.float32); dep = np.zeros(self.cap, np.float32); sad = np.zeros(self.cap, np.int32)
        check(lib().sd_batch_download_stereo(self.h, frame, _p(ur), _p(dep), _p(sad), self.cap))
        return ur, dep, sad

    # -- Frame::ComputeStereoFromRGBD
    def rgbd_from_u16(self, d_depth_ptr, stride_elems, pitch_elems, n, depth_factor, mbf, stream=None):
        check(lib().sd_batch_rgbd_from_u16(self.h, C.c_void_p(d_depth_ptr), stride_elems, pitch_elems, n, depth_factor,
                                           mbf, C.c_void_p(stream or 0)))

    def rgbd_from_f32(self, d_depth_ptr, stride_elems, pitch_elems, n, mbf, stream=None):
        check(lib().sd_batch_rgbd_from_f32(self.h, C.c_void_p(d_depth_ptr), stride_elems, pitch_elems, n, mbf,
                                           C.c_void_p(stream or 0)))

    def rgbd_from_f32_scaled(self, d_depth_ptr, stride_elems, pitch_elems, n, depth_factor, mbf, stream=None):
        """A CV_32F depth map times mDepthMapFactor (Tracking.cc:271-272 on a float image), fused into the lookup."""
        check(lib().sd_batch_rgbd_from_f32_scaled(self.h, C.c_void_p(d_depth_ptr), stride_elems, pitch_elems, n, depth_factor,
                                                  mbf, C.c_void_p(stream or 0)))

    def download_rgbd(self, image):
        ur = np.zeros(self.cap, np.float32); dep = np.zeros(self.cap, np.float32)
        check(lib().sd_batch_download_rgbd(self.h, image, _p(ur), _p(dep), self.cap))
        return ur, dep

    # -- Frame grid / UnprojectStereo / ORBmatcher::SearchByProjection(Frame, Frame)
    def assign_grid(self, n_images, cam, stream=None):
        c = camera_array(cam)
        check(lib().sd_batch_assign_grid(self.h, n_images, _p(c), C.c_void_p(stream or 0)))

    def download_grid(self, image):
        out = np.zeros(self.cap, np.int16)
        check(lib().sd_batch_download_grid(self.h, image, _p(out), self.cap))
        return out

    def download_grid_index(self, image):
        """(sortedIdx[:n_in_grid], cellStart[3073]) of a slot: key-point indices by (cell, index) and the start of every cell."""
        idx = np.zeros(self.cap, np.uint16); start = np.zeros(GRID_CELLS + 1, np.uint16)
        n = C.c_int()
        check(lib().sd_batch_download_grid_index(self.h, image, _p(idx), self.cap, _p(start), C.byref(n)))
        return idx[:n.value].copy(), start

    def unproject(self, image_step, n_frames, cam, Twc, stream=None):
        c = camera_array(cam)
        T = np.ascontiguousarray(Twc, np.float32).reshape(n_frames, 16)
        check(lib().sd_batch_unproject(self.h, 0, image_step, n_frames, _p(c), _p(T), C.c_void_p(stream or 0)))

    def set_mappoints(self, image, xw, flags):
        xw = np.ascontiguousarray(xw, np.float32); flags = np.ascontiguousarray(flags, np.uint8)
        check(lib().sd_batch_set_mappoints(self.h, image, _p(xw), _p(flags), len(flags)))

    def download_mappoints(self, image):
        xw = np.zeros((self.cap, 3), np.float32); fl = np.zeros(self.cap, np.uint8)
        check(lib().sd_batch_download_mappoints(self.h, image, _p(xw), _p(fl), self.cap))
        return xw, fl

    def search_by_projection(self, cur_index, last_index, Tcw, Tlw, cam, th, bMono=False,
                             checkOrientation=True, d_occupied=None, d_mp_desc=None, stream=None):
        c = camera_array(cam)
        ci = np.ascontiguousarray(cur_index, np.int32); li = np.ascontiguousarray(last_index, np.int32)
        n_pairs = len(ci)
        Tc = np.ascontiguousarray(Tcw, np.float32).reshape(n_pairs, 16)
        Tl = np.ascontiguousarray(Tlw, np.float32).reshape(n_pairs, 16)
        check(lib().sd_batch_search_by_projection(self.h, n_pairs, _p(ci), _p(li), _p(Tc), _p(Tl), _p(c),
                                                  th, int(bMono), int(checkOrientation), C.c_void_p(d_occupied or 0),
                                                  C.c_void_p(d_mp_desc or 0), C.c_void_p(stream or 0)))

    def search_local_map(self, frame_index, point_offset, d_points, d_point_desc, Tcw, cam, th, nnratio, d_track,
                         d_point_match, d_kp_match, d_nmatches, viewing_cos_limit=0.5, d_occupied=None, stream=None):
        """Tracking::SearchLocalPoints: Frame::isInFrustum + ORBmatcher::SearchByProjection(Frame, MapPoints, th).
        d_* are device pointers (ints); see include/sd_frontend.h for the layouts."""
        c = camera_array(cam)
        fi = np.ascontiguousarray(frame_index, np.int32); po = np.ascontiguousarray(point_offset, np.int32)
        n = len(fi)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(n, 16)
        check(lib().sd_batch_search_local_map(self.h, n, _p(fi), _p(po), C.c_void_p(d_points), C.c_void_p(d_point_desc), _p(T),
                                              _p(c), C.c_float(th), C.c_float(nnratio), C.c_float(viewing_cos_limit),
                                              C.c_void_p(d_occupied or 0), C.c_void_p(d_track), C.c_void_p(d_point_match),
                                              C.c_void_p(d_kp_match), C.c_void_p(d_nmatches), C.c_void_p(stream or 0)))

    # -- Frame::ComputeBoW, ORBmatcher::SearchByBoW
    def compute_bow(self, vocab, image_index, levelsup=4, stream=None):
        ii = np.ascontiguousarray(image_index, np.int32)
        check(lib().sd_batch_compute_bow(self.h, vocab.h, len(ii), _p(ii), levelsup, C.c_void_p(stream or 0)))

    def download_bow(self, image):
        """-> dict(word, value: the BowVector; fv_node, fv_feature: the flattened FeatureVector; f_word, f_weight, f_node: per feature)"""
        cap = self.cap
        bw = np.zeros(cap, np.uint32); bv = np.zeros(cap, np.float64); fn = np.zeros(cap, np.uint32); ff = np.zeros(cap, np.uint32)
        fw = np.zeros(cap, np.uint32); fwt = np.zeros(cap, np.float64); fnd = np.zeros(cap, np.uint32)
        nw, nf = C.c_int(), C.c_int()
        check(lib().sd_batch_download_bow(self.h, image, _p(bw), _p(bv), C.byref(nw), _p(fn), _p(ff), C.byref(nf), _p(fw), _p(fwt), _p(fnd), cap))
        n = int(self.counts(image + 1)[image])
        return dict(word=bw[:nw.value].copy(), value=bv[:nw.value].copy(), fv_node=fn[:nf.value].copy(), fv_feature=ff[:nf.value].copy(),
                    f_word=fw[:n].copy(), f_weight=fwt[:n].copy(), f_node=fnd[:n].copy())

    def search_by_bow(self, kf_index, frame_index, nnratio, checkOrientation=True, d_kf_valid=None, stream=None):
        ki = np.ascontiguousarray(kf_index, np.int32); fi = np.ascontiguousarray(frame_index, np.int32)
        check(lib().sd_batch_search_by_bow(self.h, len(ki), _p(ki), _p(fi), C.c_void_p(d_kf_valid or 0), C.c_float(nnratio),
                                           int(checkOrientation), C.c_void_p(stream or 0)))

    # -- LocalMapping::CreateNewMapPoints: ORBmatcher::SearchForTriangulation, triangulation, the neighbour loop
    def stereo_device(self):
        """Device pointers of mvuRight / mvDepth: (d_uright, d_depth, cap), both [max_images][cap] f32."""
        ur, dep = C.c_void_p(), C.c_void_p()
        cap = C.c_int()
        check(lib().sd_batch_stereo_device(self.h, C.byref(ur), C.byref(dep), C.byref(cap)))
        return ur.value, dep.value, cap.value

    def search_for_triangulation(self, kf1_index, kf2_index, Tcw1, Tcw2, cam, d_has_mp1=None, d_has_mp2=None, only_stereo=False,
                                 checkOrientation=False, stream=None):
        """ORBmatcher::SearchForTriangulation for independent pairs of slots (compute_bow must have run on them); F12 and the epipole
        come from the poses (n, 4, 4) and the camera.  Results: download_matches(pair) -> match[idx1] = idx2, vMatchedPairs, nmatches."""
        c = camera_array(cam)
        a = np.ascontiguousarray(kf1_index, np.int32).reshape(-1); d = np.ascontiguousarray(kf2_index, np.int32).reshape(-1)
        T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(-1, 16); T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(-1, 16)
        if len(d) != len(a) or len(T1) != len(a) or len(T2) != len(a):
            raise ValueError("search_for_triangulation: one slot and one pose per pair and side")
        check(lib().sd_batch_search_for_triangulation(self.h, len(a), _p(a), _p(d), _p(T1), _p(T2), _p(c), C.c_void_p(d_has_mp1 or 0),
                                                      C.c_void_p(d_has_mp2 or 0), int(only_stereo), int(checkOrientation), C.c_void_p(stream or 0)))

    def create_new_map_points(self, kf_index, kf_Tcw, neigh_offset, neigh_index, neigh_Tcw, cam, neigh_median_depth=None, d_kf_has_mp=None,
                              d_neigh_has_mp=None, stream=None):
        """The loop body of LocalMapping::CreateNewMapPoints for len(kf_index) keyframes: keyframe k owns neighbours
        [neigh_offset[k], neigh_offset[k+1]) in GetBestCovisibilityKeyFrames order.  neigh_median_depth None = the stereo / RGB-D baseline
        rule, else the monocular one.  -> (d_new, d_nnew): device pointers of sd_new_map_point [n_kf][cap] and the counts [n_kf]."""
        c = camera_array(cam)
        ki = np.ascontiguousarray(kf_index, np.int32).reshape(-1); off = np.ascontiguousarray(neigh_offset, np.int32).reshape(-1)
        ni = np.ascontiguousarray(neigh_index, np.int32).reshape(-1)
        Tk = np.ascontiguousarray(kf_Tcw, np.float32).reshape(-1, 16); Tn = np.ascontiguousarray(neigh_Tcw, np.float32).reshape(-1, 16)
        md = np.ascontiguousarray(neigh_median_depth, np.float32).reshape(-1) if neigh_median_depth is not None else None
        if len(off) != len(ki) + 1 or len(Tk) != len(ki) or len(Tn) != len(ni) or (len(off) and off[-1] != len(ni)) or (md is not None and len(md) != len(ni)):
            raise ValueError("create_new_map_points: offsets, slots and poses do not fit together")
        d_new, d_nnew = C.c_void_p(), C.c_void_p()
        check(lib().sd_batch_create_new_map_points(self.h, len(ki), _p(ki), _p(Tk), C.c_void_p(d_kf_has_mp or 0), _p(off), _p(ni), _p(Tn),
                                                   _p(md) if md is not None else None, C.c_void_p(d_neigh_has_mp or 0), _p(c),
                                                   C.byref(d_new), C.byref(d_nnew), C.c_void_p(stream or 0)))
        return d_new.value, d_nnew.value

    def download_new_map_points(self, kf):
        """The points keyframe `kf` of the last create_new_map_points created, in creation order (NEW_MAP_POINT_DTYPE)."""
        out = np.zeros(self.cap, NEW_MAP_POINT_DTYPE); n = C.c_int()
        check(lib().sd_batch_download_new_map_points(self.h, kf, _p(out), self.cap, C.byref(n)))
        return out[:n.value].copy()

    # -- LocalMapping::SearchInNeighbors: the search part of ORBmatcher::Fuse(pKF, vpMapPoints, th)
    def fuse(self, kf_index, Tcw, cand_offset, d_cand_point, d_points, d_point_desc, cam, th=3.0, d_kf_state=None, stream=None, *, n_points):
        """Job j = Fuse(slot kf_index[j], entries [cand_offset[j], cand_offset[j+1]) of d_cand_point, th) with pose Tcw[j] (assign_grid must
        have run on the slot).  An entry indexes the n_points records of d_points (sd_map_point) / d_point_desc, or is -1 for a point the
        reference skips.  d_kf_state: [n_jobs][cap] u8 (0 empty, 1 holds a point, 2 holds a bad point), None = all empty.
        -> (d_best, d_hits, d_nfused): device pointers of (bestIdx, bestDist) per entry, sd_fuse_hit per entry slot, the return values."""
        c = camera_array(cam)
        ki = np.ascontiguousarray(kf_index, np.int32).reshape(-1); off = np.ascontiguousarray(cand_offset, np.int32).reshape(-1)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 16)
        if len(off) != len(ki) + 1 or len(T) != len(ki):
            raise ValueError("fuse: one slot and one pose per job, one offset more than jobs")
        d_best, d_hits, d_nfused = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().sd_batch_fuse(self.h, len(ki), _p(ki), _p(T), _p(off), C.c_void_p(d_cand_point or 0), C.c_void_p(d_points or 0),
                                  C.c_void_p(d_point_desc or 0), int(n_points), C.c_void_p(d_kf_state or 0), _p(c), C.c_float(th),
                                  C.byref(d_best), C.byref(d_hits), C.byref(d_nfused), C.c_void_p(stream or 0)))
        self._fuse_sizes = np.diff(off)
        return d_best.value, d_hits.value, d_nfused.value

    def download_fuse(self, job):
        """Job `job` of the last fuse -> (best (n, 2) i32: bestIdx, bestDist per entry; hits (FUSE_HIT_DTYPE) in entry order; nfused)."""
        n = int(self._fuse_sizes[job]) if 0 <= job < len(getattr(self, "_fuse_sizes", ())) else 0
        best = np.zeros((max(n, 1), 2), np.int32); hits = np.zeros(max(n, 1), FUSE_HIT_DTYPE); ne, nf = C.c_int(), C.c_int()
        check(lib().sd_batch_download_fuse(self.h, job, _p(best), _p(hits), n, C.byref(ne), C.byref(nf)))
        return best[:ne.value].copy(), hits[:nf.value].copy(), nf.value

    # -- LoopClosing::ComputeSim3 / SearchAndFuse: the matchers that take a similarity Scw or two keyframes
    def fuse_sim3(self, kf_index, Scw, cand_offset, d_cand_point, d_points, d_point_desc, cam, th=4.0, d_kf_state=None, stream=None, *, n_points):
        """Job j = Fuse(slot kf_index[j], Scw[j], entries, th, vpReplacePoint): the tables and outputs of fuse(), the search without the
        chi-square and uRight tests.  Results through download_fuse."""
        c = camera_array(cam)
        ki = np.ascontiguousarray(kf_index, np.int32).reshape(-1); off = np.ascontiguousarray(cand_offset, np.int32).reshape(-1)
        T = np.ascontiguousarray(Scw, np.float32).reshape(-1, 16)
        if len(off) != len(ki) + 1 or len(T) != len(ki):
            raise ValueError("fuse_sim3: one slot and one similarity per job, one offset more than jobs")
        d_best, d_hits, d_nfused = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().sd_batch_fuse_sim3(self.h, len(ki), _p(ki), _p(T), _p(off), C.c_void_p(d_cand_point or 0), C.c_void_p(d_points or 0),
                                       C.c_void_p(d_point_desc or 0), int(n_points), C.c_void_p(d_kf_state or 0), _p(c), C.c_float(th),
                                       C.byref(d_best), C.byref(d_hits), C.byref(d_nfused), C.c_void_p(stream or 0)))
        self._fuse_sizes = np.diff(off)
        return d_best.value, d_hits.value, d_nfused.value

    def search_by_bow_kf(self, kf1_index, kf2_index, nnratio, checkOrientation=True, d_valid1=None, d_valid2=None, stream=None):
        """Pair p = SearchByBoW(slot kf1_index[p], slot kf2_index[p], vpMatches12) (compute_bow must have run on both).  d_valid1 / d_valid2:
        [n_pairs][cap] u8 device tables or None.  Results: download_matches(pair) -> match[idx1] = idx2 or -1, no pairs, nmatches."""
        k1 = np.ascontiguousarray(kf1_index, np.int32).reshape(-1); k2 = np.ascontiguousarray(kf2_index, np.int32).reshape(-1)
        if len(k1) != len(k2):
            raise ValueError("search_by_bow_kf: one slot per pair and side")
        check(lib().sd_batch_search_by_bow_kf(self.h, len(k1), _p(k1), _p(k2), C.c_void_p(d_valid1 or 0), C.c_void_p(d_valid2 or 0),
                                              C.c_float(nnratio), int(checkOrientation), C.c_void_p(stream or 0)))

    def search_by_projection_sim3(self, kf_index, Scw, cand_offset, d_cand_point, d_points, d_point_desc, d_matched, cam, th=10, stream=None, *,
                                  n_points):
        """Job j = SearchByProjection(slot kf_index[j], Scw[j], entries, vpMatched = row j of d_matched ([n_jobs][cap] i32), th).
        -> (d_assigned, d_best, d_nmatches) device pointers; results through download_projection_sim3."""
        c = camera_array(cam)
        ki = np.ascontiguousarray(kf_index, np.int32).reshape(-1); off = np.ascontiguousarray(cand_offset, np.int32).reshape(-1)
        T = np.ascontiguousarray(Scw, np.float32).reshape(-1, 16)
        if len(off) != len(ki) + 1 or len(T) != len(ki):
            raise ValueError("search_by_projection_sim3: one slot and one similarity per job, one offset more than jobs")
        d_assigned, d_best, d_nm = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().sd_batch_search_by_projection_sim3(self.h, len(ki), _p(ki), _p(T), _p(off), C.c_void_p(d_cand_point or 0), C.c_void_p(d_points or 0),
                                                       C.c_void_p(d_point_desc or 0), int(n_points), C.c_void_p(d_matched or 0), _p(c), int(th),
                                                       C.byref(d_assigned), C.byref(d_best), C.byref(d_nm), C.c_void_p(stream or 0)))
        self._loop_sizes = np.diff(off)
        return d_assigned.value, d_best.value, d_nm.value

    def download_projection_sim3(self, job):
        """Job `job` of the last search_by_projection_sim3 -> (assigned (cap,) i32, best (n, 2) i32, nmatches)."""
        n = int(self._loop_sizes[job]) if 0 <= job < len(getattr(self, "_loop_sizes", ())) else 0
        assigned = np.zeros(self.cap, np.int32); best = np.zeros((max(n, 1), 2), np.int32); ne, nm = C.c_int(), C.c_int()
        check(lib().sd_batch_download_projection_sim3(self.h, job, _p(assigned), self.cap, _p(best), n, C.byref(ne), C.byref(nm)))
        return assigned, best[:ne.value].copy(), nm.value

    # -- Tracking::Relocalization: SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
    def search_by_projection_reloc(self, frame_index, kf_index, Tcw, th, orb_dist, d_kf_point, d_frame_point, d_points, d_point_desc, cam,
                                   d_found=None, stream=None, *, n_points):
        """Job j = SearchByProjection(frame slot frame_index[j] with mTcw = Tcw[j], keyframe slot kf_index[j], sAlreadyFound, th[j],
        orb_dist[j]) (assign_grid must have run on both slots).  d_kf_point / d_frame_point: [n_jobs][cap] i32 device rows (the keyframe's
        points and the frame's mvpMapPoints on entry as indices into d_points, -1 for NULL); d_found: [n_jobs][cap] u8 per keyframe
        feature or None (include/sd_frontend.h).  th / orb_dist: a scalar or one value per job.
        -> (d_frame_point_out, d_from_kf, d_nmatches) device pointers; results through download_reloc_matches."""
        c = camera_array(cam)
        fi = np.ascontiguousarray(frame_index, np.int32).reshape(-1); ki = np.ascontiguousarray(kf_index, np.int32).reshape(-1)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 16)
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(th, np.float32), fi.shape)); o = np.ascontiguousarray(np.broadcast_to(np.asarray(orb_dist, np.int32), fi.shape))
        if len(ki) != len(fi) or len(T) != len(fi):
            raise ValueError("search_by_projection_reloc: one frame slot, one keyframe slot and one pose per job")
        d_fp, d_from, d_nm = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().sd_batch_search_by_projection_reloc(self.h, len(fi), _p(fi), _p(ki), _p(T), _p(t), _p(o), C.c_void_p(d_kf_point or 0),
                                                        C.c_void_p(d_frame_point or 0), C.c_void_p(d_found or 0), C.c_void_p(d_points or 0),
                                                        C.c_void_p(d_point_desc or 0), int(n_points), _p(c), C.byref(d_fp), C.byref(d_from),
                                                        C.byref(d_nm), C.c_void_p(stream or 0)))
        return d_fp.value, d_from.value, d_nm.value

    def download_reloc_matches(self, job):
        """Job `job` of the last search_by_projection_reloc -> (frame_point (cap,) i32, from_kf (cap,) i32, exits (cap,) i32 (SD_RELOC_*),
        best (cap, 2) i32, nmatches)."""
        fp = np.zeros(self.cap, np.int32); fk = np.zeros(self.cap, np.int32); ex = np.zeros(self.cap, np.int32); best = np.zeros((self.cap, 2), np.int32)
        nm = C.c_int()
        check(lib().sd_batch_download_reloc_matches(self.h, job, _p(fp), _p(fk), _p(ex), _p(best), self.cap, C.byref(nm)))
        return fp, fk, ex, best, nm.value

    def relocalize_refine(self, frame_index, kf_index, Tcw, d_kf_point, d_frame_point, d_points, d_point_desc, cam, stream=None, *, n_points):
        """Job j = lines 2292-2358 of Tracking::Relocalization for frame slot frame_index[j] and candidate keyframe slot kf_index[j]: Tcw[j]
        from PnPsolver::iterate, row j of d_frame_point = mvpMapPoints after lines 2300-2309, row j of d_kf_point = the candidate's points
        (both [n_jobs][cap] i32 device rows).  One launch sequence, no host synchronisation.  -> device pointer of the sd_reloc_result
        records; results through download_reloc."""
        c = camera_array(cam)
        fi = np.ascontiguousarray(frame_index, np.int32).reshape(-1); ki = np.ascontiguousarray(kf_index, np.int32).reshape(-1)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 16)
        if len(ki) != len(fi) or len(T) != len(fi):
            raise ValueError("relocalize_refine: one frame slot, one keyframe slot and one pose per job")
        d_res = C.c_void_p()
        check(lib().sd_batch_relocalize_refine(self.h, len(fi), _p(fi), _p(ki), _p(T), C.c_void_p(d_kf_point or 0), C.c_void_p(d_frame_point or 0),
                                               C.c_void_p(d_points or 0), C.c_void_p(d_point_desc or 0), int(n_points), _p(c), C.byref(d_res),
                                               C.c_void_p(stream or 0)))
        return d_res.value

    def relocalize_pnp(self, frame_index, kf_index, problems, d_bow_match, d_kf_point, d_points, d_point_desc, cam, stream=None, *, n_points,
                       probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991):
        """Job j = lines 2256-2358 of Tracking::Relocalization for frame slot frame_index[j] and candidate keyframe slot kf_index[j] as one
        launch sequence: the PnPsolver gather from row j of d_bow_match ([n_jobs][cap] i32 device: point index or -1 per frame key point),
        iterate(problems[j].n_iterations) (problems: PNP_PROBLEM_DTYPE), lines 2300-2309 and the cascade from the device pose.  -> device
        pointer of the sd_reloc_result records; everything through download_reloc_pnp."""
        c = camera_array(cam)
        fi = np.ascontiguousarray(frame_index, np.int32).reshape(-1); ki = np.ascontiguousarray(kf_index, np.int32).reshape(-1)
        pr = np.ascontiguousarray(problems, PNP_PROBLEM_DTYPE).reshape(-1)
        if len(ki) != len(fi) or len(pr) != len(fi):
            raise ValueError("relocalize_pnp: one frame slot, one keyframe slot and one problem record per job")
        d_res = C.c_void_p()
        check(lib().sd_batch_relocalize_pnp(self.h, len(fi), _p(fi), _p(ki), _p(pr), probability, min_inliers, max_iterations, min_set, epsilon, th2,
                                            C.c_void_p(d_bow_match or 0), C.c_void_p(d_kf_point or 0), C.c_void_p(d_points or 0),
                                            C.c_void_p(d_point_desc or 0), int(n_points), _p(c), C.byref(d_res), C.c_void_p(stream or 0)))
        return d_res.value

    def download_reloc_pnp(self, job):
        """Job `job` of the last relocalize_pnp -> dict(pnp (PNP_RESULT_DTYPE scalar), corr (N,) PNP_CORR_DTYPE and inliers (N,) u8 of the
        gathered problem, row (cap,) i32 handed to the cascade, result (RELOC_RESULT_DTYPE scalar), frame_point (cap,), outlier (cap,))."""
        pnp = np.zeros(1, PNP_RESULT_DTYPE); n = C.c_int(); corr = np.zeros(self.cap, PNP_CORR_DTYPE); inl = np.zeros(self.cap, np.uint8)
        row = np.zeros(self.cap, np.int32); res = np.zeros(1, RELOC_RESULT_DTYPE); fp = np.zeros(self.cap, np.int32); out = np.zeros(self.cap, np.uint8)
        check(lib().sd_batch_download_reloc_pnp(self.h, job, _p(pnp), C.byref(n), _p(corr), _p(inl), _p(row), _p(res), _p(fp), _p(out), self.cap))
        return dict(pnp=pnp[0], corr=corr[:n.value].copy(), inliers=inl[:n.value].copy(), row=row, result=res[0], frame_point=fp, outlier=out)

    def download_reloc(self, job):
        """Job `job` of the last relocalize_refine -> (result (RELOC_RESULT_DTYPE scalar), frame_point (cap,) i32, outlier (cap,) u8)."""
        res = np.zeros(1, RELOC_RESULT_DTYPE); fp = np.zeros(self.cap, np.int32); out = np.zeros(self.cap, np.uint8)
        check(lib().sd_batch_download_reloc(self.h, job, _p(res), _p(fp), _p(out), self.cap))
        return res[0], fp, out

    def download_reloc_optimisation(self, job, stage):
        """What optimisation `stage` (0 .. 2) of the job saw -> (edges (POSE_EDGE_DTYPE), outlier per edge (u8), Tcw_in (4, 4))."""
        edges = np.zeros(self.cap, POSE_EDGE_DTYPE); out = np.zeros(self.cap, np.uint8); n = C.c_int(); T = np.zeros(16, np.float32)
        check(lib().sd_batch_download_reloc_optimisation(self.h, job, stage, _p(edges), _p(out), self.cap, C.byref(n), _p(T)))
        return edges[:n.value].copy(), out[:n.value].copy(), T.reshape(4, 4)

    def download_reloc_search(self, job, which):
        """Search `which` (0, 1) of the job -> (frame_point_in, frame_point_out, from_kf, exits (each (cap,) i32), best (cap, 2), nmatches)."""
        rows = [np.zeros(self.cap, np.int32) for _ in range(4)]; best = np.zeros((self.cap, 2), np.int32); nm = C.c_int()
        check(lib().sd_batch_download_reloc_search(self.h, job, which, _p(rows[0]), _p(rows[1]), _p(rows[2]), _p(rows[3]), _p(best), self.cap, C.byref(nm)))
        return rows[0], rows[1], rows[2], rows[3], best, nm.value

    # -- ORBmatcher::SearchBySim3 (LoopClosing::ComputeSim3)
    def search_by_sim3(self, kf1_index, kf2_index, Tcw1, Tcw2, s12, R12, t12, cam, d_points, d_point_desc, d_kf1_point, d_kf2_point,
                       d_matched12, th=7.5, stream=None, *, n_points):
        """Pair p = SearchBySim3(slot kf1_index[p], slot kf2_index[p], vpMatches12, s12[p], R12[p], t12[p], th) with poses Tcw1[p] /
        Tcw2[p] (assign_grid must have run on both slots).  d_points / d_point_desc: n_points sd_map_point records and descriptors;
        d_kf1_point / d_kf2_point / d_matched12: [n_pairs][cap] int32 device tables (include/sd_frontend.h).  Results: download_sim3_matches."""
        c = camera_array(cam)
        k1 = np.ascontiguousarray(kf1_index, np.int32).reshape(-1); k2 = np.ascontiguousarray(kf2_index, np.int32).reshape(-1)
        n = len(k1)
        T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(-1, 16); T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(-1, 16)
        s = np.ascontiguousarray(s12, np.float32).reshape(-1); R = np.ascontiguousarray(R12, np.float32).reshape(-1, 9)
        t = np.ascontiguousarray(t12, np.float32).reshape(-1, 3)
        if not (len(k2) == len(T1) == len(T2) == len(s) == len(R) == len(t) == n):
            raise ValueError("search_by_sim3: one slot pair, two poses and one similarity per pair")
        check(lib().sd_batch_search_by_sim3(self.h, n, _p(k1), _p(k2), _p(T1), _p(T2), _p(s), _p(R), _p(t), _p(c), C.c_float(th),
                                            C.c_void_p(d_points or 0), C.c_void_p(d_point_desc or 0), int(n_points), C.c_void_p(d_kf1_point or 0),
                                            C.c_void_p(d_kf2_point or 0), C.c_void_p(d_matched12 or 0), C.c_void_p(stream or 0)))

    def download_sim3_matches(self, pair):
        """Pair `pair` of the last search_by_sim3 -> (match12 (cap,), vnMatch1 (cap,), vnMatch2 (cap,), nFound); -1 beyond N1 / N2."""
        m12 = np.zeros(self.cap, np.int32); m1 = np.zeros(self.cap, np.int32); m2 = np.zeros(self.cap, np.int32); nf = C.c_int()
        check(lib().sd_batch_download_sim3_matches(self.h, pair, _p(m12), _p(m1), _p(m2), self.cap, C.byref(nf)))
        return m12, m1, m2, nf.value

    def compute_sim3_refine(self, kf1_index, kf2_index, Tcw1, Tcw2, d_ransac, corr_offset, d_corr, d_inliers, d_bow12, cam, d_points,
                            d_point_desc, d_kf1_point, d_kf2_point, th=7.5, th2=10.0, fix_scale=False, stream=None, *, n_points):
        """LoopClosing::ComputeSim3 after the RANSAC for job j = (slot kf1_index[j], slot kf2_index[j]) as one launch sequence: the
        inlier BoW matches, SearchBySim3, the correspondences, OptimizeSim3, matched = ret >= 20 and Scw (include/sd_frontend.h:
        sd_batch_compute_sim3_refine).  d_ransac / d_corr / d_inliers: the device arrays of sd_sim3_ransac_device; corr_offset (n + 1,) host;
        d_bow12 / d_kf1_point / d_kf2_point: [n_jobs][cap] int32 device tables.  Results: download_sim3_refine, download_sim3_refine_stages,
        download_sim3_matches."""
        c = camera_array(cam)
        k1 = np.ascontiguousarray(kf1_index, np.int32).reshape(-1); k2 = np.ascontiguousarray(kf2_index, np.int32).reshape(-1)
        n = len(k1)
        T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(-1, 16); T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(-1, 16)
        off = np.ascontiguousarray(corr_offset, np.int32).reshape(-1)
        if not (len(k2) == len(T1) == len(T2) == len(off) - 1 == n):
            raise ValueError("compute_sim3_refine: one slot pair, two poses and one offset range per job")
        check(lib().sd_batch_compute_sim3_refine(self.h, n, _p(k1), _p(k2), _p(T1), _p(T2), C.c_void_p(d_ransac or 0), _p(off), C.c_void_p(d_corr or 0),
                                                 C.c_void_p(d_inliers or 0), C.c_void_p(d_bow12 or 0), _p(c), C.c_float(th), C.c_float(th2), int(bool(fix_scale)),
                                                 C.c_void_p(d_points or 0), C.c_void_p(d_point_desc or 0), int(n_points), C.c_void_p(d_kf1_point or 0),
                                                 C.c_void_p(d_kf2_point or 0), C.c_void_p(stream or 0)))

    def download_sim3_refine(self, job):
        """Job `job` of the last compute_sim3_refine -> (result (SIM3_REFINE_RESULT_DTYPE scalar), final12 (cap,): the final
        vpMapPointMatches per KF1 feature as idx2 / -2 / -1)."""
        res = np.zeros(1, SIM3_REFINE_RESULT_DTYPE); f12 = np.zeros(self.cap, np.int32)
        check(lib().sd_batch_download_sim3_refine(self.h, job, _p(res), _p(f12), self.cap))
        return res[0], f12

    def download_sim3_refine_stages(self, job):
        """-> (merged12 (cap,): what SearchBySim3 was given, corr (n_built,) SIM3_OPT_CORR_DTYPE, state (n_built,) u8); the search's own
        output comes from download_sim3_matches(job)."""
        m = np.zeros(self.cap, np.int32); corr = np.zeros(self.cap, SIM3_OPT_CORR_DTYPE); st = np.zeros(self.cap, np.uint8); n = C.c_int()
        check(lib().sd_batch_download_sim3_refine_stages(self.h, job, _p(m), _p(corr), _p(st), self.cap, C.byref(n)))
        return m, corr[:n.value].copy(), st[:n.value].copy()

    # -- Tracking::TrackHomo model fit (H / F from the projection matcher's point pairs)
    def estimate_motion(self, stream=None):
        check(lib().sd_batch_estimate_motion(self.h, C.c_void_p(stream or 0)))

    def download_motion(self, pair):
        H = np.zeros(9, np.float64); F = np.zeros(9, np.float64); mh = np.zeros(self.cap, np.uint8); mf = np.zeros(self.cap, np.uint8)
        n, nh, nf, flag = C.c_int(), C.c_int(), C.c_int(), C.c_int(); hf = np.zeros(9, np.float32)
        check(lib().sd_batch_download_motion(self.h, pair, _p(H), _p(F), _p(mh), _p(mf), self.cap, C.byref(n), C.byref(nh), C.byref(nf),
                                             _p(hf), C.byref(flag)))
        return dict(H=H.reshape(3, 3), F=F.reshape(3, 3), mask_h=mh[:n.value].copy(), mask_f=mf[:n.value].copy(), n_h=nh.value, n_f=nf.value,
                    HorF=hf.reshape(3, 3), flag=flag.value)

    def copy_frame(self, src, dst, stream=None):
        check(lib().sd_batch_copy_frame(self.h, src, dst, C.c_void_p(stream or 0)))

    def copy_frames(self, src, dst, stream=None):
        a = np.ascontiguousarray(src, np.int32); d = np.ascontiguousarray(dst, np.int32)
        check(lib().sd_batch_copy_frames(self.h, len(a), _p(a), _p(d), C.c_void_p(stream or 0)))

    def pose_optimize(self, pair_index, Tcw=None, stream=None):
        """Optimizer::PoseOptimization of the Current frame of each listed projection pair (sd_batch_pose_optimize): edges from the
        pair's matches; Tcw (n, 4, 4) = the prior, None = the pose the pair was matched with."""
        pi = np.ascontiguousarray(pair_index, np.int32).reshape(-1)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(len(pi), 16) if Tcw is not None else None
        self._keep_pose = (pi, T)
        check(lib().sd_batch_pose_optimize(self.h, len(pi), _p(pi), _p(T) if T is not None else None, C.c_void_p(stream or 0)))

    def download_pose(self, pair):
        """(Tcw (4, 4) f32, mvbOutlier per Current keypoint (cap,) u8, nInitialCorrespondences, return value)."""
        T = np.zeros(16, np.float32); out = np.zeros(self.cap, np.uint8); ni = C.c_int(); ng = C.c_int()
        check(lib().sd_batch_download_pose(self.h, pair, _p(T), _p(out), self.cap, C.byref(ni), C.byref(ng)))
        return T.reshape(4, 4), out, ni.value, ng.value

    def download_matches(self, pair):
        match = np.zeros(self.cap, np.int32); pairs = np.zeros((self.cap, 2), np.int32)
        npairs = C.c_int(); nm = C.c_int()
        check(lib().sd_batch_download_matches(self.h, pair, _p(match), _p(pairs), self.cap, C.byref(npairs), C.byref(nm)))
        return match, pairs[:npairs.value].copy(), nm.value

    # -- dynamic-object cull: Frame::firstSeparate, Tracking::Separate, Frame::UpdateFrame
    @staticmethod
    def pack_boxes(boxes_list, box_idx_list):
        n = len(boxes_list)
        bx = np.zeros((n, MAXB, 4), np.float64); bi = np.zeros((n, MAXB), np.int32); nb = np.zeros(n, np.int32)
        for k in range(n):
            m = len(boxes_list[k]); nb[k] = m
            if m:
                bx[k, :m] = np.asarray(boxes_list[k], np.float64).reshape(m, 4); bi[k, :m] = box_idx_list[k]
        return bx, nb, bi

    def first_separate(self, slots, boxes_list, box_idx_list, stream=None, packed=None):
        sl = np.ascontiguousarray(slots, np.int32)
        bx, nb, bi = packed if packed is not None else self.pack_boxes(boxes_list, box_idx_list)
        check(lib().sd_batch_first_separate(self.h, len(sl), _p(sl), _p(bx), _p(nb), _p(bi), C.c_void_p(stream or 0)))

    def download_boxes(self, slot):
        nb = C.c_int(); n_all = C.c_int(); n_s = C.c_int()
        bx = np.zeros((MAXB, 4), np.float64); bi = np.zeros(MAXB, np.int32); bs = np.zeros(MAXB, np.int32)
        ko = np.zeros(MAXB, np.int32); st = np.zeros(MAXB + 1, np.int32); it = np.zeros(2 * self.cap, np.int32)
        check(lib().sd_batch_download_boxes(self.h, slot, C.byref(nb), _p(bx), _p(bi), _p(bs), _p(ko), _p(st), _p(it), len(it),
                                            C.byref(n_all), C.byref(n_s)))
        m = nb.value
        return dict(nb=m, boxes=bx[:m].copy(), box_idx=bi[:m].copy(), box_status=bs[:m].copy(), kept_orig=ko[:m].copy(),
                    boxStart=st[:m + 1].copy(), boxItems=it[:st[m]].copy(), n_all=n_all.value, n_static=n_s.value)

    def download_dynamic(self, slot):
        kp = np.zeros(self.cap, KP_DTYPE); desc = np.zeros((self.cap, 32), np.uint8)
        ur = np.zeros(self.cap, np.float32); dep = np.zeros(self.cap, np.float32)
        n = C.c_int()
        check(lib().sd_batch_download_dynamic(self.h, slot, _p(kp), _p(desc), _p(ur), _p(dep), self.cap, C.byref(n)))
        m = n.value
        return kp[:m].copy(), desc[:m].copy(), ur[:m].copy(), dep[:m].copy()

    def separate(self, cur_index, ref_index, HorF, flag, last_box_idx, last_box_status, stream=None, packed_last=None):
        n = len(cur_index)
        ci = np.ascontiguousarray(cur_index, np.int32); ri = np.ascontiguousarray(ref_index, np.int32)
        if HorF is None:                     # HorF / flag from the preceding estimate_motion, on the device
            M = fl = None
        else:
            M = np.ascontiguousarray(HorF, np.float32).reshape(n, 9); fl = np.ascontiguousarray(flag, np.int32)
        if packed_last is not None:
            li, ls, nl = packed_last
        else:
            li = np.zeros((n, MAXB), np.int32); ls = np.zeros((n, MAXB), np.int32); nl = np.zeros(n, np.int32)
            for k in range(n):
                m = len(last_box_idx[k]); nl[k] = m
                li[k, :m] = last_box_idx[k]; ls[k, :m] = last_box_status[k]
        check(lib().sd_batch_separate(self.h, n, _p(ci), _p(ri), _p(M) if M is not None else None, _p(fl) if fl is not None else None, _p(li), _p(ls),
                                      _p(nl), C.c_void_p(stream or 0)))

    def download_separate(self, pair):
        ret = C.c_int(); ds = np.zeros(MAXB + 1, np.int32)
        dyn = np.zeros(2 * self.cap, np.int32); mt = np.zeros((2 * self.cap, 2), np.int32)
        check(lib().sd_batch_download_separate(self.h, pair, C.byref(ret), _p(ds), _p(dyn), _p(mt), len(dyn)))
        n = ds[MAXB]
        return ret.value, ds, dyn[:n].copy(), mt[:n].copy()

    def update_frame(self, only_if_static=True, stream=None):
        check(lib().sd_batch_update_frame(self.h, int(only_if_static), C.c_void_p(stream or 0)))

    # -- PointCloudMapping::generatePointCloud
    def backproject_dense(self, slots, d_color, color_stride, color_pitch, d_depth, depth_stride, depth_pitch, depth_factor, d_mask, mask_stride,
                          mask_pitch, cam, Twc, d_points, cap_points, d_counts, stream=None):
        sl = np.ascontiguousarray(slots, np.int32); c = camera_array(cam)
        T = np.ascontiguousarray(Twc, np.float64).reshape(len(sl), 16)
        check(lib().sd_batch_backproject_dense(self.h, len(sl), _p(sl), C.c_void_p(d_color), color_stride, color_pitch, C.c_void_p(d_depth), depth_stride,
                                               depth_pitch, C.c_float(depth_factor), C.c_void_p(d_mask or 0), mask_stride, mask_pitch, _p(c), _p(T),
                                               C.c_void_p(d_points), cap_points, C.c_void_p(d_counts), C.c_void_p(stream or 0)))

    # -- profiling
    def set_profiling(self, on):
        check(lib().sd_batch_set_profiling(self.h, int(bool(on))))

    def reset_kernel_times(self):
        check(lib().sd_batch_reset_kernel_times(self.h))

    def kernel_times(self):
        n = C.c_int()
        check(lib().sd_batch_kernel_count(self.h, C.byref(n)))
        out = {}
        for i in range(n.value):
            name = C.c_char_p(); ms = C.c_double(); cnt = C.c_int64()
            check(lib().sd_batch_kernel_times(self.h, i, C.byref(name), C.byref(ms), C.byref(cnt)))
            out[name.value.decode()] = (ms.value, cnt.value)
        return out


FUSE_HIT_DTYPE = np.dtype([("cand", "<i4"), ("idx", "<i4"), ("dist", "<i4"), ("action", "<i4"), ("other", "<i4")])     # sd_fuse_hit
FUSE_ADD, FUSE_MEET_KF, FUSE_MEET_BAD, FUSE_MEET_CANDIDATE = 1, 2, 3, 4
MAP_POINT_DTYPE = np.dtype([("xw", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"), ("flags", "<u4")])     # sd_map_point


def distinctive_descriptors(obs_offset, d_obs_desc, d_best_obs, d_desc_out=None, n_points=None, stream=None):
    """MapPoint::ComputeDistinctiveDescriptors for n points in one launch: point p owns observations [obs_offset[p], obs_offset[p+1]) of
    d_obs_desc (32 B each, vDescriptors order).  obs_offset: a device pointer (int, with n_points) or a host array, which is uploaded
    through torch; d_best_obs [n] i32 and d_desc_out (optional, [n][32] u8) are device pointers.  -> the uploaded offsets (keep them
    alive until the launch has run) or None."""
    keep = None
    if isinstance(obs_offset, int):
        if n_points is None:
            raise ValueError("distinctive_descriptors: a device offset table needs n_points")
        d_off, n = obs_offset, n_points
    else:
        import torch
        off = np.ascontiguousarray(obs_offset, np.int32).reshape(-1)
        keep = torch.from_numpy(off).cuda(); d_off, n = keep.data_ptr(), len(off) - 1
    check(lib().sd_distinctive_descriptors_device(int(n), C.c_void_p(d_off or 0), C.c_void_p(d_obs_desc or 0), C.c_void_p(d_best_obs or 0),
                                                  C.c_void_p(d_desc_out or 0), C.c_void_p(stream or 0)))
    return keep


NEW_MAP_POINT_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("xw", "<f4", (3,))])     # sd_new_map_point
MAXB = 64             # SD_MAX_BOXES (include/sd_frontend.h)
GRID_COLS, GRID_ROWS, GRID_CELLS = 64, 48, 64 * 48        # FRAME_GRID_COLS / FRAME_GRID_ROWS (include/Frame.h)
CLOUD_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1")])     # sd_cloud_point
SENSOR_MONOCULAR, SENSOR_STEREO, SENSOR_RGBD = 0, 1, 2


class _Camera(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "mbf", "mb", "mnMinX", "mnMaxX", "mnMinY", "mnMaxY")]


class TrackerParams(C.Structure):
    """sd_tracker_params (include/sd_frontend.h)."""
    _fields_ = [("sensor", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("rgb_order", C.c_int32),
                ("n_lanes", C.c_int32), ("track_last", C.c_int32), ("depth_type", C.c_int32), ("cam", _Camera), ("dist", C.c_float * 5),
                ("fps", C.c_float), ("depth_map_factor", C.c_float), ("th_depth", C.c_float), ("ini_features", C.c_int32), ("lookahead", C.c_int32)]


class LaneResult(C.Structure):
    """sd_lane_result (include/sd_frontend.h)."""
    _fields_ = [("frame_id", C.c_int32), ("cur_slot", C.c_int32), ("last_slot", C.c_int32), ("ref_slot", C.c_int32), ("ref_frame_id", C.c_int32),
                ("track_flag", C.c_int32), ("separate_ret", C.c_int32), ("n_track_matches", C.c_int32), ("n_track_pairs", C.c_int32),
                ("n_h", C.c_int32), ("n_f", C.c_int32), ("n_last_matches", C.c_int32), ("N", C.c_int32), ("N_s", C.c_int32), ("N_d", C.c_int32),
                ("n_boxes", C.c_int32), ("box_idx", C.c_int32 * MAXB), ("box_status", C.c_int32 * MAXB), ("omit", C.c_uint8 * MAXB), ("pad_", C.c_uint8 * 4),
                ("objects", (C.c_double * 4) * MAXB), ("box_velocity", (C.c_double * 2) * MAXB)]


class PoseResult(C.Structure):
    """sd_pose_result (include/sd_frontend.h)."""
    _fields_ = [("Tcw", C.c_float * 16), ("ran", C.c_int32), ("n_matches", C.c_int32), ("n_initial", C.c_int32), ("n_good", C.c_int32),
                ("n_matches_map", C.c_int32), ("ok", C.c_int32)]


class Tracker:
    """sd_tracker: System::TrackStereo / TrackRGBD / TrackMonocular for n_lanes independent camera streams, one frame per lane per call
    (Tracking::GrabImage* -> Frame::Frame -> Track_new's dynamic block -> match vs mLastFrame -> q_frame)."""

    def __init__(self, extractor, cfg, sensor, n_lanes, channels=1, rgb_order=True, track_last=True, depth_f32=False, ini_features=0, lookahead=0):
        """depth_f32: the depth images are CV_32F (Tracking.cc:271-272); ini_features: nFeatures of mpIniORBextractor for monocular lanes
        that are not initialised (Tracking.cc:127-128, 335-338), 0 = none."""
        p = TrackerParams()
        p.depth_type, p.ini_features, p.lookahead = int(bool(depth_f32)), int(ini_features), int(lookahead)
        p.sensor, p.width, p.height, p.channels, p.rgb_order = sensor, cfg["width"], cfg["height"], channels, int(bool(rgb_order))
        p.n_lanes, p.track_last = n_lanes, int(bool(track_last))
        cam = make_camera(cfg)
        for k in ("fx", "fy", "cx", "cy", "mbf", "mb", "mnMinX", "mnMaxX", "mnMinY", "mnMaxY"):
            setattr(p.cam, k, float(cam[k]))
        for k, name in enumerate(("k1", "k2", "p1", "p2", "k3")):
            p.dist[k] = float(cfg.get(name, 0.0))
        p.fps, p.depth_map_factor, p.th_depth = float(cfg["fps"]), float(cfg.get("depth_map_factor", 1.0)), float(cfg.get("th_depth", 0.0))
        self.params, self.ex, self.cfg, self.sensor, self.n_lanes = p, extractor, cfg, sensor, n_lanes
        self.images_per_lane = 2 if sensor == SENSOR_STEREO else 1
        self.h = C.c_void_p()
        check(lib().sd_tracker_create(C.byref(self.h), extractor.h, C.byref(p)))
        bh = C.c_void_p()
        check(lib().sd_tracker_batch(self.h, C.byref(bh)))
        self.batch = Batch(extractor, cfg["width"], cfg["height"], 0, handle=bh.value)
        self.results = (LaneResult * n_lanes)()

    def close(self):
        if self.h:
            self.batch.close()
            lib().sd_tracker_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(lib().sd_tracker_reset(self.h))

    def prefetch(self, d_images, stride, image_pitch, n_frames, d_depth=0, depth_stride=0, depth_pitch=0, stream=None):
        """The history-free half (cvtColor, extraction, undistortion, stereo / RGB-D association) of the next n_frames frames of every lane in one
        batch: images in frame-major order (frame k, lane s, eye e).  The following n_frames track() calls pass d_images = 0."""
        check(lib().sd_tracker_prefetch(self.h, C.c_void_p(d_images), stride, image_pitch, C.c_void_p(d_depth or 0), depth_stride, depth_pitch, n_frames,
                                        C.c_void_p(stream or 0)))

    def record_bytes(self):
        """Bytes of one prefetched-frame record (sd_tracker_prefetched_record_bytes); 0 without lookahead."""
        return int(lib().sd_tracker_prefetched_record_bytes(self.h))

    def export_prefetched(self, first_frame, n_frames, d_records, record_stride=0, stream=None):
        """Frames [first_frame, first_frame + n_frames) of the newest prefetched block -> records at d_records (record_stride bytes apart, 0 = packed),
        frame-major (frame k, lane s)."""
        check(lib().sd_tracker_export_prefetched(self.h, int(first_frame), int(n_frames), C.c_void_p(d_records), int(record_stride or self.record_bytes()),
                                                 C.c_void_p(stream or 0)))

    def import_prefetched(self, d_records, n_frames, record_stride=0, stream=None):
        """n_frames * n_lanes records (frame-major) become the next outstanding prefetched block: frames whose history-free half ran elsewhere."""
        check(lib().sd_tracker_import_prefetched(self.h, C.c_void_p(d_records), int(record_stride or self.record_bytes()), int(n_frames), C.c_void_p(stream or 0)))

    def discard_prefetched(self):
        """A worker drops its newest prefetched block after exporting it."""
        check(lib().sd_tracker_discard_prefetched(self.h))

    def set_state(self, state):
        """state: per lane, bit0 = initialised, bit1 = mState == OK && !mVelocity.empty(); None = the automatic rule."""
        if state is None:
            check(lib().sd_tracker_set_state(self.h, None))
        else:
            st = np.ascontiguousarray(state, np.int32).reshape(self.n_lanes)
            check(lib().sd_tracker_set_state(self.h, _p(st)))

    def set_mappoints(self, xw_list, flags_list):
        """The back end's MapPoints of the frames just tracked: per lane (n, 3) f32 world positions + (n,) u8 flags, or None to keep the
        lane's own stereo points."""
        S, cap = self.n_lanes, self.batch.cap
        xw = np.zeros((S, cap, 3), np.float32); fl = np.zeros((S, cap), np.uint8); n = np.full(S, -1, np.int32)
        for l in range(S):
            if xw_list[l] is None:
                continue
            k = len(flags_list[l]); n[l] = k
            xw[l, :k] = np.asarray(xw_list[l], np.float32).reshape(k, 3); fl[l, :k] = flags_list[l]
        check(lib().sd_tracker_set_mappoints(self.h, _p(xw), _p(fl), _p(n)))

    def track(self, d_images, stride, image_pitch, timestamps, boxes=None, n_boxes=None, d_depth=0, depth_stride=0, depth_pitch=0,
              Tcw=None, Twc=None, stream=None):
        """boxes: (n_lanes, MAXB, 4) f64 with n_boxes (n_lanes,) int32 (-1 = the constructor without boxes), or a list of (k, 4) arrays / None per lane."""
        S = self.n_lanes
        ts = np.ascontiguousarray(timestamps, np.float64).reshape(S)
        if boxes is not None and n_boxes is None:
            bx = np.zeros((S, MAXB, 4), np.float64); nb = np.full(S, -1, np.int32)
            for l in range(S):
                if boxes[l] is not None:
                    a = np.asarray(boxes[l], np.float64).reshape(-1, 4)
                    nb[l] = len(a); bx[l, :len(a)] = a
            boxes, n_boxes = bx, nb
        bp = _p(np.ascontiguousarray(boxes, np.float64)) if boxes is not None else None
        self._keep = (boxes, n_boxes)
        np_ = _p(np.ascontiguousarray(n_boxes, np.int32)) if n_boxes is not None else None
        tc = np.ascontiguousarray(Tcw, np.float32).reshape(S, 16) if Tcw is not None else None
        tw = np.ascontiguousarray(Twc, np.float32).reshape(S, 16) if Twc is not None else None
        check(lib().sd_tracker_track(self.h, C.c_void_p(d_images or 0), stride, image_pitch, C.c_void_p(d_depth or 0), depth_stride, depth_pitch,
                                     bp, np_, _p(ts), _p(tc) if tc is not None else None, _p(tw) if tw is not None else None,
                                     C.cast(self.results, C.c_void_p), C.c_void_p(stream or 0)))
        return self.results

    def set_pose_optimization(self, enable):
        """Opt-in TrackWithMotionModel tail: 2*th retry, PoseOptimization, nmatchesMap (sd_tracker_set_pose_optimization)."""
        check(lib().sd_tracker_set_pose_optimization(self.h, int(bool(enable))))

    def pose_results(self):
        """Per lane sd_pose_result of the last track() call."""
        out = (PoseResult * self.n_lanes)()
        check(lib().sd_tracker_pose_results(self.h, C.cast(out, C.c_void_p)))
        return out


class RefQueue:
    """q_frame of Tracking (Tracking.h:109) with the reference-frame choice of Track_new (Tracking.cc:620-666)."""

    def __init__(self):
        self.h = C.c_void_p()
        check(lib().sd_refqueue_create(C.byref(self.h)))

    def __del__(self):
        try:
            lib().sd_refqueue_destroy(self.h)
        except Exception:
            pass

    def __len__(self):
        n = C.c_int(); check(lib().sd_refqueue_size(self.h, C.byref(n))); return n.value

    def clear(self):
        check(lib().sd_refqueue_clear(self.h))

    def candidate(self, t, has_boxes=True):
        s = C.c_int(); check(lib().sd_refqueue_candidate(self.h, t, int(has_boxes), C.byref(s))); return s.value

    def reject(self):
        a = C.c_int(); check(lib().sd_refqueue_reject(self.h, C.byref(a))); return bool(a.value)

    def push(self, t, slot, has_boxes, max_frames):
        e = C.c_int(); check(lib().sd_refqueue_push(self.h, t, slot, int(has_boxes), max_frames, C.byref(e))); return e.value


def box_track(boxes, last_objects, last_box_idx, last_omit, last_velocity, img_cols, img_rows, cap=MAXB):
    """Frame::boxTrack (src/Frame.cc:481-552) through the C ABI (host code)."""
    n = len(boxes)
    bx = np.zeros((cap, 4), np.float64); bx[:n] = np.asarray(boxes, np.float64).reshape(n, 4)
    lo = np.ascontiguousarray(last_objects, np.float64).reshape(-1, 4)
    li = np.ascontiguousarray(last_box_idx, np.int32); lm = np.ascontiguousarray(last_omit, np.uint8)
    lv = np.ascontiguousarray(last_velocity, np.float64).reshape(-1, 2)
    idx = np.zeros(cap, np.int32); om = np.zeros(cap, np.uint8); vel = np.zeros((cap, 2), np.float64)
    n2 = C.c_int()
    check(lib().sd_box_track(_p(bx), n, cap, _p(lo), len(lo), _p(li), _p(lm), _p(lv), int(img_cols), int(img_rows), _p(idx), _p(om),
                             _p(vel), C.byref(n2)))
    m = n2.value
    return bx[:m].copy(), idx[:m].copy(), om[:m].copy(), vel[:m].copy()


def image_bounds(cols, rows, K4, dist5):
    """Frame::ComputeImageBounds (src/Frame.cc:844-872) through the C ABI -> (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    k = np.ascontiguousarray(K4, np.float32); d = np.ascontiguousarray(dist5, np.float32); b = np.zeros(4, np.float32)
    check(lib().sd_image_bounds(int(cols), int(rows), _p(k), _p(d), _p(b)))
    return b


def distortion_of(cfg):
    return np.array([cfg.get(k, 0.0) for k in ("k1", "k2", "p1", "p2", "k3")], np.float32)


def make_camera(cfg):
    """Frame statics: mb = mbf / fx; bounds = the image rectangle for an undistorted camera (Frame.cc:864-870), the undistorted
    corner points otherwise (ComputeImageBounds)."""
    fx = np.float32(cfg["fx"]); bf = np.float32(cfg["bf"])
    cam = dict(fx=fx, fy=np.float32(cfg["fy"]), cx=np.float32(cfg["cx"]), cy=np.float32(cfg["cy"]), mbf=bf,
               mb=np.float32(bf / fx), mnMinX=np.float32(0), mnMaxX=np.float32(cfg["width"]), mnMinY=np.float32(0),
               mnMaxY=np.float32(cfg["height"]))
    d = distortion_of(cfg)
    if d[0] != 0:
        b = image_bounds(cfg["width"], cfg["height"], [cam["fx"], cam["fy"], cam["cx"], cam["cy"]], d)
        cam.update(mnMinX=b[0], mnMaxX=b[1], mnMinY=b[2], mnMaxY=b[3])
    return cam


def camera_array(cam):
    return np.array([cam[k] for k in ("fx", "fy", "cx", "cy", "mbf", "mb", "mnMinX", "mnMaxX", "mnMinY", "mnMaxY")],
                    np.float32)


def cvt_gray_device(d_src, width, height, src_stride, src_pitch, channels, rgb_order, d_dst, dst_stride, dst_pitch,
                    n_images, stream=None):
    """cvtColor(RGB|BGR[A] -> GRAY) of Tracking::GrabImage* (src/Tracking.cc:175-200,256-269) on device buffers."""
    check(lib().sd_cvt_gray_device(C.c_void_p(d_src), width, height, src_stride, src_pitch, channels, int(rgb_order),
                                   C.c_void_p(d_dst), dst_stride, dst_pitch, n_images, C.c_void_p(stream or 0)))


def depth_to_f32_device(d_src, width, height, src_stride_elems, factor, d_dst, n_images, src_pitch_elems, stream=None):
    check(lib().sd_depth_to_f32_device(C.c_void_p(d_src), width, height, src_stride_elems, factor, C.c_void_p(d_dst),
                                       n_images, src_pitch_elems, C.c_void_p(stream or 0)))


def hamming_matrix_device(d_a, na, d_b, nb, d_out, stream=None):
    check(lib().sd_hamming_matrix_device(C.c_void_p(d_a), na, C.c_void_p(d_b), nb, C.c_void_p(d_out),
                                         C.c_void_p(stream or 0)))


FRAME_BOXES_BYTES = 16 + MAXB * 32 + 3 * MAXB * 4 + (MAXB + 1) * 4 + 4        # sizeof(sd_frame_boxes)


def batch_boxes_device(batch):
    """Device pointer of the per-slot sd_frame_boxes records."""
    p = C.c_void_p()
    check(lib().sd_batch_boxes_device(batch.h, C.byref(p)))
    return p.value


class _DevBytes:
    """Zero-copy view of library-owned HBM for torch (torch.distributed needs tensors)."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


def as_torch_u8(ptr, nbytes):
    import torch
    return torch.as_tensor(_DevBytes(ptr, nbytes), device="cuda")


def DescriptorDistance(a, b):
    """ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1804-1820), host popcount."""
    a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
    return lib().sd_descriptor_distance(_p(a), _p(b))


def device_count():
    n = C.c_int()
    rc = lib().sd_device_count(C.byref(n))
    return n.value if rc == SD_OK else 0


class Vocabulary:
    """ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) as one packed buffer in HBM."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def load_text(cls, path):
        h = C.c_void_p()
        check(lib().sd_vocab_load_text(C.byref(h), str(path).encode()))
        return cls(h)

    @classmethod
    def from_nodes(cls, voc):
        """voc: dict(k, L, scoring, weighting, parent, is_leaf, desc, weight) = the node lines of the text file."""
        h = C.c_void_p()
        par = np.ascontiguousarray(voc["parent"], np.int32); leaf = np.ascontiguousarray(voc["is_leaf"], np.uint8)
        d = np.ascontiguousarray(voc["desc"], np.uint8); w = np.ascontiguousarray(voc["weight"], np.float64)
        check(lib().sd_vocab_from_nodes(C.byref(h), int(voc["k"]), int(voc["L"]), int(voc["scoring"]), int(voc["weighting"]), len(par),
                                        _p(par), _p(leaf), _p(d), _p(w)))
        return cls(h)

    @classmethod
    def from_packed_device(cls, d_ptr, nbytes):
        h = C.c_void_p()
        check(lib().sd_vocab_from_packed_device(C.byref(h), C.c_void_p(d_ptr), C.c_size_t(nbytes)))
        return cls(h)

    @staticmethod
    def packed_bytes(n_nodes):
        f = lib().sd_vocab_packed_bytes
        f.restype = C.c_size_t
        return int(f(int(n_nodes)))

    def info(self):
        v = [C.c_int() for _ in range(6)]
        check(lib().sd_vocab_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("k", "L", "scoring", "weighting", "n_nodes", "n_words"), [x.value for x in v]))

    def packed_device(self):
        p = C.c_void_p(); n = C.c_size_t()
        check(lib().sd_vocab_packed_device(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def nodes(self):
        n = self.info()["n_nodes"]
        par = np.zeros(n, np.int32); nch = np.zeros(n, np.int32); wid = np.zeros(n, np.int32)
        d = np.zeros((n, 32), np.uint8); w = np.zeros(n, np.float64)
        check(lib().sd_vocab_download_nodes(self.h, _p(par), _p(nch), _p(wid), _p(d), _p(w)))
        return dict(parent=par, n_children=nch, word_id=wid, desc=d, weight=w)

    def close(self):
        if self.h:
            lib().sd_vocab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- Optimizer::PoseOptimization on the device (include/sd_frontend.h: sd_pose_optimize_*) ----
POSE_EDGE_DTYPE = np.dtype([("xw", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv_sigma2", "<f4"), ("kp_index", "<i4")])   # sd_pose_edge


def pose_optimize(edge_offset, edges, cams, Tcw):
    """n independent PoseOptimization problems in one launch (sd_pose_optimize_host).  edge_offset (n + 1,) int32, edges (E,)
    POSE_EDGE_DTYPE, cams: one camera dict (make_camera) or a list of n, Tcw (n, 4, 4).  Returns (Tcw (n, 4, 4) f32, outlier (E,) u8,
    n_good (n,) int32)."""
    off = np.ascontiguousarray(edge_offset, np.int32).reshape(-1)
    n = len(off) - 1
    e = np.ascontiguousarray(edges, POSE_EDGE_DTYPE).reshape(-1)
    assert len(e) == off[-1]
    cl = [cams] * n if isinstance(cams, dict) else list(cams)
    keys = ("fx", "fy", "cx", "cy", "mbf", "mb", "mnMinX", "mnMaxX", "mnMinY", "mnMaxY")        # sd_camera; the solver reads fx .. mbf
    c = np.array([[x.get(k, 0.0) for k in keys] for x in cl], np.float32).reshape(n, 10)
    T = np.ascontiguousarray(np.array(Tcw, np.float32).reshape(n, 16))
    out = np.zeros(max(len(e), 1), np.uint8); good = np.zeros(max(n, 1), np.int32)
    check(lib().sd_pose_optimize_host(n, _p(off), _p(e), _p(c), _p(T), _p(out), _p(good)))
    return T.reshape(n, 4, 4), out[:len(e)], good[:n]


# ---- Sim3Solver RANSAC on the device (include/sd_frontend.h: sd_sim3_ransac_*) ----
SIM3_CORR_DTYPE = np.dtype([("xw1", "<f4", (3,)), ("xw2", "<f4", (3,)), ("sigma2_1", "<f4"), ("sigma2_2", "<f4"), ("tag", "<i4")])     # sd_sim3_corr
SIM3_PROBLEM_DTYPE = np.dtype([("Tcw1", "<f4", (16,)), ("Tcw2", "<f4", (16,)), ("K1", "<f4", (4,)), ("K2", "<f4", (4,)), ("fix_scale", "<i4"),
                               ("reserved", "<i4"), ("seed", "<u8")])                                   # sd_sim3_problem; K = fx fy cx cy
SIM3_RESULT_DTYPE = np.dtype([("found", "<i4"), ("no_more", "<i4"), ("iteration", "<i4"), ("n_inliers", "<i4"), ("max_its", "<i4"),
                              ("reserved", "<i4"), ("T12", "<f4", (16,)), ("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4")])   # sd_sim3_result
SIM3_MAX_CORRESPONDENCES, SIM3_MAX_ITERATIONS, SIM3_MAX_PROBLEMS = 4096, 4096, 65535


def sim3_ransac(corr_offset, corr, problems, probability=0.99, min_inliers=20, max_iterations=300, device=False):
    """n independent Sim3Solver::find problems in one launch sequence (sd_sim3_ransac_host; device=True goes through
    sd_sim3_ransac_device with torch-owned device arrays and one explicit synchronisation).  corr_offset (n + 1,) int32, corr (E,)
    SIM3_CORR_DTYPE, problems (n,) SIM3_PROBLEM_DTYPE.  Returns (results (n,) SIM3_RESULT_DTYPE, inliers (E,) u8, in the order of corr)
    in either form; the effective iteration count is results["max_its"]."""
    off = np.ascontiguousarray(corr_offset, np.int32).reshape(-1)
    n = len(off) - 1
    c = np.ascontiguousarray(corr, SIM3_CORR_DTYPE).reshape(-1)
    pr = np.ascontiguousarray(problems, SIM3_PROBLEM_DTYPE).reshape(-1)
    assert len(pr) == n
    res = np.zeros(max(n, 1), SIM3_RESULT_DTYPE); inl = np.zeros(max(len(c), 1), np.uint8)
    if not device:
        check(lib().sd_sim3_ransac_host(n, _p(off), _p(c), _p(pr), probability, min_inliers, max_iterations, _p(res), _p(inl)))
        return res[:n], inl[:len(c)]
    import torch
    lib()
    d_c = torch.from_numpy(c.view(np.uint8).reshape(-1).copy() if len(c) else np.zeros(1, np.uint8)).cuda()
    d_r = torch.zeros(max(n, 1) * SIM3_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_i = torch.zeros(max(len(c), 1), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    check(lib().sd_sim3_ransac_device(n, _p(off), C.c_void_p(d_c.data_ptr()), _p(pr), probability, min_inliers, max_iterations,
                                      C.c_void_p(d_r.data_ptr()), C.c_void_p(d_i.data_ptr()), None, C.c_void_p(stream)))
    torch.cuda.synchronize()
    return d_r.cpu().numpy().view(SIM3_RESULT_DTYPE)[:n].copy(), d_i.cpu().numpy()[:len(c)].copy()


# ---- PnPsolver on the device (include/sd_frontend.h: sd_pnp_ransac_*) ----
PNP_CORR_DTYPE = np.dtype([("xw", "<f4", (3,)), ("uv", "<f4", (2,)), ("sigma2", "<f4"), ("tag", "<i4")])                # sd_pnp_corr
PNP_PROBLEM_DTYPE = np.dtype([("K", "<f4", (4,)), ("seed", "<u8"), ("start_iteration", "<i4"), ("n_iterations", "<i4")])   # sd_pnp_problem; K = fx fy cx cy
PNP_RESULT_DTYPE = np.dtype([("kind", "<i4"), ("no_more", "<i4"), ("iteration", "<i4"), ("n_inliers", "<i4"), ("best_iteration", "<i4"),
                             ("best_inliers", "<i4"), ("n_refines", "<i4"), ("min_inliers", "<i4"), ("max_its", "<i4"), ("reserved", "<i4"),
                             ("Tcw", "<f4", (16,))])                                                      # sd_pnp_result
PNP_MAX_CORRESPONDENCES, PNP_MAX_ITERATIONS, PNP_MAX_PROBLEMS = 4096, 4096, 65535


def pnp_ransac(corr_offset, corr, problems, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991,
               device=False, counts=False):
    """n independent PnPsolver::iterate problems in one launch sequence (sd_pnp_ransac_host; device=True goes through
    sd_pnp_ransac_device with torch-owned device arrays and one explicit synchronisation).  corr_offset (n + 1,) int32, corr (E,)
    PNP_CORR_DTYPE, problems (n,) PNP_PROBLEM_DTYPE; the other arguments are SetRansacParameters'.  Returns (results (n,)
    PNP_RESULT_DTYPE, inliers (E,) u8, in the order of corr) in either form; counts=True appends the debug download: an (n, stride) int32
    array whose row p holds the inlier counts of iterations 1 .. end of problem p and an (n, stride, 12) f64 array of the hypotheses
    (mRi row-major, mti), stride = the largest iteration count the arguments allow."""
    off = np.ascontiguousarray(corr_offset, np.int32).reshape(-1)
    n = len(off) - 1
    c = np.ascontiguousarray(corr, PNP_CORR_DTYPE).reshape(-1)
    pr = np.ascontiguousarray(problems, PNP_PROBLEM_DTYPE).reshape(-1)
    assert len(pr) == n
    res = np.zeros(max(n, 1), PNP_RESULT_DTYPE); inl = np.zeros(max(len(c), 1), np.uint8)
    stride = max([int(max_iterations)] + [int(q["start_iteration"]) + int(q["n_iterations"]) for q in pr]) if counts else 0
    cnt = np.zeros((max(n, 1), max(stride, 1)), np.int32) if counts else None
    pos = np.zeros((max(n, 1), max(stride, 1), 12), np.float64) if counts else None
    if not device:
        check(lib().sd_pnp_ransac_host(n, _p(off), _p(c), _p(pr), probability, min_inliers, max_iterations, min_set, epsilon, th2, _p(res),
                                       _p(inl), _p(cnt) if counts else None, _p(pos) if counts else None, stride))
        return (res[:n], inl[:len(c)], cnt[:n], pos[:n]) if counts else (res[:n], inl[:len(c)])
    import torch
    lib()
    d_c = torch.from_numpy(c.view(np.uint8).reshape(-1).copy() if len(c) else np.zeros(1, np.uint8)).cuda()
    d_r = torch.zeros(max(n, 1) * PNP_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_i = torch.zeros(max(len(c), 1), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros((max(n, 1), max(stride, 1)), dtype=torch.int32, device="cuda") if counts else None
    d_p = torch.zeros((max(n, 1), max(stride, 1), 12), dtype=torch.float64, device="cuda") if counts else None
    stream = torch.cuda.current_stream().cuda_stream
    check(lib().sd_pnp_ransac_device(n, _p(off), C.c_void_p(d_c.data_ptr()), _p(pr), probability, min_inliers, max_iterations, min_set, epsilon,
                                     th2, C.c_void_p(d_r.data_ptr()), C.c_void_p(d_i.data_ptr()),
                                     C.c_void_p(d_n.data_ptr()) if counts else None, C.c_void_p(d_p.data_ptr()) if counts else None, stride,
                                     C.c_void_p(stream)))
    torch.cuda.synchronize()
    out = (d_r.cpu().numpy().view(PNP_RESULT_DTYPE)[:n].copy(), d_i.cpu().numpy()[:len(c)].copy())
    return out + (d_n.cpu().numpy()[:n].copy(), d_p.cpu().numpy()[:n].copy()) if counts else out


# ---- Optimizer::OptimizeSim3 on the device (include/sd_frontend.h: sd_sim3_optimize_*) ----
SIM3_OPT_CORR_DTYPE = np.dtype([("xw1", "<f4", (3,)), ("xw2", "<f4", (3,)), ("obs1", "<f4", (2,)), ("obs2", "<f4", (2,)), ("inv_sigma2_1", "<f4"),
                                ("inv_sigma2_2", "<f4"), ("tag", "<i4")])                               # sd_sim3_opt_corr
SIM3_OPT_PROBLEM_DTYPE = np.dtype([("Tcw1", "<f4", (16,)), ("Tcw2", "<f4", (16,)), ("K1", "<f4", (4,)), ("K2", "<f4", (4,)), ("R12", "<f4", (9,)),
                                   ("t12", "<f4", (3,)), ("s12", "<f4"), ("th2", "<f4"), ("fix_scale", "<i4")])   # sd_sim3_opt_problem; K = fx fy cx cy
SIM3_OPT_RESULT_DTYPE = np.dtype([("ret", "<i4"), ("n_correspondences", "<i4"), ("n_bad", "<i4"), ("more_iterations", "<i4"),
                                  ("iterations", "<i4", (2,)), ("trials", "<i4", (2,)), ("stop", "<i4", (2,)), ("written", "<i4"),
                                  ("reserved", "<i4"), ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"), ("T12", "<f4", (16,))])   # sd_sim3_opt_result
assert SIM3_OPT_CORR_DTYPE.itemsize == 52 and SIM3_OPT_PROBLEM_DTYPE.itemsize == 220 and SIM3_OPT_RESULT_DTYPE.itemsize == 176
SIM3_REFINE_RESULT_DTYPE = np.dtype([("ran", "<i4"), ("matched", "<i4"), ("n_built", "<i4"), ("reserved", "<i4"), ("Scw_q", "<f8", (4,)),
                                     ("Scw_t", "<f8", (3,)), ("Scw_s", "<f8"), ("Scw", "<f4", (16,)), ("opt", SIM3_OPT_RESULT_DTYPE)])   # sd_sim3_refine_result
assert SIM3_REFINE_RESULT_DTYPE.itemsize == 320
SIM3_OPT_STOP_OK, SIM3_OPT_STOP_TRIALS, SIM3_OPT_STOP_RHO_ZERO, SIM3_OPT_STOP_NO_GAIN = 0, 1, 2, 3


def sim3_optimize(corr_offset, corr, problems, device=False):
    """n independent Optimizer::OptimizeSim3 problems in one launch (sd_sim3_optimize_host; device=True goes through
    sd_sim3_optimize_device with torch-owned device arrays and one explicit synchronisation).  corr_offset (n + 1,) int32, corr (E,)
    SIM3_OPT_CORR_DTYPE, problems (n,) SIM3_OPT_PROBLEM_DTYPE.  Returns (results (n,) SIM3_OPT_RESULT_DTYPE, state (E,) u8 in the
    order of corr: 0 inlier, 1 removed by the first check, 2 set to NULL by the last)."""
    off = np.ascontiguousarray(corr_offset, np.int32).reshape(-1)
    n = len(off) - 1
    c = np.ascontiguousarray(corr, SIM3_OPT_CORR_DTYPE).reshape(-1)
    pr = np.ascontiguousarray(problems, SIM3_OPT_PROBLEM_DTYPE).reshape(-1)
    assert len(pr) == n
    res = np.zeros(max(n, 1), SIM3_OPT_RESULT_DTYPE); st = np.zeros(max(len(c), 1), np.uint8)
    if not device:
        check(lib().sd_sim3_optimize_host(n, _p(off), _p(c), _p(pr), _p(res), _p(st)))
        return res[:n], st[:len(c)]
    import torch
    lib()
    d_c = torch.from_numpy(c.view(np.uint8).reshape(-1).copy() if len(c) else np.zeros(1, np.uint8)).cuda()
    d_r = torch.zeros(max(n, 1) * SIM3_OPT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_s = torch.zeros(max(len(c), 1), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    check(lib().sd_sim3_optimize_device(n, _p(off), C.c_void_p(d_c.data_ptr()), _p(pr), C.c_void_p(d_r.data_ptr()), C.c_void_p(d_s.data_ptr()),
                                        C.c_void_p(stream)))
    torch.cuda.synchronize()
    return d_r.cpu().numpy().view(SIM3_OPT_RESULT_DTYPE)[:n].copy(), d_s.cpu().numpy()[:len(c)].copy()


# ---- Optimizer::LocalBundleAdjustment on the device (include/sd_frontend.h: sd_local_ba_*) ----
BA_KEYFRAME_DTYPE = np.dtype([("Tcw", "<f4", (16,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("mbf", "<f4"), ("fixed", "u1"),
                              ("reserved", "u1", (3,))])                                                # sd_ba_keyframe
BA_EDGE_DTYPE = np.dtype([("kf", "<i4"), ("point", "<i4"), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv_sigma2", "<f4"), ("tag", "<i4"),
                          ("reserved", "<i4")])                                                         # sd_ba_edge
BA_STATS_DTYPE = np.dtype([("iterations", "<i4", (2,)), ("trials", "<i4", (2,)), ("rejected", "<i4", (2,)), ("n_level1", "<i4"),
                           ("n_erased", "<i4"), ("chi2", "<f8", (2,))])                                 # sd_ba_stats


def pack_ba_problems(problems):
    """The tables of sd_local_ba_*: (kf_offset, n_local, point_offset, edge_offset, kfs, xw, edges, ref_kf) of a list of problems, each
    dict(kfs (BA_KEYFRAME_DTYPE, local keyframes first), n_local, xw (P, 3), edges (BA_EDGE_DTYPE, insertion order), ref_kf (P,))."""
    kfs = [np.ascontiguousarray(p["kfs"]).view(BA_KEYFRAME_DTYPE).reshape(-1) for p in problems]
    xw = [np.ascontiguousarray(p["xw"], np.float32).reshape(-1, 3) for p in problems]
    ed = [np.ascontiguousarray(p["edges"]).view(BA_EDGE_DTYPE).reshape(-1) for p in problems]
    ref = [np.ascontiguousarray(p["ref_kf"], np.int32).reshape(-1) for p in problems]
    for x, r in zip(xw, ref):
        assert len(x) == len(r)
    off = lambda parts: np.concatenate([[0], np.cumsum([len(a) for a in parts])]).astype(np.int32)
    cat = lambda parts, dt, tail: np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0,) + tail, dt)
    return (off(kfs), np.array([int(p["n_local"]) for p in problems], np.int32), off(xw), off(ed), cat(kfs, BA_KEYFRAME_DTYPE, ()),
            cat(xw, np.float32, (3,)), cat(ed, BA_EDGE_DTYPE, ()), cat(ref, np.int32, ()))


BA_PHASES = ("index_lists", "linearisation", "schur_assembly", "factorisation", "solves", "update_chi2")


def local_ba_profile(n_problems, on=None):
    """on = True / False: the profiling switch of sd_local_ba_device.  on = None: (n_problems, 6) milliseconds per phase (BA_PHASES) of the
    last profiled call on this device."""
    if on is not None:
        check(lib().sd_local_ba_set_profiling(int(bool(on))))
        return None
    ms = np.zeros((n_problems, len(BA_PHASES)), np.float64)
    check(lib().sd_local_ba_profile(n_problems, _p(ms)))
    return ms


def local_bundle_adjustment(problems):
    """Independent LocalBundleAdjustment problems in one launch (sd_local_ba_host); see pack_ba_problems for a problem.  Returns one dict
    per problem: Tcw (n_local, 4, 4) f32, xw (P, 3), normal (P, 3), dist (P,), level1 (E,) u8, erase (E,) u8, stats (BA_STATS_DTYPE)."""
    n = len(problems)
    if n == 0:
        return []
    ko, nl, po, eo, kfs, xw, ed, ref = pack_ba_problems(problems)
    nK, nP, nE = max(len(kfs), 1), max(len(xw), 1), max(len(ed), 1)
    T = np.zeros((nK, 16), np.float32); xo = np.zeros((nP, 3), np.float32); nrm = np.zeros((nP, 3), np.float32); dist = np.zeros(nP, np.float32)
    l1 = np.zeros(nE, np.uint8); er = np.zeros(nE, np.uint8); st = np.zeros(n, BA_STATS_DTYPE)
    check(lib().sd_local_ba_host(n, _p(ko), _p(nl), _p(po), _p(eo), _p(kfs), _p(xw), _p(ed), _p(ref), _p(T), _p(xo), _p(nrm), _p(dist), _p(l1),
                                 _p(er), _p(st)))
    return [dict(Tcw=T[ko[q]:ko[q] + nl[q]].reshape(-1, 4, 4).copy(), xw=xo[po[q]:po[q + 1]].copy(), normal=nrm[po[q]:po[q + 1]].copy(),
                 dist=dist[po[q]:po[q + 1]].copy(), level1=l1[eo[q]:eo[q + 1]].copy(), erase=er[eo[q]:eo[q + 1]].copy(), stats=st[q])
            for q in range(n)]


# ---- KeyFrameDatabase on the device (include/sd_frontend.h: sd_kfdb_*) ----
KFDB_INFO_DTYPE = np.dtype([("n_sharing", "<i4"), ("max_common_words", "<i4"), ("min_common_words", "<i4"), ("nscores", "<i4"), ("n_acc", "<i4"),
                            ("n_candidates", "<i4"), ("best_acc_score", "<f4"), ("min_score_to_retain", "<f4")])     # sd_kfdb_query_info
KFDB_MEMBER_DTYPE = np.dtype([("kf_id", "<i4"), ("common_words", "<i4"), ("scored", "<i4"), ("si", "<f4")])       # sd_kfdb_member
KFDB_ACC_DTYPE = np.dtype([("acc_score", "<f4"), ("best_kf", "<i4")])                                              # sd_kfdb_acc
KFDB_MAX_NEIGHBOURS, KFDB_MAX_QUERY_WORDS = 10, 16384


def pack_bow_queries(queries):
    """[(word, value)] or [dict(word, value)] -> the CSR (offset (n + 1,) i32, word u32, value f64) the sd_kfdb_* queries take."""
    qs = [(q["word"], q["value"]) if isinstance(q, dict) else q for q in queries]
    w = [np.ascontiguousarray(a, np.uint32).reshape(-1) for a, _ in qs]
    v = [np.ascontiguousarray(b, np.float64).reshape(-1) for _, b in qs]
    for a, b in zip(w, v):
        assert len(a) == len(b)
    off = np.concatenate([[0], np.cumsum([len(a) for a in w])]).astype(np.int32)
    return off, (np.concatenate(w) if w else np.zeros(0, np.uint32)), (np.concatenate(v) if v else np.zeros(0, np.float64))


def _pack_ids(lists, n):
    """n lists of kf ids -> (offset, ids) i32, or (None, None) for None."""
    if lists is None:
        return None, None
    assert len(lists) == n
    ls = [np.ascontiguousarray(a, np.int32).reshape(-1) for a in lists]
    off = np.concatenate([[0], np.cumsum([len(a) for a in ls])]).astype(np.int32)
    return off, (np.concatenate(ls).astype(np.int32) if ls else np.zeros(0, np.int32))


class KeyFrameDatabase:
    """ORB_SLAM2::KeyFrameDatabase on the device (sd_kfdb_*): add / erase / clear, the covisibility neighbours the two queries read,
    DetectLoopCandidates, DetectRelocalizationCandidates and the score helper.  Keyframes are named by ids in [0, max_keyframes)."""

    def __init__(self, max_keyframes, max_pool_words, max_queries=1, max_query_words=KFDB_MAX_QUERY_WORDS):
        self.h = C.c_void_p()
        check(lib().sd_kfdb_create(C.byref(self.h), max_keyframes, max_pool_words, max_queries, max_query_words))
        self.max_keyframes, self.max_pool_words, self.max_queries, self.max_query_words = max_keyframes, max_pool_words, max_queries, max_query_words

    def close(self):
        if self.h:
            lib().sd_kfdb_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        check(lib().sd_kfdb_clear(self.h))

    def add(self, batch, image_index, kf_id, stream=None):
        """KeyFrameDatabase::add for batch slots with a BowVector (Batch.compute_bow): slot image_index[i] becomes entry kf_id[i]."""
        ii = np.ascontiguousarray(image_index, np.int32).reshape(-1); kk = np.ascontiguousarray(kf_id, np.int32).reshape(-1)
        assert len(ii) == len(kk)
        check(lib().sd_kfdb_add_from_batch(self.h, batch.h, len(ii), _p(ii), _p(kk), C.c_void_p(stream or 0)))

    def add_host(self, kf_id, word, value):
        w = np.ascontiguousarray(word, np.uint32).reshape(-1); v = np.ascontiguousarray(value, np.float64).reshape(-1)
        assert len(w) == len(v)
        check(lib().sd_kfdb_add_host(self.h, int(kf_id), _p(w), _p(v), len(w)))

    def erase(self, kf_id):
        kk = np.ascontiguousarray(kf_id, np.int32).reshape(-1)
        check(lib().sd_kfdb_erase(self.h, len(kk), _p(kk)))

    def set_covisible(self, kf_id, neighbours):
        """neighbours[i] = GetBestCovisibilityKeyFrames(10) of kf_id[i] as a list of at most 10 ids, best first."""
        kk = np.ascontiguousarray(kf_id, np.int32).reshape(-1)
        assert len(kk) == len(neighbours)
        ng = np.zeros((max(len(kk), 1), KFDB_MAX_NEIGHBOURS), np.int32); cnt = np.zeros(max(len(kk), 1), np.int32)
        for r, nb in enumerate(neighbours):
            nb = np.asarray(nb, np.int32).reshape(-1)
            if len(nb) > KFDB_MAX_NEIGHBOURS:
                raise SdError(SD_ERR_INVALID, "more than 10 neighbours")
            ng[r, :len(nb)] = nb; cnt[r] = len(nb)
        check(lib().sd_kfdb_set_covisible(self.h, len(kk), _p(kk), _p(ng), _p(cnt)))

    def set_covisible_from(self, covis, kf_id, stream=None):
        """set_covisible with the first ten of each keyframe's ordered list in a CovisibilityGraph, device to device."""
        kk = np.ascontiguousarray(kf_id, np.int32).reshape(-1)
        check(lib().sd_kfdb_set_covisible_from_covis(self.h, covis.h, len(kk), _p(kk if len(kk) else np.zeros(1, np.int32)), C.c_void_p(stream or 0)))

    def entry(self, kf_id):
        """-> dict(word, value, seq, live, reloc_score, neighbours) of one entry (synchronises)."""
        n, live, nn = C.c_int(), C.c_int(), C.c_int()
        seq = C.c_uint32(); rs = C.c_float()
        ng = np.zeros(KFDB_MAX_NEIGHBOURS, np.int32)
        check(lib().sd_kfdb_download_entry(self.h, int(kf_id), None, None, 0, C.byref(n), C.byref(seq), C.byref(live), C.byref(rs), _p(ng), C.byref(nn)))
        w = np.zeros(max(n.value, 1), np.uint32); v = np.zeros(max(n.value, 1), np.float64)
        check(lib().sd_kfdb_download_entry(self.h, int(kf_id), _p(w), _p(v), len(w), None, None, None, None, None, None))
        return dict(word=w[:n.value].copy(), value=v[:n.value].copy(), seq=int(seq.value), live=bool(live.value),
                    reloc_score=np.float32(rs.value), neighbours=ng[:nn.value].copy())

    def _results(self, n):
        L = lib()
        out = []
        for q in range(n):
            info = np.zeros(1, KFDB_INFO_DTYPE)
            check(L.sd_kfdb_download_candidates(self.h, q, None, 0, _p(info), None, 0, None, 0))
            I = info[0]
            cand = np.zeros(max(int(I["n_candidates"]), 1), np.int32); sh = np.zeros(max(int(I["n_sharing"]), 1), KFDB_MEMBER_DTYPE)
            acc = np.zeros(max(int(I["n_acc"]), 1), KFDB_ACC_DTYPE)
            check(L.sd_kfdb_download_candidates(self.h, q, _p(cand), len(cand), None, _p(sh), len(sh), _p(acc), len(acc)))
            out.append(dict(candidates=cand[:I["n_candidates"]].copy(), info=I.copy(), sharing=sh[:I["n_sharing"]].copy(), acc=acc[:I["n_acc"]].copy()))
        return out

    def _detect(self, reloc, queries, min_score, excluded, batch, device, stream):
        L = lib()
        if batch is not None:
            ii = np.ascontiguousarray(queries, np.int32).reshape(-1)
            n = len(ii)
        else:
            off, w, v = pack_bow_queries(queries)
            n = len(off) - 1
        if not reloc:
            ms = np.ascontiguousarray(np.broadcast_to(np.asarray(min_score, np.float32), (n,)) if n else np.zeros(0, np.float32), np.float32)
            ms = ms if len(ms) else np.zeros(1, np.float32)
            eo, ei = _pack_ids(excluded, n)
            eo_p, ei_p = (_p(eo), _p(ei if len(ei) else np.zeros(1, np.int32))) if eo is not None else (None, None)
        s = C.c_void_p(stream or 0)
        if batch is not None:
            check(L.sd_kfdb_detect_reloc_batch(self.h, batch.h, n, _p(ii), s) if reloc else
                  L.sd_kfdb_detect_loop_batch(self.h, batch.h, n, _p(ii), _p(ms), eo_p, ei_p, s))
        elif device:
            import torch
            d_w = torch.from_numpy(w.view(np.int32).copy() if len(w) else np.zeros(1, np.int32)).cuda()
            d_v = torch.from_numpy(v.copy() if len(v) else np.zeros(1, np.float64)).cuda()
            torch.cuda.synchronize()
            check(L.sd_kfdb_detect_reloc(self.h, n, _p(off), C.c_void_p(d_w.data_ptr()), C.c_void_p(d_v.data_ptr()), s) if reloc else
                  L.sd_kfdb_detect_loop(self.h, n, _p(off), C.c_void_p(d_w.data_ptr()), C.c_void_p(d_v.data_ptr()), _p(ms), eo_p, ei_p, s))
            res = self._results(n)           # synchronises before d_w / d_v go
            return res
        else:
            wq = w if len(w) else np.zeros(1, np.uint32); vq = v if len(v) else np.zeros(1, np.float64)
            check(L.sd_kfdb_detect_reloc_host(self.h, n, _p(off), _p(wq), _p(vq)) if reloc else
                  L.sd_kfdb_detect_loop_host(self.h, n, _p(off), _p(wq), _p(vq), _p(ms), eo_p, ei_p))
        return self._results(n)

    def detect_loop(self, queries, min_score, excluded=None, batch=None, device=False, stream=None):
        """DetectLoopCandidates for a list of queries: BowVectors ((word, value) pairs or dicts), or slots of `batch`.  min_score: a float
        or one per query; excluded: per query the ids of GetConnectedKeyFrames() (None = none).  device=True goes through the device-CSR
        entry point with torch-owned arrays.  Returns one dict per query: candidates (kf ids, the reference's order), info
        (KFDB_INFO_DTYPE), sharing (KFDB_MEMBER_DTYPE, list order), acc (KFDB_ACC_DTYPE, list order)."""
        return self._detect(False, queries, min_score, excluded, batch, device, stream)

    def detect_reloc(self, queries, batch=None, device=False, stream=None):
        """DetectRelocalizationCandidates for a list of queries; results as for detect_loop."""
        return self._detect(True, queries, None, None, batch, device, stream)

    def score(self, queries, lists, stream=None):
        """(float)mpVoc->score(query, entry) for the listed ids of every query -> list of f32 arrays (-1 where the id is not live)."""
        import torch
        off, w, v = pack_bow_queries(queries)
        n = len(off) - 1
        lo, li = _pack_ids(lists, n)
        d_w = torch.from_numpy(w.view(np.int32).copy() if len(w) else np.zeros(1, np.int32)).cuda()
        d_v = torch.from_numpy(v.copy() if len(v) else np.zeros(1, np.float64)).cuda()
        d_s = torch.zeros(max(len(li), 1), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        check(lib().sd_kfdb_score(self.h, n, _p(off), C.c_void_p(d_w.data_ptr()), C.c_void_p(d_v.data_ptr()), _p(lo),
                                  _p(li if len(li) else np.zeros(1, np.int32)), C.c_void_p(d_s.data_ptr()), C.c_void_p(stream or 0)))
        torch.cuda.synchronize()             # the whole device: the call ran on the database's stream
        sc = d_s.cpu().numpy()
        return [sc[lo[q]:lo[q + 1]].copy() for q in range(n)]


# ---- the covisibility graph on the device (include/sd_frontend.h: sd_covis_*) ----
COVIS_KF_INFO_DTYPE = np.dtype([("live", "<i4"), ("n_features", "<i4"), ("is_protected", "<i4"), ("parent", "<i4"), ("first_connection", "<i4"),
                                ("n_ordered", "<i4"), ("n_row", "<i4"), ("n_best", "<i4"), ("n_by_weight", "<i4")])          # sd_covis_keyframe_info
COVIS_CULL_DTYPE = np.dtype([("flag", "<i4"), ("n_mps", "<i4"), ("n_redundant", "<i4")])                                       # sd_covis_cull_result
COVIS_LOCAL_DTYPE = np.dtype([("n_keyframes", "<i4"), ("n_voted", "<i4"), ("reference_kf", "<i4"), ("n_points", "<i4"), ("overflow", "<i4"),
                              ("n_bad_entries", "<i4")])                                                                       # sd_covis_local_info
COVIS_MAX_KEYFRAMES, COVIS_LDS_KEYFRAMES = 8192, 4096


def _i32(a):
    a = np.ascontiguousarray(a, np.int32).reshape(-1)
    return a, (a if len(a) else np.zeros(1, np.int32))


class CovisibilityGraph:
    """The map's covisibility bookkeeping on the device (sd_covis_*): keyframes with their matches, map points' bad flags,
    KeyFrame::UpdateConnections, LocalMapping::KeyFrameCulling and Tracking::UpdateLocalKeyFrames / UpdateLocalPoints.  Keyframes are named
    by ids in [0, max_keyframes) -- those of a KeyFrameDatabase -- and map points by ids in [0, max_points)."""

    def __init__(self, max_keyframes, max_features, max_points, max_jobs=1, max_local_points=1 << 16):
        self.h = C.c_void_p()
        check(lib().sd_covis_create(C.byref(self.h), max_keyframes, max_features, max_points, max_jobs, max_local_points))
        self.max_keyframes, self.max_features, self.max_points, self.max_jobs, self.max_local_points = max_keyframes, max_features, max_points, max_jobs, max_local_points

    def close(self):
        if self.h:
            lib().sd_covis_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        check(lib().sd_covis_clear(self.h))

    def add(self, batch, image_index, kf_id, protected=None, stream=None):
        """Batch slots become keyframes (octave, uRight >= 0 and depth copied on the device); no matches, no connections."""
        ii, iip = _i32(image_index); kk, kkp = _i32(kf_id)
        assert len(ii) == len(kk)
        pr = None if protected is None else np.ascontiguousarray(protected, np.uint8).reshape(-1)
        assert pr is None or len(pr) == len(kk)
        check(lib().sd_covis_add_from_batch(self.h, batch.h, len(ii), _p(iip), _p(kkp), None if pr is None or not len(pr) else _p(pr), C.c_void_p(stream or 0)))

    def add_host(self, kf_id, octave, uright, depth, protected=False):
        o = np.ascontiguousarray(octave, np.uint8).reshape(-1); u = np.ascontiguousarray(uright, np.float32).reshape(-1)
        d = np.ascontiguousarray(depth, np.float32).reshape(-1)
        assert len(o) == len(u) == len(d)
        z8, zf = np.zeros(1, np.uint8), np.zeros(1, np.float32)
        check(lib().sd_covis_add_host(self.h, int(kf_id), len(o), _p(o if len(o) else z8), _p(u if len(u) else zf), _p(d if len(d) else zf), int(bool(protected))))

    def set_matches(self, kf_id, idx, mp_id):
        """mvpMapPoints[idx[i]] of keyframe kf_id[i] = mp_id[i] (-1 erases), in list order."""
        kk, kkp = _i32(kf_id); ii, iip = _i32(idx); mm, mmp = _i32(mp_id)
        assert len(kk) == len(ii) == len(mm)
        check(lib().sd_covis_set_matches(self.h, len(kk), _p(kkp), _p(iip), _p(mmp)))

    def set_matches_device(self, kf_id, idx, mp_id, stream=None):
        """The same through the device-array entry point, with torch-owned arrays (every feature listed once: the order is unspecified)."""
        import torch
        kk, kkp = _i32(kf_id); ii, iip = _i32(idx); mm, mmp = _i32(mp_id)
        assert len(kk) == len(ii) == len(mm)
        d = [torch.from_numpy(a.copy()).cuda() for a in (kkp, iip, mmp)]
        torch.cuda.synchronize()
        check(lib().sd_covis_set_matches_device(self.h, len(kk), C.c_void_p(d[0].data_ptr()), C.c_void_p(d[1].data_ptr()), C.c_void_p(d[2].data_ptr()),
                                                C.c_void_p(stream or 0)))
        torch.cuda.synchronize()             # the whole device, before the arrays go

    def set_point_bad(self, mp_id, bad=True):
        mm, mmp = _i32(mp_id)
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(bad, np.uint8), mm.shape), np.uint8)
        check(lib().sd_covis_set_point_bad(self.h, len(mm), _p(mmp), _p(b if len(b) else np.zeros(1, np.uint8))))

    def set_parent(self, kf_id, parent_id):
        kk, kkp = _i32(kf_id); pp, ppp = _i32(parent_id)
        assert len(kk) == len(pp)
        check(lib().sd_covis_set_parent(self.h, len(kk), _p(kkp), _p(ppp)))

    def erase(self, kf_id):
        kk, kkp = _i32(kf_id)
        check(lib().sd_covis_erase_keyframe(self.h, len(kk), _p(kkp)))

    def update_connections(self, kf_id, stream=None):
        """KeyFrame::UpdateConnections for the listed keyframes, as if run in list order."""
        kk, kkp = _i32(kf_id)
        check(lib().sd_covis_update_connections(self.h, len(kk), _p(kkp), C.c_void_p(stream or 0)))

    def connections(self, kf_id, best_n=10, min_weight=0):
        """-> dict(ordered_id, ordered_weight, row_id, row_weight, best (GetBestCovisibilityKeyFrames(best_n)), by_weight
        (GetCovisiblesByWeight(min_weight)), parent, live, first_connection, is_protected) of one keyframe (synchronises)."""
        info = np.zeros(1, COVIS_KF_INFO_DTYPE)
        check(lib().sd_covis_download_connections(self.h, int(kf_id), int(best_n), int(min_weight), None, None, 0, _p(info), None, None, 0))
        I = info[0]
        no, nr = int(I["n_ordered"]), int(I["n_row"])
        oi = np.zeros(max(no, 1), np.int32); ow = np.zeros(max(no, 1), np.int32); ri = np.zeros(max(nr, 1), np.int32); rw = np.zeros(max(nr, 1), np.int32)
        check(lib().sd_covis_download_connections(self.h, int(kf_id), int(best_n), int(min_weight), _p(oi), _p(ow), len(oi), _p(info), _p(ri), _p(rw), len(ri)))
        return dict(ordered_id=oi[:no].copy(), ordered_weight=ow[:no].copy(), row_id=ri[:nr].copy(), row_weight=rw[:nr].copy(),
                    best=oi[:int(I["n_best"])].copy(), by_weight=oi[:int(I["n_by_weight"])].copy(), parent=int(I["parent"]), live=bool(I["live"]),
                    first_connection=bool(I["first_connection"]), is_protected=bool(I["is_protected"]), n_features=int(I["n_features"]))

    def keyframe_culling(self, cand_kf_id, not_erase=None, monocular=False, th_depth=np.inf, stream=None):
        """LocalMapping::KeyFrameCulling over the candidates in list order -> COVIS_CULL_DTYPE array (flag, n_mps, n_redundant)."""
        kk, kkp = _i32(cand_kf_id)
        ne = None if not_erase is None else np.ascontiguousarray(not_erase, np.uint8).reshape(-1)
        assert ne is None or len(ne) == len(kk)
        check(lib().sd_covis_keyframe_culling(self.h, len(kk), _p(kkp), None if ne is None or not len(ne) else _p(ne), int(bool(monocular)),
                                              C.c_float(float(np.float32(th_depth))), C.c_void_p(stream or 0)))
        out = np.zeros(max(len(kk), 1), COVIS_CULL_DTYPE)
        n = C.c_int()
        check(lib().sd_covis_download_culling(self.h, _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def local_map(self, frames, device=False, stream=None):
        """UpdateLocalKeyFrames + UpdateLocalPoints for a list of frames, each its mvpMapPoints as point ids (-1 = null).  device=True goes
        through the device-array entry point with torch-owned arrays.  -> one dict per frame: local_kf, reference_kf, local_points, info
        (COVIS_LOCAL_DTYPE), entry_bad (u8 per entry of the frame)."""
        fr = [np.ascontiguousarray(f, np.int32).reshape(-1) for f in frames]
        off = np.concatenate([[0], np.cumsum([len(f) for f in fr])]).astype(np.int32)
        ids = np.concatenate(fr).astype(np.int32) if fr and off[-1] else np.zeros(1, np.int32)
        bad = np.zeros(max(int(off[-1]), 1), np.uint8)
        if device:
            import torch
            d_id = torch.from_numpy(ids.copy()).cuda(); d_bad = torch.zeros(len(bad), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            check(lib().sd_covis_local_map(self.h, len(fr), _p(off), C.c_void_p(d_id.data_ptr()), C.c_void_p(d_bad.data_ptr()), C.c_void_p(stream or 0)))
        else:
            check(lib().sd_covis_local_map_host(self.h, len(fr), _p(off), _p(ids), _p(bad)))
        out = []
        for q in range(len(fr)):
            info = np.zeros(1, COVIS_LOCAL_DTYPE)
            check(lib().sd_covis_download_local_map(self.h, q, _p(info), None, 0, None, 0))      # synchronises before d_id / d_bad go
            I = info[0]
            lk = np.zeros(max(int(I["n_keyframes"]), 1), np.int32); lp = np.zeros(max(int(I["n_points"]), 1), np.int32)
            check(lib().sd_covis_download_local_map(self.h, q, None, _p(lk), len(lk), _p(lp), len(lp)))
            out.append(dict(local_kf=lk[:I["n_keyframes"]].copy(), reference_kf=int(I["reference_kf"]), local_points=lp[:I["n_points"]].copy(), info=I.copy()))
        if device:
            torch.cuda.synchronize()
            bad = d_bad.cpu().numpy()
        for q in range(len(fr)):
            out[q]["entry_bad"] = bad[off[q]:off[q + 1]].copy()
        return out
