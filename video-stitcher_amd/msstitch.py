"""ctypes binding of libmsstitch.so (the HIP compositor) for tests and bench.py.

PyTorch is used only as plumbing: device memory (torch.uint8/int16/float32 tensors stand in for
cv::cuda::GpuMat) and streams.  There is no CPU fallback: importing works anywhere, but every
compute call raises MsError without a gfx950 device, and load() raises if the library is missing.

Names mirror the reference: cuda::remap -> remap, cuda::pyrDown -> pyr_down, ...,
MultiBandBlender::feed_online/blend -> Compositor.stitch (fused) -- see include/ms_stitch.h.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmsstitch.so")

MS_8UC1, MS_8UC3, MS_16SC1, MS_16SC3, MS_32FC1 = 0, 16, 3, 19, 5
BORDER_CONSTANT, BORDER_REFLECT = 0, 2
INTER_NEAREST, INTER_LINEAR = 0, 1
INTER_LINEAR_FIXPT = 0x101      # cv::remap's CPU arithmetic
PROJ_PLANE, PROJ_CYLINDRICAL, PROJ_SPHERICAL = 0, 1, 2
MAPS_ANALYTIC, MAPS_CUSTOM, MAPS_LENS = 0, 1, 2
SEAM_VORONOI, SEAM_DP = 0, 1          # ms_set_seam_finder
DP_MAX_SIDE = 4096                    # MS_DP_MAX_SIDE: the largest overlap side ms_dp_seams takes
LENS_NONE, LENS_BROWN, LENS_FISHEYE = 0, 1, 2
LENS_CYL_MAX_ELEVATION_DEG = 80
MAPS_MIN_WIDTH, MAPS_MIN_HEIGHT, MAPS_MAX_SIDE = 3, 2, 31744


class MsError(RuntimeError):
    pass


class Image(C.Structure):
    _fields_ = [("data", C.c_void_p), ("step", C.c_size_t), ("cols", C.c_int), ("rows", C.c_int), ("type", C.c_int)]      # PtrStepSz order


class Rect(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int)]

    def tuple(self):
        return (self.x, self.y, self.width, self.height)


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("num_views", C.c_int), ("src_width", C.c_int), ("src_height", C.c_int), ("projection", C.c_int),
                ("warp_scale", C.c_float), ("num_bands", C.c_int), ("enable_cpw", C.c_int),
                ("out_width", C.c_int), ("out_height", C.c_int), ("max_frames", C.c_int),
                ("view_shards", C.c_int), ("view_shard_index", C.c_int), ("cpu_flavour_remap", C.c_int),
                ("debug_simple_kernels", C.c_int), ("warp_lds_stage", C.c_int), ("raster_tile_order", C.c_int),
                ("col_shards", C.c_int), ("col_shard_index", C.c_int), ("update_mask_margin", C.c_int), ("self_check", C.c_int)]


class Lens(C.Structure):
    """ms_lens.  Lens.brown(k1, k2, p1, p2, k3, k4, k5, k6) / Lens.fisheye(k1, k2, k3, k4) fill it; max_theta_deg = 0 is the model's default"""
    _fields_ = [("struct_size", C.c_uint), ("model", C.c_int), ("k", C.c_double * 8), ("max_theta_deg", C.c_double)]

    @classmethod
    def make(cls, model, k=(), max_theta_deg=0.0):
        k = [float(v) for v in k]
        return cls(C.sizeof(cls), model, (C.c_double * 8)(*(k + [0.0] * (8 - len(k)))), float(max_theta_deg))

    @classmethod
    def brown(cls, *k, max_theta_deg=0.0):
        return cls.make(LENS_BROWN, k, max_theta_deg)

    @classmethod
    def fisheye(cls, *k, max_theta_deg=0.0):
        return cls.make(LENS_FISHEYE, k, max_theta_deg)


class PanoFrame(C.Structure):
    """ms_pano_frame: how a panorama image lies on the warper surface (Compositor.pano_frame, or PanoFrame.make for an image of one's own)"""
    _fields_ = [("struct_size", C.c_uint), ("projection", C.c_int), ("scale", C.c_float), ("u0", C.c_int), ("v0", C.c_int), ("wrap_cols", C.c_int),
                ("clamp_rows", C.c_int)]

    @classmethod
    def make(cls, projection, scale, u0, v0, wrap_cols=0, clamp_rows=0):
        return cls(C.sizeof(cls), projection, scale, u0, v0, wrap_cols, clamp_rows)


VIEW_CAMERA, VIEW_SURFACE = 0, 1
VIEW_BGR, VIEW_I420 = 0, 1
PANO_CANVAS, PANO_ROI = 0, 1
VIEW_MAX_FRAMES, VIEW_MAX_JOBS, VIEW_FRAME_GROUP, VIEW_TILE_W, VIEW_TILE_H = 64, 16, 8, 64, 16
VIEW_TILE_I420 = 32      # the I420 form's tiles are 32 x 32 pixels


class View(C.Structure):
    """ms_view: a virtual camera.  look_at_view / cube_face_view fill pinholes; View.camera / View.surface the general forms"""
    _fields_ = [("struct_size", C.c_uint), ("kind", C.c_int), ("width", C.c_int), ("height", C.c_int), ("R", C.c_float * 9), ("K", C.c_float * 9), ("lens", Lens),
                ("projection", C.c_int), ("scale", C.c_float), ("tl_u", C.c_int), ("tl_v", C.c_int)]

    @classmethod
    def camera(cls, width, height, K, R, lens=None):
        v = cls(C.sizeof(cls), VIEW_CAMERA, width, height)
        v.R[:] = [float(x) for x in list(R)]; v.K[:] = [float(x) for x in list(K)]
        v.lens = lens if lens is not None else Lens.make(LENS_NONE)
        v.projection = PROJ_SPHERICAL
        return v

    @classmethod
    def surface(cls, width, height, R, projection, scale, tl_u, tl_v):
        v = cls(C.sizeof(cls), VIEW_SURFACE, width, height)
        v.R[:] = [float(x) for x in list(R)]
        v.lens = Lens.make(LENS_NONE)
        v.projection = projection; v.scale = scale; v.tl_u = tl_u; v.tl_v = tl_v
        return v


class ViewJob(C.Structure):
    _fields_ = [("map_x", Image), ("map_y", Image), ("dst_x", C.c_int), ("dst_y", C.c_int)]


class MipLevel(C.Structure):
    """ms_mip_level: where one level of a panorama's mip chain lies in the frame's buffer (pano_mips_layout)"""
    _fields_ = [("offset", C.c_size_t), ("step", C.c_size_t), ("cols", C.c_int), ("rows", C.c_int)]


class ViewJobAA(C.Structure):
    _fields_ = [("job", ViewJob), ("rho", Image)]


VIEW_MAX_LEVELS = 6
VIEW_POSE_MAX_JOBS, VIEW_POSE_FRAME_GROUP = 8, 8


class ViewPoseJob(C.Structure):
    """ms_view_pose_job: one view of an ms_reproject_poses call (its R is read by view_pose_table only) and where it goes in every destination frame"""
    _fields_ = [("view", View), ("dst_x", C.c_int), ("dst_y", C.c_int)]


class SeamParams(C.Structure):
    _fields_ = [("seam_scale", C.c_double), ("seam_warp_scale", C.c_float), ("dilate", C.c_int), ("estimate_gains", C.c_int)]


class ViewGeom(C.Structure):
    _fields_ = [("roi", Rect)] + [(n, C.c_int) for n in ("top", "left", "bottom", "right", "x_tl", "y_tl", "x_br", "y_br")]


class PanoGeom(C.Structure):
    _fields_ = [("num_bands", C.c_int), ("dst_roi_final", Rect), ("dst_roi", Rect), ("canvas_x", C.c_int), ("canvas_y", C.c_int)]


class RigParams(C.Structure):
    _fields_ = [("num_views", C.c_int), ("src_width", C.c_int), ("src_height", C.c_int), ("hfov_deg", C.c_double),
                ("work_megapix", C.c_double), ("seam_megapix", C.c_double), ("compose_megapix", C.c_double)]


class Rig(C.Structure):
    _fields_ = [("work_scale", C.c_double), ("seam_scale", C.c_double), ("seam_work_aspect", C.c_double), ("compose_scale", C.c_double),
                ("compose_work_aspect", C.c_double), ("warped_image_scale", C.c_float), ("seam_warp_scale", C.c_float),
                ("compose_warp_scale", C.c_float), ("resize_input", C.c_int), ("compose_width", C.c_int), ("compose_height", C.c_int),
                ("K_compose", (C.c_float * 9) * 16), ("K_seam", (C.c_float * 9) * 16), ("R", (C.c_float * 9) * 16)]


class PlanStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("warp_tile_w", C.c_int), ("warp_tile_h", C.c_int), ("n_warp_tiles", C.c_int), ("n_stage1_tiles", C.c_int),
                ("n_stage1_reachable", C.c_int), ("down_tile_w", C.c_int), ("down_tile_h", C.c_int), ("n_down_tiles", C.c_int * 8),
                ("blend_tile_w", C.c_int), ("blend_tile_h", C.c_int), ("n_blend_tiles", C.c_int * 8)]


class MeshMatch(C.Structure):
    _fields_ = [("x1", C.c_float), ("y1", C.c_float), ("x2", C.c_float), ("y2", C.c_float), ("dst", C.c_int)]


class MeshParams(C.Structure):
    _fields_ = [("mesh_cols", C.c_int), ("mesh_rows", C.c_int), ("alphas", C.c_float * 4), ("global_dist", C.c_int),
                ("focal_length", C.c_float), ("compose_scale", C.c_double), ("work_scale", C.c_double), ("wrap_around", C.c_int),
                ("theta_rule", C.c_int), ("max_iterations", C.c_int), ("tolerance", C.c_double)]


class MeshInfo(C.Structure):
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("nnz", C.c_int), ("iterations", C.c_int), ("error", C.c_double)]


class RigMatch(C.Structure):
    _fields_ = [("view_a", C.c_int), ("view_b", C.c_int), ("a", C.c_double * 3), ("b", C.c_double * 3)]


class RigRefineParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("anchor_view", C.c_int), ("huber_rad", C.c_double), ("max_iters", C.c_int), ("step_tol", C.c_double),
                ("min_pair_matches", C.c_int)]


class RigRefineInfo(C.Structure):
    _fields_ = [("iterations", C.c_int), ("stop_reason", C.c_int), ("cost_initial", C.c_double), ("cost_final", C.c_double), ("matches_used", C.c_int),
                ("pairs_used", C.c_int), ("pairs_ignored", C.c_int), ("outliers", C.c_int), ("max_rotation_rad", C.c_double)]


RIG_CONVERGED, RIG_STALLED, RIG_ITERATION_LIMIT = 0, 1, 2


class PairHomography(C.Structure):
    _fields_ = [("view_a", C.c_int), ("view_b", C.c_int), ("H", C.c_double * 9), ("weight", C.c_int)]


class RigEstimateInfo(C.Structure):
    _fields_ = [("focal_estimates", C.c_int), ("tree_parent", C.c_int * 16)]


class RigPxMatch(C.Structure):
    _fields_ = [("view_a", C.c_int), ("view_b", C.c_int), ("a", C.c_double * 2), ("b", C.c_double * 2)]


class RigFocalParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("anchor_view", C.c_int), ("shared_focal", C.c_int), ("max_iters", C.c_int), ("huber_px", C.c_double),
                ("step_tol", C.c_double), ("min_pair_matches", C.c_int)]


class RigFocalInfo(C.Structure):
    _fields_ = [("iterations", C.c_int), ("stop_reason", C.c_int), ("cost_initial", C.c_double), ("cost_final", C.c_double), ("matches_used", C.c_int),
                ("pairs_used", C.c_int), ("pairs_ignored", C.c_int), ("outliers", C.c_int), ("max_rotation_rad", C.c_double), ("max_focal_ratio", C.c_double)]


class RigCoeffParams(C.Structure):
    _fields_ = RigFocalParams._fields_ + [("free_coeffs", C.c_uint)]


class RigCoeffInfo(C.Structure):
    _fields_ = RigFocalInfo._fields_ + [("max_coeff_change", C.c_double)]


class RigPpParams(C.Structure):
    _fields_ = RigFocalParams._fields_ + [("pp_prior", C.c_double)]


class RigPpInfo(C.Structure):
    _fields_ = RigFocalInfo._fields_ + [("max_pp_shift", C.c_double)]


MATCH_MAX_KEYPOINTS = 32768        # MS_MATCH_MAX_KEYPOINTS
WAVE_HORIZ, WAVE_VERT = 0, 1        # ms_wave_correct


class ViewFeatures(C.Structure):
    _fields_ = [("descriptors", Image), ("keypoints", C.POINTER(C.c_float)), ("keypoint_stride", C.c_int), ("n_keypoints", C.c_int), ("width", C.c_int),
                ("height", C.c_int)]


class PairMatchParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("match_conf", C.c_float), ("num_matches_thresh1", C.c_int), ("num_matches_thresh2", C.c_int), ("range_width", C.c_int),
                ("pair_mask", C.POINTER(C.c_ubyte)), ("ransac_reproj_threshold", C.c_double), ("ransac_max_iters", C.c_int), ("ransac_confidence", C.c_double)]


class FeatureMatch(C.Structure):
    _fields_ = [("query", C.c_int), ("train", C.c_int), ("distance", C.c_int), ("inlier", C.c_int)]


class PairMatches(C.Structure):
    _fields_ = [("view_a", C.c_int), ("view_b", C.c_int), ("first", C.c_int), ("count", C.c_int), ("n_forward", C.c_int), ("num_inliers", C.c_int), ("have_H", C.c_int),
                ("H", C.c_double * 9), ("confidence", C.c_double)]


MATCH_MAX_PROBLEMS = 64             # MS_MATCH_MAX_PROBLEMS


class MatchProblem(C.Structure):
    _fields_ = [("query_set", C.c_int), ("train_set", C.c_int)]


class ListMatchParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("ratio", C.c_double), ("find_homography", C.c_int), ("ransac_reproj_threshold", C.c_double), ("ransac_max_iters", C.c_int),
                ("ransac_confidence", C.c_double)]


class GainTrackParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("stride", C.c_int), ("smoothing", C.c_double)]


def gain_track_default_params():
    p = GainTrackParams()
    _chk(load().ms_gain_track_default_params(C.byref(p)))
    return p


class GainTrackCounters(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("solves_ok", C.c_int), ("solves_singular", C.c_int), ("updates_rejected", C.c_int)]


GAIN_PARTIAL_MAGIC = 0x50474d53
GAIN_PARTIAL_HEADER_WORDS = 8       # magic, num_views, active mask, stride, T.x, T.y, T.width, T.height


def parse_gain_partial(partial, n):
    """A partial of an n-view context (int64 cuda tensor or numpy array) -> (header dict, cnt, S) with cnt / S as n x n int64 numpy arrays (the raw sums)."""
    import numpy as np
    a = partial.cpu().numpy() if hasattr(partial, "cpu") else np.asarray(partial)
    w = a[:GAIN_PARTIAL_HEADER_WORDS // 2].view(np.uint32)
    i = w[4:8].view(np.int32)
    hdr = {"magic": int(w[0]), "num_views": int(w[1]), "active": int(w[2]), "stride": int(w[3]), "T": (int(i[0]), int(i[1]), int(i[2]), int(i[3]))}
    body = a[GAIN_PARTIAL_HEADER_WORDS // 2:]
    return hdr, body[:n * n].reshape(n, n).copy(), body[n * n:2 * n * n].reshape(n, n).copy()


GAIN_SAMPLES_MAGIC = 0x56474d53
GAIN_SAMPLES_HEADER_WORDS = 16      # magic, num_views, active mask, stride, T.x, T.y, T.width, T.height, held mask, total bytes, 6 x 0; num_views offsets follow
GAIN_MAX_SAMPLE_BUFS = 4


EXPORTS = [
    "ms_last_error", "ms_version", "ms_device_count", "ms_remap", "ms_resize_linear", "ms_convert_scale_8u", "ms_convert",
    "ms_copy_make_border", "ms_pyr_down", "ms_pyr_up", "ms_subtract_16s", "ms_add_16s", "ms_add_src_weight_32f",
    "ms_normalize_using_weight_32f", "ms_add_src_weight_16s", "ms_normalize_using_weight_16s", "ms_compare_gt_32f", "ms_compare_eq_8u", "ms_set_zero_masked_16sc3",
    "ms_bitwise_and_8u", "ms_dilate3x3_8u", "ms_build_warp_maps", "ms_custom_resize_32f", "ms_warp_roi", "ms_result_roi",
    "ms_calibrate_cameras", "ms_num_bands_rule", "ms_orb_default_params", "ms_orb_detect_and_compute", "ms_find_homography_ransac", "ms_feature_mask",
    "ms_create", "ms_destroy", "ms_set_camera", "ms_set_gain", "ms_build_maps", "ms_build_masks", "ms_set_mask",
    "ms_init_blender", "ms_set_mesh", "ms_set_meshes", "ms_set_mesh_maps", "ms_stitch", "ms_get_result_mask", "ms_get_band_cells", "ms_get_view_geom",
    "ms_get_pano_geom", "ms_get_maps", "ms_get_mask", "ms_get_weight_level", "ms_get_mesh_maps", "ms_stitch_timed",
    "ms_selftest_divide", "ms_selftest_divide_range", "ms_calib_copy", "ms_calib_read", "ms_mesh_triangle_masks", "ms_bgr_to_i420", "ms_calibrate_seam", "ms_nv12_to_bgr", "ms_partial_bytes", "ms_stitch_partial", "ms_stitch_finish", "ms_selftest_cvt_u8", "ms_init_feather", "ms_get_mesh_displacement", "ms_set_mesh_interp", "ms_feed", "ms_blend", "ms_update_mask",
    "ms_mesh_default_params", "ms_mesh_saliency", "ms_create_mesh", "ms_knn_match_hamming2", "ms_bgr_to_i420_batch", "ms_bgr_to_gray", "ms_stitch_i420", "ms_get_i420_rows", "ms_get_col_window", "ms_get_needed_views", "ms_consume_i420", "ms_resize_linear_batch", "ms_nv12_to_bgr_batch",
    "ms_save_tables", "ms_load_tables", "ms_calib_shape", "ms_stitch_nv12", "ms_get_plan_stats", "ms_get_stitch_kernels",
    "ms_set_active_views", "ms_get_active_views",
    "ms_gain_track_default_params", "ms_gain_stats", "ms_track_gains", "ms_get_gains",
    "ms_stitch_nv12_i420", "ms_gain_stats_nv12", "ms_track_gains_nv12", "ms_nv12_resize_linear_batch",
    "ms_gain_partial_bytes", "ms_get_gain_views", "ms_gain_stats_partial", "ms_gain_stats_partial_nv12", "ms_track_gains_from_partials", "ms_get_gain_track_counters",
    "ms_gain_samples_bytes", "ms_get_view_shard", "ms_get_gain_sample_views", "ms_gain_samples", "ms_gain_samples_nv12", "ms_gain_stats_from_samples", "ms_track_gains_from_samples",
    "ms_voronoi_seams", "ms_estimate_gains",
    "ms_set_maps", "ms_get_map_source",
    "ms_lens_check", "ms_lens_project", "ms_set_lens", "ms_get_lens", "ms_build_warp_maps_lens", "ms_warp_roi_lens",
    "ms_warper_rays", "ms_rig_refine_default_params", "ms_rig_accumulate", "ms_refine_rig_rotations", "ms_refine_rig",
    "ms_dp_seams", "ms_set_seam_finder", "ms_get_seam_finder",
    "ms_focals_from_homography", "ms_estimate_rig", "ms_rig_focal_default_params", "ms_rig_focal_accumulate", "ms_refine_rig_cameras", "ms_refine_rig_focals",
    "ms_pair_match_default_params", "ms_match_pairs", "ms_biggest_component", "ms_wave_correct",
    "ms_find_homography_ransac_batch",
    "ms_orb_detect_and_compute_batch",
    "ms_list_match_default_params", "ms_match_lists", "ms_feature_inputs_batch",
    "ms_lens_unproject", "ms_lens_unproject_points", "ms_rig_lens_accumulate", "ms_refine_rig_cameras_lens", "ms_refine_rig_focals_lens",
    "ms_rig_coeff_default_params", "ms_rig_coeff_accumulate", "ms_refine_rig_coeffs", "ms_refine_rig_coeffs_ctx",
    "ms_rig_pp_default_params", "ms_rig_pp_accumulate", "ms_refine_rig_pp", "ms_refine_rig_pp_ctx",
    "ms_look_at_view", "ms_cube_face_view", "ms_get_pano_frame", "ms_build_view_maps", "ms_reproject",
    "ms_pano_mips_layout", "ms_build_pano_mips", "ms_build_view_footprint", "ms_reproject_aa",
    "ms_view_pose_table", "ms_reproject_poses",
]

_lib = None


def load():
    """Load libmsstitch.so; raises (never falls back) if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MsError("libmsstitch.so not built (run video-stitcher_amd/build.sh or __graft_entry__.build()); "
                          "there is no CPU fallback")
        _lib = C.CDLL(os.environ.get("MSSTITCH_LIB", LIB_PATH))       # MSSTITCH_LIB: developer knob for A/B builds of the same ABI
        _lib.ms_last_error.restype = C.c_char_p
        _lib.ms_version.restype = C.c_char_p
    return _lib


def _chk(code):
    if code < 0:
        raise MsError("msstitch error %d: %s" % (code, load().ms_last_error().decode()))
    return code


_TYPES = {}


def _torch():
    import torch
    if not _TYPES:
        _TYPES.update({(torch.uint8, 1): MS_8UC1, (torch.uint8, 3): MS_8UC3, (torch.int16, 1): MS_16SC1,
                       (torch.int16, 3): MS_16SC3, (torch.float32, 1): MS_32FC1})
    return torch


def img(t):
    """torch tensor (H,W) or (H,W,C), last dims contiguous, on the GPU -> ms_image (borrowed)."""
    torch = _torch()
    assert t.is_cuda, "msstitch operates on device memory only"
    cn = 1 if t.dim() == 2 else t.shape[2]
    if t.dim() == 3:
        assert t.stride(2) == 1 and t.stride(1) == cn
    else:
        assert t.stride(1) == 1
    return Image(t.data_ptr(), t.stride(0) * t.element_size(), t.shape[1], t.shape[0], _TYPES[(t.dtype, cn)])


def tensor_of(image, dtype=None):
    """Borrowed ms_image (device memory owned by a context) -> torch tensor COPY."""
    torch = _torch()
    dt = {MS_8UC1: (torch.uint8, 1), MS_8UC3: (torch.uint8, 3), MS_16SC1: (torch.int16, 1), MS_16SC3: (torch.int16, 3),
          MS_32FC1: (torch.float32, 1)}[image.type]
    out = torch.empty((image.rows, image.cols) + ((dt[1],) if dt[1] > 1 else ()), dtype=dt[0], device="cuda")
    row = image.cols * dt[1] * out.element_size()
    import ctypes
    hip = _hip()
    rc = hip.hipMemcpy2D(C.c_void_p(out.data_ptr()), C.c_size_t(row), C.c_void_p(image.data), C.c_size_t(image.step),
                         C.c_size_t(row), C.c_size_t(image.rows), 3)  # hipMemcpyDeviceToDevice
    if rc != 0:
        raise MsError("hipMemcpy2D failed: %d" % rc)
    return out


_hiplib = None


def _hip():
    global _hiplib
    if _hiplib is None:
        _hiplib = C.CDLL("libamdhip64.so")
    return _hiplib


def _stream():
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_count():
    return load().ms_device_count()


def calib_copy(src, dst):
    n = src.numel() * src.element_size()
    _chk(load().ms_calib_copy(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), C.c_size_t(n), _stream()))


def calib_shape(buf, shape):
    """ms_calib_shape: every 128-byte line of `buf` (uint8 tensor, 128-byte aligned) touched once with access shape 0 / 1 / 2 (PMC calibration)"""
    _chk(load().ms_calib_shape(C.c_void_p(buf.data_ptr()), C.c_size_t(buf.numel()), int(shape), _stream()))


def calib_read(src):
    n = src.numel() * src.element_size()
    _chk(load().ms_calib_read(C.c_void_p(src.data_ptr()), C.c_size_t(n), _stream()))


def selftest_divide_range(d_lo, d_hi):
    """(mismatches, quotients checked) of DivBy against IEEE division for every float denominator in [d_lo, d_hi] x all int16 numerators."""
    bad, n = C.c_ulonglong(1), C.c_ulonglong(0)
    _chk(load().ms_selftest_divide_range(C.c_float(d_lo), C.c_float(d_hi), C.byref(bad), C.byref(n), _stream()))
    return bad.value, n.value


def selftest_cvt_u8():
    n = C.c_ulonglong(1)
    _chk(load().ms_selftest_cvt_u8(C.byref(n), _stream()))
    return n.value


def selftest_divide(dens):
    import numpy as np
    d = np.ascontiguousarray(dens, np.float32)
    return _chk(load().ms_selftest_divide(d.ctypes.data_as(C.POINTER(C.c_float)), d.size, _stream()))


# ------------------------------------------------------------------ image ops (allocate dst like the cv::cuda API)

def _new(shape, dtype):
    return _torch().empty(shape, dtype=dtype, device="cuda")


def remap(src, xmap, ymap, interpolation=INTER_LINEAR, border_type=BORDER_CONSTANT):
    dst = _new(tuple(xmap.shape) + tuple(src.shape[2:]), src.dtype)
    _chk(load().ms_remap(C.byref(img(src)), C.byref(img(xmap)), C.byref(img(ymap)), C.byref(img(dst)), interpolation, border_type, _stream()))
    return dst


def resize_linear(src, dsize=None, fx=0.0, fy=0.0):
    import numpy as np
    rows, cols = src.shape[:2]
    if dsize is None:
        dsize = (int(np.rint(cols * fx)), int(np.rint(rows * fy)))   # saturate_cast<int>(double)
    else:
        fx = fy = 0.0
    dst = _new((dsize[1], dsize[0]) + tuple(src.shape[2:]), src.dtype)
    _chk(load().ms_resize_linear(C.byref(img(src)), C.byref(img(dst)), C.c_double(fx), C.c_double(fy), _stream()))
    return dst


def resize_linear_batch(srcs, dsize=None, fx=0.0, fy=0.0):
    """n 8UC3 images of one geometry through cuda::resize's arithmetic in one launch; returns the list of resized tensors."""
    import numpy as np
    rows, cols = srcs[0].shape[:2]
    if dsize is None:
        dsize = (int(np.rint(cols * fx)), int(np.rint(rows * fy)))
    else:
        fx = fy = 0.0
    dsts = [_new((dsize[1], dsize[0], 3), srcs[0].dtype) for _ in srcs]
    n = len(srcs)
    a = (Image * n)(*[img(t) for t in srcs]); b = (Image * n)(*[img(t) for t in dsts])
    _chk(load().ms_resize_linear_batch(a, b, n, C.c_double(fx), C.c_double(fy), _stream()))
    return dsts


def convert_scale_8u(src, alpha, inplace=False):
    dst = src if inplace else _new(src.shape, src.dtype)
    _chk(load().ms_convert_scale_8u(C.byref(img(src)), C.byref(img(dst)), C.c_double(alpha), _stream()))
    return dst


def convert(src, dtype, alpha=1.0):
    dst = _new(src.shape, dtype)
    _chk(load().ms_convert(C.byref(img(src)), C.byref(img(dst)), C.c_double(alpha), _stream()))
    return dst


def copy_make_border(src, top, bottom, left, right, border_type):
    dst = _new((src.shape[0] + top + bottom, src.shape[1] + left + right) + tuple(src.shape[2:]), src.dtype)
    _chk(load().ms_copy_make_border(C.byref(img(src)), C.byref(img(dst)), top, bottom, left, right, border_type, _stream()))
    return dst


def pyr_down(src):
    dst = _new(((src.shape[0] + 1) // 2, (src.shape[1] + 1) // 2) + tuple(src.shape[2:]), src.dtype)
    _chk(load().ms_pyr_down(C.byref(img(src)), C.byref(img(dst)), _stream()))
    return dst


def pyr_up(src):
    dst = _new((src.shape[0] * 2, src.shape[1] * 2) + tuple(src.shape[2:]), src.dtype)
    _chk(load().ms_pyr_up(C.byref(img(src)), C.byref(img(dst)), _stream()))
    return dst


def subtract(a, b, dst=None):
    dst = _new(a.shape, a.dtype) if dst is None else dst
    _chk(load().ms_subtract_16s(C.byref(img(a)), C.byref(img(b)), C.byref(img(dst)), _stream()))
    return dst


def add(a, b, dst=None):
    dst = _new(a.shape, a.dtype) if dst is None else dst
    _chk(load().ms_add_16s(C.byref(img(a)), C.byref(img(b)), C.byref(img(dst)), _stream()))
    return dst


def add_src_weight_32f(src, weight, dst_roi, dst_weight_roi):
    """dst_roi / dst_weight_roi: views (tensor slices) of the pano level, i.e. dst(rc)."""
    _chk(load().ms_add_src_weight_32f(C.byref(img(src)), C.byref(img(weight)), C.byref(img(dst_roi)), C.byref(img(dst_weight_roi)),
                                      dst_roi.shape[1], dst_roi.shape[0], _stream()))


def add_src_weight_16s(src, weight, dst_roi, dst_weight_roi):
    """addSrcWeightGpu16S: 16SC3 src, 16SC1 fixed-point weights (0..256) accumulated into dst(rc) / dst_weight(rc)."""
    _chk(load().ms_add_src_weight_16s(C.byref(img(src)), C.byref(img(weight)), C.byref(img(dst_roi)), C.byref(img(dst_weight_roi)),
                                      src.shape[1], src.shape[0], _stream()))


def normalize_using_weight_16s(weight, src):
    _chk(load().ms_normalize_using_weight_16s(C.byref(img(weight)), C.byref(img(src)), src.shape[1], src.shape[0], _stream()))


def normalize_using_weight_32f(weight, src):
    _chk(load().ms_normalize_using_weight_32f(C.byref(img(weight)), C.byref(img(src)), src.shape[1], src.shape[0], _stream()))


def compare_gt(src, thr):
    dst = _new(src.shape, _torch().uint8)
    _chk(load().ms_compare_gt_32f(C.byref(img(src)), C.c_float(thr), C.byref(img(dst)), _stream()))
    return dst


def compare_eq(src, val):
    dst = _new(src.shape, _torch().uint8)
    _chk(load().ms_compare_eq_8u(C.byref(img(src)), int(val), C.byref(img(dst)), _stream()))
    return dst


def set_zero_masked(image, mask):
    _chk(load().ms_set_zero_masked_16sc3(C.byref(img(image)), C.byref(img(mask)), _stream()))


def bitwise_and(a, b):
    dst = _new(a.shape, a.dtype)
    _chk(load().ms_bitwise_and_8u(C.byref(img(a)), C.byref(img(b)), C.byref(img(dst)), _stream()))
    return dst


def dilate3x3(src):
    dst = _new(src.shape, src.dtype)
    _chk(load().ms_dilate3x3_8u(C.byref(img(src)), C.byref(img(dst)), _stream()))
    return dst


def _rects(rois):
    return (Rect * len(rois))(*[Rect(*[int(v) for v in r]) for r in rois])


def voronoi_seams(rois, masks_dev):
    """VoronoiSeamFinder::find over device masks (uint8 (h, w) tensors, each exactly its ROI's size and contiguous), edited in place.  rois: (x, y, w, h) per view."""
    n = len(masks_dev)
    assert len(rois) == n
    m = (Image * n)(*[img(t) for t in masks_dev])
    _chk(load().ms_voronoi_seams(n, _rects(rois), m, _stream()))
    return masks_dev


def dp_seams(rois, imgs_dev, masks_dev):
    """ms_dp_seams: a minimum-cost seam through every overlap, over device images (uint8 (h, w, 3)) and masks (uint8 (h, w)), each exactly its ROI's size and
    contiguous; the masks are edited in place.  rois: (x, y, w, h) per view."""
    n = len(masks_dev)
    assert len(rois) == n and len(imgs_dev) == n
    a = (Image * n)(*[img(t) for t in imgs_dev]); m = (Image * n)(*[img(t) for t in masks_dev])
    _chk(load().ms_dp_seams(n, _rects(rois), a, m, _stream()))
    return masks_dev


def estimate_gains(rois, imgs_dev, masks_dev):
    """GainCompensator::feed over device images (uint8 (h, w, 3)) and masks (uint8 (h, w)) -> (gains (n,) float64, N (n, n) int32, I (n, n) float64) on the host."""
    import numpy as np
    n = len(imgs_dev)
    assert len(rois) == n and len(masks_dev) == n
    a = (Image * n)(*[img(t) for t in imgs_dev]); m = (Image * n)(*[img(t) for t in masks_dev])
    g, N, I = np.zeros(n, np.float64), np.zeros((n, n), np.int32), np.zeros((n, n), np.float64)
    _chk(load().ms_estimate_gains(n, _rects(rois), a, m, g.ctypes.data_as(C.POINTER(C.c_double)), N.ctypes.data_as(C.POINTER(C.c_int)),
                                  I.ctypes.data_as(C.POINTER(C.c_double)), _stream()))
    return g, N, I


def _fa(v, n):
    import numpy as np
    a = np.ascontiguousarray(v, np.float32).reshape(n)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def build_warp_maps(projection, tl_u, tl_v, rows, cols, k_rinv, scale, t=None):
    torch = _torch()
    mx = _new((rows, cols), torch.float32); my = _new((rows, cols), torch.float32)
    ka, kp = _fa(k_rinv, 9)
    tp = None
    if t is not None:
        ta, tp = _fa(t, 3)
    _chk(load().ms_build_warp_maps(projection, tl_u, tl_v, C.byref(img(mx)), C.byref(img(my)), kp, kp, tp, C.c_float(scale), _stream()))
    return mx, my


def _lens_ptr(lens):
    return C.byref(lens) if lens is not None else None


def lens_check(lens):
    """ms_lens_check (host only): raises MsError for a lens the library refuses"""
    _chk(load().ms_lens_check(_lens_ptr(lens)))


def lens_project(K, lens, ray):
    """ms_lens_project (host only): the camera ray (X, Y, Z) -> ((px, py), seen); (-1, -1) when the lens does not see it"""
    ka, kp = _fa(K, 9)
    r = (C.c_double * 3)(*[float(v) for v in ray])
    px = (C.c_double * 2)()
    seen = C.c_int(-1)
    _chk(load().ms_lens_project(kp, _lens_ptr(lens), r, px, C.byref(seen)))
    return (px[0], px[1]), bool(seen.value)


def lens_unproject(K, lens, px):
    """ms_lens_unproject (host only): the source pixel (px, py) -> (the unit camera ray (3,) float64, seen); the ray is (0, 0, 0) when the lens does not see it"""
    import numpy as np
    ka, kp = _fa(K, 9)
    p = (C.c_double * 2)(float(px[0]), float(px[1]))
    ray = (C.c_double * 3)()
    seen = C.c_int(-1)
    _chk(load().ms_lens_unproject(kp, _lens_ptr(lens), p, ray, C.byref(seen)))
    return np.array(ray[:], np.float64), bool(seen.value)


def lens_unproject_points(K, lens, px):
    """ms_lens_unproject_points (device): px (n, 2) float32 source pixels -> (unit rays (n, 3) float64, seen (n,) bool); unseen points have the ray (0, 0, 0)"""
    import numpy as np
    ka, kp = _fa(K, 9)
    pa = np.ascontiguousarray(px, np.float32).reshape(-1, 2)
    n = len(pa)
    rays = np.empty((max(n, 1), 3), np.float64); seen = np.empty(max(n, 1), np.uint8)
    _chk(load().ms_lens_unproject_points(kp, _lens_ptr(lens), n, pa.ctypes.data_as(C.POINTER(C.c_float)), rays.ctypes.data_as(C.POINTER(C.c_double)),
                                         seen.ctypes.data_as(C.POINTER(C.c_ubyte)), _stream()))
    return rays[:n], seen[:n].astype(bool)


def build_warp_maps_lens(projection, tl_u, tl_v, rows, cols, K, R, lens, scale, out=None):
    """ms_build_warp_maps_lens; out: (map_x, map_y) float32 cuda tensors to fill (views of larger tensors are fine) instead of new ones"""
    torch = _torch()
    mx, my = out if out is not None else (_new((rows, cols), torch.float32), _new((rows, cols), torch.float32))
    ka, kp = _fa(K, 9); ra, rp = _fa(R, 9)
    _chk(load().ms_build_warp_maps_lens(projection, tl_u, tl_v, C.byref(img(mx)), C.byref(img(my)), kp, rp, _lens_ptr(lens), C.c_float(scale), _stream()))
    return mx, my


def look_at_view(yaw_deg, pitch_deg, roll_deg, hfov_deg, width, height):
    """ms_look_at_view (host only): a pan / tilt / zoom pinhole as a View"""
    v = View()
    _chk(load().ms_look_at_view(C.c_double(yaw_deg), C.c_double(pitch_deg), C.c_double(roll_deg), C.c_double(hfov_deg), width, height, C.byref(v)))
    return v


def cube_face_view(face, size):
    """ms_cube_face_view (host only): face 0..5 = front, right, back, left, up, down"""
    v = View()
    _chk(load().ms_cube_face_view(face, size, C.byref(v)))
    return v


def build_view_maps(pano_frame, view, out=None):
    """ms_build_view_maps: the (map_x, map_y) float32 cuda tensors of a View into the panorama image pano_frame describes; out: tensors to fill (views of larger ones are fine)"""
    torch = _torch()
    mx, my = out if out is not None else (_new((view.height, view.width), torch.float32), _new((view.height, view.width), torch.float32))
    _chk(load().ms_build_view_maps(C.byref(pano_frame), C.byref(view), C.byref(img(mx)), C.byref(img(my)), _stream()))
    return mx, my


def reproject_prepared(srcs, dsts, jobs, wrap_cols=0, clamp_rows=0, fmt=VIEW_BGR):
    """ms_reproject with the descriptors marshalled once: srcs / dsts lists of cuda tensors (one per frame), jobs a list of (map_x, map_y, dst_x, dst_y);
    returns a callable(stream_handle=None)"""
    n, m = len(srcs), len(jobs)
    a = (Image * n)(*[img(t) for t in srcs]); b = (Image * n)(*[img(t) for t in dsts])
    jt = (ViewJob * m)(*[ViewJob(img(mx), img(my), dx, dy) for mx, my, dx, dy in jobs])
    fn = load().ms_reproject

    def run(stream=None):
        _chk(fn(a, b, n, jt, m, wrap_cols, clamp_rows, fmt, stream if stream is not None else _stream()))
    run.keep = (srcs, dsts, jobs)
    return run


def reproject(srcs, dsts, jobs, wrap_cols=0, clamp_rows=0, fmt=VIEW_BGR):
    """ms_reproject: every job's view of every source panorama into its rectangle of the matching destination frame, in one launch"""
    reproject_prepared(srcs, dsts, jobs, wrap_cols, clamp_rows, fmt)()
    return dsts


def _pose_jobs(jobs):
    """jobs: a list of (View, dst_x, dst_y) or ViewPoseJob"""
    return (ViewPoseJob * max(1, len(jobs)))(*[j if isinstance(j, ViewPoseJob) else ViewPoseJob(j[0], j[1], j[2]) for j in jobs])


def view_pose_table(jobs, rig_poses=None):
    """ms_view_pose_table (host only): the (n_jobs, n_frames, 9) float32 numpy table of jobs' views under the rig rotations rig_poses ((n_frames, 3, 3) float64;
    None: one frame, every view's own R)"""
    import numpy as np
    P = None if rig_poses is None else np.ascontiguousarray(rig_poses, np.float64).reshape(-1, 9)
    n_frames = 1 if P is None else len(P)
    out = np.empty((len(jobs), n_frames, 9), np.float32)
    _chk(load().ms_view_pose_table(_pose_jobs(jobs), len(jobs), None if P is None else P.ctypes.data_as(C.POINTER(C.c_double)), n_frames,
                                   out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def reproject_poses_prepared(pano_frame, srcs, dsts, jobs, poses, fmt=VIEW_BGR):
    """ms_reproject_poses with the descriptors marshalled once: jobs a list of (View, dst_x, dst_y), poses a cuda float32 tensor of len(jobs) * len(srcs) * 9
    rotations laid out [job][frame][9]; returns a callable(stream_handle=None)"""
    torch = _torch()
    n, m = len(srcs), len(jobs)
    if not (poses.is_cuda and poses.dtype == torch.float32 and poses.is_contiguous() and poses.numel() == m * n * 9):
        raise ValueError("poses must be a contiguous cuda float32 tensor of %d x %d x 9 elements" % (m, n))
    a = (Image * n)(*[img(t) for t in srcs]); b = (Image * n)(*[img(t) for t in dsts])
    jt = _pose_jobs(jobs)
    fn = load().ms_reproject_poses
    pp = C.c_void_p(poses.data_ptr())

    def run(stream=None):
        _chk(fn(C.byref(pano_frame), a, b, n, jt, m, pp, fmt, stream if stream is not None else _stream()))
    run.keep = (srcs, dsts, jobs, poses)
    return run


def reproject_poses(pano_frame, srcs, dsts, jobs, poses, fmt=VIEW_BGR):
    """ms_reproject_poses: every job's view of every source panorama, each frame under its own rotation, in one launch and without maps"""
    reproject_poses_prepared(pano_frame, srcs, dsts, jobs, poses, fmt)()
    return dsts


def pano_mips_layout(cols, rows, levels):
    """ms_pano_mips_layout (host only): ([MipLevel] for levels 1..levels of a cols x rows 8UC3 image, bytes of one frame's buffer)"""
    lv = (MipLevel * VIEW_MAX_LEVELS)(); n = C.c_size_t(0)
    _chk(load().ms_pano_mips_layout(cols, rows, levels, lv, C.byref(n)))
    return [lv[i] for i in range(levels)], n.value


def mip_level_view(buf, level):
    """level (a MipLevel) of the chain in buf (a flat uint8 tensor that starts at the mips buffer's first byte), as a (rows, cols, 3) view"""
    return _torch().as_strided(buf, (level.rows, level.cols, 3), (level.step, 3, 1), buf.storage_offset() + level.offset)


def build_pano_mips(srcs, levels, out=None):
    """ms_build_pano_mips: the mip chains of the panoramas srcs (one launch per three levels, whatever len(srcs) is); out: flat uint8 cuda tensors to fill
    (pano_mips_layout's bytes each, 16-byte aligned) instead of new ones.  Returns the buffers."""
    torch = _torch()
    n = len(srcs)
    if out is None:
        _, nbytes = pano_mips_layout(srcs[0].shape[1], srcs[0].shape[0], levels)
        out = [_new((nbytes,), torch.uint8) for _ in range(n)]
    a = (Image * n)(*[img(t) for t in srcs])
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in out])
    _chk(load().ms_build_pano_mips(a, ptrs, n, levels, _stream()))
    return out


def build_view_footprint(pano_frame, map_x, map_y, footprint_scale=1.0, out=None):
    """ms_build_view_footprint: rho, the side in level-0 panorama pixels of the patch each view pixel covers (float32 cuda tensor of the maps' size)"""
    torch = _torch()
    rho = out if out is not None else _new(tuple(map_x.shape), torch.float32)
    _chk(load().ms_build_view_footprint(C.byref(pano_frame), C.byref(img(map_x)), C.byref(img(map_y)), C.c_double(footprint_scale), C.byref(img(rho)), _stream()))
    return rho


def reproject_aa_prepared(srcs, mips, levels, dsts, jobs, wrap_cols=0, clamp_rows=0, fmt=VIEW_BGR):
    """ms_reproject_aa with the descriptors marshalled once: mips the buffers of build_pano_mips, jobs a list of (map_x, map_y, rho, dst_x, dst_y);
    returns a callable(stream_handle=None)"""
    n, m = len(srcs), len(jobs)
    a = (Image * n)(*[img(t) for t in srcs]); b = (Image * n)(*[img(t) for t in dsts])
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in mips])
    jt = (ViewJobAA * m)(*[ViewJobAA(ViewJob(img(mx), img(my), dx, dy), img(rho)) for mx, my, rho, dx, dy in jobs])
    fn = load().ms_reproject_aa

    def run(stream=None):
        _chk(fn(a, ptrs, levels, b, n, jt, m, wrap_cols, clamp_rows, fmt, stream if stream is not None else _stream()))
    run.keep = (srcs, mips, dsts, jobs)
    return run


def reproject_aa(srcs, mips, levels, dsts, jobs, wrap_cols=0, clamp_rows=0, fmt=VIEW_BGR):
    """ms_reproject_aa: ms_reproject with a trilinear, mip-mapped lookup -- every job's view of every panorama, one launch"""
    reproject_aa_prepared(srcs, mips, levels, dsts, jobs, wrap_cols, clamp_rows, fmt)()
    return dsts


def warp_roi_lens(projection, K, R, lens, scale, src_w, src_h):
    ka, kp = _fa(K, 9); ra, rp = _fa(R, 9)
    r = Rect()
    _chk(load().ms_warp_roi_lens(projection, kp, rp, _lens_ptr(lens), C.c_float(scale), src_w, src_h, C.byref(r), _stream()))
    return r.tuple()


def warper_rays(projection, scale, R, uv, t=None):
    """ms_warper_rays (host only): absolute warper coordinates uv (n, 2) -> unit camera rays (n, 3) float64 of a camera with rotation R (3 x 3 float64)"""
    import numpy as np
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    Ra = np.ascontiguousarray(R, np.float64).reshape(9)
    out = np.empty((len(uv), 3), np.float64)
    tp = None
    if t is not None:
        ta, tp = _fa(t, 3)
    dp = C.POINTER(C.c_double)
    _chk(load().ms_warper_rays(projection, C.c_float(scale), tp, Ra.ctypes.data_as(dp), len(uv), uv.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(dp)))
    return out


def rig_refine_default_params(**kw):
    """ms_rig_refine_default_params; keyword arguments override fields"""
    p = RigRefineParams()
    _chk(load().ms_rig_refine_default_params(C.byref(p)))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def rig_matches(matches):
    """[(view_a, view_b, a (3,), b (3,)), ...] -> a RigMatch array"""
    arr = (RigMatch * max(1, len(matches)))()
    for k, (va, vb, a, b) in enumerate(matches):
        arr[k] = RigMatch(int(va), int(vb), (C.c_double * 3)(*[float(x) for x in a]), (C.c_double * 3)(*[float(x) for x in b]))
    return arr


def _rig_info(info):
    return {k: getattr(info, k) for k, _ in RigRefineInfo._fields_}


def rig_accumulate(R, matches, huber_rad=0.0):
    """ms_rig_accumulate: R (n, 3, 3) float64, matches as rig_matches takes them -> (cost, H (3n, 3n), g (3n,)) at R"""
    import numpy as np
    Ra = np.ascontiguousarray(R, np.float64)
    n = len(Ra)
    H = np.empty((3 * n, 3 * n), np.float64); g = np.empty(3 * n, np.float64)
    cost = C.c_double(0)
    dp = C.POINTER(C.c_double)
    _chk(load().ms_rig_accumulate(n, Ra.ctypes.data_as(dp), rig_matches(matches), len(matches), C.c_double(huber_rad), C.byref(cost), H.ctypes.data_as(dp),
                                  g.ctypes.data_as(dp), _stream()))
    return cost.value, H, g


def refine_rig_rotations(R, matches, params=None):
    """ms_refine_rig_rotations: R (n, 3, 3) float64, matches as rig_matches takes them -> (refined R (n, 3, 3) float64, info dict)"""
    import numpy as np
    Ra = np.ascontiguousarray(R, np.float64)
    n = len(Ra)
    out = np.empty((n, 3, 3), np.float64)
    prm = params if params is not None else rig_refine_default_params()
    info = RigRefineInfo()
    dp = C.POINTER(C.c_double)
    _chk(load().ms_refine_rig_rotations(n, Ra.ctypes.data_as(dp), rig_matches(matches), len(matches), C.byref(prm), out.ctypes.data_as(dp), C.byref(info), _stream()))
    return out, _rig_info(info)


def focals_from_homography(H):
    """ms_focals_from_homography (host only): H (3 x 3) between centred pixels -> (f0 or None, f1 or None), the focals of the source and the destination view"""
    import numpy as np
    Ha = np.ascontiguousarray(H, np.float64).reshape(9)
    f0, f1, ok0, ok1 = C.c_double(0), C.c_double(0), C.c_int(0), C.c_int(0)
    _chk(load().ms_focals_from_homography(Ha.ctypes.data_as(C.POINTER(C.c_double)), C.byref(f0), C.byref(f1), C.byref(ok0), C.byref(ok1)))
    return (f0.value if ok0.value else None), (f1.value if ok1.value else None)


def pair_homographies(pairs):
    """[(view_a, view_b, H (3 x 3), weight), ...] -> a PairHomography array"""
    arr = (PairHomography * max(1, len(pairs)))()
    for k, (va, vb, H, w) in enumerate(pairs):
        arr[k] = PairHomography(int(va), int(vb), (C.c_double * 9)(*[float(x) for row in H for x in row]), int(w))
    return arr


def estimate_rig(n_views, pairs, size, anchor=0):
    """ms_estimate_rig (host only): pairs as pair_homographies takes them, size = (width, height) of a source image -> (focals (n,), R (n, 3, 3) float64, info dict);
    info["status"] is 1 where no homography gave a focal and width + height stands in"""
    import numpy as np
    f = np.empty(n_views, np.float64); R = np.empty((n_views, 3, 3), np.float64)
    info = RigEstimateInfo()
    dp = C.POINTER(C.c_double)
    rc = _chk(load().ms_estimate_rig(n_views, pair_homographies(pairs), len(pairs), int(anchor), int(size[0]), int(size[1]), f.ctypes.data_as(dp), R.ctypes.data_as(dp),
                                     C.byref(info)))
    return f, R, {"status": rc, "focal_estimates": info.focal_estimates, "tree_parent": list(info.tree_parent)[:n_views]}


def rig_focal_default_params(**kw):
    """ms_rig_focal_default_params; keyword arguments override fields"""
    p = RigFocalParams()
    _chk(load().ms_rig_focal_default_params(C.byref(p)))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def rig_px_matches(matches):
    """[(view_a, view_b, a (2,), b (2,)), ...] -> a RigPxMatch array"""
    arr = (RigPxMatch * max(1, len(matches)))()
    for k, (va, vb, a, b) in enumerate(matches):
        arr[k] = RigPxMatch(int(va), int(vb), (C.c_double * 2)(float(a[0]), float(a[1])), (C.c_double * 2)(float(b[0]), float(b[1])))
    return arr


def _rig_focal_info(info):
    return {k: getattr(info, k) for k, _ in RigFocalInfo._fields_}


def rig_focal_accumulate(f, R, matches, huber_px=0.0):
    """ms_rig_focal_accumulate: f (n,), R (n, 3, 3) float64, matches as rig_px_matches takes them -> (cost, H (4n, 4n), g (4n,)) at these cameras"""
    import numpy as np
    fa = np.ascontiguousarray(f, np.float64); Ra = np.ascontiguousarray(R, np.float64)
    n = len(Ra)
    H = np.empty((4 * n, 4 * n), np.float64); g = np.empty(4 * n, np.float64)
    cost = C.c_double(0)
    dp = C.POINTER(C.c_double)
    _chk(load().ms_rig_focal_accumulate(n, fa.ctypes.data_as(dp), Ra.ctypes.data_as(dp), rig_px_matches(matches), len(matches), C.c_double(huber_px), C.byref(cost),
                                        H.ctypes.data_as(dp), g.ctypes.data_as(dp), _stream()))
    return cost.value, H, g


def refine_rig_cameras(f, R, matches, params=None):
    """ms_refine_rig_cameras: f (n,), R (n, 3, 3) float64, matches as rig_px_matches takes them -> (refined f (n,), refined R (n, 3, 3), info dict)"""
    import numpy as np
    fa = np.ascontiguousarray(f, np.float64); Ra = np.ascontiguousarray(R, np.float64)
    n = len(Ra)
    fo = np.empty(n, np.float64); out = np.empty((n, 3, 3), np.float64)
    prm = params if params is not None else rig_focal_default_params()
    info = RigFocalInfo()
    dp = C.POINTER(C.c_double)
    _chk(load().ms_refine_rig_cameras(n, fa.ctypes.data_as(dp), Ra.ctypes.data_as(dp), rig_px_matches(matches), len(matches), C.byref(prm), fo.ctypes.data_as(dp),
                                      out.ctypes.data_as(dp), C.byref(info), _stream()))
    return fo, out, _rig_focal_info(info)


def lens_array(lenses):
    """[Lens or None, ...] -> a Lens array, one a view; None is MS_LENS_NONE"""
    arr = (Lens * max(1, len(lenses)))()
    for v, l in enumerate(lenses):
        arr[v] = l if l is not None else Lens.make(LENS_NONE, (), 0.0)
    return arr


def rig_lens_accumulate(f, R, lenses, matches, huber_px=0.0):
    """ms_rig_lens_accumulate: rig_focal_accumulate with the views behind `lenses` (one Lens or None a view) -> (cost, H (4n, 4n), g (4n,)) at these cameras"""
    import numpy as np
    fa = np.ascontiguousarray(f, np.float64); Ra = np.ascontiguousarray(R, np.float64)
    n = len(Ra)
    assert len(lenses) == n
    H = np.empty((4 * n, 4 * n), np.float64); g = np.empty(4 * n, np.float64)
    cost = C.c_double(0)
    dp = C.POINTER(C.c_double)
    _chk(load().ms_rig_lens_accumulate(n, fa.ctypes.data_as(dp), Ra.ctypes.data_as(dp), lens_array(lenses), rig_px_matches(matches), len(matches), C.c_double(huber_px),
                                       C.byref(cost), H.ctypes.data_as(dp), g.ctypes.data_as(dp), _stream()))
    return cost.value, H, g


def refine_rig_cameras_lens(f, R, lenses, matches, params=None):
    """ms_refine_rig_cameras_lens: refine_rig_cameras with the views behind `lenses` (one Lens or None a view) -> (refined f (n,), refined R (n, 3, 3), info dict)"""
    import numpy as np
    fa = np.ascontiguousarray(f, np.float64); Ra = np.ascontiguousarray(R, np.float64)
    n = len(Ra)
    assert len(lenses) == n
    fo = np.empty(n, np.float64); out = np.empty((n, 3, 3), np.float64)
    prm = params if params is not None else rig_focal_default_params()
    info = RigFocalInfo()
    dp = C.POINTER(C.c_double)
    _chk(load().ms_refine_rig_cameras_lens(n, fa.ctypes.data_as(dp), Ra.ctypes.data_as(dp), lens_array(lenses), rig_px_matches(matches), len(matches), C.byref(prm),
                                           fo.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(info), _stream()))
    return fo, out, _rig_focal_info(info)


def rig_coeff_default_params(**kw):
    """ms_rig_coeff_default_params; keyword arguments override fields (free_coeffs: bit b frees lens.k[b])"""
    p = RigCoeffParams()
    _chk(load().ms_rig_coeff_default_params(C.byref(p)))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _rig_coeff_info(info):
    return {k: getattr(info, k) for k, _ in RigCoeffInfo._fields_}


def rig_coeff_accumulate(f, R, lens, free_coeffs, matches, huber_px=0.0):
    """ms_rig_coeff_accumulate: rig_lens_accumulate with the one Lens on every view and the coefficient rows of the free_coeffs mask last ->
    (cost, H (4n + G, 4n + G), g (4n + G,)) at these cameras and this lens"""
    import numpy as np
    fa = np.ascontiguousarray(f, np.float64); Ra = np.ascontiguousarray(R, np.float64)
    n = len(Ra)
    d = 4 * n + bin(int(free_coeffs) & 0xffffffff).count("1")
    H = np.empty((d, d), np.float64); g = np.empty(d, np.float64)
    cost = C.c_double(0)
    dp = C.POINTER(C.c_double)
    _chk(load().ms_rig_coeff_accumulate(n, fa.ctypes.data_as(dp), Ra.ctypes.data_as(dp), C.byref(lens) if lens is not None else None, C.c_uint(free_coeffs),
                                        rig_px_matches(matches), len(matches), C.c_double(huber_px), C.byref(cost), H.ctypes.data_as(dp), g.ctypes.data_as(dp), _stream()))
    return cost.value, H, g


def refine_rig_coeffs(f, R, lens, matches, params=None):
    """ms_refine_rig_coeffs: refine_rig_cameras_lens with one Lens shared by all views and params.free_coeffs of its coefficients free ->
    (refined f (n,), refined R (n, 3, 3), refined Lens, info dict)"""
    import numpy as np
    fa = np.ascontiguousarray(f, np.float64); Ra = np.ascontiguousarray(R, np.float64)
    n = len(Ra)
    fo = np.empty(n, np.float64); out = np.empty((n, 3, 3), np.float64)
    prm = params if params is not None else rig_coeff_default_params()
    info = RigCoeffInfo()
    lens_out = Lens()
    dp = C.POINTER(C.c_double)
    _chk(load().ms_refine_rig_coeffs(n, fa.ctypes.data_as(dp), Ra.ctypes.data_as(dp), C.byref(lens) if lens is not None else None, rig_px_matches(matches), len(matches),
                                     C.byref(prm), fo.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(lens_out), C.byref(info), _stream()))
    return fo, out, lens_out, _rig_coeff_info(info)


def rig_pp_default_params(**kw):
    """ms_rig_pp_default_params; keyword arguments override fields (pp_prior: the weight of the prior on the centres, 0 = none)"""
    p = RigPpParams()
    _chk(load().ms_rig_pp_default_params(C.byref(p)))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _rig_pp_info(info):
    return {k: getattr(info, k) for k, _ in RigPpInfo._fields_}


def rig_pp_accumulate(f, R, pp, lenses, matches, huber_px=0.0):
    """ms_rig_pp_accumulate: rig_lens_accumulate with the principal-point offsets pp (n, 2) among the unknowns; lenses: one Lens or None a view, or None for a rig
    without lenses -> (cost, H (6n, 6n), g (6n,)) at these cameras, view v at rows 6v .. 6v + 5 in the order (rotation, log focal, ox, oy)"""
    import numpy as np
    fa = np.ascontiguousarray(f, np.float64); Ra = np.ascontiguousarray(R, np.float64); pa = np.ascontiguousarray(pp, np.float64)
    n = len(Ra)
    assert pa.shape == (n, 2) and (lenses is None or len(lenses) == n)
    H = np.empty((6 * n, 6 * n), np.float64); g = np.empty(6 * n, np.float64)
    cost = C.c_double(0)
    dp = C.POINTER(C.c_double)
    _chk(load().ms_rig_pp_accumulate(n, fa.ctypes.data_as(dp), Ra.ctypes.data_as(dp), pa.ctypes.data_as(dp), lens_array(lenses) if lenses is not None else None,
                                     rig_px_matches(matches), len(matches), C.c_double(huber_px), C.byref(cost), H.ctypes.data_as(dp), g.ctypes.data_as(dp), _stream()))
    return cost.value, H, g


def refine_rig_pp(f, R, pp, lenses, matches, params=None):
    """ms_refine_rig_pp: refine_rig_cameras_lens with every view's principal-point offset free; pp (n, 2) float64, lenses as rig_pp_accumulate takes them ->
    (refined f (n,), refined R (n, 3, 3), refined pp (n, 2), info dict)"""
    import numpy as np
    fa = np.ascontiguousarray(f, np.float64); Ra = np.ascontiguousarray(R, np.float64); pa = np.ascontiguousarray(pp, np.float64)
    n = len(Ra)
    assert pa.shape == (n, 2) and (lenses is None or len(lenses) == n)
    fo = np.empty(n, np.float64); out = np.empty((n, 3, 3), np.float64); po = np.empty((n, 2), np.float64)
    prm = params if params is not None else rig_pp_default_params()
    info = RigPpInfo()
    dp = C.POINTER(C.c_double)
    _chk(load().ms_refine_rig_pp(n, fa.ctypes.data_as(dp), Ra.ctypes.data_as(dp), pa.ctypes.data_as(dp), lens_array(lenses) if lenses is not None else None,
                                 rig_px_matches(matches), len(matches), C.byref(prm), fo.ctypes.data_as(dp), out.ctypes.data_as(dp), po.ctypes.data_as(dp), C.byref(info),
                                 _stream()))
    return fo, out, po, _rig_pp_info(info)


def pair_match_default_params(**kw):
    """ms_pair_match_default_params; keyword arguments override fields (pair_mask: see match_pairs)"""
    p = PairMatchParams()
    _chk(load().ms_pair_match_default_params(C.byref(p)))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def view_features(features):
    """[(keypoints (n, >= 2) float32 numpy -- x, y first, ms.orb_detect_and_compute's rows as they are --, descriptors torch uint8 (rows >= n, bytes) on the device or
    None for an empty view, (width, height)), ...] -> (a ViewFeatures array, the objects it borrows from: keep them alive as long as the array)"""
    import numpy as np
    arr = (ViewFeatures * max(1, len(features)))()
    keep = []
    for v, (kp, desc, size) in enumerate(features):
        kp = np.ascontiguousarray(kp, np.float32)
        if kp.ndim != 2:
            kp = kp.reshape(-1, 2)
        keep.append((kp, desc))
        arr[v] = ViewFeatures(Image() if desc is None else img(desc), kp.ctypes.data_as(C.POINTER(C.c_float)), max(2, kp.shape[1]), kp.shape[0], int(size[0]), int(size[1]))
    return arr, keep


def match_pairs(features, matches_cap=None, params=None, pair_mask=None, **kw):
    """ms_match_pairs (detail::BestOf2NearestMatcher over every candidate pair): features as view_features takes them; keyword arguments override fields of
    ms_pair_match_params (match_conf, num_matches_thresh1, num_matches_thresh2, range_width, ransac_*); pair_mask: (n, n) uint8 or None.
    Returns a list with one dict per candidate pair: view_a, view_b, first, count, n_forward, num_inliers, have_H, H (3 x 3 float64, None without a model),
    confidence, and matches, a (count, 4) int32 array of (query in view_a, train in view_b, distance, inlier)."""
    import numpy as np
    n = len(features)
    prm = params if params is not None else pair_match_default_params(**kw)
    mask = None
    if pair_mask is not None:
        mask = np.ascontiguousarray(pair_mask, np.uint8)
        assert mask.shape == (n, n)
        prm.pair_mask = mask.ctypes.data_as(C.POINTER(C.c_ubyte))
    views, keep = view_features(features)
    pairs_cap = max(1, n * (n - 1) // 2)
    if matches_cap is None:         # a pair's list never holds more than one match per row of either view
        matches_cap = sum(max(views[i].n_keypoints, 0) for i in range(n)) * max(n - 1, 1)
    pairs = (PairMatches * pairs_cap)()
    out = np.zeros((max(1, matches_cap), 4), np.int32)
    n_pairs, n_matches = C.c_int(0), C.c_int(0)
    _chk(load().ms_match_pairs(n, views, C.byref(prm), pairs, pairs_cap, C.byref(n_pairs), out.ctypes.data_as(C.POINTER(FeatureMatch)), int(matches_cap), C.byref(n_matches),
                               _stream()))
    del keep, mask
    res = []
    for k in range(n_pairs.value):
        p = pairs[k]
        res.append({"view_a": p.view_a, "view_b": p.view_b, "first": p.first, "count": p.count, "n_forward": p.n_forward, "num_inliers": p.num_inliers, "have_H": p.have_H,
                    "H": np.array(p.H[:], np.float64).reshape(3, 3) if p.have_H else None, "confidence": p.confidence, "matches": out[p.first:p.first + p.count].copy()})
    return res


def list_match_default_params(**kw):
    """ms_list_match_default_params; keyword arguments override fields"""
    p = ListMatchParams()
    _chk(load().ms_list_match_default_params(C.byref(p)))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def match_lists(sets, problems, matches_cap=None, params=None, **kw):
    """ms_match_lists (featurefinder::matchFeatures / matchFeaturesTemporal over a list of directed problems): sets as view_features takes them, problems a list of
    (query_set, train_set); keyword arguments override fields of ms_list_match_params (ratio, find_homography, ransac_*).  Returns one dict per problem, as match_pairs
    does: view_a (the query set), view_b (the train set), first, count, n_forward, num_inliers, have_H, H (3 x 3 float64, None without a model), confidence, and
    matches, a (count, 4) int32 array of (query, train, distance, inlier)."""
    import numpy as np
    prm = params if params is not None else list_match_default_params(**kw)
    table, keep = view_features(sets)
    k = len(problems)
    probs = (MatchProblem * max(1, k))(*[MatchProblem(int(q), int(t)) for q, t in problems])
    if matches_cap is None:         # a problem's list never holds more than one match per query row
        matches_cap = sum(max(table[q].n_keypoints, 0) for q, _ in problems if 0 <= q < len(sets))
    recs = (PairMatches * max(1, k))()
    out = np.zeros((max(1, matches_cap), 4), np.int32)
    n_matches = C.c_int(0)
    _chk(load().ms_match_lists(len(sets), table, k, probs, C.byref(prm), recs, out.ctypes.data_as(C.POINTER(FeatureMatch)), int(matches_cap), C.byref(n_matches),
                               _stream() if k else None))      # (an empty list needs no device)
    del keep
    return [{"view_a": p.view_a, "view_b": p.view_b, "first": p.first, "count": p.count, "n_forward": p.n_forward, "num_inliers": p.num_inliers, "have_H": p.have_H,
             "H": np.array(p.H[:], np.float64).reshape(3, 3) if p.have_H else None, "confidence": p.confidence, "matches": out[p.first:p.first + p.count].copy()}
            for p in recs[:k]]


def pair_matches(pairs):
    """match_pairs' records (view_a, view_b, confidence are read) -> a PairMatches array, for biggest_component"""
    arr = (PairMatches * max(1, len(pairs)))()
    for k, p in enumerate(pairs):
        arr[k].view_a, arr[k].view_b, arr[k].confidence = int(p["view_a"]), int(p["view_b"]), float(p["confidence"])
    return arr


def pairs_for_estimate_rig(pairs):
    """match_pairs' records with a homography -> what estimate_rig takes: (view_a, view_b, H, weight = num_inliers)"""
    return [(p["view_a"], p["view_b"], p["H"], p["num_inliers"]) for p in pairs if p["have_H"]]


def biggest_component(n_views, pairs, conf_threshold=1.0):
    """ms_biggest_component (leaveBiggestComponent; host only): pairs as match_pairs returns them -> the ascending views of the largest component over the pairs
    with confidence >= conf_threshold (ties: the component with the lowest view)"""
    keep = (C.c_int * max(1, n_views))()
    n_keep = C.c_int(0)
    _chk(load().ms_biggest_component(int(n_views), pair_matches(pairs) if len(pairs) else None, len(pairs), C.c_double(conf_threshold), keep, C.byref(n_keep)))
    return list(keep[:n_keep.value])


def wave_correct(R, kind=WAVE_HORIZ):
    """ms_wave_correct (waveCorrect in double; host only): R (n, 3, 3) camera to rig -> (corrected R (n, 3, 3) float64, status: 1 where the input came back unchanged)"""
    import numpy as np
    Ra = np.ascontiguousarray(R, np.float64)
    out = np.empty_like(Ra)
    dp = C.POINTER(C.c_double)
    rc = _chk(load().ms_wave_correct(len(Ra), Ra.ctypes.data_as(dp), int(kind), out.ctypes.data_as(dp)))
    return out, rc


def nv12_to_bgr(src, dst=None):
    if dst is None:
        dst = _new((src.shape[0] * 2 // 3, src.shape[1], 3), _torch().uint8)
    _chk(load().ms_nv12_to_bgr(C.byref(img(src)), C.byref(img(dst)), _stream()))
    return dst


def nv12_to_bgr_batch(srcs, dsts=None):
    """cvtColor(YUV2BGR_NV12) of n cameras of one geometry in one launch; returns the list of BGR tensors."""
    if dsts is None:
        dsts = [_new((t.shape[0] * 2 // 3, t.shape[1], 3), _torch().uint8) for t in srcs]
    n = len(srcs)
    a = (Image * n)(*[img(t) for t in srcs]); b = (Image * n)(*[img(t) for t in dsts])
    _chk(load().ms_nv12_to_bgr_batch(a, b, n, _stream()))
    return dsts


def nv12_to_bgr_batch_prepared(srcs, dsts):
    """ms_nv12_to_bgr_batch with the descriptors marshalled once; returns a callable(stream_handle=None) (timed loops: building 192 ms_image per call costs
    more host time than the three launches take on the GPU)."""
    n = len(srcs)
    a = (Image * n)(*[img(t) for t in srcs]); b = (Image * n)(*[img(t) for t in dsts])
    fn = load().ms_nv12_to_bgr_batch

    def run(stream=None):
        _chk(fn(a, b, n, stream if stream is not None else _stream()))
    run.keep = (srcs, dsts)
    return run


def bgr_to_i420(src, dst=None):
    if dst is None:
        dst = _new((src.shape[0] * 3 // 2, src.shape[1]), _torch().uint8)
    _chk(load().ms_bgr_to_i420(C.byref(img(src)), C.byref(img(dst)), _stream()))
    return dst


def consume_i420(pano8u, out_size=(4096, 2048), keep_aspect_ratio=True):
    """consume()'s resize + black bars + BGR2YUV_I420 in one pass (timed.cpp:251-316).  Returns (I420 tensor (out_h * 3 / 2, out_w), image_height)."""
    ow, oh = out_size
    dst = _new((oh * 3 // 2, ow), _torch().uint8)
    ih = C.c_int(0)
    _chk(load().ms_consume_i420(C.byref(img(pano8u)), C.byref(img(dst)), ow, oh, 1 if keep_aspect_ratio else 0, C.byref(ih), _stream()))
    return dst, ih.value


def bgr_to_gray(src):
    dst = _new(tuple(src.shape[:2]), _torch().uint8)
    _chk(load().ms_bgr_to_gray(C.byref(img(src)), C.byref(img(dst)), _stream()))
    return dst


def feature_inputs_batch(views, bands=None, gray=True, masks=None):
    """ms_feature_inputs_batch: the grey images (gray=True) and / or the feature masks (masks defaults to `bands is not None`) of every 8UC3 view in one launch; bands:
    one (a_x0, a_width, b_x0, b_width) per view.  Returns (list of grey tensors or None, list of mask tensors or None)."""
    import numpy as np
    n = len(views)
    if masks is None:
        masks = bands is not None
    u8 = _torch().uint8
    g = [_new(tuple(t.shape[:2]), u8) for t in views] if gray else None
    m = [_new(tuple(t.shape[:2]), u8) for t in views] if masks else None
    b = None if bands is None else np.ascontiguousarray(bands, np.int32).reshape(n, 4)
    arr = lambda ts: (Image * max(n, 1))(*[img(t) for t in ts])
    _chk(load().ms_feature_inputs_batch(n, arr(views), None if b is None else b.ctypes.data_as(C.POINTER(C.c_int)), arr(g) if gray else None, arr(m) if masks else None,
                                        _stream()))
    return g, m


def resize_linear_batch_prepared(srcs, dsts, fx=0.0, fy=0.0):
    """cuda::resize of every srcs[i] into dsts[i] (8UC3, one geometry) in one launch; returns a callable(stream_handle=None) with the descriptors
    marshalled once (the per-frame compose-scale resize of stitch_online, timed.cpp:75-85, inside a timed loop)."""
    n = len(srcs)
    a = (Image * n)(*[img(t) for t in srcs]); b = (Image * n)(*[img(t) for t in dsts])
    fn = load().ms_resize_linear_batch
    cfx, cfy = C.c_double(fx), C.c_double(fy)

    def run(stream=None):
        _chk(fn(a, b, n, cfx, cfy, stream if stream is not None else _stream()))
    run.keep = (srcs, dsts)
    return run


def _nv12_resize_dsts(srcs, dsize, fx, fy):
    import numpy as np
    rows, cols = srcs[0].shape[0] * 2 // 3, srcs[0].shape[1]
    if dsize is None:
        dsize = (int(np.rint(cols * fx)), int(np.rint(rows * fy)))
    else:
        fx = fy = 0.0
    return [_new((dsize[1], dsize[0], 3), _torch().uint8) for _ in srcs], fx, fy


def nv12_resize_linear_batch(srcs, dsize=None, fx=0.0, fy=0.0):
    """ms_nv12_resize_linear_batch: cvtColor(YUV2BGR_NV12) + cuda::resize of n NV12 frames ((H * 3 / 2) x W uint8 tensors, one geometry) in one pass; returns
    the list of resized BGR tensors (= resize_linear_batch(nv12_to_bgr_batch(srcs), ...), bit for bit)."""
    dsts, fx, fy = _nv12_resize_dsts(srcs, dsize, fx, fy)
    nv12_resize_linear_batch_prepared(srcs, dsts, fx, fy)()
    return dsts


def nv12_resize_linear_batch_prepared(srcs, dsts, fx=0.0, fy=0.0):
    """ms_nv12_resize_linear_batch with the descriptors marshalled once; returns a callable(stream_handle=None) for timed loops."""
    n = len(srcs)
    a = (Image * n)(*[img(t) for t in srcs]); b = (Image * n)(*[img(t) for t in dsts])
    fn = load().ms_nv12_resize_linear_batch
    cfx, cfy = C.c_double(fx), C.c_double(fy)

    def run(stream=None):
        _chk(fn(a, b, n, cfx, cfy, stream if stream is not None else _stream()))
    run.keep = (srcs, dsts)
    return run


def bgr_to_i420_batch_prepared(srcs, dsts):
    """One launch converting every srcs[i] (8UC3, same geometry) into dsts[i] (contiguous I420); returns a callable(stream_handle=None)
    with the descriptors marshalled once."""
    n = len(srcs)
    a = (Image * n)(*[img(t) for t in srcs]); b = (Image * n)(*[img(t) for t in dsts])
    fn = load().ms_bgr_to_i420_batch

    def run(stream=None):
        _chk(fn(a, b, n, stream if stream is not None else _stream()))
    run.keep = (srcs, dsts)
    return run


def custom_resize(src, tx, ty):
    dst = _new((ty, tx), src.dtype)
    _chk(load().ms_custom_resize_32f(C.byref(img(src)), C.byref(img(dst)), _stream()))
    return dst


def warp_roi(projection, K, R, scale, src_w, src_h):
    ka, kp = _fa(K, 9); ra, rp = _fa(R, 9)
    r = Rect()
    _chk(load().ms_warp_roi(projection, kp, rp, C.c_float(scale), src_w, src_h, C.byref(r)))
    return r.tuple()


def result_roi(rois):
    arr = (Rect * len(rois))(*[Rect(*r) for r in rois])
    r = Rect()
    _chk(load().ms_result_roi(len(rois), arr, C.byref(r)))
    return r.tuple()


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int), ("edge_threshold", C.c_int), ("first_level", C.c_int),
                ("patch_size", C.c_int), ("fast_threshold", C.c_int)]


def orb_detect_and_compute(gray, mask=None, nfeatures=2500, scale_factor=1.2, nlevels=8, fast_threshold=20, edge_threshold=None):
    """cuda::ORB::create(nfeatures, scaleFactor, nlevels)->detectAndCompute (featurefinder.cpp:15-40): gray / mask torch uint8 (H, W) on the device.
    Returns (keypoints (n, 6) float32 numpy: x, y, response, angle, octave, size; descriptors (n, 32) uint8 torch tensor on the device), in the order
    ms_stitch.h defines (levels in turn; raster order, then the stable culls).  The batch of one: orb_detect_and_compute_batch([gray], [mask])[0]."""
    import numpy as np
    import torch
    prm = OrbParams()
    _chk(load().ms_orb_default_params(C.byref(prm)))
    prm.nfeatures, prm.scale_factor, prm.nlevels, prm.fast_threshold = nfeatures, scale_factor, nlevels, fast_threshold
    if edge_threshold is not None:
        prm.edge_threshold = edge_threshold
    cap = nfeatures + nlevels // 2      # the rounded per-level budgets can add up to (nlevels - 1) / 2 more than nfeatures (ms_stitch.h)
    kp = np.zeros((cap, 6), np.float32)
    desc = torch.zeros((cap, 32), dtype=torch.uint8, device=gray.device)
    n = C.c_int(0)
    di = img(desc)
    _chk(load().ms_orb_detect_and_compute(C.byref(img(gray)), None if mask is None else C.byref(img(mask)), C.byref(prm),
                                          kp.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(di), C.byref(n), _stream()))
    return kp[:n.value].copy(), desc[:n.value]


def orb_params(nfeatures=2500, scale_factor=1.2, nlevels=8, fast_threshold=20, edge_threshold=None):
    """ms_orb_default_params with orb_detect_and_compute's keyword arguments applied"""
    prm = OrbParams()
    _chk(load().ms_orb_default_params(C.byref(prm)))
    prm.nfeatures, prm.scale_factor, prm.nlevels, prm.fast_threshold = nfeatures, scale_factor, nlevels, fast_threshold
    if edge_threshold is not None:
        prm.edge_threshold = edge_threshold
    return prm


def orb_detect_and_compute_batch(grays, masks=None, **orb_kw):
    """ms_orb_detect_and_compute_batch: ORB for every view in one device pass (orb_detect_and_compute is this with one view).  grays: torch uint8 (H, W) tensors on the device, of any sizes;
    masks: None, or one entry per view (a tensor or None); keyword arguments as orb_detect_and_compute takes them, one set for the batch.
    Returns [(keypoints (n, 6) float32 numpy, descriptors (n, 32) uint8 torch tensor on the device, (width, height)), ...]: per view what orb_detect_and_compute
    returns, bit for bit and in its order, and the view's size behind it -- the list is what match_pairs / view_features take as it is."""
    import numpy as np
    import torch
    prm = orb_params(**orb_kw)
    n = len(grays)
    cap = prm.nfeatures + prm.nlevels // 2      # (see orb_detect_and_compute)
    kp = np.zeros((max(n, 1), cap, 6), np.float32)
    descs = [torch.zeros((cap, 32), dtype=torch.uint8, device=g.device) for g in grays]
    gi = (Image * max(n, 1))(*[img(g) for g in grays])
    di = (Image * max(n, 1))(*[img(d) for d in descs])
    mi = None
    if masks is not None:
        assert len(masks) == n
        mi = (Image * max(n, 1))(*[Image() if m is None else img(m) for m in masks])
    cnt = (C.c_int * max(n, 1))()
    _chk(load().ms_orb_detect_and_compute_batch(n, gi, mi, C.byref(prm), kp.ctypes.data_as(C.POINTER(C.c_float)), cap, di, cnt, _stream()))
    return [(kp[v, :cnt[v]].copy(), descs[v][:cnt[v]], (int(grays[v].shape[1]), int(grays[v].shape[0]))) for v in range(n)]


def find_homography_ransac(src, dst, reproj_threshold=3.0, max_iters=2000, confidence=0.995):
    """cv::findHomography(src, dst, mask, RANSAC): src / dst (n, 2) float32.  Returns (H 3x3 float64 or None, inlier mask uint8 (n,))."""
    import numpy as np
    src = np.ascontiguousarray(src, np.float32); dst = np.ascontiguousarray(dst, np.float32)
    n = len(src)
    H = np.zeros(9, np.float64)
    m = np.zeros(max(n, 1), np.uint8)
    cnt = C.c_int(0)
    rc = load().ms_find_homography_ransac(src.ctypes.data_as(C.POINTER(C.c_float)), dst.ctypes.data_as(C.POINTER(C.c_float)), n, C.c_double(reproj_threshold),
                                          max_iters, C.c_double(confidence), H.ctypes.data_as(C.POINTER(C.c_double)), m.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          C.byref(cnt), _stream())
    if rc < 0:
        _chk(rc)
    return (None if rc == 1 else H.reshape(3, 3)), m[:n]


def find_homography_ransac_batch(problems, reproj_threshold=3.0, max_iters=2000, confidence=0.995):
    """ms_find_homography_ransac_batch: problems is a list of (src, dst) float32 (n, 2) arrays, every one solved as find_homography_ransac solves it alone, all of
    them in one device pass.  Returns a list of (H 3x3 float64 or None, inlier mask uint8 (n,))."""
    import numpy as np
    srcs = [np.ascontiguousarray(s, np.float32).reshape(-1, 2) for s, _ in problems]
    dsts = [np.ascontiguousarray(d, np.float32).reshape(-1, 2) for _, d in problems]
    assert all(len(s) == len(d) for s, d in zip(srcs, dsts)), "a problem's src and dst differ in length"
    k = len(problems)
    off = np.zeros(k + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in srcs])
    total = int(off[-1])
    src = np.concatenate(srcs + [np.zeros((1, 2), np.float32)]); dst = np.concatenate(dsts + [np.zeros((1, 2), np.float32)])
    H = np.zeros((max(k, 1), 9), np.float64)
    m = np.zeros(total + 1, np.uint8)
    cnt = np.zeros(max(k, 1), np.int32); status = np.ones(max(k, 1), np.int32)
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    _chk(load().ms_find_homography_ransac_batch(k, off.ctypes.data_as(ip), src.ctypes.data_as(fp), dst.ctypes.data_as(fp), C.c_double(reproj_threshold), int(max_iters),
                                                C.c_double(confidence), H.ctypes.data_as(C.POINTER(C.c_double)), m.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                cnt.ctypes.data_as(ip), status.ctypes.data_as(ip), _stream() if k else None))      # (an empty batch needs no device)
    return [(None if status[p] else H[p].reshape(3, 3).copy(), m[off[p]:off[p + 1]].copy()) for p in range(k)]


# ------------------------------------------------------------------ compositor context

def knn_match_hamming2(query, train):
    """BFMatcher(NORM_HAMMING).knnMatch(query, train, k=2): (train_idx, distance) int32 arrays of shape (nq, 2)."""
    import numpy as np
    nq = query.shape[0]
    idx = np.empty((nq, 2), np.int32)
    dist = np.empty((nq, 2), np.int32)
    ip = C.POINTER(C.c_int)
    _chk(load().ms_knn_match_hamming2(C.byref(img(query)), C.byref(img(train)), idx.ctypes.data_as(ip), dist.ctypes.data_as(ip), _stream()))
    return idx, dist


def mesh_default_params(**kw):
    """defs.h values (10 x 10 mesh, ALPHAS, GLOBAL_DIST, wrapAround); keyword arguments override fields."""
    p = MeshParams()
    _chk(load().ms_mesh_default_params(C.byref(p)))
    for k, v in kw.items():
        if k == "alphas":
            p.alphas = (C.c_float * 4)(*v)
        else:
            assert hasattr(p, k), k
            setattr(p, k, v)
    return p


def mesh_saliency(view, mesh_cols, mesh_rows):
    import numpy as np
    out = np.empty((mesh_rows, mesh_cols, 8), np.float32)
    _chk(load().ms_mesh_saliency(C.byref(img(view)), mesh_cols, mesh_rows, out.ctypes.data_as(C.POINTER(C.c_float)), _stream()))
    return out


def mesh_triangle_masks(cell_w, cell_h):
    """The 8 fillConvexPoly triangle masks of a cell_w x cell_h mesh cell, (8, cell_h, cell_w) uint8, and their set-pixel counts."""
    import numpy as np
    out = np.empty((8, cell_h, cell_w), np.uint8)
    cnt = (C.c_uint * 8)()
    _chk(load().ms_mesh_triangle_masks(int(cell_w), int(cell_h), out.ctypes.data_as(C.POINTER(C.c_ubyte)), cnt, _stream()))
    return out, list(cnt)


def _match_array(lists):
    flat = [m for l in lists for m in l]
    arr = (MeshMatch * max(1, len(flat)))()
    for k, m in enumerate(flat):
        arr[k] = MeshMatch(float(m[0]), float(m[1]), float(m[2]), float(m[3]), int(m[4]) if len(m) > 4 else 0)
    return arr, (C.c_int * len(lists))(*[len(l) for l in lists])


def create_mesh(views, matches, params, temporal=None):
    """MeshWarper::createMesh after feature matching (ms_create_mesh).  views: warped 8UC3 device tensors; matches[v]: list of
    (x1, y1, x2, y2, dst); temporal[v]: list of (x1, y1, x2, y2).  Returns mesh_x, mesh_y (n, N, M) float32 host arrays and the solver info."""
    import numpy as np
    n = len(views)
    ims = (Image * n)(*[img(v) for v in views])
    marr, mcnt = _match_array(matches)
    tarr = tcnt = None
    if temporal is not None:
        tarr, tcnt = _match_array(temporal)
    mx = np.empty((n, params.mesh_rows, params.mesh_cols), np.float32)
    my = np.empty_like(mx)
    info = MeshInfo()
    fp = C.POINTER(C.c_float)
    _chk(load().ms_create_mesh(n, ims, marr, mcnt, tarr, tcnt, C.byref(params), mx.ctypes.data_as(fp), my.ctypes.data_as(fp),
                               C.byref(info), _stream()))
    return mx, my, {k: getattr(info, k) for k, _ in MeshInfo._fields_}


def calibrate_cameras(num_views, w, h, hfov_deg=90.0, work_megapix=0.6, seam_megapix=0.01, compose_megapix=1.4):
    """ms_calibrate_cameras: calibrateCameras + stitch_calib's scale bookkeeping (APP/calibration.cpp:28-68, 101-116, 147-181, 269-288).
    Returns a dict: the scales, and per view K_compose / K_seam / R as fp32 3x3 arrays."""
    import numpy as np
    q = RigParams(num_views, w, h, hfov_deg, work_megapix, seam_megapix, compose_megapix)
    r = Rig()
    _chk(load().ms_calibrate_cameras(C.byref(q), C.byref(r)))
    out = {k: getattr(r, k) for k in ("work_scale", "seam_scale", "seam_work_aspect", "compose_scale", "compose_work_aspect", "warped_image_scale",
                                      "seam_warp_scale", "compose_warp_scale", "resize_input", "compose_width", "compose_height")}
    for k in ("K_compose", "K_seam", "R"):
        out[k] = [np.array(list(getattr(r, k)[i]), np.float32).reshape(3, 3) for i in range(num_views)]
    return out


def num_bands_rule(pano_w, pano_h, blend_strength=5.0):
    bw, nb = C.c_float(), C.c_int()
    _chk(load().ms_num_bands_rule(pano_w, pano_h, C.c_float(blend_strength), C.byref(bw), C.byref(nb)))
    return bw.value, nb.value


class Compositor:
    """stitch_calib tables once (build_maps / build_masks / init_blender), then stitch() per frame batch."""

    def __init__(self, num_views, src_size, projection, warp_scale, num_bands=5, enable_cpw=False,
                 out_size=(0, 0), max_frames=1, simple_kernels=False, lds_stage=None, shards=1, shard_index=0, cv_remap=False,
                 col_shards=1, col_shard_index=0, update_mask_margin=0, raster_order=False):
        cfg = Config(C.sizeof(Config), num_views, src_size[0], src_size[1], projection, warp_scale, num_bands, int(enable_cpw),
                     out_size[0], out_size[1], max_frames)
        cfg.debug_simple_kernels = 1 if simple_kernels else 0   # debug: force the one-pixel-per-lane reference kernels
        cfg.warp_lds_stage = 0 if lds_stage is None else (1 if lds_stage else 2)   # True: warp source tiles staged in LDS by LDS-DMA (opt-in, measured slower); False forces the direct gathers even under MS_WARP_ASYNC=1
        cfg.raster_tile_order = 1 if raster_order else 0   # work lists in raster order instead of the XCD-aware order
        cfg.view_shards = shards; cfg.view_shard_index = shard_index   # view sharding
        cfg.col_shards = col_shards; cfg.col_shard_index = col_shard_index   # pano-column sharding
        cfg.self_check = 1 if os.environ.get("MS_CHECK_DIVIDE", "0") not in ("", "0") else 0   # (this binding is test / bench infrastructure: the LIBRARY reads no environment; tests/conftest.py sets the variable)
        cfg.update_mask_margin = update_mask_margin   # > 0: ms_update_mask is enqueue-only (double-buffered tables, work lists planned with this margin)
        cfg.cpu_flavour_remap = 1 if cv_remap else 0   # cv::remap's CPU arithmetic for the projection warp (needs simple_kernels, no CPW)
        self._ctx = C.c_void_p()
        _chk(load().ms_create(C.byref(cfg), C.byref(self._ctx)))
        self.cfg = cfg
        self.n = num_views

    def save_tables(self):
        """ms_save_tables: the calibration of this (ready) context as bytes"""
        n = C.c_size_t(0)
        _chk(load().ms_save_tables(self._ctx, None, C.c_size_t(0), C.byref(n)))
        buf = (C.c_uint8 * n.value)()
        _chk(load().ms_save_tables(self._ctx, buf, C.c_size_t(n.value), C.byref(n)))
        return bytes(buf)

    @classmethod
    def from_tables(cls, blob):
        """ms_load_tables: a ready context rebuilt from save_tables() bytes (no ms_init_blender call needed)"""
        self = cls.__new__(cls)
        self._ctx = C.c_void_p()
        b = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        _chk(load().ms_load_tables(b, C.c_size_t(len(blob)), C.byref(self._ctx), _stream()))
        self.cfg = Config.from_buffer_copy(blob[48:48 + C.sizeof(Config)])      # TablesHeader: 48 bytes in front of the ms_config
        import struct
        self.n = struct.unpack_from("<i", blob, 16)[0]      # TablesHeader::n_views
        return self

    def close(self):
        if self._ctx:
            load().ms_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_camera(self, view, K, R):
        ka, kp = _fa(K, 9); ra, rp = _fa(R, 9)
        _chk(load().ms_set_camera(self._ctx, view, kp, rp))

    def set_lens(self, view, lens):
        """ms_set_lens: a Lens, or None to clear the view's"""
        _chk(load().ms_set_lens(self._ctx, view, _lens_ptr(lens)))

    def get_lens(self, view):
        lens = Lens()
        _chk(load().ms_get_lens(self._ctx, view, C.byref(lens)))
        return lens

    def set_gain(self, view, gain):
        _chk(load().ms_set_gain(self._ctx, view, C.c_double(gain)))

    def refine_rig(self, matches, params=None):
        """ms_refine_rig: matches[v] = list of (x1, y1, x2, y2, dst) in projection-warped view pixels (create_mesh's layout) -> (R (n, 3, 3) float32 for
        set_camera, info dict).  Nothing is applied to the context."""
        import numpy as np
        marr, mcnt = _match_array(matches)
        prm = params if params is not None else rig_refine_default_params()
        out = np.empty((self.n, 3, 3), np.float32)
        info = RigRefineInfo()
        _chk(load().ms_refine_rig(self._ctx, marr, mcnt, C.byref(prm), out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(info), _stream()))
        return out, _rig_info(info)

    def refine_rig_focals(self, matches, params=None):
        """ms_refine_rig_focals: matches as refine_rig takes them -> (focals (n,) float64, R (n, 3, 3) float32, info dict).  Nothing is applied to the context."""
        import numpy as np
        marr, mcnt = _match_array(matches)
        prm = params if params is not None else rig_focal_default_params()
        f = np.empty(self.n, np.float64); out = np.empty((self.n, 3, 3), np.float32)
        info = RigFocalInfo()
        _chk(load().ms_refine_rig_focals(self._ctx, marr, mcnt, C.byref(prm), f.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_float)),
                                         C.byref(info), _stream()))
        return f, out, _rig_focal_info(info)

    def refine_rig_focals_lens(self, matches, params=None):
        """ms_refine_rig_focals_lens: refine_rig_focals for lens contexts (and analytic ones, with the same bits) -> (focals (n,) float64, R (n, 3, 3) float32, info
        dict).  Nothing is applied to the context."""
        import numpy as np
        marr, mcnt = _match_array(matches)
        prm = params if params is not None else rig_focal_default_params()
        f = np.empty(self.n, np.float64); out = np.empty((self.n, 3, 3), np.float32)
        info = RigFocalInfo()
        _chk(load().ms_refine_rig_focals_lens(self._ctx, marr, mcnt, C.byref(prm), f.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_float)),
                                              C.byref(info), _stream()))
        return f, out, _rig_focal_info(info)

    def refine_rig_coeffs(self, matches, params=None):
        """ms_refine_rig_coeffs_ctx: refine_rig_focals_lens with the coefficients params.free_coeffs of the lens all views share free -> (focals (n,) float64,
        R (n, 3, 3) float32, Lens, info dict).  Nothing is applied to the context."""
        import numpy as np
        marr, mcnt = _match_array(matches)
        prm = params if params is not None else rig_coeff_default_params()
        f = np.empty(self.n, np.float64); out = np.empty((self.n, 3, 3), np.float32)
        info = RigCoeffInfo()
        lens_out = Lens()
        _chk(load().ms_refine_rig_coeffs_ctx(self._ctx, marr, mcnt, C.byref(prm), f.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_float)),
                                             C.byref(lens_out), C.byref(info), _stream()))
        return f, out, lens_out, _rig_coeff_info(info)

    def refine_rig_pp(self, matches, params=None):
        """ms_refine_rig_pp_ctx: refine_rig_focals_lens with every view's principal point free -> (focals (n,) float64, pp (n, 2) float64: the new K[2], K[5] of
        each view, R (n, 3, 3) float32, info dict).  Nothing is applied to the context."""
        import numpy as np
        marr, mcnt = _match_array(matches)
        prm = params if params is not None else rig_pp_default_params()
        f = np.empty(self.n, np.float64); pp = np.empty((self.n, 2), np.float64); out = np.empty((self.n, 3, 3), np.float32)
        info = RigPpInfo()
        dp = C.POINTER(C.c_double)
        _chk(load().ms_refine_rig_pp_ctx(self._ctx, marr, mcnt, C.byref(prm), f.ctypes.data_as(dp), pp.ctypes.data_as(dp), out.ctypes.data_as(C.POINTER(C.c_float)),
                                         C.byref(info), _stream()))
        return f, pp, out, _rig_pp_info(info)

    def build_maps(self):
        _chk(load().ms_build_maps(self._ctx, _stream()))

    def set_maps(self, rois, xmaps, ymaps):
        """ms_set_maps: the caller's own backward maps instead of build_maps() (no cameras needed).  rois: (x, y, width, height) per view; xmaps / ymaps: float32 cuda
        tensors of height x width per view (row-strided views of larger tensors are fine).  The context keeps copies."""
        assert len(rois) == self.n and len(xmaps) == self.n and len(ymaps) == self.n
        r = (Rect * self.n)(*[Rect(*[int(v) for v in t]) for t in rois])
        xs = (Image * self.n)(*[img(t) for t in xmaps])
        ys = (Image * self.n)(*[img(t) for t in ymaps])
        _chk(load().ms_set_maps(self._ctx, r, xs, ys, _stream()))

    def map_source(self):
        """ms_get_map_source: MAPS_ANALYTIC (build_maps), MAPS_LENS (build_maps with a lens on some view) or MAPS_CUSTOM (set_maps)"""
        v = C.c_int(-1)
        _chk(load().ms_get_map_source(self._ctx, C.byref(v)))
        return v.value

    def build_masks(self, mode=1):
        _chk(load().ms_build_masks(self._ctx, mode, _stream()))

    def set_seam_finder(self, finder):
        """ms_set_seam_finder: SEAM_VORONOI (the default) or SEAM_DP -- what calibrate_seam cuts with.  build_masks(1) has no images and stays Voronoi."""
        _chk(load().ms_set_seam_finder(self._ctx, int(finder)))

    def seam_finder(self):
        v = C.c_int(-1)
        _chk(load().ms_get_seam_finder(self._ctx, C.byref(v)))
        return v.value

    def calibrate_seam(self, full_imgs, K_seam, seam_scale, seam_warp_scale, dilate=False, estimate_gains=True):
        """stitch_calib's seam-scale pipeline; returns the estimated gains."""
        import numpy as np
        arr = (Image * self.n)(*[img(t) for t in full_imgs])
        k = np.ascontiguousarray(K_seam, np.float32).reshape(self.n * 9)
        prm = SeamParams(seam_scale, seam_warp_scale, int(dilate), int(estimate_gains))
        g = (C.c_double * self.n)()
        _chk(load().ms_calibrate_seam(self._ctx, arr, k.ctypes.data_as(C.POINTER(C.c_float)), C.byref(prm), g, _stream()))
        return list(g)

    def set_mask(self, view, mask_np):
        import numpy as np
        m = np.ascontiguousarray(mask_np, np.uint8)
        _chk(load().ms_set_mask(self._ctx, view, m.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(m.strides[0])))

    def init_blender(self):
        _chk(load().ms_init_blender(self._ctx, _stream()))

    def set_mesh_interp(self, view, start, end, progress):
        """start / end: (mesh_x, mesh_y) pairs of N x M float32 host arrays."""
        import numpy as np
        a = [np.ascontiguousarray(m, np.float32) for m in (start[0], start[1], end[0], end[1])]
        n, m = a[0].shape
        fp = C.POINTER(C.c_float)
        _chk(load().ms_set_mesh_interp(self._ctx, view, a[0].ctypes.data_as(fp), a[1].ctypes.data_as(fp), a[2].ctypes.data_as(fp),
                                       a[3].ctypes.data_as(fp), n, m, C.c_float(progress), _stream()))

    def feed(self, view, image):
        _chk(load().ms_feed(self._ctx, view, C.byref(img(image)), _stream()))

    def blend(self, out8u=None, out16s=None):
        o8 = C.byref(img(out8u)) if out8u is not None else None
        o16 = C.byref(img(out16s)) if out16s is not None else None
        _chk(load().ms_blend(self._ctx, o8, o16, _stream()))

    def mesh_displacement(self, view):
        d = C.c_float(0)
        _chk(load().ms_get_mesh_displacement(self._ctx, view, C.byref(d)))
        return d.value

    def update_mask(self, view):
        _chk(load().ms_update_mask(self._ctx, view, _stream()))

    def init_feather(self, sharpness=0.02):
        _chk(load().ms_init_feather(self._ctx, C.c_float(sharpness), _stream()))

    def set_mesh(self, view, mesh_x, mesh_y):
        ax, px = _fa(mesh_x, mesh_x.size); ay, py = _fa(mesh_y, mesh_y.size)
        _chk(load().ms_set_mesh(self._ctx, view, px, py, mesh_x.shape[0], mesh_x.shape[1], _stream()))

    def set_meshes(self, meshes):
        """convertMeshesToMap for every view in one call: meshes = [(mesh_x, mesh_y)] * num_views, all N x M float32 host arrays."""
        import numpy as np
        mx = np.ascontiguousarray(np.stack([m[0] for m in meshes]), np.float32)
        my = np.ascontiguousarray(np.stack([m[1] for m in meshes]), np.float32)
        assert mx.shape[0] == self.n and mx.shape == my.shape
        fp = C.POINTER(C.c_float)
        _chk(load().ms_set_meshes(self._ctx, mx.ctypes.data_as(fp), my.ctypes.data_as(fp), mx.shape[1], mx.shape[2], _stream()))

    def set_mesh_maps(self, view, xm, ym):
        _chk(load().ms_set_mesh_maps(self._ctx, view, C.byref(img(xm)), C.byref(img(ym)), _stream()))

    def view_geom(self, view):
        g = ViewGeom()
        _chk(load().ms_get_view_geom(self._ctx, view, C.byref(g)))
        return g

    def pano_geom(self):
        g = PanoGeom()
        _chk(load().ms_get_pano_geom(self._ctx, C.byref(g)))
        return g

    def pano_frame(self, which=PANO_CANVAS):
        """ms_get_pano_frame: how the canvas (PANO_CANVAS) or the pano ROI (PANO_ROI) lies on the warper surface, for build_view_maps"""
        p = PanoFrame()
        _chk(load().ms_get_pano_frame(self._ctx, which, C.byref(p)))
        return p

    def maps(self, view):
        xm, ym = Image(), Image()
        _chk(load().ms_get_maps(self._ctx, view, C.byref(xm), C.byref(ym)))
        return tensor_of(xm), tensor_of(ym)

    def mask(self, view):
        m = Image()
        _chk(load().ms_get_mask(self._ctx, view, C.byref(m)))
        return tensor_of(m)

    def weight_level(self, view, level):
        m = Image()
        _chk(load().ms_get_weight_level(self._ctx, view, level, C.byref(m)))
        return tensor_of(m)

    def mesh_maps(self, view):
        xm, ym = Image(), Image()
        _chk(load().ms_get_mesh_maps(self._ctx, view, C.byref(xm), C.byref(ym)))
        return tensor_of(xm), tensor_of(ym)

    def result_mask(self):
        m = Image()
        _chk(load().ms_get_result_mask(self._ctx, C.byref(m)))
        return tensor_of(m)

    def band_cells(self, level):
        """(owned, exclusive, general) 64 x 16 cells of a band: see ms_get_band_cells."""
        a, b, c = C.c_uint(), C.c_uint(), C.c_uint()
        _chk(load().ms_get_band_cells(self._ctx, level, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def stitch_kernels(self):
        """(warp kernel, stage-1 kernel) of the last stitch call: ms_get_stitch_kernels, as names."""
        names = {0: "none", 1: "simple", 2: "shared_aligned", 3: "shared_unaligned", 4: "per_frame_aligned", 5: "per_frame_unaligned", 6: "nv12", 7: "lds_staged"}
        a, b = C.c_int(), C.c_int()
        _chk(load().ms_get_stitch_kernels(self._ctx, C.byref(a), C.byref(b)))
        return names[a.value], names[b.value]

    def plan_stats(self):
        """Work-list sizes of the context (ms_get_plan_stats) as a dict."""
        st = PlanStats()
        st.struct_size = C.sizeof(PlanStats)
        _chk(load().ms_get_plan_stats(self._ctx, C.byref(st)))
        return {"warp_tile": (st.warp_tile_w, st.warp_tile_h), "n_warp_tiles": st.n_warp_tiles, "n_stage1_tiles": st.n_stage1_tiles,
                "n_stage1_reachable": st.n_stage1_reachable, "down_tile": (st.down_tile_w, st.down_tile_h), "n_down_tiles": list(st.n_down_tiles),
                "blend_tile": (st.blend_tile_w, st.blend_tile_h), "n_blend_tiles": list(st.n_blend_tiles)}

    def _tables(self, frames, out8u, out16s):
        n_frames = len(frames)
        views = (Image * (n_frames * self.n))()
        k = 0
        for fr in frames:
            assert len(fr) == self.n
            for t in fr:
                views[k] = img(t) if t is not None else Image(); k += 1      # None: a view this (column / view) shard never reads
        o8 = o16 = None
        if out8u is not None:
            o8 = (Image * n_frames)(*[img(t) if t is not None else Image() for t in out8u])      # None: no 8U canvas for this frame (data == NULL)
        if out16s is not None:
            o16 = (Image * n_frames)(*[img(t) if t is not None else Image() for t in out16s])
        return n_frames, views, o8, o16

    def stitch(self, frames, out8u=None, out16s=None):
        """frames: list (per frame) of lists (per view) of uint8 HxWx3 cuda tensors."""
        n, views, o8, o16 = self._tables(frames, out8u, out16s)
        _chk(load().ms_stitch(self._ctx, n, views, o8, o16, _stream()))

    def stitch_nv12(self, frames_nv12, out8u=None, out16s=None):
        """ms_stitch_nv12: frames_nv12 = list (per frame) of lists (per view) of uint8 (H * 3 / 2) x W cuda tensors (the cameras' NV12 planes)"""
        n, views, o8, o16 = self._tables(frames_nv12, out8u, out16s)
        _chk(load().ms_stitch_nv12(self._ctx, n, views, o8, o16, _stream()))

    def prepared_nv12(self, frames_nv12, out8u=None, out16s=None):
        n, views, o8, o16 = self._tables(frames_nv12, out8u, out16s)
        fn, ctx = load().ms_stitch_nv12, self._ctx

        def run(stream=None):
            _chk(fn(ctx, n, views, o8, o16, stream if stream is not None else _stream()))
        run.keepalive = (frames_nv12, out8u, out16s, views, o8, o16)
        return run

    def prepared(self, frames, out8u=None, out16s=None):
        """Pre-marshal the descriptor tables once; returns a zero-overhead callable for timed loops."""
        n, views, o8, o16 = self._tables(frames, out8u, out16s)
        fn, ctx = load().ms_stitch, self._ctx

        def run(stream=None):
            _chk(fn(ctx, n, views, o8, o16, stream if stream is not None else _stream()))
        run.keepalive = (frames, out8u, out16s, views, o8, o16)
        return run

    def col_window(self):
        """(begin, end) pano-ROI columns this context composites (column sharding); the whole ROI otherwise."""
        a, b = C.c_int(0), C.c_int(0)
        _chk(load().ms_get_col_window(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_active_views(self, mask, stream=None):
        """ms_set_active_views: composite only the views whose bit is set (camera dropout); enqueue-only, takes effect at the next stitch call."""
        st = _stream() if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))      # a torch.cuda.Stream or a raw hipStream_t
        _chk(load().ms_set_active_views(self._ctx, C.c_uint(mask), st))

    def _one_frame(self, frames):
        assert len(frames) == self.n
        views = (Image * self.n)()
        for k, t in enumerate(frames):
            views[k] = img(t) if t is not None else Image()      # None: a view outside the active set (never read)
        return views

    def gain_stats(self, frames, stride):
        """ms_gain_stats: the exposure tracker's overlap statistics of one frame set (list per view of uint8 HxWx3 cuda tensors); (N, S) as n x n int64 numpy arrays.  Blocking."""
        import numpy as np
        N = np.zeros((self.n, self.n), dtype=np.int64)
        S = np.zeros((self.n, self.n), dtype=np.int64)
        views = self._one_frame(frames)
        _chk(load().ms_gain_stats(self._ctx, views, int(stride), N.ctypes.data_as(C.c_void_p), S.ctypes.data_as(C.c_void_p), _stream()))
        return N, S

    def track_gains(self, frames, stride=None, smoothing=None, stream=None):
        """ms_track_gains: re-estimate the view gains from one live frame set on the stream; enqueue-only, the next stitch on that stream uses them."""
        p = gain_track_default_params()
        if stride is not None:
            p.stride = int(stride)
        if smoothing is not None:
            p.smoothing = float(smoothing)
        st = _stream() if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        views = self._one_frame(frames)
        _chk(load().ms_track_gains(self._ctx, views, C.byref(p), st))

    def gain_stats_nv12(self, frames_nv12, stride):
        """ms_gain_stats_nv12: gain_stats with the frames given as the cameras' NV12 planes (list per view of uint8 (H * 3 / 2) x W cuda tensors)."""
        import numpy as np
        N = np.zeros((self.n, self.n), dtype=np.int64)
        S = np.zeros((self.n, self.n), dtype=np.int64)
        views = self._one_frame(frames_nv12)
        _chk(load().ms_gain_stats_nv12(self._ctx, views, int(stride), N.ctypes.data_as(C.c_void_p), S.ctypes.data_as(C.c_void_p), _stream()))
        return N, S

    def track_gains_nv12(self, frames_nv12, stride=None, smoothing=None, stream=None):
        """ms_track_gains_nv12: track_gains from the cameras' NV12 planes; shares the gain state with track_gains (calls may alternate)."""
        p = gain_track_default_params()
        if stride is not None:
            p.stride = int(stride)
        if smoothing is not None:
            p.smoothing = float(smoothing)
        st = _stream() if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        views = self._one_frame(frames_nv12)
        _chk(load().ms_track_gains_nv12(self._ctx, views, C.byref(p), st))

    def gains(self, stream=None, counters=False):
        """ms_get_gains: the gains the next stitch on the stream uses (numpy float64); with counters=True also (solves_ok, solves_singular)."""
        import numpy as np
        g = np.zeros(self.n, dtype=np.float64)
        ok, sing = C.c_int(0), C.c_int(0)
        st = _stream() if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        _chk(load().ms_get_gains(self._ctx, g.ctypes.data_as(C.c_void_p), C.byref(ok), C.byref(sing), st))
        return (g, ok.value, sing.value) if counters else g

    def gain_partial_bytes(self):
        """ms_gain_partial_bytes: size of one partial statistic of this context."""
        fn = load().ms_gain_partial_bytes
        fn.restype = C.c_size_t
        return int(fn(self._ctx))

    def new_gain_partial(self):
        """A zeroed device buffer for one partial (int64 elements: 8-byte aligned)."""
        torch = _torch()
        return torch.zeros(self.gain_partial_bytes() // 8, dtype=torch.int64, device="cuda")

    def gain_views(self):
        """ms_get_gain_views: bit mask of the views to upload for a time step that is tracked on (those the partial statistic reads, and those ms_stitch reads)."""
        m = C.c_uint(0)
        _chk(load().ms_get_gain_views(self._ctx, C.byref(m)))
        return m.value

    def gain_stats_partial(self, frames, stride, partial=None, nv12=False, stream=None):
        """ms_gain_stats_partial[_nv12]: this context's column-window share of the overlap statistics into `partial` (new_gain_partial() if None); enqueue-only.  Returns the partial."""
        if partial is None:
            partial = self.new_gain_partial()
        st = _stream() if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        views = self._one_frame(frames)
        fn = load().ms_gain_stats_partial_nv12 if nv12 else load().ms_gain_stats_partial
        _chk(fn(self._ctx, views, int(stride), C.c_void_p(partial.data_ptr()), st))
        return partial

    def track_gains_from_partials(self, partials, stride=None, smoothing=None, stream=None):
        """ms_track_gains_from_partials: sum the partials (device tensors, the same order on every shard), solve, smooth and publish on the stream; enqueue-only."""
        p = gain_track_default_params()
        if stride is not None:
            p.stride = int(stride)
        if smoothing is not None:
            p.smoothing = float(smoothing)
        st = _stream() if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        arr = (C.c_void_p * len(partials))(*[t.data_ptr() for t in partials])
        _chk(load().ms_track_gains_from_partials(self._ctx, arr, len(partials), C.byref(p), st))

    def gain_samples_bytes(self, stride, view_shard_index=-1):
        """ms_gain_samples_bytes: size of the sample buffer of view shard `view_shard_index` (-1: this context's own) at this stride; 0 = refused."""
        fn = load().ms_gain_samples_bytes
        fn.restype = C.c_size_t
        return int(fn(self._ctx, int(stride), int(view_shard_index)))

    def view_shard(self):
        """ms_get_view_shard: (view_shards, view_shard_index) of this context; (1, 0) without view sharding."""
        a, b = C.c_int(0), C.c_int(0)
        _chk(load().ms_get_view_shard(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def gain_sample_views(self):
        """ms_get_gain_sample_views: bit mask of the views gain_samples reads (owned and active)."""
        m = C.c_uint(0)
        _chk(load().ms_get_gain_sample_views(self._ctx, C.byref(m)))
        return m.value

    def gain_samples(self, frames, stride, samples=None, nv12=False, stream=None):
        """ms_gain_samples[_nv12]: the sample vectors of this context's own views into `samples` (a zeroed int32 cuda tensor of gain_samples_bytes(stride) if
        None); enqueue-only.  Returns the buffer."""
        if samples is None:
            samples = _torch().zeros(self.gain_samples_bytes(stride) // 4, dtype=_torch().int32, device="cuda")
        st = _stream() if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        views = self._one_frame(frames)
        fn = load().ms_gain_samples_nv12 if nv12 else load().ms_gain_samples
        _chk(fn(self._ctx, views, int(stride), C.c_void_p(samples.data_ptr()), st))
        return samples

    def gain_samples_nv12(self, frames_nv12, stride, samples=None, stream=None):
        """ms_gain_samples_nv12: gain_samples from the cameras' NV12 planes."""
        return self.gain_samples(frames_nv12, stride, samples=samples, nv12=True, stream=stream)

    def gain_stats_from_samples(self, samples, stride):
        """ms_gain_stats_from_samples: (N, S) as gain_stats reports them, formed from the shards' sample buffers (device tensors, any order).  Blocking."""
        import numpy as np
        N = np.zeros((self.n, self.n), dtype=np.int64)
        S = np.zeros((self.n, self.n), dtype=np.int64)
        arr = (C.c_void_p * len(samples))(*[t.data_ptr() for t in samples])
        _chk(load().ms_gain_stats_from_samples(self._ctx, arr, len(samples), int(stride), N.ctypes.data_as(C.c_void_p), S.ctypes.data_as(C.c_void_p), _stream()))
        return N, S

    def track_gains_from_samples(self, samples, stride=None, smoothing=None, stream=None):
        """ms_track_gains_from_samples: pair the shards' sample buffers (device tensors), solve, smooth and publish on the stream; enqueue-only."""
        p = gain_track_default_params()
        if stride is not None:
            p.stride = int(stride)
        if smoothing is not None:
            p.smoothing = float(smoothing)
        st = _stream() if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        arr = (C.c_void_p * len(samples))(*[t.data_ptr() for t in samples])
        _chk(load().ms_track_gains_from_samples(self._ctx, arr, len(samples), C.byref(p), st))

    def gain_track_counters(self, stream=None):
        """ms_get_gain_track_counters: (solves_ok, solves_singular, updates_rejected); waits for the stream."""
        k = GainTrackCounters(struct_size=C.sizeof(GainTrackCounters))
        st = _stream() if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        _chk(load().ms_get_gain_track_counters(self._ctx, C.byref(k), st))
        return k.solves_ok, k.solves_singular, k.updates_rejected

    def active_views(self):
        """Bit mask of the views the next stitch call composites (ms_get_active_views)."""
        m = C.c_uint(0)
        _chk(load().ms_get_active_views(self._ctx, C.byref(m)))
        return m.value

    def needed_views(self):
        """Bit mask of the views ms_stitch reads (column / view shards read a subset)."""
        m = C.c_uint(0)
        _chk(load().ms_get_needed_views(self._ctx, C.byref(m)))
        return m.value

    def i420_rows(self):
        """(first canvas row, rows) of the even-aligned span the I420 output holds."""
        a, b = C.c_int(0), C.c_int(0)
        _chk(load().ms_get_i420_rows(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def new_i420(self, n_frames=1):
        """Black I420 buffers (Y = 16, U = V = 128) of the size ms_stitch_i420 writes."""
        torch = _torch()
        _, rows = self.i420_rows()
        w = self.cfg.out_width
        outs = []
        for _ in range(n_frames):
            t = torch.full((rows * 3 // 2, w), 128, dtype=torch.uint8, device="cuda")
            t[:rows] = 16
            outs.append(t)
        return outs

    def prepared_i420(self, frames, out_i420):
        n, views, _, _ = self._tables(frames, None, None)
        oi = (Image * n)(*[img(t) for t in out_i420])
        fn, ctx = load().ms_stitch_i420, self._ctx

        def run(stream=None):
            _chk(fn(ctx, n, views, oi, stream if stream is not None else _stream()))
        run.keepalive = (frames, out_i420, views, oi)
        return run

    def prepared_nv12_i420(self, frames_nv12, out_i420):
        n, views, _, _ = self._tables(frames_nv12, None, None)
        oi = (Image * n)(*[img(t) for t in out_i420])
        fn, ctx = load().ms_stitch_nv12_i420, self._ctx

        def run(stream=None):
            _chk(fn(ctx, n, views, oi, stream if stream is not None else _stream()))
        run.keepalive = (frames_nv12, out_i420, views, oi)
        return run

    def stitch_nv12_i420(self, frames_nv12, out_i420):
        """ms_stitch_nv12_i420: the cameras' NV12 planes in, the encoder's planar I420 out (buffers as stitch_i420)."""
        self.prepared_nv12_i420(frames_nv12, out_i420)()

    def stitch_i420(self, frames, out_i420):
        """The panorama as planar I420 (encoder input), written by the level-0 band kernel: no 8UC3 canvas, no conversion pass."""
        self.prepared_i420(frames, out_i420)()

    def partial_bytes(self):
        load().ms_partial_bytes.restype = C.c_size_t
        return load().ms_partial_bytes(self._ctx)

    def stitch_partial(self, frames, partial):
        """frames: per frame a list of N tensors (None for views this shard does not own); partial: int16 cuda tensor."""
        n_frames = len(frames)
        views = (Image * (n_frames * self.n))()
        k = 0
        for fr in frames:
            for t in fr:
                if t is not None:
                    views[k] = img(t)
                k += 1
        _chk(load().ms_stitch_partial(self._ctx, n_frames, views, C.c_void_p(partial.data_ptr()), _stream()))

    def stitch_finish(self, n_frames, partials, out8u=None, out16s=None):
        ptrs = (C.c_void_p * len(partials))(*[p.data_ptr() for p in partials])
        o8 = (Image * n_frames)(*[img(t) for t in out8u]) if out8u is not None else None
        o16 = (Image * n_frames)(*[img(t) for t in out16s]) if out16s is not None else None
        _chk(load().ms_stitch_finish(self._ctx, n_frames, ptrs, len(partials), o8, o16, _stream()))

    def stitch_timed(self, frames, out8u=None, out16s=None):
        n, views, o8, o16 = self._tables(frames, out8u, out16s)
        cap = 32
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        k = _chk(load().ms_stitch_timed(self._ctx, n, views, o8, o16, _stream(), cap, names, ms))
        return [(names[i].decode(), ms[i]) for i in range(k)]
