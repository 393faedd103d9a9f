"""MI355X-native front-end of the ORB-SLAM2 point+line fork — host-side mirror.

Python mirror of the reference's per-frame operator interfaces, each a thin
ctypes layer over the C-ABI in include/orbpl.h (liborbpl.so, built in-tree
from csrc/ for gfx950):

  ORBextractor  — ORB_SLAM2::ORBextractor (include/ORBextractor.h:44-112)

Every call goes to the HIP library; there is no CPU fallback. If liborbpl.so
is missing or no GPU is visible, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
# ORBPL_LIB: an alternative build of the same library (dev A/B runs)
LIB_PATH = Path(os.environ.get("ORBPL_LIB") or (PKG_DIR / "liborbpl.so"))

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

ORBPL_OK = 0
ORBPL_ERR_ARG = -1
ORBPL_ERR_CAPACITY = -2
ORBPL_ERR_HIP = -3
ORBPL_ERR_NODEVICE = -4
ORBPL_ERR_OVERFLOW = -5


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


class OrbplError(RuntimeError):
    pass


_lib = None


def lib():
    """Load liborbpl.so (fails loudly: the product has no fallback path)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise OrbplError(f"{LIB_PATH} not built; run __graft_entry__.build() or make -C csrc")
        _lib = C.CDLL(str(LIB_PATH))
        for declare in _DECLARE:
            declare(_lib)
    return _lib


def _declare_core(L):
    vp, i, ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
    L.orbpl_last_error.restype = C.c_char_p
    L.orbpl_version.restype = C.c_char_p
    L.orbpl_device_count.argtypes = [ip]
    L.orbx_create.argtypes = [vp, i, i, i, i, C.POINTER(vp)]
    L.orbx_destroy.argtypes = [vp]
    L.orbx_get_scale_info.argtypes = [vp, ip, vp, vp, vp, vp]
    L.orbx_get_level_info.argtypes = [vp, vp, vp, vp]
    L.orbx_max_keypoints.argtypes = [vp]
    L.orbx_describe.argtypes = [vp, i, i, vp, vp, vp, vp, ip]
    L.orbx_extract.argtypes = [vp, vp, i, i, i, vp, vp, i, ip]
    L.orbx_extract_batch_device.argtypes = [vp, vp, i, i, C.c_int64, vp, vp, i, vp]
    L.orbx_get_pyramid.argtypes = [vp, i, i, i, i, vp, i, ip, ip]
    L.orbx_get_candidates.argtypes = [vp, vp, i, vp, ip]
    L.orbx_synchronize.argtypes = [vp]
    L.orbx_last_stage_ms.argtypes = [vp, vp]
    L.orbpl_descriptor_distance.argtypes = [vp, vp]
    L.orbpl_dev_malloc.argtypes = [i, C.c_int64, C.POINTER(vp)]
    L.orbpl_dev_free.argtypes = [i, vp]
    L.orbpl_memcpy_htod.argtypes = [i, vp, vp, C.c_int64]
    L.orbpl_host_alloc.argtypes = [C.c_int64, C.POINTER(vp)]
    L.orbpl_host_free.argtypes = [vp]
    L.orbpl_memcpy_dtoh.argtypes = [i, vp, vp, C.c_int64]
    L.orbpl_memset_d.argtypes = [i, vp, i, C.c_int64]
    L.orbpl_device_synchronize.argtypes = [i]


def check(rc, what=""):
    if rc != ORBPL_OK:
        msg = lib().orbpl_last_error().decode(errors="replace")
        raise OrbplError(f"{what} failed with {rc}: {msg}")
    return rc


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _rows_u8(image):
    """A 2-D u8 image as (array, row pitch in bytes): a view whose rows are
    contiguous (a cv::Mat ROI: step > cols) is passed as is with its pitch,
    anything else is copied contiguous."""
    a = np.asarray(image)
    if a.dtype == np.uint8 and a.ndim == 2 and a.strides[1] == 1 and a.strides[0] >= a.shape[1]:
        return a, int(a.strides[0])
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a, (a.shape[1] if a.ndim == 2 else 0)


class DeviceBuffer:
    """Owned device allocation (hipMalloc via the C-ABI)."""

    def __init__(self, nbytes, device=0):
        self.nbytes, self.device = int(nbytes), device
        p = C.c_void_p()
        check(lib().orbpl_dev_malloc(device, self.nbytes, C.byref(p)), "orbpl_dev_malloc")
        self.ptr = p.value

    @classmethod
    def from_array(cls, arr, device=0):
        arr = np.ascontiguousarray(arr)
        b = cls(arr.nbytes, device)
        b.upload(arr)
        return b

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert 0 <= offset and offset + arr.nbytes <= self.nbytes
        check(lib().orbpl_memcpy_htod(self.device, C.c_void_p(self.ptr + offset), _ptr(arr),
                                      arr.nbytes), "orbpl_memcpy_htod")

    def download(self, dtype, shape):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        check(lib().orbpl_memcpy_dtoh(self.device, _ptr(out), C.c_void_p(self.ptr), out.nbytes),
              "orbpl_memcpy_dtoh")
        return out

    def zero(self):
        check(lib().orbpl_memset_d(self.device, C.c_void_p(self.ptr), 0, self.nbytes),
              "orbpl_memset_d")

    def free(self):
        if self.ptr:
            lib().orbpl_dev_free(self.device, C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HostBuffer:
    """Page-locked host allocation (orbpl_host_alloc) viewed as a numpy array."""

    def __init__(self, shape, dtype):
        self.dtype, self.shape = np.dtype(dtype), tuple(np.atleast_1d(shape))
        nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        check(lib().orbpl_host_alloc(nbytes, C.byref(p)), "orbpl_host_alloc")
        self.ptr = p.value
        buf = (C.c_uint8 * nbytes).from_address(self.ptr)
        self.array = np.frombuffer(buf, np.uint8, nbytes).view(self.dtype).reshape(self.shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib().orbpl_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_count():
    n = C.c_int(0)
    lib().orbpl_device_count(C.byref(n))
    return n.value


def describe(nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7,
             width=640, height=480):
    """Device-free geometry of an extractor (level sizes, budgets, capacity)."""
    p = OrbParams(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
    lw = np.zeros(nlevels, np.int32)
    lh = np.zeros(nlevels, np.int32)
    nf = np.zeros(nlevels, np.int32)
    sc = np.zeros(nlevels, np.float32)
    mk = C.c_int(0)
    check(lib().orbx_describe(C.byref(p), width, height, _ptr(lw), _ptr(lh), _ptr(nf), _ptr(sc),
                              C.byref(mk)), "orbx_describe")
    return dict(width=lw, height=lh, nfeatures=nf, scale=sc, max_keypoints=mk.value)


class ORBextractor:
    """Drop-in for ORB_SLAM2::ORBextractor (ORBextractor.h:44-112).

    ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) with
    the image geometry fixed at construction (the device buffers and the
    pyramid/cell/resize tables are sized for it). ``extractor(image)`` returns
    ``(keypoints, descriptors)`` exactly like ``operator()(image, mask,
    keypoints, descriptors)``: keypoints as a KP_DTYPE structured array
    (cv::KeyPoint fields), descriptors as an (N, 32) uint8 array.
    """

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7,
                 width=640, height=480, max_batch=1, device=0):
        self._p = OrbParams(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
        self.width, self.height, self.max_batch, self.device = width, height, max_batch, device
        h = C.c_void_p()
        check(lib().orbx_create(C.byref(self._p), width, height, max_batch, device, C.byref(h)),
              "orbx_create")
        self._h = h
        self.nlevels = nlevels
        self.scaleFactor = scaleFactor
        n = C.c_int(0)
        self._scale = np.zeros(nlevels, np.float32)
        self._inv_scale = np.zeros(nlevels, np.float32)
        self._sigma2 = np.zeros(nlevels, np.float32)
        self._inv_sigma2 = np.zeros(nlevels, np.float32)
        check(lib().orbx_get_scale_info(h, C.byref(n), _ptr(self._scale), _ptr(self._inv_scale),
                                        _ptr(self._sigma2), _ptr(self._inv_sigma2)),
              "orbx_get_scale_info")
        self.max_keypoints = lib().orbx_max_keypoints(h)

    def close(self):
        if getattr(self, "_h", None):
            lib().orbx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- ORBextractor.h:60-80 getters ---
    def GetLevels(self):
        return self.nlevels

    def GetScaleFactor(self):
        return float(np.float32(self.scaleFactor))

    def GetScaleFactors(self):
        return self._scale.copy()

    def GetInverseScaleFactors(self):
        return self._inv_scale.copy()

    def GetScaleSigmaSquares(self):
        return self._sigma2.copy()

    def GetInverseScaleSigmaSquares(self):
        return self._inv_sigma2.copy()

    def __call__(self, image, mask=None):
        """operator()(image, mask, keypoints, descriptors); mask is ignored as
        in the reference (ORBextractor.h:56)."""
        if image is None or image.size == 0:
            return np.zeros(0, KP_DTYPE), None
        img, stride = _rows_u8(image)
        assert img.ndim == 2, "CV_8UC1 image expected (ORBextractor.cc:1050)"
        h, w = img.shape
        cap = self.max_keypoints
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        check(lib().orbx_extract(self._h, _ptr(img), w, h, stride, _ptr(kps), _ptr(desc), cap,
                                 C.byref(n)), "orbx_extract")
        k = n.value
        return kps[:k].copy(), (desc[:k].copy() if k else None)

    def extract_batch_device(self, d_imgs, batch, stride, frame_pitch, d_kps, d_desc, kp_pitch, d_n):
        """Batched device-resident extraction (pointers are device addresses)."""
        check(lib().orbx_extract_batch_device(self._h, C.c_void_p(d_imgs), batch, stride,
                                              frame_pitch, C.c_void_p(d_kps), C.c_void_p(d_desc),
                                              kp_pitch, C.c_void_p(d_n)),
              "orbx_extract_batch_device")

    def synchronize(self):
        check(lib().orbx_synchronize(self._h), "orbx_synchronize")

    def stage_ms(self):
        ms = np.zeros(5, np.float32)
        check(lib().orbx_last_stage_ms(self._h, _ptr(ms)), "orbx_last_stage_ms")
        return ms

    def pyramid_level(self, level, padded=False, blurred=False, frame=0):
        w, h = C.c_int(0), C.c_int(0)
        check(lib().orbx_get_pyramid(self._h, frame, level, int(padded), int(blurred), None, 0,
                                     C.byref(w), C.byref(h)), "orbx_get_pyramid")
        out = np.zeros((h.value, w.value), np.uint8)
        check(lib().orbx_get_pyramid(self._h, frame, level, int(padded), int(blurred), _ptr(out),
                                     out.size, C.byref(w), C.byref(h)), "orbx_get_pyramid")
        return out

    @property
    def mvImagePyramid(self):
        """Public member of the reference (ORBextractor.h:83): content of each
        level of the last extracted image."""
        return [self.pyramid_level(l) for l in range(self.nlevels)]

    def candidates(self, cap=1 << 21):
        """Pre-octree FAST candidates per level (debug/parity)."""
        xyr = np.zeros((cap, 3), np.float32)
        cnt = np.zeros(self.nlevels, np.int32)
        tot = C.c_int(0)
        check(lib().orbx_get_candidates(self._h, _ptr(xyr), cap, _ptr(cnt), C.byref(tot)),
              "orbx_get_candidates")
        out, off = [], 0
        for c in cnt:
            out.append(xyr[off:off + c].copy())
            off += c
        return out


def DescriptorDistance(a, b):
    """ORBmatcher::DescriptorDistance (ORBmatcher.cc:2083-2103)."""
    a = np.ascontiguousarray(a, np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    return lib().orbpl_descriptor_distance(_ptr(a), _ptr(b))


# ---------------------------------------------------------------------------
# Frame glue / matcher / pose optimiser / tracker (include/orbpl.h)
# ---------------------------------------------------------------------------
class Camera(C.Structure):
    """orbpl_camera: Camera.* settings (Examples/RGB-D/TUM1.yaml)."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("k1", C.c_float), ("k2", C.c_float), ("p1", C.c_float), ("p2", C.c_float),
                ("k3", C.c_float), ("bf", C.c_float), ("th_depth", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32)]


class Settings(C.Structure):
    """orbpl_settings: Tracking::Tracking's settings (Tracking.cc:53-147)."""
    _fields_ = [("orb", OrbParams), ("cam", Camera), ("fps", C.c_float),
                ("max_frames", C.c_int32), ("depth_map_factor", C.c_float),
                ("depth_map_factor_setting", C.c_float), ("rgb", C.c_int32)]


SENSOR = {"monocular": 0, "stereo": 1, "rgbd": 2}


def load_settings(path, sensor="rgbd"):
    """The reference's OpenCV FileStorage YAML settings through the native
    reader (orbpl_settings_load, OpenCV 3.4 FileNode semantics): (OrbParams,
    Camera, dict(fps, max_frames, depth_map_factor, rgb))."""
    out = Settings()
    L = lib()
    L.orbpl_settings_load.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
    check(L.orbpl_settings_load(str(path).encode(), SENSOR[sensor], C.byref(out)),
          "orbpl_settings_load")
    return out.orb, out.cam, dict(fps=out.fps, max_frames=out.max_frames,
                                  depth_map_factor=out.depth_map_factor,
                                  depth_map_factor_setting=out.depth_map_factor_setting,
                                  rgb=out.rgb)


def th_depth(cfg):
    """mThDepth = mbf * (float)ThDepth / fx in float arithmetic, as
    Tracking::Tracking computes it (Tracking.cc:136)."""
    return float(np.float32(cfg["bf"]) * np.float32(cfg["thdepth"]) / np.float32(cfg["fx"]))


def make_camera(cfg):
    """Camera from a settings dict (synth.TUM1 etc.); mThDepth = bf*ThDepth/fx
    (Tracking.cc:134-138, th_depth)."""
    return Camera(cfg["fx"], cfg["fy"], cfg["cx"], cfg["cy"], cfg["k1"], cfg["k2"], cfg["p1"],
                  cfg["p2"], cfg["k3"], cfg["bf"], th_depth(cfg),
                  cfg["width"], cfg["height"])


class MatchCurrent(C.Structure):
    _fields_ = [("n", C.c_int32), ("Tcw", C.c_void_p), ("kps_un", C.c_void_p),
                ("desc", C.c_void_p), ("uright", C.c_void_p)]


class MatchLast(C.Structure):
    _fields_ = [("n", C.c_int32), ("Tcw", C.c_void_p), ("kps_un", C.c_void_p),
                ("has_mp", C.c_void_p), ("outlier", C.c_void_p), ("mp_xyz", C.c_void_p),
                ("mp_desc", C.c_void_p), ("mp_nobs", C.c_void_p)]


class PoseProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("kps_un", C.c_void_p), ("uright", C.c_void_p),
                ("has_mp", C.c_void_p), ("mp_xyz", C.c_void_p), ("nl", C.c_int32),
                ("kl_obs", C.c_void_p), ("kl_octave", C.c_void_p), ("has_ml", C.c_void_p),
                ("ml_xyz", C.c_void_p), ("inv_sigma2", C.c_void_p), ("nlevels", C.c_int32)]


def _declare_track(L):
    vp, i, ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
    L.orbpl_frame_prepare.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, vp]
    L.orbm_search_by_projection_last.argtypes = [vp, vp, i, vp, vp, C.c_float, i, i, vp, ip]
    L.orbpl_pose_optimization.argtypes = [vp, vp, vp, vp, vp, ip]
    L.orbpl_pose_optimization_ex.argtypes = [vp, vp, i, vp, vp, vp, ip]
    L.orbpl_tracker_create.argtypes = [vp, vp, i, i, C.POINTER(vp)]
    L.orbpl_tracker_destroy.argtypes = [vp]
    L.orbpl_tracker_reset.argtypes = [vp, vp]
    L.orbpl_tracker_clear_velocity.argtypes = [vp, vp]
    L.orbpl_tracker_set_fps.argtypes = [vp, C.c_float]
    L.orbpl_tracker_step.argtypes = [vp, vp, vp]
    L.orbpl_tracker_synchronize.argtypes = [vp]
    L.orbpl_tracker_set_pipelined.argtypes = [vp, C.c_int]
    L.orbpl_tracker_launch_frames.argtypes = [vp, ip, ip]
    L.orbpl_tracker_get_state.argtypes = [vp, vp, vp, vp, vp, vp]
    L.orbpl_tracker_stage_ms.argtypes = [vp, vp]
    L.orbpl_tracker_kp_capacity.argtypes = [vp]
    L.orbpl_tracker_timings.argtypes = [vp, i, vp, ip]
    L.orbpl_tracker_timings_reset.argtypes = [vp]
    L.orbpl_tracker_timing_counts.argtypes = [vp]
    L.orbpl_tracker_kernel_timings.argtypes = [vp, i, vp, ip]
    L.orbpl_tracker_get_frame.argtypes = [vp, i, vp, vp, vp, vp, ip]
    L.orbpl_tracker_create_ex.argtypes = [vp, vp, i, i, i, C.POINTER(vp)]
    L.orbpl_line_frame_prepare.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, vp]
    L.orbl_frame_is_in_frustum.argtypes = [vp, i, vp, vp]
    L.orbpl_stereo_matches.argtypes = [vp, vp, vp, i, vp, vp, i, vp, vp, i, vp, vp]
    L.orbm_search_by_bow.argtypes = [i, vp, vp, vp, vp, i, vp, vp, vp, C.c_float, i, vp, ip]
    L.orbl_search_by_projection_list.argtypes = [vp, vp, i, vp, vp, vp, i, vp, vp, vp, vp, ip, ip]
    L.orbpl_frame_is_in_frustum.argtypes = [vp, C.c_float, i, vp, i, vp, vp, vp, vp, C.c_float,
                                            vp, vp, vp, vp, vp, vp]
    L.orbm_search_by_projection_local.argtypes = [vp, vp, i, vp, i, vp, vp, vp, vp, vp, vp, vp, vp,
                                                  vp, C.c_float, C.c_float, vp, ip]
    L.orbl_search_by_projection_last.argtypes = [vp, vp, i, vp, vp, i, vp, vp, vp, vp, vp, vp, ip]
    L.orbl_search_by_projection_pairs.argtypes = [vp, vp, i, i, vp, vp, vp, i, vp, vp, vp, vp, vp,
                                                  vp, vp, ip, vp, i, ip, vp, ip, ip]
    L.orbl_match_bf_knn.argtypes = [i, vp, i, vp, vp, ip]
    L.orbl_stereo_line_depths.argtypes = [vp, vp, vp, i, vp, vp, i, vp, vp]
    L.orbpl_tracker_get_status.argtypes = [vp, vp, vp, vp, vp]
    L.orbpl_tracker_get_lines.argtypes = [vp, i, vp, vp, vp, vp, ip]
    L.orbpl_tracker_line_timings.argtypes = [vp, i, vp, ip]
    L.orbpl_tracker_step_stereo.argtypes = [vp, vp, vp]
    L.orbpl_tracker_stereo_timings.argtypes = [vp, i, vp, ip]
    L.orbpl_tracker_lsd_timings.argtypes = [vp, i, vp, ip]
    L.orbpl_tracker_set_history.argtypes = [vp, i]
    L.orbpl_tracker_get_history.argtypes = [vp, i, i, vp, vp, ip]
    L.orbpl_tracker_get_local_stats.argtypes = [vp, vp, vp, vp, vp]
    L.orbpl_tracker_set_vocabulary.argtypes = [vp, vp, i]
    L.orbpl_tracker_step_host.argtypes = [vp, vp, vp, C.c_float]
    L.orbpl_tracker_get_bow.argtypes = [vp, i, vp, vp, ip, vp, ip]
    L.orbpl_tracker_get_trk.argtypes = [vp, vp]
    L.orbpl_tracker_get_map_history.argtypes = [vp, i, i, vp, ip]
    L.orbpl_tracker_get_map_errors.argtypes = [vp, vp]
    L.orbpl_tracker_get_map_keyframes.argtypes = [vp, i, vp, vp, i, vp, ip]
    L.orbpl_tracker_get_map_points.argtypes = [vp, i, i, vp, vp, vp, vp, vp, ip]
    L.orbpl_tracker_get_map_lines.argtypes = [vp, i, i, vp, vp, vp, ip]
    L.orbm_search_by_projection_kf.argtypes = [vp, vp, i, vp, vp, i, vp, vp, vp, vp, vp, vp, vp,
                                               C.c_float, i, i, vp, ip]
    L.orbm_search_by_projection_kf_batch_device.argtypes = [vp, vp, i, vp, i, C.c_float, i, i, vp]
    L.orbkf_detect_reloc.argtypes = [vp, i, i]
    L.orbkf_detect_reloc_batch_device.argtypes = [vp, i, i, vp]
    L.orbpnp_ransac_parameters.argtypes = [i, C.c_double, i, i, i, C.c_float, C.c_float, vp, vp,
                                           vp, vp, vp]
    L.orbpnp_iterate.argtypes = [vp, i, i]
    L.orbpnp_iterate_batch_device.argtypes = [vp, i, i, vp]
    L.orbsim3_ransac_parameters.argtypes = [i, C.c_double, i, i, vp]
    L.orbsim3_setup.argtypes = [vp, i, vp, i]
    L.orbsim3_setup_batch_device.argtypes = [vp, i, vp]
    L.orbsim3_iterate.argtypes = [vp, i, i]
    L.orbsim3_iterate_batch_device.argtypes = [vp, i, i, vp]
    L.orbpl_test_sim3_hypothesis.argtypes = [vp, vp, i, vp, i] + [vp] * 12
    L.orbm_search_by_sim3.argtypes = [vp, vp, i, vp, i, C.c_float]
    L.orbm_search_by_sim3_batch_device.argtypes = [vp, vp, i, vp, i, C.c_float, vp]


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _pack_rows(arrays, pitch, dtype, row=(), pad=0):
    """One pitched host column: [max(1, len(arrays)), pitch, *row] of dtype, every
    element `pad` but the first len(a) entries of row s, which are a = arrays[s]
    (None fills nothing). pitch None: one entry of shape `row` per row."""
    out = np.zeros((max(1, len(arrays)),) + (() if pitch is None else (pitch,)) + tuple(row), dtype)
    if pad:
        out[...] = pad
    for s, a in enumerate(arrays):
        if a is None:
            continue
        if pitch is None:
            out[s] = np.asarray(a).reshape(row)
        else:
            a = np.asarray(a).reshape((-1,) + tuple(row))
            out[s, :len(a)] = a
    return out


def _cols(names, dtype, row=(), pitch=None, pad=0):
    """column table entries (name, dtype, row shape, pitch key or None, pad)"""
    return tuple((k, dtype, row, pitch, pad) for k in names.split())


class PitchedProblems:
    """Base of the *DeviceProblems classes over a column table (_cols): pack() makes
    self.host, the pitched host arrays of the table (cols[name] = the per-row arrays
    of a column; a column not in cols has `rows` rows of padding, an entry of cols the
    table lacks is an array taken as it is), and with a device
    their copies self.bufs and self.batch, the batch struct over them (a d_NAME field
    is bufs[NAME], any other field is given by name). device None: no buffer, no
    library call."""

    def pack(self, table, pitches, cols, rows, device, batch, **fields):
        self.device = device
        self.host = {k: _pack_rows(cols.get(k, [None] * rows), pitches.get(pk), dt, row, pad)
                     for k, dt, row, pk, pad in table}
        self.host.update({k: v for k, v in cols.items() if k not in self.host})
        if device is None:
            return
        self.bufs = {k: DeviceBuffer.from_array(v, device) for k, v in self.host.items()}
        self.batch = self.struct(batch, **fields)

    def struct(self, cls, **fields):
        return cls(*[self.bufs[k[2:]].ptr if k.startswith("d_") else fields[k] for k, _ in cls._fields_])

    def fetch(self, *names):
        """synchronises; the named columns from the device, shaped as self.host's"""
        check(lib().orbpl_device_synchronize(self.device), "orbpl_device_synchronize")
        return [self.bufs[k].download(self.host[k].dtype, self.host[k].shape) for k in names]


def frame_prepare(camera, kps, depth=None):
    """Frame glue of the RGB-D Frame constructor (Frame.cc:135-205) on the GPU.
    Returns (kps_un, depth, uright, grid_cell, bounds)."""
    kps = _c(kps, KP_DTYPE)
    n = len(kps)
    ku = np.zeros(n, KP_DTYPE)
    d = np.zeros(n, np.float32)
    ur = np.zeros(n, np.float32)
    gc = np.zeros(n, np.int32)
    b = np.zeros(4, np.float32)
    dp = None if depth is None else _c(depth, np.float32)
    check(lib().orbpl_frame_prepare(C.byref(camera), _ptr(kps), n,
                                    None if dp is None else _ptr(dp), _ptr(ku), _ptr(d), _ptr(ur),
                                    _ptr(gc), _ptr(b)), "orbpl_frame_prepare")
    return ku, d, ur, gc, b


class ORBmatcher:
    """ORB_SLAM2::ORBmatcher(nnratio, checkOri) — per-frame SearchByProjection."""

    def __init__(self, nnratio=0.6, checkOri=True):
        self.nnratio, self.checkOri = nnratio, checkOri

    def SearchByProjectionLastFrame(self, camera, scale_factors, cur, last, th, bMono=False):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono)
        (ORBmatcher.cc:1710-1879). ``cur``/``last`` are dicts of arrays (see
        tests). Returns (match, nmatches): match[i] = last-frame index or -1."""
        sf = _c(scale_factors, np.float32)
        keep = []

        def arr(a, dt):
            a = _c(a, dt)
            keep.append(a)
            return _ptr(a)

        mc = MatchCurrent(len(cur["kps_un"]), arr(cur["Tcw"], np.float32),
                          arr(cur["kps_un"], KP_DTYPE), arr(cur["desc"], np.uint8),
                          arr(cur["uright"], np.float32))
        ml = MatchLast(len(last["kps_un"]), arr(last["Tcw"], np.float32),
                       arr(last["kps_un"], KP_DTYPE), arr(last["has_mp"], np.uint8),
                       arr(last["outlier"], np.uint8), arr(last["mp_xyz"], np.float32),
                       arr(last["mp_desc"], np.uint8), arr(last["mp_nobs"], np.int32))
        match = np.zeros(max(1, mc.n), np.int32)
        nm = C.c_int(0)
        check(lib().orbm_search_by_projection_last(C.byref(camera), _ptr(sf), len(sf),
                                                   C.byref(mc), C.byref(ml), float(th),
                                                   int(bMono), int(self.checkOri), _ptr(match),
                                                   C.byref(nm)), "orbm_search_by_projection_last")
        return match[:mc.n].copy(), nm.value

    def SearchByBoW(self, kf_node, kf_valid, kf_desc, kf_angle, f_node, f_desc, f_angle):
        """SearchByBoW(pKF, F) (ORBmatcher.cc:247-410) with per-feature
        vocabulary node ids. Returns (match, nmatches)."""
        keep = [_c(kf_node, np.int32), _c(kf_valid, np.uint8), _c(kf_desc, np.uint8),
                _c(kf_angle, np.float32), _c(f_node, np.int32), _c(f_desc, np.uint8),
                _c(f_angle, np.float32)]
        nf = len(keep[4])
        match = np.zeros(max(1, nf), np.int32)
        nm = C.c_int(0)
        check(lib().orbm_search_by_bow(len(keep[0]), _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]),
                                       _ptr(keep[3]), nf, _ptr(keep[4]), _ptr(keep[5]),
                                       _ptr(keep[6]), float(self.nnratio), int(self.checkOri),
                                       _ptr(match), C.byref(nm)), "orbm_search_by_bow")
        return match[:nf].copy(), nm.value

    def SearchByProjectionLocalMap(self, camera, scale_factors, cur, track, mp_desc, mp_nobs,
                                   cur_nobs, th):
        """SearchByProjection(F, vpLocalMapPoints, th) (ORBmatcher.cc:72-183);
        ``track`` = frame_is_in_frustum output. Returns (match, nmatches)."""
        sf = _c(scale_factors, np.float32)
        keep = []

        def arr(a, dt):
            a = _c(a, dt)
            keep.append(a)
            return _ptr(a)

        n = len(cur["kps_un"])
        mc = MatchCurrent(n, arr(np.eye(4), np.float32), arr(cur["kps_un"], KP_DTYPE),
                          arr(cur["desc"], np.uint8), arr(cur["uright"], np.float32))
        nmp = len(track["in_view"])
        match = np.zeros(max(1, n), np.int32)
        nm = C.c_int(0)
        check(lib().orbm_search_by_projection_local(
            C.byref(camera), _ptr(sf), len(sf), C.byref(mc), nmp, arr(track["in_view"], np.uint8),
            arr(track["proj_x"], np.float32), arr(track["proj_y"], np.float32),
            arr(track["proj_xr"], np.float32), arr(track["level"], np.int32),
            arr(track["view_cos"], np.float32), arr(mp_desc, np.uint8), arr(mp_nobs, np.int32),
            None if cur_nobs is None else arr(cur_nobs, np.int32), float(th), float(self.nnratio),
            _ptr(match), C.byref(nm)), "orbm_search_by_projection_local")
        return match[:n].copy(), nm.value

    def SearchByProjectionKeyFrame(self, camera, scale_factors, cur, cur_has_mp, kf, th, ORBdist):
        """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
        (ORBmatcher.cc:1891-2024), Tracking::Relocalization's matcher.
        ``cur``: dict Tcw, kps_un, desc; ``cur_has_mp[i]``: keypoint i holds a
        map point on entry; ``kf``: dict of per-feature arrays angle, valid
        (map point exists and is not bad), found (in sAlreadyFound), mp_xyz,
        mp_min_dist / mp_max_dist (raw mfMinDistance / mfMaxDistance), mp_desc.
        Returns (match, nmatches): match[i] = keyframe feature index or -1."""
        sf = _c(scale_factors, np.float32)
        keep = []

        def arr(a, dt):
            a = _c(a, dt)
            keep.append(a)
            return _ptr(a)

        n = len(cur["kps_un"])
        nkf = len(kf["angle"])
        mc = MatchCurrent(n, arr(cur["Tcw"], np.float32), arr(cur["kps_un"], KP_DTYPE),
                          arr(cur["desc"], np.uint8), None)
        match = np.zeros(max(1, n), np.int32)
        nm = C.c_int(0)
        check(lib().orbm_search_by_projection_kf(
            C.byref(camera), _ptr(sf), len(sf), C.byref(mc), arr(cur_has_mp, np.uint8), nkf,
            arr(kf["angle"], np.float32), arr(kf["valid"], np.uint8), arr(kf["found"], np.uint8),
            arr(kf["mp_xyz"], np.float32), arr(kf["mp_min_dist"], np.float32),
            arr(kf["mp_max_dist"], np.float32), arr(kf["mp_desc"], np.uint8), float(th),
            int(ORBdist), int(self.checkOri), _ptr(match), C.byref(nm)),
            "orbm_search_by_projection_kf")
        return match[:n].copy(), nm.value

    def SearchBySim3(self, camera, scale_factors, kf1, kf2, matched12, s12, R12, t12, th):
        """SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
        (ORBmatcher.cc:1441-1693). ``kf1`` / ``kf2``: dicts as for
        search_by_sim3_batch. ``matched12`` (int32 [n1], the index in keyframe
        2 of the matched point, -1 none, -2 not observed by keyframe 2) is
        updated in place. Returns nFound; the per-feature record of the call
        is left in ``self.last_sim3``."""
        o = search_by_sim3_batch(camera, scale_factors,
                                 [dict(kf1=kf1, kf2=kf2, matched12=matched12, s12=s12, R12=R12,
                                       t12=t12)], th)[0]
        matched12[...] = o["matched12"]
        self.last_sim3 = o
        return o["n_found"]


def stereo_matches(camera, left, right, kl, dl, kr, dr, frame=0):
    """Frame::ComputeStereoMatches with the pyramids of two ORBextractor
    objects (left / right) that extracted the pair: (uright, depth)."""
    kl = _c(kl, KP_DTYPE)
    kr = _c(kr, KP_DTYPE)
    dl = _c(dl, np.uint8)
    dr = _c(dr, np.uint8)
    ur = np.zeros(max(1, len(kl)), np.float32)
    dp = np.zeros(max(1, len(kl)), np.float32)
    check(lib().orbpl_stereo_matches(C.byref(camera), left._h, right._h, frame, _ptr(kl), _ptr(dl),
                                     len(kl), _ptr(kr), _ptr(dr), len(kr), _ptr(ur), _ptr(dp)),
          "orbpl_stereo_matches")
    return ur[:len(kl)].copy(), dp[:len(kl)].copy()


def frame_is_in_frustum(camera, scale_factor, nlevels, Tcw, mps, view_cos_limit=0.5):
    """Frame::IsInFrustum(MapPoint*, limit) for the map points in ``mps`` (dict:
    xyz, normal, min_dist, max_dist = the raw mfMinDistance / mfMaxDistance; the
    library applies GetMin/MaxDistanceInvariance's 0.8f / 1.2f to the range test
    and PredictScale's mfMaxDistance / dist, MapPoint.cc:387-431). Returns the
    mTrack* fields as a dict."""
    n = len(mps["xyz"])
    keep = [_c(Tcw, np.float32), _c(mps["xyz"], np.float32), _c(mps["normal"], np.float32),
            _c(mps["min_dist"], np.float32), _c(mps["max_dist"], np.float32)]
    out = dict(in_view=np.zeros(n, np.uint8), proj_x=np.zeros(n, np.float32),
               proj_y=np.zeros(n, np.float32), proj_xr=np.zeros(n, np.float32),
               level=np.zeros(n, np.int32), view_cos=np.zeros(n, np.float32))
    check(lib().orbpl_frame_is_in_frustum(
        C.byref(camera), float(scale_factor), int(nlevels), _ptr(keep[0]), n, _ptr(keep[1]),
        _ptr(keep[2]), _ptr(keep[3]), _ptr(keep[4]), float(view_cos_limit), _ptr(out["in_view"]),
        _ptr(out["proj_x"]), _ptr(out["proj_y"]), _ptr(out["proj_xr"]), _ptr(out["level"]),
        _ptr(out["view_cos"])), "orbpl_frame_is_in_frustum")
    return out


def pose_optimization(camera, prob, Tcw, outlier, line_outlier=None, fixed_line_jac=False):
    """Optimizer::PoseOptimization[WithLines] (Optimizer.cc:375-619, 2132-2486).
    ``prob``: dict of arrays. Returns (Tcw, outlier, line_outlier, n_inliers).
    fixed_line_jac: the analytic line Jacobian (ORBPL_POSE_FIXED_LINE_JAC)
    instead of the reference's as-written one (pinned P7)."""
    keep = []

    def arr(a, dt):
        a = _c(a, dt)
        keep.append(a)
        return _ptr(a)

    n = len(prob["kps_un"])
    nl = len(prob.get("kl_obs", ()))
    isg = _c(prob["inv_sigma2"], np.float32)
    P = PoseProblem(n, arr(prob["kps_un"], KP_DTYPE), arr(prob["uright"], np.float32),
                    arr(prob["has_mp"], np.uint8), arr(prob["mp_xyz"], np.float32), nl,
                    arr(prob.get("kl_obs", np.zeros((0, 4))), np.float32),
                    arr(prob.get("kl_octave", np.zeros(0)), np.int32),
                    arr(prob.get("has_ml", np.zeros(0)), np.uint8),
                    arr(prob.get("ml_xyz", np.zeros((0, 6))), np.float32), _ptr(isg), len(isg))
    T = _c(Tcw, np.float32).copy()
    out = _c(outlier, np.uint8).copy()
    lout = _c(line_outlier if line_outlier is not None else np.zeros(nl), np.uint8).copy()
    nin = C.c_int(0)
    check(lib().orbpl_pose_optimization_ex(C.byref(camera), C.byref(P), int(bool(fixed_line_jac)),
                                           _ptr(T), _ptr(out), _ptr(lout), C.byref(nin)),
          "orbpl_pose_optimization_ex")
    return T, out, lout, nin.value


def line_frame_prepare(camera, kl, depth=None):
    """Frame::UndistortKeyLines + line depths (orbpl_line_frame_prepare):
    (kl_un, depth_start, depth_end, uright_start, uright_end)."""
    kl = np.ascontiguousarray(kl, KEYLINE_DTYPE)
    n = len(kl)
    ku = np.zeros(n, KEYLINE_DTYPE)
    ds, de, us, ue = (np.zeros(n, np.float32) for _ in range(4))
    dp = None if depth is None else np.ascontiguousarray(depth, np.float32)
    check(lib().orbpl_line_frame_prepare(C.byref(camera), _ptr(kl), n,
                                         None if dp is None else _ptr(dp), _ptr(ku), _ptr(ds),
                                         _ptr(de), _ptr(us), _ptr(ue)), "orbpl_line_frame_prepare")
    return ku, ds, de, us, ue


class LineMatcher:
    """LineMatcher(0.9, true) tracking overloads on the GPU."""

    @staticmethod
    def SearchByProjectionLocalMap(camera, Tcw, cur_kl_un, cur_desc, cur_nobs, in_view, ml_xyz6,
                                   ml_desc):
        """SearchByProjection(F, vpLocalMapLines): (match, nmatches, wiped)."""
        return _line_search_list(camera, Tcw, cur_kl_un, cur_desc, cur_nobs, in_view, ml_xyz6,
                                 ml_desc)

    @staticmethod
    def SearchByProjectionRefKF(camera, Tcw, cur_kl_un, cur_desc, cur_nobs, has_ml, ml_xyz6,
                                ml_desc):
        """SearchByProjection(F, RefKF): (match, nmatches, wiped)."""
        return _line_search_list(camera, Tcw, cur_kl_un, cur_desc, cur_nobs, has_ml, ml_xyz6,
                                 ml_desc)

    @staticmethod
    def SearchByProjectionLastFrame(camera, Tcw, cur_kl_un, cur_desc, last_kl_un, has_ml, outlier,
                                    ml_xyz6, last_desc):
        keep = [np.ascontiguousarray(Tcw, np.float32), np.ascontiguousarray(cur_kl_un, KEYLINE_DTYPE),
                np.ascontiguousarray(cur_desc, np.uint8),
                np.ascontiguousarray(last_kl_un, KEYLINE_DTYPE), np.ascontiguousarray(has_ml, np.uint8),
                np.ascontiguousarray(outlier, np.uint8), np.ascontiguousarray(ml_xyz6, np.float32),
                np.ascontiguousarray(last_desc, np.uint8)]
        ncur = len(keep[1])
        match = np.zeros(max(1, ncur), np.int32)
        nm = C.c_int(0)
        check(lib().orbl_search_by_projection_last(
            C.byref(camera), _ptr(keep[0]), ncur, _ptr(keep[1]), _ptr(keep[2]), len(keep[3]),
            _ptr(keep[3]), _ptr(keep[4]), _ptr(keep[5]), _ptr(keep[6]), _ptr(keep[7]), _ptr(match),
            C.byref(nm)), "orbl_search_by_projection_last")
        return match[:ncur].copy(), nm.value


    @staticmethod
    def SearchByProjectionPairs(camera, Tcw, mode, cur_kl_un, cur_desc, cur_nobs, valid, base_kl,
                                ml_xyz6, ml_desc, ml_nobs):
        """The reference's harness overloads (orbl_search_by_projection_pairs;
        mode 0 = (Frame&, const Frame&, new_kls, match_indices), 1 = (Frame&,
        const vector<MapLine*>&, new_kls, match_indices)): (match, nmatches,
        wiped, new_kls, their map-line index, match_indices (n, 2))."""
        keep = [np.ascontiguousarray(Tcw, np.float32), np.ascontiguousarray(cur_kl_un, KEYLINE_DTYPE),
                np.ascontiguousarray(cur_desc, np.uint8), np.ascontiguousarray(valid, np.uint8),
                np.ascontiguousarray(ml_xyz6, np.float32), np.ascontiguousarray(ml_desc, np.uint8)]
        cn = None if cur_nobs is None else np.ascontiguousarray(cur_nobs, np.int32)
        mn = None if ml_nobs is None else np.ascontiguousarray(ml_nobs, np.int32)
        bk = None if base_kl is None else np.ascontiguousarray(base_kl, KEYLINE_DTYPE)
        ncur, nml = len(keep[1]), len(keep[3])
        match = np.zeros(max(1, ncur), np.int32)
        pk = np.zeros(max(1, nml), KEYLINE_DTYPE)
        ps = np.zeros(max(1, nml), np.int32)
        cap = max(1, ncur * nml)
        pairs = np.zeros((cap, 2), np.int32)
        nm, wiped, npj, npr = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().orbl_search_by_projection_pairs(
            C.byref(camera), _ptr(keep[0]), mode, ncur, _ptr(keep[1]), _ptr(keep[2]),
            None if cn is None else _ptr(cn), nml, _ptr(keep[3]), None if bk is None else _ptr(bk),
            _ptr(keep[4]), _ptr(keep[5]), None if mn is None else _ptr(mn), _ptr(pk), _ptr(ps),
            C.byref(npj), _ptr(pairs), cap, C.byref(npr), _ptr(match), C.byref(nm),
            C.byref(wiped)), "orbl_search_by_projection_pairs")
        return (match[:ncur].copy(), nm.value, bool(wiped.value), pk[:npj.value].copy(),
                ps[:npj.value].copy(), pairs[:npr.value].copy())

    @staticmethod
    def MatchBFKnn(qdesc, tdesc):
        """SearchByProjection(Frame&, KeyFrame*, vector<MapLine*>&)'s knnMatch
        + 0.75 ratio (orbl_match_bf_knn): (out, nmatches)."""
        q = np.ascontiguousarray(qdesc, np.uint8)
        t = np.ascontiguousarray(tdesc, np.uint8)
        out = np.zeros(max(1, len(t)), np.int32)
        n = C.c_int(0)
        check(lib().orbl_match_bf_knn(len(q), _ptr(q), len(t), _ptr(t), _ptr(out), C.byref(n)),
              "orbl_match_bf_knn")
        return out[:len(t)].copy(), n.value


def line_is_in_frustum(Tcw, ml_xyz6):
    """Frame::IsInFrustum(MapLine*) for n map lines (n x 6 world end points)."""
    T = np.ascontiguousarray(Tcw, np.float32)
    X = np.ascontiguousarray(ml_xyz6, np.float32)
    out = np.zeros(len(X), np.uint8)
    check(lib().orbl_frame_is_in_frustum(_ptr(T), len(X), _ptr(X), _ptr(out)),
          "orbl_frame_is_in_frustum")
    return out


def stereo_line_depths(camera, kl, desc, kr, desc_r):
    """Stereo line end-point depths (orbl_stereo_line_depths):
    (depth_start, depth_end) of the left lines, -1 without a match."""
    kl = np.ascontiguousarray(kl, KEYLINE_DTYPE)
    kr = np.ascontiguousarray(kr, KEYLINE_DTYPE)
    d = np.ascontiguousarray(desc, np.uint8)
    dr = np.ascontiguousarray(desc_r, np.uint8)
    nl = len(kl)
    ds, de = np.zeros(max(1, nl), np.float32), np.zeros(max(1, nl), np.float32)
    check(lib().orbl_stereo_line_depths(C.byref(camera), _ptr(kl), _ptr(d), nl, _ptr(kr), _ptr(dr),
                                        len(kr), _ptr(ds), _ptr(de)), "orbl_stereo_line_depths")
    return ds[:nl].copy(), de[:nl].copy()


def _line_search_list(camera, Tcw, cur_kl_un, cur_desc, cur_nobs, valid, ml_xyz6, ml_desc):
    keep = [np.ascontiguousarray(Tcw, np.float32), np.ascontiguousarray(cur_kl_un, KEYLINE_DTYPE),
            np.ascontiguousarray(cur_desc, np.uint8), np.ascontiguousarray(valid, np.uint8),
            np.ascontiguousarray(ml_xyz6, np.float32), np.ascontiguousarray(ml_desc, np.uint8)]
    cn = None if cur_nobs is None else np.ascontiguousarray(cur_nobs, np.int32)
    ncur = len(keep[1])
    match = np.zeros(max(1, ncur), np.int32)
    nm, wiped = C.c_int(0), C.c_int(0)
    check(lib().orbl_search_by_projection_list(
        C.byref(camera), _ptr(keep[0]), ncur, _ptr(keep[1]), _ptr(keep[2]),
        None if cn is None else _ptr(cn), len(keep[3]), _ptr(keep[3]), _ptr(keep[4]),
        _ptr(keep[5]), _ptr(match), C.byref(nm), C.byref(wiped)), "orbl_search_by_projection_list")
    return match[:ncur].copy(), nm.value, bool(wiped.value)


class Tracker:
    """Batched RGB-D / stereo tracker (orbpl_tracker_*): one
    TrackWithMotionModel step for n_streams independent streams per call.
    lines=True selects the point-and-line variant (ORBPL_TRACK_LINES),
    stereo=True the stereo Frame (ORBPL_TRACK_STEREO); both = the defined
    stereo points+lines mode."""

    TRACK_LINES = 1
    TRACK_STEREO = 2
    TRACK_LOCAL_MAP = 4
    TRACK_FIXED_LINE_JAC = 8
    TRACK_REFKF = 16
    TRACK_MAP = 32

    def __init__(self, orb_params, camera, n_streams, device=0, lines=False, stereo=False,
                 local_map=False, fixed_line_jac=False, refkf=False, map=False):
        h = C.c_void_p()
        self.camera, self.S, self.device, self.use_lines = camera, n_streams, device, bool(lines)
        self.stereo = bool(stereo)
        flags = ((self.TRACK_LINES if lines else 0) | (self.TRACK_STEREO if stereo else 0) |
                 (self.TRACK_LOCAL_MAP if local_map else 0) |
                 (self.TRACK_FIXED_LINE_JAC if fixed_line_jac else 0) |
                 (self.TRACK_REFKF if refkf else 0) | (self.TRACK_MAP if map else 0))
        self.map = bool(map)
        check(lib().orbpl_tracker_create_ex(C.byref(orb_params), C.byref(camera), n_streams, device,
                                            flags, C.byref(h)),
              "orbpl_tracker_create_ex")
        self._h = h
        self.kp_cap = lib().orbpl_tracker_kp_capacity(h)

    def close(self):
        if getattr(self, "_h", None):
            lib().orbpl_tracker_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, Tcw0=None):
        T = None if Tcw0 is None else _c(Tcw0, np.float32)
        check(lib().orbpl_tracker_reset(self._h, None if T is None else _ptr(T)), "reset")

    def clear_velocity(self, mask):
        """mVelocity = cv::Mat() for the streams where mask != 0: their next
        step runs TrackReferenceKeyFrame (orbpl_tracker_clear_velocity)."""
        m = np.ascontiguousarray(np.asarray(mask).astype(np.uint8).reshape(-1))
        if m.size != self.S:
            raise ValueError("clear_velocity: one mask byte per stream")
        check(lib().orbpl_tracker_clear_velocity(self._h, _ptr(m)), "orbpl_tracker_clear_velocity")

    def set_fps(self, fps):
        """Camera.fps of the settings: mMaxFrames (map trackers; 0 -> 30)."""
        check(lib().orbpl_tracker_set_fps(self._h, C.c_float(fps)), "orbpl_tracker_set_fps")

    def step_device(self, d_gray, d_depth):
        check(lib().orbpl_tracker_step(self._h, C.c_void_p(d_gray), C.c_void_p(d_depth)), "step")

    def step_host(self, h_gray, h_depth16, depth_map_factor=5000.0):
        """GrabImageRGBD from host memory: h_gray / h_depth16 = host pointers
        (HostBuffer.ptr) to n_streams u8 frames and u16 depth maps."""
        check(lib().orbpl_tracker_step_host(self._h, C.c_void_p(h_gray), C.c_void_p(h_depth16),
                                            C.c_float(depth_map_factor)), "orbpl_tracker_step_host")

    def step_stereo_device(self, d_left, d_right):
        """Stereo step: device pointers to n_streams left / right frames."""
        check(lib().orbpl_tracker_step_stereo(self._h, C.c_void_p(d_left), C.c_void_p(d_right)),
              "orbpl_tracker_step_stereo")

    def synchronize(self):
        check(lib().orbpl_tracker_synchronize(self._h), "orbpl_tracker_synchronize")

    def set_pipelined(self, on=True):
        """Overlap extraction of step t+1 with tracking of step t (2 streams)."""
        check(lib().orbpl_tracker_set_pipelined(self._h, int(bool(on))), "orbpl_tracker_set_pipelined")

    def state(self):
        S = self.S
        T = np.zeros((S, 4, 4), np.float32)
        nk, nm, ni, nmm = (np.zeros(S, np.int32) for _ in range(4))
        check(lib().orbpl_tracker_get_state(self._h, _ptr(T), _ptr(nk), _ptr(nm), _ptr(ni),
                                            _ptr(nmm)), "orbpl_tracker_get_state")
        return dict(Tcw=T, nkeypoints=nk, nmatches=nm, ninliers=ni, nmatches_map=nmm)

    def status(self):
        """ok, nlines, line_matches, line_nmatches_map per stream (last step)."""
        S = self.S
        ok, nl, lm, lnm = (np.zeros(S, np.int32) for _ in range(4))
        check(lib().orbpl_tracker_get_status(self._h, _ptr(ok), _ptr(nl), _ptr(lm), _ptr(lnm)),
              "orbpl_tracker_get_status")
        return dict(ok=ok, nlines=nl, line_matches=lm, line_nmatches_map=lnm)

    def set_vocabulary(self, voc, levelsup=4):
        """KeyFrame::ComputeBoW of every step's frame with an ORBVocabulary
        (None: off). The tracker keeps a reference so the vocabulary outlives
        its use."""
        check(lib().orbpl_tracker_set_vocabulary(self._h, voc._h if voc is not None else None,
                                                 levelsup), "orbpl_tracker_set_vocabulary")
        self._voc = voc

    def trk(self):
        """Per stream: 1 when the last step ran TrackReferenceKeyFrame."""
        out = np.zeros(self.S, np.int32)
        check(lib().orbpl_tracker_get_trk(self._h, _ptr(out)), "orbpl_tracker_get_trk")
        return out

    def bow(self, stream):
        """The last step's (bow_words, bow_values, feat_node) of one stream."""
        K = self.kp_cap
        w = np.zeros(K, np.uint32)
        v = np.zeros(K, np.float64)
        node = np.zeros(K, np.int32)
        bn, n = C.c_int(0), C.c_int(0)
        check(lib().orbpl_tracker_get_bow(self._h, stream, _ptr(w), _ptr(v), C.byref(bn),
                                          _ptr(node), C.byref(n)), "orbpl_tracker_get_bow")
        return w[:bn.value].copy(), v[:bn.value].copy(), node[:n.value].copy()

    def local_stats(self):
        """TrackLocalMap counts per stream of the last step (local_map=True)."""
        S = self.S
        a, b, c, d = (np.zeros(S, np.int32) for _ in range(4))
        check(lib().orbpl_tracker_get_local_stats(self._h, _ptr(a), _ptr(b), _ptr(c), _ptr(d)),
              "orbpl_tracker_get_local_stats")
        return dict(local_matches=a, local_inliers=b, local_line_matches=c, local_line_inliers=d)

    def lines(self, stream):
        """Undistorted KeyLines, LBD rows, line match, line outlier of one stream."""
        K = 80
        kl = np.zeros(K, KEYLINE_DTYPE)
        d = np.zeros((K, 32), np.uint8)
        m = np.zeros(K, np.int32)
        o = np.zeros(K, np.uint8)
        n = C.c_int(0)
        check(lib().orbpl_tracker_get_lines(self._h, stream, _ptr(kl), _ptr(d), _ptr(m), _ptr(o),
                                            C.byref(n)), "orbpl_tracker_get_lines")
        k = n.value
        return kl[:k], d[:k], m[:k], o[:k]

    LINE_STAGES = ("lsd", "keylines_lbd", "line_match")

    @staticmethod
    def timing_counts():
        """Floats per step of timings / line_timings / lsd_timings /
        stereo_timings as the library writes them (orbpl_tracker_timing_counts)."""
        c = np.zeros(5, np.int32)
        check(lib().orbpl_tracker_timing_counts(_ptr(c)), "orbpl_tracker_timing_counts")
        return tuple(int(x) for x in c)

    def _stage_buf(self, which, names, max_steps):
        k = self.timing_counts()[which]
        if k != len(names):
            raise RuntimeError(f"liborbpl writes {k} timing entries per step, the mirror names "
                               f"{len(names)}: library and package out of step")
        return np.zeros((max_steps, k), np.float32)

    def line_timings(self, max_steps=64):
        """(n_steps, 3) line-stage ms of the last steps (hipEvents in-stream)."""
        ms = self._stage_buf(1, self.LINE_STAGES, max_steps)
        n = C.c_int(0)
        check(lib().orbpl_tracker_line_timings(self._h, max_steps, _ptr(ms), C.byref(n)),
              "orbpl_tracker_line_timings")
        return ms[:n.value]

    LSD_STAGES = ("lsd_prep", "lsd_sort", "lsd_seed", "lsd_validate", "keylines", "lbd",
                  "line_prepare")
    # the kernels each LSD stage event pair brackets
    LSD_KERNELS = {"lsd_prep": "k_lsd_blur+k_lsd_resize+k_lsd_grad",
                   "lsd_sort": "k_lsd_sort+k_lsd_sort_local", "lsd_seed": "k_lsd_spec",
                   "lsd_validate": "k_lsd_validate+k_lsd_compact", "keylines": "k_keylines",
                   "lbd": "k_lsd_blur+k_sobel+k_lbd", "line_prepare": "k_line_prepare"}

    def launch_frames(self):
        """(orb, lsd): frames one extraction / LSD stage launch processes (the
        first half when the tracker splits that batch; lsd 0 without lines)."""
        o, l = C.c_int(0), C.c_int(0)
        check(lib().orbpl_tracker_launch_frames(self._h, C.byref(o), C.byref(l)),
              "orbpl_tracker_launch_frames")
        return o.value, l.value

    def lsd_timings(self, max_steps=64):
        """(n_steps, 7) LSD / LineExtractor kernel ms of the last steps."""
        ms = self._stage_buf(2, self.LSD_STAGES, max_steps)
        n = C.c_int(0)
        check(lib().orbpl_tracker_lsd_timings(self._h, max_steps, _ptr(ms), C.byref(n)),
              "orbpl_tracker_lsd_timings")
        return ms[:n.value]

    def set_history(self, max_steps):
        """Record every stream's pose and counts for the next max_steps steps."""
        check(lib().orbpl_tracker_set_history(self._h, int(max_steps)), "orbpl_tracker_set_history")

    def history(self, stream, max_steps=4096):
        """(Tcw (n,4,4), counts (n,12)) of one stream's recorded steps; counts in
        the oracle's order (nkeypoints, nmatches, ninliers, nmatches_map, ok,
        nlines, line_matches, line_nmatches_map, local_matches, local_inliers,
        local_line_matches, local_line_inliers)."""
        T = np.zeros((max_steps, 4, 4), np.float32)
        cnt = np.zeros((max_steps, 12), np.int32)
        n = C.c_int(0)
        check(lib().orbpl_tracker_get_history(self._h, stream, max_steps, _ptr(T), _ptr(cnt),
                                              C.byref(n)), "orbpl_tracker_get_history")
        return T[:n.value], cnt[:n.value]

    MAP_COUNTS = ("nkeypoints", "nmatches", "ninliers", "nmatches_map", "ok", "nlines",
                  "line_matches", "line_nmatches_map", "local_matches", "local_inliers",
                  "local_line_matches", "local_line_inliers", "keyframe", "keyframes",
                  "map_points", "map_lines", "temporal_points", "trk", "ref_kf", "state",
                  "local_keyframes", "local_points", "local_lines", "temporal_lines")

    def map_history(self, stream, max_steps=4096):
        """(n, 24) counts of one stream's recorded steps (map=True trackers), in
        the order of MAP_COUNTS (the oracle's MapVO.step dictionary)."""
        cnt = np.zeros((max_steps, 24), np.int32)
        n = C.c_int(0)
        check(lib().orbpl_tracker_get_map_history(self._h, stream, max_steps, _ptr(cnt),
                                                  C.byref(n)), "orbpl_tracker_get_map_history")
        return cnt[:n.value]

    def map_errors(self):
        """Per stream: capacity flags since the last reset (1 keyframe table
        full, 2 point / line pool full, 4 local list full); 0 = exact."""
        out = np.zeros(self.S, np.int32)
        check(lib().orbpl_tracker_get_map_errors(self._h, _ptr(out)), "orbpl_tracker_get_map_errors")
        return out

    def map_keyframes(self, stream, cap=64):
        """(parent (n,), [ordered connections per keyframe]) of one stream's map."""
        par = np.zeros(64, np.int32)
        ord_ = np.zeros((64, cap), np.int32)
        nord = np.zeros(64, np.int32)
        n = C.c_int(0)
        check(lib().orbpl_tracker_get_map_keyframes(self._h, stream, _ptr(par), _ptr(ord_), cap,
                                                    _ptr(nord), C.byref(n)),
              "orbpl_tracker_get_map_keyframes")
        k = n.value
        return par[:k].copy(), [ord_[j, :min(nord[j], cap)].copy() for j in range(k)]

    def map_points(self, stream, cap=1 << 17):
        """dict(nobs, desc, xyz, normal, dist) of one stream's map points."""
        nobs = np.zeros(cap, np.int32)
        desc = np.zeros((cap, 32), np.uint8)
        xyz = np.zeros((cap, 3), np.float32)
        nrm = np.zeros((cap, 3), np.float32)
        d2 = np.zeros((cap, 2), np.float32)
        n = C.c_int(0)
        check(lib().orbpl_tracker_get_map_points(self._h, stream, cap, _ptr(nobs), _ptr(desc),
                                                 _ptr(xyz), _ptr(nrm), _ptr(d2), C.byref(n)),
              "orbpl_tracker_get_map_points")
        k = min(n.value, cap)
        return dict(nobs=nobs[:k], desc=desc[:k], xyz=xyz[:k], normal=nrm[:k], dist=d2[:k])

    def map_lines(self, stream, cap=1 << 14):
        """dict(nobs, desc, pos) of one stream's map lines."""
        nobs = np.zeros(cap, np.int32)
        desc = np.zeros((cap, 32), np.uint8)
        pos = np.zeros((cap, 6), np.float32)
        n = C.c_int(0)
        check(lib().orbpl_tracker_get_map_lines(self._h, stream, cap, _ptr(nobs), _ptr(desc),
                                                _ptr(pos), C.byref(n)), "orbpl_tracker_get_map_lines")
        k = min(n.value, cap)
        return dict(nobs=nobs[:k], desc=desc[:k], pos=pos[:k])

    STEREO_STAGES = ("right_extract", "stereo_match", "right_lines", "stereo_lines")

    def stereo_timings(self, max_steps=64):
        """(n_steps, 4) stereo-stage ms of the last steps (hipEvents in-stream);
        the line stages are 0 without lines."""
        ms = self._stage_buf(3, self.STEREO_STAGES, max_steps)
        n = C.c_int(0)
        check(lib().orbpl_tracker_stereo_timings(self._h, max_steps, _ptr(ms), C.byref(n)),
              "orbpl_tracker_stereo_timings")
        return ms[:n.value]

    def stage_ms(self):
        ms = np.zeros(5, np.float32)
        check(lib().orbpl_tracker_stage_ms(self._h, _ptr(ms)), "orbpl_tracker_stage_ms")
        return ms

    STAGES = ("pyramid", "blur", "fast", "octree", "orient_desc", "glue", "match", "pose",
              "finish", "local_map", "bow")

    def timings(self, max_steps=64):
        """(n_steps, 11) per-kernel ms of the last steps (hipEvents in-stream)."""
        ms = self._stage_buf(0, self.STAGES, max_steps)
        n = C.c_int(0)
        check(lib().orbpl_tracker_timings(self._h, max_steps, _ptr(ms), C.byref(n)),
              "orbpl_tracker_timings")
        return ms[:n.value]

    KERNEL_STAGES = ("pose_motion", "pose_refkf", "pose_local", "match_local")

    def kernel_timings(self, max_steps=64):
        """(n_steps, 4) ms of every k_pose launch (motion model, reference
        keyframe, local map) and of k_match_local, each launch alone."""
        ms = self._stage_buf(4, self.KERNEL_STAGES, max_steps)
        n = C.c_int(0)
        check(lib().orbpl_tracker_kernel_timings(self._h, max_steps, _ptr(ms), C.byref(n)),
              "orbpl_tracker_kernel_timings")
        return ms[:n.value]

    def timings_reset(self):
        check(lib().orbpl_tracker_timings_reset(self._h), "orbpl_tracker_timings_reset")

    def frame(self, stream):
        K = self.kp_cap
        ku = np.zeros(K, KP_DTYPE)
        d = np.zeros((K, 32), np.uint8)
        m = np.zeros(K, np.int32)
        o = np.zeros(K, np.uint8)
        n = C.c_int(0)
        check(lib().orbpl_tracker_get_frame(self._h, stream, _ptr(ku), _ptr(d), _ptr(m), _ptr(o),
                                            C.byref(n)), "orbpl_tracker_get_frame")
        k = n.value
        return ku[:k], d[:k], m[:k], o[:k]


# ---------------------------------------------------------------------------
# Line features: LineExtractor::ExtractLineSegment (LineExtractor.cpp:12-74)
# ---------------------------------------------------------------------------
KEYLINE_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"),
                          ("pt_x", "<f4"), ("pt_y", "<f4"), ("response", "<f4"), ("size", "<f4"),
                          ("startPointX", "<f4"), ("startPointY", "<f4"), ("endPointX", "<f4"),
                          ("endPointY", "<f4"), ("sPointInOctaveX", "<f4"),
                          ("sPointInOctaveY", "<f4"), ("ePointInOctaveX", "<f4"),
                          ("ePointInOctaveY", "<f4"), ("lineLength", "<f4"),
                          ("numOfPixels", "<i4")])


def _declare_lines(L):
    vp, i, ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
    L.lsdx_create.argtypes = [i, i, i, i, C.POINTER(vp)]
    L.lsdx_destroy.argtypes = [vp]
    L.lsdx_describe.argtypes = [i, i, ip, ip, ip]
    L.lsdx_detect.argtypes = [vp, vp, i, i, i, vp, i, ip]
    L.lsdx_detect_batch_device.argtypes = [vp, vp, i, i, C.c_int64]
    L.lsdx_synchronize.argtypes = [vp]
    L.lsdx_get_lines.argtypes = [vp, i, vp, i, ip]
    L.lsdx_get_stages.argtypes = [vp, i, vp, vp, vp, ip, ip, ip]
    L.orbpl_test_introsort.argtypes = [vp, i, vp]
    L.lsdx_debug_profile.argtypes = [vp, vp]
    L.lsdx_set_serial_grow.argtypes = [vp, i]
    L.lsdx_extract.argtypes = [vp, vp, i, i, i, vp, vp, vp, i, ip]
    L.lsdx_extract_batch_device.argtypes = [vp, vp, i, i, C.c_int64]
    L.lsdx_get_keylines.argtypes = [vp, i, vp, vp, vp, i, ip]
    L.lsdx_device_outputs.argtypes = [vp, vp, vp, vp, vp]


def lsd_describe(width, height):
    """Device-free geometry of a line detector: the 0.8-scaled size and the
    smallest region that is fitted."""
    sw, sh, mr = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib().lsdx_describe(width, height, C.byref(sw), C.byref(sh), C.byref(mr)),
          "lsdx_describe")
    return dict(sw=sw.value, sh=sh.value, min_reg_size=mr.value)


class LineSegmentDetector:
    """cv::LineSegmentDetector(LSD_REFINE_ADV) as LSDDetector::detect(img, kl, 1, 1)
    runs it (LineExtractor.cpp:20-21): 0.8 Gaussian sub-sampling, region
    growing, rectangle refinement, NFA validation. detect() returns the
    segments (x1, y1, x2, y2) in detection order."""

    def __init__(self, width, height, max_batch=1, device=0):
        self.W, self.H, self.max_batch, self.device = width, height, max_batch, device
        h = C.c_void_p()
        check(lib().lsdx_create(width, height, max_batch, device, C.byref(h)), "lsdx_create")
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().lsdx_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def detect(self, img, cap=4096):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        out = np.zeros((cap, 4), np.float32)
        n = C.c_int(0)
        check(lib().lsdx_detect(self._h, _ptr(img), w, h, w, _ptr(out), cap, C.byref(n)),
              "lsdx_detect")
        return out[:n.value].copy()

    def detect_batch_device(self, d_imgs, batch, stride=None, frame_pitch=None):
        stride = self.W if stride is None else stride
        frame_pitch = self.W * self.H if frame_pitch is None else frame_pitch
        check(lib().lsdx_detect_batch_device(self._h, C.c_void_p(d_imgs), batch, stride,
                                             frame_pitch), "lsdx_detect_batch_device")

    def synchronize(self):
        check(lib().lsdx_synchronize(self._h), "lsdx_synchronize")

    def lines(self, frame, cap=4096):
        out = np.zeros((cap, 4), np.float32)
        n = C.c_int(0)
        check(lib().lsdx_get_lines(self._h, frame, _ptr(out), cap, C.byref(n)), "lsdx_get_lines")
        return out[:n.value].copy()

    def set_serial_grow(self, on=True):
        """Wave-serial seed loop (restatement order) instead of the
        speculative lane-parallel one; identical lines."""
        check(lib().lsdx_set_serial_grow(self._h, int(bool(on))), "lsdx_set_serial_grow")

    def debug_profile(self):
        out = np.zeros(8, np.int64)
        check(lib().lsdx_debug_profile(self._h, _ptr(out)), "lsdx_debug_profile")
        keys = ("grow_cyc", "rounds", "spec_regions", "total_cyc", "fit_cyc", "validate_commit_cyc",
                "max_steps", "candidates")
        d = dict(zip(keys, out.tolist()))
        d["coop_regions"] = d["max_steps"] >> 40
        d["max_steps"] &= (1 << 40) - 1
        return d

    def stages(self, frame=0):
        sw, sh = int(round(self.W * 0.8)), int(round(self.H * 0.8))
        scaled = np.zeros((sh, sw), np.uint8)
        deg = np.zeros((sh, sw), np.float32)
        order = np.zeros((sw - 1) * (sh - 1), np.uint32)
        a, b, n = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().lsdx_get_stages(self._h, frame, _ptr(scaled), _ptr(deg), _ptr(order),
                                    C.byref(a), C.byref(b), C.byref(n)), "lsdx_get_stages")
        return scaled, deg, order[:n.value]


def test_introsort(keys):
    """Device replica of std::sort(records, key greater): record order."""
    k = np.ascontiguousarray(keys, np.int32)
    perm = np.zeros(len(k), np.int32)
    check(lib().orbpl_test_introsort(_ptr(k), len(k), _ptr(perm)), "orbpl_test_introsort")
    return perm


class LineExtractor(LineSegmentDetector):
    """ORB_SLAM2::LineExtractor (include/LineExtractor.h:21-56):
    ExtractLineSegment(img) -> (key_lines, line_descriptor, keyline_coefficients)
    with scale = 1, num_octaves = 1 as Frame::ExtractLine calls it (Frame.cc:326-328)."""

    def ExtractLineSegment(self, img):
        img, stride = _rows_u8(img)
        h, w = img.shape
        kl = np.zeros(80, KEYLINE_DTYPE)
        desc = np.zeros((80, 32), np.uint8)
        coef = np.zeros((80, 3), np.float64)
        n = C.c_int(0)
        check(lib().lsdx_extract(self._h, _ptr(img), w, h, stride, _ptr(kl), _ptr(desc), _ptr(coef),
                                 80, C.byref(n)), "lsdx_extract")
        k = n.value
        return kl[:k].copy(), desc[:k].copy(), coef[:k].copy()

    def extract_batch_device(self, d_imgs, batch, stride=None, frame_pitch=None):
        stride = self.W if stride is None else stride
        frame_pitch = self.W * self.H if frame_pitch is None else frame_pitch
        check(lib().lsdx_extract_batch_device(self._h, C.c_void_p(d_imgs), batch, stride,
                                              frame_pitch), "lsdx_extract_batch_device")

    def keylines(self, frame):
        kl = np.zeros(80, KEYLINE_DTYPE)
        desc = np.zeros((80, 32), np.uint8)
        coef = np.zeros((80, 3), np.float64)
        n = C.c_int(0)
        check(lib().lsdx_get_keylines(self._h, frame, _ptr(kl), _ptr(desc), _ptr(coef), 80,
                                      C.byref(n)), "lsdx_get_keylines")
        k = n.value
        return kl[:k].copy(), desc[:k].copy(), coef[:k].copy()


# ---------------------------------------------------------------------------
# DBoW2 ORB vocabulary (ORBVocabulary, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h)
# ---------------------------------------------------------------------------
def _declare_voc(L):
    vp, i, ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
    L.orbv_load_text.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.orbv_create.argtypes = [i, i, i, i, i, vp, vp, vp, vp, C.POINTER(vp)]
    L.orbv_destroy.argtypes = [vp]
    L.orbv_info.argtypes = [vp, vp]
    L.orbv_export.argtypes = [vp, vp, vp, vp, vp]
    L.orbv_upload.argtypes = [vp, i]
    L.orbv_transform.argtypes = [vp, i, vp, i, i, vp, vp, ip, vp]
    L.orbv_transform_batch_device.argtypes = [vp, vp, C.c_int64, vp, i, i, i, vp, vp, vp, vp, vp,
                                              vp, C.c_int64, vp, vp]


class ORBVocabulary:
    """TemplatedVocabulary<FORB::TDescriptor, FORB>: loadFromTextFile (host),
    transform on the GPU. Construct with `path` (the reference's text format)
    or `arrays` (dict from to_arrays(): parent, leaf, desc, weight, k, L,
    scoring, weighting) - e.g. a rank's copy of rank 0's broadcast."""

    def __init__(self, path=None, arrays=None, device=0):
        h = C.c_void_p()
        if path is not None:
            check(lib().orbv_load_text(str(path).encode(), C.byref(h)), "orbv_load_text")
        else:
            a = arrays
            par = _c(a["parent"], np.int32)
            leaf = _c(a["leaf"], np.uint8)
            desc = _c(a["desc"], np.uint8)
            wt = _c(a["weight"], np.float64)
            check(lib().orbv_create(int(a["k"]), int(a["L"]), int(a["scoring"]),
                                    int(a["weighting"]), len(par), _ptr(par), _ptr(leaf),
                                    _ptr(desc), _ptr(wt), C.byref(h)), "orbv_create")
        self._h = h
        self.device = device
        info = np.zeros(6, np.int32)
        check(lib().orbv_info(self._h, _ptr(info)), "orbv_info")
        self.k, self.L, self.scoring, self.weighting, self.n_nodes, self.n_words = map(int, info)

    @classmethod
    def loadFromTextFile(cls, path, device=0):
        return cls(path=path, device=device)

    def to_arrays(self):
        n = self.n_nodes
        a = dict(parent=np.zeros(n, np.int32), leaf=np.zeros(n, np.uint8),
                 desc=np.zeros((n, 32), np.uint8), weight=np.zeros(n, np.float64))
        check(lib().orbv_export(self._h, _ptr(a["parent"]), _ptr(a["leaf"]), _ptr(a["desc"]),
                                _ptr(a["weight"])), "orbv_export")
        a.update(k=self.k, L=self.L, scoring=self.scoring, weighting=self.weighting)
        return a

    def upload(self):
        check(lib().orbv_upload(self._h, self.device), "orbv_upload")

    def transform(self, desc, levelsup=4):
        """-> (bow_words u32, bow_values f64, feat_node i32 per feature, -1 = stopped)"""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        words = np.zeros(max(1, n), np.uint32)
        vals = np.zeros(max(1, n), np.float64)
        node = np.zeros(max(1, n), np.int32)
        bn = C.c_int(0)
        check(lib().orbv_transform(self._h, self.device, _ptr(desc), n, levelsup, _ptr(words),
                                   _ptr(vals), C.byref(bn), _ptr(node)), "orbv_transform")
        k = bn.value
        return words[:k].copy(), vals[:k].copy(), node[:n].copy()

    def transform_batch_device(self, d_desc, desc_pitch, d_n, nframes, max_n, levelsup, out,
                               stream=None):
        """out: dict of DeviceBuffers feat_node, feat_word, feat_weight,
        bow_words, bow_vals, bow_n, err (pitch out['pitch'])."""
        check(lib().orbv_transform_batch_device(
            self._h, C.c_void_p(d_desc), desc_pitch, C.c_void_p(d_n), nframes, max_n, levelsup,
            C.c_void_p(out["feat_node"].ptr), C.c_void_p(out["feat_word"].ptr),
            C.c_void_p(out["feat_weight"].ptr), C.c_void_p(out["bow_words"].ptr),
            C.c_void_p(out["bow_vals"].ptr), C.c_void_p(out["bow_n"].ptr), out["pitch"],
            C.c_void_p(out["err"].ptr), None if stream is None else C.c_void_p(stream)),
            "orbv_transform_batch_device")

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.orbv_destroy(self._h)
            self._h = None


# ---------------------------------------------------------------------------
# KeyFrameDatabase::DetectRelocalizationCandidates (KeyFrameDatabase.cc:274-412)
# ---------------------------------------------------------------------------
KFDB_MAX_KEYFRAMES = 64
KFDB_MAX_WORDS = 4096
KFDB_COVISIBLES = 10


class KfdbProblem(C.Structure):
    _fields_ = [("nkf", C.c_int32), ("kf_off", C.c_void_p), ("kf_words", C.c_void_p),
                ("kf_vals", C.c_void_p), ("covis", C.c_void_p), ("reloc_score", C.c_void_p),
                ("nq_words", C.c_int32), ("q_words", C.c_void_p), ("q_vals", C.c_void_p),
                ("cand", C.c_void_p), ("ncand", C.c_void_p), ("common_words", C.c_void_p)]


class KfdbDeviceBatch(C.Structure):
    _fields_ = [("d_nkf", C.c_void_p), ("d_kf_off", C.c_void_p), ("d_kf_words", C.c_void_p),
                ("d_kf_vals", C.c_void_p), ("ent_pitch", C.c_int64), ("d_covis", C.c_void_p),
                ("d_reloc_score", C.c_void_p), ("d_q_n", C.c_void_p), ("d_q_words", C.c_void_p),
                ("d_q_vals", C.c_void_p), ("q_pitch", C.c_int64), ("d_cand", C.c_void_p),
                ("d_ncand", C.c_void_p), ("d_common_words", C.c_void_p)]


class MatchKfDeviceBatch(C.Structure):
    _fields_ = [("kp_pitch", C.c_int32), ("d_cur_n", C.c_void_p), ("d_Tcw", C.c_void_p),
                ("d_cur_kps_un", C.c_void_p), ("d_cur_desc", C.c_void_p),
                ("d_cur_has_mp", C.c_void_p), ("kf_pitch", C.c_int32), ("d_kf_n", C.c_void_p),
                ("d_kf_angle", C.c_void_p), ("d_kf_valid", C.c_void_p), ("d_kf_found", C.c_void_p),
                ("d_mp_xyz", C.c_void_p), ("d_mp_min_dist", C.c_void_p),
                ("d_mp_max_dist", C.c_void_p), ("d_mp_desc", C.c_void_p), ("d_match", C.c_void_p),
                ("d_nmatches", C.c_void_p)]


def detect_reloc_batch(problems, scoring=0):
    """DetectRelocalizationCandidates for a list of independent (database,
    query) problems in one launch. Each problem is a dict: ``kf_bows`` = the
    database's BowVectors [(words u32 ascending, values f64), ...] in add()
    order, ``covis`` = per keyframe the database indices of
    GetBestCovisibilityKeyFrames(10) (-1 or missing: none), ``reloc_score`` =
    mRelocScore per keyframe (float32, persistent state), ``q_words`` /
    ``q_vals`` = the query's BowVector. Returns per problem a dict: ``cand``
    (database indices in the reference's order), ``common_words``
    (mnRelocWords), ``reloc_score`` (updated copy)."""
    nq = len(problems)
    arr = (KfdbProblem * max(1, nq))()
    keep, outs = [], []
    for p, pr in enumerate(problems):
        bows = pr["kf_bows"]
        nkf = len(bows)
        off = np.zeros(nkf + 1, np.int32)
        for k, (w, _) in enumerate(bows):
            off[k + 1] = off[k] + len(w)
        kw = (np.concatenate([_c(w, np.uint32) for w, _ in bows]) if nkf
              else np.zeros(0, np.uint32))
        kv = (np.concatenate([_c(v, np.float64) for _, v in bows]) if nkf
              else np.zeros(0, np.float64))
        kw, kv = _c(kw, np.uint32), _c(kv, np.float64)
        cov = np.full((max(1, nkf), KFDB_COVISIBLES), -1, np.int32)
        for k, lst in enumerate(pr.get("covis", [])[:nkf]):
            lst = list(lst)[:KFDB_COVISIBLES]
            cov[k, :len(lst)] = lst
        rs = np.zeros(max(1, nkf), np.float32)
        if pr.get("reloc_score") is not None:
            rs[:nkf] = _c(pr["reloc_score"], np.float32)
        qw, qv = _c(pr["q_words"], np.uint32), _c(pr["q_vals"], np.float64)
        cand = np.zeros(KFDB_MAX_KEYFRAMES, np.int32)
        nc = np.zeros(1, np.int32)
        cw = np.zeros(max(1, nkf), np.int32)
        keep += [off, kw, kv, cov, rs, qw, qv, cand, nc, cw]
        arr[p] = KfdbProblem(nkf, _ptr(off), _ptr(kw), _ptr(kv), _ptr(cov), _ptr(rs), len(qw),
                             _ptr(qw), _ptr(qv), _ptr(cand), _ptr(nc), _ptr(cw))
        outs.append((nkf, cand, nc, cw, rs))
    check(lib().orbkf_detect_reloc(C.byref(arr), nq, int(scoring)), "orbkf_detect_reloc")
    return [dict(cand=cand[:int(nc[0])].copy(), common_words=cw[:nkf].copy(),
                 reloc_score=rs[:nkf].copy()) for nkf, cand, nc, cw, rs in outs]


class KeyFrameDatabase:
    """ORB_SLAM2::KeyFrameDatabase reduced to relocalisation: the keyframes'
    BowVectors in add() order, their ordered covisibles and the persistent
    mRelocScore (starts at 0.0f). Keyframes are named by the
    index add() returned; erase() leaves the other indices unchanged."""

    def __init__(self, scoring=0):
        self.scoring = scoring
        self.clear()

    def clear(self):
        self._bows, self._covis, self._score, self._alive = [], [], [], []

    def add(self, bow_words, bow_vals):
        self._bows.append((_c(bow_words, np.uint32).copy(), _c(bow_vals, np.float64).copy()))
        self._covis.append([])
        self._score.append(np.float32(0.0))
        self._alive.append(True)
        return len(self._bows) - 1

    def erase(self, idx):
        self._alive[idx] = False

    def set_covisibles(self, idx, covisibles):
        """GetBestCovisibilityKeyFrames(10) of keyframe idx, as add() indices"""
        self._covis[idx] = [int(k) for k in covisibles][:KFDB_COVISIBLES]

    def reloc_score(self, idx):
        return self._score[idx]

    def DetectRelocalizationCandidates(self, bow_words, bow_vals):
        live = [k for k, a in enumerate(self._alive) if a]
        pos = {k: j for j, k in enumerate(live)}
        pr = dict(kf_bows=[self._bows[k] for k in live],
                  covis=[[pos.get(c, -1) for c in self._covis[k]] for k in live],
                  reloc_score=np.array([self._score[k] for k in live], np.float32),
                  q_words=bow_words, q_vals=bow_vals)
        out = detect_reloc_batch([pr], self.scoring)[0]
        for j, k in enumerate(live):
            self._score[k] = out["reloc_score"][j]
        self.last_common_words = {k: int(out["common_words"][j]) for j, k in enumerate(live)}
        return [live[j] for j in out["cand"]]


# ---------------------------------------------------------------------------
# PnPsolver (PnPsolver.cc)
# ---------------------------------------------------------------------------
PNP_MAX_POINTS = 2048
PNP_MAX_ITERATIONS = 320
PNP_RAND_MAX = 2147483647


class PnpProblem(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("n", C.c_int32), ("p2d", C.c_void_p), ("sigma2", C.c_void_p),
                ("p3d", C.c_void_p), ("min_inliers", C.c_int32), ("max_its", C.c_int32),
                ("max_error", C.c_void_p), ("n_draws", C.c_int32), ("draws", C.c_void_p),
                ("iterations", C.c_void_p), ("best_inliers", C.c_void_p),
                ("best_mask", C.c_void_p), ("best_Tcw", C.c_void_p), ("Tcw", C.c_void_p),
                ("result", C.c_void_p), ("no_more", C.c_void_p), ("n_inliers", C.c_void_p),
                ("inliers", C.c_void_p), ("draws_consumed", C.c_void_p)]


class PnpDeviceBatch(C.Structure):
    _fields_ = [("d_n", C.c_void_p), ("d_cam", C.c_void_p), ("d_p2d", C.c_void_p),
                ("d_p3d", C.c_void_p), ("d_max_error", C.c_void_p), ("pt_pitch", C.c_int32),
                ("d_min_inliers", C.c_void_p), ("d_max_its", C.c_void_p),
                ("d_draws", C.c_void_p), ("draw_pitch", C.c_int32),
                ("d_iterations", C.c_void_p), ("d_best_inliers", C.c_void_p),
                ("d_best_mask", C.c_void_p), ("d_best_Tcw", C.c_void_p), ("d_Tcw", C.c_void_p),
                ("d_result", C.c_void_p), ("d_no_more", C.c_void_p),
                ("d_n_inliers", C.c_void_p), ("d_inliers", C.c_void_p),
                ("d_draws_consumed", C.c_void_p)]


def pnp_ransac_parameters(N, probability=0.99, minInliers=8, maxIterations=300, minSet=4,
                          epsilon=0.4, th2=5.991, sigma2=None):
    """PnPsolver::SetRansacParameters (:121-157) on the host, with the
    platform's log / pow. Returns (min_inliers, max_its, epsilon, max_error):
    the adjusted parameters and mvMaxError (None without sigma2)."""
    import math
    f32 = np.float32
    eps = f32(epsilon)
    with np.errstate(all="ignore"):
        n_min = int(f32(N) * eps)
        if n_min < minInliers:
            n_min = minInliers
        if n_min < minSet:
            n_min = minSet
        ratio = f32(n_min) / f32(N)
        if eps < ratio:
            eps = ratio
    if n_min == N:
        n_it = 1
    else:
        try:
            v = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3)))
        except (ValueError, ZeroDivisionError, OverflowError):
            v = None      # not a finite int: INT_MIN, as the C library pins it
        n_it = v if (v is not None and -2 ** 31 <= v < 2 ** 31) else -2 ** 31
    max_its = max(1, min(n_it, maxIterations))
    max_error = None
    if sigma2 is not None:
        max_error = _c(sigma2, f32) * f32(th2)
    return n_min, max_its, f32(eps), max_error


def pnp_hypotheses(n, min_inliers, max_its, iterations, n_iterations):
    """hypotheses iterate(n_iterations) runs at most from this state: a call
    needs 4 draws for each"""
    if n < min_inliers:
        return 0
    return max(0, max_its - iterations, n_iterations)


def pnp_new_state(n):
    return dict(iterations=0, best_inliers=0, best_mask=np.zeros(n, np.uint8),
                best_Tcw=np.zeros((4, 4), np.float32))


def pnp_iterate_batch(problems, n_iterations):
    """PnPsolver::iterate(n_iterations) for a list of independent solvers in
    one launch. Each problem is a dict: ``cam`` = (fx, fy, cx, cy), ``p2d``
    [n, 2], ``p3d`` [n, 3], ``max_error`` [n] (float32), ``min_inliers``,
    ``max_its`` (adjusted, see pnp_ransac_parameters), ``draws`` = raw rand()
    values, 4 per hypothesis the call may run (pnp_hypotheses), ``state`` =
    the dict the previous call returned (missing or None: a new solver).
    Returns per problem a dict: ``result`` (0 empty, 1 refined, 2 best at
    exhaustion), ``no_more``, ``n_inliers``, ``inliers`` bool[n], ``Tcw``
    float32[4, 4], ``draws_consumed``, ``state``."""
    ns = len(problems)
    arr = (PnpProblem * max(1, ns))()
    keep, outs = [], []
    f32, i32 = np.float32, np.int32
    for p, pr in enumerate(problems):
        p2 = _c(pr["p2d"], f32).reshape(-1, 2)
        p3 = _c(pr["p3d"], f32).reshape(-1, 3)
        n = len(p2)
        me = _c(pr["max_error"], f32).reshape(-1)
        if len(p3) != n or len(me) != n:
            raise OrbplError("p2d, p3d and max_error differ in length")
        dr = _c(pr["draws"], i32).reshape(-1)
        st = pr.get("state") or pnp_new_state(n)
        it = np.array([st["iterations"]], i32)
        bi = np.array([st["best_inliers"]], i32)
        bm = _c(st["best_mask"], np.uint8).copy()
        bT = _c(st["best_Tcw"], f32).reshape(16).copy()
        if len(bm) != n:
            raise OrbplError("state belongs to another problem")
        T = np.zeros(16, f32)
        res, nm, ni, dc = (np.zeros(1, i32) for _ in range(4))
        inl = np.zeros(max(1, n), np.uint8)
        cam = [float(c) for c in pr["cam"]]
        keep += [p2, p3, me, dr, it, bi, bm, bT, T, res, nm, ni, dc, inl]
        arr[p] = PnpProblem(cam[0], cam[1], cam[2], cam[3], n, _ptr(p2), None, _ptr(p3),
                            int(pr["min_inliers"]), int(pr["max_its"]), _ptr(me), len(dr),
                            _ptr(dr), _ptr(it), _ptr(bi), _ptr(bm), _ptr(bT), _ptr(T), _ptr(res),
                            _ptr(nm), _ptr(ni), _ptr(inl), _ptr(dc))
        outs.append((n, it, bi, bm, bT, T, res, nm, ni, dc, inl))
    check(lib().orbpnp_iterate(C.byref(arr), ns, int(n_iterations)), "orbpnp_iterate")
    return [dict(result=int(res[0]), no_more=bool(nm[0]), n_inliers=int(ni[0]),
                 inliers=inl[:n].astype(bool), Tcw=T.reshape(4, 4).copy(),
                 draws_consumed=int(dc[0]),
                 state=dict(iterations=int(it[0]), best_inliers=int(bi[0]), best_mask=bm,
                            best_Tcw=bT.reshape(4, 4)))
            for n, it, bi, bm, bT, T, res, nm, ni, dc, inl in outs]


# rand() is process-wide in the reference; so is the look-ahead queue (P29): a
# call is handed 4 draws per hypothesis it may run, the ones it did not consume
# stay queued and go to the next call, of whichever solver.
_pnp_rand_queue = []
_libc = None


def _pnp_libc():
    global _libc
    if _libc is None:
        _libc = C.CDLL(None)
        _libc.rand.restype = C.c_int
    return _libc


def pnp_srand(seed):
    """srand(seed) of the C library, dropping the draws queued before it"""
    _pnp_libc().srand(C.c_uint(seed))
    del _pnp_rand_queue[:]


def _pnp_take_rand(count):
    _pnp_libc()
    while len(_pnp_rand_queue) < count:
        _pnp_rand_queue.append(_libc.rand())
    return np.array(_pnp_rand_queue[:count], np.int32)


class PnPsolver:
    """ORB_SLAM2::PnPsolver(F, vpMapPointMatches) (:67-110): ``cam`` = (fx, fy,
    cx, cy) or a camera with those fields, ``kps_un_xy`` [n, 2] = F.mvKeysUn's
    points, ``level_sigma2_per_keypoint`` [n] = F.mvLevelSigma2[kp.octave],
    ``mp_xyz`` [n, 3] = the matched map points' world positions, ``mp_valid``
    [n] = the match exists and is not bad. The correspondences are the valid
    keypoints in index order (mvKeyPointIndices)."""

    def __init__(self, cam, kps_un_xy, level_sigma2_per_keypoint, mp_xyz, mp_valid):
        if hasattr(cam, "fx"):
            cam = (cam.fx, cam.fy, cam.cx, cam.cy)
        self.cam = tuple(float(np.float32(c)) for c in cam)
        valid = np.asarray(mp_valid).astype(bool).reshape(-1)
        self.n_keypoints = len(valid)
        self.mvKeyPointIndices = np.flatnonzero(valid)
        self.p2d = _c(np.asarray(kps_un_xy, np.float32).reshape(-1, 2)[valid], np.float32)
        self.sigma2 = _c(np.asarray(level_sigma2_per_keypoint, np.float32).reshape(-1)[valid],
                         np.float32)
        self.p3d = _c(np.asarray(mp_xyz, np.float32).reshape(-1, 3)[valid], np.float32)
        self.N = len(self.p2d)
        if self.N > PNP_MAX_POINTS:
            raise OrbplError(f"more than {PNP_MAX_POINTS} correspondences")
        self.state = pnp_new_state(self.N)
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4,
                            epsilon=0.4, th2=5.991):
        if minSet != 4:
            raise OrbplError("only minSet = 4 is built")
        self.min_inliers, self.max_its, self.epsilon, self.max_error = pnp_ransac_parameters(
            self.N, probability, minInliers, maxIterations, minSet, epsilon, th2, self.sigma2)

    def iterate(self, nIterations, draws=None):
        """Returns (Tcw float32[4, 4] or None, bNoMore, vbInliers bool per
        keypoint, nInliers). ``draws`` = raw rand() values for this call (4 per
        hypothesis it may run); None takes them from the C library's rand()
        through the process-wide look-ahead queue."""
        need = 4 * pnp_hypotheses(self.N, self.min_inliers, self.max_its,
                                  self.state["iterations"], nIterations)
        own = draws is None
        d = _pnp_take_rand(need) if own else _c(draws, np.int32)
        o = pnp_iterate_batch([dict(cam=self.cam, p2d=self.p2d, p3d=self.p3d,
                                    max_error=self.max_error, min_inliers=self.min_inliers,
                                    max_its=self.max_its, draws=d, state=self.state)],
                              nIterations)[0]
        if own:
            del _pnp_rand_queue[:o["draws_consumed"]]
        self.state = o["state"]
        self.last = o
        vb = np.zeros(self.n_keypoints, bool)
        if o["result"]:
            vb[self.mvKeyPointIndices[o["inliers"]]] = True
        return (o["Tcw"] if o["result"] else None), o["no_more"], vb, o["n_inliers"]

    def find(self):
        """(Tcw or None, vbInliers, nInliers)"""
        T, _, vb, n = self.iterate(self.max_its)
        return T, vb, n


_PNP_COLS = (_cols("n min_inliers max_its iterations best_inliers", np.int32) +
             _cols("cam", np.float32, (4,)) + _cols("best_Tcw", np.float32, (16,)) +
             _cols("p2d", np.float32, (2,), "pt") + _cols("p3d", np.float32, (3,), "pt") +
             _cols("max_error", np.float32, (), "pt") + _cols("best_mask", np.uint8, (), "pt") +
             _cols("draws", np.int32, (), "draw") +
             # out
             _cols("result no_more n_inliers draws_consumed", np.int32) +
             _cols("Tcw", np.float32, (16,)) + _cols("inliers", np.uint8, (), "pt"))


class PnpDeviceProblems(PitchedProblems):
    """The pitched device arrays of orbpnp_iterate_batch_device for a list of
    problems (dicts as for pnp_iterate_batch): iterate() launches on the null
    stream without a host round trip, download() synchronises and returns the
    outputs and the state as pnp_iterate_batch does."""

    def __init__(self, problems, draw_pitch=4 * PNP_MAX_ITERATIONS, device=0):
        f32, i32 = np.float32, np.int32
        self.ns = len(problems)
        p2d = [_c(p["p2d"], f32).reshape(-1, 2) for p in problems]
        self.n = np.array([len(a) for a in p2d], i32)
        self.pt_pitch = max([1] + [len(a) for a in p2d])
        self.draw_pitch = int(draw_pitch)
        st = [p.get("state") or pnp_new_state(len(a)) for p, a in zip(problems, p2d)]
        cols = dict(n=self.n, p2d=p2d, cam=[[float(c) for c in p["cam"]] for p in problems],
                    draws=[_c(p["draws"], i32).reshape(-1)[:self.draw_pitch] for p in problems],
                    best_Tcw=[_c(t["best_Tcw"], f32) for t in st])
        cols.update({k: [p[k] for p in problems] for k in ("p3d", "max_error", "min_inliers", "max_its")})
        cols.update({k: [t[k] for t in st] for k in ("iterations", "best_inliers", "best_mask")})
        self.pack(_PNP_COLS, dict(pt=self.pt_pitch, draw=self.draw_pitch), cols, self.ns, device,
                  PnpDeviceBatch, pt_pitch=self.pt_pitch, draw_pitch=self.draw_pitch)

    def iterate(self, n_iterations, stream=None):
        check(lib().orbpnp_iterate_batch_device(C.byref(self.batch), self.ns, int(n_iterations),
                                                stream), "orbpnp_iterate_batch_device")

    def download(self):
        res, nm, ni, dc, it, bi, inl, bm, T, bT = self.fetch(
            "result", "no_more", "n_inliers", "draws_consumed", "iterations", "best_inliers",
            "inliers", "best_mask", "Tcw", "best_Tcw")
        return [dict(result=int(res[s]), no_more=bool(nm[s]), n_inliers=int(ni[s]),
                     inliers=inl[s, :self.n[s]].astype(bool), Tcw=T[s].reshape(4, 4).copy(),
                     draws_consumed=int(dc[s]),
                     state=dict(iterations=int(it[s]), best_inliers=int(bi[s]),
                                best_mask=bm[s, :self.n[s]].copy(), best_Tcw=bT[s].reshape(4, 4).copy()))
                for s in range(self.ns)]


# ---------------------------------------------------------------------------
# Sim3Solver (Sim3Solver.cc)
# ---------------------------------------------------------------------------
SIM3_MAX_POINTS = 2048
SIM3_MAX_ITERATIONS = 320
_SIM3_CORR = (("X3Dc1", np.float32, 3), ("X3Dc2", np.float32, 3), ("P1im1", np.float32, 2),
              ("P2im2", np.float32, 2), ("max_error1", np.int32, 1), ("max_error2", np.int32, 1))
_SIM3_STATE = (("best_T12", 16), ("best_R", 9), ("best_t", 3), ("best_s", 1))


class Sim3Pair(C.Structure):
    _fields_ = ([("n1", C.c_int32)] +
                [(k, C.c_void_p) for k in ("matched12", "valid1", "xyz1", "octave1")] +
                [("n2", C.c_int32)] +
                [(k, C.c_void_p) for k in ("valid2", "xyz2", "octave2", "Tcw1", "Tcw2")] +
                [(k, C.c_float) for k in ("fx", "fy", "cx", "cy")] +
                [(k, C.c_void_p) for k in ("n", "indices1", "X3Dc1", "X3Dc2", "P1im1", "P2im2",
                                           "max_error1", "max_error2")])


class Sim3SetupDeviceBatch(C.Structure):
    _fields_ = ([("d_n1", C.c_void_p), ("d_n2", C.c_void_p), ("pitch1", C.c_int32),
                 ("pitch2", C.c_int32)] +
                [("d_" + k, C.c_void_p) for k in ("matched12", "valid1", "xyz1", "octave1",
                                                  "valid2", "xyz2", "octave2", "Tcw1", "Tcw2",
                                                  "cam", "level_sigma2")] +
                [("nlevels", C.c_int32)] +
                [("d_" + k, C.c_void_p) for k in ("n", "indices1", "X3Dc1", "X3Dc2", "P1im1",
                                                  "P2im2", "max_error1", "max_error2")])


class Sim3Problem(C.Structure):
    _fields_ = ([(k, C.c_float) for k in ("fx", "fy", "cx", "cy")] + [("n", C.c_int32)] +
                [(k, C.c_void_p) for k in ("X3Dc1", "X3Dc2", "P1im1", "P2im2", "max_error1",
                                           "max_error2")] +
                [(k, C.c_int32) for k in ("min_inliers", "max_its", "fix_scale", "n_draws")] +
                [(k, C.c_void_p) for k in ("draws", "iterations", "best_inliers", "best_mask",
                                           "best_T12", "best_R", "best_t", "best_s", "T12",
                                           "result", "no_more", "n_inliers", "inliers",
                                           "draws_consumed")])


class Sim3DeviceBatch(C.Structure):
    _fields_ = ([("d_" + k, C.c_void_p) for k in ("n", "cam", "X3Dc1", "X3Dc2", "P1im1", "P2im2",
                                                  "max_error1", "max_error2")] +
                [("pt_pitch", C.c_int32)] +
                [("d_" + k, C.c_void_p) for k in ("min_inliers", "max_its", "fix_scale", "draws")] +
                [("draw_pitch", C.c_int32)] +
                [("d_" + k, C.c_void_p) for k in ("iterations", "best_inliers", "best_mask",
                                                  "best_T12", "best_R", "best_t", "best_s", "T12",
                                                  "result", "no_more", "n_inliers", "inliers",
                                                  "draws_consumed")])


def sim3_ransac_parameters(N, probability=0.99, minInliers=6, maxIterations=300):
    """Sim3Solver::SetRansacParameters (:114-138) on the host, with the
    platform's log / pow: mRansacMaxIts for N correspondences."""
    out = np.zeros(1, np.int32)
    check(lib().orbsim3_ransac_parameters(int(N), float(probability), int(minInliers),
                                          int(maxIterations), _ptr(out)),
          "orbsim3_ransac_parameters")
    return int(out[0])


def _sim3_pair_arrays(pr):
    f32, i32, u8 = np.float32, np.int32, np.uint8
    a = dict(matched12=_c(pr["matched12"], i32).reshape(-1), valid1=_c(pr["valid1"], u8).reshape(-1),
             xyz1=_c(pr["xyz1"], f32).reshape(-1, 3), octave1=_c(pr["octave1"], i32).reshape(-1),
             valid2=_c(pr["valid2"], u8).reshape(-1), xyz2=_c(pr["xyz2"], f32).reshape(-1, 3),
             octave2=_c(pr["octave2"], i32).reshape(-1), Tcw1=_c(pr["Tcw1"], f32).reshape(16),
             Tcw2=_c(pr["Tcw2"], f32).reshape(16))
    n1, n2 = len(a["matched12"]), len(a["valid2"])
    if any(len(a[k]) != n1 for k in ("valid1", "xyz1", "octave1")) or \
            any(len(a[k]) != n2 for k in ("xyz2", "octave2")):
        raise OrbplError("per-feature arrays of a keyframe differ in length")
    cam = pr["cam"]
    if hasattr(cam, "fx"):
        cam = (cam.fx, cam.fy, cam.cx, cam.cy)
    return a, n1, n2, [float(np.float32(c)) for c in cam]


def sim3_setup(pairs, level_sigma2):
    """The Sim3Solver constructor (:37-112) on the host for a list of keyframe
    pairs. Each pair is a dict: ``matched12`` [n1] (index in keyframe 2 of the
    point matched to feature i; -1 no match, -2 a point keyframe 2 does not
    observe), ``valid1`` [n1], ``xyz1`` [n1, 3], ``octave1`` [n1], ``valid2``
    [n2], ``xyz2`` [n2, 3], ``octave2`` [n2], ``Tcw1``, ``Tcw2`` [4, 4],
    ``cam`` = (fx, fy, cx, cy). Returns per pair a dict: ``n``, ``indices1``,
    ``X3Dc1``, ``X3Dc2``, ``P1im1``, ``P2im2``, ``max_error1``, ``max_error2``."""
    sig = _c(level_sigma2, np.float32).reshape(-1)
    arr = (Sim3Pair * max(1, len(pairs)))()
    keep, outs = [], []
    for p, pr in enumerate(pairs):
        a, n1, n2, cam = _sim3_pair_arrays(pr)
        o = dict(n=np.zeros(1, np.int32), indices1=np.zeros(max(1, n1), np.int32))
        for k, dt, w in _SIM3_CORR:
            o[k] = np.zeros((max(1, n1), w) if w > 1 else max(1, n1), dt)
        keep += [a, o]
        arr[p] = Sim3Pair(n1, _ptr(a["matched12"]), _ptr(a["valid1"]), _ptr(a["xyz1"]),
                          _ptr(a["octave1"]), n2, _ptr(a["valid2"]), _ptr(a["xyz2"]),
                          _ptr(a["octave2"]), _ptr(a["Tcw1"]), _ptr(a["Tcw2"]), *cam,
                          _ptr(o["n"]), _ptr(o["indices1"]),
                          *[_ptr(o[k]) for k, _, _ in _SIM3_CORR])
        outs.append(o)
    check(lib().orbsim3_setup(C.byref(arr), len(pairs), _ptr(sig), len(sig)), "orbsim3_setup")
    res = []
    for o in outs:
        n = int(o["n"][0])
        res.append(dict(n=n, **{k: v[:n].copy() for k, v in o.items() if k != "n"}))
    return res


def sim3_hypotheses(n, min_inliers, max_its, iterations, n_iterations):
    """hypotheses iterate(n_iterations) runs at most from this state: a call
    needs 3 draws for each"""
    if n < min_inliers:
        return 0
    return max(0, min(n_iterations, max_its - iterations))


def sim3_new_state(n):
    return dict(iterations=0, best_inliers=0, best_mask=np.zeros(n, np.uint8),
                best_T12=np.zeros((4, 4), np.float32), best_R=np.zeros((3, 3), np.float32),
                best_t=np.zeros(3, np.float32), best_s=np.float32(0))


def sim3_iterate_batch(problems, n_iterations):
    """Sim3Solver::iterate(n_iterations) for a list of independent solvers in
    one launch. Each problem is a dict: ``cam`` = (fx, fy, cx, cy), ``corr`` =
    the compacted correspondences of sim3_setup, ``min_inliers``, ``max_its``
    (sim3_ransac_parameters), ``fix_scale``, ``draws`` = raw rand() values, 3
    per hypothesis the call may run (sim3_hypotheses), ``state`` = the dict the
    previous call returned (missing or None: a new solver). Returns per problem
    a dict: ``result`` (0 empty, 1 a Sim3), ``no_more``, ``n_inliers``,
    ``inliers`` bool[n] per compacted correspondence, ``T12`` float32[4, 4],
    ``draws_consumed``, ``state``."""
    ns = len(problems)
    arr = (Sim3Problem * max(1, ns))()
    keep, outs = [], []
    f32, i32 = np.float32, np.int32
    for p, pr in enumerate(problems):
        co = pr["corr"]
        c = [_c(co[k], dt).reshape((-1, w) if w > 1 else -1) for k, dt, w in _SIM3_CORR]
        n = len(c[0])
        if any(len(x) != n for x in c):
            raise OrbplError("correspondence arrays differ in length")
        dr = _c(pr["draws"], i32).reshape(-1)
        st = pr.get("state") or sim3_new_state(n)
        it = np.array([st["iterations"]], i32)
        bi = np.array([st["best_inliers"]], i32)
        bm = _c(st["best_mask"], np.uint8).copy()
        if len(bm) != n:
            raise OrbplError("state belongs to another problem")
        sv = [_c(st[k], f32).reshape(w).copy() for k, w in _SIM3_STATE]
        T = np.zeros(16, f32)
        res, nm, ni, dc = (np.zeros(1, i32) for _ in range(4))
        inl = np.zeros(max(1, n), np.uint8)
        cam = [float(x) for x in pr["cam"]]
        keep += [c, dr, it, bi, bm, sv, T, res, nm, ni, dc, inl]
        arr[p] = Sim3Problem(cam[0], cam[1], cam[2], cam[3], n, *[_ptr(x) for x in c],
                             int(pr["min_inliers"]), int(pr["max_its"]),
                             int(bool(pr["fix_scale"])), len(dr), _ptr(dr), _ptr(it), _ptr(bi),
                             _ptr(bm), *[_ptr(x) for x in sv], _ptr(T), _ptr(res), _ptr(nm),
                             _ptr(ni), _ptr(inl), _ptr(dc))
        outs.append((n, it, bi, bm, sv, T, res, nm, ni, dc, inl))
    check(lib().orbsim3_iterate(C.byref(arr), ns, int(n_iterations)), "orbsim3_iterate")
    return [dict(result=int(res[0]), no_more=bool(nm[0]), n_inliers=int(ni[0]),
                 inliers=inl[:n].astype(bool), T12=T.reshape(4, 4).copy(),
                 draws_consumed=int(dc[0]),
                 state=dict(iterations=int(it[0]), best_inliers=int(bi[0]), best_mask=bm,
                            best_T12=sv[0].reshape(4, 4), best_R=sv[1].reshape(3, 3),
                            best_t=sv[2], best_s=np.float32(sv[3][0])))
            for n, it, bi, bm, sv, T, res, nm, ni, dc, inl in outs]


class Sim3Solver:
    """ORB_SLAM2::Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale) over a
    keyframe pair as sim3_setup takes it. Draws come from the C library's
    rand() through the process-wide look-ahead queue PnPsolver uses (P29)."""

    def __init__(self, pair, level_sigma2, bFixScale=False):
        _, self.mN1, _, self.cam = _sim3_pair_arrays(pair)
        self.corr = sim3_setup([pair], level_sigma2)[0]
        self.N = self.corr["n"]
        self.mvnIndices1 = self.corr["indices1"]
        self.fix_scale = bool(bFixScale)
        self.state = sim3_new_state(self.N)
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        if minInliers < 3:
            raise OrbplError("minInliers below the minimal set of 3")
        self.min_inliers = int(minInliers)
        self.max_its = sim3_ransac_parameters(self.N, probability, minInliers, maxIterations)
        self.state["iterations"] = 0

    def iterate(self, nIterations, draws=None):
        """Returns (T12 float32[4, 4] or None, bNoMore, vbInliers bool per
        feature of keyframe 1, nInliers). ``draws`` = raw rand() values for
        this call (3 per hypothesis it may run); None takes them from rand()."""
        need = 3 * sim3_hypotheses(self.N, self.min_inliers, self.max_its,
                                   self.state["iterations"], nIterations)
        own = draws is None
        d = _pnp_take_rand(need) if own else _c(draws, np.int32)
        o = sim3_iterate_batch([dict(cam=self.cam, corr=self.corr, min_inliers=self.min_inliers,
                                     max_its=self.max_its, fix_scale=self.fix_scale, draws=d,
                                     state=self.state)], nIterations)[0]
        if own:
            del _pnp_rand_queue[:o["draws_consumed"]]
        self.state = o["state"]
        self.last = o
        vb = np.zeros(self.mN1, bool)
        if o["result"]:
            vb[self.mvnIndices1[o["inliers"]]] = True
        return (o["T12"] if o["result"] else None), o["no_more"], vb, o["n_inliers"]

    def find(self, draws=None):
        """(T12 or None, vbInliers12, nInliers)"""
        T, _, vb, n = self.iterate(self.max_its, draws)
        return T, vb, n

    def GetEstimatedRotation(self):
        return self.state["best_R"].copy()

    def GetEstimatedTranslation(self):
        return self.state["best_t"].copy()

    def GetEstimatedScale(self):
        return np.float32(self.state["best_s"])


_SIM3_COLS = (_cols("n1 n2 min_inliers fix_scale", np.int32) + _cols("cam", np.float32, (4,)) +
              _cols("Tcw1 Tcw2", np.float32, (16,)) + _cols("matched12", np.int32, (), "p1", -1) +
              _cols("valid1", np.uint8, (), "p1") + _cols("valid2", np.uint8, (), "p2") +
              _cols("xyz1", np.float32, (3,), "p1") + _cols("xyz2", np.float32, (3,), "p2") +
              _cols("octave1", np.int32, (), "p1") + _cols("octave2", np.int32, (), "p2") +
              _cols("draws", np.int32, (), "draw") +
              # out (max_its: 1 until setup() has the table's value)
              _cols("n iterations best_inliers result no_more n_inliers draws_consumed", np.int32) +
              _cols("max_its", np.int32, pad=1) + _cols("indices1", np.int32, (), "p1") +
              _cols("best_mask inliers", np.uint8, (), "p1") + _cols("T12", np.float32, (16,)) +
              tuple((k, dt, (w,), "p1", 0) for k, dt, w in _SIM3_CORR) +
              tuple((k, np.float32, (w,), None, 0) for k, w in _SIM3_STATE))


class Sim3DeviceProblems(PitchedProblems):
    """The pitched device arrays of orbsim3_setup_batch_device and
    orbsim3_iterate_batch_device for a list of keyframe pairs (dicts as for
    sim3_setup, plus ``fix_scale``, ``draws`` and optionally ``min_inliers``):
    setup() runs the constructor kernel and the host parameter table,
    iterate() launches on the null stream without a host round trip,
    download() synchronises and returns the correspondences, the outputs and
    the state as sim3_setup and sim3_iterate_batch do."""

    def __init__(self, pairs, level_sigma2, probability=0.99, minInliers=6, maxIterations=300,
                 draw_pitch=3 * SIM3_MAX_ITERATIONS, device=0):
        i32 = np.int32
        self.ns = len(pairs)
        self.draw_pitch = int(draw_pitch)
        self.params = (probability, maxIterations)
        arrs = [_sim3_pair_arrays(p) for p in pairs]
        self.n1 = np.array([a[1] for a in arrs] or [0], i32)
        self.n2 = np.array([a[2] for a in arrs] or [0], i32)
        self.pitch1 = p1 = max(1, int(self.n1.max()))
        self.pitch2 = p2 = max(1, int(self.n2.max()))
        sig = _c(level_sigma2, np.float32).reshape(-1)
        self.nlevels = len(sig)
        cols = {k: [a[0][k] for a in arrs] for k in ("matched12", "valid1", "xyz1", "octave1", "valid2",
                                                     "xyz2", "octave2", "Tcw1", "Tcw2")}
        cols.update(n1=self.n1[:self.ns], n2=self.n2[:self.ns], cam=[a[3] for a in arrs], level_sigma2=sig,
                    min_inliers=[p.get("min_inliers", minInliers) for p in pairs],
                    fix_scale=[bool(p.get("fix_scale", False)) for p in pairs],
                    draws=[_c(p.get("draws", ()), i32).reshape(-1)[:self.draw_pitch] for p in pairs])
        self.pack(_SIM3_COLS, dict(p1=p1, p2=p2, draw=self.draw_pitch), cols, self.ns, device,
                  Sim3DeviceBatch, pt_pitch=p1, draw_pitch=self.draw_pitch)
        self.min_inliers = self.host["min_inliers"]
        self.n = None
        if device is not None:
            self.setup_batch = self.struct(Sim3SetupDeviceBatch, pitch1=p1, pitch2=p2, nlevels=self.nlevels)

    def setup(self, stream=None):
        """the constructor kernel, then SetRansacParameters per solver on the
        host (it needs each N): one synchronisation"""
        check(lib().orbsim3_setup_batch_device(C.byref(self.setup_batch), self.ns, stream),
              "orbsim3_setup_batch_device")
        check(lib().orbpl_device_synchronize(self.device), "orbpl_device_synchronize")
        S = max(1, self.ns)
        self.n = self.bufs["n"].download(np.int32, S)
        mx = np.ones(S, np.int32)
        for s in range(self.ns):
            mx[s] = sim3_ransac_parameters(self.n[s], self.params[0], self.min_inliers[s],
                                           self.params[1])
        self.max_its = mx
        self.bufs["max_its"].upload(mx)

    def iterate(self, n_iterations, stream=None):
        check(lib().orbsim3_iterate_batch_device(C.byref(self.batch), self.ns, int(n_iterations),
                                                 stream), "orbsim3_iterate_batch_device")

    def download(self):
        names = ("n", "result", "no_more", "n_inliers", "draws_consumed", "iterations", "best_inliers",
                 "indices1", "inliers", "best_mask", "T12") + tuple(k for k, _, _ in _SIM3_CORR) + \
            tuple(k for k, _ in _SIM3_STATE)
        g = dict(zip(names, self.fetch(*names)))
        out = []
        for s in range(self.ns):
            n = int(g["n"][s])
            corr = dict(n=n, indices1=g["indices1"][s, :n].copy())
            for k, dt, w in _SIM3_CORR:
                corr[k] = g[k][s, :n].reshape((n, w) if w > 1 else n).copy()
            out.append(dict(corr=corr, result=int(g["result"][s]), no_more=bool(g["no_more"][s]),
                            n_inliers=int(g["n_inliers"][s]), inliers=g["inliers"][s, :n].astype(bool),
                            T12=g["T12"][s].reshape(4, 4).copy(),
                            draws_consumed=int(g["draws_consumed"][s]),
                            state=dict(iterations=int(g["iterations"][s]),
                                       best_inliers=int(g["best_inliers"][s]),
                                       best_mask=g["best_mask"][s, :n].copy(),
                                       best_T12=g["best_T12"][s].reshape(4, 4).copy(),
                                       best_R=g["best_R"][s].reshape(3, 3).copy(),
                                       best_t=g["best_t"][s].copy(),
                                       best_s=np.float32(g["best_s"][s, 0]))))
        return out


# ---------------------------------------------------------------------------
# ORBmatcher::SearchBySim3 (ORBmatcher.cc:1441-1693)
# ---------------------------------------------------------------------------
SIM3_MATCHED, SIM3_NO_POINT, SIM3_ALREADY, SIM3_BEHIND, SIM3_OUT_OF_IMAGE, SIM3_DISTANCE, \
    SIM3_EMPTY_AREA, SIM3_NO_MATCH = range(8)
SIM3_MAX_FEATURES = 2048
_SBS_KF = (("kps_un", KP_DTYPE, ()), ("desc", np.uint8, (32,)), ("valid", np.uint8, ()),
           ("xyz", np.float32, (3,)), ("min_dist", np.float32, ()), ("max_dist", np.float32, ()),
           ("mp_desc", np.uint8, (32,)))


class Sim3Keyframe(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(k, C.c_void_p) for k, _, _ in _SBS_KF] + [("Tcw", C.c_void_p)]


class Sim3MatchPair(C.Structure):
    _fields_ = ([("kf1", Sim3Keyframe), ("kf2", Sim3Keyframe), ("s12", C.c_float)] +
                [(k, C.c_void_p) for k in ("R12", "t12", "matched12", "n_found", "vn_match1",
                                           "vn_match2", "reason1", "reason2")])


class Sim3MatchDeviceBatch(C.Structure):
    _fields_ = ([("d_n1", C.c_void_p), ("d_n2", C.c_void_p), ("pitch1", C.c_int32),
                 ("pitch2", C.c_int32)] +
                [("d_%s%d" % (k, s), C.c_void_p) for s in (1, 2)
                 for k in [k for k, _, _ in _SBS_KF] + ["Tcw"]] +
                [("d_" + k, C.c_void_p) for k in ("s12", "R12", "t12", "matched12", "n_found",
                                                  "vn_match1", "vn_match2", "reason1", "reason2")])


def _sbs_keyframe(kf):
    a = {k: _c(kf[k], dt).reshape((-1,) + w) for k, dt, w in _SBS_KF}
    n = len(a["kps_un"])
    if any(len(v) != n for v in a.values()):
        raise OrbplError("per-feature arrays of a keyframe differ in length")
    a["Tcw"] = _c(kf["Tcw"], np.float32).reshape(16)
    return a, n


def search_by_sim3_batch(camera, scale_factors, pairs, th):
    """ORBmatcher::SearchBySim3 for a list of keyframe pairs in one launch.
    Each pair is a dict: ``kf1`` / ``kf2`` = dicts of per-feature arrays
    ``kps_un`` (KP_DTYPE), ``desc`` [n, 32], ``valid`` (the feature has a map
    point and it is not bad), ``xyz`` [n, 3], ``min_dist`` / ``max_dist`` (raw
    mfMinDistance / mfMaxDistance), ``mp_desc`` [n, 32], and ``Tcw`` [4, 4];
    ``matched12`` [n1]; ``s12``, ``R12`` [3, 3], ``t12`` [3]. Returns per pair
    a dict: ``n_found``, ``matched12`` (updated copy), ``vn_match1``,
    ``vn_match2``, ``reason1``, ``reason2`` (SIM3_* codes)."""
    sf = _c(scale_factors, np.float32)
    arr = (Sim3MatchPair * max(1, len(pairs)))()
    keep, outs = [], []
    i32 = np.int32
    for p, pr in enumerate(pairs):
        a1, n1 = _sbs_keyframe(pr["kf1"])
        a2, n2 = _sbs_keyframe(pr["kf2"])
        m = _c(pr["matched12"], i32).reshape(-1).copy()
        if len(m) != n1:
            raise OrbplError("matched12 and keyframe 1 differ in length")
        R, t = _c(pr["R12"], np.float32).reshape(9), _c(pr["t12"], np.float32).reshape(3)
        nf = np.zeros(1, i32)
        v1, r1 = np.zeros(max(1, n1), i32), np.zeros(max(1, n1), i32)
        v2, r2 = np.zeros(max(1, n2), i32), np.zeros(max(1, n2), i32)
        keep += [a1, a2, m, R, t, nf, v1, v2, r1, r2]
        k1 = Sim3Keyframe(n1, *[_ptr(a1[k]) for k, _, _ in _SBS_KF], _ptr(a1["Tcw"]))
        k2 = Sim3Keyframe(n2, *[_ptr(a2[k]) for k, _, _ in _SBS_KF], _ptr(a2["Tcw"]))
        arr[p] = Sim3MatchPair(k1, k2, float(pr["s12"]), _ptr(R), _ptr(t), _ptr(m), _ptr(nf),
                               _ptr(v1), _ptr(v2), _ptr(r1), _ptr(r2))
        outs.append((n1, n2, m, nf, v1, v2, r1, r2))
    check(lib().orbm_search_by_sim3(C.byref(camera), _ptr(sf), len(sf), C.byref(arr), len(pairs),
                                    float(th)), "orbm_search_by_sim3")
    return [dict(n_found=int(nf[0]), matched12=m, vn_match1=v1[:n1], vn_match2=v2[:n2],
                 reason1=r1[:n1], reason2=r2[:n2]) for n1, n2, m, nf, v1, v2, r1, r2 in outs]


_SBS_COLS = (tuple(("%s%d" % (k, side), dt, w, side, 0) for side in (1, 2) for k, dt, w in _SBS_KF) +
             _cols("Tcw1 Tcw2", np.float32, (16,)) + _cols("n1 n2", np.int32) +
             _cols("s12", np.float32) + _cols("R12", np.float32, (9,)) + _cols("t12", np.float32, (3,)) +
             _cols("matched12", np.int32, (), 1, -1) +
             # out
             _cols("n_found", np.int32) + _cols("vn_match1 reason1", np.int32, (), 1) +
             _cols("vn_match2 reason2", np.int32, (), 2))


class Sim3MatchDeviceProblems(PitchedProblems):
    """The pitched device arrays of orbm_search_by_sim3_batch_device for a list
    of pairs (dicts as for search_by_sim3_batch): run() launches without a
    host round trip, download() synchronises and returns what
    search_by_sim3_batch returns."""

    def __init__(self, pairs, device=0):
        self.ns = len(pairs)
        ks = [(_sbs_keyframe(p["kf1"]), _sbs_keyframe(p["kf2"])) for p in pairs]
        self.n1 = np.array([k[0][1] for k in ks] or [0], np.int32)
        self.n2 = np.array([k[1][1] for k in ks] or [0], np.int32)
        self.pitch = pt = (max(1, int(self.n1.max())), max(1, int(self.n2.max())))
        cols = {"%s%d" % (k, side): [kk[side - 1][0][k] for kk in ks]
                for side in (1, 2) for k in [k for k, _, _ in _SBS_KF] + ["Tcw"]}
        cols.update({k: [p[k] for p in pairs] for k in ("s12", "R12", "t12", "matched12")})
        cols.update(n1=self.n1[:self.ns], n2=self.n2[:self.ns])
        self.pack(_SBS_COLS, {1: pt[0], 2: pt[1]}, cols, self.ns, device, Sim3MatchDeviceBatch,
                  pitch1=pt[0], pitch2=pt[1])
        self.host_matched12 = self.host["matched12"]     # to restore the in/out array between runs

    def run(self, camera, scale_factors, th, stream=None):
        sf = _c(scale_factors, np.float32)
        check(lib().orbm_search_by_sim3_batch_device(C.byref(camera), _ptr(sf), len(sf),
                                                     C.byref(self.batch), self.ns, float(th),
                                                     stream), "orbm_search_by_sim3_batch_device")

    def download(self):
        nf, m, v1, r1, v2, r2 = self.fetch("n_found", "matched12", "vn_match1", "reason1", "vn_match2",
                                           "reason2")
        return [dict(n_found=int(nf[s]), matched12=m[s, :self.n1[s]].copy(),
                     vn_match1=v1[s, :self.n1[s]].copy(), vn_match2=v2[s, :self.n2[s]].copy(),
                     reason1=r1[s, :self.n1[s]].copy(), reason2=r2[s, :self.n2[s]].copy())
                for s in range(self.ns)]


# ---------------------------------------------------------------------------
# Tracking::Relocalization as one batched call
# ---------------------------------------------------------------------------
RL_OK, RL_NO_CANDIDATES, RL_FAILED, RL_DRAW_EXHAUSTED = 0, 1, 2, 3
RL_REC = ("bow_matches", "discarded", "calls", "iterations", "draws_used", "result", "no_more",
          "n_inliers", "g1", "nadd1", "g2", "nadd2", "g3")
RL_TABLE_N = 2048


class RelocProblem(C.Structure):
    _fields_ = ([("nkf", C.c_int32)] +
                [(k, C.c_void_p) for k in ("kf_off", "kf_words", "kf_vals", "covis", "reloc_score",
                                           "kf_feat_off", "kf_angle", "kf_feat_node", "kf_desc",
                                           "kf_valid", "mp_xyz", "mp_min_dist", "mp_max_dist",
                                           "mp_desc")] +
                [("n", C.c_int32)] +
                [(k, C.c_void_p) for k in ("kps_un", "uright", "desc", "feat_node")] +
                [("nq_words", C.c_int32), ("q_words", C.c_void_p), ("q_vals", C.c_void_p),
                 ("n_draw_streams", C.c_int32), ("draws", C.c_void_p)] +
                [(k, C.c_int32) for k in ("ok", "status", "winner", "rounds", "n_good",
                                          "n_candidates", "ncand")] +
                [("cand", C.c_int32 * 64), ("Tcw", C.c_float * 16), ("mp_kf_feature", C.c_void_p),
                 ("outlier", C.c_void_p), ("records", C.c_void_p)])


def _declare_reloc(L):
    vp, i = C.c_void_p, C.c_int
    L.orbrl_create.argtypes = [vp, vp, vp, i, i, i, i, C.POINTER(vp)]
    L.orbrl_destroy.argtypes = [vp]
    L.orbrl_destroy.restype = None
    L.orbrl_ransac_table.argtypes = [vp, vp, i]
    L.orbrl_relocalize.argtypes = [vp, vp, i, i]


def reloc_ransac_table(n_entries=RL_TABLE_N + 1):
    """SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)'s (min_inliers,
    max_its) for N = 0 .. n_entries - 1, as the Relocalizer's handle holds it."""
    mn = np.zeros(n_entries, np.int32)
    mx = np.zeros(n_entries, np.int32)
    check(lib().orbrl_ransac_table(_ptr(mn), _ptr(mx), n_entries), "orbrl_ransac_table")
    return mn, mx


class Relocalizer:
    """Tracking::Relocalization (Tracking.cc:2049-2269) for a batch of lost
    frames, each with its own keyframe database. A problem is a dict:
    ``kf_bows`` / ``covis`` / ``reloc_score`` as for detect_reloc_batch,
    ``kfs`` = per database keyframe a dict of per-feature arrays (angle,
    feat_node, desc, valid, mp_xyz, mp_min_dist, mp_max_dist, mp_desc),
    ``frame`` = dict(kps_un, uright, desc, feat_node, bow_words, bow_vals) and
    ``draws`` = int32 [streams, draw_pitch] raw rand() values, stream c for
    candidate c (P30)."""

    def __init__(self, camera, scale_factors, level_sigma2, max_problems=64, kp_pitch=1024,
                 draw_pitch=4 * PNP_MAX_ITERATIONS):
        sf, s2 = _c(scale_factors, np.float32), _c(level_sigma2, np.float32)
        self._h = C.c_void_p()
        self.kp_pitch, self.draw_pitch, self.max_problems = kp_pitch, draw_pitch, max_problems
        check(lib().orbrl_create(C.byref(camera), _ptr(sf), _ptr(s2), len(sf), int(max_problems),
                                 int(kp_pitch), int(draw_pitch), C.byref(self._h)), "orbrl_create")

    def close(self):
        if getattr(self, "_h", None):
            lib().orbrl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def relocalize_batch(self, problems, scoring=0):
        """Returns per problem a dict: ok, status (RL_*), winner (database
        index or -1), rounds, Tcw [4, 4], n_good, n_candidates, cand,
        mp_kf_feature [n], outlier [n], records (one dict of RL_REC per
        candidate), reloc_score (updated copy). Raises OrbplError
        (ORBPL_ERR_OVERFLOW) when a problem runs out of draws (P31); the
        results up to there are in the exception's ``results``."""
        nq = len(problems)
        arr = (RelocProblem * max(1, nq))()
        keep, outs = [], []
        for p, pr in enumerate(problems):
            bows, kfs, F = pr["kf_bows"], pr["kfs"], pr["frame"]
            nkf = len(bows)
            assert len(kfs) == nkf
            off = np.zeros(nkf + 1, np.int32)
            foff = np.zeros(nkf + 1, np.int32)
            for k in range(nkf):
                off[k + 1] = off[k] + len(bows[k][0])
                foff[k + 1] = foff[k] + len(kfs[k]["angle"])

            def cat(key, dt, shape):
                if not nkf:
                    return np.zeros((0,) + shape, dt)
                return _c(np.concatenate([_c(kf[key], dt).reshape((-1,) + shape) for kf in kfs]), dt)

            kw = (_c(np.concatenate([_c(w, np.uint32) for w, _ in bows]), np.uint32) if nkf
                  else np.zeros(0, np.uint32))
            kv = (_c(np.concatenate([_c(v, np.float64) for _, v in bows]), np.float64) if nkf
                  else np.zeros(0, np.float64))
            cov = np.full((max(1, nkf), KFDB_COVISIBLES), -1, np.int32)
            for k, lst in enumerate(pr.get("covis", [])[:nkf]):
                lst = list(lst)[:KFDB_COVISIBLES]
                cov[k, :len(lst)] = lst
            rs = np.zeros(max(1, nkf), np.float32)
            if pr.get("reloc_score") is not None:
                rs[:nkf] = _c(pr["reloc_score"], np.float32)
            ka, kn = cat("angle", np.float32, ()), cat("feat_node", np.int32, ())
            kd, kvl = cat("desc", np.uint8, (32,)), cat("valid", np.uint8, ())
            mx, mmin = cat("mp_xyz", np.float32, (3,)), cat("mp_min_dist", np.float32, ())
            mmax, md = cat("mp_max_dist", np.float32, ()), cat("mp_desc", np.uint8, (32,))
            kps, ur = _c(F["kps_un"], KP_DTYPE), _c(F["uright"], np.float32)
            fd, fn = _c(F["desc"], np.uint8), _c(F["feat_node"], np.int32)
            qw, qv = _c(F["bow_words"], np.uint32), _c(F["bow_vals"], np.float64)
            dr = _c(pr["draws"], np.int32).reshape(-1, self.draw_pitch)
            n = len(kps)
            om = np.full(max(1, n), -1, np.int32)
            oo = np.zeros(max(1, n), np.uint8)
            rec = np.zeros((64, len(RL_REC)), np.int32)
            keep += [off, foff, kw, kv, cov, rs, ka, kn, kd, kvl, mx, mmin, mmax, md, kps, ur, fd,
                     fn, qw, qv, dr, om, oo, rec]
            r = arr[p]
            r.nkf = nkf
            for name, a in (("kf_off", off), ("kf_words", kw), ("kf_vals", kv), ("covis", cov),
                            ("reloc_score", rs), ("kf_feat_off", foff), ("kf_angle", ka),
                            ("kf_feat_node", kn), ("kf_desc", kd), ("kf_valid", kvl),
                            ("mp_xyz", mx), ("mp_min_dist", mmin), ("mp_max_dist", mmax),
                            ("mp_desc", md), ("kps_un", kps), ("uright", ur), ("desc", fd),
                            ("feat_node", fn), ("q_words", qw), ("q_vals", qv), ("draws", dr),
                            ("mp_kf_feature", om), ("outlier", oo), ("records", rec)):
                setattr(r, name, a.ctypes.data if a.size else None)
            r.mp_kf_feature, r.outlier = om.ctypes.data, oo.ctypes.data
            r.n, r.nq_words, r.n_draw_streams = n, len(qw), len(dr)
            outs.append((nkf, n, om, oo, rec, rs))
        rc = lib().orbrl_relocalize(self._h, C.byref(arr), nq, int(scoring))
        if rc not in (0, -5):
            check(rc, "orbrl_relocalize")
        res = []
        for p, (nkf, n, om, oo, rec, rs) in enumerate(outs):
            r = arr[p]
            nc = r.ncand
            res.append(dict(ok=bool(r.ok), status=r.status, winner=r.winner, rounds=r.rounds,
                            Tcw=np.array(r.Tcw, np.float32).reshape(4, 4), n_good=r.n_good,
                            n_candidates=r.n_candidates, cand=np.array(r.cand[:nc], np.int32),
                            mp_kf_feature=om[:n].copy(), outlier=oo[:n].copy(),
                            records=[dict(zip(RL_REC, (int(v) for v in rec[c])))
                                     for c in range(nc)],
                            reloc_score=rs[:nkf].copy()))
        if rc == -5:
            try:
                check(rc, "orbrl_relocalize")
            except OrbplError as e:
                e.results = res
                raise
        return res

    def relocalize(self, voc, problem, levelsup=4):
        """One lost frame: Frame::ComputeBoW through ``voc`` (an ORBVocabulary)
        for ``problem["frame"]`` (its feat_node / bow_words / bow_vals are
        filled in), then relocalize_batch. The draws come from the C library's
        rand() (pnp_srand), draw_pitch values per candidate in candidate order;
        values a candidate does not consume are dropped (P30). A convenience:
        to know how many streams to draw it runs place recognition once on its
        own (detect_reloc_batch) before the call runs it again - a launch and
        a host round trip that relocalize_batch with the caller's own streams
        does not have."""
        F = dict(problem["frame"])
        bw, bv, fn = voc.transform(F["desc"], levelsup)[:3]
        F.update(bow_words=bw, bow_vals=bv, feat_node=fn)
        pre = detect_reloc_batch([dict(kf_bows=problem["kf_bows"], covis=problem.get("covis", []),
                                       reloc_score=problem.get("reloc_score"), q_words=bw,
                                       q_vals=bv)])[0]
        nc = len(pre["cand"])
        draws = np.zeros((nc, self.draw_pitch), np.int32)
        for c in range(nc):
            draws[c] = _pnp_take_rand(self.draw_pitch)
            del _pnp_rand_queue[:self.draw_pitch]
        return self.relocalize_batch([dict(problem, frame=F, draws=draws)])[0]


class RelocDeviceBatch(C.Structure):
    """orbrl_device_batch: pitched device arrays (see include/orbpl.h)"""
    _fields_ = ([(k, C.c_void_p) for k in ("d_nkf", "d_kf_off", "d_kf_words", "d_kf_vals")] +
                [("ent_pitch", C.c_int64), ("d_covis", C.c_void_p), ("d_reloc_score", C.c_void_p),
                 ("d_q_n", C.c_void_p), ("d_q_words", C.c_void_p), ("d_q_vals", C.c_void_p),
                 ("q_pitch", C.c_int64)] +
                [(k, C.c_void_p) for k in ("d_kf_first", "d_kf_n", "d_kf_angle", "d_kf_feat_node",
                                           "d_kf_desc", "d_kf_valid", "d_mp_xyz", "d_mp_min_dist",
                                           "d_mp_max_dist", "d_mp_desc", "d_n", "d_kps_un",
                                           "d_uright", "d_desc", "d_feat_node", "d_draws",
                                           "d_n_streams")] +
                [("stream_pitch", C.c_int32)] +
                [(k, C.c_void_p) for k in ("d_cand", "d_ncand", "d_ok", "d_status", "d_winner",
                                           "d_rounds", "d_n_good", "d_n_candidates", "d_Tcw",
                                           "d_mp_kf_feature", "d_outlier", "d_records")])


def _declare_reloc_device(L):
    L.orbrl_relocalize_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                C.c_void_p]


def _reloc_relocalize_batch_device(self, batch, n, scoring=0, stream=None):
    """orbrl_relocalize_batch_device over a RelocDeviceBatch of n problems"""
    check(lib().orbrl_relocalize_batch_device(self._h, C.byref(batch), int(n), int(scoring),
                                              stream), "orbrl_relocalize_batch_device")


Relocalizer.relocalize_batch_device = _reloc_relocalize_batch_device


# ---------------------------------------------------------------------------
# LocalMapping::CreateNewMapPoints + CreateNewMapLines as one batched call
# 
# ---------------------------------------------------------------------------
LM_MAX_KEYPOINTS, LM_MAX_LINES, LM_MAX_NEIGHBOURS = 2048, 256, 10
LM_RECORD_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"),
                            ("desc_from", "<i4"), ("xyz", "<f4", 3), ("normal", "<f4", 3),
                            ("min_dist", "<f4"), ("max_dist", "<f4")])
LM_LINE_RECORD_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"),
                                 ("desc_from", "<i4"), ("xyz6", "<f4", 6), ("reserved", "<i4", 2)])


class LmKeyFrame(C.Structure):
    """orblm_keyframe"""
    _fields_ = ([("id", C.c_int32), ("Tcw", C.c_void_p), ("n", C.c_int32)] +
                [(k, C.c_void_p) for k in ("kps", "kps_un", "uright", "depth", "desc",
                                           "feat_node", "has_mp", "mp_xyz")] +
                [("nl", C.c_int32)] + [(k, C.c_void_p) for k in ("klines", "ldesc", "lcoef")])


class LmProblem(C.Structure):
    """orblm_problem"""
    _fields_ = [("cur", LmKeyFrame), ("n_neigh", C.c_int32), ("neigh", C.c_void_p),
                ("points", C.c_void_p), ("n_points", C.c_int32),
                ("kf1_point_record", C.c_void_p), ("pairs", C.c_int32 * LM_MAX_NEIGHBOURS),
                ("lines", C.c_void_p), ("n_lines", C.c_int32), ("kf1_line_record", C.c_void_p),
                ("line_pairs", C.c_int32 * LM_MAX_NEIGHBOURS)]


class LmDeviceBatch(C.Structure):
    """orblm_device_batch: a pitched pool of keyframes (see include/orbpl.h)"""
    _fields_ = ([("nkf", C.c_int32), ("kp_pitch", C.c_int32), ("line_pitch", C.c_int32)] +
                [(k, C.c_void_p) for k in ("d_kf_id", "d_kf_n", "d_kf_Tcw", "d_kps", "d_kps_un",
                                           "d_uright", "d_depth", "d_desc", "d_feat_node",
                                           "d_has_mp", "d_mp_xyz", "d_kf_nl", "d_klines", "d_ldesc",
                                           "d_lcoef", "d_cur", "d_neigh", "d_points",
                                           "d_n_points", "d_kf1_point_record", "d_pairs", "d_lines",
                                           "d_n_lines", "d_kf1_line_record", "d_line_pairs")])


def _declare_localmap(L):
    vp, i = C.c_void_p, C.c_int
    L.orblm_create_new_map_features.argtypes = [vp, vp, vp, i, vp, i]
    L.orblm_create_new_map_features_batch_device.argtypes = [vp, vp, vp, i, vp, i, vp]
    L.orbm_search_for_triangulation.argtypes = [vp, vp, vp, i, vp, vp, vp, i, i, vp,
                                                C.POINTER(C.c_int), vp]
    L.orbl_search_for_triangulation.argtypes = [i, vp, i, vp, vp, C.POINTER(C.c_int)]


def _lm_arrays(kf):
    """the arrays of a keyframe dict (id, Tcw, kps, kps_un, uright, depth, desc,
    feat_node, has_mp, mp_xyz; klines, ldesc, lcoef), absent line fields = no
    lines, absent mp_xyz = zeros"""
    n = len(_c(kf["uright"], np.float32))
    a = dict(kps=_c(kf["kps"], KP_DTYPE), kps_un=_c(kf["kps_un"], KP_DTYPE),
             uright=_c(kf["uright"], np.float32), depth=_c(kf["depth"], np.float32),
             desc=_c(kf["desc"], np.uint8).reshape(n, 32), feat_node=_c(kf["feat_node"], np.int32),
             has_mp=_c(kf["has_mp"], np.uint8),
             mp_xyz=_c(kf.get("mp_xyz", np.zeros((n, 3))), np.float32).reshape(n, 3))
    ld = _c(kf.get("ldesc", np.zeros((0, 32))), np.uint8).reshape(-1, 32)
    a.update(klines=_c(kf.get("klines", np.zeros(0, KEYLINE_DTYPE)), KEYLINE_DTYPE), ldesc=ld,
             lcoef=_c(kf.get("lcoef", np.zeros((0, 3))), np.float64).reshape(-1, 3))
    return n, len(ld), a


_LM_POINT_FIELDS = ("kps", "kps_un", "uright", "depth", "desc", "feat_node", "has_mp", "mp_xyz")
_LM_LINE_FIELDS = ("klines", "ldesc", "lcoef")


def _lm_keyframe(kf, keep):
    """LmKeyFrame of a keyframe dict; the arrays it points into go to `keep`."""
    T = _c(kf["Tcw"], np.float32).reshape(16)
    n, nl, a = _lm_arrays(kf)
    keep += [T, a]
    return LmKeyFrame(int(kf["id"]), _ptr(T), n, *[_ptr(a[k]) for k in _LM_POINT_FIELDS], nl,
                      *[_ptr(a[k]) for k in _LM_LINE_FIELDS])


def _lm_outputs(n1, nl1, n_points, points, rec, pairs, n_lines, lines, lrec, lpairs):
    return dict(points=points[:n_points].copy(), kf1_point_record=rec[:n1].copy(),
                pairs=np.array(pairs, np.int32), lines=lines[:n_lines].copy(),
                kf1_line_record=lrec[:nl1].copy(), line_pairs=np.array(lpairs, np.int32))


class LocalMapper:
    """LocalMapping::CreateNewMapPoints() then CreateNewMapLines()
    (non-monocular) for many (current keyframe, <= 10 neighbours) problems in one
    launch. A problem is dict(cur=keyframe, neigh=[keyframes]), a keyframe
    dict(id, Tcw, kps, kps_un, uright, depth, desc, feat_node, has_mp, mp_xyz,
    klines, ldesc, lcoef). Results per problem: points / lines (records of
    LM_RECORD_DTYPE / LM_LINE_RECORD_DTYPE in creation order), kf1_point_record,
    kf1_line_record, pairs[10], line_pairs[10]."""

    def __init__(self, camera, scale_factors, level_sigma2):
        self.camera = camera
        self.scale = _c(scale_factors, np.float32)
        self.sigma2 = _c(level_sigma2, np.float32)
        assert len(self.scale) == len(self.sigma2)

    def _consts(self):
        return C.byref(self.camera), _ptr(self.scale), _ptr(self.sigma2), len(self.scale)

    def create_new_map_features(self, problems):
        keep, P = [], (LmProblem * max(1, len(problems)))()
        outs = []
        for p, prob in enumerate(problems):
            cur = _lm_keyframe(prob["cur"], keep)
            nb = (LmKeyFrame * max(1, len(prob["neigh"])))(
                *[_lm_keyframe(k, keep) for k in prob["neigh"]])
            pts = np.zeros(max(1, cur.n), LM_RECORD_DTYPE)
            rec = np.full(max(1, cur.n), -1, np.int32)
            lns = np.zeros(max(1, LM_MAX_NEIGHBOURS * cur.nl), LM_LINE_RECORD_DTYPE)
            lrec = np.full(max(1, cur.nl), -1, np.int32)
            keep += [nb, pts, rec, lns, lrec]
            outs.append((pts, rec, lns, lrec))
            P[p].cur, P[p].n_neigh = cur, len(prob["neigh"])
            P[p].neigh = C.cast(nb, C.c_void_p)
            P[p].points, P[p].kf1_point_record = _ptr(pts), _ptr(rec)
            P[p].lines, P[p].kf1_line_record = _ptr(lns), _ptr(lrec)
        check(lib().orblm_create_new_map_features(*self._consts(), P, len(problems)),
              "orblm_create_new_map_features")
        return [_lm_outputs(P[p].cur.n, P[p].cur.nl, P[p].n_points, outs[p][0], outs[p][1],
                            list(P[p].pairs), P[p].n_lines, outs[p][2], outs[p][3],
                            list(P[p].line_pairs)) for p in range(len(problems))]

    def search_for_triangulation(self, kf1, kf2, only_stereo=False, check_ori=False, F12=None):
        """ORBmatcher(., check_ori).SearchForTriangulation(kf1, kf2, F12, .,
        only_stereo), F12 = ComputeF12(kf1, kf2) unless given: (pairs (n, 2) in KF1
        index order, the F12 used)."""
        keep = []
        fin = None if F12 is None else _c(F12, np.float32).reshape(9)
        a, b = _lm_keyframe(kf1, keep), _lm_keyframe(kf2, keep)
        pairs = np.zeros((max(1, a.n), 2), np.int32)
        n, F12 = C.c_int(0), np.zeros((3, 3), np.float32)
        check(lib().orbm_search_for_triangulation(*self._consts(), C.byref(a), C.byref(b),
                                                  None if fin is None else _ptr(fin),
                                                  int(only_stereo), int(check_ori), _ptr(pairs),
                                                  C.byref(n), _ptr(F12)),
              "orbm_search_for_triangulation")
        return pairs[:n.value].copy(), F12


def line_search_for_triangulation(ldesc1, ldesc2):
    """LineMatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, .) over the
    two keyframes' LBD rows: pairs (n, 2) in KF1 line order."""
    a = _c(ldesc1, np.uint8).reshape(-1, 32)
    b = _c(ldesc2, np.uint8).reshape(-1, 32)
    pairs, n = np.zeros((max(1, len(a)), 2), np.int32), C.c_int(0)
    check(lib().orbl_search_for_triangulation(len(a), _ptr(a), len(b), _ptr(b), _ptr(pairs),
                                              C.byref(n)), "orbl_search_for_triangulation")
    return pairs[:n.value].copy()


def search_for_triangulation(camera, scale_factors, level_sigma2, kf1, kf2, only_stereo=False,
                             check_ori=False):
    """LocalMapper(camera, scale_factors, level_sigma2).search_for_triangulation"""
    return LocalMapper(camera, scale_factors, level_sigma2).search_for_triangulation(
        kf1, kf2, only_stereo, check_ori)


_LM_COLS = (_cols("kf_id kf_n kf_nl", np.int32) + _cols("kf_Tcw", np.float32, (16,)) +
            _cols("kps kps_un", KP_DTYPE, (), "P") + _cols("uright depth", np.float32, (), "P", -1) +
            _cols("desc", np.uint8, (32,), "P") + _cols("feat_node", np.int32, (), "P", -1) +
            _cols("has_mp", np.uint8, (), "P", 1) + _cols("mp_xyz", np.float32, (3,), "P") +
            _cols("klines", KEYLINE_DTYPE, (), "LP") + _cols("ldesc", np.uint8, (32,), "LP") +
            _cols("lcoef", np.float64, (3,), "LP") +
            # per problem: the pool indices, then out
            _cols("cur", np.int32) + _cols("neigh", np.int32, (), "NB", -1) +
            _cols("points", LM_RECORD_DTYPE, (), "P") + _cols("lines", LM_LINE_RECORD_DTYPE, (), "NLP") +
            _cols("n_points n_lines", np.int32) + _cols("kf1_point_record", np.int32, (), "P") +
            _cols("kf1_line_record", np.int32, (), "LP") +
            _cols("pairs line_pairs", np.int32, (LM_MAX_NEIGHBOURS,)))


class LmDeviceProblems(PitchedProblems):
    """The pitched device pool of orblm_create_new_map_features_batch_device for
    a list of problems (as LocalMapper.create_new_map_features takes them): run()
    launches without a host round trip, download() synchronises and returns the
    same per-problem results. repeat > 1 runs the list that many times over the
    one pool (problems are indices into it)."""

    def __init__(self, mapper, problems, device=0, repeat=1):
        self.mapper, self.ns = mapper, len(problems) * repeat
        kfs, cur, neigh = [], [], []
        for prob in problems:
            cur.append(len(kfs))
            kfs.append(prob["cur"])
            neigh.append([len(kfs) + k for k in range(len(prob["neigh"]))])
            kfs += list(prob["neigh"])
        cur, neigh = cur * repeat, neigh * repeat
        arrs = [_lm_arrays(k) for k in kfs]
        ns, nls = [a[0] for a in arrs], [a[1] for a in arrs]
        self.n1 = [ns[c] for c in cur]
        self.nl1 = [nls[c] for c in cur]
        self.pitch = P = max([1] + ns)
        self.line_pitch = LP = max([1] + nls)
        cols = {k: [a[2][k] for a in arrs] for k in _LM_POINT_FIELDS + _LM_LINE_FIELDS}
        cols.update(kf_id=[int(k["id"]) for k in kfs], kf_n=ns, kf_nl=nls, kf_Tcw=[k["Tcw"] for k in kfs],
                    cur=cur, neigh=neigh)
        self.pack(_LM_COLS, dict(P=P, LP=LP, NB=LM_MAX_NEIGHBOURS, NLP=LM_MAX_NEIGHBOURS * LP), cols, self.ns, device,
                  LmDeviceBatch, nkf=max(1, len(kfs)), kp_pitch=P, line_pitch=LP)

    def run(self, stream=None):
        check(lib().orblm_create_new_map_features_batch_device(
            *self.mapper._consts(), C.byref(self.batch), self.ns, stream),
            "orblm_create_new_map_features_batch_device")

    def download(self):
        npts, nlns, pts, rec, pairs, lns, lrec, lpairs = self.fetch(
            "n_points", "n_lines", "points", "kf1_point_record", "pairs", "lines", "kf1_line_record",
            "line_pairs")
        return [_lm_outputs(self.n1[s], self.nl1[s], int(npts[s]), pts[s], rec[s], pairs[s],
                            int(nlns[s]), lns[s], lrec[s], lpairs[s]) for s in range(self.ns)]


# ---------------------------------------------------------------------------
# LocalMapping::SearchInNeighbors with ORBmatcher::Fuse as one batched call
# 
# ---------------------------------------------------------------------------
LM_MAX_MAP_KF, LM_MAX_TARGETS = 64, 60
FUSE_REASONS = ("null", "bad", "in_kf", "behind", "out_of_image", "distance", "view",
                "empty_window", "no_match", "added", "replaced", "replaces", "bad_slot")
_SIN_POINT_IO = (("xyz", np.float32, 3), ("normal", np.float32, 3), ("min_dist", np.float32, 1),
                 ("max_dist", np.float32, 1), ("desc", np.uint8, 32), ("ref_kf", np.int32, 1),
                 ("bad", np.uint8, 1), ("n_visible", np.int32, 1), ("n_found", np.int32, 1))
_SIN_POINT_OUT = (("replaced_by", np.int32, 1), ("n_obs", np.int32, 1),
                  ("obs", np.int16, LM_MAX_MAP_KF), ("desc_src", np.int32, 2))


class LmMapKeyFrame(C.Structure):
    """orblm_map_keyframe"""
    _fields_ = ([("id", C.c_int32), ("Tcw", C.c_void_p), ("n", C.c_int32)] +
                [(k, C.c_void_p) for k in ("kps_un", "uright", "desc", "mp", "ordered")])


class LmMap(C.Structure):
    """orblm_map"""
    _fields_ = ([("nkf", C.c_int32), ("kf", C.c_void_p), ("M", C.c_int32)] +
                [(k, C.c_void_p) for k, _, _ in _SIN_POINT_IO + _SIN_POINT_OUT])


class LmSinResult(C.Structure):
    """orblm_sin_result"""
    _fields_ = [("targets", C.c_int32 * LM_MAX_TARGETS), ("n_targets", C.c_int32),
                ("n_fused", C.c_int32 * (LM_MAX_TARGETS + 1)), ("n_candidates", C.c_int32),
                ("conn_w", C.c_int32 * LM_MAX_MAP_KF), ("ordered", C.c_int32 * LM_MAX_MAP_KF),
                ("ordered_w", C.c_int32 * LM_MAX_MAP_KF), ("n_ordered", C.c_int32),
                ("add_conn", C.c_int32 * LM_MAX_MAP_KF)]


class LmSinProblem(C.Structure):
    """orblm_sin_problem"""
    _fields_ = [("map", LmMap), ("cur", C.c_int32), ("result", LmSinResult)]


class LmSinDeviceBatch(C.Structure):
    """orblm_sin_device_batch: pools of keyframes and map points (see include/orbpl.h)"""
    _fields_ = ([(k, C.c_int32) for k in ("nkf", "kp_pitch", "nmp", "list_pitch")] +
                [(k, C.c_void_p) for k in (
                    "d_prob", "d_kf_id", "d_kf_n", "d_kf_Tcw", "d_kps_un", "d_uright", "d_desc",
                    "d_mp", "d_ordered", "d_xyz", "d_normal", "d_min_dist", "d_max_dist",
                    "d_mp_desc", "d_ref_kf", "d_bad", "d_n_visible", "d_n_found", "d_replaced_by",
                    "d_n_obs", "d_obs", "d_desc_src", "d_mark", "d_result", "d_list", "d_search",
                    "d_err")])


def _declare_fuse(L):
    vp, i = C.c_void_p, C.c_int
    L.orblm_search_in_neighbors.argtypes = [vp, vp, vp, i, vp, i]
    L.orblm_search_in_neighbors_batch_device.argtypes = [vp, vp, vp, i, vp, i, vp]
    L.orbm_fuse.argtypes = [vp, vp, vp, i, vp, i, vp, i, C.c_float, C.POINTER(C.c_int), vp, vp, vp]
    L.orblm_debug_search_in_neighbors_phases.argtypes = [vp, vp, vp, i, vp, i, vp, vp]


def _sin_ordered(kf):
    o = [int(x) for x in kf.get("ordered", ())][:LM_MAX_MAP_KF]
    return np.array(o + [-1] * (LM_MAX_MAP_KF - len(o)), np.int32)


def _sin_map_arrays(m):
    """copies of a map dict's arrays (the call writes them): per keyframe
    (Tcw, kps_un, uright, desc, mp, ordered), per point the in/out and out arrays"""
    kfs = []
    for kf in m["kfs"]:
        n = len(np.asarray(kf["uright"]))
        kfs.append(dict(id=int(kf["id"]), n=n, Tcw=_c(kf["Tcw"], np.float32).reshape(16).copy(),
                        kps_un=_c(kf["kps_un"], KP_DTYPE), uright=_c(kf["uright"], np.float32),
                        desc=_c(kf["desc"], np.uint8).reshape(n, 32),
                        mp=np.array(kf["mp"], np.int32).reshape(n), ordered=_sin_ordered(kf)))
    M = len(np.asarray(m["bad"]))
    pts = {}
    for name, dt, w in _SIN_POINT_IO:
        pts[name] = np.array(m[name], dt).reshape((M, w) if w > 1 else (M,))
    for name, dt, w in _SIN_POINT_OUT:
        pts[name] = np.full((M, w) if w > 1 else (M,), -1, dt)
    return kfs, M, pts


def _sin_map_struct(m, keep):
    kfs, M, pts = _sin_map_arrays(m)
    tab = (LmMapKeyFrame * max(1, len(kfs)))(*[
        LmMapKeyFrame(k["id"], _ptr(k["Tcw"]), k["n"], _ptr(k["kps_un"]), _ptr(k["uright"]),
                      _ptr(k["desc"]), _ptr(k["mp"]), _ptr(k["ordered"])) for k in kfs])
    keep += [kfs, pts, tab]
    s = LmMap(len(kfs), C.cast(tab, C.c_void_p), M,
              *[_ptr(pts[name]) for name, _, _ in _SIN_POINT_IO + _SIN_POINT_OUT])
    return s, kfs, pts


def _sin_map_out(kfs, pts):
    out = {k: v for k, v in pts.items()}
    out["mp"] = [k["mp"] for k in kfs]
    return out


def _sin_result_out(out, r):
    nt = r.n_targets
    out.update(targets=np.array(r.targets[:nt], np.int32), n_fused=np.array(r.n_fused[:nt + 1], np.int32),
               n_candidates=int(r.n_candidates), conn_w=np.array(r.conn_w, np.int32),
               n_ordered=int(r.n_ordered), ordered=np.array(r.ordered[:max(0, r.n_ordered)], np.int32),
               ordered_w=np.array(r.ordered_w[:max(0, r.n_ordered)], np.int32),
               add_conn=np.array(r.add_conn, np.int32))
    return out


class NeighborFuser:
    """LocalMapping::SearchInNeighbors (non-monocular, the point half) for many
    independent maps in one launch, and ORBmatcher::Fuse alone. A problem is
    dict(map=map, cur=index of the current keyframe); a map is dict(kfs=[keyframe],
    xyz, normal, min_dist, max_dist, desc, ref_kf, bad, n_visible, n_found), a
    keyframe dict(id, Tcw, kps_un, uright, desc, mp, ordered) with mp the map point
    index per feature (-1 none) and ordered its covisible keyframes as indices into
    kfs. The inputs are not modified: a result holds the updated arrays (mp as a
    list per keyframe) plus replaced_by, n_obs, obs, desc_src and, for
    search_in_neighbors, targets, n_fused, n_candidates, conn_w, ordered,
    ordered_w, n_ordered, add_conn."""

    def __init__(self, camera, scale_factors, level_sigma2):
        self.camera = camera
        self.scale = _c(scale_factors, np.float32)
        self.sigma2 = _c(level_sigma2, np.float32)
        assert len(self.scale) == len(self.sigma2)

    def _consts(self):
        return C.byref(self.camera), _ptr(self.scale), _ptr(self.sigma2), len(self.scale)

    def search_in_neighbors(self, problems):
        keep, P, parts = [], (LmSinProblem * max(1, len(problems)))(), []
        for p, prob in enumerate(problems):
            P[p].map, kfs, pts = _sin_map_struct(prob["map"], keep)
            P[p].cur = int(prob["cur"])
            parts.append((kfs, pts))
        check(lib().orblm_search_in_neighbors(*self._consts(), P, len(problems)),
              "orblm_search_in_neighbors")
        return [_sin_result_out(_sin_map_out(*parts[p]), P[p].result) for p in range(len(problems))]

    def fuse(self, map_, kf, points, th=3.0):
        """ORBmatcher::Fuse(keyframe kf, points, th): (nFused, result) with
        best_idx, best_dist and reason per list entry."""
        keep = []
        s, kfs, pts = _sin_map_struct(map_, keep)
        lst = np.array(points, np.int32).reshape(-1)
        n = len(lst)
        bi, bd, rs = (np.zeros(max(1, n), np.int32) for _ in range(3))
        nf = C.c_int(0)
        check(lib().orbm_fuse(*self._consts(), C.byref(s), int(kf), _ptr(lst), n, float(th),
                              C.byref(nf), _ptr(bi), _ptr(bd), _ptr(rs)), "orbm_fuse")
        out = _sin_map_out(kfs, pts)
        out.update(best_idx=bi[:n].copy(), best_dist=bd[:n].copy(), reason=rs[:n].copy())
        return nf.value, out


def fuse(camera, scale_factors, level_sigma2, map_, kf, points, th=3.0):
    """NeighborFuser(camera, scale_factors, level_sigma2).fuse"""
    return NeighborFuser(camera, scale_factors, level_sigma2).fuse(map_, kf, points, th)


class MapPools:
    """The maps of a list of problems flattened into pooled host arrays (self.host)
    in the layout csrc/map_pool.h states: problem s is the row self.prob[s] =
    (kf0, nkf, mp0, nmp, problem[last]), what no map fills is padding (_PAD, else
    0). No library call before alloc(), which makes the device copies (self.bufs)."""

    # column: (key in a keyframe's dict, dtype, shape of a keyframe's row; "P": the pitch)
    _KF = dict(id=("id", np.int32, ()), n=("n", np.int32, ()), T=("Tcw", np.float32, (16,)),
               kps_un=("kps_un", KP_DTYPE, ("P",)), uright=("uright", np.float32, ("P",)),
               kdesc=("desc", np.uint8, ("P", 32)), mp=("mp", np.int32, ("P",)),
               ordered=("ordered", np.int32, (LM_MAX_MAP_KF,)))
    _PT = {name: (dt, (w,) if w > 1 else ()) for name, dt, w in _SIN_POINT_IO + _SIN_POINT_OUT}
    _PAD = dict(uright=-1, mp=-1, ordered=-1, bad=1, depth=-1, parent=-1)

    def __init__(self, problems, last, kf_cols, pt_cols):
        self.ns = len(problems)
        self.parts = [_sin_map_arrays(p["map"]) for p in problems]
        prob, k0, m0 = [], 0, 0
        for (kfs, M, _), p in zip(self.parts, problems):
            prob.append([k0, len(kfs), m0, M, int(p[last])])
            k0, m0 = k0 + len(kfs), m0 + M
        self.prob = np.array(prob or [[0, 0, 0, 0, 0]], np.int32)
        self.K, self.M = max(1, k0), max(1, m0)
        self.pitch = max([1] + [k["n"] for kfs, _, _ in self.parts for k in kfs])
        self.host = {}
        for c in kf_cols:
            key, dt, row = self._KF[c]
            a = self.column(c, self.K, tuple(self.pitch if x == "P" else x for x in row), dt)
            for g, k in enumerate(k for kfs, _, _ in self.parts for k in kfs):
                a[(g, slice(k["n"])) if "P" in row else g] = k[key]
        for c in pt_cols:
            a = self.column(c, self.M, *self._PT[c][::-1])
            for (_, Mp, pts), row in zip(self.parts, prob):
                a[row[2]:row[2] + Mp] = pts[c]

    def column(self, c, rows, shape, dt):
        """a new host column, all padding"""
        a = self.host[c] = np.zeros((rows,) + shape, dt)
        if c in self._PAD:
            a[...] = self._PAD[c]
        return a

    def alloc(self, device, result, **nbytes):
        """device copies of the host columns, the table, a zeroed error flag, one
        `result` per problem and uninitialised buffers of the given sizes"""
        self.device, self.result = device, result
        mk = lambda a: DeviceBuffer.from_array(a, device)
        b = self.bufs = {k: mk(v) for k, v in self.host.items()}
        b.update(prob=mk(self.prob), err=mk(np.zeros(1, np.int32)),
                 result=DeviceBuffer(max(1, self.ns) * C.sizeof(result), device))
        b.update({c: DeviceBuffer(n, device) for c, n in nbytes.items()})
        return b

    def upload(self):
        for name in self._IO:
            self.bufs[name].upload(self.host[name])

    def fetch(self, error, pt_cols, kf_cols=()):
        """synchronises; per problem: the map's arrays with the device's slots and
        named point columns, the named keyframe columns' rows, the result struct"""
        check(lib().orbpl_device_synchronize(self.device), "orbpl_device_synchronize")
        if int(self.bufs["err"].download(np.int32, 1)[0]):
            raise OrbplError(error)

        def get(c):
            if c in self.host:
                return self.bufs[c].download(self.host[c].dtype, self.host[c].shape)
            return self.bufs[c].download(self._PT[c][0], (self.M,) + self._PT[c][1])   # an out column
        mp, pt, kf = get("mp"), {c: get(c) for c in pt_cols}, {c: get(c) for c in kf_cols}
        sz = C.sizeof(self.result)
        res = self.bufs["result"].download(np.uint8, max(1, self.ns) * sz).tobytes()
        outs = []
        for s, ((kfs, Mp, pts), (k0, nk, m0, _, _)) in enumerate(zip(self.parts, self.prob)):
            out = {name: v.copy() for name, v in pts.items()}
            out.update({c: v[m0:m0 + Mp].copy() for c, v in pt.items()})
            out["mp"] = [mp[k0 + j, :k["n"]].copy() for j, k in enumerate(kfs)]
            outs.append((out, {c: v[k0:k0 + nk].copy() for c, v in kf.items()},
                         self.result.from_buffer_copy(res[s * sz:(s + 1) * sz])))
        return outs


class SinDeviceProblems(MapPools):
    """The device pools of orblm_search_in_neighbors_batch_device for a list of
    problems (as NeighborFuser.search_in_neighbors takes them): run() launches
    without a host round trip, download() synchronises and returns the same
    per-problem results. Every problem owns its range of the pools. A run
    mutates the pools: upload() restores the inputs. device=None: host arrays only."""

    _KF_COLS = ("id", "n", "T", "kps_un", "uright", "kdesc", "mp", "ordered")
    _PT_COLS = tuple(n for n, _, _ in _SIN_POINT_IO)
    _PT_OUT = tuple(n for n, _, _ in _SIN_POINT_OUT)
    _IO = ("mp",) + _PT_COLS

    def __init__(self, fuser, problems, device=0):
        super().__init__(problems, "cur", self._KF_COLS, self._PT_COLS)
        self.fuser = fuser
        self.list_pitch = L = max([self.pitch] + [M for _, M, _ in self.parts])
        if device is not None:
            M, SL = self.M, max(1, self.ns) * L * 4
            b = self.alloc(device, LmSinResult, replaced_by=M * 4, n_obs=M * 4, obs=M * LM_MAX_MAP_KF * 2,
                           desc_src=M * 8, mark=M, list=SL, search=SL)
            self.batch = LmSinDeviceBatch(self.K, self.pitch, M, L, *[b[k].ptr for k in (
                ("prob",) + self._KF_COLS + self._PT_COLS + self._PT_OUT +
                ("mark", "result", "list", "search", "err"))])

    def run(self, stream=None):
        check(lib().orblm_search_in_neighbors_batch_device(
            *self.fuser._consts(), C.byref(self.batch), self.ns, stream),
            "orblm_search_in_neighbors_batch_device")

    def run_phases(self, stream=None):
        """run() with in-kernel time stamps: per problem the microseconds spent in
        the Fuse calls' search phases, in their commit phases, and in the whole
        workgroup (synchronises)"""
        ticks = DeviceBuffer(max(1, self.ns) * 24, self.device)
        check(lib().orblm_debug_search_in_neighbors_phases(
            *self.fuser._consts(), C.byref(self.batch), self.ns, stream, ticks.ptr),
            "orblm_debug_search_in_neighbors_phases")
        check(lib().orbpl_device_synchronize(self.device), "orbpl_device_synchronize")
        return ticks.download(np.int64, (max(1, self.ns), 3))[:self.ns] / 100.0

    def download(self):
        return [_sin_result_out(out, r) for out, _, r in self.fetch(
            "orblm_search_in_neighbors_batch_device: candidate list overflow", self._PT_COLS + self._PT_OUT)]


# ---------------------------------------------------------------------------
# LocalMapping::KeyFrameCulling and MapPointCulling / MapLineCulling as batched
# calls
# ---------------------------------------------------------------------------
LM_MAX_CULL_LIST, LM_MAX_LINES = 63, 256
KFC_ACTIONS = ("kept", "culled", "first", "deferred")
RECENT_REASONS = ("was_bad", "found_ratio", "few_observations", "aged_out", "stays")


class LmKfcResult(C.Structure):
    """orblm_kfc_result"""
    _fields_ = [("list", C.c_int32 * LM_MAX_CULL_LIST), ("n_list", C.c_int32),
                ("n_mps", C.c_int32 * LM_MAX_CULL_LIST), ("n_redundant", C.c_int32 * LM_MAX_CULL_LIST),
                ("action", C.c_int32 * LM_MAX_CULL_LIST), ("n_points_bad", C.c_int32)]


class LmKfcProblem(C.Structure):
    """orblm_kfc_problem"""
    _fields_ = ([("map", LmMap), ("cur", C.c_int32)] +
                [(k, C.c_void_p) for k in ("depth", "conn_w", "ordered", "parent", "not_erase", "kf_bad",
                                           "to_be_erased", "Tcp")] + [("result", LmKfcResult)])


class LmKfcDeviceBatch(C.Structure):
    """orblm_kfc_device_batch: pools of keyframes, map points and the graph (see include/orbpl.h)"""
    _fields_ = ([(k, C.c_int32) for k in ("nkf", "kp_pitch", "nmp")] +
                [(k, C.c_void_p) for k in (
                    "d_prob", "d_kf_id", "d_kf_n", "d_kf_Tcw", "d_kps_un", "d_uright", "d_depth", "d_mp",
                    "d_conn_w", "d_ordered", "d_parent", "d_not_erase", "d_kf_bad", "d_to_be_erased",
                    "d_Tcp", "d_ref_kf", "d_bad", "d_n_obs", "d_obs", "d_result", "d_err")])


class LmRecentProblem(C.Structure):
    """orblm_recent_problem"""
    _fields_ = [("map", LmMap), ("kf_bad", C.c_void_p), ("cur_id", C.c_int32), ("first_kf", C.c_void_p),
                ("recent", C.c_void_p), ("n_recent", C.c_int32), ("reason", C.c_void_p), ("L", C.c_int32),
                ("nl", C.c_void_p), ("ml", C.c_void_p), ("line_bad", C.c_void_p),
                ("line_n_visible", C.c_void_p), ("line_n_found", C.c_void_p),
                ("line_first_kf", C.c_void_p), ("line_n_obs", C.c_void_p), ("recent_lines", C.c_void_p),
                ("n_recent_lines", C.c_int32), ("line_reason", C.c_void_p)]


def _declare_cull(L):
    vp, i = C.c_void_p, C.c_int
    L.orblm_keyframe_culling.argtypes = [vp, i, vp, i]
    L.orblm_keyframe_culling_batch_device.argtypes = [vp, vp, i, vp]
    L.orblm_cull_recent.argtypes = [i, vp, i]


def _kfc_graph_arrays(prob, kfs):
    """copies of a culling problem's graph state (the call writes them)"""
    K = len(kfs)
    ordered = np.full((K, LM_MAX_MAP_KF), -1, np.int32)
    for k, o in enumerate(prob["ordered"]):
        o = [int(x) for x in o][:LM_MAX_MAP_KF]
        ordered[k, :len(o)] = o
    depth = [_c(d, np.float32).reshape(-1).copy() for d in prob["depth"]]
    assert len(depth) == K and all(len(d) == k["n"] for d, k in zip(depth, kfs))
    Tcp = np.array(prob["Tcp"], np.float32).reshape(K, 16) if "Tcp" in prob else np.zeros((K, 16), np.float32)
    return dict(depth=depth, conn_w=np.array(prob["conn_w"], np.int32).reshape(K, K), ordered=ordered,
                parent=np.array(prob["parent"], np.int32).reshape(K),
                not_erase=np.array(prob["not_erase"], np.uint8).reshape(K),
                kf_bad=np.array(prob["kf_bad"], np.uint8).reshape(K),
                to_be_erased=np.zeros(K, np.uint8), Tcp=Tcp)


def _kfc_result_out(out, g, r):
    n = r.n_list
    out.update({k: g[k] for k in ("conn_w", "ordered", "parent", "kf_bad", "to_be_erased", "Tcp")})
    out.update(list=np.array(r.list[:n], np.int32), n_mps=np.array(r.n_mps[:n], np.int32),
               n_redundant=np.array(r.n_redundant[:n], np.int32), action=np.array(r.action[:n], np.int32),
               n_points_bad=int(r.n_points_bad))
    return out


class MapCuller:
    """LocalMapping::KeyFrameCulling and MapPointCulling / MapLineCulling
    (non-monocular) for many independent maps in one launch each. A map is the
    dict NeighborFuser takes (a keyframe's `ordered` is not read here).

    keyframes(problems): a problem is dict(map, cur, depth=[mvDepth per keyframe],
    conn_w=(nkf, nkf) weights, ordered=[list per keyframe], parent, not_erase,
    kf_bad[, Tcp]). A result holds the updated map arrays (as NeighborFuser's),
    conn_w, ordered (nkf, 64; -1 ends a list), parent, kf_bad, to_be_erased, Tcp
    and list, n_mps, n_redundant, action (KFC_ACTIONS), n_points_bad.

    recent(problems): a problem is dict(map, cur_id, first_kf, recent[, kf_bad],
    lines=dict(ml=[slot array per keyframe], bad, n_visible, n_found, first_kf,
    n_obs), recent_lines). A result holds the updated map arrays, recent, reason
    (RECENT_REASONS, per entry as passed in), ml, line_bad, recent_lines,
    line_reason. The inputs are not modified."""

    def __init__(self, camera, scale_factors, level_sigma2):
        self.camera = camera
        self.scale = _c(scale_factors, np.float32)
        self.sigma2 = _c(level_sigma2, np.float32)
        assert len(self.scale) == len(self.sigma2)

    def keyframes(self, problems):
        keep, P, parts = [], (LmKfcProblem * max(1, len(problems)))(), []
        for p, prob in enumerate(problems):
            P[p].map, kfs, pts = _sin_map_struct(prob["map"], keep)
            P[p].cur = int(prob["cur"])
            g = _kfc_graph_arrays(prob, kfs)
            dptr = (C.c_void_p * max(1, len(kfs)))(*[_ptr(d) for d in g["depth"]])
            keep += [g, dptr]
            P[p].depth = C.cast(dptr, C.c_void_p)
            for name in ("conn_w", "ordered", "parent", "not_erase", "kf_bad", "to_be_erased", "Tcp"):
                setattr(P[p], name, _ptr(g[name]))
            parts.append((kfs, pts, g))
        check(lib().orblm_keyframe_culling(C.byref(self.camera), len(self.scale), P, len(problems)),
              "orblm_keyframe_culling")
        return [_kfc_result_out(_sin_map_out(kfs, pts), g, P[p].result)
                for p, (kfs, pts, g) in enumerate(parts)]

    def keyframes_device(self, pools, stream=None):
        """orblm_keyframe_culling_batch_device over a KfcDeviceProblems: no host round trip"""
        check(lib().orblm_keyframe_culling_batch_device(
            C.byref(self.camera), C.byref(pools.batch), pools.ns, stream),
            "orblm_keyframe_culling_batch_device")

    def recent(self, problems):
        keep, P, parts = [], (LmRecentProblem * max(1, len(problems)))(), []
        i32 = lambda a: np.array(a, np.int32).reshape(-1)
        for p, prob in enumerate(problems):
            q = P[p]
            q.map, kfs, pts = _sin_map_struct(prob["map"], keep)
            K = len(kfs)
            ln = prob["lines"]
            a = dict(first_kf=i32(prob["first_kf"]), recent=i32(prob["recent"]),
                     recent_lines=i32(prob["recent_lines"]), line_bad=np.array(ln["bad"], np.uint8).reshape(-1),
                     line_n_visible=i32(ln["n_visible"]), line_n_found=i32(ln["n_found"]),
                     line_first_kf=i32(ln["first_kf"]), line_n_obs=i32(ln["n_obs"]),
                     ml=[i32(x) for x in ln["ml"]])
            assert len(a["ml"]) == K
            a["nl"] = np.array([len(x) for x in a["ml"]], np.int32)
            a["reason"] = np.zeros(len(a["recent"]), np.int32)
            a["line_reason"] = np.zeros(len(a["recent_lines"]), np.int32)
            mlptr = (C.c_void_p * max(1, K))(*[_ptr(x) for x in a["ml"]])
            keep += [a, mlptr]
            if "kf_bad" in prob:
                a["kf_bad"] = np.array(prob["kf_bad"], np.uint8).reshape(K)
                q.kf_bad = _ptr(a["kf_bad"])
            q.cur_id, q.L = int(prob["cur_id"]), len(a["line_bad"])
            q.n_recent, q.n_recent_lines = len(a["recent"]), len(a["recent_lines"])
            q.ml = C.cast(mlptr, C.c_void_p)
            for name in ("first_kf", "recent", "reason", "nl", "line_bad", "line_n_visible", "line_n_found",
                         "line_first_kf", "line_n_obs", "recent_lines", "line_reason"):
                setattr(q, name, _ptr(a[name]))
            parts.append((kfs, pts, a))
        check(lib().orblm_cull_recent(len(self.scale), P, len(problems)), "orblm_cull_recent")
        outs = []
        for p, (kfs, pts, a) in enumerate(parts):
            out = _sin_map_out(kfs, pts)
            out.update(recent=a["recent"][:P[p].n_recent].copy(), reason=a["reason"], ml=a["ml"],
                       line_bad=a["line_bad"], recent_lines=a["recent_lines"][:P[p].n_recent_lines].copy(),
                       line_reason=a["line_reason"])
            outs.append(out)
        return outs


class KfcDeviceProblems(MapPools):
    """The device pools of orblm_keyframe_culling_batch_device for a list of
    problems (as MapCuller.keyframes takes them): the map's pools, plus depth at
    kp_pitch and the graph arrays (conn_w rows at a pitch of 64).
    MapCuller.keyframes_device(pools) launches without a host round trip,
    download() synchronises and returns the same per-problem results. A run
    mutates the pools: upload() restores the inputs."""

    _KF_COLS = ("id", "n", "T", "kps_un", "uright", "mp")
    _PT_COLS, _PT_OUT = ("ref_kf", "bad"), ("n_obs", "obs")
    _GRAPH = ("conn_w", "ordered", "parent", "kf_bad", "Tcp")
    _IO = ("mp",) + _GRAPH + _PT_COLS

    def __init__(self, culler, problems, device=0):
        super().__init__(problems, "cur", self._KF_COLS, self._PT_COLS)
        self.culler, K, M, W = culler, self.K, self.M, LM_MAX_MAP_KF
        self.graphs = [_kfc_graph_arrays(p, kfs) for p, (kfs, _, _) in zip(problems, self.parts)]
        h = {c: self.column(c, K, shape, dt) for c, shape, dt in (
            ("depth", (self.pitch,), np.float32), ("conn_w", (W,), np.int32), ("ordered", (W,), np.int32),
            ("parent", (), np.int32), ("not_erase", (), np.uint8), ("kf_bad", (), np.uint8),
            ("Tcp", (16,), np.float32))}
        for (kfs, _, _), g, (k0, nk, _, _, _) in zip(self.parts, self.graphs, self.prob):
            h["conn_w"][k0:k0 + nk, :nk] = g["conn_w"]
            for name in ("ordered", "parent", "not_erase", "kf_bad", "Tcp"):
                h[name][k0:k0 + nk] = g[name]
            for j, k in enumerate(kfs):
                h["depth"][k0 + j, :k["n"]] = g["depth"][j]
        if device is not None:
            b = self.alloc(device, LmKfcResult, to_be_erased=K, n_obs=M * 4, obs=M * W * 2)
            self.batch = LmKfcDeviceBatch(K, self.pitch, M, *[b[k].ptr for k in (
                "prob", "id", "n", "T", "kps_un", "uright", "depth", "mp", "conn_w", "ordered", "parent",
                "not_erase", "kf_bad", "to_be_erased", "Tcp", "ref_kf", "bad", "n_obs", "obs", "result", "err")])

    def run(self, stream=None):
        self.culler.keyframes_device(self, stream)

    def download(self):
        parts = self.fetch("orblm_keyframe_culling_batch_device: a problem lies outside the pools",
                           self._PT_COLS + self._PT_OUT, self._GRAPH)
        tbe = self.bufs["to_be_erased"].download(np.uint8, self.K)
        outs = []
        for (out, g, r), (k0, nk, _, _, _) in zip(parts, self.prob):
            g.update(conn_w=g["conn_w"][:, :nk].copy(), to_be_erased=tbe[k0:k0 + nk].copy())
            outs.append(_kfc_result_out(out, g, r))
        return outs


# the functions that set the library's argtypes, in file order: lib() walks them once
_DECLARE = (_declare_core, _declare_track, _declare_lines, _declare_voc, _declare_reloc, _declare_reloc_device,
            _declare_localmap, _declare_fuse, _declare_cull)
