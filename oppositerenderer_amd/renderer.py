"""Python mirror of OppositeRenderer's `OptixRenderer` (RenderEngine/renderer/OptixRenderer.h:21-43)
and `StandaloneRenderManager`'s progressive loop (Standalone/StandaloneRenderManager.cpp:75-140),
bound to liborx.so through the C ABI in include/orx.h.

There is no CPU fallback: if liborx.so is missing or no HIP device is present
every entry point raises.  The oracle under oracle/ is test infrastructure and
is never imported here.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _abi
from .scenes import Camera, Scene

_HERE = os.path.dirname(os.path.abspath(__file__))
# ORX_LIB selects an alternative in-tree build (e.g. liborx_fp32.so) for A/B measurements
LIB_PATH = os.environ.get("ORX_LIB") or os.path.join(_HERE, "liborx.so")
_lib = None


class OrxError(RuntimeError):
    """Raised where the reference throws std::exception (OptixRenderer.cpp:816-820)."""

    def __init__(self, status, message):
        super().__init__(f"[orx status {status}] {message}")
        self.status = status


def load_library(path: str = LIB_PATH):
    """Load liborx.so (built in-tree by __graft_entry__.build / `make -C oppositerenderer_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise OrxError(_abi.ORX_ERR_STATE,
                       f"liborx.so not found at {path}; build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(path)
    _abi.declare_common(lib, "orx")
    lib.orx_default_config.argtypes = [C.POINTER(_abi.OrxConfig)]
    lib.orx_default_config.restype = None
    lib.orx_create.argtypes = [C.c_int, C.POINTER(_abi.OrxConfig), C.POINTER(C.c_void_p)]
    lib.orx_create.restype = C.c_int
    lib.orx_get_output_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.orx_get_output_device.restype = C.c_int
    for name in ("orx_width", "orx_height", "orx_emitted_photons_per_iteration"):
        getattr(lib, name).argtypes = [C.c_void_p]
        getattr(lib, name).restype = C.c_uint32
    lib.orx_output_bytes.argtypes = [C.c_void_p]
    lib.orx_output_bytes.restype = C.c_size_t
    lib.orx_set_shard.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.orx_set_shard.restype = C.c_int
    lib.orx_reset_timing.argtypes = [C.c_void_p]
    lib.orx_reset_timing.restype = C.c_int
    lib.orx_ppm_pipelined.argtypes = [C.c_void_p]
    lib.orx_ppm_pipelined.restype = C.c_int
    lib.orx_ppm_grid_schedule.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.orx_ppm_grid_schedule.restype = C.c_int
    lib.orx_set_iteration_pipelining.argtypes = [C.c_void_p, C.c_int]
    lib.orx_set_iteration_pipelining.restype = C.c_int
    lib.orx_stream.argtypes = [C.c_void_p]
    lib.orx_stream.restype = C.c_void_p
    # render groups (orx_create_group)
    vp = C.c_void_p
    lib.orx_default_group_config.argtypes, lib.orx_default_group_config.restype = [C.POINTER(_abi.OrxGroupConfig)], None
    lib.orx_create_group.argtypes = [C.c_uint32, C.POINTER(C.c_int), C.POINTER(_abi.OrxConfig),
                                     C.POINTER(_abi.OrxGroupConfig), C.POINTER(vp)]
    lib.orx_create_group.restype = C.c_int
    lib.orx_group_init_scene.argtypes, lib.orx_group_init_scene.restype = [vp, C.POINTER(_abi.OrxScene)], C.c_int
    lib.orx_group_render_next_iteration.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_float, C.c_int,
                                                    C.POINTER(_abi.OrxRequest)]
    lib.orx_group_render_next_iteration.restype = C.c_int
    lib.orx_group_get_output.argtypes, lib.orx_group_get_output.restype = [vp, vp, C.c_size_t], C.c_int
    lib.orx_group_world.argtypes, lib.orx_group_world.restype = [vp], C.c_uint32
    lib.orx_group_renderer.argtypes, lib.orx_group_renderer.restype = [vp, C.c_uint32], vp
    lib.orx_group_pipelined.argtypes, lib.orx_group_pipelined.restype = [vp], C.c_int
    lib.orx_group_comm_name.argtypes, lib.orx_group_comm_name.restype = [vp], C.c_char_p
    lib.orx_group_last_error.argtypes, lib.orx_group_last_error.restype = [vp], C.c_char_p
    lib.orx_group_destroy.argtypes, lib.orx_group_destroy.restype = [vp], None
    lib.orx_batch_seed.argtypes, lib.orx_batch_seed.restype = [C.c_uint32, C.c_uint32, C.c_uint64], C.c_uint32
    lib.orx_group_debug_reduce_scatter.argtypes = [vp, vp, C.c_size_t, vp]
    lib.orx_group_debug_reduce_scatter.restype = C.c_int
    lib.orx_group_debug_reduce.argtypes, lib.orx_group_debug_reduce.restype = [vp, vp, C.c_size_t, vp], C.c_int
    # photon slabs behind the group (orx_group_config.photon_partition); orx_slab_plan needs no device
    lib.orx_slab_histogram_words.argtypes, lib.orx_slab_histogram_words.restype = [C.c_uint32], C.c_size_t
    lib.orx_slab_plan.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.POINTER(C.c_uint32), vp, vp, vp]
    lib.orx_slab_plan.restype = C.c_int
    lib.orx_group_slab_plan.argtypes = [vp, C.POINTER(C.c_uint32), vp, vp]
    lib.orx_group_slab_plan.restype = C.c_int
    lib.orx_group_debug_all_to_all.argtypes, lib.orx_group_debug_all_to_all.restype = [vp, vp, vp, vp], C.c_int
    # the VCM MIS constants (pure, no device)
    fp = C.POINTER(C.c_float)
    lib.orx_vcm_mis_factors.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_int, fp, fp, fp]
    lib.orx_vcm_mis_factors.restype = C.c_int
    # checkpoint / resume: the codec (pure, no device), one renderer, groups
    sp = C.POINTER(_abi.OrxStateInfo)
    lib.orx_state_info_read.argtypes, lib.orx_state_info_read.restype = [vp, C.c_size_t, sp], C.c_int
    lib.orx_state_packed_bytes.argtypes, lib.orx_state_packed_bytes.restype = [sp], C.c_size_t
    lib.orx_state_pack.argtypes, lib.orx_state_pack.restype = [sp, vp, vp, vp, C.c_size_t], C.c_int
    lib.orx_state_unpack.argtypes = [vp, C.c_size_t, C.POINTER(vp), C.POINTER(vp)]
    lib.orx_state_unpack.restype = C.c_int
    lib.orx_scene_key.argtypes, lib.orx_scene_key.restype = [C.POINTER(_abi.OrxScene)], C.c_uint64
    for prefix in ("orx", "orx_group"):
        f = getattr(lib, prefix + "_state_bytes")
        f.argtypes, f.restype = [vp], C.c_size_t
        f = getattr(lib, prefix + "_save_state")
        f.argtypes, f.restype = [vp, vp, C.c_size_t], C.c_int
        f = getattr(lib, prefix + "_restore_state")
        f.argtypes, f.restype = [vp, vp, C.c_size_t], C.c_int
    # convergence estimate and display resolve (orx_display_convert is pure, no device)
    cp = C.POINTER(_abi.OrxConvergence)
    for prefix in ("orx", "orx_group"):
        f = getattr(lib, prefix + "_set_convergence")
        f.argtypes, f.restype = [vp, C.c_int], C.c_int
        f = getattr(lib, prefix + "_get_convergence")
        f.argtypes, f.restype = [vp, C.c_float, C.c_float, cp, vp, C.c_size_t], C.c_int
        f = getattr(lib, prefix + "_get_display")
        f.argtypes, f.restype = [vp, C.c_float, C.c_float, C.c_int32, vp, C.c_size_t], C.c_int
    lib.orx_display_convert.argtypes = [vp, C.c_size_t, C.c_float, C.c_float, C.c_int32, vp]
    lib.orx_display_convert.restype = C.c_int
    _lib = lib
    return lib


EXPORTED_SYMBOLS = (
    "orx_default_config", "orx_create", "orx_init_scene", "orx_render_next_iteration", "orx_get_output",
    "orx_get_output_device", "orx_width", "orx_height", "orx_output_bytes", "orx_emitted_photons_per_iteration",
    "orx_last_error", "orx_destroy", "orx_read_buffer", "orx_get_stats", "orx_reset_timing", "orx_ppm_pipelined",
    "orx_set_iteration_pipelining", "orx_ppm_grid_schedule",
    "orx_set_shard", "orx_set_ppm_pipeline",
    "orx_stream",
    "orx_default_group_config", "orx_create_group", "orx_group_init_scene", "orx_group_render_next_iteration",
    "orx_group_get_output", "orx_group_world", "orx_group_renderer", "orx_group_pipelined", "orx_group_comm_name",
    "orx_group_last_error", "orx_group_destroy", "orx_batch_seed", "orx_group_debug_reduce_scatter",
    "orx_group_debug_reduce", "orx_slab_plan", "orx_group_slab_plan", "orx_group_debug_all_to_all",
    "orx_vcm_mis_factors",
    "orx_state_info_read", "orx_state_packed_bytes", "orx_state_pack", "orx_state_unpack", "orx_scene_key",
    "orx_state_bytes", "orx_save_state", "orx_restore_state",
    "orx_group_state_bytes", "orx_group_save_state", "orx_group_restore_state",
    "orx_set_convergence", "orx_get_convergence", "orx_display_convert", "orx_get_display",
    "orx_group_set_convergence", "orx_group_get_convergence", "orx_group_get_display",
)


def display_convert(sum_rgb, inv_iterations: float, inv_gamma: float = 1.0 / 2.2,
                    fmt: int = _abi.DISPLAY_RGBA8) -> np.ndarray:
    """orx_display_convert on the host (no device): a running sum [...][3] float32 -> [...][4] uint8, the bytes
    getDisplayBuffer gives for the same sum."""
    lib = load_library()
    src = np.ascontiguousarray(sum_rgb, np.float32)
    assert src.shape[-1] == 3
    dst = np.empty(src.shape[:-1] + (4,), np.uint8)
    st = lib.orx_display_convert(src.ctypes.data, src.size // 3, float(inv_iterations), float(inv_gamma), int(fmt),
                                 dst.ctypes.data)
    if st != _abi.ORX_OK:
        raise OrxError(st, "orx_display_convert: factors must be finite and > 0, the format RGBA8 or BGRA8")
    return dst


def _get_convergence(obj, prefix: str, floor: float, threshold: float, tiles: bool):
    lib = obj._lib
    out = _abi.OrxConvergence()
    W, H = obj._frame_size()
    tx, ty = -(-W // _abi.CONV_TILE), -(-H // _abi.CONV_TILE)
    te = np.empty((ty, tx), np.float32) if tiles else None
    obj._check(getattr(lib, prefix + "_get_convergence")(obj._h, float(floor), float(threshold), C.byref(out),
                                                         te.ctypes.data if tiles else None, te.nbytes if tiles else 0))
    return (out, te) if tiles else out


def state_info(blob) -> _abi.OrxStateInfo:
    """The header of a checkpoint blob (orx_state_info_read: magic, version, sizes and checksums are checked);
    raises OrxError(ORX_ERR_INVALID_ARGUMENT) for anything that is not one.  Needs no device."""
    lib = load_library()
    buf = bytes(blob)
    info = _abi.OrxStateInfo()
    st = lib.orx_state_info_read(buf, len(buf), C.byref(info))
    if st != _abi.ORX_OK:
        raise OrxError(st, "not a state blob (truncated, damaged or of another format version)")
    return info


def _save_state(obj, prefix: str) -> bytes:
    lib = obj._lib
    n = getattr(lib, prefix + "_state_bytes")(obj._h)
    buf = C.create_string_buffer(max(n, 1))
    obj._check(getattr(lib, prefix + "_save_state")(obj._h, buf, n))
    return buf.raw[:n]


class RenderRequestDetails:
    """RenderServerRenderRequestDetails (clientserver/RenderServerRenderRequestDetails.h:15-33)."""

    def __init__(self, camera: Camera, scene_name: str, render_method: int, width: int, height: int,
                 ppm_alpha: float = 2.0 / 3.0):
        self.camera = camera
        self.scene_name = scene_name
        self.render_method = render_method
        self.width = width
        self.height = height
        self.ppm_alpha = ppm_alpha

    def to_abi(self) -> _abi.OrxRequest:
        r = _abi.OrxRequest()
        r.camera = self.camera.to_abi()
        r.method = self.render_method
        r.width = self.width
        r.height = self.height
        r.ppm_alpha = self.ppm_alpha
        return r


class OptixRenderer:
    """Drop-in for the reference's OptixRenderer, HIP/gfx950 underneath.

    initialize(device)                -> OptixRenderer::initialize(ComputeDevice)   (OptixRenderer.cpp:113-400)
    initScene(scene)                  -> OptixRenderer::initScene(IScene&)           (:436-485)
    renderNextIteration(...)          -> OptixRenderer::renderNextIteration          (:507-821)
    getOutputBuffer()                 -> OptixRenderer::getOutputBuffer              (:860-865)
    getWidth/getHeight/getScreenBufferSizeBytes                                      (:850-870)
    """

    PHOTON_LAUNCH_WIDTH = 1024
    PHOTON_LAUNCH_HEIGHT = 1024
    EMITTED_PHOTONS_PER_ITERATION = PHOTON_LAUNCH_WIDTH * PHOTON_LAUNCH_HEIGHT

    def __init__(self, config: _abi.OrxConfig | None = None):
        self._lib = load_library()
        self._cfg = config if config is not None else _abi.default_config()
        self._h = None
        self._initialized = False
        self._scene_abi = None

    # -- error plumbing ------------------------------------------------
    def _check(self, status):
        if status != _abi.ORX_OK:
            msg = self._lib.orx_last_error(self._h).decode() if self._h else "orx call failed"
            raise OrxError(status, msg)

    # -- reference API -------------------------------------------------
    def initialize(self, device: int = 0):
        if self._initialized:
            raise OrxError(_abi.ORX_ERR_STATE, "ERROR: Multiple OptixRenderer::initialize!")
        h = C.c_void_p()
        st = self._lib.orx_create(int(device), C.byref(self._cfg), C.byref(h))
        if st != _abi.ORX_OK:
            raise OrxError(st, f"orx_create failed on HIP device {device}")
        self._h = h
        self._initialized = True
        return self

    def initScene(self, scene: Scene):
        if not self._initialized:
            raise OrxError(_abi.ORX_ERR_STATE, "Cannot initialize scene before OptixRenderer.")
        self._scene_abi = scene.to_abi()
        self._scene = scene
        self._check(self._lib.orx_init_scene(self._h, C.byref(self._scene_abi)))

    def renderNextIteration(self, iterationNumber: int, localIterationNumber: int, PPMRadius: float,
                            createOutput: bool, details: RenderRequestDetails):
        if not self._initialized:
            raise OrxError(_abi.ORX_ERR_STATE, "Traced before OptixRenderer was initialized.")
        req = details.to_abi() if isinstance(details, RenderRequestDetails) else details
        self._check(self._lib.orx_render_next_iteration(self._h, int(iterationNumber), int(localIterationNumber),
                                                         float(PPMRadius), int(bool(createOutput)), C.byref(req)))

    def getOutputBuffer(self, out: np.ndarray | None = None) -> np.ndarray:
        """W*H*3 float32 SUM over local iterations (divide by N to display, RenderWidget.cpp:197)."""
        n = self.getScreenBufferSizeBytes()
        if out is None:
            out = np.empty(n // 4, np.float32)
        assert out.nbytes >= n and out.dtype == np.float32 and out.flags.c_contiguous
        self._check(self._lib.orx_get_output(self._h, out.ctypes.data, out.nbytes))
        return out[: n // 4].reshape(self.getHeight(), self.getWidth(), 3)

    def getOutputBufferDevice(self, dst_ptr: int, nbytes: int):
        """Device-to-device copy of the accumulation buffer (multi-GPU harness)."""
        self._check(self._lib.orx_get_output_device(self._h, C.c_void_p(dst_ptr), nbytes))

    def getWidth(self) -> int:
        return self._lib.orx_width(self._h)

    def getHeight(self) -> int:
        return self._lib.orx_height(self._h)

    def getScreenBufferSizeBytes(self) -> int:
        return self._lib.orx_output_bytes(self._h)

    def emittedPhotonsPerIteration(self) -> int:
        return self._lib.orx_emitted_photons_per_iteration(self._h)

    # -- extensions ----------------------------------------------------
    def set_shard(self, rank: int, world: int):
        self._check(self._lib.orx_set_shard(self._h, rank, world))

    def stream_handle(self) -> int:
        return self._lib.orx_stream(self._h) or 0

    def read_buffer(self, buf_id: int, dtype=np.float32) -> np.ndarray:
        n = C.c_size_t()
        self._check(self._lib.orx_read_buffer(self._h, buf_id, None, 0, C.byref(n)))
        out = np.empty(n.value // np.dtype(dtype).itemsize, dtype=dtype)
        self._check(self._lib.orx_read_buffer(self._h, buf_id, out.ctypes.data, n.value, C.byref(n)))
        return out

    def stats(self) -> _abi.OrxStats:
        s = _abi.OrxStats()
        self._check(self._lib.orx_get_stats(self._h, C.byref(s)))
        return s

    def pipelined(self) -> bool:
        """Whether the last iteration overlapped part of its work with the next one's passes (PPM: the
        gather + output; VCM: the deferred shadow rays + colours)."""
        return bool(self._lib.orx_ppm_pipelined(self._h))

    def grid_schedule(self):
        """The pipelined PPM grid build's schedule (orx_ppm_grid_schedule): (0 synchronous / 1 asynchronous /
        -1 not chosen yet, (photon + grid ms, gather ms) as measured, or zeros)."""
        ms = (C.c_float * 2)()
        mode = self._lib.orx_ppm_grid_schedule(self._h, ms)
        return mode, (float(ms[0]), float(ms[1]))

    def set_iteration_pipelining(self, mode: int):
        """Single-device PPM pipelining and VCM shadow-ray overlap: 1 on, 0 serial passes, -1 the
        ORX_PIPELINE default."""
        self._check(self._lib.orx_set_iteration_pipelining(self._h, mode))

    def _frame_size(self):
        return self.getWidth(), self.getHeight()

    def setConvergence(self, enable: bool):
        """orx_set_convergence: per-pixel statistics of the iterations' luminances (off by default); switching
        on starts a new window on the current sum."""
        self._check(self._lib.orx_set_convergence(self._h, int(bool(enable))))

    def getConvergence(self, floor: float = 1e-3, threshold: float = 0.05, tiles: bool = False):
        """orx_get_convergence -> OrxConvergence, or (OrxConvergence, tile means [tiles_y][tiles_x]) with
        tiles=True.  The error is the relative standard error of a pixel's mean luminance, its denominator
        at least `floor`."""
        return _get_convergence(self, "orx", floor, threshold, tiles)

    def getDisplayBuffer(self, inv_iterations: float, inv_gamma: float = 1.0 / 2.2,
                         fmt: int = _abi.DISPLAY_RGBA8) -> np.ndarray:
        """orx_get_display: the own rows' 8-bit image [rows][W][4], resolved on the device."""
        n = C.c_size_t()
        self._check(self._lib.orx_read_buffer(self._h, _abi.BUF_OUTPUT, None, 0, C.byref(n)))
        out = np.empty(n.value // 12 * 4, np.uint8)
        self._check(self._lib.orx_get_display(self._h, float(inv_iterations), float(inv_gamma), int(fmt),
                                              out.ctypes.data, out.nbytes))
        return out.reshape(-1, self.getWidth(), 4)

    def saveState(self) -> bytes:
        """The progressive state (RNG, running sum, the last iteration's numbers) as one blob (orx_save_state)."""
        return _save_state(self, "orx")

    def restoreState(self, blob):
        """orx_restore_state: after initScene; the next renderNextIteration of the blob's size with
        localIterationNumber != 0 continues the saved render."""
        buf = bytes(blob)
        self._check(self._lib.orx_restore_state(self._h, buf, len(buf)))

    def reset_timing(self):
        """Start a new timed region for stats().pass_ms / *_total (HIP events, no host timing)."""
        self._check(self._lib.orx_reset_timing(self._h))

    def destroy(self):
        if self._h:
            self._lib.orx_destroy(self._h)
            self._h = None
            self._initialized = False

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def next_ppm_radius(radius: float, iteration: int, alpha: float = 2.0 / 3.0) -> float:
    """StandaloneRenderManager.cpp:105-107: r^2 <- r^2 (i + alpha) / (i + 1), in double."""
    r2 = radius * radius
    return math.sqrt(r2 * (iteration + alpha) / float(iteration + 1))


class StandaloneRenderManager:
    """Headless restatement of Standalone/StandaloneRenderManager.cpp:55-140: one
    renderNextIteration per call, PPM radius schedule with alpha = 2/3, output
    fetched every `output_every` iterations (5 in the reference)."""

    PPM_ALPHA = 2.0 / 3.0

    def __init__(self, renderer, scene: Scene, method: int, width: int, height: int, camera: Camera | None = None,
                 output_every: int = 5):
        self.renderer = renderer
        self.scene = scene
        self.camera = camera or scene.default_camera
        self.camera.set_aspect_ratio(float(np.float32(width) / np.float32(height)))
        self.details = RenderRequestDetails(self.camera, scene.name, method, width, height, self.PPM_ALPHA)
        self.radius = scene.initial_ppm_radius()
        self.iteration = 0
        self.output_every = output_every
        self._compiled = False

    def render_next_iteration(self):
        if not self._compiled:
            self.renderer.initScene(self.scene)
            self._compiled = True
        out = self.iteration % self.output_every == 0
        self.renderer.renderNextIteration(self.iteration, self.iteration, self.radius, out, self.details)
        self.radius = next_ppm_radius(self.radius, self.iteration, self.PPM_ALPHA)
        self.iteration += 1

    def save(self, path):
        """Write the renderer's (or group's) state blob to `path`."""
        with open(path, "wb") as f:
            f.write(self.renderer.saveState())

    def resume(self, path):
        """Restore the blob at `path`; the next iteration continues its schedule: the iteration after the
        header's, with the radius that follows the header's (the header holds the float the renderer was
        given, so the double-precision schedule goes on from that rounding)."""
        with open(path, "rb") as f:
            blob = f.read()
        info = state_info(blob)
        if not self._compiled:
            self.renderer.initScene(self.scene)
            self._compiled = True
        self.renderer.restoreState(blob)
        self.iteration = int(info.iteration_number) + 1
        self.radius = next_ppm_radius(float(info.ppm_radius), int(info.iteration_number), self.PPM_ALPHA)
