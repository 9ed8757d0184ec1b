"""Python mirror of the render-group API (include/orx.h, orx_create_group): N renderers and the
collectives between them behind one handle, driven like one `OptixRenderer`.  The orchestration
and the communicators (LOCAL: every rank on one device; RCCL: librccl through dlopen) live in
liborx.so (csrc/orx_group.hip, csrc/orx_group_comm.hip); nothing here needs torch.  `multigpu.py` remains the
one-process-per-GPU path over torch.distributed.

There is no CPU fallback: without liborx.so or a HIP device every entry point raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .renderer import (OptixRenderer, OrxError, RenderRequestDetails, _get_convergence, _save_state, load_library,
                       state_info)
from .scenes import Scene


class _BorrowedRenderer(OptixRenderer):
    """A rank of a group (orx_group_renderer): stats and buffers; the group owns the handle."""

    def __init__(self, lib, handle, config):
        self._lib = lib
        self._cfg = config
        self._h = C.c_void_p(handle)
        self._initialized = True
        self._scene_abi = None

    def destroy(self):
        self._h = None
        self._initialized = False


class OptixRendererGroup:
    """initialize(devices)       -> orx_create_group (one rank per entry of `devices`)
    initScene(scene)             -> orx_group_init_scene
    renderNextIteration(...)     -> orx_group_render_next_iteration
    getOutputBuffer()            -> orx_group_get_output (the full W*H*3 running sum)"""

    def __init__(self, config: _abi.OrxConfig | None = None, group_config: _abi.OrxGroupConfig | None = None):
        self._lib = load_library()
        self._cfg = config if config is not None else _abi.default_config()
        self._gcfg = group_config if group_config is not None else _abi.default_group_config()
        self._h = None
        self._scene_abi = None
        self._size = (0, 0)

    def _check(self, status):
        if status != _abi.ORX_OK:
            raise OrxError(status, self._lib.orx_group_last_error(self._h).decode())

    def initialize(self, devices=(0,)):
        if self._h:
            raise OrxError(_abi.ORX_ERR_STATE, "ERROR: Multiple OptixRendererGroup::initialize!")
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        st = self._lib.orx_create_group(len(devices), devs, C.byref(self._cfg), C.byref(self._gcfg), C.byref(h))
        if st != _abi.ORX_OK:
            raise OrxError(st, self._lib.orx_group_last_error(None).decode() or "orx_create_group failed")
        self._h = h
        return self

    def initScene(self, scene: Scene):
        if not self._h:
            raise OrxError(_abi.ORX_ERR_STATE, "Cannot initialize scene before OptixRendererGroup.")
        self._scene_abi = scene.to_abi()
        self._scene = scene
        self._check(self._lib.orx_group_init_scene(self._h, C.byref(self._scene_abi)))

    def renderNextIteration(self, iterationNumber: int, localIterationNumber: int, PPMRadius: float,
                            createOutput: bool, details):
        if not self._h:
            raise OrxError(_abi.ORX_ERR_STATE, "Traced before OptixRendererGroup was initialized.")
        req = details.to_abi() if isinstance(details, RenderRequestDetails) else details
        self._check(self._lib.orx_group_render_next_iteration(self._h, int(iterationNumber), int(localIterationNumber),
                                                              float(PPMRadius), int(bool(createOutput)), C.byref(req)))
        self._size = (int(req.width), int(req.height))

    def getOutputBuffer(self) -> np.ndarray:
        """[H][W][3] float32 SUM over the iterations (ROWS: of the frame; BATCH: of every rank)."""
        W, H = self._size
        out = np.empty(W * H * 3, np.float32)
        self._check(self._lib.orx_group_get_output(self._h, out.ctypes.data, out.nbytes))
        return out.reshape(H, W, 3)

    def _frame_size(self):
        return self._size

    def setConvergence(self, enable: bool):
        """orx_group_set_convergence (ROWS; BATCH raises ORX_ERR_UNSUPPORTED)."""
        self._check(self._lib.orx_group_set_convergence(self._h, int(bool(enable))))

    def getConvergence(self, floor: float = 1e-3, threshold: float = 0.05, tiles: bool = False):
        """orx_group_get_convergence: as OptixRenderer.getConvergence, over the whole frame."""
        return _get_convergence(self, "orx_group", floor, threshold, tiles)

    def getDisplayBuffer(self, inv_iterations: float, inv_gamma: float = 1.0 / 2.2,
                         fmt: int = _abi.DISPLAY_RGBA8) -> np.ndarray:
        """orx_group_get_display: the merged frame's 8-bit image [H][W][4], converted on rank 0."""
        W, H = self._size
        out = np.empty(W * H * 4, np.uint8)
        self._check(self._lib.orx_group_get_display(self._h, float(inv_iterations), float(inv_gamma), int(fmt),
                                                    out.ctypes.data, out.nbytes))
        return out.reshape(H, W, 4)

    def saveState(self) -> bytes:
        """orx_group_save_state: ROWS, one frame blob (that of a single renderer); BATCH, a container of
        the ranks' frames."""
        return _save_state(self, "orx_group")

    def restoreState(self, blob):
        """orx_group_restore_state, after initScene."""
        buf = bytes(blob)
        self._check(self._lib.orx_group_restore_state(self._h, buf, len(buf)))
        info = state_info(buf)
        self._size = (int(info.width), int(info.height))

    def world(self) -> int:
        return self._lib.orx_group_world(self._h)

    def renderer(self, rank: int) -> OptixRenderer:
        h = self._lib.orx_group_renderer(self._h, rank)
        if not h:
            raise OrxError(_abi.ORX_ERR_INVALID_ARGUMENT, f"no rank {rank}")
        return _BorrowedRenderer(self._lib, h, self._cfg)

    def pipelined(self) -> bool:
        return bool(self._lib.orx_group_pipelined(self._h))

    def comm_name(self) -> str:
        return self._lib.orx_group_comm_name(self._h).decode()

    def debug_reduce_scatter(self, x: np.ndarray) -> np.ndarray:
        """x [world][world * block] float32 -> [world][block]: out[k][j] = sum over ranks of x[r][k * block + j]"""
        n = self.world()
        x = np.ascontiguousarray(x, np.float32)
        assert x.ndim == 2 and x.shape[0] == n and x.shape[1] % n == 0
        block = x.shape[1] // n
        out = np.empty((n, block), np.float32)
        self._check(self._lib.orx_group_debug_reduce_scatter(self._h, x.ctypes.data, block, out.ctypes.data))
        return out

    def debug_reduce(self, x: np.ndarray) -> np.ndarray:
        """x [world][n] float32 -> [n]: the sum over ranks"""
        x = np.ascontiguousarray(x, np.float32)
        assert x.ndim == 2 and x.shape[0] == self.world()
        out = np.empty(x.shape[1], np.float32)
        self._check(self._lib.orx_group_debug_reduce(self._h, x.ctypes.data, x.shape[1], out.ctypes.data))
        return out

    def slab_plan(self):
        """(axis, bin_dest uint8[1024], counts int64[world][world]) of the last ORX_PHOTONS_SLABS iteration
        (orx_group_slab_plan); ORX_ERR_STATE when there was none (rows photons, one rank)"""
        n = self.world()
        axis = C.c_uint32()
        bin_dest = np.empty(1024, np.uint8)
        counts = np.empty((n, n), np.uint64)
        st = self._lib.orx_group_slab_plan(self._h, C.byref(axis), bin_dest.ctypes.data, counts.ctypes.data)
        if st != _abi.ORX_OK:
            raise OrxError(st, "no slab plan: the last iteration did not exchange photon slabs")
        return int(axis.value), bin_dest, counts.astype(np.int64)

    def debug_all_to_all(self, x: np.ndarray, counts) -> np.ndarray:
        """x: the ranks' send buffers back to back, float32 [sum(counts)][9] (rank s's records for d = 0..n-1 in
        turn); counts [world][world] records s sends to d -> the ranks' receive buffers back to back"""
        n = self.world()
        counts = np.ascontiguousarray(counts, np.uint64)
        x = np.ascontiguousarray(x, np.float32)
        assert counts.shape == (n, n) and x.size == 9 * int(counts.sum())
        out = np.empty(x.size, np.float32)
        self._check(self._lib.orx_group_debug_all_to_all(self._h, x.ctypes.data, counts.ctypes.data, out.ctypes.data))
        return out.reshape(-1, 9)

    def destroy(self):
        if self._h:
            self._lib.orx_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
