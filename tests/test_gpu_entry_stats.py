"""What every entry that traces rays reports in trt_stats — MI355X only.

The render, feature and ray-query entries share one host frame that lays out and clears the device counters, brackets the call
with events, reads the counters back and fills trt_stats.  This file pins what that frame fills in, entry by entry, through the C ABI:

  - scenes: `back` at 33 x 25 (wave-uniform walk, 8-byte hit records) and `veach-mis` at 96 x 54 (per-lane walk: k_trace_fix launches counted);
  - every entry makes one successful call with TRT_FLAG_TIMING | TRT_FLAG_COUNT at 4 samples: in one pass, with a mem_budget of one sample
    of every path (4 passes), and — the trt_render* entries — with TRT_FLAG_OVERLAP on two slots.  The ray-query entries take no trt_params:
    one call each;
  - every integer field of Stats (INT_FIELDS) against EXPECTED, literals recorded on the MI355X from the library as it was BEFORE the
    entries shared a frame; render_ms > 0 exactly for the entries with trt_params and == 0 for the ray queries; kernel_ms[k] > 0 exactly
    where launches[k] > 0;
  - a null stats pointer is accepted by every entry;
  - the empty calls of the list entries (n == 0, sample_begin == sample_end) zero the stats and leave the sums alone; a ray query of no rays
    returns at once and leaves the stats alone.

Images, sums and hits are not looked at: the parity files own those.
"""
import ctypes as C

import numpy as np
import pytest

import tinyraytracing_amd as T
from conftest import get_scene
from tinyraytracing_amd import _abi

pytestmark = pytest.mark.gpu

F32 = np.float32
SPP = 4
SCENES = {"back": (33, 25, T.SEED_BACK), "veach-mis": (96, 54, 0x5EED0002)}
FLAGS = T.TRT_FLAG_TIMING | T.TRT_FLAG_COUNT
INT_FIELDS = ("rays_camera", "rays_shadow", "rays_indirect", "shaded_hits", "inner_visits", "tri_tests", "launches", "passes", "rows_rendered",
              "inner_node_bytes", "redo_rays")
RENDER = ("trt_render", "trt_render_device", "trt_render_samples", "trt_render_pixels", "trt_render_pixels_device", "trt_render_rays",
          "trt_render_rays_device")
FEATURES = ("trt_render_aov", "trt_render_aov_device", "trt_aov_rays", "trt_aov_rays_device")
QUERIES = ("trt_trace_closest", "trt_trace_closest_range", "trt_trace_closest_device", "trt_trace_occluded", "trt_trace_occluded_device",
           "trt_trace_points", "trt_trace_points_device")
LISTS = ("trt_render_pixels", "trt_render_pixels_device", "trt_render_rays", "trt_render_rays_device", "trt_aov_rays", "trt_aov_rays_device")


def modes_of(entry):
    return ("one", "passes", "overlap") if entry in RENDER else (("one", "passes") if entry in FEATURES else ("one",))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Inputs:
    """A handle of one scene and the arguments of every entry: the whole image as tile, as pixel list and as the camera's own rays."""

    def __init__(self, name):
        import torch
        self.w, self.h, self.seed = SCENES[name]
        self.scene = get_scene(name, self.w, self.h)
        self.n_lights = self.scene.info["n_lights"]
        self.r = T.Renderer(self.scene, 0)
        self.lib = _abi.load_hip()
        self.n = n = self.w * self.h
        self.pixels = np.arange(n, dtype=np.uint32)
        self.org, self.dir = T.camera_rays(self.scene.flat.contents.camera, self.params("one", "trt_render"), self.pixels, 0, SPP)
        t, _, _ = self.r.trace_closest(self.org[0], self.dir[0])
        self.t_max = np.where(np.arange(n) % 2 == 0, F32(0.5) * t, F32(2.0) * t).astype(F32)  # a bound in front of the hit, one behind it
        self.tri_v = self.scene.arrays()["tri_v"]
        dev = torch.device("cuda", 0)
        self.d = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in
                  (("pixels", self.pixels.view(np.int32)), ("org", self.org), ("dir", self.dir), ("t_max", self.t_max), ("tri_v", self.tri_v))}
        self.torch, self.dev = torch, dev

    def params(self, mode, entry):
        """one: the library's own budget.  passes: room for one sample of every path, so each of the SPP samples is a pass.  overlap: two slots."""
        nl = self.n_lights
        per_path = {True: (3 * 2 + 1 + 1 + 3 * nl) * 16 + 4, False: 16 + 4}[entry in RENDER]  # trt_api.hip SlotLayout / AovLayout
        if entry.startswith("trt_aov_rays"):
            per_path = T.AOV_RAYS_BYTES_PER_PATH
        return T.make_params(self.w, self.h, SPP, self.seed, flags=FLAGS | (T.TRT_FLAG_OVERLAP if mode == "overlap" else 0),
                             mem_budget=self.n * per_path if mode == "passes" else 0)

    def call(self, entry, mode="one", st=None, n=None, samples=(0, SPP), sums=None):
        """One call of `entry` -> its return code.  st: a Stats to fill or None.  n / samples: the list length and sample range of the list
        entries (for the empty calls).  sums: the host accumulators [albedo-or-sum, normal-or-sumsq, depth] to use instead of fresh zeros."""
        lib, h, torch = self.lib, self.r._h, self.torch
        p = C.byref(self.params(mode, entry))
        sp = None if st is None else C.byref(st)
        n = self.n if n is None else n
        s0, s1 = samples
        z64 = lambda *shape: np.zeros(shape, np.float64)  # noqa: E731
        t64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=self.dev)  # noqa: E731
        t32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.dev)  # noqa: E731
        d = self.d
        u32 = C.POINTER(C.c_uint32)
        if entry == "trt_render":
            return lib.trt_render(h, p, _fp(np.empty((self.h, self.w, 3), F32)), sp)
        if entry == "trt_render_device":
            return lib.trt_render_device(h, p, _vp(t32(self.h, self.w, 3)), None, sp)
        if entry == "trt_render_samples":
            return lib.trt_render_samples(h, p, 0, SPP, _dp(z64(self.h, self.w, 3)), _fp(np.empty((self.h, self.w, 3), F32)), sp)
        if entry == "trt_render_pixels":
            a = sums or [z64(n, 3), z64(n, 3)]
            return lib.trt_render_pixels(h, p, n, self.pixels.ctypes.data_as(u32), s0, s1, _dp(a[0]), _dp(a[1]), sp)
        if entry == "trt_render_pixels_device":
            a = sums or [t64(n, 3), t64(n, 3)]
            return lib.trt_render_pixels_device(h, p, n, _vp(d["pixels"]), s0, s1, _vp(a[0]), _vp(a[1]), None, sp)
        if entry == "trt_render_rays":
            a = sums or [z64(n, 3), z64(n, 3)]
            return lib.trt_render_rays(h, p, n, _fp(self.org), _fp(self.dir), self.pixels.ctypes.data_as(u32), s0, s1, _dp(a[0]), _dp(a[1]), sp)
        if entry == "trt_render_rays_device":
            a = sums or [t64(n, 3), t64(n, 3)]
            return lib.trt_render_rays_device(h, p, n, _vp(d["org"]), _vp(d["dir"]), _vp(d["pixels"]), s0, s1, _vp(a[0]), _vp(a[1]), None, sp)
        if entry == "trt_render_aov":
            return lib.trt_render_aov(h, p, _fp(np.empty((self.n, 3), F32)), _fp(np.empty((self.n, 3), F32)), _fp(np.empty(self.n, F32)), sp)
        if entry == "trt_render_aov_device":
            return lib.trt_render_aov_device(h, p, _vp(t32(self.n, 3)), _vp(t32(self.n, 3)), _vp(t32(self.n)), None, sp)
        if entry == "trt_aov_rays":
            a = sums or [z64(n, 3), z64(n, 3), z64(n)]
            return lib.trt_aov_rays(h, p, n, _fp(self.org), _fp(self.dir), s0, s1, _dp(a[0]), _dp(a[1]), _dp(a[2]), sp)
        if entry == "trt_aov_rays_device":
            a = sums or [t64(n, 3), t64(n, 3), t64(n)]
            return lib.trt_aov_rays_device(h, p, n, _vp(d["org"]), _vp(d["dir"]), s0, s1, _vp(a[0]), _vp(a[1]), _vp(a[2]), None, sp)
        # the ray queries: sample 0's rays
        org, dirs = self.org[0], self.dir[0]
        t, tri, uv = np.empty(self.n, F32), np.empty(self.n, np.int32), np.empty((self.n, 2), F32)
        i32 = C.POINTER(C.c_int32)
        if entry == "trt_trace_closest":
            return lib.trt_trace_closest(h, n, _fp(org), _fp(dirs), _fp(t), tri.ctypes.data_as(i32), _fp(uv), sp)
        if entry == "trt_trace_closest_range":
            return lib.trt_trace_closest_range(h, n, _fp(org), _fp(dirs), _fp(self.t_max), _fp(t), tri.ctypes.data_as(i32), _fp(uv), sp)
        if entry == "trt_trace_closest_device":
            d_tri = torch.empty(self.n, dtype=torch.int32, device=self.dev)
            return lib.trt_trace_closest_device(h, n, _vp(d["org"][0]), _vp(d["dir"][0]), _vp(d["t_max"]), _vp(t32(self.n)), _vp(d_tri), _vp(t32(self.n, 2)), None, sp)
        if entry == "trt_trace_occluded":
            return lib.trt_trace_occluded(h, n, _fp(org), _fp(dirs), _fp(self.t_max), np.empty(self.n, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)), sp)
        if entry == "trt_trace_occluded_device":
            occ = torch.empty(self.n, dtype=torch.uint8, device=self.dev)
            return lib.trt_trace_occluded_device(h, n, _vp(d["org"][0]), _vp(d["dir"][0]), _vp(d["t_max"]), _vp(occ), None, sp)
        if entry == "trt_trace_points":
            return lib.trt_trace_points(h, n, _fp(org), _fp(dirs), _fp(self.tri_v), self.tri_v.shape[0], _fp(np.empty((self.n, 3), F32)), sp)
        if entry == "trt_trace_points_device":
            return lib.trt_trace_points_device(h, n, _vp(d["org"][0]), _vp(d["dir"][0]), _vp(d["tri_v"]), self.tri_v.shape[0], _vp(t32(self.n, 3)), None, sp)
        raise KeyError(entry)


_inputs = {}


def inputs(name):
    if name not in _inputs:
        _inputs[name] = Inputs(name)
    return _inputs[name]


def integers(st):
    """The integer fields of a Stats in the order of INT_FIELDS, arrays as tuples."""
    return tuple(tuple(int(x) for x in v) if hasattr(v, "__len__") else int(v) for v in (getattr(st, f) for f in INT_FIELDS))


def measure(name, entry, mode):
    st = T.Stats()
    x = inputs(name)
    rc = x.call(entry, mode, st)
    assert rc == 0, f"{entry} ({mode}) failed ({rc}): {x.lib.trt_last_error().decode()}"
    return st


# (scene, entry, mode) -> INT_FIELDS: rays_camera, rays_shadow, rays_indirect, shaded_hits, inner_visits[2], tri_tests[2], launches[8], passes,
# rows_rendered, inner_node_bytes, redo_rays
EXPECTED = {
    ('back', 'trt_render', 'one'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 1, 1, 1, 1, 1, 0, 0), 1, 25, 64, 0),
    ('back', 'trt_render', 'passes'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 4, 4, 4, 4, 4, 0, 0), 4, 25, 64, 0),
    ('back', 'trt_render', 'overlap'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 2, 2, 2, 2, 2, 0, 0), 2, 25, 64, 0),
    ('back', 'trt_render_device', 'one'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 1, 1, 1, 1, 1, 0, 0), 1, 25, 64, 0),
    ('back', 'trt_render_device', 'passes'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 4, 4, 4, 4, 4, 0, 0), 4, 25, 64, 0),
    ('back', 'trt_render_device', 'overlap'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 2, 2, 2, 2, 2, 0, 0), 2, 25, 64, 0),
    ('back', 'trt_render_samples', 'one'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 1, 1, 1, 1, 1, 0, 0), 1, 25, 64, 0),
    ('back', 'trt_render_samples', 'passes'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 4, 4, 4, 4, 4, 0, 0), 4, 25, 64, 0),
    ('back', 'trt_render_samples', 'overlap'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 2, 2, 2, 2, 2, 0, 0), 2, 25, 64, 0),
    ('back', 'trt_render_pixels', 'one'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 1, 1, 1, 1, 1, 0, 0), 1, 0, 64, 0),
    ('back', 'trt_render_pixels', 'passes'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 4, 4, 4, 4, 4, 0, 0), 4, 0, 64, 0),
    ('back', 'trt_render_pixels', 'overlap'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 2, 2, 2, 2, 2, 0, 0), 2, 0, 64, 0),
    ('back', 'trt_render_pixels_device', 'one'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 1, 1, 1, 1, 1, 0, 0), 1, 0, 64, 0),
    ('back', 'trt_render_pixels_device', 'passes'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 4, 4, 4, 4, 4, 0, 0), 4, 0, 64, 0),
    ('back', 'trt_render_pixels_device', 'overlap'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (0, 2, 2, 2, 2, 2, 0, 0), 2, 0, 64, 0),
    ('back', 'trt_render_rays', 'one'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (1, 1, 1, 1, 1, 1, 0, 0), 1, 0, 64, 0),
    ('back', 'trt_render_rays', 'passes'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (4, 4, 4, 4, 4, 4, 0, 0), 4, 0, 64, 0),
    ('back', 'trt_render_rays', 'overlap'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (2, 2, 2, 2, 2, 2, 0, 0), 2, 0, 64, 0),
    ('back', 'trt_render_rays_device', 'one'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (1, 1, 1, 1, 1, 1, 0, 0), 1, 0, 64, 0),
    ('back', 'trt_render_rays_device', 'passes'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (4, 4, 4, 4, 4, 4, 0, 0), 4, 0, 64, 0),
    ('back', 'trt_render_rays_device', 'overlap'): (3300, 5344, 4943, 6097, (20769, 13850), (85649, 81644), (2, 2, 2, 2, 2, 2, 0, 0), 2, 0, 64, 0),
    ('back', 'trt_render_aov', 'one'): (3300, 0, 0, 0, (6576, 0), (22973, 0), (0, 1, 0, 0, 1, 0, 0, 0), 1, 25, 64, 0),
    ('back', 'trt_render_aov', 'passes'): (3300, 0, 0, 0, (6576, 0), (22973, 0), (0, 4, 0, 0, 4, 0, 0, 0), 4, 25, 64, 0),
    ('back', 'trt_render_aov_device', 'one'): (3300, 0, 0, 0, (6576, 0), (22973, 0), (0, 1, 0, 0, 1, 0, 0, 0), 1, 25, 64, 0),
    ('back', 'trt_render_aov_device', 'passes'): (3300, 0, 0, 0, (6576, 0), (22973, 0), (0, 4, 0, 0, 4, 0, 0, 0), 4, 25, 64, 0),
    ('back', 'trt_aov_rays', 'one'): (3300, 0, 0, 0, (6576, 0), (22973, 0), (1, 1, 0, 0, 1, 0, 0, 0), 1, 0, 64, 0),
    ('back', 'trt_aov_rays', 'passes'): (3300, 0, 0, 0, (6576, 0), (22973, 0), (4, 4, 0, 0, 4, 0, 0, 0), 4, 0, 64, 0),
    ('back', 'trt_aov_rays_device', 'one'): (3300, 0, 0, 0, (6576, 0), (22973, 0), (1, 1, 0, 0, 1, 0, 0, 0), 1, 0, 64, 0),
    ('back', 'trt_aov_rays_device', 'passes'): (3300, 0, 0, 0, (6576, 0), (22973, 0), (4, 4, 0, 0, 4, 0, 0, 0), 4, 0, 64, 0),
    ('back', 'trt_trace_closest', 'one'): (0, 0, 0, 0, (1646, 0), (5714, 0), (0, 1, 0, 0, 0, 0, 0, 0), 0, 0, 64, 0),
    ('back', 'trt_trace_closest_range', 'one'): (0, 0, 0, 0, (1646, 0), (5714, 0), (0, 1, 0, 0, 0, 0, 0, 0), 0, 0, 64, 0),
    ('back', 'trt_trace_closest_device', 'one'): (0, 0, 0, 0, (1646, 0), (5714, 0), (0, 1, 0, 0, 0, 0, 0, 0), 0, 0, 64, 0),
    ('back', 'trt_trace_occluded', 'one'): (0, 825, 0, 0, (0, 1646), (0, 5714), (0, 0, 0, 1, 0, 0, 0, 0), 0, 0, 64, 0),
    ('back', 'trt_trace_occluded_device', 'one'): (0, 825, 0, 0, (0, 1646), (0, 5714), (0, 0, 0, 1, 0, 0, 0, 0), 0, 0, 64, 0),
    ('back', 'trt_trace_points', 'one'): (0, 0, 0, 0, (1646, 0), (5714, 0), (0, 1, 0, 0, 0, 0, 0, 0), 0, 0, 64, 0),
    ('back', 'trt_trace_points_device', 'one'): (0, 0, 0, 0, (1646, 0), (5714, 0), (0, 1, 0, 0, 0, 0, 0, 0), 0, 0, 64, 0),
    ('veach-mis', 'trt_render', 'one'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 1, 1, 3, 1, 1, 0, 0), 1, 54, 80, 0),
    ('veach-mis', 'trt_render', 'passes'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 4, 4, 12, 4, 4, 0, 0), 4, 54, 80, 0),
    ('veach-mis', 'trt_render', 'overlap'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 2, 2, 6, 2, 2, 0, 0), 2, 54, 80, 0),
    ('veach-mis', 'trt_render_device', 'one'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 1, 1, 3, 1, 1, 0, 0), 1, 54, 80, 0),
    ('veach-mis', 'trt_render_device', 'passes'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 4, 4, 12, 4, 4, 0, 0), 4, 54, 80, 0),
    ('veach-mis', 'trt_render_device', 'overlap'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 2, 2, 6, 2, 2, 0, 0), 2, 54, 80, 0),
    ('veach-mis', 'trt_render_samples', 'one'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 1, 1, 3, 1, 1, 0, 0), 1, 54, 80, 0),
    ('veach-mis', 'trt_render_samples', 'passes'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 4, 4, 12, 4, 4, 0, 0), 4, 54, 80, 0),
    ('veach-mis', 'trt_render_samples', 'overlap'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 2, 2, 6, 2, 2, 0, 0), 2, 54, 80, 0),
    ('veach-mis', 'trt_render_pixels', 'one'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 1, 1, 3, 1, 1, 0, 0), 1, 0, 80, 0),
    ('veach-mis', 'trt_render_pixels', 'passes'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 4, 4, 12, 4, 4, 0, 0), 4, 0, 80, 0),
    ('veach-mis', 'trt_render_pixels', 'overlap'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 2, 2, 6, 2, 2, 0, 0), 2, 0, 80, 0),
    ('veach-mis', 'trt_render_pixels_device', 'one'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 1, 1, 3, 1, 1, 0, 0), 1, 0, 80, 0),
    ('veach-mis', 'trt_render_pixels_device', 'passes'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 4, 4, 12, 4, 4, 0, 0), 4, 0, 80, 0),
    ('veach-mis', 'trt_render_pixels_device', 'overlap'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (0, 2, 2, 6, 2, 2, 0, 0), 2, 0, 80, 0),
    ('veach-mis', 'trt_render_rays', 'one'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (1, 1, 1, 3, 1, 1, 0, 0), 1, 0, 80, 0),
    ('veach-mis', 'trt_render_rays', 'passes'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (4, 4, 4, 12, 4, 4, 0, 0), 4, 0, 80, 0),
    ('veach-mis', 'trt_render_rays', 'overlap'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (2, 2, 2, 6, 2, 2, 0, 0), 2, 0, 80, 0),
    ('veach-mis', 'trt_render_rays_device', 'one'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (1, 1, 1, 3, 1, 1, 0, 0), 1, 0, 80, 0),
    ('veach-mis', 'trt_render_rays_device', 'passes'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (4, 4, 4, 12, 4, 4, 0, 0), 4, 0, 80, 0),
    ('veach-mis', 'trt_render_rays_device', 'overlap'): (20736, 85086, 25192, 31490, (99928, 634493), (163459, 685571), (2, 2, 2, 6, 2, 2, 0, 0), 2, 0, 80, 0),
    ('veach-mis', 'trt_render_aov', 'one'): (20736, 0, 0, 0, (33343, 0), (73181, 0), (0, 1, 0, 0, 1, 0, 0, 0), 1, 54, 80, 0),
    ('veach-mis', 'trt_render_aov', 'passes'): (20736, 0, 0, 0, (33343, 0), (73181, 0), (0, 4, 0, 0, 4, 0, 0, 0), 4, 54, 80, 0),
    ('veach-mis', 'trt_render_aov_device', 'one'): (20736, 0, 0, 0, (33343, 0), (73181, 0), (0, 1, 0, 0, 1, 0, 0, 0), 1, 54, 80, 0),
    ('veach-mis', 'trt_render_aov_device', 'passes'): (20736, 0, 0, 0, (33343, 0), (73181, 0), (0, 4, 0, 0, 4, 0, 0, 0), 4, 54, 80, 0),
    ('veach-mis', 'trt_aov_rays', 'one'): (20736, 0, 0, 0, (33343, 0), (73181, 0), (1, 1, 0, 0, 1, 0, 0, 0), 1, 0, 80, 0),
    ('veach-mis', 'trt_aov_rays', 'passes'): (20736, 0, 0, 0, (33343, 0), (73181, 0), (4, 4, 0, 0, 4, 0, 0, 0), 4, 0, 80, 0),
    ('veach-mis', 'trt_aov_rays_device', 'one'): (20736, 0, 0, 0, (33343, 0), (73181, 0), (1, 1, 0, 0, 1, 0, 0, 0), 1, 0, 80, 0),
    ('veach-mis', 'trt_aov_rays_device', 'passes'): (20736, 0, 0, 0, (33343, 0), (73181, 0), (4, 4, 0, 0, 4, 0, 0, 0), 4, 0, 80, 0),
    ('veach-mis', 'trt_trace_closest', 'one'): (0, 0, 0, 0, (8338, 0), (18309, 0), (0, 1, 0, 0, 0, 0, 0, 0), 0, 0, 80, 0),
    ('veach-mis', 'trt_trace_closest_range', 'one'): (0, 0, 0, 0, (6773, 0), (9152, 0), (0, 1, 0, 0, 0, 0, 0, 0), 0, 0, 80, 0),
    ('veach-mis', 'trt_trace_closest_device', 'one'): (0, 0, 0, 0, (6773, 0), (9152, 0), (0, 1, 0, 0, 0, 0, 0, 0), 0, 0, 80, 0),
    ('veach-mis', 'trt_trace_occluded', 'one'): (0, 5184, 0, 0, (0, 5184), (0, 5240), (0, 0, 0, 1, 0, 0, 0, 0), 0, 0, 80, 0),
    ('veach-mis', 'trt_trace_occluded_device', 'one'): (0, 5184, 0, 0, (0, 5184), (0, 5240), (0, 0, 0, 1, 0, 0, 0, 0), 0, 0, 80, 0),
    ('veach-mis', 'trt_trace_points', 'one'): (0, 0, 0, 0, (8338, 0), (18309, 0), (0, 1, 0, 0, 0, 0, 0, 0), 0, 0, 80, 0),
    ('veach-mis', 'trt_trace_points_device', 'one'): (0, 0, 0, 0, (8338, 0), (18309, 0), (0, 1, 0, 0, 0, 0, 0, 0), 0, 0, 80, 0),
}


CASES = [(name, entry) for name in SCENES for entry in RENDER + FEATURES + QUERIES]


@pytest.mark.parametrize("name,entry", CASES)
def test_stats_of_a_successful_call(name, entry):
    for mode in modes_of(entry):
        st = measure(name, entry, mode)
        got = integers(st)
        print(f"{name} {entry} {mode}: {got} render_ms {st.render_ms} kernel_ms {list(st.kernel_ms)}")
        assert got == EXPECTED[(name, entry, mode)], (name, entry, mode)
        if mode == "passes":
            assert st.passes >= 3
        assert (st.render_ms > 0.0) if entry not in QUERIES else (st.render_ms == 0.0), (name, entry, mode, st.render_ms)
        for k in range(_abi.TRT_MAX_KERNELS):
            assert (st.kernel_ms[k] > 0.0) == (st.launches[k] > 0), (name, entry, mode, k, st.kernel_ms[k], st.launches[k])


@pytest.mark.parametrize("name,entry", CASES)
def test_null_stats_pointer(name, entry):
    x = inputs(name)
    for mode in modes_of(entry):
        assert x.call(entry, mode, None) == 0, (entry, mode, x.lib.trt_last_error().decode())


def _marked_stats():
    st = T.Stats()
    C.memset(C.byref(st), 0xA5, C.sizeof(st))
    return st


@pytest.mark.parametrize("entry", LISTS)
@pytest.mark.parametrize("name", SCENES)
def test_empty_list_calls_zero_the_stats_and_keep_the_sums(name, entry):
    x = inputs(name)
    host = not entry.endswith("_device")
    zero = bytes(C.sizeof(T.Stats))
    for n, samples in ((0, (0, SPP)), (x.n, (2, 2)), (0, (3, 3))):
        m = max(n, 1)
        if host:
            sums = [np.full((m, 3), 1.25), np.full((m, 3), -2.5), np.full(m, 7.0)]
            before = [a.copy() for a in sums]
        else:
            sums = [x.torch.full(shape, v, dtype=x.torch.float64, device=x.dev) for shape, v in (((m, 3), 1.25), ((m, 3), -2.5), ((m,), 7.0))]
            before = [a.clone() for a in sums]
        st = _marked_stats()
        assert x.call(entry, "one", st, n=n, samples=samples, sums=sums) == 0, x.lib.trt_last_error().decode()
        assert bytes(st) == zero, (entry, n, samples)
        assert x.call(entry, "one", None, n=n, samples=samples, sums=sums) == 0
        for a, b in zip(sums, before):
            assert bool((a == b).all()), (entry, n, samples)


@pytest.mark.parametrize("entry", QUERIES)
@pytest.mark.parametrize("name", SCENES)
def test_query_of_no_rays_leaves_the_stats_alone(name, entry):
    x = inputs(name)
    st = _marked_stats()
    assert x.call(entry, "one", st, n=0) == 0
    assert bytes(st) == bytes(_marked_stats())
    assert x.call(entry, "one", None, n=0) == 0
