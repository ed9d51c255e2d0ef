"""tinyraytracing_amd — MI355X-native path-tracing hot path of TinyRayTracing.

Python is the thin host layer used by tests and bench.py; the compute path is
libtrt_hip.so (hand-written HIP for gfx950, include/trt.h) and the loaders are
libtrt_host.so (C++, include/trt_host.h).  The classes mirror the reference's
driver (main.cpp:44-119): load the scene (readxml -> readobj -> readmtl), build
the BVH, render(), imshow().
"""
import ctypes as C
import os

from typing import NamedTuple

import numpy as np

from . import _abi, adaptive
from ._abi import Params, Stats, SceneFlat, Camera, TRT_FLAG_COUNT, TRT_FLAG_TIMING, TRT_FLAG_OVERLAP, TRT_FLAG_FIXED_NEE, TRT_FLAG_FIXED_PIXELS, TRT_FLAG_RAY_OFFSET, TRT_FLAG_SPECULAR_KS, TRT_FLAG_ONE_LIGHT, TRT_FLAG_NEAR_LIGHTS, KERNEL_NAMES, TRT_K_DENOISE, TRT_K_REFIT, AOV_RAYS_BYTES_PER_PATH  # noqa: F401

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES_DIR = os.path.join(REPO_ROOT, "scenes")

# seeds fixed by SURVEY.md §8d / BASELINE.md §2
SEED_BACK = 0x5EED0001
SEED_SOUP = 0x5EED0003
SEED_STAIRCASE = 0x5EED0004
SEED_BLOB = 0x5EED0005
SEED_LAMPS = 0x5EED0006  # Scene.named("lamps"): placement, size and radiance of the added lamps

_BUILDERS = {"sweep": 0, "binned": 1, "auto": 2}
# Triangles per BVH leaf.  The reference calls buildBVH(..., 8) (main.cpp:76); on the GPU 2 measured fastest on every
# scene larger than the Cornell box, and the topology is free: only nearest-hit + tie rules matter.
DEFAULT_LEAF = 2
TINY_LEAF = 8
SOUP_LEAF = 1   # unstructured triangle soup: one triangle per leaf (soup-1M 16 spp: 112 -> 106 ms/step)


def default_leaf(name, n_triangles):
    """Leaf size Scene.named() builds with when none is given (the topology is free: any valid tree gives the hits
    of the oracle on that same tree)."""
    if n_triangles <= 64:
        return TINY_LEAF
    return SOUP_LEAF if name == "soup" else DEFAULT_LEAF


class TrtError(RuntimeError):
    pass


class Scene:
    """Scene + BVH + flat arrays (reference: Scene in scene.h:19-36 and buildBVH, bvh.cpp:16)."""

    def __init__(self, handle):
        self._lib = _abi.load_host()
        self._h = handle
        self._built = False

    @classmethod
    def load(cls, xml_path, obj_path, mtl_path, basedir, width=0, height=0, triangulate_polygons=False):
        """scene.readxml(xml); scene.readobj(obj); scene.readmtl(mtl, basedir) (main.cpp:66-69).
        width/height override the XML resolution; triangulate_polygons fans faces of more than three vertices instead of
        keeping their first three only (the reference's behaviour, scene.cpp:162, and the default)."""
        lib = _abi.load_host()
        h = lib.trth_scene_load_opts(os.fsencode(xml_path), os.fsencode(obj_path), os.fsencode(mtl_path),
                                     os.fsencode(basedir), int(width), int(height), 1 if triangulate_polygons else 0)
        if not h:
            raise TrtError(lib.trth_last_error().decode())
        return cls(h)

    @classmethod
    def named(cls, name, width=0, height=0, leaf_num=None, builder="auto", n=None, seed=None, device=0):
        """Shipped and synthetic scenes: back, veach-mis, staircase, soup (n random triangles in
        the back box, BASELINE config 3), blob (displaced geodesic sphere, config 5), lamps (back with n = 16 more area lights
        under its ceiling: n + 1 lights, host/synth.cpp).  `device`: where builder="lbvh" runs
        (a rank of a multi-GPU job passes its own GPU; the host builders ignore it)."""
        if name in ("back", "veach-mis", "staircase"):
            d = os.path.join(SCENES_DIR, name)
            s = cls.load(os.path.join(d, name + ".xml"), os.path.join(d, name + ".obj"), os.path.join(d, name + ".mtl"), d, width, height)
        elif name == "lamps":
            d = os.path.join(SCENES_DIR, "back")
            s = cls.load(os.path.join(d, "back.xml"), os.path.join(d, "back.obj"), os.path.join(d, "back.mtl"), d, width, height)
            s._check(s._lib.trth_scene_add_lamps(s._h, SEED_LAMPS if seed is None else seed, 16 if n is None else int(n)))
        elif name in ("soup", "blob"):
            d = os.path.join(SCENES_DIR, "back")
            s = cls.load(os.path.join(d, "back.xml"), os.path.join(d, "back.obj"), os.path.join(d, "back.mtl"), d, width, height)
            s._check(s._lib.trth_scene_drop_tris(s._h, 6, 12))  # the cube of back.obj (faces 7..18)
            if name == "soup":
                s._check(s._lib.trth_scene_add_soup(s._h, SEED_SOUP if seed is None else seed, 1_000_000 if n is None else int(n)))
            else:
                s._check(s._lib.trth_scene_add_blob(s._h, SEED_BLOB if seed is None else seed, 10_000_000 if n is None else int(n)))
        else:
            raise TrtError(f"unknown scene {name!r}")
        if leaf_num is None:
            # tiny scenes are walked wave-uniformly (every node, every triangle: trt_kernels.h WalkUniform), where fewer,
            # fuller leaves are cheaper; everything else is traversed per ray, where 2 measured best
            leaf_num = default_leaf(name, s.info["n_triangles"])
        s.build_bvh(leaf_num, builder, device)
        return s

    def _check(self, rc):
        if rc != 0:
            raise TrtError(self._lib.trth_last_error().decode())

    def build_bvh(self, leaf_num=DEFAULT_LEAF, builder="auto", device=0):
        """BVHNode* root = buildBVH(scene.triangles, 0, n-1, leaf_num) (main.cpp:76 passes 8) + flattening.
        builder: "sweep" / "binned" / "auto" = the host builders (exact SAH up to 64 k triangles, 32-bin SAH above); "lbvh" = the GPU
        builder of include/trt_build.h on `device` (Morton order + radix tree; `self.build_ms` = (device ms, whole call ms))."""
        if builder == "lbvh":
            lib = _abi.load_build()
            n = self.info["n_triangles"]
            v = np.empty(max(n, 1) * 9, np.float32)
            self._check(self._lib.trth_scene_vertices(self._h, v.ctypes.data_as(C.POINTER(C.c_float)), v.size))
            cap = max(n, 2) - 1
            node_bytes = np.empty(cap * C.sizeof(_abi.BvhNode), np.uint8)  # (a ctypes array of 10 M nodes would be zeroed first)
            nodes = C.cast(node_bytes.ctypes.data, C.POINTER(_abi.BvhNode))
            order = np.empty(max(n, 1), np.uint32)
            n_nodes, depth = C.c_uint32(0), C.c_uint32(0)
            ms = (C.c_double * 2)()
            rc = lib.trt_build_lbvh(v.ctypes.data_as(C.POINTER(C.c_float)), n, int(leaf_num), int(device), nodes, cap, C.byref(n_nodes),
                                    order.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(depth), ms)
            if rc != 0:
                raise TrtError(f"trt_build_lbvh failed ({rc}): {lib.trt_build_last_error().decode()}")
            self.build_ms = (ms[0], ms[1])
            self._check(self._lib.trth_scene_adopt_bvh(self._h, nodes, n_nodes.value, order.ctypes.data_as(C.POINTER(C.c_uint32)), depth.value))
        else:
            self._check(self._lib.trth_scene_build(self._h, int(leaf_num), _BUILDERS[builder]))
        self._built = True
        return self

    @property
    def flat(self):
        p = self._lib.trth_scene_flat(self._h)
        if not p:
            raise TrtError(self._lib.trth_last_error().decode())
        return p

    @property
    def info(self):
        arr = (C.c_int64 * 8)()
        self._check(self._lib.trth_scene_info(self._h, arr))
        keys = ["width", "height", "n_vertices", "n_vn", "n_vt", "n_triangles", "n_materials", "n_lights"]
        return dict(zip(keys, [int(x) for x in arr]))

    def light_area(self, i):
        return float(self._lib.trth_scene_light_area(self._h, i))

    def material_name(self, i):
        s = self._lib.trth_scene_material_name(self._h, i)
        if s is None:
            raise TrtError(self._lib.trth_last_error().decode())
        return s.decode()

    # numpy views of the flat arrays (copies), mostly for tests
    def arrays(self):
        f = self.flat.contents
        n = f.n_tris
        out = {
            "tri_v": np.ctypeslib.as_array(f.tri_v, shape=(n, 3, 3)).copy() if n else np.zeros((0, 3, 3), np.float32),
            "tri_vn": np.ctypeslib.as_array(f.tri_vn, shape=(n, 3, 3)).copy() if n else np.zeros((0, 3, 3), np.float32),
            "tri_vt": np.ctypeslib.as_array(f.tri_vt, shape=(n, 3, 2)).copy() if n else np.zeros((0, 3, 2), np.float32),
            "tri_mat": np.ctypeslib.as_array(f.tri_mat, shape=(n,)).copy() if n else np.zeros((0,), np.int32),
            "n_nodes": int(f.n_nodes),
            "bvh_depth": int(f.bvh_depth),
        }
        return out

    def set_vertices(self, tri_v, tri_vn=None):
        """Moves the triangles of a built scene (trth_scene_set_vertices): tri_v, and tri_vn unless None, are float32 [n_triangles, 3, 3] in
        the order of the flat description (arrays()["tri_v"]).  The tree keeps its topology and gets the boxes of the moved triangles, the
        light tables are rebuilt; `flat` then describes the moved scene — for Renderer.update_geometry, or for a fresh Renderer."""
        n = self.flat.contents.n_tris
        fp = C.POINTER(C.c_float)
        arrs = []
        for name, a in (("tri_v", tri_v), ("tri_vn", tri_vn)):
            if a is None:
                arrs.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.size != n * 9:
                raise TrtError(f"set_vertices: {name} must hold {n} x 3 x 3 floats")
            arrs.append(a)
        if arrs[0] is None:
            raise TrtError("set_vertices: tri_v is needed")
        self._check(self._lib.trth_scene_set_vertices(self._h, arrs[0].ctypes.data_as(fp), None if arrs[1] is None else arrs[1].ctypes.data_as(fp)))
        return self

    def close(self):
        if self._h:
            self._lib.trth_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_params(width, height, spp, seed, tile=None, rows=None, max_depth=0, flags=0, mem_budget=0):
    p = Params()
    p.width, p.height, p.spp, p.seed = int(width), int(height), int(spp), int(seed) & 0xFFFFFFFF
    x0, y0, x1, y1 = tile if tile is not None else (0, 0, width, height)
    p.x0, p.y0, p.x1, p.y1 = int(x0), int(y0), int(x1), int(y1)
    rb, rm, rr = rows if rows is not None else (1, 1, 0)
    p.row_block, p.row_mod, p.row_rem = int(rb), int(rm), int(rr)
    p.max_depth, p.flags, p.mem_budget = int(max_depth), int(flags), int(mem_budget)
    return p


def rows_selected(p):
    """Image rows a Params selects, in output order (mirrors trt_rows_selected)."""
    ys = range(p.y0, p.y1)
    if p.row_mod <= 1:
        return list(ys)
    return [y for y in ys if (y // p.row_block) % p.row_mod == p.row_rem]


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _add_stats(total, st):
    """Accumulates the Stats of one render call into `total` (counts and times summed, max_bounces the deepest)."""
    for f in ("rays_camera", "rays_shadow", "rays_indirect", "shaded_hits", "render_ms", "passes", "rows_rendered", "redo_rays"):
        setattr(total, f, getattr(total, f) + getattr(st, f))
    for f in ("inner_visits", "tri_tests", "wave_steps", "launches", "kernel_ms", "lane_census"):
        a, b = getattr(total, f), getattr(st, f)
        for i in range(len(a)):
            a[i] += b[i]
    total.max_bounces = max(total.max_bounces, st.max_bounces)
    total.inner_node_bytes = st.inner_node_bytes


def _call(lib, entry, *args, after=()):
    """Calls `entry` of the library `lib` with a fresh Stats behind `args` (and `after` behind that) -> the Stats it filled."""
    st = Stats()
    rc = getattr(lib, entry)(*args, C.byref(st), *after)
    if rc != 0:
        raise TrtError(f"{entry} failed ({rc}): {lib.trt_last_error().decode()}")
    return st


def _tile_pixels(params, what):
    """-> the rows ys and columns xs of the tile of `params` and its pixels y * width + x in tile order (int64)."""
    ys = np.asarray(rows_selected(params), np.int64)
    xs = np.arange(params.x0, params.x1, dtype=np.int64)
    if ys.size == 0 or xs.size == 0:
        raise TrtError(f"{what}: empty tile")
    return ys, xs, (ys[:, None] * params.width + xs[None, :]).reshape(-1)


class AdaptiveResult(NamedTuple):
    image: object    # sum * spp / n_q per pixel, float64 [rows, tile_w, 3] (numpy, or a torch tensor with on_device)
    counts: object   # n_q: pixel q holds samples [0, n_q) of its stream
    error: object    # the estimated relative standard error the policy stopped on (adaptive.relative_error)
    stats: Stats     # summed over the render calls
    rounds: int      # render calls made


class Renderer:
    """Owns a trt_handle: the scene resident in HBM of one MI355X."""

    def __init__(self, scene, device=0):
        self._lib = _abi.load_hip()  # raises if the HIP extension is missing
        self._scene = scene          # keep the flat arrays alive
        h = C.c_void_p()
        rc = self._lib.trt_create(scene.flat, int(device), C.byref(h))
        if rc != 0:
            raise TrtError(f"trt_create failed ({rc}): {self._lib.trt_last_error().decode()}")
        self._h = h
        self.device = int(device)

    def _tile_shape(self, params, what=None):
        """(rows, tile_w) of the tile of `params`; an empty tile is refused in the name of `what` (None: left to the library)."""
        nrows, tw = self._lib.trt_rows_selected(C.byref(params)), params.x1 - params.x0
        if what and (nrows <= 0 or tw <= 0):
            raise TrtError(f"{what}: empty tile")
        return nrows, tw

    def render(self, params):
        """render() -> (float32 image [rows, tile_w, 3] linear radiance, Stats).  Host output."""
        out = np.empty(self._tile_shape(params, "render") + (3,), dtype=np.float32)
        return out, _call(self._lib, "trt_render", self._h, C.byref(params), out.ctypes.data_as(C.POINTER(C.c_float)))

    def render_samples(self, params, sample_begin, sample_end, accum=None):
        """Progressive render (trt_render_samples): adds samples [sample_begin, sample_end) of params.spp onto
        `accum` (float64 [rows, tile_w, 3], the running per-pixel sums; None = start from zeros).
        Returns (image so far, accum, Stats); save accum + sample_end to checkpoint, pass them back to resume."""
        shape = self._tile_shape(params, "render_samples") + (3,)
        if accum is None:
            accum = np.zeros(shape, dtype=np.float64)
        if accum.dtype != np.float64 or accum.shape != shape or not accum.flags["C_CONTIGUOUS"]:
            raise TrtError("render_samples: accum must be a contiguous float64 array of shape (rows, tile_w, 3)")
        out = np.empty(shape, dtype=np.float32)
        st = _call(self._lib, "trt_render_samples", self._h, C.byref(params), int(sample_begin), int(sample_end), accum.ctypes.data_as(C.POINTER(C.c_double)),
                   out.ctypes.data_as(C.POINTER(C.c_float)))
        return out, accum, st

    def render_pixels(self, params, pixels, sample_begin, sample_end, sums=None, sumsq=None):
        """Samples [sample_begin, sample_end) of the listed pixels only (trt_render_pixels): pixels[i] = y * width + x, any order,
        duplicates allowed.  Adds v = (double)(L_s / params.spp) and v * v of every sample onto sums / sumsq (float64 [n, 3];
        None = zeros) and returns (sums, sumsq, Stats).  numpy uint32 pixels: host arrays.  A torch tensor on this device (int32 or
        uint32): sums / sumsq are float64 tensors there, and the work runs on torch's current stream (trt_render_pixels_device)."""
        if _is_torch(pixels):
            return self._render_pixels_device(params, pixels, sample_begin, sample_end, sums, sumsq)
        pixels = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
        n = pixels.size
        sums = self._moments(sums, n, "sums")
        sumsq = self._moments(sumsq, n, "sumsq")
        fp = C.POINTER(C.c_double)
        st = _call(self._lib, "trt_render_pixels", self._h, C.byref(params), n, pixels.ctypes.data_as(C.POINTER(C.c_uint32)), int(sample_begin), int(sample_end),
                   sums.ctypes.data_as(fp), sumsq.ctypes.data_as(fp))
        return sums, sumsq, st

    @staticmethod
    def _moments(a, n, what):
        if a is None:
            return np.zeros((n, 3), np.float64)
        if not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.shape != (n, 3) or not a.flags["C_CONTIGUOUS"]:
            raise TrtError(f"render_pixels: {what} must be a contiguous float64 array of shape ({n}, 3)")
        return a

    def _render_pixels_device(self, params, pixels, sample_begin, sample_end, sums, sumsq):
        import torch
        dev = torch.device("cuda", self.device)
        if pixels.device != dev or pixels.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or pixels.dim() != 1 or not pixels.is_contiguous():
            raise TrtError(f"render_pixels: pixels must be a contiguous 1-D int32 / uint32 tensor on {dev}")
        n = pixels.numel()
        out = []
        for a, what in ((sums, "sums"), (sumsq, "sumsq")):
            if a is None:
                a = torch.zeros((n, 3), dtype=torch.float64, device=dev)
            elif a.device != dev or a.dtype != torch.float64 or tuple(a.shape) != (n, 3) or not a.is_contiguous():
                raise TrtError(f"render_pixels: {what} must be a contiguous float64 tensor of shape ({n}, 3) on {dev}")
            out.append(a)
        stream = torch.cuda.current_stream(dev).cuda_stream
        st = _call(self._lib, "trt_render_pixels_device", self._h, C.byref(params), n, C.c_void_p(pixels.data_ptr()), int(sample_begin), int(sample_end),
                   C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()), C.c_void_p(stream))
        return out[0], out[1], st

    def render_adaptive(self, params, rel_error, min_spp, max_spp, batch, on_device=False):
        """Adaptive sampling of the tile of `params` (tinyraytracing_amd/adaptive.py has the policy): every pixel gets [0, min_spp),
        then rounds of `batch` more samples go to every pixel whose estimated relative standard error of its mean luminance is above
        rel_error, until max_spp.  Pixel q ends with the samples [0, n_q) of its own stream.
        -> AdaptiveResult(image = sum * spp / n_q, float64 [rows, tile_w, 3]; counts n_q [rows, tile_w]; error [rows, tile_w];
        stats summed over the calls; rounds).  on_device: the sums, the estimates and the selection live in torch tensors on this
        device (the image is returned there too) and nothing of the image crosses to the host between rounds."""
        ys, xs, pixels = _tile_pixels(params, "render_adaptive")
        k = pixels.size
        total = Stats()

        def render(pix, s0, s1, su, sq):
            su, sq, st = self.render_pixels(params, pix, s0, s1, su, sq)
            _add_stats(total, st)
            return su, sq

        if on_device:
            import torch
            if params.width * params.height > 0x7FFFFFFF:
                raise TrtError("render_adaptive: on_device needs width * height < 2^31 (int32 pixel tensors)")
            dev = torch.device("cuda", self.device)
            pix = torch.from_numpy(pixels.astype(np.int32)).to(dev)
            sums = torch.zeros((k, 3), dtype=torch.float64, device=dev)
            sumsq = torch.zeros_like(sums)
            counts = torch.zeros(k, dtype=torch.int64, device=dev)
            sums, sumsq, counts, err, rounds = adaptive.run(render, pix, sums, sumsq, counts, rel_error, min_spp, max_spp, batch)
            image = sums * float(params.spp) / counts.to(torch.float64)[:, None]
        else:
            pix = pixels.astype(np.uint32)
            sums, sumsq = np.zeros((k, 3)), np.zeros((k, 3))
            counts = np.zeros(k, np.int64)
            sums, sumsq, counts, err, rounds = adaptive.run(render, pix, sums, sumsq, counts, rel_error, min_spp, max_spp, batch)
            image = sums * float(params.spp) / counts[:, None]
        shape = (ys.size, xs.size)
        return AdaptiveResult(image.reshape(shape + (3,)), counts.reshape(shape), err.reshape(shape), total, rounds)

    def render_denoised(self, params, aov_spp=None, iterations=5, sigma_normal=128, sigma_depth=1.0, sigma_luminance=4.0):
        """A render of the tile of `params` and its denoised image (trt_denoise).  The beauty is rendered with trt_render_pixels over every
        pixel of the tile in tile order, samples [0, params.spp) (params.spp >= 2), so `color` is exactly render(params)'s image, and its
        moments give `variance`, the variance of each pixel's mean luminance (mean_luminance_variance).  The feature buffers are
        render_aov at aov_spp samples (None = min(spp, 16)), same seed and flags.  The tile is filtered as one image: rows may not be
        interleaved.  -> dict(color, variance, albedo, normal, depth, denoised) as float32 arrays [rows, tile_w(, 3)], and stats: the
        Stats of the three calls summed."""
        if params.spp < 2:
            raise TrtError("render_denoised: spp must be >= 2 (the variance needs two samples)")
        if params.row_mod > 1:
            raise TrtError("render_denoised: the tile must not interleave rows (it is filtered as one image)")
        ys, xs, pixels = _tile_pixels(params, "render_denoised")
        shape = (ys.size, xs.size)
        total = Stats()
        sums, sumsq, st = self.render_pixels(params, pixels.astype(np.uint32), 0, params.spp)
        _add_stats(total, st)
        pa = make_params(params.width, params.height, params.spp if aov_spp is None else aov_spp, params.seed, tile=(params.x0, params.y0, params.x1, params.y1),
                         max_depth=params.max_depth, flags=params.flags, mem_budget=params.mem_budget)
        if aov_spp is None:
            pa.spp = min(params.spp, 16)
        aov, st = self.render_aov(pa, want_stats=True)
        _add_stats(total, st)
        out = {"color": sums.astype(np.float32).reshape(shape + (3,)),
               "variance": mean_luminance_variance(sums, sumsq, params.spp).reshape(shape)}
        out.update(aov)
        out["denoised"], st = denoise(out["color"], out["variance"], aov["albedo"], aov["normal"], aov["depth"], iterations=iterations,
                                      sigma_normal=sigma_normal, sigma_depth=sigma_depth, sigma_luminance=sigma_luminance, device=self.device,
                                      want_stats=True)
        _add_stats(total, st)
        out["stats"] = total
        return out

    def render_into(self, params, out_tensor, stream_ptr=0):
        """Renders into a CUDA/HIP torch tensor (float32, >= rows*tile_w*3 elements) on this device."""
        nrows, tw = self._tile_shape(params)
        need = nrows * tw * 3
        if out_tensor.numel() < need or str(out_tensor.dtype) != "torch.float32" or not out_tensor.is_cuda or not out_tensor.is_contiguous():
            raise TrtError("render_into: need a contiguous float32 device tensor with rows*tile_w*3 elements")
        return _call(self._lib, "trt_render_device", self._h, C.byref(params), C.c_void_p(out_tensor.data_ptr()), C.c_void_p(stream_ptr))

    def _aov_shapes(self, params, what):
        nrows, tw = self._tile_shape(params, what)
        return {"albedo": (nrows, tw, 3), "normal": (nrows, tw, 3), "depth": (nrows, tw)}

    def render_aov(self, params, want_stats=False):
        """First-hit feature buffers for denoisers (trt_render_aov): the mean over samples [0, params.spp) of the camera ray's first hit's
        albedo (texel or Kd), shading normal (not renormalised) and distance; a miss counts as 0, 0 and TRT_INF.
        -> dict(albedo=float32 [rows, tile_w, 3], normal=float32 [rows, tile_w, 3], depth=float32 [rows, tile_w])[, Stats]."""
        out = {k: np.empty(shape, np.float32) for k, shape in self._aov_shapes(params, "render_aov").items()}
        fp = C.POINTER(C.c_float)
        st = _call(self._lib, "trt_render_aov", self._h, C.byref(params), out["albedo"].ctypes.data_as(fp), out["normal"].ctypes.data_as(fp), out["depth"].ctypes.data_as(fp))
        return (out, st) if want_stats else out

    def render_aov_into(self, params, albedo=None, normal=None, depth=None, stream_ptr=0):
        """trt_render_aov_device: the feature buffers into contiguous float32 torch tensors on this device (albedo / normal >= rows*tile_w*3
        elements, depth >= rows*tile_w; None = not wanted, at least one given), the work on stream `stream_ptr` (0 = default).  -> Stats."""
        shapes = self._aov_shapes(params, "render_aov_into")
        given = {"albedo": albedo, "normal": normal, "depth": depth}
        if all(t is None for t in given.values()):
            raise TrtError("render_aov_into: at least one of albedo, normal, depth is needed")
        ptrs = self._device_arrays("render_aov_into", [(k, t, ("torch.float32",), int(np.prod(shapes[k]))) for k, t in given.items()], at_least=True)
        return _call(self._lib, "trt_render_aov_device", self._h, C.byref(params), *ptrs, C.c_void_p(stream_ptr))

    @staticmethod
    def _rays(org, direction, t_max, what):
        org = np.ascontiguousarray(org, dtype=np.float32).reshape(-1, 3)
        direction = np.ascontiguousarray(direction, dtype=np.float32).reshape(-1, 3)
        n = org.shape[0]
        if direction.shape[0] != n:
            raise TrtError(f"{what}: org/dir length mismatch")
        if t_max is not None:
            t_max = np.ascontiguousarray(t_max, dtype=np.float32).reshape(-1)
            if t_max.shape[0] != n:
                raise TrtError(f"{what}: t_max must hold one bound per ray")
        return org, direction, t_max, n

    def trace_closest(self, org, direction, want_stats=False, t_max=None):
        """traverseBVH on a ray batch: returns (t, tri, uv[, Stats]).  t_max (one bound per ray, None = TRT_INF): only hits with
        t < bound count (trt_trace_closest_range, include/trt.h); a ray with nothing inside its bound gets the miss record."""
        org, direction, t_max, n = self._rays(org, direction, t_max, "trace_closest")
        t = np.empty(n, np.float32)
        tri = np.empty(n, np.int32)
        uv = np.empty((n, 2), np.float32)
        fp = C.POINTER(C.c_float)
        out = (t.ctypes.data_as(fp), tri.ctypes.data_as(C.POINTER(C.c_int32)), uv.ctypes.data_as(fp))
        if t_max is None:
            st = _call(self._lib, "trt_trace_closest", self._h, n, org.ctypes.data_as(fp), direction.ctypes.data_as(fp), *out)
        else:
            st = _call(self._lib, "trt_trace_closest_range", self._h, n, org.ctypes.data_as(fp), direction.ctypes.data_as(fp), t_max.ctypes.data_as(fp), *out)
        return (t, tri, uv, st) if want_stats else (t, tri, uv)

    def trace_occluded(self, org, direction, t_max=None, want_stats=False):
        """Occlusion on a ray batch (trt_trace_occluded): a bool per ray, True iff some hit with t < bound counts (t_max: one bound per
        ray, None = TRT_INF).  The walk stops at the first such hit.  Returns occluded[, Stats]."""
        org, direction, t_max, n = self._rays(org, direction, t_max, "trace_occluded")
        occ = np.empty(n, np.uint8)
        fp = C.POINTER(C.c_float)
        st = _call(self._lib, "trt_trace_occluded", self._h, n, org.ctypes.data_as(fp), direction.ctypes.data_as(fp),
                   None if t_max is None else t_max.ctypes.data_as(fp), occ.ctypes.data_as(C.POINTER(C.c_uint8)))
        occ = occ.view(np.bool_)
        return (occ, st) if want_stats else occ

    def _device_arrays(self, what, arrays, at_least=False):
        """Checks torch tensors of this device for the *_into entries: arrays = [(name, tensor or None, dtypes, elements)]; a tensor holds
        exactly that many elements, or with at_least that many or more.  -> pointers."""
        ptrs = []
        for name, t, dtypes, need in arrays:
            if t is None:
                ptrs.append(None)
                continue
            if (not _is_torch(t) or str(t.dtype) not in dtypes or not t.is_cuda or not t.is_contiguous()
                    or (t.numel() < need if at_least else t.numel() != need)
                    or (t.device.index is not None and t.device.index != self.device)):
                raise TrtError(f"{what}: {name} must be a contiguous {' or '.join(d[6:] for d in dtypes)} tensor on cuda:{self.device} "
                               f"with {need} elements")
            ptrs.append(C.c_void_p(t.data_ptr()))
        return ptrs

    def _ray_count(self, org, what):
        if not _is_torch(org) or org.dim() != 2 or org.shape[1] != 3:
            raise TrtError(f"{what}: org must be a float32 tensor of shape (n, 3)")
        return org.shape[0]

    def trace_closest_into(self, org, direction, t, tri, uv=None, t_max=None, stream_ptr=0):
        """trt_trace_closest_device: the rays org / direction (float32 [n, 3]) and t_max (float32 [n], None = TRT_INF) are torch tensors on this
        device, and so are the outputs t (float32 [n]), tri (int32 [n]) and uv (float32 [n, 2], None = not wanted); the work runs on
        stream `stream_ptr` (0 = default).  -> Stats."""
        n = self._ray_count(org, "trace_closest_into")
        f32 = ("torch.float32",)
        p = self._device_arrays("trace_closest_into", [("org", org, f32, 3 * n), ("direction", direction, f32, 3 * n), ("t_max", t_max, f32, n),
                                                       ("t", t, f32, n), ("tri", tri, ("torch.int32",), n), ("uv", uv, f32, 2 * n)])
        if t is None or tri is None:
            raise TrtError("trace_closest_into: t and tri are needed")
        return _call(self._lib, "trt_trace_closest_device", self._h, n, *p, C.c_void_p(stream_ptr))

    def trace_occluded_into(self, org, direction, occluded, t_max=None, stream_ptr=0):
        """trt_trace_occluded_device: org / direction / t_max as for trace_closest_into; occluded: a uint8 or bool tensor [n] on this device that
        receives 1 / True where some hit counts.  The work runs on stream `stream_ptr` (0 = default).  -> Stats."""
        n = self._ray_count(org, "trace_occluded_into")
        f32 = ("torch.float32",)
        p = self._device_arrays("trace_occluded_into", [("org", org, f32, 3 * n), ("direction", direction, f32, 3 * n), ("t_max", t_max, f32, n),
                                                        ("occluded", occluded, ("torch.uint8", "torch.bool"), n)])
        if occluded is None:
            raise TrtError("trace_occluded_into: occluded is needed")
        return _call(self._lib, "trt_trace_occluded_device", self._h, n, *p, C.c_void_p(stream_ptr))

    def trace_points(self, org, dir, tri_v_other, want_stats=False):
        """trt_trace_points on host arrays: per ray the closest hit on this handle's current geometry, evaluated with its barycentrics on
        the coordinates tri_v_other (float32 [n_tris, 3, 3], post-BVH order: Scene.arrays()["tri_v"]'s layout) — where the surface each ray
        sees is, or was, on those vertices.  -> point float32 [n, 3], NaN (bits 0x7FC00000) for a miss[, Stats]."""
        org, dir, _, n = self._rays(org, dir, None, "trace_points")
        v = np.ascontiguousarray(tri_v_other, dtype=np.float32)
        if v.ndim != 3 or v.shape[1:] != (3, 3):
            raise TrtError("trace_points: tri_v_other must be a float32 array of shape (n_tris, 3, 3)")
        point = np.empty((n, 3), np.float32)
        fp = C.POINTER(C.c_float)
        st = _call(self._lib, "trt_trace_points", self._h, n, org.ctypes.data_as(fp), dir.ctypes.data_as(fp), v.ctypes.data_as(fp), v.shape[0], point.ctypes.data_as(fp))
        return (point, st) if want_stats else point

    def trace_points_into(self, org, dir, tri_v_other, point, stream_ptr=0):
        """trt_trace_points_device: org / dir (float32 [n, 3]), tri_v_other (float32 [n_tris, 3, 3]) and point (float32 [n, 3], written) are
        torch tensors on this device; the work runs on stream `stream_ptr` (0 = default).  -> Stats."""
        n = self._ray_count(org, "trace_points_into")
        if not _is_torch(tri_v_other) or tri_v_other.dim() != 3 or tuple(tri_v_other.shape[1:]) != (3, 3):
            raise TrtError("trace_points_into: tri_v_other must be a float32 tensor of shape (n_tris, 3, 3)")
        nt = tri_v_other.shape[0]
        f32 = ("torch.float32",)
        p = self._device_arrays("trace_points_into", [("org", org, f32, 3 * n), ("dir", dir, f32, 3 * n), ("tri_v_other", tri_v_other, f32, 9 * nt),
                                                      ("point", point, f32, 3 * n)])
        if any(x is None for x in p):
            raise TrtError("trace_points_into: org, dir, tri_v_other and point are needed")
        return _call(self._lib, "trt_trace_points_device", self._h, n, p[0], p[1], p[2], nt, p[3], C.c_void_p(stream_ptr))

    def render_rays(self, params, org, dir, streams=None, sample_begin=0, sums=None, sumsq=None):
        """Full paths along caller-supplied rays (trt_render_rays, include/trt.h): org / dir are float32 [S, n, 3] — sample-major, the rays of
        samples [sample_begin, sample_begin + S) of n entries ([n, 3] = one sample); streams: uint32 [n], the "pixel" word of each entry's
        random stream (None = 0..n-1).  The path of (entry i, sample s) is what trt_render traces from its bounce-0 ray on, with the stream
        (seed, streams[i], s) from draw 2.  Adds v = (double)(L / params.spp) and v * v onto sums / sumsq (float64 [n, 3]; None = zeros)
        and returns (sums, sumsq, Stats).  Entries with a NaN, an infinity or a zero direction are not traced and add nothing."""
        org = np.ascontiguousarray(org, dtype=np.float32)
        dir = np.ascontiguousarray(dir, dtype=np.float32)
        if org.ndim == 2:
            org, dir = org[None], dir[None] if dir.ndim == 2 else dir
        if org.ndim != 3 or org.shape[2] != 3 or dir.shape != org.shape:
            raise TrtError("render_rays: org and dir must both be float32 arrays of shape (S, n, 3)")
        n_samples, n = org.shape[0], org.shape[1]
        if streams is not None:
            streams = np.ascontiguousarray(streams, dtype=np.uint32).reshape(-1)
            if streams.size != n:
                raise TrtError(f"render_rays: streams must hold {n} ids")
        sums = self._moments(sums, n, "sums")
        sumsq = self._moments(sumsq, n, "sumsq")
        fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
        st = _call(self._lib, "trt_render_rays", self._h, C.byref(params), n, org.ctypes.data_as(fp), dir.ctypes.data_as(fp),
                   None if streams is None else streams.ctypes.data_as(C.POINTER(C.c_uint32)), int(sample_begin), int(sample_begin) + n_samples,
                   sums.ctypes.data_as(dp), sumsq.ctypes.data_as(dp))
        return sums, sumsq, st

    def render_rays_into(self, params, org, dir, sums, sumsq=None, streams=None, sample_begin=0, stream_ptr=0):
        """trt_render_rays_device: org / dir (float32 [S, n, 3]), streams (int32 or uint32 [n], None = 0..n-1), sums and sumsq (float64 [n, 3],
        in/out; sumsq may be None) are contiguous torch tensors on this device; the work runs on stream `stream_ptr` (0 = default).  -> Stats."""
        if not _is_torch(org) or org.dim() != 3 or org.shape[2] != 3:
            raise TrtError("render_rays_into: org must be a float32 tensor of shape (S, n, 3)")
        n_samples, n = int(org.shape[0]), int(org.shape[1])
        f32, f64 = ("torch.float32",), ("torch.float64",)
        p = self._device_arrays("render_rays_into", [("org", org, f32, 3 * n * n_samples), ("dir", dir, f32, 3 * n * n_samples),
                                                     ("streams", streams, ("torch.int32", "torch.uint32"), n), ("sums", sums, f64, 3 * n),
                                                     ("sumsq", sumsq, f64, 3 * n)])
        if dir is None or sums is None:
            raise TrtError("render_rays_into: dir and sums are needed")
        return _call(self._lib, "trt_render_rays_device", self._h, C.byref(params), n, p[0], p[1], p[2], int(sample_begin), int(sample_begin) + n_samples,
                     p[3], p[4], C.c_void_p(stream_ptr))

    def render_camera(self, params, camera, samples_per_call=1, want_stats=False, on_device=False):
        """The tile of `params` as seen by `camera` (a Camera, e.g. from look_at) — on THIS handle, whatever camera its scene was created with:
        rays are generated on the device (camera_rays_into) and rendered on the device (render_rays_into), samples_per_call samples at a
        time, accumulated in sample order.  -> float32 image [rows, tile_w, 3], bit-identical to Renderer(scene with that camera).render(params)
        [, Stats summed over the calls].  on_device: the image stays a torch tensor on this device (nothing but the stats crosses to the host)."""
        import torch
        pix, (rows, tw) = self._camera_tile(params, "render_camera")
        k = max(1, min(int(samples_per_call), params.spp))
        dev = pix.device
        n = pix.numel()
        org = torch.empty((k, n, 3), dtype=torch.float32, device=dev)
        dirs = torch.empty_like(org)
        sums = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        total = Stats()
        for s0 in range(0, params.spp, k):
            s1 = min(s0 + k, params.spp)
            camera_rays_into(camera, params, pix, s0, s1, org[:s1 - s0], dirs[:s1 - s0], device=self.device, stream_ptr=stream)
            _add_stats(total, self.render_rays_into(params, org[:s1 - s0], dirs[:s1 - s0], sums, streams=pix, sample_begin=s0, stream_ptr=stream))
        image = sums.to(torch.float32).reshape(rows, tw, 3)
        if not on_device:
            image = image.cpu().numpy()
        return (image, total) if want_stats else image

    def render_aov_rays(self, params, org, dir, sample_begin=0, sums=None, want_stats=False):
        """First-hit feature sums along caller-supplied rays (trt_aov_rays, include/trt.h): org / dir are float32 [S, n, 3] — sample-major, the
        rays of samples [sample_begin, sample_begin + S) of n entries ([n, 3] = one sample), as for render_rays.  Per ray the closest hit's
        albedo (texel or Kd), shading normal and distance (a miss, or an entry with a NaN, an infinity or a zero direction: 0, 0, TRT_INF),
        each divided by params.spp as a float and added as a double, in sample order, onto sums: a dict of contiguous float64 arrays
        albedo [n, 3], normal [n, 3], depth [n] (None = all three from zeros; a key left out or None = not wanted, at least one given).
        -> the dict of sums[, Stats]."""
        org = np.ascontiguousarray(org, dtype=np.float32)
        dir = np.ascontiguousarray(dir, dtype=np.float32)
        if org.ndim == 2 and dir.ndim == 2:
            org, dir = org[None], dir[None]
        if org.ndim != 3 or org.shape[2] != 3 or dir.shape != org.shape:
            raise TrtError("render_aov_rays: org and dir must both be float32 arrays of shape (S, n, 3)")
        n_samples, n = org.shape[0], org.shape[1]
        shapes = {"albedo": (n, 3), "normal": (n, 3), "depth": (n,)}
        if sums is None:
            sums = {k: np.zeros(shape, np.float64) for k, shape in shapes.items()}
        if not isinstance(sums, dict) or any(k not in shapes for k in sums):
            raise TrtError("render_aov_rays: sums must be a dict with the keys albedo, normal, depth")
        out = {k: a for k, a in sums.items() if a is not None}
        if not out:
            raise TrtError("render_aov_rays: at least one of albedo, normal, depth is needed")
        for k, a in out.items():
            if not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.shape != shapes[k] or not a.flags["C_CONTIGUOUS"]:
                raise TrtError(f"render_aov_rays: {k} must be a contiguous float64 array of shape {shapes[k]}")
        fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
        ptrs = [out[k].ctypes.data_as(dp) if k in out else None for k in ("albedo", "normal", "depth")]
        st = _call(self._lib, "trt_aov_rays", self._h, C.byref(params), n, org.ctypes.data_as(fp), dir.ctypes.data_as(fp), int(sample_begin),
                   int(sample_begin) + n_samples, *ptrs)
        return (out, st) if want_stats else out

    def render_aov_rays_into(self, params, org, dir, albedo=None, normal=None, depth=None, sample_begin=0, stream_ptr=0):
        """trt_aov_rays_device: org / dir (float32 [S, n, 3]) and the sums albedo, normal (float64 [n, 3]) and depth (float64 [n]; in/out, None =
        not wanted, at least one given) are contiguous torch tensors on this device; the work runs on stream `stream_ptr` (0 = default).  -> Stats."""
        if not _is_torch(org) or org.dim() != 3 or org.shape[2] != 3:
            raise TrtError("render_aov_rays_into: org must be a float32 tensor of shape (S, n, 3)")
        n_samples, n = int(org.shape[0]), int(org.shape[1])
        if albedo is None and normal is None and depth is None:
            raise TrtError("render_aov_rays_into: at least one of albedo, normal, depth is needed")
        f32, f64 = ("torch.float32",), ("torch.float64",)
        p = self._device_arrays("render_aov_rays_into", [("org", org, f32, 3 * n * n_samples), ("dir", dir, f32, 3 * n * n_samples),
                                                         ("albedo", albedo, f64, 3 * n), ("normal", normal, f64, 3 * n), ("depth", depth, f64, n)])
        if dir is None:
            raise TrtError("render_aov_rays_into: dir is needed")
        return _call(self._lib, "trt_aov_rays_device", self._h, C.byref(params), n, p[0], p[1], int(sample_begin), int(sample_begin) + n_samples,
                     p[2], p[3], p[4], C.c_void_p(stream_ptr))

    def _camera_tile(self, params, what):
        """The pixels of the tile of `params` in tile order as an int32 tensor on this device, and the tile's (rows, width)."""
        import torch
        ys, xs, pixels = _tile_pixels(params, what)
        if params.width * params.height > 0x7FFFFFFF:
            raise TrtError(f"{what}: needs width * height < 2^31 (int32 pixel tensors)")
        return torch.from_numpy(pixels.astype(np.int32)).to(torch.device("cuda", self.device)), (int(ys.size), int(xs.size))

    def render_camera_aov(self, params, camera, samples_per_call=16, want_stats=False, on_device=False):
        """The feature buffers of the tile of `params` as seen by `camera` — on THIS handle, whatever camera its scene was created with, as
        render_camera gives the beauty: rays generated on the device (camera_rays_into) and traced on the device (render_aov_rays_into),
        samples_per_call samples at a time, samples [0, params.spp) accumulated in order.  -> dict(albedo=float32 [rows, tile_w, 3],
        normal=float32 [rows, tile_w, 3], depth=float32 [rows, tile_w]), bit-identical to Renderer(scene with that camera).render_aov(params)
        [, Stats summed over the calls].  on_device: the buffers stay torch tensors on this device."""
        import torch
        pix, (rows, tw) = self._camera_tile(params, "render_camera_aov")
        k = max(1, min(int(samples_per_call), params.spp))
        dev = pix.device
        n = pix.numel()
        org = torch.empty((k, n, 3), dtype=torch.float32, device=dev)
        dirs = torch.empty_like(org)
        sums = {"albedo": torch.zeros((n, 3), dtype=torch.float64, device=dev), "normal": torch.zeros((n, 3), dtype=torch.float64, device=dev),
                "depth": torch.zeros(n, dtype=torch.float64, device=dev)}
        stream = torch.cuda.current_stream(dev).cuda_stream
        total = Stats()
        for s0 in range(0, params.spp, k):
            s1 = min(s0 + k, params.spp)
            camera_rays_into(camera, params, pix, s0, s1, org[:s1 - s0], dirs[:s1 - s0], device=self.device, stream_ptr=stream)
            _add_stats(total, self.render_aov_rays_into(params, org[:s1 - s0], dirs[:s1 - s0], sample_begin=s0, stream_ptr=stream, **sums))
        out = {"albedo": sums["albedo"].to(torch.float32).reshape(rows, tw, 3), "normal": sums["normal"].to(torch.float32).reshape(rows, tw, 3),
               "depth": sums["depth"].to(torch.float32).reshape(rows, tw)}
        if not on_device:
            out = {k_: v.cpu().numpy() for k_, v in out.items()}
        return (out, total) if want_stats else out

    def _camera_denoiser_inputs(self, params, camera, aov_spp, samples_per_call, what):
        """The device part of render_camera_denoised, shared with TemporalAccumulator: the denoiser's inputs of the tile of `params` as seen by
        `camera`, as float32 tensors on this device.  -> (color [rows, tw, 3], variance [rows, tw], aov dict, Stats summed, stream pointer)."""
        import torch
        if params.spp < 2:
            raise TrtError(f"{what}: spp must be >= 2 (the variance needs two samples)")
        if params.row_mod > 1:
            raise TrtError(f"{what}: the tile must not interleave rows (it is filtered as one image)")
        pix, (rows, tw) = self._camera_tile(params, what)
        k = max(1, min(int(samples_per_call), params.spp))
        dev = pix.device
        n = pix.numel()
        org = torch.empty((k, n, 3), dtype=torch.float32, device=dev)
        dirs = torch.empty_like(org)
        sums = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        sumsq = torch.zeros_like(sums)
        stream = torch.cuda.current_stream(dev).cuda_stream
        total = Stats()
        for s0 in range(0, params.spp, k):
            s1 = min(s0 + k, params.spp)
            camera_rays_into(camera, params, pix, s0, s1, org[:s1 - s0], dirs[:s1 - s0], device=self.device, stream_ptr=stream)
            _add_stats(total, self.render_rays_into(params, org[:s1 - s0], dirs[:s1 - s0], sums, sumsq, streams=pix, sample_begin=s0, stream_ptr=stream))
        del org, dirs
        pa = make_params(params.width, params.height, min(params.spp, 16) if aov_spp is None else aov_spp, params.seed,
                         tile=(params.x0, params.y0, params.x1, params.y1), max_depth=params.max_depth, flags=params.flags, mem_budget=params.mem_budget)
        aov, st = self.render_camera_aov(pa, camera, samples_per_call=samples_per_call, want_stats=True, on_device=True)
        _add_stats(total, st)
        color = sums.to(torch.float32).reshape(rows, tw, 3)
        variance = mean_luminance_variance(sums, sumsq, params.spp).reshape(rows, tw)
        return color, variance, aov, total, stream

    def _camera_colour_inputs(self, params, camera, aov_spp, samples_per_call, what):
        """_camera_denoiser_inputs without the second moments, for TemporalAccumulator(variance="moments"): the colour sums alone
        (render_rays_into without sumsq, so params.spp may be 1) and the feature buffers.  -> (color [rows, tw, 3], aov dict, Stats summed,
        stream pointer)."""
        import torch
        if params.spp < 1:
            raise TrtError(f"{what}: spp must be >= 1")
        if params.row_mod > 1:
            raise TrtError(f"{what}: the tile must not interleave rows (it is filtered as one image)")
        pix, (rows, tw) = self._camera_tile(params, what)
        k = max(1, min(int(samples_per_call), params.spp))
        dev = pix.device
        n = pix.numel()
        org = torch.empty((k, n, 3), dtype=torch.float32, device=dev)
        dirs = torch.empty_like(org)
        sums = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        total = Stats()
        for s0 in range(0, params.spp, k):
            s1 = min(s0 + k, params.spp)
            camera_rays_into(camera, params, pix, s0, s1, org[:s1 - s0], dirs[:s1 - s0], device=self.device, stream_ptr=stream)
            _add_stats(total, self.render_rays_into(params, org[:s1 - s0], dirs[:s1 - s0], sums, streams=pix, sample_begin=s0, stream_ptr=stream))
        del org, dirs
        pa = make_params(params.width, params.height, min(params.spp, 16) if aov_spp is None else aov_spp, params.seed,
                         tile=(params.x0, params.y0, params.x1, params.y1), max_depth=params.max_depth, flags=params.flags, mem_budget=params.mem_budget)
        aov, st = self.render_camera_aov(pa, camera, samples_per_call=samples_per_call, want_stats=True, on_device=True)
        _add_stats(total, st)
        return sums.to(torch.float32).reshape(rows, tw, 3), aov, total, stream

    def render_camera_denoised(self, params, camera, aov_spp=None, samples_per_call=16, iterations=5, sigma_normal=128, sigma_depth=1.0,
                               sigma_luminance=4.0):
        """render_denoised for the tile of `params` as seen by `camera`, on this handle: the same dict (color, variance, albedo, normal, depth,
        denoised as float32 arrays, and stats) under the same rules (params.spp >= 2, no row interleave, aov_spp None = min(spp, 16)).  The
        beauty and its moments come from render_rays_into on the camera's rays, the variance from mean_luminance_variance's operations on the
        device, the features from render_camera_aov, the filter is denoise_into: nothing but stats crosses to the host until the final copy.
        With the handle's own camera the dict is render_denoised(params)'s, bit for bit."""
        import torch
        color, variance, aov, total, stream = self._camera_denoiser_inputs(params, camera, aov_spp, samples_per_call, "render_camera_denoised")
        denoised = torch.empty_like(color)
        _add_stats(total, denoise_into(color, variance, aov["albedo"], aov["normal"], aov["depth"], denoised, iterations=iterations,
                                       sigma_normal=sigma_normal, sigma_depth=sigma_depth, sigma_luminance=sigma_luminance, stream_ptr=stream))
        out = {"color": color, "variance": variance, "denoised": denoised}
        out.update(aov)
        out = {k_: v.cpu().numpy() for k_, v in out.items()}
        out["stats"] = total
        return out

    def _light_tables(self, upd, lights_from):
        if lights_from is None:
            return
        f = lights_from.flat.contents
        upd.lights, upd.light_tris, upd.n_lights, upd.n_light_tris = f.lights, f.light_tris, f.n_lights, f.n_light_tris

    def update_geometry(self, scene_or_tri_v, tri_vn=None, lights_from=None, want_stats=False):
        """trt_update_geometry: new coordinates for the triangles of this handle, tree topology kept, boxes refitted on the GPU; afterwards the
        handle answers exactly as a fresh Renderer of the moved scene would (include/trt.h).  Given a Scene (after Scene.set_vertices) its flat
        vertices, normals and light tables are taken; given a float32 array [n, 3, 3] (host), tri_vn likewise or None = normals stay, and
        lights_from = a Scene whose light tables to take, or None = they stay (right iff no emissive triangle moved).  -> None or Stats."""
        upd = _abi.GeometryUpdate()
        keep = []
        if isinstance(scene_or_tri_v, Scene):
            f = scene_or_tri_v.flat.contents
            n = f.n_tris
            upd.tri_v, upd.tri_vn = C.cast(f.tri_v, C.c_void_p), C.cast(f.tri_vn, C.c_void_p)
            self._light_tables(upd, scene_or_tri_v)
        else:
            v = np.ascontiguousarray(scene_or_tri_v, dtype=np.float32)
            if v.ndim != 3 or v.shape[1:] != (3, 3):
                raise TrtError("update_geometry: tri_v must be a float32 array of shape (n, 3, 3)")
            n = v.shape[0]
            keep.append(v)
            upd.tri_v = v.ctypes.data
            if tri_vn is not None:
                vn = np.ascontiguousarray(tri_vn, dtype=np.float32)
                if vn.shape != v.shape:
                    raise TrtError("update_geometry: tri_vn must have tri_v's shape")
                keep.append(vn)
                upd.tri_vn = vn.ctypes.data
            self._light_tables(upd, lights_from)
        st = _call(self._lib, "trt_update_geometry", self._h, C.byref(upd), n)
        return st if want_stats else None

    def update_geometry_from(self, tri_v, tri_vn=None, lights_from=None, stream_ptr=0):
        """trt_update_geometry_device: tri_v (float32 [n, 3, 3]) and tri_vn (the same, or None = normals stay) are torch tensors on this device;
        lights_from as for update_geometry (host tables); the work runs on stream `stream_ptr` (0 = default).  -> Stats."""
        if not _is_torch(tri_v) or tri_v.dim() != 3 or tuple(tri_v.shape[1:]) != (3, 3):
            raise TrtError("update_geometry_from: tri_v must be a float32 tensor of shape (n, 3, 3)")
        n = tri_v.shape[0]
        p = self._device_arrays("update_geometry_from", [("tri_v", tri_v, ("torch.float32",), 9 * n), ("tri_vn", tri_vn, ("torch.float32",), 9 * n)])
        upd = _abi.GeometryUpdate()
        upd.tri_v, upd.tri_vn = p[0], p[1]
        self._light_tables(upd, lights_from)
        return _call(self._lib, "trt_update_geometry_device", self._h, C.byref(upd), n, C.c_void_p(stream_ptr))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.trt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GroupRenderer:
    """Owns a trt_group: the scene resident on several GPUs of one node; render() tiles the image over them in
    interleaved row stripes and gathers with ONE ncclGather on the first device (include/trt.h).  `devices` may name one
    device several times (a rehearsal on a one-GPU box: same code path, device copies instead of RCCL)."""

    def __init__(self, scene, devices):
        self._lib = _abi.load_hip()
        self._scene = scene
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        g = C.c_void_p()
        rc = self._lib.trt_group_create(scene.flat, len(devices), devs, C.byref(g))
        if rc != 0:
            raise TrtError(f"trt_group_create failed ({rc}): {self._lib.trt_last_error().decode()}")
        self._g = g
        self.devices = list(devices)

    def render(self, params):
        """-> (float32 image [tile rows, tile_w, 3], Stats summed over the devices, gather + un-interleave ms)."""
        th, tw = params.y1 - params.y0, params.x1 - params.x0
        out = np.empty((th, tw, 3), dtype=np.float32)
        gms = C.c_double(0.0)
        st = _call(self._lib, "trt_group_render", self._g, C.byref(params), out.ctypes.data_as(C.POINTER(C.c_float)), after=(C.byref(gms),))
        return out, st, gms.value

    def render_into(self, params, out_tensor):
        """trt_group_render_device: the image stays on devices[0] (a contiguous float32 torch tensor there with tile rows * tile_w * 3
        elements).  -> (Stats summed over the devices, gather + un-interleave ms)."""
        th, tw = params.y1 - params.y0, params.x1 - params.x0
        if out_tensor.numel() < th * tw * 3 or str(out_tensor.dtype) != "torch.float32" or not out_tensor.is_cuda or not out_tensor.is_contiguous():
            raise TrtError("render_into: need a contiguous float32 device tensor with tile rows * tile_w * 3 elements")
        gms = C.c_double(0.0)
        st = _call(self._lib, "trt_group_render_device", self._g, C.byref(params), C.c_void_p(out_tensor.data_ptr()), after=(C.byref(gms),))
        return st, gms.value

    def close(self):
        if getattr(self, "_g", None):
            self._lib.trt_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def look_at(eye, target, up, fovy_deg, width, height):
    """The pinhole Camera of Camera::setCamera (camera.cpp:3-17) for an eye point, a target, an up vector, a vertical field of view in
    degrees and an image of width x height pixels: the half-height tan(fovy / 2) in double, the viewport extents narrowed to float, the
    basis w = normalize(eye - target), u = normalize(up x w), v = w x u in float32."""
    f = np.float32
    eye, target, up = (np.asarray(a, f).reshape(3) for a in (eye, target, up))

    def normalize(a):
        return a * (f(1.0) / np.sqrt(f((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])))

    vh = f(2.0 * np.tan(float(fovy_deg) * 0.01745329251994329576923690768489 / 2.0))
    vw = f((float(width) / float(height)) * float(vh))
    w = normalize(eye - target)
    u = normalize(np.cross(up, w).astype(f))
    v = np.cross(w, u).astype(f)
    cam = _abi.Camera()
    hor, ver = vw * u, vh * v
    llc = eye - hor / f(2.0) - ver / f(2.0) - w
    for name, a in (("eye", eye), ("lower_left_corner", llc), ("horizontal", hor), ("vertical", ver)):
        setattr(cam, name, _abi.c_float3(*[float(x) for x in a]))
    return cam


def camera_rays(camera, params, pixels, sample_begin, sample_end):
    """trt_camera_rays (host only, no GPU): the rays trt_render traces for the listed pixels (y * width + x), samples [sample_begin,
    sample_end), of any Camera -> (org, dir), float32 [S, n, 3] in the layout Renderer.render_rays reads."""
    pixels = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
    n, n_samples = pixels.size, max(int(sample_end) - int(sample_begin), 0)
    org = np.empty((n_samples, n, 3), np.float32)
    dirs = np.empty_like(org)
    lib = _abi.load_hip()
    fp = C.POINTER(C.c_float)
    rc = lib.trt_camera_rays(C.byref(camera), C.byref(params), n, pixels.ctypes.data_as(C.POINTER(C.c_uint32)), int(sample_begin), int(sample_end),
                             org.ctypes.data_as(fp), dirs.ctypes.data_as(fp))
    if rc != 0:
        raise TrtError(f"trt_camera_rays failed ({rc}): {lib.trt_last_error().decode()}")
    return org, dirs


def camera_rays_into(camera, params, pixels, sample_begin, sample_end, org, dir, device=0, stream_ptr=0):
    """trt_camera_rays_device: the same rays on `device`; pixels (int32 or uint32 [n]), org and dir (float32 [S, n, 3], S = sample_end -
    sample_begin) are contiguous torch tensors there, the work runs on stream `stream_ptr` (0 = default)."""
    n_samples = int(sample_end) - int(sample_begin)
    if not _is_torch(pixels) or pixels.dim() != 1:
        raise TrtError("camera_rays_into: pixels must be a 1-D int32 / uint32 tensor")
    n = pixels.numel()
    ptrs = []
    for name, t, dtypes, need in (("pixels", pixels, ("torch.int32", "torch.uint32"), n), ("org", org, ("torch.float32",), 3 * n * n_samples),
                                  ("dir", dir, ("torch.float32",), 3 * n * n_samples)):
        if (not _is_torch(t) or str(t.dtype) not in dtypes or not t.is_cuda or not t.is_contiguous() or t.numel() != need
                or (t.device.index is not None and t.device.index != int(device))):
            raise TrtError(f"camera_rays_into: {name} must be a contiguous {' or '.join(d[6:] for d in dtypes)} tensor on cuda:{int(device)} with {need} elements")
        ptrs.append(C.c_void_p(t.data_ptr()))
    lib = _abi.load_hip()
    rc = lib.trt_camera_rays_device(int(device), C.byref(camera), C.byref(params), n, ptrs[0], int(sample_begin), int(sample_end), ptrs[1], ptrs[2],
                                    C.c_void_p(stream_ptr))
    if rc != 0:
        raise TrtError(f"trt_camera_rays_device failed ({rc}): {lib.trt_last_error().decode()}")


def center_rays(camera, width, height, flags=0, device=None):
    """The rays through the pixel centres of a width x height image of `camera`, on the grid trt_reproject's step 3 uses (flags:
    TRT_FLAG_FIXED_PIXELS or 0 = the reference's grid): org = eye and dir = llc + horizontal * s + vertical * t - eye, NOT normalised, in
    float32 in that order.  -> (org, dir), float32 [height * width, 3], pixel y * width + x.  device None: numpy arrays; a torch device (or
    its index): torch tensors there, the per-pixel work done by torch operations on that device (on its current stream).  What
    Renderer.trace_points makes of them does not depend on the direction's length."""
    f = np.float32
    w, h = int(width), int(height)
    if w < 1 or h < 1:
        raise TrtError("center_rays: width and height must be >= 1")
    with np.errstate(all="ignore"):  # the reference's grid divides by W - 1 and H - 1
        if int(flags) & TRT_FLAG_FIXED_PIXELS:
            s = (np.arange(w).astype(f) + f(0.5)) / f(w)
            t = (np.arange(h - 1, -1, -1).astype(f) + f(0.5)) / f(h)
        else:
            s = np.arange(w).astype(f) / (f(w) - f(1.0))
            t = np.arange(h, 0, -1).astype(f) / (f(h) - f(1.0))
    eye, llc, hor, ver = (np.array(list(getattr(camera, k)), f) for k in ("eye", "lower_left_corner", "horizontal", "vertical"))
    if device is None:
        with np.errstate(all="ignore"):
            d = ((llc + hor * s[None, :, None]) + ver * t[:, None, None]) - eye
        return np.ascontiguousarray(np.broadcast_to(eye, (h * w, 3))), np.ascontiguousarray(d.reshape(h * w, 3))
    import torch
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    s, t, eye, llc, hor, ver = (torch.from_numpy(a).to(dev) for a in (s, t, eye, llc, hor, ver))
    d = ((llc + hor * s[None, :, None]) + ver * t[:, None, None]) - eye  # separate multiplications and additions: nothing is contracted
    return eye.expand(h * w, 3).contiguous(), d.reshape(h * w, 3).contiguous()


def mean_luminance_variance(sums, sumsq, spp):
    """The variance of each pixel's mean luminance from trt_render_pixels' moments of samples [0, spp) (spp >= 2): per channel the unbiased
    sample variance of the radiance divided by spp, no covariances, weighted by LUMA^2.  sums / sumsq: float64 [n, 3] of v = L / spp and
    v * v.  -> float32 [n].  The CLI's --denoise computes it with the same float64 operations in the same order (host/render.cpp)."""
    n = float(spp)
    L = adaptive.LUMA
    if _is_torch(sums):  # float64 tensors: the same operations in the same order on their device -> a float32 tensor there
        import torch
        n_t = torch.full((), n, dtype=sums.dtype, device=sums.device)  # a tensor: torch divides by a Python number through its reciprocal
        m = sums / n_t
        vv = (sumsq / n_t - m * m) * (n / (n - 1.0))
        vm = torch.where(vv > 0.0, vv, torch.zeros_like(vv)) * n
        return ((L[0] * L[0]) * vm[:, 0] + (L[1] * L[1]) * vm[:, 1] + (L[2] * L[2]) * vm[:, 2]).to(torch.float32)
    m = sums / n
    vv = (sumsq / n - m * m) * (n / (n - 1.0))
    vm = np.where(vv > 0.0, vv, 0.0) * n
    return ((L[0] * L[0]) * vm[:, 0] + (L[1] * L[1]) * vm[:, 1] + (L[2] * L[2]) * vm[:, 2]).astype(np.float32)


def _denoise_params(iterations, sigma_normal, sigma_depth, sigma_luminance):
    dp = _abi.DenoiseParams()
    dp.iterations, dp.sigma_normal = int(iterations), int(sigma_normal)
    dp.sigma_depth, dp.sigma_luminance, dp.flags = float(sigma_depth), float(sigma_luminance), 0
    return dp


def _image_shape(color, what):
    if color.ndim != 3 or color.shape[2] != 3 or color.shape[0] < 1 or color.shape[1] < 1:
        raise TrtError(f"{what}: color must be [height, width, 3]")
    return int(color.shape[0]), int(color.shape[1])


def _device_image(color, what):
    """The image a device entry works on, from its color tensor -> height, width, device."""
    if not _is_torch(color) or color.dim() != 3:
        raise TrtError(f"{what}: color must be a float32 tensor [height, width, 3]")
    return _image_shape(color, what) + (color.device,)


# The image-space passes (denoise*, reproject*) check their arrays in one place each.  `named` lists (name, array, shape, optional) in the
# order of the C entry's arguments; only an optional entry may be None, and a None that is not optional fails as any other wrong array.

def _host_planes(what, named):
    """-> the arrays as contiguous float32 (None for an absent optional one)."""
    arrays = []
    for name, a, shape, optional in named:
        if a is not None or not optional:
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise TrtError(f"{what}: {name} must have shape {shape}, not {a.shape}")
        arrays.append(a)
    return arrays


def _device_planes(what, dev, named):
    """-> the tensors' addresses as c_void_p (None for an absent optional one)."""
    ptrs = []
    for name, t, shape, optional in named:
        if t is None and optional:
            ptrs.append(None)
            continue
        if (not _is_torch(t) or str(t.dtype) != "torch.float32" or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape
                or t.device != dev):
            raise TrtError(f"{what}: {name} must be a contiguous float32 tensor of shape {shape} on {dev}")
        ptrs.append(C.c_void_p(t.data_ptr()))
    return ptrs


def _float_ptrs(arrays):
    return [None if a is None else a.ctypes.data_as(C.POINTER(C.c_float)) for a in arrays]


def _call_hip(entry, *args):
    """Calls `entry` of libtrt_hip.so -> the Stats it filled."""
    return _call(_abi.load_hip(), entry, *args)


def denoise(color, variance, albedo, normal, depth, iterations=5, sigma_normal=128, sigma_depth=1.0, sigma_luminance=4.0, device=0, want_stats=False):
    """The edge-avoiding a-trous filter on `device` (trt_denoise, include/trt.h has the contract): color, albedo, normal [h, w, 3],
    variance (of the pixel's mean luminance) and depth [h, w], all converted to float32.  -> denoised float32 [h, w, 3][, Stats]."""
    color = np.ascontiguousarray(color, dtype=np.float32)
    h, w = _image_shape(color, "denoise")
    bufs = _host_planes("denoise", [("color", color, (h, w, 3), False), ("variance", variance, (h, w), False), ("albedo", albedo, (h, w, 3), False),
                                    ("normal", normal, (h, w, 3), False), ("depth", depth, (h, w), False)])
    out = np.empty((h, w, 3), np.float32)
    dp = _denoise_params(iterations, sigma_normal, sigma_depth, sigma_luminance)
    st = _call_hip("trt_denoise", int(device), C.byref(dp), w, h, *_float_ptrs(bufs + [out]))
    return (out, st) if want_stats else out


def denoise_into(color, variance, albedo, normal, depth, out, iterations=5, sigma_normal=128, sigma_depth=1.0, sigma_luminance=4.0, stream_ptr=0):
    """trt_denoise_device: the buffers of denoise() as contiguous float32 torch tensors on one device (color, albedo, normal and out
    [h, w, 3]; variance and depth [h, w]), the work on stream `stream_ptr` (0 = default).  Writes out; -> Stats."""
    h, w, dev = _device_image(color, "denoise_into")
    ptrs = _device_planes("denoise_into", dev, [("color", color, (h, w, 3), False), ("variance", variance, (h, w), False),
                                                ("albedo", albedo, (h, w, 3), False), ("normal", normal, (h, w, 3), False),
                                                ("depth", depth, (h, w), False), ("out", out, (h, w, 3), False)])
    dp = _denoise_params(iterations, sigma_normal, sigma_depth, sigma_luminance)
    return _call_hip("trt_denoise_device", int(dev.index or 0), C.byref(dp), w, h, *ptrs, C.c_void_p(stream_ptr))


def _despeckle_params(radius, sigma):
    dp = _abi.DespeckleParams()
    dp.radius, dp.sigma, dp.flags = int(radius), float(sigma), 0
    return dp


def despeckle(color, albedo, depth, variance=None, radius=1, sigma=3.0, device=0, want_stats=False):
    """The firefly clamp on `device` (trt_despeckle, include/trt.h has the contract, its bias and its limits): a hit pixel whose demodulated
    luminance exceeds mean + sigma * deviation of the (2 radius + 1)^2 window around it (radius 1 or 2, the pixel itself left out) is scaled
    down to that bound, and a pixel that is not a number is replaced by the window's mean.  It runs on a frame BEFORE reproject*() and
    denoise().  color, albedo [h, w, 3], depth [h, w], variance [h, w] or None, all converted to float32.
    -> dict(color [h, w, 3], variance [h, w] (variance * scale^2) or None, scale [h, w]: the factor of each pixel, 1 where it passed)[, Stats]."""
    color = np.ascontiguousarray(color, dtype=np.float32)
    h, w = _image_shape(color, "despeckle")
    bufs = _host_planes("despeckle", [("color", color, (h, w, 3), False), ("variance", variance, (h, w), True), ("albedo", albedo, (h, w, 3), False),
                                      ("depth", depth, (h, w), False)])
    out = {"color": np.empty((h, w, 3), np.float32), "variance": None if variance is None else np.empty((h, w), np.float32),
           "scale": np.empty((h, w), np.float32)}
    dp = _despeckle_params(radius, sigma)
    st = _call_hip("trt_despeckle", int(device), C.byref(dp), w, h, *_float_ptrs(bufs + list(out.values())))
    return (out, st) if want_stats else out


def despeckle_into(color, albedo, depth, out_color, variance=None, out_variance=None, out_scale=None, radius=1, sigma=3.0, stream_ptr=0):
    """trt_despeckle_device: the buffers of despeckle() as contiguous float32 torch tensors on one device (color, albedo and out_color
    [h, w, 3]; depth [h, w]; variance and out_variance [h, w], both or neither; out_scale [h, w] or None; no output may be an input), the
    work on stream `stream_ptr` (0 = default).  Writes the outputs that are given; -> Stats."""
    h, w, dev = _device_image(color, "despeckle_into")
    ptrs = _device_planes("despeckle_into", dev, [("color", color, (h, w, 3), False), ("variance", variance, (h, w), True),
                                                  ("albedo", albedo, (h, w, 3), False), ("depth", depth, (h, w), False),
                                                  ("out_color", out_color, (h, w, 3), False), ("out_variance", out_variance, (h, w), True),
                                                  ("out_scale", out_scale, (h, w), True)])
    dp = _despeckle_params(radius, sigma)
    return _call_hip("trt_despeckle_device", int(dev.index or 0), C.byref(dp), w, h, *ptrs, C.c_void_p(stream_ptr))


HISTORY_KEYS = ("cv", "length", "normal", "depth")
MOMENTS_HISTORY_KEYS = HISTORY_KEYS + ("mom",)


def _reproject_params(cur, prev, alpha, depth_tolerance, normal_threshold, max_history, flags):
    rp = _abi.ReprojectParams()
    rp.cur, rp.prev = cur, cur if prev is None else prev
    rp.alpha, rp.depth_tolerance, rp.normal_threshold = float(alpha), float(depth_tolerance), float(normal_threshold)
    rp.max_history, rp.flags = float(max_history), int(flags)
    return rp


def _moments_params(cur, prev, alpha, depth_tolerance, normal_threshold, max_history, flags, min_frames, sigma_normal, sigma_depth):
    mp = _abi.MomentsParams()
    mp.rp = _reproject_params(cur, prev, alpha, depth_tolerance, normal_threshold, max_history, flags)
    mp.min_frames, mp.sigma_normal, mp.sigma_depth = int(min_frames), int(sigma_normal), float(sigma_depth)
    return mp


def _history_planes(history, what, keys, h, w):
    """The history's entries of a validator's list: all absent (history None), or every key of `keys` given."""
    if history is None:
        history = dict.fromkeys(keys)
    elif not isinstance(history, dict) or any(history.get(k) is None for k in keys):
        raise TrtError(f"{what}: history must be None or a dict with the keys {', '.join(keys)}")
    shapes = {"cv": (h, w, 4), "length": (h, w), "normal": (h, w, 3), "depth": (h, w), "mom": (h, w, 4)}
    return [("history " + k, history[k], shapes[k], True) for k in keys]


def _host_outputs(h, w, keys):
    shapes = {"color": (h, w, 3), "variance": (h, w), "cv": (h, w, 4), "length": (h, w), "mom": (h, w, 4)}
    return {k: np.empty(shapes[k], np.float32) for k in keys}


def _reproject_host(what, color, variance, albedo, normal, depth, prev_point, cur, prev, history, alpha, depth_tolerance, normal_threshold,
                    max_history, flags, device, want_stats):
    """reproject() (prev_point None) and reproject_motion() on host arrays.  An input left None goes to the library, which refuses it."""
    color = np.ascontiguousarray(color, dtype=np.float32)
    h, w = _image_shape(color, what)
    named = [("color", color, (h, w, 3), False), ("variance", variance, (h, w), True), ("albedo", albedo, (h, w, 3), True),
             ("normal", normal, (h, w, 3), True), ("depth", depth, (h, w), True)]
    if what == "reproject_motion":
        if prev_point is None:
            raise TrtError("reproject_motion: prev_point is needed")
        named.append(("prev_point", prev_point, (h, w, 3), False))
    bufs = _host_planes(what, named + _history_planes(history, what, HISTORY_KEYS, h, w))
    out = _host_outputs(h, w, ("color", "variance", "cv", "length"))
    rp = _reproject_params(cur, prev, alpha, depth_tolerance, normal_threshold, max_history, flags)
    st = _call_hip("trt_" + what, int(device), C.byref(rp), w, h, *_float_ptrs(bufs + list(out.values())))
    return (out, st) if want_stats else out


def reproject(color, variance, albedo, normal, depth, cur, prev=None, history=None, alpha=0.2, depth_tolerance=0.1, normal_threshold=0.9,
              max_history=255.0, flags=0, device=0, want_stats=False):
    """Temporal accumulation on `device` (trt_reproject, include/trt.h has the contract): the current frame's color, albedo, normal [h, w, 3],
    variance and depth [h, w] (denoise()'s inputs), the Cameras of this frame and of the history (prev None = cur: a still camera), and the
    history: None on a first frame, else dict(cv [h, w, 4], length [h, w], normal [h, w, 3], depth [h, w]) — `cv` and `length` as an earlier
    call returned them, `normal` and `depth` that frame's own.  flags: TRT_FLAG_FIXED_PIXELS if the frames were rendered with it.  The frames
    must have been rendered with different seeds.  -> dict(color [h, w, 3], variance [h, w]: what goes on to denoise(); cv, length: the next
    history, with this frame's normal and depth)[, Stats]."""
    return _reproject_host("reproject", color, variance, albedo, normal, depth, None, cur, prev, history, alpha, depth_tolerance, normal_threshold,
                           max_history, flags, device, want_stats)


def reproject_motion(color, variance, albedo, normal, depth, prev_point, cur, prev=None, history=None, alpha=0.2, depth_tolerance=0.1,
                     normal_threshold=0.9, max_history=255.0, flags=0, device=0, want_stats=False):
    """reproject() for surfaces that move (trt_reproject_motion): one more input, prev_point [h, w, 3] — where the surface seen through each
    pixel was when the history frame was rendered: Renderer.trace_points along center_rays(cur, w, h, flags) on the vertices of that time,
    NaN where the ray misses.  The history is looked up where that point lay in `prev` (None = cur), with a still camera too.  Everything
    else, and the result, as reproject()."""
    return _reproject_host("reproject_motion", color, variance, albedo, normal, depth, prev_point, cur, prev, history, alpha, depth_tolerance,
                           normal_threshold, max_history, flags, device, want_stats)


def _reproject_device(what, color, variance, albedo, normal, depth, prev_point, cur, prev, out_color, out_variance, out_cv, out_length, history,
                      alpha, depth_tolerance, normal_threshold, max_history, flags, stream_ptr):
    """reproject_into() (prev_point None) and reproject_motion_into() on torch tensors."""
    h, w, dev = _device_image(color, what)
    motion = what == "reproject_motion_into"
    named = [("color", color, (h, w, 3), False), ("variance", variance, (h, w), False), ("albedo", albedo, (h, w, 3), False),
             ("normal", normal, (h, w, 3), False), ("depth", depth, (h, w), False)]
    named += [("prev_point", prev_point, (h, w, 3), False)] if motion else []
    named += _history_planes(history, what, HISTORY_KEYS, h, w)
    named += [("out_color", out_color, (h, w, 3), False), ("out_variance", out_variance, (h, w), False), ("out_cv", out_cv, (h, w, 4), False),
              ("out_length", out_length, (h, w), False)]
    ptrs = _device_planes(what, dev, named)
    rp = _reproject_params(cur, prev, alpha, depth_tolerance, normal_threshold, max_history, flags)
    return _call_hip("trt_reproject_motion_device" if motion else "trt_reproject_device", int(dev.index or 0), C.byref(rp), w, h, *ptrs,
                     C.c_void_p(stream_ptr))


def reproject_into(color, variance, albedo, normal, depth, cur, prev, out_color, out_variance, out_cv, out_length, history=None, alpha=0.2,
                   depth_tolerance=0.1, normal_threshold=0.9, max_history=255.0, flags=0, stream_ptr=0):
    """trt_reproject_device: the buffers of reproject() as contiguous float32 torch tensors on one device (the history's too; out_color
    [h, w, 3], out_variance [h, w], out_cv [h, w, 4], out_length [h, w]; no output may be an input), the work on stream `stream_ptr`
    (0 = default).  Writes the four outputs; -> Stats."""
    return _reproject_device("reproject_into", color, variance, albedo, normal, depth, None, cur, prev, out_color, out_variance, out_cv, out_length,
                             history, alpha, depth_tolerance, normal_threshold, max_history, flags, stream_ptr)


def reproject_motion_into(color, variance, albedo, normal, depth, prev_point, cur, prev, out_color, out_variance, out_cv, out_length, history=None,
                          alpha=0.2, depth_tolerance=0.1, normal_threshold=0.9, max_history=255.0, flags=0, stream_ptr=0):
    """trt_reproject_motion_device: reproject_into() with prev_point (float32 [h, w, 3] on the same device, Renderer.trace_points_into's
    output) after depth.  Writes the four outputs; -> Stats."""
    return _reproject_device("reproject_motion_into", color, variance, albedo, normal, depth, prev_point, cur, prev, out_color, out_variance, out_cv,
                             out_length, history, alpha, depth_tolerance, normal_threshold, max_history, flags, stream_ptr)


def reproject_moments(color, albedo, normal, depth, cur, prev=None, history=None, prev_point=None, alpha=0.2, depth_tolerance=0.1,
                      normal_threshold=0.9, max_history=255.0, flags=0, min_frames=4, sigma_normal=128, sigma_depth=1.0, device=0, want_stats=False):
    """reproject() for frames of one sample per pixel (trt_reproject_moments, include/trt.h has the contract): no variance goes in; it is
    estimated from the history of the luminance's moments where the history is at least min_frames long, and from a 7 x 7 neighbourhood
    (sigma_normal, sigma_depth: denoise()'s edge-stopping weights) where it is not.  The history has one more entry than reproject()'s:
    dict(cv, length, normal, depth, mom [h, w, 4]); prev_point [h, w, 3] as for reproject_motion(), or None = the cameras alone.
    -> dict(color, variance, cv, length, mom)[, Stats]: color and variance go on to denoise(), cv, length and mom are the next history."""
    what = "reproject_moments"
    color = np.ascontiguousarray(color, dtype=np.float32)
    h, w = _image_shape(color, what)
    named = [("color", color, (h, w, 3), False), ("albedo", albedo, (h, w, 3), True), ("normal", normal, (h, w, 3), True), ("depth", depth, (h, w), True),
             ("prev_point", prev_point, (h, w, 3), True)]  # an input left None goes to the library, which refuses it
    bufs = _host_planes(what, named + _history_planes(history, what, MOMENTS_HISTORY_KEYS, h, w))
    out = _host_outputs(h, w, ("color", "variance", "cv", "length", "mom"))
    mp = _moments_params(cur, prev, alpha, depth_tolerance, normal_threshold, max_history, flags, min_frames, sigma_normal, sigma_depth)
    st = _call_hip("trt_reproject_moments", int(device), C.byref(mp), w, h, *_float_ptrs(bufs + list(out.values())))
    return (out, st) if want_stats else out


def reproject_moments_into(color, albedo, normal, depth, cur, prev, out_color, out_variance, out_cv, out_length, out_mom, history=None,
                           prev_point=None, alpha=0.2, depth_tolerance=0.1, normal_threshold=0.9, max_history=255.0, flags=0, min_frames=4,
                           sigma_normal=128, sigma_depth=1.0, stream_ptr=0):
    """trt_reproject_moments_device: the buffers of reproject_moments() as contiguous float32 torch tensors on one device (the history's
    and prev_point too; out_color [h, w, 3], out_variance [h, w], out_cv [h, w, 4], out_length [h, w], out_mom [h, w, 4]; no output may be
    an input), the work on stream `stream_ptr` (0 = default).  Writes the five outputs; -> Stats."""
    what = "reproject_moments_into"
    h, w, dev = _device_image(color, what)
    named = [("color", color, (h, w, 3), False), ("albedo", albedo, (h, w, 3), False), ("normal", normal, (h, w, 3), False), ("depth", depth, (h, w), False),
             ("prev_point", prev_point, (h, w, 3), True)]
    named += _history_planes(history, what, MOMENTS_HISTORY_KEYS, h, w)
    named += [("out_color", out_color, (h, w, 3), False), ("out_variance", out_variance, (h, w), False), ("out_cv", out_cv, (h, w, 4), False),
              ("out_length", out_length, (h, w), False), ("out_mom", out_mom, (h, w, 4), False)]
    ptrs = _device_planes(what, dev, named)
    mp = _moments_params(cur, prev, alpha, depth_tolerance, normal_threshold, max_history, flags, min_frames, sigma_normal, sigma_depth)
    return _call_hip("trt_reproject_moments_device", int(dev.index or 0), C.byref(mp), w, h, *ptrs, C.c_void_p(stream_ptr))


class TemporalAccumulator:
    """A frame loop over a moving camera: every frame is rendered, blended into the reprojected history of the frames before it
    (reproject_into) and then filtered (denoise_into).  `params` names the image (its tile must be the whole image, spp >= 2, no row
    interleave: render_camera_denoised's rules) and the first seed; alpha, depth_tolerance, normal_threshold and max_history are
    trt_reproject's, aov_spp and samples_per_call render_camera_denoised's, denoise_kw (iterations, sigma_normal, sigma_depth,
    sigma_luminance) denoise_into's.  The history lives in torch tensors on the renderer's device and belongs to this object alone: the
    handle keeps nothing, and two accumulators on one renderer do not interact.
    variance="samples" (the default) takes the variance from the samples of each frame, hence spp >= 2.  variance="moments" takes it from
    the history instead (reproject_moments_into: the luminance's moments over time, a spatial estimate while the history is shorter than
    min_frames): spp may be 1, only the colour sums are rendered, the history keeps one more record (mom), and frame()'s own `variance`
    is None.  The accumulated colour and the history length are the same either way.
    despeckle=None (the default) leaves the frames as rendered.  True, or a dict with `radius` and / or `sigma`, sends every frame's colour
    (and, with variance="samples", its variance) through despeckle_into on the frame's stream before the reprojection: the history and the
    filter then see the clamped frame, frame() also returns `despeckle_scale`, and its `color` / `variance` stay the frame as rendered.  The
    clamp is biased and cannot tell a small emitter from a firefly (include/trt.h, trt_despeckle), hence off unless asked for.
    Geometry that moves keeps its history too: after Renderer.update_geometry_from(v1) (or update_geometry) pass the vertices the handle had
    when the previous frame was rendered, frame(camera, moved_from=v0), and every pixel looks its history up where the surface it shows
    was then.  The loop is `r.update_geometry_from(v1); acc.frame(cam, moved_from=v0)`; without moved_from a moved surface keeps or loses
    its history by the depth and normal tests alone, as trt_reproject documents."""

    def __init__(self, renderer, params, alpha=0.2, depth_tolerance=0.1, normal_threshold=0.9, max_history=255.0, aov_spp=None,
                 samples_per_call=16, variance="samples", min_frames=4, despeckle=None, **denoise_kw):
        unknown = set(denoise_kw) - {"iterations", "sigma_normal", "sigma_depth", "sigma_luminance"}
        if unknown:
            raise TrtError(f"TemporalAccumulator: unknown argument {sorted(unknown)[0]}")
        if variance not in ("samples", "moments"):
            raise TrtError("TemporalAccumulator: variance must be 'samples' or 'moments'")
        if despeckle is True:
            despeckle = {}
        if despeckle is not None:
            if not isinstance(despeckle, dict):
                raise TrtError("TemporalAccumulator: despeckle must be None, True or a dict with the keys radius, sigma")
            unknown = set(despeckle) - {"radius", "sigma"}
            if unknown:
                raise TrtError(f"TemporalAccumulator: unknown despeckle key {sorted(unknown, key=str)[0]}")
        if (params.x0, params.y0, params.x1, params.y1) != (0, 0, params.width, params.height):
            raise TrtError("TemporalAccumulator: the tile must be the whole image (the cameras' pixel grid is the image's)")
        if variance == "samples" and params.spp < 2:
            raise TrtError("TemporalAccumulator: spp must be >= 2 (the variance needs two samples)")
        if params.spp < 1:
            raise TrtError("TemporalAccumulator: spp must be >= 1")
        if params.row_mod > 1:
            raise TrtError("TemporalAccumulator: the tile must not interleave rows (it is filtered as one image)")
        self.renderer = renderer
        self.params = Params.from_buffer_copy(params)
        self.reproject_kw = dict(alpha=alpha, depth_tolerance=depth_tolerance, normal_threshold=normal_threshold, max_history=max_history,
                                 flags=params.flags & TRT_FLAG_FIXED_PIXELS)
        self.render_kw = dict(aov_spp=aov_spp, samples_per_call=samples_per_call)
        self.denoise_kw = denoise_kw
        self.variance = variance
        self.despeckle_kw = None if despeckle is None else dict(despeckle)
        # stage B of reproject_moments_into weighs its taps as the filter does
        self.moments_kw = dict(min_frames=min_frames, **{k: denoise_kw[k] for k in ("sigma_normal", "sigma_depth") if k in denoise_kw})
        self.frame_index = 0  # frames rendered so far; reset() does not rewind it, so that no seed is used twice
        self._history = None
        self._camera = None

    def reset(self):
        """Drops the history: the next frame is a first frame.  For a cut, or a change frame(moved_from=...) cannot follow (new topology,
        a surface turned by more than the normal threshold allows); geometry moved by trt_update_geometry alone needs no reset: give
        frame() the previous vertices."""
        self._history = None
        self._camera = None

    def _previous_points(self, camera, moved_from, h, w, device, stream, total):
        """Where the surface each pixel of `camera` shows lay on the vertices `moved_from` (center_rays -> Renderer.trace_points_into, its
        Stats added to `total`) -> float32 [h, w, 3] on `device`; None, and nothing traced, on a first frame or without moved_from."""
        import torch
        if moved_from is None or self._history is None:
            return None
        v0 = moved_from if _is_torch(moved_from) else torch.from_numpy(moved_from).to(device)
        org, dirs = center_rays(camera, w, h, flags=self.reproject_kw["flags"], device=device)
        point = torch.empty((h * w, 3), dtype=torch.float32, device=device)
        _add_stats(total, self.renderer.trace_points_into(org, dirs, v0.contiguous(), point, stream_ptr=stream))
        return point.view(h, w, 3)

    def frame(self, camera, on_device=False, moved_from=None):
        """Renders the frame seen by `camera` with seed params.seed + frame_index (mod 2^32), accumulates and denoises it.  -> dict(color,
        variance, albedo, normal, depth: the frame's own buffers; accumulated, accumulated_variance: the blend with the reprojected history;
        history_length; denoised: the filtered accumulated image) as float32 arrays (on_device: torch tensors on the renderer's device), and
        stats: the Stats of every call summed.  With variance="moments" the frame has no variance of its own (`variance` is None) and
        accumulated_variance is reproject_moments_into's estimate.  With despeckle the dict also holds despeckle_scale [h, w], the factor
        the clamp gave each pixel of the frame before it was accumulated; color and variance are the frame as rendered.
        moved_from: None, or the tri_v the handle's geometry had when the previous frame was rendered (float32 [n_tris, 3, 3], a torch tensor
        on the renderer's device or a numpy array): the history is then found through center_rays -> Renderer.trace_points_into(...,
        moved_from) -> reproject_motion_into, all on the frame's stream, in place of reproject_into.  Its shape is checked before anything
        is rendered; on a first frame (or after reset()) there is no history to look up, and nothing is traced."""
        import torch
        if moved_from is not None:
            if _is_torch(moved_from):
                ok = moved_from.dim() == 3 and tuple(moved_from.shape[1:]) == (3, 3) and str(moved_from.dtype) == "torch.float32"
            else:
                moved_from = np.ascontiguousarray(moved_from, dtype=np.float32)
                ok = moved_from.ndim == 3 and moved_from.shape[1:] == (3, 3)
            if not ok:
                raise TrtError("TemporalAccumulator.frame: moved_from must be a float32 array or tensor of shape (n_tris, 3, 3)")
            n_tris = self.renderer._scene.flat.contents.n_tris
            if moved_from.shape[0] != n_tris:
                raise TrtError(f"TemporalAccumulator.frame: moved_from holds {moved_from.shape[0]} triangles, the handle {n_tris}")
        p = Params.from_buffer_copy(self.params)
        p.seed = (self.params.seed + self.frame_index) & 0xFFFFFFFF
        moments = self.variance == "moments"
        if moments:
            color, aov, total, stream = self.renderer._camera_colour_inputs(p, camera, self.render_kw["aov_spp"], self.render_kw["samples_per_call"],
                                                                            "TemporalAccumulator.frame")
            variance = None
        else:
            color, variance, aov, total, stream = self.renderer._camera_denoiser_inputs(p, camera, self.render_kw["aov_spp"], self.render_kw["samples_per_call"],
                                                                                       "TemporalAccumulator.frame")
        h, w = color.shape[0], color.shape[1]
        acc, acc_var = torch.empty_like(color), torch.empty_like(aov["depth"])
        cv, length = torch.empty((h, w, 4), dtype=torch.float32, device=color.device), torch.empty_like(aov["depth"])
        mom = torch.empty_like(cv) if moments else None
        scale, frame_color, frame_variance = None, color, variance
        if self.despeckle_kw is not None:  # the history and the filter get the clamped frame; the caller keeps the frame as rendered
            color, scale = torch.empty_like(frame_color), torch.empty_like(aov["depth"])
            variance = None if frame_variance is None else torch.empty_like(frame_variance)
            _add_stats(total, despeckle_into(frame_color, aov["albedo"], aov["depth"], color, variance=frame_variance, out_variance=variance,
                                             out_scale=scale, stream_ptr=stream, **self.despeckle_kw))
        point = self._previous_points(camera, moved_from, h, w, color.device, stream, total)
        if moments:
            _add_stats(total, reproject_moments_into(color, aov["albedo"], aov["normal"], aov["depth"], camera, self._camera, acc, acc_var, cv, length, mom,
                                                     history=self._history, prev_point=point, stream_ptr=stream, **self.reproject_kw, **self.moments_kw))
        elif point is None:
            _add_stats(total, reproject_into(color, variance, aov["albedo"], aov["normal"], aov["depth"], camera, self._camera, acc, acc_var, cv, length,
                                             history=self._history, stream_ptr=stream, **self.reproject_kw))
        else:
            _add_stats(total, reproject_motion_into(color, variance, aov["albedo"], aov["normal"], aov["depth"], point, camera, self._camera,
                                                    acc, acc_var, cv, length, history=self._history, stream_ptr=stream, **self.reproject_kw))
        denoised = torch.empty_like(color)
        _add_stats(total, denoise_into(acc, acc_var, aov["albedo"], aov["normal"], aov["depth"], denoised, stream_ptr=stream, **self.denoise_kw))
        self._history = {"cv": cv, "length": length, "normal": aov["normal"], "depth": aov["depth"]}
        if moments:
            self._history["mom"] = mom
        self._camera = Camera.from_buffer_copy(camera)
        self.frame_index += 1
        out = {"color": frame_color, "variance": frame_variance, "accumulated": acc, "accumulated_variance": acc_var, "history_length": length, "denoised": denoised}
        out.update(aov)
        if scale is not None:
            out["despeckle_scale"] = scale
        if on_device:  # history_length, normal and depth are the next frame's history: the caller gets copies to do with as they please
            out.update({k_: out[k_].clone() for k_ in ("history_length", "normal", "depth")})
        else:
            out = {k_: None if v is None else v.cpu().numpy() for k_, v in out.items()}
        out["stats"] = total
        return out


def tonemap(image):
    """imshow()'s transfer: (uchar) clamp(pow(x, 1/2.2f) * 255, 0, 255) (main.cpp:34-36)."""
    lib = _abi.load_host()
    img = np.ascontiguousarray(image, dtype=np.float32)
    h, w = img.shape[0], img.shape[1]
    out = np.empty((h, w, 3), np.uint8)
    if lib.trth_tonemap(img.ctypes.data_as(C.POINTER(C.c_float)), w, h, out.ctypes.data_as(C.POINTER(C.c_uint8))) != 0:
        raise TrtError(lib.trth_last_error().decode())
    return out


def imshow(image, path):
    """Writes the linear image as <path> (PNG, stored deflate) after the reference's gamma."""
    lib = _abi.load_host()
    img = np.ascontiguousarray(image, dtype=np.float32)
    h, w = img.shape[0], img.shape[1]
    if lib.trth_write_png(os.fsencode(path), w, h, img.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise TrtError(lib.trth_last_error().decode())


def write_pfm(path, data):
    """Writes float32 [h, w, 3] (PF) or [h, w] (Pf) as a portable float map (trth_write_pfm): scale -1.0, little-endian, rows bottom to top."""
    lib = _abi.load_host()
    a = np.ascontiguousarray(data, dtype=np.float32)
    if a.ndim == 2:
        channels = 1
    elif a.ndim == 3 and a.shape[2] == 3:
        channels = 3
    else:
        raise TrtError("write_pfm: data must be [h, w] or [h, w, 3]")
    if lib.trth_write_pfm(os.fsencode(path), a.shape[1], a.shape[0], channels, a.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise TrtError(lib.trth_last_error().decode())
