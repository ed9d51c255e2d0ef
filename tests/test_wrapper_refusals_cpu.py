"""What the Python wrappers of the render, feature and ray-query entries refuse, and with which words — no GPU needed.

One table per kind of check, every row a call and the complete message it has to raise:
  - the host checks (empty tiles, width * height >= 2^31, wrong numpy arrays) on a Renderer made without trt_create whose library
    knows trt_rows_selected (plain host code) and nothing else: a wrapper that reaches another entry with these arguments fails the test;
  - the device-tensor checks, on stand-in tensors that claim a device this machine need not have: wrong dtype, shape, device or
    contiguity, an absent mandatory tensor, one element too few where an entry takes "at least", one too many where it takes "exactly";
  - the other side of each size rule: the call that is one element inside the rule reaches the entry it names;
  - the message of a failed entry, for every wrapper that reports one.
"""
import numpy as np
import pytest

import tinyraytracing_amd as T
from tinyraytracing_amd import _abi

F32, F64 = np.float32, np.float64
CAM = T.look_at((0, 0, -5), (0, 0, 0), (0, 1, 0), 40.0, 64, 36)
P = T.make_params(64, 36, 4, 1)                                # 36 rows of 64 pixels
NO_WIDTH = T.make_params(64, 36, 4, 1, tile=(5, 0, 5, 36))     # an empty tile: no columns ...
NO_ROWS = T.make_params(64, 36, 4, 1, tile=(0, 0, 64, 1), rows=(1, 2, 1))  # ... or no selected row
BIG = T.make_params(65536, 32768, 4, 1, tile=(0, 0, 2, 2))     # width * height = 2^31: the smallest image the int32 pixel tensors cannot index
N = 5
ORG, DIRS = np.zeros((N, 3), F32), np.ones((N, 3), F32)


class _Library:
    """Stands in for libtrt_hip.so.  rc None: no entry may be reached.  Otherwise every entry notes its name and returns rc."""

    def __init__(self, rc=None):
        self.rc, self.calls = rc, []
        self.trt_rows_selected = _abi.load_hip().trt_rows_selected  # host code: the rows a Params selects

    def trt_last_error(self):
        return b"stand-in"

    def __getattr__(self, name):
        if self.rc is None:
            raise AssertionError(f"the wrapper reached the library ({name}) with arguments it has to refuse")

        def entry(*args):
            self.calls.append(name)
            return self.rc
        return entry


def _renderer(rc=None):
    r = T.Renderer.__new__(T.Renderer)  # no trt_create: the checks under test come before any call into the library
    r._lib, r._h, r.device = _Library(rc), None, 0
    return r


def _group(rc=None):
    g = T.GroupRenderer.__new__(T.GroupRenderer)
    g._lib, g._g, g.devices = _Library(rc), None, [0]
    return g


def _tensor(shape, dtype="float32", device=("cuda", 0), contiguous=True):
    """A stand-in for a torch tensor on `device`: what the wrappers ask of a tensor before they hand its address on."""
    import torch

    class Tensor:
        is_cuda = device[0] == "cuda"

        def dim(self):
            return len(self.shape)

        def numel(self):
            return int(np.prod(self.shape, dtype=np.int64))

        def is_contiguous(self):
            return contiguous

        def data_ptr(self):
            return 0x1000

    Tensor.__module__ = "torch"
    t = Tensor()
    t.shape, t.dtype, t.device = tuple(shape), getattr(torch, dtype), torch.device(*device)
    return t


def _refused(call, message, *what):
    with pytest.raises(T.TrtError) as e:
        call(*what)
    assert str(e.value) == message


HOST_REFUSALS = [
    (lambda r: r.render(NO_WIDTH), "render: empty tile"),
    (lambda r: r.render(NO_ROWS), "render: empty tile"),
    (lambda r: r.render_samples(NO_WIDTH, 0, 1), "render_samples: empty tile"),
    (lambda r: r.render_samples(NO_ROWS, 0, 1), "render_samples: empty tile"),
    (lambda r: r.render_samples(P, 0, 1, accum=np.zeros((36, 64, 3), F32)),
     "render_samples: accum must be a contiguous float64 array of shape (rows, tile_w, 3)"),
    (lambda r: r.render_samples(P, 0, 1, accum=np.zeros((36, 64), F64)),
     "render_samples: accum must be a contiguous float64 array of shape (rows, tile_w, 3)"),
    (lambda r: r.render_samples(P, 0, 1, accum=np.zeros((3, 64, 36), F64).T),
     "render_samples: accum must be a contiguous float64 array of shape (rows, tile_w, 3)"),
    (lambda r: r.render_aov(NO_WIDTH), "render_aov: empty tile"),
    (lambda r: r.render_aov(NO_ROWS), "render_aov: empty tile"),
    (lambda r: r.render_aov_into(NO_WIDTH), "render_aov_into: empty tile"),  # the tile before the all-None outputs
    (lambda r: r.render_aov_into(P), "render_aov_into: at least one of albedo, normal, depth is needed"),
    (lambda r: r.render_adaptive(NO_WIDTH, 0.1, 1, 2, 1), "render_adaptive: empty tile"),
    (lambda r: r.render_adaptive(NO_ROWS, 0.1, 1, 2, 1, on_device=True), "render_adaptive: empty tile"),
    (lambda r: r.render_denoised(T.make_params(64, 36, 1, 1, tile=(5, 0, 5, 36))), "render_denoised: spp must be >= 2 (the variance needs two samples)"),
    (lambda r: r.render_denoised(NO_ROWS), "render_denoised: the tile must not interleave rows (it is filtered as one image)"),
    (lambda r: r.render_denoised(NO_WIDTH), "render_denoised: empty tile"),
    (lambda r: r.render_pixels(P, np.arange(N), 0, 1, sums=np.zeros((N, 3), F32)), "render_pixels: sums must be a contiguous float64 array of shape (5, 3)"),
    (lambda r: r.render_pixels(P, np.arange(N), 0, 1, sums=np.zeros((N + 1, 3))), "render_pixels: sums must be a contiguous float64 array of shape (5, 3)"),
    (lambda r: r.render_pixels(P, np.arange(N), 0, 1, sumsq=np.zeros((3, N)).T), "render_pixels: sumsq must be a contiguous float64 array of shape (5, 3)"),
    (lambda r: r.render_pixels(P, np.arange(N), 0, 1, sumsq=[[0.0] * 3] * N), "render_pixels: sumsq must be a contiguous float64 array of shape (5, 3)"),
    (lambda r: r.render_rays(P, ORG, DIRS[:4]), "render_rays: org and dir must both be float32 arrays of shape (S, n, 3)"),
    (lambda r: r.render_rays(P, np.zeros((N, 2), F32), np.zeros((N, 2), F32)), "render_rays: org and dir must both be float32 arrays of shape (S, n, 3)"),
    (lambda r: r.render_rays(P, ORG, DIRS, streams=np.arange(N + 1)), "render_rays: streams must hold 5 ids"),
    (lambda r: r.render_rays(P, ORG, DIRS, sums=np.zeros((N, 3), F32)), "render_pixels: sums must be a contiguous float64 array of shape (5, 3)"),
    (lambda r: r.render_aov_rays(P, ORG, DIRS[:4]), "render_aov_rays: org and dir must both be float32 arrays of shape (S, n, 3)"),
    (lambda r: r.render_aov_rays(P, ORG, DIRS, sums={"colour": None}), "render_aov_rays: sums must be a dict with the keys albedo, normal, depth"),
    (lambda r: r.render_aov_rays(P, ORG, DIRS, sums={"depth": None}), "render_aov_rays: at least one of albedo, normal, depth is needed"),
    (lambda r: r.render_aov_rays(P, ORG, DIRS, sums={"depth": np.zeros((N, 1))}), "render_aov_rays: depth must be a contiguous float64 array of shape (5,)"),
    (lambda r: r.trace_closest(ORG, DIRS[:4]), "trace_closest: org/dir length mismatch"),
    (lambda r: r.trace_closest(ORG, DIRS, t_max=np.zeros(N + 1)), "trace_closest: t_max must hold one bound per ray"),
    (lambda r: r.trace_occluded(ORG, DIRS[:4]), "trace_occluded: org/dir length mismatch"),
    (lambda r: r.trace_occluded(ORG, DIRS, t_max=np.zeros(N - 1)), "trace_occluded: t_max must hold one bound per ray"),
    (lambda r: r.trace_points(ORG, DIRS[:4], np.zeros((2, 3, 3))), "trace_points: org/dir length mismatch"),
    (lambda r: r.trace_points(ORG, DIRS, np.zeros((2, 9))), "trace_points: tri_v_other must be a float32 array of shape (n_tris, 3, 3)"),
    (lambda r: r.update_geometry(np.zeros((2, 9))), "update_geometry: tri_v must be a float32 array of shape (n, 3, 3)"),
    (lambda r: r.update_geometry(np.zeros((2, 3, 3)), tri_vn=np.zeros((3, 3, 3))), "update_geometry: tri_vn must have tri_v's shape"),
]


@pytest.mark.parametrize("row", range(len(HOST_REFUSALS)))
def test_host_refusals(row):
    call, message = HOST_REFUSALS[row]
    _refused(call, message, _renderer())


# The image of 2^31 pixels: every entry that keeps pixels in int32 tensors refuses it, after the empty tile and before it needs the device.
IMAGE_REFUSALS = [
    (lambda r: r.render_adaptive(BIG, 0.1, 1, 2, 1, on_device=True), "render_adaptive: on_device needs width * height < 2^31 (int32 pixel tensors)"),
    (lambda r: r.render_camera(NO_WIDTH, CAM), "render_camera: empty tile"),
    (lambda r: r.render_camera(NO_ROWS, CAM), "render_camera: empty tile"),
    (lambda r: r.render_camera(BIG, CAM), "render_camera: needs width * height < 2^31 (int32 pixel tensors)"),
    (lambda r: r.render_camera_aov(NO_WIDTH, CAM), "render_camera_aov: empty tile"),
    (lambda r: r.render_camera_aov(BIG, CAM), "render_camera_aov: needs width * height < 2^31 (int32 pixel tensors)"),
    (lambda r: r.render_camera_denoised(NO_WIDTH, CAM), "render_camera_denoised: empty tile"),
    (lambda r: r.render_camera_denoised(BIG, CAM), "render_camera_denoised: needs width * height < 2^31 (int32 pixel tensors)"),
]


@pytest.mark.parametrize("row", range(len(IMAGE_REFUSALS)))
def test_image_refusals(row):
    pytest.importorskip("torch")
    call, message = IMAGE_REFUSALS[row]
    _refused(call, message, _renderer())


def _t(*shape, **kw):
    return _tensor(shape, **kw)


ROWS, TW = 36, 64
RGB, ONE = ROWS * TW * 3, ROWS * TW  # 6912, 2304: what render_into / render_aov_into need of a tensor, at least


def _closest(r, **kw):
    a = dict(org=_t(N, 3), direction=_t(N, 3), t=_t(N), tri=_t(N, dtype="int32"), uv=_t(N, 2), t_max=_t(N))
    a.update(kw)
    return r.trace_closest_into(a.pop("org"), a.pop("direction"), a.pop("t"), a.pop("tri"), **a)


def _occluded(r, **kw):
    a = dict(org=_t(N, 3), direction=_t(N, 3), occluded=_t(N, dtype="uint8"), t_max=None)
    a.update(kw)
    return r.trace_occluded_into(a.pop("org"), a.pop("direction"), a.pop("occluded"), **a)


def _points(r, **kw):
    a = dict(org=_t(N, 3), dir=_t(N, 3), tri_v_other=_t(2, 3, 3), point=_t(N, 3))
    a.update(kw)
    return r.trace_points_into(**a)


def _rays(r, **kw):
    a = dict(org=_t(2, N, 3), dir=_t(2, N, 3), sums=_t(N, 3, dtype="float64"), sumsq=_t(N, 3, dtype="float64"), streams=_t(N, dtype="int32"))
    a.update(kw)
    return r.render_rays_into(P, **a)


def _aov_rays(r, **kw):
    a = dict(org=_t(2, N, 3), dir=_t(2, N, 3), albedo=_t(N, 3, dtype="float64"), normal=None, depth=_t(N, dtype="float64"))
    a.update(kw)
    return r.render_aov_rays_into(P, **a)


def _pixels(r, **kw):
    a = dict(pixels=_t(N, dtype="int32"), sums=_t(N, 3, dtype="float64"), sumsq=_t(N, 3, dtype="float64"))
    a.update(kw)
    return r.render_pixels(P, a.pop("pixels"), 0, 1, **a)


CLOSEST = "trace_closest_into: {} must be a contiguous {} tensor on cuda:0 with {} elements"
DEVICE_REFUSALS = [
    # trt_trace_closest_device: exactly n, 2 n or 3 n elements each
    (lambda r: _closest(r, org=ORG), "trace_closest_into: org must be a float32 tensor of shape (n, 3)"),
    (lambda r: _closest(r, org=_t(N, 4)), "trace_closest_into: org must be a float32 tensor of shape (n, 3)"),
    (lambda r: _closest(r, org=_t(N, 3, dtype="float64")), CLOSEST.format("org", "float32", 15)),
    (lambda r: _closest(r, org=_t(N, 3, device=("cuda", 1))), CLOSEST.format("org", "float32", 15)),
    (lambda r: _closest(r, org=_t(N, 3, device=("cpu",))), CLOSEST.format("org", "float32", 15)),
    (lambda r: _closest(r, direction=_t(16)), CLOSEST.format("direction", "float32", 15)),
    (lambda r: _closest(r, direction=_t(14)), CLOSEST.format("direction", "float32", 15)),
    (lambda r: _closest(r, direction=DIRS), CLOSEST.format("direction", "float32", 15)),
    (lambda r: _closest(r, t_max=_t(N + 1)), CLOSEST.format("t_max", "float32", 5)),
    (lambda r: _closest(r, t=_t(N, contiguous=False)), CLOSEST.format("t", "float32", 5)),
    (lambda r: _closest(r, tri=_t(N)), CLOSEST.format("tri", "int32", 5)),
    (lambda r: _closest(r, uv=_t(N, 3)), CLOSEST.format("uv", "float32", 10)),
    (lambda r: _closest(r, t=None), "trace_closest_into: t and tri are needed"),
    (lambda r: _closest(r, tri=None, uv=None), "trace_closest_into: t and tri are needed"),
    (lambda r: _closest(r, t=None, uv=_t(N)), CLOSEST.format("uv", "float32", 10)),  # the tensors given are checked before the absent ones are missed
    # trt_trace_occluded_device
    (lambda r: _occluded(r, org=_t(3, N)), "trace_occluded_into: org must be a float32 tensor of shape (n, 3)"),
    (lambda r: _occluded(r, occluded=_t(N, dtype="int32")), "trace_occluded_into: occluded must be a contiguous uint8 or bool tensor on cuda:0 with 5 elements"),
    (lambda r: _occluded(r, occluded=_t(N + 1, dtype="bool")), "trace_occluded_into: occluded must be a contiguous uint8 or bool tensor on cuda:0 with 5 elements"),
    (lambda r: _occluded(r, t_max=_t(N - 1)), "trace_occluded_into: t_max must be a contiguous float32 tensor on cuda:0 with 5 elements"),
    (lambda r: _occluded(r, occluded=None), "trace_occluded_into: occluded is needed"),
    # trt_trace_points_device
    (lambda r: _points(r, org=_t(N)), "trace_points_into: org must be a float32 tensor of shape (n, 3)"),
    (lambda r: _points(r, tri_v_other=_t(2, 9)), "trace_points_into: tri_v_other must be a float32 tensor of shape (n_tris, 3, 3)"),
    (lambda r: _points(r, tri_v_other=np.zeros((2, 3, 3), F32)), "trace_points_into: tri_v_other must be a float32 tensor of shape (n_tris, 3, 3)"),
    (lambda r: _points(r, tri_v_other=_t(2, 3, 3, dtype="float64")), "trace_points_into: tri_v_other must be a contiguous float32 tensor on cuda:0 with 18 elements"),
    (lambda r: _points(r, point=_t(N, 4)), "trace_points_into: point must be a contiguous float32 tensor on cuda:0 with 15 elements"),
    (lambda r: _points(r, point=None), "trace_points_into: org, dir, tri_v_other and point are needed"),
    (lambda r: _points(r, dir=None), "trace_points_into: org, dir, tri_v_other and point are needed"),
    # trt_render_rays_device
    (lambda r: _rays(r, org=_t(N, 3)), "render_rays_into: org must be a float32 tensor of shape (S, n, 3)"),
    (lambda r: _rays(r, org=np.zeros((2, N, 3), F32)), "render_rays_into: org must be a float32 tensor of shape (S, n, 3)"),
    (lambda r: _rays(r, dir=_t(1, N, 3)), "render_rays_into: dir must be a contiguous float32 tensor on cuda:0 with 30 elements"),
    (lambda r: _rays(r, dir=_t(31)), "render_rays_into: dir must be a contiguous float32 tensor on cuda:0 with 30 elements"),
    (lambda r: _rays(r, streams=_t(N, dtype="int64")), "render_rays_into: streams must be a contiguous int32 or uint32 tensor on cuda:0 with 5 elements"),
    (lambda r: _rays(r, sums=_t(16, dtype="float64")), "render_rays_into: sums must be a contiguous float64 tensor on cuda:0 with 15 elements"),
    (lambda r: _rays(r, sums=_t(N, 3)), "render_rays_into: sums must be a contiguous float64 tensor on cuda:0 with 15 elements"),
    (lambda r: _rays(r, sumsq=_t(14, dtype="float64")), "render_rays_into: sumsq must be a contiguous float64 tensor on cuda:0 with 15 elements"),
    (lambda r: _rays(r, sums=None), "render_rays_into: dir and sums are needed"),
    (lambda r: _rays(r, dir=None), "render_rays_into: dir and sums are needed"),
    # trt_aov_rays_device
    (lambda r: _aov_rays(r, org=_t(N, 3)), "render_aov_rays_into: org must be a float32 tensor of shape (S, n, 3)"),
    (lambda r: _aov_rays(r, org=_t(N, 3), albedo=None, depth=None), "render_aov_rays_into: org must be a float32 tensor of shape (S, n, 3)"),
    (lambda r: _aov_rays(r, albedo=None, depth=None), "render_aov_rays_into: at least one of albedo, normal, depth is needed"),
    (lambda r: _aov_rays(r, dir=_t(2, N, 3, contiguous=False)), "render_aov_rays_into: dir must be a contiguous float32 tensor on cuda:0 with 30 elements"),
    (lambda r: _aov_rays(r, albedo=_t(N, 3)), "render_aov_rays_into: albedo must be a contiguous float64 tensor on cuda:0 with 15 elements"),
    (lambda r: _aov_rays(r, normal=_t(N, dtype="float64")), "render_aov_rays_into: normal must be a contiguous float64 tensor on cuda:0 with 15 elements"),
    (lambda r: _aov_rays(r, depth=_t(N + 1, dtype="float64")), "render_aov_rays_into: depth must be a contiguous float64 tensor on cuda:0 with 5 elements"),
    (lambda r: _aov_rays(r, dir=None), "render_aov_rays_into: dir is needed"),
    # trt_update_geometry_device
    (lambda r: r.update_geometry_from(_t(2, 9)), "update_geometry_from: tri_v must be a float32 tensor of shape (n, 3, 3)"),
    (lambda r: r.update_geometry_from(np.zeros((2, 3, 3), F32)), "update_geometry_from: tri_v must be a float32 tensor of shape (n, 3, 3)"),
    (lambda r: r.update_geometry_from(_t(2, 3, 3, device=("cuda", 1))), "update_geometry_from: tri_v must be a contiguous float32 tensor on cuda:0 with 18 elements"),
    (lambda r: r.update_geometry_from(_t(2, 3, 3), tri_vn=_t(3, 3, 3)), "update_geometry_from: tri_vn must be a contiguous float32 tensor on cuda:0 with 18 elements"),
    # trt_render_pixels_device: shapes, not element counts
    (lambda r: _pixels(r, pixels=_t(N, dtype="int64")), "render_pixels: pixels must be a contiguous 1-D int32 / uint32 tensor on cuda:0"),
    (lambda r: _pixels(r, pixels=_t(N, 1, dtype="int32")), "render_pixels: pixels must be a contiguous 1-D int32 / uint32 tensor on cuda:0"),
    (lambda r: _pixels(r, pixels=_t(N, dtype="int32", device=("cuda", 1))), "render_pixels: pixels must be a contiguous 1-D int32 / uint32 tensor on cuda:0"),
    (lambda r: _pixels(r, pixels=_t(N, dtype="int32", device=("cpu",))), "render_pixels: pixels must be a contiguous 1-D int32 / uint32 tensor on cuda:0"),
    (lambda r: _pixels(r, pixels=_t(N, dtype="int32", contiguous=False)), "render_pixels: pixels must be a contiguous 1-D int32 / uint32 tensor on cuda:0"),
    (lambda r: _pixels(r, sums=_t(3 * N, dtype="float64")), "render_pixels: sums must be a contiguous float64 tensor of shape (5, 3) on cuda:0"),
    (lambda r: _pixels(r, sums=_t(N, 3)), "render_pixels: sums must be a contiguous float64 tensor of shape (5, 3) on cuda:0"),
    (lambda r: _pixels(r, sums=_t(N, 3, dtype="float64", device=("cuda", 1))), "render_pixels: sums must be a contiguous float64 tensor of shape (5, 3) on cuda:0"),
    (lambda r: _pixels(r, sumsq=_t(3, N, dtype="float64")), "render_pixels: sumsq must be a contiguous float64 tensor of shape (5, 3) on cuda:0"),
    (lambda r: _pixels(r, sumsq=_t(N, 3, dtype="float64", contiguous=False)), "render_pixels: sumsq must be a contiguous float64 tensor of shape (5, 3) on cuda:0"),
    # trt_render_aov_device: at least rows * tile_w * 3 (depth: rows * tile_w) elements
    (lambda r: r.render_aov_into(P, albedo=_t(RGB - 1)), "render_aov_into: albedo must be a contiguous float32 tensor on cuda:0 with 6912 elements"),
    (lambda r: r.render_aov_into(P, albedo=np.zeros(RGB, F32)), "render_aov_into: albedo must be a contiguous float32 tensor on cuda:0 with 6912 elements"),
    (lambda r: r.render_aov_into(P, normal=_t(RGB, dtype="float64")), "render_aov_into: normal must be a contiguous float32 tensor on cuda:0 with 6912 elements"),
    (lambda r: r.render_aov_into(P, normal=_t(RGB, device=("cuda", 1))), "render_aov_into: normal must be a contiguous float32 tensor on cuda:0 with 6912 elements"),
    (lambda r: r.render_aov_into(P, normal=_t(RGB, device=("cpu",))), "render_aov_into: normal must be a contiguous float32 tensor on cuda:0 with 6912 elements"),
    (lambda r: r.render_aov_into(P, albedo=_t(RGB), depth=_t(ONE - 1)), "render_aov_into: depth must be a contiguous float32 tensor on cuda:0 with 2304 elements"),
    (lambda r: r.render_aov_into(P, depth=_t(ROWS, TW, contiguous=False)), "render_aov_into: depth must be a contiguous float32 tensor on cuda:0 with 2304 elements"),
    # trt_render_device: at least rows * tile_w * 3 elements
    (lambda r: r.render_into(P, _t(RGB - 1)), "render_into: need a contiguous float32 device tensor with rows*tile_w*3 elements"),
    (lambda r: r.render_into(P, _t(RGB, dtype="float64")), "render_into: need a contiguous float32 device tensor with rows*tile_w*3 elements"),
    (lambda r: r.render_into(P, _t(RGB, device=("cpu",))), "render_into: need a contiguous float32 device tensor with rows*tile_w*3 elements"),
    (lambda r: r.render_into(P, _t(RGB, contiguous=False)), "render_into: need a contiguous float32 device tensor with rows*tile_w*3 elements"),
]


@pytest.mark.parametrize("row", range(len(DEVICE_REFUSALS)))
def test_device_refusals(row):
    pytest.importorskip("torch")
    call, message = DEVICE_REFUSALS[row]
    _refused(call, message, _renderer())


def test_group_refusals():
    pytest.importorskip("torch")
    message = "render_into: need a contiguous float32 device tensor with tile rows * tile_w * 3 elements"
    for t in (_t(RGB - 1), _t(RGB, dtype="int32"), _t(RGB, device=("cpu",)), _t(RGB, contiguous=False)):
        _refused(lambda g: g.render_into(P, t), message, _group())


# The other side of each rule: these reach the entry named.  ("exactly" entries with every tensor at its size; "at least" entries with
# the exact size and with one element more; an empty tile, which render_into leaves to the library.)
DEVICE_ACCEPTED = [
    (lambda r: _closest(r), "trt_trace_closest_device"),
    (lambda r: _closest(r, uv=None, t_max=None), "trt_trace_closest_device"),
    (lambda r: _closest(r, org=_t(N, 3, device=("cuda",))), "trt_trace_closest_device"),  # a device without an index is not compared
    (lambda r: _occluded(r), "trt_trace_occluded_device"),
    (lambda r: _occluded(r, occluded=_t(N, dtype="bool"), t_max=_t(N)), "trt_trace_occluded_device"),
    (lambda r: _points(r), "trt_trace_points_device"),
    (lambda r: _rays(r), "trt_render_rays_device"),
    (lambda r: _rays(r, sumsq=None, streams=None), "trt_render_rays_device"),
    (lambda r: _rays(r, streams=_t(N, dtype="uint32")), "trt_render_rays_device"),
    (lambda r: _aov_rays(r), "trt_aov_rays_device"),
    (lambda r: _aov_rays(r, albedo=None, normal=_t(N, 3, dtype="float64"), depth=None), "trt_aov_rays_device"),
    (lambda r: r.update_geometry_from(_t(2, 3, 3)), "trt_update_geometry_device"),
    (lambda r: r.update_geometry_from(_t(2, 3, 3), tri_vn=_t(2, 3, 3)), "trt_update_geometry_device"),
    (lambda r: r.render_aov_into(P, albedo=_t(RGB), normal=_t(RGB + 1), depth=_t(ONE)), "trt_render_aov_device"),
    (lambda r: r.render_aov_into(P, depth=_t(ONE + 1)), "trt_render_aov_device"),
    (lambda r: r.render_into(P, _t(RGB)), "trt_render_device"),
    (lambda r: r.render_into(P, _t(RGB + 1)), "trt_render_device"),
    (lambda r: r.render_into(NO_WIDTH, _t(1)), "trt_render_device"),
]


@pytest.mark.parametrize("row", range(len(DEVICE_ACCEPTED)))
def test_device_accepted(row):
    pytest.importorskip("torch")
    call, entry = DEVICE_ACCEPTED[row]
    r = _renderer(rc=0)
    assert isinstance(call(r), T.Stats)
    assert r._lib.calls == [entry]


def test_group_accepted():
    pytest.importorskip("torch")
    for t in (_t(RGB), _t(RGB + 1)):
        g = _group(rc=0)
        st, gather_ms = g.render_into(P, t)
        assert isinstance(st, T.Stats) and gather_ms == 0.0 and g._lib.calls == ["trt_group_render_device"]
    g = _group(rc=0)
    image, st, gather_ms = g.render(P)
    assert image.shape == (ROWS, TW, 3) and image.dtype == F32 and g._lib.calls == ["trt_group_render"]


# An entry that fails: its name, its code and the library's words.
HOST_FAILURES = [
    (lambda r: r.render(P), "trt_render"),
    (lambda r: r.render_samples(P, 0, 1), "trt_render_samples"),
    (lambda r: r.render_pixels(P, np.arange(N), 0, 1), "trt_render_pixels"),
    (lambda r: r.render_aov(P), "trt_render_aov"),
    (lambda r: r.render_rays(P, ORG, DIRS), "trt_render_rays"),
    (lambda r: r.render_aov_rays(P, ORG, DIRS), "trt_aov_rays"),
    (lambda r: r.trace_closest(ORG, DIRS), "trt_trace_closest"),
    (lambda r: r.trace_closest(ORG, DIRS, t_max=np.ones(N)), "trt_trace_closest_range"),
    (lambda r: r.trace_occluded(ORG, DIRS), "trt_trace_occluded"),
    (lambda r: r.trace_points(ORG, DIRS, np.zeros((2, 3, 3))), "trt_trace_points"),
    (lambda r: r.update_geometry(np.zeros((2, 3, 3))), "trt_update_geometry"),
]


@pytest.mark.parametrize("row", range(len(HOST_FAILURES)))
def test_host_entry_failure(row):
    call, entry = HOST_FAILURES[row]
    r = _renderer(rc=7)
    _refused(call, f"{entry} failed (7): stand-in", r)
    assert r._lib.calls == [entry]


@pytest.mark.parametrize("row", range(len(DEVICE_ACCEPTED)))
def test_device_entry_failure(row):
    pytest.importorskip("torch")
    call, entry = DEVICE_ACCEPTED[row]
    r = _renderer(rc=3)
    _refused(call, f"{entry} failed (3): stand-in", r)
    assert r._lib.calls == [entry]


def test_group_entry_failure():
    pytest.importorskip("torch")
    g = _group(rc=2)
    _refused(lambda g_: g_.render(P), "trt_group_render failed (2): stand-in", g)
    _refused(lambda g_: g_.render_into(P, _t(RGB)), "trt_group_render_device failed (2): stand-in", g)


def test_image_space_entry_failure():
    """_call_hip, the helper of the image-space passes, says the same of the real library: a refusal made on the host, no device needed."""
    with pytest.raises(T.TrtError) as e:
        T.denoise(np.zeros((4, 4, 3), F32), np.zeros((4, 4), F32), np.zeros((4, 4, 3), F32), np.zeros((4, 4, 3), F32), np.zeros((4, 4), F32), iterations=11)
    assert str(e.value) == "trt_denoise failed (1): trt_denoise: iterations must be 0..10"
