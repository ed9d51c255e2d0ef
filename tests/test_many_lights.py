"""The synthetic many-light scene (Scene.named("lamps"), host/synth.cpp) and the oracle on it: no GPU needed."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import tinyraytracing_amd as T


def _lights(scene):
    f = scene.flat.contents
    return [(f.lights[i].mat, tuple(f.lights[i].radiance), f.lights[i].area, f.lights[i].tri_first, f.lights[i].tri_count) for i in range(f.n_lights)]


def _light_tris(scene):
    f = scene.flat.contents
    return C.string_at(f.light_tris, f.n_light_tris * C.sizeof(T._abi.LightTri))


@pytest.mark.parametrize("k", [8, 64, 300])
def test_lamps_scene_has_k_more_lights_and_is_deterministic(k):
    s = T.Scene.named("lamps", 64, 36, n=k)
    assert s.info["n_lights"] == k + 1  # the box's own light stays light 0
    lights = _lights(s)
    assert all(area > 0.0 for _, _, area, _, _ in lights)
    assert len({mat for mat, _, _, _, _ in lights}) == k + 1  # a material per lamp
    a0 = lights[0][2]
    assert any(area < a0 for _, _, area, _, _ in lights[1:]) and any(area > a0 for _, _, area, _, _ in lights[1:])  # both sides of Q3
    assert any(count > 2 for _, _, _, _, count in lights[1:])  # the CDF walks several triangles
    same = T.Scene.named("lamps", 64, 36, n=k)
    other = T.Scene.named("lamps", 64, 36, n=k, seed=12345)
    a, b, c = s.arrays(), same.arrays(), other.arrays()
    for key in ("tri_v", "tri_vn", "tri_vt", "tri_mat"):
        assert np.array_equal(a[key], b[key]), key
    assert _lights(same) == lights and _light_tris(same) == _light_tris(s)
    assert not np.array_equal(np.sort(a["tri_v"].ravel()), np.sort(c["tri_v"].ravel()))
    assert _lights(other) != lights
    for x in (same, other, s):
        x.close()


def test_lamps_light_cdf_is_filled_like_readobj():
    """Per light: the triangles' cum_area is the running total of their areas and ends at the light's area (scene.cpp)."""
    s = T.Scene.named("lamps", 64, 36, n=24)
    f = s.flat.contents
    for i in range(1, f.n_lights):
        L = f.lights[i]
        cum = [f.light_tris[L.tri_first + t].cum_area for t in range(L.tri_count)]
        assert all(b > a for a, b in zip(cum, cum[1:]))
        assert cum[-1] == pytest.approx(L.area, rel=1e-6)
        # facing down, under the ceiling of the box
        for t in range(L.tri_count):
            lt = f.light_tris[L.tri_first + t]
            assert all(lt.vn[k][1] == pytest.approx(-1.0) for k in range(3))
            assert all(0.0 < lt.v[k][1] < 548.8 for k in range(3))
    s.close()


def test_default_lamps_count_is_16():
    s = T.Scene.named("lamps", 32, 18)
    assert s.info["n_lights"] == 17
    s.close()


@pytest.mark.parametrize("k", [64, 300])
def test_oracle_samples_every_light_of_a_many_light_scene(k):
    """With TRT_FLAG_FIXED_NEE every light is sampled at every shaded vertex: more than 8 shadow rays per vertex."""
    s = T.Scene.named("lamps", 64, 36, n=k)
    p = T.make_params(64, 36, 2, 0x11A7, flags=T.TRT_FLAG_FIXED_NEE)
    img, st = O.render(s.flat, p)
    assert np.isfinite(img).all() and img.max() > 0.0
    assert st.rays_shadow > 8 * st.shaded_hits > 0
    s.close()
