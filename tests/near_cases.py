"""A deterministic corpus for TRT_FLAG_NEAR_LIGHTS (tests/test_near_lights_cpu.py, tests/test_gpu_near_lights.py), written with scene_util.write_scene.

corridor(K): a diffuse floor 4K x 4 at y = 0 (x in [0, 4K], z in [-2, 2]) under K lamps of 0.5 x 0.5 that face down, at height 1 above x = 4k + 2, all of
the same radiance, each with a material of its own (a light is a material); the camera sees the whole floor.  Under a lamp's centre that lamp carries
about 300 times its neighbour's contribution (h^2 / d^4 with h = 1, d^2 = 17): where a vertex is decides which light matters, power does not.
The variants: two coincident lamps (the same vertices under two materials), black lamps (zero weight) interleaved by index, a lamp that is one
degenerate triangle of zero extent, and corridors of two and of three lamps."""
import math
import os
import tempfile

import scene_util as SU

RADIANCE = (20.0, 18.0, 15.0)
FOVY = 40.0
_dir = None
_scenes = {}


def _mtl(names):
    return SU.MTL_BASIC + "".join(f"newmtl {n}\nKd 0 0 0\nKs 0 0 0\nNs 1\nNi 1\n" for n in names)


def _write(d, name, K, lamps, w, h):
    """lamps: (material, x centre, half size or None for the degenerate triangle, radiance) per light, in light order."""
    v = ["v 0 0 -2", f"v {4 * K} 0 -2", f"v {4 * K} 0 2", "v 0 0 2"]
    faces = ["usemtl white", "f 1/1/1 4/1/1 3/1/1", "f 1/1/1 3/1/1 2/1/1"]
    vb = 5
    for mat, x, e, _ in lamps:
        faces.append(f"usemtl {mat}")
        if e is None:
            v += [f"v {x} 1 0"] * 3
            faces.append(f"f {vb}/1/2 {vb + 1}/1/2 {vb + 2}/1/2")
            vb += 3
        else:
            v += [f"v {x - e} 1 {-e}", f"v {x + e} 1 {-e}", f"v {x + e} 1 {e}", f"v {x - e} 1 {e}"]
            faces += [f"f {vb}/1/2 {vb + 1}/1/2 {vb + 2}/1/2", f"f {vb}/1/2 {vb + 2}/1/2 {vb + 3}/1/2"]
            vb += 4
    obj = "vt 0 0\nvn 0 1 0\nvn 0 -1 0\n" + "\n".join(v + faces) + "\n"
    # the camera: 60 degrees above the floor's long axis, at the distance from which the floor's length fills the image's width (and 5 % to spare)
    dist = 1.05 * 2 * K / ((w / h) * math.tan(math.radians(FOVY / 2)))
    SU.write_scene(d, name, obj, _mtl([m for m, _, _, _ in lamps]), lights=[(m, r) for m, _, _, r in lamps], w=w, h=h, fovy=FOVY,
                   eye=(2 * K, round(0.866 * dist, 3), round(0.5 * dist, 3)), lookat=(2 * K, 0, 0))


def _lamps(variant, K):
    lamps = [(f"lamp{k}", 4 * k + 2, 0.25, RADIANCE) for k in range(K)]
    if variant == "coincident":  # the lamp over x = 6 twice
        lamps.insert(2, ("twin", 6, 0.25, RADIANCE))
    elif variant == "black":     # every second light by index gives no light
        lamps = [(m, x, e, RADIANCE if k % 2 == 0 else (0.0, 0.0, 0.0)) for k, (m, x, e, _) in enumerate(lamps)]
    elif variant == "degenerate":  # light 1 is a point: no area, no weight
        lamps.insert(1, ("point", 4.0, None, RADIANCE))
    else:
        assert variant == "plain"
    return lamps


CASES = {"corridor2": ("plain", 2), "corridor3": ("plain", 3), "corridor16": ("plain", 16), "coincident": ("coincident", 4), "black": ("black", 6),
         "degenerate": ("degenerate", 4)}


def write_case(d, key, w, h):
    """Writes the files of the corpus scene `key` at w x h into the directory d (key.xml, key.obj, key.mtl)."""
    variant, K = CASES[key]
    _write(d, key, K, _lamps(variant, K), w, h)


def scene(key, w, h):
    """The corpus scene `key` at w x h, loaded once per (key, size) and kept."""
    global _dir
    k = (key, w, h)
    if k not in _scenes:
        if _dir is None:
            _dir = tempfile.TemporaryDirectory(prefix="near_cases_")
        d = os.path.join(_dir.name, f"{key}_{w}x{h}")
        os.makedirs(d, exist_ok=True)
        write_case(d, key, w, h)
        _scenes[k] = SU.load(d, key)
    return _scenes[k]


def corridor(K, w, h):
    key = f"corridor{K}"
    if key not in CASES:
        CASES[key] = ("plain", K)
    return scene(key, w, h)


def moved_lamps(s, dx=1.5, dy=0.25):
    """The vertices of scene s (Scene.arrays()["tri_v"]) with every emissive triangle moved by (dx, dy, 0): the lamps of a corridor slide along it."""
    import numpy as np
    f = s.flat.contents
    a = s.arrays()
    mats = {f.lights[i].mat for i in range(f.n_lights)}
    lamp = np.isin(a["tri_mat"], list(mats))
    v = a["tri_v"].copy()
    shape = v.shape
    v = v.reshape(len(lamp), 3, 3)
    v[lamp] += np.array([dx, dy, 0.0], np.float32)
    return v.reshape(shape).astype(np.float32)
