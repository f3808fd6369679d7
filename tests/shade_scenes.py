"""Synthetic scene files that drive the shading paths no shipped scene reaches.

In every scene under assets/ (and in edge_scenes.py) a material with `emit` has black albedos, so a
ray receives at most one nonzero radiance term, in the step it dies: the renderer's acc[ray] / kAccFlag
read-modify-write (shade_kernel's shade_slot, the flag's trip through the reorder, the home-indexed
bounce-0 term of the fused replay) never runs with acc_holds set.  Here emitters also scatter.

* glow_room: a closed cube of glowing, diffusing quads: every hit adds a nonzero term and leaves the
  ray alive.
* glow_balls: the same with spheres only (the INLINE shade path), inside a glowing shell: no ray ever
  misses.
* glow_mixed: glowing and plain surfaces in the same waves, a few rays that reach the sky, and the
  points of `scatter` the shipped materials leave out: rough glass (sqrtf(1 - magsq(perp)) of a
  negative number), ior 1 and below, roughness 1 and 2 (normalise of a near-zero vector), an even
  metal/diffuse split, negative emission (a term that cancels what acc holds), subnormal emission.
* glow_dark: every framebuffer value is a sum of float32 subnormals.
* sky_WxH: a grey floor and a mirror ball under a small seeded, non-square environment map.  sky_color
  keeps the reference's row stride of env_h (scene.cu:389-391), which stays inside the map only for
  W >= H; tall maps are refused at load and by check_scene.
"""
import contextlib
import os

import numpy as np

ROOM = ("quad %s -2 -2 -2  -2 2 -2  2 2 -2  2 -2 -2\n"      # z = -2
        "quad %s -2 -2 2  2 -2 2  2 2 2  -2 2 2\n"          # z = 2
        "quad %s -2 -2 -2  -2 -2 2  -2 2 2  -2 2 -2\n"      # x = -2
        "quad %s 2 -2 -2  2 2 -2  2 2 2  2 -2 2\n"          # x = 2
        "quad %s -2 -2 -2  2 -2 -2  2 -2 2  -2 -2 2\n"      # y = -2
        "quad %s -2 2 -2  -2 2 2  2 2 2  2 2 -2\n")         # y = 2

ROOM_CAMERA = "camera position 0 0 -1.5 forward 0 0 1 up 0 1 0 fov 80\n"

GLOW_IMAGE = (24, 16, 40, 6)        # two passes of 7680 rays
SKY_MAPS = ((16, 8), (5, 3), (7, 1))


def glow_room_scene():
    return ("material glow emit 0.5 0.2 0.1 diffuse 0.7 0.7 0.7\n"
            "material glow2 emit 0.0 0.1 0.4 diffuse 0.5 0.6 0.7\n"
            "sky 0.3 0.3 0.3\n" +
            ROOM % ("glow", "glow2", "glow", "glow2", "glow", "glow2") +
            ROOM_CAMERA +
            "image 24 16 40 6 1\n")


def glow_balls_scene():
    return ("material shell emit 0.2 0.3 0.5 diffuse 0.8 0.7 0.6\n"
            "material ball emit 0.6 0.1 0.1 diffuse 0.5 0.5 0.5 specular 0.9 0.8 0.7 metallicity 0.5 roughness 0.1\n"
            "material glass emit 0.05 0.05 0.05 ior 1.5\n"
            "sky 1 1 1\n"
            "sphere shell 0 0 0 50\n"
            "sphere ball 3 -1 6 2.5\n"
            "sphere glass -3 0 5 2\n"
            "sphere ball 0 4 9 1.5\n"
            "camera position 0 0 -8 forward 0 0 1 up 0 1 0 fov 60\n"
            "image 24 16 40 6 1\n")


def glow_mixed_scene():
    return ("material glow emit 0.5 0.2 0.1 diffuse 0.7 0.7 0.7\n"
            "material glowmetal emit 0.1 0.1 0.3 specular 0.9 0.9 0.9 metallicity 1 roughness 0.2\n"
            "material half emit 0.05 0.3 0.05 diffuse 0.6 0.6 0.6 specular 0.8 0.8 0.8 metallicity 0.5 roughness 1\n"
            "material glowglass emit 0.02 0.02 0.02 ior 1.5 roughness 0.3\n"
            "material dim emit 1e-42 0 0 diffuse 0.9 0.9 0.9\n"
            # no emission: its rays carry no flag next to flagged ones in the same wave
            "material plain diffuse 0.6 0.6 0.6\n"
            # a term that takes away from what acc holds
            "material cancel emit -0.5 0.2 0.1 diffuse 0.7 0.7 0.7\n"
            "material unity emit 0.02 0.03 0.04 ior 1\n"
            "material under emit 0.03 0.02 0.01 ior 0.8 roughness 0.1\n"
            "material fuzz emit 0.1 0.05 0.2 diffuse 0.6 0.5 0.4 specular 0.7 0.8 0.9 metallicity 0.5 roughness 2\n"
            "sky 0.3 0.3 0.3\n" +
            ROOM % ("glow", "glowmetal", "half", "glow", "dim", "half") +
            # two half walls just inside the room: the lower half at x = -1.9, the upper half at x = 1.9
            "quad plain -1.9 -2 -2  -1.9 -2 2  -1.9 0 2  -1.9 0 -2\n"
            "quad cancel 1.9 0 -2  1.9 2 -2  1.9 2 2  1.9 0 2\n"
            "sphere glowglass 0.5 -0.5 0.5 0.8\n"
            "sphere unity -1 -1.2 0.8 0.5\n"
            "sphere under -0.9 0.8 0.6 0.5\n"
            "sphere fuzz 1.1 1.0 1.0 0.5\n" +
            ROOM_CAMERA +
            "image 24 16 40 6 1\n")


def glow_dark_scene():
    return ("material faint emit 1e-40 3e-41 1e-42 diffuse 0.9 0.9 0.9\n"
            "sky 0 0 0\n" +
            ROOM % (("faint",) * 6) +
            ROOM_CAMERA +
            "image 16 12 20 4 1\n")


def pfm_name(w, h):
    return "env_%dx%d.pfm" % (w, h)


def sky_scene(w, h):
    return ("material grey diffuse 0.5 0.5 0.5\n"
            "material mirror metallicity 1\n"
            "sky_map %s\n"
            "quad grey -5 0 -5 -5 0 5 5 0 5 5 0 -5\n"
            "sphere mirror 0 1 0 1\n"
            "camera position 0 1.5 -4 forward 0 -0.1 1 up 0 1 0 fov 70\n"
            "image 24 16 20 4 1\n" % pfm_name(w, h))


def write_pfm(path, w, h):
    """A w x h map of seeded values in [0, 4) in the raw layout load_pfm reads (tools/make_envmap.py:
    three header lines, then h rows of w RGB float32 texels, no flip).  Returns the texels (h, w, 3)."""
    img = (np.random.default_rng(3).random((h, w, 3)) * 4).astype(np.float32)
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h) + np.ascontiguousarray(img, dtype="<f4").tobytes())
    return img


GLOW = {"glow_room": glow_room_scene, "glow_balls": glow_balls_scene, "glow_mixed": glow_mixed_scene,
        "glow_dark": glow_dark_scene}
SKY = ["sky_%dx%d" % wh for wh in SKY_MAPS]
NAMES = list(GLOW) + SKY


def write(dirpath):
    """Writes the scene files and the sky maps into dirpath (the asset root of the sky_* scenes);
    returns {name: path}."""
    texts = {name: f() for name, f in GLOW.items()}
    for w, h in SKY_MAPS:
        write_pfm(os.path.join(dirpath, pfm_name(w, h)), w, h)
        texts["sky_%dx%d" % (w, h)] = sky_scene(w, h)
    out = {}
    for name, text in texts.items():
        out[name] = os.path.join(dirpath, name + ".scene")
        with open(out[name], "w") as f:
            f.write(text)
    return out


@contextlib.contextmanager
def swapped_env(scene):
    """Within the block, scene's rt_scene view has the map's width and height swapped (a caller-supplied
    view, patched as in test_bvh_deeper_than_the_stack_is_refused); the buffer keeps its w * h texels."""
    v = scene.view
    saved = (v.environment_map_width, v.environment_map_height)
    v.environment_map_width, v.environment_map_height = saved[1], saved[0]
    try:
        yield
    finally:
        v.environment_map_width, v.environment_map_height = saved
