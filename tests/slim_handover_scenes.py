"""A scene for the slim bounce-0 hand-over of the virtual reorder (rt_render.hip: shade_kernel<.., SLIM>,
shade_rank_kernel), next to tests/shade_scenes.py.

Bounce 0 hands a surviving ray over as {o, d}, the hit's material index and one bit (which albedo `scatter`
multiplied into the throughput); bounce 1 rebuilds T = 1 * albedo and the "acc holds radiance" flag
has_radiance(0 + emit * 1) from the material.  slim_mix puts, all in view of the camera and so hit at bounce 0:

* tinyalb / subspec: a float32 subnormal component in the diffuse and in the specular albedo (1 * x must keep it);
* negzero: emission -0 -0 -0 (no radiance: the flag must stay clear, acc[ray] was never written);
  neg: negative emission; sub: subnormal emission (both set the flag);
* half: an even metal / diffuse split with different albedos, on a wall and on a sphere (index < sphere_count);
* pane: a dielectric with different albedos for reflection and refraction, as two quads of opposite winding (front
  and back face towards the camera) and as a sphere;
* lamp: emits with black albedos, so its rays end at bounce 0 in the same waves and tiles as the survivors;
* plain: no emission, rays without the flag next to flagged ones.
"""
import os

import shade_scenes

IMAGE = (24, 16, 40, 6)

SUBNORMAL_DIFFUSE = "1e-40"         # tinyalb's diffuse.x
SUBNORMAL_SPECULAR = "3e-41"        # subspec's specular.x


def slim_mix_scene():
    return ("material tinyalb emit 0.2 0.1 0.3 diffuse %s 0.6 0.7\n" % SUBNORMAL_DIFFUSE +
            "material subspec emit 0.1 0.2 0.1 specular %s 0.9 0.8 metallicity 1 roughness 0.1\n" % SUBNORMAL_SPECULAR +
            "material negzero emit -0 -0 -0 diffuse 0.7 0.6 0.5\n"
            "material neg emit -0.5 0.2 0.1 diffuse 0.7 0.7 0.7\n"
            "material sub emit 1e-42 0 0 diffuse 0.9 0.9 0.9\n"
            "material half emit 0.05 0.3 0.05 diffuse 0.6 0.5 0.4 specular 0.8 0.9 0.7 metallicity 0.5 roughness 0.3\n"
            "material pane emit 0.02 0.02 0.02 diffuse 0.9 0.95 1.0 specular 0.8 0.85 0.9 ior 1.5\n"
            "material lamp emit 2 2 2 diffuse 0 0 0 specular 0 0 0\n"
            "material plain diffuse 0.6 0.6 0.6\n"
            "sky 0.3 0.3 0.3\n" +
            shade_scenes.ROOM % ("plain", "tinyalb", "negzero", "neg", "sub", "subspec") +
            # the lower half of the front wall, just inside the room
            "quad half -2 -2 1.95  2 -2 1.95  2 0 1.95  -2 0 1.95\n"
            # two panes of opposite winding between the camera and the front wall
            "quad pane -1.2 -0.6 0.5  -0.2 -0.6 0.5  -0.2 0.4 0.5  -1.2 0.4 0.5\n"
            "quad pane 0.2 0.4 0.5  1.2 0.4 0.5  1.2 -0.6 0.5  0.2 -0.6 0.5\n"
            "quad lamp -0.4 0.8 1.9  0.4 0.8 1.9  0.4 1.4 1.9  -0.4 1.4 1.9\n"
            "sphere half 1.2 1.0 1.0 0.5\n"
            "sphere pane -1.1 1.0 0.8 0.45\n"
            "sphere tinyalb 0 -1.2 0.9 0.4\n" +
            shade_scenes.ROOM_CAMERA +
            "image %d %d %d %d 1\n" % IMAGE)


def write(dirpath):
    """Writes slim_mix.scene into dirpath; returns {name: path}."""
    path = os.path.join(dirpath, "slim_mix.scene")
    with open(path, "w") as f:
        f.write(slim_mix_scene())
    return {"slim_mix": path}
