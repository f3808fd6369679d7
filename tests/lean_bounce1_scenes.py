"""Scenes for the lean bounce-1 hand-over of the virtual reorder (rt_render.hip: shade_kernel<.., SLIM>,
trace_kernel<.., VSLOT>, shade_rank_kernel), next to tests/slim_handover_scenes.py.

A ray that survives bounce 0 is handed over as one 16-B record {d, t0}; the bounce-1 trace recomputes its origin as
cam + t0 * primary_dir(ray), bounce 0's own expression, and writes back a 4-B hit index for every ray and the hit point
o + closest * d for the rays that hit, which the bounce-1 shading reads instead of computing it.

* far_cam: the camera stands 5000 units from the origin and looks, through a very narrow lens, into a small lit room
  around the origin whose near wall is missing.  t0 is about 5000 and the hit points are a few units large, so
  cam + t0 * d0 cancels and rounds in its last bits: any reassociation of it shows.  Rays beside the opening go to the
  sky at bounce 0, so dead slots stand between the survivors.
* b1_mixed: a floor, two low walls, a box and a mirror ball under a sky map.  At bounce 1 a good part of the rays
  hits and a good part leaves to the sky, in the same waves: the hit-only origin stores and loads are divergent.
* b1_spheres: a floor and a mirror wall (triangles) with diffuse balls on the floor, so that many bounce-1 rays end on
  a sphere, whose normal comes from the handed-over hit point.
"""
import os

import shade_scenes

IMAGE = (24, 16, 40, 6)
SKY_MAP = (16, 8)                   # one of shade_scenes.SKY_MAPS


def far_cam_scene():
    room = shade_scenes.ROOM.splitlines(True)[1:]           # without the wall at z = -2, towards the camera
    return ("material glow emit 0.5 0.2 0.1 diffuse 0.7 0.7 0.7\n"
            "material glow2 emit 0.0 0.1 0.4 diffuse 0.5 0.6 0.7\n"
            "material plain diffuse 0.6 0.6 0.6\n"
            "material lamp emit 2 2 2 diffuse 0 0 0 specular 0 0 0\n"
            "material ball diffuse 0.5 0.5 0.5 specular 0.9 0.8 0.7 metallicity 0.5 roughness 0.1\n"
            "sky 0.3 0.3 0.3\n" +
            "".join(room) % ("glow2", "plain", "glow", "plain", "glow2") +
            "quad lamp -0.5 1.95 -0.5  -0.5 1.95 0.5  0.5 1.95 0.5  0.5 1.95 -0.5\n"
            "sphere ball 0.7 -1.2 0.3 0.8\n"
            "camera position 0 0 -5000 forward 0 0 1 up 0 1 0 fov 0.06\n"
            "image %d %d %d %d 1\n" % IMAGE)


def b1_mixed_scene():
    return ("material grey diffuse 0.5 0.5 0.5\n"
            "material red diffuse 0.7 0.3 0.3\n"
            "material glow emit 0.3 0.2 0.1 diffuse 0.6 0.6 0.6\n"
            "material mirror metallicity 1\n"
            "sky_map %s\n"
            "quad grey -5 0 -5 -5 0 5 5 0 5 5 0 -5\n"
            # two low walls behind and to the right of the ball
            "quad red -5 0 3  5 0 3  5 2.5 3  -5 2.5 3\n"
            "quad glow 3 0 -5  3 0 3  3 2.5 3  3 2.5 -5\n"
            # a box on the floor, open below
            "quad red -3 0 -1  -1.5 0 -1  -1.5 1.5 -1  -3 1.5 -1\n"
            "quad red -3 0 0.5  -3 1.5 0.5  -1.5 1.5 0.5  -1.5 0 0.5\n"
            "quad red -3 0 -1  -3 1.5 -1  -3 1.5 0.5  -3 0 0.5\n"
            "quad red -1.5 0 -1  -1.5 0 0.5  -1.5 1.5 0.5  -1.5 1.5 -1\n"
            "quad glow -3 1.5 -1  -1.5 1.5 -1  -1.5 1.5 0.5  -3 1.5 0.5\n"
            "sphere mirror 0 1 0 1\n"
            "camera position 0 1.5 -4 forward 0 -0.1 1 up 0 1 0 fov 70\n"
            "image %d %d %d %d 1\n" % ((shade_scenes.pfm_name(*SKY_MAP),) + IMAGE))


def b1_spheres_scene():
    return ("material grey diffuse 0.5 0.5 0.5\n"
            "material mirror metallicity 1\n"
            "material ball diffuse 0.8 0.6 0.4\n"
            "material glowball emit 0.2 0.1 0.3 diffuse 0.6 0.7 0.8\n"
            "material glass ior 1.5\n"
            "sky 0.4 0.5 0.6\n"
            "quad grey -6 0 -6 -6 0 6 6 0 6 6 0 -6\n"
            "quad mirror -6 0 4  6 0 4  6 5 4  -6 5 4\n"
            "sphere ball -2.2 1 1 1\n"
            "sphere glowball 0 1.2 2 1.2\n"
            "sphere ball 2.3 1 0.8 1\n"
            "sphere glass 0.9 0.5 -0.8 0.5\n"
            "sphere glowball -1 0.4 -1 0.4\n"
            "camera position 0 2 -5 forward 0 -0.15 1 up 0 1 0 fov 65\n"
            "image %d %d %d %d 1\n" % IMAGE)


SCENES = {"far_cam": far_cam_scene, "b1_mixed": b1_mixed_scene, "b1_spheres": b1_spheres_scene}
NAMES = list(SCENES)


def write(dirpath):
    """Writes the scene files and b1_mixed's sky map into dirpath (their asset root); returns {name: path}."""
    shade_scenes.write_pfm(os.path.join(dirpath, shade_scenes.pfm_name(*SKY_MAP)), *SKY_MAP)
    out = {}
    for name, f in SCENES.items():
        out[name] = os.path.join(dirpath, name + ".scene")
        with open(out[name], "w") as fh:
            fh.write(f())
    return out
