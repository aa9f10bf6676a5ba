"""Constructed cameras and scenes (reference JSON schema) for the tile-class tests: one ground
plane, a few spheres, one sample per pixel (the cameras that get class records)."""
import copy

MAT = {"name": "m", "ID": 0, "type": "diffuse", "diffuse": [0.8, 0.7, 0.6], "specular": [0.5, 0.5, 0.5], "hardness": 16}
GROUND = {"name": "ground", "type": "plane", "normal": [0.0, 1.0, 0.0], "position": [0.0, -1.0, 0.0], "materials": [0]}
WALL = {"name": "wall", "type": "plane", "normal": [0.0, 0.0, 1.0], "position": [0.0, 0.0, -9.0], "materials": [0]}
POINT = {"name": "p", "type": "point", "position": [4.0, 9.0, 5.0], "colour": [1, 1, 1], "power": 0.8}
SUN = {"name": "d", "type": "directional", "direction": [-0.4, -1.0, -0.3], "colour": [1, 1, 1], "power": 0.7}
CAM, LOOK = [0.0, 2.0, 8.0], [0.0, 0.0, 0.0]


def sphere(pos, rad, name="s", **kw):
    return dict({"name": name, "type": "sphere", "radius": rad, "position": list(pos), "materials": [0]}, **kw)


def scene_dict(cam, look, objs, lights=(POINT,), res=(72, 40), fov=50.0, planes=(GROUND,), motion=None):
    d = {"resolution": list(res), "AA": {"jitter": False, "samples": 1}, "ambient": [0.1, 0.1, 0.1],
         "camera": {"position": list(cam), "lookAt": list(look), "up": [0.0, 1.0, 0.0], "fov": fov},
         "materials": [copy.deepcopy(MAT)], "objects": [copy.deepcopy(p) for p in planes] + [copy.deepcopy(o) for o in objs],
         "lights": [copy.deepcopy(lt) for lt in lights]}
    if motion:
        d["motion"] = dict(motion)
    return d


# (a scene needs an occluder to get bins: one in front of the camera, far outside its view)
ASIDE_HIGH, ASIDE_DEEP, ASIDE_LOW = [sphere([80.0, 30.0, 0.0], 0.5)], [sphere([80.0, -30.0, 0.0], 0.5)], [sphere([80.0, -0.5, -20.0], 0.5)]
EDGE_AT = [0.9, 0.2, 0.0]  # a sphere whose padded silhouette crosses a tile border between radius 0.60 and 0.71
ONE_TIME = {"time": 0.7, "samples": 1, "final": 0}  # (one motion time; a test sets vc.motion_times for another)


def constructed(res=(72, 40)):
    """name -> scene: the cameras of tests/test_tile_class.py, for the GPU frames."""
    return {
        "sky_above": scene_dict([0.0, 2.0, 8.0], [0.0, 9.0, 6.0], ASIDE_HIGH, res=res),
        "sky_below": scene_dict([0.0, -3.0, 8.0], [0.0, -9.0, 6.0], ASIDE_DEEP, res=res),
        "plane_from_below": scene_dict([0.0, -3.0, 8.0], [0.0, 9.0, 6.0], ASIDE_HIGH, res=res),
        "horizon": scene_dict([0.0, 1.0, 8.0], [0.0, 1.0, 0.0], ASIDE_LOW, res=res),
        "sphere_at_edge": scene_dict(CAM, LOOK, [sphere(EDGE_AT, 0.66)], res=res),
        "plane_self_inside": scene_dict(CAM, [0.0, 0.0, -4.0], ASIDE_LOW, lights=[dict(POINT, position=[0.0, 1.0, 0.0])], res=res),
        "plane_self_none": scene_dict(CAM, [0.0, 0.0, -4.0], ASIDE_LOW, lights=[dict(POINT, position=[0.0, -0.9, 0.0])], res=res),
        "two_planes": scene_dict(CAM, LOOK, [sphere([0.0, 0.0, 0.0], 1.0)], planes=(GROUND, WALL), res=res),
        "directional": scene_dict(CAM, LOOK, [sphere([0.0, 0.0, 0.0], 1.0)], lights=[SUN, POINT], res=res),
        "seventeen": scene_dict(CAM, LOOK, [sphere([-4.0 + 0.5 * i, -0.8, 0.0], 0.2, name="s%d" % i) for i in range(17)], res=res),
        "moving": scene_dict(CAM, LOOK, [sphere([0.0, 0.0, 0.0], 1.0, speed=[0.5, 0.0, 0.2])], motion=ONE_TIME, res=res),
    }
