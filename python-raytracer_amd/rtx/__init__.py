"""rtx — MI355X-native drop-in for the render path of SpacewaIker/python-raytracer.

Host API (mirrors the reference's provided/*.py): ``load_scene`` (scene_parser.py),
``Scene.render`` (scene.py), the CLI in ``rtx.main`` (main.py) and ``rtx.glue`` (glue.py).
The per-pixel render loop and the intersectors run as HIP kernels in librtx.so.
"""
from .scene import (AOV_NAMES, ID_NAMES, OCCLUSION_NAMES, RESOLVED_NAMES, Scene, cosine_directions, frame_windows,  # noqa: F401
                    id_matte, light_group_table, panorama_rays, split_rows, strip_columns)
from .scene_parser import load_scene  # noqa: F401
from .io import load_bundled_scene, save_png, to_png_array  # noqa: F401
from ._native import get_option, option_names, set_option  # noqa: F401

__all__ = ["Scene", "load_scene", "load_bundled_scene", "save_png", "to_png_array", "split_rows", "strip_columns",
           "set_option", "get_option", "option_names", "frame_windows", "AOV_NAMES", "panorama_rays",
           "OCCLUSION_NAMES", "cosine_directions", "RESOLVED_NAMES", "ID_NAMES", "id_matte", "light_group_table"]
