"""The camera plugins, configured on the host by the library (mtsgpu_make_camera*)."""
import ctypes as C

import numpy as np

from . import abi
from .binding import check, lib


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _look_at(origin, target, up):
    return [abi.ptr(_f(v), abi.f32p) for v in (origin, target, up)]


def struct_of(camera):
    """the abi.Camera of a camera object, or the abi.Camera itself"""
    return camera.c if hasattr(camera, "c") else camera


class PerspectiveCamera:
    """`perspective` camera plugin: lookAt toWorld transform, fov along the smaller side, pinhole."""

    def __init__(self, origin, target, up, fov, width, height, apertureRadius=0.0, focusDepth=None):
        self.c = abi.Camera()
        check(lib().mtsgpu_make_camera(*_look_at(origin, target, up), C.c_float(fov), int(width), int(height), C.byref(self.c)), "mtsgpu_make_camera")
        if apertureRadius > 0:                       # thin lens (camera.cpp:164-166, perspective.cpp:90-103)
            self.c.aperture_radius = apertureRadius
            self.c.focus_depth = self.c.far_clip if focusDepth is None else focusDepth

    @classmethod
    def cropped(cls, desc, film_width, film_height, crop):
        """the camera of `desc` behind a film with a crop window (film.cpp:33-41): crop = (offsetX, offsetY, width, height)"""
        c = desc.camera
        self = cls.__new__(cls)
        self.c = abi.Camera()
        check(lib().mtsgpu_make_camera_crop(*_look_at(c["origin"], c["target"], c["up"]), C.c_float(c["fov"]), int(film_width), int(film_height),
                                            *[int(v) for v in crop], C.byref(self.c)), "mtsgpu_make_camera_crop")
        return self

    @classmethod
    def for_description(cls, desc, width, height):
        c = desc.camera
        if "ortho_scale" in c:
            return OrthographicCamera(c["origin"], c["target"], c["up"], c["ortho_scale"], width, height)
        return cls(c["origin"], c["target"], c["up"], c["fov"], width, height,
                   apertureRadius=c.get("aperture", 0.0), focusDepth=c.get("focus"))

    @property
    def width(self):
        return self.c.width

    @property
    def height(self):
        return self.c.height


class OrthographicCamera(PerspectiveCamera):
    """`orthographic` camera plugin (src/cameras/orthographic.cpp): toWorld = lookAt * scale(sx, sy, 1)"""

    def __init__(self, origin, target, up, scale, width, height):
        self.c = abi.Camera()
        sx, sy = (scale, scale) if np.isscalar(scale) else scale
        check(lib().mtsgpu_make_camera_ortho(*_look_at(origin, target, up), C.c_float(sx), C.c_float(sy), int(width), int(height), C.byref(self.c)),
              "mtsgpu_make_camera_ortho")
