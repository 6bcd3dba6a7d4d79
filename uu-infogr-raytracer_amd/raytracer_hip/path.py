"""Camera paths for Context.render_path / render_path_bands: one rt_camera per frame.

`replay` is the reference's input loop, recorded: between two Tick() calls the application hands key presses to
OnKeyPress (RayTracer.cs:543-554) and mouse deltas to OnMouseMove (:1058-1061), and each Tick() renders the camera
they left.  The events go through the library's own rt_camera_on_key / rt_camera_on_mouse_move, so a replayed
path is, camera for camera, what an interactive RayTracer would have rendered.
"""
from __future__ import annotations

import ctypes as C

from . import abi

KEYS = {"W": abi.RT_KEY_W, "A": abi.RT_KEY_A, "S": abi.RT_KEY_S, "D": abi.RT_KEY_D,
        "Space": abi.RT_KEY_SPACE, "LeftShift": abi.RT_KEY_SHIFT, "RightShift": abi.RT_KEY_SHIFT}


def copy_camera(camera: abi.rt_camera) -> abi.rt_camera:
    c = abi.rt_camera()
    C.memmove(C.byref(c), C.byref(camera), C.sizeof(abi.rt_camera))
    return c


def replay(camera: abi.rt_camera, events) -> list:
    """The cameras of the frames of a recorded session.  events: ("key", name or code), ("mouse", dx, dy) and
    ("frame",); the camera after each ("frame",) is emitted.  `camera` itself is not modified."""
    lib = abi.load_library()
    cam = copy_camera(camera)
    out = []
    for ev in events:
        kind = ev[0]
        if kind == "key":
            code = KEYS.get(ev[1], 0) if isinstance(ev[1], str) else int(ev[1])
            abi.check(lib, lib.rt_camera_on_key(C.byref(cam), code))
        elif kind == "mouse":
            abi.check(lib, lib.rt_camera_on_mouse_move(C.byref(cam), float(ev[1]), float(ev[2])))
        elif kind == "frame":
            out.append(copy_camera(cam))
        else:
            raise ValueError(f"unknown path event {ev!r}")
    return out


def as_array(cameras):
    """The cameras as one contiguous ctypes array (abi.rt_camera * n), as the C calls take them."""
    if isinstance(cameras, C.Array) and cameras._type_ is abi.rt_camera:
        return cameras
    cams = list(cameras)
    arr = (abi.rt_camera * len(cams))()
    for i, c in enumerate(cams):
        C.memmove(C.byref(arr, i * C.sizeof(abi.rt_camera)), C.byref(c), C.sizeof(abi.rt_camera))
    return arr
