"""Camera paths for Context.render_path / render_path_bands: one rt_camera per frame.

`replay` is the reference's input loop, recorded: between two Tick() calls the application hands key presses to
OnKeyPress (RayTracer.cs:543-554) and mouse deltas to OnMouseMove (:1058-1061), and each Tick() renders the camera
they left.  The events go through the library's own rt_camera_on_key / rt_camera_on_mouse_move, so a replayed
path is, camera for camera, what an interactive RayTracer would have rendered.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

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


def subframes(cameras, m: int) -> list:
    """The sub-frame cameras of a shutter over the key cameras (Context.render_shutter): n keys -> n * m cameras,
    sub-frame s of key k interpolated linearly towards key k + 1 at s / m -- position, yaw and pitch, each in
    binary32 as rt_camera holds them (a + (b - a) * (s / m), every step rounded to float32).  Sub-frame 0 is the
    key itself; the last key has no successor and holds.  m = 1 returns copies of the keys."""
    keys = list(cameras)
    if m < 1:
        raise ValueError("m must be at least 1")
    f32 = np.float32

    def lerp(a, b, w):
        return float(f32(f32(a) + f32(f32(f32(b) - f32(a)) * w)))

    out = []
    for k, key in enumerate(keys):
        nxt = keys[k + 1] if k + 1 < len(keys) else key
        for s in range(m):
            c = copy_camera(key)
            if s:
                w = f32(f32(s) / f32(m))
                c.position.x = lerp(key.position.x, nxt.position.x, w)
                c.position.y = lerp(key.position.y, nxt.position.y, w)
                c.position.z = lerp(key.position.z, nxt.position.z, w)
                c.yaw = lerp(key.yaw, nxt.yaw, w)
                c.pitch = lerp(key.pitch, nxt.pitch, w)
            out.append(c)
    return out


def shutter_mean(frames, m: int) -> np.ndarray:
    """The numpy reference of the shutter's resolve: frames [n * m, H, W] of 0x00RRGGBB pixels -> [n, H, W], each
    8-bit channel the round-half-up mean (sum + m // 2) >> log2(m) of its m sub-frames.  m: a power of two."""
    if m < 1 or m & (m - 1):
        raise ValueError("m must be a power of two")
    a = np.asarray(frames)
    if a.ndim != 3 or a.shape[0] % m:
        raise ValueError(f"frames {a.shape} are no [n * {m}, H, W]")
    t = m.bit_length() - 1
    px = a.astype(np.int64).reshape(a.shape[0] // m, m, a.shape[1], a.shape[2])
    out = np.zeros(px[:, 0].shape, dtype=np.int64)
    for shift in (16, 8, 0):
        ch = ((px >> shift) & 0xFF).sum(axis=1)
        out |= ((ch + m // 2) >> t) << shift
    return out.astype(np.int32)
