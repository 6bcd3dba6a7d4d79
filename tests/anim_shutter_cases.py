"""Shared by tests/test_gpu_anim_shutter.py: scene tracks with one scene and one camera per sub-frame, built from
tests/anim_cases.py's scenes by anim.tween and anim_cases.with_path_cameras, and the expected output frames -- the
shutter's rounding (path.shutter_mean, or supersample.path_resolve at k > 1) of the unchanged oracle's per-sub-frame
renders, each in that sub-frame's scene and camera (anim_cases.oracle_frames)."""
import dataclasses

import anim_cases
from raytracer_hip import anim, path, scenes
from raytracer_hip.supersample import path_resolve

RAYS = anim_cases.RAYS


def tweened(a, b, n, prefix):
    """n sub-frame scenes from key a to key b (both reproduced), sub-frame j seen from a's camera moved by path offset
    j % 6."""
    a, b = dataclasses.replace(a, name=prefix), dataclasses.replace(b, name=prefix, camera=a.camera)
    return anim_cases.named(anim_cases.with_path_cameras(anim.tween([a, b], n - 1)), prefix)


def direct_track(n, W=100, H=60):
    """anim_cases.direct_track's keys (C3's scene: a sphere crossing the frame, a growing sphere, a moving light, a
    rising floor, a changing ambient) tweened into n sub-frames."""
    t = anim_cases.direct_track(W, H)
    return tweened(t[0], t[4], n, f"ashut_direct_{n}_{W}x{H}")


def bright_track(n, W=16, H=8):
    """direct_track under an ambient of 2.1 .. 3: the floor's ambient term alone (Ka = 0.5) is above 1 in every
    sub-frame, so the pixels that stay on the floor hold 255 throughout."""
    t = anim_cases.direct_track(W, H)
    return tweened(dataclasses.replace(t[0], ambient=scenes.vec(2.5, 2.5, 2.5)),
                   dataclasses.replace(t[4], ambient=scenes.vec(3.0, 2.2, 2.1)), n, f"ashut_bright_{n}_{W}x{H}")


def bundle_track(n, W=64, H=40):
    """anim_cases.bundle_track's keys (C4's scene, half the spheres and two lights moving) tweened into n sub-frames."""
    t = anim_cases.bundle_track(W, H)
    return tweened(t[0], t[-1], n, f"ashut_bundle_{n}_{W}x{H}")


def class_track(cls, gpow, limit):
    """The 4 sub-frames tween([a, b], 3) of a class's key scenes (anim_cases.class_track's frames 0 and 2)."""
    t = anim_cases.class_track(cls, gpow, limit)
    return tweened(t[0], t[-1], 4, f"ashut_{cls}_{'gpow' if gpow else 'pow'}_lim{limit}")


def descriptor(cls, gpow, limit):
    """(family, gpow, class, K) of the ANIM_SHUTTER instantiation a track of this class runs: ANIM's."""
    return anim_cases.descriptor(cls, gpow, limit)


def cameras(track):
    return [sc.c_camera() for sc in track]


def subframes(oracle, track, k=1, W=None, H=None, view_h=None):
    """(sub-frame renders [n, k H, k W], [stats]) of the oracle, each in its own scene and camera."""
    W, H = W or track[0].width, H or track[0].height
    return anim_cases.oracle_frames(oracle, track, k * W, k * H, k * view_h if view_h else None)


def resolve(frames, k, m):
    return path.shutter_mean(frames, m) if k == 1 else path_resolve(frames, k, m)


def expected(oracle, track, m, k=1, first_frame=0, n_frames=None, W=None, H=None, view_h=None):
    """(frames [n_frames, H, W], summed ray counts) of n_frames output frames of m sub-frames from track frame
    first_frame on (to the end of the track when n_frames is None)."""
    sub, st = subframes(oracle, track, k, W, H, view_h)
    n = (len(track) - first_frame) // m if n_frames is None else n_frames
    sel = slice(first_frame, first_frame + n * m)
    return resolve(sub[sel], k, m), anim_cases.summed(st[sel])


def wrong_scene_alternatives(oracle, track, m, k=1, first_frame=0, n_frames=None):
    """What three kernels that read the wrong scene image would write, from oracle renders: every sub-frame of output
    frame z traced in (a) sub-frame 0's scene of that frame, (b) track frame first_frame + z's scene, (c) the scene
    the launch would read with first_frame ignored -- each still from the sub-frame's own camera."""
    n = (len(track) - first_frame) // m if n_frames is None else n_frames
    W, H = track[0].width, track[0].height

    def render(scene_of):
        mixed = []
        for z in range(n):
            for s in range(m):
                j = first_frame + z * m + s
                src = track[scene_of(z, s)]
                mixed.append(dataclasses.replace(src, camera=track[j].camera, name=f"{track[j].name}@{src.name}"))
        sub, _ = anim_cases.oracle_frames(oracle, mixed, k * W, k * H)
        return resolve(sub, k, m)

    return {"sub-frame 0's scene": render(lambda z, s: first_frame + z * m),
            "track frame z's scene": render(lambda z, s: first_frame + z),
            "first_frame ignored": render(lambda z, s: z * m + s)}


def assert_discriminates(oracle, track, m, k=1, first_frame=0, n_frames=None):
    """The oracle's sub-frames of every output frame are pairwise different, and the expected frames differ from each
    wrong-scene alternative (first_frame = 0 makes the third the expectation itself: it is then left out)."""
    sub, _ = subframes(oracle, track, k)
    want, _ = expected(oracle, track, m, k, first_frame, n_frames)
    for z in range(want.shape[0]):
        base = first_frame + z * m
        for a in range(m):
            for b in range(a + 1, m):
                assert (sub[base + a] != sub[base + b]).any(), f"sub-frames {a} and {b} of output frame {z} are one frame"
    for what, alt in wrong_scene_alternatives(oracle, track, m, k, first_frame, n_frames).items():
        if what == "first_frame ignored" and first_frame == 0:
            continue
        assert (alt != want).any(), f"a kernel tracing in {what} would pass"
    return want
