"""A few 64-frame rt_render_bands_batch launches of a config seen from a chosen camera (the bench's launch shape),
for counters-only profiling runs: `--pitch 1.2 --yaw 0.3` on C3 is the floor in every tile with no sphere box in view,
which prices one plane-uniform wave of the direct kernel (profiles/ab/r14_uniform_plane.txt).
    rocprofv3 --pmc SQ_INSTS_VALU ... -- python tools/plane_wave_probe.py --config C3 --pitch 1.2 --yaw 0.3 [--lib X.so]
"""
import argparse
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uu-infogr-raytracer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--yaw", type=float, default=None)
    ap.add_argument("--pitch", type=float, default=None)
    ap.add_argument("--launches", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lib", default="", help="library build to load instead of the in-tree one")
    a = ap.parse_args()
    import torch
    from raytracer_hip import Context, abi, scenes
    if a.lib:
        abi.LIB_PATH = os.path.abspath(a.lib)
    sc = scenes.config(a.config)
    if a.yaw is not None or a.pitch is not None:
        pos, yaw, pitch = sc.camera
        sc = dataclasses.replace(sc, camera=(pos, scenes.f32(a.yaw if a.yaw is not None else yaw),
                                             scenes.f32(a.pitch if a.pitch is not None else pitch)))
    W, H = sc.width, sc.height
    out = torch.empty(a.batch * W * H, dtype=torch.int32, device="cuda")
    with Context(1) as ctx:
        ctx.set_scene(sc)
        for _ in range(a.launches):
            ctx.render_bands_batch(W, H, 8, 0, 1, a.batch, out.data_ptr(), W * H * 4, abi.RT_BANDS_FRAME,
                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        st = ctx.stats()
    frame = out[:W * H].cpu()
    print(f"{os.path.basename(a.lib) or 'in-tree'} {a.config} {W}x{H} camera {sc.camera}: {a.launches} launches of {a.batch} frames, "
          f"{int((frame == 0).sum())} zero pixels in frame 0, rays per frame: reflect {st['reflect_rays'] // (a.launches * a.batch)} "
          f"shadow {st['shadow_rays'] // (a.launches * a.batch)}")


if __name__ == "__main__":
    main()
