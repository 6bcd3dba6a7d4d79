"""GPU tests of the exact paths the bench line and the C# shim take (VERDICT r1 items 3, 4,
6, 10 and ADVICE r1 bench.py:259), every call through the C ABI:

* bench.py's timed launch shape -- balanced rt_render_bands_batch launches of up to 64 full
  1920x1080 frames, one stream (and the two-stream swap chain) -- every frame's CRC against
  tests/golden/golden.json for C2 and C3 (the north-star config);
* (the single-process multi-GPU Tick and the forced RCCL gather path: tests/test_gpu_tick.py);
* the headless display hand-off (rt_write_ppm) of a GPU-rendered frame vs the oracle's pixels
  (template.cs:186-209);
* rt_count_work: nominal counts = the timed kernels' counts, executed counts bounded by them;
* the tile-codec pipeline of bench.py's N>1 path on CUDA streams (torch.distributed "nccl" =
  RCCL, world 1): decoded frames = a single-launch render.
"""
import os
import socket
import subprocess
import sys
import zlib

import numpy as np
import pytest

from raytracer_hip import Context, RayTracer, Surface, abi, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (plan_launches: the bench's own launch split)


def crc(a):
    return f"{zlib.crc32(np.ascontiguousarray(a, dtype=np.int32).tobytes()) & 0xFFFFFFFF:08x}"


@pytest.mark.parametrize("cid", ["C2", "C3"])
@pytest.mark.parametrize("steps,inflight", [(20, 1), (100, 1), (64, 1), (96, 2)])
def test_bench_launch_shape_every_frame_golden(gpu_ctx, golden, cid, steps, inflight):
    import torch
    e = golden["cases"][cid]
    sc = scenes.config(cid)
    W, H = sc.width, sc.height
    gpu_ctx.set_scene(sc)
    gpu_ctx.reset_stats()
    plan = bench.plan_launches(steps, 64)
    assert sum(plan) == steps and max(plan) - min(plan) <= 1 and max(plan) <= 64
    bufs = [torch.full((max(plan) * W * H,), -1, dtype=torch.int32, device="cuda") for _ in range(inflight)]
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(inflight - 1)]
    want = None
    for k, m in enumerate(plan):
        i = k % inflight
        if k >= inflight:  # the slot's previous launch is checked before it is reused
            streams[i].synchronize()
        gpu_ctx.render_bands_batch(W, H, H, 0, 1, m, bufs[i].data_ptr(), W * H * 4, abi.RT_BANDS_INT32,
                                   streams[i].cuda_stream)
        streams[i].synchronize()
        frames = bufs[i][:m * W * H].view(m, W * H)
        if want is None:
            want = frames[0].clone()
            assert crc(want.cpu().numpy()) == e["crc32"], f"{cid} frame 0 of launch 0"
        same = (frames == want).all(dim=1)
        assert bool(same.all()), f"{cid} launch {k}: frames {torch.nonzero(~same).flatten().tolist()} differ"
    st = gpu_ctx.stats()
    for k in ("primary_rays", "reflect_rays", "shadow_rays"):
        assert st[k] == steps * e["stats"][k], k  # frame 0 counts for every frame of a batch


def test_plain_bench_dumps_its_last_timed_frame(tmp_path, golden):
    """A plain bench.py run (no --full) of 70 frames -- two launches of 35: the dumped frame is the last slot of the
    last launch -- writes the golden C3 frame as R G B planes, and its line carries the headline alone."""
    import json
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "70", "--warmup", "3",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 70 and line["roofline"]["launches"] == 2 and line["ms_per_step"] > 0
    assert line["unit"] == "Mray/s" and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["config"]["rays_per_frame"] == sum(golden["cases"]["C3"]["stats"][k] for k in
                                                   ("primary_rays", "reflect_rays", "shadow_rays"))
    for k in ("also", "tick_by_config", "work_per_frame", "tick_fps_incl_d2h"):
        assert k not in line, k
    assert line["cpu_baseline"] is None
    rgb, rows = np.load(out / "frame_rgb.npy"), np.load(out / "frame_rows.npy")
    assert rgb.dtype == np.float32 and rgb.shape == (1080, 1920, 3) and np.array_equal(rows, np.arange(1080))
    px = (rgb[..., 0].astype(np.int32) << 16) | (rgb[..., 1].astype(np.int32) << 8) | rgb[..., 2].astype(np.int32)
    assert crc(px) == golden["cases"]["C3"]["crc32"]


def test_ppm_of_gpu_frame_matches_oracle(tmp_path, oracle):
    """Tick() of the verbatim reference scene (512x512, 2 lights, limit 32) on the GPU, written
    by rt_write_ppm: the RGB bytes are the oracle's pixels, byte for byte."""
    sc = scenes.reference(512, 512)
    surf = Surface(512, 512)
    rt = RayTracer(surf, sc)
    try:
        rt.Tick()
        path = str(tmp_path / "ref.ppm")
        surf.save_ppm(path)
    finally:
        rt.close()
    want, _ = oracle.render(sc, oracle.MODE_NEAREST)
    data = open(path, "rb").read()
    head = b"P6\n512 512\n255\n"
    assert data.startswith(head) and len(data) == len(head) + 512 * 512 * 3
    rgb = np.frombuffer(data[len(head):], dtype=np.uint8).reshape(512, 512, 3)
    u = want.view(np.uint32)
    exp = np.stack([(u >> 16) & 255, (u >> 8) & 255, u & 255], axis=-1).astype(np.uint8)
    assert np.array_equal(rgb, exp)


@pytest.mark.parametrize("cid", ["C1", "C2", "C3", "C4"])
def test_count_work(gpu_ctx, golden, cid):
    """Diagnostic kernels: same nominal counts as the golden / timed kernels, executed work
    bounded by the nominal counts, and the frame they trace is the golden frame."""
    e = golden["cases"][cid]
    sc = scenes.config(cid)
    gpu_ctx.set_scene(sc)
    w = gpu_ctx.count_work(sc.width, sc.height)
    for k in ("primary_rays", "reflect_rays", "shadow_rays"):
        assert w[k] == e["stats"][k], k
    S, P = len(sc.spheres), len(sc.planes)
    rays = w["primary_rays"] + w["reflect_rays"]
    assert w["sphere_tests"] == (rays + w["shadow_rays"]) * S and w["plane_tests"] == rays * P
    assert 0 < w["shadow_rays_run"] <= w["shadow_rays"]
    assert 0 < w["sphere_tests_run"] <= w["sphere_tests"]
    assert 0 < w["plane_tests_run"] <= w["plane_tests"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("extra,shape", [(["--rank0-codec"], "small"), ([], "small"),
                                         (["--rank0-codec", "--inflight", "3"], "small"),
                                         (["--rank0-codec"], "full"), (["--rank0-codec"], "short")])
def test_tile_pipeline_on_cuda_streams(extra, shape):
    """bench.py's N>1 tile pipeline (encode, size all_reduce, gather, decode on side streams,
    event-ordered buffer reuse) with a real RCCL process group of one rank: rank 0 checks every
    frame left in its rings against a single-launch render (--verify, exit 3 on a mismatch).
    "full": 1080p C2, 300 frames in batches of 64 with speculative gather sizes -- the shape that
    exposed speculative gathers not ordered after their encode (fixed by an encode event);
    "short": the driver's 20 frames, one batch through the gather-first path.  --inflight 3:
    batches on three trace streams (every one waits for the encode of the batch whose raw buffer
    it reuses)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    env.pop("WORLD_SIZE", None)
    size = {"small": ["--size", "640x360", "--steps", "40", "--warmup", "16", "--batch", "8"],
            "full": ["--steps", "300", "--warmup", "64"],
            "short": ["--steps", "20", "--warmup", "5"]}[shape]
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--dist-path", "--config", "C2",
           "--no-cpu-baseline"] + size + extra  # (--full: frames verified by default on the N > 1 path)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["verified_frames"] >= 16 and line["n_gpus"] == 1


@pytest.mark.parametrize("world,extra", [(2, []), (3, ["--rank0-share", "off", "--compositor", "on"]),
                                         (3, ["--rank0-share", "48"]), (4, ["--rank0-share", "auto"])])
def test_bench_multi_rank_rehearsal(world, extra):
    """bench.py --gpus N as N processes (started by bench.py itself through torch.distributed.run)
    sharing this GPU, collectives over gloo (--rehearse-gloo: RCCL refuses two ranks on one GPU):
    every rank's N > 1 code path -- its bands, the tile codec, the pipelined size reduce and
    gather, rank 0's decode (or compositor mode, or rank 0's measured share: the frame's last rows
    rendered by rank 0, the rows above traced by ranks 1..N-1 with the whole frame's view), the
    barrier and max-over-ranks timing -- with rank 0's frames checked against a single-launch render
    (--verify)."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", str(world), "--rehearse-gloo",
           "--master-port", str(_free_port()), "--config", "C3", "--size", "640x360", "--steps", "48", "--warmup", "16",
           "--batch", "8", "--no-cpu-baseline"] + extra  # (--full: frames verified by default at N > 1)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["n_gpus"] == world and line["verified_frames"] >= 16 and "rehearsal" in line


def test_driver_shape_forced_repeat_counts_one_attempt():
    """The driver's N > 1 shape (20 frames, one batch, speculative gather with the size check
    deferred past the timed region) with the speculative size forced too short (--spec-margin 0.5):
    the timed region is repeated with exact sizes, and the line reports that attempt alone -- the
    same rays per frame and wire bytes per frame as an unforced run (the counters of
    both attempts were summed) -- with every frame verified (the default at N > 1)."""
    import json
    lines = []
    for margin in ("1.25", "0.5"):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
        env.pop("WORLD_SIZE", None)
        # (--rank0-codec: rank 0 ships its own bands through the codec, so the world-1 wire is not empty)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--dist-path", "--rank0-codec", "--config", "C2",
               "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--also-dist", "", "--spec-margin", margin]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=110)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    plain, forced = lines
    assert plain["config"]["timed_region_repeats"] == 0 and forced["config"]["timed_region_repeats"] == 1
    assert plain["verified_frames"] == forced["verified_frames"] == 20
    assert forced["config"]["rays_per_frame"] == plain["config"]["rays_per_frame"]
    # wire bytes moved: the plain run gathers its speculative size (1.25 x the warm-up's wire), the
    # repeat the exact size -- once, not added to the first attempt's
    fb, pb = forced["config"]["gather_wire_bytes_per_frame"], plain["config"]["gather_wire_bytes_per_frame"]
    assert 0 < fb < pb <= 1.26 * fb
    assert forced["config"]["gather_redone_batches"] == 0
