/*
 * raytracer_hip.h -- C ABI of libraytracer_hip, the MI355X (gfx950) drop-in for the
 * per-pixel Whitted trace of TobiasDeBruijn/UU-INFOGR-Raytracer.
 *
 * The reference has no FFI: its plugin surface is the C# class
 *   RayTracer(Surface screen)          Raytracer/RayTracer.cs:535-537
 *   public readonly Surface screen     Raytracer/RayTracer.cs:506
 *   public void Tick()                 Raytracer/RayTracer.cs:886-935
 *   OnKeyPress(KeyboardKeyEventArgs)   Raytracer/RayTracer.cs:543-554
 *   OnMouseMove(MouseMoveEventArgs)    Raytracer/RayTracer.cs:1058-1061
 * plus Surface.width/height/int[] pixels (Raytracer/surface.cs:9-20).  Every entry
 * point below replaces one piece of that surface; the C# P/Invoke shim that binds
 * them is in INTEGRATION.md / shim/csharp/RayTracer.cs.
 *
 * Conventions
 *  - Plain C, blittable POD structs of float32/int32 (no packing pragmas, no torch
 *    types).  All functions return RT_OK (0) or a negative RT_ERR_* code and never
 *    throw; rt_last_error() returns the message of the last failure.
 *  - A context is used by one thread at a time (the reference calls Tick, OnKeyPress
 *    and OnMouseMove from the GLFW render thread, template.cs:175-230).
 *  - There is NO CPU fallback: rt_create fails with RT_ERR_NO_DEVICE when no gfx950
 *    device is visible.
 */
#ifndef RAYTRACER_HIP_H
#define RAYTRACER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 10

/* ---- status codes ---------------------------------------------------------- */
enum {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = -1,   /* NULL pointer, negative size, bad enum value          */
    RT_ERR_NO_DEVICE = -2,     /* no HIP device / not enough devices for n_gpus        */
    RT_ERR_HIP = -3,           /* a HIP runtime call failed (message has the HIP text) */
    RT_ERR_NO_SCENE = -4,      /* render before rt_set_scene                          */
    RT_ERR_UNSUPPORTED = -5,   /* e.g. recursion_limit above RT_MAX_RECURSION_LIMIT    */
    RT_ERR_RCCL = -6,          /* a RCCL call failed (multi-GPU contexts)              */
    RT_ERR_OOM = -7            /* device allocation failed                            */
};

/* Deepest mirror chain the kernel's per-lane level stack holds: a limit of L
 * shades levels 0..L (L+1 stack records).  The reference's own limit is 32
 * (RayTracer.cs:490). */
#define RT_MAX_RECURSION_LIMIT 63
#define RT_MAX_LIGHTS 65536  /* per-lane shadow-ray counts are kept in 24 bits */

/* ---- scene description (RayTracer.cs:60-338, :441-469) ---------------------- */
typedef struct rt_vec3 {
    float x, y, z;
} rt_vec3;

/* Material, RayTracer.cs:60-110.  Flags are derived exactly as the reference does:
 * IsMirror = km != 0, IsDiffuse = kd != 0, HasSpecularity = ks != 0 && n > 0
 * (RayTracer.cs:85-93). */
typedef struct rt_material {
    rt_vec3 kd;  /* diffuseColor  K_d */
    rt_vec3 ka;  /* ambientColor  K_a */
    rt_vec3 ks;  /* specularColor K_s */
    float n;     /* specularity   n   */
    rt_vec3 km;  /* mirrorColor   K_m */
} rt_material;

/* Sphere, RayTracer.cs:308-338 (radiusSquared = radius*radius, :336). */
typedef struct rt_sphere {
    rt_vec3 center;
    float radius;
    rt_material material;
} rt_sphere;

/* Plane, RayTracer.cs:260-303.  Planes are always checkerboard-tiled: the
 * reference's constructor ignores its isTiled argument (RayTracer.cs:289). */
typedef struct rt_plane {
    rt_vec3 center;
    rt_vec3 normal;
    rt_material material;
} rt_plane;

/* Light, RayTracer.cs:236-255. */
typedef struct rt_light {
    rt_vec3 position;
    float intensity;
} rt_light;

/* Camera state of the reference: _cameraPosition, _yaw, _pitch (RayTracer.cs:494-502).
 * The basis (RayTracer.cs:511-523) and view-plane size (RayTracer.cs:892-896) are
 * derived from it once per frame on the host with the reference's double-precision
 * trig (rt_camera_view). */
typedef struct rt_camera {
    rt_vec3 position;
    float yaw;
    float pitch;
} rt_camera;

/* Per-frame view derived from rt_camera and the surface size. */
typedef struct rt_view {
    rt_vec3 position;
    rt_vec3 right;    /* CameraRightDirection   RayTracer.cs:517-518 */
    rt_vec3 up;       /* CameraUpDirection      RayTracer.cs:522-523 */
    rt_vec3 forward;  /* CameraForwardDirection RayTracer.cs:511-513 */
    float plane_width, plane_height, near_clip;  /* viewParams RayTracer.cs:892-896 */
} rt_view;

/* Reference keys handled by OnKeyPress (RayTracer.cs:545-553). */
enum {
    RT_KEY_W = 1, RT_KEY_A = 2, RT_KEY_S = 3, RT_KEY_D = 4,
    RT_KEY_SPACE = 5, RT_KEY_SHIFT = 6
};

/* Work counters of the visible (nearest-hit) path, accumulated since the last
 * rt_reset_stats.  rays = primary + reflected segments (terminal segments included);
 * shadow_rays = shaded diffuse hits x lights.  Times are device time measured with
 * HIP events on the stream the operation runs on, for the sampled operations only (see
 * rt_set_timing): average kernel duration = kernel_ms / timed_launches.  rt_render_async
 * ticks hand the previous frame to its host buffer inside the next frame's launch (a copy
 * slice ahead of the trace workgroups): that copy's share is in the launch's kernel_ms, the
 * last frame's copy (issued by rt_wait / the next synchronous call) is not timed, and
 * copy_ms / timed_copies count rt_render's D2H copies only. */
typedef struct rt_stats {
    uint64_t frames;
    uint64_t pixels;
    uint64_t primary_rays;
    uint64_t reflect_rays;
    uint64_t shadow_rays;
    uint64_t sphere_tests;   /* algorithmic: (primary+reflect+shadow) x S */
    uint64_t plane_tests;    /* algorithmic: (primary+reflect) x P        */
    uint64_t launches;
    double kernel_ms;        /* sum of trace-kernel durations            */
    double last_kernel_ms;
    double copy_ms;          /* sum of D2H / reassembly copy durations    */
    double gather_ms;        /* sum of RCCL gather durations (multi-GPU)  */
    uint64_t timed_launches; /* launches whose durations are in kernel_ms  */
    uint64_t timed_copies;   /* copies in copy_ms                          */
    uint64_t timed_gathers;  /* gathers in gather_ms                       */
} rt_stats;

/* Nominal and executed work of one frame (rt_count_work, ABI 5).  The nominal counts are
 * SURVEY.md 8(d)'s (every primitive of every visible-path ray; Mray/s counts these rays).
 * The kernels skip work that provably cannot change a pixel -- shadow rays whose outcome
 * cannot matter (shadow_rays_run <= shadow_rays), sphere tests culled by screen boxes, wave
 * bundles and the terminal-segment rule -- so the *_run counts are what actually ran: per
 * lane, each exact IntersectsSphere / IntersectPlane evaluation whose result the lane used. */
typedef struct rt_work {
    uint64_t primary_rays, reflect_rays, shadow_rays;  /* nominal, as rt_stats          */
    uint64_t sphere_tests, plane_tests;                /* nominal, as rt_stats          */
    uint64_t shadow_rays_run;   /* shadow rays whose sphere loop ran                   */
    uint64_t sphere_tests_run;  /* exact sphere tests executed (trace + shadow rays)   */
    uint64_t plane_tests_run;   /* exact plane tests executed                          */
} rt_work;

typedef struct rt_ctx rt_ctx;

/* ---- library / device ------------------------------------------------------- */
int rt_abi_version(void);
/* Number of visible HIP devices (0 when none).  Returns RT_OK or RT_ERR_HIP. */
int rt_device_count(int* out_count);
/* Message of the last failure on ctx (ctx may be NULL: last failure of this thread). */
const char* rt_last_error(const rt_ctx* ctx);

/* ---- context lifetime  (replaces `new RayTracer(screen)`, RayTracer.cs:535) ---- */
/* n_gpus >= 1 band workers, one per device (devices 0 .. n_gpus-1; n_gpus == 1: the caller's
 * current device), each with its own HIP stream.  A frame is split into interleaved 8-row bands,
 * band b on worker b % n_gpus (ABI 9): rt_render / rt_render_async hand every
 * worker's bands to the caller's host frame over that device's own PCIe link (no gather, no
 * single-link copy of the whole frame); rt_render_device gathers them to device 0 over RCCL/xGMI
 * (ncclCommInitAll, made on first use). */
#define RT_MAX_WORKERS 64
int rt_create(int n_gpus, rt_ctx** out_ctx);
/* rt_create with flags.  RT_CREATE_RCCL_GATHER (ABI 5): rt_render gathers the bands to device 0 over
 * RCCL (grouped ncclGather, one-launch reassembly) and copies the whole frame over device 0's link --
 * for callers that need the frame assembled on device 0; communicators made at creation, any
 * n_gpus, 1 included.  RT_CREATE_SHARED_DEVICE (ABI 9): all n_gpus workers on the caller's current
 * device (a stream each) -- the multi-GPU band pipeline rehearsed on one GPU; rt_render_device then
 * writes the workers' bands straight into the frame (no RCCL: it refuses two ranks on one device). */
enum { RT_CREATE_RCCL_GATHER = 1, RT_CREATE_SHARED_DEVICE = 2 };
int rt_create_ex(int n_gpus, int flags, rt_ctx** out_ctx);
void rt_destroy(rt_ctx* ctx);

/* ---- scene (replaces the hard-coded fields RayTracer.cs:441-490) ------------- */
int rt_set_scene(rt_ctx* ctx,
                 const rt_sphere* spheres, int n_spheres,
                 const rt_plane* planes, int n_planes,
                 const rt_light* lights, int n_lights,
                 rt_vec3 ambient, int recursion_limit);

/* ---- camera (mirrors RayTracer.cs:511-523, :543-554, :892-896, :1058-1061) ---- */
int rt_set_camera(rt_ctx* ctx, const rt_camera* camera);
/* (ABI 9) The view's height: later renders of a width x height frame with height <= view_height trace
 * rows [0, height) of the view of a width x view_height frame (TracePixel's y / height, :963-965, with
 * the view's height) -- the multi-GPU pipeline's tracing ranks when rank 0 renders the frame's last rows
 * itself; 0 (the default) = each render's own height.  The debug view ignores it. */
int rt_set_view_height(rt_ctx* ctx, int view_height);
/* (ABI 10 addition) Supersampling: k = 1 (the default, off), 2, 4 or 8 samples per pixel and axis.  With
 * k > 1 every render that writes pixels -- rt_render, rt_render_async (which captures the factor with the
 * camera), rt_render_device, rt_render_bands, rt_render_bands_ex in every format and
 * rt_render_bands_batch, on contexts of any n_gpus -- still produces a width x height output, and all
 * arguments stay in output pixels (width, height, band_rows, band indices, buffer sizes, rt_set_view_height).
 * Sample (i, j) of output pixel (x, y) is the reference's pixel (k x + i, k y + j) of a k width x k height
 * frame (TracePixel :962-971), and the output pixel is, per 8-bit channel, the round-half-up mean of its
 * k*k samples after ShiftColor: (sum + k*k/2) >> 2 log2 k.  The trace kernels reduce each block in
 * registers: no sample buffer exists and the frame that leaves the device keeps its size.
 * (long long) k width * k height must not exceed 2^31 - 1 (RT_ERR_INVALID_ARG from the render calls).
 * Statistics: frames and pixels count output frames and pixels; primary_rays, reflect_rays, shadow_rays
 * and the test counts count samples (the reference's counts at k width x k height).
 * While k > 1, rt_render_bands_tiles and rt_count_work return RT_ERR_UNSUPPORTED; rt_debug_segments
 * ignores the factor (as it ignores the view height).  Single frames at k > 1 run in natural tile order
 * (rt_dispatch_order's tuner serves k = 1 only).  k = 1 is exactly the library without this call.
 * Returns RT_ERR_INVALID_ARG for a NULL ctx or any other k. */
int rt_set_supersampling(rt_ctx* ctx, int k);
int rt_get_supersampling(const rt_ctx* ctx, int* out_k);
/* (ABI 10 addition) Supersampling for the camera-path, shutter and scene-track renders: k = 1 (the default, off),
 * 2, 4 or 8.  A setting of its own, as rt_set_progressive's factor is: only rt_render_path[_bands],
 * rt_render_shutter[_bands] and rt_render_anim[_bands] read it, and every other render ignores it.
 * rt_set_supersampling keeps its meaning and its refusal: with it above 1 those six calls return
 * RT_ERR_UNSUPPORTED whatever this factor is.
 *   - Units: all arguments stay in output pixels -- width, height, band_rows, band indices, frame_stride_bytes,
 *     rt_set_view_height, buffer sizes.
 *   - Samples: sample (i, j) of output pixel (x, y) of frame f is the reference's pixel (k x + i, k y + j) of a
 *     k width x k height frame rendered with frame f's camera (and, for rt_render_anim*, frame f's scene).
 *   - Output, with a shutter of m sub-frames (m = 1 for the path and track calls): per 8-bit channel after
 *     ShiftColor, (sum over the m sub-frames and the k*k samples + m k*k / 2) >> (log2 m + 2 log2 k) -- one rounding
 *     of the whole mean, not a mean of means.  m = 1 is rt_set_supersampling's formula, k = 1 the shutter's.
 *   - Shutter bound: m * k*k <= RT_MAX_SHUTTER, so that a channel's sum and its rounding term fit 16 bits; otherwise
 *     RT_ERR_INVALID_ARG, checked with the other shutter arguments before any device call.
 *   - Frame-size bound: (long long) k width * k height (the view height, when one is set) must not exceed
 *     2^31 - 1; otherwise RT_ERR_INVALID_ARG.
 *   - The trace kernels reduce each block in registers: no sample and no sub-frame reaches memory, and the frame
 *     that leaves the device keeps its size.  rt_render_path's chunk rule counts output frames.
 *   - k = 1: exactly the launches, kernels and bytes of the library without this call.  shutter == 1 is the path
 *     call at every k.
 *   - Statistics: frames and pixels count output frames and pixels; with counting on, primary_rays grows by the
 *     traced output pixels x k*k x n_frames x shutter and reflect_rays / shadow_rays by the sum over every sample of
 *     every sub-frame; with counting off nothing grows.
 *   - rt_set_adaptive_sampling and the progressive setting stay ignored by these calls (their adaptive threshold is
 *     rt_set_path_adaptive_sampling).  Single-GPU contexts only, as before.
 * Returns RT_ERR_INVALID_ARG for a NULL ctx or out pointer, or any other k. */
int rt_set_path_supersampling(rt_ctx* ctx, int k);
int rt_get_path_supersampling(const rt_ctx* ctx, int* out_k);
/* (ABI 10 addition) Adaptive supersampling: with a threshold T in 1..256 and k > 1, only the 8x8 tiles of the
 * output whose pixels differ are supersampled (Whitted's criterion per tile); T = 0 (the default) is off -- every
 * pixel gets its k*k samples, by the kernels of rt_set_supersampling, unchanged.  At k = 1 the setting is stored
 * and ignored.  Definition, with W x H the columns and rows a call renders: P is the frame without supersampling,
 * which is sample (0, 0) of every block bit for bit; S is the supersampled frame; tile (tx, ty) is the output
 * pixels [8 tx, 8 tx + 8) x [8 ty, 8 ty + 8) clipped to W x H.  A tile is refined iff it holds two 4-adjacent
 * pixels, both inside the tile and the frame, whose values in P differ by >= T in at least one 8-bit channel
 * (pairs across a tile border do not count).  Output = S on refined tiles, P elsewhere.  T = 256 refines nothing
 * (the plain frame), T = 1 every tile that is not one colour.  A wave traces sample (0, 0) of its tile, decides,
 * and traces the other k*k - 1 samples only when refined: nothing extra is traced for the decision.
 * It applies to every render that supersamples: rt_render, rt_render_async (which captures the threshold with
 * the camera and the factor), rt_render_device, rt_render_bands, rt_render_bands_ex in every format and
 * rt_render_bands_batch, on contexts of any n_gpus.  Tiles sit on the frame's 8-row grid: with T > 0 and k > 1 a
 * band render needs band_rows % 8 == 0 or band_rows >= height (the whole frame), else RT_ERR_UNSUPPORTED before
 * any launch.  A tile's decision sees only the rows the call renders: under rt_set_view_height the last tile row
 * of a render whose height is no multiple of 8 is cut at that height, and so is its decision.
 * Cost: a throughput feature for batch renders (1080p, T = 16, k = 4: 3.4 plain frames instead of 15.8 on the 8-sphere
 * config).  A refined tile's k*k traces run one after the other in its wave, so a lone frame takes at least k*k
 * times the latency of its slowest tile and can take longer than full supersampling: leave it off in a display loop.
 * Statistics: primary_rays counts the samples traced -- one per rendered pixel and k*k - 1 more per pixel of every
 * refined tile -- and reflect_rays / shadow_rays those samples' rays; frames and pixels as for supersampling.
 * Returns RT_ERR_INVALID_ARG for a NULL ctx (or out_threshold) or a threshold outside 0..256. */
int rt_set_adaptive_sampling(rt_ctx* ctx, int threshold);
int rt_get_adaptive_sampling(const rt_ctx* ctx, int* out_threshold);
/* (ABI 10 addition) Adaptive supersampling for the camera-path and scene-track renders: a threshold T of their own,
 * 0 (the default, off) .. 256, beside rt_set_path_supersampling's factor k as rt_set_adaptive_sampling is beside
 * rt_set_supersampling's.  Only rt_render_path[_bands], rt_render_anim[_bands] and the shutter calls read it; every
 * other render ignores it, and rt_set_adaptive_sampling stays ignored by these six calls.
 *   - Definition: per output frame f, rt_set_adaptive_sampling's, with P the frame the call writes at path factor 1
 *     for frame f's camera (and, for a track, frame f's scene) and S the frame it writes at path factor k with the
 *     threshold 0.  Tiles are the 8x8 output tiles of the rendered rows; a tile is refined iff it holds two 4-adjacent
 *     pixels, both inside the tile and the frame, that differ by >= T in a channel of P; output = S on refined tiles,
 *     P elsewhere.  Every frame decides for itself, in its own view and scene.
 *   - T = 256 is the plain path frame, bit for bit.  T = 0, or k = 1, is exactly the launches, kernels and bytes of
 *     the library without this call.
 *   - A wave traces sample (0, 0) of its tile, decides with one ballot, and traces the other k*k - 1 samples only
 *     when the tile is refined: nothing extra is traced for the decision, and no sample reaches memory.
 *   - Bands: with T > 0 and k > 1 the band calls need band_rows % 8 == 0 or band_rows >= height, else
 *     RT_ERR_UNSUPPORTED before any device call.  Under rt_set_view_height a last tile row is cut at the rendered
 *     height, and so is its decision.
 *   - Shutter: shutter == 1 is the path call, as everywhere.  With T > 0, k > 1 and shutter > 1 the two shutter calls
 *     return RT_ERR_UNSUPPORTED, checked with the other shutter arguments, and write nothing: a decision on a mean of
 *     sub-frames needs the sub-frame index and the sample pass side by side in the tile trace, which is not built.
 *     That refusal is the answer while rt_set_shutter_adaptive_sampling's threshold is 0 (its default): this threshold
 *     does not cover shutters, and a caller who set only this one learns so instead of paying for full supersampling.
 *     With the shutter threshold set the shutter calls render adaptively at that threshold and do not consult this one.
 *   - Statistics: frames and pixels count output frames and pixels; with counting on, primary_rays grows by the
 *     traced output pixels x n_frames plus k*k - 1 per valid pixel of every refined tile of every frame, and
 *     reflect_rays / shadow_rays by those samples' rays, every frame counting for itself; with counting off nothing
 *     grows.
 *   - Cost (1080p, 64-frame launches, counting off): see README "Adaptive paths".  Single-GPU contexts only, as the
 *     calls themselves.
 * Returns RT_ERR_INVALID_ARG for a NULL ctx or out pointer, or a threshold outside 0..256. */
int rt_set_path_adaptive_sampling(rt_ctx* ctx, int threshold);
int rt_get_path_adaptive_sampling(const rt_ctx* ctx, int* out_threshold);
/* (ABI 10 addition) Adaptive supersampling for the camera and scene-track shutters: a threshold T of their own, 0 (the
 * default, off) .. 256.  Only rt_render_shutter[_bands] and rt_render_anim_shutter[_bands] read it, and only at
 * shutter > 1 with a path factor k > 1 (rt_set_path_supersampling): that is "in effect" below.  At shutter == 1 the
 * call remains the path or track call, reads rt_set_path_adaptive_sampling and ignores this setting; every other render
 * ignores it, and rt_set_adaptive_sampling stays ignored by these calls.
 *   - In effect: the path threshold is not consulted, so there is no refusal -- the call renders adaptively at this
 *     threshold.  Not in effect (T = 0): the library as it is without this call -- full supersampling of every
 *     sub-frame when the path threshold is 0, and RT_ERR_UNSUPPORTED when the path threshold is set.
 *   - Definition, per output frame f of m = shutter sub-frames, each in its own camera (and, for a track, its own
 *     scene): P_f is the frame the call writes at path factor 1, per channel (sum of the m sub-frames + m / 2) >>
 *     log2 m; S_f is the frame it writes at factor k with every threshold 0, (sum + m k*k / 2) >> (log2 m + 2 log2 k).
 *     Tiles are the 8x8 output tiles of the rendered rows; a tile is refined iff it holds two 4-adjacent pixels, both
 *     inside the tile and the frame, that differ by >= T in an 8-bit channel of P_f; output = S_f on refined tiles, P_f
 *     elsewhere.  One rounding only, never a mean of means.  Every output frame decides for itself.
 *   - T = 256 is the factor-1 shutter frame, bit for bit; T = 1 refines every tile whose P_f is not one colour.
 *   - A wave traces sample (0, 0) of its tile in each of the m sub-frames, decides on their rounded mean with one
 *     ballot, and traces the other m (k*k - 1) samples only when the tile is refined: nothing extra is traced for the
 *     decision, and no sub-frame and no sample reaches memory.
 *   - Bands: while in effect the band calls need band_rows % 8 == 0 or band_rows >= height, else RT_ERR_UNSUPPORTED
 *     before any device call (where the path threshold's band rule is checked).  Under rt_set_view_height a last tile
 *     row is cut at the rendered height, and so is its decision.
 *   - Bounds: shutter * k*k <= RT_MAX_SHUTTER, as without it.
 *   - Statistics: frames and pixels count output frames and pixels; with counting on, primary_rays grows by the
 *     traced output pixels x n_frames x m plus m (k*k - 1) per valid pixel of every refined tile, and reflect_rays /
 *     shadow_rays by those samples' rays, each sub-frame counting in its own view and scene; with counting off
 *     nothing grows.
 *   - rt_render_shutter and rt_render_anim_shutter go through the chunk pipeline unchanged: chunks count output
 *     frames.  Cost: see README "Adaptive shutters".  Single-GPU contexts only, as the calls themselves.
 * Returns RT_ERR_INVALID_ARG for a NULL ctx or out pointer, or a threshold outside 0..256. */
int rt_set_shutter_adaptive_sampling(rt_ctx* ctx, int threshold);
int rt_get_shutter_adaptive_sampling(const rt_ctx* ctx, int* out_threshold);
/* (ABI 10 addition) Progressive anti-aliasing for a display loop: k = 1 (the default, off), 2, 4 or 8.  While the
 * camera rests, each Tick call -- rt_render, rt_render_async, rt_render_device, and only these -- traces one more
 * sample per pixel and shows the mean so far; when anything of the view changes, the image is the plain frame again.
 * Sample order: with s = log2 k, sample n of 0 .. k*k - 1 is found from n's base-4 digits d_0 (least significant)
 * .. d_{s-1}: digit d_t gives bit s - 1 - t of the sample's column i from its bit 0, and bit s - 1 - t of its row j
 * from its bit 1.  k = 4: (i, j) = (0,0) (2,0) (0,2) (2,2) (1,0) (3,0) (1,2) (3,2) (0,1) (2,1) (0,3) (2,3) (1,1)
 * (3,1) (1,3) (3,3).  Sample (i, j) of output pixel (x, y) is the reference's pixel (k x + i, k y + j) of the
 * k width x k height frame, exactly as for rt_set_supersampling.
 * Output: P_c is, per 8-bit channel after ShiftColor, (sum of samples 0 .. c-1 + c/2) / c in integer arithmetic
 * (c/2 floors).  P_1 is the plain frame bit for bit, P_{k*k} is rt_set_supersampling(k)'s frame, and P_{4^t} is the
 * frame of rt_set_supersampling(2^t): the coarse sub-grids come first.
 * View key: the scene (any rt_set_scene makes a new one), the camera's five floats compared as bits, width, height
 * and the view height, k, and the number of band workers (a worker's accumulator follows its packed band set, which
 * no chunking changes).  The n-th consecutive Tick call whose key equals the previous Tick's outputs
 * P_min(n, k*k); any other Tick outputs P_1 and starts a new run.  rt_set_camera with unchanged values does not
 * restart; rt_reset_progressive forces a restart; a Tick that fails ends the run.  rt_render_async captures the
 * Tick's place in the run when it is queued, as it captures the camera.
 * rt_get_progressive returns the factor and the c of the last issued Tick frame (0 before any; 1 while k = 1).
 * Cost: a Tick that outputs P_1 runs exactly the launch the library runs without this call (a moving camera pays a
 * key compare on the host); the Tick for P_2 traces samples 0 and 1 in one launch and starts the accumulator
 * without reading it; the Ticks for P_3 .. P_{k*k} trace one sample per pixel; later Ticks trace nothing and emit
 * P_{k*k} from the accumulator.  Memory: 8 bytes per pixel of each worker's share, allocated at the first P_2 Tick,
 * freed by rt_set_progressive(ctx, 1) and rt_destroy.
 * Limits: while k > 1 a Tick with rt_set_supersampling also above 1 returns RT_ERR_UNSUPPORTED, and
 * (long long) k width * k height (the view height, when set) above 2^31 - 1 returns RT_ERR_INVALID_ARG.  The band,
 * batch, path, shutter and tile renders, rt_count_work and rt_debug_segments ignore the setting and do not disturb
 * a run.  Contexts of any n_gpus and flags: each worker accumulates its own share.
 * Statistics: frames and pixels count every Tick, launches the launches issued (a converged Tick's emit is one);
 * with counting on, primary_rays grows by the samples traced -- width * height, then twice that, then width *
 * height per Tick, then 0 -- and reflect_rays / shadow_rays by those samples' rays.
 * Returns RT_ERR_INVALID_ARG for a NULL ctx, a NULL out pointer or any other k. */
int rt_set_progressive(rt_ctx* ctx, int k);
int rt_get_progressive(const rt_ctx* ctx, int* out_k, int* out_samples);
int rt_reset_progressive(rt_ctx* ctx);
int rt_get_camera(const rt_ctx* ctx, rt_camera* camera);
int rt_camera_view(const rt_camera* camera, int width, int height, rt_view* out_view);
int rt_camera_on_key(rt_camera* camera, int key);
int rt_camera_on_mouse_move(rt_camera* camera, float delta_x, float delta_y);

/* ---- rendering (replaces Tick(), RayTracer.cs:886-935) ---------------------- */
/* Tick(): renders the full frame and copies it into the caller-owned host buffer
 * pixels[width*height] (Surface.pixels, 0x00RRGGBB, row-major y*width+x).
 * Synchronous: the pixels are complete on return, as template.cs:189-193 requires.
 * Every worker writes its own bands into `pixels` (registered: a copy kernel through the buffer's
 * device-mapped address, on large shares in chunks whose copies ride in the next chunk's trace
 * launch; unregistered: the runtime's copies). */
int rt_render(rt_ctx* ctx, int width, int height, int32_t* pixels);

/* Pin a caller-owned host buffer (hipHostRegister, mapped into every worker's device) so that the
 * Tick hand-off lands directly in it; the shim registers Surface.pixels once. */
int rt_register_host(rt_ctx* ctx, void* host_ptr, size_t bytes);
int rt_unregister_host(rt_ctx* ctx, void* host_ptr);

/* Device-resident variant: renders the frame into d_pixels[width*height] (device 0's memory) on
 * `hip_stream` (a hipStream_t of device 0; NULL = the HIP null stream, as everywhere in HIP) and
 * returns without synchronising.  n_gpus > 1: the workers' bands are gathered to device 0 over
 * RCCL/xGMI (RT_CREATE_SHARED_DEVICE: written straight into d_pixels), ordered after the work
 * already on hip_stream, and hip_stream waits for the frame. */
int rt_render_device(rt_ctx* ctx, int width, int height, int32_t* d_pixels, void* hip_stream);

/* Row-band shard (one process per GPU): renders the bands b = band_first,
 * band_first+band_step, ... of band_rows rows each (rows [b*band_rows, (b+1)*band_rows)
 * clipped to height) into d_out, packed band after band, each band width*band_rows
 * int32 (rows past the image are left untouched).  Returns the number of bands in
 * *out_n_bands when not NULL.  Asynchronous on hip_stream. */
int rt_render_bands(rt_ctx* ctx, int width, int height, int band_rows, int band_first,
                    int band_step, int32_t* d_out, void* hip_stream, int* out_n_bands);

/* Reassemble: copies n_bands packed bands (as written by rt_render_bands with the same
 * band_first/band_step) from d_bands into the row-major frame d_frame[width*height].
 * Asynchronous on hip_stream. */
int rt_scatter_bands(rt_ctx* ctx, int width, int height, int band_rows, int band_first,
                     int band_step, const int32_t* d_bands, int32_t* d_frame, void* hip_stream);

/* Band sets for shipping to rank 0.  Formats: RT_BANDS_INT32 (as
 * rt_render_bands) or RT_BANDS_RGB24 (3 bytes B, G, R per pixel: the top byte of
 * 0x00RRGGBB is always 0, so a quarter fewer bytes cross xGMI), or RT_BANDS_FRAME: the
 * bands straight into their rows of the row-major frame d_out[height][width] (other rows
 * untouched) -- rank 0's own share, which never travels. */
enum { RT_BANDS_INT32 = 0, RT_BANDS_RGB24 = 1, RT_BANDS_FRAME = 2 };
int rt_render_bands_ex(rt_ctx* ctx, int width, int height, int band_rows, int band_first,
                       int band_step, void* d_out, int format, void* hip_stream, int* out_n_bands);
/* n_frames frames of this rank's bands (the current camera, every frame traced in full) in
 * ONE launch: frame f's output at d_out + f * frame_stride_bytes, in `format`.  For the
 * multi-GPU pipeline, where a rank's share of a 1080p frame is a few microseconds of GPU work
 * and one launch per frame would leave the GPU waiting for the host. */
int rt_render_bands_batch(rt_ctx* ctx, int width, int height, int band_rows, int band_first,
                          int band_step, int n_frames, void* d_out, size_t frame_stride_bytes,
                          int format, void* hip_stream, int* out_n_bands);
/* (ABI 10 addition) Camera paths: one batch launch, one camera per frame -- an offline render of a camera
 * move (a fly-through, a turntable, a stereo pair, recorded input) at the batch launch's rate.
 * rt_render_path_bands: frame f = the frame rt_render_bands_ex would write with camera cameras[f] set:
 * this rank's bands of n_frames frames in ONE launch, frame f at (char*)d_out + f * frame_stride_bytes, in
 * `format` (RT_BANDS_INT32 / RGB24 / FRAME).  Asynchronous on hip_stream.
 *   - `cameras` is host memory, consumed before the call returns (the caller may reuse it at once).  The
 *     context's own camera (rt_set_camera) is neither read nor changed: a later rt_render renders it as ever.
 *   - rt_set_view_height applies to every frame, exactly as for rt_render_bands_batch.
 *   - Arguments are checked as rt_render_bands_batch checks them (single-GPU contexts only, band_rows > 0,
 *     frame_stride_bytes no smaller than a frame's output when n_frames > 1, ...); a NULL `cameras` or an
 *     n_frames <= 0 or above RT_MAX_PATH_FRAMES returns RT_ERR_INVALID_ARG.
 *   - With supersampling on (rt_set_supersampling, k > 1) both calls return RT_ERR_UNSUPPORTED.  Their own
 *     factor is rt_set_path_supersampling: with it above 1 every frame is box-filtered from k*k samples per pixel
 *     in the kernel, all arguments and the output stay in output pixels, and primary_rays counts samples.
 *   - Statistics: every frame has its own rays and counts for itself -- with rt_set_counting on,
 *     reflect_rays and shadow_rays grow by the sum over the frames and primary_rays by the traced pixels x
 *     n_frames; frames, pixels and launches behave as for rt_render_bands_batch.  With counting off the
 *     kernels count nothing (recommended for path renders that never read the counts: a counting path
 *     launch makes an atomic pair per wave per frame where the one-camera batch makes one per launch).
 *   - Path launches always run in natural tile order, one tile per workgroup: the lone-frame tuner
 *     (rt_dispatch_order) is not involved, even at n_frames == 1.
 * rt_render_path: whole frames into host memory, pixels[n_frames][height][width] (0x00RRGGBB).
 * Synchronous.  It traces into context-owned device buffers in launches of at most RT_PATH_CHUNK_FRAMES
 * frames (default: as many as keep a buffer at or below 256 MiB, at least 1; the environment variable of
 * that name, read at rt_create, overrides it) and copies each chunk out with hipMemcpyAsync on a second
 * stream.  Into a range registered through rt_register_host that copy is asynchronous: chunk c is copied
 * while chunk c + 1 traces.  Into any other memory the runtime stages the copy and the call blocks the host
 * until it is done, so the chunks are then traced and copied one after the other -- register `pixels` for
 * the overlap.  Whatever the call returns, no copy into `pixels` is still pending when it returns.
 * Memory: the frames' view records (2.5 KB each) pass through four table slots of pinned host and device
 * memory that the context keeps between calls; a slot that a long path grew (65,535 frames: about 165 MB
 * pinned and as much on the device) is cut back to the size of the next call that uses it when that call has
 * at most 256 frames, and everything is released by rt_destroy. */
#define RT_MAX_PATH_FRAMES 65535   /* grid z */
int rt_render_path_bands(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int n_frames,
                         int band_rows, int band_first, int band_step, void* d_out,
                         size_t frame_stride_bytes, int format, void* hip_stream, int* out_n_bands);
int rt_render_path(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int n_frames,
                   int32_t* pixels);
/* (ABI 10 addition) Camera-path shutter: every output frame is the mean of `shutter` sub-frame cameras, taken
 * inside the trace kernel -- motion blur, or temporal anti-aliasing by jittered cameras, at no extra output.
 * `cameras` has n_frames * shutter entries; sub-frame (f, s) is the frame rt_render_bands_ex would write with
 * cameras[f * shutter + s] set, and output frame f is, per 8-bit channel and after ShiftColor, the round-half-up
 * mean of its sub-frames: (sum + shutter / 2) >> log2(shutter).  A wave traces its tile once per sub-frame and
 * keeps the running sums in registers: no sub-frame reaches memory, and the output keeps a path render's size.
 *   - shutter is a power of two in 1..RT_MAX_SHUTTER, and n_frames * shutter <= RT_MAX_PATH_FRAMES; otherwise
 *     RT_ERR_INVALID_ARG.  shutter == 1 is rt_render_path_bands / rt_render_path itself (the same launches).
 *   - Everything else is as for the path calls: formats, frame_stride_bytes, rt_set_view_height, the context's
 *     camera left alone, natural tile order, single-GPU contexts only, RT_ERR_UNSUPPORTED while supersampling
 *     (rt_set_supersampling above 1).
 *   - rt_set_path_supersampling(k) applies: the output is the one round-half-up mean over the shutter's sub-frames
 *     and each pixel's k*k samples, and shutter * k*k must not exceed RT_MAX_SHUTTER (RT_ERR_INVALID_ARG).
 *     rt_set_shutter_adaptive_sampling(T) then supersamples only the 8x8 tiles whose shutter frame has edges.
 *   - Statistics: frames and pixels count output frames and pixels, launches one per launch; with counting on,
 *     primary_rays grows by the traced pixels x n_frames x shutter and reflect_rays / shadow_rays by the sum
 *     over every sub-frame (each sub-frame counts for itself); with counting off nothing grows.
 * rt_render_shutter: whole output frames into host memory, pixels[n_frames][height][width], synchronous, through
 * rt_render_path's chunk pipeline: RT_PATH_CHUNK_FRAMES and the 256 MiB rule count output frames, and a
 * chunk's view table holds chunk * shutter records. */
#define RT_MAX_SHUTTER 256   /* 256 * 255 + 128 = 65,408 < 65,536: a channel's sum fits a 16-bit field */
int rt_render_shutter_bands(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int n_frames,
                            int shutter, int band_rows, int band_first, int band_step, void* d_out,
                            size_t frame_stride_bytes, int format, void* hip_stream, int* out_n_bands);
int rt_render_shutter(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int n_frames,
                      int shutter, int32_t* pixels);
/* Animated scenes: one batch launch, one scene and one camera per frame (ABI 10).
 *
 * A scene track is n_frames scene images in device memory.  rt_set_scene_track builds frame f's image from exactly
 * the arguments rt_set_scene would get for that frame -- spheres[f * n_spheres + i], planes[f * n_planes + j],
 * lights[f * n_lights + k], ambients[f]; the counts and the recursion limit are those of every frame -- with the
 * same RT_* switches, and uploads the images back to back.  It replaces an earlier track, after waiting for the
 * launches that may still read it.  The context's own scene, camera, view cache and progressive run are not
 * touched: every other render behaves as before.  rt_clear_scene_track frees the track (rt_destroy does too).
 *
 * rt_render_anim_bands is rt_render_path_bands with output frame j rendered from track frame first_frame + j and
 * cameras[j]: bit for bit the frame rt_set_scene(scene first_frame + j), rt_set_camera(cameras[j]) and
 * rt_render_bands_ex write.  Asynchronous on hip_stream, every format.  rt_render_anim writes whole frames into
 * host memory through rt_render_path's chunk pipeline.
 *
 * Refusals, each before any device call and in this order.  rt_set_scene_track: a NULL context or array
 * (RT_ERR_INVALID_ARG); n_frames outside 1..RT_MAX_PATH_FRAMES (RT_ERR_INVALID_ARG); counts, limit or lights beyond
 * rt_set_scene's bounds (its codes); a track above RT_MAX_TRACK_BYTES (RT_ERR_OOM); frames whose cluster counts
 * differ (RT_ERR_UNSUPPORTED; the builders give equal counts for equal sphere counts).  The renders: a NULL context
 * or cameras, n_frames outside 1..RT_MAX_PATH_FRAMES (RT_ERR_INVALID_ARG); no track (RT_ERR_NO_SCENE); a bad frame
 * size, first_frame < 0 or first_frame + n_frames beyond the track (RT_ERR_INVALID_ARG); a context with more than
 * one worker (RT_ERR_INVALID_ARG); supersampling above 1 (RT_ERR_UNSUPPORTED); a sample frame above 2^31 - 1 under
 * rt_set_path_supersampling (RT_ERR_INVALID_ARG).  Adaptive and progressive settings are ignored, as the path calls
 * ignore them; rt_set_path_supersampling and rt_set_path_adaptive_sampling apply as they do to them, each frame's
 * samples traced, and each frame's tiles decided, in that frame's scene.
 * Frames with a light at the origin, or with a general specular exponent, may be mixed with frames without: the
 * launch takes the kernels that are exact for every light and every exponent. */
#define RT_MAX_TRACK_BYTES ((size_t)1 << 30)
int rt_set_scene_track(rt_ctx* ctx, const rt_sphere* spheres, int n_spheres, const rt_plane* planes, int n_planes,
                       const rt_light* lights, int n_lights, const rt_vec3* ambients, int recursion_limit,
                       int n_frames);
int rt_clear_scene_track(rt_ctx* ctx);
int rt_render_anim_bands(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int first_frame,
                         int n_frames, int band_rows, int band_first, int band_step, void* d_out,
                         size_t frame_stride_bytes, int format, void* hip_stream, int* out_n_bands);
int rt_render_anim(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int first_frame, int n_frames,
                   int32_t* pixels);
/* (ABI 10 addition) Scene-track shutter: the shutter of rt_render_shutter[_bands] over a scene track, so that a
 * moving object, a moving light and a moving camera blur alike.  Every output frame is the mean of `shutter`
 * sub-frames, each with its own scene and its own camera, taken inside the trace kernel: `cameras` has n_frames *
 * shutter entries, and sub-frame (f, s) is, bit for bit, the frame rt_render_anim_bands writes for track frame
 * first_frame + f * shutter + s seen from cameras[f * shutter + s].  Output frame f is, per 8-bit channel and after
 * ShiftColor, (sum + shutter / 2) >> log2(shutter) over its sub-frames.  first_frame need not be a multiple of
 * shutter.  No sub-frame reaches memory and the output keeps a track render's size.
 *   - shutter == 1 is rt_render_anim_bands / rt_render_anim itself: the same launches, kernels and bytes.
 *   - rt_set_path_supersampling(k) applies as it does to rt_render_shutter*: one rounding (sum + m k*k / 2) >>
 *     (log2 m + 2 log2 k) per channel over the m sub-frames and each pixel's k*k samples, and m * k*k must not
 *     exceed RT_MAX_SHUTTER.
 *   - With rt_set_path_adaptive_sampling in effect (a threshold, k > 1) and shutter > 1 the calls return
 *     RT_ERR_UNSUPPORTED and write nothing, as the camera shutter does -- while rt_set_shutter_adaptive_sampling's
 *     threshold is 0; with it set they render adaptively at that threshold, each sub-frame in its own scene.
 *   - Refusals, each before any device call and in this order.  First those of rt_render_anim*, in their order
 *     above, with the track bound being first_frame + n_frames * shutter <= the track's frames: a NULL context or
 *     cameras, n_frames outside 1..RT_MAX_PATH_FRAMES (RT_ERR_INVALID_ARG); no track (RT_ERR_NO_SCENE); a bad frame
 *     size, first_frame < 0 or sub-frames beyond the track (RT_ERR_INVALID_ARG); a context with more than one
 *     worker (RT_ERR_INVALID_ARG); rt_set_supersampling above 1 (RT_ERR_UNSUPPORTED); a sample frame above 2^31 - 1
 *     (RT_ERR_INVALID_ARG).  Then the shutter's: shutter not a power of two in 1..RT_MAX_SHUTTER
 *     (RT_ERR_INVALID_ARG); n_frames * shutter above RT_MAX_PATH_FRAMES (RT_ERR_INVALID_ARG); shutter * k*k above
 *     RT_MAX_SHUTTER (RT_ERR_INVALID_ARG); the adaptive refusal (RT_ERR_UNSUPPORTED).  Then the band arguments, the
 *     frame stride and a NULL pixels, as for rt_render_anim*.
 *   - Everything else is as for the track calls: formats, frame_stride_bytes, rt_set_view_height, natural tile
 *     order, single-GPU contexts only; the context's own scene, camera and progressive run stay untouched.
 *   - Statistics follow the shutter's rules, each sub-frame counting for itself in its own scene: frames and pixels
 *     count output frames and pixels; with counting on, primary_rays grows by the traced pixels x n_frames x shutter
 *     x k*k and reflect_rays / shadow_rays by the sum over every sub-frame; with counting off nothing grows.
 * rt_render_anim_shutter: whole output frames into host memory, pixels[n_frames][height][width], synchronous,
 * through rt_render_path's chunk pipeline: chunks count output frames, and a chunk of nf output frames from output
 * frame f0 takes its cameras from cameras[f0 * shutter] and its track frames from first_frame + f0 * shutter. */
int rt_render_anim_shutter_bands(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int first_frame,
                                 int n_frames, int shutter, int band_rows, int band_first, int band_step,
                                 void* d_out, size_t frame_stride_bytes, int format, void* hip_stream,
                                 int* out_n_bands);
int rt_render_anim_shutter(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int first_frame,
                           int n_frames, int shutter, int32_t* pixels);
/* Reassemble the band sets of `world` ranks (band b rendered by rank b % world with
 * band_first = rank, band_step = world), gathered rank after rank at slot_bytes intervals
 * in d_gathered, into the row-major frame d_frame[height][width] -- one launch for all
 * ranks (rank 0's side of the RCCL gather). */
int rt_scatter_gathered(rt_ctx* ctx, int width, int height, int band_rows, int world,
                        const void* d_gathered, size_t slot_bytes, int format, int32_t* d_frame,
                        void* hip_stream);

/* ---- tile codec for the gather to rank 0 (ABI 4, format 2 since ABI 6) --
 * Lossless: each rank encodes its int32 band sets (as rt_render_bands writes them, the
 * slot of the largest band set per frame) into a "wire" -- per 8x8 tile a 4-byte header (raw
 * first pixel, width code), second-difference (gradient) prediction, zigzag residuals packed
 * at 0/2/3/4/6/8 bits per channel -- and rank 0 decodes all ranks' wires straight into the
 * frames.  Rendered frames are mostly flat, so the wire is ~8-13x smaller than RGB24 at 1080p
 * (DESIGN.md 1e); the format is specified in raytracer_hip/tilecodec.py.  The wire's size
 * varies: the fixed part (header, tile headers, chunk bases) is the same on every rank, the
 * payload follows it. */
typedef struct rt_wire_layout {
    uint64_t fixed_bytes;  /* header + tile headers + chunk bases (8-aligned)          */
    uint64_t max_bytes;    /* fixed_bytes + the largest possible payload (capacity)     */
    int32_t tiles_x, tiles_y, tiles_per_frame, n_frames, n_tiles, n_chunks;
} rt_wire_layout;
/* Sizes of one rank's wire for n_frames frames (the same for every rank of `world`). */
int rt_wire_layout_of(int width, int height, int band_rows, int world, int n_frames, rt_wire_layout* out);
/* Encode n_frames band sets of `rank` (frame f at d_bands + f * frame_stride int32, each
 * at least the largest band set: bands_of(height, band_rows, 0, world) * band_rows * width)
 * into d_wire (8-aligned, max_bytes capacity).  *d_wire_bytes (device int64, may be NULL)
 * receives the wire's size in bytes.  Three launches, asynchronous on hip_stream. */
int rt_encode_bands(rt_ctx* ctx, int width, int height, int band_rows, int rank, int world,
                    const int32_t* d_bands, size_t frame_stride, int n_frames, void* d_wire,
                    int64_t* d_wire_bytes, void* hip_stream);
/* Decode the wires of ranks first_rank .. world-1 (rank r's at d_gathered + r * rank_stride,
 * 8-aligned; each region at least max_bytes) into frame f = d_frames + f * frame_stride
 * (int32, row-major) for f < n_frames: only those ranks' rows are written (first_rank = 1:
 * rank 0 rendered its own rows with RT_BANDS_FRAME).  One launch, asynchronous on hip_stream. */
int rt_decode_gathered(rt_ctx* ctx, int width, int height, int band_rows, int world, int first_rank,
                       const void* d_gathered, size_t rank_stride, int n_frames, int32_t* d_frames,
                       size_t frame_stride, void* hip_stream);
/* The encoder fused into the trace (ABI 6): trace frames frame0 .. frame0+n_frames-1 of a batch
 * of batch_frames of `rank`'s bands straight into d_wire's tile headers and the context's codec
 * scratch -- the band set never reaches HBM -- then rt_finish_wire turns the batch's first
 * n_frames (<= batch_frames) into the same wire rt_encode_bands would have made of the band sets
 * (byte for byte).  A batch may take several rt_render_bands_tiles calls; the context's scratch
 * holds one batch at a time (stream-ordered, like rt_encode_bands').  Asynchronous on hip_stream. */
int rt_render_bands_tiles(rt_ctx* ctx, int width, int height, int band_rows, int rank, int world,
                          int frame0, int n_frames, int batch_frames, void* d_wire, void* hip_stream);
int rt_finish_wire(rt_ctx* ctx, int width, int height, int band_rows, int rank, int world, int n_frames,
                   void* d_wire, int64_t* d_wire_bytes, void* hip_stream);

/* ---- one-process-per-GPU collectives on the trace stream (ABI 7) ---------------- */
/* The N > 1 tile pipeline's two exchange steps -- the all_reduce(MAX) of the wire sizes and the
 * gather of every rank's wire to rank 0 (the reference's only parallel loop is
 * RayTracer.cs:898-901) -- issued by the library itself on the caller's HIP stream, the stream
 * that traced and encoded the batch and that decodes it, so the exchange adds no cross-stream
 * hops (a torch.distributed collective runs on its own stream: a wait into it and one out of it,
 * ~20 us each in profiles/r03_dist_stages.txt).  The communicator is RCCL (the instance already
 * loaded in the process when there is one), one rank per process and device:
 *   rank 0: rt_comm_unique_id(id); share the RT_COMM_ID_BYTES with every rank (e.g. a broadcast);
 *   every rank: rt_comm_init(ctx, world, rank, id)          -- collective, on ctx's device. */
#define RT_COMM_ID_BYTES 128
/* (ABI 8) RT_OK when a librccl with every symbol the rt_comm_* calls use can be loaded in this
 * process; no communicator, socket or thread is created.  Ranks agree on the result (e.g. an
 * all_reduce(MIN)) before any of them starts rt_comm_init, which is collective: a rank that could
 * not join would leave the others blocked inside it. */
int rt_comm_probe(void);
int rt_comm_unique_id(void* out_id);
int rt_comm_init(rt_ctx* ctx, int world, int rank, const void* id);
/* In place, count int64 values on the device: every rank ends with the element-wise maximum. */
int rt_comm_allreduce_max_i64(rt_ctx* ctx, int64_t* d_values, int count, void* hip_stream);
/* Gather n_bytes from every rank's d_send to rank 0: rank r's bytes land at
 * d_recv + ((r - rotate) mod world) * recv_stride (rank 0 only; its own by a device copy).
 * Collective; n_bytes must be the same on every rank (0: nothing moves). */
int rt_comm_gather(rt_ctx* ctx, const void* d_send, size_t n_bytes, void* d_recv, size_t recv_stride, int rotate,
                   void* hip_stream);

/* ---- double-buffered frames ------------------------------ */
/* Asynchronous Tick(): captures the current camera, enqueues the trace and its hand-off into `pixels`
 * and returns; rt_wait blocks until every enqueued frame is in its host buffer.  With two host buffers
 * a caller overlaps the trace of frame k+1 with its own use of frame k (the camera of k+1 can already
 * be set).  Each worker double-buffers its band set in device memory: frame k's copy into `pixels`
 * runs on the copy engine on a second stream behind frame k's trace (registered `pixels`; a share
 * under 0.5 Mpixel at n_gpus > 1 rides instead as a copy slice in frame k+1's trace launch, and an
 * unregistered buffer gets the runtime's copies), while frame k+1 is traced.  At most 2 frames per
 * worker are in flight: the call for frame k+2 first waits on the host for frame k's copy (deeper
 * queues made the runtime block one copy call for 6-7 ms now and then, profiles/r06_tick_deep.txt;
 * RT_TICK_INFLIGHT overrides).  Measured on one MI355X (bench.py tick_*, C3 1080p, median of 3 x 20
 * frames): two frames deep with an rt_wait per pair 5.1-5.2k fps, 20 frames queued with one rt_wait
 * 5.7-5.8k fps, against 4.8k for the synchronous rt_render.  n_gpus > 1: every worker double-buffers
 * its own band set on its own streams and device (ABI 9; RT_CREATE_RCCL_GATHER contexts render
 * synchronously here). */
int rt_render_async(rt_ctx* ctx, int width, int height, int32_t* pixels);
int rt_wait(rt_ctx* ctx);

/* ---- headless display hand-off --------------------------- */
/* Writes pixels (0x00RRGGBB, row-major) as a binary PPM (P6).  Host only, no context. */
int rt_write_ppm(const char* path, const int32_t* pixels, int width, int height);

/* ---- debug ray view (RayTracer.cs:423-435, :903-934) ------- */
/* The reference's DEBUG_ENABLE view logs traced rays and draws 500 random ones as lines
 * (red primary, green secondary, blue shadow) into the lower-right 30 % inset.  Here the
 * pixels y*width+x with (y*width+x) % sample_stride == 0 are traced again and every segment
 * of their visible path is appended to out[] (at most `capacity`; *out_count receives the
 * total): primary/secondary segments end at the winning hit point (origin + 100*dir when
 * nothing is hit); shadow segments start at the shaded point with the light POSITION as
 * direction (Q2) and end at the first blocker's distance, or at t = 1 when unblocked.
 * Synchronous.  Composited on the host by raytracer_hip.debugview. */
typedef struct rt_segment {
    rt_vec3 origin;
    rt_vec3 end;
    int32_t kind;   /* 0 primary, 1 secondary (reflected), 2 shadow -- RayKind, :343-361 */
    int32_t pixel;  /* y*width + x */
} rt_segment;

int rt_debug_segments(rt_ctx* ctx, int width, int height, int sample_stride, rt_segment* out,
                      int capacity, int* out_count);

/* ---- hit buffers and picking (ABI 10 additions) -------------------------------- */
/* What a pixel sees besides its colour: per pixel, the hit that the primary ray selects by TracePixel's rule
 * (RayTracer.cs:973-993: the nearest sphere with t > 0 in scene order, the nearest plane likewise, the sphere iff
 * its t is below the plane's).  Written by a primary-only kernel -- no shading, no shadow ray, no reflection.
 *   depth     the selected primitive's IntersectResult.distance t            | nothing selected: +inf
 *   object    sphere i -> i, plane j -> n_spheres + j                        | RT_HIT_NONE
 *   position  origin + direction * t                                         | origin + direction * 100 (as
 *                                                                              rt_debug_segments' segment end)
 *   normal    sphere: Normalize(position - center); plane: its normal as set | (0, 0, 0)
 * The values are bit for bit the reference's binary32 ones.  A selected hit with t - 0.01 <= 0, which the colour
 * frame renders black (:731, :839), is still the selected hit and is reported like any other.
 *   - The buffers are those of the plain frame's rays: rt_set_supersampling, rt_set_path_supersampling, every
 *     adaptive threshold and rt_set_progressive are ignored (sample (0, 0) of each block, as rt_debug_segments), and a
 *     hit call leaves a progressive run as it is.  rt_set_view_height applies exactly as to rt_render_device.
 *   - Hit calls add nothing to rt_get_stats (no frames, pixels, launches or rays), do not read rt_set_counting and
 *     never involve the lone-frame tuner (rt_dispatch_order).
 *   - Any channel pointer may be NULL: that channel is not written.  All NULL, or a NULL rt_hit_buffers:
 *     RT_ERR_INVALID_ARG.  Each channel is [n_frames][height][width], frame f at element f * width * height.
 *   - rt_render_hits_device: the context's camera and scene, asynchronous on hip_stream.  rt_render_path_hits_device:
 *     frame f seen from cameras[f], as rt_render_path_bands -- ONE launch; cameras, n_frames and the frame size are
 *     checked as there, `cameras` is consumed before the call returns and the context's camera is neither read nor
 *     changed.  rt_render_anim_hits_device: frame f is track frame first_frame + f seen from cameras[f], as
 *     rt_render_anim_bands, with its checks of cameras, n_frames, first_frame and the track.
 *   - rt_render_hits, rt_render_path_hits, rt_render_anim_hits: the same into host memory, synchronous.  They trace
 *     into a context-owned device buffer in chunks of as many frames as keep it at or below 256 MiB (at least one)
 *     and copy each chunk out before the next; rt_destroy releases the buffer.
 *   - rt_pick: the four values the buffers hold at pixel (x, y) of the context camera's width x height frame, from a
 *     one-wave launch and a 32-byte copy.  Synchronous.  x or y outside the frame: RT_ERR_INVALID_ARG.
 *   - Contexts with more than one worker (RT_CREATE_SHARED_DEVICE ones included) return RT_ERR_UNSUPPORTED before any
 *     device call. */
#define RT_HIT_NONE (-1)
typedef struct rt_hit_buffers {
    float*   depth;
    int32_t* object;
    rt_vec3* position;
    rt_vec3* normal;
} rt_hit_buffers;
typedef struct rt_pick_result {
    int32_t object;
    float depth;
    rt_vec3 position;
    rt_vec3 normal;
} rt_pick_result;
int rt_render_hits_device(rt_ctx* ctx, int width, int height, const rt_hit_buffers* d_out, void* hip_stream);
int rt_render_path_hits_device(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int n_frames,
                               const rt_hit_buffers* d_out, void* hip_stream);
int rt_render_anim_hits_device(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int first_frame,
                               int n_frames, const rt_hit_buffers* d_out, void* hip_stream);
int rt_render_hits(rt_ctx* ctx, int width, int height, const rt_hit_buffers* out);
int rt_render_path_hits(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int n_frames,
                        const rt_hit_buffers* out);
int rt_render_anim_hits(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int first_frame, int n_frames,
                        const rt_hit_buffers* out);
int rt_pick(rt_ctx* ctx, int width, int height, int x, int y, rt_pick_result* out);

/* ---- statistics ------------------------------------------------------------- */
/* Synchronises the context's pending work, then returns the counters. */
/* Device timing of trace launches, copies and gathers with HIP event pairs: every
 * `every`-th operation of each kind is timed (the first one always), 0 = none.  Default 64:
 * an event pair costs several microseconds of GPU time, 17 % of a 1080p frame if every
 * frame were timed.  Counters (rays) are always exact (for the launches that count, rt_set_counting). */
int rt_set_timing(rt_ctx* ctx, int every);
/* Dispatch order of single-frame launches (rt_render, rt_render_device on scenes with fewer than
 * 12 spheres): the order in which the kernel's tiles start, which sets a lone frame's tail.  The
 * first launches of a scene and frame size time each candidate (0 tile rows by decreasing estimated
 * cost, 1 rows bottom to top, 2 rows varying fastest, 3 every tile by decreasing measured duration --
 * the round's first launch records each tile's duration) and keep the fastest; the pixels are the same
 * under every order.  *out_order: the candidate in use, -1 while still measuring (ABI 8 addition;
 * RT_DISPATCH_ORDER=0/1/2/3 in the environment at rt_create fixes it).  The choice is measured again
 * every 16,384 single-frame launches; candidate 3's tile durations are recorded again once the camera
 * has moved and 256 launches have used them (one device synchronisation per recording). */
int rt_dispatch_order(rt_ctx* ctx, int* out_order);
int rt_get_stats(rt_ctx* ctx, rt_stats* out_stats);
int rt_reset_stats(rt_ctx* ctx);
/* ABI 10.  on = 1 (the default): every trace launch adds its rays to the counters above (frame 0 of a
 * batch launch counts for all its frames; one device atomic pair per wave).  on = 0: the kernels count
 * nothing -- the display loop's setting, since the reference's Tick counts nothing and in a one-frame
 * launch every wave's atomics cost the frame 8-13 % (1080p; 4 % at 4K).  Launches made with counting
 * off still add to frames, pixels and launches, not to primary_rays (= the pixels of counted launches)
 * nor to the other ray and test counts.  Returns RT_ERR_INVALID_ARG unless on is 0 or 1. */
int rt_set_counting(rt_ctx* ctx, int on);
/* Traces one width x height frame of the current camera with the diagnostic kernels (same
 * pixels, plus executed-work tallies) into a context-owned buffer and returns its work.
 * Synchronous; single-GPU contexts; does not touch rt_get_stats' counters. */
int rt_count_work(rt_ctx* ctx, int width, int height, rt_work* out_work);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RAYTRACER_HIP_H */
