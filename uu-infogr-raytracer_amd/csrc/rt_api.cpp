// rt_api.cpp -- C ABI of libraytracer_hip (include/raytracer_hip.h).
//
// Host side of the drop-in: context lifetime, scene upload (with the scene-constant
// precomputation described in rt_internal.h), camera math (RayTracer.cs:511-523,
// :543-554, :892-896, :1058-1061), frame rendering (single GPU, row bands, and the
// single-process multi-GPU Tick: every device traces its interleaved row bands and hands
// them to the caller's Surface.pixels over its own PCIe link; device-resident frames are
// gathered to device 0 over RCCL/xGMI), HIP-event timing and work counters.  Never throws
// across the ABI; no CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <link.h>
#include <new>
#include <string>
#include <vector>

#include "../../include/raytracer_hip.h"
#include "rt_bands.h"
#include "rt_internal.h"
#include "rt_progressive.h"
#include "rt_scene.h"
#include "rt_view.h"

using namespace rtk;

// ----------------------------------------------------------------------------
// minimal RCCL binding (resolved with dlopen only for multi-GPU contexts, so a
// single-GPU process never needs librccl)
// ----------------------------------------------------------------------------
namespace {
typedef void* ncclComm_t;
typedef int ncclResult_t;
enum { ncclUint8 = 1, ncclInt32 = 2, ncclInt64 = 4 };
enum { ncclMax = 2 };
struct ncclUniqueId {
    char internal[RT_COMM_ID_BYTES];
};
// The librccl already mapped into the process (torch's, in a torch.distributed job), so that our
// communicator and the framework's share one RCCL instance; else the first that dlopen finds.
// Only the library itself: its basename is "librccl.so" or "librccl.so.<version>" (RCCL's net and
// tuner plugins, e.g. librccl-net.so, also contain "librccl" but lack the nccl* entry points).
bool is_librccl(const char* path) {
    const char* base = std::strrchr(path, '/');
    base = base ? base + 1 : path;
    if (std::strncmp(base, "librccl.so", 10) != 0) return false;
    for (const char* p = base + 10; *p; ++p)
        if (!(*p == '.' || (*p >= '0' && *p <= '9'))) return false;
    return true;
}
int find_loaded_rccl(struct dl_phdr_info* info, size_t, void* out) {
    if (info->dlpi_name && is_librccl(info->dlpi_name)) {
        *(std::string*)out = info->dlpi_name;
        return 1;
    }
    return 0;
}
struct Rccl {
    void* h = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Gather)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool load(std::string& err) {
        if (h) return true;
        std::string loaded;
        dl_iterate_phdr(find_loaded_rccl, &loaded);
        if (!loaded.empty()) h = dlopen(loaded.c_str(), RTLD_NOW | RTLD_NOLOAD);
        // RTLD_LOCAL: a RCCL loaded here must not interpose on one the process loads later (torch's own
        // librccl, pulled in by an `import torch` after our first RCCL context): with RTLD_GLOBAL the two
        // copies shared symbols and the process aborted at exit ("double free or corruption (!prev)", r05b) --
        // the one cause, profiles/r06_exit_abort.txt (RCCL then `import torch` aborts under RTLD_GLOBAL only)
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names)
            if (!h && (h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) {
            err = "dlopen(librccl) failed";
            return false;
        }
        CommInitAll = (decltype(CommInitAll))dlsym(h, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(h, "ncclCommDestroy");
        Gather = (decltype(Gather))dlsym(h, "ncclGather");
        GroupStart = (decltype(GroupStart))dlsym(h, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(h, "ncclGroupEnd");
        GetUniqueId = (decltype(GetUniqueId))dlsym(h, "ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))dlsym(h, "ncclCommInitRank");
        AllReduce = (decltype(AllReduce))dlsym(h, "ncclAllReduce");
        Send = (decltype(Send))dlsym(h, "ncclSend");
        Recv = (decltype(Recv))dlsym(h, "ncclRecv");
        GetErrorString = (decltype(GetErrorString))dlsym(h, "ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !Gather || !GroupStart || !GroupEnd || !GetUniqueId || !CommInitRank ||
            !AllReduce || !Send || !Recv) {
            err = "librccl lacks a symbol (ncclCommInitAll/InitRank/GetUniqueId/Gather/AllReduce/Send/Recv/Group*)";
            return false;
        }
        return true;
    }
};
Rccl g_rccl;

thread_local std::string g_last_error;

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    int kind = 0;  // 0 kernel, 1 copy, 2 gather
};

struct Device {
    int id = 0;
    hipStream_t stream = nullptr;
    void* d_scene = nullptr;
    size_t scene_cap = 0;
    int32_t* d_frame = nullptr;  // full frame (device 0 of multi-GPU contexts)
    size_t frame_cap = 0;
    int32_t* d_bands = nullptr;  // this device's packed row bands (multi-GPU)
    size_t bands_cap = 0;
    int32_t* d_gather = nullptr;  // device 0: n_gpus x padded band sets
    size_t gather_cap = 0;
    void* d_stage = nullptr;  // rt_encode_bands scratch (encodes on one context are stream-ordered)
    size_t stage_cap = 0;
    // the batch whose tiles rt_render_bands_tiles last staged in d_stage (rt_finish_wire finishes only
    // that one; rt_encode_bands reuses the scratch and clears it)
    struct {
        bool valid = false;
        int W = 0, H = 0, band_rows = 0, rank = 0, world = 0, batch_frames = 0;
        const void* wire = nullptr;
    } staged;
    int32_t* d_frames2[2] = {nullptr, nullptr};  // rt_render_async double buffer (this device's band set)
    size_t frames2_cap[2] = {0, 0};
    // rt_render_async: one in-order stream per device; frame k's D2H rides in frame k+1's launch (the
    // copy slice, LaunchParams::copy) or is issued by rt_wait -- `hand` is that pending copy
    hipStream_t async_stream = nullptr;
    struct {
        int32_t* host = nullptr;  // caller's buffer (one contiguous band set: hipMemcpyAsync on a flush)
        CopyJob job{};            // the band set -> the buffer's device-mapped address (job.words 0: none)
    } hand;
    // the copy-engine hand-off of chunk c (trace_and_copy_chunks) on its own stream, after the chunk's trace
    hipStream_t copy_stream = nullptr;
    bool copy_pending[2] = {false, false};  // rt_render_async, RT_TICK_ASYNC=stream: slot s has a copy queued
    static constexpr int RING = 16;
    // The worker's plain events, made on first use (ensure_event) and destroyed in one loop by rt_destroy.
    enum Ev {
        EV_JOIN,                              // rt_render_device at n > 1: ordering against the caller's stream
        EV_CHUNK,                             // [8] chunk c of a copy-engine hand-off traced
        EV_COPIED = EV_CHUNK + 8,             // [2] rt_render_async's copy-engine hand-off: slot s copied
        EV_RING = EV_COPIED + 2,              // [RING] frames in flight of that hand-off (rt_ctx::tick_inflight):
                                              // frame f's copy done -> EV_RING + f % RING
        EV_PATH_TRACED = EV_RING + RING,      // [2] rt_render_path: d_path[b] traced,
        EV_PATH_COPIED = EV_PATH_TRACED + 2,  // [2] copied
        EV_PROG = EV_PATH_COPIED + 2,         // the last launch that touched the progressive accumulator (d_prog)
        EV_COUNT = EV_PROG + 1
    };
    hipEvent_t ev[EV_COUNT] = {};
    uint64_t frames_issued = 0;
    // Camera-path launches (rt_render_path_bands): the frames' DevView records go through a ring of table slots
    // -- pinned staging, hipMemcpyAsync on the caller's stream ahead of the launch, an event after it; a slot is
    // reused only once its event has completed (waited for on the host), so back-to-back calls on any streams
    // never overwrite records a queued launch still reads.
    static constexpr int PATH_SLOTS = 4;
    static constexpr size_t PATH_SLOT_KEEP = 256;  // DevView records (643 KB) a slot retains between calls
    struct PathSlot {
        DevView* h_views = nullptr;  // pinned
        DevView* d_views = nullptr;
        size_t cap = 0;              // frames
        hipEvent_t done = nullptr;   // after the slot's last launch
        bool busy = false;
    } path_slot[PATH_SLOTS];
    unsigned path_next = 0;
    // rt_render_path: chunk c is traced into d_path[c % 2] (stream) and copied out by the copy engine
    // (copy_stream) under the trace of chunk c + 1
    int32_t* d_path[2] = {nullptr, nullptr};
    size_t path_cap[2] = {0, 0};
    // rt_set_progressive: this worker's accumulator, one ResolveSum per pixel of its packed band set (bands g, g + n,
    // ... of TICK_BAND_ROWS rows; one worker: the frame), made at the first Tick that accumulates.  Only PROG trace
    // launches touch it, in issue order: a Tick on another stream than the last one's (rt_render_device on the
    // caller's, rt_render_async on the async stream) first waits for EV_PROG.
    ResolveSum* d_prog = nullptr;
    size_t prog_cap = 0;
    hipStream_t prog_stream = nullptr;
    bool prog_touched = false;
    // rt_set_scene_track: the track's scene images, back to back (worker 0 only: the anim renders are single-worker)
    void* d_track = nullptr;
    size_t track_cap = 0;
    // rt_render_hits / _path_hits / _anim_hits: a chunk's requested channels, one after the other (hits_host);
    // rt_pick: its one record
    void* d_hits = nullptr;
    size_t hits_cap = 0;
    DevPick* d_pick = nullptr;
    float* d_view_tab = nullptr;  // lx[W] then ly[H] (view_tables)
    size_t view_tab_cap = 0;
    int tab_w = -1, tab_h = -1;
    float tab_pw = 0, tab_ph = 0;
    int async_next = 0;
    unsigned long long* d_counters = nullptr;
    unsigned long long* d_counters_diag = nullptr;  // rt_count_work
    std::vector<EventPair> pending, pool;
    uint64_t op_count[3] = {0, 0, 0};  // operations per timing kind (sampling phase)
    // Dispatch order of single-frame launches (order_pick): which of the ORDER_CANDIDATES the direct
    // kernel's workgroups follow, chosen by timing a few launches of each for the current scene and
    // frame size.  Every order traces the same tiles the same way: only their start order differs.
    struct OrderTuner {
        int chosen = -1;           // -1: measuring
        int turn = 0;              // next candidate to measure
        int W = 0, H = 0;          // frame size and scene generation the measurements belong to
        uint64_t scene_gen = 0, gen = 0;
        uint64_t since = 0;        // single-frame launches since the choice (re-measured every ORDER_RETUNE)
        std::vector<float> ms[4];
        // candidate 3: the tiles in decreasing order of their measured duration (the first single-frame
        // launch of a measuring round records every tile's duration; tile_order_prepare)
        struct Tiles {
            int W = 0, H = 0;
            uint64_t gen = 0, scene_gen = 0;
            bool recorded = false, built = false;
            rt_camera cam{};         // the camera of the recorded durations
            uint64_t uses = 0;       // candidate-3 launches since they were recorded
            uint32_t* d_order = nullptr;  // padded to SINGLE_WPG (ty = 0xffff past the last tile)
            uint32_t* d_cost = nullptr;   // RTC ticks per tile
            size_t order_cap = 0, cost_cap = 0;
        } tiles;
        struct Probe {
            hipEvent_t a = nullptr, b = nullptr;
            int cand = 0;
            uint64_t gen = 0;
        };
        std::vector<Probe> pending, pool;
    } order;
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 0;  // rt_comm_init (one rank per process); 0 = none
};

}  // namespace

// rt_render_async's frames in flight per worker behind the copy engine (rt_create_ex; RT_TICK_INFLIGHT)
constexpr int TICK_INFLIGHT = 2;

struct rt_ctx {
    int n_gpus = 1;            // band workers: devices, or streams on one device (RT_CREATE_SHARED_DEVICE)
    bool rccl_gather = false;  // RT_CREATE_RCCL_GATHER: rt_render gathers the bands to device 0 over RCCL, one D2H
    bool shared_device = false;  // RT_CREATE_SHARED_DEVICE: every worker on the caller's device
    bool comm_all = false;       // the single-process communicators (ncclCommInitAll) exist
    std::vector<Device> dev;
    bool has_scene = false;
    SceneLayout layout;
    rt_camera cam{};
    // rt_set_scene_track: the common layout, the stride and the per-frame host records (rt_scene.h SceneTrack, its
    // image dropped once uploaded); the images live in dev[0].d_track.  Apart from the context's scene.
    bool has_track = false;
    SceneTrack track;
    std::string last_error;
    uint64_t frames = 0, pixels = 0, launches = 0;
    uint64_t prim_rays = 0;  // traced pixels (the kernels count only reflect/shadow rays)
    double kernel_ms = 0, last_kernel_ms = 0, copy_ms = 0, gather_ms = 0;
    uint64_t timed[3] = {0, 0, 0};  // timed launches, copies, gathers
    int timing_every = 64;
    bool counting = true;  // rt_set_counting: trace launches add to the ray counters
    uint64_t scene_gen = 0;  // rt_set_scene calls (the dispatch-order measurements belong to one scene)
    int order_fixed = -1;    // RT_DISPATCH_ORDER=0/1/2: that candidate for every single-frame launch
    int path_chunk_frames = 0;  // RT_PATH_CHUNK_FRAMES: frames per launch of rt_render_path (0: by buffer size)
    int tick_inflight = 0;   // rt_render_async: frames queued per worker before the host waits (0: no bound)
    int32_t* host_staging = nullptr;
    // host ranges registered through rt_register_host and their device-mapped addresses (one per
    // worker: each device writes its band set through its own mapping): only these are written by the
    // Tick hand-off's copy kernels (anything else takes the runtime's copies)
    struct HostRange {
        char* host;
        size_t bytes;
        std::vector<char*> mapped;  // [worker], nullptr where the device has no mapping
    };
    std::vector<HostRange> host_ranges;
    // view_params cache: the camera and frame size of the last call (this scene) and the view part
    // of LaunchParams they gave (per-sphere screen boxes: a few us of host trig per launch)
    bool view_ok = false;
    rt_camera view_cam{};
    int view_w = 0, view_h = 0, view_rows = 0;
    int view_height = 0;  // rt_set_view_height: the view's height (0: each render's own frame height)
    int ss_log2 = 0;      // rt_set_supersampling: log2 of the factor k (0: off)
    int adapt_thr = 0;    // rt_set_adaptive_sampling: the threshold T in 1..256 (0: off); in effect while ss_log2 > 0
    int path_ss_log2 = 0; // rt_set_path_supersampling: log2 of the factor of the path, shutter and track renders (0: off)
    int path_adapt_thr = 0;  // rt_set_path_adaptive_sampling: the threshold T in 1..256 of those renders (0: off); in effect while path_ss_log2 > 0
    int shutter_adapt_thr = 0;  // rt_set_shutter_adaptive_sampling: the threshold T in 1..256 of the shutter renders at shutter > 1 (0: off); in effect while path_ss_log2 > 0
    // rt_set_progressive (rt_progressive.h): log2 of the factor (0: off), the run so far, the c of the last issued
    // Tick frame, and -- only while a Tick call issues its launches -- that Tick's plan (PROG_PLAIN otherwise: band,
    // batch and path renders never see one)
    int prog_log2 = 0;
    ProgRun prog_run;
    int prog_last = 0;
    ProgPlan tick_plan{PROG_PLAIN, 0, 1, 1};
    LaunchParams view_lp{};
};

// ----------------------------------------------------------------------------
// error helpers
// ----------------------------------------------------------------------------
static int fail(rt_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (ctx) ctx->last_error = buf;
    return code;
}

#define HIP_TRY(ctx, call)                                                                                 \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) return fail((ctx), RT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

#define RT_TRY(call)                     \
    do {                                 \
        const int rc_ = (call);          \
        if (rc_ != RT_OK) return rc_;    \
    } while (0)

namespace {
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

int grow(rt_ctx* ctx, void** p, size_t* cap, size_t bytes) {
    if (*cap >= bytes) return RT_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(ctx, RT_ERR_OOM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    *cap = bytes;
    return RT_OK;
}

// A lazily made handle on the current device: an ordering-only event, a non-blocking stream.
int ensure_event(rt_ctx* ctx, hipEvent_t* ev) {
    if (!*ev) HIP_TRY(ctx, hipEventCreateWithFlags(ev, hipEventDisableTiming));
    return RT_OK;
}
int ensure_stream(rt_ctx* ctx, hipStream_t* s) {
    if (!*s) HIP_TRY(ctx, hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    return RT_OK;
}

// Sum completed event pairs into the context totals (waits for them).
void drain_events(rt_ctx* ctx, Device& d) {
    for (EventPair& ep : d.pending) {
        float ms = 0.0f;
        (void)hipEventSynchronize(ep.b);
        if (hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess) {
            if (ep.kind == 0) {
                ctx->kernel_ms += ms;
                ctx->last_kernel_ms = ms;
            } else if (ep.kind == 1) {
                ctx->copy_ms += ms;
            } else {
                ctx->gather_ms += ms;
            }
            ctx->timed[ep.kind]++;
        }
        d.pool.push_back(ep);
    }
    d.pending.clear();
}

// Sampled device timing: the every-th operation of each kind on each device is bracketed
// by an event pair (rt_set_timing).  Returns whether this one is.
bool begin_timed(rt_ctx* ctx, Device& d, int kind) {
    const int every = ctx->timing_every;
    if (every <= 0 || (d.op_count[kind]++ % (uint64_t)every) != 0) return false;
    if (d.pending.size() >= 4096) drain_events(ctx, d);  // bound host memory; stalls only then
    EventPair ep;
    if (!d.pool.empty()) {
        ep = d.pool.back();
        d.pool.pop_back();
    } else {
        if (hipEventCreate(&ep.a) != hipSuccess || hipEventCreate(&ep.b) != hipSuccess) return false;
    }
    ep.kind = kind;
    (void)hipEventRecord(ep.a, d.stream);
    d.pending.push_back(ep);
    return true;
}

void end_timed(Device& d, bool timed) {
    if (timed) (void)hipEventRecord(d.pending.back().b, d.stream);
}

// The view part of lp for `cam` on a W x VH frame of the context's scene (rt_view.h view_build).  view_params (the
// context's camera, by value in the kernarg block) and the camera-path calls (one DevView per frame, view_record)
// both build their views here, so a path frame carries the values a one-camera launch would.
// scene: the records the view is built against -- the context's layout, or a track frame's (trace_anim).
int view_fill(rt_ctx* ctx, const SceneLayout& scene, const rt_camera& cam, int W, int VH, LaunchParams& lp) {
    const int rc = view_build(scene, cam, W, VH, lp);
    if (rc != RT_OK) return fail(ctx, rc, "invalid frame size %dx%d", W, VH);
    return RT_OK;
}
int view_fill(rt_ctx* ctx, const rt_camera& cam, int W, int VH, LaunchParams& lp) {
    return view_fill(ctx, ctx->layout, cam, W, VH, lp);
}

// The view of a W x VH frame (VH: rt_set_view_height, else H), of which a render traces rows [0, H).
// ss > 0 (supersampling, log2 of the factor): W and H arrive in samples, and so does the view height here.
int view_params(rt_ctx* ctx, int W, int H, LaunchParams& lp, int ss = 0) {
    const int VH = ctx->view_height > 0 ? ctx->view_height << ss : H;
    if (H > VH)
        return fail(ctx, RT_ERR_INVALID_ARG, "frame height %d above the view height %d", H >> ss, ctx->view_height);
    if (ctx->view_ok && ctx->view_w == W && ctx->view_h == VH && ctx->view_rows == H &&
        std::memcmp(&ctx->view_cam, &ctx->cam, sizeof ctx->cam) == 0) {
        copy_view(ctx->view_lp, lp);
        return RT_OK;
    }
    int rc = view_fill(ctx, ctx->cam, W, VH, lp);
    if (rc != RT_OK) return rc;
    lp.row_order_n = row_order(lp, ctx->layout, lp.row_order);  // dispatch-order candidate 0 (order_pick)
    lp.H = H;  // the rows traced (validity, band counts); a cut view's row order no longer matches: not lone
    copy_view(lp, ctx->view_lp);
    ctx->view_cam = ctx->cam, ctx->view_w = W, ctx->view_h = VH, ctx->view_rows = H, ctx->view_ok = true;
    return RT_OK;
}

// The scene part of lp: the tables of the image at `base` laid out as L says, and the scalars derived from it.
void scene_params(const rt_ctx* ctx, const Device& d, LaunchParams& lp, const SceneLayout& L, const char* base) {
    lp.sph = (const DevSphere*)(base + L.off_sph);
    lp.mat = (const DevMaterial*)(base + L.off_mat);
    lp.pl = (const DevPlane*)(base + L.off_pl);
    lp.li = (const DevLight*)(base + L.off_li);
    lp.scull = (const DevSphereCull*)(base + L.off_cull);
    lp.shcull = L.has_shcull ? (const DevShadowCull*)(base + L.off_shcull) : nullptr;
    lp.shg = L.has_shg ? (const DevShadowGrid*)(base + L.off_shg) : nullptr;
    lp.shgrid = L.has_shg ? (const unsigned long long*)(base + L.off_shgrid) : nullptr;
    lp.shslab = L.has_shg ? (const unsigned long long*)(base + L.off_shslab) : nullptr;
    lp.clus = L.n_clus ? (const DevCluster*)(base + L.off_clus) : nullptr;
    lp.shpre = L.has_shpre ? (const DevShadowCull*)(base + L.off_shpre) : nullptr;
    lp.shgrp = L.has_shgrp ? (const DevShadowGroups*)(base + L.off_shgrp) : nullptr;
    lp.n_clus = L.n_clus;
    lp.S = L.S, lp.P = L.P, lp.L = L.L, lp.limit = L.limit;
    lp.lights_a2_ok = L.lights_a2_ok ? 1 : 0;
    lp.uniform_plane = L.uniform_plane ? 1 : 0;
    lp.counters = ctx->counting ? d.d_counters : nullptr;  // nullptr: the kernels count nothing (rt_set_counting)
}
void scene_params(const rt_ctx* ctx, const Device& d, LaunchParams& lp) {
    scene_params(ctx, d, lp, ctx->layout, (const char*)d.d_scene);
}

// Per-column / per-row view-plane coordinates of TracePixel (:963-965) on the device (rt_view.h
// view_table_values: lx[W] then ly[VH]).  Rebuilt only when the frame size or view-plane size changes; frames in flight may read
// the old table, so the device is synchronised first.
int view_tables(rt_ctx* ctx, Device& d, LaunchParams& lp, int ss = 0) {
    const int VH = ctx->view_height > 0 ? ctx->view_height << ss : lp.H;  // the view's height (ly of row y)
    if (d.tab_w != lp.W || d.tab_h != VH || d.tab_pw != lp.pw || d.tab_ph != lp.ph || !d.d_view_tab) {
        std::vector<float> t((size_t)lp.W + (size_t)VH);
        view_table_values(lp.W, VH, lp.pw, lp.ph, t.data());
        HIP_TRY(ctx, hipDeviceSynchronize());
        int rc = grow(ctx, (void**)&d.d_view_tab, &d.view_tab_cap, t.size() * sizeof(float));
        if (rc != RT_OK) return rc;
        HIP_TRY(ctx, hipMemcpy(d.d_view_tab, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
        d.tab_w = lp.W, d.tab_h = VH, d.tab_pw = lp.pw, d.tab_ph = lp.ph;
    }
    lp.lxt = d.d_view_tab;
    lp.lyt = d.d_view_tab + lp.W;
    return RT_OK;
}

// Single-frame dispatch order.  A lone frame's launch ends with its slowest waves, so the order in which
// the workgroups start sets its tail (tools/wave_times.py): cheap rows last shortens it when the costly
// tiles are moderate (C1, C2: rows reversed or sorted by the cost estimate, -3 ... -9 %), while deep mirror
// chains (C3: waves of 25-40 us) run faster spread over the whole launch among cheap ones (rows varying
// fastest, -5 %) -- no one order wins every scene (profiles/ab/r04_dispatch_orders.txt).  So the library
// measures: the first single-frame launches of a scene and frame size take the candidates in turn, each
// bracketed by an event pair; once every candidate has ORDER_SAMPLES durations the one with the least
// median is kept, and measured again after ORDER_RETUNE launches (the view drifts).  Candidates:
// 0 tile rows by decreasing estimated cost (row_order), 1 tile rows bottom to top, 2 rows varying fastest
// (column-major over the 4-tile workgroups), natural row order, 3 every tile by decreasing measured
// duration (longest first: a lone frame's tail is its costliest waves started late; C3 36.3 -> 30.8 us,
// profiles/ab/r05_tile_order.txt).  The bundle kernel's lone frames (its all-lights-ok merged
// instantiation) take the same tuner: 0-2 are its natural order, 3 the measured one (C4 338 -> 302 us,
// C5 1,136 -> 1,109 us -- faster than a frame of a 64-frame batch launch, 309 / 1,125 us).
constexpr int ORDER_CANDIDATES = 4, ORDER_SAMPLES = 7;
constexpr float ORDER_MARGIN = 1.01f;  // another order replaces candidate 0 only when > 1 % faster (median)
constexpr uint64_t ORDER_RETUNE = 1u << 14;

void order_collect(Device& d) {
    Device::OrderTuner& t = d.order;
    size_t keep = 0;
    for (size_t i = 0; i < t.pending.size(); ++i) {
        Device::OrderTuner::Probe& pr = t.pending[i];
        if (hipEventQuery(pr.b) != hipSuccess) {
            t.pending[keep++] = pr;
            continue;
        }
        float ms = 0;
        if (pr.gen == t.gen && hipEventElapsedTime(&ms, pr.a, pr.b) == hipSuccess)
            t.ms[pr.cand].push_back(ms);
        t.pool.push_back(pr);
    }
    t.pending.resize(keep);
}

// The candidate for this single-frame launch; *probe: bracket it with order_begin / order_end.
int order_pick(rt_ctx* ctx, Device& d, int W, int H, bool* probe) {
    *probe = false;
    if (ctx->order_fixed >= 0) return ctx->order_fixed;
    Device::OrderTuner& t = d.order;
    if (t.W != W || t.H != H || t.scene_gen != ctx->scene_gen || (t.chosen >= 0 && ++t.since > ORDER_RETUNE)) {
        t.W = W, t.H = H, t.scene_gen = ctx->scene_gen;
        t.chosen = -1, t.turn = 0, t.since = 0, t.gen++;
        for (std::vector<float>& v : t.ms) v.clear();
    }
    if (t.chosen >= 0) return t.chosen;
    order_collect(d);
    // candidate 3 packs tile coordinates in 16 bits each (tile_order_prepare): not for frames beyond that
    const int nc = (W + 7) / 8 > 0xffff || (H + 7) / 8 > 0xffff ? 3 : ORDER_CANDIDATES;
    bool done = true;
    for (int k = 0; k < nc; ++k) done = done && t.ms[k].size() >= (size_t)ORDER_SAMPLES;
    if (done) {
        // the least median, unless candidate 0 is within the margin of it: the launches of a bench or of
        // another process on the GPU can overlap the probes, and a noise-driven choice should not stick
        float best = 0, med0 = 0;
        for (int k = 0; k < nc; ++k) {
            std::vector<float> v = t.ms[k];
            std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
            if (k == 0) med0 = v[v.size() / 2];
            if (t.chosen < 0 || v[v.size() / 2] < best) t.chosen = k, best = v[v.size() / 2];
        }
        if (med0 <= best * ORDER_MARGIN) t.chosen = 0;
        return t.chosen;
    }
    const int k = t.turn++ % nc;
    // bound the probes in flight (results arrive as the launches complete)
    *probe = t.ms[k].size() + t.pending.size() < (size_t)(4 * ORDER_SAMPLES * ORDER_CANDIDATES);
    return k;
}

bool order_begin(Device& d, int cand, hipStream_t s) {
    Device::OrderTuner& t = d.order;
    Device::OrderTuner::Probe pr;
    if (!t.pool.empty()) {
        pr = t.pool.back();
        t.pool.pop_back();
    } else if (hipEventCreate(&pr.a) != hipSuccess || hipEventCreate(&pr.b) != hipSuccess) {
        return false;
    }
    pr.cand = cand, pr.gen = t.gen;
    (void)hipEventRecord(pr.a, s);
    t.pending.push_back(pr);
    return true;
}

void order_end(Device& d, hipStream_t s) { (void)hipEventRecord(d.order.pending.back().b, s); }

// Candidate 3 of a single-frame launch (the direct kernel's 4-tile workgroups): the first launch of each
// measuring round (and of each frame size / scene) records every tile's duration instead of being timed as a
// probe; the first candidate-3 launch after it reads the durations back and uploads the tiles sorted by
// decreasing duration, ties in natural order.  The readback and the upload wait for the whole device (once
// per measuring round): the recording launch and the launches still reading the previous order may sit on
// any stream of the context (d.stream, the async stream, a caller's stream of rt_render_device).  The order
// is recorded again when the camera has moved and TILE_ORDER_REFRESH launches have used it (an interactive
// view drifts; pixels never depend on the order).  Returns the candidate to launch (candidate 3 falls back to
// 0 while its order is not ready), -1 when the buffers cannot be allocated, -2 on a HIP error (recorded).
constexpr uint64_t TILE_ORDER_REFRESH = 256;
int tile_order_prepare(rt_ctx* ctx, Device& d, int W, int H, LaunchParams& lp, int cand, bool* probe) {
    Device::OrderTuner::Tiles& o = d.order.tiles;
    if (o.gen != d.order.gen || o.scene_gen != ctx->scene_gen || o.W != W || o.H != H ||
        (o.built && o.uses >= TILE_ORDER_REFRESH && std::memcmp(&o.cam, &ctx->cam, sizeof o.cam) != 0)) {
        o.gen = d.order.gen, o.scene_gen = ctx->scene_gen, o.W = W, o.H = H;
        o.recorded = o.built = false;
    }
    const size_t tx = (size_t)(W + 7) / 8, ty = (size_t)(H + 7) / 8, n = tx * ty;
    const size_t padded = (n + SINGLE_WPG - 1) / SINGLE_WPG * SINGLE_WPG;
    if (ty > 0xffff || tx > 0xffff) return cand == 3 ? 0 : cand;  // (not representable: candidates 0-2 only)
    if (!o.recorded) {
        int rc = grow(ctx, (void**)&o.d_cost, &o.cost_cap, n * sizeof(uint32_t));
        if (rc == RT_OK) rc = grow(ctx, (void**)&o.d_order, &o.order_cap, padded * sizeof(uint32_t));
        if (rc != RT_OK) return -1;
        lp.tile_cost = o.d_cost;
        o.recorded = true;
        o.cam = ctx->cam, o.uses = 0;
        *probe = false;  // (the duration stores are not the candidate's own cost)
        return cand == 3 ? 0 : cand;
    }
    if (cand == 3 && !o.built) {
        std::vector<uint32_t> cost(n), order(padded, 0xffff0000u);
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(cost.data(), o.d_cost, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) {
            tiles_by_cost(cost.data(), n, (uint32_t)tx, order.data());
            e = hipMemcpy(o.d_order, order.data(), padded * sizeof(uint32_t), hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) {
            fail(ctx, RT_ERR_HIP, "tile order readback / upload: %s", hipGetErrorString(e));
            return -2;
        }
        o.built = true;
    }
    if (cand == 3) {
        lp.tile_order = o.d_order;
        o.uses++;
    }
    return cand;
}

// The fused encoder's target of a trace with out_fmt OUT_TILES (rt_render_bands_tiles).
struct EncTarget {
    unsigned char* wire;
    uint32_t* stage;
    int tiles_x, tpf, frame0;
};

// The tail of trace_bands and trace_path: lp launched on `stream` as one of device d's sampled-timing traces
// (`what` names the caller in the error text), the launch counted and, while the context counts
// (rt_set_counting), the pixels of rows < H in the nb launched bands (first, step) of n_frames frames; ss:
// supersampling, so samples -- but one per pixel in an adaptive launch (lp.adapt_thr, lp.view_adapt or lp.shutter_adapt > 0; of
// a shutter launch n_frames counts the sub-frames, so one per pixel and sub-frame), whose waves count the
// samples they trace beyond that on the device (CNT_EXTRA_PRIMARY, rt_get_stats).  Nothing but the launch lies between the timing events; a caller that probes the
// dispatch order brackets the whole call with order_begin / order_end.
int launch_counted(rt_ctx* ctx, Device& d, hipStream_t stream, const LaunchParams& lp, const char* what, int W, int H,
                   int band_rows, int first, int step, int nb, int n_frames, int ss, int generic_pow = -1) {
    hipStream_t saved = d.stream;
    d.stream = stream;
    const bool timed = begin_timed(ctx, d, 0);
    // (generic_pow: the launch's scene is not the context's -- a scene track's OR over its frames)
    const int e = launch_trace(lp, generic_pow < 0 ? ctx->layout.generic_pow : generic_pow != 0, false, stream);
    end_timed(d, timed);
    d.stream = saved;
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString((hipError_t)e));
    ctx->launches++;
    if (lp.adapt_thr > 0 || lp.view_adapt > 0 || lp.shutter_adapt > 0) ss = 0;
    // (a progressive launch: the samples it traces per pixel, none when it only emits)
    const uint64_t per_pixel = lp.prog_acc != nullptr ? (uint64_t)lp.prog_n : (uint64_t)1 << (2 * ss);
    for (int k = 0; k < nb && ctx->counting; ++k) {
        const long long y0 = (long long)(first + k * step) * band_rows;
        ctx->prim_rays += (uint64_t)std::min<long long>(band_rows, (long long)H - y0) * (uint64_t)W * (uint64_t)n_frames * per_pixel;
    }
    return RT_OK;
}

// Adaptive sampling in effect (rt_set_adaptive_sampling with k > 1): the 8x8 tiles of a band render sit on the
// frame's 8-row grid (rt_internal.h adaptive_band_ok; the library's own 8-row bands and chunks do).  The band
// renders ask before they touch a device, trace_bands before every launch.
int check_adaptive_bands(rt_ctx* ctx, int band_rows, int H) {
    if (ctx->ss_log2 > 0 && ctx->adapt_thr > 0 && !adaptive_band_ok(band_rows, H))
        return fail(ctx, RT_ERR_UNSUPPORTED,
                    "adaptive sampling needs bands of a multiple of 8 rows, or one band of the whole frame (band_rows %d, height %d)",
                    band_rows, H);
    return RT_OK;
}

// A trace_bands launch: bands (first, step) of `band_rows` rows of the W x H frame, at most max_bands of them
// (bands_of: how many there are), into `out`.
struct TraceReq {
    int W, H, band_rows, first, step;
    int32_t* out;
    int fmt = RT_BANDS_INT32;
    int n_frames = 1;                 // frames of the launch (grid z), frame_bytes apart in `out`
    size_t frame_bytes = 0;
    const EncTarget* enc = nullptr;   // the fused tile encoder's target
    const CopyJob* slice = nullptr;   // a Tick hand-off that rides in the launch as its copy slice
    int max_bands = INT_MAX;
    // a Tick of a progressive run (rt_ctx::tick_plan is PROG_TRACE or PROG_EMIT): the worker's accumulator at the
    // request's first band, packed like a band set; nullptr: any other launch
    ResolveSum* acc = nullptr;
};

// Launch the trace `q` on device d.
// Supersampling (rt_set_supersampling, k = 1 << ss > 1): the request is in output pixels as ever, and so
// is everything the callers do with the output (band sets, hand-offs, gathers); the launch itself works on
// the k W x k H sample frame -- the same bands, each k times as many sample rows -- and its epilogue writes
// one output pixel per k x k block (LaunchParams::ss_log2).  check_ctx bounds k W * k H.
int trace_bands(rt_ctx* ctx, Device& d, hipStream_t stream, const TraceReq& q) {
    const int W = q.W, H = q.H, band_rows = q.band_rows, first = q.first, step = q.step, n_frames = q.n_frames;
    const EncTarget* enc = q.enc;
    // A progressive Tick beyond its first frame (q.acc): a launch on the k W x k H sample frame like a supersampling
    // one, with the run's factor (rt_set_supersampling is off: TickScope::begin refused the Tick otherwise).
    const bool prog = q.acc != nullptr;
    const int ss = prog ? ctx->prog_log2 : ctx->ss_log2;
    if (ss > 0 && enc) return fail(ctx, RT_ERR_UNSUPPORTED, "the fused tile encoder does not supersample");
    const int thr = ss > 0 && !prog ? ctx->adapt_thr : 0;
    RT_TRY(check_adaptive_bands(ctx, band_rows, H));
    if (prog && (ss <= 0 || ctx->tick_plan.kind == PROG_PLAIN || enc || n_frames != 1 || !adaptive_band_ok(band_rows, H)))
        return fail(ctx, RT_ERR_UNSUPPORTED, "progressive launch outside a Tick's band plan (band_rows %d, height %d)", band_rows, H);
    LaunchParams lp;
    std::memset(&lp, 0, sizeof lp);
    RT_TRY(view_params(ctx, W << ss, H << ss, lp, ss));
    scene_params(ctx, d, lp);
    RT_TRY(view_tables(ctx, d, lp, ss));
    const int nb = std::min(bands_of(H, band_rows, first, step), q.max_bands);
    lp.band_first = first, lp.band_step = step;
    if (ss > 0) {
        // (a band of H rows or more is the frame as band 0 whatever its size: k band_rows stays below k H)
        lp.band_rows = std::min(band_rows, H) << ss;
        lp.local_rows = nb * lp.band_rows;
        lp.ss_log2 = ss;
        lp.adapt_thr = thr;
        if (prog) {
            const ProgPlan& pl = ctx->tick_plan;
            lp.prog_acc = q.acc;
            lp.prog_first = pl.first, lp.prog_n = pl.samples;
            for (int i = 0; i < pl.samples; ++i) lp.prog_pass[i] = prog_pass(ss, pl.first + i);
        }
    } else {
        lp.band_rows = band_rows;
        lp.local_rows = nb * band_rows;
    }
    lp.out = q.out;
    lp.out_fmt = q.fmt;
    lp.n_frames = n_frames;
    lp.out_frame_bytes = q.frame_bytes;
    // single-frame launches of a whole frame on the direct kernel: the dispatch order (order_pick)
    const bool with_copy = q.slice && q.slice->words;
    // (supersampling launches are never lone: natural tile order, one tile per workgroup)
    const bool whole = ss == 0 && !enc && !with_copy && band_rows >= lp.local_rows && lp.local_rows == H;
    const bool lone = n_frames <= 1 && whole && lp.S < CULL_MIN_SPHERES && lp.row_order_n == (H + 7) / 8;
    // the bundle kernel's all-lights-ok merged instantiation (C4/C5): natural or measured tile order
    const SceneLayout& L = ctx->layout;
    const bool lone_bundle = n_frames <= 1 && whole && merged_class(lp.S, lp.L, L.lights_a2_ok) == 2 && !L.generic_pow;
    bool probe = false;
    int cand = -1;
    if (lone || lone_bundle) {
        cand = order_pick(ctx, d, W, H, &probe);
        // (candidates 1 and 2 order the direct kernel's 4-tile groups: a bundle launch under them is natural order)
        if (ctx->order_fixed < 0 ? d.order.chosen < 0 || cand == 3 : cand == 3)  // measuring, or the measured order
            cand = tile_order_prepare(ctx, d, W, H, lp, cand, &probe);
        if (cand == -2) return RT_ERR_HIP;  // (rt_last_error holds the HIP error)
        if (cand < 0) return fail(ctx, RT_ERR_OOM, "tile order buffers");
        if (lone && cand == 1)
            for (int r = 0; r < lp.row_order_n; ++r) lp.row_order[r] = (uint16_t)(lp.row_order_n - 1 - r);
        if (lone && cand == 2) lp.row_order_n = 0, lp.col_major = 1;
        if (lone_bundle) lp.row_order_n = 0;
    } else {
        lp.row_order_n = 0;  // (batch launches keep the natural order: the measured one measured no better,
                             //  profiles/ab/r05_batch_tile_order_rejected.txt)
    }
    if (enc) {
        lp.out_fmt = OUT_TILES;
        lp.enc_wire = enc->wire, lp.enc_stage = enc->stage;
        lp.enc_tiles_x = enc->tiles_x, lp.enc_tpf = enc->tpf, lp.enc_frame0 = enc->frame0;
    }
    if (with_copy) {  // the previous frame's (chunk's) hand-off rides along
        lp.copy = *q.slice;
        lp.copy_z = 1;
        lp.out_frame_bytes = 0;
    }
    probe = probe && order_begin(d, cand, stream);
    if (prog) {  // the accumulator's launches run in issue order whatever streams the Ticks use
        RT_TRY(ensure_event(ctx, &d.ev[Device::EV_PROG]));
        if (d.prog_touched && d.prog_stream != stream) HIP_TRY(ctx, hipStreamWaitEvent(stream, d.ev[Device::EV_PROG], 0));
    }
    const int rc = launch_counted(ctx, d, stream, lp, "trace", W, H, band_rows, first, step, nb, n_frames, ss);
    if (probe) order_end(d, stream);
    if (prog && rc == RT_OK) {
        HIP_TRY(ctx, hipEventRecord(d.ev[Device::EV_PROG], stream));
        d.prog_stream = stream, d.prog_touched = true;
    }
    return rc;
}

// `sampled`: a render that supersamples (its k W x k H sample frame is bounded like any frame).
int check_ctx(rt_ctx* ctx, int W, int H, bool sampled = true) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    if (!ctx->has_scene) return fail(ctx, RT_ERR_NO_SCENE, "rt_set_scene has not been called");
    if (W <= 0 || H <= 0 || (long long)W * H > (1LL << 31) - 1)
        return fail(ctx, RT_ERR_INVALID_ARG, "invalid frame size %dx%d", W, H);
    if (sampled && ctx->ss_log2 > 0 && (((long long)W << ctx->ss_log2) * ((long long)H << ctx->ss_log2)) > (1LL << 31) - 1)
        return fail(ctx, RT_ERR_INVALID_ARG, "frame size %dx%d at supersampling factor %d exceeds 2^31 - 1 samples", W, H,
                    1 << ctx->ss_log2);
    return RT_OK;
}

// The band arguments of the band renders (`who` names the entry point in the error text).
int check_band_args(rt_ctx* ctx, const char* who, int band_rows, int band_first, int band_step, const void* d_out,
                    int format) {
    if (band_rows <= 0 || band_first < 0 || band_step <= 0 || !d_out ||
        (format != RT_BANDS_INT32 && format != RT_BANDS_RGB24 && format != RT_BANDS_FRAME))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: bad band arguments", who);
    return RT_OK;
}

// Worker g's device-mapped address of [host, host + bytes) when it lies inside a range registered
// through rt_register_host and both ends allow the copy kernels' 16-byte stores; else nullptr.
int32_t* mapped_host(const rt_ctx* ctx, int g, void* host, size_t bytes) {
    if (((uintptr_t)host & 15) != 0) return nullptr;
    const char* h = (const char*)host;
    for (const rt_ctx::HostRange& r : ctx->host_ranges)
        if (h >= r.host && bytes <= r.bytes && (size_t)(h - r.host) <= r.bytes - bytes) {
            char* base = (size_t)g < r.mapped.size() ? r.mapped[(size_t)g] : nullptr;
            if (!base) return nullptr;
            char* m = base + (h - r.host);
            return ((uintptr_t)m & 15) == 0 ? (int32_t*)m : nullptr;
        }
    return nullptr;
}

// The trace of bands [k0, k1) of a share into the packed band set at buf (band 0); `slice` rides in the launch.
// acc: the worker's progressive accumulator (band 0) in a Tick that uses it (tick_acc), offset like buf.
TraceReq share_req(const Share& sh, int W, int H, int k0, int k1, int32_t* buf, const CopyJob* slice = nullptr,
                   ResolveSum* acc = nullptr) {
    TraceReq q{W, H, sh.band_rows, sh.first + k0 * sh.step, sh.step, buf + (size_t)k0 * sh.band_rows * W};
    q.slice = slice;
    q.max_bands = k1 - k0;
    q.acc = acc ? acc + (size_t)k0 * sh.band_rows * W : nullptr;
    return q;
}
// Worker d's accumulator in a Tick whose plan uses it, else nullptr (the plain launch).
ResolveSum* tick_acc(const rt_ctx* ctx, const Device& d) { return ctx->tick_plan.kind != PROG_PLAIN ? d.d_prog : nullptr; }
// A Tick call (rt_render, rt_render_async, rt_render_device) under rt_set_progressive: begin() compares the view key
// with the last Tick's, advances the run and leaves the Tick's plan in ctx->tick_plan for the launches the call
// issues -- captured at enqueue time, like the camera; the scope's end takes the plan away again, so that no other
// render sees one, and a Tick that failed ends the run (its accumulator may be half written: the next Tick is P_1).
// With the feature off begin() touches nothing but the reported count.
struct TickScope {
    rt_ctx* ctx;
    bool done = false;
    explicit TickScope(rt_ctx* c) : ctx(c) {}
    ~TickScope() {
        if (!done) ctx->prog_run.count = 0;
        else ctx->prog_last = ctx->tick_plan.divisor;
        ctx->tick_plan = ProgPlan{PROG_PLAIN, 0, 1, 1};
    }
    int begin(int W, int H) {
        const int s = ctx->prog_log2, k = 1 << s;
        ctx->tick_plan = ProgPlan{PROG_PLAIN, 0, 1, 1};
        if (s == 0) return RT_OK;
        if (ctx->ss_log2 > 0)
            return fail(ctx, RT_ERR_UNSUPPORTED, "progressive accumulation (factor %d) with rt_set_supersampling(%d) on", k,
                        1 << ctx->ss_log2);
        const int VH = ctx->view_height > 0 ? ctx->view_height : H;
        if (((long long)W << s) * ((long long)VH << s) > (1LL << 31) - 1)
            return fail(ctx, RT_ERR_INVALID_ARG, "frame size %dx%d at progressive factor %d exceeds 2^31 - 1 samples", W, VH, k);
        const ProgKey key = prog_key(ctx->scene_gen, ctx->cam, W, H, ctx->view_height, k, ctx->n_gpus);
        ProgPlan plan = prog_plan(&ctx->prog_run, key);
        if (plan.kind != PROG_PLAIN) {
            const int n = ctx->n_gpus;
            for (int g = 0; g < n; ++g) {  // 8 bytes per pixel of each worker's packed band set
                Device& d = ctx->dev[(size_t)g];
                const size_t bytes = (size_t)bands_of(H, TICK_BAND_ROWS, g, n) * TICK_BAND_ROWS * (size_t)W * sizeof(ResolveSum);
                if (d.prog_cap >= bytes) continue;
                if (plan.first > 0) {  // (cannot happen: the run's second Tick sized it; never read what was not written)
                    ctx->prog_run.count = 0;
                    plan = prog_plan(&ctx->prog_run, key);
                    break;
                }
                DeviceGuard guard(d.id);
                RT_TRY(grow(ctx, (void**)&d.d_prog, &d.prog_cap, bytes));  // (hipFree waits for the launches that use it)
                d.prog_touched = false;
            }
        }
        ctx->tick_plan = plan;
        return RT_OK;
    }
};

// Issue each worker's pending rt_render_async hand-off (the last frame's D2H) on its async stream.
int flush_hand(rt_ctx* ctx) {
    if (!ctx) return RT_OK;
    for (Device& d : ctx->dev) {
        if (!d.hand.job.words) continue;
        DeviceGuard guard(d.id);
        const auto h = d.hand;
        d.hand = {};
        if (h.host && h.job.band_words == 0) {  // one contiguous band set: the runtime's copy
            HIP_TRY(ctx, hipMemcpyAsync(h.host, h.job.src, h.job.words * sizeof(int32_t), hipMemcpyDeviceToHost,
                                        d.async_stream));
        } else {
            const int e = launch_band_copy(h.job, d.async_stream);
            if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "hand-off copy: %s", hipGetErrorString((hipError_t)e));
        }
    }
    return RT_OK;
}

// rt_render_async frames still pending are completed first (the caller may reuse their buffers).
int wait_pending_async(rt_ctx* ctx) {
    for (const Device& d : ctx->dev)
        if (d.hand.job.words || d.copy_pending[0] || d.copy_pending[1]) return rt_wait(ctx);
    return RT_OK;
}

// Bands [k0, k1) of a worker's band set (src, packed from band 0) into the host frame by the runtime's copies.
int runtime_band_copy(rt_ctx* ctx, const Share& sh, int W, int H, const int32_t* src, int32_t* host, hipStream_t st,
                      bool pinned, int k0, int k1) {
    return for_band_copies(sh, W, H, k0, k1, pinned, [&](size_t dst, size_t from, size_t width, size_t rows, size_t pitch) {
        const size_t wb = width * sizeof(int32_t);
        if (pitch)
            HIP_TRY(ctx, hipMemcpy2DAsync(host + dst, pitch * sizeof(int32_t), src + from, wb, wb, rows,
                                          hipMemcpyDeviceToHost, st));
        else
            HIP_TRY(ctx, hipMemcpyAsync(host + dst, src + from, wb, hipMemcpyDeviceToHost, st));
        return (int)RT_OK;
    });
}

// The copy-engine hand-off of a share: each non-empty chunk c of nc is traced into buf (the packed band set) on
// `trace`, and once its event has fired the copy engine moves it into `host` on the worker's copy stream, under
// the trace of chunk c + 1.  The wait captures the event's record of this call, so a later frame may record the
// same event while this frame's copy is still queued.
int trace_and_copy_chunks(rt_ctx* ctx, Device& d, hipStream_t trace, const Share& sh, int W, int H, int nc,
                          int32_t* buf, int32_t* host, bool pinned) {
    RT_TRY(ensure_stream(ctx, &d.copy_stream));
    for (int c = 0; c < nc; ++c) {
        const Bands b = chunk_bands(sh, c, nc);
        if (b.k1 <= b.k0) continue;
        hipEvent_t& ev = d.ev[Device::EV_CHUNK + c];
        RT_TRY(ensure_event(ctx, &ev));
        RT_TRY(trace_bands(ctx, d, trace, share_req(sh, W, H, b.k0, b.k1, buf, nullptr, tick_acc(ctx, d))));
        HIP_TRY(ctx, hipEventRecord(ev, trace));
        HIP_TRY(ctx, hipStreamWaitEvent(d.copy_stream, ev, 0));
        RT_TRY(runtime_band_copy(ctx, sh, W, H, buf, host, d.copy_stream, pinned, b.k0, b.k1));
    }
    return RT_OK;
}

// The single-process communicators of a multi-GPU context (ncclCommInitAll over its devices), made on
// first use: the xGMI gather of rt_render_device at n > 1 and of RT_CREATE_RCCL_GATHER contexts.
int ensure_comm_all(rt_ctx* ctx) {
    if (ctx->comm_all) return RT_OK;
    if (ctx->shared_device && ctx->n_gpus > 1)
        return fail(ctx, RT_ERR_UNSUPPORTED, "RCCL needs one device per rank (RT_CREATE_SHARED_DEVICE context)");
    std::string err;
    if (!g_rccl.load(err)) return fail(ctx, RT_ERR_RCCL, "%s", err.c_str());
    const int n = ctx->n_gpus;
    std::vector<ncclComm_t> comms((size_t)n);
    std::vector<int> ids((size_t)n);
    for (int g = 0; g < n; ++g) ids[(size_t)g] = ctx->dev[(size_t)g].id;
    const ncclResult_t r = g_rccl.CommInitAll(comms.data(), n, ids.data());
    if (r != 0) return fail(ctx, RT_ERR_RCCL, "ncclCommInitAll: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    for (int g = 0; g < n; ++g) ctx->dev[(size_t)g].comm = comms[(size_t)g];
    ctx->comm_all = true;
    return RT_OK;
}

// Every worker's bands gathered into dst (device 0, row-major frame) on device 0's stream: each device
// traces its band set into its slot, a grouped ncclGather moves the slots to device 0 over xGMI, one
// scatter launch per worker reassembles them there.
int gather_frame(rt_ctx* ctx, int width, int height, int32_t* dst) {
    int rc = ensure_comm_all(ctx);
    if (rc != RT_OK) return rc;
    const int n = ctx->n_gpus;
    const int band_rows = TICK_BAND_ROWS;
    const int max_nb = bands_of(height, band_rows, 0, n);
    const size_t slot = (size_t)max_nb * band_rows * width;  // int32 elements per device
    Device& d0 = ctx->dev[0];
    for (int g = 0; g < n; ++g) {
        Device& d = ctx->dev[(size_t)g];
        DeviceGuard guard(d.id);
        rc = grow(ctx, (void**)&d.d_bands, &d.bands_cap, slot * sizeof(int32_t));
        if (rc == RT_OK && g == 0) rc = grow(ctx, (void**)&d.d_gather, &d.gather_cap, slot * n * sizeof(int32_t));
        TraceReq q{width, height, band_rows, g, n, d.d_bands};
        q.acc = tick_acc(ctx, d);
        if (rc == RT_OK) rc = trace_bands(ctx, d, d.stream, q);
        if (rc != RT_OK) return rc;
    }
    std::vector<char> gtimed((size_t)n, 0);
    for (int g = 0; g < n; ++g) {
        DeviceGuard guard(ctx->dev[(size_t)g].id);
        gtimed[(size_t)g] = begin_timed(ctx, ctx->dev[(size_t)g], 2);
    }
    if (g_rccl.GroupStart() != 0) return fail(ctx, RT_ERR_RCCL, "ncclGroupStart failed");
    for (int g = 0; g < n; ++g) {
        Device& d = ctx->dev[(size_t)g];
        DeviceGuard guard(d.id);
        const ncclResult_t r = g_rccl.Gather(d.d_bands, g == 0 ? d.d_gather : nullptr, slot, ncclInt32, 0, d.comm,
                                             d.stream);
        if (r != 0) {
            (void)g_rccl.GroupEnd();
            return fail(ctx, RT_ERR_RCCL, "ncclGather: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
        }
    }
    if (g_rccl.GroupEnd() != 0) return fail(ctx, RT_ERR_RCCL, "ncclGroupEnd failed");
    for (int g = 0; g < n; ++g) {
        DeviceGuard guard(ctx->dev[(size_t)g].id);
        end_timed(ctx->dev[(size_t)g], gtimed[(size_t)g]);
    }
    DeviceGuard guard(d0.id);
    for (int g = 0; g < n; ++g) {
        const int nb = bands_of(height, band_rows, g, n);
        const int e = launch_scatter_bands(d0.d_gather + slot * g, dst, width, height, band_rows, g, n, nb, d0.stream);
        if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "scatter: %s", hipGetErrorString((hipError_t)e));
    }
    return RT_OK;
}
}  // namespace

// ============================================================================
// exported C ABI
// ============================================================================
extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_device_count(int* out_count) {
    if (!out_count) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL out_count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) n = 0;
    else if (e != hipSuccess) return fail(nullptr, RT_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    *out_count = n;
    return RT_OK;
}

const char* rt_last_error(const rt_ctx* ctx) {
    if (ctx) return ctx->last_error.c_str();
    return g_last_error.c_str();
}

int rt_create(int n_gpus, rt_ctx** out_ctx) { return rt_create_ex(n_gpus, 0, out_ctx); }

int rt_create_ex(int n_gpus, int flags, rt_ctx** out_ctx) {
    if (!out_ctx || n_gpus < 1 || n_gpus > RT_MAX_WORKERS ||
        (flags & ~(RT_CREATE_RCCL_GATHER | RT_CREATE_SHARED_DEVICE)) != 0 ||
        ((flags & RT_CREATE_RCCL_GATHER) && (flags & RT_CREATE_SHARED_DEVICE) && n_gpus > 1))
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create: bad arguments");
    *out_ctx = nullptr;
    const bool shared = (flags & RT_CREATE_SHARED_DEVICE) != 0;
    int ndev = 0;
    if (rt_device_count(&ndev) != RT_OK || ndev == 0)
        return fail(nullptr, RT_ERR_NO_DEVICE, "no HIP device visible (libraytracer_hip has no CPU fallback)");
    if (n_gpus > ndev && !shared)
        return fail(nullptr, RT_ERR_NO_DEVICE, "rt_create(%d): only %d devices visible", n_gpus, ndev);
    rt_ctx* ctx = new (std::nothrow) rt_ctx();
    if (!ctx) return fail(nullptr, RT_ERR_OOM, "out of host memory");
    ctx->n_gpus = n_gpus;
    ctx->rccl_gather = (flags & RT_CREATE_RCCL_GATHER) != 0;
    ctx->shared_device = shared;
    // RT_DISPATCH_ORDER=0/1/2 fixes the single-frame dispatch order (order_pick; A/B and tests)
    if (const char* o = std::getenv("RT_DISPATCH_ORDER"))
        if (o[0] >= '0' && o[0] < '0' + ORDER_CANDIDATES && o[1] == 0) ctx->order_fixed = o[0] - '0';
    // RT_PATH_CHUNK_FRAMES=1..65535 fixes the frames per launch of rt_render_path (path_chunk_frames)
    if (const char* q = std::getenv("RT_PATH_CHUNK_FRAMES")) {
        const int k = std::atoi(q);
        if (k >= 1 && k <= RT_MAX_PATH_FRAMES) ctx->path_chunk_frames = k;
    }
    // rt_render_async keeps at most TICK_INFLIGHT frames per worker queued behind the copy engine: with more, one
    // hipMemcpyAsync of the hand-off now and then blocked the host for 6-7 ms (the runtime, not the copy: 5.4-7.0 ms
    // for an 8.3 MB copy that takes 160 us) -- a queued C3 run of 20 frames at 2.1-2.7k fps instead of 5.8k, in
    // runs 0 and 2 of 4 unbounded, 1 of 4 at 4, every run at 8, none at 2 or 3 (profiles/r06_tick_deep.txt).  The
    // double buffer needs no more than 2: frame k+2 is traced into frame k's buffer after frame k's copy anyway.
    // RT_TICK_INFLIGHT=0..16 overrides (0: no bound; A/B)
    ctx->tick_inflight = TICK_INFLIGHT;
    if (const char* q = std::getenv("RT_TICK_INFLIGHT")) ctx->tick_inflight = std::max(0, std::min(16, std::atoi(q)));
    ctx->dev.resize((size_t)n_gpus);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (int g = 0; g < n_gpus; ++g) {
        Device& d = ctx->dev[(size_t)g];
        d.id = (n_gpus == 1 || shared) ? cur : g;  // one device: the caller's current one
        DeviceGuard guard(d.id);
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d.id) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            int rc = fail(ctx, RT_ERR_NO_DEVICE, "device %d is %s, this build targets gfx950", d.id, prop.gcnArchName);
            g_last_error = ctx->last_error;
            rt_destroy(ctx);
            return rc;
        }
        hipError_t e = hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMalloc((void**)&d.d_counters, COUNTER_WORDS * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemset(d.d_counters, 0, COUNTER_WORDS * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipDeviceSynchronize();  // kernels run on non-blocking streams
        // The runtime loads a code object on the host inside the first launch of one of its kernels.  For part 0 of the
        // trace kernels (rt_kernel.hip "Parts": the plain and diagnostic launches, so every Tick and batch render;
        // 208 of the 928 kernels) that launch is made here -- band_copy_kernel, a kernel of that part, moves 16 bytes of the
        // zeroed counters onto their neighbours -- so that the load is part of rt_create and not of the first frame,
        // nor of whatever a caller measures in wall time from its first render on.  The other parts load at their first
        // launch, as before.
        if (e == hipSuccess)
            e = (hipError_t)launch_band_copy(CopyJob{(const int32_t*)(d.d_counters + 2), (int32_t*)d.d_counters, 4, 0, 0, 0}, d.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
        if (e != hipSuccess) {
            int rc = fail(ctx, RT_ERR_HIP, "device %d init: %s", d.id, hipGetErrorString(e));
            g_last_error = ctx->last_error;
            rt_destroy(ctx);
            return rc;
        }
    }
    if (ctx->rccl_gather) {  // the gather's communicators now, so that a missing RCCL fails here
        const int rc = ensure_comm_all(ctx);
        if (rc != RT_OK) {
            g_last_error = ctx->last_error;
            rt_destroy(ctx);
            return rc;
        }
    }
    *out_ctx = ctx;
    return RT_OK;
}

void rt_destroy(rt_ctx* ctx) {
    if (!ctx) return;
    (void)flush_hand(ctx);  // the last rt_render_async frame still reaches its (registered) buffer
    for (Device& d : ctx->dev) {
        DeviceGuard guard(d.id);
        (void)hipDeviceSynchronize();  // kernels on caller streams may still read our buffers
        for (EventPair& ep : d.pending) (void)hipEventDestroy(ep.a), (void)hipEventDestroy(ep.b);
        for (EventPair& ep : d.pool) (void)hipEventDestroy(ep.a), (void)hipEventDestroy(ep.b);
        for (auto* v : {&d.order.pending, &d.order.pool})
            for (Device::OrderTuner::Probe& pr : *v) (void)hipEventDestroy(pr.a), (void)hipEventDestroy(pr.b);
        for (hipEvent_t ev : d.ev)
            if (ev) (void)hipEventDestroy(ev);
        for (Device::PathSlot& ps : d.path_slot) {
            if (ps.done) (void)hipEventDestroy(ps.done);
            if (ps.h_views) (void)hipHostFree(ps.h_views);
            if (ps.d_views) (void)hipFree(ps.d_views);
        }
        for (int i = 0; i < 2; ++i)
            if (d.d_path[i]) (void)hipFree(d.d_path[i]);
        if (d.copy_stream) (void)hipStreamDestroy(d.copy_stream);
        if (d.comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(d.comm);
        if (d.d_scene) (void)hipFree(d.d_scene);
        if (d.d_track) (void)hipFree(d.d_track);
        if (d.d_frame) (void)hipFree(d.d_frame);
        if (d.d_bands) (void)hipFree(d.d_bands);
        if (d.d_gather) (void)hipFree(d.d_gather);
        for (int i = 0; i < 2; ++i)
            if (d.d_frames2[i]) (void)hipFree(d.d_frames2[i]);
        if (d.d_counters) (void)hipFree(d.d_counters);
        if (d.d_counters_diag) (void)hipFree(d.d_counters_diag);
        if (d.d_view_tab) (void)hipFree(d.d_view_tab);
        if (d.d_prog) (void)hipFree(d.d_prog);
        if (d.d_hits) (void)hipFree(d.d_hits);
        if (d.d_pick) (void)hipFree(d.d_pick);
        if (d.order.tiles.d_order) (void)hipFree(d.order.tiles.d_order);
        if (d.order.tiles.d_cost) (void)hipFree(d.order.tiles.d_cost);
        if (d.d_stage) (void)hipFree(d.d_stage);
        if (d.async_stream) (void)hipStreamDestroy(d.async_stream);
        if (d.stream) (void)hipStreamDestroy(d.stream);
    }
    delete ctx;
}

// The switches of rt_scene.h SceneOptions (A/B and fallback tests) as rt_set_scene and rt_set_scene_track read them:
// RT_<NAME>=0 turns a table off, RT_TRACE_CLUSTERS=0 the clusters, =2..16 sets the cluster size.
static SceneOptions scene_options_from_env() {
    auto off = [](const char* name) {
        const char* v = std::getenv(name);
        return v && std::strcmp(v, "0") == 0;
    };
    SceneOptions opt;
    opt.shadow_grid = !off("RT_SHADOW_GRID");
    if (const char* cv = std::getenv("RT_TRACE_CLUSTERS")) opt.cluster_size = std::atoi(cv);
    opt.shadow_pre = !off("RT_SHADOW_PRE");
    opt.shadow_groups = !off("RT_SHADOW_GROUPS");
    opt.mirror_box = !off("RT_MIRROR_BOX");
    opt.dark_skip = !off("RT_DARK_SKIP");
    opt.prim_foot = !off("RT_PRIM_FOOT");
    opt.uniform_plane = !off("RT_UNIFORM_PLANE");
    return opt;
}

// The argument checks rt_set_scene and rt_set_scene_track (per frame: the same counts) share.
static int check_scene_args(rt_ctx* ctx, const char* who, const void* spheres, int n_spheres, const void* planes, int n_planes,
                            const void* lights, int n_lights, int recursion_limit) {
    if (n_spheres < 0 || n_planes < 0 || n_lights < 0 || (n_spheres && !spheres) || (n_planes && !planes) ||
        (n_lights && !lights))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: bad primitive arrays", who);
    if (recursion_limit < 0) return fail(ctx, RT_ERR_INVALID_ARG, "recursion_limit must be >= 0");
    if (n_lights > RT_MAX_LIGHTS)
        return fail(ctx, RT_ERR_UNSUPPORTED, "n_lights %d > RT_MAX_LIGHTS (%d)", n_lights, RT_MAX_LIGHTS);
    if (recursion_limit > RT_MAX_RECURSION_LIMIT)
        return fail(ctx, RT_ERR_UNSUPPORTED, "recursion_limit %d > RT_MAX_RECURSION_LIMIT (%d)", recursion_limit,
                    RT_MAX_RECURSION_LIMIT);
    return RT_OK;
}

int rt_set_scene(rt_ctx* ctx, const rt_sphere* spheres, int n_spheres, const rt_plane* planes, int n_planes,
                 const rt_light* lights, int n_lights, rt_vec3 ambient, int recursion_limit) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    RT_TRY(check_scene_args(ctx, "rt_set_scene", spheres, n_spheres, planes, n_planes, lights, n_lights, recursion_limit));
    const SceneOptions opt = scene_options_from_env();
    SceneLayout L = scene_build(spheres, n_spheres, planes, n_planes, lights, n_lights, ambient, recursion_limit, opt);
    for (Device& d : ctx->dev) {
        DeviceGuard guard(d.id);
        // frames in flight on any stream (rt_render_device callers', the async slots) read
        // the scene being replaced
        HIP_TRY(ctx, hipDeviceSynchronize());
        int rc = grow(ctx, &d.d_scene, &d.scene_cap, L.bytes);
        if (rc != RT_OK) return rc;
        HIP_TRY(ctx, hipMemcpy(d.d_scene, L.host_blob.data(), L.bytes, hipMemcpyHostToDevice));
    }
    ctx->layout = std::move(L);
    ctx->has_scene = true;
    ctx->view_ok = false;
    ctx->scene_gen++;
    return RT_OK;
}

// The frames of a track are built by a thread pool (rt_scene.h track_build): a frame's build costs more than its
// trace in both families -- about 1 ms for 8 spheres and 2 lights (the shadow pre-test's group records) against a
// 20 us trace at 1080p, about 4 ms for 64 spheres and 4 lights (the shadow grids) against 0.3 ms at 4K.
// min(16, n_frames) threads, never sized by the machine; the image does not depend on the thread count.
static int track_threads(int n_frames) { return std::min(16, n_frames); }

int rt_set_scene_track(rt_ctx* ctx, const rt_sphere* spheres, int n_spheres, const rt_plane* planes, int n_planes,
                       const rt_light* lights, int n_lights, const rt_vec3* ambients, int recursion_limit, int n_frames) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    if (!ambients) return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_scene_track: NULL ambients");
    if ((n_spheres > 0 && !spheres) || (n_planes > 0 && !planes) || (n_lights > 0 && !lights))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_scene_track: bad primitive arrays");
    if (n_frames <= 0 || n_frames > RT_MAX_PATH_FRAMES)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_scene_track: a frame count outside 1..%d", RT_MAX_PATH_FRAMES);
    RT_TRY(check_scene_args(ctx, "rt_set_scene_track", spheres, n_spheres, planes, n_planes, lights, n_lights, recursion_limit));
    const SceneOptions opt = scene_options_from_env();
    const size_t frame_bytes = track_frame_bytes(n_spheres, n_planes, n_lights, opt);
    if (frame_bytes > RT_MAX_TRACK_BYTES / (size_t)n_frames)
        return fail(ctx, RT_ERR_OOM, "rt_set_scene_track: %d frames of %zu bytes exceed RT_MAX_TRACK_BYTES (%zu)", n_frames,
                    frame_bytes, (size_t)RT_MAX_TRACK_BYTES);
    SceneTrack T;
    const int tb = track_build(spheres, n_spheres, planes, n_planes, lights, n_lights, ambients, recursion_limit, n_frames, opt,
                               track_threads(n_frames), &T);
    if (tb == TRACK_CLUSTERS)
        return fail(ctx, RT_ERR_UNSUPPORTED, "rt_set_scene_track: the frames' cluster counts differ");
    if (tb != TRACK_OK || T.stride % 256 != 0)
        return fail(ctx, RT_ERR_UNSUPPORTED, "rt_set_scene_track: the frames' scene layouts differ");
    if (!ctx->dev.empty()) {
        Device& d = ctx->dev[0];
        DeviceGuard guard(d.id);
        // launches in flight on any stream may read the track being replaced
        HIP_TRY(ctx, hipDeviceSynchronize());
        ctx->has_track = false;
        RT_TRY(grow(ctx, &d.d_track, &d.track_cap, T.image.size()));
        HIP_TRY(ctx, hipMemcpy(d.d_track, T.image.data(), T.image.size(), hipMemcpyHostToDevice));
    }
    std::vector<unsigned char>().swap(T.image);
    ctx->track = std::move(T);
    ctx->has_track = true;
    return RT_OK;
}

int rt_clear_scene_track(rt_ctx* ctx) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    if (!ctx->dev.empty()) {
        Device& d = ctx->dev[0];
        DeviceGuard guard(d.id);
        if (d.d_track) {
            HIP_TRY(ctx, hipDeviceSynchronize());  // (launches that still read it)
            (void)hipFree(d.d_track);
        }
        d.d_track = nullptr, d.track_cap = 0;
    }
    ctx->has_track = false;
    ctx->track = SceneTrack{};
    return RT_OK;
}

int rt_set_view_height(rt_ctx* ctx, int view_height) {
    if (!ctx || view_height < 0) return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_view_height: bad arguments");
    ctx->view_height = view_height;
    return RT_OK;
}

int rt_set_supersampling(rt_ctx* ctx, int k) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_set_supersampling: NULL context");
    if (k != 1 && k != 2 && k != 4 && k != 8)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_supersampling: factor %d is not 1, 2, 4 or 8", k);
    ctx->ss_log2 = k == 8 ? 3 : k == 4 ? 2 : k == 2 ? 1 : 0;
    return RT_OK;
}

int rt_get_supersampling(const rt_ctx* ctx, int* out_k) {
    if (!ctx || !out_k) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_get_supersampling: NULL argument");
    *out_k = 1 << ctx->ss_log2;
    return RT_OK;
}

int rt_set_path_supersampling(rt_ctx* ctx, int k) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_set_path_supersampling: NULL context");
    if (k != 1 && k != 2 && k != 4 && k != 8)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_path_supersampling: factor %d is not 1, 2, 4 or 8", k);
    ctx->path_ss_log2 = k == 8 ? 3 : k == 4 ? 2 : k == 2 ? 1 : 0;
    return RT_OK;
}

int rt_get_path_supersampling(const rt_ctx* ctx, int* out_k) {
    if (!ctx || !out_k) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_get_path_supersampling: NULL argument");
    *out_k = 1 << ctx->path_ss_log2;
    return RT_OK;
}

int rt_set_adaptive_sampling(rt_ctx* ctx, int threshold) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_set_adaptive_sampling: NULL context");
    if (threshold < 0 || threshold > 256)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_adaptive_sampling: threshold %d is not in 0..256", threshold);
    ctx->adapt_thr = threshold;
    return RT_OK;
}

int rt_get_adaptive_sampling(const rt_ctx* ctx, int* out_threshold) {
    if (!ctx || !out_threshold) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_get_adaptive_sampling: NULL argument");
    *out_threshold = ctx->adapt_thr;
    return RT_OK;
}

int rt_set_path_adaptive_sampling(rt_ctx* ctx, int threshold) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_set_path_adaptive_sampling: NULL context");
    if (threshold < 0 || threshold > 256)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_path_adaptive_sampling: threshold %d is not in 0..256", threshold);
    ctx->path_adapt_thr = threshold;
    return RT_OK;
}

int rt_get_path_adaptive_sampling(const rt_ctx* ctx, int* out_threshold) {
    if (!ctx || !out_threshold) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_get_path_adaptive_sampling: NULL argument");
    *out_threshold = ctx->path_adapt_thr;
    return RT_OK;
}

int rt_set_shutter_adaptive_sampling(rt_ctx* ctx, int threshold) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_set_shutter_adaptive_sampling: NULL context");
    if (threshold < 0 || threshold > 256)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_shutter_adaptive_sampling: threshold %d is not in 0..256", threshold);
    ctx->shutter_adapt_thr = threshold;
    return RT_OK;
}

int rt_get_shutter_adaptive_sampling(const rt_ctx* ctx, int* out_threshold) {
    if (!ctx || !out_threshold) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_get_shutter_adaptive_sampling: NULL argument");
    *out_threshold = ctx->shutter_adapt_thr;
    return RT_OK;
}

int rt_set_progressive(rt_ctx* ctx, int k) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_set_progressive: NULL context");
    const int s = prog_log2(k);
    if (s < 0) return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_progressive: factor %d is not 1, 2, 4 or 8", k);
    if (s == ctx->prog_log2) return RT_OK;
    ctx->prog_log2 = s;  // (the factor is part of the view key: the next Tick starts a run)
    if (s == 0) {        // off: the accumulators go, once nothing in flight uses them
        RT_TRY(flush_hand(ctx));
        for (Device& d : ctx->dev) {
            if (!d.d_prog) continue;
            DeviceGuard guard(d.id);
            HIP_TRY(ctx, hipDeviceSynchronize());
            (void)hipFree(d.d_prog);
            d.d_prog = nullptr, d.prog_cap = 0, d.prog_touched = false;
        }
        ctx->prog_run.count = 0;
    }
    return RT_OK;
}

int rt_get_progressive(const rt_ctx* ctx, int* out_k, int* out_samples) {
    if (!ctx || !out_k || !out_samples) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_get_progressive: NULL argument");
    *out_k = 1 << ctx->prog_log2;
    *out_samples = ctx->prog_last;
    return RT_OK;
}

int rt_reset_progressive(rt_ctx* ctx) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_reset_progressive: NULL context");
    ctx->prog_run.count = 0;
    return RT_OK;
}

int rt_set_camera(rt_ctx* ctx, const rt_camera* camera) {
    if (!ctx || !camera) return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_camera: NULL argument");
    ctx->cam = *camera;
    return RT_OK;
}

int rt_get_camera(const rt_ctx* ctx, rt_camera* camera) {
    if (!ctx || !camera) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_get_camera: NULL argument");
    *camera = ctx->cam;
    return RT_OK;
}

// The camera basis and view plane of RayTracer.cs:511-523 and :892-896 (rt_view.h camera_view).
int rt_camera_view(const rt_camera* c, int width, int height, rt_view* out) {
    if (!c || !out || width <= 0 || height <= 0) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_camera_view: bad args");
    return camera_view(*c, width, height, out);
}

// OnKeyPress, RayTracer.cs:543-554: position +/- direction * (0.05, 0.05, 0.05).
int rt_camera_on_key(rt_camera* c, int key) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_camera_on_key: NULL camera");
    rt_view v;
    rt_camera_view(c, 1, 1, &v);
    const float m = 0.05f;
    rt_vec3 dir;
    float sign;
    switch (key) {
        case RT_KEY_W: dir = v.forward, sign = 1.0f; break;
        case RT_KEY_A: dir = v.right, sign = -1.0f; break;
        case RT_KEY_S: dir = v.forward, sign = -1.0f; break;
        case RT_KEY_D: dir = v.right, sign = 1.0f; break;
        case RT_KEY_SPACE: dir = v.up, sign = -1.0f; break;
        case RT_KEY_SHIFT: dir = v.up, sign = 1.0f; break;
        default: return RT_OK;  // `_ => _cameraPosition`
    }
    const rt_vec3 d{dir.x * m, dir.y * m, dir.z * m};
    if (sign > 0) c->position = rt_vec3{c->position.x + d.x, c->position.y + d.y, c->position.z + d.z};
    else c->position = rt_vec3{c->position.x - d.x, c->position.y - d.y, c->position.z - d.z};
    return RT_OK;
}

// OnMouseMove, RayTracer.cs:1058-1061: _yaw += DeltaX / 360; _pitch += DeltaY / 360.
int rt_camera_on_mouse_move(rt_camera* c, float dx, float dy) {
    if (!c) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_camera_on_mouse_move: NULL camera");
    c->yaw = c->yaw + dx / 360.0f;
    c->pitch = c->pitch + dy / 360.0f;
    return RT_OK;
}

int rt_render_device(rt_ctx* ctx, int width, int height, int32_t* d_pixels, void* hip_stream) {
    int rc = check_ctx(ctx, width, height);
    if (rc != RT_OK) return rc;
    if (!d_pixels) return fail(ctx, RT_ERR_INVALID_ARG, "NULL d_pixels");
    TickScope tick(ctx);
    RT_TRY(tick.begin(width, height));
    Device& d0 = ctx->dev[0];
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the HIP null stream
    if (ctx->n_gpus == 1 && !ctx->rccl_gather) {
        DeviceGuard guard(d0.id);
        TraceReq q{width, height, height, 0, 1, d_pixels};
        q.acc = tick_acc(ctx, d0);
        rc = trace_bands(ctx, d0, s, q);
    } else {
        // n > 1: the workers start after the work already on the caller's stream (d_pixels may be in use)
        // and the caller's stream waits for the whole frame
        for (Device& d : ctx->dev)
            if (!d.ev[Device::EV_JOIN]) {  // (made on its own device)
                DeviceGuard guard(d.id);
                RT_TRY(ensure_event(ctx, &d.ev[Device::EV_JOIN]));
            }
        {
            DeviceGuard guard(d0.id);
            HIP_TRY(ctx, hipEventRecord(d0.ev[Device::EV_JOIN], s));
        }
        for (Device& d : ctx->dev) {
            DeviceGuard guard(d.id);
            HIP_TRY(ctx, hipStreamWaitEvent(d.stream, d0.ev[Device::EV_JOIN], 0));
        }
        if (ctx->shared_device) {  // one device: every worker writes its bands straight into the frame
            for (int g = 0; g < ctx->n_gpus && rc == RT_OK; ++g) {
                TraceReq q{width, height, TICK_BAND_ROWS, g, ctx->n_gpus, d_pixels, RT_BANDS_FRAME};
                q.acc = tick_acc(ctx, ctx->dev[(size_t)g]);
                rc = trace_bands(ctx, ctx->dev[(size_t)g], ctx->dev[(size_t)g].stream, q);
            }
        } else {  // the RCCL gather to device 0 over xGMI, reassembled into d_pixels on device 0's stream
            rc = gather_frame(ctx, width, height, d_pixels);
        }
        if (rc != RT_OK) return rc;
        DeviceGuard guard(d0.id);
        for (size_t g = 0; g < (ctx->shared_device ? ctx->dev.size() : 1); ++g) {
            HIP_TRY(ctx, hipEventRecord(ctx->dev[g].ev[Device::EV_JOIN], ctx->dev[g].stream));
            HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->dev[g].ev[Device::EV_JOIN], 0));
        }
    }
    if (rc == RT_OK) {
        tick.done = true;
        ctx->frames++;
        ctx->pixels += (uint64_t)width * (uint64_t)height;
    }
    return rc;
}

int rt_render_bands(rt_ctx* ctx, int width, int height, int band_rows, int band_first, int band_step,
                    int32_t* d_out, void* hip_stream, int* out_n_bands) {
    return rt_render_bands_ex(ctx, width, height, band_rows, band_first, band_step, d_out, RT_BANDS_INT32, hip_stream,
                              out_n_bands);
}

int rt_render_bands_ex(rt_ctx* ctx, int width, int height, int band_rows, int band_first, int band_step, void* d_out,
                       int format, void* hip_stream, int* out_n_bands) {
    RT_TRY(check_ctx(ctx, width, height));
    RT_TRY(check_band_args(ctx, "rt_render_bands", band_rows, band_first, band_step, d_out, format));
    RT_TRY(check_adaptive_bands(ctx, band_rows, height));
    if (ctx->n_gpus != 1) return fail(ctx, RT_ERR_INVALID_ARG, "rt_render_bands needs a single-GPU context");
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    const int nb = bands_of(height, band_rows, band_first, band_step);
    const int rc = trace_bands(ctx, d, (hipStream_t)hip_stream,  // (NULL = the HIP null stream)
                               TraceReq{width, height, band_rows, band_first, band_step, (int32_t*)d_out, format});
    if (out_n_bands) *out_n_bands = nb;
    if (rc == RT_OK) ctx->pixels += (uint64_t)nb * band_rows * width;
    return rc;
}

int rt_render_bands_batch(rt_ctx* ctx, int width, int height, int band_rows, int band_first, int band_step,
                          int n_frames, void* d_out, size_t frame_stride_bytes, int format, void* hip_stream,
                          int* out_n_bands) {
    RT_TRY(check_ctx(ctx, width, height));
    RT_TRY(check_band_args(ctx, "rt_render_bands_batch", band_rows, band_first, band_step, d_out, format));
    RT_TRY(check_adaptive_bands(ctx, band_rows, height));
    if (n_frames <= 0 || n_frames > 65535)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_render_bands_batch: bad band arguments");
    if (ctx->n_gpus != 1) return fail(ctx, RT_ERR_INVALID_ARG, "rt_render_bands_batch needs a single-GPU context");
    const int nb = bands_of(height, band_rows, band_first, band_step);
    if (n_frames > 1 && frame_stride_bytes < band_output_bytes(width, height, nb, band_rows, format))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_render_bands_batch: frame stride smaller than a frame's output");
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    const TraceReq q{width, height, band_rows, band_first, band_step, (int32_t*)d_out, format, n_frames, frame_stride_bytes};
    const int rc = trace_bands(ctx, d, (hipStream_t)hip_stream, q);
    if (out_n_bands) *out_n_bands = nb;
    if (rc == RT_OK) ctx->pixels += (uint64_t)nb * band_rows * width * (uint64_t)n_frames;
    return rc;
}

int rt_scatter_bands(rt_ctx* ctx, int width, int height, int band_rows, int band_first, int band_step,
                     const int32_t* d_bands, int32_t* d_frame, void* hip_stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    if (width <= 0 || height <= 0 || band_rows <= 0 || band_first < 0 || band_step <= 0 || !d_bands || !d_frame)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_scatter_bands: bad arguments");
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the HIP null stream
    const int nb = bands_of(height, band_rows, band_first, band_step);
    int e = launch_scatter_bands(d_bands, d_frame, width, height, band_rows, band_first, band_step, nb, s);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "scatter launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int rt_scatter_gathered(rt_ctx* ctx, int width, int height, int band_rows, int world, const void* d_gathered,
                        size_t slot_bytes, int format, int32_t* d_frame, void* hip_stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    const size_t bpp = format == RT_BANDS_INT32 ? 4 : 3;
    if (width <= 0 || height <= 0 || band_rows <= 0 || world <= 0 || !d_gathered || !d_frame ||
        (format != RT_BANDS_INT32 && format != RT_BANDS_RGB24) ||
        slot_bytes < (size_t)bands_of(height, band_rows, 0, world) * band_rows * width * bpp)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_scatter_gathered: bad arguments");
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    int e = launch_scatter_gathered((const unsigned char*)d_gathered, slot_bytes, format, d_frame, width, height,
                                    band_rows, world, hip_stream);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "scatter launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

// Tile-codec wire geometry (raytracer_hip/tilecodec.py.layout): the tile grid of the
// largest band set, n_frames grids per batch, chunks of 64 tiles.
static bool codec_geom(int width, int height, int band_rows, int world, int n_frames, rtk::CodecGeom& g,
                       rt_wire_layout* lay) {
    if (width <= 0 || height <= 0 || band_rows <= 0 || world <= 0 || n_frames <= 0) return false;
    const int rows = std::max(1, bands_of(height, band_rows, 0, world)) * band_rows;
    const long long tx = (width + 7) / 8, ty = (rows + 7) / 8;
    const long long tpf = tx * ty, nt = tpf * (long long)n_frames;
    if (nt > (1LL << 26)) return false;  // 32-bit word offsets (<= 48 words per tile)
    const long long nc = (nt + 7) / 8;  // chunks of 8 tiles (one wave's)
    g = rtk::CodecGeom{};
    g.W = width, g.H = height, g.band_rows = band_rows, g.world = world;
    g.tiles_x = (int)tx, g.tiles_y = (int)ty, g.tiles_per_frame = (int)tpf, g.n_tiles = (int)nt, g.n_chunks = (int)nc;
    g.fixed_bytes = ((size_t)16 + 4 * (size_t)nt + 4 * (size_t)nc + 7) / 8 * 8;  // header, tile headers, chunk bases
    if (lay) {
        lay->fixed_bytes = g.fixed_bytes;
        lay->max_bytes = g.fixed_bytes + 8 * 24 * (size_t)nt;
        lay->tiles_x = (int32_t)tx, lay->tiles_y = (int32_t)ty, lay->tiles_per_frame = (int32_t)tpf;
        lay->n_frames = n_frames, lay->n_tiles = (int32_t)nt, lay->n_chunks = (int32_t)nc;
    }
    return true;
}

// Codec scratch of device d for geometry g (staged segments + workgroup sums), grown on demand:
// the previous user of the old buffer may still run, so growing waits for the device first.
static int ensure_stage(rt_ctx* ctx, Device& d, const rtk::CodecGeom& g) {
    const size_t need = encode_stage_bytes(g);
    if (need > d.stage_cap) {
        HIP_TRY(ctx, hipDeviceSynchronize());
        if (d.d_stage) HIP_TRY(ctx, hipFree(d.d_stage));
        d.d_stage = nullptr, d.stage_cap = 0;
        HIP_TRY(ctx, hipMalloc(&d.d_stage, need));
        d.stage_cap = need;
    }
    return RT_OK;
}

int rt_wire_layout_of(int width, int height, int band_rows, int world, int n_frames, rt_wire_layout* out) {
    rtk::CodecGeom g;
    if (!out || !codec_geom(width, height, band_rows, world, n_frames, g, out))
        return fail(nullptr, RT_ERR_INVALID_ARG, "rt_wire_layout_of: bad arguments");
    return RT_OK;
}

int rt_encode_bands(rt_ctx* ctx, int width, int height, int band_rows, int rank, int world, const int32_t* d_bands,
                    size_t frame_stride, int n_frames, void* d_wire, int64_t* d_wire_bytes, void* hip_stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    rtk::CodecGeom g;
    if (!codec_geom(width, height, band_rows, world, n_frames, g, nullptr) || rank < 0 || rank >= world ||
        !d_bands || !d_wire || ((uintptr_t)d_wire & 7) != 0 ||
        frame_stride < (size_t)std::max(1, bands_of(height, band_rows, 0, world)) * band_rows * width)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_encode_bands: bad arguments");
    g.rank = rank;
    g.n_bands = bands_of(height, band_rows, rank, world);
    g.frame_stride = frame_stride;
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    const int rc = ensure_stage(ctx, d, g);
    if (rc != RT_OK) return rc;
    d.staged.valid = false;  // the scratch now holds this encode's segments
    int e = launch_encode_bands(d_bands, (unsigned char*)d_wire, g, d_wire_bytes, d.d_stage, hip_stream);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "encode launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int rt_render_bands_tiles(rt_ctx* ctx, int width, int height, int band_rows, int rank, int world, int frame0,
                          int n_frames, int batch_frames, void* d_wire, void* hip_stream) {
    RT_TRY(check_ctx(ctx, width, height, false));
    if (ctx->ss_log2 > 0)
        return fail(ctx, RT_ERR_UNSUPPORTED, "rt_render_bands_tiles does not supersample (rt_set_supersampling(ctx, 1) first)");
    rtk::CodecGeom g;
    if (!codec_geom(width, height, band_rows, world, batch_frames, g, nullptr) || rank < 0 || rank >= world ||
        frame0 < 0 || n_frames <= 0 || n_frames > 65535 || frame0 + n_frames > batch_frames || !d_wire ||
        ((uintptr_t)d_wire & 7) != 0)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_render_bands_tiles: bad arguments");
    if (ctx->n_gpus != 1) return fail(ctx, RT_ERR_INVALID_ARG, "rt_render_bands_tiles needs a single-GPU context");
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    RT_TRY(ensure_stage(ctx, d, g));
    const EncTarget enc{(unsigned char*)d_wire, (uint32_t*)d.d_stage, g.tiles_x, g.tiles_per_frame, frame0};
    TraceReq q{width, height, band_rows, rank, world, (int32_t*)d_wire};
    q.n_frames = n_frames, q.enc = &enc;
    const int rc = trace_bands(ctx, d, (hipStream_t)hip_stream, q);
    if (rc == RT_OK) {
        ctx->pixels += (uint64_t)bands_of(height, band_rows, rank, world) * band_rows * width * (uint64_t)n_frames;
        if (frame0 == 0 || !d.staged.valid || d.staged.wire != d_wire)
            d.staged = {true, width, height, band_rows, rank, world, batch_frames, d_wire};
    }
    return rc;
}

int rt_finish_wire(rt_ctx* ctx, int width, int height, int band_rows, int rank, int world, int n_frames,
                   void* d_wire, int64_t* d_wire_bytes, void* hip_stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    rtk::CodecGeom g;
    if (!codec_geom(width, height, band_rows, world, n_frames, g, nullptr) || rank < 0 || rank >= world ||
        !d_wire || ((uintptr_t)d_wire & 7) != 0)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_finish_wire: bad arguments");
    if (ctx->n_gpus != 1) return fail(ctx, RT_ERR_INVALID_ARG, "rt_finish_wire needs a single-GPU context");
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    // only the batch rt_render_bands_tiles staged last, with the same geometry and wire
    const auto& sb = d.staged;
    if (!d.d_stage || encode_stage_bytes(g) > d.stage_cap || !sb.valid || sb.W != width || sb.H != height ||
        sb.band_rows != band_rows || sb.rank != rank || sb.world != world || sb.wire != d_wire ||
        n_frames > sb.batch_frames)
        return fail(ctx, RT_ERR_INVALID_ARG,
                    "rt_finish_wire: no rt_render_bands_tiles batch of this geometry and wire with >= %d frames",
                    n_frames);
    const int traced_rows = (bands_of(height, band_rows, rank, world) * band_rows + 7) / 8;
    int e = launch_finish_wire((unsigned char*)d_wire, g, traced_rows, d_wire_bytes, d.d_stage, hip_stream);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "finish launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int rt_decode_gathered(rt_ctx* ctx, int width, int height, int band_rows, int world, int first_rank,
                       const void* d_gathered, size_t rank_stride, int n_frames, int32_t* d_frames,
                       size_t frame_stride, void* hip_stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    rtk::CodecGeom g;
    rt_wire_layout lay;
    if (!codec_geom(width, height, band_rows, world, n_frames, g, &lay) || !d_gathered || !d_frames ||
        first_rank < 0 || first_rank > world || ((uintptr_t)d_gathered & 7) != 0 || (rank_stride & 7) != 0 ||
        (world - first_rank > 1 && rank_stride < lay.max_bytes) || frame_stride < (size_t)width * height)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_decode_gathered: bad arguments");
    if (first_rank == world) return RT_OK;
    g.rank = first_rank;
    g.frame_stride = frame_stride;
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    int e = launch_decode_gathered((const unsigned char*)d_gathered, rank_stride, d_frames, g, hip_stream);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "decode launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int rt_comm_probe(void) {
    std::string err;
    if (!g_rccl.load(err)) return fail(nullptr, RT_ERR_RCCL, "%s", err.c_str());
    return RT_OK;
}

int rt_comm_unique_id(void* out_id) {
    if (!out_id) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_comm_unique_id: NULL");
    std::string err;
    if (!g_rccl.load(err)) return fail(nullptr, RT_ERR_RCCL, "%s", err.c_str());
    ncclUniqueId id;
    const ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != 0) return fail(nullptr, RT_ERR_RCCL, "ncclGetUniqueId: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    std::memcpy(out_id, id.internal, RT_COMM_ID_BYTES);
    return RT_OK;
}

int rt_comm_init(rt_ctx* ctx, int world, int rank, const void* id) {
    if (!ctx || !id || world < 1 || rank < 0 || rank >= world)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_comm_init: bad arguments");
    if (ctx->n_gpus != 1 || ctx->rccl_gather)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_comm_init needs a single-GPU context without RT_CREATE_RCCL_GATHER");
    Device& d = ctx->dev[0];
    if (d.comm) return fail(ctx, RT_ERR_INVALID_ARG, "rt_comm_init: the context already has a communicator");
    std::string err;
    if (!g_rccl.load(err)) return fail(ctx, RT_ERR_RCCL, "%s", err.c_str());
    DeviceGuard guard(d.id);
    ncclUniqueId uid;
    std::memcpy(uid.internal, id, RT_COMM_ID_BYTES);
    const ncclResult_t r = g_rccl.CommInitRank(&d.comm, world, uid, rank);
    if (r != 0) {
        d.comm = nullptr;
        return fail(ctx, RT_ERR_RCCL, "ncclCommInitRank: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    }
    d.comm_rank = rank, d.comm_world = world;
    return RT_OK;
}

int rt_comm_allreduce_max_i64(rt_ctx* ctx, int64_t* d_values, int count, void* hip_stream) {
    if (!ctx || !d_values || count < 1) return fail(ctx, RT_ERR_INVALID_ARG, "rt_comm_allreduce_max_i64: bad arguments");
    Device& d = ctx->dev[0];
    if (!d.comm || !d.comm_world) return fail(ctx, RT_ERR_INVALID_ARG, "rt_comm_allreduce_max_i64: no rt_comm_init");
    DeviceGuard guard(d.id);
    const ncclResult_t r =
        g_rccl.AllReduce(d_values, d_values, (size_t)count, ncclInt64, ncclMax, d.comm, (hipStream_t)hip_stream);
    if (r != 0) return fail(ctx, RT_ERR_RCCL, "ncclAllReduce: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    return RT_OK;
}

int rt_comm_gather(rt_ctx* ctx, const void* d_send, size_t n_bytes, void* d_recv, size_t recv_stride, int rotate,
                   void* hip_stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    Device& d = ctx->dev[0];
    if (!d.comm || !d.comm_world) return fail(ctx, RT_ERR_INVALID_ARG, "rt_comm_gather: no rt_comm_init");
    const int world = d.comm_world, rank = d.comm_rank;
    if ((n_bytes && !d_send) || (rank == 0 && n_bytes && (!d_recv || recv_stride < n_bytes)))
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_comm_gather: bad arguments");
    if (!n_bytes) return RT_OK;
    DeviceGuard guard(d.id);
    const hipStream_t st = (hipStream_t)hip_stream;
    auto slot = [&](int r) { return (size_t)(((r - rotate) % world + world) % world) * recv_stride; };
    if (world > 1) {
        if (g_rccl.GroupStart() != 0) return fail(ctx, RT_ERR_RCCL, "ncclGroupStart failed");
        ncclResult_t r = 0;
        if (rank != 0) {
            r = g_rccl.Send(d_send, n_bytes, ncclUint8, 0, d.comm, st);
        } else {
            for (int q = 1; q < world && r == 0; ++q)
                r = g_rccl.Recv((char*)d_recv + slot(q), n_bytes, ncclUint8, q, d.comm, st);
        }
        const ncclResult_t e = g_rccl.GroupEnd();
        if (r != 0 || e != 0)
            return fail(ctx, RT_ERR_RCCL, "ncclSend/Recv: %s",
                        g_rccl.GetErrorString ? g_rccl.GetErrorString(r ? r : e) : "?");
    }
    if (rank == 0)  // rank 0's own slot
        HIP_TRY(ctx, hipMemcpyAsync((char*)d_recv + slot(0), d_send, n_bytes, hipMemcpyDeviceToDevice, st));
    return RT_OK;
}

int rt_register_host(rt_ctx* ctx, void* host_ptr, size_t bytes) {
    if (!ctx || !host_ptr || !bytes) return fail(ctx, RT_ERR_INVALID_ARG, "rt_register_host: bad arguments");
    DeviceGuard guard(ctx->dev[0].id);
    // mapped into every device's address space: each worker's copy kernel writes its own bands (a
    // coarse-grained lock, hipExtHostRegisterCoarseGrained, measured the same copy rates: r05f)
    hipError_t e = hipHostRegister(host_ptr, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        HIP_TRY(ctx, hipHostRegister(host_ptr, bytes, hipHostRegisterDefault));
    }
    rt_ctx::HostRange r{(char*)host_ptr, bytes, std::vector<char*>(ctx->dev.size(), nullptr)};
    for (size_t g = 0; g < ctx->dev.size(); ++g) {
        DeviceGuard dg(ctx->dev[g].id);
        void* mapped = nullptr;
        if (hipHostGetDevicePointer(&mapped, host_ptr, 0) == hipSuccess && mapped)
            r.mapped[g] = (char*)mapped;
        else
            (void)hipGetLastError();  // not mapped on this device: its hand-off takes the runtime's copies
    }
    ctx->host_ranges.push_back(std::move(r));
    return RT_OK;
}

int rt_unregister_host(rt_ctx* ctx, void* host_ptr) {
    if (!ctx || !host_ptr) return fail(ctx, RT_ERR_INVALID_ARG, "rt_unregister_host: bad arguments");
    // a hand-off still pending into this range is written first: nothing may touch it afterwards
    int rc = rt_wait(ctx);
    if (rc != RT_OK) return rc;
    for (size_t i = 0; i < ctx->host_ranges.size(); ++i)
        if (ctx->host_ranges[i].host == (char*)host_ptr) {
            ctx->host_ranges.erase(ctx->host_ranges.begin() + (long)i);
            break;
        }
    DeviceGuard guard(ctx->dev[0].id);
    HIP_TRY(ctx, hipHostUnregister(host_ptr));
    return RT_OK;
}

namespace {
// How a registered frame's hand-off is copied in the synchronous Tick (RT_TICK_COPY): runtime -- the
// runtime's copy engine after the trace, same stream; kernel -- the copy kernel through the device-mapped
// address, chunked (chunk c's copy rides in chunk c+1's launch, the last by the copy kernel alone);
// stream -- chunked, each chunk's copy by the copy engine on a second stream after the chunk's trace
// (event-ordered), so it runs under the next chunk's trace.  Default: stream (r05k, one GPU: C5 271 ->
// 391 fps at 4 chunks, C4 1,028 -> 1,250; the copy kernel writes host memory at ~35 GB/s against the
// copy engine's ~52).  A share of one chunk (a 1080p frame) takes the runtime's copy after the trace at
// n = 1 and the copy kernel at n > 1, whose bands are too short for pitched copies.
enum TickCopy { TICK_RUNTIME = 0, TICK_KERNEL = 1, TICK_STREAM = 2 };
TickCopy tick_copy_mode() {
    if (const char* e = std::getenv("RT_TICK_COPY")) {
        if (std::strcmp(e, "kernel") == 0) return TICK_KERNEL;
        if (std::strcmp(e, "runtime") == 0) return TICK_RUNTIME;
    }
    return TICK_STREAM;
}

// Chunks of a worker's share in a synchronous Tick.  RT_TICK_CHUNKS=1..8 fixes the count; by default one
// chunk per ~2 M pixels of the share, at most 8 (1080p: 1; C4 at n = 1: 4; C5: 8 at n = 1, 2 at n = 8;
// r05k: C4 4 chunks 1,250 fps against 8 chunks 1,016, C5 8 chunks ~ 4).
int tick_chunks(const rt_ctx* ctx, int W, int H) {
    if (const char* e = std::getenv("RT_TICK_CHUNKS")) {
        const int k = std::atoi(e);
        if (k >= 1 && k <= 8) return k;
    }
    const double share = (double)W * H / ctx->n_gpus;
    return (int)std::min(8.0, std::max(1.0, std::floor(share / 2.0e6 + 0.5)));
}

// The synchronous Tick of every worker: each traces its band set and copies it into `pixels` on its
// own stream (its own device and PCIe link); the host waits for all of them at the end.
int tick_sync(rt_ctx* ctx, int W, int H, int32_t* pixels) {
    const int n = ctx->n_gpus;
    const size_t frame_bytes = (size_t)W * H * sizeof(int32_t);
    const int chunks = tick_chunks(ctx, W, H);
    for (int g = 0; g < n; ++g) {
        Device& d = ctx->dev[(size_t)g];
        DeviceGuard guard(d.id);
        int32_t* mapped = mapped_host(ctx, g, pixels, frame_bytes);
        const TickCopy mode = mapped ? tick_copy_mode() : TICK_RUNTIME;
        const int nc = mode != TICK_RUNTIME ? chunks : 1;
        const Share sh = share_of(W, H, g, n, nc > 1);
        if (sh.nb <= 0) continue;
        RT_TRY(grow(ctx, (void**)&d.d_bands, &d.bands_cap, (size_t)sh.nb * sh.band_rows * W * sizeof(int32_t)));
        if (mode == TICK_STREAM && nc > 1) {  // chunk c: trace (stream) -> event -> copy engine (copy stream)
            RT_TRY(trace_and_copy_chunks(ctx, d, d.stream, sh, W, H, nc, d.d_bands, pixels, true));
            continue;
        }
        if (mode == TICK_RUNTIME || (nc == 1 && n == 1)) {  // the runtime's copy after the trace
            RT_TRY(trace_bands(ctx, d, d.stream, share_req(sh, W, H, 0, sh.nb, d.d_bands, nullptr, tick_acc(ctx, d))));
            const bool ctimed = begin_timed(ctx, d, 1);
            const int rc = runtime_band_copy(ctx, sh, W, H, d.d_bands, pixels, d.stream, mapped != nullptr, 0, sh.nb);
            end_timed(d, ctimed);
            if (rc != RT_OK) return rc;
            continue;
        }
        CopyJob prev{};
        for (int c = 0; c < nc; ++c) {
            const Bands b = chunk_bands(sh, c, nc);
            if (b.k1 <= b.k0) continue;
            const TraceReq q = share_req(sh, W, H, b.k0, b.k1, d.d_bands, &prev, tick_acc(ctx, d));
            RT_TRY(trace_bands(ctx, d, d.stream, q));
            prev = share_job(sh, W, H, b.k0, b.k1, q.out, mapped);
        }
        const bool ctimed = begin_timed(ctx, d, 1);
        const int e = launch_band_copy(prev, d.stream);
        end_timed(d, ctimed);
        if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "hand-off copy: %s", hipGetErrorString((hipError_t)e));
    }
    for (Device& d : ctx->dev) {
        DeviceGuard guard(d.id);
        HIP_TRY(ctx, hipStreamSynchronize(d.stream));
        if (d.copy_stream) HIP_TRY(ctx, hipStreamSynchronize(d.copy_stream));
    }
    return RT_OK;
}
}  // namespace

// Tick(): full frame into the caller's Surface.pixels, synchronous.
int rt_render(rt_ctx* ctx, int width, int height, int32_t* pixels) {
    RT_TRY(check_ctx(ctx, width, height));
    if (!pixels) return fail(ctx, RT_ERR_INVALID_ARG, "NULL pixels");
    RT_TRY(wait_pending_async(ctx));
    TickScope tick(ctx);
    RT_TRY(tick.begin(width, height));
    if (ctx->rccl_gather) {  // bands gathered to device 0 over RCCL, then the whole frame over its link
        Device& d0 = ctx->dev[0];
        const size_t frame_bytes = (size_t)width * height * sizeof(int32_t);
        {
            DeviceGuard guard(d0.id);
            RT_TRY(grow(ctx, (void**)&d0.d_frame, &d0.frame_cap, frame_bytes));
        }
        RT_TRY(gather_frame(ctx, width, height, d0.d_frame));
        DeviceGuard guard(d0.id);
        const bool ctimed = begin_timed(ctx, d0, 1);
        HIP_TRY(ctx, hipMemcpyAsync(pixels, d0.d_frame, frame_bytes, hipMemcpyDeviceToHost, d0.stream));
        end_timed(d0, ctimed);
        HIP_TRY(ctx, hipStreamSynchronize(d0.stream));
    } else {
        RT_TRY(tick_sync(ctx, width, height, pixels));
    }
    tick.done = true;
    ctx->frames++;
    ctx->pixels += (uint64_t)width * (uint64_t)height;
    return RT_OK;
}

namespace {
// The view table of a path launch: record i = the view of cams[i], in the cameras' own order (with a shutter of m,
// sub-frame s of output frame f is camera and record f * m + s).  lp: the launch's block, which comes out with the
// view of the last camera and the fields every camera shares (pw, ph, nearc, W).  No device call.
int view_table_fill(rt_ctx* ctx, const rt_camera* cams, int n_views, int W, int VH, LaunchParams& lp, DevView* table) {
    for (int i = 0; i < n_views; ++i) {
        const int rc = view_fill(ctx, cams[i], W, VH, lp);
        if (rc != RT_OK) return rc;
        view_record(lp, table[i]);
    }
    return RT_OK;
}

// The next table slot of the ring, free and with room for n_views records (trace_views states the rules).
int path_slot_take(rt_ctx* ctx, Device& d, int n_views, Device::PathSlot** out) {
    Device::PathSlot& ps = d.path_slot[d.path_next++ % Device::PATH_SLOTS];
    if (ps.busy) {  // the slot's last launch may still read its records
        HIP_TRY(ctx, hipEventSynchronize(ps.done));
        ps.busy = false;
    }
    RT_TRY(ensure_event(ctx, &ps.done));
    // (a slot keeps its buffers for the next call, but no more than PATH_SLOT_KEEP records of them: a call that
    // needs fewer finds a larger table shrunk to its own size, so one long path does not pin its tables for good)
    if (ps.cap < (size_t)n_views || (ps.cap > Device::PATH_SLOT_KEEP && (size_t)n_views <= Device::PATH_SLOT_KEEP)) {
        if (ps.h_views) (void)hipHostFree(ps.h_views);
        if (ps.d_views) (void)hipFree(ps.d_views);
        ps.h_views = nullptr, ps.d_views = nullptr, ps.cap = 0;
        const size_t bytes = (size_t)n_views * sizeof(DevView);
        hipError_t e = hipHostMalloc((void**)&ps.h_views, bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void**)&ps.d_views, bytes);
        if (e != hipSuccess) {
            if (ps.h_views) (void)hipHostFree(ps.h_views);
            ps.h_views = nullptr;
            return fail(ctx, RT_ERR_OOM, "view table of %d frames: %s", n_views, hipGetErrorString(e));
        }
        ps.cap = (size_t)n_views;
    }
    *out = &ps;
    return RT_OK;
}

// The launch of a camera-path call: n_frames frames (grid z), frame f with the view of cams[f].  The views are
// built on the host by view_fill -- the code behind every one-camera launch -- packed as DevView records into
// a table slot's pinned staging buffer and uploaded on `stream` ahead of the launch.  The context's camera and
// its view cache (view_lp) are not touched.  Natural tile order, one tile per workgroup, whatever n_frames.
// Nothing here waits for the device except a slot's own event; the shared view tables (view_tables) are rebuilt,
// with that function's synchronisation, only when the frame size changes, and a slot's buffers are reallocated
// only when a call brings more records than the slot holds, or finds it holding more than PATH_SLOT_KEEP.
// With a shutter (rt_render_shutter_bands, t = log2 of it > 0) the table holds n_frames << t records, sub-frame s
// of output frame f at f << t | s = cams' own order, and the launch -- still n_frames frames in grid z -- averages
// each frame's 1 << t records in the kernel (LaunchParams::shutter_log2); t = 0 is the path launch itself.
// With a scene track (trace_anim: track != nullptr, t = 0) frame j of the launch also has its own scene, track frame
// first_frame + j: record j is built against that frame's spheres and planes -- the primary constants, the screen
// boxes and the mirrored boxes all depend on them -- the block's scene pointers are set to that first frame's image,
// and grid z steps through the images by LaunchParams::scene_stride (the ANIM kernels).
// With both (rt_render_anim_shutter_bands: a track and t > 0) record j = f << t | s, sub-frame s of output frame f, is
// built against track frame first_frame + j in the same way, and LaunchParams::scene_shutter marks the launch: its
// waves step through the images by the sub-frame's record index, not by grid z (the ANIM_SHUTTER kernels).
// With rt_set_path_supersampling (ss = log2 k > 0) the launch works on the k W x k H sample frame as trace_bands does
// under rt_set_supersampling: the records and the shared view tables are built for that size, H and the band rows are in
// samples, and LaunchParams::view_ss selects the PATH_SS / SHUTTER_SS / ANIM_SS kernels, whose epilogue writes one pixel
// per k x k block.  Everything the callers do with the output stays in output pixels.
// With rt_set_path_adaptive_sampling besides (a threshold, ss > 0, no shutter: check_shutter refuses the combination)
// LaunchParams::view_adapt selects the PATH_ADAPT / ANIM_ADAPT kernels instead: the same block, records and tables, a grid
// in output tiles, and the host counts one primary ray per output pixel as for any adaptive launch (launch_counted).
// With rt_set_shutter_adaptive_sampling in effect (a threshold, ss > 0 and a shutter, t > 0) LaunchParams::shutter_adapt
// selects the SHUTTER_ADAPT / ANIM_SHUTTER_ADAPT kernels in the same way: SHUTTER_SS's block, records and tables, a grid in
// output tiles, and the host counts one primary ray per output pixel and sub-frame.  The path threshold is not read.
int trace_views(rt_ctx* ctx, Device& d, hipStream_t stream, int W, int H, const rt_camera* cams, int n_frames, int t,
                int band_rows, int first, int step, void* out, size_t frame_bytes, int fmt, const SceneTrack* track,
                int first_frame) {
    const int n_views = n_frames << t;  // (the callers bound it by RT_MAX_PATH_FRAMES)
    const int VH = ctx->view_height > 0 ? ctx->view_height : H;
    const int ss = ctx->path_ss_log2;  // (check_path / check_anim bounded the sample frame, check_shutter m k^2)
    if (H > VH) return fail(ctx, RT_ERR_INVALID_ARG, "frame height %d above the view height %d", H, ctx->view_height);
    Device::PathSlot* slot = nullptr;
    RT_TRY(path_slot_take(ctx, d, n_views, &slot));
    Device::PathSlot& ps = *slot;
    LaunchParams lp;
    std::memset(&lp, 0, sizeof lp);
    int rc = RT_OK;
    if (track) {
        for (int j = 0; j < n_views && rc == RT_OK; ++j) {
            rc = view_fill(ctx, track->frames[(size_t)(first_frame + j)], cams[j], W << ss, VH << ss, lp);
            if (rc == RT_OK) view_record(lp, ps.h_views[j]);
        }
    } else {
        rc = view_table_fill(ctx, cams, n_views, W << ss, VH << ss, lp, ps.h_views);
    }
    if (rc != RT_OK) return rc;
    lp.H = H << ss;  // the rows traced; pw, ph, nearc and W are the same for every camera (lxt / lyt: view_tables)
    if (track) {
        scene_params(ctx, d, lp, track->common, (const char*)d.d_track + (size_t)first_frame * track->stride);
        lp.scene_stride = track->stride;
        lp.scene_shutter = t > 0 ? 1 : 0;
    } else {
        scene_params(ctx, d, lp);
    }
    rc = view_tables(ctx, d, lp, ss);
    if (rc != RT_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ps.d_views, ps.h_views, (size_t)n_views * sizeof(DevView), hipMemcpyHostToDevice, stream));
    const int nb = bands_of(H, band_rows, first, step);
    lp.views = ps.d_views;
    lp.shutter_log2 = t;
    lp.band_first = first, lp.band_step = step;
    if (ss > 0) {  // (as trace_bands: a band of H rows or more is the frame as band 0, so k band_rows stays below k H)
        lp.band_rows = std::min(band_rows, H) << ss;
        lp.local_rows = nb * lp.band_rows;
        lp.ss_log2 = ss;
        lp.view_ss = 1;
        if (t == 0) lp.view_adapt = ctx->path_adapt_thr;
        else lp.shutter_adapt = ctx->shutter_adapt_thr;
    } else {
        lp.band_rows = band_rows, lp.local_rows = nb * band_rows;
    }
    lp.out = (int32_t*)out;
    lp.out_fmt = fmt;
    lp.n_frames = n_frames;
    lp.out_frame_bytes = frame_bytes;
    rc = launch_counted(ctx, d, stream, lp, track ? "anim" : "path", W, H, band_rows, first, step, nb, n_views, ss,
                        track ? (track->common.generic_pow ? 1 : 0) : -1);  // (primary rays: every sample of every sub-frame)
    if (rc != RT_OK) return rc;
    HIP_TRY(ctx, hipEventRecord(ps.done, stream));
    ps.busy = true;
    return RT_OK;
}
int trace_path(rt_ctx* ctx, Device& d, hipStream_t stream, int W, int H, const rt_camera* cams, int n_frames, int t,
               int band_rows, int first, int step, void* out, size_t frame_bytes, int fmt) {
    return trace_views(ctx, d, stream, W, H, cams, n_frames, t, band_rows, first, step, out, frame_bytes, fmt, nullptr, 0);
}
// n_frames frames of 1 << t sub-frames from track frame first_frame on, sub-frame j with cams[j] (check_anim bounds them).
int trace_anim(rt_ctx* ctx, Device& d, hipStream_t stream, int W, int H, const rt_camera* cams, int first_frame, int n_frames,
               int t, int band_rows, int first, int step, void* out, size_t frame_bytes, int fmt) {
    return trace_views(ctx, d, stream, W, H, cams, n_frames, t, band_rows, first, step, out, frame_bytes, fmt, &ctx->track,
                       first_frame);
}

// rt_set_path_supersampling in effect: the k W x k VH sample frame (VH: the view height when one is set) is bounded
// like any frame.
int check_path_samples(rt_ctx* ctx, const char* who, int W, int H) {
    const int s = ctx->path_ss_log2;
    const int VH = ctx->view_height > 0 ? ctx->view_height : H;
    if (s > 0 && ((long long)W << s) * ((long long)VH << s) > (1LL << 31) - 1)
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: frame size %dx%d at path supersampling factor %d exceeds 2^31 - 1 samples", who, W,
                    VH, 1 << s);
    return RT_OK;
}

// rt_set_path_adaptive_sampling in effect (a threshold and a path factor above 1), or, for a call with a shutter above 1
// (t > 0), rt_set_shutter_adaptive_sampling: the band rule of any adaptive launch (rt_internal.h adaptive_band_ok), asked
// by the band calls before they touch the device.
int check_path_adaptive_bands(rt_ctx* ctx, const char* who, int band_rows, int H, int t) {
    if (ctx->path_ss_log2 > 0 && (t > 0 ? ctx->shutter_adapt_thr : ctx->path_adapt_thr) > 0 && !adaptive_band_ok(band_rows, H))
        return fail(ctx, RT_ERR_UNSUPPORTED,
                    "%s: adaptive sampling needs bands of a multiple of 8 rows, or one band of the whole frame (band_rows %d, height %d)",
                    who, band_rows, H);
    return RT_OK;
}

int check_path(rt_ctx* ctx, const char* who, int W, int H, const rt_camera* cams, int n_frames) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    if (!cams || n_frames <= 0 || n_frames > RT_MAX_PATH_FRAMES)
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: NULL cameras or a frame count outside 1..%d", who, RT_MAX_PATH_FRAMES);
    int rc = check_ctx(ctx, W, H, false);
    if (rc != RT_OK) return rc;
    if (ctx->n_gpus != 1) return fail(ctx, RT_ERR_INVALID_ARG, "%s needs a single-GPU context", who);
    if (ctx->ss_log2 > 0)
        return fail(ctx, RT_ERR_UNSUPPORTED, "%s does not supersample under rt_set_supersampling (rt_set_path_supersampling is its factor)", who);
    return check_path_samples(ctx, who, W, H);
}

// check_path for the scene-track renders: the track stands where the scene does, then the frame range -- n_frames
// frames of `shutter` track frames each (rt_render_anim_shutter*; the shutter itself is check_shutter's to judge).
int check_anim(rt_ctx* ctx, const char* who, int W, int H, const rt_camera* cams, int first_frame, int n_frames,
               int shutter = 1) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    if (!cams || n_frames <= 0 || n_frames > RT_MAX_PATH_FRAMES)
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: NULL cameras or a frame count outside 1..%d", who, RT_MAX_PATH_FRAMES);
    if (!ctx->has_track) return fail(ctx, RT_ERR_NO_SCENE, "%s: rt_set_scene_track has not been called", who);
    if (W <= 0 || H <= 0 || (long long)W * H > (1LL << 31) - 1)
        return fail(ctx, RT_ERR_INVALID_ARG, "invalid frame size %dx%d", W, H);
    if (first_frame < 0 || (long long)first_frame + (long long)n_frames * shutter > ctx->track.n_frames)
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: frames %d..%lld outside the track's %d", who, first_frame,
                    (long long)first_frame + (long long)n_frames * shutter - 1, ctx->track.n_frames);
    if (ctx->n_gpus != 1) return fail(ctx, RT_ERR_INVALID_ARG, "%s needs a single-GPU context", who);
    if (ctx->ss_log2 > 0)
        return fail(ctx, RT_ERR_UNSUPPORTED, "%s does not supersample under rt_set_supersampling (rt_set_path_supersampling is its factor)", who);
    return check_path_samples(ctx, who, W, H);
}

// The shutter calls' own arguments, ahead of check_path's: *t = log2(shutter).  n_frames * shutter cameras make
// one view table, so their product keeps the bound of a path's frames.
int check_shutter(rt_ctx* ctx, const char* who, int n_frames, int shutter, int* t) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    if (shutter < 1 || shutter > RT_MAX_SHUTTER || (shutter & (shutter - 1)) != 0)
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: shutter %d is not a power of two in 1..%d", who, shutter, RT_MAX_SHUTTER);
    if (n_frames > 0 && (long long)n_frames * shutter > RT_MAX_PATH_FRAMES)
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: %d frames x shutter %d above %d cameras", who, n_frames, shutter,
                    RT_MAX_PATH_FRAMES);
    // (rt_set_path_supersampling: a channel's sum over the m sub-frames and the k^2 samples keeps the 16-bit fields)
    if (((long long)shutter << (2 * ctx->path_ss_log2)) > RT_MAX_SHUTTER)
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: shutter %d x path supersampling factor %d squared above %d samples per pixel", who,
                    shutter, 1 << ctx->path_ss_log2, RT_MAX_SHUTTER);
    // (the path threshold does not cover shutters: rt_set_shutter_adaptive_sampling is theirs, and while it is in effect the
    // path threshold is not consulted)
    if (shutter > 1 && ctx->path_ss_log2 > 0 && ctx->path_adapt_thr > 0 && ctx->shutter_adapt_thr == 0)
        return fail(ctx, RT_ERR_UNSUPPORTED, "%s: a shutter above 1 is not rendered under rt_set_path_adaptive_sampling with a path supersampling factor above 1 (rt_set_shutter_adaptive_sampling is the shutters' threshold)", who);
    *t = 0;
    while ((1 << *t) < shutter) ++*t;
    return RT_OK;
}

// rt_render_path_bands and rt_render_shutter_bands (t = log2 of the shutter) after their argument checks.
// first_frame >= 0: rt_render_anim_bands, the frames of the context's scene track from that one on, and
// rt_render_anim_shutter_bands with its shutter (t is then its log2, found here: check_anim's refusals come first).
int path_bands(rt_ctx* ctx, const char* who, int width, int height, const rt_camera* cameras, int n_frames, int t,
               int band_rows, int band_first, int band_step, void* d_out, size_t frame_stride_bytes, int format,
               void* hip_stream, int* out_n_bands, int first_frame = -1, int anim_shutter = 1) {
    const bool anim = first_frame != -1;
    RT_TRY(anim ? check_anim(ctx, who, width, height, cameras, first_frame, n_frames, anim_shutter)
                : check_path(ctx, who, width, height, cameras, n_frames));
    if (anim) RT_TRY(check_shutter(ctx, who, n_frames, anim_shutter, &t));
    RT_TRY(check_band_args(ctx, who, band_rows, band_first, band_step, d_out, format));
    RT_TRY(check_path_adaptive_bands(ctx, who, band_rows, height, t));
    const int nb = bands_of(height, band_rows, band_first, band_step);
    if (n_frames > 1 && frame_stride_bytes < band_output_bytes(width, height, nb, band_rows, format))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: frame stride smaller than a frame's output", who);
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    const int rc = anim ? trace_anim(ctx, d, (hipStream_t)hip_stream, width, height, cameras, first_frame, n_frames, t, band_rows,
                                     band_first, band_step, d_out, frame_stride_bytes, format)
                        : trace_path(ctx, d, (hipStream_t)hip_stream, width, height, cameras, n_frames, t, band_rows, band_first,
                                     band_step, d_out, frame_stride_bytes, format);
    if (out_n_bands) *out_n_bands = nb;
    if (rc == RT_OK) ctx->pixels += (uint64_t)nb * band_rows * width * (uint64_t)n_frames;
    return rc;
}
}  // namespace

int rt_render_path_bands(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int n_frames, int band_rows,
                         int band_first, int band_step, void* d_out, size_t frame_stride_bytes, int format,
                         void* hip_stream, int* out_n_bands) {
    return path_bands(ctx, "rt_render_path_bands", width, height, cameras, n_frames, 0, band_rows, band_first, band_step,
                      d_out, frame_stride_bytes, format, hip_stream, out_n_bands);
}

// shutter == 1 (t = 0) is the path call: the same launch, the PATH kernels.
int rt_render_shutter_bands(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int n_frames, int shutter,
                            int band_rows, int band_first, int band_step, void* d_out, size_t frame_stride_bytes,
                            int format, void* hip_stream, int* out_n_bands) {
    int t = 0;
    RT_TRY(check_shutter(ctx, "rt_render_shutter_bands", n_frames, shutter, &t));
    return path_bands(ctx, t ? "rt_render_shutter_bands" : "rt_render_path_bands", width, height, cameras, n_frames, t,
                      band_rows, band_first, band_step, d_out, frame_stride_bytes, format, hip_stream, out_n_bands);
}

// Chunks of at most path_chunk_frames frames: chunk c is traced into d_path[c % 2] on the worker's stream and
// copied out by the copy engine on copy_stream once its trace event has fired, under the trace of chunk c + 1;
// the trace of chunk c + 2 waits for that copy (the Tick pattern of tick_sync's chunks, over frames).
// rt_render_path and rt_render_shutter (t = log2 of the shutter: frames, chunks and buffers are output frames, and
// a chunk's launch takes its chunk << t cameras).  rt_render_anim_shutter: a chunk of nf output frames from output frame
// f0 takes its cameras from f0 << t and its track frames from first_frame + (f0 << t).
namespace {
int path_frames(rt_ctx* ctx, const char* who, int width, int height, const rt_camera* cameras, int n_frames, int t,
                int32_t* pixels, int first_frame = -1, int anim_shutter = 1) {
    const bool anim = first_frame != -1;  // rt_render_anim[_shutter]: the scene track's frames from that one on
    int rc = anim ? check_anim(ctx, who, width, height, cameras, first_frame, n_frames, anim_shutter)
                  : check_path(ctx, who, width, height, cameras, n_frames);
    if (rc != RT_OK) return rc;
    if (anim) RT_TRY(check_shutter(ctx, who, n_frames, anim_shutter, &t));
    if (!pixels) return fail(ctx, RT_ERR_INVALID_ARG, "NULL pixels");
    RT_TRY(wait_pending_async(ctx));
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    const size_t frame_bytes = (size_t)width * height * sizeof(int32_t);
    const size_t fit = std::max<size_t>(1, ((size_t)256 << 20) / frame_bytes);
    const int chunk = (int)std::min<size_t>((size_t)n_frames, ctx->path_chunk_frames > 0 ? (size_t)ctx->path_chunk_frames : fit);
    const int n_chunks = (n_frames + chunk - 1) / chunk;
    RT_TRY(ensure_stream(ctx, &d.copy_stream));
    hipEvent_t* const traced = &d.ev[Device::EV_PATH_TRACED], * const copied = &d.ev[Device::EV_PATH_COPIED];
    for (int i = 0; i < std::min(2, n_chunks); ++i) {
        RT_TRY(grow(ctx, (void**)&d.d_path[i], &d.path_cap[i], (size_t)chunk * frame_bytes));
        RT_TRY(ensure_event(ctx, &traced[i]));
        RT_TRY(ensure_event(ctx, &copied[i]));
    }
    // Every failure inside the loop leaves through the two synchronisations below: copies already queued into
    // `pixels` have landed (or failed) before this synchronous call returns, whatever it returns.
    auto hip_ok = [&](hipError_t e, const char* what) {
        if (e != hipSuccess) rc = fail(ctx, RT_ERR_HIP, "%s: %s failed: %s", who, what, hipGetErrorString(e));
        return e == hipSuccess;
    };
    for (int c = 0; c < n_chunks; ++c) {
        const int f0 = c * chunk, nf = std::min(chunk, n_frames - f0), b = c & 1;
        if (c >= 2 && !hip_ok(hipStreamWaitEvent(d.stream, copied[b], 0), "hipStreamWaitEvent")) break;
        rc = anim ? trace_anim(ctx, d, d.stream, width, height, cameras + ((size_t)f0 << t), first_frame + (f0 << t), nf, t, height,
                               0, 1, d.d_path[b], frame_bytes, RT_BANDS_INT32)
                  : trace_path(ctx, d, d.stream, width, height, cameras + ((size_t)f0 << t), nf, t, height, 0, 1, d.d_path[b],
                               frame_bytes, RT_BANDS_INT32);
        if (rc != RT_OK) break;
        // (into a range that is not registered the runtime stages this copy and the call returns only when it is
        // done: chunk c + 1 is then traced after the copy of chunk c, not under it)
        if (!hip_ok(hipEventRecord(traced[b], d.stream), "hipEventRecord") ||
            !hip_ok(hipStreamWaitEvent(d.copy_stream, traced[b], 0), "hipStreamWaitEvent") ||
            !hip_ok(hipMemcpyAsync(pixels + (size_t)f0 * width * height, d.d_path[b], (size_t)nf * frame_bytes,
                                   hipMemcpyDeviceToHost, d.copy_stream), "hipMemcpyAsync") ||
            !hip_ok(hipEventRecord(copied[b], d.copy_stream), "hipEventRecord"))
            break;
    }
    const hipError_t e_trace = hipStreamSynchronize(d.stream), e_copy = hipStreamSynchronize(d.copy_stream);
    if (rc != RT_OK) return rc;
    if (!hip_ok(e_trace, "hipStreamSynchronize") || !hip_ok(e_copy, "hipStreamSynchronize")) return rc;
    ctx->frames += (uint64_t)n_frames;
    ctx->pixels += (uint64_t)width * (uint64_t)height * (uint64_t)n_frames;
    return RT_OK;
}
}  // namespace

int rt_render_path(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int n_frames, int32_t* pixels) {
    return path_frames(ctx, "rt_render_path", width, height, cameras, n_frames, 0, pixels);
}

int rt_render_shutter(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int n_frames, int shutter,
                      int32_t* pixels) {
    int t = 0;
    RT_TRY(check_shutter(ctx, "rt_render_shutter", n_frames, shutter, &t));
    return path_frames(ctx, t ? "rt_render_shutter" : "rt_render_path", width, height, cameras, n_frames, t, pixels);
}

int rt_render_anim_bands(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int first_frame, int n_frames,
                         int band_rows, int band_first, int band_step, void* d_out, size_t frame_stride_bytes, int format,
                         void* hip_stream, int* out_n_bands) {
    if (first_frame == -1) first_frame = INT_MIN;  // (-1 marks the path calls inside path_bands: refused like any negative)
    return path_bands(ctx, "rt_render_anim_bands", width, height, cameras, n_frames, 0, band_rows, band_first, band_step,
                      d_out, frame_stride_bytes, format, hip_stream, out_n_bands, first_frame);
}

int rt_render_anim(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int first_frame, int n_frames,
                   int32_t* pixels) {
    if (first_frame == -1) first_frame = INT_MIN;
    return path_frames(ctx, "rt_render_anim", width, height, cameras, n_frames, 0, pixels, first_frame);
}

// shutter == 1 is the track call: the same launch, the ANIM kernels.
int rt_render_anim_shutter_bands(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int first_frame, int n_frames,
                                 int shutter, int band_rows, int band_first, int band_step, void* d_out,
                                 size_t frame_stride_bytes, int format, void* hip_stream, int* out_n_bands) {
    if (first_frame == -1) first_frame = INT_MIN;
    return path_bands(ctx, "rt_render_anim_shutter_bands", width, height, cameras, n_frames, 0, band_rows, band_first, band_step,
                      d_out, frame_stride_bytes, format, hip_stream, out_n_bands, first_frame, shutter);
}

int rt_render_anim_shutter(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int first_frame, int n_frames,
                           int shutter, int32_t* pixels) {
    if (first_frame == -1) first_frame = INT_MIN;
    return path_frames(ctx, "rt_render_anim_shutter", width, height, cameras, n_frames, 0, pixels, first_frame, shutter);
}

// ----------------------------------------------------------------------------
// Hit buffers and picking (include/raytracer_hip.h): the primary-only kernel (rt_kernel.hip hits_kernel) over the
// context's view, a camera path's or a scene track's.  Apart from every render's bookkeeping: no statistics, no
// timing samples, no Tick scope (a progressive run stays as it is), no view cache and so no dispatch tuner -- the view
// is built afresh by view_fill, a few microseconds of host trig per call.  The supersampling factors are not read: the
// records and the view tables are those of the plain W x VH frame.
// ----------------------------------------------------------------------------
namespace {
enum : int { HITS_CTX = 0, HITS_PATH = 1, HITS_ANIM = 2 };

// The refusals of the seven hit calls, each before any device call: a NULL context; more than one worker; then what
// check_path (HITS_PATH) or check_anim (HITS_ANIM) ask of cameras, n_frames, the scene or the track, the frame size
// and first_frame, in their order.
int check_hits(rt_ctx* ctx, const char* who, int kind, int W, int H, const rt_camera* cams, int first_frame, int n_frames) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    if (ctx->n_gpus != 1) return fail(ctx, RT_ERR_UNSUPPORTED, "%s needs a context with one worker", who);
    if (kind != HITS_CTX && (!cams || n_frames <= 0 || n_frames > RT_MAX_PATH_FRAMES))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: NULL cameras or a frame count outside 1..%d", who, RT_MAX_PATH_FRAMES);
    if (kind != HITS_ANIM) return check_ctx(ctx, W, H, false);
    if (!ctx->has_track) return fail(ctx, RT_ERR_NO_SCENE, "%s: rt_set_scene_track has not been called", who);
    if (W <= 0 || H <= 0 || (long long)W * H > (1LL << 31) - 1)
        return fail(ctx, RT_ERR_INVALID_ARG, "invalid frame size %dx%d", W, H);
    if (first_frame < 0 || (long long)first_frame + (long long)n_frames > ctx->track.n_frames)
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: frames %d..%lld outside the track's %d", who, first_frame,
                    (long long)first_frame + (long long)n_frames - 1, ctx->track.n_frames);
    return RT_OK;
}
int check_hit_buffers(rt_ctx* ctx, const char* who, const rt_hit_buffers* out) {
    if (!out || (!out->depth && !out->object && !out->position && !out->normal))
        return fail(ctx, RT_ERR_INVALID_ARG, "%s: NULL hit buffers, or no channel asked for", who);
    return RT_OK;
}

// One hit launch on `stream`: n_frames frames of W x H into `out`.  HITS_CTX: the context's camera (cams unused,
// n_frames 1).  HITS_PATH / HITS_ANIM: frame j from cams[j] -- and from track frame first_frame + j -- with the views
// built, staged and uploaded as trace_views does it, through the same ring of table slots.
int hits_launch(rt_ctx* ctx, Device& d, hipStream_t stream, int kind, int W, int H, const rt_camera* cams, int first_frame,
                int n_frames, const HitOut& out) {
    const int VH = ctx->view_height > 0 ? ctx->view_height : H;
    if (H > VH) return fail(ctx, RT_ERR_INVALID_ARG, "frame height %d above the view height %d", H, ctx->view_height);
    const SceneTrack* track = kind == HITS_ANIM ? &ctx->track : nullptr;
    LaunchParams lp;
    std::memset(&lp, 0, sizeof lp);
    Device::PathSlot* ps = nullptr;
    if (kind == HITS_CTX) {
        RT_TRY(view_fill(ctx, ctx->cam, W, VH, lp));
    } else {
        RT_TRY(path_slot_take(ctx, d, n_frames, &ps));
        for (int j = 0; j < n_frames; ++j) {
            RT_TRY(view_fill(ctx, track ? track->frames[(size_t)(first_frame + j)] : ctx->layout, cams[j], W, VH, lp));
            view_record(lp, ps->h_views[j]);
        }
    }
    lp.H = H;  // the rows traced
    if (track) {
        scene_params(ctx, d, lp, track->common, (const char*)d.d_track + (size_t)first_frame * track->stride);
        lp.scene_stride = track->stride;
    } else {
        scene_params(ctx, d, lp);
    }
    lp.counters = nullptr;  // (the kernel counts nothing)
    RT_TRY(view_tables(ctx, d, lp));
    if (ps) {
        HIP_TRY(ctx, hipMemcpyAsync(ps->d_views, ps->h_views, (size_t)n_frames * sizeof(DevView), hipMemcpyHostToDevice, stream));
        lp.views = ps->d_views;
    }
    lp.band_rows = H, lp.band_first = 0, lp.band_step = 1, lp.local_rows = H;  // one band: local row r is frame row r
    lp.n_frames = n_frames;
    const int e = launch_hits(lp, out, stream);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "hit launch: %s", hipGetErrorString((hipError_t)e));
    if (ps) {
        HIP_TRY(ctx, hipEventRecord(ps->done, stream));
        ps->busy = true;
    }
    return RT_OK;
}

int hits_device(rt_ctx* ctx, const char* who, int kind, int W, int H, const rt_camera* cams, int first_frame, int n_frames,
                const rt_hit_buffers* d_out, void* hip_stream) {
    RT_TRY(check_hits(ctx, who, kind, W, H, cams, first_frame, n_frames));
    RT_TRY(check_hit_buffers(ctx, who, d_out));
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    return hits_launch(ctx, d, (hipStream_t)hip_stream, kind, W, H, cams, first_frame, n_frames,
                       HitOut{d_out->depth, d_out->object, (float*)d_out->position, (float*)d_out->normal});
}

// The host calls: chunks of as many frames as keep the context's buffer (the requested channels, one after the
// other) at or below 256 MiB, at least one; a chunk is traced, copied out and waited for before the next.
int hits_host(rt_ctx* ctx, const char* who, int kind, int W, int H, const rt_camera* cams, int first_frame, int n_frames,
              const rt_hit_buffers* out) {
    RT_TRY(check_hits(ctx, who, kind, W, H, cams, first_frame, n_frames));
    RT_TRY(check_hit_buffers(ctx, who, out));
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    const size_t px = (size_t)W * (size_t)H;
    const size_t sz[4] = {out->depth ? sizeof(float) : 0, out->object ? sizeof(int32_t) : 0,
                          out->position ? sizeof(rt_vec3) : 0, out->normal ? sizeof(rt_vec3) : 0};
    char* const host[4] = {(char*)out->depth, (char*)out->object, (char*)out->position, (char*)out->normal};
    const size_t frame_bytes = px * (sz[0] + sz[1] + sz[2] + sz[3]);
    const int chunk = (int)std::min<size_t>((size_t)n_frames, std::max<size_t>(1, ((size_t)256 << 20) / frame_bytes));
    RT_TRY(grow(ctx, &d.d_hits, &d.hits_cap, (size_t)chunk * frame_bytes));
    char* dev[4];
    size_t off = 0;
    for (int c = 0; c < 4; ++c) {
        dev[c] = sz[c] ? (char*)d.d_hits + off : nullptr;
        off += (size_t)chunk * px * sz[c];
    }
    const HitOut o{(float*)dev[0], (int32_t*)dev[1], (float*)dev[2], (float*)dev[3]};
    int rc = RT_OK;
    for (int f0 = 0; f0 < n_frames && rc == RT_OK; f0 += chunk) {
        const int nf = std::min(chunk, n_frames - f0);
        rc = hits_launch(ctx, d, d.stream, kind, W, H, cams ? cams + f0 : nullptr, first_frame + f0, nf, o);
        for (int c = 0; c < 4 && rc == RT_OK; ++c)
            if (sz[c] && hipMemcpyAsync(host[c] + (size_t)f0 * px * sz[c], dev[c], (size_t)nf * px * sz[c], hipMemcpyDeviceToHost,
                                        d.stream) != hipSuccess)
                rc = fail(ctx, RT_ERR_HIP, "%s: hipMemcpyAsync failed", who);
        // (whatever happened, no copy into the caller's memory is pending when the call returns)
        const hipError_t e = hipStreamSynchronize(d.stream);
        if (rc == RT_OK && e != hipSuccess) rc = fail(ctx, RT_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    return rc;
}
}  // namespace

int rt_render_hits_device(rt_ctx* ctx, int width, int height, const rt_hit_buffers* d_out, void* hip_stream) {
    return hits_device(ctx, "rt_render_hits_device", HITS_CTX, width, height, nullptr, 0, 1, d_out, hip_stream);
}
int rt_render_path_hits_device(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int n_frames,
                               const rt_hit_buffers* d_out, void* hip_stream) {
    return hits_device(ctx, "rt_render_path_hits_device", HITS_PATH, width, height, cameras, 0, n_frames, d_out, hip_stream);
}
int rt_render_anim_hits_device(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int first_frame, int n_frames,
                               const rt_hit_buffers* d_out, void* hip_stream) {
    return hits_device(ctx, "rt_render_anim_hits_device", HITS_ANIM, width, height, cameras, first_frame, n_frames, d_out, hip_stream);
}
int rt_render_hits(rt_ctx* ctx, int width, int height, const rt_hit_buffers* out) {
    return hits_host(ctx, "rt_render_hits", HITS_CTX, width, height, nullptr, 0, 1, out);
}
int rt_render_path_hits(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int n_frames, const rt_hit_buffers* out) {
    return hits_host(ctx, "rt_render_path_hits", HITS_PATH, width, height, cameras, 0, n_frames, out);
}
int rt_render_anim_hits(rt_ctx* ctx, int width, int height, const rt_camera* cameras, int first_frame, int n_frames,
                        const rt_hit_buffers* out) {
    return hits_host(ctx, "rt_render_anim_hits", HITS_ANIM, width, height, cameras, first_frame, n_frames, out);
}

// One wave and one 32-byte copy: the pixel's view-plane coordinates are the view tables' entries (rt_view.h
// view_table_value), computed here, so no table is built or read.
int rt_pick(rt_ctx* ctx, int width, int height, int x, int y, rt_pick_result* out) {
    RT_TRY(check_hits(ctx, "rt_pick", HITS_CTX, width, height, nullptr, 0, 1));
    if (!out || x < 0 || x >= width || y < 0 || y >= height)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_pick: NULL result, or pixel (%d, %d) outside the %dx%d frame", x, y, width, height);
    const int VH = ctx->view_height > 0 ? ctx->view_height : height;
    if (height > VH) return fail(ctx, RT_ERR_INVALID_ARG, "frame height %d above the view height %d", height, ctx->view_height);
    static_assert(sizeof(rt_pick_result) == sizeof(DevPick), "rt_pick_result layout");
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    LaunchParams lp;
    std::memset(&lp, 0, sizeof lp);
    RT_TRY(view_fill(ctx, ctx->cam, width, VH, lp));
    scene_params(ctx, d, lp);
    lp.counters = nullptr;
    if (!d.d_pick) HIP_TRY(ctx, hipMalloc((void**)&d.d_pick, sizeof(DevPick)));
    const int e = launch_pick(lp, x, y, view_table_value(x, width, lp.pw), view_table_value(y, VH, lp.ph), d.d_pick, d.stream);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "rt_pick launch: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(ctx, hipMemcpyAsync(out, d.d_pick, sizeof(DevPick), hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

// Double-buffered Tick() on one in-order stream per worker.  Frame k's band set is traced into device
// buffer k % 2; its D2H copy rides in frame k+1's launch as the copy slice (grid z = 0, dispatched
// ahead of the trace workgroups, so the PCIe-bound copy of frame k runs under the trace of frame k+1)
// or is issued by rt_wait.  Buffer k % 2 is traced again by launch k+2, after launch k+1 (its copy) on
// the same stream.  The slice writes only host ranges registered through rt_register_host (their
// device-mapped addresses); any other buffer gets the runtime's copies on the same stream.  n > 1: every
// worker does the same with its own bands, stream and PCIe link.
// Measured (profiles/r03_tick_ab.txt): a trace stream and a copy stream ordered by events ran
// 175-195 us per frame in some processes and 350-1200 us in others -- torch's own kernel-on-one-
// stream / D2H-on-another pattern does the same -- while one stream ran a steady 195-200 us with
// the runtime's copy and 184-187 us with the copy slice.
int rt_render_async(rt_ctx* ctx, int width, int height, int32_t* pixels) {
    RT_TRY(check_ctx(ctx, width, height));
    if (!pixels) return fail(ctx, RT_ERR_INVALID_ARG, "NULL pixels");
    if (ctx->rccl_gather) return rt_render(ctx, width, height, pixels);
    TickScope tick(ctx);
    RT_TRY(tick.begin(width, height));
    const size_t frame_bytes = (size_t)width * height * sizeof(int32_t);
    const int n = ctx->n_gpus;
    // The hand-off of frame k: by the copy engine on a second stream, chunk by chunk after each chunk's trace
    // (event-ordered; the trace of frame k+2 into the same buffer waits for the copy), or as the copy slice
    // in frame k+1's launch.  Default (RT_TICK_ASYNC=stream|slice overrides): the copy engine, except for
    // shares under 0.5 M pixels at n > 1, whose short bands the pitched copies move slowly (r05l, one GPU,
    // two frames deep: C3 4,928 -> 5,167 fps, C4 1,034 -> 1,261, C5 268 -> 331; C2 at 8 workers 4,800 ->
    // 4,338 with the engine).
    const char* am = std::getenv("RT_TICK_ASYNC");
    const bool engine = am ? std::strcmp(am, "stream") == 0 : (n == 1 || (double)width * height / n >= 5e5);
    const int nc = engine ? tick_chunks(ctx, width, height) : 1;
    for (int g = 0; g < n; ++g) {
        Device& d = ctx->dev[(size_t)g];
        DeviceGuard guard(d.id);
        RT_TRY(ensure_stream(ctx, &d.async_stream));
        const int slot = d.async_next;
        const Share sh = share_of(width, height, g, n, nc > 1);
        const size_t bytes = std::max<size_t>(1, (size_t)sh.nb * sh.band_rows * width) * sizeof(int32_t);
        // (re)allocation: the pending copy may read the other buffer only, but nothing may still use this one
        if (d.frames2_cap[slot] < bytes || sh.nb <= 0) {
            RT_TRY(flush_hand(ctx));
            HIP_TRY(ctx, hipStreamSynchronize(d.async_stream));
            if (d.copy_stream) HIP_TRY(ctx, hipStreamSynchronize(d.copy_stream));
            d.copy_pending[0] = d.copy_pending[1] = false;
        }
        if (sh.nb <= 0) continue;  // (more workers than bands)
        RT_TRY(grow(ctx, (void**)&d.d_frames2[slot], &d.frames2_cap[slot], bytes));
        if (engine) {
            hipEvent_t& copied = d.ev[Device::EV_COPIED + slot];
            hipEvent_t* const ring = &d.ev[Device::EV_RING];
            RT_TRY(ensure_event(ctx, &copied));
            RT_TRY(flush_hand(ctx));  // (a slice-mode frame still pending)
            const uint64_t f = d.frames_issued++;
            const int cap = ctx->tick_inflight;
            if (cap > 0 && f >= (uint64_t)cap && ring[(f - cap) % Device::RING])  // at most cap frames queued
                HIP_TRY(ctx, hipEventSynchronize(ring[(f - cap) % Device::RING]));
            if (d.copy_pending[slot]) HIP_TRY(ctx, hipStreamWaitEvent(d.async_stream, copied, 0));
            const bool pinned = mapped_host(ctx, g, pixels, frame_bytes) != nullptr;
            RT_TRY(trace_and_copy_chunks(ctx, d, d.async_stream, sh, width, height, nc, d.d_frames2[slot], pixels, pinned));
            HIP_TRY(ctx, hipEventRecord(copied, d.copy_stream));
            if (cap > 0) {
                hipEvent_t& er = ring[f % Device::RING];
                RT_TRY(ensure_event(ctx, &er));
                HIP_TRY(ctx, hipEventRecord(er, d.copy_stream));
            }
            d.copy_pending[slot] = true;
            d.async_next = slot ^ 1;
            continue;
        }
        // (the pending hand-off as the launch's copy slice; none while it holds no words)
        RT_TRY(trace_bands(ctx, d, d.async_stream,
                           share_req(sh, width, height, 0, sh.nb, d.d_frames2[slot], &d.hand.job, tick_acc(ctx, d))));
        d.hand = {};  // issued (in the launch)
        int32_t* mapped = mapped_host(ctx, g, pixels, frame_bytes);
        if (mapped) {
            d.hand.host = sh.step == 1 ? pixels : nullptr;
            d.hand.job = share_job(sh, width, height, 0, sh.nb, d.d_frames2[slot], mapped);
        } else {
            RT_TRY(runtime_band_copy(ctx, sh, width, height, d.d_frames2[slot], pixels, d.async_stream, false, 0, sh.nb));
        }
        d.async_next = slot ^ 1;
    }
    tick.done = true;
    ctx->frames++;
    ctx->pixels += (uint64_t)width * (uint64_t)height;
    return RT_OK;
}

int rt_wait(rt_ctx* ctx) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    int rc = flush_hand(ctx);
    if (rc != RT_OK) return rc;
    for (Device& d : ctx->dev) {
        DeviceGuard guard(d.id);
        HIP_TRY(ctx, hipStreamSynchronize(d.stream));
        if (d.async_stream) HIP_TRY(ctx, hipStreamSynchronize(d.async_stream));
        if (d.copy_stream) HIP_TRY(ctx, hipStreamSynchronize(d.copy_stream));
        d.copy_pending[0] = d.copy_pending[1] = false;
    }
    return RT_OK;
}

// Debug ray view: re-trace every sample_stride-th pixel and append its segments.
int rt_debug_segments(rt_ctx* ctx, int width, int height, int sample_stride, rt_segment* out, int capacity,
                      int* out_count) {
    int rc = check_ctx(ctx, width, height, false);  // (the supersampling factor plays no part here)
    if (rc != RT_OK) return rc;
    if (sample_stride <= 0 || capacity < 0 || (capacity > 0 && !out) || !out_count)
        return fail(ctx, RT_ERR_INVALID_ARG, "rt_debug_segments: bad arguments");
    static_assert(sizeof(rt_segment) == sizeof(DevSegment), "rt_segment layout");
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    LaunchParams lp;
    std::memset(&lp, 0, sizeof lp);
    rc = view_params(ctx, width, height, lp);
    if (rc != RT_OK) return rc;
    scene_params(ctx, d, lp);
    lp.band_rows = height, lp.band_first = 0, lp.band_step = 1, lp.local_rows = height;
    DevSegment* d_out = nullptr;
    unsigned* d_count = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&d_count, sizeof(unsigned)));
    hipError_t e = hipMemsetAsync(d_count, 0, sizeof(unsigned), d.stream);  // same stream as the kernel
    if (e == hipSuccess && capacity > 0) e = hipMalloc((void**)&d_out, sizeof(DevSegment) * (size_t)capacity);
    if (e == hipSuccess) e = (hipError_t)launch_debug_segments(lp, sample_stride, d_out, capacity, d_count, d.stream);
    unsigned n = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&n, d_count, sizeof n, hipMemcpyDeviceToHost, d.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
    const unsigned keep = n < (unsigned)capacity ? n : (unsigned)capacity;
    if (e == hipSuccess && keep) e = hipMemcpy(out, d_out, sizeof(DevSegment) * keep, hipMemcpyDeviceToHost);
    (void)hipFree(d_count);
    if (d_out) (void)hipFree(d_out);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "rt_debug_segments: %s", hipGetErrorString(e));
    *out_count = (int)n;
    return RT_OK;
}

// Binary PPM (P6) of 0x00RRGGBB pixels -- the headless stand-in for the GL texture upload
// (template.cs:188-193), also used to eyeball frames from tests.
int rt_write_ppm(const char* path, const int32_t* pixels, int width, int height) {
    if (!path || !pixels || width <= 0 || height <= 0) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_write_ppm: bad args");
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_write_ppm: cannot open %s", path);
    std::fprintf(f, "P6\n%d %d\n255\n", width, height);
    std::vector<unsigned char> row((size_t)width * 3);
    bool ok = true;
    for (int y = 0; y < height && ok; ++y) {
        for (int x = 0; x < width; ++x) {
            const uint32_t v = (uint32_t)pixels[(size_t)y * width + x];
            row[(size_t)x * 3 + 0] = (unsigned char)(v >> 16);
            row[(size_t)x * 3 + 1] = (unsigned char)(v >> 8);
            row[(size_t)x * 3 + 2] = (unsigned char)v;
        }
        ok = std::fwrite(row.data(), 1, row.size(), f) == row.size();
    }
    ok = (std::fclose(f) == 0) && ok;
    return ok ? RT_OK : fail(nullptr, RT_ERR_INVALID_ARG, "rt_write_ppm: write failed for %s", path);
}

int rt_get_stats(rt_ctx* ctx, rt_stats* out) {
    if (!ctx || !out) return fail(ctx, RT_ERR_INVALID_ARG, "rt_get_stats: NULL argument");
    std::memset(out, 0, sizeof *out);
    unsigned long long c[4] = {0, 0, 0, 0};
    for (Device& d : ctx->dev) {
        DeviceGuard guard(d.id);
        HIP_TRY(ctx, hipDeviceSynchronize());
        drain_events(ctx, d);
        std::vector<unsigned long long> h(COUNTER_WORDS);
        HIP_TRY(ctx, hipMemcpy(h.data(), d.d_counters, COUNTER_WORDS * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost));
        for (int slot = 0; slot < COUNTER_SLOTS; ++slot)
            for (int i = 0; i < 4; ++i) c[i] += h[(size_t)slot * COUNTER_STRIDE + i];
    }
    out->frames = ctx->frames;
    out->pixels = ctx->pixels;
    // (adaptive launches: one primary ray per pixel counted on the host, the refined tiles' other samples by the waves)
    out->primary_rays = ctx->prim_rays + c[CNT_EXTRA_PRIMARY];
    out->reflect_rays = c[CNT_REFLECT];
    out->shadow_rays = c[CNT_SHADOW];
    const uint64_t S = (uint64_t)ctx->layout.S, P = (uint64_t)ctx->layout.P;
    out->sphere_tests = (out->primary_rays + c[1] + c[2]) * S;
    out->plane_tests = (out->primary_rays + c[1]) * P;
    out->launches = ctx->launches;
    out->kernel_ms = ctx->kernel_ms;
    out->last_kernel_ms = ctx->last_kernel_ms;
    out->copy_ms = ctx->copy_ms;
    out->gather_ms = ctx->gather_ms;
    out->timed_launches = ctx->timed[0];
    out->timed_copies = ctx->timed[1];
    out->timed_gathers = ctx->timed[2];
    return RT_OK;
}

int rt_dispatch_order(rt_ctx* ctx, int* out_order) {
    if (!ctx || !out_order) return fail(ctx, RT_ERR_INVALID_ARG, "NULL argument");
    // (a new scene or frame size is measured again from its first single-frame launch)
    if (ctx->dev.empty()) return fail(ctx, RT_ERR_INVALID_ARG, "context without a device");
    const Device::OrderTuner& t = ctx->dev[0].order;
    // (the tuner measures single-frame launches of view_w x view_rows traced rows, whatever the view height)
    const bool fresh = t.scene_gen == ctx->scene_gen && ctx->view_ok && t.W == ctx->view_w && t.H == ctx->view_rows;
    *out_order = ctx->order_fixed >= 0 ? ctx->order_fixed : fresh ? ctx->dev[0].order.chosen : -1;
    return RT_OK;
}

int rt_set_timing(rt_ctx* ctx, int every) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    if (every < 0) return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_timing: every must be >= 0");
    ctx->timing_every = every;
    for (Device& d : ctx->dev) d.op_count[0] = d.op_count[1] = d.op_count[2] = 0;
    return RT_OK;
}

int rt_set_counting(rt_ctx* ctx, int on) {
    if (!ctx || (on != 0 && on != 1)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_set_counting: bad arguments");
    ctx->counting = on != 0;
    return RT_OK;
}

int rt_reset_stats(rt_ctx* ctx) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "NULL context");
    for (Device& d : ctx->dev) {
        DeviceGuard guard(d.id);
        HIP_TRY(ctx, hipDeviceSynchronize());
        drain_events(ctx, d);
        HIP_TRY(ctx, hipMemset(d.d_counters, 0, COUNTER_WORDS * sizeof(unsigned long long)));
        HIP_TRY(ctx, hipDeviceSynchronize());  // the clear lands before the next frame's atomics
    }
    ctx->frames = ctx->pixels = ctx->launches = ctx->prim_rays = 0;
    ctx->kernel_ms = ctx->last_kernel_ms = ctx->copy_ms = ctx->gather_ms = 0;
    ctx->timed[0] = ctx->timed[1] = ctx->timed[2] = 0;
    for (Device& d : ctx->dev) d.op_count[0] = d.op_count[1] = d.op_count[2] = 0;
    return RT_OK;
}

int rt_count_work(rt_ctx* ctx, int width, int height, rt_work* out) {
    int rc = check_ctx(ctx, width, height, false);
    if (rc != RT_OK) return rc;
    if (ctx->ss_log2 > 0)
        return fail(ctx, RT_ERR_UNSUPPORTED, "rt_count_work does not supersample (rt_set_supersampling(ctx, 1) first)");
    if (!out) return fail(ctx, RT_ERR_INVALID_ARG, "rt_count_work: NULL out_work");
    if (ctx->n_gpus != 1) return fail(ctx, RT_ERR_INVALID_ARG, "rt_count_work needs a single-GPU context");
    Device& d = ctx->dev[0];
    DeviceGuard guard(d.id);
    LaunchParams lp;
    std::memset(&lp, 0, sizeof lp);
    rc = view_params(ctx, width, height, lp);
    if (rc != RT_OK) return rc;
    scene_params(ctx, d, lp);
    rc = view_tables(ctx, d, lp);
    if (rc != RT_OK) return rc;
    rc = grow(ctx, (void**)&d.d_frame, &d.frame_cap, (size_t)width * height * sizeof(int32_t));
    if (rc != RT_OK) return rc;
    if (!d.d_counters_diag)
        HIP_TRY(ctx, hipMalloc((void**)&d.d_counters_diag, COUNTER_WORDS * sizeof(unsigned long long)));
    HIP_TRY(ctx, hipMemsetAsync(d.d_counters_diag, 0, COUNTER_WORDS * sizeof(unsigned long long), d.stream));
    lp.counters = d.d_counters_diag;
    lp.band_rows = height, lp.band_first = 0, lp.band_step = 1, lp.local_rows = height;
    lp.out = d.d_frame;
    lp.out_fmt = RT_BANDS_INT32;
    lp.n_frames = 1;
    if (const char* sel = getenv("RT_DIAG_SEL")) lp.enc_frame0 = atoi(sel);  // RT_SHADOW_CAT diagnostic builds only
    int e = launch_trace(lp, ctx->layout.generic_pow, true, d.stream);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "rt_count_work launch: %s", hipGetErrorString((hipError_t)e));
    std::vector<unsigned long long> h(COUNTER_WORDS);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), d.d_counters_diag, COUNTER_WORDS * sizeof(unsigned long long),
                                hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(ctx, hipStreamSynchronize(d.stream));
    unsigned long long c[COUNTER_STRIDE] = {};
    for (int slot = 0; slot < COUNTER_SLOTS; ++slot)
        for (int i = 0; i < COUNTER_STRIDE; ++i) c[i] += h[(size_t)slot * COUNTER_STRIDE + i];
    const uint64_t S = (uint64_t)ctx->layout.S, P = (uint64_t)ctx->layout.P;
    std::memset(out, 0, sizeof *out);
    out->primary_rays = (uint64_t)width * (uint64_t)height;
    out->reflect_rays = c[CNT_REFLECT];
    out->shadow_rays = c[CNT_SHADOW];
    out->sphere_tests = (out->primary_rays + out->reflect_rays + out->shadow_rays) * S;
    out->plane_tests = (out->primary_rays + out->reflect_rays) * P;
    out->shadow_rays_run = c[CNT_SHADOW_RUN];
    out->sphere_tests_run = c[CNT_SPHERE_RUN];
    out->plane_tests_run = c[CNT_PLANE_RUN];
    return RT_OK;
}

}  // extern "C"
