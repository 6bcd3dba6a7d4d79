// rt_internal.h -- device-side scene layout and launch interface shared by the HIP
// kernels (rt_kernel.hip) and the C-ABI host code (rt_api.cpp).
//
// Scene layout in HBM (one contiguous, 16-byte aligned allocation per context/device,
// read through the scalar cache: every loop over primitives is wave-uniform):
//   DevSphere  [S]   {center.xyz, radius^2}                 16 B   intersection loops
//   DevMaterial[S+P] sphere materials then plane materials  64 B   shading (per-lane gather)
//   DevPlane   [P]   {center, c.n, normal, e1, e2}          64 B
//   DevLight   [L]   {position, intensity, |p|^2 terms, shadow threshold, cull frame}  64 B
// Everything that the reference recomputes per call but that depends only on scene
// constants (radius^2 :336, dot(center,normal) :594, checkerboard basis e1/e2 :760-765,
// ambient*Ka :778/:873, dot(light,light) for the shadow ray :617) is computed once on the
// host with the same binary32 operations, which yields bit-identical values.
#pragma once
#include <stdint.h>

#include "rt_resolve.h"

namespace rtk {

struct DevSphere {
    float cx, cy, cz, r2;
};

// MAT_DARK_OK (plane materials): the host part of the dark-tile skip's guard holds (rt_dark.h plane_dark_ok)
enum : uint32_t { MAT_MIRROR = 1u, MAT_DIFFUSE = 2u, MAT_SPEC = 4u, MAT_DARK_OK = 8u };

enum : uint32_t { POW_GENERIC = 0u, POW_ONE = 1u, POW_HALF = 2u, POW_TWO = 3u };

struct DevMaterial {
    float kd[3];
    float amb[3];   // ambient * Ka  (RayTracer.cs:778, :873)
    float ks[3];
    float n;
    float km[3];
    uint32_t flags;  // MAT_* (RayTracer.cs:85-93)
    uint32_t pow_kind;  // POW_* fast paths for Math.Pow(x, n) (exact; see rt_kernel.hip)
    uint32_t pad;
};

struct DevPlane {
    float cx, cy, cz, cn;  // center, dot(center, normal)
    float nx, ny, nz, pad0;
    float e1x, e1y, e1z, pad1;
    float e2x, e2y, e2z, pad2;
};

struct DevLight {
    float px, py, pz, intensity;
    float a;      // dot(p, p)       : IntersectsSphere's `a` for a shadow ray (dir = position)
    float a2;     // 2 * a
    float a4;     // 4 * a
    // Shadow threshold (2a finite and > 0): IntersectsSphere(.., 0.001f) collides iff
    // fl(-b - sqrt) >= sh_t, i.e. fl(fl(-b - sqrt) / 2a) - 0.001f > 0 without the division
    // (rt_api.cpp shadow_threshold).
    float sh_t;
    // shadow-cull frame (culling only, never in a result): A ~ p/|p| (every shadow ray of this
    // light has direction p), U, V ~ orthonormal to A
    float ax, ay, az, pad1;
    float ux, uy, uz, pad2;
    float vx, vy, vz, pad3;
};

// Per-sphere culling record: centre and a radius bound r' >= sqrt(r^2) * (1 + 2^-8).
struct DevSphereCull {
    float cx, cy, cz, rr;
};

// Sphere clusters of the bundle kernel's per-lane pre-cull (CULL_MIN_SPHERES <= S <= 64; culling only): a
// bounding sphere (centre, radius R >= |c_i - centre| + r'_i of every member, r' as in DevSphereCull) and
// the member set as a mask over sphere indices.  A trace bundle whose cone allows no culling (the reflected
// segments deep in mirror chains, where a wave's rays fan out) tests each lane's own ray against the
// clusters and takes the union of the kept clusters' members (rt_kernel.hip cluster_mask) instead of every
// sphere.  Built on the host by median splits of the centres (rt_api.cpp build_clusters).
struct DevCluster {
    float cx, cy, cz, R;
    unsigned long long members;
    unsigned long long pad;
};
// Spheres per cluster: 4, 8 and 12 measured alike (C4 303.4-304.3 us, C5 1,114.7-1,116.3 us per frame against
// 311.2-311.8 / 1,135-1,137 without clusters), 2 and 16 slower (profiles/ab/r06_clusters.txt); 8 tests the fewest
// bounds.  (tools/trace_cull_model.py ranked 2 and 4 first: it prices a cluster test too cheaply.)
constexpr int CLUSTER_SIZE = 8;
constexpr int MAX_CLUSTERS = 32;

// Per-(light, sphere) shadow-cull record (culling only): the sphere centre in the light's frame
// (C.U, C.V, C.A, rounded from double) and r' + 2^-18 |C| (the projection-error allowance,
// rt_kernel.hip shadow_sphere_cull).  [L][S], built when L * S <= SHADOW_CULL_MAX_ENTRIES (larger
// scenes trace their shadow rays without culling).
struct DevShadowCull {
    float cu, cv, ca, rr;
};
constexpr long long SHADOW_CULL_MAX_ENTRIES = 1LL << 16;
// The direct kernel's per-lane shadow pre-test (S < CULL_MIN_SPHERES; culling only): per (light, sphere) the
// centre's (u, v) in the light's frame and, with the sphere's share of the margin folded in, the axial bound
// ca' and the radius bound rr' (rt_api.cpp, rt_kernel.hip shadow_pre_keep).  Same record type, [L][S + (S & 1)].
//
// Per-light bounding hierarchy over those records (rt_scene.h build_shadow_groups; culling only): the spheres of a
// light are split into at most SHADOW_GROUPS groups by closeness in the light's (u, v), each with a record of the
// same shape -- a disc that contains its members' discs, the largest of their ca' -- and the members as a mask over
// sphere indices (S < CULL_MIN_SPHERES <= 16); `uni` contains every group the same way.  A plane-uniform wave tests
// the union before the pair loop (rt_kernel.hip shadow_scan, rt_shadow_pre.h); the group level is built and checked
// (tests/native/shadow_group_host.cpp) and not read by the kernel (profiles/ab/r15_shadow_groups.txt).  A group
// without members has mask 0 and a record no finite lane keeps.  [L], behind the pre-test records.
constexpr int SHADOW_GROUPS = 3;
struct DevShadowGroups {
    DevShadowCull uni;
    DevShadowCull grp[SHADOW_GROUPS];
    uint32_t mask[SHADOW_GROUPS];
    uint32_t pad;
};
static_assert(sizeof(DevShadowGroups) % 16 == 0, "DevShadowGroups records are 16-byte aligned in the scene image");

// Per-light shadow grid (bundle kernel's merged shadow pass, S <= 64 spheres, L <= 4 lights;
// culling only).  Every shadow ray of light l has direction p_l, so whether sphere j can block a
// hit point hp depends on hp's coordinates (u, v) across the light's axis and a along it.  The host
// tabulates, per light, a SHGRID_N x SHGRID_N grid over (u, v) of 64-bit masks -- the spheres whose
// margin-grown disc reaches the cell -- and SHGRID_SLABS + 2 axial masks -- the spheres whose
// centre may lie ahead of a slab -- valid for lanes with |hp|_1 <= `bound`; each lane looks up its
// own cell and slab (rt_kernel.hip shadow_members_grid).  Lanes beyond the bound use the bounding
// box of every disc with their own margin and the slab masks shifted by it.  Margins and the
// exactness argument: rt_api.cpp build_shadow_grid.
// The merged shadow pass (and so the grid) serves scenes with at most 64 spheres and this many lights.
constexpr int SHADOW_MERGE_L = 4;
constexpr int SHGRID_N = 64;
constexpr int SHGRID_SLABS = 32;
struct DevShadowGrid {
    float su, ou, sv, ov;  // cell coordinates: floor(fma(u, su, ou)), floor(fma(v, sv, ov))
    float sa, oa;          // slab coordinate: floor(fma(a, sa, oa)), clamped to [-1, SHGRID_SLABS]
    float bound;           // lanes with |hp|_1 <= bound use the grid
    float far_k;           // lanes beyond it: own margin far_k * |hp|_1 (2^-8 + projection error) ...
    float far_b;           // ... and slab coordinate a - (far_k * |hp|_1 - far_b), far_b = 2^-8 bound
    float bu0, bu1, bv0, bv1;  // (u, v) box of every sphere's disc grown by 2^-8 |C|_1 (no |hp| term)
    float pad;
    unsigned long long always;  // spheres never culled (no valid cull record: NaN/huge/tiny)
};
// Device layout: DevShadowGrid[L], then masks [L][SHGRID_N * SHGRID_N] (row iv, column iu), then
// slab masks [L][SHGRID_SLABS + 2] (entry ia + 1, ia = -1 .. SHGRID_SLABS).

// Work counters: each workgroup adds its totals into slot (block id % COUNTER_SLOTS) so that
// the atomics of thousands of workgroups do not serialise on one address.  Per slot:
// reflected segments and shadow rays of the visible path (every launch), and the executed
// work of the diagnostic kernels (rt_count_work): shadow rays whose sphere loop ran, exact
// sphere and plane tests run.
constexpr int COUNTER_SLOTS = 256;
constexpr int COUNTER_STRIDE = 8;
constexpr int COUNTER_WORDS = COUNTER_SLOTS * COUNTER_STRIDE;
enum : int { CNT_REFLECT = 1, CNT_SHADOW = 2, CNT_SHADOW_RUN = 3, CNT_SPHERE_RUN = 4, CNT_PLANE_RUN = 5 };
// Adaptive supersampling (rt_set_adaptive_sampling): the samples its waves traced beyond one per rendered pixel,
// k^2 - 1 per valid pixel of every refined tile -- the part of primary_rays the host cannot know (rt_get_stats).
enum : int { CNT_EXTRA_PRIMARY = 0 };

// Camera-relative sphere constants of the primary segment (origin = camera position for
// every pixel): oc = cam - center and c = Dot(oc, oc) - r^2 of IntersectsSphere
// (RayTracer.cs:614-619), computed once per frame on the host with the same binary32
// operations and passed in the kernarg block for up to MAX_PRIM_CONST spheres.
// Per-frame conservative screen box of sphere i for primary rays: pixels outside
// [x0, x1] x [y0, y1] cannot select sphere i (view_params in rt_api.cpp derives it).
struct PrimBox {
    int x0, x1, y0, y1;
};

struct PrimConst {
    float ocx, ocy, ocz, c;
};
constexpr int MAX_PRIM_CONST = 64;
// Per-view footprint of a plane for primary rays (rt_foot.h derives it and states the rule).
struct PlaneFoot {
    float a, b, c;
};
constexpr int FOOT_MAX = 4;
constexpr int ROW_ORDER_MAX = 272;  // tile rows of a 2176-row frame (4K UHD: 270)

// Scenes with at least this many spheres use wave-bundle culling (rt_kernel.hip; the bundle
// kernel on the 8-sphere configs measured +20 %, profiles/ab/r02_direct_converged_fold_rejected.txt).
constexpr int CULL_MIN_SPHERES = 12;


// A band set's copy into a frame (the Tick hand-off, rt_api.cpp share_of): `words` int32 of a packed
// band set at src -> dst, band after band: source word i of band k = i / band_words lands at dst word
// k * dst_stride + i % band_words (band_words = 0: one contiguous run).  The host guarantees 16-byte
// aligned ends and band_words, dst_stride multiples of 4 (whole 16-byte stores never straddle a band).
struct CopyJob {
    const int32_t* src;
    int32_t* dst;
    unsigned long long words;
    unsigned long long dst_stride;
    unsigned band_words;
    unsigned pad;
};

// The view of one frame of a camera-path launch (rt_render_path_bands: LaunchParams::views, one record per
// grid z in device memory): every LaunchParams field that depends on the camera, with the same values the
// by-value block of a one-camera launch carries (rt_api.cpp view_fill builds both).  pw / ph / nearc and
// the lxt / lyt tables depend only on the frame size and are shared by the frames.
struct alignas(16) DevView {
    float cam[3], right[3], up[3], fwd[3];
    int prim_const;
    int mbox_n;
    int mbox_plane[2];
    float mbox_tmax[2];
    int pad[2];
    PrimConst pc[MAX_PRIM_CONST];
    PrimBox pbox[MAX_PRIM_CONST];
    PrimBox mbox[2][CULL_MIN_SPHERES];
};
static_assert(sizeof(DevView) % 16 == 0, "DevView records are 16-byte aligned in their device table");

// Per-launch parameters (passed by value as the kernel argument block, < 4 KiB).
struct LaunchParams {
    const DevSphere* sph;
    const DevMaterial* mat;  // [S + P]
    const DevPlane* pl;
    const DevLight* li;
    const DevSphereCull* scull;  // [S]
    const DevShadowCull* shcull;  // [L][S] or NULL (no shadow culling)
    const DevShadowCull* shpre;   // [L][S + (S & 1)] the direct kernel's shadow pre-test, or NULL
    const DevShadowGrid* shg;     // [L] or NULL (no shadow grid: the per-level bound instead)
    const unsigned long long* shgrid;  // [L][SHGRID_N^2]
    const unsigned long long* shslab;  // [L][SHGRID_SLABS + 2]
    const DevCluster* clus;            // [n_clus] (n_clus 0: no per-lane pre-cull)
    const float* lxt;  // [W]: ((float)x / W - 0.5f) * pw, TracePixel :963-965
    const float* lyt;  // [H]: ((float)y / H - 0.5f) * ph
    int S, P, L, limit;
    int lights_a2_ok;  // every light's 2a = 2 p.p is finite and > 0 (the shadow loops' exact-threshold form)
    int n_clus;
    // view, RayTracer.cs:511-523 and :892-896 (computed on the host)
    float cam[3], right[3], up[3], fwd[3];
    float pw, ph, nearc;
    int W, H;
    // row mapping: local row r -> band (band_first + (r / band_rows) * band_step),
    // global row = band * band_rows + r % band_rows; pixel written at out[r * W + x].
    int band_rows, band_first, band_step, local_rows;
    int n_frames;  // grid z (frames of one batch launch, all with this view); 0 = 1
    int32_t* out;
    unsigned long long out_frame_bytes;  // batch launches: frame z of the grid at (char*)out + z * out_frame_bytes
    int out_fmt;  // 0: int32 0x00RRGGBB per pixel; 1: packed 24-bit (bytes B, G, R); 2: int32 at frame row y;
                  // 3 (OUT_TILES): the tile codec's encoder fused into the trace -- nothing at `out`,
                  // tile t's header into enc_wire and its segments into enc_stage[t * STAGE_WORDS],
                  // t = (enc_frame0 + frame) * enc_tpf + tile row * enc_tiles_x + tile column
    unsigned char* enc_wire;
    uint32_t* enc_stage;
    int enc_tiles_x, enc_tpf, enc_frame0;
    // Adaptive shutter launches (rt_set_shutter_adaptive_sampling, the SHUTTER_ADAPT / ANIM_SHUTTER_ADAPT instantiations):
    // the threshold T in 1..256 of a launch with `views`, view_ss = 1, ss_log2 > 0 and shutter_log2 > 0, 0 = none.  With
    // it set a lane is an output pixel and the grid is in output tiles, as in a PATH_ADAPT launch; the wave traces sample
    // (0, 0) of its tile in each of the m sub-frames' views (and scenes), decides on the rounded mean of those m pixels,
    // and traces the other m (k^2 - 1) samples only when the tile is refined (rt_kernel.hip shutter_adaptive_tile).
    // view_adapt stays refused with a shutter; adapt_thr stays ignored by a launch with `views`.  In the padding between
    // enc_frame0 and counters: no field moves and the block keeps its size.
    int shutter_adapt;
    unsigned long long* counters;  // COUNTER_SLOTS x COUNTER_STRIDE (CNT_*)
    // The Tick hand-off fused into a trace launch (rt_render_async: the previous frame; a chunked
    // rt_render: the previous chunk): with copy_z = 1 the launch has one more grid z-slice, z = 0,
    // whose workgroups run `copy` (device band set -> the caller's registered host buffer through its
    // device-mapped address); the launch's one frame is z = 1 (out_frame_bytes 0).  copy_z = 0: none.
    CopyJob copy;
    int copy_z;
    int prim_const;                // 1: pc[0..S) and pbox[0..S) valid (S <= MAX_PRIM_CONST)
    PrimConst pc[MAX_PRIM_CONST];
    PrimBox pbox[MAX_PRIM_CONST];
    // single-frame launches of a whole frame (the direct kernel's multi-tile workgroups): dispatch
    // position -> tile row in the order the host picked (rt_api.cpp order_pick: rows by estimated
    // cost, or bottom to top; row_order_n = the launch's tile rows, 0: natural order).  A lone
    // frame's last waves set its tail.
    int row_order_n;
    int col_major;  // single-frame launches: tile rows vary fastest in dispatch order (grid x = rows)
    uint16_t row_order[ROW_ORDER_MAX];
    // single-frame launches, measured order (order_pick candidate 3): dispatch position (workgroup x
    // SINGLE_WPG + wave, a 1-D grid) -> tile (ty << 16 | tx; ty = 0xffff pads past the last tile), and
    // tile_cost: when set, each wave stores its duration (RTC ticks) at tile ty * tiles_x + tx
    const uint32_t* tile_order;
    uint32_t* tile_cost;
    // supersampling (rt_set_supersampling): log2 of the factor k, 0 = off.  With it set W, H, band_rows and
    // local_rows above are in samples (the k W x k H frame: view tables, screen boxes and culls as for any
    // frame of that size), and the output -- one pixel per k x k block, row stride W >> ss_log2 -- is
    // written by the SS instantiations' epilogue (rt_kernel.hip resolve_tile).  Last: no other field moves.
    int ss_log2;
    // Mirrored screen boxes (the direct kernel, S < CULL_MIN_SPHERES, limit >= 1; culling only): for the first
    // MIRROR_BOX_PLANES mirror planes whose table could be built (mbox_n of them, plane index mbox_plane[k]),
    // mbox[k][i] is the screen box outside which a ray reflected by that plane at a primary hit with
    // t <= mbox_tmax[k] cannot select sphere i (rt_api.cpp mirror_boxes; in the view's pixels like pbox).
    int mbox_n;
    int mbox_plane[2];
    float mbox_tmax[2];
    PrimBox mbox[2][CULL_MIN_SPHERES];
    // Camera-path launches (rt_render_path_bands): frame z of the grid takes its view from views[z] instead of
    // cam .. fwd, prim_const, pc, pbox and mbox* above (the PATH instantiations, rt_kernel.hip); nullptr: every
    // frame has the view above.  After every earlier field: none of them moves.
    const DevView* views;
    // The shutter of a camera-path launch (rt_render_shutter_bands, the SHUTTER instantiations): log2 of the
    // cameras m averaged per output frame, 0 = an ordinary path launch.  With it set `views` holds n_frames << t
    // records, sub-frame s of grid z at views[z << t | s], and a wave traces its tile once per sub-frame and stores
    // the round-half-up mean (rt_resolve.h resolve_round_n).  Last: no other field moves.
    int shutter_log2;
    // Adaptive supersampling (rt_set_adaptive_sampling, the ADAPT instantiations): the threshold T in 1..256 of a
    // launch with ss_log2 > 0, 0 = every block is supersampled (the SS instantiations).  With it set a lane is an
    // output pixel, the wave traces sample (0, 0) of its 8x8 output tile, and the other k^2 - 1 samples only when
    // two 4-adjacent pixels of the tile differ by >= T in a channel (rt_kernel.hip adaptive_tile); the grid is in
    // output tiles.  Last: no other field moves.
    int adapt_thr;
    // Plane footprints of the view (rt_foot.h; the direct kernel's one-view instantiations; culling only): foot_n
    // >= 0: the scene has foot_n = P planes and foot[i] is plane i's record -- a pixel with view-table values
    // (lx, ly) cannot select plane i with its primary ray when fma(a, lx, fma(b, ly, c)) < 0.  -1: none (the view
    // or a plane outside the rule's domain, more than FOOT_MAX planes, no primary constants, RT_PRIM_FOOT=0).
    // Last: no other field moves.
    int foot_n;
    PlaneFoot foot[FOOT_MAX];
    // Progressive accumulation (rt_set_progressive, the PROG instantiations): prog_acc != nullptr marks the launch.
    // As in an ADAPT launch ss_log2 > 0, W, H and the rows are in samples, a lane is an output pixel and the grid is
    // in output tiles.  The wave traces prog_n (0, 1 or 2) samples of every pixel of its tile -- samples prog_first
    // and prog_first + 1 of the run, whose positions in the k x k block arrive as pass codes j k + i (sample_pixel)
    // in prog_pass -- adds them to the pixel's sums at prog_acc[r * (W >> ss_log2) + x] (r: the launch's local output
    // row, x: the output column; the packed band set's addressing whatever out_fmt), which it reads only when
    // prog_first > 0 and writes only when prog_n > 0, and stores the rounded mean of the prog_first + prog_n samples
    // (rt_resolve.h resolve_round_div) in the launch's format (rt_kernel.hip progressive_tile).  Last: no other field
    // moves.
    ResolveSum* prog_acc;
    int prog_first;
    int prog_n;
    int prog_pass[2];
    // Plane-uniform waves (the direct kernel, rt_kernel.hip trace_tile_direct; where operands come from, never what
    // is computed): 1: a wave whose level-0 records all lie on one plane shades them converged, with that plane's
    // material and geometry read through a wave-uniform index; 0: no wave is classified (a zeroed block, and
    // RT_UNIFORM_PLANE=0 through rt_set_scene).  Last: no other field moves.
    int uniform_plane;
    // Scene-track shutters (rt_render_anim_shutter_bands, the ANIM_SHUTTER / ANIM_SHUTTER_SS instantiations): 1 marks a
    // launch with `views`, a scene_stride and shutter_log2 > 0 -- a shutter launch whose sub-frame s of grid z, record
    // rec = z << shutter_log2 | s, takes its view from views[rec] and reads each of the 12 scene tables at its pointer +
    // rec * scene_stride: the image pointers are those of the launch's first sub-frame and the track's images lie
    // scene_stride apart, one per sub-frame (rt_kernel.hip SceneOf).  0: a scene_stride with a shutter stays a
    // combination no kernel is built for (a zeroed block).  In the padding between uniform_plane and
    // shgrp: no field moves and the block keeps its size.
    int scene_shutter;
    // The shadow pre-test's group and union records (DevShadowGroups [L]; the direct kernel's plane-uniform waves;
    // culling only), or nullptr: the flat loop over every pair (no pre-test records, RT_SHADOW_GROUPS=0 through
    // rt_set_scene, a zeroed block).  Last: no other field moves.
    const DevShadowGroups* shgrp;
    // Scene tracks (rt_render_anim_bands, the ANIM instantiations): the bytes between the scene images of consecutive
    // grid-z frames -- frame z reads each of the 12 scene tables above (sph .. clus, shgrp) at its pointer + z *
    // scene_stride; a null pointer stays null (rt_kernel.hip SceneOf).  The scalars derived from the scene (S, P, L,
    // limit, n_clus, lights_a2_ok, uniform_plane) are the same for every frame (rt_scene.h track_build).  0: every frame
    // has the scene at the pointers (a zeroed block).  Last: no other field moves.
    unsigned long long scene_stride;
    // Supersampled path, shutter and track launches (rt_set_path_supersampling, the PATH_SS / SHUTTER_SS / ANIM_SS
    // instantiations): 1 marks a launch with `views` and ss_log2 > 0 -- W, H, band_rows and local_rows are in samples
    // as in any supersampling launch, the DevView records are built for the k W x k H sample frame, a lane is a sample
    // and the epilogue writes one pixel per k x k block (rt_kernel.hip resolve_tile; with a shutter the block sum of
    // the lanes' sub-frame sums, shutter_tile).  0: `views` with ss_log2 > 0 stays a combination no kernel is built for
    // (a zeroed block).  Last: no other field moves.
    int view_ss;
    // Adaptive path and track launches (rt_set_path_adaptive_sampling, the PATH_ADAPT / ANIM_ADAPT instantiations): the
    // threshold T in 1..256 of a launch with `views`, view_ss = 1, ss_log2 > 0 and no shutter, 0 = none.  With it set the
    // launch is ADAPT's per frame: a lane is an output pixel, the grid is in output tiles, the wave traces sample (0, 0) of
    // its tile in frame z's view (and scene) and the other k^2 - 1 samples only when the tile is refined (rt_kernel.hip
    // adaptive_tile).  adapt_thr stays ignored by a launch with `views`.  In the tail padding behind view_ss: no field
    // moves and the block keeps its size.
    int view_adapt;
};
constexpr int MIRROR_BOX_PLANES = 2;
// Tiles per workgroup of the direct kernel's single-frame launches (8: +2.5 % on C2,
// profiles/r04_final_check.txt); the measured tile order (LaunchParams::tile_order) is padded to it.
constexpr int SINGLE_WPG = 4;
// The kernel argument block: raising ROW_ORDER_MAX or MAX_PRIM_CONST must not push it past 4 KiB.
static_assert(sizeof(LaunchParams) < 4096, "LaunchParams is passed by value as the kernarg block (< 4 KiB)");

constexpr int OUT_TILES = 3;

// ---------------------------------------------------------------------------------
// Trace kernel variants.  A trace launch runs one instantiation of one of four entry points
// (rt_kernel.hip trace_{direct,bundle}_kernel[_gpow]<K, V>); which one is decided here, on the host, from the
// launch parameters alone, and described by a TraceVariant.  Its fields but K travel to the kernels as one
// word V of named options (variant_word), which every level of the kernel code reads by name.
// ---------------------------------------------------------------------------------
// Scenes with at most DIRECT_SMAX spheres (every BASELINE config of the direct kernel) run a
// direct kernel whose sphere-pair loops are unrolled.
constexpr int DIRECT_SMAX = 8;

enum : int { TV_DIRECT = 0, TV_BUNDLE = 1 };
// PLAIN: pixels to `out`.  STATS: as PLAIN, and the diagnostic tallies of the executed work.  TILES: out_fmt
// OUT_TILES, the fused tile encoder.  SS: the supersampling epilogue.  PATH: one DevView per grid z.  SHUTTER: a
// PATH launch whose waves average 1 << shutter_log2 DevViews per grid z.  ADAPT: supersampling decided per output
// tile (LaunchParams::adapt_thr).  PROG: one Tick of a progressive run, 0-2 samples per output pixel added to an
// accumulator that outlives the launch (LaunchParams::prog_acc).  ANIM: a PATH launch whose grid z also has its own
// scene image (LaunchParams::scene_stride).  PATH_SS, SHUTTER_SS, ANIM_SS: the twins of PATH, SHUTTER and ANIM whose
// lanes are samples of the k W x k H frame, with SS's tile mapping and epilogue (LaunchParams::view_ss).  PATH_ADAPT,
// ANIM_ADAPT: PATH_SS and ANIM_SS launches that decide per output tile as ADAPT does (LaunchParams::view_adapt).
// ANIM_SHUTTER, ANIM_SHUTTER_SS: SHUTTER and SHUTTER_SS launches whose sub-frames also have their own scene image
// (LaunchParams::scene_shutter).  SHUTTER_ADAPT, ANIM_SHUTTER_ADAPT: SHUTTER_SS and ANIM_SHUTTER_SS launches that decide
// per output tile, on the mean of the sub-frames' samples (0, 0), as ADAPT does (LaunchParams::shutter_adapt).
enum : int { TM_PLAIN = 0, TM_STATS = 1, TM_TILES = 2, TM_SS = 3, TM_PATH = 4, TM_SHUTTER = 5, TM_ADAPT = 6, TM_PROG = 7, TM_ANIM = 8,
             TM_PATH_SS = 9, TM_SHUTTER_SS = 10, TM_ANIM_SS = 11, TM_PATH_ADAPT = 12, TM_ANIM_ADAPT = 13, TM_ANIM_SHUTTER = 14,
             TM_ANIM_SHUTTER_SS = 15, TM_SHUTTER_ADAPT = 16, TM_ANIM_SHUTTER_ADAPT = 17 };
struct TraceVariant {
    int family;  // TV_*
    int gpow;    // some material needs the f64 Math.Pow path: the entry points without the register caps
    int mode;    // TM_*
    int cls;     // direct: SMAX, the compile-time sphere bound (DIRECT_SMAX or 0 = none); bundle: MERGED 0, 1 or 2
    int K;       // stack records: limit + 1 rounded up to 1, 2, 4, 6, 8, or 64 (the scratch stack)
    int wpg;     // tiles (waves) per workgroup: 1, or SINGLE_WPG for a lone frame on the direct kernel
    int tord;    // 0: tiles in grid order (row_order / col_major), 1: tile_order, 2: as 0 and tile_cost recorded
};

enum : unsigned { VF_GPOW = 1u, VF_STATS = 2u, VF_TILES = 4u, VF_SS = 8u, VF_PATH = 16u, VF_SHUTTER = 32u, VF_ADAPT = 64u, VF_PROG = 128u };
// (bits 0-7 are taken and the 4-bit fields follow: ANIM sits above vf_tord's two bits)
constexpr unsigned VF_ANIM = 1u << 18;
// (the supersampled twins of PATH, SHUTTER and ANIM: flags of their own, so that no earlier word changes)
constexpr unsigned VF_PATH_SS = 1u << 19, VF_SHUTTER_SS = 1u << 20, VF_ANIM_SS = 1u << 21;
constexpr unsigned VF_VIEW_SS = VF_PATH_SS | VF_SHUTTER_SS | VF_ANIM_SS;
// (the adaptive twins of PATH_SS and ANIM_SS, likewise)
constexpr unsigned VF_PATH_ADAPT = 1u << 22, VF_ANIM_ADAPT = 1u << 23;
constexpr unsigned VF_VIEW_ADAPT = VF_PATH_ADAPT | VF_ANIM_ADAPT;
// (the scene-track twins of SHUTTER and SHUTTER_SS, likewise)
constexpr unsigned VF_ANIM_SHUTTER = 1u << 24, VF_ANIM_SHUTTER_SS = 1u << 25;
// (the adaptive twins of SHUTTER_SS and ANIM_SHUTTER_SS, likewise)
constexpr unsigned VF_SHUTTER_ADAPT = 1u << 26, VF_ANIM_SHUTTER_ADAPT = 1u << 27;
constexpr unsigned VF_VIEW_SHUTTER_ADAPT = VF_SHUTTER_ADAPT | VF_ANIM_SHUTTER_ADAPT;
constexpr unsigned vf_cls(int c) { return (unsigned)c << 8; }
constexpr unsigned vf_wpg(int w) { return (unsigned)w << 12; }
constexpr unsigned vf_tord(int t) { return (unsigned)t << 16; }
constexpr int vf_cls_of(unsigned v) { return (int)(v >> 8 & 15u); }  // SMAX (direct) / MERGED (bundle)
constexpr int vf_wpg_of(unsigned v) { return (int)(v >> 12 & 15u); }
constexpr int vf_tord_of(unsigned v) { return (int)(v >> 16 & 3u); }
static_assert(DIRECT_SMAX < 16 && SINGLE_WPG < 16, "the variant word's 4-bit fields");
constexpr unsigned variant_word(const TraceVariant& v) {
    return (v.gpow ? VF_GPOW : 0u) | (v.mode == TM_STATS ? VF_STATS : 0u) | (v.mode == TM_TILES ? VF_TILES : 0u) |
           (v.mode == TM_SS ? VF_SS : 0u) | (v.mode == TM_PATH ? VF_PATH : 0u) |
           (v.mode == TM_SHUTTER ? VF_SHUTTER : 0u) | (v.mode == TM_ADAPT ? VF_ADAPT : 0u) | (v.mode == TM_PROG ? VF_PROG : 0u) |
           (v.mode == TM_ANIM ? VF_ANIM : 0u) | (v.mode == TM_PATH_SS ? VF_PATH_SS : 0u) |
           (v.mode == TM_SHUTTER_SS ? VF_SHUTTER_SS : 0u) | (v.mode == TM_ANIM_SS ? VF_ANIM_SS : 0u) |
           (v.mode == TM_PATH_ADAPT ? VF_PATH_ADAPT : 0u) | (v.mode == TM_ANIM_ADAPT ? VF_ANIM_ADAPT : 0u) |
           (v.mode == TM_ANIM_SHUTTER ? VF_ANIM_SHUTTER : 0u) | (v.mode == TM_ANIM_SHUTTER_SS ? VF_ANIM_SHUTTER_SS : 0u) |
           (v.mode == TM_SHUTTER_ADAPT ? VF_SHUTTER_ADAPT : 0u) | (v.mode == TM_ANIM_SHUTTER_ADAPT ? VF_ANIM_SHUTTER_ADAPT : 0u) | vf_cls(v.cls) | vf_wpg(v.wpg) | vf_tord(v.tord);
}

// The bundle family's shadow pass by scene: 0 = per light (also every scene of the direct family), 1 = the
// merged pass for S <= 64 spheres and 1..SHADOW_MERGE_L lights (the scenes with shadow grids), 2 = the merged
// pass with every light's 2a finite and > 0 (the exact-threshold form).
inline int merged_class(int S, int L, bool lights_a2_ok) {
    if (S < CULL_MIN_SPHERES || !(S <= 64 && L >= 1 && L <= SHADOW_MERGE_L)) return 0;
    return lights_a2_ok ? 2 : 1;
}

// The band rule of an adaptive launch (rt_set_adaptive_sampling with k > 1): its 8x8 tiles are tiles of the frame's
// 8-row grid when the bands are multiples of 8 output rows, or when one band covers the frame.
inline bool adaptive_band_ok(int band_rows, int H) { return band_rows % 8 == 0 || band_rows >= H; }

// The instantiations that exist (1164): every mode, depth and class of both families at one tile per workgroup
// in grid order (SHUTTER, ANIM, PATH_SS, SHUTTER_SS, ANIM_SS, PATH_ADAPT, ANIM_ADAPT, ANIM_SHUTTER, ANIM_SHUTTER_SS,
// SHUTTER_ADAPT and ANIM_SHUTTER_ADAPT among them, under PATH's conditions,
// and ADAPT and PROG, under SS's: 60 of their own each); the
// direct kernel's lone-frame workgroups of SINGLE_WPG tiles in each tile order (PLAIN only); the all-lights-ok
// merged bundle kernel's tile orders (PLAIN, no GPOW).
constexpr bool trace_variant_built(const TraceVariant& v) {
    const bool plain = v.mode == TM_PLAIN;
    if (v.family == TV_DIRECT)
        return (v.cls == 0 || v.cls == DIRECT_SMAX) && (v.wpg == 1 ? v.tord == 0 : v.wpg == SINGLE_WPG && plain);
    return v.cls >= 0 && v.cls <= 2 && v.wpg == 1 && (v.tord == 0 || (plain && !v.gpow && v.cls == 2));
}

// The variant a launch of p runs; false: a combination no kernel is built for (launch_trace answers
// hipErrorInvalidValue; rt_api.cpp refuses these before any launch).  No device call.
inline bool pick_trace_variant(const LaunchParams& p, bool generic_pow, bool stats, TraceVariant* v) {
    const bool tiles = p.out_fmt == OUT_TILES, ordered = p.tile_order != nullptr || p.tile_cost != nullptr;
    if (p.shutter_log2 != 0 && (p.views == nullptr || p.shutter_log2 < 0 || p.shutter_log2 > 8)) return false;
    // (a scene track: a path launch without a shutter, whose images lie whole 256-byte steps apart)
    // (scene_shutter = 1: a track under a shutter, one image per sub-frame -- and nothing else carries the mark)
    if (p.scene_shutter != 0 && (p.scene_shutter != 1 || p.scene_stride == 0 || p.shutter_log2 <= 0 || p.view_adapt != 0)) return false;
    if (p.scene_stride != 0 && (p.views == nullptr || (p.shutter_log2 != 0 && p.scene_shutter == 0) || p.scene_stride % 256 != 0))
        return false;
    // (a progressive launch is a supersampling launch of one view, never adaptive)
    if (p.prog_acc != nullptr && (p.views != nullptr || p.ss_log2 <= 0 || p.ss_log2 > 3 || p.adapt_thr != 0 || p.prog_first < 0 ||
                                  p.prog_n < 0 || p.prog_n > 2 || p.prog_first + p.prog_n < 1 ||
                                  p.prog_first + p.prog_n > 1 << (2 * p.ss_log2)))
        return false;
    // (a supersampled path, shutter or track launch: views, a factor, and sums that fit ResolveSum's 16-bit fields)
    if (p.view_ss != 0 && (p.view_ss != 1 || p.views == nullptr || p.ss_log2 <= 0 || p.ss_log2 > 3 ||
                           p.shutter_log2 + 2 * p.ss_log2 > 8))
        return false;
    // (an adaptive path or track launch: a supersampled one without a shutter, and a threshold)
    if (p.view_adapt != 0 && (p.view_adapt < 1 || p.view_adapt > 256 || p.views == nullptr || p.view_ss != 1 || p.ss_log2 <= 0 ||
                              p.ss_log2 > 3 || p.shutter_log2 != 0))
        return false;
    // (an adaptive shutter launch: a supersampled shutter launch -- view_ss bounds shutter_log2 + 2 ss_log2 -- and a
    // threshold; the path threshold stays out of it)
    if (p.shutter_adapt != 0 && (p.shutter_adapt < 1 || p.shutter_adapt > 256 || p.views == nullptr || p.view_ss != 1 || p.ss_log2 <= 0 ||
                                 p.ss_log2 > 3 || p.shutter_log2 < 1 || p.shutter_log2 + 2 * p.ss_log2 > 8 || p.view_adapt != 0))
        return false;
    if (p.views != nullptr) {
        if ((p.ss_log2 > 0 && p.view_ss == 0) || tiles || stats || ordered || p.copy_z != 0 || p.row_order_n != 0 || p.col_major != 0)
            return false;
        v->mode = p.shutter_adapt != 0 ? (p.scene_shutter != 0 ? TM_ANIM_SHUTTER_ADAPT : TM_SHUTTER_ADAPT)
                  : p.view_adapt != 0 ? (p.scene_stride != 0 ? TM_ANIM_ADAPT : TM_PATH_ADAPT)
                  : p.scene_shutter != 0 ? (p.view_ss != 0 ? TM_ANIM_SHUTTER_SS : TM_ANIM_SHUTTER)
                  : p.view_ss != 0 ? (p.shutter_log2 > 0 ? TM_SHUTTER_SS : p.scene_stride != 0 ? TM_ANIM_SS : TM_PATH_SS)
                                 : p.shutter_log2 > 0 ? TM_SHUTTER : p.scene_stride != 0 ? TM_ANIM : TM_PATH;
    } else if (p.ss_log2 > 0) {
        if (p.ss_log2 > 3 || tiles || stats || ordered || p.adapt_thr < 0 || p.adapt_thr > 256) return false;
        v->mode = p.prog_acc != nullptr ? TM_PROG : p.adapt_thr > 0 ? TM_ADAPT : TM_SS;
    } else {
        v->mode = tiles ? TM_TILES : stats ? TM_STATS : TM_PLAIN;  // (the fused encoder never tallies)
    }
    v->gpow = generic_pow;
    // Instantiation per recursion depth: K = limit + 1 records (levels 0..limit each push at most
    // one), rounded up to the LDS stack sizes; deeper limits use the scratch stack.
    const int need = p.limit + 1;
    v->K = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 6 ? 6 : need <= 8 ? 8 : 64;
    const int tord = v->mode != TM_PLAIN ? 0 : p.tile_cost != nullptr ? 2 : p.tile_order != nullptr ? 1 : 0;
    // bundle culling pays for its per-wave bounds only with enough spheres (A/B: +15 % at
    // 8 spheres, 3x faster at 64)
    if (p.S >= CULL_MIN_SPHERES) {
        v->family = TV_BUNDLE;
        v->cls = merged_class(p.S, p.L, p.lights_a2_ok != 0);
        v->wpg = 1;
        // the all-lights-ok merged instantiation's single-frame tile orders (no GPOW); the others keep grid order
        v->tord = v->cls == 2 && !generic_pow ? tord : 0;
    } else {
        v->family = TV_DIRECT;
        v->cls = p.S <= DIRECT_SMAX ? DIRECT_SMAX : 0;
        // a lone frame: SINGLE_WPG tiles of a tile row per workgroup, in the order the host picked
        const bool lone = SINGLE_WPG > 1 && v->mode == TM_PLAIN && p.n_frames <= 1 && p.copy_z == 0;
        v->wpg = lone ? SINGLE_WPG : 1;
        v->tord = lone ? tord : 0;
    }
    return true;
}

// Debug-view segment (layout of rt_segment in include/raytracer_hip.h).
struct DevSegment {
    float ox, oy, oz, ex, ey, ez;
    int kind, pixel;
};

// Hit buffers (rt_render_hits*, include/raytracer_hip.h rt_hit_buffers): the four channels of a hit launch in device
// memory, frame z of the grid at element z * W * H of each; a null channel is not written.  position and normal as
// three floats per pixel (rt_vec3).  A picked pixel's record (rt_pick): the layout of rt_pick_result.
struct HitOut {
    float* depth;
    int32_t* object;
    float* position;
    float* normal;
};
struct DevPick {
    int32_t object;
    float depth;
    float position[3];
    float normal[3];
};

// Launchers (rt_kernel.hip).  Return hipError_t as int.
// The primary-only hit kernel over p's frame (one band: band_rows = local_rows = H), n_frames = grid z: the view of
// the block (p.views null), of views[z] (a camera path), or of views[z] with the scene image z * scene_stride on (a
// scene track).  Nothing of p beyond the view, the scene tables and the frame geometry is read.
int launch_hits(const LaunchParams& p, const HitOut& out, void* stream);
// Pixel (x, y) of p's own view with the view-plane coordinates (lx, ly) of that column and row, one wave -> *out.
int launch_pick(const LaunchParams& p, int x, int y, float lx, float ly, DevPick* out, void* stream);
int launch_debug_segments(const LaunchParams& p, int stride, DevSegment* out, int capacity, unsigned* count,
                          void* stream);
// generic_pow: some material needs the f64 Math.Pow path (exponent not 0.5, 1 or 2).
// stats: the diagnostic kernels that also tally the executed work (CNT_*_RUN).
int launch_trace(const LaunchParams& p, bool generic_pow, bool stats, void* stream);
// All ranks' gathered band sets (rank r's at g + r * slot_bytes, format fmt) -> frame.
int launch_scatter_gathered(const unsigned char* g, size_t slot_bytes, int fmt, int32_t* frame, int W, int H,
                            int band_rows, int world, void* stream);
int launch_scatter_bands(const int32_t* bands, int32_t* frame, int W, int H, int band_rows, int band_first,
                         int band_step, int n_bands, void* stream);
// A CopyJob on its own (the Tick hand-off when no later trace launch carries it: the last chunk of a
// synchronous rt_render, rt_wait's flush of rt_render_async's last frame).
int launch_band_copy(const CopyJob& job, void* stream);

// Band-set tile codec (rt_codec.hip; format: raytracer_hip/tilecodec.py).
struct CodecGeom {
    int W, H, band_rows, rank, world, n_bands;  // rank / n_bands: the encoder's rank; the decoder's first rank
    int tiles_x, tiles_y, tiles_per_frame, n_tiles, n_chunks;
    size_t frame_stride;  // elements between frames (input band sets / output frames)
    size_t fixed_bytes;   // wire: header + tile headers + chunk bases, 8-aligned
};
// n_frames band sets (frame_stride apart) of g.rank -> wire; *wire_bytes (device, may be
// NULL) receives the wire's byte size.  Two launches; `stage` = encode_stage_bytes(g) of
// device scratch that no other launch uses meanwhile.
int launch_encode_bands(const int32_t* bands, unsigned char* wire, const CodecGeom& g, int64_t* wire_bytes,
                        void* stage, void* stream);
size_t encode_stage_bytes(const CodecGeom& g);
// The second half of the encoder after traces with OUT_TILES filled the tile headers (tile rows
// >= traced_tile_rows of every frame were not traced: their headers are zeroed) and the staging
// slots: chunk totals from the headers, then the compaction of launch_encode_bands.  Two launches.
int launch_finish_wire(unsigned char* wire, const CodecGeom& g, int traced_tile_rows, int64_t* wire_bytes,
                       void* stage, void* stream);
// every rank's wire (rank r's at gathered + r * rank_stride) -> frames.  One launch.
int launch_decode_gathered(const unsigned char* gathered, size_t rank_stride, int32_t* frames, const CodecGeom& g,
                           void* stream);

}  // namespace rtk
