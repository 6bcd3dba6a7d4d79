// rt_kernel.hip -- gfx950 kernels for the per-pixel Whitted trace of
// Raytracer/RayTracer.cs (TracePixel :962-1002 -> TraceSphere/TracePlane :729-876 ->
// IntersectsSphere/IntersectPlane :590-642 -> IntersectShadowLight :573-582 ->
// *PhongShading :652-708 -> TraceSecondaryRay :789-826 -> ShiftColor :1046-1052).
//
// Design (MI355X-first, not a translation of the C# recursion):
//  * one wave64 lane per pixel; a wave covers an 8x8 pixel tile (ray coherence -> fewer
//    divergent primitive hits per wave) and is its own workgroup (A/B: 2x2-wave groups
//    +8 % on C4, where a group's LDS stack slots were held until its slowest wave ended);
//  * the scene is tiny (< 6 KB at 64 spheres) and every loop over spheres / planes / lights
//    is wave-uniform, so primitive data is read with scalar loads (SGPR operands); the
//    camera-relative sphere constants of the primary segment come in the kernarg block;
//  * the reference shades EVERY hit primitive and recurses from each mirror hit; only the
//    nearest (by the reference's own selection rules) reaches the pixel, so each lane walks
//    a single chain of segments forward (intersection only), pushing one record per
//    shaded hit onto a per-lane stack, then folds colours backward in the reference's
//    exact order: mirror term, then each light in order, then ambient
//    (RayTracer.cs:739-778, :850-873).  Bit-identical to the all-hit recursion.
//  * arithmetic is IEEE binary32 with no FMA contraction (-ffp-contract=off), correctly
//    rounded '/' and sqrt, IEEE-754-2019 maximum/minimum for .NET Math.Max/Min, f64 where
//    the reference uses Math.Pow, and .NET's (int) conversion (NaN/overflow -> INT_MIN).
//  * work the reference does but whose result provably cannot change a selection is
//    skipped (sqrt/divisions of spheres behind the ray, the far root) -- see root_t1.
#include <hip/hip_runtime.h>

#include "rt_fastmath.h"
#include "rt_codec_common.h"
#include "rt_dark.h"
#include "rt_foot.h"
#include "rt_internal.h"
#include "rt_pow.h"
#include "rt_prims.h"
#include "rt_resolve.h"
#include "rt_shadow_pre.h"

// One wave (64 lanes, an 8x8 pixel tile) per workgroup: a one-wave group releases its LDS
// stack slots as soon as it ends.  The dispatcher launches one-wave groups no faster than
// ~6.9 us per 1080p frame (tools/launch_probe.hip, a store-only kernel), but with real work
// that is not the limit: 4-wave groups and waves looping over 2/4/8 tiles all measured equal
// or slower (C2 +0..16 %, C3 +3..22 %, C4 +16..37 %; profiles/ab/r02_tiles_per_wg_rejected.txt).
constexpr int WG_THREADS = 64, TILE_W = 8, TILE_H = 8;

// Parts.  The 1164 trace instantiations take a quarter of an hour to compile as one translation unit, on one core.  The
// Makefile therefore compiles this file RT_KERNEL_PARTS = 4 times, each time with another RT_KERNEL_PART, in parallel:
// a part instantiates the trace kernels of its modes only (trace_mode_part) and defines launch_trace_part<its number>;
// part 0 also holds the kernels that are no templates and every launcher, launch_trace among them, which hands a
// descriptor to its part.  Every kernel is compiled from the same source with the same flags as in one unit; the parts'
// objects are joined into obj/rt_kernel.o.  Without the macros (make resources, asm, variant; tools) the file is one
// unit with everything in it.
#ifndef RT_KERNEL_PARTS
#define RT_KERNEL_PARTS 1
#define RT_KERNEL_PART 0
#endif
static_assert((RT_KERNEL_PARTS == 1 || RT_KERNEL_PARTS == 4) && RT_KERNEL_PART >= 0 && RT_KERNEL_PART < RT_KERNEL_PARTS,
              "one unit, or parts 0..3");

namespace rtk {

// PLAIN, STATS, ANIM_SHUTTER_ADAPT | TILES, SS, PATH, SHUTTER, SHUTTER_ADAPT | ADAPT, PROG, ANIM, PATH_SS, ANIM_SHUTTER |
// SHUTTER_SS, ANIM_SS, PATH_ADAPT, ANIM_ADAPT, ANIM_SHUTTER_SS: 264 + 300 + 300 + 300 instantiations.  (Modes come in sixties, so
// no split of the 1164 has a smaller largest part.  Part 0 is the code object that rt_create loads, with the kernels of
// every Tick and batch render.)
constexpr int trace_mode_part(int mode) {
    return RT_KERNEL_PARTS == 1 ? 0 : mode == TM_ANIM_SHUTTER_ADAPT ? 0 : mode == TM_SHUTTER_ADAPT ? 1 : mode == TM_ANIM_SHUTTER ? 2 : mode == TM_ANIM_SHUTTER_SS ? 3 : mode < TM_TILES ? 0 : mode < TM_ADAPT ? 1 : mode < TM_SHUTTER_SS ? 2 : 3;
}
static_assert(TM_STATS == 1 && TM_SHUTTER == 5 && TM_PATH_SS == 9 && TM_ANIM_ADAPT == 13 && TM_ANIM_SHUTTER == 14 && TM_ANIM_SHUTTER_SS == 15 &&
                  TM_SHUTTER_ADAPT == 16 && TM_ANIM_SHUTTER_ADAPT == 17,
              "the modes of each part");

// Frame / band output: int32 0x00RRGGBB at the packed band row r (format 0) or at the frame
// row y (format 2), or packed 24-bit (B, G, R bytes; the top byte of the int32 is always 0)
// for band sets shipped to rank 0 -- a quarter fewer bytes over xGMI (format 1).
// Format 2 (RT_BANDS_FRAME): the rank's bands straight into the row-major frame (row y).
// The Tick hand-off (CopyJob): a band set, device -> the caller's registered host buffer through its
// device-mapped address, 16 bytes per lane (both ends 16-byte aligned, checked on the host), band k
// of the packed source at k * dst_stride in the frame (one band set per device of a multi-GPU Tick,
// each device's bands cross its own PCIe link).  As a trace launch's copy slice (z = 0)
// it is dispatched before the trace workgroups, so the PCIe-bound copy of frame (or chunk) k-1 runs
// under the trace of k on one in-order stream.  Only the first COPY_WAVES workgroups copy
// (grid-strided, 4 loads in flight per lane), the others exit at once: a wave holds its slot until its
// host stores are acknowledged, and a slice of one-store waves (8,100 at 1080p) held nearly every wave
// slot of the chip until PCIe had drained them, so the trace waited.
constexpr unsigned COPY_WAVES = 512;
__device__ __forceinline__ size_t band_dst(const CopyJob& j, unsigned i) {  // source word -> frame word
    if (j.band_words == 0) return i;
    const unsigned k = i / j.band_words;  // (words < 2^31: W * H is capped on the host)
    return (size_t)k * j.dst_stride + (i - k * j.band_words);
}
__device__ __forceinline__ void copy_job(const CopyJob& j, size_t wg, size_t nwg) {
    const size_t lane = threadIdx.x & 63;
    const unsigned long long n = j.words, n4 = n / 4;
    const int4* __restrict__ s4 = (const int4*)j.src;
    const size_t step = nwg * 64;
    size_t i = wg * 64 + lane;
    if (j.band_words == 0) {
        int4* __restrict__ d4 = (int4*)j.dst;
        for (; i + 3 * step < n4; i += 4 * step) {
            const int4 a = s4[i], b = s4[i + step], c = s4[i + 2 * step], d = s4[i + 3 * step];
            d4[i] = a;
            d4[i + step] = b;
            d4[i + 2 * step] = c;
            d4[i + 3 * step] = d;
        }
        for (; i < n4; i += step) d4[i] = s4[i];
    } else {  // band_words and dst_stride are multiples of 4: a 16-byte chunk never straddles a band
        // (one chunk per lane and iteration, 32-bit chunk indices: this path shares the trace kernels'
        // register allocation, which must not grow -- 512 waves keep ~0.5 MB in flight, plenty for PCIe)
        int4* __restrict__ d4 = (int4*)j.dst;
        const unsigned bq = j.band_words / 4, sq = (unsigned)(j.dst_stride / 4);
        for (unsigned c = (unsigned)i; c < (unsigned)n4; c += (unsigned)step) {
            const unsigned k = c / bq;
            d4[k * sq + (c - k * bq)] = s4[c];
        }
    }
    if (wg == 0 && lane < n - n4 * 4) j.dst[band_dst(j, (unsigned)(n4 * 4 + lane))] = j.src[n4 * 4 + lane];
}
__device__ __forceinline__ void copy_slice(const LaunchParams& p) {
    const size_t nwg = min((size_t)gridDim.x * gridDim.y, (size_t)COPY_WAVES);
    const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (wg < nwg) copy_job(p.copy, wg, nwg);
}
#if RT_KERNEL_PART == 0
__global__ __launch_bounds__(64) void band_copy_kernel(CopyJob j) { copy_job(j, blockIdx.x, gridDim.x); }
#endif

// Pixel i (row-major in the launch's output: packed bands, or the frame for out_fmt 2) of frame z.
__device__ __forceinline__ void store_at(const LaunchParams& p, size_t i, uint32_t px32) {
    // batch frame z (a launch with the copy slice has one frame and out_frame_bytes 0)
    unsigned char* base = (unsigned char*)p.out + (size_t)blockIdx.z * p.out_frame_bytes;
    if (p.out_fmt != 1) {
        ((int32_t*)base)[i] = (int32_t)px32;
    } else {
        unsigned char* o = base + i * 3;
        o[0] = (unsigned char)px32;
        o[1] = (unsigned char)(px32 >> 8);
        o[2] = (unsigned char)(px32 >> 16);
    }
}
__device__ __forceinline__ void store_pixel(const LaunchParams& p, int r, int y, int x, uint32_t px32) {
    store_at(p, (size_t)(p.out_fmt == 2 ? y : r) * (size_t)p.W + (size_t)x, px32);
}

// Supersampling (LaunchParams::ss_log2 = s > 0, the SS instantiations): the wave's 8x8 tile holds
// samples (lane = ry * 8 + rx), and each k x k block of them, k = 1 << s, becomes one output pixel --
// the round-half-up mean per channel (rt_resolve.h) -- stored by the block's leader lane (rx, ry
// multiples of k) at column x >> s of packed row r >> s (frame row y >> s for out_fmt 2) of an output
// W >> s pixels wide.  No sample reaches memory.  Converged call; what lanes outside the frame pass never
// enters a stored pixel: W, H and the band rows are multiples of k and tiles start at multiples of 8, so
// a block is inside the launch's rows or outside them as a whole.
// The block sum is a butterfly over lane bits 0 and 3 (k >= 2), 1 and 4 (k >= 4), 2 and 5 (k = 8); k is
// wave-uniform.  In-row steps by DPP (they fold into v_add_u32_dpp), the others through the LDS
// crossbar: the tile's values stay in VGPRs (readlanes would raise the SGPR peak, see encode_tile_fused).
template <int CTRL>
__device__ __forceinline__ ResolveSum resolve_add_dpp(ResolveSum v) {
    return resolve_add(v, ResolveSum{(uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.rb, CTRL, 0xf, 0xf, false),
                                     (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.g, CTRL, 0xf, 0xf, false)});
}
template <int PATTERN>  // ds_swizzle, bit-mask mode: lane ^ xor_mask inside each group of 32 lanes
__device__ __forceinline__ ResolveSum resolve_add_swizzle(ResolveSum v) {
    return resolve_add(v, ResolveSum{(uint32_t)__builtin_amdgcn_ds_swizzle((int)v.rb, PATTERN),
                                     (uint32_t)__builtin_amdgcn_ds_swizzle((int)v.g, PATTERN)});
}
// The butterfly: every lane's v -> the sum over its k x k block, k = 1 << s (in every lane of the block).
__device__ __forceinline__ ResolveSum resolve_block_sum(ResolveSum v, int s) {
    v = resolve_add_dpp<0xb1>(v);   // quad_perm:[1,0,3,2]  lane ^ 1
    v = resolve_add_dpp<0x128>(v);  // row_ror:8            lane ^ 8
    if (s >= 2) {
        v = resolve_add_dpp<0x4e>(v);         // quad_perm:[2,3,0,1]  lane ^ 2
        v = resolve_add_swizzle<0x401f>(v);   // lane ^ 16
    }
    if (s >= 3) {
        v = resolve_add_swizzle<0x101f>(v);   // lane ^ 4
        v = resolve_add(v, ResolveSum{(uint32_t)__shfl_xor((int)v.rb, 32, 64), (uint32_t)__shfl_xor((int)v.g, 32, 64)});
    }
    return v;
}
__device__ __forceinline__ void resolve_tile(const LaunchParams& p, int r, int y, int x, bool valid, uint32_t px32) {
    const int s = p.ss_log2;
    const ResolveSum v = resolve_block_sum(resolve_unpack(px32), s);
    const int km = (1 << s) - 1;
    if (valid && ((x | r) & km) == 0)  // (r and y agree modulo k: bands are multiples of k rows)
        store_at(p, (size_t)((p.out_fmt == 2 ? y : r) >> s) * (size_t)(p.W >> s) + (size_t)(x >> s), resolve_round(v, s));
}
// SHUTTER_SS (a shutter launch whose lanes are samples): `sum` is the lane's sample summed over the 1 << t sub-frames;
// the block's leader stores the one round-half-up mean of all (1 << t) k^2 values, resolve_round_n over t + 2 s bits
// (the host bounds (1 << t) k^2 by RT_MAX_SHUTTER: rt_resolve.h's 16-bit fields hold the sum and its rounding term).
// Integer adds commute, so neither the order of the sub-frames nor that of the lanes can change a bit.
__device__ __forceinline__ void resolve_tile_sums(const LaunchParams& p, int r, int y, int x, bool valid, ResolveSum sum, int t) {
    const int s = p.ss_log2;
    const ResolveSum v = resolve_block_sum(sum, s);
    const int km = (1 << s) - 1;
    if (valid && ((x | r) & km) == 0)
        store_at(p, (size_t)((p.out_fmt == 2 ? y : r) >> s) * (size_t)(p.W >> s) + (size_t)(x >> s), resolve_round_n(v, t + 2 * s));
}

// OUT_TILES: the tile codec's encoder (rt_codec.hip encode_group, format raytracer_hip/tilecodec.py)
// fused into the trace -- the wave's 8x8 tile (lane = ry * 8 + rx) goes straight from registers to
// its tile header and staged segments, and the band set never reaches HBM.  Converged call.
// Residuals: dx = p - left (column 0: p - the tile's first pixel), minus the row above's dx (lane
// - 8); widths from the wave OR; a row's w bytes of a segment are the OR of its 8 lanes' fields.
__device__ __forceinline__ void encode_tile_fused(const LaunchParams& p, uint32_t px, bool valid) {
    const int lane = threadIdx.x & 63, rx = lane & 7, ry = lane >> 3;
    // (cross-lane steps by DPP / bpermute, so that the tile's values stay in VGPRs: readlanes
    // here would raise the direct kernel's SGPR peak above 80 and cost it a wave per SIMD)
    const uint32_t v = valid ? px & 0xffffffu : 0u;
    const uint32_t first = (uint32_t)__shfl((int)v, 0, 64);
    const size_t t = (size_t)(p.enc_frame0 + (int)blockIdx.z) * (size_t)p.enc_tpf +
                     (size_t)blockIdx.y * (size_t)p.enc_tiles_x + blockIdx.x;
    if (__builtin_amdgcn_ballot_w64(valid && v != first) == 0) {  // one colour (sky): no residual
        if (lane == 0) wire_tile_hdr(p.enc_wire)[t] = first;
        return;
    }
    const uint32_t left = row_shr<1>(v);  // lane - 1: the same row for rx >= 1
    const uint32_t dx = sub_bytes(v, rx ? left : first);
    const uint32_t above = (uint32_t)__shfl_up((int)dx, 8, 64);  // lane - 8: the row above
    const uint32_t z = valid ? zigzag_bytes(ry ? sub_bytes(dx, above) : dx) & 0xffffffu : 0u;
    uint32_t o = group8_or(z);  // the tile's OR, in every lane
    o |= (uint32_t)__shfl_xor((int)o, 8, 64);
    o |= (uint32_t)__shfl_xor((int)o, 16, 64);
    o |= (uint32_t)__shfl_xor((int)o, 32, 64);
    const uint32_t iR = width_index((o >> 16) & 0xffu), iG = width_index((o >> 8) & 0xffu),
                   iB = width_index(o & 0xffu);
    const uint32_t wm = width_at(iR) | (width_at(iG) << 4) | (width_at(iB) << 8);
    if (lane == 0) wire_tile_hdr(p.enc_wire)[t] = first | ((iR + 6u * iG + 36u * iB) << 24);
    if (wm) {  // (the same in every lane)
        unsigned char* seg = (unsigned char*)(p.enc_stage + t * STAGE_WORDS);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t w = (wm >> (4 * c)) & 15u;
            if (w) {
                const uint64_t f = (uint64_t)((z >> (16 - 8 * c)) & 0xffu) << (rx * w);
                const uint32_t lo = group8_or((uint32_t)f), hi = group8_or((uint32_t)(f >> 32));
                if (rx == 0) store_row_bits(seg + ry * w, w, ((uint64_t)hi << 32) | lo);
            }
            seg += 8 * w;
        }
    }
}

// The view of the wave's frame.  PATH (camera-path launches, rt_render_path_bands): frame z of the grid has its
// own camera, and everything that depends on it -- position and basis, the primary constants, the screen boxes
// -- is read from the frame's DevView record in device memory instead of the kernarg block.  blockIdx.z is
// wave-uniform, so the reads stay scalar loads (the kernarg block itself is read with scalar loads too: the
// same instructions from another base address).  The values are those a one-camera launch would carry.
// SHUTTER (rt_render_shutter_bands): grid z is an output frame that averages 1 << shutter_log2 sub-frames, and the
// wave traces them one after the other; the sub-frame's record index `rec` = z << shutter_log2 | s travels with the
// ViewOf as a member, from the kernel body's loop counter through every function that builds one.  It is made of
// blockIdx.z, a kernarg and a wave-uniform loop counter only, so it lives in an SGPR and the reads stay scalar
// loads.  The other views never read `rec` (it is a dead constant 0 there: their code is what it was).
// ANIM (scene tracks, rt_render_anim_bands): PATH's view -- every ViewOf member reads the frame's record exactly as
// VIEW_PATH does -- in a launch whose frames also have their own scene image (SceneOf below).
// ANIM_SHUTTER (scene-track shutters, rt_render_anim_shutter_bands): SHUTTER's view -- every ViewOf member reads record
// `rec` exactly as VIEW_SHUTTER does -- in a launch whose sub-frames also have their own scene image (SceneOf below).
constexpr int VIEW_ARGS = 0, VIEW_PATH = 1, VIEW_SHUTTER = 2, VIEW_ANIM = 3, VIEW_ANIM_SHUTTER = 4;
// PATH_SS, SHUTTER_SS, ANIM_SS (rt_set_path_supersampling): the view kind of the twin -- the records are built for the
// sample frame on the host -- and, independently of it, SS's tile mapping and epilogue (ss_of).
constexpr int view_of(unsigned V) {
    return (V & (VF_ANIM_SHUTTER | VF_ANIM_SHUTTER_SS | VF_ANIM_SHUTTER_ADAPT)) ? VIEW_ANIM_SHUTTER
           : (V & (VF_SHUTTER | VF_SHUTTER_SS | VF_SHUTTER_ADAPT)) ? VIEW_SHUTTER
           : (V & (VF_ANIM | VF_ANIM_SS | VF_ANIM_ADAPT)) ? VIEW_ANIM
           : (V & (VF_PATH | VF_PATH_SS | VF_PATH_ADAPT)) ? VIEW_PATH
                                              : VIEW_ARGS;
}
constexpr bool ss_of(unsigned V) { return (V & (VF_SS | VF_VIEW_SS | VF_ANIM_SHUTTER_SS)) != 0; }            // a lane is a sample of a k x k block
constexpr bool shutter_of(unsigned V) { return (V & (VF_SHUTTER | VF_SHUTTER_SS | VF_ANIM_SHUTTER | VF_ANIM_SHUTTER_SS)) != 0; }  // the sub-frame loop stores
// PATH_ADAPT, ANIM_ADAPT (rt_set_path_adaptive_sampling): PATH's and ANIM's view and scene reads -- the records built for
// the sample frame, as for PATH_SS -- with ADAPT's lane mapping (sample_pixel) and decision loop (adaptive_tile).
// SHUTTER_ADAPT, ANIM_SHUTTER_ADAPT (rt_set_shutter_adaptive_sampling): SHUTTER's and ANIM_SHUTTER's view and scene reads
// -- record `rec`, built for the sample frame as for SHUTTER_SS -- with ADAPT's lane mapping, and a decision loop of their
// own over sub-frames and passes (shutter_adaptive_tile).  The tile trace needs the record index and the sample pass side
// by side: they arrive packed in its one wave-uniform argument, pass << REC_BITS | rec (n_frames x shutter <=
// RT_MAX_PATH_FRAMES < 2^16 records, pass < 64), and are split with scalar operations at its top.
constexpr bool shutter_adapt_of(unsigned V) { return (V & VF_VIEW_SHUTTER_ADAPT) != 0; }
constexpr bool adapt_of(unsigned V) { return (V & (VF_ADAPT | VF_VIEW_ADAPT | VF_VIEW_SHUTTER_ADAPT)) != 0; }  // a lane is an output pixel, rec the pass
constexpr int REC_BITS = 16;
static_assert(RT_MAX_PATH_FRAMES < (1 << REC_BITS), "a shutter launch's record index fits the low bits of the tile trace's argument");
template <int PATH>
struct ViewOf {
    const LaunchParams& p;
    int rec = 0;
    __device__ __forceinline__ const DevView& v() const { return p.views[PATH == VIEW_SHUTTER || PATH == VIEW_ANIM_SHUTTER ? (unsigned)rec : blockIdx.z]; }
    __device__ __forceinline__ f3 cam() const {
        if constexpr (PATH != VIEW_ARGS) return mk(v().cam[0], v().cam[1], v().cam[2]);
        else return mk(p.cam[0], p.cam[1], p.cam[2]);
    }
    __device__ __forceinline__ f3 right() const {
        if constexpr (PATH != VIEW_ARGS) return mk(v().right[0], v().right[1], v().right[2]);
        else return mk(p.right[0], p.right[1], p.right[2]);
    }
    __device__ __forceinline__ f3 up() const {
        if constexpr (PATH != VIEW_ARGS) return mk(v().up[0], v().up[1], v().up[2]);
        else return mk(p.up[0], p.up[1], p.up[2]);
    }
    __device__ __forceinline__ f3 fwd() const {
        if constexpr (PATH != VIEW_ARGS) return mk(v().fwd[0], v().fwd[1], v().fwd[2]);
        else return mk(p.fwd[0], p.fwd[1], p.fwd[2]);
    }
    __device__ __forceinline__ int prim_const() const {
        if constexpr (PATH != VIEW_ARGS) return v().prim_const;
        else return p.prim_const;
    }
    __device__ __forceinline__ const PrimConst* pc() const {
        if constexpr (PATH != VIEW_ARGS) return v().pc;
        else return p.pc;
    }
    __device__ __forceinline__ const PrimBox* pbox() const {
        if constexpr (PATH != VIEW_ARGS) return v().pbox;
        else return p.pbox;
    }
    __device__ __forceinline__ int mbox_n() const {
        if constexpr (PATH != VIEW_ARGS) return v().mbox_n;
        else return p.mbox_n;
    }
    __device__ __forceinline__ int mbox_plane(int k) const {
        if constexpr (PATH != VIEW_ARGS) return v().mbox_plane[k];
        else return p.mbox_plane[k];
    }
    __device__ __forceinline__ float mbox_tmax(int k) const {
        if constexpr (PATH != VIEW_ARGS) return v().mbox_tmax[k];
        else return p.mbox_tmax[k];
    }
    __device__ __forceinline__ const PrimBox* mbox(int k) const {
        if constexpr (PATH != VIEW_ARGS) return v().mbox[k];
        else return p.mbox[k];
    }
    // plane footprints (rt_foot.h): the one-view launches only -- a DevView record carries none, so the PATH and
    // SHUTTER instantiations compile nothing of the sky test
    __device__ __forceinline__ int foot_n() const {
        if constexpr (PATH != VIEW_ARGS) return -1;
        else return p.foot_n;
    }
};

// The scene of the wave's frame: the 12 scene tables of LaunchParams, read through this accessor everywhere.  ANIM
// (a scene track: one scene image per grid z, LaunchParams::scene_stride bytes apart): frame z's table is the
// launch's pointer + z * scene_stride.  blockIdx.z and the stride are wave-uniform, so the address is scalar
// arithmetic and the reads stay the scalar loads they are in every other instantiation.  The tables a scene may lack
// (shcull, shpre, shg, shgrid, shslab, clus, shgrp) stay null when they are null in the block; sph, mat, pl, li and
// scull are set by every launch (rt_api.cpp scene_params).  Any other view kind: the pointer itself, a compile-time
// identity -- the code of those instantiations is what it was (static members: an accessor object's temporary inside
// a short-circuit chain moved the class-0 bundle kernels' SGPR spills by up to 15).  The kind travels as the PATH
// parameter that ViewOf takes; the functions that read the scene have no default for it, so no call can fall back to
// the launch's image.
// ANIM_SHUTTER (a scene track under a shutter: one scene image per sub-frame): the table of sub-frame `rec` = z <<
// shutter_log2 | s is the launch's pointer + rec * scene_stride.  `rec` is the value ViewOf takes, made of blockIdx.z, a
// kernarg and shutter_tile's wave-uniform loop counter, so the address stays scalar arithmetic and the reads scalar
// loads; it reaches every function that reads a scene table as a parameter without a default, and every accessor takes
// it.  The other kinds never read it: for them it is a dead argument of inlined functions (in the ADAPT and PROG
// kernels the sample pass travels in it, as it does for ViewOf).
template <int PATH>
struct SceneOf {
    template <bool NULLABLE, typename T>
    static __device__ __forceinline__ const T* at(const LaunchParams& p, const T* q, int rec) {
        if constexpr (PATH == VIEW_ANIM || PATH == VIEW_ANIM_SHUTTER) {
            const size_t i = PATH == VIEW_ANIM_SHUTTER ? (size_t)(unsigned)rec : (size_t)blockIdx.z;
            const T* z = (const T*)((const char*)q + i * (size_t)p.scene_stride);
            if constexpr (NULLABLE) return q == nullptr ? nullptr : z;
            else return z;
        } else {
            return q;
        }
    }
    static __device__ __forceinline__ const DevSphere* sph(const LaunchParams& p, int rec) { return at<false>(p, p.sph, rec); }
    static __device__ __forceinline__ const DevMaterial* mat(const LaunchParams& p, int rec) { return at<false>(p, p.mat, rec); }
    static __device__ __forceinline__ const DevPlane* pl(const LaunchParams& p, int rec) { return at<false>(p, p.pl, rec); }
    static __device__ __forceinline__ const DevLight* li(const LaunchParams& p, int rec) { return at<false>(p, p.li, rec); }
    static __device__ __forceinline__ const DevSphereCull* scull(const LaunchParams& p, int rec) { return at<false>(p, p.scull, rec); }
    static __device__ __forceinline__ const DevShadowCull* shcull(const LaunchParams& p, int rec) { return at<true>(p, p.shcull, rec); }
    static __device__ __forceinline__ const DevShadowCull* shpre(const LaunchParams& p, int rec) { return at<true>(p, p.shpre, rec); }
    static __device__ __forceinline__ const DevShadowGrid* shg(const LaunchParams& p, int rec) { return at<true>(p, p.shg, rec); }
    static __device__ __forceinline__ const unsigned long long* shgrid(const LaunchParams& p, int rec) { return at<true>(p, p.shgrid, rec); }
    static __device__ __forceinline__ const unsigned long long* shslab(const LaunchParams& p, int rec) { return at<true>(p, p.shslab, rec); }
    static __device__ __forceinline__ const DevCluster* clus(const LaunchParams& p, int rec) { return at<true>(p, p.clus, rec); }
    static __device__ __forceinline__ const DevShadowGroups* shgrp(const LaunchParams& p, int rec) { return at<true>(p, p.shgrp, rec); }
};

// Deep-recursion stack (recursion limits >= 8): whole records {hit point, t} and {incoming
// direction, primitive code}, dynamically indexed, in scratch.
template <int K>
struct ScratchStack {
    float4 a[K], b[K];
    int n = 0;
    __device__ __forceinline__ ScratchStack(float2*, float*) {}
    __device__ __forceinline__ void origin(f3) {}
    __device__ __forceinline__ void push(float4 x, float4 y) {
        a[n] = x;
        b[n] = y;
        ++n;
    }
    template <int PATH>
    __device__ __forceinline__ void pop(const LaunchParams&, float4& x, float4& y, int = 0) {
        --n;
        x = a[n];
        y = b[n];
    }
    // the level-0 record (n >= 1), as pop hands it out; the stack is left as it is
    template <int PATH>
    __device__ __forceinline__ void level0(const LaunchParams&, float4& x, float4& y, int = 0) {
        x = a[0];
        y = b[0];
    }
    __device__ __forceinline__ int code0() const { return __float_as_int(b[0].w); }  // level 0's primitive code
};

// One reflection step of the forward walk (TraceSphere :854 / TracePlane normal,
// CalculateReflectionRay :718-720): hit point of segment (o, d) at t, then the reflected
// segment.  The walks and the compact stacks' re-walk share it, so the re-walk reproduces
// every hit point and direction bit for bit.
template <int PATH>
__device__ __forceinline__ f3 reflect_at(const LaunchParams& p, f3 o, f3& d, float t, int code, int rec) {
    const f3 hp = add(o, scale(d, t));
    f3 normal;
    if (code >= 0) {
        const DevSphere& s = SceneOf<PATH>::sph(p, rec)[code];
        normal = normalize(sub(hp, mk(s.cx, s.cy, s.cz)));
    } else {
        const DevPlane& pl = SceneOf<PATH>::pl(p, rec)[~code];
        normal = mk(pl.nx, pl.ny, pl.nz);
    }
    d = sub(d, scale(normal, 2.0f * dot(d, normal)));
    return hp;
}

// Compact levels: a record is fully determined by the camera ray and the (t, primitive)
// pairs of the levels above it, so each level keeps only those 8 bytes and pop rebuilds the
// record by re-walking the reflection chain with reflect_at (bit-identical).
// Level stack for limits 0..7: the compact levels and the primary direction in LDS, one slot per thread
// ([level][thread], conflict-free), so they cost no VGPRs; pop re-walks as in CompactStack.
template <int K>
struct LdsStack {
    float2* lv;  // [K][WG_THREADS] (t, primitive code) of this workgroup
    float* dv;   // [3][WG_THREADS] primary direction
    int n = 0;
    __device__ __forceinline__ LdsStack(float2* l, float* dd) : lv(l), dv(dd) {}
    __device__ __forceinline__ void origin(f3 d) {
        dv[(threadIdx.x & 63)] = d.x;
        dv[WG_THREADS + (threadIdx.x & 63)] = d.y;
        dv[2 * WG_THREADS + (threadIdx.x & 63)] = d.z;
    }
    __device__ __forceinline__ void push(float4 x, float4 y) {
        lv[n * WG_THREADS + (threadIdx.x & 63)] = make_float2(x.w, y.w);
        ++n;
    }
    template <int PATH>
    __device__ __forceinline__ void pop(const LaunchParams& p, float4& x, float4& y, int rec = 0) {
        --n;
        f3 o = ViewOf<PATH>{p, rec}.cam();
        f3 d = mk(dv[(threadIdx.x & 63)], dv[WG_THREADS + (threadIdx.x & 63)], dv[2 * WG_THREADS + (threadIdx.x & 63)]);
#pragma unroll 1
        for (int j = 0; j < K - 1; ++j) {
            const bool go = j < n;
            if (__builtin_amdgcn_ballot_w64(go) == 0) break;
            if (go) {
                const float2 tc = lv[j * WG_THREADS + (threadIdx.x & 63)];
                o = reflect_at<PATH>(p, o, d, tc.x, __float_as_int(tc.y), rec);
            }
        }
        const float2 tk = lv[n * WG_THREADS + (threadIdx.x & 63)];
        const f3 hp = add(o, scale(d, tk.x));
        x = make_float4(hp.x, hp.y, hp.z, tk.x);
        y = make_float4(d.x, d.y, d.z, tk.y);
    }
    // the level-0 record (n >= 1) without a re-walk: pop's own operations at n = 0 -- the camera, the primary
    // direction, hp = cam + d t -- and no loop; the stack is left as it is
    template <int PATH>
    __device__ __forceinline__ void level0(const LaunchParams& p, float4& x, float4& y, int rec = 0) {
        const f3 o = ViewOf<PATH>{p, rec}.cam();
        const f3 d = mk(dv[(threadIdx.x & 63)], dv[WG_THREADS + (threadIdx.x & 63)], dv[2 * WG_THREADS + (threadIdx.x & 63)]);
        const float2 tk = lv[(threadIdx.x & 63)];
        const f3 hp = add(o, scale(d, tk.x));
        x = make_float4(hp.x, hp.y, hp.z, tk.x);
        y = make_float4(d.x, d.y, d.z, tk.y);
    }
    __device__ __forceinline__ int code0() const { return __float_as_int(lv[(threadIdx.x & 63)].y); }  // level 0's primitive code
};

// Stack type per K (= recursion limit + 1 records): the LDS stack up to 8 levels (A/B round 1:
// no VGPRs for records, -2..-5.5 % on C4/C5 against register and hybrid stacks), scratch beyond.
template <int K>
struct StackFor {
    using type = ScratchStack<K>;
    static constexpr int lds_levels = 0;
};
#define RT_LDS_STACK(K)                        \
    template <>                                \
    struct StackFor<K> {                       \
        using type = LdsStack<K>;              \
        static constexpr int lds_levels = K;   \
    };
RT_LDS_STACK(1)
RT_LDS_STACK(2)
RT_LDS_STACK(4)
RT_LDS_STACK(6)
RT_LDS_STACK(8)
#undef RT_LDS_STACK

// Sum of v over the wave (all lanes active): bit-sliced ballots and scalar popcounts, no
// LDS round trips; the loop runs once per significant bit of the largest v (uniform).
__device__ __forceinline__ unsigned wave_count(unsigned v) {
    unsigned s = 0;
    for (int j = 0; __builtin_amdgcn_ballot_w64(v != 0u) != 0; ++j, v >>= 1)
        s += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64((v & 1u) != 0u)) << j;
    return s;
}

// Per-lane work counts share one register: reflected segments (<= RT_MAX_RECURSION_LIMIT + 1)
// in the low byte, shadow rays (<= lights x 64; rt_set_scene caps lights at 65536) above.
constexpr unsigned CNT_SHADOW_SHIFT = 8;
constexpr unsigned CNT_REFL_MASK = 0xFFu;

// Executed-work tally of the diagnostic kernels (STATS = true; never the timed ones): exact
// IntersectsSphere / IntersectPlane evaluations a lane actually ran, and the shadow rays whose
// sphere loop ran (a shadow ray is skipped when its outcome cannot change the pixel, and culling
// skips sphere tests that provably cannot select) -- reported beside the nominal counts of
// SURVEY.md 8(d), which count every primitive of every ray.
// SMAX > 0: the scene has at most SMAX spheres (a compile-time bound: the pair loops over the
// sphere table are unrolled, no loop counter or pointer arithmetic on the scalar unit).
#ifndef RT_SLOT_TALLY
#define RT_SLOT_TALLY 0
#endif
// RT_SHADOW_CAT=1 (diagnostic builds, tools/shadow_slots.py): sphere_tests_run counts only the
// bundle kernel's shadow-test lane slots of one category, chosen at run time by rt_count_work's
// selector (RT_DIAG_SEL = 16 * category + level + 1, level -1 = every fold level): category 1
// useful (needed, not yet blocked), 2 needed but already blocked, 3 diffuse but not needed,
// 4 active record, not diffuse, 5 no record at this level.
#ifndef RT_SHADOW_CAT
#define RT_SHADOW_CAT 0
#endif

template <bool ON, int SMAX = 0>
struct Tally {
    static constexpr int smax = SMAX;
    __device__ __forceinline__ void sphere(bool) {}
    __device__ __forceinline__ void shadow_sphere(bool) {}
    __device__ __forceinline__ void plane(bool) {}
    __device__ __forceinline__ void shadow(bool) {}
    __device__ __forceinline__ void init(const LaunchParams&) {}
    __device__ __forceinline__ void set_level(int) {}
    __device__ __forceinline__ void shadow_cat(int, unsigned) {}
    __device__ __forceinline__ void shadow_masks(int, unsigned long long) {}
};
template <int SMAX>
struct Tally<true, SMAX> {
    static constexpr int smax = SMAX;
    unsigned s = 0, pl = 0, sh = 0;
    int lvl = 0, sel_cat = 0, sel_lvl = -1;
    // RT_SLOT_TALLY (diagnostic builds, tools/slot_probe.py): lane slots of the exact tests,
    // useful or not -- 1: every sphere test, 2: the nearest-hit tests only
    __device__ __forceinline__ void sphere(bool c) { s += (!RT_SHADOW_CAT && (RT_SLOT_TALLY || c)) ? 1u : 0u; }
    __device__ __forceinline__ void shadow_sphere(bool c) {
        s += (!RT_SHADOW_CAT && (RT_SLOT_TALLY == 1 || c)) ? 1u : 0u;
    }
    __device__ __forceinline__ void plane(bool c) { pl += c ? 1u : 0u; }
    __device__ __forceinline__ void shadow(bool c) { sh += c ? 1u : 0u; }
    __device__ __forceinline__ void init(const LaunchParams& p) {
        sel_cat = p.enc_frame0 / 16;
        sel_lvl = p.enc_frame0 % 16 - 1;
    }
    __device__ __forceinline__ void set_level(int l) { lvl = l; }
    __device__ __forceinline__ void shadow_cat(int cat, unsigned n) {
        s += (RT_SHADOW_CAT && cat + 1 == sel_cat && (sel_lvl < 0 || lvl == sel_lvl)) ? n : 0u;
    }
    // categories 6 / 7 (lane 0 only): candidates per light's shadow pass / of the union of a shaded
    // level's lights -- how far the lights' candidate sets overlap
    __device__ __forceinline__ void shadow_masks(int cat, unsigned long long m) {
        if (RT_SHADOW_CAT && cat + 1 == sel_cat && (sel_lvl < 0 || lvl == sel_lvl) && (threadIdx.x & 63) == 0)
            s += (unsigned)__builtin_popcountll(m);
    }
};

// Work counters of one wave (converged call): ballot/popcount sums, lane 0 adds the wave's
// totals to slot (wave id % COUNTER_SLOTS); primary rays are the traced pixels, counted on the
// host.  Every frame of a batch launch (grid z) traces the same view with the same
// LaunchParams, so its counts are identical: frame 0 counts for all n_frames of them -- one
// atomic pair per wave per launch instead of per frame (each device-scope atomic is a memory
// round trip on MI355X, 32 B of HBM write traffic).  In a one-frame launch every wave counts, and
// the atomics cost the frame more than their round trips: C2 19.6 -> 22.5 us, C3 36.1 -> 39.6 us,
// C4 337 -> 352 us per lone frame (+15 % L2 requests, +22 % waves parked on memory; spreading them
// over 8192 slots instead of 256 changed nothing, profiles/r05_bundle_lone.txt) -- so a
// display loop that never reads rt_get_stats turns them off (rt_set_counting, ABI 10).
// PATH (camera-path launches): every frame has its own camera and so its own counts -- each z counts for
// itself, an atomic pair per wave per frame (counting off spares them as in any launch).  SHUTTER: shutter_tile
// counts, every sub-frame for itself, and adds the wave's totals once.
template <bool ST, int PATH = VIEW_ARGS, int SM>
__device__ __forceinline__ void add_counters(const LaunchParams& p, int lane, unsigned n_refl, unsigned n_shadow,
                                             const Tally<ST, SM>& tl) {
    // wave-uniform: the first frame (behind a copy slice) counts, and only when the context counts at all
    if ((!PATH && blockIdx.z != (unsigned)p.copy_z) || p.counters == nullptr) return;
    const unsigned long long nf = !PATH && p.n_frames > 1 ? (unsigned long long)p.n_frames : 1ull;
    const unsigned b = wave_count(n_refl), c = wave_count(n_shadow);
    const unsigned slot = (blockIdx.y * gridDim.x + blockIdx.x) % COUNTER_SLOTS;
    unsigned long long* q = &p.counters[slot * COUNTER_STRIDE];
    if (lane == 0) {
        if (b) atomicAdd(q + CNT_REFLECT, b * nf);
        if (c) atomicAdd(q + CNT_SHADOW, c * nf);
    }
    if constexpr (ST) {
        const unsigned s = wave_count(tl.s), pl = wave_count(tl.pl), sh = wave_count(tl.sh);
        if (lane == 0) {
            if (sh) atomicAdd(q + CNT_SHADOW_RUN, sh * nf);
            if (s) atomicAdd(q + CNT_SPHERE_RUN, s * nf);
            if (pl) atomicAdd(q + CNT_PLANE_RUN, pl * nf);
        }
    }
}

// Plane-uniform waves of the direct kernel (trace_tile_direct), A/B builds: RT_UNIFORM_PLANE=0 compiles the
// classification and the converged level-0 fold out.
#ifndef RT_UNIFORM_PLANE
#define RT_UNIFORM_PLANE 1
#endif
// The shadow pre-test's group records in those waves (shadow_scan's GROUPS), A/B builds: RT_SHADOW_GROUPS=0 compiles
// the hierarchical path out.
#ifndef RT_SHADOW_GROUPS
#define RT_SHADOW_GROUPS 1
#endif

// Result of a nearest-hit search.
struct Hit {
    float t;
    int prim;  // >= 0 sphere, ~plane for planes, or HIT_NONE
};
constexpr int HIT_NONE = 0x7fffffff;

// Nearest-hit selection rules as selects (VALU compares and cndmasks, no scalar mask logic),
// on the bit patterns: with u(x) = bits(x) - 1 (unsigned, wrapping), +0, every negative value and
// every NaN map above u(+inf) = 0x7f7fffff, and positive floats keep their order.  `best` is
// always +inf or a taken positive distance, so "x > 0 && x < best" is exactly u(x) < u(best)
// (x = +inf: u(x) = u(+inf) >= u(best), not taken, as in the float rule) -- one compare and a
// min instead of two compares and two selects (C4 -0.5 %, C2/C3 +-0,
// profiles/ab/r02_umin_take.txt).
// TracePixel (:977, :987): t is taken iff t > 0 && best > t.
__device__ __forceinline__ void take_primary(float t, int i, float& best, int& win) {
    const unsigned u = __float_as_uint(t) - 1u, ub = __float_as_uint(best) - 1u;
    win = u < ub ? i : win;
    best = __uint_as_float(min(u, ub) + 1u);
}
// TraceSecondaryRay (:804-806): t is taken iff t - 0.01 > 0 && t - 0.01 < best, and then
// best = t (the asymmetric rule, Q5/Q6).
__device__ __forceinline__ void take_secondary(float t, int i, float& best, int& win) {
    const float tm = t - 0.01f;
    const bool b = __float_as_uint(tm) - 1u < __float_as_uint(best) - 1u;
    best = b ? t : best;
    win = b ? i : win;
}

// A plane test in a nearest-plane search (TracePixel :985-991, TraceSecondaryRay :819-821 -- the same rule):
// t = num / den is selectable only when t > 0, i.e. num and den nonzero with equal signs (zeros give +-0,
// +-inf or NaN, and +inf never beats the initial +inf); when no lane of the wave (of the active lanes, in
// divergent code) has such a pair the division and the selection are skipped -- the upper half of a
// frame for a floor, rays leaving a wall -- and otherwise every lane takes the literal quotient.
__device__ __forceinline__ void plane_take(f3 o, f3 d, const DevPlane& q, int i, float& best, int& win) {
    const float num = ((-o.x * q.nx - o.y * q.ny) - o.z * q.nz) + q.cn;
    const float den = dot(d, mk(q.nx, q.ny, q.nz));
    const bool may = (num > 0.0f && den > 0.0f) || (num < 0.0f && den < 0.0f);
    if (__builtin_amdgcn_ballot_w64(may) != 0) take_primary(num / den, i, best, win);  // (wave-uniform)
}

// DIRECT path (scenes with < CULL_MIN_SPHERES spheres): per-lane divergent walks, wave-uniform
// primitive loops.  Shading of one shaded hit (TraceSphere :847-873 / TracePlane :736-778): the
// colour is accumulated in the reference's order -- mirror term (from the deeper segment `sec`),
// then each light, then ambient.  Returns the colour; adds shadow rays to *n_shadow.
// A light's shadow test can change the pixel only through I * att * phong vs 0 * phong.  When
// every phong component is +-0 or NaN and I * att is finite, both give +-0 / NaN per
// component (the sign of a zero never reaches a pixel: only additions, products, IEEE max and
// the final clamp follow), so the test is skipped.  Ray counters are unchanged
// (shadow rays = shaded diffuse hits x lights); the diagnostic tally counts the tests that ran.
__device__ __forceinline__ bool zero_or_nan(float v) { return !(v != 0.0f && v == v); }
__device__ __forceinline__ bool shadow_matters(f3 ph, float intensity, float att) {
    const float ia = intensity * att;
    const bool finite = __builtin_fabsf(ia) < __builtin_inff();
    return !(finite && zero_or_nan(ph.x) && zero_or_nan(ph.y) && zero_or_nan(ph.z));
}

// Loop over the sphere table two spheres at a time (the device table is padded to an even count
// with a sphere that never hits, rt_set_scene): body(i) tests spheres i and i + 1.  Unrolled
// when the scene's sphere count has a compile-time bound (T::smax).
template <typename T, typename F>
__device__ __forceinline__ void for_sphere_pairs(const LaunchParams& p, F body) {
    if constexpr (T::smax > 0) {
#pragma unroll
        for (int i = 0; i < T::smax; i += 2) {
            if (i >= p.S) break;  // wave-uniform
            body(i);
        }
    } else {
        for (int i = 0; i < p.S; i += 2) body(i);
    }
}

// IntersectShadowLight's sphere loop (:577-579) for the active lanes: every sphere, a lane's
// result the OR of its tests, as in the reference.  The scalar unit bounds these kernels (one per
// CU for 4 SIMDs, profiles/r02_issue_probe.txt), so the loop is shaped for scalar economy: the
// blocked state is a VGPR value (no lane-mask phi), one 32-byte scalar load per pair, no per-lane
// loop exits (their mask bookkeeping cost ~28 scalar instructions per sphere) and no wave exit
// once every lane is blocked (it almost never fires: C2 -1.4 %, C3 -1.0 % without it,
// profiles/ab/r02_shadow_loop.txt).
// With 2a finite-positive (A2OK) and the scene's pre-test records (p.shpre, built for every S < CULL_MIN_SPHERES
// scene), a sphere's exact test runs only when some lane's pre-test keeps it: the exact pre-test (oc, b, c, disc,
// ~20 VALU) costs more than the pre-test (~10 VALU on the lane's hit point in light l's frame, computed once per
// scan), and on C2/C3 most spheres are kept by no lane of the wave (C3 -7.8 %, C2 -4.0 % per frame,
// profiles/ab/r06_direct_shadow_pre.txt).
//
// The pre-test itself (ShadowPreLane, shadow_pre_lane, shadow_pre_keep) lives in rt_shadow_pre.h, shared with the
// host check of the records.
//
// GROUPS (the converged level 0 of a plane-uniform wave, with the scene's group records p.shgrp): a scanning floor
// wave runs S per-lane pre-tests per light and on C3 about 15.7 of its 16 only establish that nothing is near.  The
// union record of the light's bounding hierarchy (DevShadowGroups, rt_scene.h build_shadow_groups: the proof) is
// tested first, by the same function with the lane margin widened once: no lane keeps the union -- not blocked, no
// sphere visited; otherwise the flat loop as it stands.  A sphere some lane's pre-test keeps keeps the union, so the
// same spheres are tested exactly, in the same ascending order: pixels, ray counts and the tallies are unchanged.
// The group level on top (a member mask from the three group records, pairs outside it skipped) gained no more on C3
// and cost the scan without records 0.3 us in spilled SGPRs and serial scalar loads: profiles/ab/r15_shadow_groups.txt.
template <bool A2OK, bool GROUPS, int PATH, typename T>
__device__ __forceinline__ bool shadow_scan(const LaunchParams& p, f3 hp, const DevLight& l, int li, T& tl, int rec) {
    int blk = 0;
    if (A2OK && SceneOf<PATH>::shpre(p, rec) != nullptr) {  // wave-uniform
        const ShadowPreLane q = shadow_pre_lane(hp.x, hp.y, hp.z, l);
        if constexpr (GROUPS) {
            // wave-uniform: no lane keeps the union of the light's discs -- not blocked, no sphere visited
            if (SceneOf<PATH>::shgrp(p, rec) != nullptr &&
                __builtin_amdgcn_ballot_w64(shadow_pre_keep(shadow_pre_widen(q, SHADOW_UNION_WIDEN), SceneOf<PATH>::shgrp(p, rec)[li].uni)) == 0)
                return false;
        }
        const DevShadowCull* e = SceneOf<PATH>::shpre(p, rec) + (size_t)li * (size_t)(p.S + (p.S & 1));
        for_sphere_pairs<T>(p, [&](int i) {
            const DevShadowCull e0 = e[i], e1 = e[i + 1];
            const bool k0 = shadow_pre_keep(q, e0), k1 = shadow_pre_keep(q, e1);
            if (__builtin_amdgcn_ballot_w64(k0) != 0) {  // wave-uniform: some lane's ray may be blocked
                tl.shadow_sphere(blk == 0);
                blk = shadow_blocked<A2OK>(hp, l, false, SceneOf<PATH>::sph(p, rec)[i]) ? 1 : blk;
            }
            if (__builtin_amdgcn_ballot_w64(k1) != 0) {
                tl.shadow_sphere(blk == 0);
                blk = shadow_blocked<A2OK>(hp, l, false, SceneOf<PATH>::sph(p, rec)[i + 1]) ? 1 : blk;
            }
        });
        return blk != 0;
    }
    for_sphere_pairs<T>(p, [&](int i) {
        tl.shadow_sphere(blk == 0);
        const DevSphere s0 = SceneOf<PATH>::sph(p, rec)[i], s1 = SceneOf<PATH>::sph(p, rec)[i + 1];
        blk = shadow_blocked<A2OK>(hp, l, false, s0) ? 1 : blk;
        tl.shadow_sphere((blk == 0) & (i + 1 < p.S));
        blk = shadow_blocked<A2OK>(hp, l, false, s1) ? 1 : blk;
    });
    return blk != 0;
}

template <bool GPOW, bool GROUPS, int PATH, typename T>
__device__ __forceinline__ f3 shade_direct(const LaunchParams& p, bool is_sphere, int prim, f3 hp, f3 d, float t, f3 sec,
                                           unsigned* n_shadow, T& tl, int rec) {
    const DevMaterial& m = SceneOf<PATH>::mat(p, rec)[is_sphere ? prim : p.S + prim];
    const uint32_t flags = m.flags;
    f3 normal;
    float tile = 1.0f;
    // A plane hit on a dark square whose light terms are provably +0 (rt_dark.h): the light loop is skipped
    bool dark = false;
    if (is_sphere) {
        const DevSphere& s = SceneOf<PATH>::sph(p, rec)[prim];
        normal = normalize(sub(hp, mk(s.cx, s.cy, s.cz)));  // SpherePhongShading :706
    } else {
        const DevPlane& pl = SceneOf<PATH>::pl(p, rec)[prim];
        normal = mk(pl.nx, pl.ny, pl.nz);
        // checkerboard, :766-770: ((int)u + (int)v) & 1, unchecked int add
        const float u = dot(mk(pl.e1x, pl.e1y, pl.e1z), hp);
        const float v = dot(mk(pl.e2x, pl.e2y, pl.e2z), hp);
        tile = checker_tile(u, v);
        dark = (flags & MAT_DARK_OK) != 0 && dark_lane_ok(hp.x, hp.y, hp.z, t, dot(d, d), tile);
    }
    f3 col = mk(0.0f, 0.0f, 0.0f);
    if (flags & MAT_MIRROR) col = add(col, mul(sec, mk(m.km[0], m.km[1], m.km[2])));
    if ((flags & MAT_DIFFUSE) && !dark) {
        const f3 view = normalize(d);  // ShapePhongShading :668 (not negated)
        // sphere: (1 / t) * t (:866);  plane: (float)(1 / Math.Pow(t, 2)) (:754), exact as 1/(t*t) in f64
        const float att = is_sphere ? sphere_att(t) : plane_att(t);
        const f3 kd = mk(m.kd[0], m.kd[1], m.kd[2]);
        // the material's specular terms once, not per light under the MAT_SPEC branch
        const f3 ks = mk(m.ks[0], m.ks[1], m.ks[2]);
        const uint32_t pk = m.pow_kind;
        const float pn = m.n;
        for (int li = 0; li < p.L; ++li) {
            const DevLight& l = SceneOf<PATH>::li(p, rec)[li];
            const bool l_ok = l.a2 > 0.0f && l.a2 < __builtin_inff();  // wave-uniform
            // ShapePhongShading, :665-695 (first: it decides whether the shadow test matters)
            const f3 ldir = normalize(sub(mk(l.px, l.py, l.pz), hp));
            f3 ph = scale(kd, nmax0(dot(normal, ldir)));
            f3 spec = mk(0.0f, 0.0f, 0.0f);
            if (flags & MAT_SPEC) {
                const f3 rs = sub(ldir, scale(normal, 2.0f * dot(ldir, normal)));
                const float sp = spec_pow<GPOW>(nmax0(dot(view, normalize(rs))), pk, pn);
                spec = mul(ks, mk(sp, sp, sp));
            }
            ph = add(ph, spec);
            bool blocked = false;
            if (shadow_matters(ph, l.intensity, att)) {
                tl.shadow(true);
                blocked = l_ok ? shadow_scan<true, GROUPS, PATH>(p, hp, l, li, tl, rec) : shadow_scan<false, false, PATH>(p, hp, l, li, tl, rec);
            }
            const float inten = blocked ? 0.0f : l.intensity;
            const float ia = inten * att;
            f3 term = mul(mk(ia, ia, ia), ph);
            if (!is_sphere) {
                term = mul(term, mk(tile, tile, tile));
                term = mk(nmax0(term.x), nmax0(term.y), nmax0(term.z));  // .Max(0f), :775
            }
            col = add(col, term);
        }
    }
    // (the nominal count: shaded diffuse hits x lights, dark or not)
    if (flags & MAT_DIFFUSE) *n_shadow += (unsigned)p.L << CNT_SHADOW_SHIFT;
    return add(col, mk(m.amb[0], m.amb[1], m.amb[2]));
}

// Level 0 of a plane-uniform wave (trace_tile_direct): shade_direct's plane arm for a plane index `plane` that is the
// same on every active lane.  The same operations in the same order -- it is that function, inlined a second time
// with is_sphere the constant false and a wave-uniform index: the sphere arm is gone, the material and plane
// records arrive by scalar loads, and the flag tests and the exponent switch are scalar branches.  The dark-square
// test, the light loop, the shadow scans, the clamps and the counts stay per lane.  Converged call on the wave's
// level-0 lanes.
template <int PATH, typename T>
__device__ __forceinline__ f3 shade_plane_uniform(const LaunchParams& p, int plane, f3 hp, f3 d, float t, f3 sec,
                                                  unsigned* n_shadow, T& tl, int rec) {
    return shade_direct<false, RT_SHADOW_GROUPS != 0, PATH>(p, false, plane, hp, d, t, sec, n_shadow, tl, rec);
}

// Candidate spheres of a wave's primary rays: those whose per-frame screen box (view_params)
// overlaps the wave's pixels.  Lanes 0 and 63 hold the wave's first and last pixel (the row
// mapping is monotonic).  The wave's start has no dependent chain of memory round trips: the
// box is one unconditional 16-byte load (lane 0's for lanes >= S), tested without
// short-circuit branches.  Converged call; p.prim_const required.
__device__ __forceinline__ unsigned long long box_mask(const LaunchParams& p, const PrimBox* tab, int x, int y) {
    const int x_lo = __builtin_amdgcn_readlane(x, 0), x_hi = __builtin_amdgcn_readlane(x, 63);
    const int y_lo = __builtin_amdgcn_readlane(y, 0), y_hi = __builtin_amdgcn_readlane(y, 63);
    const int lane = threadIdx.x & 63;
    const bool in = lane < p.S;
    const PrimBox b = tab[in ? lane : 0];
    const bool cand = in & (b.x0 <= x_hi) & (b.x1 >= x_lo) & (b.y0 <= y_hi) & (b.y1 >= y_lo);
    return __builtin_amdgcn_ballot_w64(cand);
}
template <int PATH = VIEW_ARGS>
__device__ __forceinline__ unsigned long long prim_box_mask(const LaunchParams& p, int x, int y, int rec = 0) {
    return box_mask(p, ViewOf<PATH>{p, rec}.pbox(), x, y);
}
// Candidate spheres of the wave's first reflected segments off the boxed mirror planes (LaunchParams::mbox,
// rt_api.cpp mirror_boxes): table k's mask in bits [16 k, 16 k + S) of one wave-uniform word (S < CULL_MIN_SPHERES
// <= 16).  A lane whose primary hit is plane mbox_plane[k] with t <= mbox_tmax[k] reflects into a ray that can
// select only those spheres.  Converged call; 0 without tables.
template <int PATH = VIEW_ARGS>
__device__ __forceinline__ unsigned mirror_box_masks(const LaunchParams& p, int x, int y, int rec = 0) {
    const ViewOf<PATH> vw{p, rec};
    unsigned m = 0;
    if (vw.mbox_n() > 0) {  // wave-uniform
        m = (unsigned)box_mask(p, vw.mbox(0), x, y);
        if (vw.mbox_n() > 1) m |= (unsigned)box_mask(p, vw.mbox(1), x, y) << 16;
    }
    return m;
}
// The sphere mask of a wave's first reflected segment, chosen by the lanes still walking (divergent call, every
// active lane at count 1; t, prim: the lane's primary hit): every sphere when some lane left a sphere, a plane
// without a table or a plane beyond its t_max (NaN included), else the OR of the tables of the planes that were hit.
template <int PATH = VIEW_ARGS>
__device__ __forceinline__ unsigned mirror_box_select(const LaunchParams& p, unsigned masks, float t, int prim, int rec = 0) {
    const ViewOf<PATH> vw{p, rec};
    const int pi = ~prim;  // plane index; a sphere's (prim >= 0) is excluded below: ~0 would match an unused table's -1
    const bool on0 = prim < 0 && pi == vw.mbox_plane(0) && t <= vw.mbox_tmax(0);
    const bool on1 = prim < 0 && pi == vw.mbox_plane(1) && t <= vw.mbox_tmax(1);
    if (__builtin_amdgcn_ballot_w64(!(on0 || on1)) != 0) return ~0u;
    unsigned m = 0;
    if (__builtin_amdgcn_ballot_w64(on0) != 0) m |= masks & 0xffffu;
    if (__builtin_amdgcn_ballot_w64(on1) != 0) m |= masks >> 16;
    return m;
}

// A wave's pixels: column x, local row r -> frame row y (band band_first + (r / band_rows) *
// band_step), validity, and the view-table entries lx = lxt[x], ly = lyt[y] (0 outside).
// Fast paths without a per-lane integer division: one band (every full-frame launch) and the
// 8-row bands of the multi-GPU path; the view-table loads are unconditional.  SS (supersampling: W, H and
// the rows are in samples, so the 8-row bands of the multi-worker paths arrive as 16, 32 or 64 rows):
// power-of-two bands by shifts.
struct TilePixel {
    int x, r, y;
    bool valid;
    float lx, ly;
};
template <bool SS = false>
__device__ __forceinline__ TilePixel tile_pixel(const LaunchParams& p, int x, int r) {
    TilePixel t;
    t.x = x, t.r = r;
    if (p.band_rows >= p.local_rows) {  // wave-uniform branches
        t.y = p.band_first * p.band_rows + r;
    } else if (!SS && p.band_rows == 8) {
        t.y = (p.band_first + (r >> 3) * p.band_step) * 8 + (r & 7);
    } else if (SS && (p.band_rows & (p.band_rows - 1)) == 0) {
        const int sh = 31 - __builtin_clz((unsigned)p.band_rows);
        t.y = ((p.band_first + (r >> sh) * p.band_step) << sh) + (r & (p.band_rows - 1));
    } else {
        const int band = p.band_first + (r / p.band_rows) * p.band_step;
        t.y = band * p.band_rows + (r % p.band_rows);
    }
    t.valid = x < p.W && r < p.local_rows && t.y < p.H;
    const float lx = p.lxt[t.valid ? x : 0], ly = p.lyt[t.valid ? t.y : 0];  // unconditional loads
    t.lx = t.valid ? lx : 0.0f, t.ly = t.valid ? ly : 0.0f;
    return t;
}
// ADAPT (adaptive supersampling, adaptive_tile): the wave's tile is 8x8 output pixels, lane `lane` is pixel (rx, ry) =
// (lane & 7, lane >> 3) of it and traces sample (i, j) = (pass & (k - 1), pass >> ss_log2) of its pixel's k x k
// block, k = 1 << ss_log2: column (x << ss_log2) | i of local sample row (r << ss_log2) | j of the sample frame
// LaunchParams describes; `pass` is wave-uniform.  The mapping stays monotonic in the lane, so lanes 0 and 63 still
// hold the wave's extremes (box_mask).
__device__ __forceinline__ TilePixel sample_pixel(const LaunchParams& p, int tile_x, int tile_y, int lane, int pass) {
    const int x = tile_x * TILE_W + (lane & 7), r = tile_y * TILE_H + (lane >> 3), s2 = p.ss_log2;
    return tile_pixel<true>(p, (x << s2) | (pass & ((1 << s2) - 1)), (r << s2) | (pass >> s2));
}

// Sphere part of a nearest-hit search for the active lanes.  PRIMARY with p.prim_const: the
// per-frame camera-relative constants and the wave's screen-box candidates (pmask); otherwise
// every sphere (IntersectsSphere, :613-642).  A2OK: 2a finite-positive on every active lane.
// GATED (secondary segments of the K > 1 direct kernels): pmask is the wave-uniform sphere mask of the segment
// (mirror_box_select; all ones: every sphere) and a pair runs only when one of its bits is set -- a skipped
// sphere's test yields t <= 0 or NaN on every active lane, which take_secondary rejects, and the kept ones are
// still visited in ascending index.
template <bool PRIMARY, bool A2OK, bool GATED, int PATH, typename T>
__device__ __forceinline__ void nearest_spheres(const LaunchParams& p, f3 o, f3 d, float a2, float a4, bool a2_ok,
                                                unsigned long long pmask, float& best_s, int& win_s, T& tl, int rec) {
    if (PRIMARY && ViewOf<PATH>{p, rec}.prim_const()) {
        // o == camera: oc = cam - c and c = oc.oc - r^2 are the same per frame (:614-619);
        // only the wave's candidate spheres, in ascending order (non-candidates give t <= 0)
        for (unsigned long long m = pmask; m;) {
            const int i = (int)__builtin_ctzll(m);
            m &= ~(1ull << i);
            tl.sphere(true);
            const PrimConst pc = ViewOf<PATH>{p, rec}.pc()[i];
            const float b = 2.0f * dot(mk(pc.ocx, pc.ocy, pc.ocz), d);
            const float disc = b * b - a4 * pc.c;
            const float t = A2OK ? root_t1(b, disc, a2) : (a2_ok ? root_t1(b, disc, a2) : root_full(b, disc, a2));
            take_primary(t, i, best_s, win_s);
        }
    } else {
        // pairs (the device table is padded to an even count with a sphere that never hits)
        for_sphere_pairs<T>(p, [&](int i) {
            if constexpr (GATED) {
                if ((((unsigned)pmask >> i) & 3u) == 0) return;  // wave-uniform
            }
            tl.sphere(true);
            tl.sphere(i + 1 < p.S);
            const DevSphere s0 = SceneOf<PATH>::sph(p, rec)[i], s1 = SceneOf<PATH>::sph(p, rec)[i + 1];
            const float t0 = sphere_t<A2OK>(o, d, a2, a4, a2_ok, s0);
            const float t1 = sphere_t<A2OK>(o, d, a2, a4, a2_ok, s1);
            if (PRIMARY) {
                take_primary(t0, i, best_s, win_s);
                take_primary(t1, i + 1, best_s, win_s);
            } else {
                take_secondary(t0, i, best_s, win_s);
                take_secondary(t1, i + 1, best_s, win_s);
            }
        });
    }
}

template <bool PRIMARY, bool GATED, int PATH, typename T>
__device__ __forceinline__ Hit nearest_direct(const LaunchParams& p, f3 o, f3 d, T& tl, unsigned long long pmask, int rec) {
    const float a = dot(d, d);
    const float a2 = 2.0f * a, a4 = 4.0f * a;
    const bool a2_ok = a2 > 0.0f && a2 < __builtin_inff();
    float best_s = __builtin_inff();
    int win_s = -1;
    if (__builtin_amdgcn_ballot_w64(!a2_ok) == 0)  // wave-uniform (the usual case)
        nearest_spheres<PRIMARY, true, GATED, PATH>(p, o, d, a2, a4, a2_ok, pmask, best_s, win_s, tl, rec);
    else
        nearest_spheres<PRIMARY, false, GATED, PATH>(p, o, d, a2, a4, a2_ok, pmask, best_s, win_s, tl, rec);
    float best_p = __builtin_inff();
    int win_p = -1;
    for (int i = 0; i < p.P; ++i) {
        tl.plane(true);
        plane_take(o, d, SceneOf<PATH>::pl(p, rec)[i], i, best_p, win_p);  // t > 0 && t < best (:985-991, :819-821)
    }
    if (best_s < best_p) return Hit{best_s, win_s};
    if (win_p >= 0) return Hit{best_p, ~win_p};
    return Hit{0.0f, HIT_NONE};
}

// Terminal segment (bounce count > limit): only its colour is used -- One iff a plane is
// selected with t - 0.01 > 0 and no sphere beats it (TraceSecondaryRay :789-826 with the
// terminal colours of TracePlane :734 / TraceSphere :843), otherwise Zero.  Planes first:
// with no plane hit, or the nearest within 0.01, the colour is Zero whatever the spheres do,
// so they are not tested.  Returns HIT_NONE (Zero) or the plane hit (One);
// the walk classifies it exactly as it would the full nearest hit.
template <int PATH, typename T>
__device__ __forceinline__ Hit terminal_direct(const LaunchParams& p, f3 o, f3 d, T& tl, int rec) {
    float best_p = __builtin_inff();
    int win_p = -1;
    for (int i = 0; i < p.P; ++i) {
        tl.plane(true);
        plane_take(o, d, SceneOf<PATH>::pl(p, rec)[i], i, best_p, win_p);
    }
    if (win_p < 0 || !(best_p - 0.01f > 0.0f)) return Hit{0.0f, HIT_NONE};
    const float a = dot(d, d);
    const float a2 = 2.0f * a, a4 = 4.0f * a;
    const bool a2_ok = a2 > 0.0f && a2 < __builtin_inff();
    float best_s = __builtin_inff();
    int win_s = -1;
    if (__builtin_amdgcn_ballot_w64(!a2_ok) == 0)
        nearest_spheres<false, true, false, PATH>(p, o, d, a2, a4, a2_ok, 0, best_s, win_s, tl, rec);
    else
        nearest_spheres<false, false, false, PATH>(p, o, d, a2, a4, a2_ok, 0, best_s, win_s, tl, rec);
    if (best_s < best_p) return Hit{0.0f, HIT_NONE};  // a sphere is selected: Zero
    return Hit{best_p, ~win_p};
}

// Sky waves (rt_foot.h): no primary ray of the wave's pixels can select a sphere -- its pixels lie
// outside every screen box, pmask == 0 with the primary constants on -- or a plane: every valid lane fails every
// plane's footprint rule.  Such a wave's pixels are 0 and it casts no reflected or shadow ray.  Converged call;
// false without footprints (foot_n < 0: always in the PATH and SHUTTER instantiations, which compile none of this).
template <int PATH>
__device__ __forceinline__ bool sky_tile(const LaunchParams& p, const TilePixel& t, unsigned long long pmask, int rec) {
    const ViewOf<PATH> vw{p, rec};
    const int n = vw.foot_n();
    if (n < 0 || pmask != 0 || !vw.prim_const()) return false;  // wave-uniform
    bool may = false;
#pragma unroll
    for (int i = 0; i < FOOT_MAX; ++i) {
        if (i >= n) break;  // wave-uniform
        may |= foot_may_hit(p.foot[i], t.lx, t.ly);
    }
    return __builtin_amdgcn_ballot_w64(t.valid && may) == 0;
}

// What of a variant word (rt_internal.h VF_*) the trace of one tile depends on: everything but the workgroup
// shape and the tile order, which only pick the tile.  The kernel bodies hand trace_tile_{direct,bundle} the word
// masked by it, so one instantiation serves every shape and order.
constexpr unsigned VF_TILE = ~(vf_wpg(15) | vf_tord(3));

// What the trace of one tile hands back: the lane's packed counts, reflected segments (bits 0-7) | shadow rays
// << 8, and its pixel 0x00RRGGBB (outside the frame: a value nobody stores).  SHUTTER: the tile trace neither stores nor encodes -- the
// pixel goes back to the kernel body's sub-frame loop (shutter_tile), which stores the mean.
struct TileOut {
    unsigned cnt;
    uint32_t px32;
};

// DIRECT path, one 8x8 tile: each lane walks its own chain with per-lane (divergent) control
// flow.  rec: the sub-frame's view record (SHUTTER, wave-uniform; see ViewOf; ANIM_SHUTTER: its scene image as well, see
// SceneOf), or the sample pass (ADAPT, wave-uniform;
// sample_pixel) -- the ADAPT kernels have the one view of the launch parameters and ViewOf never reads it, and the
// PATH_ADAPT / ANIM_ADAPT kernels' views read blockIdx.z alone.
template <int K, unsigned V, bool UNIFORM_OK = true, typename T>
__device__ __forceinline__ TileOut trace_tile_direct(const LaunchParams& p, int tile_x, int tile_y, float2* stk_lv,
                                                     float* stk_dv, T& tl, int recp = 0) {
    constexpr bool GPOW = (V & VF_GPOW) != 0, TILES = (V & VF_TILES) != 0, SS = ss_of(V), SHUTTER = shutter_of(V);
    constexpr bool ADAPT = adapt_of(V);
    constexpr int PATH = view_of(V);
    // (SHUTTER_ADAPT: the sample pass above the record index; every other kernel: the one value it had)
    const int rec = shutter_adapt_of(V) ? recp & ((1 << REC_BITS) - 1) : recp, pass = shutter_adapt_of(V) ? recp >> REC_BITS : recp;
    // plane-uniform waves: not in the GPOW kernels, where a second inlined pow costs an occupancy step, nor where the
    // kernel body says so (UNIFORM_OK)
    constexpr bool UNIFORM = RT_UNIFORM_PLANE && UNIFORM_OK && !GPOW;
    const int lane = threadIdx.x & 63;
    const TilePixel tpx = ADAPT ? sample_pixel(p, tile_x, tile_y, lane, pass)
                                : tile_pixel<SS>(p, tile_x * TILE_W + (lane & 7), tile_y * TILE_H + (lane >> 3));
    const int x = tpx.x, r = tpx.r, y = tpx.y;
    const bool valid = tpx.valid;
    const ViewOf<PATH> vw{p, rec};
    const unsigned long long pmask = vw.prim_const() ? prim_box_mask<PATH>(p, x, y, rec) : 0;
    // a sky wave traces nothing: every valid lane's pixel is 0, no ray beyond the primary ones, no tally
    const bool sky = sky_tile<PATH>(p, tpx, pmask, rec);  // wave-uniform
    // K == 1 (limit 0): level 1 is a terminal segment, nothing of the mirrored boxes is compiled in
    unsigned mmask = 0;
    if constexpr (K > 1) {
        if (!sky) mmask = mirror_box_masks<PATH>(p, x, y, rec);
    }

    unsigned cnt = 0;  // packed: reflected segments (bits 0-7) | shadow rays << CNT_SHADOW_SHIFT
    typename StackFor<K>::type stk(stk_lv, stk_dv);
    f3 leaf = mk(0.0f, 0.0f, 0.0f);
    uint32_t px32 = 0;
    if (valid) {
        if (!sky) {  // wave-uniform
            const f3 cam = vw.cam();
            // TracePixel primary ray, :963-971 (no half-pixel offset)
            // lx = ((float)x / W - 0.5f) * pw, ly likewise: per-column / per-row tables built on
            // the host with the same binary32 operations (view_tables in rt_api.cpp)
            const float lx = tpx.lx, ly = tpx.ly, lz = 1.0f * p.nearc;
            const f3 vp = add(add(add(cam, scale(vw.right(), lx)), scale(vw.up(), ly)), scale(vw.fwd(), lz));
            f3 d = normalize(sub(vp, cam));
            f3 o = cam;

            stk.origin(d);
            Hit h = nearest_direct<true, false, PATH>(p, o, d, tl, pmask, rec);
            int count = 0;
            for (;;) {
                if (h.prim == HIT_NONE) break;      // nothing hit: plane colour stays Zero
                if (h.t - 0.01f <= 0.0f) break;     // too close: Zero (:731, :839)
                const bool is_sphere = h.prim >= 0;
                if (count > p.limit) {              // terminal segment: Zero / One (:734, :843)
                    if (!is_sphere) leaf = mk(1.0f, 1.0f, 1.0f);
                    break;
                }
                // shaded hit: record it; mirror hits continue with the reflected segment
                const f3 hp = add(o, scale(d, h.t));
                stk.push(make_float4(hp.x, hp.y, hp.z, h.t), make_float4(d.x, d.y, d.z, __int_as_float(h.prim)));
                const int prim = is_sphere ? h.prim : ~h.prim;
                const uint32_t flags = SceneOf<PATH>::mat(p, rec)[is_sphere ? prim : p.S + prim].flags;
                if (!(flags & MAT_MIRROR)) break;
                o = reflect_at<PATH>(p, o, d, h.t, h.prim, rec);  // :854, CalculateReflectionRay :718-720
                ++count;
                ++cnt;
                // count is the same for every lane still walking: no divergence here
                if constexpr (K > 1) {
                    // the first reflected segment: the spheres its mirrored boxes allow (when the wave has tables)
                    // (count read from the first active lane: a scalar branch, and the mask stays wave-uniform)
                    unsigned smask = ~0u;
                    if (vw.mbox_n() > 0 && __builtin_amdgcn_readfirstlane(count) == 1) smask = mirror_box_select<PATH>(p, mmask, h.t, h.prim, rec);
                    h = count > p.limit ? terminal_direct<PATH>(p, o, d, tl, rec) : nearest_direct<false, true, PATH>(p, o, d, tl, smask, rec);
                } else {
                    h = count > p.limit ? terminal_direct<PATH>(p, o, d, tl, rec) : nearest_direct<false, false, PATH>(p, o, d, tl, 0, rec);
                }
            }
            // backward fold: every recorded hit is shaded in reverse order; a mirror hit
            // consumes the colour of the segment after it (levels 0..limit push at most one
            // record each, so K = limit + 1 records suffice).  Per lane, divergent: the bundle
            // kernel's converged fold with wave-level shadow culling measured slower here (C2
            // +14 %, C3 +17 %, profiles/ab/r02_direct_converged_fold_rejected.txt)
            // Plane-uniform waves: the lanes with a record (stk.n > 0) are those that pushed a level-0 one, and the
            // wave is plane-uniform when there is such a lane and every one of them hit the plane of the first -- read
            // back from the stack, so that nothing of the test is live across the walk.  Lanes that missed or were
            // too close stay outside; a sphere silhouette or a seam between two planes in the tile leaves the wave to
            // the per-lane code.  A plane-uniform wave folds down to level 1 that way (floor_n, wave-uniform),
            // reconverges on its level-0 lanes and shades level 0 once, with the lane's folded colour (`leaf`
            // without a deeper record) as the mirror term's input.
            int floor_n = 0;
            if constexpr (UNIFORM) {
                const bool rec0 = stk.n > 0;
                const unsigned long long m0 = __builtin_amdgcn_ballot_w64(rec0);
                if (p.uniform_plane && m0 != 0) {  // wave-uniform
                    const int code = rec0 ? stk.code0() : 0;
                    const int code0 = __builtin_amdgcn_readlane(code, (int)__builtin_ctzll(m0));
                    if (code0 < 0 && __builtin_amdgcn_ballot_w64(rec0 && code != code0) == 0) floor_n = 1;
                }
            }
            f3 col = leaf;
            while (stk.n > floor_n) {
                float4 ra, rb;
                stk.template pop<PATH>(p, ra, rb, rec);
                const int code = __float_as_int(rb.w);
                const bool is_s = code >= 0;
                col = shade_direct<GPOW, false, PATH>(p, is_s, is_s ? code : ~code, mk(ra.x, ra.y, ra.z),
                                               mk(rb.x, rb.y, rb.z), ra.w, col, &cnt, tl, rec);
            }
            if constexpr (UNIFORM) {
                if (floor_n != 0 && stk.n != 0) {  // the level-0 lanes of a plane-uniform wave
                    float4 ra, rb;
                    stk.template level0<PATH>(p, ra, rb, rec);
                    const int plane = ~__builtin_amdgcn_readfirstlane(__float_as_int(rb.w));
                    col = shade_plane_uniform<PATH>(p, plane, mk(ra.x, ra.y, ra.z), mk(rb.x, rb.y, rb.z), ra.w, col, &cnt, tl, rec);
                }
            }
            px32 = (shift_channel(col.x) << 16) | (shift_channel(col.y) << 8) | shift_channel(col.z);
        }
        if constexpr (!TILES && !SS && !SHUTTER && !ADAPT) store_pixel(p, r, y, x, px32);
    }
    if constexpr (TILES) encode_tile_fused(p, px32, valid);
    if constexpr (SS && !SHUTTER) resolve_tile(p, r, y, x, valid, px32);
    return TileOut{cnt, px32};
}

// SHUTTER (rt_render_shutter_bands): the wave's tile of output frame z = blockIdx.z is the mean of m = 1 <<
// shutter_log2 sub-frames, traced one after the other by `trace(p, rec, tile_x, tile_y)` with the view record rec =
// z << t | s.  The running per-channel sums (rt_resolve.h: two words of 16-bit fields, exact up to 256 sub-frames)
// are the only vector values carried across the loop; the LDS / scratch level stack is the same for every
// sub-frame.  A loop, not an unroll: the kernel holds one copy of the trace.  After it the lane's pixel position is
// derived again from the lane id (as the bundle kernel does: nothing of it is kept live through the traces) and
// valid lanes store the round-half-up mean in the launch's format.
// Ray counts: each sub-frame's packed per-lane count (8 bits of reflected segments) is reduced over the wave on
// its own (wave_count: scalar results) and the wave's totals are carried in scalar registers, 64 bits each; lane 0
// adds them to the wave's counter slot once, after the loop.  Nothing is written to global memory inside the loop
// -- no store, no atomic: the scene, view and table reads of the next sub-frame then remain loads that nothing in
// the kernel has clobbered, which is what keeps them scalar loads (an atomic per sub-frame turned 83 of the direct
// kernel's 101 scalar loads into per-lane vector loads, and so did a volatile asm, which counts as a write).
// Hoisting: everything a trace derives from the launch parameters and the tile position alone is the same in every
// sub-frame, and the compiler would compute it once ahead of the loop and keep it in registers across every trace
// (measured: 75-81 VGPRs against PATH's 56-59 in the direct kernels, 6 waves per SIMD instead of 8, and VGPR spills
// to scratch under the bundle kernels' 64-VGPR cap).  So each sub-frame gets both through an empty asm tied to the
// loop counter -- the tile position, and the address of the launch parameters, which is the kernarg segment's own
// (every trace kernel has the one argument) -- and reads and derives what it needs inside the sub-frame, as the one
// trace of a PATH kernel does.  The asm emits no instruction.
// SS (SHUTTER_SS, rt_set_path_supersampling): a lane is a sample of the k W x k H frame and carries its own sample's
// sums across the loop, exactly as above; after it the k x k block sums of those sums go through resolve_tile's
// butterfly and the block's leader stores the single rounded mean of the m k^2 values (resolve_tile_sums).  The loop
// itself is the same code.
template <bool SS, typename F>
__device__ __forceinline__ void shutter_tile(const LaunchParams& p, int tile_x, int tile_y, F trace) {
    const int t = p.shutter_log2, m = 1 << t;
    const int rec0 = (int)(blockIdx.z << t);
    const bool counting = p.counters != nullptr;  // wave-uniform
    ResolveSum acc{0u, 0u};
    unsigned long long n_refl = 0, n_shadow = 0;  // the wave's totals (wave-uniform)
#pragma unroll 1
    for (int s = 0; s < m; ++s) {  // wave-uniform
        int tx = tile_x, ty = tile_y;
        asm("" : "+s"(tx), "+s"(ty) : "s"(s));
        const __attribute__((address_space(4))) LaunchParams* kp =
            (const __attribute__((address_space(4))) LaunchParams*)__builtin_amdgcn_kernarg_segment_ptr();
        asm("" : "+s"(kp) : "s"(s));
        const TileOut o = trace(*(const LaunchParams*)kp, rec0 | s, tx, ty);
        acc = resolve_add(acc, resolve_unpack(o.px32));
        if (counting) {
            n_refl += wave_count(o.cnt & CNT_REFL_MASK);
            n_shadow += wave_count(o.cnt >> CNT_SHADOW_SHIFT);
        }
    }
    const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const TilePixel q = tile_pixel<SS>(p, tile_x * TILE_W + (ln & 7), tile_y * TILE_H + (ln >> 3));
    if constexpr (SS) resolve_tile_sums(p, q.r, q.y, q.x, q.valid, acc, t);  // (converged: every lane is back)
    else if (q.valid) store_pixel(p, q.r, q.y, q.x, resolve_round_n(acc, t));
    if (counting && ln == 0) {
        unsigned long long* c = &p.counters[((blockIdx.y * gridDim.x + blockIdx.x) % COUNTER_SLOTS) * COUNTER_STRIDE];
        if (n_refl) atomicAdd(c + CNT_REFLECT, n_refl);
        if (n_shadow) atomicAdd(c + CNT_SHADOW, n_shadow);
    }
}

// ADAPT (rt_set_adaptive_sampling with supersampling on): the wave's tile is 8x8 output pixels, a lane is one of
// them, and `trace(p, pass, tile_x, tile_y)` traces sample pass = j k + i of every pixel's k x k block (sample_pixel),
// k = 1 << ss_log2.  Pass 0 is sample (0, 0), which is bit for bit the pixel of the frame without supersampling
// (DESIGN.md section 4), so the decision costs no trace of its own: after pass 0 the wave looks for two 4-adjacent
// valid pixels of the tile that differ by >= adapt_thr in a channel (rt_resolve.h adapt_differs) -- each lane
// against the lane at -1 (rx >= 1) and at -8 (ry >= 1), by DPP / bpermute as in encode_tile_fused, one ballot --
// and leaves the loop when there is none (a flat tile: the sum is pass 0's pixel itself).  Otherwise the remaining
// k^2 - 1 passes add to the running sums (16-bit fields: at most 64 samples) and the tile stores the round-half-up
// mean.  The valid lanes of a tile form a rectangle that starts at its lane 0 (x < W, r < local_rows and y < H are
// monotonic, and a tile never straddles a band: bands are multiples of 8 output rows or the launch has one), so
// a valid lane's neighbours at -1 and -8 are valid: the lane's own validity is the pair's.
// The loop obeys what shutter_tile found: no write to global memory inside it (ray counts reduced per pass into
// scalars, added once after it, the wave's extra samples with them), and the tile position and the kernarg address
// pass through the empty asm tied to the loop counter, so that nothing is hoisted and held across the traces.  It
// also carries as little as it can (see below): with the factor, the threshold, the pass count and the counting
// flag held in SGPRs across the traces the K <= 8 bundle kernels of class 0 spilled a VGPR to scratch.
// Counting follows add_counters: frame 0 of a batch (behind a copy slice) counts for all its frames.
// VIEWS (PATH_ADAPT, ANIM_ADAPT: rt_set_path_adaptive_sampling): every grid z is a frame with its own view (and scene),
// so its decision and its counts are its own -- each z adds its totals once after the loop, as a PATH launch counts
// (no copy slice in a views launch, no product with n_frames) -- and the threshold is LaunchParams::view_adapt.  The
// loop is the same code; the view and scene of frame z are read inside the trace from blockIdx.z, never from `pass`.
template <bool VIEWS, typename F>
__device__ __forceinline__ void adaptive_tile(const LaunchParams& p, int tile_x, int tile_y, F trace) {
    // Carried across a trace: the pass counter, the sums (two VGPRs) and the wave's ray totals (three SGPRs: at
    // most 64 lanes x 64 segments x 64 passes reflected segments fit 32 bits).  Everything else -- the factor, the
    // threshold, whether the wave counts -- is read again from the launch parameters where it is used, so that
    // nothing more competes with the trace for the 80 SGPRs; the loop ends at pass 0 on a flat tile, so s != 0
    // after it says "refined".
    ResolveSum acc{0u, 0u};
    unsigned n_refl = 0;
    unsigned long long n_shadow = 0;
    int s = 0;
#pragma unroll 1
    for (;; ++s) {  // wave-uniform
        int tx = tile_x, ty = tile_y;
        asm("" : "+s"(tx), "+s"(ty) : "s"(s));
        const __attribute__((address_space(4))) LaunchParams* kp =
            (const __attribute__((address_space(4))) LaunchParams*)__builtin_amdgcn_kernarg_segment_ptr();
        asm("" : "+s"(kp) : "s"(s));
        const LaunchParams& q = *(const LaunchParams*)kp;
        const TileOut o = trace(q, s, tx, ty);
        acc = resolve_add(acc, resolve_unpack(o.px32));
        if (q.counters != nullptr && (VIEWS || blockIdx.z == (unsigned)q.copy_z)) {  // wave-uniform
            n_refl += wave_count(o.cnt & CNT_REFL_MASK);
            n_shadow += wave_count(o.cnt >> CNT_SHADOW_SHIFT);
        }
        if (s == 0) {  // the decision, on the frame without supersampling
            const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            const bool valid = sample_pixel(q, tx, ty, ln, 0).valid;
            const int thr = VIEWS ? q.view_adapt : q.adapt_thr;
            const uint32_t v = o.px32 & 0xffffffu;
            const uint32_t left = row_shr<1>(v);                        // lane - 1: the same row for rx >= 1
            const uint32_t above = (uint32_t)__shfl_up((int)v, 8, 64);  // lane - 8: the row above
            const bool differs = valid && (((ln & 7) != 0 && adapt_differs(v, left, thr)) ||
                                           ((ln >> 3) != 0 && adapt_differs(v, above, thr)));
            if (__builtin_amdgcn_ballot_w64(differs) == 0) break;  // flat
        }
        if (s + 1 >= 1 << (2 * q.ss_log2)) break;
    }
    const int s2 = p.ss_log2;
    const bool refined = s != 0;
    const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const TilePixel t = sample_pixel(p, tile_x, tile_y, ln, 0);  // the pixel's sample (0, 0)
    if (t.valid)  // (output coordinates: r and y agree modulo k, bands are multiples of k sample rows)
        store_at(p, (size_t)((p.out_fmt == 2 ? t.y : t.r) >> s2) * (size_t)(p.W >> s2) + (size_t)(t.x >> s2),
                 resolve_round(acc, refined ? s2 : 0));
    if (p.counters != nullptr && (VIEWS || blockIdx.z == (unsigned)p.copy_z)) {  // wave-uniform
        // the samples beyond one per pixel: k^2 - 1 per valid pixel of a refined tile
        const unsigned long long n_extra = refined ? (unsigned long long)((1 << (2 * s2)) - 1) *
                                                         (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(t.valid))
                                                   : 0ull;
        if (ln == 0) {
            const unsigned long long nf = !VIEWS && p.n_frames > 1 ? (unsigned long long)p.n_frames : 1ull;
            unsigned long long* c = &p.counters[((blockIdx.y * gridDim.x + blockIdx.x) % COUNTER_SLOTS) * COUNTER_STRIDE];
            if (n_refl) atomicAdd(c + CNT_REFLECT, n_refl * nf);
            if (n_shadow) atomicAdd(c + CNT_SHADOW, n_shadow * nf);
            if (n_extra) atomicAdd(c + CNT_EXTRA_PRIMARY, n_extra * nf);
        }
    }
}

// SHUTTER_ADAPT, ANIM_SHUTTER_ADAPT (rt_set_shutter_adaptive_sampling): the wave's tile is 8x8 output pixels of output frame z
// = blockIdx.z, a lane is one of them, and the frame is the mean of m = 1 << shutter_log2 sub-frames at k x k samples
// each.  One loop over i = 0 .. m k^2 - 1 in pass-major order -- pass = i >> t, sub-frame s = i & (m - 1) -- calls
// `trace(p, pass << REC_BITS | rec, tile_x, tile_y)` with the view (and scene) record rec = z << t | s: the first m
// iterations are sample (0, 0) of every sub-frame, whose rounded mean P (resolve_round_n) is bit for bit the pixel of
// the shutter frame without supersampling.  After iteration m - 1 the wave decides on P exactly as adaptive_tile does
// on its pass 0 -- each valid lane against the lanes at -1 and -8, adapt_differs, one ballot -- and a flat tile leaves
// the loop and stores P.  A refined tile runs the remaining m (k^2 - 1) iterations into the same sums (16-bit fields:
// m k^2 <= RT_MAX_SHUTTER values) and stores the one rounded mean of all of them: never a mean of means.
// The loop obeys what shutter_tile and adaptive_tile found: no store and no atomic inside it, ray counts reduced per
// iteration into scalars and added once after it with the wave's extra samples, the tile position and the kernarg
// address passed through the empty asm tied to the loop counter, and nothing carried across a trace but the counter,
// the two sum VGPRs and the wave totals -- the shutter, the factor, the threshold and the counting flag are read again
// from the launch parameters where they are used.  The loop leaves at i = m - 1 on a flat tile, so i >= m after it
// says "refined".  Counting follows the views rule: every grid z counts for itself.
template <typename F>
__device__ __forceinline__ void shutter_adaptive_tile(const LaunchParams& p, int tile_x, int tile_y, F trace) {
    ResolveSum acc{0u, 0u};
    unsigned n_refl = 0;  // (at most 64 lanes x 255 segments x 256 iterations: 32 bits)
    unsigned long long n_shadow = 0;
    int i = 0;
#pragma unroll 1
    for (;; ++i) {  // wave-uniform
        int tx = tile_x, ty = tile_y;
        asm("" : "+s"(tx), "+s"(ty) : "s"(i));
        const __attribute__((address_space(4))) LaunchParams* kp =
            (const __attribute__((address_space(4))) LaunchParams*)__builtin_amdgcn_kernarg_segment_ptr();
        asm("" : "+s"(kp) : "s"(i));
        const LaunchParams& q = *(const LaunchParams*)kp;
        const int t = q.shutter_log2, m1 = (1 << t) - 1;
        const int rec = (int)(blockIdx.z << t) | (i & m1);
        const TileOut o = trace(q, (i >> t) << REC_BITS | rec, tx, ty);
        acc = resolve_add(acc, resolve_unpack(o.px32));
        if (q.counters != nullptr) {  // wave-uniform
            n_refl += wave_count(o.cnt & CNT_REFL_MASK);
            n_shadow += wave_count(o.cnt >> CNT_SHADOW_SHIFT);
        }
        if (i == m1) {  // the decision, on the shutter frame without supersampling
            const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            const bool valid = sample_pixel(q, tx, ty, ln, 0).valid;
            const uint32_t v = resolve_round_n(acc, t);
            const uint32_t left = row_shr<1>(v);                        // lane - 1: the same row for rx >= 1
            const uint32_t above = (uint32_t)__shfl_up((int)v, 8, 64);  // lane - 8: the row above
            const bool differs = valid && (((ln & 7) != 0 && adapt_differs(v, left, q.shutter_adapt)) ||
                                           ((ln >> 3) != 0 && adapt_differs(v, above, q.shutter_adapt)));
            if (__builtin_amdgcn_ballot_w64(differs) == 0) break;  // flat
        }
        if (i + 1 >= 1 << (t + 2 * q.ss_log2)) break;
    }
    const int s2 = p.ss_log2, t = p.shutter_log2;
    const bool refined = i >= 1 << t;
    const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const TilePixel px = sample_pixel(p, tile_x, tile_y, ln, 0);  // the pixel's sample (0, 0)
    if (px.valid)  // (output coordinates: r and y agree modulo k, bands are multiples of k sample rows)
        store_at(p, (size_t)((p.out_fmt == 2 ? px.y : px.r) >> s2) * (size_t)(p.W >> s2) + (size_t)(px.x >> s2),
                 resolve_round_n(acc, refined ? t + 2 * s2 : t));
    if (p.counters != nullptr) {  // wave-uniform
        // the samples beyond one per pixel and sub-frame: m (k^2 - 1) per valid pixel of a refined tile
        const unsigned long long n_extra = refined ? (unsigned long long)(((1 << (2 * s2)) - 1) << t) *
                                                         (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(px.valid))
                                                   : 0ull;
        if (ln == 0) {
            unsigned long long* c = &p.counters[((blockIdx.y * gridDim.x + blockIdx.x) % COUNTER_SLOTS) * COUNTER_STRIDE];
            if (n_refl) atomicAdd(c + CNT_REFLECT, (unsigned long long)n_refl);
            if (n_shadow) atomicAdd(c + CNT_SHADOW, n_shadow);
            if (n_extra) atomicAdd(c + CNT_EXTRA_PRIMARY, n_extra);
        }
    }
}

// PROG (rt_set_progressive, one Tick of a resting camera): the wave's tile is 8x8 output pixels and a lane is one of
// them, as in an ADAPT launch, and `trace(p, pass, tile_x, tile_y)` traces sample pass = j k + i of every pixel's
// k x k block.  The launch names 0, 1 or 2 samples (prog_n; their pass codes in prog_pass: the host knows the run's
// sample order, rt_progressive.h); the wave traces them one after the other, adds them to the pixel's running sums
// in LaunchParams::prog_acc -- the per-pixel accumulator that outlives the launch, 8 bytes of 16-bit fields -- and
// stores the rounded mean of all prog_first + prog_n samples so far (rt_resolve.h resolve_round_div).
// The loop obeys what shutter_tile and adaptive_tile found: no write to global memory inside it, ray counts reduced
// per sample into scalars and added once after it, the tile position and the kernarg address passed through the
// empty asm tied to the loop counter, and nothing but the counter, the sums and the wave's totals carried across a
// trace.  The accumulator is read after the traces, and only when the run has earlier samples (prog_first > 0: the
// launch that starts an accumulator never reads it), so its two VGPRs are not live across a trace; then one 8-byte
// store of the new sums (prog_n > 0) and one pixel store.  With prog_n = 0 the wave only loads, rounds and stores:
// the converged Tick's frame, by the same kernel.
// Counting follows add_counters for a one-view launch: the frame behind a copy slice counts, when the context counts.
template <typename F>
__device__ __forceinline__ void progressive_tile(const LaunchParams& p, int tile_x, int tile_y, F trace) {
    ResolveSum acc{0u, 0u};
    unsigned n_refl = 0;
    unsigned long long n_shadow = 0;
#pragma unroll 1
    for (int s = 0;; ++s) {  // wave-uniform
        int tx = tile_x, ty = tile_y;
        asm("" : "+s"(tx), "+s"(ty) : "s"(s));
        const __attribute__((address_space(4))) LaunchParams* kp =
            (const __attribute__((address_space(4))) LaunchParams*)__builtin_amdgcn_kernarg_segment_ptr();
        asm("" : "+s"(kp) : "s"(s));
        const LaunchParams& q = *(const LaunchParams*)kp;
        if (s >= q.prog_n) break;
        const TileOut o = trace(q, q.prog_pass[s], tx, ty);
        acc = resolve_add(acc, resolve_unpack(o.px32));
        if (q.counters != nullptr && blockIdx.z == (unsigned)q.copy_z) {  // wave-uniform
            n_refl += wave_count(o.cnt & CNT_REFL_MASK);
            n_shadow += wave_count(o.cnt >> CNT_SHADOW_SHIFT);
        }
    }
    const int s2 = p.ss_log2;
    const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const TilePixel t = sample_pixel(p, tile_x, tile_y, ln, 0);  // the pixel's sample (0, 0): validity and rows
    if (t.valid) {  // (output coordinates: r and y agree modulo k, bands are multiples of k sample rows)
        const size_t wo = (size_t)(p.W >> s2), xo = (size_t)(t.x >> s2);
        uint2* a = (uint2*)(p.prog_acc + ((size_t)(t.r >> s2) * wo + xo));  // (ResolveSum: 8 bytes, 8-byte aligned slots)
        if (p.prog_first > 0) {  // wave-uniform
            const uint2 before = *a;
            acc = resolve_add(acc, ResolveSum{before.x, before.y});
        }
        if (p.prog_n > 0) *a = make_uint2(acc.rb, acc.g);
        store_at(p, (size_t)((p.out_fmt == 2 ? t.y : t.r) >> s2) * wo + xo, resolve_round_div(acc, p.prog_first + p.prog_n));
    }
    if (p.counters != nullptr && blockIdx.z == (unsigned)p.copy_z && ln == 0) {
        unsigned long long* c = &p.counters[((blockIdx.y * gridDim.x + blockIdx.x) % COUNTER_SLOTS) * COUNTER_STRIDE];
        if (n_refl) atomicAdd(c + CNT_REFLECT, (unsigned long long)n_refl);
        if (n_shadow) atomicAdd(c + CNT_SHADOW, n_shadow);
    }
}

// DIRECT kernel (scenes with < CULL_MIN_SPHERES spheres).
// STATS: the diagnostic build that also tallies the work actually executed (not timed).
// TILES: out_fmt OUT_TILES (the fused encoder: its own instantiation, so that the others keep their
// register budget -- the epilogue alone raises the direct kernel's SGPR peak from 79 to 83).
// WPG: waves (8x8 tiles of a tile row) per workgroup -- 1 for batch launches; SINGLE_WPG for
// single-frame launches without a copy slice (fewer, larger workgroups: the dispatcher launches
// one-wave groups no faster than ~6.9 us per 1080p frame, a floor a lone frame's launch pays in
// full, tools/launch_probe.hip).  Each wave has its own LDS stack slice.
// TORD (single-frame launches, WPG > 1): 0 = tile rows in row_order / col_major order, 1 = the measured tile
// order (tile_order, a 1-D grid), 2 = as 0 and every wave records its duration (tile_cost).  Instantiations of
// their own: the order read and the recording, compiled into the common kernel even when unused, cost a
// one-frame launch 2 % and 10 % (C2 19.9 -> 20.3 / 22.4 us, profiles/ab/r05_tile_order.txt).
// SS: the supersampling epilogue (resolve_tile) in place of the pixel stores.  PATH: frame z of the grid takes its
// view from LaunchParams::views (one DevView per grid z).  SHUTTER: a PATH launch whose waves trace 1 <<
// shutter_log2 views per grid z and store their mean (shutter_tile).  ADAPT: supersampling whose waves decide per
// 8x8 output tile whether to trace more than one sample per pixel (adaptive_tile).  PROG: a progressive Tick, whose
// waves add 0-2 samples per output pixel to the run's accumulator (progressive_tile).  ANIM: a PATH launch whose
// frame z also reads its own scene image, LaunchParams::scene_stride bytes behind frame z - 1's (SceneOf).  PATH_SS,
// SHUTTER_SS, ANIM_SS: PATH, SHUTTER and ANIM launches on the k W x k H sample frame (LaunchParams::view_ss) -- the
// twin's view and scene reads with SS's tile mapping and epilogue, which the tile traces take from the word
// independently (view_of, ss_of); SHUTTER_SS resolves the blocks of the lanes' sub-frame sums.  PATH_ADAPT,
// ANIM_ADAPT: PATH_SS and ANIM_SS launches whose waves decide per output tile as ADAPT's do (adapt_of).  ANIM_SHUTTER,
// ANIM_SHUTTER_SS: SHUTTER and SHUTTER_SS launches whose sub-frame rec also reads its own scene image, rec * scene_stride
// bytes behind the launch's (LaunchParams::scene_shutter; the same shutter_tile, the record index reaching SceneOf as it
// reaches ViewOf).  SHUTTER_ADAPT, ANIM_SHUTTER_ADAPT: SHUTTER_SS and ANIM_SHUTTER_SS launches whose waves decide per output
// tile on the mean of the sub-frames (LaunchParams::shutter_adapt, shutter_adaptive_tile).  All fifteen of the plain batch
// variants only (no STATS, no TILES, WPG 1, TORD 0: rt_internal.h trace_variant_built).
// The options arrive as one variant word V (rt_internal.h VF_*, vf_cls = SMAX) and are read from it by name.
template <int K, unsigned V>
__device__ __forceinline__ void direct_kernel_body(const LaunchParams& p) {
    constexpr bool STATS = (V & VF_STATS) != 0, SHUTTER = shutter_of(V);
    constexpr int PATH = view_of(V);
    constexpr int SMAX = vf_cls_of(V), WPG = vf_wpg_of(V), TORD = vf_tord_of(V);
    constexpr int LDS_LEVELS = StackFor<K>::lds_levels;  // LdsStack slots, else unused
    __shared__ float2 stk_lv[LDS_LEVELS > 0 ? LDS_LEVELS * WG_THREADS * WPG : 1];
    __shared__ float stk_dv[LDS_LEVELS > 0 ? 3 * WG_THREADS * WPG : 1];
    if (WPG == 1 && blockIdx.z < (unsigned)p.copy_z) {  // wave-uniform: the fused hand-off's copy slice
        copy_slice(p);
        return;
    }
    Tally<STATS, SMAX> tl;
    const int wave = WPG > 1 && TORD != 0 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))
                     : WPG > 1                ? (int)(threadIdx.x >> 6)
                                              : 0;
    float2* lv = stk_lv + (LDS_LEVELS > 0 ? wave * LDS_LEVELS * WG_THREADS : 0);
    float* dv = stk_dv + (LDS_LEVELS > 0 ? wave * 3 * WG_THREADS : 0);
    // single-frame launches: tile rows in the host's cost order (LaunchParams::row_order), optionally
    // with the rows varying fastest in dispatch order (col_major: grid x = tile rows), or any tile order
    // the host measured (tile_order: a 1-D grid, entry ty << 16 | tx)
    const bool cm = WPG > 1 && p.col_major;
    const int gx = cm ? (int)blockIdx.y : (int)blockIdx.x, gy = cm ? (int)blockIdx.x : (int)blockIdx.y;
    int tile_x = gx * WPG + wave, tile_y = WPG > 1 && gy < p.row_order_n ? (int)p.row_order[gy] : gy;
    if constexpr (TORD == 1) {
        const uint32_t t = p.tile_order[blockIdx.x * WPG + wave];
        tile_x = (int)(t & 0xffffu), tile_y = (int)(t >> 16);  // (0xffff: past the frame, no pixel valid)
    }
    // the host measuring tile costs (order_pick): the wave's cost slot (null when not measuring) and start
    // time wait in LDS -- nothing of it lives in registers across the trace (there it spilled: +9 VGPRs)
    struct TileRec {
        unsigned* slot;
        unsigned t0;
    };
    __shared__ TileRec t_rec[TORD == 2 ? WPG : 1];
    if (TORD == 2 && (threadIdx.x & 63) == 0) {
        const unsigned tiles_x = (unsigned)(p.W + TILE_W - 1) / TILE_W, tiles_y = (unsigned)(p.H + TILE_H - 1) / TILE_H;
        const bool in = p.tile_cost != nullptr && (unsigned)tile_x < tiles_x && (unsigned)tile_y < tiles_y;
        t_rec[wave] = TileRec{in ? p.tile_cost + ((unsigned)tile_y * tiles_x + (unsigned)tile_x) : nullptr,
                              in ? (unsigned)__builtin_amdgcn_s_memrealtime() : 0u};
    }
    if constexpr (shutter_adapt_of(V)) {
        shutter_adaptive_tile(p, tile_x, tile_y, [&](const LaunchParams& q, int recp, int tx, int ty) { return trace_tile_direct<K, V & VF_TILE>(q, tx, ty, lv, dv, tl, recp); });
        return;
    }
    if constexpr (SHUTTER) {
        shutter_tile<ss_of(V)>(p, tile_x, tile_y, [&](const LaunchParams& q, int rec, int tx, int ty) { return trace_tile_direct<K, V & VF_TILE>(q, tx, ty, lv, dv, tl, rec); });
        return;
    }
    if constexpr (adapt_of(V)) {
        adaptive_tile<PATH != VIEW_ARGS>(p, tile_x, tile_y, [&](const LaunchParams& q, int pass, int tx, int ty) { return trace_tile_direct<K, V & VF_TILE>(q, tx, ty, lv, dv, tl, pass); });
        return;
    }
    if constexpr ((V & VF_PROG) != 0) {  // (a sample is traced as ADAPT's passes are: the tile trace of that word)
        progressive_tile(p, tile_x, tile_y, [&](const LaunchParams& q, int pass, int tx, int ty) { return trace_tile_direct<K, ((V & VF_TILE) & ~VF_PROG) | VF_ADAPT>(q, tx, ty, lv, dv, tl, pass); });
        return;
    }
    // (the launches that record tile durations, TORD 2, run below 8 waves per SIMD already and would lose another step
    // to the plane-uniform path: they trace without it)
    const unsigned cnt = trace_tile_direct<K, V & VF_TILE, TORD != 2>(p, tile_x, tile_y, lv, dv, tl).cnt;
    add_counters<STATS, PATH>(p, threadIdx.x & 63, cnt & CNT_REFL_MASK, cnt >> CNT_SHADOW_SHIFT, tl);
    if (TORD == 2 && (threadIdx.x & 63) == 0) {
        const TileRec r = t_rec[threadIdx.x >> 6];
        if (r.slot != nullptr) *r.slot = (unsigned)__builtin_amdgcn_s_memrealtime() - r.t0;
    }
}
// amdgpu_num_sgpr(80): 8 waves per SIMD need at most 80 SGPRs (the shadow pre-test's records would take the
// scan to 87, i.e. 7 waves; capped, the allocator spills 4 to VGPR lanes: C3 24.9 -> 24.1 us, C2 15.7 -> 15.2 us,
// profiles/ab/r06_direct_shadow_pre.txt).
template <int K, unsigned V>
__global__ __launch_bounds__(WG_THREADS * vf_wpg_of(V)) __attribute__((amdgpu_num_sgpr(80))) void trace_direct_kernel(LaunchParams p) {
    static_assert(!(V & VF_GPOW), "GPOW variants run trace_direct_kernel_gpow");
    direct_kernel_body<K, V>(p);
}
// Scenes with a general specular exponent (glibc's pow on the device): ~100 VGPRs, 4-5 waves per SIMD whatever
// the SGPRs, so no cap (under it the allocator spilled 24-34 SGPRs to VGPR lanes for nothing).  An entry point of
// its own because the attribute takes no template-dependent value.
template <int K, unsigned V>
__global__ __launch_bounds__(WG_THREADS * vf_wpg_of(V)) void trace_direct_kernel_gpow(LaunchParams p) {
    static_assert((V & VF_GPOW) != 0, "variants without GPOW run trace_direct_kernel");
    direct_kernel_body<K, V>(p);
}

// ---------------------------------------------------------------------------------
// Wave-level ray bundles and conservative sphere culling.
//
// A wave's active rays (origins o_l, directions d_l) are bounded by a reference origin O,
// an origin radius R >= max |o_l - O|, a unit axis A and a direction spread
// delta >= max |d_l/|d_l| - A|.  Lane i tests sphere i against the bundle and a ballot
// gives the wave's candidate mask; the exact per-lane tests then visit only candidates,
// in ascending sphere index (so the reference's tie rules are untouched).
//
// Exactness: a sphere is culled only when, for EVERY lane, the binary32 evaluation of
// IntersectsSphere provably yields disc < 0 or b >= 0 -- both make the reference's
// distance non-selectable (root_t1).  With u = o - C and a = d.d, a first-order error
// analysis of disc = fl(fl(b*b) - fl(fl(4a)*fl(fl(u.u) - r^2))) bounds its error by
// 4a(14 eps |u|^2 + 4 eps r^2) (eps = 2^-24), so disc < 0 whenever the exact
// line-to-centre distance D satisfies D >= r (1 + 3 eps) + 9.2e-4 |u|; b >= 0 whenever
// u.d/|d| >= 4 eps |u|.  The cull demands D >= r (1 + 2^-8) + 2^-8 (|C - O| + R) and
// u.A >= 2^-8 (|C - O| + R) after subtracting the bundle slack (R, delta terms) --
// a 4x margin over the analysis, far above the rounding of the cull arithmetic itself.
// Culling is disabled for a wave when any active lane has a = d.d outside [0.5, 2]
// (trace rays) or the light's a outside [2^-40, 2^40] (shadow rays), or for spheres
// with r^2 < 2^-100 or |C - O| outside [2^-30, 2^40] (no underflow/overflow).
// ---------------------------------------------------------------------------------
struct Bundle {
    f3 O, A;
    float R, delta;
    bool ok;   // culling allowed
    bool any;  // some lane active
};

__device__ __forceinline__ float readlane_f(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ f3 readlane3(f3 v, int lane) {
    return mk(readlane_f(v.x, lane), readlane_f(v.y, lane), readlane_f(v.z, lane));
}
// Wave-uniform maximum of a non-negative float (all 64 lanes active): DPP row rotations
// give each 16-lane row its maximum, four readlanes and integer max (bit patterns of
// non-negative floats order like the floats; a NaN pattern compares above +inf) finish it.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_f<0x121>(v));  // row_ror:1
    v = fmaxf(v, dpp_f<0x122>(v));  // row_ror:2
    v = fmaxf(v, dpp_f<0x124>(v));  // row_ror:4
    v = fmaxf(v, dpp_f<0x128>(v));  // row_ror:8
    const unsigned a = (unsigned)__builtin_amdgcn_readlane(__float_as_int(v), 0);
    const unsigned b = (unsigned)__builtin_amdgcn_readlane(__float_as_int(v), 16);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane(__float_as_int(v), 32);
    const unsigned d = (unsigned)__builtin_amdgcn_readlane(__float_as_int(v), 48);
    return __uint_as_float(max(max(a, b), max(c, d)));
}
// Culling-only arithmetic (never feeds a result): hardware sqrt / rsq (about 1 ulp) instead of
// the correctly rounded sequences; the cull margins (2^-10 relative on R and delta, 2^-8 on
// the tests) are orders of magnitude above that error.
__device__ __forceinline__ float clen3(f3 v) { return __builtin_amdgcn_sqrtf(dot(v, v)); }
__device__ __forceinline__ f3 cnormalize(f3 v) { return scale(v, __builtin_amdgcn_rsqf(dot(v, v))); }
__device__ __forceinline__ f3 cross3(f3 l, f3 r) {
    return mk(l.y * r.z - l.z * r.y, l.z * r.x - l.x * r.z, l.x * r.y - l.y * r.x);
}

// Converged call (all 64 lanes).  `dir_uniform`: every lane's direction is `d` itself
// (shadow rays: the light position), so delta = 0.
__device__ __forceinline__ Bundle make_bundle(f3 o, f3 d, bool active, bool dir_uniform) {
    Bundle B;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(active);
    B.any = m != 0;
    if (m == 0) {
        B.ok = false;
        B.O = o;
        B.A = d;
        B.R = B.delta = 0.0f;
        return B;
    }
    const int ref = __builtin_ctzll(m);
    {  // midway between the first and the last active lane's origins (see make_shadow_sphere)
        const f3 a = readlane3(o, ref), b = readlane3(o, 63 - __builtin_clzll(m));
        B.O = scale(add(a, b), 0.5f);
    }
    const f3 dref = readlane3(d, ref);
    B.A = cnormalize(dref);
    float e = 0.0f, f = 0.0f;
    bool bad = false;
    if (active) {
        e = clen3(sub(o, B.O));
        bad = !(e < 0x1p40f);  // also NaN / inf origins
        if (!dir_uniform) {
            const float a = dot(d, d);
            f = clen3(sub(cnormalize(d), B.A));
            bad = bad || !(a >= 0.5f && a <= 2.0f) || !(f < 2.0f);
        }
    }
    const float R = wave_max(e);
    const float delta = dir_uniform ? 0.0f : wave_max(f);
    bad = __builtin_amdgcn_ballot_w64(bad) != 0;
    B.R = R * (1.0f + 0x1p-10f) + 0x1p-60f;
    B.delta = dir_uniform ? 0.0f : delta * (1.0f + 0x1p-10f) + 0x1p-20f;
    B.ok = !bad && R < 0x1p40f && B.delta < 0.5f;
    return B;
}

// Candidate mask of spheres [base, base+n) (n <= 64) for bundle B.  Converged call.
template <int PATH>
__device__ __forceinline__ unsigned long long cull_mask(const LaunchParams& p, const Bundle& B, int base, int n, int rec) {
    // branch-free (no exec-mask bookkeeping on the scalar unit): every lane loads and tests, lanes
    // >= n are dropped from the ballot; a sphere is culled only when the bundle allows culling,
    // its record is in range and one of the rules holds (NaN anywhere -> candidate)
    const int lane = threadIdx.x & 63;
    const bool in = lane < n;
    const DevSphereCull s = SceneOf<PATH>::scull(p, rec)[base + (in ? lane : 0)];
    const f3 w = sub(mk(s.cx, s.cy, s.cz), B.O);
    const float dc = clen3(w) * (1.0f + 0x1p-20f);
    const float mgn = 0x1p-8f * (dc + B.R);
    const float x = clen3(cross3(w, B.A));
    const bool line = (x - dc * B.delta - B.R) > s.rr + mgn;
    const bool behind = (-dot(w, B.A) - dc * B.delta - B.R * (1.0f + B.delta)) > mgn;
    const bool valid = s.rr >= 0x1p-50f && dc >= 0x1p-30f && dc < 0x1p40f;
    const bool cull = B.ok && valid && (line || behind);
    return __builtin_amdgcn_ballot_w64(in && !cull);
}

// Per-lane cluster pre-cull (p.n_clus > 0) for a trace bundle that allows no culling -- the reflected segments
// deep in mirror chains, where a wave's rays fan out into a cone of 0.5 or wider and the bundle would test
// every sphere (tools/trace_cull_model.py: such bundles hold 6.6 of the 7.3 sphere candidates a C4 wave tests
// on its reflected segments, while 1-3 spheres are reachable).  Each lane tests its own ray against the
// clusters' bounding spheres (DevCluster: R >= |c_i - Cc| + r'_i for every member) and the wave takes the
// union of the kept clusters' members.  Converged call (idle lanes carry a copy of an active lane's ray).
// Exactness (culling only, FMA allowed): cull_mask's rules for one ray (R = 0, delta = 0) applied to the
// bounding sphere -- the line misses it by the margin 2^-8 (|w|_1 + R), w = Cc - o, or its centre lies behind
// the origin by R plus that margin.  Then for every member i the line-to-centre distance exceeds
// r'_i + 2^-8 (|c_i - o| + 0) (|c_i - o| <= |w| + R) or its centre is behind by more than the margin: the
// conditions under which cull_mask drops sphere i for this lane, which make its IntersectsSphere distance
// non-selectable.  The perpendicular distance is |w x A| (no cancellation), A = d / |d| by the hardware rsq
// (~1 ulp, far inside the margin); the products are fused (culling-only arithmetic: fewer roundings).  A lane whose a = d.d is outside [0.5, 2] or whose origin is not finite
// keeps every cluster, and a cluster with a NaN R (a member without a usable cull record) is never culled.
template <int PATH>
__device__ __forceinline__ unsigned long long cluster_mask(const LaunchParams& p, f3 o, f3 d, int rec) {
    const float a = dot(d, d);
    const f3 A = cnormalize(d);
    const float ol = __builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z);
    const bool ok = a >= 0.5f && a <= 2.0f && ol < 0x1p40f;
    unsigned long long m = 0;
    for (int j = 0; j < p.n_clus; ++j) {  // wave-uniform
        const DevCluster c = SceneOf<PATH>::clus(p, rec)[j];
        const f3 w = sub(mk(c.cx, c.cy, c.cz), o);
        const float dc = (__builtin_fabsf(w.x) + __builtin_fabsf(w.y) + __builtin_fabsf(w.z)) * (1.0f + 0x1p-20f);
        const float mgn = 0x1p-8f * (dc + c.R);
        const f3 x = mk(__builtin_fmaf(w.y, A.z, -(w.z * A.y)), __builtin_fmaf(w.z, A.x, -(w.x * A.z)),
                        __builtin_fmaf(w.x, A.y, -(w.y * A.x)));  // w x A
        const float T = c.R + mgn;
        const bool line = __builtin_fmaf(x.z, x.z, __builtin_fmaf(x.y, x.y, x.x * x.x)) > T * T;
        const bool behind = -__builtin_fmaf(w.z, A.z, __builtin_fmaf(w.y, A.y, w.x * A.x)) - c.R > mgn;
        const bool valid = dc >= 0x1p-30f && dc < 0x1p40f;
        if (__builtin_amdgcn_ballot_w64(!(ok && valid && (line || behind))) != 0) m |= c.members;  // NaN: kept
    }
    return m;
}

// Shadow bundles.  Every shadow ray of light l has the same direction p_l (the light
// POSITION, Q2), so a sphere can block lane k only if the line {hp_k + s p_l} passes within
// r of its centre: a 2-D test in the light's frame (U, V, A ~ p_l/|p_l|, host-built).  One bound
// serves every light of a shaded level: the ball (O, R) around the first diffuse lane's hit
// point that holds every diffuse lane's hit point, so the hit points spread by at most R across
// and along any light's axis.  Cull rules (same error analysis and 2^-8 margin as cull_mask,
// |C - O| bounded by the L1 norm of the frame coordinates): line miss if |w_perp| - R > r' + mgn;
// behind (b >= 0 for every lane) if -w_A - R > mgn, where w = C - O.  Per light the work is the
// projection of O (uniform) and the cull itself, with the sphere centres already in each light's
// frame (DevShadowCull, host-built in double; the rounding of those projections and of O's is
// covered by the 2^-18 (|C| + |O|) allowance, far above their 2^-22 (|C| + |O|) error).  Against
// a bound per light from its exact perpendicular / axial spreads (three wave reductions per
// light): C4 -2.6 %, C5 -7.5 % (profiles/ab/r02_shadow_sphere.txt).
struct ShadowSphere {
    f3 O;
    float R, omgn;  // radius (rounded up) and 2^-18 |O|
    bool ok;
};

__device__ __forceinline__ ShadowSphere make_shadow_sphere(f3 hp, bool active) {
    ShadowSphere S;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(active);
    S.ok = false;
    S.R = 0.0f;
    S.omgn = 0.0f;
    S.O = hp;
    if (m == 0) return S;
    {
        // centre: midway between the first and the last active lane's hit points (lanes 0 and 63
        // are opposite corners of the 8x8 tile), which roughly halves R against either of them
        // (C4 -4.3 %, C5 -3.8 %, profiles/ab/r02_bundle_centre.txt); R is measured from it
        const f3 a = readlane3(hp, __builtin_ctzll(m)), b = readlane3(hp, 63 - __builtin_clzll(m));
        S.O = scale(add(a, b), 0.5f);
    }
    float e = 0.0f;
    bool bad = false;
    if (active) {
        e = clen3(sub(hp, S.O));
        bad = !(e < 0x1p40f);  // also NaN / inf
    }
    bad = __builtin_amdgcn_ballot_w64(bad) != 0;
    S.R = wave_max(e) * (1.0f + 0x1p-10f) + 0x1p-60f;
    const float olen = clen3(S.O);
    S.omgn = 0x1p-18f * olen * (1.0f + 0x1p-10f);
    S.ok = !bad && S.R < 0x1p38f && olen < 0x1p40f;
    return S;
}

// Candidate mask of spheres [base, base+n) (n <= 64) for the shadow rays of light li from the
// ball S.  Converged call.
template <int PATH>
__device__ __forceinline__ unsigned long long shadow_sphere_cull(const LaunchParams& p, const ShadowSphere& S,
                                                                 const DevLight& l, int li, int base, int n, int rec) {
    const int lane = threadIdx.x & 63;
    const bool in = lane < n;
    const bool ok = S.ok && SceneOf<PATH>::shcull(p, rec) != nullptr && l.a >= 0x1p-40f && l.a <= 0x1p40f && l.a2 < __builtin_inff();
    if (!ok) return __builtin_amdgcn_ballot_w64(in);  // (uniform) no culling: every sphere is a candidate
    // O in the light's frame (uniform); branch-free per lane, as cull_mask
    const float ou = dot(S.O, mk(l.ux, l.uy, l.uz)), ov = dot(S.O, mk(l.vx, l.vy, l.vz));
    const float oa = dot(S.O, mk(l.ax, l.ay, l.az));
    const DevShadowCull c = SceneOf<PATH>::shcull(p, rec)[(size_t)li * (size_t)p.S + (size_t)(base + (in ? lane : 0))];
    const float wu = c.cu - ou, wv = c.cv - ov, wa = c.ca - oa;
    const float dc = __builtin_fabsf(wu) + __builtin_fabsf(wv) + __builtin_fabsf(wa);  // >= |C - O|
    const float mgn = 0x1p-8f * (dc + 3.0f * S.R) + S.omgn;
    const float T = S.R + c.rr + mgn;
    const bool line = wu * wu + wv * wv > T * T;
    const bool behind = -wa - S.R > mgn;
    const bool valid = c.rr >= 0x1p-50f && dc >= 0x1p-30f && dc < 0x1p40f;
    return __builtin_amdgcn_ballot_w64(in && !(valid && (line || behind)));  // NaN anywhere -> candidate
}

// Exact tests of the candidate spheres m (bits relative to `base`) of one bundle segment, in
// ascending order (the reference's tie rules), for every lane (idle lanes trace a copy of an active
// lane's ray).  A2OK: 2a finite-positive on every lane.
template <bool PRIMARY, bool A2OK, int PATH, typename T>
__device__ __forceinline__ void bundle_candidates(const LaunchParams& p, unsigned long long m, int base, f3 o, f3 d,
                                                  float a2, float a4, bool a2_ok, bool active, float& best_s,
                                                  int& win_s, T& tl, int rec) {
    auto test = [&](int i) -> float {
        if (PRIMARY && ViewOf<PATH>{p, rec}.prim_const()) {
            // o == camera: oc = cam - c and c = oc.oc - r^2 are per-frame constants (:614-619)
            const PrimConst pc = ViewOf<PATH>{p, rec}.pc()[i];
            const float b = 2.0f * dot(mk(pc.ocx, pc.ocy, pc.ocz), d);
            const float disc = b * b - a4 * pc.c;
            return A2OK ? root_t1(b, disc, a2) : (a2_ok ? root_t1(b, disc, a2) : root_full(b, disc, a2));
        }
        return sphere_t<A2OK>(o, d, a2, a4, a2_ok, SceneOf<PATH>::sph(p, rec)[i]);
    };
    auto take = [&](float t, int i) {
        if (PRIMARY) take_primary(t, i, best_s, win_s);
        else take_secondary(t, i, best_s, win_s);
    };
    // two candidates per iteration: independent sqrt chains (ILP), selections in ascending order;
    // an odd last candidate alone (C4 -0.9 %, C5 -1.2 %; testing it twice instead: -0.5 / -0.7 %,
    // profiles/ab/r02_near_pairs.txt)
    while (m) {
        const int i0 = base + (int)__builtin_ctzll(m);
        m &= m - 1;
        if (m) {
            const int i1 = base + (int)__builtin_ctzll(m);
            m &= m - 1;
            tl.sphere(active);
            tl.sphere(active);
            const float t0 = test(i0), t1 = test(i1);
            take(t0, i0);
            take(t1, i1);
        } else {
            tl.sphere(active);
            take(test(i0), i0);
        }
    }
}

// BUNDLE path.  Nearest hit of one segment for every active lane (converged call).  PRIMARY: TracePixel's
// rule (:977, :987, :993) with the per-frame camera-relative constants; otherwise
// TraceSecondaryRay's asymmetric rule (:804-806, :819-821, :825).
// `planes`: the segment's nearest plane hit when the caller already has it (terminal segments).
template <bool PRIMARY, int PATH, typename T>
__device__ __forceinline__ Hit nearest_bundle(const LaunchParams& p, f3 o, f3 d, bool active, T& tl,
                                              unsigned long long pmask, const Hit* planes, int rec) {
    const unsigned long long am = __builtin_amdgcn_ballot_w64(active);
    if (am == 0) return Hit{0.0f, HIT_NONE};
    // primary segment: the per-frame screen boxes replace the bundle cull
    const bool use_box = PRIMARY && ViewOf<PATH>{p, rec}.prim_const();
    Bundle B{};
    if (!use_box) B = make_bundle(o, d, active, false);
    if (am != ~0ull) {  // idle lanes trace an exact copy of the first active lane's ray, so
        const int ref = __builtin_ctzll(am);  // they never add divergence (results ignored)
        const f3 ro = readlane3(o, ref), rd = readlane3(d, ref);
        if (!active) {
            o = ro;
            d = rd;
        }
    }
    const float a = dot(d, d);
    const float a2 = 2.0f * a, a4 = 4.0f * a;
    const bool a2_ok = a2 > 0.0f && a2 < __builtin_inff();
    float best_s = __builtin_inff();
    int win_s = -1;
    for (int base = 0; base < p.S; base += 64) {
        const int n = min(64, p.S - base);
        // use_box: S <= 64.  A bundle that allows no culling (cone of 0.5 or wider, far or non-finite
        // origins) takes every sphere without the per-lane cull arithmetic, whose ballot would keep every
        // sphere anyway (C4 -0.7 %, C5 -0.6 %, profiles/ab/r04_nocull_ab.txt; culling wider cones than 0.25
        // less eagerly measured +2 %).  Wave-uniform.
        // A cone too wide for the bundle cull: the per-lane cluster pre-cull when the scene has clusters (S <= 64).
        const unsigned long long all = n == 64 ? ~0ull : (1ull << n) - 1ull;
        unsigned long long m = use_box ? pmask : B.ok ? cull_mask<PATH>(p, B, base, n, rec) : p.n_clus ? cluster_mask<PATH>(p, o, d, rec) & all : all;
        // candidates in ascending order, selection by selects (take_*, no per-lane branches); the
        // root sequence is chosen once per wave (2a finite-positive on every lane: the usual case)
        if (__builtin_amdgcn_ballot_w64(!a2_ok) == 0)
            bundle_candidates<PRIMARY, true, PATH>(p, m, base, o, d, a2, a4, a2_ok, active, best_s, win_s, tl, rec);
        else
            bundle_candidates<PRIMARY, false, PATH>(p, m, base, o, d, a2, a4, a2_ok, active, best_s, win_s, tl, rec);
    }
    float best_p = __builtin_inff();
    int win_p = -1;
    if (planes) {
        best_p = planes->t;
        win_p = planes->prim;
    } else {
        for (int i = 0; i < p.P; ++i) {
            tl.plane(active);
            plane_take(o, d, SceneOf<PATH>::pl(p, rec)[i], i, best_p, win_p);  // t > 0 && t < best
        }
    }
    if (!active) return Hit{0.0f, HIT_NONE};
    if (best_s < best_p) return Hit{best_s, win_s};
    if (win_p >= 0) return Hit{best_p, ~win_p};
    return Hit{0.0f, HIT_NONE};
}

// Merged shadow pass of one shaded level (bundle kernel, S <= 64 spheres, L <= SHADOW_MERGE_L
// lights): every light's shadow rays of the wave in ONE wave-uniform loop over the union of the
// lights' candidate sets (they share the level's ShadowSphere bound, and the sets overlap: on C4
// the union holds ~1/3 of the per-light sum, profiles/r03_shadow_slots.txt).  Per candidate sphere
// oc = hp - c and c = oc.oc - r^2 are shared by the lights; b, disc and the root test are per light,
// for the lights whose candidate set holds the sphere and which still have a pending lane (both
// wave-uniform).  Operations and their order are exactly shadow_blocked's (:613-642 with
// IntersectShadowLight's :574-578), so every outcome is the same bit.  Returns the lane's blocked
// bits (bit li).  `want` (bit li): the lane's ray toward light li must be resolved -- a superset of
// the shading's `need` (shade_bundle), so every needed outcome is computed.
// Candidate sets of the lights as one register: lane i holds bit li when sphere i is a candidate
// for light li (lights some lane wants only).  Converged call.  (Hoisting the light-independent
// terms of the cull out of the light loop cut VALU 1.8 % but spilled 12 B/lane: C4 +0.8 %, C5 +0.8 %,
// profiles/ab/r03_shadow_queue_rejected.txt.)
// Candidate sets of the lights from the level's ball bound, with the light-independent terms hoisted
// out of the light loop (the merged instantiation, whose register budget has room for them; against
// one shadow_sphere_cull per light: C4 -2.6 %, profiles/ab/r04_fast_members_ab.txt): lane i loads sphere
// i's centre and r' once, w = C - O, the world-frame L1 bound dc >= |C - O| and the threshold T of
// the line rule once, and per light only projects w onto (U, V, A) -- FMA allowed, culling only --
// and applies the same two rules: line miss if |w_perp|^2 > T^2, behind if w.A < -(R + mgn).  The
// margins are shadow_sphere_cull's: 2^-8 (dc + 3R) with dc from the unprojected w, plus 2^-18
// (|O| + |C|_1) for the rounding of w and of its projections (each < 2^-21 |w|_1, far inside).
template <int PATH>
__device__ __forceinline__ unsigned shadow_members_fast(const LaunchParams& p, const ShadowSphere& SS, unsigned want, int rec) {
    const int lane = threadIdx.x & 63;
    const bool in = lane < p.S;
    const DevSphereCull c = SceneOf<PATH>::scull(p, rec)[in ? lane : 0];
    const f3 w = sub(mk(c.cx, c.cy, c.cz), SS.O);
    const float dc = (__builtin_fabsf(w.x) + __builtin_fabsf(w.y) + __builtin_fabsf(w.z)) * (1.0f + 0x1p-20f);
    const float c1 = __builtin_fabsf(c.cx) + __builtin_fabsf(c.cy) + __builtin_fabsf(c.cz);
    const float mgn = __builtin_fmaf(0x1p-8f, dc + 3.0f * SS.R, SS.omgn + 0x1p-18f * c1);
    const float T = SS.R + c.rr + mgn;
    const float T2 = T * T, nb = -(SS.R + mgn);
    // NaN anywhere -> candidate; a ball that allows no culling keeps every sphere
    const bool valid = SS.ok && SceneOf<PATH>::shcull(p, rec) != nullptr && c.rr >= 0x1p-50f && dc >= 0x1p-30f && dc < 0x1p40f &&
                       c1 < 0x1p40f;
    unsigned memb = 0;
    for (int li = 0; li < p.L; ++li) {
        if (__builtin_amdgcn_ballot_w64((want >> li) & 1u) == 0) continue;  // wave-uniform
        const DevLight& l = SceneOf<PATH>::li(p, rec)[li];
        const bool l_ok = l.a >= 0x1p-40f && l.a <= 0x1p40f && l.a2 < __builtin_inff();  // wave-uniform
        const float wu = __builtin_fmaf(w.z, l.uz, __builtin_fmaf(w.y, l.uy, w.x * l.ux));
        const float wv = __builtin_fmaf(w.z, l.vz, __builtin_fmaf(w.y, l.vy, w.x * l.vx));
        const float wa = __builtin_fmaf(w.z, l.az, __builtin_fmaf(w.y, l.ay, w.x * l.ax));
        const bool line = __builtin_fmaf(wu, wu, wv * wv) > T2;
        const bool behind = wa < nb;
        const bool cull = valid & l_ok & (line | behind);
        memb |= (in & !cull) ? (1u << li) : 0u;
    }
    return memb;
}
// OR of a 32-bit value over the wave (all 64 lanes active): DPP row rotations give each 16-lane row
// its OR, four readlanes finish it.
__device__ __forceinline__ unsigned wave_or(unsigned v) {
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false);  // row_ror:1
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false);  // row_ror:2
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false);  // row_ror:4
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);  // row_ror:8
    return (unsigned)__builtin_amdgcn_readlane((int)v, 0) | (unsigned)__builtin_amdgcn_readlane((int)v, 16) |
           (unsigned)__builtin_amdgcn_readlane((int)v, 32) | (unsigned)__builtin_amdgcn_readlane((int)v, 48);
}

// The fold level from which the shadow grids serve (below it the ball bound; at it, per wave, whichever
// fits: shade_bundle).  Level 2 measured C4 +0.6 %, C5 -1.3 % (profiles/ab/r04_w2all_and_grid_level2.txt).
constexpr int GRID_FROM_LEVEL = 1;
// Candidate sets of the lights from the per-light shadow grids (p.shg != nullptr; rt_internal.h
// DevShadowGrid, host tables and the exactness argument in rt_api.cpp build_shadow_grid): each
// lane wanting light li looks up the grid cell of its own hit point's (u, v) and the axial slab of
// its a, ANDs the two masks, and the wave ORs them -- the union of per-lane sets instead of one bound
// around every lane's hit point, which grows with their spread (deep fold levels, where the hit
// points of a wave scatter over the scene; tools/shadow_cull_model.py: C4 sphere-light pairs per
// wave 27.4 -> 7.2).  Culling-only arithmetic (FMA allowed; the margins cover the projections'
// rounding).  Same result layout as shadow_members.  Converged call.
template <int PATH>
__device__ __forceinline__ unsigned shadow_members_grid(const LaunchParams& p, f3 hp, unsigned want, int rec) {
    const int lane = threadIdx.x & 63;
    const float l1 = __builtin_fabsf(hp.x) + __builtin_fabsf(hp.y) + __builtin_fabsf(hp.z);
    unsigned memb = 0;
    for (int li = 0; li < p.L; ++li) {
        const bool w = (want >> li) & 1u;
        if (__builtin_amdgcn_ballot_w64(w) == 0) continue;  // wave-uniform
        const DevShadowGrid& g = SceneOf<PATH>::shg(p, rec)[li];
        const DevLight& l = SceneOf<PATH>::li(p, rec)[li];
        const float u = __builtin_fmaf(hp.z, l.uz, __builtin_fmaf(hp.y, l.uy, hp.x * l.ux));
        const float v = __builtin_fmaf(hp.z, l.vz, __builtin_fmaf(hp.y, l.vy, hp.x * l.vx));
        const float a = __builtin_fmaf(hp.z, l.az, __builtin_fmaf(hp.y, l.ay, hp.x * l.ax));
        const bool near = l1 <= g.bound;  // NaN: far
        // grid cell (near lanes): outside the grid no disc reaches the lane.  Branch-free (bitwise
        // ands / ors): both table loads are issued unconditionally, at clamped in-range indices
        const float xu = __builtin_fmaf(u, g.su, g.ou), xv = __builtin_fmaf(v, g.sv, g.ov);
        const bool in_grid = (xu >= 0.0f) & (xu < (float)SHGRID_N) & (xv >= 0.0f) & (xv < (float)SHGRID_N);
        const unsigned iu = (unsigned)__builtin_fminf(__builtin_fmaxf(xu, 0.0f), (float)(SHGRID_N - 1));
        const unsigned iv = (unsigned)__builtin_fminf(__builtin_fmaxf(xv, 0.0f), (float)(SHGRID_N - 1));
        const unsigned long long cell = SceneOf<PATH>::shgrid(p, rec)[(unsigned)li * (SHGRID_N * SHGRID_N) + iv * SHGRID_N + iu];
        // slab of a (far lanes: lowered by their extra margin); NaN and below the range: entry 0 (all)
        const float mg = g.far_k * l1;
        const float af = near ? a : a - (mg - g.far_b);
        const float xa = __builtin_fminf(__builtin_fmaxf(__builtin_floorf(__builtin_fmaf(af, g.sa, g.oa)), -1.0f),
                                         (float)SHGRID_SLABS);
        const unsigned long long slab = SceneOf<PATH>::shslab(p, rec)[(unsigned)li * (SHGRID_SLABS + 2) + (unsigned)((int)xa + 1)];
        // far lanes: the box of every disc grown by the lane's own margin (NaN: inside)
        const bool out_box = (u < g.bu0 - mg) | (u > g.bu1 + mg) | (v < g.bv0 - mg) | (v > g.bv1 + mg);
        const bool take = w & (near ? in_grid : !out_box);
        const unsigned long long m = take ? (near ? cell : ~0ull) & slab : 0ull;
        const unsigned long long cm = ((unsigned long long)wave_or((unsigned)(m >> 32)) << 32) |
                                      (unsigned long long)wave_or((unsigned)m) | g.always;
        memb |= ((cm >> lane) & 1ull) ? (1u << li) : 0u;
    }
    return memb;
}

// A2OK: every light of the scene has 2a = 2 p.p finite and > 0 (LaunchParams::lights_a2_ok, host-checked; the
// kernel instantiation MERGED == 2): no per-light uniform check and no literal-formula fallback in the loop
// (C4 -0.4 %, C5 -0.4 %, profiles/ab/r05_merged_loop_ab.txt).
template <bool A2OK, int PATH, typename T>
__device__ __forceinline__ unsigned shadow_merged(const LaunchParams& p, unsigned memb, f3 hp, unsigned want, bool diff,
                                                  bool act, T& tl, int rec) {
    unsigned long long U = __builtin_amdgcn_ballot_w64(memb != 0u);
    unsigned blk = 0;
    while (U) {
        const int i = (int)__builtin_ctzll(U);
        U &= U - 1;
        const unsigned mi = (unsigned)__builtin_amdgcn_readlane((int)memb, i);  // lights with sphere i
        const DevSphere sp = SceneOf<PATH>::sph(p, rec)[i];
        const f3 oc = sub(hp, mk(sp.cx, sp.cy, sp.cz));  // shared by the lights (shadow_blocked's oc, c)
        const float c = dot(oc, oc) - sp.r2;
#pragma unroll
        for (int li = 0; li < SHADOW_MERGE_L; ++li) {
            if (((mi >> li) & 1u) == 0) continue;  // wave-uniform (li < p.L)
            const bool pending = ((want & ~blk) >> li) & 1u;
            if (__builtin_amdgcn_ballot_w64(pending) == 0) continue;  // wave-uniform
            tl.shadow_cat(pending ? 0 : (((want >> li) & 1u) ? 1 : (diff ? 2 : (act ? 3 : 4))), 1u);
            tl.shadow_sphere(pending);
            const DevLight& l = SceneOf<PATH>::li(p, rec)[li];
            const float b = 2.0f * dot(oc, mk(l.px, l.py, l.pz));
            const float disc = b * b - l.a4 * c;
            bool hit = false;
            if (A2OK || (l.a2 > 0.0f && l.a2 < __builtin_inff())) {  // wave-uniform (shadow_blocked<.., THRESH>)
                if (__builtin_amdgcn_ballot_w64(sphere_candidate(b, disc)) != 0) {
                    const float sq = cr_sqrt(disc);
                    hit = -b - sq >= l.sh_t;
                }
            } else if (disc >= 0.0f) {
                const float sq = __builtin_sqrtf(disc);
                const float t2 = (-b + sq) / l.a2;
                const float t1 = (-b - sq) / l.a2;
                hit = nmin(nmax0(t1 - 0.001f), nmax0(t2 - 0.001f)) > 0.0f;
            }
            blk |= (pending && hit) ? (1u << li) : 0u;
        }
        if (__builtin_amdgcn_ballot_w64((want & ~blk) != 0u) == 0) break;  // every wanted ray resolved
    }
    return blk;
}

// Shading of one shaded hit per active lane (TraceSphere :847-873 / TracePlane :736-778),
// converged call: the colour is accumulated in the reference's order -- mirror term (from
// the deeper segment `sec`), then each light in order, then ambient.  Inactive lanes
// return `sec` unchanged.  Shadow rays (IntersectShadowLight :573-582) of the lanes that
// need them form one bundle per light (common direction = the light position).
template <bool GPOW, int MERGED, int PATH, typename T>
__device__ __forceinline__ f3 shade_bundle(const LaunchParams& p, bool act, bool is_sphere, int prim, f3 hp, f3 d, float t,
                                           f3 sec, unsigned* n_shadow, T& tl, int level, int rec) {
    // idle lanes (act false) carry a copy of an active lane's record: same branches, result dropped
    const DevMaterial& m = SceneOf<PATH>::mat(p, rec)[is_sphere ? prim : p.S + prim];
    const uint32_t flags = m.flags;
    const bool diff = act && (flags & MAT_DIFFUSE) != 0;
    // checkerboard, :766-770: ((int)u + (int)v) & 1, unchecked int add -- first, for the dark-tile skip: a
    // plane hit on a dark square whose light terms are provably +0 (rt_dark.h) takes no part in the shadow pass
    // or the light loop; `lit` are the lanes that do (one test per hit, nothing per light)
    float tile = 1.0f;
    bool dark = false;
    if (!is_sphere) {
        const DevPlane& pl = SceneOf<PATH>::pl(p, rec)[prim];
        const float u = dot(mk(pl.e1x, pl.e1y, pl.e1z), hp);
        const float v = dot(mk(pl.e2x, pl.e2y, pl.e2z), hp);
        tile = checker_tile(u, v);
        dark = (flags & MAT_DARK_OK) != 0 && dark_lane_ok(hp.x, hp.y, hp.z, t, dot(d, d), tile);
    }
    const bool lit = diff && !dark;
    // S <= 64 and L <= SHADOW_MERGE_L: every light's shadow rays of the level in one merged pass,
    // first -- before the shading's own state is live.  Every lit lane's ray toward every light
    // is resolved (a superset of the shading's `need`); a cheap back-facing filter that skipped
    // some of them measured slower (C4 420 vs 401 us: its arithmetic on every lane of every level
    // cost more than the tests it saved, profiles/ab/r03_shadow_merged.txt).
    // MERGED (an instantiation of its own, so that neither path's code and registers burden the
    // other: S <= 64, 1 <= L <= SHADOW_MERGE_L, chosen on the host)
    const bool merged = MERGED != 0 && __builtin_amdgcn_ballot_w64(lit) != 0;
    unsigned blk = 0u;
    if (merged)
        for (int li = 0; li < p.L; ++li) tl.shadow(diff);  // (diagnostic tally of the rays resolved)
    if (merged) {
        const unsigned want = lit ? (1u << p.L) - 1u : 0u;
        // per-lane grid lookups below the first fold level, where a wave's hit points scatter; at
        // level 0 (the tile's primary hits, coherent) one bound around them culls tighter than the
        // grid's cells; at the first fold level whichever fits the wave: the ball while the hit points
        // lie within one grid cell of their centre (light 0's cell size), the grid otherwise (C4 -1.3 %,
        // C5 -1.6 % against the grid there, profiles/ab/r04_adaptive_level1.txt).  Wave-uniform choices.
        unsigned memb;
        if (SceneOf<PATH>::shg(p, rec) && level > GRID_FROM_LEVEL) {
            memb = shadow_members_grid<PATH>(p, hp, want, rec);
        } else if (SceneOf<PATH>::shg(p, rec) && level == GRID_FROM_LEVEL) {
            const ShadowSphere SS = make_shadow_sphere(hp, lit);
            const float cell = 1.0f / __builtin_fmaxf(SceneOf<PATH>::shg(p, rec)[0].su, SceneOf<PATH>::shg(p, rec)[0].sv);
            memb = SS.ok && SS.R < cell ? shadow_members_fast<PATH>(p, SS, want, rec) : shadow_members_grid<PATH>(p, hp, want, rec);
        } else {
            memb = shadow_members_fast<PATH>(p, make_shadow_sphere(hp, lit), want, rec);
        }
        blk = shadow_merged<MERGED == 2, PATH>(p, memb, hp, want, diff, act, tl, rec);
    }
    f3 normal;
    if (is_sphere) {
        const DevSphere& s = SceneOf<PATH>::sph(p, rec)[prim];
        normal = normalize(sub(hp, mk(s.cx, s.cy, s.cz)));  // SpherePhongShading :706
    } else {
        const DevPlane& pl = SceneOf<PATH>::pl(p, rec)[prim];
        normal = mk(pl.nx, pl.ny, pl.nz);
    }
    f3 col = mk(0.0f, 0.0f, 0.0f);
    if (flags & MAT_MIRROR) col = add(col, mul(sec, mk(m.km[0], m.km[1], m.km[2])));
    if (__builtin_amdgcn_ballot_w64(lit) != 0) {
        const f3 view = normalize(d);  // ShapePhongShading :668 (not negated)
        // sphere: (1 / t) * t (:866);  plane: (float)(1 / Math.Pow(t, 2)) (:754), exact as 1/(t*t) in f64
        const float att = is_sphere ? sphere_att(t) : plane_att(t);
        const f3 kd = mk(m.kd[0], m.kd[1], m.kd[2]);
        const f3 ks = mk(m.ks[0], m.ks[1], m.ks[2]);  // once, not per light under the MAT_SPEC branch
        const uint32_t pk = m.pow_kind;
        const float pn = m.n;
        ShadowSphere SS{};
        if (MERGED == 0) SS = make_shadow_sphere(hp, lit);  // one bound for every light's shadow rays
        unsigned long long umask = 0;  // (diagnostic builds: the union of the lights' candidates)
        for (int li = 0; li < p.L; ++li) {
            const DevLight& l = SceneOf<PATH>::li(p, rec)[li];
            const f3 lp = mk(l.px, l.py, l.pz);
            const bool l_ok = l.a2 > 0.0f && l.a2 < __builtin_inff();  // wave-uniform
            // ShapePhongShading, :665-695 (first: it decides whether the shadow test matters)
            const f3 ldir = normalize(sub(lp, hp));
            f3 ph = scale(kd, nmax0(dot(normal, ldir)));
            f3 spec = mk(0.0f, 0.0f, 0.0f);
            if (flags & MAT_SPEC) {
                const f3 rs = sub(ldir, scale(normal, 2.0f * dot(ldir, normal)));
                const float sp = spec_pow<GPOW>(nmax0(dot(view, normalize(rs))), pk, pn);
                spec = mul(ks, mk(sp, sp, sp));
            }
            ph = add(ph, spec);
            // MERGED: every lit lane's ray toward every light is resolved (blk), so the pixel takes the
            // reference's intensity directly and the skip test (shadow_matters) is not needed
            const bool need = MERGED != 0 ? lit : lit && shadow_matters(ph, l.intensity, att);
            bool blocked = merged ? ((blk >> li) & 1u) != 0 : !need;
            if (MERGED == 0 && __builtin_amdgcn_ballot_w64(need) != 0) {  // some lane's pixel depends on this test
                // (MERGED without a lit lane: no lane needs a test)
                tl.shadow(need);
                const f3 hs = need ? hp : SS.O;  // idle lanes mirror a shading lane (results ignored)
                for (int base = 0; base < p.S; base += 64) {
                    const int n = min(64, p.S - base);
                    unsigned long long mk64 = shadow_sphere_cull<PATH>(p, SS, l, li, base, n, rec);
                    tl.shadow_masks(5, mk64);
                    umask |= mk64;
                    // candidates two at a time: independent tests (ILP across the sqrt chains),
                    // one pair of sphere loads and one exit ballot per pair; an odd last
                    // candidate is tested twice (the OR is unchanged)
                    while (mk64) {
                        const int i0 = base + (int)__builtin_ctzll(mk64);
                        mk64 &= mk64 - 1;
                        const bool two = mk64 != 0;
                        const int i1 = two ? base + (int)__builtin_ctzll(mk64) : i0;
                        if (two) mk64 &= mk64 - 1;
                        const DevSphere s0 = SceneOf<PATH>::sph(p, rec)[i0], s1 = SceneOf<PATH>::sph(p, rec)[i1];
                        tl.shadow_cat(need ? (blocked ? 1 : 0) : (diff ? 2 : (act ? 3 : 4)), 2u);
                        tl.shadow_sphere(!blocked);
                        const bool h0 = shadow_blocked<false, true>(hs, l, l_ok, s0);
                        tl.shadow_sphere(two && !blocked && !h0);
                        const bool h1 = shadow_blocked<false, true>(hs, l, l_ok, s1);
                        blocked = blocked | h0 | h1;  // no short-circuit branch
                        if (__builtin_amdgcn_ballot_w64(!blocked) == 0) break;
                    }
                    if (__builtin_amdgcn_ballot_w64(!blocked) == 0) break;
                }
            }
            const float inten = (!lit || (need && blocked)) ? 0.0f : l.intensity;
            const float ia = inten * att;
            f3 term = mul(mk(ia, ia, ia), ph);
            if (!is_sphere) {
                term = mul(term, mk(tile, tile, tile));
                term = mk(nmax0(term.x), nmax0(term.y), nmax0(term.z));  // .Max(0f), :775
            }
            if (lit) col = add(col, term);
        }
        tl.shadow_masks(6, umask);
    }
    // (the nominal count: shaded diffuse hits x lights, dark or not)
    if (diff) *n_shadow += (unsigned)p.L << CNT_SHADOW_SHIFT;
    col = add(col, mk(m.amb[0], m.amb[1], m.amb[2]));
    return act ? col : sec;
}

// Backward fold (converged call, all 64 lanes): level by level from the deepest, every recorded
// hit is shaded; a mirror hit consumes the colour of the segment after it (levels 0..limit push
// at most one record each, so K = limit + 1 records suffice).  Returns the lane's colour.
template <bool GPOW, int MERGED, int PATH, typename STK, typename T>
__device__ __forceinline__ f3 fold_converged(const LaunchParams& p, STK& stk, f3 leaf, unsigned* cnt, T& tl, int rec) {
    f3 col = leaf;
    const int depth = stk.n;
    int level = (int)wave_max((float)depth);
    while (level-- > 0) {
        const bool act = level < depth;  // this lane's top record is at `level`
        float4 ra = make_float4(0.0f, 0.0f, 0.0f, 1.0f), rb = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
        if (act) stk.template pop<PATH>(p, ra, rb, rec);
        const unsigned long long am = __builtin_amdgcn_ballot_w64(act);
        if (am != ~0ull) {  // idle lanes shade a copy of the first active lane's record
            const int ref = __builtin_ctzll(am);
            const float4 qa = make_float4(readlane_f(ra.x, ref), readlane_f(ra.y, ref), readlane_f(ra.z, ref),
                                          readlane_f(ra.w, ref));
            const float4 qb = make_float4(readlane_f(rb.x, ref), readlane_f(rb.y, ref), readlane_f(rb.z, ref),
                                          readlane_f(rb.w, ref));
            if (!act) {
                ra = qa;
                rb = qb;
            }
        }
        const int code = __float_as_int(rb.w);
        const bool is_s = code >= 0;
        tl.set_level(level);
        col = shade_bundle<GPOW, MERGED, PATH>(p, act, is_s, is_s ? code : ~code, mk(ra.x, ra.y, ra.z), mk(rb.x, rb.y, rb.z),
                                         ra.w, col, cnt, tl, level, rec);
    }
    return col;
}

// BUNDLE kernel (scenes with >= CULL_MIN_SPHERES spheres): converged control flow so that
// every segment and every light can form a wave bundle and cull the sphere list.
template <int K, unsigned V, typename T>
__device__ __forceinline__ TileOut trace_tile_bundle(const LaunchParams& p, int tile_x, int tile_y, float2* stk_lv,
                                                     float* stk_dv, T& tl, int recp = 0) {
    constexpr bool GPOW = (V & VF_GPOW) != 0, TILES = (V & VF_TILES) != 0, SS = ss_of(V), SHUTTER = shutter_of(V);
    constexpr bool ADAPT = adapt_of(V);
    constexpr int PATH = view_of(V);
    constexpr int MERGED = vf_cls_of(V);
    // (SHUTTER_ADAPT: the sample pass above the record index, as in trace_tile_direct)
    const int rec = shutter_adapt_of(V) ? recp & ((1 << REC_BITS) - 1) : recp, pass = shutter_adapt_of(V) ? recp >> REC_BITS : recp;
    const int lane = threadIdx.x & 63;
    const TilePixel tpx = ADAPT ? sample_pixel(p, tile_x, tile_y, lane, pass)
                                : tile_pixel<SS>(p, tile_x * TILE_W + (lane & 7), tile_y * TILE_H + (lane >> 3));
    const int x = tpx.x, y = tpx.y;
    const bool valid = tpx.valid;

    unsigned cnt = 0;  // packed: reflected segments (bits 0-7) | shadow rays << CNT_SHADOW_SHIFT
    const ViewOf<PATH> vw{p, rec};
    const f3 cam = vw.cam();
    // TracePixel primary ray, :963-971 (no half-pixel offset)
    // per-column / per-row tables (see the direct kernel); lanes outside the frame read 0
    const float lx = tpx.lx, ly = tpx.ly, lz = 1.0f * p.nearc;
    const f3 vp = add(add(add(cam, scale(vw.right(), lx)), scale(vw.up(), ly)), scale(vw.fwd(), lz));
    f3 d = normalize(sub(vp, cam));
    f3 o = cam;

    // forward walk: all lanes advance one segment per iteration (converged loop), each
    // shaded hit pushes a record; mirror hits continue with the reflected segment
    typename StackFor<K>::type stk(stk_lv, stk_dv);
    stk.origin(d);
    f3 leaf = mk(0.0f, 0.0f, 0.0f);
    bool active = valid;
    const unsigned long long pmask = vw.prim_const() ? prim_box_mask<PATH>(p, x, y, rec) : 0;
    Hit h = nearest_bundle<true, PATH>(p, o, d, active, tl, pmask, nullptr, rec);
    for (int count = 0;; ++count) {
        if (active) {
            const bool is_sphere = h.prim >= 0;
            if (h.prim == HIT_NONE || h.t - 0.01f <= 0.0f) {  // nothing hit / too close: Zero (:731, :839)
                active = false;
            } else if (count > p.limit) {  // terminal segment: Zero / One (:734, :843)
                if (!is_sphere) leaf = mk(1.0f, 1.0f, 1.0f);
                active = false;
            } else {
                const f3 hp = add(o, scale(d, h.t));
                stk.push(make_float4(hp.x, hp.y, hp.z, h.t), make_float4(d.x, d.y, d.z, __int_as_float(h.prim)));
                const int prim = is_sphere ? h.prim : ~h.prim;
                const uint32_t flags = SceneOf<PATH>::mat(p, rec)[is_sphere ? prim : p.S + prim].flags;
                if (!(flags & MAT_MIRROR)) {
                    active = false;
                } else {
                    o = reflect_at<PATH>(p, o, d, h.t, h.prim, rec);  // :854, CalculateReflectionRay :718-720
                    ++cnt;
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(active) == 0) break;
        if (count + 1 > p.limit) {
            // terminal segment (see terminal_direct): only lanes whose nearest plane lies beyond
            // 0.01 need the spheres; the others are Zero
            float best_p = __builtin_inff();
            int win_p = -1;
            for (int i = 0; i < p.P; ++i) {
                tl.plane(active);
                plane_take(o, d, SceneOf<PATH>::pl(p, rec)[i], i, best_p, win_p);  // t > 0 && t < best
            }
            const bool need = active && win_p >= 0 && best_p - 0.01f > 0.0f;
            h = Hit{0.0f, HIT_NONE};
            if (__builtin_amdgcn_ballot_w64(need) != 0) {
                const Hit pl{best_p, win_p};  // (idle lanes: replaced by a copy of an active lane's ray)
                const Hit hn = nearest_bundle<false, PATH>(p, o, d, need, tl, 0, &pl, rec);
                if (need) h = hn;
            }
        } else {
            h = nearest_bundle<false, PATH>(p, o, d, active, tl, 0, nullptr, rec);
        }
    }

    const f3 col = fold_converged<GPOW, MERGED, PATH>(p, stk, leaf, &cnt, tl, rec);
    const uint32_t px32 = (shift_channel(col.x) << 16) | (shift_channel(col.y) << 8) | shift_channel(col.z);
    if constexpr (TILES) encode_tile_fused(p, px32, valid);
    else if constexpr (!SHUTTER && !ADAPT) {
        // the pixel's coordinates again, from the lane id (mbcnt) and the block id: cheaper than
        // keeping x, r, y and `valid` live through the walk and the fold (64-VGPR cap: they were
        // the values spilled to scratch once the merged shadow pass raised the peak)
        const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const TilePixel q = tile_pixel<SS>(p, tile_x * TILE_W + (ln & 7), tile_y * TILE_H + (ln >> 3));
        if constexpr (SS) resolve_tile(p, q.r, q.y, q.x, q.valid, px32);
        else if (q.valid) store_pixel(p, q.r, q.y, q.x, px32);
    }
    return TileOut{cnt, px32};  // (lanes outside the frame: a value that is never stored)
}

// Occupancy: a wave's SGPRs count against a per-SIMD file of ~800 (waves per SIMD <=
// 800 / (ceil(sgpr / 16) * 16 + 16), MI355X_MICROARCH.md 'Residency'): the compiler's 93-106
// SGPRs admitted 6-7 waves per SIMD whatever its report said.  Capped at 80 (a few uniform values
// spilled to VGPR lanes) and 64 VGPRs (8 waves): C4 -2.6 %, C5 -7.5 %.  Not with GPOW (the f64
// Math.Pow path would spill ~150 B/lane to scratch).  The direct kernel is capped at 80 SGPRs too (its shadow
// pre-test, trace_direct_kernel).
// TORD: the single-frame launches' tile order as in the direct kernel (0 = natural, 1 = tile_order over the
// 2-D grid, 2 = natural and every wave records its duration in tile_cost).  V: the variant word (vf_cls = MERGED).
template <int K, unsigned V>
__device__ __forceinline__ void bundle_kernel_body(const LaunchParams& p) {
    constexpr bool STATS = (V & VF_STATS) != 0, SHUTTER = shutter_of(V);
    constexpr int PATH = view_of(V);
    constexpr int TORD = vf_tord_of(V);
    constexpr int LDS_LEVELS = StackFor<K>::lds_levels;  // LdsStack slots, else unused
    __shared__ float2 stk_lv[LDS_LEVELS > 0 ? LDS_LEVELS * WG_THREADS : 1];
    __shared__ float stk_dv[LDS_LEVELS > 0 ? 3 * WG_THREADS : 1];
    if (blockIdx.z < (unsigned)p.copy_z) {  // wave-uniform: the fused hand-off's copy slice
        copy_slice(p);
        return;
    }
    Tally<STATS> tl;
    tl.init(p);
    int tile_x = (int)blockIdx.x, tile_y = (int)blockIdx.y;
    if constexpr (TORD == 1) {
        const uint32_t t = p.tile_order[blockIdx.y * gridDim.x + blockIdx.x];
        tile_x = (int)(t & 0xffffu), tile_y = (int)(t >> 16);  // (0xffff: past the frame, no pixel valid)
    }
    struct TileRec {
        unsigned* slot;
        unsigned t0;
    };
    __shared__ TileRec t_rec[1];
    if (TORD == 2 && (threadIdx.x & 63) == 0)  // (a batch launch's frame 0 records; the others store nothing)
        t_rec[0] = TileRec{blockIdx.z == (unsigned)p.copy_z ? p.tile_cost + (blockIdx.y * gridDim.x + blockIdx.x) : nullptr,
                           (unsigned)__builtin_amdgcn_s_memrealtime()};
    if constexpr (shutter_adapt_of(V)) {
        shutter_adaptive_tile(p, tile_x, tile_y, [&](const LaunchParams& q, int recp, int tx, int ty) { return trace_tile_bundle<K, V & VF_TILE>(q, tx, ty, stk_lv, stk_dv, tl, recp); });
        return;
    }
    if constexpr (SHUTTER) {
        shutter_tile<ss_of(V)>(p, tile_x, tile_y, [&](const LaunchParams& q, int rec, int tx, int ty) { return trace_tile_bundle<K, V & VF_TILE>(q, tx, ty, stk_lv, stk_dv, tl, rec); });
        return;
    }
    if constexpr (adapt_of(V)) {
        adaptive_tile<PATH != VIEW_ARGS>(p, tile_x, tile_y, [&](const LaunchParams& q, int pass, int tx, int ty) { return trace_tile_bundle<K, V & VF_TILE>(q, tx, ty, stk_lv, stk_dv, tl, pass); });
        return;
    }
    if constexpr ((V & VF_PROG) != 0) {
        progressive_tile(p, tile_x, tile_y, [&](const LaunchParams& q, int pass, int tx, int ty) { return trace_tile_bundle<K, ((V & VF_TILE) & ~VF_PROG) | VF_ADAPT>(q, tx, ty, stk_lv, stk_dv, tl, pass); });
        return;
    }
    const unsigned cnt = trace_tile_bundle<K, V & VF_TILE>(p, tile_x, tile_y, stk_lv, stk_dv, tl).cnt;
    add_counters<STATS, PATH>(p, threadIdx.x & 63, cnt & CNT_REFL_MASK, cnt >> CNT_SHADOW_SHIFT, tl);
    if (TORD == 2 && (threadIdx.x & 63) == 0 && t_rec[0].slot != nullptr)
        *t_rec[0].slot = (unsigned)__builtin_amdgcn_s_memrealtime() - t_rec[0].t0;
}
template <int K, unsigned V>
__global__ __launch_bounds__(WG_THREADS, 8) __attribute__((amdgpu_num_sgpr(80))) void trace_bundle_kernel(
    LaunchParams p) {
    static_assert(!(V & VF_GPOW), "GPOW variants run trace_bundle_kernel_gpow");
    bundle_kernel_body<K, V>(p);
}
template <int K, unsigned V>
__global__ __launch_bounds__(WG_THREADS) void trace_bundle_kernel_gpow(LaunchParams p) {
    static_assert((V & VF_GPOW) != 0, "variants without GPOW run trace_bundle_kernel");
    bundle_kernel_body<K, V>(p);
}

#if RT_KERNEL_PART == 0  // (the kernels that are no templates: once, in part 0)
// ---------------------------------------------------------------------------------
// Debug ray view: re-trace sampled pixels with the direct path's
// selection rules and append their visible-path segments.  Not on the timed path.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void append_segment(DevSegment* out, int cap, unsigned* count, f3 o, f3 e, int kind,
                                               int pixel) {
    const unsigned i = atomicAdd(count, 1u);
    if (i < (unsigned)cap) out[i] = DevSegment{o.x, o.y, o.z, e.x, e.y, e.z, kind, pixel};
}

__global__ __launch_bounds__(256) void debug_segments_kernel(LaunchParams p, int stride, DevSegment* out, int cap,
                                                             unsigned* count) {
    constexpr int PATH = VIEW_ARGS;  // (the launch's own view and scene image)
    constexpr int rec = 0;
    const long long idx = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * (long long)stride;
    if (idx >= (long long)p.W * p.H) return;
    const int x = (int)(idx % p.W), y = (int)(idx / p.W);
    const f3 cam = mk(p.cam[0], p.cam[1], p.cam[2]);
    const float px = (float)x / (float)p.W - 0.5f;
    const float py = (float)y / (float)p.H - 0.5f;
    const f3 vp = add(add(add(cam, scale(mk(p.right[0], p.right[1], p.right[2]), px * p.pw)),
                          scale(mk(p.up[0], p.up[1], p.up[2]), py * p.ph)),
                      scale(mk(p.fwd[0], p.fwd[1], p.fwd[2]), 1.0f * p.nearc));
    f3 d = normalize(sub(vp, cam));
    f3 o = cam;
    Tally<false> tl;
    Hit h = nearest_direct<true, false, VIEW_ARGS>(p, o, d, tl, p.S >= 64 ? ~0ull : (1ull << p.S) - 1, rec);  // every sphere
    for (int level = 0;; ++level) {
        const bool none = h.prim == HIT_NONE;
        append_segment(out, cap, count, o, add(o, scale(d, none ? 100.0f : h.t)), level == 0 ? 0 : 1,
                       (int)idx);
        if (none || h.t - 0.01f <= 0.0f || level > p.limit) break;
        const bool is_sphere = h.prim >= 0;
        const int prim = is_sphere ? h.prim : ~h.prim;
        const f3 hp = add(o, scale(d, h.t));
        const DevMaterial& m = SceneOf<PATH>::mat(p, rec)[is_sphere ? prim : p.S + prim];
        if (m.flags & MAT_DIFFUSE) {
            for (int li = 0; li < p.L; ++li) {  // IntersectShadowLight's ray per light
                const DevLight& l = SceneOf<PATH>::li(p, rec)[li];
                const bool l_ok = l.a2 > 0.0f && l.a2 < __builtin_inff();
                const f3 lp = mk(l.px, l.py, l.pz);
                float tb = 1.0f;
                for (int i = 0; i < p.S; ++i) {
                    if (shadow_blocked<false>(hp, l, l_ok, SceneOf<PATH>::sph(p, rec)[i])) {
                        const f3 oc = sub(hp, mk(SceneOf<PATH>::sph(p, rec)[i].cx, SceneOf<PATH>::sph(p, rec)[i].cy, SceneOf<PATH>::sph(p, rec)[i].cz));
                        const float b = 2.0f * dot(oc, lp);
                        const float c = dot(oc, oc) - SceneOf<PATH>::sph(p, rec)[i].r2;
                        const float sq = __builtin_sqrtf(b * b - l.a4 * c);
                        tb = (-b - sq) / l.a2;
                        break;
                    }
                }
                append_segment(out, cap, count, hp, add(hp, scale(lp, tb)), 2, (int)idx);
            }
        }
        if (!(m.flags & MAT_MIRROR)) break;
        const f3 normal = is_sphere ? normalize(sub(hp, mk(SceneOf<PATH>::sph(p, rec)[prim].cx, SceneOf<PATH>::sph(p, rec)[prim].cy, SceneOf<PATH>::sph(p, rec)[prim].cz)))
                                    : mk(SceneOf<PATH>::pl(p, rec)[prim].nx, SceneOf<PATH>::pl(p, rec)[prim].ny, SceneOf<PATH>::pl(p, rec)[prim].nz);
        d = sub(d, scale(normal, 2.0f * dot(d, normal)));
        o = hp;
        h = nearest_direct<false, false, VIEW_ARGS>(p, o, d, tl, 0, rec);
    }
}

// ---------------------------------------------------------------------------------
// Hit buffers (rt_render_hits*, rt_pick): what the primary ray of a pixel selects, by TracePixel's rule (:973-993)
// as level 0 of the trace kernels applies it -- and nothing after it: no shading, no shadow ray, no reflection.
// ---------------------------------------------------------------------------------
// One pixel's record.  Nothing selected: depth +inf, object -1 (RT_HIT_NONE), the point 100 along the ray (as the
// debug view's segment end), normal 0.  A selected hit with t - 0.01 <= 0, which the colour frame renders black
// (:731, :839), is reported like any other.
struct PixelHit {
    float depth;
    int object;
    f3 pos, nrm;
};
// The primary ray of view-plane coordinates (lx, ly) (:963-971) and its selected hit: nearest_direct's, with the wave's
// screen-box candidates `pmask` when the view has primary constants.  skip (wave-uniform; a sky wave, sky_tile):
// nothing can be selected and nothing is tested.  Divergent call, as trace_tile_direct's level 0.
template <int PATH>
__device__ __forceinline__ PixelHit primary_hit(const LaunchParams& p, float lx, float ly, unsigned long long pmask, bool skip) {
    constexpr int rec = 0;  // (the views and scene images of a hit launch go by blockIdx.z alone)
    const ViewOf<PATH> vw{p, rec};
    const f3 cam = vw.cam();
    const f3 vp = add(add(add(cam, scale(vw.right(), lx)), scale(vw.up(), ly)), scale(vw.fwd(), 1.0f * p.nearc));
    const f3 d = normalize(sub(vp, cam));
    Tally<false> tl;
    Hit h{0.0f, HIT_NONE};
    if (!skip) h = nearest_direct<true, false, PATH>(p, cam, d, tl, pmask, rec);
    if (h.prim == HIT_NONE) return PixelHit{__builtin_inff(), -1, add(cam, scale(d, 100.0f)), mk(0.0f, 0.0f, 0.0f)};
    const f3 hp = add(cam, scale(d, h.t));  // :846 / :736
    if (h.prim >= 0) {
        const DevSphere s = SceneOf<PATH>::sph(p, rec)[h.prim];  // (the winner's centre: a per-lane fetch)
        return PixelHit{h.t, h.prim, hp, normalize(sub(hp, mk(s.cx, s.cy, s.cz)))};  // :706
    }
    const DevPlane& q = SceneOf<PATH>::pl(p, rec)[~h.prim];
    return PixelHit{h.t, p.S + ~h.prim, hp, mk(q.nx, q.ny, q.nz)};  // :653: the normal as given
}

// One wave per 8x8 tile, frames in grid z, each lane its own pixel: a tile row is 32 contiguous bytes of depth or
// object and 96 of position or normal.  The candidates and the sky test are trace_tile_direct's; a sky wave stores the
// nothing-selected records without a test.  No LDS, no scratch, no atomics; lanes outside the frame store nothing.
template <int PATH>
__global__ __launch_bounds__(WG_THREADS) void hits_kernel(LaunchParams p, HitOut out) {
    const int lane = threadIdx.x & 63;
    const TilePixel t = tile_pixel(p, (int)blockIdx.x * TILE_W + (lane & 7), (int)blockIdx.y * TILE_H + (lane >> 3));
    const unsigned long long pmask = ViewOf<PATH>{p, 0}.prim_const() ? prim_box_mask<PATH>(p, t.x, t.y, 0) : 0;
    const bool sky = sky_tile<PATH>(p, t, pmask, 0);  // wave-uniform
    if (!t.valid) return;
    const PixelHit h = primary_hit<PATH>(p, t.lx, t.ly, pmask, sky);
    const size_t i = (size_t)blockIdx.z * ((size_t)p.W * (size_t)p.H) + (size_t)t.y * (size_t)p.W + (size_t)t.x;
    if (out.depth) out.depth[i] = h.depth;  // (kernel arguments: wave-uniform tests)
    if (out.object) out.object[i] = h.object;
    if (out.position) {
        float* q = out.position + 3 * i;
        q[0] = h.pos.x, q[1] = h.pos.y, q[2] = h.pos.z;
    }
    if (out.normal) {
        float* q = out.normal + 3 * i;
        q[0] = h.nrm.x, q[1] = h.nrm.y, q[2] = h.nrm.z;
    }
}

// rt_pick: one wave, every lane on pixel (x, y) -- so the candidates are the spheres whose box holds the pixel --
// through the same primary_hit; lane 0 stores the record.
__global__ __launch_bounds__(WG_THREADS) void pick_kernel(LaunchParams p, int x, int y, float lx, float ly, DevPick* out) {
    const unsigned long long pmask = p.prim_const ? prim_box_mask<VIEW_ARGS>(p, x, y, 0) : 0;
    const PixelHit h = primary_hit<VIEW_ARGS>(p, lx, ly, pmask, false);
    if ((threadIdx.x & 63) == 0)
        *out = DevPick{h.object, h.depth, {h.pos.x, h.pos.y, h.pos.z}, {h.nrm.x, h.nrm.y, h.nrm.z}};
}

// Reassemble packed row bands (rt_render_bands layout) into a row-major frame.
__global__ __launch_bounds__(256) void scatter_bands_kernel(const int32_t* __restrict__ bands,
                                                            int32_t* __restrict__ frame, int W, int H, int band_rows,
                                                            int band_first, int band_step, int local_rows) {
    const size_t total = (size_t)local_rows * (size_t)W;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / (size_t)W);
        const int x = (int)(i - (size_t)r * W);
        const int y = (band_first + (r / band_rows) * band_step) * band_rows + r % band_rows;
        if (y < H) frame[(size_t)y * W + x] = bands[i];
    }
}

// Reassemble every rank's gathered band set into the row-major frame in one launch:
// frame row y is band b = y / band_rows, owned by rank b % world as its (b / world)-th band.
__global__ __launch_bounds__(256) void scatter_gathered_kernel(const unsigned char* __restrict__ g, size_t slot_bytes,
                                                               int fmt, int32_t* __restrict__ frame, int W, int H,
                                                               int band_rows, int world) {
    const size_t total = (size_t)W * (size_t)H;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / (size_t)W);
        const int x = (int)(i - (size_t)y * W);
        const int b = y / band_rows;
        const int rank = b % world;
        const size_t local = ((size_t)(b / world) * band_rows + (size_t)(y % band_rows)) * (size_t)W + (size_t)x;
        const unsigned char* src = g + (size_t)rank * slot_bytes;
        int32_t v;
        if (fmt == 0) {
            v = ((const int32_t*)src)[local];
        } else {
            const unsigned char* q = src + local * 3;
            v = (int32_t)((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16));
        }
        frame[i] = v;
    }
}

#endif  // RT_KERNEL_PART == 0

// ---------------------------------------------------------------------------------
// Trace launch: the variant (rt_internal.h pick_trace_variant), its grid, and one dispatch from the descriptor's
// runtime fields to the instantiation.
// ---------------------------------------------------------------------------------
// The grid and block of a launch of variant v: one workgroup per 8x8 tile, frames (and the copy slice) in z.  A
// lone frame on the direct kernel (wpg > 1) has wpg tiles of a tile row per workgroup, with the tile rows
// in x when col_major is set, or a 1-D grid over the padded tile_order.
#if RT_KERNEL_PART == 0
static void trace_grid(const LaunchParams& p, const TraceVariant& v, dim3* grid, dim3* block) {
    // (ADAPT, PROG, PATH_ADAPT, ANIM_ADAPT: a wave is a tile of output pixels, and W, local_rows are in samples; in
    // ANIM_SHUTTER_SS, as in SHUTTER_SS and every other SS twin, a lane is a sample and the grid is in sample tiles)
    const int as = v.mode == TM_ADAPT || v.mode == TM_PROG || v.mode == TM_PATH_ADAPT || v.mode == TM_ANIM_ADAPT ||
                           v.mode == TM_SHUTTER_ADAPT || v.mode == TM_ANIM_SHUTTER_ADAPT
                       ? p.ss_log2
                       : 0;
    const unsigned tx = (unsigned)(((p.W >> as) + TILE_W - 1) / TILE_W), ty = (unsigned)(((p.local_rows >> as) + TILE_H - 1) / TILE_H);
    const unsigned z = (unsigned)(p.n_frames > 1 ? p.n_frames : 1) + (unsigned)p.copy_z, w = (unsigned)v.wpg;
    const unsigned gxw = (tx + w - 1) / w;
    *block = dim3(WG_THREADS * w);
    if (w == 1) *grid = dim3(tx, ty, z);
    else if (p.tile_order != nullptr) *grid = dim3((tx * ty + w - 1) / w, 1u, z);
    else *grid = p.col_major ? dim3(ty, gxw, z) : dim3(gxw, ty, z);
}

#endif  // RT_KERNEL_PART == 0

// peel(leaf, Vals<>{}, field, Vals<the values it takes...>{}, field, Vals<...>{}, ...): one runtime field per
// level becomes a compile-time constant; leaf(Vals<constants...>{}) runs for the one combination that matches.
// false: a field holds a value outside its list, or the leaf said so.
template <int... VS>
struct Vals {};
template <typename F, int... DONE>
static bool peel(F& leaf, Vals<DONE...> done) {
    return leaf(done);
}
template <typename F, int... DONE, int... VS, typename... REST>
static bool peel(F& leaf, Vals<DONE...>, int field, Vals<VS...>, REST... rest) {
    return ((field == VS && peel(leaf, Vals<DONE..., VS>{}, rest...)) || ...);
}

// The instantiation of one descriptor, launched; false (and nothing instantiated) for one that is not built, or not in
// this part.
template <int FAMILY, int GPOW, int MODE, int CLS, int K, int WPG, int TORD>
static bool launch_built(Vals<FAMILY, GPOW, MODE, CLS, K, WPG, TORD>, const LaunchParams& p, dim3 grid, dim3 block,
                         hipStream_t s) {
    constexpr TraceVariant v{FAMILY, GPOW, MODE, CLS, K, WPG, TORD};
    if constexpr (trace_variant_built(v) && trace_mode_part(MODE) == RT_KERNEL_PART) {
        constexpr unsigned V = variant_word(v);
        if constexpr (FAMILY == TV_DIRECT && GPOW) hipLaunchKernelGGL((trace_direct_kernel_gpow<K, V>), grid, block, 0, s, p);
        else if constexpr (FAMILY == TV_DIRECT) hipLaunchKernelGGL((trace_direct_kernel<K, V>), grid, block, 0, s, p);
        else if constexpr (GPOW) hipLaunchKernelGGL((trace_bundle_kernel_gpow<K, V>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((trace_bundle_kernel<K, V>), grid, block, 0, s, p);
        return true;
    }
    return false;
}

// One dispatch from the descriptor's runtime fields to the instantiation, over the instantiations of part PART: each
// part's unit defines its own.
template <int PART>
bool launch_trace_part(const TraceVariant& v, const LaunchParams& p, dim3 grid, dim3 block, hipStream_t s);
template <>
bool launch_trace_part<0>(const TraceVariant& v, const LaunchParams& p, dim3 grid, dim3 block, hipStream_t s);
template <>
bool launch_trace_part<1>(const TraceVariant& v, const LaunchParams& p, dim3 grid, dim3 block, hipStream_t s);
template <>
bool launch_trace_part<2>(const TraceVariant& v, const LaunchParams& p, dim3 grid, dim3 block, hipStream_t s);
template <>
bool launch_trace_part<3>(const TraceVariant& v, const LaunchParams& p, dim3 grid, dim3 block, hipStream_t s);

template <>
bool launch_trace_part<RT_KERNEL_PART>(const TraceVariant& v, const LaunchParams& p, dim3 grid, dim3 block, hipStream_t s) {
    auto leaf = [&](auto consts) { return launch_built(consts, p, grid, block, s); };
    return peel(leaf, Vals<>{}, v.family, Vals<TV_DIRECT, TV_BUNDLE>{}, v.gpow, Vals<0, 1>{}, v.mode,
              Vals<TM_PLAIN, TM_STATS, TM_TILES, TM_SS, TM_PATH, TM_SHUTTER, TM_ADAPT, TM_PROG, TM_ANIM, TM_PATH_SS, TM_SHUTTER_SS, TM_ANIM_SS, TM_PATH_ADAPT, TM_ANIM_ADAPT, TM_ANIM_SHUTTER, TM_ANIM_SHUTTER_SS, TM_SHUTTER_ADAPT, TM_ANIM_SHUTTER_ADAPT>{}, v.cls, Vals<0, 1, 2, DIRECT_SMAX>{}, v.K,
              Vals<1, 2, 4, 6, 8, 64>{}, v.wpg, Vals<1, SINGLE_WPG>{}, v.tord, Vals<0, 1, 2>{});
}

#if RT_KERNEL_PART == 0
int launch_trace(const LaunchParams& p, bool generic_pow, bool stats, void* stream) {
    if (p.local_rows <= 0 || p.W <= 0) return (int)hipSuccess;
    TraceVariant v;
    if (!pick_trace_variant(p, generic_pow, stats, &v)) return (int)hipErrorInvalidValue;
    dim3 grid, block;
    trace_grid(p, v, &grid, &block);
    const int part = trace_mode_part(v.mode);
    bool ok = false;
    if (part == 0) ok = launch_trace_part<0>(v, p, grid, block, (hipStream_t)stream);
#if RT_KERNEL_PARTS > 1
    if (part == 1) ok = launch_trace_part<1>(v, p, grid, block, (hipStream_t)stream);
    if (part == 2) ok = launch_trace_part<2>(v, p, grid, block, (hipStream_t)stream);
    if (part == 3) ok = launch_trace_part<3>(v, p, grid, block, (hipStream_t)stream);
#endif
    // (pick_trace_variant returns built descriptors only: an unbuilt one is an error, not a kernel)
    if (!ok) return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

int launch_debug_segments(const LaunchParams& p, int stride, DevSegment* out, int capacity, unsigned* count,
                          void* stream) {
    const long long n = ((long long)p.W * p.H + stride - 1) / stride;
    if (n <= 0) return (int)hipSuccess;
    hipLaunchKernelGGL(debug_segments_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p,
                       stride, out, capacity, count);
    return (int)hipGetLastError();
}

int launch_hits(const LaunchParams& p, const HitOut& out, void* stream) {
    if (p.W <= 0 || p.H <= 0) return (int)hipSuccess;
    const dim3 grid((unsigned)((p.W + TILE_W - 1) / TILE_W), (unsigned)((p.H + TILE_H - 1) / TILE_H),
                    (unsigned)(p.n_frames > 1 ? p.n_frames : 1)), block(WG_THREADS);
    if (p.views == nullptr) hipLaunchKernelGGL(hits_kernel<VIEW_ARGS>, grid, block, 0, (hipStream_t)stream, p, out);
    else if (p.scene_stride == 0) hipLaunchKernelGGL(hits_kernel<VIEW_PATH>, grid, block, 0, (hipStream_t)stream, p, out);
    else hipLaunchKernelGGL(hits_kernel<VIEW_ANIM>, grid, block, 0, (hipStream_t)stream, p, out);
    return (int)hipGetLastError();
}

int launch_pick(const LaunchParams& p, int x, int y, float lx, float ly, DevPick* out, void* stream) {
    hipLaunchKernelGGL(pick_kernel, dim3(1), dim3(WG_THREADS), 0, (hipStream_t)stream, p, x, y, lx, ly, out);
    return (int)hipGetLastError();
}

int launch_scatter_gathered(const unsigned char* g, size_t slot_bytes, int fmt, int32_t* frame, int W, int H,
                            int band_rows, int world, void* stream) {
    const size_t total = (size_t)W * (size_t)H;
    if (total == 0) return (int)hipSuccess;
    size_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(scatter_gathered_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g,
                       slot_bytes, fmt, frame, W, H, band_rows, world);
    return (int)hipGetLastError();
}

int launch_band_copy(const CopyJob& job, void* stream) {
    if (job.words == 0) return (int)hipSuccess;
    const unsigned long long chunks = (job.words + 3) / 4;
    const unsigned wg = (unsigned)min((unsigned long long)COPY_WAVES, (chunks + 63) / 64);
    hipLaunchKernelGGL(band_copy_kernel, dim3(wg), dim3(64), 0, (hipStream_t)stream, job);
    return (int)hipGetLastError();
}

int launch_scatter_bands(const int32_t* bands, int32_t* frame, int W, int H, int band_rows, int band_first,
                         int band_step, int n_bands, void* stream) {
    const size_t total = (size_t)n_bands * band_rows * W;
    if (total == 0) return (int)hipSuccess;
    size_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(scatter_bands_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bands, frame,
                       W, H, band_rows, band_first, band_step, n_bands * band_rows);
    return (int)hipGetLastError();
}

#endif  // RT_KERNEL_PART == 0

}  // namespace rtk
