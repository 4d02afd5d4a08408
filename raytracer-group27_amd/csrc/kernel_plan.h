// kernel_plan.h -- which megakernel build a render runs: the variant bits, the named builds, the thresholds and the one
// function that chooses (plan_kernel).  Host only, no HIP header: rt_runtime.hip computes a KernelPlan once per launch and
// every consumer reads it (shape_options, the wavefront test, the frame stacks, the persistent grid, the launch);
// tests/test_kernel_plan.py pins the choice on the host build of this header.
#pragma once

#include <algorithm>
#include <cstdio>

#include "../../include/rt_amd.h"

// Kernel variants (compile-time): bit 0 RT_V_CALL = state machine (and drain lane groups) out of line;
// bit 1 RT_V_NOPF = no node prefetch in the dynamic-fetch traversal; bit 2 RT_V_NOCOOP = no drain lane
// groups; bit 4 RT_V_W4 = compiled for 4 waves per SIMD (128 VGPRs) instead of 2 (256); bit 8 RT_V_FAN =
// light-sample fans.  Every variant renders the same bits; they differ in registers, spills and occupancy.
#define RT_V_CALL 1
#define RT_V_NOPF 2
#define RT_V_NOCOOP 4
#define RT_V_W4 16  // compiled for 4 waves per SIMD (128 VGPRs)
#define RT_V_FAN 256  // dynamic fetch: the spherical-light sample fans compiled in (P.fan)

#define RT_V_W3 8    // compiled for 3 waves per SIMD (168 VGPRs)
#define RT_V_REVISIT 32  // opaque / tree kernels: the re-visit group stack of the other kernels (A/B), not DIRECT
#define RT_V_CHK 64      // tree kernel: the checked build (indices validated and reported, chk_report)
#define RT_V_SPLIT 128   // opaque kernel: a node's shadow segment traced beside its mirror child (split_node)
#define RT_V_W5 512      // opaque kernel: compiled for 5 waves per SIMD (96 VGPRs; with NOCOOP its LDS fits 20 blocks)
#define RT_V_WAVES(V) (((V) & RT_V_W5) ? 5 : ((V) & RT_V_W4) ? 4 : ((V) & RT_V_W3) ? 3 : 2)

// dynamic-fetch kernel below this many triangles only when forced (RT_OPT_KERNEL): a query on a small
// scene is a handful of node visits and the per-step refill bookkeeping does not pay (measured on
// MI355X, DESIGN.md section 6: C1/C2/C5 vs C3/C4)
#define RT_DF_MIN_TRIANGLES 65536

// Kernel variants compiled (RT_V_*).  The dynamic-fetch class ships two, chosen by
// render shape: view batches run the lean 4-waves-per-SIMD variant (state machine
// out of line, no node prefetch, no drain lane groups: C3 16 views 0.785 ms/frame vs 0.907 at 3 waves,
// 0.99 at 5, 1.11 for the 2-wave frame variant; C4 14.96 vs 17.8 / 18.7 / 24.1 ms/frame), single
// frames the 2-wave variant with the drain lane groups (their tail dominates: C3 2.16-2.19 vs
// 2.29-2.67 ms).  The whole-traversal class (small scenes) keeps the inline 2-wave variant (C2 0.76 vs
// 0.81 ms, C5 742 vs 804 ms).  The alternates are kept for A/B measurement (RT_OPT_VARIANT); all
// render identical bits.
#define RT_DF_BATCH (RT_V_CALL | RT_V_NOPF | RT_V_NOCOOP | RT_V_W4)
#define RT_DF_FRAME 0
#define RT_WT_DEFAULT 0
// the one A/B alternate: the batch variant with the drain lane groups, called out of line
#define RT_DF_ALT (RT_V_CALL | RT_V_NOPF | RT_V_W4)

// the opaque-scene kernel (rt_megakernel.hip persistent_opaque_kernel): 4 waves per SIMD for batches and single frames
// (round 4, with the direct group stack and the leaf bound 2: C3 frame 1.237 vs 1.246 ms at 3 waves,
// profiles/r04/ab_r04g_refill.log), with SPLIT (a node's shadow segment traced beside its mirror child,
// rt_megakernel.hip split_node) where the scene has one light (point or spot) and at most 16 levels (the LDS result
// bits): its lane keeps 3 dwords between phases, so the 4-wave build has no spills (31 VGPRs before) -- C3 64-view
// batch 0.376-0.378 -> 0.373 ms/frame, frame 1.045-1.074 -> 0.95-0.97 ms (profiles/r05/ab_r05m.log, ab_r05n.log).
// RT_OPT_OPAQUE 1 the 4-wave build without SPLIT, 2 the 3-wave build, 3 the 4-wave re-visit A/B, 4 / 5 SPLIT at 4 / 3
// waves, 6 / 7 SPLIT without the drain lane groups at 5 / 4 waves (A/Bs: 0.388 / 0.377 ms/frame, frames 1.26 / 1.14 ms)
#define RT_OPAQUE_V (RT_V_W4 | RT_V_NOPF)
#define RT_OPAQUE_V3 (RT_V_W3 | RT_V_NOPF)
#define RT_OPAQUE_V5S (RT_V_W5 | RT_V_NOPF | RT_V_NOCOOP | RT_V_SPLIT)   // 5 waves, no drain lane groups
#define RT_OPAQUE_V4SN (RT_V_W4 | RT_V_NOPF | RT_V_NOCOOP | RT_V_SPLIT)  // A/B: 4 waves, no drain lane groups
// launches of at least RT_V5_MIN_FRAMES frames' worth of pixels with SPLIT: 5 waves per SIMD without the drain
// lane groups (round 6, every automatic variable defined: 20 spilled VGPRs instead of 33; C3 64-view batch 0.372
// -> 0.352 ms/frame, profiles/r06/ab_r06m.log).  Its per-launch drain is longer: the views fit is 0.334 + 1.128 /
// frames ms/frame against the 4-wave build's 0.3625 + 0.766 / frames (views_r06.log, views_r05fb.log), so the
// builds cross at ~13 frames' worth -- a band-split launch at N = 8 GPUs (64 views x 1/8 of each frame) keeps
// the 4-wave build with the lane groups, and so do single frames (1.13 vs 0.92 ms without them)
#define RT_V5_MIN_FRAMES 13.0

// the recursion-tree kernel (rt_megakernel.hip persistent_tree_kernel): 4 / 3 waves per SIMD
// View batches run the 4-wave build, single frames the 3-wave one (round 6: C4 16-view batch 6.77-6.82 -> 6.09-6.13
// ms/frame, C4 frame 6.92-6.95 vs 7.32-7.57 ms at 4 waves; profiles/r06/ab_r06k*.log).  The 4-wave build faulted
// in rounds 4-5 when compiled with undef values in its IR; with every automatic variable defined (build.py
// HIP_FLAGS) it runs every size bit-identically.
#define RT_TREE_V3 (RT_V_W3 | RT_V_NOPF)
#define RT_TREE_VR (RT_V_W3 | RT_V_NOPF | RT_V_REVISIT)  // A/B: the re-visit group stack (RT_OPT_TREE 1)
// developer diagnosis of the 4-wave build's fault (RT_OPT_TREE 3): that build with every index checked (RT_V_CHK)
#define RT_TREE_V4C (RT_V_W4 | RT_V_NOPF | RT_V_CHK)
#define RT_TREE_V4 (RT_V_W4 | RT_V_NOPF)  // launches of >= 6 frames (RT_OPT_TREE 4 forces it, 5 the 3-wave build)
// by frames' worth of pixels per launch, as the opaque kernel's builds: C4 16 views over 8 / 4 / 2 GPUs' band
// shares (2 / 4 / 8 frames) 2.17 / 2.53 / 3.96 ms/frame at 3 waves vs 2.29 / 2.57 / 3.62 at 4; C2 64 views
// over 8 GPUs (8 frames) 0.017 vs 0.016 (profiles/r06/ab_r06v_*.log)
#define RT_TREE_V4_MIN_FRAMES 6.0

namespace rt {

enum KernelClass { KC_WHOLE = 0, KC_DF = 1, KC_OPAQUE = 2, KC_TREE = 3 };  // persistent_{,df_,opaque_,tree_}kernel

// what the choice reads: facts of the scene, of the render, and the context's options
struct PlanInput {
    int ntri;
    bool df_ok, glossy_material;
    int all_opaque, npl, nsl, nspot, nplane;
    int tex_on, glossy_n, sl_m, sl_n, plane_k, max_level, n_views, n_local_bands, band_rows, H;
    bool pixels;  // pixel work (a render), not rt_shade's explicit rays
    bool count;   // the counting build of the same kernel
    int opt_kernel, opt_variant, opt_opaque, opt_tree, opt_fan;
};

struct KernelPlan {
    int cls;             // KernelClass
    int variant;         // RT_V_* bits
    bool count, tex;     // the build's COUNT / TEX (TEX: the whole-traversal and dynamic-fetch classes only)
    bool opaque_pixels;  // the opaque kernel draws this scene's pixels (whether or not this launch is pixel work)
    bool pixels;
    int fan;             // KParams::fan
    int frame_bytes;     // frame stack per resident lane
    char name[64];       // rt_ctx::last_kernel: the name rocprofv3 lists for this launch (bench.py's roofline.kernel)
    bool df() const { return cls != KC_WHOLE; }  // the dynamic-fetch traversal (every class but whole-traversal)
};

inline KernelPlan plan_kernel(const PlanInput& in) {
    const int sph_n = in.nsl > 0 ? 1 + in.sl_m * in.sl_n : 0, plane_n = in.nplane > 0 ? in.plane_k * in.plane_k : 0;
    // lights whose samples the dynamic-fetch kernel traces as wave-shared fans pay for that kernel on a
    // small scene too: at least 16 and at most 64 samples per spherical or plane light (C5, 3 plane lights of
    // 8 x 8 with a glass sphere: single frame 813 -> 351 ms, 4-view batch 218 -> 204 ms/frame)
    const bool fans_pay = in.opt_fan && ((sph_n >= 16 && sph_n <= 64) || (plane_n >= 16 && plane_n <= 64));
    // the opaque-scene and the recursion-tree kernel draw scenes without textures and without glossy lobes
    // (glossy_ray_count 1, or no glossy material); any RT_OPT_VARIANT choice selects the general kernels instead
    const bool lite = in.opt_variant < 0 && !in.tex_on && (in.glossy_n == 1 || !in.glossy_material);
    // ... the opaque one (RT_OPT_OPAQUE 0: never): all materials opaque, lit by point and spot lights only
    const bool opaque_ok = lite && in.opt_opaque != 0 && in.all_opaque && in.nsl == 0 && in.nplane == 0;
    // ... the tree one (RT_OPT_TREE 0: never): spherical and plane lights fit one fan (<= 64 samples; fans on)
    const bool tree_ok = lite && in.opt_tree != 0 && in.opt_fan && sph_n <= 64 && plane_n <= 64 &&
                         (long long)in.npl + in.nsl + in.nspot + in.nplane < 65536;  // TreeLane::li
    // the dynamic-fetch traversal for large scenes, sample-heavy lights and every scene the opaque or recursion-tree
    // kernel draws (round 6: C2 64-view batch 0.268 -> 0.109 ms/frame, frame 0.626 -> 0.38-0.50 ms;
    // profiles/r06/ab_r06e.log); whole-traversal refill for the small scenes left (textures, glossy lobes)
    const bool df = in.df_ok && in.opt_kernel != RT_KERNEL_WHOLE_TRAVERSAL &&
                    (in.opt_kernel == RT_KERNEL_DYNAMIC_FETCH || in.ntri >= RT_DF_MIN_TRIANGLES || fans_pay || opaque_ok ||
                     tree_ok);
    const bool split_ok = in.npl + in.nspot == 1 && in.max_level < 16;
    // small scenes with more than one light: the recursion-tree kernel draws them faster -- C2 64-view batch 0.104
    // vs 0.100 ms/frame, frame 0.459 vs 0.376 ms, profiles/r06/ab_r06m.log -- unless RT_OPT_OPAQUE asks for the opaque one.
    // KNOWN DISAGREEMENT: opaque_ok has already chosen `df` for such a scene, so where the tree
    // kernel cannot take it either (RT_OPT_TREE 0 or RT_OPT_FAN 0) it falls to the general dynamic-fetch kernel, not
    // to the whole-traversal one.  Kept as it behaves.
    const bool small_multi_light = in.opt_opaque < 0 && in.ntri < RT_DF_MIN_TRIANGLES && !split_ok;
    const bool opaque_pixels = df && opaque_ok && !small_multi_light;
    const bool tree_pixels = df && tree_ok && !opaque_pixels;

    KernelPlan p{};
    p.count = in.count;
    p.pixels = in.pixels;
    p.opaque_pixels = opaque_pixels;
    p.cls = in.pixels && opaque_pixels ? KC_OPAQUE : in.pixels && tree_pixels ? KC_TREE : df ? KC_DF : KC_WHOLE;
    // spherical lights (bit 0) and plane lights (bit 1) as wave-shared fans (rt_megakernel.hip FanTable):
    // dynamic-fetch traversal, at most 64 samples per light (one mask)
    p.fan = (in.opt_fan && df) ? ((in.nsl > 0 && sph_n <= 64 ? 1 : 0) | (in.nplane > 0 && plane_n <= 64 ? 2 : 0)) : 0;
    if (in.opt_variant >= 0 && in.opt_variant != RT_DF_BATCH) p.fan = 0;  // fans are compiled into that variant only
    const double frames = (double)std::max(1, in.n_views) * in.n_local_bands * in.band_rows / std::max(1, in.H);
    const char* kernel = "persistent_kernel";
    if (p.cls == KC_OPAQUE) {
        kernel = "persistent_opaque_kernel";
        const int o = in.opt_opaque;
        p.variant = o == -1 && frames >= RT_V5_MIN_FRAMES && split_ok ? RT_OPAQUE_V5S
                    : o == 2                                         ? RT_OPAQUE_V3
                    : o == 3                                         ? (RT_OPAQUE_V | RT_V_REVISIT)
                    : o == 1 || !split_ok                            ? RT_OPAQUE_V
                    : o == 6                                         ? RT_OPAQUE_V5S
                    : o == 7                                         ? RT_OPAQUE_V4SN
                                                                     : ((o == 5 ? RT_OPAQUE_V3 : RT_OPAQUE_V) | RT_V_SPLIT);
        // SPLIT: max_level + 1 node frames of 32 B per resident lane
        if (p.variant & RT_V_SPLIT) p.frame_bytes = 32 * (in.max_level + 1);
    } else if (p.cls == KC_TREE) {
        kernel = "persistent_tree_kernel";
        const int t = in.opt_tree;
        p.variant = t == 1   ? RT_TREE_VR
                    : t == 3 ? RT_TREE_V4C
                    : t == 4 ? RT_TREE_V4
                    : t == 5 ? RT_TREE_V3
                             : (frames >= RT_TREE_V4_MIN_FRAMES ? RT_TREE_V4 : RT_TREE_V3);
        // the tree kernel's frame stacks: max_level frames of 48 B per resident lane
        p.frame_bytes = 48 * std::max(1, in.max_level);
    } else if (p.cls == KC_DF) {
        kernel = "persistent_df_kernel";
        // by render shape: view batches and sample-fan renders run the lean 4-wave variant (C4 single frame
        // with fans: 27.1 vs 30.3 ms), other single frames the 2-wave variant with the drain lane groups
        const int v = in.opt_variant >= 0 ? in.opt_variant : ((in.n_views > 1 || p.fan) ? RT_DF_BATCH : RT_DF_FRAME);
        p.variant = p.fan ? (v | RT_V_FAN) : v;
    } else {
        p.variant = in.opt_variant >= 0 ? in.opt_variant : RT_WT_DEFAULT;
    }
    if (p.cls == KC_OPAQUE || p.cls == KC_TREE) {
        std::snprintf(p.name, sizeof(p.name), "rt::%s<%s, %d>", kernel, p.count ? "true" : "false", p.variant);
    } else {
        p.tex = in.count || in.tex_on;  // counting builds keep the texture code (one instance each)
        std::snprintf(p.name, sizeof(p.name), "rt::%s<%s, %s, %d>", kernel, p.count ? "true" : "false",
                      p.tex ? "true" : "false", p.variant);
    }
    return p;
}

}  // namespace rt
