// Host build of csrc/kernel_plan.h: prints one line per input, the inputs and then the whole plan
// (tests/test_kernel_plan.py).  Without arguments it walks the fixed grid below; with name=value arguments it prints
// the plan of that one input (the others at their defaults: a large one-light opaque scene, a 1080-row frame).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "kernel_plan.h"

using rt::PlanInput;

#define PLAN_FIELDS(X)                                                                                              \
    X(ntri) X(df_ok) X(glossy_material) X(all_opaque) X(npl) X(nsl) X(nspot) X(nplane) X(tex_on) X(glossy_n) X(sl_m) \
    X(sl_n) X(plane_k) X(max_level) X(n_views) X(n_local_bands) X(band_rows) X(H) X(pixels) X(count) X(opt_kernel)   \
    X(opt_variant) X(opt_opaque) X(opt_tree) X(opt_fan)

static PlanInput base() {
    PlanInput in{};
    in.ntri = 65536;
    in.df_ok = true;
    in.all_opaque = 1;
    in.npl = 1;
    in.glossy_n = 1;
    in.sl_m = in.sl_n = 1;
    in.plane_k = 3;
    in.n_views = 1;
    in.n_local_bands = 135;
    in.band_rows = 8;
    in.H = 1080;
    in.pixels = true;
    in.opt_kernel = RT_KERNEL_AUTO;
    in.opt_variant = in.opt_opaque = in.opt_tree = -1;
    in.opt_fan = 1;
    return in;
}

static void emit(const PlanInput& in) {
    const rt::KernelPlan p = rt::plan_kernel(in);
#define X(f) std::printf("%d ", (int)in.f);
    PLAN_FIELDS(X)
#undef X
    std::printf("| %d %d %d %d %d %d %d %d %s\n", p.cls, p.variant, (int)p.count, (int)p.tex, (int)p.opaque_pixels,
                (int)p.pixels, p.fan, p.frame_bytes, p.name);
}

// the axes' values
static const int NTRI[] = {1000, 65535, 65536};
static const int KERNELS[] = {RT_KERNEL_AUTO, RT_KERNEL_WHOLE_TRAVERSAL, RT_KERNEL_DYNAMIC_FETCH};
static const int VARIANTS[] = {-1, 0, RT_DF_BATCH, RT_DF_ALT};
struct Sph { int nsl, m, n; };  // a spherical light of 1 + m * n samples: none, 5, 16, 64, 65
static const Sph SPH[] = {{0, 1, 1}, {1, 1, 4}, {1, 3, 5}, {1, 7, 9}, {1, 8, 8}};
struct Plane { int nplane, k; };  // a plane light of k * k samples: none, 9, 16, 64, 81
static const Plane PLANE[] = {{0, 3}, {1, 3}, {1, 4}, {1, 8}, {1, 9}};
struct Shape { int n_views, n_local_bands, band_rows, H; };  // frames' worth of pixels: 1, 5.99, 6, 12.99, 13, 64
static const Shape SHAPES[] = {{1, 135, 8, 1080}, {6, 599, 1, 600},    {6, 135, 8, 1080},
                               {13, 1299, 1, 1300}, {13, 135, 8, 1080}, {64, 135, 8, 1080}};
struct Gloss { int glossy_n; bool material; };
static const Gloss GLOSS[] = {{1, false}, {4, true}, {4, false}, {1, true}};

static void set_lights(PlanInput& in, int point_spot, const Sph& s, const Plane& p) {
    in.npl = 1;
    in.nspot = point_spot - 1;
    in.nsl = s.nsl;
    in.sl_m = s.m;
    in.sl_n = s.n;
    in.nplane = p.nplane;
    in.plane_k = p.k;
}
static void set_shape(PlanInput& in, const Shape& s) {
    in.n_views = s.n_views;
    in.n_local_bands = s.n_local_bands;
    in.band_rows = s.band_rows;
    in.H = s.H;
}

// A: which kernel class draws a scene without textures or lobes -- size, forced class, the opaque / tree options'
// eligibility values, fans, materials and every light combination, for pixel and ray work
static void grid_eligibility() {
    PlanInput in = base();
    for (int kernel : KERNELS)
        for (int ntri : NTRI)
            for (int opaque : {-1, 0, 1})
                for (int tree : {-1, 0})
                    for (int fan : {0, 1})
                        for (int all_opaque : {0, 1})
                            for (int ps : {1, 2})
                                for (const Sph& s : SPH)
                                    for (const Plane& p : PLANE)
                                        for (int pixels : {0, 1}) {
                                            in.opt_kernel = kernel;
                                            in.ntri = ntri;
                                            in.opt_opaque = opaque;
                                            in.opt_tree = tree;
                                            in.opt_fan = fan;
                                            in.all_opaque = all_opaque;
                                            set_lights(in, ps, s, p);
                                            in.pixels = pixels != 0;
                                            emit(in);
                                        }
}

// B: the size threshold and the scenes the dynamic-fetch traversal cannot or may not take
static void grid_size_and_class() {
    PlanInput in = base();
    const int lights[][2] = {{0, 0}, {2, 0}, {0, 4}};  // none; a 16-sample spherical light; an 81-sample plane light
    for (int ntri : NTRI)
        for (int kernel : KERNELS)
            for (int df_ok : {0, 1})
                for (int opaque : {-1, 0, 1})
                    for (int tree : {-1, 0})
                        for (int all_opaque : {0, 1})
                            for (int ps : {1, 2})
                                for (const auto& l : lights)
                                    for (int fan : {0, 1})
                                        for (int pixels : {0, 1}) {
                                            in.ntri = ntri;
                                            in.opt_kernel = kernel;
                                            in.df_ok = df_ok != 0;
                                            in.opt_opaque = opaque;
                                            in.opt_tree = tree;
                                            in.all_opaque = all_opaque;
                                            set_lights(in, ps, SPH[l[0]], PLANE[l[1]]);
                                            in.opt_fan = fan;
                                            in.pixels = pixels != 0;
                                            emit(in);
                                        }
}

// C: textures, glossy lobes and RT_OPT_VARIANT choices (the general kernels), by size, class, fans, lights and shape
static void grid_general() {
    PlanInput in = base();
    const int lights[][2] = {{0, 0}, {2, 0}, {0, 4}, {3, 3}};  // none; sph 16; plane 81; sph 64 and plane 64
    for (int variant : VARIANTS)
        for (int tex : {0, 1})
            for (const Gloss& g : GLOSS) {
                if (variant >= 0 && (&g - GLOSS) >= 2) continue;  // the lobe-free spellings: with the shipped variants only
                for (int kernel : KERNELS)
                    for (int ntri : {1000, 65536})
                        for (int fan : {0, 1})
                            for (const auto& l : lights)
                                for (int pixels : {0, 1})
                                    for (int s : {0, 2}) {
                                        in.opt_variant = variant;
                                        in.tex_on = tex;
                                        in.glossy_n = g.glossy_n;
                                        in.glossy_material = g.material;
                                        in.opt_kernel = kernel;
                                        in.ntri = ntri;
                                        in.opt_fan = fan;
                                        set_lights(in, 1, SPH[l[0]], PLANE[l[1]]);
                                        in.pixels = pixels != 0;
                                        set_shape(in, SHAPES[s]);
                                        emit(in);
                                    }
            }
}

// D: the general kernels' counting and textured builds (the instance's name)
static void grid_names() {
    PlanInput in = base();
    for (int count : {0, 1})
        for (int tex : {0, 1})
            for (int variant : VARIANTS)
                for (int kernel : {RT_KERNEL_WHOLE_TRAVERSAL, RT_KERNEL_DYNAMIC_FETCH})
                    for (int s : {0, 2})
                        for (int sph : {0, 2})
                            for (int pixels : {0, 1}) {
                                in.count = count != 0;
                                in.tex_on = tex;
                                in.opt_variant = variant;
                                in.opt_kernel = kernel;
                                set_shape(in, SHAPES[s]);
                                set_lights(in, 1, SPH[sph], PLANE[0]);
                                in.pixels = pixels != 0;
                                emit(in);
                            }
}

// E: the opaque kernel's builds -- every RT_OPT_OPAQUE value by launch size, depth, one or two lights and scene size
static void grid_opaque_builds() {
    PlanInput in = base();
    for (int opaque = -1; opaque <= 7; ++opaque)
        for (int tree : {-1, 0})
            for (const Shape& s : SHAPES)
                for (int max_level : {0, 15})
                    for (int ps : {1, 2})
                        for (int ntri : {1000, 65536})
                            for (int count : {0, 1}) {
                                in.opt_opaque = opaque;
                                in.opt_tree = tree;
                                set_shape(in, s);
                                in.max_level = max_level;
                                set_lights(in, ps, SPH[0], PLANE[0]);
                                in.ntri = ntri;
                                in.count = count != 0;
                                emit(in);
                            }
}

// F: the tree kernel's builds -- every RT_OPT_TREE value by launch size and depth, on a transparent scene, an opaque
// one with a spherical light and an opaque one with two lights (a small one: the tree kernel's by preference)
static void grid_tree_builds() {
    PlanInput in = base();
    const int scenes[][3] = {{0, 1, 0}, {1, 1, 2}, {1, 2, 0}};  // all_opaque, point + spot lights, SPH index
    for (int tree = -1; tree <= 5; ++tree)
        for (int opaque : {-1, 0})
            for (const Shape& s : SHAPES)
                for (int max_level : {0, 15})
                    for (const auto& sc : scenes)
                        for (int ntri : {1000, 65536})
                            for (int count : {0, 1}) {
                                in.opt_tree = tree;
                                in.opt_opaque = opaque;
                                set_shape(in, s);
                                in.max_level = max_level;
                                in.all_opaque = sc[0];
                                set_lights(in, sc[1], SPH[sc[2]], PLANE[0]);
                                in.ntri = ntri;
                                in.count = count != 0;
                                emit(in);
                            }
}

int main(int argc, char** argv) {
    if (argc > 1) {
        PlanInput in = base();
        for (int i = 1; i < argc; ++i) {
            const char* eq = std::strchr(argv[i], '=');
            bool known = false;
#define X(f)                                                                                  \
    if (eq && std::strlen(#f) == (size_t)(eq - argv[i]) && !std::strncmp(argv[i], #f, eq - argv[i])) { \
        in.f = (decltype(in.f))std::atoi(eq + 1);                                             \
        known = true;                                                                         \
    }
            PLAN_FIELDS(X)
#undef X
            if (!known) {
                std::fprintf(stderr, "kernel_plan_dump: unknown input %s\n", argv[i]);
                return 2;
            }
        }
        emit(in);
        return 0;
    }
    grid_eligibility();
    grid_size_and_class();
    grid_general();
    grid_names();
    grid_opaque_builds();
    grid_tree_builds();
    return 0;
}
