// rt_texture_view.hip -- the texture-debug view, ViewMode::Textures (included by rt_runtime.hip after
// rt_megakernel.hip, whose traversal and job -> pixel map it uses).
//
// renderRayTracing(..., textureDebugging = true) (src/main.cpp:355-356,752-761) colours every pixel with
// getFinalColorNoRayTracingJustTextures (src/main.cpp:76-109): one camera ray, its first hit, and
//   no hit                              (0, 0, 0)
//   a triangle whose mesh has a texture mat.kdTexture->getPixel(texCoord, lod), lod from the camera ray's
//                                       transferred differentials for the three mip filters, else 0
//   anything else                       (1, 1, 1)
// The view reads mat.kdTexture without looking at useTextures, so it samples whenever the context holds
// textures, whatever rt_params.use_textures says (the host sets S.tex_on from the texture count alone).
// Spheres are white: computeLevelOfDetails declines them (it needs a triangle's vertices and texture
// coordinates) and the product binds textures to triangles only (rt_material.texture of a mesh; a sphere's
// material never carries one).
//
// No render kernel serves this: every one of them is a shading state machine (Lane / Frame state, the light
// loop, a frame stack).  This kernel is the state machine's first step alone -- gen_ray_view, trace_query8,
// surface(shade, primary) -- one wave per 8x8 tile, its LDS the traversal stack and nothing else.  The same
// pass gives the first hit's primitive id and depth (picking, compositing) through two optional outputs.
//
// Tiles: block b works for XCD b % 8 (blocks go round the XCDs) and takes tile b / 8 of that XCD's job range,
// the ranges of the render kernels' job heads (xq_lo): a horizontal band of every view per XCD, so an XCD's L2
// holds that band's part of the scene.  Within the range the tiles run in job_pixel's tile order with no
// interleave (the opaque kernel's batch default): a wave's 64 rays are one 8x8 tile.

namespace rt {

// the kernel's second argument: the three outputs in the Screen::setPixel layout (view v's pixel (x, y) at
// v*W*H + (H-1-y)*W + x; rgb three floats per pixel); prim and t may be null
struct TexViewOut {
    float* rgb;
    int* prim;
    float* t;
};

__device__ __forceinline__ const TexViewOut& texture_view_out(const void* ka) {
    constexpr size_t off = (sizeof(KParams) + alignof(TexViewOut) - 1) / alignof(TexViewOut) * alignof(TexViewOut);
    return *(const TexViewOut*)(uniform_kernarg(ka) + off);
}

// blocks of a launch over view_jobs / 64 tiles per view: 8 XCD ranges of at most ceil(tiles / 8) tiles a view
__host__ __device__ __forceinline__ long long texture_view_grid(int tiles, int n_views) {
    return 8ll * n_views * ((tiles + 7) / 8);
}

// Waves per SIMD: the compiler's kernel-resource-usage remark for gfx950 reports 102 VGPRs, 90 SGPRs and no
// scratch for both instances (the peak is trace_query8's own: two nodes' planes in flight); 102 VGPRs allow 4
// waves (512 / 104), and a bound of 5 (96 VGPRs) spills 24 B per lane, so 4 it is ("The
// texture-debug view").  STK = the traversal stack's entries per lane: RT_STACK8 where the BVH8 depth fits
// (rt_ctx::df_ok; 3 KB of LDS a wave), else RT_STACK_SIZE (10 KB: LDS then holds 4 waves as well)
#ifndef RT_TV_WAVES
#define RT_TV_WAVES 4
#endif
template <int STK>
__global__ __launch_bounds__(64, RT_TV_WAVES) void texture_view_kernel(KParams, TexViewOut) {
    const void* ka = (const void*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ int stack_lds[STK * RT_WAVE];
    const KParams& P = kernel_params(ka);
    const DevScene& S = P.S;
    // the block's tile (wave-uniform)
    const int nt = P.view_jobs >> 6;
    const int x = (int)(blockIdx.x & 7u), k = (int)(blockIdx.x >> 3);
    const int lo = P.n_views * ((x * nt) >> 3), hi = P.n_views * (((x + 1) * nt) >> 3);
    if (k >= hi - lo) return;
    const int job0 = (lo + k) << 6;
    int view = 0;
    view_job(P, job0, view);
    uint32_t rpix = 0u;
    int out_row = 0;
    if (!job_pixel(P, job0 + (int)threadIdx.x, rpix, out_row)) return;  // a padding pixel of a partial tile or band
    // the pixel -> NDC rule of the render loop (src/main.cpp:350-354); no AA, no multi-sampling in this view
    const int py = (int)(rpix / (uint32_t)P.W);
    const int px = (int)(rpix - (uint32_t)py * (uint32_t)P.W);
    const float ndx = (float)px / (float)P.W * 2.0f - 1.0f;
    const float ndy = (float)py / (float)P.H * 2.0f - 1.0f;
    v3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 0.0f};
    gen_ray_view(P, view, ndx, ndy, o, d);
    Best b;
    b.t = FLT_MAX;
    b.key = -1;
    b.rec = RT_NO_HIT;
    Cnt cnt{};
    const bool hit = trace_query8<false, 8>(S, o, d, FLT_MAX, 0.0f, P.use_bvh != 0, false, b, stack_lds + threadIdx.x, cnt);
    v3 rgb{0.0f, 0.0f, 0.0f};
    int prim = -1;
    float t = FLT_MAX;
    if (hit) {
        // surface(shade, primary): barycentrics, uv and, with S.tex_on, the kd of a textured mesh from its texture
        // at the camera ray's level of detail
        const Surf s = surface(S, o, d, b, true, true);
        prim = s.prim;
        t = b.t;
        const bool textured = s.is_tri && S.tex_on && S.mat_tex[s.mesh] >= 0;
        rgb = textured ? v3{s.m.kd[0], s.m.kd[1], s.m.kd[2]} : v3{1.0f, 1.0f, 1.0f};
    }
    // Screen::setPixel's place (src/screen.cpp:32-38): out_row = view * H + (H - 1 - y); rgb goes out before prim and t
    const TexViewOut& O = texture_view_out(ka);
    const size_t at = (size_t)out_row * (size_t)P.W + (size_t)px;
    float* dst = O.rgb + at * 3;
    dst[0] = rgb.x;
    dst[1] = rgb.y;
    dst[2] = rgb.z;
    if (O.prim) O.prim[at] = prim;
    if (O.t) O.t[at] = t;
}

}  // namespace rt
