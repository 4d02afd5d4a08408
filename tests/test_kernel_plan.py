"""The render kernel choice (csrc/kernel_plan.h plan_kernel) on the host build of the header: which megakernel
class, variant bits, fan bits, frame-stack bytes and kernel name a launch gets, for a fixed grid of scenes, renders and
options (tests/cpp/kernel_plan_dump.cpp), against tests/golden/kernel_plan.txt.gz.

The golden was printed by the same dump program compiled against the predicates the header replaced (fans_pay,
lite_eligible, use_df, opaque_path, split_ok, opaque_variant, tree_path, tree_variant, variant_of, shape_options' fan
lines and launch_render's frame-size branch, copied verbatim behind stub rt_ctx / KParams structs), so a line that
differs is a render that would run another kernel than before the choice moved into the header.

The grid is a union of crosses, not one cross of every axis (that is 10^8 lines).  What is pruned, and why it cannot
interact (each by the code the golden came from):
  * frames' worth of pixels {1, 5.99, 6, 12.99, 13, 64} and max_level {0, 15}: read only once the class is chosen (the
    opaque / tree build and the frame bytes; split_ok's max_level < 16 holds for both), so they are crossed with
    every RT_OPT_OPAQUE / RT_OPT_TREE value, one or two lights, scene size and COUNT on scenes of those two classes
    (grids E, F), and held at one single frame elsewhere; the general kernels read only n_views > 1 (grids C, D).
  * RT_OPT_OPAQUE 2..7 and RT_OPT_TREE 1..5: the eligibility rules read RT_OPT_OPAQUE's sign and zero and
    RT_OPT_TREE's zero only, so the class grids (A, B) use {-1, 0, 1} and {-1, 0}; every value is in E / F.
  * textures, glossy lobes (glossy_n 4 with a glossy material) and RT_OPT_VARIANT >= 0: each alone rules out the opaque
    and tree kernels before their options, the materials or the light count are read, so grid C crosses them with
    size, forced class, fans, light samples, batch or frame and pixel / ray work only.  The two lobe-free spellings
    (glossy_n 4 without a glossy material, glossy_n 1 with one) equal glossy_n 1: crossed with RT_OPT_VARIANT -1.
  * COUNT: names the build (and keeps the texture code), chooses nothing: grids D, E, F.
  * df_ok 0: the whole-traversal kernel before anything else is read: grid B (with all sizes and forced classes).
  * the 5 x 5 spherical x plane sample counts: fully crossed in grid A (every size, forced class, eligibility option,
    fans on / off, opaque or not, one or two lights, pixels or rays); B and C use one light below, in and above the
    fan range."""
import gzip
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raytracer-group27_amd", "csrc")
DUMP = os.path.join(REPO, "tests", "cpp", "kernel_plan_dump.cpp")


def build_dump(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "kernel_plan_dump" + ("_san" if extra else ""))
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, DUMP, "-o", exe], check=True)
    return exe


def plan_of(exe, **inputs):
    """The dump program's line for one input: (kernel name, dict of the plan's other fields)."""
    line = subprocess.run([exe] + [f"{k}={int(v)}" for k, v in inputs.items()], capture_output=True, text=True,
                          check=True).stdout.strip()
    f = line.split("|")[1].split(None, 8)
    keys = ("cls", "variant", "count", "tex", "opaque_pixels", "pixels", "fan", "frame_bytes")
    return f[8], dict(zip(keys, map(int, f[:8])))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("kernel_plan"))


def test_plan_grid_matches_previous_predicates(dump, golden_dir):
    got = subprocess.run([dump], capture_output=True, text=True, check=True).stdout.splitlines()
    with gzip.open(os.path.join(golden_dir, "kernel_plan.txt.gz"), "rt") as f:
        want = f.read().splitlines()
    assert len(got) == len(want)
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, (len(bad), bad[:3])


# the shipped defaults' kernels as BENCH_r06.json and profiles/r06/ record them (1920x1080 frames in bands of 8 rows)
C3 = dict(ntri=800000, all_opaque=1, npl=1, max_level=4)
C4 = dict(ntri=800000, all_opaque=1, npl=0, nsl=1, sl_m=3, sl_n=21, max_level=0)  # sphere_light_ray_count 64: 1 + 3 * 21
C5 = dict(ntri=36, all_opaque=0, npl=0, nplane=3, plane_k=8, max_level=8, H=2160, n_local_bands=270)


@pytest.mark.parametrize("inputs,name", [
    (dict(C3, n_views=64), "rt::persistent_opaque_kernel<false, 646>"),
    (dict(C3, n_views=1), "rt::persistent_opaque_kernel<false, 146>"),
    (dict(C4, n_views=16), "rt::persistent_tree_kernel<false, 18>"),
    (dict(C4, n_views=1), "rt::persistent_tree_kernel<false, 10>"),
    (dict(C5, n_views=1), "rt::persistent_tree_kernel<false, 10>"),
], ids=["C3x64", "C3", "C4x16", "C4", "C5"])
def test_shipped_default_kernel_names(dump, inputs, name):
    assert plan_of(dump, **inputs)[0] == name


@pytest.mark.gpu
def test_small_scene_runs_the_planned_builds(R, dump):
    """Every opaque build and the tree builds on the small dragon proxy (32 000 triangles, one point light: SPLIT
    eligible) at 64x36: each launch names the kernel the host plan prints for the same inputs, and all images are
    bit-equal.  The 16-view default is the small-shape route to the 5-wave opaque build (17.8 frames' worth >= 13)."""
    import variants as V

    u, v = 200, 80
    scene, prm, _, _, _ = R.build_config("C3", dragon_uv=(u, v))
    W, H = 64, 36
    facts = dict(ntri=2 * u * v, all_opaque=1, npl=1, glossy_n=prm.glossy_ray_count, max_level=prm.max_reflection_level,
                 H=H, band_rows=8, n_local_bands=(H + 7) // 8)
    ctx = R.Context(scene)
    try:
        cams = R.turntable_cameras(16, R.aspect_of(W, H))
        first = None
        for opaque in range(-1, 8):
            with V.options(R, ctx, {R.OPT_OPAQUE: opaque}):
                img, st = ctx.render(cams[0], prm, W, H)
            assert st.kernel_name == plan_of(dump, **facts, n_views=1, opt_opaque=opaque)[0], opaque
            if first is None:
                first = img
            assert img.tobytes() == first.tobytes(), opaque
        batch = None
        for opaque, tree in ((-1, -1), (0, -1), (0, 4), (0, 5)):
            with V.options(R, ctx, {R.OPT_OPAQUE: opaque, R.OPT_TREE: tree}):
                views, st = ctx.render_views(cams, prm, W, H)
            assert st.kernel_name == plan_of(dump, **facts, n_views=16, opt_opaque=opaque, opt_tree=tree)[0], (opaque, tree)
            if batch is None:
                batch = views
                assert st.kernel_name == "rt::persistent_opaque_kernel<false, 646>"
            else:
                assert "persistent_tree_kernel" in st.kernel_name
            assert views.tobytes() == batch.tobytes(), (opaque, tree)
        assert batch[0].tobytes() == first.tobytes()
    finally:
        ctx.close()
