"""The GPU scene builder (rt_build.hip) on adversarial geometry and at its size edges, against the
brute-force oracle, which has no acceleration structure to share a bug with.

tests/test_gpu_build.py compares the GPU build with the host build on three clean meshes.  Here both
builds are compared with the oracle on generated scenes (tests/build_cases.py): triangle counts on
both sides of every compile-time boundary of the builder (16, kSmall 512, the 1 024 scan block, the
4 096 chunk / radix tile, 16 384 where the histogram scan first recurses, 65 536 where AUTO switches
over), ties in the reference BVH's sort attribute, exact duplicates, a sheet of zero z extent,
extreme size ratios, spheres among the triangles, zero-area triangles, and the two exits a scene the
GPU build declines takes.

Checks, per scene and build (numbered as in the tests below):
 1. build_info()["gpu"] is as forced;
 2. records sorted by scene index are bit-equal between the builds;
 3. ctx.ref_bvh() equals the oracle's constructBVH: boxes by bytes, the same leaves, each leaf's
    objects in stored order;
 4. ctx.intersect(rays_at(...), use_bvh) for use_bvh 0 and 1 equals the oracle's: hit, t by bytes, and
    normal / hit_point / material_index / prim_id / is_triangle by bytes where the oracle hits.

The conditions that keep check 4 honest (enough hits, enough misses, hits on duplicated triangles,
axis-parallel hits on the sheet, sphere hits) are asserts on the oracle's output alone; the tests not
marked gpu run them, and the generators, without a GPU."""
import numpy as np
import pytest

import build_cases as B
from golden_cases import IMAGES, apply

TOL = 1e-5  # tests/test_gpu_parity.py's bar
SIZES = [16, 17, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16385]

# name -> (generator(out_dir), rays, rays aimed at the pile)
CASES = {f"soup-{n}": (lambda d, n=n: B.soup(n, d), 2048, 0) for n in SIZES}
CASES.update({
    "spheres-16-3": (lambda d: B.with_spheres(16, 3, d), 2048, 0),
    "spheres-4090-7": (lambda d: B.with_spheres(4090, 7, d), 2048, 0),
    "sheet-6000": (lambda d: B.sheet(6000, d), 2048, 0),
    "dupes2-6000": (lambda d: B.dupes(6000, 2, d), 2048, 0),
    "dupes9-6000": (lambda d: B.dupes(6000, 9, d), 2048, 0),
    "spanning-6000": (lambda d: B.spanning(6000, d), 2048, 0),
    "spheres-6000-40": (lambda d: B.with_spheres(6000, 40, d), 2048, 0),
    "soup-70000": (lambda d: B.soup(70000, d), 2048, 0),
    "sheet-70000": (lambda d: B.sheet(70000, d), 2048, 0),
    "spanning-70000": (lambda d: B.spanning(70000, d), 2048, 0),
    "degenerate-6000": (lambda d: B.soup(6000, d, seed=9, degenerate=0.05), 2048, 0),
    "soup-65535": (lambda d: B.soup(65535, d), 1024, 0),
    "soup-65536": (lambda d: B.soup(65536, d), 1024, 0),
    "pile-65536-1024": (lambda d: B.pile(65536, 1024, d), 512, 64),
})
SIZE_CASES = [f"soup-{n}" for n in SIZES] + ["spheres-16-3", "spheres-4090-7"]
SHAPE_CASES = ["sheet-6000", "dupes2-6000", "dupes9-6000", "spanning-6000", "spheres-6000-40", "soup-70000",
               "sheet-70000", "spanning-70000"]


class Case:
    """One generated scene with its rays and the oracle's answers, computed once."""

    def __init__(self, R, O, name, out_dir):
        gen, n, n_pile = CASES[name]
        self.name = name
        self.scene = gen(out_dir)
        self.rays = B.rays_at(self.scene, n, seed=11, n_pile=n_pile)
        self.oracle = O.Oracle(self.scene)
        self.ref = [self.oracle.intersect(self.rays, use_bvh, R.HIT_DTYPE) for use_bvh in (0, 1)]
        for r in self.ref:
            r.setflags(write=False)

    def assert_conditions(self):
        """What the oracle alone must show for the comparison with it to mean something."""
        h = self.ref[0]
        hit = h["hit"] == 1
        n = len(h)
        assert hit.sum() >= 0.4 * n, (self.name, int(hit.sum()), n)
        assert (~hit).sum() >= 0.1 * n, (self.name, int((~hit).sum()), n)
        tri = hit & (h["is_triangle"] == 1)
        if self.name.startswith("dupes"):
            # every triangle of these scenes has an exact duplicate: the key tie-break decides prim_id
            assert (tri & np.isin(h["prim_id"], self.scene.dup_tris)).sum() >= 200, self.name
        if self.name.startswith("sheet"):
            assert (hit & B.axis_parallel(self.rays)).sum() >= 100, self.name
        if self.name.startswith("spheres"):
            assert (hit & (h["is_triangle"] == 0)).sum() >= 50, self.name
        if self.name.startswith("pile"):
            assert len(self.scene.pile_tris) == 1024 and CASES[self.name][2] >= 64


@pytest.fixture(scope="module")
def cases(R, O, tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(R, O, name, tmp_path_factory.mktemp(name.replace("-", "_")))
        return cache[name]

    yield get
    cache.clear()


# ------------------------------------------------------------------------------------------------
# without a GPU: the generators, and the conditions on the oracle alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_alone_meets_the_conditions(cases, name):
    c = cases(name)
    c.assert_conditions()
    rays = c.rays
    n = len(rays)
    assert np.all(rays["t"] == B.FLT_MAX)
    assert np.all(B.axis_parallel(rays)[n // 2 + n // 4:]) and not np.any(B.axis_parallel(rays)[:n // 2])


def test_generators_make_what_they_say(R, tmp_path):
    s = B.sheet(999, tmp_path)
    pos = s.arrays()[0]
    assert pos.shape == (999, 3, 3) and np.all(pos[:, :, 2].view(np.uint32) == 0)  # z = +0.0 exactly
    assert np.any(pos[:, :, 0] == 0) and np.any(pos[:, :, 1] == 0)
    cx = ((pos[:, 0, 0] + pos[:, 1, 0]) + pos[:, 2, 0]) / np.float32(3)
    assert len(np.unique(cx)) < 999 // 8  # whole columns share a centroid x
    for k in (2, 9):
        d = B.dupes(900, k, tmp_path)
        p = d.arrays()[0].reshape(-1, k, 9)
        assert np.all(p.view(np.uint32) == p[:, :1].view(np.uint32)) and len(d.dup_tris) == 900
    sp = B.spanning(500, tmp_path)
    ext = sp.arrays()[0].reshape(-1, 3, 3)
    size = (ext.max(axis=1) - ext.min(axis=1)).max(axis=1)
    assert sp.desc().num_triangles == 500 and size.max() / np.median(size) > 1e4
    ws = B.with_spheres(64, 12, tmp_path)
    d, pos = ws.desc(), ws.arrays()[0]
    cen = ((pos[:, 0] + pos[:, 1]) + pos[:, 2]) / np.float32(3)
    tied = sum(any(np.array_equal(np.float32(list(d.spheres[i].center)), c) for c in cen) for i in range(12))
    assert d.num_spheres == 12 and tied >= 8  # centres equal to triangle centroids on every sort axis
    d = B.with_spheres(64, 20, tmp_path).desc()
    cb = np.array([list(d.spheres[i].center) for i in range(12, 18)], np.float32).view(np.uint32)
    assert [int((cb[i] ^ cb[i + 1]).sum()) for i in (0, 2, 4)] == [0x80000000] * 3  # pairs: +0.0, then -0.0
    pl = B.pile(10, 40, tmp_path)
    p = pl.arrays()[0]
    assert np.all(p[10:].view(np.uint32) == p[10].view(np.uint32)) and list(pl.pile_tris) == list(range(10, 50))
    dg = B.soup(200, tmp_path, seed=9, degenerate=0.05).arrays()[0].astype(np.float64)
    area = np.linalg.norm(np.cross(dg[:, 1] - dg[:, 0], dg[:, 2] - dg[:, 0]), axis=1)
    assert (area == 0).sum() == 10
    assert ws.desc().num_point_lights == 1 and s.desc().num_point_lights == 1


# ------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------
def _ctx(R, scene, mode):
    R.set_build_mode(mode)
    try:
        return R.Context(scene)
    finally:
        R.set_build_mode(R.BUILD_AUTO)


def _by_scene_index(rec):
    idx = rec[:, 13].view(np.int32)
    return rec[np.argsort(idx, kind="stable")]


def _check_intersect(ctx, c, what):
    """Check 4."""
    for use_bvh in (0, 1):
        hits, ref = ctx.intersect(c.rays, use_bvh), c.ref[use_bvh]
        assert np.array_equal(hits["hit"], ref["hit"]), (c.name, what, use_bvh)
        assert hits["t"].tobytes() == ref["t"].tobytes(), (c.name, what, use_bvh)
        h = ref["hit"] == 1
        for f in ("normal", "hit_point", "material_index", "prim_id", "is_triangle"):
            assert hits[f][h].tobytes() == ref[f][h].tobytes(), (c.name, what, use_bvh, f)


def _check_ref_bvh(ctx, c, what):
    """Check 3."""
    boxes, leaf = c.oracle.bvh_nodes()
    b, node_leaf, got = ctx.ref_bvh()
    assert b.tobytes() == boxes.tobytes(), (c.name, what)
    assert np.array_equal(node_leaf >= 0, leaf.astype(bool)), (c.name, what)
    for i in range(len(leaf)):
        assert np.array_equal(got[i], c.oracle.bvh_children(i)), (c.name, what, i)


def _check_builds(R, O, c, render=False, nan_planes=False):
    """Checks 1-4 on the host build and the forced GPU build of one scene; with `render`, one 48x32
    frame at C3's knobs from both builds and from the oracle."""
    c.assert_conditions()
    host, dev = _ctx(R, c.scene, R.BUILD_HOST), _ctx(R, c.scene, R.BUILD_GPU)
    try:
        assert not host.build_info()["gpu"] and dev.build_info()["gpu"]  # 1
        hr = _by_scene_index(host.records()).view(np.uint32)  # 2
        dr = _by_scene_index(dev.records()).view(np.uint32)
        same = hr == dr
        if nan_planes:  # zero-area triangles: plane n and D are NaN; their sign and payload are not compared
            nan = np.isnan(hr.view(np.float32)) & np.isnan(dr.view(np.float32))
            nan[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 13, 14, 15]] = False
            same |= nan
        assert hr.shape == dr.shape and np.all(same), c.name
        for ctx, what in ((host, "host"), (dev, "gpu")):
            _check_ref_bvh(ctx, c, what)  # 3
            _check_intersect(ctx, c, what)  # 4
        if render:
            W, H = 48, 32
            prm = R.params(max_reflection_level=4, glossy_ray_count=1)  # C3's
            look, dist = c.scene.view
            cam = R.camera_from_trackball(look_at=look, distance=dist, aspect=R.aspect_of(W, H))
            img_h, st_h = host.render(cam, prm, W, H)
            img_d, st_d = dev.render(cam, prm, W, H)
            ref, rays = c.oracle.render(prm, W, H, look_at=look, dist=dist)
            assert st_h.rays == rays and st_d.rays == rays, (c.name, st_h.rays, st_d.rays, rays)
            assert np.array_equal(img_h.view(np.uint32), img_d.view(np.uint32)), c.name
            assert float(np.max(np.abs(img_h - ref))) <= TOL, c.name
            assert float(np.max(np.abs(img_d - ref))) <= TOL, c.name
        return hr, dr
    finally:
        host.close()
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SIZE_CASES)
def test_size_edges(R, O, cases, name):
    """a. Triangle (and object) counts on both sides of every boundary of the builder."""
    _check_builds(R, O, cases(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPE_CASES)
def test_shapes(R, O, cases, name):
    """b. Adversarial geometry at ~6 000 triangles (subtree waves after one or two levels) and, for
    soup, sheet and spanning, at ~70 000 (the level-synchronous phase, several chunks per task, the
    recursive histogram scan)."""
    _check_builds(R, O, cases(name), render=True)


@pytest.mark.gpu
def test_zero_area_triangles(R, O, cases):
    """Soup with 5 % zero-area triangles (collinear, or two equal vertices): checks 1, 3 and 4 as
    everywhere; check 2 with NaN equal to NaN in the plane fields (n.x, n.y, n.z, D) only -- a
    zero-area triangle's plane is normalize(0) = NaN on both sides, and only the NaN's sign and payload
    may differ between the host's and the device's arithmetic."""
    c = cases("degenerate-6000")
    hr, dr = _check_builds(R, O, c, nan_planes=True)
    # only the zero-area triangles may have a NaN plane (rows are in scene order)
    p = c.scene.arrays()[0].astype(np.float64)
    area = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    assert (area == 0).sum() == 300
    nan_rows = np.isnan(hr.view(np.float32)[:, [3, 7, 11, 12]]).any(axis=1)
    assert not np.any(nan_rows & (area > 0))
    print("NaN plane words that differ between the builds:", int((hr != dr).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("ntri,gpu", [(65535, False), (65536, True)])
def test_default_path_at_the_threshold(R, O, cases, ntri, gpu):
    """c. BUILD_AUTO on both sides of RT_GPU_BUILD_MIN."""
    c = cases(f"soup-{ntri}")
    c.assert_conditions()
    ctx = _ctx(R, c.scene, R.BUILD_AUTO)
    try:
        assert ctx.build_info()["gpu"] is gpu
        _check_intersect(ctx, c, "auto")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_forced_gpu_build_declines_a_pile_and_the_process_goes_on(R, golden_dir, tmp_path):
    """d. 1 024 coincident triangles among 100 others, forced GPU mode: once the SAH has isolated the
    pile, its range is larger than kSmall and has no centroid extent on any axis, so k_split takes the
    !any_ext exit (ctr->error), gpu_build returns false and rt_create destroys the half-made context
    and returns RT_ERR_INVALID.

    What runs between k_split flagging the error and the host reading it, as read in rt_build.hip:
    the failed task's Split is {best_b -1, mid 0}.  k_part_count counts bin < -1, i.e. nothing, so
    nleft is 0 for its chunks.  k_part_scatter sends every element "right", to
    idx2[0 + (ch.begin - T.begin) + rank in chunk], an index in [0, T.end - T.begin), inside [0, ntri);
    those slots may also be written by the task that owns them, a race between two valid int stores
    into a buffer nothing reads afterwards.  k_copy_chunks copies idx2 back over [ch.begin, ch.end)
    only.  No index leaves [0, ntri); the build's buffers are freed by ~Bufs after the stream has been
    synchronised.  rt_destroy(c) of the partial context frees nothing but the stream-less, empty
    rt_ctx: every pointer member is still its nullptr initialiser and gpu_build hands its outputs over
    only on success."""
    scene = B.pile(100, 1024, tmp_path)
    R.set_build_mode(R.BUILD_GPU)
    try:
        with pytest.raises(R.RtError, match="degenerate large range"):
            R.Context(scene)
        # the next context of an ordinary scene, still in forced GPU mode, renders its golden image
        name, cfg, W, H, _, over = next(i for i in IMAGES if i[0] == "c2_64x48")
        z = np.load(f"{golden_dir}/images.npz")
        s, prm, _, _, _ = R.build_config(cfg)
        ctx = R.Context(s)
        try:
            assert ctx.build_info()["gpu"]
            img, st = ctx.render(R.camera_from_trackball(aspect=R.aspect_of(W, H)), apply(prm, over), W, H)
        finally:
            ctx.close()
        assert st.rays == int(z[f"{name}__rays"])
        assert float(np.max(np.abs(img - z[f"{name}__img"]))) <= TOL
    finally:
        R.set_build_mode(R.BUILD_AUTO)


@pytest.mark.gpu
def test_auto_build_falls_back_to_the_host_on_a_pile(R, O, cases):
    """d. The same pile among 65 536 other triangles under BUILD_AUTO: the GPU build declines
    (degenerate large range) and rt_create builds on the host; 512 rays, 64 of them aimed at the pile."""
    c = cases("pile-65536-1024")
    c.assert_conditions()
    ctx = _ctx(R, c.scene, R.BUILD_AUTO)
    try:
        assert ctx.build_info()["gpu"] is False
        _check_intersect(ctx, c, "auto")
    finally:
        ctx.close()
