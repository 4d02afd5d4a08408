"""Scene generators for the GPU scene builder's tests (tests/test_gpu_build_shapes.py): adversarial
geometry (coplanar axis-aligned sheets, exact duplicates, extreme size ratios, spheres among the
triangles, piles of coincident triangles, zero-area triangles) at any triangle count, and ray sets
that reach it.

Every generator draws from numpy with a fixed seed, writes a small .obj / .mtl pair into the
directory the caller passes (pytest's tmp_path) and returns the loaded R.Scene with one point light.
Vertices are written with nine significant digits, which identify a float32 exactly.  The loader
restates Assimp's fast_atof (csrc/obj_loader.cpp), which is not correctly rounded: it may return a
neighbouring float for such text.  So the positions the loader produced (Scene.arrays()) are the
truth everywhere below -- the rays, the oracle and both builders see the same loaded scene -- and the
generators whose point is exact coincidence get it by construction instead: `sheet` uses dyadic
coordinates the parser reads exactly (asserted after the load), `dupes` and `pile` repeat `f` lines
over the same `v` lines.

The loader cannot produce -0.0: it applies the reference's identity node transform
((m0*x + m1*y) + (m2*z + m3*1), csrc/obj_loader.cpp m4_point), whose last term is +0, so a "-0.0"
in the text comes out as +0.0.  The zero-extent cases are therefore built from +0.0 only.

The scene a generator returns carries three attributes for its users: `view` = (look_at, distance)
of a camera that sees it, `dup_tris` = scene indices of triangles that have an exact duplicate,
`pile_tris` = scene indices of a pile's copies (empty arrays where there are none).
"""
import os

import numpy as np

import rt_amd as R

FLT_MAX = np.float32(np.finfo(np.float32).max)
_MTL = "newmtl shiny\nKd 0.6 0.5 0.4\nKs 0.5 0.5 0.5\nNs 20\nd 1\n"


def _txt(x):
    s = "%.9g" % float(x)
    if "e" in s:  # the parser's exponent path multiplies by powf(10, e): keep to positional text
        s = np.format_float_positional(np.float32(x), unique=True, trim="0")
    return s if ("." in s) else s + ".0"


def _write_obj(out_dir, name, verts, faces):
    """verts [n, 3] float32, faces: list of index tuples (0-based; 3 = triangle, 4 = quad)."""
    out_dir = str(out_dir)
    with open(os.path.join(out_dir, name + ".mtl"), "w") as f:
        f.write(_MTL)
    lines = [f"mtllib {name}.mtl", "o " + name, "usemtl shiny"]
    lines += ["v " + " ".join(_txt(c) for c in v) for v in np.asarray(verts, np.float32).tolist()]
    lines += ["f " + " ".join(str(i + 1) for i in fc) for fc in faces]
    path = os.path.join(out_dir, name + ".obj")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def scene_box(scene):
    """(lo, hi) of the scene's triangles and spheres, float64."""
    pos = scene.arrays()[0].reshape(-1, 3).astype(np.float64)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    d = scene.desc()
    for s in range(d.num_spheres):
        c = np.array(list(d.spheres[s].center), np.float64)
        lo, hi = np.minimum(lo, c - d.spheres[s].radius), np.maximum(hi, c + d.spheres[s].radius)
    return lo, hi


def _finish(path, ntri_expected, light=None, view=None, dup_tris=(), pile_tris=()):
    s = R.Scene()
    s.load_obj(path, normalize=False)
    assert s.desc().num_triangles == ntri_expected, (s.desc().num_triangles, ntri_expected)
    lo, hi = scene_box(s)
    c, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    s.add_point_light(tuple(c + np.array([-0.4, 0.9, -0.4]) * diag) if light is None else light, (1, 1, 1))
    s.view = (tuple(c), 1.2 * diag) if view is None else view
    s.dup_tris = np.asarray(dup_tris, np.int64)
    s.pile_tris = np.asarray(pile_tris, np.int64)
    return s


def _soup_verts(rng, ntri, lo=-1.0, hi=1.0, size=None):
    """ntri small triangles inside [lo, hi]^3: [ntri, 3, 3] float32.  The edge length follows the
    spacing of ntri points in the cube, so that a ray through the cube meets a few of them."""
    half = (hi - lo) / 2
    if size is None:
        size = 0.9 * half / max(2.0, ntri ** (1.0 / 3.0))
    cen = rng.uniform(lo + size, hi - size, size=(ntri, 1, 3))
    return (cen + rng.uniform(-size, size, size=(ntri, 3, 3))).astype(np.float32)


def _tri_faces(n, first=0):
    return [(first + 3 * i, first + 3 * i + 1, first + 3 * i + 2) for i in range(n)]


def soup(ntri, out_dir, seed=1, degenerate=0.0):
    """Small random triangles, uniform in [-1, 1]^3.  `degenerate` > 0 makes that fraction of them
    zero-area: alternately collinear (all three vertices on one line parallel to x, so that no
    rounding lifts one off it) and with two equal vertices."""
    rng = np.random.default_rng(seed)
    v = _soup_verts(rng, ntri)
    if degenerate > 0.0:
        bad = rng.choice(ntri, size=max(2, int(round(ntri * degenerate))), replace=False)
        for j, t in enumerate(bad):
            if j % 2 == 0:  # collinear along x: y and z of all three equal
                v[t, 1, 1:] = v[t, 0, 1:]
                v[t, 2, 1:] = v[t, 0, 1:]
            else:  # two equal vertices
                v[t, 2] = v[t, 1]
    path = _write_obj(out_dir, f"soup{ntri}", v.reshape(-1, 3), _tri_faces(ntri))
    return _finish(path, ntri)


def sheet(ntri, out_dir):
    """A regular grid of right triangles in the plane z = 0 exactly (the last row is ragged where
    ntri does not fill it).  Grid coordinates are multiples of
    2^-7 around 0, which the loader's parser reads exactly (asserted), so whole rows share a centroid
    y and whole columns a centroid x, bit for bit, and every box has zero z extent."""
    ncell = (ntri + 1) // 2
    nx = max(1, int(np.ceil(np.sqrt(ncell))))
    ny = (ncell + nx - 1) // nx
    step = 2.0 ** -7
    xs = (np.arange(nx + 1) - nx // 2) * step
    ys = (np.arange(ny + 1) - ny // 2) * step
    verts = np.array([(x, y, 0.0) for y in ys for x in xs], np.float32)
    vid = lambda i, j: j * (nx + 1) + i  # noqa: E731
    faces = []
    for c in range(ncell):
        i, j = c % nx, c // nx
        faces.append((vid(i, j), vid(i + 1, j), vid(i, j + 1)))
        faces.append((vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)))
    faces = faces[:ntri]
    path = _write_obj(out_dir, f"sheet{ntri}", verts, faces)
    s = _finish(path, ntri, view=((0.0, 0.0, 0.0), 1.6 * step * max(nx, ny)))
    want = verts[np.array(faces)].astype(np.float32)
    assert s.arrays()[0].tobytes() == want.tobytes(), "the loader did not read the dyadic grid exactly"
    return s


def dupes(ntri, k, out_dir, seed=2):
    """ntri // k soup triangles, each listed k times (consecutive `f` lines over the same vertices):
    exact duplicates tie in t, in every sort attribute and in every centroid."""
    rng = np.random.default_rng(seed)
    base = ntri // k
    v = _soup_verts(rng, base)
    faces = [f for f in _tri_faces(base) for _ in range(k)]
    path = _write_obj(out_dir, f"dupes{ntri}x{k}", v.reshape(-1, 3), faces)
    return _finish(path, base * k, dup_tris=np.arange(base * k))


def spanning(ntri, out_dir, seed=3):
    """Two clusters of tiny soup ([-0.01, 0.01]^3 around (-100, 0, 0) and (100, 0, 0)), one triangle
    that spans both, and one ground quad (two triangles) under everything: ntri triangles in all."""
    rng = np.random.default_rng(seed)
    n = ntri - 3
    na = n // 2
    a = _soup_verts(rng, na, -0.01, 0.01).astype(np.float64) + np.array([-100.0, 0.0, 0.0])
    b = _soup_verts(rng, n - na, -0.01, 0.01).astype(np.float64) + np.array([100.0, 0.0, 0.0])
    v = np.concatenate([a, b]).astype(np.float32).reshape(-1, 3)
    big = np.array([(-100.5, -0.02, 0.3), (100.5, -0.02, 0.3), (0.0, 40.0, -0.3)], np.float32)
    quad = np.array([(-120.0, -0.5, -60.0), (-120.0, -0.5, 60.0), (120.0, -0.5, 60.0), (120.0, -0.5, -60.0)],
                    np.float32)
    verts = np.concatenate([v, big, quad])
    faces = _tri_faces(n) + [(3 * n, 3 * n + 1, 3 * n + 2), (3 * n + 3, 3 * n + 4, 3 * n + 5, 3 * n + 6)]
    path = _write_obj(out_dir, f"spanning{ntri}", verts, faces)
    # a camera at one cluster: the tiny triangles in front, the spanning triangle and the ground behind
    return _finish(path, ntri, light=(-99.0, 3.0, 2.0), view=((-100.0, 0.0, 0.0), 0.06))


def with_spheres(ntri, nsph, out_dir, seed=4):
    """Soup plus nsph spheres.  min(nsph, 12) of the centres are centroids of triangles as the
    reference BVH computes them ((a + b + c) / 3 per axis, float32), so on whichever axis a level
    sorts by, those spheres tie with a triangle and only the stable order separates them.  From 18
    spheres on, six more come as three pairs whose centres differ only in the sign of a zero, (+0.0
    first, then -0.0) on y, z and x in turn: the reference's sort of (attribute, position) pairs holds
    the two equal and keeps them in listed order, a sort by the float's bits would not (spheres, unlike
    loaded triangles, can carry -0.0).  The rest are uniform in the cube."""
    rng = np.random.default_rng(seed)
    v = _soup_verts(rng, ntri)
    path = _write_obj(out_dir, f"spheres{ntri}_{nsph}", v.reshape(-1, 3), _tri_faces(ntri))
    s = _finish(path, ntri)
    pos = s.arrays()[0]
    cen = ((pos[:, 0] + pos[:, 1]) + pos[:, 2]) / np.float32(3)  # RefBuild's tkey, float32 ops
    assert cen.dtype == np.float32
    tied = rng.choice(ntri, size=min(nsph, 12, ntri), replace=False)
    centres = [cen[t] for t in tied]
    if nsph >= 18:
        for axis in (1, 2, 0):
            c = rng.uniform(-0.5, 0.5, 3).astype(np.float32)
            for zero in (0.0, -0.0):
                c = c.copy()
                c[axis] = zero
                centres.append(c)
    size = 0.9 / max(2.0, ntri ** (1.0 / 3.0))
    mat = R.material((0.3, 0.5, 0.7), (0.4, 0.4, 0.4), 10.0, 1.0)
    for i in range(nsph):
        c = centres[i] if i < len(centres) else rng.uniform(-0.9, 0.9, 3).astype(np.float32)
        s.add_sphere(tuple(float(x) for x in c), float(rng.uniform(1.0, 2.5) * size), mat)
    return s


def pile(n_soup, n_pile, out_dir, seed=5):
    """Soup plus one triangle listed n_pile times: n_pile coincident centroids, which no split plane
    separates."""
    rng = np.random.default_rng(seed)
    v = _soup_verts(rng, n_soup + 1)
    faces = _tri_faces(n_soup) + [(3 * n_soup, 3 * n_soup + 1, 3 * n_soup + 2)] * n_pile
    path = _write_obj(out_dir, f"pile{n_soup}_{n_pile}", v.reshape(-1, 3), faces)
    p = np.arange(n_soup, n_soup + n_pile)
    return _finish(path, n_soup + n_pile, dup_tris=p, pile_tris=p)


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def rays_at(scene, n, seed, n_pile=0):
    """n rays (R.RAY_DTYPE, t = FLT_MAX): half from origins on a sphere around the scene's box, aimed
    at jittered triangle centroids (a random point well inside the triangle; where the scene has
    spheres a quarter of these rays aim inside a sphere instead, and the first n_pile of them at the
    scene's pile); a quarter uniformly random through an enlarged box; a quarter axis-parallel, two
    direction components exactly 0, through the box's cross-section enlarged by a fifth
    (so that some of them miss).  Directions are unit length except where float32 rounding says
    otherwise."""
    rng = np.random.default_rng(seed)
    pos = scene.arrays()[0].astype(np.float64)
    d = scene.desc()
    lo, hi = scene_box(scene)
    c, ext = (lo + hi) / 2, hi - lo
    diag = float(np.linalg.norm(ext))
    n_aim, n_rand = n // 2, n // 4
    n_axis = n - n_aim - n_rand
    org, dirs = np.zeros((n, 3)), np.zeros((n, 3))
    # aimed
    tri = rng.integers(0, len(pos), size=n_aim)
    if n_pile:
        tri[:n_pile] = rng.choice(scene.pile_tris, size=n_pile)
    w = rng.uniform(0.15, 1.0, size=(n_aim, 3))
    w /= w.sum(axis=1, keepdims=True)
    tgt = np.einsum("nk,nkc->nc", w, pos[tri])
    if d.num_spheres:
        ns = n_aim // 4
        sph = rng.integers(0, d.num_spheres, size=ns)
        sc = np.array([list(d.spheres[int(i)].center) for i in sph], np.float64)
        sr = np.array([d.spheres[int(i)].radius for i in sph], np.float64)
        tgt[n_aim - ns:] = sc + _unit(rng, ns) * (0.5 * sr * rng.uniform(0, 1, ns))[:, None]
    org[:n_aim] = c + _unit(rng, n_aim) * (0.75 * diag)
    dirs[:n_aim] = tgt - org[:n_aim]
    dirs[:n_aim] /= np.linalg.norm(dirs[:n_aim], axis=1, keepdims=True)
    # uniformly random
    a, b = n_aim, n_aim + n_rand
    org[a:b] = c + rng.uniform(-0.75, 0.75, size=(n_rand, 3)) * (ext + 0.1 * diag)
    dirs[a:b] = _unit(rng, n_rand)
    # axis-parallel
    ax = rng.integers(0, 3, size=n_axis)
    sign = rng.choice([-1.0, 1.0], size=n_axis)
    p = c + rng.uniform(-0.6, 0.6, size=(n_axis, 3)) * ext
    k = np.arange(n_axis)
    p[k, ax] = c[ax] - sign * (0.5 * ext[ax] + 0.25 * diag)
    org[b:] = p
    dirs[b:][k, ax] = sign
    rays = np.zeros(n, R.RAY_DTYPE)
    rays["origin"] = org.astype(np.float32)
    rays["direction"] = dirs.astype(np.float32)
    rays["t"] = FLT_MAX
    assert np.all(np.count_nonzero(rays["direction"][b:], axis=1) == 1)
    return rays


def axis_parallel(rays):
    """Mask of the rays with two direction components exactly 0."""
    return np.count_nonzero(rays["direction"], axis=1) == 1
