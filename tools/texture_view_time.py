"""Time of the texture-debug view (rt_render_texture_views, rt::texture_view_kernel) against the nearest thing
the render kernels can do: rt_render_views of the same scene with its lights cleared and
max_reflection_level = 0, camera rays only.  C3 (the 800 000-triangle dragon proxy) at 1920x1080, one view
and a 64-view turntable batch.

    python tools/texture_view_time.py [--out profiles/texture_view/time.json] [--views 1,64]

Each leg runs in a process of its own, one after the other (one GPU process at a time), each under its own
time limit; a leg that fails or runs out of time ends the run.  Per shape a leg warms up, then reports the
median (and min / max) of stats.kernel_ms -- device events around the launch -- over its repeats, and the kernel
the stats name.  The target is view <= parent per frame in both shapes."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracer-group27_amd"))

W, H = 1920, 1080
LEG_TIMEOUT_S = 420


def leg(name, views, uv):
    import numpy as np
    import rt_amd as R

    scene, prm, _, _, desc = R.build_config("C3", dragon_uv=uv)
    prm.max_reflection_level = 0
    if name == "parent":
        scene.clear_lights()
    ctx = R.Context(scene)
    out = {"leg": name, "scene": desc, "width": W, "height": H, "shapes": []}
    for n in views:
        cams = R.turntable_cameras(n, R.aspect_of(W, H))
        call = (lambda: ctx.render_texture_views(cams, prm, W, H)) if name == "view" else \
            (lambda: ctx.render_views(cams, prm, W, H))
        warm, reps = (3, 20) if n == 1 else (2, 7)
        for _ in range(warm):
            call()
        ms, kernel, rays = [], "", 0
        for _ in range(reps):
            _, st = call()
            ms.append(float(st.kernel_ms))
            kernel, rays = st.kernel_name, int(st.rays)
        out["shapes"].append({"views": n, "kernel": kernel, "rays": rays, "repeats": reps,
                              "kernel_ms_median": float(np.median(ms)), "kernel_ms_min": min(ms),
                              "kernel_ms_max": max(ms), "ms_per_frame": float(np.median(ms)) / n})
    ctx.close()
    print("LEG " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["view", "parent"])
    ap.add_argument("--views", default="1,64")
    ap.add_argument("--dragon-uv", default="", help="U,V of the dragon proxy (default: the 800 000-triangle one)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "texture_view", "time.json"))
    a = ap.parse_args()
    views = [int(v) for v in a.views.split(",")]
    uv = tuple(int(v) for v in a.dragon_uv.split(",")) if a.dragon_uv else None
    if a.leg:
        return leg(a.leg, views, uv)
    legs = {}
    for name in ("parent", "view"):  # a fresh child process per leg; the parent holds no GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--views", a.views]
        if a.dragon_uv:
            cmd += ["--dragon-uv", a.dragon_uv]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT_S)
        lines = [l for l in r.stdout.splitlines() if l.startswith("LEG ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"leg {name} failed ({r.returncode}); nothing more is started")
        legs[name] = json.loads(lines[-1][4:])
    result = {"legs": legs, "verdict": []}
    for pv, vv in zip(legs["parent"]["shapes"], legs["view"]["shapes"]):
        result["verdict"].append({"views": vv["views"], "view_ms_per_frame": vv["ms_per_frame"],
                                  "parent_ms_per_frame": pv["ms_per_frame"],
                                  "no_slower": vv["ms_per_frame"] <= pv["ms_per_frame"]})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["verdict"]))


if __name__ == "__main__":
    main()
