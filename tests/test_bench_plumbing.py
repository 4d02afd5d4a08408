"""bench.py's roofline plumbing on the CPU: the PMC summary is used only for the exact config, kernel and
library build it was measured on, and the committed summary is keyed the way bench.py looks it up; --dump-outputs
writes a step whole or at a fixed sample.  On the GPU: one small plain run, its line and its dump."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_pmc_summary_matched_on_config_kernel_and_library(tmp_path):
    b = bench()
    k = "rt::persistent_df_kernel<false, false, 23>"
    d = {"config": b.pmc_key("C3", 64), "kernel": f"void {k}(rt::KParams, rt::JobSrc)", "lib_sha": "abc",
         "hbm_bytes_per_launch": 123.0, "note": "n"}
    p = tmp_path / "pmc.json"
    p.write_text(json.dumps(d))
    assert b.load_pmc("C3v64", k, "abc", str(p))[0] == 123.0
    assert b.load_pmc("C3v16", k, "abc", str(p))[0] is None  # another batch size
    assert b.load_pmc("C3v64", "rt::persistent_df_kernel<false, false, 0>", "abc", str(p))[0] is None
    assert b.load_pmc("C3v64", k, "def", str(p))[0] is None  # another library build
    assert b.load_pmc("C3v64", k, "abc", str(tmp_path / "missing.json"))[0] is None


def test_dump_outputs_whole_step_or_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: a step within the budget is written whole, a larger one at the documented sample of its
    pixels -- the same pixels on every run -- as float32, with the ray count as float64."""
    b = bench()
    px = np.arange(50 * 3, dtype=np.float32).reshape(50, 3)
    b.dump_outputs(str(tmp_path / "whole"), px, 1234567890123)
    got = np.load(tmp_path / "whole" / "images.npy")
    assert got.dtype == np.float32 and got.tobytes() == px.tobytes()
    rays = np.load(tmp_path / "whole" / "rays.npy")
    assert rays.dtype == np.float64 and rays.tolist() == [1234567890123.0]
    monkeypatch.setattr(b, "DUMP_PIXELS", 16)
    idx = np.sort(np.random.default_rng(b.DUMP_SEED).integers(0, 50, 16))
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), px, 7)
        got = np.load(tmp_path / d / "images.npy")
        assert got.dtype == np.float32 and got.tobytes() == px[idx].tobytes()
    assert 3 * 4 * bench().DUMP_PIXELS + 8 <= 64 * 10**6  # the dump's size limit


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(R, tmp_path):
    """A plain bench.py run (one GPU, a small C3): --steps sets the timed steps, the line carries ms_per_step and
    none of the --full records, and --dump-outputs holds the step's images and ray count as the library renders
    them in-process."""
    W, H, F = 160, 90, 3
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--views",
           str(F), "--config", "C3", "--dragon-uv", "200x80", "--resolution", f"{W}x{H}", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "Mrays/s" and line["value"] > 0
    assert not {"roofline", "cpu_baseline", "single_frame"} & set(line)
    scene, prm, _, _, _ = R.build_config("C3", dragon_uv=(200, 80))
    ctx = R.Context(scene)
    try:
        ref, st = ctx.render_views(R.turntable_cameras(F, R.aspect_of(W, H)), prm, W, H)
    finally:
        ctx.close()
    got = np.load(out / "images.npy")
    assert got.dtype == np.float32 and got.shape == (F * W * H, 3)
    assert got.tobytes() == ref.tobytes()
    assert np.load(out / "rays.npy").tolist() == [float(st.rays)]
    assert line["config"]["rays_per_frame"] == st.rays // F


def test_committed_summary_is_keyed_for_the_default_bench():
    b = bench()
    d = json.load(open(os.path.join(REPO, "profiles", "pmc_latest.json")))
    assert d["config"] == b.pmc_key("C3", b.DEFAULT_VIEWS)
    # the bench's render kernel (the opaque-scene kernel for C3 since round 3), its plain (non-counting) build
    assert any(k in d["kernel"] for k in ("persistent_opaque_kernel<false", "persistent_df_kernel<false"))
    assert d["hbm_bytes_per_launch"] > 0
