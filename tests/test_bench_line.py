"""The line bench.py prints for the driver: ONE short JSON line, the last of stdout (round 4's 24.9 KB line was not parsed).

CPU tier: compact_line() on full records of earlier runs (profiles/r0N_bench_default.json are what bench.py's `result` dict held)."""
import glob
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


RECORDS = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[4-9]_bench_default.json")) + glob.glob(os.path.join(ROOT, "profiles", "r0[5-9]_bench_full.json")))


@pytest.mark.parametrize("path", RECORDS, ids=[os.path.basename(p) for p in RECORDS])
def test_line_is_short_and_round_trips(path):
    b = _bench()
    full = json.load(open(path))
    line = b.compact_line(full)
    assert "\n" not in line
    assert len(line) < 8000 == b.LINE_LIMIT
    d = json.loads(line)
    # the contract's keys, unchanged in meaning
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["value"] == pytest.approx(full["value"], rel=1e-5)
    assert d["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    assert d["config"]["workload"] == full["config"]["workload"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in d["roofline"], k
    assert d["roofline"]["frac"] == pytest.approx(full["roofline"]["frac"], rel=1e-5)
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"], k
    assert d["parity"]["bit_identical"] is full["parity"]["bit_identical"]
    for name, leg in full.get("secondary", {}).items():
        assert d["secondary"][name]["value"] == pytest.approx(leg["value"], rel=1e-5)
        assert d["secondary"][name]["frac"] == pytest.approx(leg["roofline"]["frac"], rel=1e-5)


def test_line_sheds_keys_rather_than_grow():
    """Whatever the legs hold (long error strings, many legs), the line stays under the limit and keeps the headline."""
    b = _bench()
    full = json.load(open(RECORDS[-1]))
    full["secondary"] = {("leg%02d" % i): dict(v, config=dict(v["config"], workload="w" * 500)) for i in range(24) for v in [full["secondary"]["c3"]]}
    full["cpu_baseline"]["sample"] = "s" * 5000
    line = b.compact_line(full)
    assert len(line) < b.LINE_LIMIT
    d = json.loads(line)
    assert d["roofline"]["frac"] and d["cpu_baseline"]["value"] and d["value"]


def test_non_finite_numbers_do_not_break_the_line():
    b = _bench()
    full = json.load(open(RECORDS[-1]))
    full["roofline"]["frac_necessary"] = float("nan")
    full["secondary"]["c3"]["value"] = float("inf")
    d = json.loads(b.compact_line(full))          # strict JSON: NaN / Infinity would not load in other parsers
    assert "NaN" not in b.compact_line(full) and "Infinity" not in b.compact_line(full)
    assert d["secondary"]["c3"]["value"] is None


# what only --full adds to the result (measure / main); a plain run's result has none of it
FULL_ONLY = ("parity", "cpu_baseline", "roofline", "secondary", "tolerance_build", "frame_with_photon_pass_ms", "value_with_photon_pass")


def test_plain_line_is_the_headline_alone():
    """A plain run (no --full) times the headline only: its line has the contract's keys and the frame's description, and no
    block it did not measure (no roofline, cpu_baseline, parity, secondary legs, nor a pointer to a full record it did not write)."""
    b = _bench()
    full = json.load(open(RECORDS[-1]))
    plain = {k: v for k, v in full.items() if k not in FULL_ONLY}
    d = json.loads(b.compact_line(plain))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["value"] == pytest.approx(full["value"], rel=1e-5) and d["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    for k in FULL_ONLY + ("detail",):
        assert k not in d, k


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_the_last_frame(tmp_path, pkg):
    """bench.py without --full: exactly --steps timed steps, the lean line, and --dump-outputs writes the last timed step's frame - the
    frame the library renders for those inputs (Context.sample_image on the same camera and seed), bit for bit."""
    import subprocess
    import sys

    import numpy as np

    b = _bench()
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    d = json.loads(p.stdout.rstrip().splitlines()[-1])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["config"]["frame_finite"]
    for k in FULL_ONLY:
        assert k not in d, k
    assert sorted(os.listdir(out)) == ["radiance.npy"]
    frame = np.load(out / "radiance.npy")
    image_file, W, H, s, _ = b.WORKLOADS["c1"]
    assert frame.dtype == np.float64 and frame.shape == (H, W, 3)
    img = pkg.SceneImage(os.path.join(ROOT, "tests", "golden", image_file))
    cam = img.camera
    cam.width, cam.height, cam.sqrtspp = W, H, s
    ctx = pkg.Context(0)
    ctx.upload_image(img)
    want, _ = ctx.sample_image(cam, b.SEED, pkg.INTEGRATOR_PATH_TRACER)
    ctx.close()
    np.testing.assert_array_equal(frame, want)
    assert float(frame.mean()) == pytest.approx(d["config"]["frame_mean_radiance"], rel=1e-5)
