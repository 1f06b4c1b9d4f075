"""bench.py's plain run and --dump-outputs: a plain run prints the headline line only (what --full adds stays
null), and DIR/rgba.npy, DIR/accum.npy hold the last timed step's frame and accumulation -- float32, the same
in every run, equal to a direct render of the same frames bit for bit.  A frame beyond the size limit is
written as a fixed sample of its rows (CPU test)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 96, 70, 8


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_samples_rows_within_the_limit(tmp_path, monkeypatch):
    bench = _bench()
    rng = np.random.default_rng(7)
    h, w = 37, 13
    rgba = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32)
    acc = rng.random((h, w, 4), dtype=np.float32)
    # whole: both arrays fit
    bench.dump_outputs(str(tmp_path / "a"), rgba, acc)
    rows = np.load(tmp_path / "a" / "rows.npy")
    out = np.load(tmp_path / "a" / "rgba.npy")
    assert np.array_equal(rows, np.arange(h)) and out.dtype == np.float32 and out.shape == (h, w, 4)
    assert np.array_equal(out.astype(np.uint8).reshape(h, w * 4).view(np.uint32), rgba)
    assert np.array_equal(np.load(tmp_path / "a" / "accum.npy"), acc)
    # a limit that holds 10 rows of the two arrays: the same 10 rows in both files and in every run
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 10 * w * 16 + 5)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), rgba, acc)
    rows = np.load(tmp_path / "b" / "rows.npy").astype(np.int64)
    assert len(rows) == 10 and len(set(rows)) == 10 and np.all(np.diff(rows) > 0) and rows.max() < h
    assert np.array_equal(np.load(tmp_path / "b" / "accum.npy"), acc[rows])
    assert np.array_equal(np.load(tmp_path / "b" / "rgba.npy").astype(np.uint8).reshape(10, w * 4).view(np.uint32), rgba[rows])
    size = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert size <= bench.DUMP_BYTES + 8 * len(rows) + 3 * 128   # the limit is the two arrays'; + the row list, three .npy headers
    for f in ("rows.npy", "rgba.npy", "accum.npy"):
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f))
    # without an accumulation (N > 1) the frame alone takes the limit
    bench.dump_outputs(str(tmp_path / "e"), rgba, None)
    assert len(np.load(tmp_path / "e" / "rows.npy")) == 20 and not os.path.exists(tmp_path / "e" / "accum.npy")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    from _rt import rt
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--width", str(W),
           "--height", str(H), "--spp", str(SPP), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32+f64"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0
    assert abs(line["ms_per_step"] - 1e3 * line["rank_elapsed_s"][0] / 3) <= 0.01   # both rounded
    assert abs(line["value"] - W * H * SPP * 3 / line["rank_elapsed_s"][0] / 1e6) <= 1e-2 * line["value"]
    for k in ("roofline", "parity", "fast_mode", "cpu_baseline", "configs"):   # --full's
        assert line[k] is None, k
    c = rt.Context(0)
    try:
        c.upload(rt.Scene.cornell())
        c.resize(W, H)
        cam, _, _ = rt.camera_default(W, H)
        rgba, acc = c.render(cam, SPP, seed=0)
    finally:
        c.close()
    assert sorted(os.listdir(out)) == ["accum.npy", "rgba.npy", "rows.npy"]
    got_rgba, got_acc = np.load(out / "rgba.npy"), np.load(out / "accum.npy")
    assert got_rgba.dtype == np.float32 and got_acc.dtype == np.float32
    assert np.array_equal(np.load(out / "rows.npy"), np.arange(H))
    assert np.array_equal(got_rgba.astype(np.uint8).reshape(H, W * 4).view(np.uint32), rgba)
    assert np.array_equal(got_acc.view(np.uint32), acc.view(np.uint32))
