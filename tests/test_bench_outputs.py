"""bench.py's plain and --full runs and --dump-outputs.

CPU: the checks that take renders of their own are refused without --full;
dump_outputs writes a small canvas whole and a canvas above its byte budget
as a fixed, seeded pixel sample, finite numbers only, the non-finite sums
listed in a file of their own; without a timed step there is nothing to
write.  GPU: a plain run on a small frame prints the headline keys, leaves the --full figures null, and writes the canvas of
its last timed step: the device's own render of that frame, bit for bit."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

from _util import same_bits_or_both_nan  # noqa: E402


def test_dump_outputs_needs_a_timed_step(tmp_path):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "0", "--dump-outputs", str(tmp_path / "o")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr and not r.stdout.strip()
    assert not (tmp_path / "o").exists()


@pytest.mark.parametrize("extra", [["--check"], ["--scaling-anchors", "on"]])
def test_own_renders_need_full(extra):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", *extra], cwd=ROOT, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2
    assert "--full" in r.stderr and not r.stdout.strip()


def test_dump_outputs_whole_and_sampled(tmp_path):
    import torch

    small = torch.arange(6 * 4, dtype=torch.float32).reshape(6, 4)
    small[1, 0], small[2, 1], small[4, 2], small[4, 3] = float("nan"), float("inf"), float("-inf"), float("nan")
    assert bench.dump_outputs(str(tmp_path / "a"), small) == {"canvas": [6, 4], "canvas_nonfinite": [4, 2]}
    got, code = np.load(tmp_path / "a" / "canvas.npy"), np.load(tmp_path / "a" / "canvas_nonfinite.npy")
    assert got.dtype == np.float32 and code.dtype == np.float64 and np.isfinite(got).all()
    assert np.array_equal(code, [[4, 1], [9, 2], [18, 3], [19, 1]])  # flat index in canvas.npy, code
    want_code = np.zeros((6, 4), np.float32)
    want_code[1, 0], want_code[2, 1], want_code[4, 2], want_code[4, 3] = 1, 2, 3, 1
    fin = want_code == 0
    assert np.array_equal(got[fin], small.numpy()[fin]) and (got[~fin] == 0).all()
    assert bool(torch.isnan(small[1, 0]))  # the caller's tensor is left as it was
    assert sorted(os.listdir(tmp_path / "a")) == ["canvas.npy", "canvas_nonfinite.npy"]

    n = bench.DUMP_MAX_BYTES // 32 + 1000  # just over the whole canvas's half of the budget
    big = torch.arange(n, dtype=torch.float32)[:, None] * torch.tensor([1.0, 2.0, 3.0, 0.0])
    for d in ("b", "c"):  # twice: the sample is fixed
        bench.dump_outputs(str(tmp_path / d), big)
    got, pix = np.load(tmp_path / "b" / "canvas.npy"), np.load(tmp_path / "b" / "canvas_pixels.npy")
    code = np.load(tmp_path / "b" / "canvas_nonfinite.npy")
    assert got.dtype == np.float32 and pix.dtype == np.float64 and code.shape == (0, 2) and code.dtype == np.float64
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= bench.DUMP_MAX_BYTES
    ids = pix.astype(np.int64)
    assert len(ids) == len(got) > n // 2 and (np.diff(ids) > 0).all() and 0 <= ids[0] and ids[-1] < n
    assert np.array_equal(got, big.numpy()[ids])
    for f in ("canvas.npy", "canvas_pixels.npy", "canvas_nonfinite.npy"):
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_frame(device, tmp_path):
    import raytracingtherestofyourlife_amd as rtp

    nx, ny, spp, depth = 72, 40, 8, 10
    out = tmp_path / "out"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--nx", str(nx), "--ny", str(ny),
           "--spp", str(spp), "--depth", str(depth), "--ff-tables", "off", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["metric"] == bench.METRIC and line["unit"] == "Msamples/s" and line["higher_is_better"] is True
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0
    # (both figures are rounded to three decimals; a step of this frame takes well under a millisecond)
    assert line["value"] == pytest.approx(nx * ny * spp / line["ms_per_step"] / 1e3, rel=5e-2)
    for k in ("rmse", "bit_exact", "quality", "first_render_ms", "one_shot", "roofline", "roofline_valu",
              "cpu_baseline", "cpu_baseline_all_cores"):
        assert line[k] is None, k
    assert "scaling_anchors" not in line
    got, code = np.load(out / "canvas.npy"), np.load(out / "canvas_nonfinite.npy")
    assert line["outputs"]["arrays"] == {"canvas": [nx * ny, 4], "canvas_nonfinite": [len(code), 2]}
    assert got.dtype == np.float32 and got.shape == (nx * ny, 4) and np.isfinite(got).all()
    assert sorted(os.listdir(out)) == ["canvas.npy", "canvas_nonfinite.npy"]
    device.set_cornell_box(0)
    want, _, _, _ = device.render_pixels(rtp.default_camera(), nx, ny, spp, depth, np.arange(nx * ny, dtype=np.int64))
    marks = np.zeros(nx * ny * 4)
    marks[code[:, 0].astype(np.int64)] = code[:, 1]
    marks = marks.reshape(nx * ny, 4)
    bad = ~np.isfinite(want[:, :3])
    assert np.array_equal(marks[:, :3] != 0, bad) and (marks[:, :3][np.isnan(want[:, :3])] == 1).all()
    assert (got[:, :3][bad] == 0).all()
    assert same_bits_or_both_nan(got[:, :3][~bad], want[:, :3][~bad]).all()
