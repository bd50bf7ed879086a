"""bench.py's plain run as its callers use it: one JSON line with the headline fields, exactly --steps timed steps, nothing of --full, and
--dump-outputs writing what the last timed step computed -- finite float32 / float64 arrays under 64 MB in all, the same bytes from run to run."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps=4, warmup=2):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line = _bench(a)
    assert line["steps"] == 4 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert not {"roofline", "roofline_stress", "cpu_baseline", "stage_ms"} & set(line), sorted(line)
    files = sorted(glob.glob(str(a / "*.npy")))
    names = {os.path.basename(f)[:-4] for f in files}
    assert {"pose", "vmap", "nmap", "vmap_valid", "nmap_valid", "tsdf_sample", "color_sample", "tsdf_plane_sums", "color_plane_sums"} <= names, names
    assert sum(os.path.getsize(f) for f in files) < 64 << 20
    arrays = {n: np.load(a / (n + ".npy")) for n in names}
    assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in arrays.values()), sorted(arrays)
    for m in ("vmap", "nmap"):   # pixels without a surface: 0 in the map, 0 in the mask; the rest carry the ray-cast surface
        valid = arrays[m + "_valid"]
        assert set(np.unique(valid)) <= {0.0, 1.0} and valid.sum() > 0
        assert not arrays[m].reshape(3, *valid.shape)[:, valid == 0].any()
    assert arrays["pose"].shape == (4, 4) and np.isfinite(arrays["pose"]).all()
    assert np.abs(arrays["tsdf_plane_sums"]).sum() > 0 and arrays["color_plane_sums"][:, 3].sum() > 0   # the volumes were fused into
    _bench(b)
    for n, x in arrays.items():
        y = np.load(b / (n + ".npy"))
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=True), n
