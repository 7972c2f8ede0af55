"""bench.py's plain run on the GPU box: one JSON line with the headline only, exactly --steps timed steps, and with
--dump-outputs the last timed frame -- the golden image -- written as float32."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_reports_the_headline_and_dumps_the_last_frame(golden, tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--workload",
           "bunny_600_defaults", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    # what moved behind --full stays out of a plain run
    for key in ("pipelined", "blocks", "roofline", "cpu_baseline", "end_to_end"):
        assert key not in line, key
    c = golden["renders"]["bunny_600_defaults"]
    assert line["config"]["pgm_md5"] == c["pgm_md5"]
    image = np.load(out_dir / "image_u8.npy")
    assert image.dtype == np.float32 and image.shape == (c["height"], c["width"])
    u8 = image.astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), image)
    pgm = f"P5 {c['width']} {c['height']} 255\n".encode() + u8.tobytes()
    assert hashlib.md5(pgm).hexdigest() == c["pgm_md5"]
